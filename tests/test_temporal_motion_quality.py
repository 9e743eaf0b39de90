"""Does following the moving mesh help?  tests/temporal_motion_quality.py's four frames (the CPU oracle's samples, the torus moving about
two pixels per frame under a camera at rest) through the numpy references, against the oracle's 1024-spp picture of the last pose.  The
figures are those of profiles/motion/quality.json, which the sweep wrote; the bound r is recorded there."""
import pytest

import temporal_motion_quality as Q


@pytest.fixture(scope="module")
def fig(art):
    frames = [Q.cpu_frame(art, k)[:3] for k in range(Q.FRAMES)]
    return Q.figures(frames, Q.reference(), art.TEMPORAL_MAX_HISTORY, art.TEMPORAL_DEPTH_TOL, art.TEMPORAL_NORMAL_MIN)


def check(fig, rec):
    """the assertions the CPU test and the GPU test share"""
    print("mesh pixels %d: RMS %.4f last frame alone, %.4f camera only, %.4f with motion; elsewhere %.4f, %.4f, %.4f; lengths %s against %s; restarted %.3f"
          % (fig["mesh_pixels"], fig["mesh"]["before"], fig["mesh"]["camera_only"], fig["mesh"]["after"], fig["rest"]["before"], fig["rest"]["camera_only"],
             fig["rest"]["after"], fig["mean_length_mesh_motion"], fig["mean_length_mesh_camera_only"], fig["restarted_share_mesh_frame2"]))
    assert rec["ratio"] < 0.8 and abs(rec["bound"] - 0.5 * (1.0 + rec["ratio"])) < 1e-12       # r: halfway between the references' ratio and 1
    assert fig["mesh_pixels"] > 50
    assert fig["mesh"]["after"] < rec["bound"] * fig["mesh"]["before"]
    assert fig["rest"]["after"] <= fig["rest"]["camera_only"] and fig["rest"]["after"] < fig["rest"]["before"]      # motion is 0 there: no worse
    for k in range(1, Q.FRAMES):
        assert fig["mean_length_mesh_motion"][k] > fig["mean_length_mesh_camera_only"][k], k
    assert fig["restarted_share_mesh_frame2"] <= 0.25


def test_following_the_mesh_helps(fig):
    check(fig, Q.record())


def test_the_record_holds_these_figures(fig):
    rec = Q.record()
    for part in ("mesh", "rest"):
        for name, v in fig[part].items():
            assert abs(v - rec[part][name]) <= 1e-9 * max(1.0, abs(v)), (part, name)
    assert fig["mean_length_mesh_motion"] == rec["mean_length_mesh_motion"] and fig["restarted_share_mesh_frame2"] == rec["restarted_share_mesh_frame2"]
