"""The three rebuild counts (art_get_rebuild_info, art_get_instance_rebuild_info, art_get_mesh_rebuild_info) are kept by one piece of
code: each call counts into its own record and into no other, a refused call counts nowhere, and art_upload_scene clears all three."""
import numpy as np
import pytest

import test_gpu_refit as T
import test_gpu_two_level_reference as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def counts(backend):
    """(flat, instance tree, mesh tree) rebuilds"""
    return backend.rebuild_info().rebuilds, backend.instance_rebuild_info().rebuilds, backend.mesh_rebuild_info().rebuilds


def counted(ri):
    return ri.host_ms >= ri.build_ms > 0.0


def zero(ri):
    return (ri.rebuilds, ri.gather_ms, ri.build_ms, ri.host_ms) == (0, 0.0, 0.0, 0.0)


def test_each_rebuild_counts_into_its_own_record_only(art, backend):
    backend.upload_scene(R.placed(0, 12))                                 # the smallest scene of the mesh tests: 12 instances of two meshes
    assert counts(backend) == (0, 0, 0)
    backend.rebuild_mesh(0)
    assert counts(backend) == (0, 0, 1)
    backend.rebuild_instances()
    assert counts(backend) == (0, 1, 1)
    assert counted(backend.instance_rebuild_info()) and counted(backend.mesh_rebuild_info())
    before = [(ri.rebuilds, ri.gather_ms, ri.build_ms, ri.host_ms) for ri in (backend.rebuild_info(), backend.instance_rebuild_info(), backend.mesh_rebuild_info())]
    with pytest.raises(art.ArtError, match="out of range"):
        backend.rebuild_mesh(2)
    after = [(ri.rebuilds, ri.gather_ms, ri.build_ms, ri.host_ms) for ri in (backend.rebuild_info(), backend.instance_rebuild_info(), backend.mesh_rebuild_info())]
    assert after == before                                                # a refused call moves no figure
    backend.upload_scene(R.placed(0, 12))
    assert zero(backend.rebuild_info()) and zero(backend.instance_rebuild_info()) and zero(backend.mesh_rebuild_info())


def test_a_flat_rebuild_counts_into_rebuild_info_only(art, backend):
    from ada_ray_tracer_amd import scenes
    sd = scenes.synthetic_scene(500, 3)
    pos, nrm, _, _ = T._mesh(sd)
    backend.upload_scene(sd)
    assert counts(backend) == (0, 0, 0)
    pg, ng = T._gpu(np.asarray(pos, np.float32), np.asarray(nrm, np.float32))
    backend.rebuild_torch(pg, ng)
    assert counts(backend) == (1, 0, 0)
    assert counted(backend.rebuild_info())
    assert zero(backend.instance_rebuild_info()) and zero(backend.mesh_rebuild_info())
