"""Reference of art_adaptive_estimate_device and of art_compact_mask_device, written from the header comment of include/art_hip.h: numpy
binary64 in the order the header states, each stored float rounded once to binary32; the mean alone is binary32.  Also the planted planes
the host test (tests/test_adaptive_reference_host.py) and the GPU test (tests/test_gpu_adaptive.py) share, and the plain CPU loop of
Backend.render_adaptive over the oracle's own samples (the quality sweep of profiles/adaptive/quality.py)."""
import numpy as np

F = np.float32
D = np.float64
INF = F(np.inf)


def estimate(accum, moments, counts, aa_on, min_colours, max_samples, threshold, lum_floor):
    """accum [..., 3] float32, moments [..., 2] float32, counts [...] uint32 -> (mean [..., 3] f32, variance f32, error f32, mask uint8)"""
    accum = np.asarray(accum, F); moments = np.asarray(moments, F); counts = np.asarray(counts, np.uint32)
    with np.errstate(all="ignore"):
        per = 4 if aa_on else 1
        s = counts
        n = s.astype(D) / D(per)
        k = D(1.0) / D(per)
        r = F(1.0) / s.astype(F)                                    # (s = 0: replaced below)
        mean = np.where((s == 0)[..., None], F(0.0), r[..., None] * accum).astype(F)
        S1 = moments[..., 0].astype(D); S2 = moments[..., 1].astype(D)
        Dv = S2 - (S1 * S1) / n
        D0 = np.where(Dv < 0.0, D(0.0), Dv)                         # a NaN fails the comparison and stays
        v = (D0 * (n / (n - D(1.0)))) / n
        m = (S1 / n) * k
        var = (v * (k * k)).astype(F)
        err = ((np.sqrt(v) * k) / (np.abs(m) + D(F(lum_floor)))).astype(F)
        var = np.where(np.isnan(var), np.uint32(0x7fc00000).view(F), var).astype(F)      # a NaN is stored as THE quiet NaN
        err = np.where(np.isnan(err), np.uint32(0x7fc00000).view(F), err).astype(F)
        few = (s == 0) | (n < 2.0)
        var = np.where(few, INF, var).astype(F)
        err = np.where(few, INF, err).astype(F)
        mask = (s < np.uint32(max_samples)) & ((n < D(min_colours)) | ~(err <= F(threshold)))
        return mean, var, err, mask.astype(np.uint8)


def compact(mask, pixmap):
    """the numpy statement of art_compact_mask_device: mask [H, W] or flat, pixmap = the rank's pixel list -> the selected pixels in list order"""
    pixmap = np.asarray(pixmap, np.uint32)
    return pixmap[np.asarray(mask).reshape(-1)[pixmap] != 0]


def threshold_for(accum_q, moments_q, count_q, aa_on, lum_floor):
    """the binary32 error of one pixel, to plant a threshold exactly equal to it"""
    return estimate(accum_q, moments_q, count_q, aa_on, 2, 1 << 30, 0.0, lum_floor)[2]


def planted(W, H, aa_on, max_samples, lum_floor, seed=5):
    """(accum [H, W, 3], moments [H, W, 2], counts [H, W] uint32, threshold): random plausible planes with, planted at fixed pixels, s = 0,
    n = 1, a count that is no multiple of per, D < 0, NaN and infinite moments and accum, -0.0 accum, s at and above max_samples, and a
    threshold exactly equal to one pixel's error (pixel 11)."""
    rng = np.random.default_rng(seed)
    per = 4 if aa_on else 1
    N = W * H
    ncol = rng.integers(2, 40, N).astype(np.uint32)
    counts = (ncol * per).astype(np.uint32)
    lum = rng.uniform(0.0, 2.0, N)
    sd = rng.uniform(0.0, 1.0, N) * lum
    S1 = (ncol * lum * per).astype(F)
    S2 = (ncol * ((lum * per) ** 2 + (sd * per) ** 2)).astype(F)
    accum = (rng.uniform(0.0, 3.0, (N, 3)) * counts[:, None]).astype(F)
    mom = np.stack([S1, S2], -1).astype(F)
    nan, inf = F(np.nan), F(np.inf)
    counts[3:9] = 3 * per; counts[11] = 8 * per; counts[13] = 8 * per; counts[16] = 8 * per
    counts[0] = 0; accum[0] = (1.0, 2.0, 3.0)                                       # s = 0: the accum is not read into the mean
    counts[1] = per                                                                 # n = 1
    counts[2] = 2 * per; mom[2] = (F(4.0), F(1.0))                                  # D = 1 - 16 / 2 < 0
    mom[3] = (nan, F(1.0)); mom[4] = (F(1.0), nan); mom[5] = (inf, inf); mom[6] = (F(1.0), inf)
    accum[7] = (nan, inf, -inf); accum[8] = (F(-0.0), F(0.0), F(-0.0))
    counts[9] = max_samples; mom[9] = (F(1.0), F(100.0))                            # s at the cap, far from converged
    counts[10] = max_samples + per; mom[10] = (F(1.0), F(100.0))                    # above it
    counts[12] = max_samples - per; mom[12] = (F(1.0), F(100.0))                    # just below it: selected
    mom[11] = (F(8.0), F(12.5))                                                     # 8 colours, D = 12.5 - 64 / 8 > 0: its error is the threshold
    mom[13] = (F(0.0), F(0.0))                                                     # a black pixel: 0 / lum_floor (0 / 0 = NaN with a zero floor)
    counts[14] = 2 * per + 1                                                        # no whole number of colours: n is a fraction
    counts[15] = per + per // 2 + 1                                                 # 1 < n < 2 (aa) or n = 2 (no aa)
    mom[16] = (F(-3.0), F(9.0))                                                     # a negative mean luminance: fabs
    accum = accum.reshape(H, W, 3); mom = mom.reshape(H, W, 2); counts = counts.reshape(H, W)
    thr = F(threshold_for(accum.reshape(-1, 3)[11], mom.reshape(-1, 2)[11], counts.reshape(-1)[11], aa_on, lum_floor))
    assert np.isfinite(thr) and thr > 0
    return accum, mom, counts, thr


def adaptive_loop(rad, aa_on, budget_samples, step_vthreads, threshold, lum_floor, min_colours, max_samples, first_vthreads=None, background=(0.0, 0.0, 0.0)):
    """The plain loop of Backend.render_adaptive on the CPU.  rad [S_max, H, W, 3]: the oracle's radiance of every pixel's camera samples
    (tests/moments_ref.sample_radiance); a pixel takes sample indices spp .. spp + S - 1 in the passes that select it.  One full pass of
    first_vthreads (default step_vthreads), then estimate and masked pass until the mask is empty, the next pass would exceed the budget or
    the samples run out.  Returns (accum, moments, counts, passes)."""
    import moments_ref as M
    per = 4 if aa_on else 1
    Hh, Ww = rad.shape[1:3]
    S0 = (first_vthreads or step_vthreads) * per
    S = step_vthreads * per
    acc, mom = M.add_colours(M.colours(rad[:S0], aa_on, background))
    counts = np.full((Hh, Ww), S0, np.uint32)
    spp, used, passes = S0, S0 * Hh * Ww, 1
    while True:
        mask = estimate(acc, mom, counts, aa_on, min_colours, max_samples, threshold, lum_floor)[3].astype(bool)
        k = int(mask.sum())
        if k == 0 or used + k * S > budget_samples or spp + S > rad.shape[0]:
            break
        a2, m2 = M.add_colours(M.colours(rad[spp:spp + S][:, mask], aa_on, background), acc[mask], mom[mask])
        acc[mask] = a2; mom[mask] = m2
        counts[mask] += np.uint32(S)
        spp += S; used += k * S; passes += 1
    return acc, mom, counts, passes
