"""Constructed inputs of the tests of the cross-frame selection from means and covariances (tests/test_moments_cross_cases_cpu.py,
tests/test_gpu_moments_cross_stage.py, tests/test_gpu_temporal_moments.py; DESIGN 16, "Moments").  TEST INFRASTRUCTURE; everything is seeded.

Stage level -- the guide layers (colours, per-pixel covariances) of a frame and of a neighbour:
    stage_case(W, H, w, b, eps)   moments_cases.noisy with seed 1 for the frame and seed 2 for the neighbour: two regions, 8 samples per pixel; between pixels of
                                  one region a term has expectation about 1, so at tau = 1 the masks are neither empty nor full
    identity(W, H)                the neighbour IS the frame
    rolled(W, H)                  the neighbour is the frame rolled by ROLL = (2, -3): nb[l + 2, c - 3] = frame[l, c]
    special(W, H)                 the noisy pair with, away from each other: NaN covariances in the frame and in the neighbour, a block of equal colours and
                                  ZERO variance at the same place in both (eps = 0: nothing is counted, 0 / 0; eps > 0: distance 0), an infinite mean in the
                                  frame, a NaN mean in the frame, an infinite and a NaN mean in the neighbour
Thresholds as moments_cases.thresholds picks them: 1, a patch distance that occurs and the float below it.

Whole call -- the frames of tests/guide_cross_cases.py (oracle_lib.synth_inputs at 32 spp, one seed per frame, the layers of temporal_layers_cases.share_layers)
without their histograms, the fields motion_cases.holes, the features of guide_cross_cases.features_of, and the benefit scene."""
import numpy as np

import moments_cases as mc
import moments_cross_ref as mx

F = np.float32
ROLL = (2, -3)
FLOORS = [0.0, 1e-4]
# where the special pixels are (line, column); the frames are at least 48 x 12
NAN_COV_FRAME, NAN_COV_NB = (2, 5), (10, 45)       # (each further than the window from the infinite and NaN means of the other frame)
ZERO_BLOCK = (slice(5, 10), slice(20, 27))       # 5 x 7: a 3 x 3 patch fits inside with its whole neighbourhood
INF_MEAN_FRAME, NAN_MEAN_FRAME = (3, 33), (8, 12)
INF_MEAN_NB, NAN_MEAN_NB = (3, 14), (9, 3)

# (W, H, w, b): widths either side of the 64-pixel tile line and of tile line plus halo, heights either side of the 4-line tile, a frame smaller than the window
STAGE_FUSED = ([(W, H, 1, 6) for (W, H) in ((63, 4), (64, 5), (65, 9), (70, 4), (70, 9), (64, 9), (63, 5))] + [(9, 7, 1, 6)] +
               [(65, 9, 1, 1), (65, 9, 1, 2), (70, 5, 1, 2), (70, 13, 1, 6), (40, 28, 1, 6)])     # both forms
# w != 1 or b > 6.  b = 13 is the last radius with one staging band and the largest dynamic LDS request (64 800 B), b = 14 the first with two (15 + 14 lines)
STAGE_PLANES_ONLY = [(66, 9, 0, 2), (30, 11, 2, 6), (20, 12, 2, 12), (20, 12, 2, 13), (20, 12, 1, 14), (70, 12, 1, 13), (20, 12, 2, 15), (20, 12, 1, 15), (65, 9, 0, 6)]

_stage = {}


def _with_ref(key, m0, P0, mj, Pj, w, b, eps):
    if key not in _stage:
        D, valid = mx.distances(m0, P0, mj, Pj, w, b, eps)
        _stage[key] = dict(m0=m0, P0=P0, mj=mj, Pj=Pj, w=w, b=b, eps=eps, D=D, valid=valid, taus=mc.thresholds(D, valid))
    return _stage[key]


def pair(W, H, seeds=(1, 2)):
    """-> (colours, per-pixel covariances) of the frame and of the neighbour"""
    out = []
    for s in seeds:
        col, cov, ns, _ = mc.noisy(W, H, seed=s)
        out += [col, mc.pixel_cov(cov, ns)]
    return out


def stage_case(W, H, w, b, eps):
    """one pair of the stage test with its reference (computed once, shared read-only): dict(m0, P0, mj, Pj, w, b, eps, D, valid, taus)"""
    return _with_ref(("noisy", W, H, w, b, eps), *pair(W, H), w, b, eps)


def identity(W, H, w, b, eps):
    m0, P0, _, _ = pair(W, H)
    return _with_ref(("identity", W, H, w, b, eps), m0, P0, m0, P0, w, b, eps)


def rolled(W, H, w, b, eps):
    m0, P0, _, _ = pair(W, H)
    return _with_ref(("rolled", W, H, w, b, eps), m0, P0, np.roll(m0, ROLL, axis=(0, 1)), np.roll(P0, ROLL, axis=(0, 1)), w, b, eps)


def special_pair(W, H):
    assert W >= 48 and H >= 12
    m0, P0, mj, Pj = [a.copy() for a in pair(W, H)]
    P0[NAN_COV_FRAME] = np.nan
    Pj[NAN_COV_NB][:3] = np.nan                            # only the entries that are read
    for m, P in ((m0, P0), (mj, Pj)):
        m[ZERO_BLOCK] = F(0.5)
        P[ZERO_BLOCK] = 0
    m0[INF_MEAN_FRAME][1] = np.inf
    m0[NAN_MEAN_FRAME][2] = np.nan
    mj[INF_MEAN_NB][0] = np.inf
    mj[NAN_MEAN_NB][1] = np.nan
    return m0, P0, mj, Pj


def special(W, H, w, b, eps):
    return _with_ref(("special", W, H, w, b, eps), *special_pair(W, H), w, b, eps)


def similar_share(case):
    """(share of the in-window main pairs that are similar at tau = 1, the largest |S_j|) -- from the reference alone"""
    _, n = mx.masks_from(case["D"], case["valid"], 1.0)
    return float(n.sum()) / max(1, int(case["valid"].sum())), int(n.max())


# ---- the whole call --------------------------------------------------------------------------------------------------------------------------------------
# On these textured frames at 32 spp the moment distance at tau = 1 with a small floor leaves nearly every pixel below 3P + 1 members (fallback estimates only);
# tau = 2 with a floor of 1e-2 gives full and fallback estimates at both scales (40x28, N = 2: 39 of 165 full at scale 0, 13 of 109 at scale 1)
VAR_FLOOR = 1e-2
TAU = 2.0
# (W, H, scales, neighbours, layers, guide): every size, scale count, N, L of the issue and both guide settings, each beside every other at least once
CONFIGS = [(40, 28, 1, 1, 1, False), (40, 28, 2, 2, 3, True), (52, 36, 1, 2, 1, True), (52, 36, 2, 1, 3, False), (64, 44, 1, 1, 3, True), (64, 44, 2, 2, 1, False)]
MOTION_CONFIGS = [(64, 44, 2, 2, 3, True), (52, 36, 1, 1, 1, False), (40, 28, 2, 2, 1, False)]
_refs = {}


def frames_of(W, H):
    """[(ns, [(colours, covariances)] * 3)] of the frame and two neighbours: guide_cross_cases.frames_of without the histograms"""
    import guide_cross_cases as gc
    return [(ns, lay) for ns, _, lay in gc.frames_of(W, H)]


def select_one_scale(frame, neighbours, valids, guides, floors, tau_g, w, b, tau, eps, order, drawn):
    """the selection of one scale.  frame, neighbours[i]: (colours, sample counts, covariances) of the GUIDE layer at this level; valids[i]: None or the validity
    bytes of a warped neighbour; guides: None, or [(features, variances or None)] of every frame at this level"""
    import guide_cross_ref as gx
    import guide_ref as gr
    import marking_ref as mk
    import moments_ref as mr
    import motion_ref as mo
    import pyramid_ref as pr
    col, ns, cov = frame
    with np.errstate(all="ignore"):
        P0 = pr.pixel_cov(cov, ns)
    mask0, n0 = mr.masks(col, P0, w, b, tau, eps)
    mask0 = np.ascontiguousarray(mask0).view(np.uint32)
    if guides is not None:
        mask0, n0 = gx.gate(mask0, gr.masks(guides[0][0], guides[0][1], w, b, floors, tau_g)[0])
    frames = [(col, P0, mask0)]
    total = n0.astype(np.int32)
    cross = []
    for j, ((col_nb, ns_nb, cov_nb), valid) in enumerate(zip(neighbours, valids)):
        with np.errstate(all="ignore"):
            Pj = pr.pixel_cov(cov_nb, ns_nb)
        m, n = mx.masks(col, P0, col_nb, Pj, w, b, tau, eps)
        if valid is not None:
            m, n = mo.gate(m, n, valid, w, b)
        if guides is not None:
            m, n = gx.gate(m, gx.cross_masks(guides[0][0], guides[0][1], guides[j + 1][0], guides[j + 1][1], w, b, floors, tau_g)[0])
        frames.append((col_nb, Pj, m))
        cross.append(m)
        total = total + n
    state = mk.greedy(mask0, total, w, b, order, drawn)
    return dict(mask0=mask0, cross=cross, total=total, state=state, frames=frames)


def levels_of(ns_list, layers_list, motions, nscales):
    """-> (levels[s][f] = (ns, [(colours, covariances) per layer]) of frame f at level s, valids[s][f - 1]): a neighbour with a field is warped at full
    resolution first (sample counts and every layer), then every frame's pyramid: colours averaged, counts summed, covariances weighted by that frame's counts"""
    import motion_ref as mo
    import pyramid_ref as pr
    first, v0 = [], []
    for f, (ns, lay) in enumerate(zip(ns_list, layers_list)):
        mv = None if f == 0 or motions is None else motions[f - 1]
        if mv is None:
            first.append((np.asarray(ns, F), [(np.asarray(c, F), np.asarray(v, F)) for c, v in lay]))
            if f:
                v0.append(None)
            continue
        imgs = [np.asarray(ns, F)] + [a for c, v in lay for a in (c, v)]
        out, ok = mo.warp(imgs, mv)
        first.append((out[0], [(out[1 + 2 * k], out[2 + 2 * k]) for k in range(len(lay))]))
        v0.append(ok)
    levels, valids = [first], [v0]
    with np.errstate(all="ignore"):
        for _ in range(1, nscales):
            levels.append([(pr.downscale_sum(ns), [(pr.downscale_avg(c), pr.downscale_cov(v, ns)) for c, v in lay]) for ns, lay in levels[-1]])
            valids.append([None if v is None else mo.valid_down(v) for v in valids[-1]])
    return levels, valids


def denoise_multiscale(ns_list, layers_list, motions, guides, floors, tau_g, nscales, w, b, tau, eps, min_eig, orders, draws, dtype=np.float64):
    """the whole call in float64: the selection of every scale from layer 0 (select_one_scale), every layer's estimate on it (temporal_ref.accumulate),
    mergeOutputs coarse to fine.  ns_list[f], layers_list[f]: the sample counts and the [(colours, covariances)] of frame f, [0] the frame itself; guides: None or
    [(features, variances or None)] per frame -> ([out of layer 0 .. L-1], [stats of scale 0, 1, ...])"""
    import guide_cross_ref as gx
    import marking_ref as mk
    import motion_ref as mo
    import pyramid_ref as pr
    import temporal_ref as tr
    L = len(layers_list[0])
    levels, valids = levels_of(ns_list, layers_list, motions, nscales)
    glev = None
    if guides is not None:
        glev = gx.guide_levels(guides[0], guides[1:], [None] * (len(guides) - 1) if motions is None else list(motions), nscales)
    outs, stats = [[None] * nscales for _ in range(L)], [None] * nscales
    for s in range(nscales - 1, -1, -1):
        lv = levels[s]
        sel = select_one_scale((lv[0][1][0][0], lv[0][0], lv[0][1][0][1]), [(f[1][0][0], f[0], f[1][0][1]) for f in lv[1:]], valids[s],
                               None if glev is None else glev[s], floors, tau_g, w, b, tau, eps, orders[s], draws[s])
        stats[s] = mo.selection_stats(sel, w)
        masks = [sel["mask0"]] + sel["cross"]
        for k in range(L):
            with np.errstate(all="ignore"):
                frames = [(f[1][k][0], pr.pixel_cov(f[1][k][1], f[0]), m) for f, m in zip(lv, masks)]
            acc, cnt, items = tr.accumulate(frames, sel["total"], (sel["state"] == mk.ST_IN).astype(np.uint8), w, b, min_eig, dtype)
            assert stats[s]["processed"] == len(items)
            with np.errstate(all="ignore"):
                outs[k][s] = acc / cnt.astype(dtype)[..., None]
            if s < nscales - 1:
                outs[k][s] = pr.merge(outs[k][s], outs[k][s + 1], dtype=dtype)
    return [o[0] for o in outs], stats


def reference(W, H, S, N, L, guide, motion):
    """([layer 0 .. L-1 of the float64 composition], per-scale stats), once per configuration"""
    import guide_cross_cases as gc
    key = (W, H, S, N, L, guide, motion)
    if key not in _refs:
        fr = frames_of(W, H)[:1 + N]
        ft = gc.features_of(W, H, True)[:1 + N] if guide else None
        orders, draws = gc.orders_draws(W, H, S)
        fields = gc.fields_of(W, H, N) if motion else None
        _refs[key] = denoise_multiscale([ns for ns, _ in fr], [lay[:L] for _, lay in fr], fields, ft, gc.FLOORS, gc.TAU_G, S, 1, 6, TAU, VAR_FLOOR, 1e-8, orders, draws)
    return _refs[key]


# ---- the benefit scene -----------------------------------------------------------------------------------------------------------------------------------
# moments_cases.noisy: a static two-region scene at 8 samples per pixel; the frame is seed 1, its two neighbours are seeds 2 and 3 (independent noise on the same
# signal).  The figure is the RMSE against the noise-free signal over the main pixels, with neighbours over without.
BW, BH, B_SEEDS, B_TAU, B_FLOOR = 48, 32, (1, 2, 3), 1.0, 1e-4
_benefit = {}


def benefit_scene():
    if not _benefit:
        fr = [mc.noisy(BW, BH, seed=s) for s in B_SEEDS]
        _benefit.update(frames=[(ns, [(col, cov)]) for col, cov, ns, _ in fr], signal=fr[0][3])
    return _benefit


def rmse(out, scene):
    d = np.asarray(out, np.float64)[1:-1, 1:-1] - scene["signal"][1:-1, 1:-1]
    return float(np.sqrt(np.mean(d * d)))


def benefit_reference():
    """(RMSE with two neighbours, RMSE of the single frame) of the NumPy composition, -m 0 in scanline order, one scale"""
    import guide_cross_cases as gc
    if "ref" not in _benefit:
        sc = benefit_scene()
        orders, draws = gc.orders_draws(BW, BH, 1, m=0.0, r=0)
        fr = sc["frames"]
        res = []
        for n in (2, 0):
            (out,), _ = denoise_multiscale([ns for ns, _ in fr[:1 + n]], [lay for _, lay in fr[:1 + n]], None, None, None, None, 1, 1, 6, B_TAU, B_FLOOR, 1e-8, orders, draws)
            res.append(rmse(out, sc))
        _benefit["ref"] = tuple(res)
    return _benefit["ref"]
