"""Constructed inputs of the tests of the feature gate of the cross-frame selection (tests/test_guide_cross_cases_cpu.py, tests/test_gpu_guide_cross_stage.py,
tests/test_gpu_temporal_guided.py; DESIGN 16, "Features").  TEST INFRASTRUCTURE.

Stage level -- feature images of a frame and of a neighbour:
    stage_images(W, H, F, var)   piecewise-constant regions plus noise, the neighbour's regions displaced by (1, -2): masks with set and cleared bits in every
                                 window; per-channel floors that differ, one channel switched off (floor 0) when there are no variances and F > 1
    identity(W, H, F, var)       the neighbour IS the frame
    rolled(W, H)                 the neighbour's features are the frame's rolled by ROLL = (2, -3): nb[l + 2, c - 3] = f[l, c]
    special(W, H)                channel 0 a depth with +inf background, channel 1 switched off: inf against inf (skipped), inf against finite (dissimilar),
                                 and a 3 x 3 block of NaN in the frame around NAN_AT (every term of that pixel's patch is skipped: 0 / 0)

Whole call -- the frames of tests/test_gpu_temporal.py (oracle_lib.synth_inputs at 32 spp, one seed per frame) at 40x28, 52x36 and 64x44 with the layers of
temporal_layers_cases.share_layers, three feature channels (slanted object-id stripes the radiance does not show, the scene's ramp, a slow wave) with per-frame noise, the fields
motion_cases.holes for the configurations with motion, and the benefit scene."""
import numpy as np

F32 = np.float32
ROLL = (2, -3)
NAN_AT = (5, 8)
SEEDS = (1234, 77, 4321)
M, R, SEED = 1.0, 1, 1234


# ---- stage level -----------------------------------------------------------------------------------------------------------------------------------------
def _regions(W, H, F, dl=0, dc=0):
    l, c = np.meshgrid(np.arange(H) - dl, np.arange(W) - dc, indexing="ij")
    return np.stack([(((l // (7 + k)) + (c // (12 + k))) % 2) * 0.5 for k in range(F)], -1).astype(F32)


def stage_images(W, H, F, var, seed=1):
    """-> dict(f, v, f_nb, v_nb, floors, tau): (H, W, F) float32 images (v, v_nb None without variances), F floors, the threshold"""
    rng = np.random.default_rng(seed * 1000 + W * 31 + H * 7 + F)
    f = _regions(W, H, F) + F32(0.03) * rng.standard_normal((H, W, F)).astype(F32)
    f_nb = _regions(W, H, F, 1, -2) + F32(0.03) * rng.standard_normal((H, W, F)).astype(F32)
    v = v_nb = None
    if var:
        v = (F32(0.0025) * (F32(0.5) + rng.random((H, W, F)).astype(F32))).astype(F32)
        v_nb = (F32(0.0025) * (F32(0.5) + rng.random((H, W, F)).astype(F32))).astype(F32)
    floors = np.array([0.01 * (1 + k % 3) for k in range(F)], F32)
    if F > 1:
        floors[1] = 0.0            # with variances the channel still counts; without, it is switched off
    return dict(f=f.astype(F32), v=v, f_nb=f_nb.astype(F32), v_nb=v_nb, floors=floors, tau=1.0)


def identity(W, H, F, var, seed=2):
    c = stage_images(W, H, F, var, seed)
    c["f_nb"], c["v_nb"] = c["f"], c["v"]
    return c


def rolled(W, H, seed=3):
    """random features (no two pixels alike), no variances: bit ROLL is set wherever p and p + ROLL are main pixels, since every term there is 0 / eps = 0"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((H, W, 2)).astype(F32)
    return dict(f=f, v=None, f_nb=np.roll(f, ROLL, axis=(0, 1)), v_nb=None, floors=np.array([0.01, 0.02], F32), tau=1.0)


def special(W, H, seed=4):
    """-> the case and the pixel sets its claims are about: background (depth +inf in both frames), frame_only (finite in the frame, +inf in the neighbour)"""
    assert W >= 20 and H >= 12
    rng = np.random.default_rng(seed)
    f = np.stack([F32(2.0) + F32(0.01) * rng.standard_normal((H, W)).astype(F32), rng.standard_normal((H, W)).astype(F32)], -1).astype(F32)
    f_nb = f.copy()
    f[:, W - 6:, 0] = np.inf                       # background in both frames: inf against inf
    f_nb[:, W - 6:, 0] = np.inf
    f_nb[:, W - 9:W - 6, 0] = np.inf               # the neighbour's background reaches further: finite against inf
    l, c = NAN_AT
    f[l - 1:l + 2, c - 1:c + 2, 0] = np.nan
    return dict(f=f, v=None, f_nb=f_nb, v_nb=None, floors=np.array([0.01, 0.0], F32), tau=1.0)


# widths either side of the 64-pixel tile line and of tile line plus halo, heights either side of the 4-line tile; (W, H, F, variances, w, b)
STAGE_GEOMETRIES = ([(W, H, 3, True, 1, 6) for (W, H) in ((63, 4), (64, 5), (65, 9), (70, 4), (70, 9), (64, 4), (63, 9), (65, 5), (70, 5))] +
                    [(9, 7, 3, True, 1, 6)] +                                                      # a frame smaller than the window
                    [(20, 12, 8, True, 2, 12), (20, 12, 8, True, 2, 15), (20, 12, 5, False, 2, 15)] +  # several staging bands
                    [(65, 9, 3, True, 1, 1), (65, 9, 3, True, 1, 2), (66, 9, 2, False, 0, 2), (30, 11, 4, True, 2, 6)] +
                    [(70, 9, F, var, 1, 6) for F in (1, 3, 8) for var in (False, True)])


# ---- the whole call --------------------------------------------------------------------------------------------------------------------------------------
FLOORS = (0.02, 0.5, 0.5)
TAU_G = 1.0
# (W, H, scales, neighbours, layers, variances): every size, scale count, N, L and both variance settings of the issue, each beside every other at least once
CONFIGS = [(40, 28, 1, 1, 1, False), (40, 28, 2, 2, 3, True), (52, 36, 1, 2, 1, True), (52, 36, 2, 1, 3, False), (64, 44, 1, 1, 3, True), (64, 44, 2, 2, 1, False)]
MOTION_CONFIGS = [(64, 44, 2, 2, 3, True), (52, 36, 1, 1, 1, False)]

_frames, _refs = {}, {}


def frames_of(W, H):
    """[(ns, hist, [(colours, covariances)] * 3)] of the frame and two neighbours"""
    import oracle_lib as ol
    import temporal_layers_cases as tl
    if (W, H) not in _frames:
        out = []
        for seed in SEEDS:
            col, ns, hist, cov, _ = ol.synth_inputs(W, H, 32, seed)
            out.append((ns, hist, tl.share_layers(col, cov)))
        _frames[(W, H)] = out
    return _frames[(W, H)]


def features_of(W, H, var):
    """[(features, variances or None)] of the frame and two neighbours: slanted stripes that the radiance does not show (an object id: the gate removes members
    the histograms accept), the scene's ramp and a slow wave, with per-frame noise"""
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([np.where(((l + 2 * c) // 11) % 2 > 0, 0.8, 0.15), 0.2 + 0.6 * c / W, 0.5 + 0.4 * np.sin(12.0 * l / H)], -1).astype(F32)
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(seed + 5)
        f = (base + F32(0.02) * rng.standard_normal(base.shape).astype(F32)).astype(F32)
        v = (F32(0.0004) * (F32(1) + F32(0.5) * rng.random(base.shape).astype(F32))).astype(F32) if var else None
        out.append((f, v))
    return out


def neutral_features(W, H):
    """a guide that can gate nothing: the same finite constant in every pixel of every frame (floors 1): every term is 0 / 1"""
    f = np.empty((H, W, 2), F32)
    f[..., 0], f[..., 1] = 0.7, -2.0
    return [(f, None)] * 3


def fields_of(W, H, N):
    import motion_cases as mc
    return [mc.holes(W, H, f) for f in range(N)]


def orders_draws(W, H, S, m=M, r=R, seed=SEED):
    import motion_cases as mc
    return mc.orders_draws(W, H, S, m, r, seed)


def reference(W, H, S, N, L, var, motion):
    """([layer 0 .. L-1 of the float64 composition], per-scale stats), once per configuration"""
    import guide_cross_ref as gx
    key = (W, H, S, N, L, var, motion)
    if key not in _refs:
        fr, ft = frames_of(W, H)[:1 + N], features_of(W, H, var)[:1 + N]
        orders, draws = orders_draws(W, H, S)
        fields = fields_of(W, H, N) if motion else None
        sel, outs, stats = {}, [], None
        for k in range(L):
            single = [(lay[k][0], ns, hist, lay[k][1]) for ns, hist, lay in fr]
            out, st = gx.denoise_multiscale(single[0], single[1:], fields, ft[0], ft[1:], FLOORS, TAU_G, S, 1, 6, 1.0, 1e-8, orders, draws, selections=sel)
            assert stats is None or st == stats
            outs.append(out)
            stats = st
        _refs[key] = (outs, stats)
    return _refs[key]


# ---- the benefit scene -----------------------------------------------------------------------------------------------------------------------------------
# Two albedos under one illumination; the edge between them stands at column EDGE in the frame and at EDGE + SWEEP in both neighbours (the object moved and no
# motion field is given).  At SPP samples with multiplicative noise SIGMA the radiance histograms of the two sides overlap, so the histogram distance accepts
# patches of the other albedo across frames; the albedo feature does not.  The band the edge sweeps is columns [EDGE, EDGE + SWEEP).
BW, BH, EDGE, SWEEP, SPP, SIGMA = 48, 32, 20, 5, 8, 0.5
ALBEDO = (np.array([0.45, 0.40, 0.35], F32), np.array([0.70, 0.62, 0.55], F32))
B_FLOORS, B_TAU_G = (0.0025, 0.0025, 0.0025), 1.0
_benefit = {}


def benefit_scene():
    """-> dict(frames [(col, ns, hist, cov)] * 3, guides [(albedo image, None)] * 3, base (H, W, 3): the frame's noise-free radiance, band: its column slice)"""
    import oracle_lib as ol
    if not _benefit:
        l, c = np.meshgrid(np.arange(BH), np.arange(BW), indexing="ij")
        light = (0.8 + 0.2 * np.sin(0.2 * l))[..., None].astype(F32)
        frames, guides, base0 = [], [], None
        for i, seed in enumerate(SEEDS):
            edge = EDGE if i == 0 else EDGE + SWEEP
            albedo = np.where((c < edge)[..., None], ALBEDO[0], ALBEDO[1]).astype(F32)
            base = (albedo * light).astype(F32)
            rng = np.random.default_rng(seed + 11)
            s = np.maximum(base[:, :, None, :] * (1.0 + SIGMA * rng.standard_normal((BH, BW, SPP, 3)).astype(F32)), 0).astype(F32)
            ll = np.broadcast_to(l[:, :, None], (BH, BW, SPP)).astype(F32)
            cc = np.broadcast_to(c[:, :, None], (BH, BW, SPP)).astype(F32)
            samples = np.ascontiguousarray(np.concatenate([ll[..., None], cc[..., None], s, np.ones((BH, BW, SPP, 1), F32)], -1).reshape(-1, 6))
            ns, mean, cov, hist = ol.oracle_ops()["accumulate"](samples, BW, BH)
            frames.append((mean, ns, hist, cov))
            guides.append((albedo, None))
            if i == 0:
                base0 = base
        _benefit.update(frames=frames, guides=guides, base=base0, band=slice(EDGE, EDGE + SWEEP))
    return _benefit


def band_rmse(out, scene):
    b = scene["band"]
    d = np.asarray(out, np.float64)[1:-1, b] - scene["base"][1:-1, b]
    return float(np.sqrt(np.mean(d * d)))


def benefit_reference():
    """(guided RMSE, unguided RMSE) of the NumPy composition over the band, -m 0 in scanline order, one scale"""
    import guide_cross_ref as gx
    import temporal_ref as tr
    if "ref" not in _benefit:
        sc = benefit_scene()
        orders, draws = orders_draws(BW, BH, 1, m=0.0, r=0)
        fr, gd = sc["frames"], sc["guides"]
        guided, _ = gx.denoise_multiscale(fr[0], fr[1:], None, gd[0], gd[1:], B_FLOORS, B_TAU_G, 1, 1, 6, 1.0, 1e-8, orders, draws)
        plain, _ = tr.denoise_multiscale(fr[0], fr[1:], 1, 1, 6, 1.0, 1e-8, orders, draws)
        _benefit["ref"] = (band_rmse(guided, sc), band_rmse(plain, sc))
    return _benefit["ref"]
