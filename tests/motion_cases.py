"""Constructed inputs of the motion tests (tests/test_motion_cases_cpu.py, tests/test_gpu_motion_stage.py, tests/test_gpu_motion.py).  TEST INFRASTRUCTURE.

Stage level -- frames with histograms and sample counts from temporal_cases.frame and arbitrary bit patterns as colours and covariances (the warp is a
bit-for-bit gather: NaN payloads, -0.0 and denormals must survive it), and motion fields by name (`field`):
    zero        +0.0 everywhere
    random      integer motion, every target inside the image: all pixels valid
    ties        fractions at the x.5 ties of both parities (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, -1.5 -> -2), +-0.0 and -0.49999997 (-> -0), dx and dy cycling
                at different periods; targets that leave the image are invalid
    special     NaN, +-inf, +-2^24 and the float below 2^24 in either component, and along each border one line of targets one pixel outside the image next to
                a line of targets exactly on the border
    checker     NaN where line + column is odd, zero elsewhere: a validity checkerboard
    corner      zero motion with ONE NaN at (3, 3): the upper-left patch corner of the candidate (4, 4) of the main pixels around it

Whole call -- frames of a sample model like oracle_lib.synth_samples at 32 spp (scene_samples: half flat, half structured), one seed per frame as
tests/test_gpu_temporal.py, cut out of a common canvas so that a neighbour can be a realisation of the scene SHIFTED by a whole number of pixels.  Frame 0 carries a few one-sample pixels (THIN): a pixel of zeros in a warped
neighbour gives 0/0 = NaN distance terms wherever the frame's pixel has a bin above 1, which at 32 spp is everywhere, so only across a thin pixel does the
ungated reference keep a member that the gate removes at full resolution (at coarser levels partly valid blocks do that by themselves).
    holes(W, H, f)       the field of neighbour f of the configurations with invalid pixels: zero motion on the left, random integer motion in [-2, 2] on the
                         right, NaN on the thin pixels and on a block, +inf on a few pixels, targets above the image along the first line
    all_valid(W, H, f)   a random integer field with every target inside the image
    translated(W, H)     frame and ONE neighbour that shows the scene shifted by (+9, -8) -- beyond the search radius 6 -- and the matching constant field; its scene is the structured one everywhere (in a flat scene a shift changes little)"""
import numpy as np

import temporal_cases as tc

F = np.float32
SEEDS = (1234, 77, 4321)
SIZES = ((64, 44), (72, 48))
CONFIGS = [(W, H, S, nf) for (W, H) in SIZES for S in (1, 3) for nf in (1, 2)]          # (width, height, scales, neighbours)
M, R, SEED = 1.0, 1, 1234                                                                  # -m 1, seeded random order
SHIFT = (9, -8)                                                                            # (dx, dy) of the translated case


# ---- stage level --------------------------------------------------------------------------------------------------------------------------------------
STAGE_SIZES = ((1, 1), (2, 2), (17, 5), (64, 4), (65, 7), (257, 3))     # either side of a 64-pixel tile line and of a 256-pixel workgroup
STAGE_DEPTHS = (60, 120, 36, 24, 12, 45, 7)                             # the last two: the element-by-element form
STAGE_LAYERS = (1, 2, 4, 5, 16)
FIELDS = ("zero", "random", "ties", "special", "checker", "corner")


def bit_patterns(shape, seed):
    """float32 of arbitrary finite values sprinkled with NaNs of two payloads, an infinity, -0.0 and a denormal"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(F)
    flat = a.reshape(-1).view(np.uint32)
    special = np.array([0x7fc00000, 0x7fa00001, 0xff800000, 0x80000000, 0x00000001], np.uint32)
    pos = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 7)), replace=False)
    flat[pos] = special[np.arange(len(pos)) % len(special)]
    return a


def stage_frame(W, H, D, seed=3):
    """(colours, sample counts, histograms, covariances) of one neighbour, nothing in it zero by accident: the sample counts are 16"""
    hist, ns = tc.frame(W, H, D, 16, seed)
    return bit_patterns((H, W, 3), seed + 1), ns, hist, bit_patterns((H, W, 6), seed + 2)


def stage_layers(W, H, L, seed=11):
    return [(bit_patterns((H, W, 3), seed + 2 * k), bit_patterns((H, W, 6), seed + 2 * k + 1)) for k in range(L)]


def _inside_random(W, H, rng, reach):
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tl = np.clip(l + rng.integers(-reach, reach + 1, (H, W)), 0, H - 1)
    tcol = np.clip(c + rng.integers(-reach, reach + 1, (H, W)), 0, W - 1)
    return np.stack([tcol - c, tl - l], -1).astype(F)


def field(name, W, H, seed=5):
    rng = np.random.default_rng(seed)
    mv = np.zeros((H, W, 2), F)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if name == "zero":
        return mv
    if name == "random":
        return _inside_random(W, H, rng, 40)
    if name == "ties":
        vals = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.0, -0.0, -0.49999997, 0.49999997, 3.5], F)
        mv[..., 0] = vals[(l * W + c) % len(vals)]
        mv[..., 1] = vals[(l * W + c) // 3 % len(vals)]
        return mv
    if name == "special":
        big = F(2.0 ** 24)
        vals = [np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, F(0)), -np.nextafter(big, F(0))]
        flat = mv.reshape(-1, 2)
        for i in range(flat.shape[0]):
            if i % 3 == 0:
                flat[i, (i // 3) % 2] = vals[(i // 3) % len(vals)]
        if W > 2:
            mv[:, 1, :], mv[:, W - 2, :] = (-1, 0), (1, 0)            # exactly onto the border: valid
        if H > 2:
            mv[1, 1:W - 1, :], mv[H - 2, 1:W - 1, :] = (0, -1), (0, 1)
        mv[:, 0, :], mv[:, W - 1, :] = (-1, 0), (1, 0)                # one pixel outside the left / right border
        mv[0, :, :], mv[H - 1, :, :] = (0, -1), (0, 1)                # ... above / below
        return mv
    if name == "checker":
        mv[(l + c) % 2 == 1] = np.nan
        return mv
    if name == "corner":
        if H > 3 and W > 3:
            mv[3, 3, 0] = np.nan
        return mv
    raise KeyError(name)


# ---- the whole call -----------------------------------------------------------------------------------------------------------------------------------
def thin_pixels(W, H):
    """(line, column) of the one-sample pixels of frame 0"""
    return [(10, 12), (11, W - 24), (H - 14, 25), (H - 6, W - 9)]


_canvas = {}


SPLIT = 32          # canvas columns below it are the flat part of the scene


def scene_samples(CW, CH, seed, split=SPLIT, spp=32, sigma=0.35, spike_prob=0.01):
    """oracle_lib.synth_samples with a scene in ABSOLUTE canvas coordinates (so that two windows of one canvas show one scene): left of column SPLIT a flat
    part with a gentle gradient, where similar sets are large at every pyramid level, right of it the ramps and the 16-pixel checker of synth_samples, where
    they are small (split = 0: structured everywhere, the translated case) -- every scale of the whole-call configurations then has full estimates and fallback pixels (tests/test_motion_cases_cpu.py)"""
    rng = np.random.default_rng(seed)
    l, c = np.meshgrid(np.arange(CH), np.arange(CW), indexing="ij")
    flat = np.stack([0.4 + 0.002 * c, 0.5 + 0.04 * np.sin(0.15 * l), 0.3 + 0.002 * l], -1)
    rough = np.stack([0.2 + 0.6 * c / 64.0, 0.5 + 0.4 * np.sin(12.0 * l / 44.0), np.where((l // 16 + c // 16) % 2 > 0, 0.8, 0.15)], -1)
    base = np.where((c < split)[..., None], flat, rough).astype(F)
    s = base[:, :, None, :] * (1.0 + sigma * rng.standard_normal((CH, CW, spp, 3)).astype(F))
    s = s + (rng.random((CH, CW, spp, 1)) < spike_prob) * 4.0 * rng.random((CH, CW, spp, 3))
    s = np.maximum(s, 0).astype(F)
    ll = np.broadcast_to(l[:, :, None], (CH, CW, spp)).astype(F)
    cc = np.broadcast_to(c[:, :, None], (CH, CW, spp)).astype(F)
    return np.ascontiguousarray(np.concatenate([ll[..., None], cc[..., None], s, np.ones((CH, CW, spp, 1), F)], -1).reshape(-1, 6))


def _realisation(CW, CH, seed, thin=(), split=SPLIT):
    """(colours, sample counts, histograms, covariances) of realisation `seed` of the CW x CH canvas at 32 spp; the pixels `thin` keep their first sample only
    (their covariance, 0 / 0 from one sample, is set to 0)"""
    import oracle_lib as ol
    key = (CW, CH, seed, tuple(thin), split)
    if key not in _canvas:
        s = scene_samples(CW, CH, seed, split)
        keep = np.ones(len(s), bool)
        for (l, c) in thin:
            keep[np.nonzero((s[:, 0] == l) & (s[:, 1] == c))[0][1:]] = False
        ns, mean, cov, hist = ol.oracle_ops()["accumulate"](s[keep], CW, CH)
        for (l, c) in thin:
            assert ns[l, c, 0] == 1
            cov[l, c] = 0
        _canvas[key] = (mean, ns, hist, cov)
    return _canvas[key]


def _cut(frame, l0, c0, H, W):
    out = tuple(np.ascontiguousarray(a[l0:l0 + H, c0:c0 + W]) for a in frame)
    for a in out:
        a.setflags(write=False)
    return out


def frames_of(W, H):
    """[frame, neighbour 1, neighbour 2]: three realisations of the W x H scene, frame 0 with its thin pixels"""
    return [_cut(_realisation(W, H, seed, thin_pixels(W, H) if i == 0 else ()), 0, 0, H, W) for i, seed in enumerate(SEEDS)]


def all_valid(W, H, f):
    return _inside_random(W, H, np.random.default_rng(900 + f), 5)


def holes(W, H, f):
    rng = np.random.default_rng(700 + f)
    mv = np.zeros((H, W, 2), F)
    right = _inside_random(W, H, rng, 2)
    mv[:, 2 * W // 3:] = right[:, 2 * W // 3:]
    for (l, c) in thin_pixels(W, H):
        mv[l, c, f % 2] = np.nan
    l0, c0 = (H // 2 - 3, W // 3) if f == 0 else (6, W // 2)
    mv[l0:l0 + 5, c0:c0 + 4] = np.nan                                  # a disoccluded block
    mv[H - 9, 7, 0], mv[20, W - 5, 1], mv[5, 30, 0] = np.inf, -np.inf, F(2.0 ** 24)
    mv[0, :, 1] = -1                                                   # the first line looks above the image
    return mv


def translated(W, H):
    """-> (frame, neighbour, field): the neighbour shows at (l + ry, c + rx) what the frame shows at (l, c), (rx, ry) = SHIFT, both cut from one canvas"""
    rx, ry = SHIFT
    CW, CH = W + abs(rx), H + abs(ry)
    oc, ol_ = max(0, rx), max(0, ry)                                   # the frame's window in the canvas
    frame = _cut(_realisation(CW, CH, SEEDS[0], split=0), ol_, oc, H, W)
    nb = _cut(_realisation(CW, CH, SEEDS[1], split=0), ol_ - ry, oc - rx, H, W)   # nb[l', c'] = canvas[ol - ry + l', oc - rx + c']: nb[l + ry, c + rx] = canvas[ol + l, oc + c]
    mv = np.zeros((H, W, 2), F)
    mv[..., 0], mv[..., 1] = rx, ry
    return frame, nb, mv


def unshifted(W, H):
    """the neighbour of translated(W, H) as the frame's own window of its canvas shows it: the second realisation without the shift"""
    rx, ry = SHIFT
    return _cut(_realisation(W + abs(rx), H + abs(ry), SEEDS[1], split=0), max(0, ry), max(0, rx), H, W)


def orders_draws(W, H, S, m=M, r=R, seed=SEED):
    import bcd_amd.hip as bh
    import marking_ref as mr
    orders, draws = [], []
    for s in range(S):
        sd = bh.scale_seed(seed, s)
        orders.append(bh.visit_order(W, H, 1, r, sd))
        draws.append(mr.skip_draw(W, H, m, sd))
        W, H = W // 2, H // 2
    return orders, draws


_refs = {}


def reference(kind, W, H, S, nf):
    """(frame, per-scale stats) of motion_ref.denoise_multiscale_motion for the fields `kind` ("holes" or "valid"), once per configuration"""
    import motion_ref as mo
    key = (kind, W, H, S, nf)
    if key not in _refs:
        fr = frames_of(W, H)
        make = holes if kind == "holes" else all_valid
        orders, draws = orders_draws(W, H, S)
        _refs[key] = mo.denoise_multiscale_motion(fr[0], fr[1:1 + nf], [make(W, H, f) for f in range(nf)], S, 1, 6, 1.0, 1e-8, orders, draws)
    return _refs[key]
