"""Constructed inputs for the colour layers of a frame denoised with its neighbour frames: what bcd_hip_bayes_accumulate_temporal_layers is handed
(tests/test_gpu_temporal_layers_stage.py) and the frames of the whole call (tests/test_gpu_temporal_layers.py, tests/test_temporal_layers_cases_cpu.py).
TEST INFRASTRUCTURE.

A LayeredCase is a temporal_bayes_cases.Case -- 1 + F frames, one similar set per frame and processed pixel -- with L layers: every layer brings colours and
per-pixel covariances for EVERY frame, the masks, |S| and states are the case's.  The layers of a frame come from the builders of tests/layer_cases.py run
on that frame (kind 0 the frame itself, 1 scaled by 2^k, 2 independent content, 3 channels rotated, then the cycle on fresh content), with one seed per
frame, so layer k has the same kind and the same exponent in every frame and independent noise from frame to frame.  layer(k) is a
temporal_bayes_cases.Case of its own: temporal_ref.accumulate gives its float64 reference and float32 calibrator unchanged."""
import copy

import numpy as np

import bayes_cases as bc
import layer_cases as lc
import temporal_bayes_cases as tb

K1, FULLW, W_, B_ = tb.K1, tb.FULLW, tb.W_, tb.B_


class _Frame:
    """one frame of a temporal case in the terms the builders of layer_cases read: colours, per-pixel covariances, the frame-0 selection"""

    def __init__(self, case, f):
        self.name, self.col, self.pixcov, self.judged = "%s frame %d" % (case.name, f), case.col[f], case.pixcov[f], True
        self.mask, self.state, self.w, self.b = case.mask[0], case.state, case.w, case.b


class LayeredCase:
    def __init__(self, case, n, seed=7000):
        self.case, self.n = case, n
        self.name, self.dense = "%s, %d layers" % (case.name, n), case.dense
        shells = [_Frame(case, f) for f in range(case.F + 1)]
        per_frame = [lc.layers(sh, "sizes", n, seed + 100 * f) for f, sh in enumerate(shells)]
        self.names = [l.name[len(shells[0].name) + 3:] for l in per_frame[0]]
        self.col = [[per_frame[f][k].col for f in range(case.F + 1)] for k in range(n)]          # [layer][frame]
        self.pixcov = [[per_frame[f][k].pixcov for f in range(case.F + 1)] for k in range(n)]
        self._layers = {}

    def layer(self, k):
        """layer k as a temporal_bayes_cases.Case: the case's selection, this layer's images"""
        if k not in self._layers:
            o = copy.copy(self.case)
            o.name = "%s / layer %d (%s)" % (self.case.name, k, self.names[k])
            o.col, o.pixcov = list(self.col[k]), list(self.pixcov[k])
            self._layers[k] = o
        return self._layers[k]

    def replace(self, k, f, col=None, pixcov=None):
        """another image for layer k of frame f (before any reference of that layer is taken)"""
        assert k not in self._layers
        if col is not None:
            self.col[k][f] = np.ascontiguousarray(col, np.float32)
        if pixcov is not None:
            self.pixcov[k][f] = np.ascontiguousarray(pixcov, np.float32)

    def scale_layer(self, k, e):
        """layer k times 2^e in every frame (colours x 2^e, covariances x 4^e): far below the floor its full estimates take the redo list"""
        for f in range(self.case.F + 1):
            self.replace(k, f, self.col[k][f] * np.float32(2.0 ** e), self.pixcov[k][f] * np.float32(4.0 ** e))
        self.names[k] += " x 2^%d" % e


# ---- families of temporal_bayes_cases with layers ---------------------------------------------------------------------------------------------------
# (family, number of layers): sizes at F = 1 and F = 4 carry the layer counts 1, 2, 4, 5, 16 (a single layer; a short group; a full group; a group
# boundary; the maximum: four full groups); the other families 3 or 4 layers
# (pure noise is an extra: the issue's list is sizes, borders, centre only, non-finite, zero noise).  non-finite: the frames of that family hold a NaN and
# an inf per-pixel covariance in neighbour frames; the layer builders carry them along -- the scaled layer keeps them, the rotated layer moves them to
# another covariance entry, the independent layer has none -- so the same item is poisoned in some layers and clean in others, and the fallback item with a
# non-finite member stays finite in all of them
STAGE = [("sizes F=1", 1), ("sizes F=1", 2), ("sizes F=4", 4), ("sizes F=2", 5), ("sizes F=4", 16), ("borders", 3), ("centre only", 4), ("non-finite", 4),
         ("pure noise", 3), ("zero noise", 3)]

_stage = {}


def stage_cases(family, n):
    if (family, n) not in _stage:
        _stage[(family, n)] = [LayeredCase(c, n, 7000 + 1000 * i) for i, c in enumerate(tb.FAMILIES[family]())]
    return _stage[(family, n)]


def weak_list_case(items, F, seed):
    """`items` fallback pixels and nothing else (|S| of 1 .. 27 spread over the frames): weak lists either side of the seven pixels of a wavefront"""
    rng = np.random.default_rng(seed)
    H, W = 40, 130
    frames = tb.make_frames(H, W, rng, F)
    pts = bc.grid(H, W, W_, B_)[:items]
    assert len(pts) == items
    sets = {}
    for i, (l, c) in enumerate(pts):
        win = bc.window(l, c, H, W, W_, B_)
        total = (27, 1, 9, 26, 14, 2, 20, 5)[i % 8]
        s0 = int(rng.integers(0, total + 1))
        sets[(l, c)] = [tb.with_centre(win, s0, l, c, rng)] + [bc.subset(win, k, rng) for k in tb.split(total - s0, F, FULLW, rng)]
    return LayeredCase(tb.Case("weak list of %d F=%d" % (items, F), frames, sets), 3, seed)


def limit_case(seed=410):
    """|S| = 27 (the largest fallback) and |S| = 28 (the smallest full estimate) with the members spread over three frames, and an item with |S| = 0"""
    rng = np.random.default_rng(seed)
    H, W, F = 40, 100, 2
    frames = tb.make_frames(H, W, rng, F)
    pts = bc.grid(H, W, W_, B_)
    plan = [(9, 9, 9), (10, 9, 9), (0, 0, 0), (1, 13, 13), (1, 14, 13), (27, 0, 0), (0, 14, 14), (20, 4, 4)]
    sets = {}
    for (l, c), (n0, n1, n2) in zip(pts, plan):
        win = bc.window(l, c, H, W, W_, B_)
        sets[(l, c)] = [tb.with_centre(win, n0, l, c, rng), bc.subset(win, n1, rng), bc.subset(win, n2, rng)]
    return LayeredCase(tb.Case("27 / 28 / 0 members F=2", frames, sets), 5, seed)


def poisoned_case(seed=420):
    """a NaN covariance at one member pixel of a full item, in layer 1 of neighbour 2 only: that layer's item is NaN, no other layer's and no other item"""
    rng = np.random.default_rng(seed)
    H, W, F = 40, 100, 2
    frames = tb.make_frames(H, W, rng, F)
    pts = bc.grid(H, W, W_, B_)
    sets = {}
    for i, (l, c) in enumerate(pts):
        win = bc.window(l, c, H, W, W_, B_)
        n0, n1, n2 = ((40, 40, 40), (5, 10, 5), (60, 30, 90))[i % 3]
        sets[(l, c)] = [tb.with_centre(win, n0, l, c, rng), bc.subset(win, n1, rng), bc.subset(win, n2, rng)]
    case = LayeredCase(tb.Case("NaN covariance in layer 1 of neighbour 2", frames, sets), 3, seed)
    l, c = sets[pts[0]][2][len(sets[pts[0]][2]) // 2]
    pc = case.pixcov[1][2].copy()
    pc[l, c, 4] = np.nan
    case.replace(1, 2, pixcov=pc)
    case.poisoned_item, case.poisoned_layer = pts[0], 1
    return case


def redo_case(seed=430):
    """four layers of which 1 and 3 are scaled far below the eigenvalue floor: their full estimates take the redo list, those of the layers around them do not"""
    case = LayeredCase(tb.fam_sizes(2, seed), 4, seed)
    case.scale_layer(1, -24)       # (layer 1 is the 2^10 copy: 2^-14 of the frame, as the "below the floor" layers of layer_cases)
    case.scale_layer(3, -15)
    case.redo_layers = (1, 3)
    return case


def dense_case():
    return LayeredCase(tb.dense_case(21, 33, 2, 440, "dense 33x21 F=2"), 3, 440)


def call_sequence():
    """two layered estimates of different sizes, L and F on one context"""
    return [LayeredCase(tb.fam_sizes(1, 451), 2, 451), LayeredCase(tb.dense_case(30, 26, 2, 452, "dense 26x30 F=2"), 5, 452)]


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------------------
# 64x44 and 72x48, not the 40x28 and 52x36 of tests/test_gpu_temporal.py: at those two sizes the half-resolution scale of the F = 1 configurations has no
# full estimate at all (40x28: 216 processed, 216 fallback; 52x36: 384 / 384), so the per-layer chain would go unexercised there; these are the smallest
# sizes tried at which every configuration has fallback pixels at some scale and full estimates at every scale (test_temporal_layers_cases_cpu.py)
SIZES = ((64, 44), (72, 48))
SEEDS = (1234, 77, 4321)          # one per frame, as tests/test_gpu_temporal.py
CONFIGS = [(W, H, S, F, m, r) for (W, H) in SIZES for S in (1, 2) for F in (1, 2) for (m, r) in ((1.0, 1), (0.0, 0))]
L_WHOLE = 3


def share_layers(col, cov, n=L_WHOLE):
    """layers of a frame as a renderer splits it: the frame itself, then a smooth and a textured per-pixel, per-channel share g of it -- the layer whose
    samples are the frame's samples times g, so its mean is col g and its covariance cov (g g^T)"""
    H, W, _ = col.shape
    l, c = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    smooth = np.stack([0.2 + 0.5 * c / W, 0.6 - 0.4 * l / H, 0.3 + 0.3 * (l + c) / (H + W)], -1).astype(np.float32)
    tex = (0.999 - smooth) * np.stack([0.5 + 0.5 * np.sin(0.9 * c + 0.4 * l), 0.5 + 0.5 * np.cos(0.7 * l), ((l.astype(int) // 3 + c.astype(int) // 5) % 2) * 0.9 + 0.1], -1)
    out = [(np.ascontiguousarray(col, np.float32), np.ascontiguousarray(cov, np.float32))]
    for g in (smooth, tex.astype(np.float32)):
        gg = np.stack([g[..., 0] * g[..., 0], g[..., 1] * g[..., 1], g[..., 2] * g[..., 2], g[..., 1] * g[..., 2], g[..., 0] * g[..., 2], g[..., 0] * g[..., 1]], -1)
        out.append((np.ascontiguousarray(col * g), np.ascontiguousarray(cov * gg)))
    return out[:n]


_frames = {}


def frames_of(W, H, spp=32, sigma=0.35, spikes=0.01):
    """three frames of oracle_lib.synth_inputs, one seed each -> [(ns, hist, [(colours, covariances)] * L_WHOLE)], [0] the frame itself"""
    import oracle_lib as ol
    key = (W, H, spp, sigma, spikes)
    if key not in _frames:
        out = []
        for seed in SEEDS:
            col, ns, hist, cov = ol.synth_inputs(W, H, spp, seed, sigma, spikes)[:4]
            out.append((ns, hist, share_layers(col, cov)))
        _frames[key] = out
    return _frames[key]


_refs = {}


def reference(W, H, S, F, m, r, k, seed=1234):
    """(layer k of the result, per-scale stats) of the float64 composition on that layer alone, once per configuration and layer"""
    import bcd_amd.hip as bh
    import marking_ref as mr
    import temporal_layers_ref as tlr
    key = (W, H, S, F, m, r, k, seed)
    if key not in _refs:
        fr = frames_of(W, H)
        orders, draws, ws, hs = [], [], W, H
        for s in range(S):
            sd = bh.scale_seed(seed, s)
            orders.append(bh.visit_order(ws, hs, 1, r, sd))
            draws.append(mr.skip_draw(ws, hs, m, sd))
            ws, hs = ws // 2, hs // 2
        _refs[key] = tlr.denoise_multiscale(fr[0][0], fr[0][1], fr[0][2], fr[1:1 + F], k, S, 1, 6, 1.0, 1e-8, orders, draws)
    return _refs[key]
