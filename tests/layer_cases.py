"""Colour layers on the constructed similar sets of tests/bayes_cases.py (test infrastructure only): what bcd_hip_bayes_accumulate_layers is handed.

A layer list belongs to one bayes_cases.Case: every layer is a Case of its own with the SAME masks, |S|, states, radii and eigenvalue floor (one call
has one selection and one floor) and its own colours and per-pixel covariances, so bayes_ref.accumulate gives its float64 reference and its float32
calibrator unchanged.  The kinds, in the order of the list:
  0  the case itself;
  1  a copy scaled by 2^k, |k| >= 10 (colours x 2^k, covariances x 4^k; the floor stays the call's): a window or a covariance taken from the wrong
     layer is off by three orders of magnitude;
  2  independent content: another seed of the noise model, another signal, another noise level, its own covariance -- nothing of layer 0;
  3  layer 0 with its channels rotated (r, g, b) -> (g, b, r) and the six covariance entries permuted to match;
  non-finite family: + a layer with NaN / inf colours and a layer with NaN covariances, each between finite layers;
  floor-boundary family: + a layer scaled far below the floor (its items take the redo list), a layer scaled far above it (none does), and the
     first again: redo next to no redo in both orders.
Longer lists cycle kinds 1 - 3 with fresh seeds and exponents; every scaled / rotated layer after the first cycle is derived from a fresh independent
layer instead of layer 0.  Shared by tests/test_layers_ref_cpu.py (the calibrator stays meaningful on every layer) and tests/test_gpu_layers_stage.py."""
import numpy as np

import bayes_cases as bc
import bayes_ref as br

ROT = [1, 2, 0]                 # channels of the rotated layer: (g, b, r)
ROT6 = [1, 2, 0, 4, 5, 3]       # xx yy zz yz xz xy of the rotated channels: yy zz xx zx(= xz) yx(= xy) yz
EXPONENTS = (10, -10, 12, -11, 11, -12)


def derive(case, name, col, pixcov, judged=None):
    """a layer of `case`: its selection and floor, other images"""
    o = bc.Case.__new__(bc.Case)
    o.__dict__.update(case.__dict__)
    o.name = "%s / %s" % (case.name, name)
    o.col = np.ascontiguousarray(col, np.float32)
    o.pixcov = np.ascontiguousarray(pixcov, np.float32)
    if judged is not None:
        o.judged = judged
    return o


def scaled(case, k, src=None, tag=""):
    src = case if src is None else src
    return derive(case, "x 2^%d%s" % (k, tag), src.col * np.float32(2.0 ** k), src.pixcov * np.float32(4.0 ** k), judged=src.judged)


def rotated(case, src=None, tag=""):
    src = case if src is None else src
    return derive(case, "rotated%s" % tag, src.col[..., ROT], src.pixcov[..., ROT6], judged=src.judged)


def other_signal(H, W):
    """unlike bayes_cases.signal in every channel: other periods, other phases, other levels"""
    l, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([0.3 + 0.15 * np.cos(l / 5.0 - c / 8.0), 0.7 + 0.25 * np.sin(l / 14.0 + c / 6.0), 0.2 + 0.1 * np.cos(c / 4.0 + l / 19.0)], -1)


def independent(case, seed, sigma=0.05):
    """content that shares nothing with layer 0: its own signal, noise drawn with exactly the covariance it states (an ordinary, well-posed problem: judged)"""
    rng = np.random.default_rng(seed)
    H, W, _ = case.col.shape
    B = bc.noise_model(H, W, rng, sigma)
    col = other_signal(H, W) + np.einsum("...ij,...j->...i", B, rng.standard_normal((H, W, 3)))
    return derive(case, "independent seed %d" % seed, col, bc.cov6(B), judged=True)


def poisoned(case, seed, what):
    """an independent layer with non-finite values inside the patches of members of every second item"""
    rng = np.random.default_rng(seed)
    o = independent(case, seed + 1000)
    col, pc = o.col.copy(), o.pixcov.copy()
    H, W, _ = col.shape
    pts = np.argwhere(case.state == 1)
    for (l, c) in pts[::2]:
        pos = br.decode_members(case.mask[l, c], int(l), int(c), case.b)
        if not len(pos):
            continue
        q = pos[rng.integers(len(pos))]
        if what == "cov":
            pc[q[0], q[1], rng.integers(6)] = np.nan
        else:
            ql = min(max(q[0] + rng.integers(-case.w, case.w + 1), 0), H - 1)
            qc = min(max(q[1] + rng.integers(-case.w, case.w + 1), 0), W - 1)
            col[ql, qc, rng.integers(3)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
    return derive(case, "non-finite %s seed %d" % ("covariances" if what == "cov" else "colours", seed), col, pc, judged=True)


def base_layers(case, family, seed):
    out = [derive(case, "layer 0", case.col, case.pixcov), scaled(case, EXPONENTS[0]), independent(case, seed), rotated(case)]
    if family == "non-finite":
        out = [out[0], out[1], poisoned(case, seed + 1, "col"), out[2], poisoned(case, seed + 2, "cov"), out[3]]
    if family == "floor boundary":
        ind = independent(case, seed + 3)
        out += [scaled(case, -14, tag=" (below the floor)"), scaled(case, 14, ind, " (independent, above the floor)"), scaled(case, -16, tag=" (below the floor)")]
    return out


def layers(case, family, n, seed=7000):
    """n layers of `case`: the base list, then kinds 1 - 3 cycled with fresh seeds, on fresh independent content"""
    out = base_layers(case, family, seed)
    i = 0
    while len(out) < n:
        fresh = independent(case, seed + 10 + i, sigma=(0.05, 0.1, 0.02)[i % 3])
        kind = i % 3
        if kind == 0:
            out.append(scaled(case, EXPONENTS[(1 + i // 3) % len(EXPONENTS)], fresh, " of seed %d" % (seed + 10 + i)))
        elif kind == 1:
            out.append(fresh)
        else:
            out.append(rotated(case, fresh, " of seed %d" % (seed + 10 + i)))
        i += 1
    return out[:n]


def default_count(family):
    """layers of the per-family tests: four, and every special layer of the two families that have some"""
    return {"non-finite": 6, "floor boundary": 7}.get(family, 4)


def geometry_cases(w, b):
    """the situations of the families "sizes", "borders" and "non-finite" and a dense frame, rebuilt for patch radius w and search radius b (the
    families themselves are w = 1, b = 6): -> [(case, family name for layers())].  Sizes straddle the fallback limit 3 (2w+1)^2 + 1 and the window."""
    rng = np.random.default_rng(9000 + 100 * w + b)
    K1, side2, step = 3 * (2 * w + 1) ** 2 + 1, (2 * b + 1) ** 2, 2 * (b + w) + 1
    H, W = 4 * step + 7, 5 * step + 5                                    # 4 x 5 isolated items
    sizes = tuple(sorted(set(max(1, min(s, side2)) for s in (1, 3, K1 - 2, K1 - 1, K1, K1 + 1, K1 + 5, 2 * K1, side2 // 2, side2 - 1, side2))))
    tag = "w=%d b=%d " % (w, b)
    out = []
    col, pc = bc.noisy_frame(H, W, rng)
    out.append((bc.Case(tag + "sizes", col, pc, bc.sized_sets(H, W, rng, sizes, w, b), w=w, b=b), "sizes"))
    col, pc = bc.noisy_frame(H, W, rng)
    out.append((bc.Case(tag + "borders line 0", col, pc, {p: bc.window(p[0], p[1], H, W, w, b) for p in bc.border_points(H, W, 0, w, b)}, w=w, b=b), "borders"))
    col, pc = bc.noisy_frame(H, W, rng)
    sets = bc.sized_sets(H, W, rng, sizes[::-1], w, b)
    for i, p in enumerate(sorted(sets)[::3]):                            # every third item is poisoned: NaN colour, inf colour, NaN covariance in turn
        q = sets[p][rng.integers(len(sets[p]))]
        if i % 3 == 2:
            pc[q[0], q[1], rng.integers(6)] = np.nan
        else:
            col[q[0] + rng.integers(-w, w + 1), q[1] + rng.integers(-w, w + 1), rng.integers(3)] = np.nan if i % 3 == 0 else np.inf
    out.append((bc.Case(tag + "non-finite", col, pc, sets, w=w, b=b), "non-finite"))
    col, pc = bc.noisy_frame(bc.HD, bc.WD, rng)
    dsizes = (max(1, K1 - 20), K1 - 1, K1, K1 + 9, min(side2, 2 * K1), 5)   # half of the items are fallback pixels: overlapping aggregates of both kinds
    out.append((bc.Case(tag + "dense", col, pc, bc.dense_sets(bc.HD, bc.WD, rng, dsizes, w, b), w=w, b=b, dense=True), "sizes"))
    return out


def narrow_dense_case(W, H=37, seed=9500):
    """a dense frame W pixels wide (one 16 x 16 tile column exactly, or one with a single ragged column), fallback pixels and full estimates mixed"""
    rng = np.random.default_rng(seed + W)
    col, pc = bc.noisy_frame(H, W, rng)
    return bc.Case("dense %d wide" % W, col, pc, bc.dense_sets(H, W, rng, (5, 20, 27, 28, 40, 100)), dense=True)


def group_cases():
    """what the children of the BCD_HIP_WEAK_LAYERS_GROUP test run: a dense case with 5 layers (4 extra: groups of 1 / 2 / 3 give 1+1+1+1, 2+2, 3+1)
    and an isolated case with 4 layers (3 extra: 1+1+1, 2+1, 3), most items fallback pixels -- the only kernel the group size reaches"""
    rng = np.random.default_rng(9700)
    col, pc = bc.noisy_frame(bc.HD, bc.WD, rng)
    dense = bc.Case("group dense", col, pc, bc.dense_sets(bc.HD, bc.WD, rng, (1, 5, 9, 20, 27, 28, 64)), dense=True)
    H, W = 70, 100
    col, pc = bc.noisy_frame(H, W, rng)
    iso = bc.Case("group isolated", col, pc, bc.sized_sets(H, W, rng, (1, 9, 27, 28, 20, 5, 64, 26)))
    return [(dense, layers(dense, "sizes", 5, 9710)), (iso, layers(iso, "sizes", 4, 9720))]


_families = {}


def family_layers(family, n=None):
    """[(case, [layers])] of a family of bayes_cases.FAMILIES, once per session"""
    n = default_count(family) if n is None else n
    if (family, n) not in _families:
        _families[(family, n)] = [(c, layers(c, family, n, 7000 + 100 * i)) for i, c in enumerate(bc.FAMILIES[family]())]
    return _families[(family, n)]


_refs = {}


def references(layer):
    """float64 reference and float32 calibrator of a layer, once per session: (sum_64, count_64, items, sum_32)"""
    if id(layer) not in _refs:
        s64, c64, items = br.accumulate(*layer.args(), keep_stages=False)
        s32, _, _ = br.accumulate(*layer.args(), dtype=np.float32, keep_stages=False)
        _refs[id(layer)] = (layer, s64, c64, items, s32)
    return _refs[id(layer)][1:]


if __name__ == "__main__":
    # child of tests/test_gpu_layers_stage.py::test_layer_group_sizes_in_child_processes: the group size of the layered tile kernel is read once per
    # process from BCD_HIP_WEAK_LAYERS_GROUP; runs group_cases() through the layered stage call and stores sums and counts for the parent
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import bcd_amd.hip as bh

    ctx = bh.Context(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = {}
    for i, (case, ls) in enumerate(group_cases()):
        sums, cnt, redo = ctx.bayes_accumulate_layers([(t(l.col), t(l.pixcov)) for l in ls], t(case.mask.view(np.int32)), t(case.nsim), t(case.state), case.w, case.b, case.min_eig)
        ctx.synchronize()
        res["sums%d" % i] = np.stack([s.cpu().numpy() for s in sums])
        res["count%d" % i] = cnt.cpu().numpy()
    ctx.close()
    np.savez(sys.argv[1], **res)
