"""Plain NumPy restatements of the operations of bcd_amd/csrc/k_pointwise.hip (pyramid reducers, interpolation, merge, the per-pixel passes), in the
reference's evaluation order.  TEST INFRASTRUCTURE ONLY.

Every arithmetic operation exists in two precisions through one body of code: `dtype=F32` is the restatement the oracle is held to bit for bit
(tests/test_pyramid_cases_cpu.py), `dtype=F64` the same expression in float64 -- the yardstick of the derived rounding bounds (`gamma`).

A *variant* is a dict of switches that turns the float32 restatement into a plausible kernel mistake; MUTANTS names them.  The CPU test requires each
to change at least one bit on every case tests/pyramid_cases.py names for it, so that a kernel making that mistake could not pass the GPU test:

    pairwise     (p1 + p2) + (p3 + p4) instead of ((p1 + p2) + p3) + p4             downscale_*, merge (through its average)
    right        p1 + ((p2 + p3) + p4)                                              the same
    swap         line and column neighbour exchanged in the block: p2 <-> p3        the same
    clamp_wrap   a neighbour outside the coarse image wraps around (index mod size) interpolate, merge
    clamp_last   ... or becomes the last valid index, on the low side too           interpolate, merge
    fma          products fused into the following addition                         interpolate, merge, downscale_cov
    no_presum    wa * p2 + wa * p3 instead of wa * (p2 + p3)                         interpolate, merge
    parity       the neighbour of an even fine index taken on the far side          interpolate, merge
    w_wrong      the weight nSum / n_i of downscale_cov taken from another pixel     downscale_cov
    merge_order  (hi + up(b)) - up(a) instead of (hi - up(a)) + up(b)               merge
    divide       x / n instead of (1 / n) * x                                       pixel_cov, finalize
"""
import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24   # unit round-off of float32


def gamma(n):
    """n roundings on a term's path: the computed sum of terms is sum(t_i (1 + d_i)), |d_i| <= (1 + u)^n - 1 <= n u / (1 - n u)  (Higham, Lemma 3.1)"""
    return n * U / (1.0 - n * U)


MUTANTS = {
    "pairwise": dict(assoc="pairwise"),
    "right": dict(assoc="right"),
    "swap": dict(swap=True),
    "clamp_wrap": dict(clamp="wrap"),
    "clamp_last": dict(clamp="last"),
    "fma": dict(fma=True),
    "no_presum": dict(presum=False),
    "parity": dict(parity=-1),
    "w_wrong": dict(w_from=(1, 0, 3, 2)),
    "merge_order": dict(merge_order="add_first"),
    "divide": dict(divide=True),
}
# the operations a mutant changes at all
MUTANT_OPS = {
    "pairwise": ("dsum", "davg", "dcov", "merge"), "right": ("dsum", "davg", "dcov", "merge"), "swap": ("dsum", "davg", "dcov", "merge"),
    "clamp_wrap": ("interp", "merge"), "clamp_last": ("interp", "merge"), "fma": ("interp", "merge", "dcov"), "no_presum": ("interp", "merge"),
    "parity": ("interp", "merge"), "w_wrong": ("dcov",), "merge_order": ("merge",), "divide": ("pixcov", "finalize"),
}


def _fma(a, b, c):
    """round32(a * b + c): the product of two float32 is exact in float64"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


# ---- positions ------------------------------------------------------------------------------------------------------------------------------------
def block_index(n):
    """first and second index of the n // 2 blocks along one axis: 2 k and min(2 k + 1, n - 1)"""
    i0 = 2 * np.arange(n // 2)
    return i0, np.minimum(i0 + 1, n - 1)


def block_positions(W, H):
    """(h2, w2, 4, 2) int: (line, column) of p1 = (2l, 2c), p2 = next line, p3 = next column, p4 = both"""
    l0, l1 = block_index(H)
    c0, c1 = block_index(W)
    L = np.stack(np.broadcast_arrays(l0[:, None], l1[:, None], l0[:, None], l1[:, None]), -1)
    Cc = np.stack(np.broadcast_arrays(c0[None, :], c0[None, :], c1[None, :], c1[None, :]), -1)
    L, Cc = np.broadcast_arrays(L, Cc)
    return np.stack([L, Cc], -1)


def _fold(v, n, clamp):
    if clamp == "clamp":
        return np.clip(v, 0, n - 1)
    if clamp == "wrap":
        return np.mod(v, n)
    return np.where((v < 0) | (v >= n), n - 1, v)   # "last"


def interp_index(N, n, parity=1, clamp="clamp"):
    """main and adjacent coarse index of the N fine indices along one axis (n coarse ones): u / 2 and u / 2 -+ 1 for even / odd u, folded into the image"""
    u = np.arange(N)
    m = u // 2
    a = m + parity * ((u % 2) * 2 - 1)
    return _fold(m, n, clamp), _fold(a, n, clamp)


def interp_positions(W, H, w, h):
    """(H, W, 4, 2) int: (line, column) of the main pixel, the column neighbour, the line neighbour and the diagonal one"""
    lc, al = interp_index(H, h)
    cc, ac = interp_index(W, w)
    L = np.stack(np.broadcast_arrays(lc[:, None], lc[:, None], al[:, None], al[:, None]), -1)
    Cc = np.stack(np.broadcast_arrays(cc[None, :], ac[None, :], cc[None, :], ac[None, :]), -1)
    L, Cc = np.broadcast_arrays(L, Cc)
    return np.stack([L, Cc], -1)


# ---- the reducers ---------------------------------------------------------------------------------------------------------------------------------
def _gather4(a, swap=False):
    H, W = a.shape[0], a.shape[1]
    l0, l1 = block_index(H)
    c0, c1 = block_index(W)
    p = [a[l0][:, c0], a[l1][:, c0], a[l0][:, c1], a[l1][:, c1]]
    if swap:
        p[1], p[2] = p[2], p[1]
    return p


def _sum4(p, assoc="seq"):
    if assoc == "pairwise":
        return (p[0] + p[1]) + (p[2] + p[3])
    if assoc == "right":
        return p[0] + ((p[1] + p[2]) + p[3])
    return ((p[0] + p[1]) + p[2]) + p[3]


def downscale_sum(a, dtype=F32, **v):
    """downscaleSum: ((p1 + p2) + p3) + p4"""
    with np.errstate(all="ignore"):
        return _sum4(_gather4(np.asarray(a, F32).astype(dtype), v.get("swap", False)), v.get("assoc", "seq"))


def downscale_avg(a, dtype=F32, **v):
    """downscaleAverage / bcd_hip_downscale_avg: 0.25 * (((p1 + p2) + p3) + p4), p1 = (2l, 2c), p2 = next line, p3 = next column, p4 = both, clamped"""
    with np.errstate(all="ignore"):
        return (dtype(0.25) * downscale_sum(a, dtype, **v)).astype(dtype)


def downscale_cov_terms(cov, ns, dtype=F32, **v):
    """the four products w_i * cov_i of downscaleSampleCovarianceSum, w_i = (1/16) * nSum / n_i"""
    with np.errstate(all="ignore"):
        n = _gather4(np.asarray(ns, F32).astype(dtype), v.get("swap", False))
        c = _gather4(np.asarray(cov, F32).astype(dtype), v.get("swap", False))
        sq = dtype(1.0 / 4.0) * dtype(1.0 / 4.0)
        nsum = _sum4(n, v.get("assoc", "seq"))
        w = [sq * nsum / ni for ni in n]
        if "w_from" in v:
            w = [w[i] for i in v["w_from"]]
        return w, c


def downscale_cov(cov, ns, dtype=F32, **v):
    with np.errstate(all="ignore"):
        w, c = downscale_cov_terms(cov, ns, dtype, **v)
        if v.get("fma", False):
            acc = w[0] * c[0]
            for i in (1, 2, 3):
                acc = _fma(np.broadcast_to(w[i], c[i].shape), c[i], acc)
            return acc
        return _sum4([wi * ci for wi, ci in zip(w, c)], v.get("assoc", "seq"))


# ---- interpolation and merge ----------------------------------------------------------------------------------------------------------------------
def interpolate_terms(lo, H, W, dtype=F32, **v):
    """-> (weights, [main, column neighbour, line neighbour, diagonal]) of every fine pixel"""
    lo = np.asarray(lo, F32).astype(dtype)
    h, w = lo.shape[0], lo.shape[1]
    lc, al = interp_index(H, h, v.get("parity", 1), v.get("clamp", "clamp"))
    cc, ac = interp_index(W, w, v.get("parity", 1), v.get("clamp", "clamp"))
    return (dtype(9.0 / 16.0), dtype(3.0 / 16.0), dtype(1.0 / 16.0)), [lo[lc][:, cc], lo[lc][:, ac], lo[al][:, cc], lo[al][:, ac]]


def interpolate(lo, H, W, dtype=F32, **v):
    """interpolate: (wm * p1 + wa * (p2 + p3)) + wd * p4 with wm, wa, wd = 9/16, 3/16, 1/16 (exact in float32)"""
    with np.errstate(all="ignore"):
        (wm, wa, wd), p = interpolate_terms(lo, H, W, dtype, **v)
        if v.get("fma", False):
            return _fma(np.broadcast_to(wd, p[3].shape), p[3], _fma(np.broadcast_to(wa, p[0].shape), p[1] + p[2], wm * p[0]))
        if not v.get("presum", True):
            return ((wm * p[0] + wa * p[1]) + wa * p[2]) + wd * p[3]
        return (wm * p[0] + wa * (p[1] + p[2])) + wd * p[3]


def merge(hi, lo, dtype=F32, **v):
    """mergeOutputs: hi -= up(down(hi)); hi += up(lo)"""
    with np.errstate(all="ignore"):
        hi = np.asarray(hi, F32).astype(dtype)
        H, W = hi.shape[0], hi.shape[1]
        a = interpolate(downscale_avg(hi, dtype, **v), H, W, dtype, **v)
        b = interpolate(lo, H, W, dtype, **v)
        if v.get("merge_order") == "add_first":
            return (hi + b) - a
        return (hi - a) + b


def merge_abs_terms(hi, lo):
    """float64 sum of the absolute terms of merge: |hi| + up(down(|hi|)) + up(|lo|)  (every weight is positive)"""
    ah, al_ = np.abs(np.asarray(hi, F64)), np.abs(np.asarray(lo, F64))
    H, W = ah.shape[0], ah.shape[1]
    return ah + interpolate(downscale_avg(ah, F64), H, W, F64) + interpolate(al_, H, W, F64)


# ---- the per-pixel passes -------------------------------------------------------------------------------------------------------------------------
def pixel_cov(cov, ns, dtype=F32, **v):
    """computePixelCovFromSampleCov: cov * (1 / n); cov (..., 6), ns (..., 1)"""
    with np.errstate(all="ignore"):
        cov, ns = np.asarray(cov, F32).astype(dtype), np.asarray(ns, F32).astype(dtype)
        if v.get("divide", False):
            return cov / ns
        return cov * (dtype(1.0) / ns)


def finalize(s, cnt, dtype=F32, **v):
    """finalAggregation: (1 / (float)count) * sum; s (..., 3), cnt (...) int32.  float64: the count is exact, float32: it rounds above 2^24"""
    with np.errstate(all="ignore"):
        s = np.asarray(s, F32).astype(dtype)
        c = np.asarray(cnt, np.int32).astype(dtype)[..., None]
        if v.get("divide", False):
            return s / c
        return (dtype(1.0) / c) * s


def zero_bad(a):
    """checkAndPutToZeroNegativeInfNaNValues: v < 0, NaN and +-inf become +0; -0.0 is not below zero and stays, a negative denormal is and goes"""
    a = np.array(a, F32)
    with np.errstate(all="ignore"):
        a[(a < 0) | np.isnan(a) | np.isinf(a)] = F32(0.0)
    return a


def run(op, inputs, dtype=F32, **v):
    """one entry for the case tables: op in dsum, davg, dcov, interp (inputs: lo, H, W), merge, pixcov, finalize"""
    f = {"dsum": downscale_sum, "davg": downscale_avg, "dcov": downscale_cov, "interp": interpolate, "merge": merge, "pixcov": pixel_cov, "finalize": finalize}[op]
    return f(*inputs, dtype=dtype, **v)


def bits_differ(a, b):
    """does any element differ in its bits (NaN against NaN counts as equal)?"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return bool(np.any((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))))
