"""The constructed inputs of the pyramid and per-pixel kernel tests (tests/test_pyramid_cases_cpu.py holds them to what they claim,
tests/test_gpu_pyramid_stage.py runs them on the device).  Restatements and mutants: tests/pyramid_ref.py.

Which kernel of bcd_amd/csrc/k_pointwise.hip a case reaches is decided by the launchers from the depth D, the pixel count and the alignment:

    operation              depths D                  kernel / branch
    downscale_sum / _avg   4, 8, 12, 60              k_downscale4<0> / <1>, Q = 1, 2, 3, 15 (16-byte aligned images)
                           1, 2, 3, 5, 6, 7          k_downscale_px<0> / <1>
                           9, 15                     k_downscale<0> / <1> (per value)
                           4, 8 | 12, 60, one float  k_downscale_px | k_downscale: the alignment guard (input, output or both offset by 4 bytes)
    downscale_cov          6                         k_downscale_cov_px
    interpolate            1 ... 8                   k_interpolate_px<0>
                           9, 12, 15, 60             k_interpolate<0> (per value)
    merge / merge_         1 ... 8                   the downscale kernel of the depth, then k_merge_px
                           9, 12, 15, 60             the downscale kernel of the depth, then k_interpolate<1> + k_interpolate<2>
    pixel_cov              npix of FLAT              k_pixel_cov
    scale_begin            npix = 1                  k_pixel_cov_clear (no pair)
                           npix = 2, 256             k_pixel_cov_clear2
                           npix = 9, 255, 257        k_pixel_cov_clear2 + the one-pixel tail by k_pixel_cov_clear
                           any buffer off by 4 bytes k_pixel_cov_clear: the alignment guard
    finalize               npix of FLAT              k_finalize_px
    zero_bad_values        n = 1, 255, 256, 257      k_zero_bad

Every depth of DEPTHS runs at every size of SIZES (W x H), so each branch above meets

    2x2, 3x2, 2x3, 3x3   the coarse level is one pixel wide and / or high: clamp_pos folds both neighbours onto the main pixel
    4x4, 5x4             the smallest levels with two coarse pixels per axis; 5 is odd: the last column belongs to no block
    33x32, 34x31, 35x33  coarse levels of exactly 256, of 255 and of 272 pixels: on, below and above one 256-thread block
    23x11                a fine level of 253 pixels, both sides odd

and FLAT = 1, 2, 9, 255, 256, 257 pixels for the flat per-pixel kernels.  Three value families per (size, depth):

    index      (2^18 + 512 l + c) 2^(z - 30): every (l, c, z) distinct, the four-term sums and the interpolation exact, so that an output decodes to the
               line and column sums of its (weighted) sources (`decode`) -- a wrong source pixel, a missed clamp, a wrong channel give another number
    order      seeded, magnitudes 2^-12 ... 2^12 with full mantissas and both signs; the levels are redrawn block by block until EVERY output value
               differs under every other association (mutants pairwise, right, swap); the coarse images of interpolate, the (fine, coarse) pairs of
               merge and the covariances are taken from the first seed under which every mutant named for the case changes a bit: any other
               association, or a fused multiply-add, rounds differently
    nonfinite  the order level with NaN, +inf, -inf and -0.0 at the four corners, on two borders and in the interior

Mutants (pyramid_ref.MUTANTS) are named for a case by `named`: the association, fma, no_presum, merge_order, w_wrong and divide mutants on the order
family (on the index family the arithmetic is exact and every association gives the same bits); clamp_wrap, clamp_last and parity on the index and
order families wherever the coarse level has two pixels along an axis (with one pixel every rule folds onto it).  Sample counts of downscale_cov:
"mixed" (3, 5, 8, 37 times a power of two: the four counts of a block differ) and "zero" (a 0 in a block: nSum / 0 = inf, an all-zero block: 0 / 0)."""
import zlib

import numpy as np

import pyramid_ref as pr

F32 = np.float32
SIZES = [(2, 2), (3, 2), (2, 3), (3, 3), (4, 4), (5, 4), (33, 32), (34, 31), (35, 33), (23, 11)]
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 60]
FLAT = [1, 2, 9, 255, 256, 257]
FAMILIES = ("index", "order", "nonfinite")
COUNT_KINDS = ("mixed", "zero")
FINALIZE_COUNTS = (0, 1, 3, (1 << 24) + 1)
ZERO_BAD_LENGTHS = (1, 255, 256, 257)

# launcher branch -> (operation, depths that take it); the CPU test asks for a catching case per (branch, mutant of the operation)
BRANCHES = {
    "k_downscale4<0>": ("dsum", (4, 8, 12, 60)), "k_downscale4<1>": ("davg", (4, 8, 12, 60)),
    "k_downscale_px<0>": ("dsum", (1, 2, 3, 5, 6, 7)), "k_downscale_px<1>": ("davg", (1, 2, 3, 5, 6, 7)),
    "k_downscale<0>": ("dsum", (9, 15)), "k_downscale<1>": ("davg", (9, 15)),
    "k_downscale_cov_px": ("dcov", (6,)),
    "k_interpolate_px<0>": ("interp", (1, 2, 3, 4, 5, 6, 7, 8)), "k_interpolate<0>": ("interp", (9, 12, 15, 60)),
    "k_merge_px": ("merge", (1, 2, 3, 4, 5, 6, 7, 8)), "k_interpolate<1> + k_interpolate<2>": ("merge", (9, 12, 15, 60)),
    "k_pixel_cov / k_pixel_cov_clear / k_pixel_cov_clear2": ("pixcov", (6,)),
    "k_finalize_px": ("finalize", (3,)),
}

_cache = {}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def order_values(rng, shape, exponent=None):
    """sign * (1 + m / 2^23) * 2^e, m uniform in [0, 2^23), e uniform in [-12, 12] (or `exponent` - 1 ... + 1): exact float32 numbers with full mantissas"""
    m = rng.integers(0, 1 << 23, size=shape).astype(np.float64)
    e = (rng.integers(-12, 13, size=shape) if exponent is None else exponent + rng.integers(-1, 2, size=shape)).astype(np.float64)
    s = rng.integers(0, 2, size=shape).astype(np.float64) * 2.0 - 1.0
    return (s * (1.0 + m / float(1 << 23)) * np.exp2(e)).astype(F32)


# ---- the index-coded family ---------------------------------------------------------------------------------------------------------------------------
CODE_ONE, CODE_LINE, CODE_Z0 = 1 << 18, 1 << 9, 30


def index_image(W, H, D):
    l, c, z = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    return ((CODE_ONE + CODE_LINE * l + c).astype(np.float64) * np.exp2(z - CODE_Z0)).astype(F32)


def decode(out, scale, total):
    """an output of a linear operation on an index image, out = (sum of w_i code_i) / scale with whole weights w_i that add up to `total` (a sum of four:
    scale 1, total 4; their average: scale 4, total 4; the interpolation: scale 16, weights 9, 3, 3, 1) -> (sum of w_i line_i, sum of w_i column_i) per
    element; raises if an element is no such combination of codes of its own channel"""
    D = out.shape[-1]
    m = out.astype(np.float64) * float(scale) * np.exp2(CODE_Z0 - np.arange(D)) - float(total * CODE_ONE)
    if not (np.all(m == np.rint(m)) and np.all(m >= 0) and np.all(m < CODE_ONE)):
        raise ValueError("not a combination of index codes of the element's channel")
    m = m.astype(np.int64)
    return m // CODE_LINE, m % CODE_LINE


# ---- the order-sensitive family -----------------------------------------------------------------------------------------------------------------------
ASSOCIATIONS = ("pairwise", "right", "swap")


def order_level(W, H, D):
    """an order-family level in which every 2x2 block sum differs, in its bits, under each mutant of ASSOCIATIONS (the blocks are disjoint: the sources
    of an output that ties under a mutant are drawn again, within a factor of four of one magnitude per block -- where one term dwarfs the others
    every association rounds alike -- and that magnitude uniform over 2^-11 ... 2^11)"""
    rng = np.random.default_rng(_seed("level", W, H, D))
    a = order_values(rng, (H, W, D))
    if W < 2 or H < 2:
        return a
    pos = pr.block_positions(W, H)
    src = [a[pos[..., k, 0], pos[..., k, 1]] for k in range(4)]               # p1 ... p4 of every output value, each (h2, w2, D)
    todo = np.nonzero(np.ones(src[0].shape, bool))
    for _ in range(400):
        p = [q[todo] for q in src]
        want = pr._sum4(p).view(np.uint32)
        tie = (pr._sum4(p, "pairwise").view(np.uint32) == want) | (pr._sum4(p, "right").view(np.uint32) == want) | \
              (pr._sum4([p[0], p[2], p[1], p[3]]).view(np.uint32) == want)
        todo = tuple(i[tie] for i in todo)
        if todo[0].size == 0:
            for k in range(4):
                a[pos[..., k, 0], pos[..., k, 1]] = src[k]
            return a
        e0 = rng.integers(-11, 12, size=todo[0].size)
        for k in range(4):
            src[k][todo] = order_values(rng, (todo[0].size,), e0)
    raise AssertionError("no order-sensitive level found for %dx%dx%d" % (W, H, D))


def _first_seed(tag, make, differs):
    for s in range(4096):
        x = make(np.random.default_rng(_seed(tag, s)))
        if differs(x):
            return x
    raise AssertionError("no seed makes every named mutant visible: %r" % (tag,))


def named(mutant, op, family, W, H):
    """is `mutant` required to change a bit of `op` on the case (family, W x H)?  family: a value family, or a sample-count kind for dcov"""
    if op not in pr.MUTANT_OPS[mutant]:
        return False
    if mutant in ("clamp_wrap", "clamp_last", "parity"):
        return family in ("index", "order") and max(W // 2, H // 2) >= 2
    if op == "dcov":
        return family == "mixed"
    return family == "order"


def _visible(op, family, W, H, inputs):
    want = pr.run(op, inputs)
    return all(pr.bits_differ(pr.run(op, inputs, **pr.MUTANTS[m]), want) for m in pr.MUTANTS if named(m, op, family, W, H))


def _nonfinite(a):
    a = a.copy()
    H, W, D = a.shape
    nan, inf, nz = F32(np.nan), F32(np.inf), F32(-0.0)
    spots = [(H // 2, W // 2, inf), (min(H // 2 + 1, H - 1), W // 2, nz), (H // 2, min(W // 2 + 1, W - 1), nan),    # interior
             (0, W // 2, -inf), (H // 2, 0, nan),                                                                 # borders
             (0, 0, nan), (0, W - 1, inf), (H - 1, 0, -inf), (H - 1, W - 1, nz)]                                   # corners (last: they win on a tiny level)
    for k, (l, c, v) in enumerate(spots):
        a[l, c, k % D] = v
    return a


def level(family, W, H, D):
    """the fine image of a case, H x W x D float32 (do not modify: shared)"""
    key = ("level", family, W, H, D)
    if key not in _cache:
        if family == "index":
            _cache[key] = index_image(W, H, D)
        elif family == "order":
            _cache[key] = order_level(W, H, D)
        else:
            _cache[key] = _nonfinite(level("order", W, H, D))
    return _cache[key]


def coarse(family, W, H, D):
    """the coarse image of an interpolate case, (H // 2) x (W // 2) x D"""
    key = ("coarse", family, W, H, D)
    if key not in _cache:
        h, w = H // 2, W // 2
        if family == "index":
            _cache[key] = index_image(w, h, D)
        elif family == "order":
            _cache[key] = _first_seed(key, lambda rng: order_values(rng, (h, w, D)), lambda lo: _visible("interp", "order", W, H, (lo, H, W)))
        else:
            _cache[key] = _nonfinite(coarse("order", W, H, D))
    return _cache[key]


def merge_pair(family, W, H, D):
    """(fine image, coarse image) of a merge case.  The order family draws a pair of its own: whether another association of the average survives the
    two outer operations depends on the fine image, and on a level of four pixels few pairs show ALL mutants of merge at once"""
    key = ("merge", family, W, H, D)
    if key not in _cache:
        h, w = H // 2, W // 2
        if family == "index":
            _cache[key] = (index_image(W, H, D), index_image(w, h, D))
        elif family == "order":
            # (up to 64 values: both images within a factor of four of one magnitude, drawn per seed -- see order_level)
            narrow = (lambda rng: int(rng.integers(-11, 12))) if W * H * D <= 64 else (lambda rng: None)

            def make(rng):
                e0 = narrow(rng)
                return order_values(rng, (H, W, D), e0), order_values(rng, (h, w, D), e0)
            _cache[key] = _first_seed(key, make, lambda pair: _visible("merge", "order", W, H, pair))
        else:
            _cache[key] = tuple(_nonfinite(a) for a in merge_pair("order", W, H, D))
    return _cache[key]


_COUNT_TABLE = np.array([[3, 5], [8, 37]], F32)


def sample_counts(kind, W, H):
    """H x W x 1: the four counts of every block differ (3, 5, 8, 37 by parity, times 2^(0 ... 3) per block); "zero": a 0 as p1 of the first block,
    as p4 of the last one, and -- where there are three blocks -- a block of four zeros"""
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ns = _COUNT_TABLE[l % 2, c % 2] * np.exp2(((l // 2) * 3 + (c // 2)) % 4).astype(F32)
    if kind == "zero":
        h2, w2 = H // 2, W // 2
        ns[0, 0] = 0
        ns[2 * h2 - 1, 2 * w2 - 1] = 0
        if w2 >= 3:
            ns[0:2, 2:4] = 0
    return np.ascontiguousarray(ns[..., None], F32)


def covariances(kind, W, H):
    """-> (cov H x W x 6, ns H x W x 1)"""
    key = ("cov", kind, W, H)
    if key not in _cache:
        ns = sample_counts(kind, W, H)
        _cache[key] = (_first_seed(key, lambda rng: order_values(rng, (H, W, 6)), lambda cov: _visible("dcov", kind, W, H, (cov, ns))), ns)
    return _cache[key]


# ---- the flat per-pixel cases -------------------------------------------------------------------------------------------------------------------------
def flat_covariances(npix):
    """-> (cov npix x 6, ns npix x 1): counts 3, 5, 8, 37, 1, 7, 24 in turn, a 0 on the last pixel where there are more than two"""
    key = ("flatcov", npix)
    if key not in _cache:
        ns = np.array([3, 5, 8, 37, 1, 7, 24], F32)[np.arange(npix) % 7].reshape(npix, 1)
        if npix > 2:
            ns[-1] = 0
        _cache[key] = (_first_seed(key, lambda rng: order_values(rng, (npix, 6)), lambda cov: _visible("pixcov", "order", 0, 0, (cov, ns))), ns)
    return _cache[key]


def finalize_case(npix, turn):
    """-> (sum npix x 3, count npix int32): the counts 0, 1, 3, 2^24 + 1 in turn starting at `turn` (so one pixel meets each), then seeded counts below 170
    with 7, 11 and 13 among them; the sum of a zero count is 0 on one channel (0 * inf)"""
    key = ("finalize", npix, turn)
    if key not in _cache:
        rng = np.random.default_rng(_seed(key))
        cnt = rng.integers(1, 170, size=npix).astype(np.int32)
        cnt[3::5] = np.array([7, 11, 13], np.int32)[np.arange(cnt[3::5].size) % 3]
        k = np.arange(npix)
        special = (k % 4 == 0) | (k >= npix - 4)                       # every fourth pixel and the last four, which hold the end of the last block
        cnt[special] = np.array(FINALIZE_COUNTS, np.int64)[(k[special] + turn) % 4].astype(np.int32)

        def make(r):
            s = order_values(r, (npix, 3))
            s[cnt == 0, 1] = 0
            return s
        _cache[key] = (_first_seed(key, make, lambda s: not divide_visible(cnt) or _visible("finalize", "order", 0, 0, (s, cnt))), cnt)
    return _cache[key]


def divide_visible(cnt):
    """can x / n differ from (1 / n) * x on these counts?  Not where every count is 0 or, as a float32, a power of two (2^24 + 1 rounds to 2^24)"""
    c = np.asarray(cnt, np.int32).astype(F32)
    return bool(np.any((c > 0) & (np.frexp(c)[0] != 0.5)))


ZERO_BAD_SPECIALS = np.array([
    0x00000000, 0x80000000,             # +0, -0 (kept: -0.0 < 0 is false)
    0x00000001, 0x80000001,             # +- the smallest denormal (the negative one is below zero: zeroed)
    0x00800000, 0x80800000,             # +- FLT_MIN
    0x7F7FFFFF, 0xFF7FFFFF,             # +- FLT_MAX
    0x7F800000, 0xFF800000,             # +- inf
    0x7FC00000, 0xFFC00000,             # quiet NaNs of both signs
    0x7F800001, 0xFFABCDEF, 0x7FFFFFFF, 0xFF800001,   # NaNs with payloads, signalling ones among them
    0x3FC00000, 0xBFC00000,             # +-1.5
    0x00200000, 0x80200000,             # +- a larger denormal
], np.uint32)


def zero_bad_vector(n, turn):
    """n values, as uint32 bits: the specials in turn starting at `turn`"""
    return ZERO_BAD_SPECIALS[(np.arange(n) + turn) % ZERO_BAD_SPECIALS.size].copy()


def pyramid_cases(families=FAMILIES, sizes=SIZES, depths=DEPTHS):
    """(op, family, W, H, D, inputs) of every pyramid case: dsum, davg, interp, merge at every depth, dcov at its two sample-count kinds"""
    for (W, H) in sizes:
        for fam in families:
            for D in depths:
                hi = level(fam, W, H, D)
                yield "dsum", fam, W, H, D, (hi,)
                yield "davg", fam, W, H, D, (hi,)
                yield "interp", fam, W, H, D, (coarse(fam, W, H, D), H, W)
                yield "merge", fam, W, H, D, merge_pair(fam, W, H, D)
        for kind in COUNT_KINDS:
            yield "dcov", kind, W, H, 6, covariances(kind, W, H)


def flat_cases():
    """(op, npix, inputs, is the divide mutant named?) of the flat cases with arithmetic: pixcov per npix, finalize per (npix, turn)"""
    for n in FLAT:
        yield "pixcov", n, flat_covariances(n), True
        for turn in range(4):
            s, cnt = finalize_case(n, turn)
            yield "finalize", n, (s, cnt), divide_visible(cnt)
