"""Constructed similarity graphs for the marking stage (tests/test_gpu_marking_stage.py).  TEST INFRASTRUCTURE.

The marking kernels read three plain tensors: the window masks, |S| (`cnt`, only ever as cnt[q] >= 3 (2w+1)^2 + 1) and the state image.  Natural
masks are blobs; these are graphs built to reach what blobs never reach under control: one window offset on its own, chains as long as the frame is
wide, |S| exactly at the threshold on chosen pixels, frames narrower than a tile, the word-boundary bits of the window.

Contract of every case (tests/test_marking_cases_cpu.py holds the generators to it): masks are symmetric -- bit (dl, dc) of p is set iff bit
(-dl, -dc) of p + (dl, dc) is set --, no bit points outside the main area, pixels outside the main area have an empty mask and cnt 0.  `cnt` is the
popcount unless the family says it is free (`popcount` false).

Frame sizes sit around the 16 x 16 tile of the listed kernels and its b-wide halo: one main pixel, one tile, a ragged tile in either direction, a
tile edge, a frame narrower than a tile, a complete window."""
import collections

import numpy as np

import marking_ref as mr

Case = collections.namedtuple("Case", "name W H w b mask cnt family popcount depth ms")

SIZES = [(3, 3), (16, 16), (17, 16), (16, 33), (33, 18), (15, 40), (5, 40)]
SIZES_B12 = [(41, 30), (30, 41)]
RADII = (1, 3, 8, 6, 12)          # 1, 3, 8: the generic kernel; 6, 12: dependency lists + tile rounds
ALL_M = (0.0, 0.25, 0.5, 1.0)


def sizes(b):
    return SIZES_B12 if b == 12 else SIZES


def window(b):
    side = 2 * b + 1
    return side, side * side, (side * side - 1) // 2


def offset(k, b):
    side = 2 * b + 1
    return k // side - b, k % side - b


def pair_count(b):
    """pairs (k, mirrored k) of the window: 84 at b = 6, 312 at b = 12"""
    return window(b)[2]


def _shifted(a, dl, dc):
    """a[l + dl, c + dc] at (l, c), False outside"""
    H, W = a.shape
    out = np.zeros_like(a)
    l0, l1, c0, c1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)
    if l0 < l1 and c0 < c1:
        out[l0:l1, c0:c1] = a[l0 + dl:l1 + dl, c0 + dc:c1 + dc]
    return out


def symmetric_bits(W, H, w, b, half):
    """(H, W, (2b+1)^2) bool from `half(k)` -> (H, W) bool for the offsets k before the centre: the pair (p, p + offset(k)) is similar where half(k) is
    set at p and both are main pixels; the mirrored bit goes to the neighbour, the centre bit to every main pixel"""
    side, n, kc = window(b)
    main = mr.main_area(W, H, w)
    bits = np.zeros((H, W, n), bool)
    bits[:, :, kc] = main
    for k in range(kc):
        h = half(k)
        if h is None:
            continue
        dl, dc = offset(k, b)
        e = np.asarray(h, bool) & main & _shifted(main, dl, dc)
        bits[:, :, k] = e
        bits[:, :, n - 1 - k] = _shifted(e, -dl, -dc)
    return bits


def _case(name, W, H, w, b, bits, family, cnt=None, depth=None, ms=(1.0,)):
    popcount = cnt is None
    if popcount:
        cnt = bits.sum(-1)
    cnt = np.where(mr.main_area(W, H, w), cnt, 0).astype(np.int32)
    return Case(name, W, H, w, b, mr.pack(bits), cnt, family, popcount, depth, tuple(ms))


def fit_w(W, H, w):
    """the largest patch radius <= w that leaves a main pixel"""
    while w > 0 and (W <= 2 * w or H <= 2 * w):
        w -= 1
    return w


def free_cnt(W, H, w, strong=True):
    K1 = mr.strong_threshold(w)
    return np.full((H, W), K1 if strong else max(K1 - 1, 0), np.int32)


# ---- one offset at a time -------------------------------------------------------------------------------------------------
def one_offset(W, H, w, b, k):
    """every main pixel carries its centre bit and the pair (k, mirrored k) where that neighbour is a main pixel; cnt free, all strong.
    Written word by word (three bits per pixel): the loops over every pair of a window stay cheap"""
    side, n, kc = window(b)
    assert 0 <= k < kc
    main = mr.main_area(W, H, w)
    dl, dc = offset(k, b)
    e = main & _shifted(main, dl, dc)
    mask = np.zeros((H, W, (n + 31) // 32), np.uint32)
    for kk, a in ((kc, main), (k, e), (n - 1 - k, _shifted(e, -dl, -dc))):
        mask[:, :, kk >> 5] |= a.astype(np.uint32) << np.uint32(kk & 31)
    cnt = np.where(main, free_cnt(W, H, w), 0).astype(np.int32)
    return Case("one offset b=%d k=%d %dx%d w=%d" % (b, k, W, H, w), W, H, w, b, mask, cnt, "one offset", False, None, (1.0,))


ONE_OFFSET_FRAMES = {3: (33, 18, 1), 8: (33, 18, 1), 6: (33, 18, 1), 12: (41, 30, 1)}   # b -> (W, H, w): a tile boundary in both directions


# ---- the families ---------------------------------------------------------------------------------------------------------
def random_graph(W, H, w, b, density, seed, name=None):
    rng = np.random.default_rng(seed)
    bits = symmetric_bits(W, H, w, b, lambda k: rng.random((H, W)) < density)
    return _case(name or "random %.2f b=%d %dx%d w=%d" % (density, b, W, H, w), W, H, w, b, bits, "random", ms=ALL_M)


def full_window(W, H, w, b):
    bits = symmetric_bits(W, H, w, b, lambda k: np.ones((H, W), bool))
    return _case("full b=%d %dx%d w=%d" % (b, W, H, w), W, H, w, b, bits, "full", ms=ALL_M)


def threshold(W, H, w, b, density, pattern, seed):
    """full (density None) or random masks, cnt exactly K or K + 1 (K + 1 = 3 (2w+1)^2 + 1 is the weakest strong pixel) in a checkerboard or a
    seeded random pattern; cnt free"""
    rng = np.random.default_rng(seed)
    bits = symmetric_bits(W, H, w, b, (lambda k: np.ones((H, W), bool)) if density is None else (lambda k: rng.random((H, W)) < density))
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    strong = ((l + c) & 1) == 0 if pattern == "checker" else rng.random((H, W)) < 0.5
    cnt = mr.strong_threshold(w) - 1 + strong.astype(np.int32)
    return _case("threshold %s %s b=%d %dx%d w=%d" % ("full" if density is None else "random", pattern, b, W, H, w), W, H, w, b, bits, "threshold", cnt=cnt)


def _k_of(dl, dc, b):
    return (dl + b) * (2 * b + 1) + (dc + b)


def chain(W, H, w, b, kind):
    """every pixel similar to its two neighbours along a line only, all strong, cnt free.  `depth`: the longest run of pixels each of which has to
    wait for the one before it under the scanline order"""
    left, up = _k_of(0, -1, b), _k_of(-1, 0, b)
    Wm, Hm = W - 2 * w, H - 2 * w
    if kind == "horizontal":
        half, depth = (lambda k: np.ones((H, W), bool) if k == left else None), Wm
    elif kind == "vertical":
        half, depth = (lambda k: np.ones((H, W), bool) if k == up else None), Hm
    else:                                                            # serpentine: the rows joined end to end, at the right and the left end in turn
        join = np.zeros((H, W), bool)
        for r in range(w + 1, H - w):
            join[r, (W - 1 - w) if (r - 1 - w) % 2 == 0 else w] = True
        half = lambda k: np.ones((H, W), bool) if k == left else (join if k == up else None)
        # scanline order: a row is waited for from its left end whichever end it is joined at, and a join at the right end adds the row
        # above's last pixel in front of this row's last one: Wm + 1 after one such join, Wm + 2 from the second on
        depth = Wm + (0 if Hm < 2 else 1 if Hm < 4 else 2)
    bits = symmetric_bits(W, H, w, b, half)
    return _case("chain %s b=%d %dx%d w=%d" % (kind, b, W, H, w), W, H, w, b, bits, "chain", cnt=free_cnt(W, H, w), depth=depth, ms=ALL_M)


def isolated(W, H, w, b, strong):
    bits = symmetric_bits(W, H, w, b, lambda k: None)
    return _case("isolated %s b=%d %dx%d w=%d" % ("strong" if strong else "weak", b, W, H, w), W, H, w, b, bits, "isolated", cnt=free_cnt(W, H, w, strong))


_cases = None


def cases():
    """every case but the one-offset loops (those are generated pair by pair where they are used)"""
    global _cases
    if _cases is not None:
        return _cases
    out, i = [], 0
    for b in RADII:
        for (W, H) in sizes(b):
            w = fit_w(W, H, (1, 0, 2)[(i // 3) % 3])
            out.append(random_graph(W, H, w, b, (0.02, 0.3, 0.9)[i % 3], 1000 + i))
            out.append(full_window(W, H, fit_w(W, H, (0, 1, 2)[i % 3]), b))
            i += 1
    out.append(random_graph(33, 18, 1, 6, 0.3, 77, "random 0.30 b=6 33x18 w=1 (bands)"))
    for (W, H, w, b, density) in [(16, 16, 1, 6, 0.02), (15, 40, 1, 6, 0.3), (33, 18, 1, 6, 0.9), (41, 30, 1, 12, 0.02)]:   # the default geometry at every density
        out.append(random_graph(W, H, w, b, density, 1500 + len(out)))
    out.append(full_window(17, 16, 1, 1))                            # b = 1, w = 1: no pixel can reach 28, nothing is ever marked
    for (W, H, w, b, density) in [(33, 18, 1, 6, None), (16, 33, 1, 3, 0.3), (17, 16, 0, 1, None), (41, 30, 2, 12, 0.3), (15, 40, 2, 8, None)]:
        for pattern in ("checker", "seeded"):
            out.append(threshold(W, H, w, b, density, pattern, 2000 + len(out)))
    for (W, H, w, b, kind) in [(130, 20, 1, 6, "horizontal"), (300, 18, 1, 6, "horizontal"), (18, 130, 1, 6, "vertical"), (40, 24, 1, 6, "serpentine"),
                               (130, 20, 1, 3, "horizontal"), (18, 130, 1, 12, "vertical"), (40, 24, 0, 1, "serpentine"), (130, 20, 2, 12, "horizontal")]:
        out.append(chain(W, H, w, b, kind))
    for (W, H, w, b, strong) in [(33, 18, 1, 6, True), (33, 18, 1, 6, False), (17, 16, 0, 3, True), (30, 41, 2, 12, False)]:
        out.append(isolated(W, H, w, b, strong))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), "case names are ids"
    _cases = out
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def orders(case):
    """(order mode, seed) pairs a case is run under: scanline (every hash ties: the k < centre tie-break), the seeded random order under two
    seeds (bcd_mix32 is a bijection: no ties), and the strip order where the frame has more than one strip of 2b lines"""
    out = [(0, 0), (1, 11), (1, 4242)]
    if case.H - 2 * case.w > 2 * case.b:
        out.append((2, 0))
    return out


def visit(case, mode, seed):
    """the visiting order of the case's main pixels from the library's host-side key (bcd_hip_visit_order; strip order: the geometry travels in the seed)"""
    import bcd_amd.hip as bh
    return bh.visit_order(case.W, case.H, case.w, mode, bh.strip_order_seed(case.W, case.H, case.w, case.b) if mode == 2 else seed)


_ref_cache = {}


def reference(case, mode, seed, m, skip_seed=None):
    """marking_ref.greedy of a case, computed once per (case, order, m) and handed out read-only"""
    key = (case.name, mode, seed, m, skip_seed)
    if key not in _ref_cache:
        drawn = mr.skip_draw(case.W, case.H, m, seed if skip_seed is None else skip_seed)
        st = mr.greedy(case.mask, case.cnt, case.w, case.b, visit(case, mode, seed), drawn)
        st.setflags(write=False)
        _ref_cache[key] = st
    return _ref_cache[key]
