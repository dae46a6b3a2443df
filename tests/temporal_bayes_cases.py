"""Constructed inputs for the estimate over members of several frames (bcd_hip_bayes_accumulate_temporal; tests/test_gpu_temporal_stage.py and
tests/test_temporal_cases_cpu.py).  TEST INFRASTRUCTURE, in the manner of tests/bayes_cases.py, whose frames and set builders it uses.

A case is 1 + F frames of one smooth signal under independent noise (colours and the per-pixel covariances the noise was drawn with), and per processed
pixel one similar set per frame: the in-frame set and F cross sets, each a subset of the pixel's clipped window.  The processed pixels of an ISOLATED case
lie 2 (b + w) + 1 apart, so sum / count at the pixels an item touches are that item's own aggregate; in the DENSE case every main pixel is processed."""
import numpy as np

import bayes_cases as bc
import bayes_ref as br

W_, B_ = 1, 6
FULLW = (2 * B_ + 1) ** 2          # 169
K1 = 3 * (2 * W_ + 1) ** 2 + 1     # 28


class Case:
    def __init__(self, name, frames, sets, min_eig=1e-8, dense=False):
        """frames: list of (col, pixcov), [0] the frame itself; sets: {(l, c): [positions in frame 0, in frame 1, ...]}, each (n_f, 2)"""
        H, W, _ = frames[0][0].shape
        words = (FULLW + 31) // 32
        self.name, self.w, self.b, self.min_eig, self.dense = name, W_, B_, float(min_eig), dense
        self.col = [np.ascontiguousarray(c, np.float32) for c, _ in frames]
        self.pixcov = [np.ascontiguousarray(p, np.float32) for _, p in frames]
        self.mask = [np.zeros((H, W, words), np.uint32) for _ in frames]
        self.state = np.zeros((H, W), np.uint8)
        for (l, c), per_frame in sets.items():
            assert len(per_frame) == len(frames) and 1 <= l <= H - 2 and 1 <= c <= W - 2
            for f, pos in enumerate(per_frame):
                pos = np.asarray(pos, np.int64).reshape(-1, 2)
                assert (pos[:, 0] >= 1).all() and (pos[:, 0] <= H - 2).all() and (pos[:, 1] >= 1).all() and (pos[:, 1] <= W - 2).all()
                self.mask[f][l, c] = br.encode_members(pos, l, c, B_)    # bits only for main pixels inside the window, as the mask kernels guarantee
            self.state[l, c] = 1
        self.nsim_total = sum(br.popcount(m) for m in self.mask).astype(np.int32)
        if not dense:
            pts = np.array(sorted(sets))
            for i in range(len(pts) - 1):                                # isolation: no two items share an input or an output pixel
                assert np.abs(pts[i + 1:] - pts[i]).max(axis=1).min() >= 2 * (B_ + W_) + 1, (name, pts[i])

    @property
    def F(self):
        return len(self.col) - 1

    def frames(self):
        return [(self.col[f], self.pixcov[f], self.mask[f]) for f in range(len(self.col))]

    def args(self):
        return self.frames(), self.nsim_total, self.state, self.w, self.b, self.min_eig


def make_frames(H, W, rng, F, amp=1.0, zero_noise=False):
    out = []
    for _ in range(F + 1):
        col, pc = bc.noisy_frame(H, W, rng, amp=amp)
        out.append((col, np.zeros_like(pc) if zero_noise else pc))
    return out


def split(total, F, cap, rng):
    """`total` members over F frames, at most `cap` each"""
    assert 0 <= total <= F * cap
    parts = [0] * F
    left = total
    for f in range(F):
        rest_cap = (F - 1 - f) * cap
        lo, hi = max(0, left - rest_cap), min(cap, left)
        parts[f] = hi if f == F - 1 else int(rng.integers(lo, hi + 1))
        left -= parts[f]
    assert left == 0
    return parts


def with_centre(win, n, l, c, rng):
    """n window positions that include the pixel itself"""
    if n <= 0:
        return win[:0]
    centre = np.nonzero((win[:, 0] == l) & (win[:, 1] == c))[0]
    rest = rng.permutation(np.setdiff1d(np.arange(len(win)), centre))[:n - 1]
    return win[np.sort(np.concatenate([centre, rest]))]


# |S_0| crossed with the total |S|: 27 (the largest fallback), 28 (the smallest full estimate), 29, 170 and every window full
S0_SIZES = (1, 5, 27, 28, 169)


def totals(F):
    return (27, 28, 29, 170, FULLW * (1 + F))


def fam_sizes(F, seed):
    rng = np.random.default_rng(seed)
    H, W = 70, 100
    frames = make_frames(H, W, rng, F)
    combos = [(s0, t) for s0 in S0_SIZES for t in totals(F) if s0 <= t and t - s0 <= F * FULLW]
    pts = bc.grid(H, W, W_, B_)
    assert len(combos) <= len(pts)
    sets = {}
    for (l, c), (s0, t) in zip(pts, combos):
        win = bc.window(l, c, H, W, W_, B_)
        sets[(l, c)] = [with_centre(win, s0, l, c, rng)] + [bc.subset(win, k, rng) for k in split(t - s0, F, FULLW, rng)]
    return Case("sizes F=%d" % F, frames, sets)


def fam_borders():
    """windows leaving the image: every frame's set is the part of the window inside the frame, fully set"""
    rng = np.random.default_rng(212)
    H, W = 70, 100
    frames = make_frames(H, W, rng, 2)
    out = []
    for k in (0, 3):
        sets = {p: [bc.window(p[0], p[1], H, W, W_, B_)] * 3 for p in bc.border_points(H, W, k)}
        out.append(Case("borders line %d F=2" % k, frames, sets))
    return out


def fam_centre_only():
    """the only in-frame member is the pixel itself: full estimates (and one fallback) that live on the neighbours' statistics"""
    rng = np.random.default_rng(213)
    H, W = 40, 100
    frames = make_frames(H, W, rng, 2)
    sets = {}
    for i, (l, c) in enumerate(bc.grid(H, W, W_, B_)):
        win = bc.window(l, c, H, W, W_, B_)
        n1, n2 = ((20, 6), (27, 0), (60, 40), (169, 169), (0, 90), (100, 0))[i % 6]
        sets[(l, c)] = [np.array([[l, c]]), bc.subset(win, n1, rng), bc.subset(win, n2, rng)]
    return Case("centre only F=2", frames, sets)


def fam_pure_noise():
    rng = np.random.default_rng(214)
    H, W = 40, 100
    frames = make_frames(H, W, rng, 2, amp=0.0)
    sets = {}
    for i, (l, c) in enumerate(bc.grid(H, W, W_, B_)):
        win = bc.window(l, c, H, W, W_, B_)
        n = (169, 40)[i % 2]
        sets[(l, c)] = [with_centre(win, n, l, c, rng), bc.subset(win, n, rng), bc.subset(win, 169 - n + 10, rng)]
    return Case("pure noise F=2", frames, sets)


def fam_zero_noise():
    """noise mean 0: C - N = C, the floor decides the inverses"""
    rng = np.random.default_rng(215)
    H, W = 40, 100
    frames = make_frames(H, W, rng, 1, zero_noise=True)
    sets = {}
    for i, (l, c) in enumerate(bc.grid(H, W, W_, B_)):
        win = bc.window(l, c, H, W, W_, B_)
        n0, n1 = ((28, 20), (100, 100), (10, 60))[i % 3]
        sets[(l, c)] = [with_centre(win, n0, l, c, rng), bc.subset(win, n1, rng)]
    return Case("zero noise F=1", frames, sets)


def fam_non_finite():
    """a NaN / inf covariance at ONE member pixel of a neighbour frame: the whole item is NaN (the noise mean is non-finite), its neighbours on the grid are
    untouched; one fallback item has such a member too and stays finite (the fallback reads no covariance)"""
    rng = np.random.default_rng(216)
    H, W = 40, 100
    frames = make_frames(H, W, rng, 2)
    sets = {}
    pts = bc.grid(H, W, W_, B_)
    for i, (l, c) in enumerate(pts):
        win = bc.window(l, c, H, W, W_, B_)
        n0, n1, n2 = ((40, 40, 40), (5, 10, 5), (169, 169, 169))[i % 3]
        sets[(l, c)] = [with_centre(win, n0, l, c, rng), bc.subset(win, n1, rng), bc.subset(win, n2, rng)]
    for i, bad in ((0, np.nan), (1, np.nan), (2, np.inf)):
        f = 1 + i % 2
        l, c = sets[pts[i]][f][len(sets[pts[i]][f]) // 2]
        frames[f][1][l, c, i % 6] = bad
    return Case("non-finite covariance in a neighbour F=2", frames, sets)


FAMILIES = {
    "sizes F=1": lambda: [fam_sizes(1, 201)],
    "sizes F=2": lambda: [fam_sizes(2, 202)],
    "sizes F=4": lambda: [fam_sizes(4, 204)],
    "borders": fam_borders,
    "centre only": lambda: [fam_centre_only()],
    "pure noise": lambda: [fam_pure_noise()],
    "zero noise": lambda: [fam_zero_noise()],
    "non-finite": lambda: [fam_non_finite()],
}


def dense_case(H, W, F, seed, name):
    """every main pixel processed, random sets in every frame (full estimates and fallbacks mixed): atomics from many items on one pixel"""
    rng = np.random.default_rng(seed)
    frames = make_frames(H, W, rng, F)
    sets = {}
    for l in range(1, H - 1):
        for c in range(1, W - 1):
            win = bc.window(l, c, H, W, W_, B_)
            sizes = [int(rng.choice((3, 12, 30, 80, 169))) for _ in range(F + 1)]
            sets[(l, c)] = [with_centre(win, min(sizes[0], len(win)), l, c, rng)] + [bc.subset(win, s, rng) for s in sizes[1:]]
    return Case(name, frames, sets, dense=True)


def call_sequence():
    """four calls on one context: a few isolated items, a dense frame (many items: other list lengths, records regrown), the isolated items again, a dense
    frame of another size and frame count"""
    a = fam_sizes(1, 301)
    return [a, dense_case(34, 40, 1, 302, "dense 40x34 F=1"), a, dense_case(30, 26, 2, 303, "dense 26x30 F=2")]


def single_frame_of(case):
    """the frame-0 part of a case in the terms of bcd_hip_bayes_accumulate / bayes_ref.accumulate: (col, pixcov, mask, nsim, state, w, b, min_eig)"""
    return case.col[0], case.pixcov[0], case.mask[0], br.popcount(case.mask[0]), case.state, case.w, case.b, case.min_eig
