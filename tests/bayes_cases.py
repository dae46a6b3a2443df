"""Constructed inputs for the estimate kernels (test infrastructure only): colours, pixel covariances, similar sets, |S| and state images built
directly with seeded NumPy, family by family -- the situations the scene generator only meets by accident.  Shared by tests/test_bayes_ref_cpu.py
(the float32 calibrator must stay meaningful on every family) and tests/test_gpu_bayes_stage.py (the kernels against float64).

A family is a list of Case frames.  In an ISOLATED case the processed pixels lie 2 (b + w) + 1 apart in both directions: the windows, the member
patches and therefore the output pixels of two items never meet, sum / count at the pixels an item touches is that item's own aggregate.  In a
DENSE case every main pixel is processed (the -m 0 situation: many items add to one pixel)."""
import numpy as np

import bayes_ref

SIZES = (1, 9, 27, 28, 29, 32, 33, 63, 64, 65, 128, 168, 169)


class Case:
    def __init__(self, name, col, pixcov, sets, w=1, b=6, min_eig=1e-8, dense=False, judged=True):
        """sets: {(l, c): (n, 2) member positions}"""
        H, W, _ = col.shape
        side = 2 * b + 1
        self.name, self.w, self.b, self.min_eig, self.dense, self.judged = name, w, b, float(min_eig), dense, judged
        self.col = np.ascontiguousarray(col, np.float32)
        self.pixcov = np.ascontiguousarray(pixcov, np.float32)
        self.mask = np.zeros((H, W, (side * side + 31) // 32), np.uint32)
        self.state = np.zeros((H, W), np.uint8)
        for (l, c), pos in sets.items():
            pos = np.asarray(pos, np.int64).reshape(-1, 2)
            assert w <= l <= H - 1 - w and w <= c <= W - 1 - w
            assert (pos[:, 0] >= w).all() and (pos[:, 0] <= H - 1 - w).all() and (pos[:, 1] >= w).all() and (pos[:, 1] <= W - 1 - w).all()
            self.mask[l, c] = bayes_ref.encode_members(pos, l, c, b)     # bits only for in-frame main pixels, as the mask kernels guarantee
            self.state[l, c] = 1
        self.nsim = bayes_ref.popcount(self.mask)
        if not dense:
            pts = np.array(sorted(sets))
            for i in range(len(pts)):                                    # isolation: no two items share an input or an output pixel
                d = np.abs(pts[i + 1:] - pts[i]).max(axis=1) if i + 1 < len(pts) else np.array([99])
                assert d.min() >= 2 * (b + w) + 1, (name, pts[i])

    def args(self):
        return self.col, self.pixcov, self.mask, self.nsim, self.state, self.w, self.b, self.min_eig

    def scaled(self, k, name):
        """colours x 2^k, covariances x 4^k, floor x 4^k: the same problem in other units"""
        o = Case.__new__(Case)
        o.__dict__.update(self.__dict__)
        o.name, o.col, o.pixcov, o.min_eig = name, self.col * np.float32(2.0 ** k), self.pixcov * np.float32(4.0 ** k), self.min_eig * 4.0 ** k
        return o


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------
def signal(H, W, amp=1.0):
    l, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([0.5 + 0.2 * amp * np.sin(l / 9.0 + c / 13.0), 0.4 + 0.2 * amp * np.cos(l / 11.0 - c / 17.0), 0.6 + 0.1 * amp * np.sin(c / 7.0)], -1)


def noise_model(H, W, rng, sigma=0.1):
    """per-pixel factors B (H, W, 3, 3) of full-rank noise covariances B B^T"""
    return sigma * (0.7 * np.eye(3) + 0.3 * rng.standard_normal((H, W, 3, 3)))


def cov6(B):
    S = np.einsum("...ik,...jk->...ij", B, B)
    return np.stack([S[..., 0, 0], S[..., 1, 1], S[..., 2, 2], S[..., 1, 2], S[..., 0, 2], S[..., 0, 1]], -1)


def noisy_frame(H, W, rng, sigma=0.1, amp=1.0):
    """smooth signal + noise drawn with exactly the covariance that pixcov states"""
    B = noise_model(H, W, rng, sigma)
    col = signal(H, W, amp) + np.einsum("...ij,...j->...i", B, rng.standard_normal((H, W, 3)))
    return col, cov6(B)


# ---- item placement and similar sets -----------------------------------------------------------------------------------------------------------
def grid(H, W, w, b):
    """isolated main pixels whose whole window is in the frame"""
    step, r = 2 * (b + w) + 1, b + w
    return [(l, c) for l in range(r, H - r, step) for c in range(r, W - r, step)]


def window(l, c, H, W, w, b):
    """the main pixels of the search window, clipped like DeepImage.hpp:181-196, window order"""
    return np.array([(ql, qc) for ql in range(max(w, l - b), min(H - 1 - w, l + b) + 1) for qc in range(max(w, c - b), min(W - 1 - w, c + b) + 1)])


def subset(win, n, rng, corners=False):
    n = min(n, len(win))
    if corners and n >= 4:
        lo, hi = win.min(axis=0), win.max(axis=0)
        is_corner = ((win[:, 0] == lo[0]) | (win[:, 0] == hi[0])) & ((win[:, 1] == lo[1]) | (win[:, 1] == hi[1]))
        rest = rng.permutation(np.nonzero(~is_corner)[0])[:n - 4]
        idx = np.concatenate([np.nonzero(is_corner)[0], rest])
    else:
        idx = rng.permutation(len(win))[:n]
    return win[np.sort(idx)]


def sized_sets(H, W, rng, sizes, w=1, b=6, pts=None):
    pts = grid(H, W, w, b) if pts is None else pts
    return {p: subset(window(p[0], p[1], H, W, w, b), sizes[i % len(sizes)], rng, corners=(i // len(sizes)) % 2 == 0) for i, p in enumerate(pts)}


def dense_sets(H, W, rng, sizes, w=1, b=6):
    """every main pixel processed, a random similar set of one of the sizes (or the whole clipped window where it is smaller)"""
    out = {}
    for l in range(w, H - w):
        for c in range(w, W - w):
            out[(l, c)] = subset(window(l, c, H, W, w, b), int(sizes[rng.integers(len(sizes))]), rng)
    return out


FULL = (28, 29, 33, 64, 100, 169)          # sizes of the dense cases of the numerical families: full estimates only
HD, WD = 34, 40                            # dense frames


# ---- families -----------------------------------------------------------------------------------------------------------------------------------
def fam_sizes():
    rng = np.random.default_rng(101)
    H, W = 100, 150
    col, pc = noisy_frame(H, W, rng)
    out = [Case("sizes", col, pc, sized_sets(H, W, rng, SIZES))]
    col, pc = noisy_frame(HD, WD, rng)
    out.append(Case("sizes dense", col, pc, dense_sets(HD, WD, rng, SIZES), dense=True))
    return out


def border_points(H, W, k, w=1, b=6):
    """isolated main pixels on the k-th main line / column from each edge"""
    step = 2 * (b + w) + 1
    top = [(w + k, c) for c in range(w + k, W - w - k, step)]
    if top[-1][1] + step > W - 1 - w - k:
        top.pop()
    top.append((w + k, W - 1 - w - k))
    bottom = [(H - 1 - w - k, c) for (_, c) in top]
    rows = [l for l in range(w + k + step, H - 1 - w - k - step + 1, step)]
    return top + bottom + [(l, w + k) for l in rows] + [(l, W - 1 - w - k) for l in rows]


def fam_borders():
    rng = np.random.default_rng(102)
    H, W = 100, 150
    out = []
    for k in (0, 1, 3):
        col, pc = noisy_frame(H, W, rng)
        sets = {p: window(p[0], p[1], H, W, 1, 6) for p in border_points(H, W, k)}   # the part of the window that is in the frame, fully set
        out.append(Case("borders line %d" % k, col, pc, sets))
    col, pc = noisy_frame(HD, WD, rng)
    out.append(Case("borders dense full windows", col, pc, {(l, c): window(l, c, HD, WD, 1, 6) for l in range(1, HD - 1) for c in range(1, WD - 1)}, dense=True))
    return out


def fam_pure_noise():
    rng = np.random.default_rng(103)
    H, W = 100, 150
    col, pc = noisy_frame(H, W, rng, amp=0.0)
    out = [Case("pure noise", col, pc, sized_sets(H, W, rng, (169, 40)))]
    col, pc = noisy_frame(HD, WD, rng, amp=0.0)
    out.append(Case("pure noise dense", col, pc, dense_sets(HD, WD, rng, (169, 40)), dense=True))
    return out


def fam_constant():
    rng = np.random.default_rng(104)
    H, W = 70, 150
    col = np.broadcast_to(np.array([0.7, 0.25, 0.4]), (H, W, 3))
    out = [Case("constant", col, cov6(noise_model(H, W, rng)), sized_sets(H, W, rng, (28, 64, 169)))]
    col = np.broadcast_to(np.array([0.7, 0.25, 0.4]), (HD, WD, 3))
    out.append(Case("constant dense", col, cov6(noise_model(HD, WD, rng)), dense_sets(HD, WD, rng, FULL), dense=True))
    return out


def fam_zero_noise():
    rng = np.random.default_rng(105)
    H, W = 70, 150
    col, _ = noisy_frame(H, W, rng)
    out = [Case("zero noise", col, np.zeros((H, W, 6)), sized_sets(H, W, rng, (28, 100)))]
    col, _ = noisy_frame(HD, WD, rng)
    out.append(Case("zero noise dense", col, np.zeros((HD, WD, 6)), dense_sets(HD, WD, rng, FULL), dense=True))
    return out


def fam_low_rank():
    rng = np.random.default_rng(106)
    H, W = 70, 150
    out = []
    # (a) one channel identically 0, colour and covariance
    B = noise_model(H, W, rng)
    B[..., 1, :] = 0.0
    col = signal(H, W) + np.einsum("...ij,...j->...i", B, rng.standard_normal((H, W, 3)))
    col[..., 1] = 0.0
    out.append(Case("low rank: zero channel", col, cov6(B), sized_sets(H, W, rng, (28, 64, 169))))
    # (b) 10 distinct member patches, each 4 times: the frame is a function of (c + 3 l) mod 10, so is every 3 x 3 patch
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    res = (c + 3 * l) % 10
    col = (0.2 + 0.6 * rng.random((10, 3)))[res]
    sets = {}
    for p in grid(H, W, 1, 6):
        win = window(p[0], p[1], H, W, 1, 6)
        r = (win[:, 1] + 3 * win[:, 0]) % 10
        idx = np.concatenate([rng.permutation(np.nonzero(r == k)[0])[:4] for k in range(10)])
        sets[p] = win[np.sort(idx)]
    out.append(Case("low rank: 10 patches x 4", col, cov6(noise_model(H, W, rng)), sets))
    # (c) grey colours, full-rank noise covariance
    g = signal(H, W)[..., :1] + 0.1 * rng.standard_normal((H, W, 1))
    out.append(Case("low rank: grey", np.repeat(g, 3, axis=-1), cov6(noise_model(H, W, rng)), sized_sets(H, W, rng, (28, 64, 169))))
    g = signal(HD, WD)[..., :1] + 0.1 * rng.standard_normal((HD, WD, 1))
    out.append(Case("low rank: grey dense", np.repeat(g, 3, axis=-1), cov6(noise_model(HD, WD, rng)), dense_sets(HD, WD, rng, FULL), dense=True))
    return out


def fam_degenerate():
    """grey colours, fully correlated channel noise: every block of the noise mean has rank 1.  No numerical bar (see the GPU test)."""
    rng = np.random.default_rng(107)
    H, W = 70, 150
    sig = 0.05 + 0.1 * rng.random((H, W, 1))
    g = signal(H, W)[..., :1] + sig * rng.standard_normal((H, W, 1))
    return [Case("degenerate", np.repeat(g, 3, axis=-1), np.repeat(sig * sig, 6, axis=-1), sized_sets(H, W, rng, (28, 64, 169)), judged=False)]


def fam_floor_boundary():
    rng = np.random.default_rng(108)
    H, W = 37, 52                                                         # 2 x 3 isolated items per frame
    col, pc = noisy_frame(H, W, rng)
    base = Case("floor k=0 e=1e-08", col, pc, sized_sets(H, W, rng, (64, 169, 33)))
    out = [base] + [base.scaled(k, "floor k=%d e=1e-08" % k) for k in range(-2, -17, -2)]
    for o in out:
        o.min_eig = 1e-8                                                  # the floor stays where it is while the problem shrinks below it
    for e in (1e-5, 1e-3, 3e-2):
        o = base.scaled(0, "floor k=0 e=%g" % e)
        o.min_eig = e
        out.append(o)
    col, pc = noisy_frame(HD, WD, rng)
    out.append(Case("floor dense e=3e-2", col, pc, dense_sets(HD, WD, rng, FULL), min_eig=3e-2, dense=True))
    return out


def fam_spike(with_matching_cov=False):
    """one pixel of a member's patch 10^2 ... 10^4 times brighter than the rest: with the ordinary noise covariance ("spike"), or with a covariance
    at that pixel that matches its size ("spike + cov": what a firefly looks like to the estimate)"""
    rng = np.random.default_rng(109)
    H, W = 70, 150
    out = []
    for factor, with_cov in ((1e2, False), (1e3, False), (1e2, True), (1e3, True), (1e4, True)):
        col, pc = noisy_frame(H, W, rng)
        sets = sized_sets(H, W, rng, (64, 169, 40))
        for (l, c) in sets:                                               # one pixel of the item's 15 x 15 block, inside a member's patch
            q = sets[(l, c)][rng.integers(len(sets[(l, c)]))]
            sl, sc = q[0] + rng.integers(-1, 2), q[1] + rng.integers(-1, 2)
            col[sl, sc] *= factor
            if with_cov:
                pc[sl, sc] *= factor * factor
        out.append(Case("spike x%g%s" % (factor, " + cov" if with_cov else ""), col, pc, sets))
    return [c for c in out if c.name.endswith(" + cov") == with_matching_cov]   # (one generator, one random stream: two families)


def block_scale(H, W, pts, scales, w=1, b=6):
    """per-pixel factor: scales[i] on the 2 (b + w) + 1 block of item i, 1 elsewhere"""
    f = np.ones((H, W, 1))
    r = b + w
    for (l, c), s in zip(pts, scales):
        f[max(0, l - r):l + r + 1, max(0, c - r):c + r + 1] = s
    return f


def fam_dark():
    rng = np.random.default_rng(110)
    H, W = 100, 150
    col, pc = noisy_frame(H, W, rng)
    sets = sized_sets(H, W, rng, SIZES)
    pts = sorted(sets)
    f = np.full((H, W, 1), 1e-3)                                          # everything dark ...
    f *= block_scale(H, W, [pts[len(pts) // 2]], [1e3])                   # ... except the block of one item
    # min_eig = 1e-8 is at the size of the dark covariances (1e-2 x 1e-6): nearly every dark item then takes the redo list.  The second case scales the
    # floor with the frame, so that the accepted sweep inverse sees dark input too.
    return [Case("dark next to one bright item", col * f, pc * f * f, sets),
            Case("dark, floor scaled with the frame", col * f, pc * f * f, sets, min_eig=1e-14)]


def fam_scaling():
    rng = np.random.default_rng(111)
    H, W = 70, 150
    col, pc = noisy_frame(H, W, rng)
    base = Case("scaling k=0", col, pc, sized_sets(H, W, rng, (28, 33, 64, 128, 169)))
    return [base.scaled(k, "scaling k=%d" % k) for k in (-6, 6, 12)]


def fam_non_finite():
    rng = np.random.default_rng(112)
    H, W = 52, 150
    out = []
    for what in ("nan colour", "inf colour", "nan pixcov"):
        col, pc = noisy_frame(H, W, rng)
        sets = sized_sets(H, W, rng, (64, 9, 169, 28, 27))
        pts = sorted(sets)
        for p in pts[::3]:                                                # every third item is poisoned, its neighbours must not notice
            q = sets[p][rng.integers(len(sets[p]))]
            if what == "nan pixcov":
                pc[q[0], q[1], rng.integers(6)] = np.nan
            else:
                col[q[0] + rng.integers(-1, 2), q[1] + rng.integers(-1, 2), rng.integers(3)] = np.nan if what == "nan colour" else np.inf
        out.append(Case("non-finite: " + what, col, pc, sets))
    return out


def fam_other_kernels():
    """the geometries test_other_patch_radii runs: (w, b) -> the kernel the dispatcher of bcd_api.hip selects
       (1, 12) k_bayes27w<1, 12> + k_finish27w (window kernels of the large search radius), fallback: k_bayes_weak_tile
       (1, 3), (1, 4) k_bayes27<1> / k_bayes27<2> (gather kernels)
       (2, 3) every set is below 76: k_bayes_weak only;  (2, 6), (0, 4): k_bayes_strong_generic + k_bayes_weak"""
    rng = np.random.default_rng(113)
    out = []
    for (w, b, H, W, sizes) in ((1, 12, 110, 160, (625, 28, 27, 169, 40, 624, 65, 300)), (1, 3, 60, 100, (49, 28, 27, 40, 9, 33)), (1, 4, 60, 100, (81, 28, 27, 64, 65, 1)),
                                (2, 3, 60, 100, (49, 1, 30)), (2, 6, 80, 140, (169, 76, 75, 100, 128, 77)), (0, 4, 60, 100, (81, 4, 3, 5, 33, 64, 1))):
        for amp in (1.0, 0.0):
            col, pc = noisy_frame(H, W, rng, amp=amp)
            out.append(Case("w=%d b=%d %s" % (w, b, "sizes" if amp else "pure noise"), col, pc, sized_sets(H, W, rng, sizes, w, b), w=w, b=b))
    col, pc = noisy_frame(HD, WD, rng)
    out.append(Case("w=2 b=6 dense", col, pc, dense_sets(HD, WD, rng, (169, 76, 75, 100), 2, 6), w=2, b=6, dense=True))
    col, pc = noisy_frame(HD, WD, rng)
    out.append(Case("w=1 b=4 dense", col, pc, dense_sets(HD, WD, rng, (81, 28, 27, 64), 1, 4), w=1, b=4, dense=True))
    return out


FAMILIES = {"sizes": fam_sizes, "borders": fam_borders, "pure noise": fam_pure_noise, "constant": fam_constant, "zero noise": fam_zero_noise,
            "low rank": fam_low_rank, "degenerate": fam_degenerate, "floor boundary": fam_floor_boundary, "spike": fam_spike, "spike + cov": lambda: fam_spike(True), "dark": fam_dark,
            "scaling": fam_scaling, "non-finite": fam_non_finite, "other kernels": fam_other_kernels}


def call_sequence(H=48, W=80, counts=(600, 600, 3000, 10)):
    """one geometry, dense states, |S| >= 28 everywhere; the first `counts[i]` main pixels in a seeded order are processed in call i"""
    rng = np.random.default_rng(114)
    col, pc = noisy_frame(H, W, rng)
    sets = dense_sets(H, W, rng, (28, 33, 64, 100, 169))
    full = Case("call sequence", col, pc, sets, dense=True)
    assert (full.nsim[1:H - 1, 1:W - 1] >= 28).all() and (H - 2) * (W - 2) >= max(counts)
    order = rng.permutation((H - 2) * (W - 2))
    calls = []
    for n in counts:
        o = Case.__new__(Case)
        o.__dict__.update(full.__dict__)
        st = np.zeros((H - 2) * (W - 2), np.uint8)
        st[order[:n]] = 1
        o.state = np.zeros((H, W), np.uint8)
        o.state[1:H - 1, 1:W - 1] = st.reshape(H - 2, W - 2)
        o.name = "call sequence: %d items" % n
        calls.append(o)
    return calls
