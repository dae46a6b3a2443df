"""Reference of the Bayesian estimate that takes the similar sets as INPUT (test infrastructure only).

A NumPy restatement of denoiseSelectedPatches / denoiseOnlyMainPatch / aggregateOutputPatches written from the reference source
(src/core/DenoisingUnit.cpp:388-481, 483-693, Denoiser.cpp:357-373, 434-470; CovarianceMatrix.h:18-27) -- not from oracle/bcd_oracle.c and not
from the kernels -- with numpy.linalg.eigh in place of Eigen's solver.  In the terms of bcd_hip_bayes_accumulate: colours, per-pixel noise
covariances, similarity bit masks, |S| and the state image go in, the sum / count accumulators come out.

The same code runs in two precisions:
  dtype = float64   the reference the kernels are judged against;
  dtype = float32   the CALIBRATOR: every array and every product in float32, LAPACK ssyevd on float32 input -- what a plain fp32 evaluation of
                    the reference's formulas loses on that very case.  The bars of the GPU tests are multiples of this error, per item.
Non-finite input follows the arithmetic: a NaN / inf member poisons whatever it is added to or multiplied with.  An eigen-decomposition of a
matrix with a non-finite entry is all-NaN (every rotation of an iterative solver mixes the entry into every row; LAPACK is not called on it)."""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32


def offsets(w):
    """patch pixels, row-major (DeepImage.hpp window iteration)"""
    return [(a, d) for a in range(-w, w + 1) for d in range(-w, w + 1)]


def decode_members(words, l, c, b):
    """similar set of the main pixel (l, c) from its mask words: positions in window order (:196-219), bit k <-> (l + k // side - b, c + k % side - b)"""
    side = 2 * b + 1
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:side * side]
    k = np.nonzero(bits)[0]
    return np.stack([l + k // side - b, c + k % side - b], axis=1).astype(np.int64)


def encode_members(pos, l, c, b):
    """inverse of decode_members: uint32 mask words of the window of (l, c)"""
    side = 2 * b + 1
    words = (side * side + 31) // 32
    bits = np.zeros(words * 32, np.uint8)
    pos = np.asarray(pos, np.int64).reshape(-1, 2)
    k = (pos[:, 0] - l + b) * side + (pos[:, 1] - c + b)
    assert np.all(np.abs(pos[:, 0] - l) <= b) and np.all(np.abs(pos[:, 1] - c) <= b)
    bits[k] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def popcount(mask):
    """|S| per pixel from (H, W, words) uint32 mask words"""
    m = np.ascontiguousarray(mask).view(np.uint32)
    return np.unpackbits(m.view(np.uint8).reshape(m.shape[0], m.shape[1], -1), axis=-1).sum(axis=-1).astype(np.int32)


def _spectral(M, fn):
    """V fn(lambda) V^T (:578-630) and the eigenvalues"""
    if not np.isfinite(M).all():
        return np.full_like(M, np.nan), np.full(M.shape[0], np.nan, M.dtype)
    lam, V = np.linalg.eigh(M)
    return (V * fn(lam)) @ V.T, lam


def gather(img, pos, w):
    """(n, P, channels): the patch pixels of the members, row-major"""
    oa = np.array([a for (a, d) in offsets(w)])
    od = np.array([d for (a, d) in offsets(w)])
    return img[pos[:, 0][:, None] + oa, pos[:, 1][:, None] + od]


def stages(col, pixcov, pos, w=1, min_eig=1e-8, dtype=np.float64):
    """every intermediate of the estimate of one similar set.  col (H, W, 3), pixcov (H, W, 6; xx yy zz yz xz xy), pos (n, 2) member main
    pixels in window order.  Fallback sets (n < 3 (2w+1)^2 + 1, :182) stop at the mean (:455-481)."""
    dt = np.dtype(dtype).type
    pos = np.asarray(pos, np.int64).reshape(-1, 2)
    n = pos.shape[0]
    P = (2 * w + 1) ** 2
    K = 3 * P
    X = gather(col, pos, w).astype(dt).reshape(n, K)                     # :483-498: pixel-major, RGB
    with np.errstate(all="ignore"):
        st = {"x": X, "mean1": X.mean(axis=0)}
        if n < K + 1:
            return st
        noise6 = gather(pixcov, pos, w).astype(dt).sum(axis=0) / dt(n)   # computeNoiseCovPatchesMean (:400-419)
        N = np.zeros((K, K), dt)
        for o in range(P):
            xx, yy, zz, yz, xz, xy = noise6[o]                           # CovarianceMatrix.h:18-27
            N[3 * o:3 * o + 3, 3 * o:3 * o + 3] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
        floor = dt(min_eig)
        inv = lambda lam: dt(1.0) / np.maximum(floor, lam)
        Xc = X - st["mean1"]
        C = Xc.T @ Xc / dt(n - 1)                                        # :522-536
        clamped, eig_cmn = _spectral(C - N, lambda lam: np.maximum(dt(0.0), lam))   # :606-630
        inv1, lam1 = _spectral(clamped + N, inv)                         # :578-604
        X1 = X - (N @ (inv1 @ Xc.T)).T                                   # :656-670
        m2 = X1.mean(axis=0)
        X1c = X1 - m2
        C2 = X1c.T @ X1c / dt(n - 1)
        inv2, lam2 = _spectral(C2 + N, inv)
        X2 = X - (N @ (inv2 @ (X - m2).T)).T                             # :449-450: the NOISY patches centred on the Step-2 mean
        cond = lambda lam: float(np.max(np.maximum(floor, lam)) / np.min(np.maximum(floor, lam)))
        st.update(noise=noise6, cov1=C, cov1_minus_noise=C - N, clamped=clamped, clamped_plus_noise=clamped + N, inverse1=inv1, step1=X1,
                  mean2=m2, cov2=C2, inverse2=inv2, step2=X2, eig_cmn=eig_cmn, cond1=cond(lam1), cond2=cond(lam2))
    return st


_LIGHT = ("cond1", "cond2", "eig_cmn")


def accumulate(col, pixcov, mask, nsim, state, w, b, min_eig, dtype=np.float64, keep_stages=True):
    """-> (sum (H, W, 3) dtype, count (H, W) int32, per_item): every pixel with state == 1, members from its mask words, fallback or the two steps,
    aggregated like aggregateOutputPatches (:672-693) / denoiseOnlyMainPatch.  per_item: one dict per processed pixel in scanline order with
    "pos", "members", "n" and the stages (keep_stages=False: cond1, cond2 and the eigenvalues of C - N only)."""
    dt = np.dtype(dtype).type
    H, W, _ = col.shape
    mask = np.ascontiguousarray(mask).view(np.uint32).reshape(H, W, -1)
    acc = np.zeros((H, W, 3), dt)
    cnt = np.zeros((H, W), np.int32)
    P = (2 * w + 1) ** 2
    K = 3 * P
    oa = np.array([a for (a, d) in offsets(w)])
    od = np.array([d for (a, d) in offsets(w)])
    per_item = []
    with np.errstate(all="ignore"):
        for l, c in zip(*np.nonzero(np.asarray(state) == 1)):
            l, c = int(l), int(c)
            pos = decode_members(mask[l, c], l, c, b)
            n = pos.shape[0]
            assert n == int(nsim[l, c]), "nsim must be the popcount of the mask"
            # (an empty set, as a NaN histogram leaves it: denoiseOnlyMainPatch adds (1 / 0) * 0 = NaN and counts the estimate)
            st = stages(col, pixcov, pos, w, min_eig, dtype) if n else {"mean1": np.full(K, np.nan, dt)}
            item = {"pos": (l, c), "members": pos, "n": n}
            item.update(st if keep_stages else {k: st[k] for k in _LIGHT if k in st})
            per_item.append(item)
            if n < K + 1:
                np.add.at(acc, (l + oa, c + od), st["mean1"].reshape(P, 3))
                np.add.at(cnt, (l + oa, c + od), 1)
                continue
            rows = (pos[:, 0][:, None] + oa).ravel()
            cols = (pos[:, 1][:, None] + od).ravel()
            np.add.at(acc, (rows, cols), st["step2"].reshape(n * P, 3))
            np.add.at(cnt, (rows, cols), 1)
    return acc, cnt, per_item


def touched(item, w):
    """(rows, cols) of the output pixels the item writes"""
    oa = np.array([a for (a, d) in offsets(w)])
    od = np.array([d for (a, d) in offsets(w)])
    K1 = 3 * (2 * w + 1) ** 2 + 1
    if item["n"] < K1:
        return item["pos"][0] + oa, item["pos"][1] + od
    pos = item["members"]
    rc = np.unique(np.stack([(pos[:, 0][:, None] + oa).ravel(), (pos[:, 1][:, None] + od).ravel()], 1), axis=0)
    return rc[:, 0], rc[:, 1]


def item_error(got, ref, item, w):
    """max |got - ref| / s over the pixels the item touches, s the largest |ref| there (the per-item scale of the isolated cases)"""
    r, c = touched(item, w)
    a, b_ = np.asarray(got, np.float64)[r, c], np.asarray(ref, np.float64)[r, c]
    ok = np.isfinite(b_)
    if not ok.any():
        return 0.0
    s = float(np.max(np.abs(b_[ok])))
    d = np.abs(a - b_)[ok]
    if not np.isfinite(d).all():
        return float("inf")
    return float(d.max() / s) if s > 0 else (0.0 if d.max() == 0 else float("inf"))


def local_max(a, r=7):
    """(H, W): maximum of |a| (over the channels too) in the (2r+1) x (2r+1) neighbourhood of every pixel"""
    m = np.abs(np.asarray(a, np.float64))
    m = np.where(np.isfinite(m), m, 0.0)
    if m.ndim == 3:
        m = m.max(axis=2)
    for axis in (0, 1):
        p = np.pad(m, [(r, r) if ax == axis else (0, 0) for ax in (0, 1)])
        n, out = m.shape[axis], None
        for k in range(2 * r + 1):
            sl = p[k:k + n] if axis == 0 else p[:, k:k + n]
            out = sl.copy() if out is None else np.maximum(out, sl, out=out)
        m = out
    return m


def rel_local(a, b, r=7):
    """max |a - b| relative to the largest |b| of the pixel's (2r+1)^2 neighbourhood: what a frame-wide maximum hides in the dark parts"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = local_max(b, r)
    ok = np.isfinite(b) & (s > 0)[..., None] if b.ndim == 3 else np.isfinite(b) & (s > 0)
    d = np.abs(a - b) / (s[..., None] if b.ndim == 3 else s).clip(1e-300)
    d = d[ok]
    return float(d.max()) if d.size and np.isfinite(d).all() else (0.0 if not d.size else float("inf"))
