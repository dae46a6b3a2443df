"""NumPy float32 restatement of the feature gate of the similar-patch selection (k_similarity_guide.hip + the mask kernels of k_similarity.hip).
TEST INFRASTRUCTURE: vectorised over the frame, one displacement at a time; every NumPy float32 operation is one IEEE operation, so nothing is
contracted or reassociated.  It generalises moments_ref.planes to F channels with per-channel floors and the NaN-skip; the box sum, the masks and the
window distances are moments_ref's.

For pixels x and y = x + delta, channels k = 0 .. F-1 in order, from s = 0, n = 0 (f: features, v: the variance of the pixel's feature mean or None,
eps_k: the floor of channel k):
    d = f_k(x) - f_k(y);   q = (v_k(x) + v_k(y)) + eps_k   (v absent: q = 0 + eps_k)
    if q > 0: t = (d * d) / q;  if t == t: s = s + t, n = n + 1
    T_delta(x) = s, C_delta(x) = n
The guided selection is  mask = selection mask AND feature mask, |S| = popcount."""
import numpy as np

import moments_ref as mr
from pyramid_ref import downscale_avg  # noqa: F401  (the one restatement of bcd_hip_downscale_avg; pyramid() below and the guide tests use it)

F32 = np.float32


def _pair(f, v, eps, dl, dc):
    """T and C of displacement (dl, dc), dl >= 0, on the pixels x whose neighbour x + (dl, dc) is inside the image: (rows, cols, T, C)"""
    H, W, F = f.shape
    r0, r1 = 0, H - dl
    c0, c1 = max(0, -dc), min(W, W - dc)
    if r1 <= r0 or c1 <= c0:
        return None
    fx, fy = f[r0:r1, c0:c1], f[r0 + dl:r1 + dl, c0 + dc:c1 + dc]
    s = np.zeros(fx.shape[:2], F32)
    n = np.zeros(fx.shape[:2], np.int32)
    with np.errstate(all="ignore"):
        for k in range(F):
            d = fx[..., k] - fy[..., k]
            if v is None:
                q = np.full(d.shape, F32(0) + eps[k], F32)
            else:
                q = (v[r0:r1, c0:c1, k] + v[r0 + dl:r1 + dl, c0 + dc:c1 + dc, k]) + eps[k]
            t = (d * d) / q
            ok = (q > 0) & (t == t)
            s = np.where(ok, s + t, s)
            n = n + ok
    return (r0, r1), (c0, c1), s, n


def planes(f, v, b, floors):
    """-> T (nd, H, W) float32, C (nd, H, W) uint8, written (nd, H, W) bool: the entries whose neighbour is inside the image (the others stay 0)"""
    f = np.asarray(f, F32)
    v = None if v is None else np.asarray(v, F32)
    H, W, F = f.shape
    eps = np.asarray(floors, F32).reshape(-1)
    assert eps.size == F and (v is None or v.shape == f.shape)
    ds = mr.deltas(b)
    T = np.zeros((len(ds), H, W), F32)
    C = np.zeros((len(ds), H, W), np.uint8)
    written = np.zeros((len(ds), H, W), bool)
    for i, (dl, dc) in enumerate(ds):
        got = _pair(f, v, eps, dl, dc)
        if got is None:
            continue
        (r0, r1), (c0, c1), s, n = got
        T[i, r0:r1, c0:c1] = s
        C[i, r0:r1, c0:c1] = n
        written[i, r0:r1, c0:c1] = True
    return T, C, written


def distances_from(T, C, w, b):
    """the box sum of moments_ref.distances on given planes -> D ((2b+1)^2, H, W) float32 (+inf where not valid), valid (same shape, bool)"""
    nd, H, W = T.shape
    side = 2 * b + 1
    D = np.full((side * side, H, W), np.inf, F32)
    valid = np.zeros((side * side, H, W), bool)
    if H < 2 * w + 1 or W < 2 * w + 1:
        return D, valid
    for dl, dc in mr.deltas(b):
        i = mr.delta_index(dl, dc, b)
        r0, r1 = w, H - w - dl
        c0, c1 = max(w, w - dc), min(W - w, W - w - dc)
        if r1 <= r0 or c1 <= c0:
            continue
        s = np.zeros((r1 - r0, c1 - c0), F32)
        n = np.zeros((r1 - r0, c1 - c0), np.int32)
        with np.errstate(all="ignore"):
            for ol in range(-w, w + 1):
                for oc in range(-w, w + 1):
                    s = s + T[i, r0 + ol:r1 + ol, c0 + oc:c1 + oc]
                    n = n + C[i, r0 + ol:r1 + ol, c0 + oc:c1 + oc]
            d = s / n.astype(F32)
        k = (dl + b) * side + (dc + b)
        D[k, r0:r1, c0:c1] = d
        valid[k, r0:r1, c0:c1] = True
        k = (-dl + b) * side + (-dc + b)                 # the same pair seen from the other pixel
        D[k, r0 + dl:r1 + dl, c0 + dc:c1 + dc] = d
        valid[k, r0 + dl:r1 + dl, c0 + dc:c1 + dc] = True
    return D, valid


def distances(f, v, w, b, floors):
    T, C, _ = planes(f, v, b, floors)
    return distances_from(T, C, w, b)


def masks(f, v, w, b, floors, tau):
    """-> feature mask (H, W, words) int32, its counts (H, W) int32"""
    D, valid = distances(f, v, w, b, floors)
    return mr.masks_from(D, valid, b, tau)


def popcount(mask):
    """set bits per pixel of a (H, W, words) int32 / uint32 mask -> (H, W) int32"""
    u = np.ascontiguousarray(mask).view(np.uint32)
    return np.unpackbits(u.view(np.uint8), axis=-1).sum(-1).astype(np.int32)


def gate(mask, feature_mask):
    """the guided selection: (mask AND feature mask, popcount)"""
    m = (np.ascontiguousarray(mask).view(np.uint32) & np.ascontiguousarray(feature_mask).view(np.uint32)).view(np.int32)
    return m, popcount(m)


def pyramid(f, v, nb_scales):
    """-> [(features, variances)] per level: features averaged, variances averaged and multiplied by 0.25 (the variance of a mean of four)"""
    out = [(np.asarray(f, F32), None if v is None else np.asarray(v, F32))]
    for _ in range(1, nb_scales):
        f, v = out[-1]
        with np.errstate(all="ignore"):
            out.append((downscale_avg(f), None if v is None else (downscale_avg(v) * F32(0.25)).astype(F32)))
    return out
