"""NumPy float32 restatement of the similar-patch selection from means and covariances (k_similarity_moments.hip + the mask kernels of
k_similarity.hip).  TEST INFRASTRUCTURE: vectorised over the frame, one displacement at a time; every NumPy float32 operation is one IEEE operation, so
nothing is contracted or reassociated.

For pixels x and y = x + delta, channels k = 0, 1, 2 in order, from s = 0, n = 0 (m: colours, v_k: entries xx, yy, zz of the per-pixel covariances P,
eps: the variance floor):
    d = m_k(x) - m_k(y);   q = (v_k(x) + v_k(y)) + eps;   if q > 0: s = s + (d * d) / q, n = n + 1        (a NaN q is not counted)
    T_delta(x) = s, C_delta(x) = n
Patch distance of main pixels p and p + delta: the sum of T over the patch (row-major, from 0) over the float of the summed C; similar iff <= tau; 0 / 0 is
NaN and not similar.  The window is clipped to main pixels; bit (dl + b)(2b + 1) + (dc + b) of the mask; |S| = the number of set bits."""
import numpy as np

F = np.float32


def delta_index(dl, dc, b):
    return dc if dl == 0 else (b + 1) + (dl - 1) * (2 * b + 1) + (dc + b)


def deltas(b):
    """the half plane, in index order"""
    return [(0, dc) for dc in range(b + 1)] + [(dl, dc) for dl in range(1, b + 1) for dc in range(-b, b + 1)]


def _pair(m, v, eps, dl, dc, dtype):
    """T and C of displacement (dl, dc), dl >= 0, on the pixels x whose neighbour x + (dl, dc) is inside the image: (rows, cols, T, C)"""
    H, W, _ = m.shape
    r0, r1 = 0, H - dl
    c0, c1 = max(0, -dc), min(W, W - dc)
    if r1 <= r0 or c1 <= c0:
        return None
    mx, my = m[r0:r1, c0:c1], m[r0 + dl:r1 + dl, c0 + dc:c1 + dc]
    vx, vy = v[r0:r1, c0:c1], v[r0 + dl:r1 + dl, c0 + dc:c1 + dc]
    s = np.zeros(mx.shape[:2], dtype)
    n = np.zeros(mx.shape[:2], np.int32)
    with np.errstate(all="ignore"):
        for k in range(3):
            d = mx[..., k] - my[..., k]
            q = (vx[..., k] + vy[..., k]) + eps
            ok = q > 0
            t = (d * d) / q
            s = np.where(ok, s + t, s)
            n = n + ok
    return (r0, r1), (c0, c1), s, n


def planes(m, P, b, eps, dtype=F):
    """-> T (nd, H, W) dtype, C (nd, H, W) uint8, written (nd, H, W) bool: the entries whose neighbour is inside the image (the others stay 0)"""
    m = np.asarray(m, F).astype(dtype)
    v = np.asarray(P, F)[..., :3].astype(dtype)
    eps = dtype(F(eps))
    H, W, _ = m.shape
    ds = deltas(b)
    T = np.zeros((len(ds), H, W), dtype)
    C = np.zeros((len(ds), H, W), np.uint8)
    written = np.zeros((len(ds), H, W), bool)
    for i, (dl, dc) in enumerate(ds):
        got = _pair(m, v, eps, dl, dc, dtype)
        if got is None:
            continue
        (r0, r1), (c0, c1), s, n = got
        T[i, r0:r1, c0:c1] = s
        C[i, r0:r1, c0:c1] = n
        written[i, r0:r1, c0:c1] = True
    return T, C, written


def distances(m, P, w, b, eps, dtype=F):
    """-> D ((2b+1)^2, H, W) dtype: the patch distance of pixel p to p + (dl, dc), index (dl + b)(2b + 1) + (dc + b); valid (same shape, bool): both are
    main pixels.  Where not valid D is +inf."""
    T, C, _ = planes(m, P, b, eps, dtype)
    nd, H, W = T.shape
    side = 2 * b + 1
    D = np.full((side * side, H, W), np.inf, dtype)
    valid = np.zeros((side * side, H, W), bool)
    if H < 2 * w + 1 or W < 2 * w + 1:
        return D, valid
    for dl, dc in deltas(b):
        i = delta_index(dl, dc, b)
        # base pixels x: x and x + (dl, dc) main
        r0, r1 = w, H - w - dl
        c0, c1 = max(w, w - dc), min(W - w, W - w - dc)
        if r1 <= r0 or c1 <= c0:
            continue
        s = np.zeros((r1 - r0, c1 - c0), dtype)
        n = np.zeros((r1 - r0, c1 - c0), np.int32)
        with np.errstate(all="ignore"):
            for ol in range(-w, w + 1):
                for oc in range(-w, w + 1):
                    s = s + T[i, r0 + ol:r1 + ol, c0 + oc:c1 + oc]
                    n = n + C[i, r0 + ol:r1 + ol, c0 + oc:c1 + oc]
            d = s / n.astype(dtype)
        k = (dl + b) * side + (dc + b)
        D[k, r0:r1, c0:c1] = d
        valid[k, r0:r1, c0:c1] = True
        k = (-dl + b) * side + (-dc + b)                 # the same pair seen from the other pixel
        D[k, r0 + dl:r1 + dl, c0 + dc:c1 + dc] = d
        valid[k, r0 + dl:r1 + dl, c0 + dc:c1 + dc] = True
    return D, valid


def masks_from(D, valid, b, tau):
    """-> mask (H, W, words) int32 (the bits of the uint32 words), |S| (H, W) int32"""
    with np.errstate(invalid="ignore"):
        sim = valid & (D <= F(tau))
    nbits, H, W = sim.shape
    words = (nbits + 31) // 32
    mask = np.zeros((H, W, words), np.uint32)
    for k in range(nbits):
        mask[..., k // 32] |= sim[k].astype(np.uint32) << np.uint32(k % 32)
    return mask.view(np.int32), sim.sum(0).astype(np.int32)


def masks(m, P, w, b, tau, eps):
    D, valid = distances(m, P, w, b, eps)
    return masks_from(D, valid, b, tau)


def window_distances(D, line, col):
    """what bcd_hip_window_distances_moments returns for a main pixel: (2b+1)^2 floats, +inf outside"""
    return np.ascontiguousarray(D[:, line, col])
