"""NumPy float32 restatement of the cross-frame selection from means and covariances ("Moments"; include/bcd_hip.h, "moments").  TEST
INFRASTRUCTURE, written from the definition: vectorised over the frame, one displacement at a time; every NumPy float32 operation is one IEEE operation,
so nothing is contracted or reassociated.

For pixel x of the frame and pixel y = x + delta of neighbour j, y inside the image, channels k = 0, 1, 2 in order, from s = 0, n = 0 (m0, mj: the guide
layer's colours of the frame and of the neighbour, v0, vj: entries xx, yy, zz of their per-pixel covariances, eps: the variance floor):
    d = m0_k(x) - mj_k(y);   q = (v0_k(x) + vj_k(y)) + eps;   if q > 0: s = s + (d * d) / q, n = n + 1
    T_delta(x) = s, C_delta(x) = n
A NaN q is not counted; a NaN or infinite term IS counted.  All (2b+1)^2 displacements, index k = (dl + b)(2b + 1) + (dc + b) = mask bit k.
Patch distance of main pixel p of the frame to main pixel p + delta of the neighbour: the (2w+1)^2 entries of T_delta around p added in patch row-major order
from 0, over the float of the summed C; similar iff <= tau; 0 / 0 is NaN and never similar; pixels that are not main pixels have empty masks."""
import numpy as np

F = np.float32


def offsets(b):
    """all displacements (dl, dc) in mask-bit order"""
    return [(dl, dc) for dl in range(-b, b + 1) for dc in range(-b, b + 1)]


def planes(m0, P0, mj, Pj, b, eps):
    """-> T (side^2, H, W) float32, C (side^2, H, W) int32, written (side^2, H, W) bool: the entries whose y lies inside the image (the others stay 0)"""
    m0, mj = np.asarray(m0, F), np.asarray(mj, F)
    v0, vj = np.asarray(P0, F)[..., :3], np.asarray(Pj, F)[..., :3]
    assert m0.shape == mj.shape and v0.shape == vj.shape == m0.shape
    eps = F(eps)
    H, W, _ = m0.shape
    side = 2 * b + 1
    T, C, written = np.zeros((side * side, H, W), F), np.zeros((side * side, H, W), np.int32), np.zeros((side * side, H, W), bool)
    with np.errstate(all="ignore"):
        for k, (dl, dc) in enumerate(offsets(b)):
            l0, l1, c0, c1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)          # x with y = x + (dl, dc) inside the image
            if l0 >= l1 or c0 >= c1:
                continue
            s = np.zeros((l1 - l0, c1 - c0), F)
            n = np.zeros((l1 - l0, c1 - c0), np.int32)
            for ch in range(3):
                d = m0[l0:l1, c0:c1, ch] - mj[l0 + dl:l1 + dl, c0 + dc:c1 + dc, ch]
                q = (v0[l0:l1, c0:c1, ch] + vj[l0 + dl:l1 + dl, c0 + dc:c1 + dc, ch]) + eps
                ok = q > 0                                                                     # (False for a NaN q)
                t = (d * d) / q
                s = np.where(ok, s + t, s)
                n = n + ok
            T[k, l0:l1, c0:c1], C[k, l0:l1, c0:c1], written[k, l0:l1, c0:c1] = s, n, True
    return T, C, written


def distances(m0, P0, mj, Pj, w, b, eps):
    """-> D (side^2, H, W) float32: the patch distance of pixel p of the frame to pixel p + delta of the neighbour; valid (same shape, bool): both are main
    pixels.  Where not valid D is +inf."""
    T, C, _ = planes(m0, P0, mj, Pj, b, eps)
    nk, H, W = T.shape
    D = np.full((nk, H, W), np.inf, F)
    valid = np.zeros((nk, H, W), bool)
    if H < 2 * w + 1 or W < 2 * w + 1:
        return D, valid
    with np.errstate(all="ignore"):
        for k, (dl, dc) in enumerate(offsets(b)):
            l0, l1, c0, c1 = max(w, w - dl), min(H - w, H - w - dl), max(w, w - dc), min(W - w, W - w - dc)   # main p with a main partner
            if l0 >= l1 or c0 >= c1:
                continue
            s = np.zeros((l1 - l0, c1 - c0), F)
            n = np.zeros((l1 - l0, c1 - c0), np.int32)
            for ol in range(-w, w + 1):
                for oc in range(-w, w + 1):
                    s = s + T[k, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
                    n = n + C[k, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
            D[k, l0:l1, c0:c1] = s / n.astype(F)
            valid[k, l0:l1, c0:c1] = True
    return D, valid


def masks_from(D, valid, tau):
    """-> mask (H, W, words) uint32, |S_j| (H, W) int32"""
    with np.errstate(invalid="ignore"):
        sim = valid & (D <= F(tau))
    nbits, H, W = sim.shape
    mask = np.zeros((H, W, (nbits + 31) // 32), np.uint32)
    for k in range(nbits):
        mask[..., k // 32] |= sim[k].astype(np.uint32) << np.uint32(k % 32)
    return mask, sim.sum(0).astype(np.int32)


def masks(m0, P0, mj, Pj, w, b, tau, eps):
    D, valid = distances(m0, P0, mj, Pj, w, b, eps)
    return masks_from(D, valid, tau)


def window_distances(D, line, col):
    """what bcd_hip_window_distances_moments_cross returns for a main pixel: (2b+1)^2 floats, +inf outside"""
    return np.ascontiguousarray(D[:, line, col])
