"""NumPy reference of the adaptive sample plan (bcd_hip_accum_plan, include/bcd_hip.h): the error image in float32
with IEEE operations in the documented order, the budget split with exact Python integers."""
import numpy as np

F = np.float32
Q_INF = 1 << 24


def error_image(ns, mean, cov, eps=1e-3, min_samples=2.0):
    """ns (H, W, 1), mean (H, W, 3), cov (H, W, 6): the snapshot's statistics -> e (H, W) float32"""
    ns = np.asarray(ns, F)[..., 0]
    mean, cov = np.asarray(mean, F), np.asarray(cov, F)
    with np.errstate(all="ignore"):
        inv = F(1) / ns
        t = (cov[..., 0] * inv + cov[..., 1] * inv) + cov[..., 2] * inv
        l = (mean[..., 0] + mean[..., 1]) + mean[..., 2]
        ok = (ns >= F(min_samples)) & np.isfinite(t) & np.isfinite(l)
        e = np.sqrt(np.maximum(t / F(3), F(0))) / (F(eps) + np.maximum(l / F(3), F(0)))
    return np.where(ok, e, F(np.inf)).astype(F)


def weights(e, threshold=0.0):
    """-> (q (N,) uint64, E float32, active, unsampled)"""
    e = np.asarray(e, F).reshape(-1)
    active = e > F(threshold)
    inf = active & np.isinf(e)
    fin = active & ~inf
    E = F(e[fin].max()) if fin.any() else F(0)
    q = np.zeros(e.shape, np.uint64)
    q[inf] = Q_INF
    if fin.any():
        r = ((e[fin] / E) * F(16777216)).astype(F)
        q[fin] = np.maximum(r.astype(np.uint64), 1)
    return q, E, int(active.sum()), int(inf.sum())


def split(q, budget, offset=0, max_per_pixel=16):
    """-> (counts (N,) int64 capped, uncapped counts); floor((C_p B + u) / Q) - floor((C_{p-1} B + u) / Q) in exact integers"""
    q = np.asarray(q, np.uint64)
    C = np.cumsum(q, dtype=np.uint64)
    Q = int(C[-1]) if C.size else 0
    if Q == 0 or budget == 0:
        z = np.zeros(q.shape, np.int64)
        return z, z.copy()
    u = int(offset) % Q
    Fl = (C.astype(object) * int(budget) + u) // Q
    Fl = np.concatenate([[0], Fl]).astype(np.int64)     # F(C_{-1}) = floor(u / Q) = 0
    n = np.diff(Fl)
    return np.minimum(n, max_per_pixel), n


def plan(e, budget, offset=0, threshold=0.0, max_per_pixel=16):
    """e (H, W) -> (counts (H, W) int32, pixels (T,) int32, summary dict)"""
    q, E, active, unsampled = weights(e, threshold)
    counts, _ = split(q, budget, offset, max_per_pixel)
    pixels = np.repeat(np.arange(counts.size, dtype=np.int32), counts)
    summary = {"planned": int(counts.sum()), "active": active, "unsampled": unsampled, "max_error": float(E)}
    return counts.reshape(np.shape(e)).astype(np.int32), pixels, summary
