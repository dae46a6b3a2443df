"""Constructed frames for the similar-patch selection from means and covariances (tests/test_moments_cases_cpu.py, tests/test_gpu_moments_stage.py,
tests/test_gpu_moments.py).  TEST INFRASTRUCTURE; everything is seeded.

  noisy      two regions of constant signal (split along a slanted line, so that patches straddle it at every column phase), `spp` samples per pixel of
             Gaussian noise; mean, unbiased sample covariance and sample count per pixel as an accumulator would hold them.  Between pixels of one
             region a term (d * d) / q has expectation about 1, so at tau = 1 roughly 40 % of the same-region pairs are similar: masks neither
             empty nor full.
  special    the noisy frame with, away from each other: pixels whose covariances are NaN (q is NaN: not counted), a block of equal colours and ZERO
             variance (under eps = 0 no channel is counted and a patch inside the block has distance 0 / 0; under eps > 0 the distance is 0), one
             pixel with an infinite mean and one with a NaN mean.
Thresholds: 1, and -- chosen from the reference's own distances -- a patch distance that occurs and the float below it."""
import numpy as np

import moments_ref as mr

F = np.float32
STAGE_FRAMES = [(70, 13), (264, 20)]          # (W, H): one tile column and a bit, lines no multiple of 4 / a multiple of 4, more than 248 columns
STAGE_RADII = [1, 6, 12]
STAGE_PATCHES = [1, 2]                        # w = 2 takes k_masks, w = 1 the forward-mask kernels
FLOORS = [0.0, 1e-4]


def pixel_cov(cov, ns):
    """bcd_hip_pixel_cov in NumPy float32: cov * (1 / n)"""
    with np.errstate(all="ignore"):
        inv = F(1) / np.asarray(ns, F).reshape(ns.shape[0], ns.shape[1], 1)
        return (np.asarray(cov, F) * inv).astype(F)


def noisy(W, H, spp=8, seed=1, sigma=0.25):
    """-> colours (H, W, 3), sample covariances (H, W, 6: xx yy zz yz xz xy), sample counts (H, W, 1), the noise-free signal (H, W, 3)"""
    rng = np.random.default_rng(seed)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    right = (c + l // 2) >= W // 2
    signal = np.where(right[..., None], np.array([0.8, 0.5, 0.3]), np.array([0.3, 0.45, 0.7]))
    samples = signal[:, :, None, :] + sigma * rng.standard_normal((H, W, spp, 3))
    mean = samples.mean(2)
    dev = samples - mean[:, :, None, :]
    c2 = np.einsum("hwsi,hwsj->hwij", dev, dev) / (spp - 1)
    cov = np.stack([c2[..., 0, 0], c2[..., 1, 1], c2[..., 2, 2], c2[..., 1, 2], c2[..., 0, 2], c2[..., 0, 1]], -1)
    return mean.astype(F), cov.astype(F), np.full((H, W, 1), spp, F), signal.astype(F)


def special(W, H, spp=8, seed=1):
    """the noisy frame with the special pixels; needs W >= 40, H >= 12"""
    col, cov, ns, _ = noisy(W, H, spp, seed)
    cov[2, 5] = np.nan                                   # a main pixel next to the border
    cov[H - 3, W - 9, :3] = np.nan                       # only the entries that are read
    col[5:10, 20:27] = F(0.5)                            # 5 x 7 block: a 3 x 3 patch fits inside with its whole neighbourhood
    cov[5:10, 20:27] = 0
    col[3, 33, 1] = np.inf
    col[H - 4, 12, 2] = np.nan
    return col, cov, ns


_stage = {}


def stage_case(W, H, w, b, eps):
    """one frame of the stage test with its reference (computed once, shared read-only): dict(col, cov, ns, P, D, valid, taus)"""
    key = (W, H, w, b, eps)
    if key not in _stage:
        col, cov, ns = special(W, H, seed=W + b)
        P = pixel_cov(cov, ns)
        D, valid = mr.distances(col, P, w, b, eps)
        _stage[key] = dict(col=col, cov=cov, ns=ns, P=P, D=D, valid=valid, taus=thresholds(D, valid))
    return _stage[key]


def thresholds(D, valid):
    """1, a patch distance the reference produced near 1 (a pair exactly AT the threshold) and the float below it"""
    d = D[valid & np.isfinite(D) & (D > 0)]
    at = d[np.argmin(np.abs(d - F(1)))] if d.size else F(1)
    return [F(1), F(at), np.nextafter(F(at), F(-np.inf))]


def layers_of(col, cov, n):
    """n colour layers of one frame: the frame itself, then smooth per-pixel factors of it (colour, magnitude and covariance differ)"""
    H, W, _ = col.shape
    l, c = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    out = [(col, cov)]
    for k in range(1, n):
        g = np.stack([0.2 + 0.7 * ((c + 3 * k) % W) / W, 0.9 - 0.6 * ((l + 5 * k) % H) / H, 0.3 + 0.05 * k + 0.2 * (l + c) / (H + W)], -1).astype(F)
        gg = np.stack([g[..., 0] * g[..., 0], g[..., 1] * g[..., 1], g[..., 2] * g[..., 2], g[..., 1] * g[..., 2], g[..., 0] * g[..., 2], g[..., 0] * g[..., 1]], -1)
        out.append((np.ascontiguousarray(col * g), np.ascontiguousarray(cov * gg)))
    return out
