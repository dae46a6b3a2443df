"""Constructed frames for the feature gate of the similar-patch selection (tests/test_guide_cases_cpu.py, tests/test_gpu_guide_stage.py,
tests/test_gpu_guide.py).  TEST INFRASTRUCTURE; everything is seeded.

  features   two feature regions split along (c - l // 3) >= W // 3 -- another line than moments_cases.noisy's colour edge --; channel k has the level
             a_k = 0.2 + 0.1 k in one region and a_k + 0.3 (even k) or a_k - 0.15 (odd k) in the other, plus the smooth 0.02 sin((l + 2c) / 9 + k).
             `spp` = 8 samples of Gaussian noise with sigma = 0.05 sqrt(8) per sample, so the mean has sigma = 0.05; the variance image is the unbiased
             sample variance / 8, the variance of the pixel's feature mean.  sigma = 0 gives the noise-free features (variance 0).
  floors     1e-4 with variances, 0.01 (a tolerance of 0.1) without; tau_g = 1.
  special    the same with, away from each other: a NaN feature, a 5 x 7 block of +inf in one channel (inside it the terms are NaN and skipped, on its rim
             they are +inf and counted), one +inf pixel beside finite ones, a NaN variance (with variances), and -- without variances, F >= 2 -- channel 1
             with floor 0, which is switched off.
Thresholds: 1, and -- chosen from the reference's own distances -- a patch distance that occurs and the float below it (moments_cases.thresholds)."""
import numpy as np

import guide_ref as gr
import moments_cases as mc

F32 = np.float32
STAGE_FRAMES = mc.STAGE_FRAMES                # (70, 13), (264, 20)
STAGE_RADII = mc.STAGE_RADII                  # 1, 6, 12
STAGE_PATCHES = mc.STAGE_PATCHES              # 1, 2
STAGE_CHANNELS = [1, 3, 7, 8]
FLOOR_VAR, FLOOR_PLAIN = 1e-4, 0.01
SPP = 8


def region(W, H):
    """(H, W) bool: the second feature region"""
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (c - l // 3) >= W // 3


def features(W, H, F, seed=1, sigma=0.05):
    """-> features (H, W, F) float32 (the mean of SPP samples), variances (H, W, F) float32 (of that mean), the noise-free signal (H, W, F) float32"""
    rng = np.random.default_rng(seed)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    second = region(W, H)
    k = np.arange(F)
    a = 0.2 + 0.1 * k
    step = np.where(k % 2 == 0, 0.3, -0.15)
    signal = a + second[..., None] * step + 0.02 * np.sin((l + 2 * c)[..., None] / 9.0 + k)
    samples = signal[:, :, None, :] + sigma * np.sqrt(SPP) * rng.standard_normal((H, W, SPP, F))
    mean = samples.mean(2)
    var = samples.var(2, ddof=1) / SPP
    return mean.astype(F32), var.astype(F32), signal.astype(F32)


def floors(F, with_var, special=False):
    fl = np.full(F, FLOOR_VAR if with_var else FLOOR_PLAIN, F32)
    if special and not with_var and F >= 2:
        fl[1] = 0                                        # no variance and floor 0: the channel is switched off
    return fl


def special(W, H, F, with_var, seed=1):
    """the noisy features with the special pixels -> (features, variances or None, floors); needs W >= 40, H >= 12"""
    f, v, _ = features(W, H, F, seed)
    f[2, 5, 0] = np.nan                                  # a main pixel next to the border
    f[5:10, 20:27, F - 1 if F != 2 else 0] = np.inf      # 5 x 7 block: a 3 x 3 patch fits inside with its whole neighbourhood
    f[3, 33, 0] = np.inf                                 # beside finite ones
    if with_var:
        v[H - 3, W - 9, 0] = np.nan
    return f, (v if with_var else None), floors(F, with_var, True)


_stage = {}


def stage_case(W, H, w, b, F, with_var):
    """one frame of the stage test with its reference (computed once, shared read-only): dict(f, v, floors, D, valid, taus)"""
    key = (W, H, w, b, F, with_var)
    if key not in _stage:
        f, v, fl = special(W, H, F, with_var, seed=W + b + F)
        D, valid = gr.distances(f, v, w, b, fl)
        _stage[key] = dict(f=f, v=v, floors=fl, D=D, valid=valid, taus=mc.thresholds(D, valid))
    return _stage[key]


def across_pairs(W, H, w, b):
    """((2b+1)^2, H, W) bool: bit k of pixel p is a pair of main pixels whose two patches lie WHOLLY in different feature regions"""
    sec = region(W, H)
    whole = np.zeros((H, W), np.int8)                    # 1 / 2: the patch lies wholly in the first / second region; 0: it straddles the edge or is no main pixel
    for l in range(w, H - w):
        for k in range(w, W - w):
            p = sec[l - w:l + w + 1, k - w:k + w + 1]
            whole[l, k] = 2 if p.all() else (0 if p.any() else 1)
    side = 2 * b + 1
    across = np.zeros((side * side, H, W), bool)
    for dl in range(-b, b + 1):
        for dc in range(-b, b + 1):
            other = np.zeros((H, W), np.int8)
            l0, l1, k0, k1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)
            other[l0:l1, k0:k1] = whole[l0 + dl:l1 + dl, k0 + dc:k1 + dc]
            across[(dl + b) * side + (dc + b)] = (whole > 0) & (other > 0) & (whole != other)
    return across


def mask_bits(mask, b):
    """(H, W, words) int32 mask -> ((2b+1)^2, H, W) bool"""
    u = np.ascontiguousarray(mask).view(np.uint32)
    n = (2 * b + 1) ** 2
    return np.stack([((u[..., k // 32] >> np.uint32(k % 32)) & 1).astype(bool) for k in range(n)])
