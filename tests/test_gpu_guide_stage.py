"""GPU tests of the stage calls of the feature gate (bcd_hip_similarity_masks_guide, bcd_hip_window_distances_guide, bcd_hip_gate_masks) against
tests/guide_ref.py: masks and |S| with NO tolerance, window distances bit for bit (a NaN is a NaN: its payload is the hardware's) at a border-adjacent and an
interior main pixel, at the threshold 1, at a patch distance the reference produced and at the float below it.
Frames (tests/guide_cases.py): 70 x 13 -- one 64-column tile and a bit, lines no multiple of 4 -- and 264 x 20 -- lines a multiple of 4, more than 248
columns --, search radii 1, 6, 12, patch radii 1 (forward-mask kernels) and 2 (k_masks), 1, 3, 7 and 8 channels with and without variances; a NaN feature,
a block of infinite features, a lone infinite pixel, a NaN variance or a switched-off channel are in every frame.  b = 12 with 8 channels and variances
needs 90 KB of LDS: the case above 64 KiB.  Before each case a histogram similarity pass of another frame runs on the same context: the workspace's
planes then hold foreign values, and -- where the neighbour leaves the image -- entries nobody writes."""
import numpy as np
import pytest

import guide_cases as gc
import guide_ref as gr
import moments_cases as mc
import moments_ref as mr
from test_gpu_layers import dev
from test_gpu_moments_stage import foreign_pass

pytestmark = pytest.mark.gpu


def dev_guide(c):
    d_f, = dev(c["f"])
    d_v = dev(c["v"])[0] if c["v"] is not None else None
    return d_f, d_v


@pytest.mark.parametrize("with_var", [True, False])
@pytest.mark.parametrize("F", gc.STAGE_CHANNELS)
@pytest.mark.parametrize("w", gc.STAGE_PATCHES)
@pytest.mark.parametrize("b", gc.STAGE_RADII)
@pytest.mark.parametrize("W,H", gc.STAGE_FRAMES)
def test_masks_counts_and_window_distances_are_the_reference(hipctx, W, H, b, w, F, with_var):
    c = gc.stage_case(W, H, w, b, F, with_var)
    foreign_pass(hipctx)
    d_f, d_v = dev_guide(c)
    side = 2 * b + 1
    for tau in c["taus"]:
        mask, nsim = hipctx.similarity_masks_guide(d_f, d_v, c["floors"], float(tau), w, b)
        hipctx.synchronize()
        want_mask, want_nsim = mr.masks_from(c["D"], c["valid"], b, tau)
        got_mask, got_nsim = mask.cpu().numpy(), nsim.cpu().numpy()
        bad = int((got_mask != want_mask).sum())
        print("%dx%d w=%d b=%d F=%d %s tau=%.9g: %d similar pairs, %d mask words differ" % (W, H, w, b, F, "var" if with_var else "floors", tau, int(want_nsim.sum()), bad))
        assert np.array_equal(got_mask, want_mask)
        assert np.array_equal(got_nsim, want_nsim)
        foreign_pass(hipctx)
    assert 0 < want_nsim.sum() < c["valid"].sum()
    for line, col in ((w, W // 2), (H // 2, W // 2)):                                   # next to the border, the interior
        got = hipctx.window_distances_guide(d_f, d_v, c["floors"], w, b, line, col)
        want = mr.window_distances(c["D"], line, col)
        assert got.shape == (side * side,)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (line, col)
        assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), (line, col)
        assert np.array_equal(np.isposinf(want) & ~c["valid"][:, line, col], ~c["valid"][:, line, col])        # +inf outside the clipped window


@pytest.mark.parametrize("w,b", [(1, 6), (2, 3), (1, 12)])
def test_three_channels_are_the_moment_selection_on_the_same_numbers(hipctx, w, b):
    """the colours of moments_cases.noisy as features and the xx, yy, zz entries of its per-pixel covariances as variances, a common floor"""
    W, H, eps = 264, 20, 1e-4
    col, cov, ns, _ = mc.noisy(W, H, seed=5)
    d_col, d_cov, d_ns = dev(col, cov, ns)
    d_P = hipctx.pixel_cov(d_cov, d_ns)
    hipctx.synchronize()
    d_v = d_P[..., :3].contiguous()
    for tau in (1.0, 0.7):
        want_mask, want_nsim = hipctx.similarity_masks_moments(d_col, d_P, w, b, tau, eps)
        foreign_pass(hipctx)
        mask, nsim = hipctx.similarity_masks_guide(d_col, d_v, [eps] * 3, tau, w, b)
        hipctx.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want_mask.cpu().numpy()) and np.array_equal(nsim.cpu().numpy(), want_nsim.cpu().numpy())
        assert 0 < int(want_nsim.sum())


@pytest.mark.parametrize("b", [1, 6, 12, 15, 3])
def test_gate_masks_is_and_and_popcount(hipctx, b):
    """random words, rows of all zeros and of all ones in either operand; 1, 6 (two at a time), 20 (four at a time), 31 and 2 words per pixel"""
    import torch
    W, H = 70, 13
    words = ((2 * b + 1) ** 2 + 31) // 32
    rng = np.random.default_rng(b)
    a = rng.integers(0, 2 ** 32, (H, W, words), dtype=np.uint64).astype(np.uint32)
    g = rng.integers(0, 2 ** 32, (H, W, words), dtype=np.uint64).astype(np.uint32)
    a[0] = 0; a[1] = 0xFFFFFFFF; g[1, :30] = 0xFFFFFFFF; g[2] = 0; g[3] = 0xFFFFFFFF; a[4, ::2] = 0xFFFFFFFF
    d_a = torch.from_numpy(a.view(np.int32)).cuda()
    d_g = torch.from_numpy(g.view(np.int32)).cuda()
    d_n = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    hipctx.gate_masks(d_a, d_n, d_g, b)
    hipctx.synchronize()
    want, want_n = gr.gate(a, g)
    assert np.array_equal(d_a.cpu().numpy(), want) and np.array_equal(d_n.cpu().numpy(), want_n)
    assert np.array_equal(d_g.cpu().numpy().view(np.uint32), g)                        # the gate is read only
    assert (want_n[0] == 0).all() and (want_n[1, :30] == 32 * words).all() and (want_n[2] == 0).all()
