"""GPU tests of the selection stage from means and covariances (bcd_hip_similarity_masks_moments, bcd_hip_window_distances_moments) against
tests/moments_ref.py: masks and |S| with NO tolerance, window distances bit for bit (a NaN is a NaN: its payload is the hardware's) at a corner, an edge
and an interior main pixel, at the threshold 1, at a patch distance the reference produced and at the float below it.
Frames (tests/moments_cases.py): 70 x 13 -- one 64-column tile and a bit, lines no multiple of 4, the narrow mask kernel -- and 264 x 20 -- width a multiple
of 4, more than one 248-column wavefront --, search radii 1, 6, 12, patch radii 1 (forward-mask kernels) and 2 (k_masks), variance floors 0 and 1e-4; NaN
covariances, zero variances, infinite and NaN means are in every frame.  Before each case a histogram similarity pass of another frame runs on the same
context: the workspace's planes then hold foreign values, and -- where the neighbour leaves the image -- entries nobody writes."""
import numpy as np
import pytest

import moments_cases as mc
import moments_ref as mr
from test_gpu_layers import dev, frame

pytestmark = pytest.mark.gpu

_foreign = {}


def foreign_pass(ctx):
    """a histogram similarity pass of another frame size on the context's workspace"""
    if not _foreign:
        _, ns, hist, _ = frame(96, 40, 8)
        _foreign["t"] = dev(hist, ns)
    d_hist, d_ns = _foreign["t"]
    ctx.similarity_masks(d_hist, d_ns, 1, 6, 1.0)
    ctx.synchronize()


@pytest.mark.parametrize("eps", mc.FLOORS)
@pytest.mark.parametrize("w", mc.STAGE_PATCHES)
@pytest.mark.parametrize("b", mc.STAGE_RADII)
@pytest.mark.parametrize("W,H", mc.STAGE_FRAMES)
def test_masks_counts_and_window_distances_are_the_reference(hipctx, W, H, b, w, eps):
    c = mc.stage_case(W, H, w, b, eps)
    foreign_pass(hipctx)
    d_col, d_cov, d_ns = dev(c["col"], c["cov"], c["ns"])
    d_P = hipctx.pixel_cov(d_cov, d_ns)
    hipctx.synchronize()
    assert np.array_equal(d_P.cpu().numpy(), c["P"], equal_nan=True)            # the reference read what bcd_hip_pixel_cov returns
    side = 2 * b + 1
    for tau in c["taus"]:
        mask, nsim = hipctx.similarity_masks_moments(d_col, d_P, w, b, float(tau), eps)
        hipctx.synchronize()
        want_mask, want_nsim = mr.masks_from(c["D"], c["valid"], b, tau)
        got_mask, got_nsim = mask.cpu().numpy(), nsim.cpu().numpy()
        bad = int((got_mask != want_mask).sum())
        print("%dx%d w=%d b=%d eps=%g tau=%.9g: %d similar pairs, %d mask words differ" % (W, H, w, b, eps, tau, int(want_nsim.sum()), bad))
        assert np.array_equal(got_mask, want_mask)
        assert np.array_equal(got_nsim, want_nsim)
        foreign_pass(hipctx)
    assert want_nsim.sum() > 0
    for line, col in ((w, w), (w, W // 2), (H // 2, W // 2), (H - 1 - w, W - 1 - w)):      # corners, an edge, the interior
        got = hipctx.window_distances_moments(d_col, d_P, w, b, line, col, eps)
        want = mr.window_distances(c["D"], line, col)
        assert got.shape == (side * side,)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (line, col)
        assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), (line, col)
        assert np.array_equal(np.isposinf(want) & ~c["valid"][:, line, col], ~c["valid"][:, line, col])        # +inf outside the clipped window


def test_the_four_column_mask_kernel_reads_moment_planes(hipctx):
    """1000 x 400: the smallest frame whose forward masks take the four-column kernel (width a multiple of 4, 400 000 pixels); b = 3 keeps the reference small"""
    W, H, w, b, eps = 1000, 400, 1, 3, 1e-4
    c = mc.stage_case(W, H, w, b, eps)
    foreign_pass(hipctx)
    d_col, d_cov, d_ns = dev(c["col"], c["cov"], c["ns"])
    d_P = hipctx.pixel_cov(d_cov, d_ns)
    hipctx.synchronize()
    assert np.array_equal(d_P.cpu().numpy(), c["P"], equal_nan=True)
    for tau in c["taus"][1:]:
        mask, nsim = hipctx.similarity_masks_moments(d_col, d_P, w, b, float(tau), eps)
        hipctx.synchronize()
        want_mask, want_nsim = mr.masks_from(c["D"], c["valid"], b, tau)
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(nsim.cpu().numpy(), want_nsim)
    assert 0 < want_nsim.sum() < c["valid"].sum()
