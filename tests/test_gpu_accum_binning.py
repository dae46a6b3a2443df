"""GPU tests of the histogram binning of the accumulator kernels on the constructed streams of tests/accum_cases.py: colours on every bin
edge and beside it, the entry into saturation and the clamp, special values, exact one-hot histograms, mixed weights, every way of skipping
powf and the division, 2, 3, 85, 86 and 213 bins, frames of 35 pixels and of 1.

Every case goes through each path that can express it: the one-shot kernel (k_accumulate_samples, its own copy of the binning), dense passes
of one sample (k_accum_dense<false>), one dense pass of k >= 8 (k_accum_dense<true>, LDS-staged), the scattered add with the pixels'
samples interleaved, whole and in uneven batches through a small capacity (k_accum_segments), and -- for SPLAT -- the splatted add
through a tent filter with the samples at pixel centres (k_accum_splat), whose expected stream is splat_ref.expand's.

  nSamples, mean, covariance   the oracle's bits (NaN == NaN, the same infinities) on every path
  the paths among themselves   the same bits on all four images (they share the device's powf)
  gamma <= 1                   no powf: the histogram is the oracle's bit for bit on every path, the splatted one included
  gamma > 1                    every bin within the bound of accum_ref against float64, with U = accum_cases.U_DEVICE = 7
                               (four times the U_ref = 1.68 of the host arithmetic); a bin no sample touches is exactly 0
  onehot                       the histogram written down in accum_cases, exactly

Measured on an MI355X: the device's worst U over all cases and paths is 2.1829 (edges-86-2.2-2.5, the one-shot kernel); on the paths of the
persistent accumulator 1.8841 (specials-85-3-0.7, the same on all four paths), at the default parameters 1.4509; the splatted streams need
no U at all (27 contributions per pixel: the addition term of the bound covers them).  The host arithmetic needs 1.6794.  Every test
prints its own U and a failure names the case, the path, the pixel, the bin and its samples."""
import numpy as np
import pytest

import accum_cases as ac
import accum_ref as ar
import oracle_lib as ol
import splat_ref
from test_gpu_accumulator import bits_equal, dev, host

pytestmark = pytest.mark.gpu

TAGS = ("nSamples", "mean", "covariance", "histogram")
TENT = (2.0, 1.25)                                              # the tent filter of test_gpu_splat.py

_expected = {}


def expected(name, stream=None):
    """(the oracle's four images, the float64 reference, its bound terms) of a case's stream, computed once and shared"""
    if name not in _expected:
        c = ac.get(name.split("@")[0])
        s = ac.stream(c) if stream is None else stream
        r = ar.accumulate(s, c.W, c.H, c.nbins, c.gamma, c.maxval)
        _expected[name] = (ol.oracle_ops()["accumulate"](s, c.W, c.H, c.nbins, c.gamma, c.maxval), r, ar.bound_terms(r))
    return _expected[name]


def run_one_shot(ctx, c):
    H, W, k = c.H, c.W, c.samples.shape[1]
    w = dev(c.weights.reshape(H, W, k)) if c.weights is not None else None
    return host(ctx.accumulate_samples(dev(c.samples.reshape(H, W, k, 3)), w, c.nbins, c.gamma, c.maxval))


def run_dense(ctx, c, passes):
    H, W, k = c.H, c.W, c.samples.shape[1]
    smp = c.samples.reshape(H, W, k, 3)
    w = c.weights.reshape(H, W, k) if c.weights is not None else None
    acc = ctx.accumulator(W, H, c.nbins, c.gamma, c.maxval)
    k0 = 0
    for n in passes:
        acc.add_dense(dev(smp[:, :, k0:k0 + n]), dev(w[:, :, k0:k0 + n]) if w is not None else None)
        k0 += n
    assert k0 == k
    got = host(acc.statistics())
    assert acc.info() == (W * H * k, 0)
    acc.close()
    return got


def run_scattered(ctx, c, batches):
    """sample-major order (every pixel's first sample, then every pixel's second ...), the pixels ascending in even rounds and descending
    in odd ones: a pixel's samples keep their order and lie N apart in the batch"""
    N, k = c.samples.shape[:2]
    order = np.concatenate([np.arange(N) if s % 2 == 0 else np.arange(N)[::-1] for s in range(k)])
    rnd = np.repeat(np.arange(k), N)
    rgb = np.ascontiguousarray(c.samples[order, rnd])
    w = np.ascontiguousarray(c.weights[order, rnd]) if c.weights is not None else None
    pixel = order.astype(np.int32)
    n = N * k
    cuts = sorted({0, min(7, n), n // 3, n // 3 + 1, n}) if batches else [0, n]
    acc = ctx.accumulator(c.W, c.H, c.nbins, c.gamma, c.maxval, capacity=64 if batches else 0)
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        acc.add_samples(dev(pixel[b0:b1]), dev(rgb[b0:b1]), dev(w[b0:b1]) if w is not None else None)
    got = host(acc.statistics())
    assert acc.info() == (n, 0)
    acc.close()
    return got


def check_against_oracle(c, path, got, name=None):
    """-> the U this path needed (0 where the histogram is held to the oracle's bits)"""
    want, r, (A, B, touched) = expected(name or c.name)
    for tag, g, w in zip(TAGS[:3], got, want):
        assert bits_equal(g, w), "%s, %s: %s differs from the host arithmetic" % (c.name, path, tag)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(np.isnan(g), np.isnan(w)), (c.name, path, tag)
    hist = got[3].reshape(r.hist.shape)
    assert np.all(hist[~touched] == 0), "%s, %s: a bin that no sample touches is not 0" % (c.name, path)
    if not c.gamma > 1:
        bad = np.argwhere(hist.view(np.uint32) != want[3].reshape(hist.shape).view(np.uint32))
        assert bad.size == 0, "%s, %s: no powf, yet %d bins differ from the host arithmetic; first %s" % (c.name, path, len(bad), ar.describe(r, tuple(bad[0])))
        return 0.0
    u, at = ar.worst_u(hist, r, (A, B, touched))
    print("%s, %s: device U = %.4f" % (c.name, path, u))
    assert u <= ac.U_DEVICE, "%s, %s: U = %.4f > %d at %s: got %.9g, float64 %.17g" % (c.name, path, u, ac.U_DEVICE, ar.describe(r, at), hist[at], r.hist[at])
    return u


@pytest.mark.parametrize("name", ac.ALL)
def test_every_path_bins_like_the_reference(hipctx, name):
    c = ac.get(name)
    k = c.samples.shape[1]
    got = {"one-shot": run_one_shot(hipctx, c)}
    if c.nbins <= ac.ACCUM_MAX_BINS:
        got["dense, 1 sample per pass"] = run_dense(hipctx, c, [1] * k)
        if k >= ac.STAGE_SPP:
            got["dense, staged"] = run_dense(hipctx, c, [k])
        got["scattered"] = run_scattered(hipctx, c, False)
        got["scattered in batches"] = run_scattered(hipctx, c, True)
    assert len(got) == 1 or len(got) >= 4
    worst = max(check_against_oracle(c, path, g) for path, g in got.items())
    print("%s: worst device U = %.4f over %d paths" % (name, worst, len(got)))
    first = got["one-shot"]
    for path, g in got.items():
        for tag, a, b in zip(TAGS, g, first):
            assert bits_equal(a, b), "%s: %s of '%s' differs from the one-shot kernel's" % (name, tag, path)
    if name in ac.ONEHOT_EXPECTED:
        for path, g in got.items():
            assert np.array_equal(g[3].reshape(c.W * c.H, -1), ac.ONEHOT_EXPECTED[name]), (name, path)


@pytest.mark.parametrize("name", ac.SPLAT)
def test_splatted_path_bins_like_the_reference(hipctx, name):
    """a tent of radii (2, 1.25), every sample at its pixel's centre: each reaches the 3 x 3 pixels around it with the weights of the table"""
    import bcd_amd.hip as bh
    c = ac.get(name)
    table = bh.filter_table("tent", TENT, table_size=16)
    s = ac.stream(c)
    xy = np.ascontiguousarray(np.stack([s[:, 1] + np.float32(0.5), s[:, 0] + np.float32(0.5)], 1))
    rgb, w = np.ascontiguousarray(s[:, 2:5]), np.ascontiguousarray(s[:, 5])
    stream, added, dropped = splat_ref.expand(xy, rgb, w, c.W, c.H, TENT[0], TENT[1], table)
    assert dropped == 0 and stream.shape[0] > 5 * s.shape[0] and len(np.unique(stream[:, 5])) >= 3
    key = name + "@splat"
    expected(key, stream)
    acc = hipctx.accumulator(c.W, c.H, c.nbins, c.gamma, c.maxval)
    acc.set_filter(table, TENT)
    acc.add_splatted(dev(xy), dev(rgb), dev(w))
    got = host(acc.statistics())
    assert acc.info() == (added, dropped)
    acc.close()
    u = check_against_oracle(c, "splatted", got, key)
    print("%s: splatted device U = %.4f" % (name, u))


def test_both_entry_points_refuse_one_bin_and_accept_two(hipctx):
    """the smallest depth is 2 for both (with 2 bins only bins 0 and 1 are touched; with 1 the upper bin would be out of bounds); the
    largest are 85 and 213.  Each refusal is the library's own, by its message"""
    import torch
    import bcd_amd.hip as bh
    smp = torch.zeros((2, 3, 1, 3), dtype=torch.float32, device="cuda")
    for nbins, refusal in ((1, "bad size"), (2, None), (213, None), (214, "more than 213 bins per channel are not supported")):
        if refusal is None:
            hipctx.accumulate_samples(smp, None, nbins)
        else:
            with pytest.raises(bh.BcdHipError, match=refusal):
                hipctx.accumulate_samples(smp, None, nbins)
    for nbins, refusal in ((1, "nb_bins must be >= 2"), (0, "nb_bins must be >= 2"), (2, None), (85, None), (86, "more than 85 bins per channel are not supported")):
        if refusal is None:
            hipctx.accumulator(3, 2, nbins).close()
        else:
            with pytest.raises(bh.BcdHipError, match=refusal):
                hipctx.accumulator(3, 2, nbins)
