"""GPU tests of the persistent device SamplesAccumulator (bcd_hip_accum_*, k_accumulate.hip), its Python and C++ front-ends and raw2bcd:
nSamples / mean / covariance bit for bit against the host class on the same stream (NaN == NaN), histograms to the device powf's
round-off, and bit for bit against the one-shot device kernel, which shares its powf."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bcd_amd", "lib")
TOL = 1e-4


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    nan = np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32))
    return bool(np.all((a == b) | nan))


def hist_close(got, want):
    return float(np.max(np.abs(got - want))) < 2e-5 * max(1.0, float(np.max(want)))


def assert_matches_host(got, want):
    """got / want: (ns, mean, cov, hist); the host class's float operations in the same per-pixel order"""
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and bits_equal(got[2], want[2])
    assert hist_close(got[3], want[3])


def assert_bits(got, want):
    for g, w in zip(got, want):
        assert bits_equal(g, w)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(stats):
    return [t.cpu().numpy() for t in stats]


def stream_of(pixel, rgb, w, W):
    """(n, 6) oracle stream (line, col, r, g, b, w)"""
    pixel = np.asarray(pixel, np.int64)
    return np.ascontiguousarray(np.concatenate([(pixel // W)[:, None], (pixel % W)[:, None], rgb, w[:, None]], 1).astype(np.float32))


def dense_stream(rgb_hwk, w_hwk, row0=0):
    """oracle stream of a dense pass: pixels in order, each pixel's k samples in order"""
    rows, W, k, _ = rgb_hwk.shape
    pix = (np.arange(row0 * W, (row0 + rows) * W)[:, None] * np.ones((1, k), np.int64)).reshape(-1)
    w = np.ones(rows * W * k, np.float32) if w_hwk is None else w_hwk.reshape(-1)
    return stream_of(pix, rgb_hwk[..., :3].reshape(-1, 3), w, W)


def random_samples(rng, shape, spike=0.02):
    """positive radiance with spikes past the histogram's saturation level, and a few zeros"""
    v = (rng.random(shape, dtype=np.float32) * 1.2).astype(np.float32)
    v[rng.random(shape) < spike] *= 9.0
    v[rng.random(shape) < 0.01] = 0.0
    return v


def test_reference_fixture_scattered_in_any_order(hipctx):
    """tests/golden/ref_accumulator.npz (the reference's compiled accumulator; weights 0.5, 1 and 2) through the scattered add:
    in its order, interleaved with each pixel's own order kept, and in five uneven batches through a small fixed capacity"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_accumulator.npz"))
    s, W, H = z["samples"], int(z["W"]), int(z["H"])
    want = (z["ns"], z["mean"], z["cov"], z["hist"])
    n = s.shape[0]
    pixel = (s[:, 0].astype(np.int64) * W + s[:, 1].astype(np.int64)).astype(np.int32)
    assert len(np.unique(z["ns"])) > 1 and set(np.unique(s[:, 5])) >= {0.5, 2.0}    # (6 samples per pixel, weight sums that vary)

    def run(order, splits, capacity=0):
        acc = hipctx.accumulator(W, H, capacity=capacity)
        for b0, b1 in zip(splits[:-1], splits[1:]):
            o = order[b0:b1]
            acc.add_samples(dev(pixel[o]), dev(s[o, 2:5]), dev(s[o, 5]))
        got = host(acc.statistics())
        assert acc.info() == (n, 0)
        acc.close()
        return got

    assert_matches_host(run(np.arange(n), [0, n]), want)
    rng = np.random.default_rng(11)
    pos = rng.permutation(n)                                  # slots of a random order, given back to each pixel's samples in their order
    order = np.empty(n, np.int64)
    order[np.lexsort((np.arange(n), pixel[pos]))] = np.lexsort((np.arange(n), pixel))
    assert not np.array_equal(order, np.arange(n))
    for p in (0, 17, 390):
        assert np.array_equal(order[pixel[order] == p], np.where(pixel == p)[0])
    assert_matches_host(run(order, [0, n]), want)
    assert_matches_host(run(order, [0, 7, 300, 301, 1500, n], capacity=64), want)


@pytest.mark.parametrize("channels,weighted", [(3, False), (4, True)])
def test_progressive_passes_equal_the_one_shot_kernel(hipctx, channels, weighted):
    """spp passes of 1 spp, and passes of 3 + 5 + 1 spp (with the last one in two row bands), give the one-shot kernel's bits on all four
    outputs; 1 + 8 takes the LDS-staged form for the 8"""
    W, H, spp = 61, 37, 9
    rng = np.random.default_rng(channels)
    smp = random_samples(rng, (H, W, spp, channels))
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (H, W, spp)) if weighted else None
    want = host(hipctx.accumulate_samples(dev(smp[..., :3]), dev(w) if weighted else None))

    def passes(sizes, split_last=False):
        acc = hipctx.accumulator(W, H)
        k0 = 0
        for j, k in enumerate(sizes):
            bands = [(0, 20), (20, H)] if split_last and j == len(sizes) - 1 else [(0, H)]
            for r0, r1 in bands:
                acc.add_dense(dev(smp[r0:r1, :, k0:k0 + k]), dev(w[r0:r1, :, k0:k0 + k]) if weighted else None, row0=r0)
            k0 += k
        assert k0 == spp
        got = host(acc.statistics())
        acc.close()
        return got

    assert_bits(passes([1] * spp), want)
    assert_bits(passes([3, 5, 1], split_last=True), want)
    assert_bits(passes([1, 8]), want)


def test_snapshots_are_non_destructive_and_reset_restarts(hipctx):
    W, H, spp = 45, 30, 4
    rng = np.random.default_rng(3)
    smp = random_samples(rng, (H, W, spp, 3))
    acc = hipctx.accumulator(W, H)
    snaps = []
    for k in range(spp):
        acc.add_dense(dev(smp[:, :, k:k + 1]))
        a, b = host(acc.statistics()), host(acc.statistics())
        assert_bits(a, b)
        snaps.append(a)
        assert_bits(a, host(hipctx.accumulate_samples(dev(smp[:, :, :k + 1]))))
    assert np.all(np.isnan(snaps[0][2]))                     # a single unit-weight sample: NaN covariance from the bias factor, as the host class
    acc.reset()
    assert acc.info() == (0, 0)
    for k in range(spp):
        acc.add_dense(dev(smp[:, :, k:k + 1]))
    assert_bits(host(acc.statistics()), snaps[-1])
    assert acc.info() == (W * H * spp, 0)
    acc.close()


def test_adaptive_stream_against_the_host_class(hipctx):
    """dense passes over part of the frame, then weighted scattered extras for a random subset of pixels with out-of-range indices among
    them: the host class on the in-range stream, the dropped ones counted, never-sampled pixels with the host class's NaN bits"""
    W, H = 80, 50
    N = W * H
    rng = np.random.default_rng(5)
    acc = hipctx.accumulator(W, H, capacity=1000)
    parts = []
    for k in range(2):
        p = random_samples(rng, (30, W, 1, 4))
        acc.add_dense(dev(p), row0=10)
        parts.append(dense_stream(p, None, row0=10))
    n = 5000
    pix = rng.choice(N, 900, replace=False)[rng.integers(0, 900, n)].astype(np.int32)
    bad = rng.random(n) < 0.03
    pix[bad] = rng.choice(np.array([-1, -7, N, N + 5, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    rgb = random_samples(rng, (n, 3))
    w = rng.choice(np.array([0.25, 1.0, 3.0], np.float32), n)
    acc.add_samples(dev(pix), dev(rgb), dev(w))
    keep = ~bad
    parts.append(stream_of(pix[keep], rgb[keep], w[keep], W))
    stream = np.concatenate(parts, 0)
    want = ol.oracle_ops()["accumulate"](stream, W, H)
    got = host(acc.statistics())
    assert_matches_host(got, want)
    empty = want[0][..., 0] == 0
    assert empty.sum() > 100
    assert np.array_equal(np.isnan(got[1][empty]), np.isnan(want[1][empty])) and np.array_equal(np.isinf(got[2]), np.isinf(want[2]))
    assert acc.info() == (stream.shape[0], int(bad.sum()))
    acc.close()


def test_end_to_end_on_the_device(hipctx):
    """accumulator -> statistics() -> Context.denoise (3 scales, -m 1 -r 1) with no host copy, against the oracle denoise of the same snapshot"""
    import bcd_amd.hip as bh
    W, H = 128, 96
    rng = np.random.default_rng(9)
    samples, _ = ol.synth_samples(W, H, 8, seed=21, sigma=0.25, spike_prob=0.0)
    rgb = samples[:, 2:5].reshape(H, W, 8, 3)
    acc = hipctx.accumulator(W, H)
    acc.add_dense(dev(rgb[:, :, :4]))
    acc.add_dense(dev(rgb[:, :, 4:]))
    extra = rng.choice(W * H, 3000, replace=False).astype(np.int32)
    x_rgb = np.ascontiguousarray(rgb[extra // W, extra % W, rng.integers(0, 8, 3000)] * np.float32(1.05))
    acc.add_samples(dev(extra), dev(x_rgb))
    ns, mean, cov, hist = acc.statistics()
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    got = hipctx.denoise(mean, ns, hist, cov, 3, prm).cpu().numpy()
    c, n, h, v = host((mean, ns, hist, cov))
    assert n.min() >= 8 and len(np.unique(n)) == 2
    orders, w_, h_ = [], W, H
    for s in range(3):
        orders.append(bh.visit_order(w_, h_, 1, 1, bh.scale_seed(3, s)))
        w_, h_ = w_ // 2, h_ // 2
    want = ol.denoise_multiscale(c, n, h, v, 3, ol.params(m=1.0), orders=orders)
    assert float(np.max(np.abs(got - want)) / np.max(np.abs(want))) < TOL
    acc.close()


def test_full_size_frame_statistics(hipctx):
    """1080p: 4 dense passes of 1 spp and 2 M weighted scattered samples, against the host class on the concatenated stream"""
    W, H = 1920, 1080
    N = W * H
    rng = np.random.default_rng(1080)
    acc = hipctx.accumulator(W, H, capacity=1 << 20)
    parts = []
    for k in range(4):
        p = random_samples(rng, (H, W, 1, 3))
        acc.add_dense(dev(p))
        parts.append(dense_stream(p, None))
    n = 2_000_000
    pix = rng.integers(0, N, n).astype(np.int32)
    rgb = random_samples(rng, (n, 3))
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    acc.add_samples(dev(pix), dev(rgb), dev(w))
    parts.append(stream_of(pix, rgb, w, W))
    got = host(acc.statistics())
    assert acc.info() == (4 * N + n, 0)
    acc.close()
    want = ol.oracle_ops()["accumulate"](np.concatenate(parts, 0), W, H)
    assert_matches_host(got, want)


def test_cpp_device_accumulator_equals_host_class(hipctx):
    """bcd::DeviceSamplesAccumulator::addSample (more than one 2^20-sample batch, a host snapshot midway) against bcd::SamplesAccumulator"""
    import bcd_amd.core as core
    W, H = 200, 100
    samples, _ = ol.synth_samples(W, H, 60, seed=8, sigma=0.5, spike_prob=0.02)
    rng = np.random.default_rng(8)
    samples = np.ascontiguousarray(samples[rng.permutation(samples.shape[0])])
    samples[::5, 5] = 0.5
    samples[::9, 5] = 2.0
    want = core.accumulate(samples, W, H)
    assert_matches_host(core.device_accumulate(samples, W, H, snapshot_at=samples.shape[0] // 3), want)


def test_raw2bcd_streams_a_raw_file(hipctx, tmp_path):
    """raw2bcd in one chunk and in >= 5 chunks: identical files; _hist / _cov equal the host class's statistics, the colour file the
    half-rounded mean, and bcd_cli denoises them"""
    import bcd_amd.core as core
    W, H, spp = 160, 120, 24
    rng = np.random.default_rng(24)
    smp = random_samples(rng, (H, W, spp, 4))
    raw = tmp_path / "frame.raw"
    with open(raw, "wb") as f:
        f.write(struct.pack("<5i", 1, W, H, spp, 4))
        f.write(smp.tobytes())
    exe = os.path.join(LIB, "raw2bcd")
    outs = []
    for name, extra in (("one", []), ("many", ["--chunk-mb", "1"])):
        prefix = str(tmp_path / name)
        r = subprocess.run([exe] + extra + [str(raw), prefix], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        nchunks = int(r.stdout.split("Converted in ")[1].split()[0])
        assert nchunks == 1 if name == "one" else nchunks >= 5
        outs.append(prefix)
    for suffix in (".exr", "_hist.exr", "_cov.exr"):
        assert open(outs[0] + suffix, "rb").read() == open(outs[1] + suffix, "rb").read()
    ns, mean, cov, hist = ol.oracle_ops()["accumulate"](dense_stream(smp, None), W, H)
    hn = core.read_exr(outs[1] + "_hist.exr", True)
    assert hn.shape == (H, W, 61)
    assert bits_equal(hn[..., 60:], ns) and hist_close(hn[..., :60], hist)
    assert bits_equal(core.read_exr(outs[1] + "_cov.exr", True), cov)
    assert bits_equal(core.read_exr(outs[1] + ".exr", False), mean.astype(np.float16).astype(np.float32))
    r = subprocess.run([os.path.join(LIB, "bcd_cli"), "-i", outs[1] + ".exr", "-o", str(tmp_path / "den.exr")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(tmp_path / "den.exr")
