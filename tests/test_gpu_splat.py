"""GPU tests of the splatted add (bcd_hip_accum_set_filter / bcd_hip_accum_add_splatted, k_accum_splat in k_accumulate.hip): samples at
continuous positions through a pixel reconstruction filter.  Expected: splat_ref (the definition in NumPy float32) expands the samples
into the host class's addSample stream, the oracle accumulator (pinned bit for bit to the reference's compiled accumulator) gives the
statistics.  nSamples / mean / covariance bit for bit (NaN == NaN), histograms to the device powf's round-off, counters exact."""
import numpy as np
import pytest

import oracle_lib as ol
import splat_ref
from test_gpu_accumulator import TOL, assert_bits, assert_matches_host, dense_stream, dev, host, random_samples, stream_of

pytestmark = pytest.mark.gpu

W, H = 61, 37                                                 # not multiples of the 32 x 8 tile


def tables():
    import bcd_amd.hip as bh
    return {"gauss": ((1.5, 1.5), bh.filter_table("gaussian", 1.5, 2.0, 16)),
            "tent": ((2.0, 1.25), bh.filter_table("tent", (2.0, 1.25), table_size=16))}


def make_stream(rng, n, cluster=250, empty_box=True):
    """positions over [-2, W + 2) x [-2, H + 2) with an empty region (pixels without contributions) and a cluster in one cell"""
    xy = np.stack([rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n)], 1).astype(np.float32)
    if empty_box:
        hole = (xy[:, 0] > 38) & (xy[:, 0] < 52) & (xy[:, 1] > 20) & (xy[:, 1] < 33)
        xy[hole, 0] -= np.float32(30)
    where = rng.choice(n, cluster, replace=False)
    xy[where] = (np.array([17.0, 9.0]) + rng.random((cluster, 2))).astype(np.float32)
    rgb = random_samples(rng, (n, 3))
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    return xy, rgb, w


def expected(parts, radius, table):
    """parts: ('splat', xy, rgb, w) or ('stream', (m, 6) array) in order -> (oracle statistics, samples added, dropped)"""
    streams, added, dropped = [], 0, 0
    for p in parts:
        if p[0] == "splat":
            s, a, d = splat_ref.expand(p[1], p[2], p[3], W, H, radius[0], radius[1], table)
            streams.append(s)
            added, dropped = added + a, dropped + d
        else:
            streams.append(p[1])
            added += p[1].shape[0]
    return ol.oracle_ops()["accumulate"](np.concatenate(streams, 0), W, H), added, dropped


def splat(acc, xy, rgb, w):
    acc.add_splatted(dev(xy), dev(rgb), dev(w) if w is not None else None)


@pytest.mark.parametrize("name", ["gauss", "tent"])
def test_filtered_stream_against_the_host_class(hipctx, name):
    """Gaussian r = 1.5 and tent rx = 2, ry = 1.25: 4 samples per pixel on average, empty pixels, a cluster of 250 samples in one cell,
    weights 0.5 / 1 / 2; then the same stream in five uneven batches through a small fixed capacity: identical bits"""
    radius, table = tables()[name]
    rng = np.random.default_rng(41)
    n = 4 * W * H
    xy, rgb, w = make_stream(rng, n)
    want, added, dropped = expected([("splat", xy, rgb, w)], radius, table)
    assert dropped > 0 and (want[0][..., 0] == 0).sum() > 20 and len(np.unique(want[0])) > 100

    acc = hipctx.accumulator(W, H)
    acc.set_filter(table, radius)
    splat(acc, xy, rgb, w)
    one = host(acc.statistics())
    assert acc.info() == (added, dropped)
    acc.close()
    assert_matches_host(one, want)

    acc = hipctx.accumulator(W, H, capacity=700)
    acc.set_filter(table, radius)
    cuts = [0, 13, 1500, 1501, 6000, n]
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        splat(acc, xy[b0:b1], rgb[b0:b1], w[b0:b1])
    five = host(acc.statistics())
    assert acc.info() == (added, dropped)
    acc.close()
    assert_bits(five, one)


def test_box_of_radius_half_is_the_scattered_add(hipctx):
    """box r = 0.5 with an all-ones table: every sample goes to the pixel it lies in -- the bits of add_samples on all four outputs"""
    rng = np.random.default_rng(43)
    n = 3 * W * H
    xy = (np.stack([rng.integers(-1, W + 1, n), rng.integers(-1, H + 1, n)], 1) + rng.uniform(0.05, 0.95, (n, 2))).astype(np.float32)
    rgb = random_samples(rng, (n, 3))
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    c, l = np.floor(xy[:, 0]).astype(np.int64), np.floor(xy[:, 1]).astype(np.int64)
    inside = (c >= 0) & (c < W) & (l >= 0) & (l < H)
    pixel = np.where(inside, l * W + c, -1).astype(np.int32)
    a = hipctx.accumulator(W, H)
    a.set_filter(np.ones((4, 4), np.float32), 0.5)
    splat(a, xy, rgb, w)
    b = hipctx.accumulator(W, H)
    b.add_samples(dev(pixel), dev(rgb), dev(w))
    assert_bits(host(a.statistics()), host(b.statistics()))
    assert a.info() == b.info() == (int(inside.sum()), int((~inside).sum()))
    assert 0 < inside.sum() < n
    a.close()
    b.close()


def test_splats_interleaved_with_the_other_adds(hipctx):
    radius, table = tables()["gauss"]
    rng = np.random.default_rng(47)
    acc = hipctx.accumulator(W, H, capacity=5000)
    acc.set_filter(table, radius)
    parts = []
    for k in range(3):
        xy, rgb, w = make_stream(rng, 2 * W * H, cluster=40)
        splat(acc, xy, rgb, w)
        parts.append(("splat", xy, rgb, w))
        if k == 0:
            p = random_samples(rng, (20, W, 2, 3))
            acc.add_dense(dev(p), row0=5)
            parts.append(("stream", dense_stream(p, None, row0=5)))
        if k == 1:
            m = 3000
            pix = rng.integers(0, W * H, m).astype(np.int32)
            c, ww = random_samples(rng, (m, 3)), rng.choice(np.array([0.25, 1.0, 3.0], np.float32), m)
            acc.add_samples(dev(pix), dev(c), dev(ww))
            parts.append(("stream", stream_of(pix, c, ww, W)))
    want, added, dropped = expected(parts, radius, table)
    assert_matches_host(host(acc.statistics()), want)
    assert acc.info() == (added, dropped)
    acc.close()


def test_a_cluster_beyond_the_staging_budget(hipctx):
    """more samples in one cell than a workgroup's staging arrays can hold (64 KiB of LDS, 28 bytes per sample: fewer than 2400): the tiles
    around it read the sorted batch from global memory and give the bits of the definition; a second cluster-free region stays staged"""
    radius, table = tables()["tent"]
    rng = np.random.default_rng(53)
    n = 2 * W * H
    xy, rgb, w = make_stream(rng, n, cluster=3000, empty_box=False)
    want, added, dropped = expected([("splat", xy, rgb, w)], radius, table)
    acc = hipctx.accumulator(W, H)
    acc.set_filter(table, radius)
    splat(acc, xy, rgb, w)
    got = host(acc.statistics())
    assert acc.info() == (added, dropped)
    acc.close()
    assert_matches_host(got, want)


def test_dropped_samples_are_counted_exactly(hipctx):
    """NaN / inf positions, positions outside the extended frame, and a table whose inner ring is zero, so that samples near a pixel
    centre at the frame's border have an empty footprint"""
    table = np.ones((8, 8), np.float32)
    table[:3, :] = 0
    table[:, :3] = 0
    radius = (1.0, 1.0)
    rng = np.random.default_rng(59)
    n = 6000
    xy = np.stack([rng.uniform(-4, W + 4, n), rng.uniform(-4, H + 4, n)], 1).astype(np.float32)
    xy[::50, 0] = np.nan
    xy[7::50, 1] = np.inf
    xy[11::50, 0] = -np.inf
    xy[13::50] = (3.0e9, 5.0)
    xy[17::50] = (-2.5e9, -7.0)
    xy[19::50] = (0.5, 0.5)                                    # a pixel's centre: its own pixel has f = 0, the next ones are a full radius away
    rgb = random_samples(rng, (n, 3))
    want, added, dropped = expected([("splat", xy, rgb, None)], radius, table)
    _, centred, _ = splat_ref.expand(xy[19::50], rgb[19::50], None, W, H, 1.0, 1.0, table)
    assert centred == 0 and dropped > 7 * (n // 50) and added > n // 2
    acc = hipctx.accumulator(W, H)
    acc.set_filter(table, radius)
    splat(acc, xy, rgb, None)
    assert acc.info() == (added, dropped)
    assert_matches_host(host(acc.statistics()), want)
    acc.close()


def test_state_round_trip_between_splats(hipctx):
    radius, table = tables()["gauss"]
    rng = np.random.default_rng(61)
    a1, a2 = make_stream(rng, 3 * W * H, cluster=30), make_stream(rng, 2 * W * H, cluster=30)
    acc = hipctx.accumulator(W, H)
    acc.set_filter(table, radius)
    splat(acc, *a1)
    state = acc.export_state()
    splat(acc, *a2)
    straight, info = host(acc.statistics()), acc.info()
    acc.close()
    fresh = hipctx.accumulator(W, H)
    fresh.import_state(state)
    with pytest.raises(Exception):
        splat(fresh, *a2)                                      # the filter is not part of a state
    fresh.set_filter(table, radius)
    splat(fresh, *a2)
    assert_bits(host(fresh.statistics()), straight)
    assert fresh.info() == info
    fresh.close()


def test_filtered_statistics_feed_the_denoiser_on_the_device(hipctx):
    """>= 16 samples per pixel splatted with the Gaussian, statistics() -> Context.denoise (3 scales) with no host copy, against the oracle
    denoiser on a host copy of that same snapshot: fractional sample counts on every pixel are valid denoiser input"""
    import bcd_amd.hip as bh
    Wd, Hd, spp = 128, 96, 16
    rng = np.random.default_rng(67)
    samples, _ = ol.synth_samples(Wd, Hd, spp, seed=23, sigma=0.25, spike_prob=0.0)
    n = samples.shape[0]
    xy = (samples[:, [1, 0]] + rng.random((n, 2), dtype=np.float32)).astype(np.float32)      # jittered inside the pixel each sample was drawn for
    order = rng.permutation(n)
    acc = hipctx.accumulator(Wd, Hd, capacity=1 << 18)
    acc.set_filter("gaussian", 1.5, param=2.0, table_size=16)
    acc.add_splatted(dev(xy[order]), dev(samples[order, 2:5]))
    ns, mean, cov, hist = acc.statistics()
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    got = hipctx.denoise(mean, ns, hist, cov, 3, prm).cpu().numpy()
    c, nn, h, v = host((mean, ns, hist, cov))
    assert acc.info() == (n, 0)
    assert np.all(np.isfinite(v)) and len(np.unique(nn)) > Wd * Hd // 2 and np.any(nn != np.round(nn))
    orders, w_, h_ = [], Wd, Hd
    for s in range(3):
        orders.append(bh.visit_order(w_, h_, 1, 1, bh.scale_seed(3, s)))
        w_, h_ = w_ // 2, h_ // 2
    want = ol.denoise_multiscale(c, nn, h, v, 3, ol.params(m=1.0), orders=orders)
    assert float(np.max(np.abs(got - want)) / np.max(np.abs(want))) < TOL
    acc.close()


def test_cpp_device_accumulator_splats_and_adds_interleaved(hipctx):
    """bcd::DeviceSamplesAccumulator::splatSample interleaved with addSample, more than one 2^20-sample batch, against the definition"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    Wc, Hc = 200, 100
    radius, table = (1.0, 1.0), bh.filter_table("tent", 1.0, table_size=8)
    rng = np.random.default_rng(71)
    n = (1 << 20) + 150_000
    calls = np.empty((n, 7), np.float32)
    first = (1 << 20) + 50_000                                # splats past a whole batch of the class, then runs of 997 calls: two of
    kind = (np.arange(n) < first) | ((np.arange(n) // 997) % 3 != 0)                         # splats, one of plain adds
    calls[:, 0] = kind
    calls[:, 1] = np.where(kind, rng.uniform(-1.5, Wc + 1.5, n), rng.integers(-1, Hc + 1, n))
    calls[:, 2] = np.where(kind, rng.uniform(-1.5, Hc + 1.5, n), rng.integers(-1, Wc + 1, n))
    calls[:, 3:6] = random_samples(rng, (n, 3))
    calls[:, 6] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    got, counts = core.device_splat(calls, Wc, Hc, radius, table)
    streams, added, dropped = [], 0, 0
    edges = np.flatnonzero(np.diff(kind.astype(np.int8))) + 1
    for seg in np.split(np.arange(n), edges):
        c = calls[seg]
        if kind[seg[0]]:
            s, a, d = splat_ref.expand(c[:, 1:3], c[:, 3:6], c[:, 6], Wc, Hc, radius[0], radius[1], table)
            streams.append(s)
            added, dropped = added + a, dropped + d
        else:
            inside = (c[:, 1] >= 0) & (c[:, 1] < Hc) & (c[:, 2] >= 0) & (c[:, 2] < Wc)
            streams.append(np.ascontiguousarray(c[inside, 1:]))
            added, dropped = added + int(inside.sum()), dropped + int((~inside).sum())
    want = ol.oracle_ops()["accumulate"](np.concatenate(streams, 0), Wc, Hc)
    assert dropped > 0 and counts == (added, dropped)
    assert_matches_host(got, want)
