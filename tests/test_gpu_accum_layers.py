"""GPU tests of the accumulator's colour layers (bcd_hip_accum_*_layers, k_accumulate.hip): nine running sums per layer beside the
beauty's state.  Expected values come from the oracle alone: layer k is the mean and covariance of the oracle accumulator (pinned bit
for bit to the reference's compiled accumulator) on the stream with layer k's colours -- for splats the stream of splat_ref.expand.
Every comparison is bit for bit with NaN == NaN; the only tolerance is hist_close for the beauty's histogram against the host class."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import splat_ref
from test_gpu_accumulator import assert_bits, assert_matches_host, bits_equal, dense_stream, dev, host, random_samples, stream_of
from test_gpu_splat import make_stream, tables

pytestmark = pytest.mark.gpu

W, H, L = 61, 37, 3                                           # not multiples of the 32 x 8 splat tile, of 64 or of 256
TOL_SAME = 1e-5                                               # the layered call against the plain call on one build (test_gpu_layers.py)


def oracle(stream, w=W, h=H):
    return ol.oracle_ops()["accumulate"](np.ascontiguousarray(stream, np.float32), w, h)


def with_colours(stream, rgb):
    """the (n, 6) oracle stream with another layer's colours: same pixels, same weights, same order"""
    s = stream.copy()
    s[:, 2:5] = rgb
    return s


def layer_stats(acc):
    return [(m.cpu().numpy(), c.cpu().numpy()) for m, c in acc.layer_statistics()]


def assert_layers(got, wants):
    """got: [(mean, cov)] per layer; wants: the oracle's (ns, mean, cov, hist) per layer"""
    assert len(got) == len(wants)
    for k, ((mean, cov), want) in enumerate(zip(got, wants)):
        assert bits_equal(mean, want[1]), "layer %d: mean" % k
        assert bits_equal(cov, want[2]), "layer %d: covariance" % k


def layers_equal(a, b):
    return all(bits_equal(x[0], y[0]) and bits_equal(x[1], y[1]) for x, y in zip(a, b))


# ---- 1. dense ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels,weighted", [(3, False), (4, True)])
def test_dense_passes(hipctx, channels, weighted):
    """9 spp as [1] * 9, [3, 5, 1] with the last pass in two row bands, and [1, 8] (the beauty's LDS-staged form): every layer equals the
    oracle, the beauty has the bits of an accumulator without layers given the same passes"""
    spp = 9
    rng = np.random.default_rng(100 + channels)
    smp = random_samples(rng, (H, W, spp, channels))
    lay = [random_samples(rng, (H, W, spp, 3)) for _ in range(L)]       # layer_channels = 3 whatever `channels` is
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (H, W, spp)) if weighted else None
    wants = [oracle(dense_stream(l, w)) for l in lay]

    def passes(sizes, split_last=False, layers=L, colours=None):
        acc = hipctx.accumulator(W, H, layers=layers)
        src = smp if colours is None else colours
        k0 = 0
        for j, k in enumerate(sizes):
            bands = [(0, 20), (20, H)] if split_last and j == len(sizes) - 1 else [(0, H)]
            for r0, r1 in bands:
                ll = [dev(l[r0:r1, :, k0:k0 + k]) for l in lay] if layers else None
                acc.add_dense(dev(src[r0:r1, :, k0:k0 + k]), dev(w[r0:r1, :, k0:k0 + k]) if weighted else None, row0=r0, layers=ll)
            k0 += k
        assert k0 == spp and acc.nb_layers() == layers
        got = host(acc.statistics()), (layer_stats(acc) if layers else None)
        assert acc.info() == (W * H * spp, 0)
        acc.close()
        return got

    plain = None
    for sizes, split in (([1] * spp, False), ([3, 5, 1], True), ([1, 8], False)):
        beauty, got = passes(sizes, split)
        assert_layers(got, wants)
        if plain is None:
            plain = passes(sizes, split, layers=0)[0]
        assert_bits(beauty, plain)
    assert_matches_host(plain, oracle(dense_stream(smp, w)))
    # the route INTEGRATION.md documented before: one plain device accumulator per layer, fed the layer's colours
    k = 1
    alone = passes([3, 5, 1], True, layers=0, colours=lay[k])[0]
    assert bits_equal(alone[1], got[k][0]) and bits_equal(alone[2], got[k][1])


def test_dense_layers_of_four_channels(hipctx):
    """layer_channels = 4 beside a 3-channel beauty: the 4th float of a layer's sample is ignored"""
    rng = np.random.default_rng(104)
    smp = random_samples(rng, (H, W, 2, 3))
    lay = [random_samples(rng, (H, W, 2, 4)) for _ in range(L)]
    acc = hipctx.accumulator(W, H, layers=L)
    acc.add_dense(dev(smp), layers=[dev(l) for l in lay])
    assert_layers(layer_stats(acc), [oracle(dense_stream(l, None)) for l in lay])
    acc.close()


# ---- 2. scattered -----------------------------------------------------------------------------------------------------------------------

def test_scattered_batches(hipctx):
    """6 W H samples with indices -1, N and N + 5 mixed in, as one batch and as five uneven batches through capacity = 700"""
    N = W * H
    n = 6 * N
    rng = np.random.default_rng(200)
    pix = rng.integers(0, N, n).astype(np.int32)
    bad = rng.random(n) < 0.03
    pix[bad] = rng.choice(np.array([-1, N, N + 5], np.int64), int(bad.sum())).astype(np.int32)
    assert {-1, N, N + 5} <= set(pix[bad].tolist())
    rgb = random_samples(rng, (n, 3))
    lay = [random_samples(rng, (n, 3)) for _ in range(L)]
    w = rng.choice(np.array([0.25, 1.0, 3.0], np.float32), n)
    keep = ~bad
    base = stream_of(pix[keep], rgb[keep], w[keep], W)
    wants = [oracle(with_colours(base, l[keep])) for l in lay]

    def run(cuts, capacity):
        acc = hipctx.accumulator(W, H, capacity=capacity, layers=L)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            acc.add_samples(dev(pix[b0:b1]), dev(rgb[b0:b1]), dev(w[b0:b1]), layers=[dev(l[b0:b1]) for l in lay])
        got = host(acc.statistics()), layer_stats(acc)
        assert acc.info() == (int(keep.sum()), int(bad.sum()))
        acc.close()
        return got

    beauty1, one = run([0, n], 0)
    assert_layers(one, wants)
    assert_matches_host(beauty1, oracle(base))
    beauty5, five = run([0, 13, 1500, 1501, 6000, n], 700)
    assert layers_equal(five, one) and len(five) == L
    assert_bits(beauty5, beauty1)


# ---- 3. splatted ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cluster", [("gauss", 250), ("tent", 250), ("tent", 3000)])
def test_splatted_streams(hipctx, name, cluster):
    """the Gaussian 1.5 and tent (2, 1.25) streams of test_gpu_splat.make_stream (empty box, a cluster in one cell, dropped samples); the
    cluster of 3000 is more than the splat kernel's staging arrays hold, so the layers go through its un-staged path as well"""
    radius, table = tables()[name]
    rng = np.random.default_rng(300 + cluster)
    n = (4 if cluster == 250 else 2) * W * H
    xy, rgb, w = make_stream(rng, n, cluster=cluster, empty_box=cluster == 250)
    lay = [random_samples(rng, (n, 3)) for _ in range(L)]
    base, added, dropped = splat_ref.expand(xy, rgb, w, W, H, radius[0], radius[1], table)
    assert dropped > 0
    wants = []
    for l in lay:
        s, a, d = splat_ref.expand(xy, l, w, W, H, radius[0], radius[1], table)
        assert (a, d) == (added, dropped)
        wants.append(oracle(s))
    acc = hipctx.accumulator(W, H, layers=L)
    acc.set_filter(table, radius)
    acc.add_splatted(dev(xy), dev(rgb), dev(w), layers=[dev(l) for l in lay])
    beauty, got = host(acc.statistics()), layer_stats(acc)
    assert acc.info() == (added, dropped)                      # (dropped samples are counted once, not once per layer)
    acc.close()
    assert_layers(got, wants)
    assert_matches_host(beauty, oracle(base))
    if cluster == 250 and name == "gauss":                     # five uneven batches through a small capacity: no bit depends on the split
        acc = hipctx.accumulator(W, H, capacity=700, layers=L)
        acc.set_filter(table, radius)
        cuts = [0, 13, 1500, 1501, 6000, n]
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            acc.add_splatted(dev(xy[b0:b1]), dev(rgb[b0:b1]), dev(w[b0:b1]), layers=[dev(l[b0:b1]) for l in lay])
        assert layers_equal(layer_stats(acc), got)
        assert_bits(host(acc.statistics()), beauty)
        assert acc.info() == (added, dropped)
        acc.close()


# ---- 4. fifteen layers --------------------------------------------------------------------------------------------------------------------

def test_fifteen_layers_interleaved_adds(hipctx):
    """33 x 20, 15 layers, each a different scaling of its own random colours; a dense pass, a scattered batch and a splat batch
    interleaved: every slot of the pointer tables, and aliasing between layers"""
    w_, h_, nl = 33, 20, 15
    N = w_ * h_
    radius, table = tables()["gauss"]
    rng = np.random.default_rng(400)
    acc = hipctx.accumulator(w_, h_, capacity=900, layers=nl)
    acc.set_filter(table, radius)
    scale = [np.float32(0.25 + 0.5 * k) for k in range(nl)]
    streams = [[] for _ in range(nl)]

    p = random_samples(rng, (h_, w_, 2, 3))
    wd = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (h_, w_, 2))
    lp = [random_samples(rng, (h_, w_, 2, 3)) * scale[k] for k in range(nl)]
    acc.add_dense(dev(p), dev(wd), layers=[dev(l) for l in lp])
    for k in range(nl):
        streams[k].append(dense_stream(lp[k], wd))

    m = 2500
    pix = rng.integers(-2, N + 2, m).astype(np.int32)
    ok = (pix >= 0) & (pix < N)
    c, ws = random_samples(rng, (m, 3)), rng.choice(np.array([0.25, 1.0, 3.0], np.float32), m)
    lc = [random_samples(rng, (m, 3)) * scale[k] for k in range(nl)]
    acc.add_samples(dev(pix), dev(c), dev(ws), layers=[dev(l) for l in lc])
    for k in range(nl):
        streams[k].append(stream_of(pix[ok], lc[k][ok], ws[ok], w_))

    n = 3 * N
    xy = np.stack([rng.uniform(-2, w_ + 2, n), rng.uniform(-2, h_ + 2, n)], 1).astype(np.float32)
    cs, wsp = random_samples(rng, (n, 3)), rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    lsp = [random_samples(rng, (n, 3)) * scale[k] for k in range(nl)]
    acc.add_splatted(dev(xy), dev(cs), dev(wsp), layers=[dev(l) for l in lsp])
    added = dropped = 0
    for k in range(nl):
        s, added, dropped = splat_ref.expand(xy, lsp[k], wsp, w_, h_, radius[0], radius[1], table)
        streams[k].append(s)

    got = layer_stats(acc)
    assert acc.info() == (h_ * w_ * 2 + int(ok.sum()) + added, int((~ok).sum()) + dropped)
    acc.close()
    assert_layers(got, [oracle(np.concatenate(s, 0), w_, h_) for s in streams])
    assert len({g[0].tobytes() for g in got}) == nl          # (all different)


# ---- 5. states ----------------------------------------------------------------------------------------------------------------------------

def feed_half(acc, rng):
    """a dense pass and a scattered batch with layers"""
    import bcd_amd.hip as bh
    p = random_samples(rng, (H, W, 2, 3))
    acc.add_dense(dev(p), layers=[dev(random_samples(rng, (H, W, 2, 3))) for _ in range(acc.layers)])
    m = 3000
    pix = rng.integers(-1, W * H + 1, m).astype(np.int32)
    acc.add_samples(dev(pix), dev(random_samples(rng, (m, 3))), dev(rng.choice(np.array([0.5, 2.0], np.float32), m)),
                    layers=[dev(random_samples(rng, (m, 3))) for _ in range(acc.layers)])
    info, planes = bh.accum_layers_state_planes(acc.export_layers_state())
    assert (info["width"], info["height"], info["nb_layers"], info["nb_planes"]) == (W, H, acc.layers, 9 * acc.layers)
    return planes


def test_states_merge_import_and_reset(hipctx):
    import bcd_amd.hip as bh
    rng = np.random.default_rng(500)
    a, b = hipctx.accumulator(W, H, layers=L), hipctx.accumulator(W, H, layers=L)
    pa, pb = feed_half(a, rng), feed_half(b, rng)
    sa, sb, la, lb = a.export_state(), b.export_state(), a.export_layers_state(), b.export_layers_state()
    assert la.size == 64 + 36 * L * W * H == a.layers_state_bytes() and a.state_bytes() == 64 + 4 * 71 * W * H
    assert np.any(pa != 0) and not np.array_equal(pa, pb)
    want_planes = pa + pb                                      # one fp32 add per float

    plain_a, plain_b = hipctx.accumulator(W, H), hipctx.accumulator(W, H)          # the main state: what the existing merge gives
    plain_a.import_state(sa)
    plain_b.import_state(sb)
    plain_a.merge(plain_b)
    want_state = plain_a.export_state()
    plain_a.close()
    plain_b.close()

    c = hipctx.accumulator(W, H, layers=L)                      # import into a fresh accumulator reproduces all statistics
    c.import_state(sa)
    c.import_layers_state(la)
    assert_bits(host(c.statistics()), host(a.statistics()))
    assert layers_equal(layer_stats(c), layer_stats(a)) and c.info() == a.info()

    a.merge(b)                                                 # device merge
    assert np.array_equal(a.export_state(), want_state)
    merged = a.export_layers_state()
    assert bits_equal(bh.accum_layers_state_planes(merged)[1], want_planes)
    assert np.array_equal(b.export_state(), sb) and np.array_equal(b.export_layers_state(), lb)
    merged_stats = layer_stats(a)

    os.environ["BCD_HIP_ACCUM_MERGE_COPY"] = "1"               # the chunked-copy path of a cross-device merge
    try:
        c.merge(b)
    finally:
        del os.environ["BCD_HIP_ACCUM_MERGE_COPY"]
    assert np.array_equal(c.export_state(), want_state) and np.array_equal(c.export_layers_state(), merged)

    c.import_state(sa)                                         # merge of the serialised halves equals the device merge
    c.import_layers_state(la)
    c.merge_state(sb)
    c.merge_layers_state(lb)
    assert np.array_equal(c.export_state(), want_state) and np.array_equal(c.export_layers_state(), merged)
    assert layers_equal(layer_stats(c), merged_stats)

    c.reset()
    assert not bh.accum_layers_state_planes(c.export_layers_state())[1].any() and c.info() == (0, 0)

    # refused merges: 3 layers into 2, layers into none (and the reverse); both sides unchanged
    two, none = hipctx.accumulator(W, H, layers=2), hipctx.accumulator(W, H)
    feed_half(two, rng)
    s2, l2, s0 = two.export_state(), two.export_layers_state(), none.export_state()
    for dst, src in ((two, a), (none, a), (a, none)):
        with pytest.raises(bh.BcdHipError, match="rc=-1"):
            dst.merge(src)
    with pytest.raises(bh.BcdHipError, match="rc=-1"):
        two.import_layers_state(merged)                        # a block of another layer count
    with pytest.raises(bh.BcdHipError, match="rc=-1"):
        none.export_layers_state()
    assert np.array_equal(two.export_state(), s2) and np.array_equal(two.export_layers_state(), l2)
    assert np.array_equal(none.export_state(), s0)
    assert np.array_equal(a.export_state(), want_state) and np.array_equal(a.export_layers_state(), merged)
    for x in (a, b, c, two, none):
        x.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_alone(hipctx):
    import bcd_amd.hip as bh
    rng = np.random.default_rng(600)
    radius, table = tables()["gauss"]
    for bad_count in (0, 16, -1):
        if bad_count == 0:                                     # (Python's layers=0 is the plain accumulator: the C entry point)
            h = bh.C.c_void_p()
            rc = bh.lib().bcd_hip_accum_create_layers(hipctx.h, W, H, 20, 2.2, 2.5, 0, 0, bh.C.byref(h))
            assert rc == -1 and not h.value
        else:
            with pytest.raises(bh.BcdHipError, match="rc=-1"):
                hipctx.accumulator(W, H, layers=bad_count)
    lay, plain = hipctx.accumulator(W, H, layers=2), hipctx.accumulator(W, H)
    for acc in (lay, plain):
        acc.set_filter(table, radius)
    feed_half(lay, rng)
    plain.add_dense(dev(random_samples(rng, (H, W, 1, 3))))
    s_lay, l_lay, s_plain = lay.export_state(), lay.export_layers_state(), plain.export_state()
    assert plain.nb_layers() == 0 and lay.nb_layers() == 2

    n = 500
    p = dev(random_samples(rng, (H, W, 1, 3)))
    pix, rgb = dev(rng.integers(0, W * H, n).astype(np.int32)), dev(random_samples(rng, (n, 3)))
    xy = dev(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32))
    two = [rgb, rgb]

    def refused(call):
        with pytest.raises(bh.BcdHipError, match="rc=-1"):
            call()

    refused(lambda: lay.add_dense(p))                           # plain adds on an accumulator with layers
    refused(lambda: lay.add_samples(pix, rgb))
    refused(lambda: lay.add_splatted(xy, rgb))
    plain.layers = 2                                           # (lets the binding build a two-entry list for the plain accumulator)
    refused(lambda: plain.add_dense(p, layers=[p, p]))          # _layers adds on a plain accumulator
    refused(lambda: plain.add_samples(pix, rgb, layers=two))
    refused(lambda: plain.add_splatted(xy, rgb, layers=two))
    refused(lambda: plain.layer_statistics())
    plain.layers = 0
    refused(lambda: lay.add_dense(p, layers=[p, None]))         # a null entry in a pointer list
    refused(lambda: lay.add_samples(pix, rgb, layers=[None, rgb]))
    refused(lambda: lay.add_splatted(xy, rgb, layers=[rgb, None]))
    assert np.array_equal(lay.export_state(), s_lay) and np.array_equal(lay.export_layers_state(), l_lay)
    assert np.array_equal(plain.export_state(), s_plain)

    lay.add_samples(pix, rgb, layers=two)                       # the next valid call works
    plain.add_samples(pix, rgb)
    assert not np.array_equal(lay.export_layers_state(), l_lay) and not np.array_equal(plain.export_state(), s_plain)
    assert len(layer_stats(lay)) == 2
    lay.close()
    plain.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_into_denoise_layers(hipctx):
    """accumulate -> statistics() + layer_statistics() -> denoise_layers at 2 scales with no host copy: every output finite and within
    TOL_SAME of Context.denoise on that layer's own (mean, cov)"""
    import bcd_amd.hip as bh
    We, He, spp = 128, 96, 8
    sa, _ = ol.synth_samples(We, He, spp, seed=31, sigma=0.25, spike_prob=0.0)
    sb, _ = ol.synth_samples(We, He, spp, seed=32, sigma=0.25, spike_prob=0.0)
    la, lb = sa[:, 2:5].reshape(He, We, spp, 3), sb[:, 2:5].reshape(He, We, spp, 3)
    beauty = la + lb
    acc = hipctx.accumulator(We, He, layers=2)
    acc.add_dense(dev(beauty[:, :, :4]), layers=[dev(la[:, :, :4]), dev(lb[:, :, :4])])
    acc.add_dense(dev(beauty[:, :, 4:]), layers=[dev(la[:, :, 4:]), dev(lb[:, :, 4:])])
    ns, mean, cov, hist = acc.statistics()
    layers = [(mean, cov)] + acc.layer_statistics()
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    outs = hipctx.denoise_layers(ns, hist, layers, 2, prm)
    assert len(outs) == 3
    for (m, c), out in zip(layers, outs):
        got = out.cpu().numpy()
        want = hipctx.denoise(m, ns, hist, c, 2, prm).cpu().numpy()
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
        e = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("layer against the plain call: %.3e" % e)
        assert e <= TOL_SAME
    acc.close()


# ---- 8. the C++ class -----------------------------------------------------------------------------------------------------------------------

def test_cpp_device_accumulator_with_layers(hipctx, tmp_path):
    """bcd::DeviceSamplesAccumulator with two layers through the capi driver: runs of batch splats and batch adds in pieces of 4000 calls,
    host snapshots midway, saveState + saveLayers loaded into a second accumulator: its layer statistics equal the oracle"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    Wc, Hc, nl = 90, 50, 2
    radius, table = (1.0, 1.0), bh.filter_table("tent", 1.0, table_size=8)
    rng = np.random.default_rng(800)
    n = 30_000
    kind = (np.arange(n) // 2500) % 3 != 1                     # runs of 2500 calls: splats, plain adds, splats, ...
    calls = np.empty((n, 7), np.float32)
    calls[:, 0] = kind
    calls[:, 1] = np.where(kind, rng.uniform(-1.5, Wc + 1.5, n), rng.integers(-1, Hc + 1, n))
    calls[:, 2] = np.where(kind, rng.uniform(-1.5, Hc + 1.5, n), rng.integers(-1, Wc + 1, n))
    calls[:, 3:6] = random_samples(rng, (n, 3))
    calls[:, 6] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    lay = np.stack([random_samples(rng, (n, 3)) for _ in range(nl)])

    def expected(colours):
        streams, added, dropped = [], 0, 0
        edges = np.flatnonzero(np.diff(kind.astype(np.int8))) + 1
        for seg in np.split(np.arange(n), edges):
            c = calls[seg]
            if kind[seg[0]]:
                s, a, d = splat_ref.expand(c[:, 1:3], colours[seg], c[:, 6], Wc, Hc, radius[0], radius[1], table)
                streams.append(s)
                added, dropped = added + a, dropped + d
            else:
                inside = (c[:, 1] >= 0) & (c[:, 1] < Hc) & (c[:, 2] >= 0) & (c[:, 2] < Wc)
                streams.append(np.ascontiguousarray(np.concatenate([c[inside, 1:3], colours[seg][inside], c[inside, 6:7]], 1)))
                added, dropped = added + int(inside.sum()), dropped + int((~inside).sum())
        return oracle(np.concatenate(streams, 0), Wc, Hc), added, dropped

    want, added, dropped = expected(calls[:, 3:6])
    assert dropped > 0
    beauty, got, counts = core.device_accumulate_layers(calls, lay, Wc, Hc, radius, table, batch=4000, snapshot_at=n // 3,
                                                        state_path=tmp_path / "acc.state", layers_path=tmp_path / "acc.layers")
    assert counts == (added, dropped)
    assert_matches_host(beauty, want)
    assert_layers(got, [expected(lay[k])[0] for k in range(nl)])
    info = bh.accum_layers_state_info(np.fromfile(tmp_path / "acc.layers", np.uint8))
    assert (info["width"], info["height"], info["nb_layers"]) == (Wc, Hc, nl)
    with pytest.raises(RuntimeError):                          # 16 layers: the class is not valid
        core.device_accumulate_layers(calls[:10], np.zeros((16, 10, 3), np.float32), Wc, Hc, radius, table)
