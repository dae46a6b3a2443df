"""GPU tests of the accumulator's feature channels (bcd_hip_accum_*_features, k_accum_features.hip): two running sums per channel beside the
beauty's state, snapshotted into the feature and variance images of a guide.  Expected values come from tests/accum_features_ref.py, the
NumPy float32 restatement that tests/test_accum_features_cpu.py pins to the oracle accumulator.  Every comparison of sums and statistics is
bit for bit with NaN == NaN; snapshots are written between sentinel margins, 16-byte aligned and 4 bytes off."""
import os

import numpy as np
import pytest

import accum_features_ref as fr
import guide_cases as gc
import splat_cases as sc
from test_gpu_accumulator import assert_bits, bits_equal, dev, host, random_samples

pytestmark = pytest.mark.gpu

W, H = 61, 37                                                 # not multiples of the 32 x 8 splat tile, of 64 or of 256
N = W * H
CHANNELS = [1, 3, 8]                                          # the template's ends and an odd middle
LAYERS = [0, 2]
MARGIN = 64
SENTINEL = np.float32(-7.25)


def guarded(shape, off=0):
    """a device tensor of `shape` inside a sentinel-filled buffer, `off` floats past a 16-byte aligned margin -> (view, check())"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((MARGIN + off + n + MARGIN,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = buf[MARGIN + off:MARGIN + off + n].view(*shape)

    def check():
        h = buf.cpu().numpy()
        assert (h[:MARGIN + off] == SENTINEL).all() and (h[MARGIN + off + n:] == SENTINEL).all(), "a margin was written"
    return view, check


def dev_off(a, off):
    """the array on the device `off` floats past a 16-byte aligned address (the launcher picks its load width from the pointer)"""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty((a.size + 8,), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def snapshot(acc, off=0, variances=True):
    """feature_statistics into guarded outputs -> (features, variances or None) on the host"""
    Fc = acc.features
    f, cf = guarded((acc.H, acc.W, Fc), off)
    v, cv = guarded((acc.H, acc.W, Fc), off) if variances else (None, lambda: None)
    acc.feature_statistics(out=(f, v))
    acc.ctx.synchronize()
    cf()
    cv()
    return f.cpu().numpy(), (v.cpu().numpy() if variances else None)


def assert_snapshot(acc, ref, what=""):
    want = ref.snapshot()
    for off in (0, 1):
        f, v = snapshot(acc, off)
        assert bits_equal(f, want["mean"]), "%s: feature means (outputs %d floats off)" % (what, off)
        assert bits_equal(v, want["variance"]), "%s: variances of the means (outputs %d floats off)" % (what, off)
        assert np.all(v >= 0) and not np.isnan(v).any() and not np.signbit(v).any()
    f_only, none = snapshot(acc, 0, variances=False)
    assert none is None and bits_equal(f_only, want["mean"])


def planes_of(acc):
    import bcd_amd.hip as bh
    blk = acc.export_features_state()
    info, planes = bh.accum_features_state_planes(blk)
    assert (info["width"], info["height"], info["nb_features"], info["nb_planes"]) == (acc.W, acc.H, acc.features, 2 * acc.features)
    return planes.reshape(acc.features, 2, -1)


def layer_stats(acc):
    return [(m.cpu().numpy(), c.cpu().numpy()) for m, c in acc.layer_statistics()] if acc.layers else []


def assert_beauty_and_layers(acc, plain):
    """the beauty's four statistics, the layers' and info() have the bits of an accumulator without features given the same adds"""
    assert_bits(host(acc.statistics()), host(plain.statistics()))
    for (m, c), (pm, pc) in zip(layer_stats(acc), layer_stats(plain)):
        assert bits_equal(m, pm) and bits_equal(c, pc)
    assert acc.info() == plain.info() and acc.nb_layers() == plain.nb_layers() and plain.nb_features() == 0


def feature_samples(rng, shape):
    """feature-like channels: levels of order 1 of either sign with noise, a few exact zeros"""
    x = (rng.standard_normal(shape) * 0.2 + rng.choice(np.array([-1.5, 0.0, 0.3, 0.8]), shape[-1])).astype(np.float32)
    x[rng.random(shape) < 0.01] = 0.0
    return x


# ---- 1. dense ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels,weighted", [(3, False), (4, True)])
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("Fc", CHANNELS)
def test_dense_passes(hipctx, Fc, L, channels, weighted):
    """9 spp as [1] * 9, [3, 5, 1] with the last pass in two row bands, and [1, 8] (the beauty's LDS-staged form), the feature buffer 16-byte
    aligned, 8 bytes off and 4 bytes off: features and variances equal the restatement, the beauty and the layers have the bits of an
    accumulator without features"""
    spp = 9
    rng = np.random.default_rng(1000 + 10 * Fc + channels)
    smp = random_samples(rng, (H, W, spp, channels))
    lay = [random_samples(rng, (H, W, spp, 3)) for _ in range(L)]
    x = feature_samples(rng, (H, W, spp, Fc))
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (H, W, spp)) if weighted else None
    ref = fr.Sums(W, H, Fc).add_dense(x, w)

    def passes(sizes, split_last, features, off=0):
        acc = hipctx.accumulator(W, H, layers=L, features=Fc if features else 0)
        k0 = 0
        for j, k in enumerate(sizes):
            bands = [(0, 20), (20, H)] if split_last and j == len(sizes) - 1 else [(0, H)]
            for r0, r1 in bands:
                ll = [dev(l[r0:r1, :, k0:k0 + k]) for l in lay] if L else None
                ff = dev_off(x[r0:r1, :, k0:k0 + k], off) if features else None
                acc.add_dense(dev(smp[r0:r1, :, k0:k0 + k]), dev(w[r0:r1, :, k0:k0 + k]) if weighted else None, row0=r0, layers=ll, features=ff)
            k0 += k
        assert k0 == spp and acc.nb_features() == (Fc if features else 0)
        return acc

    first = None
    for (sizes, split), off in zip((([1] * spp, False), ([3, 5, 1], True), ([1, 8], False)), (0, 2, 1)):
        acc, plain = passes(sizes, split, True, off), passes(sizes, split, False)
        assert_snapshot(acc, ref, "%s, features %d floats off" % (sizes, off))
        assert_beauty_and_layers(acc, plain)
        assert acc.info() == (N * spp, 0)
        planes = planes_of(acc)
        assert bits_equal(planes, ref.planes)
        first = planes if first is None else first
        assert bits_equal(planes, first)
        acc.close()
        plain.close()


# ---- 2. scattered -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("Fc", CHANNELS)
def test_scattered_batches(hipctx, Fc, L):
    """6 W H samples with indices -1, N and N + 5 mixed in and 400 of them on one pixel (a long run on one thread), as one batch and as five
    uneven batches through capacity = 700"""
    n = 6 * N
    rng = np.random.default_rng(2000 + Fc)
    pix = rng.integers(0, N, n).astype(np.int32)
    pix[rng.choice(n, 400, replace=False)] = 1234
    bad = rng.random(n) < 0.03
    pix[bad] = rng.choice(np.array([-1, N, N + 5], np.int64), int(bad.sum())).astype(np.int32)
    assert {-1, N, N + 5} <= set(pix[bad].tolist()) and (pix == 1234).sum() > 300
    rgb = random_samples(rng, (n, 3))
    lay = [random_samples(rng, (n, 3)) for _ in range(L)]
    x = feature_samples(rng, (n, Fc))
    w = rng.choice(np.array([0.25, 1.0, 3.0], np.float32), n)
    ref = fr.Sums(W, H, Fc)
    assert ref.add_scattered(pix, x, w) == int(bad.sum())

    def run(cuts, capacity, features, off=0):
        acc = hipctx.accumulator(W, H, capacity=capacity, layers=L, features=Fc if features else 0)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            acc.add_samples(dev(pix[b0:b1]), dev(rgb[b0:b1]), dev(w[b0:b1]), layers=[dev(l[b0:b1]) for l in lay] if L else None,
                            features=dev_off(x[b0:b1], off) if features else None)
        return acc

    cuts = [0, 13, 1500, 1501, 6000, n]
    one, five, plain = run([0, n], 0, True), run(cuts, 700, True, off=1), run(cuts, 700, False)
    assert one.info() == (int((~bad).sum()), int(bad.sum()))   # (dropped once, not once per channel)
    assert_snapshot(one, ref, "one batch")
    assert_snapshot(five, ref, "five batches")
    assert bits_equal(planes_of(one), ref.planes) and bits_equal(planes_of(five), ref.planes)
    assert_beauty_and_layers(one, plain)
    assert_beauty_and_layers(five, plain)
    for a in (one, five, plain):
        a.close()


# ---- 3. splatted ------------------------------------------------------------------------------------------------------------------------

def filters():
    import bcd_amd.hip as bh
    return {"gauss": ((1.5, 1.5), bh.filter_table("gaussian", 1.5, 2.0, 16)), "tent": ((2.0, 2.0), bh.filter_table("tent", 2.0, table_size=16))}


def positions(rng, n, cluster=0, cell=(17.0, 3.0)):
    """positions over [-3, W + 3) x [-3, H + 3): outside the frame with footprints that reach in, outside the extended frame, with empty
    footprints; a region without samples; non-finite ones; `cluster` samples in one cell, spread over the stream"""
    xy = np.stack([rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)], 1).astype(np.float32)
    hole = (xy[:, 0] > 40) & (xy[:, 0] < 52) & (xy[:, 1] > 20) & (xy[:, 1] < 31)
    xy[hole, 0] -= np.float32(30)
    if cluster:
        xy[rng.choice(n, cluster, replace=False)] = (np.array(cell) + rng.random((cluster, 2))).astype(np.float32)
    xy[5], xy[6], xy[7] = (np.nan, 3.0), (4.0, np.inf), (-np.inf, 2.0)
    return xy


def feat_max_staged(ts, Fc):
    """samples the staging arrays of a feature splat workgroup hold at most: the LDS of the beauty's kernel (sc.max_staged) less the table
    and the ring's starts, over 4 (4 + F) bytes per sample"""
    return (65536 - 4 * (ts * ts + 2 * sc.RING_MAX + 4)) // (4 * (4 + Fc))


def tile_ring_totals(xy, contributing, nx, ny):
    """contributing samples in the ring of every 32 x 8 tile (the cells of its pixels plus (nx, ny) on each side), tiles row-major"""
    c, l = np.floor(xy[contributing, 0]).astype(np.int64), np.floor(xy[contributing, 1]).astype(np.int64)
    out = []
    for py0 in range(0, H, 8):
        for px0 in range(0, W, 32):
            out.append(int(((c >= px0 - nx) & (c < px0 + 32 + nx) & (l >= py0 - ny) & (l < py0 + 8 + ny)).sum()))
    return out


@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("Fc", CHANNELS)
@pytest.mark.parametrize("name", ["gauss", "tent"])
def test_splatted_streams(hipctx, name, Fc, L):
    """Gaussian radius 1.5 and tent radius 2 with table_size 16: one batch and five uneven chunks through capacity = 700 equal the restatement,
    pixels without contributions keep their zeros, dropped samples are counted once"""
    radius, table = filters()[name]
    rng = np.random.default_rng(3000 + Fc)
    n = 4 * N
    xy = positions(rng, n, cluster=250)
    rgb, w = random_samples(rng, (n, 3)), rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    lay = [random_samples(rng, (n, 3)) for _ in range(L)]
    x = feature_samples(rng, (n, Fc))
    ref = fr.Sums(W, H, Fc)
    added, dropped = ref.add_splatted(xy, x, w, radius[0], radius[1], table)
    assert dropped > 100 and (ref.wsum == 0).sum() > 20

    def run(cuts, capacity, features, off=0):
        acc = hipctx.accumulator(W, H, capacity=capacity, layers=L, features=Fc if features else 0)
        acc.set_filter(table, radius)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            acc.add_splatted(dev(xy[b0:b1]), dev(rgb[b0:b1]), dev(w[b0:b1]), layers=[dev(l[b0:b1]) for l in lay] if L else None,
                             features=dev_off(x[b0:b1], off) if features else None)
        return acc

    cuts = [0, 13, 1500, 1501, 6000, n]
    one, five, plain = run([0, n], 0, True, off=1), run(cuts, 700, True), run([0, n], 0, False)
    assert one.info() == five.info() == (added, dropped)
    assert_snapshot(one, ref, "one batch")
    assert_snapshot(five, ref, "five chunks")
    assert bits_equal(planes_of(one), ref.planes) and bits_equal(planes_of(five), ref.planes)
    assert_beauty_and_layers(one, plain)
    for a in (one, five, plain):
        a.close()


def test_splat_ring_over_and_under_the_staging_capacity(hipctx):
    """one stream whose first tile's ring holds more samples than the staging arrays take at F = 8 (4 (4 + 8) bytes per sample) and fewer
    than they take at F = 3: at F = 8 that tile reads the sorted batch from global memory, at F = 3 it is staged, every other tile is staged
    in both.  By construction from cap, as accum_add_splatted and bcd_launch_feat_splat compute it.  Both equal the restatement, and the
    first three channels of the F = 8 run have the bits of the F = 3 run fed those channels"""
    radius, table = filters()["gauss"]
    rng = np.random.default_rng(3100)
    n = 3 * N + 600
    xy = positions(rng, n, cluster=600)
    rgb, w = random_samples(rng, (n, 3)), rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    x = feature_samples(rng, (n, 8))
    _, e, _, added, dropped = fr.expand(xy, w, W, H, radius[0], radius[1], table)
    contributing = np.unique(e)
    assert len(contributing) == added
    nx = ny = 1                                               # smallest m with m + 0.5 >= 1.5
    ring = (32 + 2 * nx) * (8 + 2 * ny)
    totals = tile_ring_totals(xy, contributing, nx, ny)
    assert n < 1 << 16                                        # one chunk
    cap = {Fc: min(sc.staging_cap(n, ring, N, 16), feat_max_staged(16, Fc)) for Fc in (3, 8)}
    print("ring totals %s; staging capacity %d at F = 3, %d at F = 8" % (totals, cap[3], cap[8]))
    assert cap[8] == feat_max_staged(16, 8) == 1255 and cap[3] > cap[8] + 400
    assert cap[8] + 100 < totals[0] < cap[3] - 100             # the first tile: global memory at F = 8, staged at F = 3
    assert all(0 < t < cap[8] - 100 for t in totals[1:])       # the others: staged in both
    got = {}
    for Fc in (3, 8):
        ref = fr.Sums(W, H, Fc)
        assert ref.add_splatted(xy, x[:, :Fc], w, radius[0], radius[1], table) == (added, dropped)
        acc = hipctx.accumulator(W, H, features=Fc)
        acc.set_filter(table, radius)
        acc.add_splatted(dev(xy), dev(rgb), dev(w), features=dev(x[:, :Fc]))
        assert acc.info() == (added, dropped)
        assert_snapshot(acc, ref, "F = %d" % Fc)
        got[Fc] = planes_of(acc)
        assert bits_equal(got[Fc], ref.planes)
        acc.close()
    assert bits_equal(got[8][:3], got[3])


# ---- 4. special values ------------------------------------------------------------------------------------------------------------------

def test_special_values(hipctx):
    """an inf depth channel on part of the frame, a NaN sample, a pixel with one sample, a pixel with none and a constant channel: the
    outputs are the restatement's, the variances never negative, NaN or -0"""
    Fc, spp = 3, 6
    rng = np.random.default_rng(4000)
    x = feature_samples(rng, (H, W, spp, Fc))
    x[..., 0] = np.float32(0.3)                               # a constant channel: s2 / n - mean^2 rounds to either side of 0
    x[:, :, :, 0] += (np.arange(W, dtype=np.float32) / np.float32(W))[None, :, None]
    x[5:12, 20:31, :, 2] = np.inf                             # the depth of a sky region
    x[14, 7, 2, 1] = np.nan
    pix = np.repeat(np.arange(N), spp)
    keep = np.ones(N * spp, bool)
    one, none = 3 * W + 4, 30 * W + 50
    keep[one * spp + 1:(one + 1) * spp] = False               # one sample
    keep[none * spp:(none + 1) * spp] = False                 # none
    pix, xs = pix[keep].astype(np.int32), x.reshape(-1, Fc)[keep]
    rgb = random_samples(rng, (len(pix), 3))
    ref = fr.Sums(W, H, Fc).add(pix, xs)
    want = ref.snapshot()
    assert (want["vm"] < 0).any() and np.isnan(want["vm"]).any()                     # the clamp has work to do
    assert want["mean"][5, 20, 2] == np.inf and want["variance"][5, 20, 2] == 0
    assert np.isnan(want["mean"].reshape(N, Fc)[none]).all() and not want["variance"].reshape(N, Fc)[none].any()
    assert np.array_equal(want["mean"].reshape(N, Fc)[one], xs[pix == one][0]) and not want["variance"].reshape(N, Fc)[one].any()
    assert np.isnan(want["mean"][14, 7, 1]) and want["variance"][14, 7, 1] == 0
    acc = hipctx.accumulator(W, H, features=Fc)
    acc.add_samples(dev(pix), dev(rgb), features=dev(xs))
    assert_snapshot(acc, ref)
    acc.close()


# ---- 5. states --------------------------------------------------------------------------------------------------------------------------

def feed_half(acc, rng):
    """a dense pass and a scattered batch"""
    Fc, L = acc.features, acc.layers
    acc.add_dense(dev(random_samples(rng, (H, W, 2, 3))), layers=[dev(random_samples(rng, (H, W, 2, 3))) for _ in range(L)] if L else None,
                  features=dev(feature_samples(rng, (H, W, 2, Fc))) if Fc else None)
    m = 3000
    pix = rng.integers(-1, N + 1, m).astype(np.int32)
    acc.add_samples(dev(pix), dev(random_samples(rng, (m, 3))), dev(rng.choice(np.array([0.5, 2.0], np.float32), m)),
                    layers=[dev(random_samples(rng, (m, 3))) for _ in range(L)] if L else None,
                    features=dev(feature_samples(rng, (m, Fc))) if Fc else None)


@pytest.mark.parametrize("Fc,L", [(3, 0), (8, 2)])
def test_states_merge_import_and_reset(hipctx, Fc, L):
    import bcd_amd.hip as bh
    rng = np.random.default_rng(5000 + Fc)
    mk = lambda: hipctx.accumulator(W, H, layers=L, features=Fc)
    a, b = mk(), mk()
    feed_half(a, rng)
    feed_half(b, rng)
    sa, sb, fa, fb = a.export_state(), b.export_state(), a.export_features_state(), b.export_features_state()
    la, lb = (a.export_layers_state(), b.export_layers_state()) if L else (None, None)
    assert fa.size == 64 + 8 * Fc * N == a.features_state_bytes() and a.state_bytes() == 64 + 4 * 71 * N
    info = bh.accum_features_state_info(fa)
    assert (info["magic"], info["version"], info["header_bytes"], info["width"], info["height"], info["nb_features"], info["nb_planes"]) == \
        (b"BCDACCFT", 1, 64, W, H, Fc, 2 * Fc)
    pa, pb = planes_of(a), planes_of(b)
    assert np.any(pa != 0) and not np.array_equal(pa, pb)
    want_planes = pa + pb                                      # one fp32 add per float
    assert want_planes.dtype == np.float32

    c = mk()                                                  # import into a fresh accumulator: the identical snapshot
    c.import_state(sa)
    c.import_features_state(fa)
    if L:
        c.import_layers_state(la)
    assert_bits(snapshot(c), snapshot(a))
    assert_bits(host(c.statistics()), host(a.statistics()))
    assert c.info() == a.info() and np.array_equal(c.export_features_state(), fa)

    plain_a, plain_b = hipctx.accumulator(W, H), hipctx.accumulator(W, H)          # the main state: what the existing merge gives
    plain_a.import_state(sa)
    plain_b.import_state(sb)
    plain_a.merge(plain_b)
    want_state = plain_a.export_state()
    plain_a.close()
    plain_b.close()

    a.merge(b)                                                 # device merge
    merged = a.export_features_state()
    assert np.array_equal(a.export_state(), want_state) and bits_equal(planes_of(a), want_planes)
    assert np.array_equal(b.export_state(), sb) and np.array_equal(b.export_features_state(), fb)
    merged_layers = a.export_layers_state() if L else None
    merged_snapshot = snapshot(a)

    os.environ["BCD_HIP_ACCUM_MERGE_COPY"] = "1"               # the chunked-copy path of a cross-device merge
    try:
        c.merge(b)
    finally:
        del os.environ["BCD_HIP_ACCUM_MERGE_COPY"]
    assert np.array_equal(c.export_state(), want_state) and np.array_equal(c.export_features_state(), merged)
    assert not L or np.array_equal(c.export_layers_state(), merged_layers)

    c.import_state(sa)                                         # merge of the serialised halves equals the device merge
    c.import_features_state(fa)
    c.merge_state(sb)
    c.merge_features_state(fb)
    if L:
        c.import_layers_state(la)
        c.merge_layers_state(lb)
        assert np.array_equal(c.export_layers_state(), merged_layers)
    assert np.array_equal(c.export_state(), want_state) and np.array_equal(c.export_features_state(), merged)
    assert_bits(snapshot(c), merged_snapshot)

    # refused: a block of another channel count or size, merges between different channel counts; both sides untouched
    other = hipctx.accumulator(W, H, layers=L, features=Fc - 1)
    feed_half(other, rng)
    so, fo = other.export_state(), other.export_features_state()
    none = hipctx.accumulator(W, H, layers=L)
    small = hipctx.accumulator(W - 1, H, features=Fc)
    s_none = none.export_state()
    for call in (lambda: other.import_features_state(merged), lambda: other.merge_features_state(merged), lambda: other.import_features_state(fo[:-4]),
                 lambda: other.import_features_state(np.r_[fo, np.zeros(4, np.uint8)]), lambda: a.import_features_state(small.export_features_state()),
                 lambda: other.import_features_state(sa), lambda: other.merge(a), lambda: a.merge(other), lambda: none.merge(a), lambda: a.merge(none),
                 lambda: none.export_features_state(), lambda: none.features_state_bytes(), lambda: none.import_features_state(merged)):
        with pytest.raises(bh.BcdHipError, match="rc=-1"):
            call()
    assert np.array_equal(other.export_state(), so) and np.array_equal(other.export_features_state(), fo)
    assert np.array_equal(a.export_state(), want_state) and np.array_equal(a.export_features_state(), merged)
    assert np.array_equal(none.export_state(), s_none)
    other.import_features_state(fo)                            # ... and the next valid call works

    c.reset()
    assert not planes_of(c).any() and c.info() == (0, 0)
    f, v = snapshot(c)
    assert np.isnan(f).all() and not v.any()
    for acc in (a, b, c, other, none, small):
        acc.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_alone(hipctx):
    import torch
    import bcd_amd.hip as bh
    C = bh.C
    rng = np.random.default_rng(6000)
    radius, table = filters()["gauss"]
    for nl, nf in ((0, 0), (0, 9), (0, -1), (16, 3), (-1, 3)):  # F outside 1 .. 8, nb_layers outside 0 .. 15
        h = C.c_void_p()
        rc = bh.lib().bcd_hip_accum_create_features(hipctx.h, W, H, 20, 2.2, 2.5, 0, nl, nf, C.byref(h))
        assert rc == -1 and not h.value, (nl, nf)
    with pytest.raises(bh.BcdHipError, match="rc=-1"):
        hipctx.accumulator(W, H, features=9)
    feat, both, lay, plain = (hipctx.accumulator(W, H, features=3), hipctx.accumulator(W, H, layers=2, features=3), hipctx.accumulator(W, H, layers=2),
                              hipctx.accumulator(W, H))
    accs = (feat, both, lay, plain)
    for acc in accs:
        acc.set_filter(table, radius)
        feed_half(acc, rng)
    before = [(acc.export_state(), acc.export_features_state() if acc.features else None, acc.export_layers_state() if acc.layers else None) for acc in accs]
    assert [acc.nb_features() for acc in accs] == [3, 3, 0, 0] and [acc.nb_layers() for acc in accs] == [0, 2, 2, 0]

    n = 500
    p = dev(random_samples(rng, (H, W, 1, 3)))
    pf = dev(feature_samples(rng, (H, W, 1, 3)))
    pix, rgb = dev(rng.integers(0, N, n).astype(np.int32)), dev(random_samples(rng, (n, 3)))
    xf = dev(feature_samples(rng, (n, 3)))
    xy = dev(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32))
    two = [rgb, rgb]
    L = bh.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    list2 = (C.c_void_p * 2)(rgb.data_ptr(), rgb.data_ptr())
    plist2 = (C.c_void_p * 2)(p.data_ptr(), p.data_ptr())
    half = (C.c_void_p * 2)(rgb.data_ptr(), None)
    out_f, out_v = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")

    def refused(call):
        with pytest.raises(bh.BcdHipError, match="rc=-1"):
            call()

    def einval(rc, acc, word):
        msg = L.bcd_hip_last_error(hipctx.h).decode()
        assert rc == -1 and word in msg, (rc, msg)

    for acc in (feat, both):                                   # plain and _layers adds on an accumulator with features
        refused(lambda: acc.add_dense(p))
        refused(lambda: acc.add_samples(pix, rgb))
        refused(lambda: acc.add_splatted(xy, rgb))
        einval(L.bcd_hip_accum_add_dense_layers(acc.h, ptr(p), None, 0, H, 1, 3, plist2, 3), acc, "feature channels")
        einval(L.bcd_hip_accum_add_scattered_layers(acc.h, ptr(pix), ptr(rgb), None, n, list2), acc, "feature channels")
        einval(L.bcd_hip_accum_add_splatted_layers(acc.h, ptr(xy), ptr(rgb), None, n, list2), acc, "feature channels")
    for acc in (lay, plain):                                   # _features adds, statistics and block calls on an accumulator without features
        ll = list2 if acc.layers else None
        einval(L.bcd_hip_accum_add_dense_features(acc.h, ptr(p), None, 0, H, 1, 3, plist2 if acc.layers else None, 3, ptr(pf)), acc, "no feature channels")
        einval(L.bcd_hip_accum_add_scattered_features(acc.h, ptr(pix), ptr(rgb), None, n, ll, ptr(xf)), acc, "no feature channels")
        einval(L.bcd_hip_accum_add_splatted_features(acc.h, ptr(xy), ptr(rgb), None, n, ll, ptr(xf)), acc, "no feature channels")
        einval(L.bcd_hip_accum_feature_statistics(acc.h, ptr(out_f), ptr(out_v)), acc, "no feature channels")
        refused(lambda: acc.feature_statistics())
        refused(lambda: acc.export_features_state())
        refused(lambda: acc.import_features_state(before[0][1]))
        refused(lambda: acc.merge_features_state(before[0][1]))
    for acc in (feat, both):                                   # a null d_features
        ll, pl = (list2, plist2) if acc.layers else (None, None)
        einval(L.bcd_hip_accum_add_dense_features(acc.h, ptr(p), None, 0, H, 1, 3, pl, 3, None), acc, "null features")
        einval(L.bcd_hip_accum_add_scattered_features(acc.h, ptr(pix), ptr(rgb), None, n, ll, None), acc, "null features")
        einval(L.bcd_hip_accum_add_splatted_features(acc.h, ptr(xy), ptr(rgb), None, n, ll, None), acc, "null features")
    # a layer list without layers, none with them, a null entry
    einval(L.bcd_hip_accum_add_dense_features(feat.h, ptr(p), None, 0, H, 1, 3, plist2, 3, ptr(pf)), feat, "without layers")
    einval(L.bcd_hip_accum_add_scattered_features(feat.h, ptr(pix), ptr(rgb), None, n, list2, ptr(xf)), feat, "without layers")
    einval(L.bcd_hip_accum_add_splatted_features(feat.h, ptr(xy), ptr(rgb), None, n, list2, ptr(xf)), feat, "without layers")
    einval(L.bcd_hip_accum_add_dense_features(both.h, ptr(p), None, 0, H, 1, 3, None, 3, ptr(pf)), both, "null layer list")
    einval(L.bcd_hip_accum_add_scattered_features(both.h, ptr(pix), ptr(rgb), None, n, None, ptr(xf)), both, "null layer list")
    einval(L.bcd_hip_accum_add_splatted_features(both.h, ptr(xy), ptr(rgb), None, n, None, ptr(xf)), both, "null layer list")
    refused(lambda: both.add_samples(pix, rgb, features=xf))
    einval(L.bcd_hip_accum_add_scattered_features(both.h, ptr(pix), ptr(rgb), None, n, half, ptr(xf)), both, "null layer samples")
    refused(lambda: both.add_splatted(xy, rgb, layers=[None, rgb], features=xf))
    refused(lambda: both.add_dense(p, layers=[p, None], features=pf))
    # feature_statistics: a null output, equal outputs, overlapping outputs
    big = torch.empty((2 * N * 3,), device="cuda")
    einval(L.bcd_hip_accum_feature_statistics(feat.h, None, ptr(out_v)), feat, "null output")
    einval(L.bcd_hip_accum_feature_statistics(feat.h, ptr(out_f), ptr(out_f)), feat, "overlap")
    einval(L.bcd_hip_accum_feature_statistics(feat.h, C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 4 * (N * 3 - 1))), feat, "overlap")
    einval(L.bcd_hip_accum_feature_statistics(feat.h, C.c_void_p(big.data_ptr() + 4 * 5), C.c_void_p(big.data_ptr())), feat, "overlap")
    assert L.bcd_hip_accum_feature_statistics(feat.h, C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 4 * N * 3)) == 0   # back to back is fine
    # malformed blocks
    blk = before[0][1]
    bad = blk.copy()
    bad[8] = 2
    for b in (bad, blk[:-4], blk[:64], before[0][0]):
        refused(lambda: feat.import_features_state(b))
        refused(lambda: feat.merge_features_state(b))
    # nothing moved
    for acc, (s, f, l) in zip(accs, before):
        assert np.array_equal(acc.export_state(), s)
        assert f is None or np.array_equal(acc.export_features_state(), f)
        assert l is None or np.array_equal(acc.export_layers_state(), l)
    # each kind of call still works on the same context
    feat.add_samples(pix, rgb, features=xf)
    both.add_splatted(xy, rgb, layers=two, features=xf)
    lay.add_samples(pix, rgb, layers=two)
    plain.add_dense(p)
    for acc, (s, f, l) in zip(accs, before):
        assert not np.array_equal(acc.export_state(), s)
        assert f is None or not np.array_equal(acc.export_features_state(), f)
    assert len(feat.feature_statistics()) == 2
    for acc in accs:
        acc.close()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------

def test_end_to_end_into_the_guided_denoise(hipctx):
    """64 x 44, 8 spp: feature samples with per-sample noise (the two-region scene of tests/guide_cases.py) are accumulated beside the
    radiance, the snapshot goes into similarity_masks_guide and denoise_guided with and without variances.  The snapshot has the restatement's
    bits and so have the masks made from it; no pair lies across the region edge; the outputs are those of the same call fed the
    restatement's arrays by the project's bar for two runs on one build (TOL_SAME: the aggregation's float atomics arrive in an order that
    differs from run to run, so two runs on identical bits already differ in the last bits).  A neutral one-region
    feature gates nothing: the gated call equals the ungated one"""
    import bcd_amd.hip as bh
    import oracle_lib as ol
    from test_gpu_layers import TOL_SAME, rel_linf
    We, He, spp, Fc = 64, 44, 8, 3
    rng = np.random.default_rng(7000)
    s, _ = ol.synth_samples(We, He, spp, seed=31, sigma=0.25, spike_prob=0.0)
    rad = np.ascontiguousarray(s[:, 2:5].reshape(He, We, spp, 3))
    _, _, signal = gc.features(We, He, Fc, seed=7)
    x = (signal[:, :, None, :] + 0.05 * np.sqrt(spp) * rng.standard_normal((He, We, spp, Fc))).astype(np.float32)
    acc = hipctx.accumulator(We, He, features=Fc)
    acc.add_dense(dev(rad[:, :, :3]), features=dev(x[:, :, :3]))
    acc.add_dense(dev(rad[:, :, 3:]), features=dev(x[:, :, 3:]))
    ns, mean, cov, hist = acc.statistics()
    f, v = acc.feature_statistics()
    hipctx.synchronize()
    want = fr.Sums(We, He, Fc).add_dense(x).snapshot()
    assert bits_equal(f.cpu().numpy(), want["mean"]) and bits_equal(v.cpu().numpy(), want["variance"])
    assert 0.5 * 0.05 ** 2 < float(np.median(want["variance"])) < 2 * 0.05 ** 2       # the variance of the mean of 8 samples of sigma 0.05 sqrt(8)
    rf, rv = dev(want["mean"]), dev(want["variance"])
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    w, b = prm.patch_radius, prm.search_radius
    across = gc.across_pairs(We, He, w, b)
    for with_var in (True, False):
        fl = gc.floors(Fc, with_var)
        vv, rvv = (v, rv) if with_var else (None, None)
        mask, cnt = hipctx.similarity_masks_guide(f, vv, fl, 1.0, w, b)
        rmask, rcnt = hipctx.similarity_masks_guide(rf, rvv, fl, 1.0, w, b)
        hipctx.synchronize()
        assert np.array_equal(mask.cpu().numpy(), rmask.cpu().numpy()) and np.array_equal(cnt.cpu().numpy(), rcnt.cpu().numpy())
        bits = gc.mask_bits(mask.cpu().numpy(), b)
        n_across = int((bits & across).sum())
        print("%s variances: %d similar pairs, %d across the region edge" % ("with" if with_var else "without", int(bits.sum()), n_across))
        assert n_across == 0 and bits.sum() > across.shape[1] * across.shape[2]
        got = hipctx.denoise_guided(ns, hist, [(mean, cov)], 2, prm, f, vv, fl, 1.0)[0].cpu().numpy()
        ref = hipctx.denoise_guided(ns, hist, [(mean, cov)], 2, prm, rf, rvv, fl, 1.0)[0].cpu().numpy()
        e = rel_linf(got, ref)
        print("%s variances: against the call fed the restatement's arrays %.3e (bit for bit: %s)" % ("with" if with_var else "without", e,
                                                                                                     np.array_equal(got, ref)))
        assert np.all(np.isfinite(got)) and e <= TOL_SAME
    plain = hipctx.denoise_layers(ns, hist, [(mean, cov)], 2, prm)[0].cpu().numpy()
    assert rel_linf(got, plain) > 1e-3                        # the gate changed the result
    acc.close()
    # neutral: one region, the same finite constants in every sample of every pixel (floors 1, no variances): every term is 0
    const = np.empty((He, We, spp, 2), np.float32)
    const[..., 0], const[..., 1] = 0.5, -2.0
    acc = hipctx.accumulator(We, He, features=2)
    acc.add_dense(dev(rad), features=dev(const))
    nf, nv = acc.feature_statistics()
    hipctx.synchronize()
    assert np.array_equal(nf.cpu().numpy(), const[:, :, 0]) and not nv.cpu().numpy().any()
    assert_bits(host(acc.statistics()), [t.cpu().numpy() for t in (ns, mean, cov, hist)])
    neutral = hipctx.denoise_guided(ns, hist, [(mean, cov)], 2, prm, nf, None, (1.0, 1.0), 1.0)[0].cpu().numpy()
    e = rel_linf(neutral, plain)
    print("neutral guide against the unguided call %.3e" % e)
    assert e <= TOL_SAME
    acc.close()
