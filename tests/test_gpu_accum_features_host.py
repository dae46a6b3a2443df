"""GPU tests of bcd::DeviceSamplesAccumulator with feature channels, through libbcdcore.so (the capi.cpp driver behind
bcd_amd.core.device_accumulate_features): batch adds and batch splats with and without layers against the Python path bit for bit,
getFeatureStatistics, and the saveState / saveFeatures / saveLayers files loaded and merged into a second accumulator."""
import numpy as np
import pytest

import accum_features_ref as fr
from test_gpu_accumulator import assert_bits, bits_equal, dev, host, random_samples

pytestmark = pytest.mark.gpu

W, H = 45, 26
N = W * H


def calls_of(rng, n, run=1500):
    """runs of `run` calls: splats, adds, splats, ...; (kind, a, b, r, g, b, weight) as bcd_amd.core.device_splat takes them"""
    kind = (np.arange(n) // run) % 3 != 1
    calls = np.empty((n, 7), np.float32)
    calls[:, 0] = kind
    calls[:, 1] = np.where(kind, rng.uniform(-1.5, W + 1.5, n), rng.integers(-1, H + 1, n))
    calls[:, 2] = np.where(kind, rng.uniform(-1.5, H + 1.5, n), rng.integers(-1, W + 1, n))
    calls[:, 3:6] = random_samples(rng, (n, 3))
    calls[:, 6] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    return kind, calls


def python_path(hipctx, kind, calls, x, lay, radius, table, Fc, L):
    """the same calls through bcd_amd.hip.Accumulator, run by run -> (accumulator, restatement)"""
    acc = hipctx.accumulator(W, H, layers=L, features=Fc)
    acc.set_filter(table, radius)
    ref = fr.Sums(W, H, Fc)
    edges = np.flatnonzero(np.diff(kind.astype(np.int8))) + 1
    for seg in np.split(np.arange(len(kind)), edges):
        c = calls[seg]
        ll = [dev(lay[k][seg]) for k in range(L)] if L else None
        if kind[seg[0]]:
            acc.add_splatted(dev(c[:, 1:3]), dev(c[:, 3:6]), dev(c[:, 6]), layers=ll, features=dev(x[seg]))
            ref.add_splatted(c[:, 1:3], x[seg], c[:, 6], radius[0], radius[1], table)
        else:
            line, col = c[:, 1].astype(np.int64), c[:, 2].astype(np.int64)
            inside = (line >= 0) & (line < H) & (col >= 0) & (col < W)
            pix = np.where(inside, line * W + col, -1).astype(np.int32)
            acc.add_samples(dev(pix), dev(c[:, 3:6]), dev(c[:, 6]), layers=ll, features=dev(x[seg]))
            ref.add_scattered(pix, x[seg], c[:, 6])
    return acc, ref


@pytest.mark.parametrize("Fc,L", [(3, 0), (8, 2)])
def test_cpp_class_equals_the_python_path(hipctx, tmp_path, Fc, L):
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    radius, table = (1.0, 1.0), bh.filter_table("tent", 1.0, table_size=8)
    rng = np.random.default_rng(9000 + Fc)
    n = 9000
    kind, calls = calls_of(rng, n)
    x = (rng.standard_normal((n, Fc)) * 0.2 + 0.5).astype(np.float32)
    lay = np.stack([random_samples(rng, (n, 3)) for _ in range(L)]) if L else None
    acc, ref = python_path(hipctx, kind, calls, x, lay, radius, table, Fc, L)
    f, v = acc.feature_statistics()
    want_f, want_v = f.cpu().numpy(), v.cpu().numpy()
    snap = ref.snapshot()
    assert bits_equal(want_f, snap["mean"]) and bits_equal(want_v, snap["variance"])
    want_beauty = host(acc.statistics())
    want_layers = [(m.cpu().numpy(), c.cpu().numpy()) for m, c in acc.layer_statistics()] if L else []
    want_counts = acc.info()
    assert want_counts[1] > 0

    # batches of 4000 calls through the pinned batch, no files
    beauty, layers, (gf, gv), counts = core.device_accumulate_features(calls, x, W, H, layer_rgb=lay, radius=radius, table=table, batch=4000)
    assert counts == want_counts
    assert bits_equal(gf, want_f) and bits_equal(gv, want_v)
    assert_bits(beauty, want_beauty)
    for (m, c), (wm, wc) in zip(layers, want_layers):
        assert bits_equal(m, wm) and bits_equal(c, wc)
    assert len(layers) == L

    # saved, loaded into a second accumulator: the same statistics; the files are the Python path's blocks
    paths = dict(state_path=tmp_path / "acc.state", features_path=tmp_path / "acc.features", layers_path=tmp_path / "acc.layers" if L else None)
    beauty, layers, (gf, gv), counts = core.device_accumulate_features(calls, x, W, H, layer_rgb=lay, radius=radius, table=table, **paths)
    assert counts == want_counts and bits_equal(gf, want_f) and bits_equal(gv, want_v)
    assert_bits(beauty, want_beauty)
    blk = np.fromfile(paths["features_path"], np.uint8)
    info = bh.accum_features_state_info(blk)
    assert (info["width"], info["height"], info["nb_features"]) == (W, H, Fc) and np.array_equal(blk, acc.export_features_state())
    assert bits_equal(bh.accum_features_state_planes(blk)[1].reshape(Fc, 2, -1), ref.planes)

    # ... and merged into it once more: every running sum doubles
    beauty, layers, (gf, gv), counts = core.device_accumulate_features(calls, x, W, H, layer_rgb=lay, radius=radius, table=table, merge_again=True, **paths)
    assert counts == (2 * want_counts[0], 2 * want_counts[1])
    twice = fr.snapshot(ref.wsum + ref.wsum, ref.w2sum + ref.w2sum, ref.planes + ref.planes, W, H)
    assert bits_equal(gf, twice["mean"]) and bits_equal(gv, twice["variance"])
    acc.merge_state(acc.export_state())
    acc.merge_features_state(acc.export_features_state())
    if L:
        acc.merge_layers_state(acc.export_layers_state())
        for (m, c), (wm, wc) in zip(layers, acc.layer_statistics()):
            assert bits_equal(m, wm.cpu().numpy()) and bits_equal(c, wc.cpu().numpy())
    assert_bits(beauty[:3], host(acc.statistics())[:3])
    assert_bits([gf, gv], host(acc.feature_statistics()))
    acc.close()


def test_cpp_class_refusals_on_the_device(hipctx):
    """with a device: the counts out of range are not valid, the forms without features and null features are refused with a message and
    move nothing (the driver checks that no refused add was applied)"""
    import bcd_amd.core as core
    for nl, nf in ((0, 0), (0, 9), (16, 2)):
        valid, msg = core.device_features_refusals(nl, nf)
        assert not valid and msg[0]
    for nl in (0, 2):
        valid, msg = core.device_features_refusals(nl, 3)
        assert valid and msg[0] == "" and len(msg) == 6
        assert msg[1].startswith("addSample:") and msg[2].startswith("splatSample:") and msg[3].startswith("addSamples:")
        assert msg[4] == "addSamples: null features" and msg[5] == "splatSamples: null features"
    with pytest.raises(RuntimeError):
        core.device_accumulate_features(np.zeros((4, 7), np.float32), np.zeros((4, 9), np.float32), W, H)
