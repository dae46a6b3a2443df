"""CPU tests of the splatted add's host side: bcd_hip_filter_table against a NumPy double evaluation, the argument checks of
bcd_hip_accum_set_filter / bcd_hip_accum_add_splatted that need no device, and splat_ref (the definition in NumPy, which the GPU tests
compare against) against a plain triple loop."""
import ctypes as C

import numpy as np
import pytest

import bcd_amd.hip as bh
import splat_ref

EINVAL = -1


def factors(kind, r, param, ts):
    """the 1-D factor of a standard filter at d = (i + 0.5) / ts * r, in double"""
    r = float(np.float32(r))
    d = (np.arange(ts) + 0.5) / ts * r
    if kind == "box":
        return np.ones(ts)
    if kind == "tent":
        return np.maximum(0.0, 1.0 - d / r)
    if kind == "gaussian":
        a = float(np.float32(param))
        return np.maximum(0.0, np.exp(-a * d * d) - np.exp(-a * r * r))
    u = (d + r) / (2.0 * r)
    return np.maximum(0.0, 0.35875 - 0.48829 * np.cos(2 * np.pi * u) + 0.14128 * np.cos(4 * np.pi * u) - 0.01168 * np.cos(6 * np.pi * u))


@pytest.mark.parametrize("kind", ["box", "tent", "gaussian", "blackman_harris"])
@pytest.mark.parametrize("radius,ts", [((1.5, 1.5), 16), ((2.0, 0.7), 7), ((3.0, 0.5), 64), ((0.5, 2.25), 1)])
def test_filter_table_against_numpy_double(kind, radius, ts):
    got = bh.filter_table(kind, radius, param=1.7, table_size=ts)
    want = (factors(kind, radius[1], 1.7, ts)[:, None] * factors(kind, radius[0], 1.7, ts)[None, :]).astype(np.float32)   # row = y index
    assert got.shape == (ts, ts) and got.dtype == np.float32 and np.all(np.isfinite(got)) and np.all(got >= 0)
    if kind in ("box", "tent"):
        assert np.array_equal(got, want)
    else:                                                     # libm's and NumPy's exp / cos may differ in the last double bit
        assert np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(want), np.float32(1e-30))))
    assert got.max() > 0
    if ts > 1:
        assert got[0, 0] == got.max() and got[-1, -1] == got.min()                           # all four fall off with the distance


def test_filter_table_refuses_bad_arguments():
    for kw in (dict(radius=0.0), dict(radius=3.5), dict(radius=(1.0, -1.0)), dict(radius=float("nan")), dict(radius=1.0, table_size=0),
               dict(radius=1.0, table_size=65)):
        with pytest.raises(ValueError):
            bh.filter_table("tent", **kw)
    with pytest.raises(ValueError):
        bh.filter_table("mitchell", 2.0)
    with pytest.raises(ValueError):
        bh.filter_table("gaussian", 1.5, param=-1.0)
    L = bh.lib()
    out = np.zeros(16, np.float32)
    assert L.bcd_hip_filter_table(7, 1.0, 1.0, 0.0, 4, out.ctypes.data_as(C.c_void_p)) == EINVAL
    assert L.bcd_hip_filter_table(0, 1.0, 1.0, 0.0, 4, None) == EINVAL
    assert not out.any()


def test_splat_entry_points_refuse_a_null_accumulator():
    """in the manner of test_device_entry_points_fail_loudly_without_gpu: no device is touched, nothing is enqueued"""
    L = bh.lib()
    t = np.ones(4, np.float32)
    assert L.bcd_hip_accum_set_filter(None, 1.0, 1.0, 2, t.ctypes.data_as(C.c_void_p)) == EINVAL
    assert L.bcd_hip_accum_set_filter(None, 1.0, 1.0, 2, None) == EINVAL
    assert L.bcd_hip_accum_add_splatted(None, None, None, None, 0) == EINVAL
    assert L.bcd_hip_accum_add_splatted(None, None, None, None, 5) == EINVAL


def test_splat_ref_equals_the_triple_loop():
    rng = np.random.default_rng(3)
    W, H, n = 7, 5, 400
    xy = np.stack([rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)], 1).astype(np.float32)
    xy[5] = (np.nan, 1.0)
    xy[6] = (2.0, np.inf)
    xy[7] = (3.0, 2.0)                                        # on the grid
    xy[8] = (-1e30, 2.0)
    rgb = rng.random((n, 3), dtype=np.float32)
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    for radius, table in (((1.5, 1.5), bh.filter_table("gaussian", 1.5, 2.0, 16)), ((2.0, 0.75), bh.filter_table("tent", (2.0, 0.75), table_size=5)),
                          ((3.0, 3.0), bh.filter_table("blackman_harris", 3.0, table_size=64))):
        a = splat_ref.expand(xy, rgb, w, W, H, radius[0], radius[1], table, block=64)
        b = splat_ref.expand_loops(xy, rgb, w, W, H, radius[0], radius[1], table)
        assert a[1:] == b[1:] and a[1] + a[2] == n and a[2] >= 4
        assert a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert a[0].shape[0] > 2 * a[1]                        # several pixels per sample
    a = splat_ref.expand(xy, rgb, None, W, H, 1.5, 1.5, bh.filter_table("gaussian", 1.5, 2.0, 16))
    assert np.array_equal(a[0][:, 5], a[0][:, 5].astype(np.float32)) and a[0][:, 5].max() <= 1.0


def test_box_of_radius_half_expands_to_the_pixel_under_the_sample():
    rng = np.random.default_rng(4)
    W, H, n = 9, 6, 500
    xy = np.stack([rng.uniform(-1, W + 1, n), rng.uniform(-1, H + 1, n)], 1).astype(np.float32)
    xy = xy[np.all(xy != np.floor(xy), axis=1)]
    n = xy.shape[0]
    rgb = rng.random((n, 3), dtype=np.float32)
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
    stream, added, dropped = splat_ref.expand(xy, rgb, w, W, H, 0.5, 0.5, np.ones((3, 3), np.float32))
    c, l = np.floor(xy[:, 0]), np.floor(xy[:, 1])
    inside = (c >= 0) & (c < W) & (l >= 0) & (l < H)
    assert (added, dropped) == (int(inside.sum()), int((~inside).sum())) and 0 < dropped < n
    want = np.concatenate([l[inside, None], c[inside, None], rgb[inside], w[inside, None]], 1).astype(np.float32)
    assert np.array_equal(stream.view(np.uint32), want.view(np.uint32))
