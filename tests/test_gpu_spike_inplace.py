"""GPU tests of the in-place gather through a source map (bcd_hip_spike_apply_inplace, bcd_hip_spike_filter_layers_inplace; DESIGN 13, "In place").  Every
comparison is array_equal on int32 / uint32 views -- a gather is a copy of bits --, every image sits between sentinel guards that must stay untouched.
  1. every map case of tests/spike_inplace_cases.py at every size, images of depths 1, 3, 6, 7 and 60 in one call, the moved count;
  2. 32 images in one call; images 4 bytes off 16-byte alignment (depths that would otherwise move as 16-byte accesses);
  3. the real map of a spiky frame;
  4. _filter_layers_inplace is bcd_hip_spike_filter_layers, map included, with and without histograms, L = 1 and 4;
  5. two calls on one context, the second with more moved pixels (the staging buffer grows);
  6. every refusal, followed by a call that still works."""
import ctypes as C

import numpy as np
import pytest

import spike_inplace_cases as ic
from test_gpu_spike_layers import SENTINEL, bit_layers, dev_bits, guarded, guards_intact, host_bits, payload

pytestmark = pytest.mark.gpu

EINVAL = -1


def run_case(hipctx, M, depths, offset, seed):
    """the images of `depths` (random bit patterns between guards, `offset` ints off the allocation's alignment) through the map M in ONE call"""
    import torch
    H, W = M.shape
    rng = np.random.default_rng(seed)
    vals = [payload(rng, W * H * d) for d in depths]
    bufs = [guarded(v, offset) for v in vals]
    assert all(b[1].data_ptr() % 16 == 4 * (offset % 4) for b in bufs)
    d_M = torch.from_numpy(M).cuda()
    moved = hipctx.spike_apply_inplace(d_M, [b[1].view(H, W, d) for b, d in zip(bufs, depths)])
    hipctx.synchronize()
    assert moved == ic.moved(M)
    for k, (v, d) in enumerate(zip(vals, depths)):
        want = ic.reference(v.reshape(H, W, d), M).reshape(-1)
        assert np.array_equal(bufs[k][1].cpu().numpy(), want), (k, d)
        assert guards_intact(bufs[k][0], offset, v.size), (k, d)
    assert np.array_equal(d_M.cpu().numpy(), M)                                  # the map is read only


# ---- 1. every case, every size, mixed depths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ic.SIZES)
def test_every_map_case_in_place_with_mixed_depths(hipctx, W, H):
    for i, name in enumerate(ic.CASES):
        run_case(hipctx, ic.make(name, W, H), ic.DEPTHS, 0, 100 * W + i)


# ---- 2. 32 images; off alignment ----------------------------------------------------------------------------------------------------------------------------
def test_32_images_in_one_call(hipctx):
    W, H = 65, 5
    depths = [ic.DEPTHS[k % len(ic.DEPTHS)] for k in range(32)]
    for name in ("permutation", "outside"):
        run_case(hipctx, ic.make(name, W, H), depths, 0, 7)


@pytest.mark.parametrize("W,H", [(65, 5), (130, 7)])
def test_images_four_bytes_off_alignment(hipctx, W, H):
    """depths 4, 8 and 60 move as 16-byte accesses when the image is 16-byte aligned; one int further they take the scalar copies"""
    for name in ("cycle2", "chain", "permutation", "half", "outside"):
        for offset in (1, 0):
            run_case(hipctx, ic.make(name, W, H), (4, 60, 8, 1, 3, 6, 7), offset, 11 + offset)


# ---- 3. the real map ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(len(ic.REAL_SEEDS)))
def test_the_real_map_of_a_spiky_frame(hipctx, s):
    W, H = ic.REAL_SIZE
    M = ic.make("real", W, H, s)
    assert 60 <= ic.moved(M) <= 85
    run_case(hipctx, M, ic.DEPTHS, 0, 31 + s)


# ---- 4. the map and the gather in one call -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_hist", [True, False])
@pytest.mark.parametrize("L", [1, 4])
def test_filter_layers_inplace_is_filter_layers(hipctx, L, with_hist):
    import torch
    col, ns, hist, cov, M = ic.real_frame(ic.REAL_SEEDS[L % 3])
    H, W, D = hist.shape
    layers = bit_layers(col, cov, L, 200 + L)
    d_ns, d_hist = dev_bits(ns), dev_bits(hist) if with_hist else None
    d_layers = [(dev_bits(c), dev_bits(v)) for c, v in layers]
    o_ns, o_hist, outs, d_M, moved = hipctx.spike_filter_layers(d_ns, d_hist, d_layers, 2.0, count=True)
    assert moved == ic.moved(M) > 0 and np.array_equal(d_M.cpu().numpy(), M)
    # in place, every image between guards
    g_ns = guarded(ns.view(np.int32).reshape(-1), 0)
    g_hist = guarded(hist.view(np.int32).reshape(-1), 0) if with_hist else None
    g_layers = [(guarded(np.ascontiguousarray(c).view(np.int32).reshape(-1), 0), guarded(np.ascontiguousarray(v).view(np.int32).reshape(-1), 0)) for c, v in layers]
    f32 = lambda g, d: g[1].view(torch.float32).view(H, W, d)
    for own_map in (True, False):
        if not own_map:                                                          # (a second round from fresh inputs, the map in the context's scratch)
            g_ns[1].copy_(torch.from_numpy(ns.view(np.int32).reshape(-1)))
            if with_hist:
                g_hist[1].copy_(torch.from_numpy(hist.view(np.int32).reshape(-1)))
            for (gc, gv), (c, v) in zip(g_layers, layers):
                gc[1].copy_(torch.from_numpy(np.ascontiguousarray(c).view(np.int32).reshape(-1)))
                gv[1].copy_(torch.from_numpy(np.ascontiguousarray(v).view(np.int32).reshape(-1)))
        i_M, i_moved = hipctx.spike_filter_layers_inplace(f32(g_ns, 1), f32(g_hist, D) if with_hist else None, [(f32(gc, 3), f32(gv, 6)) for gc, gv in g_layers], 2.0,
                                                          own_map=own_map)
        hipctx.synchronize()
        assert i_moved == moved
        assert (i_M is None) == (not own_map) and (i_M is None or np.array_equal(i_M.cpu().numpy(), M))
        assert np.array_equal(host_bits(f32(g_ns, 1)), host_bits(o_ns)) and guards_intact(g_ns[0], 0, ns.size)
        if with_hist:
            assert np.array_equal(host_bits(f32(g_hist, D)), host_bits(o_hist)) and guards_intact(g_hist[0], 0, hist.size)
        for k, (gc, gv) in enumerate(g_layers):
            assert np.array_equal(host_bits(f32(gc, 3)), host_bits(outs[k][0])) and np.array_equal(host_bits(f32(gv, 6)), host_bits(outs[k][1])), k
            assert guards_intact(gc[0], 0, col.size) and guards_intact(gv[0], 0, cov.size), k


# ---- 5. the staging buffer grows ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_on_one_context_the_second_moves_more():
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        W, H = 130, 7
        for i, name in enumerate(("one", "cycle5", "half", "permutation", "identity", "fan_last", "cycle2")):     # 1, 5, ~450, 910, 0, 909, 2 moved pixels
            run_case(ctx, ic.make(name, W, H), ic.DEPTHS, 0, 50 + i)
        run_case(ctx, ic.make("permutation", 40, 28), (60, 60, 60, 60), 0, 99)                                # a larger frame, deeper rows
    finally:
        ctx.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_are_refused_before_any_device_work(hipctx):
    import torch
    import bcd_amd.hip as bh
    col, ns, hist, cov, M = ic.real_frame()
    H, W, D = hist.shape
    d_col, d_ns, d_hist, d_cov = (dev_bits(a) for a in (col, ns, hist, cov))
    d_col2, d_cov2 = dev_bits(col), dev_bits(cov)
    d_map = torch.from_numpy(M).cuda()
    L = bh.lib()
    VP = C.c_void_p
    p = lambda t: t.data_ptr()
    err = lambda: L.bcd_hip_last_error(hipctx.h).decode()
    moved = C.c_int32(-5)

    def apply(map_=p(d_map), w=W, h=H, depths=(3,), images=(p(d_col),), n=None, null_depths=False, null_images=False):
        dd = (C.c_int32 * max(1, len(depths)))(*depths)
        im = (VP * max(1, len(images)))(*images)
        return L.bcd_hip_spike_apply_inplace(hipctx.h, map_, w, h, None if null_depths else dd, None if null_images else im, len(images) if n is None else n,
                                             C.byref(moved)), err()

    good = (p(d_col), p(d_cov))

    def fl(layers=(good,), ns_=p(d_ns), hist_=p(d_hist), w=W, h=H, d=D, n=None, map_=None, null_list=False):
        arr = (bh.SpikeLayerInplace * max(1, len(layers)))()
        for k, (a, b) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances = a, b
        return L.bcd_hip_spike_filter_layers_inplace(hipctx.h, ns_, hist_, w, h, d, 2.0, None if null_list else arr, len(layers) if n is None else n, map_,
                                                     C.byref(moved)), err()

    torch.cuda.synchronize()
    before = [host_bits(t).copy() for t in (d_col, d_ns, d_hist, d_cov)]
    cases = {
        "apply: null map": apply(map_=None), "apply: null depths": apply(null_depths=True), "apply: null image list": apply(null_images=True),
        "apply: null image": apply(images=(None,)), "apply: W < 3": apply(w=2), "apply: H < 3": apply(h=2), "apply: beyond 31 bits": apply(w=65536, h=32768),
        "apply: depth 0": apply(depths=(0,)), "apply: negative depth": apply(depths=(3, -1), images=(p(d_col), p(d_ns))), "apply: no image": apply(n=0),
        "apply: 33 images": apply(depths=(1,) * 33, images=(p(d_ns),) * 33), "apply: the same image twice": apply(depths=(3, 3), images=(p(d_col), p(d_col))),
        "apply: two images overlap": apply(depths=(3, 1), images=(p(d_col), p(d_col) + 64)),
        "apply: an image is the map": apply(depths=(1,), images=(p(d_map),)), "apply: an image overlaps the map": apply(depths=(3, 1), images=(p(d_col), p(d_map) + 16)),
        "layers: null sample counts": fl(ns_=None), "layers: null layer list": fl(null_list=True), "layers: null colours": fl(layers=((None, good[1]),)),
        "layers: null covariances": fl(layers=((good[0], None),)), "layers: no layer": fl(n=0), "layers: 17 layers": fl(layers=(good,) * 17), "layers: W < 3": fl(w=2),
        "layers: H < 3": fl(h=2), "layers: beyond 31 bits": fl(w=65536, h=32768), "layers: histograms with depth 0": fl(d=0),
        "layers: two layers share an image": fl(layers=(good, good)), "layers: colours overlap the histograms": fl(layers=((p(d_hist) + 64, good[1]),)),
        "layers: the map is an image": fl(map_=p(d_ns)), "layers: the map overlaps the histograms": fl(map_=p(d_hist) + 256),
        "layers: sample counts are the colours": fl(ns_=p(d_col)),
    }
    for name, (rc, msg) in cases.items():
        assert rc == EINVAL and msg, (name, rc, msg)
    assert "image smaller than 3x3" in apply(w=2)[1] and "image smaller than 3x3" in fl(h=2)[1]
    hipctx.synchronize()
    assert moved.value == -5                                                     # no refused call wrote the count
    for t, b in zip((d_col, d_ns, d_hist, d_cov), before):
        assert np.array_equal(host_bits(t), b)                                   # ... or an image
    # ... and good calls go through: the context is as good as before
    rc, msg = fl(layers=(good, (p(d_col2), p(d_cov2))), map_=p(d_map))
    assert rc == 0, msg
    hipctx.synchronize()
    assert moved.value == ic.moved(M) and np.array_equal(d_map.cpu().numpy(), M)
    for t, a in ((d_col, col), (d_col2, col), (d_ns, ns), (d_hist, hist), (d_cov, cov), (d_cov2, cov)):
        assert np.array_equal(host_bits(t), ic.reference(np.ascontiguousarray(a), M).view(np.uint32))
    rc, msg = apply(depths=(1, D), images=(p(d_ns), p(d_hist)))                   # once more through the same map: the gather of the gathered images
    assert rc == 0, msg
    hipctx.synchronize()
    assert np.array_equal(host_bits(d_hist), ic.reference(ic.reference(hist, M), M).view(np.uint32))
