"""GPU tests of the spike prefilter through a source map (bcd_hip_spike_map / _apply / _filter_layers, bcd_hip_denoise_layers_host_ex).
Maps and gathered images are compared with array_equal on integer / uint32 views -- a gather is a copy of bits.  Only where a whole denoise is compared is
there a tolerance: the layer tests' TOL_SAME (same build: the float atomics of the aggregation arrive in another order) and TOL (the oracle).
  1. the map is the oracle's (finite frames) and bcd_hip_spike_filter's filtered pixel indices (every frame), `moved` counts it;
  2. the gather at every depth / image count / alignment, on random bit patterns between guards, through a hand-made map with chains, a cycle and entries
     outside the frame;
  3. bcd_hip_spike_filter_layers is bcd_hip_spike_filter on the shared images and layer 0, the NumPy gather on the other layers, with and without histograms;
  4. whole frames through the host-buffer call, the C++ library and bcd_cli;
  5. every refusal, and the old call behind the switch;
  6. a kept selection previewed from moments filtered without histograms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import spike_cases as sc
import spike_ref as sr
from test_gpu_layers import TOL, TOL_SAME, dev, frame, orders, rel_linf, split_layers

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
SENTINEL = np.uint32(0xDEADBEEF).view(np.int32)


def ident(H, W):
    return np.arange(W * H, dtype=np.int32).reshape(H, W)


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. the map -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.ALL)
def test_map_is_the_filters_decision(hipctx, name):
    import torch
    col, ns, hist, cov, factor = sc.get(name)
    H, W, _ = col.shape
    d_col, d_hist, d_cov = dev(col, hist, cov)
    d_idx = torch.arange(W * H, dtype=torch.float32, device="cuda").reshape(H, W, 1)
    maps = {}
    for f in (factor, 2.0, 0.5, 1e6):
        M, moved = hipctx.spike_map(d_col, f)
        M = maps[f] = M.cpu().numpy()
        n = int(np.count_nonzero(M != ident(H, W)))
        print("%s factor %g: moved %d of %d" % (name, f, moved, W * H))
        assert moved == n
        filtered_idx = hipctx.spike_filter(d_col, d_idx, d_hist, d_cov, f)[1].cpu().numpy().reshape(H, W)
        assert np.array_equal(M, filtered_idx.astype(np.int32))                   # the source index k_spike copies from, on every frame
        if name in sc.FINITE:
            assert np.array_equal(M, sr.source_map(col, f))
            if f == 1e6:
                assert moved == 0
    M2, none = hipctx.spike_map(d_col, factor, count=False)                       # without the counter
    assert none is None and np.array_equal(M2.cpu().numpy(), maps[factor])


# ---- 2. the gather ----------------------------------------------------------------------------------------------------------------------------------
def handmade_map(W, H, seed):
    """identity, then a third of the entries point anywhere (chains arise), one explicit chain a -> b -> c, one cycle p <-> q, and entries outside the
    frame: -1, W*H, INT32_MAX, INT32_MIN"""
    rng = np.random.default_rng(seed)
    n = W * H
    m = np.arange(n, dtype=np.int64)
    pick = rng.random(n) < 0.33
    m[pick] = rng.integers(0, n, size=int(pick.sum()))
    m[3], m[7], m[11] = 7, 11, 11 + W          # chain
    m[20], m[21] = 21, 20                      # cycle
    m[0], m[W - 1], m[n - 1], m[n - W] = -1, n, np.iinfo(np.int32).max, np.iinfo(np.int32).min
    m[64], m[W] = n + 5, -7                    # first pixel of the second strip, first pixel of the second line
    return m.astype(np.int32).reshape(H, W)


def effective(M):
    H, W = M.shape
    return np.where((M >= 0) & (M < W * H), M, ident(H, W))


def payload(rng, n):
    a = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32)
    a[rng.integers(0, n, size=min(n, 64))] = special[rng.integers(0, special.size, size=min(n, 64))]
    return a.view(np.int32)


GUARD = 64     # ints: 256 bytes, so that the guarded view keeps the allocation's alignment


def guarded(values_or_n, offset):
    """a device int32 buffer [guard | offset | n values | guard] filled with the sentinel, and the view of its n values"""
    import torch
    n = values_or_n if isinstance(values_or_n, int) else values_or_n.size
    buf = torch.full((GUARD + offset + n + GUARD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    view = buf[GUARD + offset:GUARD + offset + n]
    if not isinstance(values_or_n, int):
        view.copy_(torch.from_numpy(values_or_n))
    return buf, view


def guards_intact(buf, offset, n):
    b = buf.cpu().numpy()
    return bool(np.all(b[:GUARD + offset] == SENTINEL) and np.all(b[GUARD + offset + n:] == SENTINEL))


@pytest.mark.parametrize("align", ["aligned", "offset", "mixed"])
@pytest.mark.parametrize("depth", [1, 3, 6, 60, 36, 10])
def test_apply_moves_bits_through_any_map(hipctx, depth, align):
    """65 x 6: one full strip and a last strip of one column per line.  aligned: both bases 16-byte aligned (16-byte accesses when the depth is a multiple of
    4); offset: both one float further; mixed: only the destination is"""
    import torch
    W, H = 65, 6
    n = W * H * depth
    M = handmade_map(W, H, 5)
    d_M = torch.from_numpy(M).cuda()
    eff = effective(M).reshape(-1)
    rng = np.random.default_rng(depth * 7 + len(align))
    so, do = {"aligned": (0, 0), "offset": (1, 1), "mixed": (0, 1)}[align]
    for nimg in (1, 2, 32):
        vals = [payload(rng, n) for _ in range(nimg)]
        srcs = [guarded(v, so) for v in vals]
        dsts = [guarded(n, do) for _ in range(nimg)]
        if align == "aligned":
            assert all(s[1].data_ptr() % 16 == 0 and d[1].data_ptr() % 16 == 0 for s, d in zip(srcs, dsts))
        else:
            assert all(d[1].data_ptr() % 16 == 4 for d in dsts)
        hipctx.spike_apply(d_M, [s[1].view(H, W, depth) for s in srcs], outs=[d[1].view(H, W, depth) for d in dsts])
        hipctx.synchronize()
        for k in range(nimg):
            want = vals[k].reshape(W * H, depth)[eff].reshape(-1)
            assert np.array_equal(dsts[k][1].cpu().numpy(), want), (nimg, k)
            assert guards_intact(dsts[k][0], do, n) and guards_intact(srcs[k][0], so, n), (nimg, k)
            assert np.array_equal(srcs[k][1].cpu().numpy(), vals[k])


def test_apply_on_a_wide_frame_and_a_last_strip_of_two(hipctx):
    """130 x 9 with the map of its own colours: two full strips and a strip of two columns"""
    col, ns, hist, cov, factor = sc.get("130x9")
    M = sr.source_map(col, factor)
    d_M, _ = hipctx.spike_map(dev(col)[0], factor)
    for img in (ns, col, cov, hist):
        out, = hipctx.spike_apply(d_M, dev(img))
        assert np.array_equal(host_bits(out), sr.bits(sr.gather(img, M)))


# ---- 3. the map and the gathers in one call -----------------------------------------------------------------------------------------------------------
def bit_layers(col, cov, L, seed):
    """layer 0: the frame's colours and covariances; the others: random bit patterns (the gather copies bits, whatever they mean)"""
    rng = np.random.default_rng(seed)
    layers = [(col, cov)]
    for _ in range(L - 1):
        layers.append((payload(rng, col.size).view(np.float32).reshape(col.shape), payload(rng, cov.size).view(np.float32).reshape(cov.shape)))
    return layers


def dev_bits(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("L", [1, 2, 4, 16])
@pytest.mark.parametrize("name", ["72x50", "67x3"])
def test_filter_layers_is_the_filter_and_the_gather(hipctx, name, L):
    col, ns, hist, cov, factor = sc.get(name)
    H, W, _ = col.shape
    M = sr.source_map(col, factor)
    layers = bit_layers(col, cov, L, 100 + L)
    d_ns, d_hist = dev(ns, hist)
    d_layers = [(dev_bits(c), dev_bits(v)) for c, v in layers]
    want = hipctx.spike_filter(d_layers[0][0], d_ns, d_hist, d_layers[0][1], factor)          # colours, sample counts, histograms, covariances
    o_ns, o_hist, outs, d_M, moved = hipctx.spike_filter_layers(d_ns, d_hist, d_layers, factor, count=True)
    assert np.array_equal(d_M.cpu().numpy(), M) and moved == int(np.count_nonzero(M != ident(H, W)))
    assert np.array_equal(d_M.cpu().numpy(), hipctx.spike_map(d_layers[0][0], factor)[0].cpu().numpy())
    assert np.array_equal(host_bits(o_ns), host_bits(want[1])) and np.array_equal(host_bits(o_hist), host_bits(want[2]))
    assert np.array_equal(host_bits(outs[0][0]), host_bits(want[0])) and np.array_equal(host_bits(outs[0][1]), host_bits(want[3]))
    for k in range(L):
        assert np.array_equal(host_bits(outs[k][0]), sr.bits(sr.gather(layers[k][0], M))), k
        assert np.array_equal(host_bits(outs[k][1]), sr.bits(sr.gather(layers[k][1], M))), k
    # without histograms: the same sample counts and layers, the map in the context's scratch; the histograms of the call above are not touched
    kept_hist = o_hist.clone()
    n_ns, n_hist, n_outs, n_M = hipctx.spike_filter_layers(d_ns, None, d_layers, factor, own_map=False)
    assert n_hist is None and n_M is None
    assert np.array_equal(host_bits(n_ns), host_bits(o_ns))
    for k in range(L):
        assert np.array_equal(host_bits(n_outs[k][0]), host_bits(outs[k][0])) and np.array_equal(host_bits(n_outs[k][1]), host_bits(outs[k][1])), k
    assert np.array_equal(host_bits(o_hist), host_bits(kept_hist)) and np.array_equal(host_bits(d_hist), sr.bits(hist))


def test_ten_calls_on_one_context_with_changing_sizes():
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        names = ["3x3", "72x50", "67x3", "96x64", "40x28", "130x9", "31x17", "96x64", "3x70", "65x5"]
        for i, name in enumerate(names):
            col, ns, hist, cov, factor = sc.get(name)
            M = sr.source_map(col, factor)
            L = 1 + i % 3
            layers = bit_layers(col, cov, L, i)
            with_hist, own = i % 2 == 0, i % 3 != 0
            r = ctx.spike_filter_layers(dev(ns)[0], dev(hist)[0] if with_hist else None, [(dev_bits(c), dev_bits(v)) for c, v in layers], factor, own_map=own)
            assert np.array_equal(host_bits(r[0]), sr.bits(sr.gather(ns, M))), name
            if with_hist:
                assert np.array_equal(host_bits(r[1]), sr.bits(sr.gather(hist, M))), name
            for k in range(L):
                assert np.array_equal(host_bits(r[2][k][0]), sr.bits(sr.gather(layers[k][0], M))), (name, k)
                assert np.array_equal(host_bits(r[2][k][1]), sr.bits(sr.gather(layers[k][1], M))), (name, k)
            if own:
                assert np.array_equal(r[3].cpu().numpy(), M), name
    finally:
        ctx.close()


# ---- 4. whole frames ----------------------------------------------------------------------------------------------------------------------------------
def whole_frame(name):
    if name == "72x50":
        col, ns, hist, cov = frame(72, 50, 16)
        return col, ns, hist, cov, 2, 3, dict(m=1.0, random_order=1, seed=7)
    from test_gpu_host_stream import frame as stream_frame          # 40 x 256 with D = 60: the smallest frame whose primary layer streams in row chunks
    col, ns, hist, cov = stream_frame(40, 256, 60, 21, False)
    return col, ns, hist, cov, 1, 3, dict(m=1.0, random_order=1, seed=21)


@pytest.mark.parametrize("name", ["72x50", "40x256_streamed"])
def test_host_layers_with_the_prefilter_over_every_layer(hipctx, name):
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    col, ns, hist, cov, S, L, kw = whole_frame(name)
    H, W, D = hist.shape
    prm = bh.default_params(**kw)
    if name != "72x50":
        assert hipctx.selftest_host_stream(col, ns, hist, cov, prm, spike_factor=2.0, stop_after_chunks=0)["chunk_lines"] < H     # it does stream
    layers = split_layers(col, cov, L)
    M = sr.source_map(col, 2.0)
    assert np.count_nonzero(M != ident(H, W)) > 0
    got = hipctx.denoise_layers_host(ns, hist, layers, S, prm, spike_factor=2.0, filter_layers=True)
    # the resident statement: bcd_hip_spike_filter_layers, then bcd_hip_denoise_layers
    d_ns, d_hist = dev(ns, hist)
    f_ns, f_hist, f_layers, d_M = hipctx.spike_filter_layers(d_ns, d_hist, [tuple(dev(c, v)) for c, v in layers], 2.0)
    assert np.array_equal(d_M.cpu().numpy(), M)
    want = [o.cpu().numpy() for o in hipctx.denoise_layers(f_ns, f_hist, f_layers, S, prm)]
    od = orders(W, H, 1, 1, kw["seed"], S)
    op = ol.params(m=1.0)
    g_ns, g_hist = sr.gather(ns, M), sr.gather(hist, M)
    for k, (c, v) in enumerate(layers):
        e = rel_linf(got[k], want[k])
        ref = ol.denoise_multiscale(sr.gather(c, M), g_ns, g_hist, sr.gather(v, M), S, op, orders=od) if S > 1 else \
            ol.denoise_mono(sr.gather(c, M), g_ns, g_hist, sr.gather(v, M), op, order=od[0])
        eo = rel_linf(got[k], ref)
        print("%s layer %d: vs the resident calls %.3e, vs the oracle on gathered inputs %.3e" % (name, k, e, eo))
        assert e <= TOL_SAME
        assert eo < TOL
    plain = hipctx.denoise_host(col, ns, hist, cov, S, prm, spike_factor=2.0)
    e0 = rel_linf(got[0], plain)
    print("%s layer 0 vs denoise_host with the same factor %.3e" % (name, e0))
    assert e0 <= TOL_SAME
    # the same through the C++ library
    ok, outs = core.denoise_layers(layers, ns, hist, nscales=S, m=1.0, random_order=True, seed=kw["seed"], prefilter_factor=2.0, prefilter_layers=True)
    assert ok
    for k in range(L):
        e = rel_linf(outs[k], want[k])
        print("%s layer %d: bcd::Denoiser with setSpikePrefilterLayers vs the resident calls %.3e" % (name, k, e))
        assert e <= TOL_SAME
    assert not core.denoise_layers(layers, ns, hist, nscales=S, prefilter_factor=2.0)[0]          # without the switch: refused as before


def test_bcd_cli_prefilter_layers_end_to_end(hipctx, tmp_path):
    """bcd_cli --layer twice with --prefilter-layers and the default -p 1: every output is the library's result on the filtered inputs after the half-float
    EXR round trip (the comparison of test_bcd_cli_layers_end_to_end)"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 72, 56
    col, ns, hist, cov = core.synthetic_scene(W, H, 16, 21, 0.15, 0.02)
    layers = split_layers(col, cov, 3)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    args, on_disk = [], [(core.read_exr(stem + ".exr", False), cov)]
    for k in (1, 2):
        core.write_exr(stem + "_l%d.exr" % k, layers[k][0], False)
        core.write_exr(stem + "_l%d_cov.exr" % k, layers[k][1], True)
        args += ["--layer", stem + "_l%d.exr" % k, stem + "_l%d_cov.exr" % k, str(tmp_path / ("out_l%d.exr" % k))]
        on_disk.append((core.read_exr(stem + "_l%d.exr" % k, False), layers[k][1]))   # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    r = subprocess.run([exe, "-i", stem + ".exr", "-o", out_path, "-s", "2", "-b", "4", "-m", "0", "--seed", "5", "--prefilter-layers"] + args,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d_ns, d_hist = dev(ns, hist)
    f_ns, f_hist, f_layers, d_M, moved = hipctx.spike_filter_layers(d_ns, d_hist, [tuple(dev(c, v)) for c, v in on_disk], 2.0, count=True)
    assert moved > 0
    want = hipctx.denoise_layers(f_ns, f_hist, f_layers, 2, bh.default_params(b=4, m=0.0, seed=5))
    for k, path in enumerate([out_path, str(tmp_path / "out_l1.exr"), str(tmp_path / "out_l2.exr")]):
        got = core.read_exr(path, False)
        w = hipctx.zero_bad_values(want[k]).cpu().numpy()
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), k
    # -p 0: the flag has no effect
    r0 = subprocess.run([exe, "-i", stem + ".exr", "-o", out_path, "-p", "0", "-s", "2", "-b", "4", "-m", "0", "--seed", "5", "--prefilter-layers"] + args,
                        capture_output=True, text=True)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    unfiltered = hipctx.denoise_layers(d_ns, d_hist, [tuple(dev(c, v)) for c, v in on_disk], 2, bh.default_params(b=4, m=0.0, seed=5))
    w = hipctx.zero_bad_values(unfiltered[1]).cpu().numpy()
    assert np.max(np.abs(core.read_exr(str(tmp_path / "out_l1.exr"), False) - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w)


# ---- 5. refusals, and the old call behind the switch --------------------------------------------------------------------------------------------------
def test_invalid_calls_are_refused_before_any_device_work(hipctx):
    import torch
    import bcd_amd.hip as bh
    col, ns, hist, cov, factor = sc.get("40x28")
    H, W, D = hist.shape
    d_col, d_ns, d_hist, d_cov = dev(col, ns, hist, cov)
    o_col, o_ns, o_hist, o_cov = (torch.empty_like(t) for t in (d_col, d_ns, d_hist, d_cov))
    d_map = torch.empty((H, W), dtype=torch.int32, device="cuda")
    d_moved = torch.empty(1, dtype=torch.int32, device="cuda")
    L = bh.lib()
    VP = C.c_void_p
    p = lambda t: t.data_ptr()
    err = lambda: L.bcd_hip_last_error(hipctx.h).decode()

    def smap(col_=p(d_col), w=W, h=H, map_=p(d_map), moved=p(d_moved)):
        return L.bcd_hip_spike_map(hipctx.h, col_, w, h, 2.0, map_, moved), err()

    def apply(map_=p(d_map), w=W, h=H, depth=3, src=(p(d_col),), dst=(p(o_col),), n=None, null_lists=False):
        s = (VP * max(1, len(src)))(*src)
        d = (VP * max(1, len(dst)))(*dst)
        return L.bcd_hip_spike_apply(hipctx.h, map_, w, h, depth, None if null_lists else s, None if null_lists else d, len(src) if n is None else n), err()

    good = (p(d_col), p(d_cov), p(o_col), p(o_cov))

    def fl(layers=(good,), ns_=p(d_ns), hist_=p(d_hist), w=W, h=H, d=D, ons=p(o_ns), ohist=p(o_hist), n=None, map_=p(d_map), moved=None, null_list=False):
        arr = (bh.SpikeLayer * max(1, len(layers)))()
        for k, (a, b, c, e) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_colors_out, arr[k].d_covariances_out = a, b, c, e
        return L.bcd_hip_spike_filter_layers(hipctx.h, ns_, hist_, w, h, d, 2.0, ons, ohist, None if null_list else arr, len(layers) if n is None else n,
                                             map_, moved), err()

    o_col2, o_cov2 = torch.empty_like(d_col), torch.empty_like(d_cov)
    second = (p(d_col), p(d_cov), p(o_col2), p(o_cov2))
    cases = {
        "map: null colours": smap(col_=None), "map: null map": smap(map_=None), "map: W < 3": smap(w=2), "map: H < 3": smap(h=2),
        "map: beyond 31 bits": smap(w=65536, h=32768), "map: the map is the colours": smap(map_=p(d_col)),
        "map: the counter lies in the map": smap(moved=p(d_map) + 16),
        "apply: null map": apply(map_=None), "apply: null lists": apply(null_lists=True), "apply: null image": apply(src=(None,)),
        "apply: null output": apply(dst=(None,)), "apply: W < 3": apply(w=1), "apply: beyond 31 bits": apply(w=65536, h=32768), "apply: depth 0": apply(depth=0),
        "apply: no image": apply(n=0), "apply: 33 images": apply(src=(p(d_col),) * 33, dst=(p(o_col),) * 33),
        "apply: in place": apply(dst=(p(d_col),)), "apply: output overlaps the input": apply(dst=(p(d_col) + 12 * W,)),
        "apply: output is the map": apply(depth=1, src=(p(d_ns),), dst=(p(d_map),)),
        "apply: two outputs overlap": apply(src=(p(d_col), p(d_col)), dst=(p(o_col), p(o_col))),
        "layers: null sample counts": fl(ns_=None), "layers: null output counts": fl(ons=None), "layers: null layer list": fl(null_list=True),
        "layers: null colours": fl(layers=((None,) + good[1:],)), "layers: null covariance output": fl(layers=(good[:3] + (None,),)),
        "layers: histograms without their output": fl(ohist=None), "layers: histogram output without histograms": fl(hist_=None),
        "layers: no layer": fl(n=0), "layers: 17 layers": fl(layers=(good,) * 17), "layers: H < 3": fl(h=2), "layers: beyond 31 bits": fl(w=65536, h=32768),
        "layers: depth 0": fl(d=0), "layers: in place": fl(layers=((good[0], good[1], good[0], good[3]),)),
        "layers: two layers share an output": fl(layers=(good, good)),
        "layers: an output overlaps the histograms": fl(layers=((good[0], good[1], p(d_hist) + 64, good[3]),)),
        "layers: the map is an output": fl(map_=p(o_ns)), "layers: the counter lies in an input": fl(moved=p(d_ns)),
        "layers: output counts are the input": fl(ons=p(d_ns)),
    }
    for name, (rc, msg) in cases.items():
        assert rc == EINVAL and msg, (name, rc, msg)
    assert "image smaller than 3x3" in smap(w=2)[1] and "image smaller than 3x3" in apply(w=1)[1] and "image smaller than 3x3" in fl(h=2)[1]
    assert fl(layers=(good, second))[0] == 0                                      # ... and a good call goes through, the context is as good as before
    M = sr.source_map(col, factor)
    hipctx.synchronize()
    assert np.array_equal(d_map.cpu().numpy(), M) and np.array_equal(host_bits(o_hist), sr.bits(sr.gather(hist, M)))


def test_the_old_refusal_stays_behind_the_switch(hipctx):
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(72, 50, 16)
    prm = bh.default_params(m=1.0, random_order=1, seed=7)
    layers = split_layers(col, cov, 2)
    with pytest.raises(bh.BcdHipError) as e:
        hipctx.denoise_layers_host(ns, hist, layers, 1, prm, spike_factor=2.0, filter_layers=False)
    assert "rc=%d" % EUNSUPPORTED in str(e.value) and "several layers" in str(e.value)
    # one layer and a factor: bcd_hip_denoise_host_ex, with and without the switch
    want = hipctx.denoise_host(col, ns, hist, cov, 1, prm, spike_factor=2.0)
    for fl in (False, True):
        got, = hipctx.denoise_layers_host(ns, hist, layers[:1], 1, prm, spike_factor=2.0, filter_layers=fl)
        assert rel_linf(got, want) <= TOL_SAME
    # no factor: the switch has nothing to do
    a = hipctx.denoise_layers_host(ns, hist, layers, 1, prm, filter_layers=True)
    b = hipctx.denoise_layers_host(ns, hist, layers, 1, prm)
    for x, y in zip(a, b):
        assert rel_linf(x, y) <= TOL_SAME


# ---- 6. a kept selection, previewed from filtered moments -----------------------------------------------------------------------------------------------
def test_kept_selection_on_a_frame_filtered_without_histograms(hipctx):
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(96, 64, 16)
    S, prm = 3, bh.default_params(m=1.0, random_order=1, seed=11)
    layers = split_layers(col, cov, 4)
    d_ns, d_hist = dev(ns, hist)
    d_layers = [tuple(dev(c, v)) for c, v in layers]
    f_ns, f_hist, f_layers, _ = hipctx.spike_filter_layers(d_ns, d_hist, d_layers, 2.0)
    sel = hipctx.selection()
    try:
        first = [o.cpu().numpy() for o in hipctx.denoise_layers(f_ns, f_hist, f_layers, S, prm, keep=sel)]
        # the preview: sample counts, means and covariances only -- no histogram buffer is passed anywhere
        p_ns, none, p_layers, _ = hipctx.spike_filter_layers(d_ns, None, d_layers, 2.0, own_map=False)
        assert none is None
        outs = sel.denoise(p_layers, ns=p_ns)
        for k in range(4):
            e = rel_linf(outs[k].cpu().numpy(), first[k])
            print("layer %d: preview on the kept selection vs the kept call %.3e" % (k, e))
            assert e <= TOL_SAME
    finally:
        sel.close()
