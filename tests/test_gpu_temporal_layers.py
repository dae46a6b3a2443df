"""GPU tests of the colour layers of a frame denoised with its neighbour frames (bcd_hip_denoise_temporal_layers[_host]; DESIGN 16, "Layers") against the
float64 composition of tests/temporal_ref.py run on each layer alone (tests/temporal_layers_ref.py).

Frames from oracle_lib.synth_inputs at 32 spp, one seed per frame as in tests/test_gpu_temporal.py, at 64x44 and 72x48 (why not at that file's sizes:
tests/temporal_layers_cases.py), L = 3: the frame itself and a smooth and a textured share of it, the same shares in every frame.
  * S in {1, 2} x F in {1, 2} x (m, r) in {(1, 1), (0, 0)}: the per-scale processed / fallback / similar_total equal the reference's, every layer is within
    the project's frame bar -- 1e-4 relative L-inf -- of its float64 reference; the measured value is printed;
  * every layer within the same bar of a separate bcd_hip_denoise_temporal call on that layer, the per-scale figures identical; the per-layer redo counts
    (bcd_hip_layer_spectral_inverses) add up to the scale's figure;
  * F = 0 equals bcd_hip_denoise_layers, L = 1 equals bcd_hip_denoise_temporal;
  * the host entry point returns the device call's layers;
  * bcd::Denoiser / bcd::MultiscaleDenoiser with addLayer beside addNeighbourFrame + addNeighbourFrameLayer return the device call's layers;
    clearNeighbourFrames() gives the plain layered call again; a neighbour with a missing layer is refused;
  * bcd_cli --neighbour-layer end to end (the half-float comparison of the other CLI tests); a miscounted --neighbour-layer is an argument error;
  * a plain bcd_hip_denoise_temporal and a bcd_hip_denoise_layers after the layered call equal a fresh context's;
  * the stage timers, width, height and cu_share of every scale of the frame call and of the layered call, with profiling on and off;
  * every refusal of the frame call, then a successful call on the same context."""
import numpy as np
import pytest

import temporal_layers_cases as tl

pytestmark = pytest.mark.gpu

TOL = 1e-4        # relative to the layer's maximum (README / DESIGN 6)
L = tl.L_WHOLE


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def rel_linf(got, want):
    """relative L-inf over the values that are finite in `want`; the non-finite patterns must agree"""
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "non-finite pattern differs"
    return float(np.max(np.abs(np.where(ok, got, 0) - np.where(ok, want, 0))) / np.max(np.abs(np.where(ok, want, 0))))


def params(m, r, seed=1234):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=seed)


_dev = {}


def dev_frames(W, H):
    """the three frames on the device: [(ns, hist, [(colours, covariances)] * L)]"""
    if (W, H) not in _dev:
        _dev[(W, H)] = [(_t(ns), _t(hist), [(_t(c), _t(v)) for c, v in lay]) for ns, hist, lay in tl.frames_of(W, H)]
    return _dev[(W, H)]


def stats_of(ctx, S):
    return [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total) for s in (ctx.stats(k) for k in range(S))]


def layered(ctx, W, H, S, F, prm, nl=L):
    fr = dev_frames(W, H)
    outs = ctx.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2][:nl], [(n, h, lay[:nl]) for n, h, lay in fr[1:1 + F]], S, prm)
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs]


def single(ctx, W, H, S, F, prm, k):
    """bcd_hip_denoise_temporal on layer k alone"""
    fr = dev_frames(W, H)
    out = ctx.denoise_temporal(fr[0][2][k][0], fr[0][0], fr[0][1], fr[0][2][k][1], [(lay[k][0], n, h, lay[k][1]) for n, h, lay in fr[1:1 + F]], S, prm)
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("W,H,S,F,m,r", tl.CONFIGS)
def test_whole_call_against_the_reference_of_every_layer(hipctx, W, H, S, F, m, r):
    outs = layered(hipctx, W, H, S, F, params(m, r))
    stats = stats_of(hipctx, S)
    redo = [[hipctx.layer_spectral_inverses(s, k) for k in range(L)] for s in range(S)]
    assert [sum(x) for x in redo] == [hipctx.stats(s).spectral_inverses for s in range(S)], redo
    errs = []
    for k in range(L):
        want, wstats = tl.reference(W, H, S, F, m, r, k)
        assert stats == wstats, (k, stats, wstats)
        errs.append(rel_linf(outs[k], want))
    print("temporal-layers %dx%d S=%d F=%d m=%g: %s, against float64 per layer %s" % (W, H, S, F, m, stats, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("W,H,S,F,m,r", [(64, 44, 2, 2, 1.0, 1), (72, 48, 1, 1, 0.0, 0), (72, 48, 2, 2, 0.0, 0)])
def test_every_layer_is_the_single_layer_call_on_that_layer(hipctx, W, H, S, F, m, r):
    prm = params(m, r)
    outs = layered(hipctx, W, H, S, F, prm)
    stats = stats_of(hipctx, S)
    for k in range(L):
        want = single(hipctx, W, H, S, F, prm, k)
        assert stats_of(hipctx, S) == stats, k
        e = rel_linf(outs[k], want)
        print("temporal-layers %dx%d S=%d F=%d m=%g layer %d against bcd_hip_denoise_temporal %.2e" % (W, H, S, F, m, k, e))
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("S", [1, 2])
def test_no_neighbour_is_the_layered_call_and_one_layer_is_the_temporal_call(hipctx, S):
    W, H = tl.SIZES[0]
    prm = params(1.0, 1)
    fr = dev_frames(W, H)
    got = layered(hipctx, W, H, S, 0, prm)
    stats = stats_of(hipctx, S)
    want = hipctx.denoise_layers(fr[0][0], fr[0][1], fr[0][2], S, prm)
    hipctx.synchronize()
    assert stats_of(hipctx, S) == stats
    for k in range(L):
        assert rel_linf(got[k], want[k].cpu().numpy()) <= TOL, k
    (one,) = layered(hipctx, W, H, S, 2, prm, nl=1)
    stats = stats_of(hipctx, S)
    assert hipctx.layer_spectral_inverses(0, 0) == hipctx.stats(0).spectral_inverses
    want = single(hipctx, W, H, S, 2, prm, 0)
    assert stats_of(hipctx, S) == stats and rel_linf(one, want) <= TOL


@pytest.mark.parametrize("S,F", [(1, 1), (2, 2)])
def test_host_entry_point_returns_the_device_call_s_layers(hipctx, S, F):
    W, H = tl.SIZES[0]
    prm = params(1.0, 1)
    want = layered(hipctx, W, H, S, F, prm)
    wstats = stats_of(hipctx, S)
    fr = tl.frames_of(W, H)
    got = hipctx.denoise_temporal_layers_host(fr[0][0], fr[0][1], fr[0][2], fr[1:1 + F], S, prm)
    assert stats_of(hipctx, S) == wstats
    for k in range(L):
        assert rel_linf(got[k], want[k]) <= TOL, k
    plain = hipctx.denoise_temporal_layers_host(fr[0][0], fr[0][1], fr[0][2], [], S, prm)       # no neighbour: bcd_hip_denoise_layers_host
    d = dev_frames(W, H)
    ref = hipctx.denoise_layers(d[0][0], d[0][1], d[0][2], S, prm)
    hipctx.synchronize()
    for k in range(L):
        assert rel_linf(plain[k], ref[k].cpu().numpy()) <= TOL, k


def test_plain_calls_after_the_layered_call_equal_a_fresh_context_s():
    import bcd_amd.hip as bh
    (W, H), (W2, H2) = tl.SIZES
    prm = params(1.0, 1)
    out = {}
    for which in ("after", "fresh"):
        ctx = bh.Context(0)
        try:
            if which == "after":
                layered(ctx, W2, H2, 2, 1, prm)
                layered(ctx, W, H, 2, 2, prm)
            fr = dev_frames(W, H)
            a = single(ctx, W, H, 2, 2, prm, 1)
            sa = stats_of(ctx, 2)
            b = [o.cpu().numpy() for o in ctx.denoise_layers(fr[0][0], fr[0][1], fr[0][2], 2, prm)]
            ctx.synchronize()
            out[which] = (a, sa, b, stats_of(ctx, 2))
        finally:
            ctx.close()
    assert out["after"][1] == out["fresh"][1] and out["after"][3] == out["fresh"][3]
    assert rel_linf(out["after"][0], out["fresh"][0]) <= TOL
    for k in range(L):
        assert rel_linf(out["after"][2][k], out["fresh"][2][k]) <= TOL, k


def test_stage_timers_and_geometry_of_the_temporal_calls(hipctx):
    """bcd_hip_denoise_temporal and bcd_hip_denoise_temporal_layers (two layers) at 64x44, two scales, one neighbour, m = 1: with profiling on, the four stage
    timers of every scale are finite and not negative and the total is at least each part; width, height and cu_share are the level's; with profiling off the
    timers are zero.  No timer is compared with a number of milliseconds."""
    W, H, S, F = 64, 44, 2, 1
    prm = params(1.0, 1)
    timers = ("ms_similarity", "ms_active", "ms_bayes", "ms_total")
    calls = (("temporal", lambda: single(hipctx, W, H, S, F, prm, 0)), ("temporal-layers", lambda: layered(hipctx, W, H, S, F, prm, nl=2)))

    def geometry(name):
        for s in range(S):
            st = hipctx.stats(s)
            assert (st.width, st.height, st.cu_share) == (W >> s, H >> s, 100), (name, s, st.width, st.height, st.cu_share)

    hipctx.set_profiling(True)
    try:
        for name, call in calls:
            call()
            geometry(name)
            for s in range(S):
                st = hipctx.stats(s)
                ms = [float(getattr(st, t)) for t in timers]
                print("%s %dx%d scale %d: %s" % (name, W, H, s, " ".join("%s=%.4f" % (t, v) for t, v in zip(timers, ms))))
                assert all(np.isfinite(v) and v >= 0 for v in ms), (name, s, ms)
                assert all(ms[3] >= v for v in ms[:3]), (name, s, ms)
    finally:
        hipctx.set_profiling(False)
    for name, call in calls:
        call()
        geometry(name)
        for s in range(S):
            st = hipctx.stats(s)
            assert all(getattr(st, t) == 0 for t in timers), (name, s)


def test_refusals_of_the_frame_call_then_a_successful_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    W, H = tl.SIZES[0]
    fr = dev_frames(W, H)
    ns, hist, lay = fr[0]
    nb = [fr[1]]
    prm = params(1.0, 1)
    outs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(L)]

    def refused(call, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert code is None or ("rc=%d" % code) in str(e.value) or "support" in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                 # with neighbours, any other geometry: BCD_HIP_EUNSUPPORTED
        p = bh.default_params(m=1.0, random_order=1, w=w, b=b)
        refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb, 1, p, outs=outs), -4)
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb * 5, 1, prm, outs=outs))                      # five neighbours
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay * 6, [(fr[1][0], fr[1][1], fr[1][2] * 6)], 1, prm))  # eighteen layers
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb, 9, prm, outs=outs))                          # too many scales for the image
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb, 1, prm, outs=[outs[0], outs[1], lay[1][0]]))   # an output that is an input
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb, 1, prm, outs=[outs[0], outs[1], nb[0][2][2][0]]))  # ... of a neighbour's layer
    refused(lambda: hipctx.denoise_temporal_layers(ns, hist, lay, nb, 1, prm, outs=[outs[0], outs[1], outs[0]]))     # two layers share an output
    with pytest.raises(ValueError):                                  # a neighbour with a missing layer never reaches the library
        hipctx.denoise_temporal_layers(ns, hist, lay, [(fr[1][0], fr[1][1], fr[1][2][:2])], 1, prm, outs=outs)
    lib = bh.lib()
    la = (bh.Layer * L)()
    for k in range(L):
        la[k].d_colors, la[k].d_covariances, la[k].d_out = lay[k][0].data_ptr(), lay[k][1].data_ptr(), outs[k].data_ptr()
    fl = (bh.FrameLayer * L)()
    for k in range(L):
        fl[k].d_colors, fl[k].d_covariances = nb[0][2][k][0].data_ptr(), nb[0][2][k][1].data_ptr()
    one = (bh.FrameLayers * 1)()
    one[0].d_nsamples, one[0].d_histograms, one[0].layers = nb[0][0].data_ptr(), nb[0][1].data_ptr(), fl
    call = lambda frames, n, nsp=ns.data_ptr(), layers=la, nl=L: lib.bcd_hip_denoise_temporal_layers(hipctx.h, nsp, hist.data_ptr(), frames, n, W, H, hist.shape[2], 1,
                                                                                                      C.byref(prm), layers, nl)
    one[0].reserved = 1
    assert call(one, 1) == -1                                        # a non-NULL reserved pointer
    one[0].reserved = None
    assert call(one, -1) == -1 and call(one, 5) == -1                # nb_neighbours outside 0 .. 4
    assert call(None, 1) == -1                                       # no neighbour list
    assert call(one, 1, None) == -1                                  # a null image
    assert call(one, 1, layers=None) == -1 and call(one, 1, nl=0) == -1 and call(one, 1, nl=17) == -1   # no layer list, no layer, too many
    fl[1].d_covariances = None
    assert call(one, 1) == -1                                        # a null image in a layer of a neighbour
    fl[1].d_covariances = nb[0][2][1][1].data_ptr()
    one[0].layers = None
    assert call(one, 1) == -1                                        # a null layer list in a neighbour
    one[0].layers = fl
    one[0].d_histograms = None
    assert call(one, 1) == -1                                        # a null image in a neighbour
    assert all(float(o.abs().sum()) == 0.0 for o in outs)            # nothing ran
    got = hipctx.denoise_temporal_layers(ns, hist, lay, nb, 1, prm, outs=outs)
    hipctx.synchronize()
    stats = stats_of(hipctx, 1)
    for k in range(L):
        want, wstats = tl.reference(W, H, 1, 1, 1.0, 1, k)
        assert stats == wstats and rel_linf(got[k].cpu().numpy(), want) <= TOL, k


@pytest.mark.parametrize("S,F", [(1, 1), (2, 2)])
def test_cpp_class_returns_the_device_call_s_layers(hipctx, S, F):
    """addLayer beside addNeighbourFrame / addNeighbourFrameLayer: the device call's layers; clearNeighbourFrames() clears the neighbours' layers too and
    gives the plain layered denoise() again; a neighbour with a missing layer is refused"""
    import bcd_amd.core as core
    W, H = tl.SIZES[0]
    fr = tl.frames_of(W, H)
    d = dev_frames(W, H)
    prm = params(1.0, 1)
    want = layered(hipctx, W, H, S, F, prm)
    plain = [o.cpu().numpy() for o in hipctx.denoise_layers(d[0][0], d[0][1], d[0][2], S, prm)]
    ok, got = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2], fr[1:1 + F], S, seed=prm.order_seed)
    assert ok
    for k in range(L):
        assert rel_linf(got[k], want[k]) <= TOL, k
        assert rel_linf(got[k], plain[k]) > 10 * TOL, k                  # (the neighbours did something, in every layer)
    ok, got = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2], fr[1:1 + F], S, seed=prm.order_seed, after_clear=True)
    assert ok
    for k in range(L):
        assert rel_linf(got[k], plain[k]) <= TOL, k
    ok, _ = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2], fr[1:1 + F], S, seed=prm.order_seed, drop_layers=1)   # a neighbour with a missing layer
    assert not ok
    ok, _ = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2], fr[1:2], S, b=12, seed=prm.order_seed)               # another geometry
    assert not ok


def test_bcd_cli_neighbour_layer_end_to_end(hipctx, tmp_path):
    """bcd_cli --layer twice, --neighbour twice, each with two --neighbour-layer: the outputs are the device call's layers after the half-float EXR round
    trip; one --neighbour-layer too few is an argument error"""
    import os
    import subprocess
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 72, 56
    on_disk, nb_args = [], []
    for f, seed in enumerate((21, 22, 23)):
        col, ns, hist, cov = core.synthetic_scene(W, H, 16, seed, 0.15, 0.02)
        stem = str(tmp_path / ("frame%d" % f))
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        lay = []
        for k, (c, v) in enumerate(tl.share_layers(col, cov)):
            cpath = stem + (".exr" if k == 0 else "_l%d.exr" % k)
            vpath = stem + ("_cov.exr" if k == 0 else "_l%d_cov.exr" % k)
            core.write_exr(cpath, c, False)
            core.write_exr(vpath, v, True)
            lay.append((core.read_exr(cpath, False), v))                 # (colours go through half precision on disk)
        on_disk.append((ns, hist, lay))
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    p = lambda name: str(tmp_path / name)
    base = [exe, "-i", p("frame1.exr"), "-o", p("out.exr"), "-p", "0", "-s", "2", "-m", "1", "--seed", "5",
            "--layer", p("frame1_l1.exr"), p("frame1_l1_cov.exr"), p("out_l1.exr"), "--layer", p("frame1_l2.exr"), p("frame1_l2_cov.exr"), p("out_l2.exr")]
    nb = lambda f, n=2: ["--neighbour", p("frame%d.exr" % f)] + sum((["--neighbour-layer", p("frame%d_l%d.exr" % (f, k)), p("frame%d_l%d_cov.exr" % (f, k))] for k in range(1, 1 + n)), [])
    r = subprocess.run(base + nb(0) + nb(2), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    t3 = lambda fr: (_t(fr[0]), _t(fr[1]), [(_t(c), _t(v)) for c, v in fr[2]])
    mid, a, b = t3(on_disk[1]), t3(on_disk[0]), t3(on_disk[2])
    want = hipctx.denoise_temporal_layers(mid[0], mid[1], mid[2], [a, b], 2, bh.default_params(m=1.0, seed=5))
    for k, name in enumerate(("out.exr", "out_l1.exr", "out_l2.exr")):
        w = hipctx.zero_bad_values(want[k]).cpu().numpy()
        got = core.read_exr(p(name), False)
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), name
    r = subprocess.run(base + nb(0) + nb(2, 1), capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR in program arguments" in r.stdout and "--neighbour-layer" in r.stdout, r.stdout + r.stderr
