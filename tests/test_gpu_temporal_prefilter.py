"""GPU tests of the spike prefilter in the host frame calls (bcd_hip_denoise_temporal_host_ex; DESIGN 16, "Prefilter") against the composition that defines
it: every frame -- the frame and each neighbour -- through bcd_hip_spike_filter_layers on its own (sample counts, histograms unless in moment selection,
all layers, the decision from its own layer-0 colours; features and motion fields as they are), then the existing host call on the filtered frames.

  mode          layers  selection   gate                     motion   the existing host call
  hist_L1       1       histograms  none                     no       bcd_hip_denoise_temporal_layers_host (-> bcd_hip_denoise_temporal_host)
  hist_L3       3       histograms  none                     no       bcd_hip_denoise_temporal_layers_host
  hist_motion   2       histograms  none                     yes      bcd_hip_denoise_temporal_layers_motion_host
  hist_gate     1       histograms  F = 3 with variances     no       bcd_hip_denoise_temporal_guided_host
  mom_L1        1       moments     none                     no       bcd_hip_denoise_temporal_moments_host
  mom_L2_gate   2       moments     F = 2 without variances  yes      bcd_hip_denoise_temporal_moments_host with the guide

  * the frames of tests/test_gpu_sequence_modes.py at 40x28 (32 spp, spike probability 0.01), 1 and 2 scales, N = 1 and 2 neighbours: the stats of every scale
    and the spectral counters of every layer equal the composition's, every layer is within TOL = 1e-4 relative L-inf of it (results that differ by the order
    of the float atomics; the measured values are printed: docs/EXPERIMENTS.md);
  * asserted of the inputs: every frame of every case has moved pixels, and the prefiltered result differs from the unfiltered call's by more than 10 TOL;
  * opt = NULL and factor 0 are the delegated call; N = 0 with a factor is the single-frame host call with that factor over every layer;
  * the refusals of the call; bcd::Denoiser / MultiscaleDenoiser with setSpikePrefilterFrames and bcd_cli --neighbour ... --prefilter-frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guide_cross_cases as gc
import moments_cross_cases as xc
import test_gpu_sequence_modes as tm

pytestmark = pytest.mark.gpu

TOL = 1e-4
FACTOR = 2.0
W, H = 40, 28
CFG = {
    "hist_L1": dict(L=1, moments=False, F=0, var=False, motion=False),
    "hist_L3": dict(L=3, moments=False, F=0, var=False, motion=False),
    "hist_motion": dict(L=2, moments=False, F=0, var=False, motion=True),
    "hist_gate": dict(L=1, moments=False, F=3, var=True, motion=False),
    "mom_L1": dict(L=1, moments=True, F=0, var=False, motion=False),
    "mom_L2_gate": dict(L=2, moments=True, F=2, var=False, motion=True),
}
rel_linf = tm.rel_linf


def params(cfg, seed=1234):
    import bcd_amd.hip as bh
    return bh.default_params(m=1.0, random_order=1, seed=seed, tau=xc.TAU if cfg["moments"] else 1.0)


def frame_of(fr, cfg):
    """(ns, hist or None, layers, features or None, variances or None) of a frame of tm.frames_of, NumPy arrays"""
    F = cfg["F"]
    return (fr["ns"], None if cfg["moments"] else fr["hist"], [(c, v) for c, v in fr["layers"][:cfg["L"]]],
            np.ascontiguousarray(fr["feat"][..., :F]) if F else None, np.ascontiguousarray(fr["var"][..., :F]) if F and cfg["var"] else None)


def frames_for(cfg, N):
    """the frame (the middle one of the five) and its N neighbours"""
    fr = tm.frames_of(W, H)
    return [frame_of(fr[k], cfg) for k in ((2, 1, 3)[:N + 1])]


def fields_for(cfg, N):
    """None, or per neighbour a motion field or None: the first neighbour one pixel to the right with a disoccluded block, the second without a field"""
    if not cfg["motion"]:
        return None
    f = np.zeros((H, W, 2), np.float32)
    f[..., 0] = 1.0
    f[5:9, 10:14] = np.nan
    return [f, None][:N]


def filtered(ctx, frame):
    """one frame through bcd_hip_spike_filter_layers (out of place, on the device) -> (the frame with NumPy arrays again, moved pixels)"""
    ns, hist, layers, feat, var = frame
    f_ns, f_hist, f_layers, _, moved = ctx.spike_filter_layers(tm.t(ns), tm.t(hist), [(tm.t(c), tm.t(v)) for c, v in layers], FACTOR, count=True)
    n = lambda a: None if a is None else a.cpu().numpy()
    return (n(f_ns), n(f_hist), [(n(c), n(v)) for c, v in f_layers], feat, var), moved


def guide_kw(cfg, frames):
    if not cfg["F"]:
        return {}
    return dict(features=frames[0][3], neighbour_features=[f[3] for f in frames[1:]], variances=frames[0][4],
                neighbour_variances=[f[4] for f in frames[1:]] if cfg["var"] else None, floors=gc.FLOORS[:cfg["F"]], threshold=gc.TAU_G)


def host_ex(ctx, cfg, frames, S, prm, fields, factor):
    ns, hist, layers = frames[0][:3]
    nbs = [(f[0], f[2]) if cfg["moments"] else (f[0], f[1], f[2]) for f in frames[1:]]
    return ctx.denoise_temporal_host_ex(ns, hist, layers, nbs, S, prm, spike_factor=factor, var_floor=xc.VAR_FLOOR, motions=fields, **guide_kw(cfg, frames))


def existing_host_call(ctx, cfg, frames, S, prm, fields):
    """the host call that exists without the prefilter for these arguments"""
    ns, hist, layers = frames[0][:3]
    if cfg["moments"]:
        return ctx.denoise_temporal_moments_host(ns, layers, [(f[0], f[2]) for f in frames[1:]], S, prm, var_floor=xc.VAR_FLOOR, motions=fields, **guide_kw(cfg, frames))
    nbs = [(f[0], f[1], f[2]) for f in frames[1:]]
    if cfg["F"]:
        return ctx.denoise_temporal_guided_host(ns, hist, layers, nbs, S, prm, motions=fields, **guide_kw(cfg, frames))
    if fields is not None:
        return ctx.denoise_temporal_layers_motion_host(ns, hist, layers, nbs, fields, S, prm)
    return ctx.denoise_temporal_layers_host(ns, hist, layers, nbs, S, prm)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode", sorted(CFG))
def test_host_ex_is_the_filter_per_frame_and_the_existing_host_call(hipctx, mode, S, N):
    cfg = CFG[mode]
    L = cfg["L"]
    prm = params(cfg)
    frames, fields = frames_for(cfg, N), fields_for(cfg, N)
    both = [filtered(hipctx, f) for f in frames]
    assert all(m > 0 for _, m in both), [m for _, m in both]                     # every frame of the case has moved pixels
    want = existing_host_call(hipctx, cfg, [f for f, _ in both], S, prm, fields)
    wstats = tm.stats_of(hipctx, S, L)
    kept = [np.array(a) for a in (frames[0][0], frames[1][2][0][0])]
    got = host_ex(hipctx, cfg, frames, S, prm, fields, FACTOR)
    stats = tm.stats_of(hipctx, S, L)
    assert stats == wstats, (stats, wstats)
    assert np.array_equal(kept[0], frames[0][0]) and np.array_equal(kept[1], frames[1][2][0][0])      # the caller's images are read only
    errs = [rel_linf(g, w) for g, w in zip(got, want)]
    print("%s S=%d N=%d: moved %s; layers vs the composition %s" % (mode, S, N, [m for _, m in both], " ".join("%.2e" % e for e in errs)))
    assert len(got) == L and max(errs) <= TOL
    # the unfiltered call: the prefilter changed the result ...
    plain = existing_host_call(hipctx, cfg, frames, S, prm, fields)
    pstats = tm.stats_of(hipctx, S, L)
    assert max(rel_linf(g, p) for g, p in zip(got, plain)) > 10 * TOL
    # ... and opt = NULL and factor 0 are that call
    for factor in (None, 0.0, -1.0):
        same = host_ex(hipctx, cfg, frames, S, prm, fields, factor)
        assert tm.stats_of(hipctx, S, L) == pstats
        assert max(rel_linf(g, p) for g, p in zip(same, plain)) <= TOL, factor


@pytest.mark.parametrize("mode", ["hist_L1", "hist_L3", "hist_gate", "mom_L1", "mom_L2_gate"])
def test_no_neighbour_with_a_factor_is_the_single_frame_host_call(hipctx, mode):
    cfg = CFG[mode]
    S, prm = 2, params(cfg)
    frame = frames_for(cfg, 0)
    ns, hist, layers, feat, var = frame[0]
    # (the per-scale figures of bcd_hip_get_stats: not every single-frame host call leaves per-layer spectral counters)
    stats_of = lambda: [(s.processed, s.fallback, s.similar_total, s.spectral_inverses) for s in (hipctx.stats(k) for k in range(S))]
    got = host_ex(hipctx, cfg, frame, S, prm, None, FACTOR)
    stats = stats_of()
    if cfg["F"]:
        want = hipctx.denoise_guided_host(ns, hist, layers, S, prm, feat, variances=var, floors=gc.FLOORS[:cfg["F"]], threshold=gc.TAU_G, var_floor=xc.VAR_FLOOR,
                                          spike_factor=FACTOR, filter_layers=True)
    elif cfg["moments"]:
        want = hipctx.denoise_moments_host(ns, layers, S, prm, var_floor=xc.VAR_FLOOR, spike_factor=FACTOR, filter_layers=True)
    else:
        want = hipctx.denoise_layers_host(ns, hist, layers, S, prm, spike_factor=FACTOR, filter_layers=True)
    assert stats == stats_of() and all(st[0] > 0 for st in stats)
    for g, w in zip(got, want):
        assert rel_linf(g, w) <= TOL
    none = host_ex(hipctx, cfg, frame, S, prm, None, None)                       # no factor: the unfiltered single-frame call
    assert max(rel_linf(g, n) for g, n in zip(got, none)) > 10 * TOL


def test_refusals_then_a_good_call(hipctx):
    import bcd_amd.hip as bh
    cfg = CFG["hist_L3"]
    prm = params(cfg)
    frames = frames_for(cfg, 1)

    def refused(**kw):
        args = dict(factor=FACTOR)
        args.update(kw)
        with pytest.raises(bh.BcdHipError) as e:
            ns, hist, layers = frames[0][:3]
            hipctx.denoise_temporal_host_ex(ns, hist, layers, [(f[0], f[1], f[2]) for f in frames[1:]], args.get("S", 1), args.get("prm", prm),
                                            spike_factor=args["factor"], reserved=args.get("reserved"))
        return str(e.value)

    assert "reserved" in refused(reserved=C.addressof(C.c_int(1)))
    assert "reserved" in refused(reserved=C.addressof(C.c_int(1)), factor=0.0)
    assert "finite" in refused(factor=float("nan")) and "finite" in refused(factor=float("inf"))
    assert refused(S=0) and refused(S=9)                                         # what the delegated call refuses
    wide = bh.default_params(m=1.0, seed=1234, b=12)
    assert "rc=-4" in refused(prm=wide)                                          # BCD_HIP_EUNSUPPORTED: neighbour frames at search radius 6 only
    tiny = (np.ones((2, 5), np.float32), np.zeros((2, 5, 60), np.float32), [(np.zeros((2, 5, 3), np.float32), np.zeros((2, 5, 6), np.float32))])
    with pytest.raises(bh.BcdHipError) as e:
        hipctx.denoise_temporal_host_ex(tiny[0], tiny[1], tiny[2], [tiny], 1, prm, spike_factor=FACTOR)
    assert "smaller than 3x3" in str(e.value)
    got = host_ex(hipctx, cfg, frames, 1, prm, None, FACTOR)                     # the context is as good as before
    want = existing_host_call(hipctx, cfg, [filtered(hipctx, f)[0] for f in frames], 1, prm, None)
    assert max(rel_linf(g, w) for g, w in zip(got, want)) <= TOL


# ---- the C++ classes and the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,S,N", [("hist_L1", 2, 2), ("hist_motion", 1, 1), ("hist_gate", 1, 2), ("mom_L2_gate", 2, 1)])
def test_cpp_classes_with_the_switch(hipctx, mode, S, N):
    """bcd::Denoiser (one scale) / bcd::MultiscaleDenoiser with setSpikePrefilter and setSpikePrefilterFrames beside neighbour frames"""
    import bcd_amd.core as core
    cfg = CFG[mode]
    prm = params(cfg)
    frames, fields = frames_for(cfg, N), fields_for(cfg, N)
    want = existing_host_call(hipctx, cfg, [filtered(hipctx, f)[0] for f in frames], S, prm, fields)
    ns, hist, layers = frames[0][:3]
    kw = dict(nscales=S, seed=prm.order_seed, tau=prm.hist_dist_threshold, motions=fields, **guide_kw(cfg, frames))
    if cfg["moments"]:
        call = lambda **more: core.denoise_temporal_moments(ns, layers, [(f[0], f[2]) for f in frames[1:]], var_floor=xc.VAR_FLOOR, **kw, **more)
    elif cfg["L"] == 1 and not cfg["F"]:
        col, cov = layers[0]
        one = lambda **more: core.denoise_temporal(col, ns, hist, cov, [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in frames[1:]], **kw, **more)
        call = lambda **more: (lambda r: (r[0], [r[1]]))(one(**more))
    else:
        call = lambda **more: core.denoise_temporal_layers(ns, hist, layers, [(f[0], f[1], f[2]) for f in frames[1:]], **kw, **more)
    ok, got = call(prefilter_frames=FACTOR)
    assert ok and len(got) == cfg["L"]
    for g, w in zip(got, want):
        assert rel_linf(g, w) <= TOL
    assert not call(prefilter_without_switch=FACTOR)[0]                                 # the factor without the switch: refused as before
    ok, plain = call()
    assert ok and max(rel_linf(g, p) for g, p in zip(got, plain)) > 10 * TOL


def test_bcd_cli_neighbours_with_prefilter_frames_end_to_end(hipctx, tmp_path):
    """bcd_cli -i with two --neighbour, one --layer each and the default -p 1: with --prefilter-frames every output is the composition's layer after the
    half-float EXR round trip; without the flag the call is refused"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    import temporal_layers_cases as tl
    w, h = 72, 56
    on_disk = []
    for f, seed in enumerate((21, 22, 23)):
        col, ns, hist, cov = core.synthetic_scene(w, h, 16, seed, 0.15, 0.02)
        stem = str(tmp_path / ("frame%d" % f))
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        lay = []
        for k, (c, v) in enumerate(tl.share_layers(col, cov)[:2]):
            cpath = stem + (".exr" if k == 0 else "_l%d.exr" % k)
            vpath = stem + ("_cov.exr" if k == 0 else "_l%d_cov.exr" % k)
            core.write_exr(cpath, c, False)
            core.write_exr(vpath, v, True)
            lay.append((core.read_exr(cpath, False), v))                         # (colours go through half precision on disk)
        on_disk.append((ns, hist, lay))
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    p = lambda name: str(tmp_path / name)
    base = [exe, "-i", p("frame1.exr"), "-o", p("out.exr"), "-s", "2", "-m", "1", "--seed", "5", "--layer", p("frame1_l1.exr"), p("frame1_l1_cov.exr"), p("out_l1.exr")]
    nb = lambda f: ["--neighbour", p("frame%d.exr" % f), "--neighbour-layer", p("frame%d_l1.exr" % f), p("frame%d_l1_cov.exr" % f)]
    r = subprocess.run(base + nb(0) + nb(2) + ["--prefilter-frames"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    dev_frames = []
    for ns, hist, lay in on_disk:
        f_ns, f_hist, f_layers, _, moved = hipctx.spike_filter_layers(tm.t(ns), tm.t(hist), [(tm.t(c), tm.t(v)) for c, v in lay], FACTOR, count=True)
        assert moved > 0
        dev_frames.append((f_ns, f_hist, f_layers))
    mid, a, b = dev_frames[1], dev_frames[0], dev_frames[2]
    want = hipctx.denoise_temporal_layers(mid[0], mid[1], mid[2], [a, b], 2, bh.default_params(m=1.0, seed=5))
    for k, name in enumerate(("out.exr", "out_l1.exr")):
        x = hipctx.zero_bad_values(want[k]).cpu().numpy()
        got = core.read_exr(p(name), False)
        assert np.max(np.abs(got - x.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(x), name
    r = subprocess.run(base[:11] + nb(0)[:2] + nb(2)[:2], capture_output=True, text=True, timeout=120)      # no layers, no flag: the library's refusal
    assert r.returncode != 0 and "do not combine with the spike prefilter" in r.stdout + r.stderr
