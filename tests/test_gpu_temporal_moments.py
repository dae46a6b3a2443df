"""GPU tests of the temporal frame call of the moment selection (bcd_hip_denoise_temporal_moments[_host]; DESIGN 16, "Moments") against the NumPy composition of
tests/moments_cross_cases.py (reference: the float64 estimate on the float32 selection of tests/moments_ref.py and tests/moments_cross_ref.py).

  * 40x28, 52x36 and 64x44, 1 and 2 scales, N = 1 and 2, L = 1 and 3, with and without a guide: processed / fallback / similar_total of every scale equal the
    reference's, every output is within TOL = 1e-4 of it relative to its maximum (the project's frame bar); the same with motion fields that contain invalid
    pixels.  Measured on the MI355X: at most 4.4e-7 on the frame and the smooth share, 4.4e-6 on the textured share (layer 2);
  * nb_neighbours == 0 equals bcd_hip_denoise_moments (with a guide: bcd_hip_denoise_guided without histograms) within TOL_SAME = 1e-5 with equal stats;
  * a guide that can gate nothing equals the unguided call the same way; zero motion fields equal no fields; the host call equals the resident call;
  * Denoiser::addNeighbourFrameMoments (through libbcdcore.so) and bcd_cli --neighbour-nsamples equal the resident call;
  * bcd_hip_denoise, bcd_hip_denoise_moments and bcd_hip_denoise_temporal after such calls on the same context equal a fresh context's;
  * refusals, then a good call;
  * benefit: the static two-region scene of moments_cases.noisy at 8 spp with two neighbours of independent noise: the RMSE against the noise-free signal of
    the temporal call over that of bcd_hip_denoise_moments is below 1 and within 0.02 of the NumPy composition's ratio.  NumPy composition: 0.00949 over
    0.01852, ratio 0.513; MI355X: 0.513."""
import numpy as np
import pytest

import guide_cross_cases as gc
import moments_cross_cases as xc
from test_gpu_temporal import TOL, rel_linf, stats_of

pytestmark = pytest.mark.gpu

TOL_SAME = 1e-5
F32 = np.float32


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def params(m=gc.M, r=gc.R, tau=xc.TAU):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=gc.SEED, tau=tau)


def dev_frames(fr, L):
    return [(t(ns), [(t(c), t(v)) for c, v in lay[:L]]) for ns, lay in fr]


def moments_call(ctx, fr, L, S, fields=None, ft=None, floors=gc.FLOORS, tau_g=gc.TAU_G, prm=None, eps=xc.VAR_FLOOR):
    d = dev_frames(fr, L)
    kw = {}
    if ft is not None:
        var = ft[0][1] is not None
        kw = dict(features=t(ft[0][0]), neighbour_features=[t(f) for f, _ in ft[1:]], variances=t(ft[0][1]),
                  neighbour_variances=[t(v) for _, v in ft[1:]] if var else None, floors=floors, threshold=tau_g)
    outs = ctx.denoise_temporal_moments(d[0][0], d[0][1], d[1:], S, prm or params(), var_floor=eps, motions=None if fields is None else [t(f) for f in fields], **kw)
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs], stats_of(ctx, S)


def check_against_reference(ctx, cfg, motion):
    W, H, S, N, L, guide = cfg
    fr = xc.frames_of(W, H)[:1 + N]
    ft = gc.features_of(W, H, True)[:1 + N] if guide else None
    outs, stats = moments_call(ctx, fr, L, S, gc.fields_of(W, H, N) if motion else None, ft)
    want, wstats = xc.reference(W, H, S, N, L, guide, motion)
    assert stats == wstats, (stats, wstats)
    assert all(s["processed"] > 0 and s["similar_total"] > 0 for s in stats)
    for s in range(S):
        assert ctx.stats(s).similarity_path == 3
    for k in range(L):
        e = rel_linf(outs[k], want[k])
        print("temporal moments %s%s layer %d: %s, against float64 %.2e" % (cfg, " motion" if motion else "", k, stats, e))
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("cfg", xc.CONFIGS)
def test_whole_call_against_the_reference_composition(hipctx, cfg):
    check_against_reference(hipctx, cfg, False)


@pytest.mark.parametrize("cfg", xc.MOTION_CONFIGS)
def test_whole_call_with_motion_fields_against_the_reference_composition(hipctx, cfg):
    check_against_reference(hipctx, cfg, True)


@pytest.mark.parametrize("S,L,guide", [(1, 1, False), (2, 3, False), (2, 2, True)])
def test_no_neighbours_is_the_single_frame_call(hipctx, S, L, guide):
    W, H = 52, 36
    fr = xc.frames_of(W, H)[:1]
    ft = gc.features_of(W, H, True)[:1] if guide else None
    outs, stats = moments_call(hipctx, fr, L, S, None, ft)
    d = dev_frames(fr, L)
    if guide:
        want = hipctx.denoise_guided(d[0][0], None, d[0][1], S, params(), t(ft[0][0]), variances=t(ft[0][1]), floors=gc.FLOORS, threshold=gc.TAU_G, var_floor=xc.VAR_FLOOR)
    else:
        want = hipctx.denoise_moments(d[0][0], d[0][1], S, params(), xc.VAR_FLOOR)
    hipctx.synchronize()
    assert stats == stats_of(hipctx, S)
    for k in range(L):
        assert rel_linf(outs[k], want[k].cpu().numpy()) <= TOL_SAME, k


@pytest.mark.parametrize("W,H,S,N,L,motion", [(52, 36, 2, 2, 3, False), (64, 44, 2, 1, 1, True), (40, 28, 1, 2, 3, True)])
def test_a_guide_that_gates_nothing_is_the_unguided_call(hipctx, W, H, S, N, L, motion):
    fr, ft = xc.frames_of(W, H)[:1 + N], gc.neutral_features(W, H)[:1 + N]
    fields = gc.fields_of(W, H, N) if motion else None
    outs, stats = moments_call(hipctx, fr, L, S, fields, ft, floors=(1.0, 1.0))
    plain, pstats = moments_call(hipctx, fr, L, S, fields)
    assert stats == pstats
    for k in range(L):
        e = rel_linf(outs[k], plain[k])
        print("neutral guide %dx%d S=%d N=%d L=%d%s layer %d: against the unguided call %.2e" % (W, H, S, N, L, " motion" if motion else "", k, e))
        assert e <= TOL_SAME, (k, e)


@pytest.mark.parametrize("W,H,S,N,L", [(52, 36, 2, 2, 3), (40, 28, 1, 1, 1)])
def test_zero_motion_fields_equal_no_fields(hipctx, W, H, S, N, L):
    fr = xc.frames_of(W, H)[:1 + N]
    zero = [np.zeros((H, W, 2), F32) for _ in range(N)]
    outs, stats = moments_call(hipctx, fr, L, S, zero)
    plain, pstats = moments_call(hipctx, fr, L, S, None)
    assert stats == pstats
    for k in range(L):
        assert rel_linf(outs[k], plain[k]) <= TOL_SAME, k


@pytest.mark.parametrize("cfg,motion", [((40, 28, 2, 2, 3, True), True), ((52, 36, 1, 1, 1, False), True), ((40, 28, 1, 2, 3, False), False)])
def test_host_call_equals_the_resident_call(hipctx, cfg, motion):
    W, H, S, N, L, guide = cfg
    fr = xc.frames_of(W, H)[:1 + N]
    ft = gc.features_of(W, H, True)[:1 + N] if guide else None
    fields = gc.fields_of(W, H, N) if motion else None
    if motion and N == 2:
        fields[1] = None
    want, wstats = moments_call(hipctx, fr, L, S, fields, ft)
    kw = {}
    if guide:
        kw = dict(features=ft[0][0], neighbour_features=[f for f, _ in ft[1:]], variances=ft[0][1], neighbour_variances=[v for _, v in ft[1:]], floors=gc.FLOORS,
                  threshold=gc.TAU_G)
    got = hipctx.denoise_temporal_moments_host(fr[0][0], fr[0][1][:L], [(ns, lay[:L]) for ns, lay in fr[1:]], S, params(), var_floor=xc.VAR_FLOOR, motions=fields, **kw)
    assert stats_of(hipctx, S) == wstats
    for k in range(L):
        assert rel_linf(got[k], want[k]) <= TOL_SAME, k
    none = hipctx.denoise_temporal_moments_host(fr[0][0], fr[0][1][:L], [], S, params(), var_floor=xc.VAR_FLOOR)
    nstats = stats_of(hipctx, S)
    d = dev_frames(fr[:1], L)
    want0 = hipctx.denoise_moments(d[0][0], d[0][1], S, params(), xc.VAR_FLOOR)
    hipctx.synchronize()
    assert nstats == stats_of(hipctx, S)
    for k in range(L):
        assert rel_linf(none[k], want0[k].cpu().numpy()) <= TOL_SAME, k


def test_other_calls_after_temporal_moment_calls_equal_a_fresh_context_s():
    import bcd_amd.hip as bh
    W, H = 40, 28
    prm = params()
    full = gc.frames_of(W, H)                                              # (with histograms, for the histogram calls)
    fr = xc.frames_of(W, H)
    frame = (full[0][2][0][0], full[0][0], full[0][1], full[0][2][0][1])
    nbs = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in full[1:]]
    out = {}
    for which in ("after", "fresh"):
        ctx = bh.Context(0)
        try:
            if which == "after":
                moments_call(ctx, xc.frames_of(64, 44), 3, 2, gc.fields_of(64, 44, 2), gc.features_of(64, 44, True), prm=prm)
                moments_call(ctx, fr[:2], 1, 1, prm=prm)
            a = ctx.denoise(*[t(x) for x in frame], 2, prm)
            ctx.synchronize()
            sa = stats_of(ctx, 2)
            d = dev_frames(fr[:1], 2)
            b = ctx.denoise_moments(d[0][0], d[0][1], 2, prm, xc.VAR_FLOOR)
            ctx.synchronize()
            sb = stats_of(ctx, 2)
            c = ctx.denoise_temporal(*[t(x) for x in frame], [tuple(t(x) for x in nb) for nb in nbs], 2, prm)
            ctx.synchronize()
            sc = stats_of(ctx, 2)
            out[which] = (a.cpu().numpy(), sa, [o.cpu().numpy() for o in b], sb, c.cpu().numpy(), sc)
        finally:
            ctx.close()
    x, y = out["after"], out["fresh"]
    assert x[1] == y[1] and x[3] == y[3] and x[5] == y[5]
    assert rel_linf(x[0], y[0]) <= TOL_SAME and rel_linf(x[4], y[4]) <= TOL_SAME
    for k in range(2):
        assert rel_linf(x[2][k], y[2][k]) <= TOL_SAME, k


@pytest.mark.parametrize("S,L,guide,motion", [(1, 1, False, False), (2, 2, True, True), (2, 3, False, True)])
def test_add_neighbour_frame_moments_is_the_resident_call(hipctx, S, L, guide, motion):
    import bcd_amd.core as core
    W, H, N = 52, 36, 2
    fr = xc.frames_of(W, H)[:1 + N]
    ft = gc.features_of(W, H, True)[:1 + N] if guide else None
    fields = gc.fields_of(W, H, N) if motion else None
    if motion:
        fields[1] = None
    kw = {}
    if guide:
        kw = dict(features=ft[0][0], variances=ft[0][1], neighbour_features=[f for f, _ in ft[1:]], neighbour_variances=[v for _, v in ft[1:]], floors=gc.FLOORS,
                  threshold=gc.TAU_G)
    ok, got = core.denoise_temporal_moments(fr[0][0], fr[0][1][:L], [(ns, lay[:L]) for ns, lay in fr[1:]], nscales=S, tau=xc.TAU, seed=gc.SEED, m=gc.M,
                                            var_floor=xc.VAR_FLOOR, motions=fields, **kw)
    assert ok
    want, _ = moments_call(hipctx, fr, L, S, fields, ft)
    for k in range(L):
        e = rel_linf(got[k], want[k])
        print("addNeighbourFrameMoments S=%d L=%d layer %d: against the resident call %.2e" % (S, L, k, e))
        assert e <= TOL_SAME, (k, e)


def test_cli_neighbour_nsamples_is_the_resident_call(hipctx, tmp_path):
    """the bound of tests/test_gpu_temporal_guided.py's CLI test: bcd_cli writes its colours in half precision, so TOL_SAME of the resident result's maximum plus
    the rounding to binary16 of a value that close (2^-11 relative in the normal range, 2^-25 absolute below)"""
    import os
    import subprocess
    import bcd_amd.core as core
    W, H, N = 52, 36, 1
    fr = xc.frames_of(W, H)[:1 + N]
    disk = []
    for i, (ns, lay) in enumerate(fr):
        stem = str(tmp_path / ("frame%d" % i))
        core.write_exr(stem + ".exr", lay[0][0], False)
        core.write_exr(stem + "_cov.exr", lay[0][1], True)
        core.write_exr(stem + "_ns.exr", np.asarray(ns, F32).reshape(H, W, 1), True)
        disk.append((ns, [(core.read_exr(stem + ".exr", False), lay[0][1])]))      # (colours go through half precision on disk; there is no _hist.exr)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    s0, s1 = str(tmp_path / "frame0"), str(tmp_path / "frame1")
    r = subprocess.run([exe, "-i", s0 + ".exr", "-o", out_path, "-p", "0", "-s", "2", "-m", "1", "-d", str(xc.TAU), "--seed", str(gc.SEED), "--moment-selection",
                        str(xc.VAR_FLOOR), "--nsamples", s0 + "_ns.exr", "--neighbour", s1 + ".exr", "--neighbour-nsamples", s1 + "_ns.exr"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    (want,), _ = moments_call(hipctx, disk, 1, 2)
    w = hipctx.zero_bad_values(t(want)).cpu().numpy()
    got = core.read_exr(out_path, False)
    same = TOL_SAME * np.max(np.abs(w))
    bound = same + np.maximum(2.0 ** -11 * (np.abs(w) + same), 2.0 ** -25)
    print("bcd_cli --neighbour-nsamples: worst deviation from the resident call %.3f of the bound (TOL_SAME + binary16 rounding)" % float(np.max(np.abs(got - w) / bound)))
    assert np.all(np.abs(got - w) <= bound)
    (single,), _ = moments_call(hipctx, disk[:1], 1, 2)
    assert rel_linf(w, single) > 1e-3                                    # the neighbour did something


def test_refusals_then_a_good_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    W, H, N, L = 40, 28, 1, 2
    fr, ft = xc.frames_of(W, H)[:1 + N], gc.features_of(W, H, True)[:1 + N]
    d = dev_frames(fr, L)
    f0, v0, f1, v1 = t(ft[0][0]), t(ft[0][1]), t(ft[1][0]), t(ft[1][1])
    mv = [t(gc.fields_of(W, H, 1)[0])]
    prm = params()

    def call(guided=False, **kw):
        g = {}
        if guided:
            g = dict(features=kw.get("f0", f0), neighbour_features=kw.get("nf", [f1]), variances=kw.get("v0", v0), neighbour_variances=kw.get("nv", [v1]),
                     floors=kw.get("floors", gc.FLOORS), threshold=kw.get("tau", 1.0))
        return hipctx.denoise_temporal_moments(d[0][0], d[0][1], kw.get("nb", d[1:]), kw.get("S", 1), kw.get("prm", prm), var_floor=kw.get("eps", xc.VAR_FLOOR),
                                               motions=kw.get("mv", mv), outs=kw.get("outs"), **g)

    def refused(fn, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            fn()
        assert code is None or ("rc=%d" % code) in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                     # with neighbours, any geometry but w = 1, b = 6
        refused(lambda: call(prm=bh.default_params(m=1.0, random_order=1, w=w, b=b, tau=xc.TAU)), -4)
    refused(lambda: call(S=9))                                           # what the layered motion call refuses: too many scales ...
    refused(lambda: call(nb=d[1:] * 5, mv=mv * 5))                       # ... five neighbours
    refused(lambda: call(outs=[d[0][1][0][0], torch.empty((H, W, 3), device="cuda")]))   # ... an output that is an input
    refused(lambda: call(outs=[torch.empty((H, W, 3), device="cuda"), d[1][1][0][0]]))   # ... or a neighbour's input
    both = torch.zeros((H * W * 3,), dtype=torch.float32, device="cuda")
    refused(lambda: call(mv=[both[:H * W * 2].view(H, W, 2)], outs=[both.view(H, W, 3), torch.empty((H, W, 3), device="cuda")]))   # ... an output on a motion field
    refused(lambda: call(eps=-1.0))                                      # what bcd_hip_denoise_moments refuses
    refused(lambda: call(eps=float("nan")))
    refused(lambda: call(True, nv=None))                                 # with a guide, what the guided temporal call refuses: variances in the frame only
    refused(lambda: call(True, tau=-1.0))
    refused(lambda: call(True, floors=(0.1, float("inf"), 0.1)))
    refused(lambda: call(True, f0=both.view(H, W, 3), outs=[both.view(H, W, 3), torch.empty((H, W, 3), device="cuda")]))      # an output on a feature image
    Lb = bh.lib()
    arr, _, outs = hipctx._layer_array(d[0][1], None, H, W, "cuda")
    nb, keep = hipctx._moment_frames_array(d[1:], L, H, W, lambda x: x.data_ptr(), torch.numel)
    g, alive = hipctx._guide(f0, v0, gc.FLOORS, 1.0)
    ng = (bh.GuideImages * 1)(bh.GuideImages(f1.data_ptr(), v1.data_ptr()))
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    raw = lambda h, ns, guide, guides: Lb.bcd_hip_denoise_temporal_moments(h, ns, nb, 1, None, W, H, 1, C.byref(prm), xc.VAR_FLOOR, arr, L, guide, guides)
    assert raw(None, d[0][0].data_ptr(), None, None) == -1               # a null context
    assert raw(hipctx.h, None, None, None) == -1                         # null sample counts
    assert raw(hipctx.h, d[0][0].data_ptr(), C.byref(g), None) == -1     # a guide without the neighbours' images
    assert raw(hipctx.h, d[0][0].data_ptr(), None, ng) == -1             # ... and the reverse
    ng[0].features = None
    assert raw(hipctx.h, d[0][0].data_ptr(), C.byref(g), ng) == -1       # a NULL neighbour feature pointer
    assert all(float(o.abs().sum()) == 0.0 for o in outs)                # nothing ran
    del alive, keep
    outs, stats = moments_call(hipctx, fr, L, 1)                         # (NULL motion list: nothing is warped)
    want, wstats = xc.reference(W, H, 1, N, L, False, False)
    assert stats == wstats
    for k in range(L):
        assert rel_linf(outs[k], want[k]) <= TOL


def test_benefit_of_two_neighbour_frames(hipctx):
    """NumPy composition (CPU, float64 estimate): RMSE 0.00949 with two neighbours over 0.01852 for the single frame, ratio 0.513; the device ratio must be
    below 1 and within 0.02 of it (the agreement the guide's benefit test showed).  MI355X: 0.513"""
    sc = xc.benefit_scene()
    prm = params(0.0, 0, xc.B_TAU)
    (temporal,), _ = moments_call(hipctx, sc["frames"], 1, 1, prm=prm, eps=xc.B_FLOOR)
    (single,), _ = moments_call(hipctx, sc["frames"][:1], 1, 1, prm=prm, eps=xc.B_FLOOR)
    g, p = xc.rmse(temporal, sc), xc.rmse(single, sc)
    rg, rp = xc.benefit_reference()
    print("benefit: GPU temporal RMSE %.5f, single frame %.5f, ratio %.3f; NumPy composition temporal %.5f, single frame %.5f, ratio %.3f" % (g, p, g / p, rg, rp, rg / rp))
    assert rg / rp < 0.9
    assert g / p < 1.0
    assert abs(g / p - rg / rp) <= 0.02
