"""GPU tests of the guided temporal frame call (bcd_hip_denoise_temporal_guided[_host]; DESIGN 16, "Features") against the NumPy composition of
tests/guide_cross_ref.py on the inputs of tests/guide_cross_cases.py.

  * 40x28, 52x36 and 64x44, 1 and 2 scales, N = 1 and 2, L = 1 and 3, with and without variances: processed / fallback / similar_total of every scale equal the
    reference's, every output is within TOL = 1e-4 of it relative to its maximum (the project's frame bar); the same with motion fields that contain invalid
    pixels.  Measured on the MI355X: at most 3.0e-7 on the frame and the smooth share, 7.8e-7 on the textured share (layer 2);
  * a guide that can gate nothing (the same constant features in every frame, floors 1) gives the stats of bcd_hip_denoise_temporal_layers[_motion] and outputs
    within TOL_SAME = 1e-5 of its: the same arithmetic, differing only in the order of the float atomics;
  * nb_neighbours == 0 equals bcd_hip_denoise_guided; the host call equals the resident call;
  * a plain bcd_hip_denoise, a bcd_hip_denoise_guided and a bcd_hip_denoise_temporal after guided temporal calls on the same context equal a fresh context's;
  * refusals, then a good call;
  * benefit: the two-albedo scene of guide_cross_cases.benefit_scene, whose edge stands elsewhere in the neighbours, no motion field given: the RMSE against the
    noise-free base over the band the edge sweeps is lower with the guide than without.  NumPy composition: ratio 0.681; MI355X: 0.681."""
import numpy as np
import pytest

import guide_cross_cases as gc
from test_gpu_temporal import TOL, rel_linf, stats_of

pytestmark = pytest.mark.gpu

TOL_SAME = 1e-5
F32 = np.float32


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def params(m=gc.M, r=gc.R):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=gc.SEED)


def dev_frames(fr, L):
    return [(t(ns), t(hist), [(t(c), t(v)) for c, v in lay[:L]]) for ns, hist, lay in fr]


def guided_call(ctx, fr, ft, L, S, fields=None, floors=gc.FLOORS, tau_g=gc.TAU_G, prm=None):
    d = dev_frames(fr, L)
    var = ft[0][1] is not None
    outs = ctx.denoise_temporal_guided(d[0][0], d[0][1], d[0][2], d[1:], S, prm or params(), t(ft[0][0]), [t(f) for f, _ in ft[1:]],
                                       variances=t(ft[0][1]), neighbour_variances=[t(v) for _, v in ft[1:]] if var else None, floors=floors, threshold=tau_g,
                                       motions=None if fields is None else [t(f) for f in fields])
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs], stats_of(ctx, S)


def check_against_reference(ctx, cfg, motion):
    W, H, S, N, L, var = cfg
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.features_of(W, H, var)[:1 + N]
    outs, stats = guided_call(ctx, fr, ft, L, S, gc.fields_of(W, H, N) if motion else None)
    want, wstats = gc.reference(W, H, S, N, L, var, motion)
    assert stats == wstats, (stats, wstats)
    assert all(s["processed"] > 0 and s["similar_total"] > 0 for s in stats)
    for k in range(L):
        e = rel_linf(outs[k], want[k])
        print("guided temporal %s%s layer %d: %s, against float64 %.2e" % (cfg, " motion" if motion else "", k, stats, e))
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("cfg", gc.CONFIGS)
def test_whole_call_against_the_reference_composition(hipctx, cfg):
    check_against_reference(hipctx, cfg, False)


@pytest.mark.parametrize("cfg", gc.MOTION_CONFIGS)
def test_whole_call_with_motion_fields_against_the_reference_composition(hipctx, cfg):
    check_against_reference(hipctx, cfg, True)


@pytest.mark.parametrize("W,H,S,N,L,motion", [(52, 36, 2, 2, 3, False), (64, 44, 2, 1, 1, True), (40, 28, 1, 2, 3, True)])
def test_a_guide_that_gates_nothing_is_the_unguided_call(hipctx, W, H, S, N, L, motion):
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.neutral_features(W, H)[:1 + N]
    fields = gc.fields_of(W, H, N) if motion else None
    outs, stats = guided_call(hipctx, fr, ft, L, S, fields, floors=(1.0, 1.0))
    d = dev_frames(fr, L)
    if motion:
        plain = hipctx.denoise_temporal_layers_motion(d[0][0], d[0][1], d[0][2], d[1:], [t(f) for f in fields], S, params())
    else:
        plain = hipctx.denoise_temporal_layers(d[0][0], d[0][1], d[0][2], d[1:], S, params())
    hipctx.synchronize()
    assert stats == stats_of(hipctx, S)
    for k in range(L):
        e = rel_linf(outs[k], plain[k].cpu().numpy())
        print("neutral guide %dx%d S=%d N=%d L=%d%s layer %d: against the unguided call %.2e" % (W, H, S, N, L, " motion" if motion else "", k, e))
        assert e <= TOL_SAME, (k, e)


@pytest.mark.parametrize("S,L,var", [(1, 1, False), (2, 3, True)])
def test_no_neighbours_is_the_guided_call(hipctx, S, L, var):
    W, H = 52, 36
    fr, ft = gc.frames_of(W, H)[:1], gc.features_of(W, H, var)[:1]
    outs, stats = guided_call(hipctx, fr, ft, L, S)
    d = dev_frames(fr, L)
    want = hipctx.denoise_guided(d[0][0], d[0][1], d[0][2], S, params(), t(ft[0][0]), variances=t(ft[0][1]), floors=gc.FLOORS, threshold=gc.TAU_G)
    hipctx.synchronize()
    assert stats == stats_of(hipctx, S)
    for k in range(L):
        assert rel_linf(outs[k], want[k].cpu().numpy()) <= TOL_SAME, k


@pytest.mark.parametrize("cfg,motion", [((40, 28, 2, 2, 3, True), True), ((52, 36, 1, 1, 1, False), True), ((40, 28, 1, 2, 3, False), False)])
def test_host_call_equals_the_resident_call(hipctx, cfg, motion):
    W, H, S, N, L, var = cfg
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.features_of(W, H, var)[:1 + N]
    fields = gc.fields_of(W, H, N) if motion else None
    if motion and N == 2:
        fields[1] = None
    want, wstats = guided_call(hipctx, fr, ft, L, S, fields)
    got = hipctx.denoise_temporal_guided_host(fr[0][0], fr[0][1], fr[0][2][:L], [(ns, hist, lay[:L]) for ns, hist, lay in fr[1:]], S, params(), ft[0][0],
                                              [f for f, _ in ft[1:]], variances=ft[0][1], neighbour_variances=[v for _, v in ft[1:]] if var else None,
                                              floors=gc.FLOORS, threshold=gc.TAU_G, motions=fields)
    assert stats_of(hipctx, S) == wstats
    for k in range(L):
        assert rel_linf(got[k], want[k]) <= TOL_SAME, k
    none = hipctx.denoise_temporal_guided_host(fr[0][0], fr[0][1], fr[0][2][:L], [], S, params(), ft[0][0], [], variances=ft[0][1], floors=gc.FLOORS, threshold=gc.TAU_G)
    d = dev_frames(fr[:1], L)
    want0 = hipctx.denoise_guided(d[0][0], d[0][1], d[0][2], S, params(), t(ft[0][0]), variances=t(ft[0][1]), floors=gc.FLOORS, threshold=gc.TAU_G)
    hipctx.synchronize()
    for k in range(L):
        assert rel_linf(none[k], want0[k].cpu().numpy()) <= TOL, k


def test_other_calls_after_guided_temporal_calls_equal_a_fresh_context_s():
    import bcd_amd.hip as bh
    W, H = 40, 28
    prm = params()
    fr, ft = gc.frames_of(W, H), gc.features_of(W, H, True)
    frame = (fr[0][2][0][0], fr[0][0], fr[0][1], fr[0][2][0][1])
    nbs = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:]]
    out = {}
    for which in ("after", "fresh"):
        ctx = bh.Context(0)
        try:
            if which == "after":
                big, bft = gc.frames_of(64, 44), gc.features_of(64, 44, True)
                guided_call(ctx, big, bft, 3, 2, gc.fields_of(64, 44, 2), prm=prm)
                guided_call(ctx, fr[:2], ft[:2], 1, 1, prm=prm)
            a = ctx.denoise(*[t(x) for x in frame], 2, prm)
            ctx.synchronize()
            sa = stats_of(ctx, 2)
            d = dev_frames(fr[:1], 2)
            b = ctx.denoise_guided(d[0][0], d[0][1], d[0][2], 2, prm, t(ft[0][0]), variances=t(ft[0][1]), floors=gc.FLOORS, threshold=gc.TAU_G)
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


@pytest.mark.parametrize("S,L,var,motion", [(1, 1, False, False), (2, 2, True, True)])
def test_set_neighbour_guide_features_is_the_resident_call(hipctx, S, L, var, motion):
    import bcd_amd.core as core
    W, H, N = 52, 36, 2
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.features_of(W, H, var)[:1 + N]
    fields = gc.fields_of(W, H, N) if motion else None
    if motion:
        fields[1] = None
    ok, got = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2][:L], [(ns, hist, lay[:L]) for ns, hist, lay in fr[1:]], nscales=S, seed=gc.SEED, m=gc.M,
                                           motions=fields, features=ft[0][0], variances=ft[0][1], neighbour_features=[f for f, _ in ft[1:]],
                                           neighbour_variances=[v for _, v in ft[1:]] if var else None, floors=gc.FLOORS, threshold=gc.TAU_G)
    assert ok
    want, _ = guided_call(hipctx, fr, ft, L, S, fields)
    for k in range(L):
        e = rel_linf(got[k], want[k])
        print("setNeighbourGuideFeatures S=%d L=%d layer %d: against the resident call %.2e" % (S, L, k, e))
        assert e <= TOL_SAME, (k, e)


def test_cli_neighbour_features_is_the_resident_call(hipctx, tmp_path):
    """the bound of tests/test_gpu_guide_host.py: bcd_cli writes its colours in half precision, so TOL_SAME of the resident result's maximum plus the rounding
    to binary16 of a value that close (2^-11 relative in the normal range, 2^-25 absolute below)"""
    import os
    import subprocess
    import bcd_amd.core as core
    W, H, N = 52, 36, 1
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.features_of(W, H, True)[:1 + N]
    disk = []
    for i, (ns, hist, lay) in enumerate(fr):
        stem = str(tmp_path / ("frame%d" % i))
        core.write_exr(stem + ".exr", lay[0][0], False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        core.write_exr(stem + "_cov.exr", lay[0][1], True)
        core.write_exr(stem + "_f.exr", ft[i][0], True)
        core.write_exr(stem + "_fv.exr", ft[i][1], True)
        disk.append((ns, hist, [(core.read_exr(stem + ".exr", False), lay[0][1])]))      # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    s0, s1 = str(tmp_path / "frame0"), str(tmp_path / "frame1")
    r = subprocess.run([exe, "-i", s0 + ".exr", "-o", out_path, "-p", "0", "-s", "2", "-m", "1", "--seed", str(gc.SEED), "--features", s0 + "_f.exr", "--feature-variances",
                        s0 + "_fv.exr", "--feature-floors", ",".join(str(x) for x in gc.FLOORS), "--neighbour", s1 + ".exr", "--neighbour-features", s1 + "_f.exr",
                        "--neighbour-feature-variances", s1 + "_fv.exr"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    (want,), _ = guided_call(hipctx, disk, ft, 1, 2)
    w = hipctx.zero_bad_values(t(want)).cpu().numpy()
    got = core.read_exr(out_path, False)
    same = TOL_SAME * np.max(np.abs(w))
    bound = same + np.maximum(2.0 ** -11 * (np.abs(w) + same), 2.0 ** -25)
    print("bcd_cli --neighbour-features: worst deviation from the resident call %.3f of the bound (TOL_SAME + binary16 rounding)" % float(np.max(np.abs(got - w) / bound)))
    assert np.all(np.abs(got - w) <= bound)
    (plain,) = hipctx.denoise_temporal_layers(*[x for x in dev_frames(disk, 1)[0]], dev_frames(disk, 1)[1:], 2, params())
    assert rel_linf(w, plain.cpu().numpy()) > 1e-3                      # the gate did something


def test_refusals_then_a_good_call(hipctx):
    import torch
    import bcd_amd.hip as bh
    W, H, N, L = 40, 28, 1, 2
    fr, ft = gc.frames_of(W, H)[:1 + N], gc.features_of(W, H, True)[:1 + N]
    d = dev_frames(fr, L)
    f0, v0, f1, v1 = t(ft[0][0]), t(ft[0][1]), t(ft[1][0]), t(ft[1][1])
    mv = [t(gc.fields_of(W, H, 1)[0])]
    prm = params()

    def call(**kw):
        return hipctx.denoise_temporal_guided(d[0][0], kw.get("hist", d[0][1]), d[0][2], kw.get("nb", d[1:]), kw.get("S", 1), kw.get("prm", prm), kw.get("f0", f0),
                                              kw.get("nf", [f1]), variances=kw.get("v0", v0), neighbour_variances=kw.get("nv", [v1]), floors=kw.get("floors", gc.FLOORS),
                                              threshold=kw.get("tau", 1.0), motions=kw.get("mv", mv), outs=kw.get("outs"))

    def refused(fn, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            fn()
        assert code is None or ("rc=%d" % code) in str(e.value) or "support" in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                     # with neighbours, any geometry but w = 1, b = 6
        refused(lambda: call(prm=bh.default_params(m=1.0, random_order=1, w=w, b=b)), -4)
    refused(lambda: call(S=9))                                           # what the layered motion call refuses: too many scales ...
    refused(lambda: call(nb=d[1:] * 5, nf=[f1] * 5, nv=[v1] * 5, mv=mv * 5))          # ... five neighbours
    refused(lambda: call(outs=[d[0][2][0][0], torch.empty((H, W, 3), device="cuda")]))   # ... an output that is an input
    refused(lambda: call(nv=None))                                       # variances in the frame, none in the neighbour
    refused(lambda: call(v0=None))                                       # ... and the reverse
    refused(lambda: call(tau=-1.0))                                      # what the guided call refuses
    refused(lambda: call(floors=(0.1, float("inf"), 0.1)))
    refused(lambda: call(v0=None, nv=None, floors=(0.0, 0.0, 0.0)))
    both = torch.zeros((H * W * 3,), dtype=torch.float32, device="cuda")
    refused(lambda: call(f0=both.view(H, W, 3), outs=[both.view(H, W, 3), torch.empty((H, W, 3), device="cuda")]))      # an output on a feature image
    refused(lambda: call(nv=[both.view(H, W, 3)], outs=[torch.empty((H, W, 3), device="cuda"), both.view(H, W, 3)]))    # ... on a neighbour's variances
    with pytest.raises(ValueError):
        call(nf=[f1, f1])                                                # a miscounted list never reaches the library
    import ctypes as C
    Lb = bh.lib()
    arr, _, outs = hipctx._layer_array(d[0][2], None, H, W, "cuda")
    nb, keep = hipctx._frame_layers_array(d[1:], L, H, W, 60, lambda x: x.data_ptr(), torch.numel)
    g, alive = hipctx._guide(f0, v0, gc.FLOORS, 1.0)
    ng = (bh.GuideImages * 1)(bh.GuideImages(f1.data_ptr(), v1.data_ptr()))
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    raw = lambda hist, guide, guides: Lb.bcd_hip_denoise_temporal_guided(hipctx.h, d[0][0].data_ptr(), hist, nb, 1, None, W, H, 60, 1, C.byref(prm), arr, L, guide, guides)
    assert raw(None, C.byref(g), ng) == -1                               # no histograms: there is no cross-frame moment selection
    assert raw(d[0][1].data_ptr(), None, ng) == -1                       # a NULL guide
    assert raw(d[0][1].data_ptr(), C.byref(g), None) == -1               # a NULL list of neighbour images
    ng[0].features = None
    assert raw(d[0][1].data_ptr(), C.byref(g), ng) == -1                 # a NULL neighbour feature pointer
    assert Lb.bcd_hip_denoise_temporal_guided(None, d[0][0].data_ptr(), d[0][1].data_ptr(), nb, 1, None, W, H, 60, 1, C.byref(prm), arr, L, C.byref(g), ng) == -1
    assert all(float(o.abs().sum()) == 0.0 for o in outs)                # nothing ran
    del alive, keep
    outs, stats = guided_call(hipctx, fr, ft, L, 1)                      # (NULL motion list: nothing is warped)
    want, wstats = gc.reference(W, H, 1, N, L, True, False)
    assert stats == wstats
    for k in range(L):
        assert rel_linf(outs[k], want[k]) <= TOL


def test_benefit_across_a_moved_edge(hipctx):
    sc = gc.benefit_scene()
    prm = params(0.0, 0)
    fr = [(f[1], f[2], [(f[0], f[3])]) for f in sc["frames"]]
    (guided,), _ = guided_call(hipctx, fr, sc["guides"], 1, 1, floors=gc.B_FLOORS, tau_g=gc.B_TAU_G, prm=prm)
    d = dev_frames(fr, 1)
    (plain,) = hipctx.denoise_temporal_layers(d[0][0], d[0][1], d[0][2], d[1:], 1, prm)
    hipctx.synchronize()
    g, p = gc.band_rmse(guided, sc), gc.band_rmse(plain.cpu().numpy(), sc)
    rg, rp = gc.benefit_reference()
    print("benefit: GPU guided RMSE %.5f, unguided %.5f, ratio %.3f; NumPy composition guided %.5f, unguided %.5f, ratio %.3f" % (g, p, g / p, rg, rp, rg / rp))
    assert rg / rp <= 0.9
    assert g < p
