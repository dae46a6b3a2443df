"""GPU tests of the motion calls (bcd_hip_denoise_temporal_motion[_host], bcd_hip_denoise_temporal_layers_motion[_host]; DESIGN 16, "Motion").

Frames and fields from tests/motion_cases.py at 64x44 and 72x48, 1 and 3 scales, F = 1 and 2, -m 1 with the seeded random order; the inputs are held to
their claims without a GPU by tests/test_motion_cases_cpu.py (every scale has invalid pixels, members only the gate removes, fallback pixels and full
estimates).  The frame bar is the one tests/test_gpu_temporal.py uses for the same comparison, imported from there.
  * all-valid random fields: the per-scale processed / fallback / similar_total equal those of bcd_hip_denoise_temporal on the NumPy-warped neighbours, the
    frame is within the bar of that call's;
  * fields with invalid pixels: the per-scale figures equal motion_ref.denoise_multiscale_motion's, the frame is within the bar of its float64 result;
  * the translated scene (-m 0, so that both calls process every main pixel): similar_total equals the reference's and exceeds that of the plain temporal
    call on the same inputs;
  * all-None fields and a NULL-free list of None delegate; zero fields give the plain call's figures and frame; a neighbour with a field beside one without;
  * plain denoise_temporal, denoise_layers and bayes_accumulate after motion calls equal a fresh context's;
  * the layered call: layer k against the frame call on layer k, L = 1 delegates; the host calls return the resident calls' results;
  * every refusal, then a good call on the same context."""
import numpy as np
import pytest

import motion_cases as mc
import motion_ref as mo
import temporal_layers_cases as tl
from test_gpu_temporal import TOL, dev, rel_linf, stats_of

pytestmark = pytest.mark.gpu

F = np.float32


def params():
    import bcd_amd.hip as bh
    return bh.default_params(m=mc.M, random_order=mc.R, seed=mc.SEED)


def t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def fields_dev(fields):
    return [None if f is None else t(f) for f in fields]


def motion_call(ctx, fr, fields, S, prm=None):
    out = ctx.denoise_temporal_motion(*dev(fr[0]), [dev(f) for f in fr[1:]], fields_dev(fields), S, prm or params())
    ctx.synchronize()
    return out.cpu().numpy(), stats_of(ctx, S)


def plain_call(ctx, fr, S, prm=None):
    out = ctx.denoise_temporal(*dev(fr[0]), [dev(f) for f in fr[1:]], S, prm or params())
    ctx.synchronize()
    return out.cpu().numpy(), stats_of(ctx, S)


def warped(f, mv):
    H, W = f[2].shape[:2]
    (c, n, h, v), valid = mo.warp([f[0], np.asarray(f[1]).reshape(H, W, 1), f[2], f[3]], mv)
    assert valid.all()
    return c, n, h, v


@pytest.mark.parametrize("W,H,S,nf", mc.CONFIGS)
def test_all_valid_fields_are_the_plain_call_on_warped_neighbours(hipctx, W, H, S, nf):
    fr = mc.frames_of(W, H)[:1 + nf]
    fields = [mc.all_valid(W, H, f) for f in range(nf)]
    got, stats = motion_call(hipctx, fr, fields, S)
    want, wstats = plain_call(hipctx, [fr[0]] + [warped(f, mv) for f, mv in zip(fr[1:], fields)], S)
    assert stats == wstats, (stats, wstats)
    assert all(s["similar_total"] > 0 and 0 < s["fallback"] < s["processed"] for s in stats)
    e = rel_linf(got, want)
    print("motion all-valid %dx%d S=%d F=%d: %s, against the plain call on warped inputs %.2e" % (W, H, S, nf, stats, e))
    assert e <= TOL, e


@pytest.mark.parametrize("W,H,S,nf", mc.CONFIGS)
def test_fields_with_invalid_pixels_against_the_reference(hipctx, W, H, S, nf):
    fr = mc.frames_of(W, H)[:1 + nf]
    got, stats = motion_call(hipctx, fr, [mc.holes(W, H, f) for f in range(nf)], S)
    want, wstats = mc.reference("holes", W, H, S, nf)
    assert stats == wstats, (stats, wstats)
    e = rel_linf(got, want)
    print("motion holes %dx%d S=%d F=%d: %s, against float64 %.2e" % (W, H, S, nf, stats, e))
    assert e <= TOL, e


@pytest.mark.parametrize("W,H", mc.SIZES)
def test_translated_scene_finds_more_members_than_the_plain_call(hipctx, W, H):
    """-m 0 in scanline order: every main pixel is processed, so similar_total is the sum of |S_0| + |S_f| over the SAME pixels in both calls and the
    comparison is the one tests/test_motion_cases_cpu.py makes on the masks.  (With -m 1 a richer selection marks more pixels, fewer are processed, and the
    sum over the processed ones can fall: the NumPy reference itself gives 15355 with the field against 16110 without at 72x48.)"""
    import bcd_amd.hip as bh
    frame, nb, mv = mc.translated(W, H)
    prm = bh.default_params(m=0.0, random_order=0, seed=mc.SEED)
    orders, draws = mc.orders_draws(W, H, 1, m=0.0, r=0)
    want, wstats = mo.denoise_multiscale_motion(frame, [nb], [mv], 1, 1, 6, 1.0, 1e-8, orders, draws)
    got, stats = motion_call(hipctx, [frame, nb], [mv], 1, prm)
    _, plain = plain_call(hipctx, [frame, nb], 1, prm)
    print("translated %dx%d: similar_total with the field %d, plain %d" % (W, H, stats[0]["similar_total"], plain[0]["similar_total"]))
    assert stats == wstats, (stats, wstats)
    assert stats[0]["processed"] == plain[0]["processed"] == (W - 2) * (H - 2)
    assert stats[0]["similar_total"] > plain[0]["similar_total"]
    assert rel_linf(got, want) <= TOL


@pytest.mark.parametrize("S", [1, 3])
def test_delegation_and_zero_fields(hipctx, S):
    W, H = mc.SIZES[0]
    fr = mc.frames_of(W, H)
    want, wstats = plain_call(hipctx, fr, S)
    for fields in ([None, None], [np.zeros((H, W, 2), F)] * 2, [None, np.zeros((H, W, 2), F)]):
        got, stats = motion_call(hipctx, fr, fields, S)
        assert stats == wstats and rel_linf(got, want) <= TOL
    got, stats = motion_call(hipctx, fr[:1], [], S)                 # no neighbour, an empty list: bcd_hip_denoise
    plain = hipctx.denoise(*dev(fr[0]), S, params())
    hipctx.synchronize()
    assert stats == stats_of(hipctx, S) and rel_linf(got, plain.cpu().numpy()) <= TOL
    # one neighbour warped, one read where it lies: the reference with a None field
    fields = [mc.holes(W, H, 0), None]
    orders, draws = mc.orders_draws(W, H, S)
    want, wstats = mo.denoise_multiscale_motion(fr[0], fr[1:], fields, S, 1, 6, 1.0, 1e-8, orders, draws)
    got, stats = motion_call(hipctx, fr, fields, S)
    assert stats == wstats and rel_linf(got, want) <= TOL


def test_plain_calls_after_motion_calls_equal_a_fresh_context_s():
    import bcd_amd.hip as bh
    (W, H), (W2, H2) = mc.SIZES
    prm = params()
    out = {}
    fr = mc.frames_of(W, H)
    lay = tl.share_layers(fr[0][0], fr[0][3])
    for which in ("after", "fresh"):
        ctx = bh.Context(0)
        try:
            if which == "after":
                big = mc.frames_of(W2, H2)
                motion_call(ctx, big, [mc.holes(W2, H2, f) for f in range(2)], 3, prm)
                motion_call(ctx, fr[:2], [mc.holes(W, H, 0)], 1, prm)
            a, sa = plain_call(ctx, fr, 3, prm)
            b = [o.cpu().numpy() for o in ctx.denoise_layers(t(fr[0][1]), t(fr[0][2]), [(t(c), t(v)) for c, v in lay], 2, prm)]
            ctx.synchronize()
            sb = stats_of(ctx, 2)
            mask, nsim = ctx.similarity_masks(t(fr[0][2]), t(fr[0][1]), 1, 6, 1.0)
            state, _ = ctx.active_set(mask, nsim, 1, 6, prm.marked_skip_probability, prm.use_random_pixel_order, prm.order_seed)
            s, c = ctx.bayes_accumulate(t(fr[0][0]), ctx.pixel_cov(t(fr[0][3]), t(fr[0][1])), mask, nsim, state, 1, 6, prm.min_eigen_value)
            ctx.synchronize()
            out[which] = (a, sa, b, sb, ctx.finalize(s, c).cpu().numpy(), c.cpu().numpy())
        finally:
            ctx.close()
    x, y = out["after"], out["fresh"]
    assert x[1] == y[1] and x[3] == y[3] and np.array_equal(x[5], y[5])
    assert rel_linf(x[0], y[0]) <= TOL and rel_linf(x[4], y[4]) <= TOL
    for k in range(len(lay)):
        assert rel_linf(x[2][k], y[2][k]) <= TOL, k


def layered_inputs(W, H, nf):
    """[(ns, hist, [(colours, covariances)] * L)] of the frame and its neighbours: tests/temporal_layers_cases.py's shares of the frames of motion_cases"""
    return [(f[1], f[2], tl.share_layers(f[0], f[3])) for f in mc.frames_of(W, H)[:1 + nf]]


@pytest.mark.parametrize("W,H,S,nf", [(64, 44, 3, 2), (72, 48, 1, 1), (72, 48, 3, 1)])
def test_layered_call_is_the_frame_call_on_every_layer(hipctx, W, H, S, nf):
    prm = params()
    fr = layered_inputs(W, H, nf)
    fields = [mc.holes(W, H, f) for f in range(nf)]
    d = [(t(n), t(h), [(t(c), t(v)) for c, v in lay]) for n, h, lay in fr]
    outs = hipctx.denoise_temporal_layers_motion(d[0][0], d[0][1], d[0][2], d[1:], fields_dev(fields), S, prm)
    hipctx.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    stats = stats_of(hipctx, S)
    assert stats == mc.reference("holes", W, H, S, nf)[1]            # (the selection reads sample counts and histograms only)
    L = len(outs)
    assert [sum(hipctx.layer_spectral_inverses(s, k) for k in range(L)) for s in range(S)] == [hipctx.stats(s).spectral_inverses for s in range(S)]
    for k in range(L):
        single = [(f[2][k][0], f[0], f[1], f[2][k][1]) for f in fr]
        want, wstats = motion_call(hipctx, single, fields, S, prm)
        assert wstats == stats, k
        e = rel_linf(outs[k], want)
        print("motion layers %dx%d S=%d F=%d layer %d against the frame call %.2e" % (W, H, S, nf, k, e))
        assert e <= TOL, (k, e)
    (one,) = hipctx.denoise_temporal_layers_motion(d[0][0], d[0][1], d[0][2][:1], [(n, h, lay[:1]) for n, h, lay in d[1:]], fields_dev(fields), S, prm)
    hipctx.synchronize()
    want, wstats = motion_call(hipctx, [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr], fields, S, prm)          # L = 1 delegates
    assert rel_linf(one.cpu().numpy(), want) <= TOL
    plain = hipctx.denoise_temporal_layers(d[0][0], d[0][1], d[0][2], d[1:], S, prm)                                  # all-None fields delegate
    hipctx.synchronize()
    pstats = stats_of(hipctx, S)
    none = hipctx.denoise_temporal_layers_motion(d[0][0], d[0][1], d[0][2], d[1:], [None] * nf, S, prm)
    hipctx.synchronize()
    assert stats_of(hipctx, S) == pstats and all(rel_linf(a.cpu().numpy(), b.cpu().numpy()) <= TOL for a, b in zip(none, plain))


@pytest.mark.parametrize("S,nf", [(1, 1), (3, 2)])
def test_host_calls_return_the_resident_calls_results(hipctx, S, nf):
    W, H = mc.SIZES[0]
    prm = params()
    fr = mc.frames_of(W, H)[:1 + nf]
    fields = [mc.holes(W, H, f) for f in range(nf)]
    if nf == 2:
        fields[1] = None
    want, wstats = motion_call(hipctx, fr, fields, S, prm)
    got = hipctx.denoise_temporal_motion_host(*fr[0], fr[1:], fields, S, prm)
    assert stats_of(hipctx, S) == wstats and rel_linf(got, want) <= TOL
    plain, pstats = plain_call(hipctx, fr, S, prm)
    got = hipctx.denoise_temporal_motion_host(*fr[0], fr[1:], [None] * nf, S, prm)          # delegates to bcd_hip_denoise_temporal_host
    assert stats_of(hipctx, S) == pstats and rel_linf(got, plain) <= TOL


def test_refusals_then_a_good_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    W, H = mc.SIZES[0]
    fr = mc.frames_of(W, H)[:2]
    d, nb = dev(fr[0]), [dev(fr[1])]
    mv = [t(mc.holes(W, H, 0))]
    prm = params()

    def refused(call, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert code is None or ("rc=%d" % code) in str(e.value) or "support" in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                 # everything the plain call refuses: another geometry ...
        p = bh.default_params(m=1.0, random_order=1, w=w, b=b)
        refused(lambda: hipctx.denoise_temporal_motion(*d, nb, mv, 1, p), -4)
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb * 5, mv * 5, 1, prm))        # ... five neighbours
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb, mv, 9, prm))                # ... too many scales
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb, mv, 1, prm, out=d[0]))      # ... an output that is an input
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb, mv, 1, prm, out=nb[0][0]))
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb, None, 1, prm))              # a NULL field list with a neighbour present
    both = torch.zeros((H * W * 3,), dtype=torch.float32, device="cuda")               # an output that overlaps a motion field
    refused(lambda: hipctx.denoise_temporal_motion(*d, nb, [both[:H * W * 2].view(H, W, 2)], 1, prm, out=both.view(H, W, 3)))
    with pytest.raises(ValueError):                                                    # a miscounted list never reaches the library
        hipctx.denoise_temporal_motion(*d, nb, mv * 2, 1, prm)
    L = bh.lib()
    one = (bh.Frame * 1)()
    one[0].d_colors, one[0].d_nsamples, one[0].d_histograms, one[0].d_covariances = (x.data_ptr() for x in nb[0])
    fields = (C.c_void_p * 1)(mv[0].data_ptr())
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ptrs = [x.data_ptr() for x in d]
    call = lambda frames, n, f=fields: L.bcd_hip_denoise_temporal_motion(hipctx.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], frames, n, f, W, H, 60, 1, C.byref(prm), out.data_ptr())
    one[0].reserved = mv[0].data_ptr()
    assert call(one, 1) == -1                                        # `reserved` keeps its meaning: NULL, or refused
    one[0].reserved = None
    assert call(one, 1, None) == -1 and call(None, 1) == -1 and call(one, 5) == -1
    assert float(out.abs().sum()) == 0.0                             # nothing ran
    # the layered call: a NULL list, an output on a field
    lay = layered_inputs(W, H, 1)
    dl = [(t(n), t(h), [(t(c), t(v)) for c, v in x]) for n, h, x in lay]
    refused(lambda: hipctx.denoise_temporal_layers_motion(dl[0][0], dl[0][1], dl[0][2], dl[1:], None, 1, prm))
    outs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)] + [both.view(H, W, 3)]
    refused(lambda: hipctx.denoise_temporal_layers_motion(dl[0][0], dl[0][1], dl[0][2], dl[1:], [both[:H * W * 2].view(H, W, 2)], 1, prm, outs=outs))
    got, stats = motion_call(hipctx, fr, [mc.holes(W, H, 0)], 1, prm)
    want, wstats = mc.reference("holes", W, H, 1, 1)
    assert stats == wstats and rel_linf(got, want) <= TOL
