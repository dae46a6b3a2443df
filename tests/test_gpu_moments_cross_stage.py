"""GPU tests of the stage calls of the cross-frame moment selection (bcd_hip_similarity_masks_moments_cross, bcd_hip_window_distances_moments_cross; DESIGN 16,
"Moments") against tests/moments_cross_ref.py.  Every pixel, every mask word and every count are compared, with no tolerance and nothing left out; distances
are compared by their bits.

  * the geometries of tests/moments_cross_cases.py: widths 63, 64, 65, 70 (tile edge, tile edge plus halo), heights 4, 5, 9, a frame smaller than the window
    (9 x 7 at b = 6), b in {1, 2, 6} at w = 1 in form 1 (planes) AND form 2 (fused), which must agree with each other and with the reference; w = 0 and 2 and
    b = 12, 13 (the largest one-band LDS request), 14 and 15 (two staging bands) in form 1, where form 2 is refused with BCD_HIP_EUNSUPPORTED; form 0 is one of the two;
  * the three thresholds (1, a distance that occurs, the float below it) and both floors (0 and 1e-4);
  * the constructed cases of tests/test_moments_cross_cases_cpu.py (rolled, special values);
  * device views 4 bytes off 16-byte alignment; a histogram cross call at a larger geometry first, so that unwritten plane entries hold foreign values;
  * the identity case against bcd_hip_similarity_masks_moments on the same context;
  * refusals, then a good call."""
import numpy as np
import pytest

import moments_cross_cases as xc
import moments_cross_ref as mx
import temporal_cases as tc

pytestmark = pytest.mark.gpu

F32 = np.float32
UNSUPPORTED = -4


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def off_aligned(a):
    """a contiguous device view of `a` that starts 4 bytes past a 16-byte boundary"""
    import torch
    buf = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    view = buf[1:].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def gpu_masks(ctx, d, c, tau, form):
    m, n = ctx.similarity_masks_moments_cross(d[0], d[1], d[2], d[3], c["w"], c["b"], tau, var_floor=c["eps"], form=form)
    ctx.synchronize()
    return m.cpu().numpy().view(np.uint32), n.cpu().numpy()


def check_case(ctx, c, forms, put=t, pixels=3, taus=None):
    """every threshold of the case in every form against the reference; window distances of a few main pixels by their bits"""
    H, W, _ = c["m0"].shape
    w, b = c["w"], c["b"]
    d = [put(c[k]) for k in ("m0", "P0", "mj", "Pj")]
    last = None
    for tau in (c["taus"] if taus is None else taus):
        want_m, want_n = mx.masks_from(c["D"], c["valid"], tau)
        for form in forms:
            m, n = gpu_masks(ctx, d, c, tau, form)
            assert np.array_equal(n, want_n), (form, tau, np.argwhere(n != want_n)[:5])
            assert np.array_equal(m, want_m), (form, tau, np.argwhere(m != want_m)[:5])
        last = want_n
    if H > 2 * w and W > 2 * w:
        for (l, col) in [(w, w), (H - 1 - w, W - 1 - w), (H // 2, W // 2), (w, W - 1 - w)][:pixels]:
            got = ctx.window_distances_moments_cross(d[0], d[1], d[2], d[3], w, b, l, col, var_floor=c["eps"])
            want = mx.window_distances(c["D"], l, col)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (l, col)
            ok = ~np.isnan(want)                                           # (a NaN is a NaN: 0 / 0 has one bit pattern here, inf - inf another)
            assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), (l, col)
    return last


@pytest.mark.parametrize("W,H,w,b", xc.STAGE_FUSED)
@pytest.mark.parametrize("eps", xc.FLOORS)
def test_both_forms_against_the_reference(hipctx, W, H, w, b, eps):
    check_case(hipctx, xc.stage_case(W, H, w, b, eps), (1, 2, 0))


@pytest.mark.parametrize("W,H,w,b", xc.STAGE_PLANES_ONLY)
@pytest.mark.parametrize("eps", xc.FLOORS)
def test_planes_form_where_the_fused_form_does_not_apply(hipctx, W, H, w, b, eps):
    import bcd_amd.hip as bh
    c = xc.stage_case(W, H, w, b, eps)
    check_case(hipctx, c, (1, 0))
    d = [t(c[k]) for k in ("m0", "P0", "mj", "Pj")]
    with pytest.raises(bh.BcdHipError) as e:
        hipctx.similarity_masks_moments_cross(d[0], d[1], d[2], d[3], w, b, 1.0, var_floor=eps, form=2)
    assert ("rc=%d" % UNSUPPORTED) in str(e.value), str(e.value)


@pytest.mark.parametrize("eps", xc.FLOORS)
def test_constructed_cases(hipctx, eps):
    check_case(hipctx, xc.rolled(70, 13, 1, 6, eps), (1, 2), pixels=4)
    c = xc.special(70, 13, 1, 6, eps)
    check_case(hipctx, c, (1, 2), pixels=4, taus=list(c["taus"]) + [F32(3.0e38)])
    d = [t(c[k]) for k in ("m0", "P0", "mj", "Pj")]
    got = hipctx.window_distances_moments_cross(d[0], d[1], d[2], d[3], 1, 6, 7, 23, var_floor=eps)
    centre = got[6 * 13 + 6]                                               # inside the zero-variance block, delta = 0
    assert np.isnan(centre) if eps == 0.0 else centre == 0
    for (l, col) in (xc.INF_MEAN_FRAME, xc.NAN_MEAN_FRAME):                # a counted infinite or NaN term: nothing in the window is finite
        got = hipctx.window_distances_moments_cross(d[0], d[1], d[2], d[3], 1, 6, l, col, var_floor=eps)
        assert not np.isfinite(got).any()


@pytest.mark.parametrize("form", [1, 2])
def test_views_off_16_byte_alignment(hipctx, form):
    check_case(hipctx, xc.stage_case(65, 9, 1, 6, 1e-4), (form,), put=off_aligned, pixels=1)


def test_after_a_histogram_cross_call_at_a_larger_geometry(hipctx):
    hist, ns = tc.frame(96, 20, 12, 16, 5)
    hist_nb, ns_nb = tc.frame(96, 20, 12, 16, 6)
    hipctx.similarity_masks_cross(t(hist), t(ns), t(hist_nb), t(ns_nb), 1, 6, 1.0)   # leaves its planes (larger strides, other values) in the workspace
    for (W, H, w, b) in ((9, 7, 1, 6), (30, 11, 2, 6), (65, 9, 1, 2)):
        check_case(hipctx, xc.stage_case(W, H, w, b, 1e-4), (1,), pixels=2)


@pytest.mark.parametrize("W,H,w,b", [(70, 13, 1, 6), (40, 28, 1, 6), (65, 9, 1, 2), (30, 11, 2, 12)])
@pytest.mark.parametrize("eps", xc.FLOORS)
def test_identity_equals_the_in_frame_moment_masks_on_the_same_context(hipctx, W, H, w, b, eps):
    c = xc.identity(W, H, w, b, eps)
    d = [t(c[k]) for k in ("m0", "P0", "mj", "Pj")]
    for tau in c["taus"]:
        m0, n0 = hipctx.similarity_masks_moments(d[0], d[1], w, b, tau, var_floor=eps)
        hipctx.synchronize()
        m0, n0 = m0.cpu().numpy().view(np.uint32), n0.cpu().numpy()
        for form in ((1, 2) if w == 1 and b <= 6 else (1,)):
            m, n = gpu_masks(hipctx, d, c, tau, form)
            assert np.array_equal(m, m0) and np.array_equal(n, n0), (form, tau)
        assert n0.max() > 1


def test_refusals_then_a_good_call(hipctx):
    import torch
    import bcd_amd.hip as bh
    c = xc.stage_case(30, 11, 1, 6, 1e-4)
    d = [t(c[k]) for k in ("m0", "P0", "mj", "Pj")]

    def refused(call, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert code is None or ("rc=%d" % code) in str(e.value), str(e.value)

    good = lambda **kw: hipctx.similarity_masks_moments_cross(d[0], d[1], d[2], d[3], kw.get("w", 1), kw.get("b", 6), kw.get("tau", 1.0),
                                                              var_floor=kw.get("eps", 1e-4), form=kw.get("form", 0))
    refused(lambda: good(b=16), UNSUPPORTED)                               # what bcd_hip_similarity_masks_moments refuses
    refused(lambda: good(w=6))                                             # image smaller than a patch
    refused(lambda: good(eps=-1.0))
    refused(lambda: good(eps=float("nan")))
    refused(lambda: good(eps=float("inf")))
    refused(lambda: good(form=3))
    refused(lambda: good(form=-1))
    refused(lambda: good(form=2, b=7), UNSUPPORTED)                        # the fused form where it does not apply
    refused(lambda: good(form=2, w=2), UNSUPPORTED)
    refused(lambda: good(form=2, w=0), UNSUPPORTED)
    refused(lambda: hipctx.window_distances_moments_cross(d[0], d[1], d[2], d[3], 1, 6, 0, 5))      # not a main pixel
    refused(lambda: hipctx.window_distances_moments_cross(d[0], d[1], d[2], d[3], 1, 6, 5, 5, var_floor=-1.0))
    L = bh.lib()
    m, n = bh._mask_and_count(11, 30, 6, "cuda")
    p = [x.data_ptr() for x in d]
    torch.cuda.synchronize()
    raw = lambda h, a, bb, cc, dd, mm, nn: L.bcd_hip_similarity_masks_moments_cross(h, a, bb, cc, dd, 30, 11, 1, 6, 1.0, 1e-4, 0, mm, nn)
    assert raw(None, p[0], p[1], p[2], p[3], m.data_ptr(), n.data_ptr()) == -1
    for k in range(4):
        q = list(p)
        q[k] = None
        assert raw(hipctx.h, q[0], q[1], q[2], q[3], m.data_ptr(), n.data_ptr()) == -1
    assert raw(hipctx.h, p[0], p[1], p[2], p[3], None, n.data_ptr()) == -1
    assert raw(hipctx.h, p[0], p[1], p[2], p[3], m.data_ptr(), None) == -1
    assert int(m.abs().sum()) == 0 and int(n.sum()) == 0                   # nothing ran
    check_case(hipctx, c, (1, 2, 0), pixels=2)
