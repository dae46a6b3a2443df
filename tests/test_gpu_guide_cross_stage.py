"""GPU tests of the stage calls of the cross-frame feature gate (bcd_hip_similarity_masks_guide_cross, bcd_hip_window_distances_guide_cross,
bcd_hip_warp_features; DESIGN 16, "Features") against tests/guide_cross_ref.py.  Every pixel, every mask word and every count are compared, with no tolerance
and nothing left out; distances are compared by their bits.

  * the geometries of tests/guide_cross_cases.py: widths 63, 64, 65, 70 (tile edge, tile edge plus halo), heights 4, 5, 9, a frame smaller than the window
    (9 x 7 at b = 6), 20 x 12 at b = 12 and 15 with w = 2 (several staging bands), b in {1, 2, 6} at w = 1, w = 0 and 2, F in {1, 3, 8} with and without
    variances; the constructed cases of tests/test_guide_cross_cases_cpu.py (rolled, special values);
  * device views off 16-byte alignment; the identity case against bcd_hip_similarity_masks_guide on the same context; a histogram cross call at a larger
    geometry first, so that unwritten plane entries hold foreign values;
  * bcd_hip_warp_features bit for bit against motion_ref, validity included, F = 1, 3, 8, fields with NaN, out-of-image and half-integer entries, sentinel
    margins around the outputs;
  * refusals, then a good call."""
import numpy as np
import pytest

import guide_cross_cases as gc
import guide_cross_ref as gx
import motion_cases as mc
import temporal_cases as tc

pytestmark = pytest.mark.gpu

F32 = np.float32


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def off_aligned(a):
    """a contiguous device view of `a` that starts 4 bytes past a 16-byte boundary"""
    import torch
    if a is None:
        return None
    buf = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    view = buf[1:].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def gpu_masks(ctx, c, w, b, put=t):
    m, n = ctx.similarity_masks_guide_cross(put(c["f"]), put(c["v"]), put(c["f_nb"]), put(c["v_nb"]), c["floors"], c["tau"], w, b)
    return m.cpu().numpy().view(np.uint32), n.cpu().numpy()


def check_case(ctx, c, w, b, put=t, pixels=3):
    H, W, _ = c["f"].shape
    want_m, want_n = gx.cross_masks(c["f"], c["v"], c["f_nb"], c["v_nb"], w, b, c["floors"], c["tau"])
    m, n = gpu_masks(ctx, c, w, b, put)
    assert np.array_equal(n, want_n), np.argwhere(n != want_n)[:5]
    assert np.array_equal(m, want_m), np.argwhere(m != want_m)[:5]
    dist = gx.cross_distances(c["f"], c["v"], c["f_nb"], c["v_nb"], w, b, c["floors"])
    for (l, col) in [(w, w), (H - 1 - w, W - 1 - w), (H // 2, W // 2), (w, W - 1 - w)][:pixels]:
        got = ctx.window_distances_guide_cross(put(c["f"]), put(c["v"]), put(c["f_nb"]), put(c["v_nb"]), c["floors"], w, b, l, col)
        ok = ~(np.isnan(got) & np.isnan(dist[l, col]))                  # (a NaN is a NaN: 0 / 0 has one bit pattern here, inf - inf another)
        assert np.array_equal(np.isnan(got), np.isnan(dist[l, col])), (l, col)
        assert np.array_equal(got.view(np.uint32)[ok], dist[l, col].view(np.uint32)[ok]), (l, col)
    return want_n


@pytest.mark.parametrize("W,H,F,var,w,b", gc.STAGE_GEOMETRIES)
def test_masks_and_distances_against_the_reference(hipctx, W, H, F, var, w, b):
    n = check_case(hipctx, gc.stage_images(W, H, F, var), w, b)
    assert n.max() >= 2


def test_constructed_cases(hipctx):
    check_case(hipctx, gc.rolled(40, 14), 1, 6, pixels=4)
    check_case(hipctx, gc.special(24, 12), 1, 6, pixels=4)
    c = gc.special(24, 12)
    got = hipctx.window_distances_guide_cross(t(c["f"]), None, t(c["f_nb"]), None, c["floors"], 1, 6, *gc.NAN_AT)
    assert np.isnan(got[6 * 13 + 6])                                     # the pixel whose patch is all NaN: 0 / 0 at delta = 0


@pytest.mark.parametrize("F,var", [(3, True), (8, False), (1, True)])
def test_views_off_16_byte_alignment(hipctx, F, var):
    check_case(hipctx, gc.stage_images(65, 9, F, var), 1, 6, put=off_aligned, pixels=1)


@pytest.mark.parametrize("F,var,w,b", [(3, True, 1, 6), (8, True, 2, 15), (2, False, 1, 2)])
def test_identity_equals_the_in_frame_feature_masks_on_the_same_context(hipctx, F, var, w, b):
    c = gc.identity(70, 11, F, var)
    m, n = gpu_masks(hipctx, c, w, b)
    m0, n0 = hipctx.similarity_masks_guide(t(c["f"]), t(c["v"]), c["floors"], c["tau"], w, b)
    hipctx.synchronize()
    assert np.array_equal(m, m0.cpu().numpy().view(np.uint32)) and np.array_equal(n, n0.cpu().numpy())
    assert n.max() > 1


def test_after_a_histogram_cross_call_at_a_larger_geometry(hipctx):
    hist, ns = tc.frame(96, 20, 12, 16, 5)
    hist_nb, ns_nb = tc.frame(96, 20, 12, 16, 6)
    hipctx.similarity_masks_cross(t(hist), t(ns), t(hist_nb), t(ns_nb), 1, 6, 1.0)   # leaves its planes (larger strides, other values) in the workspace
    for (W, H, F, var, w, b) in ((9, 7, 3, True, 1, 6), (20, 12, 8, True, 2, 6), (65, 5, 1, False, 1, 2)):
        check_case(hipctx, gc.stage_images(W, H, F, var), w, b, pixels=2)


SENTINEL = 0x7fbadbad


def with_margins(shape, dtype):
    """a device tensor of `shape` inside a buffer whose margins hold a sentinel -> (buffer, view)"""
    import torch
    n, pad = int(np.prod(shape)), 64
    buf = torch.full((n + 2 * pad,), SENTINEL if dtype is torch.int32 else 0xAB, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n].view(*shape)


@pytest.mark.parametrize("F,var", [(1, False), (3, True), (8, True)])
@pytest.mark.parametrize("field", ["special", "ties", "checker", None])
def test_warp_features_bit_for_bit(hipctx, F, var, field):
    import torch
    W, H = 65, 9                                                         # 585 pixels: two full workgroups and a part
    f = mc.bit_patterns((H, W, F), 21 + F)
    v = mc.bit_patterns((H, W, F), 31 + F) if var else None
    mv = None if field is None else mc.field(field, W, H)
    want_f, want_v, want_valid = gx.warp_features(f, v, mv)
    bf, of = with_margins((H, W, F), torch.int32)
    bv, ov = with_margins((H, W, F), torch.int32) if var else (None, None)
    bm, valid = with_margins((H, W), torch.uint8)
    hipctx.warp_features(t(f), t(v), t(mv), out=(of.view(torch.float32), None if ov is None else ov.view(torch.float32), valid))
    hipctx.synchronize()
    assert np.array_equal(of.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    if var:
        assert np.array_equal(ov.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
    for buf, n in ((bf, H * W * F), (bv, H * W * F), (bm, H * W)):
        if buf is not None:
            a = buf.cpu().numpy()
            fill = SENTINEL if a.dtype == np.int32 else 0xAB
            assert (a[:64] == fill).all() and (a[64 + n:] == fill).all()
    if field in ("special", "checker"):
        assert 0 < want_valid.sum() < want_valid.size


def test_refusals_then_a_good_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    c = gc.stage_images(30, 11, 3, True)
    d = {k: t(c[k]) for k in ("f", "v", "f_nb", "v_nb")}

    def refused(call, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert code is None or ("rc=%d" % code) in str(e.value), str(e.value)

    good = lambda **kw: hipctx.similarity_masks_guide_cross(kw.get("f", d["f"]), kw.get("v", d["v"]), kw.get("f_nb", d["f_nb"]), kw.get("v_nb", d["v_nb"]),
                                                            kw.get("floors", c["floors"]), kw.get("tau", 1.0), kw.get("w", 1), kw.get("b", 6))
    refused(lambda: good(v_nb=None))                                     # variances on one side only
    refused(lambda: good(v=None))
    refused(lambda: good(b=16), -4)                                      # what bcd_hip_similarity_masks_cross refuses
    refused(lambda: good(w=6))                                           # image smaller than a patch
    refused(lambda: good(tau=-1.0))                                      # the guide's own rules
    refused(lambda: good(tau=float("nan")))
    refused(lambda: good(floors=[0.1, -0.1, 0.1]))
    refused(lambda: good(v=None, v_nb=None, floors=[0.0, 0.0, 0.0]))     # no channel can count
    nine = torch.zeros((11, 30, 9), dtype=torch.float32, device="cuda")
    refused(lambda: good(f=nine, v=nine, f_nb=nine, v_nb=nine, floors=[0.1] * 9))
    refused(lambda: hipctx.window_distances_guide_cross(d["f"], d["v"], d["f_nb"], d["v_nb"], c["floors"], 1, 6, 0, 5))     # not a main pixel
    refused(lambda: hipctx.window_distances_guide_cross(d["f"], d["v"], d["f_nb"], None, c["floors"], 1, 6, 5, 5))
    L = bh.lib()
    g, alive = hipctx._guide(d["f"], d["v"], c["floors"], 1.0)
    ng = bh.GuideImages(d["f_nb"].data_ptr(), d["v_nb"].data_ptr())
    m, n = bh._mask_and_count(11, 30, 6, "cuda")
    torch.cuda.synchronize()
    assert L.bcd_hip_similarity_masks_guide_cross(None, C.byref(g), C.byref(ng), 30, 11, 1, 6, m.data_ptr(), n.data_ptr()) == -1
    assert L.bcd_hip_similarity_masks_guide_cross(hipctx.h, None, C.byref(ng), 30, 11, 1, 6, m.data_ptr(), n.data_ptr()) == -1
    assert L.bcd_hip_similarity_masks_guide_cross(hipctx.h, C.byref(g), None, 30, 11, 1, 6, m.data_ptr(), n.data_ptr()) == -1
    assert L.bcd_hip_similarity_masks_guide_cross(hipctx.h, C.byref(g), C.byref(ng), 30, 11, 1, 6, None, n.data_ptr()) == -1
    assert L.bcd_hip_similarity_masks_guide_cross(hipctx.h, C.byref(g), C.byref(bh.GuideImages(None, d["v_nb"].data_ptr())), 30, 11, 1, 6, m.data_ptr(), n.data_ptr()) == -1
    assert int(m.abs().sum()) == 0 and int(n.sum()) == 0                 # nothing ran
    # the warp: a destination on its source, on the field, a missing or a surplus variance destination, nine channels
    mv = t(mc.field("ties", 30, 11))
    refused(lambda: hipctx.warp_features(d["f"], d["v"], mv, out=(d["f"], torch.empty_like(d["v"]), torch.empty((11, 30), dtype=torch.uint8, device="cuda"))))
    both = torch.zeros((11 * 30 * 3,), dtype=torch.float32, device="cuda")
    refused(lambda: hipctx.warp_features(d["f"], None, both[:11 * 30 * 2].view(11, 30, 2), out=(both.view(11, 30, 3), None, torch.empty((11, 30), dtype=torch.uint8, device="cuda"))))
    refused(lambda: hipctx.warp_features(d["f"], d["v"], mv, out=(torch.empty_like(d["f"]), None, torch.empty((11, 30), dtype=torch.uint8, device="cuda"))))
    refused(lambda: hipctx.warp_features(d["f"], None, mv, out=(torch.empty_like(d["f"]), torch.empty_like(d["f"]), torch.empty((11, 30), dtype=torch.uint8, device="cuda"))))
    refused(lambda: hipctx.warp_features(nine, None, mv))
    del alive
    check_case(hipctx, c, 1, 6, pixels=2)
    of, ov, valid = hipctx.warp_features(d["f"], d["v"], mv)
    hipctx.synchronize()
    wf, wv, wvalid = gx.warp_features(c["f"], c["v"], mc.field("ties", 30, 11))
    assert np.array_equal(of.cpu().numpy().view(np.uint32), wf.view(np.uint32)) and np.array_equal(valid.cpu().numpy(), wvalid)
