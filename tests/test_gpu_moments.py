"""GPU tests of bcd_hip_denoise_moments: a frame denoised with similar patches selected from the guide's means and covariances, no histogram.
Frames are 90 x 52 (levels 45 x 26 and 22 x 13: widths of both parities), seeded two-region noise at 8 spp (tests/moments_cases.py).
  (a) one scale: the frame call is the composition of the stage calls (scale_begin, similarity_masks_moments, active_set, bayes_accumulate, finalize);
  (b) three scales with a kept selection: per scale the kept masks and |S| are, bit for bit, the stage call on levels built with downscale_avg / _sum /
      _cov + pixel_cov, the kept processed pixels are active_set's on them, the selection's own denoise reproduces the outputs, the info shows D = 0, path 3;
  (c) 2 and 16 layers: layer k of the call is the kept guide-only selection's denoise of layer k;
  (d) the host call is the resident call, and with a spike factor spike_filter_layers (no histograms) followed by the resident call;
  (e) every refusal, followed by a successful call on the same context;
  (f) a histogram call of another frame gives the same result before and after a moments call.
"The same" between two runs of the same build is the project's bar: 1e-5 relative L-inf, equal non-finite patterns (the float atomics of the aggregation
arrive in another order).  The selection stage alone, against the NumPy reference: tests/test_gpu_moments_stage.py."""
import ctypes as C

import numpy as np
import pytest

import moments_cases as mc
from test_gpu_layers import TOL_SAME, dev, frame, rel_linf

pytestmark = pytest.mark.gpu

W, H = 90, 52
EPS = 1e-6
_shared = {}


def shared(ctx):
    """the frame on the device, 16 layers of it, and the three-scale call on the guide alone with its kept selection (once per session)"""
    import bcd_amd.hip as bh
    if not _shared:
        col, cov, ns, _ = mc.noisy(W, H, seed=7)
        layers = mc.layers_of(col, cov, 16)
        prm = bh.default_params(m=1.0, random_order=1, seed=21)
        d_ns, = dev(ns)
        d_layers = [tuple(dev(c, v)) for c, v in layers]
        sel = ctx.selection()
        guide = ctx.denoise_moments(d_ns, d_layers[:1], 3, prm, EPS, keep=sel)[0].cpu().numpy()
        stats = [ctx.stats(s) for s in range(3)]
        _shared.update(col=col, cov=cov, ns=ns, layers=layers, prm=prm, d_ns=d_ns, d_layers=d_layers, sel=sel, guide=guide,
                       stats=[(s.processed, s.fallback, s.similar_total, s.similarity_path, s.borderline_pairs) for s in stats])
    return _shared


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(m=1.0, random_order=1, seed=5), dict(m=0.0, random_order=0), dict(w=2, b=3, m=1.0, random_order=0, tau=1.5)])
def test_one_scale_is_the_composition_of_the_stage_calls(hipctx, kw):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm = bh.default_params(**kw)
    w, b = prm.patch_radius, prm.search_radius
    d_col, d_cov = c["d_layers"][0]
    got = hipctx.denoise_moments(c["d_ns"], [(d_col, d_cov)], 1, prm, EPS)[0].cpu().numpy()
    st = hipctx.stats(0)
    assert st.similarity_path == 3 and st.borderline_pairs == 0 and st.processed > 0
    pixcov, s, cnt = hipctx.scale_begin(d_cov, c["d_ns"])
    mask, nsim = hipctx.similarity_masks_moments(d_col, pixcov, w, b, prm.hist_dist_threshold, EPS)
    state, _ = hipctx.active_set(mask, nsim, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, 0))
    hipctx.bayes_accumulate(d_col, pixcov, mask, nsim, state, w, b, prm.min_eigen_value, out=(s, cnt))
    want = hipctx.finalize(s, cnt)
    hipctx.synchronize()
    want = want.cpu().numpy()
    e = rel_linf(got, want)
    full = st.processed - st.fallback
    print("%s: frame call vs stage calls %.3e; %d processed, %d full estimates, sum |S| %d" % (kw, e, st.processed, full, st.similar_total))
    assert e <= TOL_SAME
    assert int((state == 1).sum()) == st.processed and int(nsim[state == 1].sum()) == st.similar_total
    if w == 1:
        assert full > 0 and st.fallback > 0                   # both branches of the estimate
    assert rel_linf(got, c["col"]) > 1e-3                    # something was denoised


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------
def test_three_scales_keep_the_selection_of_the_stage_calls(hipctx):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm, sel = c["prm"], c["sel"]
    w, b = prm.patch_radius, prm.search_radius
    info = sel.info()
    assert info["valid"] and (info["W"], info["H"], info["D"], info["nb_scales"]) == (W, H, 0, 3)
    assert [(s["width"], s["height"]) for s in info["scales"]] == [(90, 52), (45, 26), (22, 13)]
    assert all(s["similarity_path"] == 3 for s in info["scales"])
    assert [(s["processed"], s["fallback"], s["similar_total"], s["similarity_path"], 0) for s in info["scales"]] == c["stats"]
    d_col, d_cov = c["d_layers"][0]
    d_ns = c["d_ns"]
    for s in range(3):
        mask, nsim, state, _ = sel.read(s)
        want_mask, want_nsim = hipctx.similarity_masks_moments(d_col, hipctx.pixel_cov(d_cov, d_ns), w, b, prm.hist_dist_threshold, EPS)
        want_state, _ = hipctx.active_set(want_mask, want_nsim, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, s))
        hipctx.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want_mask.cpu().numpy()) and np.array_equal(nsim.cpu().numpy(), want_nsim.cpu().numpy()), s
        assert np.array_equal(state.cpu().numpy() == 1, want_state.cpu().numpy() == 1), s
        assert int((state == 1).sum()) == info["scales"][s]["processed"] > 0
        assert 0 < int(want_nsim.sum()) < want_nsim.numel() * (2 * b + 1) ** 2
        if s < 2:
            d_col, d_cov, d_ns = hipctx.downscale_avg(d_col), hipctx.downscale_cov(d_cov, d_ns), hipctx.downscale_sum(d_ns)
    for concurrent in (True, False):
        hipctx.set_concurrent_scales(concurrent)
        try:
            again = sel.denoise(c["d_layers"][:1])[0].cpu().numpy()
            serial = hipctx.denoise_moments(c["d_ns"], c["d_layers"][:1], 3, prm, EPS)[0].cpu().numpy()
        finally:
            hipctx.set_concurrent_scales(True)
        e, e2 = rel_linf(again, c["guide"]), rel_linf(serial, c["guide"])
        print("%s scales: the selection's denoise vs the call that kept it %.3e; the call again %.3e" % ("concurrent" if concurrent else "serial", e, e2))
        assert e <= TOL_SAME and e2 <= TOL_SAME
    assert [(s.processed, s.fallback, s.similar_total, s.similarity_path, s.borderline_pairs) for s in (hipctx.stats(k) for k in range(3))] == c["stats"]


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 16])
def test_layers_follow_the_guides_selection(hipctx, L):
    c = shared(hipctx)
    outs = [o.cpu().numpy() for o in hipctx.denoise_moments(c["d_ns"], c["d_layers"][:L], 3, c["prm"], EPS)]
    assert len(outs) == L
    for k in range(L):
        want = c["sel"].denoise([c["d_layers"][k]])[0].cpu().numpy()
        e = rel_linf(outs[k], want)
        print("%d layers, layer %d: vs the guide-only selection's denoise %.3e" % (L, k, e))
        assert e <= TOL_SAME
    assert rel_linf(outs[0], c["guide"]) <= TOL_SAME
    assert rel_linf(outs[1], outs[0]) > 1e-2                  # the layers differ


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_call_is_the_resident_call(hipctx):
    c = shared(hipctx)
    prm = c["prm"]
    layers = c["layers"][:3]
    resident = [o.cpu().numpy() for o in hipctx.denoise_moments(c["d_ns"], c["d_layers"][:3], 3, prm, EPS)]
    host = hipctx.denoise_moments_host(c["ns"], layers, 3, prm, EPS)
    for k in range(3):
        e = rel_linf(host[k], resident[k])
        print("host call, layer %d: vs the resident call %.3e" % (k, e))
        assert e <= TOL_SAME
    # a spike factor: bcd_hip_spike_filter_layers without histograms on the resident copies, then the resident call
    col = c["col"].copy()
    for l, k in ((10, 20), (30, 61), (44, 7)):
        col[l, k] += 25.0
    spiky = [(col, c["cov"])] + layers[1:]
    d_spiky = [tuple(dev(a, v)) for a, v in spiky]
    f_ns, f_hist, f_layers, _, moved = hipctx.spike_filter_layers(c["d_ns"], None, d_spiky, 2.0, count=True)
    assert f_hist is None and moved >= 3
    want = [o.cpu().numpy() for o in hipctx.denoise_moments(f_ns, f_layers, 3, prm, EPS)]
    got = hipctx.denoise_moments_host(c["ns"], spiky, 3, prm, EPS, spike_factor=2.0, filter_layers=True, zero_bad_values=True)
    unfiltered = hipctx.denoise_moments_host(c["ns"], spiky, 3, prm, EPS)
    for k in range(3):
        e = rel_linf(got[k], np.where(np.isfinite(want[k]) & (want[k] >= 0), want[k], 0))
        print("host call with the prefilter, layer %d: vs spike_filter_layers + the resident call %.3e" % (k, e))
        assert e <= TOL_SAME
    assert rel_linf(got[0], unfiltered[0]) > 1e-3             # the prefilter did something
    one = hipctx.denoise_moments_host(c["ns"], spiky[:1], 3, prm, EPS, spike_factor=2.0)          # one layer needs no switch
    assert rel_linf(one[0], want[0]) <= TOL_SAME


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(hipctx):
    import torch
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm = c["prm"]
    (d_col, d_cov), d_ns = c["d_layers"][0], c["d_ns"]
    out_a, out_b = torch.empty_like(d_col), torch.empty_like(d_col)
    L = bh.lib()
    EINVAL, EUNSUPPORTED = -1, -4

    def call(layers, n=None, ns=d_ns.data_ptr(), w_=W, h_=H, scales=3, p=prm, floor=EPS, sel=None, null_list=False):
        arr = (bh.Layer * max(1, len(layers)))()
        for k, (a, v, o) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_out = a, v, o
        rc = L.bcd_hip_denoise_moments(hipctx.h, ns, w_, h_, scales, C.byref(p) if p is not None else None, floor, None if null_list else arr,
                                       len(layers) if n is None else n, sel)
        return rc, L.bcd_hip_last_error(hipctx.h).decode()

    good = (d_col.data_ptr(), d_cov.data_ptr(), out_a.data_ptr())
    good_b = (d_col.data_ptr(), d_cov.data_ptr(), out_b.data_ptr())
    other_ctx = bh.Context(0)
    foreign = other_ctx.selection()
    try:
        cases = {
            "null sample counts": (call([good], ns=None), EINVAL, "null image pointer"),
            "null layer list": (call([good], null_list=True), EINVAL, "null layer list"),
            "no layer": (call([good], n=0), EINVAL, "between 1 and 16"),
            "too many layers": (call([good] * 17), EINVAL, "between 1 and 16"),
            "null colours": (call([(None, good[1], good[2])]), EINVAL, "null image pointer in a layer"),
            "null covariances": (call([good, (good[0], None, good_b[2])]), EINVAL, "null image pointer in a layer"),
            "null output": (call([good, (good[0], good[1], None)]), EINVAL, "null image pointer in a layer"),
            "null parameters": (call([good], p=None), EINVAL, "null parameters"),
            "empty image": (call([good], w_=0), EINVAL, "empty input image"),
            "image smaller than a patch": (call([good], w_=2, h_=2, scales=1), EINVAL, "smaller than a patch"),
            "negative radius": (call([good], p=bh.default_params(b=-1)), EINVAL, "negative radius"),
            "search radius 16": (call([good], p=bh.default_params(b=16)), EUNSUPPORTED, "search radius > 15"),
            "no scale": (call([good], scales=0), EINVAL, "bad number of scales"),
            "too many scales": (call([good], scales=6), EINVAL, "too many scales"),
            "bad pixel order": (call([good], p=bh.default_params(random_order=3)), EINVAL, "pixel order"),
            "two equal outputs": (call([good, good]), EINVAL, "share (part of) an output"),
            "overlapping outputs": (call([good, (good[0], good[1], good[2] + 12 * W)]), EINVAL, "share (part of) an output"),
            "output is an input": (call([good, (good[0], good[1], good[0])]), EINVAL, "overlaps an input image"),
            "output overlaps the sample counts": (call([(good[0], good[1], d_ns.data_ptr())]), EINVAL, "overlaps the sample counts"),
            "negative floor": (call([good], floor=-1e-8), EINVAL, "variance floor"),
            "NaN floor": (call([good], floor=float("nan")), EINVAL, "variance floor"),
            "infinite floor": (call([good], floor=float("inf")), EINVAL, "variance floor"),
            "a selection of another context": (call([good], sel=foreign.h), EINVAL, "another context"),
        }
        for name, ((rc, msg), want_rc, want) in cases.items():
            assert rc == want_rc and want in msg, (name, rc, msg)
        assert not foreign.info()["valid"]
        assert L.bcd_hip_denoise_moments(None, d_ns.data_ptr(), W, H, 1, C.byref(prm), EPS, (bh.Layer * 1)(), 1, None) == EINVAL
    finally:
        other_ctx.close()
    # the host call: its own refusals
    with pytest.raises(bh.BcdHipError, match="not available with several layers"):
        hipctx.denoise_moments_host(c["ns"], c["layers"][:2], 1, prm, EPS, spike_factor=2.0)
    with pytest.raises(bh.BcdHipError, match="variance floor"):
        hipctx.denoise_moments_host(c["ns"], c["layers"][:1], 1, prm, -1.0)
    # stage calls
    with pytest.raises(bh.BcdHipError, match="variance floor"):
        hipctx.similarity_masks_moments(d_col, d_cov, 1, 6, 1.0, float("nan"))
    with pytest.raises(bh.BcdHipError, match="not a main pixel"):
        hipctx.window_distances_moments(d_col, d_cov, 1, 6, 0, 5, EPS)
    # a kept selection that a refused call was handed is invalid, not half-filled
    victim = hipctx.selection()
    hipctx.denoise_moments(d_ns, [(d_col, d_cov)], 1, prm, EPS, keep=victim)
    assert victim.info()["valid"]
    assert call([good], scales=6, sel=victim.h)[0] == EINVAL and not victim.info()["valid"]
    victim.close()
    # ... and the context works
    got = hipctx.denoise_moments(d_ns, [(d_col, d_cov)], 3, prm, EPS, outs=[out_a])[0].cpu().numpy()
    assert rel_linf(got, c["guide"]) <= TOL_SAME


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_histogram_call_is_unchanged_by_a_moments_call(hipctx):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    col, ns, hist, cov = frame(96, 64, 16)
    d = dev(col, ns, hist, cov)
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    before = hipctx.denoise(*d, 3, prm).cpu().numpy()
    stats_before = [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))]
    hipctx.denoise_moments(c["d_ns"], c["d_layers"][:2], 3, c["prm"], EPS)
    assert all(hipctx.stats(k).similarity_path == 3 for k in range(3))
    after = hipctx.denoise(*d, 3, prm).cpu().numpy()
    e = rel_linf(after, before)
    print("bcd_hip_denoise before vs after a moments call: %.3e" % e)
    assert e <= TOL_SAME
    assert [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))] == stats_before
    assert all(p[3] != 3 for p in stats_before)
