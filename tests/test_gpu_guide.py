"""GPU tests of bcd_hip_denoise_guided: a frame whose similar-patch selection is gated by auxiliary feature buffers.
Frames are 90 x 52 (levels 45 x 26 and 22 x 13: widths of both parities), the seeded 8 spp frame of tests/test_gpu_layers.py with three noisy feature
channels and their variances split along another line than anything in the colours (tests/guide_cases.py).
  (1) one scale: the frame call is the composition scale_begin, similarity_masks_exact, similarity_masks_guide, gate_masks, active_set, bayes_accumulate,
      finalize;
  (2) three scales kept: per scale the kept masks and |S| are, bit for bit, the unguided kept selection's AND the stage call on levels built with
      downscale_avg (times 0.25 for the variances), the kept processed pixels are active_set's on them, the selection's own denoise reproduces the outputs
      with no features given;
  (3) 2 and 16 layers follow the gated selection;
  (4) the same without histograms: the moment selection with the gate;
  (5) the host call is the resident call;
  (6) effect, on noise-free features: no pair of main pixels whose patches lie wholly in different feature regions is similar, the unguided selection of
      the same frame has such pairs, and the outputs differ;
  (7) every refusal, followed by a successful call on the same context;
  (8) an unguided call of another frame and the unguided layered call of the guided frame give the same result before and after a guided call.
"The same" between two runs of the same build is the project's bar: 1e-5 relative L-inf, equal non-finite patterns (the float atomics of the aggregation
arrive in another order).  The stage calls alone, against the NumPy reference: tests/test_gpu_guide_stage.py."""
import ctypes as C

import numpy as np
import pytest

import guide_cases as gc
import guide_ref as gr
import moments_cases as mc
from test_gpu_layers import TOL_SAME, dev, frame, rel_linf

pytestmark = pytest.mark.gpu

W, H = 90, 52
NF = 3
EPS = 1e-6
_shared = {}


def shared(ctx):
    """the frame on the device, 16 layers of it, the features, and the three-scale calls with their kept selections, unguided and guided (once per session)"""
    import bcd_amd.hip as bh
    if not _shared:
        col, ns, hist, cov = frame(W, H, 8)
        layers = mc.layers_of(col, cov, 16)
        f, v, _ = gc.features(W, H, NF, seed=7)
        fl = gc.floors(NF, True)
        prm = bh.default_params(m=1.0, random_order=1, seed=21)
        d_ns, d_hist, d_f, d_v = dev(ns, hist, f, v)
        d_layers = [tuple(dev(c, x)) for c, x in layers]
        sel_u, sel_g = ctx.selection(), ctx.selection()
        plain = ctx.denoise_layers(d_ns, d_hist, d_layers[:1], 3, prm, keep=sel_u)[0].cpu().numpy()
        guided = ctx.denoise_guided(d_ns, d_hist, d_layers[:1], 3, prm, d_f, d_v, fl, 1.0, keep=sel_g)[0].cpu().numpy()
        stats = [ctx.stats(s) for s in range(3)]
        _shared.update(col=col, cov=cov, ns=ns, hist=hist, layers=layers, f=f, v=v, fl=fl, prm=prm, d_ns=d_ns, d_hist=d_hist, d_f=d_f, d_v=d_v, d_layers=d_layers,
                       sel_u=sel_u, sel_g=sel_g, plain=plain, guided=guided,
                       stats=[(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in stats])
    return _shared


def level_guides(ctx, d_f, d_v, n):
    """the feature pyramid by the stage calls: features averaged, variances averaged and multiplied by 0.25"""
    out = [(d_f, d_v)]
    for _ in range(1, n):
        f, v = out[-1]
        f2, v2 = ctx.downscale_avg(f), None if v is None else ctx.downscale_avg(v)
        ctx.synchronize()                                                             # (the context's stream is not torch's)
        out.append((f2, None if v2 is None else (v2 * 0.25).contiguous()))
        ctx.synchronize()
    return out


# ---- (1) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(m=1.0, random_order=1, seed=5), dict(m=0.0, random_order=0), dict(w=2, b=3, m=1.0, random_order=0, tau=1.5)])
def test_one_scale_is_the_composition_of_the_stage_calls(hipctx, kw):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm = bh.default_params(**kw)
    w, b = prm.patch_radius, prm.search_radius
    d_col, d_cov = c["d_layers"][0]
    got = hipctx.denoise_guided(c["d_ns"], c["d_hist"], [(d_col, d_cov)], 1, prm, c["d_f"], c["d_v"], c["fl"], 1.0)[0].cpu().numpy()
    st = hipctx.stats(0)
    assert st.processed > 0
    pixcov, s, cnt = hipctx.scale_begin(d_cov, c["d_ns"])
    mask, nsim = hipctx.similarity_masks_exact(c["d_hist"], c["d_ns"], w, b, prm.hist_dist_threshold)
    gate, ngate = hipctx.similarity_masks_guide(c["d_f"], c["d_v"], c["fl"], 1.0, w, b)
    hipctx.synchronize()
    before = int(nsim.sum())
    hipctx.gate_masks(mask, nsim, gate, b)
    state, _ = hipctx.active_set(mask, nsim, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, 0))
    hipctx.bayes_accumulate(d_col, pixcov, mask, nsim, state, w, b, prm.min_eigen_value, out=(s, cnt))
    want = hipctx.finalize(s, cnt)
    hipctx.synchronize()
    want = want.cpu().numpy()
    e = rel_linf(got, want)
    full = st.processed - st.fallback
    print("%s: frame call vs stage calls %.3e; %d processed, %d full estimates, sum |S| %d (ungated %d, feature masks %d)"
          % (kw, e, st.processed, full, st.similar_total, before, int(ngate.sum())))
    assert e <= TOL_SAME
    assert int((state == 1).sum()) == st.processed and int(nsim[state == 1].sum()) == st.similar_total
    assert 0 < int(nsim.sum()) < min(before, int(ngate.sum()))            # the gate removed pairs, and so did the selection
    if w == 1:
        assert full > 0 and st.fallback > 0                   # both branches of the estimate
    assert rel_linf(got, c["col"]) > 1e-3                    # something was denoised


# ---- (2) ------------------------------------------------------------------------------------------------------------------------------------------
def test_three_scales_keep_the_gated_selection(hipctx):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm, sel_u, sel_g = c["prm"], c["sel_u"], c["sel_g"]
    w, b = prm.patch_radius, prm.search_radius
    info = sel_g.info()
    assert info["valid"] and (info["W"], info["H"], info["nb_scales"]) == (W, H, 3) and info["D"] == c["hist"].shape[2]
    assert [(s["width"], s["height"]) for s in info["scales"]] == [(90, 52), (45, 26), (22, 13)]
    assert [(s["processed"], s["fallback"], s["similar_total"], s["similarity_path"]) for s in info["scales"]] == c["stats"]
    guides = level_guides(hipctx, c["d_f"], c["d_v"], 3)
    for s in range(3):
        mask, nsim, state, _ = sel_g.read(s)
        mask_u, nsim_u, _, _ = sel_u.read(s)
        gate, _ = hipctx.similarity_masks_guide(guides[s][0], guides[s][1], c["fl"], 1.0, w, b)
        hipctx.synchronize()
        want_mask, want_nsim = gr.gate(mask_u.cpu().numpy(), gate.cpu().numpy())
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(nsim.cpu().numpy(), want_nsim), s
        import torch
        d_want_mask, d_want_nsim = torch.from_numpy(want_mask).cuda(), torch.from_numpy(want_nsim).cuda()
        want_state, _ = hipctx.active_set(d_want_mask, d_want_nsim, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, s))
        hipctx.synchronize()
        assert np.array_equal(state.cpu().numpy() == 1, want_state.cpu().numpy() == 1), s
        assert int((state == 1).sum()) == info["scales"][s]["processed"] > 0
        assert 0 < int(want_nsim.sum()) < int(nsim_u.sum())                         # the gate removed pairs at every level
    # the feature pyramid of the reference (tests/guide_ref.py) is what the stage calls built
    ref = gr.pyramid(c["f"], c["v"], 3)
    for s in range(3):
        assert np.array_equal(guides[s][0].cpu().numpy(), ref[s][0]) and np.array_equal(guides[s][1].cpu().numpy(), ref[s][1]), s
    for concurrent in (True, False):
        hipctx.set_concurrent_scales(concurrent)
        try:
            again = sel_g.denoise(c["d_layers"][:1])[0].cpu().numpy()               # no features given
            serial = hipctx.denoise_guided(c["d_ns"], c["d_hist"], c["d_layers"][:1], 3, prm, c["d_f"], c["d_v"], c["fl"], 1.0)[0].cpu().numpy()
        finally:
            hipctx.set_concurrent_scales(True)
        e, e2 = rel_linf(again, c["guided"]), rel_linf(serial, c["guided"])
        print("%s scales: the selection's denoise vs the call that kept it %.3e; the call again %.3e" % ("concurrent" if concurrent else "serial", e, e2))
        assert e <= TOL_SAME and e2 <= TOL_SAME
    assert [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))] == c["stats"]
    assert rel_linf(c["guided"], c["plain"]) > 1e-3                                  # the gate changed the result


# ---- (3) ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 16])
def test_layers_follow_the_gated_selection(hipctx, L):
    c = shared(hipctx)
    outs = [o.cpu().numpy() for o in hipctx.denoise_guided(c["d_ns"], c["d_hist"], c["d_layers"][:L], 3, c["prm"], c["d_f"], c["d_v"], c["fl"], 1.0)]
    assert len(outs) == L
    for k in range(L):
        want = c["sel_g"].denoise([c["d_layers"][k]])[0].cpu().numpy()
        e = rel_linf(outs[k], want)
        print("%d layers, layer %d: vs the gated selection's denoise %.3e" % (L, k, e))
        assert e <= TOL_SAME
    assert rel_linf(outs[0], c["guided"]) <= TOL_SAME
    assert rel_linf(outs[1], outs[0]) > 1e-2                  # the layers differ


# ---- (4) ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_moment_selection_is_gated_the_same_way(hipctx):
    import torch
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm = c["prm"]
    w, b = prm.patch_radius, prm.search_radius
    sel_m, sel_mg = hipctx.selection(), hipctx.selection()
    try:
        hipctx.denoise_moments(c["d_ns"], c["d_layers"][:1], 3, prm, EPS, keep=sel_m)
        outs = [o.cpu().numpy() for o in hipctx.denoise_guided(c["d_ns"], None, c["d_layers"][:2], 3, prm, c["d_f"], c["d_v"], c["fl"], 1.0, var_floor=EPS, keep=sel_mg)]
        assert all(hipctx.stats(k).similarity_path == 3 for k in range(3))
        info = sel_mg.info()
        assert info["valid"] and info["D"] == 0 and all(s["similarity_path"] == 3 for s in info["scales"])
        guides = level_guides(hipctx, c["d_f"], c["d_v"], 3)
        for s in range(3):
            mask, nsim, state, _ = sel_mg.read(s)
            mask_u, nsim_u, _, _ = sel_m.read(s)
            gate, _ = hipctx.similarity_masks_guide(guides[s][0], guides[s][1], c["fl"], 1.0, w, b)
            hipctx.synchronize()
            want_mask, want_nsim = gr.gate(mask_u.cpu().numpy(), gate.cpu().numpy())
            assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(nsim.cpu().numpy(), want_nsim), s
            want_state, _ = hipctx.active_set(torch.from_numpy(want_mask).cuda(), torch.from_numpy(want_nsim).cuda(), w, b, prm.marked_skip_probability,
                                              prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, s))
            hipctx.synchronize()
            assert np.array_equal(state.cpu().numpy() == 1, want_state.cpu().numpy() == 1), s
            assert 0 < int(want_nsim.sum()) < int(nsim_u.sum())
        for k in range(2):
            want = sel_mg.denoise([c["d_layers"][k]])[0].cpu().numpy()
            e = rel_linf(outs[k], want)
            print("moment selection with the gate, layer %d: vs the kept selection's denoise %.3e" % (k, e))
            assert e <= TOL_SAME
    finally:
        sel_m.close()
        sel_mg.close()


# ---- (5) ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_call_is_the_resident_call(hipctx):
    c = shared(hipctx)
    prm = c["prm"]
    layers = c["layers"][:3]
    resident = [o.cpu().numpy() for o in hipctx.denoise_guided(c["d_ns"], c["d_hist"], c["d_layers"][:3], 3, prm, c["d_f"], c["d_v"], c["fl"], 1.0)]
    host = hipctx.denoise_guided_host(c["ns"], c["hist"], layers, 3, prm, c["f"], c["v"], c["fl"], 1.0)
    for k in range(3):
        e = rel_linf(host[k], resident[k])
        print("host call, layer %d: vs the resident call %.3e" % (k, e))
        assert e <= TOL_SAME
    # without variances and without histograms
    fl = gc.floors(NF, False)
    resident = [o.cpu().numpy() for o in hipctx.denoise_guided(c["d_ns"], None, c["d_layers"][:2], 3, prm, c["d_f"], None, fl, 1.0, var_floor=EPS)]
    host = hipctx.denoise_guided_host(c["ns"], None, layers[:2], 3, prm, c["f"], None, fl, 1.0, var_floor=EPS, zero_bad_values=True)
    for k in range(2):
        want = np.where(np.isfinite(resident[k]) & (resident[k] >= 0), resident[k], 0)
        e = rel_linf(host[k], want)
        print("host call without histograms and variances, layer %d: vs the resident call %.3e" % (k, e))
        assert e <= TOL_SAME
    assert rel_linf(host[0], hipctx.denoise_moments_host(c["ns"], layers[:1], 3, prm, EPS)[0]) > 1e-3       # the gate did something there too


# ---- (6) ------------------------------------------------------------------------------------------------------------------------------------------
def test_no_patch_is_averaged_across_a_feature_edge(hipctx):
    """noise-free features, floors 0.01: whole-patch distances across the edge are >= 2 by construction (tests/test_guide_cases_cpu.py), tau_g = 1"""
    c = shared(hipctx)
    prm = c["prm"]
    w, b = prm.patch_radius, prm.search_radius
    f, _, _ = gc.features(W, H, NF, seed=7, sigma=0.0)
    d_f, = dev(f)
    fl = gc.floors(NF, False)
    sel = hipctx.selection()
    try:
        got = hipctx.denoise_guided(c["d_ns"], c["d_hist"], c["d_layers"][:1], 1, prm, d_f, None, fl, 1.0, keep=sel)[0].cpu().numpy()
        mask = sel.read(0)[0].cpu().numpy()
    finally:
        sel.close()
    sel = hipctx.selection()
    try:
        plain = hipctx.denoise_layers(c["d_ns"], c["d_hist"], c["d_layers"][:1], 1, prm, keep=sel)[0].cpu().numpy()
        mask_u = sel.read(0)[0].cpu().numpy()
    finally:
        sel.close()
    across = gc.across_pairs(W, H, w, b)
    n_u, n_g = int((gc.mask_bits(mask_u, b) & across).sum()), int((gc.mask_bits(mask, b) & across).sum())
    e = rel_linf(got, plain)
    print("pairs of patches wholly in different feature regions: %d similar unguided, %d guided; outputs differ by %.3e" % (n_u, n_g, e))
    assert n_u > 0                                            # precondition: the radiance statistics do not see the edge
    assert n_g == 0
    assert e > 1e-3


# ---- (7) ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(hipctx):
    import torch
    import bcd_amd.hip as bh
    c = shared(hipctx)
    prm = c["prm"]
    (d_col, d_cov), d_ns, d_hist, d_f, d_v = c["d_layers"][0], c["d_ns"], c["d_hist"], c["d_f"], c["d_v"]
    D = c["hist"].shape[2]
    out_a, out_b = torch.empty_like(d_col), torch.empty_like(d_col)
    L = bh.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    good_floors = (C.c_float * 8)(*([1e-4] * 8))

    def guide(features=d_f.data_ptr(), variances=d_v.data_ptr(), n=NF, floors=good_floors, threshold=1.0):
        fl = (C.c_float * 8)(*floors) if not isinstance(floors, C.Array) and floors is not None else floors
        return bh.Guide(features, variances, n, C.cast(fl, C.POINTER(C.c_float)) if fl is not None else None, threshold)

    def call(layers, g=None, n=None, ns=d_ns.data_ptr(), hist=d_hist.data_ptr(), w_=W, h_=H, scales=3, p=prm, floor=EPS, sel=None, null_guide=False):
        arr = (bh.Layer * max(1, len(layers)))()
        for k, (a, v, o) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_out = a, v, o
        g = guide() if g is None else g
        rc = L.bcd_hip_denoise_guided(hipctx.h, ns, hist, w_, h_, D, scales, C.byref(p) if p is not None else None, floor, arr, len(layers) if n is None else n,
                                      None if null_guide else C.byref(g), sel)
        return rc, L.bcd_hip_last_error(hipctx.h).decode()

    good = (d_col.data_ptr(), d_cov.data_ptr(), out_a.data_ptr())
    other_ctx = bh.Context(0)
    foreign = other_ctx.selection()
    nan, inf = float("nan"), float("inf")
    try:
        cases = {
            # what the underlying calls refuse
            "null sample counts": (call([good], ns=None), EINVAL, "null image pointer"),
            "no layer": (call([good], n=0), EINVAL, "between 1 and 16"),
            "too many layers": (call([good] * 17), EINVAL, "between 1 and 16"),
            "null colours": (call([(None, good[1], good[2])]), EINVAL, "null image pointer in a layer"),
            "null parameters": (call([good], p=None), EINVAL, "null parameters"),
            "empty image": (call([good], w_=0), EINVAL, "empty input image"),
            "search radius 16": (call([good], p=bh.default_params(b=16)), EUNSUPPORTED, "search radius > 15"),
            "too many scales": (call([good], scales=6), EINVAL, "too many scales"),
            "two equal outputs": (call([good, good]), EINVAL, "share (part of) an output"),
            "negative variance floor without histograms": (call([good], hist=None, floor=-1.0), EINVAL, "variance floor"),
            "NaN variance floor without histograms": (call([good], hist=None, floor=nan), EINVAL, "variance floor"),
            # the guide's own
            "null guide": (call([good], null_guide=True), EINVAL, "null guide"),
            "no channel": (call([good], guide(n=0)), EINVAL, "between 1 and 8"),
            "nine channels": (call([good], guide(n=9)), EINVAL, "between 1 and 8"),
            "null features": (call([good], guide(features=None)), EINVAL, "null feature image"),
            "null floors": (call([good], guide(floors=None)), EINVAL, "null feature floors"),
            "negative floor": (call([good], guide(floors=[1e-4, -1e-8, 1e-4] + [0] * 5)), EINVAL, "feature floor"),
            "NaN floor": (call([good], guide(floors=[nan] + [1e-4] * 7)), EINVAL, "feature floor"),
            "infinite floor": (call([good], guide(floors=[1e-4, 1e-4, inf] + [0] * 5)), EINVAL, "feature floor"),
            "negative threshold": (call([good], guide(threshold=-0.5)), EINVAL, "feature threshold"),
            "NaN threshold": (call([good], guide(threshold=nan)), EINVAL, "feature threshold"),
            "infinite threshold": (call([good], guide(threshold=inf)), EINVAL, "feature threshold"),
            "no channel can count": (call([good], guide(variances=None, floors=[0.0] * 8)), EINVAL, "no feature channel can count"),
            "a selection of another context": (call([good], sel=foreign.h), EINVAL, "another context"),
        }
        for name, ((rc, msg), want_rc, want) in cases.items():
            assert rc == want_rc and want in msg, (name, rc, msg)
        assert not foreign.info()["valid"]
        assert L.bcd_hip_denoise_guided(None, d_ns.data_ptr(), d_hist.data_ptr(), W, H, D, 1, C.byref(prm), EPS, (bh.Layer * 1)(), 1, C.byref(guide()), None) == EINVAL
        # a floor beyond the channels in use is not looked at; zero floors are fine beside variances
        assert call([good], guide(floors=[0.0, 0.0, 0.0, -1.0, nan, inf, -1.0, -1.0]))[0] == 0
    finally:
        other_ctx.close()
    # the stage calls and the host call
    with pytest.raises(bh.BcdHipError, match="feature floor"):
        hipctx.similarity_masks_guide(d_f, d_v, [1e-4, -1.0, 1e-4], 1.0, 1, 6)
    with pytest.raises(bh.BcdHipError, match="no feature channel can count"):
        hipctx.similarity_masks_guide(d_f, None, [0.0, 0.0, 0.0], 1.0, 1, 6)
    with pytest.raises(bh.BcdHipError, match="search radius > 15"):
        hipctx.similarity_masks_guide(d_f, d_v, c["fl"], 1.0, 1, 16)
    with pytest.raises(bh.BcdHipError, match="not a main pixel"):
        hipctx.window_distances_guide(d_f, d_v, c["fl"], 1, 6, 0, 5)
    with pytest.raises(bh.BcdHipError, match="feature threshold"):
        hipctx.denoise_guided_host(c["ns"], c["hist"], c["layers"][:1], 1, prm, c["f"], c["v"], c["fl"], -1.0)
    with pytest.raises(bh.BcdHipError, match="not available with several layers"):
        hipctx.denoise_guided_host(c["ns"], c["hist"], c["layers"][:2], 1, prm, c["f"], c["v"], c["fl"], 1.0, spike_factor=2.0)
    with pytest.raises(bh.BcdHipError, match="too many scales"):
        hipctx.denoise_guided_host(c["ns"], None, c["layers"][:1], 6, prm, c["f"], c["v"], c["fl"], 1.0)
    # a kept selection that a refused call was handed is invalid, not half-filled
    victim = hipctx.selection()
    hipctx.denoise_guided(d_ns, d_hist, [(d_col, d_cov)], 1, prm, d_f, d_v, c["fl"], 1.0, keep=victim)
    assert victim.info()["valid"]
    assert call([good], guide(n=9), sel=victim.h)[0] == EINVAL and not victim.info()["valid"]
    victim.close()
    # ... and the context works
    got = hipctx.denoise_guided(d_ns, d_hist, [(d_col, d_cov)], 3, prm, d_f, d_v, c["fl"], 1.0, outs=[out_b])[0].cpu().numpy()
    assert rel_linf(got, c["guided"]) <= TOL_SAME


# ---- (8) ------------------------------------------------------------------------------------------------------------------------------------------
def test_unguided_calls_are_unchanged_by_a_guided_call(hipctx):
    import bcd_amd.hip as bh
    c = shared(hipctx)
    col, ns, hist, cov = frame(96, 64, 16)
    d = dev(col, ns, hist, cov)
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    before = hipctx.denoise(*d, 3, prm).cpu().numpy()
    stats_before = [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))]
    layered_before = [o.cpu().numpy() for o in hipctx.denoise_layers(c["d_ns"], c["d_hist"], c["d_layers"][:2], 3, c["prm"])]
    layered_stats = [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))]
    hipctx.denoise_guided(c["d_ns"], c["d_hist"], c["d_layers"][:2], 3, c["prm"], c["d_f"], c["d_v"], c["fl"], 1.0)
    guided_stats = [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))]
    assert guided_stats == c["stats"] and guided_stats != layered_stats
    after = hipctx.denoise(*d, 3, prm).cpu().numpy()
    e = rel_linf(after, before)
    print("bcd_hip_denoise before vs after a guided call: %.3e" % e)
    assert e <= TOL_SAME
    assert [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))] == stats_before
    layered_after = [o.cpu().numpy() for o in hipctx.denoise_layers(c["d_ns"], c["d_hist"], c["d_layers"][:2], 3, c["prm"])]
    for k in range(2):
        e = rel_linf(layered_after[k], layered_before[k])
        print("bcd_hip_denoise_layers of the guided frame before vs after, layer %d: %.3e" % (k, e))
        assert e <= TOL_SAME
    assert [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(3))] == layered_stats
    assert rel_linf(layered_after[0], c["plain"]) <= TOL_SAME
