"""GPU tests of a frame's kept selection (bcd_hip_selection_*, bcd_hip_denoise_layers_keep) and of the moments-only snapshot of the
accumulator (bcd_hip_accum_moments).
  * _keep is bcd_hip_denoise_layers: per layer <= 1e-5 (same build, other order of the float atomics), same statistics, same per-layer spectral counts;
  * what it keeps is the selection of the stage calls on that pyramid level's inputs (masks, |S| and the count image array_equal);
  * the estimate stage on the kept selection returns the kept call's layers (4, 1 and 16 layers; concurrent and serial scales), returns layers the kept
    call never saw as the plain call on them does, survives other work on the context, and with other sample counts is what the stage calls compose;
  * it launches no distance kernel, and every refusal leaves the selection as it was.
The frames: the seven configurations of test_layers_match_the_oracle_and_the_plain_call plus two whose full-estimate / fallback counts per scale were
found with the CPU oracle (asserted through Selection.info()), so that both kinds of item occur on a fine and on a coarse level, and one with 5 x 5
patches at a threshold of 2 (10 full estimates, found the same way: the w2 configuration has none, so the list kernels' full-estimate path would go unvisited),
and one at -e 1e-3 whose full estimates take the deferred redo pass in every layer (the count image is complete only after it)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_layers import TOL, TOL_SAME, dev, frame, mixed_counts_frame, orders, rel_linf, split_layers, stats_tuple

pytestmark = pytest.mark.gpu

# name -> (inputs, scales, layers, parameters, (full estimates, fallback pixels) per scale or None)
CONFIGS = {
    "96x64_s3_m1_r1": (lambda: frame(96, 64, 16), 3, 4, dict(m=1.0, random_order=1, seed=11), None),
    "72x50_s1_m1_r0": (lambda: frame(72, 50, 16), 1, 4, dict(m=1.0, random_order=0, seed=5), None),
    "m0": (lambda: frame(61, 45, 16), 2, 4, dict(m=0.0, random_order=0), None),
    "b3": (lambda: frame(66, 50, 8), 2, 3, dict(b=3, m=1.0, random_order=1, seed=3), None),
    "b12": (lambda: frame(45, 41, 8), 1, 3, dict(b=12, m=1.0, random_order=1, seed=3), None),
    "w2": (lambda: frame(44, 36, 8), 1, 3, dict(w=2, b=4, m=1.0, random_order=1, seed=3), None),
    "mixed_counts": (lambda: mixed_counts_frame(96, 72), 2, 4, dict(m=1.0, random_order=0, seed=5), None),
    "w2_tau2": (lambda: frame(44, 36, 8), 1, 3, dict(w=2, b=4, tau=2.0, m=1.0, random_order=1, seed=3), [(10, 646)]),    # (w2 has no full estimate)
    "redo_e1e-3": (lambda: frame(64, 48, 32, 0.08, 0.0), 1, 3, dict(m=0.0, min_eig=1e-3), None),      # full estimates that take the deferred redo pass
    "noisy_m1": (lambda: frame(96, 64, 16, sigma=0.35), 3, 4, dict(m=1.0, random_order=0), [(192, 991), (15, 1088), (0, 308)]),
    "spp4_m0": (lambda: frame(96, 64, 4), 3, 4, dict(m=0.0, random_order=0), [(5825, 3), (211, 1169)]),
}
NAMES = list(CONFIGS)
_cases = {}


def spectral_counts(ctx, S, L):
    return [[ctx.layer_spectral_inverses(s, k) for k in range(L)] for s in range(S)]


def case(ctx, name):
    """the frame of a configuration on the device, its plain layered call and its _keep call (once per session): dict"""
    import bcd_amd.hip as bh
    if name not in _cases:
        make, S, L, kw, counts = CONFIGS[name]
        col, ns, hist, cov = make()
        prm = bh.default_params(**kw)
        layers = split_layers(col, cov, L)
        d_ns, d_hist = dev(ns, hist)
        d_layers = [tuple(dev(c, v)) for c, v in layers]
        plain = [o.cpu().numpy() for o in ctx.denoise_layers(d_ns, d_hist, d_layers, S, prm)]
        plain_stats, plain_spectral = stats_tuple(ctx, S), spectral_counts(ctx, S, L)
        sel = ctx.selection()
        kept = [o.cpu().numpy() for o in ctx.denoise_layers(d_ns, d_hist, d_layers, S, prm, keep=sel)]
        _cases[name] = dict(S=S, L=L, kw=kw, prm=prm, host=(col, ns, hist, cov), layers=layers, d_ns=d_ns, d_hist=d_hist, d_layers=d_layers, plain=plain,
                            plain_stats=plain_stats, plain_spectral=plain_spectral, sel=sel, kept=kept, kept_stats=stats_tuple(ctx, S),
                            kept_spectral=spectral_counts(ctx, S, L), counts=counts)
    return _cases[name]


def serial_default():
    return os.environ.get("BCD_HIP_SERIAL_SCALES", "")[:1] == "1"


# ---- 1. _keep is the layered call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_keep_is_the_layered_call(hipctx, name):
    c = case(hipctx, name)
    for k in range(c["L"]):
        e = rel_linf(c["kept"][k], c["plain"][k])
        print("%s layer %d: _keep vs denoise_layers %.3e" % (name, k, e))
        assert e <= TOL_SAME
    assert c["kept_stats"] == c["plain_stats"] and c["kept_spectral"] == c["plain_spectral"]
    if name == "redo_e1e-3":                                    # the redo pass adds to the count image after the scale's first synchronisation
        assert all(n > 0 for n in c["kept_spectral"][0]), c["kept_spectral"]
    info = c["sel"].info()
    H, W, D = c["host"][2].shape
    assert info["valid"] and (info["W"], info["H"], info["D"], info["nb_scales"]) == (W, H, D, c["S"])
    p, q = info["params"], c["prm"]
    assert all(getattr(p, f) == getattr(q, f) for f, _ in p._fields_)
    assert [(s["processed"], s["fallback"], s["similar_total"], s["similarity_path"]) for s in info["scales"]] == c["kept_stats"]
    assert [(s["width"], s["height"]) for s in info["scales"]] == [(W >> s, H >> s) for s in range(c["S"])]
    words = ((2 * q.search_radius + 1) ** 2 + 31) // 32
    need = sum((W >> s) * (H >> s) * (4 * words + 17) for s in range(c["S"]))     # mask words, |S|, state, one list, count image, sample counts
    print("%s: %d device bytes held, %.1f per pixel of the frame" % (name, info["device_bytes"], info["device_bytes"] / (W * H)))
    assert need <= info["device_bytes"] <= need * 1.07 + 8 * 600 * c["S"]          # (grow-only buffers carry 1/16 of slack)
    if c["counts"]:
        got = [(s["processed"] - s["fallback"], s["fallback"]) for s in info["scales"]]
        assert got[:len(c["counts"])] == c["counts"], got
        for s in range(min(2, c["S"])):                                             # both branches of the estimate on a fine and on a coarse level
            assert got[s][0] > 0 and got[s][1] > 0


# ---- 2. what is kept ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_kept_selection_is_that_of_the_stage_calls(hipctx, name):
    import bcd_amd.hip as bh
    c = case(hipctx, name)
    prm, kw = c["prm"], c["kw"]
    w, b = prm.patch_radius, prm.search_radius
    d_col, d_cov = c["d_layers"][0]
    d_ns, d_hist = c["d_ns"], c["d_hist"]
    for s in range(c["S"]):
        mask, nsim, state, count = c["sel"].read(s)
        want_mask, want_nsim = hipctx.similarity_masks(d_hist, d_ns, w, b, prm.hist_dist_threshold)
        assert np.array_equal(mask.cpu().numpy(), want_mask.cpu().numpy()) and np.array_equal(nsim.cpu().numpy(), want_nsim.cpu().numpy()), (name, s)
        st, _ = hipctx.active_set(want_mask, want_nsim, w, b, prm.marked_skip_probability, prm.use_random_pixel_order, bh.scale_seed(prm.order_seed, s))
        _, want_count = hipctx.bayes_accumulate(d_col, hipctx.pixel_cov(d_cov, d_ns), want_mask, want_nsim, st, w, b, prm.min_eigen_value)
        hipctx.synchronize()
        assert np.array_equal(count.cpu().numpy(), want_count.cpu().numpy()), (name, s)
        assert np.array_equal(state.cpu().numpy() == 1, st.cpu().numpy() == 1), (name, s)      # the processed pixels
        info = c["sel"].info()["scales"][s]
        assert int((state == 1).sum()) == info["processed"]
        if s + 1 < c["S"]:
            d_col, d_cov, d_hist, d_ns = hipctx.downscale_avg(d_col), hipctx.downscale_cov(d_cov, d_ns), hipctx.downscale_sum(d_hist), hipctx.downscale_sum(d_ns)


# ---- 3. reuse with the same layers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concurrent", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_reuse_returns_the_kept_layers(hipctx, name, concurrent):
    c = case(hipctx, name)
    S, L = c["S"], c["L"]
    hipctx.set_concurrent_scales(concurrent)
    try:
        for n in (L, 1, 16):
            picks = [k % L for k in range(n)]
            outs = c["sel"].denoise([c["d_layers"][k] for k in picks])
            assert len(outs) == n
            for i, k in enumerate(picks):
                e = rel_linf(outs[i].cpu().numpy(), c["kept"][k])
                if i < L:
                    print("%s %s, %d layers, layer %d: reuse vs _keep %.3e" % (name, "concurrent" if concurrent else "serial", n, i, e))
                assert e <= TOL_SAME, (n, i)
            st = stats_tuple(hipctx, S)
            assert st == c["kept_stats"]
            per_layer = spectral_counts(hipctx, S, n)
            assert [sum(p) for p in per_layer] == [hipctx.stats(s).spectral_inverses for s in range(S)]
            assert [[p[i] for i in range(min(n, L))] for p in per_layer] == [p[:min(n, L)] for p in c["kept_spectral"]]
            assert all(hipctx.stats(s).ms_similarity == 0 and hipctx.stats(s).ms_active == 0 for s in range(S))
    finally:
        hipctx.set_concurrent_scales(not serial_default())


# ---- 4. layers the kept call never saw ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96x64_s3_m1_r1", "noisy_m1", "w2", "w2_tau2"])
def test_layers_that_arrive_later(hipctx, name):
    c = case(hipctx, name)
    S, L, kw = c["S"], c["L"], c["kw"]
    col, ns, hist, cov = c["host"]
    sel = hipctx.selection()
    try:
        hipctx.denoise_layers(c["d_ns"], c["d_hist"], c["d_layers"][:1], S, c["prm"], keep=sel)
        outs = [o.cpu().numpy() for o in sel.denoise(c["d_layers"][1:])]
        H, W, _ = hist.shape
        od = orders(W, H, kw.get("w", 1), kw.get("random_order", 1), kw.get("seed", 1234), S) if kw["m"] != 0.0 else None
        for i, k in enumerate(range(1, L)):
            single = hipctx.denoise(c["d_layers"][k][0], c["d_ns"], c["d_hist"], c["d_layers"][k][1], S, c["prm"]).cpu().numpy()
            e = rel_linf(outs[i], single)
            print("%s layer %d, kept with layer 0 only: vs plain call %.3e" % (name, k, e))
            assert e <= TOL_SAME
            if name == "96x64_s3_m1_r1":
                want = ol.denoise_multiscale(c["layers"][k][0], ns, hist, c["layers"][k][1], S, ol.params(m=kw["m"]), orders=od)
                e = rel_linf(outs[i], want)
                print("   vs oracle %.3e" % e)
                assert e < TOL
    finally:
        sel.close()


# ---- 5. the selection is the selection's ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy_m1", "spp4_m0", "w2", "w2_tau2"])
def test_the_selection_survives_other_work_on_the_context(hipctx, name):
    import bcd_amd.hip as bh
    c = case(hipctx, name)
    other = case(hipctx, "72x50_s1_m1_r0")                      # another size, other list lengths, on the same workspaces
    hipctx.denoise(other["d_layers"][0][0], other["d_ns"], other["d_hist"], other["d_layers"][0][1], 1, other["prm"])
    assert hipctx.stats(0).processed != c["kept_stats"][0][0]
    outs = c["sel"].denoise(c["d_layers"])
    for k in range(c["L"]):
        e = rel_linf(outs[k].cpu().numpy(), c["kept"][k])
        print("%s layer %d after a plain call of another size: %.3e" % (name, k, e))
        assert e <= TOL_SAME
    assert stats_tuple(hipctx, c["S"]) == c["kept_stats"]
    hipctx.denoise_layers(other["d_ns"], other["d_hist"], other["d_layers"], 2, bh.default_params(m=0.0))   # every workspace buffer of two scales rewritten
    outs = c["sel"].denoise(c["d_layers"])
    for k in range(c["L"]):
        assert rel_linf(outs[k].cpu().numpy(), c["kept"][k]) <= TOL_SAME


# ---- 6. other sample counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["72x50_s1_m1_r0", "w2", "w2_tau2"])
def test_other_sample_counts_replace_the_kept_ones_in_the_estimate(hipctx, name):
    c = case(hipctx, name)
    assert c["S"] == 1
    prm = c["prm"]
    full_estimates = c["kept_stats"][0][0] - c["kept_stats"][0][1]
    ns_b = c["host"][1].copy()
    ns_b[8:30, 10:40] *= 2.0
    d_ns_b, = dev(ns_b)
    outs = [o.cpu().numpy() for o in c["sel"].denoise(c["d_layers"], ns=d_ns_b)]
    mask, nsim, state, count = c["sel"].read(0)
    pc, _ = hipctx.layers_pixel_cov([v for _, v in c["d_layers"]], d_ns_b)
    sums, cnt, _ = hipctx.bayes_accumulate_layers([(col, pc[k]) for k, (col, _) in enumerate(c["d_layers"])], mask, nsim, state, prm.patch_radius, prm.search_radius,
                                                  prm.min_eigen_value)
    want = [o.cpu().numpy() for o in hipctx.layers_finalize(sums, count)]
    assert np.array_equal(cnt.cpu().numpy(), count.cpu().numpy())
    for k in range(c["L"]):
        e = rel_linf(outs[k], want[k])
        moved = rel_linf(outs[k], c["kept"][k])
        print("%s layer %d with a block of doubled counts: vs the stage calls %.3e; moved from the kept counts' result by %.3e" % (name, k, e, moved))
        assert e <= TOL_SAME
        if full_estimates > 0:                                  # (fallback pixels average colours: no covariance, no count)
            assert moved > 100 * TOL_SAME                       # the passed counts are read
        else:
            assert moved <= TOL_SAME
    assert stats_tuple(hipctx, 1) == c["kept_stats"]            # the selection stays the kept one


def test_other_sample_counts_through_the_pyramid(hipctx):
    """three scales: the kept counts passed explicitly go through the sample-count pyramid of the reuse call and give what NULL gives; doubled counts
    everywhere halve every covariance / n at every level, which is not what the kept counts give"""
    c = case(hipctx, "noisy_m1")
    base = [o.cpu().numpy() for o in c["sel"].denoise(c["d_layers"])]
    explicit = [o.cpu().numpy() for o in c["sel"].denoise(c["d_layers"], ns=c["d_ns"])]
    d_twice, = dev(c["host"][1] * 2.0)
    twice = [o.cpu().numpy() for o in c["sel"].denoise(c["d_layers"], ns=d_twice)]
    for k in range(c["L"]):
        e = rel_linf(explicit[k], base[k])
        print("layer %d: kept counts passed explicitly vs NULL %.3e; doubled counts %.3e" % (k, e, rel_linf(twice[k], base[k])))
        assert e <= TOL_SAME
        assert rel_linf(twice[k], base[k]) > 100 * TOL_SAME
    assert stats_tuple(hipctx, 3) == c["kept_stats"]


# ---- 7. no selection work -------------------------------------------------------------------------------------------------------------------------
def test_a_reuse_call_launches_no_distance_kernel(hipctx):
    c = case(hipctx, "noisy_m1")
    sel = hipctx.selection()
    hipctx.set_profiling(True)
    try:
        hipctx.reset_kernel_time()
        hipctx.denoise_layers(c["d_ns"], c["d_hist"], c["d_layers"], c["S"], c["prm"], keep=sel)
        assert hipctx.kernel_time()[1] >= c["S"]                # (the counter sees the distance kernels of a frame)
        assert all(hipctx.stats(s).ms_similarity > 0 for s in range(c["S"]))
        hipctx.reset_kernel_time()
        outs = sel.denoise(c["d_layers"])
        assert hipctx.kernel_time()[1] == 0
        assert all(hipctx.stats(s).ms_similarity == 0 and hipctx.stats(s).ms_active == 0 for s in range(c["S"]))
        for k in range(c["L"]):
            assert rel_linf(outs[k].cpu().numpy(), c["kept"][k]) <= TOL_SAME
    finally:
        hipctx.set_profiling(False)
        sel.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_are_refused_and_leave_the_selection_alone(hipctx):
    import torch
    import bcd_amd.hip as bh
    c = case(hipctx, "72x50_s1_m1_r0")
    sel = c["sel"]
    (d_col, d_cov), d_ns, d_hist, prm = c["d_layers"][0], c["d_ns"], c["d_hist"], c["prm"]
    H, W, D = c["host"][2].shape
    out_a, out_b = torch.empty_like(d_col), torch.empty_like(d_col)
    L = bh.lib()
    EINVAL = -1

    def reuse(layers, n=None, handle=sel.h, ns_ptr=None, null_list=False):
        arr = (bh.Layer * max(1, len(layers)))()
        for k, (a, v, o) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_out = a, v, o
        rc = L.bcd_hip_selection_denoise(handle, ns_ptr, None if null_list else arr, len(layers) if n is None else n)
        return rc, L.bcd_hip_last_error(hipctx.h).decode()

    good = (d_col.data_ptr(), d_cov.data_ptr(), out_a.data_ptr())
    good_b = (d_col.data_ptr(), d_cov.data_ptr(), out_b.data_ptr())
    empty = hipctx.selection()
    cases = {
        "never filled": (reuse([good], handle=empty.h), "holds no frame"),
        "null layer list": (reuse([good], null_list=True), "null layer list"),
        "no layer": (reuse([good], n=0), "between 1 and 16"),
        "too many layers": (reuse([good] * 17), "between 1 and 16"),
        "null colours": (reuse([(None, good[1], good[2])]), "null image pointer in a layer"),
        "null covariances": (reuse([good, (good[0], None, good_b[2])]), "null image pointer in a layer"),
        "null output": (reuse([good, (good[0], good[1], None)]), "null image pointer in a layer"),
        "two equal outputs": (reuse([good, good]), "share (part of) an output"),
        "overlapping outputs": (reuse([good, (good[0], good[1], good[2] + 12 * W)]), "share (part of) an output"),
        "output is an input": (reuse([good, (good[0], good[1], good[0])]), "overlaps an input image"),
        "output overlaps the sample counts": (reuse([(good[0], good[1], d_ns.data_ptr())], ns_ptr=d_ns.data_ptr()), "overlaps the sample counts"),
    }
    for name, ((rc, msg), want) in cases.items():
        assert rc == EINVAL and want in msg, (name, rc, msg)
    assert reuse([good], handle=None)[0] == EINVAL                                # (no context to leave a message on)
    with pytest.raises(bh.BcdHipError, match="holds no frame"):
        empty.read(0)
    with pytest.raises(bh.BcdHipError, match="scale out of range"):
        sel.read(1)
    # _keep: a null selection, one of another context; and a call that fails leaves the selection invalid, not half-filled
    arr = (bh.Layer * 1)()
    arr[0].d_colors, arr[0].d_covariances, arr[0].d_out = good
    args = (d_ns.data_ptr(), d_hist.data_ptr(), W, H, D, 1, C.byref(prm), arr, 1)
    assert L.bcd_hip_denoise_layers_keep(hipctx.h, *args, None) == EINVAL and "null selection" in L.bcd_hip_last_error(hipctx.h).decode()
    other_ctx = bh.Context(0)
    try:
        foreign = other_ctx.selection()
        assert L.bcd_hip_denoise_layers_keep(hipctx.h, *args, foreign.h) == EINVAL and "another context" in L.bcd_hip_last_error(hipctx.h).decode()
        assert not foreign.info()["valid"]
    finally:
        other_ctx.close()
    victim = hipctx.selection()
    hipctx.denoise_layers(d_ns, d_hist, [(d_col, d_cov)], 1, prm, keep=victim)
    assert victim.info()["valid"]
    assert L.bcd_hip_denoise_layers_keep(hipctx.h, d_ns.data_ptr(), None, W, H, D, 1, C.byref(prm), arr, 1, victim.h) == EINVAL
    assert not victim.info()["valid"] and reuse([good], handle=victim.h)[0] == EINVAL
    assert L.bcd_hip_denoise_layers_keep(hipctx.h, d_ns.data_ptr(), d_hist.data_ptr(), W, H, D, 9, C.byref(prm), arr, 1, victim.h) == EINVAL   # too many scales
    assert not victim.info()["valid"]
    victim.close()
    empty.close()
    with pytest.raises(bh.BcdHipError, match="closed"):
        empty.info()
    # ... and the kept selection gives what it gave
    outs = sel.denoise(c["d_layers"][:2], outs=[out_a, out_b])
    for k in range(2):
        assert rel_linf(outs[k].cpu().numpy(), c["kept"][k]) <= TOL_SAME


# ---- 9. the moments-only snapshot -----------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("layers", [0, 2])
def test_moments_are_the_statistics_without_the_histograms(hipctx, layers):
    """70 x 33 (no multiple of 64 or 256): after scattered adds that leave pixels with 0 and with 1 sample (1 / 0: NaN and inf, bit for bit), after a
    dense pass, after a splatted batch; plain and with two colour layers beside the beauty; the state is not changed"""
    import torch
    W, H = 70, 33
    N = W * H
    g = torch.Generator(device="cpu").manual_seed(7 + layers)
    acc = hipctx.accumulator(W, H, layers=layers)

    def check(tag):
        want = acc.statistics()
        poison = tuple(torch.full_like(t, 123.0) for t in want[:3])
        hipctx.synchronize()                                    # (the fills ran on torch's stream)
        got = acc.moments(out=poison)
        again = acc.statistics()
        hipctx.synchronize()
        for name, a, b_, c_ in zip(("ns", "mean", "cov"), got, want, again):
            assert np.array_equal(bits(a), bits(b_)), (tag, name)
            assert np.array_equal(bits(b_), bits(c_)), (tag, name, "state changed")
        assert np.array_equal(bits(want[3]), bits(again[3]))
        fresh = acc.moments()
        hipctx.synchronize()
        assert all(np.array_equal(bits(a), bits(b_)) for a, b_ in zip(fresh, want[:3]))
        return want[0].cpu().numpy().reshape(-1)

    def lay(shape):
        return [(torch.rand(shape, generator=g) * 2).cuda() for _ in range(layers)] if layers else None

    n = N
    pix = torch.randint(0, N, (n,), generator=g, dtype=torch.int32)
    acc.add_samples(pix.cuda(), (torch.rand((n, 3), generator=g) * 3).cuda(), (torch.rand((n,), generator=g) + 0.5).cuda(), layers=lay((n, 3)))
    counts = np.bincount(pix.numpy(), minlength=N)
    ns = check("scattered")
    assert (counts == 0).any() and (counts == 1).any() and np.array_equal(ns == 0, counts == 0)
    mean = acc.moments()[1]
    hipctx.synchronize()
    mean = mean.cpu().numpy().reshape(N, 3)
    assert np.isnan(mean[counts == 0]).all() and np.isfinite(mean[counts > 0]).all()
    acc.add_dense((torch.rand((H, W, 3, 3), generator=g) * 2).cuda(), layers=lay((H, W, 3, 3)))
    check("dense")
    acc.set_filter("tent", 1.5)
    m = 2 * N
    xy = torch.rand((m, 2), generator=g) * torch.tensor([W, H], dtype=torch.float32)
    acc.add_splatted(xy.cuda(), (torch.rand((m, 3), generator=g) * 2).cuda(), None, layers=lay((m, 3)))
    check("splatted")
    acc.close()
