"""GPU tests of bcd_hip_denoise_layers: several colour layers denoised with ONE similar-patch selection.
Layer k of a layered call is what bcd_hip_denoise returns for (col_k, ns, hist, cov_k): every layer is held to the CPU oracle called once per layer
with the shared histogram (relative L-inf < 1e-4 of that layer's own maximum, the project's parity bar), to the plain call on the same build
(<= 1e-5: same arithmetic, the float atomics of the aggregation arrive in another order -- the bound of the band tests), and the per-scale
statistics of the layered call are those of the plain call on layer 0.
Beyond the split of one frame into smooth factors: 16 layers (every slot of the layer table and of the per-layer counters), 7 layers at b = 8 (groups of
three in the layered tile kernel), layers of independent content in both orders, frames on which most main pixels are fallback pixels.  Every layered
comparison also reports bayes_ref.rel_local per layer through BCD_TEST_REPORT (not asserted; docs/EXPERIMENTS.md section 11).  The stages of the
layered path on constructed similar sets: tests/test_gpu_layers_stage.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

TOL = 1e-4        # against the oracle, relative to the layer's own maximum (README / DESIGN 6)
TOL_SAME = 1e-5   # against bcd_hip_denoise on the same build
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _report(line):
    print(line)
    if os.environ.get("BCD_TEST_REPORT"):
        with open(os.environ["BCD_TEST_REPORT"], "a") as f:
            f.write(line + "\n")


def report_local(tag, k, got, want, against):
    """reported, not asserted: the error of a pixel relative to the largest value of its 15 x 15 neighbourhood -- what the frame-wide maximum of
    rel_linf hides in the dark parts of a layer (docs/EXPERIMENTS.md section 11)"""
    import bayes_ref as br
    _report("layers-frame %-34s layer %2d vs %-10s rel_linf %.3e rel_local %.3e" % (tag, k, against, rel_linf(got, want), br.rel_local(got, want)))


def dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrs]


def rel_linf(got, want):
    """relative L-inf over the values that are finite in `want`; the non-finite patterns must agree"""
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "non-finite pattern differs"
    return float(np.max(np.abs(np.where(ok, got, 0) - np.where(ok, want, 0))) / np.max(np.abs(np.where(ok, want, 0))))


def orders(W, H, w, random_order, seed, nscales):
    import bcd_amd.hip as bh
    out = []
    for s in range(nscales):
        out.append(bh.visit_order(W, H, w, random_order, bh.scale_seed(seed, s)))
        W, H = W // 2, H // 2
    return out


def scale_layer(col, cov, g):
    """the layer whose samples are the frame's samples times the per-pixel, per-channel factor g (H x W x 3): mean and covariance follow exactly"""
    g = g.astype(np.float32)
    gg = np.stack([g[..., 0] * g[..., 0], g[..., 1] * g[..., 1], g[..., 2] * g[..., 2], g[..., 1] * g[..., 2], g[..., 0] * g[..., 2],
                   g[..., 0] * g[..., 1]], -1)   # xx, yy, zz, yz, xz, xy
    return np.ascontiguousarray(col * g), np.ascontiguousarray(cov * gg)


def split_layers(col, cov, n=4):
    """layer 0: the frame itself (the beauty = the sum of the others); then a smooth, a textured and a dim (x 1e-3) share of it: they differ in
    colour, magnitude and covariance"""
    H, W, _ = col.shape
    l, c = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    smooth = np.stack([0.2 + 0.5 * c / W, 0.6 - 0.4 * l / H, 0.3 + 0.3 * (l + c) / (H + W)], -1)
    tex = 0.999 - smooth
    tex = tex * np.stack([0.5 + 0.5 * np.sin(0.9 * c + 0.4 * l), 0.5 + 0.5 * np.cos(0.7 * l), ((l.astype(int) // 3 + c.astype(int) // 5) % 2) * 0.9 + 0.1], -1)
    dim = np.full((H, W, 3), 1e-3, np.float32)
    layers = [(col, cov), scale_layer(col, cov, smooth), scale_layer(col, cov, tex), scale_layer(col, cov, dim)]
    return layers[:n]


_frames = {}


def frame(W, H, spp, sigma=0.15, spike=0.01, seed=1234):
    key = (W, H, spp, sigma, spike, seed)
    if key not in _frames:
        _frames[key] = ol.synth_inputs(W, H, spp, seed, sigma, spike)[:4]
    return _frames[key]


def mixed_counts_frame(W, H, seed=9):
    """per-pixel sample counts drawn from {16, 24, 32, 48}: a 48-spp stream thinned per pixel (general counts: the RATIO form of the distance kernel)"""
    rng = np.random.default_rng(seed)
    samples, _ = ol.synth_samples(W, H, 48, seed=seed, sigma=0.3, spike_prob=0.01)
    counts = rng.choice(np.array([16, 24, 32, 48]), size=W * H)
    keep = (np.arange(48)[None, :] < counts[:, None]).reshape(-1)
    ns, mean, cov, hist = ol.oracle_ops()["accumulate"](np.ascontiguousarray(samples[keep]), W, H)
    return mean, ns, hist, cov


def stats_tuple(ctx, S):
    return [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (ctx.stats(k) for k in range(S))]


def run_case(ctx, col, ns, hist, cov, S, nlayers=4, oracle=True, layers=None, oracle_layers=None, **kw):
    """one layered call over split_layers(col, cov) (or `layers`) checked against the oracle per layer (`oracle_layers`: only these), against the plain
    call per layer, and for the statistics of the shared selection; prints every measured figure"""
    import bcd_amd.hip as bh
    H, W, _ = hist.shape
    prm = bh.default_params(**kw)
    layers = split_layers(col, cov, nlayers) if layers is None else layers
    tag = "%dx%d S=%d L=%d %s" % (W, H, S, len(layers), " ".join("%s=%s" % kv for kv in sorted(kw.items()) if kv[0] in ("b", "w", "m", "tau")))
    d_ns, d_hist = dev(ns, hist)
    d_layers = [tuple(dev(c, v)) for c, v in layers]
    outs = [o.cpu().numpy() for o in ctx.denoise_layers(d_ns, d_hist, d_layers, S, prm)]
    shared = stats_tuple(ctx, S)
    spectral = [sum(ctx.layer_spectral_inverses(s, k) for k in range(len(layers))) for s in range(S)]
    assert spectral == [ctx.stats(s).spectral_inverses for s in range(S)]        # the scale's figure is the sum over the layers
    m, w, b = kw.get("m", 1.0), kw.get("w", 1), kw.get("b", 6)
    od = orders(W, H, w, kw.get("random_order", 1), kw.get("seed", 1234), S) if m != 0.0 else None
    op = ol.params(tau=kw.get("tau", 1.0), w=w, b=b, min_eig=kw.get("min_eig", 1e-8), m=m)
    for k, (c, v) in enumerate(layers):
        single = ctx.denoise(d_layers[k][0], d_ns, d_hist, d_layers[k][1], S, prm).cpu().numpy()
        if k == 0:
            assert stats_tuple(ctx, S) == shared, "the layered call's selection is not the plain call's on layer 0"
        e_same = rel_linf(outs[k], single)       # (also: the layer's non-finite pattern is its own single-call pattern)
        print("layer %d: vs plain call %.3e" % (k, e_same))
        report_local(tag, k, outs[k], single, "plain call")
        assert e_same <= TOL_SAME
        if oracle and (oracle_layers is None or k in oracle_layers):
            want = (ol.denoise_multiscale(c, ns, hist, v, S, op, orders=od) if S > 1 else
                    ol.denoise_mono(c, ns, hist, v, op, order=od[0] if od else None))
            e = rel_linf(outs[k], want)
            print("layer %d: vs oracle %.3e (own maximum %.3e)" % (k, e, float(np.nanmax(np.abs(want)))))
            report_local(tag, k, outs[k], want, "oracle")
            assert e < TOL
    return outs


@pytest.mark.parametrize("name", ["96x64_s3_m1_r1", "72x50_s1_m1_r0", "m0", "b3", "b12", "w2", "mixed_counts"])
def test_layers_match_the_oracle_and_the_plain_call(hipctx, name):
    if name == "96x64_s3_m1_r1":
        run_case(hipctx, *frame(96, 64, 16), 3, m=1.0, random_order=1, seed=11)
    elif name == "72x50_s1_m1_r0":
        run_case(hipctx, *frame(72, 50, 16), 1, m=1.0, random_order=0, seed=5)
    elif name == "m0":
        run_case(hipctx, *frame(61, 45, 16), 2, m=0.0, random_order=0)
    elif name == "b3":
        run_case(hipctx, *frame(66, 50, 8), 2, nlayers=3, b=3, m=1.0, random_order=1, seed=3)
    elif name == "b12":
        run_case(hipctx, *frame(45, 41, 8), 1, nlayers=3, b=12, m=1.0, random_order=1, seed=3)
    elif name == "w2":
        run_case(hipctx, *frame(44, 36, 8), 1, nlayers=3, w=2, b=4, m=1.0, random_order=1, seed=3)
    else:
        col, ns, hist, cov = mixed_counts_frame(96, 72)
        assert sorted(np.unique(ns).tolist()) == [16.0, 24.0, 32.0, 48.0]
        run_case(hipctx, col, ns, hist, cov, 2, m=1.0, random_order=0, seed=5)
        assert hipctx.stats(0).similarity_path == 2      # the RATIO form served the shared selection


def test_one_spp_frame_with_nan_distances_keeps_counts_and_finiteness_patterns(hipctx):
    """a 1-spp frame (NaN distances, |S| = 0 pixels: DESIGN 6 explains why such frames are not held to 1e-4 against the fp32 oracle): the layered
    call's statistics are the plain call's and every layer's non-finite pattern is its own single-call pattern"""
    import bcd_amd.hip as bh
    f = np.load(os.path.join(_GOLDEN, "core_lowspp.npz"))
    col, ns, hist, cov = f["col"], f["ns"], f["hist"], f["cov"]
    prm = bh.default_params(m=1.0, random_order=0)
    layers = split_layers(col, cov, 3)
    d_ns, d_hist = dev(ns, hist)
    d_layers = [tuple(dev(c, v)) for c, v in layers]
    outs = [o.cpu().numpy() for o in hipctx.denoise_layers(d_ns, d_hist, d_layers, 1, prm)]
    shared = stats_tuple(hipctx, 1)
    assert np.array_equal(np.isnan(outs[0]), np.isnan(f["out_m1"]))
    for k in range(3):
        single = hipctx.denoise(d_layers[k][0], d_ns, d_hist, d_layers[k][1], 1, prm).cpu().numpy()
        if k == 0:
            assert stats_tuple(hipctx, 1) == shared
        assert np.array_equal(np.isfinite(outs[k]), np.isfinite(single)) and np.array_equal(np.isnan(outs[k]), np.isnan(single))


def test_a_single_layer_is_the_plain_call(hipctx):
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(96, 64, 16)
    prm = bh.default_params(m=1.0, random_order=1, seed=11)
    d_col, d_ns, d_hist, d_cov = dev(col, ns, hist, cov)
    out, = hipctx.denoise_layers(d_ns, d_hist, [(d_col, d_cov)], 3, prm)
    shared = stats_tuple(hipctx, 3)
    want = hipctx.denoise(d_col, d_ns, d_hist, d_cov, 3, prm).cpu().numpy()
    assert stats_tuple(hipctx, 3) == shared
    e = rel_linf(out.cpu().numpy(), want)
    print("one layer vs plain call %.3e" % e)
    assert e <= TOL_SAME


def test_zero_layer_and_non_finite_layer_stay_on_their_own(hipctx):
    """a layer of zeros with zero covariance comes back as zeros wherever a pixel was aggregated; a layer full of NaN / inf members changes no other
    layer.  The other layers are compared with the same call WITHOUT that layer to <= 1e-5, not bit for bit: every layer has sums of its own,
    nothing of one layer is ever added to another, but the float atomics that aggregate a layer's patches arrive in an order that differs from run
    to run, so two runs of the SAME layer already differ in the last bits."""
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(72, 50, 16)
    prm = bh.default_params(m=1.0, random_order=1, seed=7)
    layers = split_layers(col, cov, 3)
    d_ns, d_hist = dev(ns, hist)
    d_layers = [tuple(dev(c, v)) for c, v in layers]
    base = [o.cpu().numpy() for o in hipctx.denoise_layers(d_ns, d_hist, d_layers, 2, prm)]
    zero = tuple(dev(np.zeros_like(col), np.zeros_like(cov)))
    bad_col = col.copy()
    bad_col[::3, ::4, 0] = np.nan
    bad_col[1::5, 2::3, 1] = np.inf
    bad_col[2::7, ::2, 2] = -np.inf
    bad_cov = cov.copy()
    bad_cov[::4, 1::3, :] = np.nan
    bad = tuple(dev(bad_col, bad_cov))
    for pos in (1, 3):   # in the middle and at the end of the list
        with_extra = list(d_layers)
        with_extra.insert(pos, bad)
        with_extra.insert(pos, zero)
        outs = [o.cpu().numpy() for o in hipctx.denoise_layers(d_ns, d_hist, with_extra, 2, prm)]
        z = outs.pop(pos)
        outs.pop(pos)
        aggregated = np.isfinite(base[0])
        assert aggregated.any() and np.all(z[aggregated] == 0.0)
        for k in range(3):
            e = rel_linf(outs[k], base[k])
            print("layer %d beside a non-finite layer at %d: %.3e" % (k, pos, e))
            assert e <= TOL_SAME


def test_spectral_redo_is_per_layer(hipctx):
    """-e 1e-3 on a low-noise frame sends full estimates to the redo list (their sweep inverse fails its checks: eigenvalues below the floor), the
    same frame scaled by 1000 (covariances by 1e6) has no eigenvalue near the floor and stays on the sweep path: in one call, in either order, each
    layer walks its own redo list and both stay inside the oracle's bar"""
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(64, 48, 32, 0.08, 0.0)
    big = (np.ascontiguousarray(col * 1000.0), np.ascontiguousarray(cov * 1.0e6))
    prm = bh.default_params(m=0.0, min_eig=1e-3)
    d_ns, d_hist = dev(ns, hist)
    op = ol.params(m=0.0, min_eig=1e-3)
    want = {"small": ol.denoise_mono(col, ns, hist, cov, op), "big": ol.denoise_mono(big[0], ns, hist, big[1], op)}
    named = {"small": tuple(dev(col, cov)), "big": tuple(dev(*big))}
    for order in (("big", "small"), ("small", "big"), ("big", "small", "small")):
        outs = hipctx.denoise_layers(d_ns, d_hist, [named[n] for n in order], 1, prm)
        st = hipctx.stats(0)
        per_layer = [hipctx.layer_spectral_inverses(0, k) for k in range(len(order))]
        print("order %s: spectral inverses per layer %s, scale total %d" % (order, per_layer, st.spectral_inverses))
        assert sum(per_layer) == st.spectral_inverses
        for n, count, out in zip(order, per_layer, outs):
            if n == "small":
                assert 0 < count <= st.processed - st.fallback
            else:
                assert count == 0
            e = rel_linf(out.cpu().numpy(), want[n])
            print("  %s: vs oracle %.3e" % (n, e))
            assert e < TOL
    assert len(set(p for p in per_layer if p)) == 1      # the same layer twice: the same redo list


def test_invalid_calls_are_refused_before_any_device_work(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(72, 50, 16)
    H, W, D = hist.shape
    prm = bh.default_params()
    d_col, d_ns, d_hist, d_cov = dev(col, ns, hist, cov)
    out_a, out_b = torch.empty_like(d_col), torch.empty_like(d_col)
    L = bh.lib()

    def call(layers, n=None, ns_ptr=d_ns.data_ptr(), hist_ptr=d_hist.data_ptr(), w=W, h=H, d=D, S=1, p=prm, null_list=False):
        arr = (bh.Layer * max(1, len(layers)))()
        for k, (c, v, o) in enumerate(layers):
            arr[k].d_colors, arr[k].d_covariances, arr[k].d_out = c, v, o
        rc = L.bcd_hip_denoise_layers(hipctx.h, ns_ptr, hist_ptr, w, h, d, S, C.byref(p) if p is not None else None, None if null_list else arr,
                                      len(layers) if n is None else n)
        return rc, L.bcd_hip_last_error(hipctx.h).decode()

    good = (d_col.data_ptr(), d_cov.data_ptr(), out_a.data_ptr())
    good_b = (d_col.data_ptr(), d_cov.data_ptr(), out_b.data_ptr())
    EINVAL, EUNSUPPORTED = -1, -4
    cases = {
        "null sample counts": (call([good], ns_ptr=None), EINVAL),
        "null histograms": (call([good], hist_ptr=None), EINVAL),
        "null layer list": (call([good], null_list=True), EINVAL),
        "null colours": (call([(None, good[1], good[2])]), EINVAL),
        "null covariances": (call([good, (good[0], None, good_b[2])]), EINVAL),
        "null output": (call([good, (good[0], good[1], None)]), EINVAL),
        "null parameters": (call([good], p=None), EINVAL),
        "no layer": (call([good], n=0), EINVAL),
        "too many layers": (call([good] * 17), EINVAL),
        "two equal outputs": (call([good, good]), EINVAL),
        "overlapping outputs": (call([good, (good[0], good[1], good[2] + 12 * W)]), EINVAL),
        "output is an input": (call([good, (good[0], good[1], good[0])]), EINVAL),
        "output overlaps the histograms": (call([(good[0], good[1], d_hist.data_ptr() + 4 * W * D)]), EINVAL),
        "empty image": (call([good], w=0), EINVAL),
        "too many scales": (call([good, good_b], S=6), EINVAL),
        "histogram depth": (call([good, good_b], d=300), EUNSUPPORTED),
        "search radius": (call([good, good_b], p=bh.default_params(b=16)), EUNSUPPORTED),
    }
    for name, ((rc, msg), want) in cases.items():
        assert rc == want and msg, (name, rc, msg)
    with pytest.raises(bh.BcdHipError):
        hipctx.denoise_layers(d_ns, d_hist, [], 1, prm)
    # ... and the context is as good as before
    outs = hipctx.denoise_layers(d_ns, d_hist, [(d_col, d_cov), (d_col, d_cov)], 1, prm, outs=[out_a, out_b])
    want = hipctx.denoise(d_col, d_ns, d_hist, d_cov, 1, prm).cpu().numpy()
    for o in outs:
        assert rel_linf(o.cpu().numpy(), want) <= TOL_SAME


def test_one_context_serves_calls_of_different_sizes_and_layer_counts(hipctx):
    """grow-only workspace: 4 layers on a larger frame, 2 layers on a smaller one (other scale count), 3 layers on the largest, then a plain
    denoise: every result is the oracle's, no state of an earlier call leaks"""
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        run_case(ctx, *frame(96, 64, 16), 3, nlayers=4, oracle=False, m=1.0, random_order=1, seed=11)
        run_case(ctx, *frame(72, 50, 16), 1, nlayers=2, m=1.0, random_order=0, seed=5)
        run_case(ctx, *frame(96, 64, 16), 3, nlayers=3, m=1.0, random_order=1, seed=11)
        col, ns, hist, cov = frame(61, 45, 16)
        got = ctx.denoise(*dev(col, ns, hist, cov), 2, bh.default_params(m=0.0, random_order=0)).cpu().numpy()
        e = rel_linf(got, ol.denoise_multiscale(col, ns, hist, cov, 2, ol.params(m=0.0)))
        print("plain call after the layered ones: vs oracle %.3e" % e)
        assert e < TOL
    finally:
        ctx.close()


def test_cxx_add_layer_goes_through_the_layered_call(hipctx):
    """bcd::Denoiser / MultiscaleDenoiser::addLayer (through capi.cpp): the outputs are the library call's; clearLayers() gives the plain denoise()
    back; a layer of the wrong size and the spike prefilter are refused"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(72, 50, 16)
    layers = split_layers(col, cov, 3)
    d_ns, d_hist = dev(ns, hist)
    for S in (1, 2):
        ok, outs = core.denoise_layers(layers, ns, hist, nscales=S, m=1.0, random_order=True, seed=21)
        assert ok
        want = hipctx.denoise_layers(d_ns, d_hist, [tuple(dev(c, v)) for c, v in layers], S, bh.default_params(m=1.0, random_order=1, seed=21))
        for k in range(3):
            assert rel_linf(outs[k], want[k].cpu().numpy()) <= TOL_SAME
    ok, outs = core.denoise_layers(layers, ns, hist, nscales=2, seed=21, after_clear=True)
    assert ok
    ok1, plain, _ = core.denoise(col, ns, hist, cov, nscales=2, seed=21)
    assert ok1 and rel_linf(outs[0], plain) <= TOL_SAME
    assert not core.denoise_layers(layers, ns, hist, size_mismatch_layer=2)[0]
    assert not core.denoise_layers(layers, ns, hist, prefilter_factor=2.0)[0]
    # zero_bad applies to every layer's output
    neg = [(c.copy(), v) for c, v in layers]
    neg[1][0][5:20, 5:20, :] = -1.0
    ok, outs = core.denoise_layers(neg, ns, hist, nscales=1, m=0.0, zero_bad=True)
    assert ok and all(np.isfinite(o).all() and (o >= 0).all() for o in outs)


def test_bcd_cli_layers_end_to_end(hipctx, tmp_path):
    """bcd_cli --layer twice: every output is the library call's result after the half-float EXR round trip (the comparison of the plain CLI test)"""
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 72, 56
    col, ns, hist, cov = core.synthetic_scene(W, H, 16, 21, 0.15, 0.02)
    layers = split_layers(col, cov, 3)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    args, on_disk = [], [(core.read_exr(stem + ".exr", False), cov)]
    for k in (1, 2):
        core.write_exr(stem + "_l%d.exr" % k, layers[k][0], False)
        core.write_exr(stem + "_l%d_cov.exr" % k, layers[k][1], True)
        args += ["--layer", stem + "_l%d.exr" % k, stem + "_l%d_cov.exr" % k, str(tmp_path / ("out_l%d.exr" % k))]
        on_disk.append((core.read_exr(stem + "_l%d.exr" % k, False), layers[k][1]))   # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    r = subprocess.run([exe, "-i", stem + ".exr", "-o", out_path, "-p", "0", "-s", "2", "-b", "4", "-m", "0", "--seed", "5"] + args,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d_ns, d_hist = dev(ns, hist)
    want = hipctx.denoise_layers(d_ns, d_hist, [tuple(dev(c, v)) for c, v in on_disk], 2, bh.default_params(b=4, m=0.0, seed=5))
    for k, path in enumerate([out_path, str(tmp_path / "out_l1.exr"), str(tmp_path / "out_l2.exr")]):
        got = core.read_exr(path, False)
        w = hipctx.zero_bad_values(want[k]).cpu().numpy()
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), k


# ---- 16 layers, a group of three, independent content, fallback-heavy frames ------------------------------------------------------------------------
def rotate_layer(col, cov):
    """(r, g, b) -> (g, b, r), the covariance entries xx yy zz yz xz xy permuted to match"""
    return np.ascontiguousarray(col[..., [1, 2, 0]]), np.ascontiguousarray(cov[..., [1, 2, 0, 4, 5, 3]])


def independent_layer(W, H, spp, seed, sigma):
    """colours and sample covariances of ANOTHER frame (other seed, other noise level) with the same sample counts: content that owes nothing to layer 0,
    which alone drives the lists, |S| and the states"""
    col, ns, hist, cov = frame(W, H, spp, sigma, 0.01, seed)
    return col, cov


def many_layers(col, cov, n, spp):
    """split_layers, then independent frames, their copies x 2^10 (covariances x 2^20) and their channel rotations in turn"""
    H, W, _ = col.shape
    layers = split_layers(col, cov, 4)
    i = 0
    while len(layers) < n:
        c, v = independent_layer(W, H, spp, 500 + i, (0.1, 0.3, 0.2)[i % 3])
        if i % 3 == 1:
            c, v = np.ascontiguousarray(c * np.float32(1024.0)), np.ascontiguousarray(v * np.float32(1024.0 * 1024.0))
        elif i % 3 == 2:
            c, v = rotate_layer(c, v)
        layers.append((c, v))
        i += 1
    return layers[:n]


def full_stats(ctx, S):
    return [(s.processed, s.fallback, s.similar_total, s.similarity_path, s.borderline_pairs, s.spectral_inverses) for s in (ctx.stats(k) for k in range(S))]


@pytest.mark.parametrize("name", ["96x64_s3", "45x41_b12"])
def test_sixteen_layers(name):
    """every slot of the layer table and of the per-layer counters in use, on a context of its own: each layer <= 1e-5 from the plain call on it, the shared
    statistics those of the plain call on layer 0, the per-layer spectral counts summing to the scale's figure, layers 0, 1, 8 and 15 < 1e-4 from the
    oracle; then a plain call and a 2-layer call on the same context give what they gave before the 16-layer call, statistics included"""
    import bcd_amd.hip as bh
    if name == "96x64_s3":
        W, H, spp, S, kw = 96, 64, 16, 3, dict(m=1.0, random_order=1, seed=11)
    else:
        W, H, spp, S, kw = 45, 41, 8, 1, dict(b=12, m=1.0, random_order=1, seed=3)
    col, ns, hist, cov = frame(W, H, spp)
    layers = many_layers(col, cov, 16, spp)
    prm = bh.default_params(**kw)
    ctx = bh.Context(0)
    try:
        d_ns, d_hist = dev(ns, hist)
        d2 = [tuple(dev(c, v)) for c, v in layers[:2]]
        before_plain = ctx.denoise(d2[0][0], d_ns, d_hist, d2[0][1], S, prm).cpu().numpy()
        before_stats = full_stats(ctx, S)
        before_two = [o.cpu().numpy() for o in ctx.denoise_layers(d_ns, d_hist, d2, S, prm)]
        before_two_stats = full_stats(ctx, S)
        run_case(ctx, col, ns, hist, cov, S, layers=layers, oracle_layers=(0, 1, 8, 15), **kw)
        after_plain = ctx.denoise(d2[0][0], d_ns, d_hist, d2[0][1], S, prm).cpu().numpy()
        assert full_stats(ctx, S) == before_stats, "a 16-layer call changed the statistics of the plain call that follows it"
        assert rel_linf(after_plain, before_plain) <= TOL_SAME
        after_two = [o.cpu().numpy() for o in ctx.denoise_layers(d_ns, d_hist, d2, S, prm)]
        assert full_stats(ctx, S) == before_two_stats, "a 16-layer call changed the statistics of the 2-layer call that follows it"
        for k in range(2):
            assert rel_linf(after_two[k], before_two[k]) <= TOL_SAME
    finally:
        ctx.close()


def test_sixteen_layers_with_redo_lists_in_every_slot(hipctx):
    """-e 1e-3 on a low-noise frame: the layers that are copies of the frame take the redo list, their copies x 1000 do not -- alternating over 16
    layers, so that the running totals in the per-layer counter slots are non-zero from the first slot to the last"""
    import bcd_amd.hip as bh
    col, ns, hist, cov = frame(64, 48, 32, 0.08, 0.0)
    small, big = (col, cov), (np.ascontiguousarray(col * 1000.0), np.ascontiguousarray(cov * 1.0e6))
    prm = bh.default_params(m=0.0, min_eig=1e-3)
    d_ns, d_hist = dev(ns, hist)
    d_small, d_big = tuple(dev(*small)), tuple(dev(*big))
    outs = hipctx.denoise_layers(d_ns, d_hist, [d_small if k % 2 == 0 else d_big for k in range(16)], 1, prm)
    st = hipctx.stats(0)
    per_layer = [hipctx.layer_spectral_inverses(0, k) for k in range(16)]
    print("spectral inverses per layer %s, scale total %d" % (per_layer, st.spectral_inverses))
    assert sum(per_layer) == st.spectral_inverses
    assert all(c == 0 for c in per_layer[1::2]) and len(set(per_layer[0::2])) == 1 and 0 < per_layer[0] <= st.processed - st.fallback
    op = ol.params(m=0.0, min_eig=1e-3)
    want = [ol.denoise_mono(small[0], ns, hist, small[1], op), ol.denoise_mono(big[0], ns, hist, big[1], op)]
    for k in (0, 1, 14, 15):
        e = rel_linf(outs[k].cpu().numpy(), want[k % 2])
        report_local("64x48 16 layers -e 1e-3", k, outs[k].cpu().numpy(), want[k % 2], "oracle")
        assert e < TOL
    hipctx.denoise(d_small[0], d_ns, d_hist, d_small[1], 1, prm)
    assert hipctx.stats(0).spectral_inverses == per_layer[0]             # a layer's count is the plain call's on that layer


def test_seven_layers_search_radius_8_groups_of_three(hipctx):
    """b = 8: three layers' windows fit the LDS of the layered tile kernel, six further layers go as 3 + 3; with four layers the one group is full"""
    col, ns, hist, cov = frame(60, 46, 8)
    layers = many_layers(col, cov, 7, 8)
    run_case(hipctx, col, ns, hist, cov, 1, layers=layers, b=8, m=1.0, random_order=1, seed=3)
    run_case(hipctx, col, ns, hist, cov, 1, layers=layers[:5], oracle=False, b=8, m=0.0, random_order=0)     # 4 further layers: 3 + 1


def test_layer_of_independent_content_in_both_orders(hipctx):
    """a layer from another frame (other seed, other noise level, its own covariance) beside the beauty: in second place the beauty's histograms
    select for it; in first place its own images drive layer 0's code path while the beauty follows"""
    col, ns, hist, cov = frame(72, 50, 16)
    other = independent_layer(72, 50, 16, 4321, 0.3)
    assert float(np.max(np.abs(col - other[0]))) > 0.1 and not np.array_equal(cov, other[1])
    for layers in ([(col, cov), other], [other, (col, cov)], [(col, cov), other, rotate_layer(*other)]):
        run_case(hipctx, col, ns, hist, cov, 2, layers=layers, m=1.0, random_order=1, seed=7)


@pytest.mark.parametrize("nlayers,m", [(4, 0.0), (5, 1.0)])
def test_fallback_heavy_frame(hipctx, nlayers, m):
    """8 samples per pixel and a histogram threshold of 0.5: in the oracle's own |S| image most main pixels are below the 28 members a full estimate
    needs (found on the CPU: 64 % of this frame), so the layered tile kernel, with its overlapping aggregates across tile borders, carries the frame"""
    W, H, tau = 72, 50, 0.5
    col, ns, hist, cov = frame(W, H, 8, 0.15, 0.01, 77)
    _, (proc, fb, nsim) = ol.denoise_mono(col, ns, hist, cov, ol.params(tau=tau, m=0.0), want_diag=True)
    main = nsim[1:H - 1, 1:W - 1]
    share = float((main < 28).mean())
    print("share of main pixels with |S| < 28 in the oracle: %.2f" % share)
    assert share >= 0.5
    layers = many_layers(col, cov, nlayers, 8)
    run_case(hipctx, col, ns, hist, cov, 1, layers=layers, tau=tau, m=m, random_order=1, seed=9)
    st = hipctx.stats(0)
    print("processed %d, fallback %d" % (st.processed, st.fallback))
    if m == 0.0:                                                         # every main pixel is processed: the fallback pixels are the oracle's
        assert st.processed == main.size and st.fallback == int((main < 28).sum()), (st.processed, st.fallback)
