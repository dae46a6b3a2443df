"""GPU tests of the sequence object in a mode (bcd_hip_sequence_create_mode, Context.sequence(..., layers=, moments=, features=); DESIGN 16, "Modes") against
the per-frame call that defines it: frame t of T comes out, per layer, as what that call returns for frame t with the neighbours max(0, t - R) ..
min(T - 1, t + R) except t in ascending order.

  mode          layers  gate                      per-frame call
  hist_L3       3       none                      Context.denoise_temporal_layers
  hist_gate     1       F = 3 with variances      Context.denoise_temporal_guided
  mom_L1        1       none                      Context.denoise_temporal_moments
  mom_L2_gate   2       F = 2 without variances   Context.denoise_temporal_moments with the guide

  * T = 5 frames (oracle_lib.synth_inputs, one seed per frame, 32 spp, the layers of temporal_layers_cases.share_layers, the features of
    guide_cross_cases.features_of) at 40x28 and 52x36 -- the sizes of tests/test_gpu_sequence.py -- R = 1 and 2, 1 and 2 scales, -m 1 -r 1, hist_L3 also
    -m 0 -r 0: per popped frame processed / fallback / similar_total of every scale and the spectral counters of every scale and layer equal the per-frame
    call's; every layer is within TOL = 1e-4 relative L-inf of it (the project's bar for results that differ by the order of float atomics); last_masks of
    every neighbour at every scale equal the stage calls on the pyramid levels the stage reducers build (in-frame: similarity_masks / _moments + the guide
    gate; cross: similarity_masks_cross / _moments_cross + similarity_masks_guide_cross through gate_masks), bit for bit; info: 4 computed / 4 transposed
    pairs at R = 1, 7 / 7 at R = 2; with set_reuse(0) every pair is computed, with the same masks, stats and layers;
  * cross_feature_passes of mode_info: one per COMPUTED pair and scale -- a transposed neighbour launches no cross feature pass;
  * device_bytes of a moments sequence is below that of the histogram sequence of the same shape by at least the histogram bytes of its slots;
  * host push and pop equal device push and pop, bytes uploaded = T x the bytes of one frame of the mode;
  * protocol: T = 1 against the single-frame call of the mode, T = 2, reset, a second sequence on the same context;
  * a sequence of bcd_hip_sequence_create beside one of bcd_hip_sequence_create_mode with one layer, histograms and no gate: the same frames, masks,
    counters and device_bytes, both equal to the per-frame call; each refuses the other's push / pop where the issue says so;
  * every argument refusal of create, push and pop, the context staying usable."""
import ctypes as C

import numpy as np
import pytest

import guide_cross_cases as gc
import moments_cross_cases as xc
import oracle_lib as ol
import temporal_layers_cases as tl

pytestmark = pytest.mark.gpu

TOL = 1e-4        # relative to the layer's maximum (tests/test_gpu_sequence.py, tests/test_gpu_temporal.py; README / DESIGN 6)
SEEDS = (1234, 77, 4321, 99, 2024)
T = len(SEEDS)
PAIRS = {1: 4, 2: 7}      # unordered pairs of T = 5 frames within R
F32 = np.float32

MODES = {
    "hist_L3": dict(L=3, moments=False, F=0, var=False),
    "hist_gate": dict(L=1, moments=False, F=3, var=True),
    "mom_L1": dict(L=1, moments=True, F=0, var=False),
    "mom_L2_gate": dict(L=2, moments=True, F=2, var=False),
}


def t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def rel_linf(got, want):
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "non-finite pattern differs"
    return float(np.max(np.abs(np.where(ok, got, 0) - np.where(ok, want, 0))) / np.max(np.abs(np.where(ok, want, 0))))


_frames = {}


def frames_of(W, H):
    """T frames as dicts of NumPy arrays: ns, hist, layers [(colours, covariances)] * 3, feat (H, W, 3), var (H, W, 3)"""
    if (W, H) not in _frames:
        l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = np.stack([np.where(((l + 2 * c) // 11) % 2 > 0, 0.8, 0.15), 0.2 + 0.6 * c / W, 0.5 + 0.4 * np.sin(12.0 * l / H)], -1).astype(F32)   # (gc.features_of)
        out = []
        for seed in SEEDS:
            col, ns, hist, cov, _ = ol.synth_inputs(W, H, 32, seed)
            rng = np.random.default_rng(seed + 5)
            f = (base + F32(0.02) * rng.standard_normal(base.shape).astype(F32)).astype(F32)
            v = (F32(0.0004) * (F32(1) + F32(0.5) * rng.random(base.shape).astype(F32))).astype(F32)
            out.append(dict(ns=ns, hist=hist, layers=tl.share_layers(col, cov), feat=f, var=v))
        _frames[(W, H)] = out
    return _frames[(W, H)]


def mode_frame(fr, mode, conv=lambda a: a):
    """the arguments of Sequence.push in `mode`"""
    m = MODES[mode]
    F = m["F"]
    return (conv(fr["ns"]), None if m["moments"] else conv(fr["hist"]), [(conv(c), conv(v)) for c, v in fr["layers"][:m["L"]]],
            conv(np.ascontiguousarray(fr["feat"][..., :F])) if F else None, conv(np.ascontiguousarray(fr["var"][..., :F])) if F and m["var"] else None)


def params(mode, m=1.0, r=1):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=1234, tau=xc.TAU if MODES[mode]["moments"] else 1.0)


def make_sequence(ctx, mode, W, H, D, S, R, prm):
    m = MODES[mode]
    return ctx.sequence(W, H, D, S, R, prm, layers=m["L"], moments=m["moments"], var_floor=xc.VAR_FLOOR, features=m["F"], feature_variances=m["var"],
                        feature_floors=gc.FLOORS[:m["F"]], feature_threshold=gc.TAU_G)


def stats_of(ctx, S, L):
    st = [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total, spectral=s.spectral_inverses) for s in (ctx.stats(k) for k in range(S))]
    return st, [[ctx.layer_spectral_inverses(s, k) for k in range(L)] for s in range(S)]


def neighbours_of(i, R, n):
    return [f for f in range(max(0, i - R), min(n - 1, i + R) + 1) if f != i]


def levels_of(ctx, d, mode, S):
    """the pyramid levels of one frame (device tensors of mode_frame) by the stage reducers: [dict(ns, hist, col, pixcov, feat, var)] of the guide layer"""
    ns, hist, layers, feat, var = d
    col, cov = layers[0]
    out = []
    for s in range(S):
        if s:
            cov = ctx.downscale_cov(cov, ns)                # (weighted by the finer level's counts)
            col = ctx.downscale_avg(col)
            hist = None if hist is None else ctx.downscale_sum(hist)
            ns = ctx.downscale_sum(ns.reshape(ns.shape[0], ns.shape[1], 1))
            feat = None if feat is None else ctx.downscale_avg(feat)
            var = None if var is None else ctx.downscale_avg(var) * 0.25
        out.append(dict(ns=ns, hist=hist, col=col, pixcov=ctx.pixel_cov(cov, ns), feat=feat, var=var))
    return out


def stage_masks(ctx, mode, prm, me, nbs):
    """[(mask, count)] of the in-frame set and of every neighbour at one level, by the stage calls: the selection pass, then the feature gate"""
    m = MODES[mode]
    tau, floors = prm.hist_dist_threshold, gc.FLOORS[:m["F"]]
    if m["moments"]:
        own = ctx.similarity_masks_moments(me["col"], me["pixcov"], 1, 6, tau, xc.VAR_FLOOR)
    else:
        own = ctx.similarity_masks(me["hist"], me["ns"], 1, 6, tau)
    if m["F"]:
        g, _ = ctx.similarity_masks_guide(me["feat"], me["var"], floors, gc.TAU_G, 1, 6)
        own = ctx.gate_masks(own[0], own[1], g, 6)
    out = [own]
    for nb in nbs:
        if m["moments"]:
            x = ctx.similarity_masks_moments_cross(me["col"], me["pixcov"], nb["col"], nb["pixcov"], 1, 6, tau, xc.VAR_FLOOR)
        else:
            x = ctx.similarity_masks_cross(me["hist"], me["ns"], nb["hist"], nb["ns"], 1, 6, tau)
        if m["F"]:
            g, _ = ctx.similarity_masks_guide_cross(me["feat"], me["var"], nb["feat"], nb["var"], floors, gc.TAU_G, 1, 6)
            x = ctx.gate_masks(x[0], x[1], g, 6)
        out.append(x)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in out]


def frame_call(ctx, mode, d, i, nbs, S, prm):
    """the per-frame call of `mode` for frame i with the neighbours nbs -> the list of outputs"""
    m = MODES[mode]
    ns, hist, layers, feat, var = d[i]
    guide = {}
    if m["F"]:
        guide = dict(features=feat, neighbour_features=[d[f][3] for f in nbs], variances=var, neighbour_variances=[d[f][4] for f in nbs] if m["var"] else None,
                     floors=gc.FLOORS[:m["F"]], threshold=gc.TAU_G)
    if m["moments"]:
        if not nbs:
            if m["F"]:
                return ctx.denoise_guided(ns, None, layers, S, prm, feat, variances=var, floors=gc.FLOORS[:m["F"]], threshold=gc.TAU_G, var_floor=xc.VAR_FLOOR)
            return ctx.denoise_moments(ns, layers, S, prm, xc.VAR_FLOOR)
        return ctx.denoise_temporal_moments(ns, layers, [(d[f][0], d[f][2]) for f in nbs], S, prm, var_floor=xc.VAR_FLOOR, **guide)
    if not nbs:
        if m["F"]:
            return ctx.denoise_guided(ns, hist, layers, S, prm, feat, variances=var, floors=gc.FLOORS[:m["F"]], threshold=gc.TAU_G)
        return ctx.denoise_layers(ns, hist, layers, S, prm)
    if m["F"]:
        return ctx.denoise_temporal_guided(ns, hist, layers, [(d[f][0], d[f][1], d[f][2]) for f in nbs], S, prm, **guide)
    return ctx.denoise_temporal_layers(ns, hist, layers, [(d[f][0], d[f][1], d[f][2]) for f in nbs], S, prm)


_refs = {}


def reference(ctx, mode, W, H, R, S, m=1.0, r=1, n=T):
    """per frame of the first n frames (outputs, stats, spectral counters, masks[scale][neighbour]) of the per-frame call and the stage calls, once per
    configuration"""
    key = (mode, W, H, R, S, m, r, n)
    if key not in _refs:
        prm = params(mode, m, r)
        L = MODES[mode]["L"]
        d = [mode_frame(f, mode, t) for f in frames_of(W, H)[:n]]
        lv = [levels_of(ctx, f, mode, S) for f in d]
        out = []
        for i in range(n):
            nbs = neighbours_of(i, R, n)
            outs = frame_call(ctx, mode, d, i, nbs, S, prm)
            ctx.synchronize()
            st = stats_of(ctx, S, L)
            masks = [stage_masks(ctx, mode, prm, lv[i][s], [lv[f][s] for f in nbs]) for s in range(S)] if nbs else []
            out.append(([o.cpu().numpy() for o in outs], st, masks))
        _refs[key] = out
    return _refs[key]


def run(seq, frames, S, L, host=False, with_masks=True):
    """the push / pop protocol over `frames` (arguments of push) -> [(index, layers, stats, masks[scale][neighbour])]"""
    ctx, out, n = seq.ctx, [], len(frames)

    def drain():
        while seq.ready():
            idx, outs = seq.pop_host() if host else seq.pop()
            st = stats_of(ctx, S, L)
            nb = len(neighbours_of(idx, seq.radius, n))
            masks = [[tuple(a.cpu().numpy() for a in seq.last_masks(k, s)) for k in range(nb + 1)] for s in range(S)] if with_masks and nb else []
            out.append((idx, [o if host else o.cpu().numpy() for o in outs], st, masks))

    for k, f in enumerate(frames):
        (seq.push_host if host else seq.push)(*f)
        if k == n - 1:
            seq.end()
        drain()
    assert seq.ready() == 0
    return out


def check_against(got, want, label=""):
    assert [g[0] for g in got] == list(range(len(want)))
    worst, bits = 0.0, 0
    for (idx, outs, st, masks), (wouts, wst, wmasks) in zip(got, want):
        assert st == wst, (idx, st, wst)
        assert all(s["similar_total"] > 0 and s["processed"] > 0 for s in st[0])
        assert len(outs) == len(wouts)
        for k, (o, w) in enumerate(zip(outs, wouts)):
            e = rel_linf(o, w)
            worst = max(worst, e)
            assert e <= TOL, (idx, k, e)
        if masks:
            assert len(masks) == len(wmasks)
            for s, (ms, wms) in enumerate(zip(masks, wmasks)):
                assert len(ms) == len(wms)
                for k, ((m, c), (wm, wc)) in enumerate(zip(ms, wms)):
                    assert np.array_equal(m, wm) and np.array_equal(c, wc), "frame %d, scale %d, neighbour %d: the masks differ" % (idx, s, k)
                    bits += int(c.sum()) if k else 0
    if label:
        print("%s: worst layer deviation from the per-frame call %.2e" % (label, worst))
    return worst, bits


CASES = [(mode, 1.0, 1) for mode in MODES] + [("hist_L3", 0.0, 0)]


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode,m,r", CASES)
def test_sequence_in_a_mode_is_the_per_frame_call(hipctx, mode, m, r, W, H, R, S):
    want = reference(hipctx, mode, W, H, R, S, m, r)
    L, F = MODES[mode]["L"], MODES[mode]["F"]
    fr = [mode_frame(f, mode, t) for f in frames_of(W, H)]
    seq = make_sequence(hipctx, mode, W, H, fr[0][1].shape[2] if fr[0][1] is not None else 0, S, R, params(mode, m, r))
    try:
        got = run(seq, fr, S, L)
        _, bits = check_against(got, want, "sequence %s %dx%d R=%d S=%d m=%g" % (mode, W, H, R, S, m))
        assert bits > 0                                                       # (the cross masks compared are not empty)
        info, mi = seq.info(), seq.mode_info()
        assert info["frames_pushed"] == info["frames_popped"] == info["pyramids_built"] == T
        assert info["cross_computed"] == info["cross_transposed"] == PAIRS[R]
        assert info["bytes_uploaded"] == 0 and info["device_bytes"] > 0
        assert (mi["nb_layers"], mi["moments"], mi["nb_features"], mi["feature_variances"]) == (L, int(MODES[mode]["moments"]), F, int(MODES[mode]["var"]))
        # a transposed neighbour launches no cross feature pass: one per computed pair and scale, none without a gate
        assert mi["cross_feature_passes"] == (PAIRS[R] * S if F else 0)
        # with set_reuse(0) every pair is computed (and gated) from both sides: the same masks, stats and layers
        seq.reset()
        seq.set_reuse(False)
        check_against(run(seq, fr, S, L), want)
        info, mi = seq.info(), seq.mode_info()
        assert info["cross_transposed"] == 0 and info["cross_computed"] == 2 * PAIRS[R]
        assert mi["cross_feature_passes"] == (2 * PAIRS[R] * S if F else 0)
    finally:
        seq.close()


def test_a_moments_sequence_holds_no_histogram(hipctx):
    W, H, R, S = 40, 28, 2, 2
    held = {}
    for mode in ("mom_L1", "hist_one"):
        fr = frames_of(W, H)
        D = fr[0]["hist"].shape[2]
        if mode == "mom_L1":
            seq, frames = make_sequence(hipctx, mode, W, H, 0, S, R, params(mode)), [mode_frame(f, mode, t) for f in fr]
        else:
            seq, frames = hipctx.sequence(W, H, D, S, R, params("hist_L3")), [(t(f["layers"][0][0]), t(f["ns"]), t(f["hist"]), t(f["layers"][0][1])) for f in fr]
        try:
            for k, f in enumerate(frames):
                seq.push(*f)
                if k == T - 1:
                    seq.end()
                while seq.ready():
                    seq.pop()
            held[mode] = seq.info()["device_bytes"]
        finally:
            seq.close()
    hist_bytes = (2 * R + 1) * (W * H + (W // 2) * (H // 2)) * D * 4            # every slot, both levels
    print("device_bytes: moments %d, histograms %d, the slots' histograms %d" % (held["mom_L1"], held["hist_one"], hist_bytes))
    assert held["mom_L1"] <= held["hist_one"] - hist_bytes


@pytest.mark.parametrize("mode,R,S", [("hist_L3", 1, 2), ("hist_gate", 2, 1), ("mom_L1", 2, 2), ("mom_L2_gate", 1, 1)])
def test_host_push_and_pop_equal_device_push_and_pop(hipctx, mode, R, S):
    W, H = 40, 28
    m = MODES[mode]
    want = reference(hipctx, mode, W, H, R, S)
    fr = [mode_frame(f, mode) for f in frames_of(W, H)]
    D = 0 if m["moments"] else fr[0][1].shape[2]
    seq = make_sequence(hipctx, mode, W, H, D, S, R, params(mode))
    try:
        check_against(run(seq, fr, S, m["L"], host=True), want)
        info = seq.info()
        assert info["bytes_uploaded"] == T * W * H * (1 + D + 9 * m["L"] + m["F"] * (2 if m["var"] else 1)) * 4
        assert info["cross_computed"] == info["cross_transposed"] == PAIRS[R]
    finally:
        seq.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_protocol_one_frame_two_frames_reset_and_a_second_sequence(hipctx, mode):
    import bcd_amd.hip as bh
    W, H, R, S = 40, 28, 2, 2
    m = MODES[mode]
    L = m["L"]
    fr = [mode_frame(f, mode, t) for f in frames_of(W, H)]
    D = 0 if m["moments"] else fr[0][1].shape[2]
    seq = make_sequence(hipctx, mode, W, H, D, S, R, params(mode))

    def refused(call, word):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert word in str(e.value), str(e.value)

    try:
        refused(seq.pop, "not ready")
        # T = 1: the single-frame call of the mode
        got1 = run(seq, fr[:1], S, L)
        check_against(got1, reference(hipctx, mode, W, H, R, S, n=1))
        refused(lambda: seq.last_masks(0, 0), "no neighbour")
        refused(lambda: seq.push(*fr[1]), "ended")
        # T = 2: the two frames are each other's only neighbours
        seq.reset()
        assert seq.ready() == 0 and seq.info()["frames_pushed"] == 0 and seq.mode_info()["cross_feature_passes"] == 0
        check_against(run(seq, fr[:2], S, L), reference(hipctx, mode, W, H, R, S, n=2))
        assert seq.info()["cross_computed"] == 1 and seq.info()["cross_transposed"] == 1
        # the ring
        seq.reset()
        for k in range(3):
            seq.push(*fr[k])
        refused(lambda: seq.push(*fr[3]), "pop first")
        seq.reset()
        check_against(run(seq, fr, S, L), reference(hipctx, mode, W, H, R, S))
        held = seq.info()["device_bytes"]
        seq.reset()
        check_against(run(seq, fr, S, L, with_masks=False), reference(hipctx, mode, W, H, R, S))
        assert seq.info()["device_bytes"] == held                             # nothing is allocated once the buffers exist
    finally:
        seq.close()
    # a second sequence of another size and radius on the same context
    W2, H2 = 52, 36
    fr2 = [mode_frame(f, mode, t) for f in frames_of(W2, H2)]
    seq2 = make_sequence(hipctx, mode, W2, H2, D, 1, 1, params(mode))
    try:
        check_against(run(seq2, fr2, 1, L), reference(hipctx, mode, W2, H2, 1, 1))
    finally:
        seq2.close()


def test_the_existing_create_call_and_the_mode_of_one_histogram_layer_are_today_s_sequence(hipctx):
    """bcd_hip_sequence_create, and bcd_hip_sequence_create_mode with one layer, histograms and no gate: the frames, stats, masks, counters and device_bytes
    of the per-frame call bcd_hip_denoise_temporal, computed here"""
    import bcd_amd.hip as bh
    W, H, R, S = 52, 36, 2, 2
    prm = params("hist_L3")
    fr = frames_of(W, H)
    D = fr[0]["hist"].shape[2]
    plain = [(t(f["layers"][0][0]), t(f["ns"]), t(f["hist"]), t(f["layers"][0][1])) for f in fr]
    want = []
    for i in range(T):
        nbs = neighbours_of(i, R, T)
        out = hipctx.denoise_temporal(*plain[i], [plain[f] for f in nbs], S, prm)
        hipctx.synchronize()
        st = [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total, spectral=s.spectral_inverses) for s in (hipctx.stats(k) for k in range(S))]
        masks = [hipctx.similarity_masks(plain[i][2], plain[i][1], 1, 6, 1.0)] + [hipctx.similarity_masks_cross(plain[i][2], plain[i][1], plain[f][2], plain[f][1], 1, 6, 1.0)
                                                                                    for f in nbs]
        want.append((out.cpu().numpy(), st, [(a.cpu().numpy(), b.cpu().numpy()) for a, b in masks]))
    results = {}
    for how in ("create", "create_mode"):
        seq = hipctx.sequence(W, H, D, S, R, prm) if how == "create" else hipctx.sequence(W, H, D, S, R, prm, layers=1)
        try:
            got = []
            for k in range(T):
                if how == "create":
                    seq.push(*plain[k])
                else:
                    seq.push(plain[k][1], plain[k][2], [(plain[k][0], plain[k][3])])
                if k == T - 1:
                    seq.end()
                while seq.ready():
                    idx, out = seq.pop()
                    out = out if how == "create" else out[0]
                    st = [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total, spectral=s.spectral_inverses)
                          for s in (hipctx.stats(k2) for k2 in range(S))]
                    nb = len(neighbours_of(idx, R, T))
                    got.append((out.cpu().numpy(), st, [tuple(a.cpu().numpy() for a in seq.last_masks(k2, 0)) for k2 in range(nb + 1)]))
            for (o, st, masks), (wo, wst, wmasks) in zip(got, want):
                assert st == wst and rel_linf(o, wo) <= TOL
                assert all(np.array_equal(a, wa) and np.array_equal(b, wb) for (a, b), (wa, wb) in zip(masks, wmasks))
            results[how] = seq.info()
            assert seq.mode_info()["cross_feature_passes"] == 0 and seq.mode_info()["nb_layers"] == 1
            if how == "create":                                                # the calls of a mode are refused, and the sequence goes on
                seq.reset()
                with pytest.raises(bh.BcdHipError) as e:
                    seq.mode = dict(layers=1, features=0)
                    try:
                        seq.push(plain[0][1], plain[0][2], [(plain[0][0], plain[0][3])])
                    finally:
                        seq.mode = None
                assert "bcd_hip_sequence_create" in str(e.value)
                seq.push(*plain[0])
                seq.end()
                ptrs = (C.c_void_p * 1)(plain[0][0].data_ptr())
                assert bh.lib().bcd_hip_sequence_pop_layers(seq.h, ptrs, 1, None) == -1 and "bcd_hip_sequence_pop" in bh.lib().bcd_hip_last_error(hipctx.h).decode()
                assert seq.pop()[0] == 0
        finally:
            seq.close()
    assert results["create"] == results["create_mode"]
    assert results["create"]["cross_computed"] == results["create"]["cross_transposed"] == PAIRS[R]
    # device_bytes, from the buffers of DESIGN 16: per level 2R + 1 slots (colours, sample counts, histograms, covariances, per-pixel covariances), the masks
    # of every pair kept (24 B per pixel), the in-frame masks and R transposed masks, and the coarse output; a grow-only buffer of n bytes holds n + n / 16 + 256
    alloc = lambda n: n + n // 16 + 256
    total = alloc((W // 2) * (H // 2) * 12)
    for npx in (W * H, (W // 2) * (H // 2)):
        total += (2 * R + 1) * (alloc(12 * npx) + alloc(4 * npx) + alloc(4 * D * npx) + 2 * alloc(24 * npx)) + (PAIRS[R] + 1 + R) * alloc(24 * npx)
    assert results["create"]["device_bytes"] == total


def test_refusals_of_create_push_and_pop_then_a_successful_run(hipctx):
    import torch
    import bcd_amd.hip as bh
    from bcd_amd._prototypes import FrameLayer, SequenceFrame, SequenceMode
    Lb = bh.lib()
    W, H, R, S = 40, 28, 1, 1
    EINVAL, EUNSUPPORTED = -1, -4
    prm = params("hist_L3")
    err = lambda: Lb.bcd_hip_last_error(hipctx.h).decode()
    fr = frames_of(W, H)
    D = fr[0]["hist"].shape[2]
    floors = (C.c_float * 3)(*gc.FLOORS)
    h = C.c_void_p()

    def mode(L=2, moments=0, var_floor=0.01, F=0, fvar=0, fl=floors, tau=1.0, reserved=None):
        return SequenceMode(L, moments, var_floor, F, fvar, C.addressof(fl) if fl is not None else None, tau, reserved)

    def create(m, w=W, hh=H, d=D, s=S, r=R, p=prm, out=C.byref(h)):
        return Lb.bcd_hip_sequence_create_mode(hipctx.h, w, hh, d, s, r, C.byref(p) if p is not None else None, C.byref(m) if m is not None else None, out)

    for L in (0, 17, -1):
        assert create(mode(L=L)) == EINVAL and "layers" in err()
    for F in (-1, 9):
        assert create(mode(F=F)) == EINVAL and "feature channels" in err()
    assert create(None) == EINVAL and create(mode(), out=None) == EINVAL and create(mode(), p=None) == EINVAL
    assert create(mode(reserved=1)) == EINVAL and "reserved" in err()
    assert create(mode(moments=2)) == EINVAL and create(mode(fvar=1)) == EINVAL
    for bad in (-1.0, float("nan"), float("inf")):
        assert create(mode(moments=1, var_floor=bad)) == EINVAL and "variance floor" in err()
        assert create(mode(F=3, tau=bad)) == EINVAL and "threshold" in err()
        assert create(mode(F=3, fl=(C.c_float * 3)(0.02, bad, 0.5))) == EINVAL and "floor" in err()
    assert create(mode(F=2, fl=(C.c_float * 2)(0.0, 0.0))) == EINVAL and "count" in err()                   # a guide that cannot count
    assert create(mode(F=2, fl=None)) == EINVAL and "floors" in err()
    assert create(mode(F=2, fvar=1, fl=(C.c_float * 2)(0.0, 0.0)), r=0) == EINVAL and "radius" in err()
    assert create(mode(), r=3) == EINVAL and create(mode(), w=0) == EINVAL and create(mode(), d=0) == EINVAL
    assert create(mode(), s=0) == EINVAL and create(mode(), s=9) == EINVAL
    assert create(mode(), d=300) == EUNSUPPORTED
    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                            # any other geometry, in every mode
        for m in (mode(), mode(moments=1), mode(L=1, F=3, fvar=1), mode(L=1)):
            assert create(m, p=bh.default_params(m=1.0, random_order=1, w=w, b=b)) == EUNSUPPORTED
            assert "patch radius 1 and search radius 6" in err()
    assert not h.value
    assert create(mode(moments=1), d=0) == 0 and h.value                        # a moments sequence takes no D
    Lb.bcd_hip_sequence_destroy(h)
    h = C.c_void_p()
    assert Lb.bcd_hip_sequence_create_mode(hipctx.h, W, H, D, S, R, C.byref(prm), C.byref(mode(L=2, F=3, fvar=1)), C.byref(h)) == 0 and h.value
    try:
        d = mode_frame(fr[0], "hist_L3", t)
        feat, var = t(fr[0]["feat"]), t(fr[0]["var"])
        torch.cuda.synchronize()
        la = (FrameLayer * 2)(FrameLayer(d[2][0][0].data_ptr(), d[2][0][1].data_ptr()), FrameLayer(d[2][1][0].data_ptr(), d[2][1][1].data_ptr()))
        good = dict(nsamples=d[0].data_ptr(), histograms=d[1].data_ptr(), layers=C.addressof(la), features=feat.data_ptr(), variances=var.data_ptr(), reserved=None)

        def push(host=False, **kw):
            f = SequenceFrame(**dict(good, **kw))
            return (Lb.bcd_hip_sequence_push_frame_host if host else Lb.bcd_hip_sequence_push_frame)(h, C.byref(f))

        for host in (False, True):
            assert push(host, nsamples=None) == EINVAL and "null" in err()
            assert push(host, histograms=None) == EINVAL and "histograms" in err()                  # missing from a histogram sequence
            assert push(host, layers=None) == EINVAL and "layer" in err()
            assert push(host, features=None) == EINVAL and "feature" in err()                        # features missing
            assert push(host, variances=None) == EINVAL and "variances" in err()                     # variances in some frames and not others
            assert push(host, reserved=1) == EINVAL and "reserved" in err()
            short = (FrameLayer * 2)(la[0], FrameLayer(None, None))
            assert push(host, layers=C.addressof(short)) == EINVAL and "layer" in err()               # a missing layer
        assert Lb.bcd_hip_sequence_push_frame(h, None) == EINVAL
        out = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr())
        idx = C.c_int64(-7)
        assert Lb.bcd_hip_sequence_pop_layers(h, ptrs, 2, C.byref(idx)) == EINVAL and "not ready" in err()
        assert push() == 0 and push() == 0
        # the plain calls on a sequence of another mode
        p4 = (d[2][0][0].data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2][0][1].data_ptr())
        assert Lb.bcd_hip_sequence_push(h, *p4) == EINVAL and "bcd_hip_sequence_push_frame" in err()
        assert Lb.bcd_hip_sequence_push_host(h, *p4) == EINVAL and "bcd_hip_sequence_push_frame" in err()
        assert Lb.bcd_hip_sequence_pop(h, out[0].data_ptr(), None) == EINVAL and "bcd_hip_sequence_pop_layers" in err()
        assert Lb.bcd_hip_sequence_pop_host(h, out[0].data_ptr(), None) == EINVAL and "bcd_hip_sequence_pop_layers" in err()
        # a pop with a wrong layer count or a null output
        for n in (1, 3, 0):
            assert Lb.bcd_hip_sequence_pop_layers(h, ptrs, n, C.byref(idx)) == EINVAL and "number of" in err()
        assert Lb.bcd_hip_sequence_pop_layers(h, None, 2, C.byref(idx)) == EINVAL and "null" in err()
        assert Lb.bcd_hip_sequence_pop_layers_host(h, (C.c_void_p * 2)(out[0].data_ptr(), None), 2, C.byref(idx)) == EINVAL and "null" in err()
        assert Lb.bcd_hip_sequence_pop_layers(h, (C.c_void_p * 2)(out[0].data_ptr(), out[0].data_ptr()), 2, C.byref(idx)) == EINVAL and "share" in err()
        assert Lb.bcd_hip_sequence_mode_info(h, None) == EINVAL
        assert idx.value == -7 and float(out[0].abs().sum() + out[1].abs().sum()) == 0.0           # nothing ran
        assert Lb.bcd_hip_sequence_pop_layers(h, ptrs, 2, None) == 0 and bool(out[1].any())        # (the index is optional)
    finally:
        Lb.bcd_hip_sequence_destroy(h)
    # a moments sequence: histograms and features are unexpected
    h = C.c_void_p()
    assert Lb.bcd_hip_sequence_create_mode(hipctx.h, W, H, 0, S, R, C.byref(prm), C.byref(mode(L=2, moments=1)), C.byref(h)) == 0
    try:
        f = SequenceFrame(**good)
        assert Lb.bcd_hip_sequence_push_frame(h, C.byref(f)) == EINVAL and "histograms" in err()
        f = SequenceFrame(**dict(good, histograms=None))
        assert Lb.bcd_hip_sequence_push_frame(h, C.byref(f)) == EINVAL and "feature" in err()
        f = SequenceFrame(**dict(good, histograms=None, features=None))
        assert Lb.bcd_hip_sequence_push_frame(h, C.byref(f)) == EINVAL and "feature" in err()    # variances alone
        f = SequenceFrame(**dict(good, histograms=None, features=None, variances=None))
        assert Lb.bcd_hip_sequence_push_frame(h, C.byref(f)) == 0
    finally:
        Lb.bcd_hip_sequence_destroy(h)
    for fn in (Lb.bcd_hip_sequence_push_frame, Lb.bcd_hip_sequence_push_frame_host):
        assert fn(None, None) == EINVAL
    assert Lb.bcd_hip_sequence_pop_layers(None, None, 1, None) == EINVAL and Lb.bcd_hip_sequence_mode_info(None, None) == EINVAL
    # the context is still usable
    mode_name = "mom_L2_gate"
    seq = make_sequence(hipctx, mode_name, W, H, 0, S, R, params(mode_name))
    try:
        check_against(run(seq, [mode_frame(f, mode_name, t) for f in fr], S, 2), reference(hipctx, mode_name, W, H, R, S))
    finally:
        seq.close()


def python_sequence(hipctx, mode, frames, R, S, prm):
    """[[layer, ...] per frame] of the Python Sequence over frames of frames_of's form"""
    m = MODES[mode]
    fr = [mode_frame(f, mode, t) for f in frames]
    H, W = frames[0]["ns"].shape[:2]
    seq = make_sequence(hipctx, mode, W, H, 0 if m["moments"] else frames[0]["hist"].shape[2], S, R, prm)
    try:
        return [g[1] for g in run(seq, fr, S, m["L"], with_masks=False)]
    finally:
        seq.close()


@pytest.mark.parametrize("mode,R,S", [("hist_L3", 2, 2), ("hist_gate", 1, 1), ("mom_L1", 1, 2), ("mom_L2_gate", 2, 1)])
def test_core_denoise_sequence_and_the_cpp_class_return_the_python_sequence_s_layers(hipctx, mode, R, S):
    """core.denoise_sequence drives bcd::SequenceDenoiser (libbcdcore.so) with setFrameSettings(true) through the host push and pop"""
    import bcd_amd.core as core
    W, H = 40, 28
    m = MODES[mode]
    frames = frames_of(W, H)[:4]
    prm = params(mode)
    want = python_sequence(hipctx, mode, frames, R, S, prm)
    F = m["F"]
    kw = dict(radius=R, nscales=S, tau=prm.hist_dist_threshold, seed=prm.order_seed, var_floor=xc.VAR_FLOOR, layers=[f["layers"][1:m["L"]] for f in frames])
    if F:
        kw.update(features=[f["feat"][..., :F] for f in frames], feature_variances=[f["var"][..., :F] for f in frames] if m["var"] else None, feature_floors=gc.FLOORS[:F],
                  feature_threshold=gc.TAU_G)
    cpp = [(f["layers"][0][0], f["ns"], None if m["moments"] else f["hist"], f["layers"][0][1]) for f in frames]
    ok, got = core.denoise_sequence(cpp, **kw)
    assert ok and len(got) == 4
    for g, w_ in zip(got, want):
        assert len(g) == m["L"]
        for a, b_ in zip(g, w_):
            assert rel_linf(a, b_) <= TOL
    # what the class refuses of a later frame, before the device is asked again: a layer fewer, other feature buffers, no layer registered at a pop
    if m["L"] > 1:
        assert not core.denoise_sequence(cpp, break_settings=8, **kw)[0]
        assert not core.denoise_sequence(cpp, break_settings=32, **kw)[0]
    if F:
        assert not core.denoise_sequence(cpp, break_settings=16, **kw)[0]


def test_bcd_cli_sequence_with_layers_and_features_end_to_end(hipctx, tmp_path):
    """bcd_cli --sequence-in with one --sequence-layer and --sequence-features (with variances) over four 40x28 frames: every output of both layers is the
    Python Sequence's after the half-float EXR round trip (the comparison of the other CLI tests)"""
    import os
    import subprocess
    import torch
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 40, 28
    frames = frames_of(W, H)[:4]
    on_disk = []
    for k, f in enumerate(frames):
        stem = str(tmp_path / ("shot.%04d" % (k + 3)))
        (col, cov), (col1, cov1) = f["layers"][0], f["layers"][1]
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(f["hist"], f["ns"]), True)
        core.write_exr(stem + "_cov.exr", cov, True)
        core.write_exr(str(tmp_path / ("diffuse.%04d.exr" % (k + 3))), col1, False)
        core.write_exr(str(tmp_path / ("diffuse_cov.%04d.exr" % (k + 3))), cov1, True)
        core.write_exr(str(tmp_path / ("feat.%04d.exr" % (k + 3))), f["feat"], True)
        core.write_exr(str(tmp_path / ("featvar.%04d.exr" % (k + 3))), f["var"], True)
        on_disk.append(dict(ns=f["ns"], hist=f["hist"], feat=f["feat"], var=f["var"],                 # (colours go through half precision on disk)
                            layers=[(core.read_exr(stem + ".exr", False), cov), (core.read_exr(str(tmp_path / ("diffuse.%04d.exr" % (k + 3))), False), cov1)]))
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    r = subprocess.run([exe, "--sequence-in", str(tmp_path / "shot.%04d.exr"), "--sequence-out", str(tmp_path / "clean.%04d.exr"), "--first", "3", "--last", "6",
                        "--temporal-radius", "2", "-p", "0", "-s", "2", "-m", "1", "--seed", "5",
                        "--sequence-layer", str(tmp_path / "diffuse.%04d.exr"), str(tmp_path / "diffuse_cov.%04d.exr"), str(tmp_path / "diffuse_clean.%04d.exr"),
                        "--sequence-features", str(tmp_path / "feat.%04d.exr"), "--sequence-feature-variances", str(tmp_path / "featvar.%04d.exr"),
                        "--sequence-feature-floors", ",".join(str(x) for x in gc.FLOORS), "--sequence-feature-threshold", str(gc.TAU_G)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    MODES["cli"] = dict(L=2, moments=False, F=3, var=True)
    try:
        want = python_sequence(hipctx, "cli", on_disk, 2, 2, bh.default_params(m=1.0, seed=5))
    finally:
        del MODES["cli"]
    for k in range(4):
        for name, layer in (("clean", 0), ("diffuse_clean", 1)):
            w_ = hipctx.zero_bad_values(torch.from_numpy(want[k][layer]).cuda()).cpu().numpy()
            got = core.read_exr(str(tmp_path / ("%s.%04d.exr" % (name, k + 3))), False)
            assert np.max(np.abs(got - w_.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w_), (k, name)
