"""GPU tests of sequences that take per-step motion fields (bcd_hip_sequence_push_frame_motion, Sequence.push(..., motion_prev=, motion_next=); DESIGN 16,
"Sequences with motion") against the frame call that defines a pop: frame t comes out as what the motion call of its mode returns for frame t with the
neighbours max(0, t - R) .. min(T - 1, t + R) except t in ascending order and the fields sequence_motion_ref.sequence_fields composes from the step fields.

  mode          layers  selection   gate                      frame call
  hist_L1       1       histograms  none                      Context.denoise_temporal_layers_motion (one layer: the plain motion call)
  hist_L3       3       histograms  none                      Context.denoise_temporal_layers_motion
  hist_gate     1       histograms  F = 3 with variances      Context.denoise_temporal_guided(motions=)
  mom_L2_gate   2       moments     F = 2 without variances   Context.denoise_temporal_moments(motions=) with the guide

  * T = 5 frames of tests/test_gpu_sequence_modes.py at 40x28 and 52x36, R = 1 and 2, 1 and 2 scales, -m 1 -r 1, the "moving" step fields of
    sequence_motion_cases (translations of up to 4 px per step, NaN pixels, sub-pixel values, one NULL `next` and one NULL `prev`): per popped frame the stats
    of every scale and the spectral counters of every layer equal the frame call's; every layer is within TOL = 1e-4 relative L-inf (results that
    differ by the order of float atomics); last_masks of every neighbour and scale equal, bit for bit, the stage calls on the warped levels (the neighbour
    gathered by motion_ref.warp, its levels by the stage reducers, the cross pass, bcd_hip_gate_masks_valid on motion_ref.valid_levels, the feature gate);
    cross_computed / cross_transposed / neighbours_warped / fields_composed are sequence_motion_ref.counters;
  * all fields NULL: frames, masks and bcd_hip_sequence_info equal those of a plain-push sequence, 4 / 4 and 7 / 7 pairs; all fields zero-valued: the same
    masks bit for bit, cross_transposed == 0, neighbours_warped == the neighbour visits; only frame 2 moving: exactly the pairs with both directions NULL
    are transposed;
  * host push against device push; the prefilter with motion against bcd_hip_denoise_temporal_host_ex with the same factor; reset and a second run;
  * every refusal."""
import ctypes as C

import numpy as np
import pytest

import guide_cross_cases as gc
import moments_cross_cases as xc
import motion_ref as mref
import sequence_motion_cases as mc
import sequence_motion_ref as sref
import test_gpu_sequence_modes as sm

pytestmark = pytest.mark.gpu

TOL = 1e-4        # relative to the layer's maximum (tests/test_gpu_sequence_modes.py; README / DESIGN 6)
T = sm.T
F32 = np.float32
MODES = dict(sm.MODES, hist_L1=dict(L=1, moments=False, F=0, var=False))
CASES = ["hist_L1", "hist_L3", "hist_gate", "mom_L2_gate"]
t = sm.t


def mode_frame(fr, mode, conv=lambda a: a):
    """the arguments of Sequence.push in `mode` (sm.mode_frame, for the modes of this file)"""
    m = MODES[mode]
    F = m["F"]
    return (conv(fr["ns"]), None if m["moments"] else conv(fr["hist"]), [(conv(c), conv(v)) for c, v in fr["layers"][:m["L"]]],
            conv(np.ascontiguousarray(fr["feat"][..., :F])) if F else None, conv(np.ascontiguousarray(fr["var"][..., :F])) if F and m["var"] else None)


def params(mode):
    import bcd_amd.hip as bh
    return bh.default_params(m=1.0, random_order=1, seed=1234, tau=xc.TAU if MODES[mode]["moments"] else 1.0)


def make_sequence(ctx, mode, W, H, D, S, R, prm):
    m = MODES[mode]
    return ctx.sequence(W, H, D, S, R, prm, layers=m["L"], moments=m["moments"], var_floor=xc.VAR_FLOOR, features=m["F"], feature_variances=m["var"],
                        feature_floors=gc.FLOORS[:m["F"]], feature_threshold=gc.TAU_G)


def field_t(f):
    return None if f is None else t(f)


def depth(mode):
    return 0 if MODES[mode]["moments"] else 60


def motion_call(ctx, mode, d, i, nbs, fields, S, prm):
    """the motion frame call of `mode` for frame i with the neighbours nbs and their fields (device tensors or None) -> the list of outputs"""
    m = MODES[mode]
    ns, hist, layers, feat, var = d[i]
    guide = {}
    if m["F"]:
        guide = dict(features=feat, neighbour_features=[d[f][3] for f in nbs], variances=var, neighbour_variances=[d[f][4] for f in nbs] if m["var"] else None,
                     floors=gc.FLOORS[:m["F"]], threshold=gc.TAU_G)
    if m["moments"]:
        return ctx.denoise_temporal_moments(ns, layers, [(d[f][0], d[f][2]) for f in nbs], S, prm, var_floor=xc.VAR_FLOOR, motions=fields, **guide)
    nb = [(d[f][0], d[f][1], d[f][2]) for f in nbs]
    if m["F"]:
        return ctx.denoise_temporal_guided(ns, hist, layers, nb, S, prm, motions=fields, **guide)
    return ctx.denoise_temporal_layers_motion(ns, hist, layers, nb, fields, S, prm)


def warped_levels(ctx, mode, frame, field, S):
    """the levels of a neighbour (a NumPy frame of sm.mode_frame) gathered through `field`, and the validity bytes of every level (None without a field)"""
    if field is None:
        return sm.levels_of(ctx, mode_frame(frame, mode, t), mode, S), [None] * S
    ns, hist, layers, feat, var = mode_frame(frame, mode)
    H, W = ns.shape[:2]
    imgs = [ns.reshape(H, W), layers[0][0], layers[0][1]] + [a for a in (hist, feat, var) if a is not None]
    out, valid = mref.warp(imgs, field)
    rest = iter(out[3:])
    w_hist, w_feat, w_var = (next(rest) if a is not None else None for a in (hist, feat, var))
    d = (t(out[0].reshape(ns.shape)), field_t(w_hist), [(t(out[1]), t(out[2]))], field_t(w_feat), field_t(w_var))
    return sm.levels_of(ctx, d, mode, S), [t(v) for v in mref.valid_levels(valid, S)]


def stage_masks(ctx, mode, prm, me, nbs, valids):
    """the masks of sm.stage_masks with the validity gate of a warped neighbour between its cross pass and its feature gate"""
    m = MODES[mode]
    tau, floors = prm.hist_dist_threshold, gc.FLOORS[:m["F"]]
    if m["moments"]:
        own = ctx.similarity_masks_moments(me["col"], me["pixcov"], 1, 6, tau, xc.VAR_FLOOR)
    else:
        own = ctx.similarity_masks(me["hist"], me["ns"], 1, 6, tau)
    if m["F"]:
        g, _ = ctx.similarity_masks_guide(me["feat"], me["var"], floors, gc.TAU_G, 1, 6)
        own = ctx.gate_masks(own[0], own[1], g, 6)
    out = [(own[0].cpu().numpy(), own[1].cpu().numpy())]
    for nb, v in zip(nbs, valids):
        if m["moments"]:
            x = ctx.similarity_masks_moments_cross(me["col"], me["pixcov"], nb["col"], nb["pixcov"], 1, 6, tau, xc.VAR_FLOOR)
        else:
            x = ctx.similarity_masks_cross(me["hist"], me["ns"], nb["hist"], nb["ns"], 1, 6, tau)
        if v is not None:
            x = ctx.gate_masks_valid(x[0], x[1], v, 1, 6)
        if m["F"]:
            g, _ = ctx.similarity_masks_guide_cross(me["feat"], me["var"], nb["feat"], nb["var"], floors, gc.TAU_G, 1, 6)
            x = ctx.gate_masks(x[0], x[1], g, 6)
        out.append((x[0].cpu().numpy(), x[1].cpu().numpy()))
    return out


_refs = {}


def reference(ctx, mode, kind, W, H, R, S):
    """per frame (outputs, stats, masks[scale][neighbour]) of the motion frame call and of the stage calls, once per configuration"""
    key = (mode, kind, W, H, R, S)
    if key not in _refs:
        prm = params(mode)
        L = MODES[mode]["L"]
        frames = sm.frames_of(W, H)
        steps = mc.step_fields(kind, W, H, T)
        d = [mode_frame(f, mode, t) for f in frames]
        own = [sm.levels_of(ctx, f, mode, S) for f in d]
        out = []
        for i in range(T):
            nbs = sref.neighbours(i, R, T)
            fields = sref.sequence_fields(steps, i, R, T)
            outs = motion_call(ctx, mode, d, i, nbs, [field_t(f) for f in fields], S, prm)
            ctx.synchronize()
            st = sm.stats_of(ctx, S, L)
            wl = [warped_levels(ctx, mode, frames[f], fld, S) for f, fld in zip(nbs, fields)]
            masks = [stage_masks(ctx, mode, prm, own[i][s], [lv[s] for lv, _ in wl], [v[s] for _, v in wl]) for s in range(S)]
            out.append(([o.cpu().numpy() for o in outs], st, masks))
        _refs[key] = out
    return _refs[key]


def pushes(mode, kind, W, H, conv=t):
    """the (args, kwargs) of every push"""
    steps = mc.step_fields(kind, W, H, T)
    cf = (lambda a: None if a is None else conv(a))
    return [(mode_frame(f, mode, conv), dict(motion_prev=cf(p), motion_next=cf(n))) for f, (p, n) in zip(sm.frames_of(W, H), steps)]


def run(seq, frames, S, L, host=False, with_masks=True):
    """sm.run with the keyword arguments of every push"""
    ctx, out, n = seq.ctx, [], len(frames)
    for k, (args, kw) in enumerate(frames):
        (seq.push_host if host else seq.push)(*args, **kw)
        if k == n - 1:
            seq.end()
        while seq.ready():
            idx, outs = seq.pop_host() if host else seq.pop()
            st = sm.stats_of(ctx, S, L)
            nb = len(sref.neighbours(idx, seq.radius, n))
            masks = [[tuple(a.cpu().numpy() for a in seq.last_masks(k, s)) for k in range(nb + 1)] for s in range(S)] if with_masks and nb else []
            out.append((idx, [o if host else o.cpu().numpy() for o in outs], st, masks))
    assert seq.ready() == 0
    return out


def counters_of(seq):
    info = seq.info()
    w, c = seq.motion_info()
    return dict(cross_computed=info["cross_computed"], cross_transposed=info["cross_transposed"], neighbours_warped=w, fields_composed=c)


def same_masks(a, b):
    assert len(a) == len(b)
    for (_, _, _, ma), (_, _, _, mb) in zip(a, b):
        assert len(ma) == len(mb)
        for sa, sb in zip(ma, mb):
            assert len(sa) == len(sb)
            for (m, c), (wm, wc) in zip(sa, sb):
                assert np.array_equal(m, wm) and np.array_equal(c, wc)


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode", CASES)
def test_sequence_with_motion_is_the_motion_frame_call(hipctx, mode, W, H, R, S):
    """measured on an MI355X over the 32 cases: worst layer deviation 1.8e-7 ... 3.0e-7 against TOL = 1e-4 ("Sequences with motion")"""
    want = reference(hipctx, mode, "moving", W, H, R, S)
    L = MODES[mode]["L"]
    seq = make_sequence(hipctx, mode, W, H, depth(mode), S, R, params(mode))
    try:
        got = run(seq, pushes(mode, "moving", W, H), S, L)
        worst, bits = sm.check_against(got, want, "sequence with motion %s %dx%d R=%d S=%d" % (mode, W, H, R, S))
        assert bits > 0                                                       # (the cross masks compared are not empty)
        assert counters_of(seq) == sref.counters(mc.step_fields("moving", W, H, T), R, T)
        info = seq.info()
        assert info["frames_pushed"] == info["frames_popped"] == info["pyramids_built"] == T and info["bytes_uploaded"] == 0
    finally:
        seq.close()


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("mode", ["hist_L1", "mom_L2_gate"])
def test_null_fields_are_a_plain_push_and_zero_fields_select_the_same(hipctx, mode, R):
    W, H, S = 40, 28, 2
    L = MODES[mode]["L"]
    visits = 2 * sm.PAIRS[R]
    fr = [mode_frame(f, mode, t) for f in sm.frames_of(W, H)]
    seq = make_sequence(hipctx, mode, W, H, depth(mode), S, R, params(mode))
    try:
        plain = sm.run(seq, fr, S, L)
        plain_info = seq.info()
        seq.reset()
        null = run(seq, pushes(mode, "null", W, H), S, L)
        assert seq.info() == plain_info and seq.motion_info() == (0, 0)
        assert plain_info["cross_computed"] == plain_info["cross_transposed"] == sm.PAIRS[R]
        same_masks(null, plain)
        for a, b in zip(null, plain):
            assert a[0] == b[0] and a[2] == b[2] and all(sm.rel_linf(x, y) <= TOL for x, y in zip(a[1], b[1]))
        seq.reset()
        zero = run(seq, pushes(mode, "zero", W, H), S, L)
        same_masks(zero, plain)
        for a, b in zip(zero, plain):
            assert a[2] == b[2] and all(sm.rel_linf(x, y) <= TOL for x, y in zip(a[1], b[1]))
        assert counters_of(seq) == dict(cross_computed=visits, cross_transposed=0, neighbours_warped=visits, fields_composed=0 if R == 1 else 6)
        assert counters_of(seq) == sref.counters(mc.step_fields("zero", W, H, T), R, T)
        assert seq.info()["device_bytes"] > plain_info["device_bytes"]        # (the slots' fields arrived with the first one)
    finally:
        seq.close()


@pytest.mark.parametrize("R", [1, 2])
def test_only_pairs_without_a_field_in_either_direction_are_transposed(hipctx, R):
    mode, W, H, S = "hist_L3", 40, 28, 1
    want = reference(hipctx, mode, "partly", W, H, R, S)
    seq = make_sequence(hipctx, mode, W, H, 60, S, R, params(mode))
    try:
        got = run(seq, pushes(mode, "partly", W, H), S, 3)
        sm.check_against(got, want)
        c = counters_of(seq)
        assert c == sref.counters(mc.step_fields("partly", W, H, T), R, T)
        assert c["cross_transposed"] == 2 and c["neighbours_warped"] == (2 if R == 1 else 6)
    finally:
        seq.close()


def test_host_push_is_device_push(hipctx):
    mode, W, H, R, S = "hist_gate", 40, 28, 2, 2
    want = reference(hipctx, mode, "moving", W, H, R, S)
    seq = make_sequence(hipctx, mode, W, H, 60, S, R, params(mode))
    try:
        got = run(seq, pushes(mode, "moving", W, H, conv=lambda a: a), S, 1, host=True)
        sm.check_against(got, want)
        fields = sum(x is not None for e in mc.step_fields("moving", W, H, T) for x in e)
        assert seq.info()["bytes_uploaded"] == (T * (1 + 60 + 9 + 3 + 3) + fields * 2) * W * H * 4
        assert counters_of(seq) == sref.counters(mc.step_fields("moving", W, H, T), R, T)
    finally:
        seq.close()


def test_the_prefilter_leaves_the_fields_alone(hipctx):
    """a frame is filtered in its own grid at its push and warped afterwards: against bcd_hip_denoise_temporal_host_ex with the same factor"""
    mode, W, H, R, S, factor = "hist_L3", 40, 28, 2, 2, 2.0
    prm = params(mode)
    frames = [mode_frame(f, mode) for f in sm.frames_of(W, H)]
    steps = mc.step_fields("moving", W, H, T)
    seq = make_sequence(hipctx, mode, W, H, 60, S, R, prm)
    try:
        seq.set_prefilter(factor)
        got = run(seq, pushes(mode, "moving", W, H), S, 3, with_masks=False)
        assert seq.prefilter_info()[0] == T and seq.prefilter_info()[1] > 0
        for i, (idx, outs, st, _) in enumerate(got):
            nbs = sref.neighbours(i, R, T)
            want = hipctx.denoise_temporal_host_ex(frames[i][0], frames[i][1], frames[i][2], [(frames[f][0], frames[f][1], frames[f][2]) for f in nbs], S, prm,
                                                   spike_factor=factor, motions=sref.sequence_fields(steps, i, R, T))
            assert idx == i and st == sm.stats_of(hipctx, S, 3)
            for k in range(3):
                e = sm.rel_linf(outs[k], want[k])
                assert e <= TOL, (i, k, e)
    finally:
        seq.close()


def test_reset_and_a_second_run(hipctx):
    mode, W, H, R, S = "mom_L2_gate", 40, 28, 2, 1
    want = reference(hipctx, mode, "moving", W, H, R, S)
    seq = make_sequence(hipctx, mode, W, H, 0, S, R, params(mode))
    try:
        fr = pushes(mode, "moving", W, H)
        sm.check_against(run(seq, fr, S, 2), want)
        first, held = counters_of(seq), seq.info()["device_bytes"]
        seq.reset()
        assert seq.motion_info() == (0, 0)
        sm.check_against(run(seq, fr, S, 2), want)
        assert counters_of(seq) == first and seq.info()["device_bytes"] == held        # (nothing was allocated again)
        seq.reset()                                                                    # a frame's fields do not outlive it: the same slots without fields
        null = run(seq, pushes(mode, "null", W, H), S, 2, with_masks=False)
        assert seq.motion_info() == (0, 0) and seq.info()["cross_transposed"] == sm.PAIRS[R]
        assert [g[0] for g in null] == list(range(T))
    finally:
        seq.close()


def test_refusals(hipctx):
    import torch
    import bcd_amd.hip as bh
    L = bh.lib()
    W, H, D = 40, 28, 60
    EINVAL = -1
    mode = "hist_L1"
    prm = params(mode)
    args = mode_frame(sm.frames_of(W, H)[0], mode, t)
    field = t(mc.translation(W, H, 1, 0))
    assert L.bcd_hip_sequence_push_frame_motion(None, None, None, None) == EINVAL
    assert L.bcd_hip_sequence_push_frame_motion_host(None, None, None, None) == EINVAL
    assert L.bcd_hip_sequence_motion_info(None, None, None) == EINVAL
    plain = hipctx.sequence(W, H, D, 1, 1, prm)
    seq = make_sequence(hipctx, mode, W, H, D, 1, 1, prm)
    try:
        frame, keep = seq._frame(*args, ptr=bh._dptr)
        fp = C.c_void_p(field.data_ptr())
        torch.cuda.synchronize()
        # a sequence of bcd_hip_sequence_create refuses the call, like _push_frame
        assert L.bcd_hip_sequence_push_frame_motion(plain.h, C.byref(frame), fp, fp) == EINVAL
        assert b"bcd_hip_sequence_create" in L.bcd_hip_last_error(hipctx.h)
        with pytest.raises(ValueError):
            plain.push(*[t(a) for a in (np.zeros((H, W, 3), F32), np.ones((H, W), F32), np.zeros((H, W, D), F32), np.zeros((H, W, 6), F32))], motion_prev=field)
        # what _push_frame refuses of the frame
        assert L.bcd_hip_sequence_push_frame_motion(seq.h, None, fp, fp) == EINVAL
        broken = bh.SequenceFrame(frame.nsamples, frame.histograms, frame.layers, None, None, 1)
        assert L.bcd_hip_sequence_push_frame_motion(seq.h, C.byref(broken), fp, None) == EINVAL
        assert b"reserved" in L.bcd_hip_last_error(hipctx.h)
        broken = bh.SequenceFrame(None, frame.histograms, frame.layers, None, None, None)
        assert L.bcd_hip_sequence_push_frame_motion(seq.h, C.byref(broken), None, fp) == EINVAL
        broken = bh.SequenceFrame(frame.nsamples, None, frame.layers, None, None, None)
        assert L.bcd_hip_sequence_push_frame_motion_host(seq.h, C.byref(broken), None, None) == EINVAL
        with pytest.raises(ValueError):
            seq.push(*args, motion_next=t(np.zeros((H, W + 1, 2), F32)))
        n, m = C.c_int64(0), C.c_int64(0)
        assert L.bcd_hip_sequence_motion_info(seq.h, None, C.byref(m)) == EINVAL and L.bcd_hip_sequence_motion_info(seq.h, C.byref(n), None) == EINVAL
        assert seq.info()["frames_pushed"] == 0
        # the ring and the end of the sequence, as for every push
        seq.push(*args, motion_next=field)
        seq.push(*args, motion_prev=field)
        with pytest.raises(bh.BcdHipError, match="pop first"):
            seq.push(*args, motion_prev=field)
        seq.end()
        with pytest.raises(bh.BcdHipError, match="ended"):
            seq.push(*args, motion_prev=field)
        # ... and the context and the sequence are usable: both frames pop, each with one warped neighbour
        assert [seq.pop()[0] for _ in range(2)] == [0, 1]
        assert seq.motion_info() == (2, 0) and seq.info()["cross_transposed"] == 0
    finally:
        seq.close()
        plain.close()


# ---- above the C ABI: core.denoise_sequence(motions=) -- which runs bcd::SequenceDenoiser::setFrameMotion -- and bcd_cli, once each at 40x28 ------------------
def test_sequence_denoiser_class_with_frame_motion(hipctx):
    import bcd_amd.core as core
    W, H, R, S = 40, 28, 2, 2
    fr = sm.frames_of(W, H)
    steps = mc.step_fields("moving", W, H, T)
    # one layer of histograms: the result has the shape of the plain sequence's
    want = reference(hipctx, "hist_L1", "moving", W, H, R, S)
    frames = [(f["layers"][0][0], f["ns"], f["hist"], f["layers"][0][1]) for f in fr]
    ok, got = core.denoise_sequence(frames, radius=R, nscales=S, seed=1234, motions=steps)
    assert ok and len(got) == T
    for g, w in zip(got, want):
        assert g.shape == (H, W, 3) and sm.rel_linf(g, w[0][0]) <= TOL
    # without fields the class takes the path it always took
    ok, still = core.denoise_sequence(frames, radius=R, nscales=S, seed=1234)
    ok2, null = core.denoise_sequence(frames, radius=R, nscales=S, seed=1234, motions=[None] * T)
    assert ok and ok2 and all(sm.rel_linf(a, b) <= TOL for a, b in zip(null, still))
    assert max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(got, still)) > 10 * TOL      # (... and the fields changed something)
    # two layers, moment selection, the feature gate
    mode = "mom_L2_gate"
    L, F = MODES[mode]["L"], MODES[mode]["F"]
    want = reference(hipctx, mode, "moving", W, H, R, S)
    frames = [(f["layers"][0][0], f["ns"], None, f["layers"][0][1]) for f in fr]
    ok, got = core.denoise_sequence(frames, radius=R, nscales=S, seed=1234, tau=params(mode).hist_dist_threshold, layers=[f["layers"][1:L] for f in fr],
                                    features=[np.ascontiguousarray(f["feat"][..., :F]) for f in fr], feature_floors=gc.FLOORS[:F], feature_threshold=gc.TAU_G,
                                    var_floor=xc.VAR_FLOOR, motions=steps)
    assert ok
    for g, w in zip(got, want):
        for k in range(L):
            assert sm.rel_linf(g[k], w[0][k]) <= TOL


def test_bcd_cli_sequence_motion_end_to_end(hipctx, tmp_path):
    """bcd_cli --sequence-in ... --sequence-motion-prev / -next over four 40x28 frames: every output is the Python Sequence's frame with the same fields after
    the half-float EXR round trip; the first frame has no `prev` file and the last no `next` file; a file missing in between is an error"""
    import os
    import subprocess
    import torch
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H, n, first = 40, 28, 4, 7
    frames = [core.synthetic_scene(W, H, 16, seed, 0.15, 0.02) for seed in (21, 22, 23, 24)]
    z = np.zeros((H, W, 2), F32)
    steps = [tuple(z if x is None else x for x in e) for e in mc.step_fields("moving", W, H, n)]
    steps[0], steps[-1] = (None, steps[0][1]), (steps[-1][0], None)
    on_disk = []
    for k, (col, ns, hist, cov) in enumerate(frames):
        stem = str(tmp_path / ("shot.%04d" % (k + first)))
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        core.write_exr(stem + "_cov.exr", cov, True)
        for name, field in zip(("prev", "next"), steps[k]):
            if field is not None:
                core.write_exr(str(tmp_path / ("%s.%04d.exr" % (name, k + first))), field, True)      # (32-bit floats: NaN and fractions survive)
        on_disk.append((core.read_exr(stem + ".exr", False), ns, hist, cov))      # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    args = [exe, "--sequence-in", str(tmp_path / "shot.%04d.exr"), "--sequence-out", str(tmp_path / "clean.%04d.exr"), "--first", str(first), "--last", str(first + n - 1),
            "--temporal-radius", "2", "-s", "2", "-m", "1", "--seed", "5", "-p", "0", "--sequence-motion-prev", str(tmp_path / "prev.%04d.exr"),
            "--sequence-motion-next", str(tmp_path / "next.%04d.exr")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seq = hipctx.sequence(W, H, 60, 2, 2, bh.default_params(m=1.0, seed=5), layers=1)
    try:
        pushed = [((t(ns), t(hist), [(t(col), t(cov))]), dict(motion_prev=field_t(p), motion_next=field_t(q))) for (col, ns, hist, cov), (p, q) in zip(on_disk, steps)]
        want = [g[1][0] for g in run(seq, pushed, 2, 1, with_masks=False)]
        assert seq.motion_info()[0] == 10 and seq.info()["cross_transposed"] == 0
    finally:
        seq.close()
    for k in range(n):
        w = hipctx.zero_bad_values(torch.from_numpy(want[k]).cuda()).cpu().numpy()
        got = core.read_exr(str(tmp_path / ("clean.%04d.exr" % (k + first))), False)
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), k
    os.remove(str(tmp_path / ("prev.%04d.exr" % (first + 2))))
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "couldn't load motion image file" in r.stdout and "prev.%04d.exr" % (first + 2) in r.stdout
