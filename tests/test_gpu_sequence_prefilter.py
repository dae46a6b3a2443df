"""GPU tests of the spike prefilter in a sequence (bcd_hip_sequence_set_prefilter / _prefilter_info; DESIGN 16, "Prefilter") against the per-frame composition
that defines it: every frame through bcd_hip_spike_filter_layers on its own (sample counts, histograms unless in moment selection, all layers; features as
pushed), then the frame call of the mode on the filtered frames.

  * T = 5 frames of tests/test_gpu_sequence.py / test_gpu_sequence_modes.py (32 spp, spike probability 0.01) at 40x28 and 52x36, R = 1 and 2, 1 and 2 scales;
    the plain sequence (bcd_hip_sequence_create) and the mode of two layers, moment selection and the feature gate;
  * per popped frame the stats of every scale equal the composition's, every layer is within TOL = 1e-4 relative L-inf of it (the project's bar for results
    that differ by the order of float atomics); the scale-0 masks of last_masks equal, bit for bit, those of the same sequence with set_reuse(0) -- and, in
    the plain mode, the stage calls on the filtered frames;
  * frames_filtered == T, pixels_moved == the sum of the per-frame counts; cross_computed / cross_transposed as without the prefilter;
  * every frame has moved pixels, and the prefiltered frames differ from the unfiltered sequence's by more than 10 TOL somewhere;
  * device push == host push; set_prefilter after a push is refused, after reset accepted; T = 1;
  * bcd::SequenceDenoiser with setSpikePrefilterFrames and bcd_cli --sequence-in ... --prefilter-frames."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sequence as ts
import test_gpu_sequence_modes as tm

pytestmark = pytest.mark.gpu

TOL = 1e-4
T = ts.T
FACTOR = 2.0
MODE = "mom_L2_gate"        # two layers, selection from means and covariances, two feature channels without variances


# ---- the plain sequence ---------------------------------------------------------------------------------------------------------------------------------------
def filtered_plain(ctx, frame):
    """(col, ns, hist, cov) device tensors -> the same through bcd_hip_spike_filter_layers, and the moved count"""
    col, ns, hist, cov = frame
    f_ns, f_hist, f_layers, _, moved = ctx.spike_filter_layers(ns, hist, [(col, cov)], FACTOR, count=True)
    return (f_layers[0][0], f_ns, f_hist, f_layers[0][1]), moved


_plain_refs = {}


def plain_reference(ctx, W, H, R, S, n=T):
    key = (W, H, R, S, n)
    if key not in _plain_refs:
        prm = ts.params(1.0, 1)
        both = [filtered_plain(ctx, ts.dev(f)) for f in ts.frames_of(W, H)[:n]]
        fr, moved = [b[0] for b in both], [b[1] for b in both]
        out = []
        for t in range(n):
            nbs = ts.neighbours_of(t, R, n)
            frame = ctx.denoise_temporal(*fr[t], [fr[f] for f in nbs], S, prm) if nbs else ctx.denoise(*fr[t], S, prm)
            ctx.synchronize()
            st = ts.stats_of(ctx, S)
            masks = [ctx.similarity_masks(fr[t][2], fr[t][1], 1, 6, prm.hist_dist_threshold)]
            masks += [ctx.similarity_masks_cross(fr[t][2], fr[t][1], fr[f][2], fr[f][1], 1, 6, prm.hist_dist_threshold) for f in nbs]
            out.append((frame.cpu().numpy(), st, [(a.cpu().numpy(), b.cpu().numpy()) for a, b in masks]))
        _plain_refs[key] = (out, moved)
    return _plain_refs[key]


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
def test_plain_sequence_with_the_prefilter_is_the_composition(hipctx, W, H, R, S):
    want, moved = plain_reference(hipctx, W, H, R, S)
    assert all(m > 0 for m in moved)                                             # every frame of the case has moved pixels
    fr = [ts.dev(f) for f in ts.frames_of(W, H)]
    kept = [[a.clone() for a in f] for f in fr]
    seq = hipctx.sequence(W, H, 60, S, R, ts.params(1.0, 1))
    try:
        seq.set_prefilter(FACTOR)
        got = ts.run(seq, fr, S)
        worst = ts.check_against(got, want, S)                                   # frames, stats, and the scale-0 masks against the stage calls on the filtered frames
        info = seq.info()
        print("prefiltered sequence %dx%d R=%d S=%d: worst deviation from the composition %.2e, moved %s" % (W, H, R, S, worst, moved))
        assert seq.prefilter_info() == (T, sum(moved))
        assert info["frames_pushed"] == info["frames_popped"] == info["pyramids_built"] == T
        assert info["cross_computed"] == info["cross_transposed"] == ts.PAIRS[R]  # as without the prefilter
        for f, k in zip(fr, kept):                                               # the caller's buffers are read only
            assert all(bool((a == b).all()) for a, b in zip(f, k))
        # the same sequence with set_reuse(0): the same masks, bit for bit
        seq.reset()
        seq.set_reuse(False)
        direct = ts.run(seq, fr, S)
        ts.check_against(direct, want, S)
        for a, b in zip(got, direct):
            assert len(a[3]) == len(b[3]) > 0
            for (m, c), (dm, dc) in zip(a[3], b[3]):
                assert np.array_equal(m, dm) and np.array_equal(c, dc)
        assert seq.prefilter_info() == (T, sum(moved))                           # (reset forgot the counters, the setting stayed)
        info = seq.info()
        assert info["cross_transposed"] == 0 and info["cross_computed"] == 2 * ts.PAIRS[R]
        # ... and the prefilter did something: against the unfiltered sequence
        seq.reset()
        seq.set_reuse(True)
        seq.set_prefilter(0.0)
        plain = ts.run(seq, fr, S, with_masks=False)
        assert seq.prefilter_info() == (0, 0)
        assert max(float(np.max(np.abs(a[1] - b[1])) / np.max(np.abs(b[1]))) for a, b in zip(got, plain)) > 10 * TOL
    finally:
        seq.close()


# ---- layers + moments + features ------------------------------------------------------------------------------------------------------------------------------
def filtered_mode(ctx, d):
    """a device frame of tm.mode_frame (ns, hist or None, layers, feat, var) -> the same with ns, hist and the layers filtered; the features stay"""
    ns, hist, layers, feat, var = d
    f_ns, f_hist, f_layers, _, moved = ctx.spike_filter_layers(ns, hist, layers, FACTOR, count=True)
    return (f_ns, f_hist, f_layers, feat, var), moved


_mode_refs = {}


def mode_reference(ctx, mode, W, H, R, S, n=T):
    key = (mode, W, H, R, S, n)
    if key not in _mode_refs:
        prm = tm.params(mode)
        L = tm.MODES[mode]["L"]
        both = [filtered_mode(ctx, tm.mode_frame(f, mode, tm.t)) for f in tm.frames_of(W, H)[:n]]
        d, moved = [b[0] for b in both], [b[1] for b in both]
        out = []
        for i in range(n):
            outs = tm.frame_call(ctx, mode, d, i, tm.neighbours_of(i, R, n), S, prm)
            ctx.synchronize()
            out.append(([o.cpu().numpy() for o in outs], tm.stats_of(ctx, S, L), []))
        _mode_refs[key] = (out, moved)
    return _mode_refs[key]


def scale0(masks):
    return masks[0] if masks else []


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
def test_sequence_in_a_mode_with_the_prefilter_is_the_composition(hipctx, W, H, R, S):
    want, moved = mode_reference(hipctx, MODE, W, H, R, S)
    assert all(m > 0 for m in moved)
    L = tm.MODES[MODE]["L"]
    fr = [tm.mode_frame(f, MODE, tm.t) for f in tm.frames_of(W, H)]
    seq = tm.make_sequence(hipctx, MODE, W, H, 0, S, R, tm.params(MODE))
    try:
        seq.set_prefilter(FACTOR)
        got = tm.run(seq, fr, S, L)
        worst, _ = tm.check_against([(g[0], g[1], g[2], []) for g in got], want)
        print("prefiltered sequence %s %dx%d R=%d S=%d: worst deviation from the composition %.2e, moved %s" % (MODE, W, H, R, S, worst, moved))
        assert seq.prefilter_info() == (T, sum(moved))
        info = seq.info()
        assert info["cross_computed"] == info["cross_transposed"] == tm.PAIRS[R]
        assert seq.mode_info()["cross_feature_passes"] == tm.PAIRS[R] * S
        seq.reset()
        seq.set_reuse(False)
        direct = tm.run(seq, fr, S, L)
        tm.check_against([(g[0], g[1], g[2], []) for g in direct], want)
        bits = 0
        for a, b in zip(got, direct):
            assert len(scale0(a[3])) == len(scale0(b[3])) > 0
            for k, ((m, c), (dm, dc)) in enumerate(zip(scale0(a[3]), scale0(b[3]))):
                assert np.array_equal(m, dm) and np.array_equal(c, dc)
                bits += int(c.sum()) if k else 0
        assert bits > 0
        seq.reset()
        seq.set_reuse(True)
        seq.set_prefilter(-1.0)                                                  # <= 0: off
        plain = tm.run(seq, fr, S, L, with_masks=False)
        assert seq.prefilter_info() == (0, 0)
        assert max(float(np.max(np.abs(a[1][k] - b[1][k])) / np.max(np.abs(b[1][k]))) for a, b in zip(got, plain) for k in range(L)) > 10 * TOL
    finally:
        seq.close()


# ---- host pushes, the protocol, one frame ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 2), (2, 1)])
def test_host_push_is_device_push(hipctx, R, S):
    W, H = 40, 28
    want, moved = plain_reference(hipctx, W, H, R, S)
    seq = hipctx.sequence(W, H, 60, S, R, ts.params(1.0, 1))
    try:
        seq.set_prefilter(FACTOR)
        ts.check_against(ts.run(seq, ts.frames_of(W, H), S, host=True), want, S)
        assert seq.prefilter_info() == (T, sum(moved))
        assert seq.info()["bytes_uploaded"] == T * W * H * (3 + 1 + 60 + 6) * 4
    finally:
        seq.close()
    want, moved = mode_reference(hipctx, MODE, W, H, R, S)
    L = tm.MODES[MODE]["L"]
    seq = tm.make_sequence(hipctx, MODE, W, H, 0, S, R, tm.params(MODE))
    try:
        seq.set_prefilter(FACTOR)
        got = tm.run(seq, [tm.mode_frame(f, MODE) for f in tm.frames_of(W, H)], S, L, host=True, with_masks=False)
        tm.check_against(got, want)
        assert seq.prefilter_info() == (T, sum(moved))
    finally:
        seq.close()


def test_protocol_and_a_sequence_of_one_frame(hipctx):
    import bcd_amd.hip as bh
    W, H, S = 40, 28, 2
    fr = [ts.dev(f) for f in ts.frames_of(W, H)]
    prm = ts.params(1.0, 1)
    seq = hipctx.sequence(W, H, 60, S, 1, prm)
    try:
        assert seq.prefilter_info() == (0, 0)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(bh.BcdHipError):
                seq.set_prefilter(bad)
        seq.set_prefilter(FACTOR)
        seq.set_prefilter(1.5)                                                   # (still no frame: accepted)
        seq.set_prefilter(FACTOR)
        seq.push(*fr[0])
        with pytest.raises(bh.BcdHipError) as e:
            seq.set_prefilter(3.0)
        assert "holds no frame" in str(e.value)
        # T = 1: the single-frame call on the filtered frame
        seq.end()
        idx, out = seq.pop()
        f0, moved = filtered_plain(hipctx, fr[0])
        want = hipctx.denoise(*f0, S, prm)
        assert idx == 0 and ts.rel_linf(out.cpu().numpy(), want.cpu().numpy()) <= TOL
        assert seq.prefilter_info() == (1, moved)
        with pytest.raises(bh.BcdHipError):
            seq.set_prefilter(0.0)                                               # popped, but not reset
        seq.reset()
        seq.set_prefilter(0.0)                                                   # after reset: accepted
        seq.push(*fr[0])
        seq.end()
        idx, out = seq.pop()
        assert ts.rel_linf(out.cpu().numpy(), hipctx.denoise(*fr[0], S, prm).cpu().numpy()) <= TOL and seq.prefilter_info() == (0, 0)
    finally:
        seq.close()
    # the mode: T = 1 is the single-frame call of the mode on the filtered frame
    d = tm.mode_frame(tm.frames_of(W, H)[0], MODE, tm.t)
    seq = tm.make_sequence(hipctx, MODE, W, H, 0, S, 2, tm.params(MODE))
    try:
        seq.set_prefilter(FACTOR)
        seq.push(*d)
        seq.end()
        idx, outs = seq.pop()
        fd, moved = filtered_mode(hipctx, d)
        want = tm.frame_call(hipctx, MODE, [fd], 0, [], S, tm.params(MODE))
        for o, w in zip(outs, want):
            assert ts.rel_linf(o.cpu().numpy(), w.cpu().numpy()) <= TOL
        assert seq.prefilter_info() == (1, moved)
    finally:
        seq.close()


# ---- the C++ class and the command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (2, 2)])
def test_the_cpp_class_with_the_switch(hipctx, R, S):
    import bcd_amd.core as core
    W, H, n = 40, 28, 4
    prm = ts.params(1.0, 1)
    want, _ = plain_reference(hipctx, W, H, R, S, n)
    ok, got = core.denoise_sequence(ts.frames_of(W, H)[:n], radius=R, nscales=S, seed=prm.order_seed, prefilter_frames=FACTOR)
    assert ok and len(got) == n
    for g, w in zip(got, want):
        assert ts.rel_linf(g, w[0]) <= TOL
    assert not core.denoise_sequence(ts.frames_of(W, H)[:n], radius=R, nscales=S, prefilter_without_switch=FACTOR)[0]     # the factor without the switch: refused as before
    # in a mode
    mwant, _ = mode_reference(hipctx, MODE, W, H, R, S, n)
    fr = tm.frames_of(W, H)[:n]
    L, F = tm.MODES[MODE]["L"], tm.MODES[MODE]["F"]
    frames = [(f["layers"][0][0], f["ns"], None, f["layers"][0][1]) for f in fr]
    ok, got = core.denoise_sequence(frames, radius=R, nscales=S, seed=1234, tau=tm.params(MODE).hist_dist_threshold, layers=[f["layers"][1:L] for f in fr],
                                    features=[np.ascontiguousarray(f["feat"][..., :F]) for f in fr], feature_floors=tm.gc.FLOORS[:F], feature_threshold=tm.gc.TAU_G,
                                    var_floor=tm.xc.VAR_FLOOR, prefilter_frames=FACTOR)
    assert ok
    for g, w in zip(got, mwant):
        for k in range(L):
            assert ts.rel_linf(g[k], w[0][k]) <= TOL


def test_bcd_cli_sequence_prefilter_frames_end_to_end(hipctx, tmp_path):
    """bcd_cli --sequence-in ... --prefilter-frames with the default -p 1 over four 40x28 frames: every output is the Python Sequence's frame with the
    prefilter after the half-float EXR round trip"""
    import torch
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 40, 28
    frames = [core.synthetic_scene(W, H, 16, seed, 0.15, 0.02) for seed in (21, 22, 23, 24)]
    on_disk = []
    for k, (col, ns, hist, cov) in enumerate(frames):
        stem = str(tmp_path / ("shot.%04d" % (k + 7)))
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        core.write_exr(stem + "_cov.exr", cov, True)
        on_disk.append((core.read_exr(stem + ".exr", False), ns, hist, cov))      # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    args = [exe, "--sequence-in", str(tmp_path / "shot.%04d.exr"), "--sequence-out", str(tmp_path / "clean.%04d.exr"), "--first", "7", "--last", "10",
            "--temporal-radius", "2", "-s", "2", "-m", "1", "--seed", "5"]
    r = subprocess.run(args + ["--prefilter-frames"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    prm = bh.default_params(m=1.0, seed=5)
    seq = hipctx.sequence(W, H, 60, 2, 2, prm)
    try:
        seq.set_prefilter(FACTOR)                                                # (--p-factor's default)
        want = [g[1] for g in ts.run(seq, [ts.dev(f) for f in on_disk], 2, with_masks=False)]
        assert seq.prefilter_info()[1] > 0
        seq.reset()
        seq.set_prefilter(0.0)
        plain = [g[1] for g in ts.run(seq, [ts.dev(f) for f in on_disk], 2, with_masks=False)]
    finally:
        seq.close()
    for k in range(4):
        w = hipctx.zero_bad_values(torch.from_numpy(want[k]).cuda()).cpu().numpy()
        got = core.read_exr(str(tmp_path / ("clean.%04d.exr" % (k + 7))), False)
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), k
    # -p 0 beside the flag: accepted, and nothing is filtered
    r = subprocess.run(args + ["--prefilter-frames", "-p", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    w = hipctx.zero_bad_values(torch.from_numpy(plain[1]).cuda()).cpu().numpy()
    got = core.read_exr(str(tmp_path / "clean.0008.exr"), False)
    assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w)
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)        # without the flag: today's message
    assert r.returncode == 1 and "add -p 0" in r.stdout
