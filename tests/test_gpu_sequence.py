"""GPU tests of the sequence object (bcd_hip_sequence_*, Context.sequence; DESIGN 16, "Sequences") against the per-frame call it is defined by:
frame t of T frames is what Context.denoise_temporal returns for frame t with the neighbours max(0, t - R) .. min(T - 1, t + R) except t in ascending order.

  * T = 5 frames (oracle_lib.synth_inputs, one seed per frame, 32 spp) at 40x28 and 52x36, R = 1 and 2, 1 and 2 scales, -m 1 -r 1 and -m 0 -r 0: per popped
    frame processed / fallback / similar_total of every scale equal the per-frame call's, the frame is within the project's frame bar of it (1e-4 relative
    L-inf: TOL of tests/test_gpu_temporal.py), last_masks of every neighbour at scale 0 equal similarity_masks_cross on the full-resolution
    frames bit for bit (neighbour 0: similarity_masks), the frame indices come in order; info: pyramids built = T, cross passes computed = transposed = the
    unordered pairs within R (4 at R = 1, 7 at R = 2); with set_reuse(0) nothing is transposed and frames, stats and masks are the same;
  * host push and pop return the device path's frames, bytes uploaded = T x the bytes of one frame;
  * protocol: a pop before ready, a push beyond the ring, end with fewer than R + 1 frames, T = 1 against Context.denoise, reset and a second identical run,
    two sequences of different sizes on one context one after the other, a plain denoise_temporal after a sequence against a fresh context's;
  * core.denoise_sequence, bcd::SequenceDenoiser and bcd_cli --sequence-in on four 40x28 frames against the Python Sequence (the CLI with the bound of the
    other CLI tests for the half-float EXR round trip);
  * every refusal of create, push and pop, then a successful run on the same context."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

TOL = 1e-4        # relative to the frame's maximum (TOL of tests/test_gpu_temporal.py; README / DESIGN 6)
SEEDS = (1234, 77, 4321, 99, 2024)
T = len(SEEDS)


def dev(frame):
    import torch
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in frame)


def rel_linf(got, want):
    """relative L-inf over the values that are finite in `want`; the non-finite patterns must agree"""
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "non-finite pattern differs"
    return float(np.max(np.abs(np.where(ok, got, 0) - np.where(ok, want, 0))) / np.max(np.abs(np.where(ok, want, 0))))


_frames = {}


def frames_of(W, H):
    if (W, H) not in _frames:
        _frames[(W, H)] = [ol.synth_inputs(W, H, 32, seed)[:4] for seed in SEEDS]
    return _frames[(W, H)]


def params(m, r, seed=1234):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=seed)


def stats_of(ctx, S):
    return [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total) for s in (ctx.stats(k) for k in range(S))]


def neighbours_of(t, R, n):
    return [f for f in range(max(0, t - R), min(n - 1, t + R) + 1) if f != t]


_refs = {}


def reference(ctx, W, H, R, S, m, r, n=T):
    """per frame of the first n frames (frame, per-scale stats, the scale-0 masks and counts of the in-frame set and of every neighbour) of the per-frame
    calls, once per configuration"""
    key = (W, H, R, S, m, r, n)
    if key not in _refs:
        fr = [dev(f) for f in frames_of(W, H)[:n]]
        prm = params(m, r)
        out = []
        for t in range(n):
            nbs = neighbours_of(t, R, n)
            if nbs:
                frame = ctx.denoise_temporal(*fr[t], [fr[f] for f in nbs], S, prm)
            else:
                frame = ctx.denoise(*fr[t], S, prm)
            ctx.synchronize()
            st = stats_of(ctx, S)
            masks = [ctx.similarity_masks(fr[t][2], fr[t][1], 1, 6, prm.hist_dist_threshold)]
            masks += [ctx.similarity_masks_cross(fr[t][2], fr[t][1], fr[f][2], fr[f][1], 1, 6, prm.hist_dist_threshold) for f in nbs]
            out.append((frame.cpu().numpy(), st, [(a.cpu().numpy(), b.cpu().numpy()) for a, b in masks]))
        _refs[key] = out
    return _refs[key]


def run(seq, frames, S, host=False, with_masks=True):
    """the push / pop protocol over `frames` -> [(index, frame, per-scale stats, scale-0 masks of the in-frame set and every neighbour)]"""
    ctx, out, n = seq.ctx, [], len(frames)

    def drain():
        while seq.ready():
            idx, frame = seq.pop_host() if host else seq.pop()
            st = stats_of(ctx, S)
            masks = []
            nb = len(neighbours_of(idx, seq.radius, n))
            if with_masks and nb:
                masks = [tuple(a.cpu().numpy() for a in seq.last_masks(k, 0)) for k in range(nb + 1)]
            out.append((idx, frame if host else frame.cpu().numpy(), st, masks))

    for k, f in enumerate(frames):
        (seq.push_host if host else seq.push)(*f)
        if k == n - 1:
            seq.end()
        drain()
    assert seq.ready() == 0
    return out


def check_against(got, want, S):
    assert [g[0] for g in got] == list(range(len(want)))                      # the frame indices come in order
    worst = 0.0
    for (idx, frame, st, masks), (wframe, wst, wmasks) in zip(got, want):
        assert st == wst, (idx, st, wst)
        assert all(s["similar_total"] > 0 and s["processed"] > 0 for s in st)
        e = rel_linf(frame, wframe)
        worst = max(worst, e)
        assert e <= TOL, (idx, e)
        if masks:
            assert len(masks) == len(wmasks)
            for k, ((m, c), (wm, wc)) in enumerate(zip(masks, wmasks)):
                assert np.array_equal(m, wm) and np.array_equal(c, wc), "frame %d, neighbour %d: the masks differ" % (idx, k)
    return worst


PAIRS = {1: 4, 2: 7}      # unordered pairs of T = 5 frames within R


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("m,r", [(1.0, 1), (0.0, 0)])
def test_sequence_is_the_per_frame_call(hipctx, W, H, R, S, m, r):
    want = reference(hipctx, W, H, R, S, m, r)
    fr = [dev(f) for f in frames_of(W, H)]
    seq = hipctx.sequence(W, H, 60, S, R, params(m, r))
    try:
        got = run(seq, fr, S)
        worst = check_against(got, want, S)
        info = seq.info()
        print("sequence %dx%d R=%d S=%d m=%g: worst frame deviation from the per-frame call %.2e; %s" % (W, H, R, S, m, worst, info))
        assert info["frames_pushed"] == info["frames_popped"] == info["pyramids_built"] == T
        assert info["cross_computed"] == info["cross_transposed"] == PAIRS[R]
        assert info["bytes_uploaded"] == 0 and info["device_bytes"] > 0
    finally:
        seq.close()


@pytest.mark.parametrize("W,H,R,S", [(40, 28, 1, 1), (52, 36, 2, 2)])
def test_without_reuse_every_pair_is_searched_from_both_sides(hipctx, W, H, R, S):
    want = reference(hipctx, W, H, R, S, 1.0, 1)
    seq = hipctx.sequence(W, H, 60, S, R, params(1.0, 1))
    try:
        seq.set_reuse(False)
        got = run(seq, [dev(f) for f in frames_of(W, H)], S)
        check_against(got, want, S)
        info = seq.info()
        assert info["cross_transposed"] == 0 and info["cross_computed"] == 2 * PAIRS[R] and info["pyramids_built"] == T
    finally:
        seq.close()


@pytest.mark.parametrize("R,S", [(1, 2), (2, 1)])
def test_host_push_and_pop_return_the_device_path_s_frames(hipctx, R, S):
    W, H = 40, 28
    want = reference(hipctx, W, H, R, S, 1.0, 1)
    seq = hipctx.sequence(W, H, 60, S, R, params(1.0, 1))
    try:
        got = run(seq, frames_of(W, H), S, host=True)
        check_against(got, want, S)
        info = seq.info()
        assert info["bytes_uploaded"] == T * W * H * (3 + 1 + 60 + 6) * 4
        assert info["cross_computed"] == info["cross_transposed"] == PAIRS[R]
    finally:
        seq.close()


def test_protocol(hipctx):
    import bcd_amd.hip as bh
    W, H, R, S = 40, 28, 2, 1
    fr = [dev(f) for f in frames_of(W, H)]
    prm = params(1.0, 1)
    seq = hipctx.sequence(W, H, 60, S, R, prm)
    try:
        def refused(call, word):
            with pytest.raises(bh.BcdHipError) as e:
                call()
            assert word in str(e.value), str(e.value)

        refused(seq.pop, "not ready")                                         # nothing pushed
        seq.push(*fr[0])
        seq.push(*fr[1])
        assert seq.ready() == 0
        refused(seq.pop, "not ready")                                         # frame 0 needs frame 2
        seq.push(*fr[2])
        assert seq.ready() == 1
        refused(lambda: seq.push(*fr[3]), "pop first")                        # frame 3 > next_pop + R
        assert seq.info()["frames_pushed"] == 3
        idx, _ = seq.pop()
        assert idx == 0
        seq.push(*fr[3])
        assert seq.ready() == 1
        # reset, then end with fewer than R + 1 frames: the two frames are each other's only neighbours
        seq.reset()
        assert seq.ready() == 0 and seq.info()["frames_pushed"] == 0 and seq.info()["cross_computed"] == 0
        want2 = reference(hipctx, W, H, R, S, 1.0, 1, n=2)
        got2 = run(seq, fr[:2], S)
        check_against(got2, want2, S)
        refused(lambda: seq.push(*fr[2]), "ended")                            # after end
        assert seq.info()["cross_computed"] == 1 and seq.info()["cross_transposed"] == 1
        # T = 1 against Context.denoise
        seq.reset()
        got1 = run(seq, fr[:1], S)
        plain = hipctx.denoise(*fr[0], S, prm)
        hipctx.synchronize()
        assert got1[0][2] == stats_of(hipctx, S) and rel_linf(got1[0][1], plain.cpu().numpy()) <= TOL
        refused(lambda: seq.last_masks(0, 0), "no neighbour")
        # reset and two identical runs
        want = reference(hipctx, W, H, R, S, 1.0, 1)
        for _ in range(2):
            seq.reset()
            check_against(run(seq, fr, S), want, S)
            assert seq.info()["cross_computed"] == seq.info()["cross_transposed"] == PAIRS[R]
        held = seq.info()["device_bytes"]
        seq.reset()
        run(seq, fr, S, with_masks=False)
        assert seq.info()["device_bytes"] == held                             # nothing is allocated once the buffers exist
    finally:
        seq.close()
    refused(lambda: seq.ready(), "closed")
    # another sequence of another size on the same context, then the per-frame call against a fresh context's
    W2, H2 = 52, 36
    seq2 = hipctx.sequence(W2, H2, 60, 2, 1, prm)
    try:
        check_against(run(seq2, [dev(f) for f in frames_of(W2, H2)], 2), reference(hipctx, W2, H2, 1, 2, 1.0, 1), 2)
    finally:
        seq2.close()
    after = hipctx.denoise_temporal(*fr[1], [fr[0], fr[2]], 2, prm)
    hipctx.synchronize()
    st_after = stats_of(hipctx, 2)
    fresh = bh.Context(0)
    try:
        want = fresh.denoise_temporal(*fr[1], [fr[0], fr[2]], 2, prm)
        fresh.synchronize()
        assert st_after == stats_of(fresh, 2) and rel_linf(after.cpu().numpy(), want.cpu().numpy()) <= TOL
    finally:
        fresh.close()


def test_refusals_of_create_push_and_pop_then_a_successful_run(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    L = bh.lib()
    W, H, R, S = 40, 28, 1, 1
    fr = [dev(f) for f in frames_of(W, H)]
    prm = params(1.0, 1)
    err = lambda: L.bcd_hip_last_error(hipctx.h).decode()
    h = C.c_void_p()
    create = lambda w, hh, d, s, r, p, out=C.byref(h): L.bcd_hip_sequence_create(hipctx.h, w, hh, d, s, r, p, out)
    EINVAL, EUNSUPPORTED = -1, -4
    assert create(W, H, 60, S, 0, C.byref(prm)) == EINVAL and "radius" in err()
    assert create(W, H, 60, S, 3, C.byref(prm)) == EINVAL and "radius" in err()
    assert create(0, H, 60, S, R, C.byref(prm)) == EINVAL and create(W, H, 0, S, R, C.byref(prm)) == EINVAL
    assert create(W, H, 60, 0, R, C.byref(prm)) == EINVAL and create(W, H, 60, 9, R, C.byref(prm)) == EINVAL          # too many scales for the image
    assert create(W, H, 60, S, R, None) == EINVAL and create(W, H, 60, S, R, C.byref(prm), None) == EINVAL
    assert create(W, H, 300, S, R, C.byref(prm)) == EUNSUPPORTED
    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                          # any other geometry
        assert create(W, H, 60, S, R, C.byref(bh.default_params(m=1.0, random_order=1, w=w, b=b))) == EUNSUPPORTED
    assert "patch radius 1 and search radius 6" in err()
    assert not h.value
    assert create(W, H, 60, S, R, C.byref(prm)) == 0 and h.value
    try:
        out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        idx = C.c_int64(-7)
        torch.cuda.synchronize()
        p = [t.data_ptr() for t in fr[0]]
        for k in range(4):                                                    # a null image
            q = list(p)
            q[k] = None
            assert L.bcd_hip_sequence_push(h, *q) == EINVAL and "null" in err()
            assert L.bcd_hip_sequence_push_host(h, *q) == EINVAL and "null" in err()
        assert L.bcd_hip_sequence_pop(h, out.data_ptr(), C.byref(idx)) == EINVAL and "not ready" in err()
        assert L.bcd_hip_sequence_push(h, *p) == 0
        assert L.bcd_hip_sequence_pop(h, out.data_ptr(), C.byref(idx)) == EINVAL and "not ready" in err()
        assert L.bcd_hip_sequence_pop_host(h, None, C.byref(idx)) == EINVAL
        assert L.bcd_hip_sequence_push(h, *[t.data_ptr() for t in fr[1]]) == 0
        assert L.bcd_hip_sequence_pop(h, None, C.byref(idx)) == EINVAL and "null" in err()
        assert L.bcd_hip_sequence_last_masks(h, 0, 0, out.data_ptr(), None) == EINVAL and "popped" in err()
        assert L.bcd_hip_sequence_info(h, None) == EINVAL
        assert idx.value == -7 and float(out.abs().sum()) == 0.0              # nothing ran
        assert L.bcd_hip_sequence_pop(h, out.data_ptr(), None) == 0           # (the index is optional)
        mask = torch.zeros((H, W, 6), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert L.bcd_hip_sequence_last_masks(h, 2, 0, mask.data_ptr(), None) == EINVAL and "neighbour" in err()
        assert L.bcd_hip_sequence_last_masks(h, 1, 1, mask.data_ptr(), None) == EINVAL and "scale" in err()
        assert L.bcd_hip_sequence_last_masks(h, 1, 0, None, None) == EINVAL
        assert L.bcd_hip_sequence_last_masks(h, 1, 0, mask.data_ptr(), None) == 0 and bool(mask.any())                # (the counts are optional)
    finally:
        L.bcd_hip_sequence_destroy(h)
    for fn in (L.bcd_hip_sequence_end, L.bcd_hip_sequence_reset):
        assert fn(None) == EINVAL
    assert L.bcd_hip_sequence_ready(None) == 0 and L.bcd_hip_sequence_push(None, *p) == EINVAL
    L.bcd_hip_sequence_destroy(None)
    seq = hipctx.sequence(W, H, 60, S, R, prm)
    try:
        check_against(run(seq, fr, S), reference(hipctx, W, H, R, S, 1.0, 1), S)
    finally:
        seq.close()


def python_sequence(hipctx, frames, R, S, prm):
    seq = hipctx.sequence(frames[0][2].shape[1], frames[0][2].shape[0], frames[0][2].shape[2], S, R, prm)
    try:
        return [g[1] for g in run(seq, [dev(f) for f in frames], S, with_masks=False)]
    finally:
        seq.close()


@pytest.mark.parametrize("R,S", [(1, 1), (2, 2)])
def test_core_denoise_sequence_and_the_cpp_class_return_the_python_sequence_s_frames(hipctx, R, S):
    """core.denoise_sequence drives bcd::SequenceDenoiser (libbcdcore.so) through the host push and pop"""
    import bcd_amd.core as core
    W, H = 40, 28
    frames = frames_of(W, H)[:4]
    prm = params(1.0, 1)
    want = python_sequence(hipctx, frames, R, S, prm)
    ok, got = core.denoise_sequence(frames, radius=R, nscales=S, seed=prm.order_seed)
    assert ok and len(got) == 4
    for g, w in zip(got, want):
        assert rel_linf(g, w) <= TOL
    assert rel_linf(got[1], hipctx.denoise(*dev(frames[1]), S, prm).cpu().numpy()) > 10 * TOL      # (the neighbours did something)
    ok, _ = core.denoise_sequence(frames, radius=R, nscales=S, unsupported=32)                  # a second frame of another size
    assert not ok


def test_bcd_cli_sequence_end_to_end(hipctx, tmp_path):
    """bcd_cli --sequence-in over four 40x28 frames: every output is the Python Sequence's frame after the half-float EXR round trip (the comparison of the
    other CLI tests)"""
    import os
    import subprocess
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
    r = subprocess.run([exe, "--sequence-in", str(tmp_path / "shot.%04d.exr"), "--sequence-out", str(tmp_path / "clean.%04d.exr"), "--first", "7", "--last", "10",
                        "--temporal-radius", "2", "-p", "0", "-s", "2", "-m", "1", "--seed", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = python_sequence(hipctx, on_disk, 2, 2, bh.default_params(m=1.0, seed=5))
    import torch
    for k in range(4):
        w = hipctx.zero_bad_values(torch.from_numpy(want[k]).cuda()).cpu().numpy()
        got = core.read_exr(str(tmp_path / ("clean.%04d.exr" % (k + 7))), False)
        assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w), k
    r = subprocess.run([exe, "--sequence-in", str(tmp_path / "shot.%04d.exr"), "--sequence-out", str(tmp_path / "clean.%04d.exr"), "--first", "7", "--last", "11", "-p", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "shot.0011.exr" in r.stdout                       # a frame that is not there
