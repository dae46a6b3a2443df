"""GPU tests of the denoising of a frame with similar patches from neighbouring frames (bcd_hip_denoise_temporal, bcd_hip_denoise_temporal_host)
against the NumPy composition of tests/temporal_ref.py (similarity_ref, marking_ref, pyramid_ref and the float64 estimate).

  * the whole call at 40x28 and 52x36, 1 and 2 scales, F = 1 and 2, -m 1 -r 1 and -m 0, frames from oracle_lib.synth_inputs at 32 spp with one seed per
    frame: processed / fallback / similar_total of every scale equal the reference's, the frame is within 1e-4 relative L-inf of it (the project's frame
    bar); the composition of the stage calls (Context.denoise_temporal_stages) is the one-scale call;
  * F = 0 against bcd_hip_denoise at 1 and 2 scales: the same per-scale figures, the frame within the same bar;
  * the host entry point returns the device call's frame;
  * every refusal of the frame call, then a successful call on the same context;
  * benefit: three realisations of one scene at 16 spp; the RMSE against the noise-free base of the F = 2 result is below that of bcd_hip_denoise on the
    middle frame.  Size and sigma (52x36, 0.5) were chosen so that the NumPy reference alone satisfies the inequality (CPU: ratio 0.69)."""
import numpy as np
import pytest

import marking_ref as mr
import oracle_lib as ol
import temporal_ref as tr

pytestmark = pytest.mark.gpu

TOL = 1e-4        # relative to the frame's maximum (README / DESIGN 6)
SEEDS = (1234, 77, 4321)


def dev(frame):
    import torch
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in frame)


def rel_linf(got, want):
    """relative L-inf over the values that are finite in `want`; the non-finite patterns must agree"""
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), "non-finite pattern differs"
    return float(np.max(np.abs(np.where(ok, got, 0) - np.where(ok, want, 0))) / np.max(np.abs(np.where(ok, want, 0))))


_frames = {}


def frames_of(W, H, spp=32, sigma=0.35, spikes=0.01):
    key = (W, H, spp, sigma, spikes)
    if key not in _frames:
        out = [ol.synth_inputs(W, H, spp, seed, sigma, spikes) for seed in SEEDS]
        _frames[key] = ([f[:4] for f in out], out[0][4])
    return _frames[key]


def params(m, r, seed=1234):
    import bcd_amd.hip as bh
    return bh.default_params(m=m, random_order=r, seed=seed)


def reference(W, H, F, S, m, r, seed=1234):
    """(frame, per-scale stats) of the NumPy composition, once per configuration"""
    import bcd_amd.hip as bh
    key = (W, H, F, S, m, r, seed)
    if key not in _refs:
        fr, _ = frames_of(W, H)
        orders, draws, ws, hs = [], [], W, H
        for s in range(S):
            sd = bh.scale_seed(seed, s)
            orders.append(bh.visit_order(ws, hs, 1, r, sd))
            draws.append(mr.skip_draw(ws, hs, m, sd))
            ws, hs = ws // 2, hs // 2
        _refs[key] = tr.denoise_multiscale(fr[0], fr[1:1 + F], S, 1, 6, 1.0, 1e-8, orders, draws)
    return _refs[key]


_refs = {}


def stats_of(ctx, S):
    return [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total) for s in (ctx.stats(k) for k in range(S))]


@pytest.mark.parametrize("W,H", [(40, 28), (52, 36)])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("m,r", [(1.0, 1), (0.0, 0)])
def test_whole_call_against_the_reference_composition(hipctx, W, H, S, F, m, r):
    fr, _ = frames_of(W, H)
    prm = params(m, r)
    out = hipctx.denoise_temporal(*dev(fr[0]), [dev(f) for f in fr[1:1 + F]], S, prm)
    hipctx.synchronize()
    want, wstats = reference(W, H, F, S, m, r)
    stats = stats_of(hipctx, S)
    assert stats == wstats, (stats, wstats)
    assert all(s["similar_total"] > 0 and s["processed"] > 0 for s in stats)
    assert [(hipctx.stats(k).width, hipctx.stats(k).height) for k in range(S)] == [(W >> k, H >> k) for k in range(S)]
    e = rel_linf(out.cpu().numpy(), want)
    print("temporal %dx%d S=%d F=%d m=%g: %s, against float64 %.2e" % (W, H, S, F, m, stats, e))
    assert e <= TOL, e


def test_stage_composition_is_the_one_scale_call(hipctx):
    W, H, F = 52, 36, 2
    fr, _ = frames_of(W, H)
    prm = params(1.0, 1)
    out, stats = hipctx.denoise_temporal_stages(*dev(fr[0]), [dev(f) for f in fr[1:1 + F]], prm)
    want, wstats = reference(W, H, F, 1, 1.0, 1)
    assert [stats] == wstats
    assert rel_linf(out.cpu().numpy(), want) <= TOL


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("m,r", [(1.0, 1), (0.0, 0)])
def test_no_neighbour_is_the_plain_call(hipctx, S, m, r):
    """F = 0: the call delegates to bcd_hip_denoise -- the same per-scale figures, similarity path included, and the frame within the bar"""
    W, H = 52, 36
    fr, _ = frames_of(W, H)
    prm = params(m, r)
    d = dev(fr[0])
    out = hipctx.denoise_temporal(*d, [], S, prm)
    hipctx.synchronize()
    got = [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(S))]
    plain = hipctx.denoise(*d, S, prm)
    hipctx.synchronize()
    assert got == [(s.processed, s.fallback, s.similar_total, s.similarity_path) for s in (hipctx.stats(k) for k in range(S))]
    assert rel_linf(out.cpu().numpy(), plain.cpu().numpy()) <= TOL


@pytest.mark.parametrize("S,F", [(1, 1), (2, 2)])
def test_host_entry_point_returns_the_device_call_s_frame(hipctx, S, F):
    W, H = 40, 28
    fr, _ = frames_of(W, H)
    prm = params(1.0, 1)
    want = hipctx.denoise_temporal(*dev(fr[0]), [dev(f) for f in fr[1:1 + F]], S, prm)
    hipctx.synchronize()
    wstats = stats_of(hipctx, S)
    got = hipctx.denoise_temporal_host(*fr[0], fr[1:1 + F], S, prm)
    assert stats_of(hipctx, S) == wstats
    assert rel_linf(got, want.cpu().numpy()) <= TOL
    plain = hipctx.denoise_temporal_host(*fr[0], [], S, prm)       # no neighbour: bcd_hip_denoise_host
    ref = hipctx.denoise(*dev(fr[0]), S, prm)
    hipctx.synchronize()
    assert rel_linf(plain, ref.cpu().numpy()) <= TOL


def test_refusals_of_the_frame_call_then_a_successful_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    W, H, F = 40, 28, 1
    fr, _ = frames_of(W, H)
    d, nb = dev(fr[0]), [dev(fr[1])]
    prm = params(1.0, 1)

    def refused(call, code=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert code is None or ("rc=%d" % code) in str(e.value) or "support" in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                 # any other geometry: BCD_HIP_EUNSUPPORTED
        p = bh.default_params(m=1.0, random_order=1, w=w, b=b)
        refused(lambda: hipctx.denoise_temporal(*d, nb, 1, p), -4)
    refused(lambda: hipctx.denoise_temporal(*d, nb * 5, 1, prm))     # five neighbours
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    refused(lambda: hipctx.denoise_temporal(*d, nb, 1, prm, out=d[0]))               # the output is an input
    refused(lambda: hipctx.denoise_temporal(*d, nb, 1, prm, out=nb[0][0]))           # ... of a neighbour
    refused(lambda: hipctx.denoise_temporal(*d, nb, 9, prm))         # too many scales for the image
    L = bh.lib()
    one = (bh.Frame * 1)()
    one[0].d_colors, one[0].d_nsamples, one[0].d_histograms, one[0].d_covariances = (t.data_ptr() for t in nb[0])
    ptrs = [t.data_ptr() for t in d]
    call = lambda frames, n, colp=ptrs[0]: L.bcd_hip_denoise_temporal(hipctx.h, colp, ptrs[1], ptrs[2], ptrs[3], frames, n, W, H, 60, 1, C.byref(prm), out.data_ptr())
    one[0].reserved = 1
    assert call(one, 1) == -1                                        # a non-NULL reserved pointer
    one[0].reserved = None
    assert call(one, -1) == -1 and call(one, 5) == -1                # nb_neighbours outside 0 .. 4
    assert call(None, 1) == -1                                       # no neighbour list
    assert call(one, 1, None) == -1                                  # a null image
    one[0].d_histograms = None
    assert call(one, 1) == -1                                        # a null image in a neighbour
    assert float(out.abs().sum()) == 0.0                             # nothing ran
    got = hipctx.denoise_temporal(*d, nb, 1, prm)
    hipctx.synchronize()
    want, wstats = reference(W, H, F, 1, 1.0, 1)
    assert stats_of(hipctx, 1) == wstats and rel_linf(got.cpu().numpy(), want) <= TOL


def test_neighbours_lower_the_error_against_the_noise_free_base(hipctx):
    W, H = 52, 36
    fr, base = frames_of(W, H, spp=16, sigma=0.5, spikes=0.0)
    prm = params(1.0, 1)
    mid = dev(fr[1])
    plain = hipctx.denoise(*mid, 1, prm)
    hipctx.synchronize()
    out, stats = hipctx.denoise_temporal_stages(*mid, [dev(fr[0]), dev(fr[2])], prm)
    rmse = lambda x: float(np.sqrt(np.mean((x.cpu().numpy()[1:-1, 1:-1].astype(np.float64) - base[1:-1, 1:-1]) ** 2)))
    print("benefit 52x36 16 spp sigma 0.5: RMSE plain %.5f, F = 2 %.5f, ratio %.3f" % (rmse(plain), rmse(out), rmse(out) / rmse(plain)))
    assert rmse(out) < rmse(plain)


@pytest.mark.parametrize("S,F", [(1, 1), (2, 2)])
def test_cpp_class_returns_the_device_call_s_frame(hipctx, S, F):
    """bcd::Denoiser / bcd::MultiscaleDenoiser::addNeighbourFrame: the device call's frame; clearNeighbourFrames() gives the plain denoise() again"""
    import bcd_amd.core as core
    W, H = 40, 28
    fr, _ = frames_of(W, H)
    prm = params(1.0, 1)
    want = hipctx.denoise_temporal(*dev(fr[0]), [dev(f) for f in fr[1:1 + F]], S, prm).cpu().numpy()
    plain = hipctx.denoise(*dev(fr[0]), S, prm).cpu().numpy()
    ok, got = core.denoise_temporal(*fr[0], fr[1:1 + F], S, seed=prm.order_seed)
    assert ok and rel_linf(got, want) <= TOL
    assert rel_linf(got, plain) > 10 * TOL                            # (the neighbours did something)
    ok, got = core.denoise_temporal(*fr[0], fr[1:1 + F], S, seed=prm.order_seed, after_clear=True)
    assert ok and rel_linf(got, plain) <= TOL
    ok, _ = core.denoise_temporal(*fr[0], [fr[1]] * 5, S, seed=prm.order_seed)          # five neighbours: refused, denoise() returns false
    assert not ok
    ok, _ = core.denoise_temporal(*fr[0], fr[1:2], S, b=12, seed=prm.order_seed)        # another geometry
    assert not ok


def test_bcd_cli_neighbour_end_to_end(hipctx, tmp_path):
    """bcd_cli --neighbour twice: the output is the device call's frame after the half-float EXR round trip (the comparison of the other CLI tests)"""
    import os
    import subprocess
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    W, H = 72, 56
    frames = [core.synthetic_scene(W, H, 16, seed, 0.15, 0.02) for seed in (21, 22, 23)]
    on_disk = []
    for k, (col, ns, hist, cov) in enumerate(frames):
        stem = str(tmp_path / ("frame%d" % k))
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
        core.write_exr(stem + "_cov.exr", cov, True)
        on_disk.append((core.read_exr(stem + ".exr", False), ns, hist, cov))      # (colours go through half precision on disk)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    r = subprocess.run([exe, "-i", str(tmp_path / "frame1.exr"), "-o", out_path, "-p", "0", "-s", "2", "-m", "1", "--seed", "5",
                        "--neighbour", str(tmp_path / "frame0.exr"), "--neighbour", str(tmp_path / "frame2.exr")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = hipctx.denoise_temporal(*dev(on_disk[1]), [dev(on_disk[0]), dev(on_disk[2])], 2, bh.default_params(m=1.0, seed=5))
    w = hipctx.zero_bad_values(want).cpu().numpy()
    got = core.read_exr(out_path, False)
    assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w)
    r = subprocess.run([exe, "-i", str(tmp_path / "frame1.exr"), "-o", out_path, "-p", "0", "-b", "4", "--neighbour", str(tmp_path / "frame0.exr")],
                       capture_output=True, text=True)
    assert r.returncode != 0                                         # another geometry: refused
