"""GPU tests of the motion fields in the host library and the command-line tool (bcd::Denoiser / bcd::MultiscaleDenoiser::setNeighbourMotion, bcd_cli
--neighbour-motion), at 64x44 on the frames and fields of tests/motion_cases.py, against the device calls that tests/test_gpu_motion.py holds to the reference.

  * setNeighbourMotion through core.denoise_temporal(motions=...): the device call's frame at 1 and 3 scales, with one neighbour and with two of which one has
    no field; a list of None is the plain call; clearNeighbourFrames() clears the fields with the frames;
  * beside colour layers (core.denoise_temporal_layers(motions=...)): the layered device call's layers;
  * bcd_cli --neighbour-motion with a two-channel EXR and with a wider one (the first two channels count): the device call's frame after the half-float round
    trip of the colours; before any --neighbour, and in another size than the frame's, it is an argument error."""
import os
import subprocess

import numpy as np
import pytest

import motion_cases as mc
import temporal_layers_cases as tl
from test_gpu_temporal import TOL, dev, rel_linf

pytestmark = pytest.mark.gpu

W, H = mc.SIZES[0]


def t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def params(seed=mc.SEED):
    import bcd_amd.hip as bh
    return bh.default_params(m=mc.M, random_order=mc.R, seed=seed)


def device_call(ctx, fr, fields, S, prm=None):
    out = ctx.denoise_temporal_motion(*dev(fr[0]), [dev(f) for f in fr[1:]], [None if f is None else t(f) for f in fields], S, prm or params())
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("S,nf", [(1, 1), (3, 2)])
def test_set_neighbour_motion_returns_the_device_call_s_frame(hipctx, S, nf):
    import bcd_amd.core as core
    fr = mc.frames_of(W, H)[:1 + nf]
    fields = [mc.holes(W, H, f) for f in range(nf)]
    if nf == 2:
        fields[0] = None
    want = device_call(hipctx, fr, fields, S)
    plain = hipctx.denoise_temporal(*dev(fr[0]), [dev(f) for f in fr[1:]], S, params()).cpu().numpy()
    ok, got = core.denoise_temporal(*fr[0], fr[1:], S, seed=mc.SEED, motions=fields)
    assert ok and rel_linf(got, want) <= TOL
    assert rel_linf(got, plain) > 10 * TOL                            # (the field did something)
    ok, got = core.denoise_temporal(*fr[0], fr[1:], S, seed=mc.SEED, motions=[None] * nf)
    assert ok and rel_linf(got, plain) <= TOL
    single = hipctx.denoise(*dev(fr[0]), S, params()).cpu().numpy()
    ok, got = core.denoise_temporal(*fr[0], fr[1:], S, seed=mc.SEED, motions=fields, after_clear=True)
    assert ok and rel_linf(got, single) <= TOL


def test_set_neighbour_motion_beside_colour_layers(hipctx):
    import bcd_amd.core as core
    S, nf = 3, 1
    prm = params()
    frames = mc.frames_of(W, H)[:1 + nf]
    fr = [(f[1], f[2], tl.share_layers(f[0], f[3])) for f in frames]
    fields = [mc.holes(W, H, 0)]
    d = [(t(n), t(h), [(t(c), t(v)) for c, v in lay]) for n, h, lay in fr]
    want = hipctx.denoise_temporal_layers_motion(d[0][0], d[0][1], d[0][2], d[1:], [t(fields[0])], S, prm)
    hipctx.synchronize()
    ok, got = core.denoise_temporal_layers(fr[0][0], fr[0][1], fr[0][2], fr[1:], S, seed=mc.SEED, motions=fields)
    assert ok
    for k in range(len(got)):
        assert rel_linf(got[k], want[k].cpu().numpy()) <= TOL, k


def test_bcd_cli_neighbour_motion_end_to_end(hipctx, tmp_path):
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    frames = mc.frames_of(W, H)
    on_disk = []
    for k, (col, ns, hist, cov) in enumerate(frames):
        stem = str(tmp_path / ("frame%d" % k))
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", core.merge_hist_ns(np.ascontiguousarray(hist), np.ascontiguousarray(ns)), True)
        core.write_exr(stem + "_cov.exr", cov, True)
        on_disk.append((core.read_exr(stem + ".exr", False), ns, hist, cov))      # (colours go through half precision on disk)
    fields = [mc.holes(W, H, 0), mc.holes(W, H, 1)]
    core.write_exr(str(tmp_path / "mv1.exr"), fields[0], True)
    wide = np.concatenate([fields[1], np.full((H, W, 2), 7.0, np.float32)], -1)           # four channels: the first two count
    core.write_exr(str(tmp_path / "mv2.exr"), wide, True)
    assert np.array_equal(core.read_exr(str(tmp_path / "mv1.exr"), True).view(np.uint32), fields[0].view(np.uint32))          # (NaN and inf survive the file)
    core.write_exr(str(tmp_path / "small.exr"), np.zeros((H - 2, W, 2), np.float32), True)
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    out_path = str(tmp_path / "out.exr")
    base = [exe, "-i", str(tmp_path / "frame0.exr"), "-o", out_path, "-p", "0", "-s", "2", "-m", "1", "--seed", "5"]
    r = subprocess.run(base + ["--neighbour", str(tmp_path / "frame1.exr"), "--neighbour-motion", str(tmp_path / "mv1.exr"),
                               "--neighbour", str(tmp_path / "frame2.exr"), "--neighbour-motion", str(tmp_path / "mv2.exr")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = hipctx.denoise_temporal_motion(*dev(on_disk[0]), [dev(on_disk[1]), dev(on_disk[2])], [t(f) for f in fields], 2, bh.default_params(m=1.0, seed=5))
    w = hipctx.zero_bad_values(want).cpu().numpy()
    got = core.read_exr(out_path, False)
    assert np.max(np.abs(got - w.astype(np.float16).astype(np.float32))) <= 2e-3 * np.max(w)
    plain = hipctx.zero_bad_values(hipctx.denoise_temporal(*dev(on_disk[0]), [dev(on_disk[1]), dev(on_disk[2])], 2, bh.default_params(m=1.0, seed=5))).cpu().numpy()
    assert np.max(np.abs(got - plain)) > 2e-2 * np.max(w)            # (... and not the plain temporal call's)
    r = subprocess.run(base + ["--neighbour-motion", str(tmp_path / "mv1.exr"), "--neighbour", str(tmp_path / "frame1.exr")], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR in program arguments" in r.stdout          # before any --neighbour
    r = subprocess.run(base + ["--neighbour", str(tmp_path / "frame1.exr"), "--neighbour-motion", str(tmp_path / "small.exr")], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR in program arguments" in r.stdout          # another size than the frame's
