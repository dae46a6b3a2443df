"""CPU tests of the selection from means and covariances (bcd_hip_denoise_moments): the C ABI declares and exports the entry points, they
refuse a null context, nothing falls back to a CPU path when no device is there, bcd_cli --moment-selection does not look for a histogram file, and
setMomentSelection is reachable through libbcdcore.so.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import bcd_amd.core as core
import bcd_amd.hip as bh
import moments_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
NAMES = ("bcd_hip_similarity_masks_moments", "bcd_hip_window_distances_moments", "bcd_hip_denoise_moments", "bcd_hip_denoise_moments_host")
EINVAL = -1


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    L = bh.lib()
    for name in NAMES:
        assert name + "(" in txt and name in bh.SYMBOLS and hasattr(L, name), name
    assert "3 = planes from means and covariances" in txt and "NOT offered" in txt


def test_null_context_is_refused():
    L = bh.lib()
    prm = bh.default_params()
    layer = (bh.Layer * 1)()
    host_layer = (bh.HostLayer * 1)()
    opt = bh.LayersHostOptions(0.0, 0, 0)
    assert L.bcd_hip_similarity_masks_moments(None, None, None, 8, 8, 1, 6, 1.0, 1e-8, None, None) == EINVAL
    assert L.bcd_hip_window_distances_moments(None, None, None, 8, 8, 1, 6, 1e-8, 3, 3, None) == EINVAL
    assert L.bcd_hip_denoise_moments(None, None, 8, 8, 1, C.byref(prm), 1e-8, layer, 1, None) == EINVAL
    assert L.bcd_hip_denoise_moments_host(None, None, 8, 8, 1, C.byref(prm), C.byref(opt), 1e-8, host_layer, 1) == EINVAL


def test_no_cpu_path_without_a_device():
    import torch
    if torch.cuda.is_available():
        return
    h = C.c_void_p()
    assert bh.lib().bcd_hip_ctx_create(C.byref(h), 0, None) == -2 and not h.value      # BCD_HIP_EDEVICE: no context, so no call to fall back from
    col, cov, ns, _ = mc.noisy(24, 20)
    for scales in (1, 2):
        ok, outs = core.denoise_moments([(col, cov)], ns, scales)
        assert not ok and not outs[0].any()                                          # bcd::Denoiser::denoise() returns false, nothing is written


def test_set_moment_selection_is_reachable_through_libbcdcore():
    assert hasattr(core.lib(), "bcdcore_denoise_moments")
    col, cov, ns, _ = mc.noisy(24, 20)
    # several devices are refused with a message before any device is asked for
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport bcd_amd.core as core, moments_cases as mc\n"
                        "col, cov, ns, _ = mc.noisy(24, 20)\nok, _ = core.denoise_moments([(col, cov)], ns, 1, devices=[0, 1])\nprint('OK' if ok else 'REFUSED')"
                        % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "REFUSED" in r.stdout and "not available over several devices" in r.stderr, r.stdout + r.stderr
    # one device: the request gets as far as asking for the device -- no histogram image was demanded on the way
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport bcd_amd.core as core, moments_cases as mc\n"
                        "col, cov, ns, _ = mc.noisy(24, 20)\nok, _ = core.denoise_moments([(col, cov), (col * 0.5, cov * 0.25)], ns, 2)\nprint('OK' if ok else 'REFUSED')"
                        % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "REFUSED" in r.stdout and "no usable HIP device" in r.stderr and "histogram" not in r.stderr, r.stdout + r.stderr


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_moment_selection_does_not_look_for_a_histogram_file(tmp_path):
    col, cov, ns, _ = mc.noisy(24, 20)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_cov.exr", cov, True)
    core.write_exr(stem + "_ns.exr", ns, True)
    out = str(tmp_path / "out.exr")
    assert not os.path.exists(stem + "_hist.exr")
    r = _cli("-i", stem + ".exr", "-o", out)                                          # the histogram path does look for it
    assert r.returncode != 0 and "couldn't load input histogram image file" in r.stdout
    for tail in (["--moment-selection", "--nsamples", "8"], ["--moment-selection", "1e-6", "--nsamples", stem + "_ns.exr"],
                 ["--nsamples", "8", "-s", "1", "--moment-selection"]):
        r = _cli("-i", stem + ".exr", "-o", out, *tail)
        assert r.returncode == 2 and "no usable HIP device" in r.stderr, r.stdout + r.stderr
        assert "histogram" not in r.stdout and "histogram" not in r.stderr
    r = _cli("-i", stem + ".exr", "-o", out, "--moment-selection")
    assert r.returncode != 0 and "needs the sample counts" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "--moment-selection", "--nsamples", "8", "--devices", "0,1")
    assert r.returncode != 0 and "not available with several devices" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "--moment-selection", "-1", "--nsamples", "8")
    assert r.returncode != 0 and "finite non-negative" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--nsamples", "8")
    assert r.returncode != 0 and "goes with --moment-selection" in r.stdout
    assert "--moment-selection [floor]" in _cli("--help").stdout
    assert not os.path.exists(out)
