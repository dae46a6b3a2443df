"""CPU tests of the feature gate's plumbing: the header declares and the library exports the entry points, the definition stands in the header,
a null context is refused, setGuideFeatures is reachable through libbcdcore.so and refuses what it must with a message before any device is asked for,
and bcd_cli --features checks its arguments before any device work.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import bcd_amd.core as core
import bcd_amd.hip as bh
import guide_cases as gc
import moments_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
NAMES = ("bcd_hip_similarity_masks_guide", "bcd_hip_window_distances_guide", "bcd_hip_gate_masks", "bcd_hip_denoise_guided", "bcd_hip_denoise_guided_host")
EINVAL = -1


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    L = bh.lib()
    for name in NAMES:
        assert name + "(" in txt and name in bh.SYMBOLS and hasattr(L, name), name
    assert re.search(r"typedef struct bcd_hip_guide \{\s*const float \*features;[^}]*const float \*variances;[^}]*int32_t\s+nb_channels;[^}]*const float \*floors;[^}]*float\s+threshold;\s*\} bcd_hip_guide;", txt)
    assert "#define BCD_HIP_GUIDE_MAX_CHANNELS 8" in txt
    assert "if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }" in txt          # the definition, in the header
    assert "mask = selection mask AND feature mask" in txt and "NOT offered with a guide" in txt
    # the ctypes mirror has the layout of the C struct on this ABI: pointer, pointer, int32 (+ padding), pointer, float (+ padding)
    assert C.sizeof(bh.Guide) == 40 and bh.Guide.nb_channels.offset == 16 and bh.Guide.floors.offset == 24 and bh.Guide.threshold.offset == 32
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 15." in design and "if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }" in design


def test_null_context_is_refused():
    L = bh.lib()
    prm = bh.default_params()
    layer = (bh.Layer * 1)()
    host_layer = (bh.HostLayer * 1)()
    opt = bh.LayersHostOptions(0.0, 0, 0)
    g = bh.Guide(None, None, 1, None, 1.0)
    assert L.bcd_hip_similarity_masks_guide(None, C.byref(g), 8, 8, 1, 2, None, None) == EINVAL
    assert L.bcd_hip_window_distances_guide(None, C.byref(g), 8, 8, 1, 2, 3, 3, None) == EINVAL
    assert L.bcd_hip_gate_masks(None, None, None, None, 8, 8, 2) == EINVAL
    assert L.bcd_hip_denoise_guided(None, None, None, 8, 8, 0, 1, C.byref(prm), 1e-8, layer, 1, C.byref(g), None) == EINVAL
    assert L.bcd_hip_denoise_guided_host(None, None, None, 8, 8, 0, 1, C.byref(prm), C.byref(opt), 1e-8, host_layer, 1, C.byref(g)) == EINVAL


def _child(body):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport numpy as np\nimport bcd_amd.core as core, moments_cases as mc, guide_cases as gc\n"
            "col, cov, ns, _ = mc.noisy(24, 20)\nf, v, _ = gc.features(24, 20, 3)\n%s\nprint('OK' if ok else 'REFUSED')" % (ROOT, os.path.join(ROOT, "tests"), body))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


def test_set_guide_features_is_reachable_through_libbcdcore():
    assert hasattr(core.lib(), "bcdcore_denoise_guided")
    refused = {
        "ok, _ = core.denoise_guided([(col, cov)], ns, None, f, v, [1e-4] * 3, devices=[0, 1])": "not available over several devices",
        "ok, _ = core.denoise_guided([(col, cov)], ns, None, f, v, [1e-4] * 2)": "2 feature floors for 3 feature channels",
        "ok, _ = core.denoise_guided([(col, cov)], ns, None, f, None, [1e-2] * 3, feature_width_override=20)": "the feature image must be 24x20",
        "ok, _ = core.denoise_guided([(col, cov)], ns, None, np.zeros((20, 24, 9), np.float32), None, [1e-2] * 9)": "with 1 to 8 channels",
        "ok, _ = core.denoise_guided([(col, cov)], ns, None, f, v[..., :2], [1e-4] * 3)": "the feature variance image must be 24x20x3",
    }
    for body, message in refused.items():
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and message in r.stderr and "HIP device" not in r.stderr.replace("several devices", ""), body + r.stdout + r.stderr
    # a well-formed guide gets as far as asking for the device, with and without histograms' stand-in (the moment selection); so does a null features pointer
    for body in ("ok, _ = core.denoise_guided([(col, cov), (col * 0.5, cov * 0.25)], ns, None, f, v, [1e-4] * 3, nscales=2)",
                 "ok, _ = core.denoise_guided([(col, cov)], ns, None, f, None, [0.01, 0.0, 0.01], 0.5)",
                 "ok, _ = core.denoise_guided([(col, cov)], ns, None, None)"):
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and "no usable HIP device" in r.stderr and "feature" not in r.stderr, body + r.stdout + r.stderr


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_checks_the_feature_arguments_before_any_device_work(tmp_path):
    col, cov, ns, _ = mc.noisy(24, 20)
    f, v, _ = gc.features(24, 20, 3)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_cov.exr", cov, True)
    core.write_exr(stem + "_f.exr", f, True)
    core.write_exr(stem + "_fv.exr", v, True)
    core.write_exr(stem + "_f2.exr", f[..., :2], True)
    core.write_exr(stem + "_fsmall.exr", f[:10], True)
    out = str(tmp_path / "out.exr")
    base = ["-i", stem + ".exr", "-o", out, "--moment-selection", "--nsamples", "8"]
    assert (core.read_exr(stem + "_f.exr", True) == f).all()                            # multi-channel EXR files keep float32
    good = [["--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01"],
            ["--features", stem + "_f.exr", "--feature-variances", stem + "_fv.exr", "--feature-floors", "1e-4,0,1e-4", "--feature-threshold", "0.5"]]
    for tail in good:
        r = _cli(*base, *tail)
        assert r.returncode == 2 and "no usable HIP device" in r.stderr and "ERROR" not in r.stdout, r.stdout + r.stderr
    bad = {
        ("--features", stem + "_f.exr"): "--features needs --feature-floors",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,0.01"): "2 --feature-floors for 3 feature channels",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,-1,0.01"): "finite non-negative",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,,0.01"): "finite non-negative",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,inf,0.01"): "finite non-negative",
        ("--features", stem + "_f.exr", "--feature-floors", "0,0,0"): "no feature channel can count",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01", "--feature-threshold", "-1"): "finite non-negative",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01", "--feature-threshold", "nan"): "finite non-negative",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01", "--feature-variances", stem + "_f2.exr"): "but the feature image is 24x20x3",
        ("--features", stem + "_fsmall.exr", "--feature-floors", "0.01,0.01,0.01"): "but the input color image is 24x20",
        ("--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01", "--devices", "0,1"): "not available with several devices",
        ("--features", str(tmp_path / "missing.exr"), "--feature-floors", "0.01"): "couldn't load feature image file",
        ("--feature-floors", "0.01"): "go with --features",
        ("--feature-variances", stem + "_fv.exr"): "go with --features",
    }
    for tail, message in bad.items():
        r = _cli(*base, *tail)
        assert r.returncode == 1 and message in r.stdout, (tail, r.stdout + r.stderr)
    text = _cli("--help").stdout
    for flag in ("--features <file>", "--feature-variances <file>", "--feature-floors <a,b,...>", "--feature-threshold <float>"):
        assert flag in text
    assert not os.path.exists(out)
