"""CPU tests of the plumbing of the cross-frame feature gate ("Features"): the header declares and the library exports the entry points, the
definition stands in the header and in DESIGN, a null context is refused, setNeighbourGuideFeatures is reachable through libbcdcore.so and denoise() refuses
what it must with a message before any device is asked for, and bcd_cli --neighbour-features checks its arguments before any device work.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import bcd_amd.core as core
import bcd_amd.hip as bh
import guide_cases as gc
import moments_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
NAMES = ("bcd_hip_denoise_temporal_guided", "bcd_hip_denoise_temporal_guided_host", "bcd_hip_similarity_masks_guide_cross", "bcd_hip_window_distances_guide_cross",
         "bcd_hip_warp_features")
EINVAL = -1
TERM = "if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }"


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    L = bh.lib()
    for name in NAMES:
        assert name + "(" in txt and name in bh.SYMBOLS and hasattr(L, name), name
    assert "typedef struct { const float *features; const float *variances;" in txt and "} bcd_hip_guide_images;" in txt
    assert C.sizeof(bh.GuideImages) == 16 and bh.GuideImages.variances.offset == 8
    assert txt.count(TERM) == 2 and "d = f0_k(x) - fj_k(y)" in txt       # the definition, in the header: the in-frame term and the cross term
    assert "cross mask &= G_j" in txt
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    features = design[design.index("### Features"):]
    assert TERM in features and "d = f0_k(x) - fj_k(y)" in features and "k_pairdist_guide_cross" in features
    for text in (txt, design):
        assert "the moment and the feature-gated selection" not in text  # the "do not combine" sentences this makes untrue are gone


def test_null_context_is_refused():
    L = bh.lib()
    prm = bh.default_params()
    layer = (bh.Layer * 1)()
    g = bh.Guide(None, None, 1, None, 1.0)
    ng = bh.GuideImages(None, None)
    assert L.bcd_hip_denoise_temporal_guided(None, None, None, None, 0, None, 8, 8, 12, 1, C.byref(prm), layer, 1, C.byref(g), C.byref(ng)) == EINVAL
    assert L.bcd_hip_denoise_temporal_guided_host(None, None, None, None, 0, None, 8, 8, 12, 1, C.byref(prm), layer, 1, C.byref(g), C.byref(ng)) == EINVAL
    assert L.bcd_hip_similarity_masks_guide_cross(None, C.byref(g), C.byref(ng), 8, 8, 1, 2, None, None) == EINVAL
    assert L.bcd_hip_window_distances_guide_cross(None, C.byref(g), C.byref(ng), 8, 8, 1, 2, 3, 3, None) == EINVAL
    assert L.bcd_hip_warp_features(None, C.byref(ng), 3, None, 8, 8, None, None, None) == EINVAL


def _child(body):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport numpy as np\nimport bcd_amd.core as core, moments_cases as mc, guide_cases as gc\n"
            "col, cov, ns, _ = mc.noisy(24, 20)\nhist = np.ones((20, 24, 12), np.float32)\nf, v, _ = gc.features(24, 20, 3)\n"
            "nb = [(ns, hist, [(col, cov)])] * 2\nkw = dict(floors=[1e-2] * 3)\n%s\nprint('OK' if ok else 'REFUSED')" % (ROOT, os.path.join(ROOT, "tests"), body))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


def test_set_neighbour_guide_features_is_reachable_through_libbcdcore():
    assert hasattr(core.lib(), "bcdcore_denoise_temporal_guided")
    refused = {
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f, f], devices=[0, 1], **kw)": "not available over several devices",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f, f], moment_selection=True, **kw)":
            "not available with the moment selection",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f, f], neighbours_with_features=1, **kw)":
            "neighbour frame 2 has no feature buffers (setNeighbourGuideFeatures)",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=None, **kw)": "neighbour frame 1 has no feature buffers",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f[..., :2]] * 2, **kw)":
            "the feature image of neighbour frame 1 must be 24x20x3",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, variances=v, neighbour_features=[f, f], **kw)":
            "feature variances must be given for the frame and every neighbour frame or for none",
        "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f, f], neighbour_variances=[v, v], **kw)":
            "feature variances must be given for the frame and every neighbour frame or for none",
        "ok, _ = core.denoise_temporal(col, ns, hist, cov, [(col, ns, hist, cov)], features=f, neighbour_features=[f[:, :, :1]], **kw)":
            "the feature image of neighbour frame 1 must be 24x20x3",
    }
    for body, message in refused.items():
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and message in r.stderr and "HIP device" not in r.stderr.replace("several devices", ""), body + r.stdout + r.stderr
    # well-formed feature buffers get as far as asking for the device: with and without variances, layers and motion, one and two scales
    for body in ("ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov)], nb, features=f, neighbour_features=[f, f], **kw)",
                 "ok, _ = core.denoise_temporal_layers(ns, hist, [(col, cov), (col * 0.5, cov * 0.25)], [(ns, hist, [(col, cov), (col, cov)])], nscales=2, features=f, variances=v, "
                 "neighbour_features=[f], neighbour_variances=[v], motions=[np.zeros((20, 24, 2), np.float32)], **kw)",
                 "ok, _ = core.denoise_temporal(col, ns, hist, cov, [(col, ns, hist, cov)], features=f, neighbour_features=[f], **kw)"):
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and "no usable HIP device" in r.stderr and "feature" not in r.stderr, body + r.stdout + r.stderr


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_checks_the_neighbour_feature_arguments_before_any_device_work(tmp_path):
    import numpy as np
    col, cov, ns, _ = mc.noisy(24, 20)
    f, v, _ = gc.features(24, 20, 3)
    hist = np.concatenate([np.ones((20, 24, 12), np.float32), np.asarray(ns, np.float32).reshape(20, 24, 1)], -1)   # <frame>_hist.exr: the bins, then the sample count
    for name in ("frame", "nb"):
        stem = str(tmp_path / name)
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_hist.exr", hist, True)
        core.write_exr(stem + "_cov.exr", cov, True)
    stem, nb = str(tmp_path / "frame"), str(tmp_path / "nb")
    core.write_exr(stem + "_f.exr", f, True)
    core.write_exr(stem + "_fv.exr", v, True)
    core.write_exr(stem + "_f2.exr", f[..., :2], True)
    core.write_exr(stem + "_fsmall.exr", f[:10], True)
    out = str(tmp_path / "out.exr")
    base = ["-i", stem + ".exr", "-o", out]
    feat = ["--features", stem + "_f.exr", "--feature-floors", "0.01,0.01,0.01"]
    good = [base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr"],
            base + feat + ["--feature-variances", stem + "_fv.exr", "--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr", "--neighbour-feature-variances",
                           stem + "_fv.exr", "--neighbour", nb + ".exr", "--neighbour-feature-variances", stem + "_fv.exr", "--neighbour-features", stem + "_f.exr"]]
    for args in good:
        r = _cli(*args)
        assert r.returncode == 2 and "no usable HIP device" in r.stderr and "ERROR" not in r.stdout, r.stdout + r.stderr
    bad = [
        (base + feat + ["--neighbour", nb + ".exr"], "has no --neighbour-features while --features is given"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr", "--neighbour", nb + ".exr"], "has no --neighbour-features while --features is given"),
        (base + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr"], "has --neighbour-features but there is no --features"),
        (base + feat + ["--neighbour-features", stem + "_f.exr"], "--neighbour-features follows the --neighbour it belongs to"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-feature-variances", stem + "_fv.exr"], "has no --neighbour-features while --features is given"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr", "--neighbour-feature-variances", stem + "_fv.exr"], "feature variances go with the frame and every neighbour or with none"),
        (base + feat + ["--feature-variances", stem + "_fv.exr", "--neighbour", nb + ".exr", "--neighbour-features", stem + "_f.exr"], "feature variances go with the frame and every neighbour or with none"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_f2.exr"], "must be 24x20x3 like the --features image"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", stem + "_fsmall.exr"], "must be 24x20x3 like the --features image"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features", str(tmp_path / "missing.exr")], "couldn't load neighbour feature image file"),
        (base + feat + ["--neighbour", nb + ".exr", "--neighbour-features"], "expecting <file.exr> after --neighbour-features"),
    ]
    for args, message in bad:
        r = _cli(*args)
        assert r.returncode == 1 and message in r.stdout, (args, r.stdout + r.stderr)
    text = _cli("--help").stdout
    for flag in ("--neighbour-features <file>", "--neighbour-feature-variances <file>"):
        assert flag in text
    assert not os.path.exists(out)
