"""CPU tests of the plumbing of the cross-frame moment selection ("Moments"): the header declares and the library exports the four entry points, the
definition stands in the header and in DESIGN, a null context is refused, the band rule of the planes kernel is stated where the kernel is,
addNeighbourFrameMoments is reachable through libbcdcore.so and denoise() refuses what it must with a message before any device is asked for, and bcd_cli
--neighbour-nsamples checks its arguments before any device work.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import bcd_amd.core as core
import bcd_amd.hip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
NAMES = ("bcd_hip_similarity_masks_moments_cross", "bcd_hip_window_distances_moments_cross", "bcd_hip_denoise_temporal_moments", "bcd_hip_denoise_temporal_moments_host")
EINVAL = -1
TERM = "if (q > 0.f) { s = s + (d * d) / q; n = n + 1; }"
GUIDE_TERM = "if (q > 0.f) { t = (d * d) / q;  if (t == t) { s = s + t; n = n + 1; } }"


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    L = bh.lib()
    for name in NAMES:
        assert name + "(" in txt and name in bh.SYMBOLS and hasattr(L, name), name
    assert txt.index("int bcd_hip_warp_features(") < txt.index("int bcd_hip_similarity_masks_moments_cross(") < txt.index("int bcd_hip_denoise_band(")   # behind "Features"


def test_the_definition_stands_in_the_header_and_in_design():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    block = txt[txt.index("/* ---- moments: the cross-frame selection"):txt.index("int bcd_hip_similarity_masks_moments_cross(")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### Moments"):design.index("**Tests of the frame call.**")]
    for text in (block, section):
        assert "d = m0_k(x) - mj_k(y)" in text and "q = (v0_k(x) + vj_k(y)) + eps" in text and TERM in text
        assert GUIDE_TERM not in text                                    # the feature term skips a NaN term; this one counts it
        assert "bcd_hip_pixel_cov" in text and "not reliably dissimilar" in text and "(dl + b)(2b + 1) + (dc + b)".replace(" ", "") in text.replace(" ", "")
    assert "a NaN or infinite term IS counted" in block and "a NaN or infinite term IS counted" in section
    assert "k_pairdist_moments_cross" in section and "k_masks_moments_cross_fused" in section
    assert txt.count(GUIDE_TERM) == 2                                    # the in-frame and the cross feature term, and no third
    for text in (txt, design):
        assert "there is no cross-frame moment selection" not in text    # the sentences this makes untrue are gone


def test_null_context_is_refused():
    L = bh.lib()
    prm = bh.default_params()
    layer = (bh.Layer * 1)()
    assert L.bcd_hip_similarity_masks_moments_cross(None, None, None, None, None, 8, 8, 1, 2, 1.0, 1e-8, 0, None, None) == EINVAL
    assert L.bcd_hip_window_distances_moments_cross(None, None, None, None, None, 8, 8, 1, 2, 1e-8, 3, 3, None) == EINVAL
    assert L.bcd_hip_denoise_temporal_moments(None, None, None, 0, None, 8, 8, 1, C.byref(prm), 1e-8, layer, 1, None, None) == EINVAL
    assert L.bcd_hip_denoise_temporal_moments_host(None, None, None, 0, None, 8, 8, 1, C.byref(prm), 1e-8, layer, 1, None, None) == EINVAL


def test_every_accepted_search_radius_has_a_band_within_64_kib():
    """the band rule as k_similarity_moments_cross.hip states it, restated here: 6 planes of (64 + 2b) x (4 + nl - 1) floats"""
    src = open(os.path.join(ROOT, "bcd_amd", "csrc", "k_similarity_moments_cross.hip")).read()
    assert "int bcd_pairdist_moments_cross_band(int b)" in src and "PMX_LDS_LIMIT = 64 * 1024" in src
    for b in range(0, 16):
        side = 2 * b + 1
        line = 6 * (64 + 2 * b) * 4
        max_nl = 65536 // line - 3
        bands = -(-side // max_nl)
        nl = -(-side // bands)
        assert nl >= 1 and 6 * (64 + 2 * b) * (4 + nl - 1) * 4 <= 65536, b
        assert (bands == 1) == (b <= 13)
    for b in range(1, 7):                                                # the fused form: neighbour and frame planes, two term tiles, two count tiles
        assert (6 * (66 + 2 * b) * (6 + 2 * b) + 10 * 66 * 6) * 4 <= 65536


def _child(body):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport numpy as np\nimport bcd_amd.core as core, moments_cases as mc, guide_cases as gc\n"
            "col, cov, ns, _ = mc.noisy(24, 20)\nf, v, _ = gc.features(24, 20, 3)\nlay = [(col, cov)]\nnb = [(ns, lay)] * 2\nkw = dict(floors=[1e-2] * 3)\n%s\n"
            "print('OK' if ok else 'REFUSED')" % (ROOT, os.path.join(ROOT, "tests"), body))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


def test_add_neighbour_frame_moments_is_reachable_and_refuses_before_any_device():
    assert hasattr(core.lib(), "bcdcore_denoise_temporal_moments")
    assert "void addNeighbourFrameMoments(const DenoiserInputs& i_rFrame)" in open(os.path.join(ROOT, "include", "bcd", "core", "Denoiser.h")).read()
    refused = {
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, plain_neighbours=1)": "not available with the moment selection",                 # a mixed list
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, plain_neighbours=2)": "every neighbour must be added that way",                  # today's refusal stands
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, moment_selection=False)": "addNeighbourFrameMoments need the selection from means and covariances (setMomentSelection(true))",
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, moment_selection=False, plain_neighbours=1)": "addNeighbourFrameMoments need the selection from means and covariances",
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, devices=[0, 1])": "not available over several devices",                          # the one-device check
        "ok, _ = core.denoise_temporal_moments(ns, lay * 2, [(ns, lay * 2)] * 2, drop_layers=1)": "exactly one layer (addNeighbourFrameLayer) per added layer",   # the size checks
        "ok, _ = core.denoise_temporal_moments(ns, lay, nb, features=f, variances=v, neighbour_features=[f, f], **kw)":
            "feature variances must be given for the frame and every neighbour frame or for none",
    }
    for body, message in refused.items():
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and message in r.stderr and "HIP device" not in r.stderr.replace("several devices", ""), body + r.stdout + r.stderr
    # well-formed calls get as far as asking for the device: plain, with layers, two scales and a motion field, with the feature gate
    for body in ("ok, _ = core.denoise_temporal_moments(ns, lay, nb)",
                 "ok, _ = core.denoise_temporal_moments(ns, lay * 2, [(ns, lay * 2)], nscales=2, motions=[np.zeros((20, 24, 2), np.float32)], var_floor=1e-4)",
                 "ok, _ = core.denoise_temporal_moments(ns, lay, nb, features=f, variances=v, neighbour_features=[f, f], neighbour_variances=[v, v], **kw)"):
        r = _child(body)
        assert r.returncode == 0 and "REFUSED" in r.stdout and "no usable HIP device" in r.stderr and "moment" not in r.stderr, body + r.stdout + r.stderr


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_checks_the_neighbour_sample_count_arguments_before_any_device_work(tmp_path):
    import numpy as np
    import moments_cases as mc
    col, cov, ns, _ = mc.noisy(24, 20)
    hist = np.concatenate([np.ones((20, 24, 12), np.float32), np.asarray(ns, np.float32).reshape(20, 24, 1)], -1)   # <frame>_hist.exr: the bins, then the sample count
    for name in ("frame", "nb"):
        stem = str(tmp_path / name)
        core.write_exr(stem + ".exr", col, False)
        core.write_exr(stem + "_cov.exr", cov, True)
    stem, nb = str(tmp_path / "frame"), str(tmp_path / "nb")
    core.write_exr(stem + "_hist.exr", hist, True)                       # (the neighbour has NO _hist.exr: under --moment-selection none is loaded)
    core.write_exr(nb + "_ns.exr", np.asarray(ns, np.float32).reshape(20, 24, 1), True)
    core.write_exr(nb + "_ns3.exr", col, True)
    out = str(tmp_path / "out.exr")
    base = ["-i", stem + ".exr", "-o", out, "-p", "0", "--moment-selection"]      # (neighbour frames do not combine with the spike prefilter)
    good = [base + ["--nsamples", "8", "--neighbour", nb + ".exr"],                                                    # the numeric --nsamples serves the neighbour
            base + ["--nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples", nb + "_ns.exr"],
            base + ["-h", stem + "_hist.exr", "--neighbour", nb + ".exr", "--neighbour-nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples", nb + "_ns.exr"]]   # (the frame's counts: its -h file)
    for args in good:
        r = _cli(*args)
        assert r.returncode == 2 and "no usable HIP device" in r.stderr and "ERROR" not in r.stdout, (args, r.stdout + r.stderr)
    bad = [
        (base + ["-h", stem + "_hist.exr", "--neighbour", nb + ".exr"], ("--neighbour-nsamples <file|n>", "numeric --nsamples")),                 # neither: the error names both
        (base + ["--nsamples", nb + "_ns.exr", "--neighbour", nb + ".exr"], ("--neighbour-nsamples <file|n>", "numeric --nsamples")),   # a FILE --nsamples is the frame's alone
        (["-i", stem + ".exr", "-o", out, "--neighbour", stem + ".exr", "--neighbour-nsamples", "8"], ("--neighbour-nsamples goes with --moment-selection",)),
        (base + ["--nsamples", "8", "--neighbour-nsamples", "8"], ("--neighbour-nsamples follows the --neighbour it belongs to",)),
        (base + ["--nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples"], ("expecting <file|n> after --neighbour-nsamples",)),
        (base + ["--nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples", "-3"], ("expecting a positive number or an EXR file",)),
        (base + ["--nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples", nb + "_ns3.exr"], ("couldn't load a one-channel sample count image",)),
        (base + ["--nsamples", "8", "--neighbour", nb + ".exr", "--neighbour-nsamples", str(tmp_path / "missing.exr")], ("couldn't load a one-channel sample count image",)),
    ]
    for args, messages in bad:
        r = _cli(*args)
        assert r.returncode == 1 and all(m in r.stdout for m in messages), (args, r.stdout + r.stderr)
    r = _cli("-i", stem + ".exr", "-o", out, "--neighbour", nb + ".exr")                                              # without --moment-selection the histograms are still asked for
    assert r.returncode == 1 and "couldn't load neighbour histogram image file" in r.stdout
    assert "--neighbour-nsamples <file|n>" in _cli("--help").stdout
    assert not os.path.exists(out)
