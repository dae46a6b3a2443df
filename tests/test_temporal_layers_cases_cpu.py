"""CPU tests of the test infrastructure and of the public surface of the layered temporal call ("Layers"): no GPU.

  * the whole-call configurations of tests/temporal_layers_cases.py: the per-scale processed / fallback / similar_total of the per-layer reference runs
    (tests/temporal_layers_ref.py: temporal_ref.denoise_multiscale on each layer alone) are identical across the layers -- the selection sees no colour --,
    every configuration has fallback pixels at some scale and full estimates at every scale, so both halves of the estimate stage are exercised;
  * the constructed stage cases are what they promise: every layer has the case's selection, layer k has the same kind in every frame, the scaled and
    rotated layers are exact images of their sources, the special items (|S| = 27, 28, 0; the poisoned member; the layers below the floor) exist;
  * the reference of a layer scaled by a power of two (far above the floor) is the scaled reference: a layer's estimate depends on that layer alone;
  * the header declares and the library exports the three entry points, which refuse a null context without touching a device;
  * bcd_cli --neighbour-layer: the help text, and every argument error (too few operands, no --neighbour ahead of it, a missing file, a count that differs
    from the number of --layer arguments, another size) before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bayes_ref as br
import layer_cases as lc
import temporal_layers_cases as tl
import temporal_layers_ref as tlr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bcd_hip_denoise_temporal_layers", "bcd_hip_denoise_temporal_layers_host", "bcd_hip_bayes_accumulate_temporal_layers")


@pytest.mark.parametrize("W,H,S,F,m,r", tl.CONFIGS)
def test_selection_figures_agree_across_layers_and_cover_both_kinds_of_item(W, H, S, F, m, r):
    stats = [tl.reference(W, H, S, F, m, r, k)[1] for k in range(tl.L_WHOLE)]
    assert all(s == stats[0] for s in stats[1:]), stats
    assert any(s["fallback"] > 0 for s in stats[0]), stats[0]
    assert all(s["processed"] - s["fallback"] > 0 for s in stats[0]), stats[0]
    outs = [tl.reference(W, H, S, F, m, r, k)[0] for k in range(tl.L_WHOLE)]
    assert not np.allclose(outs[0], outs[1]) and not np.allclose(outs[1], outs[2])       # (the layers are different images)


def test_stage_cases_share_the_selection_and_keep_their_kinds_from_frame_to_frame():
    case = tl.stage_cases("sizes F=2", 5)[0]
    base = case.case
    assert [case.layer(k).F for k in range(5)] == [2] * 5
    for k in range(5):
        lk = case.layer(k)
        assert lk.mask is base.mask and lk.state is base.state and lk.nsim_total is base.nsim_total
    for f in range(3):
        assert np.array_equal(case.col[0][f], base.col[f]) and np.array_equal(case.pixcov[0][f], base.pixcov[f])                      # kind 0: the frame
        k = lc.EXPONENTS[0]
        assert np.array_equal(case.col[1][f], base.col[f] * np.float32(2.0 ** k)) and np.array_equal(case.pixcov[1][f], base.pixcov[f] * np.float32(4.0 ** k))
        assert np.array_equal(case.col[3][f], base.col[f][..., lc.ROT]) and np.array_equal(case.pixcov[3][f], base.pixcov[f][..., lc.ROT6])
        assert np.abs(case.col[2][f] - base.col[f]).max() > 0.05                       # kind 2: nothing of the frame
    assert np.abs(case.col[2][0] - case.col[2][1]).max() > 0.01                        # ... and independent noise from frame to frame


def test_special_items_exist():
    lim = tl.limit_case()
    n = sorted(int(x) for x in lim.case.nsim_total[lim.case.state == 1])
    assert n.count(27) >= 2 and n.count(28) >= 3 and n.count(0) == 1
    spread = [br.popcount(m)[lim.case.state == 1] for m in lim.case.mask]
    assert sum(1 for i in range(len(spread[0])) if all(s[i] > 0 for s in spread)) >= 3  # members in every one of the three frames
    for items in (1, 6, 7, 8):
        c = tl.weak_list_case(items, 1, 400 + items).case
        nn = c.nsim_total[c.state == 1]
        assert len(nn) == items and (nn < tl.K1).all() and (nn > 0).all()
    p = tl.poisoned_case()
    assert np.isnan(p.pixcov[1][2]).sum() == 1 and all(np.isfinite(p.pixcov[k][f]).all() for k in range(3) for f in range(3) if (k, f) != (1, 2))
    s64, _, items = tlr.accumulate(p, 1)
    bad = [it for it in items if it["n"] >= tl.K1 and not np.isfinite(s64[br.touched(it, 1)]).any()]
    assert [it["pos"] for it in bad] == [tuple(p.poisoned_item)]
    for k in (0, 2):
        s, _, its = tlr.accumulate(p, k)
        assert all(np.isfinite(s[br.touched(it, 1)]).all() for it in its)


def test_the_reference_of_a_scaled_layer_is_the_scaled_reference():
    case = tl.stage_cases("sizes F=1", 2)[0]
    s0, c0, _ = tlr.accumulate(case, 0)
    s1, c1, _ = tlr.accumulate(case, 1)
    assert np.array_equal(c0, c1)
    scale = 2.0 ** lc.EXPONENTS[0]
    ok = np.isfinite(s0)
    assert np.allclose(s1[ok], s0[ok] * scale, rtol=1e-6, atol=0)


def test_header_declares_and_library_exports_the_entry_points():
    import bcd_amd.hip as bh
    text = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    lib = bh.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in bh.SYMBOLS and hasattr(lib, name)
    for struct in ("bcd_hip_frame_layer", "bcd_hip_frame_layers", "bcd_hip_stage_frame_layers"):
        assert re.search(r"}\s*%s;" % struct, text), struct
    assert C.sizeof(bh.FrameLayers) == 4 * C.sizeof(C.c_void_p) and C.sizeof(bh.FrameLayer) == 2 * C.sizeof(C.c_void_p)
    assert C.sizeof(bh.StageFrameLayers) == 3 * C.sizeof(C.c_void_p)


def test_calls_without_a_context_are_errors_not_crashes():
    import bcd_amd.hip as bh
    lib = bh.lib()
    prm = bh.default_params()
    assert lib.bcd_hip_denoise_temporal_layers(None, None, None, None, 1, 8, 8, 20, 1, C.byref(prm), None, 2) == -1
    assert lib.bcd_hip_denoise_temporal_layers_host(None, None, None, None, 1, 8, 8, 20, 1, C.byref(prm), None, 2) == -1
    assert lib.bcd_hip_bayes_accumulate_temporal_layers(None, None, 2, 2, None, None, 8, 8, 1, 6, 1e-8, None, None, None) == -1


# ---- bcd_cli --neighbour-layer: every argument error comes before any device work (no device is visible to the child) ----------------------------------
def _cli(*args):
    import subprocess
    import bcd_amd.core as core
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)


def _write_frame(tmp_path, name, seed):
    import bcd_amd.core as core
    col, ns, hist, cov = core.synthetic_scene(24, 20, 4, seed, 0.15, 0.0)
    stem = str(tmp_path / name)
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    return stem, col, cov


def test_cli_usage_names_the_neighbour_layer_argument():
    assert "--neighbour-layer <color> <cov>" in _cli("--help").stdout


def test_cli_neighbour_layer_argument_errors(tmp_path):
    import bcd_amd.core as core
    a, col, cov = _write_frame(tmp_path, "a", 5)
    b, _, _ = _write_frame(tmp_path, "b", 6)
    out, lout = str(tmp_path / "out.exr"), str(tmp_path / "layer_out.exr")
    base = ["-i", a + ".exr", "-o", out, "-p", "0"]
    layer = ["--layer", a + ".exr", a + "_cov.exr", lout]
    r = _cli(*base, "--neighbour", b + ".exr", "--neighbour-layer", b + ".exr")                           # too few operands
    assert r.returncode != 0 and "after --neighbour-layer" in r.stdout, r.stdout + r.stderr
    r = _cli(*base, *layer, "--neighbour-layer", b + ".exr", b + "_cov.exr", "--neighbour", b + ".exr")  # ahead of every --neighbour
    assert r.returncode != 0 and "follows the --neighbour" in r.stdout, r.stdout + r.stderr
    r = _cli(*base, *layer, "--neighbour", b + ".exr", "--neighbour-layer", str(tmp_path / "nothing.exr"), b + "_cov.exr")
    assert r.returncode != 0 and "couldn't load neighbour layer color image file" in r.stdout, r.stdout + r.stderr
    r = _cli(*base, *layer, "--neighbour", b + ".exr")                                                    # a neighbour without its layer
    assert r.returncode != 0 and "0 --neighbour-layer argument(s) but there are 1 --layer" in r.stdout, r.stdout + r.stderr
    r = _cli(*base, "--neighbour", b + ".exr", "--neighbour-layer", b + ".exr", b + "_cov.exr")          # a neighbour's layer without a --layer
    assert r.returncode != 0 and "1 --neighbour-layer argument(s) but there are 0 --layer" in r.stdout, r.stdout + r.stderr
    core.write_exr(b + "_small.exr", np.ascontiguousarray(col[:-2]), False)
    r = _cli(*base, *layer, "--neighbour", b + ".exr", "--neighbour-layer", b + "_small.exr", b + "_cov.exr")   # another size
    assert r.returncode != 0 and "neighbour layer" in r.stdout and "24x20" in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(out) and not os.path.exists(lout)
