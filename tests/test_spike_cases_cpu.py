"""CPU tests of the spike prefilter through a source map: the frames of tests/spike_cases.py are what they claim to be, a gather through the map
reproduces the filter (the oracle's and the reference's own compiled one) bit for bit, the C ABI declares and exports the new entry points, and
bcd_cli --prefilter-layers gets past argument checking.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bcd_amd.core as core
import bcd_amd.hip as bh
import oracle_lib as ol
import spike_cases as sc
import spike_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
_GOLDEN = os.path.join(ROOT, "tests", "golden")


def _ident(M):
    return np.arange(M.size, dtype=np.int32).reshape(M.shape)


@pytest.mark.parametrize("name", sc.ALL)
def test_cases_are_what_they_claim(name):
    col, ns, hist, cov, factor = sc.get(name)
    H, W, _ = col.shape
    M = sr.source_map(col, factor)
    moved = int(np.count_nonzero(M != _ident(M)))
    print("%s: %dx%d moved %d (%.1f %%), chains %d, offsets %s" % (name, W, H, moved, 100.0 * moved / M.size, sr.chains(M), sr.max_offsets(M)))
    assert M.min() >= 0 and M.max() < W * H
    dl, dc = sr.max_offsets(M)
    assert dl <= 2 and dc <= 2                          # border pixels use the window centred one pixel inward
    Mn, flags = sr.numpy_map(col, factor)
    assert np.array_equal(M, Mn)                        # the oracle and the NumPy statement of the rule agree, non-finite windows included
    if name in sc.NAMED:
        assert moved > 0
    if name == "96x64":
        assert sr.chains(M) >= 1                        # the case an in-place gather gets wrong
        inplace = col.reshape(-1, 3).copy()
        for p, q in enumerate(M.reshape(-1)):
            inplace[p] = inplace[q]
        assert not np.array_equal(sr.bits(inplace.reshape(col.shape)), sr.bits(sr.gather(col, M)))
    if name == "constant":
        assert moved == 0 and not flags.any()
    if name == "all_spikes":
        assert flags.all() and moved > M.size // 2
    if name == "nonfinite":
        assert not np.isfinite(col).all() and (col < 0).any() and moved > 0
        for l, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert not np.isfinite(col[l, c]).all() or (col[l, c] < 0).any()


@pytest.mark.parametrize("name", sc.ALL)
def test_gather_through_the_map_is_the_filter_bit_for_bit(name):
    col, ns, hist, cov, factor = sc.get(name)
    M = sr.source_map(col, factor)
    want = ol.oracle_ops()["spike"](col, ns, hist, cov, factor)
    for tag, img, w in zip(("colours", "sample counts", "histograms", "covariances"), (col, ns, hist, cov), want):
        assert np.array_equal(sr.bits(sr.gather(img, M)), sr.bits(w)), tag


def test_gather_reproduces_the_reference_filters_stored_outputs():
    """tests/golden/ref_spike.npz: inputs and the outputs of the reference's own compiled SpikeRemovalFilter"""
    g = np.load(os.path.join(_GOLDEN, "ref_spike.npz"))
    M = sr.source_map(g["mean"], float(g["factor"]))
    assert np.count_nonzero(M != _ident(M)) > 0
    for src, dst in (("mean", "o_mean"), ("ns", "o_ns"), ("hist", "o_hist"), ("cov", "o_cov")):
        assert np.array_equal(sr.bits(sr.gather(g[src], M)), sr.bits(g[dst])), src


def test_header_declares_and_library_exports_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    assert re.search(r"int bcd_hip_spike_map\(bcd_hip_ctx \*ctx, const float \*d_colors, int W, int H, float factor, int32_t \*d_map, int32_t \*d_moved", txt)
    assert re.search(r"int bcd_hip_spike_apply\(bcd_hip_ctx \*ctx, const int32_t \*d_map, int W, int H, int depth, const float \*const \*d_src, "
                     r"float \*const \*d_dst, int nb_images", txt)
    assert re.search(r"typedef struct \{ const float \*d_colors, \*d_covariances; float \*d_colors_out, \*d_covariances_out; \} bcd_hip_spike_layer;", txt)
    assert re.search(r"int bcd_hip_spike_filter_layers\(bcd_hip_ctx \*ctx, const float \*d_nsamples, const float \*d_histograms", txt)
    assert re.search(r"typedef struct \{ float spike_factor; int32_t zero_bad_values; int32_t filter_layers; \} bcd_hip_layers_host_options;", txt)
    assert re.search(r"int bcd_hip_denoise_layers_host_ex\(bcd_hip_ctx \*ctx, const float \*h_nsamples, const float \*h_histograms, int W, int H, int D, "
                     r"int nb_scales,\s*const bcd_hip_params \*prm, const bcd_hip_layers_host_options \*opt,\s*const bcd_hip_host_layer \*layers, int nb_layers\);", txt)
    lib = bh.lib()
    for s in ("bcd_hip_spike_map", "bcd_hip_spike_apply", "bcd_hip_spike_filter_layers", "bcd_hip_denoise_layers_host_ex"):
        assert hasattr(lib, s) and s in bh.SYMBOLS, s
    assert C.sizeof(bh.SpikeLayer) == 4 * C.sizeof(C.c_void_p)
    assert C.sizeof(bh.LayersHostOptions) == 12
    assert C.sizeof(bh.HostLayer) == 3 * C.sizeof(C.c_void_p)
    assert hasattr(core.lib(), "bcdcore_denoise_layers_ex")


def test_new_calls_without_a_context_are_errors_not_crashes():
    L = bh.lib()
    assert L.bcd_hip_spike_map(None, None, 8, 8, 2.0, None, None) == -1
    assert L.bcd_hip_spike_apply(None, None, 8, 8, 3, None, None, 1) == -1
    assert L.bcd_hip_spike_filter_layers(None, None, None, 8, 8, 60, 2.0, None, None, None, 1, None, None) == -1
    opt = bh.LayersHostOptions(2.0, 0, 1)
    assert L.bcd_hip_denoise_layers_host_ex(None, None, None, 8, 8, 60, 1, None, C.byref(opt), None, 2) == -1


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_usage_names_the_flag():
    r = _cli("--help")
    assert "--prefilter-layers" in r.stdout


def test_cli_prefilter_layers_gets_past_argument_checking(tmp_path):
    col, ns, hist, cov = core.synthetic_scene(24, 20, 4, 3, 0.2, 0.0)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    out, lout = str(tmp_path / "out.exr"), str(tmp_path / "layer_out.exr")
    layer = ["--layer", stem + ".exr", stem + "_cov.exr", lout]
    r = _cli("-i", stem + ".exr", "-o", out, *layer)                              # -p defaults to 1: refused, and the refusal names the flag
    assert r.returncode != 0 and "add -p 0" in r.stdout and "--prefilter-layers" in r.stdout
    for extra in ([], ["-p", "1"]):
        r = _cli("-i", stem + ".exr", "-o", out, *extra, *layer, "--prefilter-layers")
        text = r.stdout + r.stderr
        assert "add -p 0" not in text and "ERROR in program arguments" not in text, text
        assert r.returncode != 0 and "no usable HIP device" in text, text         # it got as far as asking for a device
