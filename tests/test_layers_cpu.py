"""CPU tests of the colour-layer feature (bcd_hip_denoise_layers): the C ABI declares and exports it, bcd_cli --layer refuses bad arguments before
any device work, and the C++ additions (addLayer / clearLayers) compile against include/bcd and leave a denoiser without layers as it was.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bcd_amd.core as core
import bcd_amd.hip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")


def test_header_declares_and_library_exports_the_layered_call():
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    assert re.search(r"typedef struct \{ const float \*d_colors; const float \*d_covariances; float \*d_out; \} bcd_hip_layer;", txt)
    assert re.search(r"int bcd_hip_denoise_layers\(bcd_hip_ctx \*ctx, const float \*d_nsamples, const float \*d_histograms, int W, int H, int D, "
                     r"int nb_scales,\s*const bcd_hip_params \*prm, const bcd_hip_layer \*layers, int nb_layers\);", txt)
    m = re.search(r"#define BCD_HIP_MAX_LAYERS (\d+)", txt)
    assert m and int(m.group(1)) == bh.MAX_LAYERS == 16
    lib = bh.lib()
    for s in ("bcd_hip_denoise_layers", "bcd_hip_denoise_layers_host", "bcd_hip_layer_spectral_inverses"):
        assert hasattr(lib, s) and s in bh.SYMBOLS
    assert C.sizeof(bh.Layer) == 3 * C.sizeof(C.c_void_p)
    # the stage entry points of the layered kernels (parity tests)
    assert re.search(r"typedef struct \{ const float \*d_colors; const float \*d_pixel_cov; float \*d_sum; \} bcd_hip_stage_layer;", txt)
    assert re.search(r"int bcd_hip_bayes_accumulate_layers\(bcd_hip_ctx \*ctx, const bcd_hip_stage_layer \*layers, int nb_layers,\s*const uint32_t \*d_mask, const int32_t \*d_nsim, "
                     r"const uint8_t \*d_state,\s*int W, int H, int patch_radius, int search_radius, float min_eigen_value,\s*int32_t \*d_count, int32_t \*h_redo\);", txt)
    for s in ("bcd_hip_bayes_accumulate_layers", "bcd_hip_layers_pixel_cov", "bcd_hip_layers_finalize", "bcd_hip_layers_downscale_avg", "bcd_hip_layers_downscale_cov",
              "bcd_hip_layers_merge"):
        assert hasattr(lib, s) and s in bh.SYMBOLS and re.search(r"int %s\(bcd_hip_ctx \*ctx, " % s, txt), s
    assert C.sizeof(bh.StageLayer) == 3 * C.sizeof(C.c_void_p)


def test_layered_call_without_a_context_is_an_error_not_a_crash():
    L = bh.lib()
    arr = (bh.Layer * 1)()
    assert L.bcd_hip_denoise_layers(None, None, None, 8, 8, 60, 1, None, arr, 1) == -1
    n = C.c_int32(7)
    assert L.bcd_hip_layer_spectral_inverses(None, 0, 0, C.byref(n)) == -1
    arr = (bh.StageLayer * 1)()
    assert L.bcd_hip_bayes_accumulate_layers(None, arr, 1, None, None, None, 8, 8, 1, 6, 1e-8, None, None) == -1
    for fn, args in (("bcd_hip_layers_pixel_cov", (None, 1, None, 8, 8, None, None)), ("bcd_hip_layers_finalize", (None, None, 1, None, C.c_int64(64))),
                     ("bcd_hip_layers_downscale_avg", (None, None, 1, 8, 8)), ("bcd_hip_layers_downscale_cov", (None, None, 1, None, 8, 8)), ("bcd_hip_layers_merge", (None, None, 1, 8, 8))):
        assert getattr(L, fn)(None, *args) == -1, fn


def _write_frame(tmp_path, W=24, H=20):
    col, ns, hist, cov = core.synthetic_scene(W, H, 4, 3, 0.2, 0.0)
    stem = str(tmp_path / "frame")
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)
    return stem, col, cov


def _cli(*args):
    # (no device is visible to the child: whatever it reports, it reports before any device work)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, env=env)


def test_cli_usage_names_the_layer_argument():
    r = _cli("--help")
    assert "--layer <color> <cov> <output>" in r.stdout


def test_cli_layer_with_too_few_operands(tmp_path):
    stem, _, _ = _write_frame(tmp_path)
    out = str(tmp_path / "out.exr")
    for tail in (["--layer"], ["--layer", stem + ".exr"], ["--layer", stem + ".exr", stem + "_cov.exr"]):
        r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", *tail)
        assert r.returncode != 0 and "after --layer" in r.stdout, r.stdout + r.stderr
        assert not os.path.exists(out)


def test_cli_layer_with_a_missing_file(tmp_path):
    stem, _, _ = _write_frame(tmp_path)
    out, lout = str(tmp_path / "out.exr"), str(tmp_path / "layer_out.exr")
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--layer", str(tmp_path / "nothing.exr"), stem + "_cov.exr", lout)
    assert r.returncode != 0 and "couldn't load layer color image file" in r.stdout and "nothing.exr" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--layer", stem + ".exr", str(tmp_path / "nothing_cov.exr"), lout)
    assert r.returncode != 0 and "couldn't load layer covariance matrix image file" in r.stdout
    assert not os.path.exists(out) and not os.path.exists(lout)


def test_cli_layer_with_another_size_or_the_prefilter(tmp_path):
    stem, col, cov = _write_frame(tmp_path)
    out, lout = str(tmp_path / "out.exr"), str(tmp_path / "layer_out.exr")
    core.write_exr(stem + "_small.exr", np.ascontiguousarray(col[:-2]), False)
    core.write_exr(stem + "_small_cov.exr", np.ascontiguousarray(cov[:, :-3]), True)
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--layer", stem + "_small.exr", stem + "_cov.exr", lout)
    assert r.returncode != 0 and "layer color image" in r.stdout and "24x18" in r.stdout and "24x20" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--layer", stem + ".exr", stem + "_small_cov.exr", lout)
    assert r.returncode != 0 and "layer covariance image" in r.stdout and "21x20x6" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "--layer", stem + ".exr", stem + "_cov.exr", lout)          # -p defaults to 1
    assert r.returncode != 0 and "add -p 0" in r.stdout
    r = _cli("-i", stem + ".exr", "-o", out, "-p", "0", "--layer", stem + ".exr", stem + "_cov.exr", out)
    assert r.returncode != 0 and "is also the -o output" in r.stdout
    assert not os.path.exists(out) and not os.path.exists(lout)


def test_cxx_layer_api_compiles_and_validates_against_the_public_headers(tmp_path):
    """addLayer / clearLayers / getLayers through include/bcd only: a program that checks the bookkeeping and that a bad layer is refused by
    denoise() with a message, before any device is asked for"""
    src = tmp_path / "layers.cpp"
    src.write_text(r'''
#include "Denoiser.h"
#include "MultiscaleDenoiser.h"
#include <cstdio>
using namespace bcd;
int main()
{
	const int W = 12, H = 10;
	Deepimf col(W, H, 3), ns(W, H, 1), hist(W, H, 60), cov(W, H, 6), out(W, H, 3), lcol(W, H, 3), lcov(W, H - 1, 6), lout;
	col.fill(0.5f); ns.fill(4.f); hist.fill(0.f); cov.fill(0.f); lcol.fill(0.25f); lcov.fill(0.f);
	DenoiserInputs in;
	in.m_pColors = &col; in.m_pNbOfSamples = &ns; in.m_pHistograms = &hist; in.m_pSampleCovariances = &cov;
	DenoiserOutputs o;
	o.m_pDenoisedColors = &out;
	MultiscaleDenoiser m(2);
	Denoiser d;
	HipEngineSettings* settings[2] = { &m, &d };
	IDenoiser* denoisers[2] = { &m, &d };
	for(int i = 0; i < 2; ++i)
	{
		if(!settings[i]->getLayers().empty()) return 10;
		settings[i]->addLayer(&lcol, &lcov, &lout);
		if(settings[i]->getLayers().size() != 1 || settings[i]->getLayers()[0].m_pDenoisedColors != &lout) return 11;
		denoisers[i]->setInputs(in);
		denoisers[i]->setOutputs(o);
		if(denoisers[i]->denoise()) return 12;            // the layer's covariance image is one line short
		settings[i]->clearLayers();
		settings[i]->addLayer(&lcol, nullptr, &lout);
		if(denoisers[i]->denoise()) return 13;            // null image
		settings[i]->clearLayers();
		settings[i]->addLayer(&lcol, &cov, &out);
		if(denoisers[i]->denoise()) return 14;            // writes into the primary output
		settings[i]->clearLayers();
		if(!settings[i]->getLayers().empty()) return 15;
	}
	std::printf("LAYERS OK\n");
	return 0;
}
''')
    lib_dir = os.path.dirname(core.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    exe = str(tmp_path / "layers")
    cmd = ["g++", "-std=c++17", "-Wall", "-I", inc, "-I", os.path.join(inc, "bcd", "core"), "-I", os.path.join(inc, "bcd", "io"), str(src), "-o", exe,
           "-L" + lib_dir, "-lbcdcore", "-lbcd_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "LAYERS OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
    for msg in ("added colour layer 1 must bring a 12x10x3 color image", "nullptr for an image of added colour layer 1", "writes into the primary output image"):
        assert msg in r.stderr


def test_denoiser_without_layers_validates_as_before():
    """the zero-layer denoise() is the reference's: same refusals (the existing host-library tests cover the messages), no layer bookkeeping in the way"""
    col, ns, hist, cov = core.synthetic_scene(16, 12, 2)
    ok, _, _ = core.denoise(None, ns, hist, cov, 1)
    assert not ok
    ok, _, _ = core.denoise(col, ns, hist, cov, 1, hist_width_override=9)
    assert not ok
    ok, _ = core.denoise_layers([(col, cov), (col, cov)], ns, hist, size_mismatch_layer=1)
    assert not ok
