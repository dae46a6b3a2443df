"""CPU tests of libbcdcore (the C++ mirror of the reference's include/bcd API): SamplesAccumulator and Utils against
the oracle / reference fixtures, synthetic scenes, and IDenoiser input validation (no GPU needed: validation runs
before any device work)."""
import os

import numpy as np
import pytest

import bcd_amd.core as core
import oracle_lib as ol

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_samples_accumulator_matches_reference_fixture():
    f = np.load(os.path.join(G, "ref_accumulator.npz"))
    got = core.accumulate(f["samples"], int(f["W"]), int(f["H"]))
    for g, k in zip(got, ("ns", "mean", "cov", "hist")):
        assert same(g, f[k]), k


def test_samples_accumulator_other_histogram_parameters():
    samples, _ = ol.synth_samples(12, 9, 7, seed=2, sigma=0.6, spike_prob=0.2)
    for nbins, gamma, maxval in [(20, 2.2, 2.5), (10, 1.0, 1.0), (32, 3.0, 0.0)]:
        a = core.accumulate(samples, 12, 9, nbins, gamma, maxval)
        b = ol.oracle_ops()["accumulate"](samples, 12, 9, nbins, gamma, maxval)
        assert all(same(x, y) for x, y in zip(a, b))
        assert np.allclose(a[3].sum(-1), 3 * a[0][..., 0])       # each sample adds weight 1 to each channel's histogram


def test_spike_filter_host_loops_match_the_reference_fixture_bit_for_bit():
    """SpikeRemovalFilter::filterOnHost -- what filter() runs when no HIP device is usable -- against tests/golden/ref_spike.npz, the outputs of the
    reference's own SpikeRemovalFilter.cpp (float-abs semantics); product code, nothing of oracle/ in it.  On a box without a device filter()
    itself takes this path: the images must never come back untouched (the reference's filter is a host function)"""
    f = np.load(os.path.join(G, "ref_spike.npz"))
    got = core.spike_filter_host(f["mean"], f["ns"], f["hist"], f["cov"], float(f["factor"]))
    for g, k in zip(got, ("o_mean", "o_ns", "o_hist", "o_cov")):
        assert same(g, f[k]), k
    assert not same(f["mean"], f["o_mean"])          # (the fixture does contain spikes)
    via_filter = core.spike_filter(f["mean"], f["ns"], f["hist"], f["cov"], float(f["factor"]))   # device if there is one, else the host loops
    for g, k in zip(via_filter, ("o_mean", "o_ns", "o_hist", "o_cov")):
        assert same(g, f[k]), k
    # a frame too small for a 3 x 3 neighbourhood is left alone
    tiny = [np.ascontiguousarray(f[k][:2, :5]) for k in ("mean", "ns", "hist", "cov")]
    assert all(same(a, b) for a, b in zip(core.spike_filter_host(*tiny), tiny))


def test_histogram_packing_roundtrip():
    f = np.load(os.path.join(G, "ref_pyramid.npz"))
    m = core.merge_hist_ns(f["hist"], f["ns"])
    assert m.shape[-1] == 61 and same(m[..., 60:], f["ns"]) and same(m[..., :60], f["hist"])
    h, n = core.split_hist_ns(m)
    assert same(h, f["hist"]) and same(n, f["ns"])


def test_synthetic_scene_is_seeded_and_band_consistent():
    a = core.synthetic_scene(40, 30, 4, seed=5)
    b = core.synthetic_scene(40, 30, 4, seed=5)
    c = core.synthetic_scene(40, 30, 4, seed=6)
    assert all(same(x, y) for x, y in zip(a, b)) and not same(a[0], c[0])
    band = core.synthetic_scene(40, 30, 4, seed=5, first_line=8, nb_lines=13)
    assert all(same(x[8:21], y) for x, y in zip(a, band))
    col, ns, hist, cov = a
    assert (ns == 4).all() and np.isfinite(cov).all() and (hist >= 0).all()


def test_denoiser_rejects_bad_inputs_like_the_reference():
    col, ns, hist, cov = core.synthetic_scene(16, 12, 2)
    assert core.denoise(None, ns, hist, cov)[0] is False             # nullptr input (Denoiser.cpp:266-293)
    assert core.denoise(col, ns, hist, cov, hist_width_override=8)[0] is False  # size mismatch (:321-346)
    assert core.denoise(col[:0], ns[:0], hist[:0], cov[:0])[0] is False  # empty (:294-320)


def test_explicit_cpu_request_is_refused_in_strict_mode(capfd, monkeypatch):
    """DenoiserParameters::m_useCuda = false asks for the CPU/OpenMP loop of the reference (src/core/Denoiser.cpp:99-110,241-265), which this library
    does not have.  Default (round 5): the request is declined with a note and the HIP device serves the call (GPU test
    test_cpu_request_is_declined_with_a_note_and_served_by_the_device); under BCD_STRICT_CPU_REQUEST=1 it is refused -- `false` and a message on
    cerr, on any host, with or without a GPU, before any device work"""
    monkeypatch.setenv("BCD_STRICT_CPU_REQUEST", "1")
    col, ns, hist, cov = core.synthetic_scene(16, 12, 2)
    for nscales in (1, 2):
        ok, out, _ = core.denoise(col, ns, hist, cov, nscales, use_cuda=False)
        assert ok is False and not out.any()
    assert "m_useCuda = false" in capfd.readouterr().err


def test_samples_accumulator_thread_safe_variant():
    """SamplesAccumulatorThreadSafe::addSampleThreadSafely (declared by the reference, include/bcd/core/SamplesAccumulator.h:82-97, but
    left without a constructor and without a lock, src/core/SamplesAccumulator.cpp:156-165): 8 threads feeding the same pixels give the
    sequential statistics up to the summation order of each pixel's samples"""
    samples, _ = ol.synth_samples(9, 7, 64, seed=4, sigma=0.5, spike_prob=0.1)   # 64 samples per pixel, consecutive in the list:
    a = core.accumulate(samples, 9, 7)                                           # threads (round-robin) meet on every pixel
    b = core.accumulate_threadsafe(samples, 9, 7, threads=8)
    assert same(a[0], b[0])                                                      # sample counts: integer-valued sums, exact
    for x, y in zip(a[1:], b[1:]):
        assert np.allclose(x, y, rtol=2e-5, atol=1e-6)
    one = core.accumulate_threadsafe(samples, 9, 7, threads=1)
    assert all(same(x, y) for x, y in zip(a, one))                               # one thread: the very same sequence


def test_jacobi_quad_schedule_matches_the_kernel_constants():
    """tools/jacobi_schedule.py builds and CHECKS the resolvable 2-(28,4,1) design behind k_jacobi27_quads (every pair of slots in one quad per
    sweep, every slot home after nine super-rounds, conflict-free LDS placement); the tables it prints must be the ones compiled into
    bcd_amd/csrc/bayes27_jacobi.h"""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "jacobi_schedule.py")], capture_output=True, text=True, check=True).stdout
    src = open(os.path.join(root, "bcd_amd", "csrc", "bayes27_jacobi.h")).read()
    for name in ("JSX", "JSY", "JPLACE"):
        want = re.search(r"constexpr int %s\[28\] = \{([^}]*)\}" % name, out).group(1).split(",")
        got = re.search(r"constexpr int %s\[28\] = \{([^}]*)\}" % name, src).group(1).split(",")
        assert [int(v) for v in want] == [int(v) for v in got], name
    assert re.search(r"constexpr int JIDLE_ROW = (\d+);", out).group(1) == re.search(r"constexpr int JIDLE_ROW = (\d+);", src).group(1)


def test_strip_visiting_order_is_the_reference_list():
    """bcd_hip_visit_order mode 2 against a restatement of reorderPixelSetJumpNextChunk (src/core/Denoiser.cpp:393-414): chunks of
    (W - 2w) * 2b pixels, the even ones first, then the odd ones; what is left of a partial chunk stays where it was"""
    import bcd_amd.hip as bh

    def reference_list(W, H, w, b):
        Wm, Hm = W - 2 * w, H - 2 * w
        lst = [(w + i // Wm) * W + w + i % Wm for i in range(Wm * Hm)]
        chunk, out, o = Wm * 2 * b, None, 0
        nfull = len(lst) // chunk
        out = list(lst)
        for start in range(2):
            for ch in range(start, nfull, 2):
                out[o:o + chunk] = lst[ch * chunk:(ch + 1) * chunk]
                o += chunk
        return np.array(out, np.int32)

    for W, H, w, b in [(40, 61, 1, 6), (33, 50, 1, 3), (64, 24, 1, 6), (30, 100, 2, 4), (20, 13, 1, 6), (25, 26, 1, 12)]:
        got = bh.visit_order(W, H, w, 2, bh.strip_order_seed(W, H, w, b))
        assert np.array_equal(got, reference_list(W, H, w, b)), (W, H, w, b)


REF_CLI = "/root/reference/src/cli/main.cpp"


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="the reference tree is only present in the authoring container")
def test_reference_cli_source_compiles_and_links_unchanged_against_this_library(tmp_path):
    """the boundary is source / link compatibility with `namespace bcd`.  The reference's own caller, src/cli/main.cpp (:9-26 its
    includes, :436-472 its use of IDenoiser / SpikeRemovalFilter / ImageIO), is compiled UNCHANGED against include/bcd and linked with
    libbcdcore.so; the binary then prints the reference's usage text.  Two things the reference gets from Eigen's headers are supplied on
    the command line: <cstring> / <cmath> (forced includes) and an EMPTY file for main.cpp's vestigial `#include <Eigen/Dense>` (nothing of
    Eigen is used there; the file is made in the test's temporary directory).  Nothing is computed by this binary: it is a boundary check,
    not an oracle."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(core.LIB_PATH)
    (tmp_path / "Eigen").mkdir()
    (tmp_path / "Eigen" / "Dense").write_text("")
    exe = str(tmp_path / "reference_cli")
    inc = os.path.join(root, "include")
    cmd = ["g++", "-std=c++17", "-include", "cstring", "-include", "cmath", "-I", str(tmp_path), "-I", inc, "-I", os.path.join(inc, "bcd", "core"),
           "-I", os.path.join(inc, "bcd", "io"), REF_CLI, "-o", exe, "-L" + lib_dir, "-lbcdcore", "-lbcd_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert "Missing required program argument(s): -i -h -c -o" in r.stdout and "--use-cuda" in r.stdout


def test_reference_cli_imports_resolve_against_this_library(tmp_path):
    """The link half of the test above without the reference tree: every symbol of namespace bcd that the reference's src/cli/main.cpp,
    compiled against include/bcd, leaves for a library to define (tests/golden/ref_cli_imports.txt, `make_golden.py cli`) is referenced
    by a stub that must link against libbcdcore.so without undefined symbols and load with every reference bound at start (-z now)."""
    import subprocess
    syms = [ln.strip() for ln in open(os.path.join(G, "ref_cli_imports.txt")) if ln.strip() and not ln.startswith("#")]
    assert len(syms) >= 5
    lib_dir = os.path.dirname(core.LIB_PATH)
    src = tmp_path / "stub.c"
    src.write_text("".join("extern char %s[];\n" % s for s in syms) +
                   "void *volatile keep[] = {%s};\nint main(void) { return keep[0] == 0; }\n" % ", ".join(syms))
    exe = str(tmp_path / "stub")
    cmd = ["gcc", "-fPIC", str(src), "-o", exe, "-Wl,--no-as-needed", "-L" + lib_dir, "-lbcdcore", "-lbcd_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + lib_dir, "-Wl,-z,now"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
