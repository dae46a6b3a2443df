"""CPU tests around the in-place spike prefilter and the prefilter of every frame (bcd_hip_spike_apply_inplace / _filter_layers_inplace,
bcd_hip_denoise_temporal_host_ex, bcd_hip_sequence_set_prefilter; DESIGN 13 "In place", 16 "Prefilter").  No GPU needed.
  1. the map generator of tests/spike_inplace_cases.py: every case has the structure it names;
  2. the mutants a passing kernel cannot be: a sequential in-place loop, ascending or descending, differs from the reference on the cycle and chain cases;
  3. the new prototypes and structures agree with the header, and the calls refuse a null handle;
  4. bcd_cli --prefilter-frames is accepted where it applies, and today's message stays without it;
  5. bcd::Denoiser and bcd::SequenceDenoiser with setSpikePrefilterFrames pass their refusals and fail only for want of a device; without the switch they
     refuse with today's messages."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spike_inplace_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ic.SIZES + (ic.REAL_SIZE,)


def _ident(n):
    return np.arange(n)


def _image(W, H, d):
    return np.arange(W * H * d, dtype=np.float32).reshape(H, W, d)          # every value its own: a wrong source shows


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_every_case_has_the_structure_it_names(W, H):
    n = W * H
    for name in ic.CASES:
        M = ic.make(name, W, H)
        assert M.shape == (H, W) and M.dtype == np.int32, name
        assert np.array_equal(M, ic.make(name, W, H)), name                  # deterministic
    m = {name: ic.effective(ic.make(name, W, H)) for name in ic.CASES}
    mv = {name: np.flatnonzero(m[name] != _ident(n)) for name in ic.CASES}
    assert mv["identity"].size == 0
    assert mv["one"].size == 1
    p, q = mv["cycle2"]
    assert q == p + 1 and m["cycle2"][p] == q and m["cycle2"][q] == p         # a swap of two adjacent pixels
    c = mv["cycle5"]
    assert c.size == 5
    walk, at = [], c[0]
    for _ in range(5):
        walk.append(at)
        at = m["cycle5"][at]
    assert at == c[0] and sorted(walk) == sorted(c)                          # one cycle through the five
    up, down = ic.chain_paths(W, H)
    assert len(up) >= 4 and len(down) >= 4 and not set(up) & set(down)
    for path in (up, down):
        for a, b in zip(path[:-1], path[1:]):
            assert m["chain"][a] == b                                        # every pixel reads the next one of its path ...
        assert m["chain"][path[-1]] == path[-1]                              # ... and the last one stays
    assert all(b > a for a, b in zip(up[:-1], up[1:])) and all(b < a for a, b in zip(down[:-1], down[1:]))
    assert mv["chain"].size == len(up) + len(down) - 2
    assert any(a // W != b // W for a, b in zip(up[:-1], up[1:]))            # across a line boundary
    if n > 130:
        assert any(a // 64 != b // 64 for a, b in zip(up[:-1], up[1:]))      # across a multiple of 64 in the linear index
    assert mv["permutation"].size == n and np.array_equal(np.sort(m["permutation"]), _ident(n))    # a permutation, 100 % moved
    at, steps = 0, 0
    while True:
        at, steps = m["permutation"][at], steps + 1
        if at == 0:
            break
    assert steps == n                                                        # one cycle
    assert np.all(m["fan_first"] == 0) and mv["fan_first"].size == n - 1
    assert np.all(m["fan_last"] == n - 1) and mv["fan_last"].size == n - 1
    if n >= 100:
        assert 0.3 * n < mv["half"].size < 0.7 * n
    raw = ic.make("outside", W, H).reshape(-1).astype(np.int64)
    assert raw[0] < 0 or raw[0] >= n
    assert np.any(raw < 0) and np.any(raw >= n)
    if n >= 100:
        assert {int(np.iinfo(np.int32).max), int(np.iinfo(np.int32).min), n, -1} <= set(raw.tolist())
    assert np.all((m["outside"] >= 0) & (m["outside"] < n)) and np.all(m["outside"][(raw < 0) | (raw >= n)] == _ident(n)[(raw < 0) | (raw >= n)])
    for name in ic.CASES:
        assert ic.moved(ic.make(name, W, H)) == mv[name].size, name


def test_the_real_maps_move_pixels_next_to_each_other():
    """the oracle's decision on the spiky 40 x 28 frames (32 spp, spike probability 0.01) at factor 2: 69 to 75 moved pixels, some of them adjacent"""
    import spike_ref as sr
    W, H = ic.REAL_SIZE
    for s, seed in enumerate(ic.REAL_SEEDS):
        M = ic.make("real", W, H, s)
        m = ic.effective(M)
        moved = m != _ident(W * H)
        grid = moved.reshape(H, W)
        adjacent = int(np.count_nonzero(grid[:, 1:] & grid[:, :-1]) + np.count_nonzero(grid[1:] & grid[:-1]))
        print("seed %d: %d of %d moved, %d adjacent pairs, %d chains" % (seed, moved.sum(), W * H, adjacent, sr.chains(M)))
        assert 60 <= moved.sum() <= 85 and adjacent >= 1
        assert np.all(np.abs(m // W - _ident(W * H) // W) <= 2) and np.all(np.abs(m % W - _ident(W * H) % W) <= 2)   # a source is in the pixel's 3 x 3 window (one inward at the border)


# ---- 2. the mutants -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ic.SIZES)
def test_a_sequential_in_place_loop_is_wrong_on_cycles_and_chains(W, H):
    for depth in (1, 3):
        img = _image(W, H, depth)
        for name in ("cycle2", "cycle5", "chain", "permutation"):
            M = ic.make(name, W, H)
            want = ic.reference(img, M)
            assert not np.array_equal(ic.sequential(img, M), want), (name, "ascending")
            assert not np.array_equal(ic.sequential(img, M, descending=True), want), (name, "descending")
        for name in ("identity", "one", "fan_first", "fan_last"):           # ... and right where nothing read is written first
            M = ic.make(name, W, H)
            assert np.array_equal(ic.sequential(img, M), ic.reference(img, M)), name


def test_reference_is_the_gather_of_the_out_of_place_tests():
    import spike_ref as sr
    W, H = 65, 5
    for name in ("half", "permutation", "chain"):
        M = ic.make(name, W, H)
        for d in ic.DEPTHS:
            img = _image(W, H, d)
            assert np.array_equal(ic.reference(img, M), sr.gather(img, M))
    M = ic.make("outside", W, H)
    img = _image(W, H, 3)
    assert np.array_equal(ic.reference(img, M), sr.gather(img, ic.effective(M).reshape(H, W)))


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------------------------------------------
NEW = ["bcd_hip_spike_apply_inplace", "bcd_hip_spike_filter_layers_inplace", "bcd_hip_denoise_temporal_host_ex", "bcd_hip_sequence_set_prefilter",
       "bcd_hip_sequence_prefilter_info"]


def test_the_new_prototypes_agree_with_the_header():
    import bcd_amd._prototypes as bp
    import bcd_amd.hip as bh
    from test_abi_prototypes import header_prototypes, header_structures
    want, structs = header_prototypes(), header_structures()
    L = bh.lib()
    for name in NEW:
        assert name in want and name in bp.PROTOTYPES and name in bh.SYMBOLS and hasattr(L, name), name
        assert bp.PROTOTYPES[name][0] is want[name][0] and list(bp.PROTOTYPES[name][1]) == want[name][1], name
    for s, mirror in (("bcd_hip_spike_layer_inplace", bp.SpikeLayerInplace), ("bcd_hip_temporal_host_options", bp.TemporalHostOptions)):
        assert [f for f, _ in mirror._fields_] == [f for f, _, _, _ in structs[s]], s
    assert C.sizeof(bp.SpikeLayerInplace) == 2 * C.sizeof(C.c_void_p) and C.sizeof(bp.TemporalHostOptions) == 2 * C.sizeof(C.c_void_p)
    assert bp.PROTOTYPES["bcd_hip_denoise_temporal_host_ex"][1][-1] is C.POINTER(bp.TemporalHostOptions)
    # the host call takes the arguments of the moments host call, the histograms behind the sample counts, D behind H, the options last
    mom = list(bp.PROTOTYPES["bcd_hip_denoise_temporal_moments_host"][1])
    assert list(bp.PROTOTYPES["bcd_hip_denoise_temporal_host_ex"][1]) == mom[:2] + [C.c_void_p] + mom[2:7] + [C.c_int] + mom[7:] + [C.POINTER(bp.TemporalHostOptions)]
    for name in ("spike_apply_inplace", "spike_filter_layers_inplace", "denoise_temporal_host_ex"):
        assert hasattr(bh.Context, name), name
    assert hasattr(bh.Sequence, "set_prefilter") and hasattr(bh.Sequence, "prefilter_info")


def test_new_calls_without_a_handle_are_errors_not_crashes():
    import bcd_amd.hip as bh
    L = bh.lib()
    n, m = C.c_int64(0), C.c_int64(0)
    opt = bh.TemporalHostOptions(2.0, None)
    assert L.bcd_hip_spike_apply_inplace(None, None, 8, 8, None, None, 1, None) == -1
    assert L.bcd_hip_spike_filter_layers_inplace(None, None, None, 8, 8, 60, 2.0, None, 1, None, None) == -1
    assert L.bcd_hip_denoise_temporal_host_ex(None, None, None, None, 1, None, 8, 8, 60, 1, None, 0.0, None, 1, None, None, C.byref(opt)) == -1
    assert L.bcd_hip_sequence_set_prefilter(None, 2.0) == -1
    assert L.bcd_hip_sequence_prefilter_info(None, C.byref(n), C.byref(m)) == -1


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    import bcd_amd.core as core
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # (no device is visible to the child: what it reports, it reports before any device work)
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=env)


def test_cli_usage_names_the_flag():
    assert "--prefilter-frames" in _cli("--help").stdout


def test_cli_sequence_takes_the_flag(tmp_path):
    seq = ["--sequence-in", str(tmp_path / "in.%04d.exr"), "--sequence-out", str(tmp_path / "out.%04d.exr"), "--first", "0", "--last", "3"]
    r = _cli(*seq)                                                           # the CLI's default is -p 1: today's message, with the new way out
    assert r.returncode == 1 and "ERROR in program arguments" in r.stdout and "add -p 0" in r.stdout and "--prefilter-frames" in r.stdout
    for extra in ([], ["-p", "1"], ["-p", "1", "--p-factor", "1.5"], ["-p", "0"]):     # with the flag: as far as the first frame's file
        for order in (seq + ["--prefilter-frames"] + extra, ["--prefilter-frames"] + extra + seq):
            r = _cli(*order)
            assert r.returncode == 1 and "couldn't load input color image file" in r.stdout and "in.0000.exr" in r.stdout, (order, r.stdout, r.stderr)
            assert "add -p 0" not in r.stdout and "HIP device" not in r.stdout + r.stderr
    r = _cli(*(seq + ["--prefilter-frame"]))                                 # a misspelt flag stays an error
    assert r.returncode == 1 and "ERROR in program arguments" in r.stdout


def _write_frame(core, stem, col, ns, hist, cov):
    core.write_exr(stem + ".exr", col, False)
    core.write_exr(stem + "_hist.exr", core.merge_hist_ns(hist, ns), True)
    core.write_exr(stem + "_cov.exr", cov, True)


def test_cli_neighbours_take_the_flag(tmp_path):
    """-i with --neighbour and the default -p 1: with the flag the call gets past every refusal and fails for want of a device (without it, a call with
    histogram neighbours is refused by the library behind the device request: tests/test_gpu_temporal_prefilter.py); --layer beside --neighbour needs no
    --prefilter-layers then; under --moment-selection the library's refusal comes ahead of the device and is gone with the flag"""
    import bcd_amd.core as core
    a = core.synthetic_scene(24, 20, 4, 3, 0.2, 0.0)
    b = core.synthetic_scene(24, 20, 4, 4, 0.2, 0.0)
    f0, f1, out = str(tmp_path / "f0"), str(tmp_path / "f1"), str(tmp_path / "out.exr")
    _write_frame(core, f0, *a)
    _write_frame(core, f1, *b)
    base = ["-i", f0 + ".exr", "-o", out, "--neighbour", f1 + ".exr"]
    r = _cli(*base, "--prefilter-frames")
    text = r.stdout + r.stderr
    assert r.returncode != 0 and "spike prefilter" not in text and "ERROR in program arguments" not in text and "no usable HIP device" in text, text
    layer = ["--layer", f0 + ".exr", f0 + "_cov.exr", str(tmp_path / "l.exr"), "--neighbour-layer", f1 + ".exr", f1 + "_cov.exr"]
    r = _cli(*base, *layer)
    assert r.returncode != 0 and "add -p 0" in r.stdout
    r = _cli(*base, *layer, "--prefilter-frames")
    text = r.stdout + r.stderr
    assert r.returncode != 0 and "add -p 0" not in text and "ERROR in program arguments" not in text and "no usable HIP device" in text, text
    r = _cli(*base, "--prefilter-frames", "-p", "0")                         # -p 0: accepted, nothing to do
    text = r.stdout + r.stderr
    assert "ERROR in program arguments" not in text and "no usable HIP device" in text, text
    r = _cli("-i", f0 + ".exr", "-o", out, *layer[:4], "--prefilter-frames")   # no neighbour: the switch changes nothing, --layer keeps its refusal
    assert r.returncode != 0 and "add -p 0" in r.stdout
    # the moment selection: sample counts from one-channel files, no histogram is read
    core.write_exr(f0 + "_ns.exr", a[1].reshape(20, 24, 1), True)
    core.write_exr(f1 + "_ns.exr", b[1].reshape(20, 24, 1), True)
    mom = base + ["--moment-selection", "--nsamples", f0 + "_ns.exr", "--neighbour-nsamples", f1 + "_ns.exr"]
    r = _cli(*mom)
    assert r.returncode != 0 and "do not combine with the spike prefilter" in r.stdout + r.stderr and "HIP device" not in r.stdout + r.stderr, r.stdout + r.stderr
    r = _cli(*mom, "--prefilter-frames")
    text = r.stdout + r.stderr
    assert r.returncode != 0 and "spike prefilter" not in text and "no usable HIP device" in text, text


# ---- 5. the classes ---------------------------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import bcd_amd.core as core
W, H, D = 12, 9, 60
col, ns, hist, cov = np.zeros((H, W, 3), np.float32), np.ones((H, W), np.float32), np.zeros((H, W, D), np.float32), np.zeros((H, W, 6), np.float32)
kind, kw = sys.argv[1], eval(sys.argv[2])
if kind == "temporal":
    ok = core.denoise_temporal(col, ns, hist, cov, [(col, ns, hist, cov)], **kw)[0]
elif kind == "layers":
    ok = core.denoise_temporal_layers(ns, hist, [(col, cov), (col, cov)], [(ns, hist, [(col, cov), (col, cov)])], **kw)[0]
elif kind == "moments":
    ok = core.denoise_temporal_moments(ns, [(col, cov), (col, cov)], [(ns, [(col, cov), (col, cov)])], **kw)[0]
elif kind == "moments1":
    ok = core.denoise_temporal_moments(ns, [(col, cov)], [(ns, [(col, cov)])], **kw)[0]
elif kind == "sequence":
    ok = core.denoise_sequence([(col, ns, hist, cov)] * 2, **kw)[0]
else:
    ok = core.denoise_sequence([(col, ns, hist, cov)] * 2, layers=[[(col, cov)]] * 2, **kw)[0]
print("OK" if ok else "REFUSED")
""" % ROOT


def _child(kind, **kw):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _CHILD, kind, repr(kw)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "REFUSED" in r.stdout, (kind, kw, r.stdout, r.stderr)
    return r.stderr


# kind -> a refusal of the class itself that must still come first (None: the class has none that this wrapper can provoke)
_OWN_REFUSAL = {"temporal": None, "layers": None, "moments": (dict(drop_layers=1), "exactly one layer"), "moments1": None,
                "sequence": (dict(radius=3), "temporal radius"), "sequence_modes": (dict(radius=3), "temporal radius")}


@pytest.mark.parametrize("kind", sorted(_OWN_REFUSAL))
def test_classes_with_the_switch_fail_only_for_want_of_a_device(kind):
    """(the child sees no device, wherever the test runs)"""
    import inspect
    import bcd_amd.core as core
    fn = {"temporal": core.denoise_temporal, "layers": core.denoise_temporal_layers, "moments": core.denoise_temporal_moments, "moments1": core.denoise_temporal_moments,
          "sequence": core.denoise_sequence, "sequence_modes": core.denoise_sequence}[kind]
    named = inspect.signature(fn, follow_wrapped=False).parameters["prefilter_frames"]           # a keyword of its own, not swallowed by a **kw
    assert named.kind is inspect.Parameter.KEYWORD_ONLY and named.default == 0.0
    err = _child(kind, prefilter_frames=2.0)
    assert "no usable HIP device" in err and "spike prefilter" not in err, err
    if _OWN_REFUSAL[kind]:
        kw, message = _OWN_REFUSAL[kind]
        err = _child(kind, prefilter_frames=2.0, **kw)
        assert message in err and "HIP device" not in err, err


def test_without_the_switch_todays_messages_remain():
    """setSpikePrefilter without setSpikePrefilterFrames (prefilter_without_switch; bit 3 of `unsupported` / bit 1 of `break_settings` on a sequence)"""
    for kind, kw in (("sequence", dict(unsupported=8)), ("sequence_modes", dict(break_settings=2)), ("sequence", dict(prefilter_without_switch=2.0)),
                     ("sequence_modes", dict(prefilter_without_switch=2.0))):
        err = _child(kind, **kw)
        assert "no spike prefilter" in err and "HIP device" not in err, (kind, kw, err)
    err = _child("moments1", prefilter_without_switch=2.0)
    assert "do not combine with the spike prefilter" in err and "HIP device" not in err, err
    err = _child("moments", prefilter_without_switch=2.0)                          # (beside added layers the layers' own refusal comes first, as it did)
    assert "not available with added colour layers" in err and "HIP device" not in err, err
    import bcd_amd.core as core
    import inspect
    for fn in (core.denoise_temporal, core.denoise_temporal_layers, core.denoise_temporal_moments, core.denoise_sequence):
        assert "prefilter_frames" in inspect.signature(fn, follow_wrapped=False).parameters, fn
