"""CPU tests of what the modes of a sequence rest on (bcd_hip_sequence_create_mode; DESIGN 16, "Modes"): the cross moment distance and the cross feature
distance are symmetric under the swap of the two frames as the histogram distance is, so the cross masks of (B -> A) are the transposition
(tests/sequence_ref.transpose_masks) of those of (A -> B), bit for bit, and the transposition distributes over the AND of the feature gate.

  * random float32 frames at 20x14 and 13x9, b = 6 (13x9: a frame smaller than the window) and b = 2, thresholds at the median of the reference's own finite
    distances, so that the masks are neither empty nor full (asserted); the frames with special values of moments_cross_cases.special_pair (zeros, equal
    pixels, NaN and infinite entries) and guide_cross_cases.special, which the references define;
  * the feature symmetry with and without variances; transpose(gate(m, g)) == gate(transpose(m), transpose(g)) on reference masks and on random words;
  * the moving-edge scene of guide_cross_cases.benefit_scene: the feature gate removes at least one bit of a cross mask and leaves at least one, and the
    gated masks of (B -> A) are the transposition of those of (A -> B);
  * the refusals of bcd::SequenceDenoiser with setFrameSettings(true) (through libbcdcore.so, in a child process) and of bcd_cli --sequence-in with the
    --sequence-layer / --sequence-moments / --sequence-features arguments, with no device visible; the new prototypes agree with the header."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guide_cross_cases as gc
import guide_cross_ref as gx
import moments_cross_cases as xc
import moments_cross_ref as mx
import sequence_ref as sq
import temporal_ref as tr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def popcount(mask):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), axis=-1).sum(axis=-1)


def neither_empty_nor_full(mask, count, H, W, w, b):
    main = max(0, H - 2 * w) * max(0, W - 2 * w)
    assert 0 < int(count.sum()) < main * min((2 * b + 1) ** 2, main), "vacuous masks"


def moment_frames(W, H, seed):
    rng = np.random.default_rng(seed)
    m = (0.5 + 0.1 * rng.standard_normal((H, W, 3))).astype(F32)
    P = np.zeros((H, W, 6), F32)
    P[..., :3] = (0.005 + 0.015 * rng.random((H, W, 3))).astype(F32)
    P[..., 3:] = (0.001 * rng.standard_normal((H, W, 3))).astype(F32)
    return m, P


@pytest.mark.parametrize("W,H,b", [(20, 14, 6), (13, 9, 6), (20, 14, 2), (13, 9, 2)])
def test_moment_cross_masks_of_the_swapped_pair_are_the_transposition(W, H, b):
    (mA, PA), (mB, PB) = moment_frames(W, H, 1), moment_frames(W, H, 2)
    eps = 1e-4
    D, valid = mx.distances(mA, PA, mB, PB, 1, b, eps)
    tau = float(np.median(D[valid & np.isfinite(D)]))
    ab, nab = mx.masks(mA, PA, mB, PB, 1, b, tau, eps)
    ba, nba = mx.masks(mB, PB, mA, PA, 1, b, tau, eps)
    neither_empty_nor_full(ab, nab, H, W, 1, b)
    t, nt = sq.transpose_masks(ab, b)
    assert np.array_equal(t, np.ascontiguousarray(ba).view(np.uint32)) and np.array_equal(nt, nba)


@pytest.mark.parametrize("eps", xc.FLOORS)
def test_moment_symmetry_with_zeros_equal_pixels_nan_and_infinite_entries(eps):
    W, H, b = 48, 12, 6
    m0, P0, mj, Pj = xc.special_pair(W, H)
    assert not np.isfinite(m0).all() and not np.isfinite(P0).all() and (P0[xc.ZERO_BLOCK] == 0).all()
    for tau in (1.0, 4.0):
        ab, nab = mx.masks(m0, P0, mj, Pj, 1, b, tau, eps)
        ba, nba = mx.masks(mj, Pj, m0, P0, 1, b, tau, eps)
        t, nt = sq.transpose_masks(ab, b)
        assert np.array_equal(t, np.ascontiguousarray(ba).view(np.uint32)) and np.array_equal(nt, nba)
    neither_empty_nor_full(ab, nab, H, W, 1, b)


@pytest.mark.parametrize("var", [True, False])
@pytest.mark.parametrize("W,H,b", [(20, 14, 6), (13, 9, 6), (20, 14, 2), (13, 9, 2)])
def test_feature_cross_masks_of_the_swapped_pair_are_the_transposition(W, H, b, var):
    c = gc.stage_images(W, H, 3, var)
    d = gx.cross_distances(c["f"], c["v"], c["f_nb"], c["v_nb"], 1, b, c["floors"])
    tau = float(np.median(d[np.isfinite(d)]))
    ab, nab = gx.cross_masks(c["f"], c["v"], c["f_nb"], c["v_nb"], 1, b, c["floors"], tau)
    ba, nba = gx.cross_masks(c["f_nb"], c["v_nb"], c["f"], c["v"], 1, b, c["floors"], tau)
    neither_empty_nor_full(ab, nab, H, W, 1, b)
    t, nt = sq.transpose_masks(ab, b)
    assert np.array_equal(t, ba) and np.array_equal(nt, nba)


def test_feature_symmetry_with_the_special_values_the_reference_defines():
    W, H, b = 20, 12, 6
    got = gc.special(W, H)
    c = got[0] if isinstance(got, tuple) else got
    assert not np.isfinite(c["f"]).all()
    ab, nab = gx.cross_masks(c["f"], c["v"], c["f_nb"], c["v_nb"], 1, b, c["floors"], c["tau"])
    ba, nba = gx.cross_masks(c["f_nb"], c["v_nb"], c["f"], c["v"], 1, b, c["floors"], c["tau"])
    t, nt = sq.transpose_masks(ab, b)
    assert np.array_equal(t, ba) and np.array_equal(nt, nba)
    assert int(nab.sum()) > 0


@pytest.mark.parametrize("W,H,b", [(20, 14, 6), (13, 9, 6), (20, 14, 2)])
def test_the_transposition_distributes_over_the_gate(W, H, b):
    rng = np.random.default_rng(W * H + b)
    words, nbits = sq.words_of(b), (2 * b + 1) ** 2
    keep = sq.pack(np.ones((H, W, nbits), bool), b)                                      # (no padding bits)
    m = rng.integers(0, 2 ** 32, (H, W, words), dtype=np.uint64).astype(np.uint32) & keep
    g = rng.integers(0, 2 ** 32, (H, W, words), dtype=np.uint64).astype(np.uint32) & keep
    gated, n = gx.gate(m, g)
    lhs, nl = sq.transpose_masks(gated, b)
    rhs, nr = gx.gate(sq.transpose_masks(m, b)[0], sq.transpose_masks(g, b)[0])
    assert np.array_equal(lhs, rhs) and np.array_equal(nl, nr)
    assert 0 < int(n.sum()) < int(popcount(m).sum())


def test_moving_edge_the_gate_removes_bits_and_the_gated_masks_transpose():
    sc = gc.benefit_scene()
    (_, nsA, hA, _), (_, nsB, hB, _) = sc["frames"][0], sc["frames"][1]
    (fA, _), (fB, _) = sc["guides"][0], sc["guides"][1]
    b = 6
    gated = {}
    for key, (h0, n0, f0, h1, n1, f1) in dict(ab=(hA, nsA, fA, hB, nsB, fB), ba=(hB, nsB, fB, hA, nsA, fA)).items():
        m, nm = tr.cross_masks(h0, n0, h1, n1, 1, b, 1.0)
        g, _ = gx.cross_masks(f0, None, f1, None, 1, b, gc.B_FLOORS, gc.B_TAU_G)
        gm, ng = gx.gate(np.ascontiguousarray(m).view(np.uint32), g)
        gated[key] = (gm, ng)
        if key == "ab":
            H, W = ng.shape
            neither_empty_nor_full(m, nm, H, W, 1, b)
            removed = (ng < nm) & (ng > 0)
            assert removed.any(), "the gate removes no bit of a cross mask that keeps one"
    t, nt = sq.transpose_masks(gated["ab"][0], b)
    assert np.array_equal(t, gated["ba"][0]) and np.array_equal(nt, gated["ba"][1])


# ---- the refusals of the layers above that need no device ------------------------------------------------------------------------------------------
def _cli(*args):
    import bcd_amd.core as core
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)


def test_bcd_cli_sequence_mode_argument_errors(tmp_path):
    """every misuse of the --sequence-layer / --sequence-moments / --sequence-features arguments is an argument error (exit code 1, "ERROR in program
    arguments") before any file is read or a device is asked for"""
    pat = lambda name: str(tmp_path / (name + ".%04d.exr"))
    seq = ["--sequence-in", pat("in"), "--sequence-out", pat("out"), "--first", "0", "--last", "3", "-p", "0"]
    cases = [
        (seq + ["--sequence-layer", pat("l"), pat("lc")], "after --sequence-layer"),
        (seq + ["--sequence-layer", pat("l"), pat("lc"), str(tmp_path / "lo.exr")], "three file patterns with one %d"),
        (seq + ["--sequence-layer", pat("l"), pat("lc"), pat("l")], "would overwrite its input"),
        (seq + ["--sequence-layer", pat("l"), pat("lc"), pat("out")], "would overwrite another file"),
        (seq + ["--sequence-layer", pat("l"), pat("lc"), pat("lo")] * 16, "at most 15"),
        (seq + ["--sequence-moments", "1e-4"], "--sequence-nsamples"),
        (seq + ["--sequence-moments", "-1", "--sequence-nsamples", pat("ns")], "variance floor"),
        (seq + ["--sequence-moments", "nan", "--sequence-nsamples", pat("ns")], "variance floor"),
        (seq + ["--sequence-moments", "inf", "--sequence-nsamples", pat("ns")], "variance floor"),
        (seq + ["--sequence-nsamples", pat("ns")], "goes with --sequence-moments"),
        (seq + ["--sequence-feature-floors", "0.1"], "go with --sequence-features"),
        (seq + ["--sequence-feature-variances", pat("v")], "go with --sequence-features"),
        (seq + ["--sequence-features", pat("f")], "--sequence-feature-floors"),
        (seq + ["--sequence-features", str(tmp_path / "f.exr"), "--sequence-feature-floors", "0.1"], "one %d"),
        (seq + ["--sequence-features", pat("f"), "--sequence-feature-floors", "0.1,-2"], "non-negative"),
        (seq + ["--sequence-features", pat("f"), "--sequence-feature-floors", "0.1,nan"], "non-negative"),
        (seq + ["--sequence-features", pat("f"), "--sequence-feature-floors", "0,0"], "no feature channel can count"),
        (seq + ["--sequence-features", pat("f"), "--sequence-feature-floors", ",".join(["0.1"] * 9)], "1 to 8"),
        (seq + ["--sequence-features", pat("f"), "--sequence-feature-floors", "0.1", "--sequence-feature-threshold", "-1"], "--sequence-feature-threshold"),
        (seq + ["--sequence-layer", pat("l"), pat("lc"), pat("lo"), "-b", "12"], "-w 1 and -b 6"),
    ]
    for args, message in cases:
        r = _cli(*args)
        assert r.returncode == 1 and "ERROR in program arguments" in r.stdout and message in r.stdout, (args, r.stdout, r.stderr)
        assert "HIP device" not in r.stdout + r.stderr
    r = _cli(*(seq + ["--sequence-layer", pat("l"), pat("lc"), pat("lo"), "--sequence-features", pat("f"), "--sequence-feature-floors", "0.1,0.1"]))
    assert r.returncode == 1 and "couldn't load input color image file" in r.stdout and "in.0000.exr" in r.stdout      # well-formed: the first file is looked for
    assert "--sequence-layer" in _cli("--help").stdout and "--sequence-moments" in _cli("--help").stdout


def test_sequence_denoiser_mode_refusals_need_no_device():
    """bcd::SequenceDenoiser with setFrameSettings(true) (through libbcdcore.so) refuses what a sequence in a mode does not serve, with a message, before a
    device is asked for: in a child process, so that the message on cerr can be read"""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import bcd_amd.core as core
W, H, D = 12, 9, 60
kw = eval(sys.argv[1])
hist = None if kw.pop("moments", False) else np.zeros((H, W, D), np.float32)
f = (np.zeros((H, W, 3), np.float32), np.ones((H, W), np.float32), hist, np.zeros((H, W, 6), np.float32))
nl = kw.pop("nl", 1)
F = kw.pop("F", 0)
var = kw.pop("var", False)
lay = [[(f[0], f[3])] * nl] * 2
if F:
    kw.update(features=[np.zeros((H, W, F), np.float32)] * 2, feature_variances=[np.zeros((H, W, F), np.float32)] * 2 if var else None)
ok, _ = core.denoise_sequence([f, f], layers=lay, **kw)
print("OK" if ok else "REFUSED")
""" % ROOT
    nan, inf = float("nan"), float("inf")
    cases = [(dict(radius=0), "temporal radius"), (dict(radius=3), "temporal radius"), (dict(nscales=0), "number of scales"), (dict(b=12), "patch radius 1 and search radius 6"),
             (dict(w=2), "patch radius 1 and search radius 6"), (dict(nscales=4), "too many scales"),
             (dict(break_settings=1), "no neighbour frames of its own"), (dict(break_settings=2), "no spike prefilter"), (dict(break_settings=4), "several devices"),
             (dict(nl=16), "added colour layers"),
             (dict(moments=True, var_floor=-1.0), "variance floor"), (dict(moments=True, var_floor=nan), "variance floor"), (dict(moments=True, var_floor=inf), "variance floor"),
             (dict(F=9, feature_floors=[0.1] * 9), "1 to 8"), (dict(F=2, feature_floors=[0.1]), "one feature floor per feature channel"),
             (dict(F=2, feature_floors=[0.1, -1.0]), "feature floor"), (dict(F=2, feature_floors=[0.1, nan]), "feature floor"),
             (dict(F=2, feature_floors=[0.0, 0.0]), "can count"), (dict(F=2, feature_floors=[0.1, 0.1], feature_threshold=-1.0), "feature threshold"),
             (dict(F=2, feature_floors=[0.1, 0.1], feature_threshold=inf), "feature threshold")]
    for kw, message in cases:
        r = subprocess.run([sys.executable, "-c", code, repr(kw).replace("nan", "float('nan')").replace("inf", "float('inf')")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "REFUSED" in r.stdout, (kw, r.stdout, r.stderr)
        assert message in r.stderr and "HIP device" not in r.stderr, (kw, r.stderr)


def test_the_new_prototypes_agree_with_the_header():
    import ctypes as C
    import bcd_amd._prototypes as bp
    from test_abi_prototypes import header_prototypes, header_structures
    want, structs = header_prototypes(), header_structures()
    new = ["bcd_hip_sequence_create_mode", "bcd_hip_sequence_push_frame", "bcd_hip_sequence_push_frame_host", "bcd_hip_sequence_pop_layers",
           "bcd_hip_sequence_pop_layers_host", "bcd_hip_sequence_mode_info"]
    for name in new:
        assert name in want and name in bp.PROTOTYPES, name
        assert bp.PROTOTYPES[name][0] is want[name][0] and list(bp.PROTOTYPES[name][1]) == want[name][1], name
    assert bp.PROTOTYPES["bcd_hip_sequence_create_mode"][1][7] is C.POINTER(bp.SequenceMode)
    for s, mirror in (("bcd_hip_sequence_mode", bp.SequenceMode), ("bcd_hip_sequence_frame", bp.SequenceFrame), ("bcd_hip_sequence_mode_info", bp.SequenceModeInfo)):
        assert [f for f, _ in mirror._fields_] == [f for f, _, _, _ in structs[s]], s
    assert "reserved" in dict(bp.SequenceMode._fields_) and "reserved" in dict(bp.SequenceFrame._fields_)
