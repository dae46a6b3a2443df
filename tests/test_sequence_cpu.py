"""CPU tests of the mask transposition a sequence rests on (tests/sequence_ref.py against tests/temporal_ref.py; DESIGN 16, "Sequences").  No GPU needed.

  * the symmetry itself: transpose_masks(cross_masks(A, B)) equals cross_masks(B, A), masks and counts, on oracle_lib.synth_inputs frames of two seeds at
    40x28, tau = 1.0, with a member count above 0 and below the candidate count;
  * the transposition applied twice is the identity on those masks;
  * the definition's edge rules on random masks: bits towards pixels outside the image and padding bits come out zero, counts are popcounts;
  * the bcd_cli --sequence-in argument errors and the bcd::SequenceDenoiser refusals, none of which asks for a device."""
import os
import subprocess
import sys

import numpy as np

import oracle_lib as ol
import sequence_ref as sq
import temporal_ref as tr

W, H, w, b, TAU = 40, 28, 1, 6, 1.0

_cache = {}


def pair_masks():
    if not _cache:
        (_, ns_a, hist_a, _, _), (_, ns_b, hist_b, _, _) = (ol.synth_inputs(W, H, 32, seed) for seed in (1234, 77))
        _cache["ab"] = tr.cross_masks(hist_a, ns_a, hist_b, ns_b, w, b, TAU)
        _cache["ba"] = tr.cross_masks(hist_b, ns_b, hist_a, ns_a, w, b, TAU)
    return _cache["ab"], _cache["ba"]


def test_transposed_cross_masks_are_the_cross_masks_of_the_swapped_pair():
    (ab_m, ab_c), (ba_m, ba_c) = pair_masks()
    members, candidates = int(ab_c.sum()), (W - 2 * w) * (H - 2 * w) * (2 * b + 1) ** 2
    assert 0 < members < candidates, (members, candidates)
    tm, tc = sq.transpose_masks(ab_m, b)
    assert np.array_equal(tm, np.ascontiguousarray(ba_m).view(np.uint32)) and np.array_equal(tc, ba_c)
    assert int(ba_c.sum()) == members


def test_transposition_twice_is_the_identity():
    (ab_m, ab_c), _ = pair_masks()
    m1, _ = sq.transpose_masks(ab_m, b)
    m2, c2 = sq.transpose_masks(m1, b)
    assert np.array_equal(m2, np.ascontiguousarray(ab_m).view(np.uint32)) and np.array_equal(c2, ab_c)


def test_edge_rules_of_the_definition():
    rng = np.random.default_rng(3)
    for (ww, hh, bb) in ((5, 4, 6), (9, 3, 2), (1, 1, 6)):
        words = sq.words_of(bb)
        raw = rng.integers(0, 2 ** 32, (hh, ww, words), dtype=np.uint64).astype(np.uint32)      # bits outside the image and padding bits set too
        m, c = sq.transpose_masks(raw, bb)
        bits = sq.unpack(m, bb)
        assert not (bits & ~sq.in_image_bits(hh, ww, bb)).any()
        assert np.array_equal(sq.pack(bits, bb), m)                                               # (padding bits zero)
        assert np.array_equal(c, bits.sum(axis=2))


# ---- the refusals of the layers above that need no device ------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args):
    import bcd_amd.core as core
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)


def test_bcd_cli_sequence_argument_errors(tmp_path):
    """every misuse of --sequence-in is an argument error (exit code 1, "ERROR in program arguments") before any file is read or a device is asked for"""
    seq = ["--sequence-in", str(tmp_path / "in.%04d.exr"), "--sequence-out", str(tmp_path / "out.%04d.exr"), "--first", "0", "--last", "3", "-p", "0"]
    some = str(tmp_path / "x.exr")
    cases = [
        (seq + ["-i", some], "-i is not available with --sequence-in"),
        (seq + ["-o", some], "-o is not available with --sequence-in"),
        (seq + ["--neighbour", some], "--neighbour is not available with --sequence-in"),
        (seq + ["--layer", some, some, some], "--layer is not available with --sequence-in"),
        (seq + ["--features", some], "--features is not available with --sequence-in"),
        (seq + ["--moment-selection"], "--moment-selection is not available with --sequence-in"),
        (seq + ["--devices", "0-1"], "--devices is not available with --sequence-in"),
        (seq[:2] + seq[4:], "--sequence-out <pattern with %d> is required"),
        (seq[2:], "--sequence-in needs a file pattern with one %d"),
        (["--sequence-in", str(tmp_path / "in.exr")] + seq[2:], "--sequence-in needs a file pattern with one %d"),
        (["--sequence-in", str(tmp_path / "in.%s.exr")] + seq[2:], "--sequence-in needs a file pattern with one %d"),
        (["--sequence-in", str(tmp_path / "in.%d.%d.exr")] + seq[2:], "--sequence-in needs a file pattern with one %d"),
        (seq[:2] + ["--sequence-out", seq[1]] + seq[4:], "would overwrite"),
        (seq[:4] + ["--last", "3", "-p", "0"], "--first <a> and --last <b>"),
        (seq[:4] + ["--first", "4", "--last", "3", "-p", "0"], "--first <a> and --last <b>"),
        (seq + ["--temporal-radius", "0"], "--temporal-radius must be 1 or 2"),
        (seq + ["--temporal-radius", "3"], "--temporal-radius must be 1 or 2"),
        (seq[:-2], "add -p 0"),                                                                   # the CLI's default is -p 1
        (seq + ["-b", "12"], "-w 1 and -b 6"),
        (seq + ["-w", "2"], "-w 1 and -b 6"),
        (seq + ["--bogus", "1"], "unknown argument --bogus"),
        (seq + ["--first"], "expecting a value after --first"),
    ]
    for args, message in cases:
        r = _cli(*args)
        assert r.returncode == 1 and "ERROR in program arguments" in r.stdout and message in r.stdout, (args, r.stdout, r.stderr)
        assert "HIP device" not in r.stdout + r.stderr
    r = _cli(*seq)                                                                                # well-formed: the first frame's file is looked for
    assert r.returncode == 1 and "couldn't load input color image file" in r.stdout and "in.0000.exr" in r.stdout
    assert "--sequence-in <pattern>" in _cli("--help").stdout


def test_sequence_denoiser_refusals_need_no_device():
    """bcd::SequenceDenoiser (through libbcdcore.so) refuses what a sequence does not serve with its own message, before a device is asked for: in a child
    process, so that the message on cerr can be read"""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import bcd_amd.core as core
W, H, D = 12, 9, 60
f = (np.zeros((H, W, 3), np.float32), np.ones((H, W), np.float32), np.zeros((H, W, D), np.float32), np.zeros((H, W, 6), np.float32))
kw = eval(sys.argv[1])
ok, _ = core.denoise_sequence([f, f], **kw)
print("OK" if ok else "REFUSED")
""" % ROOT
    cases = [(dict(radius=0), "temporal radius"), (dict(radius=3), "temporal radius"), (dict(nscales=0), "number of scales"), (dict(b=12), "patch radius 1 and search radius 6"),
             (dict(w=2), "patch radius 1 and search radius 6"), (dict(unsupported=1), "no added colour layers"), (dict(unsupported=2), "no neighbour frames of its own"),
             (dict(unsupported=4), "no moment selection"), (dict(unsupported=8), "no spike prefilter"), (dict(unsupported=16), "several devices"),
             (dict(nscales=4), "too many scales")]
    for kw, message in cases:
        r = subprocess.run([sys.executable, "-c", code, repr(kw)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "REFUSED" in r.stdout, (kw, r.stdout, r.stderr)
        assert message in r.stderr and "HIP device" not in r.stderr, (kw, r.stderr)
