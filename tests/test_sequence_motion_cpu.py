"""CPU tests of the motion fields of a sequence ("Sequences with motion"): the NumPy reference of the composition against the property that
defines it, the NULL rules, the keep/transpose rule, the prototypes against the header, and the refusals of the command line and of
bcd::SequenceDenoiser::setFrameMotion that need no device.

  * warp(warp(X, b), a) == warp(X, compose(a, b)) bit for bit in every image (motion_ref.warp), the validity of the right side being valid_a(p) AND
    valid_b(q(p)); the left side's own validity byte only says that q lies inside the image, and its pixel is zero wherever X warped by b was invalid.
    Random fields at 7x5 and 33x9 with vectors that leave the image at either step, and the special-value fields of sequence_motion_cases (NaN, +-inf,
    +-2^24, -0.0, the halves, sums that reach 2^24);
  * a composition with one None operand is the other operand itself, with two it is None; sequence_fields lists the neighbours' fields in ascending order;
  * a pair is transposed exactly when neither of its directions has a field, as a function of which step fields are None."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as mref
import sequence_motion_cases as mc
import sequence_motion_ref as sref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("W,H", [(7, 5), (33, 9)])
def test_two_warps_are_one_warp_by_the_composed_field(W, H):
    rng = np.random.default_rng(W)
    X = [(rng.random((H, W, 3)) + 0.5).astype(F32), (rng.random((H, W)) + 0.5).astype(F32)]          # (no zero: a zero pixel is an invalid one)
    seen = dict(broken_a=0, outside_a=0, broken_b=0, outside_b=0, valid=0, big_sum=0)
    for a, b in mc.field_pairs(W, H):
        ab = sref.compose(a, b)
        mid, valid_b = mref.warp(X, b)
        left, inside_a = mref.warp(mid, a)
        right, valid_ab = mref.warp(X, ab)
        ok_a, sl, sc = mref.sources(a, H, W)
        both = ok_a & valid_b.astype(bool)[sl, sc]
        for l, r in zip(left, right):
            assert np.array_equal(bits(l), bits(r))
        assert np.array_equal(valid_ab.astype(bool), both)
        assert np.array_equal(inside_a.astype(bool), ok_a)
        assert np.all(left[1][~both] == 0) and np.all(left[1][both] > 0)
        # the composed field itself: integers, never -0.0, NaN in both components or in neither
        nan = np.isnan(ab)
        assert np.array_equal(nan[..., 0], nan[..., 1])
        assert np.array_equal(ab[~nan], np.rint(ab[~nan])) and not np.any(np.signbit(ab[~nan]) & (ab[~nan] == 0))
        assert not np.any(nan[..., 0] & both)                                  # (a broken pixel is never a valid one)
        with np.errstate(invalid="ignore"):
            fin_a = np.isfinite(a).all(-1) & (np.abs(a) < mc.BIG).all(-1)
            b_q = b[sl, sc]
            fin_b = np.isfinite(b_q).all(-1) & (np.abs(b_q) < mc.BIG).all(-1)
        seen["broken_a"] += int((~fin_a).sum()); seen["outside_a"] += int((fin_a & ~ok_a).sum())
        seen["broken_b"] += int((ok_a & ~fin_b).sum()); seen["outside_b"] += int((ok_a & fin_b & ~both).sum())
        seen["valid"] += int(both.sum()); seen["big_sum"] += int((ok_a & fin_b & nan[..., 0]).sum())
    assert all(v > 0 for k, v in seen.items() if k != "big_sum"), seen
    if W == 33:
        assert seen["big_sum"] > 0, seen


def test_rounding_and_limits_of_the_composition():
    f = lambda *v: np.array(v, F32).reshape(1, -1, 2)
    z = np.zeros((1, 4, 2), F32)
    # halves round to even, -0.0 and -0.5 give +0.0
    got = sref.compose(f(0.5, -0.5, 1.5, -0.0, 2.5, 0, -1.5, 0), z)
    want = f(0, 0, 2, 0, np.nan, np.nan, -2, 0)            # (pixel 2 + 2 leaves the 4-pixel line)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(want)))
    # the limit is 2^24 itself, for either step and for the sum
    big, below = F32(2.0 ** 24), np.nextafter(F32(2.0 ** 24), F32(0))
    assert np.isnan(sref.compose(f(big, 0, -big, 0, 0, big, 0, np.inf), z)).all()
    got = sref.compose(z, f(big, 0, below, 0, 0, -below, np.nan, 0))
    assert np.isnan(got[0, 0]).all() and np.array_equal(got[0, 1], [below, 0]) and np.array_equal(got[0, 2], [0, -below]) and np.isnan(got[0, 3]).all()
    got = sref.compose(f(1, 0, 0, 0, 0, 0, -1, 0), f(0, 0, below, 0, -below, 0, 0, 0))       # (pixels 0 and 1 read b(1), pixels 2 and 3 read b(2))
    assert np.isnan(got[0, 0]).all() and np.array_equal(got[0, 1], [below, 0]) and np.array_equal(got[0, 2], [-below, 0]) and np.isnan(got[0, 3]).all()


def test_null_rules_and_the_fields_of_a_pop():
    W, H, T = 7, 5, 5
    a, b = mc.field_pairs(W, H)[1]
    assert sref.compose_fields(None, None) is None
    assert sref.compose_fields(a, None) is a and sref.compose_fields(None, b) is b
    assert np.array_equal(bits(np.nan_to_num(sref.compose_fields(a, b))), bits(np.nan_to_num(sref.compose(a, b))))
    st = mc.step_fields("moving", W, H, T)
    assert st[1][1] is None and st[3][0] is None and all(x is not None for k, e in enumerate(st) for j, x in enumerate(e) if (k, j) not in ((1, 1), (3, 0)))
    same = lambda x, y: (x is None and y is None) or (x is not None and y is not None and np.array_equal(bits(np.nan_to_num(x)), bits(np.nan_to_num(y))))
    # R = 1: the step fields themselves; the ends of the sequence have one neighbour
    assert [x is None for x in sref.sequence_fields(st, 1, 1, T)] == [False, True]
    assert sref.sequence_fields(st, 0, 1, T)[0] is st[0][1] and sref.sequence_fields(st, 4, 1, T)[0] is st[4][0]
    # R = 2, frame 2: t - 2 = compose(prev[2], prev[1]), t - 1 = prev[2], t + 1 = next[2], t + 2 = compose(next[2], next[3])
    got = sref.sequence_fields(st, 2, 2, T)
    want = [sref.compose(st[2][0], st[1][0]), st[2][0], st[2][1], sref.compose(st[2][1], st[3][1])]
    assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want))
    # one None step yields the other as it is: 3 -> 1 is prev[2] (prev[3] is None), 0 -> 2 is next[0] (next[1] is None)
    assert sref.sequence_fields(st, 3, 2, T)[0] is st[2][0] and sref.sequence_fields(st, 0, 2, T)[1] is st[0][1]
    assert sref.sequence_fields(mc.step_fields("null", W, H, T), 2, 2, T) == [None] * 4
    # distance-2 vectors of the moving sequence exceed the search radius
    far = sref.sequence_fields(st, 2, 2, T)[3]
    assert np.nanmax(np.abs(far)) > 6


def test_a_pair_is_transposed_exactly_when_neither_direction_has_a_field():
    W, H, T = 4, 3, 5
    z = np.zeros((H, W, 2), F32)
    for R, pairs in ((1, 4), (2, 7)):
        assert sref.counters(mc.step_fields("null", W, H, T), R, T) == dict(cross_computed=pairs, cross_transposed=pairs, neighbours_warped=0, fields_composed=0)
        visits = 2 * pairs
        c = sref.counters(mc.step_fields("zero", W, H, T), R, T)
        assert c == dict(cross_computed=visits, cross_transposed=0, neighbours_warped=visits, fields_composed=0 if R == 1 else 6)
    # every subset of the two step fields between frames 0 and 1
    for prev1 in (None, z):
        for next0 in (None, z):
            st = [(None, next0), (prev1, None)]
            assert sref.pair_is_transposed(st, 0, 1) == sref.pair_is_transposed(st, 1, 0) == (prev1 is None and next0 is None)
    # two frames apart: any of the four steps between them breaks the pair
    for k in range(16):
        n0, n1, p2, p1 = (z if k >> i & 1 else None for i in range(4))
        st = [(None, n0), (p1, n1), (p2, None)]
        assert sref.pair_is_transposed(st, 0, 2) == (k == 0)
    # only frame 2 moves: its pairs with 1 and 3 are computed from both sides, and at R = 2 every pair whose path crosses a field of frame 2
    st = mc.step_fields("partly", W, H, T)
    tr = lambda R: sorted((f, t) for t in range(T) for f in sref.neighbours(t, R, T) if f < t and sref.pair_is_transposed(st, t, f))
    assert tr(1) == [(0, 1), (3, 4)]
    assert tr(2) == [(0, 1), (3, 4)]            # (0,2), (1,2), (2,3), (2,4) touch frame 2; (1,3) passes through it from either side
    c = sref.counters(st, 2, T)
    assert c["cross_transposed"] == 2 and c["cross_computed"] == 12 and c["neighbours_warped"] == 6 and c["fields_composed"] == 0


def test_the_prototypes_name_the_new_entry_points():
    import bcd_amd._prototypes as pr
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    for name, nargs in (("bcd_hip_compose_motion", 6), ("bcd_hip_sequence_push_frame_motion", 4), ("bcd_hip_sequence_push_frame_motion_host", 4),
                        ("bcd_hip_sequence_motion_info", 3)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, txt)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == nargs == len(pr.PROTOTYPES[name][1])
    assert "motion fields (a warped neighbour breaks the symmetry)" not in txt


# ---- the layers above the C ABI: what they refuse, they refuse before a device is asked for (no device is visible to the child) --------------------------
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _cli(*args):
    import bcd_amd.core as core
    exe = os.path.join(os.path.dirname(core.LIB_PATH), "bcd_cli")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=NO_DEVICE)


def test_bcd_cli_sequence_motion_argument_errors(tmp_path):
    seq = ["--sequence-in", str(tmp_path / "in.%04d.exr"), "--sequence-out", str(tmp_path / "out.%04d.exr"), "--first", "0", "--last", "3", "-p", "0"]
    prev, nxt, some = str(tmp_path / "prev.%04d.exr"), str(tmp_path / "next.%04d.exr"), str(tmp_path / "x.exr")
    cases = [
        (["-i", some, "-o", some, "--sequence-motion-prev", prev], "go with --sequence-in"),
        (["--sequence-motion-next", nxt], "go with --sequence-in"),
        (seq + ["--sequence-motion-prev", some], "need a file pattern with one %d"),
        (seq + ["--sequence-motion-next", str(tmp_path / "n.%d.%d.exr")], "need a file pattern with one %d"),
        (seq + ["--sequence-motion-prev"], "expecting a value after --sequence-motion-prev"),
        (seq + ["--sequence-motion-prev", prev, "--neighbour-motion", some], "--neighbour-motion is not available with --sequence-in"),      # (stays refused as it is)
    ]
    for args, message in cases:
        r = _cli(*args)
        assert r.returncode == 1 and "ERROR in program arguments" in r.stdout and message in r.stdout, (args, r.stdout, r.stderr)
        assert "HIP device" not in r.stdout + r.stderr
    r = _cli(*(seq + ["--sequence-motion-prev", prev, "--sequence-motion-next", nxt]))            # well-formed: the first frame's file is looked for
    assert r.returncode == 1 and "couldn't load input color image file" in r.stdout and "in.0000.exr" in r.stdout
    assert "--sequence-motion-prev <pattern>" in _cli("--help").stdout


def test_set_frame_motion_refusals_need_no_device():
    """bcd::SequenceDenoiser::setFrameMotion (through libbcdcore.so, in a child process whose cerr can be read): a field with another channel count or size
    makes pushFrame() return false with a message before a device is asked for; a well-formed one gets as far as asking for the device"""
    import sys
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import bcd_amd.core as core
W, H, D = 12, 9, 60
f = (np.zeros((H, W, 3), np.float32), np.ones((H, W), np.float32), np.zeros((H, W, D), np.float32), np.zeros((H, W, 6), np.float32))
z = np.zeros((H, W, 2), np.float32)
kw = eval(sys.argv[1])
ok, _ = core.denoise_sequence([f, f], motions=[(None, z), (z, None)], **kw)
print("OK" if ok else "REFUSED")
""" % ROOT
    for kw, message in ((dict(break_motion=1), "needs 2 channels and the frame's size (12x9), not 12x9x3"), (dict(break_motion=2), "needs 2 channels and the frame's size (12x9), not 11x9x2"),
                        (dict(layers=[[], []], break_motion=3), "not 11x9x3")):
        r = subprocess.run([sys.executable, "-c", code, repr(kw)], capture_output=True, text=True, timeout=120, env=NO_DEVICE)
        assert r.returncode == 0 and "REFUSED" in r.stdout, (kw, r.stdout, r.stderr)
        assert message in r.stderr and "towards the next frame" in r.stderr and "HIP device" not in r.stderr, (kw, r.stderr)
    r = subprocess.run([sys.executable, "-c", code, "{}"], capture_output=True, text=True, timeout=120, env=NO_DEVICE)
    assert r.returncode == 0 and "REFUSED" in r.stdout and "no usable HIP device" in r.stderr, (r.stdout, r.stderr)
    import bcd_amd.core as core
    with pytest.raises(ValueError):
        z = np.zeros((4, 4, 2), F32)
        core.denoise_sequence([(np.zeros((4, 4, 3), F32), np.ones((4, 4), F32), np.zeros((4, 4, 8), F32), np.zeros((4, 4, 6), F32))] * 2, motions=[(z, z)])
