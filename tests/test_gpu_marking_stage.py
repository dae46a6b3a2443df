"""GPU tests of the marking kernels (bcd_amd/csrc/k_active.hip) on constructed similarity graphs.

bcd_hip_active_set / _init / _step take the masks, |S| and the state image as plain tensors: every case of tests/marking_cases.py is handed to them
directly and the state image is compared with tests/marking_ref.py -- the reference's sequential marking pass, pixel after pixel -- under the
scanline order (every hash ties: the k < centre tie-break), the seeded random order (two seeds) and the strip order, and under skip probabilities
0, 0.25, 0.5 and 1.  The result is integers: every comparison is array_equal, there is no tolerance in this file.

  * whole problem: the state image, nothing left undecided, rounds == 0 for m = 0, 1 <= rounds <= main pixels otherwise (the count itself is
    not asserted: within a launch a tile may or may not see its neighbour's fresh decisions; it is written through BCD_TEST_REPORT);
  * one offset at a time: every pair (k, mirrored k) of the window on its own -- every bit position of window_bits, earlier_bit, the per-line
    slicing of k_mark_round and the generic kernel's k / side, bits 31 / 32 of every word and the last bit of the last word included;
  * step by step: the count a step returns is the number of undecided bytes of the state (the counter-line fold), a decision is final the moment
    it is made, and the count strictly decreases;
  * row bands with a row offset, halo lines decided or still undecided;
  * sequences of problems on one context: radii 6, 3, 12, 6, refilled buffers (the dependency cache is keyed by pointers), deep then shallow;
  * refusals of the entry points;
  * the list compaction k_active_lists through bcd_hip_selftest_active_lists, around the 8 x 1024 pixels of a workgroup.

Which kernel a case reaches (active_step_enqueue in bcd_api.hip): b = 6, 12 -> k_mark_deps<b> once, then k_mark_round<b>; any other radius (here
1, 3, 8) -> k_active_round.

Measured on the MI355X: the file runs in 6 s (36 tests with tests/test_abi.py).  Launches per whole problem (BCD_TEST_REPORT): the 298-deep
chain of the 300x18 frame takes 39 launches under the scanline and strip orders and 3 under the random order at b = 6 (in-tile chains resolve
inside a launch), the 128-deep chain of 130x20 at b = 3 takes 128 and 6 - 7 (one level per launch), the vertical chain at b = 12 takes 18, 7 and 3.
Twelve mutated builds of k_active.hip and what each turned red: docs/EXPERIMENTS.md section 14."""
import ctypes as C
import os

import numpy as np
import pytest

import marking_cases as mc
import marking_ref as mr

pytestmark = pytest.mark.gpu


def _report(line):
    if os.environ.get("BCD_TEST_REPORT"):
        with open(os.environ["BCD_TEST_REPORT"], "a") as f:
            f.write("%s %s\n" % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], line))


def t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


_dev = {}


def dev(case):
    if case.name not in _dev:
        _dev[case.name] = (t(case.mask), t(case.cnt))
    return _dev[case.name]


def main_pixels(case):
    return (case.W - 2 * case.w) * (case.H - 2 * case.w)


def run_whole(hipctx, case, mode, seed, m, tensors=None):
    mask, cnt = tensors or dev(case)
    hipctx.synchronize()
    state, rounds = hipctx.active_set(mask, cnt, case.w, case.b, m, mode, seed)
    hipctx.synchronize()
    return state.cpu().numpy(), rounds


def check_whole(hipctx, case, mode, seed, m, tensors=None):
    st, rounds = run_whole(hipctx, case, mode, seed, m, tensors)
    what = (case.name, "order %d seed %d m %g" % (mode, seed, m))
    want = mc.reference(case, mode, seed, m)
    assert not (st == mr.ST_UNDECIDED).any(), what
    assert np.array_equal(st, want), what + ("%d pixels differ, first at %s" % ((st != want).sum(), np.argwhere(st != want)[:4].tolist()),)
    if m <= 0:
        assert rounds == 0 and np.array_equal(st == mr.ST_IN, mr.main_area(case.W, case.H, case.w)), what
    else:
        assert 1 <= rounds <= main_pixels(case), what + (rounds,)
    return rounds


@pytest.mark.parametrize("family", ["random", "full", "threshold", "chain", "isolated"])
def test_whole_problem_equals_the_sequential_reference(hipctx, family):
    sel = [c for c in mc.cases() if c.family == family]
    assert sel
    for case in sel:
        for (mode, seed) in mc.orders(case):
            for m in case.ms:
                rounds = check_whole(hipctx, case, mode, seed, m)
                if case.depth is not None and m == 1.0:
                    _report("%s order %d seed %d: depth %d (scanline), %d launches" % (case.name, mode, seed, case.depth, rounds))


@pytest.mark.parametrize("b", [3, 8, 6, 12])
def test_every_window_offset_on_its_own(hipctx, b):
    W, H, w = mc.ONE_OFFSET_FRAMES[b]
    seen = 0
    # (the listed kernels compare hashes cell by cell only under the random order, where a wrong cell shows by chance per pair: two seeds there)
    orders = ((0, 0), (1, 11), (1, 4242)) if b in (6, 12) else ((0, 0), (1, 11))
    for k in range(mc.pair_count(b)):
        case = mc.one_offset(W, H, w, b, k)
        tensors = (t(case.mask), t(case.cnt))
        for (mode, seed) in orders:
            st, rounds = run_whole(hipctx, case, mode, seed, 1.0, tensors)
            want = mr.greedy(case.mask, case.cnt, w, b, mc.visit(case, mode, seed), mr.skip_draw(W, H, 1.0, seed))
            assert np.array_equal(st, want), (case.name, mode, mc.offset(k, b), np.argwhere(st != want)[:4].tolist())
            assert 1 <= rounds <= main_pixels(case)
            seen += int((want == mr.ST_OUT).any())
    assert seen == len(orders) * mc.pair_count(b)                              # every pair marked somebody: no offset was checked on an empty graph


# ---- step by step ---------------------------------------------------------------------------------------------------------------------------
def step_until_done(hipctx, mask, cnt, state, w, b, rb, re, mode, key_seed, row_offset, want_owned, what, first=True):
    """active_step until it returns 0; after every step: the count is the number of undecided bytes of the owned lines, every decided owned pixel
    holds its final value, and the count has gone down.  -> (state as numpy, number of steps)"""
    before, steps = None, 0
    limit = int(np.count_nonzero(want_owned != mr.ST_NONE)) + 2
    while True:
        left = hipctx.active_step(mask, cnt, state, w, b, rb, re, mode, key_seed, row_offset, first and steps == 0)
        hipctx.synchronize()
        st = state.cpu().numpy()
        steps += 1
        own = st[rb:re]
        assert left == int((own == mr.ST_UNDECIDED).sum()), what + ("step %d" % steps,)
        decided = own != mr.ST_UNDECIDED
        assert np.array_equal(own[decided], want_owned[decided]), what + ("a decision of step %d is not final" % steps,)
        assert before is None or left < before, what + ("the count went from %d to %d" % (before or 0, left),)
        if left == 0:
            return st, steps
        assert steps < limit, what
        before = left


STEP_CASES = ["chain horizontal b=6 300x18 w=1", "chain horizontal b=3 130x20 w=1", "chain vertical b=12 18x130 w=1", "chain serpentine b=6 40x24 w=1",
              "random 0.30 b=6 33x18 w=1 (bands)", "full b=8 15x40 w=1", "full b=12 41x30 w=1", "threshold random seeded b=3 16x33 w=1"]


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_by_step_counts_and_final_decisions(hipctx, name):
    import bcd_amd.hip as bh
    case = mc.by_name(name)
    mask, cnt = dev(case)
    for (mode, seed) in mc.orders(case):
        for m in (1.0, 0.5):
            want = mc.reference(case, mode, seed, m)
            key_seed = bh.strip_order_seed(case.W, case.H, case.w, case.b) if mode == 2 else seed
            hipctx.synchronize()
            state = hipctx.active_init(cnt, case.w, 0, case.H, m, seed, 0)
            hipctx.synchronize()
            st0 = state.cpu().numpy()
            assert np.array_equal(st0 == mr.ST_UNDECIDED, mr.skip_draw(case.W, case.H, m, seed) & mr.main_area(case.W, case.H, case.w))
            st, steps = step_until_done(hipctx, mask, cnt, state, case.w, case.b, 0, case.H, mode, key_seed, 0, want, (name, mode, seed, m))
            assert np.array_equal(st, want)
            _report("%s order %d seed %d m %g: %d steps" % (name, mode, seed, m, steps))


# ---- row bands ------------------------------------------------------------------------------------------------------------------------------
def bands_of(H):
    """owned line ranges [r0, r1): the frame's first band, one that begins at a tile boundary, one a line off it, the frame's last band"""
    out = [(0, min(H, 9)), (16, min(H, 23)), (17, min(H, 33)), (max(0, H - 6), H)]
    return [(r0, r1) for (r0, r1) in out if r0 < r1]


def waits_for_the_halo(case, want, order, top, r0, r1, bot):
    """is there an owned pixel that is processed in the end and has an earlier strong similar neighbour in a halo line?  With the halo undecided
    it cannot be decided: nothing says yet that this neighbour will not mark it."""
    W = case.W
    rank = np.full(W * case.H, -1, np.int64)
    rank[order] = np.arange(order.size)
    ptr, idx = mr.members(case.mask, case.b)
    strong = case.cnt.reshape(-1) >= mr.strong_threshold(case.w)
    for p in np.flatnonzero(want.reshape(-1) == mr.ST_IN):
        if not r0 <= p // W < r1:
            continue
        q = idx[ptr[p]:ptr[p + 1]]
        ql = q // W
        if (strong[q] & (rank[q] < rank[p]) & (q != p) & (((ql >= top) & (ql < r0)) | ((ql >= r1) & (ql < bot)))).any():
            return True
    return False


def band_cases():
    out = [mc.by_name(n) for n in ("chain vertical b=6 18x130 w=1", "chain vertical b=12 18x130 w=1", "chain serpentine b=6 40x24 w=1",
                                   "chain horizontal b=3 130x20 w=1", "random 0.30 b=6 33x18 w=1 (bands)", "random 0.30 b=6 15x40 w=1",
                                   "random 0.30 b=3 16x33 w=1", "random 0.90 b=12 30x41 w=1", "random 0.30 b=8 15x40 w=1")]
    for (W, H, w, b, ks) in [(17, 40, 1, 6, (0, 6, 31, 32, 78, 83)), (17, 40, 1, 3, (0, 3, 21, 23)), (30, 41, 1, 12, (12, 31, 32, 300, 311))]:
        out += [mc.one_offset(W, H, w, b, k) for k in ks]
    return out


@pytest.mark.parametrize("halo_undecided", [False, True], ids=["halo decided", "halo undecided first"])
def test_row_bands_with_a_row_offset(hipctx, halo_undecided):
    import torch
    cases = band_cases()
    assert len(cases) >= 20 and {c.family for c in cases} == {"chain", "random", "one offset"}
    waited = 0
    for case in cases:
        W, H, w, b = case.W, case.H, case.w, case.b
        assert b >= w                                                # (the band's own border lines are then halo lines or true border lines)
        for (mode, seed) in ((0, 0), (1, 11)):
            for m in ((1.0,) if halo_undecided else (1.0, 0.5)):
                want = mc.reference(case, mode, seed, m) if case.family != "one offset" else \
                    mr.greedy(case.mask, case.cnt, w, b, mc.visit(case, mode, seed), mr.skip_draw(W, H, m, seed))
                for (r0, r1) in bands_of(H):
                    top, bot = max(0, r0 - b), min(H, r1 + b)
                    rb, re = r0 - top, r1 - top
                    what = (case.name, "order %d seed %d m %g" % (mode, seed, m), "lines [%d, %d) of band [%d, %d)" % (r0, r1, top, bot))
                    mask, cnt = t(case.mask[top:bot]), t(case.cnt[top:bot])
                    halo = want[top:bot].copy()
                    halo[rb:re] = mr.ST_NONE
                    hipctx.synchronize()
                    state = hipctx.active_init(cnt, w, rb, re, m, seed, top)
                    hipctx.synchronize()

                    def put_halo(h):
                        hd = torch.from_numpy(h).cuda()
                        state[:rb] = hd[:rb]
                        state[re:] = hd[re:]
                        hipctx.synchronize()
                    first = True
                    if halo_undecided:
                        put_halo(np.where(halo == mr.ST_NONE, mr.ST_NONE, mr.ST_UNDECIDED).astype(np.uint8))
                        left = hipctx.active_step(mask, cnt, state, w, b, rb, re, mode, seed, top, True)
                        hipctx.synchronize()
                        own = state.cpu().numpy()[rb:re]
                        assert left == int((own == mr.ST_UNDECIDED).sum()), what
                        decided = own != mr.ST_UNDECIDED
                        assert np.array_equal(own[decided], want[r0:r1][decided]), what + ("decided against an undecided halo",)
                        if waits_for_the_halo(case, want, mc.visit(case, mode, seed), top, r0, r1, bot):
                            assert left > 0, what
                            waited += 1
                        first = False
                        if left == 0:
                            continue
                    put_halo(halo)
                    st, _ = step_until_done(hipctx, mask, cnt, state, w, b, rb, re, mode, seed, top, want[r0:r1], what, first)
                    assert np.array_equal(st[rb:re], want[r0:r1]), what
                    assert np.array_equal(st[:rb], halo[:rb]) and np.array_equal(st[re:], halo[re:]), what + ("halo lines were written",)
    assert not halo_undecided or waited >= 20


# ---- sequences of problems on one context -----------------------------------------------------------------------------------------------------
def test_radii_back_to_back_on_one_context(hipctx):
    for name in ("random 0.30 b=6 33x18 w=1 (bands)", "random 0.30 b=3 16x33 w=1", "random 0.30 b=12 41x30 w=1", "full b=6 33x18 w=1",
                 "full b=3 16x33 w=1", "random 0.30 b=6 15x40 w=1"):
        case = mc.by_name(name)
        for (mode, seed) in ((1, 11), (0, 0)):
            check_whole(hipctx, case, mode, seed, 1.0)


def test_refilled_buffers_between_two_problems(hipctx):
    """same device pointers, other contents: the dependency lists of the first problem must not serve the second"""
    a, b_, c = mc.by_name("random 0.30 b=6 33x18 w=1 (bands)"), mc.by_name("threshold full checker b=6 33x18 w=1"), mc.by_name("isolated strong b=6 33x18 w=1")
    mask, cnt = t(a.mask), t(a.cnt)
    state = None
    for case in (a, b_, c, a):
        mask.copy_(t(case.mask))
        cnt.copy_(t(case.cnt))
        for (mode, seed) in ((0, 0), (1, 4242)):
            want = mc.reference(case, mode, seed, 1.0)
            hipctx.synchronize()
            state = hipctx.active_init(cnt, case.w, 0, case.H, 1.0, seed, 0, state)
            # (no synchronisation between init and the first step here: the two entry points launch on one stream and are ordered by it)
            st, _ = step_until_done(hipctx, mask, cnt, state, case.w, case.b, 0, case.H, mode, seed, 0, want, (case.name, mode, seed))
            assert np.array_equal(st, want), (case.name, mode)
            check_whole(hipctx, case, mode, seed, 1.0, (mask, cnt))


def test_deep_then_shallow_and_back(hipctx):
    """the first batch of a problem is sized by what the previous one needed (random order)"""
    deep, shallow = mc.by_name("chain horizontal b=6 300x18 w=1"), mc.by_name("random 0.02 b=6 16x16 w=1")
    for case in (deep, shallow, shallow, deep, shallow, deep):
        for mode in (1, 0):
            check_whole(hipctx, case, mode, 11, 1.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_any_device_work(hipctx):
    import torch
    import bcd_amd.hip as bh
    case = mc.by_name("random 0.30 b=6 33x18 w=1 (bands)")
    mask, cnt = dev(case)
    W, H, w, b = case.W, case.H, case.w, case.b
    state = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
    hipctx.synchronize()
    L, dp = bh.lib(), bh._dp
    rounds, left = C.c_int32(-5), C.c_int32(-5)

    def whole(mask_p, cnt_p, state_p, W_, H_, w_, b_):
        return L.bcd_hip_active_set(hipctx.h, mask_p, cnt_p, W_, H_, w_, b_, 0, max(H_, 0), C.c_float(1.0), 0, C.c_uint32(0), state_p, C.byref(rounds))

    def step(mask_p, cnt_p, state_p, W_, H_, w_, b_, out=C.byref(left)):
        return L.bcd_hip_active_step(hipctx.h, mask_p, cnt_p, W_, H_, w_, b_, 0, max(H_, 0), 0, C.c_uint32(0), 0, 1, state_p, out)

    bad = [(None, dp(cnt), dp(state), W, H, w, b), (dp(mask), None, dp(state), W, H, w, b), (dp(mask), dp(cnt), None, W, H, w, b),
           (dp(mask), dp(cnt), dp(state), 0, H, w, b), (dp(mask), dp(cnt), dp(state), W, 0, w, b), (dp(mask), dp(cnt), dp(state), W, -3, w, b),
           (dp(mask), dp(cnt), dp(state), W, H, -1, b), (dp(mask), dp(cnt), dp(state), W, H, w, -1)]
    for i, args in enumerate(bad):
        for fn in (whole, step):
            assert fn(*args) != 0
            msg = L.bcd_hip_last_error(hipctx.h).decode()
            assert ("bad argument" if i < 3 else "marking: empty image or negative radius") in msg, msg   # null pointers | geometry
    assert step(dp(mask), dp(cnt), dp(state), W, H, w, b, None) != 0 and "bad argument" in L.bcd_hip_last_error(hipctx.h).decode()
    for (W_, H_, w_) in ((0, H, w), (W, 0, w), (W, H, -1)):          # the same words from the first half of the pair
        assert L.bcd_hip_active_init(hipctx.h, dp(cnt), W_, H_, w_, 0, max(H_, 0), C.c_float(1.0), C.c_uint32(0), 0, dp(state)) != 0
        assert "marking: empty image or negative radius" in L.bcd_hip_last_error(hipctx.h).decode()
    assert L.bcd_hip_active_init(hipctx.h, None, W, H, w, 0, H, C.c_float(1.0), C.c_uint32(0), 0, dp(state)) != 0
    assert "bad argument" in L.bcd_hip_last_error(hipctx.h).decode()
    hipctx.synchronize()
    assert (state == 7).all() and rounds.value == -5 and left.value == -5
    # ... and the context still works
    check_whole(hipctx, case, 0, 0, 1.0)
    with pytest.raises(bh.BcdHipError, match="row range|bad argument"):
        hipctx.selftest_active_lists(state, cnt, w, 3, H + 1)
    with pytest.raises(bh.BcdHipError, match="row range|bad argument"):
        hipctx.selftest_active_lists(state, cnt, w, 5, 4)


# ---- the list compaction ----------------------------------------------------------------------------------------------------------------------
def list_problem(W, H, w, seed, kind="mixed"):
    """state and cnt images (cnt free): every state value, |S| on both sides of the threshold"""
    rng = np.random.default_rng(seed)
    K1 = mr.strong_threshold(w)
    state = rng.choice(np.array([0, 1, 1, 1, 2, 3], np.uint8), size=(H, W))
    cnt = rng.choice(np.array([0, 1, K1 - 1, K1, K1 + 1, K1 + 400], np.int32), size=(H, W))
    if kind == "all in":
        state[...] = mr.ST_IN
    elif kind == "none in":
        state[state == mr.ST_IN] = mr.ST_OUT
    elif kind == "strong only":
        cnt = np.maximum(cnt, K1).astype(np.int32)
    elif kind == "weak only":
        cnt = np.minimum(cnt, K1 - 1).astype(np.int32)
    elif kind == "large":
        state[...] = mr.ST_IN
        cnt[...] = 1 << 20
    return state, cnt


def check_lists(hipctx, state, cnt, w, rb, re, what):
    H, W = state.shape
    K1 = mr.strong_threshold(w)
    strong, weak, ns, nw, total = hipctx.selftest_active_lists(t(state), t(cnt), w, rb, re, fill=-7)
    hipctx.synchronize()
    strong, weak = strong.cpu().numpy(), weak.cpu().numpy()
    own = np.zeros((H, W), bool)
    own[rb:re] = True
    sel = own & (state == mr.ST_IN)
    want_s, want_w = np.flatnonzero((sel & (cnt >= K1)).reshape(-1)), np.flatnonzero((sel & (cnt < K1)).reshape(-1))
    assert (ns, nw) == (want_s.size, want_w.size), what
    assert np.array_equal(np.sort(strong[:ns]), want_s) and np.array_equal(np.sort(weak[:nw]), want_w), what
    assert (strong[ns:] == -7).all() and (weak[nw:] == -7).all(), what + ("written past the list's end",)
    assert total == int(cnt.astype(np.int64)[sel].sum()), what
    return ns, nw, total


# (W, H, first owned line, owned lines): owned ranges of 8191, 8192 and 8193 pixels around the 8 x 1024 pixels of a workgroup, two workgroups and a
# pixel, 1 and 63 pixels; a line of the frame follows every owned range, and row_begin * W is no multiple of 64 in six of the nine
LIST_SHAPES = [(8191, 3, 1, 1), (64, 131, 2, 128), (8192, 3, 1, 1), (2731, 5, 1, 3), (16385, 3, 1, 1), (1, 3, 1, 1), (63, 3, 1, 1), (9, 10, 2, 7), (37, 29, 0, 28)]


@pytest.mark.parametrize("kind", ["mixed", "all in", "none in", "strong only", "weak only"])
def test_list_compaction_equals_the_sets(hipctx, kind):
    for i, (W, H, rb, rows) in enumerate(LIST_SHAPES):
        assert rb + rows < H
        for w in (1, 0, 2):
            state, cnt = list_problem(W, H, w, 100 * i + w, kind)
            if kind != "none in":                                    # the pixel behind the owned range is processed and strong: it must not be listed
                state[rb + rows, 0], cnt[rb + rows, 0] = mr.ST_IN, mr.strong_threshold(w) + 3
            ns, nw, _ = check_lists(hipctx, state, cnt, w, rb, rb + rows, (kind, W, H, rb, rows, w))
            if kind == "all in":
                assert ns + nw == rows * W
            if kind in ("none in", "weak only"):
                assert ns == 0
            if kind in ("none in", "strong only"):
                assert nw == 0
    assert (8191, 8192, 8193) == tuple(sorted(r * W for (W, H, rb, r) in LIST_SHAPES)[k] for k in (4, 6, 7))
    assert sum((rb * W) % 64 != 0 for (W, H, rb, r) in LIST_SHAPES) >= 6


def test_list_compaction_sums_past_32_bits(hipctx):
    state, cnt = list_problem(2731, 5, 1, 5, "large")
    ns, nw, total = check_lists(hipctx, state, cnt, 1, 1, 4, "large")
    assert ns == 8193 > 4096 and nw == 0 and total == 8193 << 20 and total > 1 << 32


def test_list_compaction_behind_a_skip_word(hipctx):
    import torch
    state, cnt = list_problem(64, 131, 1, 9)
    for word, skipped in ((0, False), (1, True), (1 << 40, True), (-1, True)):
        sw = torch.tensor([word], dtype=torch.int64, device="cuda")
        strong, weak, ns, nw, total = hipctx.selftest_active_lists(t(state), t(cnt), 1, 2, 130, sw, fill=-7)
        hipctx.synchronize()
        if skipped:
            assert (ns, nw, total) == (0, 0, 0) and (strong == -7).all() and (weak == -7).all(), word
        else:
            assert ns > 0 and nw > 0 and total > 0 and int((strong != -7).sum()) == ns and int((weak != -7).sum()) == nw
