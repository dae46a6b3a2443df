"""CPU tests of the marking stage's test bed: the generators of tests/marking_cases.py keep their contract, and tests/marking_ref.py (the
sequential restatement of the reference's marking strategy) agrees with two independent statements of the same thing: the fixed-point
characterisation, by brute force, and the oracle's processed set on a natural frame."""
import numpy as np
import pytest

import marking_cases as mc
import marking_ref as mr


def check_contract(case):
    W, H, w, b = case.W, case.H, case.w, case.b
    side, n, kc = mc.window(b)
    assert case.mask.shape == (H, W, (n + 31) // 32) and case.mask.dtype == np.uint32 and case.cnt.shape == (H, W) and case.cnt.dtype == np.int32
    bits = mr.unpack(case.mask, b)
    assert np.array_equal(mr.pack(bits), case.mask), "bits above the window's last one"
    main = mr.main_area(W, H, w)
    assert not bits[~main].any() and not case.cnt[~main].any(), "pixels outside the main area carry nothing"
    for k in range(n):
        dl, dc = mc.offset(k, b)
        assert not (bits[:, :, k] & ~mc._shifted(main, dl, dc)).any(), ("a bit points outside the main area", k)
        assert np.array_equal(bits[:, :, k], mc._shifted(bits[:, :, n - 1 - k], dl, dc)), ("symmetry", k)
    assert np.array_equal(bits[:, :, kc], main), "every main pixel is in its own set"
    if case.popcount:
        assert np.array_equal(case.cnt, bits.sum(-1))


@pytest.mark.parametrize("family", ["random", "full", "threshold", "chain", "isolated"])
def test_generated_cases_keep_the_contract(family):
    sel = [c for c in mc.cases() if c.family == family]
    assert sel
    for c in sel:
        check_contract(c)
        assert c.popcount == (family in ("random", "full"))


def test_case_list_covers_what_it_claims():
    cs = mc.cases()
    for b in mc.RADII:
        for fam in ("random", "full"):
            assert {(c.W, c.H) for c in cs if c.b == b and c.family == fam} >= set(mc.sizes(b))
    assert {c.w for c in cs} == {0, 1, 2}
    assert any(len(mc.orders(c)) == 4 and c.b == 3 and c.H == 33 for c in cs) and any(len(mc.orders(c)) == 4 and c.b == 6 and c.H == 40 for c in cs)
    assert (mc.pair_count(6), mc.pair_count(12)) == (84, 312)
    # threshold cases hold both sides of 3 P + 1 and nothing else
    for c in cs:
        if c.family == "threshold":
            K1 = mr.strong_threshold(c.w)
            assert set(np.unique(c.cnt[mr.main_area(c.W, c.H, c.w)])) == {K1 - 1, K1}
    # b = 1, w = 1: a window of 9 never reaches 28
    c = mc.by_name("full b=1 17x16 w=1")
    assert c.cnt.max() == 9 < mr.strong_threshold(1)


@pytest.mark.parametrize("b", [3, 8, 6, 12])
def test_one_offset_cases_keep_the_contract(b):
    W, H, w = mc.ONE_OFFSET_FRAMES[b]
    assert W * H <= 1300 and W > 16 and H > 16
    side, n, kc = mc.window(b)
    seen = set()
    for k in range(mc.pair_count(b)):
        c = mc.one_offset(W, H, w, b, k)
        if k % 7 == 0 or k in (31, 32) or k == kc - 1:               # (the full check is a loop over the window: a sample of the pairs, the rest by popcount)
            check_contract(c)
        bits = mr.unpack(c.mask, b)
        assert 2 <= bits.sum(-1).max() <= 3 and set(np.flatnonzero(bits.any((0, 1)))) == {k, kc, n - 1 - k}
        seen |= {k, n - 1 - k}
    assert seen == set(range(n)) - {kc}                              # every bit of the window, the last one of the last word included
    assert (n - 1) >> 5 == c.mask.shape[2] - 1


def dependency_depth(case, order):
    """longest run p1, p2, ... in which each pixel is a strong similar neighbour visited earlier than the next one"""
    ptr, idx = mr.members(case.mask, case.b)
    strong = case.cnt.reshape(-1) >= mr.strong_threshold(case.w)
    depth = np.zeros(case.W * case.H, np.int64)
    done = np.zeros(case.W * case.H, bool)
    for p in order.tolist():
        q = idx[ptr[p]:ptr[p + 1]]
        q = q[done[q] & strong[q] & (q != p)]
        depth[p] = 1 + (depth[q].max() if q.size else 0)
        done[p] = True
    return int(depth.max())


def test_chain_depths_are_what_the_generator_states():
    sel = [c for c in mc.cases() if c.family == "chain"]
    assert len(sel) >= 7
    for c in sel:
        assert dependency_depth(c, mc.visit(c, 0, 0)) == c.depth, c.name
    c = mc.by_name("chain horizontal b=6 300x18 w=1")
    assert c.depth == c.W - 2 == 298                                 # 19 tiles side by side
    assert mc.by_name("chain vertical b=6 18x130 w=1").depth == 128


def fixed_point_holds(case, order, drawn, state):
    """brute force: p is processed <=> p's draw says "never skip", or no q != p of S(p) is visited earlier, strong and processed"""
    W, H, b = case.W, case.H, case.b
    side = 2 * b + 1
    rank = np.full(W * H, -1, np.int64)
    rank[order] = np.arange(order.size)
    bits = mr.unpack(case.mask, b)
    K1 = mr.strong_threshold(case.w)
    main = mr.main_area(W, H, case.w)
    for l in range(H):
        for c in range(W):
            if not main[l, c]:
                if state[l, c] != mr.ST_NONE:
                    return False
                continue
            hit = False
            for k in np.flatnonzero(bits[l, c]):
                ql, qc = l + k // side - b, c + k % side - b
                if (ql, qc) != (l, c) and case.cnt[ql, qc] >= K1 and rank[ql * W + qc] < rank[l * W + c] and state[ql, qc] == mr.ST_IN:
                    hit = True
            want = mr.ST_OUT if (hit and drawn[l, c]) else mr.ST_IN
            if state[l, c] != want:
                return False
    return True


def test_greedy_satisfies_the_fixed_point_characterisation():
    names = ["random 0.30 b=3 16x33 w=1", "random 0.90 b=1 17x16 w=1", "full b=6 16x16 w=1", "threshold random checker b=3 16x33 w=1",
             "chain serpentine b=1 40x24 w=0", "random 0.30 b=6 33x18 w=1 (bands)", "full b=3 3x3 w=1"]
    for name in names:
        case = mc.by_name(name)
        for (mode, seed) in mc.orders(case):
            for m in (1.0, 0.5):
                order = mc.visit(case, mode, seed)
                drawn = mr.skip_draw(case.W, case.H, m, seed)
                st = mc.reference(case, mode, seed, m)
                assert fixed_point_holds(case, order, drawn, st), (name, mode, seed, m)
                assert not (st == mr.ST_UNDECIDED).any()
        assert (mc.reference(case, 0, 0, 0.0) == mr.ST_IN).sum() == (case.W - 2 * case.w) * (case.H - 2 * case.w)


def test_fixed_point_check_notices_a_wrong_state():
    case = mc.by_name("random 0.30 b=6 33x18 w=1 (bands)")
    order, drawn = mc.visit(case, 0, 0), mr.skip_draw(case.W, case.H, 1.0, 0)
    st = mc.reference(case, 0, 0, 1.0).copy()
    assert (st == mr.ST_OUT).any() and (st == mr.ST_IN).any()
    l, c = np.argwhere(st == mr.ST_OUT)[0]
    st[l, c] = mr.ST_IN
    assert not fixed_point_holds(case, order, drawn, st)


def test_skip_draw_restates_the_oracle_engines_arithmetic():
    """same numbers as the draw of tests/oracle_engine.py (which the band tests hold against the engine), global index included"""
    import oracle_engine
    import torch
    eng = oracle_engine.OracleEngine(None)
    for (W, H, m, seed, off) in [(33, 18, 0.25, 11, 0), (17, 40, 0.5, 4242, 23), (300, 18, 0.75, 0, 1000)]:
        st = eng.active_init(torch.zeros((H, W), dtype=torch.int32), 0, 0, H, m, seed, off).numpy()
        assert np.array_equal(st == 3, mr.skip_draw(W, H, m, seed, off))
    assert mr.skip_draw(5, 4, 1.0, 3).all() and not mr.skip_draw(5, 4, 0.0, 3).any()


@pytest.mark.parametrize("random_order", [0, 1])
def test_greedy_equals_the_oracles_processed_set_on_a_natural_frame(random_order):
    """the frame of test_processed_set_matches_reference_order: masks and processed set from the oracle, the order from the library's key"""
    import bcd_amd.hip as bh
    import oracle_lib as ol
    W, H, w, b = 72, 50, 1, 6
    col, ns, hist, cov, _ = ol.synth_inputs(W, H, 16, 1234, 0.35, 0.0)
    order = bh.visit_order(W, H, w, random_order, 77)
    _, (proc, fb, nsim) = ol.denoise_mono(col, ns, hist, cov, ol.params(m=1.0), order=order, want_diag=True)
    mask, cnt = ol.similarity_masks(ns, hist, w, b, 1.0)
    st = mr.greedy(mask, cnt, w, b, order, mr.skip_draw(W, H, 1.0, 77))
    assert np.array_equal(st == mr.ST_IN, proc == 1)
    assert (st == mr.ST_OUT).any() and np.array_equal(st != mr.ST_NONE, mr.main_area(W, H, w))
