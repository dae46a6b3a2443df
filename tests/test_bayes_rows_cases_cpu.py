"""CPU tests of the row-band cases (tests/bayes_rows_cases.py): what tests/test_gpu_bayes_rows.py relies on, stated for the float64 reference alone.

For every (case, cut list) pair the GPU tests run, the references of the bands -- bayes_ref.accumulate on the case with the states outside the band
zeroed -- add up to the reference of the frame: the counts exactly, the sums within 1e-12 of the frame's largest value (measured: 0 on the isolated
cases, where a pixel belongs to one item, at most 3.3e-15 on the dense ones).  So a kernel that is held to every band's reference and to the frame's
reference of the bands called one after the other is held to one consistent thing.  The lists themselves: every one has a band with items and one
without; over all of them there are a boundary inside a 16-line tile and one on a multiple of 16, a single line, an empty band; the dense 3 x 3 cases
that have fallback items have them beside full estimates in at least two bands (the tiled fallback kernel's row test is cut through by a band edge
with work on both sides).  The speculative and chain tests: how many items the `call sequence` calls own in lines [7, 41), and that the chain
problem has owned pixels that cannot be decided while the halo lines are undecided -- the reason its first round is always skipped."""
import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br
import bayes_rows_cases as rc
import marking_cases as mc
import marking_ref as mr
from test_gpu_marking_stage import waits_for_the_halo

NAMES = [n for _, n in rc.SELECTED]


def test_every_selected_case_exists_and_has_a_cut_list():
    assert len(set(NAMES)) == len(NAMES) == 15 and set(NAMES) == set(rc.CUTS)
    for family, name in rc.SELECTED:
        c = rc.case(name)
        assert family in bc.FAMILIES and c.name == name
        cuts = rc.CUTS[name]
        assert cuts[0] == 0 and cuts[-1] == c.col.shape[0] and all(a <= b for a, b in zip(cuts[:-1], cuts[1:])), name
        assert rc.call_range(c, *rc.bands(name)[0])[0] == -3 and rc.call_range(c, *rc.bands(name)[-1])[1] == c.col.shape[0] + 5
        assert c.col.shape[0] <= 110 and c.col.shape[1] <= 160
    inner = [r for n in NAMES for r in rc.CUTS[n][1:-1]]
    assert any(r % 16 == 0 for r in inner) and any(r % 16 != 0 for r in inner)
    widths = [b - a for n in NAMES for a, b in rc.bands(n)]
    assert 1 in widths and 0 in widths


@pytest.mark.parametrize("name", NAMES)
def test_band_references_add_up_to_the_frame(name):
    c = rc.case(name)
    K1 = 3 * (2 * c.w + 1) ** 2 + 1
    s64, c64, items = br.accumulate(*c.args(), keep_stages=False)
    s_sum, c_sum = np.zeros_like(s64), np.zeros_like(c64)
    per_band = []
    for (r0, r1) in rc.bands(name):
        o = rc.banded(c, r0, r1)
        assert np.array_equal(o.state[r0:r1], c.state[r0:r1]) and not o.state[:r0].any() and not o.state[r1:].any()
        s, n, it = br.accumulate(*o.args(), keep_stages=False)
        assert [i["pos"] for i in it] == [i["pos"] for i in items if r0 <= i["pos"][0] < r1]
        # what a band writes stays within b + w lines of it (the halo the band driver exchanges)
        touched = np.flatnonzero(n.any(axis=1))
        assert touched.size == 0 or (touched.min() >= r0 - c.b - c.w and touched.max() < r1 + c.b + c.w), (name, r0, r1)
        with np.errstate(invalid="ignore"):
            s_sum += s
        c_sum += n
        per_band.append((sum(1 for i in it if i["n"] < K1), sum(1 for i in it if i["n"] >= K1)))
        # the poisoned states differ from the case's outside the band only, and do differ there
        p = rc.poisoned_state(c, r0, r1)
        assert np.array_equal(p[r0:r1], c.state[r0:r1])
        if r1 - r0 < c.state.shape[0] - 2 * c.w:
            assert (np.delete(p, np.s_[r0:r1], axis=0) == mr.ST_IN).any() and (np.delete(p, np.s_[r0:r1], axis=0) == mr.ST_UNDECIDED).any()
    assert np.array_equal(c_sum, c64), name
    ok = np.isfinite(s64)
    assert np.array_equal(np.isfinite(s_sum), ok), name
    err = float(np.max(np.abs(s_sum[ok] - s64[ok])) / np.max(np.abs(s64[ok])))
    print("bands of %-30s fallback / full items per band %s, sums add up to %.1e" % (name, per_band, err))
    assert err <= 1e-12, (name, err)
    assert any(a + b > 0 for a, b in per_band) and any(a + b == 0 for a, b in per_band), (name, per_band)
    assert sum(a for a, _ in per_band) == sum(1 for i in items if i["n"] < K1)
    if c.dense and c.w == 1:
        if name == "borders dense full windows":                     # (every clipped window holds at least 7 x 7 pixels: full estimates only)
            assert all(a == 0 for a, _ in per_band)
        else:
            assert sum(1 for a, b in per_band if a > 0 and b > 0) >= 2, (name, per_band)
    if name == "sizes dense":
        assert (sum(a for a, _ in per_band), len(items)) == (273, 1216)


def test_call_sequence_items_in_the_speculative_band():
    """lines [7, 41) of the four `call sequence` calls: the third call's count sets a hint above 512, so that the skipped and the wanted call that
    follow it have the first chunk of estimate kernels launched ahead"""
    counts = [int(c.state[7:41].sum()) for c in bc.call_sequence()]
    print("call sequence, items in lines [7, 41):", counts)
    assert counts[2] >= 512 and counts[2] + counts[2] // 8 + 1024 < (1 << 18) and 0 < counts[3] < 512
    assert all(n > 0 for n in counts)


def test_word_problems_wait_for_their_halo():
    """the marking problems the word is read on: in 7 of the 8 with m = 1 an owned pixel waits for an undecided halo line, so the word is seen with a count
    (m < 1 is left out: a pixel the draw spares is processed whatever its neighbours do, and the criterion does not look at the draw)"""
    from test_gpu_marking_stage import bands_of
    case = mc.by_name("random 0.30 b=6 15x40 w=1")
    n = 0
    for (mode, seed) in ((0, 0), (1, 11)):
        want = mc.reference(case, mode, seed, 1.0)
        for (r0, r1) in bands_of(case.H):
            n += waits_for_the_halo(case, want, mc.visit(case, mode, seed), max(0, r0 - case.b), r0, r1, min(case.H, r1 + case.b))
    assert n >= 7, n


@pytest.mark.parametrize("order", [(0, 0), (1, 11)], ids=["scanline", "random"])
def test_chain_problem_waits_for_its_halo(order):
    c, g = rc.chain_problem()
    r0, r1 = rc.CHAIN_BAND
    mode, seed = order
    want = mc.reference(g, mode, seed, 1.0)
    assert waits_for_the_halo(g, want, mc.visit(g, mode, seed), r0 - g.b, r0, r1, r1 + g.b)
    band = rc.banded(rc.with_state(c, np.where(want == mr.ST_IN, 1, 0), "chain"), r0, r1)
    n = band.nsim[band.state == 1]
    print("chain problem, order %d: %d processed pixels in the band, %d of them fallback" % (mode, n.size, int((n < 28).sum())))
    assert (n >= 28).sum() >= 20 and (n < 28).sum() >= 1
    assert np.array_equal(br.popcount(c.mask), c.nsim)
