"""CPU tests of the constructed similarity frames (tests/similarity_cases.py) and of the NumPy emulation they are judged by (tests/similarity_ref.py).

The GPU tests compare the kernels with similarity_ref; here similarity_ref is held to the compiled oracle (oracle/bcd_oracle.c) bit for bit -- masks and |S|
at every threshold of every case, window distances at the pixels the GPU tests read -- so the oracle stays the arbiter.  The second half holds the
families to what they claim: the list overflows where it should, binary16 rounds as far as the search promised, the ladders tie and straddle."""
import time

import numpy as np
import pytest

import oracle_lib as ol
import similarity_cases as sc
import similarity_ref as sr

F = np.float32
SMALL = sc.names(large=False)
LARGE = sc.names(large=True)


def marks_of(case):
    """main pixels whose window distances are compared: the corners of the main area, the pixels on the seam, the guard pixels"""
    w, W, H = case.w, case.W, case.H
    pix = {(w, w), (w, W - 1 - w), (H - 1 - w, w), (H - 1 - w, W - 1 - w)} | set(case.marks)
    if case.seam:
        cb, lb = case.seam
        pix |= {(min(max(lb, w), H - 1 - w), min(max(cb, w), W - 1 - w)), (min(max(lb - 1, w), H - 1 - w), min(max(cb - 1, w), W - 1 - w))}
    return sorted(pix)


@pytest.mark.parametrize("name", SMALL)
def test_emulation_equals_the_oracle_at_every_threshold(name):
    case = sc.by_name(name)
    assert len(case.taus) >= 3
    for tau in case.taus:
        mask, cnt = case.reference(tau)
        wmask, wcnt = ol.similarity_masks(case.ns, case.hist, case.w, case.b, float(tau))
        assert np.array_equal(mask, wmask) and np.array_equal(cnt, wcnt), (name, float(tau))
    for (l, c) in marks_of(case):
        want = ol.window_distances(case.ns, case.hist, case.w, case.b, l, c)
        assert np.array_equal(case.dist[l, c].view(np.uint32), want.view(np.uint32)), (name, l, c)


@pytest.mark.parametrize("name", LARGE)
def test_large_cases_on_a_crop_and_by_their_period(name):
    """a 160 x 48 crop of a large frame: the emulation equals the oracle, and one period of distances tiled over the crop equals the emulation -- the form
    the full-size reference takes (the full-size emulation itself: 2 s for the sparse plateau, over 30 s for the fully occupied histograms)"""
    case = sc.by_name(name)
    W, H = 160, 48
    hist, ns = case.make(W, H)
    dist = sr.distances32(hist, ns, case.b, case.w, case.bins)
    valid = sr.window_valid(W, H, case.w, case.b)
    assert len(case.taus) == 3
    for tau in case.taus:
        mask, cnt = sr.masks_from(dist, tau)
        wmask, wcnt = ol.similarity_masks(ns, hist, case.w, case.b, float(tau))
        assert np.array_equal(mask, wmask) and np.array_equal(cnt, wcnt)
        tmask, tcnt = sr.tile_masks(case.dist, valid, tau)
        assert np.array_equal(tmask, mask) and np.array_equal(tcnt, cnt)
    assert sc.ties(dist, case.b, case.taus[0]) >= 1000


def test_full_size_reference_of_a_large_case_is_quick():
    case = sc.by_name("large sparse 1000x400 b=6")
    t0 = time.perf_counter()
    mask, cnt = case.reference(case.taus[0])
    assert mask.shape == (400, 1000, 6) and time.perf_counter() - t0 < 30.0
    assert 0 < int(cnt.sum()) < cnt.size * 169


# ---- the families do what they claim ---------------------------------------------------------------------------------------
def test_checkerboard_overflows_the_list_and_the_sparse_plateau_does_not():
    for variant in ("n16", "n12"):
        c = sc.by_name("plateau checker 64x40 " + variant)
        for tau in (c.values[0], sr.prev(c.values[0]), sr.next_(c.values[0])):
            assert sc.in_band(c.dist, c.b, tau) > sc.capacity(c.W, c.H)
    for variant in sc.VARIANTS:
        c = sc.by_name("plateau sparse 64x40 " + variant)
        for v in c.values:
            assert 1000 < sc.in_band(c.dist, c.b, v) < sc.capacity(c.W, c.H) // 2
    c = sc.by_name("plateau stripes 64x40 n16")
    assert len(set(float(v) for v in c.values)) == 3


def test_limit_plateaus_sit_exactly_on_the_ends_of_the_binary16_range():
    c = sc.by_name("limits 2^-6 and 64 64x40")
    assert sc.ties(c.dist, c.b, sc.TAU_MIN) >= 1000 and sc.ties(c.dist, c.b, sc.TAU_MAX) >= 1000
    assert sr.prev(sc.TAU_MIN) in c.taus and sr.next_(sc.TAU_MAX) in c.taus


@pytest.mark.parametrize("word,sign", [("down", -1), ("up", 1)])
def test_half_family_reaches_nine_tenths_of_the_binary16_bound(word, sign):
    c = sc.by_name("half rounds %s 40x24 n16" % word)
    T, C, valid = sr.planes32(c.hist, c.ns, c.b, c.bins)
    t = np.unique(T[valid & (T > 0)])
    assert t.size == 1                                               # one cross term: all nine entries of a patch are this number
    rel = float(sr.half(t[0])) / float(t[0]) - 1.0
    assert sign * rel >= 0.9 * 2.0 ** -11 and rel == c.half_rel
    d = float(c.values[0])
    for f in sc.HALF_OFFSETS:                                        # d_ref on either side of the listed thresholds, at f 2^-10 from them
        for s in (1, -1):
            tau = F(d / F(1 + s * f * 2.0 ** -10))
            assert tau in c.taus and abs(d / float(tau) - 1 - s * f * 2.0 ** -10) < 2.0 ** -22


def test_counts_family_has_the_edge_bins_the_empty_patches_and_the_full_ones():
    c = sc.by_name("counts edge and empty 48x32 n16")
    h = c.hist
    types = {tuple(h[l, cc, 40:42]) for l in range(c.H) for cc in range(c.W)}
    assert (F(0.75), F(0)) in types and (F(0.25), F(0.25) + F(2.0 ** -23)) in types and (F(0.75), F(0.75)) in types
    assert F(0.75) + F(0.25) == F(1) and F(0.75) + (F(0.25) + F(2.0 ** -23)) == sr.next_(F(1))
    _, cnt = c.reference(c.taus[0])
    side = 2 * c.b + 1
    assert np.isnan(c.dist[16, 12, (side * side - 1) // 2])          # inside the empty block: 0 / 0 against itself
    assert int(cnt[16, 12]) == 0 and np.count_nonzero(cnt[1:-1, 1:-1] == 0) >= 50
    for D in (60, 36, 24):
        c = sc.by_name("counts full D=%d 40x24 n16" % D)
        T, C, valid = sr.planes32(c.hist, c.ns, c.b, c.bins)
        assert (C[valid] == D).all()                                 # every bin of every pair counts: D per pixel pair, 9 D per patch (540 at D = 60)
        assert len(c.bins) == D


def test_guard_family_sits_on_the_guards_and_one_ulp_outside():
    top, nlo, nhi = F(2.0 ** 20), F(2.0 ** -10), F(2.0 ** 16)
    for kind in sc.GUARD_KINDS:
        c = sc.by_name("guard %s 48x24" % kind)
        inside = c.hist.max() <= top and c.ns.min() >= nlo and c.ns.max() <= nhi
        assert inside == c.inside
        if kind == "uni":
            assert c.hist.max() == top and (c.ns == nhi).all()
        if kind == "mixed":
            assert c.hist.max() == top and c.ns.min() == nlo and c.ns.max() == nhi
    assert sc.by_name("guard out bin 48x24").hist.max() == sr.next_(top)
    assert sc.by_name("guard out n low 48x24").ns.min() == sr.prev(nlo)
    assert sc.by_name("guard out n high 48x24").ns.max() == sr.next_(nhi)


@pytest.mark.parametrize("name", [n for n in SMALL if not n.startswith(("limits", "drawn"))])
def test_every_ladder_ties_and_straddles_both_band_edges(name):
    """at its tie threshold a ladder has at least 1 000 pairs with d_ref == tau; among its thresholds within 2 ulp of RN(d / (1 -+ 2^-10)) the band edge
    the kernels compute -- RN(tau (1 -+ 2^-10)) in float32 -- falls on both sides of d"""
    case = sc.by_name(name)
    one = F(1)
    for d in case.values:
        assert sc.ties(case.dist, case.b, d) >= 1000, (name, float(d))
        assert d in case.taus
        if case.short:
            continue
        for edge in (one - sc.DELTA, one + sc.DELTA):
            centre = F(d / edge)
            group = [t for t in case.taus if abs(int(F(t).view(np.int32)) - int(centre.view(np.int32))) <= 2]
            assert len(group) == 5
            moved = [F(t * edge) for t in group]
            assert any(m < d for m in moved) and any(m >= d for m in moved) and any(m > d for m in moved) and any(m <= d for m in moved)


def test_drawn_counts_case_meets_every_pair_of_counts_and_still_ties():
    c = sc.by_name("drawn counts sparse 64x40")
    n = c.ns[:, :, 0]
    pairs = {(float(a), float(b)) for a, b in zip(n[:, :-1].ravel(), n[:, 1:].ravel())}
    assert len(pairs) == 16                                          # every (n1, n2) of {8, 12, 16, 24}^2 already among horizontal neighbours
    assert len(c.taus) == 24 and all(sc.ties(c.dist, c.b, d) == k >= 100 for d, k in c.drawn)
