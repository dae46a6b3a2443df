"""CPU tests that hold the cross-frame selection reference (tests/temporal_ref.py) to its claims, without a GPU.

  * a neighbour identical to the frame: the cross distances are the in-frame distances of tests/similarity_ref.py bit for bit at every window offset
    (diff = n2 b1 - n1 b2 changes sign with the roles of the two pixels, its square and the commutative products do not), so the cross reference inherits
    what tests/test_similarity_cases_cpu.py establishes against the compiled oracle;
  * a neighbour that is the frame rolled by (2, -3): the distance is exactly 0 at that displacement wherever both patches are valid, and the planes of
    that displacement are zero sums over the full bin counts;
  * masks: bit layout, |S_f|, NaN and +inf never similar;
  * the estimate reference over members of several frames: with one frame it is tests/bayes_ref.py bit for bit; the neighbours lend statistics only; the
    float32 calibrator stays meaningful on every family of tests/temporal_bayes_cases.py;
  * one scale of the whole composition without neighbours: the oracle's frame on the committed 40 x 28 fixture."""
import os

import numpy as np
import pytest

import bayes_ref as br
import marking_ref as mr
import similarity_ref as sr
import temporal_bayes_cases as tb
import temporal_cases as tc
import temporal_ref as tr

F = np.float32


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("W,H,D,b,w,kind", [(20, 16, 60, 6, 1, 16), (33, 21, 60, 3, 2, "mixed"), (12, 11, 24, 3, 0, 24), (9, 14, 15, 4, 1, 1)])
def test_identical_neighbour_gives_the_in_frame_distances_bit_for_bit(W, H, D, b, w, kind):
    hist, ns = tc.frame(W, H, D, kind, seed=3)
    cross = tr.cross_distances32(hist, ns, hist, ns, b, w)
    own = sr.distances32(hist, ns, b, w)
    assert same_bits(cross, own)
    assert np.isfinite(own).any()
    if kind == 1:
        assert np.isnan(own).any()                                   # (the 1-spp frame has patch pairs without a counted bin)
    for tau in (F(0), F(0.5), F(1), F(np.inf)):
        m1, n1 = sr.masks_from(cross, tau)
        m2, n2 = sr.masks(hist, ns, w, b, tau)
        assert np.array_equal(m1, m2) and np.array_equal(n1, n2)


@pytest.mark.parametrize("kind", [16, "mixed"])
def test_rolled_neighbour_has_distance_zero_at_its_displacement(kind):
    W, H, D, b, w = 24, 18, 60, 6, 1
    dl, dc = 2, -3
    hist, ns = tc.frame(W, H, D, kind, seed=5)
    hist_nb, ns_nb = np.roll(hist, (dl, dc), axis=(0, 1)), np.roll(ns, (dl, dc), axis=(0, 1))      # nb[l + 2, c - 3] = frame[l, c]
    d = tr.cross_distances32(hist, ns, hist_nb, ns_nb, b, w)
    k = (dl + b) * (2 * b + 1) + (dc + b)
    valid = sr.window_valid(W, H, w, b)[:, :, k]
    assert valid.sum() == (H - 2 * w - dl) * (W - 2 * w + dc)
    assert np.array_equal(d[:, :, k][valid], np.zeros(valid.sum(), F))
    assert np.isinf(d[:, :, k][~valid]).all()
    assert (d[np.isfinite(d)] > 0).any()                             # (other displacements are not degenerate)
    mask, cnt = sr.masks_from(d, F(0))
    assert (((mask[:, :, k >> 5] >> np.uint32(k & 31)) & 1).astype(bool) == valid).all()
    assert (cnt[valid] >= 1).all()


def test_planes_are_not_symmetric_between_two_frames():
    """T_delta(x) and T_-delta(x + delta) are different pixel pairs between two frames: every displacement needs its own plane"""
    case = tc.by_name("20x16")
    T, C, valid = tr.cross_planes32(*case.frames, case.b)
    b, side = case.b, 2 * case.b + 1
    k_fwd, k_bwd = (1 + b) * side + (2 + b), (-1 + b) * side + (-2 + b)
    assert valid[k_fwd, :-1, :-2].all() and valid[k_bwd, 1:, 2:].all()
    assert not np.array_equal(T[k_fwd, :-1, :-2], T[k_bwd, 1:, 2:])


def test_masks_skip_nan_and_outside():
    case = tc.by_name("20x16 1 spp against 1 spp")
    d = case.dist
    assert np.isnan(d).any() and np.isinf(d).any() and np.isfinite(d).any()
    mask, cnt = case.reference(F(np.inf))
    assert np.array_equal(cnt, np.isfinite(d).sum(-1))
    side = 2 * case.b + 1
    bits = np.unpackbits(mask.view(np.uint8), axis=-1, bitorder="little")[:, :, :side * side].astype(bool)
    assert np.array_equal(bits, np.isfinite(d))
    w = case.w
    border = np.ones((case.H, case.W), bool)
    border[w:case.H - w, w:case.W - w] = False
    assert (cnt[border] == 0).all()


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_case_has_thresholds_on_its_distances(name):
    case = tc.by_name(name)
    taus = case.taus
    d = case.dist
    if name == "20x16 1 spp against 1 spp":                          # coinciding bins give diff = 0: distances are 0 or NaN, one threshold serves
        assert taus == [F(0)] and np.isnan(d).any() and (d == 0).any() and not (d[np.isfinite(d)] > 0).any()
        return
    if "1 spp" in name and case.w == 0:
        assert np.isnan(d).any()
    assert len(taus) >= 4, (name, taus)
    hits = sum(int(np.count_nonzero(d == t)) for t in taus)
    assert hits >= 3, (name, hits)                                   # thresholds that equal distances of the case
    sizes = {int(case.reference(t)[1].sum()) for t in taus}
    assert len(sizes) >= 3, (name, sizes)                            # ... and that select different sets


# ---- the estimate reference over members of several frames ------------------------------------------------------------------------------------------


def test_one_frame_estimate_reference_is_bayes_ref():
    """F = 0: the same operations in the same order as tests/bayes_ref.py -- equal bit for bit, in both precisions"""
    case = tb.fam_sizes(1, 201)
    one = tb.single_frame_of(case)
    col, pixcov, mask, nsim, state, w, b, min_eig = one
    for dtype in (np.float64, np.float32):
        s0, c0, items0 = br.accumulate(*one, dtype=dtype, keep_stages=False)
        s1, c1, items1 = tr.accumulate([(col, pixcov, mask)], nsim, state, w, b, min_eig, dtype=dtype)
        assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
        assert [i["pos"] for i in items0] == [i["pos"] for i in items1] and [i["n"] for i in items0] == [i["n"] for i in items1]
        assert int((c1 > 0).sum()) > 0 and any(i["n"] >= tb.K1 for i in items1) and any(i["n"] < tb.K1 for i in items1)


def test_neighbours_lend_statistics_only():
    """the estimates are aggregated for the in-frame members alone, whatever the neighbours add: the count image is one per patch pixel of every in-frame
    member of a full estimate and of the main patch of a fallback; with the same in-frame sets, neighbours move the full estimates and not the counts"""
    case = tb.fam_sizes(2, 202)
    s, c, items = tr.accumulate(*case.args())
    want = np.zeros_like(c)
    offs = br.offsets(case.w)
    for it in items:
        centres = it["members"] if it["n"] >= tb.K1 else np.array([it["pos"]])
        for (l, cc) in centres:
            for (a, d) in offs:
                want[l + a, cc + d] += 1
    assert np.array_equal(c, want)
    assert any(it["n"] >= tb.K1 and len(it["members"]) == 1 for it in items)          # a full estimate that lives on the neighbours' members
    one = tb.single_frame_of(case)
    s0, c0, items0 = br.accumulate(*one, keep_stages=False)
    both = [(a, b_) for a, b_ in zip(items0, items) if a["n"] >= tb.K1 and b_["n"] > a["n"]]
    assert len(both) >= 2
    for a, b_ in both:
        r, cc = br.touched(b_, case.w)
        assert np.array_equal(c0[r, cc], c[r, cc]) and not np.allclose(s0[r, cc], s[r, cc], rtol=1e-9, atol=0)


@pytest.mark.parametrize("family", sorted(tb.FAMILIES))
def test_float32_calibrator_stays_meaningful_on_every_family(family):
    """the bar of the GPU test is a multiple of the calibrator's error: it must be small, and no finite item may be excluded"""
    for case in tb.FAMILIES[family]():
        s64, c64, items = tr.accumulate(*case.args())
        s32, c32, _ = tr.accumulate(*case.args(), dtype=np.float32)
        assert np.array_equal(c64, c32) and np.array_equal(np.isfinite(s64), np.isfinite(s32))
        e32 = [br.item_error(s32, s64, it, case.w) for it in items if it["n"] >= tb.K1 and np.isfinite(s64[br.touched(it, case.w)]).all()]
        assert len(e32) >= 3 and max(e32) <= 1e-2, (case.name, len(e32), max(e32))


def test_one_scale_composition_without_neighbours_matches_the_oracle_fixture():
    """F = 0, -m 0, scanline order on the committed 40 x 28 fixture: the composition's masks are the fixture's and its frame is the oracle's within the
    bar tests/test_bayes_ref_cpu.py uses for the same fixture"""
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "core_regression.npz"))
    H, W, _ = f["col"].shape
    w, b = 1, 6
    order = np.array([l * W + c for l in range(w, H - w) for c in range(w, W - w)])
    out, stats, state = tr.denoise_one_scale((f["col"], f["ns"], f["hist"], f["cov"]), [], w, b, 1.0, 1e-8, order, mr.skip_draw(W, H, 0.0, 0))
    mask, cnt = sr.masks(f["hist"], f["ns"], w, b, 1.0)
    assert np.array_equal(mask, f["mask"]) and np.array_equal(cnt, f["cnt"])
    assert stats["processed"] == (H - 2 * w) * (W - 2 * w) and stats["similar_total"] == int(f["cnt"][w:H - w, w:W - w].sum())
    err = np.max(np.abs(out - f["out_m0"])) / np.max(np.abs(f["out_m0"]))
    assert err < 1e-5, err


def test_the_reference_alone_satisfies_the_benefit_inequality():
    """the configuration of the GPU benefit test (52 x 36, 16 spp, sigma 0.5, two neighbours): the NumPy composition's RMSE against the noise-free base is
    below the single-frame composition's -- size and sigma of that test were chosen by this check"""
    import oracle_lib as ol
    import bcd_amd.hip as bh
    W, H = 52, 36
    frames, base = [], None
    for seed in (1234, 77, 4321):
        col, ns, hist, cov, base0 = ol.synth_inputs(W, H, 16, seed, 0.5, 0.0)
        frames.append((col, ns, hist, cov))
        base = base0 if base is None else base
    order, drawn = bh.visit_order(W, H, 1, 1, 1234), mr.skip_draw(W, H, 1.0, 1234)
    plain, _, _ = tr.denoise_one_scale(frames[1], [], 1, 6, 1.0, 1e-8, order, drawn)
    both, _, _ = tr.denoise_one_scale(frames[1], [frames[0], frames[2]], 1, 6, 1.0, 1e-8, order, drawn)
    rmse = lambda x: float(np.sqrt(np.mean((x[1:-1, 1:-1] - base[1:-1, 1:-1]) ** 2)))
    assert rmse(both) < rmse(plain), (rmse(both), rmse(plain))
