"""CPU tests of the float64 / float32 reference of the Bayesian estimate (tests/bayes_ref.py) and of the constructed families
(tests/bayes_cases.py) the GPU stage tests judge the estimate kernels with.

The module is tied to the oracle twice (the committed 40 x 28 fixture with the fixture's masks; a frame where every main pixel of the window
is similar, which the oracle can evaluate itself with a threshold nothing exceeds), and the families are tied to the float32 calibrator: an
item whose plain-fp32 evaluation is more than 1e-2 from float64 is meaningless in fp32 for anybody and is not judged numerically on the GPU --
at most 5 % of the full-estimate items of a family may be like that.  The cap is met by changing the INPUTS of a family, never the cap."""
import os

import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br
import oracle_lib as ol

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

EXCLUDE_ABOVE = 1e-2   # calibrator error beyond which an item is checked for count and finiteness only
EXCLUSION_CAP = 0.05   # ... and the share of a family's full-estimate items that may be


def _pixcov(cov, ns):
    out = np.empty_like(cov)
    H, W, _ = cov.shape
    ol.oracle().bcdo_pixel_cov_from_sample_cov(ol._fp(cov), ol._fp(ns), W, H, ol._fp(out))
    return out


def _all_main(H, W, w):
    st = np.zeros((H, W), np.uint8)
    st[w:H - w, w:W - w] = 1
    return st


def test_mask_words_round_trip():
    rng = np.random.default_rng(0)
    for b in (3, 6, 12):
        side = 2 * b + 1
        k = np.sort(rng.permutation(side * side)[:rng.integers(1, side * side)])
        pos = np.stack([40 + k // side - b, 50 + k % side - b], 1)
        words = br.encode_members(pos, 40, 50, b)
        assert words.size == (side * side + 31) // 32
        assert np.array_equal(br.decode_members(words, 40, 50, b), pos)          # window order
        assert br.popcount(words.reshape(1, 1, -1))[0, 0] == len(k)


def test_fixture_masks_reproduce_the_fixture_image():
    f = np.load(os.path.join(G, "core_regression.npz"))
    H, W, _ = f["col"].shape
    acc, cnt, items = br.accumulate(f["col"], _pixcov(f["cov"], f["ns"]), f["mask"], f["cnt"], _all_main(H, W, 1), 1, 6, 1e-8, keep_stages=False)
    n = np.array([i["n"] for i in items]).reshape(H - 2, W - 2)
    seen = f["nsim"][1:H - 1, 1:W - 1] >= 0                              # (the fixture's diagnostics are those of its -m 1 run: visited pixels only)
    assert seen.any() and np.array_equal(n[seen], f["nsim"][1:H - 1, 1:W - 1][seen]) and np.array_equal(n[seen] < 28, f["fallback"][1:H - 1, 1:W - 1][seen] > 0)
    assert (n < 28).any() and (n >= 28).any()                            # both paths
    got, want = acc / cnt[..., None], f["out_m0"]
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-5, err


@pytest.mark.parametrize("W,H,b", [(40, 30, 6), (33, 21, 3)])
def test_every_window_pixel_similar_agrees_with_the_oracle(W, H, b):
    """the one family of constructed sets the oracle can evaluate too: a threshold nothing exceeds on a frame with finite histogram distances"""
    col, ns, hist, cov, _ = ol.synth_inputs(W, H, 16, 21, 0.3, 0.0)
    want, (proc, fb, nsim) = ol.denoise_mono(col, ns, hist, cov, ol.params(tau=1e30, b=b, m=0), want_diag=True)
    sets = {(l, c): bc.window(l, c, H, W, 1, b) for l in range(1, H - 1) for c in range(1, W - 1)}
    case = bc.Case("all similar", col, _pixcov(cov, ns), sets, b=b, dense=True)
    assert np.array_equal(case.nsim[1:H - 1, 1:W - 1], nsim[1:H - 1, 1:W - 1])      # finite distances everywhere: the oracle's sets ARE the windows
    assert np.array_equal(case.mask, ol.similarity_masks(ns, hist, 1, b, 1e30)[0])
    acc, cnt, _ = br.accumulate(*case.args(), keep_stages=False)
    got = acc / cnt[..., None]
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-5, err


def test_calibrator_runs_in_float32_and_non_finite_members_poison_only_their_item():
    case = bc.FAMILIES["non-finite"]()[0]
    s64, c64, it64 = br.accumulate(*case.args())
    s32, c32, it32 = br.accumulate(*case.args(), dtype=np.float32)
    assert s32.dtype == np.float32 and all(v.dtype == np.float32 for i in it32 for k, v in i.items() if isinstance(v, np.ndarray) and k != "members")
    assert np.array_equal(c64, c32) and np.array_equal(np.isfinite(s64), np.isfinite(s32))
    bad = [i for i in it64 if not np.isfinite(s64[br.touched(i, 1)]).all()]
    assert len(bad) == len(it64[::3])                                    # the poisoned items and no other
    for i in bad:
        if i["n"] >= 28:                                                 # a full estimate is NaN throughout, a fallback mean in one entry
            assert np.isnan(s64[br.touched(i, 1)]).all()
        else:
            assert np.isnan(s64[br.touched(i, 1)]).sum() == 1


@pytest.mark.parametrize("what", ["nan covariance", "inf covariance", "nan colour"])
def test_non_finite_input_poisons_the_same_pixels_as_in_the_oracle(what):
    """bayes_ref._spectral does not hand a matrix with a non-finite entry to LAPACK (which may raise or return anything) but returns NaNs throughout,
    as an iterative solver leaves them -- and the estimate kernels were made to agree with that.  This ties the rule to the oracle: with every window
    pixel similar and one poisoned input value, the non-finite pixels of the oracle's frame are exactly those of the module's."""
    W, H, b = 40, 30, 6
    col, ns, hist, cov, _ = ol.synth_inputs(W, H, 16, 21, 0.3, 0.0)
    col, cov = col.copy(), cov.copy()
    if what == "nan colour":
        col[14, 19, 1] = np.nan
    else:
        cov[14, 19, 3] = np.nan if what == "nan covariance" else np.inf
    want = ol.denoise_mono(col, ns, hist, cov, ol.params(tau=1e30, b=b, m=0))
    sets = {(l, c): bc.window(l, c, H, W, 1, b) for l in range(1, H - 1) for c in range(1, W - 1)}
    case = bc.Case("all similar, one poisoned value", col, _pixcov(cov, ns), sets, b=b, dense=True)
    acc, cnt, _ = br.accumulate(*case.args(), keep_stages=False)
    got = acc / cnt[..., None]
    assert 0 < np.isnan(want).sum() < want.size
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    assert np.max(np.abs(got[ok] - want[ok])) / np.max(np.abs(want[ok])) < 1e-5


@pytest.mark.parametrize("family", sorted(bc.FAMILIES))
def test_family_is_well_formed_and_the_calibrator_stays_inside_the_exclusion_cap(family):
    cases = bc.FAMILIES[family]()
    isolated, full, excluded, worst = 0, 0, 0, 0.0
    for case in cases:
        assert np.array_equal(case.nsim, br.popcount(case.mask))
        s64, c64, it64 = br.accumulate(*case.args(), keep_stages=False)
        s32, c32, _ = br.accumulate(*case.args(), dtype=np.float32, keep_stages=False)
        assert np.array_equal(c64, c32)
        if case.dense:
            assert len(it64) == (case.col.shape[0] - 2 * case.w) * (case.col.shape[1] - 2 * case.w)
            continue
        isolated += len(it64)
        owners = np.zeros(c64.shape, np.int32)
        for i in it64:
            owners[br.touched(i, case.w)] += 1
        assert owners.max() == 1 and np.array_equal(owners > 0, c64 > 0)  # isolation: no output pixel is written by two items
        if not case.judged:
            continue
        K1 = 3 * (2 * case.w + 1) ** 2 + 1
        e32 = np.array([br.item_error(s32, s64, i, case.w) for i in it64 if i["n"] >= K1])
        full += len(e32)
        excluded += int((e32 > EXCLUDE_ABOVE).sum())
        worst = max([worst] + list(e32[e32 <= EXCLUDE_ABOVE]))
    assert isolated >= 24, isolated
    assert excluded <= EXCLUSION_CAP * full, (family, excluded, full)
    print("%s: %d isolated items, %d full estimates, %d excluded, max e_32 %.2e" % (family, isolated, full, excluded, worst))


def test_call_sequence_cases_have_the_item_counts_the_launch_logic_needs():
    calls = bc.call_sequence()
    assert [int((c.state == 1).sum()) for c in calls] == [600, 600, 3000, 10]
    assert all((c.nsim[c.state == 1] >= 28).all() for c in calls)
