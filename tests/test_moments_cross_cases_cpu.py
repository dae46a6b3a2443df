"""No GPU: the NumPy restatement of the cross-frame moment selection (tests/moments_cross_ref.py) and the constructed cases (tests/moments_cross_cases.py) held
to their claims, so that the GPU tests compare against something that is itself checked ("Moments").

  * a neighbour that IS the frame gives moments_ref.masks (the in-frame selection) bit for bit;
  * on inputs with no NaN term and one common floor the masks are guide_cross_ref.cross_masks with F = 3 (the feature term differs only in skipping NaN terms);
  * a rolled neighbour: the bit of the roll's displacement is set wherever both patches are main;
  * every special pixel does what the definition says;
  * every stage case is neither full nor empty: between 5 % and 95 % of the in-window main pairs are similar at tau = 1 and some |S_j| is at least 2.
    noisy seed 1 against seed 2 at tau = 1, eps = 1e-4, w = 1: 33.5 % (70x13, b = 6), 27.4 % (40x28, b = 6), 39.2 % (65x9, b = 2)."""
import numpy as np
import pytest

import guide_cross_ref as gx
import moments_cross_cases as xc
import moments_cross_ref as mx
import moments_ref as mr

F = np.float32
SIZES = [(70, 13, 1, 6), (40, 28, 1, 6), (65, 9, 1, 2)]


def bit(mask, k):
    return (mask[..., k // 32] >> np.uint32(k % 32)) & np.uint32(1)


@pytest.mark.parametrize("W,H,w,b", SIZES + [(30, 11, 2, 3)])
@pytest.mark.parametrize("eps", xc.FLOORS)
def test_identity_is_the_in_frame_selection(W, H, w, b, eps):
    c = xc.identity(W, H, w, b, eps)
    for tau in c["taus"]:
        m, n = mx.masks_from(c["D"], c["valid"], tau)
        wm, wn = mr.masks(c["m0"], c["P0"], w, b, tau, eps)
        assert np.array_equal(m, np.ascontiguousarray(wm).view(np.uint32)) and np.array_equal(n, wn)
        assert n.max() >= 2


@pytest.mark.parametrize("W,H,w,b", SIZES)
def test_without_nan_terms_it_is_the_feature_term_with_three_channels(W, H, w, b):
    eps = 1e-4
    c = xc.stage_case(W, H, w, b, eps)
    for tau in c["taus"]:
        m, n = mx.masks_from(c["D"], c["valid"], tau)
        gm, gn = gx.cross_masks(c["m0"], c["P0"][..., :3], c["mj"], c["Pj"][..., :3], w, b, [eps] * 3, tau)
        assert np.array_equal(m, gm) and np.array_equal(n, gn)


@pytest.mark.parametrize("W,H,w,b", SIZES[:2] + [(65, 9, 1, 3), (30, 11, 2, 4)])       # (the roll lies inside the window)
def test_rolled_neighbour_sets_the_bit_of_the_roll(W, H, w, b):
    c = xc.rolled(W, H, w, b, 1e-4)
    m, _ = mx.masks_from(c["D"], c["valid"], 1.0)
    dl, dc = xc.ROLL
    k = (dl + b) * (2 * b + 1) + (dc + b)
    both = np.zeros((H, W), bool)
    both[max(w, w - dl):min(H - w, H - w - dl), max(w, w - dc):min(W - w, W - w - dc)] = True
    assert both.sum() > 0
    assert np.array_equal(bit(m, k).astype(bool), both)                    # set wherever both patches are main, and nowhere else
    assert np.all(c["D"][k][both] == 0)                                    # every term is 0 / q, q > 0


def test_special_pixels_do_what_the_definition_says():
    W, H, w, b = 70, 13, 1, 6
    side = 2 * b + 1
    centre = b * side + b
    for eps in xc.FLOORS:
        c = xc.special(W, H, w, b, eps)
        T, C, written = mx.planes(c["m0"], c["P0"], c["mj"], c["Pj"], b, eps)
        l, col = xc.NAN_COV_FRAME
        assert np.all(C[:, l, col][written[:, l, col]] == 0) and np.all(T[:, l, col][written[:, l, col]] == 0)   # a NaN q is not counted, whatever the partner
        l, col = xc.NAN_COV_NB
        assert C[centre, l, col] == 0                                      # ... read from the neighbour too
        # an infinite or NaN mean: the term is counted and poisons every patch that holds the pixel
        for (l, col), frame_side in ((xc.INF_MEAN_FRAME, True), (xc.NAN_MEAN_FRAME, True), (xc.INF_MEAN_NB, False), (xc.NAN_MEAN_NB, False)):
            assert C[centre, l, col] == 3 and not np.isfinite(T[centre, l, col])
            m, n = mx.masks_from(c["D"], c["valid"], np.float32(3.0e38))
            if frame_side:
                assert np.all(n[l - 1:l + 2, col - 1:col + 2] == 0)        # every main pixel whose patch holds it has an empty cross mask
            else:
                for k, (dl, dc) in enumerate(mx.offsets(b)):               # every bit that points at a patch holding it is clear
                    ls = slice(max(w, l - 1 - dl), max(0, min(H - w, l + 2 - dl)))
                    cs = slice(max(w, col - 1 - dc), max(0, min(W - w, col + 2 - dc)))
                    assert not bit(m, k)[ls, cs].any()
        # the zero-variance block, patch inside the block against patch inside the block
        inner_l, inner_c = slice(6, 9), slice(21, 26)
        for k, (dl, dc) in enumerate(mx.offsets(b)):
            if abs(dl) > 2 or abs(dc) > 4:
                continue
            for l in range(6, 9):
                for col in range(21, 26):
                    if not (6 <= l + dl < 9 and 21 <= col + dc < 26):
                        continue
                    d = c["D"][k, l, col]
                    assert (np.isnan(d) if eps == 0.0 else d == 0), (eps, k, l, col, d)
        m, _ = mx.masks_from(c["D"], c["valid"], 1.0)
        assert bool(bit(m, centre)[7, 23]) == (eps > 0)                    # 0 / 0 is never similar; distance 0 is


@pytest.mark.parametrize("W,H,w,b", xc.STAGE_FUSED + xc.STAGE_PLANES_ONLY)
@pytest.mark.parametrize("eps", xc.FLOORS)
def test_stage_cases_are_neither_full_nor_empty(W, H, w, b, eps):
    c = xc.stage_case(W, H, w, b, eps)
    if not c["valid"].any():
        pytest.fail("no main pixel pair in %dx%d at w = %d" % (W, H, w))
    share, largest = xc.similar_share(c)
    assert 0.05 <= share <= 0.95 and largest >= 2, (share, largest)


def test_the_shares_the_module_quotes():
    got = [round(100 * xc.similar_share(xc.stage_case(W, H, w, b, 1e-4))[0], 1) for W, H, w, b in SIZES]
    print("similar shares at tau = 1, eps = 1e-4:", got)
    assert got == [33.5, 27.4, 39.2]


def test_thresholds_sit_on_a_distance_that_occurs():
    c = xc.stage_case(70, 13, 1, 6, 1e-4)
    one, at, below = c["taus"]
    n_at, n_below = (mx.masks_from(c["D"], c["valid"], t)[1].sum() for t in (at, below))
    assert n_at > n_below                                                  # the pair AT the threshold is similar, and is lost one float below
