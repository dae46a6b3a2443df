"""CPU tests that hold the NumPy reference of the cross-frame feature gate (tests/guide_cross_ref.py) and the constructed cases (tests/guide_cross_cases.py)
to their claims, without a GPU ("Features"):
  * a neighbour equal to the frame gives guide_ref.masks bit for bit;
  * a neighbour whose features are the frame's rolled by (2, -3) has bit delta = (2, -3) set on every main pixel whose partner is a main pixel;
  * inf against inf is skipped, inf against a finite value is dissimilar, a NaN in the only counted channel over a pixel's patch empties its masks, delta = 0
    included;
  * two deliberately wrong mutants (second operand from the frame; planes filed under -delta) are caught;
  * the warp of the features is motion_ref's gather; the gate is a pure AND; the benefit scene gives the reference a guided / unguided ratio of at most 0.9."""
import numpy as np
import pytest

import guide_cross_cases as gc
import guide_cross_ref as gx
import guide_ref as gr
import motion_cases as mc
import motion_ref as mo
import similarity_ref as sr

W_, B_ = 1, 6
SIDE = 2 * B_ + 1


def bit(mask, dl, dc, b=B_):
    k = (dl + b) * (2 * b + 1) + (dc + b)
    return (np.ascontiguousarray(mask).view(np.uint32)[..., k >> 5] >> np.uint32(k & 31)) & 1


def masks_of(c, w=W_, b=B_, **mutant):
    return gx.cross_masks(c["f"], c["v"], c["f_nb"], c["v_nb"], w, b, c["floors"], c["tau"], **mutant)


@pytest.mark.parametrize("F,var,w,b", [(3, True, 1, 6), (1, False, 1, 6), (8, True, 2, 3), (2, False, 0, 2)])
def test_a_neighbour_equal_to_the_frame_gives_the_in_frame_masks(F, var, w, b):
    c = gc.identity(41, 13, F, var)
    m, n = masks_of(c, w, b)
    m0, n0 = gr.masks(c["f"], c["v"], w, b, c["floors"], c["tau"])
    assert np.array_equal(m, m0.view(np.uint32)) and np.array_equal(n, n0)
    assert 0 < n[w:-w or None, w:-w or None].min() and n.max() > 1      # (delta = 0 everywhere, more somewhere)


def test_rolled_features_set_the_bit_of_the_roll():
    W, H = 40, 14
    c = gc.rolled(W, H)
    m, n = masks_of(c)
    dl, dc = gc.ROLL
    want = np.zeros((H, W), np.uint32)
    want[max(1, 1 - dl):min(H - 1, H - 1 - dl), max(1, 1 - dc):min(W - 1, W - 1 - dc)] = 1      # main pixels whose partner is a main pixel
    assert want.sum() > 0 and np.array_equal(bit(m, dl, dc), want)
    assert np.array_equal(n, want.astype(np.int32))                      # random features: no other pair is alike


def test_special_values():
    W, H = 24, 12
    c = gc.special(W, H)
    T, C, written = gx.cross_planes(c["f"], c["v"], c["f_nb"], c["v_nb"], B_, c["floors"])
    k0 = B_ * SIDE + B_
    assert (C[k0][:, W - 6:] == 0).all() and (T[k0][:, W - 6:] == 0).all()            # inf against inf: the term is NaN and skipped
    assert (C[k0][:, W - 9:W - 6] == 1).all() and np.isinf(T[k0][:, W - 9:W - 6]).all()   # finite against inf: counted, infinite
    assert (C <= 1).all()                                                # channel 1 (floor 0, no variances) never counts
    m, n = masks_of(c)
    assert bit(m, 0, 0)[1:-1, 1:W - 10].sum() == (H - 2) * (W - 11) - 1   # away from the background delta = 0 is similar, but for ...
    l, cc = gc.NAN_AT
    assert n[l, cc] == 0 and not m[l, cc].any()                          # ... the pixel whose whole patch is NaN: 0 / 0, delta = 0 included
    assert n[l, cc + 1] > 0                                              # (a patch with some NaN pixels still counts the others)
    assert (n[:, W - 5:] == 0).all()                                     # background patches: nothing counts, 0 / 0
    assert (bit(m, 0, 0)[1:-1, W - 10:W - 6] == 0).all()                 # a patch that holds finite-against-inf: infinite distance


def test_mutants_are_caught():
    c = gc.rolled(40, 14)
    good, _ = masks_of(c)
    dl, dc = gc.ROLL
    for mutant in (dict(second="frame"), dict(flip=True)):
        bad, _ = masks_of(c, **mutant)
        assert not np.array_equal(bad, good), mutant
        assert bit(bad, dl, dc).sum() == 0, mutant                       # the claim of the rolled case fails
    s = gc.stage_images(70, 9, 3, True)
    assert not np.array_equal(masks_of(s, flip=True)[0], masks_of(s)[0])
    assert not np.array_equal(masks_of(s, second="frame")[0], masks_of(s)[0])


def test_constructed_stage_cases_have_set_and_cleared_bits():
    for (W, H, F, var, w, b) in gc.STAGE_GEOMETRIES:
        c = gc.stage_images(W, H, F, var)
        m, n = masks_of(c, w, b)
        main = n[w:H - w, w:W - w]
        window = sr.window_valid(W, H, w, b).sum(-1)[w:H - w, w:W - w]     # the partners a main pixel has
        assert main.max() >= 2 and (main < window).any(), (W, H, F, var, w, b)
        assert (n[:w] == 0).all() and (n[:, :w] == 0).all()


def test_feature_warp_is_the_gather_of_the_other_images():
    W, H = 17, 9
    f, v = mc.bit_patterns((H, W, 5), 3), mc.bit_patterns((H, W, 5), 4)
    mv = mc.field("special", W, H)
    wf, wv, valid = gx.warp_features(f, v, mv)
    (col,), valid2 = mo.warp([f], mv)
    assert np.array_equal(wf.view(np.uint32), col.view(np.uint32)) and np.array_equal(valid, valid2)
    assert 0 < valid.sum() < valid.size
    assert (wf.view(np.uint32)[valid == 0] == 0).all() and (wv.view(np.uint32)[valid == 0] == 0).all()


def test_gate_is_a_pure_and():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 2 ** 32, (5, 7, 6), dtype=np.uint64).astype(np.uint32)
    g = rng.integers(0, 2 ** 32, (5, 7, 6), dtype=np.uint64).astype(np.uint32)
    m, n = gx.gate(a, g)
    assert np.array_equal(m, a & g) and np.array_equal(n, gr.popcount(a & g))


@pytest.mark.parametrize("cfg,motion", [(gc.CONFIGS[1], False), (gc.CONFIGS[3], False), (gc.MOTION_CONFIGS[0], True)])
def test_whole_call_configurations_are_gated_and_have_both_kinds_of_pixels(cfg, motion):
    """the features of the whole-call cases remove members that the histograms accept (else the frame tests would not see the gate), and the finest scale keeps
    full estimates beside fallback pixels"""
    import motion_ref as mo
    W, H, S, N, L, var = cfg
    _, stats = gc.reference(W, H, S, N, L, var, motion)
    fr = [(lay[0][0], ns, hist, lay[0][1]) for ns, hist, lay in gc.frames_of(W, H)[:1 + N]]
    orders, draws = gc.orders_draws(W, H, S)
    plain = mo.select_multiscale_motion(fr[0], fr[1:], gc.fields_of(W, H, N) if motion else [None] * N, S, 1, 6, 1.0, orders, draws)
    for s in range(S):
        assert stats[s] != mo.selection_stats(plain[s], 1), s
        assert stats[s]["processed"] > 0 and stats[s]["similar_total"] > 0
    assert 0 < stats[0]["fallback"] < stats[0]["processed"]


def test_benefit_scene_separates_the_reference():
    guided, plain = gc.benefit_reference()
    print("benefit scene, NumPy composition: guided RMSE %.5f, unguided %.5f, ratio %.3f" % (guided, plain, guided / plain))
    assert guided / plain <= 0.9
