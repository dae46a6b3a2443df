"""CPU tests that hold the motion reference (tests/motion_ref.py) and the constructed inputs (tests/motion_cases.py) to their claims, without a GPU.

  * a zero field: `warp` is the identity bit for bit, every pixel is valid, `gate` changes nothing;
  * the rounding and validity rules on the named fields: ties to even of both parities, +-0.0, -0.49999997, NaN, +-inf, +-2^24, one pixel outside each border;
  * the validity pyramid on odd and even sizes, pvalid and the gate on a single invalid pixel at a patch corner;
  * the translated case: with its field the cross masks are those of the unshifted realisation wherever pvalid holds, and the sum of |S_f| over the main
    pixels is strictly greater than with a zero field;
  * conditions on the inputs of the GPU whole-call tests, checked on the reference alone: every configuration has, at every scale, invalid pixels, at least
    one main pixel whose cross set loses a member to the gate that the ungated reference keeps, and both fallback and full-estimate pixels; the all-valid
    fields have no invalid pixel."""
import numpy as np
import pytest

import marking_ref as mr
import motion_cases as mc
import motion_ref as mo
import temporal_ref as tr

F = np.float32


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


@pytest.mark.parametrize("W,H", [(1, 1), (17, 5), (33, 21)])
def test_zero_field_is_the_identity_and_the_gate_changes_nothing(W, H):
    fr = mc.stage_frame(W, H, 24)
    for mv in (mc.field("zero", W, H), None):
        out, valid = mo.warp(fr, mv)
        assert valid.all() and all(same_bits(a, b) for a, b in zip(out, fr))
    if W < 3:
        return
    m, n = tr.cross_masks(fr[2], fr[1], *mc.stage_frame(W, H, 24, seed=9)[2:0:-1], 1, 6, F(2.0))
    assert n.sum() > 0
    mg, ng = mo.gate(m, n, np.ones((H, W), np.uint8), 1, 6)
    assert np.array_equal(mg, m) and np.array_equal(ng, n)


def test_rounding_to_nearest_even_and_the_validity_rules():
    W, H = 9, 7
    mv = np.zeros((H, W, 2), F)
    row = [(0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (-0.0, 0), (-0.49999997, 0), (0.49999997, 0)]
    mv[3, 4, 0] = 0.0
    for i, (dx, want) in enumerate(row):
        one = mv.copy()
        one[3, 4, 0] = dx
        ok, sl, sc = mo.sources(one, H, W)
        assert ok[3, 4] and (sl[3, 4], sc[3, 4]) == (3, 4 + want), (dx, sc[3, 4])
        one[3, 4] = (0, dx)
        ok, sl, sc = mo.sources(one, H, W)
        assert ok[3, 4] and (sl[3, 4], sc[3, 4]) == (3 + want, 4)
    big = F(2.0 ** 24)
    for bad in (np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, F(0)), 5.0, -5.0):
        for comp in (0, 1):
            one = mv.copy()
            one[3, 4, comp] = bad
            ok, _, _ = mo.sources(one, H, W)
            assert not ok[3, 4] and ok.sum() == H * W - 1, bad
    one = mv.copy()
    one[3, 4] = (4, 3)                                                # the last column and line: inside
    assert mo.sources(one, H, W)[0].all()
    sp = mc.field("special", 65, 7)
    ok, _, _ = mo.sources(sp, 7, 65)
    assert not ok[:, 0].any() and not ok[:, -1].any() and not ok[0].any() and not ok[-1].any()
    assert ok[2:-2, 1].all() and ok[2:-2, -2].all() and ok[1, 1:-1].all() and ok[-2, 1:-1].all()      # exactly onto the border
    assert 0 < ok[2:-2, 2:-2].sum() < ok[2:-2, 2:-2].size
    ck = mo.sources(mc.field("checker", 17, 5), 5, 17)[0]
    l, c = np.meshgrid(np.arange(5), np.arange(17), indexing="ij")
    assert np.array_equal(ck, (l + c) % 2 == 0)
    ties = mo.sources(mc.field("ties", 65, 7), 7, 65)[0]
    assert 0 < ties.sum() < ties.size
    rnd = mc.field("random", 65, 7)
    assert mo.sources(rnd, 7, 65)[0].all() and len(np.unique(rnd)) > 20


def test_invalid_pixels_are_positive_zero_and_valid_ones_are_gathered():
    W, H = 17, 5
    fr = mc.stage_frame(W, H, 12)
    mv = mc.field("special", W, H)
    out, valid = mo.warp(fr, mv)
    ok, sl, sc = mo.sources(mv, H, W)
    assert 0 < ok.sum() < ok.size
    for a, g in zip(fr, out):
        assert (g[~ok].view(np.uint32) == 0).all()
        assert same_bits(g[ok], a[sl[ok], sc[ok]])


@pytest.mark.parametrize("W,H", [(2, 2), (5, 4), (7, 7), (16, 11), (33, 21)])
def test_validity_pyramid_down_to_one_pixel(W, H):
    rng = np.random.default_rng(W * 100 + H)
    v = (rng.random((H, W)) < 0.8).astype(np.uint8)
    levels = mo.valid_levels(v, 6)
    for fine, coarse in zip(levels, levels[1:]):
        h, w = fine.shape
        assert coarse.shape == (h // 2, w // 2)
        for l in range(h // 2):
            for c in range(w // 2):
                assert coarse[l, c] == fine[2 * l:2 * l + 2, 2 * c:2 * c + 2].all()
    assert levels[-1].size <= 1 or min(levels[-1].shape) >= 1
    ones = mo.valid_levels(np.ones((H, W), np.uint8), 3)
    assert all(x.all() for x in ones)


def test_one_invalid_pixel_at_a_patch_corner_removes_exactly_the_candidates_around_it():
    W, H, w, b = 20, 16, 1, 6
    valid = mo.sources(mc.field("corner", W, H), H, W)[0].astype(np.uint8)
    assert valid.sum() == W * H - 1 and not valid[3, 3]
    pv = mo.pvalid(valid, w)
    want = np.zeros((H, W), bool)
    want[w:H - w, w:W - w] = True
    want[2:5, 2:5] = False
    assert np.array_equal(pv, want)
    words = ((2 * b + 1) ** 2 + 31) // 32
    ones = np.full((H, W, words), 0xffffffff, np.uint32)
    m, n = mo.gate(ones, np.zeros((H, W), np.int32), valid, w, b)
    bits = np.unpackbits(m.view(np.uint8).reshape(H, W, -1), axis=-1, bitorder="little")[:, :, :(2 * b + 1) ** 2].astype(bool)
    for (l, c) in ((1, 1), (4, 4), (8, 9), (H - 2, W - 2), (10, 3)):
        for k, (dl, dc) in enumerate(tr.window_offsets(b)):
            ql, qc = l + dl, c + dc
            assert bits[l, c, k] == (w <= ql <= H - 1 - w and w <= qc <= W - 1 - w and bool(pv[ql, qc])), (l, c, dl, dc)
        assert n[l, c] == bits[l, c].sum()
    assert not m[0].any() and not m[:, 0].any() and n[0].sum() == 0 and n[:, -1].sum() == 0      # pixels that are not main pixels


@pytest.mark.parametrize("W,H", mc.SIZES)
def test_translated_case_finds_the_unshifted_realisation_s_members(W, H):
    w, b, tau = 1, 6, F(1.0)
    frame, nb, mv = mc.translated(W, H)
    plain_nb = mc.unshifted(W, H)
    (col, ns, hist, cov), valid = mo.warp([nb[0], nb[1], nb[2], nb[3]], mv)
    pv = mo.pvalid(valid, w)
    assert 0 < pv.sum() < (W - 2) * (H - 2)
    assert same_bits(hist[valid.astype(bool)], plain_nb[2][valid.astype(bool)])          # the warped neighbour IS the unshifted realisation where it is valid
    m_w, n_w = mo.gate(*tr.cross_masks(frame[2], frame[1], hist, ns, w, b, tau), valid, w, b)
    m_u, n_u = mo.gate(*tr.cross_masks(frame[2], frame[1], plain_nb[2], plain_nb[1], w, b, tau), valid, w, b)
    assert np.array_equal(m_w, m_u) and np.array_equal(n_w, n_u)
    m_0, n_0 = tr.cross_masks(frame[2], frame[1], nb[2], nb[1], w, b, tau)               # a zero field: the neighbour where it lies
    main = (slice(w, H - w), slice(w, W - w))
    print("translated %dx%d: sum |S_f| with the field %d, with a zero field %d" % (W, H, n_w[main].sum(), n_0[main].sum()))
    assert n_w[main].sum() > n_0[main].sum()


@pytest.mark.parametrize("W,H,S,nf", mc.CONFIGS)
def test_whole_call_configurations_exercise_the_gate_at_every_scale(W, H, S, nf):
    fr = mc.frames_of(W, H)
    orders, draws = mc.orders_draws(W, H, S)
    fields = [mc.holes(W, H, f) for f in range(nf)]
    sels = mo.select_multiscale_motion(fr[0], fr[1:1 + nf], fields, S, 1, 6, F(1.0), orders, draws)
    _, valids = mo.warped_levels(fr[0], fr[1:1 + nf], fields, S)
    for s, sel in enumerate(sels):
        st = mo.selection_stats(sel, 1)
        lost = sum(int((x > 0).sum()) for x in sel["lost"])
        inval = [int((v == 0).sum()) for v in valids[s]]
        print("%dx%d S=%d F=%d scale %d: invalid %s, pixels that lose a member %d, %s" % (W, H, S, nf, s, inval, lost, st))
        assert all(0 < i < v.size for i, v in zip(inval, valids[s]))
        assert lost >= 1
        assert 0 < st["fallback"] < st["processed"]
    for f in range(nf):
        assert mo.sources(mc.all_valid(W, H, f), H, W)[0].all() and len(np.unique(mc.all_valid(W, H, f))) > 5
