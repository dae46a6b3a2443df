"""CPU tests that hold tests/guide_ref.py -- the NumPy float32 restatement of the feature gate that the GPU stage test compares with bit for
bit -- to its claims, on the constructed frames of tests/guide_cases.py.  No GPU needed.
  * T / C are bitwise symmetric, and the vectorised planes are those of a scalar restatement of the definition on sampled pixel pairs;
  * F = 3 with a common floor is moments_ref.planes on the same numbers, bit for bit;
  * NaN terms are skipped (NaN features, inf against inf, NaN variances), infinite terms are counted, a channel with floor 0 and no variance is off;
  * every stage case leaves at least 1 % of the valid pairs set and at least 1 % clear at tau_g = 1 (a condition on the inputs, not a tolerance);
  * a pair AT the threshold is in, one ulp below it is out;
  * the pyramid rule: features averaged, variances averaged and multiplied by 0.25;
  * the noise-free frame of the effect test: whole-patch distances across the feature edge are >= 2."""
import numpy as np
import pytest

import guide_cases as gc
import guide_ref as gr
import moments_cases as mc
import moments_ref as mr

F32 = np.float32
W, H = 70, 13


def scalar_pair(f, v, eps, x, y):
    """the definition, one float32 operation after the other, for pixels x and y (line, column)"""
    s, n = F32(0), 0
    with np.errstate(all="ignore"):
        for k in range(f.shape[2]):
            d = F32(f[x][k]) - F32(f[y][k])
            q = (F32(F32(v[x][k]) + F32(v[y][k])) if v is not None else F32(0)) + F32(eps[k])
            if q > 0:
                t = F32(F32(d * d) / q)
                if t == t:
                    s = F32(s + t)
                    n += 1
    return s, n


def bits(a):
    return np.asarray(a, F32).view(np.int32)


@pytest.mark.parametrize("with_var", [True, False])
@pytest.mark.parametrize("F", [1, 3, 8])
def test_planes_are_the_definition_and_bitwise_symmetric(F, with_var):
    b = 6
    c = gc.stage_case(W, H, 1, b, F, with_var)
    f, v, fl = c["f"], c["v"], c["floors"]
    T, C, written = gr.planes(f, v, b, fl)
    assert written.any() and not written.all()
    rng = np.random.default_rng(3)
    special = [(2, 5), (H - 3, W - 9), (7, 23), (5, 20), (9, 26), (3, 33)]
    pixels = special + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(120)]
    checked = 0
    for x in pixels:
        for dl, dc in mr.deltas(b)[::5] + [(0, 0), (0, 1), (1, 0), (b, -b), (b, b)]:
            y = (x[0] + dl, x[1] + dc)
            i = mr.delta_index(dl, dc, b)
            if not (0 <= y[0] < H and 0 <= y[1] < W):
                assert not written[i][x]
                continue
            assert written[i][x]
            s_xy, n_xy = scalar_pair(f, v, fl, x, y)
            s_yx, n_yx = scalar_pair(f, v, fl, y, x)
            assert bits(s_xy) == bits(s_yx) and n_xy == n_yx                      # T_delta(x) == T_-delta(x + delta), bit for bit
            assert bits(T[i][x]) == bits(s_xy) and C[i][x] == n_xy, (x, dl, dc)
            checked += 1
    assert checked > 1500


@pytest.mark.parametrize("eps", mc.FLOORS + [0.01])
def test_three_channels_with_a_common_floor_are_the_moment_planes(eps):
    """on the same numbers: the colours of moments_cases.noisy as features, the xx, yy, zz entries of its per-pixel covariances as variances"""
    b = 6
    col, cov, ns, _ = mc.noisy(W, H, seed=5)
    P = mc.pixel_cov(cov, ns)
    T, C, written = gr.planes(col, P[..., :3], b, [eps] * 3)
    Tm, Cm, wm = mr.planes(col, P, b, eps)
    assert np.array_equal(written, wm) and np.array_equal(C, Cm) and np.array_equal(bits(T), bits(Tm))
    assert (C[written] == 3).all() or eps == 0.0
    # ... and with [v, 0, 0, 0]-style zero variances: no variance image at all is the moment planes of zero covariances
    if eps > 0:
        T0, C0, _ = gr.planes(col, None, b, [eps] * 3)
        Tz, Cz, _ = mr.planes(col, np.zeros_like(P), b, eps)
        assert np.array_equal(C0, Cz) and np.array_equal(bits(T0), bits(Tz))


def test_nan_terms_are_skipped_and_infinite_terms_are_counted():
    b, w, F = 3, 1, 3
    for with_var in (True, False):
        c = gc.stage_case(W, H, w, b, F, with_var)
        f, v, fl = c["f"], c["v"], c["floors"]
        T, C, written = gr.planes(f, v, b, fl)
        D, valid = c["D"], c["valid"]
        full = F if with_var else F - 1                     # (without variances channel 1 has floor 0: switched off)
        i01 = mr.delta_index(0, 1, b)
        # a NaN feature: its channel is skipped in every pair of the pixel, the others count
        x = (2, 5)
        for i in range(len(mr.deltas(b))):
            if written[i][x]:
                assert C[i][x] == full - 1 and np.isfinite(T[i][x])
        # inside the block inf - inf is NaN: skipped; on its rim the term is +inf: counted
        assert C[i01][7, 23] == full - 1 and np.isfinite(T[i01][7, 23])
        assert C[i01][7, 26] == full and np.isposinf(T[i01][7, 26])                 # (7, 26) inside, (7, 27) outside
        assert C[0][7, 23] == full - 1 and T[0][7, 23] == 0                          # the pixel with itself
        # one infinite pixel beside finite ones: every pair with a neighbour is +inf and counted, with itself NaN and skipped
        assert np.isposinf(T[i01][3, 33]) and C[i01][3, 33] == full and np.isposinf(T[i01][3, 32])
        assert C[0][3, 33] == full - 1
        # a patch deep inside the block is compared through its other channels: similar to itself
        centre = b * (2 * b + 1) + b
        assert D[centre][7, 23] == 0
        # a patch that holds the lone infinite pixel is infinitely far from every other patch, and at distance 0 from itself
        d = D[:, 3, 33][valid[:, 3, 33]]
        assert np.isposinf(d).sum() == d.size - 1 and D[centre][3, 33] == 0
        if with_var:
            y = (H - 3, W - 9)                              # a NaN variance: q is NaN, the channel is not counted
            for i in range(len(mr.deltas(b))):
                if written[i][y]:
                    assert C[i][y] == full - 1
        else:
            # the switched-off channel changes nothing: the planes are those of the other channels alone
            keep = [k for k in range(F) if k != 1]
            T2, C2, _ = gr.planes(f[..., keep], None, b, fl[keep])
            assert np.array_equal(C, C2) and np.array_equal(bits(T), bits(T2))


ALL_STAGE = [(Wf, Hf, w, b, F, var) for (Wf, Hf) in gc.STAGE_FRAMES + [(90, 52)] for b in gc.STAGE_RADII for w in gc.STAGE_PATCHES for F in gc.STAGE_CHANNELS
             for var in (True, False)]


def test_every_stage_case_has_set_and_clear_pairs():
    """at tau_g = 1 at least 1 % of the valid pairs are similar and at least 1 % are not: a mask of all ones or all zeros would test nothing"""
    worst_set, worst_clear = 1.0, 1.0
    for (Wf, Hf, w, b, F, var) in ALL_STAGE:
        if (Wf, Hf) == (90, 52):
            f, v, _ = gc.features(Wf, Hf, F, seed=7)
            D, valid = gr.distances(f, v if var else None, w, b, gc.floors(F, var))
        else:
            c = gc.stage_case(Wf, Hf, w, b, F, var)
            D, valid = c["D"], c["valid"]
        with np.errstate(invalid="ignore"):
            frac = float((valid & (D <= F32(1))).sum()) / float(valid.sum())
        print("%dx%d w=%d b=%d F=%d %s: %.4f of the valid pairs set" % (Wf, Hf, w, b, F, "with variances" if var else "floors only", frac))
        worst_set, worst_clear = min(worst_set, frac), min(worst_clear, 1 - frac)
        assert frac >= 0.01 and 1 - frac >= 0.01, (Wf, Hf, w, b, F, var, frac)
    print("smallest set fraction %.4f, smallest clear fraction %.4f" % (worst_set, worst_clear))


@pytest.mark.parametrize("with_var", [True, False])
@pytest.mark.parametrize("w,b", [(1, 6), (2, 3)])
def test_a_pair_at_the_threshold_is_in_and_one_ulp_below_is_out(w, b, with_var):
    c = gc.stage_case(W, H, w, b, 3, with_var)
    D, valid = c["D"], c["valid"]
    one, at, below = c["taus"]
    assert at > 0 and below < at and np.nextafter(below, F32(np.inf)) == at
    on_it = valid & (D == at)
    assert on_it.sum() >= 2                                 # the pair, seen from both of its pixels
    m_at, n_at = mr.masks_from(D, valid, b, at)
    m_below, n_below = mr.masks_from(D, valid, b, below)
    assert np.array_equal(n_at - n_below, on_it.sum(0))
    assert (m_at != m_below).any()                          # at least one bit flips
    assert np.array_equal(gr.popcount(m_at), n_at)


def test_the_gate_is_a_pure_and():
    b, w = 3, 1
    c = gc.stage_case(W, H, w, b, 3, True)
    gate, n_gate = mr.masks_from(c["D"], c["valid"], b, 1.0)
    col, cov, ns, _ = mc.noisy(W, H, seed=W + b)
    sel, n_sel = mr.masks(col, mc.pixel_cov(cov, ns), w, b, 1.0, 1e-4)
    m, n = gr.gate(sel, gate)
    assert np.array_equal(m.view(np.uint32), sel.view(np.uint32) & gate.view(np.uint32)) and np.array_equal(n, gr.popcount(m))
    assert (n <= np.minimum(n_sel, n_gate)).all() and 0 < n.sum() < min(n_sel.sum(), n_gate.sum())
    centre = b * (2 * b + 1) + b
    bit = lambda a: (a[..., centre // 32].view(np.uint32) >> np.uint32(centre % 32)) & 1
    assert np.array_equal(bit(m), bit(sel) & bit(gate))    # no special case for the centre bit


def test_the_pyramid_rule():
    Wp, Hp, F = 45, 26, 3                                   # an odd width: the last column is dropped, as by bcd_hip_downscale_avg
    f, v, _ = gc.features(Wp, Hp, F, seed=3)
    levels = gr.pyramid(f, v, 3)
    assert [l[0].shape for l in levels] == [(26, 45, 3), (13, 22, 3), (6, 11, 3)]
    f1, v1 = levels[1]
    l, k, z = 4, 7, 1
    quad = lambda a: F32(F32(0.25) * F32(F32(F32(a[2 * l, 2 * k, z] + a[2 * l + 1, 2 * k, z]) + a[2 * l, 2 * k + 1, z]) + a[2 * l + 1, 2 * k + 1, z]))
    assert bits(f1[l, k, z]) == bits(quad(f)) and bits(v1[l, k, z]) == bits(F32(quad(v) * F32(0.25)))
    # the variance of a mean of four independent pixels is a quarter of their mean variance
    assert np.allclose(v1, 0.25 * 0.25 * (v[0:26:2, 0:44:2] + v[1:26:2, 0:44:2] + v[0:26:2, 1:44:2] + v[1:26:2, 1:44:2]), rtol=1e-5)
    assert gr.pyramid(f, None, 2)[1][1] is None
    # threshold and floors stay: between pixels of one region the expected term stays about 1 at every level
    for fs, vs in levels[:2]:
        T, C, written = gr.planes(fs, vs, 1, gc.floors(F, True))
        sec = gc.region(Wp, Hp) if fs.shape[0] == Hp else None
        if sec is not None:
            i = mr.delta_index(0, 1, 1)
            same = written[i] & (sec == np.roll(sec, -1, 1))
            assert 0.5 < float(np.mean(T[i][same] / C[i][same])) < 2.0


def test_noise_free_features_separate_the_regions():
    """the frame of the GPU effect test: sigma = 0, floors 0.01.  Across the edge a channel differs by 0.3 (even k) or 0.15 (odd k) up to the smooth term's
    2 * 0.02, so a term is at least (0.15 - 0.04)^2 / 0.01 = 1.21 and the mean over a channel set that starts with an even channel is above 2; pairs of
    main pixels whose patches lie wholly in different regions are never similar at tau_g = 1."""
    Wf, Hf, w, b = 90, 52, 1, 6
    for F in (1, 3, 7):
        f, _, _ = gc.features(Wf, Hf, F, seed=7, sigma=0.0)
        D, valid = gr.distances(f, None, w, b, gc.floors(F, False))
        across = gc.across_pairs(Wf, Hf, w, b)
        across &= valid
        assert across.sum() > 1000
        assert (D[across] >= 2).all(), (F, float(D[across].min()))
