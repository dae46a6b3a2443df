"""CPU tests that hold tests/moments_ref.py -- the NumPy float32 restatement of the selection from means and covariances that the GPU stage
test compares with bit for bit -- to its claims, on the constructed frames of tests/moments_cases.py.  No GPU needed.
  * T / C are bitwise symmetric, and the vectorised planes are those of a scalar restatement of the definition on sampled pixel pairs;
  * a pixel's distance to itself is 0 wherever q > 0; with eps = 0 a pixel of zero variance is not similar to itself (0 / 0);
  * NaN covariances are not counted, NaN / infinite means make the patches that hold them not similar;
  * a pair AT the threshold is in, one ulp below it is out;
  * the float32 reference agrees with a float64 evaluation of the same formula within a bound derived from the operation count."""
import numpy as np
import pytest

import moments_cases as mc
import moments_ref as mr

F = np.float32
W, H = 70, 13


def scalar_pair(m, v, eps, x, y):
    """the definition, one float32 operation after the other, for pixels x and y (line, column)"""
    s, n = F(0), 0
    eps = F(eps)
    with np.errstate(all="ignore"):
        for k in range(3):
            d = F(m[x][k]) - F(m[y][k])
            q = F(F(v[x][k]) + F(v[y][k])) + eps
            if q > 0:
                s = F(s + F(F(d * d) / q))
                n += 1
    return s, n


def bits(a):
    return np.asarray(a, F).view(np.int32)


@pytest.mark.parametrize("eps", mc.FLOORS)
def test_planes_are_the_definition_and_bitwise_symmetric(eps):
    b = 6
    c = mc.stage_case(W, H, 1, b, eps)
    T, C, written = mr.planes(c["col"], c["P"], b, eps)
    assert written.any() and not written.all()
    rng = np.random.default_rng(3)
    special = [(2, 5), (H - 3, W - 9), (7, 23), (3, 33), (H - 4, 12)]
    pixels = special + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(150)]
    checked = 0
    for x in pixels:
        for dl, dc in mr.deltas(b)[::5] + [(0, 0), (b, -b), (b, b)]:
            y = (x[0] + dl, x[1] + dc)
            i = mr.delta_index(dl, dc, b)
            if not (0 <= y[0] < H and 0 <= y[1] < W):
                assert not written[i][x]
                continue
            assert written[i][x]
            s_xy, n_xy = scalar_pair(c["col"], c["P"], eps, x, y)
            s_yx, n_yx = scalar_pair(c["col"], c["P"], eps, y, x)
            assert bits(s_xy) == bits(s_yx) and n_xy == n_yx                      # T_delta(x) == T_-delta(x + delta), bit for bit
            assert bits(T[i][x]) == bits(s_xy) and C[i][x] == n_xy, (x, dl, dc)
            checked += 1
    assert checked > 2000


def test_self_distance_and_the_variance_floor():
    b, w = 3, 1
    centre = (b * (2 * b + 1) + b)
    inside = (7, 23)                                       # its 3 x 3 patch lies inside the block of equal colours and zero variance
    for eps in mc.FLOORS:
        c = mc.stage_case(W, H, w, b, eps)
        D, valid = c["D"], c["valid"]
        assert valid[centre, w:H - w, w:W - w].all() and not valid[centre, 0].any()
        T, C, _ = mr.planes(c["col"], c["P"], b, eps)
        own_q_positive = C[0] == 3                         # every channel counted in the pixel's pair with itself
        patch_ok = np.zeros((H, W), bool)
        for l in range(w, H - w):
            for k in range(w, W - w):
                patch_ok[l, k] = own_q_positive[l - w:l + w + 1, k - w:k + w + 1].all() and np.isfinite(c["col"][l - w:l + w + 1, k - w:k + w + 1]).all()
        assert patch_ok.sum() > 400
        assert (D[centre][patch_ok] == 0).all()            # q > 0 everywhere in the patch: the distance to itself is exactly 0
        mask, nsim = mr.masks_from(D, valid, b, 1.0)
        bit = (mask[..., centre // 32].view(np.uint32) >> np.uint32(centre % 32)) & 1
        if eps == 0.0:
            assert np.isnan(D[centre][inside])             # no channel is counted anywhere in the patch: 0 / 0
            assert bit[inside] == 0                        # ... so the pixel is not similar to itself
        else:
            assert D[centre][inside] == 0 and bit[inside] == 1
        assert (bit[patch_ok] == 1).all()


def test_nan_and_infinite_inputs():
    b, w, eps = 3, 1, 1e-4
    c = mc.stage_case(W, H, w, b, eps)
    T, C, written = mr.planes(c["col"], c["P"], b, eps)
    D, valid = c["D"], c["valid"]
    side = 2 * b + 1
    # NaN covariances: q is NaN for every pair of the pixel, no channel is counted, nothing is added
    for x in ((2, 5), (H - 3, W - 9)):
        for i in range(len(mr.deltas(b))):
            if written[i][x]:
                assert C[i][x] == 0 and T[i][x] == 0
    # ... but the pixel's patches are still compared through their other eight pixels
    assert np.isfinite(D[:, 2, 5][valid[:, 2, 5]]).all()
    # a NaN mean poisons every patch that holds it; an infinite mean makes them infinitely far (inf - inf with itself: NaN)
    mask, nsim = mr.masks_from(D, valid, b, 1.0e30)
    for x, kind in (((H - 4, 12), "nan"), ((3, 33), "inf")):
        for ol in (-1, 0, 1):
            for oc in (-1, 0, 1):
                p = (x[0] + ol, x[1] + oc)
                if not (w <= p[0] < H - w and w <= p[1] < W - w):
                    continue
                d = D[:, p[0], p[1]][valid[:, p[0], p[1]]]
                assert d.size > 0 and not np.isfinite(d).any(), (kind, p)
                if kind == "nan":
                    assert np.isnan(d).all()
                assert nsim[p] == 0                        # not similar to anything, itself included, at any finite threshold
    assert (nsim > 0).sum() > 300


@pytest.mark.parametrize("w,b", [(1, 6), (2, 3)])
def test_a_pair_at_the_threshold_is_in_and_one_ulp_below_is_out(w, b):
    eps = 1e-4
    c = mc.stage_case(W, H, w, b, eps)
    D, valid = c["D"], c["valid"]
    one, at, below = c["taus"]
    assert at > 0 and below < at and np.nextafter(below, F(np.inf)) == at
    on_it = valid & (D == at)
    assert on_it.sum() >= 2                                 # the pair, seen from both of its pixels
    _, n_at = mr.masks_from(D, valid, b, at)
    _, n_below = mr.masks_from(D, valid, b, below)
    assert np.array_equal(n_at - n_below, on_it.sum(0))
    _, n_one = mr.masks_from(D, valid, b, one)
    main = (H - 2 * w) * (W - 2 * w)
    frac = n_one.sum() / float(valid.sum())
    print("w=%d b=%d: %.1f %% of the pairs of main pixels are similar at tau = 1" % (w, b, 100 * frac))
    assert 0.05 < frac < 0.8 and n_one.max() < valid.sum(0).max() and main > 0      # masks neither empty nor full


@pytest.mark.parametrize("w,b", [(1, 6), (2, 3)])
def test_float32_reference_against_float64(w, b):
    """Inputs: the noisy frame (finite, variances > 0, eps > 0: every q > 0, every term >= 0).  Relative error of a float32 patch distance against the
    float64 evaluation of the same formula on the same float32 inputs, u = 2^-24:
      per term (d * d) / q: d carries one rounding and enters squared (2u), the product one (u), q two additions of non-negative values (2u), the
      division one (u): 6u;  a term then passes through at most 2 additions inside T (three channels, the first added to 0 exactly) and
      (2w+1)^2 - 1 additions of the patch sum (all summands >= 0, so relative errors do not grow);  one division by the exactly converted count.
    k = 6 + 2 + ((2w+1)^2 - 1) + 1 roundings: the bar is (1 + u)^k - 1 plus the float64 side's own 2^-50.  For w = 1 that is 17 u = 1.0e-6; counting
    every addition of the 27-term chain instead (4 + 26 + 1 = 31 u) would be looser.  Derived, not tuned."""
    eps = 1e-4
    col, cov, ns, _ = mc.noisy(W, H, seed=11)
    P = mc.pixel_cov(cov, ns)
    assert (P[..., :3] > 0).all()
    D32, valid = mr.distances(col, P, w, b, eps)
    D64, valid64 = mr.distances(col, P, w, b, eps, dtype=np.float64)
    assert np.array_equal(valid, valid64)
    a, r = D32[valid].astype(np.float64), D64[valid]
    assert np.isfinite(r).all() and (r >= 0).all()
    u = 2.0 ** -24
    k = 6 + 2 + ((2 * w + 1) ** 2 - 1) + 1
    bar = (1 + u) ** k - 1 + 2.0 ** -50
    nz = r > 0
    rel = np.max(np.abs(a[nz] - r[nz]) / r[nz])
    print("w=%d b=%d: max relative deviation float32 vs float64 %.3e (bar %.3e, %d pairs)" % (w, b, rel, bar, nz.sum()))
    assert (a[~nz] == 0).all()
    assert rel <= bar
