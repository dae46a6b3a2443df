"""CPU tests of the layer lists the layered stage tests run on (tests/layer_cases.py): every layer of every family keeps the float32 calibrator
meaningful (the exclusion cap of tests/test_bayes_ref_cpu.py, per family AND layer: the GPU bars are multiples of that layer's own e_32), the layers
share the case's selection and differ in content as they claim, and the float64 reference commutes with the two exact transformations."""
import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br
import layer_cases as lc

EXCLUDE_ABOVE = 1e-2   # (as tests/test_bayes_ref_cpu.py)
EXCLUSION_CAP = 0.05


@pytest.mark.parametrize("family", sorted(bc.FAMILIES))
def test_every_layer_of_a_family_stays_inside_the_exclusion_cap(family):
    """per (family, layer): at most 5 % of the full-estimate items of the isolated cases have e_32 > 1e-2.  A layer that breaks the cap gets another
    transformation or seed in layer_cases.py; the cap stays."""
    fl = lc.family_layers(family)
    n = lc.default_count(family)
    assert all(len(ls) == n for _, ls in fl)
    for k in range(n):
        full, excluded, worst = 0, 0, 0.0
        for case, ls in fl:
            layer = ls[k]
            assert layer.mask is case.mask and layer.nsim is case.nsim and layer.state is case.state and (layer.w, layer.b, layer.min_eig) == (case.w, case.b, case.min_eig)
            if case.dense or not layer.judged:
                continue
            s64, c64, items, s32 = lc.references(layer)
            K1 = 3 * (2 * case.w + 1) ** 2 + 1
            e32 = np.array([br.item_error(s32, s64, i, case.w) for i in items if i["n"] >= K1])
            full += len(e32)
            excluded += int((e32 > EXCLUDE_ABOVE).sum())
            worst = max([worst] + list(e32[e32 <= EXCLUDE_ABOVE]))
        print("%s layer %d (%s): %d full estimates, %d excluded, max e_32 %.2e" % (family, k, fl[0][1][k].name.split(" / ")[-1], full, excluded, worst))
        assert excluded <= EXCLUSION_CAP * full, (family, k, fl[0][1][k].name, excluded, full)


def test_layer_lists_contain_what_they_promise():
    case = bc.FAMILIES["sizes"]()[0]
    for n in (2, 4, 5, 7, 16):
        ls = lc.layers(case, "sizes", n)
        assert len(ls) == n and np.array_equal(ls[0].col, case.col) and np.array_equal(ls[0].pixcov, case.pixcov)
        assert len(set(l.name for l in ls)) == n
    ls = lc.layers(case, "sizes", 16)
    assert np.array_equal(ls[1].col, case.col * np.float32(2.0 ** 10)) and np.array_equal(ls[1].pixcov, case.pixcov * np.float32(4.0 ** 10))
    assert np.array_equal(ls[3].col[..., 2], case.col[..., 0]) and np.array_equal(ls[3].pixcov[..., 5], case.pixcov[..., 3])   # x'y' = yz
    # no two layers carry the same colours, and the independent ones do not correlate with layer 0's noise
    for i in range(16):
        for j in range(i + 1, 16):
            assert not np.array_equal(ls[i].col, ls[j].col), (i, j)
    r0 = case.col - bc.signal(*case.col.shape[:2])
    r2 = ls[2].col - lc.other_signal(*case.col.shape[:2])
    assert abs(float(np.corrcoef(r0.ravel(), r2.ravel())[0, 1])) < 0.02
    nf = lc.layers(bc.FAMILIES["non-finite"]()[0], "non-finite", lc.default_count("non-finite"))
    assert [bool(np.isfinite(l.col).all()) for l in nf[1:]] == [False, False, True, True, False]      # (scaled / rotated layer 0 keep layer 0's poison)
    assert not np.isfinite(nf[2].col).all() and np.isfinite(nf[2].pixcov).all() and np.isinf(nf[2].col).any() and np.isnan(nf[2].col).any()
    assert np.isfinite(nf[4].col).all() and np.isnan(nf[4].pixcov).any()
    assert np.isfinite(nf[3].col).all() and np.isfinite(nf[3].pixcov).all()                          # a finite layer between the two


def test_reference_of_a_power_of_two_scaled_layer_is_the_scaled_reference():
    """in the scaled units (floor x 4^k: Case.scaled) every float64 operation commutes with the power of two: bit for bit.  With the CALL's floor, as the
    layer lists have it, the same holds wherever the floor binds in neither problem (the well-conditioned family "sizes")."""
    case = bc.FAMILIES["floor boundary"]()[0]
    s0, c0, _ = br.accumulate(*case.args(), keep_stages=False)
    for k in (10, -12):
        s, c, _ = br.accumulate(*case.scaled(k, "scaled").args(), keep_stages=False)
        assert np.array_equal(c, c0) and np.array_equal(s, s0 * 2.0 ** k)
    case = bc.FAMILIES["sizes"]()[0]
    s0, c0, _, _ = lc.references(lc.family_layers("sizes")[0][1][0])
    s, c, _, _ = lc.references(lc.family_layers("sizes")[0][1][1])
    assert np.array_equal(c, c0) and np.array_equal(s, s0 * 2.0 ** lc.EXPONENTS[0])


def test_reference_of_the_channel_rotation_is_the_rotated_reference():
    """a permutation of the channels permutes rows and columns of every matrix: the same eigenvalues, sums in another order -- float64 round-off"""
    for family in ("sizes", "low rank"):
        case, ls = lc.family_layers(family)[0]
        s0, c0, items, _ = lc.references(ls[0])
        s3, c3, _, _ = lc.references(ls[3])
        assert np.array_equal(c0, c3)
        e = max(br.item_error(s3, s0[..., lc.ROT], it, case.w) for it in items)
        print("%s: rotated reference against reference of the rotation, per item: %.2e" % (family, e))
        assert e < 1e-9, e
