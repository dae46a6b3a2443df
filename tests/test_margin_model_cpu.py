"""CPU check of the margin decision (tests/margin_ref.py) against the float32 transcription of the reference (tests/similarity_ref.py), over the
families of tests/similarity_cases.py: every w = 1 case of a depth the approximate kernel has, at the thresholds of its ladder, in each form of the
distance kernel that writes margin planes for its sample counts (n = 16: uniform; n = 12 and mixed counts: the reference's operations, which the
device takes where the RATIO form -- it keeps T and C planes -- declines).

The condition takes no tolerance: zero decided pairs may disagree with the reference, i.e. every disagreement between the sign of the margin sum and
the reference lies inside the band B and is listed.  The `half` family -- all nine entries of a patch rounded the same way by binary16 -- runs its whole
ladder; the other cases the threshold on the plateau, its two float neighbours and both edges of the T / C planes' band."""
import numpy as np
import pytest

import margin_ref as mr
import similarity_cases as sc

F = np.float32
CASES = [c.name for c in sc.small_cases() if c.w == 1 and c.D in (60, 36, 24)]


def thresholds(case):
    taus = [t for t in case.taus if sc.TAU_MIN <= t <= sc.TAU_MAX]
    if case.family == "half":
        return taus
    return taus[:3] + [t for i, t in enumerate(taus) if i in (3, 8)]


def forms(case):
    return ["uniform"] if case.variant == "n16" else ["general"]


@pytest.mark.parametrize("name", CASES)
def test_no_decided_pair_disagrees_with_the_reference(name):
    case = sc.by_name(name)
    checked = 0
    for form in forms(case):
        for tau in thresholds(case):
            E, touched, _ = mr.margin_planes(case.hist, case.ns, case.b, tau, form, case.bins)
            wrong, border, decided = mr.check(case.dist, mr.decide(E, touched, case.b, case.D, tau), tau)
            assert wrong == 0, (name, form, float(tau), wrong)
            assert decided > 0, (name, form, float(tau))
            checked += 1
    assert checked > 0, name


def test_a_tie_is_listed_and_a_patch_without_a_live_bin_is_not():
    """on the sparse plateau at tau = d every tie is borderline (the band can never be narrower than the reference's own rounding); in the frame with a
    block of empty histograms the pairs without any counted bin are decided (not similar), not listed"""
    case = sc.by_name("plateau sparse 64x40 n16")
    tau = case.values[0]
    E, touched, _ = mr.margin_planes(case.hist, case.ns, case.b, tau, "uniform", case.bins)
    dec = mr.decide(E, touched, case.b, case.D, tau)
    side = 2 * case.b + 1
    fwd = np.zeros(side * side, bool)
    fwd[(side * side - 1) // 2 + 1:] = True
    ties = (case.dist == tau) & fwd[None, None, :]
    assert ties.sum() > 1000 and (dec[ties] == 2).all()
    case = sc.by_name("counts edge and empty 48x32 n16")
    tau = case.values[0]
    E, touched, _ = mr.margin_planes(case.hist, case.ns, case.b, tau, "uniform", case.bins)
    dec = mr.decide(E, touched, case.b, case.D, tau)
    empty = np.isnan(case.dist) & fwd[None, None, :]
    assert empty.sum() > 100 and (dec[empty] == 0).all()
