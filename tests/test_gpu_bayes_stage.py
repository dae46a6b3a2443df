"""GPU tests of the Bayesian estimate kernels on constructed similar sets, per item, against float64.

bcd_hip_bayes_accumulate takes masks, |S| and the state image as arguments: every case of tests/bayes_cases.py is handed to it directly and
compared with tests/bayes_ref.py (float64 NumPy, written from the reference text).  The processed pixels of an isolated case are 2 (b + w) + 1
apart, so sum / count at the pixels an item touches are that item's own aggregate and a failure names the item.

What is asserted (nothing in a bar comes from a GPU run):
  * count equals the reference's integers everywhere; the set of non-finite entries of sum equals the reference's;
  * fallback items (|S| < 3 (2w+1)^2 + 1): |sum - mean_64| <= |S| u max|x| per entry, u = 2^-24;
  * full estimates, per item: e_hip = max |sum_hip - sum_64| / s, s the largest |sum_64| over the pixels THAT ITEM touches, and
        e_hip <= 4 max(e_32, median of e_32 over the family, 8 u)
    e_32 being the same quantity for the float32 calibrator (bayes_ref with dtype = float32) computed here on the CPU.  The factor 4 is the margin
    for the two documented differences from a plain fp32 evaluation: summation order on the matrix core and the early-stopped Jacobi with its
    first-order correction.  An item with e_32 > 1e-2 is checked for count and finiteness only; at most 5 % of a family (test_bayes_ref_cpu.py);
  * dense cases (every main pixel processed: atomics from many items on one pixel): the same rule with the error of a pixel taken relative
    to the largest |sum_64| of its 15 x 15 neighbourhood, over the frame;
  * everything again with bcd_hip_set_strict_eigensolver(True): same bar, and per family max e_strict <= 1.5 max e_prod + 8 u;
  * the paths: bcd_hip_bayes_last_redo_count() > 0 where a family exists to reach the redo list (k_bayes27w<2> after a declined sweep inverse),
    and == 0 on well-conditioned cases: both sides of the acceptance test of the sweep inverse.
Two tests per family: what needs no numerical bar (counts, patterns, fallback means, paths, strict against production), and the per-item bar.

Which family reaches which kernel (dispatcher: bayes() in bcd_api.hip):
  w = 1, b = 6    k_bayes27w<1> -> k_jacobi27_quads -> k_finish27w, redo list k_bayes27w<2>; fallback k_bayes_weak_tile    every family but the last
  w = 1, b = 12   k_bayes27w<1, 12> -> k_jacobi27_quads -> k_finish27w<12>, redo list k_bayes27<2> (|S| up to 625)             other kernels
  w = 1, b = 3, 4 k_bayes27<1> -> k_jacobi27_quads -> k_bayes27<2> (gather kernels; no redo list, no counter)             other kernels
  w = 2, b = 6    k_bayes_strong_generic, fallback k_bayes_weak;   w = 2, b = 3: k_bayes_weak only;   w = 0, b = 4: generic    other kernels

Measured on the MI355X: MEASURED below, the table per family in docs/EXPERIMENTS.md section 6."""
import os

import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br

pytestmark = pytest.mark.gpu

U = br.U32
MARGIN = 4.0
FLOOR = 8 * U
EXCLUDE_ABOVE = 1e-2
EXCLUSION_CAP = 0.05

# Measured on the MI355X after the two kernel fixes this test bed led to (power-of-two rescaling in the sweep inverse, NaN mean for a non-finite
# noise mean): the largest e_hip / max(e_32, median e_32, 8 u) over a family's isolated items, production | strict rule.  The bar is 4.
#   sizes 0.82 | 0.82   borders 0.72 | 0.67   pure noise 1.21 | 1.21   constant 0.75 | 0.75   zero noise 0.34 | 0.34   low rank 0.83 | 0.83
#   floor boundary 2.08 | 1.57   dark 2.17 | 2.33   scaling 0.61 | 0.65   non-finite (its finite items) 0.77 | 0.77   spike 3.55 | 3.46
#   other kernels 3.77 | 3.77 ("w=2 b=6 sizes", k_bayes_strong_generic with K = 75, an item with |S| = 100: e_hip 1.8e-6 where e_32 is 2.5e-7 and the floor
#   8 u = 4.8e-7 sets the bar; "w=2 b=6 pure noise" 3.54; every other geometry -- b = 12, b = 3, 4 gather kernels, w = 0 -- stays at or below 1.2)
#   spike + cov 27.4 | 4.37: the one family over the bar (by a factor 27.4 / 4 = 6.9 under the production rule, 1.09 under the strict one), see KNOWN_MISSES
#   degenerate: not judged (e_32 and e_hip both 0.19)
# Before the fixes: "scaling" x 2^6: e_hip 7e-6 ... 1.9e-4 (ratio up to 400), x 2^12: 0.1 ... 0.9; "spike" x 1000: up to 1.7e-3; "spike + cov" x 10^4: up to
# 1e12; "non-finite" (NaN pixcov): 49 ... 450 of an item's 441 ... 675 output values NaN where the reference has all of them NaN.


def _report(line):
    print(line)
    if os.environ.get("BCD_TEST_REPORT"):
        with open(os.environ["BCD_TEST_REPORT"], "a") as f:
            f.write(line + "\n")


def run_hip(hipctx, case):
    """-> (sum, count, items the finish kernel handed to the redo list or None where the counter does not exist)"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s, c = hipctx.bayes_accumulate(t(case.col), t(case.pixcov), t(case.mask.view(np.int32)), t(case.nsim), t(case.state), case.w, case.b, case.min_eig)
    redo = hipctx.bayes_last_redo_count() if (case.w == 1 and case.b in (6, 12)) else None   # (the gather and generic kernels have no redo list)
    hipctx.synchronize()
    return s.cpu().numpy(), c.cpu().numpy(), redo


_refs = {}


def references(case):
    """float64 reference and float32 calibrator of a case, once per session (the strict run reuses them)"""
    if id(case) not in _refs:
        s64, c64, items = br.accumulate(*case.args(), keep_stages=False)
        s32, _, _ = br.accumulate(*case.args(), dtype=np.float32, keep_stages=False)
        _refs[id(case)] = (case, s64, c64, items, s32)
    return _refs[id(case)][1:]


def check_exact_parts(case, s_hip, c_hip, s64, c64):
    assert np.array_equal(c_hip, c64), (case.name, "count", np.argwhere(c_hip != c64)[:5])
    if case.judged:
        assert np.array_equal(np.isfinite(s_hip), np.isfinite(s64)), (case.name, "non-finite pattern", np.argwhere(np.isfinite(s_hip) != np.isfinite(s64))[:5])
    else:
        assert np.isfinite(s_hip)[np.isfinite(s64)].all(), (case.name, "non-finite value where float64 has none")


def check_fallback_items(case, s_hip, s64, items):
    """mean of <= 3 (2w+1)^2 values: |S| u max|x| per entry, max|x| over the members' values of that entry"""
    K1 = 3 * (2 * case.w + 1) ** 2 + 1
    for it in items:
        if not 0 < it["n"] < K1:
            continue
        x = np.abs(br.gather(case.col, it["members"], case.w).astype(np.float64))     # (n, P, 3)
        bound = it["n"] * U * x.max(axis=0)
        r, c = br.touched(it, case.w)
        d = np.abs(s_hip[r, c].astype(np.float64) - s64[r, c])
        ok = np.isfinite(s64[r, c])
        assert (d[ok] <= bound[ok]).all(), (case.name, it["pos"], it["n"], float((d[ok] / bound[ok].clip(1e-300)).max()))


def item_errors(case, s_hip, s64, s32, items):
    """per full-estimate item with a finite reference: (item, e_hip, e_32)"""
    K1 = 3 * (2 * case.w + 1) ** 2 + 1
    out = []
    for it in items:
        if it["n"] < K1 or not np.isfinite(s64[br.touched(it, case.w)]).all():
            continue
        out.append((it, br.item_error(s_hip, s64, it, case.w), br.item_error(s32, s64, it, case.w)))
    return out


def judge_exact(family, cases, results):
    """counts, non-finite patterns and the fallback means of every case: nothing here depends on a numerical bar"""
    for case, (s_hip, c_hip, _) in zip(cases, results):
        s64, c64, items, s32 = references(case)
        check_exact_parts(case, s_hip, c_hip, s64, c64)
        if not case.dense:
            check_fallback_items(case, s_hip, s64, items)


def family_figures(family, cases, results):
    """-> (figures of the family, rows (case, item, e_hip, e_32, bar or None if excluded), dense rows (case, e_hip, e_32)); asserts nothing but the cap"""
    rows, dense = [], []
    for case, (s_hip, c_hip, _) in zip(cases, results):
        s64, c64, items, s32 = references(case)
        if case.dense:
            if case.judged:
                dense.append((case, br.rel_local(s_hip, s64), br.rel_local(s32, s64)))
            continue
        rows += [(case, it, eh, e3) for (it, eh, e3) in item_errors(case, s_hip, s64, s32, items)]
    e32 = np.array([r[3] for r in rows])
    ehip = np.array([r[2] for r in rows])
    fig = dict(items=len(rows), excluded=0, max_e32=0.0, max_ehip=0.0, max_ratio=0.0, max_raw_ratio=0.0,
               dense=max([eh / max(e3, FLOOR) for (_, eh, e3) in dense] + [0.0]))
    if not len(rows):
        return fig, [], dense
    if not cases[0].judged:                                              # (the degenerate family: reported, not judged)
        fig.update(max_e32=float(e32.max()), max_ehip=float(ehip.max()), max_raw_ratio=float((ehip / e32.clip(FLOOR)).max()))
        return fig, [], dense
    keep = e32 <= EXCLUDE_ABOVE
    assert (~keep).sum() <= EXCLUSION_CAP * len(rows), (family, int((~keep).sum()), len(rows))
    bar = MARGIN * np.maximum(np.maximum(e32, np.median(e32)), FLOOR)
    fig.update(excluded=int((~keep).sum()), max_e32=float(e32[keep].max()), max_ehip=float(ehip[keep].max()), median_e32=float(np.median(e32)),
               max_ratio=float((ehip / bar * MARGIN)[keep].max()), max_raw_ratio=float((ehip / e32.clip(1e-300))[keep & (e32 > 0)].max(initial=0.0)))
    return fig, [(c, it, eh, e3, (b_ if k else None)) for (c, it, eh, e3), b_, k in zip(rows, bar, keep)], dense


def judge_numerical(family, cases, results):
    fig, rows, dense = family_figures(family, cases, results)
    for case, e_hip, e_32 in dense:
        assert e_hip <= MARGIN * max(e_32, FLOOR), (case.name, e_hip, e_32)
    for case, it, eh, e3, b_ in rows:
        assert b_ is None or eh <= b_, "%s item %s |S| = %d: e_hip %.3e > bar %.3e (e_32 %.3e, family median %.3e); cond1 %.2e cond2 %.2e, eigenvalues of C - N in [%.2e, %.2e]" % (
            case.name, it["pos"], it["n"], eh, b_, e3, fig["median_e32"], it["cond1"], it["cond2"], float(np.min(it["eig_cmn"])), float(np.max(it["eig_cmn"])))
    return fig


# Path coverage, asserted: cases that exist to reach the redo list (the floor is inside the spectrum of the matrices that are inverted, or an eigenvalue
# is exactly 0: the sweep inverse must decline and k_bayes27w<2> take the item) ...
REDO_EXPECTED = ("floor k=0 e=0.03", "floor dense e=3e-2", "floor k=-12 e=1e-08", "floor k=-14 e=1e-08", "floor k=-16 e=1e-08", "low rank: zero channel")
# ... and well-conditioned cases on the other side of the acceptance test, where every sweep inverse must be accepted
REDO_FORBIDDEN = ("floor k=0 e=1e-08", "floor k=-4 e=1e-08", "sizes", "pure noise", "dark, floor scaled with the frame")

_hip = {}


def hip_results(hipctx, family):
    """(cases, production results, strict results) of a family, once per session"""
    if family not in _hip:
        import bcd_amd.hip as bh
        cases = bc.FAMILIES[family]()
        prod = [run_hip(hipctx, c) for c in cases]
        try:
            bh.set_strict_eigensolver(True)
            strict = [run_hip(hipctx, c) for c in cases]
        finally:
            bh.set_strict_eigensolver(False)
        _hip[family] = (cases, prod, strict)
    return _hip[family]


@pytest.mark.parametrize("family", sorted(bc.FAMILIES))
def test_estimate_kernels_counts_non_finite_patterns_fallback_means_and_paths(hipctx, family):
    """what does not depend on a numerical bar, for every family, under both stopping rules; and which path the items took"""
    cases, prod, strict = hip_results(hipctx, family)
    for case, (_, _, redo) in zip(cases, prod):
        if redo:
            _report("bayes-stage %-14s %-30s redo list: %d items" % (family, case.name, redo))
        if case.name in REDO_EXPECTED:
            assert redo > 0, (case.name, redo)
        if case.name in REDO_FORBIDDEN:
            assert redo == 0, (case.name, redo)
    judge_exact(family, cases, prod)
    judge_exact(family, cases, strict)
    if cases[0].judged:                                                  # the strict rule is not worse than the production rule
        fp, fs = family_figures(family, cases, prod)[0], family_figures(family, cases, strict)[0]
        assert fs["max_ehip"] <= 1.5 * fp["max_ehip"] + FLOOR, (family, fs["max_ehip"], fp["max_ehip"])


# A family that misses its numerical bar stays in, as a strict expected failure of THAT bar with the measured figures (docs/EXPERIMENTS.md section 6);
# its counts, non-finite patterns, fallback means and the strict / production relation are asserted by the test above.
KNOWN_MISSES = {
    "spike + cov": "one pixel 10^2 ... 10^4 times brighter than its patch with a covariance to match, cond(C1) 2.6e4 ... 3.5e8.  Production rule: 12 of 120 items at "
                   "2.8e-6 ... 1.3e-5 where the float32 calibrator is 2.5e-8 ... 2.4e-6 on the same item, e_hip / max(e_32, median, 8 u) up to 27.4 (bar 4).  Strict "
                   "rule: up to 4.37, 1.0e-5 at worst.  So the cause is the early stop of the eigensolver: off^2 <= 2e-9 diag^2 is relative to the WHOLE matrix, whose "
                   "norm is the spike's variance (1e4 ... 1e6 times the ordinary eigenvalues), so the residual it leaves is as large as or larger than the eigenvalues "
                   "the ordinary pixels live on, and the first-order correction of max(0, .) does not hold where the residual exceeds the gaps.  Not the sweep "
                   "inverse, F C F^T or the affine output form (float32 simulations of the same items).  The remaining 1.09 x under the strict rule is the solver's "
                   "26 u against LAPACK's 3 u.  A fix belongs in the stop rule (per-row instead of global) and is not part of this change.",
}


@pytest.mark.parametrize("family", [pytest.param(f, marks=pytest.mark.xfail(strict=True, reason=KNOWN_MISSES[f])) if f in KNOWN_MISSES else f
                                    for f in sorted(bc.FAMILIES)])
def test_estimate_kernels_per_item_against_float64(hipctx, family):
    cases, prod, strict = hip_results(hipctx, family)
    figs = []
    for results in (prod, strict):
        fig, rows, dense = family_figures(family, cases, results)
        figs.append(fig)
        for case, e_hip, e_32 in dense:
            _report("bayes-stage %-14s %-30s dense: e_32 %.2e e_hip %.2e" % (family, case.name, e_32, e_hip))
    fp, fs = figs
    _report("bayes-stage %-14s | %d | %d | %.1e | %.1e | %.2f | %.1f | %.1e | %.2f | %.1f | dense %.2f / %.2f" % (
        family, fp["items"], fp["excluded"], fp["max_e32"], fp["max_ehip"], fp["max_ratio"], fp["max_raw_ratio"],
        fs["max_ehip"], fs["max_ratio"], fs["max_raw_ratio"], fp["dense"], fs["dense"]))
    judge_numerical(family, cases, prod)
    judge_numerical(family, cases, strict)


def test_call_sequence_of_the_stateful_launch_logic(hipctx):
    """bayes() in bcd_api.hip keeps the previous call's item count per geometry: one context of its own, one geometry, four calls --
    600 items (first call: synchronous), 600 (launched ahead for 600 + 1/8 + 1024 with the length read on the device), 3 000 (the guess too small:
    chunks of the guessed size, records regrown), 10 (ahead with nearly every wavefront idle).  Each call against float64, a pixel's error
    relative to the largest |sum_64| of its 15 x 15 neighbourhood, bar 4 max(the calibrator's same figure, 8 u)."""
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        for case in bc.call_sequence():
            s_hip, c_hip, _ = run_hip(ctx, case)
            s64, c64, items, s32 = references(case)
            check_exact_parts(case, s_hip, c_hip, s64, c64)
            e_hip, e_32 = br.rel_local(s_hip, s64), br.rel_local(s32, s64)
            _report("bayes-stage %-14s %-30s e_32 %.2e e_hip %.2e" % ("call sequence", case.name, e_32, e_hip))
            assert e_hip <= MARGIN * max(e_32, FLOOR), (case.name, e_hip, e_32)
    finally:
        ctx.close()
