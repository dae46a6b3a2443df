"""GPU tests of k_prepare_solve27, the prepare and eigensolver phases of a full estimate in one persistent kernel, against the two kernels it
replaces (k_bayes27w<1>, then k_jacobi27_quads).

Both forms call the same device functions on the same inputs in the same order, and the records they leave (A after the solver, V, C, noise + mean,
eigenvalues, the redo list's counter) do not depend on which wavefront takes which item: bcd_hip_selftest_prepare_solve runs both on one list and
counts the 32-bit words in which the records differ.  The expected count is 0 and 0 is asserted -- not a tolerance.

Lists (inputs from tests/bayes_cases.py):
  * 1, 2 and 3 items (an absent second matrix, one pair, a pair and a half), the first two with |S| = 28 and |S| = 169;
  * every full estimate of the "sizes" frame (|S| from 28 to 169, an odd and an even count);
  * the "non-finite: nan pixcov" frame: items whose noise mean poisons them (noise_poisons_item);
  * a 96 x 96 frame with every main pixel processed and its whole window similar (the -m 0 state) at a CU share of 1 %: two dozen wavefronts with
    some 180 tasks each, the LDS area reused by prepare and solve again and again;
  * the list's length read on the device: longer than the records' capacity (the clamp to the capacity) and shorter (wavefronts without an item).
And the estimate call itself (bcd_hip_bayes_accumulate) on three families with the fused kernel and with the two launches: counts, non-finite
patterns, fallback means and the per-item bar of tests/test_gpu_bayes_stage.py against float64, for both."""
import numpy as np
import pytest

import bayes_cases as bc
import test_gpu_bayes_stage as stage

pytestmark = pytest.mark.gpu

K1 = 28                                                                   # |S| from which an item gets the full estimate (3 (2w+1)^2 + 1, w = 1)


def full_items(case):
    """pixel indices (line * W + column) of the full estimates of a case, scan order"""
    H, W = case.state.shape
    l, c = np.nonzero((case.state == 1) & (case.nsim >= K1))
    return (l * W + c).astype(np.int32)


def differing_words(hipctx, case, items, **kw):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = hipctx.selftest_prepare_solve(t(case.col), t(case.pixcov), t(case.mask.view(np.int32)), t(items), **kw)
    hipctx.synchronize()
    return n


_cases = {}


def case_of(name):
    if not _cases:
        _cases["sizes"] = bc.fam_sizes()[0]
        _cases["nan pixcov"] = [c for c in bc.fam_non_finite() if c.name.endswith("nan pixcov")][0]
    return _cases[name]


def test_one_two_and_three_items_smallest_and_largest_set(hipctx):
    case = case_of("sizes")
    items = full_items(case)
    size = case.nsim.reshape(-1)[items]
    assert (size == 28).any() and (size == 169).any()
    first = [items[size == 28][0], items[size == 169][0], items[size == 64][0]]
    for n in (1, 2, 3):
        assert differing_words(hipctx, case, np.array(first[:n], np.int32)) == 0, n


def test_every_full_estimate_of_the_sizes_frame_odd_and_even_count(hipctx):
    case = case_of("sizes")
    items = full_items(case)
    assert len(items) >= 20 and set(case.nsim.reshape(-1)[items]) >= {28, 29, 32, 33, 63, 64, 65, 128, 168, 169}
    odd = items if len(items) % 2 else items[:-1]
    assert differing_words(hipctx, case, odd) == 0
    assert differing_words(hipctx, case, items[:len(odd) - 1]) == 0


def test_items_poisoned_by_their_noise_mean(hipctx):
    case = case_of("nan pixcov")
    items = full_items(case)
    # (a NaN in the per-pixel covariance of a member: the item's noise mean is not finite)
    poisoned = [p for p in items if not np.isfinite(case.pixcov[max(0, p // case.col.shape[1] - 7):p // case.col.shape[1] + 8,
                                                               max(0, p % case.col.shape[1] - 7):p % case.col.shape[1] + 8]).all()]
    assert len(poisoned) >= 2 and len(poisoned) < len(items)
    assert differing_words(hipctx, case, items) == 0


def test_dense_frame_at_a_low_cu_share_reuses_the_lds_area(hipctx):
    H = W = 96
    rng = np.random.default_rng(115)
    col, pc = bc.noisy_frame(H, W, rng)
    case = bc.Case("all in", col, pc, {(l, c): bc.window(l, c, H, W, 1, 6) for l in range(1, H - 1) for c in range(1, W - 1)}, dense=True)
    items = full_items(case)
    assert len(items) == (H - 2) * (W - 2)
    assert differing_words(hipctx, case, items, cu_share_pct=1) == 0


def test_list_length_read_on_the_device_clamps_both_ways(hipctx):
    case = case_of("sizes")
    items = full_items(case)
    n = len(items)
    assert n >= 20
    assert differing_words(hipctx, case, items, capacity=n // 2 | 1, list_len=n) == 0          # the list is longer than the records' capacity
    assert differing_words(hipctx, case, items, capacity=n + 37, list_len=n - (n % 2 == 0)) == 0  # shorter: an odd count, wavefronts without an item
    assert differing_words(hipctx, case, items, capacity=n, list_len=0) == 0                    # nothing listed


@pytest.mark.parametrize("family", ["sizes", "non-finite", "floor boundary"])
def test_estimate_call_fused_and_as_two_launches(hipctx, family):
    import bcd_amd.hip as bh
    cases, fused, _ = stage.hip_results(hipctx, family)                    # (the default: fused)
    try:
        bh.set_fused_prepare_solve(False)
        split = [stage.run_hip(hipctx, c) for c in cases]
    finally:
        bh.set_fused_prepare_solve(True)
    for case, (s_f, c_f, redo_f), (s_s, c_s, redo_s) in zip(cases, fused, split):
        assert np.array_equal(c_f, c_s), case.name
        assert redo_f == redo_s, (case.name, redo_f, redo_s)               # (the same records: the same items decline the sweep inverse)
    for results in (fused, split):
        stage.judge_exact(family, cases, results)                          # counts, non-finite patterns, fallback means against float64
        stage.judge_numerical(family, cases, results)                      # the per-item bar of test_gpu_bayes_stage.py
