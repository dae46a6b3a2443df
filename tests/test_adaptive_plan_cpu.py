"""CPU tests of adaptive sample planning: the C ABI's defaults and argument checks (no device needed), and the invariants of the
NumPy reference (tests/plan_ref.py) that the GPU tests hold the device to."""
import ctypes as C

import numpy as np
import pytest

import bcd_amd.hip as bh
import plan_ref as pr


def test_default_plan_params():
    p = bh.default_plan_params()
    assert (p.threshold, p.min_samples, p.max_per_pixel) == (0.0, 2.0, 16)
    assert p.eps == np.float32(1e-3)


def test_plan_rejects_a_null_accumulator():
    L = bh.lib()
    pix = (C.c_int32 * 4)(*[-7] * 4)
    summ = bh.PlanSummary(-1, -1, -1, -1.0)
    prm = bh.default_plan_params()
    rc = L.bcd_hip_accum_plan(None, C.byref(prm), 4, 0, None, None, C.cast(pix, C.c_void_p), 4, C.byref(summ))
    assert rc == -1                                              # BCD_HIP_EINVAL
    assert list(pix) == [-7] * 4 and summ.planned == -1


@pytest.mark.parametrize("seed", range(6))
def test_reference_split_invariants(seed):
    """random weights (zeros, the 2^24 of unsampled pixels, 1s): before the cap the counts sum to the budget and each is the floor or the
    ceiling of its share; the cap only lowers counts; offsets move the leftovers, not the total"""
    rng = np.random.default_rng(seed)
    N = int(rng.integers(1, 3000))
    q = rng.integers(0, 1 << 24, N).astype(np.uint64)
    q[rng.random(N) < 0.3] = 0
    q[rng.random(N) < 0.05] = pr.Q_INF
    q[rng.random(N) < 0.05] = 1
    Q = int(q.sum())
    for B in (0, 1, N // 3, N, 7 * N + 5, (1 << 31) - 1):
        seen = set()
        for off in (0, 1, 12345, (1 << 64) - 1):
            capped, n = pr.split(q, B, off, 16)
            if Q == 0 or B == 0:
                assert not n.any() and not capped.any()
                continue
            assert int(n.sum()) == B
            lo = np.array(q.astype(object) * B // Q, np.int64)
            assert np.all((n == lo) | (n == lo + 1)) and np.all(n[q == 0] == 0)
            assert np.array_equal(capped, np.minimum(n, 16))
            seen.add(tuple(n.tolist()))
        if Q and B and any(q.astype(object) * B % Q):
            assert len(seen) > 1


def test_reference_error_and_plan():
    """+inf for empty, one-sample and below-min_samples pixels; q = 2^24 for them; the list is the counts expanded in pixel order"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    ns = np.array([[[0.0], [1.0], [4.0], [4.0], [4.0]]], np.float32)
    mean = np.array([[[nan] * 3, [0.5] * 3, [0.5] * 3, [0.0] * 3, [0.2, 0.3, 0.4]]], np.float32)
    cov = np.array([[[nan] * 6, [inf] * 6, [0.04] * 3 + [0] * 3, [0.0] * 6, [0.01, 0.02, 0.03, 0, 0, 0]]], np.float32)
    e = pr.error_image(ns, mean, cov)
    assert np.isinf(e[0, 0]) and np.isinf(e[0, 1]) and e[0, 3] == 0
    F = np.float32
    assert e[0, 2] == np.sqrt(((F(0.04) * F(0.25) + F(0.04) * F(0.25)) + F(0.04) * F(0.25)) / F(3)) / (F(1e-3) + F(1.5) / F(3))
    q, E, active, unsampled = pr.weights(e)
    assert (active, unsampled) == (4, 2) and E == max(e[0, 2], e[0, 4])
    assert list(q) == [1 << 24, 1 << 24, int(e[0, 2] / E * F(16777216)), 0, int(e[0, 4] / E * F(16777216))]
    counts, pixels, summ = pr.plan(e, 10, max_per_pixel=3)
    assert np.array_equal(pixels, np.repeat(np.arange(5), counts.reshape(-1))) and summ["planned"] == int(counts.sum())
    assert counts[0, 3] == 0 and counts.max() <= 3
