"""GPU tests of adaptive sample planning on the device accumulator (bcd_hip_accum_plan, Accumulator.plan,
DeviceSamplesAccumulator::planSamples): the error image, counts, pixel list and summary bit for bit against tests/plan_ref.py on the
statistics of the reference-pinned host accumulator fed the same stream; the plan leaves the state alone; a closed adaptive loop beats
uniform passes; an adaptive snapshot denoises like the oracle; the C++ class plans what the Python call plans."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import plan_ref as pr
from test_gpu_accumulator import bits_equal, dense_stream, dev, host, random_samples, stream_of

pytestmark = pytest.mark.gpu

TOL = 1e-4


def mixed_stream(acc, rng, W, H, rows=(2, None)):
    """dense 1-spp passes over rows [r0, r1), then weighted scattered extras (single samples on otherwise empty pixels, spikes and zeros
    among the colours); returns the oracle stream of everything that was added"""
    r0, r1 = rows[0], rows[1] if rows[1] is not None else H - 2
    N = W * H
    parts = []
    for k in range(2):
        p = random_samples(rng, (r1 - r0, W, 1, 3))
        acc.add_dense(dev(p), row0=r0)
        parts.append(dense_stream(p, None, row0=r0))
    n = 3 * N
    pix = rng.integers(0, N, n).astype(np.int32)
    pix[rng.random(n) < 0.5] = rng.integers(r0 * W, r1 * W)     # (half of them on the dense rows)
    rgb = random_samples(rng, (n, 3), spike=0.05)
    rgb[rng.random(n) < 0.02] = 0.0
    w = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), n)
    acc.add_samples(dev(pix), dev(rgb), dev(w))
    parts.append(stream_of(pix, rgb, w, W))
    return np.concatenate(parts, 0)


def ref_error(stream, W, H, **kw):
    ns, mean, cov, _ = ol.oracle_ops()["accumulate"](stream, W, H)
    return pr.error_image(ns, mean, cov, **kw)


def check_plan(acc, e, budget, offset=0, threshold=0.0, max_per_pixel=16):
    """the device plan against the reference, and the invariants of the definition; returns the summary"""
    pixels, counts, err, summ = acc.plan(budget, offset=offset, threshold=threshold, max_per_pixel=max_per_pixel, error=True)
    want_counts, want_pixels, want_summ = pr.plan(e, budget, offset, threshold, max_per_pixel)
    assert bits_equal(err.cpu().numpy(), e)
    got_counts, got_pixels = counts.cpu().numpy(), pixels.cpu().numpy()
    assert np.array_equal(got_counts, want_counts)
    assert np.array_equal(got_pixels, want_pixels)
    assert {k: summ[k] for k in ("planned", "active", "unsampled")} == {k: want_summ[k] for k in ("planned", "active", "unsampled")}
    assert bits_equal(np.float32(summ["max_error"]), np.float32(want_summ["max_error"]))
    T = summ["planned"]
    assert got_pixels.shape == (T,) and int(got_counts.sum()) == T <= budget
    assert np.all(np.diff(got_pixels) >= 0)
    assert np.array_equal(np.bincount(got_pixels, minlength=e.size), got_counts.reshape(-1))
    q, _, _, _ = pr.weights(e, threshold)
    _, uncapped = pr.split(q, budget, offset, max_per_pixel)
    Q = int(q.sum())
    if Q and budget:
        assert int(uncapped.sum()) == budget
        share = q.astype(object) * budget
        lo = np.array(share // Q, np.int64)
        assert np.all((uncapped == lo) | (uncapped == lo + 1))
        if uncapped.max() <= max_per_pixel:
            assert T == budget
    else:
        assert T == 0
    return summ


def test_error_image_bit_for_bit(hipctx):
    """dense and weighted scattered passes, never-sampled rows, one-sample pixels, spikes and zeros: e and its +inf cases, with the
    default parameters and with others"""
    W, H = 80, 50
    rng = np.random.default_rng(1)
    acc = hipctx.accumulator(W, H, capacity=4096)
    stream = mixed_stream(acc, rng, W, H)
    ns, mean, cov, _ = ol.oracle_ops()["accumulate"](stream, W, H)
    for kw in ({}, {"eps": 0.25, "min_samples": 5.0}, {"eps": 1e-6, "min_samples": 0.0}):
        e = pr.error_image(ns, mean, cov, **kw)
        _, _, err, summ = acc.plan(100, error=True, **{"eps": kw.get("eps", 1e-3), "min_samples": kw.get("min_samples", 2.0)})
        assert bits_equal(err.cpu().numpy(), e)
        fin = np.isfinite(e)
        assert fin.sum() > W * H // 4 and (~fin).sum() > 2 * W    # (the never-sampled rows, and the one-sample pixels)
        assert summ["unsampled"] == int((~fin).sum()) and summ["active"] == int((e > 0).sum())
    single = (ns[..., 0] >= 2) & ~np.isfinite(pr.error_image(ns, mean, cov))
    assert single.sum() > 10                                     # one sample of weight >= 2: infinite bias factor -> e = inf
    acc.close()


def test_plan_bit_for_bit(hipctx):
    W, H = 80, 50
    N = W * H
    rng = np.random.default_rng(2)
    acc = hipctx.accumulator(W, H)
    e = ref_error(mixed_stream(acc, rng, W, H), W, H)
    s = check_plan(acc, e, 0)
    assert s["planned"] == 0 and s["active"] > 0
    active = s["active"]
    check_plan(acc, e, active // 3)                              # fewer samples than active pixels
    s = check_plan(acc, e, 50 * N)                               # the cap binds
    assert N < s["planned"] < 50 * N
    check_plan(acc, e, 50 * N, max_per_pixel=65535)
    for off in (0, 7, (1 << 63) + 5):
        check_plan(acc, e, N + 17, offset=off)
    s = check_plan(acc, e, 3 * N, threshold=1e30)                # only the e = inf pixels stay active
    assert s["active"] == s["unsampled"] > 0 and s["max_error"] == 0.0
    check_plan(acc, e, N, threshold=float(np.median(e[np.isfinite(e)])))
    acc.close()
    dense = hipctx.accumulator(W, H)                             # every e finite; a threshold above them all: T = 0, Q = 0
    parts = []
    for k in range(3):
        p = random_samples(rng, (H, W, 1, 3))
        dense.add_dense(dev(p))
        parts.append(dense_stream(p, None))
    e1 = ref_error(np.concatenate(parts, 0), W, H)
    assert np.all(np.isfinite(e1))
    s = check_plan(dense, e1, 3 * N, threshold=float(e1.max()))
    assert s == {"planned": 0, "active": 0, "unsampled": 0, "max_error": 0.0}
    dense.close()
    fresh = hipctx.accumulator(W, H)                             # every pixel unsampled
    e0 = np.full((H, W), np.inf, np.float32)
    s = check_plan(fresh, e0, 2 * N + 3, offset=5)
    assert s["unsampled"] == N and s["max_error"] == 0.0
    fresh.close()


@pytest.mark.parametrize("W,H", [(1, 1), (67, 13), (1920, 1080)])
def test_plan_odd_sizes(hipctx, W, H):
    N = W * H
    rng = np.random.default_rng(W)
    acc = hipctx.accumulator(W, H, capacity=1 << 20)
    parts = []
    for k in range(3):
        p = random_samples(rng, (H, W, 1, 3))
        acc.add_dense(dev(p))
        parts.append(dense_stream(p, None))
    e = ref_error(np.concatenate(parts, 0), W, H)
    for B, off in ((N, 0), (5 * N + 1, 3), (max(1, N // 7), 11)):
        check_plan(acc, e, B, offset=off)
    acc.close()


def test_plan_is_non_destructive_repeatable_and_validated(hipctx):
    import bcd_amd.hip as bh
    import torch
    W, H = 64, 40
    rng = np.random.default_rng(3)
    acc = hipctx.accumulator(W, H, capacity=2048)
    mixed_stream(acc, rng, W, H)
    before = host(acc.statistics())
    a = acc.plan(3 * W * H, offset=9, error=True)
    b = acc.plan(3 * W * H, offset=9, error=True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert a[3] == b[3]
    for x, y in zip(before, host(acc.statistics())):
        assert bits_equal(x, y)

    L = bh.lib()
    N, B = W * H, 100
    err = torch.full((N,), -2.0, device="cuda")
    cnt = torch.full((N,), -3, dtype=torch.int32, device="cuda")
    pix = torch.full((B,), -4, dtype=torch.int32, device="cuda")
    summ = torch.full((4,), -5, dtype=torch.int64, device="cuda")
    keep = [t.clone() for t in (err, cnt, pix, summ)]
    ok = bh.default_plan_params()
    dp = lambda t: C.c_void_p(t.data_ptr())
    ds = lambda t: C.cast(dp(t), C.POINTER(bh.PlanSummary))      # (the summary lives on the device: its address as the prototype's struct pointer)
    cases = [(None, ok, B, dp(pix), B, ds(summ)), (acc.h, None, B, dp(pix), B, ds(summ)), (acc.h, ok, B, None, B, ds(summ)),
             (acc.h, ok, B, dp(pix), B, None), (acc.h, ok, B, dp(pix), B - 1, ds(summ)), (acc.h, ok, -1, dp(pix), B, ds(summ)),
             (acc.h, ok, 1 << 31, dp(pix), 1 << 32, ds(summ))]
    for kw in ({"threshold": float("nan")}, {"threshold": -1.0}, {"threshold": float("inf")}, {"eps": 0.0}, {"eps": float("nan")},
               {"min_samples": float("nan")}, {"min_samples": -1.0}, {"max_per_pixel": 0}, {"max_per_pixel": 65536}):
        cases.append((acc.h, bh.default_plan_params(**kw), B, dp(pix), B, ds(summ)))
    for h, prm, budget, p, cap, s in cases:
        rc = L.bcd_hip_accum_plan(h, C.byref(prm) if prm is not None else None, budget, 0, dp(err), dp(cnt), p, cap, s)
        assert rc == -1
    torch.cuda.synchronize()
    for x, y in zip((err, cnt, pix, summ), keep):
        assert torch.equal(x, y)
    assert L.bcd_hip_accum_plan(acc.h, C.byref(ok), B, 0, dp(err), dp(cnt), dp(pix), B, ds(summ)) == 0
    torch.cuda.synchronize()
    assert int(summ[0]) == B and int(cnt.sum()) == B
    acc.close()


def synthetic_renderer(W, H, seed):
    import torch
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    L = (0.5 + 0.3 * torch.sin(x / 9) * torch.cos(y / 7)).reshape(-1)
    sigma = torch.where(x < W // 2, 0.05, 1.0).reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(seed)

    def draw(pix):
        z = torch.randn(pix.shape[0], generator=g, device="cuda")
        i = pix.long()
        v = L[i] * (1 + sigma[i] * z)
        return v[:, None].expand(-1, 3).contiguous()
    return L, draw


@pytest.mark.parametrize("seed", [1, 2])
def test_closed_loop_beats_uniform_passes(hipctx, seed):
    """4 spp dense, then 12 passes of W*H samples: planned (default parameters, a new offset each pass) against uniform 1-spp passes"""
    import torch
    W, H = 256, 192
    N = W * H
    every = torch.arange(N, device="cuda", dtype=torch.int32)
    results = {}
    for mode in ("adaptive", "uniform"):
        L, draw = synthetic_renderer(W, H, seed)
        acc = hipctx.accumulator(W, H, capacity=N)
        for k in range(4):
            acc.add_dense(draw(every).reshape(H, W, 1, 3))
        added = torch.zeros(N, dtype=torch.int64, device="cuda")
        for it in range(12):
            if mode == "adaptive":
                pix, counts, _, summ = acc.plan(N, offset=it)
                assert summ["planned"] == pix.shape[0] and summ["unsampled"] == 0
                added += counts.reshape(-1)
                acc.add_samples(pix, draw(pix))
            else:
                added += 1
                acc.add_dense(draw(every).reshape(H, W, 1, 3))
        mean = acc.statistics()[1][..., 0].reshape(-1)
        rms = float(torch.sqrt(torch.mean(((mean - L) / L) ** 2)))
        a = added.reshape(H, W)
        results[mode] = (rms, float(a[:, W // 2:].sum()) / float(a[:, :W // 2].sum()))
        acc.close()
    assert results["adaptive"][1] >= 8.0, results
    assert results["adaptive"][0] <= 0.92 * results["uniform"][0], results


def test_adaptive_snapshot_into_the_denoiser(hipctx):
    """8 spp dense, then planned passes: the snapshot (every pixel >= 8 samples, uneven counts) -> Context.denoise, against the oracle"""
    import bcd_amd.hip as bh
    W, H = 96, 64
    N = W * H
    samples, _ = ol.synth_samples(W, H, 8, seed=31, sigma=0.3, spike_prob=0.0)
    rgb = samples[:, 2:5].reshape(H, W, 8, 3)
    extra, _ = ol.synth_samples(W, H, 8, seed=32, sigma=0.3, spike_prob=0.0)
    extra = extra[:, 2:5].reshape(N, 8, 3)
    acc = hipctx.accumulator(W, H)
    acc.add_dense(dev(rgb))
    for it in range(3):
        pix, _, _, _ = acc.plan(N // 2, offset=it, max_per_pixel=4)
        p = pix.cpu().numpy()
        j = (np.arange(p.size) + it) % 8
        acc.add_samples(pix, dev(np.ascontiguousarray(extra[p, j])))
    ns, mean, cov, hist = acc.statistics()
    prm = bh.default_params(m=1.0, random_order=1, seed=3)
    got = hipctx.denoise(mean, ns, hist, cov, 3, prm).cpu().numpy()
    c, n, h, v = host((mean, ns, hist, cov))
    assert n.min() >= 8 and len(np.unique(n)) > 2
    orders, w_, h_ = [], W, H
    for s in range(3):
        orders.append(bh.visit_order(w_, h_, 1, 1, bh.scale_seed(3, s)))
        w_, h_ = w_ // 2, h_ // 2
    want = ol.denoise_multiscale(c, n, h, v, 3, ol.params(m=1.0), orders=orders)
    assert float(np.max(np.abs(got - want)) / np.max(np.abs(want))) < TOL
    acc.close()


def test_cpp_plan_equals_the_python_plan(hipctx):
    """DeviceSamplesAccumulator::planSamples with every sample still in the addSample buffer, against Accumulator.plan on the same stream"""
    import bcd_amd.core as core
    W, H = 60, 40
    samples, _ = ol.synth_samples(W, H, 6, seed=12, sigma=0.5, spike_prob=0.02)
    rng = np.random.default_rng(12)
    samples = np.ascontiguousarray(samples[rng.permutation(samples.shape[0])][: samples.shape[0] - 500])
    samples[::7, 5] = 2.0
    pixel = (samples[:, 0].astype(np.int64) * W + samples[:, 1].astype(np.int64)).astype(np.int32)
    acc = hipctx.accumulator(W, H)
    acc.add_samples(dev(pixel), dev(samples[:, 2:5]), dev(samples[:, 5]))
    for B, off, K in ((W * H, 4, 16), (7 * W * H, 1, 3)):
        want, want_summ = acc.plan(B, offset=off, max_per_pixel=K)[0::3]
        got, got_summ = core.device_plan(samples, W, H, B, offset=off, max_per_pixel=K)
        assert np.array_equal(got, want.cpu().numpy())
        assert got_summ == want_summ
        # two rejected calls first (a budget of 2^31 with the samples still buffered, then max_per_pixel 0): the next valid call plans
        got, got_summ = core.device_plan(samples, W, H, B, offset=off, max_per_pixel=K, invalid_first=True)
        assert np.array_equal(got, want.cpu().numpy())
        assert got_summ == want_summ
    acc.close()


def test_python_plan_checks_the_budget_first(hipctx):
    W, H = 16, 8
    acc = hipctx.accumulator(W, H)
    acc.add_dense(dev(random_samples(np.random.default_rng(4), (H, W, 3, 3))))
    for budget in (-1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError):
            acc.plan(budget)
    pixels, counts, _, summ = acc.plan(W * H)
    assert summ["planned"] == W * H == int(counts.sum()) == pixels.shape[0]
    acc.close()


def test_closing_the_context_closes_its_accumulators():
    """an accumulator must not outlive its context: Context.close destroys the open ones first, and their own close is then a no-op"""
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    a, b = ctx.accumulator(8, 4), ctx.accumulator(3, 3)
    b.close()
    ctx.close()
    assert a.h is None and b.h is None and ctx.h is None
    a.close()
    del a, b
