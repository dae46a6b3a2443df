#!/usr/bin/env python3
"""GPU box: the five layer-batched streaming kernels of bcd_hip_denoise_layers (per-pixel covariances + cleared sums, finalisation, colour and covariance
pyramid reducers, merge) through their stage calls, on L layers of independent content: BIT FOR BIT against the single-image stage calls, and through those
against the CPU oracle (pinned to the reference's compiled units for these stages; the finalisation, which the oracle has no operation for, against its
float32 expression (1 / count) * sum).  Sample counts and count-image entries of zero are part of every case: the inf / NaN patterns must agree too.
Test infrastructure: tests/test_gpu_layers_stage.py imports check_case / geometries.  usage: python tools/fuzz_layers_streaming.py [n_cases] [seed]"""
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import oracle_lib as ol  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))


def geometries(n_cases, seed):
    """seeded (W, H, L, case seed): sizes from 4 x 4 up (as tools/fuzz_streaming.py), every layer count of the ABI"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(4, 200)), int(rng.integers(4, 140)), int(rng.integers(1, 17)), int(rng.integers(1, 1 << 30))) for _ in range(n_cases)]


def layer_images(W, H, L, seed):
    """L layers of independent content at scales 2^-8 ... 2^8, shared sample counts and a count image, both with zeros"""
    rng = np.random.default_rng(seed)
    f = lambda *shape: np.ascontiguousarray(rng.standard_normal(shape), np.float32)
    scale = [np.float32(2.0 ** int(rng.integers(-8, 9))) for _ in range(L)]
    col = [f(H, W, 3) * s for s in scale]
    cov = [f(H, W, 6) * s * s for s in scale]
    sums = [f(H, W, 3) * s for s in scale]
    lo = [f(H // 2, W // 2, 3) * s for s in scale]
    ns = rng.choice(np.array([0, 1, 2, 3, 8, 16, 37], np.float32), size=(H, W, 1), p=[0.1, 0.15, 0.15, 0.15, 0.15, 0.15, 0.15])
    cnt = rng.integers(0, 170, size=(H, W)).astype(np.int32)
    cnt[rng.random((H, W)) < 0.1] = 0
    return col, cov, sums, lo, np.ascontiguousarray(ns), cnt


def check_case(ctx, W, H, L, seed):
    """-> names of the stages that differ (empty: every stage bit-exact, layered == single-image == oracle)"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    o = ol.oracle_ops()
    col, cov, sums, lo, ns, cnt = layer_images(W, H, L, seed)
    d_col, d_cov, d_sums, d_lo = [[dev(a) for a in lst] for lst in (col, cov, sums, lo)]
    d_ns, d_cnt = dev(ns), dev(cnt)
    fails = []

    def compare(name, layered, single, oracle):
        for k in range(L):
            got, one = layered[k].cpu().numpy(), single(k).cpu().numpy()
            if not bits_equal(got, one):
                fails.append("%s layer %d: layered != single-image call" % (name, k))
            if not bits_equal(one, oracle(k)):
                fails.append("%s layer %d: single-image call != oracle" % (name, k))

    def pixcov_oracle(k):
        want = np.empty_like(cov[k])
        ol.oracle().bcdo_pixel_cov_from_sample_cov(ol._fp(cov[k]), ol._fp(ns), W, H, ol._fp(want))
        return want

    def finalize_f32(k):
        with np.errstate(all="ignore"):
            return (np.float32(1.0) / cnt.astype(np.float32))[..., None] * sums[k]

    pc, cleared = ctx.layers_pixel_cov(d_cov, d_ns)
    if not bool((cleared.view(torch.int32) == 0).all()):
        fails.append("pixel covariances: sums not cleared to +0")
    compare("pixel covariances", pc, lambda k: ctx.pixel_cov(d_cov[k], d_ns), pixcov_oracle)
    compare("finalize", ctx.layers_finalize(d_sums, d_cnt), lambda k: ctx.finalize(d_sums[k], d_cnt), finalize_f32)
    if W >= 2 and H >= 2:
        compare("downscale_avg", ctx.layers_downscale_avg(d_col), lambda k: ctx.downscale_avg(d_col[k]), lambda k: o["davg"](col[k]))
        compare("downscale_cov", ctx.layers_downscale_cov(d_cov, d_ns), lambda k: ctx.downscale_cov(d_cov[k], d_ns), lambda k: o["dcov"](cov[k], ns))
        compare("merge", ctx.layers_merge(d_col, d_lo), lambda k: ctx.merge(d_col[k], d_lo[k]), lambda k: o["merge"](col[k], lo[k]))
        for k in range(L):                                               # the inputs of the out-of-place wrappers are untouched
            if not bits_equal(d_col[k].cpu().numpy(), col[k]):
                fails.append("merge layer %d: input changed" % k)
    return fails


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    ctx = bh.Context(0)
    t0, bad = time.time(), 0
    for i, (W, H, L, s) in enumerate(geometries(n_cases, seed)):
        fails = check_case(ctx, W, H, L, s)
        bad += 1 if fails else 0
        print("%4d: %3dx%-3d %2d layers  %s" % (i, W, H, L, "bit-exact" if not fails else "DIFFER: " + "; ".join(fails[:4]) + "   <-- MISMATCH"), flush=True)
    print("%d cases, %d mismatches, %.0f s" % (n_cases, bad, time.time() - t0))
    ctx.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
