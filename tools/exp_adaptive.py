#!/usr/bin/env python3
"""GPU box: adaptive sample planning (bcd_hip_accum_plan) timed with HIP events after warm-up, median of repeats, at 1080p and 4K for
budgets of 1 and 8 samples per pixel; the accumulator holds 4 dense spp of noisy colours, so every pixel is active.  Reports ms, the bytes
the plan must move (PLAN_BYTES_PER_PIXEL per pixel + 4 per planned sample) and that traffic as GB/s and as a share of
the HBM bound.  A budget of 0 runs every kernel but the expansion.  For the per-kernel split, run it under
`rocprofv3 --kernel-trace --stats`.
usage: python tools/exp_adaptive.py [--reps N] [--hbm-gbps 8000]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402

# error pass 44 in + 4 out; scan of q 4 in + 8 out; counts 8 in (C_p, C_{p-1} of the same line) + 4 out; scan of the counts 4 + 4;
# expansion 4 in (the ends) -- plus 4 B per planned sample
PLAN_BYTES_PER_PIXEL = 48 + 12 + 12 + 8 + 4


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0, help="HBM bandwidth the share is taken of (MI355X: 8 TB/s)")
    a = ap.parse_args()
    # the plan runs on the context's stream; bind it to torch's current stream so that the events bracket it
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    L = bh.lib()
    prm = bh.default_plan_params()
    res = {}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        N = W * H
        acc = ctx.accumulator(W, H, capacity=1 << 20)
        acc.add_dense((torch.rand((H, W, 4, 3), generator=g, device="cuda") * 1.5).contiguous())
        err = torch.empty((H, W), dtype=torch.float32, device="cuda")
        counts = torch.empty((H, W), dtype=torch.int32, device="cuda")
        summ = torch.empty((4,), dtype=torch.int64, device="cuda")
        for spp in (0, 1, 8):
            B = spp * N
            pixels = torch.empty((max(B, 1),), dtype=torch.int32, device="cuda")
            args = (acc.h, C.byref(prm), B, 0, C.c_void_p(err.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(pixels.data_ptr()),
                    pixels.numel(), C.cast(C.c_void_p(summ.data_ptr()), C.POINTER(bh.PlanSummary)))

            def run():
                assert L.bcd_hip_accum_plan(*args) == 0
            ms = timed(run, a.reps)
            torch.cuda.synchronize()
            T = int(summ[0])
            nbytes = N * PLAN_BYTES_PER_PIXEL + 4 * T
            res["plan_%dspp_%s" % (spp, name)] = {"ms": round(ms, 4), "planned": T, "GBps": round(nbytes / ms / 1e6, 1),
                                                   "hbm_share": round(nbytes / ms / 1e6 / a.hbm_gbps, 3)}
            del pixels
        acc.close()
        del err, counts
    torch.cuda.synchronize()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
