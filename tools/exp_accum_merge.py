#!/usr/bin/env python3
"""GPU box: accumulator states (bcd_hip_accum_export / _import / _merge_state / _merge) at 1080p and 4K, 20 bins.
  device merge (k_accum_merge over the whole state): HIP events after warm-up, median of repeats; GB/s of the 12 B per float it must
    move (two reads, one write) and its share of the 6.29 TB/s copy rate docs/EXPERIMENTS.md section 10 uses as its bound;
  export, import and host merge_state: wall time per call from a resident host buffer (PCIe plus the host copy into pinned staging);
  cross-device merge (device 1 into device 0), when two GPUs are visible; otherwise reported as not measured.
usage: python tools/exp_accum_merge.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402

PLANES = 11 + 3 * 20
COPY_RATE = 6.29e12


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


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    # bound to torch's current stream so that the events bracket the merge kernel
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        floats = PLANES * W * H
        dst, src = ctx.accumulator(W, H), ctx.accumulator(W, H)
        for acc in (dst, src):
            acc.add_dense(torch.rand((H, W, 2, 3), generator=g, device="cuda") * 1.5)
        ms = timed(lambda: dst.merge(src), a.reps)
        res["merge_" + name] = {"ms": round(ms, 4), "GBps": round(12 * floats / ms / 1e6, 1),
                                "of_copy_rate": round(12 * floats / (ms * 1e-3) / COPY_RATE, 3),
                                "bound_ms": round(12 * floats / COPY_RATE * 1e3, 4)}
        host_reps = max(3, a.reps // 4)
        st = src.export_state()
        bytes_ = st.size
        ms_e = wall(lambda: src.export_state(), host_reps)
        ms_i = wall(lambda: dst.import_state(st), host_reps)
        ms_m = wall(lambda: dst.merge_state(st), host_reps)
        for k, v in (("export", ms_e), ("import", ms_i), ("merge_state", ms_m)):
            res[k + "_" + name] = {"ms": round(v, 2), "GBps": round(bytes_ / v / 1e6, 2)}
        if torch.cuda.device_count() > 1:
            c1 = bh.Context(1)
            far = c1.accumulator(W, H)
            far.import_state(st)
            ms_x = wall(lambda: dst.merge(far), host_reps)
            res["cross_device_merge_" + name] = {"ms": round(ms_x, 2), "GBps": round(bytes_ / ms_x / 1e6, 2)}
            far.close()
            c1.close()
        else:
            res["cross_device_merge_" + name] = "not measured: one GPU visible"
        res["state_bytes_" + name] = bytes_
        dst.close()
        src.close()
        del st
    ctx.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
