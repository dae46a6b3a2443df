#!/usr/bin/env python3
"""GPU box: the device SamplesAccumulator (bcd_hip_accum_*) timed with HIP events after warm-up, median of repeats.
  dense 1-spp pass and snapshot at 1080p / 4K: ms and GB/s against the bytes each kernel must move;
  scattered add of 1 M / 8 M samples over a 1080p frame: Msamples/s (run under `rocprofv3 --kernel-trace --stats` for the sort's share);
  --raw: raw2bcd on a 1080p x 64-spp, 3-channel file against the host class on the same samples (1 thread, and 16 through the thread-safe
  variant; sample stream already in memory).
usage: python tools/exp_accumulate.py [--reps N] [--raw DIR]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402

D = 60
DENSE_BYTES_PER_PIXEL = 12 + 2 * 11 * 4 + 2 * 6 * 4          # 3 floats in; 11 sums and the 6 touched bins read and written
SNAPSHOT_BYTES_PER_PIXEL = (11 + D) * 4 + (10 + D) * 4       # state read; ns, mean, cov, hist written


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
    ap.add_argument("--raw", default="")
    a = ap.parse_args()
    # the accumulator runs on the context's stream; bind it to torch's current stream so that the events bracket it
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        N = W * H
        acc = ctx.accumulator(W, H)
        smp = torch.rand((H, W, 1, 3), generator=g, device="cuda") * 1.5
        ms = timed(lambda: acc.add_dense(smp), a.reps)
        out = acc.statistics()
        ms_s = timed(lambda: acc.statistics(out), a.reps)
        res["dense_1spp_" + name] = {"ms": round(ms, 4), "GBps": round(N * DENSE_BYTES_PER_PIXEL / ms / 1e6, 1)}
        res["snapshot_" + name] = {"ms": round(ms_s, 4), "GBps": round(N * SNAPSHOT_BYTES_PER_PIXEL / ms_s / 1e6, 1)}
        smp8 = torch.rand((H, W, 8, 3), generator=g, device="cuda") * 1.5
        ms8 = timed(lambda: acc.add_dense(smp8), max(5, a.reps // 4))
        res["dense_8spp_" + name] = {"ms": round(ms8, 4), "Msamples_per_s": round(8 * N / ms8 / 1e3, 1)}
        acc.close()
        del smp, smp8, out
    W, H = 1920, 1080
    for n in (1 << 20, 8 << 20):
        acc = ctx.accumulator(W, H, capacity=n)
        pix = torch.randint(0, W * H, (n,), generator=g, device="cuda", dtype=torch.int32)
        rgb = torch.rand((n, 3), generator=g, device="cuda")
        w = torch.rand((n,), generator=g, device="cuda") + 0.5
        ms = timed(lambda: acc.add_samples(pix, rgb, w), max(5, a.reps // 2))
        res["scattered_%dM" % (n >> 20)] = {"ms": round(ms, 4), "Msamples_per_s": round(n / ms / 1e3, 1)}
        acc.close()
    torch.cuda.synchronize()
    ctx.close()
    if a.raw:
        W, H, spp = 1920, 1080, 64
        path = os.path.join(a.raw, "frame_1080p_64spp.raw")
        rng = np.random.default_rng(64)
        with open(path, "wb") as f:
            f.write(struct.pack("<5i", 1, W, H, spp, 3))
            for l0 in range(0, H, 60):
                f.write((rng.random((60, W, spp, 3), dtype=np.float32) * 1.5).tobytes())
        exe = os.path.join(ROOT, "bcd_amd", "lib", "raw2bcd")
        t = time.perf_counter()
        r = subprocess.run([exe, path, os.path.join(a.raw, "out")], capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t
        assert r.returncode == 0, r.stderr
        res["raw2bcd_1080p_64spp"] = {"file_GB": round(os.path.getsize(path) / 1e9, 3), "wall_s": round(wall, 3)}
        smp = np.fromfile(path, np.float32, offset=20).reshape(-1, 3)
        pix = np.arange(W * H, dtype=np.int64).repeat(spp)
        stream = np.empty((smp.shape[0], 6), np.float32)
        stream[:, 0], stream[:, 1], stream[:, 2:5], stream[:, 5] = pix // W, pix % W, smp, 1.0
        del smp, pix
        t = time.perf_counter()
        core.accumulate(stream, W, H)
        res["host_class_1thread_s"] = round(time.perf_counter() - t, 3)
        ns, mean, cov, hist = (np.empty((H, W, d), np.float32) for d in (1, 3, 6, D))
        t = time.perf_counter()
        core.lib().bcdcore_accumulate_threadsafe(core._fp(stream), core.C.c_longlong(stream.shape[0]), W, H, 20, core.C.c_float(2.2),
                                                 core.C.c_float(2.5), 16, core._fp(ns), core._fp(mean), core._fp(cov), core._fp(hist))
        res["host_class_16threads_s"] = round(time.perf_counter() - t, 3)
        os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
