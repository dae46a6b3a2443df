#!/usr/bin/env python3
"""GPU box: what the selection from means and covariances costs and how well it denoises (bcd_hip_denoise_moments; DESIGN.md section 14,
docs/EXPERIMENTS.md section 18).
Timing, at 1920 x 1080 and 3840 x 2160 (32 spp, 3 scales, b = 6, -m 1 -r 1, as bench.py), resident inputs, every shape warmed up, a figure is the median
of --reps host-clock timings around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats:
  denoise / layers4     bcd_hip_denoise and bcd_hip_denoise_layers (4 layers): the existing calls
  moments1 / moments4   bcd_hip_denoise_moments with 1 and 4 layers
  pairdist_moments      the new distance kernel alone at full resolution, by the library's events (bcd_hip_kernel_time around the stage call): ms, and
                        the bytes it stores (5 per plane entry whose neighbour is inside the image) over that time
With a library that has no moments entry points (BCD_HIP_LIB pointing at a build of the parent commit: run the two alternately in one visit) only the two
existing calls are measured.
Quality (--quality), on the synthetic scene against its noise-free signal, 960 x 540, 3 scales, at 4, 16 and 64 spp: RMSE of the noisy input, of
bcd_hip_denoise at tau = 1, and of bcd_hip_denoise_moments at tau in {1, 1.5, 2}.
usage: python tools/exp_moments.py [--reps N] [--sizes 1920x1080,3840x2160] [--no-timing] [--quality] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import make_layers, timings  # noqa: E402


def stored_bytes(W, H, b):
    n = 0
    for dl in range(b + 1):
        for dc in range(0 if dl == 0 else -b, b + 1):
            n += (H - dl) * (W - abs(dc))
    return 5 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--var-floor", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    have = hasattr(bh.lib(), "bcd_hip_denoise_moments")
    ctx = bh.Context(0)
    S, b = 3, 6
    res = dict(library=bh.LIB_PATH, moments_calls=have, reps=a.reps, timing={}, quality={})
    for size in ([] if a.no_timing else a.sizes.split(",")):
        W, H = (int(x) for x in size.split("x"))
        col, ns, hist, cov = core.synthetic_scene(W, H, 32, 1234, 0.35, 0.01)
        prm = bh.default_params(m=1.0, random_order=1)
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, 4)]
        outs = [torch.empty_like(layers[0][0]) for _ in layers]
        row = {}
        row["denoise"] = timings(lambda: ctx.denoise(layers[0][0], d_ns, d_hist, layers[0][1], S, prm, out=outs[0]), a.reps, a.warmup)
        row["layers4"] = timings(lambda: ctx.denoise_layers(d_ns, d_hist, layers, S, prm, outs=outs), a.reps, a.warmup)
        if have:
            row["moments1"] = timings(lambda: ctx.denoise_moments(d_ns, layers[:1], S, prm, a.var_floor, outs=outs[:1]), a.reps, a.warmup)
            row["moments1_stats"] = [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total, path=s.similarity_path)
                                     for s in (ctx.stats(k) for k in range(S))]
            row["moments4"] = timings(lambda: ctx.denoise_moments(d_ns, layers, S, prm, a.var_floor, outs=outs), a.reps, a.warmup)
            pixcov = ctx.pixel_cov(layers[0][1], d_ns)
            ms = []
            for _ in range(a.warmup + a.reps):
                ctx.reset_kernel_time()
                ctx.similarity_masks_moments(layers[0][0], pixcov, 1, b, 1.0, a.var_floor)
                t, n = ctx.kernel_time()
                assert n == 1
                ms.append(t)
            ms = np.array(ms[a.warmup:])
            med = float(np.median(ms))
            nbytes = stored_bytes(W, H, b)
            row["pairdist_moments"] = dict(ms=round(med, 4), min=round(float(ms.min()), 4), max=round(float(ms.max()), 4), stored_bytes=nbytes,
                                           stored_GBps=round(nbytes / (med * 1e-3) / 1e9, 1))
            row["denoise_again"] = timings(lambda: ctx.denoise(layers[0][0], d_ns, d_hist, layers[0][1], S, prm, out=outs[0]), a.reps, 1)   # (drift of the visit)
        res["timing"][size] = row
        print(size, json.dumps(row), flush=True)
        del d_ns, d_hist, layers, outs
    if a.quality and have:
        W, H = 960, 540
        truth = core.synthetic_scene(W, H, 1, 1234, 0.0, 0.0)[0].astype(np.float64)
        rmse = lambda x: float(np.sqrt(np.mean((x.astype(np.float64) - truth) ** 2)))
        for spp in (4, 16, 64):
            col, ns, hist, cov = core.synthetic_scene(W, H, spp, 1234, 0.35, 0.0)
            d = [torch.from_numpy(x).cuda() for x in (col, ns, hist, cov)]
            row = dict(input=round(rmse(col), 6))
            prm = bh.default_params(m=1.0, random_order=1, tau=1.0)
            row["histogram_tau1"] = round(rmse(ctx.denoise(*d, S, prm).cpu().numpy()), 6)
            row["histogram_similar_per_pixel"] = round(ctx.stats(0).similar_total / max(1, ctx.stats(0).processed), 1)
            for tau in (1.0, 1.5, 2.0):
                prm = bh.default_params(m=1.0, random_order=1, tau=tau)
                out = ctx.denoise_moments(d[1], [(d[0], d[3])], S, prm, a.var_floor)[0].cpu().numpy()
                row["moments_tau%g" % tau] = round(rmse(out), 6)
                row["moments_tau%g_similar_per_pixel" % tau] = round(ctx.stats(0).similar_total / max(1, ctx.stats(0).processed), 1)
            res["quality"][str(spp)] = row
            print("quality %d spp" % spp, json.dumps(row), flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
