#!/usr/bin/env python3
"""GPU box: what the feature gate of the similar-patch selection costs (bcd_hip_denoise_guided; DESIGN.md section 15, docs/EXPERIMENTS.md section 19).
At 1920 x 1080 and 3840 x 2160 (32 spp, 3 scales, b = 6, -m 1 -r 1, as bench.py), resident inputs, every shape warmed up, a figure is the median of
--reps host-clock timings around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats:
  denoise / layers4          bcd_hip_denoise and bcd_hip_denoise_layers (4 layers): the existing calls
  guided1_f7 / guided4_f7    bcd_hip_denoise_guided with 1 and 4 layers, F = 7 feature channels, no variances (floors 0.01)
  guided1_f3v / guided4_f3v  the same with F = 3 and variances (floors 1e-4)
  moments1 / guided_moments1_f7   bcd_hip_denoise_moments and bcd_hip_denoise_guided without histograms, one layer
  pairdist_guide_f7 / _f3v   the new distance kernel alone at full resolution, by the library's events (bcd_hip_kernel_time around the stage call): ms,
                             and the bytes it stores (5 per plane entry whose neighbour is inside the image) over that time
  gate_stage_f7 / _f3v       the whole stage the gate adds to a scale -- distance kernel, mask kernels, AND kernel -- by the host clock around
                             similarity_masks_guide + gate_masks at full resolution
With a library that has no guided entry points (BCD_HIP_LIB pointing at a build of the parent commit: run the two alternately in one visit) only the two
existing calls are measured.
usage: python tools/exp_guided.py [--reps N] [--sizes 1920x1080,3840x2160] [--out FILE.json]"""
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
from exp_moments import stored_bytes  # noqa: E402


def features(W, H, F, seed=1):
    """F feature channels of a frame: two regions split along a slanted line, a smooth term, noise of sigma 0.05 in the mean; and the variance of that mean"""
    rng = np.random.default_rng(seed)
    l, c = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    second = ((c - l // 3) >= W // 3).astype(np.float32)
    k = np.arange(F, dtype=np.float32)
    f = (0.2 + 0.1 * k) + second[..., None] * np.where(k % 2 == 0, 0.3, -0.15).astype(np.float32) + 0.02 * np.sin((l + 2 * c)[..., None] / 9.0 + k)
    f = f.astype(np.float32) + 0.05 * rng.standard_normal((H, W, F), dtype=np.float32)
    v = (0.0025 * (0.6 + 0.8 * rng.random((H, W, F), dtype=np.float32))).astype(np.float32)
    return np.ascontiguousarray(f, np.float32), v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    have = hasattr(bh.lib(), "bcd_hip_denoise_guided")
    ctx = bh.Context(0)
    S, b = 3, 6
    res = dict(library=bh.LIB_PATH, guided_calls=have, reps=a.reps, timing={})
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        col, ns, hist, cov = core.synthetic_scene(W, H, 32, 1234, 0.35, 0.01)
        prm = bh.default_params(m=1.0, random_order=1)
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, 4)]
        outs = [torch.empty_like(layers[0][0]) for _ in layers]
        stats = lambda: [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total, path=s.similarity_path) for s in (ctx.stats(k) for k in range(S))]
        row = {}
        row["denoise"] = timings(lambda: ctx.denoise(layers[0][0], d_ns, d_hist, layers[0][1], S, prm, out=outs[0]), a.reps, a.warmup)
        row["denoise_stats"] = stats()
        row["layers4"] = timings(lambda: ctx.denoise_layers(d_ns, d_hist, layers, S, prm, outs=outs), a.reps, a.warmup)
        if have:
            guides = {}
            f7, _ = features(W, H, 7)
            f3, v3 = features(W, H, 3)
            guides["f7"] = (torch.from_numpy(f7).cuda(), None, [0.01] * 7)
            guides["f3v"] = (torch.from_numpy(f3).cuda(), torch.from_numpy(v3).cuda(), [1e-4] * 3)
            for name, (d_f, d_v, fl) in guides.items():
                row["guided1_" + name] = timings(lambda: ctx.denoise_guided(d_ns, d_hist, layers[:1], S, prm, d_f, d_v, fl, 1.0, outs=outs[:1]), a.reps, a.warmup)
                row["guided1_%s_stats" % name] = stats()
                row["guided4_" + name] = timings(lambda: ctx.denoise_guided(d_ns, d_hist, layers, S, prm, d_f, d_v, fl, 1.0, outs=outs), a.reps, a.warmup)
                ms = []
                for _ in range(a.warmup + a.reps):
                    ctx.reset_kernel_time()
                    ctx.similarity_masks_guide(d_f, d_v, fl, 1.0, 1, b)
                    t, n = ctx.kernel_time()
                    assert n == 1
                    ms.append(t)
                ms = np.array(ms[a.warmup:])
                med = float(np.median(ms))
                nbytes = stored_bytes(W, H, b)
                row["pairdist_guide_" + name] = dict(ms=round(med, 4), min=round(float(ms.min()), 4), max=round(float(ms.max()), 4), stored_bytes=nbytes,
                                                     stored_GBps=round(nbytes / (med * 1e-3) / 1e9, 1))
                mask, cnt = ctx.similarity_masks(d_hist, d_ns, 1, b, 1.0)
                ctx.synchronize()

                def stage():
                    gate, _ = ctx.similarity_masks_guide(d_f, d_v, fl, 1.0, 1, b)
                    ctx.gate_masks(mask, cnt, gate, b)
                row["gate_stage_" + name] = timings(stage, a.reps, a.warmup)
                del mask, cnt
            row["moments1"] = timings(lambda: ctx.denoise_moments(d_ns, layers[:1], S, prm, 1e-8, outs=outs[:1]), a.reps, a.warmup)
            d_f, d_v, fl = guides["f7"]
            row["guided_moments1_f7"] = timings(lambda: ctx.denoise_guided(d_ns, None, layers[:1], S, prm, d_f, d_v, fl, 1.0, outs=outs[:1]), a.reps, a.warmup)
            row["denoise_again"] = timings(lambda: ctx.denoise(layers[0][0], d_ns, d_hist, layers[0][1], S, prm, out=outs[0]), a.reps, 1)   # (drift of the visit)
            row["layers4_again"] = timings(lambda: ctx.denoise_layers(d_ns, d_hist, layers, S, prm, outs=outs), a.reps, 1)
            del guides, d_f, d_v
        res["timing"][size] = row
        print(size, json.dumps(row), flush=True)
        del d_ns, d_hist, layers, outs
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
