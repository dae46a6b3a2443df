#!/usr/bin/env python3
"""GPU box: what several colour layers cost with one shared similar-patch selection (bcd_hip_denoise_layers).
Frames (1920 x 1080, 32 spp, 3 scales, b = 6, as bench.py):  headline (-m 1 -r 1, ramps + checker), textured (pattern 1), m0 (-m 0: every
pixel estimated).  For L = 1, 2, 4, 8:
  layered   one bcd_hip_denoise_layers call over L layers;
  separate  L consecutive bcd_hip_denoise calls (the only route before the layered call existed).
Inputs are resident, every shape is warmed up, a figure is the median of --reps host-clock timings around calls that end in a stream
synchronisation; `spread` is (max - min) / median of those repeats, the noise a difference has to beat.
Copied into a checkout of a commit that has no layered call (the parent, for the "existing path did not slow down" comparison) it measures
`separate` only.
usage: python tools/exp_layers.py [--reps N] [--frames headline,textured,m0] [--layers 1,2,4,8] [--layered-only] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402


def timings(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 4), spread=round(float((t.max() - t.min()) / med), 4), min=round(float(t.min()), 4), max=round(float(t.max()), 4))


def make_layers(col, cov, L):
    """L layers that differ in colour and magnitude: layer 0 is the frame, layer k its samples times a per-channel factor"""
    out = [(col, cov)]
    for k in range(1, L):
        g = np.array([0.9 / k, 0.2 + 0.1 * k, 1.0 / (1 + (k % 3))], np.float32)
        gg = np.array([g[0] * g[0], g[1] * g[1], g[2] * g[2], g[1] * g[2], g[0] * g[2], g[0] * g[1]], np.float32)
        out.append((np.ascontiguousarray(col * g), np.ascontiguousarray(cov * gg)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--frames", default="headline,textured,m0")
    ap.add_argument("--layers", default="1,2,4,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--layered-only", action="store_true", help="skip the separate calls (kernel traces of the layered call alone)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    layered_available = hasattr(bh.lib(), "bcd_hip_denoise_layers")
    ctx = bh.Context(0)
    W, H, S = a.width, a.height, 3
    counts = [int(x) for x in a.layers.split(",")]
    frames = {"headline": dict(pattern=0, m=1.0), "textured": dict(pattern=1, m=1.0), "m0": dict(pattern=0, m=0.0)}
    res = dict(width=W, height=H, scales=S, reps=a.reps, layered_call=layered_available, frames={})
    for name in a.frames.split(","):
        f = frames[name]
        col, ns, hist, cov = core.synthetic_scene(W, H, 32, 1234, 0.35, 0.01, pattern=f["pattern"])
        prm = bh.default_params(m=f["m"], random_order=1)
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, max(counts))]
        outs = [torch.empty_like(layers[0][0]) for _ in layers]
        reps = a.reps if f["m"] != 0.0 else max(3, a.reps // 3)   # (the -m 0 frame takes ~60 ms per layer)
        rows = {}
        for L in counts:
            def separate():
                for k in range(L):
                    ctx.denoise(layers[k][0], d_ns, d_hist, layers[k][1], S, prm, out=outs[k])
            row = {} if a.layered_only else dict(separate=timings(separate, reps, a.warmup))
            if layered_available:
                def layered():
                    ctx.denoise_layers(d_ns, d_hist, layers[:L], S, prm, outs=outs[:L])
                row["layered"] = timings(layered, reps, a.warmup)
                if "separate" in row:
                    row["speedup"] = round(row["separate"]["ms"] / row["layered"]["ms"], 3)
            rows[str(L)] = row
            print(name, "L=%d" % L, json.dumps(row), flush=True)
        res["frames"][name] = rows
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
