#!/usr/bin/env python3
"""GPU box: what the spike prefilter costs as a source map and a gather (bcd_hip_spike_map / _apply / _filter_layers) against
bcd_hip_spike_filter on the same frame in the same run.
Frames: the synthetic scene at 1920 x 1080 and 3840 x 2160 (16 spp, 20 bins: D = 60), factor 2.  Per frame:
  map            bcd_hip_spike_map alone (with the moved counter)                                        108 B read (L2 serves the overlap) + 4 B written per pixel
  apply_d<k>     bcd_hip_spike_apply of one image of depth 1, 3, 6, 60                                   4 + 8 k B per pixel
  spike_filter   bcd_hip_spike_filter (k_spike: decision and copies in one kernel)
and for L = 1 and 4 layers:
  filter_layers          bcd_hip_spike_filter_layers with histograms   (at L = 1 it moves what k_spike moves, plus 8 B per pixel of map)
  filter_layers_moments  the same with d_histograms = NULL: sample counts, means and covariances only
Inputs and outputs are resident and allocated once; a figure is the median of --reps host-clock timings around ten enqueues that end in one
synchronisation, divided by ten; `spread` is (max - min) / median of those repeats.
usage: python tools/exp_spike_layers.py [--reps N] [--sizes 1920x1080,3840x2160] [--layers 1,4] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import make_layers, timings  # noqa: E402

VP = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--layers", default="1,4")
    ap.add_argument("--factor", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    L_ = bh.lib()
    ctx = bh.Context(0)
    counts = [int(x) for x in a.layers.split(",")]
    res = dict(library=bh.LIB_PATH, reps=a.reps, factor=a.factor, frames={})

    def per_call(fn):
        t = timings(lambda: [fn() for _ in range(10)], a.reps, a.warmup)
        return dict(ms=round(t["ms"] / 10, 5), spread=t["spread"], min=round(t["min"] / 10, 5), max=round(t["max"] / 10, 5))

    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        n = W * H
        col, ns, hist, cov = core.synthetic_scene(W, H, 16, 1234, 0.35, 0.01)
        D = hist.shape[-1]
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, max(counts))]
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        o_ns, o_hist = torch.empty_like(d_ns), torch.empty_like(d_hist)
        outs = [(torch.empty_like(c), torch.empty_like(v)) for c, v in layers]
        d_map = torch.empty((H, W), dtype=torch.int32, device="cuda")
        d_moved = torch.zeros(1, dtype=torch.int32, device="cuda")
        p = lambda t: t.data_ptr()
        chk = ctx._chk
        row = {}
        row["map"] = per_call(lambda: chk(L_.bcd_hip_spike_map(ctx.h, p(layers[0][0]), W, H, a.factor, p(d_map), p(d_moved))))
        row["moved_share"] = round(int(d_moved.item()) / n, 5)
        for depth, src, dst in ((1, d_ns, o_ns), (3, layers[0][0], outs[0][0]), (6, layers[0][1], outs[0][1]), (D, d_hist, o_hist)):
            s, d = (VP * 1)(p(src)), (VP * 1)(p(dst))
            r = per_call(lambda: chk(L_.bcd_hip_spike_apply(ctx.h, p(d_map), W, H, depth, s, d, 1)))
            r["GBps"] = round(n * (4 + 8 * depth) / (r["ms"] * 1e-3) / 1e9, 1)
            row["apply_d%d" % depth] = r
        c0, v0 = layers[0]
        row["spike_filter"] = per_call(lambda: chk(L_.bcd_hip_spike_filter(ctx.h, p(c0), p(d_ns), p(d_hist), p(v0), W, H, D, a.factor, p(outs[0][0]), p(o_ns),
                                                                           p(o_hist), p(outs[0][1]))))
        row["spike_filter"]["GBps"] = round(n * (108 + 8 * (10 + D)) / (row["spike_filter"]["ms"] * 1e-3) / 1e9, 1)
        for L in counts:
            arr = (bh.SpikeLayer * L)()
            for k in range(L):
                arr[k].d_colors, arr[k].d_covariances, arr[k].d_colors_out, arr[k].d_covariances_out = p(layers[k][0]), p(layers[k][1]), p(outs[k][0]), p(outs[k][1])
            full = per_call(lambda: chk(L_.bcd_hip_spike_filter_layers(ctx.h, p(d_ns), p(d_hist), W, H, D, a.factor, p(o_ns), p(o_hist), arr, L, p(d_map), None)))
            part = per_call(lambda: chk(L_.bcd_hip_spike_filter_layers(ctx.h, p(d_ns), None, W, H, D, a.factor, p(o_ns), None, arr, L, p(d_map), None)))
            row["L%d" % L] = dict(filter_layers=full, filter_layers_moments=part, ratio=round(full["ms"] / part["ms"], 2))
        row["spike_filter_again"] = per_call(lambda: chk(L_.bcd_hip_spike_filter(ctx.h, p(c0), p(d_ns), p(d_hist), p(v0), W, H, D, a.factor, p(outs[0][0]), p(o_ns),
                                                                                 p(o_hist), p(outs[0][1]))))   # (the same call after the others: drift of the visit)
        if "L1" in row:
            row["L1_vs_spike_filter"] = round(row["L1"]["filter_layers"]["ms"] / row["spike_filter"]["ms"], 3)
        res["frames"][size] = row
        print(size, json.dumps(row), flush=True)
        del layers, outs, d_ns, d_hist, o_ns, o_hist, d_map
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
