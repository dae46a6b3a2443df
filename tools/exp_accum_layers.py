#!/usr/bin/env python3
"""GPU box: the accumulator's colour layers (bcd_hip_accum_*_layers) against the route without them -- one plain accumulator per layer fed
the same stream -- at 1080p with 4 extra layers, random colours.  HIP events after warm-up, medians of `--reps` (at least 15), the two
routes alternating in one process, the whole comparison made `--runs` times (two by default) so that the repeat-to-repeat spread shows.
  dense 1-spp pass, snapshot, scattered add of 1 M samples, splat of 1 spp through a Gaussian of radius 1.5: ms per route;
  state bytes per route.
The byte counts are what each route must move, computed from the shapes; GB/s is that over the measured time.
usage: python tools/exp_accum_layers.py [--reps N] [--runs R] [--layers L]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402

W, H, D = 1920, 1080, 60
N = W * H
DENSE_FULL = 12 + 2 * 11 * 4 + 2 * 6 * 4                      # a full accumulator pass: sample in; 11 sums and 6 touched bins read and written
DENSE_LAYER = 12 + 2 * 9 * 4                                  # a layer's pass: sample in; 9 sums read and written
SNAP_FULL = (11 + D) * 4 + (10 + D) * 4                       # state read; ns, mean, cov, hist written
SNAP_LAYER = (2 + 9) * 4 + 9 * 4                              # two weight sums and 9 sums read; mean, cov written


def alternating(fns, reps, warm=3):
    """median ms of each callable, the callables taking turns inside every repeat"""
    for _ in range(warm):
        for f in fns:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
    for row in ev:
        for f, (a, b) in zip(fns, row):
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return [float(np.median([row[i][0].elapsed_time(row[i][1]) for row in ev])) for i in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--layers", type=int, default=4)
    a = ap.parse_args()
    reps, L = max(15, a.reps), a.layers
    # the accumulators run on the context's stream; bind it to torch's current stream so that the events bracket them
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    n = 1 << 20
    lay = ctx.accumulator(W, H, capacity=N, layers=L)
    sep = [ctx.accumulator(W, H, capacity=N) for _ in range(L + 1)]
    for acc in [lay] + sep:
        acc.set_filter("gaussian", 1.5, param=2.0, table_size=16)
    smp = [torch.rand((H, W, 1, 3), generator=g, device="cuda") * 1.5 for _ in range(L + 1)]
    pix = torch.randint(0, N, (n,), generator=g, device="cuda", dtype=torch.int32)
    rgb = [torch.rand((n, 3), generator=g, device="cuda") for _ in range(L + 1)]
    w = torch.rand((n,), generator=g, device="cuda") + 0.5
    xy = torch.rand((N, 2), generator=g, device="cuda") * torch.tensor([float(W), float(H)], device="cuda")
    srgb = [torch.rand((N, 3), generator=g, device="cuda") for _ in range(L + 1)]
    out_l, out_ll = lay.statistics(), lay.layer_statistics()
    out_s = [acc.statistics() for acc in sep]

    def snap_layered():
        lay.statistics(out_l)
        lay.layer_statistics(out_ll)

    pairs = {
        "dense_1spp": (lambda: lay.add_dense(smp[0], layers=smp[1:]), lambda: [acc.add_dense(s) for acc, s in zip(sep, smp)]),
        "snapshot": (snap_layered, lambda: [acc.statistics(o) for acc, o in zip(sep, out_s)]),
        "scattered_1M": (lambda: lay.add_samples(pix, rgb[0], w, layers=rgb[1:]), lambda: [acc.add_samples(pix, c, w) for acc, c in zip(sep, rgb)]),
        "splat_1spp_gauss1.5": (lambda: lay.add_splatted(xy, srgb[0], layers=srgb[1:]), lambda: [acc.add_splatted(xy, c) for acc, c in zip(sep, srgb)]),
    }
    bytes_px = {"dense_1spp": (DENSE_FULL + L * DENSE_LAYER, (L + 1) * DENSE_FULL), "snapshot": (SNAP_FULL + L * SNAP_LAYER, (L + 1) * SNAP_FULL)}
    res = {"frame": [W, H], "layers": L, "reps": reps, "runs": []}
    for _ in range(max(1, a.runs)):
        run = {}
        for name, fns in pairs.items():
            r = reps if name in ("dense_1spp", "snapshot") else max(15, reps // 2)
            ms_l, ms_s = alternating(fns, r)
            run[name] = {"layered_ms": round(ms_l, 4), "separate_ms": round(ms_s, 4), "ratio": round(ms_s / ms_l, 3)}
            if name in bytes_px:
                run[name]["layered_GBps"] = round(N * bytes_px[name][0] / ms_l / 1e6, 1)
                run[name]["separate_GBps"] = round(N * bytes_px[name][1] / ms_s / 1e6, 1)
        res["runs"].append(run)
    res["bytes_per_pixel"] = {k: {"layered": v[0], "separate": v[1]} for k, v in bytes_px.items()}
    res["state_bytes"] = {"layered": lay.state_bytes() + lay.layers_state_bytes(), "separate": sum(acc.state_bytes() for acc in sep)}
    torch.cuda.synchronize()
    for acc in [lay] + sep:
        acc.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
