#!/usr/bin/env python3
"""GPU box: the accumulator's feature channels (bcd_hip_accum_*_features) at 1080p with F = 7 channels (albedo, normal, depth), random
values.  HIP events after warm-up, medians of `--reps` (at least 15) with the quartiles as the spread, the routes alternating in one process:
  (1) the 1-spp dense pass, a scattered add of 1 M samples and a 1-spp splat through a Gaussian of radius 1.5 on an accumulator with the
      features, beside the same adds on one without: the feature part is the difference; bytes per pixel and rate for the dense pass;
  (2) the feature snapshot;
  (3) the route without the feature: the 7 channels pushed in triples as 3 colour layers (bcd_hip_accum_create_layers), layer_statistics
      and moments for the snapshot, and a pointwise pass for the variance of the mean;
  (4) with --parent-lib: bcd_hip_accum_add_dense, _add_dense_layers (L = 4) and _add_splatted of this build beside another build of the
      library (the commit before), in child processes that take turns (a process loads one library).
The byte counts are what each route must move, computed from the shapes; GB/s is that over the measured time.
usage: python tools/exp_accum_features.py [--reps N] [--parent-lib PATH] [--rounds R]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, F = 1920, 1080, 7
N = W * H
DENSE_FEATURES = 20 * F + 4                                   # the feature pass: 4 F sample, 4 weight, 8 F in and 8 F out of the planes
DENSE_LAYER = 12 + 4 + 2 * 9 * 4                              # a layer's pass: sample and weight in; 9 sums read and written
SNAP_FEATURES = 8 + 8 * F + 8 * F                             # two weight sums and 2 F sums read; means and variances written
SNAP_LAYER = (2 + 9) * 4 + 9 * 4                              # two weight sums and 9 sums read; mean, cov written


def alternating(fns, reps, warm=3):
    """(median, lower quartile, upper quartile) ms of each callable, the callables taking turns inside every repeat"""
    import torch
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
    out = []
    for i in range(len(fns)):
        t = [row[i][0].elapsed_time(row[i][1]) for row in ev]
        out.append(tuple(round(float(q), 4) for q in np.percentile(t, [50, 25, 75])))
    return out


def existing_calls(reps):
    """the adds that exist without the feature, on whatever library BCD_HIP_LIB names: median ms and quartiles"""
    import torch
    import bcd_amd.hip as bh
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    plain, lay = ctx.accumulator(W, H, capacity=N), ctx.accumulator(W, H, capacity=N, layers=4)
    plain.set_filter("gaussian", 1.5, param=2.0, table_size=16)
    smp = [torch.rand((H, W, 1, 3), generator=g, device="cuda") * 1.5 for _ in range(5)]
    xy = torch.rand((N, 2), generator=g, device="cuda") * torch.tensor([float(W), float(H)], device="cuda")
    rgb = torch.rand((N, 3), generator=g, device="cuda")
    t = alternating([lambda: plain.add_dense(smp[0]), lambda: lay.add_dense(smp[0], layers=smp[1:]), lambda: plain.add_splatted(xy, rgb)], reps)
    torch.cuda.synchronize()
    plain.close()
    lay.close()
    ctx.close()
    return dict(zip(("add_dense", "add_dense_layers_L4", "add_splatted"), t))


def features(reps):
    import torch
    import bcd_amd.hip as bh
    ctx = bh.Context(0, torch.cuda.current_stream())
    g = torch.Generator(device="cuda").manual_seed(1)
    n = 1 << 20
    feat, plain, lay = ctx.accumulator(W, H, capacity=N, features=F), ctx.accumulator(W, H, capacity=N), ctx.accumulator(W, H, capacity=N, layers=3)
    for acc in (feat, plain, lay):
        acc.set_filter("gaussian", 1.5, param=2.0, table_size=16)
    rnd = lambda *shape: torch.rand(shape, generator=g, device="cuda")
    smp, x = rnd(H, W, 1, 3) * 1.5, rnd(H, W, 1, F)
    pix = torch.randint(0, N, (n,), generator=g, device="cuda", dtype=torch.int32)
    rgb, xs, w = rnd(n, 3), rnd(n, F), rnd(n) + 0.5
    xy = rnd(N, 2) * torch.tensor([float(W), float(H)], device="cuda")
    srgb, sx = rnd(N, 3), rnd(N, F)
    # the route without the feature: the channels in triples, the last triple padded
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (9 - F,), device="cuda")], -1)
    triples = lambda t: [pad(t)[..., 3 * k:3 * k + 3].contiguous() for k in range(3)]
    x3, xs3, sx3 = triples(x), triples(xs), triples(sx)
    out_f = feat.feature_statistics()
    out_l, out_m = lay.layer_statistics(), lay.moments()
    var = [torch.empty_like(m) for m, _ in out_l]

    def layer_snapshot():
        lay.layer_statistics(out_l)
        lay.moments(out_m)
        for k, (_, c) in enumerate(out_l):                    # unit weights: the variance of the mean is the variance over n
            torch.clamp(c[..., :3] / out_m[0], min=0, out=var[k])

    res = {"frame": [W, H], "features": F, "reps": reps}
    names = ("with_features", "without", "as_3_layers")
    for name, fns in {
        "dense_1spp": (lambda: feat.add_dense(smp, features=x), lambda: plain.add_dense(smp), lambda: lay.add_dense(smp, layers=x3)),
        "scattered_1M": (lambda: feat.add_samples(pix, rgb, w, features=xs), lambda: plain.add_samples(pix, rgb, w), lambda: lay.add_samples(pix, rgb, w, layers=xs3)),
        "splat_1spp_gauss1.5": (lambda: feat.add_splatted(xy, srgb, features=sx), lambda: plain.add_splatted(xy, srgb), lambda: lay.add_splatted(xy, srgb, layers=sx3)),
    }.items():
        t = alternating(fns, reps)
        row = {k: {"ms": v[0], "quartiles": v[1:]} for k, v in zip(names, t)}
        row["feature_part_ms"] = round(t[0][0] - t[1][0], 4)
        row["layer_part_ms"] = round(t[2][0] - t[1][0], 4)
        if name == "dense_1spp":
            row["feature_part_bytes_per_pixel"], row["layer_part_bytes_per_pixel"] = DENSE_FEATURES, 3 * DENSE_LAYER
            row["feature_part_GBps"] = round(N * DENSE_FEATURES / max(row["feature_part_ms"], 1e-6) / 1e6, 1)
            row["layer_part_GBps"] = round(N * 3 * DENSE_LAYER / max(row["layer_part_ms"], 1e-6) / 1e6, 1)
        res[name] = row
    t = alternating([lambda: feat.feature_statistics(out_f), layer_snapshot], reps)
    res["snapshot"] = {"features": {"ms": t[0][0], "quartiles": t[0][1:], "bytes_per_pixel": SNAP_FEATURES,
                                    "GBps": round(N * SNAP_FEATURES / t[0][0] / 1e6, 1)},
                       "as_3_layers": {"ms": t[1][0], "quartiles": t[1][1:], "bytes_per_pixel_of_layer_statistics": 3 * SNAP_LAYER}}
    res["state_bytes"] = {"features": feat.features_state_bytes(), "as_3_layers": lay.layers_state_bytes()}
    torch.cuda.synchronize()
    for acc in (feat, plain, lay):
        acc.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent-lib", default=None, help="libbcd_hip.so of the commit before, for (4)")
    ap.add_argument("--rounds", type=int, default=2, help="turns each library takes in (4)")
    ap.add_argument("--child-existing", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    reps = max(15, a.reps)
    if a.child_existing:
        print(json.dumps(existing_calls(reps)))
        return
    res = features(reps)
    if a.parent_lib:
        turns = []
        for _ in range(max(1, a.rounds)):
            for build, lib in (("this", None), ("parent", os.path.abspath(a.parent_lib))):
                env = dict(os.environ)
                env.pop("BCD_HIP_LIB", None)
                if lib:
                    env["BCD_HIP_LIB"] = lib
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-existing", "--reps", str(reps)], env=env, capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("the %s build's child failed:\n%s" % (build, r.stderr[-2000:]))
                turns.append({"build": build, **json.loads(r.stdout.strip().splitlines()[-1])})
        res["existing_calls"] = turns
    print(json.dumps(res))


if __name__ == "__main__":
    main()
