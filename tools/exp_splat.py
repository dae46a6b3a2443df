#!/usr/bin/env python3
"""GPU box: the splatted add (bcd_hip_accum_add_splatted) timed with HIP events on the context's stream after
warm-up, median of repeats, one process.  1080p and 4K, 1 and 8 samples per pixel per batch at jittered positions, filters
(a) box 0.5, (b) Gaussian 1.5 (alpha 2), (c) tent 2.  For each, three numbers:
  splat      the new call;
  parent     the route without it: the footprints expanded on the device by the caller (torch ops, `expand_ms`, timed apart) and
             add_samples of the expanded entries (`parent_ms`); skipped (null) above 2^30 entries, the scattered add's chunk limit;
  floor      add_samples of the n unexpanded samples at their floor pixels: the same sort without the gather.
The first configuration of each filter also checks that the parent route and the new call leave the same nSamples / mean / covariance bits.
One JSON line per configuration goes to stdout and, if given, to --out as soon as it is measured.
usage: python tools/exp_splat.py [--reps N] [--only 1080p:8:gauss] [--out FILE]
(run one configuration under `rocprofv3 --kernel-trace --stats -- python tools/exp_splat.py --only ...` for the kernels' shares)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402

FILTERS = {"box": ("box", (0.5, 0.5), 0.0), "gauss": ("gaussian", (1.5, 1.5), 2.0), "tent": ("tent", (2.0, 2.0), 0.0)}
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
SLICE = 1 << 22                                               # samples expanded at a time (bounds the intermediates)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def expand(xy, rgb, w, W, H, radius, table):
    """the caller-side expansion of the parent route: (pixel int32, rgb, w * f) in the definition's order (sample, line, col)"""
    TS = table.shape[0]
    rx, ry = np.float32(radius[0]), np.float32(radius[1])
    inv_rx, inv_ry = float(np.float32(1) / rx), float(np.float32(1) / ry)
    nx = int(np.ceil(float(rx) - 0.5))                         # cells further away hold no sample within the radius
    ny = int(np.ceil(float(ry) - 0.5))
    dl, dc = torch.meshgrid(torch.arange(-ny, ny + 1, device="cuda"), torch.arange(-nx, nx + 1, device="cuda"), indexing="ij")
    dl, dc = dl.reshape(1, -1), dc.reshape(1, -1)
    pix, col3, wf = [], [], []
    for b0 in range(0, xy.shape[0], SLICE):
        x, y = xy[b0:b0 + SLICE, 0:1], xy[b0:b0 + SLICE, 1:2]
        col, line = torch.floor(x).long() + dc, torch.floor(y).long() + dl
        dx, dy = ((col.float() + 0.5) - x).abs(), ((line.float() + 0.5) - y).abs()
        ix = (dx * inv_rx * float(TS)).long().clamp_(0, TS - 1)
        iy = (dy * inv_ry * float(TS)).long().clamp_(0, TS - 1)
        f = table[iy, ix]
        inside = (dx < float(rx)) & (dy < float(ry)) & (col >= 0) & (col < W) & (line >= 0) & (line < H) & (f != 0)
        s, c = inside.nonzero(as_tuple=True)
        pix.append((line[s, c] * W + col[s, c]).int())
        col3.append(rgb[b0:b0 + SLICE][s])
        wf.append(w[b0:b0 + SLICE][s] * f[s, c])
    return torch.cat(pix), torch.cat(col3), torch.cat(wf)


def measure(ctx, size, spp, fname, reps, g):
    W, H = SIZES[size]
    kind, radius, param = FILTERS[fname]
    n = W * H * spp
    table = bh.filter_table(kind, radius, param, 16)
    dtable = torch.from_numpy(table).cuda()
    cells = torch.arange(W * H, device="cuda").repeat_interleave(spp)[torch.randperm(n, generator=g, device="cuda")]
    xy = torch.stack([(cells % W).float(), (cells // W).float()], 1) + torch.rand((n, 2), generator=g, device="cuda") * 0.998 + 0.001
    xy = xy.contiguous()
    rgb = torch.rand((n, 3), generator=g, device="cuda") * 1.5
    w = torch.rand((n,), generator=g, device="cuda") + 0.5
    res = {"size": size, "spp": spp, "filter": fname, "samples": n}
    acc = ctx.accumulator(W, H)
    acc.set_filter(table, radius)
    ms = timed(lambda: acc.add_splatted(xy, rgb, w), reps)
    res["splat_ms"] = round(ms, 4)
    res["splat_Msamples_per_s"] = round(n / ms / 1e3, 1)
    floor_pix = cells.int()
    ms_f = timed(lambda: acc.add_samples(floor_pix, rgb, w), reps)
    res["floor_ms"] = round(ms_f, 4)
    res["splat_over_floor"] = round(ms / ms_f, 3)
    torch.cuda.synchronize()
    est = n * (1 if fname == "box" else (2 * radius[0]) * (2 * radius[1]))
    if est * 1.05 < (1 << 30):
        out = [None]

        def do_expand():
            out[0] = None
            out[0] = expand(xy, rgb, w, W, H, radius, dtable)
        res["expand_ms"] = round(timed(do_expand, max(2, reps // 3), warm=1), 4)
        pix_e, rgb_e, w_e = out[0]
        res["entries"] = int(pix_e.shape[0])
        ms_p = timed(lambda: acc.add_samples(pix_e, rgb_e, w_e), reps)
        res["parent_ms"] = round(ms_p, 4)
        res["parent_over_splat"] = round(ms_p / ms, 3)
        if spp == 1 and size == "1080p":                       # the two routes leave the same bits
            a, b = ctx.accumulator(W, H), ctx.accumulator(W, H)
            a.set_filter(table, radius)
            a.add_splatted(xy, rgb, w)
            b.add_samples(pix_e, rgb_e, w_e)
            sa, sb = a.statistics(), b.statistics()
            torch.cuda.synchronize()
            res["same_bits_as_parent"] = all(bool(torch.equal(u.view(torch.int32), v.view(torch.int32))) for u, v in zip(sa[:3], sb[:3]))
            res["info"] = [list(a.info()), list(b.info())]
            a.close()
            b.close()
    else:
        res["expand_ms"] = res["parent_ms"] = None
        res["note"] = "parent route not measured: about %.2e expanded entries, above 2^30" % est
    acc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = bh.Context(0, torch.cuda.current_stream())          # the events bracket the context's stream
    g = torch.Generator(device="cuda").manual_seed(1)
    todo = [tuple(a.only.split(":"))] if a.only else [(s, k, f) for s in SIZES for k in ("1", "8") for f in FILTERS]
    for size, spp, fname in todo:
        res = measure(ctx, size, int(spp), fname, a.reps if int(spp) == 1 else max(3, a.reps // 3), g)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
