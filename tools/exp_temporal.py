#!/usr/bin/env python3
"""GPU box: what similar patches from neighbouring frames cost, stage by stage (docs/EXPERIMENTS.md section 21).
At 1920 x 1080 and 3840 x 2160, one scale, 32 spp, b = 6, -m 1 -r 1, resident inputs, every shape warmed up; a figure is the median of --reps host-clock
timings around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats:
  similarity          bcd_hip_similarity_masks: the in-frame selection (85 displacements through the approximate planes, verified at the threshold)
  cross               bcd_hip_similarity_masks_cross for ONE neighbour: 169 exact displacements, masks and counts
  estimate            bcd_hip_bayes_accumulate on the in-frame selection and its marking
  estimate_F1 / _F2   bcd_hip_bayes_accumulate_temporal with 1 and 2 neighbours, on the marking of the in-frame masks with the total |S|
  denoise1            bcd_hip_denoise with one scale
  stages_F0 / _F1 / _F2   Context.denoise_temporal_stages (the stage calls one after the other, each synchronised) with 0, 1 and 2 neighbours
  denoise3 / temporal3_F1 / _F2 / _F4   bcd_hip_denoise and bcd_hip_denoise_temporal with 3 scales (F = 4 adds two further realisations of the scene)
With --quality: RMSE against the noise-free base at 960 x 540, 16 spp, of the noisy frame, of bcd_hip_denoise (one scale) and of the composition with 1 and
2 neighbours (realisations of the same scene under other seeds).
usage: python tools/exp_temporal.py [--reps N] [--sizes 1920x1080,3840x2160] [--quality] [--out FILE.json]"""
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
from exp_layers import timings  # noqa: E402


def scene(W, H, spp, seed, sigma=0.35, spikes=0.01):
    return [torch.from_numpy(x).cuda() for x in core.synthetic_scene(W, H, spp, seed, sigma, spikes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = bh.Context(0)
    w, b, tau = 1, 6, 1.0
    prm = bh.default_params(m=1.0, random_order=1)
    res = dict(library=bh.LIB_PATH, reps=a.reps, timing={}, quality={})
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        fr = [scene(W, H, 32, seed) for seed in (1234, 77, 4321)]
        col, ns, hist, cov = fr[0]
        row = {}
        row["similarity"] = timings(lambda: ctx.similarity_masks(hist, ns, w, b, tau), a.reps, a.warmup)
        words = ((2 * b + 1) ** 2 + 31) // 32
        out = (torch.zeros((H, W, words), dtype=torch.int32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
        row["cross"] = timings(lambda: ctx.similarity_masks_cross(hist, ns, fr[1][2], fr[1][1], w, b, tau, out=out), a.reps, a.warmup)
        mask, nsim = ctx.similarity_masks(hist, ns, w, b, tau)
        ctx.synchronize()
        frames, total = [(col, ctx.pixel_cov(cov, ns), mask)], [nsim.clone()]
        for f in fr[1:]:
            m_nb, n_nb = ctx.similarity_masks_cross(hist, ns, f[2], f[1], w, b, tau)
            frames.append((f[0], ctx.pixel_cov(f[3], f[1]), m_nb))
            total.append(total[-1] + n_nb)
        ctx.synchronize()
        acc = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
        for F in (0, 1, 2):
            state, _ = ctx.active_set(mask, total[F], w, b, 1.0, 1, prm.order_seed)
            ctx.synchronize()
            n_in = int((state == 1).sum())
            n_full = int(((state == 1) & (total[F] >= 28)).sum())
            if F == 0:
                def plain():
                    ctx.bayes_accumulate(col, frames[0][1], mask, nsim, state, w, b, 1e-8, out=acc)
                    ctx.synchronize()
                row["estimate"] = dict(timings(plain, a.reps, a.warmup), processed=n_in, full=n_full)
            else:
                row["estimate_F%d" % F] = dict(timings(lambda: ctx.bayes_accumulate_temporal(frames[:1 + F], total[F], state, w, b, 1e-8, out=acc), a.reps, a.warmup),
                                               processed=n_in, full=n_full, similar_total=int(total[F][state == 1].sum()))
        row["denoise1"] = timings(lambda: ctx.denoise(col, ns, hist, cov, 1, prm), a.reps, a.warmup)
        for F in (0, 1, 2):
            row["stages_F%d" % F] = timings(lambda: ctx.denoise_temporal_stages(col, ns, hist, cov, fr[1:1 + F], prm), a.reps, a.warmup)
        more = fr + [scene(W, H, 32, seed) for seed in (99, 555)]
        row["denoise3"] = timings(lambda: ctx.denoise(col, ns, hist, cov, 3, prm), a.reps, a.warmup)
        for F in (1, 2, 4):
            row["temporal3_F%d" % F] = timings(lambda: ctx.denoise_temporal(col, ns, hist, cov, more[1:1 + F], 3, prm), a.reps, a.warmup)
        del more
        res["timing"][size] = row
        print(size, json.dumps(row), flush=True)
        del fr, frames, total, acc, out, mask, nsim
    if a.quality:
        W, H = 960, 540
        truth = core.synthetic_scene(W, H, 1, 1234, 0.0, 0.0)[0].astype(np.float64)
        rmse = lambda x: float(np.sqrt(np.mean((x.cpu().numpy().astype(np.float64)[1:-1, 1:-1] - truth[1:-1, 1:-1]) ** 2)))
        fr = [scene(W, H, 16, seed, 0.35, 0.0) for seed in (77, 1234, 4321)]
        mid = fr[1]
        q = dict(input=round(rmse(mid[0]), 6), denoise1=round(rmse(ctx.denoise(*mid, 1, prm)), 6))
        for F, nb in ((1, [fr[0]]), (2, [fr[0], fr[2]])):
            o, st = ctx.denoise_temporal_stages(*mid, nb, prm)
            q["stages_F%d" % F] = round(rmse(o), 6)
            q["stages_F%d_stats" % F] = st
        res["quality"]["960x540 16 spp"] = q
        print("quality", json.dumps(q), flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
