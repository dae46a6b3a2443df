#!/usr/bin/env python3
"""GPU box: what one shared selection saves when the colour layers of a frame are denoised with its neighbour frames (DESIGN.md section 16 "Layers",
docs/EXPERIMENTS.md section 23).  1920 x 1080, 32 spp, b = 6, -m 1 -r 1, resident inputs, every shape warmed up; a figure is the median of --reps host-clock
timings around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats:
  layered_S{1,3}_L{1,2,4}_F{1,2}    bcd_hip_denoise_temporal_layers
  separate_S{1,3}_L{1,2,4}_F{1,2}   L calls of bcd_hip_denoise_temporal, one per layer, of the same build
  fallback_layered_L{2,4}_F{1,2}    bcd_hip_bayes_accumulate_temporal_layers on the selection's FALLBACK pixels alone (the states of the full estimates
                                    cleared, so the chain of full estimates has nothing to do: the lists and one launch of k_bayes_weak_temporal_layers)
  fallback_separate_L{2,4}_F{1,2}   L calls of bcd_hip_bayes_accumulate_temporal on the same states (the lists and k_bayes_weak_temporal, L times)
With --parent-lib FILE (a libbcd_hip.so built from the parent commit): bcd_hip_denoise_temporal (F = 2), bcd_hip_denoise_layers (L = 4) and bcd_hip_denoise at
1 and 3 scales, in child processes that load this build and the parent's alternately, --rounds times each (`base` in the result: per library the median
of the rounds' medians and every round's median).
usage: python tools/exp_temporal_layers.py [--reps N] [--size 1920x1080] [--parent-lib FILE] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import make_layers, timings  # noqa: E402


def scene(W, H, spp, seed, sigma=0.35, spikes=0.01):
    return core.synthetic_scene(W, H, spp, seed, sigma, spikes)


def frames_on_device(W, H, L):
    """three frames -> [(ns, hist, [(colours, covariances)] * L)] on the device, the same shares of every frame"""
    out = []
    for seed in (1234, 77, 4321):
        col, ns, hist, cov = scene(W, H, 32, seed)
        lay = [(torch.from_numpy(np.ascontiguousarray(c)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda()) for c, v in make_layers(col, cov, L)]
        out.append((torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda(), lay))
    return out


def base_child(a):
    """the three calls that run unedited kernels, on whatever library BCD_HIP_LIB names"""
    W, H = (int(x) for x in a.size.split("x"))
    ctx = bh.Context(0)
    prm = bh.default_params(m=1.0, random_order=1)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    row = {}
    for S in (1, 3):
        row["denoise_S%d" % S] = timings(lambda: ctx.denoise(lay[0][0], ns, hist, lay[0][1], S, prm), a.reps, a.warmup)
        row["layers_S%d_L4" % S] = timings(lambda: ctx.denoise_layers(ns, hist, lay, S, prm), a.reps, a.warmup)
        nb = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:]]
        row["temporal_S%d_F2" % S] = timings(lambda: ctx.denoise_temporal(lay[0][0], ns, hist, lay[0][1], nb, S, prm), a.reps, a.warmup)
    ctx.close()
    print("BASE " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--base-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if a.base_child:
        return base_child(a)
    W, H = (int(x) for x in a.size.split("x"))
    w, b, tau = 1, 6, 1.0
    prm = bh.default_params(m=1.0, random_order=1)
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, timing={}, fallback={}, base={})
    ctx = bh.Context(0)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    for S in (1, 3):
        for F in (1, 2):
            for L in (1, 2, 4):
                nb = [(f[0], f[1], f[2][:L]) for f in fr[1:1 + F]]
                outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(L)]
                res["timing"]["layered_S%d_L%d_F%d" % (S, L, F)] = timings(lambda: ctx.denoise_temporal_layers(ns, hist, lay[:L], nb, S, prm, outs=outs), a.reps, a.warmup)

                def separate():
                    for k in range(L):
                        ctx.denoise_temporal(lay[k][0], ns, hist, lay[k][1], [(f[2][k][0], f[0], f[1], f[2][k][1]) for f in fr[1:1 + F]], S, prm, out=outs[k])
                res["timing"]["separate_S%d_L%d_F%d" % (S, L, F)] = timings(separate, a.reps, a.warmup)
                print(S, F, L, json.dumps({k: v for k, v in res["timing"].items() if k.endswith("S%d_L%d_F%d" % (S, L, F))}), flush=True)
    # ---- the fallback pixels alone, on the selection of the finest scale
    mask, nsim = ctx.similarity_masks(hist, ns, w, b, tau)
    ctx.synchronize()
    masks, total = [mask], [nsim.clone()]
    for f in fr[1:]:
        m_nb, n_nb = ctx.similarity_masks_cross(hist, ns, f[1], f[0], w, b, tau)
        masks.append(m_nb)
        total.append(total[-1] + n_nb)
    pixcov = [[ctx.pixel_cov(v, f[0]) for _, v in f[2]] for f in fr]
    ctx.synchronize()
    for F in (1, 2):
        state, _ = ctx.active_set(mask, total[F], w, b, 1.0, 1, prm.order_seed)
        ctx.synchronize()
        weak_only = torch.where((state == 1) & (total[F] < 28), state, torch.zeros_like(state)).contiguous()
        n_weak = int((weak_only == 1).sum())
        for L in (2, 4):
            sums = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(L)]
            cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            frames = [([(fr[f][2][k][0], pixcov[f][k]) for k in range(L)], masks[f]) for f in range(1 + F)]
            res["fallback"]["fallback_layered_L%d_F%d" % (L, F)] = dict(
                timings(lambda: ctx.bayes_accumulate_temporal_layers(frames, total[F], weak_only, w, b, 1e-8, out=(sums, cnt)), a.reps, a.warmup), fallback=n_weak)

            def separate():
                for k in range(L):
                    ctx.bayes_accumulate_temporal([(fr[f][2][k][0], pixcov[f][k], masks[f]) for f in range(1 + F)], total[F], weak_only, w, b, 1e-8, out=(sums[k], cnt))
            res["fallback"]["fallback_separate_L%d_F%d" % (L, F)] = dict(timings(separate, a.reps, a.warmup), fallback=n_weak)
    print("fallback", json.dumps(res["fallback"]), flush=True)
    ctx.close()
    del fr, masks, total, pixcov
    torch.cuda.empty_cache()
    # ---- the calls whose kernels this build does not edit, beside the parent's library
    if a.parent_lib:
        rounds = {"this": [], "parent": []}
        for _ in range(a.rounds):
            for which, path in (("this", bh.LIB_PATH), ("parent", os.path.abspath(a.parent_lib))):
                env = dict(os.environ, BCD_HIP_LIB=path)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--base-child", "--reps", str(a.reps), "--warmup", str(a.warmup), "--size", a.size],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("the %s library's child failed:\n%s%s" % (which, r.stdout, r.stderr))
                rounds[which].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BASE ")][-1][5:]))
        for which, rows in rounds.items():
            res["base"][which] = {k: dict(ms=round(float(np.median([r[k]["ms"] for r in rows])), 4), rounds=[r[k]["ms"] for r in rows],
                                          spread=max(r[k]["spread"] for r in rows)) for k in rows[0]}
        print("base", json.dumps(res["base"]), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
