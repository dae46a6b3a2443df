#!/usr/bin/env python3
"""GPU box: what the motion path of the temporal calls costs (DESIGN.md section 16 "Motion", docs/EXPERIMENTS.md section 24).  1920 x 1080, 32 spp, D = 60,
b = 6, -m 1 -r 1, resident inputs, every shape warmed up; a figure is the median of --reps host-clock timings around calls that end in a synchronisation,
`spread` is (max - min) / median of those repeats:
  warp_frame              bcd_hip_warp_frame alone (k_warp_frame<60>), with the rate of its bytes: 2 x (10 + D) x 4 B/px of images, 8 B/px of field, 1 B/px of
                          validity; the field is integer motion within +-8 pixels with 2 % NaN
  copy_same_bytes         a device-to-device hipMemcpyAsync of as many bytes, timed the same way in the same run; `warp_over_copy` is the ratio
  warp_layers_L4          bcd_hip_warp_layers for four layers
  gate                    bcd_hip_gate_masks_valid alone (k_valid_patch + k_masks_gate_valid) on the cross masks of a neighbour
  motion_S{1,3}_F{1,2}    bcd_hip_denoise_temporal_motion with zero-valued fields (every neighbour is copied and gated, nothing is removed)
  plain_S{1,3}_F{1,2}     bcd_hip_denoise_temporal on the same inputs
  motion_layers_S{1,3}_L4_F{1,2} / plain_layers_...   the layered twins
With --parent-lib FILE (a libbcd_hip.so built from the parent commit): bcd_hip_denoise, bcd_hip_denoise_temporal (F = 2) and bcd_hip_denoise_layers /
bcd_hip_denoise_temporal_layers (L = 4) in child processes that load this build and the parent's alternately, --rounds times each.
usage: python tools/exp_motion.py [--reps N] [--size 1920x1080] [--parent-lib FILE] [--rounds N] [--out FILE.json]"""
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
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import timings  # noqa: E402
from exp_temporal_layers import frames_on_device  # noqa: E402


def base_child(a):
    """the calls that run unedited kernels, on whatever library BCD_HIP_LIB names"""
    W, H = (int(x) for x in a.size.split("x"))
    ctx = bh.Context(0)
    prm = bh.default_params(m=1.0, random_order=1)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    nb = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:]]
    nbl = [(f[0], f[1], f[2]) for f in fr[1:]]
    row = {}
    for S in (1, 3):
        row["denoise_S%d" % S] = timings(lambda: ctx.denoise(lay[0][0], ns, hist, lay[0][1], S, prm), a.reps, a.warmup)
        row["temporal_S%d_F2" % S] = timings(lambda: ctx.denoise_temporal(lay[0][0], ns, hist, lay[0][1], nb, S, prm), a.reps, a.warmup)
        row["temporal_layers_S%d_L4_F2" % S] = timings(lambda: ctx.denoise_temporal_layers(ns, hist, lay, nbl, S, prm), a.reps, a.warmup)
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
    w, b, tau, D = 1, 6, 1.0, 60
    prm = bh.default_params(m=1.0, random_order=1)
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, stage={}, timing={}, base={})
    ctx = bh.Context(0)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    npix = W * H
    # ---- the stage kernels alone
    rng = np.random.default_rng(5)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mv = np.stack([np.clip(c + rng.integers(-8, 9, (H, W)), 0, W - 1) - c, np.clip(l + rng.integers(-8, 9, (H, W)), 0, H - 1) - l], -1).astype(np.float32)
    mv[rng.random((H, W)) < 0.02] = np.nan
    d_mv = torch.from_numpy(mv).cuda()
    nbf = (fr[1][2][0][0], fr[1][0], fr[1][1], fr[1][2][0][1])
    dst = [torch.empty_like(x) for x in nbf] + [torch.empty((H, W), dtype=torch.uint8, device="cuda")]
    warp_bytes = npix * (2 * (10 + D) * 4 + 8 + 1)
    t = timings(lambda: ctx.warp_frame(*nbf, d_mv, out=dst), a.reps, a.warmup)
    res["stage"]["warp_frame"] = dict(t, bytes=warp_bytes, gb_per_s=round(warp_bytes / t["ms"] / 1e6, 1))
    src8 = torch.empty((warp_bytes // 2,), dtype=torch.uint8, device="cuda")
    dst8 = torch.empty_like(src8)
    tc = timings(lambda: dst8.copy_(src8), a.reps, a.warmup)                  # (reads and writes warp_bytes / 2 each: the same traffic)
    res["stage"]["copy_same_bytes"] = dict(tc, bytes=warp_bytes, gb_per_s=round(warp_bytes / tc["ms"] / 1e6, 1))
    res["stage"]["warp_over_copy"] = round(t["ms"] / tc["ms"], 3)
    ldst = ([(torch.empty_like(cc), torch.empty_like(vv)) for cc, vv in fr[1][2]], dst[4])
    res["stage"]["warp_layers_L4"] = timings(lambda: ctx.warp_layers(fr[1][2], d_mv, out=ldst), a.reps, a.warmup)
    del src8, dst8, ldst
    m_nb, n_nb = ctx.similarity_masks_cross(hist, ns, fr[1][1], fr[1][0], w, b, tau)
    ctx.synchronize()
    copies = [(m_nb.clone(), n_nb.clone()) for _ in range(a.reps + a.warmup)]          # (the gate works in place: every repeat gets untouched masks)
    it = iter(copies)
    res["stage"]["gate"] = timings(lambda: ctx.gate_masks_valid(*next(it), dst[4], w, b), a.reps, a.warmup)
    print("stage", json.dumps(res["stage"]), flush=True)
    del copies, m_nb, n_nb
    torch.cuda.empty_cache()
    # ---- the calls: zero fields beside the plain calls
    zero = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    for S in (1, 3):
        for F in (1, 2):
            nb = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:1 + F]]
            nbl = [(f[0], f[1], f[2]) for f in fr[1:1 + F]]
            key = "S%d_F%d" % (S, F)
            res["timing"]["motion_" + key] = timings(lambda: ctx.denoise_temporal_motion(lay[0][0], ns, hist, lay[0][1], nb, [zero] * F, S, prm, out=out), a.reps, a.warmup)
            res["timing"]["plain_" + key] = timings(lambda: ctx.denoise_temporal(lay[0][0], ns, hist, lay[0][1], nb, S, prm, out=out), a.reps, a.warmup)
            key = "S%d_L4_F%d" % (S, F)
            res["timing"]["motion_layers_" + key] = timings(lambda: ctx.denoise_temporal_layers_motion(ns, hist, lay, nbl, [zero] * F, S, prm, outs=outs), a.reps, a.warmup)
            res["timing"]["plain_layers_" + key] = timings(lambda: ctx.denoise_temporal_layers(ns, hist, lay, nbl, S, prm, outs=outs), a.reps, a.warmup)
            print(S, F, json.dumps({k: v["ms"] for k, v in res["timing"].items() if k.endswith("F%d" % F) and ("S%d" % S) in k}), flush=True)
    ctx.close()
    del fr
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
