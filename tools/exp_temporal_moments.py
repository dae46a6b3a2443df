#!/usr/bin/env python3
"""GPU box: what the cross-frame selection from means and covariances costs (bcd_hip_denoise_temporal_moments; DESIGN.md section 16 "Moments",
docs/EXPERIMENTS.md section 27).  1920 x 1080, 32 spp, b = 6, -m 1 -r 1, resident inputs, every shape warmed up; a figure is the median of --reps host-clock
timings around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats.
  pairdist_moments_cross      k_pairdist_moments_cross alone, by the library's events (bcd_hip_kernel_time around the stage call in form 1), with the rate of its
                              stores: 5 bytes per plane entry whose neighbour pixel is inside the image, over all (2b+1)^2 displacements
  masks_moments_cross_fused   k_masks_moments_cross_fused alone, the same way (form 2)
  cross_stage_form{1,2}       the cross stage of one neighbour by the host clock around bcd_hip_similarity_masks_moments_cross: form 1 is the distance kernel
                              and k_masks_cross, form 2 the one fused kernel
  cross_stage_hist            bcd_hip_similarity_masks_cross on the same frames' histograms (D = 60), for scale
  moments_S{1,3}_L{1,4}_N{1,2}      bcd_hip_denoise_temporal_moments;  hist_S.._L.._N..: bcd_hip_denoise_temporal_layers on the same frames; with the guide "f7"
                              of tools/exp_temporal_guided.py: moments_guided_.. beside bcd_hip_denoise_temporal_guided (hist_guided_..); the *_stats rows
                              hold processed / fallback / similar_total of every scale (the two selections differ, so does the work behind them)
With --parent-lib FILE (a libbcd_hip.so built from the parent commit): bcd_hip_denoise, bcd_hip_denoise_moments (L = 1) and bcd_hip_denoise_temporal (N = 2) at
3 scales in child processes that load this build and the parent's alternately, --rounds times each.
usage: python tools/exp_temporal_moments.py [--reps N] [--size 1920x1080] [--parent-lib FILE] [--rounds N] [--out FILE.json]"""
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
from exp_temporal_guided import cross_stored_bytes, guides_on_device  # noqa: E402
from exp_temporal_layers import frames_on_device  # noqa: E402

VAR_FLOOR = 1e-8


def base_child(a):
    """the calls whose kernels this build does not edit, on whatever library BCD_HIP_LIB names"""
    W, H = (int(x) for x in a.size.split("x"))
    ctx = bh.Context(0)
    prm = bh.default_params(m=1.0, random_order=1)
    fr = frames_on_device(W, H, 1)
    ns, hist, lay = fr[0]
    nb = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:3]]
    row = {}
    row["denoise_S3"] = timings(lambda: ctx.denoise(lay[0][0], ns, hist, lay[0][1], 3, prm), a.reps, a.warmup)
    row["moments_L1_S3"] = timings(lambda: ctx.denoise_moments(ns, lay[:1], 3, prm, VAR_FLOOR), a.reps, a.warmup)
    row["temporal_S3_N2"] = timings(lambda: ctx.denoise_temporal(lay[0][0], ns, hist, lay[0][1], nb, 3, prm), a.reps, a.warmup)
    ctx.close()
    print("BASE " + json.dumps(row), flush=True)


def kernel_ms(ctx, call, reps, warmup):
    """the distance kernel of `call` by the library's events"""
    ms = []
    for _ in range(warmup + reps):
        ctx.reset_kernel_time()
        call()
        t, n = ctx.kernel_time()
        assert n == 1
        ms.append(t)
    ms = np.array(ms[warmup:])
    med = float(np.median(ms))
    return dict(ms=round(med, 4), min=round(float(ms.min()), 4), max=round(float(ms.max()), 4), spread=round(float((ms.max() - ms.min()) / med), 4))


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
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, stage={}, timing={}, base={})
    ctx = bh.Context(0)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    # ---- the cross stage of one neighbour
    P0, P1 = ctx.pixel_cov(lay[0][1], ns), ctx.pixel_cov(fr[1][2][0][1], fr[1][0])
    c0, c1 = lay[0][0], fr[1][2][0][0]
    out = bh._mask_and_count(H, W, b, "cuda")
    stage = lambda form: ctx.similarity_masks_moments_cross(c0, P0, c1, P1, w, b, tau, VAR_FLOOR, form, out=out)
    nbytes = cross_stored_bytes(W, H, b)
    k1 = kernel_ms(ctx, lambda: stage(1), a.reps, a.warmup)
    res["stage"]["pairdist_moments_cross"] = dict(k1, stored_bytes=nbytes, stored_GBps=round(nbytes / (k1["ms"] * 1e-3) / 1e9, 1))
    res["stage"]["masks_moments_cross_fused"] = kernel_ms(ctx, lambda: stage(2), a.reps, a.warmup)
    for _ in range(2):                                                       # (twice, alternately: the two forms are compared with each other)
        for form in (1, 2):
            res["stage"].setdefault("cross_stage_form%d" % form, []).append(timings(lambda: stage(form), a.reps, a.warmup))
    m1 = ctx.similarity_masks_moments_cross(c0, P0, c1, P1, w, b, tau, VAR_FLOOR, 1)[0].clone()
    m2 = ctx.similarity_masks_moments_cross(c0, P0, c1, P1, w, b, tau, VAR_FLOOR, 2)[0]
    res["stage"]["forms_agree"] = bool(torch.equal(m1, m2))
    res["stage"]["cross_stage_hist"] = timings(lambda: ctx.similarity_masks_cross(hist, ns, fr[1][1], fr[1][0], w, b, tau, out=out), a.reps, a.warmup)
    print("stage", json.dumps(res["stage"]), flush=True)
    del P0, P1, out, m1, m2
    torch.cuda.empty_cache()
    # ---- the frame call beside the histogram call of the same build
    guides = guides_on_device(W, H, 3)
    g, fl = guides["f7"]
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    stats = lambda S: [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total) for s in (ctx.stats(k) for k in range(S))]
    for S in (1, 3):
        for L in (1, 4):
            for N in (1, 2):
                nbl = [(f[0], f[1], f[2][:L]) for f in fr[1:1 + N]]
                nbm = [(f[0], f[2][:L]) for f in fr[1:1 + N]]
                key = "S%d_L%d_N%d" % (S, L, N)
                gkw = dict(variances=None, neighbour_variances=None, floors=fl, threshold=1.0)
                calls = {
                    "hist_" + key: lambda: ctx.denoise_temporal_layers(ns, hist, lay[:L], nbl, S, prm, outs=outs[:L]),
                    "moments_" + key: lambda: ctx.denoise_temporal_moments(ns, lay[:L], nbm, S, prm, VAR_FLOOR, outs=outs[:L]),
                    "hist_guided_" + key: lambda: ctx.denoise_temporal_guided(ns, hist, lay[:L], nbl, S, prm, g[0][0], [x[0] for x in g[1:1 + N]], outs=outs[:L], **gkw),
                    "moments_guided_" + key: lambda: ctx.denoise_temporal_moments(ns, lay[:L], nbm, S, prm, VAR_FLOOR, features=g[0][0],
                                                                                  neighbour_features=[x[0] for x in g[1:1 + N]], outs=outs[:L], **gkw),
                }
                for name, call in calls.items():
                    res["timing"][name] = timings(call, a.reps, a.warmup)
                    res["timing"][name + "_stats"] = stats(S)
                print(key, json.dumps({k: v["ms"] for k, v in res["timing"].items() if key in k and not k.endswith("_stats")}), flush=True)
    ctx.close()
    del fr, guides
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
