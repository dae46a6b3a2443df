#!/usr/bin/env python3
"""GPU box: what the feature gate of the cross-frame selection costs (bcd_hip_denoise_temporal_guided; DESIGN.md section 16 "Features", docs/EXPERIMENTS.md
section 26).  1920 x 1080, 32 spp, D = 60, b = 6, -m 1 -r 1, resident inputs, every shape warmed up; a figure is the median of --reps host-clock timings
around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats.  The guides are those of tools/exp_guided.py: "f7" (F = 7, no
variances, floors 0.01) and "f3v" (F = 3 with variances, floors 1e-4), one realisation per frame:
  pairdist_guide_cross_*   k_pairdist_guide_cross alone, by the library's events (bcd_hip_kernel_time around the stage call), with the rate of its stores:
                           5 bytes per plane entry whose neighbour pixel is inside the image, over all (2b+1)^2 displacements
  cross_stage_*            what one neighbour adds to a scale -- planes, masks, AND -- by the host clock around similarity_masks_guide_cross + gate_masks
  warp_features_*          bcd_hip_warp_features alone, with the rate of its bytes (features and variances read and written, 8 B/px of field, 1 B/px of
                           validity); copy_same_bytes_*: a device-to-device copy of as many bytes, timed the same way
  guided_S{1,3}_L{1,4}_N{1,2}_*  bcd_hip_denoise_temporal_guided;  plain_S.._L.._N..: bcd_hip_denoise_temporal_layers on the same inputs; the *_stats rows hold
                           processed / fallback / similar_total of every scale (a guide that removes pairs leaves more pixels to process)
With --parent-lib FILE (a libbcd_hip.so built from the parent commit): bcd_hip_denoise, bcd_hip_denoise_guided (F = 7, L = 1) and bcd_hip_denoise_temporal
(N = 2) at 3 scales in child processes that load this build and the parent's alternately, --rounds times each.
usage: python tools/exp_temporal_guided.py [--reps N] [--size 1920x1080] [--parent-lib FILE] [--rounds N] [--out FILE.json]"""
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
from exp_guided import features  # noqa: E402
from exp_layers import timings  # noqa: E402
from exp_temporal_layers import frames_on_device  # noqa: E402


def guides_on_device(W, H, frames):
    """{name: ([(features, variances or None) per frame], floors)}"""
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    f7 = [features(W, H, 7, seed=1 + i) for i in range(frames)]
    f3 = [features(W, H, 3, seed=11 + i) for i in range(frames)]
    return {"f7": ([(dev(f), None) for f, _ in f7], [0.01] * 7), "f3v": ([(dev(f), dev(v)) for f, v in f3], [1e-4] * 3)}


def cross_stored_bytes(W, H, b):
    return 5 * sum((H - abs(dl)) * (W - abs(dc)) for dl in range(-b, b + 1) for dc in range(-b, b + 1))


def base_child(a):
    """the calls whose kernels this build does not edit, on whatever library BCD_HIP_LIB names"""
    W, H = (int(x) for x in a.size.split("x"))
    ctx = bh.Context(0)
    prm = bh.default_params(m=1.0, random_order=1)
    fr = frames_on_device(W, H, 1)
    ns, hist, lay = fr[0]
    nb = [(f[2][0][0], f[0], f[1], f[2][0][1]) for f in fr[1:3]]
    f7, _ = features(W, H, 7)
    d_f = torch.from_numpy(f7).cuda()
    row = {}
    row["denoise_S3"] = timings(lambda: ctx.denoise(lay[0][0], ns, hist, lay[0][1], 3, prm), a.reps, a.warmup)
    row["guided_f7_L1_S3"] = timings(lambda: ctx.denoise_guided(ns, hist, lay[:1], 3, prm, d_f, None, [0.01] * 7, 1.0), a.reps, a.warmup)
    row["temporal_S3_N2"] = timings(lambda: ctx.denoise_temporal(lay[0][0], ns, hist, lay[0][1], nb, 3, prm), a.reps, a.warmup)
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
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, stage={}, timing={}, base={})
    ctx = bh.Context(0)
    fr = frames_on_device(W, H, 4)
    ns, hist, lay = fr[0]
    npix = W * H
    guides = guides_on_device(W, H, 3)
    rng = np.random.default_rng(5)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mv = np.stack([np.clip(c + rng.integers(-8, 9, (H, W)), 0, W - 1) - c, np.clip(l + rng.integers(-8, 9, (H, W)), 0, H - 1) - l], -1).astype(np.float32)
    mv[rng.random((H, W)) < 0.02] = np.nan
    d_mv = torch.from_numpy(mv).cuda()
    # ---- the stage kernels alone
    m_nb, n_nb = ctx.similarity_masks_cross(hist, ns, fr[1][1], fr[1][0], w, b, tau)
    ctx.synchronize()
    for name, (g, fl) in guides.items():
        (f0, v0), (f1, v1) = g[0], g[1]
        ms = []
        for _ in range(a.warmup + a.reps):
            ctx.reset_kernel_time()
            ctx.similarity_masks_guide_cross(f0, v0, f1, v1, fl, 1.0, w, b)
            t, n = ctx.kernel_time()
            assert n == 1
            ms.append(t)
        ms = np.array(ms[a.warmup:])
        med, nbytes = float(np.median(ms)), cross_stored_bytes(W, H, b)
        res["stage"]["pairdist_guide_cross_" + name] = dict(ms=round(med, 4), min=round(float(ms.min()), 4), max=round(float(ms.max()), 4), stored_bytes=nbytes,
                                                             stored_GBps=round(nbytes / (med * 1e-3) / 1e9, 1))
        gate = bh._mask_and_count(H, W, b, "cuda")
        copies = [(m_nb.clone(), n_nb.clone()) for _ in range(a.reps + a.warmup)]      # (the AND works in place: every repeat gets untouched masks)
        it = iter(copies)

        def stage():
            gm, _ = ctx.similarity_masks_guide_cross(f0, v0, f1, v1, fl, 1.0, w, b, out=gate)
            ctx.gate_masks(*next(it), gm, b)
        res["stage"]["cross_stage_" + name] = timings(stage, a.reps, a.warmup)
        del copies
        F = f1.shape[2]
        nbytes = npix * ((2 if v1 is not None else 1) * 2 * F * 4 + 8 + 1)
        dst = (torch.empty_like(f1), None if v1 is None else torch.empty_like(v1), torch.empty((H, W), dtype=torch.uint8, device="cuda"))
        t = timings(lambda: ctx.warp_features(f1, v1, d_mv, out=dst), a.reps, a.warmup)
        res["stage"]["warp_features_" + name] = dict(t, bytes=nbytes, gb_per_s=round(nbytes / t["ms"] / 1e6, 1))
        src8 = torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda")
        dst8 = torch.empty_like(src8)
        tc = timings(lambda: dst8.copy_(src8), a.reps, a.warmup)                       # (reads and writes nbytes / 2 each: the same traffic)
        res["stage"]["copy_same_bytes_" + name] = dict(tc, bytes=nbytes, gb_per_s=round(nbytes / tc["ms"] / 1e6, 1))
        del src8, dst8, dst, gate
    print("stage", json.dumps(res["stage"]), flush=True)
    del m_nb, n_nb
    torch.cuda.empty_cache()
    # ---- the frame call beside the unguided layered call of the same build
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    stats = lambda S: [dict(processed=s.processed, fallback=s.fallback, similar_total=s.similar_total) for s in (ctx.stats(k) for k in range(S))]
    for S in (1, 3):
        for L in (1, 4):
            for N in (1, 2):
                nbl = [(f[0], f[1], f[2][:L]) for f in fr[1:1 + N]]
                key = "S%d_L%d_N%d" % (S, L, N)
                res["timing"]["plain_" + key] = timings(lambda: ctx.denoise_temporal_layers(ns, hist, lay[:L], nbl, S, prm, outs=outs[:L]), a.reps, a.warmup)
                res["timing"]["plain_%s_stats" % key] = stats(S)
                for name, (g, fl) in guides.items():
                    call = lambda: ctx.denoise_temporal_guided(ns, hist, lay[:L], nbl, S, prm, g[0][0], [x[0] for x in g[1:1 + N]], variances=g[0][1],
                                                               neighbour_variances=None if g[0][1] is None else [x[1] for x in g[1:1 + N]], floors=fl, threshold=1.0,
                                                               outs=outs[:L])
                    res["timing"]["guided_%s_%s" % (key, name)] = timings(call, a.reps, a.warmup)
                    res["timing"]["guided_%s_%s_stats" % (key, name)] = stats(S)
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
