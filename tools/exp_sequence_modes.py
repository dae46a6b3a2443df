#!/usr/bin/env python3
"""GPU box: what a sequence in a mode saves over the matching per-frame call (DESIGN.md section 16 "Modes", docs/EXPERIMENTS.md section 29).
At 1920 x 1080, 32 spp, 3 scales, b = 6, -m 1 -r 1, every shape warmed up; a figure is the median of --reps host-clock timings around calls that end in a
synchronisation, `spread` is (max - min) / median of those repeats.  The modes:
  hist_L4        histograms, 4 colour layers, no gate          bcd_hip_denoise_temporal_layers
  guided_F7      histograms, 1 layer, 7 feature channels        bcd_hip_denoise_temporal_guided
  mom_L1         moments, 1 layer                               bcd_hip_denoise_temporal_moments
  mom_L4_F7      moments, 4 layers, 7 feature channels          bcd_hip_denoise_temporal_moments with the guide
per mode:
  cross_{mode}, gate_{mode}   the cross pass of one pair by its stage call and, with the gate, bcd_hip_similarity_masks_guide_cross: one cross stage
  per R in 1, 2:
    call_{mode}_R{R}          the per-frame call on a frame with its 2R neighbours, called per frame as a user without the sequence would
    sequence_{mode}_R{R}      one steady-state step of the sequence: the pop of frame t and the push of frame t + R (the frames cycle)
  condition_{mode}_R{R}       sequence <= parent's call - R x (cross + gate) / 2 ?
--parent-lib names the library of the parent commit's build: its per-frame calls are timed in child processes of this tool (BCD_HIP_LIB, --calls-only) before
and after this build's figures -- alternately, in the same visit -- and the bound uses the median of the two; this build's per-frame calls stand beside them.
usage: python tools/exp_sequence_modes.py [--reps N] [--size 1920x1080] [--scales 3] [--parent-lib FILE.so] [--modes a,b] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import timings  # noqa: E402
from exp_sequence import summary  # noqa: E402

MODES = {
    "hist_L4": dict(L=4, moments=False, F=0),
    "guided_F7": dict(L=1, moments=False, F=7),
    "mom_L1": dict(L=1, moments=True, F=0),
    "mom_L4_F7": dict(L=4, moments=True, F=7),
}
VAR_FLOOR, TAU_MOMENTS, TAU_G = 1e-4, 2.0, 1.0
FLOORS = (0.01,) * 7


def make_frames(W, H, n):
    """n frames as dicts of device tensors: ns, hist, 4 layers (the frame and three per-channel shares of it), 7 feature channels (no variances)"""
    l, c = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    gains = [np.ones((H, W, 3), np.float32)] + [np.stack([0.2 + 0.6 * ((c / W + 0.3 * k) % 1), 0.7 - 0.4 * l / H, 0.3 + 0.1 * k + 0 * l], -1).astype(np.float32) for k in range(3)]
    feat = np.stack([((l // (40 + 9 * k) + c // (64 + 7 * k)) % 2) * 0.6 + 0.2 for k in range(7)], -1).astype(np.float32)
    out = []
    for seed in (1234, 77, 4321, 99, 555, 31, 32, 33)[:n]:
        col, ns, hist, cov = core.synthetic_scene(W, H, 32, seed, 0.35, 0.01)
        rng = np.random.default_rng(seed)
        layers = []
        for g in gains:
            gg = np.stack([g[..., 0] * g[..., 0], g[..., 1] * g[..., 1], g[..., 2] * g[..., 2], g[..., 1] * g[..., 2], g[..., 0] * g[..., 2], g[..., 0] * g[..., 1]], -1)
            layers.append((torch.from_numpy(np.ascontiguousarray(col * g)).cuda(), torch.from_numpy(np.ascontiguousarray(cov * gg)).cuda()))
        f = (feat + np.float32(0.01) * rng.standard_normal(feat.shape).astype(np.float32)).astype(np.float32)
        out.append(dict(ns=torch.from_numpy(ns).cuda(), hist=torch.from_numpy(hist).cuda(), layers=layers, feat=torch.from_numpy(f).cuda()))
    return out


def call_of(ctx, mode, fr, mid, nbs, S, prm, outs):
    m = MODES[mode]
    me, L, F = fr[mid], m["L"], m["F"]
    lay = me["layers"][:L]
    guide = dict(features=me["feat"], neighbour_features=[fr[k]["feat"] for k in nbs], floors=FLOORS[:F], threshold=TAU_G) if F else {}
    if m["moments"]:
        return lambda: ctx.denoise_temporal_moments(me["ns"], lay, [(fr[k]["ns"], fr[k]["layers"][:L]) for k in nbs], S, prm, var_floor=VAR_FLOOR, outs=outs, **guide)
    nb = [(fr[k]["ns"], fr[k]["hist"], fr[k]["layers"][:L]) for k in nbs]
    if F:
        return lambda: ctx.denoise_temporal_guided(me["ns"], me["hist"], lay, nb, S, prm, outs=outs, **guide)
    return lambda: ctx.denoise_temporal_layers(me["ns"], me["hist"], lay, nb, S, prm, outs=outs)


def steady_state(seq, frames, reps, warm, outs):
    seq.reset()
    n, k = len(frames), 0
    while seq.ready() == 0:
        seq.push(*frames[k % n])
        k += 1
    t = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq.pop(out=outs)
        seq.push(*frames[k % n])
        torch.cuda.synchronize()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
        k += 1
    return summary(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--scales", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--calls-only", action="store_true", help="the per-frame calls of the library BCD_HIP_LIB names, nothing of a sequence (an older build)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    modes = [m for m in a.modes.split(",") if m]
    W, H = (int(x) for x in a.size.split("x"))
    S = a.scales
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, scales=S, timing={}, device_bytes={}, parent=[], condition={})
    row = res["timing"]

    def parent_calls():
        if not a.parent_lib or a.calls_only:
            return
        cmd = [sys.executable, os.path.abspath(__file__), "--calls-only", "--reps", str(a.reps), "--warmup", str(a.warmup), "--size", a.size, "--scales", str(S),
               "--frames", str(a.frames), "--modes", ",".join(modes)]
        r = subprocess.run(cmd, env=dict(os.environ, BCD_HIP_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        res["parent"].append(json.loads(r.stdout.strip().splitlines()[-1])["timing"])
        print("parent", json.dumps(res["parent"][-1]), flush=True)

    parent_calls()                                                   # (before any GPU work of this process: one process at a time holds the frames)
    ctx = bh.Context(0)
    fr = make_frames(W, H, a.frames)
    mid = a.frames // 2
    mask_out = (torch.zeros((H, W, 6), dtype=torch.int32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
    for mode in modes:
        m = MODES[mode]
        L, F = m["L"], m["F"]
        prm = bh.default_params(m=1.0, random_order=1, tau=TAU_MOMENTS if m["moments"] else 1.0)
        outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(L)]
        x, y = fr[mid], fr[mid + 1]
        if m["moments"]:
            px, py = ctx.pixel_cov(x["layers"][0][1], x["ns"]), ctx.pixel_cov(y["layers"][0][1], y["ns"])
            row["cross_" + mode] = timings(lambda: ctx.similarity_masks_moments_cross(x["layers"][0][0], px, y["layers"][0][0], py, 1, 6, prm.hist_dist_threshold, VAR_FLOOR,
                                                                                      out=mask_out), a.reps, a.warmup)
        else:
            row["cross_" + mode] = timings(lambda: ctx.similarity_masks_cross(x["hist"], x["ns"], y["hist"], y["ns"], 1, 6, 1.0, out=mask_out), a.reps, a.warmup)
        stage = row["cross_" + mode]["ms"]
        if F:
            fx, fy = x["feat"][..., :F].contiguous(), y["feat"][..., :F].contiguous()
            row["gate_" + mode] = timings(lambda: ctx.similarity_masks_guide_cross(fx, None, fy, None, FLOORS[:F], TAU_G, 1, 6, out=mask_out), a.reps, a.warmup)
            stage += row["gate_" + mode]["ms"]
        for R in (1, 2):
            key = "%s_R%d" % (mode, R)
            nbs = [k for k in range(mid - R, mid + R + 1) if k != mid]
            row["call_" + key] = timings(call_of(ctx, mode, fr, mid, nbs, S, prm, outs), a.reps, a.warmup)
            if a.calls_only:
                continue
            seq = ctx.sequence(W, H, 0 if m["moments"] else x["hist"].shape[2], S, R, prm, layers=L, moments=m["moments"], var_floor=VAR_FLOOR, features=F,
                               feature_floors=FLOORS[:F], feature_threshold=TAU_G)
            frames = [(f["ns"], None if m["moments"] else f["hist"], f["layers"][:L], f["feat"][..., :F].contiguous() if F else None, None) for f in fr]
            row["sequence_" + key] = steady_state(seq, frames, a.reps, a.warmup, outs)
            res["device_bytes"][key] = seq.info()["device_bytes"]
            seq.close()
            res["condition"][key] = dict(cross_stage_ms=round(stage, 4), margin_ms=round(R * stage / 2, 4))
            print(key, json.dumps({k: v for k, v in row.items() if key in k}), "device_bytes", res["device_bytes"][key], flush=True)
    ctx.close()
    del fr
    torch.cuda.empty_cache()
    parent_calls()
    for key, c in res["condition"].items():
        ref = [p["call_" + key]["ms"] for p in res["parent"]] or [row["call_" + key]["ms"]]     # (without --parent-lib: this build's own call)
        c["parent_call_ms"] = round(float(np.median(ref)), 4)
        c["bound_ms"] = round(c["parent_call_ms"] - c["margin_ms"], 4)
        c["sequence_ms"] = row["sequence_" + key]["ms"]
        c["this_call_ms"] = row["call_" + key]["ms"]
        c["met"] = bool(c["sequence_ms"] <= c["bound_ms"])
        print("condition", key, json.dumps(c), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
