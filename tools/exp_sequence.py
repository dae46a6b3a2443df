#!/usr/bin/env python3
"""GPU box: what the sequence object saves over the per-frame temporal call (DESIGN.md section 16 "Sequences", docs/EXPERIMENTS.md section 28).
At 1920 x 1080, 32 spp, b = 6, -m 1 -r 1, every shape warmed up; a figure is the median of --reps host-clock timings around calls that end in a
synchronisation, `spread` is (max - min) / median of those repeats:
  transpose           bcd_hip_transpose_masks_cross (k_masks_transpose) on the cross masks of one pair
  cross               bcd_hip_similarity_masks_cross for the same pair (k_pairdist_cross + k_masks_cross): what the transposition replaces
  per R in 1, 2 and S in 1, 3 scales, device-resident and through the host entry points:
    call_R{R}_S{S}[_host]       bcd_hip_denoise_temporal[_host] on a frame with its 2R neighbours, called per frame as a user without the sequence would
    sequence_R{R}_S{S}[_host]   one steady-state step of the sequence: the push of frame t + R and the pop of frame t (frames cycle through --frames scenes)
    noreuse_R{R}_S{S}           the same step with set_reuse(0): the ring and the pyramids alone
  call_F1_S1          the per-frame call with ONE neighbour at one scale: call_R1_S1 - call_F1_S1 is what one neighbour costs the per-frame call
  condition           sequence_R1_S1 <= call_R1_S1 - (call_R1_S1 - call_F1_S1) / 2 ?  (the one performance condition of the feature)
  device_bytes        held by the sequence, per configuration
usage: python tools/exp_sequence.py [--reps N] [--size 1920x1080] [--frames 5] [--no-host] [--out FILE.json]"""
import argparse
import json
import os
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


def summary(t):
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 4), spread=round(float((t.max() - t.min()) / med), 4), min=round(float(t.min()), 4), max=round(float(t.max()), 4))


def steady_state(seq, frames, reps, warm, host, out=None):
    """steps of (push frame t + R, pop frame t) once the window is full; the frames cycle"""
    seq.reset()
    n, k = len(frames), 0
    push = seq.push_host if host else seq.push
    while seq.ready() == 0:                                          # fill the window
        push(*frames[k % n])
        k += 1
    t = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if host:
            seq.pop_host()
        else:
            seq.pop(out=out)
        push(*frames[k % n])
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
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = bh.Context(0)
    W, H = (int(x) for x in a.size.split("x"))
    prm = bh.default_params(m=1.0, random_order=1)
    host_frames = [core.synthetic_scene(W, H, 32, seed, 0.35, 0.01) for seed in (1234, 77, 4321, 99, 555, 31, 32, 33)[:a.frames]]
    fr = [[torch.from_numpy(x).cuda() for x in f] for f in host_frames]
    D = fr[0][2].shape[2]
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, frames=a.frames, timing={}, device_bytes={})
    row = res["timing"]

    # ---- the stage alone, beside what it replaces
    hist, ns = fr[0][2], fr[0][1]
    words = 6
    out = (torch.zeros((H, W, words), dtype=torch.int32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
    row["cross"] = timings(lambda: ctx.similarity_masks_cross(hist, ns, fr[1][2], fr[1][1], 1, 6, 1.0, out=out), a.reps, a.warmup)
    ab = out[0].clone()
    tr = (torch.zeros_like(ab), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
    row["transpose"] = timings(lambda: ctx.transpose_masks_cross(ab, 6, out=tr), a.reps, a.warmup)
    ba = ctx.similarity_masks_cross(fr[1][2], fr[1][1], hist, ns, 1, 6, 1.0)
    assert torch.equal(tr[0], ba[0]) and torch.equal(tr[1], ba[1]), "the transposed masks are not the masks of the swapped pair"
    print("stage", json.dumps({k: row[k] for k in ("cross", "transpose")}), flush=True)
    del out, ab, tr, ba

    # ---- the per-frame call beside the sequence
    frame_out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    mid = a.frames // 2
    row["call_F1_S1"] = timings(lambda: ctx.denoise_temporal(*fr[mid], [fr[mid + 1]], 1, prm, out=frame_out), a.reps, a.warmup)
    print("call_F1_S1", json.dumps(row["call_F1_S1"]), flush=True)
    for R in (1, 2):
        nbs = [k for k in range(mid - R, mid + R + 1) if k != mid]
        for S in (1, 3):
            key = "R%d_S%d" % (R, S)
            row["call_" + key] = timings(lambda: ctx.denoise_temporal(*fr[mid], [fr[k] for k in nbs], S, prm, out=frame_out), a.reps, a.warmup)
            seq = ctx.sequence(W, H, D, S, R, prm)
            row["sequence_" + key] = steady_state(seq, fr, a.reps, a.warmup, False, frame_out)
            info = seq.info()
            res["device_bytes"][key] = info["device_bytes"]
            seq.set_reuse(False)
            row["noreuse_" + key] = steady_state(seq, fr, a.reps, a.warmup, False, frame_out)
            seq.set_reuse(True)
            if not a.no_host:
                row["call_%s_host" % key] = timings(lambda: ctx.denoise_temporal_host(*host_frames[mid], [host_frames[k] for k in nbs], S, prm), a.reps, a.warmup)
                row["sequence_%s_host" % key] = steady_state(seq, host_frames, a.reps, a.warmup, True)
            seq.close()
            print(key, json.dumps({k: v for k, v in row.items() if key in k}), "device_bytes", info["device_bytes"], flush=True)
    one_neighbour = row["call_R1_S1"]["ms"] - row["call_F1_S1"]["ms"]
    bound = row["call_R1_S1"]["ms"] - one_neighbour / 2
    res["condition"] = dict(one_neighbour_ms=round(one_neighbour, 4), bound_ms=round(bound, 4), sequence_ms=row["sequence_R1_S1"]["ms"],
                            met=bool(row["sequence_R1_S1"]["ms"] <= bound))
    print("condition", json.dumps(res["condition"]), flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
