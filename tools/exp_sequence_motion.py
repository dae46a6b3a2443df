#!/usr/bin/env python3
"""GPU box: what a sequence that takes motion fields costs and saves (DESIGN.md section 16 "Sequences with motion", docs/EXPERIMENTS.md section 34).
At 1920 x 1080, 32 spp, D = 60, b = 6, -m 1 -r 1, one colour layer of histograms, every shape warmed up; a figure is the median of --reps host-clock timings
around calls that end in a synchronisation, `spread` is (max - min) / median of those repeats.
  compose                 bcd_hip_compose_motion alone (k_motion_compose<true>), with the rate of its 24 B per pixel (two fields read, one written)
  copy_24B                a device-to-device copy of 12 B per pixel (read + write: the same 24 B per pixel of traffic), in the same run
  per R in 1, 2, at --scales scales, every field zero-valued (every neighbour is warped, nothing is transposed, the frames select as without motion):
    call_R{R}             bcd_hip_denoise_temporal_motion on a frame with its 2R neighbours and their fields, called per frame as a user without the sequence would
    sequence_R{R}         one steady-state step of the resident sequence: the pop of frame t and the motion push of frame t + R (the frames cycle)
    call_host_R{R}, sequence_host_R{R}   the same through the host entry points (bcd_hip_denoise_temporal_motion_host; push_frame_motion_host and pop_layers_host)
    condition_R{R}        sequence <= call, resident and host, beyond the larger of the two spreads?
  existing calls, this build beside --parent-lib (the library of the parent commit's build) alternately, parent - this - parent in child processes:
    null_sequence_R2      a steady-state step of a plain-push sequence (no field anywhere), R = 2
    temporal_N2           bcd_hip_denoise_temporal with two neighbours
    denoise               bcd_hip_denoise
usage: python tools/exp_sequence_motion.py [--reps N] [--size 1920x1080] [--scales 3] [--parent-lib FILE.so] [--out FILE.json]"""
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


def steady_state(seq, pushes, reps, warm, host, outs):
    """steps of (pop frame t, push frame t + R) once the window is full; pushes: (args, kwargs) per frame, cycled"""
    seq.reset()
    push = seq.push_host if host else seq.push
    n, k = len(pushes), 0
    while seq.ready() == 0:
        push(*pushes[k % n][0], **pushes[k % n][1])
        k += 1
    t = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if host:
            seq.pop_host()
        else:
            seq.pop(out=outs)
        push(*pushes[k % n][0], **pushes[k % n][1])
        torch.cuda.synchronize()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
        k += 1
    return summary(t)


def existing_calls(ctx, host_frames, dev, S, prm, reps, warm):
    """the calls that exist in the parent commit too -> {name: timing}"""
    H, W, D = host_frames[0][2].shape
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    row = {}
    row["denoise"] = timings(lambda: ctx.denoise(*dev[2], S, prm, out=out), reps, warm)
    row["temporal_N2"] = timings(lambda: ctx.denoise_temporal(*dev[2], [dev[1], dev[3]], S, prm, out=out), reps, warm)
    seq = ctx.sequence(W, H, D, S, 2, prm)
    row["null_sequence_R2"] = steady_state(seq, [(f, {}) for f in dev], reps, warm, False, out)
    seq.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--scales", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--existing-only", action="store_true", help="the calls an older build has too, of the library BCD_HIP_LIB names")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    W, H = (int(x) for x in a.size.split("x"))
    S, T = a.scales, 5
    res = dict(library=bh.LIB_PATH, reps=a.reps, size=a.size, scales=S, timing={}, parent=[], condition={})
    row = res["timing"]

    def parent_calls():
        if not a.parent_lib or a.existing_only:
            return
        cmd = [sys.executable, os.path.abspath(__file__), "--existing-only", "--reps", str(a.reps), "--warmup", str(a.warmup), "--size", a.size, "--scales", str(S)]
        r = subprocess.run(cmd, env=dict(os.environ, BCD_HIP_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        res["parent"].append(json.loads(r.stdout.strip().splitlines()[-1])["timing"])
        print("parent", json.dumps(res["parent"][-1]), flush=True)

    parent_calls()                                                   # (before any GPU work of this process: one process at a time holds the frames)
    ctx = bh.Context(0)
    prm = bh.default_params(m=1.0, random_order=1)
    host_frames = [core.synthetic_scene(W, H, 32, seed, 0.35, 0.01) for seed in (1234, 77, 4321, 99, 555)[:T]]
    dev = [tuple(torch.from_numpy(x).cuda() for x in f) for f in host_frames]
    row.update(existing_calls(ctx, host_frames, dev, S, prm, a.reps, a.warmup))
    if not a.existing_only:
        npix = W * H
        # ---- the composition kernel beside a copy of the same traffic
        rng = np.random.default_rng(1)
        fa, fb = (torch.from_numpy(np.rint(rng.standard_normal((H, W, 2)) * 4).astype(np.float32)).cuda() for _ in range(2))
        fo = torch.empty_like(fa)
        row["compose"] = timings(lambda: ctx.compose_motion(fa, fb, out=fo), a.reps, a.warmup)
        src = torch.empty(npix * 3, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        row["copy_24B"] = timings(lambda: dst.copy_(src), a.reps, a.warmup)
        for k in ("compose", "copy_24B"):
            row[k]["GB_per_s"] = round(npix * 24 / (row[k]["ms"] * 1e-3) / 1e9, 1)
        print("compose", json.dumps(row["compose"]), "copy", json.dumps(row["copy_24B"]), flush=True)
        # ---- a sequence with zero-valued fields beside the per-frame motion call
        zero_h = np.zeros((H, W, 2), np.float32)
        zero_d = torch.from_numpy(zero_h).cuda()
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for R in (1, 2):
            nbs = [k for k in range(2 - R, 2 + R + 1) if k != 2]
            row["call_R%d" % R] = timings(lambda: ctx.denoise_temporal_motion(*dev[2], [dev[k] for k in nbs], [zero_d] * len(nbs), S, prm, out=out), a.reps, a.warmup)
            row["call_host_R%d" % R] = timings(lambda: ctx.denoise_temporal_motion_host(*host_frames[2], [host_frames[k] for k in nbs], [zero_h] * len(nbs), S, prm),
                                               a.reps, a.warmup)
            seq = ctx.sequence(W, H, 60, S, R, prm, layers=1)
            mode_args = lambda f: (f[1], f[2], [(f[0], f[3])])
            row["sequence_R%d" % R] = steady_state(seq, [(mode_args(f), dict(motion_prev=zero_d, motion_next=zero_d)) for f in dev], a.reps, a.warmup, False, [out])
            warped, composed = seq.motion_info()
            row["sequence_host_R%d" % R] = steady_state(seq, [(mode_args(f), dict(motion_prev=zero_h, motion_next=zero_h)) for f in host_frames], a.reps, a.warmup, True,
                                                        None)
            res["condition"]["R%d" % R] = dict(warped_per_pop=2 * R, transposed=seq.info()["cross_transposed"])
            seq.close()
            for form in ("", "_host"):
                s, c = row["sequence%s_R%d" % (form, R)], row["call%s_R%d" % (form, R)]
                slack = max(s["spread"], c["spread"]) * c["ms"]
                res["condition"]["R%d" % R]["met" + form] = bool(s["ms"] <= c["ms"] + slack)
            print("R", R, json.dumps({k: v for k, v in row.items() if k.endswith("R%d" % R)}), json.dumps(res["condition"]["R%d" % R]), flush=True)
    ctx.close()
    del dev
    torch.cuda.empty_cache()
    parent_calls()                                                   # (parent - this - parent: this build's figures stand between the two)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
