#!/usr/bin/env python3
"""GPU box: what the in-place spike prefilter costs beside its out-of-place twin, and what the prefilter of every frame adds to a sequence and to a host
frame call (bcd_hip_spike_filter_layers_inplace, bcd_hip_sequence_set_prefilter, bcd_hip_denoise_temporal_host_ex; DESIGN.md sections 13 "In place" and 16
"Prefilter").  Four parts, each a key of the JSON line:

  inplace    bcd_hip_spike_filter_layers_inplace beside bcd_hip_spike_filter_layers in the same run, on the frame of tools/exp_spike_layers.py (synthetic
             scene, 16 spp, D = 60) at factor 2 and at the factor of --factors whose moved share is closest to 1 %, 1920 x 1080 and 3840 x 2160, L = 1 and
             4, with and without histograms.  The decision depends on layer 0's colours alone, so those are restored (12 B per pixel, device to device)
             ahead of every in-place call; `restore` is that copy and its synchronisation alone, `inplace_net` = inplace - restore.  The in-place call
             synchronises (it reads the moved count back), so the twin is given both ways: `twin_batched` is ten enqueues and one synchronisation,
             divided by ten, `twin_synced` one call and one synchronisation.
  sequence   a push and the pop it makes ready, per frame, over --frames frames at 1920 x 1080 and 3 scales, R = 1 and 2, device pushes and host pushes, with
             the prefilter beside without; `extra_bytes`: the map, the list and the staging buffer the prefilter adds on the context.
  host       bcd_hip_denoise_temporal_host_ex with a factor beside the host call it delegates to (one layer, histograms, N = 2), 1920 x 1080, 3 scales.
  existing   bcd_hip_denoise, bcd_hip_denoise_temporal (N = 2) and a plain R = 1 sequence (per frame): the calls a build without this feature has too.  Run
             with BCD_HIP_LIB pointing at the parent commit's libbcd_hip.so for the other half of the comparison (--parts existing).
A figure is the median of --reps host-clock timings that end in a synchronisation; `spread` is (max - min) / median of those repeats.
usage: python tools/exp_prefilter_frames.py [--reps N] [--parts inplace,sequence,host,existing] [--sizes 1920x1080,3840x2160] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import make_layers, timings  # noqa: E402


def part_inplace(ctx, a):
    L_ = bh.lib()
    chk, p = ctx._chk, (lambda t: t.data_ptr())
    out = {}
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        n = W * H
        col, ns, hist, cov = core.synthetic_scene(W, H, 16, 1234, 0.35, 0.01)
        D = hist.shape[-1]
        counts = [int(x) for x in a.layers.split(",")]
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, max(counts))]
        pristine = layers[0][0].clone()
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        o_ns, o_hist = torch.empty_like(d_ns), torch.empty_like(d_hist)
        outs = [(torch.empty_like(c), torch.empty_like(v)) for c, v in layers]
        d_map = torch.empty((H, W), dtype=torch.int32, device="cuda")
        d_moved = torch.zeros(1, dtype=torch.int32, device="cuda")
        shares = {}
        for f in [float(x) for x in a.factors.split(",")]:
            torch.cuda.synchronize()
            chk(L_.bcd_hip_spike_map(ctx.h, p(pristine), W, H, f, p(d_map), p(d_moved)))
            ctx.synchronize()
            shares[f] = int(d_moved.item()) / n
        low = min((f for f in shares if f != 2.0), key=lambda f: abs(shares[f] - 0.01))
        rows = {"moved_share_by_factor": {str(f): round(s, 5) for f, s in shares.items()}}

        def restore():
            layers[0][0].copy_(pristine)
            torch.cuda.synchronize()

        for factor in (2.0, low):
            row = dict(moved_share=round(shares[factor], 5), restore=timings(restore, a.reps, a.warmup))
            for L in counts:
                for with_hist in (True, False):
                    arr = (bh.SpikeLayer * L)()
                    inp = (bh.SpikeLayerInplace * L)()
                    for k in range(L):
                        arr[k].d_colors, arr[k].d_covariances, arr[k].d_colors_out, arr[k].d_covariances_out = p(layers[k][0]), p(layers[k][1]), p(outs[k][0]), p(outs[k][1])
                        inp[k].d_colors, inp[k].d_covariances = p(layers[k][0]), p(layers[k][1])
                    hp, ohp = (p(d_hist), p(o_hist)) if with_hist else (None, None)
                    restore()
                    twin = lambda: chk(L_.bcd_hip_spike_filter_layers(ctx.h, p(d_ns), hp, W, H, D, factor, p(o_ns), ohp, arr, L, p(d_map), None))
                    tb = timings(lambda: [twin() for _ in range(10)], a.reps, a.warmup)
                    ts_ = timings(twin, a.reps, a.warmup)
                    moved = C.c_int32(0)

                    def inplace():
                        restore()
                        chk(L_.bcd_hip_spike_filter_layers_inplace(ctx.h, p(d_ns), hp, W, H, D, factor, inp, L, p(d_map), C.byref(moved)))

                    ti = timings(inplace, a.reps, a.warmup)
                    net = ti["ms"] - row["restore"]["ms"]
                    depth_sum, images = 1 + (D if with_hist else 0) + 9 * L, 1 + (1 if with_hist else 0) + 2 * L
                    row["L%d_%s" % (L, "hist" if with_hist else "nohist")] = dict(
                        twin_batched=dict(ms=round(tb["ms"] / 10, 5), spread=tb["spread"]), twin_synced=ts_, inplace=ti, inplace_net=round(net, 5), moved=moved.value,
                        # map: 12 B read + 4 B written; twin: 8 B per value and the map once more per image; in place: the map twice more, for the count and for the list,
                        # then per MOVED pixel 16 B per value (source -> staging -> destination) and the list written once and read twice per image
                        twin_bytes_per_pixel=16 + 8 * depth_sum + 4 * images,
                        inplace_bytes_per_pixel=round(24 + (moved.value / n) * (16 * depth_sum + 8 + 16 * images), 1),
                        ratio_vs_batched=round(net / (tb["ms"] / 10), 3), ratio_vs_synced=round(net / ts_["ms"], 3))
            rows["factor_%g" % factor] = row
        out[size] = rows
        print("inplace", size, json.dumps(rows), flush=True)
        del layers, outs, d_ns, d_hist, o_ns, o_hist, d_map, pristine
        torch.cuda.empty_cache()
    return out


def sequence_frames(W, H, T):
    return [core.synthetic_scene(W, H, 16, 1234 + k, 0.35, 0.01) for k in range(T)]


def run_sequence(seq, frames, host):
    """pushes and pops every frame; -> seconds of the whole run"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, f in enumerate(frames):
        (seq.push_host if host else seq.push)(*f)
        if k == len(frames) - 1:
            seq.end()
        while seq.ready():
            seq.pop_host() if host else seq.pop()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_frame(seq, frames, host, reps):
    t = []
    for r in range(reps + 1):
        seq.reset()
        s = run_sequence(seq, frames, host) * 1e3 / len(frames)
        if r:
            t.append(s)
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms=round(med, 4), spread=round(float((t.max() - t.min()) / med), 4))


def part_sequence(ctx, a, plain_only=False):
    W, H, S = 1920, 1080, 3
    host_frames = sequence_frames(W, H, a.frames)
    dev_frames = [tuple(torch.from_numpy(x).cuda() for x in f) for f in host_frames]
    prm = bh.default_params(m=1.0, random_order=1)
    out = {}
    for R in ((1,) if plain_only else (1, 2)):
        for host in ((False,) if plain_only else (False, True)):
            frames = host_frames if host else dev_frames
            seq = ctx.sequence(W, H, 60, S, R, prm)
            row = dict(plain=per_frame(seq, frames, host, a.seq_reps))
            if not plain_only:
                seq.reset()
                seq.set_prefilter(2.0)
                row["prefilter"] = per_frame(seq, frames, host, a.seq_reps)
                filtered, moved = seq.prefilter_info()
                row["moved_per_frame"] = moved // max(1, filtered)
                row["extra_ms"] = round(row["prefilter"]["ms"] - row["plain"]["ms"], 4)
                row["extra_bytes"] = dict(map=W * H * 4, list=8 * row["moved_per_frame"], staging=4 * 70 * row["moved_per_frame"])
            out["R%d_%s" % (R, "host" if host else "device")] = row
            print("sequence", R, "host" if host else "device", json.dumps(row), flush=True)
            seq.close()
    return out


def part_host(ctx, a):
    W, H, S = 1920, 1080, 3
    fr = sequence_frames(W, H, 3)
    prm = bh.default_params(m=1.0, random_order=1)
    lay = lambda f: [(f[0], f[3])]
    nbs = [(fr[0][1], fr[0][2], lay(fr[0])), (fr[2][1], fr[2][2], lay(fr[2]))]
    base = timings(lambda: ctx.denoise_temporal_layers_host(fr[1][1], fr[1][2], lay(fr[1]), nbs, S, prm), a.seq_reps, 1)
    null = timings(lambda: ctx.denoise_temporal_host_ex(fr[1][1], fr[1][2], lay(fr[1]), nbs, S, prm, spike_factor=None), a.seq_reps, 1)
    with_f = timings(lambda: ctx.denoise_temporal_host_ex(fr[1][1], fr[1][2], lay(fr[1]), nbs, S, prm, spike_factor=2.0), a.seq_reps, 1)
    row = dict(delegated=base, host_ex_null=null, host_ex_factor=with_f, extra_ms=round(with_f["ms"] - base["ms"], 4))
    print("host", json.dumps(row), flush=True)
    return row


def part_existing(ctx, a):
    W, H, S = 1920, 1080, 3
    fr = [tuple(torch.from_numpy(x).cuda() for x in f) for f in sequence_frames(W, H, 3)]
    prm = bh.default_params(m=1.0, random_order=1)
    out = torch.empty_like(fr[0][0])
    row = dict(denoise=timings(lambda: ctx.denoise(*fr[1], S, prm), a.reps, 2),
               denoise_temporal_N2=timings(lambda: ctx.denoise_temporal(*fr[1], [fr[0], fr[2]], S, prm, out=out), a.reps, 2))
    del fr
    torch.cuda.empty_cache()
    row["sequence_R1_per_frame"] = part_sequence(ctx, a, plain_only=True)["R1_device"]["plain"]
    print("existing", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seq-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--parts", default="inplace,sequence,host,existing")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--layers", default="1,4")
    ap.add_argument("--factors", default="2.0,2.3,2.4,2.5,2.55,2.6")  # (in a window of nine no value lies further than 8/3 standard deviations from the mean)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = bh.Context(0)
    res = dict(library=bh.LIB_PATH, reps=a.reps, seq_reps=a.seq_reps)
    parts = dict(inplace=part_inplace, sequence=part_sequence, host=part_host, existing=part_existing)
    for name in a.parts.split(","):
        res[name] = parts[name](ctx, a)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
