#!/usr/bin/env python3
"""GPU box: what a kept selection costs and saves (bcd_hip_denoise_layers_keep / bcd_hip_selection_denoise), and the
moments-only snapshot of the accumulator against the full one.
Frames (1920 x 1080, 32 spp, 3 scales, b = 6, -m 1 -r 1, as bench.py): headline (ramps + checker), textured (pattern 1).  For L = 1 and 4 layers:
  layers   one bcd_hip_denoise_layers call                                   (i)
  keep     the same call leaving its selection in a bcd_hip_selection        (ii)   keep - layers = the copies
  reuse    bcd_hip_selection_denoise on that selection                       (iii)
and, once per frame and L with profiling on and serial scales, ms_similarity + ms_active per scale as bcd_hip_get_stats reports them: what a reuse call
does not run.  Then bcd_hip_accum_statistics against bcd_hip_accum_moments at 1920 x 1080 and 3840 x 2160 (20 bins, one dense pass accumulated)  (iv).
Inputs are resident, every shape is warmed up, a figure is the median of --reps host-clock timings around calls that end in a synchronisation; `spread` is
(max - min) / median of those repeats, the noise a difference has to beat.
With a library that has no selection entry points (BCD_HIP_LIB pointing at a build of the parent commit, for the "the existing call did not slow down"
comparison: run the two alternately) it measures `layers` only.
usage: python tools/exp_selection.py [--reps N] [--frames headline,textured] [--layers 1,4] [--no-accum] [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bcd_amd.core as core  # noqa: E402
import bcd_amd.hip as bh  # noqa: E402
from exp_layers import make_layers, timings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--frames", default="headline,textured")
    ap.add_argument("--layers", default="1,4")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--no-accum", action="store_true", help="skip the snapshot comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    kept_available = hasattr(bh.lib(), "bcd_hip_selection_denoise")
    ctx = bh.Context(0)
    W, H, S = a.width, a.height, 3
    counts = [int(x) for x in a.layers.split(",")]
    frames = {"headline": dict(pattern=0, m=1.0), "textured": dict(pattern=1, m=1.0)}
    res = dict(library=bh.LIB_PATH, width=W, height=H, scales=S, reps=a.reps, selection_calls=kept_available, frames={}, snapshot={})
    for name in a.frames.split(","):
        f = frames[name]
        col, ns, hist, cov = core.synthetic_scene(W, H, 32, 1234, 0.35, 0.01, pattern=f["pattern"])
        prm = bh.default_params(m=f["m"], random_order=1)
        d_ns, d_hist = torch.from_numpy(ns).cuda(), torch.from_numpy(hist).cuda()
        layers = [(torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()) for c, v in make_layers(col, cov, max(counts))]
        outs = [torch.empty_like(layers[0][0]) for _ in layers]
        rows = {}
        for L in counts:
            def plain():
                ctx.denoise_layers(d_ns, d_hist, layers[:L], S, prm, outs=outs[:L])
            row = dict(layers=timings(plain, a.reps, a.warmup))
            if kept_available:
                sel = ctx.selection()

                def keep():
                    ctx.denoise_layers(d_ns, d_hist, layers[:L], S, prm, outs=outs[:L], keep=sel)

                def reuse():
                    sel.denoise(layers[:L], outs=outs[:L])
                row["keep"] = timings(keep, a.reps, a.warmup)
                row["reuse"] = timings(reuse, a.reps, a.warmup)
                row["layers_again"] = timings(plain, a.reps, 1)          # (the same call after the others: drift of the visit)
                row["copy_ms"] = round(row["keep"]["ms"] - row["layers"]["ms"], 4)
                row["saved_ms"] = round(row["layers"]["ms"] - row["reuse"]["ms"], 4)
                row["selection_bytes"] = sel.info()["device_bytes"]
                # what the reuse call leaves out, by the library's own events (serial scales: the stages of one scale are not overlapped by another scale's)
                ctx.set_profiling(True)
                ctx.set_concurrent_scales(False)
                plain()
                st = [ctx.stats(s) for s in range(S)]
                row["serial_profiled"] = dict(ms_similarity=[round(s.ms_similarity, 4) for s in st], ms_active=[round(s.ms_active, 4) for s in st],
                                              ms_bayes=[round(s.ms_bayes, 4) for s in st])
                row["serial_selection_ms"] = round(sum(s.ms_similarity + s.ms_active for s in st), 4)
                ctx.set_profiling(False)
                row["serial"] = dict(layers=timings(plain, a.reps, 2), reuse=timings(reuse, a.reps, 2))
                ctx.set_concurrent_scales(True)
                sel.close()
            rows[str(L)] = row
            print(name, "L=%d" % L, json.dumps(row), flush=True)
        res["frames"][name] = rows
        del d_ns, d_hist, layers, outs
    if kept_available and not a.no_accum:
        for (w, h) in ((1920, 1080), (3840, 2160)):
            acc = ctx.accumulator(w, h, nbins=20)
            acc.add_dense(torch.rand((h, w, 1, 3), device="cuda"))
            full = acc.statistics()
            part = acc.moments()
            def per_call(fn, warm):                                  # ten enqueues per timed window (a snapshot is a fraction of a millisecond)
                t = timings(lambda: [fn() for _ in range(10)], a.reps, warm)
                return dict(t, ms=round(t["ms"] / 10, 5), min=round(t["min"] / 10, 5), max=round(t["max"] / 10, 5))
            row = dict(statistics=per_call(lambda: acc.statistics(out=full), a.warmup), moments=per_call(lambda: acc.moments(out=part), a.warmup))
            row["statistics_again"] = per_call(lambda: acc.statistics(out=full), 1)
            row["ratio"] = round(row["statistics"]["ms"] / row["moments"]["ms"], 2)
            n = w * h
            row["moments_GBps"] = round(n * 84 / (row["moments"]["ms"] * 1e-3) / 1e9, 1)         # 44 B read + 40 B written per pixel
            row["statistics_GBps"] = round(n * 564 / (row["statistics"]["ms"] * 1e-3) / 1e9, 1)  # 44 + 240 B read, 40 + 240 B written
            res["snapshot"]["%dx%d" % (w, h)] = row
            print("snapshot %dx%d" % (w, h), json.dumps(row), flush=True)
            acc.close()
            del full, part
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
