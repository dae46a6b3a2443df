"""Which kernels of the 27-component estimate chain a frame launches, and how: for comparing two builds launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o TAG -- python tools/chain_launches.py frame W H B [ROOT]
    python tools/chain_launches.py table DIR [OUT]

`frame` denoises one small single-scale synthetic frame with -m 0 (every main pixel takes the full estimate) and search radius B through the engine
of the tree ROOT (default: this one); `table` turns the kernel trace under DIR into rows (kernel, grid in threads, workgroup, static LDS bytes,
dispatches) of the chain's kernels.  (The trace's LDS column holds the static segment only; dynamic LDS is not in it.)"""
import csv
import glob
import os
import re
import sys
from collections import Counter


def frame(W, H, b, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    assert os.path.abspath(bh.__file__).startswith(root), bh.__file__
    col, ns, hist, cov = core.synthetic_scene(W, H, 16, 7, 0.15, 0.0)
    ctx = bh.Context(0)
    d = [torch.from_numpy(a).cuda() for a in (col, ns, hist, cov)]
    got = ctx.denoise(*d, 1, bh.default_params(b=b, w=1, m=0.0, random_order=1, seed=3)).cpu().numpy()
    print("frame ok", root, W, H, b, "finite", bool(np.isfinite(got).all()), "mean %.6f" % float(got.mean()))
    ctx.close()


def table(directory, out=None):
    chain = re.compile(r"k_bayes27|k_jacobi27|k_finish27|k_prepare_solve27|k_prepare27t")
    paths = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)
    assert paths, "no kernel trace under " + directory
    rows = Counter()
    for p in paths:
        for r in csv.DictReader(open(p)):
            if chain.search(r["Kernel_Name"]):
                name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                rows[(name, "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ"), r["LDS_Block_Size"])] += 1
    lines = ["%-24s %12s %10s %8s %6s" % ("kernel", "grid", "workgroup", "LDS", "calls")]
    lines += ["%-24s %12s %10s %8s %6d" % (k + (n,)) for k, n in sorted(rows.items())]
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    if sys.argv[1] == "frame":
        frame(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), os.path.abspath(sys.argv[5] if len(sys.argv) > 5 else os.path.join(os.path.dirname(__file__), "..")))
    else:
        table(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
