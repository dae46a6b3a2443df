"""GPU tests of the margin planes: the approximate distance planes as ONE signed binary16 value E = T - tau C per pixel pair (k_pairdist_rw<MARGIN> in
k_similarity_fast.hip) and the mask kernels that decide from the sum of nine E and of their absolute values (k_fwd_masks_w1m / _w1v4m in k_similarity.hip).

Every test compares masks and |S| of the production path bit for bit with the exact path (bcd_hip_set_fast_similarity(ctx, 0)) and checks that the
pass stayed on the approximate planes with its borderline list not overflowed.  The frames are seeded draws: `spp` samples per pixel and channel
scattered over a few bins around a slowly varying centre, so that patch distances lie on both sides of every threshold used.  Shapes are the smallest
at which the kernels can go wrong: more than one 64-column tile and a ragged last one, a frame smaller than a tile and than the search window, three
search radii, the three histogram depths, thresholds at both ends of the admitted range, the three forms of the distance kernel (uniform power-of-two
counts, a uniform count that is no power of two, mixed counts), pixel pairs without a live bin, entries beyond binary16, and a workspace whose plane
buffer held fp32 planes just before.  (The four-column kernel needs 400 000 pixels: the large cases of tests/test_gpu_similarity_stage.py run it.)

Measured on the MI355X (docs/EXPERIMENTS.md section 3): 13 tests in 9.2 s, 6.6 s of them the two child processes of the environment-switch test, every
other test below 0.3 s.  Borderline pairs, margin planes / T / C planes: textured 256 x 128 at tau = 1: 1 340 / 2 882; sparse plateau (n = 16) on the
plateau and its float neighbours: equal; family `half` (one live bin per pixel pair): 27 444 at both edges of the T / C planes' band, where those list
27 444 at one edge and 0 at the other -- the band's constant term stands in for the count the margins do not carry."""
import os
import subprocess
import sys

import numpy as np
import pytest

import similarity_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
TAUS = (2.0 ** -6, 0.5, 1.0, 1.5, 64.0)


def _report(line):
    print(line)
    if os.environ.get("BCD_TEST_REPORT"):
        with open(os.environ["BCD_TEST_REPORT"], "a") as f:
            f.write("%s %s\n" % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], line))


def drawn_frame(W, H, D=60, spp=32, seed=0, counts="uniform"):
    """histograms of `spp` samples per channel around a centre that drifts across the frame; counts: 'uniform', or 'mixed' = a seeded quarter of the
    pixels carries 3 spp samples (histogram and count), the others spp: counts mixed 1 : 3"""
    rng = np.random.default_rng(seed)
    per = D // 3
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n = np.full((H, W), spp, np.int64)
    if counts == "mixed":
        n = np.where(rng.random((H, W)) < 0.25, 3 * spp, spp)
    hist = np.zeros((H, W, D), F)
    for ch in range(3):
        centre = per / 2 + (per / 4) * np.sin(0.21 * c + 0.13 * l + ch) + ((c // 16 + l // 12) & 1) * 2.0
        for k in range(int(n.max())):
            pos = np.clip(np.rint(centre + rng.normal(0.0, 1.3, (H, W))), 0, per - 1).astype(np.int64)
            np.add.at(hist, (l[k < n], c[k < n], ch * per + pos[k < n]), F(1))
    return np.ascontiguousarray(hist), np.ascontiguousarray(n.astype(F)[:, :, None])


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(mask, cnt):
    return mask.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


def exact(ctx, d_hist, d_ns, b, tau):
    try:
        ctx.set_fast_similarity(False)
        return host(*ctx.similarity_masks(d_hist, d_ns, 1, b, float(tau)))
    finally:
        ctx.set_fast_similarity(True)


def check(ctx, hist, ns, b, taus=TAUS, paths=(1, 2)):
    """masks and |S| of the margin planes == the exact path's at every threshold; -> [(path, listed)]"""
    d_hist, d_ns = dev(hist, ns)
    H, W = hist.shape[:2]
    out = []
    for tau in taus:
        want = exact(ctx, d_hist, d_ns, b, tau)
        ctx.set_margin_planes(True)
        got = host(*ctx.similarity_masks(d_hist, d_ns, 1, b, float(tau)))
        path, listed, cap = ctx.similarity_last_path()
        assert path in paths, (float(tau), path)
        assert cap == sc.capacity(W, H) and 0 <= listed <= cap, (float(tau), listed, cap)
        assert np.array_equal(got[0], want[0]), (float(tau), int(np.count_nonzero((got[0] ^ want[0]).any(-1))))
        assert np.array_equal(got[1], want[1]), float(tau)
        out.append((path, listed))
    return out


@pytest.mark.parametrize("W,H,b", [(72, 40, 6), (9, 7, 6), (40, 33, 3), (40, 33, 12)])
def test_uniform_frame_at_every_threshold(hipctx, W, H, b):
    hist, ns = drawn_frame(W, H, seed=W + b)
    got = check(hipctx, hist, ns, b, paths=(1,))
    _report("uniform %dx%d b=%d: borderline pairs per threshold %s" % (W, H, b, [n for _, n in got]))


@pytest.mark.parametrize("D", [24, 36])
def test_the_other_histogram_depths(hipctx, D):
    hist, ns = drawn_frame(72, 40, D=D, seed=D)
    check(hipctx, hist, ns, 6, paths=(1,))


@pytest.mark.parametrize("counts,spp", [("uniform", 24), ("mixed", 16)])
def test_general_sample_counts(hipctx, counts, spp):
    """24 samples everywhere (rho = 1 through the RATIO form) and counts mixed 1 : 3.  The RATIO form keeps its T and C planes (path 2); where its own
    check declines at a low threshold the pass is repeated with the reference's operations on margin planes (path 1), and the workspace remembers the
    frame size: the thresholds run from the highest down, and a frame width no other test uses keeps that memory out of this one"""
    hist, ns = drawn_frame(76 if counts == "uniform" else 84, 40, spp=spp, seed=spp, counts=counts)
    got = check(hipctx, hist, ns, 6, taus=TAUS[::-1])
    assert got[0][0] == 2, got                                       # tau = 64: the RATIO form
    assert counts == "uniform" or got[-1][0] == 1, got               # mixed counts at tau = 2^-6: it declines, the general margin form serves
    hist, ns = drawn_frame(9 if counts == "uniform" else 11, 7, spp=spp, seed=spp + 1, counts=counts)
    check(hipctx, hist, ns, 6, taus=TAUS[::-1])


def test_pairs_without_a_live_bin(hipctx):
    """a block of empty histograms wider than the search window, and single empty pixels: patch pairs with no counted bin at all (0 / 0 in the reference:
    never similar, and never listed) beside patches in which only some entries are empty"""
    hist, ns = drawn_frame(72, 40, seed=5)
    hist[8:30, 10:40] = 0
    hist[3, 50] = 0
    hist[35, 60:63] = 0
    got = check(hipctx, hist, ns, 6, paths=(1,))
    # the block holds ~17 x 25 pixels whose whole windows are empty: were those pairs listed, every threshold would list > 30 000
    assert max(n for _, n in got) < 20000, got


def test_entries_beyond_binary16(hipctx):
    """bins of 2^19 against empty bins: terms of 2^19 per pixel pair, +inf in the plane; pairs of two such pixels (d = 0) stay similar"""
    hist, ns = drawn_frame(72, 40, seed=6)
    hist[10:14, 20:44:3, 7] = F(2.0 ** 19)
    hist[25, 30, 58] = F(2.0 ** 20)
    check(hipctx, hist, ns, 6, paths=(1,))


def test_workspace_that_held_fp32_planes_just_before(hipctx):
    """the exact kernels leave fp32 T planes and counts of a LARGER frame in the workspace; the margin pass that follows must not read any of it"""
    big, nbig = drawn_frame(96, 64, seed=8)
    exact(hipctx, *dev(big, nbig), 6, 1.0)
    hist, ns = drawn_frame(72, 40, seed=9)
    d_hist, d_ns = dev(hist, ns)
    hipctx.set_margin_planes(True)
    got = host(*hipctx.similarity_masks(d_hist, d_ns, 1, 6, 1.0))
    assert hipctx.similarity_last_path()[0] == 1
    want = exact(hipctx, d_hist, d_ns, 6, 1.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_borderline_counts_of_margin_planes_and_tc_planes(hipctx):
    """the same masks from both kinds of planes; the number of pairs each sends to the exact re-evaluation is recorded (the band is 2^-10 A + const
    for the margin planes, 2^-10 tau C for the T / C planes), on the constructed threshold cases and on a 256 x 128 textured frame"""
    import bcd_amd.core as core
    frames = []
    for name in ("plateau sparse 64x40 n16", "half rounds down 40x24 n16", "half rounds up 40x24 n16", "plateau sparse 64x40 mixed"):
        case = sc.by_name(name)
        frames.append((name, case.hist, case.ns, case.b, case.taus[:3] + case.taus[3:4] + case.taus[8:9]))
    _, ns, hist, _ = core.synthetic_scene(256, 128, 32, 1234, 0.35, 0.01, pattern=1)
    frames.append(("textured 256x128", hist, ns, 6, [F(1.0)]))
    try:
        for name, hist, ns, b, taus in frames:
            d_hist, d_ns = dev(hist, ns)
            H, W = hist.shape[:2]
            for tau in taus:
                want = exact(hipctx, d_hist, d_ns, b, tau)
                listed = {}
                for kind, on in (("margin", True), ("T/C", False)):
                    hipctx.set_margin_planes(on)
                    got = host(*hipctx.similarity_masks(d_hist, d_ns, 1, b, float(tau)))
                    path, n, cap = hipctx.similarity_last_path()
                    assert path >= 1 and n <= cap, (name, kind, float(tau), path, n, cap)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, kind, float(tau))
                    listed[kind] = n
                _report("%s tau %r: borderline pairs margin %d, T/C %d" % (name, float(tau), listed["margin"], listed["T/C"]))
    finally:
        hipctx.set_margin_planes(True)


def test_environment_switch_for_the_tc_planes_reproduces_the_oracle():
    """BCD_HIP_TC_PLANES=1 (read once per process: run in a child) keeps the T and C planes; a 3-scale host-buffer frame tall enough for the streamed
    upload -- the planes are then computed ahead of the last chunk -- against the oracle, with and without the switch"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, oracle_lib as ol, bcd_amd.core as core, bcd_amd.hip as bh\n"
            "W, H, S = 80, 272, 3\n"
            "col, ns, hist, cov = core.synthetic_scene(W, H, 16, 11, 0.12, 0.005)\n"
            "ctx = bh.Context(0)\n"
            "got = ctx.denoise_host(col, ns, hist, cov, S, bh.default_params(m=1.0, random_order=1, seed=4))\n"
            "orders = [bh.visit_order(W >> s, H >> s, 1, 1, bh.scale_seed(4, s)) for s in range(S)]\n"
            "want = ol.denoise_multiscale(col, ns, hist, cov, S, ol.params(m=1.0), orders=orders)\n"
            "print('ERR %%.3e PATH %%d' %% (np.max(np.abs(got - want)) / np.max(np.abs(want)), ctx.stats(0).similarity_path))\n") % (root, os.path.join(root, "tests"))
    for value in ("1", "0"):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, BCD_HIP_TC_PLANES=value), timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("ERR")][-1].split()
        assert float(line[1]) < 1e-4 and int(line[3]) == 1, (value, line)
