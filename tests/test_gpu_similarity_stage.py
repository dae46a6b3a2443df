"""GPU tests of similar-patch selection (k_similarity.hip, k_similarity_fast.hip, similarity() in bcd_api.hip) on constructed histograms, at the threshold.

Every case of tests/similarity_cases.py goes through the stage with the threshold ON its distance values: on a value shared by thousands of pairs and its
float neighbours, and on RN(d / (1 -+ 2^-10)) +- 0, 1, 2 ulp, the edges of the band inside which the fast path re-evaluates a pair exactly.  The reference is
tests/similarity_ref.py, which tests/test_similarity_cases_cpu.py holds to the compiled oracle bit for bit.  Masks, |S|, counts and distances are compared
with array_equal: the only tolerances in this file are the derived bounds of the binary16 planes against float64.

  * masks and |S| of the production path, of the fast path switched off and of bcd_hip_similarity_masks_exact, each against the reference (so also
    against each other), at every threshold of every case; the two 400 000-pixel frames (four-column kernels / narrow kernels) against one tiled period;
  * window distances at the corners of the main area, on the seams and at the guard pixels, bit for bit;
  * the approximate planes (uniform, general and RATIO form) against float64: counts exact, unwritten entries untouched, every entry within
    T64 (2^-11 + (2 D + 22) u) + 2^-24 (+ 10 u r max(B1, B2) for the RATIO form) -- operation counts of the kernel, not a run;
  * bcd_hip_selftest_approx_distance on the worst-case binary16 frames: below 2^-10 / 1.9, the bar of the whole-frame tests;
  * the paths: the checkerboard overflows the borderline list and ends on the exact kernels, the sparse plateau stays on the approximate planes with a
    borderline count between the CPU's counts of pairs inside tau (1 +- 2^-11) and tau (1 +- 2^-9);
  * a sequence of frames on one fresh context (uniform, mixed, uniform, 12 samples, overflow, RATIO declined, same size again, another size), the path
    read after each call.

Measured on the MI355X (BCD_TEST_REPORT; docs/EXPERIMENTS.md section 15): 242 tests in 9.4 s, the slowest 0.7 s, a 400 000-pixel case 0.1 - 0.3 s, a small case 0.01 - 0.11 s.
    planes against float64, largest |T16 - T64| / bound:  uniform 0.982, general 0.982 (both on the `half` family: the binary16 store at 0.98 of its
                                                          2^-11), RATIO 0.968; plateaus 0.73, fully occupied histograms 0.95
    selftest_approx_distance on the worst-case frames:    4.40e-4 (binary16 rounds down), 4.88e-4 (up); whole frames measure 2.4e-4, the bar is 5.14e-4
    borderline pairs of the sparse plateau:               23 839 listed = the CPU's count of pairs on the plateau, at tau = d, its neighbours and the
                                                          five thresholds around RN(d / (1 - 2^-10)); 0 at the five around RN(d / (1 + 2^-10))
Mutated builds and what each turned red: docs/EXPERIMENTS.md section 15.
"""
import os

import numpy as np
import pytest

import similarity_cases as sc
import similarity_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
SMALL = sc.names(large=False)
LARGE = sc.names(large=True)


def _report(line):
    if os.environ.get("BCD_TEST_REPORT"):
        with open(os.environ["BCD_TEST_REPORT"], "a") as f:
            f.write("%s %s\n" % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], line))


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(mask, cnt):
    return mask.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


def three_paths(ctx, d_hist, d_ns, w, b, tau, exact=True):
    """masks and |S| of the production path, of the fast path switched off, and of the exact entry point"""
    out = {}
    try:
        ctx.set_fast_similarity(True)
        out["production"] = host(*ctx.similarity_masks(d_hist, d_ns, w, b, float(tau)))
        ctx.set_fast_similarity(False)
        out["fast path off"] = host(*ctx.similarity_masks(d_hist, d_ns, w, b, float(tau)))
    finally:
        ctx.set_fast_similarity(True)
    if exact:
        out["exact entry"] = host(*ctx.similarity_masks_exact(d_hist, d_ns, w, b, float(tau)))
    return out


def describe(case, which, tau, got, want):
    """the first differing mask bit as a pair: pixel, displacement, d_ref (a mismatch is a finding about the kernels)"""
    diff = got ^ want
    l, c, word = [int(x[0]) for x in np.nonzero(diff)]
    bit = int(diff[l, c, word]).bit_length() - 1
    k = 32 * word + bit
    side = 2 * case.b + 1
    d = None if case.large else float(case.dist[l, c, k]) if k < side * side else None
    return "%s, %s, tau %r: pixel (%d, %d) offset (%d, %d) bit %d: got %d, d_ref %r; %d pixels differ" % (
        case.name, which, float(tau), l, c, k // side - case.b, k % side - case.b, k, (int(got[l, c, word]) >> bit) & 1, d, int(np.count_nonzero(diff.any(-1))))


# ---- masks, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_masks_at_every_threshold_on_three_paths(hipctx, name):
    case = sc.by_name(name)
    d_hist, d_ns = dev(case.hist, case.ns)
    for tau in case.taus:
        wmask, wcnt = case.reference(tau)
        for which, (mask, cnt) in three_paths(hipctx, d_hist, d_ns, case.w, case.b, tau).items():
            assert np.array_equal(mask, wmask), describe(case, which, tau, mask, wmask)
            assert np.array_equal(cnt, wcnt), (name, which, float(tau))


@pytest.mark.parametrize("name", LARGE)
def test_masks_of_the_large_frames_on_two_paths(hipctx, name):
    """1000 x 400: W % 4 == 0 and 400 000 pixels, the smallest frame on k_fwd_masks_w1v4a / k_fwd_masks_w1v4 (b = 3: 25 planes, the last one evaluated
    twice); 1001 x 400: the narrow kernels at that size"""
    case = sc.by_name(name)
    d_hist, d_ns = dev(*case.frame())
    for tau in case.taus:
        wmask, wcnt = case.reference(tau)
        for which, (mask, cnt) in three_paths(hipctx, d_hist, d_ns, case.w, case.b, tau, exact=False).items():
            assert np.array_equal(mask, wmask), describe(case, which, tau, mask, wmask)
            assert np.array_equal(cnt, wcnt), (name, which, float(tau))


# ---- distances -------------------------------------------------------------------------------------------------------------
def marks_of(case):
    w, W, H = case.w, case.W, case.H
    pix = {(w, w), (w, W - 1 - w), (H - 1 - w, w), (H - 1 - w, W - 1 - w)} | set(case.marks)
    if case.seam:
        cb, lb = case.seam
        pix |= {(min(max(lb, w), H - 1 - w), min(max(cb, w), W - 1 - w)), (min(max(lb - 1, w), H - 1 - w), min(max(cb - 1, w), W - 1 - w))}
    return sorted(pix)


@pytest.mark.parametrize("name", SMALL)
def test_window_distances_bit_for_bit(hipctx, name):
    """corners of the main area, a pixel on either side of each seam, the guard pixels; NaN (no counted bin) and +inf (outside the window) included"""
    case = sc.by_name(name)
    d_hist, d_ns = dev(case.hist, case.ns)
    for (l, c) in marks_of(case):
        got = hipctx.window_distances(d_hist, d_ns, case.w, case.b, l, c)
        assert np.array_equal(got.view(np.uint32), case.dist[l, c].view(np.uint32)), (name, l, c)


# ---- the planes against float64 --------------------------------------------------------------------------------------------
PLANE_CASES = [n for n in SMALL if n.split(" ")[0] in ("plateau", "half", "counts", "drawn") or n.startswith("seam column 64") or n.startswith("width 65")]
_worst = {}


@pytest.mark.parametrize("name", PLANE_CASES)
def test_approximate_planes_against_float64(hipctx, name):
    """k_pairdist_rw in its uniform (n = 16 cases), general and RATIO form (the other cases): bin counts equal the float64 reference's, entries whose
    neighbour leaves the image keep the fill byte, and every entry lies within the bound its operation counts give: each of the <= D terms carries
    (2 + 1) u against the real quotient and goes through <= D additions, against float64 T64 (1 + (2 D + 22) u) with the reference's own D + 9; the
    binary16 store adds 2^-11 relative, or half a subnormal step 2^-25 below 2^-14.  The RATIO form adds 10 u r max(B1, B2) (its header)."""
    import torch
    case = sc.by_name(name)
    D, b = case.D, case.b
    T64, C64, valid = sr.planes64(case.hist, case.ns, b, case.bins)
    d_hist, d_ns = dev(case.hist, case.ns)
    forms = [("uniform", 16.0, False)] if case.variant == "n16" else [("general", 0.0, False), ("ratio", 0.0, True)]
    rel_bound = 2.0 ** -11 + (2 * D + 22) * U
    for form, uni_n, ratio in forms:
        planes, counts, flag = hipctx.approx_planes(d_hist, d_ns, b, uni_n, ratio_form=ratio, tau=1.0)
        torch.cuda.synchronize()
        T16, Cn = planes.cpu().numpy(), counts.cpu().numpy()
        assert (flag & 3) == 0, (name, form, flag)                   # inside the guarded range, the count given is every pixel's
        assert np.array_equal(Cn[valid], C64[valid].astype(np.uint8)), (name, form)
        assert (Cn[~valid] == 0xFF).all() and (T16.view(np.uint16)[~valid] == 0xFFFF).all(), (name, form)
        bound = T64 * rel_bound + 2.0 ** -24
        if ratio:
            bound = bound + 10 * U * ratio_absolute_term(case)
        err = np.abs(T16.astype(np.float64) - T64)
        worst = float(np.max((err / bound)[valid]))
        _worst[form] = max(_worst.get(form, 0.0), worst)
        _report("planes %s: largest |T16 - T64| / bound %.3f (largest so far %.3f)" % (form, worst, _worst[form]))
        assert worst <= 1.0, (name, form, worst)


def ratio_absolute_term(case):
    """r max(B1, B2) per plane entry: B the mass of a histogram, r = max(n1 / n2, n2 / n1)"""
    b = case.b
    H, W, D = case.hist.shape
    mass = case.hist.astype(np.float64).sum(-1)
    n = case.ns.reshape(H, W).astype(np.float64)
    out = np.zeros((sr.delta_count(b), H, W))
    for (dl, dc) in sr.forward_offsets(b):
        v = sr._views(n, dl, dc)
        if v is None:
            continue
        n1, n2, sl = v
        m1, m2, _ = sr._views(mass, dl, dc)
        out[sr.delta_index(dl, dc, b)][sl] = np.maximum(n1 / n2, n2 / n1) * np.maximum(m1, m2)
    return out


@pytest.mark.parametrize("kind", sc.GUARD_KINDS)
def test_range_flag_on_the_guards_and_one_ulp_outside(hipctx, kind):
    """bins of exactly 2^20, counts of exactly 2^-10 and 2^16 are inside the range where pd_div<true> is proven exact: flag bit 0 of the approximate
    kernel stays clear and its bin counts are the reference's; one ulp outside, the flag is raised.  (The division itself is held bit for bit by
    test_masks_at_every_threshold...: the guard cases carry thresholds ON the distances of the guard pixels -- similarity_cases.guard_thresholds --,
    which the production path above 64 and the fast path switched off decide from the planes of k_pairdist<FAST = true>.)"""
    case = sc.by_name("guard %s 48x24" % kind)
    uni = 65536.0 if "uni" in kind else 0.0
    planes, counts, flag = hipctx.approx_planes(*dev(case.hist, case.ns), case.b, uni)
    assert (flag & 1) == (0 if case.inside else 1) and (flag & 2) == 0, (kind, flag)
    if case.inside:
        T, C, valid = sr.planes32(case.hist, case.ns, case.b, case.bins)
        assert np.array_equal(counts.cpu().numpy()[valid], C[valid].astype(np.uint8))


@pytest.mark.parametrize("word", ["down", "up"])
def test_patch_distances_of_the_worst_case_binary16_frames_stay_under_the_bar(hipctx, word):
    """all nine entries of a patch lose (gain) 0.9 .. 1 times 2^-11 in the binary16 store: the derived worst case of the planes is 4.97e-4, the bar of the
    whole-frame tests 2^-10 / 1.9 = 5.14e-4 (whole frames measure 2.4e-4)"""
    case = sc.by_name("half rounds %s 40x24 n16" % word)
    rel, count_mismatches, flags = hipctx.selftest_approx_distance(*dev(case.hist, case.ns), case.b)
    _report("selftest_approx_distance, binary16 rounds %s: %.4e" % (word, rel))
    assert count_mismatches == 0 and flags == 2
    assert rel >= 0.9 * 2.0 ** -11 - (2 * case.D + 20) * U           # the frame is what it claims to be on the device too (less the fp32 round-off)
    assert rel < 2.0 ** -10 / 1.9, rel


# ---- the paths taken -------------------------------------------------------------------------------------------------------
def ratio_expected(case, tau):
    """2 where the RATIO form's verdict 10 kappa G <= 4096 tau is clear of its threshold, 1 where it fails clearly (the reference's operations on the
    approximate planes), None within a percent of it.  kappa = max B / n, G = max over the pixel pairs with a counted bin of r max(n1, n2) / C"""
    H, W, D = case.hist.shape
    n = case.ns.reshape(H, W).astype(np.float64)
    kappa = float(np.max(case.hist.astype(np.float64).sum(-1) / n))
    T, C, valid = sr.planes32(case.hist, case.ns, case.b, case.bins)
    G = 0.0
    for (dl, dc) in sr.forward_offsets(case.b):
        v = sr._views(n, dl, dc)
        if v is None:
            continue
        n1, n2, sl = v
        c = C[sr.delta_index(dl, dc, case.b)][sl]
        if (c > 0).any():
            G = max(G, float(np.max((np.maximum(n1 / n2, n2 / n1) * np.maximum(n1, n2) / np.maximum(c, 1))[c > 0])))
    lhs, rhs = 10 * kappa * G, 4096 * float(tau)
    return 2 if lhs < 0.99 * rhs else 1 if lhs > 1.01 * rhs else None


def run_and_check(ctx, case, tau):
    mask, cnt = host(*ctx.similarity_masks(*dev(case.hist, case.ns), case.w, case.b, float(tau)))
    wmask, wcnt = case.reference(tau)
    assert np.array_equal(mask, wmask), describe(case, "production", tau, mask, wmask)
    assert np.array_equal(cnt, wcnt)
    return ctx.similarity_last_path()


def test_checkerboard_leaves_the_fast_path_and_the_sparse_plateau_stays_on_it():
    import bcd_amd.hip as bh
    ctx = bh.Context(0)                                              # (a workspace without a memory of mixed counts or declined sizes)
    try:
        case = sc.by_name("plateau checker 64x40 n16")
        for tau in case.taus[:3]:                                    # d, prev(d), next(d): 85 884 pairs in the band, 65 536 list entries
            assert sc.in_band(case.dist, case.b, tau) > sc.capacity(case.W, case.H)
            assert run_and_check(ctx, case, tau) == (0, 0, 0)
        far = F(2.0) * case.values[0]                                # the same frame away from its plateau: nothing listed, the fast path serves it
        assert run_and_check(ctx, case, far) == (1, 0, sc.capacity(case.W, case.H))
        for name, path in (("plateau sparse 64x40 n16", 1), ("plateau sparse 64x40 n12", 2), ("plateau sparse 64x40 mixed", 2)):
            case = sc.by_name(name)
            checked = 0
            for tau in case.taus:
                if path == 2 and ratio_expected(case, tau) != 2:
                    continue                                         # (a threshold so low that the RATIO form declines: the sequence test has such a frame)
                checked += 1
                got, listed, cap = run_and_check(ctx, case, tau)
                lo, hi = sc.in_band(case.dist, case.b, tau, 0.5), sc.in_band(case.dist, case.b, tau, 2.0)
                _report("%s tau %r: path %d, %d listed, CPU %d inside +-2^-11, %d inside +-2^-9" % (name, float(tau), got, listed, lo, hi))
                assert got == path and cap == sc.capacity(case.W, case.H)
                assert lo <= listed <= hi, (name, float(tau), lo, listed, hi)
            assert checked >= 13, (name, checked)                    # at least one whole ladder per variant went through the assertions
    finally:
        ctx.close()


def declining_frame():
    """the sparse plateau with sample counts spread 1 : 64 in a 2 x 2 tile (160 and 10 240 samples per pixel), histograms in proportion: the RATIO form's
    verdict fails by three orders of magnitude, as on the frame of test_ratio_form_declines_... in tests/test_gpu_parity.py"""
    W, H = 64, 40
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    scale = np.where((l ^ c) & 1, F(640), F(10))[:, :, None].astype(F)
    base = sc.PLATEAU_TYPES[sc.sparse(W, H)]
    case = sc.Case("plateau sparse 64x40 counts 1:64", "plateau", np.ascontiguousarray(base * scale), np.ascontiguousarray(F(16) * scale), nvalues=2, variant="mixed")
    return case


def test_sequence_of_frames_on_one_context():
    import bcd_amd.hip as bh
    uniform, mixed, twelve = (sc.by_name("plateau sparse 64x40 " + v) for v in ("n16", "mixed", "n12"))
    overflow, other = sc.by_name("plateau checker 64x40 n16"), sc.by_name("half rounds up 40x24 mixed")
    declining = declining_frame()
    tau_mixed = max(mixed.values)
    assert ratio_expected(mixed, tau_mixed) == 2 and ratio_expected(twelve, twelve.values[0]) == 2
    assert ratio_expected(declining, declining.values[0]) == 1 and ratio_expected(other, other.values[0]) == 2
    assert (declining.W, declining.H) == (mixed.W, mixed.H) != (other.W, other.H)
    cap = sc.capacity(64, 40)
    ctx = bh.Context(0)
    try:
        steps = [(uniform, uniform.values[0], 1), (mixed, tau_mixed, 2), (uniform, uniform.values[0], 1),   # (the third: the workspace now scans first)
                 (twelve, twelve.values[0], 2), (overflow, overflow.values[0], 0), (declining, declining.values[0], 1),
                 (mixed, tau_mixed, 1),                               # the size has declined: the approximate planes of the reference's operations
                                                                      # (the getter reports the pass that counted, not whether RATIO was tried first)
                 (other, other.values[0], 2)]                         # another size: the RATIO form again
        for i, (case, tau, path) in enumerate(steps):
            got, listed, capacity = run_and_check(ctx, case, tau)
            _report("step %d %s: path %d, %d listed" % (i + 1, case.name, got, listed))
            assert got == path, (i + 1, case.name, got, path)
            assert capacity == (0 if path == 0 else sc.capacity(case.W, case.H)) and (path == 0 or 0 < listed <= cap)
    finally:
        ctx.close()
