"""GPU tests of the cross-frame selection stage (bcd_hip_similarity_masks_cross, bcd_hip_window_distances_cross; k_similarity_cross.hip) and of the estimate
over members of several frames (bcd_hip_bayes_accumulate_temporal; k_bayes_temporal.hip) against tests/temporal_ref.py, which
tests/test_temporal_cases_cpu.py holds to tests/similarity_ref.py (and through it to the compiled oracle) and to tests/bayes_ref.py.

  * masks, |S_f| and window distances bit for bit on the cases of tests/temporal_cases.py: 20x16, 33x21, 5x40 and 70x10 (two tiles of the distance
    kernel); b = 3, 6, 12 with w = 1; b = 3 with w = 0 and 2; D = 60, 24 (staged kernel) and 15 (generic kernel); one power of two as sample count, 24 spp,
    counts drawn per pixel and differently in the two frames, a 1-spp frame (NaN distances).  The thresholds are distances of the case and their two float
    neighbours, so the comparison sits on ties; the outputs lie between sentinel margins that must survive;
  * a frame against itself: the cross masks are those of bcd_hip_similarity_masks bit for bit (production path and exact entry point);
  * the refusals of the stage, then a successful call on the same context.
The selection is compared with array_equal: no tolerance.  The estimate (second half of the file): per item against float64 with the bar of
tests/test_gpu_bayes_stage.py, counts and non-finite patterns exact, on the families of tests/temporal_bayes_cases.py -- |S_0| in {1, 5, 27, 28, 169} crossed
with totals 27, 28, 29, 170 and 169 (1 + F) for F = 1, 2, 4; windows leaving the image; the pixel itself as the only in-frame member; pure noise; zero noise
mean; a non-finite covariance in a neighbour member -- four calls on one context with changing list lengths and record sizes (the temporal chain waits
for its list lengths and has no launch-ahead logic to walk; what is held is that it leaves bayes()'s alone) followed by a plain bcd_hip_bayes_accumulate, one frame against the plain
call, and the refusals.
Measured on the MI355X: largest e_hip / max(e_32, median e_32, 8 u) per family 0.20 ... 1.33 (bar 4); dense frames e_hip 3.8e-7 ... 4.8e-7."""
import numpy as np
import pytest

import bayes_ref as br
import temporal_bayes_cases as tb
import temporal_cases as tc
import temporal_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 96
SENTINEL = 0x5A5A5A5A


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays]      # (a copy: the cases' arrays are read-only)


def guarded(H, W, words):
    """mask and count tensors inside larger buffers filled with a sentinel -> (mask, count, check())"""
    import torch
    nm, nc = H * W * words, H * W
    bm = torch.full((nm + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    bc = torch.full((nc + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")

    def check():
        for buf, n in ((bm, nm), (bc, nc)):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all(), "a margin was written"
    return bm[GUARD:GUARD + nm].view(H, W, words), bc[GUARD:GUARD + nc].view(H, W), check


def describe(case, tau, got, want):
    diff = got ^ want
    l, c, word = [int(x[0]) for x in np.nonzero(diff)]
    bit = int(diff[l, c, word]).bit_length() - 1
    k = 32 * word + bit
    side = 2 * case.b + 1
    d = float(case.dist[l, c, k]) if k < side * side else None
    return "%s, tau %r: pixel (%d, %d) offset (%d, %d) bit %d: got %d, d_ref %r; %d pixels differ" % (
        case.name, float(tau), l, c, k // side - case.b, k % side - case.b, k, (int(got[l, c, word]) >> bit) & 1, d, int(np.count_nonzero(diff.any(-1))))


def same_bits(a, b):
    """bit for bit; NaN against NaN whatever its sign and payload"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("name", tc.NAMES)
def test_cross_masks_and_counts_at_every_threshold(hipctx, name):
    case = tc.by_name(name)
    d = dev(*case.frames)
    words = ((2 * case.b + 1) ** 2 + 31) // 32
    for tau in case.taus:
        wmask, wcnt = case.reference(tau)
        mask, cnt, check = guarded(case.H, case.W, words)
        hipctx.similarity_masks_cross(*d, case.w, case.b, float(tau), out=(mask, cnt))
        check()
        mask, cnt = mask.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
        assert np.array_equal(mask, wmask), describe(case, tau, mask, wmask)
        assert np.array_equal(cnt, wcnt), (name, float(tau))


@pytest.mark.parametrize("name", tc.NAMES)
def test_cross_window_distances_bit_for_bit(hipctx, name):
    """corners of the main area and its middle; NaN (no counted bin) and +inf (outside the window) included"""
    case = tc.by_name(name)
    d = dev(*case.frames)
    for (l, c) in case.marks():
        got = hipctx.window_distances_cross(*d, case.w, case.b, l, c)
        assert same_bits(got, case.dist[l, c]), (name, l, c)


@pytest.mark.parametrize("W,H,D,b,w,kind", [(33, 21, 60, 6, 1, 16), (33, 21, 60, 6, 1, "mixed"), (70, 10, 24, 3, 1, 24), (20, 16, 15, 3, 2, "mixed"), (20, 16, 60, 12, 1, 1)])
def test_a_frame_against_itself_gives_the_in_frame_masks(hipctx, W, H, D, b, w, kind):
    hist, ns = tc.frame(W, H, D, kind, seed=7)
    d_hist, d_ns = dev(hist, ns)
    for tau in (0.0, 0.4, 1.0, 3.0):
        mask, cnt = hipctx.similarity_masks_cross(d_hist, d_ns, d_hist, d_ns, w, b, tau)
        for own in (hipctx.similarity_masks, hipctx.similarity_masks_exact):
            wmask, wcnt = own(d_hist, d_ns, w, b, tau)
            assert np.array_equal(mask.cpu().numpy(), wmask.cpu().numpy()), (own.__name__, tau)
            assert np.array_equal(cnt.cpu().numpy(), wcnt.cpu().numpy()), (own.__name__, tau)
        assert int(cnt.sum()) > 0


def test_refusals_leave_the_context_usable(hipctx):
    import torch
    import bcd_amd.hip as bh
    case = tc.by_name("20x16")
    d_hist, d_ns, d_hist_nb, d_ns_nb = dev(*case.frames)
    with pytest.raises(bh.BcdHipError):                              # search radius above 15
        hipctx.similarity_masks_cross(d_hist, d_ns, d_hist_nb, d_ns_nb, 1, 16, 1.0)
    with pytest.raises(bh.BcdHipError):                              # negative radius
        hipctx.similarity_masks_cross(d_hist, d_ns, d_hist_nb, d_ns_nb, -1, 6, 1.0)
    with pytest.raises(bh.BcdHipError):                              # not a main pixel
        hipctx.window_distances_cross(d_hist, d_ns, d_hist_nb, d_ns_nb, 1, 6, 0, 5)
    with pytest.raises(ValueError):                                  # a neighbour of another size
        hipctx.similarity_masks_cross(d_hist, d_ns, d_hist_nb[:, :10].contiguous(), d_ns_nb[:, :10].contiguous(), 1, 6, 1.0)
    big = torch.zeros((3, 3, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(bh.BcdHipError):                              # histogram depth above 255
        hipctx.similarity_masks_cross(big, torch.ones((3, 3, 1), device="cuda"), big, torch.ones((3, 3, 1), device="cuda"), 1, 1, 1.0)
    tau = case.taus[1]
    mask, cnt = hipctx.similarity_masks_cross(d_hist, d_ns, d_hist_nb, d_ns_nb, case.w, case.b, float(tau))
    wmask, wcnt = case.reference(tau)
    assert np.array_equal(mask.cpu().numpy().view(np.uint32), wmask) and np.array_equal(cnt.cpu().numpy(), wcnt)


# ---- the estimate over members of several frames (bcd_hip_bayes_accumulate_temporal) -----------------------------------------------------------
# Per item against float64 (tests/temporal_ref.py on tests/bayes_ref.py), items 2 (b + w) + 1 apart; the bar is that of tests/test_gpu_bayes_stage.py:
#     e_hip <= 4 max(e_32, median of e_32 over the family, 8 u)
# e_32 the same quantity for the float32 calibrator; counts and the set of non-finite entries are exact; fallback items: |sum - mean_64| <= |S| u max|x|.
# Nothing in a bar comes from a GPU run.
U = br.U32
MARGIN = 4.0
FLOOR = 8 * U
EXCLUDE_ABOVE = 1e-2     # (as in tests/test_gpu_bayes_stage.py: such an item is checked for count and finiteness only; none is expected here)

_refs = {}


def references(case):
    """float64 reference and float32 calibrator of a case, once per session"""
    if id(case) not in _refs:
        s64, c64, items = tr.accumulate(*case.args())
        s32, _, _ = tr.accumulate(*case.args(), dtype=np.float32)
        _refs[id(case)] = (case, s64, c64, items, s32)
    return _refs[id(case)][1:]


def run_temporal(ctx, case):
    import torch
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    frames = [(t(c), t(p), t(m.view(np.int32))) for (c, p, m) in case.frames()]
    s, c = ctx.bayes_accumulate_temporal(frames, t(case.nsim_total), t(case.state), case.w, case.b, case.min_eig)
    return s.cpu().numpy(), c.cpu().numpy()


def check_exact_parts(case, s_hip, c_hip, s64, c64):
    assert np.array_equal(c_hip, c64), (case.name, "count", np.argwhere(c_hip != c64)[:5])
    assert np.array_equal(np.isfinite(s_hip), np.isfinite(s64)), (case.name, "non-finite pattern", np.argwhere(np.isfinite(s_hip) != np.isfinite(s64))[:5])


def check_fallback_items(case, s_hip, s64, items):
    """mean of <= 27 values per entry: |S| u max|x|, max|x| over the members' values of that entry (members of every frame)"""
    for it in items:
        if not 0 < it["n"] < tb.K1:
            continue
        masks = [m for (_, _, m) in case.frames()]
        mem = tr.members_of(masks, it["pos"][0], it["pos"][1], case.b)
        x = np.concatenate([np.abs(br.gather(case.col[f], mem[mem[:, 0] == f, 1:], case.w).astype(np.float64)) for f in np.unique(mem[:, 0])])
        bound = it["n"] * U * x.max(axis=0)
        r, c = br.touched(it, case.w)
        d = np.abs(s_hip[r, c].astype(np.float64) - s64[r, c])
        assert (d <= bound).all(), (case.name, it["pos"], it["n"], float((d / bound.clip(1e-300)).max()))


@pytest.mark.parametrize("family", sorted(tb.FAMILIES))
def test_temporal_estimate_per_item_against_float64(hipctx, family):
    rows = []
    for case in tb.FAMILIES[family]():
        s_hip, c_hip = run_temporal(hipctx, case)
        s64, c64, items, s32 = references(case)
        check_exact_parts(case, s_hip, c_hip, s64, c64)
        check_fallback_items(case, s_hip, s64, items)
        for it in items:
            if it["n"] < tb.K1 or not np.isfinite(s64[br.touched(it, case.w)]).all():
                continue
            rows.append((case, it, br.item_error(s_hip, s64, it, case.w), br.item_error(s32, s64, it, case.w)))
    assert len(rows) >= 3, (family, len(rows))
    e32 = np.array([r[3] for r in rows])
    assert (e32 <= EXCLUDE_ABOVE).all(), (family, float(e32.max()))
    bar = MARGIN * np.maximum(np.maximum(e32, np.median(e32)), FLOOR)
    worst = max(r[2] / b_ * MARGIN for r, b_ in zip(rows, bar))
    print("temporal-stage %-12s | %d items | max e_32 %.1e | max e_hip %.1e | largest e_hip / max(e_32, median, 8 u) %.2f" % (
        family, len(rows), float(e32.max()), max(r[2] for r in rows), worst))
    for (case, it, eh, e3), b_ in zip(rows, bar):
        assert eh <= b_, "%s item %s |S| = %d (%d in the frame): e_hip %.3e > bar %.3e (e_32 %.3e, family median %.3e); cond1 %.2e cond2 %.2e" % (
            case.name, it["pos"], it["n"], len(it["members"]), eh, b_, e3, float(np.median(e32)), it["cond1"], it["cond2"])


def test_non_finite_covariance_in_a_neighbour_poisons_the_whole_item(hipctx):
    case = tb.FAMILIES["non-finite"]()[0]
    s_hip, c_hip = run_temporal(hipctx, case)
    s64, c64, items, _ = references(case)
    poisoned = [it for it in items if it["n"] >= tb.K1 and not np.isfinite(s64[br.touched(it, case.w)]).any()]
    assert len(poisoned) == 2                                        # (the NaN item and the inf item; the fallback item with a NaN member stays finite)
    for it in poisoned:
        assert np.isnan(s_hip[br.touched(it, case.w)]).all(), it["pos"]


def dense_check(case, s_hip, c_hip):
    s64, c64, items, s32 = references(case)
    check_exact_parts(case, s_hip, c_hip, s64, c64)
    if case.dense:
        e_hip, e_32 = br.rel_local(s_hip, s64), br.rel_local(s32, s64)
        print("temporal-stage %-20s dense: e_32 %.2e e_hip %.2e" % (case.name, e_32, e_hip))
        assert e_hip <= MARGIN * max(e_32, FLOOR), (case.name, e_hip, e_32)
    else:
        for it in items:
            if it["n"] >= tb.K1:
                eh, e3 = br.item_error(s_hip, s64, it, case.w), br.item_error(s32, s64, it, case.w)
                e32_all = [br.item_error(s32, s64, j, case.w) for j in items if j["n"] >= tb.K1]
                assert eh <= MARGIN * max(e3, float(np.median(e32_all)), FLOOR), (case.name, it["pos"], eh, e3)


def test_four_calls_on_one_context_then_a_plain_estimate():
    """isolated items, a dense frame (other list lengths, the records regrown), the isolated items again, a dense frame of another size and frame count -- each
    against float64 --; then a plain bcd_hip_bayes_accumulate on the same context, whose result must match that of a fresh context within the same bar."""
    import torch
    import bcd_amd.hip as bh
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    seq = tb.call_sequence()
    plain = tb.single_frame_of(seq[1])
    col, pixcov, mask, nsim, state, w, b, min_eig = plain
    s64, c64, _ = br.accumulate(*plain, keep_stages=False)
    s32, _, _ = br.accumulate(*plain, dtype=np.float32, keep_stages=False)
    out = {}
    for which in ("after temporal calls", "fresh"):
        ctx = bh.Context(0)
        try:
            if which == "after temporal calls":
                for case in seq:
                    dense_check(case, *run_temporal(ctx, case))
            s, c = ctx.bayes_accumulate(t(col), t(pixcov), t(mask.view(np.int32)), t(nsim), t(state), w, b, min_eig)
            ctx.synchronize()
            out[which] = (s.cpu().numpy(), c.cpu().numpy())
        finally:
            ctx.close()
    e_32 = br.rel_local(s32, s64)
    for which, (s, c) in out.items():
        assert np.array_equal(c, c64), which
        assert br.rel_local(s, s64) <= MARGIN * max(e_32, FLOOR), (which, br.rel_local(s, s64), e_32)
    assert np.array_equal(out["fresh"][1], out["after temporal calls"][1])
    assert br.rel_local(out["after temporal calls"][0], out["fresh"][0]) <= MARGIN * max(e_32, FLOOR)


def test_one_frame_is_the_plain_estimate(hipctx):
    """nb_frames = 1: the temporal prepare kernel leaves the records of the in-frame kernels, so the chain computes what bcd_hip_bayes_accumulate computes
    (same arithmetic up to the order in which a chunk is staged; the float atomics of the aggregation may arrive in another order)"""
    import torch
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    case = tb.fam_sizes(1, 201)
    col, pixcov, mask, nsim, state, w, b, min_eig = tb.single_frame_of(case)
    s1, c1 = hipctx.bayes_accumulate_temporal([(t(col), t(pixcov), t(mask.view(np.int32)))], t(nsim), t(state), w, b, min_eig)
    s0, c0 = hipctx.bayes_accumulate(t(col), t(pixcov), t(mask.view(np.int32)), t(nsim), t(state), w, b, min_eig)
    hipctx.synchronize()
    s64, c64, items = br.accumulate(col, pixcov, mask, nsim, state, w, b, min_eig, keep_stages=False)
    s32, _, _ = br.accumulate(col, pixcov, mask, nsim, state, w, b, min_eig, dtype=np.float32, keep_stages=False)
    assert np.array_equal(c1.cpu().numpy(), c64) and np.array_equal(c0.cpu().numpy(), c64)
    e32 = [br.item_error(s32, s64, it, w) for it in items if it["n"] >= tb.K1]
    for it in items:
        if it["n"] >= tb.K1:
            bar = MARGIN * max(br.item_error(s32, s64, it, w), float(np.median(e32)), FLOOR)
            assert br.item_error(s1.cpu().numpy(), s64, it, w) <= bar, it["pos"]
            assert br.item_error(s1.cpu().numpy(), s0.cpu().numpy().astype(np.float64), it, w) <= bar, it["pos"]


def test_estimate_refusals_leave_the_context_usable(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    case = tb.fam_zero_noise()
    frames = [(t(c), t(p), t(m.view(np.int32))) for (c, p, m) in case.frames()]
    nsim, state = t(case.nsim_total), t(case.state)
    H, W = case.state.shape

    def with_masks_of(b):
        words = ((2 * b + 1) ** 2 + 31) // 32
        return [(c, p, torch.zeros((H, W, words), dtype=torch.int32, device="cuda")) for (c, p, _) in frames]

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                 # any other geometry: BCD_HIP_EUNSUPPORTED, with a message
        rc = None
        try:
            hipctx.bayes_accumulate_temporal(with_masks_of(b), nsim, state, w, b, case.min_eig)
        except bh.BcdHipError as e:
            rc = str(e)
        assert rc is not None and "support" in rc, (w, b, rc)
    with pytest.raises(bh.BcdHipError):                              # more than four neighbours
        hipctx.bayes_accumulate_temporal(frames * 3, nsim, state, 1, 6, case.min_eig)
    L = bh.lib()
    one = (bh.StageFrame * 1)()
    one[0].d_colors, one[0].d_pixel_cov, one[0].d_mask = frames[0][0].data_ptr(), frames[0][1].data_ptr(), None
    s = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    args = (nsim.data_ptr(), state.data_ptr(), W, H, 1, 6, 1e-8, s.data_ptr(), c.data_ptr())
    assert L.bcd_hip_bayes_accumulate_temporal(hipctx.h, one, 1, *args) == -1            # a null image in a frame
    assert L.bcd_hip_bayes_accumulate_temporal(hipctx.h, one, 0, *args) == -1            # no frame
    assert L.bcd_hip_bayes_accumulate_temporal(hipctx.h, None, 1, *args) == -1           # no frame list
    with pytest.raises(bh.BcdHipError):                              # an accumulator that is an input
        hipctx.bayes_accumulate_temporal(frames, nsim, state, 1, 6, case.min_eig, out=(frames[0][0], c))
    with pytest.raises(bh.BcdHipError):                              # the count image is the total |S|
        hipctx.bayes_accumulate_temporal(frames, nsim, state, 1, 6, case.min_eig, out=(s, nsim))
    assert float(s.abs().sum()) == 0.0 and int(c.sum()) == 0         # refused before any device work
    s_hip, c_hip = run_temporal(hipctx, case)
    s64, c64, _, _ = references(case)
    check_exact_parts(case, s_hip, c_hip, s64, c64)
