"""GPU tests of the estimate stage over several frames for several colour layers on one selection (bcd_hip_bayes_accumulate_temporal_layers:
k_bayes_weak_temporal_layers for the fallback pixels of every layer, the chain k_prepare27t / solver / finish per layer; DESIGN 16, "Layers") on the
constructed cases of tests/temporal_layers_cases.py.  The reference of layer k is tests/temporal_ref.py on that layer alone (tests/temporal_layers_ref.py);
the bars are those of tests/test_gpu_temporal_stage.py, nothing in them comes from a GPU run:
    full estimates, per item:   e_hip <= 4 max(e_32, median of e_32 over the (family, layer), 8 u)
    dense frame:                neighbourhood-relative error <= 4 max(e_32, 8 u)
What is asserted:
  * isolated cases (families sizes, borders, centre only, non-finite, zero noise and, as an extra, pure noise; layers scaled, independent, rotated): the ONE count image and every
    fallback item's sums equal bcd_hip_bayes_accumulate_temporal on that layer alone bit for bit (one atomic lands on a cleared pixel); counts and
    non-finite patterns equal the float64 reference's; full estimates per item against float64, the ratios printed;
  * layer counts 1, 2, 4, 5, 16 (a single layer, a short group, a full group of the fallback kernel, a group boundary, the maximum); F = 1, 2, 4;
  * weak lists of 1, 6, 7, 8 items (either side of the seven pixels of a wavefront), F = 1 and F = 4;
  * |S| = 27 (fallback) and |S| = 28 (full) with members in three frames; |S| = 0 gives NaN in every layer;
  * the non-finite family (a NaN and an inf covariance in neighbour frames, a fallback item with such a member): the items are NaN in the layers that
    carry the value, finite in the independent layer, the fallback item finite in every layer;
  * a NaN covariance in one layer of one neighbour poisons that layer's item and no other layer; layers built to take the redo list take it whatever
    their neighbours in the list do, and h_redo says so per layer (equal to bcd_hip_bayes_last_redo_count after the single-layer call on that layer);
  * a dense 33 x 21 frame, L = 3, F = 2, against float64;
  * two layered estimates of different sizes, L and F on one context, then a plain bcd_hip_bayes_accumulate equal to a fresh context's;
  * the refusals, then a successful call.
Every sum image and the count image lie between sentinel margins that must survive."""
import numpy as np
import pytest

import bayes_ref as br
import temporal_bayes_cases as tb
import temporal_layers_cases as tl
import temporal_layers_ref as tlr
import test_gpu_temporal_stage as ts

pytestmark = pytest.mark.gpu

U, MARGIN, FLOOR, EXCLUDE_ABOVE, GUARD, SENTINEL = ts.U, ts.MARGIN, ts.FLOOR, ts.EXCLUDE_ABOVE, ts.GUARD, ts.SENTINEL


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def guarded_out(H, W, L):
    """L zeroed sum images and one zeroed count image inside buffers filled with a sentinel -> (sums, count, check())"""
    import torch
    bufs = []

    def make(n):
        b = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        b[GUARD:GUARD + n] = 0
        bufs.append((b, n))
        return b[GUARD:GUARD + n]
    sums = [make(H * W * 3).view(torch.float32).view(H, W, 3) for _ in range(L)]
    cnt = make(H * W).view(H, W)

    def check():
        for b, n in bufs:
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all(), "a margin was written"
    return sums, cnt, check


def run_layered(ctx, lcase):
    """-> ([sum per layer], count, [redo per layer], the call's total)"""
    case = lcase.case
    H, W = case.state.shape
    masks = [_t(m.view(np.int32)) for m in case.mask]
    frames = [([(_t(lcase.col[k][f]), _t(lcase.pixcov[k][f])) for k in range(lcase.n)], masks[f]) for f in range(case.F + 1)]
    sums, cnt, check = guarded_out(H, W, lcase.n)
    sums, cnt, redo = ctx.bayes_accumulate_temporal_layers(frames, _t(case.nsim_total), _t(case.state), case.w, case.b, case.min_eig, out=(sums, cnt))
    total = ctx.bayes_last_redo_count()
    ctx.synchronize()
    check()
    return [s.cpu().numpy() for s in sums], cnt.cpu().numpy(), redo, total


def run_single(ctx, layer):
    """bcd_hip_bayes_accumulate_temporal on one layer alone -> (sum, count, redo)"""
    s, c = ts.run_temporal(ctx, layer)
    return s, c, ctx.bayes_last_redo_count()


_refs = {}


def references(lcase, k):
    """(sum_64, count_64, items, sum_32) of layer k, once per session"""
    key = (id(lcase), k)
    if key not in _refs:
        s64, c64, items = tlr.accumulate(lcase, k)
        s32, _, _ = tlr.accumulate(lcase, k, dtype=np.float32)
        _refs[key] = (lcase, s64, c64, items, s32)
    return _refs[key][1:]


def check_exact(ctx, lcase, layered):
    """what needs no numerical bar: the count image, the patterns, the fallback items bit for bit, the redo counts -- against the single-layer call and float64"""
    sums, cnt, redo, total = layered
    assert len(sums) == len(redo) == lcase.n
    for k in range(lcase.n):
        layer = lcase.layer(k)
        s1, c1, r1 = run_single(ctx, layer)
        s64, c64, items, _ = references(lcase, k)
        assert np.array_equal(cnt, c1), (layer.name, "the count image differs from the single-layer call's", np.argwhere(cnt != c1)[:5])
        ts.check_exact_parts(layer, sums[k], cnt, s64, c64)
        assert redo[k] == r1, (layer.name, "redo count: layered %d, single-layer call %d" % (redo[k], r1), redo)
        if lcase.dense:
            continue
        for it in items:
            if it["n"] < tb.K1:
                at = br.touched(it, layer.w)
                assert ts.same_bits(np.ascontiguousarray(sums[k][at]), np.ascontiguousarray(s1[at])), (layer.name, it["pos"], it["n"], sums[k][at], s1[at])
        ts.check_fallback_items(layer, sums[k], s64, items)
    assert total == sum(redo), (lcase.name, total, redo)


def check_items(tag, lcases, results):
    """the per-item bar per layer position over the cases of a family; prints the largest ratio of every layer"""
    judged = 0
    for k in range(lcases[0].n):
        rows = []
        for lcase, (sums, _, _, _) in zip(lcases, results):
            s64, _, items, s32 = references(lcase, k)
            for it in items:
                if it["n"] < tb.K1 or not np.isfinite(s64[br.touched(it, 1)]).all():
                    continue
                rows.append((lcase.layer(k), it, br.item_error(sums[k], s64, it, 1), br.item_error(s32, s64, it, 1)))
        if not rows:
            continue
        e32 = np.array([r[3] for r in rows])
        assert (e32 <= EXCLUDE_ABOVE).all(), (tag, k, float(e32.max()))
        bar = MARGIN * np.maximum(np.maximum(e32, np.median(e32)), FLOOR)
        worst = max(r[2] / b_ * MARGIN for r, b_ in zip(rows, bar))
        print("temporal-layers-stage %-14s layer %2d %-32s | %3d items | max e_32 %.1e | max e_hip %.1e | largest e_hip / max(e_32, median, 8 u) %.2f" % (
            tag, k, lcases[0].names[k][:32], len(rows), float(e32.max()), max(r[2] for r in rows), worst))
        for (layer, it, eh, e3), b_ in zip(rows, bar):
            assert eh <= b_, "%s item %s |S| = %d (%d in the frame): e_hip %.3e > bar %.3e (e_32 %.3e, median %.3e)" % (
                layer.name, it["pos"], it["n"], len(it["members"]), eh, b_, e3, float(np.median(e32)))
        judged += len(rows)
    return judged


@pytest.mark.parametrize("family,n", tl.STAGE)
def test_families_and_layer_counts_against_the_single_layer_call_and_float64(hipctx, family, n):
    lcases = tl.stage_cases(family, n)
    results = [run_layered(hipctx, lc_) for lc_ in lcases]
    for lcase, res in zip(lcases, results):
        check_exact(hipctx, lcase, res)
    assert check_items("%s L=%d" % (family, n), lcases, results) >= 3 * n


def test_non_finite_family_poisons_item_by_item_and_layer_by_layer(hipctx):
    """the NaN and the inf covariance of the family sit in neighbour frames: the two full items that have such a member are NaN in the layers that carry the
    value (the frame, its scaled copy, its rotation) and finite in the independent layer; the fallback item with such a member is finite in every layer"""
    (lcase,) = tl.stage_cases("non-finite", 4)
    bad = [np.argwhere(~np.isfinite(pc)) for pc in lcase.case.pixcov]
    assert sum(len(b) for b in bad) == 3 and np.isinf(np.concatenate([pc[~np.isfinite(pc)] for pc in lcase.case.pixcov])).sum() == 1
    sums, cnt, redo, _ = run_layered(hipctx, lcase)
    for k in range(lcase.n):
        s64, c64, items, _ = references(lcase, k)
        ts.check_exact_parts(lcase.layer(k), sums[k], cnt, s64, c64)
        poisoned = [it for it in items if it["n"] >= tb.K1 and np.isnan(sums[k][br.touched(it, 1)]).all()]
        assert len(poisoned) == (0 if k == 2 else 2), (k, [it["pos"] for it in poisoned])
        assert np.isnan(sums[k]).sum() == sum(np.isnan(sums[k][br.touched(it, 1)]).sum() for it in poisoned), k
        for it in items:
            if it["n"] < tb.K1:
                assert np.isfinite(sums[k][br.touched(it, 1)]).all(), (k, it["pos"])


@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("items", [1, 6, 7, 8])
def test_weak_lists_either_side_of_a_wavefront(hipctx, items, F):
    lcase = tl.weak_list_case(items, F, 400 + 10 * F + items)
    res = run_layered(hipctx, lcase)
    check_exact(hipctx, lcase, res)
    assert int(res[1].sum()) == 9 * items and res[2] == [0, 0, 0]


def test_27_and_28_members_over_three_frames_and_an_empty_set(hipctx):
    lcase = tl.limit_case()
    res = run_layered(hipctx, lcase)
    check_exact(hipctx, lcase, res)
    assert check_items("27 / 28 / 0", [lcase], [res]) >= 3 * lcase.n
    (l, c), = [p for p in zip(*np.nonzero(lcase.case.state == 1)) if lcase.case.nsim_total[p] == 0]
    for k in range(lcase.n):
        assert np.isnan(res[0][k][l - 1:l + 2, c - 1:c + 2]).all(), k                     # |S| = 0: NaN in every layer
        assert np.isnan(res[0][k]).sum() == 27
    assert (res[1][l - 1:l + 2, c - 1:c + 2] == 1).all()


def test_a_non_finite_covariance_poisons_its_own_layer_only(hipctx):
    lcase = tl.poisoned_case()
    res = run_layered(hipctx, lcase)
    check_exact(hipctx, lcase, res)
    _, _, items, _ = references(lcase, lcase.poisoned_layer)
    (item,) = [it for it in items if it["pos"] == tuple(lcase.poisoned_item)]
    at = br.touched(item, 1)
    for k in range(lcase.n):
        if k == lcase.poisoned_layer:
            assert np.isnan(res[0][k][at]).all() and np.isnan(res[0][k]).sum() == np.isnan(res[0][k][at]).sum()
        else:
            assert np.isfinite(res[0][k]).all(), k
    assert check_items("poisoned", [lcase], [res]) > 0


def test_layers_built_for_the_redo_list_take_it_whatever_their_neighbours_do(hipctx):
    lcase = tl.redo_case()
    res = run_layered(hipctx, lcase)
    check_exact(hipctx, lcase, res)                                   # (h_redo[k] is the single-layer call's count, layer by layer)
    redo = res[2]
    print("temporal-layers-stage redo per layer %s" % redo)
    for k in range(lcase.n):
        assert (redo[k] > 0) == (k in lcase.redo_layers), redo
    assert check_items("redo", [lcase], [res]) > 0


def dense_check(lcase, res):
    sums, cnt, _, _ = res
    for k in range(lcase.n):
        s64, c64, _, s32 = references(lcase, k)
        ts.check_exact_parts(lcase.layer(k), sums[k], cnt, s64, c64)
        e_hip, e_32 = br.rel_local(sums[k], s64), br.rel_local(s32, s64)
        print("temporal-layers-stage %-24s layer %d dense: e_32 %.2e e_hip %.2e" % (lcase.case.name, k, e_32, e_hip))
        assert e_hip <= MARGIN * max(e_32, FLOOR), (lcase.name, k, e_hip, e_32)


def test_dense_frame_against_float64(hipctx):
    lcase = tl.dense_case()
    res = run_layered(hipctx, lcase)
    dense_check(lcase, res)
    for k in range(lcase.n):                                          # ... and the single-layer call: the same count image, the same redo count
        s1, c1, r1 = run_single(hipctx, lcase.layer(k))
        assert np.array_equal(res[1], c1) and res[2][k] == r1
        assert br.rel_local(res[0][k], s1.astype(np.float64)) <= 1e-5


def test_two_layered_calls_then_a_plain_estimate_equal_to_a_fresh_context_s():
    import bcd_amd.hip as bh
    seq = tl.call_sequence()
    plain = tb.single_frame_of(seq[0].case)
    col, pixcov, mask, nsim, state, w, b, min_eig = plain
    s64, c64, _ = br.accumulate(*plain, keep_stages=False)
    s32, _, _ = br.accumulate(*plain, dtype=np.float32, keep_stages=False)
    out = {}
    for which in ("after layered temporal calls", "fresh"):
        ctx = bh.Context(0)
        try:
            if which != "fresh":
                res = run_layered(ctx, seq[0])
                check_exact(ctx, seq[0], res)
                dense_check(seq[1], run_layered(ctx, seq[1]))
            s, c = ctx.bayes_accumulate(_t(col), _t(pixcov), _t(mask.view(np.int32)), _t(nsim), _t(state), w, b, min_eig)
            ctx.synchronize()
            out[which] = (s.cpu().numpy(), c.cpu().numpy())
        finally:
            ctx.close()
    e_32 = br.rel_local(s32, s64)
    for which, (s, c) in out.items():
        assert np.array_equal(c, c64), which
        assert br.rel_local(s, s64) <= MARGIN * max(e_32, FLOOR), (which, br.rel_local(s, s64), e_32)
    a, f = out["after layered temporal calls"], out["fresh"]
    assert np.array_equal(a[1], f[1]) and br.rel_local(a[0], f[0].astype(np.float64)) <= MARGIN * max(e_32, FLOOR)


def test_refusals_leave_the_context_usable(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    lcase = tl.stage_cases("sizes F=1", 2)[0]
    case = lcase.case
    H, W = case.state.shape
    masks = [_t(m.view(np.int32)) for m in case.mask]
    frames = [([(_t(lcase.col[k][f]), _t(lcase.pixcov[k][f])) for k in range(2)], masks[f]) for f in range(2)]
    nsim, state = _t(case.nsim_total), _t(case.state)
    sums, cnt, check = guarded_out(H, W, 2)

    def refused(call, word=None):
        with pytest.raises(bh.BcdHipError) as e:
            call()
        assert word is None or word in str(e.value), str(e.value)

    for (w, b) in ((1, 12), (2, 6), (0, 6), (1, 3)):                 # any other geometry: BCD_HIP_EUNSUPPORTED, with a message
        words = ((2 * b + 1) ** 2 + 31) // 32
        other = [(ls, torch.zeros((H, W, words), dtype=torch.int32, device="cuda")) for (ls, _) in frames]
        refused(lambda: hipctx.bayes_accumulate_temporal_layers(other, nsim, state, w, b, case.min_eig, out=(sums, cnt)), "support")
    refused(lambda: hipctx.bayes_accumulate_temporal_layers(frames * 3, nsim, state, 1, 6, case.min_eig, out=(sums, cnt)))              # six frames
    seventeen = [(ls * 9, m) for (ls, m) in frames]
    refused(lambda: hipctx.bayes_accumulate_temporal_layers([(ls[:17], m) for ls, m in seventeen], nsim, state, 1, 6, case.min_eig))     # 17 layers
    refused(lambda: hipctx.bayes_accumulate_temporal_layers(frames, nsim, state, 1, 6, case.min_eig, out=([sums[0], sums[0]], cnt)))     # a shared sum image
    refused(lambda: hipctx.bayes_accumulate_temporal_layers(frames, nsim, state, 1, 6, case.min_eig, out=([sums[0], frames[1][0][1][0]], cnt)))  # a sum that is an input
    refused(lambda: hipctx.bayes_accumulate_temporal_layers(frames, nsim, state, 1, 6, case.min_eig, out=(sums, nsim)))                 # the count image is |S|
    L = bh.lib()
    cols = (C.c_void_p * 2)(frames[0][0][0][0].data_ptr(), None)
    pcs = (C.c_void_p * 2)(frames[0][0][0][1].data_ptr(), frames[0][0][1][1].data_ptr())
    one = (bh.StageFrameLayers * 1)()
    one[0].d_colors, one[0].d_pixel_cov, one[0].d_mask = cols, pcs, masks[0].data_ptr()
    sp = (C.c_void_p * 2)(sums[0].data_ptr(), sums[1].data_ptr())
    redo = (C.c_int32 * 2)()
    tail = (nsim.data_ptr(), state.data_ptr(), W, H, 1, 6, 1e-8, sp, cnt.data_ptr(), redo)
    assert L.bcd_hip_bayes_accumulate_temporal_layers(hipctx.h, one, 1, 2, *tail) == -1        # a null image in a layer of a frame
    assert L.bcd_hip_bayes_accumulate_temporal_layers(hipctx.h, one, 0, 2, *tail) == -1        # no frame
    assert L.bcd_hip_bayes_accumulate_temporal_layers(hipctx.h, one, 1, 0, *tail) == -1        # no layer
    assert L.bcd_hip_bayes_accumulate_temporal_layers(hipctx.h, None, 1, 1, *tail) == -1       # no frame list
    check()
    assert all(float(s.abs().sum()) == 0.0 for s in sums) and int(cnt.sum()) == 0              # refused before any device work
    res = run_layered(hipctx, lcase)
    check_exact(hipctx, lcase, res)
