"""GPU tests of the row-band estimate and of its speculative launch, per item, against float64.

bcd_hip_bayes_accumulate_rows is the estimate stage of the multi-GPU band driver (bcd_multi.hip): the processed pixels of lines [row_begin, row_end)
of a FULL state image, optionally behind a device word (`d_skip_if`) that the marking batch enqueued ahead of it leaves at zero when the estimate is
wanted.  bcd_hip_active_step_enqueue writes that word: the count of undecided pixels, + 2^40 when the last similarity pass has to be repeated.  The
test bed of the whole-frame twin (tests/bayes_cases.py, tests/bayes_ref.py, the helpers and the bar of tests/test_gpu_bayes_stage.py -- imported, the
same code: 4 max(e_32, family median of e_32, 8 u) per item, the 15 x 15 local figure on dense cases) is pointed at the band entry points, on the
bands of tests/bayes_rows_cases.py (held to their conditions by tests/test_bayes_rows_cases_cpu.py).

  a. one band against its own reference: the full state image with a seeded mix of IN / UNDECIDED / NONE outside the owned lines, into zeroed
     accumulators; count equal everywhere, non-finite pattern equal, fallback means within |S| u max|x|, full estimates within the bar, and every
     pixel the band's reference does not touch holds bit-zero sums (a halo item listed, a fallback tile that ignores the row range);
  b. the bands of a cut list one after the other into the same accumulators on a fresh context, against the frame's reference (records, hint and
     counters carried from band to band);
  c. the speculative call, both outcomes, deterministic: word 5 -> skipped, prefilled accumulators bit-identical, redo count 0; word 0 -> the band's
     reference; on the four `call sequence` calls (458, 458, 2 240 and 6 items in lines [7, 41)), then 2 240 and 458 again: from the skipped call that
     follows the first 2 240 on, the first chunk of estimate kernels is launched ahead for the previous length and must find an empty list when the
     list kernel skipped; one skipped call on another frame size in between;
  d. the word: equal to the UNDECIDED bytes of the owned lines and to what bcd_hip_active_step_collect returns, batch after batch until 0, final
     states equal to marking_ref; with_verdict: + 2^40 exactly when bcd_hip_similarity_masks_verdict says redo (one frame of each kind);
  e. the chain as the band driver runs it, on a stream of its own: init, enqueue with the word, the word copied to pinned host memory in stream
     order, the speculative estimate, collect; the halo lines are undecided in the first round (nothing exchanged yet: owned pixels wait for them, the
     round is skipped -- a 78-deep chain would not do at this size, a scanline batch of 16 launches resolves it) and decided afterwards;
  f. refusals before any device work, then a good call on the same context.

Measured on the MI355X: MEASURED below and docs/EXPERIMENTS.md section 6b."""
import ctypes as C

import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br
import bayes_rows_cases as rc
import marking_cases as mc
import marking_ref as mr
import test_gpu_bayes_stage as stage
import test_gpu_marking_stage as marking

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = stage.MARGIN, stage.FLOOR
FAMILIES = sorted({f for f, _ in rc.SELECTED})
SPEC_BAND = (7, 41)

# MEASURED on the MI355X (no kernel changed; the table per case in docs/EXPERIMENTS.md section 6b): 22 tests in 17 s -- the two count / pattern tests of
# "other kernels" 3.5 ... 3.8 s each (the CPU references of "w=2 b=6 dense"), the speculative sequence 2.0 s, "borders" 1.3 s and 0.9 s, the rest under 0.6 s each.
# The word: first words of the 16 band problems 0 ... 208 (13 not 0); with the verdict 79 then 0 on the ordinary frame, 2^40 + 457 then 2^40 on the other.
# Largest e_hip / bar (the bar with its factor 4), one band | bands summed:
#   sizes 0.21 | 0.21   sizes dense 0.13 | 0.11   borders line 0, 1, 3: 0.16, 0.18, 0.18 | the same   borders dense 0.12 | 0.10
#   non-finite nan colour, inf colour, nan pixcov: 0.19, 0.18, 0.14 | the same   w=1 b=12 0.24 | 0.24   w=1 b=3 0.14 | 0.14   w=0 b=4 0.21 | 0.21
#   w=2 b=6 sizes 0.94 | 0.94 (the 3.77 / 4 of the whole-frame table: the same item of k_bayes_strong_generic)   w=2 b=6 dense 0.32 | 0.28   w=1 b=4 dense 0.13 | 0.15
#   speculative calls 0.11 ... 0.14   chain 0.09 (rounds skipped / run: scanline 1 / 1, random order 3 / 1)
# Four builds with one line changed (docs/EXPERIMENTS.md section 6b) turn 19, 19, 1 and 2 of the 22 tests red.


def T(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


_dev = {}


def dev(case):
    """(colours, per-pixel covariances, masks, |S|) of a case on the device, once per frame (banded copies and call-sequence calls share them)"""
    key = (id(case.col), id(case.mask))
    if key not in _dev:
        _dev[key] = (case, T(case.col), T(case.pixcov), T(case.mask), T(case.nsim))
    return _dev[key][1:]


def run_rows(ctx, case, state, rb, re, out=None, skip_word=None):
    """-> (sum, count, skipped) as NumPy arrays / int; `state` is the state image handed to the call"""
    col, pixcov, mask, nsim = dev(case)
    st = T(state)
    ctx.synchronize()
    s, c, skipped = ctx.bayes_accumulate_rows(col, pixcov, mask, nsim, st, case.w, case.b, case.min_eig, rb, re, out=out, skip_word=skip_word)
    ctx.synchronize()
    return s, c, skipped


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_untouched(name, s_hip, c_hip, c64):
    """a pixel no item of the band touches: zero count and bit-zero sums"""
    z = c64 == 0
    assert not c_hip[z].any() and not bits(s_hip)[z].any(), (name, "written outside the band's items", np.argwhere(z & (bits(s_hip).any(axis=2) | (c_hip != 0)))[:5])


def worst_ratios(rows, dense):
    """{case name: largest e_hip / bar} of family_figures' rows"""
    out = {}
    base = lambda case: case.name.split(" lines [")[0]                    # (the bands of a case together)
    for case, it, eh, e3, b_ in rows:
        if b_ is not None:
            out[base(case)] = max(out.get(base(case), 0.0), eh / b_)
    for case, eh, e3 in dense:
        out[base(case)] = max(out.get(base(case), 0.0), eh / (MARGIN * max(e3, FLOOR)))
    return out


def selected(family):
    return [rc.case(n) for f, n in rc.SELECTED if f == family]


# ---- a. one band against its own reference ------------------------------------------------------------------------------------------------------
_single = {}


def single_band_results(hipctx, family):
    """(banded cases, results) of every band of every selected case of the family, each into zeroed accumulators; once per session"""
    if family not in _single:
        cases, results = [], []
        for c in selected(family):
            for (r0, r1) in rc.bands(c.name):
                rb, re = rc.call_range(c, r0, r1)
                s, n, _ = run_rows(hipctx, c, rc.poisoned_state(c, r0, r1), rb, re)
                cases.append(rc.banded(c, r0, r1))
                results.append((s.cpu().numpy(), n.cpu().numpy(), None))
        _single[family] = (cases, results)
    return _single[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_one_band_counts_patterns_fallback_means_and_untouched_pixels(hipctx, family):
    cases, results = single_band_results(hipctx, family)
    assert len(cases) >= 4
    stage.judge_exact(family, cases, results)
    for case, (s_hip, c_hip, _) in zip(cases, results):
        s64, c64, items, s32 = stage.references(case)
        check_untouched(case.name, s_hip, c_hip, c64)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_band_per_item_against_float64(hipctx, family):
    cases, results = single_band_results(hipctx, family)
    fig, rows, dense = stage.family_figures(family, cases, results)
    for name, r in sorted(worst_ratios(rows, dense).items()):
        stage._report("bayes-rows one band      %-48s e_hip / bar %.3f" % (name, r))
    stage.judge_numerical(family, cases, results)


# ---- b. the bands of a cut list add up to the frame ------------------------------------------------------------------------------------------------
_summed = {}


def summed_results(family):
    if family not in _summed:
        import torch
        import bcd_amd.hip as bh
        ctx = bh.Context(0)
        try:
            cases, results = selected(family), []
            for c in cases:
                H, W, _ = c.col.shape
                out = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"))
                for (r0, r1) in rc.bands(c.name):
                    rb, re = rc.call_range(c, r0, r1)
                    run_rows(ctx, c, rc.poisoned_state(c, r0, r1, seed=1), rb, re, out=out)
                results.append((out[0].cpu().numpy(), out[1].cpu().numpy(), None))
        finally:
            ctx.close()
        _summed[family] = (cases, results)
    return _summed[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_bands_add_up_to_the_frame_counts_patterns_and_fallback_means(family):
    cases, results = summed_results(family)
    stage.judge_exact(family, cases, results)
    for case, (s_hip, c_hip, _) in zip(cases, results):
        check_untouched(case.name, s_hip, c_hip, stage.references(case)[1])


@pytest.mark.parametrize("family", FAMILIES)
def test_bands_add_up_to_the_frame_per_item_against_float64(family):
    cases, results = summed_results(family)
    fig, rows, dense = stage.family_figures(family, cases, results)
    for name, r in sorted(worst_ratios(rows, dense).items()):
        stage._report("bayes-rows bands summed  %-48s e_hip / bar %.3f" % (name, r))
    stage.judge_numerical(family, cases, results)


# ---- c. the speculative call, both outcomes ------------------------------------------------------------------------------------------------------------
def prefill(rng, H, W):
    return rng.uniform(0.5, 2.0, (H, W, 3)).astype(np.float32), rng.integers(1, 9, (H, W)).astype(np.int32)


def skipped_call_leaves_everything(ctx, case, rb, re, word, host, rng):
    H, W, _ = case.col.shape
    pre_s, pre_c = prefill(rng, H, W)
    out = (T(pre_s), T(pre_c))
    word.fill_(5)
    host[0] = 5
    s, c, skipped = run_rows(ctx, case, case.state, rb, re, out=out, skip_word=(word, host))
    assert skipped == 1, case.name
    assert ctx.bayes_last_redo_count() == 0, case.name
    ctx.synchronize()
    assert np.array_equal(bits(s.cpu().numpy()), bits(pre_s)) and np.array_equal(c.cpu().numpy(), pre_c), (case.name, "a skipped call wrote to the accumulators")


def wanted_call_equals_the_band(ctx, case, r0, r1, word, host, what):
    word.zero_()
    host[0] = 0
    s, c, skipped = run_rows(ctx, case, case.state, r0, r1, skip_word=(word, host))
    assert skipped == 0, case.name
    band = rc.banded(case, r0, r1)
    s_hip, c_hip = s.cpu().numpy(), c.cpu().numpy()
    s64, c64, items, s32 = stage.references(band)
    stage.check_exact_parts(band, s_hip, c_hip, s64, c64)
    check_untouched(band.name, s_hip, c_hip, c64)
    e_hip, e_32 = br.rel_local(s_hip, s64), br.rel_local(s32, s64)
    stage._report("bayes-rows %-13s %-48s e_hip / bar %.3f" % (what, band.name, e_hip / (MARGIN * max(e_32, FLOOR))))
    assert e_hip <= MARGIN * max(e_32, FLOOR), (band.name, e_hip, e_32)      # (the bar of test_call_sequence_of_the_stateful_launch_logic)


def test_speculative_call_skipped_and_wanted_on_the_call_sequence():
    import torch
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        word, host = torch.zeros((1,), dtype=torch.int64, device="cuda"), np.zeros((1,), np.int64)
        rng = np.random.default_rng(5)
        r0, r1 = SPEC_BAND
        seq = bc.call_sequence()
        other = rc.case("sizes dense")                                   # another frame size: 34 x 40
        for i, case in enumerate(seq + [seq[2], seq[0]]):
            skipped_call_leaves_everything(ctx, case, r0, r1, word, host, rng)
            wanted_call_equals_the_band(ctx, case, r0, r1, word, host, "speculative")
            if i == 2:                                                   # between two wanted calls of the sequence
                skipped_call_leaves_everything(ctx, other, 5, 16, word, host, rng)
    finally:
        ctx.close()


# ---- d. the word ----------------------------------------------------------------------------------------------------------------------------------
def batches_until_decided(ctx, mask, cnt, state, w, b, rb, re, mode, seed, top, what, verdict=None):
    """marking batches with the word until it says 0 -> (state as NumPy, [(word, undecided, launches, redo)]); after every batch the word is the number
    of UNDECIDED bytes of the owned lines (+ 2^40 when `verdict` -- called after the synchronisation -- says the masks have to be recomputed)"""
    log, before = [], None
    limit = (re - rb) * state.shape[1] + 2
    while True:
        st, entry = one_batch(ctx, mask, cnt, state, w, b, rb, re, mode, seed, top, what, verdict)
        log.append(entry)
        left = entry[1]
        assert before is None or left < before, what + (log,)
        if left == 0:
            return st, log
        assert len(log) < limit, what
        before = left


def one_batch(ctx, mask, cnt, state, w, b, rb, re, mode, seed, top, what, verdict=None):
    """-> (state as NumPy, (word, undecided, launches, redo)) of one marking batch with the word, held to the state image"""
    import torch
    word = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ctx.synchronize()
    ctx.active_step_enqueue(mask, cnt, state, w, b, rb, re, mode, seed, top, total=word, with_verdict=verdict is not None)
    ctx.synchronize()
    st = state.cpu().numpy()
    left = int((st[rb:re] == mr.ST_UNDECIDED).sum())
    undecided, launches = ctx.active_step_collect()
    redo = verdict() if verdict is not None else 0
    got = int(word.cpu().numpy()[0])
    entry = (got, undecided, launches, redo)
    assert undecided == left and launches >= 1, what + (entry, left)
    assert got == left + ((1 << 40) if redo else 0), what + (entry, left)
    return st, entry


def test_word_counts_the_undecided_pixels_of_the_owned_lines(hipctx):
    import torch
    case = mc.by_name("random 0.30 b=6 15x40 w=1")
    W, H, w, b = case.W, case.H, case.w, case.b
    batches, waited = 0, []
    for (mode, seed) in ((0, 0), (1, 11)):
        for m in (1.0, 0.5):
            want = mc.reference(case, mode, seed, m)
            for (r0, r1) in marking.bands_of(H):
                top, bot = max(0, r0 - b), min(H, r1 + b)
                rb, re = r0 - top, r1 - top
                what = (case.name, "order %d seed %d m %g" % (mode, seed, m), "lines [%d, %d) of band [%d, %d)" % (r0, r1, top, bot))
                mask, cnt = T(case.mask[top:bot]), T(case.cnt[top:bot])
                halo = want[top:bot].copy()
                halo[rb:re] = mr.ST_NONE
                hipctx.synchronize()
                state = hipctx.active_init(cnt, w, rb, re, m, seed, top)

                def put_halo(h):
                    hd = torch.from_numpy(h).cuda()
                    state[:rb] = hd[:rb]
                    state[re:] = hd[re:]
                # the halo lines undecided first (nothing exchanged yet): where an owned pixel waits for one of them, the word is not 0
                put_halo(np.where(halo == mr.ST_NONE, mr.ST_NONE, mr.ST_UNDECIDED).astype(np.uint8))
                st, first = one_batch(hipctx, mask, cnt, state, w, b, rb, re, mode, seed, top, what)
                decided = st[rb:re] != mr.ST_UNDECIDED
                assert np.array_equal(st[rb:re][decided], want[r0:r1][decided]), what + ("decided against an undecided halo",)
                # (m = 1 only: with m < 1 a pixel the draw spares is processed whatever its neighbours do, and the criterion does not look at the draw)
                if m == 1.0 and marking.waits_for_the_halo(case, want, mc.visit(case, mode, seed), top, r0, r1, bot):
                    assert first[0] > 0, what + (first,)
                waited.append(first[0])
                put_halo(halo)
                if first[0] != 0:
                    st, log = batches_until_decided(hipctx, mask, cnt, state, w, b, rb, re, mode, seed, top, what)
                    batches += len(log)
                hipctx.synchronize()
                st = state.cpu().numpy()
                assert np.array_equal(st[rb:re], want[r0:r1]), what
                assert np.array_equal(st[:rb], halo[:rb]) and np.array_equal(st[re:], halo[re:]), what + ("halo lines were written",)
    assert sum(1 for x in waited if x > 0) >= 7, waited                  # the word was seen with a count in it, not only as 0 (7 of the 8 problems with m = 1 wait)
    stage._report("bayes-rows the word: first words against an undecided halo %s, then %d batches" % (waited, batches))


def test_word_carries_the_verdict_of_the_deferred_similarity_pass(hipctx):
    import oracle_lib as ol
    import bcd_amd.core as core
    import bcd_amd.hip as bh
    import torch
    L = bh.lib()
    _, ns_a, hist_a, _, _ = ol.synth_inputs(40, 30, 16, 21, 0.3, 0.0)              # an ordinary frame
    W, H = 128, 160                                                              # one pixel outside the range the production distance kernels guard
    _, ns_b, hist_b, _ = core.synthetic_scene(W, H, 16, 4, 0.2, 0.0)
    hist_b, ns_b = hist_b.copy(), ns_b.copy()
    hist_b[H - 20, 33, :] *= 4.0e6
    ns_b[H - 20, 33] *= 4.0e6
    b, seen = 6, []

    def verdict():
        r = C.c_int(-1)
        assert L.bcd_hip_similarity_masks_verdict(hipctx.h, C.byref(r)) == 0 and r.value in (0, 1)
        return r.value

    for name, hist, ns in (("ordinary", hist_a, ns_a), ("outside the guarded range", hist_b, ns_b)):
        H, W, D = hist.shape
        d_hist, d_ns = T(hist), T(ns)
        mask = torch.zeros((H, W, ((2 * b + 1) ** 2 + 31) // 32), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        hipctx.synchronize()
        assert L.bcd_hip_similarity_masks_deferred(hipctx.h, d_hist.data_ptr(), d_ns.data_ptr(), W, H, D, 1, b, 1.0, mask.data_ptr(), cnt.data_ptr()) == 0
        # lines [8, H - 8) with the b halo lines on either side still undecided: owned pixels wait for them, the first word carries a count that is not 0
        rb, re = 8, H - 8
        state = hipctx.active_init(cnt, 1, rb, re, 1.0, 3, 0)
        state[rb - b:rb, 1:W - 1] = mr.ST_UNDECIDED
        state[re:re + b, 1:W - 1] = mr.ST_UNDECIDED
        _, first = one_batch(hipctx, mask, cnt, state, 1, b, rb, re, 1, 3, 0, (name,), verdict)
        assert first[1] > 0, (name, first)
        state[rb - b:rb, 1:W - 1] = mr.ST_OUT                            # the halo decided (nobody there marks anybody)
        state[re:re + b, 1:W - 1] = mr.ST_OUT
        st, log = batches_until_decided(hipctx, mask, cnt, state, 1, b, rb, re, 1, 3, 0, (name,), verdict)
        assert not (st[rb:re] == mr.ST_UNDECIDED).any() and (st[rb:re, 1:W - 1] != mr.ST_NONE).all()
        assert len({r for (_, _, _, r) in [first] + log}) == 1           # (the verdict is the pass's: the same after every batch)
        seen.append(first[3])
        stage._report("bayes-rows the word with the verdict, %s frame: %s" % (name, [first] + log))
    assert seen == [0, 1], seen                                          # both sides of the test the word repeats on the device


# ---- e. the chain as the band driver runs it --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [(0, 0), (1, 11)], ids=["scanline", "random"])
def test_chain_marking_batch_word_speculative_estimate(order):
    import torch
    import bcd_amd.hip as bh
    mode, seed = order
    c, g = rc.chain_problem()
    H, W, _ = c.col.shape
    w, b = c.w, c.b
    r0, r1 = rc.CHAIN_BAND
    want = mc.reference(g, mode, seed, 1.0)
    halo_rows = np.zeros((H, W), bool)
    halo_rows[r0 - b:r0] = halo_rows[r1:r1 + b] = True
    halo_rows &= mr.main_area(W, H, w)
    halo_undecided = np.where(halo_rows, mr.ST_UNDECIDED, mr.ST_NONE).astype(np.uint8)
    halo_decided = np.where(halo_rows, want, mr.ST_NONE).astype(np.uint8)
    stream = torch.cuda.Stream()
    ctx = bh.Context(0, stream=stream)
    try:
        with torch.cuda.stream(stream):
            col, pixcov, mask, nsim = T(c.col), T(c.pixcov), T(c.mask), T(c.nsim)
            state = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            S = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            N = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            word = torch.zeros((1,), dtype=torch.int64, device="cuda")
            host = torch.zeros((1,), dtype=torch.int64).pin_memory()
            host_np = host.numpy()

            def put_halo(h):
                hd = T(h)
                state[:r0] = hd[:r0]
                state[r1:] = hd[r1:]

            ctx.active_init(nsim, w, r0, r1, 1.0, seed, 0, state)
            put_halo(halo_undecided)                                     # nothing exchanged yet
            outcomes = []
            while True:
                ctx.active_step_enqueue(mask, nsim, state, w, b, r0, r1, mode, seed, 0, total=word)
                host.copy_(word, non_blocking=True)                      # in stream order, behind the batch
                _, _, skipped = ctx.bayes_accumulate_rows(col, pixcov, mask, nsim, state, w, b, c.min_eig, r0, r1, out=(S, N), skip_word=(word, host_np))
                stream.synchronize()
                undecided, _ = ctx.active_step_collect()
                left = int((state[r0:r1] == mr.ST_UNDECIDED).sum().item())
                assert int(host_np[0]) == undecided == left and skipped == (1 if left else 0), (outcomes, int(host_np[0]), undecided, left, skipped)
                outcomes.append(skipped)
                if not skipped:
                    break
                assert not bits(S.cpu().numpy()).any() and not N.cpu().numpy().any(), "a skipped round wrote to the accumulators"
                assert len(outcomes) < 200
                if len(outcomes) == 1:
                    put_halo(halo_decided)                               # the exchange of the boundary states
            stream.synchronize()
            st, s_hip, c_hip = state.cpu().numpy(), S.cpu().numpy(), N.cpu().numpy()
    finally:
        ctx.close()
    assert outcomes[0] == 1 and outcomes[-1] == 0, outcomes                # both outcomes occurred
    assert np.array_equal(st[r0:r1], want[r0:r1])
    band = rc.banded(rc.with_state(c, np.where(want == mr.ST_IN, 1, 0), "chain order %d" % mode), r0, r1)
    s64, c64, items, s32 = stage.references(band)
    stage.check_exact_parts(band, s_hip, c_hip, s64, c64)
    check_untouched(band.name, s_hip, c_hip, c64)
    e_hip, e_32 = br.rel_local(s_hip, s64), br.rel_local(s32, s64)
    stage._report("bayes-rows chain         %-48s rounds %s e_hip / bar %.3f" % (band.name, outcomes, e_hip / (MARGIN * max(e_32, FLOOR))))
    assert e_hip <= MARGIN * max(e_32, FLOOR), (band.name, e_hip, e_32)


# ---- f. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_any_device_work_then_a_good_call(hipctx):
    import torch
    import bcd_amd.hip as bh
    L = bh.lib()
    rng = np.random.default_rng(6)
    c = rc.case("sizes dense")
    H, W, _ = c.col.shape
    col, pixcov, mask, nsim = dev(c)
    state = T(c.state)
    pre_s, pre_c = prefill(rng, H, W)
    s, n = T(pre_s), T(pre_c)
    word, host = torch.zeros((1,), dtype=torch.int64, device="cuda"), np.zeros((1,), np.int64)
    hipctx.synchronize()
    skipped = C.c_int(-5)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(images=None, w=c.w, rb=5, re=16, d_word=None, h_word=None, sk=None):
        a = [p(x) for x in (col, pixcov, mask, nsim, state)] + [p(s), p(n)]
        for k in (images or ()):
            a[k] = None
        rc_ = L.bcd_hip_bayes_accumulate_rows(hipctx.h, a[0], a[1], a[2], a[3], a[4], W, H, w, c.b, c.min_eig, a[5], a[6], rb, re, d_word, h_word, sk)
        return rc_, L.bcd_hip_last_error(hipctx.h).decode()

    h_ptr = C.c_void_p(host.ctypes.data)
    for k in range(7):                                                   # null images
        rc_, msg = call(images=(k,))
        assert rc_ != 0 and "bad argument" in msg, (k, rc_, msg)
    for kw in (dict(d_word=p(word), h_word=None, sk=C.byref(skipped)), dict(d_word=p(word), h_word=h_ptr, sk=None)):
        rc_, msg = call(**kw)
        assert rc_ != 0 and "speculative" in msg, (kw, rc_, msg)
    c2 = rc.case("w=2 b=6 sizes")                                        # a skip word beside 5 x 5 patches
    H2, W2, _ = c2.col.shape
    pre_s2, pre_c2 = prefill(rng, H2, W2)
    out2 = (T(pre_s2), T(pre_c2))
    hipctx.synchronize()
    with pytest.raises(bh.BcdHipError, match="speculative"):
        hipctx.bayes_accumulate_rows(*dev(c2), T(c2.state), c2.w, c2.b, c2.min_eig, 0, H2, out=out2, skip_word=(word, host))
    with pytest.raises(ValueError):
        hipctx.bayes_accumulate_rows(col, pixcov, mask, nsim, state, c.w, c.b, c.min_eig, 0, H, skip_word=(word, host.astype(np.int32)))
    for (rb, re) in ((20, 20), (30, 10), (H + 2, H + 9), (-9, -2), (-4, 0)):   # row_begin >= row_end once clamped: nothing to do, and that is not an error
        rc_, msg = call(rb=rb, re=re)
        assert rc_ == 0, (rb, re, rc_, msg)
    hipctx.synchronize()
    assert skipped.value == -5
    assert np.array_equal(bits(s.cpu().numpy()), bits(pre_s)) and np.array_equal(n.cpu().numpy(), pre_c)
    assert np.array_equal(bits(out2[0].cpu().numpy()), bits(pre_s2)) and np.array_equal(out2[1].cpu().numpy(), pre_c2)
    # ... and the context still works
    s_hip, c_hip, _ = run_rows(hipctx, c, c.state, 5, 16)
    band = rc.banded(c, 5, 16)
    s_hip, c_hip = s_hip.cpu().numpy(), c_hip.cpu().numpy()
    s64, c64, items, s32 = stage.references(band)
    stage.check_exact_parts(band, s_hip, c_hip, s64, c64)
    assert br.rel_local(s_hip, s64) <= MARGIN * max(br.rel_local(s32, s64), FLOOR)
