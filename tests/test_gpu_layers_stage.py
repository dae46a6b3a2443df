"""GPU tests of the layered estimate path per stage, per item and at up to 16 layers.

bcd_hip_bayes_accumulate_layers hands constructed similar sets (tests/bayes_cases.py) with a list of layers (tests/layer_cases.py) to the code a frame of
bcd_hip_denoise_layers runs per scale: bayes() on layer 0, then layers_follow() -- k_bayes_weak_tile_layers<G> for the fallback pixels of all further
layers, the full-estimate chain per layer, per-layer redo lists.  Every layer is a Case of its own: float64 reference and float32 calibrator come from
tests/bayes_ref.py unchanged, the bars are those of tests/test_gpu_bayes_stage.py (MARGIN, FLOOR, EXCLUDE_ABOVE; nothing in a bar comes from a GPU run).

What is asserted, per family of bayes_cases.FAMILIES (4 layers; 6 / 7 with the special layers of "non-finite" / "floor boundary"), under the production
rule and under bcd_hip_set_strict_eigensolver(True), and per geometry (w, b) x layer count of GEOMETRIES:
  * the count image equals the reference's integers: the further layers add nothing to it;
  * every layer's non-finite pattern equals its float64 pattern (the `judged` rule of the single-layer test);
  * isolated cases: every layer's sum image is BIT FOR BIT the sum image of bcd_hip_bayes_accumulate on that layer alone, at every position of the list
    (so a non-finite layer changes no bit of another layer: that layer's bits are those of a call that never saw the non-finite one);
  * dense cases: <= 1e-5 from the single-layer call (float atomics arrive in another order), a pixel's error relative to the largest value of its
    15 x 15 neighbourhood, and the neighbourhood-relative bar against float64;
  * fallback items: |sum - mean_64| <= |S| u max|x| per entry, per layer;
  * full estimates: e_hip <= 4 max(e_32, median e_32 of that (family, layer), 8 u), per layer; "spike + cov" is the same strict expected failure, for
    the same cause (KNOWN_MISSES of the single-layer test: layer 0 IS the single-layer chain);
  * the redo count of every layer equals bcd_hip_bayes_last_redo_count after the single-layer call on that layer; their sum is the call's total.
Group sizes of k_bayes_weak_tile_layers<G>: G = min(4, further layers, what fits 64 KiB): b = 6 -> <4> (and <1>, <2>, <3> with 2, 3, 4 layers), b = 8
-> <3>, b = 12 -> <2>; BCD_HIP_WEAK_LAYERS_GROUP = 1, 2, 3 in child processes (ragged last groups 3 + 1 and 2 + 1).
The five layer-batched streaming kernels are checked bit for bit by tools/fuzz_layers_streaming.py (layered == single-image call == oracle).

Measured on the MI355X: docs/EXPERIMENTS.md section 11."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bayes_cases as bc
import bayes_ref as br
import layer_cases as lc
import test_gpu_bayes_stage as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_layers_streaming as fls  # noqa: E402

pytestmark = pytest.mark.gpu

U, MARGIN, FLOOR, EXCLUDE_ABOVE = st.U, st.MARGIN, st.FLOOR, st.EXCLUDE_ABOVE
TOL_SAME = 1e-5          # dense cases against the single-layer stage call: the documented bound for float-atomic arrival order

_report = st._report


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    nan = np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32))
    return (a == b) | nan


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_layered(hipctx, case, layers):
    """-> ([sum per layer], count, [redo per layer], the call's total)"""
    sums, c, redo = hipctx.bayes_accumulate_layers([(_t(l.col), _t(l.pixcov)) for l in layers], _t(case.mask.view(np.int32)), _t(case.nsim), _t(case.state),
                                                   case.w, case.b, case.min_eig)
    total = hipctx.bayes_last_redo_count()
    hipctx.synchronize()
    return [s.cpu().numpy() for s in sums], c.cpu().numpy(), redo, total


_single = {}


def run_single(hipctx, layer, strict):
    """bcd_hip_bayes_accumulate on one layer alone, once per session and stopping rule: (sum, count, redo)"""
    key = (id(layer), strict)
    if key not in _single:
        s, c = hipctx.bayes_accumulate(_t(layer.col), _t(layer.pixcov), _t(layer.mask.view(np.int32)), _t(layer.nsim), _t(layer.state), layer.w, layer.b, layer.min_eig)
        redo = hipctx.bayes_last_redo_count()
        hipctx.synchronize()
        _single[key] = (layer, s.cpu().numpy(), c.cpu().numpy(), redo)
    return _single[key][1:]


def references(layer):
    """the session's references of a layer, also where the helpers of the single-layer test look for them"""
    r = lc.references(layer)
    st._refs.setdefault(id(layer), (layer,) + tuple(r))
    return r


def run_both_rules(hipctx, pairs):
    """[(case, layers)] -> {strict: [(layered result, [single results])]}"""
    import bcd_amd.hip as bh
    out = {}
    for strict in (False, True):
        try:
            bh.set_strict_eigensolver(strict)
            out[strict] = [(run_layered(hipctx, case, ls), [run_single(hipctx, l, strict) for l in ls]) for case, ls in pairs]
        finally:
            bh.set_strict_eigensolver(False)
    return out


def check_exact(tag, case, layers, layered, singles, dense_ref_layers=None):
    """everything that needs no numerical bar against float64: counts, patterns, bit equality / atomic-order bound against the single-layer calls,
    fallback means, redo counts"""
    sums, cnt, redo, total = layered
    assert len(sums) == len(layers) == len(redo)
    for k, layer in enumerate(layers):
        s1, c1, r1 = singles[k]
        assert np.array_equal(cnt, c1), (tag, layer.name, "count image differs from the single-layer call's", np.argwhere(cnt != c1)[:5])
        assert redo[k] == r1, (tag, layer.name, "redo count: layered %d, single-layer call %d" % (redo[k], r1), redo)
        if not case.dense:
            eq = bits_equal(sums[k], s1)
            assert eq.all(), "%s %s (position %d of %d): %d values differ from bcd_hip_bayes_accumulate on that layer alone, first at %s: %r / %r" % (
                tag, layer.name, k, len(layers), int((~eq).sum()), np.argwhere(~eq)[0], sums[k][tuple(np.argwhere(~eq)[0])], s1[tuple(np.argwhere(~eq)[0])])
        else:
            assert np.array_equal(np.isfinite(sums[k]), np.isfinite(s1)), (tag, layer.name, "non-finite pattern differs from the single-layer call's")
            e = br.rel_local(sums[k], s1)
            _report("layers-stage %-28s %-60s vs single-layer call %.2e" % (tag, layer.name, e))
            assert e <= TOL_SAME, (tag, layer.name, e)
        if case.dense and dense_ref_layers is not None and k not in dense_ref_layers:
            continue
        s64, c64, items, s32 = references(layer)
        st.check_exact_parts(layer, sums[k], cnt, s64, c64)
        if not case.dense:
            st.check_fallback_items(layer, sums[k], s64, items)
    assert total == sum(redo), (tag, case.name, total, redo)


def figures(tag, pairs, results, dense_ref_layers=None):
    """per layer position: the figures of st.family_figures with that layer's own e_32 and the median over the (family, layer)'s items; every item
    beyond half its bar is reported.  -> [(position, figures, cases, results)]; asserts nothing but the exclusion cap"""
    out = []
    n = min(len(ls) for _, ls in pairs)
    for k in range(n):
        cases_k, results_k = [], []
        for (case, ls), (layered, _) in zip(pairs, results):
            if case.dense and dense_ref_layers is not None and k not in dense_ref_layers:
                continue
            references(ls[k])
            cases_k.append(ls[k])
            results_k.append((layered[0][k], layered[1], layered[2][k]))
        fig, rows, dense = st.family_figures("%s layer %d" % (tag, k), cases_k, results_k)
        for case, it, eh, e3, b_ in rows:
            if b_ is not None and eh > 0.5 * b_:
                _report("layers-stage item  %s | %s item %s |S| = %d | e_hip %.3e e_32 %.3e bar %.3e ratio %.2f" % (tag, case.name, it["pos"], it["n"], eh, e3, b_, MARGIN * eh / b_))
        out.append((k, fig, cases_k, results_k))
    return out


def judge(tag, figs):
    """the per-item bar per layer position (dense cases: neighbourhood-relative), after everything has been reported"""
    for k, fig, cases_k, results_k in figs:
        st.judge_numerical("%s layer %d" % (tag, k), cases_k, results_k)
    return [(k, fig) for k, fig, _, _ in figs]


# ---- every family, 4 layers ---------------------------------------------------------------------------------------------------------------------
_fam = {}


def family_results(hipctx, family):
    if family not in _fam:
        pairs = lc.family_layers(family)
        _fam[family] = (pairs, run_both_rules(hipctx, pairs))
    return _fam[family]


@pytest.mark.parametrize("family", sorted(bc.FAMILIES))
def test_layered_estimate_counts_patterns_bit_equality_fallback_means_and_redo_counts(hipctx, family):
    pairs, res = family_results(hipctx, family)
    for strict in (False, True):
        for (case, ls), (layered, singles) in zip(pairs, res[strict]):
            check_exact("%s%s" % (family, " strict" if strict else ""), case, ls, layered, singles)
    if family == "floor boundary":
        # the layers that exist to take / not to take the redo list do: a layer's redo list is its own, whatever its neighbours in the list do
        for (case, ls), (layered, _) in zip(pairs, res[False]):
            if case.name == "floor k=0 e=1e-08":
                redo = layered[2]
                _report("layers-stage floor boundary %s redo per layer %s" % (case.name, redo))
                assert redo[0] == 0 and redo[1] == 0 and redo[4] > 0 and redo[5] == 0 and redo[6] > 0, redo


# A (family, layer position) that misses its bar although the layered path is not at fault stays in, as a strict expected failure of THAT bar with the
# measured figures (docs/EXPERIMENTS.md section 11); every other layer of the family is judged by the test below, and its counts, patterns, bit equality
# with the single-layer call, fallback means and redo counts by the test above.
LAYER_MISSES = {
    ("spike", 3): "the channel rotation of \"spike x1000\", item (37, 97), |S| = 40, cond(C1) 2.2e6: under the STRICT rule e_hip 2.98e-5 against a bar of 2.15e-5 (e_32 5.4e-6): "
                  "5.5 x max(e_32, median, 8 u), bar 4; under the production rule 1.19e-5, 2.2 x.  The same item unrotated (layer 0): 1.76e-5 / 1.71e-5, 3.6 x / 3.5 x.  The "
                  "sums are bit for bit those of bcd_hip_bayes_accumulate on the rotated layer alone and the same from run to run, so the layered path adds nothing: it is the "
                  "estimate chain on this input.  Cause: with cond 1e4 ... 3e6 the family amplifies the eigensolver's rounding (18 ... 26 u per eigenvalue against LAPACK's "
                  "3 ... 7 u, docs/EXPERIMENTS.md section 6) -- item by item e_hip is 0.9 ... 7.6 x e_32 under either rule, higher under one rule as often as under the other, and "
                  "the single-layer family already stands at 3.55 / 3.46 of the 4 it may use.  The rotation permutes rows and columns of every matrix, the solver "
                  "rounds along another path, and one of 80 items lands beyond the bar.  A tighter solver, not the layered path, would move it; not part of this change.",
}


@pytest.mark.parametrize("family,k", [pytest.param(f, k, marks=pytest.mark.xfail(strict=True, reason=r)) for (f, k), r in sorted(LAYER_MISSES.items())])
def test_known_layer_misses_per_item_against_float64(hipctx, family, k):
    pairs, res = family_results(hipctx, family)
    for strict in (False, True):
        judge(family, [f for f in figures(family + (" strict" if strict else ""), pairs, res[strict]) if f[0] == k])


@pytest.mark.parametrize("family", [pytest.param(f, marks=pytest.mark.xfail(strict=True, reason=st.KNOWN_MISSES[f])) if f in st.KNOWN_MISSES else f
                                    for f in sorted(bc.FAMILIES)])
def test_layered_estimate_per_item_against_float64(hipctx, family):
    pairs, res = family_results(hipctx, family)
    lines, both = {}, []
    for strict in (False, True):
        both.append(figures(family + (" strict" if strict else ""), pairs, res[strict]))
        for k, fig, _, _ in both[-1]:
            lines.setdefault(k, []).append(fig)
    for k, (fp, fs) in sorted(lines.items()):
        _report("layers-stage %-14s | layer %d %-40s | %d | %d | %.1e | %.1e | %.2f | %.1e | %.2f | dense %.2f / %.2f" % (
            family, k, pairs[0][1][k].name.split(" / ")[-1], fp["items"], fp["excluded"], fp["max_e32"], fp["max_ehip"], fp["max_ratio"], fs["max_ehip"], fs["max_ratio"],
            fp["dense"], fs["dense"]))
    for strict in (False, True):
        judge(family + (" strict" if strict else ""), [f for f in both[strict] if (family, f[0]) not in LAYER_MISSES])


def test_spike_cov_family_per_layer_figures_and_its_independent_layer(hipctx):
    """the figures of "spike + cov" per layer (its bar is an expected failure above): reported for docs/EXPERIMENTS.md section 11; and the independent
    layer of that family, which has no spike, is held to the bar here -- the miss is layer 0's content, not the layered path"""
    pairs, res = family_results(hipctx, "spike + cov")
    for strict in (False, True):
        for k in range(4):
            cases_k = [ls[k] for _, ls in pairs]
            for l in cases_k:
                references(l)
            results_k = [(layered[0][k], layered[1], layered[2][k]) for layered, _ in res[strict]]
            fig = st.family_figures("spike + cov layer %d" % k, cases_k, results_k)[0]
            _report("layers-stage spike + cov    | layer %d %s | %s | max e_hip %.1e ratio %.2f" % (k, cases_k[0].name.split(" / ")[-1], "strict" if strict else "production",
                                                                                                  fig["max_ehip"], fig["max_ratio"]))
            if k == 2:
                st.judge_numerical("spike + cov layer 2", cases_k, results_k)


# ---- geometries and layer counts -------------------------------------------------------------------------------------------------------------------
# (w, b): the kernels the dispatcher selects, and the layer counts run there
GEOMETRIES = {
    (1, 6): (2, 5, 7, 16),      # k_bayes_weak_tile_layers<1> (2 layers), <4> (5: one full group; 7: 4 + 2; 16: 4 + 4 + 4 + 3), windowed chain, redo lists
    (1, 8): (4, 7),             # <3>: 3; 3 + 3.  gather chain
    (1, 12): (3, 16),           # <2>: 2; 7 x 2 + 1.  k_bayes27w<1, 12> chain
    (1, 3): (4,), (1, 4): (4,),  # gather kernels, <3>
    (2, 6): (4,), (2, 3): (4,),  # the list kernel per layer (k_bayes_weak), k_bayes_strong_generic
    (0, 4): (4,),               # generic
}
DENSE_REF_LAYERS = (0, 1, 2, 3, 8, 15)   # layers of a 16-layer dense case that get a float64 reference (all of them are held to the single-layer call)

_geom = {}


def geometry_pairs(w, b):
    if (w, b) not in _geom:
        n = max(GEOMETRIES[(w, b)])                                      # (a shorter list is the head of the longest one: references and single-layer calls are shared)
        _geom[(w, b)] = [(case, lc.layers(case, fam, n, 8000 + 10 * i)) for i, (case, fam) in enumerate(lc.geometry_cases(w, b))]
    return _geom[(w, b)]


@pytest.mark.parametrize("w,b,n", [(w, b, n) for (w, b), counts in sorted(GEOMETRIES.items()) for n in counts])
def test_geometries_and_layer_counts(hipctx, w, b, n):
    import bcd_amd.hip as bh
    pairs = [(case, ls[:n]) for case, ls in geometry_pairs(w, b)]
    tag = "w=%d b=%d L=%d" % (w, b, n)
    try:
        res = run_both_rules(hipctx, pairs)
    except bh.BcdHipError as e:                                          # a geometry check_params refuses: the refusal is the result
        assert "rc=-4" in str(e) and ("LDS" in str(e) or "not supported" in str(e)), str(e)
        _report("layers-stage %s refused: %s" % (tag, e))
        return
    ratios, both = [], []
    for strict in (False, True):
        for (case, ls), (layered, singles) in zip(pairs, res[strict]):
            check_exact(tag + (" strict" if strict else ""), case, ls, layered, singles, DENSE_REF_LAYERS)
        both.append(figures(tag + (" strict" if strict else ""), pairs, res[strict], DENSE_REF_LAYERS))
        ratios.append((max(f["max_ratio"] for _, f, _, _ in both[-1]), max(f["dense"] for _, f, _, _ in both[-1])))
    _report("layers-stage geometry | %s | max ratio over layers %.2f | strict %.2f | dense %.2f / %.2f" % (tag, ratios[0][0], ratios[1][0], ratios[0][1], ratios[1][1]))
    for strict in (False, True):
        judge(tag, both[strict])


@pytest.mark.parametrize("W", [16, 17])
def test_frames_one_tile_wide_with_and_without_a_ragged_column(hipctx, W):
    case = lc.narrow_dense_case(W)
    pairs = [(case, lc.layers(case, "sizes", 5, 9600 + W))]
    res = run_both_rules(hipctx, pairs)
    for strict in (False, True):
        (layered, singles), = res[strict]
        check_exact("%d wide%s" % (W, " strict" if strict else ""), case, pairs[0][1], layered, singles)
        judge("%d wide" % W, figures("%d wide" % W, pairs, res[strict]))


def test_invalid_stage_calls_are_refused_before_any_device_work(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    case = bc.FAMILIES["floor boundary"]()[0]
    H, W, _ = case.col.shape
    d = dict(col=_t(case.col), pc=_t(case.pixcov), mask=_t(case.mask.view(np.int32)), nsim=_t(case.nsim), state=_t(case.state))
    s_a, s_b = torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W, 3), device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    L = bh.lib()

    def call(layers, n=None, mask=d["mask"].data_ptr(), count=cnt.data_ptr(), w=1, b=6, width=W, null_list=False):
        arr = (bh.StageLayer * max(1, len(layers)))()
        for k, (c, v, o) in enumerate(layers):
            arr[k].d_colors, arr[k].d_pixel_cov, arr[k].d_sum = c, v, o
        rc = L.bcd_hip_bayes_accumulate_layers(hipctx.h, None if null_list else arr, len(layers) if n is None else n, mask, d["nsim"].data_ptr(), d["state"].data_ptr(),
                                               width, H, w, b, 1e-8, count, None)
        return rc, L.bcd_hip_last_error(hipctx.h).decode()

    good = (d["col"].data_ptr(), d["pc"].data_ptr(), s_a.data_ptr())
    good_b = (d["col"].data_ptr(), d["pc"].data_ptr(), s_b.data_ptr())
    EINVAL, EUNSUPPORTED = -1, -4
    cases = {
        "null mask": (call([good], mask=None), EINVAL), "null count": (call([good], count=None), EINVAL), "null layer list": (call([good], null_list=True), EINVAL),
        "null colours": (call([(None, good[1], good[2])]), EINVAL), "null covariances": (call([good, (good[0], None, good_b[2])]), EINVAL),
        "null sum": (call([good, (good[0], good[1], None)]), EINVAL), "no layer": (call([good], n=0), EINVAL), "too many layers": (call([good] * 17), EINVAL),
        "two equal sums": (call([good, good]), EINVAL), "overlapping sums": (call([good, (good[0], good[1], good[2] + 12 * W)]), EINVAL),
        "sum is an input": (call([good, (good[0], good[1], good[0])]), EINVAL), "sum is the count image": (call([(good[0], good[1], cnt.data_ptr())]), EINVAL),
        "empty image": (call([good], width=0), EINVAL), "negative radius": (call([good], w=-1), EINVAL), "search radius": (call([good, good_b], b=16), EUNSUPPORTED),
    }
    for name, ((rc, msg), want) in cases.items():
        assert rc == want and msg, (name, rc, msg)
    assert not s_a.any() and not s_b.any() and not cnt.any()            # nothing was launched
    for fn, args in (("bcd_hip_layers_finalize", (None, None, 1, None, C.c_int64(4))), ("bcd_hip_layers_downscale_avg", (None, None, 1, 8, 8)),
                     ("bcd_hip_layers_merge", (None, None, 17, 8, 8)), ("bcd_hip_layers_downscale_cov", (None, None, 0, None, 8, 8)),
                     ("bcd_hip_layers_pixel_cov", (None, 1, None, 8, 8, None, None))):
        assert getattr(L, fn)(hipctx.h, *args) == EINVAL, fn
    # ... and the context is as good as before
    ls = lc.layers(case, "sizes", 2)
    layered = run_layered(hipctx, case, ls)
    check_exact("after refusals", case, ls, layered, [run_single(hipctx, l, False) for l in ls])


def test_sixteen_layer_redo_counters_leave_the_similarity_verdict_alone(hipctx):
    """the per-layer redo counters of a 16-layer call come back into 15 host slots that lie two slots below the flags of the similarity pass
    (bcd_hip_similarity_masks_deferred / _verdict): with non-zero running totals up to the last slot, the verdict of a pass made before the estimate
    is the same after it"""
    import ctypes as C
    import oracle_lib as ol
    import bcd_amd.hip as bh
    W, H, b = 40, 30, 6
    col, ns, hist, cov, _ = ol.synth_inputs(W, H, 16, 21, 0.3, 0.0)
    d_hist, d_ns = _t(hist), _t(ns)
    import torch
    mask = torch.zeros((H, W, ((2 * b + 1) ** 2 + 31) // 32), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    L = bh.lib()
    assert L.bcd_hip_similarity_masks_deferred(hipctx.h, d_hist.data_ptr(), d_ns.data_ptr(), W, H, hist.shape[2], 1, b, 1.0, mask.data_ptr(), cnt.data_ptr()) == 0
    hipctx.synchronize()
    redo_masks = C.c_int(-1)
    assert L.bcd_hip_similarity_masks_verdict(hipctx.h, C.byref(redo_masks)) == 0 and redo_masks.value == 0
    case = next(c for c in bc.FAMILIES["floor boundary"]() if c.name == "floor k=0 e=1e-08")
    ls = lc.layers(case, "floor boundary", 16)
    layered = run_layered(hipctx, case, ls)
    redo = layered[2]
    _report("layers-stage 16 layers on %s: redo per layer %s" % (case.name, redo))
    assert redo[4] > 0 and redo[6] > 0 and layered[3] == sum(redo)
    after = C.c_int(-1)
    assert L.bcd_hip_similarity_masks_verdict(hipctx.h, C.byref(after)) == 0 and after.value == 0, "the estimate stage changed the verdict of the similarity pass"
    check_exact("16 layers after a deferred pass", case, ls, layered, [run_single(hipctx, l, False) for l in ls])


# ---- BCD_HIP_WEAK_LAYERS_GROUP: read once per process ----------------------------------------------------------------------------------------------
def test_layer_group_sizes_in_child_processes(tmp_path):
    """G = 1, 2, 3 forced through the environment in a fresh child each, one after the other, each under a time limit; the first abnormal exit ends the
    test.  The parent holds the children's arrays to float64 computed here: counts, patterns, the fallback bound per entry and layer (the group size
    only reaches the fallback kernel), the per-item / neighbourhood bars for the rest."""
    pairs = lc.group_cases()
    child = os.path.join(ROOT, "tests", "layer_cases.py")
    for G in (1, 2, 3):
        out = str(tmp_path / ("group%d.npz" % G))
        r = subprocess.run([sys.executable, child, out], env=dict(os.environ, BCD_HIP_WEAK_LAYERS_GROUP=str(G)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, "group size %d: the child ended with %d; no further child is started\n%s" % (G, r.returncode, (r.stdout + r.stderr)[-2000:])
        f = np.load(out)
        for i, (case, ls) in enumerate(pairs):
            sums, cnt = f["sums%d" % i], f["count%d" % i]
            fake = []
            for k, layer in enumerate(ls):
                s64, c64, items, s32 = references(layer)
                st.check_exact_parts(layer, sums[k], cnt, s64, c64)
                if not case.dense:
                    st.check_fallback_items(layer, sums[k], s64, items)
                fake.append(None)
            res = [((list(sums), cnt, [None] * len(ls), None), fake)]
            figs = judge("group %d %s" % (G, case.name), figures("group %d %s" % (G, case.name), [(case, ls)], res))
            _report("layers-stage group size %d | %s | max ratio %.2f dense %.2f" % (G, case.name, max(fg["max_ratio"] for _, fg in figs), max(fg["dense"] for _, fg in figs)))


# ---- the layer-batched streaming kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(97, 65), (64, 48), (5, 7), (4, 4)])
@pytest.mark.parametrize("L", [1, 2, 16])
def test_streaming_stage_calls_bitexact(hipctx, W, H, L):
    fails = fls.check_case(hipctx, W, H, L, 1000 * L + W)
    assert not fails, fails[:6]


def test_seeded_random_geometries_of_the_layered_streaming_stages_bitexact(hipctx):
    bad = []
    for i, (W, H, L, seed) in enumerate(fls.geometries(40, 11)):
        fails = fls.check_case(hipctx, W, H, L, seed)
        if fails:
            bad.append((i, W, H, L, fails[:3]))
    assert not bad, bad[:5]
