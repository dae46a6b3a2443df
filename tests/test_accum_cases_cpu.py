"""CPU tests of the constructed streams for the accumulator's binning (tests/accum_cases.py): the cases are what they claim to be, the
oracle accumulator is pinned on them to the reference's compiled one (live when oracle/_ref is present, and through tests/golden/
ref_accum_cases.npz anywhere), the project's host class equals the oracle bit for bit, and the oracle stays within the per-bin bound
against the float64 reference (accum_ref) with the recorded U_REF.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import accum_cases as ac
import accum_ref as ar
import bcd_amd.core as core
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_accum_cases.npz")
F32 = np.float32

_cache = {}


def oracle_of(name):
    """the oracle's four images of a case, computed once"""
    if name not in _cache:
        c = ac.get(name)
        _cache[name] = ol.oracle_ops()["accumulate"](ac.stream(c), c.W, c.H, c.nbins, c.gamma, c.maxval)
    return _cache[name]


def bits_equal(a, b):
    """the same bits, NaN == NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_case_shapes_and_frames():
    names = set(ac.ALL)
    for prm in ac.PARAMS:
        assert {"edges-%d-%g-%g" % prm, "specials-%d-%g-%g" % prm} <= names
    sizes = {ac.get(n).W * ac.get(n).H for n in ac.ALL}
    assert 1 in sizes and 35 in sizes                                  # one pixel; fewer pixels than a wavefront
    for n in ac.ALL:
        c = ac.get(n)
        N = c.W * c.H
        assert N < 400 and N % 64 != 0
        assert c.samples.dtype == F32 and c.samples.shape[0] == N and c.samples.shape[2] == 3
        assert c.weights is None or (c.weights.dtype == F32 and c.weights.shape == c.samples.shape[:2])
        assert (c.nbins > ac.ACCUM_MAX_BINS) == ((c.nbins, c.gamma, c.maxval) in ac.ONE_SHOT_PARAMS)
        if (c.nbins, c.gamma, c.maxval) in ac.ONE_SHOT_PARAMS:
            assert (c.W, c.H, c.samples.shape[1]) == (9, 7, 2)
    assert [p[0] for p in ac.ONE_SHOT_PARAMS] == [86, 213]
    assert 3 * 85 * 64 * 4 <= 64 * 1024 < 3 * 86 * 64 * 4 and 3 * 213 * 64 * 4 <= 160 * 1024 < 3 * 214 * 64 * 4
    assert set(ac.SPLAT) <= set(ac.ACCUM) and ac.U_DEVICE == math.ceil(4 * ac.U_REF)


@pytest.mark.parametrize("prm", ac.PARAMS, ids=lambda p: "%d-%g-%g" % p)
def test_every_bin_and_both_branches_are_reached(prm):
    """edges and specials of a parameter set together: every bin 0 .. nbins - 2 is the lower bin of some sample in every channel, the
    linear and the saturation branch are both taken (2 bins: saturation only), the clamp is reached, and the three channels of an edges
    sample carry different j"""
    nbins, gamma, maxval = prm
    v = np.concatenate([ac.transform(ac.get("%s-%d-%g-%g" % ((f,) + prm)).samples, gamma, maxval).reshape(-1, 3) for f in ("edges", "specials")])
    pos = v * (nbins - 2)
    lo = np.where(np.floor(pos) < nbins - 2, np.floor(pos), nbins - 2).astype(int)
    inner = np.abs(pos - np.rint(pos)) > 0.25                          # well inside a bin: the lower bin does not depend on powf's last bits
    for ch in range(3):
        assert set(lo[inner[:, ch] | (v[:, ch] > 1), ch]) == set(range(nbins - 1)), ch
        assert (v[:, ch] > 1).any() and (v[:, ch] == 2).any()
        assert nbins == 2 or (v[:, ch] < 1).any()
    L, js, _ = ac.edge_list(nbins, gamma, maxval)
    e = ac.get("edges-%d-%g-%g" % prm).samples.reshape(-1, 3)
    j_of = {float(x): int(j) for x, j in zip(L[::-1], js[::-1])}
    jj = np.array([[j_of[float(x)] for x in row] for row in e])
    assert np.all(jj[:, 0] != jj[:, 1]) and np.all(jj[:, 1] != jj[:, 2]) and np.all(jj[:, 0] != jj[:, 2])
    assert set(jj.reshape(-1)) == set(range(2 * ac.scale(nbins) + 1))  # every edge, through the clamp


@pytest.mark.parametrize("prm", ac.PARAMS + ac.ONE_SHOT_PARAMS, ids=lambda p: "%d-%g-%g" % p)
def test_edge_colours_sit_on_their_edges(prm):
    """the float64 bin position of every edge colour is within one fp32 ulp of its integer, and its fp32 neighbours are on either side"""
    nbins, gamma, maxval = prm
    m = ac.scale(nbins)
    L, js, kinds = ac.edge_list(nbins, gamma, maxval)
    for kind in (0, 1, 2):
        x, j = L[kinds == kind], js[kinds == kind]
        raw = np.where(x > 0, x.astype(np.float64), 0.0)               # (unclamped: the clamp hides the side of the last edge)
        if gamma > 1:
            raw = raw ** ac.exponent(gamma)
        if maxval > 0:
            raw = raw / np.float64(F32(maxval))
        pos = raw * m
        if kind == 1:
            assert np.all(np.abs(pos - j) <= np.spacing(j.astype(F32)).astype(np.float64))
        elif kind == 0:
            assert np.all(pos[1:] < j[1:]) and x[0] < 0                # (below colour 0: a negative subnormal, clamped to 0)
        else:
            assert np.all(pos > j)


def test_every_edges_case_holds_all_four_kinds_of_entry():
    """the float below an edge colour, the edge colour, the float above and the middle of a bin, in every channel of every edges case -- the
    sampled ones (86 and 213 bins on 126 slots, 35 pixels, 1 pixel) included; the sampled depths reach a part of the bins only, which the
    frame size fixes: the first and the last lower bin are among them"""
    for name in ac.ALL:
        if not name.startswith("edges"):
            continue
        c = ac.get(name)
        L, js, kinds = ac.edge_list(c.nbins, c.gamma, c.maxval)
        kind_of = {}
        for x, kd in zip(L, kinds):
            kind_of.setdefault(float(x), set()).add(int(kd))
        for ch in range(3):
            seen = set()
            for x in c.samples[:, :, ch].reshape(-1):
                seen |= kind_of[float(x)]
            assert seen == {0, 1, 2, 3}, (name, ch, seen)
        if c.nbins > ac.ACCUM_MAX_BINS:
            v = ac.transform(c.samples, c.gamma, c.maxval)
            lo = np.minimum(np.floor(v * (c.nbins - 2)), c.nbins - 2)
            assert lo.min() == 0 and lo.max() == c.nbins - 2 and (v > 1.5).any() and len(np.unique(lo)) < c.nbins - 1


def test_staged_kernel_cases_cover_the_depths():
    """what the GPU test relies on: the cases of k >= 8 samples per pixel take the LDS-staged dense kernel at the default depth, at 85 bins
    (65 280 B of LDS), at 2 bins and on the 1-pixel frame"""
    staged = [n for n in ac.ACCUM if ac.get(n).samples.shape[1] >= ac.STAGE_SPP]
    assert {ac.get(n).nbins for n in staged} >= {2, 18, 20, 85} and "edges1x1-20-2.2-2.5" in staged


def test_rounding_up_happens_at_inner_edges_and_never_into_saturation():
    ex = ac.rounding_up_examples((20, 0.5, 2.5))
    assert len(ex) >= 3 and all(v * 18 < j for _, v, j in ex)
    used = set(ex_x for ex_x, _, _ in ex)
    assert used & set(float(x) for x in ac.get("edges-20-0.5-2.5").samples.reshape(-1))
    below_one = np.nextafter(F32(1), F32(0))
    for nbins, _, _ in ac.PARAMS + ac.ONE_SHOT_PARAMS:
        m = nbins - 2
        assert m == 0 or F32(below_one * F32(m)) < F32(m), nbins       # (the proof in accum_cases: v < 1 never reaches the saturation branch)
    for m in range(1, 4096):
        assert F32(below_one * F32(m)) < F32(m)


def test_special_values_are_special():
    for prm in ac.PARAMS:
        nbins, gamma, maxval = prm
        S = ac.special_values(gamma, maxval)
        assert np.signbit(S[1]) and S[1] == 0 and np.isnan(S[3]) and S[4] == np.inf and S[5] == -np.inf
        assert 0 < S[6] < np.finfo(F32).tiny == S[7] and S[8] == np.finfo(F32).max
        v = ac.transform(S, gamma, maxval)
        assert abs(v[9] - 1) < 1e-6 and abs(v[10] - 2) < 1e-6 and v[11] == 2
        assert np.all(v[[0, 1, 2, 3, 5]] == 0) and v[4] == 2 and v[12] == 2
        smp = ac.get("specials-%d-%g-%g" % prm).samples
        for i, s in enumerate(S):                                      # alone in pixel i
            assert bits_equal(smp[i], np.full(smp[i].shape, s, F32))
        mixed = smp[2 * S.size:]
        assert np.isnan(mixed).any() and np.isinf(mixed).any() and np.isfinite(mixed[:, 0]).all()


def test_weights_family_mixes_the_weights_and_shares_bins():
    for prm in ac.WEIGHT_PARAMS:
        c = ac.get("weights-%d-%g-%g" % prm)
        assert c.samples.shape[1] == 9 >= ac.STAGE_SPP and set(np.unique(c.weights)) == set(ac.WEIGHT_SET)
        assert (c.weights.sum(1) > 0).all()
        assert np.mean([len(set(row)) >= 4 for row in c.weights]) > 0.8                       # mixed within a pixel
        v = ac.transform(c.samples, c.gamma, c.maxval)
        lo = np.minimum(np.floor(v * (c.nbins - 2)), c.nbins - 2)
        assert np.mean([len(set(lo[p, :, ch])) < 9 for p in range(lo.shape[0]) for ch in range(3)]) == 1.0   # samples share bins
        assert (v[:, :, 2] > 1).any()                                  # the last bin of the last channel is written


@pytest.mark.parametrize("nbins", ac.ONEHOT_BINS)
def test_onehot_expectation_is_one_hot_and_the_oracle_agrees(nbins):
    name = "onehot-%d" % nbins
    c, want = ac.get(name), ac.ONEHOT_EXPECTED[name]
    N = c.W * c.H
    assert N > 3 * nbins and N % 64 and want.shape == (N, 3 * nbins)
    w3 = want.reshape(N, 3, nbins)
    assert np.all(w3.sum(2) == 1) and set(np.unique(want)) == {0.0, 1.0}
    for ch in range(3):
        assert np.array_equal(np.argmax(w3[:, ch], 1), (np.arange(N) + 7 * ch) % (nbins - 1))
        assert set(np.argmax(w3[:, ch], 1)) == set(range(nbins - 1))
    assert bits_equal(oracle_of(name)[3].reshape(N, -1), want)


@pytest.mark.skipif(not ol.ref_available(), reason="oracle/_ref not built (the stored outputs of the next test pin the same)")
def test_oracle_equals_the_live_compiled_reference():
    r = ol.ref_ops()
    for name in ac.ALL:
        c = ac.get(name)
        want = r["accumulate"](ac.stream(c), c.W, c.H, c.nbins, c.gamma, c.maxval)
        for tag, g, w in zip(("ns", "mean", "cov", "hist"), oracle_of(name), want):
            assert bits_equal(g, w), (name, tag)


def test_oracle_equals_the_compiled_references_stored_outputs():
    """tests/golden/ref_accum_cases.npz (make_golden.py accum): the cases' inputs as they were when the reference ran, and its outputs"""
    z = np.load(GOLDEN)
    assert {k.split("/")[0] for k in z.files} == set(ac.ALL)
    for name in ac.ALL:
        c = ac.get(name)
        assert bits_equal(z[name + "/samples"], c.samples), name
        assert (c.weights is None) == (name + "/weights" not in z.files) and (c.weights is None or bits_equal(z[name + "/weights"], c.weights))
        for tag, g in zip(("ns", "mean", "cov", "hist"), oracle_of(name)):
            assert bits_equal(g, z[name + "/" + tag]), (name, tag)


def test_host_class_equals_the_oracle():
    for name in ac.ALL:
        c = ac.get(name)
        got = core.accumulate(ac.stream(c), c.W, c.H, c.nbins, c.gamma, c.maxval)
        for tag, g, w in zip(("ns", "mean", "cov", "hist"), got, oracle_of(name)):
            assert bits_equal(g, w), (name, tag)


def test_oracle_obeys_the_bound_with_u_ref():
    """U_ref: the smallest U for which the host arithmetic obeys the per-bin bound on every case; the recorded constant covers it (and is
    not stale by more than a tenth), without powf half an ulp of the division is all there is, and untouched bins are exactly 0"""
    worst, where = 0.0, None
    for name in ac.ALL:
        c = ac.get(name)
        r = ar.accumulate(ac.stream(c), c.W, c.H, c.nbins, c.gamma, c.maxval)
        terms = ar.bound_terms(r)
        hist = oracle_of(name)[3].reshape(r.hist.shape)
        u, at = ar.worst_u(hist, r, terms)
        print("%-24s U = %.4f  %s" % (name, u, ar.describe(r, at) if u > 1 else ""))
        assert np.all(hist[~terms[2]] == 0), name
        assert np.allclose(r.ns, oracle_of(name)[0].reshape(-1), rtol=1e-6, equal_nan=True)
        if not c.gamma > 1:
            assert u <= 0.5, name
        if u > worst:
            worst, where = u, name
    print("U_ref = %.4f at %s; recorded %.4g, device bound %d" % (worst, where, ac.U_REF, ac.U_DEVICE))
    assert ac.U_REF - 0.1 <= worst <= ac.U_REF


def test_float64_reference_statistics_track_the_oracle():
    """computeSampleStatistics of accum_ref against the oracle on a case with finite statistics (a sanity check of the reference itself)"""
    c = ac.get("edges-20-2.2-2.5")
    r = ar.accumulate(ac.stream(c), c.W, c.H, c.nbins, c.gamma, c.maxval)
    ns, mean, cov, hist = oracle_of(c.name)
    big = float(c.samples.max()) ** 2                                 # the covariance is a difference of sums of this size, rounded in fp32
    assert np.allclose(r.mean, mean.reshape(-1, 3), rtol=1e-5) and np.allclose(r.cov, cov.reshape(-1, 6), rtol=1e-3, atol=1e-5 * big)
    assert np.allclose(r.hist.sum(1), 3 * r.ns) and np.allclose(hist.reshape(r.hist.shape).sum(1), 3 * r.ns, rtol=1e-5)
