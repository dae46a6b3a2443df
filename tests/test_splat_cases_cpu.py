"""CPU tests of the constructed cases for the splatted add (tests/splat_cases.py): the two host restatements of the definition agree on
them, the gather form of k_accum_splat (cells within n, not K) loses nothing on any of them -- the classes with n == K included --, every
deliberately wrong gather model (splat_cases.MUTANTS) is told from the definition by some case in what the device test compares, and the
cases are what they are named for.  No GPU needed."""
import numpy as np
import pytest

import oracle_lib as ol
import splat_cases as sc
import splat_ref

F32 = np.float32

_cache = {}


def bits_equal(a, b):
    """the same bits, NaN == NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def definition_of(name):
    """(stream, samples_added, dropped) of a case by splat_ref.expand, computed once"""
    if name not in _cache:
        _cache[name] = sc.definition(sc.get(name))
    return _cache[name]


def statistics(c, stream):
    return ol.oracle_ops()["accumulate"](stream, c.W, c.H, c.nbins, c.gamma, c.maxval)


@pytest.mark.parametrize("name", sc.ALL)
def test_both_restatements_of_the_definition_agree(name):
    """no case is left out: the largest has fewer than 6000 samples, which the triple loop does in about two seconds"""
    c = sc.get(name)
    stream, added, dropped = definition_of(name)
    s2, a2, d2 = splat_ref.expand_loops(c.xy, c.rgb, c.weights, c.W, c.H, c.rx, c.ry, c.table)
    assert (a2, d2) == (added, dropped) and added + dropped == c.xy.shape[0]
    assert bits_equal(s2, stream)


@pytest.mark.parametrize("name", sc.ALL)
def test_the_gather_form_never_cuts_the_definition(name):
    """a cell further than n from a pixel holds no sample within the radius, so gathering from +-n cells gives what
    the definition's +-K candidates give -- the same contributions in the same order with the same weights, and the same counters"""
    c = sc.get(name)
    stream, added, dropped = definition_of(name)
    s2, a2, d2 = sc.gather(c)
    assert (a2, d2) == (added, dropped)
    assert bits_equal(s2, stream)
    wsum = np.zeros(c.W * c.H, np.float64)                      # (what the issue names: the per-pixel weight sums)
    w2 = wsum.copy()
    np.add.at(wsum, (stream[:, 0] * c.W + stream[:, 1]).astype(np.int64), stream[:, 5].astype(np.float64))
    np.add.at(w2, (s2[:, 0] * c.W + s2[:, 1]).astype(np.int64), s2[:, 5].astype(np.float64))
    assert np.array_equal(wsum, w2)


def test_every_mutant_is_separated_by_some_case():
    """a mutant is separated by a case when its four statistics (through the oracle accumulator: float32 sums in the order of AccSums::add)
    or its (samples_added, dropped) differ from the definition's -- what tests/test_gpu_splat_cases.py compares"""
    matrix = {m: [] for m in sc.MUTANTS}
    for name in sc.ALL:
        c = sc.get(name)
        stream, added, dropped = definition_of(name)
        want = None
        for m in sc.MUTANTS:
            s2, a2, d2 = sc.gather(c, m)
            hit = (a2, d2) != (added, dropped)
            if not hit and not bits_equal(s2, stream):           # (the same stream gives the same statistics)
                want = statistics(c, stream) if want is None else want
                hit = not all(bits_equal(g, w) for g, w in zip(statistics(c, s2), want))
            matrix[m].append(hit)
    width = max(len(n) for n in sc.ALL)
    print("\n%-*s  %s" % (width, "case", "  ".join(sc.MUTANTS)))
    for k, name in enumerate(sc.ALL):
        print("%-*s  %s" % (width, name, "  ".join(("x" if matrix[m][k] else ".").center(len(m)) for m in sc.MUTANTS)))
    print("%-*s  %s" % (width, "cases that separate", "  ".join(str(sum(matrix[m])).center(len(m)) for m in sc.MUTANTS)))
    for m in sc.MUTANTS:
        assert any(matrix[m]), "no case separates the mutant '%s' from the definition" % m
    clamp = [k for k, n in enumerate(sc.ALL) if n.startswith("clamp")]
    assert all(matrix["no-clamp"][k] for k in clamp)            # every clamp case is there for this one
    assert all(matrix["n-1"][k] for k, n in enumerate(sc.ALL) if n.startswith("class") and sc.get(n).facts["classes"][0][1] > 0)


def test_classes_are_the_stated_ones():
    assert len(sc.RADII) == len(sc.CLASSES) == 10
    assert [sc.geometry(r) for r in sc.RADII] == [(1, 0), (1, 0), (1, 1), (2, 1), (2, 1), (2, 2), (3, 2), (3, 2), (4, 3), (4, 3)]
    names = sc.FAMILIES["class"]
    on_x = [sc.get(n).facts["classes"][0] for n in names]
    on_y = [sc.get(n).facts["classes"][1] for n in names]
    assert on_x == sc.CLASSES and on_y == sc.CLASSES[::-1]
    assert all(sc.get(n).rx != sc.get(n).ry for n in names)
    radii = [(float(sc.get(n).rx), float(sc.get(n).ry)) for n in names]
    assert (3.0, 0.25) in radii and (0.25, 3.0) in radii
    for n in names:
        c = sc.get(n)
        for r in (c.rx, c.ry):
            K, nn = sc.geometry(r)
            assert splat_ref.filter_geometry(r, r)[4] == K and nn <= K
        for axis in ("dx", "dy"):
            assert c.facts[axis]["eq"] > 0 and c.facts[axis]["beside"] > 0 and c.facts[axis]["centre"] == 3
        assert c.facts["dx"]["below"] + c.facts["dy"]["below"] > 0 and c.facts["dx"]["above"] + c.facts["dy"]["above"] > 0
    assert sum((sc.get(n).facts["classes"][0][0] == sc.get(n).facts["classes"][0][1]) for n in names) == 2     # n == K on x, twice; as on y


def test_lattice_positions_are_on_the_comparisons():
    c = sc.get("class-3-0.25")
    x = c.xy[:, 0]
    frac = x - np.floor(x)
    assert (frac == 0).sum() > 100 and (frac == F32(0.5)).sum() > 100                       # cell borders and pixel centres
    for beside in (sc.above, sc.below):                       # and the floats beside them
        assert np.isin(x, [beside(F32(col)) for col in range(33)]).sum() > 50 and np.isin(x, [beside(F32(col) + F32(0.5)) for col in range(33)]).sum() > 50
    assert np.any(x == sc.above(0.0)) and np.any(x == sc.below(0.0))                         # (the smallest subnormals)
    cells = set(zip(np.floor(c.xy[:, 0]).astype(int).tolist(), np.floor(c.xy[:, 1]).astype(int).tolist()))
    assert {(cx, cy) for cx in range(-5, 33 + 5) for cy in range(-2, 9 + 2)} <= cells         # the frame extended by K + 1
    order = np.lexsort((c.xy[:, 0], c.xy[:, 1]))
    assert not np.array_equal(order, np.arange(order.size))                                  # shuffled
    assert set(np.unique(c.weights)) == {0.5, 1.0, 2.0}
    stream, added, dropped = definition_of(c.name)
    assert dropped > 0 and added > 0
    # a pixel's contributions come from several cells in non-monotone batch order
    e = sc._evaluate(c, True)
    s, k = np.nonzero(e["inside"])
    p = e["line"][s, k] * c.W + e["col"][s, k]
    key = e["l0"][s] * 1000 + e["c0"][s]
    one = p == np.argmax(np.bincount(p))                      # (the pixel with the most contributions)
    assert len(set(key[one])) >= 5 and np.any(np.diff(key[one]) < 0) and np.any(np.diff(key[one]) > 0)


def test_clamp_cases_reach_the_clamp():
    r = F32(1.75)
    d = sc.below(r)
    assert d < r and F32(d * (F32(1) / r)) == F32(1)
    assert {sc.get(n).table.shape[0] for n in sc.FAMILIES["clamp"]} == {1, 3, 64}
    for n in sc.FAMILIES["clamp"]:
        c = sc.get(n)
        assert c.facts["clamp"] > 0 and (c.rx == r or c.ry == r)
        T, ts = c.table, c.table.shape[0]
        flat = np.concatenate([T.reshape(-1), [sc.SENTINEL]])
        for iy in range(ts):                                  # what index ts of row iy would read is not the row's last entry
            assert flat[iy * ts + ts] != T[iy, ts - 1]
        if c.rx == r:
            want = {float(F32((F32(col) + F32(0.5)) - d)) for col in range(4)}
            assert want <= set(c.xy[:, 0].astype(float).tolist())
    assert sum(sc.get(n).facts["clamp"] for n in sc.ALL if not n.startswith("clamp")) == 0   # (none of the other radii reaches it)


def test_border_verdicts_sample_by_sample():
    for n in sc.FAMILIES["borders"]:
        c = sc.get(n)
        labels, want = c.facts["labels"], c.facts["verdicts"]
        assert len(labels) == len(want) == c.xy.shape[0]
        for i, (label, w) in enumerate(zip(labels, want)):
            _, a, d = splat_ref.expand(c.xy[i:i + 1], c.rgb[i:i + 1], c.weights[i:i + 1], c.W, c.H, c.rx, c.ry, c.table)
            assert (a, d) == ((1, 0) if w else (0, 1)), (n, label)
        _, added, dropped = definition_of(n)
        assert (added, dropped) == (sum(want), len(want) - sum(want)) and added >= 4
        for kind in ("== -K", "below -K", "below size + K", "== size + K", "-0", "NaN", "+inf", "-inf", "3e9", "first pixel at dx == r"):
            assert "x " + kind in labels and "y " + kind in labels
        assert "pixel centre under a zero entry" in labels


def test_frames_and_tables():
    assert sc.FRAMES == [(1, 1), (5, 3), (31, 7), (32, 8), (33, 9), (64, 16), (130, 2), (2, 70)]
    assert len(sc.FAMILIES["frame"]) == 24
    for n in sc.FAMILIES["frame"]:
        c = sc.get(n)
        _, added, dropped = definition_of(n)
        assert added > 0 and dropped > 0
    assert [sc.get(n).table.shape[0] for n in sc.FAMILIES["table"]] == [1, 2, 7, 64, 64]
    for n in sc.FAMILIES["table"][:4]:
        T = sc.get(n).table
        assert np.all(T > 0) and (T.shape[0] == 1 or np.all((T != T.T)[~np.eye(T.shape[0], dtype=bool)]))
    assert max(sc.get(n).xy.shape[0] for n in sc.ALL) < 6000 and max(c.W * c.H for c in map(sc.get, sc.ALL)) <= 64 * 16


def test_staging_cases_by_the_budget():
    """DESIGN.md section 10, LDS budget: (65536 - 4 (ts^2 + 2 * 532 + 4)) / 28 samples"""
    assert sc.max_staged(16) == 2151 and sc.max_staged(64) == 1602 and sc.max_staged(1) == (65536 - 4 * 1069) // 28
    f = {n: sc.get(n).facts for n in sc.FAMILIES["staging"]}
    for n, v in f.items():
        print("%-22s ring totals %s, cap %d of %d: %s" % (n, v["ring_totals"], v["cap"], v["budget"],
                                                           ", ".join("staged" if s else "global memory" for s in v["staged"])))
        assert v["classes"] == ((4, 3), (4, 3))
    assert 2 * f["staging-half"]["ring_totals"][0] <= 2151 and f["staging-half"]["staged"] == [True]
    assert f["staging-double"]["ring_totals"][0] >= 2 * 2151 and f["staging-double"]["staged"] == [False]
    a, b = f["staging-cluster-ts16"], f["staging-cluster-ts64"]
    assert a["ring_totals"] == b["ring_totals"] and a["cap"] == 2151 and b["cap"] == 1602
    assert a["staged"] == [True] * 4 and b["staged"] == [False, True, True, True]
    assert np.array_equal(sc.get("staging-cluster-ts16").xy, sc.get("staging-cluster-ts64").xy)


def test_default_parameter_variants():
    for n in sc.DEFAULTS:
        c, d = sc.get(n), sc.get(n + "@default")
        assert (d.nbins, d.gamma, d.maxval) == (20, 2.2, 2.5) and c.gamma == 1.0 and d.xy is c.xy and d.rgb is c.rgb
    assert [sc.get(n).facts["family"] for n in sc.DEFAULTS] == list(sc.FAMILIES)
