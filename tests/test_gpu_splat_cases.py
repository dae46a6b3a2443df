"""GPU tests of the splatted add on the constructed cases of tests/splat_cases.py: every (K, n) class of radii on each axis with n == K
among them, positions on the comparisons (dx == r and the floats beside it, cell borders, the borders of the key frame), the index clamp
at r = 1.75, tables of 1 to 64, frames below, at and one past the 32 x 8 tile, and ring totals on either side of the staging budget.

Expected: splat_ref.expand (the definition) gives the addSample stream and the counters, the oracle accumulator the statistics.  The cases
carry gamma = 1, where no powf is involved: all four outputs are held to the oracle's bits (tests/test_gpu_accum_binning.py establishes
that for the splatted path).  One case per family also runs at the default parameters, with the histogram bound of
test_gpu_accumulator.assert_matches_host.  tests/test_splat_cases_cpu.py shows that each of seven wrong kernels (<= for <, no clamp,
n one too small, a transposed table, exchanged inverses, a cell-ordered merge, drops counted per contribution) fails one of these."""
import numpy as np
import pytest

import oracle_lib as ol
import splat_cases as sc
from test_gpu_accumulator import assert_bits, assert_matches_host, bits_equal, dev, host, random_samples

pytestmark = pytest.mark.gpu

_expected = {}


def oracle(c, stream):
    return ol.oracle_ops()["accumulate"](np.ascontiguousarray(stream, np.float32), c.W, c.H, c.nbins, c.gamma, c.maxval)


def expected(name):
    """(the oracle's four images of the definition's stream, samples_added, dropped) of a case, computed once and left alone"""
    if name not in _expected:
        c = sc.get(name)
        stream, added, dropped = sc.definition(c)
        _expected[name] = (oracle(c, stream), added, dropped)
    return _expected[name]


def accumulator(ctx, c, **kw):
    acc = ctx.accumulator(c.W, c.H, c.nbins, c.gamma, c.maxval, **kw)
    acc.set_filter(c.table, (float(c.rx), float(c.ry)))
    return acc


def run(ctx, c, cuts=None, **kw):
    """one add_splatted call, or one per piece -> (the four images, info)"""
    n = c.xy.shape[0]
    acc = accumulator(ctx, c, **kw)
    cuts = [0, n] if cuts is None else cuts
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        acc.add_splatted(dev(c.xy[b0:b1]), dev(c.rgb[b0:b1]), dev(c.weights[b0:b1]))
    got, info = host(acc.statistics()), acc.info()
    acc.close()
    return got, info


def assert_case(c, got, info, want, added, dropped):
    assert info == (added, dropped), "%s: (samples_added, dropped) = %s, the definition has %s" % (c.name, info, (added, dropped))
    if c.gamma > 1:
        assert_matches_host(got, want)
        return
    for tag, g, w in zip(("nSamples", "mean", "covariance", "histogram"), got, want):
        if not bits_equal(g, w):
            g2, w2 = g.reshape(c.H * c.W, -1), w.reshape(c.H * c.W, -1)
            bad = np.flatnonzero(np.any((g2.view(np.uint32) != w2.view(np.uint32)) & ~(np.isnan(g2) & np.isnan(w2)), axis=1))
            p = int(bad[0])
            raise AssertionError("%s: %s differs from the definition at %d pixels; first (col %d, line %d): got %s, expected %s"
                                 % (c.name, tag, bad.size, p % c.W, p // c.W, g2[p], w2[p]))


@pytest.mark.parametrize("name", sc.ALL + [n + "@default" for n in sc.DEFAULTS])
def test_case_equals_the_definition(hipctx, name):
    c = sc.get(name)
    want, added, dropped = expected(name)
    assert (c.gamma == 1.0) == (not name.endswith("@default"))
    got, info = run(hipctx, c)
    assert_case(c, got, info, want, added, dropped)


def test_uneven_pieces_through_a_small_capacity(hipctx):
    """the 33 x 9 case at n = 3 in five uneven calls on an accumulator of capacity 700, so that the longer calls are split into chunks of
    700 as well: the bits of the single call"""
    name = "frame-33x9-n3"
    c = sc.get(name)
    n = c.xy.shape[0]
    want, added, dropped = expected(name)
    one, info = run(hipctx, c)
    assert_case(c, one, info, want, added, dropped)
    cuts = [0, 13, 900, 901, 1600, n]
    assert n - 1600 > 700 and 900 - 13 > 700
    pieces, info = run(hipctx, c, cuts, capacity=700)
    assert info == (added, dropped)
    assert_bits(pieces, one)


@pytest.mark.parametrize("name", ["frame-33x9-n3", "class-1.5+-1.5"])
def test_two_layers_at_the_widest_ring_and_at_n_equal_k(hipctx, name):
    """the LAYER instantiation of k_accum_splat at the 38 x 14 ring and where the ring starts at the edge of the key frame: each layer equals
    the definition on its own colours, the beauty is unchanged"""
    c = sc.get(name)
    (Kx, nx), (Ky, ny) = c.facts["classes"]
    assert (nx, ny) == (3, 3) or nx == Kx
    rng = np.random.default_rng(7)
    lay = [random_samples(rng, c.rgb.shape) for _ in range(2)]
    want, added, dropped = expected(name)
    acc = accumulator(hipctx, c, layers=2)
    acc.add_splatted(dev(c.xy), dev(c.rgb), dev(c.weights), layers=[dev(l) for l in lay])
    beauty, info = host(acc.statistics()), acc.info()
    got = [(m.cpu().numpy(), v.cpu().numpy()) for m, v in acc.layer_statistics()]
    acc.close()
    assert_case(c, beauty, info, want, added, dropped)
    for k, l in enumerate(lay):
        stream, a, d = sc.definition(c._replace(rgb=l))
        assert (a, d) == (added, dropped)
        w = oracle(c, stream)
        assert bits_equal(got[k][0], w[1]), "%s, layer %d: mean" % (name, k)
        assert bits_equal(got[k][1], w[2]), "%s, layer %d: covariance" % (name, k)


def test_two_filters_on_one_accumulator_without_synchronisation(hipctx):
    """filter A (3, 0.25, a 64 x 64 table), a splat, filter B (nextafter(0.5), 1.75, a 1 x 1 table), a splat, A again, a splat -- nothing
    between the calls waits for the device, so the second and third set_filter find the table's pinned staging buffer in flight: the
    statistics are the oracle's on the three expanded streams one after the other"""
    W, H = 33, 9
    A = (sc.RADII[9], sc.RADII[0], sc.ramp_table(64))
    B = (sc.RADII[2], np.float32(1.75), sc.ramp_table(1))
    parts = []
    for k, (rx, ry, T) in enumerate((A, B, A)):
        xy, _ = sc.constructed_positions(W, H, rx, ry, 3, 4)
        parts.append(sc.make_case("two-filters-%d" % k, W, H, rx, ry, T, xy, 700 + k))
    assert parts[0].facts["classes"] == ((4, 3), (1, 0)) and parts[1].facts["classes"] == ((1, 1), (3, 2)) and parts[1].facts["clamp"] > 0
    assert not np.array_equal(parts[0].xy, parts[2].xy)
    c0 = parts[0]
    on_device = [(dev(c.xy), dev(c.rgb), dev(c.weights)) for c in parts]                     # (uploaded before the first call)
    acc = hipctx.accumulator(W, H, c0.nbins, c0.gamma, c0.maxval)
    for c, d in zip(parts, on_device):
        acc.set_filter(c.table, (float(c.rx), float(c.ry)))
        acc.add_splatted(*d)
    got, info = host(acc.statistics()), acc.info()
    acc.close()
    streams, added, dropped = [], 0, 0
    for c in parts:
        s, a, d = sc.definition(c)
        streams.append(s)
        added, dropped = added + a, dropped + d
    assert all(s.shape[0] > 1000 for s in streams)
    assert_case(c0, got, info, oracle(c0, np.concatenate(streams, 0)), added, dropped)
