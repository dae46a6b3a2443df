"""Constructed positions, radii, tables and frames for the splatted add (k_accum_splat_keys / _cells / k_accum_splat in k_accumulate.hip;
tests/test_splat_cases_cpu.py, tests/test_gpu_splat_cases.py).  TEST INFRASTRUCTURE, NumPy only; importing it loads no native library.

The definition is tests/splat_ref.py.  Random positions and the radii 0.5 .. 2.0 leave the kernels' edge logic unreached; these cases put
samples on it.  Every float is built in float32 and what a case is named for is asserted here, at import.  A case is
    (W, H, rx, ry, table, nbins, gamma, maxval, xy [n, 2], rgb [n, 3], weights [n], name, facts)
with facts a dict of what the case claims (its classes, the contributions that reach the index clamp, per-sample verdicts, ring totals).
The cases carry gamma = 1 (no powf: the device's histogram is held to the oracle's bits); get(name + "@default") is the same case at the
accumulator's default parameters.

The two neighbour ranges of an axis of radius r (restated from bcd_hip_accum_set_filter and DESIGN.md section 10):
    K = (int)ceilf(r + 0.5f)                       the candidate range of the definition, and the extension of the key frame
    n = the smallest integer with n + 0.5f >= r    the cells a pixel gathers from (the ring of a tile is its cells plus n on each side)
n <= K always, and n == K where r + 0.5f rounds down to an integer: r = nextafter(0.5f), nextafter(1.5f).

Families:
  class-*     one case per (K, n) class of RADII on x against another class on y (rx != ry), 33 x 9: the lattice of lattice() on every
              cell of the frame extended by K + 1, and the cross product of the positions that put dx (dy) at r, the floats beside r
              and the floats beside the position of dx == r for the pixels 0 .. 2, with those pixels' centres.  Shuffled with a fixed seed.
  clamp-*     r = 1.75 on x, on y and on both, tables of 1, 3 and 64, 6 x 5: dx = nextbelow(1.75f) < r while dx * (1.f / r) rounds to
              1.0f, so (int)(dx * inv_r * ts) = ts and the clamp to ts - 1 is what keeps the index in its row.  All entries of
              ramp_table differ, so the entry an unclamped flat index reads -- the first of the next row, or one past the table -- is another.
  borders-*   one sample per verdict of the key-frame test and the footprint test, on x and on y; facts["verdicts"] says which are added.
  frame-*     1x1, 5x3, 31x7, 32x8, 33x9, 64x16, 130x2, 2x70 at n = 0, n = 3 (the 38 x 14 ring) and n == K on both axes.
  table-*     tables of 1, 2, 7 and 64 with T[i][j] != T[j][i], and Blackman-Harris of radius 3 at 64.
  staging-*   ring totals against the staging budget of a workgroup, see max_staged().

MUTANTS: gather(case, mutant) is a CPU model of the kernel -- the definition restricted to the cells within n of a pixel, with the
kernel's splat_weight -- with one deliberate error.  Unmutated it gives the definition's stream; every mutant must differ from the
definition on some case in what the device test sees (the four statistics, samples_added, dropped).  Truncation in place of floor is
not listed: the pixels it would lose lie outside the frame."""
import collections
import math

import numpy as np

import splat_ref
from test_gpu_accumulator import random_samples

F32 = np.float32

Case = collections.namedtuple("Case", "W H rx ry table nbins gamma maxval xy rgb weights name facts")

NBINS, GAMMA, MAXVAL = 20, 1.0, 2.5                # the cases' own parameters: no powf
DEFAULT_PARAMS = (20, 2.2, 2.5)                    # Context.accumulator's defaults
WEIGHTS = np.array([0.5, 1.0, 2.0], F32)
SENTINEL = F32(1024.0)                             # what the "no-clamp" mutant reads past the table

TILE_X, TILE_Y = 32, 8                             # SPLAT_TX, SPLAT_TY
RING_MAX = (TILE_X + 6) * (TILE_Y + 6)             # SPLAT_RING_MAX: 38 x 14 = 532 cells


def below(v):
    return np.nextafter(F32(v), F32(-np.inf))


def above(v):
    return np.nextafter(F32(v), F32(np.inf))


def geometry(r):
    """(K, n) of one axis, restated"""
    r = F32(r)
    K = int(np.ceil(r + F32(0.5)))
    n = 0
    while F32(n) + F32(0.5) < r:
        n += 1
    return K, min(n, K)


RADII = [F32(0.25), F32(0.5), above(0.5), F32(1.0), F32(1.5), above(1.5), F32(2.0), F32(2.5), above(2.5), F32(3.0)]
RADIUS_TAGS = ["0.25", "0.5", "0.5+", "1", "1.5", "1.5+", "2", "2.5", "2.5+", "3"]
CLASSES = [(1, 0), (1, 0), (1, 1), (2, 1), (2, 1), (2, 2), (3, 2), (3, 2), (4, 3), (4, 3)]
assert [geometry(r) for r in RADII] == CLASSES
assert all(r.dtype == F32 and 0 < r <= 3 for r in RADII) and RADII[2] > 0.5 and RADII[5] > 1.5 and RADII[8] > 2.5
for _r, (_K, _n) in zip(RADII, CLASSES):
    assert splat_ref.filter_geometry(_r, _r)[4:] == (_K, _K)
    assert F32(_n) + F32(0.5) >= _r and (_n == 0 or F32(_n - 1) + F32(0.5) < _r)
# n == K: r + 0.5f is a tie between an integer and the float above it and rounds to the even one, the integer
assert RADII[2] + F32(0.5) == F32(1) and RADII[5] + F32(0.5) == F32(2) and RADII[8] + F32(0.5) > F32(3)


def max_staged(ts):
    """samples the staging arrays of a workgroup hold at most ("LDS budget": 64 KiB less the table, the ring's
    starts g0[532] and b0[532 + 4], over 28 bytes per sample)"""
    return (65536 - 4 * (ts * ts + 2 * RING_MAX + 4)) // 28


assert max_staged(16) == 2151 and max_staged(64) == 1602


def staging_cap(m, ring, N, ts):
    """the capacity of the staging arrays for a chunk of m samples (accum_add_splatted): 1.5 times the average ring, 8 sigma and 64"""
    avg = m * ring / N
    return int(min(float(max_staged(ts)), 1.5 * avg + 8.0 * math.sqrt(avg) + 64.0))


def ramp_table(ts, zeros=()):
    """all entries different, positive and T[i][j] != T[j][i]; zeros: (row, column) slices set to 0 for an empty footprint"""
    T = (F32(0.5) + np.arange(ts * ts, dtype=F32).reshape(ts, ts) / F32(2 * ts * ts)).astype(F32)
    assert len(np.unique(T)) == ts * ts and np.all(T > 0) and (ts == 1 or np.all((T != T.T)[~np.eye(ts, dtype=bool)]))
    for rows, cols in zeros:
        T[rows, cols] = 0
    return T


# ---- positions ----------------------------------------------------------------------------------------------------------------------------

def cell_positions(c):
    """six positions of cell c = [c, c + 1): its border, the float above it, the floats around the centre, the last float of the cell"""
    c = F32(c)
    p = [c, above(c), below(c + F32(0.5)), c + F32(0.5), above(c + F32(0.5)), below(c + F32(1))]
    assert all(v.dtype == F32 and np.floor(v) == c for v in p) and all(a < b for a, b in zip(p[:-1], p[1:]))
    return p


def lattice(W, H, Kx, Ky, per_cell):
    """per_cell positions in every cell of the frame extended by K + 1: the pairs of cell_positions rotate with the cell, so that all 36
    occur and neighbouring cells differ"""
    ox = {c: cell_positions(c) for c in range(-(Kx + 1), W + Kx + 1)}
    oy = {c: cell_positions(c) for c in range(-(Ky + 1), H + Ky + 1)}
    out = []
    for cy in sorted(oy):
        for cx in sorted(ox):
            for j in range(per_cell):
                q = (5 * cx + 7 * cy + 11 * j) % 36
                out.append((ox[cx][q % 6], oy[cy][q // 6]))
    return np.array(out, F32).reshape(-1, 2)


def radius_positions(r, size, cols):
    """positions of one axis at which a pixel 0 .. cols - 1 sees dx == r ("eq": excluded), nextbelow(r) ("below": included) and
    nextafter(r) ("above"), built as (col + 0.5f) -/+ value and kept where float32 gives exactly that dx; "beside": the floats on either
    side of an "eq" position; "centre": dx == 0"""
    r = F32(r)
    out = {"eq": [], "below": [], "above": [], "beside": [], "centre": []}
    for col in range(min(size, cols)):
        ctr = F32(col) + F32(0.5)
        out["centre"].append(ctr)
        for sign in (-1, 1):
            for tag, v in (("eq", r), ("below", below(r)), ("above", above(r))):
                x = F32(ctr - v) if sign < 0 else F32(ctr + v)
                if np.abs(ctr - x) == v:
                    out[tag].append(x)
                    if tag == "eq":
                        out["beside"] += [below(x), above(x)]
    return out


def constructed_positions(W, H, rx, ry, per_cell, cols):
    """-> (xy, facts): the lattice and the cross product of the two axes' radius_positions"""
    (Kx, _), (Ky, _) = geometry(rx), geometry(ry)
    px, py = radius_positions(rx, W, cols), radius_positions(ry, H, cols)
    xs, ys = np.array(sum(px.values(), []), F32), np.array(sum(py.values(), []), F32)
    cross = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    facts = {"dx": {k: len(v) for k, v in px.items()}, "dy": {k: len(v) for k, v in py.items()}}
    return np.concatenate([lattice(W, H, Kx, Ky, per_cell), cross]).astype(F32), facts


# ---- the gather model and its mutants -------------------------------------------------------------------------------------------------------

MUTANTS = ["le", "no-clamp", "n-1", "transposed", "swapped-inv", "cell-order", "dropped-per-contribution"]


def _evaluate(c, gathered, mutant=None):
    """the footprint test for every sample of the key frame and every pixel of its neighbourhood: +-n cells (gathered, as k_accum_splat
    and k_accum_splat_keys) or +-K (the definition)"""
    T = np.ascontiguousarray(c.table, F32)
    ts = T.shape[0]
    rx, ry = F32(c.rx), F32(c.ry)
    inv_rx, inv_ry = F32(1) / rx, F32(1) / ry
    (Kx, nx), (Ky, ny) = geometry(rx), geometry(ry)
    if mutant == "n-1":
        nx, ny = max(nx - 1, 0), max(ny - 1, 0)
    if mutant == "transposed":
        T = np.ascontiguousarray(T.T)
    if mutant == "swapped-inv":
        inv_rx, inv_ry = inv_ry, inv_rx
    ax, ay = (nx, ny) if gathered else (Kx, Ky)
    x, y = c.xy[:, 0], c.xy[:, 1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & (x >= F32(-Kx)) & (x < F32(c.W + Kx)) & (y >= F32(-Ky)) & (y < F32(c.H + Ky))
    idx = np.nonzero(ok)[0]
    x, y = x[idx][:, None], y[idx][:, None]
    c0, l0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    dl, dc = np.meshgrid(np.arange(-ay, ay + 1), np.arange(-ax, ax + 1), indexing="ij")
    col, line = c0 + dc.reshape(1, -1), l0 + dl.reshape(1, -1)
    dx, dy = np.abs((col.astype(F32) + F32(0.5)) - x), np.abs((line.astype(F32) + F32(0.5)) - y)
    assert dx.dtype == F32 and dy.dtype == F32
    near = ((dx <= rx) & (dy <= ry)) if mutant == "le" else ((dx < rx) & (dy < ry))
    ix, iy = (dx * inv_rx * F32(ts)).astype(np.int64), (dy * inv_ry * F32(ts)).astype(np.int64)
    if mutant == "no-clamp":
        flat = np.concatenate([T.reshape(-1), np.full(ts + 2, SENTINEL, F32)])
        f = flat[np.minimum(iy * ts + ix, flat.size - 1)]
    else:
        f = T[np.minimum(iy, ts - 1), np.minimum(ix, ts - 1)]
    inside = near & (col >= 0) & (col < c.W) & (line >= 0) & (line < c.H) & (f != 0)
    return dict(idx=idx, c0=c0[:, 0], l0=l0[:, 0], col=col, line=line, f=f, inside=inside, clamped=inside & ((ix >= ts) | (iy >= ts)))


def gather(c, mutant=None):
    """-> (stream (m, 6) float32 as splat_ref.expand's, samples_added, dropped) of the gather model"""
    assert mutant is None or mutant in MUTANTS
    e = _evaluate(c, True, mutant)
    n, inside = c.xy.shape[0], e["inside"]
    dropped = n - int(np.count_nonzero(inside.any(axis=1)))
    if mutant == "dropped-per-contribution":
        dropped = (n - e["idx"].size) + int(np.count_nonzero(~inside))
    s, k = np.nonzero(inside)                                  # sample after sample, each line ascending, col ascending
    i = e["idx"][s]
    wf = c.weights[i] * e["f"][s, k]
    assert wf.dtype == F32
    stream = np.stack([e["line"][s, k].astype(F32), e["col"][s, k].astype(F32), c.rgb[i, 0], c.rgb[i, 1], c.rgb[i, 2], wf], 1)
    if mutant == "cell-order":                                 # a pixel's contributions cell after cell (ring order), not by batch position
        stream = stream[np.lexsort((i, e["c0"][s], e["l0"][s]))]
    return np.ascontiguousarray(stream, F32), n - dropped, dropped


def definition(c):
    return splat_ref.expand(c.xy, c.rgb, c.weights, c.W, c.H, c.rx, c.ry, c.table)


def clamp_reached(c):
    """contributions of the definition whose index is ts before the clamp, on either axis"""
    return int(np.count_nonzero(_evaluate(c, False)["clamped"]))


def verdicts(c):
    """per sample: does it contribute (the definition, sample by sample)"""
    e = _evaluate(c, False)
    out = np.zeros(c.xy.shape[0], bool)
    out[e["idx"]] = e["inside"].any(axis=1)
    return out


def ring_totals(c):
    """per tile of 32 x 8 pixels, row-major: the samples in the cells of its ring that are not dropped -- what k_accum_splat compares with
    the capacity of its staging arrays"""
    (_, nx), (_, ny) = geometry(c.rx), geometry(c.ry)
    e = _evaluate(c, False)
    keep = e["inside"].any(axis=1)
    c0, l0 = e["c0"][keep], e["l0"][keep]
    out = []
    for py0 in range(0, c.H, TILE_Y):
        for px0 in range(0, c.W, TILE_X):
            out.append(int(np.count_nonzero((c0 >= px0 - nx) & (c0 < px0 + TILE_X + nx) & (l0 >= py0 - ny) & (l0 < py0 + TILE_Y + ny))))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

_cases = {}
_lazy = {}                                         # name -> builder of a case that needs the native library: built by the first get()
ALL = []
FAMILIES = collections.OrderedDict()


def make_case(name, W, H, rx, ry, table, xy, seed, facts=None, shuffle=True):
    """a case on the positions xy, in an order shuffled with the seed, colours of random_samples and weights 0.5, 1 and 2"""
    rng = np.random.default_rng(seed)
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    if shuffle:
        xy = np.ascontiguousarray(xy[rng.permutation(xy.shape[0])])
    n = xy.shape[0]
    rx, ry = F32(rx), F32(ry)
    facts = dict(facts or {}, classes=(geometry(rx), geometry(ry)))
    c = Case(W, H, rx, ry, np.ascontiguousarray(table, F32), NBINS, GAMMA, MAXVAL, xy, random_samples(rng, (n, 3)), rng.choice(WEIGHTS, n),
             name, facts)
    c.facts["clamp"] = clamp_reached(c)
    assert xy.dtype == F32 and c.rgb.dtype == F32 and c.weights.dtype == F32
    return c


def _add(family, name, W, H, rx, ry, table, xy, seed, facts, shuffle=True):
    assert name not in ALL
    c = _cases[name] = make_case(name, W, H, rx, ry, table, xy, seed, dict(facts, family=family), shuffle)
    ALL.append(name)
    FAMILIES.setdefault(family, []).append(name)
    return c


def _build_classes():
    for i, tag in enumerate(RADIUS_TAGS):
        j = len(RADII) - 1 - i                                 # (0.25, 3), (0.5, 2.5+), ... (3, 0.25): every class on x and on y
        rx, ry = RADII[i], RADII[j]
        assert rx != ry
        xy, facts = constructed_positions(33, 9, rx, ry, 6, 3)
        c = _add("class", "class-%s-%s" % (tag, RADIUS_TAGS[j]), 33, 9, rx, ry, ramp_table(5), xy, 100 + i, facts)
        assert c.facts["classes"] == (CLASSES[i], CLASSES[j])
        for axis in ("dx", "dy"):
            assert facts[axis]["eq"] > 0 and facts[axis]["beside"] > 0


def _build_clamp():
    r = F32(1.75)
    d = below(r)
    assert d < r and F32(d * (F32(1) / r)) == F32(1)           # inside the radius, yet the quotient rounds to 1: the index before the clamp is ts
    for col in range(4):
        x = F32((F32(col) + F32(0.5)) - d)
        assert np.abs((F32(col) + F32(0.5)) - x) == d          # these positions have exactly that dx in float32
    for k, (tag, rx, ry) in enumerate((("x", r, F32(1.0)), ("y", F32(1.0), r), ("xy", r, r))):
        for ts in (1, 3, 64):
            assert F32(F32(d * (F32(1) / r)) * F32(ts)) == F32(ts)
            xy, facts = constructed_positions(6, 5, rx, ry, 2, 4)
            c = _add("clamp", "clamp-%s-ts%d" % (tag, ts), 6, 5, rx, ry, ramp_table(ts), xy, 200 + 10 * k + ts, facts)
            assert c.facts["clamp"] > 0 and facts["dx" if tag != "y" else "dy"]["below"] >= 4


def _build_borders():
    for k, (tag, rx, ry) in enumerate((("r1", F32(1.0), F32(1.0)), ("nK", above(0.5), above(1.5)))):
        W, H = 5, 3
        (Kx, _), (Ky, _) = geometry(rx), geometry(ry)
        T = ramp_table(4, zeros=((0, slice(None)), (slice(None), 0)))                       # dx or dy below r / 4: no contribution
        samples, labels, want = [], [], []
        for axis, (size, K, r, ro) in enumerate(((W, Kx, rx, ry), (H, Ky, ry, rx))):
            other = F32(F32(1.5) - F32(0.6) * ro)              # the other axis: 0.6 r from the centre of pixel 1, index 2 of 4
            edge = F32(size) - F32(0.5)                        # the centre of the last pixel
            zero = F32(-0.0)
            assert np.signbit(zero) and zero == 0
            plain = [("== -K", F32(-K), False), ("below -K", below(-K), False), ("below size + K", below(size + K), False),
                     ("== size + K", F32(size + K), False), ("-0", zero, True), ("NaN", F32(np.nan), False), ("+inf", F32(np.inf), False),
                     ("-inf", F32(-np.inf), False), ("3e9", F32(3e9), False)]
            first, inner = F32(F32(0.5) - r), F32(F32(0.5) - below(r))                       # left of pixel 0: dx == r is outside, nextbelow(r) inside
            assert np.abs(F32(0.5) - first) == r and np.abs(F32(0.5) - inner) == below(r)
            plain += [("first pixel at dx == r", first, False), ("first pixel at dx == nextbelow(r)", inner, True)]
            last = F32(edge + r)                               # right of the last pixel, where (size - 0.5f) + r is a float
            if np.abs(edge - last) == r:
                assert np.abs(edge - below(last)) < r
                plain += [("last pixel at dx == r", last, False), ("last pixel, the float below that position", below(last), True)]
            else:
                assert tag == "nK"
            for label, v, added in plain:
                samples.append((v, other) if axis == 0 else (other, v))
                labels.append("xy"[axis] + " " + label)
                want.append(added)
        samples.append((F32(2.5), F32(1.5)))                   # a pixel's centre: index 0 on both axes, where the table is 0
        labels.append("pixel centre under a zero entry")
        want.append(False)
        c = _add("borders", "borders-" + tag, W, H, rx, ry, T, np.array(samples, F32), 300 + k, {"labels": labels, "verdicts": want}, shuffle=False)
        got = verdicts(c)
        assert [bool(g) for g in got] == want, [(l, bool(g), w) for l, g, w in zip(labels, got, want) if bool(g) != w]


FRAMES = [(1, 1), (5, 3), (31, 7), (32, 8), (33, 9), (64, 16), (130, 2), (2, 70)]
FRAME_CLASSES = [("n0", RADII[1], RADII[0]), ("n3", RADII[9], RADII[8]), ("nK", RADII[5], RADII[2])]


def _build_frames():
    for a, (W, H) in enumerate(FRAMES):
        for b, (tag, rx, ry) in enumerate(FRAME_CLASSES):
            (Kx, nx), (Ky, ny) = geometry(rx), geometry(ry)
            assert {"n0": nx == ny == 0, "n3": nx == ny == 3, "nK": nx == Kx and ny == Ky}[tag]
            _add("frame", "frame-%dx%d-%s" % (W, H, tag), W, H, rx, ry, ramp_table(6), lattice(W, H, Kx, Ky, 3), 400 + 10 * a + b, {})


def _blackman_harris():
    """the one case whose table comes from the library (bcd_hip_filter_table, host only).  Built by the first get() and not at import: a test
    module that loaded the library while pytest collects would map its HIP runtime before torch has mapped its own, and the context of the
    GPU tests would then fail to open"""
    import bcd_amd.hip as bh
    T = bh.filter_table("blackman_harris", 3.0, table_size=64)
    assert T.shape == (64, 64) and T.dtype == F32 and np.all(T >= 0)
    xy, facts = constructed_positions(9, 5, F32(3.0), F32(3.0), 6, 3)
    return make_case("table-blackman-harris-ts64", 9, 5, F32(3.0), F32(3.0), T, xy, 599, dict(facts, family="table"))


def _build_tables():
    rx, ry = F32(2.0), F32(1.25)
    for ts in (1, 2, 7, 64):
        xy, facts = constructed_positions(9, 5, rx, ry, 6, 3)
        _add("table", "table-ts%d" % ts, 9, 5, rx, ry, ramp_table(ts), xy, 500 + ts, facts)
    _lazy["table-blackman-harris-ts64"] = _blackman_harris
    ALL.append("table-blackman-harris-ts64")
    FAMILIES["table"].append("table-blackman-harris-ts64")


def _build_staging():
    """The path a tile takes: staged iff its ring total <= cap = min(max_staged(ts), 1.5 avg + 8 sqrt(avg) + 64), avg = n * ring / (W H).
    On a one-tile frame at n = 3 the ring is 532 cells for 256 pixels, so 1.5 avg alone is more than 3 n: cap < total only through
    max_staged.  No case sits within a factor of 2 of the switch, except the pair, which sits between the two budgets on purpose."""
    rx, ry = RADII[9], RADII[8]                                # n = 3 on both axes: the 38 x 14 ring
    (Kx, nx), (Ky, ny) = geometry(rx), geometry(ry)
    ring = (TILE_X + 2 * nx) * (TILE_Y + 2 * ny)
    assert ring == RING_MAX

    def finish(c, must_stage):
        tot = ring_totals(c)
        cap = staging_cap(c.xy.shape[0], ring, c.W * c.H, c.table.shape[0])
        c.facts.update(ring_totals=tot, cap=cap, staged=[t <= cap for t in tot], budget=max_staged(c.table.shape[0]))
        assert c.facts["staged"][0] == must_stage
        return tot, cap

    # staged: the lattice's one sample per cell, at most half of the 2151 of a 16 x 16 table in the ring
    c = _add("staging", "staging-half", 32, 8, rx, ry, ramp_table(16), lattice(32, 8, Kx, Ky, 1), 600, {})
    tot, cap = finish(c, True)
    assert len(tot) == 1 and 0 < 2 * tot[0] <= max_staged(16) and cap >= tot[0] and tot[0] == definition(c)[1]
    # not staged: 4600 samples inside the frame, all in the one ring, at least double the budget
    rng = np.random.default_rng(601)
    xy = (rng.random((4600, 2), dtype=F32) * np.array([32, 8], F32)).astype(F32)
    c = _add("staging", "staging-double", 32, 8, rx, ry, ramp_table(16), xy, 601, {})
    tot, cap = finish(c, False)
    assert len(tot) == 1 and tot[0] >= 2 * max_staged(16) and cap == max_staged(16) and tot[0] == definition(c)[1]
    # the pair: 1800 samples in cell (16, 4) of a 33 x 9 frame and 150 elsewhere.  The chunk is dense enough for cap = max_staged at both
    # table sizes; the first tile's ring holds the cluster: staged under the 2151 of ts = 16, from global memory over the 1602 of ts = 64
    rng = np.random.default_rng(602)
    cluster = (np.array([16, 4], F32) + rng.random((1800, 2), dtype=F32)).astype(F32)
    rest = (rng.random((150, 2), dtype=F32) * np.array([33 + 2 * Kx, 9 + 2 * Ky], F32) - np.array([Kx, Ky], F32)).astype(F32)
    xy = np.concatenate([cluster, rest])
    assert np.all(np.floor(cluster) == np.array([16, 4], F32))
    for ts, must_stage in ((16, True), (64, False)):
        c = _add("staging", "staging-cluster-ts%d" % ts, 33, 9, rx, ry, ramp_table(ts), xy, 602, {})
        tot, cap = finish(c, must_stage)
        assert cap == max_staged(ts) and len(tot) == 4 and 1800 <= tot[0] <= 1950 and all(t <= 150 for t in tot[1:])
        assert max_staged(64) < tot[0] <= max_staged(16) and all(c.facts["staged"][1:])


_build_classes()
_build_clamp()
_build_borders()
_build_frames()
_build_tables()
_build_staging()

DEFAULTS = ["class-3-0.25", "clamp-xy-ts3", "borders-r1", "frame-33x9-n3", "table-ts7", "staging-cluster-ts64"]   # one per family
assert [_cases[n].facts["family"] for n in DEFAULTS] == list(FAMILIES)


def get(name):
    """a case; name + "@default": the same at the accumulator's default parameters (gamma 2.2: the histogram goes through powf)"""
    if name.endswith("@default"):
        c = get(name[:-len("@default")])
        return c._replace(nbins=DEFAULT_PARAMS[0], gamma=DEFAULT_PARAMS[1], maxval=DEFAULT_PARAMS[2], name=name)
    if name in _lazy:
        _cases[name] = _lazy.pop(name)()
    return _cases[name]
