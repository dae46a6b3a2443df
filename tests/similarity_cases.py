"""Constructed histogram frames for similar-patch selection (tests/test_gpu_similarity_stage.py).  TEST INFRASTRUCTURE.

Rendered frames put a few thousand of 10^8 patch pairs near the threshold and none on it.  These frames are made of two or three pixel TYPES (a type = one
histogram), so their patch distances take a handful of values shared by thousands of pairs, and the threshold -- a free float parameter -- is placed on
those values: on a value d itself and its float neighbours (the comparison at equality), and on the edges of the verified band around it,
RN(d / (1 -+ 2^-10)) and the floats within 2 ulp (the test that sends a pair to the exact re-evaluation).  Everything is closed-form or seeded.

A case carries hist, ns, b, w, its occupied bins and its threshold list; the reference distances (similarity_ref.distances32) are computed once per case
and shared read-only.  The families:
  plateau    checkerboard of two types (every pair of odd displacement ties: the borderline list overflows), a sparse plateau (one pixel in 23 of the
             second type: the list holds thousands of pairs and does not overflow), three types in stripes; `limits`: plateaus exactly on 2^-6 and 64,
             the ends of the range the binary16 planes serve
  half       a checkerboard with ONE cross term t per pixel pair, t found by a search so that binary16 rounds it down (or, the twin, up) by 0.9 .. 1
             times 2^-11: all nine entries of a patch err the same way, the worst case of the error analysis in k_similarity_fast.hip
  counts     bins with b1 + b2 exactly 1 (skipped) and next(1) (counted), patches without any counted bin (d = 0 / 0), fully occupied histograms
             (60 bins per pixel pair, 540 per patch) at the three depths the approximate kernel has
  guard      bins exactly 2^20 and counts exactly 2^-10 and 2^16 (inside the range where the scale-free division is proven exact), and each one ulp outside
  seams      the sparse plateau with the two types swapped beyond a column and a line, the column at the tile boundaries of the kernels (62, 64, 248
             columns per wavefront or tile); frame widths around them; frames lower than the search window
  geometry   w = 2, w = 0, b = 12, b = 3
  drawn      the sparse plateau with counts drawn per pixel, independently: the thresholds are the ties that remain
  large      1000 x 400 (the smallest frame that takes the four-column kernels) and 1001 x 400 (the narrow kernels at that size); periodic, so
             the reference is one period tiled (similarity_ref.periodic_distances32)
Every small case comes with n = 16 everywhere (the uniform kernel), n = 12 everywhere (rho = 1 through the RATIO form) and n from {8, 12, 16, 24} in a
seeded 2 x 2 tile with the histograms scaled by n / 16 (RATIO form; pairs of one type keep distance 0, the plateaus split into a few values each)."""
import numpy as np

import similarity_ref as sr

F = np.float32
DELTA = F(2.0 ** -10)
TAU_MIN, TAU_MAX = F(2.0 ** -6), F(64.0)     # thresholds the binary16 planes serve (BCD_APPROX_TAU_MIN / _MAX)
CAPACITY_FLOOR = 1 << 16                     # the borderline list holds max(npix, 2^16) pairs
SPARSE = 23


def capacity(W, H):
    return max(W * H, CAPACITY_FLOOR)


# ---- pixel types ---------------------------------------------------------------------------------------------------------
def _type(D, entries):
    h = np.zeros(D, F)
    per = D // 3
    for ch, bins in enumerate(entries):
        for k, v in bins.items():
            h[ch * per + k] = v
    return h


# channel 0: the same two bins, other weights; channel 1: a bin the first type lacks; channel 2: a bin with b1 + b2 == 1 against the first type
TYPE_A = _type(60, [{3: 10, 4: 6}, {7: 16}, {10: 4, 11: 4, 12: 4, 13: 4}])
TYPE_B = _type(60, [{3: 7, 4: 9}, {7: 11, 8: 5}, {10: 4, 11: 4, 12: 4, 13: 3, 14: 1}])
TYPE_C = _type(60, [{3: 12, 4: 4}, {7: 13, 9: 3}, {10: 6, 11: 2, 12: 4, 13: 4}])
PLATEAU_TYPES = np.stack([TYPE_A, TYPE_B, TYPE_C])


def full_types(D, seed=5):
    """two fully occupied histograms: every bin 1 .. 4, so b1 + b2 > 1 for every bin of every pair"""
    return np.random.default_rng(seed).integers(1, 5, (2, D)).astype(F)


# ---- type maps -----------------------------------------------------------------------------------------------------------
def _lc(W, H):
    return np.meshgrid(np.arange(H), np.arange(W), indexing="ij")


def checker(W, H):
    l, c = _lc(W, H)
    return (l + c) & 1


def sparse(W, H):
    l, c = _lc(W, H)
    return ((c + 7 * l) % SPARSE == 0).astype(np.int64)


def stripes3(W, H):
    l, c = _lc(W, H)
    return (c // 4) % 3


def seam(W, H, cb, lb):
    l, c = _lc(W, H)
    return sparse(W, H) ^ (c >= cb) ^ (l >= lb)


# ---- sample counts -------------------------------------------------------------------------------------------------------
VARIANTS = ("n16", "n12", "mixed")


def with_counts(base, variant, seed=0):
    """(hist, ns) of a frame of base histograms under one of the three sample-count variants"""
    H, W, D = base.shape
    if variant == "n16":
        ns = np.full((H, W, 1), 16, F)
        hist = base
    elif variant == "n12":
        ns = np.full((H, W, 1), 12, F)
        hist = base
    else:
        tile = np.random.default_rng(100 + seed).permutation(np.array([8, 12, 16, 24], F)).reshape(2, 2)
        l, c = _lc(W, H)
        ns = tile[l & 1, c & 1].astype(F)[:, :, None]
        hist = base * (ns / F(16))
    return np.ascontiguousarray(hist, F), np.ascontiguousarray(ns, F)


# ---- thresholds ----------------------------------------------------------------------------------------------------------
def ladder(d):
    """the 13 thresholds of a distance value: the value and its neighbours, both band edges and the floats within 2 ulp of them"""
    d = F(d)
    lo, hi = F(d / (F(1) - DELTA)), F(d / (F(1) + DELTA))
    return [d, sr.prev(d), sr.next_(d)] + [sr.ulps(lo, k) for k in (0, -1, 1, -2, 2)] + [sr.ulps(hi, k) for k in (0, -1, 1, -2, 2)]


def short_ladder(d):
    d = F(d)
    return [d, sr.prev(d), F(d / (F(1) - DELTA))]


def in_range(taus):
    out = []
    for t in taus:
        if TAU_MIN <= t <= TAU_MAX and not any(t == o for o in out):
            out.append(t)
    return out


def forward_distances(dist, b):
    """the distances of the forward pairs (each unordered pair of distinct main pixels once): offsets after the centre"""
    side = 2 * b + 1
    kc = (side * side - 1) // 2
    d = dist[:, :, kc + 1:]
    return d[np.isfinite(d)]


def plateau_values(dist, b, lo=TAU_MIN * 2, hi=TAU_MAX / 2):
    """(values, populations) of the non-zero distances inside (lo, hi), most populated first"""
    d = forward_distances(dist, b)
    d = d[(d > lo) & (d < hi)]
    v, n = np.unique(d, return_counts=True)
    order = np.argsort(-n, kind="stable")
    return v[order], n[order]


def in_band(dist, b, tau, width=1.0):
    """forward pairs strictly inside tau (1 +- width 2^-10)"""
    d = forward_distances(dist, b).astype(np.float64)
    t = float(tau)
    return int(np.count_nonzero((d > t * (1 - width * float(DELTA))) & (d < t * (1 + width * float(DELTA)))))


def ties(dist, b, tau):
    return int(np.count_nonzero(forward_distances(dist, b) == F(tau)))


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, hist, ns, b=6, w=1, nvalues=1, short=False, taus=None, pick=None, seam=None, marks=(), variant="n16",
                 make=None, period=None, size=None):
        self.name, self.family, self.b, self.w, self.variant = name, family, b, w, variant
        self.hist, self.ns = hist, ns
        self.make, self.period = make, period                         # large cases: the frame at any size, and its period
        self.H, self.W, self.D = (hist.shape if hist is not None else (size[1], size[0], 60))
        self.nvalues, self.short, self.pick, self._taus = nvalues, short, pick, taus
        self.seam, self.marks = seam, tuple(marks)                    # (seam column, seam line); pixels whose distances the GPU test reads
        self._dist = self._bins = self._values = None
        self.large = make is not None
        self.extra = []

    @property
    def bins(self):
        if self._bins is None:
            self._bins = sr.occupied_bins(self.hist if not self.large else self.make(2 * SPARSE, 2 * SPARSE)[0])
        return self._bins

    @property
    def dist(self):
        """reference distances, computed once and read-only; a large case holds ONE PERIOD of them"""
        if self._dist is None:
            if self.large:
                d = sr.periodic_distances32(self.make, self.period, self.W, self.H, self.b, self.w, self.bins)
            else:
                d = sr.distances32(self.hist, self.ns, self.b, self.w, self.bins)
            d.setflags(write=False)
            self._dist = d
        return self._dist

    @property
    def values(self):
        """the plateau values the ladders stand on"""
        if self._values is None:
            v, n = plateau_values(self.dist, self.b)
            if self.pick is not None:
                keep = [i for i in range(len(v)) if self.pick(self, v[i], n[i])]
                v, n = v[keep], n[keep]
            self._values = [F(x) for x in v[:self.nvalues]]
        return self._values

    @property
    def taus(self):
        if self._taus is None:
            out = []
            for d in self.values:
                out += short_ladder(d) if self.short else ladder(d)
            self._taus = in_range(out)
            for t in self.extra:                                      # (thresholds that are not bound to the binary16 range)
                if not any(t == o for o in self._taus):
                    self._taus.append(t)
        return self._taus

    def frame(self):
        """(hist, ns) -- a large case builds its arrays on demand (96 MB)"""
        return self.make(self.W, self.H) if self.large else (self.hist, self.ns)

    def reference(self, tau):
        if self.large:
            if getattr(self, "_valid", None) is None:
                self._valid = sr.window_valid(self.W, self.H, self.w, self.b)
            return sr.tile_masks(self.dist, self._valid, tau)
        return sr.masks_from(self.dist, tau)

    def __repr__(self):
        return self.name


def _below_half_capacity(case, v, n):
    """a value whose band holds more than 1 000 pairs and fewer than half the list's capacity"""
    return n >= 1000 and in_band(case.dist, case.b, v) < capacity(case.W, case.H) // 2


def _small(name, family, tmap, types=PLATEAU_TYPES, **kw):
    """the three sample-count variants of a frame of types"""
    out = []
    for variant in VARIANTS:
        hist, ns = with_counts(types[tmap], variant, seed=len(name))   # (the tile's permutation: any fixed number per frame)
        nv = kw.get("nvalues", 1)
        out.append(Case("%s %s" % (name, variant), family, hist, ns, variant=variant, **dict(kw, nvalues=nv if variant != "mixed" else max(nv, 4))))
    return out


def search_half_rounding(direction, y=F(8), start=F(12.5), span=1 << 20):
    """float32 x such that t = RN(RN((x - y)^2) / (x + y)) loses (direction -1) or gains (+1) at least 0.9 * 2^-11 of its value when rounded to binary16:
    t just below (above) the midpoint of two binary16 numbers next to a power of two.  Deterministic: the first hit after `start`"""
    x = F(start) + np.arange(span, dtype=np.float64) * float(np.spacing(F(start)))
    x = x.astype(F)
    diff = x - y
    t = (diff * diff) / (x + y)
    rel = sr.half(t).astype(np.float64) / t.astype(np.float64) - 1.0
    hit = np.flatnonzero(rel <= -0.9 * 2.0 ** -11) if direction < 0 else np.flatnonzero(rel >= 0.9 * 2.0 ** -11)
    assert hit.size, "no float in the searched span rounds that far"
    return x[hit[0]], F(y), t[hit[0]], rel[hit[0]]


def half_types(direction):
    x, y, t, rel = search_half_rounding(direction)
    return np.stack([_type(60, [{5: x}, {}, {}]), _type(60, [{5: y}, {}, {}])]), t, rel


HALF_OFFSETS = (0.25, 0.5, 0.9, 0.99, 1.01)      # d_ref at these multiples of 2^-10 from tau, on either side


def _half_cases():
    out = []
    for direction, word in ((-1, "down"), (1, "up")):
        types, t, rel = half_types(direction)
        for c in _small("half rounds %s 40x24" % word, "half", checker(40, 24), types=types):
            if c.variant == "n16":                                    # (the search is for the uniform kernel's term; the other variants run the ladder alone)
                d = c.values[0]
                extra = [F(d / F(1 + s * f * float(DELTA))) for f in HALF_OFFSETS for s in (1, -1)]
                c._taus = in_range(ladder(d) + extra)
                c.half_rel = rel
            out.append(c)
    return out


def _counts_cases():
    out = []
    # bins summing to exactly 1 (0.75 + 0.25: skipped) and to next(1) (0.75 + next-but-one(0.25) = 1 + 2^-23: counted), beside the plateau types' bins
    e = np.stack([TYPE_A.copy(), TYPE_B.copy(), TYPE_A.copy(), np.zeros(60, F)])
    e[0, 40] = e[2, 40] = 0.75
    e[1, 40] = 0.25
    e[2, 41] = 0.75
    e[1, 41] = F(0.25) + F(2.0 ** -23)
    e[3, 0] = 0.5                                                     # the empty type: no bin of it counts against itself (0.5 + 0.5 == 1)
    W, H = 48, 32
    tmap = sparse(W, H) * 1
    tmap[:, W // 2:] = np.where(tmap[:, W // 2:] == 0, 2, 1)          # right half: type 2 (its bin 41 reaches next(1) against type 1)
    tmap[6:26, 4:22] = 3                                              # a block of empty pixels wider than a search window
    out += _small("counts edge and empty 48x32", "counts", tmap, types=e, nvalues=2)
    for D in (60, 36, 24):
        out += _small("counts full D=%d 40x24" % D, "counts", sparse(40, 24), types=full_types(D))
    return out


def guard_frame(kind):
    """a sparse plateau with four guard pixels: bins of exactly 2^20 (two pixels, 512 apart in that bin), sample counts of exactly 2^-10 and 2^16; `kind`
    moves one of them one ulp outside.  -> hist, ns, the guard pixels"""
    W, H = 48, 24
    hist, ns = with_counts(PLATEAU_TYPES[sparse(W, H)], "n16")
    ns = ns.copy()
    ns[:] = 65536 if kind in ("uni", "out bin uni") else 16           # `uni`: every count 2^16, the largest the uniform kernel takes
    pix = [(8, 10), (8, 14), (14, 20), (15, 30)]
    top = F(2.0 ** 20)
    hist[8, 10, 59], hist[8, 14, 59] = top, top - F(512)
    if kind not in ("uni", "out bin uni"):
        ns[14, 20, 0], ns[15, 30, 0] = F(2.0 ** -10), F(2.0 ** 16)
    if kind.startswith("out bin"):
        hist[8, 10, 59] = sr.next_(top)
    elif kind == "out n low":
        ns[14, 20, 0] = sr.prev(F(2.0 ** -10))
    elif kind == "out n high":
        ns[15, 30, 0] = sr.next_(F(2.0 ** 16))
    return hist, ns, pix


GUARD_KINDS = ("uni", "mixed", "out bin uni", "out bin", "out n low", "out n high")


GUARD_OFFSETS = ((0, 4), (0, 1), (1, 0))


def guard_thresholds(case):
    """d, prev(d), next(d) of the distances from every guard pixel to three neighbours ((0, 4) joins the two pixels with bins of 2^20 and 2^20 - 512):
    distances whose terms divide by sums of 2^21 and by count products of 2^-20 .. 2^32, decided at equality -- the scale-free division of the exact
    kernels is held bit for bit where its range ends.  Most lie above 64 (a count of 2^16 beside counts of 16): no range filter"""
    side = 2 * case.b + 1
    out = []
    for (l, c) in case.marks:
        for (dl, dc) in GUARD_OFFSETS:
            d = case.dist[l, c, (dl + case.b) * side + (dc + case.b)]
            if np.isfinite(d) and d > 0:
                out += [F(d), sr.prev(d), sr.next_(d)]
    return out


def _guard_cases():
    out = []
    for kind in GUARD_KINDS:
        hist, ns, pix = guard_frame(kind)
        c = Case("guard %s 48x24" % kind, "guard", hist, ns, nvalues=2, marks=pix, variant="n16" if "uni" in kind else "mixed")
        c.inside = not kind.startswith("out")
        c.extra = guard_thresholds(c)
        out.append(c)
    return out


def limit_types():
    """d(A, B) = 2^-6 and d(A, C) = 64 exactly on checkerboards: per pixel pair two counted bins, terms (1/32, 0) and (0, 128), nine equal entries"""
    A = _type(60, [{2: 16.5}, {6: 128}, {}])
    B = _type(60, [{2: 15.5}, {6: 128}, {}])
    Cc = _type(60, [{2: 16.5}, {6: 0}, {}])
    return np.stack([A, B, Cc])


def _limit_case():
    W, H = 64, 40
    tmap = checker(W, H)
    tmap[:, W // 2:] *= 2                                             # left half A / B, right half A / C
    hist, ns = with_counts(limit_types()[tmap], "n16")
    taus = [TAU_MIN, sr.prev(TAU_MIN), sr.next_(TAU_MIN), TAU_MAX, sr.next_(TAU_MAX), sr.prev(TAU_MAX)]
    return Case("limits 2^-6 and 64 64x40", "limits", hist, ns, taus=taus)


SEAM_COLUMNS = (61, 62, 63, 64, 124, 248)
WIDTHS = (62, 63, 64, 65, 125, 249)
HEIGHTS = (3, 4, 5, 7)


def _seam_cases():
    out = []
    for i, cb in enumerate(SEAM_COLUMNS):
        lb = (3, 4)[i & 1]
        out += _small("seam column %d line %d 256x16" % (cb, lb), "seams", seam(256, 16, cb, lb), seam=(cb, lb))
    for i, W in enumerate(WIDTHS):
        H = 40 if W < 100 else 20                                     # (enough pairs for a thousand ties per value under mixed counts)
        out += _small("width %d x%d" % (W, H), "seams", seam(W, H, W // 2, (3, 4)[i & 1]), seam=(W // 2, (3, 4)[i & 1]))
    for H in HEIGHTS:
        out += _small("height %d 400 wide" % H, "seams", checker(400, H))
    return out


def _drawn_case():
    """sample counts drawn per pixel (seeded, independent) from {8, 12, 16, 24}, histograms in proportion: every pair of counts meets at every displacement
    through the RATIO form.  The plateaus scatter into hundreds of values; the thresholds are the ties that remain: d, prev(d), next(d) of the eight most
    populated values (no thousand pairs per value here: tests/test_similarity_cases_cpu.py exempts this family from that claim)"""
    W, H = 64, 40
    rng = np.random.default_rng(2024)
    ns = rng.choice(np.array([8, 12, 16, 24], F), size=(H, W, 1)).astype(F)
    hist = np.ascontiguousarray(PLATEAU_TYPES[sparse(W, H)] * (ns / F(16)), F)
    c = Case("drawn counts sparse 64x40", "drawn", hist, ns, variant="mixed", taus=[])
    v, n = plateau_values(c.dist, c.b)
    c.drawn = list(zip(v[:8], n[:8]))
    c._taus = in_range([t for d in v[:8] for t in (F(d), sr.prev(d), sr.next_(d))])
    return c


def _geometry_cases():
    out = []
    for (w, b) in ((2, 6), (0, 4), (1, 12), (1, 3)):
        W = 160 if w == 0 else 64                                     # (w = 0: a pair is one pixel pair, few of them tie)
        out += _small("geometry w=%d b=%d %dx40" % (w, b, W), "geometry", sparse(W, 40), w=w, b=b, short=True)
    return out


def _large_cases():
    out = []
    for W in (1000, 1001):
        for b in (6, 3):
            for pattern, types in (("sparse", PLATEAU_TYPES), ("full", full_types(60))):
                make = (lambda W_, H_, types=types: with_counts(types[sparse(W_, H_)], "n16"))
                out.append(Case("large %s %dx400 b=%d" % (pattern, W, b), "large", None, None, b=b, short=True, make=make, period=(SPARSE, SPARSE), size=(W, 400)))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        out = []
        out += _small("plateau checker 64x40", "plateau", checker(64, 40))
        out += _small("plateau sparse 64x40", "plateau", sparse(64, 40), pick=_below_half_capacity)
        out += _small("plateau stripes 64x40", "plateau", stripes3(64, 40), nvalues=3)
        out.append(_limit_case())
        out += [_drawn_case()] + _half_cases() + _counts_cases() + _guard_cases() + _seam_cases() + _geometry_cases() + _large_cases()
        names = [c.name for c in out]
        assert len(set(names)) == len(names), "case names are ids"
        _cases = out
    return _cases


def small_cases():
    return [c for c in cases() if not c.large]


def large_cases():
    return [c for c in cases() if c.large]


def by_name(name):
    return next(c for c in cases() if c.name == name)


def names(family=None, large=None):
    return [c.name for c in cases() if (family is None or c.family == family) and (large is None or c.large == large)]
