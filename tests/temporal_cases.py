"""Seeded pairs of histogram frames for the cross-frame selection tests (tests/test_gpu_temporal_stage.py, tests/test_temporal_cases_cpu.py).  TEST
INFRASTRUCTURE.

A frame is one noisy realisation of a fixed smooth scene: per pixel and channel, n samples around the scene's value are binned into D / 3 bins (integer bin
values, like an accumulator fed unit weights).  Two frames of one scene with different seeds are what neighbouring frames of an animation look like to the
selection: the same surfaces under independent noise.  The sample counts are one power of two, 24 everywhere, drawn per pixel (and differently in the two
frames), or 1 -- a 1-spp frame has one bin of 1 per channel, so b1 + b2 > 1 only where the neighbour hit the same bin, and patch pairs without such a bin have
distance 0 / 0 = NaN.

A case carries the two frames, the geometry and its thresholds: distance values taken from the reference (temporal_ref.cross_distances32) and their two
float neighbours, so that the threshold sits ON distances (ties included).  The reference distances are computed once per case and shared read-only."""
import numpy as np

import similarity_ref as sr
import temporal_ref as tr

F = np.float32
MIXED = np.array([8, 12, 16, 24, 32], F)


def counts(W, H, kind, seed):
    if kind == "mixed":
        return np.random.default_rng(1000 + seed).choice(MIXED, (H, W, 1)).astype(F)
    return np.full((H, W, 1), F(kind), F)


def frame(W, H, D, kind, seed):
    """(hist (H, W, D), ns (H, W, 1)) float32: realisation `seed` of the scene with sample counts `kind` (a number, or "mixed")"""
    per = D // 3
    ns = counts(W, H, kind, seed)
    nmax = int(ns.max())
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([0.25 + 0.5 * c / max(W - 1, 1), 0.5 + 0.3 * np.sin(0.7 * l), np.where((l // 5 + c // 7) % 2, 0.7, 0.3)], -1)      # (H, W, 3)
    rng = np.random.default_rng(seed)
    val = base[:, :, :, None] + 0.12 * rng.standard_normal((H, W, 3, nmax))
    idx = np.clip((val * per).astype(np.int64), 0, per - 1)
    live = np.arange(nmax)[None, None, None, :] < ns[:, :, :, None].astype(np.int64)
    hist = np.zeros((H, W, D), F)
    for ch in range(3):
        for k in range(per):
            hist[:, :, ch * per + k] = ((idx[:, :, ch, :] == k) & live[:, :, 0, :]).sum(-1)
    return hist, ns


class Case:
    def __init__(self, name, W, H, D=60, b=6, w=1, kinds=(16, 16), seeds=(1, 2)):
        self.name, self.W, self.H, self.D, self.b, self.w, self.kinds, self.seeds = name, W, H, D, b, w, kinds, seeds
        self._frames = self._dist = None

    @property
    def frames(self):
        """(hist, ns, hist_nb, ns_nb)"""
        if self._frames is None:
            a = frame(self.W, self.H, self.D, self.kinds[0], self.seeds[0])
            nb = a if self.seeds[1] == self.seeds[0] and self.kinds[1] == self.kinds[0] else frame(self.W, self.H, self.D, self.kinds[1], self.seeds[1])
            for x in a + nb:
                x.setflags(write=False)
            self._frames = a + nb
        return self._frames

    @property
    def dist(self):
        if self._dist is None:
            d = tr.cross_distances32(*self.frames, self.b, self.w)
            d.setflags(write=False)
            self._dist = d
        return self._dist

    @property
    def taus(self):
        """three distance values of the case (the most populated positive one and two quantiles), each with its two float neighbours, and 0"""
        d = self.dist[np.isfinite(self.dist)]
        pos = d[d > 0]
        out = [F(0)]
        if len(pos):
            v, n = np.unique(pos, return_counts=True)
            for x in (v[np.argmax(n)], np.quantile(pos, 0.25, method="nearest"), np.quantile(pos, 0.6, method="nearest")):
                for t in (F(x), sr.prev(x), sr.next_(x)):
                    if not any(t == o for o in out):
                        out.append(t)
        return out

    def reference(self, tau):
        return sr.masks_from(self.dist, tau)

    def marks(self):
        """pixels whose window distances are read: the corners of the main area and its middle"""
        w, W, H = self.w, self.W, self.H
        return sorted({(w, w), (w, W - 1 - w), (H - 1 - w, w), (H - 1 - w, W - 1 - w), (H // 2, W // 2)})


def _cases():
    out = [Case("%dx%d" % (W, H), W, H) for (W, H) in ((20, 16), (33, 21), (5, 40), (70, 10))]          # (70 columns: two tiles of the distance kernel)
    out += [Case("33x21 b=%d" % b, 33, 21, b=b) for b in (3, 12)]
    out += [Case("33x21 b=3 w=%d" % w, 33, 21, b=3, w=w) for w in (0, 2)]
    out += [Case("20x16 D=%d" % D, 20, 16, D=D) for D in (24, 15)]
    out += [Case("20x16 24 spp", 20, 16, kinds=(24, 24)), Case("20x16 mixed counts", 20, 16, kinds=("mixed", "mixed")),
            Case("20x16 16 spp against mixed", 20, 16, kinds=(16, "mixed")), Case("20x16 24 spp against 1 spp", 20, 16, kinds=(24, 1)),
            Case("20x16 1 spp against 1 spp", 20, 16, kinds=(1, 1)),          # (every distance is 0 or NaN: one threshold)
            Case("20x16 b=3 w=0 2 spp against 1 spp", 20, 16, b=3, w=0, kinds=(2, 1))]       # (one-pixel patches: NaN beside positive distances)
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]


def by_name(name):
    return CASES[NAMES.index(name)]
