"""Constructed sample streams for the accumulator's histogram binning (tests/test_gpu_accum_binning.py, tests/test_accum_cases_cpu.py).
TEST INFRASTRUCTURE.

The binning of one colour channel (SamplesAccumulator::addSample; acc_bin in k_accumulate.hip and its copy in k_accumulate_samples):
    v = max(x, 0); if gamma > 1: v = powf(v, 1.f / gamma); if max_value > 0: v = v / max_value; v = min(v, 2)
    fi = v * (nbins - 2); lo = int(fi)
    lo < nbins - 2:  bins lo, lo + 1 get w * (1 - (fi - lo)), w * (fi - lo)                  (the linear branch)
    else:            bins nbins - 2, nbins - 1 get w * (1 - (v - 1)), w * (v - 1)            (the saturation branch)
Random radiance puts no value on a bin edge, on v = 1 or on the clamp.  These streams do.  A case is
    (W, H, nbins, gamma, max_value, samples [N, k, 3] float32, weights [N, k] float32 or None, name),
pixel p = line * W + col, its k samples in accumulation order.  Families:
  edges      for every j in 0 .. 2 (nbins - 2) the colour whose transformed value is j / (nbins - 2) -- found in float64 by inverting the
             normalisation and the gamma curve (with the fp32 exponent 1.f / gamma), rounded to fp32 -- with its two fp32 neighbours and the
             colour of (j + 0.5) / (nbins - 2), the middle of the bin above the edge (so that every bin is a lower bin whatever powf rounds
             to).  j <= nbins - 2 are the edges of the linear branch, j = nbins - 2 the entry into saturation, j = 2 (nbins - 2) the clamp.
             The three channels of a sample carry different j.
  specials   0, -0, -1, NaN, +inf, -inf, 1e-40, FLT_MIN, FLT_MAX, the colours of v = 1 and v = 2, the float above the latter and 1.5 times it:
             alone in a pixel (every sample, every channel), one per channel, and one among ordinary samples.
  onehot     gamma = 1, max_value = 0, nbins - 2 a power of two: pixel p's one unit-weight sample is the colour b / (nbins - 2) with
             b = (p + 7 c) mod (nbins - 1) in channel c; every operation is exact, the histogram is 1 in bin b of channel c and 0 elsewhere.
  weights    k = 9 samples per pixel (one dense pass of it is LDS-staged) from five neighbouring entries of the edges list, so that
             samples share bins, with weights 0, 2^-20, 0.5, 1, 3 and 2^20 mixed within a pixel: the order of the fp32 additions matters.
Parameter sets (PARAMS): the default, an odd depth, the smallest depths, the accumulator's largest, and each way of skipping powf and the
division.  ONE_SHOT_PARAMS: 86 bins (the first to need more than 64 KiB of dynamic LDS) and 213 (the most the CU's LDS holds), which only
bcd_hip_accumulate_samples accepts, on a 9 x 7 frame with 2 samples per pixel: 126 slots per channel for 340 and 848 entries, so these two
SAMPLE the edges list (every 7th and 15th entry, all four kinds among them) and do not cover every edge or bin.

2 bins.  With nbins = 2 the factor nbins - 2 is 0: fi = 0, lo = 0 is not < 0, so every value takes the saturation branch with lo = 0 and
the weights 2 - v and v - 1 go to bins 0 and 1 -- in bounds (with 1 bin lo + 1 would not be).  Both entry points accept 2; the cases
include it.  Its "edges" are v = 0, 1, 2.

"v * (nbins - 2) rounds up to nbins - 2 while v < 1" has no case, because it cannot happen in fp32.  Let m = nbins - 2 with
2^e <= m < 2^(e+1).  v < 1 means v <= 1 - 2^-24, so the exact product is at least m 2^-24 >= 2^(e-24) below m.  For m > 2^e the floats
below m are 2^(e-23) apart: the product is at least half a spacing away from m and at most half a spacing from the float below it
(m 2^-24 < 2^(e-23)), and the only tie, m 2^-24 = 2^(e-24), needs m = 2^e.  For m = 2^e the floats below m are 2^(e-24) apart and
m - m 2^-24 is one of them.  So fl(v m) < m, and the switch into saturation happens at v = 1 exactly; the edges family has v = 1 and the
floats around it, and the CPU test checks fl(prev(1) m) < m for every m in use.  What does happen is the same at an inner edge:
fl(v m) = j although v < j / m, because j / m is no float.  rounding_up_examples() finds such colours in the edges family of a parameter
set where v is computable without powf."""
import collections
import math

import numpy as np

F32 = np.float32
F64 = np.float64

Case = collections.namedtuple("Case", "W H nbins gamma maxval samples weights name")

PARAMS = [(20, 2.2, 2.5), (21, 2.2, 2.5), (3, 2.2, 2.5), (85, 3.0, 0.7), (10, 1.0, 0.0), (18, 1.0, 1.0), (20, 0.5, 2.5), (20, 2.2, -1.0),
          (2, 2.2, 2.5), (2, 1.0, 1.0)]
DEFAULT = PARAMS[0]
ONE_SHOT_PARAMS = [(86, 2.2, 2.5), (213, 2.2, 2.5)]
ACCUM_MAX_BINS = 85                                # bcd_hip_accum_create; bcd_hip_accumulate_samples goes to 213
STAGE_SPP = 8                                      # dense passes of at least this many samples per pixel take the LDS-staged kernel
WEIGHT_SET = np.array([0.0, 2.0 ** -20, 0.5, 1.0, 3.0, 2.0 ** 20], F32)
FRAME = (19, 13)                                   # 247 pixels: three full wavefronts and one of 55

# U of the per-bin bound (accum_ref.bound_terms).  U_REF: the smallest U for which the host arithmetic with the C library's powf obeys the
# bound on every case (measured by test_accum_cases_cpu.py::test_oracle_obeys_the_bound_with_u_ref: 1.6794, at specials-86-2.2-2.5;
# 1.57 at 85 bins, 1.20 at the default parameters).  The device's powf is another implementation that is allowed a few ulps: it gets
# four times that.
U_REF = 1.68
U_DEVICE = int(math.ceil(4 * U_REF))


def scale(nbins):
    """the bin positions of the edges are j / scale, j = 0 .. 2 scale (2 bins: v = 0, 1, 2)"""
    return max(nbins - 2, 1)


def exponent(gamma):
    """the exponent the code applies: 1.f / gamma evaluated in fp32"""
    return F64(F32(1) / F32(gamma))


def transform(x, gamma, maxval):
    """float64 transformed value of colours x (any shape): the definition with the fp32 exponent, everything else exact"""
    x = np.asarray(x, F64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(x > 0, x, 0.0)
        if gamma > 1:
            v = np.power(v, exponent(gamma))
        if maxval > 0:
            v = v / F64(F32(maxval))
        return np.minimum(v, 2.0)


def colour_of(v, gamma, maxval):
    """float64 colour whose transformed value is v"""
    x = F64(v) * (F64(F32(maxval)) if maxval > 0 else 1.0)
    if gamma > 1:
        x = x ** (1.0 / exponent(gamma))
    return x


def edge_list(nbins, gamma, maxval):
    """-> (colours [4 G] float32, j [4 G], kind [4 G]) for G = 2 scale + 1 edges; kind 0: the float below the edge colour, 1: the edge
    colour, 2: the float above, 3: the middle of the bin above the edge"""
    m = scale(nbins)
    cols, js, kinds = [], [], []
    for j in range(2 * m + 1):
        x = F32(colour_of(j / m, gamma, maxval))
        for kind, c in enumerate((np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf)), F32(colour_of((j + 0.5) / m, gamma, maxval)))):
            cols.append(c)
            js.append(j)
            kinds.append(kind)
    return np.array(cols, F32), np.array(js), np.array(kinds)


def _channel_offset(nbins):
    """entries of the edges list between the channels of one sample: a third of the edges, so the three j differ"""
    return 4 * max(1, (2 * scale(nbins) + 1) // 3)


def edges(prm, W=FRAME[0], H=FRAME[1], k=3, tag="edges"):
    nbins, gamma, maxval = prm
    L, _, _ = edge_list(nbins, gamma, maxval)
    N, n = W * H, L.size
    step = max(1, -(-n // (N * k))) | 1            # a frame with fewer slots than entries takes every step-th one; odd, so that all four
                                                   # kinds of entry (below, on and above an edge, middle of a bin) keep turning up
    slot = (np.arange(N * k).reshape(N, k, 1) * step + np.arange(3).reshape(1, 1, 3) * _channel_offset(nbins)) % n
    return Case(W, H, nbins, gamma, maxval, np.ascontiguousarray(L[slot]), None, "%s-%d-%g-%g" % (tag, nbins, gamma, maxval))


def special_values(gamma, maxval):
    with np.errstate(over="ignore"):
        x1, x2 = F32(colour_of(1.0, gamma, maxval)), F32(colour_of(2.0, gamma, maxval))
        return np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-40, np.finfo(F32).tiny, np.finfo(F32).max, x1, x2,
                         np.nextafter(x2, F32(np.inf)), F32(1.5) * x2], F32)


def ordinary(rng, shape, gamma, maxval):
    """colours whose transformed values are uniform in [0, 1.2)"""
    v = rng.random(shape) * 1.2
    x = v * (F64(F32(maxval)) if maxval > 0 else 1.0)
    if gamma > 1:
        x = x ** (1.0 / exponent(gamma))
    return x.astype(F32)


def specials(prm, W=FRAME[0], H=FRAME[1], k=3, tag="specials"):
    nbins, gamma, maxval = prm
    S = special_values(gamma, maxval)
    N, n = W * H, S.size
    assert N >= 3 * n and k >= 2
    smp = ordinary(np.random.default_rng(nbins), (N, k, 3), gamma, maxval)
    for p in range(N):
        if p < n:
            smp[p] = S[p]                                            # alone: every sample, every channel
        elif p < 2 * n:
            smp[p] = S[(p + 4 * np.arange(3)) % n]                   # one per channel
        else:
            smp[p, 1, p % 3] = S[p % n]                              # one among ordinary samples
    return Case(W, H, nbins, gamma, maxval, smp, None, "%s-%d-%g-%g" % (tag, nbins, gamma, maxval))


def onehot(nbins, W=13, H=9):
    """-> (case, expected histogram [N, 3 nbins])"""
    m = nbins - 2
    assert m & (m - 1) == 0 and W * H > 3 * nbins and (W * H) % 64
    N = W * H
    b = (np.arange(N).reshape(N, 1) + 7 * np.arange(3).reshape(1, 3)) % (nbins - 1)
    smp = (b.astype(F64) / m).astype(F32).reshape(N, 1, 3)
    want = np.zeros((N, 3, nbins), F32)
    np.put_along_axis(want, b[:, :, None], F32(1), axis=2)
    return Case(W, H, nbins, 1.0, 0.0, smp, None, "onehot-%d" % nbins), want.reshape(N, 3 * nbins)


def weights(prm, W=FRAME[0], H=FRAME[1]):
    nbins, gamma, maxval = prm
    L, _, _ = edge_list(nbins, gamma, maxval)
    N, k, G = W * H, 9, 2 * scale(nbins) + 1
    p, s, c = np.arange(N).reshape(N, 1, 1), np.arange(k).reshape(1, k, 1), np.arange(3).reshape(1, 1, 3)
    slot = (4 * ((p + c * max(1, G // 3)) % G) + s % 5) % L.size     # the four entries of an edge and the float below the next edge
    w = np.random.default_rng(1000 + nbins).choice(WEIGHT_SET, (N, k))
    return Case(W, H, nbins, gamma, maxval, np.ascontiguousarray(L[slot]), np.ascontiguousarray(w), "weights-%d-%g-%g" % (nbins, gamma, maxval))


WEIGHT_PARAMS = [DEFAULT, (85, 3.0, 0.7), (18, 1.0, 1.0), (2, 2.2, 2.5)]
ONEHOT_BINS = [10, 18, 34]


def _build():
    cases, exact = collections.OrderedDict(), {}
    for prm in PARAMS:
        for c in (edges(prm), specials(prm)):
            cases[c.name] = c
    for prm in WEIGHT_PARAMS:
        c = weights(prm)
        cases[c.name] = c
    for nb in ONEHOT_BINS:
        c, want = onehot(nb)
        cases[c.name], exact[c.name] = c, want
    c = edges(DEFAULT, 7, 5, 5, tag="edges7x5")                      # fewer pixels than a wavefront
    cases[c.name] = c
    c = edges(DEFAULT, 1, 1, 9, tag="edges1x1")                      # one pixel; 9 samples, so a dense pass of it is staged
    cases[c.name] = c
    for prm in ONE_SHOT_PARAMS:
        for c in (edges(prm, 9, 7, 2), specials(prm, 9, 7, 2)):
            cases[c.name] = c
    return cases, exact


CASES, ONEHOT_EXPECTED = _build()
ALL = list(CASES)
ACCUM = [n for n in ALL if CASES[n].nbins <= ACCUM_MAX_BINS]          # cases the persistent accumulator accepts
SPLAT = ["edges-20-2.2-2.5", "specials-20-2.2-2.5", "edges-18-1-1"]  # through the splatted add: the default parameters, and one set without powf


def get(name):
    return CASES[name]


def stream(case):
    """(N k, 6) float32 addSample stream (line, col, r, g, b, w): pixels in order, each pixel's samples in order"""
    N, k = case.samples.shape[:2]
    p = np.repeat(np.arange(N), k)
    w = np.ones(N * k, F32) if case.weights is None else case.weights.reshape(-1)
    return np.ascontiguousarray(np.concatenate([(p // case.W)[:, None], (p % case.W)[:, None], case.samples.reshape(-1, 3), w[:, None]], 1).astype(F32))


def rounding_up_examples(prm):
    """colours of the edges list of a parameter set WITHOUT powf whose fp32 product v * (nbins - 2) is the integer j although v < j / (nbins - 2)
    exactly: -> [(colour, v, j)].  v = x / max_value is one IEEE division, so NumPy's fp32 gives the bits of any implementation."""
    nbins, gamma, maxval = prm
    assert not gamma > 1
    L, js, _ = edge_list(nbins, gamma, maxval)
    out = []
    for x, j in zip(L, js):
        if not x > 0 or j > nbins - 2:
            continue
        v = F32(x) / F32(maxval) if maxval > 0 else F32(x)
        fi = F32(v * F32(nbins - 2))
        if fi == F32(j) and F64(v) * (nbins - 2) < j:
            out.append((float(x), float(v), int(j)))
    return out
