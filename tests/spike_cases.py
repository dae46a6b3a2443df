"""The frames of the source-map tests (tests/test_spike_cases_cpu.py holds them to what they claim, tests/test_gpu_spike_layers.py runs them on the
device).  A case is (colours, sample counts, histograms, covariances, factor); the named frames come from oracle_lib.synth_inputs, the others are
constructed.  Moved share and chain count at factor 2, as measured on the CPU with the oracle:

    W x H    spp  sigma  spikes   moved   chains
    40x28    16   0.35   0.01     8.3 %   0
    72x50     8   0.15   0.01     8.0 %   0
    96x64    32   0.35   0        3.5 %   1      <- the one case where an in-place gather would go wrong
    31x17     4   0.35   0.05    10.2 %   0
    3x3       8   0.35   0.05    11.1 %   0
    67x3      8   0.35   0.02     8.5 %   0
    3x70      8   0.35   0.02    11.9 %   0
    65x5, 130x9: a last strip of one and of two columns behind one and two full 64-pixel strips"""
import numpy as np

import oracle_lib as ol

FACTOR = 2.0

# name -> (W, H, spp, sigma, spike probability)
NAMED = {
    "40x28": (40, 28, 16, 0.35, 0.01),
    "72x50": (72, 50, 8, 0.15, 0.01),
    "96x64": (96, 64, 32, 0.35, 0.0),
    "31x17": (31, 17, 4, 0.35, 0.05),
    "3x3": (3, 3, 8, 0.35, 0.05),
    "67x3": (67, 3, 8, 0.35, 0.02),
    "3x70": (3, 70, 8, 0.35, 0.02),
    "65x5": (65, 5, 8, 0.35, 0.02),
    "130x9": (130, 9, 8, 0.35, 0.02),
}
CONSTRUCTED = ("nonfinite", "constant", "all_spikes")
FINITE = tuple(NAMED) + ("constant", "all_spikes")
ALL = tuple(NAMED) + CONSTRUCTED

_cache = {}


def _synth(W, H, spp, sigma, s):
    col, ns, hist, cov = ol.synth_inputs(W, H, spp, sigma=sigma, spike_prob=s)[:4]
    return col, ns, hist, cov


def _nonfinite():
    """NaN, +inf, -inf and negative colours in a handful of windows, the four corners and all four borders included"""
    col, ns, hist, cov = (a.copy() for a in _synth(37, 21, 8, 0.35, 0.02))
    H, W, _ = col.shape
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    col[0, 0, 0] = nan
    col[0, W - 1, 1] = inf
    col[H - 1, 0, 2] = -inf
    col[H - 1, W - 1, :] = -3.0
    col[0, 11, 1] = nan          # borders
    col[H - 1, 20, 0] = inf
    col[9, 0, 2] = -inf
    col[12, W - 1, 0] = -7.5
    col[5, 5, :] = nan           # interior windows
    col[10, 17, 0] = inf
    col[10, 18, 0] = -inf        # inf and -inf in one window: the mean is NaN
    col[15, 30, 1] = -2.0
    col[16, 8, 2] = np.float32(-0.0)
    return col, ns, hist, cov


def _constant():
    """every colour the same: standard deviation 0, no value further than 0 from the mean, nothing is a spike"""
    col, ns, hist, cov = (a.copy() for a in _synth(33, 9, 4, 0.35, 0.0))
    col[...] = np.float32(0.375)
    return col, ns, hist, cov


def get(name):
    """(colours, sample counts, histograms, covariances, factor)"""
    if name not in _cache:
        if name in NAMED:
            _cache[name] = _synth(*NAMED[name]) + (FACTOR,)
        elif name == "nonfinite":
            _cache[name] = _nonfinite() + (FACTOR,)
        elif name == "constant":
            _cache[name] = _constant() + (FACTOR,)
        elif name == "all_spikes":
            # factor 0: a pixel is a spike as soon as one channel differs from its window's mean, which on a noisy frame is every pixel (checked on
            # the CPU); at the factors a renderer uses no frame makes every pixel the outlier of its own window
            _cache[name] = _synth(66, 7, 4, 0.35, 0.05) + (0.0,)
        else:
            raise KeyError(name)
    return _cache[name]
