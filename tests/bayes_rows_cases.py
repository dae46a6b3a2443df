"""Row bands of the constructed estimate cases (test infrastructure only): tests/bayes_cases.py frames handed to bcd_hip_bayes_accumulate_rows.

A band is a range of lines [r0, r1) of a case; banded(case, r0, r1) is the case whose state image is zero outside those lines -- what the entry
point must compute when it is given the FULL state image and the row range: the items of the owned lines, with everything they write up to b + w
lines beyond either edge.  CUTS holds the cut lists (r_0, r_1, ..., r_n: the bands are [r_i, r_i+1)) per frame, chosen so that over the lists
  * a boundary falls inside a 16-line tile of the fallback kernel and one on a multiple of 16;
  * a band is a single line, one is empty (r_i == r_i+1), one owns no processed pixel;
  * the first band is passed as row_begin = -3 and the last as row_end = H + 5 (call_range): the entry point clamps.
tests/test_bayes_rows_cases_cpu.py holds the lists to what the GPU tests rely on; tests/test_gpu_bayes_rows.py runs them."""
import numpy as np

import bayes_cases as bc
import marking_cases as mc
import marking_ref as mr

# (family, case name) of every case the band tests run, and the cut list of each
SELECTED = [("sizes", "sizes"), ("sizes", "sizes dense"),
            ("borders", "borders line 0"), ("borders", "borders line 1"), ("borders", "borders line 3"), ("borders", "borders dense full windows"),
            ("non-finite", "non-finite: nan colour"), ("non-finite", "non-finite: inf colour"), ("non-finite", "non-finite: nan pixcov"),
            ("other kernels", "w=1 b=12 sizes"), ("other kernels", "w=1 b=3 sizes"), ("other kernels", "w=2 b=6 sizes"), ("other kernels", "w=0 b=4 sizes"),
            ("other kernels", "w=2 b=6 dense"), ("other kernels", "w=1 b=4 dense")]

DENSE_34 = (0, 5, 16, 17, 17, 34)            # 34 x 40 dense frames: inside the first tile, on 16, a single line, an empty band
ISOLATED_100 = (0, 6, 7, 33, 48, 100)        # 100 x 150, items on lines 7, 22, ... (b = 6): [0, 6) and the single line [6, 7) own nothing
CUTS = {
    "sizes": ISOLATED_100, "borders line 0": ISOLATED_100, "borders line 1": ISOLATED_100, "borders line 3": ISOLATED_100,
    "sizes dense": DENSE_34, "borders dense full windows": DENSE_34, "w=1 b=4 dense": DENSE_34,
    "w=1 b=12 sizes": (0, 12, 13, 60, 110),  # items on lines 13, 40, 67, 94
    # every line of this frame from 2 to 31 is processed: the empty band [16, 16) is the one band of the list without an item
    "w=2 b=6 dense": (0, 9, 16, 16, 34),
    # 52 x 150, items on lines 7, 22, 37: the single line [7, 8) owns a row of items, [8, 16) none, [16, 16) is empty
    "non-finite: nan colour": (0, 7, 8, 16, 16, 37, 52), "non-finite: inf colour": (0, 7, 8, 16, 16, 37, 52), "non-finite: nan pixcov": (0, 7, 8, 16, 16, 37, 52),
    "w=1 b=3 sizes": (0, 4, 5, 16, 31, 32, 60),   # 60 x 100, items on lines 4, 13, ..., 49: two single lines that own items
    "w=2 b=6 sizes": (0, 8, 9, 32, 42, 80),       # 80 x 140, items on lines 8, 25, 42, 59: [0, 8) and [32, 42) own nothing
    "w=0 b=4 sizes": (0, 13, 14, 16, 48, 60),     # 60 x 100, items on lines 4, 13, ..., 49: [14, 16) owns nothing
}

_cases = {}


def case(name):
    """the bayes_cases.Case of that name, built once per session"""
    if not _cases:
        for family in sorted({f for f, _ in SELECTED}):
            for c in bc.FAMILIES[family]():
                _cases[c.name] = c
    return _cases[name]


def bands(name):
    cuts = CUTS[name]
    return list(zip(cuts[:-1], cuts[1:]))


def call_range(c, r0, r1):
    """(row_begin, row_end) as the band is handed to the entry point: the frame's first and last band reach past the frame"""
    H = c.col.shape[0]
    return (-3 if r0 == 0 else r0), (H + 5 if r1 == H else r1)


_banded = {}


def banded(c, r0, r1):
    """the case with the state image zeroed outside lines [max(0, r0), min(H, r1)); one object per (case, band), so that references are computed once"""
    key = (id(c), r0, r1)
    if key not in _banded:
        H = c.col.shape[0]
        o = bc.Case.__new__(bc.Case)
        o.__dict__.update(c.__dict__)
        o.state = np.zeros_like(c.state)
        a, e = max(0, r0), min(H, r1)
        if a < e:
            o.state[a:e] = c.state[a:e]
        o.name = "%s lines [%d, %d)" % (c.name, r0, r1)
        _banded[key] = (c, o)
    return _banded[key][1]


def poisoned_state(c, r0, r1, seed=0):
    """the state image of the case with a seeded mix of IN, UNDECIDED and NONE on the main pixels outside the owned lines: states of halo lines belong to
    their owners, an entry point that listed one of them would add an item the reference of the band does not have.  (Main pixels only: whatever a wrong
    kernel then does stays inside the images.)"""
    H, W = c.state.shape
    w = c.w
    rng = np.random.default_rng(1000 * seed + 31 * max(r0, 0) + r1)
    st = c.state.copy()
    mix = rng.choice(np.array([mr.ST_IN, mr.ST_UNDECIDED, mr.ST_NONE, mr.ST_IN], np.uint8), size=(H, W))
    out = np.ones((H, W), bool)
    out[max(0, r0):max(0, min(H, r1))] = False
    out &= mr.main_area(W, H, w)
    st[out] = mix[out]
    return st


# ---- the chain as the band driver runs it: marking on symmetric masks, then the estimate of the band ------------------------------------------------
CHAIN_BAND = (7, 41)
_chain = []


def chain_problem():
    """-> (Case on the `call sequence` frame (48 x 80) with the masks of a seeded symmetric random graph and every state 0, marking case of the same
    masks).  The estimate cases' own similar sets are not symmetric, which the marking kernels require (tests/marking_cases.py)."""
    if not _chain:
        full = bc.call_sequence()[0]
        H, W, _ = full.col.shape
        g = mc.random_graph(W, H, 1, 6, 0.3, 4711, "random 0.30 b=6 80x48 w=1 (estimate chain)")
        o = bc.Case.__new__(bc.Case)
        o.__dict__.update(full.__dict__)
        o.name, o.mask, o.nsim, o.state = "chain", g.mask, g.cnt, np.zeros((H, W), np.uint8)
        _chain.append((o, g))
    return _chain[0]


def with_state(c, state, name):
    o = bc.Case.__new__(bc.Case)
    o.__dict__.update(c.__dict__)
    o.state, o.name = np.ascontiguousarray(state, np.uint8), name
    return o
