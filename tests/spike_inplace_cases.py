"""The maps of the in-place gather tests (bcd_hip_spike_apply_inplace; DESIGN 13, "In place"): a generator of source maps by structure, the NumPy reference
and the two mutants a passing kernel cannot be.  tests/test_spike_inplace_cpu.py holds every case to the structure it names, tests/test_gpu_spike_inplace.py
runs them on the device.

A map M is an H x W int32 image; m(p) = M[p] when 0 <= M[p] < W*H, else p.  After the gather every image holds at p what it held BEFORE at m(p).

    identity      nothing moves
    one           one moved pixel
    cycle2        a swap p <-> q of two adjacent pixels
    cycle5        a cycle of five pixels spread over the frame
    chain         two chains of at least four pixels, one that reads upwards (p <- p' > p) and one that reads downwards, the first across a line boundary
                  and -- where the frame has more than 130 pixels -- across a multiple of 64 in the linear pixel index
    permutation   one random cycle through every pixel: 100 % moved
    fan_first     every pixel reads pixel 0
    fan_last      every pixel reads the last pixel
    half          about half the pixels read a random pixel (chains, cycles and fan-out as they fall)
    outside       `half` with a fifth of the entries outside [0, W*H): negative, W*H, INT32_MAX, INT32_MIN
    real          the oracle's decision on a spiky synthetic frame (40 x 28 only)"""
import numpy as np

CASES = ("identity", "one", "cycle2", "cycle5", "chain", "permutation", "fan_first", "fan_last", "half", "outside")
REAL_SIZE = (40, 28)   # W, H of the "real" case
REAL_SEEDS = (11, 12, 13)
SIZES = ((3, 3), (64, 4), (63, 3), (65, 5), (130, 7))
DEPTHS = (1, 3, 6, 7, 60)

_cache = {}


def chain_paths(W, H):
    """(upward path, downward path): along each, a pixel reads the next one.  The upward path crosses 63 -> 64 and a line boundary where the frame's first
    half holds them; the downward path is its mirror image from the last pixel"""
    n = W * H
    up = sorted(p for p in {62, 63, 64, 65, W - 2, W - 1, W, W + 1} if 0 <= p < (n - 1) // 2)
    if len(up) < 4:
        up = [0, 1, 2, 3]
    down = [n - 1 - p for p in up]
    return up, down


def real_frame(seed=REAL_SEEDS[0]):
    """(colours, sample counts, histograms, covariances) of the spiky 40 x 28 frame and its map at factor 2"""
    import oracle_lib as ol
    import spike_ref as sr
    key = ("real", seed)
    if key not in _cache:
        W, H = REAL_SIZE
        col, ns, hist, cov = ol.synth_inputs(W, H, 32, seed=seed, spike_prob=0.01)[:4]
        _cache[key] = (col, ns, hist, cov, sr.source_map(col, 2.0))
    return _cache[key]


def make(name, W, H, seed=0):
    """the map of a case as an H x W int32 array"""
    n = W * H
    rng = np.random.default_rng(1000 * seed + 7 * W + H)
    m = np.arange(n, dtype=np.int64)
    if name == "identity":
        pass
    elif name == "one":
        m[n // 2] = n // 2 - 1
    elif name == "cycle2":
        p = n // 2
        m[p], m[p + 1] = p + 1, p
    elif name == "cycle5":
        c = [(k * n) // 5 + 1 for k in range(5)]
        for i in range(5):
            m[c[i]] = c[(i + 1) % 5]
    elif name == "chain":
        for path in chain_paths(W, H):
            for a, b in zip(path[:-1], path[1:]):
                m[a] = b
    elif name == "permutation":
        order = rng.permutation(n)                     # one cycle: order[i] reads order[i + 1]
        m[order] = np.roll(order, -1)
    elif name == "fan_first":
        m[:] = 0
    elif name == "fan_last":
        m[:] = n - 1
    elif name in ("half", "outside"):
        pick = rng.random(n) < 0.5
        m[pick] = rng.integers(0, n, size=int(pick.sum()))
        if name == "outside":
            bad = np.array([-1, -n, n, n + 1, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int64)
            where = rng.random(n) < 0.2
            where[[0, n - 1]] = True
            m[where] = bad[rng.integers(0, bad.size, size=int(where.sum()))]
    elif name == "real":
        assert (W, H) == REAL_SIZE
        return real_frame(REAL_SEEDS[seed % len(REAL_SEEDS)])[4].copy()
    else:
        raise KeyError(name)
    return m.astype(np.int32).reshape(H, W)


def effective(M):
    """m(p) as a flat int64 array"""
    m = M.reshape(-1).astype(np.int64)
    return np.where((m >= 0) & (m < m.size), m, np.arange(m.size))


def moved(M):
    """the number of pixels with m(p) != p"""
    return int(np.count_nonzero(effective(M) != np.arange(M.size)))


def reference(img, M):
    """the gather: out[p] = img[m(p)], out of place"""
    d = img.size // M.size
    return np.ascontiguousarray(img.reshape(-1, d)[effective(M)].reshape(img.shape))


def sequential(img, M, descending=False):
    """the mutant: pixel by pixel IN PLACE, in ascending (or descending) pixel order -- what a kernel without staging computes in one of its orders"""
    d = img.size // M.size
    out = img.reshape(-1, d).copy()
    m = effective(M)
    for p in (range(M.size - 1, -1, -1) if descending else range(M.size)):
        out[p] = out[m[p]]
    return out.reshape(img.shape)
