"""NumPy emulation of similar-patch selection (oracle/bcd_oracle.c: pixel_summed_hist_distance, bcdo_patch_distance, bcdo_similarity_masks), operation by
operation in float32, and the same quantities in float64 real arithmetic.  TEST INFRASTRUCTURE.

float32 NumPy arithmetic rounds every operation to nearest, like the oracle built without contraction, so the planes, distances and masks here are the
oracle's bit for bit (tests/test_similarity_cases_cpu.py holds them to it at every threshold of every case); the GPU tests then use this module as their
reference, which costs a loop over the OCCUPIED bins of a frame instead of all of them and runs on frames of any size.

Layout: forward displacements (dl, dc) in the half plane dl > 0 or (dl == 0 and dc >= 0), index delta_index(dl, dc, b) -- the order of the kernels'
planes; planes are (nd, H, W) with entry [di, l, c] the pixel pair (l, c), (l + dl, c + dc), valid where that neighbour lies in the image; distances are
(H, W, (2b+1)^2) with +inf outside the clipped window (bcdo_window_distances) and mask bit k = (dl + b) (2b + 1) + (dc + b)."""
import numpy as np

F = np.float32
DELTA = 2.0 ** -10             # half-width of the verified band (BCD_APPROX_DELTA)
U = 2.0 ** -24                 # unit round-off of float32


def delta_count(b):
    return (b + 1) + b * (2 * b + 1)


def delta_index(dl, dc, b):
    return dc if dl == 0 else (b + 1) + (dl - 1) * (2 * b + 1) + (dc + b)


def forward_offsets(b):
    return [(0, dc) for dc in range(b + 1)] + [(dl, dc) for dl in range(1, b + 1) for dc in range(-b, b + 1)]


def occupied_bins(hist):
    """bins that can pass `b1 + b2 > 1` for some pixel pair"""
    m = hist.reshape(-1, hist.shape[-1]).max(0)
    return np.flatnonzero(m > 0.5)


def half(x):
    return np.asarray(x).astype(np.float16)


def prev(x):
    return np.nextafter(F(x), F(-np.inf))


def next_(x):
    return np.nextafter(F(x), F(np.inf))


def ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = next_(x) if k > 0 else prev(x)
    return x


def _views(a, dl, dc):
    """(a at x, a at x + (dl, dc)) over the pixels x whose neighbour lies in the image, and the slices of x"""
    H, W = a.shape[:2]
    l0, l1, c0, c1 = 0, H - dl, max(0, -dc), min(W, W - dc)
    if l0 >= l1 or c0 >= c1:
        return None
    return a[l0:l1, c0:c1], a[l0 + dl:l1 + dl, c0 + dc:c1 + dc], (slice(l0, l1), slice(c0, c1))


def planes32(hist, ns, b, bins=None):
    """-> (T (nd, H, W) float32, C (nd, H, W) int32, valid (nd, H, W) bool): per pixel pair the sequential sum over the bins with RN(b1 + b2) > 1 of
    RN(RN(diff^2) / den), diff = RN(RN(n2 b1) - RN(n1 b2)), den = RN(RN(n1 n2) RN(b1 + b2)), and the number of such bins"""
    H, W, D = hist.shape
    hist = np.asarray(hist, F)
    n = np.asarray(ns, F).reshape(H, W)
    bins = occupied_bins(hist) if bins is None else bins
    hb = np.ascontiguousarray(np.moveaxis(hist[:, :, bins], -1, 0))      # (nbins, H, W)
    nd = delta_count(b)
    T, C, valid = np.zeros((nd, H, W), F), np.zeros((nd, H, W), np.int32), np.zeros((nd, H, W), bool)
    with np.errstate(all="ignore"):
        for (dl, dc) in forward_offsets(b):
            v = _views(n, dl, dc)
            if v is None:
                continue
            n1, n2, sl = v
            n12 = n1 * n2
            s_, c_ = np.zeros(n1.shape, F), np.zeros(n1.shape, np.int32)
            for k in range(len(bins)):
                b1, b2, _ = _views(hb[k], dl, dc)
                s = b1 + b2
                use = s > F(1)
                if not use.any():
                    continue
                diff = n2 * b1 - n1 * b2
                term = (diff * diff) / (n12 * s)
                s_ = np.where(use, s_ + term, s_)
                c_ += use
            di = delta_index(dl, dc, b)
            T[di][sl], C[di][sl], valid[di][sl] = s_, c_, True
    return T, C, valid


def planes64(hist, ns, b, bins=None):
    """the same quantities in float64 real arithmetic (no intermediate float32 rounding); the skip test is the float32 one"""
    H, W, D = hist.shape
    hist = np.asarray(hist, F)
    n = np.asarray(ns, F).reshape(H, W)
    bins = occupied_bins(hist) if bins is None else bins
    hb = np.ascontiguousarray(np.moveaxis(hist[:, :, bins], -1, 0))
    nd = delta_count(b)
    T, C, valid = np.zeros((nd, H, W), np.float64), np.zeros((nd, H, W), np.int32), np.zeros((nd, H, W), bool)
    with np.errstate(all="ignore"):
        for (dl, dc) in forward_offsets(b):
            v = _views(n, dl, dc)
            if v is None:
                continue
            n1, n2 = v[0].astype(np.float64), v[1].astype(np.float64)
            sl = v[2]
            s_, c_ = np.zeros(n1.shape, np.float64), np.zeros(n1.shape, np.int32)
            for k in range(len(bins)):
                b1, b2, _ = _views(hb[k], dl, dc)
                use = (b1 + b2) > F(1)
                if not use.any():
                    continue
                x1, x2 = b1.astype(np.float64), b2.astype(np.float64)
                diff = n2 * x1 - n1 * x2
                s_ = s_ + np.where(use, diff * diff / np.where(use, n1 * n2 * (x1 + x2), 1.0), 0.0)
                c_ += use
            di = delta_index(dl, dc, b)
            T[di][sl], C[di][sl], valid[di][sl] = s_, c_, True
    return T, C, valid


def _distances(T, C, w, b, dtype):
    nd, H, W = T.shape
    side = 2 * b + 1
    out = np.full((H, W, side * side), np.inf, dtype)
    Hm, Wm = H - 2 * w, W - 2 * w
    if Hm <= 0 or Wm <= 0:
        return out
    with np.errstate(all="ignore"):
        for (dl, dc) in forward_offsets(b):
            # main pixels p (lines w .. H-1-w) whose partner p + (dl, dc) is a main pixel
            l0, l1, c0, c1 = w, H - w - dl, max(w, w - dc), min(W - w, W - w - dc)
            if l0 >= l1 or c0 >= c1:
                continue
            di = delta_index(dl, dc, b)
            s, n = np.zeros((l1 - l0, c1 - c0), dtype), np.zeros((l1 - l0, c1 - c0), np.int32)
            for ol in range(-w, w + 1):                              # the nine entries row-major from 0 (0 + t0 == t0)
                for oc in range(-w, w + 1):
                    s = s + T[di, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
                    n = n + C[di, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
            d = s / n.astype(dtype)                                  # one division; 0 / 0 = NaN
            out[l0:l1, c0:c1, (dl + b) * side + (dc + b)] = d
            out[l0 + dl:l1 + dl, c0 + dc:c1 + dc, (b - dl) * side + (b - dc)] = d
    return out


def distances32(hist, ns, b, w, bins=None, planes=None):
    """(H, W, (2b+1)^2) float32 patch distances of every main pixel to its clipped window, +inf elsewhere; NaN where no bin of the patch pair counts"""
    T, C, _ = planes32(hist, ns, b, bins) if planes is None else planes
    return _distances(T, C, w, b, F)


def distances64(hist, ns, b, w, bins=None, planes=None):
    T, C, _ = planes64(hist, ns, b, bins) if planes is None else planes
    return _distances(T, C, w, b, np.float64)


def pack(bits):
    """(H, W, n) bool -> (H, W, ceil(n / 32)) uint32, bit k in word k >> 5"""
    H, W, n = bits.shape
    words = (n + 31) // 32
    pad = np.zeros((H, W, words * 32), bool)
    pad[:, :, :n] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view("<u4")


def masks_from(dist, tau):
    """masks and |S| of bcdo_similarity_masks from the window distances: d <= tau (NaN and the +inf outside the window never are)"""
    bits = dist <= F(tau)
    if np.isinf(F(tau)):
        bits &= np.isfinite(dist)
    return pack(bits), bits.sum(-1).astype(np.int32)


def masks(hist, ns, w, b, tau, bins=None):
    return masks_from(distances32(hist, ns, b, w, bins), tau)


def window_valid(W, H, w, b):
    """(H, W, (2b+1)^2) bool: p and p + offset(k) are both main pixels (the clipped window of bcdo_similarity_masks)"""
    side = 2 * b + 1
    out = np.zeros((H, W, side * side), bool)
    main = np.zeros((H, W), bool)
    if H > 2 * w and W > 2 * w:
        main[w:H - w, w:W - w] = True
    for dl in range(-b, b + 1):
        for dc in range(-b, b + 1):
            l0, l1, c0, c1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)
            if l0 < l1 and c0 < c1:
                out[l0:l1, c0:c1, (dl + b) * side + (dc + b)] = main[l0:l1, c0:c1] & main[l0 + dl:l1 + dl, c0 + dc:c1 + dc]
    return out


def periodic_distances32(make, period, W, H, b, w, bins=None):
    """distances of a frame whose histograms and counts repeat with `period` = (lines, columns): d(p, p + delta) depends on p modulo the period wherever
    both patches lie in the image, so one period (computed inside a crop with a margin of b + w on every side) serves the whole frame.
    make(W, H) -> (hist, ns) of the frame at any size, pixel (0, 0) at phase 0.  -> (period lines, period columns, (2b+1)^2) float32"""
    pl, pc = period
    m = b + w
    ml, mc = -(-m // pl) * pl, -(-m // pc) * pc                      # margins that keep the phase
    hist, ns = make(mc + pc + m, ml + pl + m)
    d = distances32(hist, ns, b, w, bins)
    return d[ml:ml + pl, mc:mc + pc]


def tile_masks(dper, valid, tau):
    """masks of the full frame from one period of distances and window_valid() of the frame"""
    H, W, n = valid.shape
    pl, pc = dper.shape[:2]
    bits = dper <= F(tau)
    full = np.tile(bits, (-(-H // pl), -(-W // pc), 1))[:H, :W] & valid
    return pack(full), full.sum(-1).astype(np.int32)
