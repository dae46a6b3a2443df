"""References of the spike prefilter's source map (include/bcd_hip.h, "the spike prefilter through a source map"): the map M[p] = the pixel that
SpikeRemovalFilter::filter copies into p, and the gather through it.

source_map   the oracle's filter fed pixel indices as the sample-count image: the filtered sample counts ARE the map (float32 holds the indices
             exactly, the frames are far below 2^24 pixels)
gather       img[M] in NumPy
numpy_map    a second, independent statement of the decision in NumPy float32 (sequential sums in the filter's order, IEEE operations, no
             contraction), with the spike flags: what "every pixel is a spike" or "nothing is a spike" is checked against"""
import numpy as np

import oracle_lib as ol


def source_map(col, factor):
    H, W, _ = col.shape
    assert W * H < (1 << 24)
    idx = np.arange(W * H, dtype=np.float32).reshape(H, W, 1)
    hist = np.zeros((H, W, 1), np.float32)
    cov = np.zeros((H, W, 6), np.float32)
    _, n, _, _ = ol.oracle_ops()["spike"](np.ascontiguousarray(col, np.float32), idx, hist, cov, factor)
    m = n.reshape(H, W).astype(np.int64)
    assert np.array_equal(m.astype(np.float32), n.reshape(H, W))
    return m.astype(np.int32)


def gather(img, M):
    """img (H x W x depth, any dtype) gathered through the map M (H x W): out[p] = img[M[p]]"""
    H, W = M.shape
    flat = img.reshape(H * W, -1)
    return np.ascontiguousarray(flat[M.reshape(-1)].reshape(img.shape))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chains(M):
    """moved pixels whose source is itself moved"""
    m = M.reshape(-1)
    ident = np.arange(m.size)
    moved = m != ident
    return int(np.count_nonzero(moved & moved[m]))


def max_offsets(M):
    """(largest line distance, largest column distance) between a pixel and its source"""
    H, W = M.shape
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return int(np.max(np.abs(M // W - l))), int(np.max(np.abs(M % W - c)))


def numpy_map(col, factor):
    """(map, spike flags) by the filter's rules in float32: window of nine centred on the pixel, one pixel inward at the border; per channel the mean
    (sum / 9) and standard deviation (sqrt(sum of squares / 8)) summed in window order; a spike when |value - mean| > factor * sd in one channel
    (a comparison with NaN is false); the replacement is the first window member with the smallest L1 distance sum to the nine"""
    col = np.ascontiguousarray(col, np.float32)
    H, W, _ = col.shape
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cl, cc = np.clip(l, 1, H - 2), np.clip(c, 1, W - 2)
    nl = [cl + d for d in (-1, 0, 1) for _ in range(3)]
    nc = [cc + d for _ in range(3) for d in (-1, 0, 1)]
    v = [col[nl[k], nc[k]] for k in range(9)]                       # nine H x W x 3 images
    f32 = np.float32
    with np.errstate(all="ignore"):
        total = np.zeros((H, W, 3), f32)
        for k in range(9):
            total = total + v[k]
        avg = total / f32(9)
        total = np.zeros((H, W, 3), f32)
        for k in range(9):
            total = total + (v[k] - avg) * (v[k] - avg)
        sd = np.sqrt(total / f32(8))
        spike = np.any(np.abs(col - avg) > f32(factor) * sd, axis=-1)
        best = np.zeros((H, W), np.int64)
        bestd = np.full((H, W), -1.0, f32)
        for m in range(9):
            tot = np.zeros((H, W), f32)
            for i in range(9):
                d = np.abs(v[i] - v[m])
                tot = tot + ((d[..., 0] + d[..., 1]) + d[..., 2])
            take = (bestd < 0) | (tot < bestd)
            bestd = np.where(take, tot, bestd)
            best = np.where(take, m, best)
    src = (cl - 1 + best // 3) * W + (cc - 1 + best % 3)
    M = np.where(spike, src, l * W + c).astype(np.int32)
    return M, spike
