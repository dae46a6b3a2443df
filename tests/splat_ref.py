"""Host restatement of the splatted add's definition (include/bcd_hip.h, bcd_hip_accum_add_splatted) in NumPy float32: expands samples at
continuous positions into the (line, col, r, g, b, w * f) stream that bcd::SamplesAccumulator::addSample would be fed -- for each sample
in order, line ascending, col ascending -- and counts the samples that contribute and those that are dropped.  The expected statistics
are oracle_lib.oracle_ops()["accumulate"](stream, W, H).  tests/splat_cases.py holds the constructed cases (radii of every neighbour-range
class, positions on the comparisons, the index clamp, tile-sized frames) and a gather model of the kernel that is checked against this."""
import numpy as np

F32 = np.float32


def filter_geometry(rx, ry):
    """(rx, ry, inv_rx, inv_ry) as float32 and (Kx, Ky) of the definition"""
    rx, ry = F32(rx), F32(ry)
    return rx, ry, F32(1) / rx, F32(1) / ry, int(np.ceil(rx + F32(0.5))), int(np.ceil(ry + F32(0.5)))


def expand(xy, rgb, weights, W, H, rx, ry, table, block=1 << 16):
    """-> (stream (m, 6) float32, samples_added, dropped)"""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    rgb = np.ascontiguousarray(rgb, F32).reshape(-1, 3)
    n = xy.shape[0]
    w = np.ones(n, F32) if weights is None else np.ascontiguousarray(weights, F32)
    T = np.ascontiguousarray(table, F32)
    TS = T.shape[0]
    assert T.shape == (TS, TS) and 1 <= TS <= 64
    rx, ry, inv_rx, inv_ry, Kx, Ky = filter_geometry(rx, ry)
    dl, dc = np.meshgrid(np.arange(-Ky, Ky + 1), np.arange(-Kx, Kx + 1), indexing="ij")      # candidates: line ascending, col ascending
    dl, dc = dl.reshape(1, -1), dc.reshape(1, -1)
    parts, added = [], 0
    for b0 in range(0, n, block):
        x, y = xy[b0:b0 + block, 0], xy[b0:b0 + block, 1]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(x) & np.isfinite(y) & (x >= F32(-Kx)) & (x < F32(W + Kx)) & (y >= F32(-Ky)) & (y < F32(H + Ky))
        idx = np.nonzero(ok)[0]
        x, y = x[idx][:, None], y[idx][:, None]
        col = np.floor(x).astype(np.int64) + dc
        line = np.floor(y).astype(np.int64) + dl
        dx = np.abs((col.astype(F32) + F32(0.5)) - x)
        dy = np.abs((line.astype(F32) + F32(0.5)) - y)
        assert dx.dtype == F32 and dy.dtype == F32
        ix = np.minimum((dx * inv_rx * F32(TS)).astype(np.int64), TS - 1)
        iy = np.minimum((dy * inv_ry * F32(TS)).astype(np.int64), TS - 1)
        f = T[np.clip(iy, 0, TS - 1), np.clip(ix, 0, TS - 1)]
        inside = (dx < rx) & (dy < ry) & (col >= 0) & (col < W) & (line >= 0) & (line < H) & (f != 0)
        added += int(np.count_nonzero(inside.any(axis=1)))
        s, c = np.nonzero(inside)                                  # row-major: sample after sample, each in candidate order
        e = idx[s] + b0
        wf = w[e] * f[s, c]
        assert wf.dtype == F32
        parts.append(np.stack([line[s, c].astype(F32), col[s, c].astype(F32), rgb[e, 0], rgb[e, 1], rgb[e, 2], wf], 1))
    stream = np.concatenate(parts, 0) if parts else np.zeros((0, 6), F32)
    return np.ascontiguousarray(stream, F32), added, n - added


def expand_loops(xy, rgb, weights, W, H, rx, ry, table):
    """the same by a plain triple loop (the definition read line by line); for tiny cases"""
    T = np.asarray(table, F32)
    TS = T.shape[0]
    rx, ry, inv_rx, inv_ry, Kx, Ky = filter_geometry(rx, ry)
    out, added = [], 0
    for i in range(len(xy)):
        x, y = F32(xy[i][0]), F32(xy[i][1])
        w = F32(1) if weights is None else F32(weights[i])
        if not (np.isfinite(x) and np.isfinite(y)) or not (F32(-Kx) <= x < F32(W + Kx)) or not (F32(-Ky) <= y < F32(H + Ky)):
            continue
        c0, l0, any_ = int(np.floor(x)), int(np.floor(y)), False
        for line in range(l0 - Ky, l0 + Ky + 1):
            for col in range(c0 - Kx, c0 + Kx + 1):
                dx, dy = np.abs((F32(col) + F32(0.5)) - x), np.abs((F32(line) + F32(0.5)) - y)
                if not (dx < rx and dy < ry) or not (0 <= col < W and 0 <= line < H):
                    continue
                ix = min(int(F32(F32(dx * inv_rx) * F32(TS))), TS - 1)
                iy = min(int(F32(F32(dy * inv_ry) * F32(TS))), TS - 1)
                f = T[iy, ix]
                if f != 0:
                    any_ = True
                    out.append([F32(line), F32(col), F32(rgb[i][0]), F32(rgb[i][1]), F32(rgb[i][2]), F32(w * f)])
        added += any_
    return np.array(out, F32).reshape(-1, 6), added, len(xy) - added
