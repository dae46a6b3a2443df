"""NumPy reference of the motion path of the temporal calls (k_warp.hip, bcd_hip_denoise_temporal_motion; DESIGN.md section 16, "Motion").  TEST
INFRASTRUCTURE.

A motion field is (H, W, 2) float32, (dx, dy) per pixel of the frame: pixel (l, c) of the frame shows what pixel (l + ry, c + rx) of the neighbour shows,
rx = rint(dx), ry = rint(dy) (np.rint rounds halves to even, as rintf does).  The pixel is valid when dx and dy are finite, |dx|, |dy| < 2^24 and the source
lies inside the image.  `warp` gathers bit for bit (fancy indexing copies), invalid pixels are +0.0.  `valid_levels` follows tests/pyramid_ref.py's blocks:
coarse pixel (l, c) reads (2l, 2l + 1) x (2c, 2c + 1), a last odd line or column is read by nobody.  `pvalid` is the AND over the patch, False where the pixel
is not a main pixel; `gate` clears bit delta of main pixel p unless p + delta is a main pixel with pvalid (pixels that are not main pixels end with empty
masks and count 0, as the cross masks leave them).

denoise_one_scale_motion / denoise_multiscale_motion are temporal_ref.denoise_one_scale / denoise_multiscale with the neighbours warped at full resolution
and the gate between every neighbour's cross masks and the sum of the counts; a neighbour whose field is None is read where it lies and is not gated."""
import numpy as np

import marking_ref as mr
import pyramid_ref as pr
import similarity_ref as sr
import temporal_ref as tr

F = np.float32
LIMIT = F(2.0 ** 24)


def sources(mv, H, W):
    """-> (valid (H, W) bool, source line (H, W) int64, source column (H, W) int64; the indices of invalid pixels are 0)"""
    mv = np.asarray(mv, F).reshape(H, W, 2)
    dx, dy = mv[..., 0], mv[..., 1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(dx) & np.isfinite(dy) & (np.abs(dx) < LIMIT) & (np.abs(dy) < LIMIT)
        rx = np.rint(np.where(ok, dx, F(0))).astype(np.int64)
        ry = np.rint(np.where(ok, dy, F(0))).astype(np.int64)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sl, sc = l + ry, c + rx
    ok &= (sl >= 0) & (sl < H) & (sc >= 0) & (sc < W)
    return ok, np.where(ok, sl, 0), np.where(ok, sc, 0)


def warp(images, mv):
    """images: arrays (H, W) or (H, W, k) of one neighbour -> (their warped twins, valid (H, W) uint8).  mv None: zero motion"""
    H, W = images[0].shape[:2]
    ok, sl, sc = sources(np.zeros((H, W, 2), F) if mv is None else mv, H, W)
    out = []
    for a in images:
        a = np.asarray(a, F)
        g = a.reshape(H, W, -1)[sl, sc]
        g[~ok] = F(0)
        out.append(np.ascontiguousarray(g.reshape(a.shape)))
    return out, ok.astype(np.uint8)


def valid_down(valid):
    v = np.asarray(valid).astype(bool)
    H, W = v.shape
    h2, w2 = H // 2, W // 2
    l0, l1 = pr.block_index(H)
    c0, c1 = pr.block_index(W)
    out = v[l0][:, c0] & v[l1][:, c0] & v[l0][:, c1] & v[l1][:, c1]
    return out.reshape(h2, w2).astype(np.uint8)


def valid_levels(valid, nscales):
    out = [np.asarray(valid, np.uint8)]
    for _ in range(1, nscales):
        out.append(valid_down(out[-1]))
    return out


def pvalid(valid, w):
    v = np.asarray(valid).astype(bool)
    H, W = v.shape
    out = np.zeros((H, W), bool)
    if H <= 2 * w or W <= 2 * w:
        return out
    acc = np.ones((H - 2 * w, W - 2 * w), bool)
    for ol in range(-w, w + 1):
        for oc in range(-w, w + 1):
            acc &= v[w + ol:H - w + ol, w + oc:W - w + oc]
    out[w:H - w, w:W - w] = acc
    return out


def gate(mask, count, valid, w, b):
    """-> (gated masks (H, W, words) uint32, gated counts (H, W) int32); the inputs are left as they are"""
    H, W = np.asarray(valid).shape
    mask = np.ascontiguousarray(mask).view(np.uint32).reshape(H, W, -1)
    pv = pvalid(valid, w)
    out = np.zeros_like(mask)
    side = 2 * b + 1
    for k, (dl, dc) in enumerate(tr.window_offsets(b)):
        l0, l1, c0, c1 = max(w, w - dl), min(H - w, H - w - dl), max(w, w - dc), min(W - w, W - w - dc)      # main p with a main partner
        if l0 >= l1 or c0 >= c1:
            continue
        bit = np.uint32(1) << np.uint32(k & 31)
        keep = ((mask[l0:l1, c0:c1, k >> 5] & bit) != 0) & pv[l0 + dl:l1 + dl, c0 + dc:c1 + dc]
        out[l0:l1, c0:c1, k >> 5] |= np.where(keep, bit, np.uint32(0))
    cnt = np.unpackbits(out.view(np.uint8).reshape(H, W, -1), axis=-1)[..., :].sum(-1).astype(np.int32)
    assert side * side <= out.shape[-1] * 32
    return out, cnt


# ---- the whole composition ----------------------------------------------------------------------------------------------------------------------------
def select_one_scale(frame, neighbours, valids, w, b, tau, order, drawn):
    """the selection of one scale: -> dict(mask0, cross (gated masks per neighbour), total, state, lost (members the gate removed, per neighbour and pixel),
    frames (the list temporal_ref.accumulate takes))"""
    col, ns, hist, cov = frame
    mask0, n0 = sr.masks(hist, ns, w, b, tau)
    frames = [(col, pr.pixel_cov(cov, ns), mask0)]
    total = n0.astype(np.int32)
    cross, lost = [], []
    for (col_nb, ns_nb, hist_nb, cov_nb), v in zip(neighbours, valids):
        m, n = tr.cross_masks(hist, ns, hist_nb, ns_nb, w, b, tau)
        if v is not None:
            mg, ng = gate(m, n, v, w, b)
            lost.append(n.astype(np.int32) - ng)
            m, n = mg, ng
        else:
            lost.append(np.zeros_like(n, dtype=np.int32))
        with np.errstate(all="ignore"):
            frames.append((col_nb, pr.pixel_cov(cov_nb, ns_nb), m))
        cross.append(m)
        total = total + n
    state = mr.greedy(mask0, total, w, b, order, drawn)
    return dict(mask0=mask0, cross=cross, total=total, state=state, lost=lost, frames=frames)


def selection_stats(sel, w):
    K1 = 3 * (2 * w + 1) ** 2 + 1
    proc = sel["state"] == mr.ST_IN
    n = sel["total"][proc]
    return dict(processed=int(proc.sum()), fallback=int((n < K1).sum()), similar_total=int(n.sum()))


def denoise_one_scale_motion(frame, neighbours, valids, w, b, tau, min_eig, order, drawn, dtype=np.float64):
    """temporal_ref.denoise_one_scale on (already warped) neighbours with their validity images (None: not gated) -> (out, stats, selection)"""
    sel = select_one_scale(frame, neighbours, valids, w, b, tau, order, drawn)
    s, c, items = tr.accumulate(sel["frames"], sel["total"], (sel["state"] == mr.ST_IN).astype(np.uint8), w, b, min_eig, dtype)
    with np.errstate(all="ignore"):
        out = s / c.astype(dtype)[..., None]
    stats = selection_stats(sel, w)
    assert stats["processed"] == len(items)
    return out, stats, sel


def warped_levels(frame, neighbours, motions, nscales):
    """-> (levels[s] = [frame, neighbour 1, ...] at level s, valids[s] = [validity of neighbour 1 .. at level s, or None])"""
    first = [tuple(np.asarray(a, F) for a in frame)]
    v0 = []
    for f, mv in zip(neighbours, motions):
        if mv is None:
            first.append(tuple(np.asarray(a, F) for a in f))
            v0.append(None)
        else:
            H, W = np.asarray(f[2]).shape[:2]
            (c, n, h, v), ok = warp([f[0], np.asarray(f[1], F).reshape(H, W, 1), f[2], f[3]], mv)
            first.append((c, n.reshape(np.asarray(f[1]).shape), h, v))
            v0.append(ok)
    levels, valids = [first], [v0]
    with np.errstate(all="ignore"):
        for s in range(1, nscales):
            levels.append([(pr.downscale_avg(c), pr.downscale_sum(n), pr.downscale_sum(h), pr.downscale_cov(v, n)) for (c, n, h, v) in levels[-1]])
            valids.append([None if v is None else valid_down(v) for v in valids[-1]])
    return levels, valids


def select_multiscale_motion(frame, neighbours, motions, nscales, w, b, tau, orders, draws):
    """the selections of every scale (no estimate): [select_one_scale of scale 0, 1, ...]"""
    levels, valids = warped_levels(frame, neighbours, motions, nscales)
    return [select_one_scale(levels[s][0], levels[s][1:], valids[s], w, b, tau, orders[s], draws[s]) for s in range(nscales)]


def denoise_multiscale_motion(frame, neighbours, motions, nscales, w, b, tau, min_eig, orders, draws, dtype=np.float64):
    """the whole motion call -> (out (H, W, 3) dtype, [stats of scale 0, 1, ...])"""
    levels, valids = warped_levels(frame, neighbours, motions, nscales)
    outs, stats = [None] * nscales, [None] * nscales
    for s in range(nscales - 1, -1, -1):
        outs[s], stats[s], _ = denoise_one_scale_motion(levels[s][0], levels[s][1:], valids[s], w, b, tau, min_eig, orders[s], draws[s], dtype)
        if s < nscales - 1:
            outs[s] = pr.merge(outs[s], outs[s + 1], dtype=dtype)
    return outs[0], stats
