"""NumPy float32 restatement of the feature gate of the cross-frame selection ("Features"; k_similarity_guide_cross.hip, k_masks_cross, k_gate_masks,
k_warp_features).  TEST INFRASTRUCTURE: vectorised over the frame, one displacement at a time; every NumPy float32 operation is one IEEE operation.

For pixel x of the frame and pixel y = x + delta of neighbour j, y inside the image, channels k = 0 .. F-1 in order, from s = 0, n = 0 (f0, v0: the frame's
features and variances, fj, vj: the neighbour's, eps_k: the floor of channel k):
    d = f0_k(x) - fj_k(y);   q = (v0_k(x) + vj_k(y)) + eps_k   (no variances: q = 0 + eps_k)
    if q > 0: t = (d * d) / q;  if t == t: s = s + t, n = n + 1
    T_delta(x) = s, C_delta(x) = n
for ALL (2b+1)^2 displacements, plane k = (dl + b)(2b + 1) + (dc + b) being mask bit k (temporal_ref.window_offsets).  The box sum, the clipped window and the
masks are temporal_ref.cross_distances32 / similarity_ref.masks_from on these planes; the gate is guide_ref.gate.

Further down the whole call: temporal_ref's estimate on gated masks, guide_ref.pyramid per frame, motion_ref's warp of the features and its validity gate."""
import numpy as np

import guide_ref as gr
import marking_ref as mr
import motion_ref as mo
import pyramid_ref as pr
import similarity_ref as sr
import temporal_ref as tr

F32 = np.float32


def cross_planes(f, v, f_nb, v_nb, b, floors, second=None, flip=False):
    """-> T (side^2, H, W) float32, C (side^2, H, W) int32, written (side^2, H, W) bool (the entries whose y lies in the image; the others stay 0).
    second / flip build the deliberately WRONG mutants of tests/test_guide_cross_cases_cpu.py: second="frame" reads the second operand from the frame,
    flip=True files the plane of delta under -delta."""
    f, f_nb = np.asarray(f, F32), np.asarray(f_nb, F32)
    assert (v is None) == (v_nb is None) and f.shape == f_nb.shape
    v = None if v is None else np.asarray(v, F32)
    v_nb = None if v_nb is None else np.asarray(v_nb, F32)
    if second == "frame":
        f_nb, v_nb = f, v
    H, W, F = f.shape
    eps = np.asarray(floors, F32).reshape(-1)
    assert eps.size == F
    side = 2 * b + 1
    T, C, written = np.zeros((side * side, H, W), F32), np.zeros((side * side, H, W), np.int32), np.zeros((side * side, H, W), bool)
    with np.errstate(all="ignore"):
        for k, (dl, dc) in enumerate(tr.window_offsets(b)):
            got = tr._views2(f, f_nb, dl, dc)
            if got is None:
                continue
            fx, fy, sl = got
            if v is not None:
                vx, vy, _ = tr._views2(v, v_nb, dl, dc)
            s = np.zeros(fx.shape[:2], F32)
            n = np.zeros(fx.shape[:2], np.int32)
            for c in range(F):
                d = fx[..., c] - fy[..., c]
                q = np.full(d.shape, F32(0) + eps[c], F32) if v is None else (vx[..., c] + vy[..., c]) + eps[c]
                t = (d * d) / q
                ok = (q > 0) & (t == t)
                s = np.where(ok, s + t, s)
                n = n + ok
            kk = (-dl + b) * side + (-dc + b) if flip else k
            T[kk][sl], C[kk][sl], written[kk][sl] = s, n, True
    return T, C, written


def cross_distances(f, v, f_nb, v_nb, w, b, floors, **mutant):
    """(H, W, side^2) float32 cross feature distances of every main pixel to the main pixels of the neighbour in its clipped window, +inf elsewhere"""
    return tr.cross_distances32(None, None, None, None, b, w, planes=cross_planes(f, v, f_nb, v_nb, b, floors, **mutant))


def cross_masks(f, v, f_nb, v_nb, w, b, floors, tau, **mutant):
    """the cross feature mask G_j (H, W, words) uint32 and its counts (H, W) int32"""
    m, n = sr.masks_from(cross_distances(f, v, f_nb, v_nb, w, b, floors, **mutant), tau)
    return np.ascontiguousarray(m).view(np.uint32), n


def gate(mask, feature_mask):
    """(mask AND feature mask) as uint32 words, popcount"""
    m, n = gr.gate(mask, feature_mask)
    return m.view(np.uint32), n


def warp_features(f, v, mv):
    """-> (warped features, warped variances or None, valid (H, W) uint8): motion_ref.warp of the feature images"""
    imgs = [f] if v is None else [f, v]
    out, valid = mo.warp(imgs, mv)
    return out[0], (None if v is None else out[1]), valid


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------------------
def select_one_scale(frame, neighbours, valids, guides, floors, tau_g, w, b, tau, order, drawn):
    """motion_ref.select_one_scale with the gates of "Features": guides[f] = (features, variances or None) of frame f at this level, [0] the frame's"""
    col, ns, hist, cov = frame
    f0, v0 = guides[0]
    mask0, _ = sr.masks(hist, ns, w, b, tau)
    mask0, n0 = gate(mask0, gr.masks(f0, v0, w, b, floors, tau_g)[0])
    frames = [(col, pr.pixel_cov(cov, ns), mask0)]
    total = n0.astype(np.int32)
    cross = []
    for (col_nb, ns_nb, hist_nb, cov_nb), valid, (fj, vj) in zip(neighbours, valids, guides[1:]):
        m, n = tr.cross_masks(hist, ns, hist_nb, ns_nb, w, b, tau)
        if valid is not None:
            m, n = mo.gate(m, n, valid, w, b)
        m, n = gate(m, cross_masks(f0, v0, fj, vj, w, b, floors, tau_g)[0])
        with np.errstate(all="ignore"):
            frames.append((col_nb, pr.pixel_cov(cov_nb, ns_nb), m))
        cross.append(m)
        total = total + n
    state = mr.greedy(mask0, total, w, b, order, drawn)
    return dict(mask0=mask0, cross=cross, total=total, state=state, frames=frames)


def guide_levels(guide, neighbour_guides, motions, nscales):
    """-> levels[s] = [(features, variances) of the frame, of neighbour 1, ...] at level s: a neighbour with a field is warped at full resolution first"""
    first = [(np.asarray(guide[0], F32), None if guide[1] is None else np.asarray(guide[1], F32))]
    for (f, v), mv in zip(neighbour_guides, motions):
        if mv is None:
            first.append((np.asarray(f, F32), None if v is None else np.asarray(v, F32)))
        else:
            wf, wv, _ = warp_features(f, v, mv)
            first.append((wf, wv))
    pyr = [gr.pyramid(f, v, nscales) for f, v in first]
    return [[p[s] for p in pyr] for s in range(nscales)]


def denoise_multiscale(frame, neighbours, motions, guide, neighbour_guides, floors, tau_g, nscales, w, b, tau, min_eig, orders, draws, dtype=np.float64,
                       selections=None):
    """the whole guided temporal call on one layer.  frame, neighbours[i]: (col, ns, hist, cov); motions: None or one field / None per neighbour; guide,
    neighbour_guides[i]: (features, variances or None) -> (out (H, W, 3) dtype, [stats of scale 0, 1, ...]).  selections: a dict that keeps the selection
    of every scale -- it reads sample counts, histograms and features only, so a further layer of the same frames (other colours and covariances) passes
    the dict of the first and only its estimate is computed"""
    motions = [None] * len(neighbours) if motions is None else list(motions)
    levels, valids = mo.warped_levels(frame, neighbours, motions, nscales)
    glev = guide_levels(guide, neighbour_guides, motions, nscales)
    outs, stats = [None] * nscales, [None] * nscales
    for s in range(nscales - 1, -1, -1):
        if selections is not None and s in selections:
            sel = dict(selections[s])
            with np.errstate(all="ignore"):
                sel["frames"] = [(f[0], pr.pixel_cov(f[3], f[1]), m) for f, m in zip(levels[s], [sel["mask0"]] + sel["cross"])]
        else:
            sel = select_one_scale(levels[s][0], levels[s][1:], valids[s], glev[s], floors, tau_g, w, b, tau, orders[s], draws[s])
            if selections is not None:
                selections[s] = sel
        acc, cnt, items = tr.accumulate(sel["frames"], sel["total"], (sel["state"] == mr.ST_IN).astype(np.uint8), w, b, min_eig, dtype)
        with np.errstate(all="ignore"):
            outs[s] = acc / cnt.astype(dtype)[..., None]
        stats[s] = mo.selection_stats(sel, w)
        assert stats[s]["processed"] == len(items)
        if s < nscales - 1:
            outs[s] = pr.merge(outs[s], outs[s + 1], dtype=dtype)
    return outs[0], stats
