"""NumPy reference of the cross-frame similar-patch selection (k_similarity_cross.hip), operation by operation in float32, in the
style of tests/similarity_ref.py.  TEST INFRASTRUCTURE.

The frame t has histograms hist (H, W, D) and sample counts ns; a neighbour frame f of the sequence has hist_nb, ns_nb of the same shape.  For the pixel
pair x of the frame and x + (dl, dc) of the neighbour, the plane entry is the sequential sum over the bins with RN(b1 + b2) > 1 of RN(RN(diff^2) / den),
diff = RN(RN(n2 b1) - RN(n1 b2)), den = RN(RN(n1 n2) RN(b1 + b2)), with b1, n1 of the frame and b2, n2 of the neighbour, and the number of such bins.
The planes are not symmetric between two frames, so every displacement of the window has its own: planes are (side^2, H, W), side = 2b + 1, plane
k = (dl + b) side + (dc + b) -- the mask bit of that displacement --, valid where the neighbour pixel lies in the image.  Distances are
(H, W, side^2) with +inf outside the clipped window of main pixels; masks and |S_f| come from similarity_ref.masks_from.

float32 NumPy arithmetic rounds every operation to nearest, as the reference built without contraction does; tests/test_temporal_cases_cpu.py holds this
module to tests/similarity_ref.py (which tests/test_similarity_cases_cpu.py holds to the compiled oracle) on a frame compared with itself.

Further down: the estimate over members given as (frame, line, column), in float64 and float32, built on tests/bayes_ref.py; one scale of the whole
composition from similarity_ref, marking_ref, pyramid_ref and the above; and the multiscale call (every frame's pyramid, merges coarse to fine)."""
import numpy as np

import bayes_ref as br
import marking_ref as mr
import pyramid_ref as pr
import similarity_ref as sr

F = np.float32


def window_offsets(b):
    """all displacements of the window in mask-bit order"""
    return [(dl, dc) for dl in range(-b, b + 1) for dc in range(-b, b + 1)]


def _views2(a, a_nb, dl, dc):
    """(a at x, a_nb at x + (dl, dc)) over the pixels x whose neighbour pixel lies in the image, and the slices of x; dl and dc of either sign"""
    H, W = a.shape[:2]
    l0, l1, c0, c1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)
    if l0 >= l1 or c0 >= c1:
        return None
    return a[l0:l1, c0:c1], a_nb[l0 + dl:l1 + dl, c0 + dc:c1 + dc], (slice(l0, l1), slice(c0, c1))


def cross_bins(hist, hist_nb):
    """bins that can pass `b1 + b2 > 1` for some pixel pair of the two frames"""
    return np.union1d(sr.occupied_bins(hist), sr.occupied_bins(hist_nb))


def cross_planes32(hist, ns, hist_nb, ns_nb, b, bins=None):
    """-> (T (side^2, H, W) float32, C (side^2, H, W) int32, valid (side^2, H, W) bool)"""
    H, W, D = hist.shape
    assert hist_nb.shape == hist.shape
    hist, hist_nb = np.asarray(hist, F), np.asarray(hist_nb, F)
    n, n_nb = np.asarray(ns, F).reshape(H, W), np.asarray(ns_nb, F).reshape(H, W)
    bins = cross_bins(hist, hist_nb) if bins is None else bins
    hb = np.ascontiguousarray(np.moveaxis(hist[:, :, bins], -1, 0))          # (nbins, H, W)
    hb_nb = np.ascontiguousarray(np.moveaxis(hist_nb[:, :, bins], -1, 0))
    side = 2 * b + 1
    T, C, valid = np.zeros((side * side, H, W), F), np.zeros((side * side, H, W), np.int32), np.zeros((side * side, H, W), bool)
    with np.errstate(all="ignore"):
        for k, (dl, dc) in enumerate(window_offsets(b)):
            v = _views2(n, n_nb, dl, dc)
            if v is None:
                continue
            n1, n2, sl = v
            n12 = n1 * n2
            s_, c_ = np.zeros(n1.shape, F), np.zeros(n1.shape, np.int32)
            for i in range(len(bins)):
                b1, b2, _ = _views2(hb[i], hb_nb[i], dl, dc)
                s = b1 + b2
                use = s > F(1)
                if not use.any():
                    continue
                diff = n2 * b1 - n1 * b2
                term = (diff * diff) / (n12 * s)
                s_ = np.where(use, s_ + term, s_)
                c_ += use
            T[k][sl], C[k][sl], valid[k][sl] = s_, c_, True
    return T, C, valid


def cross_distances32(hist, ns, hist_nb, ns_nb, b, w, bins=None, planes=None):
    """(H, W, side^2) float32 patch distances of every main pixel of the frame to the main pixels of the neighbour in its clipped window, +inf elsewhere;
    NaN where no bin of the patch pair counts"""
    T, C, _ = cross_planes32(hist, ns, hist_nb, ns_nb, b, bins) if planes is None else planes
    nk, H, W = T.shape
    side = 2 * b + 1
    out = np.full((H, W, side * side), np.inf, F)
    if H <= 2 * w or W <= 2 * w:
        return out
    with np.errstate(all="ignore"):
        for k, (dl, dc) in enumerate(window_offsets(b)):
            # main pixels p whose partner p + (dl, dc) is a main pixel
            l0, l1, c0, c1 = max(w, w - dl), min(H - w, H - w - dl), max(w, w - dc), min(W - w, W - w - dc)
            if l0 >= l1 or c0 >= c1:
                continue
            s, n = np.zeros((l1 - l0, c1 - c0), F), np.zeros((l1 - l0, c1 - c0), np.int32)
            for ol in range(-w, w + 1):                              # the patch entries row-major from 0 (0 + t0 == t0)
                for oc in range(-w, w + 1):
                    s = s + T[k, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
                    n = n + C[k, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
            out[l0:l1, c0:c1, k] = s / n.astype(F)                   # one division; 0 / 0 = NaN
    return out


def cross_masks(hist, ns, hist_nb, ns_nb, w, b, tau, bins=None):
    """masks (H, W, words) uint32 and |S_f| (H, W) int32 of one neighbour"""
    return sr.masks_from(cross_distances32(hist, ns, hist_nb, ns_nb, b, w, bins), tau)


# ---- the estimate over members of several frames ---------------------------------------------------------------------------------------------------
# Built on tests/bayes_ref.py (a restatement of denoiseSelectedPatches / denoiseOnlyMainPatch / aggregateOutputPatches from the reference text), run in
# float64 (the reference the kernels are judged against) or float32 (the calibrator, LAPACK ssyevd on float32 input).  Frame 0 is the frame itself;
# members are (frame, line, column) in member order: S_0 in window order, then S_1 .. S_F, each in window order.
def stages(cols, pixcovs, members, w=1, min_eig=1e-8, dtype=np.float64):
    """every intermediate of the estimate of one similar set spread over several frames.  cols / pixcovs: lists of (H, W, 3) / (H, W, 6) images,
    members (n, 3).  Noise mean, colour mean and covariance run over ALL members, each member's per-pixel covariance from its own frame; "step2" holds the
    estimates of the members of frame 0 only (the neighbours lend statistics).  Fallback sets (n < 3 (2w+1)^2 + 1) stop at the mean over all members."""
    dt = np.dtype(dtype).type
    members = np.asarray(members, np.int64).reshape(-1, 3)
    n = members.shape[0]
    P = (2 * w + 1) ** 2
    K = 3 * P
    X = np.empty((n, K), dt)
    N6 = np.empty((n, P, 6), dt)
    for f in np.unique(members[:, 0]):
        sel = members[:, 0] == f
        X[sel] = br.gather(cols[f], members[sel, 1:], w).astype(dt).reshape(-1, K)        # :483-498: pixel-major, RGB
        N6[sel] = br.gather(pixcovs[f], members[sel, 1:], w).astype(dt)
    own = members[:, 0] == 0
    with np.errstate(all="ignore"):
        st = {"x": X, "mean1": X.mean(axis=0)}
        if n < K + 1:
            return st
        noise6 = N6.sum(axis=0) / dt(n)                                  # computeNoiseCovPatchesMean (:400-419)
        N = np.zeros((K, K), dt)
        for o in range(P):
            xx, yy, zz, yz, xz, xy = noise6[o]                           # CovarianceMatrix.h:18-27
            N[3 * o:3 * o + 3, 3 * o:3 * o + 3] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
        floor = dt(min_eig)
        inv = lambda lam: dt(1.0) / np.maximum(floor, lam)
        Xc = X - st["mean1"]
        C = Xc.T @ Xc / dt(n - 1)                                        # :522-536
        clamped, eig_cmn = br._spectral(C - N, lambda lam: np.maximum(dt(0.0), lam))      # :606-630
        inv1, lam1 = br._spectral(clamped + N, inv)                      # :578-604
        X1 = X - (N @ (inv1 @ Xc.T)).T                                   # :656-670
        m2 = X1.mean(axis=0)
        X1c = X1 - m2
        C2 = X1c.T @ X1c / dt(n - 1)
        inv2, lam2 = br._spectral(C2 + N, inv)
        X2 = X[own] - (N @ (inv2 @ (X[own] - m2).T)).T                   # :449-450, for the members of the frame itself
        cond = lambda lam: float(np.max(np.maximum(floor, lam)) / np.min(np.maximum(floor, lam)))
        st.update(noise=noise6, cov1=C, step2=X2, eig_cmn=eig_cmn, cond1=cond(lam1), cond2=cond(lam2))
    return st


def members_of(masks, l, c, b):
    """(n, 3) members of the main pixel (l, c) from the mask words of every frame, in member order"""
    out = []
    for f, m in enumerate(masks):
        pos = br.decode_members(m[l, c], l, c, b)
        out.append(np.concatenate([np.full((len(pos), 1), f, np.int64), pos], axis=1))
    return np.concatenate(out, axis=0)


def accumulate(frames, nsim_total, state, w, b, min_eig, dtype=np.float64):
    """frames: list of (col, pixcov, mask), [0] the frame itself -> (sum (H, W, 3) dtype, count (H, W) int32, per_item) in the terms of
    bcd_hip_bayes_accumulate_temporal.  per_item: "pos", "members" (the IN-FRAME members (n0, 2): what the item writes), "n" (the total |S|), cond1, cond2,
    eig_cmn -- the fields tests/bayes_ref.py's touched() and item_error() read."""
    dt = np.dtype(dtype).type
    cols, pixcovs = [f[0] for f in frames], [f[1] for f in frames]
    H, W, _ = cols[0].shape
    masks = [np.ascontiguousarray(f[2]).view(np.uint32).reshape(H, W, -1) for f in frames]
    acc = np.zeros((H, W, 3), dt)
    cnt = np.zeros((H, W), np.int32)
    P = (2 * w + 1) ** 2
    K = 3 * P
    oa = np.array([a for (a, d) in br.offsets(w)])
    od = np.array([d for (a, d) in br.offsets(w)])
    per_item = []
    with np.errstate(all="ignore"):
        for l, c in zip(*np.nonzero(np.asarray(state) == 1)):
            l, c = int(l), int(c)
            mem = members_of(masks, l, c, b)
            n = mem.shape[0]
            assert n == int(nsim_total[l, c]), "nsim_total must be the popcount of the masks of all frames"
            st = stages(cols, pixcovs, mem, w, min_eig, dtype) if n else {"mean1": np.full(K, np.nan, dt)}
            pos = mem[mem[:, 0] == 0, 1:]
            item = {"pos": (l, c), "members": pos, "n": n}
            item.update({k: st[k] for k in ("cond1", "cond2", "eig_cmn") if k in st})
            per_item.append(item)
            if n < K + 1:
                np.add.at(acc, (l + oa, c + od), st["mean1"].reshape(P, 3))
                np.add.at(cnt, (l + oa, c + od), 1)
                continue
            rows = (pos[:, 0][:, None] + oa).ravel()
            cols_ = (pos[:, 1][:, None] + od).ravel()
            np.add.at(acc, (rows, cols_), st["step2"].reshape(len(pos) * P, 3))
            np.add.at(cnt, (rows, cols_), 1)
    return acc, cnt, per_item


# ---- one scale of the whole composition -------------------------------------------------------------------------------------------------------------
def denoise_one_scale(frame, neighbours, w, b, tau, min_eig, order, drawn, dtype=np.float64):
    """frame, neighbours[i]: (col, ns, hist, cov).  In-frame masks (similarity_ref), cross masks per neighbour, the reference's sequential marking on the
    in-frame masks and the total |S| (marking_ref.greedy: a processed pixel with |S| >= 3P + 1 marks its in-frame members), the estimate over all members,
    finalAggregation.  order: the visiting order (linear indices of the main pixels), drawn: marking_ref.skip_draw.
    -> (out (H, W, 3) dtype, dict(processed, fallback, similar_total), state)"""
    col, ns, hist, cov = frame
    mask0, n0 = sr.masks(hist, ns, w, b, tau)
    frames = [(col, pr.pixel_cov(cov, ns), mask0)]
    total = n0.astype(np.int32)
    for (col_nb, ns_nb, hist_nb, cov_nb) in neighbours:
        m, n = cross_masks(hist, ns, hist_nb, ns_nb, w, b, tau)
        frames.append((col_nb, pr.pixel_cov(cov_nb, ns_nb), m))
        total = total + n
    state = mr.greedy(mask0, total, w, b, order, drawn)
    s, c, items = accumulate(frames, total, (state == mr.ST_IN).astype(np.uint8), w, b, min_eig, dtype)
    with np.errstate(all="ignore"):
        out = s / c.astype(dtype)[..., None]
    K1 = 3 * (2 * w + 1) ** 2 + 1
    stats = dict(processed=len(items), fallback=sum(1 for i in items if i["n"] < K1), similar_total=int(sum(i["n"] for i in items)))
    return out, stats, state


def denoise_multiscale(frame, neighbours, nscales, w, b, tau, min_eig, orders, draws, dtype=np.float64):
    """the whole call: every frame's pyramid by the reducers of pyramid_ref (colours averaged, counts and histograms summed, covariances weighted by the
    counts), scale s on level s of every frame with orders[s] / draws[s], mergeOutputs coarse to fine.
    -> (out (H, W, 3) dtype, [stats of scale 0, 1, ...])"""
    levels = [[tuple(np.asarray(a, F) for a in f) for f in [frame] + list(neighbours)]]
    for s in range(1, nscales):
        levels.append([(pr.downscale_avg(c), pr.downscale_sum(n), pr.downscale_sum(h), pr.downscale_cov(v, n)) for (c, n, h, v) in levels[-1]])
    outs, stats = [None] * nscales, [None] * nscales
    for s in range(nscales - 1, -1, -1):
        outs[s], stats[s], _ = denoise_one_scale(levels[s][0], levels[s][1:], w, b, tau, min_eig, orders[s], draws[s], dtype)
        if s < nscales - 1:
            outs[s] = pr.merge(outs[s], outs[s + 1], dtype=dtype)
    return outs[0], stats
