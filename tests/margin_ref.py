"""NumPy model of the margin planes (k_pairdist_rw<MARGIN> in k_similarity_fast.hip, k_fwd_masks_w1m / _w1v4m in k_similarity.hip).  TEST INFRASTRUCTURE.

A margin plane holds one signed binary16 value per pixel pair, E = sum over the live bins of (d^2 / s - tau), and the mask kernels decide a patch pair
from SE = sum of its nine E and A = sum of their absolute values: similar when SE < -B, not similar when SE > B or when no entry of the patch has a
live bin, borderline (re-evaluated exactly on the device) otherwise, B = band_rel A + band_abs (bcd_margin_band in bcd_common.h; derivation in
k_similarity.hip).  This module evaluates the two margin forms of the distance kernel (the RATIO form keeps T and C planes) in float32 with a correctly rounded reciprocal and fma -- the device's
reciprocal is within one ulp of it, which the bound allows for -- rounds to binary16, and decides.  What the model must show is a condition, not a
tolerance: no decided pair may disagree with the float32 transcription of the reference (similarity_ref.distances32)."""
import numpy as np

import similarity_ref as sr

F = np.float32
U = 2.0 ** -24


def band(D, tau):
    """(band_rel, band_abs) as bcd_margin_band computes them"""
    fp = (2.0 * D + 32.0) * U
    rel = 2.0 * (2.0 ** -11 + 8.0 * U + fp) * (1.0 + 1e-3)
    ab = 2.0 * (fp * 18.0 * float(tau) * D + 9.0 * U) * (1.0 + 1e-3)
    return F(rel), F(ab)


def fma(a, b, c):
    """RN32(a b + c): the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def rcp(x):
    return (1.0 / np.asarray(x, np.float64)).astype(F)


def margin_planes(hist, ns, b, tau, form, bins=None):
    """-> (E16 (nd, H, W) float16, touched (nd, H, W) bool, valid).  form: 'uniform' (equal power-of-two counts: the margin accumulated bin by bin)
    or 'general' (the reference's diff and den, rcp + fma, E = fma(-tau, C, T'))"""
    H, W, D = hist.shape
    hist = np.asarray(hist, F)
    n = np.asarray(ns, F).reshape(H, W)
    tau = F(tau)
    bins = sr.occupied_bins(hist) if bins is None else bins
    hb = np.ascontiguousarray(np.moveaxis(hist[:, :, bins], -1, 0))
    nd = sr.delta_count(b)
    E, touched, valid = np.zeros((nd, H, W), np.float16), np.zeros((nd, H, W), bool), np.zeros((nd, H, W), bool)
    with np.errstate(all="ignore"):
        for (dl, dc) in sr.forward_offsets(b):
            v = sr._views(n, dl, dc)
            if v is None:
                continue
            n1, n2, sl = v
            n12 = n1 * n2
            acc, cnt = np.zeros(n1.shape, F), np.zeros(n1.shape, np.int32)
            for k in range(len(bins)):
                b1, b2, _ = sr._views(hb[k], dl, dc)
                s = b1 + b2
                use = s > F(1)
                if not use.any():
                    continue
                if form == "uniform":
                    d = b1 - b2
                    q = fma(d, d, -s) if tau == F(1) else fma(d, d, -(tau * s))
                    new = fma(q, rcp(s), acc)
                else:
                    d = n2 * b1 - n1 * b2
                    new = fma(d * d, rcp(n12 * s), acc)
                acc = np.where(use, new, acc)
                cnt += use
            if form != "uniform":
                acc = fma(-tau, cnt.astype(F), acc)
            e16 = acc.astype(np.float16)
            e16 = np.where(cnt > 0, np.where(e16 == 0, np.float16(0.0), e16), np.float16(-0.0))     # a touched zero is +0, "no live bin" is -0
            di = sr.delta_index(dl, dc, b)
            E[di][sl], touched[di][sl], valid[di][sl] = e16, cnt > 0, True
    return E, touched, valid


def decide(E16, touched, b, D, tau):
    """-> (H, W, (2b+1)^2) int8 over the forward offsets of the main pixels (w = 1): 1 decided similar, 0 decided not similar, 2 borderline, -1 outside"""
    nd, H, W = E16.shape
    side = 2 * b + 1
    out = np.full((H, W, side * side), -1, np.int8)
    rel, ab = band(D, tau)
    e = E16.astype(F)
    w = 1
    with np.errstate(all="ignore"):
        for (dl, dc) in sr.forward_offsets(b):
            l0, l1, c0, c1 = w, H - w - dl, max(w, w - dc), min(W - w, W - w - dc)
            if l0 >= l1 or c0 >= c1:
                continue
            di = sr.delta_index(dl, dc, b)
            se, a, any_touched = None, np.zeros((l1 - l0, c1 - c0), F), np.zeros((l1 - l0, c1 - c0), bool)
            for ol in (-1, 0, 1):
                for oc in (-1, 0, 1):
                    v = e[di, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
                    se = v.copy() if se is None else se + v
                    a = a + np.abs(v)
                    any_touched |= touched[di, l0 + ol:l1 + ol, c0 + oc:c1 + oc]
            B = fma(rel, a, ab)
            res = np.full(se.shape, 2, np.int8)
            res[se < -B] = 1
            res[se > B] = 0
            res[~any_touched] = 0
            out[l0:l1, c0:c1, (dl + b) * side + (dc + b)] = res
    return out


def check(case_dist, decision, tau):
    """-> (wrong decisions, borderline pairs, decided pairs) against the reference distances (NaN: never similar)"""
    known = decision >= 0
    with np.errstate(all="ignore"):
        ref = case_dist <= F(tau)
    wrong = int(np.count_nonzero(known & (decision != 2) & ((decision == 1) != ref)))
    return wrong, int(np.count_nonzero(decision == 2)), int(np.count_nonzero(known & (decision != 2)))
