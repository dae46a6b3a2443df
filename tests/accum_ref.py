"""Float64 reference of SamplesAccumulator::addSample and computeSampleStatistics (the definition in include/bcd_hip.h and the comments of
k_accumulate.hip), one sample at a time in plain NumPy, and the per-bin error bound that the device's histograms are held to.
TEST INFRASTRUCTURE.

Only the exponent 1.f / gamma is evaluated in fp32, as the code does; everything else is float64 on the fp32 inputs.

The bound.  For gamma > 1 a device bin may differ from the float64 bin by the error of powf, the fp32 rounding of the division and of
v * (nbins - 2), and the fp32 additions into the bin, nothing else:

    |got - ref64| <= sum over the samples touching the bin of w ((nbins - 2) U ulp32(v) + 3 * 2^-24) + k 2^-24 sum(w)

k: samples in the pixel, sum(w): the pixel's weight sum, U: ulps of v granted to powf and the division together.  A sample TOUCHES the two
bins its float64 position falls between; when that position is within NEAR_ULPS ulps of v of a bin edge J the fp32 position may be on the
other side, so it touches J - 1, J and J + 1.  With 2 bins the factor nbins - 2 is taken as 1: the saturation weight is v - 1 itself.
A bin that no sample of its pixel touches must be exactly 0."""
import numpy as np

F32 = np.float32
F64 = np.float64
EPS = 2.0 ** -24
NEAR_ULPS = 16.0


class Result:
    """hist, ns, mean, cov: float64 images flattened over pixels ([N, D], [N], [N, 3], [N, 6]); per sample of the stream: pixel [n],
    w [n], v [n, 3] (transformed value), pos [n, 3] (v * (nbins - 2)), lo [n, 3] (lower bin); per pixel: wsum [N], count [N]"""


def accumulate(stream, W, H, nbins, gamma, maxval):
    stream = np.asarray(stream, F32)
    N, D, n = W * H, 3 * nbins, stream.shape[0]
    wsum, w2sum, msum, csum, hist = np.zeros(N), np.zeros(N), np.zeros((N, 3)), np.zeros((N, 6)), np.zeros((N, D))
    count = np.zeros(N, np.int64)
    pixel, V, POS, LO = np.zeros(n, np.int64), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3), np.int64)
    expo = F64(F32(1) / F32(gamma))
    mv = F64(F32(maxval))
    sat = 2.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(n):                                            # addSample
            line, col = int(stream[i, 0]), int(stream[i, 1])
            R, G, B, w = (F64(x) for x in stream[i, 2:6])
            p = line * W + col
            pixel[i] = p
            count[p] += 1
            wsum[p] += w
            w2sum[p] += w * w
            msum[p] += (w * R, w * G, w * B)
            csum[p] += (w * R * R, w * G * G, w * B * B, w * G * B, w * R * B, w * R * G)
            for ch, x in enumerate((R, G, B)):
                v = x if x > 0 else 0.0
                if gamma > 1:
                    v = v ** expo
                if maxval > 0:
                    v = v / mv
                v = sat if v > sat else v
                fi = v * (nbins - 2)
                lo = int(fi)
                if lo < nbins - 2:
                    hw = fi - lo
                else:
                    lo, hw = nbins - 2, (v - 1.0) / (sat - 1.0)
                hist[p, ch * nbins + lo] += w * (1.0 - hw)
                hist[p, ch * nbins + lo + 1] += w * hw
                V[i, ch], POS[i, ch], LO[i, ch] = v, fi, lo
        inv = 1.0 / wsum                                              # computeSampleStatistics
        mean = inv[:, None] * msum
        cv = csum * inv[:, None]
        cv[:, 0] -= mean[:, 0] * mean[:, 0]; cv[:, 1] -= mean[:, 1] * mean[:, 1]; cv[:, 2] -= mean[:, 2] * mean[:, 2]
        cv[:, 3] -= mean[:, 1] * mean[:, 2]; cv[:, 4] -= mean[:, 0] * mean[:, 2]; cv[:, 5] -= mean[:, 0] * mean[:, 1]
        cov = cv * (1.0 / (1.0 - w2sum / (wsum * wsum)))[:, None]
    r = Result()
    r.W, r.H, r.nbins, r.gamma, r.maxval = W, H, nbins, gamma, maxval
    r.hist, r.ns, r.mean, r.cov = hist, wsum, mean, cov
    r.pixel, r.w, r.v, r.pos, r.lo, r.wsum, r.count = pixel, stream[:, 5].astype(F64), V, POS, LO, wsum, count
    return r


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


def bound_terms(r):
    """-> (A, B, touched), each [N, D]: the bound of a bin is A U + B; touched: some sample of the pixel touches the bin"""
    nbins, N, D, n = r.nbins, r.hist.shape[0], r.hist.shape[1], r.pixel.size
    m = max(nbins - 2, 1)
    A, B, touched = np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, D), bool)
    u = ulp32(r.v)                                                    # [n, 3]
    J = np.rint(r.pos).astype(np.int64)
    near = (np.abs(r.pos - J) <= m * NEAR_ULPS * u) & (J <= nbins - 2)
    rows, w = np.arange(n), np.abs(r.w)
    for ch in range(3):
        T = np.zeros((n, nbins), bool)                                # sample i touches bin b of this channel
        T[rows, r.lo[:, ch]] = True
        T[rows, r.lo[:, ch] + 1] = True
        for d in (-1, 0, 1):
            b = J[:, ch] + d
            ok = near[:, ch] & (b >= 0) & (b <= nbins - 1)
            T[rows[ok], b[ok]] = True
        sl = slice(ch * nbins, (ch + 1) * nbins)
        np.add.at(A[:, sl], r.pixel, (w * m * u[:, ch])[:, None] * T)
        np.add.at(B[:, sl], r.pixel, (w * 3 * EPS)[:, None] * T)
        np.logical_or.at(touched[:, sl], r.pixel, T)
    B += (r.count * EPS * r.wsum)[:, None]
    return A, B, touched


def worst_u(got, r, terms=None):
    """the smallest U for which `got` ([N, D]) obeys the bound, and where: -> (U, (pixel, bin)); inf when a bin is beyond its U-free part
    with no U term to grow"""
    A, B, _ = terms if terms is not None else bound_terms(r)
    excess = np.abs(np.asarray(got, F64).reshape(r.hist.shape) - r.hist) - B
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(excess <= 0, 0.0, np.where(A > 0, excess / A, np.inf))
    at = np.unravel_index(int(np.argmax(need)), need.shape)
    return float(need[at]), (int(at[0]), int(at[1]))


def describe(r, at):
    """the samples of pixel at[0] in the channel of bin at[1]: for a failure message"""
    p, b = at
    ch = b // r.nbins
    rows = np.flatnonzero(r.pixel == p)
    return "pixel %d channel %d bin %d: samples (w, v, position) %s" % (p, ch, b - ch * r.nbins, [(float(r.w[i]), float(r.v[i, ch]), float(r.pos[i, ch])) for i in rows])
