"""Host restatement of the accumulator's feature channels (include/bcd_hip.h, bcd_hip_accum_*_features) in NumPy float32, sequential per
pixel in stream order: the sums, the snapshot, the block layout, and the splat through splat_ref.expand.  TEST INFRASTRUCTURE.
tests/test_accum_features_cpu.py pins it to the oracle accumulator (itself pinned to the reference's compiled one): channel k's mean and
unclamped v are mean[0] and cov[0] of an accumulator fed x_k as its first colour channel."""
import struct

import numpy as np

import splat_ref

F32 = np.float32
MAGIC = b"BCDACCFT"
HEADER_BYTES = 64


class Sums:
    """the running sums of a W x H frame with F channels: wsum, w2sum (N,), the beauty's; planes (F, 2, N): per channel s1, then s2"""

    def __init__(self, W, H, F):
        self.W, self.H, self.F, self.N = W, H, F, W * H
        self.wsum, self.w2sum = np.zeros(self.N, F32), np.zeros(self.N, F32)
        self.planes = np.zeros((F, 2, self.N), F32)

    def add(self, pixel, x, w=None):
        """pixel (n,) indices line * W + col, all inside the frame; x (n, F); w (n,) or None (all 1): every pixel's contributions in the
        order of the stream, one float32 operation after the other.  Round r applies the r-th contribution of every pixel that has one."""
        pixel = np.asarray(pixel, np.int64).reshape(-1)
        n = pixel.shape[0]
        x = np.ascontiguousarray(x, F32).reshape(n, self.F)
        w = np.ones(n, F32) if w is None else np.ascontiguousarray(w, F32).reshape(n)
        assert n == 0 or (pixel.min() >= 0 and pixel.max() < self.N)
        order = np.argsort(pixel, kind="stable")
        p = pixel[order]
        first = np.r_[0, np.flatnonzero(np.diff(p)) + 1] if n else np.zeros(0, np.int64)
        rank = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(int(rank.max()) + 1 if n else 0):
                e = order[rank == r]
                q, wr, xr = pixel[e], w[e], x[e]
                self.wsum[q] += wr
                self.w2sum[q] += wr * wr
                wx = wr[:, None] * xr                               # w * x
                self.planes[:, 0, q] += wx.T
                self.planes[:, 1, q] += (wx * xr).T                 # (w * x) * x
        assert self.planes.dtype == F32 and self.wsum.dtype == F32
        return self

    def add_dense(self, x, w=None, row0=0):
        """x (rows, W, k, F), w (rows, W, k) or None: pixels in order, each pixel's k samples in order"""
        rows, W, k, F = x.shape
        assert W == self.W and F == self.F
        pix = np.repeat(np.arange(row0 * W, (row0 + rows) * W), k)
        return self.add(pix, x.reshape(-1, F), None if w is None else w.reshape(-1))

    def add_scattered(self, pixel, x, w=None):
        """as the device's scattered add: indices outside [0, N) are dropped -> number dropped"""
        pixel = np.asarray(pixel, np.int64)
        ok = (pixel >= 0) & (pixel < self.N)
        self.add(pixel[ok], np.asarray(x, F32)[ok], None if w is None else np.asarray(w, F32)[ok])
        return int((~ok).sum())

    def add_splatted(self, xy, x, w, rx, ry, table):
        """as the device's splatted add: every sample to the pixels of its footprint with w * f -> (samples added, dropped)"""
        pix, e, wf, added, dropped = expand(xy, w, self.W, self.H, rx, ry, table)
        self.add(pix, np.asarray(x, F32).reshape(-1, self.F)[e], wf)
        return added, dropped

    def snapshot(self):
        return snapshot(self.wsum, self.w2sum, self.planes, self.W, self.H)

    def block(self):
        return block(self.planes, self.W, self.H)


def expand(xy, w, W, H, rx, ry, table):
    """the stream of splat_ref.expand as (pixel, sample index, w * f), with its counts: the sample index rides in the red channel"""
    n = np.asarray(xy).reshape(-1, 2).shape[0]
    assert n < 1 << 24
    tag = np.zeros((n, 3), F32)
    tag[:, 0] = np.arange(n)
    s, added, dropped = splat_ref.expand(xy, tag, w, W, H, rx, ry, table)
    pix = s[:, 0].astype(np.int64) * W + s[:, 1].astype(np.int64)
    return pix, s[:, 2].astype(np.int64), np.ascontiguousarray(s[:, 5]), added, dropped


def snapshot(wsum, w2sum, planes, W, H):
    """-> dict of (H, W, F) float32 images: mean, v (the unclamped bias-corrected variance, cov[0] of the accumulator), vm (the variance of
    the weighted mean before the clamp) and variance (what the device stores); the formulas of include/bcd_hip.h, one operation each"""
    F = planes.shape[0]
    wsum, w2sum = np.asarray(wsum, F32), np.asarray(w2sum, F32)
    s1, s2 = planes[:, 0], planes[:, 1]
    with np.errstate(all="ignore"):
        inv = F32(1) / wsum
        mean = inv * s1
        cv = s2 * inv
        cv = cv - mean * mean
        r = w2sum / (wsum * wsum)
        bias = F32(1) / (F32(1) - r)
        v = cv * bias
        vm = v * r
        var = np.where(vm > 0, vm, F32(0)).astype(F32)
    img = lambda a: np.ascontiguousarray(a.reshape(F, H, W).transpose(1, 2, 0))
    out = dict(mean=img(mean), v=img(v), vm=img(vm), variance=img(var))
    assert all(a.dtype == F32 for a in out.values())
    return out


def header(W, H, F, magic=MAGIC, version=1, header_bytes=HEADER_BYTES, nb_planes=None, reserved=bytes(32)):
    return struct.pack("<8sIIiiiI32s", magic, version, header_bytes, W, H, F, 2 * F if nb_planes is None else nb_planes, reserved)


def block(planes, W, H):
    """the serialised feature block of (F, 2, N) planes as a uint8 array: 64 + 8 F W H bytes"""
    F = planes.shape[0]
    b = header(W, H, F) + np.ascontiguousarray(planes, "<f4").tobytes()
    assert len(b) == HEADER_BYTES + 8 * F * W * H
    return np.frombuffer(b, np.uint8).copy()
