"""GPU tests of the pyramid and per-pixel kernels (bcd_amd/csrc/k_pointwise.hip) on every branch of their launchers, bit for bit against the CPU oracle
(NaN matches NaN), on the constructed cases of tests/pyramid_cases.py -- its table says which kernel a case reaches; tests/test_pyramid_cases_cpu.py
holds the cases to what they claim and the oracle to the float32 restatements, whose mutants say which mistakes a passing kernel cannot make.

Every buffer a call reads or writes lies in an allocation of its own between two margins of 64 sentinel words (`Guarded`; the calls go through
bh.lib() where the Context wrapper would allocate the output itself): after each call the margins of all of them are unchanged and the inputs still
hold their bits -- the check that the 32-bit index forms and the tail launch write only what they own.

  downscale_sum / _avg   every size x depth x value family (index, order, nonfinite)
  downscale_cov          every size, sample counts "mixed" and "zero" (nSum / 0, 0 / 0)
  interpolate, merge     every size x depth x family; merge in place (bcd_hip_merge on a guarded copy) and out of place (Context.merge) agree
  finalize               1, 2, 9, 255, 256, 257 pixels; counts 0, 1, 3, 2^24 + 1 on every pixel position modulo four and on the last pixels
  zero_bad_values        the special vector at lengths 1 (every special on its own), 255, 256, 257: exact bits out
  pixel_cov, scale_begin the same pixel counts; the accumulators handed over filled with ones come back zero in every bit
  misaligned views       input, output or both one float off a 16-byte boundary: the launchers must take the scalar kernels (a vector access to such
                         an address is never issued: the guard is in the launcher, the tests only pass the views) and give the aligned call's bits
  layer-batched forms    tests/test_gpu_layers_stage.py runs them at 4x4, 5x7, 64x48, 97x65 and on random sizes from 4x4 up, without margins; here:
                         the tiny sizes below 4 and the three block-boundary sizes, 1 and 16 layers, against the oracle directly, with margins
  frame-level link       a two-scale frame whose histograms have 5 bins per channel (D = 15: the per-value k_downscale<0> builds the histogram
                         level) and one with 4 (D = 12: k_downscale4<0>, Q = 3), against the oracle's multiscale run at the suite's TOL"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import pyramid_cases as pc
from test_gpu_parity import TOL, bits_equal, rel_linf

pytestmark = pytest.mark.gpu

MARGIN = 64                      # sentinel words before and after every buffer (256 bytes: the payload stays 16-byte aligned)
SENTINEL = 0x5A5AA5A5            # as a float32: 1.5e16, as an int32: 1515890085 -- nothing a kernel here writes
_VP = C.c_void_p
_I32 = C.POINTER(C.c_int32)


class Guarded:
    """a device buffer of `shape` between two sentinel margins; shift: floats by which the payload is moved off its 16-byte boundary"""

    def __init__(self, shape, init=None, dtype=np.float32, shift=0, fill=None):
        import torch
        n = int(np.prod(shape))
        self.raw = torch.full((MARGIN + shift + n + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi = MARGIN + shift, MARGIN + shift + n
        self.t = self.raw[self.lo:self.hi].view(torch.float32 if dtype == np.float32 else torch.int32).view(tuple(shape))
        self.init = None if init is None else np.ascontiguousarray(init, dtype)
        if init is not None:
            assert self.init.shape == tuple(shape)
            self.t.copy_(torch.from_numpy(self.init))
        elif fill is not None:
            self.t.fill_(fill)

    @property
    def p(self):
        return _VP(self.t.data_ptr())

    def numpy(self):
        return self.t.cpu().numpy()

    def intact(self):
        """margins unchanged, and -- for an input -- the payload too"""
        ok = bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())
        if self.init is not None:
            ok = ok and np.array_equal(self.numpy().view(np.uint32), self.init.view(np.uint32))
        return ok


def call(ctx, name, *args):
    import bcd_amd.hip as bh
    ctx.torch.cuda.synchronize()                     # (the fills and uploads ran on torch's stream)
    ctx._chk(getattr(bh.lib(), name)(ctx.h, *args))
    ctx.torch.cuda.synchronize()


def all_intact(*bufs):
    return all(b.intact() for b in bufs)


_oracle_results = {}


def want(op, key, inputs):
    """the oracle's result of a case, computed once"""
    if (op, key) not in _oracle_results:
        o = ol.oracle_ops()
        _oracle_results[(op, key)] = {"dsum": o["dsum"], "davg": o["davg"], "dcov": o["dcov"], "interp": o["interp"], "merge": o["merge"]}[op](*inputs)
    return _oracle_results[(op, key)]


def oracle_pixel_cov(cov, ns):
    out = np.empty_like(cov)
    ol.oracle().bcdo_pixel_cov_from_sample_cov(ol._fp(cov), ol._fp(ns), ns.size, 1, ol._fp(out))
    return out


def oracle_finalize(s, cnt):
    out = np.empty_like(s)
    ol.oracle().bcdo_finalize(ol._fp(s), cnt.ctypes.data_as(_I32), C.c_int64(cnt.size), ol._fp(out))
    return out


def run_downscale(ctx, mode, a, shift_in=0, shift_out=0):
    H, W, D = a.shape
    src, dst = Guarded(a.shape, a, shift=shift_in), Guarded((H // 2, W // 2, D), shift=shift_out)
    call(ctx, "bcd_hip_downscale_sum" if mode == "dsum" else "bcd_hip_downscale_avg", src.p, W, H, D, dst.p)
    assert all_intact(src, dst), (mode, W, H, D, shift_in, shift_out)
    return dst.numpy()


# ---- downscale --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", pc.DEPTHS)
def test_downscale_sum_and_avg_on_every_size_and_family(hipctx, D):
    for (W, H) in pc.SIZES:
        for fam in pc.FAMILIES:
            a = pc.level(fam, W, H, D)
            for mode in ("dsum", "davg"):
                assert bits_equal(run_downscale(hipctx, mode, a), want(mode, (fam, W, H, D), (a,))), (mode, fam, W, H, D)


@pytest.mark.parametrize("kind", pc.COUNT_KINDS)
def test_downscale_cov_on_every_size(hipctx, kind):
    for (W, H) in pc.SIZES:
        cov, ns = pc.covariances(kind, W, H)
        g_cov, g_ns, out = Guarded(cov.shape, cov), Guarded(ns.shape, ns), Guarded((H // 2, W // 2, 6))
        call(hipctx, "bcd_hip_downscale_cov", g_cov.p, g_ns.p, W, H, out.p)
        assert all_intact(g_cov, g_ns, out), (W, H)
        assert bits_equal(out.numpy(), want("dcov", (kind, W, H), (cov, ns))), (kind, W, H)


# ---- interpolate and merge --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", pc.DEPTHS)
def test_interpolate_and_merge_on_every_size_and_family(hipctx, D):
    import torch
    for (W, H) in pc.SIZES:
        h, w = H // 2, W // 2
        for fam in pc.FAMILIES:
            lo = pc.coarse(fam, W, H, D)
            g_lo, out = Guarded(lo.shape, lo), Guarded((H, W, D))
            call(hipctx, "bcd_hip_interpolate", g_lo.p, w, h, D, out.p, W, H)
            assert all_intact(g_lo, out), (fam, W, H, D)
            assert bits_equal(out.numpy(), want("interp", (fam, W, H, D), (lo, H, W))), ("interpolate", fam, W, H, D)
            hi, lo = pc.merge_pair(fam, W, H, D)
            expect = want("merge", (fam, W, H, D), (hi, lo))
            g_lo, g_hi = Guarded(lo.shape, lo), Guarded(hi.shape)
            g_hi.t.copy_(torch.from_numpy(hi))
            call(hipctx, "bcd_hip_merge", g_hi.p, W, H, g_lo.p, D)                    # merge_: in place
            assert all_intact(g_lo, g_hi), (fam, W, H, D)
            assert bits_equal(g_hi.numpy(), expect), ("merge_", fam, W, H, D)
            d_hi, d_lo = torch.from_numpy(hi).cuda(), torch.from_numpy(lo).cuda()
            assert bits_equal(hipctx.merge(d_hi, d_lo).cpu().numpy(), expect), ("merge", fam, W, H, D)
            assert bits_equal(d_hi.cpu().numpy(), hi)                                  # out of place: the input keeps its bits


# ---- the flat per-pixel kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", pc.FLAT)
def test_finalize_on_awkward_counts(hipctx, npix):
    for turn in range(4):
        s, cnt = pc.finalize_case(npix, turn)
        g_s, g_c, out = Guarded(s.shape, s), Guarded(cnt.shape, cnt, dtype=np.int32), Guarded(s.shape)
        call(hipctx, "bcd_hip_finalize", g_s.p, g_c.p, C.c_int64(npix), out.p)
        assert all_intact(g_s, g_c, out), (npix, turn)
        assert bits_equal(out.numpy(), oracle_finalize(s, cnt)), (npix, turn)


@pytest.mark.parametrize("n", pc.ZERO_BAD_LENGTHS)
def test_zero_bad_values_exact_bits(hipctx, n):
    for turn in range(pc.ZERO_BAD_SPECIALS.size if n == 1 else 3):
        bits = pc.zero_bad_vector(n, turn)
        expect = bits.copy()
        ol.oracle().bcdo_zero_bad_values(expect.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(n))
        g = Guarded((n,), dtype=np.int32)
        g.t.copy_(hipctx.torch.from_numpy(bits.view(np.int32)))
        call(hipctx, "bcd_hip_zero_bad_values", g.p, C.c_int64(n))
        got = g.numpy().view(np.uint32)
        assert g.intact(), (n, turn)
        assert np.array_equal(got, expect), (n, turn, [hex(v) for v in bits[got != expect][:4]])       # NaN -> +0, -0.0 kept, a negative denormal -> +0
        kept = expect == bits
        assert np.array_equal(got[kept], bits[kept]) and np.all(got[~kept] == 0)                         # every value the oracle keeps is unchanged


def run_scale_begin(ctx, cov, ns, shifts=(0, 0, 0, 0, 0)):
    """-> (per-pixel covariances, sum, count) of bcd_hip_scale_begin on W = npix, H = 1; shifts: of cov, ns, pixcov, sum, count"""
    n = ns.size
    g_cov, g_ns = Guarded(cov.shape, cov, shift=shifts[0]), Guarded(ns.shape, ns, shift=shifts[1])
    out = Guarded(cov.shape, shift=shifts[2])
    s = Guarded((n, 3), shift=shifts[3], fill=1.0)
    c = Guarded((n,), dtype=np.int32, shift=shifts[4], fill=1)
    call(ctx, "bcd_hip_scale_begin", g_cov.p, g_ns.p, n, 1, out.p, s.p, c.p)
    assert all_intact(g_cov, g_ns, out, s, c), (n, shifts)
    return out.numpy(), s.numpy(), c.numpy()


@pytest.mark.parametrize("npix", pc.FLAT)
def test_pixel_cov_and_scale_begin(hipctx, npix):
    cov, ns = pc.flat_covariances(npix)
    expect = oracle_pixel_cov(cov, ns)
    g_cov, g_ns, out = Guarded(cov.shape, cov), Guarded(ns.shape, ns), Guarded(cov.shape)
    call(hipctx, "bcd_hip_pixel_cov", g_cov.p, g_ns.p, npix, 1, out.p)
    assert all_intact(g_cov, g_ns, out)
    assert bits_equal(out.numpy(), expect)
    pixcov, s, c = run_scale_begin(hipctx, cov, ns)
    assert bits_equal(pixcov, expect)
    assert not s.view(np.uint32).any() and not c.any()                  # zero in every element (+0.0: no bit set), the last pixel of an odd count included


# ---- the alignment guard ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 12, 60])
def test_downscale_of_views_one_float_off_alignment(hipctx, D):
    """depths that are multiples of four take k_downscale4, whose loads and stores are 16 bytes wide, only where both images are 16-byte aligned"""
    for (W, H) in [(2, 2), (5, 4), (33, 32), (35, 33)]:
        for fam in ("order", "nonfinite"):
            a = pc.level(fam, W, H, D)
            for mode in ("dsum", "davg"):
                aligned = run_downscale(hipctx, mode, a)
                assert bits_equal(aligned, want(mode, (fam, W, H, D), (a,)))
                for shifts in ((1, 0), (0, 1), (1, 1), (2, 3)):
                    assert bits_equal(run_downscale(hipctx, mode, a, *shifts), aligned), (mode, fam, W, H, D, shifts)
    # merge averages the (misaligned) fine image into its own aligned scratch
    W, H = 5, 4
    hi, lo = pc.merge_pair("order", W, H, D)
    g_lo, g_hi = Guarded(lo.shape, lo, shift=1), Guarded(hi.shape, shift=1)
    g_hi.t.copy_(hipctx.torch.from_numpy(hi))
    call(hipctx, "bcd_hip_merge", g_hi.p, W, H, g_lo.p, D)
    assert all_intact(g_lo, g_hi) and bits_equal(g_hi.numpy(), want("merge", ("order", W, H, D), (hi, lo)))


@pytest.mark.parametrize("npix", [2, 9, 256, 257])
def test_scale_begin_of_views_one_float_off_alignment(hipctx, npix):
    """k_pixel_cov_clear2 moves the covariances 16 and the counts, sums and counters 8 bytes at a time: any one view off by a float takes the per-value kernel"""
    cov, ns = pc.flat_covariances(npix)
    expect = oracle_pixel_cov(cov, ns)
    for shifts in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (2, 0, 2, 0, 0), (3, 1, 2, 3, 1)):
        pixcov, s, c = run_scale_begin(hipctx, cov, ns, shifts)
        assert bits_equal(pixcov, expect), (npix, shifts)
        assert not s.view(np.uint32).any() and not c.any(), (npix, shifts)


# ---- the layer-batched forms --------------------------------------------------------------------------------------------------------------------------
def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.t.data_ptr() for b in bufs])


@pytest.mark.parametrize("W,H", [(2, 2), (3, 2), (2, 3), (3, 3), (33, 32), (34, 31), (35, 33)])
@pytest.mark.parametrize("L", [1, 16])
def test_layer_batched_forms_at_tiny_and_block_boundary_sizes(hipctx, W, H, L):
    import bcd_amd.hip as bh
    lib = bh.lib()
    o = ol.oracle_ops()
    h, w, npix = H // 2, W // 2, W * H
    scale = [np.float32(2.0 ** ((5 * k) % 17 - 8)) for k in range(L)]              # a magnitude of its own per layer: 2^-8 ... 2^8
    cov0, ns = pc.covariances("zero", W, H)
    hi0, lo0 = pc.merge_pair("order", W, H, 3)
    cnt = pc.finalize_case(npix, 0)[1]
    covs = [cov0 * s * s for s in scale]
    cols = [pc.level("nonfinite" if k == 1 else "order", W, H, 3) * s for k, s in enumerate(scale)]
    his, los = [hi0 * s for s in scale], [lo0 * s for s in scale]
    sums = [pc.finalize_case(npix, k % 4)[0] * s for k, s in enumerate(scale)]
    g_ns, g_cnt = Guarded(ns.shape, ns), Guarded(cnt.shape, cnt, dtype=np.int32)

    g_cov = [Guarded(a.shape, a) for a in covs]
    pixcov, cleared = Guarded((L, npix, 6)), Guarded((L, npix, 3), fill=1.0)
    call(hipctx, "bcd_hip_layers_pixel_cov", _ptrs(g_cov), L, g_ns.p, W, H, pixcov.p, cleared.p)
    assert all_intact(g_ns, pixcov, cleared, *g_cov)
    assert not cleared.numpy().view(np.uint32).any()
    got = pixcov.numpy()
    for k in range(L):
        assert bits_equal(got[k], oracle_pixel_cov(covs[k].reshape(npix, 6), ns.reshape(npix, 1))), ("pixel_cov", k)

    g_sum, outs = [Guarded(a.shape, a) for a in sums], [Guarded((npix, 3)) for _ in range(L)]
    call(hipctx, "bcd_hip_layers_finalize", _ptrs(g_sum), _ptrs(outs), L, g_cnt.p, npix)
    assert all_intact(g_cnt, *g_sum, *outs)
    for k in range(L):
        assert bits_equal(outs[k].numpy(), oracle_finalize(sums[k], cnt)), ("finalize", k)

    g_col, outs = [Guarded(a.shape, a) for a in cols], [Guarded((h, w, 3)) for _ in range(L)]
    call(hipctx, "bcd_hip_layers_downscale_avg", _ptrs(g_col), _ptrs(outs), L, W, H)
    assert all_intact(*g_col, *outs)
    for k in range(L):
        assert bits_equal(outs[k].numpy(), o["davg"](cols[k])), ("downscale_avg", k)

    outs = [Guarded((h, w, 6)) for _ in range(L)]
    call(hipctx, "bcd_hip_layers_downscale_cov", _ptrs(g_cov), _ptrs(outs), L, g_ns.p, W, H)
    assert all_intact(g_ns, *g_cov, *outs)
    for k in range(L):
        assert bits_equal(outs[k].numpy(), o["dcov"](covs[k], ns)), ("downscale_cov", k)

    g_lo, g_hi = [Guarded(a.shape, a) for a in los], [Guarded(a.shape) for a in his]
    for g, a in zip(g_hi, his):
        g.t.copy_(hipctx.torch.from_numpy(a))
    call(hipctx, "bcd_hip_layers_merge", _ptrs(g_hi), _ptrs(g_lo), L, W, H)
    assert all_intact(*g_lo, *g_hi)
    for k in range(L):
        assert bits_equal(g_hi[k].numpy(), o["merge"](his[k], los[k])), ("merge", k)


# ---- the frame-level link ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [5, 4])
def test_two_scale_frame_with_few_bins_against_the_oracle(hipctx, nbins):
    """5 bins per channel: D = 15, neither a multiple of four nor shallow -- the histogram level of the second scale is built by the per-value
    k_downscale<0>; 4 bins: D = 12, k_downscale4<0> with three groups per pixel"""
    import torch
    import bcd_amd.hip as bh
    W, H = 40, 30
    samples, _ = ol.synth_samples(W, H, 16, seed=5, sigma=0.2, spike_prob=0.0)
    ns, col, cov, hist = ol.oracle_ops()["accumulate"](samples, W, H, nbins)
    assert hist.shape == (H, W, 3 * nbins)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (col, ns, hist, cov)]
    assert bits_equal(hipctx.downscale_sum(d[2]).cpu().numpy(), ol.oracle_ops()["dsum"](hist))       # the level the second scale works on
    got = hipctx.denoise(*d, 2, bh.default_params(m=0.0)).cpu().numpy()
    expect = ol.denoise_multiscale(col, ns, hist, cov, 2, ol.params(m=0.0))
    ok = np.isfinite(expect)
    assert np.array_equal(np.isfinite(got), ok)
    assert rel_linf(np.where(ok, got, 0), np.where(ok, expect, 0)) < TOL
