"""GPU tests of accumulator states (bcd_hip_accum_export / _import / _merge_state / _merge, k_accum_merge; format v1 in
include/bcd_hip.h): the format pins the accumulator's semantics, export / import round trips bit for bit, a merge is one fp32 add per
element, disjoint and sample-parallel splits merge back into the single stream, merges keep stream order across contexts, refused calls
leave the state alone, and the C++ class and raw2bcd front-ends write and read the same bytes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bcd_amd.core as core
import bcd_amd.hip as bh
from test_gpu_accumulator import bits_equal, dev, host, random_samples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW2BCD = os.path.join(ROOT, "bcd_amd", "lib", "raw2bcd")
EINVAL = -1


def planes_of(state):
    return bh.accum_state_planes(state)[1]


def statistics_from_planes(p):
    """acc_statistics (k_accumulate.hip) restated in float32, in its operation order: (ns, mean, cov) in DeepImage layout"""
    f1 = np.float32(1)
    with np.errstate(all="ignore"):
        wsum, w2 = p[0], p[1]
        inv = f1 / wsum
        mean = [inv * p[2 + i] for i in range(3)]
        cv = [p[5 + i] * inv for i in range(6)]
        cv[0] = cv[0] - mean[0] * mean[0]
        cv[1] = cv[1] - mean[1] * mean[1]
        cv[2] = cv[2] - mean[2] * mean[2]
        cv[3] = cv[3] - mean[1] * mean[2]
        cv[4] = cv[4] - mean[0] * mean[2]
        cv[5] = cv[5] - mean[0] * mean[1]
        bias = f1 / (f1 - w2 / (wsum * wsum))
        cov = [c * bias for c in cv]
    return wsum[..., None], np.stack(mean, -1), np.stack(cov, -1)


def feed(acc, rng, W, H, dense_spp=2, scattered=None, dyadic=False):
    """a dense pass over every row and a weighted scattered batch (with out-of-range indices); the tensors are kept alive until the
    caller's next synchronisation"""
    colours = (lambda shape: (rng.integers(0, 128, shape) / 64.0).astype(np.float32)) if dyadic else (lambda shape: random_samples(rng, shape))
    keep = []
    if dense_spp:
        d = dev(colours((H, W, dense_spp, 3)))
        acc.add_dense(d)
        keep.append(d)
    n = scattered if scattered is not None else 3 * W * H
    if n:
        pix = rng.integers(-3, W * H + 3, n).astype(np.int32)
        w = np.ones(n, np.float32) if dyadic else rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
        t = (dev(pix), dev(colours((n, 3))), dev(w))
        acc.add_samples(*t)
        keep.append(t)
    return keep


def snapshot(acc):
    return host(acc.statistics())


def export_equal(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# ---- 1. the format pins the semantics -------------------------------------------------------------------------------------------------

def test_format_pins_the_accumulator_semantics(hipctx):
    W, H = 37, 23
    acc = hipctx.accumulator(W, H)
    st = acc.export_state()
    assert st.dtype == np.uint8 and st.size == 64 + 4 * 71 * W * H == acc.state_bytes()
    info, planes = bh.accum_state_planes(st)
    assert (info["magic"], info["version"], info["header_bytes"], info["width"], info["height"], info["nb_bins"], info["nb_planes"]) == \
        (b"BCDACCST", 1, 64, W, H, 20, 71)
    assert bits_equal(np.float32(info["gamma"]), np.float32(2.2)) and info["max_value"] == 2.5
    assert (info["samples_added"], info["dropped"]) == (0, 0)
    assert not np.any(planes.view(np.uint32))                     # a fresh accumulator: every plane +0
    assert not np.any(st[56:64])                                  # reserved
    rng = np.random.default_rng(1)
    keep = feed(acc, rng, W, H)
    st = acc.export_state()
    info, planes = bh.accum_state_planes(st)
    ns, mean, cov, hist = snapshot(acc)
    assert (info["samples_added"], info["dropped"]) == acc.info() and info["dropped"] > 0
    assert bits_equal(planes[0], ns[..., 0])                      # plane 0 is nSamples
    rns, rmean, rcov = statistics_from_planes(planes)
    assert bits_equal(rns, ns) and bits_equal(rmean, mean) and bits_equal(rcov, cov)
    assert bits_equal(planes[11:].transpose(1, 2, 0), hist)       # the bins channel-major, as the snapshot interleaves them
    assert np.all(planes[0] > 0)
    del keep
    acc.close()


# ---- 2. round trip --------------------------------------------------------------------------------------------------------------------

def test_export_import_round_trip(hipctx):
    W, H = 41, 19
    rng = np.random.default_rng(2)
    a, b = hipctx.accumulator(W, H), hipctx.accumulator(W, H, capacity=1000)
    k = feed(a, rng, W, H)
    sa = a.export_state()
    feed(b, np.random.default_rng(99), W, H)                      # (replaced entirely)
    b.import_state(sa)
    assert export_equal(b.export_state(), sa)
    for x, y in zip(snapshot(a), snapshot(b)):
        assert bits_equal(x, y)
    assert a.info() == b.info()
    pa, pb = a.plan(W * H, offset=3, error=True), b.plan(W * H, offset=3, error=True)
    assert np.array_equal(pa[0].cpu().numpy(), pb[0].cpu().numpy()) and np.array_equal(pa[1].cpu().numpy(), pb[1].cpu().numpy())
    assert bits_equal(pa[2].cpu().numpy(), pb[2].cpu().numpy()) and pa[3] == pb[3]
    r1, r2 = np.random.default_rng(3), np.random.default_rng(3)   # the same further batches keep them identical
    k += feed(a, r1, W, H, dense_spp=1) + feed(b, r2, W, H, dense_spp=1)
    assert export_equal(a.export_state(), b.export_state())
    b.import_state(bytes(sa))                                     # any bytes-like buffer
    assert export_equal(b.export_state(), sa)
    a.close()
    b.close()


# ---- 3. merge ---------------------------------------------------------------------------------------------------------------------------

def test_merge_is_one_add_per_element(hipctx):
    W, H = 29, 31
    dst, src, via = hipctx.accumulator(W, H), hipctx.accumulator(W, H), hipctx.accumulator(W, H)
    k = feed(dst, np.random.default_rng(4), W, H) + feed(src, np.random.default_rng(5), W, H, dense_spp=3)
    d0, s0 = dst.export_state(), src.export_state()
    dst.merge(src)
    d1 = dst.export_state()
    assert export_equal(src.export_state(), s0)                   # the source is not changed
    assert bits_equal(planes_of(d1), planes_of(d0) + planes_of(s0))    # float32 + float32: one IEEE add per element
    i0, i1, si = bh.accum_state_info(d0), bh.accum_state_info(d1), bh.accum_state_info(s0)
    assert (i1["samples_added"], i1["dropped"]) == (i0["samples_added"] + si["samples_added"], i0["dropped"] + si["dropped"])
    assert dst.info() == (i1["samples_added"], i1["dropped"])
    via.import_state(d0)
    via.merge_state(s0)                                           # the host path gives the same bytes
    assert export_equal(via.export_state(), d1)
    src.import_state(d0)                                          # B into A has the bits of A into B
    via.import_state(s0)
    via.merge(src)
    assert export_equal(via.export_state(), d1)
    for a in (dst, src, via):
        a.close()


def test_merge_at_a_multi_chunk_size(hipctx):
    """1920 x 1080 x 20 bins: 589 MB, about 9 staging chunks of 64 MiB; the device merge, the host merge_state and the chunked copy path of
    a cross-device merge (forced on one device) give the same bytes, and the planes are the float32 sums"""
    W, H = 1920, 1080
    a, b = hipctx.accumulator(W, H), hipctx.accumulator(W, H)
    k = feed(a, np.random.default_rng(6), W, H, dense_spp=1, scattered=1 << 20) + feed(b, np.random.default_rng(7), W, H, dense_spp=1, scattered=0)
    sa, sb = a.export_state(), b.export_state()
    assert sa.size == 64 + 4 * 71 * W * H > 8 * (64 << 20)
    c = hipctx.accumulator(W, H)
    c.import_state(sa)
    assert export_equal(c.export_state(), sa)                     # a round trip through the chunks
    c.merge_state(sb)
    sc = c.export_state()
    assert bits_equal(planes_of(sc), planes_of(sa) + planes_of(sb))
    a.merge(b)
    assert export_equal(a.export_state(), sc)
    c.import_state(sa)
    os.environ["BCD_HIP_ACCUM_MERGE_COPY"] = "1"
    try:
        c.merge(b)
    finally:
        del os.environ["BCD_HIP_ACCUM_MERGE_COPY"]
    assert export_equal(c.export_state(), sc)
    assert export_equal(b.export_state(), sb)
    for x in (a, b, c):
        x.close()


# ---- 4. / 5. splits -------------------------------------------------------------------------------------------------------------------

def test_disjoint_split_by_rows_is_exact(hipctx):
    """alternate rows to A and B through scattered adds, in one stream's order: the merge equals the single accumulator bit for bit
    (x + (+0) == x for every sum)"""
    W, H = 45, 26
    rng = np.random.default_rng(8)
    n = 6 * W * H
    pix = rng.integers(0, W * H, n).astype(np.int32)
    rgb = random_samples(rng, (n, 3))
    w = rng.choice(np.array([0.5, 1.0, 3.0], np.float32), n)
    even = (pix // W) % 2 == 0
    one, a, b = hipctx.accumulator(W, H), hipctx.accumulator(W, H), hipctx.accumulator(W, H)
    t = [(dev(pix[m]), dev(rgb[m]), dev(w[m])) for m in (np.ones(n, bool), even, ~even)]
    for acc, args in zip((one, a, b), t):
        acc.add_samples(*args)
    a.merge(b)
    assert export_equal(a.export_state(), one.export_state())
    for x, y in zip(snapshot(a), snapshot(one)):
        assert bits_equal(x, y)
    for x in (one, a, b):
        x.close()


def test_sample_parallel_split(hipctx):
    """each pixel's first k samples to A, the rest to B (two renders of one frame with different seeds), merged"""
    W, H, spp, k = 40, 30, 7, 3
    for dyadic in (False, True):
        rng = np.random.default_rng(9)
        s = (rng.integers(0, 128, (H, W, spp, 3)) / 64.0).astype(np.float32) if dyadic else random_samples(rng, (H, W, spp, 3))
        one, a, b = hipctx.accumulator(W, H), hipctx.accumulator(W, H), hipctx.accumulator(W, H)
        t = [dev(s), dev(np.ascontiguousarray(s[:, :, :k])), dev(np.ascontiguousarray(s[:, :, k:]))]
        one.add_dense(t[0])
        a.add_dense(t[1])
        b.add_dense(t[2])
        sa, sb = a.export_state(), b.export_state()
        a.merge(b)
        got, want = snapshot(a), snapshot(one)
        assert np.array_equal(got[0], want[0])                    # unit weights: nSamples exact
        assert a.info() == one.info() == (W * H * spp, 0)
        for g, w_ in zip(got[1:], want[1:]):                      # mean, covariance, histograms: another summation order
            assert float(np.max(np.abs(g - w_))) <= 1e-5 * max(1.0, float(np.max(np.abs(w_))))
        if dyadic:                                                # multiples of 1/64: weight, colour and moment sums are exact
            assert bits_equal(planes_of(a.export_state())[:11], planes_of(one.export_state())[:11])
            assert bits_equal(got[1], want[1]) and bits_equal(got[2], want[2])
            # the merged snapshot denoises like an accumulator imported from the summed state: the same inputs bit for bit
            summed = sa.copy()
            planes_of(summed)[:] = planes_of(sa) + planes_of(sb)
            summed[40:48] = np.frombuffer(struct.pack("<q", W * H * spp), np.uint8)
            c = hipctx.accumulator(W, H)
            c.import_state(summed)
            sc = host(c.statistics())
            for x, y in zip(got, sc):
                assert bits_equal(x, y)
            prm = bh.default_params(m=1.0, random_order=1, seed=5)
            outs = []
            for acc in (a, c):
                ns, mean, cov, hist = acc.statistics()
                hipctx.synchronize()
                outs.append(hipctx.denoise(mean, ns, hist, cov, 2, prm).cpu().numpy())
            # (the denoiser's aggregation uses float atomics, so equal inputs agree to its own run-to-run round-off)
            assert np.all(np.isfinite(outs[0])) and float(np.max(np.abs(outs[0] - outs[1]))) <= 1e-5 * max(1.0, float(np.max(np.abs(outs[0]))))
            c.close()
        for x in (one, a, b):
            x.close()


# ---- 6. stream order across contexts ---------------------------------------------------------------------------------------------------

def test_merge_keeps_stream_order_across_contexts(hipctx):
    """dst and src on two contexts of device 0, each with its own stream: an add enqueued on src, then merge without a synchronisation,
    then another add on src -- dst receives src after the first add only"""
    W, H = 1920, 270
    c1, c2 = bh.Context(0), bh.Context(0)
    dst, src, ref = c1.accumulator(W, H), c2.accumulator(W, H), hipctx.accumulator(W, H)
    rng = np.random.default_rng(10)
    k = feed(dst, rng, W, H, dense_spp=1, scattered=0)
    first = dev(random_samples(rng, (H, W, 8, 3)))               # a long pass: the merge must wait for it
    second = dev(random_samples(rng, (H, W, 8, 3)))
    d0 = dst.export_state()
    ref.add_dense(first)
    want = planes_of(d0) + planes_of(ref.export_state())
    src.add_dense(first)
    dst.merge(src)
    src.add_dense(second)                                         # must not reach dst
    got = dst.export_state()
    assert bits_equal(planes_of(got), want)
    assert bh.accum_state_info(got)["samples_added"] == W * H * 9
    src.close()
    dst.close()
    ref.close()
    c2.close()
    c1.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_untouched(hipctx):
    W, H = 23, 17
    L = bh.lib()
    acc = hipctx.accumulator(W, H)
    k = feed(acc, np.random.default_rng(11), W, H)
    good = acc.export_state()
    others = [hipctx.accumulator(W + 1, H), hipctx.accumulator(W, H + 1), hipctx.accumulator(W, H, nbins=16),
              hipctx.accumulator(W, H, gamma=2.0), hipctx.accumulator(W, H, maxval=float(np.nextafter(np.float32(2.5), np.float32(3))))]

    def mutated(offset, value):
        s = good.copy()
        s[offset:offset + len(value)] = np.frombuffer(value, np.uint8)
        return s
    bad_states = [o.export_state() for o in others] + [
        mutated(0, b"BCDACCSX"), mutated(8, struct.pack("<I", 2)), mutated(56, b"\1"), mutated(12, struct.pack("<I", 65)),
        good[:-4].copy(), np.concatenate([good, np.zeros(4, np.uint8)]), good[:64].copy(), mutated(40, struct.pack("<q", -1))]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for s in bad_states:
        for fn in (L.bcd_hip_accum_import, L.bcd_hip_accum_merge_state):
            assert fn(acc.h, ptr(s), s.size) == EINVAL
            assert export_equal(acc.export_state(), good)
    for o in others + [acc]:                                      # mismatched accumulators, and dst == src
        assert L.bcd_hip_accum_merge(acc.h, o.h) == EINVAL
        assert export_equal(acc.export_state(), good)
    assert L.bcd_hip_accum_import(acc.h, None, good.size) == EINVAL
    assert L.bcd_hip_accum_merge_state(acc.h, None, good.size) == EINVAL
    assert L.bcd_hip_accum_merge(acc.h, None) == EINVAL and L.bcd_hip_accum_merge(None, acc.h) == EINVAL
    assert L.bcd_hip_accum_export(acc.h, None, good.size) == EINVAL and L.bcd_hip_accum_export(None, ptr(good), good.size) == EINVAL
    small = np.zeros(good.size - 1, np.uint8)
    assert L.bcd_hip_accum_export(acc.h, ptr(small), small.size) == EINVAL and not small.any()
    assert L.bcd_hip_accum_state_bytes(acc.h, None) == EINVAL and L.bcd_hip_accum_state_bytes(None, None) == EINVAL
    with pytest.raises(bh.BcdHipError, match="another frame size"):
        acc.import_state(bad_states[0])
    assert export_equal(acc.export_state(), good)
    acc.merge_state(good)                                         # the next valid calls succeed
    assert bits_equal(planes_of(acc.export_state()), planes_of(good) + planes_of(good))
    acc.import_state(good)
    assert export_equal(acc.export_state(), good)
    for o in others + [acc]:
        o.close()


# ---- 8. the C++ class ---------------------------------------------------------------------------------------------------------------

def stream6(rng, W, H, n):
    """(n, 6) (line, col, r, g, b, w) with a few samples outside the frame"""
    line, col = rng.integers(-1, H + 1, n), rng.integers(0, W, n)
    return np.concatenate([line[:, None], col[:, None], random_samples(rng, (n, 3)), rng.choice(np.array([0.5, 1.0, 2.0]), n)[:, None]],
                          1).astype(np.float32)


def test_cpp_class_save_load_merge(hipctx, tmp_path):
    W, H = 33, 21
    rng = np.random.default_rng(12)
    s1, s2 = stream6(rng, W, H, 5 * W * H), stream6(rng, W, H, 4 * W * H)
    py = hipctx.accumulator(W, H)                                 # the same streams through the Python binding
    valid = lambda s: (s[:, 0] >= 0) & (s[:, 0] < H)
    for s in (s1,):
        pix = np.where(valid(s), s[:, 0].astype(np.int64) * W + s[:, 1].astype(np.int64), -1).astype(np.int32)
        t = (dev(pix), dev(np.ascontiguousarray(s[:, 2:5])), dev(np.ascontiguousarray(s[:, 5])))
        py.add_samples(*t)
    a, b, c = core.DeviceAccumulator(W, H), core.DeviceAccumulator(W, H), core.DeviceAccumulator(W, H)
    a.add(s1)                                                     # (left in the class's host batch: save flushes it)
    fa = tmp_path / "a.bcdacc"
    a.save_state(fa)
    pa = py.export_state()
    assert np.array_equal(np.fromfile(fa, np.uint8), pa)          # the file is the Python export
    assert np.array_equal(a.export_state(), pa)
    c.load_state(fa)
    assert np.array_equal(c.export_state(), pa)
    b.add(s2)
    sb = b.export_state()
    fb = tmp_path / "b.bcdacc"
    b.save_state(fb)
    a.merge(b)                                                    # merge
    want = planes_of(pa) + planes_of(sb)
    got = a.export_state()
    assert bits_equal(planes_of(got), want)
    c.merge_state(fb)                                             # mergeState
    assert np.array_equal(c.export_state(), got)
    stats, counts = c.statistics()
    assert counts == (bh.accum_state_info(got)["samples_added"], bh.accum_state_info(got)["dropped"]) and counts[1] > 0
    bad = tmp_path / "bad.bcdacc"
    bad.write_bytes(bytes(pa[:-8]))
    with pytest.raises(RuntimeError, match="bad.bcdacc"):
        c.load_state(bad)
    with pytest.raises(RuntimeError, match="cannot open"):
        c.merge_state(tmp_path / "missing.bcdacc")
    assert np.array_equal(c.export_state(), got)                  # still usable, unchanged
    other = core.DeviceAccumulator(W + 2, H)
    with pytest.raises(RuntimeError):
        c.merge(other)
    x, y, z = core.DeviceAccumulator(W, H), core.DeviceAccumulator(W, H), core.DeviceAccumulator(W, H)
    x.add(s2[:100])                                               # pending on the source side: merge applies it first
    y.merge(x)
    assert np.array_equal(y.export_state(), x.export_state())
    z.add(s1[:50])                                                # pending on the destination side too
    z.merge(x)
    w_ = core.DeviceAccumulator(W, H)
    w_.add(s1[:50])
    w_.export_state()                                             # (flushes)
    w_.merge(x)
    assert np.array_equal(z.export_state(), w_.export_state())
    for q in (a, b, c, other, x, y, z, w_):
        q.close()
    py.close()


# ---- 9. raw2bcd ---------------------------------------------------------------------------------------------------------------------

def write_raw(path, samples):
    H, W, spp, ch = samples.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", 1, W, H, spp, ch))
        f.write(np.ascontiguousarray(samples, np.float32).tobytes())


def raw2bcd(*args):
    r = subprocess.run([RAW2BCD] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def outputs(prefix):
    p = str(prefix)
    return core.read_exr(p + ".exr", False), core.read_exr(p + "_cov.exr", True), core.read_exr(p + "_hist.exr", True)


def test_raw2bcd_save_and_merge_states(hipctx, tmp_path):
    W, H = 27, 14
    for dyadic in (False, True):
        rng = np.random.default_rng(13)
        mk = (lambda shape: (rng.integers(0, 128, shape) / 64.0).astype(np.float32)) if dyadic else (lambda shape: random_samples(rng, shape))
        sa, sb = mk((H, W, 3, 4)), mk((H, W, 2, 4))
        d = tmp_path / ("dyadic" if dyadic else "random")
        d.mkdir()
        write_raw(d / "a.raw", sa)
        write_raw(d / "b.raw", sb)
        raw2bcd("--save-state", d / "a.bcdacc", d / "a.raw", d / "outA")
        raw2bcd("--save-state", d / "b.bcdacc", d / "b.raw", d / "outB")
        raw2bcd("--save-state", d / "s.bcdacc", "--merge-state", d / "a.bcdacc", "--merge-state", d / "b.bcdacc", d / "states")
        raw2bcd("--merge-state", d / "b.bcdacc", d / "a.raw", d / "mixed", "--save-state", d / "m.bcdacc")
        for x, y in zip(outputs(d / "states"), outputs(d / "mixed")):
            assert bits_equal(x, y)
        st = np.fromfile(d / "s.bcdacc", np.uint8)
        assert np.array_equal(st, np.fromfile(d / "m.bcdacc", np.uint8))
        a_st, b_st = np.fromfile(d / "a.bcdacc", np.uint8), np.fromfile(d / "b.bcdacc", np.uint8)
        assert bits_equal(planes_of(st), planes_of(a_st) + planes_of(b_st))
        assert bh.accum_state_info(st)["samples_added"] == W * H * 5
        # the state raw2bcd saves is the one the Python accumulator exports for the same passes
        acc = hipctx.accumulator(W, H)
        t = dev(sa)
        acc.add_dense(t)
        assert np.array_equal(acc.export_state(), a_st)
        acc.close()
        if dyadic:                                                # the concatenated samples in one file: mean and covariance exact
            write_raw(d / "ab.raw", np.concatenate([sa, sb], 2))
            raw2bcd(d / "ab.raw", d / "single")
            one, merged = outputs(d / "single"), outputs(d / "states")
            assert bits_equal(one[0], merged[0]) and bits_equal(one[1], merged[1])
            assert bits_equal(one[2][..., -1], merged[2][..., -1])     # nSamples, the last channel of _hist


# ---- 10. two GPUs -------------------------------------------------------------------------------------------------------------------

def test_cross_device_merge_equals_same_device_merge(hipctx):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    W, H = 640, 360
    c1 = bh.Context(1)
    a, b, src = hipctx.accumulator(W, H), hipctx.accumulator(W, H), c1.accumulator(W, H)
    k = feed(a, np.random.default_rng(14), W, H)
    s = feed(b, np.random.default_rng(15), W, H)
    sb = b.export_state()
    src.import_state(sb)
    a0 = a.export_state()
    a.merge(b)                                                    # same device
    want = a.export_state()
    a.import_state(a0)
    a.merge(src)                                                  # from device 1
    assert export_equal(a.export_state(), want)
    assert export_equal(src.export_state(), sb)
    src.close()
    c1.close()
    a.close()
    b.close()
