"""CPU tests of the accumulator's feature channels (bcd_hip_accum_*_features): the NumPy restatement tests/accum_features_ref.py against the
oracle accumulator (pinned to the reference's compiled one), the clamp of the variance of the mean, the feature block's header check (host
only), the new prototypes, and the refusals that need no device."""
import ctypes as C
import struct

import numpy as np
import pytest

import accum_features_ref as fr
import bcd_amd.hip as bh
import oracle_lib as ol

F32 = np.float32
EINVAL = -1
W, H = 23, 11


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def oracle(pix, rgb, w):
    s = np.concatenate([(pix // W)[:, None], (pix % W)[:, None], rgb, w[:, None]], 1).astype(F32)
    return ol.oracle_ops()["accumulate"](np.ascontiguousarray(s), W, H)


def assert_pinned(sums, pix, x, w):
    """channels in triples as colours through the oracle accumulator: same pixels, weights and order"""
    snap = sums.snapshot()
    Fc = x.shape[1]
    for k0 in range(0, Fc, 3):
        rgb = np.zeros((x.shape[0], 3), F32)
        n = min(3, Fc - k0)
        rgb[:, :n] = x[:, k0:k0 + n]
        ns, mean, cov, _ = oracle(pix, rgb, w)
        assert bits_equal(ns[..., 0], sums.wsum.reshape(H, W))
        assert bits_equal(snap["mean"][..., k0:k0 + n], mean[..., :n]), "mean of channels %d.." % k0
        assert bits_equal(snap["v"][..., k0:k0 + n], cov[..., :n]), "variance of channels %d.." % k0
    return snap


def test_restatement_equals_the_oracle_on_a_weighted_scattered_stream():
    rng = np.random.default_rng(1)
    n, Fc = 9 * W * H, 7
    pix = rng.integers(0, W * H, n)
    pix[:400] = 5                                             # a long run on one pixel
    x = (rng.standard_normal((n, Fc)) * 0.3 + np.arange(Fc) * 0.2).astype(F32)
    w = rng.choice(np.array([0.25, 1.0, 3.0], F32), n)
    sums = fr.Sums(W, H, Fc).add(pix, x, w)
    snap = assert_pinned(sums, pix, x, w)
    assert np.all(snap["variance"] >= 0) and not np.isnan(snap["variance"]).any()
    pos = snap["vm"] > 0
    assert pos.mean() > 0.95 and bits_equal(snap["variance"][pos], snap["vm"][pos])
    # in two pieces: the sums go on where they stopped
    two = fr.Sums(W, H, Fc).add(pix[:1000], x[:1000], w[:1000]).add(pix[1000:], x[1000:], w[1000:])
    assert bits_equal(two.planes, sums.planes) and bits_equal(two.wsum, sums.wsum) and bits_equal(two.w2sum, sums.w2sum)


def test_restatement_equals_the_oracle_on_an_expanded_splat_stream():
    rng = np.random.default_rng(2)
    n, Fc = 5 * W * H, 4
    xy = np.stack([rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n)], 1).astype(F32)
    xy[7] = (np.nan, 1.0)
    x = rng.random((n, Fc), dtype=F32)
    w = rng.choice(np.array([0.5, 1.0, 2.0], F32), n)
    table = bh.filter_table("gaussian", 1.5, 2.0, 16)
    pix, e, wf, added, dropped = fr.expand(xy, w, W, H, 1.5, 1.5, table)
    assert dropped > 0 and added + dropped == n and len(pix) > 2 * added
    sums = fr.Sums(W, H, Fc)
    assert sums.add_splatted(xy, x, w, 1.5, 1.5, table) == (added, dropped)
    assert_pinned(sums, pix, x[e], wf)


def test_variance_of_the_mean_is_v_over_n_for_unit_weights():
    """vm = v * (w2sum / wsum^2) against v / n: two expressions of one number, within 1 ulp"""
    rng = np.random.default_rng(3)
    n, Fc = 6 * W * H, 3
    pix = np.r_[np.arange(W * H), np.arange(W * H), rng.integers(0, W * H, n - 2 * W * H)]        # two samples or more everywhere
    x = rng.random((n, Fc), dtype=F32)
    sums = fr.Sums(W, H, Fc).add(pix, x)
    assert np.array_equal(sums.wsum, sums.w2sum) and sums.wsum.min() >= 2
    snap = sums.snapshot()
    want = snap["v"] / sums.wsum.reshape(H, W, 1)
    assert want.dtype == F32
    ulp = np.abs(snap["vm"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and np.all(np.sign(snap["vm"]) == np.sign(want))


def test_clamp_cases():
    Fc = 3
    sums = fr.Sums(W, H, Fc)
    one, none, inf, nan, const = 0, 1, 2, 3, 4
    pix = np.array([one] + [inf] * 3 + [nan] * 3 + [const] * 7)
    x = np.full((len(pix), Fc), 0.5, F32)
    x[1:4, 1] = np.inf                                        # an infinite depth
    x[5, 2] = np.nan
    x[7:, 0] = F32(0.1)                                       # a constant channel: s2 / n - mean^2 rounds to either side of 0
    sums.add(pix, x)
    snap = sums.snapshot()
    img = lambda name, p: snap[name].reshape(-1, Fc)[p]
    assert np.array_equal(img("mean", one), x[0]) and np.isnan(img("vm", one)).all() and not img("variance", one).any()          # 0 * inf
    assert np.isnan(img("mean", none)).all() and not img("variance", none).any()
    assert img("mean", inf)[1] == np.inf and np.isnan(img("vm", inf)[1]) and img("variance", inf)[1] == 0 and img("variance", inf)[0] == 0
    assert np.isnan(img("mean", nan)[2]) and img("variance", nan)[2] == 0 and np.isfinite(img("mean", nan)[:2]).all()
    # negative round-off: among constant channels of many values some have v < 0
    vals = np.linspace(0.01, 0.99, 500, dtype=F32)
    many = fr.Sums(500, 1, 1).add(np.repeat(np.arange(500), 7), np.repeat(vals, 7)[:, None])
    s = fr.snapshot(many.wsum, many.w2sum, many.planes, 500, 1)
    assert (s["vm"] < 0).any() and np.all(s["variance"] >= 0) and np.all(s["variance"][s["vm"] < 0] == 0)
    assert not np.signbit(s["variance"]).any() and not np.signbit(snap["variance"]).any()                                        # +0, never -0
    assert img("variance", const)[0] >= 0


# ---- the feature block's header (host only) -----------------------------------------------------------------------------------------------

def info_rc(buf, size=None):
    a = np.frombuffer(bytes(buf), np.uint8)
    h = bh.FeaturesHeader()
    rc = bh.lib().bcd_hip_accum_features_state_info(a.ctypes.data_as(C.c_void_p), a.size if size is None else size, C.byref(h))
    return rc, h


def good_block(Fc=3):
    return bytes(fr.block(np.arange(Fc * 2 * W * H, dtype=F32).reshape(Fc, 2, W * H), W, H))


def test_header_layout_and_a_well_formed_block():
    assert C.sizeof(bh.FeaturesHeader) == 64 == fr.HEADER_BYTES == bh.STATE_HEADER_BYTES
    for Fc in (1, 3, 8):
        b = good_block(Fc)
        assert len(b) == 64 + 8 * Fc * W * H
        rc, h = info_rc(b)
        assert rc == 0 and (bytes(h.magic), h.version, h.header_bytes, h.width, h.height, h.nb_features, h.nb_planes) == (b"BCDACCFT", 1, 64, W, H, Fc, 2 * Fc)
        info, planes = bh.accum_features_state_planes(b)
        assert info["nb_features"] == Fc and planes.shape == (Fc, 2, H, W) and planes[Fc - 1, 1, H - 1, W - 1] == Fc * 2 * W * H - 1
    assert bh.lib().bcd_hip_accum_features_state_info(np.frombuffer(good_block(), np.uint8).ctypes.data_as(C.c_void_p), len(good_block()), None) == 0


def malformed():
    body = good_block()[64:]
    hdr = lambda **kw: fr.header(W, H, 3, **kw) + body
    cases = {
        "magic": hdr(magic=b"BCDACCLY"), "version": hdr(version=2), "header_bytes": hdr(header_bytes=60), "nb_planes": hdr(nb_planes=3),
        "width": fr.header(W + 1, H, 3) + body, "height": fr.header(W, H - 1, 3) + body, "width 0": fr.header(0, H, 3) + body,
        "negative height": fr.header(W, -H, 3) + body, "nb_features": fr.header(W, H, 2) + body,
        "F = 0": fr.header(W, H, 0), "F = 9": fr.header(W, H, 9) + bytes(8 * 9 * W * H),
        "4 bytes short": good_block()[:-4], "4 bytes long": good_block() + bytes(4), "header only": good_block()[:64], "short header": good_block()[:60],
        "reserved first": hdr(reserved=b"\x01" + bytes(31)), "reserved last": hdr(reserved=bytes(31) + b"\x01"), "empty": b"",
    }
    return sorted(cases.items())


@pytest.mark.parametrize("case,buf", malformed())
def test_malformed_blocks_are_refused(case, buf):
    assert info_rc(buf)[0] == EINVAL if len(buf) else bh.lib().bcd_hip_accum_features_state_info(None, 0, None) == EINVAL
    with pytest.raises(ValueError):
        bh.accum_features_state_info(buf)


def test_size_argument_and_the_other_blocks():
    b = good_block()
    assert info_rc(b, len(b) - 4)[0] == EINVAL and info_rc(b, len(b) + 4)[0] == EINVAL and info_rc(b, -1)[0] == EINVAL
    assert bh.lib().bcd_hip_accum_features_state_info(None, len(b), None) == EINVAL
    a = np.frombuffer(b, np.uint8)
    assert bh.lib().bcd_hip_accum_layers_state_info(a.ctypes.data_as(C.c_void_p), a.size, None) == EINVAL           # not a layer block, not a state
    assert bh.lib().bcd_hip_accum_state_info(a.ctypes.data_as(C.c_void_p), a.size, None) == EINVAL


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------

NEW = ["bcd_hip_accum_create_features", "bcd_hip_accum_nb_features", "bcd_hip_accum_add_dense_features", "bcd_hip_accum_add_scattered_features",
       "bcd_hip_accum_add_splatted_features", "bcd_hip_accum_feature_statistics", "bcd_hip_accum_features_state_info",
       "bcd_hip_accum_features_state_bytes", "bcd_hip_accum_export_features", "bcd_hip_accum_import_features", "bcd_hip_accum_merge_features_state"]


def test_new_prototypes_are_declared_and_match_the_header():
    import re
    import bcd_amd._prototypes as bp
    from test_abi_prototypes import header_prototypes, header_text
    want = header_prototypes()
    L = bh.lib()
    for name in NEW:
        assert name in bp.PROTOTYPES and name in bh.SYMBOLS and hasattr(L, name), name
        assert bp.PROTOTYPES[name][0] is want[name][0] and list(bp.PROTOTYPES[name][1]) == want[name][1], name
    # each _features add is its _layers form plus one pointer
    for kind in ("dense", "scattered", "splatted"):
        assert bp.PROTOTYPES["bcd_hip_accum_add_%s_features" % kind][1] == bp.PROTOTYPES["bcd_hip_accum_add_%s_layers" % kind][1] + [C.c_void_p]
    assert bp.PROTOTYPES["bcd_hip_accum_create_features"][1] == bp.PROTOTYPES["bcd_hip_accum_create_layers"][1][:-1] + [C.c_int, C.c_void_p]
    _, macros = header_text()
    assert macros["BCD_HIP_ACCUM_MAX_FEATURES"] == macros["BCD_HIP_GUIDE_MAX_CHANNELS"] == bh.ACCUM_MAX_FEATURES == 8
    assert macros["BCD_HIP_ACCUM_FEATURES_HEADER_BYTES"] == C.sizeof(bh.FeaturesHeader) and macros["BCD_HIP_ACCUM_FEATURES_VERSION"] == 1
    assert struct.calcsize("<8sIIiiiI32s") == 64
    doc = open(bh.__file__.replace("hip.py", "../include/bcd_hip.h")).read()
    assert re.search(r"BCDACCFT", doc)


def test_entry_points_refuse_a_null_accumulator_and_fail_loudly_without_a_gpu():
    """no device is touched, nothing is enqueued"""
    import torch
    L = bh.lib()
    n = C.c_int64(0)
    k = C.c_int(0)
    assert L.bcd_hip_accum_nb_features(None, C.byref(k)) == EINVAL
    assert L.bcd_hip_accum_add_dense_features(None, None, None, 0, 1, 1, 3, None, 3, None) == EINVAL
    assert L.bcd_hip_accum_add_scattered_features(None, None, None, None, 5, None, None) == EINVAL
    assert L.bcd_hip_accum_add_splatted_features(None, None, None, None, 0, None, None) == EINVAL
    assert L.bcd_hip_accum_feature_statistics(None, None, None) == EINVAL
    assert L.bcd_hip_accum_features_state_bytes(None, C.byref(n)) == EINVAL
    for fn in (L.bcd_hip_accum_export_features, L.bcd_hip_accum_import_features, L.bcd_hip_accum_merge_features_state):
        assert fn(None, None, 64) == EINVAL
    h = C.c_void_p(1)
    assert L.bcd_hip_accum_create_features(None, 8, 8, 20, 2.2, 2.5, 0, 0, 3, C.byref(h)) == EINVAL
    if torch.cuda.is_available():
        return
    ctx = C.c_void_p()
    assert L.bcd_hip_ctx_create(C.byref(ctx), 0, None) == -2 and not ctx.value          # BCD_HIP_EDEVICE: no context, so no accumulator


def test_cpp_class_refusals_need_no_device():
    """bcd::DeviceSamplesAccumulator: F = 0 or 9 is not valid; on an accumulator with features the single-sample adds, the batch form without
    features and null features are refused with a message, decided before the device is looked at"""
    import torch
    import bcd_amd.core as core
    for Fc in (0, 9):
        valid, msg = core.device_features_refusals(0, Fc)
        assert not valid and "feature channels must be in [1, 8]" in msg[0]
    valid, msg = core.device_features_refusals(16, 2)
    assert not valid and "layers must be in [0, 15]" in msg[0]
    for nl in (0, 2):
        valid, msg = core.device_features_refusals(nl, 3)
        assert valid == torch.cuda.is_available()
        assert msg[1].startswith("addSample:") and msg[2].startswith("splatSample:") and msg[3].startswith("addSamples:")
        assert all("feature" in m for m in msg[1:4])
        assert msg[4] == "addSamples: null features" and msg[5] == "splatSamples: null features"
