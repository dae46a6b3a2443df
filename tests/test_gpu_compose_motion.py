"""GPU tests of bcd_hip_compose_motion (k_motion_compose.hip; DESIGN 16, "Sequences with motion") against tests/sequence_motion_ref.py, bit for bit: the
isnan masks are equal and the bits of every other value are (the payload of a NaN is not compared).

  * shapes 1x1, 3x5, 255x1, 256x1 and 257x3 (one pixel either side of a 256-pixel workgroup), random fields that leave the image at either step;
  * the special-value fields of sequence_motion_cases: NaN, +-inf, +-2^24 and the floats beside it, -0.0, the halves (round to even), a sum of 2^24;
  * sentinel margins around `out` stay untouched;
  * views offset by one float on a, b and out separately: the launcher's 4-byte-aligned instantiation;
  * the warp identity on the device: bcd_hip_warp_frame (D = 12) through the composed field equals two warps, with validity valid_a(p) AND valid_b(q(p));
  * every refusal, then a good call on the same context."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as mref
import sequence_motion_cases as mc
import sequence_motion_ref as sref

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (3, 5), (255, 1), (256, 1), (257, 3)]      # (W, H)
SENTINEL = F32(-777.25)


def t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def same_bits(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(np.where(nan, F32(0), got).view(np.uint32), np.where(nan, F32(0), want).view(np.uint32))


def in_view(a, offset, margin=16):
    """`a` as a contiguous device view `offset` floats into a buffer of sentinels -> (view, buffer)"""
    import torch
    n = a.size
    buf = torch.full((n + 2 * margin,), float(SENTINEL), dtype=torch.float32, device="cuda")
    v = buf[margin + offset:margin + offset + n].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    return v, buf


def margins_intact(buf, offset, n, margin=16):
    h = buf.cpu().numpy()
    return np.all(h[:margin + offset] == SENTINEL) and np.all(h[margin + offset + n:] == SENTINEL)


@pytest.mark.parametrize("W,H", SHAPES)
def test_compose_is_the_reference_bit_for_bit(hipctx, W, H):
    for k, (a, b) in enumerate(mc.field_pairs(W, H)):
        want = sref.compose(a, b)
        out, buf = in_view(np.full((H, W, 2), SENTINEL, F32), 0)
        hipctx.compose_motion(t(a), t(b), out=out)
        got = out.cpu().numpy()
        assert same_bits(got, want), "%dx%d, pair %d" % (W, H, k)
        assert margins_intact(buf, 0, got.size)
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok], np.rint(got[ok])) and not np.any(np.signbit(got[ok]) & (got[ok] == 0))   # (integers, no -0.0)


@pytest.mark.parametrize("which", ["a", "b", "out"])
@pytest.mark.parametrize("W,H", [(3, 5), (257, 3)])
def test_views_one_float_into_a_buffer(hipctx, W, H, which):
    a, b = mc.field_pairs(W, H)[0]
    sa, sb = mc.special_pair(W, H)
    for a, b in ((a, b), (sa, sb)):
        want = sref.compose(a, b)
        va, _ = in_view(a, 1 if which == "a" else 0)
        vb, _ = in_view(b, 1 if which == "b" else 0)
        off = 1 if which == "out" else 0
        vo, buf = in_view(np.full((H, W, 2), SENTINEL, F32), off)
        assert (va.data_ptr() % 8 == 4) == (which == "a") and (vb.data_ptr() % 8 == 4) == (which == "b") and (vo.data_ptr() % 8 == 4) == (which == "out")
        hipctx.compose_motion(va, vb, out=vo)
        assert same_bits(vo.cpu().numpy(), want)
        assert margins_intact(buf, off, want.size)


def test_warp_identity_on_the_device(hipctx):
    W, H, D = 33, 9, 12
    rng = np.random.default_rng(5)
    col, ns, hist, cov = (rng.random(s).astype(F32) + F32(0.5) for s in ((H, W, 3), (H, W), (H, W, D), (H, W, 6)))
    X = [t(x) for x in (col, ns, hist, cov)]
    for a, b in mc.field_pairs(W, H) + [mc.special_pair(W, H)]:
        ab = hipctx.compose_motion(t(a), t(b))
        once = hipctx.warp_frame(*X, ab)
        mid = hipctx.warp_frame(*X, t(b))
        twice = hipctx.warp_frame(*mid[:4], t(a))
        for g, w in zip(once[:4], twice[:4]):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.cpu().numpy().view(np.uint32))
        ok_a, sl, sc = mref.sources(a, H, W)
        valid_b = mid[4].cpu().numpy().astype(bool)
        assert np.array_equal(once[4].cpu().numpy().astype(bool), ok_a & valid_b[sl, sc])
        assert np.array_equal(twice[4].cpu().numpy().astype(bool), ok_a)            # (the second warp only knows that q is inside the image)
        assert np.all(twice[0].cpu().numpy()[ok_a & ~valid_b[sl, sc]] == 0)
        assert same_bits(ab.cpu().numpy(), sref.compose(a, b))


def test_refusals_leave_the_context_usable(hipctx):
    import torch
    import bcd_amd.hip as bh
    L = bh.lib()
    W, H = 8, 6
    a, b = mc.field_pairs(W, H)[0]
    da, db = t(a), t(b)
    out = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    EINVAL = -1
    assert L.bcd_hip_compose_motion(None, p(da), p(db), W, H, p(out)) == EINVAL
    bad = [(None, p(db), W, H, p(out)), (p(da), None, W, H, p(out)), (p(da), p(db), W, H, None), (p(da), p(db), 0, H, p(out)), (p(da), p(db), W, -1, p(out)),
           (p(da), p(db), W, H, p(da)), (p(da), p(db), W, H, p(db)), (p(da), p(db), W, H, C.c_void_p(da.data_ptr() + 4)),
           (p(da), p(db), W, H, C.c_void_p(db.data_ptr() + W * H * 8 - 4))]
    for args in bad:
        assert L.bcd_hip_compose_motion(hipctx.h, *args) == EINVAL, args
        assert L.bcd_hip_last_error(hipctx.h)
    with pytest.raises(ValueError):
        hipctx.compose_motion(da, t(np.zeros((H, W + 1, 2), F32)))
    assert same_bits(hipctx.compose_motion(da, db, out=out).cpu().numpy(), sref.compose(a, b))
    assert same_bits(hipctx.compose_motion(da, da).cpu().numpy(), sref.compose(a, a))          # (the two inputs may be one field)
