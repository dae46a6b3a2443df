"""GPU tests of the stage calls of the motion path (k_warp.hip; DESIGN 16, "Motion") against tests/motion_ref.py, bit for bit.

  * bcd_hip_warp_frame on every size of motion_cases.STAGE_SIZES (1x1 .. 257x3: either side of a 64-pixel line and of a 256-pixel workgroup) x every depth
    of STAGE_DEPTHS (60, 120, 36, 24, 12: the 16-byte form; 45 and 7: the element form) x every named field (zero, None, random, ties, special, checker,
    corner), the destinations inside sentinel margins that must survive, once 16-byte aligned and once 4 bytes off (which the 16-byte depths then serve with
    the element form): colours, sample counts, histograms, covariances and the validity bytes equal the reference's bits, NaN payloads and -0.0 included;
  * bcd_hip_warp_layers the same for L = 1, 2, 4, 5, 16;
  * bcd_hip_valid_downscale level by level on odd and even sizes down to one pixel;
  * bcd_hip_gate_masks_valid on constructed masks -- all ones, a single bit per displacement, random masks -- under validity images that clip at each border,
    for (w, b) = (1, 6), (2, 6), (1, 2), (2, 2); a gate that empties a set (|S_f| = 0) and gates that leave exactly 27 and 28 members;
  * the refusals of the stage calls, then a good call on the same context."""
import numpy as np
import pytest

import motion_cases as mc
import motion_ref as mo
import temporal_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = np.float32(-7.25)
MARGIN = 64          # floats either side of a destination


def boxed(shape, off, dtype=None):
    """a contiguous device tensor of `shape` inside a sentinel-filled buffer, `off` elements past a 16-byte aligned margin -> (view, whole buffer)"""
    import torch
    dtype = dtype or torch.float32
    n = int(np.prod(shape))
    buf = torch.full((MARGIN + off + n + MARGIN,), float(SENTINEL) if dtype == torch.float32 else 0xA5, dtype=dtype, device="cuda")
    return buf[MARGIN + off:MARGIN + off + n].view(*shape), buf


def placed(a, off):
    """the array on the device at `off` floats past an aligned address"""
    import torch
    view, _ = boxed(a.shape, off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def margins_intact(view_buf, off):
    view, buf = view_buf
    n = view.numel()
    fill = float(SENTINEL) if buf.dtype.is_floating_point else 0xA5
    return bool((buf[:MARGIN + off] == fill).all()) and bool((buf[MARGIN + off + n:] == fill).all())


def bits(t):
    a = t.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def fields_of(W, H):
    return [("none", None)] + [(name, mc.field(name, W, H)) for name in mc.FIELDS]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D", mc.STAGE_DEPTHS)
@pytest.mark.parametrize("W,H", mc.STAGE_SIZES)
def test_warp_frame_bit_for_bit(hipctx, W, H, D, off):
    import torch
    fr = mc.stage_frame(W, H, D)
    src = [placed(a, off) for a in fr]
    for name, mv in fields_of(W, H):
        want, wvalid = mo.warp(fr, mv)
        out = [boxed(a.shape, off) for a in fr] + [boxed((H, W), off, torch.uint8)]
        d_mv = None if mv is None else placed(mv, off)
        got = hipctx.warp_frame(*src, d_mv, out=[o[0] for o in out])
        hipctx.synchronize()
        assert np.array_equal(got[4].cpu().numpy(), wvalid), name
        for k, (g, w_) in enumerate(zip(got[:4], want)):
            assert np.array_equal(bits(g), np.ascontiguousarray(w_).view(np.uint32)), (name, k)
        assert all(margins_intact(o, off) for o in out), name
        if name == "special" and W * H > 4:
            assert 0 < wvalid.sum() < wvalid.size


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("L", mc.STAGE_LAYERS)
@pytest.mark.parametrize("W,H", mc.STAGE_SIZES)
def test_warp_layers_bit_for_bit(hipctx, W, H, L, off):
    import torch
    layers = mc.stage_layers(W, H, L)
    src = [(placed(c, off), placed(v, off)) for c, v in layers]
    for name, mv in fields_of(W, H):
        want, wvalid = mo.warp([a for pair in layers for a in pair], mv)
        out = [(boxed((H, W, 3), off), boxed((H, W, 6), off)) for _ in range(L)]
        valid = boxed((H, W), off, torch.uint8)
        d_mv = None if mv is None else placed(mv, off)
        got, gvalid = hipctx.warp_layers(src, d_mv, out=([(c[0], v[0]) for c, v in out], valid[0]))
        hipctx.synchronize()
        assert np.array_equal(gvalid.cpu().numpy(), wvalid), name
        for k, (c, v) in enumerate(got):
            assert np.array_equal(bits(c), want[2 * k].view(np.uint32)) and np.array_equal(bits(v), want[2 * k + 1].view(np.uint32)), (name, k)
        assert all(margins_intact(c, off) and margins_intact(v, off) for c, v in out) and margins_intact(valid, off), name


@pytest.mark.parametrize("W,H", [(2, 2), (3, 2), (5, 4), (7, 7), (16, 11), (33, 21), (130, 9), (257, 6)])
def test_valid_downscale_down_to_one_pixel(hipctx, W, H):
    import torch
    rng = np.random.default_rng(31 * W + H)
    for density in (0.85, 0.5, 1.0):
        v = (rng.random((H, W)) < density).astype(np.uint8)
        d = torch.from_numpy(v).cuda()
        while min(v.shape) >= 2:
            want = mo.valid_down(v)
            out = hipctx.valid_downscale(d)
            hipctx.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), v.shape
            v, d = want, out
        assert min(v.shape) == 1 or v.size == 0


def validity_images(W, H):
    """validity images whose invalid pixels sit at each border, at patch corners and as a checkerboard"""
    rng = np.random.default_rng(W + 7 * H)
    out = {"all valid": np.ones((H, W), np.uint8)}
    for name, sl in (("first line", (0, slice(None))), ("last line", (H - 1, slice(None))), ("first column", (slice(None), 0)), ("last column", (slice(None), W - 1))):
        v = np.ones((H, W), np.uint8)
        v[sl] = 0
        out[name] = v
    out["corner"] = mo.sources(mc.field("corner", W, H), H, W)[0].astype(np.uint8)
    out["checker"] = mo.sources(mc.field("checker", W, H), H, W)[0].astype(np.uint8)
    out["random"] = (rng.random((H, W)) < 0.9).astype(np.uint8)
    out["none valid"] = np.zeros((H, W), np.uint8)
    return out


def constructed_masks(W, H, b, seed=3):
    side = 2 * b + 1
    words = (side * side + 31) // 32
    rng = np.random.default_rng(seed)
    out = {"all ones": np.full((H, W, words), 0xffffffff, np.uint32)}            # (bits beyond the window and of clipped displacements included)
    single = np.zeros((H, W, words), np.uint32)
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    k = (l * W + c) % (side * side)                                              # every displacement is some pixel's single bit
    np.put_along_axis(single, (k >> 5)[..., None], (np.uint32(1) << (k & 31).astype(np.uint32))[..., None], axis=-1)
    out["single bit"] = single
    out["random"] = rng.integers(0, 2 ** 32, (H, W, words), dtype=np.uint64).astype(np.uint32)
    return out


@pytest.mark.parametrize("w,b", [(1, 6), (2, 6), (1, 2), (2, 2)])
@pytest.mark.parametrize("W,H", [(20, 16), (70, 9), (5, 5)])
def test_gate_on_constructed_masks(hipctx, W, H, w, b):
    import torch
    for mname, mask in constructed_masks(W, H, b).items():
        for vname, valid in validity_images(W, H).items():
            wm, wn = mo.gate(mask, None, valid, w, b)
            d_mask = torch.from_numpy(mask.view(np.int32).copy()).cuda()
            d_count = torch.full((H, W), -5, dtype=torch.int32, device="cuda")
            hipctx.gate_masks_valid(d_mask, d_count, torch.from_numpy(valid).cuda(), w, b)
            hipctx.synchronize()
            assert np.array_equal(d_mask.cpu().numpy().view(np.uint32), wm), (mname, vname)
            assert np.array_equal(d_count.cpu().numpy(), wn), (mname, vname)
            if vname == "none valid":
                assert wn.sum() == 0
            if vname == "all valid" and mname == "all ones" and min(W, H) > 2 * w:
                centre = wn[H // 2, W // 2]
                assert centre == (min(H - 1 - w, H // 2 + b) - max(w, H // 2 - b) + 1) * (min(W - 1 - w, W // 2 + b) - max(w, W // 2 - b) + 1)


def test_gate_empties_a_set_and_leaves_27_and_28_members(hipctx):
    """the sizes either side of the 3P + 1 rule come out of the gate exactly: three main pixels with 30 members each -- 13 on each of two lines and 4, three
    columns apart, on a third -- of which 3, 2 and all sit on patches with an invalid pixel (one invalid pixel below a member of the third line is in that
    member's patch alone)"""
    import torch
    W, H, w, b = 60, 20, 1, 6
    side = 2 * b + 1
    words = (side * side + 31) // 32
    mask = np.zeros((H, W, words), np.uint32)
    valid = np.ones((H, W), np.uint8)
    l = 9
    pts = {(l, 7): 3, (l, 25): 2, (l, 45): 30}               # main pixel -> members to lose
    sparse = (-5, -2, 1, 4)
    for (_, c), lose in pts.items():
        members = [(dl, dc) for dl in (-3, -1) for dc in range(-6, 7)] + [(1, dc) for dc in sparse]
        assert len(members) == 30
        for (dl, dc) in members:
            k = (dl + b) * side + (dc + b)
            mask[l, c, k >> 5] |= np.uint32(1) << np.uint32(k & 31)
        if lose == 30:
            valid[l - 4:l + 3, c - 7:c + 8] = 0
        else:
            for dc in sparse[:lose]:
                valid[l + 2, c + dc] = 0
    wm, wn = mo.gate(mask, None, valid, w, b)
    assert [int(wn[p]) for p in pts] == [27, 28, 0], [int(wn[p]) for p in pts]
    d_mask = torch.from_numpy(mask.view(np.int32).copy()).cuda()
    d_count = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    hipctx.gate_masks_valid(d_mask, d_count, torch.from_numpy(valid).cuda(), w, b)
    hipctx.synchronize()
    assert np.array_equal(d_mask.cpu().numpy().view(np.uint32), wm) and np.array_equal(d_count.cpu().numpy(), wn)
    assert [int(d_count[p]) for p in pts] == [27, 28, 0]


def test_gate_after_the_cross_masks_is_the_reference_s(hipctx):
    """the stage composition: bcd_hip_similarity_masks_cross on a warped neighbour, then the gate, against cross_masks + gate of the references"""
    import torch
    import temporal_cases as tc
    W, H, D, w, b, tau = 33, 21, 60, 1, 6, F(1.0)
    fr = (None,) + tc.frame(W, H, D, 2, 3)[::-1]                     # (-, ns, hist) at 2 spp: many pixels without a bin above 1, so zeros can pass ungated
    nb = list(mc.stage_frame(W, H, D, seed=9))
    nb[2], nb[1] = tc.frame(W, H, D, 2, 9)
    mv = np.zeros((H, W, 2), F)
    mv[3, 3, 0], mv[10:13, 20:23], mv[0, :, 1], mv[:, W - 1, 0] = np.nan, np.nan, -1, 2
    (col, ns, hist, cov), valid = mo.warp(nb, mv)
    m, n = tr.cross_masks(fr[2], fr[1], hist, ns, w, b, tau)
    wm, wn = mo.gate(m, n, valid, w, b)
    assert 0 < wn.sum() < n.sum()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = hipctx.warp_frame(*[t(a) for a in nb], t(mv))
    gm, gn = hipctx.similarity_masks_cross(t(fr[2]), t(fr[1]), g[2], g[1], w, b, float(tau))
    hipctx.synchronize()
    assert np.array_equal(gn.cpu().numpy(), n)
    hipctx.gate_masks_valid(gm, gn, g[4], w, b)
    hipctx.synchronize()
    assert np.array_equal(gm.cpu().numpy().view(np.uint32).reshape(wm.shape), wm) and np.array_equal(gn.cpu().numpy(), wn)


def test_refusals_of_the_stage_calls_then_good_calls(hipctx):
    import torch
    import bcd_amd.hip as bh
    W, H, D = 17, 5, 24
    fr = mc.stage_frame(W, H, D)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src = [t(a) for a in fr]
    mv = t(mc.field("random", W, H))
    good = lambda: [torch.empty_like(a) for a in src] + [torch.empty((H, W), dtype=torch.uint8, device="cuda")]

    def refused(call):
        with pytest.raises(bh.BcdHipError):
            call()

    for k in range(4):                                               # a destination that is an input
        out = good()
        out[k] = src[k]
        refused(lambda: hipctx.warp_frame(*src, mv, out=out))
    big = torch.empty((H * W * 6,), dtype=torch.float32, device="cuda")
    out = good()
    out[0], out[3] = big[:H * W * 3].view(H, W, 3), big[:H * W * 6].view(H, W, 6)             # two destinations overlap
    refused(lambda: hipctx.warp_frame(*src, mv, out=out))
    field6 = torch.zeros((H, W, 6), dtype=torch.float32, device="cuda")                        # the field lies inside a destination
    out = good()
    out[3] = field6
    refused(lambda: hipctx.warp_frame(*src, field6.view(-1)[:H * W * 2].view(H, W, 2), out=out))
    layers = [(t(c), t(v)) for c, v in mc.stage_layers(W, H, 2)]
    dst = [(torch.empty_like(c), torch.empty_like(v)) for c, v in layers]
    valid = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    refused(lambda: hipctx.warp_layers(layers, mv, out=([dst[0], (dst[1][0], layers[0][1])], valid)))
    refused(lambda: hipctx.warp_layers(layers, mv, out=([dst[0], (dst[0][0], dst[1][1])], valid)))
    refused(lambda: hipctx.warp_layers(layers * 9, mv))                                        # eighteen layers
    m = torch.zeros((H, W, 6), dtype=torch.int32, device="cuda")
    c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    m16 = torch.zeros((H, W, (33 * 33 + 31) // 32), dtype=torch.int32, device="cuda")
    refused(lambda: hipctx.gate_masks_valid(m16, c, valid, 1, 16))                            # search radius > 15
    refused(lambda: hipctx.gate_masks_valid(m, c, valid, 3, 6))                               # the image is smaller than a patch
    refused(lambda: hipctx.valid_downscale(torch.ones((1, 5), dtype=torch.uint8, device="cuda")))
    want, wvalid = mo.warp(fr, mv.cpu().numpy())
    got = hipctx.warp_frame(*src, mv)
    hipctx.synchronize()
    assert np.array_equal(got[4].cpu().numpy(), wvalid) and all(np.array_equal(bits(g), w_.view(np.uint32)) for g, w_ in zip(got[:4], want))
