"""GPU tests of the mask transposition of a sequence alone (k_masks_transpose.hip through bcd_hip_transpose_masks_cross / Context.transpose_masks_cross;
DESIGN 16, "Sequences") against tests/sequence_ref.py, bit for bit -- no tolerance anywhere.

  * random masks (every bit drawn independently, bits towards pixels outside the image cleared): b = 6 at 63x3, 64x4, 65x5, 130x9, 1x1 and 13x40 -- either
    side of a tile in both directions, several tiles, frames smaller than the window --, b = 1, 2, 3 at 65x5; padding bits zero, counts = popcounts,
    a NULL count accepted, sentinel margins around both outputs untouched;
  * single-bit masks: one bit at one pixel, for every k at b = 6, moves to bit nbits - 1 - k of the partner pixel and nowhere else;
  * full masks come back as full masks; the transposition twice is the identity;
  * real masks: similarity_masks_cross(A, B) transposed equals similarity_masks_cross(B, A), masks and counts, at 40x28 and 65x37;
  * refusals: null pointers, out aliasing in, b = 0, b = 7 (BCD_HIP_EUNSUPPORTED), then a good call on the same context."""
import numpy as np
import pytest

import oracle_lib as ol
import sequence_ref as sq

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
MARGIN = 64          # int32 words in front of and behind each output


def random_masks(W, H, b, seed):
    """every bit that points inside the image drawn with probability 1/2"""
    rng = np.random.default_rng(seed)
    bits = (rng.random((H, W, (2 * b + 1) ** 2)) < 0.5) & sq.in_image_bits(H, W, b)
    return sq.pack(bits, b)


def t(mask):
    import torch
    return torch.from_numpy(np.ascontiguousarray(mask).view(np.int32)).cuda()


def run_guarded(ctx, mask, b, with_count=True):
    """the stage into outputs carved out of sentinel-filled allocations -> (masks uint32, counts or None); asserts the margins"""
    import torch
    H, W, words = mask.shape
    big_m = torch.full((MARGIN + H * W * words + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    big_c = torch.full((MARGIN + H * W + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    om = big_m[MARGIN:MARGIN + H * W * words].view(H, W, words)
    oc = big_c[MARGIN:MARGIN + H * W].view(H, W)
    ctx.transpose_masks_cross(t(mask), b, out=(om, oc if with_count else None))
    bm, bc = big_m.cpu().numpy(), big_c.cpu().numpy()
    assert (bm[:MARGIN] == SENTINEL).all() and (bm[-MARGIN:] == SENTINEL).all(), "the margins of the mask output were written"
    assert (bc[:MARGIN] == SENTINEL).all() and (bc[-MARGIN:] == SENTINEL).all(), "the margins of the count output were written"
    if not with_count:
        assert (bc == SENTINEL).all(), "a count image was written although none was given"
    return om.cpu().numpy().view(np.uint32), oc.cpu().numpy() if with_count else None


def popcounts(mask):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), axis=-1).sum(axis=-1).astype(np.int32)


CASES = [(63, 3, 6), (64, 4, 6), (65, 5, 6), (130, 9, 6), (1, 1, 6), (13, 40, 6), (65, 5, 1), (65, 5, 2), (65, 5, 3)]


@pytest.mark.parametrize("W,H,b", CASES)
def test_random_masks_against_the_definition(hipctx, W, H, b):
    mask = random_masks(W, H, b, 100 * W + H + b)
    want_m, want_c = sq.transpose_masks(mask, b)
    got_m, got_c = run_guarded(hipctx, mask, b)
    assert np.array_equal(got_m, want_m)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_c, popcounts(got_m))
    nbits = (2 * b + 1) ** 2
    if nbits % 32:
        assert not (got_m[:, :, -1] >> np.uint32(nbits % 32)).any(), "padding bits of the last word are set"
    if W * H > 1:
        assert 0 < int(want_c.sum()) < W * H * nbits
    no_c, none = run_guarded(hipctx, mask, b, with_count=False)               # a NULL count is accepted
    assert none is None and np.array_equal(no_c, want_m)
    back, _ = run_guarded(hipctx, got_m, b)                                   # twice: the identity (no bit of `mask` points outside the image)
    assert np.array_equal(back, mask)


def test_single_bits_move_to_the_partner_pixel(hipctx):
    """for every k at b = 6: bit k alone at pixel p -> bit nbits - 1 - k alone at p + delta_k (all 169 in one image: the partners are distinct)"""
    b, side = 6, 13
    nbits, words = side * side, sq.words_of(b)
    W, H = 70, 20
    p = (9, 33)                                                               # every p + delta_k lies in the image; a tile boundary (column 64) is not crossed ...
    for (pl, pc) in (p, (10, 62)):                                            # ... and here it is
        for k in range(nbits):
            mask = np.zeros((H, W, words), np.uint32)
            mask[pl, pc, k >> 5] = np.uint32(1) << np.uint32(k & 31)
            if k % 24 and (pl, pc) != p:                                      # every k at the first pixel, a sample of them across the tile boundary
                continue
            got_m, got_c = hipctx.transpose_masks_cross(t(mask), b)
            got_m = got_m.cpu().numpy().view(np.uint32)
            want = np.zeros_like(mask)
            ql, qc, j = pl + k // side - b, pc + k % side - b, nbits - 1 - k
            want[ql, qc, j >> 5] = np.uint32(1) << np.uint32(j & 31)
            assert np.array_equal(got_m, want), k
            assert int(got_c.sum()) == 1 and int(got_c[ql, qc]) == 1


@pytest.mark.parametrize("W,H,b", [(65, 5, 6), (13, 40, 6), (130, 9, 3)])
def test_full_masks_come_back_full(hipctx, W, H, b):
    full = sq.pack(sq.in_image_bits(H, W, b), b)
    got_m, got_c = run_guarded(hipctx, full, b)
    assert np.array_equal(got_m, full) and np.array_equal(got_c, popcounts(full))


_frames = {}


def frames_of(W, H):
    if (W, H) not in _frames:
        _frames[(W, H)] = [ol.synth_inputs(W, H, 32, seed)[:4] for seed in (1234, 77)]
    return _frames[(W, H)]


@pytest.mark.parametrize("W,H", [(40, 28), (65, 37)])
def test_real_cross_masks_of_a_pair_are_transposes_of_each_other(hipctx, W, H):
    import torch
    (_, ns_a, hist_a, _), (_, ns_b, hist_b, _) = frames_of(W, H)
    d = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    ab_m, ab_c = hipctx.similarity_masks_cross(d(hist_a), d(ns_a), d(hist_b), d(ns_b), 1, 6, 1.0)
    ba_m, ba_c = hipctx.similarity_masks_cross(d(hist_b), d(ns_b), d(hist_a), d(ns_a), 1, 6, 1.0)
    tr_m, tr_c = hipctx.transpose_masks_cross(ab_m.clone(), 6)
    members, candidates = int(ab_c.sum()), (W - 2) * (H - 2) * 169
    assert 0 < members < candidates
    assert torch.equal(tr_m, ba_m) and torch.equal(tr_c, ba_c)
    assert int(ba_c.sum()) == members                                         # (a pair is a member from both sides)


def test_refusals_then_a_good_call(hipctx):
    import ctypes as C
    import torch
    import bcd_amd.hip as bh
    lib = bh.lib()
    W, H, b = 20, 10, 6
    mask = random_masks(W, H, b, 5)
    m_in, m_out = t(mask), torch.zeros((H, W, 6), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda x: C.c_void_p(x.data_ptr())
    call = lambda *a: lib.bcd_hip_transpose_masks_cross(hipctx.h, *a)
    err = lambda: lib.bcd_hip_last_error(hipctx.h).decode()
    EINVAL, EUNSUPPORTED = -1, -4
    assert call(None, W, H, b, p(m_out), p(cnt)) == EINVAL and "null" in err()
    assert call(p(m_in), W, H, b, None, p(cnt)) == EINVAL and "null" in err()
    assert call(p(m_in), W, H, b, p(m_in), p(cnt)) == EINVAL and "overlap" in err()                      # out aliasing in
    assert call(p(m_in), W, H, b, C.c_void_p(m_in.data_ptr() + 24), p(cnt)) == EINVAL and "overlap" in err()
    assert call(p(m_in), W, H, b, p(m_out), p(m_out)) == EINVAL and "overlap" in err()                   # the counts inside the masks
    assert call(p(m_in), 0, H, b, p(m_out), p(cnt)) == EINVAL and call(p(m_in), W, -1, b, p(m_out), p(cnt)) == EINVAL
    assert call(p(m_in), W, H, 0, p(m_out), p(cnt)) == EINVAL and "search radius" in err()
    assert call(p(m_in), W, H, 7, p(m_out), p(cnt)) == EUNSUPPORTED and "1 to 6" in err()
    assert not m_out.any() and not cnt.any()                                                            # nothing ran
    got_m, got_c = hipctx.transpose_masks_cross(m_in, b, out=(m_out, cnt))
    want_m, want_c = sq.transpose_masks(mask, b)
    assert np.array_equal(got_m.cpu().numpy().view(np.uint32), want_m) and np.array_equal(got_c.cpu().numpy(), want_c)
