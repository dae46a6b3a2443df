"""NumPy reference of the mask transposition of a sequence (k_masks_transpose.hip, bcd_hip_transpose_masks_cross; DESIGN.md section 16, "Sequences"),
written straight from the definition.  TEST INFRASTRUCTURE.

side = 2b + 1, nbits = side^2, words = ceil(nbits / 32), delta_k = (k // side - b, k % side - b).  For every pixel p and every k < nbits: if p + delta_k
lies in the image, out(p) bit k = in(p + delta_k) bit (nbits - 1 - k); otherwise the bit is 0.  Bits >= nbits of the last word are 0; count(p) is the
popcount of the output mask."""
import numpy as np


def words_of(b):
    return ((2 * b + 1) ** 2 + 31) // 32


def unpack(mask, b):
    """(H, W, words) uint32 / int32 -> (H, W, nbits) bool"""
    m = np.ascontiguousarray(mask).view(np.uint32)
    nbits = (2 * b + 1) ** 2
    k = np.arange(nbits)
    return ((m[:, :, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def pack(bits, b):
    """(H, W, nbits) bool -> (H, W, words) uint32, the padding bits zero"""
    H, W, nbits = bits.shape
    out = np.zeros((H, W, words_of(b)), np.uint32)
    for k in range(nbits):
        out[:, :, k >> 5] |= bits[:, :, k].astype(np.uint32) << np.uint32(k & 31)
    return out


def transpose_masks(mask, b):
    """-> (masks (H, W, words) uint32, counts (H, W) int32) of the definition"""
    bits = unpack(mask, b)
    H, W, nbits = bits.shape
    side = 2 * b + 1
    out = np.zeros_like(bits)
    for k in range(nbits):
        dl, dc = k // side - b, k % side - b
        l0, l1, c0, c1 = max(0, -dl), min(H, H - dl), max(0, -dc), min(W, W - dc)       # the pixels p with p + delta_k in the image
        if l0 < l1 and c0 < c1:
            out[l0:l1, c0:c1, k] = bits[l0 + dl:l1 + dl, c0 + dc:c1 + dc, nbits - 1 - k]
    return pack(out, b), out.sum(axis=2).astype(np.int32)


def in_image_bits(H, W, b):
    """(H, W, nbits) bool: bit k of pixel p points at a pixel inside the image"""
    side = 2 * b + 1
    k = np.arange(side * side)
    l = np.arange(H)[:, None, None] + (k // side - b)[None, None, :]
    c = np.arange(W)[None, :, None] + (k % side - b)[None, None, :]
    return (l >= 0) & (l < H) & (c >= 0) & (c < W)
