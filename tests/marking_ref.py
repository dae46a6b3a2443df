"""The marking strategy of the reference, restated sequentially (src/core/DenoisingUnit.cpp:164-173,182-191,690).  TEST INFRASTRUCTURE.

The reference visits the main pixels in a fixed order.  A visited pixel that an earlier pixel has marked is skipped with the skip probability m
(here: if its skip draw says so); otherwise it is processed.  A processed pixel whose similar set holds at least 3 (2w+1)^2 + 1 patches marks every
pixel of that set; a processed pixel with a smaller set takes the fallback path and marks nobody.  That is all `greedy` does, pixel after pixel: it is
NOT the fixed-point formulation of k_active.hip, shares no code with tests/oracle_engine.py and never calls the library's marking.

Masks: (H, W, words) uint32, bit k = (dl + b) (2b+1) + (dc + b) of pixel p set <=> p + (dl, dc) is in S(p).  States: the engine's encoding
(bcd_common.h)."""
import numpy as np

ST_NONE, ST_IN, ST_OUT, ST_UNDECIDED = 0, 1, 2, 3


def strong_threshold(w):
    """|S| from which a processed pixel takes the full estimate and marks its set: 3 P + 1, P = (2w+1)^2 (DenoisingUnit.cpp:182)"""
    return 3 * (2 * w + 1) ** 2 + 1


def main_area(W, H, w):
    a = np.zeros((H, W), bool)
    if H > 2 * w and W > 2 * w:
        a[w:H - w, w:W - w] = True
    return a


def unpack(mask, b):
    """(H, W, words) uint32 -> (H, W, (2b+1)^2) bool"""
    n = (2 * b + 1) ** 2
    m = np.ascontiguousarray(mask, np.uint32)
    k = np.arange(n)
    return ((m[:, :, k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def pack(bits):
    """(H, W, n) bool -> (H, W, ceil(n / 32)) uint32"""
    H, W, n = bits.shape
    words = (n + 31) // 32
    out = np.zeros((H, W, words), np.uint32)
    for k in range(n):
        out[:, :, k >> 5] |= bits[:, :, k].astype(np.uint32) << np.uint32(k & 31)
    return out


def members(mask, b):
    """the similar sets as a CSR pair (ptr (H W + 1,), idx): idx[ptr[p]:ptr[p + 1]] = linear indices of S(p)"""
    H, W, _ = mask.shape
    side = 2 * b + 1
    m = np.ascontiguousarray(mask, np.uint32)
    l, c, j = np.nonzero(m)                                          # the words that hold a bit, sorted by pixel, then their bits in ascending order
    i, bit = np.nonzero((m[l, c, j][:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1))
    l, c, k = l[i], c[i], j[i] * 32 + bit
    idx = (l + k // side - b) * W + (c + k % side - b)
    ptr = np.zeros(H * W + 1, np.int64)
    np.cumsum(np.bincount(l * W + c, minlength=H * W), out=ptr[1:])
    return ptr, idx.astype(np.int64)


def _mix32(x):
    """bcd_mix32 on uint32 arrays"""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x


def unit_hash(idx, seed):
    """bcd_unit_hash in uint32 / float32: uniform in [0, 1) per global pixel index"""
    with np.errstate(over="ignore"):
        s = _mix32(np.array([(seed ^ 0x51ed270b) & 0xFFFFFFFF], np.uint32))[0]
        h = _mix32(np.asarray(idx, np.uint32) * np.uint32(0x9E3779B1) + s)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def skip_draw(W, H, m, seed, row_offset=0):
    """(H, W) bool: would this pixel be skipped if it is marked?  All true for m >= 1, all false for m <= 0; in between the engine's per-pixel
    draw on the GLOBAL pixel index (row_offset = line of the full frame under line 0)"""
    if m <= 0:
        return np.zeros((H, W), bool)
    if m >= 1:
        return np.ones((H, W), bool)
    l, c = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    return unit_hash(((l + row_offset) * W + c) & 0xFFFFFFFF, seed) < np.float32(m)


def greedy(mask, cnt, w, b, order, drawn):
    """the state image after the reference's sequential pass over the main pixels in `order` (linear indices line * W + col)"""
    H, W, _ = mask.shape
    ptr, idx = members(mask, b)
    strong = (np.asarray(cnt).reshape(-1) >= strong_threshold(w)).tolist()
    skip = np.asarray(drawn, bool).reshape(-1).tolist()
    ptr_l = ptr.tolist()
    marked = np.zeros(H * W, bool)
    state = np.full(H * W, ST_NONE, np.uint8)
    for p in np.asarray(order).tolist():
        if skip[p] and marked[p]:
            state[p] = ST_OUT
            continue
        state[p] = ST_IN
        if strong[p]:
            marked[idx[ptr_l[p]:ptr_l[p + 1]]] = True
    return state.reshape(H, W)
