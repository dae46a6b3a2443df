"""Seeded uint32 bit images for the sparse histogram upload (bcd_amd/csrc/bcd_sparse_upload.hip) and the byte-counter rule its header documents.

A case is an image, the piece length it travels with and what every piece is MEANT to be: "sparse" (at most 55 % non-zero words: packed),
"dense" (at least 65 %: the piece that turns the frame dense), "edge_sparse" / "edge_dense" (exactly 0.6 n and 0.6 n + 1 non-zero words of a piece
of n, n divisible by 5: either side of the rule `nonzero * 10 > n * 6`).  tests/test_sparse_cases_cpu.py holds the generator to these promises, so
that a GPU test cannot pass by taking another path than the one its name says; the expected counters are computed from the promises, not by
re-applying the rule to the image.  Only the all-zero word is "zero": -0.0f, denormals, infinities and NaNs are values."""
import numpy as np

BLOCK = 2048                      # floats per unpack workgroup: 64 mask words
TASK = 16 * BLOCK                 # floats per packing task
PIECE = 12 << 20                  # the production piece
SMALL_PIECE = 65536

# bit patterns that are values to the packer although arithmetic may treat them as zero, or not as numbers at all
SPECIAL = np.array([0x80000000,                                     # -0.0f
                    0x00000001, 0x007FFFFF, 0x80000001, 0x00400000,  # denormals (smallest, largest, negative, middle)
                    0x7F800000, 0xFF800000,                          # +inf, -inf
                    0x7FC00000, 0xFFC00001, 0x7FC12345,              # quiet NaNs, with payloads
                    0x7F800001, 0xFFA54321, 0x7FBFFFFF,              # signalling NaNs, with payloads
                    0xFFFFFFFF], np.uint32)


class Case:
    def __init__(self, group, name, words, kinds, piece=0):
        self.group, self.name, self.words, self.kinds, self.piece = group, name, np.ascontiguousarray(words, np.uint32), list(kinds), piece
        self.id = "%s-%s" % (group, name)

    @property
    def piece_len(self):
        return self.piece or PIECE

    def pieces(self):
        """[(begin, end)] of the pieces the image travels in"""
        n, p = self.words.size, self.piece_len
        return [(i, min(n, i + p)) for i in range(0, n, p)]


def values(rng, k, special_share=0.05):
    """k non-zero words: random bits with the special patterns mixed in"""
    v = rng.integers(1, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    sp = rng.random(k) < special_share
    v[sp] = SPECIAL[rng.integers(0, SPECIAL.size, int(sp.sum()))]
    return v


def image(rng, n, nonzero, special_share=0.05):
    """n words with EXACTLY `nonzero` non-zero ones at random places"""
    w = np.zeros(n, np.uint32)
    w[rng.permutation(n)[:nonzero]] = values(rng, nonzero, special_share)
    return w


def by_density(rng, n, density):
    # (rounded away from the 60 % rule: down at or below 55 %, up at or above 65 %)
    k = np.floor(density * n + 1e-9) if density <= 0.55 else np.ceil(density * n - 1e-9)
    return image(rng, n, int(k))


def kind_of(density):
    assert density <= 0.55 or density >= 0.65
    return "sparse" if density <= 0.55 else "dense"


LENGTHS = [1, 3, 4, 5, 31, 32, 33, 2047, 2048, 2049, TASK - 1, TASK + 1, 5 * TASK + 37]
DENSITIES = [0.0, 0.01, 0.3, 0.55, 0.65, 1.0]
EDGE_N = 5 * BLOCK                # divisible by 5


def pattern_cases(seed=11):
    rng = np.random.default_rng(seed)
    out = []
    # every special pattern at every position of a 32-word group (and so of a 4-value store group), zeros between them: 3 blocks + a tail
    n = 3 * BLOCK + 45
    w = np.zeros(n, np.uint32)
    idx = np.arange(0, n, 3)
    w[idx] = SPECIAL[(idx // 3 + idx // 96) % SPECIAL.size]
    out.append(Case("patterns", "every_pattern_every_lane", w, ["sparse"]))
    # only special patterns, at random places
    out.append(Case("patterns", "random_places", image(rng, 2 * TASK + 333, 9000, special_share=1.0), ["sparse"]))
    # a block of nothing but -0.0f (arithmetic zero, 2048 values to the packer) between zero blocks
    w = np.zeros(4 * BLOCK, np.uint32)
    w[BLOCK:2 * BLOCK] = 0x80000000
    out.append(Case("patterns", "block_of_negative_zero", w, ["sparse"]))
    return out


def length_cases(seed=12):
    rng = np.random.default_rng(seed)
    out = []
    for n in LENGTHS:
        k = 1 if n < 4 else int(round(0.3 * n))          # (n = 1: one value of one -- a dense piece; n = 3: one of three)
        out.append(Case("lengths", "n%d" % n, image(rng, n, k), ["dense" if n == 1 else "sparse"]))
    return out


def block_cases(seed=13):
    rng = np.random.default_rng(seed)
    out = []
    out.append(Case("blocks", "all_zero", np.zeros(3 * BLOCK + 7, np.uint32), ["sparse"]))
    # whole blocks of values between whole blocks of zeros (nv = 2048 and nv = 0)
    w = np.zeros(8 * BLOCK, np.uint32)
    for blk in (1, 4, 6):
        w[blk * BLOCK:(blk + 1) * BLOCK] = values(rng, BLOCK)
    out.append(Case("blocks", "full_between_empty", w, ["sparse"]))
    # a full block whose values start 1, 2, 3 and 0 words past a 16-byte boundary of the stream: (one value)(full) four times, then empty blocks
    # -- the stream offsets of the full blocks are 1, 2050, 4099, 6148 -- and the same with 2 and 3 values in front of the first full block
    for lead in (1, 2, 3):
        w = np.zeros(12 * BLOCK, np.uint32)
        for pair in range(4):
            k = lead if pair == 0 else 1
            w[2 * pair * BLOCK + rng.permutation(BLOCK)[:k]] = values(rng, k)
            w[(2 * pair + 1) * BLOCK:(2 * pair + 2) * BLOCK] = values(rng, BLOCK)
        out.append(Case("blocks", "full_after_%d" % lead, w, ["sparse"]))
    w = np.zeros(2 * BLOCK + 101, np.uint32)
    w[-1] = 0x3F800000
    out.append(Case("blocks", "only_the_last_word", w, ["sparse"]))
    return out


def stream_offsets_of_full_blocks(words):
    """values in front of every block that is all values, taken modulo 4: the LDS window alignments a single-task image exercises"""
    nz = (words.reshape(-1, BLOCK) != 0).sum(1)
    before = np.concatenate([[0], np.cumsum(nz)[:-1]])
    return sorted(set(int(o) % 4 for o, k in zip(before, nz) if k == BLOCK))


def density_cases(seed=14):
    rng = np.random.default_rng(seed)
    out = [Case("densities", "d%g" % d, by_density(rng, EDGE_N, d), [kind_of(d)]) for d in DENSITIES]
    out.append(Case("densities", "edge_0.6n", image(rng, EDGE_N, EDGE_N * 3 // 5), ["edge_sparse"]))
    out.append(Case("densities", "edge_0.6n_plus_1", image(rng, EDGE_N, EDGE_N * 3 // 5 + 1), ["edge_dense"]))
    return out


def pieces_image(rng, lens, densities):
    return np.concatenate([by_density(rng, n, d) for n, d in zip(lens, densities)])


def multi_piece_cases(seed=15):
    rng = np.random.default_rng(seed)
    P = SMALL_PIECE
    out = []
    lens = [P] * 7 + [1237]                                   # three staging buffers: the rotation goes round twice; the tail is no multiple of 4
    out.append(Case("multi", "seven_pieces_ragged_tail", pieces_image(rng, lens, [0.3, 0.05, 0.5, 0.0, 0.2, 0.55, 0.1, 0.4]), ["sparse"] * 8, P))
    out.append(Case("multi", "sparse_dense_sparse", pieces_image(rng, [P] * 3, [0.2, 0.8, 0.2]), ["sparse", "dense", "sparse"], P))
    out.append(Case("multi", "dense_first", pieces_image(rng, [P, P, 999], [0.9, 0.1, 0.1]), ["dense", "sparse", "sparse"], P))
    return out


def production_case(seed=16):
    """two production pieces and 37 floats, about 100 MB, density 0.15 (a random mask: a permutation of 25 M places is slow)"""
    rng = np.random.default_rng(seed)
    n = 2 * PIECE + 37
    w = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    w[rng.random(n, dtype=np.float32) >= 0.15] = 0
    w[::100003] = 0x80000000
    return Case("production", "two_pieces_and_37", w, ["sparse"] * 3)


def sequence_cases(seed=17):
    """ten uploads for ONE context, in this order: lengths that grow, shrink and grow past the staging buffers' first allocation (a piece longer than
    the production one: the only way a staging buffer grows), another pattern on every call"""
    rng = np.random.default_rng(seed)
    big = 16 << 20
    plan = [(1000, 0, 0.3), (70001, 0, 0.1), (300000, SMALL_PIECE, 0.5), (5000, 0, 0.02), (37, 0, 0.4), (200000, SMALL_PIECE, 0.25),
            (PIECE + (1 << 20) + 5, big, 0.1), (4096, 0, 0.55), (70001, 0, 0.45), (2049, 0, 0.3)]
    out = []
    for i, (n, piece, d) in enumerate(plan):
        if n > PIECE:
            w = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            w[rng.random(n, dtype=np.float32) >= d] = 0
        else:
            w = by_density(rng, n, d)
        c = Case("sequence", "call%d_n%d" % (i, n), w, ["sparse"] * len(range(0, n, piece or PIECE)), piece)
        out.append(c)
    return out


def small_cases():
    """everything but the production-size image and the sequence"""
    return pattern_cases() + length_cases() + block_cases() + density_cases() + multi_piece_cases()


def expected_counters(case, dense_before=False):
    """(raw bytes, sent bytes, dense afterwards) of one upload of the case from what its pieces are meant to be: a packed piece is 64 mask words, one
    offset and one count per block of 2048 plus its non-zero words; a dense piece and every piece after it in the frame travel as they are"""
    sent, dense = 0, dense_before
    for (a, b), kind in zip(case.pieces(), case.kinds):
        if not dense and kind in ("dense", "edge_dense"):
            dense = True
        if dense:
            sent += 4 * (b - a)
        else:
            sent += 4 * (66 * ((b - a + BLOCK - 1) // BLOCK) + int(np.count_nonzero(case.words[a:b])))
    return 4 * case.words.size, sent, dense
