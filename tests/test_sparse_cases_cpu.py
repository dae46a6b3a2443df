"""CPU tests of tests/sparse_cases.py: the generator keeps the promises the GPU tests of the sparse upload rest on (tests/test_gpu_sparse_upload.py),
so that none of them passes by taking another path than the one its case names."""
import numpy as np

import sparse_cases as sc


def fractions(case):
    return [(b - a, int(np.count_nonzero(case.words[a:b]))) for a, b in case.pieces()]


def all_cases():
    return sc.small_cases() + sc.sequence_cases()


def test_every_piece_is_what_its_case_says():
    cases = all_cases()
    assert len(set(c.id for c in cases)) == len(cases)
    for c in cases:
        assert c.words.dtype == np.uint32 and c.words.ndim == 1 and c.piece % 4 == 0
        fr = fractions(c)
        assert len(fr) == len(c.kinds), c.id
        for (n, k), kind in zip(fr, c.kinds):
            if kind == "sparse":
                assert k * 100 <= n * 55, (c.id, n, k)
            elif kind == "dense":
                assert k * 100 >= n * 65, (c.id, n, k)
            elif kind == "edge_sparse":
                assert n % 5 == 0 and k * 5 == n * 3 and not k * 10 > n * 6, (c.id, n, k)
            elif kind == "edge_dense":
                assert n % 5 == 0 and k == n * 3 // 5 + 1 and k * 10 > n * 6, (c.id, n, k)
            else:
                raise AssertionError("unknown kind %r" % kind)


def test_the_production_size_case():
    c = sc.production_case()
    assert c.words.size == 2 * (12 << 20) + 37 and c.piece == 0
    assert [n for n, _ in fractions(c)] == [12 << 20, 12 << 20, 37]
    for n, k in fractions(c):
        assert k * 100 <= n * 55
    total = np.count_nonzero(c.words) / c.words.size
    assert 0.14 < total < 0.16
    assert c.words.nbytes < 101 * 2 ** 20


def test_the_cases_the_issue_lists_are_there():
    by = {}
    for c in all_cases():
        by.setdefault(c.group, []).append(c)
    assert sorted(c.words.size for c in by["lengths"]) == sorted([1, 3, 4, 5, 31, 32, 33, 2047, 2048, 2049, 16 * 2048 - 1, 16 * 2048 + 1, 5 * 16 * 2048 + 37])
    assert all(np.count_nonzero(c.words) > 0 for c in by["lengths"])
    # densities: 0, 0.01, 0.3, 0.55, 0.65, 1.0 and the two sides of the boundary, one piece of n divisible by 5 each
    got = sorted(np.count_nonzero(c.words) / c.words.size for c in by["densities"])
    n = sc.EDGE_N
    want = sorted([0.0, 0.01, 0.3, 0.55, 0.65, 1.0, 0.6, (0.6 * n + 1) / n])
    assert n % 5 == 0 and np.allclose(got, want, atol=0.6 / n) and all(len(c.kinds) == 1 and c.words.size == n for c in by["densities"])
    assert [c.kinds[0] for c in by["densities"] if c.kinds[0].startswith("edge")] == ["edge_sparse", "edge_dense"]
    # multi-piece: 7 pieces + a ragged tail; sparse, dense, sparse
    m = {c.name: c for c in by["multi"]}
    assert all(c.piece == 65536 for c in by["multi"])
    seven = m["seven_pieces_ragged_tail"]
    assert len(seven.pieces()) == 8 and seven.words.size % 65536 not in (0,) and seven.words.size % 4 != 0 and seven.words.size % 32 != 0
    assert m["sparse_dense_sparse"].kinds == ["sparse", "dense", "sparse"] and len(m["sparse_dense_sparse"].pieces()) == 3
    # the sequence: ten calls, lengths that grow, shrink and grow past the production piece (the staging buffers' first allocation)
    seq = by["sequence"]
    sizes = [c.words.size for c in seq]
    assert len(seq) == 10 and sizes[1] > sizes[0] and sizes[3] < sizes[2] and max(sizes) > sc.PIECE and sizes.index(max(sizes)) not in (0, 9)
    big = seq[sizes.index(max(sizes))]
    assert big.piece > big.words.size                     # one piece longer than the production piece: the staging buffer has to grow
    assert len(set(c.words[:37].tobytes() for c in seq)) == 10


def test_bit_patterns():
    sp = sc.SPECIAL
    f = sp.view(np.float32)
    assert 0 not in sp and len(set(sp.tolist())) == sp.size
    assert 0x80000000 in sp and 0x00000001 in sp and 0xFFFFFFFF in sp
    with np.errstate(invalid="ignore"):
        assert np.isposinf(f).sum() == 1 and np.isneginf(f).sum() == 1
    nan = np.isnan(f)
    quiet = (sp & 0x00400000) != 0
    assert (nan & quiet).sum() >= 3 and (nan & ~quiet).sum() >= 3 and ((sp[nan] & 0x003FFFFF) != 0).sum() >= 4        # payloads
    denormal = ((sp & 0x7F800000) == 0) & ((sp & 0x007FFFFF) != 0)
    assert denormal.sum() >= 3
    pats = {c.name: c for c in sc.pattern_cases()}
    w = pats["every_pattern_every_lane"].words
    idx = np.nonzero(w)[0]
    seen = set(zip(w[idx].tolist(), (idx % 32).tolist()))
    assert len(seen) == sp.size * 32                      # every pattern at every lane position of a 32-word group
    assert set(np.unique(pats["random_places"].words).tolist()) == set(sp.tolist()) | {0}
    assert np.count_nonzero(pats["block_of_negative_zero"].words) == sc.BLOCK


def test_block_shapes():
    b = {c.name: c for c in sc.block_cases()}
    assert not b["all_zero"].words.any() and b["all_zero"].words.size > 2 * sc.BLOCK
    nz = (b["full_between_empty"].words.reshape(-1, sc.BLOCK) != 0).sum(1)
    assert set(nz.tolist()) == {0, sc.BLOCK}
    for lead in (1, 2, 3):
        c = b["full_after_%d" % lead]
        assert c.words.size <= sc.TASK                    # one packing task: the order of the stream is the order of the blocks
        nz = (c.words.reshape(-1, sc.BLOCK) != 0).sum(1)
        assert nz[0] == lead and nz[1] == sc.BLOCK        # a full window directly after `lead` values
        assert sc.stream_offsets_of_full_blocks(c.words) == [0, 1, 2, 3]
        assert 0 in nz[2:]                                # and blocks without values (nv = 0) at stream offsets of every kind
    last = b["only_the_last_word"].words
    assert np.count_nonzero(last) == 1 and last[-1] != 0 and last.size % 4 != 0


def test_expected_counters_follow_the_documented_format():
    """64 mask words + one offset + one count per block of 2048, plus the values; a dense piece and all after it as they are"""
    c = {x.name: x for x in sc.multi_piece_cases()}["sparse_dense_sparse"]
    P = 65536
    k0 = int(np.count_nonzero(c.words[:P]))
    assert sc.expected_counters(c) == (4 * 3 * P, 4 * (66 * 32 + k0) + 4 * P + 4 * P, True)
    assert sc.expected_counters(c, dense_before=True) == (4 * 3 * P, 4 * 3 * P, True)
    one = sc.Case("x", "y", np.array([0, 5, 0], np.uint32), ["sparse"])
    assert sc.expected_counters(one) == (12, 4 * (66 + 1), False)
