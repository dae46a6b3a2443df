"""CPU tests (no GPU) of tests/pyramid_ref.py and tests/pyramid_cases.py: the float32 restatements equal the oracle -- and, where they are built, the
reference's compiled units, and the reference-generated fixture -- bit for bit on every constructed case; each lies within a DERIVED bound of its
float64 form; and the cases hold what their table claims: every mutant changes a bit of every case named for it, every launcher branch has a catching
case for every mutant of its operation, and the index-coded images decode to the expected source positions."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import pyramid_cases as pc
import pyramid_ref as pr

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and not pr.bits_differ(a, b)


def library_ops(ops):
    return {"dsum": ops["dsum"], "davg": ops["davg"], "dcov": ops["dcov"], "interp": ops["interp"], "merge": ops["merge"]}


def check_against(ops):
    bad = []
    for op, fam, W, H, D, inputs in pc.pyramid_cases():
        if not bits_equal(pr.run(op, inputs), library_ops(ops)[op](*inputs)):
            bad.append((op, fam, W, H, D))
    assert not bad, bad[:10]


def test_restatements_equal_the_oracle_bit_for_bit():
    check_against(ol.oracle_ops())


@pytest.mark.skipif(not ol.ref_available(), reason="oracle/_ref not built (the reference-generated fixture of the next test pins the same operations)")
def test_restatements_equal_the_reference_units_bit_for_bit():
    check_against(ol.ref_ops())


def test_restatements_equal_the_reference_generated_fixture():
    f = np.load(os.path.join(GOLDEN, "ref_pyramid.npz"))
    H, W, _ = f["mean"].shape
    assert bits_equal(pr.downscale_sum(f["hist"]), f["dsum_hist"])
    assert bits_equal(pr.downscale_sum(f["ns"]), f["dsum_ns"])
    assert bits_equal(pr.downscale_avg(f["mean"]), f["davg_mean"])
    assert bits_equal(pr.downscale_cov(f["cov"], f["ns"]), f["dcov"])
    up = pr.interpolate(f["davg_mean"], H, W)
    assert bits_equal(up, f["interp"])
    assert bits_equal(pr.merge(f["mean"], pr.downscale_avg(up)), f["merge"])


def test_flat_restatements_equal_the_oracle_bit_for_bit():
    o = ol.oracle()
    for op, n, inputs, _ in pc.flat_cases():
        if op == "pixcov":
            cov, ns = inputs
            want = np.empty_like(cov)
            o.bcdo_pixel_cov_from_sample_cov(ol._fp(cov), ol._fp(ns), n, 1, ol._fp(want))
        else:
            s, cnt = inputs
            want = np.empty_like(s)
            o.bcdo_finalize(ol._fp(s), cnt.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(n), ol._fp(want))
        assert bits_equal(pr.run(op, inputs), want), (op, n)


def test_zero_bad_restatement_equals_the_oracle_and_keeps_what_it_claims():
    o = ol.oracle()
    for n in pc.ZERO_BAD_LENGTHS:
        for turn in range(pc.ZERO_BAD_SPECIALS.size if n == 1 else 3):
            bits = pc.zero_bad_vector(n, turn)
            want = bits.copy()
            o.bcdo_zero_bad_values(want.view(F32).ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(n))
            got = pr.zero_bad(bits.view(F32)).view(np.uint32)
            assert np.array_equal(got, want), (n, turn)
            assert np.all((want == bits) | (want == 0))                   # a value is kept with all its bits or becomes +0
    bits = pc.ZERO_BAD_SPECIALS
    out = dict(zip(bits.tolist(), pr.zero_bad(bits.view(F32)).view(np.uint32).tolist()))
    kept = [0x00000000, 0x80000000, 0x00000001, 0x00800000, 0x7F7FFFFF, 0x3FC00000, 0x00200000]      # -0.0 among them
    assert all(out[b] == b for b in kept)
    assert all(out[b] == 0 for b in bits.tolist() if b not in kept)       # the negative denormals, every NaN of either sign, both infinities


# ---- float32 against float64: derived bounds ----------------------------------------------------------------------------------------------------------
def within(got32, want64, bound, tag):
    """|float32 - float64| <= bound wherever the float64 value is finite; elsewhere the same non-finite value"""
    ok = np.isfinite(want64)
    with np.errstate(all="ignore"):
        err = np.abs(got32.astype(F64) - want64)
    assert np.all(err[ok] <= bound[ok]), (tag, float(np.max(err[ok] / np.maximum(bound[ok], 1e-300))))
    assert np.array_equal(np.isnan(got32[~ok]), np.isnan(want64[~ok])) and np.array_equal(got32[~ok][~np.isnan(got32[~ok])], want64[~ok][~np.isnan(want64[~ok])]), tag


def test_float32_restatements_within_derived_bounds_of_float64():
    """The bound of a sum of terms is gamma(n) * (the sum of the absolute terms in float64), n = the roundings on the longest path of a term through the
    float32 expression and gamma(n) = n u / (1 - n u), u = 2^-24 (pyramid_ref.gamma).  No case underflows (magnitudes 2^-36 ... 2^25), so no absolute
    term is needed.  Nothing here is a measured number:
      dsum, davg   ((p1 + p2) + p3) + p4: p1 passes 3 additions; the factor 0.25 is exact                                              n = 3
      interp       (wm p1 + wa (p2 + p3)) + wd p4 with exact weights: p2 passes its sum, its product and 2 additions                    n = 4
      merge        (hi - up(a)) + up(b), a = davg(hi): 3 for the average, 4 through the interpolation, 2 for the two outer operations   n = 9
      dcov         w_i = (1/16) nSum / n_i: 3 additions of non-negative counts (no cancellation: a relative error), an exact factor,
                   1 division; then 1 product and up to 3 additions                                                                     n = 8
      pixcov       1 / n and one product                                                                                                n = 2
      finalize     the conversion of the count, 1 / count and one product                                                               n = 3"""
    with np.errstate(all="ignore"):
        for op, fam, W, H, D, inputs in pc.pyramid_cases():
            got, want = pr.run(op, inputs), pr.run(op, inputs, dtype=F64)
            if op in ("dsum", "davg"):
                terms = pr.downscale_sum(np.abs(inputs[0]), F64) * (1.0 if op == "dsum" else 0.25)
                n = 3
            elif op == "interp":
                (wm, wa, wd), p = pr.interpolate_terms(np.abs(inputs[0]), H, W, F64)
                terms, n = wm * p[0] + wa * (p[1] + p[2]) + wd * p[3], 4
            elif op == "merge":
                terms, n = pr.merge_abs_terms(*inputs), 9
            else:
                w, c = pr.downscale_cov_terms(np.abs(inputs[0]), inputs[1], F64)
                terms, n = sum(wi * ci for wi, ci in zip(w, c)), 8
            within(got, want, pr.gamma(n) * terms, (op, fam, W, H, D))
        for op, npix, inputs, _ in pc.flat_cases():
            got, want = pr.run(op, inputs), pr.run(op, inputs, dtype=F64)
            within(got, want, pr.gamma(2 if op == "pixcov" else 3) * np.abs(want), (op, npix))


# ---- the cases hold what they claim ---------------------------------------------------------------------------------------------------------------
def test_every_mutant_changes_every_case_named_for_it_and_every_branch_has_a_catching_case():
    caught = set()       # (op, depth, mutant)
    missed = []
    for op, fam, W, H, D, inputs in pc.pyramid_cases(families=("index", "order")):
        want = pr.run(op, inputs)
        for m in pr.MUTANTS:
            if pc.named(m, op, fam, W, H):
                if pr.bits_differ(pr.run(op, inputs, **pr.MUTANTS[m]), want):
                    caught.add((op, D, m))
                else:
                    missed.append((m, op, fam, W, H, D))
    for op, npix, inputs, divide_named in pc.flat_cases():
        if divide_named:
            if pr.bits_differ(pr.run(op, inputs, divide=True), pr.run(op, inputs)):
                caught.add((op, inputs[0].shape[-1], "divide"))
            else:
                missed.append(("divide", op, npix))
    assert not missed, missed[:10]
    uncaught = [(b, D, m) for b, (op, depths) in pc.BRANCHES.items() for D in depths for m in pr.MUTANTS
                if op in pr.MUTANT_OPS[m] and (op, D, m) not in caught]
    assert not uncaught, uncaught[:10]
    assert all(any(op in pr.MUTANT_OPS[m] for op, _ in pc.BRANCHES.values()) for m in pr.MUTANTS)      # no mutant without a branch to catch it in


def test_every_value_of_an_order_level_is_sensitive_to_the_association():
    for (W, H) in pc.SIZES:
        for D in (1, 4, 9, 60):
            a = pc.level("order", W, H, D)
            want = pr.downscale_sum(a).view(np.uint32)
            for m in pc.ASSOCIATIONS:
                assert np.all(pr.downscale_sum(a, **pr.MUTANTS[m]).view(np.uint32) != want), (W, H, D, m)
            e = np.frexp(a)[1]
            assert e.min() >= -11 and e.max() <= 13 and (D * W * H < 200 or (e.min() <= -9 and e.max() >= 11))       # spread over about 2^+-12


def _block_positions_scalar(W, H):
    """MultiscaleDenoiser.cpp:256-266, pixel by pixel"""
    out = np.empty((H // 2, W // 2, 4, 2), np.int64)
    for l in range(H // 2):
        for c in range(W // 2):
            l1, c1 = min(2 * l + 1, H - 1), min(2 * c + 1, W - 1)
            out[l, c] = [(2 * l, 2 * c), (l1, 2 * c), (2 * l, c1), (l1, c1)]
    return out


def _interp_positions_scalar(W, H, w, h):
    """MultiscaleDenoiser.cpp:473-512, pixel by pixel"""
    clamp = lambda v, n: 0 if v <= 0 else (n - 1 if v >= n else v)
    out = np.empty((H, W, 4, 2), np.int64)
    for ul in range(H):
        for uc in range(W):
            l, c = ul // 2, uc // 2
            al, ac = clamp(l + ((ul % 2) * 2 - 1), h), clamp(c + ((uc % 2) * 2 - 1), w)
            lc, cc = max(0, min(l, h - 1)), max(0, min(c, w - 1))
            out[ul, uc] = [(lc, cc), (lc, ac), (al, cc), (al, ac)]
    return out


@pytest.mark.parametrize("W,H", pc.SIZES)
def test_index_coded_images_decode_to_the_expected_source_positions(W, H):
    w, h = W // 2, H // 2
    blocks, interp = _block_positions_scalar(W, H), _interp_positions_scalar(W, H, w, h)
    assert np.array_equal(pr.block_positions(W, H), blocks) and np.array_equal(pr.interp_positions(W, H, w, h), interp)
    assert len({v for v in pc.level("index", W, H, 60).ravel().tolist()}) == W * H * 60             # every (l, c, z) holds a distinct value
    for D in pc.DEPTHS:
        hi, lo = pc.level("index", W, H, D), pc.coarse("index", W, H, D)
        for out, scale in ((pr.downscale_sum(hi), 1), (pr.downscale_avg(hi), 4)):
            sl, sc = pc.decode(out, scale, 4)
            # a block is {2l, b} x {2c, e}, every line and every column twice: from the sums and the output's own position, b and e
            b = sl // 2 - blocks[:, :, 0, 0][..., None]
            e = sc // 2 - blocks[:, :, 0, 1][..., None]
            for z in range(D):
                got = np.stack([np.stack([blocks[:, :, 0, 0], blocks[:, :, 0, 1]], -1), np.stack([b[..., z], blocks[:, :, 0, 1]], -1),
                                np.stack([blocks[:, :, 0, 0], e[..., z]], -1), np.stack([b[..., z], e[..., z]], -1)], 2)
                assert np.array_equal(got, blocks) and np.all(sl[..., z] % 2 == 0) and np.all(sc[..., z] % 2 == 0), (D, z, scale)
        sl, sc = pc.decode(pr.interpolate(lo, H, W), 16, 16)
        # weights 9, 3, 3, 1: the main line weighs 12, the adjacent one 4 and lies at most one line away: sl = 16 main + 4 (adjacent - main)
        ml, mc = (sl + 4) // 16, (sc + 4) // 16
        assert np.all((sl - 16 * ml) % 4 == 0) and np.all((sc - 16 * mc) % 4 == 0)
        al, ac = ml + (sl - 16 * ml) // 4, mc + (sc - 16 * mc) // 4
        for z in range(D):
            got = np.stack([np.stack([ml[..., z], mc[..., z]], -1), np.stack([ml[..., z], ac[..., z]], -1),
                            np.stack([al[..., z], mc[..., z]], -1), np.stack([al[..., z], ac[..., z]], -1)], 2)
            assert np.array_equal(got, interp), (D, z)
        # a wrong channel or a source outside the table is no code at all
        if D > 1:
            with pytest.raises(ValueError):
                pc.decode(np.roll(pr.downscale_sum(hi), 1, axis=-1), 1, 4)


def test_special_cases_hold_what_they_claim():
    for (W, H) in pc.SIZES:
        a = pc.level("nonfinite", W, H, 3)
        assert not np.isfinite(a[[0, 0, H - 1], [0, W - 1, 0]]).all(-1).any() and (np.signbit(a[H - 1, W - 1]) & (a[H - 1, W - 1] == 0)).any(), (W, H)   # the corners
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and (np.signbit(a) & (a == 0)).any(), (W, H)
        ns = pc.sample_counts("zero", W, H)
        n4 = pr._gather4(ns)
        assert any((n == 0).any() for n in n4)                                                     # a 0 inside a 2x2 block
        mixed = pr._gather4(pc.sample_counts("mixed", W, H))
        assert all(np.all(mixed[i] != mixed[j]) for i in range(4) for j in range(i))               # the four counts of every block differ
        with np.errstate(all="ignore"):
            out = pr.downscale_cov(*pc.covariances("zero", W, H))
        assert np.isinf(out).any() or np.isnan(out).any()
    for n in pc.FLAT:
        seen = set()
        for turn in range(4):
            s, cnt = pc.finalize_case(n, turn)
            seen |= set(cnt.tolist())
            assert cnt[0] == pc.FINALIZE_COUNTS[turn]
        assert set(pc.FINALIZE_COUNTS) <= seen
    assert np.float32((1 << 24) + 1) == np.float32(1 << 24)                                        # the conversion of that count rounds
