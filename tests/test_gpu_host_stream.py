"""The streamed schedule of bcd_hip_denoise_host_ex (host_stream_frame in bcd_amd/csrc/bcd_host.hip) on its own: the frame arrives in row chunks, the
lines that have arrived are prefiltered and the finest scale's approximate distance planes are launched for the tile rows whose lines are complete.

bcd_hip_selftest_host_stream runs that function -- the one a frame runs -- stops it after k chunks and fills every buffer it touches with 0xFF bytes
first.  Expected progress is computed HERE from two dependency statements, not taken from the code:
    a filtered line r reads the input lines r - 1 .. r + 1, clamped inward at the frame border;
    tile row t of the planes reads the histogram lines [4 t, min(H, 4 t + 4 + b)).
The progress reported must be the LARGEST these allow for the lines that have arrived (so the streaming cannot quietly degrade to "everything after the
last chunk"), and what is claimed must equal, bit for bit, Context.spike_filter and ONE launch of the full-frame plane launcher (bcd_hip_approx_planes) on
the resident frame -- a line claimed too early has read 0xFF bytes and cannot match; what is not claimed must still hold the 0xFF bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP = 16
TILE = 4


def rebin(hist, D):
    """the 3 x 20 bins of the synthetic scene as 3 x (D / 3): the last bin takes the rest (non-negative, same sums)"""
    H, W, _ = hist.shape
    nb = D // 3
    h = hist.reshape(H, W, 3, 20)
    out = h[..., :nb].copy()
    out[..., nb - 1] = h[..., nb - 1:].sum(-1)
    return np.ascontiguousarray(out.reshape(H, W, D))


_frames = {}


def frame(W, H, D, seed, mixed):
    key = (W, H, D, seed, mixed)
    if key not in _frames:
        import bcd_amd.core as core
        col, ns, hist, cov = core.synthetic_scene(W, H, SPP, seed, 0.2, 0.01)
        hist = rebin(hist, D) if D != 60 else hist
        if mixed == "decline":                               # 160 or 10 240 samples per pixel at random: the RATIO form's error bound fails on such a spread
            scale = np.where(np.random.default_rng(seed).random((H, W, 1)) < 0.5, 640.0, 10.0).astype(np.float32)
            ns, hist = ns * scale, hist * scale
        elif mixed:                                          # half the frame carries 12 samples: no uniform count.  True: the upper half, so the first pixel's
            ns = ns.copy(); hist = hist.copy()               # count is no power of two; "late": the lower half -- the first pixel says 16 and only the host's
            rows = slice(H // 2, H) if mixed == "late" else slice(0, H // 2)   # strided look at the counts finds the frame mixed
            ns[rows] = 12.0
            hist[rows] *= np.float32(0.75)
        _frames[key] = tuple(np.ascontiguousarray(a, np.float32) for a in (col, ns, hist, cov))
    return _frames[key]


def dev(*arrs):
    import torch
    return [torch.from_numpy(a).cuda() for a in arrs]


def same_bits(a, b):
    import torch
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def all_ff(a):
    import torch
    return bool((a.contiguous().view(torch.uint8) == 0xFF).all())


def expected_progress(H, b, arrived, prefilter):
    """(lines filtered, tile rows of planes) the two dependency statements allow once the input lines [0, arrived) are there"""
    have = lambda line: line < arrived
    usable = arrived
    if prefilter:
        usable = 0
        while usable < H and have(max(usable - 1, 0)) and have(usable) and have(min(usable + 1, H - 1)):
            usable += 1
    tiles = 0
    while tiles * TILE < H and min(H, TILE * tiles + TILE + b) <= usable:
        tiles += 1
    return (usable if prefilter else 0), tiles


_resident = {}


def resident(hipctx, key, imgs, b, spike_factor, uni_n, ratio_form, tau):
    """the single-launch answers on the resident frame, computed once per configuration"""
    k = key + (b, spike_factor)
    if k not in _resident:
        d = dev(*imgs)
        if spike_factor > 0:
            d = hipctx.spike_filter(*d, spike_factor)
        planes, counts, flag = hipctx.approx_planes(d[2], d[1], b, uni_n, ratio_form=ratio_form, tau=tau)
        _resident.clear()                                    # (one configuration at a time: the planes of the large shapes are tens of MB)
        _resident[k] = (d, planes, counts, flag)
    return _resident[k]


# (W, H, b, D, mixed sample counts, sweep every stop)
CONFIGS = [(40, 256, 3, 60, False, False), (65, 257, 6, 36, False, True), (64, 300, 12, 24, False, False), (130, 520, 6, 60, False, False),
           (40, 256, 12, 36, False, False), (65, 257, 3, 24, False, False), (64, 300, 6, 60, False, False), (130, 520, 12, 24, False, False),
           (65, 257, 12, 60, True, False), (64, 300, 3, 36, "late", False), (40, 256, 6, 24, True, False), (130, 520, 3, 36, "late", False),
           (48, 264, 6, 60, "decline", False)]


@pytest.mark.parametrize("spike_factor", [0.0, 2.0], ids=["plain", "prefilter"])
@pytest.mark.parametrize("W,H,b,D,mixed,sweep", CONFIGS, ids=["%dx%d-b%d-D%d%s" % (c[0], c[1], c[2], c[3], {False: "", True: "-mixed"}.get(c[4], "-%s" % c[4])) for c in CONFIGS])
def test_schedule_claims_exactly_what_has_arrived_and_computes_it_bit_for_bit(hipctx, W, H, b, D, mixed, sweep, spike_factor):
    import bcd_amd.hip as bh
    key = (W, H, D, 100 + W + H, mixed)
    imgs = frame(*key)
    prm = bh.default_params(b=b)
    prefilter = spike_factor > 0
    want_uni = 0.0 if mixed else float(SPP)
    # general sample counts travel through the RATIO form of the kernel, as on a resident frame: its planes from one launch, its verdict (flag value 4) once
    # the last tile row is in.  The "decline" frame is one whose verdict fails: bit 2 must be there with all chunks in, as after the single launch, and
    # only then.  (This entry point never goes on to similarity(), so the workspace does not remember the size as declined.)
    ref_imgs, ref_planes, ref_counts, ref_flag = resident(hipctx, key, imgs, b, spike_factor, want_uni, bool(mixed), prm.hist_dist_threshold)
    assert ref_flag == (4 if mixed == "decline" else 0)
    probe = hipctx.selftest_host_stream(*imgs, prm, spike_factor=spike_factor, stop_after_chunks=0)
    chunk = probe["chunk_lines"]
    assert chunk >= 64 and chunk % TILE == 0 and probe["chunks_done"] == 0 and probe["rows_filtered"] == 0 and probe["tile_rows_done"] == 0
    assert all_ff(probe["planes"]) and all_ff(probe["counts"]) and all_ff(probe["images"][2]) and all_ff(probe["hist_uploaded"])
    nchunks = (H + chunk - 1) // chunk
    assert 4 <= nchunks <= 9
    if H == 257:
        assert H - (nchunks - 1) * chunk == 1              # the frame ends in a chunk of one line
    stops = range(1, nchunks + 1) if sweep else sorted({1, nchunks - 1, nchunks})
    for k in stops:
        got = hipctx.selftest_host_stream(*imgs, prm, spike_factor=spike_factor, stop_after_chunks=(k if k < nchunks else -1))
        arrived = min(H, k * chunk)
        rows, tiles = expected_progress(H, b, arrived, prefilter)
        where = "after %d of %d chunks (%d lines)" % (k, nchunks, arrived)
        assert (got["chunks_done"], got["chunk_lines"]) == (k, chunk), where
        assert (got["rows_filtered"], got["tile_rows_done"]) == (rows, tiles), where
        if k == nchunks:
            assert tiles == (H + TILE - 1) // TILE and (rows == H or not prefilter)
        assert got["uni_n"] == want_uni and got["ratio_form"] == (1 if mixed else 0), where
        assert got["range_flag"] == (ref_flag if k == nchunks else ref_flag & ~4), where
        # the images the planes are computed on: filtered lines [0, rows) with the prefilter, else the uploaded copies
        hist_lines = arrived
        if prefilter:
            for g, r in zip(got["images"], ref_imgs):
                assert same_bits(g[:rows], r[:rows]), where
                assert all_ff(g[rows:]), where
        else:
            for i, (g, r) in enumerate(zip(got["images"], ref_imgs)):
                n = hist_lines if i == 2 else H              # (colours, counts and covariances travel whole beside the first chunk)
                assert same_bits(g[:n], r[:n]), where
                assert all_ff(g[n:]), where
        up = got["hist_uploaded"]
        host_hist = dev(imgs[2])[0]
        assert same_bits(up[:hist_lines], host_hist[:hist_lines]) and all_ff(up[hist_lines:]), where
        # the planes: tile rows [0, tiles) as ONE launch on the resident frame computes them, the rest untouched
        lines = min(H, TILE * tiles)
        assert same_bits(got["planes"][:, :lines], ref_planes[:, :lines]), where
        assert same_bits(got["counts"][:, :lines], ref_counts[:, :lines]), where
        assert all_ff(got["planes"][:, lines:]) and all_ff(got["counts"][:, lines:]), where
    assert k == nchunks


def test_expected_progress_is_the_dependency_statements():
    """(the helper itself, on cases small enough to enumerate by hand)"""
    assert expected_progress(10, 3, 0, True) == (0, 0) and expected_progress(10, 3, 0, False) == (0, 0)
    assert expected_progress(10, 3, 5, True) == (4, 0)      # lines 0 .. 3 have all their neighbours; tile row 0 needs lines [0, 7)
    assert expected_progress(10, 3, 8, True) == (7, 1)      # tile row 0: [0, 7) filtered; tile row 1 needs [4, 10)
    assert expected_progress(10, 3, 8, False) == (0, 1)
    assert expected_progress(10, 3, 10, True) == (10, 3)    # the last line is clamped inward: complete once the frame is
    assert expected_progress(10, 3, 10, False) == (0, 3)
    assert expected_progress(257, 6, 256, True) == (255, 62) and expected_progress(257, 6, 256, False) == (0, 61 + 1)
    assert expected_progress(257, 6, 257, False) == (0, 65)


# ---- whole calls at streaming size

def rel_linf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def integer_stats(ctx, scales):
    out = []
    for s in range(scales):
        st = ctx.stats(s)
        out.append((st.processed, st.fallback, st.spectral_inverses, st.similarity_path, st.borderline_pairs))
    return out


def predicted_upload_bytes(hist, chunk):
    """(raw, sent) of a frame whose histogram lines travel in chunks of `chunk` lines, one piece each (every chunk here is far below 12 Mi floats): a
    chunk with more than 60 % of non-zero words, and every chunk after it, travels as it is; a packed chunk is 66 words per block of 2048 + its values"""
    H = hist.shape[0]
    words = hist.view(np.uint32)
    sent, dense = 0, False
    for r0 in range(0, H, chunk):
        part = words[r0:r0 + chunk]
        n, nz = part.size, int(np.count_nonzero(part))
        assert n < (12 << 20) and not 0.55 * n < nz < 0.65 * n  # (the frames of this test stay away from the boundary)
        dense = dense or nz * 10 > n * 6
        sent += 4 * n if dense else 4 * (66 * ((n + 2047) // 2048) + nz)
    return 4 * words.size, sent


def whole_call(ctx, W, H, D, scales, spike_factor, mixed, seed, chunk=None):
    """one frame through denoise_host and through denoise on resident (filtered) inputs -> everything the tests below compare"""
    import bcd_amd.hip as bh
    imgs = frame(W, H, D, seed, mixed)
    prm = bh.default_params(m=1.0, random_order=1, seed=seed)
    if chunk is None:                                        # the chunk length of this geometry (the probe leaves 0xFF bytes in the device copies)
        chunk = ctx.selftest_host_stream(*imgs, prm, spike_factor=spike_factor, stop_after_chunks=0)["chunk_lines"]
    got = ctx.denoise_host(*imgs, scales, prm, spike_factor=spike_factor)
    stats_host = integer_stats(ctx, scales)
    upload = ctx.last_upload_bytes()
    d = dev(*imgs)
    if spike_factor > 0:
        d = ctx.spike_filter(*d, spike_factor)
    want = ctx.denoise(*d, scales, prm).cpu().numpy()
    stats_resident = integer_stats(ctx, scales)
    return {"got": got, "want": want, "host": stats_host, "resident": stats_resident, "upload": upload, "predicted": predicted_upload_bytes(imgs[2], chunk),
            "chunk": chunk}


def check_whole_call(r):
    assert r["host"] == r["resident"]                        # processed, fallback, spectral inverses, similarity path, borderline pairs: every scale
    assert r["host"][0][3] in (1, 2)                         # (the finest scale stayed on the approximate planes the upload computed)
    assert rel_linf(r["got"], r["want"]) < 1e-5              # (the order of the float atomics: test_streamed_host_upload_equals_the_resident_path)
    assert r["upload"] == r["predicted"] and r["upload"][1] < r["upload"][0]


WHOLE = [(40, 256, 60, 1, 0.0, False, 21), (90, 330, 36, 3, 2.0, False, 22), (64, 300, 60, 2, 0.0, True, 23), (77, 257, 36, 2, 2.0, "late", 24)]
WHOLE_IDS = ["%dx%d-D%d-S%d%s%s" % (c[0], c[1], c[2], c[3], "-prefilter" if c[4] else "", {False: "", True: "-mixed"}.get(c[5], "-%s" % c[5])) for c in WHOLE]


@pytest.mark.parametrize("case", WHOLE, ids=WHOLE_IDS)
def test_whole_call_at_streaming_size_equals_the_resident_path(hipctx, case):
    """colours within 1e-5, the integer statistics of every scale -- the similarity path among them: with mixed sample counts both paths run the RATIO form of
    the distance kernel (2), the host path in row partitions with the verdict behind the last one -- and the upload byte counters as the rule predicts"""
    r = whole_call(hipctx, *case)
    check_whole_call(r)
    assert r["host"][0][3] == (2 if case[5] else 1)


def test_a_declined_ratio_verdict_on_the_streamed_path_repeats_the_pass_and_is_remembered():
    """a streamed frame whose counts spread 1 : 64 (the frame of test_ratio_form_declines_... at streaming size), on contexts that have not met it: the
    planes launched ahead take the RATIO form, its verdict behind the last tile row declines, similarity() repeats the pass with the reference's
    operations -- statistics and similarity_path (1 after the redo) as on the resident path, colours within 1e-5 -- and the workspace remembers the size:
    the next host frame of this size is launched with the reference's operations from its first chunk"""
    import bcd_amd.hip as bh
    W, H, D, seed = 48, 264, 60, 41
    imgs = frame(W, H, D, seed, "decline")
    prm = bh.default_params(m=1.0, random_order=1, seed=seed)
    host, res = bh.Context(0), bh.Context(0)
    try:
        probe = lambda: host.selftest_host_stream(*imgs, prm, stop_after_chunks=0)
        assert (probe()["uni_n"], probe()["ratio_form"]) == (0.0, 1)
        got = host.denoise_host(*imgs, 1, prm)
        stats_host = integer_stats(host, 1)
        assert probe()["ratio_form"] == 0                    # declined and remembered: only the verdict of the streamed launches can have said so
        d = dev(*imgs)
        _, _, flag = res.approx_planes(d[2], d[1], prm.search_radius, 0.0, ratio_form=True, tau=prm.hist_dist_threshold)
        assert flag == 4                                     # (the frame does decline)
        want = res.denoise(*d, 1, prm).cpu().numpy()
        assert stats_host == integer_stats(res, 1) and stats_host[0][3] == 1
        assert rel_linf(got, want) < 1e-5
        again = host.denoise_host(*imgs, 1, prm)             # the second host frame: the reference's operations ahead of the last chunk, no redo
        assert integer_stats(host, 1) == stats_host and rel_linf(again, want) < 1e-5
    finally:
        host.close()
        res.close()


def test_two_frames_back_to_back_on_one_context():
    """same size, different content, one context: the device copies still hold the first frame when the second one streams in"""
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        a = whole_call(ctx, 56, 288, 60, 2, 2.0, False, 31)
        b = whole_call(ctx, 56, 288, 60, 2, 2.0, False, 32, chunk=a["chunk"])     # (no probe in between: nothing clears the first frame's lines)
        check_whole_call(a)
        check_whole_call(b)
        assert rel_linf(a["got"], b["got"]) > 1e-3           # (different content)
    finally:
        ctx.close()
