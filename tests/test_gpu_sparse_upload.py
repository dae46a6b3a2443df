"""The sparse histogram upload (bcd_amd/csrc/bcd_sparse_upload.hip) on its own, bit for bit: bcd_hip_selftest_sparse_upload sends a host image through
the context's uploader -- the packers, the task stream, the rotating staging buffers, the dense decision, k_sparse_unpack -- and the device copy must
hold the SAME BITS, the words either side of it must be untouched and the byte counters must say what travelled in which form.  The images and what
their pieces are meant to be come from tests/sparse_cases.py (held to its promises by tests/test_sparse_cases_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sparse_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                      # words either side of the destination (a multiple of 4: the destination keeps the allocation's alignment)
SENTINEL = 0xA5A5A5A5


def first_difference(got, want):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else "%d of %d words differ, first at %d: got %08x, want %08x" % (bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def upload_checked(ctx, case, new_frame=True, misalign=0):
    """uploads the case into a slice of a larger tensor; asserts the bits and the guards; -> the frame's (raw, sent) counters"""
    import torch
    n = case.words.size
    big = torch.full((GUARD + misalign + n + GUARD,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    assert big.data_ptr() % 16 == 0
    dst = big[GUARD + misalign:GUARD + misalign + n].view(torch.float32)
    assert dst.data_ptr() % 16 == 4 * misalign
    torch.cuda.synchronize()
    _, counters = ctx.selftest_sparse_upload(case.words, dst, new_frame=new_frame, piece_floats=case.piece)
    got = big.cpu().numpy().view(np.uint32)
    lo, hi = GUARD + misalign, GUARD + misalign + n
    assert (got[:lo] == SENTINEL).all(), "%s: words in front of the destination were written" % case.id
    assert (got[hi:] == SENTINEL).all(), "%s: words behind the destination were written" % case.id
    diff = first_difference(got[lo:hi], case.words)
    assert diff is None, "%s: %s" % (case.id, diff)
    return counters


SMALL = sc.small_cases()


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_uploaded_bits_guards_and_counters(hipctx, case):
    raw, sent = upload_checked(hipctx, case)
    want_raw, want_sent, _ = sc.expected_counters(case)
    assert (raw, sent) == (want_raw, want_sent)
    packed_all = all(k in ("sparse", "edge_sparse") for k in case.kinds)
    if packed_all and case.words.size >= 5 * sc.BLOCK and np.count_nonzero(case.words) * 2 < case.words.size:
        assert sent < raw                                    # (the packed form is the smaller one where it is chosen on an image of some size)


@pytest.mark.parametrize("name", ["sparse_dense_sparse", "dense_first", "seven_pieces_ragged_tail"])
def test_dense_decision_is_sticky_within_a_frame_and_forgotten_by_the_next(hipctx, name):
    """the third piece of (sparse, dense, sparse) travels plain; the same image as a NEW frame gives the same counters again (the decision was reset); the
    same image as a continuation of the frame adds to the counters and -- once the frame is dense -- travels plain from its first piece"""
    case = {c.name: c for c in sc.multi_piece_cases()}[name]
    raw1, sent1, dense1 = sc.expected_counters(case)
    assert upload_checked(hipctx, case) == (raw1, sent1)
    assert upload_checked(hipctx, case) == (raw1, sent1)
    raw2, sent2, _ = sc.expected_counters(case, dense_before=dense1)
    assert upload_checked(hipctx, case, new_frame=False) == (raw1 + raw2, sent1 + sent2)
    assert sent2 == (raw2 if dense1 else sent1)


def test_destination_off_16_byte_alignment_travels_plain(hipctx):
    """k_sparse_unpack stores 16-byte groups: a destination one float off travels as a plain copy, and the counters say so"""
    case = {c.name: c for c in sc.length_cases()}["n%d" % (5 * sc.TASK + 37)]
    n = case.words.size
    assert upload_checked(hipctx, case, misalign=1) == (4 * n, 4 * n)
    raw, sent = upload_checked(hipctx, case)                # (and the aligned destination packs the same image)
    assert raw == 4 * n and sent == sc.expected_counters(case)[1] < raw


def test_production_piece_length(hipctx):
    """two pieces of 12 Mi floats and 37 more: the piece length bcd_hip_denoise_host_ex uses, on about 100 MB"""
    case = sc.production_case()
    assert upload_checked(hipctx, case) == sc.expected_counters(case)[:2]


def test_a_sequence_of_uploads_on_one_context():
    """ten uploads on a context of their own: lengths that grow, shrink and grow past the staging buffers' first allocation, another pattern each time --
    a staging buffer that kept something of an earlier call shows in the bits"""
    import bcd_amd.hip as bh
    ctx = bh.Context(0)
    try:
        for case in sc.sequence_cases():
            assert upload_checked(ctx, case) == sc.expected_counters(case)[:2], case.id
    finally:
        ctx.close()


# ---- every packer the host offers, at 0 (the caller packs alone), 1 and 15 pool threads: both environment variables are read once per process, so
# each combination runs in a fresh child process (this file as a script: no torch, the HIP runtime through ctypes)
_child_failed = []


@pytest.mark.parametrize("simd", ["scalar", "avx2", "avx512"])
def test_every_packer_at_every_thread_count_in_child_processes(simd):
    for threads in (0, 1, 15):
        if _child_failed:
            pytest.fail("not started: an earlier child failed (%s)" % _child_failed[0])
        env = dict(os.environ, BCD_HIP_UPLOAD_SIMD=simd, BCD_HIP_UPLOAD_THREADS=str(threads))
        what = "BCD_HIP_UPLOAD_SIMD=%s BCD_HIP_UPLOAD_THREADS=%d" % (simd, threads)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            _child_failed.append(what + ": timed out")
            pytest.fail(_child_failed[0])
        if r.returncode != 0:
            _child_failed.append("%s: exit status %d\n%s\n%s" % (what, r.returncode, r.stdout[-1500:], r.stderr[-1500:]))
            pytest.fail(_child_failed[0])
        kind = int(r.stdout.split("KIND")[1].split()[0])
        print("%s -> packer %d, %s cases" % (what, kind, r.stdout.split("CASES")[1].split()[0]))
        assert kind in (0, 2, 5)
        if simd == "scalar":
            assert kind == 0                                  # the scalar form always exists; the others run where the host has them
        if simd == "avx2":
            assert kind in (0, 2)


def _child():
    """bit-pattern, length and multi-piece cases through bcd_hip_selftest_sparse_upload with whatever packer and thread count the environment selects;
    prints the packer kind; any mismatch is an exception (exit status 1)"""
    import ctypes as C
    sys.path.insert(0, ROOT)
    import bcd_amd.hip as bh
    lib = bh.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    h = C.c_void_p()
    chk(lib.bcd_hip_ctx_create(C.byref(h), 0, None), "bcd_hip_ctx_create")
    cases = sc.pattern_cases() + sc.length_cases() + sc.multi_piece_cases()
    for case in cases:
        n = case.words.size
        total = GUARD + n + GUARD
        d = C.c_void_p()
        chk(hip.hipMalloc(C.byref(d), 4 * total), "hipMalloc")
        try:
            chk(hip.hipMemset(d, 0xA5, 4 * total), "hipMemset")
            chk(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            raw, sent = C.c_int64(0), C.c_int64(0)
            rc = lib.bcd_hip_selftest_sparse_upload(h, case.words.ctypes.data_as(C.c_void_p), n, C.c_void_p(d.value + 4 * GUARD), 1, case.piece, C.byref(raw), C.byref(sent))
            if rc != 0:
                raise RuntimeError("%s: rc=%d: %s" % (case.id, rc, lib.bcd_hip_last_error(h).decode()))
            got = np.empty(total, np.uint32)
            chk(hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d, 4 * total, 2), "hipMemcpy")  # (2: device to host)
        finally:
            hip.hipFree(d)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), "%s: a guard word was written" % case.id
        diff = first_difference(got[GUARD:GUARD + n], case.words)
        assert diff is None, "%s: %s" % (case.id, diff)
        assert (raw.value, sent.value) == sc.expected_counters(case)[:2], "%s: counters %s" % (case.id, (raw.value, sent.value))
    v = np.arange(1, 33, dtype=np.uint32)
    out = np.zeros(64, np.uint32)
    bits, cnt = C.c_uint32(0), C.c_int(0)
    kind = lib.bcd_hip_selftest_pack32(v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(bits), C.byref(cnt))
    lib.bcd_hip_ctx_destroy(h)
    print("KIND %d CASES %d" % (kind, len(cases)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        _child()
    else:
        sys.exit("usage: %s --child" % sys.argv[0])
