"""CPU tests of the accumulator's colour layers (bcd_hip_accum_*_layers, include/bcd_hip.h): every new entry point refuses a null
accumulator without touching a device, and bcd_hip_accum_layers_state_info / accum_layers_state_info accept a well-formed layer block
and refuse each malformed field."""
import ctypes as C
import struct

import numpy as np
import pytest

import bcd_amd.hip as bh

EINVAL = -1


def header(W=5, H=3, L=2, magic=b"BCDACCLY", version=1, header_bytes=64, planes=None, reserved=bytes(32)):
    planes = 9 * L if planes is None else planes
    return magic + struct.pack("<IIiiiI", version, header_bytes, W, H, L, planes) + reserved


def block(W=5, H=3, L=2, extra=0, **kw):
    """a header and its planes (zeros; `extra` floats more or fewer than the format asks for)"""
    return header(W, H, L, **kw) + np.zeros(max(0, 9 * L * W * H + extra), np.float32).tobytes()


def info_rc(buf, size=None):
    a = np.frombuffer(buf, np.uint8)
    out = bh.LayersHeader()
    rc = bh.lib().bcd_hip_accum_layers_state_info(a.ctypes.data_as(C.c_void_p), len(buf) if size is None else size, C.byref(out))
    return rc, out


def test_layer_entry_points_refuse_a_null_accumulator():
    """in the manner of test_splat_entry_points_refuse_a_null_accumulator: no device is touched, nothing is enqueued"""
    L = bh.lib()
    h = C.c_void_p()
    n, b = C.c_int(7), C.c_int64(7)
    one = (C.c_void_p * 1)()
    buf = np.frombuffer(block(), np.uint8)
    assert L.bcd_hip_accum_create_layers(None, 8, 8, 20, 2.2, 2.5, 0, 2, C.byref(h)) == EINVAL and not h.value
    assert L.bcd_hip_accum_nb_layers(None, C.byref(n)) == EINVAL and n.value == 7
    assert L.bcd_hip_accum_add_dense_layers(None, None, None, 0, 1, 1, 3, one, 3) == EINVAL
    for count in (0, 5):
        assert L.bcd_hip_accum_add_scattered_layers(None, None, None, None, count, one) == EINVAL
        assert L.bcd_hip_accum_add_splatted_layers(None, None, None, None, count, one) == EINVAL
    assert L.bcd_hip_accum_layer_statistics(None, one, one) == EINVAL
    assert L.bcd_hip_accum_layers_state_bytes(None, C.byref(b)) == EINVAL and b.value == 7
    assert L.bcd_hip_accum_export_layers(None, buf.ctypes.data_as(C.c_void_p), buf.size) == EINVAL
    assert L.bcd_hip_accum_import_layers(None, buf.ctypes.data_as(C.c_void_p), buf.size) == EINVAL
    assert L.bcd_hip_accum_merge_layers_state(None, buf.ctypes.data_as(C.c_void_p), buf.size) == EINVAL


def test_header_layout_is_64_bytes():
    assert len(header()) == 64 and C.sizeof(bh.LayersHeader) == 64
    f = bh.LayersHeader
    assert (f.magic.offset, f.version.offset, f.header_bytes.offset, f.width.offset, f.height.offset, f.nb_layers.offset, f.nb_planes.offset,
            f.reserved.offset) == (0, 8, 12, 16, 20, 24, 28, 32)
    assert f.reserved.size == 32
    assert bh.ACCUM_MAX_LAYERS == bh.MAX_LAYERS - 1 == 15


def test_well_formed_block_is_accepted():
    s = block(W=7, H=4, L=3)
    assert len(s) == 64 + 36 * 3 * 7 * 4
    rc, h = info_rc(s)
    assert rc == 0 and (h.width, h.height, h.nb_layers, h.nb_planes) == (7, 4, 3, 27)
    d = bh.accum_layers_state_info(s)
    assert d == {"magic": b"BCDACCLY", "version": 1, "header_bytes": 64, "width": 7, "height": 4, "nb_layers": 3, "nb_planes": 27}
    info, planes = bh.accum_layers_state_planes(bytearray(s))
    assert info == d and planes.shape == (3, 9, 4, 7) and planes.dtype == np.float32
    assert bh.lib().bcd_hip_accum_layers_state_info(C.c_char_p(s), C.c_int64(len(s)), None) == 0     # (out may be NULL)
    for L in (1, 15):
        assert info_rc(block(L=L))[0] == 0


@pytest.mark.parametrize("case,buf", [
    ("magic", block(magic=b"BCDACCST")),
    ("version0", block(version=0)),
    ("version2", block(version=2)),
    ("header_bytes", block(header_bytes=128)),
    ("layers0", header(L=0, planes=0)),
    ("layers16", block(L=16)),
    ("layers_negative", header(L=-1, planes=9) + bytes(36 * 15)),
    ("planes", header(L=2, planes=22) + bytes(4 * 22 * 15)),
    ("width0", block(W=0, H=3)),
    ("too_many_pixels", header(W=1 << 16, H=1 << 15)),
    ("short_by_one_float", block(extra=-1)),
    ("long_by_one_float", block(extra=1)),
    ("long_by_one_byte", block() + b"\0"),
    ("reserved_first", block(reserved=b"\1" + bytes(31))),
    ("reserved_last", block(reserved=bytes(31) + b"\1")),
    ("header_only", header()),
    ("truncated_header", header()[:63]),
    ("empty", b""),
])
def test_malformed_blocks_are_refused(case, buf):
    if buf:
        assert info_rc(buf)[0] == EINVAL
    with pytest.raises(ValueError):
        bh.accum_layers_state_info(buf)


def test_size_argument_is_the_whole_block():
    s = block()
    assert info_rc(s, len(s))[0] == 0
    assert info_rc(s, len(s) - 4)[0] == EINVAL and info_rc(s, len(s) + 4)[0] == EINVAL and info_rc(s, 63)[0] == EINVAL
    assert bh.lib().bcd_hip_accum_layers_state_info(None, C.c_int64(len(s)), None) == EINVAL


def test_a_v1_state_is_not_a_layer_block_and_the_reverse():
    s = block()
    with pytest.raises(ValueError):
        bh.accum_state_info(s)
    v1 = b"BCDACCST" + struct.pack("<IIiiiffIqq", 1, 64, 5, 3, 20, 2.2, 2.5, 71, 0, 0) + bytes(8) + bytes(4 * 71 * 15)
    assert bh.accum_state_info(v1)["nb_planes"] == 71
    with pytest.raises(ValueError):
        bh.accum_layers_state_info(v1)
