"""CPU tests of serialised accumulator states (format v1, include/bcd_hip.h): bcd_hip_accum_state_info / accum_state_info accept a
well-formed header and refuse each malformed field without a device, and raw2bcd refuses a bad --merge-state file (rc 1) before the
device is touched."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bcd_amd.hip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bcd_amd", "lib", "raw2bcd")


def header(W=5, H=3, bins=20, gamma=2.2, maxv=2.5, magic=b"BCDACCST", version=1, header_bytes=64, planes=None, added=0, dropped=0,
           reserved=bytes(8)):
    planes = 11 + 3 * bins if planes is None else planes
    return magic + struct.pack("<IIiiiffIqq", version, header_bytes, W, H, bins, gamma, maxv, planes, added, dropped) + reserved


def state(W=5, H=3, bins=20, extra=0, **kw):
    """a header and its planes (zeros; `extra` floats more or fewer than the format asks for)"""
    return header(W, H, bins, **kw) + np.zeros((11 + 3 * bins) * W * H + extra, np.float32).tobytes()


def info_rc(buf, size=None):
    L = bh.lib()
    a = np.frombuffer(buf, np.uint8)
    out = bh.StateHeader()
    return L.bcd_hip_accum_state_info(a.ctypes.data_as(C.c_void_p), len(buf) if size is None else size, C.byref(out)), out


def test_header_layout_is_64_bytes():
    assert len(header()) == 64 and C.sizeof(bh.StateHeader) == 64
    assert bh.StateHeader.samples_added.offset == 40 and bh.StateHeader.dropped.offset == 48 and bh.StateHeader.reserved.offset == 56


def test_well_formed_state_is_accepted():
    s = state(W=7, H=4, bins=16, gamma=2.0, maxv=1.5, added=123, dropped=4)
    rc, h = info_rc(s)
    assert rc == 0
    assert (h.width, h.height, h.nb_bins, h.nb_planes, h.samples_added, h.dropped) == (7, 4, 16, 59, 123, 4)
    d = bh.accum_state_info(s)
    assert d["magic"] == b"BCDACCST" and d["version"] == 1 and d["header_bytes"] == 64
    assert (d["width"], d["height"], d["nb_bins"], d["gamma"], d["max_value"]) == (7, 4, 16, 2.0, 1.5)
    info, planes = bh.accum_state_planes(bytearray(s))
    assert info == d and planes.shape == (59, 4, 7) and planes.dtype == np.float32
    assert bh.lib().bcd_hip_accum_state_info(C.c_char_p(s), C.c_int64(len(s)), None) == 0       # (out may be NULL)
    for bins in (2, 85):
        assert info_rc(state(bins=bins))[0] == 0


@pytest.mark.parametrize("case,buf", [
    ("magic", state(magic=b"BCDACCSX")),
    ("version0", state(version=0)),
    ("version2", state(version=2)),
    ("header_bytes", state(header_bytes=128)),
    ("bins1", state(bins=1)),
    ("bins86", state(bins=86)),
    ("width0", state(W=0, H=3)),
    ("height_negative", header(W=5, H=-3) + bytes(4 * 71 * 15)),
    ("too_many_pixels", header(W=1 << 16, H=1 << 15)),
    ("planes", header(planes=70) + bytes(4 * 70 * 15)),
    ("short_by_one_float", state(extra=-1)),
    ("long_by_one_float", state(extra=1)),
    ("long_by_one_byte", state() + b"\0"),
    ("reserved", state(reserved=b"\0\0\0\0\0\0\0\1")),
    ("negative_added", state(added=-1)),
    ("negative_dropped", state(dropped=-5)),
    ("header_only", header()),
    ("truncated_header", header()[:63]),
    ("empty", b""),
])
def test_malformed_states_are_refused(case, buf):
    if buf:
        assert info_rc(buf)[0] == -1                               # BCD_HIP_EINVAL
    with pytest.raises(ValueError):
        bh.accum_state_info(buf)


def test_size_argument_is_the_whole_state():
    s = state()
    assert info_rc(s, len(s))[0] == 0
    assert info_rc(s, len(s) - 4)[0] == -1 and info_rc(s, len(s) + 4)[0] == -1 and info_rc(s, 63)[0] == -1
    assert bh.lib().bcd_hip_accum_state_info(None, C.c_int64(len(s)), None) == -1


# ---- raw2bcd --merge-state / --save-state: refusals before the device ----------------------------------------------------------------

def run(*args):
    assert os.path.exists(EXE), "raw2bcd is not built: run `python -m bcd_amd.build`"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def device_touched(r):
    # the same check as tests/test_raw2bcd_cli.py: every device-side failure names the device or a bcd_hip_* call
    return "device" in r.stderr.lower() or "bcd_hip" in r.stderr


def write_raw(path, W, H, spp=2, channels=3):
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", 1, W, H, spp, channels))
        f.write(np.zeros(W * H * spp * channels, np.float32).tobytes())


def refused(r, tmp_path, message):
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert not device_touched(r), r.stderr
    assert not any(p.name.startswith("out") for p in tmp_path.iterdir())      # nothing written


def test_save_state_without_a_path_is_a_usage_error(tmp_path):
    r = run("--save-state")
    assert r.returncode == 1 and "Usage: raw2bcd" in r.stdout and "--save-state takes a file path" in r.stderr
    r = run("--merge-state")
    assert r.returncode == 1 and "--merge-state takes a file path" in r.stderr
    assert run("--save-state", tmp_path / "s.bcdacc", "only_one").returncode == 1     # one positional still needs a --merge-state


@pytest.mark.parametrize("case,content,message", [
    ("missing", None, "cannot open state file"),
    ("truncated", header()[:40], "shorter than its 64-byte header"),
    ("short", state(W=4, H=4, extra=-3), "its header claims"),
    ("long", state(W=4, H=4, extra=2), "its header claims"),
    ("magic", state(W=4, H=4, magic=b"NOTASTAT"), "is not an accumulator state"),
    ("version", state(W=4, H=4, version=7), "is not an accumulator state"),
    ("reserved", state(W=4, H=4, reserved=b"\1" + bytes(7)), "is not an accumulator state"),
    ("width", state(W=5, H=4), "holds a 5 x 4 frame"),
    ("height", state(W=4, H=3), "holds a 4 x 3 frame"),
    ("bins", state(W=4, H=4, bins=16), "raw2bcd accumulates 20 bins, gamma 2.2, max 2.5"),
    ("gamma", state(W=4, H=4, gamma=2.0), "raw2bcd accumulates 20 bins"),
    ("max", state(W=4, H=4, maxv=2.5000002), "raw2bcd accumulates 20 bins"),
])
def test_bad_merge_state_is_refused_before_the_device(tmp_path, case, content, message):
    raw = tmp_path / "frame.raw"
    write_raw(raw, 4, 4)
    st = tmp_path / (case + ".bcdacc")
    if content is not None:
        st.write_bytes(content)
    good = tmp_path / "good.bcdacc"
    good.write_bytes(state(W=4, H=4))
    r = run("--merge-state", st, raw, tmp_path / "out")                            # after a raw file
    refused(r, tmp_path, message)
    assert st.name in r.stderr or case == "missing" and "missing" in r.stderr       # the message names the file
    r = run("--merge-state", good, "--merge-state", st, "--save-state", tmp_path / "out.bcdacc", tmp_path / "out")   # states only
    refused(r, tmp_path, message)


def test_states_only_take_the_frame_size_of_the_first_state(tmp_path):
    a, b = tmp_path / "a.bcdacc", tmp_path / "b.bcdacc"
    a.write_bytes(state(W=6, H=2))
    b.write_bytes(state(W=4, H=3))
    refused(run("--merge-state", a, "--merge-state", b, tmp_path / "out"), tmp_path, "holds a 4 x 3 frame, the others 6 x 2")


def test_raw_file_is_checked_before_the_states(tmp_path):
    raw = tmp_path / "bad.raw"
    raw.write_bytes(struct.pack("<5i", 1, 4, 4, 2, 5))
    st = tmp_path / "s.bcdacc"
    st.write_bytes(state(W=4, H=4))
    refused(run("--merge-state", st, raw, tmp_path / "out"), tmp_path, "nbOfChannels is 5")
