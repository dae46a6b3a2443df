"""CPU tests of the raw2bcd front-end (bcd_amd/host/raw2bcd.cpp): usage, and the header / size checks that refuse a bad raw file
before the device is touched (the reference's converter reads past them silently)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bcd_amd", "lib", "raw2bcd")


def run(*args):
    assert os.path.exists(EXE), "raw2bcd is not built: run `python -m bcd_amd.build`"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def write_raw(path, header, payload_floats=0):
    with open(path, "wb") as f:
        f.write(header)
        f.write(np.zeros(payload_floats, np.float32).tobytes())


def device_touched(r):
    # every device-side failure names the device or a bcd_hip_* call; the header checks come first
    return "device" in r.stderr.lower() or "bcd_hip" in r.stderr


def test_no_arguments_prints_usage_and_fails():
    r = run()
    assert r.returncode != 0
    assert "Usage: raw2bcd" in r.stdout and "<outputPrefix>" in r.stdout


def test_wrong_argument_count_and_bad_chunk_flag():
    assert run("only_one").returncode != 0
    r = run("--chunk-mb", "0", "a", "b")
    assert r.returncode != 0 and "--chunk-mb" in r.stderr


def test_missing_input_file(tmp_path):
    r = run(tmp_path / "nope.raw", tmp_path / "out")
    assert r.returncode != 0 and "cannot open" in r.stderr and not device_touched(r)


@pytest.mark.parametrize("case,header,floats,message", [
    ("truncated", struct.pack("<3i", 1, 4, 4), 0, "truncated header"),
    ("channels5", struct.pack("<5i", 1, 4, 4, 2, 5), 4 * 4 * 2 * 5, "nbOfChannels is 5"),
    ("channels2", struct.pack("<5i", 1, 4, 4, 2, 2), 4 * 4 * 2 * 2, "nbOfChannels is 2"),
    ("zero_width", struct.pack("<5i", 1, 0, 4, 2, 3), 0, "must be positive"),
    ("negative_spp", struct.pack("<5i", 1, 4, 4, -1, 3), 0, "must be positive"),
    ("short", struct.pack("<5i", 1, 8, 6, 4, 4), 8 * 6 * 4 * 4 - 1, "its header claims"),
    ("huge", struct.pack("<5i", 1, 2 ** 30, 2 ** 30, 2 ** 30, 4), 0, "more than"),
])
def test_bad_raw_files_are_refused_before_the_device(tmp_path, case, header, floats, message):
    src = tmp_path / (case + ".raw")
    write_raw(src, header, floats)
    r = run(src, tmp_path / "out")
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert not device_touched(r), r.stderr
    assert not any(p.name.startswith("out") for p in tmp_path.iterdir())      # nothing written
