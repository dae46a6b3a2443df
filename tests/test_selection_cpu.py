"""CPU tests of the kept-selection boundary: the ctypes mirrors of struct bcd_hip_selection_info / bcd_hip_selection_scale have the header's fields in the
header's order and the size a C compiler gives them; without a device nothing can be created; a closed Selection raises."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import bcd_amd.hip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bcd_hip.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def struct_fields(txt, opening):
    """[(C type, name, array length or None)] of the struct whose definition starts with `opening`"""
    body = re.search(re.escape(opening) + r"\s*\{(.*?)\}", txt, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for name in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(\w+)\])?\s*$", name)
            out.append((ctype, m.group(1), m.group(2)))
    return out


CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "bcd_hip_params": bh.Params, "bcd_hip_selection_scale": bh.SelectionScale}


def check_mirror(mirror, fields, defines):
    assert [n for _, n, _ in fields] == [n for n, _ in mirror._fields_]
    for (ctype, name, length), (_, got) in zip(fields, mirror._fields_):
        want = CTYPES[ctype]
        if length is not None:
            want = want * int(defines.get(length, length))
        assert C.sizeof(got) == C.sizeof(want) and (got is want or (length is not None and got._type_ is want._type_ and got._length_ == want._length_)), name


def test_selection_info_mirror_has_the_headers_fields_and_size(tmp_path):
    txt = header_text()
    defines = dict(re.findall(r"#define\s+(BCD_HIP_\w+)\s+(\d+)\s*$", txt, flags=re.M))
    assert int(defines["BCD_HIP_SELECTION_MAX_SCALES"]) == bh.SELECTION_MAX_SCALES
    check_mirror(bh.SelectionScale, struct_fields(txt, "typedef struct bcd_hip_selection_scale"), defines)
    check_mirror(bh.SelectionInfo, struct_fields(txt, "struct bcd_hip_selection_info"), defines)
    # the sizes a C compiler gives them (the header is C: a struct tag and an entry point share the name bcd_hip_selection_info)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bcd_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(struct bcd_hip_selection_info), '
                   'sizeof(bcd_hip_selection_scale), sizeof(bcd_hip_params)); return 0; }\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(bh.SelectionInfo), C.sizeof(bh.SelectionScale), C.sizeof(bh.Params)]


def test_the_new_entry_points_are_declared_with_the_issues_arguments():
    txt = " ".join(header_text().split())
    for proto in ("int bcd_hip_selection_create(bcd_hip_ctx *ctx, bcd_hip_selection **sel);",
                  "void bcd_hip_selection_destroy(bcd_hip_selection *sel);",
                  "int bcd_hip_selection_denoise(bcd_hip_selection *sel, const float *d_nsamples, const bcd_hip_layer *layers, int nb_layers);",
                  "int bcd_hip_selection_info(const bcd_hip_selection *sel, struct bcd_hip_selection_info *out);",
                  "int bcd_hip_selection_read(bcd_hip_selection *sel, int scale, uint32_t *d_mask, int32_t *d_nsim, uint8_t *d_state, int32_t *d_count);",
                  "int bcd_hip_accum_moments(bcd_hip_accum *acc, float *d_nsamples, float *d_mean, float *d_cov);"):
        assert proto in txt, proto
    assert "const bcd_hip_layer *layers, int nb_layers, bcd_hip_selection *sel);" in txt


def test_without_a_device_nothing_is_created():
    import torch
    L = bh.lib()
    h = C.c_void_p()
    assert L.bcd_hip_selection_create(None, C.byref(h)) == -1 and not h.value        # no context, no selection
    assert L.bcd_hip_selection_create(None, None) == -1
    assert L.bcd_hip_selection_denoise(None, None, None, 1) == -1
    assert L.bcd_hip_selection_read(None, 0, None, None, None, None) == -1
    assert L.bcd_hip_selection_info(None, C.byref(bh.SelectionInfo())) == -1
    assert L.bcd_hip_accum_moments(None, None, None, None) == -1
    L.bcd_hip_selection_destroy(None)                                                  # (a null handle is ignored)
    if torch.cuda.is_available():
        return
    with pytest.raises(bh.BcdHipError):
        bh.Context(0).selection()


class _NoContext:
    h = None
    device = 0

    def _chk(self, rc):
        raise AssertionError("a closed selection reached the library")


def test_a_closed_selection_raises():
    sel = bh.Selection.__new__(bh.Selection)
    sel.ctx, sel.h = _NoContext(), None                       # what close() leaves behind
    for call in (sel.info, lambda: sel.read(0), lambda: sel.denoise([]), sel._handle):
        with pytest.raises(bh.BcdHipError, match="closed"):
            call()
    sel.close()                                               # (closing twice is fine)
