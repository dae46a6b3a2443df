"""CPU tests of the binding's declaration of the C ABI: every prototype and every structure mirror of bcd_amd/_prototypes.py is derived again
from include/bcd_hip.h by the mapping rule of that module's docstring and compared; the table is applied when the library loads."""
import ctypes as C
import os
import re

import bcd_amd._prototypes as bp
import bcd_amd.hip as bh
from test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "long long": C.c_longlong,
           "float": C.c_float}
FIELD_SCALARS = dict(SCALARS, uint8_t=C.c_uint8, char=C.c_char)
RESTYPES = {"int": C.c_int, "void": None, "char *": C.c_char_p, "uint32_t": C.c_uint32}
OPAQUE = {"bcd_hip_ctx", "bcd_hip_accum", "bcd_hip_selection", "bcd_hip_multi"}
POINTEES = set(SCALARS) | OPAQUE | {"void", "char", "uint8_t"}          # a pointer to one of these, at any depth, is a c_void_p
MIRRORS = {s._c_name_: s for s in vars(bp).values() if isinstance(s, type) and issubclass(s, C.Structure) and hasattr(s, "_c_name_")}
UNMIRRORED = {"bcd_hip_warped_layer"}                                   # header structs the binding has no Structure for (passed as c_void_p)


def header_text():
    """include/bcd_hip.h without comments and preprocessor lines; -> (text, {macro: int})"""
    txt = open(os.path.join(ROOT, "include", "bcd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    macros = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(BCD_HIP_\w+)[ \t]+(.+?)[ \t]*$", txt, flags=re.M):
        expr = re.sub(r"BCD_HIP_\w+", lambda m: str(macros[m.group(0)]), expr)
        assert re.fullmatch(r"[\d\s()+\-*]+", expr), (name, expr)
        macros[name] = int(eval(expr, {}))
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    return txt, macros


def declarator(base, decl, macros):
    """'*d_colors' / 'reserved[8]' / '*const *d_sum' of a base type -> (base, pointer depth, name, array length or None); a parameter array is a pointer"""
    stars = decl.count("*")
    m = re.fullmatch(r"(\w+)\s*(?:\[\s*(\w+)\s*\])?", decl.replace("*", " ").strip())
    assert m, (base, decl)
    n = m.group(2)
    return base, stars, m.group(1), None if n is None else int(macros.get(n, n))


def map_parameter(base, stars, length):
    if length is not None:
        stars += 1
    if stars == 0:
        if base == "bcd_hip_progress_fn":
            return bp.PROGRESS_FN
        return SCALARS[base]                                            # (KeyError: a C type the rule does not know)
    if stars == 1 and base in MIRRORS:
        return C.POINTER(MIRRORS[base])
    if stars == 1 and base in UNMIRRORED:
        return C.c_void_p
    assert base in POINTEES, "no rule for a pointer (depth %d) to %r" % (stars, base)
    return C.c_void_p


def header_prototypes():
    """{name: (restype, [argtypes])} of every `ret bcd_hip_name(args);` of the header, mapped by the rule; anything else that is left between two
    semicolons once the structures and typedefs are taken out fails"""
    txt, macros = header_text()
    txt = re.sub(r"(typedef\s+)?struct\s*\w*\s*\{[^{}]*\}\s*\w*\s*;", "", txt)
    txt = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", txt)
    txt, n = re.subn(r"typedef\s+void\s*\(\s*\*\s*bcd_hip_progress_fn\s*\)\s*\([^()]*\)\s*;", "", txt)
    assert n == 1
    txt = txt.replace('extern "C" {', "")
    protos, arrays = {}, 0
    for stmt in txt.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"([\w *]+?)\b(bcd_hip_\w+) ?\(([^()]*)\)", stmt)
        assert m, "not a prototype: %r" % stmt
        ret, name, args = re.sub(r"\bconst\b", "", m.group(1)).strip(), m.group(2), m.group(3)
        assert name not in protos, name
        argtypes = []
        for a in [] if args.strip() == "void" else args.split(","):
            a = re.sub(r"\b(const|struct)\b", " ", a).strip()
            bm = re.fullmatch(r"(long long|\w+)\b\s*(.*)", a)
            base, stars, _, length = declarator(bm.group(1), bm.group(2), macros)
            arrays += length is not None
            argtypes.append(map_parameter(base, stars, length))
        protos[name] = (RESTYPES[" ".join(ret.replace("*", " *").split())], argtypes)
    assert arrays == 1                                                  # (int32_t counts_out[4] of bcd_hip_selftest_active_lists)
    return protos


def header_structures():
    """{C name: [(field, base type, pointer depth, array length or None)]} of every structure the header defines"""
    txt, macros = header_text()
    found = re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", txt)
    found += [(body, name) for name, body in re.findall(r"^struct\s+(\w+)\s*\{([^{}]*)\}\s*;", txt, flags=re.M)]     # (struct bcd_hip_selection_info)
    assert len(found) == txt.count("{") - 1                             # (every brace pair but extern "C")
    out = {}
    for body, name in found:
        fields = []
        for stmt in body.split(";"):
            stmt = re.sub(r"\bconst\b", " ", stmt).strip()
            if not stmt:
                continue
            base, rest = re.fullmatch(r"(\w+)\b\s*(.*)", stmt, flags=re.S).groups()
            fields += [declarator(base, d.strip(), macros) for d in rest.split(",")]
        out[name] = [(f, b, s, n) for b, s, f, n in fields]
    return out


# the pointer fields that are typed, because they are assigned ctypes arrays or pointers, which a c_void_p field does not take; every other is c_void_p
TYPED_FIELDS = {("bcd_hip_guide", "floors"), ("bcd_hip_frame_layers", "layers"), ("bcd_hip_stage_frame_layers", "d_colors"),
                ("bcd_hip_stage_frame_layers", "d_pixel_cov")}


def field_type(struct, field, base, stars, length):
    """the one ctypes type a mirror gives a field, by the field rule of bcd_amd/_prototypes.py"""
    if stars == 0:
        t = MIRRORS[base] if base in MIRRORS else FIELD_SCALARS[base]
        return t if length is None else t * length
    assert length is None and (base in MIRRORS or base in POINTEES), base
    if (struct, field) not in TYPED_FIELDS:
        return C.c_void_p
    if stars == 2:
        return C.POINTER(C.c_void_p)
    return C.POINTER(MIRRORS[base] if base in MIRRORS else SCALARS[base])


def table_keys():
    """the keys of the PROTOTYPES literal as written (a dict display drops a repeated key without a word)"""
    import ast
    tree = ast.parse(open(bp.__file__).read())
    node, = [n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "PROTOTYPES"]
    return [k.value for k in node.keys]


def test_every_prototype_matches_the_header():
    want = header_prototypes()
    assert len(want) >= 158
    assert sorted(want) == header_symbols() == sorted(bh.SYMBOLS) == sorted(bp.PROTOTYPES)
    assert sorted(table_keys()) == sorted(bp.PROTOTYPES)                # (no entry written twice)
    for name in bh.SYMBOLS:
        restype, argtypes = bp.PROTOTYPES[name]
        assert restype is want[name][0], "%s: restype %r, the header says %r" % (name, restype, want[name][0])
        assert list(argtypes) == want[name][1], "%s: argtypes %r, the header says %r" % (name, list(argtypes), want[name][1])


def test_every_structure_matches_the_header():
    structs = header_structures()
    assert set(structs) == set(MIRRORS) | UNMIRRORED and not set(MIRRORS) & UNMIRRORED
    for s in vars(bp).values():                                         # every Structure of the binding names the struct it mirrors
        if isinstance(s, type) and issubclass(s, C.Structure) and s is not C.Structure:
            assert MIRRORS.get(getattr(s, "_c_name_", None)) is s, s
    assert all(s in structs and f in dict(MIRRORS[s]._fields_) for s, f in TYPED_FIELDS)
    for name, mirror in MIRRORS.items():
        assert [f for f, _ in mirror._fields_] == [f for f, _, _, _ in structs[name]], name
        for (f, t), (_, base, stars, length) in zip(mirror._fields_, structs[name]):
            assert t is field_type(name, f, base, stars, length), "%s.%s: %r, the header says %s%s" % (name, f, t, base, " *" * stars)
    _, macros = header_text()
    assert bh.MAX_LAYERS == macros["BCD_HIP_MAX_LAYERS"] and bh.SELECTION_MAX_SCALES == macros["BCD_HIP_SELECTION_MAX_SCALES"]
    assert bh.ACCUM_MAX_LAYERS == macros["BCD_HIP_ACCUM_MAX_LAYERS"] and bh.MULTI_ID_BYTES == macros["BCD_HIP_MULTI_ID_BYTES"]
    assert bh.STATE_HEADER_BYTES == macros["BCD_HIP_ACCUM_STATE_HEADER_BYTES"] == C.sizeof(bh.StateHeader)
    assert macros["BCD_HIP_ACCUM_LAYERS_HEADER_BYTES"] == C.sizeof(bh.LayersHeader)


def test_table_is_applied_on_load():
    L = bh.lib()
    assert len(L.bcd_hip_denoise.argtypes) == 11
    for name, (restype, argtypes) in bp.PROTOTYPES.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name
    assert L.bcd_hip_scale_seed(10, 0) == 10
    assert L.bcd_hip_accum_state_info(None, 2 ** 33, None) == -1
