"""The ctypes prototypes of the text detector's C-ABI against the header that documents it (no GPU).

vsr_amd/_lib.py binds every symbol of include/vsr_hip.h by hand (SIGNATURES).  A launcher whose ctypes argument list is shifted or
has an int where the header has an int64_t still loads and still launches -- with garbage strides.  Here the prototypes of every
vsr_det_launch_*, vsr_host_trace_borders and vsr_gemm_plan_* are parsed from the header and held to SIGNATURES in argument count and
kind (pointer, int, int64, float) and in the return type, so such a slip fails on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsr_hip.h")
WANTED = re.compile(r"^(vsr_det_launch_\w+|vsr_host_trace_borders|vsr_gemm_plan_\w+)$")


def _header_kind(arg):
    """kind of one C parameter declaration"""
    a = arg.strip()
    if "*" in a or "[" in a:
        return "pointer"
    a = re.sub(r"\b(const|unsigned|signed)\b", " ", a).split()
    t = a[0]
    if t in ("int64_t", "uint64_t", "size_t", "long"):
        return "int64"
    if t in ("int", "int32_t", "uint32_t"):
        return "int"
    if t == "float":
        return "float"
    raise AssertionError(f"unparsed parameter {arg!r}")


def _header_prototypes():
    """{name: (return kind, [argument kinds])} of the wanted declarations of include/vsr_hip.h, comments stripped"""
    src = open(HEADER).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(vsr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        if not WANTED.match(name):
            continue
        args = args.strip()
        kinds = [] if args in ("", "void") else [_header_kind(a) for a in args.split(",")]
        assert name not in out, f"{name} is declared twice"
        out[name] = (ret, kinds)
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or isinstance(t, type) and issubclass(t, C._Pointer):
        return "pointer"
    if t is C.c_float:
        return "float"
    if t is C.c_double:
        return "double"
    if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ":
        return {4: "int", 8: "int64"}.get(C.sizeof(t), f"integer of {C.sizeof(t)} bytes")
    raise AssertionError(f"unparsed ctypes type {t!r}")


def test_parser_reads_the_kinds():
    """the two parsers on declarations whose answer is known: a parser that calls everything an int would pass every comparison"""
    assert [_header_kind(a) for a in ("const float* x", "int64_t HW", "int32_t cap", "float p0", "vsr_gemm_plan_t** out", "void* stream",
                                      "const uint8_t* img", "int n")] == ["pointer", "int64", "int", "float", "pointer", "pointer", "pointer", "int"]
    assert [_ctypes_kind(t) for t in (C.c_void_p, C.c_int, C.c_int64, C.c_float, C.POINTER(C.c_void_p), C.c_char_p, None, C.c_int32)] == \
        ["pointer", "int", "int64", "float", "pointer", "pointer", "void", "int"]
    with pytest.raises(AssertionError):
        _header_kind("double d")


def test_det_prototypes_match_the_header(built_lib):
    decl, sigs = _header_prototypes(), built_lib.SIGNATURES
    bound = {n for n in sigs if WANTED.match(n)}
    # the 20 launchers of csrc/det_kernels.hip (18 forward kernels, ccl, db_boxes), the host border tracer and the three plan calls
    assert len([n for n in decl if n.startswith("vsr_det_launch_")]) == 20, sorted(decl)
    assert {"vsr_host_trace_borders", "vsr_gemm_plan_create", "vsr_gemm_plan_run", "vsr_gemm_plan_destroy"} <= set(decl)
    assert bound == set(decl), f"declared, not bound: {sorted(set(decl) - bound)}; bound, not declared: {sorted(bound - set(decl))}"
    bad = []
    for name in sorted(decl):
        ret, kinds = decl[name]
        restype, argtypes = sigs[name]
        got_ret, got = _ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes]
        if got_ret != ret:
            bad.append(f"{name}: returns {ret} in the header, {got_ret} in SIGNATURES")
        if len(got) != len(kinds):
            bad.append(f"{name}: {len(kinds)} arguments in the header, {len(got)} in SIGNATURES")
            continue
        bad += [f"{name}: argument {i} is {k} in the header, {g} in SIGNATURES" for i, (k, g) in enumerate(zip(kinds, got)) if k != g]
    assert not bad, "\n".join(bad)
