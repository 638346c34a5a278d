"""CPU test: what llmrec_amd/_lib.py derives from include/llmrec_hip.h - every struct (_lib.STRUCT) and every constant (_lib.CONST) - is what
the C compiler makes of the same header. For EVERY derived struct one generated C program prints sizeof(T) and, per field (the members of
an inline union included, as u.m), offsetof and sizeof; for every constant its value. A wrong layout would silently corrupt an argument
block; a misread field or constant name does not compile. The same check runs the parser over small synthetic headers."""
import ctypes
import re
import subprocess

import pytest

from llmrec_amd import _lib, ops


def _py_facts(structs, consts):
    facts = {}

    def walk(typename, st, prefix, base):
        for name, ctype in st._fields_:
            f = getattr(st, name)
            facts["%s %s%s" % (typename, prefix, name)] = (base + f.offset, f.size)
            if issubclass(ctype, ctypes.Union):
                walk(typename, ctype, prefix + name + ".", base + f.offset)
    for typename, st in structs.items():
        facts[typename] = (ctypes.sizeof(st),)
        walk(typename, st, "", 0)
    facts.update((name, (value,)) for name, value in consts.items())
    return facts


def differences(header, structs, consts, tmp_path):
    """[(what, C, ctypes)] wherever gcc and the derived classes / constants disagree ([] = none); a program gcc refuses is a difference."""
    want = _py_facts(structs, consts)
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % header, "int main(void) {"]
    for key in want:
        t, _, f = key.partition(" ")
        if f:
            src.append('printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (t, f, t, f, t, f))
        elif t in structs:
            src.append('printf("%s %%zu\\n", sizeof(%s));' % (t, t))
        else:
            src.append('printf("%s %%lld\\n", (long long)(%s));' % (t, t))
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    r = subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], capture_output=True, text=True)
    if r.returncode != 0:
        return [("gcc", r.stderr[-2000:], None)]
    got = {}
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        parts = line.split()
        n = 2 if len(parts) == 4 else 1                                       # "T field offset size" | "T size" | "CONSTANT value"
        got[" ".join(parts[:n])] = tuple(int(x) for x in parts[n:])
    return [(k, got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)]


@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    """(the facts ctypes states about every struct and constant of the header, where gcc differs): one program, one compile per module"""
    return _py_facts(_lib.STRUCT, _lib.CONST), differences(_lib.HEADER, _lib.STRUCT, _lib.CONST, tmp_path_factory.mktemp("layout"))


def test_ctypes_structs_match_the_header(header_check):
    # every typedef of the header is bound (names by a regex of the test's own), and every bound struct and constant is gcc's
    facts, diff = header_check
    assert list(_lib.STRUCT) == re.findall(r"\}\s*(llmrec_\w+_t)\s*;", open(_lib.HEADER).read()) and len(_lib.STRUCT) == 17
    assert all(st.__doc__ == name and issubclass(st, ctypes.Structure) for name, st in _lib.STRUCT.items())
    assert diff == []
    assert set(_lib.STRUCT) | set(_lib.CONST) <= set(facts) and {"LLMREC_EUNSUPPORTED", "LLMREC_BPR_WIDE_MAX_B"} <= set(_lib.CONST)
    assert "LLMREC_ROW_STAMP" not in _lib.CONST                              # function-like macros stay out
    assert (ops.EPI_NONE, ops.EPI_SOFTMAX, ops.EPI_SOFTMAX_BWD) == (0, 1, 2) and ops.TOPK_MODES == {"exact": 0, "prefilter": 1}
    assert _lib.EUNSUPPORTED == _lib.CONST["LLMREC_EUNSUPPORTED"] == -4


def test_spmm_problem_layout_and_group_limits(header_check):
    """llmrec_spmm_problem_t (the grouped launch, llmrec_spmm_multi_f32): every field is in the generated check and gcc agrees."""
    facts, diff = header_check
    st = ops.SpmmProblemC
    assert st is _lib.STRUCT["llmrec_spmm_problem_t"] and len(st._fields_) == 16
    assert all("llmrec_spmm_problem_t " + f[0] in facts for f in st._fields_) and "llmrec_spmm_problem_t" in facts
    assert [d for d in diff if d[0].startswith("llmrec_spmm_problem_t") or d[0] == "gcc"] == []
    assert _lib.CONST["LLMREC_SPMM_MAX_PROBLEMS"] == 4 and _lib.CONST["LLMREC_ABI_VERSION"] == 8
    assert "llmrec_spmm_multi_f32" in _lib.parse_header()


def test_guest_struct_layouts_kinds_and_entry_point(header_check):
    """llmrec_spmm_guest_t, its inline union's members and their three typedefs (llmrec_spmm_multi_guest_f32)."""
    facts, diff = header_check
    members = {"sampler": ops.GuestSamplerC, "plan_reach": ops.GuestPlanReachC, "losses": ops.GuestLossesC}
    for m, st in members.items():
        assert st is _lib.STRUCT["llmrec_guest_%s_t" % m] and "llmrec_spmm_guest_t u." + m in facts
        assert all("%s %s" % (st.__doc__, f[0]) in facts for f in st._fields_) and st.__doc__ in facts
    G = ops.SpmmGuestC                                                       # a field-less subclass of the derived class, with `keep`
    assert issubclass(G, _lib.STRUCT["llmrec_spmm_guest_t"]) and G.keep is None and [f[0] for f in G._fields_] == ["kind", "u"]
    assert ctypes.sizeof(G) == facts["llmrec_spmm_guest_t"][0] and (G.kind.offset, G.u.offset) == (0, facts["llmrec_spmm_guest_t u"][0])
    assert {"llmrec_spmm_guest_t", "llmrec_spmm_guest_t kind", "llmrec_spmm_guest_t u"} <= set(facts)
    assert [d for d in diff if "guest" in d[0] or d[0] == "gcc"] == []
    assert (ops.GUEST_SAMPLER, ops.GUEST_PLAN_REACH, ops.GUEST_LOSSES) == tuple(
        _lib.CONST["LLMREC_SPMM_GUEST_" + k] for k in ("SAMPLER", "PLAN_REACH", "LOSSES")) == (1, 2, 3)
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8
    assert len(_lib.parse_header()["llmrec_spmm_multi_guest_f32"][1]) == 4


def test_the_layout_check_is_not_vacuous(tmp_path, monkeypatch):
    job = _lib.STRUCT["llmrec_zero_rows_job_t"]
    dropped = type("llmrec_zero_rows_job_t", (ctypes.Structure,), {"_fields_": job._fields_[:-1]})
    diff = differences(_lib.HEADER, dict(_lib.STRUCT, llmrec_zero_rows_job_t=dropped), {}, tmp_path)
    assert [d[0] for d in diff] == ["llmrec_zero_rows_job_t"], diff          # a dropped field: the size
    renamed = type("llmrec_zero_tensor_t", (ctypes.Structure,), {"_fields_": [("q", ctypes.c_void_p), ("n", ctypes.c_int64)]})
    assert differences(_lib.HEADER, {"llmrec_zero_tensor_t": renamed}, {}, tmp_path)[0][0] == "gcc"      # a misread name does not compile
    assert differences(_lib.HEADER, {}, dict(_lib.CONST, LLMREC_TOPK_MAX=65), tmp_path) == [("LLMREC_TOPK_MAX", (64,), (65,))]
    monkeypatch.setitem(_lib._SCALARS, "int32_t", ctypes.c_int64)             # a wrong scalar width, through the parser
    diff = differences(_lib.HEADER, _lib.parse_structs(), {}, tmp_path)
    assert ("llmrec_zero_rows_job_t d", (24, 4), (24, 8)) in diff, diff[:5]                               # (same offset: only the field size tells)


SYNTHETIC = """#include <stdint.h>
typedef struct { int32_t n; const float* p; } pad_t;               /* padding before the pointer */
typedef struct { float f; double d; } fd_t;
typedef struct { uint8_t tag; pad_t inner; fd_t more; } by_value_t;  // structs by value
typedef struct {
    int32_t kind;   /* a comment; with a semicolon */
    union { uint8_t small; fd_t big; const int64_t* const* ptr; } u;
} union_t;
typedef struct { int32_t a, b; float x, *y, z; uint64_t last; } lists_t;
"""


def test_parser_on_synthetic_headers(tmp_path):
    h = tmp_path / "synthetic.h"
    h.write_text(SYNTHETIC)
    st = _lib.parse_structs(str(h))
    assert list(st) == ["pad_t", "fd_t", "by_value_t", "union_t", "lists_t"]
    assert differences(str(h), st, {}, tmp_path) == []
    C = ctypes
    assert st["pad_t"]._fields_ == [("n", C.c_int32), ("p", C.c_void_p)] and st["pad_t"].p.offset == 8
    assert (st["fd_t"].d.offset, ctypes.sizeof(st["fd_t"])) == (8, 16)
    assert st["by_value_t"]._fields_[1:] == [("inner", st["pad_t"]), ("more", st["fd_t"])]
    u = dict(st["union_t"]._fields_)["u"]
    assert issubclass(u, C.Union) and u._fields_ == [("small", C.c_uint8), ("big", st["fd_t"]), ("ptr", C.c_void_p)] and C.sizeof(u) == 16
    assert st["lists_t"]._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("x", C.c_float), ("y", C.c_void_p), ("z", C.c_float),
                                      ("last", C.c_uint64)]


@pytest.mark.parametrize("decl", ["float rows[4];", "int32_t flag : 3;", "int (*callback)(int);", "struct { int32_t a; } nested;",
                                  "size_t n;", "void v;", "int32_t a, float b;", "int32_t;"])
def test_parser_rejects_what_it_does_not_understand(tmp_path, decl):
    h = tmp_path / "bad.h"
    h.write_text("typedef struct { int32_t ok; } fine_t;\ntypedef struct { int32_t first; %s int32_t after; } bad_t;\n" % decl)
    with pytest.raises(ValueError, match="bad_t") as e:                       # named: the typedef and the declaration
        _lib.parse_structs(str(h))
    assert decl.rstrip(";").split("{")[0].strip() in str(e.value)


def test_parser_rejects_other_typedef_forms(tmp_path):
    h = tmp_path / "bad.h"
    for text in ("typedef struct tagged { int32_t a; } tagged_t;", "typedef struct { int32_t a; } one_t, two_t;"):
        h.write_text(text)
        with pytest.raises(ValueError):
            _lib.parse_structs(str(h))


def test_spmm_shape_policy():
    # launch-bound graphs: 32 nnz per lane group, wide operands in 64-column slices; HBM-bound graphs: 128 / 512
    assert ops.spmm_shape(64, 55_146) == (0, (128, 2048, 2048))
    assert ops.spmm_shape(448, 55_146) == (64, (128, 2048, 2048))
    assert ops.spmm_shape(448, 55_146, whole_row=True) == (0, (32, 512, 512))
    assert ops.spmm_shape(64, 36_000_000) == (0, (512, 16384, 16384))
    assert ops.spmm_shape(128, 1_000_000_000) == (0, (256, 8192, 8192))
    assert ops.spmm_shape(20, 1000)[0] == 0
