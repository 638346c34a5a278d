"""tools/isa_diff.py on three tiny kernels (hipcc cross-compiles for gfx950, no GPU): the tool that decides whether a kernel refactor
changed the arithmetic must itself tell the three cases apart -

  the same source twice                                        -> nothing reported, exit status 0
  a * b + c rewritten as fmaf(a, b, c), contraction off        -> reported with a floating-point opcode difference, exit status 1
  the expression moved into a __forceinline__ helper           -> identical instruction stream, exit status 0"""
import importlib.util
import io
import os

import pytest

from tests._hipcc import needs_hipcc

pytestmark = needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "_Z4axpyPKfS0_S0_Pf"

KERNEL = """#include <hip/hip_runtime.h>
%s
__global__ void axpy(const float* a, const float* b, const float* c, float* o) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = %s;
}
"""
HELPER = """__device__ __forceinline__ float mul_add(float a, float b, float c) {
#pragma clang fp contract(off)
    return a * b + c;
}"""
VARIANTS = {"plain": ("", "a[i] * b[i] + c[i]"), "fused": ("", "fmaf(a[i], b[i], c[i])"), "helper": (HELPER, "mul_add(a[i], b[i], c[i])")}


@pytest.fixture(scope="module")
def isa_diff():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def trees(isa_diff, tmp_path_factory):
    """one directory of assembly per variant, compiled once by the tool from a source directory that holds the kernel as axpy.hip (the tool
    pairs functions by file and symbol); the tests hand the tool these directories, its second kind of input"""
    dirs = {}
    for name, (helper, expr) in VARIANTS.items():
        src, asm = tmp_path_factory.mktemp(name + "_src"), tmp_path_factory.mktemp(name)
        (src / "axpy.hip").write_text(KERNEL % (helper, expr))
        assert list(isa_diff.assembly(str(src), str(asm))) == ["axpy"] and (asm / "axpy.s").exists()
        dirs[name] = str(asm)
    return dirs


def report(isa_diff, a, b):
    out = io.StringIO()
    asm_a, asm_b = isa_diff.assembly(a, None), isa_diff.assembly(b, None)
    assert SYMBOL in isa_diff.functions(asm_a["axpy"]) and SYMBOL in isa_diff.functions(asm_b["axpy"]), list(isa_diff.functions(asm_a["axpy"]))
    only, changed, fp_changed = isa_diff.compare(asm_a, asm_b, out)
    print(out.getvalue())
    return only, changed, fp_changed, out.getvalue()


def test_a_source_against_itself_reports_nothing(isa_diff, trees):
    only, changed, fp_changed, text = report(isa_diff, trees["plain"], trees["plain"])
    assert only == [] and changed == [] and fp_changed == []
    assert "differs" not in text and "only in" not in text
    assert isa_diff.main(["isa_diff", trees["plain"], trees["plain"]]) == 0


def test_a_written_out_fma_is_a_floating_point_difference(isa_diff, trees):
    only, changed, fp_changed, text = report(isa_diff, trees["plain"], trees["fused"])
    assert only == []
    assert changed == [("axpy", SYMBOL)] and fp_changed == [("axpy", SYMBOL)]
    fp_line = [ln for ln in text.splitlines() if ln.strip().startswith("floating point:")]
    assert len(fp_line) == 1 and "equal" not in fp_line[0] and "_f32" in fp_line[0], text
    assert isa_diff.main(["isa_diff", trees["plain"], trees["fused"]]) == 1


def test_a_helper_moved_into_a_forceinline_function_is_identical(isa_diff, trees):
    only, changed, fp_changed, _ = report(isa_diff, trees["plain"], trees["helper"])
    assert only == [] and changed == [] and fp_changed == []
    assert isa_diff.main(["isa_diff", trees["plain"], trees["helper"]]) == 0
