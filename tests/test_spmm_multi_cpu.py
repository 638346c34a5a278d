"""CPU: the grouped SpMM launch (llmrec_spmm_multi_f32) - the ctypes mirror of llmrec_spmm_problem_t has the C layout, and the grouped
kernels keep the registers and occupancy of the single-problem kernels they group (hipcc's resource remarks)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from llmrec_amd import _lib, ops

HERE = os.path.dirname(os.path.abspath(__file__))
SPMM = os.path.join(os.path.dirname(HERE), "llmrec_amd", "csrc", "spmm.hip")


def test_spmm_problem_layout(tmp_path):
    text = open(_lib.HEADER).read()
    end = re.search(r"\}\s*llmrec_spmm_problem_t\s*;", text)
    assert end
    body = text[text.index("{", text.rfind("typedef struct", 0, end.start())) + 1:end.start()]
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert [f[0] for f in ops.SpmmProblemC._fields_] == names
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % _lib.HEADER, "int main(void) {",
           'printf("%zu", sizeof(llmrec_spmm_problem_t));']
    src += ['printf(" %%zu", offsetof(llmrec_spmm_problem_t, %s));' % n for n in names]
    src += ['printf("\\n");', "return 0; }"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(ops.SpmmProblemC) == out[0]
    assert [getattr(ops.SpmmProblemC, f[0]).offset for f in ops.SpmmProblemC._fields_] == out[1:]
    assert _lib.CONST["LLMREC_SPMM_MAX_PROBLEMS"] == 4 and _lib.CONST["LLMREC_ABI_VERSION"] == 8
    assert "llmrec_spmm_multi_f32" in _lib.parse_header()


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_grouped_kernels_keep_the_single_kernels_occupancy():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, SPMM], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
        for key in ("VGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur].setdefault(key, int(m.group(1)))
    # _ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb0ELb0EEEvNS_8SpmmArgsE <-> _ZN6llmrec17spmm_multi_kernelILi16ELi1ELi4ELb0ELb0EEEvNS_9SpmmMultiE
    pairs = 0
    for name, u in res.items():
        m = re.match(r"_ZN6llmrec17spmm_multi_kernel(I.*E)EvNS_9SpmmMultiE$", name)
        if not m:
            continue
        single = res.get("_ZN6llmrec11spmm_kernel%sEvNS_8SpmmArgsE" % m.group(1))
        assert single is not None, name
        assert u["Occupancy [waves/SIMD]"] == single["Occupancy [waves/SIMD]"], (name, u, single)
        assert u["LDS Size [bytes/block]"] == single["LDS Size [bytes/block]"] and u.get("ScratchSize [bytes/lane]", 0) == 0, (name, u)
        pairs += 1
    assert pairs == 14, pairs                      # 7 vector-load families x {unweighted, weighted}
    # the bench's two instances (d = 64): registers as before the grouped launch existed
    k = lambda w: "_ZN6llmrec11spmm_kernelILi16ELi1ELi4ELb%dELb0EEEvNS_8SpmmArgsE" % w
    assert res[k(0)]["VGPRs"] == 71 and res[k(0)]["Occupancy [waves/SIMD]"] == 7
    assert res[k(1)]["VGPRs"] == 90 and res[k(1)]["Occupancy [waves/SIMD]"] == 5
