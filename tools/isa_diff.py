#!/usr/bin/env python3
"""Compare the device assembly of two versions of the kernels, function by function (CPU only: hipcc cross-compiles).

    python tools/isa_diff.py PARENT BRANCH

Each side is a source tree (its llmrec_amd/csrc is compiled: every entry of build.SOURCES with build.FLAGS plus
--cuda-device-only -S), a directory of .hip files, or a directory of .s files. The report lists the symbols only one side has, the
symbols whose instruction streams differ and, for each of those, the opcode counts that differ - the floating-point ones
(mnemonics containing _f32, _f64, _f16, _bf16 or mfma) separately: a refactor may move registers and reorder instructions, but a
changed floating-point count is a changed contraction, i.e. new bits. Exit status 1 when a floating-point count or a symbol set
differs. The tool only compares; it knows no instruction by name."""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmrec_amd import build  # noqa: E402

FP = ("_f32", "_f64", "_f16", "_bf16", "mfma")
SYMBOL = re.compile(r"^([A-Za-z_$][\w$.]*):")        # a function's label; local block labels start with a dot


def assembly(side, tmp):
    """{file stem: assembly text} of one side."""
    if glob.glob(os.path.join(side, "*.s")):
        return {os.path.basename(p)[:-2]: open(p).read() for p in sorted(glob.glob(os.path.join(side, "*.s")))}
    csrc = os.path.join(side, "llmrec_amd", "csrc")
    if os.path.isdir(csrc):
        srcs = [os.path.join(csrc, s) for s in build.SOURCES if os.path.exists(os.path.join(csrc, s))]   # (a file one side lacks: "only in")
    else:
        srcs = sorted(glob.glob(os.path.join(side, "*.hip")))

    def one(src):
        out = os.path.join(tmp, os.path.basename(src)[:-4] + ".s")
        r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stderr[-4000:]))
        return os.path.basename(src)[:-4], open(out).read()

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(ex.map(one, srcs))


def functions(text):
    """{symbol: [instruction or local label, ...]}: comments and assembler directives dropped."""
    funcs, cur, in_text = {}, None, True
    for line in text.splitlines():
        line = line.split(";")[0].split("//")[0].strip()
        if not line:
            continue
        m = SYMBOL.match(line) if in_text else None
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif line.startswith(".") and not line.endswith(":"):
            if line.split()[0] in (".text", ".section", ".amdgpu_metadata"):
                in_text = bool(re.match(r"\.text\b|\.section\s+\.text", line))   # kernel descriptors, data and metadata are not code
                cur = None                            # (a function's label follows the directive that re-enters its section)
        elif cur is not None:
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))   # block labels carry the function's ordinal in its file
    return {k: v for k, v in funcs.items() if v}


def opcodes(stream):
    return collections.Counter(i.split()[0] for i in stream if not i.endswith(":"))


def compare(a, b, out=sys.stdout):
    """a, b: {file stem: assembly text}. Prints the report; returns (symbol sets differ, streams differ, fp counts differ)."""
    fa = {(f, s): v for f, t in a.items() for s, v in functions(t).items()}
    fb = {(f, s): v for f, t in b.items() for s, v in functions(t).items()}
    only = sorted(set(fa) ^ set(fb))
    for key in only:
        print("only in %s: %s %s" % ("A" if key in fa else "B", key[0], key[1]), file=out)
    changed = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    fp_changed = []
    for key in changed:
        ca, cb = opcodes(fa[key]), opcodes(fb[key])
        delta = {op: (ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
        fp = {op: d for op, d in delta.items() if any(t in op for t in FP)}
        if fp:
            fp_changed.append(key)
        print("differs: %s %s (%d -> %d instructions)" % (key[0], key[1], sum(ca.values()), sum(cb.values())), file=out)
        print("    opcode counts: %s" % (", ".join("%s %d -> %d" % (op, x, y) for op, (x, y) in delta.items()) or "equal"), file=out)
        print("    floating point: %s" % (", ".join("%s %d -> %d" % (op, x, y) for op, (x, y) in fp.items()) or "equal"), file=out)
    print("%d functions, %d only on one side, %d with a different instruction stream, %d of them with different floating-point counts"
          % (len(set(fa) | set(fb)), len(only), len(changed), len(fp_changed)), file=out)
    return only, changed, fp_changed


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        only, _, fp_changed = compare(assembly(argv[1], ta), assembly(argv[2], tb))
    return 1 if only or fp_changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
