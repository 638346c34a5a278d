"""ctypes binding of the C ABI declared in include/llmrec_hip.h.

Everything that crosses the ABI is parsed from the header itself at import - the prototypes (parse_header), the argument-block structs
(parse_structs -> STRUCT) and the constants (header_constants -> CONST: the object-like #defines and the status enum) - so the Python side
cannot drift from the C declarations. There is deliberately NO fallback: if libllmrec_hip.so is missing or a call
returns a non-zero status, a RuntimeError is raised (the product path must fail loudly rather
than silently run something else)."""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "llmrec_hip.h")
HOST_HEADER = os.path.join(os.path.dirname(HERE), "include", "llmrec_host.h")      # libllmrec_host.so: utility/load_data.py binds it with parse_header
# LLMREC_LIB: tools/ load the instrumented build (python -m llmrec_amd.build --tools) through the same binding
LIB_PATH = os.environ.get("LLMREC_LIB") or os.path.join(HERE, "lib", "libllmrec_hip.so")

_SCALARS = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
    "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float,
    "double": ctypes.c_double, "llmrec_stream_t": ctypes.c_void_p, "void": None,
}


def _code(path: str, directives: bool = False) -> str:
    """The header without its comments and (unless directives) without its preprocessor lines."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return text if directives else re.sub(r"#[^\n]*", " ", text)


def parse_header(path: str = HEADER):
    """Return {name: (restype, [argtypes], [argnames])} for every prototype in the header."""
    text = _code(path)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(llmrec_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.startswith("typedef"):
            continue
        restype = ctypes.c_char_p if "char" in ret and "*" in ret else _SCALARS[ret.replace("const", "").strip()]
        argtypes, argnames = [], []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                argnames.append(re.findall(r"\w+", a)[-1])
                if "*" in a:
                    argtypes.append(ctypes.c_void_p)
                else:
                    argtypes.append(_SCALARS[a.replace("const", "").split()[0]])
        protos[name] = (restype, argtypes, argnames)
    return protos


def _closing_brace(text: str, i: int) -> int:
    """Index of the brace that closes the one at text[i]."""
    depth = 0
    for m in re.compile(r"[{}]").finditer(text, i):
        depth += 1 if m.group() == "{" else -1
        if depth == 0:
            return m.start()
    raise ValueError("unbalanced braces")


def _fields(body: str, known: dict, owner: str):
    """The ctypes _fields_ of a struct / union body. A declarator with a `*` is a c_void_p (as in the prototypes); a scalar comes from
    _SCALARS; a member of an earlier typedef is that class by value; `union { ... } name;` is a Union of the same rules. Anything else -
    an array, a bit-field, a function pointer, a nested struct, an unknown type - is an error, never skipped."""
    def bad(decl, why):
        return ValueError("%s: cannot bind `%s` (%s)" % (owner, " ".join(decl.split()), why))
    fields, i = [], 0
    while body[i:].strip():
        brace, semi = body.find("{", i), body.find(";", i)
        if semi < 0:
            raise bad(body[i:], "no `;`")
        if 0 <= brace < semi:                                    # a braced member: only `union { ... } name;`
            close = _closing_brace(body, brace)
            semi = body.find(";", close)
            decl = body[i:semi if semi >= 0 else len(body)]
            name = body[close + 1:semi].strip() if semi >= 0 else ""
            if body[i:brace].split() != ["union"] or not re.fullmatch(r"\w+", name):
                raise bad(decl, "only `union { ... } name;` may be nested")
            inner = "%s.%s" % (owner, name)
            fields.append((name, type(inner, (ctypes.Union,), {"_fields_": _fields(body[brace + 1:close], known, inner), "__doc__": inner})))
        else:
            decl = body[i:semi]
            parts = [[w for w in p.split() if w != "const"] for p in decl.replace("*", " * ").split(",")]
            base = [w for w in parts[0][:-1] if w != "*"]
            if re.search(r"[^\w\s\*,]", decl) or len(base) != 1 or not all(p and re.fullmatch(r"[A-Za-z_]\w*", p[-1]) for p in parts):
                raise bad(decl, "an array, bit-field, function pointer or other form the binding does not know")
            ctype = known.get(base[0]) or _SCALARS.get(base[0])
            if ctype is None:
                raise bad(decl, "unknown type `%s`" % base[0])
            for n, p in enumerate(parts):
                if n and [w for w in p[:-1] if w != "*"]:
                    raise bad(decl, "a second type in one declaration")
                fields.append((p[-1], ctypes.c_void_p if "*" in p else ctype))
        i = semi + 1
    return fields


def parse_structs(path: str = HEADER):
    """Return {typedef name: ctypes.Structure subclass} for every `typedef struct { ... } name;` of the header, in header order."""
    text = _code(path)
    typedefs = list(re.finditer(r"\btypedef\s+struct\b\s*(.)", text))
    typedef_name = re.compile(r"\s*([A-Za-z_]\w*)\s*;")
    out = {}
    for m in typedefs:
        close = _closing_brace(text, m.end(1) - 1) if m.group(1) == "{" else -1
        tail = typedef_name.match(text, close + 1) if close >= 0 else None
        if not tail or tail.group(1) in out:
            raise ValueError("%s: `%s ...` is not `typedef struct { ... } new_name;`" % (path, " ".join(text[m.start():m.start() + 60].split())))
        name = tail.group(1)
        out[name] = type(name, (ctypes.Structure,), {"_fields_": _fields(text[m.end(1):close], out, name), "__doc__": name})
    if len(out) != len(typedefs):
        raise ValueError("%s: %d typedef structs bound, %d declared" % (path, len(out), len(typedefs)))
    return out


def header_constants(path: str = HEADER):
    """Return {name: value} for the object-like `#define LLMREC_*` (function-like macros stay out) and the `enum { ... }` entries."""
    text = _code(path, directives=True)
    out = {}
    # a decimal literal, or a power of two written (1 << n)
    for m in re.finditer(r"#define\s+(LLMREC_\w+)\s+(?:(-?\d+)|\(1\s*<<\s*(\d+)\))", text):
        out[m.group(1)] = int(m.group(2)) if m.group(2) is not None else 1 << int(m.group(3))
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for entry in filter(None, (e.strip() for e in body.split(","))):
            m = re.fullmatch(r"(LLMREC_\w+)\s*=\s*(-?\d+)", entry)
            if not m:
                raise ValueError("%s: cannot read the enum entry `%s`" % (path, entry))
            out[m.group(1)] = int(m.group(2))
    return out


CONST = header_constants()
STRUCT = parse_structs()
_lib = None
_protos = None


def load():
    """Load the shared library (once) and attach the parsed prototypes."""
    global _lib, _protos
    if _lib is not None:
        return _lib
    # torch bundles its own ROCm runtime (torch/lib/libamdhip64.so); it must be the one in the
    # process before this library resolves libamdhip64.so.7, or two HIP runtimes get loaded and
    # launches fail with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "llmrec_amd: %s is missing. Build it with `python -m llmrec_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the HIP hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    _protos = parse_header()
    for name, (restype, argtypes, _) in _protos.items():
        fn = getattr(lib, name)            # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.llmrec_abi_version() != CONST["LLMREC_ABI_VERSION"]:
        raise RuntimeError("llmrec_amd: libllmrec_hip.so ABI %d != header ABI %d; rebuild"
                           % (lib.llmrec_abi_version(), CONST["LLMREC_ABI_VERSION"]))
    _lib = lib
    return lib


_TRACE = os.environ.get("LLMREC_TRACE_CALLS", "0") == "1"
n_calls = 0      # entry-point invocations so far (FusedStep reports the per-step delta: a launch-count proxy without a profiler)


EUNSUPPORTED = CONST["LLMREC_EUNSUPPORTED"]       # the arguments are valid but outside what the library compiled


def _invoke(name: str, args) -> int:
    global n_calls
    n_calls += 1
    lib = load()
    if _TRACE:                                               # LLMREC_TRACE_CALLS=1 (debugging a device fault): name each entry point, synchronise behind it
        import sys
        import torch
        print("[llmrec] %s" % name, file=sys.stderr, flush=True)
        status = getattr(lib, name)(*args)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize()
    else:
        status = getattr(lib, name)(*args)
    return status


def _raise(name: str, status: int):
    lib = load()
    raise RuntimeError("%s failed: %s (%s)" % (
        name, lib.llmrec_status_string(status).decode(), lib.llmrec_last_error().decode()))


def call(name: str, *args):
    """Invoke an int-returning entry point; raise on a non-zero status."""
    status = _invoke(name, args)
    if status != 0:
        _raise(name, status)


def call_unless_unsupported(name: str, *args) -> bool:
    """call(), except that LLMREC_EUNSUPPORTED (nothing was launched) returns False: the caller then takes another path."""
    status = _invoke(name, args)
    if status == EUNSUPPORTED:
        return False
    if status != 0:
        _raise(name, status)
    return True


def query(name: str, *args) -> int:
    """Invoke an int64-returning size query."""
    return int(getattr(load(), name)(*args))
