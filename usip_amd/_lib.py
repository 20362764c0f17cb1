"""ctypes loader of libusip_hip.so -- the only way the product reaches its kernels.

There is no fallback: if the library is missing or fails to load, every operator raises.

The interface is declared once, in include/usip_hip.h.  This module reads that file when it is imported (read_header):
SIGNATURES (the argument and result types lib() installs on every entry point), STRUCTS (the ctypes classes of the
header's structs) and ABI all come from it, so a new entry point or struct field needs its declaration and nothing here.
A declaration the reader cannot map is an error at import, never a guess.  A header that usip_hip.h includes from its own
directory is read the same way into INCLUDED[its file name]; include/usip_hip_indoor_pairs.h's pair is also
STRUCTS_INCLUDED and SIGNATURES_INCLUDED.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# USIP_LIB=<path>: load another BUILD of the same library (same-box A/B of two builds, tools/ab_build.sh); never a fallback
LIB_PATH = os.environ.get("USIP_LIB") or os.path.join(_HERE, "libusip_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "usip_hip.h")      # where usip_amd/build.py takes it from
_lib = None

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
            "unsigned": ctypes.c_uint, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
_POINTEES = ("void", "char", "uint8_t", "unsigned long long")               # types the header only ever points to
_TYPED_POINTERS = {"char": ctypes.c_char_p, "int": ctypes.POINTER(ctypes.c_int), "unsigned": ctypes.POINTER(ctypes.c_uint)}
_DECL = re.compile(r"\s*(?:typedef\s+struct\s+\w*\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
                   r"|(?P<res>[\w\s*]+?)\b(?P<fn>\w+)\s*\((?P<args>[^()]*)\)\s*;"
                   r'|enum\s*\{[^{}]*\}\s*;|extern\s+"C"\s*\{|\})')


def _ctype(text, structs):
    """C type text ("long long", "const float*", "usip_pairs_recipe") -> its ctypes type; every pointer that is not
    const char*, int* or unsigned* goes as an address."""
    base, stars = " ".join(re.sub(r"\bconst\b|\*", " ", text).split()), text.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base in structs:
        return structs[base]
    if stars == 1 and (base in _SCALARS or base in structs or base in _POINTEES):
        return _TYPED_POINTERS.get(base, ctypes.c_void_p)
    raise ValueError("usip_amd: include/usip_hip.h: unknown type %r" % text.strip())


def _declaration(text, structs):
    """`const float* At`, `double a, b`, `float* pc[2]` -> [(name, ctypes type)]."""
    out, base = [], None
    for part in text.split(","):
        m = re.fullmatch(r"\s*(.*?)(\w+)\s*(?:\[(\d+)\])?\s*", part, re.S)
        if m is None or (base is None and not m.group(1).strip()):
            raise ValueError("usip_amd: include/usip_hip.h: cannot read the declaration %r" % " ".join(text.split()))
        kind = m.group(1) if base is None else base + m.group(1)        # `double a, b`: b takes a's type without its stars
        base = m.group(1).replace("*", " ") if base is None else base
        try:
            t = _ctype(kind, structs)
        except ValueError as e:
            raise ValueError("%s in %r" % (e, " ".join(text.split()))) from None
        out.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
    return out


def read_header(text, known=None):
    """C header text -> (STRUCTS: name -> ctypes.Structure class, SIGNATURES: name -> (argtypes, restype)), from every
    `typedef struct ... { ... } name;` and every function declaration, in order.  Anything else but an enum and the
    extern "C" braces raises, and so does a type that is not in the tables above: nothing is guessed.  known: the structs
    of the header that includes this one, which its declarations may name; they are not returned again."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).rstrip()
    structs, signatures, pos = dict(known or {}), {}, 0
    while pos < len(text):
        m = _DECL.match(text, pos)
        if m is None:
            raise ValueError("usip_amd: include/usip_hip.h: cannot read the declaration %r"
                             % " ".join(text[pos:].split(";")[0].split()))
        pos = m.end()
        if m.group("struct"):
            fields = [f for stmt in m.group("body").split(";") if stmt.strip() for f in _declaration(stmt, structs)]
            structs[m.group("struct")] = type(m.group("struct"), (ctypes.Structure,), {"_fields_": fields})
        elif m.group("fn"):
            args = m.group("args").strip()
            params = [] if args == "void" else [d for p in args.split(",") for d in _declaration(p, structs)]
            try:
                signatures[m.group("fn")] = ([t for _, t in params], _ctype(m.group("res"), structs))
            except ValueError as e:
                raise ValueError("%s in %r" % (e, " ".join(m.group(0).split()))) from None
    return {k: v for k, v in structs.items() if k not in (known or {})}, signatures


# once per process; ABI = "abi=<n>" of usip_version(), bumped in the header with every incompatible change of it
with open(HEADER) as _f:
    _text = _f.read()
ABI = int(re.search(r"^#define USIP_ABI (\d+)$", _text, re.M).group(1))
STRUCTS, SIGNATURES = read_header(_text)
# the headers usip_hip.h includes from its own directory (#include "usip_hip_indoor_pairs.h"), read the same way: a part of
# the interface kept in a file of its own has its structs and signatures here, and lib() installs both
INCLUDED = {}                                  # header file name -> (its structs, its signatures), in the order of inclusion
for _name in re.findall(r'^#include "(\w+\.h)"$', _text, re.M):
    _known = dict(STRUCTS)
    for _st, _ in INCLUDED.values():
        _known.update(_st)
    with open(os.path.join(os.path.dirname(HEADER), _name)) as _f:
        INCLUDED[_name] = read_header(_f.read(), known=_known)
# the first header that was split off keeps the names its users read it under
STRUCTS_INCLUDED, SIGNATURES_INCLUDED = INCLUDED.get("usip_hip_indoor_pairs.h", ({}, {}))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "usip_amd: %s is missing. Build it with `python -m usip_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback." % LIB_PATH)
        # PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's).  The tensors we
        # are handed live in THAT runtime, so it must be the one already loaded when our library's
        # dependency is resolved: import torch first, then check that exactly one HIP runtime is mapped.
        import torch  # noqa: F401
        try:
            l = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise RuntimeError("usip_amd: cannot load %s: %s" % (LIB_PATH, e)) from e
        try:
            with open("/proc/self/maps") as f:
                runtimes = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        except OSError:
            runtimes = []
        if len(runtimes) > 1:
            raise RuntimeError("usip_amd: two HIP runtimes are loaded (%s); import torch before anything "
                               "that links libamdhip64" % ", ".join(runtimes))
        for name, (args, res) in list(SIGNATURES.items()) + [s for _, sg in INCLUDED.values() for s in sg.items()]:
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        # ctypes cannot see that a library was built from another header, and results depend on three compile flags (an SLP-vectorised build gave
        # rare wrong values on gfx950): the library says what it is, anything else is refused
        ver = l.usip_version().decode()
        if ("abi=%d" % ABI) not in ver.split() or "flags=no-contract,no-fast-math,no-slp" not in ver.split():
            raise RuntimeError("usip_amd: %s reports %r; this package needs abi=%d built by usip_amd/build.py "
                               "(-ffp-contract=off -fno-fast-math -fno-slp-vectorize)" % (LIB_PATH, ver, ABI))
        # measurement knobs for same-box A/B runs: USIP_TUNE="x3_gemm_tile=3,index_max_ch=4" (include/usip_hip.h)
        for item in filter(None, os.environ.get("USIP_TUNE", "").split(",")):
            name, _, value = item.partition("=")
            if l.usip_set_tuning(name.strip().encode(), int(value)) != 0:
                raise RuntimeError("usip_amd: USIP_TUNE names an unknown knob or value: %r" % item)
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError("usip_amd: %s: invalid argument (USIP_EINVAL)" % what)
    raise RuntimeError("usip_amd: %s: HIP error %d" % (what, rc))
