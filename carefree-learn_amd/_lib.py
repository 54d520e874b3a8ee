"""ctypes binding of libcfhip.so (the C-ABI declared in include/cfhip.h).

The library is built in-tree by `__graft_entry__.build()` / `build_lib.sh` and must sit next to
this file.  There is NO fallback: if it is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import re
from ctypes import c_uint64, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# CFHIP_LIB selects another build of the same C-ABI (the benchmark tools use it for the -DCFHIP_ABLATE library)
LIB_PATH = os.environ.get("CFHIP_LIB") or os.path.join(_HERE, "libcfhip.so")

_lib: Optional[ctypes.CDLL] = None


# The C-ABI has ONE definition, include/cfhip.h; everything below is read from it when this module is imported, nothing is
# retyped here.  The package runs in-tree only (cflearn_amd.py at the repository root maps the import name), so the header
# sits at ../include/cfhip.h from this file; like the library, a missing header is an error, not a fallback.
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cfhip.h")
_SCALARS = {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float, "double": c_double}


def _ctype(decl: str, where: str):
    """ctypes type of one C declarator (`const float* gamma`, `int64_t lda`, a bare return type): the scalars of _SCALARS,
    `const char*` -> c_char_p, every other pointer -> c_void_p; anything else raises, naming the prototype"""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else c_void_p
    words = [w for w in words if w != "const"]
    if not words or words[0] not in _SCALARS or len(words) > 2:
        raise ValueError(f"cfhip.h: unrecognised type {decl.strip()!r} in {where}")
    return _SCALARS[words[0]]


def parse_header(text: str):
    """(signatures {name: (restype, argtypes)}, structs {name: _fields_}, defines {CFHIP_*: int}) of a header written like
    include/cfhip.h: prototypes `ret cfhip_name(args);`, `typedef struct`s of plain fields, integer #defines"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CFHIP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)  # read as C: the extern "C" braces
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = structs[name] = []
        for decl in filter(None, map(str.strip, body.split(";"))):  # `int M, N, K` declares three fields of one type
            first, *more = decl.split(",")
            ctype = _ctype(first, f"struct {name}")
            if more and ctype in (c_void_p, c_char_p):
                raise ValueError(f"cfhip.h: one pointer per declaration expected, got {decl!r} in struct {name}")
            fields += [(n.split()[-1].lstrip("*"), ctype) for n in (first.replace("*", "* "), *more)]
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    signatures = {}
    for stmt in filter(None, map(str.strip, text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(cfhip_\w+)\s*\(([^()]*)\)", stmt)
        if m is None:
            raise ValueError(f"cfhip.h: not a prototype of the form `ret cfhip_name(args)`: {' '.join(stmt.split())[:80]!r}")
        ret, name, args = m.groups()
        args = [] if args.strip() in ("", "void") else args.split(",")
        signatures[name] = (_ctype(ret, name), [_ctype(a, name) for a in args])
    return signatures, structs, defines


def read_header(path: str = HEADER_PATH):
    if not os.path.isfile(path):
        raise RuntimeError(f"cfhip.h not found at {path}: the binding is derived from the header that ships in the repository "
                           "(include/ next to the package directory) — there is no hand-written table to fall back to")
    with open(path) as f:
        return parse_header(f.read())


# SIGNATURES: name -> (restype, argtypes) of every entry point; DEFINES: the integer CFHIP_* #defines
SIGNATURES, _STRUCTS, DEFINES = read_header()


class GemmProblem(ctypes.Structure):
    """`cfhip_gemm_problem` of include/cfhip.h (one weight-gradient GEMM of a grouped launch)."""

    _fields_ = _STRUCTS["cfhip_gemm_problem"]


# Entry points that stay on ctypes whether or not the vectorcall module is built (csrc/gen_fastcall.py leaves them out,
# tests/test_capi.py expects exactly these): their callers pass ctypes objects (byref / struct arrays that a recorded launch
# plan must keep alive) or strings — a handful of calls per step.  The first six are host-side queries that launch nothing.
HOST_QUERIES = ("cfhip_version", "cfhip_last_error", "cfhip_set_option", "cfhip_gemm_kernel_name", "cfhip_attn_plan", "cfhip_gemm_last_config")
CTYPES_ONLY = HOST_QUERIES + ("cfhip_gemm_bf16_grouped_tn", "cfhip_layernorm_bwd_partials", "cfhip_layernorm_bwd2")
CTYPES_ONLY_PREFIX = ("cfhip_comm_",)


def ctypes_only(name: str) -> bool:
    return name in CTYPES_ONLY or name.startswith(CTYPES_ONLY_PREFIX)


def host_query(name: str) -> bool:
    """nothing to replay: launch recording passes these through (the `_workspace` size queries are plain numbers in and out,
    so unlike HOST_QUERIES they are served by the vectorcall module)"""
    return name in HOST_QUERIES or name.endswith("_workspace")


def lib_exists() -> bool:
    return os.path.isfile(LIB_PATH)


# Launch recording (fused.StackPlan, round 4): while RECORDER is a list, every C-ABI call made through `load().<name>(...)`
# is executed AND appended as (function, argument tuple) — raw pointers, sizes, stream handles: exactly what a replay needs.
RECORDER: Optional[list] = None


class _Recording:
    __slots__ = ("lib",)

    def __init__(self, lib: ctypes.CDLL) -> None:
        self.lib = lib

    def __getattr__(self, name: str):
        fn = getattr(self.lib, name)
        rec = RECORDER
        if host_query(name):
            return fn

        def call(*args):
            rc = fn(*args)
            if rec is not None:
                rec.append((0, fn, args))
            return rc

        return call


# Vectorcall wrappers (csrc/gen_fastcall.py -> _cfhip_fast.<abi>.so, built next to libcfhip.so): the same entry points of the
# same loaded library, entered through METH_FASTCALL functions that read the integer arguments straight out of the call's
# argument array instead of through ctypes' per-argument converters — ~0.3 us instead of 3-6 us per launch on the one thread
# that issues every launch of a step.  Optional acceleration of the HOST path only (CFHIP_FASTCALL=0 or a missing module:
# plain ctypes); entry points whose callers pass ctypes objects stay on ctypes either way.
FAST_PATH = os.path.join(_HERE, "_cfhip_fast" + (__import__("sysconfig").get_config_var("EXT_SUFFIX") or ".so"))
fast_bound = 0  # entry points served by the vectorcall module in this process


class _FastLib:
    """attribute access = the vectorcall wrapper when there is one, else the ctypes function of the same CDLL"""

    def __init__(self, cdll: ctypes.CDLL, fast) -> None:
        global fast_bound
        self.__dict__["_cdll"] = cdll
        n = 0
        for name in fast.names():
            if name in SIGNATURES and fast.bind(name, ctypes.cast(getattr(cdll, name), c_void_p).value):
                self.__dict__[name] = getattr(fast, name)
                n += 1
        fast_bound = n

    def __getattr__(self, name: str):
        return getattr(self.__dict__["_cdll"], name)


def _load_fast():
    if os.environ.get("CFHIP_FASTCALL", "1") == "0" or not os.path.isfile(FAST_PATH):
        return None
    import importlib.util

    spec = importlib.util.spec_from_file_location("_cfhip_fast", FAST_PATH)
    if spec is None or spec.loader is None:
        return None
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load() -> ctypes.CDLL:
    """Load libcfhip.so once; raises if it has not been built (no CPU / eager fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib if RECORDER is None else _Recording(_lib)  # type: ignore[return-value]
    if not lib_exists():
        raise RuntimeError(
            f"libcfhip.so not found at {LIB_PATH}: run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or ./build_lib.sh) first — the HIP path has no fallback"
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    fast = _load_fast()
    _lib = lib if fast is None else _FastLib(lib, fast)  # type: ignore[assignment]
    return _lib  # type: ignore[return-value]


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().cfhip_last_error()
        raise RuntimeError(f"cfhip {what} failed (code {rc}): {msg.decode() if msg else ''}")
