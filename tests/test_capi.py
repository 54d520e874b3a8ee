"""The C-ABI library: loads, exports every symbol include/cfhip.h declares, the ctypes table derived from the
header agrees with it (by name here, by type through a C compiler), and argument validation returns errors
(no compute without a GPU)."""
import ctypes
import os
import re
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

import cflearn_amd
from cflearn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cfhip_\w+)\s*\(", text)))


def test_header_symbols_exported():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"libcfhip.so does not export {n}"


def test_ctypes_table_matches_header():
    """names only, found by a regex of this file: guards `_lib.parse_header` against dropping a prototype"""
    assert sorted(_lib.SIGNATURES) == _declared()


C_SCALAR = {c_int: "int", c_int64: "int64_t", c_uint64: "uint64_t", c_size_t: "size_t", c_float: "float", c_double: "double"}


def _abi_check_source(header_text, signatures, fields):
    """A C file that holds `&cfhip_x` in a function pointer spelled from each row of `signatures`, and the layout of
    `fields` as _Static_asserts on cfhip_gemm_problem: a C compiler then compares the rows with the header it includes,
    and `_lib.parse_header` has no part in that.  Return type and every scalar are spelled from the row alone.  ctypes has
    one type for all data pointers and C has none, so a pointer position borrows the header's own words for that parameter
    (its text up to the last `*`), and must have a `*` there; c_char_p must be spelled `const char*`."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    lines = ["#include <stddef.h>", "#include <stdint.h>", '#include "cfhip.h"']
    for name, (restype, argtypes) in signatures.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        params = [] if m.group(1).strip() == "void" else m.group(1).split(",")
        spelled = []  # as many as the ROW has: the compiler judges the arity too
        for i, t in enumerate(argtypes):
            param = params[i] if i < len(params) else "void*"
            if t in C_SCALAR:
                spelled.append(C_SCALAR[t])
                continue
            assert t in (c_void_p, c_char_p) and "*" in param, f"{name} argument {i}: {t.__name__} against `{param.strip()}`"
            spelled.append(" ".join(param[:param.rindex("*") + 1].split()))
            assert (t is c_char_p) == (spelled[-1] == "const char*"), f"{name} argument {i}: {t.__name__} against `{param.strip()}`"
        ret = "const char*" if restype is c_char_p else C_SCALAR[restype]
        lines.append(f"{ret} (*const p_{name})({', '.join(spelled) or 'void'}) = &{name};")
    lines.append(f'_Static_assert(sizeof(cfhip_gemm_problem) == {ctypes.sizeof(_lib.GemmProblem)}, "sizeof");')
    for fname, ftype in fields:
        lines.append(f'_Static_assert(offsetof(cfhip_gemm_problem, {fname}) == {getattr(_lib.GemmProblem, fname).offset}, "{fname} offset");')
        lines.append(f'_Static_assert(sizeof(((cfhip_gemm_problem*)0)->{fname}) == {ctypes.sizeof(ftype)}, "{fname} size");')
    return "\n".join(lines) + "\n"


def _abi_check(tmp_path, header_text, signatures, fields=None):
    """compile (never link, never run) the file above against `header_text` saved as cfhip.h; the compiler's result"""
    inc = tmp_path / "include"
    inc.mkdir(exist_ok=True)
    (inc / "cfhip.h").write_text(header_text)
    src = tmp_path / "abi_check.c"
    src.write_text(_abi_check_source(header_text, signatures, _lib.GemmProblem._fields_ if fields is None else fields))
    return subprocess.run([os.environ.get("CC", "gcc"), "-std=c11", "-c", "-Werror", "-Wincompatible-pointer-types", f"-I{inc}",
                           str(src), "-o", str(tmp_path / "abi_check.o")], capture_output=True, text=True)


def _header_text():
    with open(_lib.HEADER_PATH) as f:
        return f.read()


def test_ctypes_table_types_match_header_by_compiler(tmp_path):
    """Every row of `_lib.SIGNATURES` (arity, return type, every scalar type, pointer or scalar at every position) and the
    layout of `_lib.GemmProblem` against include/cfhip.h, judged by gcc: a `c_int` where the header says `int64_t` or
    `size_t` would be truncated silently by ctypes and by the vectorcall module alike, and is a compile error here."""
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "cfhip.h"))
    r = _abi_check(tmp_path, _header_text(), _lib.SIGNATURES)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(_lib.GemmProblem) == 80 and _lib.GemmProblem.lda.offset == 48  # 4 pointers, 3 int, pad, 3 int64, 2 int


def test_abi_checks_bite(tmp_path):
    """Mutants.  (1) the header's `int64_t lda` of cfhip_gemm_bf16 becomes `int`: the derived table differs, and with the
    table held fixed the compile check fails.  (2) the header fixed, one row of the table narrowed (`int64_t n` -> c_int,
    `size_t workspace_bytes` -> c_int), an argument dropped or added, a return type changed: the compile check fails each time.
    (3) one struct field narrowed in the header (`int64_t lda, ldb, ldc` -> int): derived fields differ, _Static_asserts fail."""
    good = _header_text()
    sigs = {k: (r, list(a)) for k, (r, a) in _lib.SIGNATURES.items()}

    mutant = good.replace("int M, int N, int K, int64_t lda, int64_t ldb,", "int M, int N, int K, int lda, int64_t ldb,", 1)  # the first is cfhip_gemm_bf16
    assert mutant != good
    derived = _lib.parse_header(mutant)[0]
    assert derived["cfhip_gemm_bf16"][1][9] is c_int and _lib.SIGNATURES["cfhip_gemm_bf16"][1][9] is c_int64
    assert {k for k in sigs if derived[k] != _lib.SIGNATURES[k]} == {"cfhip_gemm_bf16"}
    r = _abi_check(tmp_path, mutant, _lib.SIGNATURES)
    assert r.returncode != 0 and "p_cfhip_gemm_bf16" in r.stderr, r.stderr

    def row_mutant(name, change):
        rows = {k: (r, list(a)) for k, (r, a) in sigs.items()}
        rows[name] = change(*rows[name])
        r = _abi_check(tmp_path, good, rows)
        assert r.returncode != 0 and f"p_{name}" in r.stderr, (name, r.stderr)

    assert sigs["cfhip_gelu_fwd"][1][2] is c_int64 and sigs["cfhip_colsum_bf16"][1][7] is c_size_t
    row_mutant("cfhip_gelu_fwd", lambda r, a: (r, a[:2] + [c_int] + a[3:]))
    row_mutant("cfhip_colsum_bf16", lambda r, a: (r, a[:7] + [c_int] + a[8:]))
    assert sigs["cfhip_dropout"][1][4] is c_double  # the one double of the ABI: a c_float row would pass half its bits
    row_mutant("cfhip_dropout", lambda r, a: (r, a[:4] + [c_float] + a[5:]))
    row_mutant("cfhip_spin", lambda r, a: (r, a[:1]))
    row_mutant("cfhip_spin", lambda r, a: (r, a + [c_int]))
    row_mutant("cfhip_colsum_workspace", lambda r, a: (c_int, a))
    with pytest.raises(AssertionError, match="cfhip_spin argument 0"):  # a pointer row against a scalar parameter
        _abi_check(tmp_path, good, {**sigs, "cfhip_spin": (c_int, [c_void_p, c_void_p])})
    row_mutant("cfhip_spin", lambda r, a: (r, [c_int, c_int]))  # a scalar row against a pointer parameter

    mutant = good.replace("  int64_t lda, ldb, ldc;", "  int lda, ldb, ldc;")
    assert mutant != good
    fields = _lib.parse_header(mutant)[1]["cfhip_gemm_problem"]
    assert fields != _lib.GemmProblem._fields_ and [n for n, _ in fields] == [n for n, _ in _lib.GemmProblem._fields_]
    r = _abi_check(tmp_path, mutant, _lib.SIGNATURES)
    assert r.returncode != 0 and "static assertion failed" in r.stderr, r.stderr


def test_header_parser_cases():
    """`_lib.parse_header` on strings: what it must read, and that it refuses what it does not know"""
    sigs, structs, defines = _lib.parse_header("""
        #ifndef X_H
        #define X_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define CFHIP_A 3     /* a comment with a prototype in it: int cfhip_ghost(int x); */
        #define CFHIP_NEG (-2)
        #define CFHIP_NOT_AN_INT 1.5f
        // int cfhip_ghost2(void);
        int cfhip_many(const void* A, float* out,
                       int M, int64_t ld,   /* split over lines */
                       uint64_t seed, size_t bytes, float eps,
                       double p, void* stream);
        int cfhip_none(void);
        const char* cfhip_text(const char* name, char* out);
        size_t cfhip_size(const void* const* tables, void** comm, const int32_t *plan, const uint8_t* mask);
        typedef struct cfhip_s {
          const void* A;
          float *g;
          int M, N;      /* two fields */
          int64_t ld;
        } cfhip_s;
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert sigs == {
        "cfhip_many": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_uint64, c_size_t, c_float, c_double, c_void_p]),
        "cfhip_none": (c_int, []),
        "cfhip_text": (c_char_p, [c_char_p, c_void_p]),
        "cfhip_size": (c_size_t, [c_void_p, c_void_p, c_void_p, c_void_p]),
    }
    assert structs == {"cfhip_s": [("A", c_void_p), ("g", c_void_p), ("M", c_int), ("N", c_int), ("ld", c_int64)]}
    assert defines == {"CFHIP_A": 3, "CFHIP_NEG": -2}
    for bad, what in (("int cfhip_f(long n);", "'long n' in cfhip_f"), ("int cfhip_f(unsigned int n);", "cfhip_f"),
                      ("short cfhip_f(int n);", "'short' in cfhip_f"), ("int cfhip_f(uint8_t flag);", "cfhip_f"), ("int cfhip_f(long double p);", "cfhip_f"),
                      ("int cfhip_f(int (*callback)(int));", "not a prototype"), ("int other_name(int n);", "not a prototype"),
                      ("typedef struct s { short x; } s;", "struct s"), ("int cfhip_f(int n) { return n; }", "not a prototype")):
        with pytest.raises(ValueError, match=re.escape(what)):
            _lib.parse_header(bad)


def test_missing_header_fails_loudly(tmp_path):
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "cfhip.h"))):
        _lib.read_header(str(tmp_path / "cfhip.h"))


def test_header_constants_reach_ops():
    """the public names and values of ops' shared constants, now read from the header's #defines"""
    from cflearn_amd import ops

    assert (ops.EPI_NONE, ops.EPI_GELU, ops.EPI_RESIDUAL, ops.EPI_DGELU, ops.EPI_QGELU, ops.EPI_DQGELU) == (0, 1, 2, 3, 4, 5)
    assert ops.SAMPLE_ROW == 8 and ops.SAMPLERS == {"ddim": 0, "basic": 1} and ops.PARAMETERIZATIONS == {"eps": 0, "x0": 1, "v": 2}
    assert ops.TIME_PROJ_MAX == 32 and ops.PACK_GROUP_MAX == 64
    conv = open(os.path.join(ROOT, "carefree-learn_amd", "csrc", "conv.hip")).read()
    assert "TP_MAX = CFHIP_TIME_PROJ_MAX;" in conv and "PK_MAX = CFHIP_PACK_GROUP_MAX;" in conv


def test_version_and_error_string():
    lib = _lib.load()
    assert lib.cfhip_version() == 100
    # invalid arguments are rejected before any launch, with a message
    rc = lib.cfhip_gemm_bf16(None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, None, 0, None, 0, None)
    assert rc == -1
    assert b"null" in lib.cfhip_last_error()
    rc = lib.cfhip_layernorm_fwd(1, 0, 1, 1, 1, None, None, 4, 6, 8, 8, 1e-6, None)
    assert rc == -1 and b"multiple of 4" in lib.cfhip_last_error()
    # (long sequences are no longer an error: the chunked kernels take them) head_dim outside the supported set is
    rc = lib.cfhip_attn_fwd_dh(16, 16, 16, 16, None, None, 1, 1, 300, 300, 200, 256, 256, 256, 256, 256, 256, 0, 0, 0,
                               0.125, 0, None)
    assert rc == -1 and b"head_dim" in lib.cfhip_last_error()
    with pytest.raises(RuntimeError, match="head_dim"):
        _lib.check(rc, "attn_fwd")
    # GroupNorm's split form (splits > 1) refuses what only the one-workgroup forms take: inner % 8 != 0, and in backward
    # more than CFHIP_GN_MAX_CG channels per group (the pointers are never dereferenced: the refusal comes before any launch)
    p = 256
    rc = lib.cfhip_groupnorm_fwd(p, 0, None, p, p, p, p, p, 1, 8, 4, 12, 1e-6, 0, 0, 2, p, None)
    assert rc == -1 and b"groupnorm_fwd: the split form" in lib.cfhip_last_error()
    rc = lib.cfhip_groupnorm_bwd(p, p, 0, None, p, p, p, p, p, p, p, None, 1, 8, 4, 12, 0, 0, 2, p, None)
    assert rc == -1 and b"groupnorm_bwd: the split form" in lib.cfhip_last_error()
    assert _lib.DEFINES["CFHIP_GN_MAX_CG"] == 128
    rc = lib.cfhip_groupnorm_bwd(p, p, 0, None, p, p, p, p, p, p, p, None, 1, 136, 1, 16, 0, 0, 2, p, None)
    assert rc == -1 and b"groupnorm_bwd: the split form" in lib.cfhip_last_error() and b"128 channels per group" in lib.cfhip_last_error()


def test_workspace_queries():
    lib = _lib.load()
    assert lib.cfhip_colsum_workspace(12608, 768) >= 768 * 4
    assert lib.cfhip_layernorm_bwd_workspace(12608, 768) >= 2 * 768 * 4


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libcfhip.so"))
    with pytest.raises(RuntimeError, match="no fallback"):
        _lib.load()


def test_ops_refuse_cpu_tensors():
    import torch

    a = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP device"):
        cflearn_amd.ops.gemm(a, a)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "carefree-learn_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "vit_oracle" not in src and "refharness" not in src and "import oracle" not in src, f


def test_conv3x3_host_side_checks_and_split_heuristic():
    """No launch happens: argument validation and the split-K decision of the implicit-GEMM convolution."""
    lib = _lib.load()
    # one K-step = 32 channels of a tap
    rc = lib.cfhip_conv3x3_nhwc_bf16(16, 16, None, 16, 1, 8, 8, 48, 64, None, 0, None)
    assert rc == -1 and b"multiple of 32" in lib.cfhip_last_error()
    rc = lib.cfhip_conv3x3_nhwc_bf16(16, 16, None, 16, 1, 8, 8, 64, 60, None, 0, None)
    assert rc == -1 and b"multiple of 8" in lib.cfhip_last_error()
    rc = lib.cfhip_conv3x3_wgrad_nhwc_bf16(16, 16, 16, 0, None, 0, 1, 1, 8, 64, 64, 1, None, 0, None)
    assert rc == -1 and b"bad image shape" in lib.cfhip_last_error()
    rc = lib.cfhip_conv3x3_pack_filters(16, 16, 8, 12, 0, None)
    assert rc == -1
    # zoo UNet at 64^2 x 8: level 0 (32768 pixels x 320) fills the chip -> no split, no workspace; the deeper levels
    # (8192 x 640: 160 tiles, 2048 x 1280: 80, 512 x 1280: 40) split and ask for split * pixels * Cout fp32
    assert lib.cfhip_conv3x3_workspace(8, 64, 64, 320, 320) == 0
    for (hw, cin, cout) in ((32, 640, 640), (16, 1280, 1280), (8, 1280, 1280)):
        nbytes = lib.cfhip_conv3x3_workspace(8, hw, hw, cin, cout)
        pixels = 8 * hw * hw
        assert nbytes > 0 and nbytes % (pixels * cout * 4) == 0
        split = nbytes // (pixels * cout * 4)
        assert 2 <= split <= (9 * cin // 64) // 8
    assert lib.cfhip_conv3x3_wgrad_workspace(320, 640, 4) == 4 * 640 * (9 * 320 + 1) * 4


def test_vectorcall_entry_module_is_the_same_library():
    """`_cfhip_fast` (csrc/gen_fastcall.py): METH_FASTCALL wrappers of the SAME loaded libcfhip.so, generated from
    `_lib.SIGNATURES` — every entry point whose arguments are plain numbers is served by it, the others (ctypes objects /
    strings at their call sites) stay on ctypes; wrong argument counts / types are Python errors raised BEFORE the library
    is entered; return codes and error strings are the library's."""
    if not os.path.isfile(_lib.FAST_PATH) or os.environ.get("CFHIP_FASTCALL", "1") == "0":
        pytest.skip("the vectorcall module is not built (build_lib.sh / __graft_entry__.build() builds it)")
    lib = _lib.load()
    assert type(lib).__name__ == "_FastLib" and _lib.fast_bound >= 75
    cdll = lib.__dict__["_cdll"]
    fast_names = [n for n in _lib.SIGNATURES if n in lib.__dict__]
    slow_names = [n for n in _lib.SIGNATURES if n not in lib.__dict__]
    assert "cfhip_gemm_bf16" in fast_names and "cfhip_adam_step_dev" in fast_names and "cfhip_attn_fwd_dh" in fast_names
    assert all(_lib.ctypes_only(n) for n in slow_names), slow_names
    args = (None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, None, 0, None, 0, None)
    assert lib.cfhip_gemm_bf16(*args) == cdll.cfhip_gemm_bf16(*args) == -1 and b"null" in lib.cfhip_last_error()
    assert lib.cfhip_colsum_workspace(1000, 64) == cdll.cfhip_colsum_workspace(1000, 64) > 0
    assert lib.cfhip_layernorm_bwd_workspace(512, 768) == cdll.cfhip_layernorm_bwd_workspace(512, 768)
    with pytest.raises(TypeError, match="23 arguments"):
        lib.cfhip_gemm_bf16(1, 2, 3)
    with pytest.raises(TypeError):
        lib.cfhip_colsum_workspace("a", 3)
    with pytest.raises((TypeError, OverflowError)):
        lib.cfhip_gemm_bf16(*(("x",) + args[1:]))


def test_kernels_spill_only_where_documented(tmp_path):
    """The code objects inside the built libcfhip.so: no kernel uses scratch memory except the three head_dim-64 long-sequence attention
    instantiations DESIGN.md §3.5 names (12-36 bytes; built without scratch they are 6-16 % slower, profiles/r05/attn_ndt4_scratch_ab.txt).
    Read from the kernels' metadata notes with the ROCm LLVM tools — a compiler flag or an edit that makes a kernel spill shows up here,
    on the CPU, before it costs anything on the GPU."""
    import re
    import shutil
    import subprocess

    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("ROCm LLVM tools or the built library are missing")
    fat = tmp_path / "fat.bin"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", _lib.LIB_PATH, str(tmp_path / "stripped.so")], check=True)
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]  # one bundle per translation unit
    assert len(starts) >= 10, len(starts)
    kernels, spilling = 0, {}
    for i, off in enumerate(starts):
        blob = tmp_path / f"bundle{i}.bin"
        blob.write_bytes(data[off:starts[i + 1] if i + 1 < len(starts) else len(data)])
        elf = tmp_path / f"code{i}.elf"
        subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={blob}",
                        f"--output={elf}"], check=True, capture_output=True)
        notes = subprocess.run([tools[2], "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            kernels += 1
            if int(scratch) > 0:
                spilling[name] = int(scratch)
    shutil.rmtree(tmp_path, ignore_errors=True)
    assert kernels > 400, kernels
    allowed = ("attn_fwd2_kernelILb1ELi4ELb0E", "attn_fwd2_kernelILb0ELi4ELb0E", "attn_bwd_dq2_kernelILb1ELi4E")
    unexpected = {k: v for k, v in spilling.items() if not any(a in k for a in allowed)}
    assert not unexpected, unexpected
    assert all(v <= 64 for v in spilling.values()), spilling
