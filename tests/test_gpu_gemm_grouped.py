"""The grouped weight-gradient GEMM (csrc/gemm_grouped.hip, cfhip_gemm_bf16_grouped_tn): every kernel instantiation, per element.

dW_i [M, N] (+)= dY_i^T X_i and db_i [M] (+)= colsum(dY_i) against float64 on the same bf16 operands.  Operands are bf16 of
seeded fp64 randn scaled 0.5 .. 1, read from NaN-surrounded buffers (`poisoned`); outputs are views with ldc > N between
sentinel rows inside byte-guarded buffers, NaN where the launch writes, 3.0 (dW) / 5.0 (db) where it accumulates; every case
ends with the guard check and no element is left out of any comparison.  float64 references stay on the CPU, computed once per
operand pair (`_REF`).

Error model (derived from the kernel, one line per term; the one of test_gpu_kernel_edges.py::test_gemm_grouped_with_sentinel_gaps):
  * dW: an f32 MFMA sum of K exact products (bf16 x bf16 fits f32), stored once -> ulps = 1, k = K + 1, cond = |dY|^T |X|;
    accumulating adds one f32 addition to the 3.0 already there -> k + 1, cond + 3.
  * db: the ones-operand MFMA sum of K values, then the ordered f32 sum of the bg_parts partial sums of the tile row (bg_parts =
    tile columns, or 1 under +16) and the store / accumulate -> k = K + bg_parts + 1, cond = sum |dY| (+ 5 when accumulating).
  * K <= 600 everywhere: the bound is about K 2^-24 cond and one missing product about cond / K, so a dropped product exceeds the
    bound more than forty-fold (at the benchmark's K = 25 216 it would not: tests/test_gpu_gemm.py keeps the large K).
  * where the code documents bit-exactness (ring depth and DMA placement change no arithmetic order; +32 renumbers tiles only; a
    second launch finds the arrival counters back at zero) the comparison is `torch.equal`.

The kernel is gemm_grouped_tn_kernel<C, D, BG, PLACE, STRIDED>: ring variants 0 .. 4 (`grouped_variant & 15`) x BG (any problem
of the launch has a bias gradient) x STRIDED (any problem of the launch is row-periodic) = 20 instantiations.  Tests that launch
(variant v, BG, STRIDED), v = 0 .. 4:
  (v, BG = 0, STRIDED = 0)  test_every_instantiation[v{v}-no_bias-dense]
  (v, BG = 1, STRIDED = 0)  test_every_instantiation[v{v}-some_bias-dense], test_k_steps_against_the_ring[v{v}-*];
                            v = 0, 3: test_host_flags_change_no_dw_bit[v{v}-*]; v = 0: test_tile_edges[*],
                            test_bias_gradient_sharing[*], test_the_24_problem_cut[*]; v = 0, 1: test_strided_offset_operands[v{v}-dense]
  (v, BG = 0, STRIDED = 1)  test_every_instantiation[v{v}-no_bias-periodic]
  (v, BG = 1, STRIDED = 1)  test_every_instantiation[v{v}-some_bias-periodic]; v = 0, 1: test_strided_offset_operands[v{v}-periodic]
(every non-zero variant is also compared bit for bit with variant 0 on the same table).  The refusals of the C entry are
called through the ctypes handle with a hand-built cfhip_gemm_problem table: a refused table launches nothing, wherever in it
the invalid problem sits."""
import ctypes
import re

import pytest
import torch

from helpers import _gemm_ref, assert_elementwise, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
DW_FILL, DB_FILL = 3.0, 5.0
VARIANTS = [0, 1, 2, 3, 4]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


@pytest.fixture
def variant():
    """sets the process-wide `grouped_variant`; back to 0 whatever the test did"""
    yield lambda v: ops.set_option("grouped_variant", v)
    ops.set_option("grouped_variant", 0)


# ---------------------------------------------------------------------------------------------
# operands, references, outputs, the per-element check
# ---------------------------------------------------------------------------------------------

_OPS, _REF = {}, {}


def _randn(shape, seed):
    """bf16 of seeded fp64 randn, scaled 0.5 .. 1 (by the seed)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * (0.5 + 0.125 * (seed % 5))).to(BF16)


def _operands(m, n, k, seed, period=0):
    """dY [K, M] and X [K, N] (CPU bf16, built once per key); period > 0: dY is zero outside the rows that are multiples of
    it (as tests/test_gpu_grouped_rows.py builds them), X random in all rows"""
    key = (m, n, k, seed, period)
    if key not in _OPS:
        a, b = _randn((k, m), seed), _randn((k, n), seed + 7919)
        if period:
            keep = torch.zeros(k, 1, dtype=torch.bool)
            keep[::period] = True
            a = torch.where(keep, a, torch.zeros_like(a))
        _OPS[key] = (a, b)
    return _OPS[key]


def _want(key, a, b):
    """(dW, |dY|^T |X|, db, sum |dY|) in float64, once per operand pair"""
    if key not in _REF:
        w, c = _gemm_ref(a, b, True, True)
        a64 = a.double()
        _REF[key] = (w, c, a64.sum(0), a64.abs().sum(0))
    return _REF[key]


def _dw(G, m, n, acc, pad=8):
    return G.out2d(m, n, n + pad, F32, DEV, fill=DW_FILL if acc else NAN)


def _db(G, m, acc):
    return G.out2d(1, m, m, F32, DEV, fill=DB_FILL if acc else NAN).view(m)


def _parts(n, flags=0):
    """workgroups of a tile row that share the bias-gradient reduction"""
    return 1 if flags & 16 else (n + 255) // 256


def _check(tag, ref, k, out, acc, bg=None, bg_acc=False, parts=1):
    w, c, bw, bc = ref
    assert_elementwise(out, w + (DW_FILL if acc else 0.0), out_dtype=F32, ulps=1, cond=c + (DW_FILL if acc else 0.0),
                       k=k + 1 + (1 if acc else 0), what=f"{tag} dW")
    if bg is not None:
        assert_elementwise(bg, bw + (DB_FILL if bg_acc else 0.0), out_dtype=F32, ulps=1, cond=bc + (DB_FILL if bg_acc else 0.0),
                           k=k + parts + 1, what=f"{tag} db")


# ---------------------------------------------------------------------------------------------
# 1. every instantiation: variant x bias gradient x walk on one table of six problems
# ---------------------------------------------------------------------------------------------

# (M, N, K, period of the periodic walk, dW +=, bias gradient in the "some" case, db +=).  (264, 520): a ragged second tile row and
# three tile columns; (768, 256): tiles_m > tiles_n; (256, 776): tiles_m < tiles_n, four workgroups share db; K is no multiple of
# 32 anywhere; the periodic problems (K = 3 x 197 and 7 x 33) sit in the middle: the host's "periodic first" order moves both.
TABLE = [
    (264, 520, 333, 0, False, True, True),
    (768, 256, 591, 197, True, True, False),
    (256, 776, 231, 33, False, True, True),
    (8, 8, 40, 0, True, False, False),
    (248, 264, 600, 0, True, True, False),
    (512, 512, 77, 0, False, False, False),
]


def _run_table(G, bias, periodic, check_tag=None, flags=0):
    """launch TABLE -> [(dW, db or None)] on the device; `check_tag`: also every problem per element and the unused db sentinels"""
    probs, unused = [], []
    for i, (m, n, k, period, acc, has_b, bg_acc) in enumerate(TABLE):
        a, b = _operands(m, n, k, 10 + i, period if periodic else 0)
        bg = _db(G, m, bg_acc)
        if not (bias and has_b):
            unused.append((i, bg, bg.clone()))
            bg = None
        probs.append((G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV)), _dw(G, m, n, acc), acc, bg, bg_acc) + ((period,) if periodic and period else ()))
    if periodic:
        assert [len(p) for p in probs] == [6, 7, 7, 6, 6, 6]
    ops.gemm_grouped_tn(probs)
    torch.cuda.synchronize()
    if check_tag is not None:
        for i, (p, (m, n, k, period, acc, _, bg_acc)) in enumerate(zip(probs, TABLE)):
            ref = _want(("table", i, periodic), *_operands(m, n, k, 10 + i, period if periodic else 0))
            _check(f"{check_tag} problem {i} ({m}x{n}x{k})", ref, k, p[2], acc, p[4], bg_acc, _parts(n, flags))
        for i, bg, before in unused:  # a problem without a bias gradient: the buffer it was not given keeps every bit
            assert _same_bits(bg, before), f"{check_tag} problem {i}: a db buffer the launch was not given changed"
    return [(p[2], p[4]) for p in probs]


def _same_bits(x, y):
    """torch.equal on the bit patterns (NaN-filled buffers compare too)"""
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _first_difference(x, y):
    d = torch.nonzero(x.view(torch.int32) != y.view(torch.int32))
    i = tuple(d[0].tolist())
    return f"{d.shape[0]} elements differ, first at {i}: {x[i].item()!r} vs {y[i].item()!r}"


@pytest.mark.parametrize("walk", ["dense", "periodic"])
@pytest.mark.parametrize("bias", ["no_bias", "some_bias"])
@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: f"v{v}")
def test_every_instantiation(G, variant, v, bias, walk):
    """per element for every problem, and bit for bit the same table at variant 0: ring depth and DMA placement change no
    arithmetic order"""
    variant(v)
    got = _run_table(G, bias == "some_bias", walk == "periodic", check_tag=f"variant {v} {bias} {walk}")
    variant(0)
    base = _run_table(G, bias == "some_bias", walk == "periodic")
    for i, ((out, bg), (out0, bg0)) in enumerate(zip(got, base)):
        assert _same_bits(out, out0), f"variant {v} vs 0, problem {i} dW: {_first_difference(out, out0)}"
        assert (bg is None) == (bg0 is None)
        if bg is not None:
            assert _same_bits(bg, bg0), f"variant {v} vs 0, problem {i} db: {_first_difference(bg, bg0)}"
    G.check()


@pytest.mark.parametrize("flags", [16, 32, 48], ids=lambda f: f"plus{f}")
@pytest.mark.parametrize("v", [0, 3], ids=lambda v: f"v{v}")
def test_host_flags_change_no_dw_bit(G, variant, v, flags):
    """+16 (the first tile column alone reduces db) and +32 (row-major tile order) on the dense table with bias gradients: dW
    bit-equal to the plain variant; db bit-equal under +32, within the model (bg_parts = 1) where the sharing differs"""
    variant(v + flags)
    got = _run_table(G, True, False, check_tag=f"variant {v} + {flags}", flags=flags)
    variant(v)
    plain = _run_table(G, True, False)
    for i, ((out, bg), (out0, bg0)) in enumerate(zip(got, plain)):
        assert _same_bits(out, out0), f"variant {v} + {flags}, problem {i} dW: {_first_difference(out, out0)}"
        if bg is not None and not flags & 16:
            assert _same_bits(bg, bg0), f"variant {v} + {flags}, problem {i} db: {_first_difference(bg, bg0)}"
    G.check()


# ---------------------------------------------------------------------------------------------
# 2. K against the ring: one to seven K-steps, the last one ragged, exact or one row over
# ---------------------------------------------------------------------------------------------

RING_K = [1, 8, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193]


@pytest.mark.parametrize("mn", [(8, 8), (264, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: f"v{v}")
def test_k_steps_against_the_ring(G, variant, v, mn):
    """K-steps below, at and above the prefetch distance (2 or 3) and the slot count (4 or 5): the prologue stages more than
    the reduction holds, the trailing zero-fill DMAs wrap.  The operands end at row K inside NaN: a step staged past K shows."""
    m, n = mn
    variant(v)
    for k in RING_K:
        a, b = _operands(m, n, k, 1000 + k)
        ref = _want(("ring", m, n, k), a, b)
        ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
        for acc in (False, True):
            out, bg = _dw(G, m, n, acc), _db(G, m, acc)
            ops.gemm_grouped_tn([(ad, bd, out, acc, bg, acc)])
            _check(f"variant {v} {m}x{n} K={k} acc={acc}", ref, k, out, acc, bg, acc, _parts(n))
        G.check()


# ---------------------------------------------------------------------------------------------
# 3. tile edges: M and N around one and two 256-wide tiles
# ---------------------------------------------------------------------------------------------

EDGE_SHAPES = [(8, 8), (248, 248), (256, 256), (264, 264), (504, 504), (512, 512), (520, 520),  # the diagonal
               (8, 520), (520, 8), (248, 264), (264, 248), (256, 512), (512, 256), (504, 520), (520, 504)]


@pytest.mark.parametrize("mn", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_edges(G, mn):
    m, n = mn
    k = 72
    a, b = _operands(m, n, k, 2000 + m + 3 * n)
    ref = _want(("edge", m, n), a, b)
    ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
    for acc in (False, True):
        out, bg = _dw(G, m, n, acc), _db(G, m, not acc)
        ops.gemm_grouped_tn([(ad, bd, out, acc, bg, not acc)])
        _check(f"{m}x{n}x{k} acc={acc}", ref, k, out, acc, bg, not acc, _parts(n))
    G.check()


# ---------------------------------------------------------------------------------------------
# 4. bias-gradient sharing: fewer, as many and more K-steps than tile columns
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("flags", [0, 16], ids=["shared", "plus16"])
@pytest.mark.parametrize("n", [256, 512, 776, 1000])
def test_bias_gradient_sharing(G, variant, n, flags):
    """1 .. 4 tile columns against 1 .. 5 K-steps: a workgroup that owns no bias K-step still posts a zero partial sum and takes
    its ticket.  Each case runs twice on the stream into fresh outputs: the counters returned to zero, the bits repeat."""
    m = 264
    variant(flags)
    for j, k in enumerate((32, 64, 96, 128, 160)):
        a, b = _operands(m, n, k, 3000 + n + k)
        ref = _want(("share", n, k), a, b)
        ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
        acc = bool(j & 1)
        runs = []
        for _ in range(2):
            out, bg = _dw(G, m, n, acc), _db(G, m, acc)
            ops.gemm_grouped_tn([(ad, bd, out, acc, bg, acc)])
            runs.append((out, bg))
        for r, (out, bg) in enumerate(runs):
            _check(f"N={n} K={k} flags={flags} run {r}", ref, k, out, acc, bg, acc, _parts(n, flags))
        assert _same_bits(runs[1][0], runs[0][0]), f"N={n} K={k} dW: {_first_difference(runs[1][0], runs[0][0])}"
        assert _same_bits(runs[1][1], runs[0][1]), f"N={n} K={k} db: {_first_difference(runs[1][1], runs[0][1])}"
        G.check()


# ---------------------------------------------------------------------------------------------
# 5. strided and offset operands, ldc = N + 4
# ---------------------------------------------------------------------------------------------

STRIDED_SPECS = [(264, 520, 394, 197, True), (8, 8, 99, 33, True), (256, 264, 75, 0, False)]  # (M, N, K, period, bias gradient)


def _slice_of_wider(G, t, left, right):
    """t [K, C] as the column slice [left : left + C] of a [K, left + C + right] device matrix that is NaN everywhere else"""
    k, c = t.shape
    wide = torch.full((k, left + c + right), NAN, dtype=BF16)
    wide[:, left:left + c] = t
    return G.poisoned(wide.to(DEV))[:, left:left + c]


@pytest.mark.parametrize("walk", ["dense", "periodic"])
@pytest.mark.parametrize("v", [0, 1], ids=lambda v: f"v{v}")
def test_strided_offset_operands(G, variant, v, walk):
    """dY and X are column slices (offsets of 8 and 16 elements, lda > M, ldb > N) of matrices that hold NaN outside the slice:
    a read past the tile's rows or past K reaches the output as NaN.  The dW blocks (ldc = N + 4) share one buffer with
    sentinel floats between them."""
    periodic = walk == "periodic"
    offs, end = [], 64
    for (m, n, *_) in STRIDED_SPECS:
        offs.append(end)
        end += m * (n + 4) + 64  # 64 sentinel floats between two blocks
    outs = G.region((end,), F32, DEV, lambda w: [w[o:o + m * (n + 4)].view(m, n + 4)[:, :n] for o, (m, n, *_) in zip(offs, STRIDED_SPECS)])
    probs = []
    for i, ((m, n, k, period, has_b), out) in enumerate(zip(STRIDED_SPECS, outs)):
        a, b = _operands(m, n, k, 4000 + i, period if periodic else 0)
        acc = bool(i & 1)
        out.fill_(DW_FILL if acc else NAN)
        assert out.stride(0) == n + 4 and out.data_ptr() % 16 == 0
        ad, bd = _slice_of_wider(G, a, 8, 16), _slice_of_wider(G, b, 16, 8)
        assert ad.stride(0) == m + 24 and bd.stride(0) == n + 24
        probs.append((ad, bd, out, acc, _db(G, m, not acc) if has_b else None, not acc) + ((period,) if periodic and period else ()))
    variant(v)
    ops.gemm_grouped_tn(probs)
    for i, (p, (m, n, k, period, _)) in enumerate(zip(probs, STRIDED_SPECS)):
        ref = _want(("strided", i, periodic), *_operands(m, n, k, 4000 + i, period if periodic else 0))
        _check(f"variant {v} {walk} problem {i} ({m}x{n}x{k})", ref, k, p[2], p[3], p[4], p[5], _parts(n))
    G.check()


# ---------------------------------------------------------------------------------------------
# 6. the 24-problem cut and the refusals of the C entry
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("count", [24, 25, 48, 49])
def test_the_24_problem_cut(G, count):
    """one, two, two and three launches; 49 distinct (M, N) and K: a problem routed to another's output fails on its values"""
    probs, meta = [], []
    for j in range(count):
        m, n, k = 8 * (1 + j % 7), 8 * (1 + j // 7), 40 + 3 * j
        a, b = _operands(m, n, k, 5000 + j)
        acc, has_b, bg_acc = bool(j & 1), j % 3 != 0, bool(j & 2)
        probs.append((G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV)), _dw(G, m, n, acc), acc, _db(G, m, bg_acc) if has_b else None, bg_acc))
        meta.append((("cut", j), a, b, k))
    assert len({(p[2].shape, m[3]) for p, m in zip(probs, meta)}) == count
    ops.gemm_grouped_tn(probs)
    for j, (p, (key, a, b, k)) in enumerate(zip(probs, meta)):
        _check(f"{count} problems, problem {j}", _want(key, a, b), k, p[2], p[3], p[4], p[5], 1)
    G.check()


# The refusal table: 32 valid problems (M = N = 16, K = 40, lda = ldb = ldc = 32) that accumulate into sentinel-filled outputs.
# Every operand lies inside a buffer wide enough for each altered descriptor below, should a launch ever take one.
R_COUNT, R_M, R_K, R_LD = 32, 16, 40, 32


def _refusal_table(G):
    a, b = _operands(R_LD, R_LD, R_K, 6000)
    ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
    rows = R_M + 2
    dws = G.region((R_COUNT * rows + 2, R_LD), F32, DEV, lambda w: [w[2 + i * rows:2 + i * rows + R_M, :R_M] for i in range(R_COUNT)])
    dbs = G.region((R_COUNT, R_LD), F32, DEV, lambda w: [w[i, :R_M] for i in range(R_COUNT)])
    arr = (_lib.GemmProblem * R_COUNT)()
    for i, (dw, db) in enumerate(zip(dws, dbs)):
        dw.fill_(DW_FILL)
        db.fill_(DB_FILL)
        pr = arr[i]
        pr.A, pr.B, pr.C, pr.bias_grad = ad.data_ptr(), bd.data_ptr(), dw.data_ptr(), db.data_ptr()
        pr.M, pr.N, pr.K, pr.k_period = R_M, R_M, R_K, 0
        pr.lda, pr.ldb, pr.ldc = R_LD, R_LD, R_LD
        pr.accumulate, pr.bias_grad_accumulate = 1, 1
    torch.cuda.synchronize()
    return arr, dws, dbs, (a[:, :R_M], b[:, :R_M])


def _call(arr, count):
    return _lib.load().cfhip_gemm_bf16_grouped_tn(ctypes.cast(arr, ctypes.c_void_p), count, ops._stream())


def _untouched(dws, dbs):
    torch.cuda.synchronize()
    for i, (dw, db) in enumerate(zip(dws, dbs)):
        assert bool((dw == DW_FILL).all()), f"dW of problem {i} was written"
        assert bool((db == DB_FILL).all()), f"db of problem {i} was written"


def _set(field, value):
    return lambda pr: setattr(pr, field, value(pr) if callable(value) else value)


REFUSALS = {
    "null_A": _set("A", None), "null_B": _set("B", None), "null_C": _set("C", None),
    "M_0": _set("M", 0), "N_0": _set("N", 0), "K_0": _set("K", 0),
    "M_12": _set("M", 12), "N_12": _set("N", 12),
    "lda_M_plus_4": _set("lda", R_M + 4), "ldb_N_plus_4": _set("ldb", R_M + 4), "ldc_N_plus_2": _set("ldc", R_M + 2),
    "A_plus_8_bytes": _set("A", lambda pr: pr.A + 8), "B_plus_8_bytes": _set("B", lambda pr: pr.B + 8),
    "C_plus_8_bytes": _set("C", lambda pr: pr.C + 8),
}


def test_the_refusal_table_itself_is_accepted(G):
    arr, dws, dbs, (a, b) = _refusal_table(G)
    assert _call(arr, R_COUNT) == 0, _lib.load().cfhip_last_error()
    ref = _want(("refusal",), a.contiguous(), b.contiguous())
    for i, (dw, db) in enumerate(zip(dws, dbs)):
        _check(f"problem {i}", ref, R_K, dw, True, db, True, 1)
    G.check()


def test_an_empty_table_is_refused(G):
    arr, dws, dbs, _ = _refusal_table(G)
    assert _call(arr, 0) == _lib.DEFINES["CFHIP_ERR_INVALID"]
    assert b"no problems" in _lib.load().cfhip_last_error()
    _untouched(dws, dbs)
    G.check()


@pytest.mark.parametrize("index", [0, 30])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_a_refused_table_launches_nothing(G, what, index):
    """the invalid problem first, or in the second launch of the table (index 30 of 32, behind 24 valid problems that would
    accumulate): CFHIP_ERR_INVALID, the message names the problem, and after a synchronize every output holds its sentinel"""
    arr, dws, dbs, _ = _refusal_table(G)
    REFUSALS[what](arr[index])
    rc = _call(arr, R_COUNT)
    msg = (_lib.load().cfhip_last_error() or b"").decode()
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"], (rc, msg)
    assert re.search(rf"problem {index}\b", msg), msg
    _untouched(dws, dbs)
    G.check()
