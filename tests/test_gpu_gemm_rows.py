"""cfhip_gemm_bf16_rows (`ops.gemm(..., config_rows=)`) and cfhip_head_rows_zero, per element: the head-token rows of a stack.

The last block of a stack read at its head token launches M = B rows that sit T rows apart in full-size [B T, .] tensors
(lda = T K, ldc = T ld: the output, aux_in and aux_out are strided views) under the tile configuration of the whole B T-row
launch.  The contract (gemm.hip, fused.py, head_tail.hip): every head row is bit-identical to the same row of the whole launch,
and no other row is written — with ldc = T ld a row mask that is off by one lands a whole sample away.

The harness of test_gpu_gemm_epilogues.py (`guarded_ops`, operands inside NaN, float64 references of the bf16-rounded operands,
`assert_elementwise` with that file's error models).  Each cell runs twice: the whole launch (M = B T, no config_rows) into
NaN-filled views, and the rows launch into the head rows of a second, sentinel-filled set of full-size tensors (`G.region`: only
the head rows may change, byte for byte; they start as NaN).  The rows launch reads its A and its aux_in from tensors whose other
rows are NaN.  Three assertions per cell: `torch.equal` with rows b T of the whole launch (output and aux_out), every head row
against float64, every other element of the full-size tensors still the sentinel's bit pattern.  And a fourth, because every tile
configuration computes the same bits (test_k_step_depth_control): both launches ran on the configuration of the whole problem,
read back from the library after the launch (cfhip_gemm_last_config).

Shapes per configuration: (B, T) = (1, 5), (3, 5), (5, 197), (BM + 1, 2) (head rows in a second tile row), N = BN + 4 (nt only),
BN + 8, 2 BN, K = 72 / 200 alternating; ld = N + 4 where N % 8 == 4, else N + 8.

Measured on an MI355X: 136 cells per configuration (96 nt, 40 nn), 2 312 in all, none failed; 184 tensor pairs per configuration
compared bit-equal (outputs, stored pre-activations, the GELU cells without aux_out against those with: 3 128 in all).  The
heuristic's own choices (15 / 3 / 1 / 0): 20 cases, 29 tensor pairs bit-equal.  K-step control: 0 of 1 792 elements differ."""
import pytest
import torch

from helpers import _gemm_ref, assert_elementwise, guarded_ops
from test_gpu_gemm import TILE_CONFIG_NAMES, _kernel_name
from test_gpu_gemm_epilogues import (BF16, BM, BN, DEV, EPI_OF, F32, LAYOUTS, _act, _act_grad, _fast_gate, _ldc, _randn, _view_of,
                                     accepted, expected_config, expected_name)

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402

SENTINEL = -7.25  # the pad of G.region: exact in bf16
GUARD_ROWS = 2
_INT = {BF16: torch.int16, F32: torch.int32}
CELLS_NT, CELLS_NN = 12 * 8, 8 * 5  # per configuration


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _stack(g, b, t, n, ld, dtype, pad=SENTINEL):
    """a full-size [b t, n] tensor (leading dimension ld) inside GUARD_ROWS rows of `pad` above and below, all `pad`, of which only
    the b head rows may change -> (the whole [b t + 2 GUARD_ROWS, ld] block, the head rows: [b, n], t ld apart, NaN)"""
    box = {}

    def views(w):
        box["whole"] = w
        return [w[GUARD_ROWS:GUARD_ROWS + b * t, :n][::t]]

    (heads,) = g.region((b * t + 2 * GUARD_ROWS, ld), dtype, DEV, views, pad=pad)
    assert heads.shape == (b, n) and heads.stride() == ((t * ld, 1) if b > 1 else heads.stride())
    heads.fill_(float("nan"))
    return box["whole"], heads


def _stack_in(g, full, t, ld):
    """the head rows of the CPU tensor `full` [b t, n] as a strided device view into a full-size tensor whose other rows are NaN"""
    m, n = full.shape
    _, heads = _stack(g, m // t, t, n, ld, full.dtype, pad=float("nan"))
    heads.copy_(full[::t].to(DEV))
    return heads


def _ran():
    """the tile configuration the latest ops.gemm of this thread was launched on, reroutes applied (-1: the generic kernel)"""
    return _lib.load().cfhip_gemm_last_config()


def _others_untouched(whole, heads_of):
    """every element of `whole` outside its head rows still holds the sentinel's bit pattern"""
    w = whole.clone()
    heads_of(w).fill_(SENTINEL)
    return bool((w.view(_INT[w.dtype]) == torch.tensor(SENTINEL, dtype=w.dtype).view(_INT[w.dtype]).item()).all())


class Stack:
    """b samples of t rows: A [b t, K] on the device inside NaN, a second copy whose rows other than b t are NaN (the operand of the
    rows launch), B, an f32 bias; the float64 product of the HEAD rows and its cond"""

    def __init__(self, g, layout, b, t, n, k):
        a_trans, b_trans = LAYOUTS[layout]
        assert not a_trans
        self.layout, self.b, self.t, self.n, self.k, self.b_trans = layout, b, t, n, k, b_trans
        m = b * t
        a = _randn((m, k), 3 * m + k, dtype=BF16)
        bm = _randn((k, n) if b_trans else (n, k), 5 * n + k, dtype=BF16)
        holes = torch.full_like(a, float("nan"))
        holes[::t] = a[::t]
        self.ad, self.ah, self.bd = g.poisoned(a.to(DEV)), g.poisoned(holes.to(DEV))[::t], g.poisoned(bm.to(DEV))
        assert self.ah.shape == (b, k) and (b == 1 or self.ah.stride(0) == t * k)
        self.want, self.cond = _gemm_ref(a[::t], bm, False, b_trans)
        self.bias = _randn(n, 7 * n + 1)
        self.biasd = g.poisoned(self.bias.to(DEV))
        self.saved = {}  # head rows of the GELU cells with aux_out, for the cells without

    def whole(self, out, **kw):
        """-> the configuration the launch ran on"""
        ops.gemm(self.ad, self.bd, b_trans=self.b_trans, out=out, **kw)
        return _ran()

    def rows(self, out, **kw):
        ts = [self.ah, self.bd, out] + [kw.get(name) for name in ("bias", "aux_in", "aux_out")]
        # (the MFMA path: the tile configurations are what this file is about)
        assert _fast_gate(self.b, self.n, self.k, self.t * self.k, self.bd.stride(0), out.stride(0), False, self.b_trans, *ts)
        ops.gemm(self.ah, self.bd, b_trans=self.b_trans, out=out, config_rows=self.b * self.t, **kw)
        return _ran()


def run_rows_cell(g, p, cell, tag):
    """the whole launch, the rows launch and the three checks of one cell -> the number of tensor pairs found bit-equal"""
    kind, dtype = cell["kind"], cell.get("dtype", BF16)
    b, t, n, k = p.b, p.t, p.n, p.k
    m = b * t
    ld = cell.get("ld") or _ldc(n)
    bias = p.biasd if cell.get("bias") else None
    want, cond, kb = p.want, p.cond, k
    if bias is not None:
        want, cond, kb = want + p.bias.double(), cond + p.bias.double().abs(), kb + 1
    full = g.out2d(m, n, ld, dtype, DEV)
    whole, heads = _stack(g, b, t, n, ld, dtype)
    pairs, stacks = [("output", heads, full)], [whole]
    kw_whole, kw_rows = {}, {}
    aux = None
    if kind in ("gelu", "qgelu") and cell["aux_out"]:
        pre_full = g.out2d(m, n, ld, BF16, DEV)
        pre_whole, pre_heads = _stack(g, b, t, n, ld, BF16)
        kw_whole["aux_out"], kw_rows["aux_out"] = pre_full, pre_heads
        pairs.append(("aux_out", pre_heads, pre_full))
        stacks.append(pre_whole)
    elif kind == "residual":
        aux = _randn((m, n), 11 * m + n, dtype=dtype)
    elif kind in ("dgelu", "dqgelu"):
        aux = _randn((m, n), 13 * m + n, 2.0).clamp(-6, 6).to(BF16)  # the saved pre-activation
    if aux is not None:
        kw_whole["aux_in"], kw_rows["aux_in"] = _view_of(g, aux, ld), _stack_in(g, aux, t, ld)
        aux = aux[::t].double()
    ran_whole = p.whole(full, bias=bias, epilogue=EPI_OF[kind], **kw_whole)
    ran_rows = p.rows(heads, bias=bias, epilogue=EPI_OF[kind], **kw_rows)
    if "aux_out" in kw_rows:
        p.saved[(kind, ld)] = heads.clone()
    assert ran_whole == ran_rows == cell["runs"], f"{tag}: the whole launch ran configuration {ran_whole}, the rows launch {ran_rows}"
    # 1. bit for bit the rows b t of the whole launch
    for name, h, f in pairs:
        assert torch.equal(h, f[::t]), f"{tag}: {name} differs from the whole launch in {int((h != f[::t]).sum())} of {h.numel()} elements"
    # 2. every head row per element (the error models of test_gpu_gemm_epilogues.run_cell)
    if kind == "none":
        # f32 sum of K exact products (+ bias), one rounding
        assert_elementwise(heads, want, out_dtype=dtype, cond=cond, k=kb, what=tag)
    elif kind in ("gelu", "qgelu"):
        if cell["aux_out"]:
            pre = kw_rows["aux_out"]
            # the stored pre-activation: f32 sum of K exact products + bias, one rounding
            assert_elementwise(pre, want, out_dtype=BF16, cond=cond, k=kb, what=f"{tag} pre-activation")
            p64 = pre.cpu().double()
            # the activation of the bf16 pre-activation: fast intrinsics (+ A&S erf), one rounding
            assert_elementwise(heads, _act(kind, p64), out_dtype=BF16, cond=p64.abs() * (1 + p64 * p64), k=8, what=tag)
        else:
            # the same arithmetic without the store of the pre-activation
            assert torch.equal(heads, p.saved[(kind, ld)]), f"{tag}: differs from the rows launch with aux_out"
    elif kind == "residual":
        # f32 sum of K exact products + bias + residual, one rounding
        assert_elementwise(heads, want + aux, out_dtype=dtype, cond=cond + aux.abs(), k=kb + 1, what=tag)
    elif kind in ("dgelu", "dqgelu"):
        gp = _act_grad(kind, aux)
        # (f32 sum of K exact products) x g'(pre) by fast intrinsics, one rounding: both terms in one cond, k = 1
        c = k * cond * gp.abs() + 8 * want.abs() * aux.abs() * (1 + aux * aux)
        assert_elementwise(heads, want * gp, out_dtype=BF16, cond=c, k=1, what=tag)
    else:
        raise AssertionError(kind)
    # 3. no other row, no padding column, no sentinel row was written
    for w in stacks:
        assert _others_untouched(w, lambda x: x[GUARD_ROWS:GUARD_ROWS + m, :n][::t]), f"{tag}: a row other than the head rows was written"
    return len(pairs) + (1 if kind in ("gelu", "qgelu") and not cell["aux_out"] else 0)


def stack_cells(cfg):
    """[(layout, B, T, N, K), cell] of one configuration, in running order (a GELU cell with aux_out before the one without)"""
    bm, bn = BM[cfg], BN[cfg]
    shapes = ((1, 5), (3, 5), (5, 197), (bm + 1, 2))
    cells = []
    for si, (b, t) in enumerate(shapes):
        for ni, n in enumerate((bn + 4, bn + 8, 2 * bn)):
            key = ("nt", b, t, n, (72, 200)[(si + ni) % 2])
            cells += [(key, dict(kind="none", bias=True, dtype=dt)) for dt in (BF16, F32)]
            for kind in ("gelu", "qgelu"):
                cells += [(key, dict(kind=kind, bias=True, aux_out=ao)) for ao in (True, False)]
            cells += [(key, dict(kind="residual", bias=True, dtype=dt)) for dt in (BF16, F32)]
    for si, (b, t) in enumerate(shapes):
        for ni, n in enumerate((bn + 8, 2 * bn)):
            key = ("nn", b, t, n, (72, 200)[(si + ni) % 2])
            cells += [(key, dict(kind="none", bias=bias)) for bias in (False, True)]
            cells += [(key, dict(kind="dgelu")), (key, dict(kind="dqgelu"))]
            # fused's `hv0`: the output is a tensor of this slice alone, [B T, N] dense, written from an operand K wide
            cells.append((key, dict(kind="none", ld=n)))
    return cells


def _tag(cfg, key, cell):
    extras = " ".join(f"{a}={v}" for a, v in cell.items() if a != "kind")
    return f"cfg{cfg} {key[0]} B={key[1]} T={key[2]} N={key[3]} K={key[4]} {cell['kind']} {extras}"


@pytest.mark.parametrize("cfg", list(range(17)))
def test_head_rows_of_every_config(G, cfg):
    cells = stack_cells(cfg)
    assert len(cells) == CELLS_NT + CELLS_NN  # nothing skipped silently
    ops.set_option("gemm_config", cfg)
    try:
        problem, ran, equal, failed = None, 0, 0, []
        for key, cell in cells:
            if problem is None or problem[0] != key:
                G.check()  # the buffers of the problem before this one
                problem = (key, Stack(G, *key))
            layout, b, t, n, k = key
            epi = EPI_OF[cell["kind"]]
            assert accepted(layout, epi)
            # the kernel is the one the configuration of the WHOLE launch names, reroutes included (1 -> 3 for RESIDUAL / GELU')
            assert _kernel_name(b * t, n, k, *LAYOUTS[layout], epi) == expected_name(cfg, layout, epi), _tag(cfg, key, cell)
            try:
                equal += run_rows_cell(G, problem[1], dict(cell, runs=expected_config(cfg, layout, epi)), _tag(cfg, key, cell))
            except AssertionError as e:  # every cell runs: the report names all the cells that are wrong, not the first
                failed.append(str(e))
            ran += 1
        print(f"cfg {cfg}: {ran} cells, {equal} tensor pairs bit-equal, {len(failed)} cells failed")
        assert ran == len(cells)
        assert not failed, f"{len(failed)} of {ran} cells:\n" + "\n".join(failed)
    finally:
        ops.set_option("gemm_config", -1)
    G.check()


def test_reroutes_under_config_rows_are_named():
    """what the table above relies on: 1 has no RESIDUAL / GELU' epilogue (-> 3); 8 has every row-major-A layout"""
    assert expected_config(1, "nt", ops.EPI_RESIDUAL) == 3 and expected_config(1, "nn", ops.EPI_DGELU) == 3
    assert expected_config(1, "nn", ops.EPI_DQGELU) == 3 and expected_config(1, "nt", ops.EPI_GELU) == 1
    assert all(expected_config(8, lay, epi) == 8 for lay, epis in (("nt", (0, 1, 2, 4)), ("nn", (0, 3, 5))) for epi in epis)


# ---------------------------------------------------------------------------------------------
# the heuristic's own choice (no forced gemm_config)
# ---------------------------------------------------------------------------------------------

# pick_config under the default heuristic (9), rows = config_rows, read from gemm.hip: from 512 rows on, 128x64x64 (3) while
# t14 = ceil(rows / 192) ceil(N / 128) < 160; else from 1 024 rows on the four-wave 192x128x64 (15); below 1 024 rows nn -> 1 and
# nt -> 3 (N <= 1 024) / 0.  N = 2 560 (20 tile columns): t14 reaches 160 at 8 tile rows = 1 345 rows, so 1 023 / 1 024 rows run 3
# on both sides; the 1 023 / 1 024 step itself is visible only where t14 >= 160 at 1 024 rows (6 tile rows): N = 3 584.  The
# 256-wide launches of the D = 256 stack have t14 = 16: configuration 3 at every row count from 512 on, nn included.
HEURISTIC = [
    # layout, N, T, config_rows, configuration
    ("nt", 2560, 197, 1379, 15), ("nn", 2560, 197, 1379, 15),  # B = 7, T = 197: FF1 forward / FF2 dX of the D = 256 stack
    ("nt", 2560, 192, 1344, 3), ("nt", 2560, 192, 1345, 15), ("nt", 2560, 193, 1351, 15),
    ("nn", 2560, 192, 1344, 3), ("nn", 2560, 192, 1345, 15), ("nn", 2560, 193, 1351, 15),
    ("nt", 2560, 146, 1023, 3), ("nt", 2560, 146, 1024, 3), ("nn", 2560, 146, 1023, 3), ("nn", 2560, 146, 1024, 3),
    ("nt", 3584, 146, 1023, 0), ("nt", 3584, 146, 1024, 15), ("nn", 3584, 146, 1023, 1), ("nn", 3584, 146, 1024, 15),
    ("nt", 256, 197, 1379, 3), ("nn", 256, 197, 1379, 3), ("nn", 256, 73, 511, 1), ("nn", 256, 73, 512, 3),
]


@pytest.mark.parametrize("layout,n,t,rows,cfg", HEURISTIC, ids=[f"{h[0]}_N{h[1]}_T{h[2]}_rows{h[3]}" for h in HEURISTIC])
def test_heuristic_choice_under_config_rows(G, layout, n, t, rows, cfg):
    """M = 7 head rows, T rows apart, out of `rows`: the forward form is FF1's (GELU, bias, stored pre-activation), the nn form
    FF2's dX (GELU' of a strided pre-activation); K = 136 (a tail against both K-step depths).  Configuration 1 has no GELU'
    epilogue (it would reroute to 3): where the heuristic answers 1 the kernel name is also asserted for the plain nn form."""
    b, k = 7, 136
    assert (b - 1) * t < rows
    b_trans = layout == "nn"
    epi = ops.EPI_DGELU if b_trans else ops.EPI_GELU
    assert _kernel_name(rows, n, k, False, b_trans, epi) == expected_name(cfg, layout, epi)
    assert _kernel_name(rows, n, k, False, b_trans, 0) == f"gemm_bf16_kernel<false, {str(b_trans).lower()}, 0, {TILE_CONFIG_NAMES[cfg]}>"
    a = _randn((rows, k), rows + n, dtype=BF16)
    bm = _randn((k, n) if b_trans else (n, k), 2 * rows + n, dtype=BF16)
    head_idx = torch.arange(b) * t
    holes = torch.full_like(a, float("nan"))
    holes[head_idx] = a[head_idx]
    ad, bd = G.poisoned(a.to(DEV)), G.poisoned(bm.to(DEV))
    ah = G.poisoned(holes.to(DEV))[:(b - 1) * t + 1:t]
    ld = n + 8

    def stack(dtype, pad=SENTINEL):  # `_stack` for rows that need not be a multiple of T
        box = {}

        def views(w):
            box["whole"] = w
            return [w[GUARD_ROWS:GUARD_ROWS + (b - 1) * t + 1:t, :n]]

        (h,) = G.region((rows + 2 * GUARD_ROWS, ld), dtype, DEV, views, pad=pad)
        h.fill_(float("nan"))
        return box["whole"], h

    full = G.out2d(rows, n, ld, BF16, DEV)
    whole, heads = stack(BF16)
    stacks, pairs = [whole], [(heads, full)]
    want, cond = _gemm_ref(a[head_idx], bm, False, b_trans)
    if b_trans:
        pre = _randn((rows, n), 3 * rows + n, 2.0).clamp(-6, 6).to(BF16)
        _, pre_heads = stack(BF16, pad=float("nan"))
        pre_heads.copy_(pre[head_idx].to(DEV))
        ops.gemm(ad, bd, b_trans=True, epilogue=epi, aux_in=_view_of(G, pre, ld), out=full)
        ran_whole = _ran()
        ops.gemm(ah, bd, b_trans=True, epilogue=epi, aux_in=pre_heads, out=heads, config_rows=rows)
        ran_rows = _ran()
        p64 = pre[head_idx].double()
        gp = _act_grad("dgelu", p64)
        # (f32 sum of K exact products) x g'(pre) by fast intrinsics, one rounding: both terms in one cond, k = 1
        assert_elementwise(heads, want * gp, out_dtype=BF16, cond=k * cond * gp.abs() + 8 * want.abs() * p64.abs() * (1 + p64 * p64), k=1,
                           what="GELU' head rows")
    else:
        bias = _randn(n, 7 * n + 1)
        biasd = G.poisoned(bias.to(DEV))
        pre_full = G.out2d(rows, n, ld, BF16, DEV)
        pre_whole, pre_heads = stack(BF16)
        stacks.append(pre_whole)
        pairs.append((pre_heads, pre_full))
        ops.gemm(ad, bd, bias=biasd, epilogue=epi, aux_out=pre_full, out=full)
        ran_whole = _ran()
        ops.gemm(ah, bd, bias=biasd, epilogue=epi, aux_out=pre_heads, out=heads, config_rows=rows)
        ran_rows = _ran()
        # the stored pre-activation: f32 sum of K exact products + bias, one rounding; its activation: fast intrinsics, one rounding
        assert_elementwise(pre_heads, want + bias.double(), out_dtype=BF16, cond=cond + bias.double().abs(), k=k + 1, what="pre-activation")
        p64 = pre_heads.cpu().double()
        assert_elementwise(heads, _act("gelu", p64), out_dtype=BF16, cond=p64.abs() * (1 + p64 * p64), k=8, what="GELU head rows")
    # the 7 rows ran on the configuration of the `rows`-row launch — not on the one pick_config gives 7 rows (nt: 3 / 0, nn: 1)
    assert ran_whole == ran_rows == expected_config(cfg, layout, epi), (ran_whole, ran_rows)
    for h, f in pairs:
        assert torch.equal(h, f[head_idx.to(DEV)]), f"{int((h != f[head_idx.to(DEV)]).sum())} of {h.numel()} elements differ from the whole launch"
    for w in stacks:
        assert _others_untouched(w, lambda x: x[GUARD_ROWS:GUARD_ROWS + (b - 1) * t + 1:t, :n])
    G.check()


def _heads_under(g, cfg, ah, bd, b, t, n):
    ops.set_option("gemm_config", cfg)
    try:
        _, heads = _stack(g, b, t, n, n + 8, F32)
        ops.gemm(ah, bd, out=heads, config_rows=b * t)
        assert _ran() == cfg
        return heads.clone()
    finally:
        ops.set_option("gemm_config", -1)


def test_k_step_depth_control(G):
    """Do the bit-equality assertions of this file have power against a launch under the WRONG configuration?  The same 7 head rows
    (FF2's shape of the D = 256 stack: N = 256, K = 2 560, f32 output) under configurations 1 and 0: the same 128x128 tile on the
    same wave grid, K-steps 32 and 64 deep.
    Measured on an MI355X: 0 of the 1 792 elements differ.  Every configuration feeds v_mfma_f32_16x16x32_bf16 the same 32-deep
    k-substeps in ascending order into one accumulator per element (compute_tile), so a 64-deep K-step is two 32-deep ones: the bits
    of an output element do not depend on the configuration, and the comparison with the whole launch canNOT see a `config_rows`
    that is ignored.  No assertion is made on the count (either outcome is within the contract); it is printed.  What pins the
    configuration instead is cfhip_gemm_last_config — the configuration the launch was made on — asserted after every whole and
    every rows launch of this file against the forced / heuristic configuration of the whole problem."""
    b, t, n, k = 7, 197, 256, 2560
    a = _randn((b * t, k), 1, dtype=BF16)
    bm = _randn((n, k), 2, dtype=BF16)
    ah, bd = G.poisoned(a.to(DEV))[::t], G.poisoned(bm.to(DEV))
    names = []
    for cfg in (1, 0):
        ops.set_option("gemm_config", cfg)
        names.append(_kernel_name(b * t, n, k, False, False, 0))
        ops.set_option("gemm_config", -1)
    assert names == [f"gemm_bf16_kernel<false, false, 0, {TILE_CONFIG_NAMES[c]}>" for c in (1, 0)]
    h32, h64 = _heads_under(G, 1, ah, bd, b, t, n), _heads_under(G, 0, ah, bd, b, t, n)
    want, cond = _gemm_ref(a[::t], bm, False, False)
    for h, what in ((h32, "K-step 32"), (h64, "K-step 64")):
        # f32 sum of K exact products, one rounding
        assert_elementwise(h, want, out_dtype=F32, cond=cond, k=k, what=what)
    differ = int((h32 != h64).sum())
    print(f"K-step control: {differ} of {h32.numel()} head-row elements differ between configurations 1 (K-step 32) and 0 (K-step 64)")
    G.check()


# ---------------------------------------------------------------------------------------------
# the generic kernel and the refusals
# ---------------------------------------------------------------------------------------------


def test_generic_kernel_under_config_rows(G):
    """a 10-class head (N = 10 fails the N % 4 gate) with config_rows set: the generic kernel, one thread per element of the M head
    rows; per element, bit-equal to the whole launch, the other rows untouched"""
    b, t, n, k, ld = 3, 5, 10, 64, 12
    p = Stack(G, "nt", b, t, n, k)
    want, cond = p.want + p.bias.double(), p.cond + p.bias.double().abs()
    for dt in (BF16, F32):
        full = G.out2d(b * t, n, ld, dt, DEV)
        whole, heads = _stack(G, b, t, n, ld, dt)
        assert not _fast_gate(b, n, k, t * k, k, t * ld, False, False, p.ah, p.bd, heads, p.biasd)
        p.whole(full, bias=p.biasd)
        ops.gemm(p.ah, p.bd, bias=p.biasd, out=heads, config_rows=b * t)
        assert _ran() == -1
        # f32 fmaf chain of depth K + the bias, one rounding
        assert_elementwise(heads, want, out_dtype=dt, cond=cond, k=k + 1, what=f"generic rows {dt}")
        assert torch.equal(heads, full[::t])
        assert _others_untouched(whole, lambda x: x[GUARD_ROWS:GUARD_ROWS + b * t, :n][::t])
    G.check()


ROWS_REFUSALS = [
    ("a_trans", dict(a_trans=True)), ("split_k", dict(split_k=2)), ("accumulate", dict(accumulate=True)), ("bias_grad", dict(bias_grad=True)),
    ("config_rows_below_m", dict(config_rows=2)),
]


@pytest.mark.parametrize("kw", [pytest.param(r[1], id=r[0]) for r in ROWS_REFUSALS])
def test_ops_gemm_refuses_what_the_rows_entry_does_not_take(G, kw):
    kw = dict(kw)
    b, t, n, k = 3, 5, 136, 72
    a_trans = kw.pop("a_trans", False)
    a = G.poisoned(_randn((k, b) if a_trans else (b * t, k), 1, dtype=BF16).to(DEV))
    bd = G.poisoned(_randn((k, n) if a_trans else (n, k), 2, dtype=BF16).to(DEV))
    whole, heads = _stack(G, b, t, n, n + 8, F32)
    heads.fill_(SENTINEL)
    if kw.get("bias_grad"):
        kw["bias_grad"] = G.out2d(1, b, b, F32, DEV, fill=SENTINEL).view(b)
    kw.setdefault("config_rows", b * t)
    with pytest.raises(ValueError, match="config_rows takes a_trans = False, no split_k / accumulate / bias_grad, and at least m rows"):
        ops.gemm(a if a_trans else a[::t], bd, a_trans=a_trans, b_trans=a_trans, out=heads, **kw)
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all()), "a refused request wrote to its output"
    if kw.get("bias_grad") is not None:
        assert bool((kw["bias_grad"] == SENTINEL).all())
    G.check()


def test_raw_entry_refuses_config_rows_below_m(G):
    """cfhip_gemm_bf16_rows itself: config_rows = M - 1 is an error and writes nothing; config_rows = M is a launch of its own rows"""
    b, t, n, k, ld = 3, 5, 136, 72, 144
    p = Stack(G, "nt", b, t, n, k)
    whole, heads = _stack(G, b, t, n, ld, BF16)
    heads.fill_(SENTINEL)
    lib = _lib.load()

    def call(config_rows):
        return lib.cfhip_gemm_bf16_rows(p.ah.data_ptr(), p.bd.data_ptr(), heads.data_ptr(), None, None, None, b, n, k, t * k, k, t * ld, 0, 0,
                                        0, config_rows, ops._stream())

    rc = call(b - 1)
    torch.cuda.synchronize()
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"] and b"config_rows" in lib.cfhip_last_error(), (rc, lib.cfhip_last_error())
    assert bool((whole == SENTINEL).all()), "a refused request wrote to its output"
    assert call(b) == 0
    # f32 sum of K exact products, one rounding
    assert_elementwise(heads, p.want, out_dtype=BF16, cond=p.cond, k=k, what="config_rows = M")
    assert _others_untouched(whole, lambda x: x[GUARD_ROWS:GUARD_ROWS + b * t, :n][::t])
    G.check()


# ---------------------------------------------------------------------------------------------
# cfhip_head_rows_zero
# ---------------------------------------------------------------------------------------------

ZERO_SHAPES = [  # rows, cols, row stride (elements)
    (1, 8, 8), (3, 8, 24), (65, 136, 136), (197, 768, 3072),
    (2731, 3072, 3072),  # 384 (bf16) / 768 (f32) chunks a row: more than the 4 096 x 256 threads of the capped grid, a second pass
]


def _zero_block(g, rows, cols, stride, dtype):
    box = {}

    def views(w):
        box["whole"] = w
        return [w[GUARD_ROWS:GUARD_ROWS + rows, :cols]]

    (x,) = g.region((rows + 2 * GUARD_ROWS, stride), dtype, DEV, views)
    return box["whole"], x


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols,stride", ZERO_SHAPES)
def test_head_rows_zero(G, rows, cols, stride, dtype):
    """the first `cols` columns of every row are +0.0 bit for bit; the other columns, the rows above and below and the byte guards
    keep what they held"""
    whole, x = _zero_block(G, rows, cols, stride, dtype)
    x.fill_(float("nan"))
    if rows == 2731:
        assert rows * (cols * x.element_size() // 16) > 4096 * 256
    ops.head_rows_zero(x, cols)
    torch.cuda.synchronize()
    bits = whole.view(_INT[dtype])
    assert int((bits[GUARD_ROWS:GUARD_ROWS + rows, :cols] != 0).sum()) == 0, "an element is not +0.0"
    assert _others_untouched(whole, lambda w: w[GUARD_ROWS:GUARD_ROWS + rows, :cols])
    G.check()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_head_rows_zero_refusals_leave_everything_untouched(G, dtype):
    rows, cols, stride = 5, 16, 24
    whole, x = _zero_block(G, rows, cols, stride, dtype)
    es = x.element_size()
    lib = _lib.load()
    ptr = x.data_ptr()
    assert ptr % 16 == 0 and (stride * es) % 16 == 0 and (cols * es) % 16 == 0
    part = 8 // es  # elements of half a chunk
    cases = [
        ("row bytes not a multiple of 16", (ptr, rows, cols - part, stride, es)),
        ("row stride not a multiple of 16 bytes", (ptr, rows, cols, stride + part, es)),
        ("base one element off a 16-byte boundary", (ptr + es, rows, cols, stride, es)),
        ("rows overlap", (ptr, rows, cols, cols - 16 // es, es)),
        ("rows = 0", (ptr, 0, cols, stride, es)), ("rows < 0", (ptr, -1, cols, stride, es)),
        ("cols = 0", (ptr, rows, 0, stride, es)), ("cols < 0", (ptr, rows, -16 // es, stride, es)),
        ("1-byte elements", (ptr, rows, 16, stride, 1)), ("8-byte elements", (ptr, rows, 2, 4, 8)), ("3-byte elements", (ptr, rows, 16, 32, 3)),
        ("null", (None, rows, cols, stride, es)),
    ]
    assert (ptr + es) % 16 == es  # 2 / 4 bytes off
    for what, args in cases:
        rc = lib.cfhip_head_rows_zero(*args, ops._stream())
        torch.cuda.synchronize()
        assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"] and b"head_rows_zero" in lib.cfhip_last_error(), (what, rc, lib.cfhip_last_error())
        assert bool((whole == SENTINEL).all()), f"{what}: a refused request wrote"
    with pytest.raises(ValueError, match="16-byte aligned rows"):
        ops.head_rows_zero(whole[GUARD_ROWS:GUARD_ROWS + rows, part:part + 8], 8)  # (ops.py refuses a misaligned view by itself)
    assert bool((whole == SENTINEL).all())
    assert lib.cfhip_head_rows_zero(ptr, rows, cols, stride, es, ops._stream()) == 0  # the same block, accepted
    torch.cuda.synchronize()
    assert int((whole.view(_INT[dtype])[GUARD_ROWS:GUARD_ROWS + rows, :cols] != 0).sum()) == 0
    assert _others_untouched(whole, lambda w: w[GUARD_ROWS:GUARD_ROWS + rows, :cols])
    G.check()
