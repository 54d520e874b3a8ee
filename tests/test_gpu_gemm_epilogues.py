"""cfhip_gemm_bf16: every epilogue path of every tile configuration, the generic kernel and the refusals, per element.

The harness of test_gpu_kernel_edges.py: `guarded_ops` (the split-K workspace ops.gemm allocates starts as NaN between byte
guards), operands read from NaN-surrounded buffers, every output / aux_in / aux_out a view with ldc > N whose padding
columns and guard rows hold a sentinel, a float64 reference on the same bf16-rounded operands, `assert_elementwise` (or
`torch.equal` where two launches must agree bit for bit), the guard check at the end.

Under a forced `gemm_config` the epilogue of that configuration runs with its own WCOLS / LPR / RPP / PPM / NIT and its own
aux prefetch ring: the shapes are 2 x 2 tiles with a ragged last tile both ways (M = BM + 1 / BM + 8, N = BN + 4 / BN + 8:
BN + 4 is the N % 8 != 0 form of the bf16 accesses, the nt layout only) and K = 72 / 200 (a tail against the 32- and the
64-deep K-step).  ldc = N + 4 where N % 8 == 4 and N + 8 otherwise; four more cells per configuration write bf16 rows with
ldc % 8 == 4 (N = BN + 8, ldc = N + 4: 16-byte accesses at 8-byte aligned rows).

Error models (one line at each call; the header of test_gpu_kernel_edges.py):
  * an f32 sum of K exact products: cond = |A| @ |B|, k = K; + 1 each for the bias, the residual and the accumulate read;
    a split-K sum adds the slice count;
  * GELU outputs against gelu64 / x sig64(1.702 x) of the pre-activation the kernel stored: k = 8, cond = |p| (1 + p^2);
  * GELU': want = (A @ B) g'(pre); the matrix term K |A| @ |B| |g'(pre)| and the fast intrinsics' 8 |A @ B| |pre| (1 + pre^2)
    folded into one cond with k = 1."""
import pytest
import torch

from helpers import (F32_EPS_HALF, _gelu64, _gelu_grad64, _gemm_ref, _sig64, assert_elementwise, guarded_ops, ulp_out)
from test_gpu_gemm import TILE_CONFIG_NAMES, _kernel_name

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# tile sizes of gemm_config 0 .. 16 (the table of test_gemm_out_view_every_config)
BM = (128, 128, 128, 128, 128, 128, 128, 256, 256, 256, 128, 256, 256, 256, 192, 192, 128)
BN = (128, 128, 128, 64, 128, 64, 64, 256, 128, 128, 256, 128, 256, 256, 128, 128, 256)
LAYOUTS = {"nt": (False, False), "nn": (False, True), "tn": (True, True)}  # layout -> (a_trans, b_trans)
EPI_OF = {"none": 0, "gelu": ops.EPI_GELU, "qgelu": ops.EPI_QGELU, "residual": ops.EPI_RESIDUAL, "dgelu": ops.EPI_DGELU,
          "dqgelu": ops.EPI_DQGELU}
SPLITS = ((296, 4), (72, 7))  # K = 296 in 4: slices of 128, 128 and 40 (the K tail); K = 72 in 7: clamped to its two K-steps
CELLS_NT_NN, CELLS_TN = 52 + 3 + 18 + 1, 12  # per configuration; the tn cells exist when M % 8 == 0 (M is a column count)


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def accepted(layout, epilogue):
    """what launch_layout provides: GELU / RESIDUAL (and quick GELU) forward, GELU' (and its quick form) on the input
    gradient layout, the weight-gradient layout without an epilogue"""
    return epilogue in {"nt": (0, 1, 2, 4), "nn": (0, 3, 5), "tn": (0,)}[layout]


def expected_config(cfg, layout, epilogue, bias_grad=False):
    """resolve_config (gemm.hip): the configuration that runs a request under the forced configuration `cfg`"""
    if cfg == 8 and layout == "tn":
        cfg = 1  # the 256x128x32 phase kernel has no weight-gradient layout
    if bias_grad and (7 <= cfg <= 13 or cfg == 16):
        cfg = 1  # the fused bias gradient exists on plain tiles up to 192x128
    if cfg == 1 and epilogue in (ops.EPI_RESIDUAL, ops.EPI_DGELU, ops.EPI_DQGELU):
        cfg = 3  # 128x128x32 on two stages has no RESIDUAL / GELU' epilogue
    return cfg


def expected_name(cfg, layout, epilogue):
    run = expected_config(cfg, layout, epilogue)
    a_trans, b_trans = LAYOUTS[layout]
    base = {ops.EPI_QGELU: ops.EPI_GELU, ops.EPI_DQGELU: ops.EPI_DGELU}.get(epilogue, epilogue)
    kernel = "gemm_bf16_phase_kernel" if 7 <= run <= 12 else "gemm_bf16_kernel"
    return f"{kernel}<{str(a_trans).lower()}, {str(b_trans).lower()}, {base}, {TILE_CONFIG_NAMES[run]}>"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=_gen(seed), dtype=torch.float64) * scale).to(dtype)


def _ldc(n):
    return n + 4 if n % 8 == 4 else n + 8


def _slices(k, split):
    """the K slices cfhip_gemm_bf16 makes of a request for `split`: whole 64-deep steps per slice, no empty slice"""
    steps = -(-k // 64)
    split = max(1, min(split, steps))
    per = -(-steps // split)
    return -(-steps // per)


def _act(kind, p64):
    return _gelu64(p64) if kind == "gelu" else p64 * _sig64(1.702 * p64)


def _act_grad(kind, p64):
    if kind == "dgelu":
        return _gelu_grad64(p64)
    s = _sig64(1.702 * p64)
    return s * (1 + 1.702 * p64 * (1 - s))


class Problem:
    """bf16 operands of one (layout, M, N, K) on the device inside NaN, their float64 product and its cond, an f32 bias"""

    def __init__(self, g, layout, m, n, k):
        a_trans, b_trans = LAYOUTS[layout]
        self.layout, self.m, self.n, self.k, self.a_trans, self.b_trans = layout, m, n, k, a_trans, b_trans
        a = _randn((k, m) if a_trans else (m, k), 3 * m + k, dtype=BF16)
        b = _randn((k, n) if b_trans else (n, k), 5 * n + k, dtype=BF16)
        self.a, self.ad, self.bd = a, g.poisoned(a.to(DEV)), g.poisoned(b.to(DEV))
        self.want, self.cond = _gemm_ref(a, b, a_trans, b_trans)
        self.bias = _randn(n, 7 * n + 1)
        self.biasd = g.poisoned(self.bias.to(DEV))
        self.saved = {}  # outputs of the GELU cells with aux_out, for the cells without

    def gemm(self, out, **kw):
        return ops.gemm(self.ad, self.bd, a_trans=self.a_trans, b_trans=self.b_trans, out=out, **kw)


def _view_of(g, t, ld):
    """a CPU [m, n] tensor as a device view with leading dimension ld inside sentinel columns and rows"""
    v = g.out2d(t.shape[0], t.shape[1], ld, t.dtype, DEV)
    v.copy_(t.to(DEV))
    return v


def run_cell(g, p, cell, tag):
    """one launch (two for the bias gradient's output pair) and its per-element checks -> nothing; raises on a mismatch"""
    kind, dtype = cell["kind"], cell.get("dtype", BF16)
    m, n, k = p.m, p.n, p.k
    ld = cell.get("ld") or _ldc(n)
    split = cell.get("split", 1)
    ns = _slices(k, split)
    extra = ns if ns > 1 else 0
    bias = p.biasd if cell.get("bias") else None
    want, cond, kb = p.want, p.cond, k
    if bias is not None:
        want, cond, kb = want + p.bias.double(), cond + p.bias.double().abs(), kb + 1
    if kind == "none":
        acc = cell.get("accumulate", False)
        out = g.out2d(m, n, ld, dtype, DEV, fill=2.0) if acc else g.out2d(m, n, ld, dtype, DEV)
        p.gemm(out, bias=bias, accumulate=acc, split_k=split)
        add = 2.0 if acc else 0.0
        # f32 sum of K exact products (+ bias) (+ the accumulate read) (+ one addition per K slice), one rounding
        assert_elementwise(out, want + add, out_dtype=dtype, cond=cond + add, k=kb + (1 if acc else 0) + extra, what=tag)
    elif kind in ("gelu", "qgelu"):
        out = g.out2d(m, n, ld, BF16, DEV)
        if cell["aux_out"]:
            pre = g.out2d(m, n, ld, BF16, DEV)
            p.gemm(out, bias=bias, epilogue=EPI_OF[kind], aux_out=pre)
            p.saved[(kind, ld)] = out.clone()
            # the stored pre-activation: f32 sum of K exact products + bias, one rounding
            assert_elementwise(pre, want, out_dtype=BF16, cond=cond, k=kb, what=f"{tag} pre-activation")
            p64 = pre.cpu().double()
            # the activation of the bf16 pre-activation: fast intrinsics (+ A&S erf), one rounding
            assert_elementwise(out, _act(kind, p64), out_dtype=BF16, cond=p64.abs() * (1 + p64 * p64), k=8, what=tag)
        else:
            p.gemm(out, bias=bias, epilogue=EPI_OF[kind])
            # the same arithmetic without the store of the pre-activation: bit for bit the output of the cell with aux_out
            assert torch.equal(out, p.saved[(kind, ld)]), f"{tag}: differs from the launch with aux_out"
    elif kind == "residual":
        res = _randn((m, n), 11 * m + n, dtype=dtype)
        out = g.out2d(m, n, ld, dtype, DEV)
        p.gemm(out, bias=bias, epilogue=ops.EPI_RESIDUAL, aux_in=_view_of(g, res, ld))
        # f32 sum of K exact products + bias + residual, one rounding
        assert_elementwise(out, want + res.double(), out_dtype=dtype, cond=cond + res.double().abs(), k=kb + 1, what=tag)
    elif kind in ("dgelu", "dqgelu"):
        pre = _randn((m, n), 13 * m + n, 2.0).clamp(-6, 6).to(BF16)  # the saved pre-activation
        out = g.out2d(m, n, ld, BF16, DEV)
        p.gemm(out, epilogue=EPI_OF[kind], aux_in=_view_of(g, pre, ld))
        p64 = pre.double()
        gp = _act_grad(kind, p64)
        # (f32 sum of K exact products) x g'(pre) by fast intrinsics, one rounding: both terms in one cond, k = 1
        c = k * cond * gp.abs() + 8 * want.abs() * p64.abs() * (1 + p64 * p64)
        assert_elementwise(out, want * gp, out_dtype=BF16, cond=c, k=1, what=tag)
    elif kind == "bgrad":
        acc = cell["accumulate"]
        out = g.out2d(m, n, ld, F32, DEV, fill=2.0) if acc else g.out2d(m, n, ld, F32, DEV)
        bg = g.out2d(1, m, m, F32, DEV, fill=-1.0) if acc else g.out2d(1, m, m, F32, DEV)
        p.gemm(out, accumulate=acc, split_k=split, bias_grad=bg.view(m), bias_grad_accumulate=acc)
        add, one = (2.0, 1) if acc else (0.0, 0)
        # dW: f32 sum of K exact products (+ the accumulate read) (+ one addition per K slice)
        assert_elementwise(out, want + add, out_dtype=F32, cond=cond + add, k=k + one + extra, what=f"{tag} dW")
        # db: f32 sum of the K bf16 values of a column of dY (+ the accumulate read) (+ one addition per K slice)
        a64 = p.a.double()
        assert_elementwise(bg.view(m), a64.sum(0) - one, out_dtype=F32, cond=a64.abs().sum(0) + one, k=k + one + extra, what=f"{tag} db")
    else:
        raise AssertionError(kind)


def config_cells(cfg):
    """[(layout, M, N, K), cell] of one configuration, in running order (a GELU cell with aux_out before the one without)"""
    bm, bn = BM[cfg], BN[cfg]
    cells = []
    # nt: every (M, N), K alternating
    for (m, n, k) in ((bm + 1, bn + 4, 72), (bm + 8, bn + 4, 200), (bm + 1, bn + 8, 200), (bm + 8, bn + 8, 72)):
        key = ("nt", m, n, k)
        cells += [(key, dict(kind="none", bias=True, dtype=dt)) for dt in (BF16, F32)]
        for kind in ("gelu", "qgelu"):
            cells += [(key, dict(kind=kind, bias=True, aux_out=ao)) for ao in (True, False)]
        cells += [(key, dict(kind="residual", bias=True, dtype=dt)) for dt in (BF16, F32)]
        cells.append((key, dict(kind="none", dtype=F32, accumulate=True)))
    for (k, split) in SPLITS:
        for (m, n) in ((bm + 1, bn + 4), (bm + 8, bn + 8)):
            cells += [(("nt", m, n, k), dict(kind="none", bias=bias, dtype=dt, split=split)) for bias in (False, True) for dt in (BF16, F32)]
    # bf16 rows at ldc % 8 == 4 with N % 8 == 0: 16-byte accesses of rows that are only 8-byte aligned
    key, ld4 = ("nt", bm + 1, bn + 8, 72), bn + 12
    cells += [(key, dict(kind="none", bias=True, dtype=BF16, ld=ld4)), (key, dict(kind="gelu", bias=True, aux_out=True, ld=ld4)),
              (key, dict(kind="residual", bias=True, dtype=BF16, ld=ld4))]
    # nn (N % 8 == 0)
    for (m, n, k) in ((bm + 1, bn + 8, 72), (bm + 8, bn + 8, 200)):
        key = ("nn", m, n, k)
        cells += [(key, dict(kind="none", bias=bias, dtype=dt)) for bias in (False, True) for dt in (BF16, F32)]
        cells += [(key, dict(kind="dgelu")), (key, dict(kind="dqgelu")), (key, dict(kind="none", dtype=F32, accumulate=True))]
    for (k, split), m in zip(SPLITS, (bm + 1, bm + 8)):
        cells += [(("nn", m, bn + 8, k), dict(kind="none", bias=bias, dtype=F32, split=split)) for bias in (False, True)]
    cells.append((("nn", bm + 1, bn + 8, 72), dict(kind="dgelu", ld=bn + 12)))
    # tn (M % 8 == 0: M is a column count of the operand)
    m, n = bm + 8, bn + 8
    if m % 8 == 0:
        for (k, split) in SPLITS:
            cells += [(("tn", m, n, k), dict(kind="none", bias=bias, dtype=F32, split=split)) for bias in (False, True)]
        for (k, split) in ((72, 1), (200, 1)) + SPLITS:
            cells += [(("tn", m, n, k), dict(kind="bgrad", accumulate=acc, split=split)) for acc in (False, True)]
    return cells


def _tag(cfg, key, cell):
    extras = " ".join(f"{a}={v}" for a, v in cell.items() if a != "kind")
    return f"cfg{cfg} {key[0]} {key[1]}x{key[2]}x{key[3]} {cell['kind']} {extras}"


@pytest.mark.parametrize("cfg", list(range(17)))
def test_every_epilogue_of_every_config(G, cfg):
    cells = config_cells(cfg)
    assert len(cells) == CELLS_NT_NN + (CELLS_TN if (BM[cfg] + 8) % 8 == 0 else 0)  # nothing skipped silently
    assert _slices(296, 4) == 3 and _slices(72, 7) == 2
    ops.set_option("gemm_config", cfg)
    try:
        problem, ran, failed = None, 0, []
        for key, cell in cells:
            if problem is None or problem[0] != key:
                G.check()  # the buffers of the problem before this one
                problem = (key, Problem(G, *key))
            layout, (m, n, k) = key[0], key[1:]
            epi = EPI_OF.get(cell["kind"], 0)
            assert accepted(layout, epi)
            if cell["kind"] != "bgrad":  # the kernel this cell runs is the one the configuration names, reroutes included
                assert _kernel_name(m, n, k, *LAYOUTS[layout], epi) == expected_name(cfg, layout, epi), _tag(cfg, key, cell)
            try:
                run_cell(G, problem[1], cell, _tag(cfg, key, cell))
            except AssertionError as e:  # every cell runs: the report names all the cells that are wrong, not the first
                failed.append(str(e))
            ran += 1
        assert ran == len(cells)
        assert not failed, f"{len(failed)} of {ran} cells:\n" + "\n".join(failed)
    finally:
        ops.set_option("gemm_config", -1)
    G.check()


def test_reroutes_are_named_as_reroutes():
    """configuration 1 has no RESIDUAL / GELU' epilogue (-> 3), configuration 8 no weight-gradient layout (-> 1)"""
    try:
        ops.set_option("gemm_config", 1)
        for layout, epi in (("nt", ops.EPI_RESIDUAL), ("nn", ops.EPI_DGELU), ("nn", ops.EPI_DQGELU)):
            name = _kernel_name(136, 136, 72, *LAYOUTS[layout], epi)
            assert TILE_CONFIG_NAMES[3] in name and TILE_CONFIG_NAMES[1] not in name, name
        for layout, epi in (("nt", ops.EPI_NONE), ("nt", ops.EPI_GELU), ("nt", ops.EPI_QGELU), ("nn", ops.EPI_NONE), ("tn", ops.EPI_NONE)):
            assert TILE_CONFIG_NAMES[1] in _kernel_name(136, 136, 72, *LAYOUTS[layout], epi)
        ops.set_option("gemm_config", 8)
        name = _kernel_name(136, 136, 72, True, True, 0)
        assert name == f"gemm_bf16_kernel<true, true, 0, {TILE_CONFIG_NAMES[1]}>"
        assert _kernel_name(136, 136, 72, False, True, 0) == f"gemm_bf16_phase_kernel<false, true, 0, {TILE_CONFIG_NAMES[8]}>"
    finally:
        ops.set_option("gemm_config", -1)


# ---------------------------------------------------------------------------------------------
# the generic kernel
# ---------------------------------------------------------------------------------------------


def _fast_gate(m, n, k, lda, ldb, ldc, a_trans, b_trans, *tensors):
    """the alignment gate of cfhip_gemm_bf16: True = the MFMA path takes the request"""
    k_ok = (a_trans and b_trans) or k % 8 == 0
    return bool(k_ok and lda % 8 == 0 and ldb % 8 == 0 and n % 4 == 0 and ldc % 4 == 0 and (not a_trans or m % 8 == 0)
                and (not b_trans or n % 8 == 0) and all(t is None or t.data_ptr() % 16 == 0 for t in tensors))


def _generic_gemm(p, out, **kw):
    """p.gemm for a request that must take the generic kernel"""
    ts = [p.ad, p.bd, out] + [kw.get(name) for name in ("bias", "aux_in", "aux_out")]
    assert not _fast_gate(p.m, p.n, p.k, p.ad.stride(0), p.bd.stride(0), out.stride(0), p.a_trans, p.b_trans, *ts)
    return p.gemm(out, **kw)


GENERIC = [
    # layout, M, N, K
    ("nt", 7, 3, 10), ("nn", 7, 3, 10), ("tn", 7, 3, 10),
    ("nt", 33, 5, 17), ("nn", 33, 5, 17), ("tn", 33, 5, 17),
    ("nt", 16, 10, 64),  # a 10-class head: forward,
    ("nn", 16, 64, 10),  # dX = dY W (K = 10 classes),
    ("tn", 10, 64, 16),  # dW = dY^T X (M = 10 classes) with the bias gradient
]


@pytest.mark.parametrize("layout,m,n,k", GENERIC)
def test_generic_kernel_every_epilogue(G, layout, m, n, k):
    """one thread per output element, an fmaf chain over k: bias, bf16 / f32 output and accumulate in every layout, and the
    epilogues of each layout (the rule of the MFMA path, `accepted`): GELU / quick GELU with and without aux_out and the
    bf16 / f32 residual forward, GELU' / quick GELU' on the input-gradient layout, the bias gradient on the weight-gradient one"""
    p = Problem(G, layout, m, n, k)
    ld = n + 3
    tag = f"generic {layout} {m}x{n}x{k}"
    want, cond = p.want, p.cond
    wb, cb = want + p.bias.double(), cond + p.bias.double().abs()
    for dt in (BF16, F32):
        out = G.out2d(m, n, ld, dt, DEV)
        _generic_gemm(p, out)
        # f32 fmaf chain of depth K, one rounding
        assert_elementwise(out, want, out_dtype=dt, cond=cond, k=k, what=f"{tag} {dt}")
        out = G.out2d(m, n, ld, dt, DEV)
        _generic_gemm(p, out, bias=p.biasd)
        # + the bias
        assert_elementwise(out, wb, out_dtype=dt, cond=cb, k=k + 1, what=f"{tag} bias {dt}")
        if not accepted(layout, ops.EPI_RESIDUAL):
            continue
        res = _randn((m, n), 17 * m + n, dtype=dt)
        out = G.out2d(m, n, ld, dt, DEV)
        _generic_gemm(p, out, bias=p.biasd, epilogue=ops.EPI_RESIDUAL, aux_in=_view_of(G, res, ld))
        # + the bias + the residual (bf16 or f32 with the output)
        assert_elementwise(out, wb + res.double(), out_dtype=dt, cond=cb + res.double().abs(), k=k + 2, what=f"{tag} residual {dt}")
    out = G.out2d(m, n, ld, F32, DEV, fill=2.0)
    _generic_gemm(p, out, accumulate=True)
    # + the accumulate read
    assert_elementwise(out, want + 2.0, out_dtype=F32, cond=cond + 2.0, k=k + 1, what=f"{tag} accumulate")
    for kind in ("gelu", "qgelu") if accepted(layout, ops.EPI_GELU) else ():
        out, pre = G.out2d(m, n, ld, BF16, DEV), G.out2d(m, n, ld, BF16, DEV)
        _generic_gemm(p, out, bias=p.biasd, epilogue=EPI_OF[kind], aux_out=pre)
        # the stored pre-activation: the chain + bias, one rounding; the activation of it: fast intrinsics, one rounding
        assert_elementwise(pre, wb, out_dtype=BF16, cond=cb, k=k + 1, what=f"{tag} {kind} pre-activation")
        p64 = pre.cpu().double()
        assert_elementwise(out, _act(kind, p64), out_dtype=BF16, cond=p64.abs() * (1 + p64 * p64), k=8, what=f"{tag} {kind}")
        out2 = G.out2d(m, n, ld, BF16, DEV)
        _generic_gemm(p, out2, bias=p.biasd, epilogue=EPI_OF[kind])
        assert torch.equal(out2, out), f"{tag} {kind}: differs from the launch with aux_out"
    for kind in ("dgelu", "dqgelu") if accepted(layout, ops.EPI_DGELU) else ():
        pre = _randn((m, n), 19 * m + n, 2.0).clamp(-6, 6).to(BF16)
        out = G.out2d(m, n, ld, BF16, DEV)
        _generic_gemm(p, out, epilogue=EPI_OF[kind], aux_in=_view_of(G, pre, ld))
        p64 = pre.double()
        gp = _act_grad(kind, p64)
        # (the chain) x g'(pre) by fast intrinsics, one rounding: both terms in one cond, k = 1
        c = k * cond * gp.abs() + 8 * want.abs() * p64.abs() * (1 + p64 * p64)
        assert_elementwise(out, want * gp, out_dtype=BF16, cond=c, k=1, what=f"{tag} {kind}")
    if layout == "tn":
        a64 = p.a.double()
        for acc in (False, True):
            out = G.out2d(m, n, ld, F32, DEV, fill=2.0) if acc else G.out2d(m, n, ld, F32, DEV)
            bg = G.out2d(1, m, m, F32, DEV, fill=-1.0) if acc else G.out2d(1, m, m, F32, DEV)
            _generic_gemm(p, out, accumulate=acc, bias_grad=bg.view(m), bias_grad_accumulate=acc)
            add, one = (2.0, 1) if acc else (0.0, 0)
            # dW: the chain (+ the accumulate read); db: an f32 chain over the K values of dY's column (+ the read)
            assert_elementwise(out, want + add, out_dtype=F32, cond=cond + add, k=k + one, what=f"{tag} dW acc={acc}")
            assert_elementwise(bg.view(m), a64.sum(0) - one, out_dtype=F32, cond=a64.abs().sum(0) + one, k=k + one, what=f"{tag} db acc={acc}")
    G.check()


def _shifted(g, t):
    """a contiguous device copy of `t` that starts one element into its (NaN-led) storage"""
    flat = torch.cat([torch.full((1,), float("nan"), dtype=t.dtype), t.flatten()])
    return g.poisoned(flat.to(DEV))[1:].view(t.shape)


def test_misaligned_operands_take_the_generic_kernel(G):
    """an aligned problem whose A starts 2 bytes, or whose bias starts 4 bytes, off a 16-byte boundary: the gate sends it to
    the generic kernel (right values, no NaN from in front of the view), never to 16-byte accesses"""
    m, n, k = 136, 72, 72
    p = Problem(G, "nt", m, n, k)
    ld = n + 8
    want, cond = p.want + p.bias.double(), p.cond + p.bias.double().abs()
    fast = G.out2d(m, n, ld, BF16, DEV)
    assert _fast_gate(m, n, k, k, k, ld, False, False, p.ad, p.bd, fast, p.biasd)
    p.gemm(fast, bias=p.biasd)
    # f32 sum of K exact products + bias, one rounding (every launch below)
    assert_elementwise(fast, want, out_dtype=BF16, cond=cond, k=k + 1, what="aligned")
    a_off, bias_off = _shifted(G, p.a), _shifted(G, p.bias)
    assert a_off.data_ptr() % 16 == 2 and a_off.is_contiguous() and bias_off.data_ptr() % 16 == 4
    bound = 2 * (ulp_out(want.abs(), BF16) + (k + 1) * F32_EPS_HALF * cond)  # the sum of the two launches' bounds
    for what, a, bias in (("A 2 bytes off", a_off, p.biasd), ("bias 4 bytes off", p.ad, bias_off)):
        out = G.out2d(m, n, ld, BF16, DEV)
        assert not _fast_gate(m, n, k, k, k, ld, False, False, a, p.bd, out, bias)
        ops.gemm(a, p.bd, bias=bias, out=out)
        assert_elementwise(out, want, out_dtype=BF16, cond=cond, k=k + 1, what=what)
        assert bool(((out.cpu().double() - fast.cpu().double()).abs() <= bound).all()), f"{what}: differs from the MFMA path's result"
    G.check()


# ---------------------------------------------------------------------------------------------
# refusals: real, correctly sized tensors; the library's message; nothing written
# ---------------------------------------------------------------------------------------------

SENTINEL = 1.25

REFUSALS = [
    # id, (a_trans, b_trans), gemm keywords (tensors by name), out dtype, the library's message
    ("layout_tn_only_a", (True, False), dict(), BF16, r"layout \(a_trans=1, b_trans=0\) is not provided"),
    ("accumulate_bf16", (False, False), dict(accumulate=True), BF16, "accumulate needs f32 output and epilogue NONE"),
    ("accumulate_epilogue", (False, False), dict(accumulate=True, epilogue="residual", aux_in=F32), F32, "accumulate needs f32 output and epilogue NONE"),
    ("gelu_f32", (False, False), dict(epilogue="gelu"), F32, "epilogues write bf16"),
    ("gelu_nn", (False, True), dict(epilogue="gelu"), BF16, r"epilogue 1 is not provided for layout \(0,1\)"),
    ("dgelu_nt", (False, False), dict(epilogue="dgelu", aux_in=BF16), BF16, r"epilogue 3 is not provided for layout \(0,0\)"),
    ("residual_tn", (True, True), dict(epilogue="residual", aux_in=BF16), BF16, r"epilogue 2 is not provided for layout \(1,1\)"),
    ("bias_grad_nt", (False, False), dict(bias_grad=True), F32, r"fused bias gradient exists for layout \(1,1\) only"),
    ("split_epilogue", (False, False), dict(split_k=2, epilogue="gelu"), BF16, "split_k supports epilogue NONE only"),
    ("split_generic", (False, False), dict(split_k=2, shape=(7, 3, 10)), F32, "split_k needs the aligned fast path"),
    ("residual_no_aux", (False, False), dict(epilogue="residual"), BF16, "epilogue 2 needs aux_in"),
]


@pytest.mark.parametrize("layout,kw,dtype,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_refusals_leave_the_output_untouched(G, layout, kw, dtype, message):
    kw = dict(kw)
    m, n, k = kw.pop("shape", (136, 72, 72))
    a_trans, b_trans = layout
    a = G.poisoned(_randn((k, m) if a_trans else (m, k), 1, dtype=BF16).to(DEV))
    b = G.poisoned(_randn((k, n) if b_trans else (n, k), 2, dtype=BF16).to(DEV))
    ld = n + 8
    out = G.out2d(m, n, ld, dtype, DEV, fill=SENTINEL)
    if "epilogue" in kw:
        kw["epilogue"] = EPI_OF[kw["epilogue"]]
    if "aux_in" in kw:
        kw["aux_in"] = G.out2d(m, n, ld, kw["aux_in"], DEV, fill=0.5)
    if kw.get("bias_grad"):
        kw["bias_grad"] = G.out2d(1, m, m, F32, DEV, fill=SENTINEL).view(m)
    with pytest.raises(RuntimeError, match=r"cfhip gemm failed \(code -?\d+\): .*" + message):
        ops.gemm(a, b, a_trans=a_trans, b_trans=b_trans, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused request wrote to its output"
    if kw.get("bias_grad") is not None:
        assert bool((kw["bias_grad"] == SENTINEL).all())
    G.check()


def test_workspace_one_float_short_is_refused(G):
    """the raw entry point: a buffer that is large enough, declared one float short of the three slices K = 296 / 4 makes"""
    m, n, k, split = 136, 72, 296, 4
    a = G.poisoned(_randn((m, k), 1, dtype=BF16).to(DEV))
    b = G.poisoned(_randn((n, k), 2, dtype=BF16).to(DEV))
    ld = n + 8
    out = G.out2d(m, n, ld, F32, DEV, fill=SENTINEL)
    ws = G.empty((split * m * n,), dtype=F32, device=DEV)
    need = _slices(k, split) * m * n * 4
    lib = _lib.load()

    def call(ws_bytes):
        return lib.cfhip_gemm_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), None, None, None, m, n, k, k, k, ld, 0, 0, 0, 1, 0,
                                   split, ws.data_ptr(), ws_bytes, None, 0, ops._stream())

    rc = call(need - 4)
    torch.cuda.synchronize()
    assert rc == _lib.DEFINES["CFHIP_ERR_WORKSPACE"] and b"workspace" in lib.cfhip_last_error(), (rc, lib.cfhip_last_error())
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(ws).all()), "a refused request wrote to its output or its workspace"
    assert call(need) == 0  # exactly enough is enough
    want, cond = _gemm_ref(a.cpu(), b.cpu(), False, False)
    # f32 sum of K exact products, one addition per K slice
    assert_elementwise(out, want, out_dtype=F32, cond=cond, k=k + 3, what="split-K with the exact workspace")
    G.check()
