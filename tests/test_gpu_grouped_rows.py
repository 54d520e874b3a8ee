"""Row-periodic problems of the grouped weight-gradient launch (`k_period` of cfhip_gemm_problem, fused.HEAD_ROW_DW).

A problem whose A operand (dY) is zero in every row r with r % period != 0 walks only the 32-row K-steps that hold a row
t * period.  The visited K-steps are the dense walk's own chunks and every skipped one would have added products with a zero
row of A, so C and the bias gradient must be BIT-equal to the dense launch of the same operands: that is asserted per case,
next to the fp64 bound tests/test_gpu_gemm.py uses for the grouped kernel (relative L2 2e-5 on the same bf16 operands).
Shapes: (264, 520) = a ragged second tile row and three tile columns (the bias-gradient reduction is shared three ways),
(768, 256) = three tile rows of one column, (8, 8) = one ragged tile; periods 32 (every chunk visited), 33, 50 (two head rows
can sit in neighbouring chunks; K = 150 is ragged) and 197 (the ViT's token count; most chunks skipped); 1, 3, 5 and 40 head
rows, K = heads * period (165, 150, 985 ... are no multiples of 32: the last chunk is ragged and the trailing DMAs must not
stage it twice)."""
import pytest
import torch

from helpers import assert_close, guarded_ops
from test_gpu_head_tail import EPS, NAMES, _make_params

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import fused, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(264, 520), (768, 256), (8, 8)]
PERIODS = [32, 33, 50, 197]
HEADS = [1, 3, 5, 40]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _operands(m, n, period, heads, seed):
    """A [K, M] bf16, zero outside rows that are multiples of `period`; B [K, N] random in all rows; K = heads * period"""
    k = heads * period
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(k, m)
    a[::period] = torch.randn(heads, m, generator=g)
    return a.to(BF16), torch.randn(k, n, generator=g).to(BF16)


def _outputs(g, m, n, acc):
    """guarded C (leading dimension n + 8) and bias gradient; 3.0 / 5.0 where the launch accumulates, NaN where it writes"""
    out = g.out2d(m, n, n + 8, F32, DEV, **(dict(fill=3.0) if acc else {}))
    bg = g.out2d(1, m, m, F32, DEV, **(dict(fill=5.0) if acc else {}))
    return out, bg.view(m)


_REF = {}


def _want(a, b, key):
    """fp64 product and column sums of the bf16 operands (computed once per operand pair)"""
    if key not in _REF:
        _REF[key] = (a.double().t() @ b.double(), a.double().sum(0))
    return _REF[key]


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("mn", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_periodic_walk_is_bit_equal_to_the_dense_launch(G, mn, period):
    m, n = mn
    for heads in HEADS:
        a, b = _operands(m, n, period, heads, 1000 * period + heads)
        ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
        w, bw = _want(a, b, (m, n, period, heads))
        for acc in (False, True):
            tag = f"M={m} N={n} period={period} heads={heads} K={heads * period} acc={acc}"
            dense, dense_bg = _outputs(G, m, n, acc)
            rows, rows_bg = _outputs(G, m, n, acc)
            ops.gemm_grouped_tn([(ad, bd, dense, acc, dense_bg, acc)])
            ops.gemm_grouped_tn([(ad, bd, rows, acc, rows_bg, acc, period)])
            assert torch.equal(rows, dense), tag
            assert torch.equal(rows_bg, dense_bg), tag
            assert_close(rows.cpu(), w + (3.0 if acc else 0.0), 2e-5, f"{tag} dW")
            assert_close(rows_bg.cpu(), bw + (5.0 if acc else 0.0), 2e-5, f"{tag} db")
        G.check()


def test_a_launch_mixes_dense_and_periodic_problems(G):
    """problem 0 dense (random in every row), problems 1 and 2 periodic with different periods, one of them without a bias gradient"""
    g = torch.Generator().manual_seed(77)
    dense_a, dense_b = torch.randn(333, 264, generator=g).to(BF16), torch.randn(333, 136, generator=g).to(BF16)
    a1, b1 = _operands(520, 264, 197, 5, 78)
    a2, b2 = _operands(72, 768, 50, 3, 79)
    ops_in = [(dense_a, dense_b, 0, True), (a1, b1, 197, True), (a2, b2, 50, False)]
    dev = [(G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))) for a, b, _, _ in ops_in]
    mixed, alone = [], []
    for (a, b, period, has_b), (ad, bd) in zip(ops_in, dev):
        for table, per in ((mixed, period), (alone, 0)):
            out, bg = _outputs(G, a.shape[1], b.shape[1], False)
            table.append((ad, bd, out, False, bg if has_b else None, False) + ((per,) if per else ()))
    assert [len(p) for p in mixed] == [6, 7, 7]
    ops.gemm_grouped_tn(mixed)
    for p in alone:
        ops.gemm_grouped_tn([p])
    for i, (pm, pa, (a, b, _, has_b)) in enumerate(zip(mixed, alone, ops_in)):
        assert torch.equal(pm[2], pa[2]), i
        assert_close(pm[2].cpu(), a.double().t() @ b.double(), 2e-5, f"problem {i} dW")
        if has_b:
            assert torch.equal(pm[4], pa[4]), i
            assert_close(pm[4].cpu(), a.double().sum(0), 2e-5, f"problem {i} db")


def test_more_periodic_problems_than_one_launch_takes(G):
    """26 problems: the 24-per-launch cut; both launches hold dense and periodic problems"""
    rows, dense = [], []
    for j in range(26):
        period = (0, 33, 64)[j % 3]
        m, n = 8 * (1 + j % 5), 8 * (2 + j % 4)
        if period:
            a, b = _operands(m, n, period, 3 + j % 2, 300 + j)
        else:
            g = torch.Generator().manual_seed(300 + j)
            a, b = torch.randn(70 + j, m, generator=g).to(BF16), torch.randn(70 + j, n, generator=g).to(BF16)
        ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
        acc = bool(j & 1)
        for table, per in ((rows, period), (dense, 0)):
            out, bg = _outputs(G, m, n, acc)
            table.append((ad, bd, out, acc, bg if j & 2 else None, acc) + ((per,) if per else ()))
    ops.gemm_grouped_tn(rows)
    ops.gemm_grouped_tn(dense)
    for j, (pr, pd) in enumerate(zip(rows, dense)):
        assert torch.equal(pr[2], pd[2]), j
        a, b = pr[0].cpu(), pr[1].cpu()
        assert_close(pr[2].cpu(), a.double().t() @ b.double() + (3.0 if pr[3] else 0.0), 2e-5, f"problem {j} dW")
        if pr[4] is not None:
            assert torch.equal(pr[4], pd[4]), j
            assert_close(pr[4].cpu(), a.double().sum(0) + (5.0 if pr[3] else 0.0), 2e-5, f"problem {j} db")


@pytest.mark.parametrize("period", [64, 197])
def test_skipped_chunks_are_not_read(G, period):
    """B is NaN in every row of every 32-row chunk that holds no multiple of the period (A is zero there): the periodic walk
    gives the result it gives on the clean B, all finite; the dense walk multiplies those NaNs by A's zeros"""
    m, n, heads = 264, 520, 5
    a, b = _operands(m, n, period, heads, 9)
    k = heads * period
    visited = torch.zeros((k + 31) // 32, dtype=torch.bool)
    visited[torch.arange(0, k, period) // 32] = True
    assert not visited.all()
    b_nan = b.clone()
    b_nan[~visited.repeat_interleave(32)[:k]] = float("nan")
    ad = G.poisoned(a.to(DEV))
    res = {}
    for name, bb, per in (("clean", b, period), ("rows", b_nan, period), ("dense", b_nan, 0)):
        out, bg = _outputs(G, m, n, False)
        ops.gemm_grouped_tn([(ad, G.poisoned(bb.to(DEV)), out, False, bg, False) + ((per,) if per else ())])
        res[name] = (out, bg)
    assert torch.isfinite(res["rows"][0]).all() and torch.isfinite(res["rows"][1]).all()
    assert torch.equal(res["rows"][0], res["clean"][0]) and torch.equal(res["rows"][1], res["clean"][1])
    assert torch.isnan(res["dense"][0]).any()
    assert_close(res["rows"][0].cpu(), a.double().t() @ b.double(), 2e-5, "dW")


@pytest.mark.parametrize("period", [1, 31])
def test_periods_below_a_k_step_are_refused(G, period):
    """0 < k_period < 32: the library's error, before anything is launched (the valid problem in front is not run either)"""
    a, b = _operands(8, 8, 32, 3, 5)
    ad, bd = G.poisoned(a.to(DEV)), G.poisoned(b.to(DEV))
    first, first_bg = _outputs(G, 8, 8, True)
    second, second_bg = _outputs(G, 8, 8, True)
    with pytest.raises(RuntimeError, match="k_period must be 0 .dense. or at least 32"):
        ops.gemm_grouped_tn([(ad, bd, first, False, first_bg, False), (ad, bd, second, False, second_bg, False, period)])
    torch.cuda.synchronize()
    for t, v in ((first, 3.0), (second, 3.0), (first_bg, 5.0), (second_bg, 5.0)):
        assert bool((t == v).all())
    with pytest.raises(ValueError, match="6 or 7 entries"):
        ops.gemm_grouped_tn([(ad, bd, first, False, first_bg, False, 32, 0)])


# ---------------------------------------------------------------------------------------------
# the step engine: fused.HEAD_ROW_DW
# ---------------------------------------------------------------------------------------------

ED, EHEADS, EFF = 256, 4, 512  # (256 wide: every LayerNorm backward runs the deterministic kernel, tests/test_gpu_head_tail.py)


def _spy(monkeypatch):
    """ops.gemm_grouped_tn that also records every problem table it is handed"""
    tables = []
    real = ops.gemm_grouped_tn
    monkeypatch.setattr(ops, "gemm_grouped_tn", lambda pr: (tables.append(list(pr)), real(pr))[1])
    return tables


def _stack_grads(x, blocks, wgt, words, row_dw, monkeypatch):
    monkeypatch.setattr(fused, "HEAD_ROW_DW", row_dw)
    x = x.clone().requires_grad_(True)
    ps = [[torch.nn.Parameter(p.to(DEV)) for p in blk] for blk in blocks]
    metas = tuple((EHEADS, EPS, EPS, False, 0, 0, words, True) for _ in blocks)
    y = fused.mixing_stack(x, metas, None, False, [p for blk in ps for p in blk])
    (y[:, 0].float() * wgt).sum().backward()
    torch.cuda.synchronize()
    return {f"{i}.{n}": p.grad for i, blk in enumerate(ps) for n, p in zip(NAMES, blk)}


@pytest.mark.parametrize("words", [2, 1], ids=["two_word_stream", "one_word_stream"])
@pytest.mark.parametrize("b", [3, 5])
@pytest.mark.parametrize("t", [33, 197])
def test_head_row_weight_gradients_equal_the_dense_tables(t, b, words, monkeypatch):
    """a 2-block head-token stack: all 24 parameter gradients bit-equal with HEAD_ROW_DW on and off, and the premise — the
    operands that carry a period are zero in every row the period skips — checked on the very tensors the launch was handed"""
    assert fused.HEAD_ONLY and fused.HEAD_ROW_DW
    monkeypatch.setattr(fused, "STACK_PLANS", False)
    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "DW_MIN_TILES", 0)  # (16 tiles: below the default the weight gradients would not be grouped at all)
    tables = _spy(monkeypatch)
    blocks = _make_params(7, ED, EFF)
    g = torch.Generator().manual_seed(100 * t + b)
    x = torch.randn(b, t, ED, generator=g).to(DEV)
    wgt = torch.randn(b, ED, generator=g).to(DEV)
    off = _stack_grads(x, blocks, wgt, words, False, monkeypatch)
    assert tables and all(len(p) == 6 for tb in tables for p in tb)
    assert sum(len(tb) for tb in tables) == 8
    del tables[:]
    on = _stack_grads(x, blocks, wgt, words, True, monkeypatch)
    probs = [p for tb in tables for p in tb]
    periodic = [p for p in probs if len(p) == 7]
    # the last block: w2, w1, out_w and the Q rows of in_w carry the period; its K / V rows and the first block stay dense
    assert len(probs) == 9 and sorted(tuple(p[2].shape) for p in periodic) == sorted([(ED, EFF), (EFF, ED), (ED, ED), (ED, ED)])
    assert all(p[6] == t for p in periodic)
    skipped = torch.ones(b * t, dtype=torch.bool, device=DEV)
    skipped[::t] = False
    for p in periodic:  # d2[0], dpre, dx1, dqkv[:, :d]
        assert p[0].shape[0] == b * t and not bool(p[0][skipped].any()), tuple(p[0].shape)
        assert bool(p[0][~skipped].any())
    assert len(on) == len(off) == 24
    for k in off:
        assert on[k] is not None and torch.equal(on[k], off[k]), k


def test_stacks_not_read_at_the_head_token_get_no_period(monkeypatch):
    """`apply_head=False` keeps the full last block: every row of its gradients is live and no problem may carry a period; the
    same encoder read through its head token does"""
    monkeypatch.setattr(fused, "STACK_PLANS", False)
    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "DW_MIN_TILES", 0)
    tables = _spy(monkeypatch)
    torch.manual_seed(3)
    enc = C.vit_b16_classifier(10, img_size=32, patch_size=4, latent_dim=ED, num_layers=2).to(DEV).encoder.encoder  # T = 65
    tokens = torch.randn(4, 65, ED, device=DEV)
    enc.forward_tokens(tokens, apply_head=False).float().square().mean().backward()
    torch.cuda.synchronize()
    assert tables and all(len(p) == 6 for tb in tables for p in tb)
    del tables[:]
    enc.forward_tokens(tokens).float().square().mean().backward()
    torch.cuda.synchronize()
    assert sum(len(p) == 7 and p[6] == 65 for tb in tables for p in tb) == 4
    del tables[:]
    monkeypatch.setattr(fused, "HEAD_ROW_DW", False)
    enc.forward_tokens(tokens).float().square().mean().backward()
    torch.cuda.synchronize()
    assert tables and all(len(p) == 6 for tb in tables for p in tb)


def test_head_row_weight_gradients_under_a_launch_plan(monkeypatch):
    """6 AdamW steps of a 2-layer ViT (T = 65, batch 8) through `TrainStep`: step 2 records the launch plan, step 3 is its first
    replay, later replays find the incoming gradient at another address and repoint the problem table (A / B / C only: the period
    stays).  Parameters after every step are bit-equal between HEAD_ROW_DW on and off."""
    from cflearn_amd.engine import TrainStep

    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "DW_MIN_TILES", 0)
    monkeypatch.setattr(fused, "STACK_PLANS", True)
    moved = []
    repoint = fused.StackPlan.repoint
    monkeypatch.setattr(fused.StackPlan, "repoint",
                        lambda self, sites, base: (moved.append(sum(type(s[2]) is tuple for s in sites)), repoint(self, sites, base))[1])

    def run(row_dw):
        monkeypatch.setattr(fused, "HEAD_ROW_DW", row_dw)
        fused._plans.clear()
        del moved[:]
        try:
            torch.manual_seed(3)
            m = C.vit_b16_classifier(10, img_size=32, patch_size=4, latent_dim=ED, num_layers=2).to(DEV)
            ts = TrainStep(m, lr=1e-3, weight_decay=0.01)
            gen = torch.Generator().manual_seed(5)
            batches = [(torch.randn(8, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (8,), generator=gen).to(DEV)) for _ in range(3)]
            out, junk = [], []
            for i in range(6):
                if i >= 3:  # take the cached block the incoming gradient lived in: the next one arrives at another address
                    junk.append(torch.empty(8, 65, ED, dtype=F32, device=DEV))
                ts.step(*batches[i % 3])
                torch.cuda.synchronize()
                out.append(ts.arena.flat_p.clone())
            plan = next(iter(fused._plans.values()))
            assert plan.ready_fwd and plan.ready_bwd and not plan.disabled
            periods = sorted(int(tb[i].k_period) for kind, tb, cnt in plan.bwd if kind == 3 for i in range(cnt))
            return out, periods, sum(moved)
        finally:
            fused._plans.clear()

    off, periods_off, _ = run(False)
    on, periods_on, table_rows_moved = run(True)
    assert periods_off == [0] * 8 and periods_on == [0] * 5 + [65] * 4, (periods_off, periods_on)
    assert table_rows_moved > 0  # a replay moved operands of the recorded problem table
    for i, (p0, p1) in enumerate(zip(off, on)):
        assert torch.equal(p0, p1), i
