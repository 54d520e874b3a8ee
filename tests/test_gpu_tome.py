"""Token merging on the HIP path (csrc/tome.hip, cflearn_amd/tome.py): the match kernel per row against float64 on the same bf16
inputs, the select kernel against the (value descending, position ascending) order on synthetic values, merge and unmerge_add per
element against float64 built from the kernel's own (validated) tables, a SpatialTransformerBlock with `tome_info` against the
reference's fp32 CPU run (tests/golden/tome_small.pt - tools/gen_tome_golden.py), and the structural / bit-exact behaviour of the
UNet, the ControlNet and the samplers with hooks set.

Error model of one score (u = 2^-24; exact arithmetic = float64 on the same bf16 inputs):
    score_ij = (dot_ij * rinv_i) * rinv_j,   dot_ij = sum_c a_ic b_jc,   rinv_t = 1 / sqrt(sum_c x_tc^2)
  * dot: the C products of bf16 values are exact in f32; their f32 accumulation (any order, C - 1 additions) is off by at most
    C u sum_c |a_ic b_jc|;
  * each sum of squares has C f32 roundings on non-negative terms: relative error <= C u; the square root halves it and adds one
    rounding, the division another: rinv is off by at most (C / 2 + 2) u of itself, twice (src and dst);
  * the two products: 2 u.
  With A_ij = (sum_c |a_ic b_jc|) rinv_i rinv_j >= |score_ij| (the absolute-value evaluation):
    tol_ij = (C + 2 (C / 2 + 2) + 2 + 2) u A_ij = (2 C + 8) u A_ij        (the last 2: room for the second-order terms).
A row is "in the band" when its best and second-best float64 scores lie within tol_best + tol_second of each other: an f32
evaluation may pick either.  Every row, in the band or not: score64[i, got_i] >= max_j score64[i, j] - tol_i,got - tol_i,best.
Outside the band the index must be the float64 arg-max (the lowest one).  The base cases have no row in the band (seeds chosen on
the CPU beforehand; asserted)."""
import functools
import os

import pytest
import torch

from helpers import assert_elementwise, guarded_ops, rel_l2

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops, tome  # noqa: E402

DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
YARDSTICK = 1.1


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _k(c):
    return 2 * c + 8


# ---------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------


def match_reference(x, src, dst, got_idx=None, chunk=2048):
    """float64 on x (f32 holding bf16 values) [B, N, C]: per src row the lowest arg-max, the max, its A (absolute-value evaluation),
    whether the row is in the band, and - given the kernel's indices - the slack of each row: score64[got] - (max - tol_got - tol_best)
    (>= 0 passes) and A at the kernel's index.  Rows go through in chunks: nothing of size n_src x n_dst x B stays."""
    b, n, c = x.shape
    x64 = x.double()
    sq = (x64 * x64).sum(-1)
    rinv = torch.where(sq > 0, sq.rsqrt(), torch.zeros_like(sq))
    src, dst = src.long(), dst.long()
    d64, rd = x64[:, dst], rinv[:, dst]
    out = dict(argmax=[], max=[], cond=[], band=[], slack=[], cond_got=[])
    for i0 in range(0, src.numel(), chunk):
        s = src[i0:i0 + chunk]
        a64, rs = x64[:, s], rinv[:, s]
        scale = rs[:, :, None] * rd[:, None, :]
        score = (a64 @ d64.transpose(1, 2)) * scale
        absev = (a64.abs() @ d64.abs().transpose(1, 2)) * scale
        tol = _k(c) * U * absev
        best = score.max(-1).values
        arg = (score == best[..., None]).to(torch.int8).argmax(-1)  # the lowest index of the maximum
        tol_best = tol.gather(-1, arg[..., None])[..., 0]
        if dst.numel() > 1:
            masked = score.scatter(-1, arg[..., None], float("-inf"))
            second = masked.max(-1)
            band = (best - second.values) <= tol_best + tol.gather(-1, second.indices[..., None])[..., 0]
        else:
            band = torch.zeros_like(best, dtype=torch.bool)
        out["argmax"].append(arg)
        out["max"].append(best)
        out["cond"].append(absev.gather(-1, arg[..., None])[..., 0])
        out["band"].append(band)
        if got_idx is not None:
            g = got_idx[:, i0:i0 + chunk].long()[..., None]
            out["slack"].append(score.gather(-1, g)[..., 0] - (best - tol.gather(-1, g)[..., 0] - tol_best))
            out["cond_got"].append(absev.gather(-1, g)[..., 0])
    return {k: torch.cat(v, 1) for k, v in out.items() if v}


def _tokens(b, n, c, seed):
    return torch.randn((b, n, c), generator=_gen(seed)).to(BF16).float()


# (B, h, w, C, seed): no row of theirs is in the band (seeds chosen on the CPU with match_reference; asserted).  Seeds 1, 2, 3 were
# the first tried; at 32x32 / C 320 (768 rows of 256 scores, tol ~ 4e-5) seeds 4 and 40 .. 50 left 1 - 4 rows in the band, 51 none.
BASE_CASES = [(2, 8, 8, 64, 1), (2, 16, 12, 64, 2), (2, 9, 7, 40, 3), (1, 32, 32, 320, 51)]
# C = 8 and C = 1280 (the narrowest and the widest rows: 1 and 40 k-steps) at 8x8; 9x7: n_src = 51, not a multiple of the 16-row
# wave tile nor of the 64-row workgroup; 3x3: one dst token; C = 328 / 648: the first widths of the 20- and 40-k-step kernels;
# 40x36 with C = 72: more dst rows (360) than one LDS tile of any kernel, C not a multiple of 32
MORE_CASES = [(2, 8, 8, 8, 5), (2, 8, 8, 1280, 6), (3, 9, 7, 24, 7), (2, 3, 3, 16, 8), (1, 8, 8, 328, 9), (1, 10, 8, 648, 10),
              (1, 40, 36, 72, 11)]


@functools.lru_cache(maxsize=None)
def _match_case(b, h, w, c, seed):
    x = _tokens(b, h * w, c, seed)
    src, dst = tome.split_tables(h, w, 2, 2, seed, True)
    return x, src, dst


def _run_match(G, x, src, dst):
    xd = G.poisoned(x.to(BF16).to(DEV))
    node_max, node_idx = ops.tome_match(xd, G.index(src.to(DEV)), G.index(dst.to(DEV)))
    assert node_max.dtype == F32 and node_idx.dtype == I32
    assert tuple(node_max.shape) == tuple(node_idx.shape) == (x.shape[0], src.numel())
    return node_max.cpu(), node_idx.cpu()


def _check_match(x, src, dst, node_max, node_idx, what, base=False):
    c = x.shape[-1]
    assert int(node_idx.min()) >= 0 and int(node_idx.max()) < dst.numel(), what
    ref = match_reference(x, src, dst, node_idx)
    nband = int(ref["band"].sum())
    print(f"{what}: {nband} of {ref['band'].numel()} rows in the band, least slack {float(ref['slack'].min()):.3e}")
    if base:
        assert nband == 0, f"{what}: {nband} rows of a base case are in the band"
    bad = torch.nonzero(ref["slack"] < 0)
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} rows beyond the float64 bound, first {bad[:5].tolist()}"
    wrong = torch.nonzero((node_idx.long() != ref["argmax"]) & ~ref["band"])
    assert wrong.numel() == 0, f"{what}: {wrong.shape[0]} rows outside the band differ from the float64 arg-max, first {wrong[:5].tolist()}"
    # the index is validated: node_max against the float64 score AT that index, with the error model's k and its A
    assert_elementwise(node_max, match_reference_value(x, src, dst, node_idx), out_dtype=F32, ulps=0.0, cond=ref["cond_got"], k=_k(c),
                       what=f"{what} node_max")


def match_reference_value(x, src, dst, idx):
    """float64 score of (row i, dst idx[b, i])"""
    x64 = x.double()
    sq = (x64 * x64).sum(-1)
    rinv = torch.where(sq > 0, sq.rsqrt(), torch.zeros_like(sq))
    a = x64[:, src.long()]
    d = torch.gather(x64[:, dst.long()], 1, idx.long()[..., None].expand(-1, -1, x.shape[-1]))
    bi = torch.arange(x.shape[0])[:, None]
    return (a * d).sum(-1) * rinv[:, src.long()] * rinv[bi, dst.long()[idx.long()]]


@pytest.mark.parametrize("case", BASE_CASES + MORE_CASES, ids=lambda c: f"B{c[0]}-{c[1]}x{c[2]}-C{c[3]}")
def test_match_random(G, case):
    x, src, dst = _match_case(*case)
    node_max, node_idx = _run_match(G, x, src, dst)
    _check_match(x, src, dst, node_max, node_idx, f"match {case}", base=case in BASE_CASES)


def test_match_128x128(G):
    """N = 16 384 with C = 8: 12 288 src rows against 4 096 dst rows, 192 workgroups a sample; the float64 reference in row chunks"""
    x, src, dst = _match_case(1, 128, 128, 8, 12)
    node_max, node_idx = _run_match(G, x, src, dst)
    _check_match(x, src, dst, node_max, node_idx, "match 128x128 C8")


def test_match_exact_ties_take_the_lowest_dst(G):
    """32x16 tokens: 128 dst rows, two LDS tiles of the C = 64 kernel.  dst 5, 70 and 100 hold the same vector v (another lane
    group, another 16-row tile, another LDS tile), dst 66 and 90 the same vector u: identical rows give bit-identical scores, so
    the src rows near v must report 5 and those near u 66"""
    h, w, c = 32, 16, 64
    src, dst = tome.split_tables(h, w, 2, 2, 21, True)
    g = _gen(21)
    x = torch.randn((2, h * w, c), generator=g)
    v, u = torch.randn((c,), generator=g), torch.randn((c,), generator=g)
    for j in (5, 70, 100):
        x[:, dst[j]] = v
    for j in (66, 90):
        x[:, dst[j]] = u
    half = src.numel() // 2
    x[:, src[:half].long()] = v + 0.05 * x[:, src[:half].long()]
    x[:, src[half:].long()] = u + 0.05 * x[:, src[half:].long()]
    x = x.to(BF16).float()
    node_max, node_idx = _run_match(G, x, src, dst)
    assert bool((node_idx[:, :half] == 5).all()) and bool((node_idx[:, half:] == 66).all())
    ref = match_reference(x, src, dst, node_idx)
    assert bool((ref["slack"] >= 0).all()) and bool((ref["argmax"] == node_idx).all())


def test_match_zero_rows_are_finite(G):
    """a zero row has inverse norm 0 here (the reference divides by zero): its scores are 0, finite; everything else is untouched"""
    x, src, dst = _match_case(2, 8, 8, 64, 1)
    x = x.clone()
    x[0, src[7]] = 0.0
    x[1, dst[3]] = 0.0
    node_max, node_idx = _run_match(G, x, src, dst)
    assert bool(torch.isfinite(node_max).all())
    assert float(node_max[0, 7]) == 0.0 and int(node_idx[0, 7]) == 0
    assert int(node_idx.min()) >= 0 and int(node_idx.max()) < dst.numel()
    ref = match_reference(x, src, dst, node_idx)
    assert bool((ref["slack"] >= 0).all())


def test_match_refuses_what_is_outside_the_kernels(G):
    src, dst = (t.to(DEV) for t in tome.split_tables(8, 8, 2, 2, 1, True))
    for c in (4, 12, 1288):
        with pytest.raises(NotImplementedError, match="C = "):
            ops.tome_match(torch.zeros((1, 64, c), dtype=BF16, device=DEV), src, dst)
    with pytest.raises(ValueError, match="do not split"):
        ops.tome_match(torch.zeros((1, 65, 8), dtype=BF16, device=DEV), src, dst)
    with pytest.raises(TypeError):
        ops.tome_match(torch.zeros((1, 64, 8), dtype=F32, device=DEV), src, dst)


# ---------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------


def select_reference(vals, idx, src, dst, r):
    """the four tables from the definition: the (value descending, position ascending) prefix of length r is merged; merged rows
    are [unmerged src, ascending token | dst, ascending token]; members of a dst ascending"""
    b, n_src = vals.shape
    n_dst, n = dst.numel(), n_src + dst.numel()
    n_unm = n_src - r
    row_of_token = torch.empty((b, n), dtype=I32)
    token_of_row = torch.empty((b, n - r), dtype=I32)
    member_off = torch.zeros((b, n_dst + 1), dtype=I32)
    members = torch.empty((b, r), dtype=I32)
    for s in range(b):
        order = torch.sort(-vals[s].double(), stable=True).indices
        taken = torch.zeros(n_src, dtype=torch.bool)
        taken[order[:r]] = True
        unm = torch.nonzero(~taken).view(-1)
        token_of_row[s, :n_unm] = src[unm]
        token_of_row[s, n_unm:] = dst
        row_of_token[s, src[unm].long()] = torch.arange(n_unm, dtype=I32)
        row_of_token[s, dst.long()] = n_unm + torch.arange(n_dst, dtype=I32)
        mpos = torch.nonzero(taken).view(-1)
        row_of_token[s, src[mpos].long()] = n_unm + idx[s, mpos]
        by_dst = torch.sort(idx[s, mpos].long(), stable=True).indices  # positions ascending inside each dst
        members[s] = src[mpos[by_dst]]
        member_off[s, 1:] = torch.cumsum(torch.bincount(idx[s, mpos].long(), minlength=n_dst), 0).to(I32)
    return row_of_token, token_of_row, member_off, members


def _select_values(kind, b, n_src, n_dst, seed):
    g = _gen(seed)
    if kind == "dup":  # nine distinct values, negative ones among them: whatever r is, duplicates sit on both sides of the threshold
        vals = torch.randint(-4, 5, (b, n_src), generator=g).float() / 4.0
        vals[vals == 0] = 0.125  # (the order of -0 and +0 is not part of the contract)
    else:
        vals = torch.rand((b, n_src), generator=g) * 2 - 1
    idx = torch.randint(0, n_dst, (b, n_src), generator=g).to(I32)
    if kind == "dup":  # a third of the rows go to dst 0 (long member lists, many per 1024-row chunk), dst 1 gets none
        idx[torch.rand((b, n_src), generator=g) < 0.33] = 0
        idx[idx == 1] = 2 if n_dst > 2 else 0
    return vals, idx


SELECT_SHAPES = {"48": (8, 8), "49152": (256, 256), "2250": (60, 50)}


@functools.lru_cache(maxsize=None)
def _select_case(shape, kind, r):
    h, w = SELECT_SHAPES[shape]
    src, dst = tome.split_tables(h, w, 2, 2, 5, True)
    n_src = src.numel()
    assert str(n_src) == shape
    r = {"one": 1, "all_but_one": n_src - 1, "all": n_src, "half": n_src // 2}[r]
    vals, idx = _select_values(kind, 2, n_src, dst.numel(), n_src + r)
    return src, dst, vals, idx, r, select_reference(vals, idx, src, dst, r)


def _run_select(G, vals, idx, src, dst, r):
    return ops.tome_select(G.poisoned(vals.to(DEV)), G.index(idx.to(DEV)), G.index(src.to(DEV)), G.index(dst.to(DEV)), r)


@pytest.mark.parametrize("r", ["one", "half", "all_but_one", "all"])
@pytest.mark.parametrize("kind", ["dup", "distinct"])
@pytest.mark.parametrize("shape", ["48", "2250", "49152"])
def test_select_is_the_ordered_prefix(G, shape, kind, r):
    """n_src = 48 (less than a wave-scan chunk), 2250 (three chunks, the last partial), 49 152 (N = 65 536: nothing held in
    LDS); r = 1, half, n_src - 1, n_src; values with duplicates across the threshold and distinct ones: the chosen set, the row
    order and the member lists equal the definition exactly (so the tables agree with each other), and a second run is bit-identical"""
    src, dst, vals, idx, r, want = _select_case(shape, kind, r)
    got = _run_select(G, vals, idx, src, dst, r)
    names = ("row_of_token", "token_of_row", "member_off", "members")
    for name, g, wnt in zip(names, got, want):
        assert g.dtype == I32 and tuple(g.shape) == tuple(wnt.shape), name
        assert torch.equal(g.cpu(), wnt), f"{name}: {int((g.cpu() != wnt).sum())} entries differ"
    again = _run_select(G, vals, idx, src, dst, r)
    for name, g, a in zip(names, got, again):
        assert torch.equal(g, a), f"{name}: two runs differ"
    # consistency, stated on its own: every row's token maps back to the row; a merged token's row is a dst row
    rot, tor, moff, mem = (t.cpu().long() for t in got)
    n_unm = src.numel() - r
    for s in range(rot.shape[0]):
        assert torch.equal(rot[s, tor[s]], torch.arange(tor.shape[1]))
        assert int(moff[s, -1]) == r and bool((rot[s, mem[s]] >= n_unm).all())


def test_select_refusals():
    src, dst = (t.to(DEV) for t in tome.split_tables(8, 8, 2, 2, 1, True))
    vals, idx = torch.zeros((1, 48), device=DEV), torch.zeros((1, 48), dtype=I32, device=DEV)
    for r in (0, 49):
        with pytest.raises(ValueError, match="r = "):
            ops.tome_select(vals, idx, src, dst, r)


# ---------------------------------------------------------------------------------------------
# merge / unmerge_add
# ---------------------------------------------------------------------------------------------

# (h, w, C, r kind): 9x7 C 40 (rows of 5 chunks), 8x8 C 64 with r = n_src (nothing stays unmerged), 16x12 C 520 (65 chunks: a lane
# takes two), 8x8 C 1280
MERGE_CASES = [(9, 7, 40, "half"), (8, 8, 64, "all"), (16, 12, 520, "half"), (8, 8, 1280, "half")]


def _tables(G, h, w, rkind, seed):
    """validated tables of a skewed assignment: dst 0 takes a third of the merged rows, dst 1 none, others 0 / 1 / a few"""
    src, dst = tome.split_tables(h, w, 2, 2, seed, True)
    n_src = src.numel()
    r = n_src if rkind == "all" else n_src // 2
    vals, idx = _select_values("dup", 2, n_src, dst.numel(), seed)
    got = _run_select(G, vals, idx, src, dst, r)
    want = select_reference(vals, idx, src, dst, r)
    for g, wnt in zip(got, want):
        assert torch.equal(g.cpu(), wnt)
    counts = (want[2][:, 1:] - want[2][:, :-1])
    assert int(counts.min()) == 0 and int((counts == 1).sum()) > 0 and int(counts.max()) >= 5
    return src, dst, r, got, want


@pytest.mark.parametrize("h,w,c,rkind", MERGE_CASES, ids=[f"{m[0]}x{m[1]}-C{m[2]}-{m[3]}" for m in MERGE_CASES])
def test_merge_and_unmerge_add(G, h, w, c, rkind):
    """merge per element against float64 (count f32 additions, one division, one bf16 rounding: 0.5 ulp of bf16 + (count + 1) u of
    the absolute-value mean), unmerged rows and member-free dst rows bit for bit; unmerge_add with a bf16, an f32 and no residual
    (one f32 add, one rounding: 0.5 ulp, + 1 u of |res| + |y| for the bf16 output's second rounding); unmerge(merge(x)) returns the
    tokens that were not merged bit for bit"""
    src, dst, r, got, want = _tables(G, h, w, rkind, 31 + c)
    rot, tor, moff, mem = got
    n = h * w
    n_unm = src.numel() - r
    x = _tokens(2, n, c, 77 + c)
    merged = ops.tome_merge(G.poisoned(x.to(BF16).to(DEV)), tor, moff, mem)
    assert merged.dtype == BF16 and tuple(merged.shape) == (2, n - r, c)
    m = merged.float().cpu()
    w_rot, w_tor, w_moff, w_mem = (t.long() for t in want)
    x64 = x.double()
    ref = torch.empty((2, n - r, c), dtype=torch.float64)
    cond = torch.zeros_like(ref)
    exact = torch.zeros((2, n - r), dtype=torch.bool)
    for s in range(2):
        ref[s, :n_unm] = x64[s, w_tor[s, :n_unm]]
        exact[s, :n_unm] = True
        for j in range(dst.numel()):
            mm = w_mem[s, w_moff[s, j]:w_moff[s, j + 1]]
            rows = torch.cat([x64[s, dst[j].long()][None], x64[s, mm]])
            ref[s, n_unm + j] = rows.sum(0) / rows.shape[0]
            cond[s, n_unm + j] = rows.abs().sum(0)  # (count additions + one division) x the absolute-value mean
            exact[s, n_unm + j] = mm.numel() == 0
    assert torch.equal(m[exact], ref[exact].float()), "an unmerged row or a dst row without members is not a copy"
    assert_elementwise(m, ref, out_dtype=BF16, ulps=0.5, cond=cond, k=1.0, what="merge")

    y = _tokens(2, n - r, c, 99 + c)
    yd = G.poisoned(y.to(BF16).to(DEV))
    y_tok = torch.stack([y[s, w_rot[s]] for s in range(2)])  # the plain unmerge
    res = torch.randn((2, n, c), generator=_gen(5 + c))
    out = ops.tome_unmerge_add(yd, rot)
    assert out.dtype == BF16 and torch.equal(out.float().cpu(), y_tok)
    out = ops.tome_unmerge_add(yd, rot, out_f32=True)
    assert out.dtype == F32 and torch.equal(out.cpu(), y_tok)
    out = ops.tome_unmerge_add(yd, rot, G.poisoned(res.to(DEV)))
    assert out.dtype == F32
    assert_elementwise(out, res.double() + y_tok.double(), out_dtype=F32, ulps=0.5, what="unmerge_add f32")
    res16 = res.to(BF16).float()
    out = ops.tome_unmerge_add(yd, rot, G.poisoned(res16.to(BF16).to(DEV)))
    assert out.dtype == BF16
    assert_elementwise(out, res16.double() + y_tok.double(), out_dtype=BF16, ulps=0.5, cond=res16.abs() + y_tok.abs(), k=1.0,
                       what="unmerge_add bf16")

    back = ops.tome_unmerge_add(merged, rot).float().cpu()
    for s in range(2):
        kept = torch.cat([w_tor[s, :n_unm], dst.long()[(w_moff[s, 1:] - w_moff[s, :-1]) == 0]])
        assert torch.equal(back[s, kept], x[s, kept]), "unmerge(merge(x)) changed a token that was not merged"
        taken = w_mem[s]
        assert torch.equal(back[s, taken], m[s, w_rot[s, taken]])  # a merged src token receives its dst's row


# ---------------------------------------------------------------------------------------------
# block against the reference
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "tome_small.pt"), map_location="cpu", weights_only=False)


def seeded_state(shapes, seed):
    """tools/gen_first_stage_golden.py::seeded_state, line for line: the parameters no fixture stores"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        n = torch.randn(shape, generator=g)
        if len(shape) == 1:
            out[name] = 1.0 + 0.1 * n if name.endswith("weight") else 0.1 * n
        else:
            out[name] = n / float(torch.Size(shape[1:]).numel()) ** 0.5
    return out


def _block(fx):
    m = C.SpatialTransformerBlock(**fx["block_cfg"])
    m.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, fx["block_seed"]), strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("key", [f"{s}-{f}" for s in ("8x8", "9x7") for f in ("attn", "all", "cross_mlp")])
def test_block_against_the_reference(fx, key):
    """first the HIP tables equal the recorded merge exactly (the fixture's inputs make the decision independent of precision: its
    asserted margins are >= 8 x the reference's own fp32 / bf16 score spread), then the output is held to the usual yardstick"""
    rec = fx["blocks"][key]
    h, w, r = rec["h"], rec["w"], rec["r"]
    block = _block(fx)
    x = rec["x"].to(DEV)
    info = tome.setup_tome_info(rec["tome_info"])
    info["size"] = (h, w)
    sizes = tome.merge_sizes(h * w, info)
    assert sizes == (h, w, r)
    tm = tome.TokenMerge(x, info, sizes)
    assert torch.equal(tm.src_idx.cpu(), rec["src"]) and torch.equal(tm.dst_idx.cpu(), rec["dst"])
    rot, moff, mem = tm.row_of_token.cpu().long(), tm.member_off.cpu().long(), tm.members.cpu().long()
    n_unm = rec["src"].numel() - r
    for s in range(x.shape[0]):
        pairs = sorted((int(t), int(rec["dst"][int(rot[s, t]) - n_unm])) for t in mem[s].tolist())
        assert pairs == [tuple(p) for p in rec["pairs"][s].tolist()], f"{key}: sample {s} merges other pairs than the reference"
    block.setup_hooks(tome_info=rec["tome_info"])
    block.tome_info["size"] = (h, w)
    with torch.no_grad():
        y = block(x, rec["context"].to(DEV))
    assert tuple(y.shape) == tuple(rec["y"].shape) and bool(torch.isfinite(y).all())
    ours, theirs = rel_l2(y, rec["y"]), rel_l2(rec["y_bf16"], rec["y"])
    print(f"block {key}: ours {ours:.3e}, reference bf16 {theirs:.3e}, ratio {ours / theirs:.2f}")
    assert ours <= YARDSTICK * theirs, f"block {key}: rel-L2 {ours:.3e} vs fp32 > {YARDSTICK} x the reference's bf16 {theirs:.3e}"


def test_block_gate_closed_or_nothing_to_merge_is_the_plain_block(fx):
    """ratio 0 (r = 0), a closed gate (the block sees a quarter of the tokens, max_downsample 1) and hooks switched off again: bit
    for bit the block without hooks; with grad wanted the block refuses"""
    rec = fx["blocks"]["8x8-all"]
    block = _block(fx)
    x, ctx = rec["x"].to(DEV).to(BF16), rec["context"].to(DEV)
    with torch.no_grad():
        plain = block(x, ctx)
        for info, size in ((dict(ratio=0.0, seed=1), (8, 8)), (dict(ratio=0.5, seed=1), (16, 16))):
            block.setup_hooks(tome_info=info)
            block.tome_info["size"] = size
            assert torch.equal(block(x, ctx), plain)
        block.setup_hooks(tome_info=dict(seed=1, merge_mlp=True))
        block.tome_info["size"] = (8, 8)
        merged = block(x, ctx)
        assert merged.dtype == plain.dtype and tuple(merged.shape) == tuple(plain.shape) and not torch.equal(merged, plain)
        assert torch.equal(block(x, ctx), merged)  # a fixed seed: the same split, the same result
    with pytest.raises(NotImplementedError, match="§8"):
        block(x, ctx)
    block.setup_hooks()
    with torch.no_grad():
        assert torch.equal(block(x, ctx), plain)


# ---------------------------------------------------------------------------------------------
# UNet, ControlNet, samplers: structural and bit-exact checks (no numeric comparison with the reference at this level: real
# activations have near-ties, a bf16 run and the fp32 reference legitimately merge different tokens)
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def small(golden):
    u = golden("unet_small.pt")
    m = C.build_module("unet_diffuser", config=dict(u["cfg"]))
    m.load_state_dict(u["sd"])
    return m.to(DEV).eval(), u


def _calls(monkeypatch):
    seen = []
    real = ops.tome_match

    def spy(x, src_idx, dst_idx):
        seen.append(tuple(x.shape))
        return real(x, src_idx, dst_idx)

    monkeypatch.setattr(ops, "tome_match", spy)
    return seen


def test_unet_with_hooks(small, monkeypatch):
    unet, u = small
    x, t, ctx = u["x"].to(DEV), u["timesteps"].to(DEV), u["context"].to(DEV)
    seen = _calls(monkeypatch)
    try:
        with torch.no_grad():
            plain = unet(x, timesteps=t, context=ctx)
            assert not seen
            unet.setup_hooks(tome_info=dict(ratio=0.0))
            assert torch.equal(unet(x, timesteps=t, context=ctx), plain) and not seen  # r = 0: the plain path, bit for bit
            unet.setup_hooks(tome_info=dict(seed=3))
            a = unet(x, timesteps=t, context=ctx)
            # 16x16 input: the blocks at downsample 1 see 256 tokens and merge, those at downsample 2 (64 tokens) stay plain
            assert seen and all(s[1] == 256 for s in seen)
            at_one = len(seen)
            b = unet(x, timesteps=t, context=ctx)
            assert torch.equal(a, b) and len(seen) == 2 * at_one  # a fixed seed: eager == eager
            assert a.dtype == plain.dtype and tuple(a.shape) == tuple(plain.shape) and bool(torch.isfinite(a).all())
            assert not torch.equal(a, plain)
            del seen[:]
            unet.setup_hooks(tome_info=dict(seed=3, max_downsample=2, merge_crossattn=True, merge_mlp=True))
            c = unet(x, timesteps=t, context=ctx)
            assert {s[1] for s in seen} == {256, 64} and len(seen) > at_one and bool(torch.isfinite(c).all())
            del seen[:]
            unet.setup_hooks(tome_info=dict(use_rand=True))  # no seed: a fresh split per block forward, still finite
            d = unet(x, timesteps=t, context=ctx)
            assert len(seen) == at_one and bool(torch.isfinite(d).all())
            unet.setup_hooks()
            del seen[:]
            assert torch.equal(unet(x, timesteps=t, context=ctx), plain) and not seen
        with pytest.raises(TypeError):
            unet.setup_hooks(tome=dict())
        with pytest.raises(NotImplementedError, match="§8"):
            unet.setup_hooks(style_reference_states={})
    finally:
        unet.setup_hooks()


@pytest.mark.parametrize("kind", ["ddim", "k_dpmpp_2m", "k_euler_a", "k_heun"])
def test_samplers_with_hooks(small, kind):
    """every sampler runs with ToMe set; with a fixed seed eager == eager, and graph == eager bit for bit (ddim, k_dpmpp_2m); without
    one the capture refuses by name"""
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    unet, u = small
    s = make_sampler(kind, unet, NoiseSchedule(device=DEV))
    kw = dict(num_samples=2, shape=(3, 16, 16), cond=u["context"].to(DEV), num_steps=5, seed=5)
    try:
        plain = s.sample(**kw)
        unet.setup_hooks(tome_info=dict(seed=7))
        eager = s.sample(**kw)
        assert tuple(eager.shape) == tuple(plain.shape) and bool(torch.isfinite(eager).all()) and not torch.equal(eager, plain)
        assert torch.equal(s.sample(**kw), eager)
        if kind in ("ddim", "k_dpmpp_2m"):
            assert torch.equal(s.sample(**kw, use_graph=True), eager)
            unet.setup_hooks(tome_info=dict(use_rand=False))
            assert torch.equal(s.sample(**kw, use_graph=True), s.sample(**kw))
            unet.setup_hooks(tome_info=dict())  # a random split and no seed
            assert bool(torch.isfinite(s.sample(**kw)).all())
            with pytest.raises(ValueError, match="fixed split"):
                s.sample(**kw, use_graph=True)
            torch.cuda.synchronize()
        unet.setup_hooks()
        assert torch.equal(s.sample(**kw), plain)
    finally:
        unet.setup_hooks()


def test_controlnet_with_hooks_on_both_models(monkeypatch):
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler
    from cflearn_amd.modules import UNetDiffuser
    from controlnet_weights import fill_parameters

    g = torch.load(os.path.join(GOLDEN, "controlnet_small.pt"), map_location="cpu", weights_only=False)
    torch.manual_seed(0)
    unet, cn = UNetDiffuser(**g["unet_cfg"]), C.ControlNet(**g["cfg"])
    fill_parameters(unet, g["unet_seed"])
    fill_parameters(cn, g["control_seed"])
    unet, cn = unet.to(DEV).eval(), cn.to(DEV).eval()
    i = {k: g[k].to(DEV) for k in ("x_t", "hint", "timesteps", "context")}
    seen = _calls(monkeypatch)
    with torch.no_grad():
        ctrl = cn(i["x_t"], i["hint"], timesteps=i["timesteps"], context=i["context"], scales=g["scales"])
        plain = unet(i["x_t"], timesteps=i["timesteps"], context=i["context"], control=ctrl)
        assert not seen
        cn.setup_hooks(tome_info=dict(seed=2))
        ctrl_m = cn(i["x_t"], i["hint"], timesteps=i["timesteps"], context=i["context"], scales=g["scales"])
        in_cn = len(seen)
        assert in_cn > 0 and len(ctrl_m) == len(ctrl) and all(a.shape == b.shape for a, b in zip(ctrl_m, ctrl))
        unet.setup_hooks(tome_info=dict(seed=2))
        out = unet(i["x_t"], timesteps=i["timesteps"], context=i["context"], control=ctrl_m)
        assert len(seen) > in_cn and tuple(out.shape) == tuple(plain.shape) and bool(torch.isfinite(out).all())
    smp = make_sampler("ddim", unet, NoiseSchedule(device=DEV), control_model=cn, control_scales=g["scales"])
    z = torch.randn(i["x_t"].shape, generator=_gen(6)).to(DEV)
    kw = dict(cond=i["context"], num_steps=4, seed=3, hint=i["hint"])
    a = smp.sample(z, **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(smp.sample(z, **kw), a)
    assert torch.equal(smp.sample(z, **kw, use_graph=True), a)
    cn.setup_hooks()
    unet.setup_hooks()
    with pytest.raises(NotImplementedError, match="§8"):
        cn.setup_hooks(style_reference_states={})
