"""CPU self-tests of the per-element and guard helpers (tests/helpers.py): they show the gap a whole-tensor
rel-L2 leaves and that the per-element check and the guarded allocations close it.  No GPU needed."""
import math

import pytest
import torch

from helpers import (GuardedOps, assert_attn_backward, assert_attn_forward, assert_close, assert_conv3x3_rows, assert_elementwise,
                     attn_mask as make_mask, attn_ref, conv3x3_rows_ref, guarded_ops, ulp_out)


def test_one_wrong_element_passes_rel_l2_but_not_elementwise():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1_000_000, generator=g, dtype=torch.float64)
    got = ref.to(torch.bfloat16)
    got[654_321] += 1.0
    assert_close(got, ref, 4e-3, "one wrong element")  # the whole-tensor norm does not see it
    with pytest.raises(AssertionError, match=r"(?s)1 of 1000000 elements out of bound.*\[654321\]"):
        assert_elementwise(got, ref, out_dtype=torch.bfloat16, what="one wrong element")


def test_correctly_rounded_bf16_passes_at_one_ulp():
    g = torch.Generator().manual_seed(1)
    ref = torch.cat([torch.randn(100_000, generator=g, dtype=torch.float64) * 10.0 ** e for e in (-30, -3, 0, 3, 30)])
    ref = torch.cat([ref, torch.tensor([0.0, -0.0, 1e-40, 2.0 ** -126, 65504.0, 3.3e38])])
    assert_elementwise(ref.to(torch.bfloat16), ref, out_dtype=torch.bfloat16, ulps=1.0, what="bf16 RNE")
    assert_elementwise(ref.to(torch.float32), ref, out_dtype=torch.float32, ulps=1.0, what="f32 RNE")
    # ... and one ulp more than that does not
    bad = ref.to(torch.bfloat16).double()
    bad[7] += 2 * ulp_out(ref[7:8].abs(), torch.bfloat16)[0]
    with pytest.raises(AssertionError, match=r"\[7\]"):
        assert_elementwise(bad, ref, out_dtype=torch.bfloat16, ulps=1.0)


def test_ulp_spacing():
    u = ulp_out(torch.tensor([1.0, 1.5, 2.0, 3.99, 0.0, 1e-300]), torch.bfloat16)
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133]
    assert ulp_out(torch.tensor([1.0]), torch.float32).item() == 2.0 ** -23


def test_accumulation_term():
    ref = torch.tensor([0.0], dtype=torch.float64)
    got = torch.tensor([3e-6])
    with pytest.raises(AssertionError):
        assert_elementwise(got, ref, out_dtype=torch.float32)
    # an f32 sum of 100 terms of size 1 may be off by ~100 * 2^-24
    assert_elementwise(got, ref, out_dtype=torch.float32, cond=torch.tensor([100.0]), k=100)


def test_nan_and_inf_positions_must_match():
    ref = torch.tensor([1.0, 2.0, float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
    assert_elementwise(ref.float(), ref, out_dtype=torch.float32)
    for i, v in ((0, float("nan")), (2, 3.0), (3, -float("inf")), (4, 1e30), (1, float("inf"))):
        got = ref.float().clone()
        got[i] = v
        with pytest.raises(AssertionError, match=rf"\[{i}\]"):
            assert_elementwise(got, ref, out_dtype=torch.float32)


def _past(t, at):
    """a one-element view of t's storage at flat element `at` (may lie outside t itself)"""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + at)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("where", [-1, "end"])
def test_write_outside_a_guarded_allocation_fails_check(dtype, where):
    g = GuardedOps()
    t = g.empty((5, 3), dtype=dtype)
    assert t.data_ptr() % 256 == 0
    if t.is_floating_point():
        assert torch.isnan(t.float()).all()
    t.fill_(1)
    g.check()  # writing the interior is fine
    t = g.empty(5, 3, dtype=dtype)
    _past(t, t.numel() if where == "end" else -1).fill_(1)
    with pytest.raises(AssertionError, match=r"(?s)\(5, 3\).*first at byte offset " + ("-" if where == -1 else "")):
        g.check()


def test_unwritten_element_of_a_guarded_empty_shows_as_nan():
    g = GuardedOps()
    out = g.empty((1000,), dtype=torch.float32)
    ref = torch.arange(1000, dtype=torch.float64)
    out[:999] = ref[:999].float()  # a kernel that forgets its last element
    g.check()
    with pytest.raises(AssertionError, match=r"(?s)1 of 1000 elements out of bound.*\[999\] got nan"):
        assert_elementwise(out, ref, out_dtype=torch.float32)


def test_zeros_and_empty_like():
    g = GuardedOps()
    z = g.zeros((7,), dtype=torch.float32)
    assert torch.equal(z, torch.zeros(7))
    e = g.empty_like(torch.ones(3, 4, dtype=torch.bfloat16))
    assert e.shape == (3, 4) and e.dtype == torch.bfloat16 and torch.isnan(e.float()).all()
    g.check()


def test_poisoned_input_reads_past_the_end_see_nan():
    g = GuardedOps()
    x = g.poisoned(torch.arange(10, dtype=torch.float32))
    assert torch.equal(x, torch.arange(10, dtype=torch.float32)) and x.data_ptr() % 256 == 0
    assert torch.isnan(_past(x, 10)).all() and torch.isnan(_past(x, -1)).all()
    idx = g.index(torch.tensor([3, 1, 2]))
    assert _past(idx, 3).item() == 0 and _past(idx, -1).item() == 0
    g.check()
    x = g.poisoned(torch.arange(10, dtype=torch.float32))
    _past(x, 11).fill_(0.0)  # an input's guards are checked for writes as well
    with pytest.raises(AssertionError, match="input"):
        g.check()


def test_out2d_padding_and_guard_rows():
    g = GuardedOps()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    assert out.shape == (4, 5) and out.stride() == (8, 1)
    out.fill_(0.5)
    g.check()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    _past(out, 5).fill_(0.5)  # a column store past N (ldc > N)
    with pytest.raises(AssertionError, match="out2d 4x5 ld 8"):
        g.check()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    _past(out, 4 * 8).fill_(0.5)  # the row after the last
    with pytest.raises(AssertionError, match="out2d"):
        g.check()


def test_region_with_sentinel_gaps():
    g = GuardedOps()
    a, b = g.region((10, 4), torch.float32, "cpu", lambda w: (w[1:4], w[6:9]))
    a.fill_(1.0)
    b.fill_(2.0)
    g.check()
    a, b = g.region((10, 4), torch.float32, "cpu", lambda w: (w[1:4], w[6:9]))
    _past(a, 12).fill_(1.0)  # problem a writes one row into the gap
    with pytest.raises(AssertionError, match="region"):
        g.check()


def test_guarded_ops_patches_only_ops_torch(monkeypatch):
    from cflearn_amd import functional, ops

    g = guarded_ops(monkeypatch)
    assert ops.torch.empty is not torch.empty and ops.torch.bfloat16 is torch.bfloat16
    assert functional.torch is torch
    t = ops.torch.empty((2, 3), dtype=torch.float32, device="cpu")
    assert torch.isnan(t).all() and len(g.allocs) == 1
    g.check()


# ---------------------------------------------------------------------------------------------
# the attention error model is the right size: an emulation of the kernels' arithmetic passes it, three planted defects do not
# ---------------------------------------------------------------------------------------------

LOG2E = 1.4426950408889634


def _emulated_attention(q, k, v, heads, dh, mask, causal, scale, block, defect=None):
    """The arithmetic of the chunked forward kernels in f32 torch on the CPU: f32 scores, online softmax over `block`-key
    blocks in the log2 domain (running maximum, exp2, rescale of O and of the row sum by alpha), P rounded to bf16
    before the PV product, f32 accumulation, O = acc * (1 / l) rounded to bf16, lse = (m + log2 l) / log2 e in f32.
    `defect`: "key" (the score of one key of one row is lost), "rescale" (the P tile of one 16-row tile of one block is
    left as taken against the old running maximum after the maximum of one of its rows changed), "columns" (the last 8
    columns of every head stay 0).  Returns O, lse and whether the defect was planted."""
    bsz, tq, _ = q.shape
    tk = k.shape[1]
    sh = lambda t, n: t.float().view(bsz, n, heads, dh).transpose(1, 2)  # noqa: E731
    Q, K, V = sh(q, tq), sh(k, tk), sh(v, tk)
    keep = torch.ones(tq, tk, dtype=torch.bool)
    if causal:
        keep = torch.tril(keep)
    if mask is not None:
        keep = keep & mask
    keep = keep.expand(bsz, heads, tq, tk).clone()
    if defect == "key":
        alive_keys = torch.nonzero(keep[0, 1, tq // 2]).view(-1)
        keep[0, 1, tq // 2, alive_keys[len(alive_keys) // 2]] = False
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    m = torch.full((bsz, heads, tq), -math.inf)
    l = torch.zeros((bsz, heads, tq))
    acc = torch.zeros((bsz, heads, tq, dh))
    for c, j0 in enumerate(range(0, tk, block)):
        j1 = min(tk, j0 + block)
        s = (Q @ K[:, :, j0:j1].transpose(-1, -2)) * sl2
        s = s.masked_fill(~keep[..., j0:j1], -math.inf)
        m_new = torch.maximum(m, s.amax(-1))
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        e = torch.exp2(s - m_use[..., None])
        l = l * alpha + e.sum(-1)
        pt = e.clone()
        if defect == "rescale" and c >= 1:  # the first 16-row tile with a row whose maximum rose by more than 1 (log2 domain)
            rose = torch.nonzero((alpha[0, 0] < 0.5) & (alpha[0, 0] > 0)).view(-1)
            if len(rose):  # its P tile is still the one taken against the OLD maximum
                tile = int(rose[0]) // 16 * 16
                pt[0, 0, tile:tile + 16] = torch.exp2(s[0, 0, tile:tile + 16] - m[0, 0, tile:tile + 16, None])
                defect = "rescale: planted"
        acc = acc * alpha[..., None] + pt.to(torch.bfloat16).float() @ V[:, :, j0:j1]
        m = m_new
    o = acc * (1.0 / l)[..., None]
    if defect == "columns":
        o[..., dh - 8:] = 0.0
    lse = (m + torch.log2(l)) * torch.tensor(1.0 / LOG2E, dtype=torch.float32)
    return o.to(torch.bfloat16).transpose(1, 2).reshape(bsz, tq, heads * dh), lse, defect != "rescale"


ATTN_EMULATION_SHAPES = [
    # dh, Tq, Tk, mode, mask kind, block: shapes of tests/test_gpu_attn_dispatch.py (385 is its largest Tk)
    (192, 70, 257, "mask", "full", 128),
    (64, 385, 385, "causal", "band", 64),
    (160, 70, 385, "mask", "prefix", 128),
    (40, 600, 77, "plain", None, 64),
    (64, 37, 53, "plain", None, 64),
    (24, 100, 140, "mask", "pad", 64),
    (192, 130, 200, "mask", "rand", 128),
]


@pytest.mark.parametrize("dh,tq,tk,mode,mask_kind,block", ATTN_EMULATION_SHAPES)
def test_attention_bounds_fit_an_emulation_of_the_kernel_arithmetic(dh, tq, tk, mode, mask_kind, block):
    bsz, heads = 1, 2
    gen = torch.Generator().manual_seed(dh + tq + tk)
    q, k, v = (torch.randn((bsz, t, heads * dh), generator=gen, dtype=torch.float64).to(torch.bfloat16) for t in (tq, tk, tk))
    mask = make_mask(mask_kind, bsz, heads, tq, tk) if mask_kind else None
    scale = 1.0 / math.sqrt(dh)
    ref = attn_ref(q, k, v, heads, dh, mask, mode == "causal", scale)
    o, lse, _ = _emulated_attention(q, k, v, heads, dh, mask, mode == "causal", scale, block)
    assert_attn_forward(o, lse, ref, scale, tag="emulation")
    if tk <= block:
        return  # (one block: no rescale to leave out)
    for defect in ("key", "rescale", "columns"):
        o, lse, planted = _emulated_attention(q, k, v, heads, dh, mask, mode == "causal", scale, block, defect)
        assert planted, "no row's maximum rose after the first block: the defect had nowhere to go"
        with pytest.raises(AssertionError, match="out of bound"):
            assert_attn_forward(o, lse, ref, scale, tag=f"emulation with defect {defect}")


def _emulated_attention_backward(q, k, v, o, lse, do, heads, dh, mask, causal, scale, defect=None):
    """The arithmetic of the backward kernels in f32 torch on the CPU: delta = rowsum(dO * O) from the bf16 O, f32 S and
    dP, P = exp2(S scale log2e - lse log2e) from the forward's f32 lse, P and dS = P (dP - delta) rounded to bf16 before
    their products, f32 accumulation, bf16 dQ / dK / dV.  `defect`: "key" (the largest dS element of one row lost), "columns" (the last 8
    columns of dQ, dK and dV stay 0), "delta" (delta of one 16-row tile taken as 0)."""
    bsz, tq, _ = q.shape
    tk = k.shape[1]
    sh = lambda t, n: t.float().view(bsz, n, heads, dh).transpose(1, 2)  # noqa: E731
    Q, K, V, O, dO = sh(q, tq), sh(k, tk), sh(v, tk), sh(o, tq), sh(do, tq)
    keep = torch.ones(tq, tk, dtype=torch.bool)
    if causal:
        keep = torch.tril(keep)
    if mask is not None:
        keep = keep & mask
    keep = keep.expand(bsz, heads, tq, tk)
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    delta = (dO * O).sum(-1, keepdim=True)
    if defect == "delta":
        delta[0, 0, 16:32] = 0.0
    p = torch.exp2((Q @ K.transpose(-1, -2)) * sl2 - (lse * torch.tensor(LOG2E, dtype=torch.float32))[..., None])
    p = torch.where(keep, p, torch.zeros_like(p))
    ds = p * (dO @ V.transpose(-1, -2) - delta)
    if defect == "key":
        ds[0, 1, tq // 2, int(ds[0, 1, tq // 2].abs().argmax())] = 0.0  # (the row's largest: a key that carries weight)
    pb, dsb = p.to(torch.bfloat16).float(), ds.to(torch.bfloat16).float()
    dq, dk, dv = dsb @ K * scale, dsb.transpose(-1, -2) @ Q * scale, pb.transpose(-1, -2) @ dO
    if defect == "columns":
        for t in (dq, dk, dv):
            t[..., dh - 8:] = 0.0
    back = lambda z: z.to(torch.bfloat16).transpose(1, 2).reshape(bsz, -1, heads * dh)  # noqa: E731
    return back(dq), back(dk), back(dv)


@pytest.mark.parametrize("dh,tq,tk,mode,mask_kind,block", ATTN_EMULATION_SHAPES)
def test_attention_backward_bounds_fit_an_emulation_of_the_kernel_arithmetic(dh, tq, tk, mode, mask_kind, block):
    bsz, heads = 1, 2
    gen = torch.Generator().manual_seed(dh + tq + tk)
    q, k, v, do = (torch.randn((bsz, t, heads * dh), generator=gen, dtype=torch.float64).to(torch.bfloat16) for t in (tq, tk, tk, tq))
    mask = make_mask(mask_kind, bsz, heads, tq, tk) if mask_kind else None
    scale = 1.0 / math.sqrt(dh)
    causal = mode == "causal"
    ref = attn_ref(q, k, v, heads, dh, mask, causal, scale)
    o, lse, _ = _emulated_attention(q, k, v, heads, dh, mask, causal, scale, block)
    dq, dk, dv = _emulated_attention_backward(q, k, v, o, lse, do, heads, dh, mask, causal, scale)
    assert_attn_backward(dq, dk, dv, ref, do, scale, tag="emulation")
    for defect in ("key", "columns", "delta"):
        dq, dk, dv = _emulated_attention_backward(q, k, v, o, lse, do, heads, dh, mask, causal, scale, defect)
        with pytest.raises(AssertionError, match="out of bound"):
            assert_attn_backward(dq, dk, dv, ref, do, scale, tag=f"emulation with defect {defect}")


# ---------------------------------------------------------------------------------------------
# the convolution bound is the right size: f32 arithmetic passes it, one wrong border tap does not
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_bias", [True, False])
def test_conv3x3_bound_fits_f32_arithmetic_and_sees_one_wrong_border_tap(with_bias):
    """The per-element assertion of tests/test_gpu_conv_kernels.py on (2, 64, 168, 13, 11): torch's f32 convolution of the same
    bf16 operands, rounded once to bf16, stays inside it; a copy in which the left-edge tap (ky, kx) = (1, 0) of ONE image row reads
    the previous row's last pixel (flat pixel p - 1) instead of the zero padding does not: the 168 outputs of that pixel are named."""
    b, cin, cout, h, w = 2, 64, 168, 13, 11
    g = torch.Generator().manual_seed(13)
    x = torch.randn((b, cin, h, w), generator=g, dtype=torch.float64).to(torch.bfloat16)
    wt = (torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64) / (3.0 * cin ** 0.5)).to(torch.bfloat16)
    bias = torch.randn(cout, generator=g) if with_bias else None
    ref = conv3x3_rows_ref(x, wt, bias)
    y = torch.nn.functional.conv2d(x.float(), wt.float(), bias, padding=1)
    rows = lambda t: t.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(b * h * w, cout)  # noqa: E731
    assert_conv3x3_rows(rows(y), ref, cin, "f32 convolution")
    bad = y.clone()
    img, row = 1, 5
    bad[img, :, row, 0] += wt[:, :, 1, 0].float() @ x[img, :, row - 1, w - 1].float()
    first = ((img * h + row) * w) * cout
    with pytest.raises(AssertionError, match=rf"(?s)of {b * h * w * cout} elements out of bound.*\[{first}"):
        assert_conv3x3_rows(rows(bad), ref, cin, "one wrong border tap")
