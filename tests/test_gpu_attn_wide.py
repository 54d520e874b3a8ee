"""The wide-head attention forward (csrc/attn_wide.hip, `ops.attn_wide_fwd`): head widths past the 192 of the dispatcher's
kernels, per element against float64, inside guarded buffers — the method of test_gpu_attn_dispatch.py.

Operands are bf16 in NaN-surrounded buffers, outputs start as NaN between byte guards; O and lse are compared element by
element with `helpers.attn_ref` under the error model of `helpers.assert_attn_forward`, unchanged: the wide kernels are the
general forward carried on to more 64-column halves, with the same roundings (f32 scores of depth dh, P rounded to bf16 before
P V, one exp2 and one product rounding on O and on l per staged key chunk).  The model's online-softmax term counts one rescale
per 64 keys; head widths above 448 stage 32 keys at a time and rescale twice as often (8 ceil(Tk / 64) instead of 4 ceil(Tk /
64) units of 2^-24, beside the 2^16 of the bf16 rounding of P): no term was added to `k` for it and `ulps` is untouched.

Shapes: the first width past the old limit (200), a multiple of 64 (256), a width whose last 64-column half is ragged (264) and
the maximum (512); one key and one query, ragged lengths inside one chunk, one key past two 64-key chunks' worth of queries and
keys, more than one 128-row query workgroup, and 2 CH + 5 keys (CH = the staged chunk)."""
import math

import pytest
import torch

from helpers import assert_attn_forward, attn_ref, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
CH = _lib.DEFINES["CFHIP_ATTN_WIDE_CHUNK"]
SHAPES = [(1, 1), (37, 53), (70, 129), (130, 130), (33, 2 * CH + 5)]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(BF16)


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("tq,tk", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("dh", [200, 256, 264, 512])
def test_wide_forward_per_element(G, dh, tq, tk, heads):
    """plain strides with and without lse (the same O bit for bit), and, where Tq = Tk, the three operands read in place out of
    one packed [B, T, 3, H dh] projection"""
    bsz, d = 2, heads * dh
    seed0 = 7 * dh + 3 * tq + tk + heads
    q, k, v = _randn((bsz, tq, d), seed0), _randn((bsz, tk, d), seed0 + 1), _randn((bsz, tk, d), seed0 + 2)
    qd, kd, vd = (G.poisoned(t.to(DEV)) for t in (q, k, v))
    sc = 1.0 / math.sqrt(dh)
    ref = attn_ref(q, k, v, heads, dh, None, False, sc)
    tag = f"wide dh{dh} {tq}x{tk} H{heads}"
    o, lse = ops.attn_wide_fwd(qd, kd, vd, heads, head_dim=dh)  # (allocated through the guarded `ops.torch`)
    assert o.dtype == BF16 and tuple(o.shape) == (bsz, tq, d) and tuple(lse.shape) == (bsz, heads, tq)
    assert_attn_forward(o, lse, ref, sc, tag=tag)
    o2, none = ops.attn_wide_fwd(qd, kd, vd, heads, head_dim=dh, want_lse=False)
    assert none is None and torch.equal(o2, o), f"{tag}: O differs without an lse buffer"
    G.check()
    if tq == tk:
        qkv = torch.stack((q, k, v), dim=2)  # [B, T, 3, H dh]
        qkv_d = G.poisoned(qkv.to(DEV))
        o3, lse3 = ops.attn_wide_fwd(qkv_d[:, :, 0], qkv_d[:, :, 1], qkv_d[:, :, 2], heads, head_dim=dh, scale=sc)
        assert torch.equal(o3, o) and torch.equal(lse3, lse), f"{tag}: the packed projection gives another result"


def test_wide_forward_scale_and_out_view(G):
    """an explicit scale, and `out=` a column block of a wider row (the token stride of O is not H dh)"""
    dh, tq, tk, bsz = 264, 19, 70, 2
    q, k, v = _randn((bsz, tq, dh), 1), _randn((bsz, tk, dh), 2), _randn((bsz, tk, dh), 3)
    qd, kd, vd = (G.poisoned(t.to(DEV)) for t in (q, k, v))
    sc = 0.037
    (whole,) = G.region((bsz, tq, dh + 24), BF16, DEV, lambda w: [w[:, :, 8:8 + dh]])
    whole.fill_(float("nan"))
    o, lse = ops.attn_wide_fwd(qd, kd, vd, 1, head_dim=dh, scale=sc, out=whole)
    assert o is whole
    assert_attn_forward(o, lse, attn_ref(q, k, v, 1, dh, None, False, sc), sc, tag="wide out view")


def test_wide_refuses_what_it_does_not_cover():
    x = torch.zeros((1, 4, 512), dtype=BF16, device=DEV)
    for dh in (192, 520, 260):
        with pytest.raises(ValueError, match="head_dim"):
            ops.attn_wide_fwd(x[..., :dh], x[..., :dh], x[..., :dh], 1, head_dim=dh)
    with pytest.raises(ValueError, match="head_dim"):  # the dispatcher's entry keeps its limit
        ops.attn_fwd(x[..., :200].contiguous(), x[..., :200].contiguous(), x[..., :200].contiguous(), 1, head_dim=200)
