"""NBM (neural basis model) on the kernels of csrc/nbm.hip: the host side of the reference's `nbm` (modules/ml/nbm.py) — the autograd
Functions of the per-basis MLPs and of the featurizer, and the parameter holders whose state-dict keys are the reference's.

`BasesFn` packs W2 once per forward (`ops.nbm_pack`) and runs one `ops.nbm_bases` launch for all bases and rows; it saves x, the index
table and the pack, nothing of size B D NB H.  Its backward is one `ops.nbm_bases_grad` call that recomputes the hidden layers and
writes every wanted gradient: each parameter's destination is claimed through `functional.param_grad` (nested, so that ONE launch
serves all of them and every claim is committed after it), a parameter with requires_grad = False gets a null destination and no
reduce launch.  `FeaturizeFn` is the grouped 1x1 convolution over the bases (`ops.nbm_featurize` / `ops.nbm_featurize_grad`), `HeadFn`
the f32 Linear head."""
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from . import functional as HF
from . import ops
from .functional import grads_in_one_launch  # noqa: F401  (its home since the RWKV mixers share it)


def _basis_views(w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, w3: Tensor, b3: Tensor, order: int):
    """the conv parameters of one NBMBlock as the matrices of the kernels: w1 [NB, H, o], b1 [NB, H], W2 [NB, H, H], b2, w3 [NB, H], b3"""
    nb = b3.numel()
    h = b1.numel() // nb
    d = lambda t: t.detach()  # noqa: E731
    return d(w1).view(nb, h, order), d(b1).view(nb, h), d(w2).view(nb, h, h), d(b2).view(nb, h), d(w3).view(nb, h), d(b3).view(nb)


class BasesFn(Function):
    """bases f32 [B, D, NB] of one order from x f32 [B, F]; replaces NBMBlock.forward (modules/ml/nbm.py:98-120).  The six parameters
    are the block's conv weights and biases in their nn.Conv1d shapes."""

    NAMES = ("dw1", "db1", "dw2", "db2", "dw3", "db3")

    @staticmethod
    def forward(ctx: Any, x: Tensor, idx: ops.NbmIndex, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, w3: Tensor, b3: Tensor) -> Tensor:
        order = idx.shape[1]
        v1, c1, v2, c2, v3, c3 = _basis_views(w1, b1, w2, b2, w3, b3, order)
        xd = x.detach()
        if xd.stride(-1) != 1:
            xd = xd.contiguous()
        packed = ops.nbm_pack(v2)
        out = ops.nbm_bases(xd, idx, v1, c1, packed, c2, v3, c3)
        ctx.params = (w1, b1, w2, b2, w3, b3)
        ctx.idx = idx
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xd, packed)
        return out

    @staticmethod
    def backward(ctx: Any, dbases: Tensor):  # type: ignore
        xd, packed = ctx.saved_tensors
        idx = ctx.idx
        v1, c1, _, c2, v3, _ = _basis_views(*ctx.params, idx.shape[1])
        want = {name: p for name, p in zip(BasesFn.NAMES, ctx.params) if p.requires_grad}
        want_dx = ctx.needs_input_grad[0]
        dbases = dbases.float().contiguous()
        dx: List[Optional[Tensor]] = [None]

        def launch(dests: Dict[str, Tensor], accumulate: Sequence[str]) -> None:
            dx[0] = ops.nbm_bases_grad(dbases, xd, idx, v1, c1, packed, c2, v3, dests=dests, accumulate=accumulate, want_dx=want_dx)

        grads = grads_in_one_launch(want, launch) if (want or want_dx) else {}
        return (dx[0], None, *(grads.get(name) for name in BasesFn.NAMES))


class FeaturizeFn(Function):
    """feat f32 [B, D] = the grouped 1x1 convolution of NBM.featurizer (modules/ml/nbm.py:168-174, 189-194) over bases f32 [B, D, NB];
    weight [D, NB, 1] and bias [D] are nn.Conv1d's."""

    @staticmethod
    def forward(ctx: Any, bases: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
        bd = bases.detach().contiguous()
        feat = ops.nbm_featurize(bd, weight.detach().view(weight.shape[0], -1), bias.detach())
        ctx.weight, ctx.bias = weight, bias
        if weight.requires_grad:
            ctx.save_for_backward(bd)
        return feat

    @staticmethod
    def backward(ctx: Any, dfeat: Tensor):  # type: ignore
        weight, bias = ctx.weight, ctx.bias
        bd = ctx.saved_tensors[0] if weight.requires_grad else None
        wf = weight.detach().view(weight.shape[0], -1)
        dfeat = dfeat.float().contiguous()
        want = {name: p for name, p in (("dwf", weight), ("dbf", bias)) if p.requires_grad}
        want_dbases = ctx.needs_input_grad[0]
        dbases: List[Optional[Tensor]] = [None]

        def launch(dests: Dict[str, Tensor], accumulate: Sequence[str]) -> None:
            dbases[0] = ops.nbm_featurize_grad(dfeat, bd, wf, dwf=dests.get("dwf"), dbf=dests.get("dbf"), accumulate=accumulate,
                                               want_dbases=want_dbases)

        grads = grads_in_one_launch(want, launch) if (want or want_dbases) else {}
        return dbases[0], grads.get("dwf"), grads.get("dbf")


class SeparableMapping(nn.Module):
    """the parameters of one grouped 1x1 layer (modules/ml/nbm.py:18-51): `conv.weight` [NB out, in, 1] and `conv.bias` [NB out] with
    nn.Conv1d's own initialisation.  The layer is never called: `BasesFn` reads its parameters."""

    def __init__(self, in_dim: int, out_dim: int, num_groups: int):
        super().__init__()
        self.in_dim, self.out_dim, self.num_groups = in_dim, out_dim, num_groups
        self.conv = nn.Conv1d(in_dim * num_groups, out_dim * num_groups, 1, groups=num_groups, bias=True)


class NBMBlock(nn.Module):
    """the bases of one order (modules/ml/nbm.py:54-120): `net.0`, `net.1`, `net.2` = order -> H -> H -> 1 per basis"""

    def __init__(self, order: int, num_bases: int, hidden: int):
        super().__init__()
        self.order, self.num_bases, self.hidden = order, num_bases, hidden
        self.net = nn.Sequential(SeparableMapping(order, hidden, num_bases), SeparableMapping(hidden, hidden, num_bases),
                                 SeparableMapping(hidden, 1, num_bases))

    def forward(self, net: Tensor, idx: ops.NbmIndex) -> Tensor:
        if idx.shape[1] != self.order:
            raise ValueError(f"length of every tuple in indices must be {self.order}, got a table of width {idx.shape[1]}")
        convs = [m.conv for m in self.net]
        return BasesFn.apply(net, idx, convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias, convs[2].weight, convs[2].bias)


def featurize(bases: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    return FeaturizeFn.apply(bases, weight, bias)


class HeadFn(Function):
    """logits f32 [B, out] = feat W^T + b of NBM.head (modules/ml/nbm.py:175, 198) in f32 on `ops.sgemm_f32`: latent_dim features
    wide and output_dim outputs, a product of no weight in time.  `functional.linear` rounds x, W, the incoming gradient and dX to
    bf16; here that put head.bias (the column sum of dy) and featurizer.bias (the column sum of dX) at 1.13 .. 1.30 x the
    reference's own bf16-autocast distance, so the head keeps f32 end to end: the bias rides in the product as one more
    column ([feat, 1] [W, b]^T), dX = dy W, dW = dy^T feat, db = the column sum of dy (`ops.colreduce_f32`)."""

    @staticmethod
    def forward(ctx: Any, feat: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
        fd = feat.detach()
        ones = torch.ones((fd.shape[0], 1), dtype=fd.dtype, device=fd.device)
        y = ops.sgemm_f32(torch.cat([fd, ones], 1), torch.cat([weight.detach(), bias.detach()[:, None]], 1))
        ctx.weight, ctx.bias = weight, bias
        ctx.save_for_backward(fd)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (fd,) = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy = dy.float().contiguous()
        dx = ops.sgemm_f32(dy, weight.detach().contiguous(), b_trans=True) if ctx.needs_input_grad[0] else None
        gw = gb = None
        if weight.requires_grad:
            gw = HF.store_param_grad(weight, ops.sgemm_f32(dy, fd.contiguous(), a_trans=True, b_trans=True))
        if bias.requires_grad:
            gb = HF.param_grad(bias, lambda out, acc: ops.colreduce_f32(dy, out=out.view(-1), accumulate=acc))
        return dx, gw, gb


def head(feat: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    return HeadFn.apply(feat, weight, bias)


def check_nary(nary: Dict[str, Sequence[Sequence[int]]], input_dim: int) -> Dict[str, List[Tuple[int, ...]]]:
    """the reference's `nary` with every tuple as a tuple of ints; orders outside the kernels are refused by name"""
    out: Dict[str, List[Tuple[int, ...]]] = {}
    for key, tuples in nary.items():
        order = int(key)
        if not 1 <= order <= ops.NBM_MAX_ORDER:
            raise NotImplementedError(f"nbm: order {order} is outside the basis kernels (1 .. {ops.NBM_MAX_ORDER}; DESIGN §8)")
        packs = [tuple(int(i) for i in pack) for pack in tuples]
        for i, pack in enumerate(packs):
            if len(pack) != order:
                raise ValueError(f"length of every tuple in indices must be {order}, but got {pack} at index {i}")
            if any(not 0 <= c < input_dim for c in pack):
                raise ValueError(f"nbm: tuple {pack} addresses a feature outside [0, {input_dim})")
        if not packs:
            raise ValueError(f"nbm: order {order} has no tuples")
        out[str(key)] = packs
    return out
