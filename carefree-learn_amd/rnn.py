"""GRU / LSTM layers on the recurrent kernels of csrc/rnn.hip: the host side of the reference's `ml_rnn` (modules/ml/rnn.py:13-85) — the
autograd Function of the recurrence and the single-layer, batch_first `GRU` / `LSTM` modules that `modules.RNN` stacks.

One layer forward: the input projection of all time steps, gx = x W_ih^T + b_ih, is one `functional.linear` per direction (its dX,
dW_ih and db_ih are LinearFn's; `linear` takes any input width — narrow tabular widths run on its shape-agnostic kernel — so no
feature column is padded here).  With `two_word_input`, which `modules.RNN` sets on its first layer, an f32 input enters as two bf16
words and the projection is `InputProjFn` below: two GEMMs on the same W_ih, the second adding into the first in f32.
`RecurrentFn` packs W_hh (`ops.rnn_pack`, once per forward) and runs one `ops.rnn_fwd` launch per
direction, both directions writing their half of one [B, T, D H] buffer.  In training mode the forward kernel saves the gate values
(and the LSTM's cell states) and the bf16 state each step started from; the backward is one `ops.rnn_bwd` launch per direction, then
dW_hh = dgh^T h_prev as one `tn` GEMM over the B T rows and db_hh as the column sum of dgh, each only when its parameter asks for a
gradient, through `functional.param_grad`.  Under torch.no_grad() nothing is saved."""
import math
from typing import Any, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from . import functional as HF
from . import ops

CELL_IDS = {"GRU": ops.RNN_GRU, "LSTM": ops.RNN_LSTM}


class RecurrentFn(Function):
    """y f32 [B, T, D H] of one layer from gx (f32 [B, T, G H]) per direction; replaces the recurrence inside nn.GRU / nn.LSTM
    (modules/ml/rnn.py:82-85 with `None` initial states)."""

    @staticmethod
    def forward(ctx: Any, cell: int, save: bool, gx_f: Tensor, w_hh_f: Tensor, b_hh_f: Tensor, gx_r: Optional[Tensor],
                w_hh_r: Optional[Tensor], b_hh_r: Optional[Tensor]) -> Tensor:
        dirs = [(gx_f, w_hh_f, b_hh_f)] + ([] if gx_r is None else [(gx_r, w_hh_r, b_hh_r)])
        b, steps = gx_f.shape[0], gx_f.shape[1]
        h = w_hh_f.shape[1]
        y = torch.empty((b, steps, len(dirs) * h), dtype=torch.float32, device=gx_f.device)
        keep = []
        for d, (gx, w, bias) in enumerate(dirs):
            packed = ops.rnn_pack(w.detach().contiguous(), cell)
            _, _, _, saved = ops.rnn_fwd(gx.detach().contiguous(), packed, bias.detach().contiguous(), cell, y=y[:, :, d * h:(d + 1) * h],
                                         reverse=d == 1, save=save)
            if save:
                gates, cseq, hprev = saved
                keep += [packed, gates, hprev] + ([cseq] if cseq is not None else [])
        ctx.cell, ctx.h, ctx.ndir, ctx.saved_any = cell, h, len(dirs), save
        ctx.params = [(w, bias) for _, w, bias in dirs]
        if save:
            ctx.save_for_backward(y, *keep)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        if not ctx.saved_any:
            raise RuntimeError("RecurrentFn: this forward ran without saving its gates")
        y, *keep = ctx.saved_tensors
        cell, h = ctx.cell, ctx.h
        per = 4 if cell == ops.RNN_LSTM else 3
        dy = dy.float().contiguous()
        grads = []
        for d in range(ctx.ndir):
            packed, gates, hprev = keep[d * per:d * per + 3]
            cseq = keep[d * per + 3] if per == 4 else None
            w, bias = ctx.params[d]
            need_gx = ctx.needs_input_grad[2 + 3 * d]
            if not (need_gx or w.requires_grad or bias.requires_grad):
                grads += [None, None, None]
                continue
            sl = slice(d * h, (d + 1) * h)
            dgx, dgh, _, _ = ops.rnn_bwd(dy[:, :, sl], packed, cell, (gates, cseq, hprev), y[:, :, sl], reverse=d == 1)
            dgh2, hp2 = dgh.view(-1, dgh.shape[-1]), hprev.view(-1, h)
            gw = gb = None
            if w.requires_grad:  # dW_hh = sum_t dgh_t^T h_{t-1}: one tn GEMM over the B T rows
                gw = HF.param_grad(w, lambda out, acc: ops.gemm(dgh2, hp2, a_trans=True, b_trans=True, out=out, accumulate=acc))
            if bias.requires_grad:
                gb = HF.param_grad(bias, lambda out, acc: ops.colsum(dgh2, out=out.view(-1), accumulate=acc))
            grads += [dgx if need_gx else None, gw, gb]
        if ctx.ndir == 1:
            grads += [None, None, None]
        return (None, None, *grads)


class InputProjFn(Function):
    """gx f32 [B, T, G H] = x W_ih^T + b_ih with the f32 x taken as two bf16 words, hi = bf16(x) and lo = bf16(x - hi)
    (`ops.split_f32`; x = hi + lo to 2^-17): raw tabular / time-series features are not scaled for an 8-bit mantissa.  Two GEMMs on
    the same bf16 W_ih, the second adding into the first in f32 (residual epilogue); dW_ih = dgx^T hi + dgx^T lo as two `tn` GEMMs
    inside ONE claim of the parameter's gradient (two LinearFn calls on one weight would each commit it), db_ih the column sum,
    dX = dgx W_ih once."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
        hi, lo = ops.split_f32(x.detach().reshape(-1, x.shape[-1]).contiguous())
        w16 = HF.shadow_bf16(weight)
        gx = ops.gemm(hi, w16, bias=bias.detach().contiguous(), out_dtype=torch.float32)
        gx = ops.gemm(lo, w16, epilogue=ops.EPI_RESIDUAL, aux_in=gx, out_dtype=torch.float32)
        ctx.save_for_backward(hi, lo, w16)
        ctx.weight, ctx.bias, ctx.x_shape = weight, bias, x.shape
        return gx.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx: Any, dgx: Tensor):  # type: ignore
        hi, lo, w16 = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        d2 = HF._as_bf16_2d(dgx)
        if not d2.is_contiguous():
            d2 = d2.contiguous()
        dx = ops.gemm(d2, w16, b_trans=True).view(ctx.x_shape) if ctx.needs_input_grad[0] else None  # bf16; autograd casts
        gw = gb = None

        def dw_into(out: Tensor, acc: bool) -> None:
            ops.gemm(d2, hi, a_trans=True, b_trans=True, out=out, accumulate=acc)
            ops.gemm(d2, lo, a_trans=True, b_trans=True, out=out, accumulate=True)

        if weight.requires_grad:
            gw = HF.param_grad(weight, dw_into)
        if bias.requires_grad:
            gb = HF.param_grad(bias, lambda out, acc: ops.colsum(d2, out=out.view(-1), accumulate=acc))
        return dx, gw, gb


def recurrence(cell: int, gx_f: Tensor, w_hh_f: Tensor, b_hh_f: Tensor, gx_r: Optional[Tensor] = None, w_hh_r: Optional[Tensor] = None,
               b_hh_r: Optional[Tensor] = None) -> Tensor:
    tensors = (gx_f, w_hh_f, b_hh_f, gx_r, w_hh_r, b_hh_r)
    save = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
    return RecurrentFn.apply(cell, save, *tensors)


class _RecurrentLayer(nn.Module):
    """One batch_first layer with nn.GRU's / nn.LSTM's parameter names, shapes, registration order and `reset_parameters`."""

    cell_name = ""
    gate_count = 0

    def __init__(self, input_size: int, hidden_size: int, bidirectional: bool = False, two_word_input: bool = False):
        super().__init__()
        self.two_word_input = two_word_input  # an f32 input enters the projection as two bf16 words (InputProjFn)
        if not ops.rnn_hidden_ok(hidden_size):
            raise NotImplementedError(f"{self.cell_name}: hidden_size = {hidden_size} is outside the recurrent kernels (a multiple of 8, "
                                      f"8 .. {ops.RNN_MAX_HIDDEN}; DESIGN §8)")
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bidirectional
        gh = self.gate_count * hidden_size
        for suffix in ("", "_reverse") if bidirectional else ("",):
            self.register_parameter(f"weight_ih_l0{suffix}", nn.Parameter(torch.empty(gh, input_size)))
            self.register_parameter(f"weight_hh_l0{suffix}", nn.Parameter(torch.empty(gh, hidden_size)))
            self.register_parameter(f"bias_ih_l0{suffix}", nn.Parameter(torch.empty(gh)))
            self.register_parameter(f"bias_hh_l0{suffix}", nn.Parameter(torch.empty(gh)))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -stdv, stdv)

    def forward(self, net: Tensor) -> Tensor:
        if net.dim() != 3 or net.shape[-1] != self.input_size:
            raise ValueError(f"{self.cell_name}: [B, T, {self.input_size}] expected, got {tuple(net.shape)}")
        if not net.is_cuda:
            raise RuntimeError(f"{self.cell_name}: the input must live on the HIP device (got {net.device}); there is no CPU path")
        args = []
        two_words = self.two_word_input and net.dtype == torch.float32
        for suffix in ("", "_reverse") if self.bidirectional else ("",):
            w_ih, b_ih = getattr(self, f"weight_ih_l0{suffix}"), getattr(self, f"bias_ih_l0{suffix}")
            gx = InputProjFn.apply(net, w_ih, b_ih) if two_words else HF.linear(net, w_ih, b_ih, out_f32=True)
            args += [gx, getattr(self, f"weight_hh_l0{suffix}"), getattr(self, f"bias_hh_l0{suffix}")]
        return recurrence(CELL_IDS[self.cell_name], *args)


class GRU(_RecurrentLayer):
    """nn.GRU(input_size, hidden_size, batch_first=True, bidirectional=...), one layer, zero initial state; returns the hidden
    sequence f32 [B, T, D H] (the reference drops the final state, modules/ml/rnn.py:84)"""

    cell_name, gate_count = "GRU", 3


class LSTM(_RecurrentLayer):
    """nn.LSTM(input_size, hidden_size, batch_first=True, bidirectional=...), one layer, zero initial states"""

    cell_name, gate_count = "LSTM", 4


def tanh_cell_refusal(*_: Any, **__: Any) -> Tuple[()]:
    raise NotImplementedError("cell = 'RNN': the tanh cell is not built (DESIGN §8); 'GRU' and 'LSTM' are")


# the reference's rnn_dict (modules/ml/rnn.py:13-17): an unknown name is a KeyError from this lookup, as there
rnn_dict = {"LSTM": LSTM, "GRU": GRU, "RNN": tanh_cell_refusal}
