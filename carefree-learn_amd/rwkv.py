"""RWKV token and channel mixers on the kernels of csrc/rwkv.hip: the autograd Functions behind `modules.RWKVTokenMixer` and
`modules.RWKVChannelMixer` (reference mixed_stacks/token_mixers.py:107-206, mixed_stacks/channel_mixers.py:69-113).

`TimeMixFn` is the time shift and the two or three mixes in one launch (bf16 rows for the GEMMs) together with the projections those
rows feed (f32 out); its backward is the dX / dW GEMMs, then one launch for dx and the per-workgroup partials of the mix gradients
plus one fixed-order reduce.  `WkvFn` is the WKV scan, y leaving as bf16 rows, and on top of it the token mixer's `output` layer with
the residual in its GEMM's epilogue; with gradients enabled the forward saves the two f32 scan states a and b, under torch.no_grad()
the scan allocates nothing but y.  `SquaredReluFn` (with the channel mixer's `value` layer on top) and `GateFn` are its elementwise steps.  The projections sit inside the two Functions because autograd casts a Function's input gradient to that input's
dtype: between separate nodes the gradients around the bf16 rows would be rounded to bf16 a second time.

Every parameter gradient of this file (the mixes, info_decay) is claimed through `functional.param_grad`; a parameter with
requires_grad = False gets a null destination: nothing is computed or reduced for it."""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from . import functional as HF
from . import ops


def _bf16_rows(d: Tensor) -> Tensor:
    """a gradient as contiguous bf16 (what the GEMMs' dX is already)"""
    if d.dtype != torch.bfloat16:
        d = ops.to_bf16(d.float().contiguous())
    return d if d.is_contiguous() else d.contiguous()


def _activation(x: Tensor) -> Tensor:
    xd = x.detach()
    if xd.dtype not in (torch.float32, torch.bfloat16):
        xd = xd.float()
    return xd if xd.is_contiguous() else xd.contiguous()


class TimeMixFn(Function):
    """The time shift, the mixes and the projections they feed: (k, v, r) or, with `mv` / `wv` None, (k, r), f32 [B, T, N_j] =
    (x * m_j + shift(x) * (1 - m_j)) W_j^T; replaces token_mixers.py:179-186, 201 / channel_mixers.py:107-110, 113.  The mixes are the
    [1, 1, C] parameters, the weights the [N_j, C] ones of the bias-free Linear layers.  One launch writes the mixed rows in bf16, one
    GEMM per projection (f32 out).  The projections sit inside this Function so that their input gradients reach the time-mix backward
    in f32: autograd would cast them to the dtype of the bf16 rows, and the LayerNorm backward behind the mixer rounds their sum to
    bf16 anyway, one rounding on that path instead of two.  dW_j = d_j^T rows_j goes through `functional.linear_param_grads`, the
    mix gradients through one launch with every claim nested (`functional.grads_in_one_launch`)."""

    NAMES = ("dmk", "dmv", "dmr")

    @staticmethod
    def forward(ctx: Any, x: Tensor, mk: Tensor, mv: Optional[Tensor], mr: Tensor, wk: Tensor, wv: Optional[Tensor], wr: Tensor):  # type: ignore
        xd = _activation(x)
        flat = [None if m is None else m.detach().reshape(-1) for m in (mk, mv, mr)]
        rows = ops.rwkv_time_mix(xd, flat[0], flat[1], flat[2])
        weights = [w for w in (wk, wv, wr) if w is not None]
        w16s = [HF.shadow_bf16(w) for w in weights]
        c = xd.shape[-1]
        outs = tuple(ops.gemm(r.view(-1, c), w16, out_dtype=torch.float32).view(*xd.shape[:-1], w16.shape[0]) for r, w16 in zip(rows, w16s))
        ctx.mixes, ctx.weights = (mk, mv, mr), weights
        ctx.save_for_backward(xd, *rows, *w16s)
        return outs

    @staticmethod
    def backward(ctx: Any, *douts: Tensor):  # type: ignore
        xd, *rest = ctx.saved_tensors
        n = len(rest) // 2
        rows, w16s = rest[:n], rest[n:]
        mk, mv, mr = ctx.mixes
        c = xd.shape[-1]
        want = {name: p for name, p in zip(TimeMixFn.NAMES, ctx.mixes) if p is not None and p.requires_grad}
        want_dx = ctx.needs_input_grad[0]
        ds: List[Optional[Tensor]] = []
        gws: List[Optional[Tensor]] = []
        for dout, row, w16, w in zip(douts, rows, w16s, ctx.weights):
            d2 = _bf16_rows(dout).view(-1, w16.shape[0])
            ds.append(ops.gemm(d2, w16, b_trans=True, out_dtype=torch.float32).view(xd.shape) if (want or want_dx) else None)
            gws.append(HF.linear_param_grads(d2, row.view(-1, c), w, None)[0] if w.requires_grad else None)
        flat = [None if m is None else m.detach().reshape(-1) for m in ctx.mixes]
        dx: List[Optional[Tensor]] = [None]

        def launch(dests: Dict[str, Tensor], accumulate: Sequence[str]) -> None:
            dx[0] = ops.rwkv_time_mix_grad(ds[0], ds[1] if n == 3 else None, ds[-1], xd, flat[0], flat[1], flat[2],
                                           dests={k: d.view(-1) for k, d in dests.items()}, accumulate=accumulate, want_dx=want_dx)

        grads = HF.grads_in_one_launch(want, launch) if (want or want_dx) else {}
        gw = iter(gws)
        gwk, gwv, gwr = next(gw), (next(gw) if n == 3 else None), next(gw)
        return (dx[0], *(grads.get(name) for name in TimeMixFn.NAMES), gwk, gwv, gwr)


def time_mix(x: Tensor, mk: Tensor, mv: Optional[Tensor], mr: Tensor, wk: Tensor, wv: Optional[Tensor], wr: Tensor) -> Tuple[Tensor, ...]:
    return TimeMixFn.apply(x, mk, mv, mr, wk, wv, wr)


class WkvFn(Function):
    """y bf16 [B, T, L] = sigmoid(r) * wkv, replacing token_mixers.py:184-203, and, given `w_out`, the `output` layer on top of it
    (token_mixers.py:205): y W_out^T with `residual` added in the GEMM's epilogue (the result has the residual's dtype, bf16 without
    one).  The output layer sits inside this Function for the reason given in `TimeMixFn`: its input gradient, the scan's dy, stays
    f32, and the residual's gradient is handed on unrounded.  `info_decay` is the [L, 1] parameter; `save`: keep the scan states for a
    backward (decided by `wkv` below, outside the Function, where grad mode is visible)."""

    @staticmethod
    def forward(ctx: Any, save: bool, k: Tensor, v: Tensor, r: Tensor, info_decay: Tensor, w_out: Optional[Tensor],
                residual: Optional[Tensor]) -> Tensor:
        kd, vd, rd = (t.detach().float().contiguous() for t in (k, v, r))
        decay = info_decay.detach().reshape(-1)
        ctx.info_decay, ctx.saved_any, ctx.w_out = info_decay, save, w_out
        if save:
            y, sa, sb = ops.rwkv_wkv(kd, vd, rd, decay, save=True)
        else:
            y = ops.rwkv_wkv(kd, vd, rd, decay)
        if w_out is None:
            out = y
        else:
            w16 = HF.shadow_bf16(w_out)
            y2 = y.view(-1, y.shape[-1])
            if residual is None:
                out = ops.gemm(y2, w16)
            else:
                r2 = _activation(residual).view(-1, w16.shape[0])
                out = ops.gemm(y2, w16, epilogue=ops.EPI_RESIDUAL, aux_in=r2, out_dtype=r2.dtype)
            out = out.view(*y.shape[:-1], w16.shape[0])
        if save:
            ctx.save_for_backward(kd, vd, rd, sa, sb, *(() if w_out is None else (y, w16)))
        return out

    @staticmethod
    def backward(ctx: Any, d: Tensor):  # type: ignore
        if not ctx.saved_any:
            raise RuntimeError("WkvFn: this forward ran without saving its scan states")
        kd, vd, rd, sa, sb, *proj = ctx.saved_tensors
        info_decay, w_out = ctx.info_decay, ctx.w_out
        need = ctx.needs_input_grad
        decay = info_decay.detach().reshape(-1)
        gw = None
        if proj:
            y, w16 = proj
            d2 = _bf16_rows(d).view(-1, w16.shape[0])
            dy = ops.gemm(d2, w16, b_trans=True, out_dtype=torch.float32).view(y.shape)
            if w_out.requires_grad:
                gw = HF.linear_param_grads(d2, y.view(-1, y.shape[-1]), w_out, None)[0]
        else:
            dy = _activation(d)
        out: List[Any] = [None]
        if info_decay.requires_grad:
            def compute(dst: Tensor, acc: bool) -> None:
                out[0] = ops.rwkv_wkv_grad(dy, kd, vd, rd, decay, sa, sb, d_decay=dst.view(-1), accumulate=acc)

            gd = HF.param_grad(info_decay, compute)
        else:
            gd = None
            if any(need[1:4]):
                out[0] = ops.rwkv_wkv_grad(dy, kd, vd, rd, decay, sa, sb)
        dk, dv, dr = out[0] if out[0] is not None else (None, None, None)
        return None, dk if need[1] else None, dv if need[2] else None, dr if need[3] else None, gd, gw, d if need[6] else None


def wkv(k: Tensor, v: Tensor, r: Tensor, info_decay: Tensor, w_out: Optional[Tensor] = None, residual: Optional[Tensor] = None) -> Tensor:
    tensors = (k, v, r, info_decay, w_out, residual)
    save = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
    return WkvFn.apply(save, *tensors)


class SquaredReluFn(Function):
    """bf16 relu(h)^2, replacing channel_mixers.py:111, and, given `w_value`, the `value` layer on top of it (channel_mixers.py:112):
    f32 relu(h)^2 W_value^T.  Inside one Function the layer's input gradient reaches the relu^2 backward in f32 (see `TimeMixFn`)."""

    @staticmethod
    def forward(ctx: Any, h: Tensor, w_value: Optional[Tensor]) -> Tensor:
        hd = _activation(h)
        kk = ops.rwkv_relu2(hd)
        ctx.w_value = w_value
        if w_value is None:
            ctx.save_for_backward(hd)
            return kk
        w16 = HF.shadow_bf16(w_value)
        ctx.save_for_backward(hd, kk, w16)
        return ops.gemm(kk.view(-1, kk.shape[-1]), w16, out_dtype=torch.float32).view(*kk.shape[:-1], w16.shape[0])

    @staticmethod
    def backward(ctx: Any, d: Tensor):  # type: ignore
        w_value = ctx.w_value
        if w_value is None:
            (hd,) = ctx.saved_tensors
            return ops.rwkv_relu2_grad(_activation(d), hd), None
        hd, kk, w16 = ctx.saved_tensors
        d2 = _bf16_rows(d).view(-1, w16.shape[0])
        gw = HF.linear_param_grads(d2, kk.view(-1, kk.shape[-1]), w_value, None)[0] if w_value.requires_grad else None
        dh = None
        if ctx.needs_input_grad[0]:
            dh = ops.rwkv_relu2_grad(ops.gemm(d2, w16, b_trans=True, out_dtype=torch.float32).view(hd.shape), hd)
        return dh, gw


def squared_relu(h: Tensor, w_value: Optional[Tensor] = None) -> Tensor:
    return SquaredReluFn.apply(h, w_value)


class GateFn(Function):
    """sigmoid(r) * kv (+ residual) from the f32 outputs of the receptance and value GEMMs; replaces channel_mixers.py:113 and the
    block's residual add.  The result has the residual's dtype, bf16 without one."""

    @staticmethod
    def forward(ctx: Any, r: Tensor, kv: Tensor, residual: Optional[Tensor]) -> Tensor:
        rd, kd = (t.detach().float().contiguous() for t in (r, kv))
        res = None if residual is None else _activation(residual)
        ctx.save_for_backward(rd, kd)
        return ops.rwkv_gate(rd, kd, res)

    @staticmethod
    def backward(ctx: Any, d: Tensor):  # type: ignore
        rd, kd = ctx.saved_tensors
        dr = dkv = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dr, dkv = ops.rwkv_gate_grad(_activation(d), rd, kd)
        return dr, dkv, d if ctx.needs_input_grad[2] else None


def gate(r: Tensor, kv: Tensor, residual: Optional[Tensor] = None) -> Tensor:
    return GateFn.apply(r, kv, residual)


def check_input(net: Tensor, who: str, in_dim: int, num_tokens: Optional[int] = None) -> None:
    if net.dim() != 3 or net.shape[-1] != in_dim:
        raise ValueError(f"{who}: [B, T, {in_dim}] expected, got {tuple(net.shape)}")
    if num_tokens is not None and net.shape[1] != num_tokens:
        raise ValueError(f"{who}: built for num_tokens = {num_tokens}, got T = {net.shape[1]} (the reference's decay kernel has num_tokens taps: "
                         "its convolution fails on any other length)")
    if not net.is_cuda:
        raise RuntimeError(f"{who}: the input must live on the HIP device (got {net.device}); there is no CPU path")


def check_dims(who: str, in_dim: int, latent_dim: int) -> None:
    if in_dim % 8 != 0 or latent_dim % 8 != 0 or in_dim < 8 or latent_dim < 8:
        raise NotImplementedError(f"{who}: in_dim = {in_dim}, latent_dim = {latent_dim}: both must be multiples of 8 (the bf16 rows of the "
                                  "GEMMs; DESIGN §8)")
