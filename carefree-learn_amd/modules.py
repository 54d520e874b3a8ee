"""Drop-in `nn.Module`s mirroring `cflearn.modules` for the ViT training path.

Same constructor keywords, attribute names and state_dict keys as the reference classes (cited per
class), so reference checkpoints load and `build_module(name, config=...)` configs are unchanged;
the arithmetic runs on the HIP kernels through `functional` / `fused`.  Features of the reference
classes that are outside the hot path (pruners, style-modulated convs, spatial reduction, custom
softmax callbacks...) raise NotImplementedError instead of silently doing something else.
"""
import math
import os
import sys
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.nn import Module

from . import functional as HF
from . import fused
from . import ops
from . import tome as _tome
from . import rnn as _rnn
from . import nbm as _nbm
from . import rwkv as _rwkv
from .registry import (
    attentions,
    build_module,
    channel_mixers,
    decoders,
    encoders,
    generators,
    register_module,
    safe_execute,
    shallow_copy_dict,
    token_mixers,
    update_dict,
)

LATENT_KEY = "latent"  # reference constants.py:3-7
PREDICTIONS_KEY = "predictions"


class Lambda(Module):
    """reference modules/common.py:89-100"""

    def __init__(self, fn: Callable, name: Optional[str] = None):
        super().__init__()
        self.name, self.fn = name, fn

    def extra_repr(self) -> str:
        return "" if self.name is None else self.name

    def forward(self, *args: Any, **kwargs: Any) -> Any:
        return self.fn(*args, **kwargs)


# ---------------------------------------------------------------------------------------------
# Linear family
# ---------------------------------------------------------------------------------------------


class Pruner(Module):
    """reference modules/core/customs.py:317-413: a soft mask on a WEIGHT matrix, `w * mask(|w|)` — parameter-sized element-wise math
    in front of `F.linear`, so it runs as torch ops on the fp32 parameter (autograd carries the gradients to the weight and, for
    `auto_prune`, to the four learnable scalars); the product with the activations stays on the HIP GEMM.  State keys as in the
    reference (`alpha`, `beta`, `gamma`, `max_ratio`, `eps`, `exp`, `mask`, depending on the method).

      simplified      mask = m(min(max_ratio, beta |w|^exp))
      hard / soft /   mask = m(min(max_ratio, beta log max(eps, |w| / (gamma mean|w|))))     with m(t) = max(alpha / beta t, t)
      auto_prune      (auto_prune: the four scalars are parameters, stored through an inverse softplus and read through softplus)
      surgery         mask = the `mask` buffer (the reference's threshold updates use the out-of-place `masked_fill` and drop its
                      result, customs.py:386-387: the buffer stays all ones — mirrored)"""

    _DEFAULTS = {
        "surgery": dict(alpha=1.0, beta=4.0, gamma=1.0e-4, eps=1.0e-12),
        "simplified": dict(alpha=0.01, beta=1.0, max_ratio=1.0, exp=0.5),
        "hard_prune": dict(alpha=1.0e-4, beta=1.0, gamma=1.0, max_ratio=1.0, eps=1.0e-12),
        None: dict(alpha=1.0e-2, beta=1.0, gamma=1.0, max_ratio=1.0, eps=1.0e-12),  # auto_prune and every other name
    }

    def __init__(self, config: Dict[str, Any], w_shape: Optional[List[int]] = None):
        super().__init__()
        self.method = config.setdefault("method", "auto_prune")
        table = self._DEFAULTS.get(self.method, self._DEFAULTS[None])
        if self.method == "surgery":
            if w_shape is None:
                raise ValueError("`w_shape` of `Pruner` should be provided when `surgery` is used")
            self.register_buffer("mask", torch.ones(*w_shape, dtype=torch.float32))
        values = {k: torch.tensor([config.setdefault(k, v)], dtype=torch.float32) for k, v in table.items()}
        if self.method not in ("surgery", "simplified"):
            if not all(float(values[k]) > 0 for k in ("alpha", "beta", "gamma", "max_ratio")):
                raise ValueError("parameters should greater than 0. in pruner")
        learnable = ("alpha", "beta", "gamma", "max_ratio") if self.method == "auto_prune" else ()
        for k, v in values.items():
            if k in learnable:
                setattr(self, k, nn.Parameter(torch.log(torch.exp(v) - 1)))  # softplus^-1
            else:
                self.register_buffer(k, v)
        self._repr_keys = list(table)

    def _scalar(self, name: str) -> Tensor:
        v = getattr(self, name)
        return torch.nn.functional.softplus(v) if self.method == "auto_prune" else v

    def forward(self, w: Tensor) -> Tensor:
        if self.method == "surgery":
            return w * self.mask
        w_abs = w.abs()
        alpha, beta, ratio = self._scalar("alpha"), self._scalar("beta"), self._scalar("max_ratio")
        if self.method == "simplified":
            t = torch.min(ratio, beta * w_abs.pow(self.exp))
        else:
            t = torch.log(torch.max(self.eps, w_abs / (w_abs.mean() * self._scalar("gamma"))))
            t = torch.min(ratio, beta * t)
        return w * torch.max(alpha / beta * t, t)

    def extra_repr(self) -> str:
        if self.method == "auto_prune":
            return f"method='{self.method}'"
        return f"method='{self.method}', " + ", ".join(f"{k}={getattr(self, k).item():g}" for k in self._repr_keys)


class Linear(Module):
    """reference modules/core/customs.py:23-114 — state keys `linear.weight`, `linear.bias`
    (or `w1`, `w2`, `b` for the low-rank form; `pruner.*` / `pruner1.*` / `pruner2.*` with `pruner_config`)."""

    def __init__(self, in_dim: int, out_dim: int, *, bias: bool = True,
                 pruner_config: Optional[Dict[str, Any]] = None, init_method: Optional[str] = None,
                 rank: Optional[int] = None, rank_ratio: Optional[float] = None, hook: Any = None):
        super().__init__()
        full_rank = min(in_dim, out_dim)
        if rank is None and rank_ratio is not None:
            rank = round(full_rank * rank_ratio)
        if rank is None:
            self.w1 = self.w2 = self.b = None
            self.linear = nn.Linear(in_dim, out_dim, bias)
        else:
            self.w1 = nn.Parameter(torch.zeros(rank, in_dim))
            self.w2 = nn.Parameter(torch.zeros(out_dim, rank))
            self.b = nn.Parameter(torch.zeros(1, out_dim)) if bias else None
            self.linear = None
        self.pruner = self.pruner1 = self.pruner2 = None
        if pruner_config is not None:  # (round 5; customs.py:54-62)
            if rank is None:
                self.pruner = Pruner(pruner_config, [out_dim, in_dim])
            else:
                self.pruner1 = Pruner(pruner_config, [rank, in_dim])
                self.pruner2 = Pruner(pruner_config, [out_dim, rank])
        init_fn = getattr(nn.init, f"{init_method or 'xavier_normal'}_", nn.init.xavier_normal_)
        self.init_weights_with(lambda t: init_fn(t, 1.0 / math.sqrt(2.0)))
        self.hook = hook
        self.out_f32 = False  # set by classifiers: emit fp32 logits straight from the GEMM epilogue

    @property
    def weight(self) -> Tensor:
        return self.linear.weight if self.linear is not None else torch.matmul(self.w2, self.w1)

    @property
    def bias(self) -> Optional[Tensor]:
        return self.b if self.linear is None else self.linear.bias

    def forward(self, net: Tensor, *, act: int = HF.ACT_NONE, residual: Optional[Tensor] = None) -> Tensor:
        inp = net
        if _native_lora(self.hook):
            return self.hook.linear_forward(self, net, act=act, residual=residual, out_f32=self.out_f32)
        if self.hook is not None:
            inp = self.hook.before_forward(inp)
        if self.linear is not None:
            weight = self.linear.weight if self.pruner is None else self.pruner(self.linear.weight)
            net = HF.linear(net, weight, self.linear.bias, act=act, residual=residual, out_f32=self.out_f32)
        else:
            w1 = self.w1 if self.pruner1 is None else self.pruner1(self.w1)
            w2 = self.w2 if self.pruner2 is None else self.pruner2(self.w2)
            net = HF.linear(net, w1, None)
            net = HF.linear(net, w2, self.b, act=act, residual=residual, out_f32=self.out_f32)
        if self.hook is not None:
            net = self.hook.after_forward(inp, net)
        return net

    def init_weights_with(self, w_init_fn: Callable[[Tensor], None]) -> None:
        with torch.no_grad():
            if self.linear is not None:
                w_init_fn(self.linear.weight.data)
                if self.linear.bias is not None:
                    self.linear.bias.data.zero_()
            else:
                w_init_fn(self.w1.data)
                w_init_fn(self.w2.data)
                if self.b is not None:
                    self.b.data.zero_()


class _HijackMixin:
    """reference hijacks.py:33-49: keeps ctor args for LoRA cloning, optional before/after hook."""

    def __init__(self, *args: Any, hook: Any = None, **kwargs: Any):
        self.args = args
        self.kwargs = shallow_copy_dict(kwargs)
        super().__init__(*args, **kwargs)
        self.hook = hook


class HijackLinear(_HijackMixin, nn.Linear):
    """reference hijacks.py:52-53 — state keys `weight`, `bias`."""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        inp = net
        if _native_lora(self.hook):
            return self.hook.linear_forward(self, net)
        if self.hook is not None:
            inp = self.hook.before_forward(inp)
        net = HF.linear(net, self.weight, self.bias)
        if self.hook is not None:
            net = self.hook.after_forward(inp, net)
        return net


class HijackCustomLinear(_HijackMixin, Linear):
    """reference hijacks.py:56-57 (the out_linear of Attention, the two layers of FeedForward)."""


# ---------------------------------------------------------------------------------------------
# LoRA adapters (reference modules/core/hijacks.py:82-206,300-470)
# ---------------------------------------------------------------------------------------------


def _native_lora(hook: Any) -> bool:
    """the layer's hook is this package's LoRALinearHook / LoRAConvHook in training mode: the adapter runs on the HIP path
    (HF.LoRALinearFn / HF.LoRAConv2dFn) instead of before_forward / the base op / after_forward; every other hook object takes the
    generic path"""
    return isinstance(hook, _LoRAMappingHook) and hook.training


def _hooked_linear(layer: Any, net: Tensor, *, residual: Optional[Tensor] = None, out_f32: bool = False) -> Tensor:
    """`HF.linear(net, layer.weight, layer.bias, ...)` of a Hijack layer whose `hook` is set, for the call sites that issue the GEMM
    themselves (a 1x1 HijackConv2d over token rows counts: its filter is the [Cout, Cin] matrix).  A native LoRA hook in training
    mode runs `linear_forward`; any other hook object gets before_forward / after_forward around the GEMM — in eval mode that is
    the weight injection, so the weight is read AFTER before_forward."""
    hook = layer.hook
    if _native_lora(hook):
        return hook.linear_forward(layer, net, residual=residual, out_f32=out_f32)
    inp = hook.before_forward(net)
    w = layer.weight
    out = HF.linear(inp, w.view(w.shape[0], -1), layer.bias, residual=residual, out_f32=out_f32)
    return hook.after_forward(inp, out)


def _weight_data_replaced(w: Tensor) -> None:
    """`w.data` was re-pointed (LoRA injection / clean-up).  The forward kernels read `functional.shadow_bf16(w)`, which is keyed on
    `w._version` — and an assignment to `.data` does not bump it.  (a) A parameter outside any arena: the cached copy would be
    served as is; dropping the version key makes the next forward cast again.  (b) A parameter of an `optim.ParamArena`: its shadow is
    a slice of the arena's bf16 buffer that only the optimizer kernel refreshes; with the key dropped `shadow_bf16` casts the
    current `.data` INTO that slice, and does so again after the clean-up has pointed `.data` back at the arena's master copy."""
    if hasattr(w, "_cfhip_shadow_version"):
        w._cfhip_shadow_version = None


class _LoRAMappingHook(Module):
    """what LoRALinearHook and LoRAConvHook share (reference hijacks.py:90-172, ILoRAHook + ILoRAMappingHook): the host-cached
    scale, weight injection and its clean-up"""

    backup: Optional[Tensor] = None
    injected: bool = False
    scale: float = 1.0

    @property
    def m(self) -> Any:
        return self._ms[0]

    # -- scale ------------------------------------------------------------------------------------
    def refresh_alpha(self) -> None:
        """re-read `alpha` on the host (one device read); call it after writing `alpha.data` by hand"""
        self._alpha_host = float(self.alpha.detach().float().cpu())
        self.injected = False

    @property
    def alpha_scale(self) -> float:
        return self._alpha_host / self.lora_down.weight.shape[0]

    @property
    def full_scale(self) -> float:
        return self.scale * self.alpha_scale

    def set_scale(self, scale: float) -> None:
        self.scale = scale
        self.refresh_alpha()

    def _load_from_state_dict(self, *args: Any, **kwargs: Any) -> None:
        super()._load_from_state_dict(*args, **kwargs)
        self.refresh_alpha()

    def inject(self, w: nn.Parameter, updown: Tensor, index: Optional[int] = None) -> None:
        if self.backup is None and (index is None or index == 0):
            self.backup = w.data
        w.data = (w.data if self.backup is None else self.backup) + updown
        _weight_data_replaced(w)
        self.injected = True

    def cleanup(self) -> None:
        if not self.injected:
            return
        self.injected = False
        if self.backup is not None:
            w = self.m.weight
            w.data = self.backup
            _weight_data_replaced(w)
            self.backup = None

    def before_forward(self, inp: Tensor, index: Optional[int] = None) -> Tensor:
        if self.training:
            self.cleanup()
        elif not self.injected:
            weight = self.m.weight
            self.to(weight)
            self.inject(weight, self.get_updown(), index)
        return inp


class LoRALinearHook(_LoRAMappingHook):
    """reference hijacks.py:90-206 (ILoRAHook + ILoRAMappingHook + LoRALinearHook): parameters `lora_down.weight` [rank, in],
    `lora_up.weight` [out, rank], `alpha` (a scalar); `normal_(std = 1 / rank)` / zeros / `scale` (0.1); dropout 0.1 on the low-rank
    term; optional diagonal `selector`.

    Training: `Linear` / `HijackLinear` call `linear_forward`, one `HF.LoRALinearFn` — base GEMM, `ops.lora_down`, `ops.lora_up_add`
    on the GEMM's output, then the activation: act(x W^T + b + s drop(up(down(x)))), the reference's order (hijacks.py:42-49,
    157-166).  s = `scale` * alpha / rank with alpha read on the host once per `set_scale` / `load_state_dict` / `refresh_alpha`
    (the reference calls `alpha.item()` in every forward, hijacks.py:129-131); like there, alpha gets no gradient.
    Eval: the reference's weight injection (hijacks.py:99-117,147-155), `weight.data = backup + s Bm A` with the product from
    `ops.gemm`, undone by `cleanup()` or by the next training-mode forward."""

    def __init__(self, in_features: int, out_features: int, *args: Any, rank: int = 4, dropout: float = 0.1,
                 scale: float = 0.1, **kwargs: Any) -> None:
        super().__init__()
        if rank > min(in_features, out_features):
            raise ValueError(f"LoRA rank {rank} must be less or equal than {min(in_features, out_features)}")
        if rank > ops.LORA_MAX_RANK:
            raise NotImplementedError(f"LoRA rank {rank}: the adapter kernels cover ranks up to {ops.LORA_MAX_RANK}")
        if kwargs.get("pruner_config") is not None:
            raise NotImplementedError("a LoRA adapter on a Linear with `pruner_config` is outside the accelerated hot path")
        if kwargs.get("rank_ratio") is not None:
            raise NotImplementedError("a LoRA adapter on a low-rank Linear (`rank=` / `rank_ratio=`) is outside the accelerated hot path")
        self.rank = rank
        self.lora_down = nn.Linear(in_features, rank, bias=False)
        self.selector: Module = nn.Identity()
        self.lora_up = nn.Linear(rank, out_features, bias=False)
        self.dropout = nn.Dropout(dropout)
        # a parameter for the state dict's sake, as in the reference; it never receives a gradient there (`alpha.item()`), so it is
        # marked frozen here: an arena / optimizer then leaves it alone (a zero gradient plus weight decay would move it away from
        # the host copy below)
        self.register_parameter("alpha", nn.Parameter(torch.tensor(scale), requires_grad=False))
        nn.init.normal_(self.lora_down.weight, std=1.0 / rank)
        nn.init.zeros_(self.lora_up.weight)
        self._alpha_host = float(scale)
        self._ms: List[Module] = []

    @classmethod
    def create_with(cls, m: Any, rank: int) -> "LoRALinearHook":
        if m.kwargs.get("rank") is not None:
            raise NotImplementedError("a LoRA adapter on a low-rank Linear (`rank=` / `rank_ratio=`) is outside the accelerated hot path")
        self = cls(*m.args, rank=rank, **m.kwargs)
        self._ms = [m]
        return self

    def set_selector(self, diag: Tensor) -> None:
        assert diag.shape == (self.rank,)
        self.selector = nn.Linear(self.rank, self.rank, bias=False)
        self.selector.weight.data = torch.diag(diag).to(self.lora_up.weight.data)

    def _down(self) -> Tensor:
        """lora_down.weight with the diagonal selector folded in: diag(d) (A x) = (diag(d) A) x — [rank, in] element-wise work on the host side"""
        a = self.lora_down.weight
        if isinstance(self.selector, nn.Identity):
            return a
        return torch.diagonal(self.selector.weight).unsqueeze(1) * a

    # -- training: the native path ------------------------------------------------------------------
    def linear_forward(self, layer: Any, net: Tensor, *, act: int = HF.ACT_NONE, residual: Optional[Tensor] = None,
                       out_f32: bool = False) -> Tensor:
        self.cleanup()
        inner = getattr(layer, "linear", layer)  # the project's Linear keeps an nn.Linear; HijackLinear is one
        if inner is None or getattr(layer, "pruner", None) is not None:
            raise NotImplementedError("a LoRA adapter on a low-rank or pruned Linear is outside the accelerated hot path")
        # The reference runs the hook of a HijackCustomLinear TWICE per training forward: IBasicHijackMixin.forward (hijacks.py:42-49)
        # wraps customs.Linear.forward (customs.py:81-100), and both read the same `self.hook` — base + 2 s up(down(x)), while the
        # eval-mode injection adds s Bm A once.  Mirrored (adapters trained there were trained under it; tests/golden/lora_linear.pt
        # records it) as one launch at twice the scale; with dropout the reference draws two masks, here the one mask counts twice
        # (the same expectation).
        times = 2.0 if isinstance(layer, HijackCustomLinear) else 1.0
        return HF.lora_linear(net, inner.weight, inner.bias, self._down(), self.lora_up.weight, times * self.full_scale,
                              self.dropout.p, act=act, residual=residual, out_f32=out_f32)

    # -- eval: weight injection ---------------------------------------------------------------------
    def get_updown(self) -> Tensor:
        """s Bm A as f32 [out, in], the product on `ops.gemm` (bf16 factors — what the training path multiplies with —, f32
        accumulation; the rank is zero-padded to the GEMM's multiple of 8 in two rank-sized temporaries)"""
        up, down = self.lora_up.weight.detach(), self._down().detach()
        r8 = (self.rank + 7) // 8 * 8
        up16 = torch.zeros((up.shape[0], r8), dtype=torch.bfloat16, device=up.device)
        down16 = torch.zeros((r8, down.shape[1]), dtype=torch.bfloat16, device=up.device)
        up16[:, :self.rank] = up
        down16[:self.rank] = down
        return ops.gemm(up16, down16, b_trans=True, out_dtype=torch.float32) * self.full_scale

    def after_forward(self, inp: Tensor, out: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("LoRALinearHook in training mode runs through `linear_forward` (HF.LoRALinearFn); the layer it is attached "
                               "to does not know that path — attach it to Linear / HijackLinear / HijackCustomLinear")
        return out


def _square(v: Any, what: str) -> int:
    if isinstance(v, (tuple, list)):
        if len(set(v)) != 1:
            raise NotImplementedError(f"LoRAConvHook: {what} {tuple(v)} is not square")
        v = v[0]
    if not isinstance(v, int):
        raise NotImplementedError(f"LoRAConvHook: {what} {v!r} is outside the accelerated hot path")
    return v


class LoRAConvHook(_LoRAMappingHook):
    """reference hijacks.py:208-266 (ILoRAHook + ILoRAMappingHook + LoRAConvHook): the reference's constructor signature,
    parameters `lora_down.weight` [rank, Cin, k, k] (a k x k convolution with the base layer's stride and padding),
    `lora_up.weight` [Cout, rank, 1, 1], `alpha` (a scalar, frozen, read on the host once per `set_scale` / `load_state_dict` /
    `refresh_alpha`); `normal_(std = 1 / rank)` / zeros / `scale` (0.1); dropout 0.1 on the low-rank term; optional diagonal
    `selector`.

    Geometry on the hot path: square kernel, groups 1, zero padding, dilation 1, (kernel, padding) in {(1, 0), (3, 1)}, stride 1
    (1x1) or 1 / 2 (3x3), Cin % 8 == Cout % 8 == 0, rank <= ops.LORA_MAX_RANK; anything else raises NotImplementedError here.

    Training: `HijackConv2d.forward` calls `conv_forward`, one `HF.LoRAConv2dFn` around the base convolution:
    conv(x, W) + b + s drop(up(down(x))).  A 1x1 layer whose owner runs it as a GEMM over token rows (SpatialTransformer's
    `to_latent` / `from_latent`) calls `linear_forward`, the Linear adapter's `HF.LoRALinearFn` on the same factors.
    Eval: weight injection with the EXACT merged filter, `weight.data = backup + s sum_c up[o][c] down[c][i][ky][kx]`, so that the
    injected layer computes what the training forward computes (without dropout).  For 1x1 that is the reference's `get_updown`.
    For 3x3 the reference (hijacks.py:143) multiplies `up[..., 0, 0] @ down[..., 0, 0]` — tap [0, 0] of `lora_down` only — and
    broadcasts the product over all nine taps, which is 4.6e-2 .. 0.38 rel-L2 away from its OWN training-mode output on the cases
    of tests/golden/lora_conv.pt; that formula is deliberately not mirrored."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: Any, stride: Any = 1, padding: Any = 0, dilation: Any = 1,
                 groups: int = 1, *args: Any, rank: int = 4, dropout: float = 0.1, scale: float = 0.1, **kwargs: Any) -> None:
        super().__init__()
        if rank > ops.LORA_MAX_RANK:
            raise NotImplementedError(f"LoRA rank {rank}: the adapter kernels cover ranks up to {ops.LORA_MAX_RANK}")
        k, st, pad, dil = (_square(v, n) for v, n in ((kernel_size, "kernel"), (stride, "stride"), (padding, "padding"), (dilation, "dilation")))
        if groups != 1 or dil != 1 or kwargs.get("padding_mode", "zeros") != "zeros":
            raise NotImplementedError("LoRAConvHook: grouped, dilated or non-zero-padded convolutions are outside the adapter kernels")
        if (k, pad) not in ((1, 0), (3, 1)) or st not in ((1,) if k == 1 else (1, 2)):
            raise NotImplementedError(f"LoRAConvHook: kernel {k} / padding {pad} / stride {st}: the adapter kernels cover 1x1 (padding 0, "
                                      "stride 1) and 3x3 (padding 1, stride 1 or 2)")
        if in_channels % 8 != 0 or out_channels % 8 != 0:
            raise NotImplementedError(f"LoRAConvHook: {in_channels} -> {out_channels} channels: the adapter kernels need multiples of 8")
        if rank > min(in_channels, out_channels):
            raise ValueError(f"LoRA rank {rank} must be less or equal than {min(in_channels, out_channels)}")
        self.rank = rank
        self.lora_down = nn.Conv2d(in_channels, rank, k, stride=st, padding=pad, bias=False)
        self.selector: Module = nn.Identity()
        self.lora_up = nn.Conv2d(rank, out_channels, 1, bias=False)
        self.dropout = nn.Dropout(dropout)
        # frozen for the reasons given in LoRALinearHook
        self.register_parameter("alpha", nn.Parameter(torch.tensor(scale), requires_grad=False))
        nn.init.normal_(self.lora_down.weight, std=1.0 / rank)
        nn.init.zeros_(self.lora_up.weight)
        self._alpha_host = float(scale)
        self._ms: List[Module] = []

    @classmethod
    def create_with(cls, m: Any, rank: int) -> "LoRAConvHook":
        self = cls(*m.args, rank=rank, **m.kwargs)
        self._ms = [m]
        return self

    def set_selector(self, diag: Tensor) -> None:
        assert diag.shape == (self.rank,)
        self.selector = nn.Conv2d(self.rank, self.rank, 1, bias=False)
        self.selector.weight.data = torch.diag(diag).to(self.lora_up.weight.data).view(self.rank, self.rank, 1, 1)

    def _down(self) -> Tensor:
        """lora_down.weight with the diagonal selector folded in (see LoRALinearHook._down)"""
        a = self.lora_down.weight
        if isinstance(self.selector, nn.Identity):
            return a
        return torch.diagonal(self.selector.weight.view(self.rank, self.rank)).view(-1, 1, 1, 1) * a

    # -- training: the native path ------------------------------------------------------------------
    def conv_forward(self, layer: Any, net: Tensor) -> Tensor:
        self.cleanup()
        return HF.lora_conv2d(net, layer.weight, layer.bias, layer.stride[0], layer.padding[0], layer.dilation[0], self._down(),
                              self.lora_up.weight, self.full_scale, self.dropout.p)

    def linear_forward(self, layer: Any, net: Tensor, *, act: int = HF.ACT_NONE, residual: Optional[Tensor] = None,
                       out_f32: bool = False) -> Tensor:
        """a 1x1 layer applied to token rows [..., Cin] as the GEMM it is"""
        self.cleanup()
        if self.lora_down.kernel_size != (1, 1):
            raise NotImplementedError("LoRAConvHook.linear_forward: only a 1x1 convolution is a Linear over token rows")
        w = layer.weight
        return HF.lora_linear(net, w.view(w.shape[0], -1), layer.bias, self._down(), self.lora_up.weight, self.full_scale,
                              self.dropout.p, act=act, residual=residual, out_f32=out_f32)

    # -- eval: weight injection ---------------------------------------------------------------------
    def get_updown(self) -> Tensor:
        """s * sum_c up[o][c] down[c][i][ky][kx] as f32 [Cout, Cin, k, k]: one `ops.gemm` over the [rank, Cin k k] matrix of
        `lora_down` (bf16 factors — what the training path multiplies with —, f32 accumulation, the rank zero-padded to 8)"""
        up, down = self.lora_up.weight.detach(), self._down().detach()
        r8 = (self.rank + 7) // 8 * 8
        up16 = torch.zeros((up.shape[0], r8), dtype=torch.bfloat16, device=up.device)
        down16 = torch.zeros((r8, down[0].numel()), dtype=torch.bfloat16, device=up.device)
        up16[:, :self.rank] = up.view(up.shape[0], self.rank)
        down16[:self.rank] = down.reshape(self.rank, -1)
        return (ops.gemm(up16, down16, b_trans=True, out_dtype=torch.float32) * self.full_scale).view(up.shape[0], *down.shape[1:])

    def after_forward(self, inp: Tensor, out: Tensor) -> Tensor:
        if self.training:
            raise RuntimeError("LoRAConvHook in training mode runs through `conv_forward` (HF.LoRAConv2dFn); the layer it is attached "
                               "to does not know that path — attach it to HijackConv2d")
        return out


class LoRAAttentionHook(Module):
    """reference hijacks.py:269-297 (inference-time injection into `in_w` only) — not on the accelerated hot path"""

    def __init__(self, *args: Any, **kwargs: Any) -> None:
        raise NotImplementedError("LoRAAttentionHook: the packed-projection adapter is inference-time injection only in the reference and "
                                  "outside the accelerated hot path; adapt the block's Linear layers")


class LoRAPack(NamedTuple):
    """reference hijacks.py:300-302"""

    rank: int
    hooks: Dict[str, _LoRAMappingHook]


class LoRAManager:
    """reference hijacks.py:305-470: `prepare` builds one LoRALinearHook per Hijack(Custom)Linear and one LoRAConvHook per
    HijackConv2d under `m` (or under the modules whose class name is in `target_ancestors`), `inject` attaches a pack's hooks,
    `cleanup` restores injected weights and detaches them.  Keys are the module names `inject` looks up (the reference joins prefix
    and name with a dot even when the prefix is empty and then never finds such keys again; here an empty part is left out).
    Convolutions whose geometry the adapter kernels do not cover (LoRAConvHook; the UNet's 3 / 4-channel stem and its 3-channel
    head) and `Attention.in_w` are outside the accelerated path: `prepare` leaves them alone and lists their names in `skipped`."""

    def __init__(self) -> None:
        self.m: Optional[Module] = None
        self.injected = False
        self.lora_packs: Dict[str, LoRAPack] = {}
        self.skipped: List[str] = []

    def has(self, key: str) -> bool:
        return key in self.lora_packs

    def build_pack(self, *keys: str) -> Optional[LoRAPack]:
        packs = [self.lora_packs[k] for k in keys if k in self.lora_packs]
        if not packs:
            return None
        if len(packs) == 1:
            return packs[0]
        ranks = {pack.rank for pack in packs}
        hooks: Dict[str, _LoRAMappingHook] = {}
        for pack in packs:
            for k, v in pack.hooks.items():
                if k in hooks:
                    raise NotImplementedError(f"two LoRA packs adapt '{k}': stacked adapters (MultiHooks) are outside the accelerated hot path")
                hooks[k] = v
        return LoRAPack(ranks.pop() if len(ranks) == 1 else -1, hooks)

    def load_pack_with(self, key: str, d: Dict[str, Tensor]) -> None:
        pack = self.lora_packs.get(key)
        if pack is None:
            raise ValueError(f"cannot find '{key}' pack")
        for k, v in pack.hooks.items():
            for n, p in v.named_parameters():
                tp = d[f"{k}.{n}"]
                assert p.data.shape == tp.shape
                p.data = tp.to(p.data)
            v.refresh_alpha()

    def prepare(self, m: Module, *, key: str, rank: int, target_ancestors: Optional[set] = None) -> None:
        self.lora_packs.pop(key, None)
        pack = LoRAPack(rank, {})
        self.m = m
        self.skipped = []
        if target_ancestors is None:
            self._prepare(m, "", pack)
        else:
            for name, module in m.named_modules():
                if module.__class__.__name__ in target_ancestors:
                    self._prepare(module, name, pack)
        self.lora_packs[key] = pack

    def inject(self, m: Module, *keys: str) -> None:
        if self.m is None:
            raise ValueError("LoRA is not prepared, please call `prepare` first.")
        if m is not self.m:
            raise ValueError("prepared module does not match the incoming module.")
        pack = self.build_pack(*keys)
        if pack is None:
            raise ValueError(f"cannot build LoRAPack with {', '.join(keys)}")
        pivot = next(iter(m.parameters()))
        num_injected = 0
        for name, module in m.named_modules():
            hook = pack.hooks.get(name)
            if hook is not None:
                if not isinstance(module, _HijackMixin):
                    raise ValueError(f"`hook` is found for '{name}' but it is not a Hijack module")
                hook.to(pivot)
                hook.train(module.training)
                module.hook = hook
                num_injected += 1
        if num_injected != len(pack.hooks):
            import warnings

            warnings.warn(f"only {num_injected}/{len(pack.hooks)} hooks are injected, which could lead to unexpected behaviours")
        self.injected = True

    def cleanup(self, m: Module) -> None:
        if not self.injected:
            raise ValueError("LoRA is not injected, please call `inject` first.")
        if m is not self.m:
            raise ValueError("injected module does not match the incoming module.")
        for module in m.modules():
            if isinstance(module, _HijackMixin) and isinstance(module.hook, _LoRAMappingHook):
                module.hook.cleanup()
                module.hook = None
        self.injected = False

    def set_scale(self, key: str, scale: float) -> None:
        pack = self.lora_packs.get(key)
        if pack is None:
            raise ValueError(f"cannot find LoRAPack '{key}'")
        for hook in pack.hooks.values():
            hook.set_scale(scale)

    def set_scales(self, scales: Dict[str, float]) -> None:
        for k, v in scales.items():
            self.set_scale(k, v)

    def _prepare(self, m: Module, prefix: str, pack: LoRAPack) -> None:
        for name, module in m.named_modules():
            key = ".".join(part for part in (prefix, name) if part)
            if isinstance(module, (HijackLinear, HijackCustomLinear)):
                pack.hooks[key] = LoRALinearHook.create_with(module, pack.rank)
            elif isinstance(module, HijackConv2d):
                try:
                    pack.hooks[key] = LoRAConvHook.create_with(module, pack.rank)
                except NotImplementedError:  # a geometry without adapter kernels: reported, not adapted
                    self.skipped.append(key)
            elif isinstance(module, (nn.Conv2d, Attention)) and hasattr(module, "hook"):
                self.skipped.append(key)


class LayerNorm(nn.LayerNorm):
    """`NormFactory("layer").make(dim)` (reference norms.py:88-89,118-119): nn.LayerNorm with
    eps defaulting to 1e-6; state keys `weight`, `bias`."""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if not self.elementwise_affine or len(self.normalized_shape) != 1:
            raise NotImplementedError("only affine LayerNorm over the last dim is on the hot path")
        return HF.layer_norm(net, self.weight, self.bias, self.eps, getattr(self, "out_f32", False))


class LN(LayerNorm):
    """`NormFactory("layer_norm").make(dim)` (reference norms.py:30-46, 84-85): nn.LayerNorm over the last dim for everything but a 4-D
    input with a 1-D `normalized_shape`, where it is the reference's own per-sample normalisation — ONE mean and one UNBIASED standard
    deviation over C*H*W, `(x - mean) / (std + eps)`, per-channel affine (`cfhip_layernorm4d_*`).  State keys `weight`, `bias`."""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if net.dim() != 4 or len(self.normalized_shape) != 1:
            return super().forward(net)
        if self.elementwise_affine:
            return HF.layer_norm_4d(net, self.weight, self.bias, self.eps)
        return HF.layer_norm_4d(net, None, None, self.eps)


class _BatchNormMixin:
    """nn.BatchNorm{1,2}d semantics (reference norms.py:20-27,90-93) on `cfhip_batchnorm_fwd/bwd`: training
    mode normalises with the batch statistics and updates running_mean / running_var (unbiased) /
    num_batches_tracked; eval mode uses the running statistics.  State keys are nn.BatchNorm's."""

    def _bn(self, net: Tensor) -> Tensor:
        if self.momentum is None:
            raise NotImplementedError("cumulative-average BatchNorm (momentum=None) is not built")
        training = self.training or not self.track_running_stats
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        rm = self.running_mean if self.track_running_stats else None
        rv = self.running_var if self.track_running_stats else None
        return HF.batch_norm(net, self.weight, self.bias, rm, rv, self.eps, self.momentum, training)


class BatchNorm2d(_BatchNormMixin, nn.BatchNorm2d):
    """`NormFactory("batch").make(dim)`: [B, C, H, W]"""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if net.dim() != 4:
            raise ValueError(f"expected 4D input (got {net.dim()}D input)")
        return self._bn(net)


class BatchNorm1d(_BatchNormMixin, nn.BatchNorm1d):
    """`NormFactory("batch1d")`: [B, C] or [B, C, L]"""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if net.dim() not in (2, 3):
            raise ValueError(f"expected 2D or 3D input (got {net.dim()}D input)")
        return self._bn(net)


class BN(BatchNorm1d):
    """reference norms.py:20-27: BatchNorm1d that takes token-major [B, T, C] by transposing"""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if net.dim() == 3:
            return super().forward(net.transpose(1, 2).contiguous()).transpose(1, 2)
        return super().forward(net)


class LeakyReLU(Module):
    """`build_activation("leaky_relu_0.2")` (reference activations.py:35-40)"""

    def __init__(self, negative_slope: float = 0.01, inplace: bool = True):
        super().__init__()
        self.negative_slope, self.inplace = negative_slope, inplace

    def extra_repr(self) -> str:
        return f"negative_slope={self.negative_slope}"

    def forward(self, net: Tensor) -> Tensor:
        return HF.leaky_relu(net, self.negative_slope)


class ReLU(LeakyReLU):
    """`build_activation("ReLU")` (reference activations.py:41-48)"""

    def __init__(self, inplace: bool = True):
        super().__init__(0.0, inplace)

    def extra_repr(self) -> str:
        return ""


def build_activation(name: Optional[str], config: Optional[Dict[str, Any]] = None) -> Module:
    """reference activations.py:27-53, restricted to the activations that have a HIP kernel"""
    if name is None:
        return nn.Identity()
    config = dict(config or {})
    if name.startswith("leaky_relu"):
        splits = name.split("_")
        if len(splits) == 3:
            config["negative_slope"] = float(splits[-1])
        return LeakyReLU(**config)
    if name.lower() == "relu":
        return ReLU(**config)
    if name == "sine":  # (reference activations.py:130-137; the kernel lives with the Siren's, csrc/siren.hip)
        from .siren import Sine

        return Sine(**config)
    raise NotImplementedError(f"activation '{name}' as a stand-alone module is not on the accelerated hot path")


class NormFactory:
    """reference norms.py:70-140 restricted to what the transformer path uses."""

    def __init__(self, norm_type: Optional[str]):
        self.norm_type = norm_type

    @property
    def use_bias(self) -> bool:
        return self.norm_type is None or not self.norm_type.startswith("batch")

    def make(self, *args: Any, **kwargs: Any) -> Module:
        if self.norm_type is None:
            return nn.Identity()
        if self.norm_type == "layer":
            kw = update_dict(kwargs, {"eps": 1.0e-6})
            return LayerNorm(*args, **kw)
        if self.norm_type == "layer_norm":
            kw = update_dict(kwargs, {"eps": 1.0e-6})
            return LN(*args, **kw)
        if self.norm_type == "batch":
            kw = update_dict(kwargs, {"affine": True, "track_running_stats": True})
            return BatchNorm2d(*args, **kw)
        if self.norm_type == "batch1d":
            return BatchNorm1d(*args, **kwargs)
        if self.norm_type == "batch_norm":
            return BN(*args, **kwargs)
        raise NotImplementedError(f"normalization '{self.norm_type}' is not on the accelerated hot path")

    def inject_to(self, dim: int, norm_kwargs: Dict[str, Any], current_blocks: List[Module],
                  *subsequent_blocks: Module) -> None:
        """reference norms.py:126-140 (the "spectral" wrapper form is not built)"""
        if self.norm_type is not None:
            current_blocks.append(self.make(dim, **norm_kwargs))
        else:
            current_blocks.append(nn.Identity())
        current_blocks.extend(subsequent_blocks)


# ---------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------


class AttentionOutput(NamedTuple):
    output: Tensor
    weights: Optional[Tensor]


def expand_module_mask(mask: Tensor, num_heads: int) -> Tensor:
    """Reference mask quirk (attentions.py:246-253): the [B, Tq, Tk] `True = zeroed` mask is
    `repeat(H,1,1).view(-1,H,Tq,Tk)`-ed, i.e. (b, h) uses mask[(b*H + h) % B].  Integer index
    arithmetic -> bit-exact.  Returns the uint8 KEEP mask [B, H, Tq, Tk]."""
    if mask.dim() == 2:  # [Tq, Tk] broadcast (causal masks of the text tower)
        return (~mask).to(torch.uint8)[None, None]
    b = mask.shape[0]
    idx = (torch.arange(b * num_heads, device=mask.device) % b).view(b, num_heads)
    return (~mask)[idx].to(torch.uint8)


@attentions.register("basic")
class Attention(Module):
    """reference modules/core/attentions.py:57-279.  Parameters: `in_w` [3D, Din] + `qkv_bias`
    (self attention), or `q_w` + `kv_w` / `q_w`,`k_w`,`v_w` with their biases; `out_linear`."""

    customize_sdp: bool = False

    def __init__(self, input_dim: int, num_heads: int = 1, *, bias: bool = True, dropout: float = 0.0,
                 qk_scale: Optional[float] = None, kv_same: Optional[bool] = None,
                 qkv_bias_same: bool = True, is_self_attention: bool = False, k_dim: Optional[int] = None,
                 v_dim: Optional[int] = None, embed_dim: Optional[int] = None,
                 activation: Optional[str] = None, activation_config: Optional[Dict[str, Any]] = None,
                 out_linear_config: Optional[Dict[str, Any]] = None, reduction_ratio: Optional[int] = None,
                 hook: Any = None):
        super().__init__()
        for what, hit in (("spatial `reduction_ratio`", reduction_ratio is not None and reduction_ratio > 1),
                          ("`activation` on q/k/v", activation is not None)):
            if hit:
                raise NotImplementedError(f"{what} is outside the accelerated hot path")
        # -- geometry.  The attribute names, the parameter names / shapes / initialisers and their REGISTRATION ORDER are the
        # reference's state_dict contract (attentions.py:57-147; tests/test_host_logic.py compares key for key); how they are
        # derived is this file's: one table of projection weights and one of biases per operand layout.
        self.input_dim, self.num_heads = input_dim, num_heads
        self.qkv_same = bool(is_self_attention)
        if self.qkv_same:
            for name, given in (("k_dim", k_dim), ("v_dim", v_dim)):
                if given not in (None, input_dim):
                    raise ValueError(f"self attention is used but `{name}` != `input_dim`")
            self.k_dim = self.v_dim = input_dim
        else:
            self.k_dim = k_dim or input_dim
            self.v_dim = v_dim or self.k_dim
        self.kv_same = (k_dim is None or v_dim is None or k_dim == v_dim) if kv_same is None else kv_same
        self.embed_dim = e = embed_dim or input_dim
        self.head_dim, rest = divmod(e, num_heads)
        if rest:
            raise ValueError("`embed_dim` must be divisible by `num_heads`")
        self.scaling = qk_scale or float(self.head_dim) ** 0.5

        def trunc(w: Tensor) -> None:
            nn.init.trunc_normal_(w, std=0.02)

        layout = "packed" if self.qkv_same else ("q+kv" if self.kv_same else "q,k,v")
        weights = {
            "packed": (("in_w", 3 * e, input_dim, trunc),),
            "q+kv": (("q_w", e, input_dim, trunc), ("kv_w", 2 * e, input_dim, trunc)),
            "q,k,v": (("q_w", e, input_dim, nn.init.xavier_uniform_), ("k_w", e, self.k_dim, nn.init.xavier_uniform_),
                      ("v_w", e, self.v_dim, nn.init.xavier_uniform_)),
        }[layout]
        if not bias:
            biases: tuple = ()
        elif not qkv_bias_same:
            biases = (("q_bias", e), ("k_bias", e), ("v_bias", e))
        elif layout == "q+kv":
            biases = (("q_bias", e), ("kv_bias", 2 * e))
        else:
            biases = (("qkv_bias", 3 * e),)
        for name in ("in_w", "q_w", "k_w", "v_w", "kv_w", "q_bias", "k_bias", "v_bias", "kv_bias", "qkv_bias"):
            setattr(self, name, None)
        for name, rows, cols, init in weights:
            w = nn.Parameter(torch.empty(rows, cols))
            init(w)
            setattr(self, name, w)
        for name, rows in biases:
            setattr(self, name, nn.Parameter(torch.zeros(rows)))
        self.out_linear = HijackCustomLinear(e, input_dim, **(out_linear_config or {}))
        self.dropout = dropout
        self.activation = nn.Identity()
        self.reduction = None
        self.hook = hook

    # -- reference hooks of the slow path (attentions.py:151-157); overriding them is refused in forward()
    def _get_weights(self, raw_weights: Tensor) -> Tensor:
        return torch.softmax(raw_weights, dim=-1)

    def _weights_callback(self, weights: Tensor) -> Tensor:
        return weights

    # -- projections --------------------------------------------------------------------------
    def _project(self, q: Tensor, k: Tensor, v: Tensor) -> Tuple[Optional[Tensor], Tensor, Tensor, Tensor]:
        """returns (packed qkv or None, q, k, v)"""
        e = self.embed_dim
        if self.qkv_same:
            qkv = HF.linear(q, self.in_w, self.qkv_bias)
            return qkv, qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:]
        if self.kv_same:
            qq = HF.linear(q, self.q_w, self.q_bias)
            kv = HF.linear(k, self.kv_w, self.kv_bias)
            return None, qq, kv[..., :e], kv[..., e:]
        if self.qkv_bias is not None:
            qb, kb, vb = self.qkv_bias.chunk(3)
        else:
            qb, kb, vb = self.q_bias, self.k_bias, self.v_bias
        return None, HF.linear(q, self.q_w, qb), HF.linear(k, self.k_w, kb), HF.linear(v, self.v_w, vb)

    def forward(self, q: Tensor, k: Tensor, v: Tensor, *, hw: Optional[Tuple[int, int]] = None,
                mask: Optional[Tensor] = None, require_weights: bool = False,
                deterministic: bool = False, residual: Optional[Tensor] = None) -> AttentionOutput:
        drop = self.dropout if (self.training and 0.0 < self.dropout < 1.0) else 0.0  # attentions.py:254: on the probabilities
        slow = require_weights or self.customize_sdp  # attentions.py:256-268: the weights are materialised and returned
        if slow:
            if type(self)._get_weights is not Attention._get_weights or type(self)._weights_callback is not Attention._weights_callback:
                raise NotImplementedError("a custom `_get_weights` / `_weights_callback` replaces the softmax the HIP kernels fuse")
        if self.head_dim % 8 != 0 or self.head_dim > 192:
            raise NotImplementedError(f"HIP attention kernels take head_dim = a multiple of 8 up to 192, got {self.head_dim}")
        qkv_inp = q, k, v
        if self.hook is not None:
            qkv_inp = self.hook.before_forward(qkv_inp)
        packed, qq, kk, vv = self._project(q, k, v)
        if self.hook is not None:
            qq, kk, vv = self.hook.after_forward(qkv_inp, (qq, kk, vv))
            packed = None
        keep = None if mask is None else expand_module_mask(mask, self.num_heads)
        if slow:
            if packed is not None:
                d = packed.shape[-1] // 3
                qq, kk, vv = packed[..., :d], packed[..., d:2 * d], packed[..., 2 * d:]
            # training dropout (attentions.py:263-264) acts on the weights that are returned AND multiply v: same Philox mask in both
            out, weights = HF.attention_with_weights(qq, kk, vv, self.num_heads, keep, False, self.head_dim, 1.0 / self.scaling, drop)
            return AttentionOutput(self.out_linear(out, residual=residual), weights)
        if self.head_dim != 64:
            # the general-head_dim kernels (`cfhip_attn_*_dh`, what CrossAttention uses) take separate q / k / v views
            if packed is not None:
                d = packed.shape[-1] // 3
                qq, kk, vv = packed[..., :d], packed[..., d:2 * d], packed[..., 2 * d:]
            out = HF.attention_core(qq, kk, vv, self.num_heads, keep, False, self.head_dim, drop)
        elif packed is not None:
            out = HF.packed_self_attention(packed, self.num_heads, keep, False, drop)
        else:
            out = HF.attention_core(qq, kk, vv, self.num_heads, keep, False, 64, drop)
        net = self.out_linear(out, residual=residual)
        return AttentionOutput(net, None)


# ---------------------------------------------------------------------------------------------
# mixers
# ---------------------------------------------------------------------------------------------


class Dropout(Module):
    """nn.Dropout on the HIP path (no parameters, same position in every `nn.Sequential` as the reference's, so
    state_dict keys are unchanged): Philox mask regenerated in backward (`functional.DropoutFn`), identity in eval
    mode or for p outside (0, 1).  `inject_mask` (uint8, 1 = keep; consumed by the next forward) pins the mask for
    parity tests — given the mask the result is bit-equal to torch's."""

    def __init__(self, p: float = 0.5, inplace: bool = False):
        super().__init__()
        self.p, self.inplace = float(p), inplace
        self.inject_mask: Optional[Tensor] = None

    def forward(self, net: Tensor) -> Tensor:
        mask, self.inject_mask = self.inject_mask, None
        return HF.dropout(net, self.p, self.training, mask)

    def extra_repr(self) -> str:
        return f"p={self.p}"


class DropPath(Module):
    """reference modules/core/customs.py:429-446: `net.div(keep) * floor(keep + U[0, 1))` per sample, training only.
    `inject_mask` (f32 [B] of 0 / 1; consumed by the next forward) pins the sample mask for parity tests."""

    def __init__(self, dropout: float = 0.0):
        super().__init__()
        self.dropout = dropout
        self.inject_mask: Optional[Tensor] = None

    def forward(self, net: Tensor) -> Tensor:
        mask, self.inject_mask = self.inject_mask, None
        return HF.drop_path(net, self.dropout, self.training, mask)

    def extra_repr(self) -> str:
        return str(self.dropout)


class ITokenMixer(Module):
    def __init__(self, in_dim: int, num_tokens: int):
        super().__init__()
        self.in_dim, self.num_tokens = in_dim, num_tokens


class IChannelMixer(Module):
    def __init__(self, in_dim: int, latent_dim: int, dropout: float):
        super().__init__()
        self.in_dim, self.latent_dim, self.dropout = in_dim, latent_dim, dropout


@token_mixers.register("attention")
class AttentionTokenMixer(ITokenMixer):
    """reference mixed_stacks/token_mixers.py:57-83"""

    def __init__(self, in_dim: int, num_tokens: int, *, attention_type: str = "basic",
                 **attention_kwargs: Any):
        super().__init__(in_dim, num_tokens)
        attention_kwargs.setdefault("bias", False)
        attention_kwargs.setdefault("num_heads", 8)
        attention_kwargs["input_dim"] = in_dim
        attention_kwargs.setdefault("is_self_attention", True)
        self.net = attentions.build(attention_type, config=attention_kwargs)

    def forward(self, net: Tensor, hw: Optional[Tuple[int, int]] = None, *, deterministic: bool = False,
                mask: Optional[Tensor] = None, residual: Optional[Tensor] = None) -> Tensor:
        return self.net(net, net, net, hw=hw, mask=mask, deterministic=deterministic,
                        residual=residual).output


class _Act(Module):
    def __init__(self, name: str):
        super().__init__()
        self.name = name

    def forward(self, net: Tensor) -> Tensor:
        if self.name == "quick_gelu":
            raise NotImplementedError("quick GELU exists as a GEMM epilogue only (FeedForward.forward)")
        return HF.gelu(net)


class GEGLU(Module):
    """reference activations.py:150-158: `net` = HijackLinear(in, 2 * out); value * gelu(gate)"""

    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.net = HijackLinear(in_dim, out_dim * 2)

    def forward(self, net: Tensor) -> Tensor:
        return HF.geglu(self.net(net))


@channel_mixers.register("ff")
class FeedForward(IChannelMixer):
    """reference mixed_stacks/channel_mixers.py:15-43 — `net.0` Linear, `net.1` act, `net.2`
    Dropout, `net.3` Linear, (`net.4` Dropout); state keys `net.0.linear.*`, `net.3.linear.*`."""

    def __init__(self, in_dim: int, latent_dim: int, dropout: float, activation: str = "GELU",
                 add_last_dropout: bool = True):
        super().__init__(in_dim, latent_dim, dropout)
        if activation not in ("GELU", "quick_gelu", "geglu"):
            raise NotImplementedError(f"activation '{activation}' is not on the accelerated hot path yet")
        self.activation = activation
        blocks: List[Module]
        if activation == "geglu":  # state keys `net.0.net.*` (GEGLU's Linear(in, 2 * latent)), `net.2.linear.*`
            blocks = [GEGLU(in_dim, latent_dim)]
        else:
            blocks = [HijackCustomLinear(in_dim, latent_dim), _Act(activation)]
        blocks += [Dropout(dropout), HijackCustomLinear(latent_dim, in_dim)]
        if add_last_dropout:
            blocks.append(Dropout(dropout))
        self.add_last_dropout = add_last_dropout
        self.net = nn.Sequential(*blocks)

    @property
    def need_2d(self) -> bool:
        return False

    @property
    def drops(self) -> bool:
        return self.training and 0.0 < self.dropout < 1.0

    def forward(self, net: Tensor, *, residual: Optional[Tensor] = None) -> Tensor:
        drops = self.drops
        last = len(self.net) - (2 if self.add_last_dropout else 1)  # index of the second Linear
        if self.activation == "geglu":
            h = self.net[0](net)
        else:  # bias + activation (exact-erf GELU / quick GELU) fused in the GEMM epilogue
            h = self.net[0](net, act=HF.ACT_GELU if self.activation == "GELU" else HF.ACT_QGELU)
        if not drops:
            return self.net[last](h, residual=residual)
        # dropout > 0 (training): the reference's op sequence, the last dropout sits between the second Linear and
        # the residual add, so the add cannot ride in the GEMM epilogue
        h = self.net[last - 1](h)
        out = self.net[last](h)
        if self.add_last_dropout:
            out = self.net[last + 1](out)
        return out if residual is None else HF.add(residual, out) if residual.dtype == out.dtype else residual + out



def _rwkv_init_linears(module: Module, zero_keys: Sequence[str]) -> None:
    """token_mixers.py:127-134 / channel_mixers.py:86-93: walk the state dict in order, zero the named layers, orthogonal otherwise"""
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if any(zero_k in k for zero_k in zero_keys):
                nn.init.zeros_(v)
            else:
                nn.init.orthogonal_(v)


def _rwkv_ramp(in_dim: int) -> Tensor:
    x = torch.ones(1, 1, in_dim)
    for i in range(in_dim):
        x[0, 0, i] = i / in_dim
    return x


@token_mixers.register("rwkv")
class RWKVTokenMixer(ITokenMixer):
    """reference mixed_stacks/token_mixers.py:107-206 — `key`, `value`, `receptance`, `output` (nn.Linear without bias: they hold the
    weights, the products are GEMMs of `rwkv.TimeMixFn` and `functional.linear`), `info_decay` [L, 1], the int64 buffer `time_curve` [1, T], `time_mix_k / v / r`
    [1, 1, C]; same keys, order and initial values.  The shift and mixes, the WKV term and the sigmoid gate are the kernels of
    csrc/rwkv.hip (`rwkv.TimeMixFn`, `rwkv.WkvFn`): two recurrences along T instead of two T-tap grouped convolutions."""

    f32_input = True  # (MixingBlock: the pre-norm LayerNorm hands over f32, the time mix rounds to bf16 once)

    def __init__(self, layer_idx: int, num_layers: int, num_tokens: int, in_dim: int, latent_dim: int):
        super().__init__(in_dim, num_tokens)
        latent_dim = latent_dim or in_dim
        _rwkv.check_dims("RWKVTokenMixer", in_dim, latent_dim)
        self.ci = self.latent_dim = latent_dim
        self.key = nn.Linear(in_dim, latent_dim, bias=False)
        self.value = nn.Linear(in_dim, latent_dim, bias=False)
        self.receptance = nn.Linear(in_dim, latent_dim, bias=False)
        self.output = nn.Linear(latent_dim, in_dim, bias=False)
        _rwkv_init_linears(self, ("key", "receptance", "output"))
        zero_to_one = layer_idx / (num_layers - 1)
        one_to_almost0 = 1.0 - (layer_idx / num_layers)
        f1_begin, f1_end, f2_begin, f2_end = 3.0, 1.2, 0.65, 0.4
        first_sa_layer_id = int(num_layers > 2)
        mul = layer_idx - first_sa_layer_id
        divider = num_layers - 1 - first_sa_layer_id
        f1 = f1_begin + mul / divider * (f1_end - f1_begin)
        f2 = f2_begin + mul / divider * (f2_end - f2_begin)
        if layer_idx == first_sa_layer_id:
            f1 += 0.5
        elif layer_idx == num_layers - 2:
            f2 = 0.4
        elif layer_idx == num_layers - 1:
            f2 = 0.37
        decay = torch.ones(latent_dim, 1)
        for h in range(latent_dim):
            decay[h][0] = math.pow(f2, h / (latent_dim - 1) * 7.0) * f1
        self.info_decay = nn.Parameter(decay.log())
        self.register_buffer("time_curve", torch.arange(-num_tokens + 1, 1)[None])
        x = _rwkv_ramp(in_dim)
        self.time_mix_k = nn.Parameter(torch.pow(x, one_to_almost0))
        self.time_mix_v = nn.Parameter(torch.pow(x, one_to_almost0) + 0.3 * zero_to_one)
        self.time_mix_r = nn.Parameter(torch.pow(x, 0.5 * one_to_almost0))

    @property
    def need_2d(self) -> bool:
        return False

    def forward(self, net: Tensor, hw: Optional[Tuple[int, int]] = None, *, deterministic: bool = False,
                residual: Optional[Tensor] = None) -> Tensor:
        _rwkv.check_input(net, "RWKVTokenMixer", self.in_dim, self.num_tokens)
        k, v, r = _rwkv.time_mix(net, self.time_mix_k, self.time_mix_v, self.time_mix_r, self.key.weight, self.value.weight,
                                 self.receptance.weight)
        return _rwkv.wkv(k, v, r, self.info_decay, self.output.weight, residual)  # the residual add rides in the output GEMM's epilogue


@channel_mixers.register("rwkv")
class RWKVChannelMixer(IChannelMixer):
    """reference mixed_stacks/channel_mixers.py:69-113 — `key` [L, C], `value` [C, L], `receptance` [C, C] (nn.Linear without bias),
    `time_mix_k / r` [1, 1, C].  sigmoid(receptance(in_r)) * value(relu(key(in_k))^2); like the reference's, it has no dropout layer."""

    f32_input = True

    def __init__(self, layer_idx: int, num_layers: int, in_dim: int, latent_dim: int, dropout: float):
        super().__init__(in_dim, latent_dim, dropout)
        _rwkv.check_dims("RWKVChannelMixer", in_dim, latent_dim)
        self.key = nn.Linear(in_dim, latent_dim, bias=False)
        self.value = nn.Linear(latent_dim, in_dim, bias=False)
        self.receptance = nn.Linear(in_dim, in_dim, bias=False)
        _rwkv_init_linears(self, ("value", "receptance"))
        one_to_almost0 = 1.0 - (layer_idx / num_layers)
        x = _rwkv_ramp(in_dim)
        self.time_mix_k = nn.Parameter(torch.pow(x, one_to_almost0))
        self.time_mix_r = nn.Parameter(torch.pow(x, one_to_almost0))

    @property
    def need_2d(self) -> bool:
        return False

    def forward(self, net: Tensor, *, residual: Optional[Tensor] = None) -> Tensor:
        _rwkv.check_input(net, "RWKVChannelMixer", self.in_dim)
        h, r = _rwkv.time_mix(net, self.time_mix_k, None, self.time_mix_r, self.key.weight, None, self.receptance.weight)
        kv = _rwkv.squared_relu(h, self.value.weight)
        return _rwkv.gate(r, kv, residual)  # the residual add rides in the gate kernel


class PreNorm(Module):
    """reference high_level.py:26-60 (non-attention use: norm then module)."""

    def __init__(self, *dims: int, module: Module, norm_type: Optional[str] = "layer",
                 norm_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__()
        self.norms = nn.ModuleList([NormFactory(norm_type).make(dim, **(norm_kwargs or {})) for dim in dims])
        self.module = module

    def forward(self, *xs: Tensor, **kwargs: Any) -> Tensor:
        return self.module(*[norm(x) for x, norm in zip(xs, self.norms)], **kwargs)


# ---------------------------------------------------------------------------------------------
# MixingBlock / MixedStackedEncoder
# ---------------------------------------------------------------------------------------------


class MixingBlock(Module):
    """reference mixed_stacks/api.py:41-185 — `token_norm`, `token_mixing`, `channel_norm`,
    `channel_mixing`."""

    def __init__(self, layer_idx: int, num_layers: int, num_tokens: int, in_dim: int, latent_dim: int, *,
                 norm_position: str = "pre_norm", token_mixing_type: str,
                 token_mixing_config: Optional[Dict[str, Any]] = None,
                 token_mixing_dropout: Optional[float] = None, channel_mixing_type: str = "ff",
                 channel_mixing_config: Optional[Dict[str, Any]] = None, dropout: float = 0.0,
                 drop_path: float = 0.0, norm_type: Optional[str] = "batch_norm",
                 norm_kwargs: Optional[Dict[str, Any]] = None, residual_after_norm: bool = False):
        super().__init__()
        if norm_position not in ("pre_norm", "post_norm"):
            raise ValueError("`norm_position` should be either 'pre_norm' or 'post_norm'")  # api.py:79-81
        if residual_after_norm:
            raise NotImplementedError("residual_after_norm is outside the hot path")
        self.norm_position = norm_position
        self.drop_path = DropPath(drop_path)  # api.py:84: one DropPath module, used on both branches
        tm = dict(token_mixing_config or {})
        tm.update(layer_idx=layer_idx, num_layers=num_layers, num_tokens=num_tokens, in_dim=in_dim,
                  latent_dim=latent_dim, dropout=dropout)
        self.token_norm = NormFactory(norm_type).make(in_dim, **(norm_kwargs or {}))
        self.token_mixing = token_mixers.build(token_mixing_type, config=tm)
        self.token_mixing_dropout = Dropout(dropout if token_mixing_dropout is None else token_mixing_dropout)
        cm = dict(channel_mixing_config or {})
        cm.update(layer_idx=layer_idx, num_layers=num_layers, in_dim=in_dim, latent_dim=latent_dim,
                  dropout=dropout)
        self.residual_after_norm = residual_after_norm
        self.channel_norm = NormFactory(norm_type).make(in_dim, **(norm_kwargs or {}))
        self.channel_mixing = channel_mixers.build(channel_mixing_type, config=cm)
        # a mixer that works on its input elementwise before its first GEMM (rwkv: the time mix) sets `f32_input` and is handed the
        # LayerNorm's f32 output: its GEMM operands are then rounded to bf16 once, as under the reference's autocast, not twice
        if norm_position == "pre_norm":
            for norm, mixer in ((self.token_norm, self.token_mixing), (self.channel_norm, self.channel_mixing)):
                if getattr(mixer, "f32_input", False) and isinstance(norm, LayerNorm):
                    norm.out_f32 = True
        self.use_fused = True

    def _stochastic(self) -> bool:
        """any dropout / stochastic depth active in this forward (training mode with a rate in (0, 1))"""
        if not self.training:
            return False
        rates = (self.drop_path.dropout, self.token_mixing_dropout.p, getattr(self.channel_mixing, "dropout", 0.0))
        return any(0.0 < r < 1.0 for r in rates)

    def _fusable(self) -> bool:
        tmix, cmix = self.token_mixing, self.channel_mixing
        if self.norm_position != "pre_norm":  # the fused block / stack kernels are the pre-norm form
            return False
        if self._stochastic():  # ... and have no random masks: composed path
            return False
        if not (isinstance(tmix, AttentionTokenMixer) and isinstance(cmix, FeedForward)):
            return False
        att = tmix.net
        if not (isinstance(att, Attention) and att.qkv_same and att.hook is None and att.head_dim == 64):
            return False
        if not (isinstance(self.token_norm, LayerNorm) and isinstance(self.channel_norm, LayerNorm)):
            return False
        if cmix.activation == "geglu":
            return False
        lins = (att.out_linear, cmix.net[0], cmix.net[3])
        if any(l.linear is None or l.hook is not None for l in lins):
            return False
        params = [att.in_w, att.out_linear.linear.weight, cmix.net[0].linear.weight, cmix.net[3].linear.weight]
        return all(HF._is_direct(p) for p in params)

    def fused_params(self) -> list:
        """the 12 parameters in the order fused.MixingBlockFn / MixingStackFn take them"""
        att, ff = self.token_mixing.net, self.channel_mixing
        return [self.token_norm.weight, self.token_norm.bias, att.in_w, att.qkv_bias,
                att.out_linear.linear.weight, att.out_linear.linear.bias, self.channel_norm.weight,
                self.channel_norm.bias, ff.net[0].linear.weight, ff.net[0].linear.bias,
                ff.net[3].linear.weight, ff.net[3].linear.bias]

    def fused_meta(self) -> tuple:
        return (self.token_mixing.net.num_heads, self.token_norm.eps, self.channel_norm.eps,
                self.channel_mixing.activation == "quick_gelu")

    def forward(self, net: Tensor, hw: Optional[Tuple[int, int]] = None, *, deterministic: bool = False,
                mask: Optional[Tensor] = None, causal: bool = False, **kwargs: Any) -> Tensor:
        """`causal=True` is the kernel-side form of the text tower's `triu(1)` mask (nlp/encoder/transformer.py:
        44-50): no mask tensor is read."""
        if self.use_fused and not kwargs and net.dim() == 3 and self._fusable():
            keep = None if mask is None else expand_module_mask(mask, self.token_mixing.net.num_heads)
            return fused.mixing_block(net, *self.fused_params(), *self.fused_meta()[:3], keep, causal,
                                      self.fused_meta()[3])
        # composed path: same kernels, one autograd node per op
        tkw = dict(hw=hw, deterministic=deterministic, residual=net)
        if causal and mask is None:
            t = net.shape[1]
            mask = torch.ones(t, t, dtype=torch.bool, device=net.device).triu_(1)
        if mask is not None:
            tkw["mask"] = mask
        tkw.update(kwargs)
        stoch = self._stochastic()

        def plus(x: Tensor, branch: Tensor) -> Tensor:
            return x + branch.to(x.dtype) if x.dtype != branch.dtype else HF.add(x, branch)

        if self.norm_position == "post_norm":
            # api.py:160-185: x = LN(x + dp(drop(token_mix(x)))); x = LN(x + dp(channel_mix(x)))
            if not stoch:
                s1 = self.token_mixing(net, **tkw)  # the residual add rides in the output GEMM's epilogue
            else:
                tkw.pop("residual")
                s1 = plus(net, self.drop_path(self.token_mixing_dropout(self.token_mixing(net, **tkw))))
            net = self.token_norm(s1)
            if not stoch:
                s2 = self.channel_mixing(net, residual=net)
            else:
                s2 = plus(net, self.drop_path(self.channel_mixing(net)))
            return self.channel_norm(s2)
        if not self._stochastic():
            net = self.token_mixing(self.token_norm(net), **tkw)
            return self.channel_mixing(self.channel_norm(net), residual=net)
        # dropout / DropPath active (api.py:130-158): branch -> dropout -> drop_path -> + residual, op by op
        tkw.pop("residual")
        branch = self.drop_path(self.token_mixing_dropout(self.token_mixing(self.token_norm(net), **tkw)))
        net = net + branch.to(net.dtype) if net.dtype != branch.dtype else HF.add(net, branch)
        branch = self.drop_path(self.channel_mixing(self.channel_norm(net)))
        return net + branch.to(net.dtype) if net.dtype != branch.dtype else HF.add(net, branch)


class PositionalEncoding(Module):
    """reference mixed_stacks/api.py:188-267 — parameter `pos_encoding` [1, T, D]."""

    def __init__(self, dim: int, num_tokens: int, dropout: float = 0.0, *, num_head_tokens: int,
                 is_vision: bool, enable: bool = True):
        super().__init__()
        self.pos_drop = None
        self.pos_encoding = None
        if enable:
            self.pos_drop = Dropout(p=dropout)
            self.pos_encoding = nn.Parameter(torch.zeros(1, num_tokens, dim))
            nn.init.trunc_normal_(self.pos_encoding, std=0.02)
        self.num_head_tokens = num_head_tokens
        self.is_vision = is_vision

    def interpolate_pos_encoding(self, num_tokens_now: int, hwp: Optional[Tuple[int, int, int]]) -> Tensor:
        """reference api.py:231-267 (vision encodings at a non-native resolution): the [sqrt(T) x sqrt(T)] grid of
        learned encodings is resampled bicubically (align_corners=False, recompute_scale_factor=True — toolkit.py:
        2841-2861) to the current patch grid; head-token encodings pass through.  A once-per-forward resample of a
        [1, T, D] table: done with torch's interpolate (glue, like the argmax of the CLIP pooling), its gradient flows
        back to the parameter through autograd."""
        import math

        pos = self.pos_encoding
        num_current = num_tokens_now - self.num_head_tokens
        num_history = pos.shape[1] - self.num_head_tokens
        h = w = patch_size = None
        if hwp is not None:
            h, w, patch_size = hwp
        if num_current == num_history and w == h:
            return pos
        if w is None or h is None or patch_size is None:
            raise ValueError("`hwp` should be provided for `interpolate_pos_encoding`")
        head = pos[:, :self.num_head_tokens] if self.num_head_tokens > 0 else None
        grid = pos[:, self.num_head_tokens:]
        dim = pos.shape[-1]
        sqrt = math.sqrt(num_history)
        wh_ratio = w / h
        pw = math.sqrt(num_current * wh_ratio) + 0.1
        ph = math.sqrt(num_current / wh_ratio) + 0.1
        grid = torch.nn.functional.interpolate(grid.reshape(1, int(sqrt), int(sqrt), dim).permute(0, 3, 1, 2),
                                               mode="bicubic", scale_factor=(pw / sqrt, ph / sqrt),
                                               recompute_scale_factor=True, align_corners=False)
        assert int(pw) == grid.shape[-2] and int(ph) == grid.shape[-1]
        grid = grid.permute(0, 2, 3, 1).reshape(1, -1, dim)
        return grid if head is None else torch.cat([head, grid], dim=1)


class MixedStackedEncoder(Module):
    """reference mixed_stacks/api.py:270-458: optional head token, learned positional encoding (native
    resolution), optional embedding norm, pre-norm blocks, head = `x[:, 0]` (head token) or identity, normalised
    before (`PreNorm`, state keys `head.norms.0.*`) or after (`head_norm.*`) the head.  Poolers other than the
    head token / identity, aux heads and dropouts are outside the accelerated hot path."""

    def __init__(self, in_dim: int, num_tokens: int, *, token_mixing_type: str,
                 token_mixing_config: Optional[Dict[str, Any]] = None, channel_mixing_type: str = "ff",
                 channel_mixing_config: Optional[Dict[str, Any]] = None, num_layers: int = 4,
                 dropout: float = 0.0, dpr_list: Optional[List[float]] = None, drop_path_rate: float = 0.1,
                 norm_position: str = "pre_norm", norm_type: Optional[str] = "batch_norm",
                 norm_kwargs: Optional[Dict[str, Any]] = None, embedding_norm: Optional[Module] = None,
                 embedding_dropout: Optional[float] = None, residual_after_norm: bool = False,
                 latent_dim: Optional[int] = None, latent_dim_ratio: float = 1.0,
                 use_head_token: bool = False, head_pooler: Optional[str] = "mean",
                 use_positional_encoding: bool = False,
                 is_vision_positional_encoding: Optional[bool] = None,
                 positional_encoding_dropout: float = 0.0, no_head_norm: Optional[bool] = None,
                 norm_after_head: bool = False, aux_heads: Optional[List[str]] = None):
        super().__init__()
        if aux_heads is not None:
            raise NotImplementedError("aux heads are outside the accelerated hot path")
        if not use_head_token and head_pooler is not None:
            raise NotImplementedError(f"head pooler '{head_pooler}' is outside the accelerated hot path "
                                      "(head token or `head_pooler=None` are built)")
        if no_head_norm is None:
            no_head_norm = norm_position == "post_norm"
        self.no_head_norm = bool(no_head_norm)  # api.py:372-377: post-norm stacks end in a LayerNorm already
        self.aux_heads = None
        if use_head_token:
            self.head_token = nn.Parameter(torch.zeros(1, 1, in_dim))
            num_head_tokens = 1
        else:
            self.head_token = None
            num_head_tokens = 0
        self.num_heads = num_head_tokens
        num_tokens += num_head_tokens
        if is_vision_positional_encoding is None:
            if use_positional_encoding:
                raise ValueError("`is_vision_positional_encoding` should be specified when "
                                 "`use_positional_encoding` is set to True")
            is_vision_positional_encoding = False
        self.pos_encoding = PositionalEncoding(in_dim, num_tokens, positional_encoding_dropout,
                                               num_head_tokens=num_head_tokens,
                                               is_vision=bool(is_vision_positional_encoding),
                                               enable=use_positional_encoding)
        self.embedding_norm = embedding_norm
        if isinstance(embedding_norm, LayerNorm):
            embedding_norm.out_f32 = True  # its output is the residual stream of the blocks: f32 in, f32 out (see ViTEncoder.forward)
        self.embedding_dropout = None if embedding_dropout is None else Dropout(embedding_dropout)  # api.py:330-333
        if dpr_list is None:
            dpr_list = [x.item() for x in torch.linspace(0, drop_path_rate, num_layers)]
        if latent_dim is None:
            latent_dim = int(round(in_dim * latent_dim_ratio))
        self.mixing_blocks = nn.ModuleList([
            MixingBlock(i, num_layers, num_tokens, in_dim, latent_dim, norm_position=norm_position,
                        token_mixing_type=token_mixing_type,
                        token_mixing_config=shallow_copy_dict(token_mixing_config or {}),
                        channel_mixing_type=channel_mixing_type,
                        channel_mixing_config=shallow_copy_dict(channel_mixing_config or {}),
                        dropout=dropout, drop_path=dp, norm_type=norm_type, norm_kwargs=norm_kwargs,
                        residual_after_norm=residual_after_norm)
            for i, dp in enumerate(dpr_list)
        ])
        head: Module = Lambda(lambda x: x[:, 0], name="head_token") if use_head_token else nn.Identity()
        if self.no_head_norm:
            self.head_norm = None
            self.head = head
        elif norm_after_head:
            self.head_norm = NormFactory(norm_type).make(in_dim, **(norm_kwargs or {}))
            self.head = head
        else:
            self.head_norm = None
            self.head = PreNorm(in_dim, module=head, norm_type=norm_type, norm_kwargs=norm_kwargs)
        if self.head_token is not None:
            nn.init.trunc_normal_(self.head_token, std=0.02)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m: Module) -> None:
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0.0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0.0)
            nn.init.constant_(m.weight, 1.0)

    fuse_stack = True  # all blocks as ONE autograd node when every block can take the fused path
    head_only_tail = True  # a fused stack read at its head token alone may run its last block's projection / FF GEMMs on the head rows only; False: never (the CLIP towers)

    def _head_ln(self) -> Module:
        return self.head_norm if self.head_norm is not None else self.head.norms[0]

    def post_process(self, net: Tensor) -> Tensor:
        # LayerNorm is row-wise, so LN(x)[:, 0] == LN(x[:, 0]) (PreNorm head) — and with `norm_after_head` the
        # reference computes LN(x[:, 0]) itself: normalise token 0 only (1/T of the PreNorm work, identical
        # result) by handing the kernel a strided row view.  Identity head (text tower): every token.
        if self.no_head_norm:  # post-norm stacks: the last block already ended in its LayerNorm
            return net[:, 0] if self.head_token is not None else net
        if self.head_token is not None:
            return self._head_ln()(net[:, 0])
        return self._head_ln()(net)

    def check_fused_token_assembly(self) -> None:
        """The ViT / CLIP entry points add the positional encoding inside their token-assembly kernels: a dropout ON
        the encoding (api.py:220, `positional_encoding_dropout` > 0 in training) has no place there."""
        drop = self.pos_encoding.pos_drop
        if drop is not None and self.training and 0.0 < drop.p < 1.0:
            raise NotImplementedError("positional_encoding_dropout > 0 is not provided by the fused token-assembly "
                                      "kernels (patch embedding / token embedding); use the generic pre_process path")

    def pre_process(self, net: Tensor, *, hwp: Any = None, deterministic: bool = False) -> Tensor:
        """Generic token input [B, T, D] (reference :419-438).  The ViT / CLIP entry points do NOT come through
        here: they fuse head token / positional add into their token-assembly kernels."""
        if self.head_token is not None:
            net = torch.cat([self.head_token.expand(net.shape[0], -1, -1).to(net.dtype), net], dim=1)
        if self.pos_encoding.pos_encoding is not None:
            pos = self.pos_encoding.pos_encoding
            heads = self.pos_encoding.num_head_tokens
            if self.pos_encoding.is_vision:
                span = net.shape[1]
                if pos.shape[1] != net.shape[1] or hwp is not None:
                    pos = self.pos_encoding.interpolate_pos_encoding(net.shape[1], hwp)
            else:
                # api.py:216-227: sequence encodings cover the first T - num_head_tokens positions of the stream
                # (the head token sits in FRONT, so the last feature token goes without one — mirrored as is)
                span = net.shape[1] - heads
                pos = pos[:, :span]
            if self.pos_encoding.pos_drop is not None:
                pos = self.pos_encoding.pos_drop(pos)  # api.py:220: the dropout acts on the encoding itself
            net = net.float()
            if span == net.shape[1]:
                net = net + pos
            else:
                net = torch.cat([net[:, :span] + pos, net[:, span:]], dim=1)
        if self.embedding_norm is not None:
            net = self.embedding_norm(net)
        if self.embedding_dropout is not None:
            net = self.embedding_dropout(net)
        return net

    def forward_tokens(self, tokens: Tensor, *, hw: Optional[Tuple[int, int]] = None,
                       deterministic: bool = False, causal: bool = False, mask: Optional[Tensor] = None,
                       clip_skip: int = 0, apply_head: bool = True) -> Tensor:
        """`tokens` = the output of pre_process (or of a fused token-assembly kernel + embedding norm)."""
        net = tokens
        blocks = list(self.mixing_blocks)
        if clip_skip > 0:
            blocks = blocks[:len(blocks) - clip_skip]
        if (self.fuse_stack and len(blocks) > 1 and net.dim() == 3 and mask is None
                and all(b.use_fused and b._fusable() for b in blocks)):
            # one autograd node for the whole stack (fused.MixingStackFn)
            metas, params = [], []
            slices = getattr(self, "stack_slices", None)
            sf, sb = (slices, 0) if isinstance(slices, int) else (tuple(slices) + (0, 0))[:2] if slices else (0, 0)
            # 8th entry, `head_only`: what leaves this call is `net[:, 0]` of the stack's output (post_process: the head token, under
            # either position of the head norm), so the last block may run its projection / FF GEMMs on the head rows only (fused.HEAD_ONLY)
            head_only = bool(apply_head and self.head_token is not None and clip_skip == 0 and not causal and self.head_only_tail
                             and torch.is_grad_enabled())  # (evaluation without grad keeps the full block)
            extra = (int(sf or 0), int(sb or 0), int(getattr(self, "grad_stream_words", 0) or 0), head_only)  # (0 = the module default of fused.py)
            for b in blocks:
                metas.append(b.fused_meta() + extra)
                params.extend(b.fused_params())
            net = fused.mixing_stack(net, tuple(metas), None, causal, params)
        else:
            for block in blocks:
                net = block(net, hw, deterministic=deterministic, mask=mask, causal=causal)
        return self.post_process(net) if apply_head else net

    def forward(self, net: Tensor, *, hw: Optional[Tuple[int, int]] = None, hwp: Any = None,
                deterministic: bool = False) -> Tensor:
        return self.forward_tokens(self.pre_process(net, hwp=hwp, deterministic=deterministic), hw=hw,
                                   deterministic=deterministic)


# ---------------------------------------------------------------------------------------------
# patch embedding / ViT encoder / classifier
# ---------------------------------------------------------------------------------------------


class Conv2d(Module):
    """reference convs/basic.py:41-184 — parameters `weight` [out, in / groups, k, k], `bias`.  groups = 1: implicit GEMM /
    im2row + MFMA GEMM (`functional.Conv2dFn`); groups > 1 (depthwise included): the direct kernels of
    `functional.GroupedConv2dFn`; the stride == kernel, padding 0 form of the ViT patch embedding has its own fused path
    (`functional.patch_tokens`).

    Round 5 — the constructor / forward options that used to raise (none is used by a named benchmark configuration):
      * `padding="reflection[N]"` (basic.py:61-75): `cfhip_reflect_pad2d_*` in front of an unpadded convolution;
      * `transform_kernel`, `demodulate`, `weight_scale`, `style` (basic.py:116-150; the StyleGAN forms): these act on the
        WEIGHT tensor — parameter-sized element-wise math, done with torch ops on the fp32 parameter (autograd carries their
        gradients back to it); the convolution of the activations still runs on the HIP path (`style` makes it a grouped
        convolution with one group per sample, as in the reference);
      * `forward(transpose=True)` (basic.py:151-160): `functional.ConvTranspose2dFn`, groups = 1."""

    def __init__(self, in_channels: int, out_channels: int, *, kernel_size: int, groups: int = 1,
                 stride: int = 1, dilation: int = 1, padding: Any = "same", transform_kernel: bool = False,
                 bias: bool = True, demodulate: bool = False, weight_scale: Optional[float] = None,
                 gain: float = math.sqrt(2.0)):
        super().__init__()
        self.reflection_pad: Optional[Tuple[int, int, int, int]] = None
        if padding == "same":
            padding = kernel_size // 2
        elif isinstance(padding, str) and padding.startswith("reflection"):
            n = kernel_size // 2 if padding == "reflection" else int(padding[len("reflection"):])
            pads = [n, n, n, n]  # (left, right, top, bottom)
            if transform_kernel:  # the transformed kernel is one tap larger: one more row / column at the top / left
                pads[0] += 1
                pads[2] += 1
            self.reflection_pad = tuple(pads)
            padding = 0
        elif not isinstance(padding, int):
            raise ValueError(f"padding = {padding!r}: an int, 'same' or 'reflection[N]'")
        if groups < 1 or in_channels % groups or out_channels % groups:
            raise ValueError(f"`groups` ({groups}) must divide in_channels ({in_channels}) and out_channels ({out_channels})")
        self.in_c, self.out_c, self.kernel_size = in_channels, out_channels, kernel_size
        self.groups, self.stride, self.dilation, self.padding = groups, stride, dilation, padding
        self.transform_kernel, self.demodulate, self.weight_scale = transform_kernel, demodulate, weight_scale
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        with torch.no_grad():
            nn.init.xavier_normal_(self.weight.data, gain / math.sqrt(2.0))
            if self.bias is not None:
                self.bias.zero_()

    def _effective_weight(self, style: Optional[Tensor]) -> Tensor:
        """the weight the convolution sees (basic.py:116-150), in the reference's order: kernel transform, style modulation,
        demodulation, scale.  Untouched parameters pass through as they are (the direct-gradient path of Conv2dFn)."""
        w: Tensor = self.weight
        if self.transform_kernel:  # average of the four one-tap shifts of the zero-padded kernel: [.., k + 1, k + 1]
            wp = torch.nn.functional.pad(w, [1, 1, 1, 1])
            w = (wp[:, :, 1:, 1:] + wp[:, :, :-1, 1:] + wp[:, :, 1:, :-1] + wp[:, :, :-1, :-1]) * 0.25
        if style is not None:      # [B, out, in, k, k]: one filter bank per sample
            w = w[None] * style.to(w.dtype)[:, None, :, None, None]
        if self.demodulate:
            w = w * torch.rsqrt(w.pow(2).sum([-3, -2, -1], keepdim=True) + 1e-8)
        if self.weight_scale is not None:
            w = w * self.weight_scale
        return w

    def forward(self, net: Tensor, style: Optional[Tensor] = None, *, transpose: bool = False) -> Tensor:
        b = net.shape[0]
        if style is not None:
            if self.bias is not None:
                raise ValueError("`bias` should not be used when `style` is provided")
            if self.groups != 1:
                raise ValueError("`groups` should be 1 when `style` is provided")
            if self.reflection_pad is not None:
                raise ValueError("`reflection_pad` should not be used when `style` is provided, maybe you want to use `same` padding?")
        if self.reflection_pad is not None:
            net = HF.reflect_pad2d(net, self.reflection_pad)
        w = self._effective_weight(style)
        bias, groups = self.bias, self.groups
        if style is not None:  # a grouped convolution over the batch: sample i sees filter bank i
            groups = b
            net = net.reshape(1, b * net.shape[1], *net.shape[2:])
            w = w.reshape(b * self.out_c, *w.shape[2:])
        if transpose:
            if groups != 1:
                raise NotImplementedError("transposed convolution with groups > 1 (or `style`) is outside the accelerated hot path")
            out = HF.conv_transpose2d(net, w.transpose(0, 1).contiguous(), self.stride, self.padding, self.dilation)
            if bias is not None:  # (per-channel add of a parameter: a torch op; autograd gives its gradient)
                out = out + bias.to(out.dtype).view(1, -1, 1, 1)
            return out
        out = HF.conv2d(net, w.contiguous(), bias, self.stride, self.padding, self.dilation, groups)
        if style is None:
            return out
        return out.reshape(b, -1, *out.shape[2:])

    def extra_repr(self) -> str:
        return (f"{self.in_c}, {self.out_c}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, dilation={self.dilation}, bias={self.bias is not None}, demodulate={self.demodulate}")


class DepthWiseConv2d(Module):
    """reference convs/basic.py:187-201: 3x3 / stride 1 / pad 1 convolution with one filter per channel; state key `net.*`"""

    def __init__(self, dim: int):
        super().__init__()
        self.net = Conv2d(dim, dim, kernel_size=3, stride=1, padding=1, bias=True, groups=dim)

    def forward(self, net: Tensor) -> Tensor:
        return self.net(net)


def get_conv_blocks(in_channels: int, out_channels: int, kernel_size: int, stride: int, *, bias: bool = True,
                    norm_type: Optional[str] = None, norm_kwargs: Optional[Dict[str, Any]] = None,
                    activation: Any = None, conv_base: Any = None, pre_activate: bool = False, **conv2d_kwargs: Any) -> List[Module]:
    """reference convs/basic.py:529-571 (no ECA / CA blocks, no demodulation).  `conv_base`: the convolution class (default `Conv2d`;
    the PixelCNN passes `MaskedConv2d` with its `mask_type`), called with keywords as the reference calls it."""
    conv = (conv_base or Conv2d)(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, bias=bias,
                                 **conv2d_kwargs)
    blocks: List[Module] = []
    if not pre_activate:
        blocks.append(conv)
    NormFactory(norm_type).inject_to(out_channels, norm_kwargs or {}, blocks)
    if activation is not None:
        blocks.append(build_activation(activation) if isinstance(activation, str) else activation)
    if pre_activate:
        blocks.append(conv)
    return blocks


class ChannelPadding(Module):
    """reference core/high_level.py:59-105: a learned token of `latent_channels` channels (one per class when `num_classes` is given;
    global, or a `map_dim` x `map_dim` map) concatenated to the input and mapped back to `in_channels` by a bias-free Linear (`is_1d`)
    or 1x1 Conv2d.  State keys `channel_padding`, `mapping.weight`.  The token's lookup / repeat / concatenation are torch indexing ops
    (autograd carries the token's gradient); the mapping runs on the HIP path."""

    def __init__(self, in_channels: int, latent_channels: int, map_dim: Optional[int] = None, *, is_1d: bool = False,
                 num_classes: Optional[int] = None):
        super().__init__()
        self.in_channels, self.latent_channels, self.map_dim = in_channels, latent_channels, map_dim
        self.is_global = map_dim is None
        self.is_conditional = num_classes is not None
        if self.is_global:
            map_dim = 1
        self.channel_padding = nn.Parameter(torch.randn((num_classes or 1), latent_channels, map_dim, map_dim))
        in_nc = in_channels + latent_channels
        if is_1d:
            self.mapping = Linear(in_nc, in_channels, bias=False)
        else:
            self.mapping = Conv2d(in_nc, in_channels, kernel_size=1, bias=False)

    def forward(self, net: Tensor, labels: Optional[Tensor] = None) -> Tensor:
        if not self.is_conditional:
            padding = self.channel_padding.repeat(net.shape[0], 1, 1, 1)
        else:
            if labels is None:
                raise ValueError("`labels` should be provided in conditional `ChannelPadding`")
            padding = self.channel_padding[labels.view(-1)]
        if self.is_global:
            if net.dim() == 2:
                padding = padding.view(padding.shape[0], -1)
            else:
                padding = padding.repeat(1, 1, *net.shape[-2:])
        return self.mapping(torch.cat([net, padding.to(net.dtype)], dim=1))

    def extra_repr(self) -> str:
        map_dim_str = "global" if self.is_global else f"{self.map_dim}x{self.map_dim}"
        return f"{self.in_channels}+{self.latent_channels}, {map_dim_str}"


@encoders.register("vanilla")
class VanillaEncoder(Module):
    """reference cv/encoder/vanilla.py:18-104: conv(k = first_kernel_size) -> norm -> act, then
    `num_downsample` stride-2 convs (the last one bare); state keys `encoder.<i>.*` of the nn.Sequential."""

    def __init__(self, in_channels: int, num_downsample: int, latent_channels: int = 256, *, kernel_size: int = 3,
                 first_kernel_size: int = 7, start_channels: Optional[int] = None, num_residual_blocks: int = 0,
                 residual_dropout: float = 0.0, residual_kwargs: Optional[Dict[str, Any]] = None,
                 norm_type: Optional[str] = "batch", norm_kwargs: Optional[Dict[str, Any]] = None,
                 activation: str = "leaky_relu_0.2", padding: str = "same"):
        super().__init__()
        if num_residual_blocks != 0:
            raise NotImplementedError("residual blocks in VanillaEncoder are outside the accelerated hot path")
        self.in_channels, self.num_downsample = in_channels, num_downsample
        self.latent_channels, self.first_kernel_size = latent_channels, first_kernel_size
        if start_channels is None:
            start_channels = int(round(latent_channels / (2 ** num_downsample)))
        if start_channels <= 0:
            raise ValueError(f"latent_channels ({latent_channels}) is too small for num_downsample ({num_downsample})")
        blocks = get_conv_blocks(in_channels, start_channels, first_kernel_size, 1, norm_type=norm_type,
                                 norm_kwargs=norm_kwargs, activation=activation, padding=padding)
        in_nc = start_channels
        for i in range(num_downsample):
            is_last = i == num_downsample - 1
            out_nc = latent_channels if is_last else min(in_nc * 2, latent_channels)
            blocks.extend(get_conv_blocks(in_nc, out_nc, kernel_size, 2, norm_type=None if is_last else norm_type,
                                          activation=None if is_last else activation, padding=padding))
            in_nc = out_nc
        self.encoder = nn.Sequential(*blocks)

    def forward(self, net: Tensor) -> Tensor:
        return self.encoder(net)

    def encode(self, net: Tensor) -> Tensor:
        return self(net)


@encoders.register("vanilla_1d")
class VanillaEncoder1D(Module):
    """reference cv/encoder/vanilla.py:107-158: VanillaEncoder + AdaptiveAvgPool2d((1,1)) + squeeze -> [B, latent]"""

    def __init__(self, in_channels: int, num_downsample: int, latent_dim: int = 128, *,
                 img_size: Optional[int] = None, kernel_size: int = 3, first_kernel_size: int = 7,
                 start_channels: Optional[int] = None, num_residual_blocks: int = 0, residual_dropout: float = 0.0,
                 residual_kwargs: Optional[Dict[str, Any]] = None, norm_type: Optional[str] = "batch",
                 activation: str = "leaky_relu_0.2", padding: str = "same", pool: str = "average"):
        super().__init__()
        if pool != "average":
            raise NotImplementedError("only `pool='average'` is on the accelerated hot path")
        self.in_channels, self.latent_dim = in_channels, latent_dim
        self.encoder = VanillaEncoder(in_channels, num_downsample, latent_dim, kernel_size=kernel_size,
                                      first_kernel_size=first_kernel_size, start_channels=start_channels,
                                      num_residual_blocks=num_residual_blocks, residual_dropout=residual_dropout,
                                      residual_kwargs=residual_kwargs, norm_type=norm_type, activation=activation,
                                      padding=padding)
        self.pool = nn.AdaptiveAvgPool2d((1, 1))  # parameter-free: kept for the module tree / repr

    def forward(self, net: Tensor) -> Tensor:
        return HF.global_avg_pool(self.encoder(net))

    def encode(self, net: Tensor) -> Tensor:
        return self(net)


class Mapping(Module):
    """reference modules/core/mappings.py:34-87: Linear -> (BN) -> activation -> (Dropout); state keys
    `linear.linear.*`, `bn.*`."""

    def __init__(self, in_dim: int, out_dim: int, *, bias: Optional[bool] = None,
                 pruner_config: Optional[dict] = None, dropout: float = 0.5, batch_norm: bool = True,
                 activation: Optional[str] = "ReLU", activation_config: Optional[Dict[str, Any]] = None,
                 init_method: str = "xavier_normal", rank: Optional[int] = None,
                 rank_ratio: Optional[float] = None):
        super().__init__()
        if bias is None:
            bias = not batch_norm
        self.linear = Linear(in_dim, out_dim, bias=bias, pruner_config=pruner_config, init_method=init_method,
                             rank=rank, rank_ratio=rank_ratio)
        self.bn = BN(out_dim) if batch_norm else None
        self.activation = None if activation is None else build_activation(activation, activation_config)
        self.dropout = Dropout(dropout) if 0.0 < dropout < 1.0 else None  # mappings.py:66-67

    @property
    def weight(self) -> Tensor:
        return self.linear.weight

    @property
    def bias(self) -> Optional[Tensor]:
        return self.linear.bias

    def forward(self, net: Tensor) -> Tensor:
        net = self.linear(net)
        if self.bn is not None:
            net = self.bn(net)
        if self.activation is not None:
            net = self.activation(net)
        if self.dropout is not None:
            net = self.dropout(net)
        return net


@register_module("fcnn")
class FCNN(Module):
    """reference modules/ml/fcnn.py:12-57: `Mapping` per hidden unit + nn.Linear head; state keys
    `net.<i>.linear.linear.*`, `net.<n>.{weight,bias}`.  Logits are fp32."""

    def __init__(self, input_dim: int, output_dim: int, hidden_units: Optional[List[int]] = None, *,
                 mapping_type: str = "basic", bias: bool = True, activation: str = "ReLU", batch_norm: bool = False,
                 dropout: float = 0.0, rank: Optional[int] = None, rank_ratio: Optional[float] = None):
        super().__init__()
        if mapping_type != "basic":
            raise NotImplementedError(f"mapping type '{mapping_type}' is outside the accelerated hot path")
        if hidden_units is None:
            dim = max(32, min(1024, 2 * input_dim))
            hidden_units = 2 * [dim]
        blocks: List[Module] = []
        for hidden_unit in hidden_units:
            blocks.append(Mapping(input_dim, hidden_unit, bias=bias, activation=activation, batch_norm=batch_norm,
                                  dropout=dropout, rank=rank, rank_ratio=rank_ratio))
            input_dim = hidden_unit
        blocks.append(HijackLinear(input_dim, output_dim, bias))
        self.hidden_units = hidden_units
        self.net = nn.Sequential(*blocks)

    def forward(self, net: Tensor) -> Tensor:
        for blk in self.net[:-1]:
            net = blk(net)
        head = self.net[-1]
        if getattr(head, "hook", None) is not None:
            return _hooked_linear(head, net, out_f32=True)
        return HF.linear(net, head.weight, head.bias, out_f32=True)


@register_module("ml_rnn")
class RNN(Module):
    """reference modules/ml/rnn.py:20-85: a stack of single-layer, batch_first GRU / LSTM cells (`rnn_list.<i>.weight_ih_l0`,
    `weight_hh_l0`, `bias_ih_l0`, `bias_hh_l0` and their `_reverse` forms: nn.GRU's / nn.LSTM's own keys and shapes, so checkpoints
    load both ways), orthogonal weights and zero biases, then `FCNN` (`head.net.*`) on the last time step.  f32 parameters, f32 logits.
    The recurrence runs on the persistent kernels of csrc/rnn.hip (`rnn.RecurrentFn`); the input projections are `functional.linear`,
    which takes any feature width, so no feature column is padded; the first layer reads its f32 features as two bf16 words
    (`rnn.InputProjFn`).  cell = 'RNN' (the tanh cell) and hidden sizes outside the kernels
    (a multiple of 8, 8 .. 256) are refused."""

    def __init__(self, input_dim: int, output_dim: int, cell: str = "GRU", num_layers: int = 1, hidden_size: int = 256,
                 bidirectional: bool = False, hidden_units: Optional[List[int]] = None, *, mapping_type: str = "basic", bias: bool = True,
                 activation: str = "ReLU", batch_norm: bool = False, dropout: float = 0.0):
        super().__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        rnn_dim = self._init_rnn(cell, num_layers, hidden_size, bidirectional)
        self.head = FCNN(rnn_dim, output_dim, hidden_units, mapping_type=mapping_type, bias=bias, activation=activation,
                         batch_norm=batch_norm, dropout=dropout)

    def _init_rnn(self, cell: str, num_layers: int, hidden_size: int, bidirectional: bool) -> int:
        rnn_base = _rnn.rnn_dict[cell]
        rnn_dim = hidden_size * (1 + int(bidirectional))
        input_dimensions = [self.input_dim] + [rnn_dim] * (num_layers - 1)
        rnn_list = []
        for index, dim in enumerate(input_dimensions):
            # the first layer reads raw f32 features: both bf16 words of them (rnn.InputProjFn); deeper layers read hidden states
            rnn = rnn_base(dim, hidden_size=hidden_size, bidirectional=bidirectional, two_word_input=index == 0)
            with torch.no_grad():
                for name, param in rnn.named_parameters():
                    if "weight" in name:
                        nn.init.orthogonal_(param)
                    elif "bias" in name:
                        nn.init.zeros_(param)
            rnn_list.append(rnn)
        self.rnn_list = nn.ModuleList(rnn_list)
        return rnn_dim

    def forward(self, net: Tensor) -> Tensor:
        for rnn in self.rnn_list:
            net = rnn(net)
        return self.head(net[:, -1].contiguous())


@register_module("nbm")
class NBM(Module):
    """reference modules/ml/nbm.py:123-231: per feature tuple, `num_bases` small MLPs (order -> H -> H -> 1, ReLU) shared by all tuples
    of an order, a per-tuple mix of the bases (`featurizer`) and a Linear head.  State keys and shapes are the reference's
    (`bases.<order>.net.<i>.conv.{weight,bias}`, `featurizer.*`, `head.*`; nn.Conv1d's / nn.Linear's init), so checkpoints load both
    ways.  The bases run on the fused kernels of csrc/nbm.hip (`nbm.BasesFn`, one launch per order; nothing of size B D NB H exists),
    the featurizer on `nbm.FeaturizeFn`, the head in f32 on `nbm.HeadFn`.  f32 parameters, f32 logits.  BatchNorm and dropout inside
    the bases, other activations, hidden widths that are not two equal ones inside the kernels' range (a multiple of 8, 8 .. 256),
    orders above 4 and bias = False are refused by name."""

    def __init__(self, input_dim: int, output_dim: int, *, nary: Optional[Dict[str, List[Tuple[int, ...]]]] = None, num_bases: int = 64,
                 bases_dropout: float = 0.0, hidden_units: Optional[List[int]] = None, bias: bool = True, activation: str = "ReLU",
                 batch_norm: bool = False, dropout: float = 0.0):
        super().__init__()
        if hidden_units is None:
            dim = max(32, min(1024, 2 * input_dim))
            hidden_units = 2 * [dim]
        if batch_norm:
            raise NotImplementedError("nbm: batch_norm = True (BatchNorm inside the bases) is not built (DESIGN §8)")
        if 0.0 < dropout < 1.0:
            raise NotImplementedError(f"nbm: dropout = {dropout} inside the bases is not built (DESIGN §8); `bases_dropout` is")
        if activation != "ReLU":
            raise NotImplementedError(f"nbm: activation '{activation}' is not built (DESIGN §8); the basis kernels apply ReLU")
        if not bias:
            raise NotImplementedError("nbm: bias = False is not built (DESIGN §8)")
        hidden_units = list(hidden_units)
        if len(hidden_units) != 2 or hidden_units[0] != hidden_units[1] or not ops.nbm_hidden_ok(hidden_units[0]):
            raise NotImplementedError(f"nbm: hidden_units = {hidden_units} is outside the basis kernels: exactly two equal widths, a multiple "
                                      f"of 8, 8 .. {ops.NBM_MAX_HIDDEN} (DESIGN §8)")
        if num_bases < 1:
            raise ValueError(f"nbm: num_bases = {num_bases}")
        self.input_dim, self.output_dim, self.bias, self.num_bases = input_dim, output_dim, bias, num_bases
        from itertools import combinations

        self.nary = _nbm.check_nary(nary or {"1": list(combinations(range(input_dim), 1))}, input_dim)
        self.bases = nn.ModuleDict({order: _nbm.NBMBlock(int(order), num_bases, hidden_units[0]) for order in self.nary})
        self.bases_dropout = float(bases_dropout)
        self.all_indices: List[Tuple[int, ...]] = []
        for indices in self.nary.values():
            self.all_indices += indices
        self.latent_dim = len(self.all_indices)
        self.featurizer = nn.Conv1d(self.latent_dim * num_bases, self.latent_dim, kernel_size=1, groups=self.latent_dim, bias=True)
        self.head = nn.Linear(self.latent_dim, output_dim, bias=True)
        self._tables: Dict[Any, ops.NbmIndex] = {}

    def _table(self, indices: Sequence[Tuple[int, ...]], width: int, device: torch.device) -> ops.NbmIndex:
        key = (tuple(indices), width, str(device))
        if key not in self._tables:
            self._tables[key] = ops.nbm_index(list(indices), len(indices[0]), width, device)
        return self._tables[key]

    def _flat(self, net: Tensor) -> Tensor:
        if not net.is_cuda:
            raise RuntimeError(f"nbm: the input must live on the HIP device (got {net.device}); there is no CPU path")
        if net.dim() > 2:
            net = net.contiguous().view(len(net), -1)
        return net if net.dtype == torch.float32 else net.float()

    def forward(self, net: Tensor, *, return_features: bool = False) -> Tensor:
        net = self._flat(net)
        if net.shape[1] != self.input_dim:
            raise ValueError(f"nbm: [B, {self.input_dim}] expected, got {tuple(net.shape)}")
        bases = []
        for order, indices in self.nary.items():
            base = self.bases[order](net, self._table(indices, self.input_dim, net.device))
            bases.append(HF.dropout(base, self.bases_dropout, self.training))
        net = bases[0] if len(bases) == 1 else torch.cat(bases, dim=1)  # [B, latent_dim, num_bases]
        net = _nbm.featurize(net, self.featurizer.weight, self.featurizer.bias)
        if return_features:
            return net
        return _nbm.head(net, self.head.weight, self.head.bias)

    def inspect(self, net: Tensor, x_dims: Tuple[int, ...], y_dim: int, *, already_extracted: bool = False) -> Tensor:
        """the contribution of one tuple to one output (modules/ml/nbm.py:201-231): eval mode, the same kernels with D = 1"""
        x_dims = tuple(int(i) for i in x_dims)
        try:
            idx = self.all_indices.index(x_dims)
        except ValueError:
            raise ValueError(f"`x_dims` ({x_dims}) is not in the pre-defined nary")
        order = len(x_dims)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                net = self._flat(net)
                indices = [tuple(range(order))] if already_extracted else [x_dims]
                base = self.bases[str(order)](net, self._table(indices, net.shape[1], net.device))  # [B, 1, num_bases]
                feat = _nbm.featurize(base, self.featurizer.weight[idx:idx + 1], self.featurizer.bias[idx:idx + 1])  # [B, 1]
                return feat * self.head.weight[y_dim, idx]
        finally:
            self.train(was_training)


class VanillaPatchEmbed(Module):
    """reference high_level.py:153-188 — `projection` Conv2d(k = stride = patch)."""

    def __init__(self, img_size: int, patch_size: int, in_channels: int, latent_dim: int = 128,
                 **conv_kwargs: Any):
        super().__init__()
        if img_size % patch_size != 0:
            raise ValueError(f"`img_size` ({img_size}) should be divisible by `patch_size` ({patch_size})")
        self.img_size, self.patch_size = img_size, patch_size
        self.in_channels, self.latent_dim = in_channels, latent_dim
        self.projection = Conv2d(in_channels, latent_dim, kernel_size=patch_size, stride=patch_size,
                                 padding=0, **conv_kwargs)

    @property
    def num_patches(self) -> int:
        return (self.img_size // self.patch_size) ** 2


to_patches: Dict[str, Any] = {"vanilla": VanillaPatchEmbed}


@encoders.register("vit")
class ViTEncoder(Module):
    """reference cv/encoder/transformer.py:17-100, made `IEncoder`-conformant (`encode`,
    `in_channels`, `latent_dim`) so that `cv_clf(encoder="vit")` works — it crashes in the
    reference.  State keys: `to_patches.projection.*`, `encoder.*`, `output_projection`."""

    def __init__(self, *, img_size: int, patch_size: int, in_channels: int, latent_dim: int = 384,
                 to_patches_type: str = "vanilla", to_patches_config: Optional[Dict[str, Any]] = None,
                 num_layers: int = 12, dropout: float = 0.0, drop_path_rate: float = 0.0,
                 norm_type: Optional[str] = "layer", norm_kwargs: Optional[Dict[str, Any]] = None,
                 embedding_norm: Optional[Module] = None, residual_after_norm: bool = False,
                 feedforward_dim_ratio: float = 4.0, attention_kwargs: Optional[Dict[str, Any]] = None,
                 feedforward_kwargs: Optional[Dict[str, Any]] = None, use_head_token: bool = True,
                 head_pooler: Optional[str] = "mean", use_positional_encoding: bool = True,
                 norm_after_head: bool = False, output_dim: Optional[int] = None):
        super().__init__()
        cfg = dict(to_patches_config or {})
        cfg.update(img_size=img_size, patch_size=patch_size, in_channels=in_channels, latent_dim=latent_dim)
        self.to_patches = to_patches[to_patches_type](**cfg)
        attention_kwargs = dict(attention_kwargs or {})
        attention_kwargs.setdefault("bias", True)
        attention_kwargs.setdefault("num_heads", latent_dim // 64)
        self.encoder = MixedStackedEncoder(
            latent_dim, self.to_patches.num_patches, token_mixing_type="attention",
            token_mixing_config=attention_kwargs, channel_mixing_config=feedforward_kwargs,
            num_layers=num_layers, dropout=dropout, drop_path_rate=drop_path_rate, norm_type=norm_type,
            norm_kwargs=norm_kwargs, embedding_norm=embedding_norm, residual_after_norm=residual_after_norm,
            latent_dim_ratio=feedforward_dim_ratio, head_pooler=head_pooler, use_head_token=use_head_token,
            use_positional_encoding=use_positional_encoding, is_vision_positional_encoding=True,
            norm_after_head=norm_after_head,
        )
        self.in_channels, self.latent_dim, self.img_size = in_channels, latent_dim, img_size
        if output_dim is None:
            self.output_projection = None
        else:
            self.output_projection = nn.Parameter((latent_dim ** -0.5) * torch.randn(latent_dim, output_dim))

    def forward(self, net: Tensor, *, hw: Optional[Tuple[int, int]] = None, hwp: Any = None,
                deterministic: bool = False) -> Tensor:
        conv = self.to_patches.projection
        enc = self.encoder
        enc.check_fused_token_assembly()
        pos = enc.pos_encoding.pos_encoding
        psz = self.to_patches.patch_size
        gh, gw = net.shape[-2] // psz, net.shape[-1] // psz
        if net.shape[-1] != self.img_size or net.shape[-2] != self.img_size:
            # non-native resolution: resampled positional grid (api.py:231-267; the caller passes hwp like upstream)
            pos = enc.pos_encoding.interpolate_pos_encoding(gh * gw + enc.pos_encoding.num_head_tokens, hwp)
        tokens = HF.patch_tokens(net, conv.weight, conv.bias, enc.head_token, pos)
        if enc.embedding_norm is not None:
            # CLIP vision tower: LayerNorm before the blocks.  Its output IS the residual stream: f32 like its input, as under the
            # reference's autocast (cv/encoder/transformer.py:60-64).  Rounds 2-5 handed a bf16 copy on and the whole tower ran a
            # bf16 stream: image features 9.2e-3 from fp32 where the reference's own bf16 run sits at 5.7e-3 — found by
            # test_clip_b32_step_vs_oracle (round 6); the small fixture's 2 layers hid it.
            tokens = enc.embedding_norm(tokens)  # (`out_f32`, set by MixedStackedEncoder.__init__)
        if enc.embedding_dropout is not None:
            tokens = enc.embedding_dropout(tokens)
        out = enc.forward_tokens(tokens, hw=(gh, gw), deterministic=deterministic)
        if self.output_projection is not None:
            out = HF.linear(out, self.output_projection.t(), None, out_f32=True)
        return out

    def encode(self, net: Tensor) -> Tensor:
        return self(net)


@register_module("cv_clf")
class VanillaClassifier(Module):
    """reference cv/classifier/vanilla.py:16-66 — `encoder` + `head` Linear; returns
    {"predictions": logits} (fp32 logits, what accelerate's bf16 wrapper hands the loss)."""

    def __init__(self, in_channels: int, num_classes: int, img_size: Optional[int] = None,
                 latent_dim: int = 128, aux_num_classes: Optional[Dict[str, int]] = None, *,
                 encoder: str = "vanilla_1d", encoder_config: Optional[Dict[str, Any]] = None):
        super().__init__()
        if aux_num_classes is not None:
            raise NotImplementedError("auxiliary heads are outside the accelerated hot path")
        self.img_size = img_size
        cfg = dict(encoder_config or {})
        cfg.setdefault("img_size", img_size)
        cfg.setdefault("in_channels", in_channels)
        cfg.setdefault("latent_dim", latent_dim)
        self.encoder = encoders.build(encoder, config=cfg)
        self.head = Linear(latent_dim, num_classes)
        self.head.out_f32 = True
        self.aux_keys = None

    def forward(self, net: Tensor, *, return_latent: bool = False) -> Dict[str, Tensor]:
        latent = self.encoder.encode(net)
        if return_latent:
            return {LATENT_KEY: latent}
        return {PREDICTIONS_KEY: self.head(latent)}


def vit_b16_classifier(num_classes: int = 1000, img_size: int = 224, **encoder_overrides: Any) -> VanillaClassifier:
    """ViT-B/16: latent 768, 12 layers, 12 heads (latent // 64), FF ratio 4, patch 16 — the
    configuration BASELINE.json's metric is quoted on."""
    cfg: Dict[str, Any] = dict(patch_size=16, latent_dim=768, num_layers=12)
    cfg.update(encoder_overrides)
    return VanillaClassifier(3, num_classes, img_size, cfg["latent_dim"], encoder="vit", encoder_config=cfg)


# ---------------------------------------------------------------------------------------------
# text transformer / CLIP towers
# ---------------------------------------------------------------------------------------------


@register_module("tet")
class TeTEncoder(Module):
    """reference nlp/encoder/transformer.py:17-99 — `encoder` (MixedStackedEncoder without head token, learned
    positional encoding) and, with `use_triu_attn_mask`, the bool buffer `attention_mask` = triu(1) (True = masked).
    On the HIP path the causal mask is a kernel flag (`causal=True`), the buffer exists for state_dict parity."""

    def __init__(self, latent_dim: int = 384, context_length: int = 77, *, use_triu_attn_mask: bool = False,
                 num_layers: int = 12, dropout: float = 0.0, drop_path_rate: float = 0.0,
                 norm_position: str = "pre_norm", norm_type: Optional[str] = "layer",
                 norm_kwargs: Optional[Dict[str, Any]] = None, embedding_norm: Optional[Module] = None,
                 embedding_dropout: Optional[float] = None, residual_after_norm: bool = False,
                 feedforward_dim_ratio: float = 4.0, attention_kwargs: Optional[Dict[str, Any]] = None,
                 feedforward_kwargs: Optional[Dict[str, Any]] = None, use_positional_encoding: bool = True,
                 head_pooler: Optional[str] = None, no_head_norm: Optional[bool] = None,
                 norm_after_head: bool = False):
        super().__init__()
        if not use_triu_attn_mask:
            self.attention_mask = None
        else:
            mask = torch.ones(context_length, context_length, dtype=torch.bool).triu_(1)
            self.register_buffer("attention_mask", mask)
        attention_kwargs = dict(attention_kwargs or {})
        attention_kwargs.setdefault("bias", True)
        attention_kwargs.setdefault("num_heads", 6)
        self.encoder = MixedStackedEncoder(
            latent_dim, context_length, token_mixing_type="attention", token_mixing_config=attention_kwargs,
            channel_mixing_config=feedforward_kwargs, num_layers=num_layers, dropout=dropout,
            drop_path_rate=drop_path_rate, norm_position=norm_position, norm_type=norm_type, norm_kwargs=norm_kwargs,
            embedding_norm=embedding_norm, embedding_dropout=embedding_dropout,
            residual_after_norm=residual_after_norm, latent_dim_ratio=feedforward_dim_ratio, use_head_token=False,
            head_pooler=head_pooler, use_positional_encoding=use_positional_encoding,
            is_vision_positional_encoding=False, no_head_norm=no_head_norm, norm_after_head=norm_after_head,
        )

    def forward_embedded(self, tokens: Tensor, *, apply_head: bool = True, clip_skip: int = 0) -> Tensor:
        """`tokens` already carry the positional encoding (fused into the embedding lookup kernel)."""
        if self.encoder.embedding_norm is not None:
            tokens = self.encoder.embedding_norm(tokens)
        if self.encoder.embedding_dropout is not None:
            tokens = self.encoder.embedding_dropout(tokens)
        return self.encoder.forward_tokens(tokens, causal=self.attention_mask is not None, clip_skip=clip_skip,
                                           apply_head=apply_head)

    def forward(self, net: Tensor, mask: Optional[Tensor] = None, *, apply_head: bool = True, clip_skip: int = 0,
                **kwargs: Any) -> Tensor:
        net = self.encoder.pre_process(net, **kwargs)
        if mask is None:
            return self.encoder.forward_tokens(net, causal=self.attention_mask is not None, clip_skip=clip_skip,
                                               apply_head=apply_head)
        t = net.shape[1]
        if t != mask.shape[0]:
            mask = mask[:t, :t]
        return self.encoder.forward_tokens(net, mask=mask, clip_skip=clip_skip, apply_head=apply_head)


@register_module("clip")
class CLIP(Module):
    """reference multimodal/clip.py:22-256 + multimodal/schema.py:10-32 (`IPerceptor`): ViT image tower
    (patch conv without bias, embedding LayerNorm, quick GELU, LayerNorm after the head token, `output_projection`)
    and causal text tower (nn.Embedding + learned positions, quick GELU, EOT pooling, `text_projection`), both
    L2-normalised.  State keys: `logit_scale`, `vit.*`, `token_embedding.weight`, `text_transformer.*`,
    `text_projection.*`."""

    def __init__(self, img_size: int = 224, latent_dim: int = 512, *, use_vision: bool = True, in_channels: int = 3,
                 vision_latent_dim: int = 768, vision_patch_size: int = 32, vision_num_heads: int = 12,
                 vision_num_layers: int = 12, vision_norm_eps: float = 1.0e-5,
                 vision_feedforward_activation: str = "quick_gelu", use_text: bool = True, vocab_size: int = 49408,
                 context_length: int = 77, use_text_triu_attn_mask: bool = True,
                 token_type_size: Optional[int] = None, text_latent_dim: int = 512, text_padding_idx: int = 0,
                 use_text_embedding_norm: bool = False, text_embedding_dropout: Optional[bool] = None,
                 text_dropout: float = 0.0, text_num_heads: int = 8, text_num_layers: int = 12,
                 text_norm_position: str = "pre_norm", text_norm_eps: float = 1.0e-5,
                 text_feedforward_activation: str = "quick_gelu", text_head_pooler: Optional[str] = None):
        super().__init__()
        if token_type_size is not None or text_dropout > 0.0 or text_head_pooler is not None:
            raise NotImplementedError("token-type embeddings / text dropout / text poolers are outside the hot path")
        self.img_size, self.context_length = img_size, context_length
        self.logit_scale = nn.Parameter(torch.tensor(math.log(1 / 0.07)))
        if not use_vision:
            self.vit = None
        else:
            self.vision_latent_dim = vision_latent_dim
            self.vit = ViTEncoder(
                img_size=img_size, patch_size=vision_patch_size, in_channels=in_channels,
                latent_dim=vision_latent_dim, to_patches_config={"bias": False}, num_layers=vision_num_layers,
                norm_kwargs={"eps": vision_norm_eps}, embedding_norm=LayerNorm(vision_latent_dim, vision_norm_eps),
                attention_kwargs={"num_heads": vision_num_heads},
                feedforward_kwargs={"activation": vision_feedforward_activation}, norm_after_head=True,
                output_dim=latent_dim,
            )
            self.vit.encoder.head_only_tail = False  # the towers keep the full last block (measured and tuned as they are)
        if not use_text:
            self.token_embedding = self.token_type_embedding = self.text_transformer = None
            self.text_latent_dropout = self.text_projection = None
        else:
            self.text_num_layers, self.text_latent_dim = text_num_layers, text_latent_dim
            self.token_embedding = nn.Embedding(vocab_size, text_latent_dim, padding_idx=text_padding_idx)
            self.token_type_embedding = None
            self.text_transformer = TeTEncoder(
                text_latent_dim, context_length, use_triu_attn_mask=use_text_triu_attn_mask,
                num_layers=text_num_layers, dropout=text_dropout, norm_position=text_norm_position,
                norm_kwargs={"eps": text_norm_eps},
                embedding_norm=LayerNorm(text_latent_dim, text_norm_eps) if use_text_embedding_norm else None,
                embedding_dropout=text_embedding_dropout, attention_kwargs={"num_heads": text_num_heads},
                feedforward_kwargs={"activation": text_feedforward_activation}, head_pooler=text_head_pooler,
            )
            self.text_head_pooler = text_head_pooler
            self.text_latent_dropout = nn.Dropout(text_dropout)
            self.text_projection = HijackLinear(text_latent_dim, latent_dim)
        # (The contrastive loss makes the per-sample gradients of the SHARED parameters — head token, positional encodings, the
        # embedding LayerNorm — nearly cancel in the batch sum; with the residual-gradient stream rounded to one bf16 word twice per
        # block they came out 1.3-1.5 x further from fp32 than the reference's own bf16 run, whose stream gradient is f32:
        # tests/test_gpu_clip.py::test_clip_b32_step_vs_oracle.  That test is why fused.GRAD_STREAM_WORDS is 2 for every f32 stream.)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """reference clip.py:188-207"""
        if self.token_embedding is None:
            return
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        tld = self.text_latent_dim
        text_encoder = self.text_transformer.encoder
        nn.init.normal_(text_encoder.pos_encoding.pos_encoding, std=0.01)
        proj_std = (tld ** -0.5) * ((2 * self.text_num_layers) ** -0.5)
        attn_std, fc_std = tld ** -0.5, (2 * tld) ** -0.5
        for block in text_encoder.mixing_blocks:
            attn, mlp = block.token_mixing.net, block.channel_mixing.net
            nn.init.normal_(attn.in_w, std=attn_std)
            nn.init.normal_(attn.out_linear.weight, std=proj_std)
            nn.init.normal_(mlp[0].weight, std=fc_std)
            nn.init.normal_(mlp[3].weight, std=proj_std)
        nn.init.normal_(self.text_projection.weight, std=tld ** -0.5)
        nn.init.zeros_(self.text_projection.bias)

    def encode_image(self, image: Tensor) -> Tensor:
        if self.vit is None:
            raise ValueError("`vit` is not initialized, please set `use_vision=True` when initializing `CLIP`")
        return HF.l2_normalize(self.vit(image, deterministic=True))

    def encode_text(self, indices: Tensor, *, apply_pooling: bool = True, deterministic: bool = True,
                    clip_skip: int = 0) -> Tensor:
        if self.token_embedding is None:
            raise ValueError("`token_embedding` is not initialized, please set `use_text=True` when "
                             "initializing `CLIP`")
        enc = self.text_transformer.encoder
        pos = enc.pos_encoding.pos_encoding
        pad = self.token_embedding.padding_idx
        # embedding lookup + positional add in one gather kernel -> f32 stream [B, T, D]
        enc.check_fused_token_assembly()
        tokens = HF.embedding(indices, self.token_embedding.weight, pos, -1 if pad is None else pad)
        if not apply_pooling:
            return self.text_transformer.forward_embedded(tokens, clip_skip=clip_skip)
        net = self.text_transformer.forward_embedded(tokens, clip_skip=clip_skip, apply_head=False)
        # EOT pooling BEFORE the head LayerNorm (row-wise, so LN(x)[b, i] == LN(x[b, i])): B rows instead of B*T
        pooled = HF.gather_rows(net, indices.argmax(dim=-1))
        pooled = enc.post_process(pooled)
        if getattr(self.text_projection, "hook", None) is not None:
            feat = _hooked_linear(self.text_projection, pooled, out_f32=True)
        else:
            feat = HF.linear(pooled, self.text_projection.weight, self.text_projection.bias, out_f32=True)
        return HF.l2_normalize(feat)

    def forward(self, image: Tensor, text: Tensor) -> Tensor:
        """logits_per_image (reference multimodal/schema.py:25-30), fp32 similarity kernel"""
        from .contrastive import similarity_logits

        return similarity_logits(self.encode_image(image), self.encode_text(text), self.logit_scale)

    # Round 5: the two towers are independent until the similarity matrix, and their kernels are small (ViT-B/32: 50 tokens, the text
    # tower: 77 tokens x 512 channels — a half-batch GEMM is ~200 tiles for 512 slots).  `towers_side_by_side` runs the text tower on
    # lane 1 while the image tower runs on the caller's stream, each as ONE batch pipeline (`stack_slices` = 1): two different kernel
    # streams in flight instead of two slices of one tower after the other, half as many launches (profiles/r05/clip_towers_ab.txt).
    towers_side_by_side = os.environ.get("CFHIP_CLIP_TOWERS", "1") != "0"

    def _encode_both(self, image: Tensor, text: Tensor) -> Tuple[Tensor, Tensor]:
        side = HF.SideStream.fork(1) if (self.towers_side_by_side and image.is_cuda and self.vit is not None
                                         and self.text_transformer is not None and torch.is_grad_enabled()) else None
        if side is None or side == HF.cur_stream():
            return self.encode_image(image), self.encode_text(text)
        main = HF.cur_stream()
        keep = (self.vit.encoder.stack_slices if hasattr(self.vit.encoder, "stack_slices") else None,
                getattr(self.text_transformer.encoder, "stack_slices", None))
        # (forward slices, backward slices): in the forward the weight-gradient lane is idle, so the image tower may still take it for a
        # second batch slice (CFHIP_CLIP_TOWERS=2: three forward pipelines); the backward keeps one pipeline per tower + the dW lane
        self.vit.encoder.stack_slices = (2, 1) if os.environ.get("CFHIP_CLIP_TOWERS", "1") == "2" else 1
        self.text_transformer.encoder.stack_slices = 1
        try:
            with HF.on_stream(side):
                txt = self.encode_text(text)
            img = self.encode_image(image)
        finally:
            self.vit.encoder.stack_slices, self.text_transformer.encoder.stack_slices = keep
        HF.rec_wait_stream(main, side)
        txt.record_stream(main)  # allocated under lane 1, consumed on the caller's stream
        return img, txt

    def contrastive_loss(self, image: Tensor, text: Tensor, group: Any = None) -> Tensor:
        """Symmetric InfoNCE over the local batch against the embeddings of every rank (contrastive.py; the
        reference has no training loss for CLIP: new design, parity unpinned)."""
        from .contrastive import clip_contrastive_loss

        img, txt = self._encode_both(image, text)
        return clip_contrastive_loss(img, txt, self.logit_scale, group)


# ---------------------------------------------------------------------------------------------
# UNet residual blocks (reference modules/core/convs/residual.py:86-253, hijacks.py:64-65)
# ---------------------------------------------------------------------------------------------


class HijackConv2d(_HijackMixin, nn.Conv2d):
    """reference hijacks.py:64-65 (`conv_nd(2, ...)`): nn.Conv2d parameters (`weight`, `bias`), groups 1, zero padding"""

    def forward(self, net: Tensor) -> Tensor:  # type: ignore
        if (self.groups != 1 or self.padding_mode != "zeros" or self.stride[0] != self.stride[1]
                or self.padding[0] != self.padding[1] or self.dilation[0] != self.dilation[1]
                or self.kernel_size[0] != self.kernel_size[1] or isinstance(self.padding, str)):
            raise NotImplementedError("only square, zero-padded, ungrouped convolutions are on the accelerated hot path")
        inp = net
        if _native_lora(self.hook):
            return self.hook.conv_forward(self, net)
        if self.hook is not None:
            inp = self.hook.before_forward(inp)
        net = HF.conv2d(inp, self.weight, self.bias, self.stride[0], self.padding[0], self.dilation[0])
        if self.hook is not None:
            net = self.hook.after_forward(inp, net)
        return net


class GroupNorm(nn.GroupNorm):
    """nn.GroupNorm (`make_norm`, residual.py:194) on `cfhip_groupnorm_fwd/bwd`; `add` / `silu` expose the kernel's
    fused time-embedding add in front and SiLU behind; `scale_shift=(scale, shift)` (f32 [B, C] each) is the scale-shift
    form `norm(net) * (1 + scale) + shift` of residual.py:236-239, still one kernel each way."""

    def forward(self, net: Tensor, *, add: Optional[Tensor] = None, silu: bool = False,  # type: ignore
                scale_shift: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
        if not self.affine:
            raise NotImplementedError("GroupNorm without affine parameters is outside the accelerated hot path")
        weight, bias = self.weight, self.bias
        if scale_shift is not None:
            weight, bias = HF.scale_shift_affine(self.weight, self.bias, scale_shift[0], scale_shift[1])
        return HF.group_norm(net, weight, bias, self.num_groups, self.eps, add, silu)


def _plain_children(mod: Module) -> bool:
    """No user hook anywhere under `mod` (the `hook=` of the Hijack layers, nn.Module forward hooks, pruners): what a taped node
    (functional.run_taped) requires, because a hook's torch ops would fall out of the node's gradient."""
    for m in mod.modules():
        if m._forward_hooks or m._forward_pre_hooks or getattr(m, "hook", None) is not None:
            return False
        if getattr(m, "pruner", None) is not None or getattr(m, "pruner1", None) is not None:
            return False
    return True


_tape_break_warned = [False]


def _tape_broke(mod: Module, err: Exception) -> None:
    mod._tape_ok = False
    if not _tape_break_warned[0]:
        _tape_break_warned[0] = True
        print(f"cfhip: {type(mod).__name__} runs as separate autograd nodes from now on ({err})", file=sys.stderr)


class ResDownsample(Module):
    """reference residual.py:86-117: conv3x3 stride 2 (`use_conv`) or 2x2 average pooling"""

    def __init__(self, in_channels: int, use_conv: bool, *, signal_dim: int = 2, out_channels: Optional[int] = None,
                 padding: int = 1):
        super().__init__()
        if signal_dim != 2:
            raise NotImplementedError("only 2-D signals are on the accelerated hot path")
        out_channels = out_channels or in_channels
        if not use_conv:
            if in_channels != out_channels:
                raise ValueError("`in_channels` should be equal to `out_channels` when `use_conv` is set to False")
            self.net: Module = nn.AvgPool2d(kernel_size=2, stride=2)
        else:
            self.net = HijackConv2d(in_channels, out_channels, 3, stride=2, padding=padding)

    def forward(self, net: Tensor) -> Tensor:
        if isinstance(self.net, nn.AvgPool2d):
            return HF.avg_pool2(net)
        return self.net(net)


class ResUpsample(Module):
    """reference residual.py:120-151: nearest x2, then an optional conv3x3"""

    def __init__(self, in_channels: int, use_conv: bool, *, signal_dim: int = 2, out_channels: Optional[int] = None,
                 padding: int = 1):
        super().__init__()
        if signal_dim != 2:
            raise NotImplementedError("only 2-D signals are on the accelerated hot path")
        self.signal_dim = signal_dim
        self.conv = HijackConv2d(in_channels, out_channels or in_channels, 3, padding=padding) if use_conv else None

    def forward(self, net: Tensor) -> Tensor:
        net = HF.upsample2(net)
        return net if self.conv is None else self.conv(net)


class ResidualBlockWithTimeEmbedding(Module):
    """reference residual.py:154-253: GN(32) -> SiLU -> [resample] -> conv3x3 -> (+ Linear(SiLU(t))) -> GN(32) -> SiLU ->
    conv3x3 (zero-initialised) -> + shortcut(inp).  State keys: `norm1.*`, `conv1.*`, `time_embedding.*`, `norm2.*`,
    `conv2.*`, `shortcut.*`.  GroupNorm, the time-embedding add in front of norm2 (or, with `use_scale_shift_norm`, the
    `norm2(net) * (1 + scale) + shift` modulation behind it) and both SiLUs are two fused kernels each way; `dropout`
    is the Philox kernel of `Dropout`.  `use_checkpoint=True` recomputes the block in backward like the reference
    (residual.py:217-222).  (`safe_clip_` only acts on non-finite values and is omitted.)"""

    def __init__(self, in_channels: int, out_channels: Optional[int] = None, *, signal_dim: int = 2,
                 dropout: float = 0.0, norm_eps: float = 1.0e-6, use_conv_shortcut: bool = False,
                 integrate_upsample: bool = False, integrate_downsample: bool = False,
                 time_embedding_channels: int = 512, use_scale_shift_norm: bool = False,
                 use_checkpoint: bool = False):
        super().__init__()
        if signal_dim != 2:
            raise NotImplementedError("only 2-D signals are on the accelerated hot path")
        self.in_channels = in_channels
        out_channels = out_channels or in_channels
        self.out_channels = out_channels
        self.use_conv_shortcut, self.use_scale_shift_norm = use_conv_shortcut, use_scale_shift_norm
        self.use_checkpoint = use_checkpoint  # residual.py:217-222: recompute the block in backward (HF.gradient_checkpoint)
        self.resample = integrate_upsample or integrate_downsample
        if not self.resample:
            self.inp_resample = self.net_resample = None
        elif integrate_upsample:
            self.inp_resample = ResUpsample(in_channels, False)
            self.net_resample = ResUpsample(in_channels, False)
        else:
            self.inp_resample = ResDownsample(in_channels, False)
            self.net_resample = ResDownsample(in_channels, False)
        self.activation = nn.SiLU()
        self.norm1 = GroupNorm(num_groups=32, num_channels=in_channels, eps=norm_eps)
        self.conv1 = HijackConv2d(in_channels, out_channels, 3, 1, 1)
        if time_embedding_channels > 0:
            self.time_embedding = HijackLinear(time_embedding_channels,
                                               2 * out_channels if use_scale_shift_norm else out_channels)
        self.norm2 = GroupNorm(num_groups=32, num_channels=out_channels, eps=norm_eps)
        self.dropout = Dropout(dropout)
        self.conv2 = HijackConv2d(out_channels, out_channels, 3, 1, 1)
        with torch.no_grad():  # zero_module (modules/common.py:177-180)
            for p in self.conv2.parameters():
                p.zero_()
        if in_channels != out_channels:
            self.shortcut = (HijackConv2d(in_channels, out_channels, 3, 1, 1) if use_conv_shortcut
                             else HijackConv2d(in_channels, out_channels, 1, 1, 0))

    def forward(self, net: Tensor, time_net: Optional[Tensor] = None) -> Tensor:
        if self.use_checkpoint:  # residual.py:210-216 (a no-op without grad mode)
            if time_net is None:
                return HF.gradient_checkpoint(lambda n: self._forward(n, None), (net,), self.parameters(), True)
            return HF.gradient_checkpoint(self._forward, (net, time_net), self.parameters(), True)
        if self._taped(net):  # the whole block as ONE autograd node (functional.run_taped)
            tensors = (net,) + (() if time_net is None else (time_net,)) + tuple(self.parameters())
            try:
                return HF.run_taped(lambda: self._forward(net, time_net), tensors)
            except HF.TapeBreak as err:
                _tape_broke(self, err)
        return self._forward(net, time_net)

    _tape_ok = True

    def _taped(self, net: Tensor) -> bool:
        """the configurations whose op sequence is Functions only: no scale-shift modulation (torch.chunk), no active dropout
        (its Philox draws would repeat on a fall-back), no hooks"""
        return (HF.TAPED_NODES[0] and self._tape_ok and net.is_cuda and torch.is_grad_enabled() and not self.use_scale_shift_norm
                and not (self.training and 0.0 < self.dropout.p < 1.0) and _plain_children(self))

    def _forward(self, net: Tensor, time_net: Optional[Tensor] = None) -> Tensor:
        inp = net
        net = self.norm1(net, silu=True)
        if self.inp_resample is not None:
            inp = self.inp_resample(inp)
            net = self.net_resample(net)
        net = self.conv1(net)
        if self.in_channels != self.out_channels:
            inp = self.shortcut(inp)
        add = scale_shift = None
        if time_net is not None:
            t = HF.time_pre_lookup(self, time_net)  # all blocks' projections in one launch at the top of the UNet's forward
            if t is None:
                t = HF.silu_f32(time_net)
                if getattr(self.time_embedding, "hook", None) is not None:
                    t = _hooked_linear(self.time_embedding, t, out_f32=True)
                else:
                    t = HF.linear(t, self.time_embedding.weight, self.time_embedding.bias, out_f32=True)  # [B, Cout] / [B, 2 Cout]
            if self.use_scale_shift_norm:
                scale_shift = tuple(torch.chunk(t, 2, dim=1))  # residual.py:236-239
            else:
                add = t
        net = self.norm2(net, add=add, silu=True, scale_shift=scale_shift)
        net = self.dropout(net)
        net = self.conv2(net)
        return HF.add(inp, net)


# ---------------------------------------------------------------------------------------------
# UNet self attention over pixels (reference attentions.py:373-460), the `use_spatial_transformer=False` UNets
# ---------------------------------------------------------------------------------------------


class MultiHeadSpatialAttention(Module):
    """reference attentions.py:373-460: GroupNorm(32) -> 1x1 conv1d to 3C -> per-head softmax(q^T k / sqrt(hd)) v over
    the H*W pixels -> 1x1 conv1d (zero-initialised) -> + input.  State keys `norm.*`, `to_qkv.{weight [3C, C, 1], bias}`,
    `to_out.*` as in the reference.  Here the pixels become token-major rows once ([B, HW, C]), the two 1x1 convolutions
    are GEMMs over them (three for q / k / v: each reads the ROWS of `to_qkv.weight` that belong to it, so no activation
    is permuted — `split_qkv_before_heads=False`, the reference default, interleaves q / k / v per head along the 3C
    output channels) and the attention is the flash kernel for general head widths; the reference scales q and k by
    hd^-1/4 each, the kernel applies hd^-1/2 to their product."""

    def __init__(self, in_channels: int, *, num_heads: Optional[int] = 1, num_head_channels: Optional[int] = None,
                 split_qkv_before_heads: bool = False, use_checkpoint: bool = False):
        super().__init__()
        self.in_channels = in_channels
        if num_head_channels is None:
            if num_heads is None:
                raise ValueError("either `num_heads` or `num_head_channels` should be provided")
            self.num_heads = num_heads
        else:
            self.num_heads = in_channels // num_head_channels
        head_dim = in_channels // self.num_heads
        if head_dim * self.num_heads != in_channels or head_dim % 8 != 0 or head_dim > 192:
            raise NotImplementedError(f"head width {head_dim} is outside the attention kernels (multiples of 8 up to 192)")
        self.split_qkv_before_heads = split_qkv_before_heads
        self.use_checkpoint = use_checkpoint
        self.norm = GroupNorm(32, in_channels)
        self.to_qkv = nn.Conv1d(in_channels, in_channels * 3, 1)
        self.to_out = nn.Conv1d(in_channels, in_channels, 1)
        with torch.no_grad():  # zero_module
            for p in self.to_out.parameters():
                p.zero_()

    def forward(self, net: Tensor) -> Tensor:
        if self.use_checkpoint:
            return HF.gradient_checkpoint(self._forward, (net,), self.parameters(), True)
        return self._forward(net)

    def _qkv_rows(self) -> Tuple[List[Tensor], List[Tensor]]:
        c, h = self.in_channels, self.num_heads
        hd = c // h
        w, b = self.to_qkv.weight.view(3 * c, c), self.to_qkv.bias
        if self.split_qkv_before_heads:  # channels [q (all heads) | k | v]
            return [w[i * c:(i + 1) * c] for i in range(3)], [b[i * c:(i + 1) * c] for i in range(3)]
        w4, b3 = w.view(h, 3, hd, c), b.view(h, 3, hd)  # channels [head][q | k | v][hd]
        return [w4[:, i].reshape(c, c) for i in range(3)], [b3[:, i].reshape(c) for i in range(3)]

    def _forward(self, net: Tensor) -> Tensor:
        if getattr(self.to_qkv, "hook", None) is not None or getattr(self.to_out, "hook", None) is not None:
            # (the per-head row split of the packed projection has no adapter form; the zoo UNet uses spatial transformers)
            raise NotImplementedError("MultiHeadSpatialAttention: a hook on `to_qkv` / `to_out` is outside the accelerated hot path")
        b, c, h, w = net.shape
        tokens = HF.nchw_to_tokens(self.norm(net))  # [B, HW, C]
        ws, bs = self._qkv_rows()
        q, k, v = (HF.linear(tokens, wi, bi) for wi, bi in zip(ws, bs))
        o = HF.attention_core(q, k, v, self.num_heads, None, False, c // self.num_heads)
        out = HF.linear(o, self.to_out.weight.view(c, c), self.to_out.bias)
        return HF.add(net, HF.tokens_to_nchw(out, h, w))


# ---------------------------------------------------------------------------------------------
# UNet spatial transformer (reference attentions.py:498-569, mixed_stacks/api.py:766-893)
# ---------------------------------------------------------------------------------------------


FUSE_SELF_ATTENTION_QKV = True  # CrossAttention without a context: to_q | to_k | to_v as one GEMM when their weights are adjacent


class CrossAttention(Module):
    """reference attentions.py:498-569: `to_q` / `to_k` / `to_v` (HijackLinear, no bias), `out_linear.0` (HijackLinear)
    + Dropout; heads of `head_dim` channels (any multiple of 8 up to 192), context = the input when None."""

    def __init__(self, *, query_dim: int, context_dim: Optional[int] = None, num_heads: int = 8, head_dim: int = 64,
                 dropout: float = 0.0):
        super().__init__()
        self.has_context = context_dim is not None
        latent_dim = head_dim * num_heads
        context_dim = context_dim or query_dim
        self.num_heads, self.head_dim = num_heads, head_dim
        self.to_q = HijackLinear(query_dim, latent_dim, bias=False)
        self.to_k = HijackLinear(context_dim, latent_dim, bias=False)
        self.to_v = HijackLinear(context_dim, latent_dim, bias=False)
        self.out_linear = nn.Sequential(HijackLinear(latent_dim, query_dim), Dropout(dropout))

    def _plain_projections(self) -> bool:
        """to_q / to_k / to_v are full-rank, hook-free, bias-free Linear layers (what the packed projection replaces)"""
        return all(type(m) is HijackLinear and getattr(m, "hook", None) is None and m.bias is None
                   for m in (self.to_q, self.to_k, self.to_v))

    def forward(self, net: Tensor, *, context: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                residual: Optional[Tensor] = None) -> Tensor:
        keep = None
        if mask is not None:  # [B*H, Tq, Tk] bool, True = masked (the reference inverts it before sdp_attn)
            b = net.shape[0]
            keep = (~mask).view(b, self.num_heads, mask.shape[-2], mask.shape[-1]).to(torch.uint8)
        if context is None and FUSE_SELF_ATTENTION_QKV and self._plain_projections() and HF.qkv_weights_adjacent(
                self.to_q.weight, self.to_k.weight, self.to_v.weight):
            # self attention, the three projection weights back to back in the arena: one packed projection GEMM
            qkv = HF.qkv_linear(net, self.to_q.weight, self.to_k.weight, self.to_v.weight)
            o = HF.packed_self_attention(qkv, self.num_heads, keep, False, 0.0, self.head_dim)
        else:
            q = self.to_q(net)
            if context is None:
                context = net
            k, v = self.to_k(context), self.to_v(context)
            o = HF.attention_core(q, k, v, self.num_heads, keep, False, self.head_dim)
        lin, drop = self.out_linear[0], self.out_linear[1]
        hooked = getattr(lin, "hook", None) is not None
        if self.training and 0.0 < drop.p < 1.0:  # attentions.py:517-521: Linear -> Dropout, then the caller's residual
            out = drop(_hooked_linear(lin, o) if hooked else HF.linear(o, lin.weight, lin.bias))
            return out if residual is None else HF.add(residual, out)
        if hooked:
            return _hooked_linear(lin, o, residual=residual)
        return HF.linear(o, lin.weight, lin.bias, residual=residual)


class SpatialTransformerBlock(Module):
    """reference mixed_stacks/api.py:766-827: LN -> self attention -> +x; LN -> cross attention(context) -> +x;
    LN -> GEGLU feed-forward -> +x (the residual adds ride in the GEMM epilogues); `use_checkpoint=True` recomputes
    the block in backward.  `setup_hooks(tome_info=...)` merges tokens around the three lines at inference (csrc/tome.hip, DESIGN
    §3.5e); the constructor's `hooks_kwargs` and the style-reference hooks are not built."""

    def __init__(self, query_dim: int, num_heads: int, head_dim: int, *, dropout: float = 0.0,
                 context_dim: Optional[int] = None, feedforward_multiplier: float = 4.0,
                 feedforward_activation: str = "geglu", use_checkpoint: bool = False,
                 hooks_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__()
        if hooks_kwargs:
            raise NotImplementedError("SpatialTransformer hooks are outside the accelerated hot path")
        self.attn1 = CrossAttention(query_dim=query_dim, num_heads=num_heads, head_dim=head_dim, dropout=dropout)
        self.ff = FeedForward(query_dim, round(query_dim * feedforward_multiplier), dropout,
                              activation=feedforward_activation, add_last_dropout=False)
        self.attn2 = CrossAttention(query_dim=query_dim, context_dim=context_dim, num_heads=num_heads,
                                    head_dim=head_dim, dropout=dropout)
        self.norm1, self.norm2, self.norm3 = LayerNorm(query_dim), LayerNorm(query_dim), LayerNorm(query_dim)
        self.use_checkpoint = use_checkpoint
        self.tome_info: Optional[Dict[str, Any]] = None

    def setup_hooks(self, *, tome_info: Optional[Dict[str, Any]] = None, style_reference_states: Optional[Dict[str, Any]] = None) -> None:
        """SpatialTransformerHooks.setup (api.py:654-677): `tome_info` (keys and defaults of tome.TOME_DEFAULTS, optional `seed`)
        switches token merging on for this block's inference forward, None switches it off"""
        self.tome_info = _checked_hooks(tome_info, style_reference_states)

    def forward(self, net: Tensor, context: Optional[Tensor] = None) -> Tensor:
        if self.tome_info is not None:
            out = self._tome_forward(net, context)
            if out is not None:
                return out
        if self.use_checkpoint:  # mixed_stacks/api.py:806-813 (a no-op without grad mode)
            if context is None:
                return HF.gradient_checkpoint(lambda n: self._forward(n, None), (net,), self.parameters(), True)
            return HF.gradient_checkpoint(self._forward, (net, context), self.parameters(), True)
        return self._forward(net, context)

    def _forward(self, net: Tensor, context: Optional[Tensor] = None) -> Tensor:
        # every `residual=net` below is the tensor the LayerNorm in the same line has just read, and the GEMM that adds it back consumes
        # that LayerNorm's output: the three gradient fan-ins of a block ride in the LayerNorm backward kernels (functional.fanin_links)
        with HF.fanin_links():
            net = self.attn1(self.norm1(net), residual=net)
            net = self.attn2(self.norm2(net), context=context, residual=net)
            return self.ff(self.norm3(net), residual=net)

    def _tome_forward(self, net: Tensor, context: Optional[Tensor]) -> Optional[Tensor]:
        """SpatialTransformerHooks.forward with `tome_info` (api.py:679-685): net = u(f(m(norm(net)))) + net three times, m / u the
        identity where the line's `merge_*` flag is off (that line then keeps its GEMM residual epilogue).  A merged line runs
        attention / feed-forward on N - r rows and ends in the unmerge + residual kernel.  None: the gate is closed or r <= 0, the
        caller takes the plain path.  Forward only."""
        info = self.tome_info
        if torch.is_grad_enabled() and (net.requires_grad or (context is not None and context.requires_grad)
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("token merging is forward only (DESIGN §8: no backward through merge / unmerge): run a block with "
                                      "`tome_info` under torch.no_grad(), or switch it off with setup_hooks()")
        sizes = _tome.merge_sizes(net.shape[1], info)
        if sizes is None:
            return None
        tm = _tome.TokenMerge(net, info, sizes)
        if info["merge_attn"]:
            net = tm.unmerge_add(self.attn1(tm.merge(self.norm1(net))), net)
        else:
            net = self.attn1(self.norm1(net), residual=net)
        if info["merge_crossattn"]:
            net = tm.unmerge_add(self.attn2(tm.merge(self.norm2(net)), context=context), net)
        else:
            net = self.attn2(self.norm2(net), context=context, residual=net)
        if info["merge_mlp"]:
            return tm.unmerge_add(self.ff(tm.merge(self.norm3(net))), net)
        return self.ff(self.norm3(net), residual=net)


def _checked_hooks(tome_info: Optional[Dict[str, Any]], style_reference_states: Optional[Dict[str, Any]]) -> Optional[Dict[str, Any]]:
    if style_reference_states is not None:
        raise NotImplementedError("`style_reference_states` (the style-reference hooks of SpatialTransformerHooks) is not built: DESIGN §8")
    return _tome.setup_tome_info(tome_info)


def _setup_block_hooks(root: Module, tome_info: Optional[Dict[str, Any]], style_reference_states: Optional[Dict[str, Any]]) -> None:
    _checked_hooks(tome_info, style_reference_states)  # (refusals hold for a model without SpatialTransformer blocks too)
    for m in root.modules():
        if isinstance(m, SpatialTransformerBlock):
            m.setup_hooks(tome_info=tome_info, style_reference_states=style_reference_states)


class SpatialTransformer(Module):
    """reference mixed_stacks/api.py:830-893: GroupNorm(32, eps 1e-6) -> to_latent (1x1 conv or Linear) -> tokens
    [B, HW, C] -> blocks -> from_latent (zero-initialised) -> + input.  A 1x1 convolution over NCHW is a Linear over
    the token-major rows, so the NCHW <-> token-major transposes happen once on the way in and once on the way out."""

    def __init__(self, in_channels: int, num_heads: int, head_dim: int, *, num_layers: int = 1, dropout: float = 0.0,
                 context_dim: Optional[int] = None, use_linear: bool = False, use_checkpoint: bool = False,
                 hooks_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__()
        self.norm = GroupNorm(32, in_channels, 1.0e-6, affine=True)
        self.use_linear = use_linear
        latent_channels = num_heads * head_dim
        if not use_linear:
            self.to_latent: Module = HijackConv2d(in_channels, latent_channels, 1, 1, 0)
        else:
            self.to_latent = HijackLinear(in_channels, latent_channels)
        self.blocks = nn.ModuleList([
            SpatialTransformerBlock(latent_channels, num_heads, head_dim, dropout=dropout, context_dim=context_dim,
                                    use_checkpoint=use_checkpoint, hooks_kwargs=hooks_kwargs)
            for _ in range(num_layers)
        ])
        self.from_latent: Module = (HijackConv2d(latent_channels, in_channels, 1, 1, 0) if not use_linear
                                    else HijackLinear(in_channels, latent_channels))
        with torch.no_grad():  # zero_module
            for p in self.from_latent.parameters():
                p.zero_()

    _tape_ok = True

    def setup_hooks(self, *, tome_info: Optional[Dict[str, Any]] = None, style_reference_states: Optional[Dict[str, Any]] = None) -> None:
        """every block's `setup_hooks` (each keeps its own copy of `tome_info`, as each reference block's hooks object does)"""
        _setup_block_hooks(self, tome_info, style_reference_states)

    def _taped(self, net: Tensor, context: Optional[Tensor]) -> bool:
        """Functions only: Linear-free of hooks, no recomputed blocks, no active dropout, no mask (CrossAttention is called without)"""
        if not (HF.TAPED_NODES[0] and self._tape_ok and net.is_cuda and torch.is_grad_enabled()):
            return False
        if any(block.tome_info is not None for block in self.blocks):
            return False
        for block in self.blocks:
            if block.use_checkpoint or (self.training and (0.0 < block.ff.dropout < 1.0 or 0.0 < block.attn1.out_linear[1].p < 1.0)):
                return False
        return _plain_children(self)

    def forward(self, net: Tensor, context: Optional[Tensor]) -> Tensor:
        if self._taped(net, context):  # norm, projections, every block and the residual add as ONE autograd node
            tensors = (net,) + (() if context is None else (context,)) + tuple(self.parameters())
            try:
                return HF.run_taped(lambda: self._forward(net, context), tensors)
            except HF.TapeBreak as err:
                _tape_broke(self, err)
        return self._forward(net, context)

    def _forward(self, net: Tensor, context: Optional[Tensor]) -> Tensor:
        inp = net
        b, c, h, w = net.shape
        tokens = HF.nchw_to_tokens(self.norm(net))  # [B, HW, C]
        if getattr(self.to_latent, "hook", None) is not None:
            tokens = _hooked_linear(self.to_latent, tokens)
        else:
            wl = self.to_latent.weight
            tokens = HF.linear(tokens, wl.view(wl.shape[0], -1), self.to_latent.bias)
        for block in self.blocks:
            tokens = block(tokens, context=context)
        if getattr(self.from_latent, "hook", None) is not None:
            tokens = _hooked_linear(self.from_latent, tokens)
        else:
            wo = self.from_latent.weight
            tokens = HF.linear(tokens, wo.view(wo.shape[0], -1), self.from_latent.bias)
        return HF.add(inp, HF.tokens_to_nchw(tokens, h, w))


# ---------------------------------------------------------------------------------------------
# UNet (reference modules/multimodal/diffusion/unet.py:25-322)
# ---------------------------------------------------------------------------------------------


class TimestepAttnSequential(nn.Sequential):
    """reference unet.py:31-45: residual blocks get the time embedding, spatial transformers the context"""

    def forward(self, net: Tensor, time_net: Tensor, context: Optional[Tensor] = None) -> Tensor:  # type: ignore
        for layer in self:
            if isinstance(layer, ResidualBlockWithTimeEmbedding):
                net = layer(net, time_net)
            elif isinstance(layer, SpatialTransformer):
                net = layer(net, context)
            else:  # MultiHeadSpatialAttention, resampling, the stem convolution
                net = layer(net)
        return net


def _unet_block_makers(ted: int, *, num_heads: Optional[int], num_head_channels: Optional[int], use_spatial_transformer: bool,
                       num_transformer_layers: int, context_dim: Optional[int], dropout: float, resample_with_conv: bool,
                       resample_with_resblock: bool, use_scale_shift_norm: bool, use_linear_in_transformer: bool, use_checkpoint: bool):
    """(res, attn, down, up): the block constructors `UNetDiffuser` and `ControlNet` share (unet.py:153-213 and :381-431)"""

    def res(in_c: int, out_c: int, **kwargs: Any) -> Module:
        return ResidualBlockWithTimeEmbedding(in_c, out_c, norm_eps=1.0e-5, time_embedding_channels=ted,
                                              dropout=dropout, use_checkpoint=use_checkpoint,
                                              use_scale_shift_norm=use_scale_shift_norm, **kwargs)

    def attn(in_c: int) -> Module:
        if num_head_channels is not None:
            n_heads, head_c = in_c // num_head_channels, num_head_channels
        else:
            if num_heads is None:
                raise ValueError("either `num_heads` or `num_head_channels` should be provided")
            n_heads, head_c = num_heads, in_c // num_heads
        if not use_spatial_transformer:  # unet.py:174-180
            return MultiHeadSpatialAttention(in_c, num_heads=n_heads, num_head_channels=head_c,
                                             use_checkpoint=use_checkpoint)
        return SpatialTransformer(in_c, n_heads, head_c, num_layers=num_transformer_layers,
                                  context_dim=context_dim, use_linear=use_linear_in_transformer,
                                  use_checkpoint=use_checkpoint)

    def down(in_c: int) -> Module:  # unet.py:192-203
        if not resample_with_resblock:
            return TimestepAttnSequential(ResDownsample(in_c, resample_with_conv, out_channels=in_c))
        return TimestepAttnSequential(res(in_c, in_c, integrate_downsample=True))

    def up(in_c: int) -> Module:  # unet.py:205-213
        if not resample_with_resblock:
            return ResUpsample(in_c, resample_with_conv, out_channels=in_c)
        return res(in_c, in_c, integrate_upsample=True)

    return res, attn, down, up


def _unet_input_blocks(in_channels: int, start_channels: int, channel_multipliers: Tuple[int, ...], num_res_blocks: int,
                       attention_downsample_rates: Tuple[int, ...], res: Any, attn: Any, down: Any):
    """(input blocks, their output channels, the channels and the down-sampling rate after the last one): unet.py:215-240 / :433-480"""
    input_blocks: List[Module] = [TimestepAttnSequential(HijackConv2d(in_channels, start_channels, 3, padding=1))]
    skip_channels = [start_channels]
    in_nc, rate = start_channels, 1
    for i, mult in enumerate(channel_multipliers):
        for _ in range(num_res_blocks):
            out_nc = mult * start_channels
            blocks = [res(in_nc, out_nc)]
            in_nc = out_nc
            if rate in attention_downsample_rates:
                blocks.append(attn(in_nc))
            input_blocks.append(TimestepAttnSequential(*blocks))
            skip_channels.append(in_nc)
        if i != len(channel_multipliers) - 1:
            input_blocks.append(down(in_nc))
            rate *= 2
            skip_channels.append(in_nc)
    return input_blocks, skip_channels, in_nc, rate


def _unet_time_net(te: Any, label_embedding: Optional[Module], timesteps: Tensor, labels: Optional[Tensor], start_channels: int) -> Tensor:
    """f32 [B, 4 * start]: the sinusoidal embedding through the time MLP, plus the label embedding (unet.py:295-304 / :512-519)"""
    if timesteps.is_floating_point():  # the sigma-space samplers' fractional timesteps (samplers/k_samplers.py:219-230)
        time_net = ops.timestep_embedding(timesteps.to(torch.float32), start_channels)
    else:
        time_net = ops.timestep_embedding(timesteps.to(torch.int64), start_channels)  # f32 [B, start]
    if getattr(te[0], "hook", None) is not None or getattr(te[2], "hook", None) is not None:
        time_net = _hooked_linear(te[0], time_net, out_f32=True) if te[0].hook is not None else HF.linear(time_net, te[0].weight, te[0].bias, out_f32=True)
        time_net = HF.silu_f32(time_net)
        time_net = _hooked_linear(te[2], time_net, out_f32=True) if te[2].hook is not None else HF.linear(time_net, te[2].weight, te[2].bias, out_f32=True)
    else:
        time_net = HF.linear(time_net, te[0].weight, te[0].bias, out_f32=True)
        time_net = HF.linear(HF.silu_f32(time_net), te[2].weight, te[2].bias, out_f32=True)  # f32 [B, 4 * start]
    if label_embedding is not None:  # unet.py:303-304
        time_net = time_net + HF.embedding(labels.reshape(-1).to(torch.int64), label_embedding.weight)
    return time_net


class _UNetTrunk(Module):
    """what the forward of `UNetDiffuser` and `ControlNet` asks of its own sub-modules before it runs them"""

    def setup_hooks(self, *, tome_info: Optional[Dict[str, Any]] = None, style_reference_states: Optional[Dict[str, Any]] = None) -> None:
        """unet.py:84-90: the hooks of every SpatialTransformer block.  `tome_info` switches token merging on (inference forward
        only), `setup_hooks()` restores the plain path."""
        _setup_block_hooks(self, tome_info, style_reference_states)

    def _write_tome_size(self, net: Tensor) -> None:
        """before_unet_forward (api.py:723-734, unet.py:277-278 / :499-500): the input's spatial size into every enabled block"""
        blocks = getattr(self, "_st_blocks", None)
        if blocks is None:
            blocks = [m for m in self.modules() if isinstance(m, SpatialTransformerBlock)]
            object.__setattr__(self, "_st_blocks", blocks)
        for block in blocks:
            if block.tome_info is not None:
                block.tome_info["size"] = (int(net.shape[-2]), int(net.shape[-1]))

    def _packable_convs(self) -> List[Module]:
        convs = getattr(self, "_pack_convs", None)
        if convs is None:  # 3x3 / stride 1 / pad 1 convolutions whose weight goes to Conv2dFn as it is, on the implicit route (Cin % 32, Cout % 8)
            convs = [m for m in self.modules()
                     if type(m) is HijackConv2d and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
                     and m.groups == 1 and m.padding_mode == "zeros" and m.in_channels % 32 == 0 and m.out_channels % 8 == 0]
            object.__setattr__(self, "_pack_convs", convs)
        return [m for m in convs if getattr(m, "hook", None) is None]

    def _time_projection_blocks(self) -> List[Module]:
        blocks = getattr(self, "_time_blocks", None)
        if blocks is None:
            blocks = [m for m in self.modules()
                      if isinstance(m, ResidualBlockWithTimeEmbedding) and type(getattr(m, "time_embedding", None)) in (HijackLinear, nn.Linear)]
            object.__setattr__(self, "_time_blocks", blocks)  # (a plain list: not a registered sub-module container)
        return [m for m in blocks if not m.use_checkpoint and getattr(m.time_embedding, "hook", None) is None]


@register_module("unet_diffuser")
class UNetDiffuser(_UNetTrunk):
    """reference unet.py:76-322: time embedding MLP (+ class-label embedding), input blocks (ResBlock [+ attention] x
    num_res_blocks, down-sampling), middle block, output blocks over channel-concatenated skip connections (+
    up-sampling), GroupNorm -> SiLU -> conv head.  Attention = `SpatialTransformer` (`use_spatial_transformer=True`, the
    zoo `diffusion/ddpm` configuration; conv or `use_linear_in_transformer` projections) or `MultiHeadSpatialAttention`;
    resampling = conv / pooling / nearest, or ResBlocks with `resample_with_resblock`; `use_scale_shift_norm`, `dropout`
    and ControlNet residuals (`control`, `only_mid_control`) as in the reference.  State keys are the reference's
    (`time_embedding.{0,2}.*`, `label_embedding.weight`, `input_blocks.<i>.<j>.*`, `residual.*`, `output_blocks.*`,
    `head.{0,2}.*`).  `setup_hooks(tome_info=...)` switches token merging on in every SpatialTransformer block (inference; DESIGN
    §3.5e).  3-D signals and the constructor's `hooks_kwargs` are outside the accelerated hot path."""

    def __init__(self, in_channels: int, out_channels: int, *, num_heads: Optional[int] = None,
                 num_head_channels: Optional[int] = None, use_spatial_transformer: bool = False,
                 num_transformer_layers: int = 1, context_dim: Optional[int] = None, signal_dim: int = 2,
                 start_channels: int = 320, num_res_blocks: int = 2,
                 attention_downsample_rates: Tuple[int, ...] = (1, 2, 4), dropout: float = 0.0,
                 channel_multipliers: Tuple[int, ...] = (1, 2, 4, 8), resample_with_conv: bool = True,
                 resample_with_resblock: bool = False, use_scale_shift_norm: bool = False,
                 num_classes: Optional[int] = None, use_linear_in_transformer: bool = False,
                 use_checkpoint: bool = False, hooks_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__()
        if signal_dim != 2 or hooks_kwargs:
            raise NotImplementedError("only the 2-D UNet without SpatialTransformer hooks is on the accelerated hot path")
        self.in_channels, self.out_channels, self.context_dim = in_channels, out_channels, context_dim
        self.num_heads, self.num_head_channels = num_heads, num_head_channels
        self.start_channels, self.num_res_blocks = start_channels, num_res_blocks
        self.attention_downsample_rates = tuple(attention_downsample_rates)
        self.channel_multipliers = tuple(channel_multipliers)
        self.use_scale_shift_norm, self.num_classes = use_scale_shift_norm, num_classes
        ted = start_channels * 4
        self.time_embedding = nn.Sequential(HijackLinear(start_channels, ted), nn.SiLU(), HijackLinear(ted, ted))
        self.label_embedding = None if num_classes is None else nn.Embedding(num_classes, ted)  # unet.py:148-151

        res, attn, down, up = _unet_block_makers(
            ted, num_heads=num_heads, num_head_channels=num_head_channels, use_spatial_transformer=use_spatial_transformer,
            num_transformer_layers=num_transformer_layers, context_dim=context_dim, dropout=dropout,
            resample_with_conv=resample_with_conv, resample_with_resblock=resample_with_resblock,
            use_scale_shift_norm=use_scale_shift_norm, use_linear_in_transformer=use_linear_in_transformer,
            use_checkpoint=use_checkpoint)
        input_blocks, skip_channels, in_nc, rate = _unet_input_blocks(
            in_channels, start_channels, self.channel_multipliers, num_res_blocks, self.attention_downsample_rates, res, attn, down)
        self.input_blocks = nn.ModuleList(input_blocks)
        self.residual = TimestepAttnSequential(res(in_nc, in_nc), attn(in_nc), res(in_nc, in_nc))
        output_blocks: List[Module] = []
        for i, mult in list(enumerate(self.channel_multipliers))[::-1]:
            for idx in range(num_res_blocks + 1):
                idx_nc = skip_channels.pop()
                out_nc = start_channels * mult
                blocks = [res(in_nc + idx_nc, out_nc)]
                in_nc = out_nc
                if rate in self.attention_downsample_rates:
                    blocks.append(attn(in_nc))
                if i != 0 and idx == num_res_blocks:
                    blocks.append(up(in_nc))
                    rate //= 2
                output_blocks.append(TimestepAttnSequential(*blocks))
        self.output_blocks = nn.ModuleList(output_blocks)
        head_conv = HijackConv2d(start_channels, out_channels, 3, padding=1)
        with torch.no_grad():  # zero_module
            for p in head_conv.parameters():
                p.zero_()
        self.head = nn.Sequential(GroupNorm(32, in_nc), nn.SiLU(), head_conv)

    def forward(self, net: Tensor, *, timesteps: Tensor, context: Optional[Tensor] = None,
                labels: Optional[Tensor] = None, control: Any = None, only_mid_control: bool = False) -> Tensor:
        if (labels is None) ^ (self.num_classes is None):
            raise ValueError("`labels` should be given iff `num_classes` is specified")
        self._write_tome_size(net)
        time_net = _unet_time_net(self.time_embedding, self.label_embedding, timesteps, labels, self.start_channels)
        control = None if control is None else list(control)
        nets: List[Tensor] = []
        # Round 5: between the stem and the head every activation travels as the NHWC rows the implicit-GEMM convolutions read and
        # write (channels_last views of logical [B, C, H, W] tensors, `functional.NHWC`): no NCHW <-> NHWC hop around the
        # convolutions, GroupNorm on the rows, token matrices of the transformers as views.  The head (3 output channels)
        # returns NCHW like the reference.
        prev = HF.NHWC[0]
        # (with few samples the NHWC GroupNorm has to cut a sample into row slices and merge them — three launches — and loses to the
        # NCHW path: 256^2 x 1 457 -> 485 ms; with a batch the group form is one launch and the step gains: 64^2 x 8 60.6 -> 59.6 ms)
        HF.NHWC[0] = HF.NHWC_ENABLED and net.is_cuda and net.shape[0] * 32 >= ops.GN_NHWC_GROUP_MIN_WORKGROUPS
        try:
            # every residual block's Linear(SiLU(time_net)) in one launch (functional.time_proj_all); blocks that recompute themselves in
            # backward, use the scale-shift modulation's 2C projection all the same, or carry hooks / low-rank weights fall out of the list
            HF.time_proj_all(time_net, self._time_projection_blocks())
            # ... and both filter matrices of every plain 3x3 convolution (functional.prepack_convs: two launches instead of two per
            # convolution; inside `functional.frozen_conv_packs(self)` the forward matrices packed once on entry, nothing packed here)
            if net.is_cuda:
                HF.pack_convs_of(self)
            for block in self.input_blocks:
                net = block(net, time_net, context)
                nets.append(net)
            net = self.residual(net, time_net, context)
            if control is not None:  # unet.py:311-318
                net = HF.add(net, control.pop())
            for block in self.output_blocks:
                skip = nets.pop()
                if control is not None and not only_mid_control:
                    skip = HF.add(skip, control.pop())
                net = block(HF.concat_channels(net, skip), time_net, context)
            net = self.head[0](net, silu=True)  # GroupNorm + SiLU in one kernel
            return self.head[2](net)
        finally:
            HF.NHWC[0] = prev
            HF.time_pre_clear()
            HF.pack_pre_clear()


def _zero_module(mod: Module) -> Module:
    """modules/common.py:177-180"""
    with torch.no_grad():
        for p in mod.parameters():
            p.zero_()
    return mod


class ControlNet(_UNetTrunk):
    """reference unet.py:325-535: a trainable copy of the UNet's encoder (time MLP, input blocks, middle block) that also takes a
    pixel-space `hint` at 8x the latent's side.  `input_hint_block` (eight 3x3 convolutions with SiLU between them, three of stride 2,
    the last zero-initialised) brings the hint to the stem's shape; it is added after the first input block.  Every input block's
    output and the middle block's go through a zero-initialised 1x1 convolution: the list `UNetDiffuser.forward(control=...)` takes,
    middle last.  State keys are the reference's (`time_embed.{0,2}.*`, `label_embedding.weight`, `input_hint_block.{0,2,...,14}.*`,
    `input_blocks.<i>.<j>.*`, `zero_convs.<i>.0.*`, `middle_block.{0,1,2}.*`, `middle_block_out.0.*`).

    The five narrow hint convolutions (`functional.direct_conv_ok`) run on the direct kernel (csrc/conv_direct.hip) — the hint at 512^2
    is the widest data of the step and their im2row matrices are 9x that —, the other three on Conv2dFn; SiLU on cfhip_silu_bf16."""

    HINT_WIDTHS = ((16, 1), (16, 1), (32, 2), (32, 1), (96, 2), (96, 1), (256, 2))  # (channels, stride) of the hint block's first seven layers

    def __init__(self, in_channels: int, hint_channels: int, *, num_heads: Optional[int] = None,
                 num_head_channels: Optional[int] = None, use_spatial_transformer: bool = False,
                 num_transformer_layers: int = 1, context_dim: Optional[int] = None, signal_dim: int = 2,
                 start_channels: int = 320, num_res_blocks: int = 2,
                 attention_downsample_rates: Tuple[int, ...] = (1, 2, 4), dropout: float = 0.0,
                 channel_multipliers: Tuple[int, ...] = (1, 2, 4, 8), resample_with_conv: bool = True,
                 resample_with_resblock: bool = False, use_scale_shift_norm: bool = False,
                 num_classes: Optional[int] = None, use_linear_in_transformer: bool = False,
                 use_checkpoint: bool = False, hooks_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__()
        if signal_dim != 2 or hooks_kwargs:
            raise NotImplementedError("only the 2-D ControlNet without SpatialTransformer hooks is on the accelerated hot path")
        self.in_channels, self.hint_channels, self.context_dim = in_channels, hint_channels, context_dim
        self.num_heads, self.num_head_channels = num_heads, num_head_channels
        self.start_channels, self.num_res_blocks = start_channels, num_res_blocks
        self.attention_downsample_rates = tuple(attention_downsample_rates)
        self.channel_multipliers = tuple(channel_multipliers)
        self.use_scale_shift_norm, self.num_classes = use_scale_shift_norm, num_classes
        ted = start_channels * 4
        self.time_embed = nn.Sequential(HijackLinear(start_channels, ted), nn.SiLU(), HijackLinear(ted, ted))
        self.label_embedding = None if num_classes is None else nn.Embedding(num_classes, ted)
        res, attn, down, _ = _unet_block_makers(
            ted, num_heads=num_heads, num_head_channels=num_head_channels, use_spatial_transformer=use_spatial_transformer,
            num_transformer_layers=num_transformer_layers, context_dim=context_dim, dropout=dropout,
            resample_with_conv=resample_with_conv, resample_with_resblock=resample_with_resblock,
            use_scale_shift_norm=use_scale_shift_norm, use_linear_in_transformer=use_linear_in_transformer,
            use_checkpoint=use_checkpoint)
        hint_layers: List[Module] = []
        c = hint_channels
        for width, stride in self.HINT_WIDTHS:  # unet.py:441-457
            hint_layers += [HijackConv2d(c, width, 3, stride=stride, padding=1), nn.SiLU()]
            c = width
        hint_layers.append(_zero_module(HijackConv2d(c, start_channels, 3, padding=1)))
        self.input_hint_block = TimestepAttnSequential(*hint_layers)
        input_blocks, skip_channels, in_nc, _ = _unet_input_blocks(
            in_channels, start_channels, self.channel_multipliers, num_res_blocks, self.attention_downsample_rates, res, attn, down)
        self.input_blocks = nn.ModuleList(input_blocks)
        self.zero_convs = nn.ModuleList([self.make_zero_conv(ch) for ch in skip_channels])
        self.middle_block = TimestepAttnSequential(res(in_nc, in_nc), attn(in_nc), res(in_nc, in_nc))
        self.middle_block_out = self.make_zero_conv(in_nc)

    @staticmethod
    def make_zero_conv(channels: int) -> TimestepAttnSequential:
        return TimestepAttnSequential(_zero_module(HijackConv2d(channels, channels, 1, padding=0)))

    @property
    def num_control_scales(self) -> int:
        return len(self.zero_convs) + 1

    def load_encoder_from(self, unet: "UNetDiffuser") -> None:
        """the usual trainable-copy start: the UNet's time MLP, label embedding, input blocks and middle block, key by key"""
        own = self.state_dict()
        pairs = (("time_embedding.", "time_embed."), ("label_embedding.", "label_embedding."), ("input_blocks.", "input_blocks."),
                 ("residual.", "middle_block."))
        with torch.no_grad():
            for key, value in unet.state_dict().items():
                for src, dst in pairs:
                    if not key.startswith(src):
                        continue
                    mine = own.get(dst + key[len(src):])
                    if mine is None or mine.shape != value.shape:
                        raise ValueError(f"load_encoder_from: '{key}' is {tuple(value.shape)} in the UNet, "
                                         f"{None if mine is None else tuple(mine.shape)} as '{dst + key[len(src):]}' here")
                    mine.copy_(value)

    def _guided_hint(self, hint: Tensor) -> Tensor:
        # inside `functional.frozen_conv_packs(self)` (a sampler run: same weights, same hint for every model evaluation) the direct
        # layers' filter operands and the padded NHWC hint are made by the first evaluation and kept in that context's dict
        frozen = HF.frozen_packs_of(self)
        net = hint
        if frozen is not None and HF.DIRECT_HINT_CONV:
            key = ("hint", hint.data_ptr(), tuple(hint.shape), hint._version)
            if key not in frozen:
                frozen[key] = HF.pad_hint_nhwc(hint)
            net = frozen[key]
        for layer in self.input_hint_block:
            if isinstance(layer, nn.SiLU):
                net = HF.silu_bf16(net)
            elif (HF.DIRECT_HINT_CONV and layer.hook is None
                  and HF.direct_conv_ok(layer.in_channels, layer.out_channels, layer.kernel_size[0], layer.stride[0], layer.padding[0], layer.dilation[0])):
                wp = None
                if frozen is not None:
                    if id(layer.weight) not in frozen:
                        frozen[id(layer.weight)] = (ops.conv3x3_direct_pack(layer.weight.detach().contiguous(), 0), None)
                    wp = frozen[id(layer.weight)][0]
                net = HF.direct_conv3x3(net, layer.weight, layer.bias, layer.stride[0], wp)
            else:
                net = layer(net)
        return net

    def forward(self, net: Tensor, hint: Tensor, *, timesteps: Tensor, context: Optional[Tensor] = None,
                labels: Optional[Tensor] = None, scales: Optional[Sequence[float]] = None) -> List[Tensor]:
        """The control list of unet.py:502-535, each entry times its `scales` entry (`DDPM.control_scales`, ddpm.py:413-419; None:
        ones).  hint: [B, hint_channels, 8 H, 8 W]."""
        if (labels is None) ^ (self.num_classes is None):
            raise ValueError("`labels` should be given iff `num_classes` is specified")
        if scales is not None and len(scales) != self.num_control_scales:
            raise ValueError(f"`scales` must hold {self.num_control_scales} floats, got {len(scales)}")
        if hint.dim() != 4 or hint.shape[1] != self.hint_channels or hint.shape[0] != net.shape[0]:
            raise ValueError("`hint` must be [B, hint_channels, 8 H, 8 W]")
        self._write_tome_size(net)
        time_net = _unet_time_net(self.time_embed, self.label_embedding, timesteps, labels, self.start_channels)
        prev = HF.NHWC[0]
        HF.NHWC[0] = HF.NHWC_ENABLED and net.is_cuda and net.shape[0] * 32 >= ops.GN_NHWC_GROUP_MIN_WORKGROUPS
        try:
            HF.time_proj_all(time_net, self._time_projection_blocks())
            if net.is_cuda:
                HF.pack_convs_of(self)
            guided_hint: Optional[Tensor] = self._guided_hint(hint)
            outs: List[Tensor] = []
            for block, zero_conv in zip(self.input_blocks, self.zero_convs):
                net = block(net, time_net, context)
                if guided_hint is not None:  # unet.py:526-528
                    net = HF.add(net, guided_hint)
                    guided_hint = None
                outs.append(zero_conv(net, time_net, context))
            net = self.middle_block(net, time_net, context)
            outs.append(self.middle_block_out(net, time_net, context))
            if scales is not None:
                outs = [o if float(s) == 1.0 else HF.scale_bf16(o, float(s)) for o, s in zip(outs, scales)]
            return outs
        finally:
            HF.NHWC[0] = prev
            HF.time_pre_clear()
            HF.pack_pre_clear()

    def _packable_convs(self) -> List[Module]:
        """(the hint layers that run on the direct kernel read the weight itself: nothing to pack for them)"""
        direct = set()
        if HF.DIRECT_HINT_CONV:
            direct = {id(m) for m in self.input_hint_block if isinstance(m, HijackConv2d)
                      and HF.direct_conv_ok(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0])}
        return [m for m in super()._packable_convs() if id(m) not in direct]


# ---------------------------------------------------------------------------------------------
# KL autoencoder: the first stage of latent diffusion (reference modules/cv/ae/kl.py, ae/common.py, cv/encoder/attn.py,
# cv/decoder/attn.py, core/attentions.py:330-370,572-587, cv/common.py:42-115,338-349)
# ---------------------------------------------------------------------------------------------


def _token_projection(layer: Any, tokens: Tensor) -> Tensor:
    """a 1x1 HijackConv2d over token rows [..., Cin] as the GEMM it is; a hook is honoured as `HijackConv2d.forward` honours it
    (native LoRA through `LoRAConvHook.linear_forward`, otherwise before_forward / after_forward)"""
    if getattr(layer, "hook", None) is not None:
        return _hooked_linear(layer, tokens)
    w = layer.weight
    return HF.linear(tokens, w.view(w.shape[0], -1), layer.bias)


class SpatialAttention(Module):
    """reference attentions.py:330-370: GroupNorm -> 1x1 convolutions to q / k / v -> ONE head over all C channels,
    softmax(q k^T / sqrt(C)) v over the H*W pixels -> 1x1 convolution -> + input.  State keys `group_norm.*` and
    `to_q | to_k | to_v | to_out.{weight [C, C, 1, 1], bias}` as in the reference.  The pixels become token-major rows once and the
    four convolutions are GEMMs over them.  C <= 192 runs on the dispatcher's attention kernels (`HF.attention_core`, with
    backward); 192 < C <= 512 on the wide forward (`HF.attention_wide`, csrc/attn_wide.hip), which is forward-only: an input that
    requires grad raises there, naming the wide head.  C must be a multiple of 8.  The output is bf16 like every activation here,
    except for an f32 input, whose residual sum stays f32."""

    def __init__(self, in_channels: int, *, num_groups: int = 32, eps: float = 1.0e-6):
        super().__init__()
        wide_max = ops._lib.DEFINES["CFHIP_ATTN_WIDE_MAX_HEAD_DIM"]
        if in_channels % 8 != 0 or in_channels > wide_max:
            raise NotImplementedError(f"SpatialAttention: {in_channels} channels are outside the attention kernels (one head of a "
                                      f"multiple of 8 up to {wide_max} channels)")
        self.in_channels = in_channels
        self.group_norm = GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=eps)
        self.to_q = HijackConv2d(in_channels, in_channels, 1, 1, 0)
        self.to_k = HijackConv2d(in_channels, in_channels, 1, 1, 0)
        self.to_v = HijackConv2d(in_channels, in_channels, 1, 1, 0)
        self.to_out = HijackConv2d(in_channels, in_channels, 1, 1, 0)

    def forward(self, net: Tensor) -> Tensor:
        b, c, h, w = net.shape
        tokens = HF.nchw_to_tokens(self.group_norm(net))  # [B, HW, C]
        q, k, v = (_token_projection(layer, tokens) for layer in (self.to_q, self.to_k, self.to_v))
        if c <= 192:
            o = HF.attention_core(q, k, v, 1, None, False, c)
        else:
            o = HF.attention_wide(q, k, v, 1, c)
        out = HF.tokens_to_nchw(_token_projection(self.to_out, o), h, w)
        if net.dtype == torch.float32:
            # an f32 input keeps an f32 residual sum, as it does in the reference under autocast (`inp + net` promotes): one torch
            # add, off the autoencoder's path, where every activation that reaches this module is bf16
            return net + out.float()
        return HF.add(net, out)


def make_attention(in_channels: int, attention_type: str, **kwargs: Any) -> Module:
    """reference attentions.py:572-587 for the types the autoencoder uses: "spatial" and "none"; the others name themselves"""
    if attention_type == "none":
        return nn.Identity(in_channels)
    kwargs["in_channels"] = in_channels
    if attention_type == "spatial":
        return safe_execute(SpatialAttention, kwargs)
    if attention_type in ("cross", "multi_head_spatial", "linear_depth_wise") or attentions.has(attention_type):
        raise NotImplementedError(f"make_attention: attention type '{attention_type}' is not built here ('spatial' and 'none' are)")
    raise ValueError(f"unrecognized attention type '{attention_type}' occurred")


class Downsample(Module):
    """reference cv/encoder/attn.py:14-28: `F.pad(net, (0, 1, 0, 1))` + conv3x3 stride 2 padding 0 as ONE gather with the padding
    on the bottom / right only (`HF.conv2d(..., pad_hi=1)`: no padded copy), or 2x2 average pooling.  State keys `conv.*`."""

    def __init__(self, in_channels: int, with_conv: bool):
        super().__init__()
        self.conv = HijackConv2d(in_channels, in_channels, 3, 2, 0) if with_conv else None

    def forward(self, net: Tensor) -> Tensor:
        if self.conv is None:
            return HF.avg_pool2(net)
        conv = self.conv
        if conv.hook is not None:
            raise NotImplementedError("Downsample: a hook on the asymmetrically padded convolution is outside the accelerated hot path")
        return HF.conv2d(net, conv.weight, conv.bias, 2, 0, 1, pad_hi=1)


class Upsample(Module):
    """reference cv/decoder/attn.py:18-30: nearest x2, then an optional conv3x3.  State keys `conv.*`."""

    def __init__(self, in_channels: int, with_conv: bool):
        super().__init__()
        self.conv = HijackConv2d(in_channels, in_channels, 3, 1, 1) if with_conv else None

    def forward(self, net: Tensor) -> Tensor:
        net = HF.upsample2(net)
        return net if self.conv is None else self.conv(net)


def _run_blocks(blocks: nn.Sequential, net: Tensor) -> Tensor:
    """an nn.Sequential of the autoencoder with every `GroupNorm, nn.SiLU` pair as the one fused kernel (the containers keep the
    reference's layout, so that the numeric state keys match)"""
    mods = list(blocks)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, GroupNorm) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.SiLU):
            net = m(net, silu=True)
            i += 2
        else:
            net = m(net)
            i += 1
    return net


def _res_block(in_channels: int, out_channels: int, dropout: float) -> Module:
    return ResidualBlockWithTimeEmbedding(in_channels, out_channels, dropout=dropout, time_embedding_channels=0)


@encoders.register("attention")
class AttentionEncoder(Module):
    """reference cv/encoder/attn.py:31-97, same constructor keywords; `encoder` is the reference's nn.Sequential (state keys
    `encoder.<n>.*`)."""

    def __init__(self, img_size: int, in_channels: int, inner_channels: int, latent_channels: int, channel_multipliers: Tuple[int, ...], *,
                 num_res_blocks: int, attention_resolutions: Tuple[int, ...] = (), dropout: float = 0.0, downsample_with_conv: bool = True,
                 attention_type: str = "spatial"):
        super().__init__()
        self.img_size, self.in_channels, self.inner_channels, self.latent_channels = img_size, in_channels, inner_channels, latent_channels
        self.num_downsample = len(channel_multipliers)
        self.num_res_blocks = num_res_blocks
        blocks: List[Module] = [HijackConv2d(in_channels, inner_channels, 3, 1, 1)]
        current_resolution = img_size
        self.in_channel_multipliers = in_channel_multipliers = (1,) + tuple(channel_multipliers)
        in_nc = 0
        for i in range(self.num_downsample):
            in_nc = inner_channels * in_channel_multipliers[i]
            out_nc = inner_channels * channel_multipliers[i]
            for _ in range(num_res_blocks):
                blocks.append(_res_block(in_nc, out_nc, dropout))
                in_nc = out_nc
                if current_resolution in attention_resolutions:
                    blocks.append(make_attention(in_nc, attention_type))
            if i != self.num_downsample - 1:
                blocks.append(Downsample(in_nc, downsample_with_conv))
                current_resolution //= 2
        blocks += [_res_block(in_nc, in_nc, dropout), make_attention(in_nc, attention_type), _res_block(in_nc, in_nc, dropout)]
        blocks += [GroupNorm(num_groups=32, num_channels=in_nc, eps=1.0e-6), nn.SiLU(), HijackConv2d(in_nc, latent_channels, 3, 1, 1)]
        self.encoder = nn.Sequential(*blocks)

    def forward(self, net: Tensor) -> Tensor:
        return _run_blocks(self.encoder, net)

    def encode(self, net: Tensor) -> Tensor:
        return self(net)


class DecoderInputs:
    """reference cv/common.py:53-75, the fields this path uses: `z`, `no_head`, `apply_tanh`, `labels`, `kwargs`"""

    def __init__(self, z: Tensor, labels: Optional[Tensor] = None, apply_tanh: Optional[bool] = None, no_head: bool = False,
                 kwargs: Optional[Dict[str, Any]] = None):
        self.z, self.labels, self.apply_tanh, self.no_head, self.kwargs = z, labels, apply_tanh, no_head, kwargs


@decoders.register("attention")
class AttentionDecoder(Module):
    """reference cv/decoder/attn.py:33-100 + IDecoder.decode (cv/common.py:110-115), same constructor keywords; `decoder` and `head`
    are the reference's nn.Sequential containers.  `inputs.no_head` returns the features in front of the head.  `apply_tanh`
    (the constructor's, or `inputs.apply_tanh`) RAISES NotImplementedError: there is no tanh kernel here, and the zoo autoencoders
    are built without it."""

    def __init__(self, img_size: int, out_channels: int, inner_channels: int, latent_channels: int, channel_multipliers: Tuple[int, ...], *,
                 num_res_blocks: int, attention_resolutions: Tuple[int, ...] = (), dropout: float = 0.0, upsample_with_conv: bool = True,
                 attention_type: str = "spatial", apply_tanh: bool = False):
        super().__init__()
        self.img_size, self.out_channels, self.inner_channels, self.latent_channels = img_size, out_channels, inner_channels, latent_channels
        self.num_upsample = len(channel_multipliers)
        self.num_res_blocks = num_res_blocks
        self.apply_tanh = apply_tanh
        in_nc = inner_channels * channel_multipliers[-1]
        blocks: List[Module] = [HijackConv2d(latent_channels, in_nc, 3, 1, 1)]
        blocks += [_res_block(in_nc, in_nc, dropout), make_attention(in_nc, attention_type), _res_block(in_nc, in_nc, dropout)]
        current_resolution = img_size // 2 ** (self.num_upsample - 1)
        for i in reversed(range(self.num_upsample)):
            out_nc = inner_channels * channel_multipliers[i]
            for _ in range(num_res_blocks + 1):
                blocks.append(_res_block(in_nc, out_nc, dropout))
                in_nc = out_nc
                if current_resolution in attention_resolutions:
                    blocks.append(make_attention(in_nc, attention_type))
            if i != 0:
                blocks.append(Upsample(in_nc, upsample_with_conv))
                current_resolution *= 2
        self.decoder = nn.Sequential(*blocks)
        self.head = nn.Sequential(GroupNorm(num_groups=32, num_channels=in_nc, eps=1.0e-6), nn.SiLU(), HijackConv2d(in_nc, out_channels, 3, 1, 1))

    def forward(self, inputs: DecoderInputs) -> Tensor:
        net = _run_blocks(self.decoder, inputs.z)
        return net if inputs.no_head else _run_blocks(self.head, net)

    def decode(self, inputs: DecoderInputs) -> Tensor:
        apply_tanh = inputs.apply_tanh
        if apply_tanh or (apply_tanh is None and self.apply_tanh):
            raise NotImplementedError("AttentionDecoder: `apply_tanh` has no kernel on the accelerated hot path")
        return self(inputs)


class EncoderDecoder(Module):
    """reference cv/common.py:338-349: `encoder` / `decoder` built by name from the `encoders` / `decoders` registries"""

    def __init__(self, *, encoder: str = "vanilla", decoder: str = "vanilla", encoder_config: Optional[Dict[str, Any]] = None,
                 decoder_config: Optional[Dict[str, Any]] = None):
        super().__init__()
        self.encoder = encoders.build(encoder, config=encoder_config)
        self.decoder = decoders.build(decoder, config=decoder_config)


class GaussianDistribution:
    """reference cv/ae/kl.py:18-66 over the moments [B, 2E, h, w] the `to_embedding` convolution leaves (bf16, NCHW or channels-last,
    read in place).  `sample` and `kl()` are ONE launch of `cfhip_gaussian_posterior` each; `mean`, `log_var`, `std`, `var` are
    plain f32 torch views / expressions of the moments for inspection, and so are `nll` and the `other is not None` form of `kl`:
    they are off the training path.

    sample(seed=, offset=, noise=, scale_factor=): `noise` (f32, the latent's shape) reproduces a given draw; `seed` (and
    `offset`) name the Philox stream `ops.randn` regenerates; with neither, the pair comes from the process-wide stream
    (`ops.PhiloxState`).  `scale_factor` is LDM.preprocess's (ldm.py:183-190), folded into the same kernel."""

    key = "distribution"

    def __init__(self, net: Tensor, deterministic: bool = False):
        self.net = net if net.dtype == torch.bfloat16 else ops.to_bf16(net.float().contiguous())
        self.device = net.device
        self.deterministic = deterministic

    @property
    def mean(self) -> Tensor:
        return torch.chunk(self.net.float(), 2, dim=1)[0]

    @property
    def log_var(self) -> Tensor:
        return torch.clamp(torch.chunk(self.net.float(), 2, dim=1)[1], -30.0, 20.0)

    @property
    def std(self) -> Tensor:
        return torch.zeros_like(self.mean) if self.deterministic else torch.exp(0.5 * self.log_var)

    @property
    def var(self) -> Tensor:
        return torch.zeros_like(self.mean) if self.deterministic else torch.exp(self.log_var)

    def sample(self, *, seed: Optional[int] = None, offset: int = 0, noise: Optional[Tensor] = None, scale_factor: float = 1.0,
               out: Optional[Tensor] = None) -> Tensor:
        if self.deterministic:
            return self.mode(scale_factor=scale_factor, out=out)
        if noise is None and seed is None:
            seed, offset = ops.PhiloxState.take((self.net.numel() // 2 + 3) // 4)
        return ops.gaussian_posterior(self.net, scale_factor=scale_factor, seed=seed or 0, offset=offset, noise=noise, out=out)[0]

    def mode(self, *, scale_factor: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
        return ops.gaussian_posterior(self.net, scale_factor=scale_factor, deterministic=True, out=out)[0]

    def kl(self, other: Optional["GaussianDistribution"] = None) -> Tensor:
        if self.deterministic:
            return torch.tensor([0.0], device=self.device)
        if other is None:
            return ops.gaussian_posterior(self.net, want_z=False, want_kl=True)[1]
        spread = ((self.mean - other.mean).square() + self.var) / other.var
        return 0.5 * (spread - 1.0 - self.log_var + other.log_var).sum(dim=(1, 2, 3))

    def nll(self, sample: Tensor, dims: Tuple[int, ...] = (1, 2, 3)) -> Tensor:
        if self.deterministic:
            return torch.tensor([0.0], device=self.device)
        return 0.5 * (math.log(2.0 * math.pi) + self.log_var + (sample - self.mean).square() / self.var).sum(dim=dims)


class _AttentionAutoEncoder(Module):
    """reference IAttentionAutoEncoder (cv/ae/common.py:12-75): the constructor both autoencoders share — `generator` (attention
    encoder / decoder), `to_embedding`, `from_embedding` — and `generate_z`.  `enc_double_channels`: the encoder and `to_embedding`
    put out twice the channels (the KL moments)."""

    enc_double_channels: bool

    def __init__(self, img_size: int, in_channels: int, out_channels: int, inner_channels: int, latent_channels: int,
                 channel_multipliers: Tuple[int, ...], *, embedding_channels: int, num_res_blocks: int,
                 attention_resolutions: Tuple[int, ...] = (), dropout: float = 0.0, resample_with_conv: bool = True,
                 attention_type: str = "spatial", apply_tanh: bool = False):
        super().__init__()
        self.z_size = img_size // 2 ** (len(channel_multipliers) - 1)
        self.img_size, self.in_channels, self.out_channels = img_size, in_channels, out_channels
        self.inner_channels, self.latent_channels = inner_channels, latent_channels
        self.channel_multipliers = channel_multipliers
        self.embedding_channels = embedding_channels
        module_config = dict(img_size=img_size, in_channels=in_channels, out_channels=out_channels, inner_channels=inner_channels,
                             latent_channels=latent_channels, channel_multipliers=channel_multipliers, num_res_blocks=num_res_blocks,
                             attention_resolutions=attention_resolutions, dropout=dropout, downsample_with_conv=resample_with_conv,
                             upsample_with_conv=resample_with_conv, attention_type=attention_type)
        enc_config, dec_config = shallow_copy_dict(module_config), shallow_copy_dict(module_config)
        enc_scaler = 1 + int(self.enc_double_channels)
        enc_config["latent_channels"] = enc_scaler * latent_channels
        dec_config["apply_tanh"] = apply_tanh
        self.generator = EncoderDecoder(encoder="attention", decoder="attention", encoder_config=enc_config, decoder_config=dec_config)
        self.to_embedding = HijackConv2d(enc_scaler * latent_channels, enc_scaler * embedding_channels, 1)
        self.from_embedding = HijackConv2d(embedding_channels, latent_channels, 1)

    def generate_z(self, num_samples: int) -> Tensor:
        shape = [num_samples, self.embedding_channels, self.z_size, self.z_size]
        return torch.randn(shape, device=next(self.parameters()).device)

    def decode(self, inputs: DecoderInputs) -> Tensor:
        inputs.z = self.from_embedding(inputs.z)
        return self.generator.decoder.decode(inputs)


@generators.register("ae_kl")
class AttentionAutoEncoderKL(_AttentionAutoEncoder):
    """reference cv/ae/kl.py:69-121 on IAttentionAutoEncoder (cv/ae/common.py:12-75), same constructor keywords and state keys
    (`generator.encoder.encoder.<n>.*`, `generator.decoder.decoder.<n>.*`, `generator.decoder.head.<n>.*`, `to_embedding.*`,
    `from_embedding.*`): a reference checkpoint loads with `load_state_dict(strict=True)`.  `encode` returns the
    GaussianDistribution of the moments; `decode` takes DecoderInputs (z f32 or bf16 [B, E, h, w]).  The vector-quantised sibling
    (`ae_vq`, cv/ae/vq.py) is `AttentionAutoEncoderVQ` below; it is not registered."""

    enc_double_channels = True

    def encode(self, net: Tensor) -> GaussianDistribution:
        return GaussianDistribution(self.to_embedding(self.generator.encoder.encode(net)))

    def get_results(self, net: Tensor, *, sample_posterior: bool = True, no_head: bool = False,
                    apply_tanh: Optional[bool] = None) -> Tuple[Tensor, GaussianDistribution]:
        distribution = self.encode(net)
        z = distribution.sample() if sample_posterior else distribution.mode()
        return self.decode(DecoderInputs(z=z, no_head=no_head, apply_tanh=apply_tanh)), distribution

    def reconstruct(self, net: Tensor, *, labels: Optional[Tensor] = None, kwargs: Optional[Dict[str, Any]] = None) -> Optional[Tensor]:
        return self.get_results(net, **dict(kwargs or {}, sample_posterior=False))[0]

    def forward(self, net: Tensor, *, sample_posterior: bool = True, no_head: bool = False,
                apply_tanh: Optional[bool] = None) -> Dict[str, Any]:
        net, distribution = self.get_results(net, sample_posterior=sample_posterior, no_head=no_head, apply_tanh=apply_tanh)
        return {PREDICTIONS_KEY: net, GaussianDistribution.key: distribution}


class VQCodebookOut(NamedTuple):
    """reference cv/common.py:352-359"""

    z_e: Tensor
    z_q: Tensor
    indices: Tensor
    z_q_g: Optional[Tensor] = None

    def to_dict(self) -> Dict[str, Any]:
        return self._asdict()


class VQCodebook(Module):
    """reference cv/common.py:362-400, forward only: `embedding.weight` f32 [num_codes, code_dimension], initialised
    uniform(-1 / N, 1 / N).  `forward(z_e)` is ONE launch of `cfhip_vq_nearest` on the `to_embedding` output as it lies (bf16 or f32,
    NCHW or channels-last): indices int64 [B, h, w] and z_q f32 [B, D, h, w] = scale_factor * embedding.weight[indices] (the
    reference's value: its straight-through expression z_e + (z_q - z_e).detach() only matters to a backward).  The squared norms
    of the codes are cached, keyed on the weight's `_version` and data pointer: the codebook is frozen under LDM.  `z_q_g`, only
    when asked, is `embedding.weight[indices].view_as(z_e)` as in the reference — pixel-major rows reshaped, NOT permuted, into
    the NCHW shape; that is what the reference computes and it is kept on purpose — in plain torch indexing, off the hot path.
    Training the codebook is not built: an input that requires grad while grad mode is on raises."""

    def __init__(self, num_codes: int, code_dimension: int):
        super().__init__()
        self.num_codes, self.code_dimension = num_codes, code_dimension
        self.embedding = nn.Embedding(num_codes, code_dimension)
        span = 1.0 / num_codes
        self.embedding.weight.data.uniform_(-span, span)
        self._sq_key: Optional[Tuple[int, int]] = None
        self._sq: Optional[Tensor] = None

    def code_sqnorm(self) -> Tensor:
        w = self.embedding.weight
        key = (w._version, w.data_ptr())
        if self._sq is None or self._sq_key != key:
            self._sq, self._sq_key = ops.vq_code_sqnorm(w.detach()), key
        return self._sq

    def forward(self, z_e: Tensor, *, return_z_q_g: bool = False, scale_factor: float = 1.0) -> VQCodebookOut:
        if z_e.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("VQCodebook is forward-only: the straight-through gradient and the codebook / commitment "
                                      "losses of autoencoder training are not built (DESIGN §8); run it under torch.no_grad()")
        weight = self.embedding.weight
        indices, z_q = ops.vq_nearest(z_e, weight.detach(), code_sq=self.code_sqnorm(), scale_factor=scale_factor)
        if not return_z_q_g:
            return VQCodebookOut(z_e, z_q, indices)
        return VQCodebookOut(z_e, z_q, indices, weight[indices].view(z_e.shape))


class AttentionAutoEncoderVQ(_AttentionAutoEncoder):
    """reference cv/ae/vq.py:16-114 on IAttentionAutoEncoder, same constructor keywords and state keys (the KL class's, with
    single-width `to_embedding`, plus `codebook.embedding.weight`): a reference checkpoint loads with `load_state_dict(strict=True)`.
    Forward-only (see VQCodebook).  `encode(..., scale_factor=)` folds LDM.preprocess's scale (ldm.py:183-190) into the lookup
    launch.  Not registered as "ae_vq" in `generators` yet: construct it directly."""

    enc_double_channels = False

    def __init__(self, img_size: int, in_channels: int, out_channels: int, inner_channels: int, latent_channels: int,
                 channel_multipliers: Tuple[int, ...], *, num_codes: int, embedding_channels: int, num_res_blocks: int,
                 attention_resolutions: Tuple[int, ...] = (), dropout: float = 0.0, resample_with_conv: bool = True,
                 attention_type: str = "spatial", apply_tanh: bool = False):
        super().__init__(img_size, in_channels, out_channels, inner_channels, latent_channels, channel_multipliers,
                         embedding_channels=embedding_channels, num_res_blocks=num_res_blocks, attention_resolutions=attention_resolutions,
                         dropout=dropout, resample_with_conv=resample_with_conv, attention_type=attention_type, apply_tanh=apply_tanh)
        self.codebook = VQCodebook(num_codes, embedding_channels)

    def generate_z(self, num_samples: int) -> Tensor:
        return self.codebook(super().generate_z(num_samples), return_z_q_g=False).z_q

    def encode(self, net: Tensor, *, return_z_q_g: bool = True, scale_factor: float = 1.0) -> VQCodebookOut:
        net = self.to_embedding(self.generator.encoder.encode(net))
        return self.codebook(net, return_z_q_g=return_z_q_g, scale_factor=scale_factor)

    def get_results(self, net: Tensor, *, no_head: bool = False, apply_tanh: Optional[bool] = None,
                    return_z_q_g: bool = True) -> Tuple[Tensor, VQCodebookOut]:
        out = self.encode(net, return_z_q_g=return_z_q_g)
        return self.decode(DecoderInputs(z=out.z_q, no_head=no_head, apply_tanh=apply_tanh)), out

    def reconstruct(self, net: Tensor, *, labels: Optional[Tensor] = None, kwargs: Optional[Dict[str, Any]] = None) -> Optional[Tensor]:
        return self.get_results(net, **dict(kwargs or {}, return_z_q_g=False))[0]

    def forward(self, net: Tensor, *, no_head: bool = False, apply_tanh: Optional[bool] = None, return_z_q_g: bool = True) -> Dict[str, Any]:
        net, out = self.get_results(net, no_head=no_head, apply_tanh=apply_tanh, return_z_q_g=return_z_q_g)
        results = {PREDICTIONS_KEY: net}
        results.update(out.to_dict())
        return results


# ---------------------------------------------------------------------------------------------
# The RRDB (ESRGAN) upscaler (reference modules/cv/translator/rrdb.py), forward only, on the dense-block convolution
# ---------------------------------------------------------------------------------------------


class ResidualDenseBlock(Module):
    """reference rrdb.py:12-29: the parameters only (conv1 .. conv5, the reference's keys and shapes); RRDBNet.forward runs them"""

    def __init__(self, in_channels: int, grow_channels: int):
        super().__init__()
        for i in range(4):
            setattr(self, f"conv{i + 1}", nn.Conv2d(in_channels + i * grow_channels, grow_channels, 3, 1, 1))
        self.conv5 = nn.Conv2d(in_channels + 4 * grow_channels, in_channels, 3, 1, 1)

    def forward(self, net: Tensor) -> Tensor:
        raise NotImplementedError("a ResidualDenseBlock holds parameters only: RRDBNet.forward runs the whole net on dense buffers")


class RRDB(Module):
    """reference rrdb.py:32-44: three dense blocks (parameters only, see ResidualDenseBlock)"""

    def __init__(self, in_channels: int, grow_channels: int):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(in_channels, grow_channels)
        self.rdb2 = ResidualDenseBlock(in_channels, grow_channels)
        self.rdb3 = ResidualDenseBlock(in_channels, grow_channels)

    def forward(self, net: Tensor) -> Tensor:
        raise NotImplementedError("an RRDB holds parameters only: RRDBNet.forward runs the whole net on dense buffers")


@register_module("rrdb")
class RRDBNet(Module):
    """reference rrdb.py:58-102 (the zoo's sr/esr and sr/esr.anime), same constructor and state-dict keys, f32 parameters: a reference
    checkpoint loads with `load_state_dict`.  Forward only.  `forward(net)` takes f32 or bf16 [B, C, H, W] on the device and returns f32
    [B, out_channels, H scale, W scale] after one input launch (`ops.pixel_unshuffle_nhwc`) and 15 num_layers + 6 launches of
    `ops.conv3x3_dense`: a dense block keeps [inp, net1 .. net4] in one bf16 buffer [B H W][latent + 4 grow] whose slices the convolutions
    read and write (no torch.cat), LeakyReLU, `* 0.2 + inp` of the block and of the RRDB, `net + body` and both nearest upsamplings are
    inside those launches, and the last one stores f32 NCHW.  Four dense buffers: one keeps conv_first's output for `net + body`, three
    rotate (an RRDB's input has to outlive its three blocks).  Packed filters are cached per parameter version.
    Only latent_channels = 64 with grow_channels = 32 is covered by the kernel; training is not built."""

    def __init__(self, in_channels: int = 3, out_channels: Optional[int] = None, *, scale: int = 4, latent_channels: int = 64,
                 grow_channels: int = 32, num_layers: int = 23):
        super().__init__()
        if scale not in (1, 2, 4):
            raise ValueError(f"RRDBNet: scale = {scale} (1, 2 or 4)")
        if latent_channels != 64 or grow_channels != 32:
            raise NotImplementedError(f"RRDBNet: latent_channels = {latent_channels}, grow_channels = {grow_channels}: the dense-block "
                                      "convolution covers latent_channels = 64 with grow_channels = 32 (DESIGN §8)")
        if num_layers < 1:
            raise ValueError(f"RRDBNet: num_layers = {num_layers} (>= 1)")
        self.scale = scale
        self.in_channels = in_channels
        self.out_channels = out_channels = out_channels or in_channels
        self.latent_channels, self.grow_channels, self.num_layers = latent_channels, grow_channels, num_layers
        self.unshuffle = 4 // scale  # rrdb.py:73-76, :91-94
        if in_channels * self.unshuffle ** 2 > 192 or out_channels > 64:
            raise NotImplementedError(f"RRDBNet: in_channels = {in_channels} at scale {scale} / out_channels = {out_channels}: the "
                                      "dense-block convolution covers 192 input and 64 output channels (DESIGN §8)")
        self.conv_first = nn.Conv2d(in_channels * self.unshuffle ** 2, latent_channels, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(latent_channels, grow_channels) for _ in range(num_layers)])
        self.conv_body = nn.Conv2d(latent_channels, latent_channels, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(latent_channels, latent_channels, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(latent_channels, latent_channels, 3, 1, 1)
        self.conv_hr = nn.Conv2d(latent_channels, latent_channels, 3, 1, 1)
        self.conv_last = nn.Conv2d(latent_channels, out_channels, 3, 1, 1)
        self._packs: Dict[int, Tuple[Tuple[int, int], Tensor]] = {}

    def _packed(self, conv: nn.Conv2d) -> Tuple[Tensor, Tensor]:
        """(packed bf16 filters, f32 bias) of one convolution, repacked when the weight's version or storage changes"""
        w = conv.weight
        key = (w._version, w.data_ptr())
        hit = self._packs.get(id(conv))
        if hit is None or hit[0] != key:
            hit = self._packs[id(conv)] = (key, ops.conv3x3_dense_pack(w.detach().contiguous()))
        return hit[1], conv.bias.detach()

    def _check(self, net: Tensor) -> Tuple[int, int, int]:
        if torch.is_grad_enabled() and (net.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("RRDBNet is forward only: the backward through the dense blocks is not built (DESIGN §8); call "
                                      "`upscale(x)` or run it under torch.no_grad()")
        if net.dim() != 4 or net.shape[1] != self.in_channels:
            raise ValueError(f"RRDBNet: [B, {self.in_channels}, H, W] expected, got {tuple(net.shape)}")
        s = self.unshuffle
        if net.shape[2] % s or net.shape[3] % s:
            raise ValueError(f"RRDBNet: H = {net.shape[2]}, W = {net.shape[3]} must be divisible by {s} at scale {self.scale}")
        if not net.is_cuda:
            raise RuntimeError(f"RRDBNet: the input must live on the HIP device (got {net.device}); there is no CPU path")
        if net.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"RRDBNet: float32 or bfloat16 input expected, got {net.dtype}")
        return net.shape[0], net.shape[2] // s, net.shape[3] // s

    def forward(self, net: Tensor) -> Tensor:
        b, h, w = self._check(net)
        lat, grow, wide = self.latent_channels, self.grow_channels, self.latent_channels + 4 * self.grow_channels
        rows = b * h * w
        bf16 = torch.bfloat16
        x0 = ops.pixel_unshuffle_nhwc(net.detach().contiguous(), self.unshuffle)
        dense = [torch.empty((rows, wide), dtype=bf16, device=net.device) for _ in range(4)]

        def conv(layer: nn.Conv2d, x: Tensor, y: Tensor, hh: int = h, ww: int = w, **kw: Any) -> None:
            wp, bias = self._packed(layer)
            ops.conv3x3_dense(x, wp, bias, y, b, hh, ww, **kw)

        def rdb(block: ResidualDenseBlock, src: Tensor, dst: Tensor, outer: Optional[Tensor]) -> None:
            """src[:, :lat] holds the block's input, src[:, lat:] receives net1 .. net4; the block's output goes to dst[:, :lat]"""
            for i in range(4):
                cin = lat + i * grow
                conv(getattr(block, f"conv{i + 1}"), src[:, :cin], src[:, cin:cin + grow], epilogue="lrelu", slope=0.2)
            if outer is None:
                conv(block.conv5, src, dst[:, :lat], epilogue="res1", s1=0.2, r1=src[:, :lat])
            else:  # the third block of an RRDB: its own `* 0.2 + inp`, then the RRDB's (rrdb.py:44)
                conv(block.conv5, src, dst[:, :lat], epilogue="res2", s1=0.2, r1=src[:, :lat], s2=0.2, r2=outer[:, :lat])

        conv(self.conv_first, x0.view(rows, -1), dense[0][:, :lat])
        cur = 0  # dense[0] keeps conv_first's output until `net + body`; 1 .. 3 rotate
        for block in self.body:
            p, q = [i for i in (1, 2, 3) if i != cur][:2]
            rdb(block.rdb1, dense[cur], dense[p], None)
            rdb(block.rdb2, dense[p], dense[q], None)
            rdb(block.rdb3, dense[q], dense[p], dense[cur])
            cur = p
        free = [i for i in (1, 2, 3) if i != cur][0]
        trunk = dense[free][:, :lat]
        conv(self.conv_body, dense[cur][:, :lat], trunk, epilogue="res1", s1=1.0, r1=dense[0][:, :lat])  # net + body (rrdb.py:96-97)
        side2 = torch.empty((4 * rows, lat), dtype=bf16, device=net.device)
        conv(self.conv_up1, trunk, side2, epilogue="lrelu", slope=0.2, up2=True)
        side4 = torch.empty((16 * rows, lat), dtype=bf16, device=net.device)
        conv(self.conv_up2, side2, side4, 2 * h, 2 * w, epilogue="lrelu", slope=0.2, up2=True)
        hr = torch.empty((16 * rows, lat), dtype=bf16, device=net.device)
        conv(self.conv_hr, side4, hr, 4 * h, 4 * w, epilogue="lrelu", slope=0.2)
        out = torch.empty((b, self.out_channels, 4 * h, 4 * w), dtype=torch.float32, device=net.device)
        conv(self.conv_last, hr, out, 4 * h, 4 * w)
        return out

    def upscale(self, net: Tensor) -> Tensor:
        """`forward` in eval mode under torch.no_grad()"""
        training = self.training
        self.eval()
        try:
            with torch.no_grad():
                return self(net)
        finally:
            self.train(training)


# ---------------------------------------------------------------------------------------------
# A16: tabular encoder (reference modules/core/ml_encoder.py:131-258, models/ml/common.py:27-93)
# ---------------------------------------------------------------------------------------------


class _EmbeddingTable(Module):
    """reference ml_encoder.Embedding (:45-70): parameter `weights` [in_dim, out_dim]; the lookup itself happens in
    the encoder's gather kernel, the dropout (default 0.1, :113-117) on the embedding block of its output."""

    def __init__(self, in_dim: int, out_dim: int, init_std: float = 0.02, dropout: float = 0.1):
        super().__init__()
        weights = torch.empty(in_dim, out_dim)
        nn.init.trunc_normal_(weights, mean=0.0, std=init_std, a=-2.0 * init_std, b=2.0 * init_std)
        self.weights = nn.Parameter(weights)
        self.dropout = Dropout(dropout) if 0.0 < dropout < 1.0 else None
        self.in_dim, self.out_dim = in_dim, out_dim

    def extra_repr(self) -> str:
        return f"{self.in_dim} -> {self.out_dim}"


def _embedding_out_dim(in_dim: int, out_dim: Any) -> int:
    """ml_encoder.get_embedding_config (:90-111)"""
    import math

    if isinstance(out_dim, int):
        return out_dim
    if out_dim == "log":
        return math.ceil(math.log2(in_dim))
    if out_dim == "sqrt":
        return math.ceil(math.sqrt(in_dim))
    if out_dim == "auto":
        return max(4, min(8, math.ceil(math.log2(in_dim))))
    raise ValueError(f"embedding dim '{out_dim}' is not defined")


@register_module("ml.encoder")
class MLEncoder(Module):
    """`Encoder` of the reference (ml_encoder.py:131-258) with `CommonMLModel.encode`'s concatenation (models/ml/
    common.py:67-87) folded in: `forward(x)` returns `merged_all` = [numerical | one-hot | embedding] from ONE gather
    kernel (`cfhip_ml_encode_fwd`); `encode_result(x)` returns the reference's (indices, one_hot, embedding) triple.
    `settings`: {"<column>": dict(dim=..., methods="embedding" | "one_hot" | [both], method_configs={...})} — the
    fields of the reference's `MLEncoderSettings` (schema.py:1956-1990), as dicts or objects with those attributes.
    State-dict keys as in the reference: `embeddings.<column>.weights`, buffer `dims`."""

    def __init__(self, settings: Dict[str, Any], global_encoder_settings: Any = None):
        super().__init__()
        get = lambda obj, key, default=None: (obj.get(key, default) if isinstance(obj, dict) else getattr(obj, key, default))  # noqa: E731
        ges_dim = get(global_encoder_settings, "embedding_dim") if global_encoder_settings is not None else None
        ges_drop = get(global_encoder_settings, "embedding_dropout") if global_encoder_settings is not None else None
        self.embeddings = nn.ModuleDict()
        self.tgt_columns: List[int] = []
        self.one_hot_columns: List[int] = []
        self.embedding_columns: List[int] = []
        dims: List[int] = []
        self.one_hot_dim = self.embedding_dim = self.dim_increment = 0
        for str_idx in sorted(settings):
            st = settings[str_idx]
            idx, dim = int(str_idx), int(get(st, "dim"))
            methods = get(st, "methods", "embedding")
            methods = [methods] if isinstance(methods, str) else list(methods)
            dims.append(dim)
            self.tgt_columns.append(idx)
            if "one_hot" in methods:
                self.one_hot_columns.append(idx)
                self.one_hot_dim += dim
                self.dim_increment += dim - 1
            if "embedding" in methods:
                kw = dict(get(st, "method_configs") or {})
                out_dim = _embedding_out_dim(dim, kw.get("out_dim", "auto" if ges_dim is None else ges_dim))
                init = kw.get("init_config", {"mean": 0.0, "std": 0.02})
                if kw.get("init_method", "truncated_normal") != "truncated_normal":
                    raise NotImplementedError("embedding init methods other than truncated_normal are not provided")
                drop = kw.get("dropout", 0.1 if ges_drop is None else ges_drop)
                self.embedding_columns.append(idx)
                self.embeddings[str_idx] = _EmbeddingTable(dim, out_dim, float(init.get("std", 0.02)), float(drop))
                self.embedding_dim += out_dim
                self.dim_increment += out_dim - 1
        self.categorical_dim = self.one_hot_dim + self.embedding_dim
        self.use_one_hot, self.use_embedding = bool(self.one_hot_columns), bool(self.embedding_columns)
        self.is_empty = not self.use_one_hot and not self.use_embedding
        self.register_buffer("dims", torch.tensor(dims, dtype=torch.float32))
        self._dims_int = dims
        self._plans: Dict[int, Any] = {}

    def _plan(self, num_features: int, device: torch.device) -> Any:
        """Output-column plan for inputs with `num_features` columns (built once per width and device)."""
        key = (num_features, str(device))
        if key in self._plans:
            return self._plans[key]
        bad = [c for c in self.tgt_columns if not 0 <= c < num_features]
        if bad:  # the kernel reads x[b, column] without a range check of its own
            raise ValueError(f"tabular encoder: categorical column(s) {bad} outside the input's {num_features} features")
        dim_of = dict(zip(self.tgt_columns, self._dims_int))
        rows: List[List[int]] = []
        numerical = [c for c in range(num_features) if c not in self.tgt_columns]
        for c in numerical:
            rows.append([c, 0, 0, 0, 0, 0])
        for c in self.one_hot_columns:
            rows.extend([c, 1, v, 0, dim_of[c], 0] for v in range(dim_of[c]))
        emb_slices = []
        for t_id, c in enumerate(self.embedding_columns):
            tab = self.embeddings[str(c)]
            emb_slices.append((len(rows), tab.out_dim))
            rows.extend([c, 2, k, t_id, dim_of[c], tab.out_dim] for k in range(tab.out_dim))
        plan = torch.tensor(rows, dtype=torch.int32).to(device)
        cols = torch.tensor(self.tgt_columns, dtype=torch.int32).to(device)
        dims = torch.tensor(self._dims_int, dtype=torch.int32).to(device)
        self._plans[key] = (plan, len(rows), len(numerical), emb_slices, cols, dims)
        return self._plans[key]

    def _table_pointers(self, device: torch.device) -> Tuple[Optional[Tensor], List[Tensor]]:
        tables = [self.embeddings[str(c)].weights for c in self.embedding_columns]
        if not tables:
            return None, []
        ptrs = tuple(t.data_ptr() for t in tables)
        if getattr(self, "_ptr_key", None) != ptrs:
            self._ptr_key = ptrs
            self._ptr_dev = torch.tensor(list(ptrs), dtype=torch.int64).to(device)
        return self._ptr_dev, tables

    def forward(self, x_batch: Tensor) -> Tensor:
        """merged_all [B, F - K + one_hot_dim + embedding_dim] (f32)"""
        lead = x_batch.shape[:-1]
        x2 = x_batch.reshape(-1, x_batch.shape[-1]).float().contiguous()
        plan, out_dim, n_num, emb_slices, _, _ = self._plan(x2.shape[1], x2.device)
        ptrs, tables = self._table_pointers(x2.device)
        out = HF.MLEncodeFn.apply(x2, plan, ptrs, out_dim, *tables)
        if self.training and any(self.embeddings[str(c)].dropout is not None for c in self.embedding_columns):
            pieces = [out[:, :emb_slices[0][0]]] if emb_slices else [out]
            for (start, width), c in zip(emb_slices, self.embedding_columns):
                piece = out[:, start:start + width]
                drop = self.embeddings[str(c)].dropout
                pieces.append(piece if drop is None else drop(piece.contiguous()))
            out = torch.cat(pieces, dim=-1)
        return out.view(*lead, out.shape[-1])

    def encode_result(self, x_batch: Tensor) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
        """(indices int64 [B, K], one_hot [B, one_hot_dim] or None, embedding [B, embedding_dim] or None) — the
        reference's `EncodingResult` (ml_encoder.py:73-88, eval-mode embedding: no dropout)."""
        x2 = x_batch.reshape(-1, x_batch.shape[-1]).float().contiguous()
        plan, out_dim, n_num, emb_slices, cols, dims = self._plan(x2.shape[1], x2.device)
        ptrs, tables = self._table_pointers(x2.device)
        indices = ops.ml_encode_indices(x2, cols, dims)
        merged = HF.MLEncodeFn.apply(x2, plan, ptrs, out_dim, *tables)
        one_hot = merged[:, n_num:n_num + self.one_hot_dim] if self.use_one_hot else None
        embedding = merged[:, n_num + self.one_hot_dim:] if self.use_embedding else None
        return indices, one_hot, embedding


class CommonMLModule(Module):
    """`CommonMLModel.forward` (models/ml/common.py:27-93) as a module: `m["encoder"]` (or None) + `m["module"]`;
    `module_config["input_dim"]` grows by the encoder's `dim_increment` (:45-52)."""

    def __init__(self, module_name: str, module_config: Dict[str, Any], encoder_settings: Optional[Dict[str, Any]] = None,
                 global_encoder_settings: Any = None):
        super().__init__()
        self.m = nn.ModuleDict()
        encoder = None if encoder_settings is None else MLEncoder(encoder_settings, global_encoder_settings)
        cfg = shallow_copy_dict(module_config)
        if encoder is not None:
            cfg["input_dim"] = cfg["input_dim"] + encoder.dim_increment
            self.m["encoder"] = encoder
        cfg["input_dim"] *= cfg.get("num_history", 1)
        self.m["module"] = build_module(module_name, config=cfg)

    def forward(self, net: Tensor, **kwargs: Any) -> Any:
        if "encoder" in self.m and not self.m["encoder"].is_empty:
            net = self.m["encoder"](net)
        if net.dim() > 2:
            net = net.contiguous().view(len(net), -1)
        return self.m["module"](net, **kwargs)
