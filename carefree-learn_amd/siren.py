"""Siren and ImgSiren on the fused coordinate-MLP kernel of csrc/siren.hip: the host side of the reference's `cflearn.modules.implicit`
(siren.py) -- `make_grid`, `img_siren_head`, the parameter holders `SirenLayer` and `Modulator` with the reference's state-dict keys,
initial values and random-number order, `Siren`, `ImgSiren`, and the stand-alone `Sine` activation of `build_activation("sine")`.

`SirenFn` packs the hidden and head weights once per forward (`ops.siren_pack`) and runs ONE `ops.siren_fwd` launch for all layers and
the head.  Without a wanted gradient nothing of size M x latent exists; with one it keeps the sine and cosine of every layer as bf16
words (DESIGN §3.19 weighs this against recomputing).  Its backward is one `ops.siren_bwd` launch, then one `ops.siren_reduce` per
wanted f32 sum and one `tn` GEMM per wanted hidden weight, every parameter's destination claimed through `functional.param_grad`
(nested, `functional.grads_in_one_launch`); a parameter with requires_grad = False gets no destination and no reduce launch.  The
Function is once-differentiable: `ddr`'s create_graph=True density needs a double backward that is not built."""
import math
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import functional as HF
from . import nbm, ops

LABEL_KEY = "labels"  # reference constants.py:7


def make_grid(size: int, in_dim: int, device: Optional[torch.device] = None) -> Tensor:
    """reference siren.py:21-24, computed on the CPU (torch.linspace's CPU values are the reference's bits) and moved"""
    tensors = [torch.linspace(-1.0, 1.0, steps=size)] * in_dim
    grid = torch.stack(torch.meshgrid(*tensors, indexing="ij"), dim=-1)
    grid = grid.view(1, -1, grid.shape[-1])
    return grid if device is None else grid.to(device)


def img_siren_head(size: int, out_channels: int) -> Callable[[Tensor], Tensor]:
    """reference siren.py:27-33"""

    def _head(t: Tensor) -> Tensor:
        t = t.view(-1, size, size, out_channels)
        t = t.permute(0, 3, 1, 2)
        return t

    return _head


class SineFn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor, w: float) -> Tensor:
        xd = x.detach().float().contiguous()
        ctx.w = w
        ctx.save_for_backward(xd)
        return ops.sine_fwd(xd, w)

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (xd,) = ctx.saved_tensors
        return ops.sine_bwd(dy.float().contiguous(), xd, ctx.w), None


class Sine(nn.Module):
    """`build_activation("sine", {"w": ...})` (reference activations.py:130-137): f32 sin(w x) on the elementwise kernels of csrc/siren.hip"""

    def __init__(self, *, w: float = 1.0):
        super().__init__()
        self.w = w

    def extra_repr(self) -> str:
        return f"w={self.w}"

    def forward(self, net: Tensor) -> Tensor:
        if not net.is_cuda:
            raise RuntimeError(f"Sine: the input must live on the HIP device (got {net.device}); there is no CPU path")
        return SineFn.apply(net, float(self.w))


class SirenLayer(nn.Module):
    """the parameters of one layer (reference siren.py:36-70): `weight` [out_dim, in_dim] and `bias` [out_dim] drawn as there (the weight
    first).  The layer is never called: `SirenFn` reads its parameters."""

    def __init__(self, in_dim: int, out_dim: int, *, w_sin: float = 1.0, c_init: float = 6.0, bias: bool = True, is_first: bool = False,
                 activation: Optional[nn.Module] = None):
        super().__init__()
        self.in_dim, self.is_first, self.w_sin = in_dim, is_first, w_sin
        weight = torch.zeros(out_dim, in_dim)
        w_std = (1.0 / in_dim) if is_first else (math.sqrt(c_init / in_dim) / w_sin)
        weight.uniform_(-w_std, w_std)
        self.weight = nn.Parameter(weight)
        self.bias = None
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_dim).uniform_(-w_std, w_std))
        self.activation = activation if activation is not None else Sine(w=w_sin)


class ReluF32Fn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        y = ops.relu_f32_fwd(x.detach().float().contiguous())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (y,) = ctx.saved_tensors
        return ops.relu_f32_bwd(dy.float().contiguous(), y)


class Modulator(nn.Module):
    """reference siren.py:73-94: `blocks.<i>.0` = nn.Linear(latent or 2 latent, latent), then ReLU; over the B latent rows in f32 end to
    end: the Linear on the f32 GEMM (`nbm.head`: `ops.sgemm_f32`, f32 gradients), the ReLU on the f32 kernel of csrc/siren.hip, the
    concatenation a torch indexing op.  On the bf16 `functional.linear` path pre-activations near zero flip their ReLU mask, and with B
    rows a few flips put modulator.blocks.1.0.weight at 1.07 x the reference's bf16-autocast distance."""

    def __init__(self, in_dim: int, latent_dim: int, num_layers: int):
        super().__init__()
        blocks = []
        for i in range(num_layers):
            dim = in_dim if i == 0 else (latent_dim + in_dim)
            blocks.append(nn.Sequential(nn.Linear(dim, latent_dim), nn.ReLU(inplace=True)))
        self.blocks = nn.ModuleList(blocks)

    def forward(self, z: Tensor) -> Tuple[Tensor, ...]:
        z = z.float().contiguous()
        net, nets = z, []
        for block in self.blocks:
            net = ReluF32Fn.apply(nbm.head(net, block[0].weight, block[0].bias))
            nets.append(net)
            net = torch.cat((net, z), dim=1)
        return tuple(nets)


class SirenFn(Function):
    """out f32 [B, N, out_dim] of Siren.forward's layer loop and head (reference siren.py:185-187).  `x` is init f32 [B, N, in_dim], or
    with `shared` the grid f32 [N, in_dim]; `mods` f32 [L, B, latent]; params = the L layer weights, the head weight and, with `bias`,
    the L layer biases and the head bias."""

    @staticmethod
    def forward(ctx: Any, sh: ops.SirenShape, shared: bool, bias: bool, save: bool, x: Tensor, mods: Tensor, *params: Tensor) -> Tensor:
        n_l = sh.layers
        weights = [p.detach() for p in params[:n_l + 1]]
        xd = x.detach().reshape(-1, sh.in_dim)
        md = mods.detach()
        packed = ops.siren_pack(weights[1:n_l], weights[n_l], transposed=save)
        bcat = torch.cat([p.detach().reshape(-1) for p in params[n_l + 1:]]) if bias else None
        out, ss, sc = ops.siren_fwd(sh, xd, shared, weights[0], packed, bcat, md, save=save)
        ctx.sh, ctx.shared, ctx.bias, ctx.params = sh, shared, bias, params
        if save:
            ctx.save_for_backward(xd, md, packed, ss, sc)
        return out.view(sh.b, sh.n, sh.out_dim)

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        if not ctx.saved_tensors:
            raise RuntimeError("SirenFn: the forward ran without grad mode and saved nothing; there is nothing to differentiate")
        xd, md, packed, ss, sc = ctx.saved_tensors
        sh, params = ctx.sh, ctx.params
        n_l = sh.layers
        names = [f"w{i}" for i in range(n_l)] + ["wh"] + ([f"b{i}" for i in range(n_l)] + ["bh"] if ctx.bias else [])
        want = {name: p for name, p in zip(names, params) if p.requires_grad}
        want_dx = ctx.needs_input_grad[4] and not ctx.shared
        want_dm = ctx.needs_input_grad[5]
        dyd = dy.float().reshape(sh.m, sh.out_dim).contiguous()
        res: List[Optional[Tensor]] = [None, None]

        def launch(dests: Dict[str, Tensor], accumulate: Sequence[str]) -> None:
            hidden = [i for i in range(1, n_l) if f"w{i}" in dests]
            ws, dx, dpre, hprev = ops.siren_bwd(sh, dyd, xd, ctx.shared, params[0].detach(), packed, params[n_l].detach(), md, ss, sc,
                                                want_dx=want_dx, want_hidden=bool(hidden))
            res[0] = dx
            for name, dest in dests.items():
                acc = name in accumulate
                if name == "w0":
                    ops.siren_reduce(sh, ws, "dw0", dest, accumulate=acc)
                elif name == "wh":
                    ops.siren_reduce(sh, ws, "dwhead", dest, accumulate=acc)
                elif name == "bh":
                    ops.siren_reduce(sh, ws, "dbhead", dest, accumulate=acc)
                elif name[0] == "b":
                    ops.siren_reduce(sh, ws, "db", dest, layer=int(name[1:]), accumulate=acc)
                else:  # a hidden weight: dW_l = dpre_l^T h_{l-1}, one tn GEMM over the M rows
                    i = int(name[1:])
                    # (a [latent, latent] result has at most four output tiles: without the split four workgroups walk all M rows)
                    ops.gemm(dpre[i - 1], hprev[i - 1], a_trans=True, b_trans=True, out=dest, accumulate=acc,
                             split_k=ops.pick_split_k(sh.latent, sh.latent, sh.m))
            if want_dm:
                res[1] = ops.siren_reduce(sh, ws, "dmods", torch.empty_like(md))

        grads = HF.grads_in_one_launch(want, launch) if (want or want_dx or want_dm) else {}
        dx = res[0].view(sh.b, sh.n, sh.in_dim) if res[0] is not None else None
        return (None, None, None, None, dx, res[1], *(grads.get(name) for name in names))


def _check_ranges(in_dim: int, out_dim: int, latent_dim: int, num_layers: int, final_activation: Optional[str]) -> None:
    if not ops.siren_latent_ok(latent_dim):
        raise NotImplementedError(f"Siren: latent_dim = {latent_dim} is outside the kernel (a multiple of 32 in 32 .. {ops.SIREN_MAX_LATENT}; "
                                  "DESIGN §8)")
    if not 1 <= in_dim <= ops.SIREN_MAX_IN:
        raise NotImplementedError(f"Siren: in_dim = {in_dim} is outside the kernel (1 .. {ops.SIREN_MAX_IN}; DESIGN §8)")
    if not 1 <= out_dim <= ops.SIREN_MAX_OUT:
        raise NotImplementedError(f"Siren: out_dim = {out_dim} is outside the kernel (1 .. {ops.SIREN_MAX_OUT}; DESIGN §8)")
    if num_layers < 1:
        raise NotImplementedError(f"Siren: num_layers = {num_layers} is outside the kernel (>= 1; DESIGN §8)")
    if final_activation is not None:
        raise NotImplementedError(f"Siren: final_activation = {final_activation!r} is not built, only None is (DESIGN §8)")


class Siren(nn.Module):
    """reference siren.py:97-187.  State keys `grid`, `blocks.<i>.weight/bias`, `modulator.blocks.<i>.0.weight/bias`,
    `head.weight/bias`; the same torch.manual_seed gives the reference's parameters bit for bit."""

    grid: Optional[Tensor]

    def __init__(self, size: Optional[int], in_dim: int, out_dim: int, latent_dim: int, *, num_layers: int = 4, w_sin: float = 1.0,
                 w_sin_initial: float = 30.0, bias: bool = True, final_activation: Optional[str] = None, keep_edge: bool = True,
                 use_modulator: bool = True):
        super().__init__()
        _check_ranges(in_dim, out_dim, latent_dim, num_layers, final_activation)
        self.in_dim, self.out_dim, self.num_layers, self.latent_dim = in_dim, out_dim, num_layers, latent_dim
        self.w_sin, self.w_sin_initial, self.has_bias = w_sin, w_sin_initial, bias
        blocks = []
        for i in range(num_layers):
            is_first = i == 0
            blocks.append(SirenLayer(in_dim if is_first else latent_dim, latent_dim, w_sin=w_sin_initial if is_first else w_sin, bias=bias,
                                     is_first=is_first))
        self.blocks = nn.ModuleList(blocks)
        self.keep_edge = keep_edge
        if size is None:
            self.grid = None
        else:
            self.register_buffer("grid", make_grid(size, in_dim))
        self.modulator = Modulator(latent_dim, latent_dim, num_layers) if use_modulator else None
        self.head = SirenLayer(latent_dim, out_dim, w_sin=w_sin, bias=bias, activation=nn.Identity())
        self._grids: Dict[Tuple[int, str], Tensor] = {}

    def _sized_grid(self, size: int, device: torch.device) -> Tensor:
        key = (size, str(device))
        if key not in self._grids:
            self._grids[key] = make_grid(size, self.in_dim, device)[0].contiguous()
        return self._grids[key]

    def forward(self, inp: Union[Tensor, Tuple[Tensor, ...]], *, init: Optional[Tensor] = None, size: Optional[int] = None) -> Tensor:
        n_l = self.num_layers
        if self.modulator is None:
            if isinstance(inp, Tensor):
                raise TypeError("Siren: without a modulator `inp` is the tuple of modulations, one [B, latent_dim] tensor per layer")
            mods = tuple(inp)
            if len(mods) < n_l:
                raise ValueError(f"Siren: {len(mods)} modulations for {n_l} layers (the reference's zip would drop layers)")
            mods = mods[:n_l]
        else:
            if not isinstance(inp, Tensor) or inp.dim() != 2 or inp.shape[1] != self.latent_dim:
                raise ValueError(f"Siren: a [B, {self.latent_dim}] latent expected, got {tuple(inp.shape) if isinstance(inp, Tensor) else type(inp)}")
            mods = None
        if init is None:
            if self.grid is None and size is None:
                raise ValueError("`init` should be provided for None sized `Siren`")
            if size is not None and not self.keep_edge:
                raise NotImplementedError("Siren: `size=` with keep_edge=False: the reference's grid[1:-1] slices the leading dimension of a "
                                          "[1, N, d] grid and yields an empty tensor (siren.py:181-182); not built (DESIGN §8)")
            if self.modulator is None:
                raise NotImplementedError("Siren: a tuple of modulations without `init`: the reference repeats the grid by the number of "
                                          "layers, not by the batch size (siren.py:183); not built (DESIGN §8)")
        if mods is None:
            if not inp.is_cuda:
                raise RuntimeError(f"Siren: the latent must live on the HIP device (got {inp.device}); there is no CPU path")
            mods = self.modulator(inp)
        b = mods[0].shape[0]
        for m in mods:
            if m.dim() != 2 or tuple(m.shape) != (b, self.latent_dim):
                raise ValueError(f"Siren: every modulation must be [B, {self.latent_dim}], got {tuple(m.shape)}")
        if init is not None and (init.dim() != 3 or init.shape[0] != b or init.shape[2] != self.in_dim):
            raise ValueError(f"Siren: `init` must be [{b}, N, {self.in_dim}], got {tuple(init.shape)}")
        for m in mods:
            if not m.is_cuda:
                raise RuntimeError(f"Siren: the modulations must live on the HIP device (got {m.device}); there is no CPU path")
        device = mods[0].device
        if init is not None:
            if not init.is_cuda:
                raise RuntimeError(f"Siren: `init` must live on the HIP device (got {init.device}); there is no CPU path")
            x, shared, n = init.float().contiguous(), False, init.shape[1]
        else:
            x = self.grid[0] if size is None else self._sized_grid(size, device)
            if x.device != device:
                raise RuntimeError(f"Siren: the grid buffer lives on {x.device}, the latent on {device}")
            shared, n = True, x.shape[0]
        sh = ops.SirenShape(b, n, self.in_dim, self.latent_dim, self.out_dim, n_l, self.w_sin_initial, self.w_sin)
        stacked = torch.stack([m.float() for m in mods]).contiguous()
        params = [blk.weight for blk in self.blocks] + [self.head.weight]
        if self.has_bias:
            params += [blk.bias for blk in self.blocks] + [self.head.bias]
        # (inside Function.forward grad mode is off and needs_input_grad follows requires_grad alone: an inference forward under
        # torch.no_grad() must not keep the [L, M, latent] words)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, stacked, *params))
        return SirenFn.apply(sh, shared, self.has_bias, save, x, stacked, *params)


class ImgSiren(nn.Module):
    """reference siren.py:190-252; state keys `siren.*` and, conditional, `cond_padding.*`"""

    def __init__(self, img_size: int, out_channels: int, latent_dim: int = 256, num_classes: Optional[int] = None, conditional_dim: int = 16, *,
                 num_layers: int = 4, w_sin: float = 1.0, w_sin_initial: float = 30.0, bias: bool = True, final_activation: Optional[str] = None):
        super().__init__()
        from .modules import ChannelPadding, Lambda

        _check_ranges(2, out_channels, latent_dim, num_layers, final_activation)
        self.out_channels = out_channels
        self.cond_padding = None
        if num_classes is not None:
            self.cond_padding = ChannelPadding(latent_dim, conditional_dim, is_1d=True, num_classes=num_classes)
            self.cond_padding.mapping.out_f32 = True  # the conditioned latent enters the f32 modulator unrounded
        self.siren = Siren(img_size, 2, out_channels, latent_dim, num_layers=num_layers, w_sin=w_sin, w_sin_initial=w_sin_initial, bias=bias,
                           final_activation=final_activation)
        self.head = Lambda(img_siren_head(img_size, out_channels), name="head")

    def forward(self, net: Tensor, batch: Dict[str, Tensor]) -> Tensor:
        if self.cond_padding is not None:
            net = self.cond_padding(net, batch[LABEL_KEY].view(-1))
        net = self.siren(net)
        return self.head(net)

    def decode(self, z: Tensor, *, labels: Optional[Tensor], size: Optional[int] = None) -> Tensor:
        if self.cond_padding is not None:
            if labels is None:
                raise ValueError("`labels` should be provided in conditional `ImgSiren`")
            z = self.cond_padding(z, labels)
        net = self.siren(z, size=size)
        if size is None:
            return self.head(net)
        return img_siren_head(size, self.out_channels)(net)


__all__ = ["make_grid", "img_siren_head", "Sine", "SirenLayer", "Modulator", "Siren", "ImgSiren"]
