"""The PixelCNN prior of the VQ pipeline (reference modules/cv/ar/pixel_cnn.py): `MaskedConv2d`, `PixelCNN` and its sampler on
csrc/pixelcnn.hip.

Training and the plain forward: a masked 7x7 layer with channels in multiples of 32 runs on the live-tap kernels of csrc/conv_masked.hip
(`MaskedConv2dFn` below, chosen by `functional.masked_conv_route`); every other geometry (the first layer without an embedding, other
kernel sizes) is `Conv2dFn` on the weight times the mask.  BatchNorm2d and LeakyReLU are the existing modules.

Sampling is not the reference's loop of img_size^2 forwards.  In eval mode the net is causal in raster order, so one pixel needs one
output column per layer; `PixelCNN.sample` prepares the live-tap filter packs, BatchNorm's eval affine and the per-code input table
once (`SamplerPlan`) and then walks every pixel inside ONE `ops.pixelcnn_sample` launch.  What a call launches is documented at
`PixelCNN.sample`."""
from typing import Any, List, NamedTuple, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from . import functional as HF
from . import ops
from .modules import BatchNorm2d, ChannelPadding, Conv2d, Lambda, LeakyReLU, _weight_data_replaced, get_conv_blocks
from .registry import register_auto_regressor


class MaskedConv2dFn(Function):
    """F.conv2d(x, weight * mask, bias, padding=3) of a `masked_conv_route(...) == MASKED` layer on the live taps only (T = 24 for mask
    "A", 25 for "B"): Conv2dFn's contract on both sides (NCHW or channels_last in, f32 / bf16; bf16 out, channels_last when `HF.NHWC[0]`
    asks for it).  Forward and dX are cfhip_conv_masked_bf16 on the forward / transposed live-tap pack (both packed HERE from the f32
    weight, never in backward, where an optimizer step inside backward may already be rewriting it); dW is the live-tap gather of the
    saved input in row chunks of `ops.MASKED_GATHER_BYTES` and one `tn` GEMM per chunk accumulating into a [Cout, T Cin] f32 buffer,
    then placed into the [Cout, Cin, 7, 7] gradient through `param_grad` (a direct leaf adds on a second pass, an arena slot is
    overwritten after a lazy zero-grad, a frozen weight is neither claimed nor launched for) with the masked taps written as zeros;
    db the column sum.  The masked taps of `weight` are never read."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], taps: int) -> Tensor:
        xn = HF.to_nhwc(x)
        b, cin, h, w = xn.shape
        cout = weight.shape[0]
        x_rows = HF.nhwc_rows(xn)
        wd = weight.detach().contiguous()
        y_rows = ops.conv_masked(x_rows, ops.conv_masked_pack(wd, taps), None if bias is None else bias.detach().reshape(-1).contiguous(),
                                 b, h, w, taps)
        ctx.weight, ctx.bias, ctx.taps, ctx.xshape = weight, bias, taps, (b, cin, h, w)
        ctx.nhwc_in = HF.is_nhwc(x) and x.dtype == torch.bfloat16
        need_dx = ctx.needs_input_grad[0]
        ctx.save_for_backward(x_rows, ops.conv_masked_pack(wd, taps, transposed=True) if need_dx else None)
        return HF._rows_out(y_rows, b, cout, h, w, HF.NHWC[0])

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x_rows, wpt = ctx.saved_tensors
        weight, bias, taps = ctx.weight, ctx.bias, ctx.taps
        b, cin, h, w = ctx.xshape
        cout = weight.shape[0]
        dy = HF.as_bf16_act(dy)
        dy_rows = HF.nhwc_rows(dy) if HF.is_nhwc(dy) else ops.transpose_batched(dy.contiguous().view(b, cout, h * w)).view(b * h * w, cout)
        dy_rows = dy_rows.contiguous()
        gw = gb = None
        if weight.requires_grad:
            def dw_into(out: Tensor, acc: bool) -> None:
                rows = b * h * w
                chunk = max(256, min(rows, ops.MASKED_GATHER_BYTES // (2 * taps * cin)) // 8 * 8)
                dwp = torch.empty((cout, taps * cin), dtype=torch.float32, device=out.device)
                work = torch.empty((min(chunk, rows), taps * cin), dtype=torch.bfloat16, device=out.device)
                for r0 in range(0, rows, chunk):
                    n = min(chunk, rows - r0)
                    g = ops.conv_masked_gather(x_rows, b, h, w, taps, r0, n, out=work[:n])
                    ops.gemm(dy_rows[r0:r0 + n], g, a_trans=True, b_trans=True, out=dwp, accumulate=r0 > 0)
                live = dwp.view(cout, taps, cin).permute(0, 2, 1)
                grid = out.view(cout, cin, 49)
                if acc:
                    grid[:, :, :taps] += live
                else:
                    grid[:, :, :taps] = live
                    grid[:, :, taps:] = 0.0

            gw = HF.param_grad(weight, dw_into)
        if bias is not None and bias.requires_grad:
            gb = HF.param_grad(bias, lambda out, acc: ops.colsum(dy_rows, out=out.view(-1), accumulate=acc))
        dx = None
        if ctx.needs_input_grad[0]:
            dx_rows = ops.conv_masked(dy_rows, wpt, None, b, h, w, taps, mirror=True)
            dx = HF.rows_to_nhwc(dx_rows, b, cin, h, w) if ctx.nhwc_in else ops.transpose_batched(dx_rows.view(b, h * w, cin)).view(b, cin, h, w)
        return dx, gw, gb, None


def masked_conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], taps: int) -> Tensor:
    return HF._apply(MaskedConv2dFn, x, weight, bias, taps)


class MaskedConv2d(Conv2d):
    """reference pixel_cnn.py:20-65: `Conv2d` whose taps at and after the centre (mask "A") or after it (mask "B") in raster order are
    zero.  Buffer `mask` (the weight's shape: 1 on the rows above the centre and on the centre row left of the centre, "B" also on the
    centre).  The forward zeroes the masked taps of the parameter in place as the reference does (`weight.data *= mask`), so a
    checkpoint written after a forward equals the reference's.

    One deliberate deviation: the gradient of a masked tap is exactly ZERO here (the live-tap route writes zeros there; on the other
    route the convolution sees `weight * mask`, whose backward multiplies by the mask; `transform_kernel`, `demodulate` and `style`,
    which would carry gradient to the masked taps, are refused); the reference's convolution hands back the unmasked gradient there.  Those values never reach the function
    (the taps are zeroed again before every use), but they do enter a global gradient-norm clip; zero is the gradient of the function
    that is computed."""

    mask: Tensor

    def __init__(self, mask_type: str, in_channels: int, out_channels: int, *, kernel_size: int, groups: int = 1, stride: int = 1,
                 dilation: int = 1, padding: Any = "same", transform_kernel: bool = False, bias: bool = True, demodulate: bool = False):
        if mask_type not in ("A", "B"):
            raise ValueError(f"mask_type = {mask_type!r}: 'A' or 'B'")
        if transform_kernel or demodulate:
            raise NotImplementedError("MaskedConv2d: `transform_kernel` / `demodulate` act on the whole filter and would reach the masked "
                                      "taps; the PixelCNN uses neither")
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, groups=groups, stride=stride, dilation=dilation,
                         padding=padding, transform_kernel=transform_kernel, bias=bias, demodulate=demodulate)
        self.mask_type = mask_type
        _, _, h, w = self.weight.shape
        mask = torch.ones_like(self.weight.data)
        mask[:, :, h // 2, w // 2 + (mask_type == "B"):] = 0.0
        mask[:, :, h // 2 + 1:] = 0.0
        self.register_buffer("mask", mask)

    def zero_masked_taps(self) -> None:
        """`weight.data *= mask`.  An in-place write through `.data` does not bump the parameter's version, which keys its bf16 shadow
        (`functional.shadow_bf16`; inside an `optim.ParamArena` the shadow is a slice only the optimizer refreshes): the key is dropped
        so that whoever reads the shadow next casts the zeroed values."""
        self.weight.data.mul_(self.mask)
        _weight_data_replaced(self.weight)

    def _effective_weight(self, style: Optional[Tensor]) -> Tensor:
        if style is not None:
            raise NotImplementedError("MaskedConv2d: `style` is not built (its modulation would carry gradient to the masked taps)")
        return super()._effective_weight(style) * self.mask  # equal to the weight after the zeroing; its backward zeroes the masked taps' gradient

    def forward(self, net: Tensor, style: Optional[Tensor] = None, *, transpose: bool = False) -> Tensor:
        self.zero_masked_taps()
        route = HF.masked_conv_route(self.in_c, self.out_c, self.kernel_size, self.stride, self.padding, self.dilation, self.groups)
        plain = style is None and not transpose and self.reflection_pad is None and self.weight_scale is None
        if HF.MASKED_CONV and route == HF.MASKED and plain:  # the live-tap kernels: the masked taps are never read, their gradient is written as zeros
            return masked_conv2d(net, self.weight, self.bias, ops.MASKED_TAPS[self.mask_type])
        return super().forward(net, style, transpose=transpose)


class Embedding(nn.Embedding):
    """nn.Embedding (pixel_cnn.py:115) on the HIP lookup: f32 [..., D]"""

    def forward(self, indices: Tensor) -> Tensor:  # type: ignore
        return HF.embedding(indices, self.weight)


class SamplerPlan(NamedTuple):
    """what `PixelCNN.sampler_plan` prepares once per call (see ops.pixelcnn_sample / include/cfhip.h)"""

    in_table: Tensor   # bf16 [U, K, Cin0]
    label_row: Tensor  # int32 [B]
    packs: Tensor
    scale: Tensor      # f32 [L, C]
    shift: Tensor
    head_pack: Tensor
    head_bias: Tensor


class SamplerState(NamedTuple):
    """what a walk over the pixels leaves behind and a later launch continues from"""

    codes: Tensor            # int64 [B, 1, H, W]
    in0: Tensor              # bf16 [B, H, W, Cin0]
    act: Tensor              # bf16 [L, B, H, W, C]
    logits: Tensor           # f32 [B, H, W, K] (return_logits) or the [B, K] scratch


def sample_philox_range(num_samples: int, img_size: int, offset: int = 0) -> Tuple[int, int]:
    """the half-open Philox counter range [lo, hi) a `PixelCNN.sample(num_samples, img_size=img_size, offset=offset)` draws from under
    its seed: one word per pixel, element e = (b H + i) W + j uses word e % 4 of counter offset + e // 4 (csrc/pixelcnn.hip)"""
    total = int(num_samples) * int(img_size) * int(img_size)
    return int(offset), int(offset) + (total + 3) // 4


@register_auto_regressor("pixel_cnn")
class PixelCNN(nn.Module):
    """reference pixel_cnn.py:68-165 (IAutoRegressor): codes int64 [B, 1, H, W] -> logits [B, num_codes, H, W].  Same constructor
    keywords and state-dict keys (`to_blocks.1.weight` with `need_embedding`, `channel_padding.*`, `net.<l>.0.{weight,mask}`,
    `net.<l>.1.*` of the BatchNorm, `net.<L>.{weight,bias}` of the head)."""

    def __init__(self, num_codes: int, in_channels: int = 3, need_embedding: bool = False, latent_channels: int = 128, *,
                 norm_type: Optional[str] = "batch", num_layers: int = 6, channel_padding: Optional[int] = 16,
                 num_classes: Optional[int] = None):
        super().__init__()
        if in_channels != 1:
            raise ValueError("`PixelCNN` requires `in_channels` to be 1")
        self.in_channels, self.num_codes, self.latent_channels, self.num_classes = in_channels, num_codes, latent_channels, num_classes
        self.need_embedding, self.norm_type, self.num_layers = need_embedding, norm_type, num_layers

        def _get_block(in_nc: int, out_nc: int, mask_type: str) -> nn.Sequential:
            return nn.Sequential(*get_conv_blocks(in_nc, out_nc, 7, 1, bias=False, norm_type=norm_type, activation=LeakyReLU(0.2),
                                                  conv_base=MaskedConv2d, padding=3, mask_type=mask_type))

        if not need_embedding:
            start_channels = in_channels
            self.to_blocks = nn.Sequential(Lambda(lambda t: t.float() / (num_codes - 1), name="normalize"))
        else:
            start_channels = latent_channels
            self.to_blocks = nn.Sequential(Lambda(lambda t: t.squeeze(1), name="squeeze"), Embedding(num_codes, latent_channels),
                                           Lambda(lambda t: t.permute(0, 3, 1, 2), name="permute"))
        self.channel_padding = None
        if channel_padding is not None:
            self.channel_padding = ChannelPadding(start_channels, channel_padding, num_classes=num_classes)
        elif num_classes is not None:
            raise ValueError("`channel_padding` should be provided when `num_classes` is provided")
        blocks: List[nn.Module] = [_get_block(start_channels, latent_channels, "A")]
        for _ in range(num_layers - 1):
            blocks.append(_get_block(latent_channels, latent_channels, "B"))
        blocks.append(Conv2d(latent_channels, num_codes, kernel_size=1))
        self.net = nn.Sequential(*blocks)

    @property
    def is_conditional(self) -> bool:
        return self.num_classes is not None

    def get_sample_labels(self, num_samples: int, class_idx: Optional[int] = None) -> Optional[Tensor]:
        """reference cv/common.py IConditional.get_sample_labels"""
        if self.num_classes is None:
            return None
        device = next(self.parameters()).device
        if class_idx is not None:
            return torch.full([num_samples], class_idx, device=device)
        return torch.randint(self.num_classes, [num_samples], device=device)

    def forward(self, net: Tensor, labels: Optional[Tensor] = None) -> Tensor:
        net = self.to_blocks(net)
        if self.channel_padding is not None:
            net = self.channel_padding(net, labels)
        return self.net(net)

    # ---- sampling -------------------------------------------------------------------------------------------------------------

    def _sampler_refusal(self) -> None:
        if self.training:
            raise RuntimeError("PixelCNN.sample needs eval mode: in training mode BatchNorm normalises with the statistics of the batch, "
                               "which lets every pixel see every other one (the net is no longer causal) and makes the reference's own "
                               "result depend on the batch it is drawn in; call .eval() first")
        if self.norm_type not in (None, "batch"):
            raise NotImplementedError(f"PixelCNN.sample: norm_type = '{self.norm_type}' is not built into the sampling kernel "
                                      "(None and 'batch' are)")
        why = ops.pixelcnn_shape_refusal(self.latent_channels, self.num_codes, self.num_layers)
        if why is not None:
            raise NotImplementedError(f"PixelCNN.sample: {why}")

    @torch.no_grad()
    def sampler_plan(self, labels: Optional[Tensor], num_samples: int) -> SamplerPlan:
        """filter packs, BatchNorm's eval affine and the input table of one `sample` call.  The table is the module's own
        `to_blocks` + `channel_padding` run on every code (and every distinct label of the call) as a [U K, 1, 1, 1] batch, so its
        rounding is the forward's."""
        self._sampler_refusal()
        dev = next(self.parameters()).device
        k, c, nl = self.num_codes, self.latent_channels, self.num_layers
        if self.is_conditional:
            if labels is None:
                raise ValueError("`labels` should be provided for a conditional PixelCNN")
            uniq, inverse = torch.unique(labels.view(-1).to(dev), return_inverse=True)
            if inverse.numel() != num_samples:
                raise ValueError(f"`labels` holds {inverse.numel()} entries for {num_samples} samples")
        else:
            uniq, inverse = None, torch.zeros(num_samples, dtype=torch.int64, device=dev)
        u = 1 if uniq is None else uniq.numel()
        all_codes = torch.arange(k, device=dev).repeat(u).view(u * k, 1, 1, 1)
        x0 = self.to_blocks(all_codes)
        if self.channel_padding is not None:
            x0 = self.channel_padding(x0, None if uniq is None else uniq.repeat_interleave(k))
        in_table = x0.reshape(u, k, -1).to(torch.bfloat16).contiguous()
        packs, scales, shifts = [], [], []
        for l in range(nl):
            conv, norm = self.net[l][0], self.net[l][1]
            conv.zero_masked_taps()
            taps = 24 if l == 0 else 25
            w = conv.weight.detach()
            packs.append(ops.pixelcnn_pack(w.permute(0, 2, 3, 1).reshape(c, 49, w.shape[1])[:, :taps].reshape(c, -1)))
            if isinstance(norm, BatchNorm2d):
                sc = norm.weight.detach().float() * torch.rsqrt(norm.running_var.float() + norm.eps)
                scales.append(sc)
                shifts.append(norm.bias.detach().float() - norm.running_mean.float() * sc)
            else:
                scales.append(torch.ones(c, device=dev))
                shifts.append(torch.zeros(c, device=dev))
        head = self.net[nl]
        return SamplerPlan(in_table, inverse.to(torch.int32).contiguous(), torch.cat(packs), torch.stack(scales).contiguous(),
                           torch.stack(shifts).contiguous(), ops.pixelcnn_pack(head.weight.detach().view(k, c)),
                           head.bias.detach().float().contiguous())

    def sampler_state(self, num_samples: int, img_size: int, *, forced: Optional[Tensor] = None, return_logits: bool = False) -> SamplerState:
        dev = next(self.parameters()).device
        shape = (num_samples, self.in_channels, img_size, img_size)
        if forced is not None:
            if tuple(forced.shape) != shape or forced.dtype != torch.int64:
                raise ValueError(f"`forced` must be int64 {list(shape)}, got {forced.dtype} {list(forced.shape)}")
            codes = forced.to(dev).contiguous().clone()
            if codes.numel() and not bool(((codes >= 0) & (codes < self.num_codes)).all()):
                raise ValueError(f"`forced` holds codes outside [0, {self.num_codes})")
        else:
            codes = torch.zeros(shape, dtype=torch.int64, device=dev)
        cin0 = self.latent_channels if self.need_embedding else 1
        b, s, c = num_samples, img_size, self.latent_channels
        return SamplerState(codes, torch.empty((b, s, s, cin0), dtype=torch.bfloat16, device=dev),
                            torch.empty((self.num_layers, b, s, s, c), dtype=torch.bfloat16, device=dev),
                            torch.empty((b, s, s, self.num_codes) if return_logits else (b, self.num_codes), dtype=torch.float32, device=dev))

    def sample_pixels(self, plan: SamplerPlan, state: SamplerState, first_pixel: int, last_pixel: int, *, forced: bool = False,
                      seed: int = 0, offset: int = 0) -> None:
        """ONE launch over the pixels [first_pixel, last_pixel) of `state`; chained calls over consecutive ranges equal one call over
        their union bit for bit."""
        ops.pixelcnn_sample(state.codes, plan.label_row, plan.in_table, state.in0, state.act, plan.packs, plan.scale, plan.shift,
                            plan.head_pack, plan.head_bias, state.logits, first_pixel=first_pixel, last_pixel=last_pixel, forced=forced,
                            seed=seed, offset=offset)

    @torch.no_grad()
    def sample(self, num_samples: int, *, img_size: int, labels: Optional[Tensor] = None, class_idx: Optional[int] = None,
               seed: Optional[int] = None, offset: int = 0, forced: Optional[Tensor] = None,
               return_logits: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """reference pixel_cnn.py:142-165: int64 codes [num_samples, 1, img_size, img_size], drawn pixel by pixel in raster order.

        The draw is the library's Philox4x32-10 stream, not torch's generator: `seed` (None: one from torch's CPU generator) and
        `offset` select it, `sample_philox_range` tells which counters a call consumes, and a pixel's draw depends on (seed, offset,
        sample index, pixel) only.  `forced` (int64 [B, 1, H, W]) replaces the draw by the given codes (teacher forcing);
        `return_logits` also returns the f32 logits [B, H, W, num_codes] every pixel was drawn from.

        Launches: the walk over all img_size^2 pixels is exactly ONE `cfhip_pixelcnn_sample` launch.  In front of it the preparation
        (`sampler_plan`) makes num_layers + 1 `ops.pixelcnn_pack` calls and one forward of `to_blocks` + `channel_padding` on the
        [labels x num_codes] table: the same sequence of operations for a given module and label set whatever `img_size` is."""
        self._sampler_refusal()
        if not self.is_conditional:
            labels = None
        elif labels is None:
            labels = self.get_sample_labels(num_samples, class_idx)
        state = self.sampler_state(num_samples, img_size, forced=forced, return_logits=return_logits)
        plan = self.sampler_plan(labels, num_samples)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.sample_pixels(plan, state, 0, img_size * img_size, forced=forced is not None, seed=seed, offset=offset)
        return (state.codes, state.logits) if return_logits else state.codes
