"""Tensor-level wrappers over the C-ABI (include/cfhip.h).  No autograd here.

Every function takes / returns torch tensors that live on the HIP device, launches on torch's
current stream and never synchronises.  PyTorch is used only as the owner of device memory.
"""
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import ctypes

import torch
from torch import Tensor

from . import _lib

_H = _lib.DEFINES  # the CFHIP_* integer #defines of include/cfhip.h: every constant below that the library shares is read from it
EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_QGELU, EPI_DQGELU = (_H["CFHIP_EPI_" + e] for e in ("NONE", "GELU", "RESIDUAL", "DGELU", "QGELU", "DQGELU"))

bf16 = torch.bfloat16
f32 = torch.float32


# The raw handle of torch's current HIP stream.  `torch.cuda.current_stream().cuda_stream` builds a Stream object through
# four Python layers (9 us per call: 768 + ~800 calls = 14 ms of the host's 65 ms per UNet 64^2 step, tools/host_profile.py);
# the two C entry points behind it take ~0.3 us.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: Tensor, dtype: torch.dtype, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"cfhip: `{name}` must live on the HIP device (got {t.device})")
    if t.dtype != dtype:
        raise TypeError(f"cfhip: `{name}` must be {dtype}, got {t.dtype}")


def _mat(t: Tensor, name: str) -> Tuple[int, int, int]:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"cfhip: `{name}` must be 2-D with a contiguous last dim, got {tuple(t.shape)} / {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def set_option(name: str, value: int) -> None:
    """process-wide tuning knob of libcfhip.so (see cfhip_set_option in include/cfhip.h)"""
    _lib.check(_lib.load().cfhip_set_option(name.encode(), int(value)), "set_option")


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------


FORCE_SPLIT_K = 0  # A/B runs: > 0 = every weight-gradient GEMM takes this split


def pick_split_k(m: int, n: int, k: int) -> int:
    """Split the reduction when the output has too few 128x128 tiles to fill 256 CUs."""
    if FORCE_SPLIT_K > 0:
        return FORCE_SPLIT_K
    tiles = ((m + 127) // 128) * ((n + 127) // 128)
    steps = (k + 63) // 64
    if tiles >= 256 or steps < 16:
        return 1
    # (deeper than 32: the reduce pass costs more than it fills.  Round 6 tried 64-128 slices aimed at 1 024 workgroups for long reductions
    # over <= 16 tiles: 256^2 x 1 UNet step -5 ms, level at 64^2 x 8 — and nothing once such reductions of >= 49 152 rows go to the grouped
    # whole-K launches (fused.LINEAR_DW_MIN_ROWS), which is worth as much: profiles/r06/unet_split_deep_ab.txt; removed)
    split = min(steps // 4, (512 + tiles - 1) // tiles, 32)
    return max(1, split)


class GemmTimer:
    """Opt-in (bench.py's roofline pass): HIP-event pairs around every GEMM launch of the REAL training step, recorded
    on the stream the kernel is launched on (torch's current stream at the call: the main stream or a side stream),
    keyed by (layout, M, N, K, epilogue).  Off by default: `ops.GEMM_TIMER is None` costs one attribute read."""

    def __init__(self) -> None:
        self.records: list = []

    def durations(self) -> dict:
        """key -> [count, total seconds]; synchronises on the recorded events.  A launch that took more than 8 x the median of
        its key (one 100 ms hiccup among 72 launches of a 150 us kernel was seen once: a profile step that had to grow the
        allocator) counts with the median instead — the table describes the steady state."""
        per: dict = {}
        for key, e0, e1 in self.records:
            e1.synchronize()
            per.setdefault(key, []).append(e0.elapsed_time(e1) * 1.0e-3)
        out: dict = {}
        for key, ds in per.items():
            med = sorted(ds)[len(ds) // 2]
            out[key] = [len(ds), sum(d if d <= 8.0 * med else med for d in ds)]
        return out


GEMM_TIMER: Optional[GemmTimer] = None


class FlopCounter:
    """Opt-in (bench.py --workload unet | clip): algorithmic MFMA-class FLOPs of the launches of a step, by family.
    GEMM 2*M*N*K; implicit 3x3 convolution 2 * pixels * Cout * 9 * Cin (forward, input gradient = the same kernel,
    weight gradient); attention 4 * B * H * Tq * Tk * dh forward and 2.5x that backward (5 products: the algorithmic
    count, not the 7 the two-pass backward executes)."""

    def __init__(self) -> None:
        self.flops = {"gemm": 0.0, "conv3x3": 0.0, "attention": 0.0}

    def total(self) -> float:
        return sum(self.flops.values())


FLOP_COUNTER: Optional[FlopCounter] = None


def gemm(
    a: Tensor,
    b: Tensor,
    *,
    a_trans: bool = False,
    b_trans: bool = False,
    bias: Optional[Tensor] = None,
    epilogue: int = EPI_NONE,
    aux_in: Optional[Tensor] = None,
    aux_out: Optional[Tensor] = None,
    out: Optional[Tensor] = None,
    out_dtype: torch.dtype = bf16,
    accumulate: bool = False,
    split_k: int = 1,
    bias_grad: Optional[Tensor] = None,
    bias_grad_accumulate: bool = False,
    config_rows: int = 0,
) -> Tensor:
    """C[m,n] = epilogue(sum_k A(m,k) B(n,k)); see cfhip_gemm_bf16 in include/cfhip.h.
    `bias_grad` (f32 [M], layout a_trans & b_trans only): (+)= sum_k A(m,k), i.e. colsum(dY) of a dW GEMM.
    `config_rows` > 0: these m rows belong to a row-wise problem of that many rows and are computed under ITS tile configuration
    (cfhip_gemm_bf16_rows: bit-identical to the same rows of the whole launch); a_trans, split_k, accumulate, bias_grad excluded."""
    # (this wrapper runs 400-500 times per UNet / CLIP step on the thread that issues every launch: shapes and strides are
    # read once as tuples, the checks are inline — tools/host_profile.py had it at 10 us per call, a tenth of the host's step)
    if a.dtype is not bf16 or b.dtype is not bf16 or not a.is_cuda or not b.is_cuda:
        _need(a, bf16, "a")
        _need(b, bf16, "b")
    sha, shb, sta, stb = a.shape, b.shape, a.stride(), b.stride()
    if len(sha) != 2 or sta[1] != 1:
        _mat(a, "a")
    if len(shb) != 2 or stb[1] != 1:
        _mat(b, "b")
    lda, ldb = sta[0], stb[0]
    m, k = (sha[1], sha[0]) if a_trans else (sha[0], sha[1])
    n, kb = (shb[1], shb[0]) if b_trans else (shb[0], shb[1])
    if k != kb:
        raise ValueError(f"cfhip gemm: reduction dims differ ({k} vs {kb})")
    if out is None:
        out = torch.empty((m, n), dtype=out_dtype, device=a.device)
        ldc, odt = n, out_dtype
    else:
        odt, sho, sto = out.dtype, out.shape, out.stride()
        if not out.is_cuda or (odt is not bf16 and odt is not f32) or len(sho) != 2 or sho[0] != m or sho[1] != n or sto[1] != 1:
            raise ValueError("cfhip gemm: bad `out`")
        ldc = sto[0]
    if bias is not None and (bias.dtype is not f32 or not bias.is_cuda or bias.numel() != n or not bias.is_contiguous()):
        _need(bias, f32, "bias")
        raise ValueError("cfhip gemm: bias must be a contiguous f32 [N]")
    if aux_in is not None or aux_out is not None:
        for t, nm in ((aux_in, "aux_in"), (aux_out, "aux_out")):
            if t is not None:
                # the residual operand follows the output dtype (f32 residual stream); everything else is bf16
                _need(t, f32 if (nm == "aux_in" and epilogue == EPI_RESIDUAL and odt is f32) else bf16, nm)
                stt = t.stride()
                if tuple(t.shape) != (m, n) or stt[1] != 1 or stt[0] != ldc:
                    raise ValueError(f"cfhip gemm: `{nm}` must match the output layout")
    if bias_grad is not None:
        _need(bias_grad, f32, "bias_grad")
        if bias_grad.numel() != m or not bias_grad.is_contiguous():
            raise ValueError("cfhip gemm: bias_grad must be a contiguous f32 [M]")
    ws, ws_bytes = None, 0
    if split_k > 1:
        ws = torch.empty((split_k * m * (n + (1 if bias_grad is not None else 0)),), dtype=f32, device=a.device)
        ws_bytes = ws.numel() * 4
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["gemm"] += 2.0 * m * n * k
    timer = GEMM_TIMER
    if timer is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if config_rows:
        if a_trans or split_k > 1 or accumulate or bias_grad is not None or config_rows < m:
            raise ValueError("cfhip gemm: config_rows takes a_trans = False, no split_k / accumulate / bias_grad, and at least m rows")
        rc = _lib.load().cfhip_gemm_bf16_rows(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(bias), _p(aux_in), _p(aux_out), m, n, k, lda,
                                              ldb, ldc, int(b_trans), epilogue, 1 if odt is f32 else 0, int(config_rows), _stream())
    else:
        rc = _lib.load().cfhip_gemm_bf16(
            a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(bias), _p(aux_in), _p(aux_out), m, n, k, lda,
            ldb, ldc, int(a_trans), int(b_trans), epilogue, 1 if odt is f32 else 0,
            int(accumulate), split_k, _p(ws), ws_bytes, _p(bias_grad), int(bias_grad_accumulate), _stream(),
        )
    _lib.check(rc, "gemm")
    if timer is not None:
        e1.record()
        layout = "tn" if a_trans else ("nn" if b_trans else "nt")
        timer.records.append(((layout, m, n, k, int(epilogue)), e0, e1))
    return out


def gemm_grouped_tn(problems: list) -> None:
    """Weight gradients of several Linear layers in ONE launch (cfhip_gemm_bf16_grouped_tn).

    `problems`: list of (dy [K, M] bf16, x [K, N] bf16, out [M, N] f32, accumulate, bias_grad f32 [M] or None,
    bias_grad_accumulate[, row_period]): out (+)= dy^T x, bias_grad (+)= colsum(dy).  256 x 256 tiles of all problems share the
    chip and every tile runs its whole reduction: no split-K workspace, no reduce pass.
    `row_period` (optional 7th entry; 0 = dense): the caller GUARANTEES that every row r of dy with r % row_period != 0 is zero;
    the tiles of that problem then walk only the K-steps that hold a row r = i * row_period — same bits, fewer steps
    (`k_period` of cfhip_gemm_problem: at least 32, the library rejects 0 < row_period < 32)."""
    if not problems:
        return
    arr = (_lib.GemmProblem * len(problems))()
    flops = 0.0
    for i, (dy, x, out, acc, bg, bg_acc, *period) in enumerate(problems):
        if len(period) > 1:
            raise ValueError(f"cfhip gemm_grouped_tn: problem {i}: 6 or 7 entries expected, got {6 + len(period)}")
        _need(dy, bf16, "dy")
        _need(x, bf16, "x")
        _need(out, f32, "out")
        k, m, lda = _mat(dy, "dy")
        kb, n, ldb = _mat(x, "x")
        if k != kb or tuple(out.shape) != (m, n) or out.stride(1) != 1:
            raise ValueError(f"cfhip gemm_grouped_tn: problem {i}: dy {tuple(dy.shape)} x {tuple(x.shape)} out {tuple(out.shape)}")
        if bg is not None:
            _need(bg, f32, "bias_grad")
            if bg.numel() != m or not bg.is_contiguous():
                raise ValueError("cfhip gemm_grouped_tn: bias_grad must be a contiguous f32 [M]")
        pr = arr[i]
        pr.A, pr.B, pr.C, pr.bias_grad = dy.data_ptr(), x.data_ptr(), out.data_ptr(), _p(bg)
        pr.M, pr.N, pr.K = m, n, k
        pr.lda, pr.ldb, pr.ldc = lda, ldb, out.stride(0)
        pr.accumulate, pr.bias_grad_accumulate = int(bool(acc)), int(bool(bg_acc))
        pr.k_period = int(period[0]) if period else 0
        flops += 2.0 * m * n * k
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["gemm"] += flops
    timer = GEMM_TIMER
    if timer is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if _lib.RECORDER is not None:
        # the operand addresses of this launch live in a host table, not in the argument tuple: a launch plan that moves its
        # input (fused.StackPlan.repoint) must be able to find and rewrite them — kind-3 entry = the table
        _lib.RECORDER.append((3, arr, len(problems)))
    rc = _lib.load().cfhip_gemm_bf16_grouped_tn(ctypes.cast(arr, ctypes.c_void_p), len(problems), _stream())
    _lib.check(rc, "gemm_grouped_tn")
    if timer is not None:
        e1.record()
        timer.records.append((("tn-grouped", tuple((int(pr.M), int(pr.N), int(pr.K)) for pr in arr), 0, 0, 0), e0, e1))


def colsum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[n] (f32) (+)= sum_m x[m, n]   (bias gradient)."""
    _need(x, bf16, "x")
    m, n, ldx = _mat(x, "x")
    if out is None:
        out = torch.empty((n,), dtype=f32, device=x.device)
        accumulate = False
    _need(out, f32, "out")
    lib = _lib.load()
    nbytes = lib.cfhip_colsum_workspace(m, n)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=x.device)
    rc = lib.cfhip_colsum_bf16(x.data_ptr(), out.data_ptr(), m, n, ldx, int(accumulate), ws.data_ptr(),
                               ws.numel() * 4, _stream())
    _lib.check(rc, "colsum")
    return out


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------


def layernorm_fwd(
    x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out: Optional[Tensor] = None,
    mean: Optional[Tensor] = None, rstd: Optional[Tensor] = None, out_f32: bool = False,
) -> Tuple[Tensor, Tensor, Tensor]:
    """x: bf16 or f32 [M, D] (row stride free) -> y bf16 (f32 with `out_f32`, f32 rows only) [M, D], mean f32 [M], rstd f32 [M]
    (`out` / `mean` / `rstd`: caller-owned destinations, e.g. row slices of larger tensors)."""
    _need(x, x.dtype if x.dtype in (bf16, f32) else bf16, "x")
    _need(gamma, f32, "gamma")
    _need(beta, f32, "beta")
    m, d, xs = _mat(x, "x")
    if out is not None:
        out_f32 = out.dtype == f32
    if out_f32 and x.dtype != f32:
        raise ValueError("cfhip layernorm_fwd: an f32 output is built for f32 rows only")
    y = torch.empty((m, d), dtype=f32 if out_f32 else bf16, device=x.device) if out is None else out
    mean = torch.empty((m,), dtype=f32, device=x.device) if mean is None else mean
    rstd = torch.empty((m,), dtype=f32, device=x.device) if rstd is None else rstd
    rc = _lib.load().cfhip_layernorm_fwd(
        x.data_ptr(), int(x.dtype == f32) | (2 if out_f32 else 0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
        rstd.data_ptr(), m, d, xs, y.stride(0), float(eps), _stream(),
    )
    _lib.check(rc, "layernorm_fwd")
    return y, mean, rstd


def layernorm4d_fwd(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    """The reference's 4-D `LN` (norms.py:30-46) on a contiguous bf16 [B, C, H, W]: per-sample mean / UNBIASED std over C*H*W,
    y = (x - mean) / (std + eps) * weight[c] + bias[c].  Returns (y bf16, mean f32 [B], std f32 [B])."""
    _need(x, bf16, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("cfhip layernorm4d_fwd: a contiguous [B, C, H, W] tensor is expected")
    if (weight is None) != (bias is None):
        raise ValueError("cfhip layernorm4d_fwd: weight and bias come together")
    b, c, h, w = x.shape
    lib = _lib.load()
    nbytes = lib.cfhip_layernorm4d_workspace(b, c, h * w)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    mean = torch.empty((b,), dtype=f32, device=x.device)
    std = torch.empty((b,), dtype=f32, device=x.device)
    _lib.check(lib.cfhip_layernorm4d_fwd(x.data_ptr(), _p(weight), _p(bias), y.data_ptr(), mean.data_ptr(), std.data_ptr(), b, c, h * w,
                                         float(eps), ws.data_ptr(), nbytes, _stream()), "layernorm4d_fwd")
    return y, mean, std


def layernorm4d_bwd(dy: Tensor, x: Tensor, weight: Optional[Tensor], mean: Tensor, std: Tensor, eps: float, *, want_dx: bool = True,
                    dweight: Optional[Tensor] = None, dbias: Optional[Tensor] = None, accumulate: bool = False) -> Optional[Tensor]:
    """dx bf16 (or None), dweight / dbias f32 [C] (+)= in place when given"""
    _need(dy, bf16, "dy")
    _need(x, bf16, "x")
    if dy.shape != x.shape or not dy.is_contiguous() or not x.is_contiguous():
        raise ValueError("cfhip layernorm4d_bwd: dy and x must be contiguous [B, C, H, W] of one shape")
    b, c, h, w = x.shape
    lib = _lib.load()
    nbytes = lib.cfhip_layernorm4d_workspace(b, c, h * w)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x) if want_dx else None
    _lib.check(lib.cfhip_layernorm4d_bwd(dy.data_ptr(), x.data_ptr(), _p(weight), mean.data_ptr(), std.data_ptr(), _p(dx), _p(dweight),
                                         _p(dbias), int(accumulate), b, c, h * w, float(eps), ws.data_ptr(), nbytes, _stream()),
               "layernorm4d_bwd")
    return dx


def layernorm_bwd(
    dy: Tensor,
    x: Tensor,
    gamma: Tensor,
    mean: Tensor,
    rstd: Tensor,
    *,
    dx_add: Optional[Tensor] = None,
    dgamma: Optional[Tensor] = None,
    dbeta: Optional[Tensor] = None,
    accumulate: bool = False,
    want_dx: bool = True,
    want_param_grads: bool = True,
    dx_out: Optional[Tensor] = None,
    dx_add_lo: Optional[Tensor] = None,
    dx_lo_out: Optional[Tensor] = None,
) -> Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """x bf16 or f32.  Returns (dx bf16 [M, D] (+ dx_add), dgamma f32 [D], dbeta f32 [D]).  `dx_out`: dense bf16 [M, D]
    destination for dx (e.g. a row slice of a full-batch tensor).  `dx_add_lo` / `dx_lo_out`: the SECOND bf16 words of dx_add / dx
    when the residual-gradient stream is carried in two words (cfhip_layernorm_bwd2), dense [M, D] like the first."""
    _need(dy, bf16, "dy")
    _need(x, x.dtype if x.dtype in (bf16, f32) else bf16, "x")
    m, d, xs = _mat(x, "x")
    _, _, dys = _mat(dy, "dy")
    if dx_out is not None and want_dx:
        _need(dx_out, bf16, "dx_out")
        if tuple(dx_out.shape) != (m, d) or dx_out.stride(0) != d or dx_out.stride(1) != 1:
            raise ValueError("cfhip layernorm_bwd: dx_out must be a dense [M, D] bf16 tensor")
        dx = dx_out
    else:
        dx = torch.empty((m, d), dtype=bf16, device=x.device) if want_dx else None
    if dx_add is not None:
        _need(dx_add, bf16, "dx_add")
        if tuple(dx_add.shape) != (m, d) or dx_add.stride(0) != d or dx_add.stride(1) != 1:
            raise ValueError("cfhip layernorm_bwd: dx_add must be a dense [M, D] bf16 tensor")
    if not want_param_grads:
        dgamma = dbeta = None
    elif dgamma is None:
        dgamma = torch.empty((d,), dtype=f32, device=x.device)
        dbeta = torch.empty((d,), dtype=f32, device=x.device)
        accumulate = False
    lib = _lib.load()
    nbytes = lib.cfhip_layernorm_bwd_workspace(m, d) if want_param_grads else 0
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=x.device)
    if want_dx and (dx_add_lo is not None or dx_lo_out is not None):
        _check_lo(dx_add_lo, dx_lo_out, m, d)
        rc = lib.cfhip_layernorm_bwd2(
            dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dx_add),
            _p(dx_add_lo), _p(dx), _p(dx_lo_out), _p(dgamma), _p(dbeta), m, d, dys, xs, d, int(accumulate), ws.data_ptr(), nbytes,
            None, _stream())
        _lib.check(rc, "layernorm_bwd2")
        return dx, dgamma, dbeta
    rc = lib.cfhip_layernorm_bwd(
        dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
        _p(dx_add),
        _p(dx), _p(dgamma), _p(dbeta), m, d, dys, xs, d,
        int(accumulate), ws.data_ptr(), nbytes, _stream(),
    )
    _lib.check(rc, "layernorm_bwd")
    return dx, dgamma, dbeta


def _check_lo(dx_add_lo: Optional[Tensor], dx_lo_out: Optional[Tensor], m: int, d: int) -> None:
    for t, name in ((dx_add_lo, "dx_add_lo"), (dx_lo_out, "dx_lo_out")):
        if t is not None:
            _need(t, bf16, name)
            if tuple(t.shape) != (m, d) or t.stride(0) != d or t.stride(1) != 1:
                raise ValueError(f"cfhip layernorm_bwd: {name} must be a dense [M, D] bf16 tensor")


def split_f32(src: Tensor, hi: Optional[Tensor] = None, lo: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """f32 -> (hi, lo) bf16 with hi = bf16(v), lo = bf16(v - hi): the two words of the residual-gradient stream (cfhip_split_f32_bf16x2)"""
    _need(src, f32, "src")
    src = src.contiguous()
    hi = torch.empty(src.shape, dtype=bf16, device=src.device) if hi is None else hi
    lo = torch.empty(src.shape, dtype=bf16, device=src.device) if lo is None else lo
    _lib.check(_lib.load().cfhip_split_f32_bf16x2(src.data_ptr(), hi.data_ptr(), lo.data_ptr(), src.numel(), _stream()), "split_f32_bf16x2")
    return hi, lo


def join_bf16x2(hi: Tensor, lo: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """(hi, lo) bf16 -> f32 hi + lo (exact) (cfhip_join_bf16x2_f32)"""
    _need(hi, bf16, "hi")
    _need(lo, bf16, "lo")
    if not (hi.is_contiguous() and lo.is_contiguous() and hi.shape == lo.shape):
        raise ValueError("cfhip join_bf16x2: two dense bf16 tensors of one shape expected")
    out = torch.empty(hi.shape, dtype=f32, device=hi.device) if out is None else out
    _lib.check(_lib.load().cfhip_join_bf16x2_f32(hi.data_ptr(), lo.data_ptr(), out.data_ptr(), hi.numel(), _stream()), "join_bf16x2_f32")
    return out


def layernorm_bwd_partials(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, *, dx_add: Optional[Tensor] = None,
                           dx_out: Optional[Tensor] = None, dx_add_lo: Optional[Tensor] = None,
                           dx_lo_out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, int]:
    """The row kernel of `layernorm_bwd` alone: dx (+ dx_add) and the per-workgroup partial sums of dgamma | dbeta.  Returns
    (dx, workspace, rows) for `layernorm_bwd_reduce` — which may run on another stream (cfhip_layernorm_bwd_partials / _reduce)."""
    _need(dy, bf16, "dy")
    m, d, xs = _mat(x, "x")
    _, _, dys = _mat(dy, "dy")
    dx = dx_out if dx_out is not None else torch.empty((m, d), dtype=bf16, device=x.device)
    lib = _lib.load()
    nbytes = lib.cfhip_layernorm_bwd_workspace(m, d)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=x.device)
    rows = ctypes.c_int(0)
    if dx_add_lo is not None or dx_lo_out is not None:
        _check_lo(dx_add_lo, dx_lo_out, m, d)
        rc = lib.cfhip_layernorm_bwd2(dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      _p(dx_add), _p(dx_add_lo), dx.data_ptr(), _p(dx_lo_out), None, None, m, d, dys, xs, dx.stride(0), 0,
                                      ws.data_ptr(), nbytes, ctypes.byref(rows), _stream())
        _lib.check(rc, "layernorm_bwd2 (partials)")
        return dx, ws, rows.value
    rc = lib.cfhip_layernorm_bwd_partials(dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), gamma.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), _p(dx_add), dx.data_ptr(), m, d, dys, xs, dx.stride(0), ws.data_ptr(),
                                          nbytes, ctypes.byref(rows), _stream())
    _lib.check(rc, "layernorm_bwd_partials")
    return dx, ws, rows.value


def layernorm_bwd_reduce(ws: Tensor, rows: int, d: int, dgamma: Tensor, dbeta: Tensor, accumulate: bool) -> None:
    rc = _lib.load().cfhip_layernorm_bwd_reduce(ws.data_ptr(), rows, d, dgamma.data_ptr(), dbeta.data_ptr(), int(accumulate), _stream())
    _lib.check(rc, "layernorm_bwd_reduce")


# ---------------------------------------------------------------------------------------------
# attention (head_dim 64).  q / k / v / o are [B, T, H*64] views (any batch / token strides).
# ---------------------------------------------------------------------------------------------


def _bth(t: Tensor, name: str) -> Tuple[int, int, int, int, int]:
    _need(t, bf16, name)
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"cfhip attention: `{name}` must be [B, T, H*head_dim] with a contiguous last dim")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(0), t.stride(1)


def _mask_args(mask: Optional[Tensor], b: int, h: int, tq: int, tk: int):
    """mask: bool/uint8 'keep' mask broadcastable to [B, H, Tq, Tk] (True = attend)."""
    if mask is None:
        return None, None, 0, 0, 0
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    if mask.dtype != torch.uint8:
        raise TypeError("cfhip attention: mask must be bool or uint8")
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    mask = mask.expand(b, h, tq, tk)
    if mask.stride(3) != 1:
        mask = mask.contiguous()
    return mask, mask.data_ptr(), mask.stride(0), mask.stride(1), mask.stride(2)


def attn_fwd(
    q: Tensor, k: Tensor, v: Tensor, num_heads: int, *, mask: Optional[Tensor] = None,
    causal: bool = False, scale: Optional[float] = None, head_dim: int = 64, dropout_p: float = 0.0,
    seed: int = 0, offset: int = 0, out: Optional[Tensor] = None, lse: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor]:
    """Returns (o bf16 [B, Tq, H*head_dim] contiguous, lse f32 [B, H, Tq]).  head_dim 64 with both lengths <= 256
    takes the LDS-resident kernels; anything else (head_dim any multiple of 8 up to 192) the chunked general ones.
    `dropout_p` > 0: dropout on the attention probabilities, mask = f(seed, offset) (see `attn_dropout_blocks`)."""
    b, tq, d, q_sb, q_st = _bth(q, "q")
    _, tk, _, k_sb, k_st = _bth(k, "k")
    _, _, _, v_sb, v_st = _bth(v, "v")
    if d != num_heads * head_dim or head_dim % 8 or not 8 <= head_dim <= 192:
        raise ValueError(f"cfhip attention: embed {d} != heads {num_heads} x head_dim {head_dim} "
                         "(head_dim: a multiple of 8 in [8, 192])")
    if (k_sb, k_st) != (v_sb, v_st):
        raise ValueError("cfhip attention: k and v must share batch / token strides")
    if scale is None:
        scale = 1.0 / math.sqrt(float(head_dim))
    o = torch.empty((b, tq, d), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((b, num_heads, tq), dtype=f32, device=q.device) if lse is None else lse
    keep, mp, ms_b, ms_h, ms_q = _mask_args(mask, b, num_heads, tq, tk)
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["attention"] += 4.0 * b * num_heads * tq * tk * head_dim
    if dropout_p > 0.0:
        rc = _lib.load().cfhip_attn_fwd_dropout(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, b, num_heads, tq,
            tk, int(head_dim), q_sb, q_st, k_sb, k_st, o.stride(0), o.stride(1), ms_b, ms_h, ms_q, float(scale),
            int(causal), float(dropout_p), int(seed), int(offset), _stream(),
        )
    else:
        rc = _lib.load().cfhip_attn_fwd_dh(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, b, num_heads, tq,
            tk, int(head_dim), q_sb, q_st, k_sb, k_st, o.stride(0), o.stride(1), ms_b, ms_h, ms_q, float(scale),
            int(causal), _stream(),
        )
    _lib.check(rc, "attn_fwd")
    return o, lse


def attn_wide_fwd(q: Tensor, k: Tensor, v: Tensor, num_heads: int = 1, *, head_dim: int, scale: Optional[float] = None,
                  out: Optional[Tensor] = None, want_lse: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """Forward-only attention for heads wider than `attn_fwd` takes: 192 < head_dim <= 512, a multiple of 8 (cfhip_attn_wide_fwd,
    csrc/attn_wide.hip).  Operands as `attn_fwd` ([B, T, H*head_dim] bf16 with batch / token strides: a packed projection is
    read in place); no mask, not causal, no dropout.  Returns (o bf16 [B, Tq, H*head_dim], lse f32 [B, H, Tq] or None)."""
    b, tq, d, q_sb, q_st = _bth(q, "q")
    _, tk, _, k_sb, k_st = _bth(k, "k")
    _, _, _, v_sb, v_st = _bth(v, "v")
    wide_max = _lib.DEFINES["CFHIP_ATTN_WIDE_MAX_HEAD_DIM"]
    if d != num_heads * head_dim or head_dim % 8 or not 192 < head_dim <= wide_max:
        raise ValueError(f"cfhip wide attention: embed {d} != heads {num_heads} x head_dim {head_dim} "
                         f"(head_dim: a multiple of 8 in (192, {wide_max}])")
    if (k_sb, k_st) != (v_sb, v_st):
        raise ValueError("cfhip wide attention: k and v must share batch / token strides")
    if scale is None:
        scale = 1.0 / math.sqrt(float(head_dim))
    o = torch.empty((b, tq, d), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((b, num_heads, tq), dtype=f32, device=q.device) if want_lse else None
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["attention"] += 4.0 * b * num_heads * tq * tk * head_dim
    rc = _lib.load().cfhip_attn_wide_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse), b, num_heads, tq, tk,
                                         int(head_dim), q_sb, q_st, k_sb, k_st, o.stride(0), o.stride(1), float(scale), _stream())
    _lib.check(rc, "attn_wide_fwd")
    return o, lse


def attn_plan(tq: int, tk: int, *, backward: bool = False, mask: object = None, causal: bool = False, head_dim: int = 64,
              dropout_p: float = 0.0, parts: int = 3, lse: bool = True) -> List[str]:
    """The kernel instantiations `attn_fwd` (or, with `backward`, one `attn_bwd` call of these `parts`) launches for these
    lengths under the current options, in launch order and spelled as tools/attn_kernel_census.py prints them
    (cfhip_attn_plan: a host-side query, no device needed).  `mask`: a mask tensor, or True / False for whether one is
    given; `lse`: the forward is handed an lse buffer (`attn_fwd` always does)."""
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().cfhip_attn_plan(int(backward), int(head_dim), int(tq), int(tk), int(mask is not None and mask is not False),
                                     int(causal), int(dropout_p > 0.0), int(parts), int(bool(lse)), buf, 128)
    _lib.check(rc, "attn_plan")
    return buf.value.decode().split("\n")


def attn_probs(q: Tensor, k: Tensor, lse: Tensor, num_heads: int, *, mask: Optional[Tensor] = None, causal: bool = False,
               scale: Optional[float] = None, head_dim: int = 64) -> Tensor:
    """f32 [B, H, Tq, Tk]: the attention weights behind `attn_fwd`'s output, exp(scale q.k - lse) with masked slots 0
    (cfhip_attn_probs: the reference's `require_weights` path, attentions.py:256-268)."""
    b, tq, d, q_sb, q_st = _bth(q, "q")
    _, tk, _, k_sb, k_st = _bth(k, "k")
    _need(lse, f32, "lse")
    if scale is None:
        scale = 1.0 / math.sqrt(float(head_dim))
    out = torch.empty((b, num_heads, tq, tk), dtype=f32, device=q.device)
    keep, mp, ms_b, ms_h, ms_q = _mask_args(mask, b, num_heads, tq, tk)
    rc = _lib.load().cfhip_attn_probs(q.data_ptr(), k.data_ptr(), lse.data_ptr(), mp, out.data_ptr(), b, num_heads, tq, tk,
                                      int(head_dim), q_sb, q_st, k_sb, k_st, ms_b, ms_h, ms_q, float(scale), int(causal), _stream())
    _lib.check(rc, "attn_probs")
    return out


def attn_probs_bwd(q: Tensor, k: Tensor, lse: Tensor, d_probs: Tensor, num_heads: int, *, mask: Optional[Tensor] = None,
                   causal: bool = False, scale: Optional[float] = None, head_dim: int = 64) -> Tuple[Tensor, Tensor]:
    """(dq, dk) bf16 [B, T, H*head_dim]: what a gradient on the returned weights adds to the input gradients"""
    b, tq, d, q_sb, q_st = _bth(q, "q")
    _, tk, _, k_sb, k_st = _bth(k, "k")
    _need(lse, f32, "lse")
    _need(d_probs, f32, "d_probs")
    if tuple(d_probs.shape) != (b, num_heads, tq, tk) or not d_probs.is_contiguous():
        raise ValueError("cfhip attn_probs_bwd: d_probs must be a contiguous f32 [B, H, Tq, Tk]")
    if scale is None:
        scale = 1.0 / math.sqrt(float(head_dim))
    ws = torch.empty_like(d_probs)
    dq = torch.empty((b, tq, d), dtype=bf16, device=q.device)
    dk = torch.empty((b, tk, d), dtype=bf16, device=q.device)
    keep, mp, ms_b, ms_h, ms_q = _mask_args(mask, b, num_heads, tq, tk)
    rc = _lib.load().cfhip_attn_probs_bwd(q.data_ptr(), k.data_ptr(), lse.data_ptr(), mp, d_probs.data_ptr(), ws.data_ptr(),
                                          dq.data_ptr(), dk.data_ptr(), b, num_heads, tq, tk, int(head_dim), q_sb, q_st, k_sb, k_st,
                                          ms_b, ms_h, ms_q, float(scale), int(causal), _stream())
    _lib.check(rc, "attn_probs_bwd")
    return dq, dk


def attn_dropout_blocks(b: int, num_heads: int, tq: int, tk: int) -> int:
    """Philox counters one attention call with dropout consumes (`PhiloxState.take` this many)"""
    return b * num_heads * ((tq + 3) // 4) * ((tk + 3) // 4)


def attn_dropout_p(dropout_p: float) -> float:
    """the probability the kernels apply: p quantised to 1 / 256 (csrc/attn.hip set_dropout: thresh = lrintf(256 p), clamped to 1 .. 255)"""
    return min(max(int(round(float(dropout_p) * 256.0)), 1), 255) / 256.0


def attn_dropout_mask(b: int, num_heads: int, tq: int, tk: int, dropout_p: float, seed: int, offset: int,
                      device: object = "cuda") -> Tensor:
    """uint8 [B, H, Tq, Tk] (1 = keep): the mask `attn_fwd(..., dropout_p, seed, offset)` applies"""
    out = torch.empty((b, num_heads, tq, tk), dtype=torch.uint8, device=device)
    rc = _lib.load().cfhip_attn_dropout_mask(out.data_ptr(), b, num_heads, tq, tk, float(dropout_p), int(seed),
                                             int(offset), _stream())
    _lib.check(rc, "attn_dropout_mask")
    return out


def attn_bwd(
    q: Tensor, k: Tensor, v: Tensor, o: Tensor, d_o: Tensor, lse: Tensor, num_heads: int, *,
    dq: Tensor, dk: Tensor, dv: Tensor, mask: Optional[Tensor] = None, causal: bool = False,
    scale: Optional[float] = None, parts: int = 3, delta: Optional[Tensor] = None, head_dim: int = 64,
    dropout_p: float = 0.0, seed: int = 0, offset: int = 0,
) -> None:
    """Writes dq / dk / dv (bf16, SAME strides as q / k / v — e.g. views of one packed buffer)."""
    b, tq, d, q_sb, q_st = _bth(q, "q")
    _, tk, _, k_sb, k_st = _bth(k, "k")
    _bth(v, "v")
    _, _, _, o_sb, o_st = _bth(o, "o")
    _, _, _, do_sb, do_st = _bth(d_o, "d_o")
    if (o_sb, o_st) != (do_sb, do_st):
        raise ValueError("cfhip attention: o and d_o must share strides")
    for t, ref, nm in ((dq, q, "dq"), (dk, k, "dk"), (dv, v, "dv")):
        _need(t, bf16, nm)
        if t.shape != ref.shape or t.stride() != ref.stride():
            raise ValueError(f"cfhip attention: `{nm}` must have the shape and strides of its primal")
    if scale is None:
        scale = 1.0 / math.sqrt(float(head_dim))
    if delta is None:
        delta = torch.empty((b, num_heads, tq), dtype=f32, device=q.device)
    keep, mp, ms_b, ms_h, ms_q = _mask_args(mask, b, num_heads, tq, tk)
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["attention"] += 10.0 * b * num_heads * tq * tk * head_dim
    if dropout_p > 0.0:
        rc = _lib.load().cfhip_attn_bwd_dropout(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(),
            delta.data_ptr(), mp, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), b, num_heads, tq, tk, int(head_dim),
            q_sb, q_st, k_sb, k_st, o_sb, o_st, ms_b, ms_h, ms_q, float(scale), int(causal), int(parts),
            float(dropout_p), int(seed), int(offset), _stream(),
        )
    else:
        rc = _lib.load().cfhip_attn_bwd_dh(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(),
            delta.data_ptr(), mp, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), b, num_heads, tq, tk, int(head_dim),
            q_sb, q_st, k_sb, k_st, o_sb, o_st, ms_b, ms_h, ms_q, float(scale), int(causal), int(parts), _stream(),
        )
    _lib.check(rc, "attn_bwd")


# ---------------------------------------------------------------------------------------------
# head-only tail of a pre-norm block (csrc/head_tail.hip, `gemm(..., config_rows=)`; the caller is fused._block_fwd / _block_bwd)
# ---------------------------------------------------------------------------------------------


def _rows16(t: Tensor, name: str) -> None:
    if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16:
        raise ValueError(f"cfhip head tail: `{name}` must be a 2-D device tensor of 16-byte aligned rows")


def head_rows_zero(x: Tensor, cols: int) -> None:
    """the first `cols` columns of every row of `x` := 0 (cfhip_head_rows_zero)"""
    _rows16(x, "x")
    rc = _lib.load().cfhip_head_rows_zero(x.data_ptr(), x.shape[0], cols, x.stride(0), x.element_size(), _stream())
    _lib.check(rc, "head_rows_zero")


# ---------------------------------------------------------------------------------------------
# ViT glue
# ---------------------------------------------------------------------------------------------


def im2row(img: Tensor, patch: int) -> Tensor:
    """img [B, C, H, W] (f32 or bf16, contiguous) -> bf16 [B*gh*gw, C*P*P] in (c, ph, pw) order."""
    if img.dtype not in (f32, bf16) or not img.is_cuda or not img.is_contiguous() or img.dim() != 4:
        raise ValueError("cfhip im2row: img must be a contiguous f32/bf16 [B, C, H, W] device tensor")
    b, c, hh, ww = img.shape
    rows = torch.empty((b * (hh // patch) * (ww // patch), c * patch * patch), dtype=bf16, device=img.device)
    rc = _lib.load().cfhip_im2row(img.data_ptr(), int(img.dtype == bf16), rows.data_ptr(), b, c, hh, ww,
                                  patch, _stream())
    _lib.check(rc, "im2row")
    return rows


def assemble_tokens_fwd(patches: Tensor, head_token: Tensor, pos: Tensor, b: int,
                        out_dtype: torch.dtype = f32) -> Tensor:
    """patches bf16 [B*Np, D]; head_token f32 [D]; pos f32 [(Np+1)*D] -> x0 [B, Np+1, D] (f32 residual
    stream by default: head_token / pos are f32 parameters, the reference's sum type-promotes)."""
    _need(patches, bf16, "patches")
    _need(head_token, f32, "head_token")
    _need(pos, f32, "pos")
    d = patches.shape[-1]
    np_ = patches.numel() // (b * d)
    x0 = torch.empty((b, np_ + 1, d), dtype=out_dtype, device=patches.device)
    rc = _lib.load().cfhip_assemble_tokens_fwd(patches.data_ptr(), head_token.data_ptr(), pos.data_ptr(),
                                               x0.data_ptr(), int(out_dtype == f32), b, np_, d, _stream())
    _lib.check(rc, "assemble_tokens_fwd")
    return x0


def assemble_tokens_bwd(
    dx0: Tensor, dhead: Optional[Tensor], dpos: Optional[Tensor], accumulate: bool,
    want_dpatches: bool = True,
) -> Optional[Tensor]:
    """dx0 bf16 [B, Np+1, D] contiguous -> dpatches bf16 [B*Np, D]; dhead / dpos f32 (+)=."""
    _need(dx0, bf16, "dx0")
    if not dx0.is_contiguous():
        raise ValueError("cfhip assemble_tokens_bwd: dx0 must be contiguous")
    b, t, d = dx0.shape
    dpatches = torch.empty((b * (t - 1), d), dtype=bf16, device=dx0.device) if want_dpatches else None
    rc = _lib.load().cfhip_assemble_tokens_bwd(dx0.data_ptr(), _p(dpatches), _p(dhead), _p(dpos), b, t - 1,
                                               d, int(accumulate), _stream())
    _lib.check(rc, "assemble_tokens_bwd")
    return dpatches


# ---------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------


def to_bf16(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """f32 -> bf16 (round-to-nearest-even) through the HIP cast kernel; bf16 passes through."""
    if x.dtype == bf16 and out is None:
        return x
    _need(x, f32, "x")
    if not x.is_contiguous():
        x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    _lib.check(rc, "cast_f32_to_bf16")
    return out


def to_f32(x: Tensor) -> Tensor:
    if x.dtype == f32:
        return x
    _need(x, bf16, "x")
    if not x.is_contiguous():
        x = x.contiguous()
    out = torch.empty(x.shape, dtype=f32, device=x.device)
    rc = _lib.load().cfhip_cast_bf16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    _lib.check(rc, "cast_bf16_to_f32")
    return out


def _ew(fn_name: str, *tensors: Tensor) -> Tensor:
    for i, t in enumerate(tensors):
        _need(t, bf16, f"arg{i}")
        if not t.is_contiguous():
            raise ValueError(f"cfhip {fn_name}: tensors must be contiguous")
    out = torch.empty_like(tensors[0])
    fn = getattr(_lib.load(), fn_name)
    rc = fn(*[t.data_ptr() for t in tensors], out.data_ptr(), out.numel(), _stream())
    _lib.check(rc, fn_name)
    return out


def gelu_fwd(x: Tensor) -> Tensor:
    return _ew("cfhip_gelu_fwd", x)


def gelu_bwd(dy: Tensor, x: Tensor) -> Tensor:
    return _ew("cfhip_gelu_bwd", dy, x)


def quick_gelu_fwd(x: Tensor) -> Tensor:
    return _ew("cfhip_quick_gelu_fwd", x)


def quick_gelu_bwd(dy: Tensor, x: Tensor) -> Tensor:
    return _ew("cfhip_quick_gelu_bwd", dy, x)


def add(a: Tensor, b: Tensor) -> Tensor:
    return _ew("cfhip_add_bf16", a, b)


def transpose(x: Tensor) -> Tensor:
    _need(x, bf16, "x")
    r, c, ld = _mat(x, "x")
    out = torch.empty((c, r), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_transpose_bf16(x.data_ptr(), out.data_ptr(), r, c, ld, out.stride(0), _stream())
    _lib.check(rc, "transpose")
    return out


# ---------------------------------------------------------------------------------------------
# optimiser / loss
# ---------------------------------------------------------------------------------------------


def adam_step(
    p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Optional[Tensor], *, lr: float, beta1: float,
    beta2: float, eps: float, weight_decay: float, decoupled: bool, step: int, grad_scale: float = 1.0,
) -> None:
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _need(t, f32, nm)
        if not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError("cfhip adam_step: flat contiguous f32 buffers of equal length expected")
    if p_bf16 is not None:
        _need(p_bf16, bf16, "p_bf16")
    rc = _lib.load().cfhip_adam_step(
        p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(p_bf16), p.numel(), float(lr),
        float(beta1), float(beta2), float(eps), float(weight_decay), int(decoupled), int(step),
        float(grad_scale), _stream(),
    )
    _lib.check(rc, "adam_step")


def sumsq(g: Tensor) -> Tensor:
    _need(g, f32, "g")
    out = torch.zeros((1,), dtype=f32, device=g.device)
    rc = _lib.load().cfhip_sumsq_f32(g.data_ptr(), out.data_ptr(), g.numel(), _stream())
    _lib.check(rc, "sumsq")
    return out


def softmax_xent(logits: Tensor, labels: Tensor, grad_scale: float, want_grad: bool = True):
    """Returns (loss_sum f32 [1], dlogits f32 [B, C] = (softmax - onehot) * grad_scale)."""
    _need(logits, f32, "logits")
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise TypeError("cfhip softmax_xent: labels must be int64 on the device")
    if not logits.is_contiguous():
        logits = logits.contiguous()
    labels = labels.reshape(-1).contiguous()
    b, c = logits.shape
    loss = torch.zeros((1,), dtype=f32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    rc = _lib.load().cfhip_softmax_xent(logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), _p(dlogits),
                                        b, c, float(grad_scale), _stream())
    _lib.check(rc, "softmax_xent")
    return loss, dlogits


def softmax_focal(logits: Tensor, labels: Tensor, grad_scale: float, *, gamma: float = 2.0, eps: float = 1.0e-6,
                  want_grad: bool = True):
    """Focal loss of reference losses/basic.py:170-206: returns (loss_sum f32 [1], dlogits f32 [B, C])."""
    _need(logits, f32, "logits")
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise TypeError("cfhip softmax_focal: labels must be int64 on the device")
    if not logits.is_contiguous():
        logits = logits.contiguous()
    labels = labels.reshape(-1).contiguous()
    b, c = logits.shape
    loss = torch.zeros((1,), dtype=f32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    rc = _lib.load().cfhip_softmax_focal(logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), _p(dlogits),
                                         b, c, float(gamma), float(eps), float(grad_scale), _stream())
    _lib.check(rc, "softmax_focal")
    return loss, dlogits


# ---------------------------------------------------------------------------------------------
# conv / batch-norm family (K8 general form, K9, K10)
# ---------------------------------------------------------------------------------------------


def conv_out_hw(h: int, w: int, kh: int, kw: int, stride: int, pad: int, dil: int) -> Tuple[int, int]:
    return ((h + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1)


def conv_out_hw_pad(h: int, w: int, kh: int, kw: int, stride: int, pad: int, pad_hi: int, dil: int) -> Tuple[int, int]:
    """the same with `pad` zero rows / columns before the image and `pad_hi` after it"""
    return ((h + pad + pad_hi - dil * (kh - 1) - 1) // stride + 1, (w + pad + pad_hi - dil * (kw - 1) - 1) // stride + 1)


def conv_im2row(x: Tensor, kh: int, kw: int, stride: int, pad: int, dil: int = 1, pad_hi: Optional[int] = None) -> Tensor:
    """x [B, C, H, W] (f32 / bf16, contiguous) -> rows bf16 [B*Ho*Wo, Kp], k = (c, ky, kx), Kp = K rounded up to 8.
    `pad_hi`: the zero padding after the image (bottom / right) where it differs from `pad` (top / left): cfhip_conv_im2row_pad."""
    if x.dtype not in (f32, bf16) or not x.is_cuda or not x.is_contiguous() or x.dim() != 4:
        raise ValueError("cfhip conv_im2row: x must be a contiguous f32/bf16 [B, C, H, W] device tensor")
    b, c, h, w = x.shape
    kp = (c * kh * kw + 7) // 8 * 8
    if pad_hi is None:
        ho, wo = conv_out_hw(h, w, kh, kw, stride, pad, dil)
        rows = torch.empty((b * ho * wo, kp), dtype=bf16, device=x.device)
        rc = _lib.load().cfhip_conv_im2row(x.data_ptr(), int(x.dtype == f32), rows.data_ptr(), b, c, h, w, kh, kw,
                                           stride, pad, dil, kp, _stream())
    else:
        ho, wo = conv_out_hw_pad(h, w, kh, kw, stride, pad, pad_hi, dil)
        rows = torch.empty((b * max(ho, 0) * max(wo, 0), kp), dtype=bf16, device=x.device)
        rc = _lib.load().cfhip_conv_im2row_pad(x.data_ptr(), int(x.dtype == f32), rows.data_ptr(), b, c, h, w, kh, kw,
                                               stride, pad, pad_hi, pad, pad_hi, dil, kp, _stream())
    _lib.check(rc, "conv_im2row")
    return rows


def conv_row2im(drows: Tensor, shape: Tuple[int, int, int, int], kh: int, kw: int, stride: int, pad: int,
                dil: int = 1, pad_hi: Optional[int] = None) -> Tensor:
    """drows bf16 [B*Ho*Wo, Kp] -> dx bf16 [B, C, H, W] (gather-sum of the overlapping windows); `pad_hi` as `conv_im2row`."""
    _need(drows, bf16, "drows")
    if not drows.is_contiguous():
        drows = drows.contiguous()
    b, c, h, w = shape
    dx = torch.empty(shape, dtype=bf16, device=drows.device)
    if pad_hi is None:
        rc = _lib.load().cfhip_conv_row2im(drows.data_ptr(), dx.data_ptr(), b, c, h, w, kh, kw, stride, pad, dil,
                                           drows.shape[1], _stream())
    else:
        ho, wo = conv_out_hw_pad(h, w, kh, kw, stride, pad, pad_hi, dil)
        if drows.shape[0] != b * ho * wo:
            raise ValueError(f"cfhip conv_row2im: {drows.shape[0]} rows given, the geometry has {b} x {ho} x {wo}")
        rc = _lib.load().cfhip_conv_row2im_pad(drows.data_ptr(), dx.data_ptr(), b, c, h, w, kh, kw, stride, pad, pad_hi, pad,
                                               pad_hi, dil, drows.shape[1], _stream())
    _lib.check(rc, "conv_row2im")
    return dx


def transpose_batched(x: Tensor) -> Tensor:
    """x [batch, R, C] (f32 / bf16, contiguous) -> bf16 [batch, C, R]."""
    if x.dtype not in (f32, bf16) or not x.is_cuda or not x.is_contiguous() or x.dim() != 3:
        raise ValueError("cfhip transpose_batched: x must be a contiguous f32/bf16 [batch, R, C] device tensor")
    n, r, c = x.shape
    out = torch.empty((n, c, r), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_transpose_batched(x.data_ptr(), int(x.dtype == f32), out.data_ptr(), n, r, c, _stream())
    _lib.check(rc, "transpose_batched")
    return out


def batchnorm_fwd(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], running_mean: Optional[Tensor],
                  running_var: Optional[Tensor], eps: float, momentum: float, training: bool):
    """x [B, C, *] (f32 / bf16, contiguous) -> (y bf16, mean f32 [C], rstd f32 [C]); running stats updated in place."""
    if x.dtype not in (f32, bf16) or not x.is_cuda or not x.is_contiguous() or x.dim() < 2:
        raise ValueError("cfhip batchnorm_fwd: x must be a contiguous f32/bf16 [B, C, ...] device tensor")
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _need(t, f32, nm)
    y = torch.empty(x.shape, dtype=bf16, device=x.device)
    mean = torch.empty((c,), dtype=f32, device=x.device)
    rstd = torch.empty((c,), dtype=f32, device=x.device)
    rc = _lib.load().cfhip_batchnorm_fwd(x.data_ptr(), int(x.dtype == f32), _p(gamma), _p(beta), y.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), _p(running_mean), _p(running_var), b, c,
                                         inner, float(eps), float(momentum), int(training), _stream())
    _lib.check(rc, "batchnorm_fwd")
    return y, mean, rstd


def batchnorm_bwd(dy: Tensor, x: Tensor, gamma: Optional[Tensor], mean: Tensor, rstd: Tensor, *, training: bool,
                  want_dx: bool = True, dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None,
                  accumulate: bool = False):
    """Returns (dx bf16 | None, dgamma f32 [C], dbeta f32 [C])."""
    _need(dy, bf16, "dy")
    if not dy.is_contiguous():
        dy = dy.contiguous()
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    dx = torch.empty(x.shape, dtype=bf16, device=x.device) if want_dx else None
    if dgamma is None:
        dgamma, accumulate = torch.empty((c,), dtype=f32, device=x.device), False
        dbeta = torch.empty((c,), dtype=f32, device=x.device)
    rc = _lib.load().cfhip_batchnorm_bwd(dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), _p(gamma), mean.data_ptr(),
                                         rstd.data_ptr(), _p(dx), dgamma.data_ptr(), dbeta.data_ptr(), b, c, inner,
                                         int(accumulate), int(training), _stream())
    _lib.check(rc, "batchnorm_bwd")
    return dx, dgamma, dbeta


def leaky_relu_fwd(x: Tensor, slope: float) -> Tensor:
    _need(x, bf16, "x")
    if not x.is_contiguous():
        x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_leaky_relu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), float(slope), _stream()),
               "leaky_relu_fwd")
    return y


def leaky_relu_bwd(dy: Tensor, x: Tensor, slope: float) -> Tensor:
    _need(dy, bf16, "dy")
    _need(x, bf16, "x")
    if not dy.is_contiguous():
        dy = dy.contiguous()
    dx = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_leaky_relu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), float(slope),
                                                _stream()), "leaky_relu_bwd")
    return dx


def avgpool_fwd(x: Tensor) -> Tensor:
    """x bf16 [B, C, H, W] -> bf16 [B, C] (AdaptiveAvgPool2d((1, 1)) + squeeze)."""
    _need(x, bf16, "x")
    if not x.is_contiguous():
        x = x.contiguous()
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    y = torch.empty((b, c), dtype=bf16, device=x.device)
    _lib.check(_lib.load().cfhip_avgpool_fwd(x.data_ptr(), y.data_ptr(), b * c, inner, _stream()), "avgpool_fwd")
    return y


def avgpool_bwd(dy: Tensor, shape: Tuple[int, ...]) -> Tensor:
    _need(dy, bf16, "dy")
    if not dy.is_contiguous():
        dy = dy.contiguous()
    b, c = shape[0], shape[1]
    dx = torch.empty(shape, dtype=bf16, device=dy.device)
    inner = dx.numel() // (b * c)
    _lib.check(_lib.load().cfhip_avgpool_bwd(dy.data_ptr(), dx.data_ptr(), b * c, inner, _stream()), "avgpool_bwd")
    return dx


# ---------------------------------------------------------------------------------------------
# row gather / scatter-add, L2 normalisation (CLIP text tower)
# ---------------------------------------------------------------------------------------------


def embedding_fwd(table: Tensor, indices: Tensor, pos: Optional[Tensor] = None, *, period: int = 0,
                  out_dtype: torch.dtype = f32) -> Tensor:
    """out[n] = table[indices[n]] (+ pos[n % period]); table f32 [V, D], indices int64 [...], pos f32 [>= period, D]."""
    _need(table, f32, "table")
    if indices.dtype != torch.int64 or not indices.is_cuda:
        raise TypeError("cfhip embedding_fwd: indices must be int64 on the device")
    if table.dim() != 2 or not table.is_contiguous():
        raise ValueError("cfhip embedding_fwd: table must be a contiguous [V, D] matrix")
    idx = indices.reshape(-1).contiguous()
    v, d = table.shape
    if pos is not None:
        _need(pos, f32, "pos")
        if not pos.is_contiguous() or pos.shape[-1] != d or pos.numel() < period * d:
            raise ValueError("cfhip embedding_fwd: pos must be contiguous [>= period, D]")
    out = torch.empty((idx.numel(), d), dtype=out_dtype, device=table.device)
    rc = _lib.load().cfhip_embedding_fwd(table.data_ptr(), idx.data_ptr(), _p(pos), out.data_ptr(),
                                         int(out_dtype == f32), idx.numel(), d, int(period), v, _stream())
    _lib.check(rc, "embedding_fwd")
    return out.view(*indices.shape, d)


def embedding_bwd(dy: Tensor, indices: Tensor, dtable: Tensor, padding_idx: int = -1) -> None:
    """dtable[indices[n]] += dy[n] (dtable f32 [V, D], owned / zeroed by the caller)."""
    _need(dtable, f32, "dtable")
    if dy.dtype not in (f32, bf16) or not dy.is_cuda:
        raise TypeError("cfhip embedding_bwd: dy must be f32 / bf16 on the device")
    v, d = dtable.shape
    dy2 = dy.reshape(-1, d).contiguous()
    idx = indices.reshape(-1).contiguous()
    rc = _lib.load().cfhip_embedding_bwd(dy2.data_ptr(), int(dy2.dtype == f32), idx.data_ptr(), dtable.data_ptr(),
                                         idx.numel(), d, v, int(padding_idx), _stream())
    _lib.check(rc, "embedding_bwd")


def l2norm_fwd(x: Tensor) -> Tuple[Tensor, Tensor]:
    _need(x, f32, "x")
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    y = torch.empty_like(x2)
    inv = torch.empty((x2.shape[0],), dtype=f32, device=x.device)
    _lib.check(_lib.load().cfhip_l2norm_fwd(x2.data_ptr(), y.data_ptr(), inv.data_ptr(), x2.shape[0], x2.shape[1],
                                            _stream()), "l2norm_fwd")
    return y.view(x.shape), inv


def l2norm_bwd(dy: Tensor, y: Tensor, inv: Tensor) -> Tensor:
    _need(dy, f32, "dy")
    dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
    y2 = y.reshape(-1, y.shape[-1]).contiguous()
    dx = torch.empty_like(dy2)
    _lib.check(_lib.load().cfhip_l2norm_bwd(dy2.data_ptr(), y2.data_ptr(), inv.data_ptr(), dx.data_ptr(), dy2.shape[0],
                                            dy2.shape[1], _stream()), "l2norm_bwd")
    return dx.view(dy.shape)


# ---------------------------------------------------------------------------------------------
# UNet residual-block pieces: GroupNorm (+ additive term, + SiLU), SiLU, x2 resampling, timestep embedding
# ---------------------------------------------------------------------------------------------


def colreduce_f32(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[d] (+)= sum_r x[r][d] for a contiguous f32 [R, D] matrix."""
    _need(x, f32, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError("cfhip colreduce_f32: contiguous [R, D] matrix expected")
    if out is None:
        out, accumulate = torch.empty((x.shape[1],), dtype=f32, device=x.device), False
    _lib.check(_lib.load().cfhip_colreduce_f32(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], int(accumulate),
                                               _stream()), "colreduce_f32")
    return out


def colreduce2_f32(xa: Tensor, xb: Tensor, out_a: Tensor, out_b: Tensor, accumulate: bool) -> None:
    """out_a[d] (+)= sum_r xa[r][d] and the same for (xb, out_b) — two contiguous f32 [R, D] matrices of one shape — in one launch"""
    _need(xa, f32, "xa")
    _need(xb, f32, "xb")
    if xa.dim() != 2 or xa.shape != xb.shape or not xa.is_contiguous() or not xb.is_contiguous():
        raise ValueError("cfhip colreduce2_f32: two contiguous [R, D] matrices of one shape expected")
    _lib.check(_lib.load().cfhip_colreduce2_f32(xa.data_ptr(), out_a.data_ptr(), xb.data_ptr(), out_b.data_ptr(), xa.shape[0], xa.shape[1],
                                                int(accumulate), _stream()), "colreduce2_f32")


def _gn_affine_stride(gamma: Tensor, beta: Tensor, b: int, c: int) -> int:
    if gamma.shape != beta.shape or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError("cfhip groupnorm: gamma / beta must be contiguous and of one shape")
    if tuple(gamma.shape) == (c,):
        return 0
    if tuple(gamma.shape) == (b, c):
        return c
    raise ValueError(f"cfhip groupnorm: gamma must be [C] or [B, C], got {tuple(gamma.shape)}")


GN_TARGET_WORKGROUPS = 1024  # four 4-wave workgroups per CU; 0: never split
GN_MIN_SLICE = 2048  # elements of `inner` per slice and channel below which splitting stops paying


def gn_splits(b: int, c: int, groups: int, inner: int) -> int:
    """Slices per (sample, group) of the split GroupNorm kernels: enough workgroups to fill the chip when B * G alone does
    not (batch 1 at 256^2: 32 workgroups on 256 CUs), never slices shorter than GN_MIN_SLICE elements per channel."""
    if GN_TARGET_WORKGROUPS <= 0 or inner % 8 != 0:
        return 1
    want = -(-GN_TARGET_WORKGROUPS // (b * groups))
    return max(1, min(64, want, inner // GN_MIN_SLICE))


GN_NHWC_TARGET_WORKGROUPS = 1024
GN_NHWC_MIN_ROWS = 16


GN_NHWC_GROUP_MAX_ROWS = 48  # rows per thread up to which the group form is used
GN_NHWC_GROUP_MIN_WORKGROUPS = 128  # B * G from which one workgroup per (sample, group) fills the chip


def gn_nhwc_splits(b: int, inner: int, c: int = 0, groups: int = 0, backward: bool = False) -> int:
    """0: the group form (one workgroup per (sample, group), ONE launch each way: enough samples, an even number of channels per group);
    otherwise the row slices per sample of the slice form (few samples, e.g. 256^2 x 1): ~4 workgroups per CU, >= GN_NHWC_MIN_ROWS rows each"""
    if groups and c % groups == 0:
        cpg = c // groups
        if b * groups >= GN_NHWC_GROUP_MIN_WORKGROUPS and cpg % 2 == 0 and cpg <= 256:
            # a thread of the group form owns ceil(inner / row lanes) rows as 2 cpg-byte chunks (20-60 bytes of every 640-3 840-byte
            # row on the UNet's upper levels): fine while there are few, but with many rows per thread the slice form's whole-row
            # 16-byte accesses win although it is three launches — alone only beyond the 88 rows the group form can keep in
            # registers (64^2 x 8 x 960: 281 / 246 us forward / backward against 94 / 126, `tools/gn_nhwc_bench.py`), inside the
            # step, beside the weight-gradient GEMMs of the other queue, already from ~50 (64^2 x 8 step: threshold none / 88 / 48 /
            # 32 / 16 / 0 = 59.3 / 58.8 / 58.3 / +0.4 / +1.4 / +3.0 ms, `profiles/r05/gn_nhwc_form_rule_ab.txt`)
            d = cpg // 2  # dwords per row chunk; a thread reads 4 / 2 / 1 of them with one access (groupnorm.hip: gn_group_vw)
            vw = 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1
            row_lanes = 256 // (d // vw)
            if -(-inner // row_lanes) <= GN_NHWC_GROUP_MAX_ROWS:
                return 0
            # (forward: 32 slices — its statistics kernel reads the slice twice, the second time out of L2; backward: 64)
            return max(1, min(64 if backward else 32, inner // 32))
    want = -(-GN_NHWC_TARGET_WORKGROUPS // b)
    return max(1, min(want, inner // GN_NHWC_MIN_ROWS, 4096))


def groupnorm_nhwc_fwd(rows: Tensor, b: int, gamma: Tensor, beta: Tensor, groups: int, eps: float, *, add: Optional[Tensor] = None,
                       silu: bool = False):
    """rows bf16 [B * inner, C] (NHWC) -> (y rows bf16, mean f32 [B * G], rstd f32 [B * G]); y = [SiLU](GN(x + add[b, c])).
    gamma / beta: f32 [C], or [B, C] = one affine per sample."""
    _need(rows, bf16, "rows")
    _need(gamma, f32, "gamma")
    _need(beta, f32, "beta")
    if rows.dim() != 2 or not rows.is_contiguous() or rows.shape[0] % b:
        raise ValueError("cfhip groupnorm_nhwc_fwd: contiguous bf16 [B * inner, C] rows expected")
    c = rows.shape[1]
    inner = rows.shape[0] // b
    affine_bs = _gn_affine_stride(gamma, beta, b, c)
    if add is not None:
        _need(add, f32, "add")
        if tuple(add.shape) != (b, c) or not add.is_contiguous():
            raise ValueError("cfhip groupnorm_nhwc_fwd: add must be contiguous f32 [B, C]")
    lib = _lib.load()
    splits = gn_nhwc_splits(b, inner, c, groups)
    y = torch.empty_like(rows)
    mean = torch.empty((b * groups,), dtype=f32, device=rows.device)
    rstd = torch.empty((b * groups,), dtype=f32, device=rows.device)
    ws = None if splits == 0 else torch.empty((max(4, lib.cfhip_groupnorm_nhwc_workspace(b, c, groups, splits, 0, 0)) // 4,), dtype=f32,
                                              device=rows.device)
    rc = lib.cfhip_groupnorm_nhwc_fwd(rows.data_ptr(), _p(add), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), b, c, groups, inner, float(eps), int(silu), affine_bs, splits, _p(ws), _stream())
    _lib.check(rc, "groupnorm_nhwc_fwd")
    return y, mean, rstd


def groupnorm_nhwc_bwd(dy: Tensor, rows: Tensor, b: int, gamma: Tensor, beta: Tensor, mean: Tensor, rstd: Tensor, groups: int, *,
                       add: Optional[Tensor] = None, silu: bool = False):
    """Returns (dx rows bf16, dgamma_part f32 [B, C], dbeta_part f32 [B, C], dadd f32 [B, C] | None): the per-sample partial sums are
    reduced over B by the caller (`colreduce_f32(part, out=param.grad)`), or ARE the gradient of a per-sample affine."""
    _need(dy, bf16, "dy")
    _need(rows, bf16, "rows")
    if dy.shape != rows.shape or not dy.is_contiguous() or not rows.is_contiguous():
        raise ValueError("cfhip groupnorm_nhwc_bwd: dy and x must be contiguous bf16 rows of one shape")
    c = rows.shape[1]
    inner = rows.shape[0] // b
    affine_bs = _gn_affine_stride(gamma, beta, b, c)
    lib = _lib.load()
    splits = gn_nhwc_splits(b, inner, c, groups, True)
    dx = torch.empty_like(rows)
    dg = torch.empty((b, c), dtype=f32, device=rows.device)
    db = torch.empty((b, c), dtype=f32, device=rows.device)
    dadd = torch.empty((b, c), dtype=f32, device=rows.device) if add is not None else None
    ws = None if splits == 0 else torch.empty((max(4, lib.cfhip_groupnorm_nhwc_workspace(b, c, groups, splits, 1, int(add is not None))) // 4,),
                                              dtype=f32, device=rows.device)
    rc = lib.cfhip_groupnorm_nhwc_bwd(dy.data_ptr(), rows.data_ptr(), _p(add), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), _p(dadd), b, c, groups, inner,
                                      int(silu), affine_bs, splits, _p(ws), _stream())
    _lib.check(rc, "groupnorm_nhwc_bwd")
    return dx, dg, db, dadd


def upsample2_nhwc(rows: Tensor, b: int, h: int, w: int, backward: bool = False) -> Tensor:
    """nearest x2 on NHWC rows [B * H * W, C] (h, w = the SMALL size): forward -> [B * 4 H W, C]; backward: dy rows [B * 4 H W, C] -> dx"""
    _need(rows, bf16, "rows")
    c = rows.shape[1]
    n_in = b * h * w * (4 if backward else 1)
    if rows.dim() != 2 or not rows.is_contiguous() or rows.shape[0] != n_in:
        raise ValueError("cfhip upsample2_nhwc: contiguous bf16 rows of the stated geometry expected")
    out = torch.empty((b * h * w * (1 if backward else 4), c), dtype=bf16, device=rows.device)
    fn = _lib.load().cfhip_upsample2_nhwc_bwd if backward else _lib.load().cfhip_upsample2_nhwc_fwd
    _lib.check(fn(rows.data_ptr(), out.data_ptr(), b, h, w, c, _stream()), "upsample2_nhwc")
    return out


GN_MAX_CG = _H["CFHIP_GN_MAX_CG"]  # channels per group of the backward's 8-per-lane and split kernels


def _gn_form(splits: int, cg: int, ws_per_slice: int, *tensors: Tensor):
    """(splits, workspace) of one NCHW GroupNorm call.  The split form is demoted to the one-workgroup form (splits = 1, no
    workspace) for what it cannot take: a misaligned view, or more than GN_MAX_CG channels per group (`cg`: backward only, 0 in
    forward); the library then picks the 8-per-lane or the scalar kernel from what it is handed."""
    if splits > 1 and (cg > GN_MAX_CG or any(t.data_ptr() % 16 for t in tensors)):
        splits = 1
    ws = torch.empty((ws_per_slice * splits,), dtype=f32, device=tensors[0].device) if splits > 1 else None
    return splits, ws


def groupnorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, *, add: Optional[Tensor] = None,
                  silu: bool = False):
    """x [B, C, ...] f32 / bf16 -> (y bf16, mean f32 [B*G], rstd f32 [B*G]); y = [SiLU](GN(x + add[b, c])).
    gamma / beta: f32 [C], or [B, C] = one affine per sample (the scale-shift norm of residual.py:236-239)."""
    if x.dtype not in (f32, bf16) or not x.is_cuda or not x.is_contiguous() or x.dim() < 2:
        raise ValueError("cfhip groupnorm_fwd: x must be a contiguous f32/bf16 [B, C, ...] device tensor")
    _need(gamma, f32, "gamma")
    _need(beta, f32, "beta")
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    affine_bs = _gn_affine_stride(gamma, beta, b, c)
    if add is not None:
        _need(add, f32, "add")
        if tuple(add.shape) != (b, c) or not add.is_contiguous():
            raise ValueError("cfhip groupnorm_fwd: add must be contiguous f32 [B, C]")
    y = torch.empty(x.shape, dtype=bf16, device=x.device)
    mean = torch.empty((b * groups,), dtype=f32, device=x.device)
    rstd = torch.empty((b * groups,), dtype=f32, device=x.device)
    splits, ws = _gn_form(gn_splits(b, c, groups, inner), 0, b * groups * 2, x)
    rc = _lib.load().cfhip_groupnorm_fwd(x.data_ptr(), int(x.dtype == f32), _p(add), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), b, c, groups, inner, float(eps), int(silu), affine_bs,
                                         splits, _p(ws), _stream())
    _lib.check(rc, "groupnorm_fwd")
    return y, mean, rstd


def groupnorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, beta: Tensor, mean: Tensor, rstd: Tensor, groups: int, *,
                  add: Optional[Tensor] = None, silu: bool = False, reduce: bool = True):
    """Returns (dx bf16, dgamma, dbeta, dadd f32 [B, C] | None); dgamma / dbeta have the shape of gamma ([C], or [B, C]
    for a per-sample affine).  reduce=False: the per-sample partial sums [B, C] are returned as they are (the caller
    reduces them over B where they belong, e.g. `colreduce_f32(part, out=param.grad)`)."""
    _need(dy, bf16, "dy")
    if not dy.is_contiguous():
        dy = dy.contiguous()
    b, c = x.shape[0], x.shape[1]
    inner = x.numel() // (b * c)
    affine_bs = _gn_affine_stride(gamma, beta, b, c)
    dx = torch.empty(x.shape, dtype=bf16, device=x.device)
    dg_part = torch.empty((b, c), dtype=f32, device=x.device)
    db_part = torch.empty((b, c), dtype=f32, device=x.device)
    dadd = torch.empty((b, c), dtype=f32, device=x.device) if add is not None else None
    splits, ws = _gn_form(gn_splits(b, c, groups, inner), c // groups, b * c * 3, x, dy)
    rc = _lib.load().cfhip_groupnorm_bwd(dy.data_ptr(), x.data_ptr(), int(x.dtype == f32), _p(add), gamma.data_ptr(), beta.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dg_part.data_ptr(), db_part.data_ptr(),
                                         _p(dadd), b, c, groups, inner, int(silu), affine_bs, splits, _p(ws), _stream())
    _lib.check(rc, "groupnorm_bwd")
    if affine_bs or not reduce:
        return dx, dg_part, db_part, dadd
    return dx, colreduce_f32(dg_part), colreduce_f32(db_part), dadd


TIME_PROJ_MAX = _H["CFHIP_TIME_PROJ_MAX"]  # problems per launch of the grouped time-embedding projection


def _time_proj_table(rows) -> "ctypes.Array":
    """4 int64 per problem, a HOST array that lives until the call returns (the pointers travel in the kernel arguments)"""
    flat = [int(v) for row in rows for v in row]
    return (ctypes.c_int64 * len(flat))(*flat)


def time_proj_fwd(emb: Tensor, weights16, biases, t16: Tensor):
    """out_i = Linear_i(SiLU(emb)) for every (weight bf16 [N_i, K], bias f32 [N_i] or None) in ONE launch; returns the list of f32
    [B, N_i] outputs and fills t16 = bf16 SiLU(emb) [B, K] (cfhip_time_proj_fwd; reference residual.py:226-239 per block)"""
    _need(emb, f32, "emb")
    b, k = emb.shape
    outs = [torch.empty((b, w.shape[0]), dtype=f32, device=emb.device) for w in weights16]
    rows = []
    for w, bias, out in zip(weights16, biases, outs):
        _need(w, bf16, "weight")
        if w.shape[1] != k or not w.is_contiguous() or (bias is not None and (bias.dtype != f32 or not bias.is_contiguous())):
            raise ValueError("cfhip time_proj_fwd: contiguous bf16 [N, K] weights and f32 [N] biases expected")
        rows.append((w.data_ptr(), 0 if bias is None else bias.data_ptr(), out.data_ptr(), w.shape[0]))
    table = _time_proj_table(rows)
    _lib.check(_lib.load().cfhip_time_proj_fwd(emb.data_ptr(), b, k, ctypes.addressof(table), len(rows), t16.data_ptr(), _stream()),
               "time_proj_fwd")
    return outs


def time_proj_bwd(emb: Tensor, weights16, dys, dys16) -> Tensor:
    """d_emb = SiLU'(emb) * sum_i bf16(dY_i) W_i in two launches (partial sums per 64 columns, then their sum in a fixed order);
    dys[i] None = no gradient for output i; dys16[i]: bf16 [B, N_i] buffers that receive the rounded dY_i (or None)"""
    b, k = emb.shape
    rows = []
    nblk = 0
    for w, dy, dy16 in zip(weights16, dys, dys16):
        if dy is not None and (dy.dtype != f32 or not dy.is_contiguous() or dy.shape != (b, w.shape[0])):
            raise ValueError("cfhip time_proj_bwd: contiguous f32 [B, N] gradients expected")
        rows.append((w.data_ptr(), 0 if dy is None else dy.data_ptr(), 0 if dy16 is None else dy16.data_ptr(), w.shape[0]))
        nblk += (w.shape[0] + 63) // 64
    table = _time_proj_table(rows)
    partial = torch.empty((nblk, (b + 7) // 8 * 8, k), dtype=f32, device=emb.device)
    d_emb = torch.empty_like(emb)
    _lib.check(_lib.load().cfhip_time_proj_bwd(emb.data_ptr(), b, k, ctypes.addressof(table), len(rows), partial.data_ptr(),
                                               d_emb.data_ptr(), _stream()), "time_proj_bwd")
    return d_emb


def silu_f32_fwd(x: Tensor) -> Tensor:
    _need(x, f32, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_silu_f32_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "silu_f32_fwd")
    return y


def silu_f32_bwd(dy: Tensor, x: Tensor) -> Tensor:
    _need(dy, f32, "dy")
    _need(x, f32, "x")
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_silu_f32_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), _stream()),
               "silu_f32_bwd")
    return dx


def _resample(name: str, x: Tensor, out_hw: Tuple[int, int], small_hw: Tuple[int, int]) -> Tensor:
    _need(x, bf16, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"cfhip {name}: contiguous bf16 [B, C, H, W] expected")
    b, c = x.shape[0], x.shape[1]
    out = torch.empty((b, c, out_hw[0], out_hw[1]), dtype=bf16, device=x.device)
    rc = getattr(_lib.load(), f"cfhip_{name}")(x.data_ptr(), out.data_ptr(), b * c, small_hw[0], small_hw[1], _stream())
    _lib.check(rc, name)
    return out


def reflect_pad2d_fwd(x: Tensor, pads: Tuple[int, int, int, int]) -> Tensor:
    """nn.ReflectionPad2d((left, right, top, bottom)): x [B, C, H, W] bf16 / f32 -> bf16 [B, C, H + t + b, W + l + r]."""
    _need(x, x.dtype if x.dtype in (bf16, f32) else bf16, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("cfhip reflect_pad2d: contiguous [B, C, H, W] expected")
    pl, pr, pt, pb = (int(v) for v in pads)
    b, c, h, w = x.shape
    out = torch.empty((b, c, h + pt + pb, w + pl + pr), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_reflect_pad2d_fwd(x.data_ptr(), int(x.dtype == f32), out.data_ptr(), b * c, h, w, pl, pr, pt, pb, _stream())
    _lib.check(rc, "reflect_pad2d_fwd")
    return out


def reflect_pad2d_bwd(dy: Tensor, pads: Tuple[int, int, int, int]) -> Tensor:
    _need(dy, bf16, "dy")
    if dy.dim() != 4 or not dy.is_contiguous():
        raise ValueError("cfhip reflect_pad2d_bwd: contiguous bf16 [B, C, Ho, Wo] expected")
    pl, pr, pt, pb = (int(v) for v in pads)
    b, c, ho, wo = dy.shape
    h, w = ho - pt - pb, wo - pl - pr
    dx = torch.empty((b, c, h, w), dtype=bf16, device=dy.device)
    rc = _lib.load().cfhip_reflect_pad2d_bwd(dy.data_ptr(), dx.data_ptr(), b * c, h, w, pl, pr, pt, pb, _stream())
    _lib.check(rc, "reflect_pad2d_bwd")
    return dx


def upsample2_fwd(x: Tensor) -> Tensor:
    h, w = x.shape[2], x.shape[3]
    return _resample("upsample2_fwd", x, (2 * h, 2 * w), (h, w))


def upsample2_bwd(dy: Tensor) -> Tensor:
    h, w = dy.shape[2] // 2, dy.shape[3] // 2
    return _resample("upsample2_bwd", dy, (h, w), (h, w))


def avgpool2_fwd(x: Tensor) -> Tensor:
    if x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError("cfhip avgpool2: even spatial sizes expected")
    h, w = x.shape[2] // 2, x.shape[3] // 2
    return _resample("avgpool2_fwd", x, (h, w), (h, w))


def avgpool2_bwd(dy: Tensor) -> Tensor:
    h, w = dy.shape[2], dy.shape[3]
    return _resample("avgpool2_bwd", dy, (2 * h, 2 * w), (h, w))


def timestep_embedding(t: Tensor, dim: int, max_period: float = 10000.0) -> Tensor:
    """t int64 [B] -> f32 [B, dim] = [cos(t f) | sin(t f)] (reference multimodal/diffusion/unet.py:52-74); an f32 t (the sigma-space
    samplers' fractional timesteps) takes the float entry, arg = t * f"""
    if t.dtype == f32 and t.is_cuda and t.dim() == 1:
        out = torch.empty((t.shape[0], dim), dtype=f32, device=t.device)
        _lib.check(_lib.load().cfhip_timestep_embedding_f32(t.contiguous().data_ptr(), out.data_ptr(), t.shape[0], dim,
                                                            float(max_period), _stream()), "timestep_embedding_f32")
        return out
    if t.dtype != torch.int64 or not t.is_cuda or t.dim() != 1:
        raise TypeError("cfhip timestep_embedding: t must be int64 (or f32) [B] on the device")
    out = torch.empty((t.shape[0], dim), dtype=f32, device=t.device)
    _lib.check(_lib.load().cfhip_timestep_embedding(t.contiguous().data_ptr(), out.data_ptr(), t.shape[0], dim,
                                                    float(max_period), _stream()), "timestep_embedding")
    return out


def conv3x3_nhwc(x_rows: Tensor, wk: Tensor, bias: Optional[Tensor], b: int, h: int, w: int) -> Tensor:
    """Implicit-GEMM 3x3 / stride 1 / pad 1 convolution: x_rows bf16 [B*H*W, Cin] (NHWC), wk bf16 [Cout, 9*Cin] with
    k = (ky*3 + kx)*Cin + c, bias f32 [Cout] | None -> bf16 [B*H*W, Cout]."""
    _need(x_rows, bf16, "x_rows")
    _need(wk, bf16, "wk")
    m, cin = x_rows.shape
    cout = wk.shape[0]
    if m != b * h * w or wk.shape[1] != 9 * cin or not x_rows.is_contiguous() or not wk.is_contiguous():
        raise ValueError(f"cfhip conv3x3_nhwc: x_rows {tuple(x_rows.shape)} / wk {tuple(wk.shape)} do not match "
                         f"B={b} H={h} W={w} (dense NHWC rows and [Cout, 9*Cin] filters expected)")
    if bias is not None:
        _need(bias, f32, "bias")
    y = torch.empty((m, cout), dtype=bf16, device=x_rows.device)
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["conv3x3"] += 2.0 * m * cout * 9 * cin
    lib = _lib.load()
    nbytes = lib.cfhip_conv3x3_workspace(b, h, w, cin, cout)  # > 0 when the shape splits its reduction
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=x_rows.device)
    _lib.check(lib.cfhip_conv3x3_nhwc_bf16(x_rows.data_ptr(), wk.data_ptr(), _p(bias), y.data_ptr(), b, h, w, cin, cout,
                                           ws.data_ptr(), nbytes, _stream()), "conv3x3_nhwc")
    return y


def conv3x3_wgrad_ok(b: int, h: int, w: int) -> bool:
    return h >= 2 and w >= 2 and h < 65536 and w < 65536 and b * h * w * max(h, w) < (1 << 32)


def _gconv_args(x_shape, w: Tensor, stride: int, pad: int, dil: int, groups: int):
    b, cin, h, wd = x_shape
    cout, cgi, kh, kw = w.shape
    if cin % groups or cout % groups or cgi != cin // groups:
        raise ValueError(f"cfhip grouped conv: weight {tuple(w.shape)} does not fit Cin {cin} with groups {groups}")
    return [b, cin, h, wd, cout, kh, kw, int(stride), int(pad), int(dil), int(groups)]


def conv2d_grouped_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int, groups: int) -> Tensor:
    """F.conv2d(x, w, bias, stride, pad, dil, groups) for groups > 1 (cfhip_conv2d_grouped_fwd): x bf16 NCHW, w bf16
    [Cout, Cin / groups, kh, kw], bias f32 -> y bf16 NCHW"""
    _need(x, bf16, "x")
    _need(w, bf16, "w")
    args = _gconv_args(x.shape, w, stride, pad, dil, groups)
    ho, wo = conv_out_hw(x.shape[2], x.shape[3], w.shape[2], w.shape[3], stride, pad, dil)
    y = torch.empty((x.shape[0], w.shape[0], ho, wo), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_conv2d_grouped_fwd(x.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), *args, _stream())
    _lib.check(rc, "conv2d_grouped_fwd")
    return y


def conv2d_grouped_bwd_input(dy: Tensor, w: Tensor, x_shape, stride: int, pad: int, dil: int, groups: int) -> Tensor:
    _need(dy, bf16, "dy")
    _need(w, bf16, "w")
    dx = torch.empty(tuple(x_shape), dtype=bf16, device=dy.device)
    rc = _lib.load().cfhip_conv2d_grouped_bwd_input(dy.data_ptr(), w.data_ptr(), dx.data_ptr(),
                                                    *_gconv_args(x_shape, w, stride, pad, dil, groups), _stream())
    _lib.check(rc, "conv2d_grouped_bwd_input")
    return dx


def conv2d_grouped_bwd_weight(dy: Tensor, x: Tensor, dw: Tensor, accumulate: bool, bias_grad: Optional[Tensor],
                              bias_grad_accumulate: bool, stride: int, pad: int, dil: int, groups: int) -> None:
    """dw f32 [Cout, Cin / groups, kh, kw] (+)= the filter gradient, bias_grad f32 [Cout] (+)= dy summed over b, y, x"""
    _need(dy, bf16, "dy")
    _need(x, bf16, "x")
    _need(dw, f32, "dw")
    rc = _lib.load().cfhip_conv2d_grouped_bwd_weight(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), int(accumulate), _p(bias_grad),
                                                     int(bias_grad_accumulate), *_gconv_args(x.shape, dw, stride, pad, dil, groups),
                                                     _stream())
    _lib.check(rc, "conv2d_grouped_bwd_weight")


def conv3x3_wgrad_nhwc(dy_rows: Tensor, x_rows: Tensor, b: int, h: int, w: int, split_k: int = 1,
                       out: Optional[Tensor] = None, accumulate: bool = False, bias_grad: Optional[Tensor] = None,
                       bias_grad_accumulate: bool = False) -> Tensor:
    """dy_rows bf16 [B*H*W, Cout], x_rows bf16 [B*H*W, Cin] (NHWC) -> f32 [Cout, Cin, 3, 3] (the reference's filter
    layout), written or added to `out`."""
    _need(dy_rows, bf16, "dy_rows")
    _need(x_rows, bf16, "x_rows")
    m, cout = dy_rows.shape
    cin = x_rows.shape[1]
    if m != b * h * w or x_rows.shape[0] != m or not dy_rows.is_contiguous() or not x_rows.is_contiguous():
        raise ValueError("cfhip conv3x3_wgrad_nhwc: dense NHWC rows [B*H*W, C] expected for both operands")
    if bias_grad is not None:
        _need(bias_grad, f32, "bias_grad")
    if out is None:
        out, accumulate = torch.empty((cout, cin, 3, 3), dtype=f32, device=dy_rows.device), False
    else:
        _need(out, f32, "out")
        if out.numel() != cout * cin * 9 or not out.is_contiguous():
            raise ValueError("cfhip conv3x3_wgrad_nhwc: `out` must be a contiguous f32 [Cout, Cin, 3, 3]")
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["conv3x3"] += 2.0 * m * cout * 9 * cin
    lib = _lib.load()
    nbytes = lib.cfhip_conv3x3_wgrad_workspace(cin, cout, split_k)
    ws = torch.empty((nbytes // 4,), dtype=f32, device=dy_rows.device)
    _lib.check(lib.cfhip_conv3x3_wgrad_nhwc_bf16(dy_rows.data_ptr(), x_rows.data_ptr(), out.data_ptr(), int(accumulate),
                                                 _p(bias_grad), int(bias_grad_accumulate), b, h, w, cin, cout, split_k,
                                                 ws.data_ptr(), nbytes, _stream()), "conv3x3_wgrad_nhwc")
    return out


def conv3x3_pack_filters(w16: Tensor, rotate: bool, out: Optional[Tensor] = None) -> Tensor:
    """w16 bf16 [Cout, Cin, 3, 3] -> [Cout, 9*Cin] (k = (ky, kx, c)) or, rotate=True, [Cin, 9*Cout] with the taps rotated
    by 180 degrees (k = (ky, kx, co)): the filter matrices of conv3x3_nhwc for the forward / the input gradient."""
    _need(w16, bf16, "w16")
    if w16.dim() != 4 or tuple(w16.shape[2:]) != (3, 3) or not w16.is_contiguous():
        raise ValueError("cfhip conv3x3_pack_filters: contiguous bf16 [Cout, Cin, 3, 3] expected")
    cout, cin = w16.shape[0], w16.shape[1]
    if out is None:
        out = torch.empty((cin, 9 * cout) if rotate else (cout, 9 * cin), dtype=bf16, device=w16.device)
    _lib.check(_lib.load().cfhip_conv3x3_pack_filters(w16.data_ptr(), out.data_ptr(), cout, cin, int(rotate), _stream()),
               "conv3x3_pack_filters")
    return out


def conv3x3_direct_dims(cout: int, cin: int, mode: int) -> Tuple[int, int, int]:
    """(N, Cp, Kp) of the direct 3x3 convolution's filter operand wp[N][Kp] (cfhip_conv3x3_direct_pack): mode 0 the forward, 1 the
    input gradient"""
    n = cout if mode == 0 else (cin + 7) // 8 * 8
    cp = ((cin if mode == 0 else cout) + 7) // 8 * 8
    return n, cp, (9 * cp + 31) // 32 * 32


def conv3x3_direct_pack(w: Tensor, mode: int) -> Tensor:
    """f32 [Cout, Cin, 3, 3] -> bf16 wp [N, Kp], k = tap * Cp + c, zero padded; mode 1: channels swapped, taps mirrored"""
    _need(w, f32, "w")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not w.is_contiguous():
        raise ValueError("cfhip conv3x3_direct_pack: contiguous f32 [Cout, Cin, 3, 3] expected")
    cout, cin = w.shape[0], w.shape[1]
    n, _, kp = conv3x3_direct_dims(cout, cin, mode)
    wp = torch.empty((n, kp), dtype=bf16, device=w.device)
    _lib.check(_lib.load().cfhip_conv3x3_direct_pack(w.data_ptr(), wp.data_ptr(), cout, cin, int(mode), _stream()), "conv3x3_direct_pack")
    return wp


def conv3x3_direct(x: Tensor, wp: Tensor, bias: Optional[Tensor], h: int, w: int, stride: int, mode: int) -> Tensor:
    """The direct 3x3 / pad 1 convolution on NHWC bf16.  (h, w): the image of the FORWARD's input.  mode 0: x [B, h, w, Cp] ->
    [B, ho, wo, N] (+ bias f32 [N]); mode 1: x = dY [B, ho, wo, Cp] -> dX [B, h, w, N]."""
    _need(x, bf16, "x")
    _need(wp, bf16, "wp")
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    b, cp = x.shape[0], x.shape[-1]
    n = wp.shape[0]
    if x.dim() != 4 or not x.is_contiguous() or tuple(x.shape[1:3]) != ((h, w) if mode == 0 else (ho, wo)) or not wp.is_contiguous() \
            or wp.shape[1] != (9 * cp + 31) // 32 * 32:
        raise ValueError(f"cfhip conv3x3_direct: x {tuple(x.shape)} / wp {tuple(wp.shape)} do not match h={h} w={w} stride={stride} "
                         f"mode={mode} (dense NHWC and [N, Kp] filters expected)")
    if bias is not None:
        _need(bias, f32, "bias")
        if bias.numel() != n or not bias.is_contiguous():
            raise ValueError("cfhip conv3x3_direct: bias must be contiguous f32 [N]")
    y = torch.empty((b, ho, wo, n) if mode == 0 else (b, h, w, n), dtype=bf16, device=x.device)
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["conv3x3"] += 2.0 * b * ho * wo * n * 9 * cp
    _lib.check(_lib.load().cfhip_conv3x3_direct_bf16(x.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), b, h, w, cp, n, int(stride),
                                                     int(mode), _stream()), "conv3x3_direct")
    return y


DENSE_EPILOGUES = {name: _H["CFHIP_DENSE_EPI_" + name.upper()] for name in ("none", "lrelu", "res1", "res2")}
DENSE_TILE = (_H["CFHIP_DENSE_TILE_H"], _H["CFHIP_DENSE_TILE_W"])  # output pixels per workgroup of the dense-block convolution


def conv3x3_dense_pack(w: Tensor) -> Tensor:
    """f32 [Cout, Cin, 3, 3] -> the filter operand of `conv3x3_dense`: bf16 wp [N, Kp] in the layout of cfhip_conv3x3_direct_pack mode 0
    (k = tap * Cp + c, Cp = Cin rounded up to 8, Kp = 9 Cp rounded up to 32), N = Cout rounded up to 16, 32 or 64; the rows past Cout and
    every padded k are exact zeros."""
    _need(w, f32, "w")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not w.is_contiguous():
        raise ValueError("cfhip conv3x3_dense_pack: contiguous f32 [Cout, Cin, 3, 3] expected")
    cout, cin = w.shape[0], w.shape[1]
    if cout > 64 or cin > 192:
        raise ValueError(f"cfhip conv3x3_dense_pack: Cout = {cout}, Cin = {cin} (the kernel covers Cout <= 64, Cin <= 192)")
    n = 16 if cout <= 16 else 32 if cout <= 32 else 64
    _, _, kp = conv3x3_direct_dims(cout, cin, 0)
    wp = (torch.empty if n == cout else torch.zeros)((n, kp), dtype=bf16, device=w.device)
    _lib.check(_lib.load().cfhip_conv3x3_direct_pack(w.data_ptr(), wp.data_ptr(), cout, cin, 0, _stream()), "conv3x3_dense_pack")
    return wp


def _dense_rows(t: Tensor, name: str, rows: int, width: Optional[int] = None) -> int:
    """row stride of a bf16 slice [rows, width] of a dense NHWC buffer"""
    _need(t, bf16, name)
    if t.dim() != 2 or t.shape[0] != rows or (width is not None and t.shape[1] != width) or (t.stride(1) != 1 and t.shape[1] > 1):
        raise ValueError(f"cfhip conv3x3_dense: `{name}` must be bf16 [{rows}, {width if width is not None else 'C'}] with unit channel "
                         f"stride, got {tuple(t.shape)} / {t.stride()}")
    ld = t.stride(0) if rows > 1 else max(t.stride(0), t.shape[1])
    if ld % 8 or ld < t.shape[1] or t.data_ptr() % 16:
        raise ValueError(f"cfhip conv3x3_dense: `{name}` needs a row stride that is a multiple of 8 and a 16-byte aligned first channel "
                         f"(stride {ld}, offset {t.storage_offset()})")
    return ld


def conv3x3_dense(x: Tensor, wp: Tensor, bias: Optional[Tensor], y: Tensor, b: int, h: int, w: int, *, epilogue: str = "none",
                  slope: float = 0.2, r1: Optional[Tensor] = None, s1: float = 1.0, r2: Optional[Tensor] = None, s2: float = 1.0,
                  up2: bool = False) -> Tensor:
    """The dense-block 3x3 / pad 1 convolution (cfhip_conv3x3_dense_bf16) on slices of NHWC buffers, written into `y`.
    x: bf16 [b h w, Cin], a channel-prefix view of a buffer (any row stride that is a multiple of 8); wp: `conv3x3_dense_pack`.
    y: a bf16 view [b ho wo, n_store] of a buffer, or a contiguous f32 [b, n_store, ho, wo] (the net's last layer); ho = 2 h with `up2`
    (the nearest 2x upsampling of x is read, not built).  epilogue: none | lrelu (slope) | res1 (s1 v + r1) | res2 ((s1 v + r1) s2 + r2),
    r1 / r2 bf16 views [b ho wo, n_store].  bias f32 [n_store] or None.  The library refuses an output that overlaps what is read."""
    if epilogue not in DENSE_EPILOGUES:
        raise ValueError(f"cfhip conv3x3_dense: unknown epilogue {epilogue!r} ({', '.join(DENSE_EPILOGUES)})")
    _need(wp, bf16, "wp")
    ho, wo = (2 * h, 2 * w) if up2 else (h, w)
    ld_in = _dense_rows(x, "x", b * h * w)
    cin, n = x.shape[1], wp.shape[0]
    if wp.dim() != 2 or not wp.is_contiguous() or wp.shape[1] != (9 * cin + 31) // 32 * 32 or cin % 8:
        raise ValueError(f"cfhip conv3x3_dense: wp {tuple(wp.shape)} does not match Cin = {cin} ([N, Kp] of conv3x3_dense_pack, Cin % 8 == 0)")
    f32_out = y.dtype == f32
    if f32_out:
        _need(y, f32, "y")
        if y.dim() != 4 or not y.is_contiguous() or y.shape[0] != b or tuple(y.shape[2:]) != (ho, wo):
            raise ValueError(f"cfhip conv3x3_dense: an f32 `y` must be contiguous [{b}, n_store, {ho}, {wo}], got {tuple(y.shape)}")
        n_store, ld_out = y.shape[1], 0
    else:
        ld_out = _dense_rows(y, "y", b * ho * wo)
        n_store = y.shape[1]
    if not 1 <= n_store <= n:
        raise ValueError(f"cfhip conv3x3_dense: y holds {n_store} channels, the filters {n}")
    if bias is not None:
        _need(bias, f32, "bias")
        if bias.numel() != n_store or not bias.is_contiguous():
            raise ValueError(f"cfhip conv3x3_dense: bias must be contiguous f32 [{n_store}]")
    need = {"none": 0, "lrelu": 0, "res1": 1, "res2": 2}[epilogue]
    if (r1 is None) != (need < 1) or (r2 is None) != (need < 2):
        raise ValueError(f"cfhip conv3x3_dense: epilogue {epilogue!r} takes {need} residual operand(s)")
    ld_r1 = _dense_rows(r1, "r1", b * ho * wo, n_store) if r1 is not None else 0
    ld_r2 = _dense_rows(r2, "r2", b * ho * wo, n_store) if r2 is not None else 0
    if FLOP_COUNTER is not None:
        FLOP_COUNTER.flops["conv3x3"] += 2.0 * b * ho * wo * n_store * 9 * cin
    _lib.check(_lib.load().cfhip_conv3x3_dense_bf16(x.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), _p(r1), _p(r2), b, h, w, cin, n,
                                                    n_store, ld_in, ld_out, ld_r1, ld_r2, DENSE_EPILOGUES[epilogue], float(slope), float(s1),
                                                    float(s2), int(up2), int(f32_out), _stream()), "conv3x3_dense")
    return y


def pixel_unshuffle_map(c: int, h: int, w: int, s: int) -> Tensor:
    """int64 [h / s, w / s, c s^2]: the flat index into one [c, h, w] image that channel `k s^2 + dy s + dx` of output pixel (oy, ox)
    takes, k the image channel — the host statement of the reference's `pixel_unshuffle` (rrdb.py:47-55) that `pixel_unshuffle_nhwc`
    implements"""
    if s not in (1, 2, 4) or h % s or w % s:
        raise ValueError(f"cfhip pixel_unshuffle: s = {s} (1, 2 or 4) must divide H = {h} and W = {w}")
    oc = torch.arange(c * s * s)
    k, dy, dx = oc // (s * s), oc // s % s, oc % s
    oy, ox = torch.arange(h // s).view(-1, 1, 1), torch.arange(w // s).view(1, -1, 1)
    return (k * h + oy * s + dy) * w + ox * s + dx


def pixel_unshuffle_nhwc(x: Tensor, s: int) -> Tensor:
    """x [B, C, H, W] f32 or bf16 -> bf16 NHWC [B, H / s, W / s, Cp] with the channel order of `pixel_unshuffle_map`, Cp = C s^2 rounded
    up to a multiple of 8, padding channels zero (s = 1: the layout change alone)"""
    if not x.is_cuda:
        raise RuntimeError(f"cfhip: `x` must live on the HIP device (got {x.device})")
    if x.dtype not in (f32, bf16):
        raise TypeError(f"cfhip pixel_unshuffle_nhwc: x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"cfhip pixel_unshuffle_nhwc: contiguous [B, C, H, W] expected, got {tuple(x.shape)} / {x.stride()}")
    b, c, h, w = x.shape
    if s not in (1, 2, 4) or h % s or w % s:
        raise ValueError(f"cfhip pixel_unshuffle_nhwc: s = {s} (1, 2 or 4) must divide H = {h} and W = {w}")
    y = torch.empty((b, h // s, w // s, (c * s * s + 7) // 8 * 8), dtype=bf16, device=x.device)
    _lib.check(_lib.load().cfhip_pixel_unshuffle_nhwc(x.data_ptr(), int(x.dtype == f32), y.data_ptr(), b, c, h, w, int(s), _stream()),
               "pixel_unshuffle_nhwc")
    return y


def silu_bf16_fwd(x: Tensor) -> Tensor:
    _need(x, bf16, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_silu_bf16_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "silu_bf16_fwd")
    return y


def silu_bf16_bwd(dy: Tensor, x: Tensor) -> Tensor:
    _need(dy, bf16, "dy")
    _need(x, bf16, "x")
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_silu_bf16_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), _stream()), "silu_bf16_bwd")
    return dx


def scale_bf16(x: Tensor, scale: float) -> Tensor:
    """bf16(scale * x) of a contiguous bf16 tensor"""
    _need(x, bf16, "x")
    if not x.is_contiguous():
        raise ValueError("cfhip scale_bf16: contiguous bf16 expected")
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_scale_bf16(x.data_ptr(), y.data_ptr(), x.numel(), float(scale), _stream()), "scale_bf16")
    return y


PACK_GROUP_MAX = _H["CFHIP_PACK_GROUP_MAX"]  # problems per launch of conv3x3_pack_grouped


def conv3x3_pack_grouped(items) -> None:
    """items: (w16 bf16 [Cout, Cin, 3, 3], out, rotate) — `conv3x3_pack_filters` for all of them in ceil(len / 64) launches"""
    lib = _lib.load()
    for i in range(0, len(items), PACK_GROUP_MAX):
        flat = []
        for w16, out, rotate in items[i:i + PACK_GROUP_MAX]:
            if w16.dtype != bf16 or w16.dim() != 4 or tuple(w16.shape[2:]) != (3, 3) or not w16.is_contiguous() or out.dtype != bf16 \
                    or out.numel() != w16.numel():
                raise ValueError("cfhip conv3x3_pack_grouped: contiguous bf16 [Cout, Cin, 3, 3] filters and bf16 outputs of the same size expected")
            flat += [w16.data_ptr(), out.data_ptr(), w16.shape[0], w16.shape[1], int(bool(rotate))]
        table = (ctypes.c_int64 * len(flat))(*flat)
        _lib.check(lib.cfhip_conv3x3_pack_filters_grouped(ctypes.addressof(table), len(flat) // 5, _stream()), "conv3x3_pack_filters_grouped")


def sgemm_f32(a: Tensor, b: Tensor, *, a_trans: bool = False, b_trans: bool = False,
              alpha_dev: Optional[Tensor] = None, alpha: float = 1.0) -> Tensor:
    """fp32 C[m,n] = alpha * alpha_dev[0] * sum_k A(m,k) B(n,k) on dense f32 matrices (a: [M,K] or, a_trans, [K,M];
    b: [N,K] or, b_trans, [K,N]) -- the CLIP similarity logits and the products of their backward."""
    _need(a, f32, "a")
    _need(b, f32, "b")
    if a.dim() != 2 or b.dim() != 2 or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("cfhip sgemm_f32: dense 2-D f32 operands expected")
    m, k = (a.shape[1], a.shape[0]) if a_trans else (a.shape[0], a.shape[1])
    n, kb = (b.shape[1], b.shape[0]) if b_trans else (b.shape[0], b.shape[1])
    if k != kb:
        raise ValueError(f"cfhip sgemm_f32: reduction dims differ ({k} vs {kb})")
    if alpha_dev is not None:
        _need(alpha_dev, f32, "alpha_dev")
    out = torch.empty((m, n), dtype=f32, device=a.device)
    _lib.check(_lib.load().cfhip_sgemm_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0), b.stride(0),
                                           int(a_trans), int(b_trans), _p(alpha_dev), float(alpha), _stream()), "sgemm_f32")
    return out


def dot_f32(a: Tensor, b: Tensor) -> Tensor:
    """f32 [1] = sum(a * b) over two dense f32 tensors of equal size."""
    _need(a, f32, "a")
    _need(b, f32, "b")
    if a.numel() != b.numel() or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("cfhip dot_f32: dense f32 tensors of equal size expected")
    out = torch.zeros((1,), dtype=f32, device=a.device)
    _lib.check(_lib.load().cfhip_dot_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "dot_f32")
    return out


def spin(microseconds: int) -> None:
    """One idle wavefront on the current stream (stream self-check, see functional.distinct_stream)."""
    _lib.check(_lib.load().cfhip_spin(int(microseconds), _stream()), "spin")


def ema_update(ema: Tensor, p: Tensor, decay: float) -> None:
    """ema <- (1 - decay) * p + decay * ema over flat contiguous f32 buffers (bit-exact with the torch expression)."""
    _need(ema, f32, "ema")
    _need(p, f32, "p")
    if not ema.is_contiguous() or not p.is_contiguous() or ema.numel() != p.numel():
        raise ValueError("cfhip ema_update: contiguous f32 buffers of equal length expected")
    _lib.check(_lib.load().cfhip_ema_update(ema.data_ptr(), p.data_ptr(), p.numel(), float(1.0 - decay), float(decay),
                                            _stream()), "ema_update")


def geglu_fwd(vg: Tensor) -> Tensor:
    """vg bf16 [..., 2L] -> value * gelu(gate), bf16 [..., L]"""
    _need(vg, bf16, "vg")
    if not vg.is_contiguous() or vg.shape[-1] % 8:
        raise ValueError("cfhip geglu_fwd: contiguous [..., 2L] with L a multiple of 4 expected")
    l = vg.shape[-1] // 2
    out = torch.empty((*vg.shape[:-1], l), dtype=bf16, device=vg.device)
    _lib.check(_lib.load().cfhip_geglu_fwd(vg.data_ptr(), out.data_ptr(), vg.numel() // (2 * l), l, _stream()), "geglu_fwd")
    return out


def geglu_bwd(dy: Tensor, vg: Tensor) -> Tensor:
    _need(dy, bf16, "dy")
    _need(vg, bf16, "vg")
    l = vg.shape[-1] // 2
    dvg = torch.empty_like(vg)
    _lib.check(_lib.load().cfhip_geglu_bwd(dy.contiguous().data_ptr(), vg.data_ptr(), dvg.data_ptr(),
                                           vg.numel() // (2 * l), l, _stream()), "geglu_bwd")
    return dvg


def copy_strided(src: Tensor, dst: Tensor, batch: int, n: int, src_bs: int, dst_bs: int, src_off: int = 0,
                 dst_off: int = 0) -> None:
    """dst.flat[dst_off + b*dst_bs + i] = src.flat[src_off + b*src_bs + i] for b < batch, i < n (bf16)"""
    _need(src, bf16, "src")
    _need(dst, bf16, "dst")
    rc = _lib.load().cfhip_copy_strided_bf16(src.data_ptr() + 2 * src_off, dst.data_ptr() + 2 * dst_off, batch, n, src_bs,
                                             dst_bs, _stream())
    _lib.check(rc, "copy_strided_bf16")


def copy_strided2(src_a: Tensor, dst_a: Tensor, n_a: int, sa_bs: int, da_bs: int, src_b: Tensor, dst_b: Tensor, n_b: int, sb_bs: int,
                  db_bs: int, batch: int, *, src_a_off: int = 0, dst_a_off: int = 0, src_b_off: int = 0, dst_b_off: int = 0) -> None:
    """two `copy_strided` with the same batch count in one launch (a channel concatenation, or its backward split)"""
    for t, nm in ((src_a, "src_a"), (dst_a, "dst_a"), (src_b, "src_b"), (dst_b, "dst_b")):
        _need(t, bf16, nm)
    rc = _lib.load().cfhip_copy_strided2_bf16(src_a.data_ptr() + 2 * src_a_off, dst_a.data_ptr() + 2 * dst_a_off, n_a, sa_bs, da_bs,
                                              src_b.data_ptr() + 2 * src_b_off, dst_b.data_ptr() + 2 * dst_b_off, n_b, sb_bs, db_bs,
                                              batch, _stream())
    _lib.check(rc, "copy_strided2_bf16")


def q_sample(x: Tensor, noise: Tensor, t: Tensor, sqrt_ac: Tensor, sqrt_1mac: Tensor, out_dtype: torch.dtype = f32) -> Tensor:
    """x_t = sqrt_ac[t] * x + sqrt_1mac[t] * noise per sample (reference samplers/schema.py:94-108)"""
    for tt, nm in ((x, "x"), (noise, "noise"), (sqrt_ac, "sqrt_ac"), (sqrt_1mac, "sqrt_1mac")):
        _need(tt, f32, nm)
    if t.dtype != torch.int64 or not t.is_cuda:
        raise TypeError("cfhip q_sample: timesteps must be int64 on the device")
    x, noise = x.contiguous(), noise.contiguous()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    b = x.shape[0]
    rc = _lib.load().cfhip_q_sample(x.data_ptr(), noise.data_ptr(), t.contiguous().data_ptr(), sqrt_ac.data_ptr(),
                                    sqrt_1mac.data_ptr(), out.data_ptr(), int(out_dtype == f32), b, x.numel() // b,
                                    _stream())
    _lib.check(rc, "q_sample")
    return out


def mse_loss(pred: Tensor, target: Tensor, grad_scale: float, want_grad: bool = True):
    """Returns (loss_sum f32 [1] = sum_b mean((pred_b - target_b)^2), dpred bf16 = grad_scale * d loss_sum / d pred)."""
    _need(pred, bf16, "pred")
    _need(target, f32, "target")
    pred, target = pred.contiguous(), target.contiguous()
    b = pred.shape[0]
    loss = torch.zeros((1,), dtype=f32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    rc = _lib.load().cfhip_mse_loss(pred.data_ptr(), target.data_ptr(), loss.data_ptr(), _p(dpred), b, pred.numel() // b,
                                    float(grad_scale), _stream())
    _lib.check(rc, "mse_loss")
    return loss, dpred


SAMPLE_ROW = _H["CFHIP_SAMPLE_ROW"]  # f32 scalars per step in the sampler's table
SAMPLERS = {k: _H["CFHIP_SAMPLER_" + k.upper()] for k in ("ddim", "basic")}
PARAMETERIZATIONS = {k: _H["CFHIP_PARAM_" + k.upper()] for k in ("eps", "x0", "v")}
KSAMPLE_ROW = _H["CFHIP_KSAMPLE_ROW"]  # f32 scalars per model evaluation in a sigma-space sampler's table
KSAMPLERS = {k: _H["CFHIP_KSAMPLER_" + k[2:].upper()] for k in ("k_euler_a", "k_heun", "k_dpmpp_2m")}


def randn(n: int, seed: int, offset: int, device: torch.device, out: Optional[Tensor] = None) -> Tensor:
    """f32 [n] standard normals: Philox4x32-10 at counter (seed, offset + i / 4), Box-Muller (cfhip_randn_f32)"""
    if out is None:
        out = torch.empty((int(n),), dtype=f32, device=device)
    _need(out, f32, "out")
    if not out.is_contiguous() or out.numel() != n or n <= 0:
        raise ValueError("cfhip randn: a contiguous f32 output of n > 0 elements expected")
    _lib.check(_lib.load().cfhip_randn_f32(out.data_ptr(), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(offset) & 0xFFFFFFFFFFFFFFFF, _stream()), "randn_f32")
    return out


def gaussian_posterior(moments: Tensor, *, scale_factor: float = 1.0, seed: int = 0, offset: int = 0, noise: Optional[Tensor] = None,
                       deterministic: bool = False, want_z: bool = True, want_kl: bool = False,
                       out: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(z, kl) of the KL autoencoder's posterior (cfhip_gaussian_posterior): moments bf16 [B, 2E, h, w], dense NCHW or channels-last,
    read in place -> z f32 [B, E, h, w] = scale_factor * (mean + exp(0.5 clamp(log_var, -30, 20)) * n) and, with `want_kl`,
    kl f32 [B] = 0.5 sum(mean^2 + var - 1 - log_var).  n: `noise` (f32, the shape of z), nothing (`deterministic`: the mode), or
    the normals `randn(z.numel(), seed, offset)` holds at the same flat index."""
    _need(moments, bf16, "moments")
    if moments.dim() != 4 or moments.shape[1] % 2:
        raise ValueError("cfhip gaussian_posterior: moments must be [B, 2E, h, w]")
    b, c2, h, w = moments.shape
    if moments.is_contiguous():
        cl = 0
    elif moments.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        raise ValueError("cfhip gaussian_posterior: moments must be dense NCHW or channels-last")
    e = c2 // 2
    if not (want_z or want_kl):
        raise ValueError("cfhip gaussian_posterior: nothing asked for")
    z = None
    if want_z:
        z = torch.empty((b, e, h, w), dtype=f32, device=moments.device) if out is None else out
        _need(z, f32, "out")
        if tuple(z.shape) != (b, e, h, w) or not z.is_contiguous():
            raise ValueError("cfhip gaussian_posterior: `out` must be a contiguous f32 [B, E, h, w]")
    if noise is not None:
        _need(noise, f32, "noise")
        if deterministic or tuple(noise.shape) != (b, e, h, w) or not noise.is_contiguous():
            raise ValueError("cfhip gaussian_posterior: `noise` must be a contiguous f32 [B, E, h, w] (and not `deterministic`)")
    kl = torch.empty((b,), dtype=f32, device=moments.device) if want_kl else None
    rc = _lib.load().cfhip_gaussian_posterior(moments.data_ptr(), cl, _p(z), _p(kl), _p(noise), int(deterministic), b, e, h * w,
                                              float(scale_factor), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                              _stream())
    _lib.check(rc, "gaussian_posterior")
    return z, kl


VQ_MAX_DIM = _H["CFHIP_VQ_MAX_DIM"]  # widest code the nearest-code kernel takes


def vq_chunk(code_dimension: int) -> int:
    """codes of a `code_dimension`-wide codebook the nearest-code kernel holds in LDS at once (cfhip_vq_chunk; 0: unsupported)"""
    return int(_lib.load().cfhip_vq_chunk(int(code_dimension)))


def _vq_codebook(codebook: Tensor) -> Tuple[int, int]:
    _need(codebook, f32, "codebook")
    if codebook.dim() != 2 or not codebook.is_contiguous() or codebook.shape[0] < 1:
        raise ValueError("cfhip vq: the codebook must be a contiguous f32 [N, D] with N >= 1")
    n, d = codebook.shape
    if not 1 <= d <= VQ_MAX_DIM:
        raise NotImplementedError(f"cfhip vq: code dimension {d} is outside [1, {VQ_MAX_DIM}] (CFHIP_VQ_MAX_DIM)")
    return n, d


def vq_code_sqnorm(codebook: Tensor) -> Tensor:
    """f32 [N]: sum_d e_jd^2 of the codebook f32 [N, D] (cfhip_vq_code_sqnorm), what `vq_nearest` takes as `code_sq`"""
    n, d = _vq_codebook(codebook)
    out = torch.empty((n,), dtype=f32, device=codebook.device)
    _lib.check(_lib.load().cfhip_vq_code_sqnorm(codebook.data_ptr(), out.data_ptr(), n, d, _stream()), "vq_code_sqnorm")
    return out


def vq_nearest(z: Tensor, codebook: Tensor, *, code_sq: Optional[Tensor] = None, scale_factor: float = 1.0,
               want_z_q: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """(indices, z_q) of the nearest codebook row per pixel (cfhip_vq_nearest): z bf16 or f32 [B, D, h, w], dense NCHW or
    channels-last, read in place; codebook f32 [N, D]; code_sq f32 [N] = `vq_code_sqnorm(codebook)` (computed here when not
    given) -> indices int64 [B, h, w] = the lowest index of the least |z - e_j|^2 and, with `want_z_q`, z_q f32 [B, D, h, w]
    (contiguous) = scale_factor * codebook[indices].  The [B h w, N] distance matrix is never formed."""
    n, d = _vq_codebook(codebook)
    if not z.is_cuda:
        raise RuntimeError(f"cfhip: `z` must live on the HIP device (got {z.device})")
    if z.dtype not in (bf16, f32):
        raise TypeError(f"cfhip: `z` must be {bf16} or {f32}, got {z.dtype}")
    if z.dim() != 4 or z.shape[1] != d or z.numel() == 0:
        raise ValueError(f"cfhip vq_nearest: z must be a non-empty [B, {d}, h, w] for this codebook, got {tuple(z.shape)}")
    b, _, h, w = z.shape
    if z.is_contiguous():
        cl = 0
    elif z.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        raise ValueError("cfhip vq_nearest: z must be dense NCHW or channels-last")
    if code_sq is None:
        code_sq = vq_code_sqnorm(codebook)
    _need(code_sq, f32, "code_sq")
    if tuple(code_sq.shape) != (n,) or not code_sq.is_contiguous():
        raise ValueError("cfhip vq_nearest: `code_sq` must be a contiguous f32 [N]")
    indices = torch.empty((b, h, w), dtype=torch.int64, device=z.device)
    z_q = torch.empty((b, d, h, w), dtype=f32, device=z.device) if want_z_q else None
    rc = _lib.load().cfhip_vq_nearest(z.data_ptr(), int(z.dtype == f32), cl, codebook.data_ptr(), code_sq.data_ptr(), indices.data_ptr(),
                                      _p(z_q), b, d, h * w, n, float(scale_factor), _stream())
    _lib.check(rc, "vq_nearest")
    return indices, z_q


TOME_MAX_CHANNELS = _H["CFHIP_TOME_MAX_CHANNELS"]
TOME_MAX_TOKENS = _H["CFHIP_TOME_MAX_TOKENS"]


def _tome_tokens(x: Tensor, name: str, who: str) -> Tuple[int, int, int]:
    """x bf16 [B, N, C] contiguous within the limits of csrc/tome.hip, checked before any launch"""
    _need(x, bf16, name)
    if x.dim() != 3 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"cfhip {who}: `{name}` must be a non-empty contiguous [B, N, C], got {tuple(x.shape)}")
    b, n, c = x.shape
    if c % 8 != 0 or not 8 <= c <= TOME_MAX_CHANNELS:
        raise NotImplementedError(f"cfhip {who}: C = {c} is outside the token-merging kernels (C % 8 == 0, 8 <= C <= {TOME_MAX_CHANNELS})")
    if n > TOME_MAX_TOKENS or b > 65535:
        raise NotImplementedError(f"cfhip {who}: B = {b}, N = {n} is outside the token-merging kernels (N <= {TOME_MAX_TOKENS}, B <= 65535)")
    return b, n, c


def _tome_table(t: Tensor, shape: Tuple[int, ...], name: str, who: str) -> None:
    _need(t, torch.int32, name)
    if tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"cfhip {who}: `{name}` must be a contiguous int32 {list(shape)}, got {tuple(t.shape)}")


def _tome_split(src_idx: Tensor, dst_idx: Tensor, n: int, who: str) -> Tuple[int, int]:
    n_src, n_dst = src_idx.numel(), dst_idx.numel()
    _tome_table(src_idx, (n_src,), "src_idx", who)
    _tome_table(dst_idx, (n_dst,), "dst_idx", who)
    if n_src < 1 or n_dst < 1 or n_src + n_dst != n:
        raise ValueError(f"cfhip {who}: {n_src} src + {n_dst} dst tokens do not split N = {n}")
    return n_src, n_dst


def tome_match(x: Tensor, src_idx: Tensor, dst_idx: Tensor) -> Tuple[Tensor, Tensor]:
    """(node_max f32 [B, n_src], node_idx int32 [B, n_src]) (cfhip_tome_match): per src token the largest cosine to a dst token and
    the lowest dst position that has it.  x bf16 [B, N, C]; src_idx / dst_idx int32 token ids of the split.  The [B, n_src, n_dst]
    matrix is never formed; the workspace is one f32 per token."""
    b, n, c = _tome_tokens(x, "x", "tome_match")
    n_src, n_dst = _tome_split(src_idx, dst_idx, n, "tome_match")
    rinv = torch.empty((b, n), dtype=f32, device=x.device)
    node_max = torch.empty((b, n_src), dtype=f32, device=x.device)
    node_idx = torch.empty((b, n_src), dtype=torch.int32, device=x.device)
    rc = _lib.load().cfhip_tome_match(x.data_ptr(), src_idx.data_ptr(), dst_idx.data_ptr(), rinv.data_ptr(), node_max.data_ptr(),
                                      node_idx.data_ptr(), b, n, c, n_src, n_dst, _stream())
    _lib.check(rc, "tome_match")
    return node_max, node_idx


def tome_select(node_max: Tensor, node_idx: Tensor, src_idx: Tensor, dst_idx: Tensor, r: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(row_of_token int32 [B, N], token_of_row int32 [B, N - r], member_off int32 [B, n_dst + 1], members int32 [B, r])
    (cfhip_tome_select): the r src rows with the largest node_max (ties: lowest position) are merged into their node_idx; merged rows
    are [unmerged src, ascending token | dst, ascending token]; members[member_off[j]:member_off[j + 1]] = the tokens merged into
    dst j, ascending."""
    _need(node_max, f32, "node_max")
    if node_max.dim() != 2 or not node_max.is_contiguous():
        raise ValueError("cfhip tome_select: `node_max` must be a contiguous f32 [B, n_src]")
    b = node_max.shape[0]
    n_src, n_dst = _tome_split(src_idx, dst_idx, src_idx.numel() + dst_idx.numel(), "tome_select")
    n = n_src + n_dst
    _tome_table(node_idx, (b, n_src), "node_idx", "tome_select")
    if tuple(node_max.shape) != (b, n_src):
        raise ValueError(f"cfhip tome_select: `node_max` is {tuple(node_max.shape)}, the split has {n_src} src tokens")
    if n > TOME_MAX_TOKENS or not 1 <= b <= 65535:
        raise NotImplementedError(f"cfhip tome_select: B = {b}, N = {n} is outside the token-merging kernels")
    r = int(r)
    if not 1 <= r <= n_src:
        raise ValueError(f"cfhip tome_select: r = {r} outside [1, n_src = {n_src}]")
    dev = node_max.device
    row_of_token = torch.empty((b, n), dtype=torch.int32, device=dev)
    token_of_row = torch.empty((b, n - r), dtype=torch.int32, device=dev)
    member_off = torch.empty((b, n_dst + 1), dtype=torch.int32, device=dev)
    members = torch.empty((b, r), dtype=torch.int32, device=dev)
    cursor = torch.empty((b, n_dst), dtype=torch.int32, device=dev)
    rc = _lib.load().cfhip_tome_select(node_max.data_ptr(), node_idx.data_ptr(), src_idx.data_ptr(), dst_idx.data_ptr(),
                                       row_of_token.data_ptr(), token_of_row.data_ptr(), member_off.data_ptr(), members.data_ptr(),
                                       cursor.data_ptr(), b, n, n_src, n_dst, r, _stream())
    _lib.check(rc, "tome_select")
    return row_of_token, token_of_row, member_off, members


def tome_merge(x: Tensor, token_of_row: Tensor, member_off: Tensor, members: Tensor) -> Tensor:
    """bf16 [B, N - r, C] (cfhip_tome_merge) from x bf16 [B, N, C] and the tables of `tome_select`: an unmerged row is a copy, a dst
    row (dst + sum of its members) / (1 + count), f32, members in ascending token order, one rounding"""
    b, n, c = _tome_tokens(x, "x", "tome_merge")
    r = members.shape[-1]
    n_dst = member_off.shape[-1] - 1
    n_src = n - n_dst
    if not 1 <= r <= n_src or n_dst < 1:
        raise ValueError(f"cfhip tome_merge: tables of r = {r}, n_dst = {n_dst} do not fit N = {n}")
    _tome_table(token_of_row, (b, n - r), "token_of_row", "tome_merge")
    _tome_table(member_off, (b, n_dst + 1), "member_off", "tome_merge")
    _tome_table(members, (b, r), "members", "tome_merge")
    out = torch.empty((b, n - r, c), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_tome_merge(x.data_ptr(), token_of_row.data_ptr(), member_off.data_ptr(), members.data_ptr(), out.data_ptr(),
                                      b, n, c, n_src, n_dst, r, _stream())
    _lib.check(rc, "tome_merge")
    return out


def tome_unmerge_add(y: Tensor, row_of_token: Tensor, residual: Optional[Tensor] = None, *, out_f32: bool = False) -> Tensor:
    """[B, N, C] (cfhip_tome_unmerge_add): out[b, t] = residual[b, t] + y[b, row_of_token[b, t]], one f32 add and one rounding, in the
    residual's dtype (bf16 or f32); without a residual the plain unmerge, f32 with `out_f32`, else bf16.  y bf16 [B, N - r, C]."""
    b, rows, c = _tome_tokens(y, "y", "tome_unmerge_add")
    n = row_of_token.shape[-1]
    _tome_table(row_of_token, (b, n), "row_of_token", "tome_unmerge_add")
    if not rows < n <= TOME_MAX_TOKENS:
        raise ValueError(f"cfhip tome_unmerge_add: {rows} merged rows do not come from N = {n} tokens")
    if residual is not None:
        if not residual.is_cuda or residual.dtype not in (bf16, f32):
            raise TypeError(f"cfhip tome_unmerge_add: `residual` must be {bf16} or {f32} on the HIP device")
        if tuple(residual.shape) != (b, n, c) or not residual.is_contiguous():
            raise ValueError(f"cfhip tome_unmerge_add: `residual` must be a contiguous [{b}, {n}, {c}], got {tuple(residual.shape)}")
        out_f32 = residual.dtype == f32
    out = torch.empty((b, n, c), dtype=f32 if out_f32 else bf16, device=y.device)
    rc = _lib.load().cfhip_tome_unmerge_add(y.data_ptr(), row_of_token.data_ptr(), _p(residual), out.data_ptr(), int(out_f32), b, n, c,
                                            n - rows, _stream())
    _lib.check(rc, "tome_unmerge_add")
    return out


def _sample_step_operands(who: str, row: int, x: Tensor, xin: Tensor, out_c: Tensor, table: Tensor, k: Tensor, out_u: Optional[Tensor],
                          noise: Optional[Tensor], aux: Optional[Tensor] = None) -> Tuple[int, int, int, int, int]:
    """What `diffusion_sample_step` and `k_sample_step` (`who`) both require of their operands -> (B, n = C H W, B n, the
    table's rows, the copies of the state `xin` holds)"""
    _need(x, f32, "x")
    _need(xin, bf16, "xin")
    _need(out_c, bf16, "out_c")
    _need(table, f32, "table")
    _need(k, torch.int32, "k")
    for t_, nm in ((x, "x"), (xin, "xin"), (out_c, "out_c"), (table, "table")):
        if not t_.is_contiguous():
            raise ValueError(f"cfhip {who}: `{nm}` must be contiguous")
    b = x.shape[0]
    total = x.numel()
    n = total // b
    if n % 4 != 0:
        raise ValueError(f"cfhip {who}: C * H * W = {n} must be a multiple of 4")
    if out_c.numel() != total:
        raise ValueError(f"cfhip {who}: `out_c` must have the state's size")
    for t_, nm, dt in ((out_u, "out_u", bf16), (aux, "aux", f32)):
        if t_ is not None:
            _need(t_, dt, nm)
            if t_.numel() != total or not t_.is_contiguous():
                raise ValueError(f"cfhip {who}: `{nm}` must be contiguous with the state's size")
    if xin.numel() not in (total, 2 * total):
        raise ValueError(f"cfhip {who}: `xin` must hold one or two copies of the state")
    if table.dim() != 2 or table.shape[1] != row or table.shape[0] < 1:
        raise ValueError(f"cfhip {who}: table must be [rows, {row}]")
    rows = table.shape[0]
    if k.numel() != 1:
        raise ValueError(f"cfhip {who}: `k` is one int32 counter")
    if noise is not None:
        _need(noise, f32, "noise")
        if noise.numel() != rows * total or not noise.is_contiguous():
            raise ValueError(f"cfhip {who}: the noise bank must be contiguous [{rows}, {b}, ...] f32")
    return b, n, total, rows, xin.numel() // total


def diffusion_sample_step(x: Tensor, xin: Tensor, out_c: Tensor, table: Tensor, k: Tensor, *, kind: str, parameterization: str,
                          out_u: Optional[Tensor] = None, scale: float = 1.0, noise: Optional[Tensor] = None,
                          temperature: float = 1.0, clip_last: bool = False, seed: int = 0, offset: int = 0) -> None:
    """One reverse step in place on the f32 state x [B, ...]: reads row k[0] of `table` ([steps, SAMPLE_ROW] f32), the bf16
    model output(s) and the noise (bank [steps, B, ...] f32, or Philox at (seed, offset + k B n / 4 + i / 4)); writes x and
    xin (bf16 [B, ...] or [2B, ...]: the next UNet input, both halves when guidance runs one 2B-batch forward)."""
    if kind not in SAMPLERS:
        raise ValueError(f"cfhip diffusion_sample_step: unrecognized sampler '{kind}'")
    if parameterization not in PARAMETERIZATIONS:
        raise ValueError(f"cfhip diffusion_sample_step: unrecognized parameterization '{parameterization}'")
    b, n, total, steps, dup = _sample_step_operands("diffusion_sample_step", SAMPLE_ROW, x, xin, out_c, table, k, out_u, noise)
    rc = _lib.load().cfhip_diffusion_sample_step(
        x.data_ptr(), xin.data_ptr(), out_c.data_ptr(), _p(out_u), float(scale), table.data_ptr(), steps, k.data_ptr(),
        _p(noise), b, n, SAMPLERS[kind], PARAMETERIZATIONS[parameterization], float(temperature), int(bool(clip_last)),
        dup, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _stream())
    _lib.check(rc, "diffusion_sample_step")


def diffusion_sample_advance(k: Tensor, table: Tensor, timesteps: Tensor) -> None:
    """k += 1 and timesteps[:] = table[k, 0] (while k is a row of the table), on the device"""
    _need(k, torch.int32, "k")
    _need(table, f32, "table")
    _need(timesteps, torch.int64, "timesteps")
    if table.dim() != 2 or table.shape[1] != SAMPLE_ROW or not table.is_contiguous() or not timesteps.is_contiguous():
        raise ValueError(f"cfhip diffusion_sample_advance: a contiguous [steps, {SAMPLE_ROW}] table and timesteps expected")
    _lib.check(_lib.load().cfhip_diffusion_sample_advance(k.data_ptr(), table.data_ptr(), table.shape[0], timesteps.data_ptr(),
                                                          timesteps.numel(), _stream()), "diffusion_sample_advance")


def k_sample_step(x: Tensor, aux: Optional[Tensor], xin: Tensor, out_c: Tensor, table: Tensor, k: Tensor, *, kind: str,
                  parameterization: str, out_u: Optional[Tensor] = None, scale: float = 1.0, noise: Optional[Tensor] = None,
                  clip_last: bool = False, seed: int = 0, offset: int = 0) -> None:
    """One model evaluation of a sigma-space sampler ("k_euler_a" | "k_heun" | "k_dpmpp_2m") in place on the f32 state x [B, ...]:
    reads row k[0] of `table` ([rows, KSAMPLE_ROW] f32, one row per evaluation), the bf16 model output(s), the f32 `aux` of x's
    size (heun's d between its stages, dpmpp_2m's old_denoised; None for euler_a) and, for euler_a, the noise (bank [rows, B, ...]
    f32, or Philox at (seed, offset + k B n / 4 + i / 4)); writes x, aux and xin (bf16 [B, ...] or [2B, ...]: the next UNet input
    times its c_in)."""
    if kind not in KSAMPLERS:
        raise ValueError(f"cfhip k_sample_step: unrecognized sampler '{kind}'")
    if parameterization not in ("eps", "v"):
        raise ValueError("only `v` / `eps` parameterization is supported in `k_samplers`")
    if kind != "k_euler_a":
        if aux is None:
            raise ValueError(f"cfhip k_sample_step: '{kind}' needs the auxiliary buffer")
        if noise is not None:
            raise ValueError(f"cfhip k_sample_step: '{kind}' draws no noise")
    b, n, total, rows, dup = _sample_step_operands("k_sample_step", KSAMPLE_ROW, x, xin, out_c, table, k, out_u, noise, aux)
    rc = _lib.load().cfhip_k_sample_step(
        x.data_ptr(), _p(aux), xin.data_ptr(), out_c.data_ptr(), _p(out_u), float(scale), table.data_ptr(), rows, k.data_ptr(),
        _p(noise), b, n, KSAMPLERS[kind], PARAMETERIZATIONS[parameterization], int(bool(clip_last)), dup,
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _stream())
    _lib.check(rc, "k_sample_step")


def k_sample_advance(k: Tensor, table: Tensor, timesteps: Tensor) -> None:
    """k += 1 and timesteps[:] = table[k, 0] (while k is a row of the table), on the device; timesteps f32 (fractional) or int64"""
    _need(k, torch.int32, "k")
    _need(table, f32, "table")
    if timesteps.dtype not in (f32, torch.int64) or not timesteps.is_cuda:
        raise TypeError("cfhip k_sample_advance: timesteps must be f32 or int64 on the device")
    if table.dim() != 2 or table.shape[1] != KSAMPLE_ROW or not table.is_contiguous() or not timesteps.is_contiguous():
        raise ValueError(f"cfhip k_sample_advance: a contiguous [rows, {KSAMPLE_ROW}] table and timesteps expected")
    _lib.check(_lib.load().cfhip_k_sample_advance(k.data_ptr(), table.data_ptr(), table.shape[0], timesteps.data_ptr(),
                                                  int(timesteps.dtype == torch.int64), timesteps.numel(), _stream()), "k_sample_advance")


MERGE_NOISE = {k: _H["CFHIP_MERGE_NOISE_" + k.upper()] for k in ("philox", "unified", "bank")}


def _ref_operands(who: str, x: Tensor, ref: Tensor, mask: Tensor) -> Tuple[int, int, int]:
    """What the `_ref` entry points require of the reference of the state x [B, C, H, W]: ref f32 [B, C, H, W], mask f32
    [B or 1, 1 or C, H, W], both contiguous; the mask is not expanded -> (its batch stride, its channel stride, H W)"""
    if x.dim() != 4:
        raise ValueError(f"cfhip {who}: with a reference the state must be [B, C, H, W]")
    _need(ref, f32, "ref")
    _need(mask, f32, "mask")
    b, c, h, w = x.shape
    if tuple(ref.shape) != (b, c, h, w) or not ref.is_contiguous():
        raise ValueError(f"cfhip {who}: `ref` must be a contiguous f32 {[b, c, h, w]}, got {list(ref.shape)}")
    if mask.dim() != 4 or mask.shape[0] not in (1, b) or mask.shape[1] not in (1, c) or tuple(mask.shape[2:]) != (h, w) or not mask.is_contiguous():
        raise ValueError(f"cfhip {who}: `mask` must be a contiguous f32 [{b} or 1, 1 or {c}, {h}, {w}], got {list(mask.shape)}")
    hw = h * w
    cs = hw if mask.shape[1] == c and c > 1 else 0
    bs = 0 if mask.shape[0] == 1 else (c * hw if cs else hw)
    return bs, cs, hw


def _merge_operands(who: str, x: Tensor, side: Tensor, rows: int, merge_noise: Optional[Tensor], merge_noise_mode: str,
                    merge_row0: int) -> int:
    """the side table and the merge noise of a DDIM / basic launch with a reference -> the noise mode's code"""
    if merge_noise_mode not in MERGE_NOISE:
        raise ValueError(f"cfhip {who}: merge noise mode '{merge_noise_mode}' (philox | unified | bank)")
    _need(side, f32, "side")
    if tuple(side.shape) != (rows, 2) or not side.is_contiguous():
        raise ValueError(f"cfhip {who}: the side table must be a contiguous f32 [{rows}, 2], got {list(side.shape)}")
    if not 0 <= int(merge_row0) < rows:
        raise ValueError(f"cfhip {who}: merge_row0 = {merge_row0} outside [0, {rows})")
    if (merge_noise is None) != (merge_noise_mode == "philox"):
        raise ValueError(f"cfhip {who}: `merge_noise` goes with the unified and bank modes (and only with them)")
    if merge_noise is not None:
        _need(merge_noise, f32, "merge_noise")
        want = x.numel() * (rows - int(merge_row0) if merge_noise_mode == "bank" else 1)
        if merge_noise.numel() != want or not merge_noise.is_contiguous():
            raise ValueError(f"cfhip {who}: `merge_noise` must be a contiguous f32 " +
                             (f"[{rows - int(merge_row0)}, B, ...] bank" if merge_noise_mode == "bank" else "tensor of the state's shape"))
    return MERGE_NOISE[merge_noise_mode]


def diffusion_sample_step_ref(x: Tensor, xin: Tensor, out_c: Tensor, table: Tensor, k: Tensor, *, ref: Tensor, mask: Tensor, side: Tensor,
                              kind: str, parameterization: str, out_u: Optional[Tensor] = None, scale: float = 1.0,
                              noise: Optional[Tensor] = None, temperature: float = 1.0, clip_last: bool = False, seed: int = 0,
                              offset: int = 0, merge_noise: Optional[Tensor] = None, merge_noise_mode: str = "philox",
                              merge_row0: int = 0) -> None:
    """`diffusion_sample_step` with a reference (cfhip_diffusion_sample_step_ref): after row k < rows - 1 the new state is merged
    with the noised reference as the reference sampler does at the top of step k + 1, x = mask * (side[k + 1, 0] * ref +
    side[k + 1, 1] * nz) + (1 - mask) * x.  ref f32 [B, C, H, W]; mask f32 [B or 1, 1 or C, H, W] (not expanded); side f32 [rows, 2];
    nz: Philox at (seed, offset + (rows + k + 1) B n / 4 + i / 4) ("philox"), `merge_noise` [B, C, H, W] for every merge
    ("unified"), or entry k + 1 - merge_row0 of the bank `merge_noise` [rows - merge_row0, B, C, H, W] ("bank")."""
    who = "diffusion_sample_step_ref"
    if kind not in SAMPLERS:
        raise ValueError(f"cfhip {who}: unrecognized sampler '{kind}'")
    if parameterization not in PARAMETERIZATIONS:
        raise ValueError(f"cfhip {who}: unrecognized parameterization '{parameterization}'")
    b, n, total, steps, dup = _sample_step_operands(who, SAMPLE_ROW, x, xin, out_c, table, k, out_u, noise)
    bs, cs, hw = _ref_operands(who, x, ref, mask)
    mode = _merge_operands(who, x, side, steps, merge_noise, merge_noise_mode, merge_row0)
    rc = _lib.load().cfhip_diffusion_sample_step_ref(
        x.data_ptr(), xin.data_ptr(), out_c.data_ptr(), _p(out_u), float(scale), table.data_ptr(), steps, k.data_ptr(),
        _p(noise), b, n, SAMPLERS[kind], PARAMETERIZATIONS[parameterization], float(temperature), int(bool(clip_last)),
        dup, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, ref.data_ptr(), mask.data_ptr(), bs, cs, hw,
        side.data_ptr(), _p(merge_noise), mode, int(merge_row0), _stream())
    _lib.check(rc, who)


def diffusion_sample_merge(x: Tensor, xin: Tensor, k: Tensor, *, ref: Tensor, mask: Tensor, side: Tensor, seed: int = 0, offset: int = 0,
                           merge_noise: Optional[Tensor] = None, merge_noise_mode: str = "philox", merge_row0: int = 0) -> None:
    """The merge in front of row k[0] on its own (cfhip_diffusion_sample_merge), in place on the f32 state x [B, C, H, W]; xin
    (bf16, one or two copies) = the merged state.  Operands as `diffusion_sample_step_ref`; a k outside [merge_row0, rows) is a no-op."""
    who = "diffusion_sample_merge"
    _need(x, f32, "x")
    _need(xin, bf16, "xin")
    _need(k, torch.int32, "k")
    if not x.is_contiguous() or not xin.is_contiguous():
        raise ValueError(f"cfhip {who}: `x` and `xin` must be contiguous")
    b, total = x.shape[0], x.numel()
    n = total // b
    if n % 4 != 0:
        raise ValueError(f"cfhip {who}: C * H * W = {n} must be a multiple of 4")
    if xin.numel() not in (total, 2 * total):
        raise ValueError(f"cfhip {who}: `xin` must hold one or two copies of the state")
    if k.numel() != 1:
        raise ValueError(f"cfhip {who}: `k` is one int32 counter")
    if side.dim() != 2:
        raise ValueError(f"cfhip {who}: the side table must be [rows, 2]")
    rows = side.shape[0]
    bs, cs, hw = _ref_operands(who, x, ref, mask)
    mode = _merge_operands(who, x, side, rows, merge_noise, merge_noise_mode, merge_row0)
    rc = _lib.load().cfhip_diffusion_sample_merge(
        x.data_ptr(), xin.data_ptr(), rows, k.data_ptr(), b, n, xin.numel() // total, int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(offset) & 0xFFFFFFFFFFFFFFFF, ref.data_ptr(), mask.data_ptr(), bs, cs, hw, side.data_ptr(), _p(merge_noise), mode,
        int(merge_row0), _stream())
    _lib.check(rc, who)


def k_sample_step_ref(x: Tensor, aux: Optional[Tensor], xin: Tensor, out_c: Tensor, table: Tensor, k: Tensor, *, ref: Tensor, mask: Tensor,
                      kind: str, parameterization: str, out_u: Optional[Tensor] = None, scale: float = 1.0,
                      noise: Optional[Tensor] = None, clip_last: bool = False, seed: int = 0, offset: int = 0) -> None:
    """`k_sample_step` with a reference (cfhip_k_sample_step_ref): every evaluation's denoised value becomes mask * ref +
    (1 - mask) * denoised before the rule uses it (dpmpp_2m keeps the merged value in aux).  ref f32 [B, C, H, W]; mask f32
    [B or 1, 1 or C, H, W] (not expanded)."""
    who = "k_sample_step_ref"
    if kind not in KSAMPLERS:
        raise ValueError(f"cfhip {who}: unrecognized sampler '{kind}'")
    if parameterization not in ("eps", "v"):
        raise ValueError("only `v` / `eps` parameterization is supported in `k_samplers`")
    if kind != "k_euler_a":
        if aux is None:
            raise ValueError(f"cfhip {who}: '{kind}' needs the auxiliary buffer")
        if noise is not None:
            raise ValueError(f"cfhip {who}: '{kind}' draws no noise")
    b, n, total, rows, dup = _sample_step_operands(who, KSAMPLE_ROW, x, xin, out_c, table, k, out_u, noise, aux)
    bs, cs, hw = _ref_operands(who, x, ref, mask)
    rc = _lib.load().cfhip_k_sample_step_ref(
        x.data_ptr(), _p(aux), xin.data_ptr(), out_c.data_ptr(), _p(out_u), float(scale), table.data_ptr(), rows, k.data_ptr(),
        _p(noise), b, n, KSAMPLERS[kind], PARAMETERIZATIONS[parameterization], int(bool(clip_last)), dup,
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, ref.data_ptr(), mask.data_ptr(), bs, cs, hw, _stream())
    _lib.check(rc, who)


def diffusion_loss(pred: Tensor, target: Tensor, weight: Tensor, loss_type: str = "l2", want_grad: bool = True):
    """DDPMStep.loss_fn's per-sample objective: returns (per_sample f32 [B] = mean_inner f(pred - target), dpred bf16 =
    weight[b] * f' / inner); f = square ("l2") or abs ("l1")."""
    _need(pred, bf16, "pred")
    _need(target, f32, "target")
    _need(weight, f32, "weight")
    if loss_type not in ("l1", "l2"):
        raise ValueError(f"unrecognized loss '{loss_type}' occurred")
    pred, target, weight = pred.contiguous(), target.contiguous(), weight.contiguous()
    b = pred.shape[0]
    if weight.numel() != b or target.numel() != pred.numel():
        raise ValueError("cfhip diffusion_loss: shapes differ")
    per_sample = torch.zeros((b,), dtype=f32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    rc = _lib.load().cfhip_diffusion_loss(pred.data_ptr(), target.data_ptr(), weight.data_ptr(), per_sample.data_ptr(),
                                          _p(dpred), b, pred.numel() // b, 1 if loss_type == "l1" else 0, _stream())
    _lib.check(rc, "diffusion_loss")
    return per_sample, dpred


# ---------------------------------------------------------------------------------------------
# A12: dropout / DropPath (csrc/random.hip).  The generator state is (seed, offset): every call that draws random bits
# advances `offset` by the number of Philox counters it consumed, so that no two calls share bits and a backward pass
# can regenerate its mask from the (seed, offset) pair the forward recorded.
# ---------------------------------------------------------------------------------------------


class PhiloxState:
    """Process-wide counter-based generator state.  The stream starts from `torch.initial_seed()` + the rank of the process
    (so `torch.manual_seed` / the reference's `seed_everything` before the first draw seed it, and data-parallel ranks
    draw different masks); `manual_seed` (re)starts it explicitly.  (seed, offset) travel to the kernels as launch
    ARGUMENTS: a captured hipGraph would replay one frozen pair — the same masks every step — so drawing while a
    stream is capturing is an error (run stochastic modules eagerly: `TrainStep(use_graph=False)`)."""

    seed: Optional[int] = None  # None: derived from torch.initial_seed() + RANK at the first draw
    offset: int = 0

    @classmethod
    def manual_seed(cls, seed: int) -> None:
        cls.seed, cls.offset = int(seed) & 0xFFFFFFFFFFFFFFFF, 0

    @classmethod
    def take(cls, counters: int) -> Tuple[int, int]:
        """Reserve `counters` Philox counters; returns the (seed, offset) to hand to the kernel."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("cfhip: a dropout / DropPath mask was drawn during hipGraph capture: the (seed, offset) pair "
                               "would be frozen into the graph and every replay would apply the same mask; run models with "
                               "dropout or drop_path eagerly (TrainStep(use_graph=False))")
        if cls.seed is None:
            import os

            cls.seed = (torch.initial_seed() + 0x9E3779B97F4A7C15 * (int(os.environ.get("RANK", "0")) + 1)) & 0xFFFFFFFFFFFFFFFF
        off = cls.offset
        cls.offset += int(counters)
        return cls.seed, off


def dropout(x: Tensor, p: float, *, seed: int = 0, offset: int = 0, mask: Optional[Tensor] = None,
            want_mask: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """y = keep ? x / (1 - p) : 0 (bf16 or f32, any shape).  `mask` (uint8, same number of elements) injects the keep
    mask instead of the Philox stream keyed by (seed, offset).  Returns (y, mask_out or None)."""
    if x.dtype not in (bf16, f32):
        raise TypeError(f"cfhip dropout: x must be bf16 or f32, got {x.dtype}")
    _need(x, x.dtype, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    if mask is not None:
        _need(mask, torch.uint8, "mask")
        if mask.numel() != x.numel():
            raise ValueError("cfhip dropout: mask must have one byte per element of x")
        mask = mask.contiguous()
    mask_out = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_mask else None
    rc = _lib.load().cfhip_dropout(x.data_ptr(), y.data_ptr(), int(x.dtype == f32), x.numel(), float(p), int(seed),
                                   int(offset), _p(mask), _p(mask_out), _stream())
    _lib.check(rc, "dropout")
    return y, mask_out


def drop_path_mask(batch: int, keep_prob: float, device: torch.device, *, seed: int = 0, offset: int = 0) -> Tensor:
    """mask[b] = floor(keep_prob + u_b) in {0, 1} (f32 [B]) — reference customs.py:439-441"""
    out = torch.empty((batch,), dtype=f32, device=device)
    rc = _lib.load().cfhip_drop_path_mask(out.data_ptr(), batch, float(keep_prob), int(seed), int(offset), _stream())
    _lib.check(rc, "drop_path_mask")
    return out


def drop_path(x: Tensor, mask: Tensor, keep_prob: float) -> Tensor:
    """y[b] = (x[b] / keep_prob) * mask[b] for a [B, ...] tensor (bf16 or f32); also its own backward on dy."""
    if x.dtype not in (bf16, f32):
        raise TypeError(f"cfhip drop_path: x must be bf16 or f32, got {x.dtype}")
    _need(x, x.dtype, "x")
    _need(mask, f32, "mask")
    x = x.contiguous()
    b = x.shape[0]
    if mask.numel() != b:
        raise ValueError("cfhip drop_path: one mask value per sample")
    y = torch.empty_like(x)
    rc = _lib.load().cfhip_drop_path(x.data_ptr(), y.data_ptr(), int(x.dtype == f32), mask.contiguous().data_ptr(),
                                     float(keep_prob), b, x.numel() // b, _stream())
    _lib.check(rc, "drop_path")
    return y


# ---------------------------------------------------------------------------------------------
# LoRA adapters of Linear layers (csrc/lora.hip): skinny product, rank-r update in place, tall reduction.  `p`, `seed`,
# `offset`: the keep mask of `dropout` over the contiguous index space of the wide tensor, regenerated inside the kernels.
# ---------------------------------------------------------------------------------------------

LORA_MAX_RANK = 64


def _lora_wide(t: Tensor, name: str, stride_mult: int = 8) -> Tuple[int, int, int]:
    """rows, columns, row stride of a wide operand: 2-D, columns a multiple of 8, 16-byte aligned"""
    rows, cols, ld = _mat(t, name)
    if rows < 1 or cols % 8 != 0 or cols < 8 or (ld % stride_mult != 0 and rows > 1) or t.data_ptr() % 16 != 0:
        raise ValueError(f"cfhip lora: `{name}` must be 16-byte aligned [rows, cols] with cols % 8 == 0 and a row stride that is "
                         f"a multiple of {stride_mult}, got {tuple(t.shape)} / {t.stride()}")
    return rows, cols, ld if rows > 1 else cols  # (the stride of a single row is never used)


def _lora_factor(f: Tensor, wide: int, wide_first: bool, name: str) -> Tuple[int, int]:
    """rank and leading dimension of a factor [r, wide] (wide_first False) or [wide, r] (True), bf16"""
    _need(f, bf16, name)
    a, b, ld = _mat(f, name)
    r, w = (b, a) if wide_first else (a, b)
    if w != wide:
        raise ValueError(f"cfhip lora: `{name}` {tuple(f.shape)} does not match the wide dimension {wide}")
    if not 1 <= r <= LORA_MAX_RANK:
        raise ValueError(f"cfhip lora: rank {r} outside 1 .. {LORA_MAX_RANK}")
    return r, ld


def _lora_thin(h: Tensor, rows: int, r: int, name: str) -> None:
    _need(h, bf16, name)
    if tuple(h.shape) != (rows, r) or not h.is_contiguous():
        raise ValueError(f"cfhip lora: `{name}` must be a contiguous bf16 [{rows}, {r}], got {tuple(h.shape)} / {h.stride()}")


def _lora_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"cfhip lora: p = {p} must be in [0, 1)")
    return p


def lora_down(x: Tensor, f: Tensor, *, f_trans: bool = False, scale: float = 1.0, p: float = 0.0, seed: int = 0,
              offset: int = 0) -> Tensor:
    """h [M, r] (bf16) = scale * (mask . x) F^T.  x bf16 [M, K] (row stride allowed); f = [r, K] (forward: lora_down.weight), or
    [K, r] with `f_trans` (backward: x = dy, f = lora_up.weight, the mask of the forward's (p, seed, offset))."""
    _need(x, bf16, "x")
    m, k, ldx = _lora_wide(x, "x")
    r, ldf = _lora_factor(f, k, f_trans, "f")
    if not f_trans and (ldf % 8 != 0 or f.data_ptr() % 16 != 0):
        raise ValueError("cfhip lora_down: the [r, K] factor must be 16-byte aligned with a row stride that is a multiple of 8")
    h = torch.empty((m, r), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_lora_down(x.data_ptr(), f.data_ptr(), h.data_ptr(), m, k, r, ldx, ldf, int(f_trans), float(scale),
                                     _lora_p(p), int(seed), int(offset), _stream())
    _lib.check(rc, "lora_down")
    return h


def lora_up_add(y: Tensor, h: Tensor, f: Tensor, *, f_trans: bool = False, scale: float = 1.0, p: float = 0.0, seed: int = 0,
                offset: int = 0) -> Tensor:
    """y [M, N] (bf16 or f32, in place) += scale * mask . (h F^T).  f = [N, r] (forward: lora_up.weight), or [r, N] with `f_trans`
    (backward: y = the base GEMM's dX, h = dh, f = lora_down.weight).  Dropped positions keep their bits."""
    if y.dtype not in (bf16, f32):
        raise TypeError(f"cfhip lora_up_add: y must be bf16 or f32, got {y.dtype}")
    _need(y, y.dtype, "y")
    m, n, ldy = _lora_wide(y, "y", 4)
    r, ldf = _lora_factor(f, n, not f_trans, "f")
    _lora_thin(h, m, r, "h")
    rc = _lib.load().cfhip_lora_up_add(h.data_ptr(), f.data_ptr(), y.data_ptr(), int(y.dtype == f32), m, n, r, ldf, ldy,
                                       int(f_trans), float(scale), _lora_p(p), int(seed), int(offset), _stream())
    _lib.check(rc, "lora_up_add")
    return y


def lora_wgrad(t: Tensor, u: Tensor, out: Tensor, *, out_trans: bool = False, accumulate: bool = False, scale: float = 1.0,
               p: float = 0.0, seed: int = 0, offset: int = 0) -> Tensor:
    """out (f32) (+)= scale * (mask . t)^T u over the M rows of t bf16 [M, J] and u bf16 [M, r]: out [J, r] (d lora_up.weight: t = dy,
    u = h) or [r, J] with `out_trans` (d lora_down.weight: t = x, u = dh).  Row splits, f32 partials, fixed-order sum: deterministic."""
    _need(t, bf16, "t")
    _need(out, f32, "out")
    m, j, ldt = _lora_wide(t, "t")
    if u.dim() != 2 or not 1 <= u.shape[1] <= LORA_MAX_RANK:
        raise ValueError(f"cfhip lora_wgrad: `u` must be [M, r] with r in 1 .. {LORA_MAX_RANK}, got {tuple(u.shape)}")
    r = u.shape[1]
    _lora_thin(u, m, r, "u")
    if tuple(out.shape) != ((r, j) if out_trans else (j, r)) or not out.is_contiguous():
        raise ValueError(f"cfhip lora_wgrad: `out` must be a contiguous f32 {(r, j) if out_trans else (j, r)}, got {tuple(out.shape)}")
    lib = _lib.load()
    nbytes = lib.cfhip_lora_wgrad_workspace(m, j, r)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=t.device)
    rc = lib.cfhip_lora_wgrad(t.data_ptr(), u.data_ptr(), out.data_ptr(), m, j, r, ldt, int(out_trans), int(accumulate),
                              float(scale), _lora_p(p), int(seed), int(offset), ws.data_ptr(), ws.numel() * 4, _stream())
    _lib.check(rc, "lora_wgrad")
    return out


# LoRA adapters of Conv2d layers: the 3x3 / pad 1 / stride 1 or 2 down factor on NHWC rows (every 1x1 piece is one of the three
# calls above).  `f` is the bf16 [r, C, 3, 3] copy of lora_down.weight in the parameter's own layout.


def lora_conv_out_hw(h: int, w: int, stride: int) -> Tuple[int, int]:
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _lora_conv_factor(f: Tensor, c: int) -> int:
    _need(f, bf16, "f")
    if f.dim() != 4 or tuple(f.shape[1:]) != (c, 3, 3) or not f.is_contiguous():
        raise ValueError(f"cfhip lora_conv: `f` must be a contiguous bf16 [r, {c}, 3, 3], got {tuple(f.shape)} / {f.stride()}")
    r = f.shape[0]
    if not 1 <= r <= LORA_MAX_RANK:
        raise ValueError(f"cfhip lora: rank {r} outside 1 .. {LORA_MAX_RANK}")
    return r


def _lora_conv_geom(b: int, h: int, w: int, stride: int) -> None:
    if min(b, h, w) < 1 or stride not in (1, 2):
        raise ValueError(f"cfhip lora_conv: B = {b}, H = {h}, W = {w} must be positive and the stride 1 or 2, got {stride}")


def lora_conv_down(x: Tensor, f: Tensor, b: int, h: int, w: int, stride: int = 1, *, scale: float = 1.0) -> Tensor:
    """h [B Ho Wo, r] (bf16) = scale * conv3x3(x, f), pad 1, on NHWC rows: x bf16 [B H W, C] (row stride allowed)."""
    _need(x, bf16, "x")
    _lora_conv_geom(b, h, w, stride)
    m, c, ldx = _lora_wide(x, "x")
    if m != b * h * w:
        raise ValueError(f"cfhip lora_conv_down: `x` has {m} rows, B H W = {b * h * w}")
    r = _lora_conv_factor(f, c)
    ho, wo = lora_conv_out_hw(h, w, stride)
    out = torch.empty((b * ho * wo, r), dtype=bf16, device=x.device)
    rc = _lib.load().cfhip_lora_conv_down(x.data_ptr(), f.data_ptr(), out.data_ptr(), b, h, w, c, r, stride, ldx, float(scale), _stream())
    _lib.check(rc, "lora_conv_down")
    return out


def lora_conv_dx(dh: Tensor, f: Tensor, b: int, h: int, w: int, stride: int = 1, *, out: Optional[Tensor] = None,
                 accumulate: bool = False) -> Tensor:
    """dx [B H W, C] (bf16) (+)= the transposed 3x3 convolution of dh bf16 [B Ho Wo, r] with f.  `out` (row stride allowed) is
    written, or with `accumulate` updated in one read-modify-write pass (the base convolution's dX); without it a new matrix."""
    _lora_conv_geom(b, h, w, stride)
    if f.dim() != 4:
        raise ValueError(f"cfhip lora_conv_dx: `f` must be [r, C, 3, 3], got {tuple(f.shape)}")
    c = f.shape[1]
    r = _lora_conv_factor(f, c)
    ho, wo = lora_conv_out_hw(h, w, stride)
    _lora_thin(dh, b * ho * wo, r, "dh")
    if out is None:
        if accumulate:
            raise ValueError("cfhip lora_conv_dx: `accumulate` needs `out`")
        out = torch.empty((b * h * w, c), dtype=bf16, device=dh.device)
    _need(out, bf16, "out")
    m, c2, lddx = _lora_wide(out, "out")
    if (m, c2) != (b * h * w, c):
        raise ValueError(f"cfhip lora_conv_dx: `out` must be [{b * h * w}, {c}], got {tuple(out.shape)}")
    rc = _lib.load().cfhip_lora_conv_dx(dh.data_ptr(), f.data_ptr(), out.data_ptr(), b, h, w, c, r, stride, lddx, int(accumulate), _stream())
    _lib.check(rc, "lora_conv_dx")
    return out


def lora_conv_wgrad(dh: Tensor, x: Tensor, out: Tensor, b: int, h: int, w: int, stride: int = 1, *, accumulate: bool = False,
                    scale: float = 1.0) -> Tensor:
    """out f32 [r, C, 3, 3] (+)= scale * sum over the output pixels m of dh[m][c] * x[neighbour(m, ky, kx)][ci]: d lora_down.weight
    in the parameter's layout.  Row splits, f32 partials, fixed-order sum: deterministic."""
    _need(x, bf16, "x")
    _need(out, f32, "out")
    _lora_conv_geom(b, h, w, stride)
    m, c, ldx = _lora_wide(x, "x")
    if m != b * h * w:
        raise ValueError(f"cfhip lora_conv_wgrad: `x` has {m} rows, B H W = {b * h * w}")
    if dh.dim() != 2 or not 1 <= dh.shape[1] <= LORA_MAX_RANK:
        raise ValueError(f"cfhip lora_conv_wgrad: `dh` must be [B Ho Wo, r] with r in 1 .. {LORA_MAX_RANK}, got {tuple(dh.shape)}")
    r = dh.shape[1]
    ho, wo = lora_conv_out_hw(h, w, stride)
    _lora_thin(dh, b * ho * wo, r, "dh")
    if tuple(out.shape) != (r, c, 3, 3) or not out.is_contiguous():
        raise ValueError(f"cfhip lora_conv_wgrad: `out` must be a contiguous f32 {(r, c, 3, 3)}, got {tuple(out.shape)}")
    lib = _lib.load()
    nbytes = lib.cfhip_lora_conv_wgrad_workspace(b, h, w, c, r, stride)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=f32, device=x.device)
    rc = lib.cfhip_lora_conv_wgrad(dh.data_ptr(), x.data_ptr(), out.data_ptr(), b, h, w, c, r, stride, ldx, int(accumulate),
                                   float(scale), ws.data_ptr(), ws.numel() * 4, _stream())
    _lib.check(rc, "lora_conv_wgrad")
    return out


# ---------------------------------------------------------------------------------------------
# A16: tabular encoder gather (csrc/tabular.hip)
# ---------------------------------------------------------------------------------------------


def ml_encode_fwd(x: Tensor, plan: Tensor, tables: Optional[Tensor], out_dim: int) -> Tensor:
    """x f32 [B, F] -> merged_all f32 [B, out_dim]; `plan` int32 [out_dim, 6] on the device (see include/cfhip.h),
    `tables` int64 device array of embedding-table base pointers (or None when there is no embedding column)."""
    _need(x, f32, "x")
    _need(plan, torch.int32, "plan")
    b, f, xs = _mat(x, "x")
    out = torch.empty((b, out_dim), dtype=f32, device=x.device)
    rc = _lib.load().cfhip_ml_encode_fwd(x.data_ptr(), b, f, xs, plan.data_ptr(), out_dim, _p(tables), out.data_ptr(),
                                         _stream())
    _lib.check(rc, "ml_encode_fwd")
    return out


def ml_encode_indices(x: Tensor, cols: Tensor, dims: Tensor) -> Tensor:
    """int64 [B, K]: the reference's `EncodingResult.indices` (oob -> 0, truncation)"""
    _need(x, f32, "x")
    _need(cols, torch.int32, "cols")
    _need(dims, torch.int32, "dims")
    b, _, xs = _mat(x, "x")
    k = cols.numel()
    out = torch.empty((b, k), dtype=torch.int64, device=x.device)
    rc = _lib.load().cfhip_ml_encode_indices(x.data_ptr(), b, xs, cols.data_ptr(), dims.data_ptr(), k, out.data_ptr(),
                                             _stream())
    _lib.check(rc, "ml_encode_indices")
    return out


def ml_encode_bwd(dout: Tensor, x: Tensor, plan: Tensor, dtables: Optional[Tensor], want_dx: bool) -> Optional[Tensor]:
    _need(dout, f32, "dout")
    _need(x, f32, "x")
    b, f, xs = _mat(x, "x")
    dout = dout.contiguous()
    dx = torch.zeros((b, f), dtype=f32, device=x.device) if want_dx else None
    rc = _lib.load().cfhip_ml_encode_bwd(dout.data_ptr(), x.data_ptr(), b, f, xs, plan.data_ptr(), dout.shape[1],
                                         _p(dtables), _p(dx), _stream())
    _lib.check(rc, "ml_encode_bwd")
    return dx


# ---------------------------------------------------------------------------------------------
# GRU / LSTM recurrence (csrc/rnn.hip)
# ---------------------------------------------------------------------------------------------

RNN_GRU, RNN_LSTM = _H["CFHIP_RNN_GRU"], _H["CFHIP_RNN_LSTM"]
RNN_MAX_HIDDEN = _H["CFHIP_RNN_MAX_HIDDEN"]
RNN_GATES = {RNN_GRU: 3, RNN_LSTM: 4}


def rnn_hidden_ok(h: int) -> bool:
    return h % 8 == 0 and 8 <= h <= RNN_MAX_HIDDEN


def _rnn_cell(cell: int, h: int, who: str) -> int:
    if cell not in RNN_GATES:
        raise ValueError(f"cfhip {who}: unknown cell id {cell} (RNN_GRU = {RNN_GRU}, RNN_LSTM = {RNN_LSTM})")
    if not rnn_hidden_ok(h):
        raise NotImplementedError(f"cfhip {who}: H = {h} is outside the recurrent kernels (H % 8 == 0, 8 <= H <= {RNN_MAX_HIDDEN})")
    return RNN_GATES[cell]


def _rnn_state(t: Optional[Tensor], b: int, h: int, name: str, who: str) -> None:
    if t is not None:
        _need(t, f32, name)
        if tuple(t.shape) != (b, h) or not t.is_contiguous():
            raise ValueError(f"cfhip {who}: `{name}` must be a contiguous f32 [{b}, {h}], got {tuple(t.shape)}")


def _rnn_seq(t: Tensor, b: int, steps: int, h: int, name: str, who: str) -> int:
    """t: f32 [B, T, H] whose rows (b, t) are `ld` apart with ld >= H (a column slice of a contiguous [B, T, ld]) -> ld"""
    _need(t, f32, name)
    if tuple(t.shape) != (b, steps, h) or t.stride(2) != 1 or t.stride(1) < h or t.stride(0) != steps * t.stride(1):
        raise ValueError(f"cfhip {who}: `{name}` must be [{b}, {steps}, {h}] with rows a fixed stride >= {h} apart, got "
                         f"{tuple(t.shape)} / {t.stride()}")
    return t.stride(1)


def rnn_pack(w_hh: Tensor, cell: int) -> Tensor:
    """bf16 1-D (cfhip_rnn_pack): W_hh f32 [G H, H] in MFMA fragment order, for the forward and for the backward product"""
    _need(w_hh, f32, "w_hh")
    if w_hh.dim() != 2 or not w_hh.is_contiguous():
        raise ValueError(f"cfhip rnn_pack: `w_hh` must be a contiguous f32 [G H, H], got {tuple(w_hh.shape)}")
    h = w_hh.shape[1]
    g = _rnn_cell(cell, h, "rnn_pack")
    if w_hh.shape[0] != g * h:
        raise ValueError(f"cfhip rnn_pack: `w_hh` is {tuple(w_hh.shape)}, expected [{g * h}, {h}]")
    lib = _lib.load()
    nbytes = lib.cfhip_rnn_pack_workspace(cell, h)
    packed = torch.empty((nbytes // 2,), dtype=bf16, device=w_hh.device)
    _lib.check(lib.cfhip_rnn_pack(w_hh.data_ptr(), packed.data_ptr(), nbytes, cell, h, _stream()), "rnn_pack")
    return packed


def rnn_fwd(gx: Tensor, packed: Tensor, b_hh: Tensor, cell: int, *, h0: Optional[Tensor] = None, c0: Optional[Tensor] = None,
            y: Optional[Tensor] = None, reverse: bool = False, save: bool = False, want_state: bool = False):
    """(y, hT, cT, saved) (cfhip_rnn_fwd): gx f32 [B, T, G H] contiguous, b_hh f32 [G H]; y f32 [B, T, H], allocated here or the
    caller's (one half of a bidirectional [B, T, 2 H] buffer).  `want_state`: hT (and the LSTM's cT) f32 [B, H], else None.
    `save`: saved = (gates f32 [B, T, 4 H], cseq f32 [B, T, H] or None (GRU), hprev16 bf16 [B, T, H]) for `rnn_bwd`, else None —
    without it the launch writes nothing but y (and the states asked for)."""
    _need(gx, f32, "gx")
    _need(b_hh, f32, "b_hh")
    _need(packed, bf16, "packed")
    if gx.dim() != 3 or not gx.is_contiguous():
        raise ValueError(f"cfhip rnn_fwd: `gx` must be a contiguous f32 [B, T, G H], got {tuple(gx.shape)}")
    if cell not in RNN_GATES:
        raise ValueError(f"cfhip rnn_fwd: unknown cell id {cell}")
    b, steps, gh = gx.shape
    h = gh // RNN_GATES[cell]
    g = _rnn_cell(cell, h, "rnn_fwd")
    lib = _lib.load()
    if g * h != gh or b < 1 or steps < 1 or b_hh.numel() != gh or not b_hh.is_contiguous():
        raise ValueError(f"cfhip rnn_fwd: gx {tuple(gx.shape)} / b_hh {tuple(b_hh.shape)} do not fit a cell of {g} gates")
    if packed.numel() * 2 != lib.cfhip_rnn_pack_workspace(cell, h) or not packed.is_contiguous():
        raise ValueError(f"cfhip rnn_fwd: `packed` is not rnn_pack's output for H = {h}")
    lstm = cell == RNN_LSTM
    _rnn_state(h0, b, h, "h0", "rnn_fwd")
    _rnn_state(c0, b, h, "c0", "rnn_fwd")
    if c0 is not None and not lstm:
        raise ValueError("cfhip rnn_fwd: `c0` belongs to the LSTM")
    if y is None:
        y = torch.empty((b, steps, h), dtype=f32, device=gx.device)
    ldy = _rnn_seq(y, b, steps, h, "y", "rnn_fwd")
    hT = torch.empty((b, h), dtype=f32, device=gx.device) if want_state else None
    cT = torch.empty((b, h), dtype=f32, device=gx.device) if want_state and lstm else None
    gates = cseq = hprev = None
    if save:
        gates = torch.empty((b, steps, 4 * h), dtype=f32, device=gx.device)
        cseq = torch.empty((b, steps, h), dtype=f32, device=gx.device) if lstm else None
        hprev = torch.empty((b, steps, h), dtype=bf16, device=gx.device)
    rc = lib.cfhip_rnn_fwd(gx.data_ptr(), packed.data_ptr(), b_hh.data_ptr(), _p(h0), _p(c0), y.data_ptr(), ldy, _p(hT), _p(cT),
                           _p(gates), _p(cseq), _p(hprev), cell, b, steps, h, int(reverse), _stream())
    _lib.check(rc, "rnn_fwd")
    return y, hT, cT, ((gates, cseq, hprev) if save else None)


def rnn_bwd(dy: Optional[Tensor], packed: Tensor, cell: int, saved, y: Optional[Tensor], *, h0: Optional[Tensor] = None,
            c0: Optional[Tensor] = None, dhT: Optional[Tensor] = None, dcT: Optional[Tensor] = None, reverse: bool = False,
            want_dstate: bool = False):
    """(dgx, dgh, dh0, dc0) (cfhip_rnn_bwd): dy f32 [B, T, H] (rows a fixed stride apart, or None = zero), `saved` and `y` from
    `rnn_fwd(save=True)` with the same h0 / c0 / reverse; dhT / dcT f32 [B, H] or None (zero).  dgx bf16 [B, T, G H] is the gradient
    of gx, dgh that of h W_hh^T + b_hh (the LSTM's is dgx itself); dh0 / dc0 f32 [B, H] with `want_dstate`, else None."""
    gates, cseq, hprev = saved
    _need(gates, f32, "gates")
    _need(packed, bf16, "packed")
    if gates.dim() != 3 or not gates.is_contiguous() or gates.shape[2] % 4:
        raise ValueError(f"cfhip rnn_bwd: `gates` must be a contiguous f32 [B, T, 4 H], got {tuple(gates.shape)}")
    b, steps, h = gates.shape[0], gates.shape[1], gates.shape[2] // 4
    g = _rnn_cell(cell, h, "rnn_bwd")
    lstm = cell == RNN_LSTM
    lib = _lib.load()
    if packed.numel() * 2 != lib.cfhip_rnn_pack_workspace(cell, h) or not packed.is_contiguous():
        raise ValueError(f"cfhip rnn_bwd: `packed` is not rnn_pack's output for H = {h}")
    if lstm:
        if cseq is None:
            raise ValueError("cfhip rnn_bwd: the LSTM needs the saved cell states")
        _need(cseq, f32, "cseq")
        if tuple(cseq.shape) != (b, steps, h) or not cseq.is_contiguous():
            raise ValueError(f"cfhip rnn_bwd: `cseq` must be a contiguous f32 [{b}, {steps}, {h}]")
    elif c0 is not None or dcT is not None:
        raise ValueError("cfhip rnn_bwd: `c0` / `dcT` belong to the LSTM")
    lddy = 0 if dy is None else _rnn_seq(dy, b, steps, h, "dy", "rnn_bwd")
    ldy = 0
    if not lstm and steps > 1:
        if y is None:
            raise ValueError("cfhip rnn_bwd: the GRU reads h_{t-1} from `y`")
        ldy = _rnn_seq(y, b, steps, h, "y", "rnn_bwd")
    else:
        y = None
    for t, name in ((h0, "h0"), (c0, "c0"), (dhT, "dhT"), (dcT, "dcT")):
        _rnn_state(t, b, h, name, "rnn_bwd")
    dgx = torch.empty((b, steps, g * h), dtype=bf16, device=gates.device)
    dgh = None if lstm else torch.empty((b, steps, g * h), dtype=bf16, device=gates.device)
    dh0 = torch.empty((b, h), dtype=f32, device=gates.device) if want_dstate else None
    dc0 = torch.empty((b, h), dtype=f32, device=gates.device) if want_dstate and lstm else None
    rc = lib.cfhip_rnn_bwd(_p(dy), lddy, _p(dhT), _p(dcT), packed.data_ptr(), _p(y), ldy, _p(h0), _p(c0), gates.data_ptr(), _p(cseq),
                           dgx.data_ptr(), _p(dgh), _p(dh0), _p(dc0), cell, b, steps, h, int(reverse), _stream())
    _lib.check(rc, "rnn_bwd")
    return dgx, (dgx if lstm else dgh), dh0, dc0


# ---------------------------------------------------------------------------------------------
# PixelCNN sampling (csrc/pixelcnn.hip)
# ---------------------------------------------------------------------------------------------

PIXELCNN_MAX_CHANNELS = _H["CFHIP_PIXELCNN_MAX_CHANNELS"]
PIXELCNN_MAX_CODES = _H["CFHIP_PIXELCNN_MAX_CODES"]
PIXELCNN_ROWS = 16  # batch rows of one workgroup


def pixelcnn_shape_refusal(latent_channels: int, num_codes: int, num_layers: int) -> Optional[str]:
    """why the sampling kernel refuses this net, or None.  Pure host logic."""
    if latent_channels % 32 != 0 or not 32 <= latent_channels <= PIXELCNN_MAX_CHANNELS:
        return f"latent_channels = {latent_channels} is outside the sampler (a multiple of 32, 32 .. {PIXELCNN_MAX_CHANNELS})"
    if not 2 <= num_codes <= PIXELCNN_MAX_CODES:
        return f"num_codes = {num_codes} is outside the sampler (2 .. {PIXELCNN_MAX_CODES})"
    if num_layers < 1:
        return f"num_layers = {num_layers}"
    return None


def pixelcnn_pack(w2d: Tensor) -> Tensor:
    """bf16 1-D: the f32 / bf16 matrix W [N, K] as the B operand of csrc/pixelcnn.hip — N padded to a multiple of 16 and K to a multiple
    of 32 with zeros; fragment (n, kk), lane l holds W[16 n + (l & 15)][32 kk + 8 (l >> 4) + e], e = 0 .. 7.  Torch indexing only."""
    n, k = w2d.shape
    np_, kp = (n + 15) // 16 * 16, (k + 31) // 32 * 32
    w = torch.zeros((np_, kp), dtype=bf16, device=w2d.device)
    w[:n, :k] = w2d.to(bf16)  # round-to-nearest-even, as the cast kernel behind `functional.shadow_bf16`
    return w.view(np_ // 16, 16, kp // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def pixelcnn_sample(codes: Tensor, label_row: Tensor, in_table: Tensor, in0: Tensor, act: Tensor, packs: Tensor, scale: Tensor,
                    shift: Tensor, head_pack: Tensor, head_bias: Tensor, logits: Tensor, *, first_pixel: int, last_pixel: int,
                    forced: bool, seed: int, offset: int) -> None:
    """one launch of cfhip_pixelcnn_sample over the pixels [first_pixel, last_pixel): `codes` int64 [B, 1, H, W] is written there (or
    read, `forced`), `in0` bf16 [B, H, W, Cin0] and `act` bf16 [L, B, H, W, C] are the state the walk leaves and continues from;
    `logits` f32 [B, H, W, K] keeps every pixel's logits, [B, K] is a scratch.  See include/cfhip.h for the other operands."""
    for t, dt, name in ((codes, torch.int64, "codes"), (label_row, torch.int32, "label_row"), (in_table, bf16, "in_table"), (in0, bf16, "in0"),
                        (act, bf16, "act"), (packs, bf16, "packs"), (scale, f32, "scale"), (shift, f32, "shift"), (head_pack, bf16, "head_pack"),
                        (head_bias, f32, "head_bias"), (logits, f32, "logits")):
        _need(t, dt, name)
        if not t.is_contiguous():
            raise ValueError(f"cfhip pixelcnn_sample: `{name}` must be contiguous")
    if act.dim() != 5 or codes.dim() != 4 or codes.shape[1] != 1:
        raise ValueError(f"cfhip pixelcnn_sample: act {tuple(act.shape)} / codes {tuple(codes.shape)}: [L, B, H, W, C] and [B, 1, H, W] expected")
    nl, b, h, w, c = act.shape
    u, k, cin0 = in_table.shape
    why = pixelcnn_shape_refusal(c, k, nl)
    if why is not None:
        raise NotImplementedError(f"cfhip pixelcnn_sample: {why}")
    kp0, kp = (24 * cin0 + 31) // 32 * 32, 25 * c
    per_pixel = logits.dim() == 4
    want = {"codes": (b, 1, h, w), "label_row": (b,), "in0": (b, h, w, cin0), "packs": (c * kp0 + (nl - 1) * c * kp,), "scale": (nl, c),
            "shift": (nl, c), "head_pack": ((k + 15) // 16 * 16 * c,), "head_bias": (k,), "logits": (b, h, w, k) if per_pixel else (b, k)}
    have = {"codes": codes, "label_row": label_row, "in0": in0, "packs": packs, "scale": scale, "shift": shift, "head_pack": head_pack,
            "head_bias": head_bias, "logits": logits}
    for name, shape in want.items():
        if tuple(have[name].shape) != shape:
            raise ValueError(f"cfhip pixelcnn_sample: `{name}` is {tuple(have[name].shape)}, expected {shape}")
    if cin0 not in (1, c):
        raise ValueError(f"cfhip pixelcnn_sample: the first layer reads {cin0} channels, expected 1 or {c}")
    if not 0 <= first_pixel <= last_pixel <= h * w:
        raise ValueError(f"cfhip pixelcnn_sample: pixel range [{first_pixel}, {last_pixel}) is not inside [0, {h * w})")
    rc = _lib.load().cfhip_pixelcnn_sample(codes.data_ptr(), label_row.data_ptr(), in_table.data_ptr(), in0.data_ptr(), act.data_ptr(),
                                           packs.data_ptr(), scale.data_ptr(), shift.data_ptr(), head_pack.data_ptr(), head_bias.data_ptr(),
                                           logits.data_ptr(), int(per_pixel), b, h, w, c, cin0, nl, k, first_pixel, last_pixel, int(forced),
                                           seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF, _stream())
    _lib.check(rc, "pixelcnn_sample")


# ---------------------------------------------------------------------------------------------
# Masked 7x7 convolution on the live taps (csrc/conv_masked.hip)
# ---------------------------------------------------------------------------------------------

MASKED_TAPS = {"A": 24, "B": 25}
MASKED_GATHER_BYTES = 64 << 20  # the live-tap gather's workspace: the weight gradient walks the rows in chunks of this size


def conv_masked_pack(weight: Tensor, taps: int, transposed: bool = False) -> Tensor:
    """bf16 [Cout, taps Cin] (or [Cin, taps Cout], `transposed`) of the f32 [Cout, Cin, 7, 7] filters: live taps only"""
    _need(weight, f32, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (7, 7) or not weight.is_contiguous():
        raise ValueError(f"cfhip conv_masked_pack: `weight` must be a contiguous [Cout, Cin, 7, 7], got {tuple(weight.shape)}")
    cout, cin = weight.shape[:2]
    out = torch.empty((cin, taps * cout) if transposed else (cout, taps * cin), dtype=bf16, device=weight.device)
    _lib.check(_lib.load().cfhip_conv_masked_pack(weight.data_ptr(), out.data_ptr(), cout, cin, taps, int(transposed), _stream()), "conv_masked_pack")
    return out


def conv_masked(x_rows: Tensor, pack: Tensor, bias: Optional[Tensor], b: int, h: int, w: int, taps: int, mirror: bool = False) -> Tensor:
    """bf16 rows [B H W, Co] (cfhip_conv_masked_bf16) from x_rows bf16 [B H W, Ci] and pack bf16 [Co, taps Ci]"""
    _need(x_rows, bf16, "x_rows")
    _need(pack, bf16, "pack")
    if x_rows.dim() != 2 or not x_rows.is_contiguous() or x_rows.shape[0] != b * h * w or not pack.is_contiguous():
        raise ValueError(f"cfhip conv_masked: x_rows {tuple(x_rows.shape)} must be contiguous [{b * h * w}, Ci], pack contiguous")
    ci, co = x_rows.shape[1], pack.shape[0]
    if pack.shape[1] != taps * ci:
        raise ValueError(f"cfhip conv_masked: pack {tuple(pack.shape)} does not hold {taps} taps of {ci} channels")
    if bias is not None:
        _need(bias, f32, "bias")
        if bias.numel() != co or not bias.is_contiguous():
            raise ValueError(f"cfhip conv_masked: bias {tuple(bias.shape)} for {co} output channels")
    y = torch.empty((b * h * w, co), dtype=bf16, device=x_rows.device)
    _lib.check(_lib.load().cfhip_conv_masked_bf16(x_rows.data_ptr(), pack.data_ptr(), _p(bias), y.data_ptr(), b, h, w, ci, co, taps, int(mirror),
                                                  _stream()), "conv_masked")
    return y


def conv_masked_gather(x_rows: Tensor, b: int, h: int, w: int, taps: int, row0: int, nrows: int, out: Optional[Tensor] = None) -> Tensor:
    """bf16 [nrows, taps Ci] (cfhip_conv_masked_gather): rows [row0, row0 + nrows) of the live-tap matrix of x_rows bf16 [B H W, Ci]"""
    _need(x_rows, bf16, "x_rows")
    if x_rows.dim() != 2 or not x_rows.is_contiguous() or x_rows.shape[0] != b * h * w:
        raise ValueError(f"cfhip conv_masked_gather: x_rows {tuple(x_rows.shape)} must be contiguous [{b * h * w}, Ci]")
    ci = x_rows.shape[1]
    if out is None:
        out = torch.empty((nrows, taps * ci), dtype=bf16, device=x_rows.device)
    elif out.dtype != bf16 or tuple(out.shape) != (nrows, taps * ci) or not out.is_contiguous():
        raise ValueError(f"cfhip conv_masked_gather: `out` must be a contiguous bf16 [{nrows}, {taps * ci}]")
    _lib.check(_lib.load().cfhip_conv_masked_gather(x_rows.data_ptr(), out.data_ptr(), row0, nrows, b, h, w, ci, taps, _stream()), "conv_masked_gather")
    return out


# ---------------------------------------------------------------------------------------------
# NBM: per-basis MLPs and the featurizer (csrc/nbm.hip)
# ---------------------------------------------------------------------------------------------

NBM_MAX_HIDDEN = _H["CFHIP_NBM_MAX_HIDDEN"]
NBM_MAX_ORDER = _H["CFHIP_NBM_MAX_ORDER"]
NBM_GRADS = ("dw1", "db1", "dw2", "db2", "dw3", "db3")  # bit i of cfhip_nbm_bases_bwd's `accumulate`


def nbm_hidden_ok(h: int) -> bool:
    return h % 8 == 0 and 8 <= h <= NBM_MAX_HIDDEN


class NbmIndex:
    """The index table of the basis kernels: `table` int32 [D, order] (contiguous) and `features`, the number of feature columns its
    entries were checked against.  The kernels trust the table, so the wrappers take this pair and nothing else; `nbm_index` is the
    checked way to make one, `to(device)` moves it."""

    def __init__(self, table: Tensor, features: int):
        if table.dtype != torch.int32 or table.dim() != 2 or not table.is_contiguous() or table.numel() == 0:
            raise ValueError(f"cfhip NbmIndex: a contiguous int32 [D, order] table expected, got {tuple(table.shape)} {table.dtype}")
        self.table, self.features = table, int(features)

    @property
    def shape(self):
        return self.table.shape

    def to(self, device) -> "NbmIndex":
        return NbmIndex(self.table.to(device), self.features)


def nbm_index(indices, order: int, num_features: int, device) -> NbmIndex:
    """`NbmIndex` on `device`: the feature columns of every tuple, checked HERE against `num_features`; the pair carries that width
    so that `nbm_bases` can refuse a narrower x."""
    idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1, order)
    if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= num_features:
        raise ValueError(f"cfhip nbm_index: feature columns must lie in [0, {num_features}), got {idx.tolist()}")
    return NbmIndex(idx.to(torch.int32).to(device).contiguous(), num_features)


def _nbm_shapes(x: Tensor, idx: NbmIndex, w1: Tensor, b1: Tensor, b2: Tensor, w3: Tensor, b3: Optional[Tensor], packed: Tensor, who: str):
    if not isinstance(idx, NbmIndex):
        raise TypeError(f"cfhip {who}: `idx` must be the NbmIndex `nbm_index` returns, got {type(idx).__name__}")
    _need(x, f32, "x")
    _need(idx.table, torch.int32, "idx.table")
    _need(packed, bf16, "packed")
    b, f, ldx = _mat(x, "x")
    if idx.features > f:
        raise ValueError(f"cfhip {who}: `idx` addresses {idx.features} feature columns, x has {f}")
    d, o = idx.shape
    if w1.dim() != 3 or w1.shape[2] != o:
        raise ValueError(f"cfhip {who}: `w1` must be [NB, H, {o}], got {tuple(w1.shape)}")
    nb, h = w1.shape[0], w1.shape[1]
    if not nbm_hidden_ok(h) or not 1 <= o <= NBM_MAX_ORDER:
        raise NotImplementedError(f"cfhip {who}: H = {h}, order = {o} is outside the basis kernels (H % 8 == 0, 8 <= H <= {NBM_MAX_HIDDEN}, "
                                  f"1 <= order <= {NBM_MAX_ORDER})")
    for t, shape, name in ((w1, (nb, h, o), "w1"), (b1, (nb, h), "b1"), (b2, (nb, h), "b2"), (w3, (nb, h), "w3"), (b3, (nb,), "b3")):
        if t is None:
            continue
        _need(t, f32, name)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"cfhip {who}: `{name}` must be a contiguous f32 {list(shape)}, got {tuple(t.shape)}")
    if b < 1 or b * d >= 2 ** 31 - 1:
        raise ValueError(f"cfhip {who}: B D = {b * d} rows")
    if packed.numel() * 2 != _lib.load().cfhip_nbm_pack_workspace(nb, h) or not packed.is_contiguous():
        raise ValueError(f"cfhip {who}: `packed` is not nbm_pack's output for NB = {nb}, H = {h}")
    return b, f, ldx, d, o, nb, h


def nbm_pack(w2: Tensor) -> Tensor:
    """bf16 1-D (cfhip_nbm_pack): W2 f32 [NB, H, H] in MFMA fragment order, for the forward and for the backward product"""
    _need(w2, f32, "w2")
    if w2.dim() != 3 or w2.shape[1] != w2.shape[2] or not w2.is_contiguous():
        raise ValueError(f"cfhip nbm_pack: `w2` must be a contiguous f32 [NB, H, H], got {tuple(w2.shape)}")
    nb, h = w2.shape[0], w2.shape[1]
    if not nbm_hidden_ok(h):
        raise NotImplementedError(f"cfhip nbm_pack: H = {h} is outside the basis kernels (H % 8 == 0, 8 <= H <= {NBM_MAX_HIDDEN})")
    lib = _lib.load()
    nbytes = lib.cfhip_nbm_pack_workspace(nb, h)
    packed = torch.empty((nbytes // 2,), dtype=bf16, device=w2.device)
    _lib.check(lib.cfhip_nbm_pack(w2.data_ptr(), packed.data_ptr(), nbytes, nb, h, _stream()), "nbm_pack")
    return packed


def nbm_bases(x: Tensor, idx: NbmIndex, w1: Tensor, b1: Tensor, packed: Tensor, b2: Tensor, w3: Tensor, b3: Tensor,
              out: Optional[Tensor] = None) -> Tensor:
    """bases f32 [B, D, NB] (cfhip_nbm_bases_fwd): x f32 [B, F] (rows a fixed stride apart), idx from `nbm_index`, w1 [NB, H, order],
    b1 / b2 / w3 [NB, H], b3 [NB], `packed` from `nbm_pack`.  Allocates nothing but the result."""
    b, _, ldx, d, o, nb, h = _nbm_shapes(x, idx, w1, b1, b2, w3, b3, packed, "nbm_bases")
    if out is None:
        out = torch.empty((b, d, nb), dtype=f32, device=x.device)
    elif out.dtype != f32 or tuple(out.shape) != (b, d, nb) or not out.is_contiguous():
        raise ValueError(f"cfhip nbm_bases: `out` must be a contiguous f32 [{b}, {d}, {nb}]")
    rc = _lib.load().cfhip_nbm_bases_fwd(x.data_ptr(), ldx, idx.table.data_ptr(), w1.data_ptr(), b1.data_ptr(), packed.data_ptr(), b2.data_ptr(),
                                         w3.data_ptr(), b3.data_ptr(), out.data_ptr(), b, d, nb, h, o, _stream())
    _lib.check(rc, "nbm_bases")
    return out


def nbm_bases_grad(dbases: Tensor, x: Tensor, idx: NbmIndex, w1: Tensor, b1: Tensor, packed: Tensor, b2: Tensor, w3: Tensor, *,
                   dests: dict, accumulate: Sequence = (), want_dx: bool = False) -> Optional[Tensor]:
    """cfhip_nbm_bases_bwd: `dests` maps names of NBM_GRADS to f32 destinations of the parameters' shapes (a missing or None entry is
    frozen: not reduced, nothing written); names in `accumulate` are added to, the others overwritten.  Returns dx f32 [B, F] with
    `want_dx`, else None.  The workspace is a torch tensor that lives for this call."""
    b, f, ldx, d, o, nb, h = _nbm_shapes(x, idx, w1, b1, b2, w3, None, packed, "nbm_bases_grad")
    _need(dbases, f32, "dbases")
    if tuple(dbases.shape) != (b, d, nb) or not dbases.is_contiguous():
        raise ValueError(f"cfhip nbm_bases_grad: `dbases` must be a contiguous f32 [{b}, {d}, {nb}], got {tuple(dbases.shape)}")
    shapes = {"dw1": (nb, h, o), "db1": (nb, h), "dw2": (nb, h, h), "db2": (nb, h), "dw3": (nb, h), "db3": (nb,)}
    unknown = (set(dests) | set(accumulate)) - set(NBM_GRADS)
    if unknown:
        raise ValueError(f"cfhip nbm_bases_grad: unknown destinations {sorted(unknown)}")
    ptrs, mask = [], 0
    for bit, name in enumerate(NBM_GRADS):
        t = dests.get(name)
        if t is not None:
            _need(t, f32, name)
            if t.numel() != math.prod(shapes[name]) or not t.is_contiguous():
                raise ValueError(f"cfhip nbm_bases_grad: `{name}` must be a contiguous f32 of {math.prod(shapes[name])} elements")
            if name in accumulate:
                mask |= 1 << bit
        ptrs.append(_p(t))
    lib = _lib.load()
    nbytes = lib.cfhip_nbm_bases_bwd_workspace(b * d, nb, h, o, int(want_dx))
    ws = torch.empty((nbytes // 4,), dtype=f32, device=x.device)
    dx = torch.empty((b, f), dtype=f32, device=x.device) if want_dx else None
    rc = lib.cfhip_nbm_bases_bwd(dbases.data_ptr(), x.data_ptr(), ldx, idx.table.data_ptr(), w1.data_ptr(), b1.data_ptr(), packed.data_ptr(),
                                 b2.data_ptr(), w3.data_ptr(), *ptrs, _p(dx), mask, ws.data_ptr(), nbytes, b, d, f, nb, h, o, _stream())
    _lib.check(rc, "nbm_bases_grad")
    return dx


def nbm_featurize(bases: Tensor, wf: Tensor, bf: Tensor) -> Tensor:
    """feat f32 [B, D] (cfhip_nbm_featurize_fwd): bases f32 [B, D, NB], wf f32 [D, NB], bf f32 [D]"""
    for t, name in ((bases, "bases"), (wf, "wf"), (bf, "bf")):
        _need(t, f32, name)
    if bases.dim() != 3 or not bases.is_contiguous():
        raise ValueError(f"cfhip nbm_featurize: `bases` must be a contiguous f32 [B, D, NB], got {tuple(bases.shape)}")
    b, d, nb = bases.shape
    if wf.numel() != d * nb or bf.numel() != d or not wf.is_contiguous() or not bf.is_contiguous():
        raise ValueError(f"cfhip nbm_featurize: wf {tuple(wf.shape)} / bf {tuple(bf.shape)} do not fit bases {tuple(bases.shape)}")
    feat = torch.empty((b, d), dtype=f32, device=bases.device)
    _lib.check(_lib.load().cfhip_nbm_featurize_fwd(bases.data_ptr(), wf.data_ptr(), bf.data_ptr(), feat.data_ptr(), b, d, nb, _stream()),
               "nbm_featurize")
    return feat


def nbm_featurize_grad(dfeat: Tensor, bases: Optional[Tensor], wf: Tensor, *, dwf: Optional[Tensor] = None, dbf: Optional[Tensor] = None,
                       accumulate: Sequence = (), want_dbases: bool = True) -> Optional[Tensor]:
    """cfhip_nbm_featurize_bwd: dfeat f32 [B, D] -> dbases f32 [B, D, NB] (returned with `want_dbases`), dwf [D, NB] (needs `bases`)
    and dbf [D] written into the given destinations (None = frozen); names in `accumulate` ("dwf", "dbf") are added to."""
    _need(dfeat, f32, "dfeat")
    _need(wf, f32, "wf")
    if dfeat.dim() != 2 or not dfeat.is_contiguous() or wf.dim() < 2 or not wf.is_contiguous() or wf.shape[0] != dfeat.shape[1]:
        raise ValueError(f"cfhip nbm_featurize_grad: dfeat {tuple(dfeat.shape)} / wf {tuple(wf.shape)}: contiguous [B, D] and [D, NB] expected")
    b, d = dfeat.shape
    nb = wf.numel() // d
    if dwf is not None:
        if bases is None:
            raise ValueError("cfhip nbm_featurize_grad: dwf needs `bases`")
        _need(bases, f32, "bases")
        if tuple(bases.shape) != (b, d, nb) or not bases.is_contiguous():
            raise ValueError(f"cfhip nbm_featurize_grad: `bases` must be a contiguous f32 [{b}, {d}, {nb}]")
    for t, n, name in ((dwf, d * nb, "dwf"), (dbf, d, "dbf")):
        if t is not None:
            _need(t, f32, name)
            if t.numel() != n or not t.is_contiguous():
                raise ValueError(f"cfhip nbm_featurize_grad: `{name}` must be a contiguous f32 of {n} elements")
    mask = (1 if "dwf" in accumulate else 0) | (2 if "dbf" in accumulate else 0)
    lib = _lib.load()
    nbytes = lib.cfhip_nbm_featurize_bwd_workspace(b, d, nb)
    ws = torch.empty((nbytes // 4,), dtype=f32, device=dfeat.device)
    dbases = torch.empty((b, d, nb), dtype=f32, device=dfeat.device) if want_dbases else None
    rc = lib.cfhip_nbm_featurize_bwd(dfeat.data_ptr(), _p(bases if dwf is not None else None), wf.data_ptr(), _p(dbases), _p(dwf), _p(dbf),
                                     mask, ws.data_ptr(), nbytes, b, d, nb, _stream())
    _lib.check(rc, "nbm_featurize_grad")
    return dbases


# -------------------------------------------------------------------------------------------------------------------------------------
# RWKV mixers: time shift + mixes, the WKV scan, relu^2 and the gate (csrc/rwkv.hip)
# -------------------------------------------------------------------------------------------------------------------------------------
RWKV_CHUNK = _H["CFHIP_RWKV_CHUNK"]
RWKV_MAX_WAVES = _H["CFHIP_RWKV_MAX_WAVES"]
RWKV_MIXES = ("dmk", "dmv", "dmr")  # bit i of cfhip_rwkv_time_mix_bwd's `accumulate`


def _rwkv_act(t: Tensor, name: str, who: str) -> int:
    """1 for a contiguous f32 activation, 0 for bf16; anything else is refused"""
    if not t.is_cuda:
        raise RuntimeError(f"cfhip {who}: `{name}` must live on the HIP device (got {t.device})")
    if t.dtype not in (f32, bf16):
        raise TypeError(f"cfhip {who}: `{name}` must be float32 or bfloat16, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"cfhip {who}: `{name}` must be contiguous, got strides {t.stride()}")
    return int(t.dtype == f32)


def _rwkv_vec(t: Optional[Tensor], n: int, name: str, who: str) -> None:
    if t is None:
        return
    _need(t, f32, name)
    if t.numel() != n or not t.is_contiguous():
        raise ValueError(f"cfhip {who}: `{name}` must be a contiguous f32 of {n} elements, got {tuple(t.shape)}")


def _rwkv_btc(x: Tensor, name: str, who: str) -> Tuple[int, int, int]:
    if x.dim() != 3:
        raise ValueError(f"cfhip {who}: `{name}` must be [B, T, C], got {tuple(x.shape)}")
    return x.shape[0], x.shape[1], x.shape[2]


def rwkv_time_mix(x: Tensor, mk: Tensor, mv: Optional[Tensor], mr: Tensor) -> Tuple[Tensor, ...]:
    """bf16 [B, T, C] per mix (cfhip_rwkv_time_mix_fwd): x f32 or bf16 [B, T, C], the mixes f32 of C elements; `mv` None = the two
    mixes (k, r) of the channel mixer.  Returns (in_k, in_v, in_r) or (in_k, in_r)."""
    xf = _rwkv_act(x, "x", "rwkv_time_mix")
    b, t, c = _rwkv_btc(x, "x", "rwkv_time_mix")
    for m, name in ((mk, "mk"), (mv, "mv"), (mr, "mr")):
        _rwkv_vec(m, c, name, "rwkv_time_mix")
    outs = [torch.empty((b, t, c), dtype=bf16, device=x.device) for _ in range(2 if mv is None else 3)]
    ok, orr = outs[0], outs[-1]
    ov = None if mv is None else outs[1]
    rc = _lib.load().cfhip_rwkv_time_mix_fwd(x.data_ptr(), xf, mk.data_ptr(), _p(mv), mr.data_ptr(), ok.data_ptr(), _p(ov), orr.data_ptr(), b, t, c,
                                             _stream())
    _lib.check(rc, "rwkv_time_mix")
    return tuple(outs)


def rwkv_time_mix_grad(dk: Tensor, dv: Optional[Tensor], dr: Tensor, x: Tensor, mk: Tensor, mv: Optional[Tensor], mr: Tensor, *,
                       dests: Dict[str, Optional[Tensor]], accumulate: Sequence[str] = (), want_dx: bool = True) -> Optional[Tensor]:
    """cfhip_rwkv_time_mix_bwd: d_j f32 or bf16 [B, T, C] (one dtype) -> dx (x's dtype, returned with `want_dx`) and the mix gradients written into
    `dests` (names of RWKV_MIXES -> f32 of C elements; a missing or None entry is frozen: not computed, not reduced); names in
    `accumulate` are added to."""
    who = "rwkv_time_mix_grad"
    xf = _rwkv_act(x, "x", who)
    b, t, c = _rwkv_btc(x, "x", who)
    dfs = set()
    for d, name in ((dk, "dk"), (dv, "dv"), (dr, "dr")):
        if d is not None:
            dfs.add(_rwkv_act(d, name, who))
            if tuple(d.shape) != (b, t, c):
                raise ValueError(f"cfhip {who}: `{name}` must be [{b}, {t}, {c}], got {tuple(d.shape)}")
    if len(dfs) != 1:
        raise TypeError(f"cfhip {who}: dk, dv and dr must share one dtype")
    df = dfs.pop()
    if (dv is None) != (mv is None):
        raise ValueError(f"cfhip {who}: `dv` and `mv` go together")
    for m, name in ((mk, "mk"), (mv, "mv"), (mr, "mr")):
        _rwkv_vec(m, c, name, who)
    unknown = (set(dests) | set(accumulate)) - set(RWKV_MIXES)
    if unknown or (mv is None and dests.get("dmv") is not None):
        raise ValueError(f"cfhip {who}: unknown destinations {sorted(unknown) or ['dmv']}")
    mask, ptrs = 0, []
    for bit, name in enumerate(RWKV_MIXES):
        d = dests.get(name)
        _rwkv_vec(d, c, name, who)
        if d is not None and name in accumulate:
            mask |= 1 << bit
        ptrs.append(_p(d))
    wanted = any(p is not None for p in ptrs)
    if not wanted and not want_dx:
        return None
    lib = _lib.load()
    nbytes = lib.cfhip_rwkv_time_mix_bwd_workspace(b, t, c) if wanted else 0
    ws = torch.empty((nbytes // 4,), dtype=f32, device=x.device) if wanted else None
    dx = torch.empty_like(x) if want_dx else None
    rc = lib.cfhip_rwkv_time_mix_bwd(dk.data_ptr(), _p(dv), dr.data_ptr(), df, x.data_ptr(), xf, mk.data_ptr(), _p(mv), mr.data_ptr(), _p(dx), *ptrs,
                                     mask, _p(ws), nbytes, b, t, c, _stream())
    _lib.check(rc, who)
    return dx


def _rwkv_kvr(k: Tensor, v: Tensor, r: Tensor, decay: Tensor, who: str) -> Tuple[int, int, int]:
    b, t, l = _rwkv_btc(k, "k", who)
    for x, name in ((k, "k"), (v, "v"), (r, "r")):
        _need(x, f32, name)
        if tuple(x.shape) != (b, t, l) or not x.is_contiguous():
            raise ValueError(f"cfhip {who}: `{name}` must be a contiguous f32 [{b}, {t}, {l}], got {tuple(x.shape)} / {x.stride()}")
    _rwkv_vec(decay, l, "info_decay", who)
    return b, t, l


def rwkv_wkv(k: Tensor, v: Tensor, r: Tensor, info_decay: Tensor, *, save: bool = False, waves: int = 0):
    """y bf16 [B, T, L] = sigmoid(r) * wkv (cfhip_rwkv_wkv_fwd) from k, v, r f32 [B, T, L] and info_decay f32 of L elements.  With
    `save` returns (y, a, b), the two f32 scan states the backward reads; without it allocates nothing but y.  `waves`: chunks per
    pass of a workgroup (0 = chosen from the shape); the result does not depend on it."""
    b, t, l = _rwkv_kvr(k, v, r, info_decay, "rwkv_wkv")
    y = torch.empty((b, t, l), dtype=bf16, device=k.device)
    sa = torch.empty((b, t, l), dtype=f32, device=k.device) if save else None
    sb = torch.empty((b, t, l), dtype=f32, device=k.device) if save else None
    rc = _lib.load().cfhip_rwkv_wkv_fwd(k.data_ptr(), v.data_ptr(), r.data_ptr(), info_decay.data_ptr(), y.data_ptr(), _p(sa), _p(sb), b, t, l,
                                        int(waves), _stream())
    _lib.check(rc, "rwkv_wkv")
    return (y, sa, sb) if save else y


def rwkv_wkv_grad(dy: Tensor, k: Tensor, v: Tensor, r: Tensor, info_decay: Tensor, sa: Tensor, sb: Tensor, *, d_decay: Optional[Tensor] = None,
                  accumulate: bool = False, waves: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """(dk, dv, dr) bf16 [B, T, L] (cfhip_rwkv_wkv_bwd) from dy (f32 or bf16) and what `rwkv_wkv(save=True)` returned; `d_decay` (f32 of L
    elements, None = frozen: no partials, no reduce launch) is written, or added to with `accumulate`."""
    who = "rwkv_wkv_grad"
    b, t, l = _rwkv_kvr(k, v, r, info_decay, who)
    dyf = _rwkv_act(dy, "dy", who)
    for x, name in ((sa, "a"), (sb, "b")):
        _need(x, f32, name)
    for x, name in ((dy, "dy"), (sa, "a"), (sb, "b")):
        if tuple(x.shape) != (b, t, l) or not x.is_contiguous():
            raise ValueError(f"cfhip {who}: `{name}` must be a contiguous [{b}, {t}, {l}], got {tuple(x.shape)}")
    _rwkv_vec(d_decay, l, "d_decay", who)
    lib = _lib.load()
    nbytes = lib.cfhip_rwkv_wkv_bwd_workspace(b, l) if d_decay is not None else 0
    ws = torch.empty((nbytes // 4,), dtype=f32, device=k.device) if d_decay is not None else None
    dk, dv, dr = (torch.empty((b, t, l), dtype=bf16, device=k.device) for _ in range(3))
    rc = lib.cfhip_rwkv_wkv_bwd(dy.data_ptr(), dyf, k.data_ptr(), v.data_ptr(), r.data_ptr(), info_decay.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), _p(d_decay), int(bool(accumulate and d_decay is not None)), _p(ws),
                                nbytes, b, t, l, int(waves), _stream())
    _lib.check(rc, who)
    return dk, dv, dr


def rwkv_relu2(h: Tensor) -> Tensor:
    """bf16 relu(h)^2 (cfhip_rwkv_relu2_fwd), h f32 or bf16"""
    hf = _rwkv_act(h, "h", "rwkv_relu2")
    out = torch.empty(h.shape, dtype=bf16, device=h.device)
    _lib.check(_lib.load().cfhip_rwkv_relu2_fwd(h.data_ptr(), hf, out.data_ptr(), h.numel(), _stream()), "rwkv_relu2")
    return out


def rwkv_relu2_grad(d: Tensor, h: Tensor) -> Tensor:
    """bf16 2 relu(h) d (cfhip_rwkv_relu2_bwd), d f32 or bf16 of h's shape"""
    hf = _rwkv_act(h, "h", "rwkv_relu2_grad")
    df = _rwkv_act(d, "d", "rwkv_relu2_grad")
    if d.shape != h.shape:
        raise ValueError(f"cfhip rwkv_relu2_grad: `d` must have the shape {tuple(h.shape)}, got {tuple(d.shape)}")
    dh = torch.empty(h.shape, dtype=bf16, device=h.device)
    _lib.check(_lib.load().cfhip_rwkv_relu2_bwd(d.data_ptr(), df, h.data_ptr(), hf, dh.data_ptr(), h.numel(), _stream()), "rwkv_relu2_grad")
    return dh


def rwkv_gate(r: Tensor, kv: Tensor, residual: Optional[Tensor] = None) -> Tensor:
    """sigmoid(r) * kv (+ residual) (cfhip_rwkv_gate_fwd): r, kv f32 of one shape; the result has the residual's dtype (f32 or bf16),
    bf16 without one"""
    who = "rwkv_gate"
    for x, name in ((r, "r"), (kv, "kv")):
        _need(x, f32, name)
    if r.shape != kv.shape or not r.is_contiguous() or not kv.is_contiguous():
        raise ValueError(f"cfhip {who}: r {tuple(r.shape)} and kv {tuple(kv.shape)} must be contiguous and of one shape")
    rf = 0
    if residual is not None:
        rf = _rwkv_act(residual, "residual", who)
        if residual.shape != r.shape:
            raise ValueError(f"cfhip {who}: residual {tuple(residual.shape)} does not fit {tuple(r.shape)}")
    out = torch.empty(r.shape, dtype=bf16 if residual is None else residual.dtype, device=r.device)
    rc = _lib.load().cfhip_rwkv_gate_fwd(r.data_ptr(), kv.data_ptr(), _p(residual), rf, out.data_ptr(), int(out.dtype == f32), r.numel(), _stream())
    _lib.check(rc, who)
    return out


def rwkv_gate_grad(d: Tensor, r: Tensor, kv: Tensor) -> Tuple[Tensor, Tensor]:
    """(dr, dkv) bf16 (cfhip_rwkv_gate_bwd): d f32 or bf16 of r's shape"""
    who = "rwkv_gate_grad"
    df = _rwkv_act(d, "d", who)
    for x, name in ((r, "r"), (kv, "kv")):
        _need(x, f32, name)
    if not (d.shape == r.shape == kv.shape) or not r.is_contiguous() or not kv.is_contiguous():
        raise ValueError(f"cfhip {who}: d {tuple(d.shape)}, r {tuple(r.shape)} and kv {tuple(kv.shape)} must be contiguous and of one shape")
    dr = torch.empty(r.shape, dtype=bf16, device=r.device)
    dkv = torch.empty(r.shape, dtype=bf16, device=r.device)
    _lib.check(_lib.load().cfhip_rwkv_gate_bwd(d.data_ptr(), df, r.data_ptr(), kv.data_ptr(), dr.data_ptr(), dkv.data_ptr(), r.numel(), _stream()), who)
    return dr, dkv


# -------------------------------------------------------------------------------------------------------------------------------------
# Siren: the fused coordinate MLP and the stand-alone sine (csrc/siren.hip)
# -------------------------------------------------------------------------------------------------------------------------------------
SIREN_MAX_LATENT = _H["CFHIP_SIREN_MAX_LATENT"]
SIREN_MAX_IN = _H["CFHIP_SIREN_MAX_IN"]
SIREN_MAX_OUT = _H["CFHIP_SIREN_MAX_OUT"]
SIREN_KINDS = {"db": _H["CFHIP_SIREN_DB"], "dw0": _H["CFHIP_SIREN_DW0"], "dwhead": _H["CFHIP_SIREN_DWHEAD"], "dbhead": _H["CFHIP_SIREN_DBHEAD"],
               "dmods": _H["CFHIP_SIREN_DMODS"]}


def siren_latent_ok(latent: int) -> bool:
    return latent % 32 == 0 and 32 <= latent <= SIREN_MAX_LATENT


class SirenShape:
    """the integers and the two sine frequencies that every Siren entry takes: B samples of N rows, in_dim -> latent x num_layers ->
    out_dim.  Refuses what the kernel refuses, by name, before any launch."""

    __slots__ = ("b", "n", "in_dim", "latent", "out_dim", "layers", "w_first", "w_hidden")

    def __init__(self, b: int, n: int, in_dim: int, latent: int, out_dim: int, layers: int, w_first: float, w_hidden: float):
        if not siren_latent_ok(latent):
            raise NotImplementedError(f"cfhip siren: latent_dim = {latent} is outside the kernel (a multiple of 32 in 32 .. {SIREN_MAX_LATENT}; DESIGN §8)")
        if not 1 <= in_dim <= SIREN_MAX_IN:
            raise NotImplementedError(f"cfhip siren: in_dim = {in_dim} is outside the kernel (1 .. {SIREN_MAX_IN}; DESIGN §8)")
        if not 1 <= out_dim <= SIREN_MAX_OUT:
            raise NotImplementedError(f"cfhip siren: out_dim = {out_dim} is outside the kernel (1 .. {SIREN_MAX_OUT}; DESIGN §8)")
        if layers < 1:
            raise NotImplementedError(f"cfhip siren: num_layers = {layers} is outside the kernel (>= 1; DESIGN §8)")
        if b < 1 or n < 1 or b * n >= 2 ** 31 - 1:
            raise ValueError(f"cfhip siren: B = {b}, N = {n}: M = B N must lie in 1 .. 2^31 - 2")
        self.b, self.n, self.in_dim, self.latent, self.out_dim, self.layers = b, n, in_dim, latent, out_dim, layers
        self.w_first, self.w_hidden = float(w_first), float(w_hidden)

    @property
    def m(self) -> int:
        return self.b * self.n

    def ints(self) -> Tuple[int, int, int, int, int, int]:
        return self.b, self.n, self.in_dim, self.latent, self.out_dim, self.layers


def _siren_f32(t: Tensor, shape: Tuple[int, ...], name: str, who: str) -> None:
    _need(t, f32, name)
    if tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"cfhip {who}: `{name}` must be a contiguous f32 {list(shape)}, got {tuple(t.shape)} / {t.stride()}")


def siren_pack(hidden: Sequence[Tensor], head_w: Tensor, *, transposed: bool = False) -> Tensor:
    """bf16 1-D (cfhip_siren_pack per weight): the hidden weights f32 [latent, latent] in layer order, then the head's f32 [out_dim,
    latent], each in MFMA fragment order for the forward; with `transposed` every hidden weight also for the backward product (the
    head's backward reads the f32 weight: its pack is the forward's alone)"""
    _need(head_w, f32, "head_w")
    if head_w.dim() != 2 or not head_w.is_contiguous():
        raise ValueError(f"cfhip siren_pack: `head_w` must be a contiguous f32 [out_dim, latent], got {tuple(head_w.shape)}")
    out_dim, latent = head_w.shape
    if not siren_latent_ok(latent) or not 1 <= out_dim <= SIREN_MAX_OUT:
        raise NotImplementedError(f"cfhip siren_pack: latent_dim = {latent}, out_dim = {out_dim} is outside the kernel (DESIGN §8)")
    for i, w in enumerate(hidden):
        _siren_f32(w, (latent, latent), f"hidden[{i}]", "siren_pack")
    lib = _lib.load()
    hid, head = lib.cfhip_siren_pack_workspace(latent, latent, int(transposed)), lib.cfhip_siren_pack_workspace(out_dim, latent, 0)
    packed = torch.empty(((len(hidden) * hid + head) // 2,), dtype=bf16, device=head_w.device)
    base = packed.data_ptr()
    for i, w in enumerate(hidden):
        _lib.check(lib.cfhip_siren_pack(w.data_ptr(), base + i * hid, hid, latent, latent, int(transposed), _stream()), "siren_pack")
    _lib.check(lib.cfhip_siren_pack(head_w.data_ptr(), base + len(hidden) * hid, head, out_dim, latent, 0, _stream()), "siren_pack")
    return packed


def _siren_operands(sh: SirenShape, x: Tensor, x_shared: bool, w0: Tensor, packed: Tensor, mods: Tensor, who: str, need_transposed: bool = False) -> bool:
    """checks the operands the entries share; returns whether `packed` holds the transposed hidden packs"""
    _siren_f32(x, (sh.n if x_shared else sh.m, sh.in_dim), "x", who)
    _siren_f32(w0, (sh.latent, sh.in_dim), "w0", who)
    _siren_f32(mods, (sh.layers, sh.b, sh.latent), "mods", who)
    _need(packed, bf16, "packed")
    lib = _lib.load()
    head = lib.cfhip_siren_pack_workspace(sh.out_dim, sh.latent, 0)
    sizes = [(sh.layers - 1) * lib.cfhip_siren_pack_workspace(sh.latent, sh.latent, t) + head for t in (0, 1)]
    have = packed.numel() * 2
    if have not in (sizes[1:] if need_transposed else sizes) or not packed.is_contiguous():
        raise ValueError(f"cfhip {who}: `packed` is not siren_pack's output for {sh.layers} layers of latent {sh.latent} and out_dim {sh.out_dim}"
                         + (" with transposed = True" if need_transposed else ""))
    return have == sizes[1]


def siren_fwd(sh: SirenShape, x: Tensor, x_shared: bool, w0: Tensor, packed: Tensor, bias: Optional[Tensor], mods: Tensor, *,
              save: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """(out f32 [M, out_dim], sin words, cos words) (cfhip_siren_fwd, one launch): x f32 [M, in_dim] (or, `x_shared`, the grid f32 [N,
    in_dim] of every sample), w0 f32 [latent, in_dim], `packed` from `siren_pack` (with or without the transposed part), bias f32 [layers * latent + out_dim] or None, mods
    f32 [layers, B, latent].  With `save` the bf16 [layers, M, latent] sine and cosine words the backward reads, else (out, None, None)
    and nothing of size M * latent exists."""
    transposed = _siren_operands(sh, x, x_shared, w0, packed, mods, "siren_fwd")
    if bias is not None:
        _siren_f32(bias, (sh.layers * sh.latent + sh.out_dim,), "bias", "siren_fwd")
    out = torch.empty((sh.m, sh.out_dim), dtype=f32, device=x.device)
    ss = torch.empty((sh.layers, sh.m, sh.latent), dtype=bf16, device=x.device) if save else None
    sc = torch.empty_like(ss) if save else None
    rc = _lib.load().cfhip_siren_fwd(x.data_ptr(), int(x_shared), w0.data_ptr(), packed.data_ptr(), int(transposed), _p(bias), mods.data_ptr(), out.data_ptr(), _p(ss),
                                     _p(sc), *sh.ints(), sh.w_first, sh.w_hidden, _stream())
    _lib.check(rc, "siren_fwd")
    return out, ss, sc


def siren_bwd(sh: SirenShape, dy: Tensor, x: Tensor, x_shared: bool, w0: Tensor, packed: Tensor, head_w: Tensor, mods: Tensor, ss: Tensor,
              sc: Tensor, *, want_dx: bool = False, want_hidden: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """(workspace, dx, dpre, hprev) (cfhip_siren_bwd, one launch): dy f32 [M, out_dim]; `ss` / `sc` from `siren_fwd(save=True)`.  dx f32
    [M, in_dim] with `want_dx`; with `want_hidden` dpre and hprev bf16 [layers - 1, M, latent], the operands of the hidden weights'
    tn GEMMs.  Every other gradient is read out of the workspace by `siren_reduce`."""
    _siren_operands(sh, x, x_shared, w0, packed, mods, "siren_bwd", need_transposed=True)
    _siren_f32(dy, (sh.m, sh.out_dim), "dy", "siren_bwd")
    _siren_f32(head_w, (sh.out_dim, sh.latent), "head_w", "siren_bwd")
    for t, name in ((ss, "ss"), (sc, "sc")):
        _need(t, bf16, name)
        if tuple(t.shape) != (sh.layers, sh.m, sh.latent) or not t.is_contiguous():
            raise ValueError(f"cfhip siren_bwd: `{name}` must be the contiguous bf16 [{sh.layers}, {sh.m}, {sh.latent}] siren_fwd saved")
    lib = _lib.load()
    nbytes = lib.cfhip_siren_bwd_workspace(*sh.ints())
    ws = torch.empty((nbytes // 4,), dtype=f32, device=dy.device)
    dx = torch.empty((sh.m, sh.in_dim), dtype=f32, device=dy.device) if want_dx else None
    hidden = want_hidden and sh.layers > 1
    dpre = torch.empty((sh.layers - 1, sh.m, sh.latent), dtype=bf16, device=dy.device) if hidden else None
    hprev = torch.empty_like(dpre) if hidden else None
    rc = lib.cfhip_siren_bwd(dy.data_ptr(), x.data_ptr(), int(x_shared), w0.data_ptr(), packed.data_ptr(), head_w.data_ptr(), mods.data_ptr(),
                             ss.data_ptr(), sc.data_ptr(), _p(dx), _p(dpre), _p(hprev), ws.data_ptr(), nbytes, *sh.ints(), sh.w_first, sh.w_hidden,
                             _stream())
    _lib.check(rc, "siren_bwd")
    return ws, dx, dpre, hprev


def siren_reduce(sh: SirenShape, ws: Tensor, kind: str, dest: Tensor, *, layer: int = 0, accumulate: bool = False) -> Tensor:
    """cfhip_siren_reduce: one gradient out of `siren_bwd`'s workspace into `dest` (f32, contiguous): kind "db" (the bias of `layer`),
    "dw0", "dwhead", "dbhead" or "dmods" ([layers, B, latent])"""
    if kind not in SIREN_KINDS:
        raise ValueError(f"cfhip siren_reduce: unknown kind {kind!r}")
    sizes = {"db": sh.latent, "dw0": sh.latent * sh.in_dim, "dwhead": sh.out_dim * sh.latent, "dbhead": sh.out_dim,
             "dmods": sh.layers * sh.b * sh.latent}
    _need(ws, f32, "ws")
    _need(dest, f32, "dest")
    if dest.numel() != sizes[kind] or not dest.is_contiguous():
        raise ValueError(f"cfhip siren_reduce: `dest` of {kind} must be a contiguous f32 of {sizes[kind]} elements, got {tuple(dest.shape)}")
    rc = _lib.load().cfhip_siren_reduce(ws.data_ptr(), ws.numel() * 4, SIREN_KINDS[kind], int(layer), dest.data_ptr(), int(accumulate), *sh.ints(),
                                        _stream())
    _lib.check(rc, "siren_reduce")
    return dest


def sine_fwd(x: Tensor, w: float) -> Tensor:
    """f32 sin(w x) (cfhip_sine_fwd) of a contiguous f32 tensor"""
    _need(x, f32, "x")
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("cfhip sine_fwd: a contiguous, non-empty tensor expected")
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_sine_fwd(x.data_ptr(), y.data_ptr(), x.numel(), float(w), _stream()), "sine_fwd")
    return y


def sine_bwd(dy: Tensor, x: Tensor, w: float) -> Tensor:
    """f32 dy w cos(w x) (cfhip_sine_bwd)"""
    _need(dy, f32, "dy")
    _need(x, f32, "x")
    if not x.is_contiguous() or not dy.is_contiguous() or dy.shape != x.shape or x.numel() == 0:
        raise ValueError("cfhip sine_bwd: two contiguous, non-empty tensors of one shape expected")
    dx = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_sine_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), float(w), _stream()), "sine_bwd")
    return dx


def relu_f32_fwd(x: Tensor) -> Tensor:
    """f32 max(x, 0) (cfhip_relu_f32_fwd) of a contiguous f32 tensor"""
    _need(x, f32, "x")
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("cfhip relu_f32_fwd: a contiguous, non-empty tensor expected")
    y = torch.empty_like(x)
    _lib.check(_lib.load().cfhip_relu_f32_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "relu_f32_fwd")
    return y


def relu_f32_bwd(dy: Tensor, y: Tensor) -> Tensor:
    """f32 (y > 0 ? dy : 0) (cfhip_relu_f32_bwd), y the forward's output"""
    _need(dy, f32, "dy")
    _need(y, f32, "y")
    if not y.is_contiguous() or not dy.is_contiguous() or dy.shape != y.shape or y.numel() == 0:
        raise ValueError("cfhip relu_f32_bwd: two contiguous, non-empty tensors of one shape expected")
    dx = torch.empty_like(y)
    _lib.check(_lib.load().cfhip_relu_f32_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.numel(), _stream()), "relu_f32_bwd")
    return dx
