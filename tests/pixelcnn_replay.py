"""float64 replicas of what csrc/pixelcnn.hip computes, in numpy / torch float64 on the CPU (nothing of the project's kernels is called):

  * `masked_conv64`: the 7x7 / padding 3 masked convolution as an explicit loop over the LIVE taps only (masked taps are never read:
    a NaN there does not reach the result), on whatever values it is given (the callers round the operands to bf16 first);
  * `layer_step64` / `head_step64`: ONE layer / the head of the sampler at every pixel of a map, from the bf16 activations the layer
    below left, with the kernel's rounding points: the sum over the live taps in float64 (the kernel: one f32 MFMA chain), the f32
    scale and shift, LeakyReLU(0.2) — the value the kernel then rounds to bf16 — and `cond`, the same sum on absolute values, which
    bounds the f32 chain's error;
  * `draw64`: the inverse-CDF pick from f32 logits and the Philox word of tests/philox_ref.py, with the distance of u from the two CDF
    boundaries of the pick (a pixel is decidable when that distance exceeds the f32 evaluation's error)."""
import numpy as np
import torch

import philox_ref as P


def live_taps(mask_type: str, k: int = 7):
    """[(di, dj)] of the live taps of a k x k mask in row-major order: the rows above the centre, then the centre row left of the centre,
    and for "B" the centre itself"""
    c = k // 2
    taps = [(i, j) for i in range(c) for j in range(k)] + [(c, j) for j in range(c + (mask_type == "B"))]
    return taps


def mask_of(mask_type: str, k: int = 7) -> torch.Tensor:
    m = torch.zeros(k, k, dtype=torch.float64)
    for i, j in live_taps(mask_type, k):
        m[i, j] = 1.0
    return m


def masked_conv64(x: torch.Tensor, w: torch.Tensor, mask_type: str):
    """x [B, Cin, H, W], w [Cout, Cin, k, k] -> (y, cond) float64 [B, Cout, H, W]: stride 1, zero padding k // 2, live taps only"""
    b, cin, h, wd = x.shape
    k = w.shape[-1]
    c = k // 2
    x64, w64 = x.double(), w.double()
    xp = torch.zeros((b, cin, h + 2 * c, wd + 2 * c), dtype=torch.float64)
    xp[:, :, c:c + h, c:c + wd] = x64
    y = torch.zeros((b, w.shape[0], h, wd), dtype=torch.float64)
    cond = torch.zeros_like(y)
    for i, j in live_taps(mask_type, k):
        win = xp[:, :, i:i + h, j:j + wd]
        y += torch.einsum("bchw,oc->bohw", win, w64[:, :, i, j])
        cond += torch.einsum("bchw,oc->bohw", win.abs(), w64[:, :, i, j].abs())
    return y, cond


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).double()


def layer_step64(below_nhwc: torch.Tensor, weight: torch.Tensor, mask_type: str, scale: torch.Tensor, shift: torch.Tensor):
    """below_nhwc: bf16-valued [B, H, W, Cin] (what the kernel left for the layer below); weight f32 [C, Cin, 7, 7] (rounded to bf16 here,
    as the pack is); scale, shift f32 [C] -> (v, cond) float64 [B, H, W, C]: the value the kernel rounds to bf16 and stores"""
    y, cond = masked_conv64(below_nhwc.double().permute(0, 3, 1, 2), bf16(weight), mask_type)
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    v = y * sc + sh
    v = torch.where(v > 0, v, 0.2 * v)
    return v.permute(0, 2, 3, 1), (cond * sc.abs() + sh.abs()).permute(0, 2, 3, 1)


def head_step64(top_nhwc: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
    """top_nhwc bf16-valued [B, H, W, C]; weight f32 [K, C]; bias f32 [K] -> (logits, cond) float64 [B, H, W, K]"""
    t, w = top_nhwc.double(), bf16(weight)
    return t @ w.t() + bias.double(), t.abs() @ w.abs().t() + bias.double().abs()


def uniforms(b: int, h: int, w: int, seed: int, offset: int) -> np.ndarray:
    """float64 [b, h, w]: u of every pixel — element e = (b H + i) W + j is word e % 4 of counter offset + e // 4; u = (w >> 8) 2^-24"""
    n = b * h * w
    words = P.philox4x32_10(P.counters(offset, (n + 3) // 4), seed).reshape(-1)[:n]
    return ((words >> np.uint32(8)).astype(np.float64) * P.TWO_M24).reshape(b, h, w)


def draw64(logits: np.ndarray, u: np.ndarray):
    """logits [..., K] (f32 values), u [...] -> (pick int64 [...], margin float64 [...]): the smallest k whose running sum of
    exp(l - max) exceeds u * total, K - 1 when none does; margin = the distance of u from the nearer of the pick's two CDF boundaries
    (cdf[pick - 1] <= u < cdf[pick])"""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    cdf = np.cumsum(e, axis=-1) / e.sum(axis=-1, keepdims=True)
    k = l.shape[-1]
    pick = np.minimum((cdf <= u[..., None]).sum(axis=-1), k - 1)
    hi = np.take_along_axis(cdf, pick[..., None], axis=-1)[..., 0]
    lo = np.where(pick > 0, np.take_along_axis(cdf, np.maximum(pick - 1, 0)[..., None], axis=-1)[..., 0], 0.0)
    margin = np.minimum(np.where(pick > 0, u - lo, np.inf), np.where(pick < k - 1, hi - u, np.inf))
    return pick.astype(np.int64), margin
