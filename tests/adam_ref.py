"""float64 reference of the fused Adam / AdamW update (csrc/elementwise.hip: adam_kernel, adam_dev_kernel) and its error model.

The kernels compute, per element and in f32,
    gg = g * gscale;  decoupled: pp = p * (1 - lr * wd)   else: gg += wd * p        (neither when wd == 0)
    m' = b1 * m + (1 - b1) * gg
    v' = b2 * v + (1 - b2) * gg * gg
    p' = pp - (lr / bc1) * (m' / (sqrt(v') * bc2_rsqrt + eps))
from eight f32 scalars.  `adam_ref` evaluates the same expressions in float64 ON THOSE f32 SCALAR VALUES (the scalars are
inputs of the kernel, not part of its arithmetic) and returns with every output its `cond`: the same expression on absolute
values, the quantity `helpers.assert_elementwise` scales its `k * 2^-24` term with.

Rounding counts (K_M, K_V, K_P: the `k` of the tests), from `adam_update` in the kernel source, which switches contraction off
and spells its fused multiply-adds out.  A sum inherits the larger count of its terms plus one, a product the sum of its
factors' counts plus one, an fma rounds once for its product and sum together:
  gg      2   g * gscale, fma(wd, p, gg)
  m'      5   gg (2), 1 - b1 (1), their product (1), the final sum (1); b1 * m (1) is the shorter branch
  v'      8   gg twice (4), 1 - b2 (1), two products (2), the final fma(b2, v, .) (1)
  p'     15   m' (5); the denominator 7 = v' through the square root (8 / 2), sqrtf, * bc2_rsqrt, + eps; the division (1);
              lr / bc1 (1); the final fma(-step_size, ., pp) (1); pp = p * fma(-lr, wd, 1) (2) is the shorter branch
sqrtf and the division are correctly rounded in device code (hipcc's default).  An IEEE f32 model of the kernel on the inputs of
`mixed_state`, over both decay forms and every scalar of the tests, needed k < 2 for each output."""
import math
from typing import NamedTuple, Tuple

import torch

K_M, K_V, K_P = 5, 8, 15
HYPER_NAMES = ("lr", "beta1", "beta2", "eps", "wd", "bc1", "bc2_rsqrt", "gscale")


def f32(x: float) -> float:
    """the float32 value a C `float` argument or an f32 tensor element takes for the Python float `x`"""
    return float(torch.tensor(x, dtype=torch.float32))


class Hyper(NamedTuple):
    lr: float
    beta1: float
    beta2: float
    eps: float
    wd: float
    bc1: float
    bc2_rsqrt: float
    gscale: float

    def tensor(self) -> torch.Tensor:
        return torch.tensor(list(self), dtype=torch.float32)


def hyper_capi(lr, beta1, beta2, eps, wd, step, gscale=1.0) -> Hyper:
    """The scalars adam_kernel receives from `cfhip_adam_step`: its float arguments, the float values of its double betas, and
    the bias corrections computed in double from the betas AS GIVEN: bc1 = (float)(1 - pow(beta1, step)),
    (float)(1 / sqrt(1 - pow(beta2, step))).  Call the entry with the same unrounded betas."""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return Hyper(f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd), f32(bc1), f32(1.0 / math.sqrt(bc2)), f32(gscale))


def hyper_fused(lr, beta1, beta2, eps, wd, step, gscale=1.0) -> Hyper:
    """The record `FusedAdam._fill_hyper` stores: Python-float arithmetic on the betas of the parameter group, every entry
    rounded on its way into the f32 tensor."""
    h = torch.zeros(8, dtype=torch.float32)
    h[0], h[1], h[2], h[3], h[4], h[7] = lr, beta1, beta2, eps, wd, gscale
    h[5] = 1.0 - beta1 ** step
    h[6] = 1.0 / math.sqrt(1.0 - beta2 ** step)
    return Hyper(*h.tolist())


def mixed_state(n: int, seed: int):
    """f32 p, g, m, v of `n` elements that cycle through five regimes with period 5 (coprime to the 4 lanes of a vector, so every
    f32x4 holds different ones): 0 unit scale; 1 gradients and moments near 1e-12; 2 g = m = v = 0; 3 values near 1e4; 4 zero
    first moment.  Magnitudes are scale * (0.25 + |N(0, 1)|) with random signs: nothing non-zero is small enough for a product of
    the update ((1 - beta2) g^2 included, also under grad_scale = 1/3) to fall below 2^-100."""
    gen = torch.Generator().manual_seed(seed)

    def mag():
        return 0.25 + torch.randn(n, generator=gen, dtype=torch.float64).abs()

    def signed():
        return mag() * (torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1)

    cls = torch.arange(n) % 5
    p, g, m, v = signed(), signed(), signed(), mag() ** 2
    tiny, big = cls == 1, cls == 3
    g[tiny], m[tiny], v[tiny] = g[tiny] * 1e-12, m[tiny] * 1e-12, v[tiny] * 1e-24
    for t in (g, m, v):
        t[cls == 2] = 0.0
    p[big], g[big], m[big], v[big] = p[big] * 1e4, g[big] * 1e4, m[big] * 1e4, v[big] * 1e8
    m[cls == 4] = 0.0
    return tuple(t.float() for t in (p, g, m, v))


def adam_ref(p, g, m, v, h, decoupled) -> Tuple[Tuple[torch.Tensor, torch.Tensor], ...]:
    """-> (p', cond_p), (m', cond_m), (v', cond_v) in float64 from float64 copies of the state and the scalars `h` (a Hyper or
    any 8-sequence in the order of HYPER_NAMES).  Give f32-rounded scalars for a kernel comparison, unrounded ones (bc1 =
    1 - beta1^t, bc2_rsqrt = 1 / sqrt(1 - beta2^t)) for the textbook update."""
    lr, b1, b2, eps, wd, bc1, bc2_rsqrt, gscale = (float(x) for x in h)
    p, g, m, v = (torch.as_tensor(t, dtype=torch.float64) for t in (p, g, m, v))
    gg, cgg = g * gscale, (g * gscale).abs()
    pp = p
    if wd != 0.0:
        if decoupled:
            pp = p * (1.0 - lr * wd)
        else:
            gg, cgg = gg + wd * p, cgg + abs(wd) * p.abs()
    m2 = b1 * m + (1.0 - b1) * gg
    cm = abs(b1) * m.abs() + abs(1.0 - b1) * cgg
    v2 = b2 * v + (1.0 - b2) * gg * gg
    cv = abs(b2) * v.abs() + abs(1.0 - b2) * cgg * cgg
    denom = torch.sqrt(v2) * bc2_rsqrt + eps
    step_size = lr / bc1
    p2 = pp - step_size * (m2 / denom)
    cp = pp.abs() + abs(step_size) * cm / denom
    return (p2, cp), (m2, cm), (v2, cv)
