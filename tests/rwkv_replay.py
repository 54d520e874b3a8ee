"""float64 replica of the RWKV mixers in the recurrence form of csrc/rwkv.hip, forward and adjoints, and the per-element error bounds
of its f32 arithmetic.

The bounds.  u = 2^-24 is one f32 rounding.  A scan s[t] = lam s[t-1] + x[t] is evaluated by the kernel as fma chains over fixed chunks
(local scan, chunk-to-chunk carries, lam^(i+1) by repeated multiplication): the term x[s] of s[t] passes d = |t - s| steps, and whichever
way it takes, it meets at most d multiplications by a rounded power of the rounded lam and at most d + 2 roundings of a sum it is part
of.  With RL the relative error of the computed lam in units of u (lam = expf(-expf(w)), expf good to 1 ulp = 2 u: RL = 2 exp(w) + 2,
taken as 2 exp(w) + 3), its error is at most u |x[s]| lam^d ((RL + 1) d + 2).  Summed over s that is the SAME recurrence run on
absolute values, once plain (A) and once weighted by the step count (D[t] = lam (D[t-1] + A[t-1])):
    |error of s[t]|  <=  scan(errors of x)[t] + u ((RL + 2) D[t] + 6 A[t])          (`scan_error`; one unit of slack per count)
Everything else is elementwise: each product, sum, quotient counts u of its magnitude, expf 2 u, sigmoid(r) = 1 / (1 + expf(-r)) 4 u,
1 - sigmoid = expf(-r) sigmoid 7 u.  A bf16 output adds half a bf16 ulp, 2^-8 of the magnitude at most, an f32 output u of it.
Only first-order terms are kept: the largest count here is ~2 000 u = 1.2e-4, its square is far below the slack above."""
import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

U = 2.0 ** -24
HALF_BF16 = 2.0 ** -8  # half an ulp of a bf16 value z is at most z 2^-8
EPS = 1.0e-6
f64 = torch.float64


def scan(x: Tensor, lam: Tensor, reverse: bool = False) -> Tensor:
    """s[t] = lam s[t -+ 1] + x[t] over dim 1 of [B, T, L]; lam [L]"""
    out = torch.empty_like(x)
    s = torch.zeros_like(x[:, 0])
    steps = range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])
    for t in steps:
        s = lam * s + x[:, t]
        out[:, t] = s
    return out


def scan_steps(x: Tensor, lam: Tensor, reverse: bool = False) -> Tensor:
    """D[t] = sum_s lam^|t-s| |t-s| x[s] over the steps before (after, with `reverse`) t"""
    out = torch.empty_like(x)
    a = torch.zeros_like(x[:, 0])
    d = torch.zeros_like(a)
    steps = range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])
    for t in steps:
        d = lam * (d + a)
        a = lam * a + x[:, t]
        out[:, t] = d
    return out


def scan_error(x_abs: Tensor, x_err: Tensor, lam: Tensor, rl: Tensor, reverse: bool = False) -> Tuple[Tensor, Tensor]:
    """(A, E): the scan of the magnitudes and the bound of the docstring for the scan of values of magnitude <= x_abs, error <= x_err"""
    a = scan(x_abs, lam, reverse)
    return a, scan(x_err, lam, reverse) + U * ((rl + 2.0) * scan_steps(x_abs, lam, reverse) + 6.0 * a)


def decay_of(info_decay: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(lam, exp(w), RL) per channel"""
    w = info_decay.reshape(-1).to(f64)
    ew = w.exp()
    return (-ew).exp(), ew, 2.0 * ew + 3.0


def shift(x: Tensor) -> Tensor:
    return torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)


# ---- time mix ----------------------------------------------------------------------------------------------------------------------


def time_mix(x: Tensor, mixes) -> Tuple[list, list]:
    """([in_j], [bound_j]) for x [B, T, C] and mixes of C elements; the bound is for the bf16 output"""
    x = x.to(f64)
    xs = shift(x)
    outs, bounds = [], []
    for m in mixes:
        m = m.reshape(-1).to(f64)
        val = x * m + xs * (1.0 - m)
        mag = (x * m).abs() + (xs * (1.0 - m)).abs()
        err = 3.0 * U * mag  # the subtraction, the product, the fma
        outs.append(val)
        bounds.append(err + HALF_BF16 * (val.abs() + err))
    return outs, bounds


def time_mix_backward(ds, x: Tensor, mixes, out_bf16: bool) -> Dict[str, Tensor]:
    """dx, dm (one per mix) and their bounds from the gradients d_j [B, T, C] (exact inputs)"""
    x = x.to(f64)
    diff = x - shift(x)
    dx = torch.zeros_like(x)
    mag = torch.zeros_like(x)
    dms, dm_bounds = [], []
    rows = x.shape[0] * x.shape[1]
    for d, m in zip(ds, mixes):
        d, m = d.to(f64), m.reshape(-1).to(f64)
        nxt = torch.cat([d[:, 1:], torch.zeros_like(d[:, :1])], 1)
        dx = dx + d * m + nxt * (1.0 - m)
        mag = mag + (d * m).abs() + (nxt * (1.0 - m)).abs()
        dms.append((d * diff).sum((0, 1)))
        # one rounding of x - x', one per fma of the chain over the rows of a chunk and per add over the chunks: at most rows + 2 on a path
        dm_mag = (d * diff).abs().sum((0, 1))
        dm_bounds.append(U * (rows + 3.0) * dm_mag + U * dms[-1].abs())
    err = 7.0 * U * mag  # six terms, each with its (1 - m) rounding: at most seven roundings on a path
    half = HALF_BF16 if out_bf16 else U
    return dict(dx=dx, dx_bound=err + half * (dx.abs() + err), dm=dms, dm_bound=dm_bounds)


# ---- the WKV scan ------------------------------------------------------------------------------------------------------------------


def wkv_forward(k: Tensor, v: Tensor, r: Tensor, info_decay: Tensor) -> Dict[str, Tensor]:
    k, v, r = k.to(f64), v.to(f64), r.to(f64)
    lam, ew, rl = decay_of(info_decay)
    e = k.exp()
    a, a_err = scan_error(e, 2.0 * U * e, lam, rl)
    a_rel = a_err / (a + EPS) + U  # of a + eps
    n = e * v / (a + EPS)
    n_err = n.abs() * (5.0 * U + a_rel)
    b = scan(n, lam)
    b_abs, b_err = scan_error(n.abs(), n_err, lam, rl)
    sig = torch.sigmoid(r)
    y = sig * b
    y_err = sig * b_err + 5.0 * U * sig * b_abs
    return dict(k=k, v=v, r=r, lam=lam, ew=ew, rl=rl, e=e, a=a, n=n, b=b, sig=sig, y=y, a_err=a_err, a_rel=a_rel, b_abs=b_abs, b_err=b_err,
                a_bound=a_err + U * a, b_bound=b_err + U * b_abs, y_bound=y_err + HALF_BF16 * (y.abs() + y_err))


def wkv_backward(dy: Tensor, fw: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """dk, dv, dr [B, T, L], d_decay [L] and their bounds from dy (exact: it arrives as bf16) and `wkv_forward`'s record"""
    dy = dy.to(f64)
    lam, ew, rl = fw["lam"], fw["ew"], fw["rl"]
    e, v, a, b, n, sig = fw["e"], fw["v"], fw["a"], fw["b"], fw["n"], fw["sig"]
    q = 1.0 / (a + EPS)
    g = dy * sig
    G = scan(g, lam, True)
    da = -G * n * q
    H = scan(da, lam, True)
    dv = G * e * q
    dk = (G * v * q + H) * e
    dr = dy * b * sig * (1.0 - sig)
    prev = lambda t: torch.cat([torch.zeros_like(t[:, :1]), t[:, :-1]], 1)  # noqa: E731  (t >= 1 only: the t = 0 term is zero)
    dlam = (G * prev(b) + H * prev(a)).sum((0, 1))
    d_decay = dlam * (-lam * ew)
    # bounds
    q_rel = fw["a_rel"] + U
    n_rel = 4.0 * U + q_rel
    G_abs, G_err = scan_error(g.abs(), 5.0 * U * g.abs(), lam, rl, True)
    da_abs = G_abs * n.abs() * q
    da_err = G_err * n.abs() * q + da_abs * (n_rel + q_rel + 2.0 * U)
    H_abs, H_err = scan_error(da_abs, da_err, lam, rl, True)
    dv_mag = G_abs * e * q
    dv_err = G_err * e * q + dv_mag * (4.0 * U + q_rel)
    t1_mag = G_abs * v.abs() * q
    s_err = G_err * v.abs() * q + t1_mag * (q_rel + 2.0 * U) + H_err + U * (t1_mag + H_abs)
    dk_mag = (t1_mag + H_abs) * e
    dk_err = e * s_err + 3.0 * U * dk_mag
    dr_mag = dy.abs() * sig * (1.0 - sig)
    dr_err = dr_mag * (fw["b_err"] + 14.0 * U * fw["b_abs"])
    b_abs_p, b_err_p, a_p, a_err_p = prev(fw["b_abs"]), prev(fw["b_err"]), prev(a), prev(fw["a_err"])
    term_mag = G_abs * b_abs_p + H_abs * a_p
    term_err = G_err * b_abs_p + G_abs * b_err_p + H_err * a_p + H_abs * a_err_p + 2.0 * U * term_mag
    adds = dy.shape[0] + dy.shape[1] + 2.0  # the steps of a chunk, the chunks of a sample, the samples: fewer than T + B + 2 on a path
    dlam_mag = term_mag.sum((0, 1))
    dlam_err = term_err.sum((0, 1)) + adds * U * dlam_mag
    dd_err = lam * ew * (dlam_err + (rl + 4.0) * U * dlam_mag)

    def bf16_bound(val, err):
        return err + HALF_BF16 * (val.abs() + err)

    return dict(dk=dk, dv=dv, dr=dr, d_decay=d_decay, dlam=dlam, dk_bound=bf16_bound(dk, dk_err), dv_bound=bf16_bound(dv, dv_err),
                dr_bound=bf16_bound(dr, dr_err), d_decay_bound=dd_err + U * d_decay.abs())


class Wkv(torch.autograd.Function):
    """y = sigmoid(r) * wkv(k, v) in the recurrence form with the adjoints of `wkv_backward`: what `gradcheck` checks and what the
    module replicas below differentiate through"""

    @staticmethod
    def forward(ctx, k, v, r, info_decay):
        fw = wkv_forward(k, v, r, info_decay)
        ctx.fw, ctx.shape = fw, info_decay.shape
        return fw["y"]

    @staticmethod
    def backward(ctx, dy):
        bw = wkv_backward(dy, ctx.fw)
        return bw["dk"], bw["dv"], bw["dr"], bw["d_decay"].reshape(ctx.shape)


# ---- the modules, float64, from a state dict with the reference's keys ---------------------------------------------------------------


def mixed(x: Tensor, m: Tensor) -> Tensor:
    return x * m + shift(x) * (1.0 - m)


def token_mixer(x: Tensor, p: Dict[str, Tensor], prefix: str = "") -> Tensor:
    g = lambda name: p[prefix + name]  # noqa: E731
    k = mixed(x, g("time_mix_k")) @ g("key.weight").t()
    v = mixed(x, g("time_mix_v")) @ g("value.weight").t()
    r = mixed(x, g("time_mix_r")) @ g("receptance.weight").t()
    return Wkv.apply(k, v, r, g("info_decay")) @ g("output.weight").t()


def channel_mixer(x: Tensor, p: Dict[str, Tensor], prefix: str = "") -> Tensor:
    g = lambda name: p[prefix + name]  # noqa: E731
    kk = torch.relu(mixed(x, g("time_mix_k")) @ g("key.weight").t()) ** 2
    kv = kk @ g("value.weight").t()
    return torch.sigmoid(mixed(x, g("time_mix_r")) @ g("receptance.weight").t()) * kv


LN_EPS = 1.0e-6  # NormFactory("layer") of the reference: nn.LayerNorm(dim, eps=1e-6)


def encoder(x: Tensor, p: Dict[str, Tensor], num_layers: int, eps: float = LN_EPS) -> Tensor:
    """the pre-norm MixedStackedEncoder with rwkv mixers, LayerNorm, no pooler: blocks, then the head's LayerNorm"""
    ln = lambda t, pre: torch.nn.functional.layer_norm(t, t.shape[-1:], p[pre + "weight"], p[pre + "bias"], eps)  # noqa: E731
    for i in range(num_layers):
        pre = f"mixing_blocks.{i}."
        x = x + token_mixer(ln(x, pre + "token_norm."), p, pre + "token_mixing.")
        x = x + channel_mixer(ln(x, pre + "channel_norm."), p, pre + "channel_mixing.")
    return ln(x, "head.norms.0.")


def run_module(kind: str, state: Dict[str, Tensor], x: Tensor, dy: Tensor, num_layers: Optional[int] = None):
    """(y, dx, {name: gradient}) in float64 for the loss sum(y * dy)"""
    p = {k: v.detach().to(f64).requires_grad_(True) for k, v in state.items() if v.is_floating_point()}
    xg = x.detach().to(f64).requires_grad_(True)
    y = token_mixer(xg, p) if kind == "token" else channel_mixer(xg, p) if kind == "channel" else encoder(xg, p, int(num_layers))
    (y * dy.to(f64)).sum().backward()
    return y.detach(), xg.grad, {k: v.grad for k, v in p.items()}
