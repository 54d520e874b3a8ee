"""A float64 replica of the basis kernels of csrc/nbm.hip, in their operation order, with each bf16 rounding switchable, and the
per-element error bounds that follow from that order (all in units of u = 2^-24, the form `helpers.assert_elementwise` takes:
|got - want| <= 1 ulp(want) + 1 * u * bound).

Forward, per row m, basis g (header of csrc/nbm.hip):
  pre1 = u . w1 + b1 in f32 (o roundings): e1 = (o + 1) u (|u| . |w1| + |b1|); with the dyadic operands of nbm_weights.kernel_case
         it is exact, the replica then sees the kernel's own h1 = relu(pre1) and splits it into the same two words;
  h1   = max(pre1, 0) enters the products as two bf16 words hi + lo (`two_words`);
  pre2 = MFMA chain over 2 Kp / 32 instructions (f32 accumulation of exact bf16 products) + b2: e2 = (2 Kp + 2) u (|h1| . |W2| + |b2|);
  bases = per-lane fma chain over NT terms, 4 folds, + b3: error <= sum_j |w3_j| e2_j + (NT + 6) u (sum_j |h2_j w3_j| + |b3|).
         A unit whose pre2 lies within e2 of zero may be live on one side only: its h2 differs by at most e2 — inside the first term.

Backward.  dpre2 = [pre2 > 0] dbases w3 (exact for the dyadic operands) is rounded to bf16 as the MFMA operand of dh1 and dW2; the
sums over rows run in f32 in a fixed order of at most M + 8 additions.  A unit (m, g, j) with |pre2| <= e2 — the zero band — may have
its mask flipped: dpre2 there changes by at most F = |dbases w3_j| (1 + 2^-8), and every output's bound carries the magnitude of that
change pushed through the same products (`flip` terms below), so no element is excluded:
  db3          (M + 8) u sum |dbases|
  db2_j        (M + 8) u sum_m |dpre2|                                + sum_m F
  dw3_j        (M + 8) u sum_m |dbases h2| + sum_m |dbases| e2        (a flipped unit has h2 <= e2)
  dW2_jk       (2 M + 8) u sum_m |dpre2 h1|                           + sum_m F h1_k
  dh1_mk       (Kp + 2) u sum_j |dpre2 W2_jk|                         + sum_j F |W2_jk|            =: E (dpre1 = [pre1 > 0] dh1: E where live)
  db1_k        (M + 8) u sum_m |dpre1|                                + sum_m E
  dw1_kj       (M + 9) u sum_m |dpre1 u_j|                            + sum_m E |u_j|
  du_mj (per g) (NT + 6) u sum_k |dpre1 w1_kj|                        + sum_k E |w1_kj|
  dx_bf        sum over its (g, d, j) of the du bounds + (NB + D o) u sum |du|
The layer-1 mask [pre1 > 0] is exact with the dyadic operands; `zero_band_share` also reports |pre1| <= e1 for general ones."""
import torch

U = 2.0 ** -24


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).double()


def two_words(t: torch.Tensor) -> torch.Tensor:
    """hi + lo, hi = bf16(t), lo = bf16(t - hi) (float64 sum of the two words the kernel multiplies)"""
    hi = bf16_round(t)
    return hi + bf16_round(t - hi)


def _kp(h: int) -> int:
    return (h + 31) // 32 * 32


def _nt(h: int) -> int:
    return (h + 15) // 16


def gather(x: torch.Tensor, idx) -> torch.Tensor:
    """u float64 [B, D, o]"""
    return x.double()[:, torch.as_tensor(idx, dtype=torch.long)]


class Replay:
    """forward and backward of the bases in float64.  round_h1 (to two words) / round_w2 / round_dp2: the bf16 roundings of the kernels."""

    def __init__(self, case: dict, round_h1: bool = True, round_w2: bool = True, round_dp2: bool = True):
        d64 = lambda t: t.detach().cpu().double()  # noqa: E731
        self.idx = case["idx"]
        self.x, self.w1, self.b1, self.b2, self.w3, self.b3 = (d64(case[k]) for k in ("x", "w1", "b1", "b2", "w3", "b3"))
        self.w2 = bf16_round(case["w2"].detach().cpu()) if round_w2 else d64(case["w2"])
        self.round_dp2 = round_dp2
        nb, h, o = self.w1.shape
        self.nb, self.h, self.o = nb, h, o
        b, f = self.x.shape
        self.u = gather(self.x, self.idx).reshape(-1, o)                                         # [M, o]
        self.m = self.u.shape[0]
        self.b, self.f, self.d = b, f, len(self.idx)
        self.pre1 = torch.einsum("mo,gko->mgk", self.u, self.w1) + self.b1                        # [M, NB, H]
        self.e1 = (o + 1) * U * (torch.einsum("mo,gko->mgk", self.u.abs(), self.w1.abs()) + self.b1.abs())
        h1 = self.pre1.clamp_min(0)
        self.h1 = two_words(h1) if round_h1 else h1
        self.pre2 = torch.einsum("mgk,gjk->mgj", self.h1, self.w2) + self.b2
        self.e2 = (2 * _kp(h) + 2) * U * (torch.einsum("mgk,gjk->mgj", self.h1.abs(), self.w2.abs()) + self.b2.abs())
        self.h2 = self.pre2.clamp_min(0)
        self.bases = torch.einsum("mgj,gj->mg", self.h2, self.w3) + self.b3
        self.band = self.pre2.abs() <= self.e2                                                    # the zero band of layer 2

    def zero_band_share(self) -> float:
        near1 = (self.pre1.abs() <= self.e1) & (self.pre1 != 0)
        return max(float(self.band.double().mean()), float(near1.double().mean()))

    def bases_bound(self) -> torch.Tensor:
        """units of u"""
        carry = torch.einsum("mgj,gj->mg", self.e2, self.w3.abs()) / U
        return carry + (_nt(self.h) + 6) * (torch.einsum("mgj,gj->mg", self.h2, self.w3.abs()) + self.b3.abs())

    def backward(self, dbases: torch.Tensor):
        """(grads, bounds): dicts over dw1, db1, dw2, db2, dw3, db3, dx; bounds in units of u"""
        m, nb, h, o = self.m, self.nb, self.h, self.o
        dv = dbases.detach().cpu().double().reshape(m, nb)
        live2 = (self.pre2 > 0).double()
        dp2 = live2 * dv[:, :, None] * self.w3
        dp2m = bf16_round(dp2) if self.round_dp2 else dp2
        flip = self.band.double() * (dv[:, :, None] * self.w3).abs() * (1 + 2.0 ** -8)        # F [M, NB, H(j)]
        ksum = m + 8
        g, bd = {}, {}
        g["db3"] = dv.sum(0)
        bd["db3"] = ksum * dv.abs().sum(0)
        g["db2"] = dp2.sum(0)
        bd["db2"] = ksum * dp2.abs().sum(0) + flip.sum(0) / U
        g["dw3"] = (dv[:, :, None] * self.h2).sum(0)
        bd["dw3"] = ksum * (dv[:, :, None] * self.h2).abs().sum(0) + (dv.abs()[:, :, None] * self.e2).sum(0) / U
        g["dw2"] = torch.einsum("mgj,mgk->gjk", dp2m, self.h1)
        bd["dw2"] = (2 * m + 8) * torch.einsum("mgj,mgk->gjk", dp2m.abs(), self.h1.abs()) + torch.einsum("mgj,mgk->gjk", flip, self.h1.abs()) / U
        dh1 = torch.einsum("mgj,gjk->mgk", dp2m, self.w2)
        live1 = (self.pre1 > 0).double()
        err = live1 * ((_kp(h) + 2) * U * torch.einsum("mgj,gjk->mgk", dp2m.abs(), self.w2.abs())
                       + torch.einsum("mgj,gjk->mgk", flip, self.w2.abs()))                      # E [M, NB, H(k)], absolute
        dp1 = live1 * dh1
        g["db1"] = dp1.sum(0)
        bd["db1"] = ksum * dp1.abs().sum(0) + err.sum(0) / U
        g["dw1"] = torch.einsum("mgk,mo->gko", dp1, self.u)
        bd["dw1"] = (ksum + 1) * torch.einsum("mgk,mo->gko", dp1.abs(), self.u.abs()) + torch.einsum("mgk,mo->gko", err, self.u.abs()) / U
        du = torch.einsum("mgk,gko->mgo", dp1, self.w1)                                          # [M, NB, o]
        du_abs = torch.einsum("mgk,gko->mgo", dp1.abs(), self.w1.abs())
        du_bd = (_nt(h) + 6) * du_abs + torch.einsum("mgk,gko->mgo", err, self.w1.abs()) / U
        dx = torch.zeros(self.b, self.f, dtype=torch.float64)
        dx_bd = torch.zeros(self.b, self.f, dtype=torch.float64)
        dus, dua, dub = (t.sum(1).view(self.b, self.d, o) for t in (du, du_abs, du_bd))
        for di, pack in enumerate(self.idx):
            for j, col in enumerate(pack):
                dx[:, col] += dus[:, di, j]
                dx_bd[:, col] += dub[:, di, j] + (nb + self.d * o) * dua[:, di, j]
        g["dx"], bd["dx"] = dx, dx_bd
        return g, bd


def featurize(bases: torch.Tensor, wf: torch.Tensor, bf: torch.Tensor):
    """(feat float64 [B, D], bound in units of u): one fma chain over the NB bases, then the bias"""
    b64, w64 = bases.detach().cpu().double(), wf.detach().cpu().double().view(wf.shape[0], -1)
    feat = torch.einsum("bdg,dg->bd", b64, w64) + bf.detach().cpu().double()
    cond = torch.einsum("bdg,dg->bd", b64.abs(), w64.abs()) + bf.detach().cpu().double().abs()
    return feat, (b64.shape[2] + 1) * cond


def featurize_backward(dfeat: torch.Tensor, bases: torch.Tensor, wf: torch.Tensor):
    """(grads, bounds) over dbases (one product), dwf and dbf (sums over the B samples: at most B + 64 additions)"""
    df, b64, w64 = dfeat.detach().cpu().double(), bases.detach().cpu().double(), wf.detach().cpu().double().view(wf.shape[0], -1)
    k = df.shape[0] + 64
    g = {"dbases": df[:, :, None] * w64, "dwf": torch.einsum("bd,bdg->dg", df, b64), "dbf": df.sum(0)}
    bd = {"dbases": g["dbases"].abs(), "dwf": k * torch.einsum("bd,bdg->dg", df.abs(), b64.abs()), "dbf": k * df.abs().sum(0)}
    return g, bd
