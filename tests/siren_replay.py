"""A float64 numpy replica of csrc/siren.hip in the kernel's operation order, with the kernel's operand rounding (bf16 words where the
kernel rounds) and a per-element error bound carried through every stage.  Nothing here is tuned: each bound is the sum of

  f32 accumulation      n * 2^-24 * sum |a| |b| for a chain or a sum of n terms in any order (n = the terms + 8 for the folds)
  the sine's argument   |w| * (bound of pre) + 2^-24 |w pre| (the product's rounding), |sin'|, |cos'| <= 1, plus 4 * 2^-24 for the
                        library's sine / cosine (2 ulp at 1)
  a re-rounded word     `flip(x, e)`: the kernel rounds ITS value, at most e from the replica's x, to bf16.  If x is farther than e from
                        the nearest rounding boundary both round to the same word and the error is exactly 0; else one flip, at
                        most e + 2 spacings
  products              the factors' bounds times the other factor's magnitude (e.g. |mod| * w on d pre), plus 2^-24 per rounding.

`rounded=False` switches every bf16 rounding off: that is the reference's fp32 arithmetic in float64, which the host test compares
with the recorded reference outputs."""
import numpy as np

U = 2.0 ** -24


def rb(x):
    """float64 -> the nearest bfloat16 (ties to even), as float64"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def flip(x, e):
    """bound of |bf16(x') - bf16(x)| over |x' - x| <= e"""
    ax = np.abs(x)
    spacing = np.where(ax > 0, 2.0 ** (np.floor(np.log2(np.maximum(ax, 1e-300))) - 7.0), 0.0)
    d = np.abs(x - rb(x))
    # to the nearest rounding boundary; below a power of two the boundary sits at a quarter spacing, which the second term covers
    dist = np.maximum(np.minimum(spacing / 2 - d, d + spacing / 4), 0.0)
    return np.where(e >= dist, e * (1 + 2.0 ** -7) + 2 * spacing, 0.0)


class Replica:
    """weights: list of L float arrays [latent, in] and the head's; biases: list of L + 1 arrays or None; mods [L, B, latent]"""

    def __init__(self, weights, head_w, biases, w_first, w_hidden, rounded=True):
        self.W = [np.asarray(w, np.float64) for w in weights]
        self.Wh = np.asarray(head_w, np.float64)
        self.b = None if biases is None else [np.asarray(b, np.float64) for b in biases]
        self.w_first, self.w_hidden, self.rounded = float(w_first), float(w_hidden), rounded

    def _rb(self, x):
        return rb(x) if self.rounded else x

    def _flip(self, x, e):
        return flip(x, e) if self.rounded else e

    def forward(self, x, samp, mods):
        """x [M, in_dim], samp [M] sample of every row, mods [L, B, latent] -> (out, bound); keeps what the backward reads"""
        x, mods = np.asarray(x, np.float64), np.asarray(mods, np.float64)
        L, H = len(self.W), self.W[0].shape[0]
        self.x, self.samp, self.mods, self.keep = x, samp, mods, []
        hb = ehb = None
        for l in range(L):
            if l == 0:
                b0 = self.b[0] if self.b is not None else np.zeros(H)
                pre = x @ self.W[0].T + b0
                epre = (x.shape[1] + 1) * U * (np.abs(x) @ np.abs(self.W[0]).T + np.abs(b0))
            else:
                wb = self._rb(self.W[l])
                pre = hb @ wb.T
                epre = ehb @ np.abs(wb).T + H * U * (np.abs(hb) @ np.abs(wb).T)
                if self.b is not None:
                    pre = pre + self.b[l]
                    epre = epre + U * np.abs(pre)
            w = self.w_first if l == 0 else self.w_hidden
            arg = w * pre
            earg = abs(w) * epre + U * np.abs(arg)
            s, c = np.sin(arg), np.cos(arg)
            es = earg + 4 * U
            m = mods[l][samp]
            hf = s * m
            ehf = es * np.abs(m) + U * np.abs(hf)
            hb, ehb = self._rb(hf), self._flip(hf, ehf)
            self.keep.append(dict(S=self._rb(s), eS=self._flip(s, es), C=self._rb(c), eC=self._flip(c, es), m=m))
        whb = self._rb(self.Wh)
        out = hb @ whb.T
        eout = ehb @ np.abs(whb).T + H * U * (np.abs(hb) @ np.abs(whb).T)
        if self.b is not None:
            out = out + self.b[L]
            eout = eout + U * np.abs(out)
        return out, eout

    def backward(self, dy):
        """dy [M, out_dim] -> {name: (value, bound)}: w<l>, b<l>, wh, bh, dmods [L, B, latent], dx [M, in_dim]"""
        dy = np.asarray(dy, np.float64)
        L, H, M = len(self.W), self.W[0].shape[0], dy.shape[0]
        B = self.mods.shape[1]
        onehot = np.zeros((B, M))
        onehot[self.samp, np.arange(M)] = 1.0
        rows = onehot.sum(1)[:, None] + 8
        nsum = M + 8
        res = {}
        dh = dy @ self.Wh
        edh = dy.shape[1] * U * (np.abs(dy) @ np.abs(self.Wh))
        res["bh"] = (dy.sum(0), nsum * U * np.abs(dy).sum(0))
        dmods, edmods = np.zeros_like(self.mods), np.zeros_like(self.mods)
        for l in range(L - 1, -1, -1):
            k = self.keep[l]
            S, eS, C, eC, m = k["S"], k["eS"], k["C"], k["eC"], k["m"]
            w = self.w_first if l == 0 else self.w_hidden
            q = dh * S
            eq = edh * np.abs(S) + np.abs(dh) * eS + U * np.abs(q)
            dmods[l] = onehot @ q
            edmods[l] = onehot @ eq + rows * U * (onehot @ np.abs(q))
            dp = dh * m * w * C
            edp = edh * np.abs(m * w * C) + np.abs(dh * m * w) * eC + 3 * U * np.abs(dp)
            res[f"b{l}"] = (dp.sum(0), edp.sum(0) + nsum * U * np.abs(dp).sum(0))
            if l == L - 1:
                hh = S * m
                ehh = eS * np.abs(m) + U * np.abs(hh)
                res["wh"] = (dy.T @ hh, np.abs(dy).T @ ehh + nsum * U * (np.abs(dy).T @ np.abs(hh)))
            dpb, edpb = self._rb(dp), self._flip(dp, edp)
            if l >= 1:
                kp = self.keep[l - 1]
                hpf = kp["S"] * kp["m"]
                hp, ehp = self._rb(hpf), self._flip(hpf, kp["eS"] * np.abs(kp["m"]) + U * np.abs(hpf))
                res[f"w{l}"] = (dpb.T @ hp, edpb.T @ np.abs(hp) + np.abs(dpb).T @ ehp + edpb.T @ ehp + (M + 16) * U * (np.abs(dpb).T @ np.abs(hp)))
                wb = self._rb(self.W[l])
                dh = dpb @ wb
                edh = edpb @ np.abs(wb) + H * U * (np.abs(dpb) @ np.abs(wb))
            else:
                ax = np.abs(self.x)
                res["w0"] = (dp.T @ self.x, edp.T @ ax + nsum * U * (np.abs(dp).T @ ax))
                res["dx"] = (dp @ self.W[0], edp @ np.abs(self.W[0]) + (H + 8) * U * (np.abs(dp) @ np.abs(self.W[0])))
        res["dmods"] = (dmods, edmods)
        return res


def from_state(state, prefix, num_layers, bias, w_first=30.0, w_hidden=1.0, rounded=True):
    """the Replica of a Siren whose parameters sit in `state` under `prefix` (torch tensors)"""
    f = lambda k: state[prefix + k].detach().double().cpu().numpy()  # noqa: E731
    weights = [f(f"blocks.{i}.weight") for i in range(num_layers)]
    biases = [f(f"blocks.{i}.bias") for i in range(num_layers)] + [f("head.bias")] if bias else None
    return Replica(weights, f("head.weight"), biases, w_first, w_hidden, rounded)
