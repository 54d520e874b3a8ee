"""float64 replica of ONE GRU step and ONE LSTM step, forward and backward, in PyTorch's definitions (gate order r, z, n and
i, f, g, o), written the way csrc/rnn.hip cuts the work: gx = x W_ih^T + b_ih comes in, gh = h W_hh^T + b_hh is formed here.

`h_mat` is the state as the matrix operand (the kernels round it to bf16 there and only there); it defaults to `h`.
The backward functions take the gate values the forward returned, as the kernels take the ones they saved, and return
(dgx, dgh, dh_prev[, dc_prev]); `dgh_mat` likewise stands for dgh as the operand of the carry product dgh W_hh.

The `*_bound` functions return the forward error model of the kernels in units of 2^-24 (u), element by element, from the operation
order in the header of csrc/rnn.hip; the tests hand them to helpers.assert_elementwise as `cond` with k = 1."""
import torch


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def gru_step(gx, h, w_hh, b_hh, h_mat=None):
    hd = h.shape[1]
    gh = (h if h_mat is None else h_mat) @ w_hh.t() + b_hh
    r = _sig(gx[:, :hd] + gh[:, :hd])
    z = _sig(gx[:, hd:2 * hd] + gh[:, hd:2 * hd])
    ghn = gh[:, 2 * hd:]
    n = torch.tanh(gx[:, 2 * hd:] + r * ghn)
    return (1.0 - z) * n + z * h, (r, z, n, ghn)


def gru_step_bwd(dh, h, w_hh, gates, dgh_mat=None):
    r, z, n, ghn = gates
    dn = dh * (1.0 - z)
    dz = dh * (h - n)
    dnp = dn * (1.0 - n * n)
    dzp = dz * z * (1.0 - z)
    drp = dnp * ghn * r * (1.0 - r)
    dgx = torch.cat([drp, dzp, dnp], 1)
    dgh = torch.cat([drp, dzp, dnp * r], 1)
    return dgx, dgh, dh * z + (dgh if dgh_mat is None else dgh_mat) @ w_hh


def lstm_step(gx, h, c, w_hh, b_hh, h_mat=None):
    hd = h.shape[1]
    a = gx + (h if h_mat is None else h_mat) @ w_hh.t() + b_hh
    i, f, o = _sig(a[:, :hd]), _sig(a[:, hd:2 * hd]), _sig(a[:, 3 * hd:])
    g = torch.tanh(a[:, 2 * hd:3 * hd])
    cn = f * c + i * g
    return o * torch.tanh(cn), cn, (i, f, g, o)


def lstm_step_bwd(dh, dc, c_prev, c_new, w_hh, gates, dgh_mat=None):
    i, f, g, o = gates
    tc = torch.tanh(c_new)
    dcc = dc + dh * o * (1.0 - tc * tc)
    dgx = torch.cat([dcc * g * i * (1.0 - i), dcc * c_prev * f * (1.0 - f), dcc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], 1)
    return dgx, dgx, (dgx if dgh_mat is None else dgh_mat) @ w_hh, dcc * f


# ---- error model of the forward kernels, in units of u = 2^-24 ------------------------------------------------------------------------
# pre-activation a = gx + (sum_k h_k w_k + b): H additions of exact products, the bias and the gx add -> (H + 2) u on the sum of the
# absolute values.  sig = rcp(1 + exp2(-a log2 e)): the argument's rounding moves sig by |a| sig (1 - sig) u <= 0.23 u, exp2 and rcp are
# 1 ulp (2 u relative) each, the add 1 u: <= 4 u absolute, and |sig'| <= 1 / 4.  tanh = 1 - 2 rcp(1 + exp2(2 a log2 e)): <= 9 u
# absolute by the same count (0.45 + 1 + 2 + 4 + 1), |tanh'| <= 1.
SIG_U, TANH_U = 4.0, 9.0


def _pre_bound(gx, h_mat, w_hh, b_hh):
    return (h_mat.shape[1] + 2) * (gx.abs() + h_mat.abs() @ w_hh.abs().t() + b_hh.abs())


def gru_bound(gx, h, w_hh, b_hh, h_mat, gates):
    hd = h.shape[1]
    r, z, n, ghn = gates
    e = _pre_bound(gx, h_mat, w_hh, b_hh)
    er, ez = e[:, :hd] / 4 + SIG_U, e[:, hd:2 * hd] / 4 + SIG_U
    arg = gx[:, 2 * hd:].abs() + (r * ghn).abs()
    en = e[:, 2 * hd:] + ghn.abs() * er + arg + TANH_U           # the fma's own rounding: u |arg|
    return (n.abs() + h.abs()) * ez + en + 3.0 * (n.abs() + h.abs())  # h' = (1 - z) n + z h: sub, mul, fma


def lstm_bound(gx, c, w_hh, b_hh, h_mat, gates):
    hd = c.shape[1]
    i, f, g, o = gates
    e = _pre_bound(gx, h_mat, w_hh, b_hh)
    ei, ef, eo = e[:, :hd] / 4 + SIG_U, e[:, hd:2 * hd] / 4 + SIG_U, e[:, 3 * hd:] / 4 + SIG_U
    eg = e[:, 2 * hd:3 * hd] + TANH_U
    ec = c.abs() * ef + ei + eg + 2.0 * (c.abs() + 1.0)          # c' = f c + i g: mul, fma
    return eo + ec + TANH_U + 1.0, ec                             # h' = o tanh(c'); and c' itself
