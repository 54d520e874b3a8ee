"""The fused LayerNorm + pool kernels (csrc/pool_rows.hip) per element against float64, and MixedStackedEncoder with the "mean" and
"sequence" head poolers against the fixture recorded from the reference (tests/golden/head_poolers.pt).

Error model of the kernel cases, u = 2^-24, every term evaluated in float64 from the same inputs (`_reference`).  A row lives in
4 ceil(D / 256) registers per lane and is summed by a per-lane chain and six shuffle stages: `depth` = 4 ceil(D / 256) + 8 roundings.
  y (NORM form)  dy_ = (depth + 6) u cy, cy = 2 (|x| + |mean|) rstd |gamma| + |beta| (statistics and the affine map; plain form: 0)
  logit          E = sum_d |w| dy_ + (depth + 2) u (sum_d |y w| + |b_p|);  p has the relative error rp = 2 max_t E + 8 u (logit and lse)
  out            sum_t p dy_ + sum_t p |y| (rp + (4 T + 16) u): T accumulations and at most T rescales of the online softmax, the merge
  dlogit         p (e_s + e_c + (rp + 2 u)(|y . dout| + |out . dout|)), e_s / e_c the dot products' own errors (depth + 2 roundings on the
                 absolute products, plus the errors of y and of out)
  dy = p dout + dlogit w_p: rp p |dout| + (its dlogit term) |w_p| + 2 u (|p dout| + |dlogit w_p|)
  dx             the LayerNorm backward on g = dy gamma with cx = (|x| + |mean|) rstd:  rstd (e_g + mean e_g + |xhat| mean(e_g |xhat|))
                 + 2 (depth + 8) u rstd (|g| + mean |g| + cx mean(|g| cx)), then one rounding to x's dtype (plain form: dy's bound)
  dgamma, dbeta, dw_p, db_p: the sums over the B T rows of the addends' bounds plus B T u sum |addend| (any summation order); db_p is
                 zero in exact arithmetic and is held to that bound alone.
Worst measured error / (bound + the store's ulp) over all cases (MI355X): out 0.02, dx 0.50 (bf16 rows; 0.07 for f32 rows), dgamma 0.04,
dbeta 0.09, dw_p 0.001, db_p 0.000."""
import os

import pytest
import torch

from helpers import F32_EPS_HALF as U, assert_elementwise, guarded_ops, rel_l2, ulp_out

pytestmark = pytest.mark.gpu
DEV, EPS, CHUNK = "cuda:0", 1e-6, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, bf16 = torch.float32, torch.bfloat16

# (D, T, B, x dtype, NORM form, mode, b_p, chunk_rows, where the largest of logits spread over +-30 sits)
BASE = (96, 19, 3, f32, True, "sequence", True, CHUNK, None)
CASES = [(d, t, 3, f32, True, "sequence", True, CHUNK, None) for d in (8, 96, 260, 2048) for t in (1, 7, 8, 9, 19)]  # T around chunk, 2 chunk + 3
CASES += [BASE[:2] + (1,) + BASE[3:], BASE[:3] + (bf16,) + BASE[4:], BASE[:4] + (False,) + BASE[5:], BASE[:5] + ("mean", False) + BASE[7:],
          BASE[:4] + (False, "mean", False) + BASE[7:], BASE[:6] + (False,) + BASE[7:], BASE[:7] + (0, None),
          (260, 9, 3, bf16, True, "sequence", True, CHUNK, None), (2048, 9, 1, bf16, True, "mean", False, CHUNK, None),
          (96, 19, 3, f32, False, "sequence", True, CHUNK, "first"), (96, 19, 3, f32, False, "sequence", True, CHUNK, "last")]
_ID = lambda c: f"D{c[0]}-T{c[1]}-B{c[2]}-{'f32' if c[3] == f32 else 'bf16'}-{'norm' if c[4] else 'plain'}-{c[5]}{'+b' if c[6] else ''}-chunk{c[7]}{'-max-' + c[8] if c[8] else ''}"  # noqa: E731


def _inputs(case):
    d, t, b, dtype, norm, mode, bias, _, spread = case
    gen = torch.Generator().manual_seed(1000 * d + t)
    r = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    x = (r(b, t, d) * 1.5 + 0.25).to(dtype)
    w = r(d) * (2.0 / d ** 0.5) if mode == "sequence" else None
    if spread:  # plain form: logit = x[.., 0] + (small terms): -30 .. 30 over the rows, the largest in the first or the last chunk
        ramp = torch.linspace(-30.0, 30.0, t)
        x[:, :, 0] = ramp.flip(0) if spread == "first" else ramp
        w = r(d) * 0.01
        w[0] = 1.0
    return dict(x=x, gamma=1.0 + 0.2 * r(d) if norm else None, beta=0.2 * r(d) if norm else None, w=w,
                bp=r(1) if bias else None, dout=r(b, d))


def _reference(case, t_in):
    """float64: the torch composition with its autograd gradients, and the bounds of the module docstring (already in units of 1)"""
    d, t, b, _, norm, mode, _, _, _ = case
    depth = 4 * -(-d // 256) + 8
    leaf = lambda v: None if v is None else v.double().clone().requires_grad_()  # noqa: E731
    x, gamma, beta, w, bp = (leaf(t_in[k]) for k in ("x", "gamma", "beta", "w", "bp"))
    dout = t_in["dout"].double()
    y = torch.nn.functional.layer_norm(x, (d,), gamma, beta, EPS) if norm else x
    if mode == "sequence":
        logit = y @ w + (0.0 if bp is None else bp)
        p = torch.softmax(logit, 1)
        out = (p.unsqueeze(1) @ y).squeeze(1)
    else:
        p = torch.full((b, t), 1.0 / t, dtype=torch.float64)
        out = y.mean(1)
    out.backward(dout)
    want = dict(out=out.detach(), dx=x.grad, dgamma=None if gamma is None else gamma.grad, dbeta=None if beta is None else beta.grad,
                dw=None if w is None else w.grad, db=None if bp is None else torch.zeros(1, dtype=torch.float64))
    with torch.no_grad():
        xd, yd, p = x.detach(), y.detach(), p.detach()
        zero, one = torch.zeros_like(xd), torch.ones_like(xd)
        mean = xd.mean(2, keepdim=True)
        rstd = 1.0 / torch.sqrt(xd.var(2, unbiased=False, keepdim=True) + EPS) if norm else one[..., :1]
        xh = (xd - mean) * rstd if norm else zero
        cx = (xd.abs() + mean.abs()) * rstd if norm else zero
        e_y = (depth + 6) * U * (2 * cx * gamma.detach().abs() + beta.detach().abs()) if norm else zero
        wa = w.detach().abs() if w is not None else torch.zeros(d, dtype=torch.float64)
        E = e_y @ wa + (depth + 2) * U * (yd.abs() @ wa + (0.0 if bp is None else bp.detach().abs()))
        rp = 2 * E.max(1, keepdim=True).values + 8 * U  # [B, 1]
        pe = p.unsqueeze(2)
        b_out = (pe * e_y).sum(1) + (pe * yd.abs()).sum(1) * (rp + (4 * t + 16) * U)
        s2, c = yd @ dout.unsqueeze(2), (want["out"] * dout).sum(1).view(b, 1, 1)  # [B, T, 1], [B, 1, 1]
        e_s = e_y @ dout.abs().unsqueeze(2) + (depth + 2) * U * (yd.abs() @ dout.abs().unsqueeze(2))
        e_c = ((b_out * dout.abs()).sum(1) + (depth + 2) * U * (want["out"].abs() * dout.abs()).sum(1)).view(b, 1, 1)
        seq = 1.0 if mode == "sequence" else 0.0
        dl = seq * pe * (s2 - c)
        e_dl = seq * pe * (e_s + e_c + (rp.unsqueeze(2) + 2 * U) * (s2.abs() + c.abs()))
        do = dout.unsqueeze(1)
        dy = pe * do + dl * (w.detach() if w is not None else 0.0)
        e_dy = rp.unsqueeze(2) * pe * do.abs() + e_dl * wa + 2 * U * (pe * do.abs() + dl.abs() * wa)
        if norm:
            ga = gamma.detach().abs()
            e_g, g = e_dy * ga, dy.abs() * ga
            m = lambda v: v.mean(2, keepdim=True)  # noqa: E731
            b_dx = rstd * (e_g + m(e_g) + xh.abs() * m(e_g * xh.abs())) + 2 * (depth + 8) * U * rstd * (g + m(g) + cx * m(g * cx))
        else:
            b_dx = e_dy + zero
        n = b * t
        rows = lambda v: v.sum((0, 1))  # noqa: E731
        bound = dict(out=b_out, dx=b_dx,
                     dgamma=rows(e_dy * xh.abs() + dy.abs() * depth * U * cx) + n * U * rows((dy * xh).abs()),
                     dbeta=rows(e_dy) + n * U * rows(dy.abs()),
                     dw=rows(e_dl * yd.abs() + dl.abs() * e_y) + n * U * rows((dl * yd).abs()),
                     db=(rows(e_dl) + n * U * rows(dl.abs())).view(1))
    return want, bound


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_pool_rows_per_element(case, monkeypatch):
    from cflearn_amd import ops

    d, t, b, dtype, norm, mode, bias, chunk, _ = case
    t_in = _inputs(case)
    want, bound = _reference(case, t_in)
    g = guarded_ops(monkeypatch)
    dev = {k: None if v is None else g.poisoned(v.to(DEV)) for k, v in t_in.items()}
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)  # noqa: E731
    runs = []
    for _ in range(2):
        out, lse, mean, rstd = ops.pool_rows_fwd(dev["x"], dev["gamma"], dev["beta"], EPS, mode, dev["w"], dev["bp"], chunk_rows=chunk)
        dests = dict(dgamma=nan(d) if norm else None, dbeta=nan(d) if norm else None, dpool_w=nan(d) if mode == "sequence" else None,
                     dpool_b=nan(1) if bias else None)
        dx = ops.pool_rows_bwd(dev["dout"], out, lse, dev["x"], dev["gamma"], dev["beta"], mean, rstd, mode, dev["w"], dev["bp"],
                               chunk_rows=chunk, **dests)
        runs.append(dict(out=out, dx=dx, dgamma=dests["dgamma"], dbeta=dests["dbeta"], dw=dests["dpool_w"], db=dests["dpool_b"]))
    g.check()
    for k, ref in want.items():
        if ref is None:
            continue
        got = runs[0][k]
        assert torch.equal(got, runs[1][k]), f"{k}: a repeated call differs"
        out_dtype, ulps = dtype if k == "dx" else f32, 0 if k == "db" else 1  # the store's own rounding on top of the model
        err = (got.double().cpu().reshape(ref.shape) - ref).abs()
        full = (bound[k] + ulps * ulp_out(ref.abs(), out_dtype)).clamp_min(1e-300)
        print(f"{k}: worst error / bound {(err / full).max().item():.3f}")
        assert_elementwise(got.reshape(ref.shape), ref, out_dtype=out_dtype, ulps=ulps, cond=bound[k], k=1.0 / U, what=k)


def test_gradient_destinations_write_accumulate_null():
    from cflearn_amd import ops

    t_in = {k: None if v is None else v.to(DEV) for k, v in _inputs(BASE).items()}
    x, gamma, beta, w, bp, dout = (t_in[k] for k in ("x", "gamma", "beta", "w", "bp", "dout"))
    out, lse, mean, rstd = ops.pool_rows_fwd(x, gamma, beta, EPS, "sequence", w, bp, chunk_rows=CHUNK)
    names = ("dgamma", "dbeta", "dpool_w", "dpool_b")

    def run(fill, accumulate=(), only=names, want_dx=True):
        dests = {k: torch.full((1 if k == "dpool_b" else 96,), fill, device=DEV) for k in only}
        dx = ops.pool_rows_bwd(dout, out, lse, x, gamma, beta, mean, rstd, "sequence", w, bp, want_dx=want_dx, accumulate=accumulate,
                               chunk_rows=CHUNK, **dests)
        return dx, dests

    dx, written = run(float("nan"))
    _, added = run(1.0, accumulate=("dgamma", "dpool_b"))  # two are added to, two written, in one call
    for k in names:
        want = written[k] + 1.0 if k in ("dgamma", "dpool_b") else written[k]  # one f32 addition of the same sum: the same bits
        assert torch.equal(added[k], want), k
    dx_none, alone = run(float("nan"), only=("dpool_w",), want_dx=False)  # null destinations and no dx: the rest is unchanged
    assert dx_none is None and torch.equal(alone["dpool_w"], written["dpool_w"])
    dx_only, _ = run(0.0, only=())
    assert torch.equal(dx_only, dx)


@pytest.mark.parametrize("pooler", ["mean", "sequence"])
def test_encoder_vs_reference(pooler, monkeypatch):
    """output, dx and every parameter gradient within 1.1 x the reference's own bf16-autocast distance from its fp32 run.  Two entries
    have no such yardstick (tools/gen_pool_golden.py): the mean pooler's head-norm bias gradient is sum_b dy in the reference, exact in
    f32, where the kernel adds the B T rounded addends dy / T: per element within (B T + 2) 2^-24 sum_b |dy|; the gradient of the
    sequence pooler's projection bias is zero in exact arithmetic: the B T roundings of its sum stay below 1e-4 of the largest entry of
    the projection weight's gradient, the same addends times |y| ~ 1.  Then, with the projection frozen, no destination is handed to
    the backward for it (the kernel skips the reduce of a null destination) and its `.grad` stays None."""
    import cflearn_amd as C
    from cflearn_amd import ops

    fx = torch.load(os.path.join(ROOT, "tests", "golden", "head_poolers.pt"), map_location="cpu", weights_only=False)
    rec = fx["modules"][pooler]
    net = C.MixedStackedEncoder(**fx["kwargs"], head_pooler=pooler)
    net.load_state_dict({**fx["stack_sd"], **rec["sd"]}, strict=True)
    net = net.to(DEV)
    x = rec["x"].to(DEV).requires_grad_()
    y = net(x)
    assert y.dtype == f32 and tuple(y.shape) == tuple(rec["y"].shape)
    (y * rec["dy"].to(DEV)).sum().backward()
    late = []
    for name, got, ref, dist in [("y", y, rec["y"], rec["y_dist"]), ("dx", x.grad, rec["dx"], rec["dx_dist"])] + [
            (k, p.grad, rec["grads"][k], rec["grad_dist"][k]) for k, p in net.named_parameters()]:
        got = got.detach().float().cpu()
        got = got[::4] if got.shape != ref.shape else got  # (large gradients are recorded as every fourth row)
        if name.endswith("projection.linear.bias"):
            ok, err = float(got.abs().max()) <= 1e-4 * float(rec["grads"]["head.module.projection.linear.weight"].abs().max()), float(got.abs().max())
        elif dist == 0.0:
            bt = rec["x"].shape[0] * rec["x"].shape[1]
            ok, err = bool(((got - ref).abs() <= (bt + 2) * U * rec["dy"].abs().sum(0)).all()), float((got - ref).abs().max())
        else:
            err = rel_l2(got, ref)
            ok = err <= 1.1 * dist
        print(f"{pooler} {name}: {err:.3e} (reference under bf16 autocast {dist:.3e})")
        if not ok:
            late.append(f"{name}: {err:.3e} against {dist:.3e}")
    assert not late, f"{len(late)} tensors outside 1.1 x their yardstick:\n" + "\n".join(late)
    if pooler == "sequence":
        proj = net.head.module.projection.linear
        proj.weight.requires_grad_(False), proj.bias.requires_grad_(False)
        net.zero_grad(set_to_none=True)
        calls, real = [], ops.pool_rows_bwd
        monkeypatch.setattr(ops, "pool_rows_bwd", lambda *a, **kw: calls.append(kw) or real(*a, **kw))
        net(rec["x"].to(DEV)).sum().backward()
        assert len(calls) == 1 and "dpool_w" not in calls[0] and "dpool_b" not in calls[0] and "dgamma" in calls[0]
        assert proj.weight.grad is None and proj.bias.grad is None and net.head.norms[0].weight.grad is not None
