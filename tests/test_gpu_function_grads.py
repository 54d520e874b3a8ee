"""Every autograd Function of the package, per element against float64, under partial freezing.

The cases, their float64 references and their error models live in tests/function_cases.py.  Each case runs with all of its
differentiable inputs asking for a gradient and with each one alone; cases with parameters run in three parameter modes:
  direct    a leaf f32 nn.Parameter whose `.grad` is None: the Function writes the gradient itself;
  returned  the parameter handed in as a non-leaf (`p * 1`): the Function must return the gradient; a frozen parameter arrives as a
            no-grad view of a trainable leaf, which must NOT be resolved to that leaf;
  arena     the parameters in an `optim.ParamArena` whose gradient storage holds a sentinel, `zero_grad(lazy=True)` before each of
            two backward passes: every requested gradient is overwritten, a frozen parameter's slot keeps the sentinel bit for bit.
The forward output and every requested gradient are compared per element (`assert_elementwise`); an input that asked for nothing has
no gradient, a frozen parameter is not claimed and not changed; a second pass without zeroing adds (direct mode).  Outputs the wrappers
allocate sit between guards, floating inputs in NaN-surrounded buffers."""
import contextlib
import functools

import pytest
import torch

import function_cases as FC
from function_cases import BF16, CASES, F32
from helpers import assert_elementwise, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import contrastive as HC  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd import optim  # noqa: E402

SENTINEL = 12345.6787109375  # exactly representable in f32


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


@pytest.fixture(scope="module")
def one_process_group(tmp_path_factory):
    """the default process group of one rank (gloo, file store) for the gather over ranks"""
    import torch.distributed as dist

    made = False
    if not dist.is_initialized():
        store = dist.FileStore(str(tmp_path_factory.mktemp("pg") / "store"), 1)
        dist.init_process_group("gloo", store=store, rank=0, world_size=1)
        made = True
    yield
    if made:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# the float64 side, once per case
# ---------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def reference(name: str, which: str):
    """(vals, dys, ys, grads, bounds) of a case for the output gradient `which`: "one", "two" (another dy), "ones" (dy = 1)"""
    c = CASES[name]
    vals = c.make()
    ys0 = FC.as_tuple(c.ref(FC.values64(c, vals, grad=False)))
    if which == "ones":
        dys = [torch.ones_like(y) for y in ys0]
    else:
        dys = FC.make_dys(c, ys0, 1 if which == "one" else 2)
    ys, gs = FC.grads64(c, vals, dys)
    return vals, dys, ys, gs, FC.bounds(c, vals, dys, ys, gs)


def check(got, ref, bound, what):
    ulps, units, dtype = bound
    if isinstance(ulps, torch.Tensor):  # per element (0 where the reference is structurally zero, 1 elsewhere)
        ulps = ulps.reshape(-1)
    assert tuple(got.shape) == tuple(ref.shape) or got.numel() == ref.numel(), f"{what}: shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
    assert_elementwise(got.detach().reshape(ref.shape), ref, out_dtype=dtype, ulps=ulps, cond=units, k=1.0 if units is not None else 0.0, what=what)


# ---------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------


class Run:
    """one case on the device: the tensors handed to the call, the leaves whose `.grad` is read, the frozen parameters"""

    def __init__(self, c, on, mode, G):
        self.c, self.on, self.mode, self.G = c, set(on), mode, G
        self.dev = "cpu" if c.name == "gather_rows_with_grad" else "cuda"
        self.vals = c.make()
        self.t, self.leaves, self.frozen = {}, {}, {}
        self.arena = None
        plist = []
        for k, val in self.vals.items():
            if not isinstance(val, torch.Tensor):
                self.t[k] = val
            elif not val.is_floating_point():
                self.t[k] = G.index(val.to(self.dev)) if self.dev == "cuda" else val
            elif k in c.params:
                plist.append(k)
            else:
                dv = self._place(k, val)
                if k in c.diff:
                    dv.requires_grad_(k in self.on)
                    self.leaves[k] = dv
                self.t[k] = dv
        for k in plist:
            val = self.vals[k]
            if mode == "arena":
                p = torch.nn.Parameter(val.to(self.dev).clone())
                self.leaves[k] = self.t[k] = p
                continue
            p = torch.nn.Parameter(self._place(k, val))
            self.leaves[k] = p
            if mode == "returned":
                if k in self.on:
                    self.t[k] = p * 1
                else:
                    # a weight frozen on purpose: a view that does not require grad over the storage of a trainable leaf
                    self.t[k] = p.detach().view(p.shape)
                    assert self.t[k].is_leaf and not self.t[k].requires_grad and self.t[k]._is_view() and self.t[k].data_ptr() == p.data_ptr()
                    self.frozen[k] = p
            else:
                p.requires_grad_(k in self.on)
                self.t[k] = p
                if k not in self.on:
                    self.frozen[k] = p
        if mode == "arena" and plist:
            self.arena = optim.ParamArena([self.leaves[k] for k in plist], with_shadow=True)
            for k in plist:
                if k not in self.on:
                    self.leaves[k].requires_grad_(False)
                    self.frozen[k] = self.leaves[k]
            self.arena.flat_g.fill_(SENTINEL)
            self.arena.zero_grad(lazy=True)

    def _place(self, k, val):
        if self.dev == "cpu":
            return val.clone()
        if k in self.c.nhwc_in:  # the channels_last view a producing convolution hands on
            return self.G.poisoned(val.permute(0, 2, 3, 1).contiguous().to(self.dev)).permute(0, 3, 1, 2)
        return self.G.poisoned(val.to(self.dev))

    def forward(self):
        keep = HF.NHWC[0]
        HF.NHWC[0] = self.c.nhwc
        try:
            with (self.c.scope() if self.c.scope is not None else contextlib.nullcontext()):
                return FC.as_tuple(self.c.call(self.t))
        finally:
            HF.NHWC[0] = keep

    def backward(self, ys, dys, form="dense"):
        if form == "ones":
            sum(y.float().sum() for y in ys).backward()  # an expanded (stride-0) output gradient
        elif form == "f32":
            sum((y.float() * d.to(y.device, F32).reshape(y.shape)).sum() for y, d in zip(ys, dys)).backward()
        else:
            gs = [d.to(y.device, y.dtype).reshape(y.shape) for y, d in zip(ys, dys)]
            if form == "channels_last":
                gs = [g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g for g in gs]
            torch.autograd.backward(ys, gs)
        HF.SideStream.join()
        if self.dev == "cuda":
            torch.cuda.synchronize()

    def grad(self, k):
        g = self.leaves[k].grad
        assert g is not None, f"{self.c.name}: {k} asked for a gradient and has none"
        if self.arena is not None and k in self.c.params:
            assert g.data_ptr() == self.arena.grad_view(self.leaves[k]).data_ptr(), f"{k}: `.grad` left the arena"
        return g

    def check_values(self, ys, which, tag, outputs=True):
        _, _, rys, rgs, bnd = reference(self.c.name, which)
        if outputs:
            assert len(ys) == len(rys)
            for i, (y, r) in enumerate(zip(ys, rys)):
                assert y.dtype == self.c.out[i], f"{tag} y{i}: dtype {y.dtype}"
                check(y, r, bnd[f"y{i}"], f"{tag} y{i}")
        for k in self.c.diff:
            if k in self.on:
                check(self.grad(k), rgs[k], bnd[k], f"{tag} d{k}")

    def check_frozen(self, tag):
        for k in self.c.diff:
            if k in self.on:
                continue
            leaf = self.leaves[k]
            if k not in self.c.params:
                assert leaf.grad is None, f"{tag}: {k} asked for nothing and has a gradient"
                continue
            assert torch.equal(leaf.detach().cpu().reshape(-1), self.vals[k].reshape(-1)), f"{tag}: the frozen parameter {k} changed"
            if self.mode == "arena":
                slot = self.arena.grad_view(leaf)
                assert torch.equal(slot.cpu(), torch.full(slot.shape, SENTINEL)), f"{tag}: the gradient slot of the frozen parameter {k} was written"
                assert getattr(leaf, "_cfhip_fresh", None) is True, f"{tag}: the frozen parameter {k} was committed"
            else:
                assert leaf.grad is None, f"{tag}: the frozen parameter {k} was claimed (`.grad` set)"
                assert not getattr(leaf, "_cfhip_fresh", False), f"{tag}: the frozen parameter {k} carries a fresh mark"


def patterns(c):
    if len(c.diff) <= 1:
        return [("all", tuple(c.diff))]
    return [("all", tuple(c.diff))] + [(f"only_{k}", (k,)) for k in c.diff]


def modes(c):
    if c.modes is not None:
        return c.modes
    return ("direct", "returned", "arena") if c.params else ("plain",)


MIXING = ("mixing_block", "mixing_stack")  # their value checks walk the block link by link: test_mixing_* below
GRID = [pytest.param(n, pn, on, m, id=f"{n}-{pn}-{m}") for n in sorted(CASES) if CASES[n].refused is None and n not in MIXING
        for pn, on in patterns(CASES[n]) for m in modes(CASES[n])]


@pytest.mark.parametrize("name,pname,on,mode", GRID)
def test_function_gradients(G, request, name, pname, on, mode):
    c = CASES[name]
    if HC.GatherRowsWithGradFn in c.fns:
        request.getfixturevalue("one_process_group")
    tag = f"{name} [{pname}, {mode}]"
    run = Run(c, on, mode, G)
    ys = run.forward()
    if not c.diff:  # a forward-only Function
        run.check_values(ys, "one", tag)
        return
    dys1 = reference(name, "one")[1]
    run.backward(ys, dys1)
    run.check_values(ys, "one", tag)
    run.check_frozen(tag)
    if mode == "direct":
        # a second pass without zeroing: every parameter gradient is the sum of the two references — both passes' units, the two
        # roundings to f32 of the parts (2 units each on its |reference|) and the rounding of the sum (2 units on the parts again)
        dys2, _, rg2, b2 = reference(name, "two")[1:]
        _, _, _, rg1, b1 = reference(name, "one")
        run.backward(run.forward(), dys2)
        for k in c.params:
            if k in run.on:
                u1, u2 = (b[k][1] if b[k][1] is not None else 0.0 for b in (b1, b2))
                units = u1 + u2 + (2 * (b1[k][0] + b2[k][0]) + 2) * (rg1[k].abs() + rg2[k].abs())
                check(run.grad(k), rg1[k] + rg2[k], (1, units, F32), f"{tag} second pass, sum d{k}")
        run.check_frozen(tag + " second pass")
    if mode == "arena":
        run.arena.zero_grad(lazy=True)
        ys2 = run.forward()
        run.backward(ys2, reference(name, "two")[1])
        for k in c.params:
            if k in run.on:
                check(run.grad(k), reference(name, "two")[3][k], reference(name, "two")[4][k], f"{tag} after a lazy zero-grad d{k}")
        run.check_frozen(tag + " after a lazy zero-grad")


REFUSED = [n for n in sorted(CASES) if CASES[n].refused is not None]


@pytest.mark.parametrize("name", REFUSED)
def test_refused_combinations_raise(G, name):
    c = CASES[name]
    exc, text = c.refused
    run = Run(c, c.diff, "direct" if c.params else "plain", G)
    with pytest.raises(exc, match=text):
        run.forward()


def dy_forms(c):
    """a dense f32 dy, the expanded dy of `y.float().sum()` and, where an output is 4-D, a channels_last dy"""
    ys = FC.as_tuple(c.ref(FC.values64(c, c.make(), grad=False)))
    return ["f32", "ones"] + (["channels_last"] if any(y.dim() == 4 for y in ys) else [])


FORMS = [pytest.param(n, f, id=f"{n}-{f}") for n in sorted(CASES) if CASES[n].dy_forms and n not in MIXING for f in dy_forms(CASES[n])]


@pytest.mark.parametrize("name,form", FORMS)
def test_output_gradient_forms(G, request, name, form):
    """the all-on pattern under a dense f32 dy, the expanded dy of `y.float().sum()` and, for 4-D outputs, a channels_last dy: the
    same gradients within the same bounds as under a dense dy of the output's type"""
    c = CASES[name]
    if HC.GatherRowsWithGradFn in c.fns:
        request.getfixturevalue("one_process_group")
    run = Run(c, c.diff, modes(c)[0], G)
    ys = run.forward()
    which = "ones" if form == "ones" else "one"
    run.backward(ys, reference(name, which)[1], form)
    run.check_values(ys, which, f"{name} [dy {form}]")


def test_dy_forms_cover_every_family():
    fams = {c.family for c in CASES.values() if c.family}
    with_forms = {c.family for c in CASES.values() if c.dy_forms}
    # (families whose only cases are refused or forward-only have no backward to vary)
    assert fams - with_forms <= {"attn_wide"}, sorted(fams - with_forms)


# ---------------------------------------------------------------------------------------------
# TapedFn and _CheckpointFn: the same chain plain, as one taped node and checkpointed
# ---------------------------------------------------------------------------------------------


def test_taped_and_checkpointed_chain_bit_equal(G):
    results = {}
    for kind in ("plain", "taped", "checkpoint"):
        vals = FC.wrap_make()
        t = {"x": G.poisoned(vals["x"].cuda()).requires_grad_(True)}
        for k in FC.WRAP_PARAMS:
            t[k] = torch.nn.Parameter(G.poisoned(vals[k].cuda()))
        y = FC.wrap_call(kind, t)
        dy = FC.R(tuple(y.shape), 77, 1.0, BF16).cuda()
        y.backward(dy)
        HF.SideStream.join()
        torch.cuda.synchronize()
        assert all(t[k].grad is not None for k in t), kind
        results[kind] = {"y": y.detach().cpu(), **{k: t[k].grad.detach().cpu() for k in t}}
    for kind in ("taped", "checkpoint"):
        for k, want in results["plain"].items():
            assert torch.equal(results[kind][k], want), f"{kind}: {k} differs from the plain chain"


# ---------------------------------------------------------------------------------------------
# MixingBlockFn / MixingStackFn: the block walked link by link
# ---------------------------------------------------------------------------------------------
# The block stores its forward intermediates (ln1, qkv, o, x1, ln2, pre, h) in bf16 and hands them to backward: they are read from the
# node and every link is held against float64 ON THE INTERMEDIATE THE KERNELS ACTUALLY PRODUCED, at the model of that link's own case
# above (LayerNorm, Linear, attention, the GELU epilogue).  Backward intermediates are not observable; each link of the backward is
# linear in the gradient it receives, so the bound of a result is its own link's model plus the bound of the incoming gradient
# carried through the link on absolute values (|W| for a GEMM, the absolute LayerNorm / attention backward), plus the bf16 rounding
# of every intermediate gradient (dpre, dln2, dx1, d_o, dqkv, dln1): first order, nothing measured.

U = 2.0 ** -24
MIX_PATTERNS = [("all", ("x",) + FC.MIX_PARAMS), ("only_x", ("x",))] + [(f"only_{k}", (k,)) for k in FC.MIX_PARAMS]


def _rb(t):
    return 2.0 ** -8 * t.abs()


def _ln_parts(x, w, eps):
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return mu, rstd, (x - mu) * rstd


def _ln_fwd_err(x, w, b, eps):
    d = x.shape[-1]
    mu, rstd, xhat = _ln_parts(x, w, eps)
    return U * ((3 * d + 16) * ((x - mu).abs() + mu.abs() + x.abs()) * rstd * w.abs() + 2 * ((w * xhat).abs() + b.abs()))


def _ln_bwd64(dy, e_dy, x, w, eps, add, e_add):
    """(dx, e_dx, dgamma, e_dgamma, dbeta, e_dbeta) of LayerNorm backward with the fan-in gradient `add` folded in (function_cases._ln_err)"""
    d, m = x.shape[-1], x.shape[0]
    mu, rstd, xhat = _ln_parts(x, w, eps)
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True)) + add
    lab = lambda q, one: rstd * (q + q.mean(-1, keepdim=True) + (xhat.abs() + one) * (q * xhat.abs()).mean(-1, keepdim=True))  # noqa: E731
    e_dx = lab(e_dy * w.abs(), 0.0) + U * ((3 * d + 16) * lab(g.abs(), 1.0) * (1 + xhat.abs()) + add.abs()) + e_add
    xa = xhat.abs()
    dg, db = (dy * xhat).sum(0), dy.sum(0)
    e_dg = (e_dy * xa).sum(0) + U * ((m + 8) * (dy.abs() * xa).sum(0) + (3 * d + 16) * (dy.abs() * (xa + 1)).sum(0))
    e_db = e_dy.sum(0) + U * (m + 8) * dy.abs().sum(0)
    return dx, e_dx, dg, e_dg, db, e_db


def _mix_walk(saved, v, dy):
    """{name: (got bf16 intermediate, float64 link result, absolute bound)} of the forward, and {input: (reference gradient, bound)}"""
    from helpers import attn_k_product

    d, hid, eps, heads = FC.MIX["d"], FC.MIX["hid"], FC.MIX["eps"], FC.MIX["heads"]
    dh, t, bsz = d // heads, FC.MIX["t"], FC.MIX["b"]
    m = bsz * t
    c = lambda z: z.detach().cpu().double()  # noqa: E731
    x, ln1, qkv, o, x1, ln2, pre, h = (c(saved[i]) for i in (0, 3, 4, 5, 7, 10, 11, 12))
    w = {k: v[k].detach() for k in FC.MIX_PARAMS}
    kp = attn_k_product(dh, t)
    sc = 1.0 / dh ** 0.5
    q3 = qkv.view(bsz, t, 3 * d)
    sh = lambda z: z.reshape(bsz, t, heads, dh).transpose(1, 2)  # noqa: E731
    back = lambda z: z.transpose(1, 2).reshape(m, d)  # noqa: E731
    Q, K, V = sh(q3[..., :d]), sh(q3[..., d:2 * d]), sh(q3[..., 2 * d:])
    o_ref, p = FC._attn64(q3[..., :d], q3[..., d:2 * d], q3[..., 2 * d:], heads, dh)
    lin = lambda a, wt, b: (a @ wt.t() + b, a.abs() @ wt.abs().t() + b.abs())  # noqa: E731
    fwd = {}
    fwd["ln1"] = (ln1, FC._ln_ref(x, w["ln1_w"], w["ln1_b"], eps), _ln_fwd_err(x, w["ln1_w"], w["ln1_b"], eps))
    r, a = lin(ln1, w["in_w"], w["qkv_b"])
    fwd["qkv"] = (qkv, r, U * (d + 2) * a)
    fwd["o"] = (o, o_ref.reshape(m, d), U * kp * back(p @ V.abs()))
    r, a = lin(o, w["out_w"], w["out_b"])
    fwd["x1"] = (x1, r + x, U * (d + 3) * (a + x.abs()))
    fwd["ln2"] = (ln2, FC._ln_ref(x1, w["ln2_w"], w["ln2_b"], eps), _ln_fwd_err(x1, w["ln2_w"], w["ln2_b"], eps))
    r, a = lin(ln2, w["w1"], w["b1"])
    fwd["pre"] = (pre, r, U * (d + 2) * a)
    fwd["h"] = (h, FC.gelu64(pre), U * 8 * pre.abs() * (1 + pre * pre))  # of the pre-activation the kernel stored
    r, a = lin(h, w["w2"], w["b2"])
    fwd["y"] = (None, r + x1, U * (hid + 3) * (a + x1.abs()))
    # ---- backward, on the forward the kernels produced
    dy = dy.reshape(m, d)
    gr = {}
    A, Aa = dy @ w["w2"], dy.abs() @ w["w2"].abs()
    gp = FC.gelu_grad64(pre)
    dpre = A * gp
    e_dpre = _rb(dpre) + U * ((d + 1) * Aa * gp.abs() + 8 * A.abs() * pre.abs() * (1 + pre * pre))  # test_gpu_gemm_epilogues' GELU' model
    gr["w2"] = (dy.t() @ h, U * (m + 8) * (dy.abs().t() @ h.abs()))
    gr["b2"] = (dy.sum(0), U * (m + 8) * dy.abs().sum(0))
    gr["w1"] = (dpre.t() @ ln2, e_dpre.t() @ ln2.abs() + U * (m + 8) * (dpre.abs().t() @ ln2.abs()))
    gr["b1"] = (dpre.sum(0), e_dpre.sum(0) + U * (m + 8) * dpre.abs().sum(0))
    dln2 = dpre @ w["w1"]
    e_dln2 = e_dpre @ w["w1"].abs() + U * (hid + 1) * (dpre.abs() @ w["w1"].abs()) + _rb(dln2)
    dx1, e_dx1, dg, e_dg, db, e_db = _ln_bwd64(dln2, e_dln2, x1, w["ln2_w"], eps, dy, torch.zeros_like(dy))
    gr["ln2_w"], gr["ln2_b"] = (dg, e_dg), (db, e_db)
    e_dx1 = e_dx1 + _rb(dx1)
    gr["out_w"] = (dx1.t() @ o, e_dx1.t() @ o.abs() + U * (m + 8) * (dx1.abs().t() @ o.abs()))
    gr["out_b"] = (dx1.sum(0), e_dx1.sum(0) + U * (m + 8) * dx1.abs().sum(0))
    d_o = dx1 @ w["out_w"]
    e_do = e_dx1 @ w["out_w"].abs() + U * (d + 1) * (dx1.abs() @ w["out_w"].abs()) + _rb(d_o)
    # attention backward (helpers.assert_attn_backward's model) and the incoming bound through its absolute form
    dO, eO = sh(d_o.view(bsz, t, d)), sh(e_do.view(bsz, t, d))
    Oh = p @ V
    dP = dO @ V.transpose(-1, -2)
    dS = p * (dP - (dO * Oh).sum(-1, keepdim=True))
    cdS = p * (dO.abs() @ V.abs().transpose(-1, -2) + (dO.abs() * Oh.abs()).sum(-1, keepdim=True))
    edS = p * (eO @ V.abs().transpose(-1, -2) + (eO * Oh.abs()).sum(-1, keepdim=True))
    dq, dk, dv = back(dS @ K * sc), back(dS.transpose(-1, -2) @ Q * sc), back(p.transpose(-1, -2) @ dO)
    e_dq = U * 2 * kp * back(cdS @ K.abs() * sc) + back(edS @ K.abs() * sc)
    e_dk = U * 2 * kp * back(cdS.transpose(-1, -2) @ Q.abs() * sc) + back(edS.transpose(-1, -2) @ Q.abs() * sc)
    e_dv = U * kp * back(p.transpose(-1, -2) @ dO.abs()) + back(p.transpose(-1, -2) @ eO)
    dqkv = torch.cat([dq, dk, dv], 1)
    e_dqkv = torch.cat([e_dq, e_dk, e_dv], 1) + _rb(dqkv)
    gr["in_w"] = (dqkv.t() @ ln1, e_dqkv.t() @ ln1.abs() + U * (m + 8) * (dqkv.abs().t() @ ln1.abs()))
    gr["qkv_b"] = (dqkv.sum(0), e_dqkv.sum(0) + U * (m + 8) * dqkv.abs().sum(0))
    dln1 = dqkv @ w["in_w"]
    e_dln1 = e_dqkv @ w["in_w"].abs() + U * (3 * d + 1) * (dqkv.abs() @ w["in_w"].abs()) + _rb(dln1)
    dx, e_dx, dg, e_dg, db, e_db = _ln_bwd64(dln1, e_dln1, x, w["ln1_w"], eps, dx1, e_dx1)
    gr["ln1_w"], gr["ln1_b"] = (dg, e_dg), (db, e_db)
    gr["x"] = (dx, e_dx)
    return fwd, gr


def _mix_saved(y):
    """what the node keeps for backward (a stack whose call is being recorded as a launch plan keeps it with the plan)"""
    node = y.grad_fn
    return node.saved_tensors if len(node.saved_tensors) else node.plan.all_saved


@pytest.mark.parametrize("mode", ["direct", "arena"])
@pytest.mark.parametrize("pname,on", [pytest.param(p, o, id=p) for p, o in MIX_PATTERNS])
@pytest.mark.parametrize("name", MIXING)
def test_mixing_block_and_stack(G, name, pname, on, mode):
    c = CASES[name]
    tag = f"{name} [{pname}, {mode}]"
    run = Run(c, on, mode, G)
    v = FC.values64(c, run.vals, grad=False)
    (y,) = run.forward()
    saved = _mix_saved(y)
    ys0 = FC.as_tuple(c.ref(v))
    sums = {}
    # (arena: a third pass — a stack's first call runs plainly, its second is recorded as a launch plan, its third replays the plan)
    passes = (("one", 1), ("two", 2)) + ((("three", 3),) if mode == "arena" else ())
    for which, seed in passes:
        dy = FC.make_dys(c, ys0, seed)[0]
        fwd, gr = _mix_walk(saved, v, dy)
        for key, (got, want, e) in fwd.items():
            check(y.reshape(want.shape) if got is None else got, want, (1, e / U, BF16), f"{tag} pass {which} {key}")
        run.backward((y,), [dy])
        for k in run.on:
            ref, e = gr[k]
            dt = F32 if k in c.params else BF16
            if which == "two" and k in c.params and mode == "direct":  # no zeroing in between: the sum of the two passes
                ref, e = sums[k][0] + ref, sums[k][1] + e + U * 6 * (sums[k][0].abs() + ref.abs())
            check(run.grad(k), ref.reshape(run.vals[k].shape), (1, (e / U).reshape(run.vals[k].shape), dt), f"{tag} pass {which} d{k}")
            sums[k] = (ref, e)
        run.check_frozen(f"{tag} pass {which}")
        if which != passes[-1][0]:
            if mode == "arena":
                run.arena.zero_grad(lazy=True)
            else:
                run.leaves["x"].grad = None
            (y,) = run.forward()
            saved = _mix_saved(y)


@pytest.mark.parametrize("form", ["f32", "ones"])
@pytest.mark.parametrize("name", MIXING)
def test_mixing_output_gradient_forms(G, name, form):
    """the all-on pattern under a dense f32 dy and the expanded dy of `y.float().sum()`: the same walk, the same bounds"""
    c = CASES[name]
    run = Run(c, c.diff, "direct", G)
    v = FC.values64(c, run.vals, grad=False)
    (y,) = run.forward()
    ys0 = FC.as_tuple(c.ref(v))
    dy = torch.ones_like(ys0[0]) if form == "ones" else FC.make_dys(c, ys0, 1)[0]
    _, gr = _mix_walk(_mix_saved(y), v, dy)
    run.backward((y,), [dy], form)
    for k in c.diff:
        ref, e = gr[k]
        check(run.grad(k), ref.reshape(run.vals[k].shape), (1, (e / U).reshape(run.vals[k].shape), F32 if k in c.params else BF16),
              f"{name} [dy {form}] d{k}")


# ---------------------------------------------------------------------------------------------
# a view of a parameter taken under torch.no_grad() stands for itself, never for its base
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["linear_plain_mfma", "lora_linear", "time_proj"])
def test_no_grad_view_is_not_resolved_to_its_base(G, name):
    """the Functions that look through views of whole parameters (`whole_param`): a view cached under torch.no_grad() reaches them as a
    leaf of its own; the parameter behind it is neither claimed nor written, whatever the view itself receives"""
    c = CASES[name]
    run = Run(c, c.diff, "direct", G)
    bases = {}
    for k in c.params:
        base = run.leaves[k]
        with torch.no_grad():
            run.t[k] = base.view(base.shape)
        assert run.t[k]._is_view() and run.t[k]._base is base and run.t[k].is_leaf
        bases[k] = base
    ys = run.forward()
    run.backward(ys, reference(name, "one")[1])
    run.leaves = {k: v for k, v in run.leaves.items() if k not in bases}
    run.on -= set(bases)
    run.check_values(ys, "one", f"{name} [no-grad views]")
    for k, base in bases.items():
        assert base.grad is None and not getattr(base, "_cfhip_fresh", False), f"{name}: the parameter behind the view {k} was claimed"
        assert torch.equal(base.detach().cpu().reshape(-1), run.vals[k].reshape(-1)), f"{name}: the parameter behind the view {k} changed"
