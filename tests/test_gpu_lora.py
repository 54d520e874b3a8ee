"""LoRA adapters on the GPU: the three kernels of csrc/lora.hip per element against float64 (guarded outputs, poisoned inputs), then
`LoRALinearFn` / `LoRALinearHook` / `LoRAManager` against the reference's own numbers (tests/golden/lora_linear.pt).

Error models of the kernel tests (`assert_elementwise`: ulps = 1 of the output type, plus k f32 roundings times the same product on
absolute values):
  * lora_down: one MFMA accumulator per output over the whole reduction — a chain of at most K f32 additions of exact bf16 products —
    then the multiplication by the scale: k = K + 1; one rounding to bf16.
  * lora_up_add: a chain of r additions, then fma(scale, acc, y) — one rounding, which for f32 y is the output rounding: k = r + 1.
  * lora_wgrad: rows_per_split additions inside a split, splits - 1 ordered additions of the partial sums, the scale, the add into
    `out` when accumulating: k = rows_per_split + splits + 1.
With p > 0 the kernels multiply by scale / (1 - p) formed in f32: one more rounding (k + 1)."""
import pytest
import torch

from helpers import assert_close, assert_elementwise, guarded_ops

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import _lib, functional as HF, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# (M, K, N, r): every M of {1, 63, 394, 4100} (below one wave, one row short of a stripe, 2 x 197, several stripes per workgroup
# with a ragged tail), K of {40, 768}, N of {24, 200, 3072}, r of {1, 4, 16, 17, 64}; (394, 768, ., 64) and (63, ., 3072, 64) take
# the chunked-factor path of lora_down in its two factor layouts; N = 3072 spans 12 column blocks of lora_up_add / 48 of lora_wgrad
CASES = [(1, 40, 24, 1), (63, 40, 200, 4), (394, 768, 24, 64), (4100, 40, 200, 17), (63, 768, 3072, 64), (394, 40, 3072, 16),
         (4100, 768, 24, 4)]
SEED, OFFSET = 0x1234567, 7


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _mk(shape, seed, scale=1.0):
    """bf16-representable values"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(BF16)


def _strided(G, t, pad=8):
    """a device copy with a row stride larger than the row (the padding holds a sentinel) inside a guarded buffer"""
    v = G.out2d(t.shape[0], t.shape[1], t.shape[1] + pad, t.dtype, DEV)
    v.copy_(t.to(DEV))
    return v


def _keep(m, n, p):
    """the keep mask of ops.dropout at (SEED, OFFSET) over a contiguous [m, n]"""
    if p == 0.0:
        return torch.ones(m, n, dtype=torch.float64)
    _, mask = ops.dropout(torch.ones(m, n, dtype=F32, device=DEV), p, seed=SEED, offset=OFFSET, want_mask=True)
    return mask.cpu().double()


@pytest.mark.parametrize("m,k,n,r", CASES)
def test_lora_down_per_element(G, m, k, n, r):
    x, a = _mk((m, k), 1), _mk((r, k), 2, 0.25)
    s = 0.75
    h = ops.lora_down(_strided(G, x), G.poisoned(a.to(DEV)), scale=s)
    assert h.shape == (m, r) and h.dtype == BF16
    assert_elementwise(h, s * (x.double() @ a.double().t()), out_dtype=BF16, cond=s * (x.double().abs() @ a.double().abs().t()),
                       k=k + 1, what="h = x A^T")
    # the backward form: dh = s (mask . dy) Bm, factor [N, r], both with and without the mask
    dy, bm = _mk((m, n), 3), _mk((n, r), 4, 0.25)
    for p in (0.0, 0.25):
        keep = _keep(m, n, p)
        dh = ops.lora_down(_strided(G, dy), G.poisoned(bm.to(DEV)), f_trans=True, scale=s, p=p, seed=SEED, offset=OFFSET)
        sc = s / (1.0 - p)
        assert_elementwise(dh, sc * ((keep * dy.double()) @ bm.double()), out_dtype=BF16,
                           cond=sc * ((keep * dy.double().abs()) @ bm.double().abs()), k=n + 2, what=f"dh p={p}")


@pytest.mark.parametrize("ydt", [BF16, F32])
@pytest.mark.parametrize("m,k,n,r", CASES)
def test_lora_up_add_per_element(G, m, k, n, r, ydt):
    h, bm = _mk((m, r), 5), _mk((n, r), 6, 0.25)
    y0 = _mk((m, n), 7).to(ydt)
    s = 0.5
    prod, cond = h.double() @ bm.double().t(), h.double().abs() @ bm.double().abs().t()
    for p in (0.0, 0.25):
        keep = _keep(m, n, p)
        y = _strided(G, y0)
        ops.lora_up_add(y, G.poisoned(h.to(DEV)), G.poisoned(bm.to(DEV)), scale=s, p=p, seed=SEED, offset=OFFSET)
        sc = s / (1.0 - p)
        assert_elementwise(y, y0.double() + sc * keep * prod, out_dtype=ydt, cond=y0.double().abs() + sc * keep * cond, k=r + 2,
                           what=f"y += p={p}")
        got = y.cpu()
        dropped = keep == 0
        assert torch.equal(got[dropped].view(torch.int16 if ydt is BF16 else torch.int32),
                           y0[dropped].view(torch.int16 if ydt is BF16 else torch.int32)), "a dropped position of y changed"
    # the backward form on the dX the base GEMM wrote: dx += dh A, factor [r, K], no mask
    dh, a = _mk((m, r), 8), _mk((r, k), 9, 0.25)
    dx0 = _mk((m, k), 10).to(ydt)
    dx = _strided(G, dx0)
    ops.lora_up_add(dx, G.poisoned(dh.to(DEV)), G.poisoned(a.to(DEV)), f_trans=True)
    assert_elementwise(dx, dx0.double() + dh.double() @ a.double(), out_dtype=ydt,
                       cond=dx0.double().abs() + dh.double().abs() @ a.double().abs(), k=r + 1, what="dx += dh A")


def _wgrad_k(m, j, r):
    """rows_per_split (a multiple of 32, at least 128, never more than the rows there are) + splits + 1"""
    splits = _lib.load().cfhip_lora_wgrad_workspace(m, j, r) // (j * r * 4)
    rows = max(128, (-(-m // splits) + 31) // 32 * 32)
    return min(m, rows) + splits + 1


def test_kept_positions_are_those_of_dropout():
    """updates that cannot vanish (ones times ones into zeros): the positions the kernels touch are ops.dropout's keep mask at the
    same (seed, offset), bit for bit"""
    m, n, r, p = 63, 200, 4, 0.25
    _, mask = ops.dropout(torch.ones(m, n, dtype=F32, device=DEV), p, seed=SEED, offset=OFFSET, want_mask=True)
    ones = lambda *sh: torch.ones(*sh, dtype=BF16, device=DEV)  # noqa: E731
    for ydt in (F32, BF16):
        y = ops.lora_up_add(torch.zeros(m, n, dtype=ydt, device=DEV), ones(m, r), ones(n, r), p=p, seed=SEED, offset=OFFSET)
        assert torch.equal(y != 0, mask.bool())
    g = ops.lora_wgrad(ones(1, n), ones(1, r), torch.empty(n, r, dtype=F32, device=DEV), p=p, seed=SEED, offset=OFFSET)
    _, row = ops.dropout(torch.ones(1, n, dtype=F32, device=DEV), p, seed=SEED, offset=OFFSET, want_mask=True)
    assert torch.equal(g != 0, row.bool().view(n, 1).expand(n, r))
    eye = torch.eye(n, dtype=BF16, device=DEV)[:, :r].contiguous()  # dh[m][c] = keep[m][c] for c < r
    dh = ops.lora_down(ones(m, n), eye, f_trans=True, p=p, seed=SEED, offset=OFFSET)
    assert torch.equal(dh != 0, mask.bool()[:, :r])


@pytest.mark.parametrize("m,k,n,r", CASES)
def test_lora_wgrad_per_element(G, m, k, n, r):
    dy, h = _mk((m, n), 11), _mk((m, r), 12)
    s = 0.5
    for p in (0.0, 0.25):
        keep = _keep(m, n, p)
        sc = s / (1.0 - p)
        want = sc * ((keep * dy.double()).t() @ h.double())
        cond = sc * ((keep * dy.double().abs()).t() @ h.double().abs())
        out = G.out2d(1, n * r, n * r, F32, DEV).view(n, r)
        ops.lora_wgrad(_strided(G, dy), G.poisoned(h.to(DEV)), out, scale=s, p=p, seed=SEED, offset=OFFSET)
        assert_elementwise(out, want, out_dtype=F32, cond=cond, k=_wgrad_k(m, n, r) + 1, what=f"dBm p={p}")
        ops.lora_wgrad(_strided(G, dy), G.poisoned(h.to(DEV)), out, accumulate=True, scale=s, p=p, seed=SEED, offset=OFFSET)
        assert_elementwise(out, 2 * want, out_dtype=F32, cond=2 * cond, k=_wgrad_k(m, n, r) + 2, what=f"dBm += p={p}")
    x, dh = _mk((m, k), 13), _mk((m, r), 14)
    out = G.out2d(1, r * k, r * k, F32, DEV).view(r, k)
    ops.lora_wgrad(_strided(G, x), G.poisoned(dh.to(DEV)), out, out_trans=True)
    assert_elementwise(out, dh.double().t() @ x.double(), out_dtype=F32, cond=dh.double().abs().t() @ x.double().abs(),
                       k=_wgrad_k(m, k, r), what="dA = dh^T x")


def test_lora_wgrad_is_deterministic():
    m, n, r = 4100, 200, 17
    dy, h = _mk((m, n), 15).to(DEV), _mk((m, r), 16).to(DEV)
    outs = [ops.lora_wgrad(dy, h, torch.empty(n, r, dtype=F32, device=DEV), scale=0.5, p=0.25, seed=SEED, offset=OFFSET).clone()
            for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_argument_checks():
    x = torch.zeros(8, 40, dtype=BF16, device=DEV)
    with pytest.raises(ValueError):
        ops.lora_down(x[:, :36], torch.zeros(4, 36, dtype=BF16, device=DEV))  # K % 8
    with pytest.raises(ValueError):
        ops.lora_down(x, torch.zeros(65, 40, dtype=BF16, device=DEV))  # r <= 64
    with pytest.raises(ValueError):
        ops.lora_down(x.view(-1)[4:4 + 7 * 40].view(7, 40), torch.zeros(4, 40, dtype=BF16, device=DEV))  # alignment
    with pytest.raises(TypeError):
        ops.lora_down(x.float(), torch.zeros(4, 40, dtype=BF16, device=DEV))
    with pytest.raises(ValueError):
        ops.lora_up_add(torch.zeros(8, 24, dtype=F32, device=DEV), torch.zeros(8, 4, dtype=BF16, device=DEV),
                        torch.zeros(24, 4, dtype=BF16, device=DEV), p=1.0)


# ---------------------------------------------------------------------------------------------
# LoRALinearFn / the hook against the reference's fp32 numbers
# ---------------------------------------------------------------------------------------------


def _hooked(cls, rec, sc, alpha, frozen=False, dropout=0.0):
    nin, nout, rank = rec["shape"]
    layer = getattr(C, cls)(nin, nout)
    inner = layer.linear if hasattr(layer, "linear") else layer
    hook = C.LoRALinearHook.create_with(layer, rank)
    hook.dropout.p = dropout
    with torch.no_grad():
        inner.weight.copy_(rec["wq"].float() * sc["w"])
        inner.bias.copy_(rec["bq"].float() * sc["w"])
        hook.lora_down.weight.copy_(rec["aq"].float() * sc["a"])
        hook.lora_up.weight.copy_(rec["bmq"].float() * sc["a"])
        hook.alpha.fill_(alpha)
    hook.refresh_alpha()
    layer.hook = hook
    layer.to(DEV)
    inner.weight.requires_grad_(not frozen)
    inner.bias.requires_grad_(not frozen)
    return layer, inner, hook


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("cls", ["HijackLinear", "HijackCustomLinear"])
def test_lora_linear_against_the_reference(golden, cls, frozen):
    """tolerances: those of test_gpu_modules.test_linear_golden (rel-L2 1e-2 for outputs and bias gradients, 1.5e-2 for input and weight
    gradients): a K-long bf16 product plus an r-long one is the same error class"""
    g = golden("lora_linear.pt")
    for rec in g["layers"]:
        want = rec["results"][cls]
        layer, inner, hook = _hooked(cls, rec, g["scales"], g["alpha"], frozen)
        layer.train()
        x = (rec["xq"].float() * g["scales"]["x"]).to(DEV).requires_grad_(True)
        y = layer(x)
        tag = f"{cls} {rec['shape']}"
        assert y.dtype == BF16
        assert_close(y, want["y"], 1e-2, f"{tag} y")
        y.backward((rec["gyq"].float() * g["scales"]["x"]).to(DEV).to(BF16))
        HF.SideStream.join()
        assert_close(x.grad, want["gx"], 1.5e-2, f"{tag} gx")
        assert_close(hook.lora_down.weight.grad, want["ga"], 1.5e-2, f"{tag} ga")
        assert_close(hook.lora_up.weight.grad, want["gbm"], 1.5e-2, f"{tag} gbm")
        assert hook.alpha.grad is None and hook.lora_up.weight.grad.dtype == F32
        if frozen:
            assert inner.weight.grad is None and inner.bias.grad is None
        else:
            assert_close(inner.weight.grad[::rec["row_step"]], rec["gw_rows"], 1.5e-2, f"{tag} gw")
            assert_close(inner.bias.grad, rec["gb"], 1e-2, f"{tag} gb")


def test_feedforward_order_of_the_activation(golden):
    """the low-rank term of the first layer enters before the GELU (an add after it is 0.42 away: test_lora_host)"""
    g = golden("lora_linear.pt")
    ff, sc = g["ff"], g["scales"]
    nin, lat, rank = ff["shape"]
    m = C.FeedForward(nin, lat, 0.0, "GELU")
    for idx in (0, 3):
        layer, q = m.net[idx], ff[f"net{idx}"]
        hook = C.LoRALinearHook.create_with(layer, rank)
        hook.dropout.p = 0.0
        with torch.no_grad():
            layer.linear.weight.copy_(q["wq"].float() * sc["w"])
            layer.linear.bias.copy_(q["bq"].float() * sc["w"])
            hook.lora_down.weight.copy_(q["aq"].float() * sc["a"])
            hook.lora_up.weight.copy_(q["bmq"].float() * sc["a"])
            hook.alpha.fill_(g["alpha"])
        hook.refresh_alpha()
        layer.hook = hook
    m.to(DEV).train()
    x = (ff["xq"].float() * sc["x"]).to(DEV).requires_grad_(True)
    y = m(x)
    assert_close(y, ff["y"], 1e-2, "ff y")
    y.backward((ff["gyq"].float() * sc["x"]).to(DEV).to(BF16))
    HF.SideStream.join()
    assert_close(x.grad, ff["gx"], 1.5e-2, "ff gx")


def test_frozen_base_launches_no_weight_gradient(golden, monkeypatch):
    g = golden("lora_linear.pt")
    rec = g["layers"][1]
    calls = []
    real_gemm, real_grouped, real_colsum = ops.gemm, ops.gemm_grouped_tn, ops.colsum
    monkeypatch.setattr(ops, "gemm", lambda a, b, **kw: (calls.append("tn" if kw.get("a_trans") else "gemm"), real_gemm(a, b, **kw))[1])
    monkeypatch.setattr(ops, "gemm_grouped_tn", lambda pr: (calls.append("grouped"), real_grouped(pr))[1])
    monkeypatch.setattr(ops, "colsum", lambda *a, **kw: (calls.append("colsum"), real_colsum(*a, **kw))[1])
    x0 = (rec["xq"].float() * g["scales"]["x"]).to(DEV)
    gy = (rec["gyq"].float() * g["scales"]["x"]).to(DEV).to(BF16)
    grads = {}
    for frozen in (True, False):
        layer, inner, hook = _hooked("HijackCustomLinear", rec, g["scales"], g["alpha"], frozen)
        layer.train()
        x = x0.clone().requires_grad_(True)
        calls.clear()
        layer(x).backward(gy)
        HF.SideStream.join()
        torch.cuda.synchronize()
        if frozen:
            assert inner.weight.grad is None and inner.bias.grad is None
            assert calls == ["gemm", "gemm"], calls  # forward and dX; no dW / db launch of any kind
        else:
            assert any(c in ("tn", "grouped") for c in calls), calls
            grads["lora"] = (inner.weight.grad.clone(), inner.bias.grad.clone())
    plain = C.HijackCustomLinear(*rec["shape"][:2]).to(DEV)
    with torch.no_grad():
        plain.linear.weight.copy_(inner.weight)
        plain.linear.bias.copy_(inner.bias)
    x = x0.clone().requires_grad_(True)
    plain(x).backward(gy)
    HF.SideStream.join()
    torch.cuda.synchronize()
    assert torch.equal(plain.linear.weight.grad, grads["lora"][0]) and torch.equal(plain.linear.bias.grad, grads["lora"][1])


@pytest.mark.parametrize("arena", [False, True])
def test_eval_injection_and_the_stale_shadow(golden, arena):
    g = golden("lora_linear.pt")
    rec = g["layers"][2]
    layer, inner, hook = _hooked("HijackCustomLinear", rec, g["scales"], g["alpha"])
    if arena:
        C.ParamArena([inner.weight, inner.bias])
    w0 = inner.weight.detach().clone()
    x = (rec["xq"].float() * g["scales"]["x"]).to(DEV)

    def base_out(w):
        return HF.linear(x, w.clone(), inner.bias.detach().clone())

    with torch.no_grad():
        layer.train()
        layer(x)  # the bf16 shadow of the base weight is cached now
        layer.eval()
        y = layer(x)
        assert hook.injected and not torch.equal(inner.weight.detach(), w0)
        assert_close(inner.weight.detach()[::rec["row_step"]], rec["w_injected_rows"], 1e-5, "injected weight")
        assert_close(y, rec["y_eval"], 1e-2, "y eval")
        assert torch.equal(y, base_out(inner.weight.detach())), "eval output is not that of the injected weight (stale shadow)"
        assert torch.equal(layer(x), y)
        # back to training: the first forward restores the weight — and the shadow has to follow
        layer.train()
        layer(x)
        assert not hook.injected and torch.equal(inner.weight.detach(), w0)
        assert torch.equal(HF.shadow_bf16(inner.weight), w0.to(BF16)), "stale shadow after train()"
        # eval again, then cleanup(): the output is the base weight's
        layer.eval()
        assert torch.equal(layer(x), y)
        hook.cleanup()
        layer.hook = None
        assert torch.equal(inner.weight.detach(), w0)
        if arena:
            assert inner.weight.data_ptr() == inner.weight._cfhip_arena.flat_p.data_ptr()
        assert torch.equal(layer(x), base_out(w0)), "stale shadow after cleanup()"


def test_gradient_checkpoint_repeats_the_dropout_mask(golden):
    g = golden("lora_linear.pt")
    rec = g["layers"][1]
    layer, inner, hook = _hooked("HijackLinear", rec, g["scales"], g["alpha"], dropout=0.25)
    layer.train()
    x0 = (rec["xq"].float() * g["scales"]["x"]).to(DEV)
    gy = (rec["gyq"].float() * g["scales"]["x"]).to(DEV).to(BF16)
    params = list(layer.parameters())
    runs = []
    for ckpt in (False, True):
        ops.PhiloxState.manual_seed(5)
        for p in params:
            p.grad = None
        x = x0.clone().requires_grad_(True)
        y = HF.gradient_checkpoint(lambda t: layer(t), (x,), params, ckpt)
        y.backward(gy)
        HF.SideStream.join()
        torch.cuda.synchronize()
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params if p.grad is not None])
    assert len(runs[0]) == len(runs[1]) == 6  # y, gx, gW, gb, gA, gBm
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    nodrop = _hooked("HijackLinear", rec, g["scales"], g["alpha"])[0].train()
    assert not torch.equal(nodrop(x0), runs[0][0])  # the mask did something


def test_tiny_end_to_end_fine_tuning(golden):
    """vit_small, rank-4 adapters on every Linear of two blocks, base frozen, adapter parameters alone in the arena, five FusedAdam steps"""
    from cflearn_amd.engine import TrainStep

    g = golden("vit_small.pt")
    cfg = dict(g["cfg"])
    model = C.build_module("cv_clf", config=dict(in_channels=3, num_classes=g["num_classes"], img_size=cfg.pop("img_size"),
                                                 latent_dim=cfg["latent_dim"], encoder="vit", encoder_config=cfg))
    model.load_state_dict(g["sd"])
    model = model.to(DEV)
    for p in model.parameters():
        p.requires_grad_(False)
    base = {k: v.detach().clone() for k, v in model.state_dict().items()}
    blocks = [n for n, m in model.named_modules() if isinstance(m, C.MixingBlock)][:2]
    mgr = C.LoRAManager()
    torch.manual_seed(11)
    mgr.prepare(model, key="ft", rank=4, target_ancestors={"MixingBlock"})
    hooks = mgr.lora_packs["ft"].hooks
    for k in [k for k in hooks if not k.startswith(tuple(b + "." for b in blocks))]:
        del hooks[k]
    assert len(hooks) == 6  # out_linear and the two FeedForward layers of each block
    mgr.inject(model, "ft")
    model.train()
    ops.PhiloxState.manual_seed(3)
    ts = TrainStep(model, lr=2.0e-3)
    assert {id(p) for p in ts.arena.params} == {id(p) for h in hooks.values() for p in (h.lora_down.weight, h.lora_up.weight)}
    img, labels = g["img"].to(DEV), g["labels"].view(-1).to(DEV)
    losses = [ts.step(img, labels).item() for _ in range(5)]
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        losses.append(ts.step(img, labels).item())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    names = {e.name for e in prof.events()}
    assert not names & {"aten::mm", "aten::addmm", "aten::matmul", "aten::linear", "aten::bmm", "aten::dropout", "aten::native_dropout"}, names
    now = model.state_dict()
    assert all(torch.equal(now[k], v) for k, v in base.items()), "a frozen base parameter changed"
    assert any(float(h.lora_up.weight.abs().max()) > 0 for h in hooks.values())
