"""Convolution LoRA adapters on the GPU: the three 3x3 kernels of csrc/lora.hip per element against float64 (guarded outputs,
poisoned inputs), `LoRAConv2dFn` / `LoRAConvHook` against the reference's own numbers (tests/golden/lora_conv.pt), and a small
UNetDiffuser with every hook of a `LoRAManager` pack attached.

Error models of the kernel tests (`assert_elementwise`: ulps = 1 of the output type, plus k f32 roundings times the same product on
absolute values):
  * lora_conv_down: one MFMA accumulator per output over the 9 C products of the taps, then the scale: k = 9 C + 1; one bf16 rounding.
  * lora_conv_dx: one accumulator over the 9 r products of (tap, rank): k = 9 r + 1; when accumulating, the add onto the bf16 value
    that was there: k + 1.
  * lora_conv_wgrad: rows_per_split additions inside a split, splits - 1 ordered additions of the partial sums, the scale, the add
    into `out` when accumulating: k = rows_per_split + splits + 1 (+ 1), derived from the workspace query like test_gpu_lora._wgrad_k."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, assert_elementwise, guarded_ops, rel_l2

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import _lib, functional as HF, modules as M, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# (B, H, W, C, stride, r)
CASES = [
    (1, 1, 1, 8, 1, 1),       # every tap but the centre falls outside; C below one K-step
    (2, 5, 7, 40, 1, 4),      # a 64-row stripe crosses the image and batch boundary; C tail
    (2, 5, 7, 40, 2, 17),     # odd sizes under stride 2, Ho x Wo = 3 x 4; odd rank
    (3, 9, 6, 64, 2, 64),     # factor larger than one LDS image: the chunked path
    (2, 33, 31, 32, 1, 16),   # several stripes per workgroup with a ragged tail
    (1, 2, 16, 320, 1, 64),   # a UNet channel count
]


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


def _rows(t):
    """[B, C, H, W] -> NHWC rows [B H W, C]"""
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous()


def _nchw(rows, b, h, w):
    return rows.view(b, h, w, -1).permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def refs():
    """float64 references of the three kernels per case, computed once from the bf16-rounded inputs"""
    out = {}
    for i, (b, h, w, c, s, r) in enumerate(CASES):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        x, f = _mk((b, c, h, w), 20 + i), _mk((r, c, 3, 3), 40 + i, 0.25)
        dh = _mk((b, r, ho, wo), 60 + i)
        xd, fd, dhd = x.double(), f.double(), dh.double()
        out[(b, h, w, c, s, r)] = dict(
            x=x, f=f, dh=dh, ho=ho, wo=wo,
            down=_rows(F.conv2d(xd, fd, None, s, 1)), down_c=_rows(F.conv2d(xd.abs(), fd.abs(), None, s, 1)),
            dx=_rows(torch.nn.grad.conv2d_input((b, c, h, w), fd, dhd, s, 1)),
            dx_c=_rows(torch.nn.grad.conv2d_input((b, c, h, w), fd.abs(), dhd.abs(), s, 1)),
            wg=torch.nn.grad.conv2d_weight(xd, (r, c, 3, 3), dhd, s, 1),
            wg_c=torch.nn.grad.conv2d_weight(xd.abs(), (r, c, 3, 3), dhd.abs(), s, 1))
    return out


@pytest.mark.parametrize("case", CASES)
def test_conv_down_per_element(G, refs, case):
    b, h, w, c, s, r = case
    ref = refs[case]
    sc = 0.75
    got = ops.lora_conv_down(_strided(G, _rows(ref["x"])), G.poisoned(ref["f"].to(DEV)), b, h, w, s, scale=sc)
    assert got.shape == (b * ref["ho"] * ref["wo"], r) and got.dtype == BF16
    assert_elementwise(got, sc * ref["down"], out_dtype=BF16, cond=sc * ref["down_c"], k=9 * c + 1, what="h = conv3x3(x, f)")


@pytest.mark.parametrize("case", CASES)
def test_conv_dx_per_element(G, refs, case):
    b, h, w, c, s, r = case
    ref = refs[case]
    dh_rows = _rows(ref["dh"])
    dx = G.out2d(b * h * w, c, c + 8, BF16, DEV)
    ops.lora_conv_dx(G.poisoned(dh_rows.to(DEV)), G.poisoned(ref["f"].to(DEV)), b, h, w, s, out=dx)
    assert_elementwise(dx, ref["dx"], out_dtype=BF16, cond=ref["dx_c"], k=9 * r + 1, what="dx = conv3x3^T(dh, f)")
    dx0 = _mk((b * h * w, c), 99)
    dx = _strided(G, dx0)
    ops.lora_conv_dx(G.poisoned(dh_rows.to(DEV)), G.poisoned(ref["f"].to(DEV)), b, h, w, s, out=dx, accumulate=True)
    assert_elementwise(dx, dx0.double() + ref["dx"], out_dtype=BF16, cond=dx0.double().abs() + ref["dx_c"], k=9 * r + 2, what="dx += ...")
    fresh = ops.lora_conv_dx(dh_rows.to(DEV), ref["f"].to(DEV), b, h, w, s)
    assert fresh.shape == (b * h * w, c) and fresh.is_contiguous()


def _conv_wgrad_k(b, h, w, c, r, s):
    """rows_per_split (a multiple of 32, at least 128, never more than the rows there are) + splits + 1"""
    m = b * ((h - 1) // s + 1) * ((w - 1) // s + 1)
    splits = _lib.load().cfhip_lora_conv_wgrad_workspace(b, h, w, c, r, s) // (9 * c * r * 4)
    rows = max(128, (-(-m // splits) + 31) // 32 * 32)
    return min(m, rows) + splits + 1


@pytest.mark.parametrize("case", CASES)
def test_conv_wgrad_per_element(G, refs, case):
    b, h, w, c, s, r = case
    ref = refs[case]
    sc = 0.5
    k = _conv_wgrad_k(b, h, w, c, r, s)
    out = G.out2d(1, r * c * 9, r * c * 9, F32, DEV).view(r, c, 3, 3)
    args = (G.poisoned(_rows(ref["dh"]).to(DEV)), _strided(G, _rows(ref["x"])), out, b, h, w, s)
    ops.lora_conv_wgrad(*args, scale=sc)
    assert_elementwise(out, sc * ref["wg"], out_dtype=F32, cond=sc * ref["wg_c"], k=k, what="d lora_down.weight")
    ops.lora_conv_wgrad(*args, scale=sc, accumulate=True)
    assert_elementwise(out, 2 * sc * ref["wg"], out_dtype=F32, cond=2 * sc * ref["wg_c"], k=k + 1, what="d lora_down.weight, accumulated")


def test_conv_wgrad_is_deterministic(refs):
    case = CASES[4]
    b, h, w, c, s, r = case
    ref = refs[case]
    dh, x = _rows(ref["dh"]).to(DEV), _rows(ref["x"]).to(DEV)
    outs = [ops.lora_conv_wgrad(dh, x, torch.empty(r, c, 3, 3, dtype=F32, device=DEV), b, h, w, s, scale=0.5).clone() for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_argument_checks():
    x = torch.zeros(2 * 4 * 4, 16, dtype=BF16, device=DEV)
    f = torch.zeros(4, 16, 3, 3, dtype=BF16, device=DEV)
    with pytest.raises(ValueError):
        ops.lora_conv_down(x, f, 2, 4, 4, 3)  # stride
    with pytest.raises(ValueError):
        ops.lora_conv_down(x, f, 2, 4, 5, 1)  # rows != B H W
    with pytest.raises(ValueError):
        ops.lora_conv_down(x, torch.zeros(65, 16, 3, 3, dtype=BF16, device=DEV), 2, 4, 4, 1)  # r <= 64
    with pytest.raises(TypeError):
        ops.lora_conv_down(x.float(), f, 2, 4, 4, 1)
    with pytest.raises(ValueError):
        ops.lora_conv_dx(torch.zeros(32, 4, dtype=BF16, device=DEV), f, 2, 4, 4, 1, accumulate=True)  # nothing to accumulate into
    lib = _lib.load()
    h = torch.zeros(32, 4, dtype=BF16, device=DEV)
    # the C entry points themselves: the error code and the message
    rc = lib.cfhip_lora_conv_down(x.data_ptr(), f.data_ptr(), h.data_ptr(), 2, 4, 4, 12, 4, 1, 16, 1.0, 0)
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"] and b"multiple of 8" in lib.cfhip_last_error()
    rc = lib.cfhip_lora_conv_dx(h.data_ptr(), f.data_ptr(), x.data_ptr(), 2, 4, 4, 16, 4, 3, 16, 0, 0)
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"] and b"stride" in lib.cfhip_last_error()
    out = torch.zeros(4, 16, 3, 3, dtype=F32, device=DEV)
    rc = lib.cfhip_lora_conv_wgrad(h.data_ptr(), x.data_ptr(), out.data_ptr(), 2, 4, 4, 16, 4, 1, 16, 0, 1.0, 0, 0, 0)
    assert rc == _lib.DEFINES["CFHIP_ERR_WORKSPACE"] and b"workspace" in lib.cfhip_last_error()
    assert lib.cfhip_lora_conv_wgrad_workspace(2, 4, 4, 16, 4, 3) == 0


# ---------------------------------------------------------------------------------------------
# LoRAConv2dFn / the hook against the reference's fp32 numbers
# ---------------------------------------------------------------------------------------------


def _hooked(rec, g, frozen=False, dropout=0.0):
    cin, cout, k, stride, pad, rank, _, _ = rec["case"]
    sc = g["scales"]
    layer = M.HijackConv2d(cin, cout, k, stride, pad)
    hook = C.LoRAConvHook.create_with(layer, rank)
    hook.dropout.p = dropout
    with torch.no_grad():
        layer.weight.copy_(rec["wq"].float() * sc["w"])
        layer.bias.copy_(rec["bq"].float() * sc["w"])
        hook.lora_down.weight.copy_(rec["aq"].float() * sc["a"])
        hook.lora_up.weight.copy_(rec["bmq"].float() * sc["a"])
        hook.alpha.fill_(g["alpha"])
    hook.refresh_alpha()
    layer.hook = hook
    layer.to(DEV)
    layer.weight.requires_grad_(not frozen)
    layer.bias.requires_grad_(not frozen)
    return layer, hook


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("frozen", [False, True])
def test_lora_conv_against_the_reference(golden, frozen, nhwc):
    """tolerances: those of test_gpu_modules' convolution golden test and test_gpu_lora.test_lora_linear_against_the_reference (rel-L2
    1e-2 for outputs and bias gradients, 1.5e-2 for input and weight gradients): a 9 C-long bf16 product plus an r-long one is the
    same error class"""
    g = golden("lora_conv.pt")
    for rec in g["layers"]:
        cin, cout, k, stride, pad, rank, h, w = rec["case"]
        b = g["batch"]
        layer, hook = _hooked(rec, g, frozen)
        layer.train()
        x0 = rec["xq"].float() * g["scales"]["x"]
        gy0 = rec["gyq"].float() * g["scales"]["x"]
        tag = f"{tuple(rec['case'])} nhwc={nhwc}"
        prev = HF.NHWC[0]
        HF.NHWC[0] = nhwc
        try:
            if nhwc:  # NHWC rows in, NHWC rows out, the gradient arrives as NHWC rows
                rows = _rows(x0).to(DEV).to(BF16).requires_grad_(True)
                y = layer(HF.rows_to_nhwc(rows, b, cin, h, w))
                assert HF.is_nhwc(y)
                y.backward(HF.rows_to_nhwc(_rows(gy0).to(DEV).to(BF16), b, cout, y.shape[2], y.shape[3]))
                gx = _nchw(rows.grad, b, h, w)
            else:
                x = x0.to(DEV).requires_grad_(True)
                y = layer(x)
                assert y.is_contiguous()
                y.backward(gy0.to(DEV).to(BF16))
                gx = x.grad
        finally:
            HF.NHWC[0] = prev
        HF.SideStream.join()
        assert y.dtype == BF16
        assert_close(y, rec["y"], 1e-2, f"{tag} y")
        assert_close(gx, rec["gx"], 1.5e-2, f"{tag} gx")
        assert_close(hook.lora_down.weight.grad, rec["ga"], 1.5e-2, f"{tag} ga")
        assert_close(hook.lora_up.weight.grad, rec["gbm"], 1.5e-2, f"{tag} gbm")
        assert hook.alpha.grad is None and hook.lora_down.weight.grad.dtype == F32
        if frozen:
            assert layer.weight.grad is None and layer.bias.grad is None
        else:
            assert_close(layer.weight.grad[::rec["row_step"]], rec["gw_rows"], 1.5e-2, f"{tag} gw")
            assert_close(layer.bias.grad, rec["gb"], 1e-2, f"{tag} gb")


def test_frozen_base_launches_no_weight_gradient(golden, monkeypatch):
    g = golden("lora_conv.pt")
    calls = []
    real = {n: getattr(ops, n) for n in ("gemm", "gemm_grouped_tn", "colsum", "conv3x3_wgrad_nhwc")}
    monkeypatch.setattr(ops, "gemm", lambda a, b, **kw: (calls.append("tn" if kw.get("a_trans") else "gemm"), real["gemm"](a, b, **kw))[1])
    for n in ("gemm_grouped_tn", "colsum", "conv3x3_wgrad_nhwc"):
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **kw: (calls.append(_n), real[_n](*a, **kw))[1])
    owed = ("tn", "gemm_grouped_tn", "colsum", "conv3x3_wgrad_nhwc")
    for rec in g["layers"]:
        for frozen in (True, False):
            layer, hook = _hooked(rec, g, frozen)
            layer.train()
            x = (rec["xq"].float() * g["scales"]["x"]).to(DEV).requires_grad_(True)
            calls.clear()
            layer(x).backward((rec["gyq"].float() * g["scales"]["x"]).to(DEV).to(BF16))
            HF.SideStream.join()
            torch.cuda.synchronize()
            if frozen:
                assert layer.weight.grad is None and layer.bias.grad is None
                assert not any(c in owed for c in calls), calls  # no dW / db launch of any kind
            else:
                assert any(c in owed for c in calls), calls


@pytest.mark.parametrize("arena", [False, True])
def test_eval_injection_uses_the_merged_filter(golden, arena):
    """the FIRST eval forward equals the reference's training-mode output (the 3x3 eval target: the exactly merged filter), not the
    reference's broadcast-tap injection; cleanup() restores the weight bit for bit"""
    g = golden("lora_conv.pt")
    for rec in g["layers"]:
        k = rec["case"][2]
        layer, hook = _hooked(rec, g)
        if arena:
            C.ParamArena([layer.weight, layer.bias])
        w0 = layer.weight.detach().clone()
        x = (rec["xq"].float() * g["scales"]["x"]).to(DEV)
        with torch.no_grad():
            layer.train()
            base_train = layer(x)  # the bf16 shadow of the base weight is cached now
            layer.eval()
            y = layer(x)
            assert hook.injected and not torch.equal(layer.weight.detach(), w0)
            assert_close(y, rec["y"], 1e-2, f"{tuple(rec['case'])} first eval forward")
            assert_close(y, base_train, 1e-2, "eval vs training forward")
            if k == 1:
                assert_close(layer.weight.detach(), rec["w_injected"], 1e-5, "injected weight")
                assert_close(y, rec["y_eval"], 1e-2, "y eval")
            else:
                assert rec["eval_ref_rel"] > 4e-2  # what mirroring hijacks.py:143 would have cost
            assert torch.equal(layer(x), y)
            hook.cleanup()
            layer.hook = None
            assert torch.equal(layer.weight.detach(), w0)
            if arena:
                assert layer.weight.data_ptr() == layer.weight._cfhip_arena.flat_p.data_ptr()
            plain = HF.conv2d(x, w0.clone(), layer.bias.detach().clone(), rec["case"][3], rec["case"][4])
            assert torch.equal(layer(x), plain), "stale shadow after cleanup()"


def test_gradient_checkpoint_repeats_the_dropout_mask(golden):
    g = golden("lora_conv.pt")
    rec = g["layers"][1]
    layer, hook = _hooked(rec, g, dropout=0.25)
    layer.train()
    x0 = (rec["xq"].float() * g["scales"]["x"]).to(DEV)
    gy = (rec["gyq"].float() * g["scales"]["x"]).to(DEV).to(BF16)
    params = [p for p in layer.parameters() if p.requires_grad]
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
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params])
    assert len(runs[0]) == len(runs[1]) == 6  # y, gx, gW, gb, gA, gBm
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    nodrop = _hooked(rec, g)[0].train()
    assert not torch.equal(nodrop(x0), runs[0][0])  # the mask did something


# ---------------------------------------------------------------------------------------------
# A small UNet with every hook of a pack attached
# ---------------------------------------------------------------------------------------------


def _small_unet():
    torch.manual_seed(7)
    unet = M.UNetDiffuser(4, 4, num_head_channels=32, use_spatial_transformer=True, start_channels=32, num_res_blocks=1,
                          attention_downsample_rates=(1,), channel_multipliers=(1, 2))
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():  # the zero-initialised convolutions would hide everything upstream of them
        for p in unet.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=gen) * (0.5 / max(1, p[0].numel()) ** 0.5))
    return unet.to(DEV)


def _merged_copy(unet, pack, training=True):
    """a hook-free deep copy whose weights are the merged weights, formed on the host in fp32.  A HijackCustomLinear (the feed-forward
    layers of the transformer blocks) counts its adapter TWICE in training mode and once when injected for eval: the reference's own
    behaviour, mirrored by LoRALinearHook and pinned by tests/golden/lora_linear.pt — so the two modes have different merged weights
    there, and only there."""
    plain = copy.deepcopy(unet)
    for m in plain.modules():
        if hasattr(m, "hook"):
            m.hook = None
    mods = dict(plain.named_modules())
    with torch.no_grad():
        for name, hook in pack.hooks.items():
            layer = mods[name]
            up, down = hook.lora_up.weight.detach().float().cpu(), hook.lora_down.weight.detach().float().cpu()
            times = 2.0 if training and isinstance(layer, C.HijackCustomLinear) else 1.0
            if down.dim() == 4:
                upd = torch.einsum("oc,cikl->oikl", up[:, :, 0, 0], down)
            else:
                upd = up @ down
            w = layer.linear.weight if isinstance(layer, C.HijackCustomLinear) else layer.weight
            w.copy_((w.detach().float().cpu() + times * hook.full_scale * upd).to(w.device))
    return plain


def test_unet_end_to_end_with_every_hook(golden):
    unet = _small_unet()
    x = (torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9))).to(DEV)
    t = torch.tensor([3, 500], device=DEV)
    with torch.no_grad():
        unet.eval()
        base = unet(x, timesteps=t).float().clone()
    mgr = C.LoRAManager()
    mgr.prepare(unet, key="k", rank=4)
    pack = mgr.lora_packs["k"]
    kinds = {type(h).__name__ for h in pack.hooks.values()}
    assert kinds == {"LoRAConvHook", "LoRALinearHook"}
    assert sorted(mgr.skipped) == ["head.2", "input_blocks.0.0"]  # 4 input / output channels: no adapter kernels
    gen = torch.Generator().manual_seed(10)
    for hook in pack.hooks.values():
        hook.dropout.p = 0.0
        with torch.no_grad():
            hook.lora_up.weight.copy_(torch.randn(hook.lora_up.weight.shape, generator=gen) * 0.1)
            hook.alpha.fill_(4.0)
        hook.refresh_alpha()
    for p in unet.parameters():
        p.requires_grad_(False)
    unet.train()
    mgr.inject(unet, "k")
    # (a) every hook of the pack takes part in training
    y = unet(x, timesteps=t)
    y.float().square().mean().backward()
    HF.SideStream.join()
    torch.cuda.synchronize()
    for name, hook in pack.hooks.items():
        for prm in (hook.lora_down.weight, hook.lora_up.weight):
            assert prm.grad is not None and float(prm.grad.abs().max()) > 0.0, f"{name}: an adapter factor received no gradient"
    assert all(p.grad is None for p in unet.parameters() if not p.requires_grad)
    # (b) the output is that of the merged weights
    plain = _merged_copy(unet, pack).train()
    plain_eval = _merged_copy(unet, pack, training=False).eval()  # (before the eval forward injects into `unet` itself)
    with torch.no_grad():
        want = plain(x, timesteps=t).float()
        want_eval = plain_eval(x, timesteps=t).float()
    assert rel_l2(want, base) > 0.1, "the adapters move the output too little for the comparison to tell"
    assert_close(y.float(), want, 1e-2, "adapted training output vs merged weights")
    # (c) eval: the first forward after injection (inside the sampler's frozen-pack scope) uses the merged filters
    unet.eval()
    with torch.no_grad():
        with HF.frozen_conv_packs(unet):
            y_eval = unet(x, timesteps=t).float()
        print(f"eval output vs eval-merged weights {rel_l2(y_eval, want_eval):.3e}, vs training-merged weights {rel_l2(y_eval, want):.3e}")
        assert_close(y_eval, want_eval, 1e-2, "first eval forward vs merged weights")
        assert any(isinstance(m, C.HijackCustomLinear) for m in unet.modules())  # (why `want_eval` is not `want`)
        mgr.cleanup(unet)
        assert torch.equal(unet(x, timesteps=t).float(), base), "cleanup() did not restore the base output"
    # (d) the packed per-head projection has no adapter form
    msa = M.MultiHeadSpatialAttention(32, num_heads=1).to(DEV)
    msa.to_qkv.hook = object()
    with pytest.raises(NotImplementedError):
        msa(torch.randn(1, 32, 4, 4, device=DEV))
