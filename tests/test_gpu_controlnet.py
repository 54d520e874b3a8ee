"""ControlNet on the GPU: the direct 3x3 convolution and the bf16 SiLU per element against float64, DirectConv3x3Fn against
Conv2dFn's im2row route, the module / train step / samplers against the reference's CPU run (tests/golden/controlnet_small.pt,
tools/gen_controlnet_golden.py).

Error model of the direct kernel (helpers.assert_conv3x3_rows): every output is an f32 sum of 9 C exact bf16 x bf16 products and the
bias, C the channels the kernel reduces over (Cin in the forward, Cout in the input gradient), rounded once to bf16: 1 bf16 ulp plus
(9 C + 1) f32 roundings of the absolute-value convolution."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import _sig64, assert_close, assert_elementwise, guarded_ops

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controlnet_small.pt")

IMAGES = [(2, 5, 19), (1, 6, 33), (2, 7, 16)]
LAYERS = [(3, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2)]  # the five narrow hint layers
# what `direct_conv_ok` admits beyond them reaches the other channel paddings of the kernel: Cp 24 (forward), 48, 64 and 80 (input
# gradient), and six channel tiles with Cp 8
OTHER_LAYERS = [(24, 48, 1), (20, 64, 2), (8, 80, 1)]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)


def _nhwc_padded(t, cp):
    """[B, C, H, W] -> dense [B, H, W, cp] with zero channels appended"""
    b, c, h, w = t.shape
    out = torch.zeros((b, h, w, cp), dtype=t.dtype)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def _packed_ref(w, mode):
    """the operand of cfhip_conv3x3_direct_pack built on the host: wp[N][Kp], k = tap * Cp + c"""
    cout, cin = w.shape[:2]
    n, cp, kp = ops.conv3x3_direct_dims(cout, cin, mode)
    wp = torch.zeros((n, kp), dtype=BF16)
    src = w.to(BF16)
    if mode == 1:
        src = src.flip(2, 3).transpose(0, 1)
    body = torch.zeros((n, 9, cp), dtype=BF16)
    body[:src.shape[0], :, :src.shape[1]] = src.reshape(src.shape[0], src.shape[1], 9).transpose(1, 2)
    wp[:, :9 * cp] = body.reshape(n, 9 * cp)
    return wp


@pytest.mark.parametrize("image,layer", [(i, l) for i in IMAGES for l in LAYERS] + [(IMAGES[1], l) for l in OTHER_LAYERS],
                         ids=lambda v: "x".join(map(str, v)))
def test_direct_conv_per_element(G, image, layer):
    (b, h, w), (cin, cout, s) = image, layer
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    seed = 1000 * cin + 10 * h + s
    wt = _randn((cout, cin, 3, 3), seed, (9 * cin) ** -0.5)
    w64 = wt.to(BF16).double()
    bias = _randn((cout,), seed + 1)
    wd = G.poisoned(wt.to(DEV))
    for mode in (0, 1):
        n, cp, kp = ops.conv3x3_direct_dims(cout, cin, mode)
        wp = ops.conv3x3_direct_pack(wd, mode)
        assert tuple(wp.shape) == (n, kp) and torch.equal(wp.cpu(), _packed_ref(wt, mode)), f"pack mode {mode}"
        if mode == 0:
            x = _randn((b, cin, h, w), seed + 2, dtype=BF16)
            x64 = x.double()
            for bs in (None, bias):
                got = ops.conv3x3_direct(G.poisoned(_nhwc_padded(x, cp).to(DEV)), wp, None if bs is None else G.poisoned(bs.to(DEV)),
                                         h, w, s, 0)
                b64 = None if bs is None else bs.double()
                want = F.conv2d(x64, w64, b64, stride=s, padding=1)
                cond = F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), stride=s, padding=1)
                assert tuple(got.shape) == (b, ho, wo, cout)
                assert_elementwise(got, want.permute(0, 2, 3, 1), out_dtype=BF16, ulps=1, cond=cond.permute(0, 2, 3, 1), k=9 * cin + 1,
                                   what=f"forward {image} {layer} bias={bs is not None}")
        else:
            dy = _randn((b, cout, ho, wo), seed + 3, dtype=BF16)
            dy64 = dy.double()
            opad = (h - ((ho - 1) * s + 1), w - ((wo - 1) * s + 1))  # the odd sizes under stride 2
            want = F.conv_transpose2d(dy64, w64, None, stride=s, padding=1, output_padding=opad)
            cond = F.conv_transpose2d(dy64.abs(), w64.abs(), None, stride=s, padding=1, output_padding=opad)
            assert tuple(want.shape) == (b, cin, h, w)
            for bs in (None, _randn((n,), seed + 4)):
                got = ops.conv3x3_direct(G.poisoned(_nhwc_padded(dy, cp).to(DEV)), wp, None if bs is None else G.poisoned(bs.to(DEV)),
                                         h, w, s, 1)
                assert tuple(got.shape) == (b, h, w, n)
                add = torch.zeros(cin, dtype=torch.float64) if bs is None else bs[:cin].double()
                assert_elementwise(got[..., :cin], want.permute(0, 2, 3, 1) + add, out_dtype=BF16, ulps=1,
                                   cond=cond.permute(0, 2, 3, 1) + add.abs(), k=9 * cout + 1,
                                   what=f"input gradient {image} {layer} bias={bs is not None}")
                if n != cin:  # the channels that pad Cin to a multiple of 8 hold the bias alone: every filter there is zero
                    pad = got[..., cin:].float().cpu()
                    assert torch.equal(pad, torch.zeros_like(pad) if bs is None else bs[cin:].to(BF16).float().expand_as(pad))
        G.check()


@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_silu_bf16_per_element(G, n):
    x = _randn(n, 30 + n, 3.0, BF16)
    dy = _randn(n, 40 + n, 1.0, BF16)
    xd, dyd = G.poisoned(x.to(DEV)), G.poisoned(dy.to(DEV))
    x64, dy64 = x.double(), dy.double()
    s = _sig64(x64)
    # the bound of the f32 pair (test_gpu_kernel_edges.test_f32_silu_ema): fast exp2 / rcp, 1 ulp each, and the rounded exp2 argument
    assert_elementwise(ops.silu_bf16_fwd(xd), x64 * s, out_dtype=BF16, ulps=2, cond=(x64 * s).abs() * (1 + x64.abs()), k=8,
                       what=f"silu bf16 n={n}")
    assert_elementwise(ops.silu_bf16_bwd(dyd, xd), dy64 * s * (1 + x64 * (1 - s)), out_dtype=BF16, ulps=2,
                       cond=dy64.abs() * (1 + x64.abs()) ** 2, k=8, what=f"silu_bwd bf16 n={n}")


@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_scale_bf16_per_element(G, n):
    x = _randn(n, 50 + n, 3.0, BF16)
    xd = G.poisoned(x.to(DEV))
    for scale in (0.75, 1.3):
        # one f32 product (1.3 is not exact in f32: its rounding is one more unit of the product), rounded once to bf16
        want = x.double() * float(torch.tensor(scale, dtype=F32))
        assert_elementwise(ops.scale_bf16(xd, scale), want, out_dtype=BF16, ulps=1, cond=want.abs(), k=1, what=f"scale {scale} n={n}")
    empty = torch.empty((0,), dtype=BF16, device=DEV)
    assert ops.scale_bf16(empty, 2.0).numel() == 0 and ops.silu_bf16_fwd(empty).numel() == 0 and ops.silu_bf16_bwd(empty, empty).numel() == 0


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "x".join(map(str, l)))
def test_direct_fn_against_im2row_route(monkeypatch, layer):
    """the same inputs through DirectConv3x3Fn and through Conv2dFn on its im2row route: outputs and input gradients within the sum
    of the two kernels' error models (each is within one model of the exact result), weight and bias gradients bit-equal (shared code)"""
    cin, cout, s = layer
    b, h, w = 2, 7, 19
    monkeypatch.setattr(HF, "IMPLICIT_CONV", False)  # (32 -> 32 would take the implicit route)
    assert HF.conv_route(cin, cout, 3, 3, s, 1, 1, h, w)[0] == HF.IM2ROW
    x = _randn((b, cin, h, w), 7 + cin, dtype=BF16)
    wt = _randn((cout, cin, 3, 3), 8 + cin, (9 * cin) ** -0.5)
    bias = _randn((cout,), 9 + cin)
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    dy = _randn((b, cout, ho, wo), 10 + cin, dtype=BF16).to(DEV)
    outs = []
    for fn in (lambda *a: HF.direct_conv3x3(*a, s), lambda *a: HF.Conv2dFn.apply(*a, s, 1, 1)):
        xd = x.to(DEV).requires_grad_(True)
        wd, bd = wt.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
        y = fn(xd, wd, bd)
        y.backward(dy)
        HF.SideStream.join()
        torch.cuda.synchronize()
        outs.append((y.detach(), xd.grad, wd.grad, bd.grad))
    (y1, dx1, gw1, gb1), (y2, dx2, gw2, gb2) = outs
    x64, w64, dy64 = x.double(), wt.to(BF16).double(), dy.cpu().double()
    cond = F.conv2d(x64.abs(), w64.abs(), bias.double().abs(), stride=s, padding=1)
    assert_elementwise(y1, y2.double(), out_dtype=BF16, ulps=2, cond=cond, k=2 * (9 * cin + 1), what=f"forward {layer}")
    opad = (h - ((ho - 1) * s + 1), w - ((wo - 1) * s + 1))
    cond = F.conv_transpose2d(dy64.abs(), w64.abs(), None, stride=s, padding=1, output_padding=opad)
    # the im2row route rounds each tap's partial sum (over Cout) to bf16 before row2im adds the nine: 2^-9 relative each, together at
    # most 2^-9 = 2^15 x 2^-24 of the absolute-value sum, on top of the two f32 models
    assert_elementwise(dx1, dx2.double(), out_dtype=BF16, ulps=2, cond=cond, k=2 * (9 * cout + 1) + 2 ** 15, what=f"input gradient {layer}")
    assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2), f"weight / bias gradient {layer}"


# ---------------------------------------------------------------------------------------------
# the module, the train step and the samplers against the reference's CPU run
# ---------------------------------------------------------------------------------------------


def pytest_generate_tests(metafunc):
    if "handover" in metafunc.fixturenames:
        metafunc.parametrize("handover", ["nchw", "nhwc"], indirect=True)


@pytest.fixture
def handover(request, monkeypatch):
    """which activation layout the models hand between their layers (the GroupNorm threshold decides it from the batch size)"""
    monkeypatch.setattr(ops, "GN_NHWC_GROUP_MIN_WORKGROUPS", 1 if request.param == "nhwc" else 1 << 30)
    return request.param


@pytest.fixture(scope="module")
def fixture():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def _models(g, zero_init=False):
    """(unet, control_net) with the fixture's parameters on the device; `zero_init`: the ControlNet as its constructor leaves it"""
    from controlnet_weights import fill_parameters
    from cflearn_amd.modules import UNetDiffuser

    torch.manual_seed(0)
    unet, cn = UNetDiffuser(**g["unet_cfg"]), C.ControlNet(**g["cfg"])
    fill_parameters(unet, g["unet_seed"])
    if not zero_init:
        fill_parameters(cn, g["control_seed"])
    return unet.to(DEV), cn.to(DEV)


def _inputs(g):
    return {k: g[k].to(DEV) for k in ("x_t", "hint", "timesteps", "context", "noise")}


def _sampled(p_grad):
    from controlnet_weights import sample_gradient

    return sample_gradient(p_grad.detach().float().cpu())


def test_module_against_the_reference(fixture, handover):
    """the control list, the UNet output computed with it, the loss and every ControlNet parameter gradient, with the bounds of
    test_gpu_unet.test_unet_variants_golden"""
    g = fixture
    unet, cn = _models(g)
    unet.requires_grad_(False)
    i = _inputs(g)
    ctrl = cn(i["x_t"], i["hint"], timesteps=i["timesteps"], context=i["context"], scales=g["scales"])
    assert len(ctrl) == len(g["control"])
    for j, (got, want) in enumerate(zip(ctrl, g["control"])):
        assert_close(got, want, 2e-2, f"control {j}")
    y = unet(i["x_t"], timesteps=i["timesteps"], context=i["context"], control=ctrl)
    assert_close(y, g["y"], 2e-2, "unet output with control")
    loss = F.mse_loss(y.float(), i["noise"])
    assert abs(loss.item() - g["loss"].item()) <= 1e-2 * abs(g["loss"].item())
    (loss * g["loss_scale"]).backward()
    HF.SideStream.join()
    assert all(p.grad is None for p in unet.parameters())
    for k, p in cn.named_parameters():
        assert p.grad is not None, k
        assert_close(_sampled(p.grad), g["grads"][k], 8e-2, f"control net grad {k}", abs_floor=2e-4)


def test_zero_initialised_control_changes_nothing(fixture, handover):
    g = fixture
    unet, cn = _models(g, zero_init=True)
    i = _inputs(g)
    with torch.no_grad():
        ctrl = cn(i["x_t"], i["hint"], timesteps=i["timesteps"], context=i["context"], scales=g["scales"])
        assert all(not c.any() for c in ctrl)  # exactly zero (-0.0 included)
        y0 = unet(i["x_t"], timesteps=i["timesteps"], context=i["context"])
        y1 = unet(i["x_t"], timesteps=i["timesteps"], context=i["context"], control=ctrl)
    assert torch.equal(y0, y1)


def _train_once(g, step_in_backward, **config):
    from cflearn_amd.diffusion import ControlNetTrainStep, NoiseSchedule

    unet, cn = _models(g)
    before = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    start = {k: p.detach().clone() for k, p in cn.named_parameters()}
    s = NoiseSchedule(device=DEV)
    ts = ControlNetTrainStep(unet, cn, s, control_scales=g["scales"], lr=1e-3, step_in_backward=step_in_backward, **config)
    i = _inputs(g)
    # the x whose q_sample at (timesteps, noise) is the fixture's x_t
    sh = [-1, 1, 1, 1]
    a, b = s.sqrt_alphas_cumprod[i["timesteps"]].double().view(sh), s.sqrt_one_minus_alphas_cumprod[i["timesteps"]].double().view(sh)
    x = ((i["x_t"].double() - b * i["noise"].double()) / a).float()
    loss = ts.step(x, i["hint"], i["context"], timesteps=i["timesteps"], noise=i["noise"])
    torch.cuda.synchronize()
    return ts, unet, cn, before, start, loss


def test_train_step_trains_the_control_net_and_only_it(fixture):
    g = fixture
    ts, unet, cn, before, start, loss = _train_once(g, False)
    assert abs(loss.item() - g["loss"].item()) <= 1e-2 * abs(g["loss"].item())
    for k, p in cn.named_parameters():
        assert_close(_sampled(ts.arena.grad_view(p)) * g["loss_scale"], g["grads"][k], 8e-2, f"arena grad {k}", abs_floor=2e-4)
        assert not torch.equal(p.detach(), start[k]), f"{k} did not move"
    for k, v in unet.state_dict().items():
        assert torch.equal(v, before[k]), f"the frozen UNet's {k} changed"
    assert all(p.grad is None and not p.requires_grad for p in unet.parameters())
    _, _, cn2, _, _, loss2 = _train_once(g, True)
    assert torch.equal(loss, loss2)
    for (k, p), q in zip(cn.named_parameters(), cn2.parameters()):
        assert torch.equal(p.detach(), q.detach()), f"step_in_backward changes {k}"


def test_optimizer_ranges_that_cut_the_hint_block(fixture):
    """the optimizer step inside backward in ranges of 4 KB (every hint convolution in a range of its own): a direct layer's weight is updated as soon as its own
    gradient is in, while the input gradient of that layer and the rest of the hint block's backward are still to come — they must
    not read the updated weight.  Bit-identical to the step after backward."""
    g = fixture
    _, _, cn, _, _, loss = _train_once(g, False)
    ts2, _, cn2, _, _, loss2 = _train_once(g, True, range_bytes=4096)
    ib = ts2.optimizer.in_backward
    direct = [m.weight for m in cn2.input_hint_block if isinstance(m, torch.nn.Conv2d)][:5]
    assert len({ib.range_of[ib._index[id(w)]] for w in direct}) == 5, "the five direct layers must sit in five optimizer ranges"
    assert ib.launched_in_backward > 0
    assert torch.equal(loss, loss2)
    for (k, p), q in zip(cn.named_parameters(), cn2.parameters()):
        assert torch.equal(p.detach(), q.detach()), f"4 KB optimizer ranges change {k}"


@pytest.mark.parametrize("mode", ["eager", "graph", "cfg", "cfg_two_forwards"])
@pytest.mark.parametrize("kind", ["ddim", "k_euler_a"])
def test_sampler_with_control_is_the_plain_loop(fixture, kind, mode):
    """three model evaluations with the fixture models and an explicit noise bank: bit-identical to the loop written here"""
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    g = fixture
    unet, cn = _models(g)
    i = _inputs(g)
    steps = 3 if kind == "ddim" else 4  # (a sigma-space run of n steps evaluates the model n - 1 times)
    b = i["x_t"].shape[0]
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(i["x_t"].shape, generator=gen).to(DEV)
    bank = torch.randn((3, *i["x_t"].shape), generator=gen).to(DEV)
    s = NoiseSchedule(device=DEV)
    cfg = {}
    if mode.startswith("cfg"):  # equal context lengths: one batched forward; unequal: two forwards, each with its own control list
        ulen = i["context"].shape[1] - (2 if mode == "cfg_two_forwards" else 0)
        cfg = dict(unconditional_cond=torch.randn((1, ulen, i["context"].shape[2]), generator=gen).to(DEV), unconditional_guidance_scale=3.0)
    smp = make_sampler(kind, unet, s, control_model=cn, control_scales=g["scales"], **cfg)
    got = smp.sample(z, cond=i["context"], num_steps=steps, noise=bank, hint=i["hint"], use_graph=mode == "graph")
    # the plain loop
    gb = 2 * b if mode == "cfg" else b
    st, first_in = smp._begin(z.clone(), steps, gb)
    x, table, ts = st["x"], st["table"], st["ts"]
    assert table.shape[0] == 3
    xin = torch.cat([first_in] * (gb // b)).to(BF16)
    ctx, hint = i["context"], i["hint"]
    ctx_u = cfg["unconditional_cond"].repeat_interleave(b, dim=0) if cfg else None
    if mode == "cfg":
        ctx = torch.cat([ctx, ctx_u]).contiguous()
        hint = torch.cat([hint, hint]).contiguous()
    k = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for _ in range(3):
            ctrl = cn(xin, hint, timesteps=ts, context=ctx, scales=g["scales"])
            out = unet(xin, timesteps=ts, context=ctx, control=ctrl)
            out, out_u = (out[:b].contiguous(), out[b:].contiguous()) if mode == "cfg" else (out.contiguous(), None)
            if mode == "cfg_two_forwards":
                ctrl = cn(xin, hint, timesteps=ts, context=ctx_u, scales=g["scales"])
                out_u = unet(xin, timesteps=ts, context=ctx_u, control=ctrl).contiguous()
            if kind == "ddim":
                ops.diffusion_sample_step(x, xin, out, table, k, kind=kind, parameterization="eps", out_u=out_u,
                                          scale=smp.unconditional_guidance_scale, noise=bank, temperature=1.0, clip_last=True, seed=0,
                                          offset=z.numel() // 4)
                ops.diffusion_sample_advance(k, table, ts)
            else:
                ops.k_sample_step(x, st["aux"], xin, out, table, k, kind=kind, parameterization="eps", out_u=out_u,
                                  scale=smp.unconditional_guidance_scale, noise=bank, clip_last=True, seed=0, offset=z.numel() // 4)
                ops.k_sample_advance(k, table, ts)
    assert torch.equal(got, x)


@pytest.mark.parametrize("kind", ["ddim", "k_euler_a"])
def test_sampler_with_zero_initialised_control_is_the_sampler_without(fixture, kind):
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    g = fixture
    unet, cn = _models(g, zero_init=True)
    i = _inputs(g)
    z = torch.randn(i["x_t"].shape, generator=torch.Generator().manual_seed(6)).to(DEV)
    s = NoiseSchedule(device=DEV)
    kw = dict(cond=i["context"], num_steps=4, seed=3)
    with_cn = make_sampler(kind, unet, s, control_model=cn).sample(z, hint=i["hint"], **kw)
    assert torch.equal(with_cn, make_sampler(kind, unet, s).sample(z, **kw))
