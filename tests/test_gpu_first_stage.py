"""The first stage of latent diffusion on the HIP path: the posterior kernel (cfhip_gaussian_posterior), the asymmetric
down-sampling convolution (cfhip_conv_im2row_pad / _row2im_pad), SpatialAttention, the KL autoencoder against the reference's
fp32 CPU run (tests/golden/spatial_attention.pt, ae_kl_small.pt, ae_kl_wide_outputs.pt — tools/gen_first_stage_golden.py), and
the latent paths of DDPMTrainStep and DiffusionSampler."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, assert_elementwise, bf16_round, guarded_ops, rel_l2

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# posterior kernel
# ---------------------------------------------------------------------------------------------


def _moments(bsz, e, h, w, seed):
    """bf16 moments [B, 2E, h, w] on the CPU: log_var spread over both clamp limits (-30, 20), a few elements far beyond"""
    g = _gen(seed)
    m = torch.randn((bsz, 2 * e, h, w), generator=g, dtype=torch.float64)
    m[:, e:] *= 6.0
    flat = m[:, e:].reshape(-1)
    flat[0::5] = -37.5
    flat[1::7] = 26.0
    flat[2::11] = -30.0
    flat[3::13] = 20.0
    m[:, e:] = flat.view(bsz, e, h, w)
    return m.to(BF16)


def _moments_dev(G, m, channels_last):
    if not channels_last:
        return G.poisoned(m.to(DEV))
    b, c, h, w = m.shape
    rows = G.poisoned(m.permute(0, 2, 3, 1).contiguous().to(DEV))  # [B, h, w, 2E]
    return rows.permute(0, 3, 1, 2)


POSTERIOR_CASES = [(e, hw) for e in (3, 4, 8) for hw in ((1, 1), (5, 5), (16, 16))]


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("e,hw", POSTERIOR_CASES, ids=[f"E{e}-{h * w}px" for e, (h, w) in POSTERIOR_CASES])
def test_posterior_sample(G, e, hw, channels_last):
    """z = s (mean + exp(0.5 clamp(log_var)) n) per element against float64 on the same bf16 moments, n = the kernel's own
    normals regenerated with ops.randn at the same (seed, offset).  Error model, in units of 2^-24 on cond = |s| (|mean| + std |n|):
    expf within 1 ulp (2; its argument 0.5 log_var is exact), the product std n (1), the sum (1), the product with s (1), the
    f32 rounding of scale_factor itself (1): k = 6, plus the output's own rounding (ulps = 1).  The same normals passed
    explicitly give the same bits."""
    bsz, (h, w) = 2, hw
    scale, seed, offset = 0.18215, 20240 + e, 77 + h
    m = _moments(bsz, e, h, w, 31 * e + h)
    md = _moments_dev(G, m, channels_last)
    assert md.is_contiguous() or md.is_contiguous(memory_format=torch.channels_last)
    z, kl = ops.gaussian_posterior(md, scale_factor=scale, seed=seed, offset=offset)
    assert kl is None and z.dtype == F32 and tuple(z.shape) == (bsz, e, h, w) and z.is_contiguous()
    n = ops.randn(z.numel(), seed, offset, z.device).view(z.shape)
    mean, lv = m[:, :e].double(), m[:, e:].double().clamp(-30.0, 20.0)
    std = torch.exp(0.5 * lv)
    n64 = n.cpu().double()
    assert_elementwise(z, scale * (mean + std * n64), out_dtype=F32, ulps=1, cond=abs(scale) * (mean.abs() + std * n64.abs()), k=6,
                       what=f"posterior z E{e} {h}x{w}")
    z2, _ = ops.gaussian_posterior(md, scale_factor=scale, noise=G.poisoned(n))
    assert torch.equal(z2, z), "explicit normals: another result than the Philox draw of the same normals"
    z3, _ = ops.gaussian_posterior(md, scale_factor=scale, seed=seed, offset=offset + 1)
    assert not torch.equal(z3, z), "another offset drew the same latent"


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("e,hw", POSTERIOR_CASES, ids=[f"E{e}-{h * w}px" for e, (h, w) in POSTERIOR_CASES])
def test_posterior_mode_and_kl(G, e, hw, channels_last):
    """`deterministic`: z = s * mean, exactly (one f32 product).  kl[b] = 0.5 sum (mean^2 + var - 1 - log_var) per sample against
    float64, cond = the sum of the absolute terms; k: per term mean^2 (1), expf (2) and three additions (3), the per-lane chain of
    ceil(n / 256) additions, the 6-step wave fold and the 3 additions across the four waves, the final halving being exact:
    k = 15 + ceil(n / 256)."""
    bsz, (h, w) = 3, hw
    scale = 0.18215
    m = _moments(bsz, e, h, w, 17 * e + w)
    md = _moments_dev(G, m, channels_last)
    z, kl = ops.gaussian_posterior(md, scale_factor=scale, deterministic=True, want_kl=True)
    assert torch.equal(z.cpu(), m[:, :e].float() * scale)
    mean, lv = m[:, :e].double(), m[:, e:].double().clamp(-30.0, 20.0)
    want = 0.5 * (mean ** 2 + torch.exp(lv) - 1.0 - lv).sum(dim=(1, 2, 3))
    cond = 0.5 * (mean ** 2 + torch.exp(lv) + 1.0 + lv.abs()).sum(dim=(1, 2, 3))
    n = e * h * w
    assert_elementwise(kl, want, out_dtype=F32, ulps=1, cond=cond, k=15 + -(-n // 256), what=f"posterior kl E{e} {h}x{w}")
    _, kl_only = ops.gaussian_posterior(md, want_z=False, want_kl=True)
    assert torch.equal(kl_only, kl)


# ---------------------------------------------------------------------------------------------
# asymmetric down-sampling: F.pad(x, (0, 1, 0, 1)) + conv3x3 stride 2 padding 0 as one gather + GEMM
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cout", [8, 24])
@pytest.mark.parametrize("cin", [8, 32])
@pytest.mark.parametrize("h,w", [(8, 8), (9, 7)])
def test_asymmetric_downsample_conv(h, w, cin, cout):
    """forward, dX, dW and db against F.pad + F.conv2d in float64 on the bf16-rounded operands, at the tolerances
    test_gpu_conv.py holds the im2row route to (rel-L2 4e-3 / 4e-3 / 2e-3 / 1e-5); and the symmetric padding of 1 gives another
    output, so the old route cannot pass this test"""
    bsz = 2
    g = _gen(h * 100 + w * 10 + cin + cout)
    x = bf16_round(torch.randn(bsz, cin, h, w, generator=g))
    wt = bf16_round(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5))
    bias = torch.randn(cout, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wt, bias))
    yr = F.conv2d(F.pad(xr, (0, 1, 0, 1)), wr, br, stride=2, padding=0)
    dy = bf16_round(torch.randn(yr.shape, generator=g))
    yr.backward(dy.double())
    xd = x.to(DEV).to(BF16).requires_grad_(True)
    wl, bl = wt.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    y = HF.conv2d(xd, wl, bl, 2, 0, 1, pad_hi=1)
    assert y.dtype == BF16 and tuple(y.shape) == tuple(yr.shape)
    y.backward(dy.to(DEV).to(BF16))
    HF.SideStream.join()
    assert_close(HF.to_nchw(y.detach()), yr.detach(), 4e-3, "forward")
    assert_close(HF.to_nchw(xd.grad), xr.grad, 4e-3, "dX")
    assert_close(wl.grad, wr.grad, 2e-3, "dW")
    assert_close(bl.grad, br.grad, 1e-5, "db")
    y_sym = HF.conv2d(xd.detach(), wl.detach(), bl.detach(), 2, 1, 1)
    assert tuple(y_sym.shape) == tuple(y.shape) or (h, w) == (9, 7)
    if tuple(y_sym.shape) == tuple(y.shape):
        assert rel_l2(HF.to_nchw(y_sym), yr.detach()) > 0.1, "the symmetric padding of 1 reads the same pixels?"


# ---------------------------------------------------------------------------------------------
# modules against the reference's fp32 CPU run; yardstick = the reference's own bf16-autocast run
# ---------------------------------------------------------------------------------------------

YARDSTICK = 1.25  # our rel-L2 from the fp32 result <= 1.25 x the reference's own bf16 distance from it (per output tensor)


def _golden(name):
    return torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=False)


def seeded_state(shapes, seed):
    """tools/gen_first_stage_golden.py::seeded_state, line for line: the parameters no fixture stores"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        n = torch.randn(shape, generator=g)
        if len(shape) == 1:
            out[name] = 1.0 + 0.1 * n if name.endswith("weight") else 0.1 * n
        else:
            out[name] = n / float(torch.Size(shape[1:]).numel()) ** 0.5
    return out


def _filled(module, seed):
    module.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed), strict=True)
    return module.to(DEV)


def _yardstick(got, want, ref_bf16, what):
    ours, theirs = rel_l2(got, want), rel_l2(ref_bf16, want)
    print(f"{what}: ours {ours:.3e}, reference bf16 {theirs:.3e}, ratio {ours / theirs:.2f}")
    assert ours <= YARDSTICK * theirs, f"{what}: rel-L2 {ours:.3e} vs fp32 > {YARDSTICK} x the reference's bf16 {theirs:.3e} (ratio {ours / theirs:.2f})"


SEEDS = dict(attn64=6401, attn256=25601)


@pytest.mark.parametrize("c", [64, 256])
def test_spatial_attention_forward_yardstick(c):
    """C = 64: the dispatcher's kernels; C = 256: the wide forward"""
    g = _golden("spatial_attention.pt")[c]
    m = _filled(C.SpatialAttention(c), SEEDS[f"attn{c}"]).eval()
    with torch.no_grad():
        y = m(g["x"].to(DEV))
    assert tuple(y.shape) == tuple(g["y"].shape)
    _yardstick(HF.to_nchw(y), g["y"], g["y_bf16"], f"SpatialAttention C{c} y")


def test_spatial_attention_gradients_and_guards():
    g = _golden("spatial_attention.pt")[64]
    m = _filled(C.SpatialAttention(64), SEEDS["attn64"]).eval()
    x = g["x"].to(DEV).requires_grad_(True)
    y = m(x)
    y.backward(g["gy"].to(DEV).to(y.dtype))
    HF.SideStream.join()
    _yardstick(x.grad, g["gx"], g["gx_bf16"], "SpatialAttention C64 dX")
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert sorted(grads) == sorted(g["grads"]) and len(grads) == 10
    for name, want in g["grads"].items():
        _yardstick(grads[name], want, g["grads_bf16"][name], f"SpatialAttention C64 d {name}")
    # the wide head is forward-only: an input that wants a gradient is refused by name
    wide = _filled(C.SpatialAttention(256), SEEDS["attn256"])
    xw = _golden("spatial_attention.pt")[256]["x"].to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="wide head"):
        wide(xw)
    with pytest.raises(NotImplementedError):
        C.SpatialAttention(520)
    with pytest.raises(NotImplementedError, match="multi_head_spatial"):
        C.make_attention(64, "multi_head_spatial")


def test_spatial_attention_native_lora_on_to_q():
    """a native LoRA hook on `to_q` (training mode, dropout 0): the forward is that of a hook-free module whose `to_q` filter is
    W + s up down, the product formed in float64.  Both run the same kernels; they differ by bf16 roundings of the merged filter,
    of the low-rank intermediate and of q (2^-9 relative each), which pass through the softmax logits into the output at a few
    times 2^-8: rel-L2 1e-2, the bound test_gpu_lora_conv.py holds adapted against merged weights to."""
    c = 64
    g = _golden("spatial_attention.pt")[c]
    m = _filled(C.SpatialAttention(c), SEEDS["attn64"])
    x = g["x"].to(DEV)
    with torch.no_grad():
        base = m(x).float()
    hook = C.LoRAConvHook.create_with(m.to_q, 4).to(DEV)
    hook.dropout.p = 0.0
    gen = _gen(11)
    with torch.no_grad():
        hook.lora_up.weight.copy_(torch.randn(hook.lora_up.weight.shape, generator=gen) * 0.5)
        hook.alpha.fill_(4.0)
    hook.refresh_alpha()
    hook.train()
    m.to_q.hook = hook
    y = m(x).float()
    m.to_q.hook = None
    merged = _filled(C.SpatialAttention(c), SEEDS["attn64"])
    with torch.no_grad():
        up, down = hook.lora_up.weight.double().cpu().view(c, 4), hook.lora_down.weight.double().cpu().view(4, c)
        w = merged.to_q.weight.double().cpu().view(c, c) + hook.full_scale * (up @ down)
        merged.to_q.weight.copy_(w.float().view(c, c, 1, 1).to(DEV))
        want = merged(x).float()
    assert rel_l2(want, base) > 0.05, "the adapter moves the output too little for the comparison to tell"
    assert_close(y, want, 1e-2, "SpatialAttention with a native LoRA hook on to_q vs merged weights")


@pytest.mark.parametrize("name,key", [("ae_kl_small.pt", "small"), ("ae_kl_wide_outputs.pt", "wide")])
def test_ae_kl_against_reference(name, key):
    """encode (the moments) and decode(mode) of the whole autoencoder: 64-wide attention on the dispatcher's kernels (small) and a
    512-wide bottleneck on the wide forward (wide), every layer type, both narrow 1x1 embeddings"""
    g = _golden(name)
    m = C.registry.generators.build("ae_kl", config=dict(g["cfg"]))
    m = _filled(m, g["seed"]).eval()
    with torch.no_grad():
        dist = m.encode(g["x"].to(DEV))
        moments = HF.to_nchw(dist.net)
        decoded = HF.to_nchw(m.decode(C.DecoderInputs(z=dist.mode())))
        rec = m.reconstruct(g["x"].to(DEV))
    assert tuple(moments.shape) == tuple(g["moments"].shape) and tuple(decoded.shape) == tuple(g["decoded"].shape)
    assert torch.equal(HF.to_nchw(rec), decoded)
    _yardstick(moments, g["moments"], g["moments_bf16"], f"ae_kl {key} moments")
    _yardstick(decoded, g["decoded"], g["decoded_bf16"], f"ae_kl {key} decode(mode)")
    with pytest.raises(NotImplementedError, match="apply_tanh"):
        m.decode(C.DecoderInputs(z=dist.mode(), apply_tanh=True))
    with torch.no_grad():
        feats = m.decode(C.DecoderInputs(z=dist.mode(), no_head=True))
    assert feats.shape[1] == g["cfg"]["inner_channels"] * g["cfg"]["channel_multipliers"][0]
    kl = dist.kl()
    mean, lv = moments.double().cpu()[:, :4], moments.double().cpu()[:, 4:].clamp(-30, 20)
    assert_close(kl, 0.5 * (mean ** 2 + lv.exp() - 1 - lv).sum(dim=(1, 2, 3)), 1e-5, "GaussianDistribution.kl")


# ---------------------------------------------------------------------------------------------
# the latent path: DDPMTrainStep / DiffusionSampler with a first stage
# ---------------------------------------------------------------------------------------------

SCALE = 0.18215


def _small_ae():
    g = _golden("ae_kl_small.pt")
    return _filled(C.registry.generators.build("ae_kl", config=dict(g["cfg"])), g["seed"]), g


def _small_unet():
    """the small UNet of test_gpu_lora_conv.py (4 latent channels in and out), zero-initialised convolutions filled"""
    from cflearn_amd import modules as M

    torch.manual_seed(7)
    unet = M.UNetDiffuser(4, 4, num_head_channels=32, use_spatial_transformer=True, start_channels=32, num_res_blocks=1,
                          attention_downsample_rates=(1,), channel_multipliers=(1, 2))
    gen = _gen(8)
    with torch.no_grad():
        for p in unet.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=gen) * (0.5 / max(1, p[0].numel()) ** 0.5))
    return unet.to(DEV)


def test_latent_train_step():
    from cflearn_amd.diffusion import DDPMTrainStep, NoiseSchedule

    ae, g = _small_ae()
    before = {k: v.clone() for k, v in ae.state_dict().items()}
    img = g["x"].to(DEV)
    gen = _gen(21)
    batches = [(torch.randint(0, 1000, (2,), generator=gen).to(DEV), torch.randn((2, 4, 8, 8), generator=gen).to(DEV)) for _ in range(3)]
    seed = 4242
    ts = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3, first_stage=ae, first_stage_scale_factor=SCALE)
    assert not ae.training and all(not p.requires_grad for p in ae.parameters())
    arena_ids = {id(p) for p in ts.arena.params}
    assert arena_ids and not any(id(p) in arena_ids for p in ae.parameters())
    # the same step by hand: encode -> posterior kernel with that seed -> a step without a first stage
    with torch.no_grad():
        dist = ae.encode(img)
        latent0, _ = ops.gaussian_posterior(dist.net, scale_factor=SCALE, seed=seed, offset=0)
        latent1, _ = ops.gaussian_posterior(dist.net, scale_factor=SCALE, seed=seed, offset=ts.latent_draw(1, latent0.numel(), seed)[1])
    assert tuple(latent0.shape) == (2, 4, 8, 8) and not torch.equal(latent0, latent1)
    plain = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3)
    losses, losses_plain = [], []
    for (t, eps), latent in zip(batches[:2], (latent0, latent1)):
        losses.append(ts.step(img, timesteps=t, noise=eps, seed=seed).item())
        losses_plain.append(plain.step(latent, timesteps=t, noise=eps).item())
    HF.SideStream.join()
    torch.cuda.synchronize()
    assert losses == losses_plain, (losses, losses_plain)  # (step 2 equal: the second draw is the stream's next block, not the first again)
    for (n, p), (_, q) in zip(ts.unet.named_parameters(), plain.unet.named_parameters()):
        assert torch.equal(p, q), f"{n}: the updated parameters differ from the step fed the hand-made latent"
    for k, v in ae.state_dict().items():
        assert torch.equal(v, before[k]), f"first stage {k} changed"
    assert all(p.grad is None for p in ae.parameters())
    # the mode: no draw
    det = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3, first_stage=ae, first_stage_scale_factor=SCALE)
    plain2 = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3)
    t, eps = batches[0]
    assert det.step(img, timesteps=t, noise=eps, deterministic=True).item() == plain2.step(dist.mode(scale_factor=SCALE), timesteps=t, noise=eps).item()
    with pytest.raises(ValueError):
        plain2.step(latent0, timesteps=t, noise=eps, deterministic=True)


def test_latent_train_step_as_a_hipgraph_matches_eager():
    """the encode and the posterior kernel are inside the recorded body; the normals of each step are drawn in front of the replay
    from the step's own (seed, offset): the third replayed step has the eager loss (2e-3 relative, the bound
    test_gpu_unet.py::test_ddpm_train_step_as_a_hipgraph_matches_the_eager_step holds the UNet alone to)"""
    from cflearn_amd.diffusion import DDPMTrainStep, NoiseSchedule

    gen = _gen(22)
    batches = [(torch.randint(0, 1000, (2,), generator=gen).to(DEV), torch.randn((2, 4, 8, 8), generator=gen).to(DEV)) for _ in range(3)]
    losses = {}
    for graph in (False, True):
        ae, g = _small_ae()
        ts = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3, use_graph=graph, first_stage=ae, first_stage_scale_factor=SCALE,
                           first_stage_seed=99)
        losses[graph] = [ts.step(g["x"].to(DEV), timesteps=t, noise=eps).item() for t, eps in batches]
    assert len(set(losses[False])) == 3
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) <= 2e-3 * abs(b) + 1e-5, (losses[True], losses[False])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_latent_sampler_decodes(use_graph):
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    ae, _ = _small_ae()
    unet = _small_unet().eval()
    z = torch.randn((2, 4, 8, 8), generator=_gen(23)).to(DEV)
    sampler = make_sampler("ddim", unet, NoiseSchedule(device=DEV), first_stage=ae, first_stage_scale_factor=SCALE)
    img = sampler.sample(z, num_steps=3, use_graph=use_graph)
    latent = sampler.sample(z, num_steps=3, use_graph=use_graph, return_latent=True)
    assert tuple(latent.shape) == (2, 4, 8, 8) and latent.dtype == F32 and tuple(img.shape) == (2, 3, 16, 16)
    with torch.no_grad():
        want = ae.decode(C.DecoderInputs(z=latent / SCALE))
    assert torch.equal(img, want)
    assert float(latent.abs().max()) <= 1.0  # clip_output acts on the latent
    plain = make_sampler("ddim", unet, NoiseSchedule(device=DEV)).sample(z, num_steps=3, use_graph=use_graph)
    assert torch.equal(plain, latent)
