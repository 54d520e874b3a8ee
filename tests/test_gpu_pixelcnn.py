"""The PixelCNN prior on the GPU: the module against the reference's recorded logits and gradients, and the sampling kernel of
csrc/pixelcnn.hip.

Bounds.  Against the reference's fp32 numbers everything has to stay within 1.1 x the distance the reference itself shows under
torch.autocast("cpu", bfloat16) (recorded per quantity in tests/golden/pixelcnn_small.pt; 1.1 is the project's standing margin).
The sampler is also checked per element, layer by layer, against the float64 replica of tests/pixelcnn_replay.py fed the bf16
activations the kernel itself left for the layer below, so each bound covers ONE layer's arithmetic as the kernel's header states it:
an f32 chain of T Cin products (exact: bf16 x bf16 fits f32) and the fma of the affine — k = T Cin + 2 roundings on the absolute sum —
then one bf16 rounding (1 ulp: the f32 error may cross a rounding boundary); the head: C + 1 roundings, f32 output.  Everything that
concerns the split of a walk into launches, the batch size or a repeated seed is checked bit for bit."""
import numpy as np
import pytest
import torch

from helpers import GuardedOps, assert_elementwise, rel_l2
import pixelcnn_replay as R
from pixelcnn_weights import fill_parameters, grad_positions

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd import ops, pixelcnn  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MARGIN = 1.1


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pixelcnn_small.pt")


def _model(rec, train=False):
    m = C.PixelCNN(**rec["kwargs"])
    fill_parameters(m, rec["seed"])
    return m.to(DEV).train(train)


def _labels(rec):
    return None if rec["labels"] is None else rec["labels"].to(DEV)


def _nhwc(logits_nchw):
    return logits_nchw.permute(0, 2, 3, 1).contiguous()


# ---- the module ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("index", range(3))
def test_module_eval_logits_against_the_reference(fx, index):
    rec = fx["configs"][index]
    m = _model(rec)
    with torch.no_grad():
        y = m(rec["codes"].to(DEV), _labels(rec))
    assert tuple(y.shape) == tuple(rec["eval_logits"].shape)
    d = rel_l2(y, rec["eval_logits"])
    print(f"{rec['name']}: eval logits rel-L2 {d:.3e} (reference's own bf16 distance {rec['eval_dist']:.3e})")
    assert d <= MARGIN * rec["eval_dist"], (rec["name"], d, rec["eval_dist"])
    # a checkpoint written after a forward holds the zeroed taps, as the reference's does
    for l in range(rec["kwargs"]["num_layers"]):
        conv = m.net[l][0]
        assert not conv.weight.data[conv.mask == 0].any()


@pytest.mark.parametrize("index", range(3))
def test_module_train_logits_and_gradients_against_the_reference(fx, index):
    rec = fx["configs"][index]
    m = _model(rec, train=True)
    y = m(rec["codes"].to(DEV), _labels(rec))
    (y.float() * rec["dy"].to(DEV)).sum().backward()
    HF.SideStream.join()
    torch.cuda.synchronize()
    d = rel_l2(y, rec["train_logits"])
    print(f"{rec['name']}: train logits rel-L2 {d:.3e} (reference's own bf16 distance {rec['train_dist']:.3e})")
    assert d <= MARGIN * rec["train_dist"], (rec["name"], d, rec["train_dist"])
    masks = {k[:-len("mask")] + "weight": v.reshape(-1).cpu() for k, v in m.named_buffers() if k.endswith(".mask")}
    worst = []
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        pos = grad_positions(p.numel())
        got, want = p.grad.detach().float().cpu().reshape(-1)[pos], rec["grads"][name]
        if name in masks:
            live = masks[name][pos] != 0
            assert int((~live).sum()) > 0 and not got[~live].any(), f"{name}: the gradient of a masked tap must be exactly zero"
            assert not p.grad[m.get_buffer(name[:-len("weight")] + "mask") == 0].any(), name
            got, want = got[live], want[live]
        dg = rel_l2(got, want)
        print(f"{rec['name']} {name}: grad rel-L2 {dg:.3e} (reference's own {rec['grad_dist'][name]:.3e})")
        if dg > MARGIN * rec["grad_dist"][name]:
            worst.append((name, dg, rec["grad_dist"][name]))
    assert not worst, worst


@pytest.mark.parametrize("arena", [False, True])
def test_masked_taps_stay_zero_for_an_arena_parameter(arena):
    """the in-place zeroing must reach the values the convolution multiplies, for a parameter inside a ParamArena too: poisoning the
    masked taps of the parameter before a forward changes nothing"""
    torch.manual_seed(3)
    conv = C.MaskedConv2d("B", 32, 32, kernel_size=7, bias=False).to(DEV)
    if arena:
        arena = C.ParamArena([conv.weight])  # noqa: F841 (kept alive)
    x = torch.randn(2, 32, 5, 6, device=DEV)
    with torch.no_grad():
        y0 = conv(x).clone()
        conv.weight.data[conv.mask == 0] = 3.0
        HF.shadow_bf16(conv.weight)  # somebody casts the poisoned values into the shadow
        y1 = conv(x)
    assert torch.equal(y0, y1) and not conv.weight.data[conv.mask == 0].any()
    assert not HF.shadow_bf16(conv.weight)[conv.mask == 0].any()


@pytest.mark.parametrize("index", range(3))
def test_module_is_causal_on_the_device(fx, index):
    rec = fx["configs"][index]
    m = _model(rec)
    codes = rec["codes"].to(DEV)
    other = codes.clone()
    other[:, :, 4, 5] = (other[:, :, 4, 5] + 7) % rec["kwargs"]["num_codes"]
    with torch.no_grad():
        y0, y1 = m(codes, _labels(rec)), m(other, _labels(rec))
    w = codes.shape[-1]
    same = (y0 == y1).all(dim=1).reshape(codes.shape[0], -1)
    assert bool(same[:, :4 * w + 5 + 1].all()), "a logit at or before the changed pixel moved"
    assert not bool(same[:, 4 * w + 6].all())


# ---- the sampler, teacher-forced -------------------------------------------------------------------------------------------------


def _guarded_state(g, m, b, size_hw, k, forced=None, return_logits=True):
    h, w = size_hw
    cin0 = m.latent_channels if m.need_embedding else 1
    codes = g.index(forced.to(DEV) if forced is not None else torch.zeros((b, 1, h, w), dtype=torch.int64, device=DEV))
    return pixelcnn.SamplerState(codes, g.empty((b, h, w, cin0), dtype=BF16, device=DEV),
                                 g.empty((m.num_layers, b, h, w, m.latent_channels), dtype=BF16, device=DEV),
                                 g.empty((b, h, w, k) if return_logits else (b, k), dtype=F32, device=DEV))


@pytest.mark.parametrize("index", range(3))
def test_forced_sampler_against_the_reference_and_the_replica(fx, index):
    rec = fx["configs"][index]
    kw = rec["kwargs"]
    m = _model(rec)
    b, _, h, w = rec["codes"].shape
    k = kw["num_codes"]
    g = GuardedOps()
    state = _guarded_state(g, m, b, (h, w), k, forced=rec["codes"])  # NaN-filled: nothing unwritten may reach a result
    plan = m.sampler_plan(_labels(rec), b)
    m.sample_pixels(plan, state, 0, h * w, forced=True)
    g.check()
    assert torch.equal(state.codes.cpu(), rec["codes"])
    logits = state.logits
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(state.act.float()).all())
    d = rel_l2(logits, _nhwc(rec["eval_logits"]))
    print(f"{rec['name']}: forced sampler logits rel-L2 {d:.3e} (reference's own bf16 distance {rec['eval_dist']:.3e})")
    assert d <= MARGIN * rec["eval_dist"], (rec["name"], d, rec["eval_dist"])
    # the same through the public call
    codes2, logits2 = m.sample(b, img_size=h, labels=_labels(rec), forced=rec["codes"][:, :, :, :h].contiguous(), return_logits=True)
    assert tuple(logits2.shape) == (b, h, h, k) and torch.equal(codes2.cpu(), rec["codes"][:, :, :, :h])
    # ---- per element, one layer at a time, from what the kernel left below ----
    rows = plan.label_row.long()
    table = plan.in_table[rows[:, None, None], state.codes[:, 0]]  # [B, H, W, Cin0]
    assert torch.equal(state.in0, table)
    _check_layers_and_head(m, plan, state, rec["name"])


def _check_layers_and_head(m, plan, state, tag):
    """every layer and the head per element, each from the bf16 activations the kernel left below it"""
    k, nl = m.num_codes, m.num_layers
    below = state.in0.cpu()
    for l in range(nl):
        conv = m.net[l][0]
        want, cond = R.layer_step64(below, conv.weight.detach().cpu(), "A" if l == 0 else "B", plan.scale[l].cpu(), plan.shift[l].cpu())
        taps_cin = (24 if l == 0 else 25) * conv.weight.shape[1]
        assert_elementwise(state.act[l], want, out_dtype=BF16, ulps=1, cond=cond, k=taps_cin + 2, what=f"{tag} layer {l}")
        below = state.act[l].cpu()
    head = m.net[nl]
    want, cond = R.head_step64(below, head.weight.detach().cpu().view(k, -1), head.bias.detach().cpu())
    assert_elementwise(state.logits, want, out_dtype=F32, ulps=1, cond=cond, k=m.latent_channels + 1, what=f"{tag} logits")


@pytest.mark.parametrize("c,k,b,embedding,norm", [(128, 100, 17, False, "batch"), (160, 100, 17, True, None), (256, 1024, 3, False, "batch")])
def test_wide_nets_take_the_other_kernel_paths(c, k, b, embedding, norm):
    """what the fixture's configurations do not reach: one full tile per wave (128 channels), two tiles per wave with a second tile past
    the layer's width on some waves (160) and on none (256), a code count that is no multiple of 16 or 64 and the largest one (16 codes
    per lane in the draw), a last workgroup with one row of 16.  Free-running, so the draw is checked too; then per element.
    Undecidable draws: the expected share is at most 2e-5 K = 2 % at K = 1024; on these 45 .. 255 pixels 10 % is never reached by chance."""
    h, w, seed, offset = 3, 5, 77, 9
    m = C.PixelCNN(k, 1, embedding, c, norm_type=norm, num_layers=2, num_classes=3)
    fill_parameters(m, 4000 + c)
    m = m.to(DEV).eval()
    labels = torch.arange(b, device=DEV) % 3
    g = GuardedOps()
    state = _guarded_state(g, m, b, (h, w), k)
    plan = m.sampler_plan(labels, b)
    m.sample_pixels(plan, state, 0, h * w, seed=seed, offset=offset)
    g.check()
    assert bool(torch.isfinite(state.logits).all())
    pick, margin = R.draw64(state.logits.cpu().numpy(), R.uniforms(b, h, w, seed, offset))
    decidable = margin > 1e-5
    got = state.codes[:, 0].cpu().numpy()
    assert np.array_equal(got[decidable], pick[decidable]) and decidable.mean() >= 0.9, (int((got != pick)[decidable].sum()), decidable.mean())
    assert torch.equal(state.in0, plan.in_table[plan.label_row.long()[:, None, None], state.codes[:, 0]])
    _check_layers_and_head(m, plan, state, f"C={c} K={k} B={b}")


@pytest.mark.parametrize("index", range(3))
def test_one_launch_equals_chained_launches(fx, index):
    rec = fx["configs"][index]
    m = _model(rec)
    b, h, w, k = 3, 5, 6, rec["kwargs"]["num_codes"]
    labels = None if rec["labels"] is None else torch.tensor([1, 3, 1], device=DEV)
    plan = m.sampler_plan(labels, b)

    def walk(cuts):
        g = GuardedOps()
        state = _guarded_state(g, m, b, (h, w), k)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            m.sample_pixels(plan, state, lo, hi, seed=99, offset=3)
        g.check()
        return state

    whole = walk([0, h * w])
    assert whole.codes.min() >= 0 and whole.codes.max() < k and whole.codes.unique().numel() > 2
    for name, cuts in (("one pixel each", list(range(h * w + 1))), ("rows", list(range(0, h * w + 1, w))), ("uneven", [0, 1, 8, 8, 21, h * w])):
        part = walk(cuts)
        for field in ("codes", "logits", "in0", "act"):
            a, c = getattr(whole, field), getattr(part, field)
            assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)), f"{rec['name']} {name}: {field} differs"


# ---- the draw ------------------------------------------------------------------------------------------------------------------------


def test_draw_follows_the_philox_stream(fx):
    rec = fx["configs"][0]
    m = _model(rec)
    b, s, k, seed, offset = 32, 8, rec["kwargs"]["num_codes"], 0x5EED5EED5EED, 1 << 33
    codes, logits = m.sample(b, img_size=s, seed=seed, offset=offset, return_logits=True)
    u = R.uniforms(b, s, s, seed, offset)
    pick, margin = R.draw64(logits.cpu().numpy(), u)
    decidable = margin > 1e-5
    got = codes[:, 0].cpu().numpy()
    assert np.array_equal(got[decidable], pick[decidable]), f"{int((got != pick)[decidable].sum())} decidable pixels differ"
    undecidable = 1.0 - decidable.mean()
    print(f"draw: {undecidable:.2%} of {decidable.size} pixels undecidable, {np.unique(got).size} distinct codes")
    assert undecidable <= 0.01 and np.unique(got).size > k // 2
    # the stream is the seed's and the offset's, nothing else
    again = m.sample(b, img_size=s, seed=seed, offset=offset)
    assert torch.equal(again, codes)
    assert not torch.equal(m.sample(b, img_size=s, seed=seed, offset=offset + 1), codes)
    assert not torch.equal(m.sample(b, img_size=s, seed=seed + 1, offset=offset), codes)
    # rows 0 .. 15 of a B = 32 call are a B = 16 call
    half, half_logits = m.sample(16, img_size=s, seed=seed, offset=offset, return_logits=True)
    assert torch.equal(half, codes[:16]) and torch.equal(half_logits, logits[:16])


def test_draw_distribution():
    """every conv and head weight zero: each pixel is a draw from softmax(head bias), whatever was drawn before.  Chi-square of the 4096
    draws against it, 7 degrees of freedom: below 29.88, the 1e-4 critical value"""
    k, b, s = 8, 64, 8
    m = C.PixelCNN(k, 1, latent_channels=32, num_layers=2).to(DEV).eval()
    probs = torch.arange(1, k + 1, dtype=torch.float64) / 36.0
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("net.") and p.dim() == 4:
                p.zero_()
        m.net[2].bias.copy_(probs.log().float())
    codes = m.sample(b, img_size=s, seed=20261020)
    counts = torch.bincount(codes.reshape(-1).cpu(), minlength=k).double()
    expected = probs * b * s * s
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"chi-square {chi2:.2f} (counts {counts.tolist()})")
    assert counts.sum() == b * s * s and chi2 < 29.88


def test_a_sample_call_is_one_sampling_launch(monkeypatch):
    """the walk over the pixels is ONE cfhip_pixelcnn_sample launch whatever img_size is, behind num_layers + 1 pack calls; and the whole
    call — the torch operations of the preparation included, as the profiler records them on the host — is the same sequence of
    operations at every img_size"""
    m = C.PixelCNN(16, 1, latent_channels=32, num_layers=3).to(DEV).eval()
    calls = []
    real_sample, real_pack = ops.pixelcnn_sample, ops.pixelcnn_pack
    monkeypatch.setattr(ops, "pixelcnn_sample", lambda *a, **kw: (calls.append("sample"), real_sample(*a, **kw))[1])
    monkeypatch.setattr(ops, "pixelcnn_pack", lambda *a, **kw: (calls.append("pack"), real_pack(*a, **kw))[1])
    m.sample(3, img_size=2, seed=1)  # (lazy initialisations)
    sequences = []
    for size in (2, 4, 9):
        calls.clear()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            out = m.sample(3, img_size=size, seed=1)
        assert tuple(out.shape) == (3, 1, size, size)
        assert calls == ["pack"] * 4 + ["sample"], (size, calls)
        sequences.append([e.name for e in prof.events() if e.name.startswith("aten::")])
    assert sequences[0] == sequences[1] == sequences[2] and len(sequences[0]) > 0


# ---- the live-tap convolution kernels of csrc/conv_masked.hip, per element -----------------------------------------------------------
# Bounds: the forward / dX are one f32 chain of T Ci exact products (bf16 x bf16 fits f32) plus the bias, k = T Ci + 1 roundings on the
# same sum of absolute values, then one bf16 rounding (1 ulp: the f32 error may cross a rounding boundary).  dW is the tn GEMM's f32 sum
# over the B H W rows, in row chunks added in f32: k = B H W + (chunks) + 1 on the absolute sum, 1 ulp of the f32 result.

CHANNELS = [(32, 32), (64, 32), (96, 64), (128, 128)]
SHAPES = [(1, 1, 1), (2, 5, 7), (1, 9, 33), (2, 11, 37)]  # edges narrower than the halo; a tile edge crossed in both directions


def _conv_case(cin, cout, b, h, w, mask_type):
    gen = torch.Generator().manual_seed(cin * 131 + cout * 17 + b * 7 + h * 3 + w + (mask_type == "B"))
    x = torch.randn(b, cin, h, w, generator=gen).to(BF16)
    wt = (torch.randn(cout, cin, 7, 7, generator=gen) * (2.0 / (25 * cin) ** 0.5)).to(BF16).float()
    bias = torch.randn(cout, generator=gen) * 0.3
    dy = torch.randn(b, cout, h, w, generator=gen).to(BF16)
    return x, wt, bias, dy


def _rows(t):  # [B, C, H, W] -> NHWC rows
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _ref_backward(x, wt, dy, mask_type):
    """float64 dX and dW of the masked convolution with their sums of absolute values"""
    m = R.mask_of(mask_type)
    x64, w64, dy64 = x.double().requires_grad_(True), (wt.double() * m).requires_grad_(True), dy.double()
    torch.nn.functional.conv2d(x64, w64, padding=3).backward(dy64)
    xa, wa = x.double().abs().requires_grad_(True), (wt.double().abs() * m).requires_grad_(True)
    torch.nn.functional.conv2d(xa, wa, padding=3).backward(dy64.abs())
    return x64.grad, w64.grad * m, xa.grad, wa.grad * m


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_masked_kernel_forward_and_dx_per_element(mask_type, cin, cout, b, h, w, monkeypatch):
    from helpers import guarded_ops

    taps = ops.MASKED_TAPS[mask_type]
    x, wt, bias, dy = _conv_case(cin, cout, b, h, w, mask_type)
    g = guarded_ops(monkeypatch)  # every output of ops.* sits between guard bytes
    xr, dyr = g.poisoned(_rows(x).to(DEV)), g.poisoned(_rows(dy).to(DEV))
    wd = wt.to(DEV)
    want, cond = R.masked_conv64(x, wt, mask_type)
    for with_bias in (False, True):
        y = ops.conv_masked(xr, ops.conv_masked_pack(wd, taps), bias.to(DEV) if with_bias else None, b, h, w, taps)
        ref = want + bias.double().view(1, -1, 1, 1) if with_bias else want
        cnd = cond + bias.double().abs().view(1, -1, 1, 1) if with_bias else cond
        assert_elementwise(y, _rows(ref), out_dtype=BF16, ulps=1, cond=_rows(cnd), k=taps * cin + 1, what=f"forward bias={with_bias}")
    # the masked taps of the source weight are never read: NaN there, bit-identical output
    poisoned = torch.where(R.mask_of(mask_type).bool(), wt, torch.full_like(wt, float("nan"))).to(DEV)
    y0 = ops.conv_masked(xr, ops.conv_masked_pack(wd, taps), None, b, h, w, taps)
    y1 = ops.conv_masked(xr, ops.conv_masked_pack(poisoned, taps), None, b, h, w, taps)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    dx_want, _, dx_cond, _ = _ref_backward(x, wt, dy, mask_type)
    dx = ops.conv_masked(dyr, ops.conv_masked_pack(poisoned, taps, transposed=True), None, b, h, w, taps, mirror=True)
    assert_elementwise(dx, _rows(dx_want), out_dtype=BF16, ulps=1, cond=_rows(dx_cond), k=taps * cout + 1, what="dX")
    g.check()


@pytest.mark.parametrize("b,h,w", SHAPES)
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_masked_weight_gradient_per_element(mask_type, cin, cout, b, h, w, monkeypatch):
    """through MaskedConv2dFn, each shape run twice: a direct leaf adds on the second pass, an arena slot is overwritten after a lazy
    zero-grad; the workspace is cut down so that the larger shapes take several row chunks"""
    taps = ops.MASKED_TAPS[mask_type]
    x, wt, _, dy = _conv_case(cin, cout, b, h, w, mask_type)
    monkeypatch.setattr(ops, "MASKED_GATHER_BYTES", 300 * 2 * taps * cin)  # chunks of 296 rows
    chunks = -(-b * h * w // 296)
    _, dw_want, _, dw_cond = _ref_backward(x, wt, dy, mask_type)
    masked = (R.mask_of(mask_type) == 0).expand(cout, cin, 7, 7)
    xd, dyd = x.to(DEV), dy.to(DEV)
    for arena in (False, True):
        weight = torch.nn.Parameter(wt.clone().to(DEV))
        holder = C.ParamArena([weight]) if arena else None
        passes = []
        for _ in range(2):
            if arena:
                holder.zero_grad(lazy=True)
            pixelcnn.masked_conv2d(xd, weight, None, taps).backward(dyd)
            HF.SideStream.join()
            torch.cuda.synchronize()
            passes.append(weight.grad.detach().clone())
        assert_elementwise(passes[0], dw_want, out_dtype=F32, ulps=1, cond=dw_cond, k=b * h * w + chunks + 1, what=f"dW arena={arena}")
        assert not passes[0][masked].any() and not passes[1][masked].any(), "the gradient of a masked tap must be exactly zero"
        if arena:
            assert torch.equal(passes[1], passes[0]), "an arena slot is overwritten after a lazy zero-grad"
        else:
            assert torch.equal(passes[1], passes[0] * 2), "a direct leaf adds on the second pass"


def test_frozen_masked_weight_causes_no_weight_gradient_launch(monkeypatch):
    calls = []
    real_gather, real_gemm = ops.conv_masked_gather, ops.gemm
    monkeypatch.setattr(ops, "conv_masked_gather", lambda *a, **kw: (calls.append("gather"), real_gather(*a, **kw))[1])
    monkeypatch.setattr(ops, "gemm", lambda *a, **kw: (calls.append("gemm"), real_gemm(*a, **kw))[1])
    conv = C.MaskedConv2d("B", 32, 32, kernel_size=7, bias=False).to(DEV)
    x = torch.randn(2, 32, 5, 7, device=DEV, requires_grad=True)
    for frozen in (True, False):
        conv.weight.requires_grad_(not frozen)
        conv.weight.grad = None
        calls.clear()
        conv(x).float().sum().backward()
        HF.SideStream.join()
        torch.cuda.synchronize()
        if frozen:
            assert calls == [] and conv.weight.grad is None and x.grad is not None
        else:
            assert calls == ["gather", "gemm"] and conv.weight.grad is not None


def test_masked_route_equals_the_unmasked_one_closely(monkeypatch):
    """the module on the live-tap kernels against the same module on Conv2dFn with the zeroed weight: the same products, summed in
    another order and rounded once to bf16 — within two bf16 ulps' worth of rel-L2"""
    torch.manual_seed(5)
    conv = C.MaskedConv2d("B", 64, 32, kernel_size=7, bias=True).to(DEV)
    x = torch.randn(2, 64, 9, 11, device=DEV)
    with torch.no_grad():
        y_masked = conv(x)
        monkeypatch.setattr(HF, "MASKED_CONV", False)
        y_plain = conv(x)
    assert tuple(y_masked.shape) == tuple(y_plain.shape) and rel_l2(y_masked, y_plain) < 2 * 2.0 ** -8
