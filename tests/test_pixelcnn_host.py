"""The PixelCNN prior without a GPU: registry and export, state-dict parity with the reference's recorded keys, checkpoint round
trips, the mask values, `get_conv_blocks(conv_base=...)`, `ChannelPadding`'s shapes, the C-ABI declaration and build lists, every
refusal that must fire before a launch, and the float64 replicas of tests/pixelcnn_replay.py (the masked convolution against
torch.nn.functional.conv2d and its causality, the draw against a hand case, the consumed Philox counters)."""
import os
import re

import numpy as np
import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, modules, ops, pixelcnn, registry

import philox_ref as P
import pixelcnn_replay as R
from pixelcnn_weights import fill_parameters, seeded_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pixelcnn_small.pt")


def test_registry_and_export():
    assert registry.auto_regressors.get("pixel_cnn") is C.PixelCNN
    assert C.module_dict["auto_regressors.pixel_cnn"] is C.PixelCNN
    m = C.build_auto_regressor("pixel_cnn", num_codes=8, in_channels=1, latent_channels=32, num_layers=2, unknown_keyword=1)
    assert isinstance(m, C.PixelCNN) and isinstance(m.net[0][0], C.MaskedConv2d) and isinstance(m.channel_padding, C.ChannelPadding)
    assert not m.is_conditional and m.get_sample_labels(3) is None

    @C.register_auto_regressor("pixelcnn_host_test_entry")
    class Other(torch.nn.Module):
        pass

    assert registry.auto_regressors.has("pixelcnn_host_test_entry")
    del C.module_dict["auto_regressors.pixelcnn_host_test_entry"]


@pytest.mark.parametrize("index", range(3))
def test_state_dict_matches_reference(fx, index):
    rec = fx["configs"][index]
    m = C.PixelCNN(**rec["kwargs"])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in rec["state"]], rec["name"]


@pytest.mark.parametrize("index", range(3))
def test_checkpoint_round_trip(fx, index):
    rec = fx["configs"][index]
    m = C.PixelCNN(**rec["kwargs"])
    state = seeded_state(m, rec["seed"])
    m.load_state_dict(state, strict=True)
    back = m.state_dict()
    assert list(back) == [k for k, _ in rec["state"]] and all(torch.equal(back[k], state[k]) for k in state)


def test_in_channels_refusal():
    with pytest.raises(ValueError, match="`PixelCNN` requires `in_channels` to be 1"):
        C.PixelCNN(16)  # the reference's default in_channels = 3 is refused there too
    with pytest.raises(ValueError, match="`channel_padding` should be provided"):
        C.PixelCNN(16, 1, channel_padding=None, num_classes=3)


@pytest.mark.parametrize("k", [7, 3])
@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_mask_values(mask_type, k):
    conv = C.MaskedConv2d(mask_type, 2, 3, kernel_size=k)
    assert conv.mask.shape == conv.weight.shape and "mask" in dict(conv.named_buffers())
    c = k // 2
    want = torch.zeros(k, k)
    want[:c] = 1.0
    want[c, :c + (mask_type == "B")] = 1.0
    assert torch.equal(conv.mask, want.expand(3, 2, k, k))
    assert int(want.sum()) == {(7, "A"): 24, (7, "B"): 25, (3, "A"): 4, (3, "B"): 5}[(k, mask_type)]
    assert torch.equal(R.mask_of(mask_type, k).float(), want)
    # the replica's tap order is the pack's: the live taps are the first T row-major positions of the window
    assert [i * k + j for i, j in R.live_taps(mask_type, k)] == list(range(int(want.sum())))
    with pytest.raises(ValueError, match="mask_type"):
        C.MaskedConv2d("C", 2, 3, kernel_size=k)


def test_zeroing_is_in_place_and_drops_the_shadow_key():
    conv = C.MaskedConv2d("A", 2, 3, kernel_size=7, bias=False)
    with torch.no_grad():
        conv.weight.fill_(1.0)
    conv.weight._cfhip_shadow_version = conv.weight._version  # as if a shadow had been cast from the unmasked values
    version = conv.weight._version
    conv.zero_masked_taps()
    assert torch.equal(conv.weight.data, conv.mask) and conv.weight._version == version
    assert conv.weight._cfhip_shadow_version is None
    w = conv._effective_weight(None)
    (w * torch.ones_like(w)).sum().backward()
    assert torch.equal(conv.weight.grad, conv.mask)  # the gradient of a masked tap is exactly zero


def test_get_conv_blocks_conv_base():
    plain = modules.get_conv_blocks(4, 8, 3, 1, norm_type="batch", activation="leaky_relu_0.2", padding=1)
    assert [type(b) for b in plain] == [C.Conv2d, C.BatchNorm2d, modules.LeakyReLU] and type(plain[0]) is C.Conv2d
    assert plain[0].bias is not None and plain[0].padding == 1 and plain[0].stride == 1
    masked = modules.get_conv_blocks(4, 8, 7, 1, bias=False, norm_type=None, activation=modules.LeakyReLU(0.2), conv_base=C.MaskedConv2d,
                                     padding=3, mask_type="B")
    assert [type(b) for b in masked] == [C.MaskedConv2d, torch.nn.Identity, modules.LeakyReLU]  # the block keeps its Sequential indices
    assert masked[0].mask_type == "B" and masked[0].bias is None and masked[0].in_c == 4 and masked[0].out_c == 8


def test_channel_padding_forms():
    for kw, shape in ((dict(), (1, 6, 1, 1)), (dict(map_dim=5), (1, 6, 5, 5)), (dict(num_classes=3), (3, 6, 1, 1)),
                      (dict(map_dim=5, num_classes=3), (3, 6, 5, 5))):
        m = C.ChannelPadding(2, 6, **kw)
        assert tuple(m.channel_padding.shape) == shape and isinstance(m.mapping, C.Conv2d)
        assert tuple(m.mapping.weight.shape) == (2, 8, 1, 1) and m.mapping.bias is None
        assert list(m.state_dict()) == ["channel_padding", "mapping.weight"]
    m = C.ChannelPadding(2, 6, is_1d=True, num_classes=3)
    assert isinstance(m.mapping, C.Linear) and tuple(m.mapping.weight.shape) == (2, 8) and m.mapping.bias is None
    with pytest.raises(ValueError, match="`labels` should be provided"):
        m(torch.zeros(1, 2))


def test_entry_declared_cited_and_built():
    assert "cfhip_pixelcnn_sample" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("PixelCNN sampling"):header.index("cfhip_pixelcnn_sample(")]
    for cite in ("pixel_cnn.py:142-165", "pixel_cnn.py:136-140", "pixel_cnn.py:20-65"):
        assert cite in block, cite
    assert ops.PIXELCNN_MAX_CODES >= 1024 and ops.PIXELCNN_MAX_CHANNELS == 256
    import __graft_entry__ as G

    assert "pixelcnn" in G.SOURCES
    script = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert re.search(r"^for f in .*\bpixelcnn\b.*; do$", script, flags=re.M)
    assert os.path.isfile(os.path.join(ROOT, "carefree-learn_amd", "csrc", "pixelcnn.hip"))


def _refused(rc, needle):
    assert rc != 0
    msg = _lib.load().cfhip_last_error().decode()
    assert needle in msg, msg


def test_c_refusals_fire_before_any_launch():
    """no device is touched: the pointers are made-up addresses (16-byte aligned), every call must return before its launch"""
    lib = _lib.load()
    p = 4096

    def call(codes=p, c=32, cin0=1, nl=1, k=8, b=1, h=2, w=2, first=0, last=4):
        return lib.cfhip_pixelcnn_sample(codes, p, p, p, p, p, p, p, p, p, p, 0, b, h, w, c, cin0, nl, k, first, last, 0, 1, 0, None)

    for c in (0, 16, 48, 288):
        _refused(call(c=c), f"latent_channels = {c}")
    _refused(call(k=ops.PIXELCNN_MAX_CODES + 1), f"num_codes = {ops.PIXELCNN_MAX_CODES + 1}")
    _refused(call(k=1), "num_codes = 1")
    _refused(call(nl=0), "num_layers = 0")
    _refused(call(cin0=16), "first layer reads 16 channels")
    _refused(call(b=0), "B = 0")
    _refused(call(first=3, last=2), "pixel range [3, 2)")
    _refused(call(last=5), "pixel range [0, 5)")
    _refused(call(codes=None), "null operand")
    _refused(call(codes=p + 4), "misaligned operand")
    assert call(first=2, last=2) == 0  # an empty range launches nothing


def test_module_refusals_fire_before_any_launch():
    """on a CPU module: each refusal is raised before anything is allocated on, or launched to, a device"""
    m = C.PixelCNN(16, 1, latent_channels=32, num_layers=2)
    with pytest.raises(RuntimeError, match="needs eval mode.*causal"):
        m.sample(2, img_size=4)
    m.eval()
    with pytest.raises(ValueError, match=r"`forced` must be int64 \[2, 1, 4, 4\]"):
        m.sample(2, img_size=4, forced=torch.zeros(2, 1, 4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"`forced` must be int64"):
        m.sample(2, img_size=4, forced=torch.zeros(2, 1, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"outside \[0, 16\)"):
        m.sample(2, img_size=4, forced=torch.full((2, 1, 4, 4), 16, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="latent_channels = 48"):
        C.PixelCNN(16, 1, latent_channels=48, num_layers=2).eval().sample(2, img_size=4)
    with pytest.raises(NotImplementedError, match=f"num_codes = {ops.PIXELCNN_MAX_CODES + 1}"):
        C.PixelCNN(ops.PIXELCNN_MAX_CODES + 1, 1, latent_channels=32, num_layers=1).eval().sample(2, img_size=4)
    m.norm_type = "instance"  # (the constructor refuses norms without a module; the sampler names the one it is asked for)
    with pytest.raises(NotImplementedError, match="norm_type = 'instance'"):
        m.sample(2, img_size=4)
    assert ops.pixelcnn_shape_refusal(256, 1024, 1) is None and ops.pixelcnn_shape_refusal(32, 2, 9) is None
    cond = C.PixelCNN(16, 1, latent_channels=32, num_layers=1, num_classes=3).eval()
    with pytest.raises(ValueError, match="holds 3 entries for 2 samples"):
        cond.sampler_plan(torch.tensor([0, 1, 2]), 2)


def test_pack_layout():
    """fragment (n, kk), lane l, element e = W[16 n + (l & 15)][32 kk + 8 (l >> 4) + e]; zero padding to [16, 32] multiples"""
    w = torch.arange(20 * 40, dtype=torch.float32).view(20, 40) % 251
    pack = ops.pixelcnn_pack(w).float().view(2, 2, 64, 8)
    for n, kk, lane, e in ((0, 0, 0, 0), (0, 1, 17, 3), (1, 0, 63, 7), (1, 1, 5, 1), (1, 1, 35, 0)):
        row, col = 16 * n + (lane & 15), 32 * kk + 8 * (lane >> 4) + e
        want = float(w[row, col]) if row < 20 and col < 40 else 0.0
        assert float(pack[n, kk, lane, e]) == want, (n, kk, lane, e)


@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_conv_replica_against_torch(mask_type):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 5, 9, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 7, 7, generator=g, dtype=torch.float64)
    want = torch.nn.functional.conv2d(x, w * R.mask_of(mask_type), padding=3)
    poisoned = torch.where(R.mask_of(mask_type).bool(), w, torch.full_like(w, float("nan")))
    got, cond = R.masked_conv64(x, poisoned, mask_type)  # the masked taps are never read
    assert torch.allclose(got, want, rtol=0, atol=1e-12) and bool((cond >= got.abs() - 1e-12).all())


@pytest.mark.parametrize("mask_type", ["A", "B"])
def test_conv_replica_is_causal(mask_type):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 2, 6, 8, generator=g, dtype=torch.float64)
    w = torch.randn(3, 2, 7, 7, generator=g, dtype=torch.float64)
    y0, _ = R.masked_conv64(x, w, mask_type)
    x2 = x.clone()
    x2[:, :, 3, 4] += 1.0
    y1, _ = R.masked_conv64(x2, w, mask_type)
    changed = (y0 != y1).any(dim=1)[0].reshape(-1)
    first = 3 * 8 + 4 + (mask_type == "A")  # "B" sees its own pixel, "A" only the ones before it
    assert not changed[:first].any() and changed[first]


def test_draw_replica_hand_case():
    logits = np.log(np.array([[1.0, 2.0, 1.0]]))  # cdf 0.25, 0.75, 1
    for u, pick, margin in ((0.0, 0, 0.25), (0.2, 0, 0.05), (0.25, 1, 0.0), (0.5, 1, 0.25), (0.8, 2, 0.05), (1.0 - 2.0 ** -24, 2, 0.25 - 2.0 ** -24)):
        got, m = R.draw64(logits, np.array([u]))
        assert got[0] == pick and abs(m[0] - margin) < 1e-12, (u, got, m)
    # an all-equal row of a large K: u picks floor(u K)
    got, _ = R.draw64(np.zeros((1, 8)), np.array([0.49]))
    assert got[0] == 3


def test_uniforms_follow_the_flat_stream():
    u = R.uniforms(2, 3, 5, P.SEED, 7)
    words = P.philox4x32_10(P.counters(7, 8), P.SEED).reshape(-1)
    e = (1 * 3 + 2) * 5 + 4
    assert u[1, 2, 4] == float(words[e] >> 8) * 2.0 ** -24 and e // 4 == 7


def test_consumed_counter_range():
    assert C.sample_philox_range(64, 32) == (0, 64 * 32 * 32 // 4)
    assert C.sample_philox_range(3, 3, offset=100) == (100, 100 + 7)  # 27 words: the last counter is used in part
    lo, hi = pixelcnn.sample_philox_range(2, 4, offset=5)
    assert (lo, hi) == (5, 13) and pixelcnn.sample_philox_range(2, 4, offset=hi)[0] == hi  # the next call continues where this ended


def test_seeded_parameters_are_bf16_exact_and_non_trivial(fx):
    rec = fx["configs"][0]
    m = C.PixelCNN(**rec["kwargs"])
    fill_parameters(m, rec["seed"])
    bn = m.net[1][1]
    assert bn.running_mean.abs().max() > 0.1 and 0.5 <= float(bn.running_var.min()) < float(bn.running_var.max()) <= 1.5
    w = m.net[1][0].weight
    assert torch.equal(w.to(torch.bfloat16).float(), w) and 0.01 < float(w.detach().std()) < 0.1


def test_masked_conv_route_table():
    from cflearn_amd import functional as HF

    route = HF.masked_conv_route
    for cin, cout in ((32, 32), (64, 32), (96, 64), (128, 128), (256, 256)):
        assert route(cin, cout, 7, 1, 3, 1) == HF.MASKED
    # the first layer without an embedding, channels outside multiples of 32, and every other geometry: Conv2dFn on the zeroed weight
    for args in ((1, 128, 7, 1, 3, 1), (48, 32, 7, 1, 3, 1), (32, 48, 7, 1, 3, 1), (32, 16, 7, 1, 3, 1), (32, 32, 3, 1, 1, 1),
                 (32, 32, 7, 2, 3, 1), (32, 32, 7, 1, 2, 1), (32, 32, 7, 1, 3, 2), (32, 32, 5, 1, 2, 1)):
        assert route(*args) == HF.UNMASKED, args
    assert route(32, 32, 7, 1, 3, 1, 2) == HF.UNMASKED
    assert ops.MASKED_TAPS == {"A": 24, "B": 25}


def test_masked_conv_entries_declared_cited_and_refusing():
    for name in ("cfhip_conv_masked_pack", "cfhip_conv_masked_bf16", "cfhip_conv_masked_gather"):
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("Masked 7x7 convolution"):header.index("cfhip_conv_masked_pack(")]
    for cite in ("pixel_cnn.py:20-65", "pixel_cnn.py:90-104", "pixel_cnn.py:136-140"):
        assert cite in block, cite
    import __graft_entry__ as G

    assert "conv_masked" in G.SOURCES
    assert re.search(r"^for f in .*\bconv_masked\b.*; do$", open(os.path.join(ROOT, "build_lib.sh")).read(), flags=re.M)
    lib, p = _lib.load(), 4096
    _refused(lib.cfhip_conv_masked_bf16(p, p, None, p, 1, 4, 4, 48, 32, 25, 0, None), "channels 48 -> 32")
    _refused(lib.cfhip_conv_masked_bf16(p, p, None, p, 1, 4, 4, 32, 16, 25, 0, None), "channels 32 -> 16")
    _refused(lib.cfhip_conv_masked_bf16(p, p, None, p, 1, 4, 4, 32, 32, 49, 0, None), "49 live taps")
    _refused(lib.cfhip_conv_masked_bf16(None, p, None, p, 1, 4, 4, 32, 32, 25, 0, None), "null operand")
    _refused(lib.cfhip_conv_masked_bf16(p, p, None, p, 0, 4, 4, 32, 32, 25, 0, None), "B = 0")
    _refused(lib.cfhip_conv_masked_pack(p, p, 32, 1, 24, 0, None), "channels 1 -> 32")
    _refused(lib.cfhip_conv_masked_gather(p, p, 10, 10, 1, 4, 4, 32, 25, None), "rows [10, 20)")
    _refused(lib.cfhip_conv_masked_gather(p, None, 0, 4, 1, 4, 4, 32, 25, None), "null operand")


def test_masked_conv2d_refuses_what_would_reach_the_masked_taps():
    with pytest.raises(NotImplementedError, match="transform_kernel"):
        C.MaskedConv2d("A", 2, 3, kernel_size=7, transform_kernel=True)
    with pytest.raises(NotImplementedError, match="demodulate"):
        C.MaskedConv2d("A", 2, 3, kernel_size=7, demodulate=True)
    with pytest.raises(NotImplementedError, match="`style`"):
        C.MaskedConv2d("A", 2, 3, kernel_size=7, bias=False)._effective_weight(torch.ones(1, 2))
