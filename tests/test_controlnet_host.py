"""ControlNet, host side: state-dict layout against the reference's (recorded in tests/golden/controlnet_small.pt), initialisation,
`load_encoder_from`, which convolutions the direct kernel takes, the refusals, the C-ABI entries.  No GPU."""
import os

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib
from cflearn_amd import functional as HF
from cflearn_amd.diffusion import ControlNetTrainStep, make_sampler
from cflearn_amd.modules import UNetDiffuser

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controlnet_small.pt")
# (Cin, Cout, stride) of the hint block's eight convolutions at hint_channels 3, start_channels 320 (unet.py:441-457)
HINT_LAYERS = [(3, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2), (256, 320, 1)]


@pytest.fixture(scope="module")
def fixture():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def _layout(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def test_state_dict_layout_is_the_reference_s(fixture):
    g = fixture
    assert _layout(C.ControlNet(**g["cfg"])) == g["control_keys"]
    assert _layout(UNetDiffuser(**g["unet_cfg"])) == g["unet_keys"]  # (the constructors share their helpers)
    with torch.device("meta"):
        zoo = C.ControlNet(**g["zoo_cfg"])
    assert _layout(zoo) == g["zoo_keys"]
    assert len(zoo.zero_convs) == 12 and zoo.num_control_scales == 13
    keys = [k for k, _ in g["zoo_keys"]]
    assert keys[0] == "time_embed.0.weight" and "middle_block_out.0.bias" == keys[-1]
    assert {k.split(".")[1] for k in keys if k.startswith("input_hint_block.")} == {"0", "2", "4", "6", "8", "10", "12", "14"}


def test_zero_initialisation(fixture):
    cn = C.ControlNet(**fixture["cfg"])
    zeros = [m for seq in list(cn.zero_convs) + [cn.middle_block_out] for m in seq] + [cn.input_hint_block[14]]
    assert len(zeros) == len(cn.input_blocks) + 2
    for m in zeros:
        assert not m.weight.any() and not m.bias.any()
    assert cn.input_hint_block[12].weight.any()
    zoo_like = C.ControlNet(4, 3, num_heads=2, start_channels=32, num_res_blocks=2, channel_multipliers=(1, 2, 4, 8))
    assert len(zoo_like.zero_convs) + 1 == 13  # the 13 zero convolutions of the zoo layout
    assert all(not p.any() for seq in list(zoo_like.zero_convs) + [zoo_like.middle_block_out] for p in seq.parameters())


def test_load_encoder_from(fixture):
    g = fixture
    torch.manual_seed(1)
    unet, cn = UNetDiffuser(**g["unet_cfg"]), C.ControlNet(**g["cfg"])
    hint_before = cn.input_hint_block[0].weight.detach().clone()
    cn.load_encoder_from(unet)
    own = cn.state_dict()
    copied = 0
    for k, v in unet.state_dict().items():
        for src, dst in (("time_embedding.", "time_embed."), ("input_blocks.", "input_blocks."), ("residual.", "middle_block.")):
            if k.startswith(src):
                assert torch.equal(own[dst + k[len(src):]], v), k
                copied += 1
    assert copied == sum(1 for k in own if k.startswith(("time_embed.", "input_blocks.", "middle_block.")))
    assert torch.equal(cn.input_hint_block[0].weight, hint_before)
    wider = UNetDiffuser(**{**g["unet_cfg"], "context_dim": 24})
    with pytest.raises(ValueError, match="attn2.to_k|to_k"):
        cn.load_encoder_from(wider)
    first = next(k for k, v in wider.state_dict().items() if v.shape != unet.state_dict()[k].shape)
    with pytest.raises(ValueError, match=first.replace(".", r"\.")):
        cn.load_encoder_from(wider)


def test_which_convolutions_the_direct_kernel_takes(fixture):
    assert [HF.direct_conv_ok(cin, cout, 3, s, 1, 1) for cin, cout, s in HINT_LAYERS] == [True] * 5 + [False] * 3
    for bad in ((16, 16, 1, 1, 0, 1), (16, 16, 3, 1, 0, 1), (16, 16, 3, 1, 1, 2), (16, 16, 3, 3, 1, 1), (16, 24, 3, 1, 1, 1),
                (16, 112, 3, 1, 1, 1), (33, 32, 3, 1, 1, 1)):
        assert not HF.direct_conv_ok(*bad), bad
    # nothing of the UNet's own qualifies
    with torch.device("meta"):
        unet = UNetDiffuser(4, 4, num_heads=8, use_spatial_transformer=True, context_dim=768)
    convs = [m for m in unet.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) > 60
    assert not any(HF.direct_conv_ok(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0]) for m in convs)
    # and conv_route answers what it answered before this module existed, at the hint block's geometries (512^2 hint)
    sides = [512, 512, 512, 256, 256, 128, 128, 64]
    want = [("im2row", 16), ("im2row", 16), ("im2row", 32), ("implicit", 32), ("im2row", 96), ("implicit", 96), ("im2row", 256), ("implicit", 320)]
    assert [HF.conv_route(cin, cout, 3, 3, s, 1, 1, hw, hw) for (cin, cout, s), hw in zip(HINT_LAYERS, sides)] == want
    cn = C.ControlNet(**fixture["cfg"])
    packable = {id(m) for m in cn._packable_convs()}
    assert id(cn.input_hint_block[6]) not in packable and id(cn.input_hint_block[10]) in packable and id(cn.input_hint_block[14]) in packable


def test_refusals(fixture):
    g = fixture
    for cls, args in ((C.ControlNet, (4, 3)), (UNetDiffuser, (4, 4))):
        with pytest.raises(NotImplementedError):
            cls(*args, num_heads=2, start_channels=32, signal_dim=3)
        with pytest.raises(NotImplementedError):
            cls(*args, num_heads=2, start_channels=32, hooks_kwargs={"a": 1})
    unet, cn = UNetDiffuser(**g["unet_cfg"]), C.ControlNet(**g["cfg"])
    with pytest.raises(ValueError):
        cn(g["x_t"], g["hint"], timesteps=g["timesteps"], context=g["context"], scales=[1.0])
    with pytest.raises(ValueError):
        cn(g["x_t"], g["hint"][:, :2], timesteps=g["timesteps"], context=g["context"])
    with pytest.raises(ValueError):
        cn(g["x_t"], g["hint"], timesteps=g["timesteps"], context=g["context"], labels=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        ControlNetTrainStep(unet, cn, use_graph=True)
    with pytest.raises(ValueError):
        ControlNetTrainStep(unet, cn, control_scales=[1.0, 2.0])
    z = torch.zeros(2, 4, 8, 8)
    for kind in ("ddim", "basic", "k_euler_a", "k_heun", "k_dpmpp_2m"):
        with pytest.raises(ValueError):
            make_sampler(kind, unet).sample(z, hint=g["hint"])
        s = make_sampler(kind, unet, control_model=cn)
        assert s.control_model is cn and s.control_scales is None and s.only_mid_control is False
        with pytest.raises(ValueError):
            s.sample(z)  # a control model wants its hint
        with pytest.raises(ValueError):
            s.sample(z, hint=g["hint"][:, :, :32])
        with pytest.raises(NotImplementedError):
            s.sample(z, hint=g["hint"], control=[z])
        with pytest.raises(NotImplementedError):
            make_sampler(kind, unet, control_model={"canny": cn})
        with pytest.raises(ValueError):
            make_sampler(kind, unet, control_model=cn, control_scales=[1.0])
        with pytest.raises(ValueError):
            make_sampler(kind, unet, control_scales=[1.0] * 5)


def test_frozen_unet_and_arena_cover(fixture):
    g = fixture
    unet, cn = UNetDiffuser(**g["unet_cfg"]), C.ControlNet(**g["cfg"])
    ts = ControlNetTrainStep(unet, cn, step_in_backward=False)
    assert all(not p.requires_grad for p in unet.parameters())
    assert {id(p) for p in ts.arena.params} == {id(p) for p in cn.parameters()}
    assert ts.unet is unet and ts.control_net is cn and not ts.use_graph


def test_entry_points_are_declared():
    for name, n in (("cfhip_conv3x3_direct_pack", 6), ("cfhip_conv3x3_direct_bf16", 12), ("cfhip_silu_bf16_fwd", 4),
                    ("cfhip_silu_bf16_bwd", 5), ("cfhip_scale_bf16", 5)):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    import __graft_entry__ as entry

    assert "conv_direct" in entry.SOURCES
    assert " conv_direct" in open(os.path.join(os.path.dirname(entry.__file__), "build_lib.sh")).read()
