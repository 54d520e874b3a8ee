"""mix_ff without a device: the registry, the state dict against the reference's MixFeedForward, the restated formula against the
reference module, the refusals of the module path and of the C entries of csrc/conv_dw_rows.hip."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import cflearn_amd as C  # noqa: F401
from cflearn_amd import _lib, functional as HF, modules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_mixer():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refharness

    if not refharness.reference_available():
        pytest.skip("the reference tree is not available")
    refharness.load_reference()
    return __import__("importlib").import_module("cflearn.modules.core.mixed_stacks.channel_mixers").MixFeedForward(32, 64, 0.0)


def test_builds_through_the_registry_and_the_binding():
    mixer = M.channel_mixers.build("mix_ff", config=dict(in_dim=32, latent_dim=64, dropout=0.0, layer_idx=0, num_layers=1))
    assert isinstance(mixer, M.MixFeedForward) and mixer.need_2d
    blk = M.MixingBlock(0, 1, 30, 32, 64, token_mixing_type="attention", channel_mixing_type="mix_ff", norm_type="layer")
    assert isinstance(blk.channel_mixing, M.MixFeedForward) and not blk._fusable()
    conv = mixer.net[2].net  # the reference's initial values: Conv2d's constructor as DepthWiseConv2d uses it
    assert tuple(conv.weight.shape) == (64, 1, 3, 3) and float(conv.bias.detach().abs().max()) == 0.0 and float(conv.weight.detach().std()) > 0.0
    assert {"cfhip_dwconv3x3_rows_fwd", "cfhip_dwconv3x3_rows_bwd", "cfhip_dwconv3x3_rows_bwd_workspace"} <= set(_lib.SIGNATURES)
    with open(os.path.join(ROOT, "README.md")) as f:
        assert f"{len(_lib.SIGNATURES)} entry points" in f.read()


def test_state_dict_and_restated_formula_are_the_references():
    """names, shapes and a strict load; and what tests/test_gpu_mixff.py compares the HIP path with (F.linear, F.conv2d(groups=L),
    F.gelu) equals the reference's module to 1e-6 in fp32"""
    ref = _reference_mixer().eval()
    ours, p = M.MixFeedForward(32, 64, 0.0), ref.state_dict()
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in p.items()}
    assert list(p) == ["net.0.linear.weight", "net.0.linear.bias", "net.2.net.weight", "net.2.net.bias", "net.6.linear.weight",
                       "net.6.linear.bias"] and tuple(p["net.2.net.weight"].shape) == (64, 1, 3, 3)
    ours.load_state_dict(p, strict=True)
    torch.manual_seed(3)
    x = torch.randn(2, 6, 5, 32)
    t = F.linear(x, p["net.0.linear.weight"], p["net.0.linear.bias"]).permute(0, 3, 1, 2)
    t = F.conv2d(t, p["net.2.net.weight"], p["net.2.net.bias"], padding=1, groups=64).flatten(2).transpose(1, 2)
    want = F.linear(F.gelu(t), p["net.6.linear.weight"], p["net.6.linear.bias"])
    with torch.no_grad():
        assert float((ref(x) - want).abs().max()) <= 1e-6


def test_module_path_refusals():
    with pytest.raises(NotImplementedError, match="latent_dim = 60"):
        M.MixFeedForward(32, 60, 0.0)
    x = torch.zeros(2, 30, 32)
    for position in ("pre_norm", "post_norm"):
        blk = M.MixingBlock(0, 1, 30, 32, 64, token_mixing_type="attention", channel_mixing_type="mix_ff", norm_type="layer", norm_position=position)
        with pytest.raises(ValueError, match="`hw` should be provided when FFN needs 2d input"):
            blk(x)
        with pytest.raises(ValueError, match="does not cover the 30 tokens"):
            blk(x, (4, 7))
    with pytest.raises(ValueError, match="rows with `hw`"):
        blk.channel_mixing(x)
    with pytest.raises(ValueError, match="does not cover"):
        blk.channel_mixing(x, hw=(4, 7))
    w, bias, rows = torch.zeros(64, 1, 3, 3), torch.zeros(64), torch.zeros(2, 30, 64)
    for args, name in (((rows, w, bias, 2, 1, 1, 64), "stride = 2"), ((rows, w, bias, 1, 0, 1, 64), "padding = 0"),
                       ((rows, w, bias, 1, 1, 2, 64), "dilation = 2"), ((rows, w, bias, 1, 1, 1, 32), "groups = 32"),
                       ((rows, torch.zeros(64, 1, 5, 5), bias, 1, 1, 1, 64), "kernel size"),
                       ((torch.zeros(2, 30, 60), torch.zeros(60, 1, 3, 3), None, 1, 1, 1, 60), "C % 8 = 4")):
        with pytest.raises(NotImplementedError, match=name):
            HF.GroupedConv2dFn.apply(*args, (6, 5))


def test_c_entries_refuse_before_any_launch():
    """made-up pointers: every refusal (code -1 and its message) comes before a launch could touch them"""
    lib = _lib.load()
    X, W, Y, DY, WS = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
    fwd = lambda x=X, ldx=64, y=Y, ldy=64, c=64, b=2, wp=W: lib.cfhip_dwconv3x3_rows_fwd(x, ldx, wp, None, y, ldy, b, 6, 5, c, 1, None)
    bwd = lambda dx=Y, lddx=64, dw=W + 4096, ws=WS, nb=1 << 20, c=64: lib.cfhip_dwconv3x3_rows_bwd(
        DY, 64, X, 64, W, None, dx, lddx, dw, 0, None, 0, 2, 6, 5, c, 1, ws, nb, None)
    for call, needle in ((lambda: fwd(c=60, ldx=60, ldy=60), "C = 60 is not a multiple of 8"), (lambda: fwd(ldx=56), "ld_x = 56"),
                         (lambda: fwd(ldy=68), "ld_y = 68"), (lambda: fwd(x=X + 8), "x is not 16-byte aligned"),
                         (lambda: fwd(wp=W + 4), "16-byte aligned"), (lambda: fwd(y=X + 64), "y overlaps x"),
                         (lambda: fwd(b=1 << 27), "31-bit row index"), (lambda: bwd(c=12), "C = 12 is not a multiple of 8"),
                         (lambda: bwd(lddx=32), "ld_dx = 32"), (lambda: bwd(dx=DY + 128), "dx overlaps x or dy"),
                         (lambda: bwd(dx=Y + 2), "dx is not 16-byte aligned"), (lambda: bwd(nb=64), "workspace of"),
                         (lambda: bwd(dw=X + 256), "overlaps a rows operand"), (lambda: bwd(ws=DY), "overlaps a rows operand"),
                         (lambda: bwd(dx=None, dw=None), "no output asked for")):
        assert call() == -1, needle
        assert needle in lib.cfhip_last_error().decode(), needle
    assert lib.cfhip_dwconv3x3_rows_bwd_workspace(2, 6, 5, 64) > 0 and lib.cfhip_dwconv3x3_rows_bwd_workspace(2, 6, 5, 60) == 0
