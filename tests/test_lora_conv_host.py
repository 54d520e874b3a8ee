"""Convolution LoRA adapters, host side (no GPU): the C-ABI entries, LoRAConvHook's constructor contract, LoRAManager with both
hook kinds, and a float64 self-check of tests/golden/lora_conv.pt (the reference's fp32 numbers, tools/gen_lora_conv_golden.py)."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import cflearn_amd as C
from cflearn_amd import _lib, modules as M
from helpers import rel_l2


def _dec(rec, g):
    sc = g["scales"]
    f = lambda q, s: q.double() * s  # noqa: E731
    return dict(w=f(rec["wq"], sc["w"]), b=f(rec["bq"], sc["w"]), a=f(rec["aq"], sc["a"]), bm=f(rec["bmq"], sc["a"]),
                x=f(rec["xq"], sc["x"]), gy=f(rec["gyq"], sc["x"]))


def test_entry_points_are_declared():
    want = {"cfhip_lora_conv_down": 12, "cfhip_lora_conv_dx": 12, "cfhip_lora_conv_wgrad_workspace": 6, "cfhip_lora_conv_wgrad": 15}
    for name, n in want.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n, (name, len(_lib.SIGNATURES[name][1]))
    assert _lib.SIGNATURES["cfhip_lora_conv_wgrad_workspace"][0] is _lib.c_size_t


def test_hook_shapes_signature_and_init(golden):
    keys = golden("lora_conv.pt")["keys"]
    torch.manual_seed(0)
    hook = C.LoRAConvHook(32, 40, 3, 1, 1, rank=4)
    assert {n: tuple(p.shape) for n, p in hook.named_parameters()} == keys["param_shapes"]
    sig = inspect.signature(C.LoRAConvHook.__init__)
    got = [(n, None if p.default is inspect.Parameter.empty else p.default, str(p.kind)) for n, p in sig.parameters.items() if n != "self"]
    assert got == keys["ctor"]
    init = keys["init"]
    assert float(hook.lora_up.weight.abs().max()) == init["up_abs_max"] == 0.0
    assert abs(float(hook.lora_down.weight.std()) * 4 - 1.0) < 0.1 and abs(init["down_std_times_rank"] - 1.0) < 0.1
    assert float(hook.alpha) == pytest.approx(init["alpha"]) and hook.dropout.p == init["dropout"]
    assert not hook.alpha.requires_grad and hook.full_scale == pytest.approx(1.0 * init["alpha"] / 4)


@pytest.mark.parametrize("args,kwargs", [
    ((8, 8, 3), {}),                       # 3x3 with padding 0
    ((8, 8, 3, 1, 1, 1, 2), {}),           # groups 2
    ((8, 8, 3, 1, 1, 2), {}),              # dilation 2
    ((3, 8, 3, 1, 1), {"rank": 2}),        # Cin = 3
    ((72, 72, 3, 1, 1), {"rank": 65}),     # rank 65
    ((8, 8, 1, 2, 0), {}),                 # strided 1x1
    ((8, 8, 5, 1, 2), {}),                 # 5x5
])
def test_out_of_scope_geometries_raise(args, kwargs):
    with pytest.raises(NotImplementedError):
        C.LoRAConvHook(*args, **kwargs)


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = M.HijackConv2d(8, 16, 3, 1, 1)
        self.head = C.HijackLinear(16, 8)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.block = _Block()
        self.stem = M.HijackConv2d(3, 8, 3, padding=1)  # 3 input channels: no adapter kernels


def test_manager_prepares_both_hook_kinds(golden):
    keys = golden("lora_conv.pt")["keys"]
    tiny = _Tiny()
    before = {k: v.clone() for k, v in tiny.state_dict().items()}
    mgr = C.LoRAManager()
    mgr.prepare(tiny, key="a", rank=2, target_ancestors={"_Block"})
    pack = mgr.lora_packs["a"]
    assert sorted(pack.hooks) == keys["hooks"]
    assert {k: type(v).__name__ for k, v in pack.hooks.items()} == keys["hook_classes"]
    mgr.inject(tiny, "a")
    assert isinstance(tiny.block.conv.hook, C.LoRAConvHook) and isinstance(tiny.block.head.hook, C.LoRALinearHook)
    assert [k for k in tiny.state_dict() if k.startswith("block.")] == keys["state_dict"]
    assert mgr.build_pack("a") is pack
    mgr.set_scale("a", 0.5)
    assert tiny.block.conv.hook.scale == 0.5
    mgr.cleanup(tiny)
    assert tiny.block.conv.hook is None and tiny.block.head.hook is None
    after = tiny.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # without target ancestors the whole tree is walked: the 3-channel stem is reported, not adapted
    mgr.prepare(tiny, key="b", rank=2)
    assert sorted(mgr.lora_packs["b"].hooks) == ["block.conv", "block.head"] and mgr.skipped == ["stem"]


def test_fixture_self_check_in_float64(golden):
    """the exactly merged filter reproduces the reference's training output and gradients; the reference's own eval-mode formula for
    3x3 (tap [0, 0] broadcast over the nine taps, hijacks.py:143) is far outside the 1e-2 GPU tolerance"""
    g = golden("lora_conv.pt")
    assert [tuple(r["case"]) for r in g["layers"]] == [(8, 16, 1, 1, 0, 4, 5, 7), (32, 40, 3, 1, 1, 4, 5, 7), (32, 64, 3, 2, 1, 17, 6, 9),
                                                        (64, 32, 3, 1, 1, 16, 8, 8)]
    for rec in g["layers"]:
        cin, cout, k, stride, pad, rank, h, w = rec["case"]
        d = _dec(rec, g)
        s = g["alpha"] / rank
        up = d["bm"][:, :, 0, 0]
        a = d["a"].clone().requires_grad_(True)
        upp = up.clone().requires_grad_(True)
        wgt = d["w"].clone().requires_grad_(True)
        b = d["b"].clone().requires_grad_(True)
        x = d["x"].clone().requires_grad_(True)
        merged = wgt + s * torch.einsum("oc,cikl->oikl", upp, a)
        y = F.conv2d(x, merged, b, stride, pad)
        y.backward(d["gy"])
        tag = str(tuple(rec["case"]))
        assert rel_l2(y.detach(), rec["y"].double()) < 1e-5, tag
        assert rel_l2(x.grad, rec["gx"].double()) < 1e-5, tag
        assert rel_l2(a.grad, rec["ga"].double()) < 1e-5, tag
        assert rel_l2(upp.grad, rec["gbm"].double()[:, :, 0, 0]) < 1e-5, tag
        assert rel_l2(wgt.grad[::rec["row_step"]], rec["gw_rows"].double()) < 1e-5, tag
        assert rel_l2(b.grad, rec["gb"].double()) < 1e-5, tag
        assert rec["merged_rel"] < 1e-5
        with torch.no_grad():
            if k == 1:
                assert rel_l2(merged.detach(), rec["w_injected"].double()) < 1e-6, tag
                assert rel_l2(rec["y_eval"].double(), rec["y"].double()) < 1e-5, tag
            else:
                bcast = d["w"] + s * (up @ d["a"][:, :, 0, 0])[..., None, None]
                far = rel_l2(F.conv2d(d["x"], bcast, d["b"], stride, pad), rec["y"].double())
                assert far == pytest.approx(rec["eval_ref_rel"], rel=1e-3) and far > 4e-2, (tag, far)
