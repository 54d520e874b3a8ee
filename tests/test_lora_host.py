"""LoRA adapters, host side (no GPU): names, shapes, inits and the manager's life cycle against what the reference's own classes
gave (tests/golden/lora_linear.pt, tools/gen_lora_golden.py), the out-of-scope cases, the C-ABI entries."""
import inspect

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, modules as M


class Tiny(torch.nn.Module):
    """the generator's tiny model, on this package's classes"""

    def __init__(self) -> None:
        super().__init__()
        self.ff = C.FeedForward(16, 32, 0.0, "GELU")
        self.head = C.HijackLinear(16, 8)


def test_constructor_names_shapes_inits(golden):
    keys = golden("lora_linear.pt")["keys"]
    sig = inspect.signature(C.LoRALinearHook.__init__)
    got = [(n, None if p.default is inspect.Parameter.empty else p.default, str(p.kind)) for n, p in sig.parameters.items() if n != "self"]
    assert got == keys["ctor"]
    torch.manual_seed(3)
    hook = C.LoRALinearHook(64, 48, rank=8)
    assert {n: tuple(p.shape) for n, p in hook.named_parameters()} == keys["param_shapes"]
    assert list(hook.state_dict()) == ["alpha", "lora_down.weight", "lora_up.weight"]
    # normal_(std = 1 / rank) on 512 values: the sample std is within 15 % (4.8 sigma of its own spread); zeros; alpha; dropout
    assert abs(float(hook.lora_down.weight.std()) * 8 - 1.0) < 0.15 and abs(keys["init"]["down_std_times_rank"] - 1.0) < 0.15
    assert float(hook.lora_up.weight.abs().max()) == keys["init"]["up_abs_max"] == 0.0
    assert float(hook.alpha) == pytest.approx(keys["init"]["alpha"]) and hook.dropout.p == keys["init"]["dropout"] == 0.1
    assert not hook.alpha.requires_grad  # no gradient in the reference either (`alpha.item()`): kept out of arenas and optimizers
    with pytest.raises(ValueError) as e:
        C.LoRALinearHook(8, 8, rank=9)
    assert str(e.value) == keys["rank_error"]


def test_alpha_is_read_on_the_host_once():
    hook = C.LoRALinearHook(16, 16, rank=4, scale=0.5)
    assert hook.full_scale == pytest.approx(0.5 / 4)
    hook.set_scale(2.0)
    assert hook.full_scale == pytest.approx(2.0 * 0.5 / 4)
    sd = hook.state_dict()
    sd["alpha"] = torch.tensor(0.25)
    hook.load_state_dict(sd)
    assert hook.full_scale == pytest.approx(2.0 * 0.25 / 4)
    with torch.no_grad():
        hook.alpha.fill_(1.0)
    assert hook.full_scale == pytest.approx(2.0 * 0.25 / 4)  # cached: no device read per forward
    hook.refresh_alpha()
    assert hook.full_scale == pytest.approx(2.0 / 4)


def test_manager_life_cycle_and_keys(golden):
    keys = golden("lora_linear.pt")["keys"]
    tiny = Tiny()
    before = list(tiny.state_dict())
    mgr = C.LoRAManager()
    with pytest.raises(ValueError):
        mgr.inject(tiny, "a")
    mgr.prepare(tiny, key="a", rank=2, target_ancestors={"FeedForward"})
    assert mgr.has("a") and not mgr.injected
    pack = mgr.lora_packs["a"]
    assert isinstance(pack, C.LoRAPack) and pack.rank == 2 and sorted(pack.hooks) == keys["hooks"]
    assert list(tiny.state_dict()) == before  # prepared, not attached
    with pytest.raises(ValueError):
        mgr.cleanup(tiny)
    with pytest.raises(ValueError):
        mgr.inject(Tiny(), "a")
    mgr.inject(tiny, "a")
    assert mgr.injected and list(tiny.state_dict()) == keys["state_dict"]
    assert all(tiny.get_submodule(k).hook is pack.hooks[k] for k in pack.hooks) and tiny.head.hook is None
    mgr.set_scales({"a": 0.5})
    assert all(h.scale == 0.5 and not h.injected for h in pack.hooks.values())
    tiny.eval()
    assert all(not h.training for h in pack.hooks.values())
    mgr.cleanup(tiny)
    assert not mgr.injected and list(tiny.state_dict()) == before
    assert all(tiny.get_submodule(k).hook is None for k in pack.hooks)
    # the whole model without ancestors: the keys are the names `inject` looks up
    mgr.prepare(tiny, key="b", rank=2)
    assert sorted(mgr.lora_packs["b"].hooks) == sorted(keys["hooks"] + ["head"])
    mgr.inject(tiny, "b")
    assert isinstance(tiny.head.hook, C.LoRALinearHook)


def test_out_of_scope_cases_raise():
    with pytest.raises(NotImplementedError):
        M.LoRAConvHook(8, 8, 3)
    with pytest.raises(NotImplementedError):
        M.LoRAAttentionHook(8, 8, rank=2)
    with pytest.raises(NotImplementedError):
        C.LoRALinearHook.create_with(C.HijackCustomLinear(16, 16, rank=4), 2)
    with pytest.raises(NotImplementedError):
        C.LoRALinearHook.create_with(C.HijackCustomLinear(16, 16, rank_ratio=0.5), 2)
    with pytest.raises(NotImplementedError):
        C.LoRALinearHook.create_with(C.HijackCustomLinear(16, 16, pruner_config={}), 2)
    with pytest.raises(NotImplementedError):
        C.LoRALinearHook(128, 128, rank=65)
    hook = C.LoRALinearHook(16, 16, rank=2)
    with pytest.raises(RuntimeError):
        hook.after_forward(torch.zeros(1, 16), torch.zeros(1, 16))  # training mode has one path: linear_forward
    mgr = C.LoRAManager()
    mgr.prepare(Tiny(), key="a", rank=2)
    mgr.lora_packs["b"] = mgr.lora_packs["a"]
    with pytest.raises(NotImplementedError):
        mgr.build_pack("a", "b")


def test_entry_points_come_from_the_header():
    for name, nargs in (("cfhip_lora_down", 14), ("cfhip_lora_up_add", 15), ("cfhip_lora_wgrad_workspace", 3), ("cfhip_lora_wgrad", 16)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.host_query("cfhip_lora_wgrad_workspace") and not _lib.ctypes_only("cfhip_lora_up_add")


def test_wrong_activation_order_is_far_outside_the_tolerance(golden):
    """The FeedForward record must tell the two orders apart: with the fixture's numbers, in fp32 on the CPU, the low-rank term added
    after the GELU lands 0.42 away (rel-L2) from the reference's output — 40 x the 1e-2 the GPU test allows — while the order the
    package implements reproduces it."""
    g = golden("lora_linear.pt")
    ff, sc, alpha = g["ff"], g["scales"], g["alpha"]
    rank = ff["shape"][2]
    s = 2 * alpha / rank  # HijackCustomLinear: the reference runs the hook twice (tools/gen_lora_golden.py)
    x = ff["xq"].float() * sc["x"]
    p = {k: {n: v.float() * (sc["a"] if n in ("aq", "bmq") else sc["w"]) for n, v in ff[k].items()} for k in ("net0", "net3")}

    def layer(t, q, act_first):
        base = t @ q["wq"].t() + q["bq"]
        low = s * (t @ q["aq"].t() @ q["bmq"].t())
        return torch.nn.functional.gelu(base) + low if act_first else base + low

    right = layer(torch.nn.functional.gelu(layer(x, p["net0"], False)), p["net3"], False)
    wrong = layer(layer(x, p["net0"], True), p["net3"], False)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    assert rel(right, ff["y"]) < 1e-5
    assert rel(wrong, ff["y"]) > 0.1 and abs(rel(wrong, ff["y"]) - ff["wrong_order_rel"]) < 1e-4
