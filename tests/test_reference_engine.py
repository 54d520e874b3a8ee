"""This package and the oracle restatements against what the reference's OWN code computed on CPU, frozen in
tests/golden/reference_engine.pt by oracle/gen_reference_engine.py (the inputs and initial weights are stored with
every result, so nothing here needs the reference tree):

  * the drop-in boundary: INTEGRATION.md §2's registry override executed on a registry with the reference's names,
    building the FCNN the way the reference's `build_module` does (modules/common.py:37-53: `safe_execute`);
  * the pin of `oracle/trainer_oracle.py` (the step-engine restatement the GPU tests drive the HIP modules with)
    against the reference's `IDLModel.train` / `get_update_fn` / `Trainer.clip_norm_step` (schema.py:977-986,
    1174-1294; trainer.py:170-176): the same losses and weights on the same model and batches;
  * gradient checkpointing (`toolkit.py:2535-2647`) around modules of this package (row U6);
  * `Pruner` and the `Conv2d` options against the reference modules.

The fixture was made on one CPU.  PyTorch's CPU math (exp / log / reductions) can differ in the last bit between CPU
models and instruction sets, so values computed here are compared to within a few float32 ulps of the largest
stored value (`_assert_ulps`).  The largest difference measured across two CPU models and PyTorch's CPU instruction
set levels was 1.6e-7 of the largest value.  A logic difference shows up many orders of magnitude above that.

Every test here is `not gpu`.
"""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import trainer_oracle as TO  # noqa: E402


def _assert_ulps(a, b, what: str = "", ulps: int = 8) -> None:
    """|a - b| <= `ulps` float32 ulps of max|b|, elementwise (see the module docstring)"""
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bound = ulps * 2.0 ** -23 * b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= bound, f"{what}: max|diff| {err:.3e} > {bound:.3e} ({ulps} ulps of max|ref|)"


@pytest.fixture(scope="module")
def frozen():
    return torch.load(os.path.join(ROOT, "tests", "golden", "reference_engine.pt"), map_location="cpu", weights_only=False)


def test_registry_override_on_the_reference_module_dict(frozen):
    """INTEGRATION.md §2 on a registry that holds the reference's names: after the override, building by name the way
    the reference's `build_module` does (`safe_execute(module_dict[name], config)`, the only way its models create
    modules) hands out this package's classes, which keep the reference's constructor keywords and
    state_dict keys (the reference's FCNN state_dict is stored)."""
    import cflearn_amd as C
    from cflearn_amd.registry import module_dict as ours_dict
    from cflearn_amd.registry import safe_execute

    ref = frozen["registry"]
    module_dict = {name: None for name in ref["names"]}  # the reference's registry, values left out
    n = C.override_reference_registry(module_dict)
    assert n >= 5
    assert set(module_dict) == set(ref["names"]) | set(ours_dict)
    cfg = dict(input_dim=10, output_dim=3, hidden_units=[16, 16])
    ours = safe_execute(module_dict["fcnn"], dict(cfg, some_unknown_keyword=1))  # safe_execute drops extras
    assert type(ours).__module__.startswith("cflearn_amd")
    assert list(ours.state_dict().keys()) == list(ref["fcnn_sd"].keys())
    ours.load_state_dict(ref["fcnn_sd"])  # checkpoints move both ways
    for k, v in ours.state_dict().items():
        assert torch.equal(v, ref["fcnn_sd"][k]), k
    clf = safe_execute(module_dict["cv_clf"], dict(in_channels=1, num_classes=10, img_size=28, latent_dim=64,
                                                   encoder="vanilla_1d", encoder_config=dict(num_downsample=3)))
    assert type(clf).__module__.startswith("cflearn_amd")


def _mlp() -> torch.nn.Module:
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))


def _batches(n: int):
    g = torch.Generator().manual_seed(7)
    return [{TO.INPUT_KEY: torch.randn(8, 12, generator=g), TO.LABEL_KEY: torch.randint(0, 4, (8, 1), generator=g)}
            for _ in range(n)]


@pytest.mark.parametrize("loss_name,grad_accumulate,clip_norm", [("focal", 1, 0.0), ("cross_entropy", 2, 0.05),
                                                                  ("focal", 3, 0.1)])
def test_step_engine_oracle_matches_the_reference(frozen, loss_name, grad_accumulate, clip_norm):
    """`oracle/trainer_oracle.StepEngine` against the reference's `CommonDLModel.train` driven by a trainer object
    that carries the reference's own `Trainer.clip_norm_step`: the same losses (the `.item()` values) and weights after
    6 batches, with gradient accumulation and clipping (bit-equal on the CPU that made the fixture)."""
    ref = frozen["step_engine"][(loss_name, grad_accumulate, clip_norm)]
    mine = _mlp()
    eng = TO.StepEngine(mine, loss_name, torch.optim.SGD(mine.parameters(), lr=0.1), grad_accumulate=grad_accumulate,
                        clip_norm=clip_norm)
    eng.fit(_batches(6))
    _assert_ulps([d[TO.LOSS_KEY] for d in eng.loss_log], ref["losses"], "losses")
    assert len(list(mine.parameters())) == len(ref["params"])
    for i, (a, b) in enumerate(zip(mine.parameters(), ref["params"])):
        _assert_ulps(a, b, f"parameter {i}")
    for a, b in zip(mine.parameters(), _mlp().parameters()):
        assert not torch.equal(a, b)  # and training did move them


def test_reference_gradient_checkpoint_reenters_custom_functions(frozen):
    """Row U6: `gradient_checkpoint` (the reference's toolkit.py:2535-2647; this package's `functional.gradient_checkpoint`
    keeps its signature and semantics) re-runs the wrapped forward inside backward under `torch.autograd.grad` — a
    second, re-entrant trip through every custom autograd Function in it.  The parameter-gradient protocol of this
    package's Functions (write straight into `.grad`, return None, run the gradient-ready callbacks) must survive that:
    exercised here with the CPU stand-in that follows the same protocol (tests/test_ddp_gloo._DirectLinear), against the
    gradients the reference's checkpoint produced around a plain Linear on the same weights and input; the HIP
    Functions themselves are covered on the GPU by tests/test_gpu_unet.py::test_gradient_checkpoint_matches_plain_backward."""
    from test_ddp_gloo import _DirectLinear

    from cflearn_amd.functional import gradient_checkpoint

    ref = frozen["gradient_checkpoint"]
    lin = torch.nn.Linear(6, 6)
    lin.load_state_dict(ref["sd"])
    for p in lin.parameters():
        p.grad = torch.zeros_like(p)
    x = ref["x"].clone().requires_grad_(True)

    def block(inp):
        return torch.tanh(_DirectLinear.apply(inp, lin.weight, lin.bias))

    y = gradient_checkpoint(block, (x,), tuple(lin.parameters()), True)
    y.sum().backward()
    gw, gb, gx = lin.weight.grad.clone(), lin.bias.grad.clone(), x.grad.clone()
    assert torch.allclose(gx, ref["gx"], atol=1e-6)
    assert torch.allclose(gw, ref["gw"], atol=1e-6) and torch.allclose(gb, ref["gb"], atol=1e-6)
    # plain autograd on the same math
    lin2 = torch.nn.Linear(6, 6)
    lin2.load_state_dict(ref["sd"])
    x2 = ref["x"].clone().requires_grad_(True)
    torch.tanh(lin2(x2)).sum().backward()
    assert torch.allclose(gx, x2.grad, atol=1e-6)
    assert torch.allclose(gw, lin2.weight.grad, atol=1e-6) and torch.allclose(gb, lin2.bias.grad, atol=1e-6)


def test_lazy_loss_patch_on_a_stand_in_train_step(monkeypatch):
    """(f)3 for cflearn users: `compat.patch_lazy_losses()` replaces `cflearn.models.common.CommonTrainStep.loss_fn`
    (models/common.py:31-43: `.item()` on every loss key, every step) by one that hands out `LazyFloat`s.  Here the two
    modules the patch reads are stand-ins with the reference's names and call signature: 60 SGD steps of a small model
    whose losses a trainer-like loop reads only every 10 steps — the values are read back only when consumed, they are
    the loss values, training still learns, and `restore_losses` puts the original back."""
    from cflearn_amd import compat

    class TrainStepLoss(types.SimpleNamespace):
        def __init__(self, loss, losses):
            super().__init__(loss=loss, losses=losses)

    class CommonTrainStep:
        def __init__(self, loss):
            self.loss = loss

        def loss_fn(self, m, state, batch, forward_results, **kwargs):
            losses = self.loss.run(forward_results, batch, state)
            return TrainStepLoss(losses[TO.LOSS_KEY], {k: v.item() for k, v in losses.items()})

    common = types.ModuleType("cflearn.models.common")
    common.CommonTrainStep, common.TrainStepLoss = CommonTrainStep, TrainStepLoss
    constants = types.ModuleType("cflearn.constants")
    constants.LOSS_KEY = TO.LOSS_KEY
    monkeypatch.setitem(sys.modules, "cflearn.models.common", common)
    monkeypatch.setitem(sys.modules, "cflearn.constants", constants)

    class _Loss:
        @staticmethod
        def run(forward_results, batch, state):
            return TO.run_loss("focal", forward_results, batch)

    model = _mlp()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    step = CommonTrainStep(_Loss())
    orig = compat.patch_lazy_losses()
    seen, exact = [], []
    try:
        assert CommonTrainStep.loss_fn is not orig
        batches = _batches(4)
        for i in range(60):
            batch = batches[i % len(batches)]
            out = step.loss_fn(model, object(), batch, {TO.PREDICTIONS_KEY: model(batch[TO.INPUT_KEY])})
            opt.zero_grad()
            out.loss.backward()
            opt.step()
            seen.append(out.losses[TO.LOSS_KEY])
            exact.append(out.loss.item())
            if i % 10 == 9:  # the monitor / logging steps read the value
                assert f"{seen[-1]:.6f}" == f"{exact[-1]:.6f}"
    finally:
        compat.restore_losses(orig)
    assert CommonTrainStep.loss_fn is orig
    assert len(seen) == 60 and all(isinstance(v, compat.LazyFloat) for v in seen)
    assert sum(v.is_materialized for v in seen) == 6
    assert [float(v) for v in seen] == exact
    assert float(seen[-1]) < float(seen[0])


@pytest.mark.parametrize("method", ["auto_prune", "hard_prune", "soft_prune", "simplified", "surgery"])
def test_pruner_matches_the_reference_bit_for_bit(frozen, method):
    """`Linear(pruner_config=...)` (customs.py:54-62,84-96): the weight mask of `modules.Pruner` against the reference's
    `Pruner` (customs.py:317-413) — same state keys and bit-equal initial values, the same masked weight and gradients to
    the weight and (auto_prune) to the four learnable scalars (bit-equal on the CPU that made the fixture).  Pure
    weight-space math: torch ops on both sides."""
    import cflearn_amd as C

    ref = frozen["pruner"][method]
    b = C.modules.Pruner({"method": method}, [12, 20])
    sa, sb = ref["sd"], b.state_dict()
    assert ref["keys"] == list(sb) or set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    wb = ref["w"].clone().requires_grad_(True)
    yb = b(wb)
    _assert_ulps(yb, ref["y"], "masked weight")
    yb.backward(ref["g"])
    _assert_ulps(wb.grad, ref["w_grad"], "weight gradient")
    pa, pb = ref["param_grads"], dict(b.named_parameters())
    assert set(pa) == set(pb) and (set(pa) == {"alpha", "beta", "gamma", "max_ratio"}) == (method == "auto_prune")
    for k in pa:
        _assert_ulps(pb[k].grad, pa[k], k)
    lin_b = C.Linear(20, 12, pruner_config={"method": method})
    assert set(ref["linear_keys"]) == set(lin_b.state_dict())


@pytest.mark.parametrize("kw", [
    dict(kernel_size=3, padding="reflection"), dict(kernel_size=3, padding="reflection2", bias=False),
    dict(kernel_size=3, transform_kernel=True), dict(kernel_size=3, padding="reflection", transform_kernel=True),
    dict(kernel_size=3, demodulate=True), dict(kernel_size=3, weight_scale=0.37),
    dict(kernel_size=3, bias=False, demodulate=True, style=True), dict(kernel_size=1, bias=False, style=True),
    dict(kernel_size=4, stride=2, padding=1, transpose=True), dict(kernel_size=3, padding=1, bias=False, transpose=True, weight_scale=2.0),
])
def test_conv2d_option_logic_matches_the_reference_with_torch_standing_in_for_the_kernels(frozen, kw, monkeypatch):
    """The round-5 Conv2d options (convs/basic.py:41-177): everything AROUND the convolution kernel — which padding, which
    weight the convolution sees (kernel transform, style modulation, demodulation, scale), the grouped-over-the-batch reshape of the
    stylised form, the transposed weight — with the three HIP entry points replaced by their torch definitions
    (`F.pad(mode="reflect")`, `F.conv2d`, `F.conv_transpose2d`), against the reference module on the same weights and input.
    (The kernels themselves are compared with the same torch calls on the GPU: tests/test_gpu_conv.py.)"""
    import torch.nn.functional as F

    import cflearn_amd as C
    from cflearn_amd import functional as HF

    ref = frozen["conv2d"][repr(kw)]
    kw = dict(kw)
    transpose = kw.pop("transpose", False)
    kw.pop("style", None)
    b = C.Conv2d(6, 8, **kw)
    b.load_state_dict(ref["sd"])
    monkeypatch.setattr(HF, "reflect_pad2d", lambda x, pads: F.pad(x, list(pads), mode="reflect"))
    monkeypatch.setattr(HF, "conv2d", lambda x, w, bias, s, p, d=1, g=1: F.conv2d(x, w, bias, stride=s, padding=p, dilation=d, groups=g))
    monkeypatch.setattr(HF, "conv_transpose2d", lambda x, wt, s, p, d=1: F.conv_transpose2d(x, wt, None, stride=s, padding=p, dilation=d))
    ya = ref["y"]
    yb = b(ref["x"], ref["style"], transpose=transpose)
    assert ya.shape == yb.shape
    assert (ya - yb).abs().max() <= 1e-5 * max(1.0, ya.abs().max().item()), (ya - yb).abs().max()
    yb.backward(ref["g"])
    assert (ref["weight_grad"] - b.weight.grad).abs().max() <= 1e-4 * ref["weight_grad"].abs().max()
