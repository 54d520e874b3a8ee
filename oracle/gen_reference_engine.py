"""Freeze what the REFERENCE'S OWN code computes for the `not gpu` tests that compare this package (and the oracle
restatements) with it: tests/golden/reference_engine.pt.  — TEST INFRASTRUCTURE ONLY.

Build container only (imports the reference from /root/reference through oracle/refharness):

    python oracle/gen_reference_engine.py

The tests then run from the fixture alone, on any machine:
  * tests/test_oracle.py::test_oracle_vs_reference_live — ViTEncoder + Linear head and self-attention outputs;
  * tests/test_reference_engine.py — the step engine (`CommonDLModel.train` + `Trainer.clip_norm_step`), `Pruner`,
    `Conv2d` options, the registry's names / FCNN state_dict keys, and `gradient_checkpoint` around a Linear.
Every entry is the reference's fp32 CPU result on seeded inputs; the inputs and initial weights are stored with it.
"""
import os
import sys
import types
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import trainer_oracle as TO  # noqa: E402
import vit_oracle as O  # noqa: E402
from refharness import import_cflearn, load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "reference_engine.pt")

# the parametrisations of tests/test_reference_engine.py (the fixture is keyed by them)
STEP_CASES = [("focal", 1, 0.0), ("cross_entropy", 2, 0.05), ("focal", 3, 0.1)]
PRUNE_METHODS = ["auto_prune", "hard_prune", "soft_prune", "simplified", "surgery"]
CONV_CASES = [
    dict(kernel_size=3, padding="reflection"), dict(kernel_size=3, padding="reflection2", bias=False),
    dict(kernel_size=3, transform_kernel=True), dict(kernel_size=3, padding="reflection", transform_kernel=True),
    dict(kernel_size=3, demodulate=True), dict(kernel_size=3, weight_scale=0.37),
    dict(kernel_size=3, bias=False, demodulate=True, style=True), dict(kernel_size=1, bias=False, style=True),
    dict(kernel_size=4, stride=2, padding=1, transpose=True), dict(kernel_size=3, padding=1, bias=False, transpose=True, weight_scale=2.0),
]


def _sd(m: torch.nn.Module) -> dict:
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def gen_vit_live(ref) -> dict:
    torch.manual_seed(3)
    enc = ref.ViTEncoder(img_size=32, patch_size=16, in_channels=3, latent_dim=64, num_layers=1)
    head = ref.Linear(64, 5)
    sd = {f"encoder.{k}": v.detach().clone() for k, v in enc.state_dict().items()}
    sd.update({f"head.{k}": v.detach().clone() for k, v in head.state_dict().items()})
    img = torch.randn(3, 3, 32, 32)
    with torch.no_grad():
        logits = head(enc(img))
    att = ref.Attention(64, 1, is_self_attention=True)
    x = torch.randn(2, 9, 64)
    mask = torch.rand(2, 9, 9) < 0.2
    mask[:, range(9), range(9)] = False
    with torch.no_grad():
        att_out = att(x, x, x, mask=mask).output
    assert (O.vit_classifier(img, sd, 1, 1) - logits).abs().max() < 2e-5
    return dict(sd=sd, img=img, logits=logits, att_sd=_sd(att), x=x, mask=mask, att_out=att_out)


def _mlp() -> torch.nn.Module:
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))


def _batches(n: int):
    g = torch.Generator().manual_seed(7)
    return [{TO.INPUT_KEY: torch.randn(8, 12, generator=g), TO.LABEL_KEY: torch.randint(0, 4, (8, 1), generator=g)}
            for _ in range(n)]


def gen_step_engine(cflearn) -> dict:
    """`CommonDLModel.train` driven by a trainer object that carries the reference's own `Trainer.clip_norm_step`:
    the `.item()` losses of 6 SGD batches and the weights after them."""
    CommonDLModel = sys.modules["cflearn.models.common"].CommonDLModel
    build_loss = sys.modules["cflearn.losses"].build_loss
    Trainer = sys.modules["cflearn.trainer"].Trainer

    class _Accel:
        sync_gradients = True

        @staticmethod
        def backward(loss):
            loss.backward()

        @staticmethod
        def clip_grad_norm_(params, max_norm):
            return torch.nn.utils.clip_grad_norm_(params, max_norm)

    out = {}
    for loss_name, grad_accumulate, clip_norm in STEP_CASES:
        ref = CommonDLModel()
        ref.m = _mlp()
        ref.loss = build_loss(loss_name)
        opt_ref = torch.optim.SGD(ref.m.parameters(), lr=0.1)
        trainer = types.SimpleNamespace(state=TO.State(), accelerator=_Accel(), optimizers={"all": opt_ref},
                                        config=TO.Config(grad_accumulate, clip_norm), should_autocast=False,
                                        model_for_training=ref.m, scheduler_step=lambda: None, _gradient_norm=None)
        trainer.clip_norm_step = types.MethodType(Trainer.clip_norm_step, trainer)
        losses = []
        for i, batch in enumerate(_batches(6)):
            trainer.state.step += 1
            losses.append(ref.train(i, batch, trainer, {}, {}).loss_dict[TO.LOSS_KEY])
        out[(loss_name, grad_accumulate, clip_norm)] = dict(
            losses=losses, params=[p.detach().clone() for p in ref.m.parameters()])
    return out


def gen_pruner() -> dict:
    customs = sys.modules["cflearn.modules.core.customs"]
    out = {}
    for method in PRUNE_METHODS:
        a = customs.Pruner({"method": method}, [12, 20])
        sd = _sd(a)
        torch.manual_seed(3)
        w = torch.randn(12, 20)
        wa = w.clone().requires_grad_(True)
        y = a(wa)
        g = torch.randn_like(w)
        y.backward(g)
        lin = customs.Linear(20, 12, pruner_config={"method": method})
        out[method] = dict(keys=list(sd), sd=sd, w=w, y=y.detach(), g=g, w_grad=wa.grad.clone(),
                           param_grads={k: p.grad.clone() for k, p in a.named_parameters()},
                           linear_keys=list(lin.state_dict()))
    return out


def gen_conv2d() -> dict:
    basic = sys.modules["cflearn.modules.core.convs.basic"]
    out = {}
    for case in CONV_CASES:
        kw = dict(case)
        style_on, transpose = kw.pop("style", False), kw.pop("transpose", False)
        torch.manual_seed(5)
        a = basic.Conv2d(6, 8, **kw)
        x = torch.randn(3, 6, 9, 9)
        style = torch.randn(3, 6) if style_on else None
        y = a(x, style, transpose=transpose)
        g = torch.randn_like(y)
        y.backward(g)
        out[repr(case)] = dict(sd=_sd(a), x=x, style=style, y=y.detach(), g=g, weight_grad=a.weight.grad.clone())
    return out


def gen_registry() -> dict:
    common = sys.modules["cflearn.modules.common"]
    torch.manual_seed(9)
    fcnn = common.build_module("fcnn", config=dict(input_dim=10, output_dim=3, hidden_units=[16, 16]))
    return dict(names=sorted(common.module_dict), fcnn_sd=_sd(fcnn))


def gen_gradient_checkpoint() -> dict:
    """The reference's `gradient_checkpoint` (toolkit.py:2535-2647) around tanh(Linear(x)): gradients of sum()."""
    gradient_checkpoint = sys.modules["cflearn.toolkit"].gradient_checkpoint
    torch.manual_seed(0)
    lin = torch.nn.Linear(6, 6)
    x = torch.randn(5, 6, requires_grad=True)
    sd = _sd(lin)
    y = gradient_checkpoint(lambda inp: torch.tanh(lin(inp)), (x,), tuple(lin.parameters()), True)
    y.sum().backward()
    return dict(sd=sd, x=x.detach().clone(), gx=x.grad.clone(), gw=lin.weight.grad.clone(), gb=lin.bias.grad.clone())


def main() -> None:
    torch.set_num_threads(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch.cuda.amp.autocast deprecation inside the reference
        ref = load_reference()
        cflearn = import_cflearn()
        fixture = dict(vit_live=gen_vit_live(ref), step_engine=gen_step_engine(cflearn), pruner=gen_pruner(),
                       conv2d=gen_conv2d(), registry=gen_registry(), gradient_checkpoint=gen_gradient_checkpoint())
    torch.save(fixture, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
