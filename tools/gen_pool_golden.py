"""Generate the head-pooler fixture from the reference's own code on the CPU (cflearn/modules/core/mixed_stacks/poolers.py:27-39,
api.py:270-458):

    python tools/gen_pool_golden.py

  tests/golden/head_poolers.pt:
    "keys": for head_pooler "mean" / "sequence" in the three head-norm positions ("pre": the default PreNorm head, "after":
      norm_after_head=True, "none": no_head_norm=True) the (name, shape) of every state-dict entry of the reference's
      MixedStackedEncoder(64, 10, attention, norm_type="layer", 2 layers) whose name starts with "head";
    "kwargs": the constructor keywords shared by all of them;
    "modules": for each pooler in the default position one record: `sd` = the reference's state dict (the stack's entries are stored
      once, under "stack_sd"; a record holds only its "head*" entries), the input `x` [16, 10, 64], the output gradient `dy`, the
      reference's fp32 output `y`, and for the loss sum(y * dy) its `dx` and `grads` per parameter name; then the reference's own
      rel-L2 distance from those under torch.autocast("cpu", bfloat16): `y_dist`, `dx_dist`, `grad_dist` per name.  A gradient of
      more than 2 048 elements is stored as every fourth row, and its distance is taken over those rows.
      Two distances are not yardsticks: the mean pooler's `head.norms.0.bias` gradient is the plain sum of the dyadic `dy` over the
      batch (exact in both runs: distance 0), and the sequence pooler's projection bias has a gradient that is zero in exact
      arithmetic (a softmax does not see a shift of its logits): both runs hold rounding noise.

ASSERTED here: every y_dist >= 1e-3 (the yardstick is not vacuous) and the sequence pooler's weights are far from uniform (the largest
softmax weight of a sample is at least 3 / T on average), so the projection matters.

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same bytes."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 4421
D, T, BATCH = 64, 10, 16
KWARGS = dict(in_dim=D, num_tokens=T, token_mixing_type="attention", token_mixing_config=dict(num_heads=1), num_layers=2,
              norm_type="layer", drop_path_rate=0.0, latent_dim=D)
POSITIONS = {"pre": {}, "after": dict(norm_after_head=True), "none": dict(no_head_norm=True)}
MIN_BF16_REL = 1e-3
MAX_GRAD_ELEMS, GRAD_ROW_STEP = 2048, 4  # a larger gradient is stored (and its distance taken) as every fourth row


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run(net, x, dy, autocast):
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = net(xg)
    else:
        y = net(xg)
    (y.float() * dy).sum().backward()
    grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    return y.detach().float().clone(), grads, xg.grad.detach().clone()


def fill(net, seed):
    """matrices N(0, 0.1), norm weights 1 + N(0, 0.1), every bias N(0, 0.1); the pooler's projection N(0, 0.5)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in net.named_parameters():
            noise = torch.randn(p.shape, generator=gen)
            if "projection" in k and k.startswith("head"):
                p.copy_(noise * 0.5)
            elif p.dim() >= 2 or k.endswith("bias"):
                p.copy_(noise * 0.1)
            else:
                p.copy_(1.0 + noise * 0.1)


def generate():
    torch.set_num_threads(1)
    import_cflearn()
    Encoder = importlib.import_module("cflearn.modules.core.mixed_stacks.api").MixedStackedEncoder
    keys, modules, stack_sd = {}, {}, None
    for pooler in ("mean", "sequence"):
        for pos, extra in POSITIONS.items():
            torch.manual_seed(SEED)
            net = Encoder(**KWARGS, head_pooler=pooler, **extra)
            keys[f"{pooler}/{pos}"] = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("head")]
        torch.manual_seed(SEED)
        net = Encoder(**KWARGS, head_pooler=pooler)
        fill(net, SEED)
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        if stack_sd is None:
            stack_sd = {k: v for k, v in sd.items() if not k.startswith("head")}
        assert all(torch.equal(sd[k], v) for k, v in stack_sd.items())
        gen = torch.Generator().manual_seed(SEED + 1)
        x = torch.randn((BATCH, T, D), generator=gen)
        dy = (torch.randn((BATCH, D), generator=gen) * 32.0).round().clamp(-127.0, 127.0) / 32.0
        y, grads, dx = run(net, x, dy, False)
        y16, grads16, dx16 = run(net, x, dy, True)
        for k in [k for k, g in grads.items() if g.numel() > MAX_GRAD_ELEMS]:  # every GRAD_ROW_STEP-th row of a matrix
            grads[k], grads16[k] = grads[k][::GRAD_ROW_STEP].clone(), grads16[k][::GRAD_ROW_STEP].clone()
        rec = dict(sd={k: v for k, v in sd.items() if k.startswith("head")}, x=x, dy=dy, y=y, dx=dx, grads=grads, y_dist=rel_l2(y16, y),
                   dx_dist=rel_l2(dx16, dx), grad_dist={k: rel_l2(grads16[k], grads[k]) for k in grads})
        assert rec["y_dist"] >= MIN_BF16_REL, (pooler, rec["y_dist"])
        if pooler == "sequence":
            with torch.no_grad():
                feats = net.head.norms[0](net.mixing_blocks[1](net.mixing_blocks[0](x)))
                peak = torch.softmax(net.head.module.projection(feats), dim=1).amax(1).mean()
            assert float(peak) >= 3.0 / T, float(peak)
        modules[pooler] = rec
    return dict(keys=keys, kwargs=dict(KWARGS), stack_sd=stack_sd, modules=modules)


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "head_poolers.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for name, rec in data["modules"].items():
        gd = rec["grad_dist"]
        print(f"  {name}: y std {float(rec['y'].std()):.3f}, y_dist {rec['y_dist']:.3e}, dx_dist {rec['dx_dist']:.3e}, "
              f"grad_dist {min(gd.values()):.3e} .. {max(gd.values()):.3e}")


if __name__ == "__main__":
    main()
