"""Generate the NBM fixture from the reference's own code on the CPU (cflearn/modules/ml/nbm.py):

    python tools/gen_nbm_golden.py

  tests/golden/nbm_small.pt
    "states"   for the four constructor configurations of CONFIGS (default at input_dim = 12; input_dim = 20, i.e. H = 40; orders
               1 + 2 with a repeated feature; three bases of width 8 and order 3): the keywords and the (name, shape) of every entry
               of the reference's state dict, in order;
    "configs"  the same four: keywords, the seed of the parameters, the input `x`, the output gradient `dy`, the reference's fp32
               logits `y`, its `return_features` output `feat`, and its gradients for the loss sum(logits * dy) (`grads` per parameter
               name, `dx`), and the reference's own distance under torch.autocast("cpu", bfloat16) from those: `y_dist`, `feat_dist`,
               `grad_dist` per name, `dx_dist` (rel-L2).  A gradient of more than 8 192 elements is stored as every
               `grad_rows[name]`-th row, and its distance is taken over those rows.  `w2_effect`: rel-L2 by which the logits move when
               every net.1.conv.weight is zeroed;
    "inspect"  two `inspect` calls of the reference (configuration index, x_dims, y_dim, already_extracted, input, fp32 output).

Batch sizes.  The yardstick of the module test is a DISTANCE BETWEEN TWO NOISE REALISATIONS: the reference's bf16 run and this package's
run round different things, and for a gradient that is a sum of n independently rounded addends either distance scatters by about
1 / sqrt(2 n) around its expectation.  The smallest gradient is head.bias: output_dim numbers, each the sum over the batch of the
bf16-rounded dy, the same mechanism on both sides.  The batches are sized for n = output_dim * B >= 200 there, a scatter of 5 % or
less against the 10 % margin of "1.1 x the reference's distance": 72 samples at output_dim = 3, 104 at output_dim = 2.

Seeds.  A configuration's seed is the first of SEED + index + 100 n whose fp32 gradients agree with a float64 run of the same reference
to 2e-6 (no ReLU mask differs between the two): see config_fixture.

Parameters are not stored: tests/nbm_weights.fill_parameters(model, seed) rebuilds them.  ASSERTED here: y_dist >= 1e-3 for every
configuration (the yardstick of the module test is not vacuous) and w2_effect >= 0.1 (the hidden product matters).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same values."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from nbm_weights import fill_parameters  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 7411
MIXED = {"1": [(0,), (1,), (2,), (3,), (4,), (5,)], "2": [(0, 1), (2, 2), (1, 4), (0, 5)]}
TRIPLES = {"3": [(0, 1, 2), (1, 3, 4), (2, 2, 0)]}
# (name, constructor keywords, batch size)
CONFIGS = [
    ("default12", dict(input_dim=12, output_dim=3), 72),
    ("h40", dict(input_dim=20, output_dim=2), 104),
    ("mixed", dict(input_dim=6, output_dim=3, nary=MIXED, num_bases=32, hidden_units=[64, 64]), 72),
    ("triples", dict(input_dim=5, output_dim=2, nary=TRIPLES, num_bases=3, hidden_units=[8, 8]), 104),
]
INSPECT = [(2, (2, 2), 1, False), (3, (1, 3, 4), 0, True)]
MIN_BF16_REL = 1e-3
MIN_W2_EFFECT = 0.1
MAX_GRAD_ELEMS = 8192


def _nbm():
    import_cflearn()
    return importlib.import_module("cflearn.modules.ml.nbm")


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run(net, x, dy, autocast):
    net.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = net(xg)
            with torch.no_grad():
                feat = net(x, return_features=True)
    else:
        y = net(xg)
        with torch.no_grad():
            feat = net(x, return_features=True)
    (y.float() * dy).sum().backward()
    grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    return y.detach().float().clone(), feat.detach().float().clone(), grads, xg.grad.detach().clone()


def config_fixture(mod, index, name, kw, batch):
    """the first seed SEED + index + 100 n whose fp32 run has no ReLU unit on the other side of zero than the float64 run of the same
    reference (one such unit of 10^6 moves a gradient by 1e-3: the fp32 record would then not be THE gradient, and the replica test
    of tests/test_nbm_host.py could not meet it to 1e-5).  Decided from the reference alone."""
    for attempt in range(16):
        rec, net = _config_fixture(mod, SEED + index + 100 * attempt, name, kw, batch)
        if rec is not None:
            return rec, net
    raise AssertionError(f"{name}: no seed with an fp32 run free of mask flips")


def _config_fixture(mod, seed, name, kw, batch):
    net = mod.NBM(**kw)
    fill_parameters(net, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, kw["input_dim"]), generator=gen)
    dy = torch.randn((batch, kw["output_dim"]), generator=gen)
    y, feat, grads, dx = run(net, x, dy, False)
    net.double()
    _, _, grads64, dx64 = run(net, x.double(), dy.double(), False)
    net.float()
    if max([rel_l2(dx, dx64.float())] + [rel_l2(grads[k], grads64[k]) for k in grads]) > 2e-6:
        return None, None
    y16, feat16, grads16, dx16 = run(net, x, dy, True)
    grad_rows = {k: -(-g.numel() // MAX_GRAD_ELEMS) for k, g in grads.items() if g.numel() > MAX_GRAD_ELEMS}
    for k, step in grad_rows.items():
        grads[k], grads16[k] = grads[k][::step].clone(), grads16[k][::step].clone()
    y_dist = rel_l2(y16, y)
    assert y_dist >= MIN_BF16_REL, (name, y_dist)
    with torch.no_grad():
        keep = {k: p.clone() for k, p in net.named_parameters() if k.endswith("net.1.conv.weight")}
        for k, p in net.named_parameters():
            if k in keep:
                p.zero_()
        w2_effect = rel_l2(net(x).float(), y)
        for k, p in net.named_parameters():
            if k in keep:
                p.copy_(keep[k])
    assert keep and w2_effect >= MIN_W2_EFFECT, (name, w2_effect)
    rec = dict(name=name, kwargs=kw, seed=seed, x=x, dy=dy, y=y, feat=feat, dx=dx, grads=grads, grad_rows=grad_rows, y_dist=y_dist,
               feat_dist=rel_l2(feat16, feat), grad_dist={k: rel_l2(grads16[k], grads[k]) for k in grads}, dx_dist=rel_l2(dx16, dx),
               w2_effect=w2_effect)
    return rec, net


def generate():
    torch.set_num_threads(1)
    mod = _nbm()
    states = [dict(name=name, kwargs=dict(kw), state=[(k, tuple(v.shape)) for k, v in mod.NBM(**kw).state_dict().items()])
              for name, kw, _ in CONFIGS]
    configs, nets = [], []
    for i, (name, kw, batch) in enumerate(CONFIGS):
        rec, net = config_fixture(mod, i, name, kw, batch)
        configs.append(rec)
        nets.append(net)
    inspects = []
    for index, x_dims, y_dim, extracted in INSPECT:
        x = configs[index]["x"]
        inp = x[:, list(x_dims)].contiguous() if extracted else x
        with torch.no_grad():
            out = nets[index].inspect(inp, x_dims, y_dim, already_extracted=extracted)
        inspects.append(dict(config=index, x_dims=x_dims, y_dim=y_dim, already_extracted=extracted, input=inp.clone(), out=out.float().clone()))
    return dict(states=states, configs=configs, inspect=inspects)


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "nbm_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        gd = rec["grad_dist"]
        print(f"  {rec['name']}: y std {float(rec['y'].std()):.3f}, feat std {float(rec['feat'].std()):.3f}, y_dist {rec['y_dist']:.3e}, "
              f"feat_dist {rec['feat_dist']:.3e}, dx_dist {rec['dx_dist']:.3e}, grad_dist {min(gd.values()):.3e} .. {max(gd.values()):.3e}, "
              f"w2_effect {rec['w2_effect']:.3f}")
    for rec in data["inspect"]:
        print(f"  inspect {rec['x_dims']} -> y{rec['y_dim']}: {tuple(rec['out'].shape)}, std {float(rec['out'].std()):.3f}")


if __name__ == "__main__":
    main()
