"""Generate the ml_rnn fixture from the reference's own code on the CPU (cflearn/modules/ml/rnn.py):

    python tools/gen_rnn_golden.py

  tests/golden/rnn_small.pt
    "states"   for the four constructor configurations of STATE_CONFIGS (default GRU, LSTM, 2-layer bidirectional GRU, H = 40): the
               keywords and the (name, shape) of every entry of the reference's state dict, in order;
    "configs"  the same four cells, with a narrow head (hidden_units = [48]) so that every gradient fits the fixture: keywords, the
               seed of the parameters, the input `x`, the output gradient `dy`, the reference's fp32 logits `y` and its gradients for
               the loss sum(logits * dy) (`grads` per parameter name, `dx`), and the reference's own distance under
               torch.autocast("cpu", bfloat16) from those: `y_dist`, `grad_dist` per name, `dx_dist` (rel-L2).  A gradient of more
               than 8 192 elements (the matrices at H = 256) is stored as every `grad_rows[name]`-th row, and its distance is taken
               over those rows.  `hh_effect`: rel-L2 by which the logits move when every weight_hh* is zeroed;
    "steps"    for each cell the seed, x [B, 1, F], h0 and c0 [B, H] (float64) of the one-step replica test.

Parameters are not stored: tests/rnn_weights.fill_parameters(model, seed) rebuilds them (scaled: see that file).  ASSERTED here:
y_dist >= 1e-3 for every configuration (the yardstick of the module test is not vacuous) and hh_effect >= 0.1 (the recurrence matters).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same values."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from rnn_weights import fill_parameters, step_tensors  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 5309
# (name, constructor keywords, input shape [B, T, F])
STATE_CONFIGS = [
    ("gru", dict(input_dim=24, output_dim=3), (5, 9, 24)),
    ("lstm", dict(input_dim=24, output_dim=3, cell="LSTM"), (5, 9, 24)),
    ("bigru2", dict(input_dim=24, output_dim=3, num_layers=2, bidirectional=True), (5, 9, 24)),
    ("gru_h40", dict(input_dim=10, output_dim=3, hidden_size=40), (3, 7, 10)),
]
HEAD = dict(hidden_units=[48])
MIN_BF16_REL = 1e-3
MIN_HH_EFFECT = 0.1
MAX_GRAD_ELEMS = 8192
STEP_SEEDS = {"GRU": 811, "LSTM": 812}


def _rnn():
    import_cflearn()
    return importlib.import_module("cflearn.modules.ml.rnn")


def rel_l2(a, b):
    """0 for a reference that is exactly zero and met exactly (dW_hh of the last layer's reverse direction: `net[:, -1]` is its
    first step, taken from the zero state)"""
    if not b.any() and not a.any():
        return 0.0
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
    return y.detach().float().clone(), {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}, xg.grad.detach().clone()


def config_fixture(mod, index, name, kw, shape):
    seed = SEED + index
    kw = dict(kw, **HEAD)
    net = mod.RNN(**kw)
    fill_parameters(net, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen)
    dy = torch.randn((shape[0], kw["output_dim"]), generator=gen)
    y, grads, dx = run(net, x, dy, False)
    y16, grads16, dx16 = run(net, x, dy, True)
    grad_rows = {k: -(-g.numel() // MAX_GRAD_ELEMS) for k, g in grads.items() if g.numel() > MAX_GRAD_ELEMS}
    for k, step in grad_rows.items():
        grads[k], grads16[k] = grads[k][::step].clone(), grads16[k][::step].clone()
    y_dist = rel_l2(y16, y)
    assert y_dist >= MIN_BF16_REL, (name, y_dist)
    with torch.no_grad():
        keep = {k: p.clone() for k, p in net.named_parameters() if "weight_hh" in k}
        for k, p in net.named_parameters():
            if k in keep:
                p.zero_()
        hh_effect = rel_l2(net(x).float(), y)
        for k, p in net.named_parameters():
            if k in keep:
                p.copy_(keep[k])
    assert hh_effect >= MIN_HH_EFFECT, (name, hh_effect)
    return dict(name=name, kwargs=kw, seed=seed, x=x, dy=dy, y=y, dx=dx, grads=grads, grad_rows=grad_rows, y_dist=y_dist,
                grad_dist={k: rel_l2(grads16[k], grads[k]) for k in grads}, dx_dist=rel_l2(dx16, dx), hh_effect=hh_effect)


def generate():
    torch.set_num_threads(1)
    mod = _rnn()
    states = [dict(name=name, kwargs=dict(kw), state=[(k, tuple(v.shape)) for k, v in mod.RNN(**kw).state_dict().items()])
              for name, kw, _ in STATE_CONFIGS]
    configs = [config_fixture(mod, i, name, kw, shape) for i, (name, kw, shape) in enumerate(STATE_CONFIGS)]
    steps = {}
    for cell, seed in STEP_SEEDS.items():
        _, x, h0, c0 = step_tensors(cell, seed)
        steps[cell] = dict(seed=seed, x=x, h0=h0, c0=c0)
    return dict(states=states, configs=configs, steps=steps)


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "rnn_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        gd = rec["grad_dist"]
        print(f"  {rec['name']}: y std {float(rec['y'].std()):.3f}, y_dist {rec['y_dist']:.3e}, dx_dist {rec['dx_dist']:.3e}, grad_dist "
              f"{min(gd.values()):.3e} .. {max(gd.values()):.3e}, hh_effect {rec['hh_effect']:.3f}")


if __name__ == "__main__":
    main()
