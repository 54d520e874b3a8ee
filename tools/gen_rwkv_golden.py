"""Generate the RWKV fixture from the reference's own code on the CPU (cflearn/modules/core/mixed_stacks/token_mixers.py:107-206,
channel_mixers.py:69-113, api.py):

    python tools/gen_rwkv_golden.py

  tests/golden/rwkv_small.pt, "configs": five records —
    the token mixer and the channel mixer stand-alone at layer_idx 1 and 3 of a 4-layer stack, and a 3-layer MixedStackedEncoder with
    token_mixing_type = channel_mixing_type = "rwkv", norm_type = "layer", head_pooler = None, drop_path_rate = 0.0; all at C = 64,
    L = 96, T = 24.  Per record: `kind` ("token", "channel", "encoder"), the constructor keywords, the seed, `state` = (name, shape,
    dtype) of every entry of the reference's state dict in order, `init` = the reference's initial info_decay / time_mix_* values, the
    input `x`, the output gradient `dy`, the reference's fp32 output `y`, and for the loss sum(y * dy) its `dx` and `grads` per parameter
    name; then the reference's own rel-L2 distance from those under torch.autocast("cpu", bfloat16): `y_dist`, `dx_dist`, `grad_dist`
    per name.  A gradient of more than 2 048 elements is stored as every `grad_rows[name]`-th row, and its distance is taken over
    those rows.  `dy` is dyadic (multiples of 2^-5 below 4 in magnitude: exact in bfloat16, and any sum of them over the batch is exact
    in float32), because the head LayerNorm's bias gradient is that plain sum: the reference computes it without any bf16 rounding
    (distance 0), and only an order-independent sum can be met exactly.  `decay_effect` (token mixer and encoder): rel-L2 by which the output moves when every info_decay is set to +10, i.e.
    lam = 0 and the scan forgets everything before the current step.

Batch size.  The yardstick of the module tests is a distance between two noise realisations (tools/gen_nbm_golden.py explains the
scatter): a gradient that sums n independently rounded addends scatters by about 1 / sqrt(2 n).  The smallest gradients here are the
time mixes and info_decay, 64 / 96 numbers that each sum over the B T = 96 positions: n >= 6 144 >= 200 at B = 4.

Parameters are not stored: tests/rwkv_weights.fill_parameters(model, seed) rebuilds the Linear weights (std 0.1), everything else keeps
the constructor's value.  ASSERTED here: every y_dist >= 1e-3 (the yardstick is not vacuous) and every decay_effect >= 0.1 (the scan
matters).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same bytes."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from rwkv_weights import fill_parameters  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 9173
C, L, T, BATCH = 64, 96, 24, 4
ENCODER = dict(in_dim=C, num_tokens=T, token_mixing_type="rwkv", channel_mixing_type="rwkv", num_layers=3, norm_type="layer",
               head_pooler=None, drop_path_rate=0.0, latent_dim=L)
# (name, kind, constructor keywords)
CONFIGS = [
    ("token_l1", "token", dict(layer_idx=1, num_layers=4, num_tokens=T, in_dim=C, latent_dim=L)),
    ("token_l3", "token", dict(layer_idx=3, num_layers=4, num_tokens=T, in_dim=C, latent_dim=L)),
    ("channel_l1", "channel", dict(layer_idx=1, num_layers=4, in_dim=C, latent_dim=L, dropout=0.0)),
    ("channel_l3", "channel", dict(layer_idx=3, num_layers=4, in_dim=C, latent_dim=L, dropout=0.0)),
    ("encoder3", "encoder", ENCODER),
]
MIN_BF16_REL = 1e-3
MIN_DECAY_EFFECT = 0.1
MAX_GRAD_ELEMS = 2048


def _classes():
    import_cflearn()
    pre = "cflearn.modules.core.mixed_stacks."
    return {"token": importlib.import_module(pre + "token_mixers").RWKVTokenMixer,
            "channel": importlib.import_module(pre + "channel_mixers").RWKVChannelMixer,
            "encoder": importlib.import_module(pre + "api").MixedStackedEncoder}


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


def config_fixture(classes, index, name, kind, kw):
    seed = SEED + index
    torch.manual_seed(seed)
    net = classes[kind](**kw)
    state = [(k, tuple(v.shape), str(v.dtype)) for k, v in net.state_dict().items()]
    init = {k: v.detach().clone() for k, v in net.state_dict().items() if k.endswith("info_decay") or "time_mix_" in k}
    fill_parameters(net, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((BATCH, T, C), generator=gen)
    dy = (torch.randn((BATCH, T, C), generator=gen) * 32.0).round().clamp(-127.0, 127.0) / 32.0
    y, grads, dx = run(net, x, dy, False)
    y16, grads16, dx16 = run(net, x, dy, True)
    grad_rows = {k: -(-g.numel() // MAX_GRAD_ELEMS) for k, g in grads.items() if g.numel() > MAX_GRAD_ELEMS}
    for k, step in grad_rows.items():
        grads[k], grads16[k] = grads[k][::step].clone(), grads16[k][::step].clone()
    y_dist = rel_l2(y16, y)
    assert y_dist >= MIN_BF16_REL, (name, y_dist)
    rec = dict(name=name, kind=kind, kwargs=dict(kw), seed=seed, state=state, init=init, x=x, dy=dy, y=y, dx=dx, grads=grads, grad_rows=grad_rows, y_dist=y_dist,
               dx_dist=rel_l2(dx16, dx), grad_dist={k: rel_l2(grads16[k], grads[k]) for k in grads})
    decays = [p for k, p in net.named_parameters() if k.endswith("info_decay")]
    if decays:
        with torch.no_grad():
            keep = [p.clone() for p in decays]
            for p in decays:
                p.fill_(10.0)
            rec["decay_effect"] = rel_l2(net(x).float(), y)
            for p, old in zip(decays, keep):
                p.copy_(old)
        assert rec["decay_effect"] >= MIN_DECAY_EFFECT, (name, rec["decay_effect"])
    return rec


def generate():
    torch.set_num_threads(1)
    classes = _classes()
    return dict(configs=[config_fixture(classes, i, *cfg) for i, cfg in enumerate(CONFIGS)])


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "rwkv_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        gd = rec["grad_dist"]
        print(f"  {rec['name']}: y std {float(rec['y'].std()):.3f}, y_dist {rec['y_dist']:.3e}, dx_dist {rec['dx_dist']:.3e}, "
              f"grad_dist {min(gd.values()):.3e} .. {max(gd.values()):.3e}, decay_effect {rec.get('decay_effect', float('nan')):.3f}")


if __name__ == "__main__":
    main()
