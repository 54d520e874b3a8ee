"""Generate the Siren fixture from the reference's own code on the CPU (cflearn/modules/implicit/siren.py):

    python tools/gen_siren_golden.py

  tests/golden/siren_small.pt, "configs": five records --
    Siren(5, 2, 1, 32, num_layers=2) at B = 3 (M = 75: a ragged last tile, tiles that straddle samples), Siren(5, 2, 3, 96, num_layers=4)
    at B = 3, Siren(8, 2, 3, 256, num_layers=4) at B = 4, the DDR form Siren(None, 1, 2, 32, num_layers=2, bias=False,
    use_modulator=False) with a tuple of modulations [5, 32] and init [5, 7, 1], and a conditional ImgSiren(8, 3, 64, num_classes=4)
    through `forward` and through `decode(size=6)`.
  Per record: `kind` ("siren", "img"), the constructor's `args` / `kwargs`, the `seed`, `state` = (name, shape, dtype) of every entry
  of the reference's state dict in order, `init_sha` = sha256 over the bytes of the reference's initial parameters under
  torch.manual_seed(seed) (and `grid`, the registered buffer, where there is one), the inputs (`z`, or `mods` and `init`, and
  `labels`), a dyadic `dy` (multiples of 2^-5 below 4 in magnitude: a sum of them over the rows is exact in float32, so head.bias's
  gradient can be met exactly), the reference's fp32 output `y` and for the loss sum(y * dy) its `grads` per parameter name and the
  input gradients `dz` / `dmods` / `dinit`; then the reference's own rel-L2 distance from those under torch.autocast("cpu",
  bfloat16): `y_dist`, `grad_dist` per name, `dz_dist`, `dmods_dist`, `dinit_dist`.  The ImgSiren record also holds `y_decode` /
  `y_decode_dist` of decode(size=6).  A gradient of more than 2 048 elements is stored as every `grad_rows[name]`-th row and its
  distance is taken over those rows.  `sub_floor`: the tensors whose yardstick falls below 1e-3 (head.bias: its gradient is the plain
  sum of dy, which the reference computes without any rounding): the tests bound those by the float64 replica instead.

Parameters are not stored: tests/siren_weights.fill_parameters(model, seed) rebuilds them.  ASSERTED here: every y_dist and every
weight's grad_dist >= 1e-3 (the yardstick is not vacuous).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same bytes."""
import hashlib
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from siren_weights import fill_parameters  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 4211
# (name, kind, args, kwargs, batch)
CONFIGS = [
    ("siren_32x2", "siren", (5, 2, 1, 32), dict(num_layers=2), 3),
    ("siren_96x4", "siren", (5, 2, 3, 96), dict(num_layers=4), 3),
    ("siren_256x4", "siren", (8, 2, 3, 256), dict(num_layers=4), 4),
    ("ddr_form", "siren", (None, 1, 2, 32), dict(num_layers=2, bias=False, use_modulator=False), 5),
    ("img_siren", "img", (8, 3, 64), dict(num_classes=4), 4),
]
DDR_ROWS = 7
DECODE_SIZE = 6
MIN_BF16_REL = 1e-3
MAX_GRAD_ELEMS = 2048


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def dyadic(shape, gen):
    return (torch.randn(shape, generator=gen) * 32.0).round().clamp(-127.0, 127.0) / 32.0


def sha(net):
    h = hashlib.sha256()
    for _, p in net.named_parameters():
        h.update(p.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(net, kind, inputs, dy, autocast):
    net.zero_grad(set_to_none=True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in inputs.items() if v.is_floating_point()}

    def call():
        if kind == "img":
            return net(leaves["z"], {"labels": inputs["labels"]})
        if "z" in leaves:
            return net(leaves["z"])
        return net(tuple(leaves["mods"].unbind(0)), init=leaves["init"])

    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = call()
    else:
        y = call()
    (y.float() * dy).sum().backward()
    grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    return y.detach().float().clone(), grads, {k: v.grad.detach().float().clone() for k, v in leaves.items()}


def config_fixture(classes, index, name, kind, args, kw, batch):
    seed = SEED + index
    torch.manual_seed(seed)
    net = classes[kind](*args, **kw)
    state = [(k, tuple(v.shape), str(v.dtype)) for k, v in net.state_dict().items()]
    rec = dict(name=name, kind=kind, args=args, kwargs=dict(kw), seed=seed, state=state, init_sha=sha(net))
    siren = net.siren if kind == "img" else net
    if siren.grid is not None:
        rec["grid"] = siren.grid.detach().clone()
    fill_parameters(net, seed)
    gen = torch.Generator().manual_seed(seed)
    latent = siren.latent_dim
    if siren.modulator is None:
        inputs = dict(mods=torch.randn((siren.num_layers, batch, latent), generator=gen),
                      init=torch.rand((batch, DDR_ROWS, siren.in_dim), generator=gen) * 2.0 - 1.0)
    else:
        inputs = dict(z=torch.randn((batch, latent), generator=gen))
    if kind == "img":
        inputs["labels"] = torch.randint(0, kw["num_classes"], (batch,), generator=gen)
    y_shape = (batch, args[1], args[0], args[0]) if kind == "img" else (batch, DDR_ROWS if siren.grid is None else siren.grid.shape[1], args[2])
    dy = dyadic(y_shape, gen)
    y, grads, din = run(net, kind, inputs, dy, False)
    y16, grads16, din16 = run(net, kind, inputs, dy, True)
    assert tuple(y.shape) == y_shape, (name, tuple(y.shape))
    grad_rows = {k: -(-g.numel() // MAX_GRAD_ELEMS) for k, g in grads.items() if g.numel() > MAX_GRAD_ELEMS}
    for k, step in grad_rows.items():
        grads[k], grads16[k] = grads[k][::step].clone(), grads16[k][::step].clone()
    rec.update(inputs)
    rec.update(dy=dy, y=y, grads=grads, grad_rows=grad_rows, y_dist=rel_l2(y16, y), grad_dist={k: rel_l2(grads16[k], grads[k]) for k in grads})
    for k, g in din.items():
        rec["d" + k], rec["d" + k + "_dist"] = g, rel_l2(din16[k], g)
    assert rec["y_dist"] >= MIN_BF16_REL, (name, rec["y_dist"])
    rec["sub_floor"] = sorted(k for k, d in rec["grad_dist"].items() if d < MIN_BF16_REL)
    for k in rec["sub_floor"]:
        assert not k.endswith("weight"), (name, k, rec["grad_dist"][k])
    if kind == "img":
        with torch.no_grad():
            yd = net.decode(inputs["z"], labels=inputs["labels"], size=DECODE_SIZE).float().clone()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                yd16 = net.decode(inputs["z"], labels=inputs["labels"], size=DECODE_SIZE).float()
        rec["y_decode"], rec["y_decode_dist"] = yd, rel_l2(yd16, yd)
        assert rec["y_decode_dist"] >= MIN_BF16_REL, (name, rec["y_decode_dist"])
    return rec


def generate():
    torch.set_num_threads(1)
    import_cflearn()
    mod = importlib.import_module("cflearn.modules.implicit.siren")
    classes = {"siren": mod.Siren, "img": mod.ImgSiren}
    return dict(configs=[config_fixture(classes, i, *cfg) for i, cfg in enumerate(CONFIGS)])


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "siren_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        gd = rec["grad_dist"]
        wd = [d for k, d in gd.items() if k.endswith("weight")]
        bd = [d for k, d in gd.items() if k.endswith("bias")] or [float("nan")]
        ins = {k: f"{v:.3e}" for k, v in rec.items() if k in ("dz_dist", "dmods_dist", "dinit_dist", "y_decode_dist")}
        print(f"  {rec['name']}: y std {float(rec['y'].std()):.3f}, y_dist {rec['y_dist']:.3e}, weights {min(wd):.3e} .. {max(wd):.3e}, "
              f"biases {min(bd):.3e} .. {max(bd):.3e}, {ins}, sub_floor {rec['sub_floor']}")


if __name__ == "__main__":
    main()
