"""Generate the RRDB upscaler fixture from the reference's own code on the CPU (cflearn/modules/cv/translator/rrdb.py):

    python tools/gen_rrdb_golden.py

  tests/golden/rrdb_small.pt
    "configs"    three nets with num_layers = 2: scale 4 on [2, 3, 12, 20], scale 2 on [1, 3, 16, 12], scale 1 on [1, 3, 16, 16]; for each
                 the constructor keywords, the seed of its parameters, the input `x`, the reference's fp32 output `y`, its output under
                 torch.autocast("cpu", bfloat16) `y_bf16`, and the smallest / largest standard deviation over its convolutions' outputs;
    "default_state"  (name, shape) of every entry of the state dict of the reference's DEFAULT net (23 layers), in order;
    "unshuffle"  the reference's `pixel_unshuffle` of an index ramp [1, 3, 8, 12] for s = 2 and s = 4.

Parameters are not stored: tests/rrdb_weights.fill_parameters(model, seed) rebuilds them (scaled: see that file).  Two things are
ASSERTED here: with forward hooks on the reference, every convolution's output has a standard deviation in [0.25, 4] (no layer hides
behind the residual path), and rel_l2(y_bf16, y) >= 1e-3 (the yardstick of the module test is not vacuous).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same values."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from rrdb_weights import fill_parameters  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 4117
# (name, constructor keywords, input shape)
CONFIGS = [
    ("x4", dict(in_channels=3, scale=4, num_layers=2), (2, 3, 12, 20)),
    ("x2", dict(in_channels=3, scale=2, num_layers=2), (1, 3, 16, 12)),
    ("x1", dict(in_channels=3, scale=1, num_layers=2), (1, 3, 16, 16)),
]
STD_RANGE = (0.25, 4.0)
MIN_BF16_REL = 1e-3
RAMP_SHAPE = (1, 3, 8, 12)


def _rrdb():
    import_cflearn()
    return importlib.import_module("cflearn.modules.cv.translator.rrdb")


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def config_fixture(mod, index, name, kw, shape):
    seed = SEED + index
    net = mod.RRDBNet(**kw)
    fill_parameters(net, seed)
    net.eval()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    stds = {}
    hooks = [m.register_forward_hook(lambda _m, _i, out, key=key: stds.__setitem__(key, float(out.float().std())))
             for key, m in net.named_modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        y = net(x).float().clone()
        for h in hooks:
            h.remove()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y_bf16 = net(x).float().clone()
    assert len(stds) == 15 * kw["num_layers"] + 6, len(stds)
    lo, hi = min(stds.values()), max(stds.values())
    assert STD_RANGE[0] <= lo and hi <= STD_RANGE[1], (name, min(stds, key=stds.get), lo, max(stds, key=stds.get), hi)
    spread = rel_l2(y_bf16, y)
    assert spread >= MIN_BF16_REL, (name, spread)
    return dict(name=name, kwargs=dict(kw), seed=seed, x=x, y=y, y_bf16=y_bf16, conv_std_min=lo, conv_std_max=hi)


def generate():
    torch.set_num_threads(1)
    mod = _rrdb()
    configs = [config_fixture(mod, i, name, kw, shape) for i, (name, kw, shape) in enumerate(CONFIGS)]
    default_state = [(k, tuple(v.shape)) for k, v in mod.RRDBNet().state_dict().items()]
    n = 1
    for d in RAMP_SHAPE:
        n *= d
    ramp = torch.arange(n, dtype=torch.float32).view(RAMP_SHAPE)
    unshuffle = {s: mod.pixel_unshuffle(ramp, s).clone() for s in (2, 4)}
    return dict(configs=configs, default_state=default_state, unshuffle=dict(ramp=ramp, out=unshuffle))


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "rrdb_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        print(f"  {rec['name']}: y {tuple(rec['y'].shape)} std {float(rec['y'].std()):.3f}, conv output std {rec['conv_std_min']:.3f} .. "
              f"{rec['conv_std_max']:.3f}, rel_l2(y_bf16, y) {rel_l2(rec['y_bf16'], rec['y']):.3e}")


if __name__ == "__main__":
    main()
