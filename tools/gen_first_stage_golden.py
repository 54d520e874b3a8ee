"""Generate the fixtures of the KL-autoencoder first stage from the reference's own classes on the CPU:

    python tools/gen_first_stage_golden.py

  tests/golden/ae_kl_keys.pt          state-dict names and shapes of a small `ae_kl` (names and shapes only)
  tests/golden/spatial_attention.pt   `SpatialAttention` (attentions.py:330-370) at C = 64 and C = 256 on 6x5 pixels: input, output;
                                      at C = 64 also the output gradient fed in and the gradients of the input and of every parameter
  tests/golden/ae_kl_small.pt         `ae_kl` (cv/ae/kl.py) img 16, inner 32, multipliers (1, 2), one residual block per level,
                                      attention_resolutions (8,), embedding 4, latent 4: input [2, 3, 16, 16], the moments, decode(mode)
  tests/golden/ae_kl_wide_outputs.pt  the same with inner 32, multipliers (1, 16) on 8x8 images: a 512-wide bottleneck attention

Needs the reference tree (oracle/refharness finds it); writes data only.  No fixture stores parameters: every model is filled, in
the sorted order of its state-dict names, from `torch.Generator().manual_seed(seed)` on the CPU by `seeded_state` below, which the
tests repeat line for line (25 M parameters of the wide model would be 100 MB).  Every result is stored twice: the fp32 run
(`*`), and the reference's own run under `torch.autocast("cpu", dtype=torch.bfloat16)` (`*_bf16`) — the yardstick: the HIP path's
distance from the fp32 result is held against the reference's own bf16 distance from it.  Single-threaded and seeded: a second
run writes the same values.  `generate()` returns the fixtures in memory (tests/test_first_stage_host.py compares them with the
committed files)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = dict(img_size=16, in_channels=3, out_channels=3, inner_channels=32, latent_channels=4, channel_multipliers=(1, 2),
             embedding_channels=4, num_res_blocks=1, attention_resolutions=(8,))
WIDE = dict(img_size=8, in_channels=3, out_channels=3, inner_channels=32, latent_channels=4, channel_multipliers=(1, 16),
            embedding_channels=4, num_res_blocks=1, attention_resolutions=())
SEEDS = dict(attn64=6401, attn256=25601, small=1601, wide=801)


def seeded_state(shapes, seed):
    """{name: tensor} for {name: shape}: 1-D `weight`s (the norms' gains) 1 + 0.1 n, other 1-D tensors 0.1 n, filters n / sqrt(fan_in),
    drawn in the sorted order of the names from one CPU generator"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        n = torch.randn(shape, generator=g)
        if len(shape) == 1:
            out[name] = 1.0 + 0.1 * n if name.endswith("weight") else 0.1 * n
        else:
            out[name] = n / float(torch.Size(shape[1:]).numel()) ** 0.5
    return out


def _fill(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(seeded_state(shapes, seed), strict=True)
    return shapes


def _both(run):
    """(fp32 result, the reference's bf16-autocast result as f32) of `run()`, each a tuple of tensors"""
    full = run()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        low = run()
    return tuple(t.detach().float().clone() for t in full), tuple(t.detach().float().clone() for t in low)


def spatial_attention_fixture(cf):
    import importlib

    att = importlib.import_module("cflearn.modules.core.attentions")
    out = {}
    for c in (64, 256):
        m = att.SpatialAttention(c)
        _fill(m, SEEDS[f"attn{c}"])
        m.eval()
        g = torch.Generator().manual_seed(SEEDS[f"attn{c}"] + 1)
        x = torch.randn((2, c, 6, 5), generator=g)
        gy = torch.randn((2, c, 6, 5), generator=g)
        names = [n for n, _ in m.named_parameters()]

        def run():
            m.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(c == 64)
            y = m(xi)
            if c != 64:
                return (y,)
            y.float().backward(gy)
            return (y, xi.grad) + tuple(p.grad for _, p in m.named_parameters())

        full, low = _both(run)
        rec = dict(x=x, y=full[0], y_bf16=low[0])
        if c == 64:
            rec.update(gy=gy, gx=full[1], gx_bf16=low[1], grads=dict(zip(names, full[2:])), grads_bf16=dict(zip(names, low[2:])))
        out[c] = rec
    return out


def ae_fixture(cf, cfg, seed):
    import importlib

    kl = importlib.import_module("cflearn.modules.cv.ae.kl")
    common = importlib.import_module("cflearn.modules.cv.common")
    m = kl.AttentionAutoEncoderKL(**cfg)
    shapes = _fill(m, seed)
    m.eval()
    size = cfg["img_size"]
    x = torch.randn((2, 3, size, size), generator=torch.Generator().manual_seed(seed + 1))

    def run():
        with torch.no_grad():
            dist = m.encode(x)
            return dist.net, m.decode(common.DecoderInputs(z=dist.mode()))

    full, low = _both(run)
    rec = dict(cfg=dict(cfg), seed=seed, x=x, moments=full[0], decoded=full[1], moments_bf16=low[0], decoded_bf16=low[1])
    return rec, shapes


def generate():
    torch.set_num_threads(1)
    cf = import_cflearn()
    small, shapes = ae_fixture(cf, SMALL, SEEDS["small"])
    wide, _ = ae_fixture(cf, WIDE, SEEDS["wide"])
    keys = dict(cfg=dict(SMALL), keys=[(k, tuple(v)) for k, v in shapes.items()])
    return {"ae_kl_keys.pt": keys, "spatial_attention.pt": spatial_attention_fixture(cf), "ae_kl_small.pt": small,
            "ae_kl_wide_outputs.pt": wide}


def main() -> None:
    for name, data in generate().items():
        path = os.path.join(GOLDEN, name)
        torch.save(data, path)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
