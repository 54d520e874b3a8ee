"""Parameters of the Siren fixtures (tests/golden/siren_small.pt holds none): every parameter redrawn from a seed, in
`named_parameters` order, from one CPU generator, at the scale of the reference's own initialisation (siren.py:52-60, nn.Linear):

  blocks.0.weight / bias          uniform(+-1 / in_dim): with w_sin_initial = 30 the first sine sees arguments up to ~60 rad
  blocks.<i>.*, head.*            uniform(+-sqrt(6 / latent) / w_sin)
  modulator.*, cond_padding.mapping.*  uniform(+-1 / sqrt(fan_in))
  cond_padding.channel_padding    standard normal

The module tests therefore do not depend on the constructor's random-number order (the host test pins that separately)."""
import math

import torch


def fill_parameters(model: torch.nn.Module, seed: int, w_sin: float = 1.0) -> None:
    gen = torch.Generator().manual_seed(seed)
    bound = 1.0
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("channel_padding"):
                p.copy_(torch.randn(p.shape, generator=gen).to(p.device))
                continue
            if p.dim() >= 2:  # a bias takes the bound of the weight before it
                fan_in = p.shape[1]
                if "modulator" in name or "cond_padding" in name:
                    bound = 1.0 / math.sqrt(fan_in)
                elif name.endswith("blocks.0.weight"):
                    bound = 1.0 / fan_in
                else:
                    bound = math.sqrt(6.0 / fan_in) / w_sin
            p.copy_(((torch.rand(p.shape, generator=gen) * 2.0 - 1.0) * bound).to(p.device))
