"""Generate tests/golden/controlnet_small.pt: the reference's own `ControlNet` and `UNetDiffuser`
(modules/multimodal/diffusion/unet.py) on the CPU in fp32 at one tiny configuration.

    python tools/gen_controlnet_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * cfg / unet_cfg: the constructor keywords of the two models (start_channels 64, multipliers (1, 2), one ResBlock per level,
    spatial transformers at both rates, 4 heads, context_dim 16, 3 hint channels, 4 latent channels), B = 2, latent 8x8, hint 64x64.
    64 start channels, not 32: GroupNorm(32) over 32 channels normalises every channel on its own, which cancels the bias of the
    convolution and the time projection in front of it exactly — their gradients would be rounding noise (1e-10 here);
  * control_seed / unet_seed: the parameters are not stored (2.9 M values; a committed file is limited to 1 MiB): both models are
    filled by tests/controlnet_weights.fill_parameters(model, seed), an exact integer hash on a bf16 grid that the tests repeat on
    this package's models.  Nothing stays zero, so gradients reach every layer.  control_keys / unet_keys: (key, shape) of both
    state dicts in registration order; zoo_cfg / zoo_keys: the same list for the zoo configuration (start_channels 320,
    multipliers (1, 2, 4, 8), built on the meta device);
  * x_t, hint, timesteps, context, noise, scales (not all 1): the inputs, as DDPM.denoise feeds them (ddpm.py:412-419, 457-459);
  * control: the control list after the scales; y: the UNet output with that list; loss: mean-squared error against `noise`;
  * grads: d (loss_scale * loss) / d p for every ControlNet parameter p, through controlnet_weights.sample_gradient (a tensor of
    more than 1024 elements keeps 1024 hashed positions, which fall on every tap, row and column: the size limit again); loss_scale: the factor (a power of two, 1 when none is
    needed) that lifts the smallest gradient's max |g| to at least 50 x the absolute floor of the test's comparison (2e-4).
Single-threaded and seeded: a second run writes the same bytes."""
import importlib
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from controlnet_weights import fill_parameters, sample_gradient  # noqa: E402
from refharness import import_cflearn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "controlnet_small.pt")
COMMON = dict(num_heads=4, use_spatial_transformer=True, context_dim=16, start_channels=64, num_res_blocks=1,
              attention_downsample_rates=(1, 2), channel_multipliers=(1, 2))
B, LATENT, HINT_CHANNELS, IN_CHANNELS, CONTEXT_LEN = 2, 8, 3, 4, 5
ABS_FLOOR, LIFT = 2.0e-4, 50.0
CONTROL_SEED, UNET_SEED = 11, 12


def main() -> None:
    torch.set_num_threads(1)
    import_cflearn()
    unet_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.unet")
    torch.manual_seed(7301)
    control_net = unet_mod.ControlNet(IN_CHANNELS, HINT_CHANNELS, **COMMON)
    unet = unet_mod.UNetDiffuser(IN_CHANNELS, IN_CHANNELS, **COMMON)
    fill_parameters(control_net, CONTROL_SEED)
    fill_parameters(unet, UNET_SEED)
    gen = torch.Generator().manual_seed(7302)
    x_t = torch.randn((B, IN_CHANNELS, LATENT, LATENT), generator=gen)
    hint = torch.rand((B, HINT_CHANNELS, 8 * LATENT, 8 * LATENT), generator=gen)
    timesteps = torch.tensor([37, 811], dtype=torch.int64)
    context = torch.randn((B, CONTEXT_LEN, COMMON["context_dim"]), generator=gen)
    noise = torch.randn((B, IN_CHANNELS, LATENT, LATENT), generator=gen)
    n_out = len(control_net.zero_convs) + 1
    scales = [1.0, 0.75, 1.25, 0.5, 1.5][:n_out]
    assert len(scales) == n_out and any(s != 1.0 for s in scales)
    unet.requires_grad_(False)

    def run(loss_scale: float):
        control_net.zero_grad()
        ctrl = control_net(x_t, hint, timesteps=timesteps, context=context)
        ctrl = [c * s for c, s in zip(ctrl, scales)]  # ddpm.py:419
        recorded = [c.detach().clone() for c in ctrl]
        y = unet(x_t, timesteps=timesteps, context=context, control=ctrl, only_mid_control=False)  # (pops the list)
        loss = F.mse_loss(y, noise)
        (loss * loss_scale).backward()
        return recorded, y.detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in control_net.named_parameters()}

    loss_scale = 1.0
    while True:
        control, y, loss, grads = run(loss_scale)
        weakest = min(float(g.abs().max()) for g in grads.values())
        if weakest >= LIFT * ABS_FLOOR:
            break
        assert weakest > 0.0, "a ControlNet parameter gets no gradient at all"
        loss_scale *= 2.0
    for k, g in grads.items():
        assert float(g.abs().max()) >= LIFT * ABS_FLOOR, k
    assert all(p.grad is None for p in unet.parameters())
    zoo_cfg = dict(in_channels=4, hint_channels=3, num_heads=8, use_spatial_transformer=True, context_dim=768)
    with torch.device("meta"):
        zoo = unet_mod.ControlNet(**zoo_cfg)
    out = dict(zoo_cfg=zoo_cfg, zoo_keys=[(k, tuple(v.shape)) for k, v in zoo.state_dict().items()],
               cfg=dict(in_channels=IN_CHANNELS, hint_channels=HINT_CHANNELS, **COMMON),
               unet_cfg=dict(in_channels=IN_CHANNELS, out_channels=IN_CHANNELS, **COMMON),
               control_seed=CONTROL_SEED, unet_seed=UNET_SEED,
               control_keys=[(k, tuple(v.shape)) for k, v in control_net.state_dict().items()],
               unet_keys=[(k, tuple(v.shape)) for k, v in unet.state_dict().items()],
               x_t=x_t, hint=hint, timesteps=timesteps, context=context, noise=noise, scales=scales,
               control=control, y=y, loss=loss, grads={k: sample_gradient(g) for k, g in grads.items()}, loss_scale=loss_scale)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); loss {loss.item():.6f}, loss_scale {loss_scale}, "
          f"weakest gradient max |g| {weakest:.3e}")


if __name__ == "__main__":
    main()
