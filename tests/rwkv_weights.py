"""Parameters of the RWKV fixtures (tests/golden/rwkv_small.pt holds none): the Linear weights of the rwkv mixers drawn from a seed.

With the reference's own initialisation (zero matrices stand-alone, trunc_normal(0.02) inside MixedStackedEncoder) the mixers hardly
move their input: the reference's bf16-autocast distance of the encoder's output is 1.2e-4, no yardstick.  Standard deviation 0.1 puts
k, v and r at order one.  info_decay, the time mixes and the LayerNorm parameters keep their constructors' values."""
import torch

LINEARS = ("key.weight", "value.weight", "receptance.weight", "output.weight")
STD = 0.1


def fill_parameters(model: torch.nn.Module, seed: int, std: float = STD) -> None:
    """every `key / value / receptance / output` weight of `model`, in `named_parameters` order, from one CPU generator"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(LINEARS):
                p.copy_((torch.randn(p.shape, generator=gen) * std).to(p.device))
