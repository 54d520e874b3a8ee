"""The parameters of tests/golden/rrdb_small.pt, rebuilt instead of stored (the pattern of tests/controlnet_weights.py, whose integer
hash this reuses).

Both the generator (tools/gen_rrdb_golden.py, on the reference's RRDBNet) and the tests (on this package's) fill a model with
`fill_parameters(model, seed)`: every value is an integer code in [-127, 127] from a hash of (seed, tensor index, element index) times
a power of two, the same bits on every machine and exact in bf16.
  * filters: code * 2^k, 2^k the power of two nearest GAIN / (73.3 sqrt(fan_in)) (73.3: the standard deviation of the codes), so a
    convolution's output has about GAIN times the RMS of its input.  With torch's default initialisation (0.58 / sqrt(fan_in)) the
    LeakyReLU chain decays, the whole net's output has amplitude 0.07 and the residual path hides every convolution; GAIN = 1.2 keeps
    every convolution's output between 0.25 and 4 (asserted by the generator with forward hooks on the reference).
  * biases: code / 512."""
import math

import torch

from controlnet_weights import hashed_codes

GAIN = 1.2
CODE_STD = 73.3


def fill_parameters(model: torch.nn.Module, seed: int) -> None:
    with torch.no_grad():
        for index, (name, p) in enumerate(model.named_parameters()):
            codes = hashed_codes(p.numel(), seed * 1000003 + index).view(p.shape)
            if p.dim() >= 2:
                fan_in = p[0].numel()
                value = codes.float() * 2.0 ** round(math.log2(GAIN / (CODE_STD * math.sqrt(fan_in))))
            else:
                value = codes.float() / 512.0
            assert torch.equal(value.to(torch.bfloat16).float(), value), name
            p.copy_(value)


def seeded_state(model: torch.nn.Module, seed: int) -> dict:
    """a state dict of fresh tensors holding what `fill_parameters(model, seed)` writes (the model itself is left as it is)"""
    import copy

    clone = copy.deepcopy(model).cpu()
    fill_parameters(clone, seed)
    return {k: v.clone() for k, v in clone.state_dict().items()}
