"""The parameters of tests/golden/pixelcnn_small.pt, rebuilt instead of stored (the convention of tests/rnn_weights.py, on the integer
hash of tests/controlnet_weights.py).

Both the generator (tools/gen_pixelcnn_golden.py, on the reference's PixelCNN) and the tests (on this package's) fill a model with
`fill_parameters(model, seed)`: every value is an integer code in [-127, 127] from a hash of (seed, tensor index, element index) times
a power of two, the same bits on every machine and exact in bf16.
  * filters, matrices, the embedding table and the channel-padding token: code * 2^k, 2^k the power of two nearest
    GAIN / (73.3 sqrt(fan_in)) (73.3: the standard deviation of the codes; fan_in = the elements of one output's filter).  Half of a
    masked filter is zeroed by its first forward, so GAIN = 2 keeps the activations at a few tenths through the stack;
  * BatchNorm: weight 1 + code / 256, bias code / 256, and NON-TRIVIAL running statistics (they are buffers, filled here too):
    running_mean code / 512, running_var 1 + code / 256 in [0.5, 1.5];
  * other biases: code / 256.
`mask` and `num_batches_tracked` are left as the constructor made them."""
import math

import torch

from controlnet_weights import hashed_codes, hashed_codes_raw

GAIN = 2.0
CODE_STD = 73.3
GRAD_LIMIT = 1024


def fill_parameters(model: torch.nn.Module, seed: int) -> None:
    bn_weights = {name + ".weight" for name, m in model.named_modules() if hasattr(m, "running_mean")}
    with torch.no_grad():
        tensors = list(model.named_parameters()) + [(n, b) for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))]
        for index, (name, p) in enumerate(tensors):
            codes = hashed_codes(p.numel(), seed * 1000003 + index).view(p.shape).to(p.dtype)
            if name.endswith("running_mean"):
                value = codes / 512.0
            elif name.endswith("running_var") or name in bn_weights:
                value = 1.0 + codes / 256.0
            elif p.dim() >= 2:
                value = codes * 2.0 ** round(math.log2(GAIN / (CODE_STD * math.sqrt(p[0].numel()))))
            else:
                value = codes / 256.0
            p.copy_(value)


def seeded_state(model: torch.nn.Module, seed: int) -> dict:
    """a state dict of fresh tensors holding what `fill_parameters(model, seed)` writes (the model itself is left as it is)"""
    import copy

    clone = copy.deepcopy(model).cpu()
    fill_parameters(clone, seed)
    return {k: v.clone() for k, v in clone.state_dict().items()}


def grad_positions(numel: int) -> torch.Tensor:
    """the flat positions of a gradient that the fixture keeps: all of them up to GRAD_LIMIT elements, else the distinct ones among
    GRAD_LIMIT hashed positions (hashed, not strided: a stride shares factors with the 7 x 7 taps and the channel counts), sorted"""
    if numel <= GRAD_LIMIT:
        return torch.arange(numel)
    return torch.unique(hashed_codes_raw(GRAD_LIMIT, numel * 31 + 7) % numel)
