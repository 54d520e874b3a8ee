"""The parameters of tests/golden/rnn_small.pt, rebuilt instead of stored (the pattern of tests/rrdb_weights.py, on the integer hash of
tests/controlnet_weights.py).

Both the generator (tools/gen_rnn_golden.py, on the reference's RNN) and the tests (on this package's) fill a model with
`fill_parameters(model, seed)`: every value is an integer code in [-127, 127] from a hash of (seed, tensor index, element index) times
a power of two, the same bits on every machine.
  * matrices: code * 2^k, 2^k the power of two nearest GAIN / (73.3 sqrt(fan_in)) (73.3: the standard deviation of the codes).  With
    the reference's orthogonal initialisation the rows of a [G H, fan_in] matrix have norm sqrt(fan_in / (G H)) or 1, the gates stay
    near 1 / 2 and the hidden states have a standard deviation of 0.04 .. 0.15: the recurrent product would hardly show in the logits.
    GAIN = 1.5 puts the pre-activations at a standard deviation above 1 (the generator asserts that zeroing every weight_hh moves the
    reference's logits by rel-L2 >= 0.1).
  * biases: code / 256."""
import math

import torch

from controlnet_weights import hashed_codes

GAIN = 1.5
CODE_STD = 73.3


def fill_parameters(model: torch.nn.Module, seed: int) -> None:
    with torch.no_grad():
        for index, (name, p) in enumerate(model.named_parameters()):
            codes = hashed_codes(p.numel(), seed * 1000003 + index).view(p.shape)
            if p.dim() >= 2:
                value = codes.to(p.dtype) * 2.0 ** round(math.log2(GAIN / (CODE_STD * math.sqrt(p.shape[1]))))
            else:
                value = codes.to(p.dtype) / 256.0
            p.copy_(value)


def seeded_state(model: torch.nn.Module, seed: int) -> dict:
    """a state dict of fresh tensors holding what `fill_parameters(model, seed)` writes (the model itself is left as it is)"""
    import copy

    clone = copy.deepcopy(model).cpu()
    fill_parameters(clone, seed)
    return {k: v.clone() for k, v in clone.state_dict().items()}


def step_tensors(cell: str, seed: int, b: int = 5, f: int = 6, h: int = 8):
    """float64 tensors of one recurrent step for the replica tests: x [B, 1, F], h0 and c0 [B, H], and a seeded nn.GRU / nn.LSTM"""
    g = torch.Generator().manual_seed(seed)
    layer = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM}[cell](f, h, batch_first=True).double()
    fill_parameters(layer, seed)
    x = torch.randn(b, 1, f, generator=g, dtype=torch.float64)
    h0 = torch.randn(b, h, generator=g, dtype=torch.float64) * 0.5
    c0 = torch.randn(b, h, generator=g, dtype=torch.float64)
    return layer, x, h0, c0
