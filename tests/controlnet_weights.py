"""The parameters of tests/golden/controlnet_small.pt, rebuilt instead of stored.

The two models of that fixture have 2.9 M parameters; the file holds what the reference computed from them, not the parameters.
Both the generator (tools/gen_controlnet_golden.py, on the reference's models) and the tests (on this package's) fill a model with
`fill_parameters(model, seed)`: every value comes from an integer hash of (seed, tensor index, element index) in exact int64
arithmetic, scaled by a power of two — the same bits on every machine and torch version, and exact in bf16.
  * matrices / filters: code * 2^k, code in [-127, 127], 2^k the power of two nearest 1 / (128 sqrt(fan_in)) (the standard deviation
    of torch's default initialisation, 0.58 / sqrt(fan_in));
  * the gains of GroupNorm / LayerNorm (1-D `weight`): 1 + (code // 8) / 64, in [0.75, 1.25];
  * biases: code / 2048.
Nothing stays at zero: the zero-initialised convolutions of the reference get values like every other, so gradients reach every layer."""
import math

import torch

_M32 = 0xFFFFFFFF


def hashed_codes_raw(n: int, seed: int) -> torch.Tensor:
    """int64 [n] in [0, 2^32): the murmur3 finaliser of (element index * golden ratio + seed), 32-bit arithmetic inside int64"""
    x = (torch.arange(n, dtype=torch.int64) * 0x9E3779B1 + (seed * 0x85EBCA77 & _M32)) & _M32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    x = x ^ (x >> 16)
    return x


def hashed_codes(n: int, seed: int) -> torch.Tensor:
    """int64 [n] in [-127, 127] out of `hashed_codes_raw`"""
    return hashed_codes_raw(n, seed) % 255 - 127


def fill_parameters(model: torch.nn.Module, seed: int) -> None:
    with torch.no_grad():
        for index, (name, p) in enumerate(model.named_parameters()):
            codes = hashed_codes(p.numel(), seed * 1000003 + index).view(p.shape)
            if p.dim() >= 2:
                fan_in = p[0].numel()
                value = codes.float() * 2.0 ** round(math.log2(1.0 / (128.0 * math.sqrt(fan_in))))
            elif name.endswith("weight"):
                value = 1.0 + torch.div(codes, 8, rounding_mode="floor").float() / 64.0
            else:
                value = codes.float() / 2048.0
            assert torch.equal(value.to(torch.bfloat16).float(), value), name
            p.copy_(value)


def sample_gradient(g: torch.Tensor, limit: int = 1024) -> torch.Tensor:
    """what the fixture keeps of one parameter's gradient: all of it up to `limit` elements, else the elements at `limit` hashed
    flat positions (the integer hash above, modulo the size).  Hashed, not strided: a stride shares factors with the 3 x 3 taps and
    the channel counts and would visit one tap of a filter only; these positions fall on every tap, row and column."""
    flat = g.reshape(-1)
    if flat.numel() <= limit:
        return flat.clone()
    pos = (hashed_codes_raw(limit, flat.numel() * 31 + 7) % flat.numel()).sort().values
    return flat[pos].clone()
