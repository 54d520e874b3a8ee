"""The parameters of tests/golden/nbm_small.pt and the operands of the per-element kernel tests, rebuilt from seeds instead of stored
(the pattern of tests/rnn_weights.py, on the integer hash of tests/controlnet_weights.py).

`fill_parameters(model, seed)` (the generator tools/gen_nbm_golden.py calls it on the reference's NBM, the tests on this package's):
every value is an integer code in [-127, 127] from a hash of (seed, tensor index, element index) times a power of two.
  * matrices (conv / linear weights): code * 2^k, 2^k the power of two nearest GAIN / (73.3 sqrt(fan_in)) (73.3: the standard
    deviation of the codes; fan_in: the inputs of one output unit — `order`, H, H, num_bases, latent_dim).  The codes are symmetric, so
    about half the hidden units of either layer are live; with GAIN = 1 a ReLU layer hands on 0.7 of its input's deviation and the
    bases, features and logits come out at order 1 (the generator prints them).
  * biases: code / 256.

`kernel_case(...)`: the operands of one per-element case of the basis kernels.  x, w1, b1, w3 and dbases are small dyadic numbers
(code / 64, code / 128, code / 256, code * 2^-k, code / 128), so pre1 = u . w1 + b1 (at most 17 significant bits) and dpre2 = dbases w3
(14 bits) are EXACT in f32: the float64 replica sees the same h1 (and rounds it to the same bf16) and the same dpre2 as the kernel, and
the only differences left are f32 accumulation orders and ReLU masks of layer 2 that flip inside the forward bound."""
import math

import torch

from controlnet_weights import hashed_codes

GAIN = 1.0
CODE_STD = 73.3


def fill_parameters(model: torch.nn.Module, seed: int) -> None:
    with torch.no_grad():
        for index, (name, p) in enumerate(model.named_parameters()):
            codes = hashed_codes(p.numel(), seed * 1000003 + index).view(p.shape)
            if p.dim() >= 2:
                fan_in = p[0].numel()
                value = codes.to(p.dtype) * 2.0 ** round(math.log2(GAIN / (CODE_STD * math.sqrt(fan_in))))
            else:
                value = codes.to(p.dtype) / 256.0
            p.copy_(value)


def kernel_case(h: int, nb: int, b: int, f: int, idx, seed: int) -> dict:
    """f32 CPU operands of the basis kernels: x [B, F], idx (list of D tuples of one order o), w1 [NB, H, o], b1, b2, w3 [NB, H],
    w2 [NB, H, H], b3 [NB], dbases [B, D, NB]"""
    d, o = len(idx), len(idx[0])

    def codes(i, *shape):
        return hashed_codes(math.prod(shape), seed * 1000003 + i).view(shape).float()

    pow2 = lambda v: 2.0 ** round(math.log2(v))  # noqa: E731
    return dict(
        x=codes(0, b, f) / 64.0, idx=[tuple(t) for t in idx], w1=codes(1, nb, h, o) / 128.0, b1=codes(2, nb, h) / 256.0,
        w2=codes(3, nb, h, h) * pow2(1.5 / (CODE_STD * math.sqrt(h))), b2=codes(4, nb, h) / 256.0,
        w3=codes(5, nb, h) * pow2(1.5 / (CODE_STD * math.sqrt(h))), b3=codes(6, nb) / 256.0, dbases=codes(7, b, d, nb) / 128.0)


# the pruned cross of the per-element cases: (H, NB, B, F, idx, seed); M = B * len(idx).  Every H, NB, M and order of the issue's lists
# occurs; REPEAT has a feature in several tuples and twice in one.
REPEAT = [(0, 1), (2, 2), (1, 2), (0, 3)]
KERNEL_CASES = {
    "h8_nb1_m300_o1": (8, 1, 100, 3, [(0,), (1,), (2,)], 11),
    "h8_nb64_m1_o4": (8, 64, 1, 5, [(4, 0, 2, 1)], 12),
    "h40_nb3_m17_o2": (40, 3, 17, 4, [(3, 1)], 13),
    "h40_nb64_m65_o1": (40, 64, 13, 5, [(0,), (1,), (2,), (3,), (4,)], 14),
    "h40_nb3_m300_o2_repeat": (40, 3, 75, 4, REPEAT, 15),
    "h256_nb3_m65_o4": (256, 3, 65, 6, [(5, 0, 3, 3)], 16),
    "h256_nb1_m17_o1": (256, 1, 17, 2, [(1,)], 17),
    "h256_nb3_m300_o2_repeat": (256, 3, 75, 4, REPEAT, 18),
}
