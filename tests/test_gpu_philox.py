"""Every Philox-drawing kernel against the host Philox4x32-10 reference (tests/philox_ref.py, itself pinned to the
Random123 known-answer vectors by test_philox_host.py): the dropout and DropPath masks and values, the attention-dropout
mask, the normals, and the counters each stochastic call consumes.  Masks are compared with `torch.equal`; values given
the mask are compared with the torch CPU expression the kernels' headers promise; normals per element against float64.
Outputs are guarded allocations, floating inputs are poisoned (`G`, as in test_gpu_kernel_edges.py).  Sizes sit at the
4-wide loops' tails and just past each grid-stride loop's first pass; seeds and offsets exercise the key's and the
counter's high words and the carry between the counter's words."""
import numpy as np
import pytest
import torch

import philox_ref as R
from helpers import assert_elementwise, guarded_ops
from philox_ref import ONES_WORDS, SEED, ZERO_WORDS, ZERO_WORDS_A

pytestmark = pytest.mark.gpu

from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd import ops  # noqa: E402
from cflearn_amd.modules import GaussianDistribution  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
OFFSETS = [0, 7, 2 ** 32 - 2, 2 ** 40 + 5]  # 2^32 - 2: the counter carries into its high word inside the tensor
STREAMS = [(s, o) for s in (SEED, 0) for o in OFFSETS]
ONE_STREAM = [(SEED, 2 ** 32 - 2)]  # the large tensors: the carry, a key with a high word
DROPOUT_GROUPS = 4096 * 256  # groups of 4 elements one pass of random.hip's stride loops covers
RANDN_GROUPS = 2048 * 256    # the same of sample.hip's
DROPOUT_P = [0.0, 0.25, 0.3, 0.6, 0.9, 0.999]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _x(n, seed, dtype):
    """finite, non-zero values of both signs"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3.0
    x = torch.where(x.abs() < 0.01, torch.full_like(x, 0.5), x)
    return x.to(dtype)


def _dropout_want(x, keep, p):
    """torch's dropout given the mask: the noise `mask / (1 - p)` is formed in x's dtype (1 - p in double, as Python does)"""
    return x * (keep.to(x.dtype) / (1 - p))


@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 63, 65, 257, 4 * DROPOUT_GROUPS + 5])
def test_dropout_mask_is_the_host_stream_and_values_are_torchs(G, n, p):
    """mask_out == the host keep mask (element i: word i % 4 of counter offset + i // 4, keep iff u >= f32(p)), and y equals
    torch's `x * (mask.to(x.dtype) / (1 - p))` evaluated on the CPU in x's dtype, f32 and bf16 (`torch.equal`: the sign of a
    dropped negative element's zero is not compared).  mask_out is a guarded allocation: a 4-byte mask store past an odd
    tail fails the guard check.  At the tail sizes the same y results with the mask injected.  The last n is a second pass
    of the stride loop and a scalar tail."""
    for seed, off in (STREAMS if n < 1000 else ONE_STREAM):
        keep = torch.from_numpy(R.dropout_keep(n, p, seed, off))
        if p == 0.0:
            assert bool(keep.all())
        for dtype in (F32, BF16):
            x = _x(n, n + 1, dtype)
            y, m = ops.dropout(G.poisoned(x.to(DEV)), p, seed=seed, offset=off, want_mask=True)
            assert m.dtype == torch.uint8 and torch.equal(m.cpu(), keep), (n, p, hex(seed), off, dtype)
            want = _dropout_want(x, keep, p)
            assert want.dtype == dtype
            bad = (y.cpu() != want)
            assert not bool(bad.any()), (n, p, dtype, int(bad.sum()), y.cpu()[bad][:4].tolist(), want[bad][:4].tolist())
            if n < 1000:
                yi, _ = ops.dropout(G.poisoned(x.to(DEV)), p, mask=G.index(keep.to(DEV)))
                assert torch.equal(yi.cpu(), want), (n, p, dtype)
        G.check()


def test_dropout_at_the_edge_words():
    """offset = an edge counter, n = 4: a word with u = 0 is dropped for every p > 0 and kept at p = 0 (the comparison is
    `>=`); a word with u = 1 - 2^-24 is kept at p = 0.999"""
    x = torch.ones(4, device=DEV)
    for c, w in ZERO_WORDS + ZERO_WORDS_A:
        for p in DROPOUT_P:
            _, m = ops.dropout(x, p, seed=SEED, offset=c, want_mask=True)
            assert torch.equal(m.cpu(), torch.from_numpy(R.dropout_keep(4, p, SEED, c)))
            assert int(m[w]) == (1 if p == 0.0 else 0), (c, w, p)
    for c, w in ONES_WORDS:
        _, m = ops.dropout(x, 0.999, seed=SEED, offset=c, want_mask=True)
        assert torch.equal(m.cpu(), torch.from_numpy(R.dropout_keep(4, 0.999, SEED, c))) and int(m[w]) == 1, (c, w)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 255, 257])
def test_drop_path_mask_is_the_host_stream(G, B):
    """sample b: floor(f32(keep_prob) + u) with u from word b % 4 of counter offset + b // 4"""
    for keep_prob in (1.0, 0.8, 0.5, 0.05):
        for seed, off in STREAMS:
            m = ops.drop_path_mask(B, keep_prob, DEV, seed=seed, offset=off)
            assert m.dtype == F32 and torch.equal(m.cpu(), torch.from_numpy(R.drop_path_mask(B, keep_prob, seed, off))), \
                (B, keep_prob, hex(seed), off)
        G.check()
    # the zero word: floor(keep_prob + 0) = 0 for every keep_prob < 1; the all-ones word: floor(0.05 + (1 - 2^-24)) = 1
    c, w = ZERO_WORDS[0]
    assert ops.drop_path_mask(4, 0.8, DEV, seed=SEED, offset=c)[w].item() == 0.0
    c, w = ONES_WORDS[0]
    assert ops.drop_path_mask(4, 0.05, DEV, seed=SEED, offset=c)[w].item() == 1.0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,inner", [(1, 4), (3, 8), (5, 260), (5, 4 * (2 ** 18 + 1))])
def test_drop_path_values_are_torchs(G, B, inner, dtype):
    """y == the CPU `x.div(keep_prob) * mask.view(-1, 1)` in x's dtype (true division, then the 0 / 1 product), with masks
    that hold both values; the last shape has more groups of 4 than one pass of the stride loop covers"""
    x = _x(B * inner, B + inner, dtype).view(B, inner)
    pattern = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0])[:B]
    masks = [pattern, 1.0 - pattern] if inner < 1000 else [pattern]
    for keep_prob in ((0.8, 0.5, 0.05) if inner < 1000 else (0.8,)):
        for mask in masks:
            y = ops.drop_path(G.poisoned(x.to(DEV)), G.poisoned(mask.to(DEV)), keep_prob)
            want = x.div(keep_prob) * mask.to(dtype).view(-1, 1)
            assert y.dtype == dtype and torch.equal(y.cpu(), want), (B, inner, dtype, keep_prob, mask.tolist())
    G.check()


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 41, 50), (2, 3, 419, 421)])
def test_attn_dropout_mask_is_the_host_stream(G, shape):
    """entry (b, h, i, j): byte j % 4 of word i % 4 of counter offset + ((b H + h) ceil(Tq / 4) + i // 4) ceil(Tk / 4) + j // 4,
    kept iff byte >= thresh = clamp(round(256 p), 1, 255).  The attention kernels are compared with this export per element
    (test_gpu_attn*.py), so this pins them too.  The last shape has more than 4096 x 256 elements: the stride loop's
    second pass."""
    B, H, Tq, Tk = shape
    big = B * H * Tq * Tk > 4096 * 256
    assert big == (shape == (2, 3, 419, 421))
    for p in (0.001, 0.1, 0.25, 0.5, 0.999):
        thresh = R.attn_thresh(p)
        assert ops.attn_dropout_p(p) == thresh / 256 and 1 - ops.attn_dropout_p(p) == 1 - thresh / 256
        for seed, off in (ONE_STREAM + [(0, 7)] if big else STREAMS):
            m = ops.attn_dropout_mask(B, H, Tq, Tk, p, seed, off, DEV)
            assert m.dtype == torch.uint8 and tuple(m.shape) == shape
            assert torch.equal(m.cpu(), torch.from_numpy(R.attn_keep(B, H, Tq, Tk, p, seed, off))), (shape, p, hex(seed), off)
        G.check()
    assert [R.attn_thresh(p) for p in (0.001, 0.999)] == [1, 255]  # both clamps were in the list


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1025, 4 * RANDN_GROUPS + 6])
def test_randn_is_box_muller_on_the_host_stream(G, n):
    """Every element: |z - z64| <= ulp_f32(|z64|) + 8 * 2^-24 * rad, z64 the float64 Box-Muller of the host words (pairs
    (w0, w1) and (w2, w3), u = ((w >> 8) + 1) 2^-24, z = rad (cos, sin)(2 pi u_b), rad = sqrt(-2 ln u_a)).  The 8 units are
    the allowance for a short chain of library transcendentals (log, sqrt, sincospi and two products);
    test_philox_host.py shows a plain f32 evaluation stays inside it.  This detects exchanged words or pairs, exchanged
    sine and cosine, an interval closed at 0 and a wrong counter.  It does NOT detect a shift of u_b by one unit of 2^-24:
    that moves z by 2 pi 2^-24 rad, less than the bound.  The last n is the stride loop's second pass and a tail of 2."""
    for seed, off in (STREAMS if n < 10000 else ONE_STREAM):
        z64, rad = R.normals64(n, seed, off)
        z = ops.randn(n, seed, off, DEV)
        assert z.dtype == F32 and tuple(z.shape) == (n,)
        assert_elementwise(z, torch.from_numpy(z64), out_dtype=F32, ulps=1, cond=torch.from_numpy(rad), k=8,
                           what=f"randn n={n} seed={seed:#x} offset={off}")
    G.check()


def test_randn_at_the_edge_words(G):
    """offset = an edge counter, n = 4: finite everywhere (u_a = 2^-24 is the largest radius, u is never 0); a pair with
    u_a = 1 is exactly (+-0, +-0); a pair with u_b = 1 has the sine component exactly +-0 and the cosine component equal
    to the radius (within the bound of the test above, against the float64 radius)"""
    for c, w in ZERO_WORDS + ZERO_WORDS_A + ONES_WORDS:
        z = ops.randn(4, SEED, c, DEV).cpu()
        z64, rad = R.normals64(4, SEED, c)
        assert bool(torch.isfinite(z).all()), (c, w, z.tolist())
        assert_elementwise(z, torch.from_numpy(z64), out_dtype=F32, ulps=1, cond=torch.from_numpy(rad), k=8, what=f"edge {c}")
        if (c, w) in ONES_WORDS and w % 2 == 0:
            assert z[w].item() == 0.0 and z[w + 1].item() == 0.0, (c, w, z.tolist())
        if (c, w) in ONES_WORDS and w % 2 == 1:
            assert z[w].item() == 0.0 and z[w - 1].item() > 0.0, (c, w, z.tolist())
            assert_elementwise(z[w - 1], torch.tensor(rad[w]), out_dtype=F32, ulps=1, cond=torch.tensor(rad[w]), k=8, what=f"rad {c}")
    c, w = ZERO_WORDS_A[0]
    assert abs(ops.randn(4, SEED, c, DEV).cpu()[w:w + 2].double().norm().item() - np.sqrt(-2.0 * np.log(2.0 ** -24))) < 1e-5


def test_stream_accounting_of_the_stochastic_calls():
    """what each call takes from `ops.PhiloxState`: dropout ceil(n / 4) counters, DropPath ceil(B / 4), the posterior's
    draw ceil(latent elements / 4) — and that the masks are the host stream's at those offsets"""
    saved = ops.PhiloxState.seed, ops.PhiloxState.offset
    try:
        s = SEED
        ops.PhiloxState.manual_seed(s)
        assert (ops.PhiloxState.seed, ops.PhiloxState.offset) == (s, 0)
        y5 = HF.dropout(torch.ones(5, device=DEV), 0.3, True)
        assert ops.PhiloxState.offset == 2
        y8 = HF.dropout(torch.ones(8, device=DEV), 0.6, True)
        assert ops.PhiloxState.offset == 4
        assert torch.equal((y5 != 0).cpu(), torch.from_numpy(R.dropout_keep(5, 0.3, s, 0)).bool())
        assert torch.equal((y8 != 0).cpu(), torch.from_numpy(R.dropout_keep(8, 0.6, s, 2)).bool())
        yb = HF.drop_path(torch.ones(5, 4, device=DEV), 0.5, True)
        assert ops.PhiloxState.offset == 6
        want = torch.from_numpy(R.drop_path_mask(5, 0.5, s, 4))
        assert set(want.tolist()) == {0.0, 1.0}  # this seed draws both
        assert torch.equal(yb.cpu(), torch.ones(5, 4).div(0.5) * want.view(-1, 1))
        moments = (torch.randn(2, 6, 3, 5, generator=torch.Generator().manual_seed(0)) * 0.5).to(BF16).to(DEV)
        dist = GaussianDistribution(moments)
        z = dist.sample()
        numel = moments.numel()
        assert numel // 2 == z.numel() == 90 and ops.PhiloxState.offset == 6 + (numel // 2 + 3) // 4 == 29
        assert torch.equal(z, dist.sample(seed=s, offset=6)) and ops.PhiloxState.offset == 29  # an explicit pair takes nothing
        # the draw itself: z = mean + exp(0.5 log_var) * n with n the host stream's normals at offset 6
        n64, rad = R.normals64(90, s, 6)
        mean, lv = moments.double().cpu()[:, :3].reshape(-1), moments.double().cpu()[:, 3:].reshape(-1)
        std = torch.exp(0.5 * lv)
        want_z = mean + std * torch.from_numpy(n64)
        # one exp (library), one product and one sum on top of the normal's own 8 units
        cond = mean.abs() + std * (torch.from_numpy(rad) + torch.from_numpy(n64).abs() * (1 + lv.abs()))
        assert_elementwise(z.reshape(-1), want_z, out_dtype=F32, ulps=1, cond=cond, k=12, what="posterior draw")
    finally:
        ops.PhiloxState.seed, ops.PhiloxState.offset = saved
