"""The float64 Adam reference of the optimizer tests (adam_ref.py) against torch.optim, and the two host recipes of the
hyper-parameter record against each other."""
import math

import pytest
import torch

import adam_ref as A

BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)]
STEPS = [1, 2, 7, 1000, 100000]


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("decoupled", [False, True])
def test_reference_follows_torch_optim(decoupled, wd):
    """Six float64 steps of torch.optim.Adam (L2 decay) / AdamW (decoupled) and of adam_ref with unrounded scalars: the two write
    the same update with differently placed roundings (lerp, sqrt(v) / sqrt(bc2), addcdiv), so they agree to a few float64
    roundings of cond per step — 64 units of 2^-53 over the six."""
    n, lr, b1, b2, eps = 257, 1e-2, 0.9, 0.999, 1e-8
    gen = torch.Generator().manual_seed(11)
    w = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = w.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 7):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        w.grad = g.clone()
        opt.step()
        h = (lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 / math.sqrt(1.0 - b2 ** t), 1.0)
        (p, cp), (m, cm), (v, cv) = A.adam_ref(p, g, m, v, h, decoupled)
        st = opt.state[w]
        for name, got, want, cond in (("p", w.detach(), p, cp), ("m", st["exp_avg"], m, cm), ("v", st["exp_avg_sq"], v, cv)):
            bad = (got - want).abs() > 64 * 2.0 ** -53 * cond
            assert not bad.any(), (name, t, int(bad.sum()), (got - want).abs().max().item())
    assert (w.detach() - p).abs().max().item() < 1e-15 and p.abs().max().item() > 1  # (and the comparison is of real values)


@pytest.mark.parametrize("betas", BETAS)
@pytest.mark.parametrize("step", STEPS)
def test_hyper_record_recipes_agree_bit_for_bit(step, betas):
    """cfhip_adam_step's scalars (double arithmetic on its double betas) and FusedAdam's record: the same eight floats, from the
    recipe in adam_ref and from a real FusedAdam on the host"""
    from cflearn_amd.optim import FusedAdam, ParamArena

    args = (3e-3, betas[0], betas[1], 1e-8, 0.05, step, 1.0 / 3.0)
    capi, fused = A.hyper_capi(*args), A.hyper_fused(*args)
    assert capi == fused, (capi, fused)
    opt = FusedAdam(None, lr=3e-3, betas=betas, eps=1e-8, weight_decay=0.05,
                    arena=ParamArena([torch.nn.Parameter(torch.zeros(8))], with_shadow=False))
    opt.grad_scale = 1.0 / 3.0
    opt.step_count = step - 1
    opt.prepare_step()
    assert opt.step_count == step
    assert torch.equal(opt._hyper_dev, capi.tensor()), (opt._hyper_dev, capi)
    # what the corrections are: those of the betas as given (torch.optim's), not of their float values
    b1, b2 = betas
    assert capi.bc1 == A.f32(1.0 - b1 ** step) and capi.bc2_rsqrt == A.f32(1.0 / math.sqrt(1.0 - b2 ** step))
