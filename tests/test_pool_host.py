"""Head poolers "mean" / "sequence" of MixedStackedEncoder, host side: module tree against the reference's recorded key names
(tests/golden/head_poolers.pt, tools/gen_pool_golden.py), what stays refused, and the argument checks of cfhip_pool_rows_*."""
import inspect
import os

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib
from cflearn_amd import functional as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = torch.load(os.path.join(ROOT, "tests", "golden", "head_poolers.pt"), map_location="cpu", weights_only=False)
POSITIONS = {"pre": {}, "after": dict(norm_after_head=True), "none": dict(no_head_norm=True)}


@pytest.mark.parametrize("pooler", ["mean", "sequence"])
@pytest.mark.parametrize("position", list(POSITIONS))
def test_constructor_builds_the_reference_tree(pooler, position):
    net = C.MixedStackedEncoder(**FX["kwargs"], head_pooler=pooler, **POSITIONS[position])
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("head")]
    assert got == FX["keys"][f"{pooler}/{position}"]
    if pooler == "sequence":
        proj = [m for m in net.modules() if isinstance(m, C.modules.SequencePooler)][0].projection.linear
        # `_init_weights`: trunc_normal_(std=0.02) and a zero bias (the Linear's own xavier init would give std 0.124 here)
        assert float(proj.weight.detach().std()) < 0.04 and float(proj.bias.detach().abs().max()) == 0.0


@pytest.mark.parametrize("pooler", ["mean", "sequence"])
def test_reference_checkpoint_loads_strictly(pooler):
    net = C.MixedStackedEncoder(**FX["kwargs"], head_pooler=pooler)
    net.load_state_dict({**FX["stack_sd"], **FX["modules"][pooler]["sd"]}, strict=True)


def test_what_stays_refused():
    kw = FX["kwargs"]
    with pytest.raises(NotImplementedError, match="tanh"):
        C.MixedStackedEncoder(**kw, head_pooler="bert")
    with pytest.raises(NotImplementedError, match="aux heads"):
        C.MixedStackedEncoder(**kw, head_pooler="sequence", aux_heads=["a"])
    with pytest.raises(ValueError, match="unrecognized head_pooler 'max'"):
        C.MixedStackedEncoder(**kw, head_pooler="max")
    net = C.MixedStackedEncoder(**kw, head_pooler="sequence")
    net.head.module.projection.hook = object()
    with pytest.raises(NotImplementedError, match="hook"):
        net.post_process(torch.zeros(1, 10, 64))
    with pytest.raises(ValueError, match="unrecognized pool"):
        HF.pooled_layer_norm(torch.zeros(1, 2, 8), None, None, 1e-6, "max")


def test_c_entries_refuse_bad_arguments():
    """before any launch: the pointers are never dereferenced"""
    lib = _lib.load()
    p, q = 4096, 1 << 20

    def fwd(x=p, ld=8, out=q, D=8, T=4):
        return lib.cfhip_pool_rows_fwd(x, 1, ld, None, None, None, None, out, q + 4096, None, None, 2, T, D, 0, 1e-6, 0, None, 0, None)

    def bwd(x=p, D=8, dx=q):
        return lib.cfhip_pool_rows_bwd(q + 8192, None, None, x, 1, D, None, None, None, None, None, None, dx, D, None, None, None, None,
                                       0, 2, 4, D, 0, 0, None, 0, None)

    for call, text in ((lambda: fwd(D=6, ld=8), b"multiple of 4"), (lambda: fwd(D=2052, ld=2052), b"exceeds 2048"), (lambda: fwd(x=None), b"x is null"),
                       (lambda: fwd(out=p + 64), b"overlaps x"), (lambda: fwd(ld=4), b"ld_x"), (lambda: fwd(x=p + 4), b"16-byte aligned"),
                       (lambda: bwd(D=6), b"multiple of 4"), (lambda: bwd(D=2052), b"exceeds 2048"), (lambda: bwd(x=None), b"x is null"),
                       (lambda: bwd(dx=p + 32), b"dx overlaps x")):
        assert call() == -1 and text in lib.cfhip_last_error(), (text, lib.cfhip_last_error())
    assert lib.cfhip_pool_rows_workspace(2, 4, 6, 0, 0) == 0 and lib.cfhip_pool_rows_workspace(128, 196, 768, 0, 0) == 256 * 772 * 4
    assert lib.cfhip_pool_rows_workspace(128, 196, 768, 196, 0) == 0  # one chunk per sample: one launch, no workspace
    assert len(_lib.SIGNATURES) == 196


def test_layer_norm_fn_keeps_its_old_argument_lists(monkeypatch):
    """`LayerNormFn.apply(x, w, b, eps[, out_f32])` runs the LayerNorm launch it ran before (the same arguments reach ops.layernorm_fwd),
    and the new arguments are trailing and optional"""
    names = list(inspect.signature(HF.LayerNormFn.forward).parameters)
    assert names == ["ctx", "x", "weight", "bias", "eps", "out_f32", "pool", "pool_w", "pool_b"]
    seen = []

    def fake_fwd(x2, gamma, beta, eps, out_f32=False):
        seen.append((tuple(x2.shape), eps, out_f32))
        return x2 * 2, x2.new_zeros(x2.shape[0]), x2.new_ones(x2.shape[0])

    monkeypatch.setattr(HF.ops, "layernorm_fwd", fake_fwd)
    x, w, b = torch.ones(2, 3, 8), torch.ones(8), torch.zeros(8)
    assert torch.equal(HF.LayerNormFn.apply(x, w, b, 1e-6), x * 2) and torch.equal(HF.layer_norm(x, w, b, 1e-5, out_f32=True), x * 2)
    assert seen == [((6, 8), 1e-6, False), ((6, 8), 1e-5, True)]
