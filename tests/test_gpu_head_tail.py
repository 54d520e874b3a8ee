"""The head-only tail of a stack's last block (fused.HEAD_ONLY, csrc/head_tail.hip, cfhip_gemm_bf16_rows) against the full last block.

A two-block pre-norm stack at D = 128 (2 heads of 64), FF = 256, read at token 0 only: with the 8th meta entry set the last
block runs its projection, FF1 + GELU, FF2 and their dX GEMMs on the B head rows only — in place in the full-size tensors, under
the tile configuration of the full launch — and every other launch (LayerNorm, attention, the weight gradients) as always, on
tensors whose skipped rows are zero.

Every output element of a GEMM is the same K-ordered accumulation whatever rows share its launch, and the launches that stay see
exact zeros where the full block has values that are multiplied by a zero gradient: the forward head rows and every gradient
whose kernel is deterministic are BIT-equal on both paths, and that is asserted.  The LayerNorm parameter gradients of this
128-wide model fold through LDS float atomics (not reproducible run to run on either path): like every tensor, they are also
measured against an fp64 torch evaluation of the same stack, and the head-only path's relative L2 error may be at most 1.1 x the
full path's.
B = 5 runs as two unequal batch slices (2 + 3), B = 3 and B = 1 as one pass.
Those cases set HEAD_ONLY_MIN_ROWS to 0 and stay below 1 024 rows (configurations 3 and 1); the regime the default threshold
leaves — 1 379-row slices at D = 256 / FF = 2 560, configurations 15 and 3 — is test_head_only_tail_in_the_regime_production_uses."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2
from test_gpu_gemm import TILE_CONFIG_NAMES, _kernel_name

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import _lib, fused, ops  # noqa: E402

DEV = "cuda"
D, HEADS, FF, EPS = 128, 2, 256, 1.0e-5
NAMES = ("ln1_w", "ln1_b", "in_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")


def _make_params(seed, d=D, ff=FF):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std  # noqa: E731
    blocks = []
    for _ in range(2):
        blocks.append([1.0 + r(d, std=0.1), r(d, std=0.1), r(3 * d, d, std=d ** -0.5), r(3 * d, std=0.1), r(d, d, std=d ** -0.5),
                       r(d, std=0.1), 1.0 + r(d, std=0.1), r(d, std=0.1), r(ff, d, std=d ** -0.5), r(ff, std=0.1),
                       r(d, ff, std=ff ** -0.5), r(d, std=0.1)])
    return blocks


def _reference(x, blocks, wgt, heads=HEADS):
    """fp64 torch: the stack (heads of 64), loss = sum(wgt * y[:, 0]); returns (y[:, 0], {name: gradient})"""
    x = x.double().requires_grad_(True)
    ps = [[p.double().to(x.device).requires_grad_(True) for p in blk] for blk in blocks]
    net = x
    b, t, d = x.shape
    assert d == 64 * heads
    for ln1_w, ln1_b, in_w, qkv_b, out_w, out_b, ln2_w, ln2_b, w1, b1, w2, b2 in ps:
        qkv = F.layer_norm(net, (d,), ln1_w, ln1_b, EPS) @ in_w.t() + qkv_b
        q, k, v = (u.view(b, t, heads, 64).transpose(1, 2) for u in qkv.split(d, dim=-1))
        att = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
        net = net + att.transpose(1, 2).reshape(b, t, d) @ out_w.t() + out_b
        net = net + F.gelu(F.layer_norm(net, (d,), ln2_w, ln2_b, EPS) @ w1.t() + b1) @ w2.t() + b2
    head = net[:, 0]
    (head * wgt.double()).sum().backward()
    grads = {"x": x.grad}
    for i, blk in enumerate(ps):
        grads.update({f"{i}.{n}": p.grad for n, p in zip(NAMES, blk)})
    return head.detach(), grads


def _run(x, blocks, wgt, words, head_only, heads=HEADS):
    x = x.clone().requires_grad_(True)
    ps = [[torch.nn.Parameter(p.to(DEV)) for p in blk] for blk in blocks]
    metas = tuple((heads, EPS, EPS, False, 0, 0, words, head_only) for _ in blocks)
    y = fused.mixing_stack(x, metas, None, False, [p for blk in ps for p in blk])
    head = y[:, 0]
    (head.float() * wgt).sum().backward()
    torch.cuda.synchronize()
    grads = {"x": x.grad}
    for i, blk in enumerate(ps):
        grads.update({f"{i}.{n}": p.grad for n, p in zip(NAMES, blk)})
    return head.detach().clone(), grads


def _slice_rows(b):
    """samples per batch slice of a stack call of batch b (fused._forward_body / _slice_cuts)"""
    n = fused.FWD_HALVES
    if n <= 1 or b < 2 * n:
        return [b]
    cuts = fused._slice_cuts(b, n)
    return [cuts[i + 1] - cuts[i] for i in range(n)]


@pytest.mark.parametrize("words", [2, 1], ids=["two_word_stream", "one_word_stream"])
@pytest.mark.parametrize("b", [1, 3, 5])
@pytest.mark.parametrize("t", [5, 33, 197])
def test_head_only_tail_matches_the_full_last_block(t, b, words, monkeypatch):
    """Measured on an MI355X: in all 18 cases the forward head rows and all 25 gradient tensors came out bit-equal, every error ratio
    against fp64 1.000; the figures are printed before they are asserted."""
    assert fused.HEAD_ONLY and fused.FWD_HALVES == 2 and fused.BWD_HALVES == 2
    monkeypatch.setattr(fused, "STACK_PLANS", False)  # (raw parameters have no gradient arena: no plan would be made anyway)
    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", 0)  # (the default leaves stacks of fewer than 1 024 rows on the full block)
    calls = []
    gemm = ops.gemm

    def counting_gemm(*a, **k):
        if k.get("config_rows"):
            calls.append((a[0].shape[0], k["config_rows"]))
        return gemm(*a, **k)

    monkeypatch.setattr(ops, "gemm", counting_gemm)
    blocks = _make_params(7)
    g = torch.Generator().manual_seed(100 * t + b)
    x = torch.randn(b, t, D, generator=g).to(DEV)
    wgt = torch.randn(b, D, generator=g).to(DEV)
    head_full, grads_full = _run(x, blocks, wgt, words, False)
    assert not calls
    head_tail, grads_tail = _run(x, blocks, wgt, words, True)
    # three forward and three dX GEMMs per batch slice, each of that slice's samples under the configuration of all its rows
    assert sorted(calls) == sorted((nb, nb * t) for nb in _slice_rows(b) for _ in range(6)), calls
    head_ref, grads_ref = _reference(x, blocks, wgt)
    assert set(grads_tail) == set(grads_full) == set(grads_ref) and len(grads_ref) == 25
    e_full, e_tail = rel_l2(head_full, head_ref), rel_l2(head_tail, head_ref)
    print(f"T={t} B={b} words={words}: forward head rows full {e_full:.3e} tail {e_tail:.3e} bit-equal: {torch.equal(head_full, head_tail)}")
    assert torch.equal(head_full, head_tail)
    bad, unequal = {}, []
    for k in grads_ref:
        assert grads_tail[k] is not None and torch.isfinite(grads_tail[k]).all(), k
        ef, et = rel_l2(grads_full[k], grads_ref[k]), rel_l2(grads_tail[k], grads_ref[k])
        same = torch.equal(grads_full[k], grads_tail[k])
        print(f"  {k:10s} full {ef:.3e} tail {et:.3e} ratio {et / max(ef, 1e-30):.3f} bit-equal: {same}")
        if et > 1.1 * ef:
            bad[k] = (et, ef)
        if not same and "ln" not in k:  # (ln1_w / ln1_b / ln2_w / ln2_b: the atomic kernel at this width)
            unequal.append(k)
    assert not bad, bad
    assert not unequal, unequal


def test_head_only_tail_in_the_regime_production_uses(monkeypatch):
    """HEAD_ONLY_MIN_ROWS at its default (1 024): D = 256 (4 heads of 64), FF = 2 560, T = 197, B = 14 = two batch slices of
    7 x 197 = 1 379 rows.  Under the default heuristic the launches of 2 560 columns (FF1 forward, FF2's GELU' dX) run the four-wave
    192x128x64 tile, configuration 15 (ceil(1379 / 192) x 20 = 160 tiles), the 256-wide ones 128x64x64, configuration 3 (16 tiles <
    160: pick_config's rule for 512 rows and more, which precedes its `b_trans -> 1`, so the two 256-wide nn launches run 3 too):
    asserted for each of the 12 launches, by kernel name and by the configuration the launch was made on (cfhip_gemm_last_config).
    Which gradients are deterministic at this width, from norm.hip: every LayerNorm backward of this stack asks for dx and the
    parameter gradients in one call (fused.SPLIT_LN_BWD is off, raw parameters do not defer the reduce) with D % 8 == 0, D <= 1 280,
    16-byte aligned dense rows and, on the two-word stream, a second output word — `fused_ok` in ln_bwd_impl — so it runs
    layernorm_bwd_fused_kernel, which folds its waves through LDS in a fixed order (no atomics), and the second batch slice
    accumulates after the first (`ln_done`).  So all 25 gradients must be bit-equal, the four LayerNorm ones included.
    Measured on an MI355X (printed before it is asserted): the forward head rows bit-equal, relative L2 error against fp64 2.991e-03
    on both paths; all 25 gradients bit-equal, their errors 1.604e-03 (1.b2) to 7.795e-03 (0.ln1_w), every tail / full ratio 1.000."""
    d, heads, ff, t, b, words = 256, 4, 2560, 197, 14, 2
    assert fused.HEAD_ONLY and fused.FWD_HALVES == 2 and fused.BWD_HALVES == 2 and fused.HEAD_ONLY_MIN_ROWS == 1024
    assert not fused.SPLIT_LN_BWD
    monkeypatch.setattr(fused, "STACK_PLANS", False)  # (raw parameters have no gradient arena: no plan would be made anyway)
    calls = []
    gemm = ops.gemm
    lay = {False: "nt", True: "nn"}

    def counting_gemm(*a, **k):
        rows = k.get("config_rows")
        if rows:
            b_trans = bool(k.get("b_trans", False))
            n, kk = (a[1].shape[1], a[1].shape[0]) if b_trans else a[1].shape
            epi = k.get("epilogue", 0)
            want = 15 if n == ff else 3
            name = _kernel_name(rows, n, kk, False, b_trans, epi)
            assert n in (d, ff) and name == f"gemm_bf16_kernel<false, {str(b_trans).lower()}, {epi}, {TILE_CONFIG_NAMES[want]}>", name
            calls.append((lay[b_trans], a[0].shape[0], rows, n, kk, epi, want))
            out = gemm(*a, **k)
            ran = _lib.load().cfhip_gemm_last_config()  # (the launch itself, on this thread: the name above is asked for a shape)
            assert ran == want, (calls[-1], ran)
            return out
        return gemm(*a, **k)

    monkeypatch.setattr(ops, "gemm", counting_gemm)
    blocks = _make_params(11, d, ff)
    g = torch.Generator().manual_seed(100 * t + b)
    x = torch.randn(b, t, d, generator=g).to(DEV)
    wgt = torch.randn(b, d, generator=g).to(DEV)
    head_full, grads_full = _run(x, blocks, wgt, words, False, heads)
    assert not calls
    head_tail, grads_tail = _run(x, blocks, wgt, words, True, heads)
    per_slice = [("nt", 7, 1379, d, d, ops.EPI_RESIDUAL, 3), ("nt", 7, 1379, ff, d, ops.EPI_GELU, 15), ("nt", 7, 1379, d, ff, ops.EPI_RESIDUAL, 3),
                 ("nn", 7, 1379, ff, d, ops.EPI_DGELU, 15), ("nn", 7, 1379, d, ff, ops.EPI_NONE, 3), ("nn", 7, 1379, d, d, ops.EPI_NONE, 3)]
    assert _slice_rows(b) == [7, 7] and sorted(calls) == sorted(per_slice * 2), calls
    head_ref, grads_ref = _reference(x, blocks, wgt, heads)
    assert set(grads_tail) == set(grads_full) == set(grads_ref) and len(grads_ref) == 25
    e_full, e_tail = rel_l2(head_full, head_ref), rel_l2(head_tail, head_ref)
    print(f"D={d} FF={ff} T={t} B={b} words={words}: forward head rows full {e_full:.3e} tail {e_tail:.3e} bit-equal: {torch.equal(head_full, head_tail)}")
    bad, unequal = {}, []
    for k in grads_ref:
        assert grads_tail[k] is not None and torch.isfinite(grads_tail[k]).all(), k
        ef, et = rel_l2(grads_full[k], grads_ref[k]), rel_l2(grads_tail[k], grads_ref[k])
        same = torch.equal(grads_full[k], grads_tail[k])
        print(f"  {k:10s} full {ef:.3e} tail {et:.3e} ratio {et / max(ef, 1e-30):.3f} bit-equal: {same}")
        if et > 1.1 * ef:
            bad[k] = (et, ef)
        if not same:
            unequal.append(k)
    assert torch.equal(head_full, head_tail)
    assert e_tail <= 1.1 * e_full
    assert not bad, bad
    assert not unequal, unequal


def _tiny_vit(seed=3):
    torch.manual_seed(seed)
    cfg = dict(patch_size=8, latent_dim=D, num_layers=2, feedforward_dim_ratio=2.0)
    m = C.VanillaClassifier(3, 10, 32, D, encoder="vit", encoder_config=cfg)  # 16 patches + head token: T = 17
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    return m


def test_plan_replay_equals_the_unplanned_path():
    """4 AdamW steps of a small ViT through `TrainStep` with the head-only tail: recorded / replayed launch plans (twin shadow arenas,
    optimizer ranges inside backward, the buffers the tail needs zeroed once and kept by the plan) against CFHIP_STACK_PLANS = 0:
    every loss and every parameter."""
    from cflearn_amd.engine import TrainStep

    sd = {k: v.detach().clone() for k, v in _tiny_vit().state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = [torch.randn(5, 3, 32, 32, generator=g).to(DEV) for _ in range(4)]
    labels = [torch.randint(0, 10, (5,), generator=g).to(DEV) for _ in range(4)]
    keep, keep_rows = fused.STACK_PLANS, fused.HEAD_ONLY_MIN_ROWS
    fused.HEAD_ONLY_MIN_ROWS = 0
    res = {}
    calls = []
    tail = ops.head_rows_zero
    try:
        ops.head_rows_zero = lambda *a: (calls.append(1), tail(*a))[1]
        for plans in (True, False):
            fused.STACK_PLANS = plans
            fused._plans.clear()
            m = _tiny_vit()
            m.load_state_dict(sd)
            m = m.to(DEV)
            ts = TrainStep(m, lr=1e-2)
            n0 = len(calls)
            losses = [ts.step(i, l).item() for i, l in zip(imgs, labels)]
            torch.cuda.synchronize()
            res[plans] = (losses, {k: p.detach().clone() for k, p in m.named_parameters()}, len(calls) - n0)
    finally:
        fused.STACK_PLANS, fused.HEAD_ONLY_MIN_ROWS = keep, keep_rows
        ops.head_rows_zero = tail
        fused._plans.clear()
    assert res[False][2] == 40  # 5 tensors zeroed per batch slice in every step: 4 steps x 2 slices x 5
    assert res[True][2] == 20  # ... and, under a plan, in the unplanned first and the recorded second step only
    # the same launches with the same arguments — but not bitwise at this width: the scalar loss is a sum of per-sample f32 atomics,
    # and 128-wide LayerNorm parameter gradients fold through LDS float atomics (the bounds tests/test_gpu_train.py uses for both)
    for l1, l0 in zip(res[True][0], res[False][0]):
        assert abs(l1 - l0) <= 1e-5 * abs(l0), (res[True][0], res[False][0])
    for k, p in res[False][1].items():
        assert rel_l2(res[True][1][k], p) <= 2e-6, (k, rel_l2(res[True][1][k], p))


def test_stacks_not_read_at_the_head_token_keep_the_full_block(monkeypatch):
    """`apply_head=False` and a stack without a head token never take the tail; the same stack read through its head does"""
    calls = []
    gemm = ops.gemm
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: (calls.append(1) if k.get("config_rows") else None, gemm(*a, **k))[1])
    monkeypatch.setattr(fused, "STACK_PLANS", False)
    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", 0)
    enc = _tiny_vit().to(DEV).encoder.encoder
    torch.manual_seed(1)
    tokens = torch.randn(4, 17, D, device=DEV)
    enc.forward_tokens(tokens, apply_head=False).float().square().mean().backward()
    assert not calls
    enc.forward_tokens(tokens, clip_skip=1).float().square().mean().backward()
    assert not calls
    cfg = dict(token_mixing_type="attention", token_mixing_config=dict(num_heads=HEADS, bias=True), num_layers=2, drop_path_rate=0.0,
               norm_type="layer", latent_dim_ratio=2.0, use_head_token=False, head_pooler=None)
    plain = C.MixedStackedEncoder(D, 17, **cfg).to(DEV)
    assert all(b._fusable() for b in plain.mixing_blocks)
    plain.forward_tokens(tokens).float().square().mean().backward()
    assert not calls
    with torch.no_grad():
        enc.forward_tokens(tokens)  # evaluation without grad: the full path
    assert not calls
    enc.forward_tokens(tokens).float().square().mean().backward()
    torch.cuda.synchronize()
    assert len(calls) == 12  # (two batch slices x (3 forward + 3 dX GEMMs))
