"""Host side of the head-only tail (fused.HEAD_ONLY): when `MixedStackedEncoder.forward_tokens` asks for it (the 8th entry of the
stack's metas), when the stack node honours the request, and that both are part of a launch plan's key.  No device needed."""
import torch

import cflearn_amd as C
from cflearn_amd import fused

D = 128


def _encoder(**kw):
    cfg = dict(token_mixing_type="attention", token_mixing_config=dict(num_heads=2, bias=True), num_layers=2, drop_path_rate=0.0,
               norm_type="layer", latent_dim_ratio=2.0, use_head_token=True, head_pooler=None)
    cfg.update(kw)
    return C.MixedStackedEncoder(D, 4, **cfg)


def _asked(enc, monkeypatch, **kw):
    """the `head_only` entries of the metas `forward_tokens(**kw)` hands to the stack node (None: it did not take the stack node)"""
    seen = []

    def stack(net, metas, keep_mask, causal, params):
        seen.append(metas)
        return net

    monkeypatch.setattr(fused, "mixing_stack", stack)
    monkeypatch.setattr(enc, "post_process", lambda net: net)
    enc.forward_tokens(torch.zeros(2, 5, D), **kw)
    if not seen:
        return None
    flags = {m[7] for m in seen[0]}
    assert len(flags) == 1 and all(len(m) == 8 for m in seen[0])
    return flags.pop()


def test_forward_tokens_asks_for_the_tail_only_when_the_head_token_is_all_that_leaves(monkeypatch):
    assert _asked(_encoder(), monkeypatch) is True  # PreNorm head
    assert _asked(_encoder(norm_after_head=True), monkeypatch) is True
    assert _asked(_encoder(), monkeypatch, apply_head=False) is False
    assert _asked(_encoder(num_layers=3), monkeypatch, clip_skip=1) is False
    assert _asked(_encoder(), monkeypatch, causal=True) is False
    with torch.no_grad():  # evaluation without grad
        assert _asked(_encoder(), monkeypatch) is False
    assert _asked(_encoder(use_head_token=False), monkeypatch) is False  # identity head: every token leaves
    off = _encoder()
    off.head_only_tail = False  # what the CLIP towers set
    assert _asked(off, monkeypatch) is False
    # post-norm blocks never reach the stack node that carries the flag (forward_tokens takes it only when every block is fusable)
    assert not any(b._fusable() for b in _encoder(norm_position="post_norm").mixing_blocks)
    assert all(b._fusable() for b in _encoder().mixing_blocks)
    from cflearn_amd.modules import CLIP

    clip = CLIP(img_size=32, vision_patch_size=16, vision_latent_dim=D, vision_num_layers=2, vision_num_heads=2, latent_dim=64,
                use_text=False)
    assert clip.vit.encoder.head_only_tail is False


def test_stack_node_honours_the_request_for_training_passes_without_mask_only(monkeypatch):
    on = ((2, 1e-5, 1e-5, False, 0, 0, 0, True),) * 2
    off = ((2, 1e-5, 1e-5, False, 0, 0, 0, False),) * 2
    short = ((2, 1e-5, 1e-5, False),) * 2  # metas of callers that know nothing of the flag
    ho = fused.MixingStackFn._head_only
    rows = fused.HEAD_ONLY_MIN_ROWS
    assert ho(on, None, False, True, rows)
    assert not ho(on, None, False, True, rows - 1)  # too few rows for the tail to pay
    assert not ho(off, None, False, True, rows) and not ho(short, None, False, True, rows)
    assert not ho(on, None, False, False, rows)  # evaluation: no backward follows
    assert not ho(on, None, True, True, rows)  # causal
    assert not ho(on, torch.ones(1, dtype=torch.bool), False, True, rows)  # masked
    monkeypatch.setattr(fused, "HEAD_ONLY", False)  # CFHIP_HEAD_ONLY=0
    assert not ho(on, None, False, True, rows)


def test_the_flag_and_the_switch_are_part_of_the_plan_key(monkeypatch):
    x = torch.zeros(2, 5, D)
    on = ((2, 1e-5, 1e-5, False, 0, 0, 0, True),) * 2
    off = ((2, 1e-5, 1e-5, False, 0, 0, 0, False),) * 2
    state = (1, 0)
    k_on, k_off = fused._plan_key(x, on, None, False, state), fused._plan_key(x, off, None, False, state)
    assert k_on != k_off and k_on == fused._plan_key(x, on, None, False, state)
    monkeypatch.setattr(fused, "HEAD_ONLY", not fused.HEAD_ONLY)
    assert fused._plan_key(x, on, None, False, state) != k_on
    assert fused._plan_key(x, on, None, False, state)[-1] == state  # (StackPlan reads the gradient state from the last entry)
    monkeypatch.undo()
    monkeypatch.setattr(fused, "HEAD_ONLY_MIN_ROWS", fused.HEAD_ONLY_MIN_ROWS + 1)
    assert fused._plan_key(x, on, None, False, state) != k_on
