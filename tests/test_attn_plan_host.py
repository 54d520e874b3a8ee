"""The attention dispatcher's plan (cfhip_attn_plan / ops.attn_plan), read without a GPU.

  * closed set: over a grid of head widths, lengths, modes, parts and option values the planned names are exactly the
    dispatcher's kernels in the built library's gfx950 code objects (tools/attn_kernel_census.py symbols): nothing planned
    is missing from the library, nothing compiled is unreachable (what the empty docs/attn_unreachable.json claims);
  * the recorded trace: every dispatcher row of docs/ATTN_DISPATCH.md (the kernels of csrc/attn.hip and of its family files) (instantiation -> pytest ids of
    tests/test_gpu_attn_dispatch.py that launched it under a kernel trace) agrees with the plan of that case, looked up in
    that module's own tables;
  * the plan follows the options, and the SUMCOL rule the GPU module reads from the plan is the one it used to spell out."""
import ctypes
import importlib.util
import os
import re

import pytest

import test_gpu_attn_dispatch as dispatch
from cflearn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_DISPATCHER = {"attn_dropout_mask_kernel"}  # csrc/attn.hip, launched by cfhip_attn_dropout_mask alone


def _census_tool():
    spec = importlib.util.spec_from_file_location("attn_kernel_census", os.path.join(ROOT, "tools", "attn_kernel_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def options():
    """set(name=value, ...); the library's defaults come back afterwards, also on failure (the options are process-wide)"""
    def _set(**kw):
        for name, value in {**dispatch.DEFAULTS, **kw}.items():
            ops.set_option(name, value)
    try:
        yield _set
    finally:
        _set()


def test_plan_is_exactly_the_compiled_dispatcher_kernels(options):
    compiled = set(_census_tool().symbols(_lib.LIB_PATH))
    assert len(compiled) == 111
    dispatcher = {n for n in compiled if not n.startswith("attn_probs")} - OUTSIDE_DISPATCHER
    assert len(dispatcher) == 106

    edges = (1, 32, 33, 64, 65, 128, 129, 160, 161, 224, 225, 256, 257)
    modes = ((0, 0), (1, 0), (0, 1))  # plain / mask / causal
    option_sets = [{}] + [dict(attn_two_tiles=511 & ~(1 << b)) for b in range(9)] + [dict(attn_one_pass=v) for v in (0, 1, 2)] \
        + [dict(attn_persistent=v) for v in (0, 7)] + [dict(attn_short_max=v) for v in (0, 32, 256)]
    plan, buf = _lib.load().cfhip_attn_plan, ctypes.create_string_buffer(128)
    seen = set()
    for opt in option_sets:
        options(**opt)
        for dh in range(8, 200, 8):
            for tq in edges:
                for tk in edges:
                    for mask, causal in modes:
                        for drop in (0, 1):
                            for lse in (0, 1):  # the forward does not read parts, the backward does not read lse
                                assert plan(0, dh, tq, tk, mask, causal, drop, 0, lse, buf, 128) == 0
                                seen.add(buf.value)
                            for parts in (1, 2, 3):
                                assert plan(1, dh, tq, tk, mask, causal, drop, parts, 1, buf, 128) == 0
                                seen.add(buf.value)
    planned = {name for text in seen for name in text.decode().split("\n")}
    assert planned - dispatcher == set(), "planned, not in the library"
    assert dispatcher - planned == set(), "compiled, never planned"
    assert max(text.count(b"\n") for text in seen) <= 2  # at most three steps: delta, dQ, dK / dV


def _tabled_cases():
    """pytest id -> (run_attention keywords, options, parts, dropout) of the three tabled tests, from the module's own tables"""
    cases = {}
    for c in dispatch.CASES:
        kw, opt = c.values
        cases[f"test_dispatch[{c.id}]"] = (kw, opt, (3,), 0.0)
    (parts_mark,) = [m for m in dispatch.test_backward_parts.pytestmark if m.args[0] == "parts"]
    for cid, kw, opt in dispatch.PARTS_SHAPES:
        for pid, parts in zip(parts_mark.kwargs["ids"], parts_mark.args[1]):
            cases[f"test_backward_parts[{cid}-{pid}]"] = (kw, opt, parts, 0.0)
    for c in dispatch.DROP_CASES:
        dh, tq, tk, mode, parts = c.values
        kw = dict(dh=dh, tq=tq, tk=tk, mode=mode, mask_kind="full" if mode == "mask" else None)
        cases[f"test_dropout_forms[{c.id}]"] = (kw, {}, parts, 0.3)
    return cases


def _launched(kw, parts, dropout):
    """the kernels run_attention(**kw) launches: the forward, one backward call per entry of `parts`, and with dropout the
    mask kernel behind ops.attn_dropout_mask"""
    how = dict(mask=kw.get("mask_kind") is not None, causal=kw.get("mode") == "causal", head_dim=kw["dh"], dropout_p=dropout)
    names = ops.attn_plan(kw["tq"], kw["tk"], **how)
    for part in parts:
        names += ops.attn_plan(kw["tq"], kw["tk"], backward=True, parts=part, **how)
    return names + (["attn_dropout_mask_kernel"] if dropout else [])


def test_plan_agrees_with_the_recorded_trace(options):
    rows = re.findall(r"^\| `(attn_[^`]+)` \| `([^`]+)`(?: `([^`]+)`)? \((\d+)\) \| \|$", open(os.path.join(ROOT, "docs", "ATTN_DISPATCH.md")).read(), flags=re.M)
    rows = [r for r in rows if not r[0].startswith("attn_probs")]
    assert len(rows) == 107
    cases = _tabled_cases()
    assert len(cases) == 425 + 3 * 17 + 39
    for kernel, first, last, _ in rows:
        assert first in cases, f"{kernel}: no case in the test module's tables for {first}"
        for tid in filter(None, (first, last)):
            if tid not in cases:
                assert tid.startswith(("test_one2_equals_one_bit_for_bit[", "test_persistent_forward_equals_one_shot_bit_for_bit[")), tid
                continue
            kw, opt, parts, dropout = cases[tid]
            options(**opt)
            assert kernel in _launched(kw, parts, dropout), f"{tid} launched {kernel} in the trace; the plan: {_launched(kw, parts, dropout)}"


def test_sumcol_cases_are_the_ones_spelled_out_before(options):
    """the looser lse term of test_gpu_attn_dispatch goes to the SUMCOL forward: plain, no dropout, head_dim 40 or 56, option
    bits 1 and 16 (the rule the module carried as `uses_sumcol` before it asked the plan)"""
    hits = 0
    for tid, (kw, opt, _, dropout) in _tabled_cases().items():
        options(**opt)
        tt = opt.get("attn_two_tiles", 511)
        plain = kw.get("mode", "plain") == "plain" and kw.get("mask_kind") is None
        want = bool(plain and not dropout and kw["dh"] in (40, 56) and (tt & 1) and (tt & 16))
        (fwd,) = ops.attn_plan(kw["tq"], kw["tk"], mask=kw.get("mask_kind") is not None, causal=kw.get("mode") == "causal", head_dim=kw["dh"],
                               dropout_p=dropout)
        assert (fwd.startswith("attn_fwd2_kernel<") and fwd.endswith(",true>")) == want, (tid, fwd)
        hits += want
    assert hits > 20


def test_plan_follows_the_options_and_restores_them(options):
    assert ops.attn_plan(37, 53, head_dim=40) == ["attn_fwd2_kernel<true,3,true>"]
    options(attn_two_tiles=511 & ~16)
    assert ops.attn_plan(37, 53, head_dim=40) == ["attn_fwd2_kernel<true,3,false>"]
    options(attn_two_tiles=511 & ~1)
    assert ops.attn_plan(37, 53, head_dim=40) == ["attn_gen_fwd_kernel<1,true,false>"]
    options()
    assert ops.attn_plan(37, 53, head_dim=40) == ["attn_fwd2_kernel<true,3,true>"]
    # the ViT shape: one launch with both parts, the persistent pair when they are asked for one by one
    assert ops.attn_plan(197, 197, backward=True) == ["attn_bwd_one2_kernel<7>"]
    assert ops.attn_plan(197, 197, backward=True, parts=1) == ["attn_bwd_dq_pers_kernel<7>"]
    assert ops.attn_plan(70, 129, backward=True, parts=2, head_dim=40) == ["attn_delta_kernel", "attn_bwd_dkv2_kernel<true,3,true>"]
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attn_plan(16, 16, head_dim=20)
    with pytest.raises(RuntimeError, match="parts"):
        ops.attn_plan(16, 16, backward=True, parts=0)
