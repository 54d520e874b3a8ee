"""The names cfhip_gemm_kernel_name gives, against the GEMM kernels the built library holds, read without a GPU.

  * every request cfhip_gemm_bf16 accepts under a forced tile configuration (17 configurations x 3 layouts x epilogues
    0 .. 5, the rule of tests/test_gpu_gemm_epilogues.py: `accepted`) is named, and the name is the leading template
    arguments of a gemm_bf16_kernel / gemm_bf16_phase_kernel instantiation in the library's gfx950 code objects
    (tools/attn_kernel_census.py: code_objects, normalise, symbols);
  * closed set: every compiled non-convolution instantiation of the two templates is the kernel of such a request, or the
    bias-gradient form (BG = true) of a weight-gradient request on a tile that has one; what is left must be listed, with a
    reason, in docs/gemm_unreachable.json, and the file must list nothing else."""
import ctypes
import importlib.util
import json
import os
import re

import pytest

from cflearn_amd import _lib, ops
from test_gpu_gemm import TILE_CONFIG_NAMES
from test_gpu_gemm_epilogues import LAYOUTS, accepted, expected_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPLATES = ("gemm_bf16_kernel<", "gemm_bf16_phase_kernel<")


def _census_tool():
    spec = importlib.util.spec_from_file_location("attn_kernel_census", os.path.join(ROOT, "tools", "attn_kernel_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled():
    tool = _census_tool()
    names = tool.symbols(_lib.LIB_PATH, "gemm_bf16_")
    assert tool.symbols(_lib.LIB_PATH) == tool.symbols(_lib.LIB_PATH, "attn_")  # the default keeps the attention census
    return tool, [n for n in names if n.startswith(TEMPLATES)]


def _conv_arg(symbol):
    """the CONV template argument: the first one after the Cfg<...> type"""
    return int(re.search(r"Cfg<[\d,]+>,(\d+)", symbol).group(1))


def _requested(tool):
    """normalised name -> (cfg, layout, epilogue) of every accepted request under every forced configuration"""
    fn, buf = _lib.load().cfhip_gemm_kernel_name, ctypes.create_string_buffer(128)
    names = {}
    try:
        for cfg in range(17):
            ops.set_option("gemm_config", cfg)
            for layout, (a_trans, b_trans) in LAYOUTS.items():
                for epi in range(6):
                    if not accepted(layout, epi):
                        continue
                    assert fn(264, 264, 72, int(a_trans), int(b_trans), epi, buf, 128) == 0
                    name = buf.value.decode()
                    run = expected_config(cfg, layout, epi)
                    kernel = "gemm_bf16_phase_kernel" if 7 <= run <= 12 else "gemm_bf16_kernel"
                    tf = lambda v: "true" if v else "false"  # noqa: E731
                    base = {4: 1, 5: 3}.get(epi, epi)  # the quick forms run the GELU / GELU' instantiations
                    assert name == f"{kernel}<{tf(a_trans)}, {tf(b_trans)}, {base}, {TILE_CONFIG_NAMES[run]}>", (cfg, layout, epi, name)
                    names.setdefault(tool.normalise(name), (cfg, layout, epi))
    finally:
        ops.set_option("gemm_config", -1)
    return names


def test_every_named_kernel_is_compiled_and_every_compiled_kernel_is_named(compiled):
    tool, symbols = compiled
    plain = [s for s in symbols if _conv_arg(s) == 0]
    assert len(symbols) == 114 and len(plain) == 108  # (6 convolution forms: CONV = 1 forward / input gradient, 2 filter gradient)
    requested = _requested(tool)
    reached = set()
    for name, why in requested.items():
        lead = name[:-1] + ","  # `kernel<AT,BT,EPI,Cfg<..>>` -> `kernel<AT,BT,EPI,Cfg<..>,`: then CONV (and BG)
        hits = [s for s in plain if s.startswith(lead)]
        assert hits, f"{why}: {name} is not in the library"
        # the request itself runs the form without a bias gradient; the weight-gradient layout's BG = true sibling is what the
        # same request runs with `bias_grad` on the tiles that have one (resolve_config sends the others to configuration 1)
        for s in hits:
            rest = s[len(lead):-1].split(",")
            assert rest[0] == "0" and (len(rest) == 1 or rest[1] in ("false", "true")), s
            if len(rest) == 2 and rest[1] == "true":
                assert name.startswith("gemm_bf16_kernel<true,true,0,"), s
                cfg = why[0]
                assert not (7 <= cfg <= 13 or cfg == 16), f"{s}: a bias-gradient form on a configuration that reroutes it"
            reached.add(s)
    remainder = sorted(set(plain) - reached)
    listed = json.load(open(os.path.join(ROOT, "docs", "gemm_unreachable.json")))
    assert all(isinstance(v, str) and v and "\n" not in v for v in listed.values())
    assert sorted(listed) == remainder, "docs/gemm_unreachable.json must list exactly the compiled kernels no request reaches"


def test_last_config_is_a_host_query_that_a_refused_request_leaves_alone():
    """cfhip_gemm_last_config: the configuration of the latest LAUNCH of this thread (-2 before the first, -1 the generic kernel)"""
    lib = _lib.load()
    assert _lib.host_query("cfhip_gemm_last_config") and _lib.ctypes_only("cfhip_gemm_last_config")
    before = lib.cfhip_gemm_last_config()
    assert -2 <= before <= 16
    assert lib.cfhip_gemm_bf16(None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, None, 0, None, 0, None) == -1
    assert lib.cfhip_gemm_bf16_rows(None, None, None, None, None, None, 2, 8, 8, 8, 8, 8, 0, 0, 0, 1, None) == -1  # config_rows < M
    assert lib.cfhip_gemm_last_config() == before


def test_bias_gradient_forms_are_the_tiles_up_to_192x128(compiled):
    _, symbols = compiled
    bg = {re.search(r"Cfg<[\d,]+>", s).group(0) for s in symbols if _conv_arg(s) == 0 and s.endswith(",true>")}
    want = {TILE_CONFIG_NAMES[c].replace(" ", "") for c in range(17) if not (7 <= c <= 13 or c == 16)}
    assert bg == want
