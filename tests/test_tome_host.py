"""Host-side checks of token merging (no device): the split tables and the gate / r / size arithmetic of cflearn_amd.tome against
what tools/gen_tome_golden.py recorded from the reference (tests/golden/tome_small.pt), `setup_hooks` defaults and refusals, the C
entry points of csrc/tome.hip and their refusals, and the forward-only guard of a ToMe-enabled block."""
import os

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops, tome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = {"cfhip_tome_match": 12, "cfhip_tome_select": 15, "cfhip_tome_merge": 12, "cfhip_tome_unmerge_add": 10}
P = 4096  # a non-null, aligned "pointer": every call below is refused before anything could read it


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(GOLDEN, "tome_small.pt"), weights_only=False)


def test_split_tables_equal_the_reference_sets(G):
    """8x8, 16x12, 9x7 (margins) with 2x2 cells, one sx=1 / sy=2 case, use_rand on and off, two seeds: src and dst as SETS are the
    reference's CPU run's; here both tables are ascending, int32, disjoint and cover every token"""
    cases = [s["case"] for s in G["splits"]]
    shapes = {(c[0], c[1], c[2], c[3]) for c in cases}
    assert {(8, 8, 2, 2), (16, 12, 2, 2), (9, 7, 2, 2), (8, 6, 1, 2)} <= shapes
    assert {c[4] for c in cases} == {3, 1234} and {c[5] for c in cases} == {True, False}
    for rec in G["splits"]:
        h, w, sx, sy, seed, use_rand = rec["case"]
        src, dst = tome.split_tables(h, w, sx, sy, seed, use_rand)
        assert src.dtype == dst.dtype == torch.int32 and src.device.type == "cpu"
        assert torch.equal(src, rec["src"]) and torch.equal(dst, rec["dst"]), rec["case"]
        assert dst.numel() == (h // sy) * (w // sx) and src.numel() + dst.numel() == h * w
        assert bool((src[1:] > src[:-1]).all()) and bool((dst[1:] > dst[:-1]).all())
        assert sorted(src.tolist() + dst.tolist()) == list(range(h * w))
        if not use_rand:  # cell position 0: the top-left token of every cell
            assert dst.tolist() == [y * sy * w + x * sx for y in range(h // sy) for x in range(w // sx)]
    # the margin of 9x7 is src; a seed changes the split, use_rand=False ignores it
    src, dst = tome.split_tables(9, 7, 2, 2, 3, True)
    assert all(t in src.tolist() for t in [6, 13, 56, 57, 62])
    assert not torch.equal(tome.split_tables(8, 8, 2, 2, 3, True)[1], tome.split_tables(8, 8, 2, 2, 1234, True)[1])
    assert torch.equal(tome.split_tables(8, 8, 2, 2, 3, False)[1], tome.split_tables(8, 8, 2, 2, 1234, False)[1])


def test_gate_r_and_sizes_equal_compute_merge(G):
    odd = 0
    for rec in G["sizes"]:
        h0, w0, d, ratio, md, sx, sy = rec["case"]
        info = tome.setup_tome_info(dict(ratio=ratio, max_downsample=md, sx=sx, sy=sy))
        info["size"] = (h0, w0)
        got = tome.merge_sizes(rec["num_tokens"], info)
        if not rec["merged"]:
            assert got is None, rec
            continue
        h, w, r = got
        assert r == rec["r"] and (h // sy) * (w // sx) == rec["n_dst"], (rec, got)
        assert h * w == rec["num_tokens"]
        odd += (h % 2) + (w % 2) > 0
    assert odd >= 8 and sum(r["merged"] for r in G["sizes"]) >= 30 and sum(not r["merged"] for r in G["sizes"]) >= 30
    with pytest.raises(RuntimeError, match="size"):
        tome.merge_sizes(64, tome.setup_tome_info({}))


def test_setup_hooks_defaults_and_refusals():
    block = C.SpatialTransformerBlock(64, 2, 32, context_dim=32)
    assert block.tome_info is None
    given = dict(ratio=0.25, seed=5)
    block.setup_hooks(tome_info=given)
    assert block.tome_info == dict(ratio=0.25, max_downsample=1, sx=2, sy=2, use_rand=True, merge_attn=True, merge_crossattn=False,
                                   merge_mlp=False, seed=5)
    assert given == dict(ratio=0.25, seed=5) and block.tome_info is not given  # a copy, as shallow_copy_dict makes
    block.setup_hooks(tome_info={})
    assert block.tome_info == tome.TOME_DEFAULTS and "seed" not in block.tome_info
    block.setup_hooks()
    assert block.tome_info is None
    with pytest.raises(TypeError):
        block.setup_hooks(tome=dict())
    with pytest.raises(TypeError, match="ration"):
        block.setup_hooks(tome_info=dict(ration=0.5))
    with pytest.raises(NotImplementedError, match="§8"):
        block.setup_hooks(style_reference_states=dict(style_fidelity=0.5))
    # the constructors keep refusing `hooks_kwargs`
    with pytest.raises(NotImplementedError):
        C.SpatialTransformerBlock(64, 2, 32, hooks_kwargs=dict(tome_info={}))
    with pytest.raises(NotImplementedError):
        C.SpatialTransformer(64, 2, 32, hooks_kwargs=dict(tome_info={}))

    st = C.SpatialTransformer(64, 2, 32, num_layers=2, context_dim=32)
    st.setup_hooks(tome_info=dict(seed=1))
    infos = [b.tome_info for b in st.blocks]
    assert all(i is not None and i["seed"] == 1 for i in infos) and infos[0] is not infos[1]
    st.setup_hooks()
    assert all(b.tome_info is None for b in st.blocks)
    with pytest.raises(NotImplementedError, match="§8"):
        st.setup_hooks(style_reference_states={})
    for cls in (C.modules.UNetDiffuser, C.ControlNet):
        assert callable(getattr(cls, "setup_hooks"))


def test_block_with_tome_refuses_grad_before_any_device_work():
    """on the CPU: were anything launched or any table built, this would fail for another reason"""
    block = C.SpatialTransformerBlock(64, 2, 32, context_dim=32)
    block.setup_hooks(tome_info=dict(seed=1))
    block.tome_info["size"] = (8, 8)
    x = torch.zeros(1, 64, 64)
    with pytest.raises(NotImplementedError, match="§8"):
        block(x, torch.zeros(1, 5, 32))  # grad mode on, parameters require grad
    for p in block.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="§8"):
        block(x.clone().requires_grad_(True), torch.zeros(1, 5, 32))


def _refused(rc, *words):
    msg = _lib.load().cfhip_last_error()
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"], rc
    assert msg and all(w.encode() in msg for w in words), msg


def test_entry_points_are_declared_built_and_cited():
    lib = _lib.load()
    for name, nargs in NEW_ENTRIES.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None and not _lib.ctypes_only(name)
    assert _lib.DEFINES["CFHIP_TOME_MAX_CHANNELS"] == ops.TOME_MAX_CHANNELS == 1280
    assert _lib.DEFINES["CFHIP_TOME_MAX_TOKENS"] == ops.TOME_MAX_TOKENS == 65536
    header = open(_lib.HEADER_PATH).read()
    for cite in ("mixed_stacks/api.py:473-589", ":592-618", ":679-685", "api.py:536-545", "api.py:552-560", "api.py:562-587"):
        assert cite in header, f"cfhip.h does not cite {cite}"
    assert " tome;" in open(os.path.join(ROOT, "build_lib.sh")).read()
    import __graft_entry__ as entry

    assert "tome" in entry.SOURCES and os.path.isfile(os.path.join(entry.CSRC, "tome.hip"))


def test_c_abi_limits_are_checked_before_any_launch():
    lib = _lib.load()

    def match(x=P, b=1, n=64, c=64, n_src=48, n_dst=16):
        return lib.cfhip_tome_match(x, P, P, P, P, P, b, n, c, n_src, n_dst, None)

    _refused(match(x=None), "tome_match", "null")
    _refused(match(c=12), "tome_match", "C = 12")
    _refused(match(c=0), "tome_match", "C = 0")
    _refused(match(c=1288), "tome_match", "C = 1288", "1280")
    _refused(match(n=65537, n_src=65521), "tome_match", "N = 65537", "65536")
    _refused(match(b=0), "tome_match", "B = 0")
    _refused(match(n_src=47), "tome_match", "do not split")
    _refused(match(n_src=64, n_dst=0), "tome_match", "do not split")
    _refused(match(x=P + 8), "tome_match", "misaligned")

    def select(r=24, n=64, n_src=48, n_dst=16, cursor=P):
        return lib.cfhip_tome_select(P, P, P, P, P, P, P, P, cursor, 1, n, n_src, n_dst, r, None)

    _refused(select(cursor=None), "tome_select", "null")
    _refused(select(r=0), "tome_select", "r = 0")
    _refused(select(r=49), "tome_select", "r = 49")
    _refused(select(n=65540, n_src=65524), "tome_select", "N = 65540")
    _refused(lib.cfhip_tome_merge(P, P, P, P, P, 1, 64, 20, 48, 16, 24, None), "tome_merge", "C = 20")
    _refused(lib.cfhip_tome_merge(P, P, P, P, P, 1, 64, 64, 48, 16, 0, None), "tome_merge", "r = 0")
    _refused(lib.cfhip_tome_merge(P, P, P, P, P + 2, 1, 64, 64, 48, 16, 24, None), "tome_merge", "misaligned")
    _refused(lib.cfhip_tome_unmerge_add(P, P, None, P, 0, 1, 64, 4, 24, None), "tome_unmerge_add", "C = 4")
    _refused(lib.cfhip_tome_unmerge_add(P, P, None, P, 0, 1, 64, 64, 64, None), "tome_unmerge_add", "r = 64")
    _refused(lib.cfhip_tome_unmerge_add(P, None, None, P, 0, 1, 64, 64, 24, None), "tome_unmerge_add", "null")


def test_ops_refuse_before_any_launch():
    i32 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tome_match(torch.zeros(1, 8, 8, dtype=torch.bfloat16), i32, i32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tome_select(torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), i32, i32, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tome_merge(torch.zeros(1, 8, 8, dtype=torch.bfloat16), i32, i32, i32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tome_unmerge_add(torch.zeros(1, 6, 8, dtype=torch.bfloat16), torch.zeros(1, 8, dtype=torch.int32))


def test_fixture_records_its_margins(G):
    """the generator asserted them; what the GPU test relies on is written in the file"""
    assert sorted(G["blocks"]) == sorted(f"{s}-{f}" for s in ("8x8", "9x7") for f in ("attn", "all", "cross_mlp"))
    for key, rec in G["blocks"].items():
        assert rec["margin_factor"] == 8.0
        assert rec["gap_top2"] >= 8.0 * rec["score_spread"] > 0 and rec["gap_r"] >= 8.0 * rec["score_spread"], key
        assert tuple(rec["pairs"].shape) == (2, rec["r"], 2) and rec["r"] == min(rec["src"].numel(), int(rec["h"] * rec["w"] * 0.5))
        assert tuple(rec["y"].shape) == tuple(rec["y_bf16"].shape) == tuple(rec["x"].shape) == (2, rec["h"] * rec["w"], 64)


def test_fixture_matches_a_regeneration(G):
    """the committed fixture against tools/gen_tome_golden.py run now, in memory, through oracle.refharness"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refharness

    if not refharness.reference_available():
        pytest.skip("the reference tree is not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_tome_golden as gen

    threads = torch.get_num_threads()
    try:
        fresh = gen.generate()  # (single-threaded)
    finally:
        torch.set_num_threads(threads)
    assert sorted(fresh) == sorted(G) and fresh["block_cfg"] == G["block_cfg"] and fresh["block_seed"] == G["block_seed"]
    for a, b in zip(fresh["splits"], G["splits"]):
        assert a["case"] == b["case"] and torch.equal(a["src"], b["src"]) and torch.equal(a["dst"], b["dst"])
    assert fresh["sizes"] == G["sizes"]
    for key, rec in G["blocks"].items():
        now = fresh["blocks"][key]
        assert sorted(now) == sorted(rec)
        for name in ("x", "context", "pairs", "src", "dst"):
            assert torch.equal(now[name], rec[name]), (key, name)
        assert now["r"] == rec["r"] and now["tome_info"] == rec["tome_info"]
        assert torch.allclose(now["y"], rec["y"], rtol=1e-4, atol=1e-6), key
        # (the reference's bf16 run: another CPU's kernels may round a bf16 intermediate the other way)
        assert float((now["y_bf16"] - rec["y_bf16"]).norm() / rec["y_bf16"].norm()) < 5e-3, key
