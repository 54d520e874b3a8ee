"""The RWKV mixers without a GPU: the registry entries, state-dict parity with the reference's recorded keys, the closed-form initial
values, the initialisation stand-alone and inside MixedStackedEncoder, every refusal, the C-ABI declarations and build lists, and the
float64 replica of tests/rwkv_replay.py against the reference's recorded fp32 outputs and gradients (with `gradcheck` of its adjoints)."""
import os
import re

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops
from cflearn_amd.registry import channel_mixers, token_mixers

import rwkv_replay as R
from helpers import rel_l2
from rwkv_weights import fill_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> number of arguments
ENTRIES = {"cfhip_rwkv_time_mix_fwd": 12, "cfhip_rwkv_time_mix_bwd_workspace": 3, "cfhip_rwkv_time_mix_bwd": 20, "cfhip_rwkv_wkv_fwd": 12,
           "cfhip_rwkv_wkv_bwd_workspace": 2, "cfhip_rwkv_wkv_bwd": 20, "cfhip_rwkv_relu2_fwd": 5, "cfhip_rwkv_relu2_bwd": 7,
           "cfhip_rwkv_gate_fwd": 8, "cfhip_rwkv_gate_bwd": 8}
CLASSES = {"token": C.RWKVTokenMixer, "channel": C.RWKVChannelMixer, "encoder": C.MixedStackedEncoder}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rwkv_small.pt")


def build(rec):
    torch.manual_seed(rec["seed"])
    return CLASSES[rec["kind"]](**rec["kwargs"])


def test_registry_and_export():
    assert C.module_dict["token_mixer.rwkv"] is C.RWKVTokenMixer and C.module_dict["channel_mixer.rwkv"] is C.RWKVChannelMixer
    # the surplus keys MixingBlock passes (`dropout` to the token mixer, `num_tokens`-less config to the channel mixer) are dropped
    tm = token_mixers.build("rwkv", config=dict(layer_idx=1, num_layers=4, num_tokens=24, in_dim=16, latent_dim=24, dropout=0.1))
    cm = channel_mixers.build("rwkv", config=dict(layer_idx=1, num_layers=4, in_dim=16, latent_dim=24, dropout=0.1, activation="GELU"))
    assert isinstance(tm, C.RWKVTokenMixer) and isinstance(tm, C.modules.ITokenMixer) and tm.need_2d is False
    assert isinstance(cm, C.RWKVChannelMixer) and isinstance(cm, C.modules.IChannelMixer) and cm.need_2d is False
    assert all(isinstance(m, torch.nn.Linear) and m.bias is None for m in (tm.key, tm.value, tm.receptance, tm.output, cm.key, cm.value, cm.receptance))
    enc = C.MixedStackedEncoder(16, 8, token_mixing_type="rwkv", channel_mixing_type="rwkv", num_layers=2, norm_type="layer", head_pooler=None)
    assert all(isinstance(b.token_mixing, C.RWKVTokenMixer) and isinstance(b.channel_mixing, C.RWKVChannelMixer) and not b._fusable()
               for b in enc.mixing_blocks)


def test_only_rwkv_blocks_get_the_f32_hand_over():
    """`MixingBlock` sets `out_f32` on a pre-norm LayerNorm only for a mixer that declares `f32_input`: attention / ff blocks keep
    their bf16 hand-over, a mixed block gets it on the rwkv side alone, post-norm blocks never"""
    kw = dict(num_layers=2, norm_type="layer", head_pooler=None)
    f32 = lambda norm: bool(getattr(norm, "out_f32", False))  # noqa: E731
    assert not hasattr(C.AttentionTokenMixer, "f32_input") and not hasattr(C.FeedForward, "f32_input")
    for b in C.MixedStackedEncoder(64, 8, token_mixing_type="attention", channel_mixing_type="ff", **kw).mixing_blocks:
        assert not f32(b.token_norm) and not f32(b.channel_norm)
    for b in C.MixedStackedEncoder(64, 8, token_mixing_type="rwkv", channel_mixing_type="rwkv", **kw).mixing_blocks:
        assert f32(b.token_norm) and f32(b.channel_norm)
    for b in C.MixedStackedEncoder(64, 8, token_mixing_type="rwkv", channel_mixing_type="ff", **kw).mixing_blocks:
        assert f32(b.token_norm) and not f32(b.channel_norm)
    for b in C.MixedStackedEncoder(64, 8, token_mixing_type="attention", channel_mixing_type="rwkv", **kw).mixing_blocks:
        assert not f32(b.token_norm) and f32(b.channel_norm)
    for b in C.MixedStackedEncoder(64, 8, token_mixing_type="rwkv", channel_mixing_type="rwkv", norm_position="post_norm", **kw).mixing_blocks:
        assert not f32(b.token_norm) and not f32(b.channel_norm)


@pytest.mark.parametrize("index", range(5))
def test_state_dict_matches_reference(fx, index):
    rec = fx["configs"][index]
    state = build(rec).state_dict()
    assert [(k, tuple(v.shape), str(v.dtype)) for k, v in state.items()] == [tuple(e) for e in rec["state"]], rec["name"]
    if rec["kind"] == "encoder":
        assert len(state) == 56


@pytest.mark.parametrize("index", range(5))
def test_initial_decay_and_mixes_match_reference(fx, index):
    rec = fx["configs"][index]
    state = build(rec).state_dict()
    assert rec["init"] and all(k.endswith("info_decay") or "time_mix_" in k for k in rec["init"])
    for k, want in rec["init"].items():
        assert float((state[k] - want).abs().max()) <= 1e-6, k


def test_initialisation_alone_and_inside_the_encoder(fx):
    torch.manual_seed(11)
    tm = C.RWKVTokenMixer(1, 4, 24, 64, 96)
    cm = C.RWKVChannelMixer(1, 4, 64, 96, 0.0)
    for w in (tm.key.weight, tm.receptance.weight, tm.output.weight, cm.value.weight, cm.receptance.weight):
        assert float(w.abs().max()) == 0.0
    for w in (tm.value.weight, cm.key.weight):  # orthogonal: [96, 64] has orthonormal columns
        assert float((w.t() @ w - torch.eye(64)).abs().max()) < 1e-5
    enc = build(fx["configs"][4])
    seen = 0
    for name, p in enc.named_parameters():
        if name.endswith(("key.weight", "value.weight", "receptance.weight", "output.weight")):
            assert 0.015 <= float(p.std()) <= 0.025, (name, float(p.std()))
            seen += 1
    assert seen == 21


@pytest.mark.parametrize("index", range(5))
def test_checkpoint_round_trip(fx, index):
    rec = fx["configs"][index]
    m = build(rec)
    state = {k: (torch.randn(s, generator=torch.Generator().manual_seed(i)) if "float" in d else torch.zeros(s, dtype=torch.int64))
             for i, (k, s, d) in enumerate(rec["state"])}
    m.load_state_dict(state, strict=True)
    back = m.state_dict()
    assert list(back) == list(state) and all(torch.equal(back[k], state[k]) for k in state)


@pytest.mark.parametrize("index", range(5))
def test_replica_reproduces_the_reference(fx, index):
    """ties tests/rwkv_replay.py (recurrences and hand-written adjoints, float64) to the reference's conv formulation on the CPU"""
    rec = fx["configs"][index]
    model = build(rec)
    fill_parameters(model, rec["seed"])
    y, dx, grads = R.run_module(rec["kind"], model.state_dict(), rec["x"], rec["dy"], rec["kwargs"].get("num_layers"))
    assert rel_l2(y, rec["y"].double()) < 1e-5 and rel_l2(dx, rec["dx"].double()) < 1e-5
    assert set(grads) == set(rec["grads"])
    for k, want in rec["grads"].items():
        got = grads[k][::rec["grad_rows"][k]] if k in rec["grad_rows"] else grads[k]
        if float(want.norm()) == 0.0:
            assert float(got.norm()) == 0.0, k
        else:
            assert rel_l2(got, want.double()) < 1e-5, (k, rel_l2(got, want.double()))


def test_replica_adjoints_pass_gradcheck():
    gen = torch.Generator().manual_seed(3)
    k, v, r = (torch.randn((2, 5, 3), generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    w = (torch.randn((3, 1), generator=gen, dtype=torch.float64) * 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(R.Wkv.apply, (k, v, r, w), eps=1e-6, atol=1e-7, rtol=1e-5)
    # the step-weighted scan of the bounds is what its definition says
    x = torch.rand((1, 6, 2), generator=gen, dtype=torch.float64)
    lam = torch.tensor([0.5, 0.9], dtype=torch.float64)
    for rev in (False, True):
        want = torch.zeros_like(x)
        for t in range(6):
            for s in range(6):
                if (s > t) if rev else (s < t):
                    want[:, t] += lam ** abs(t - s) * abs(t - s) * x[:, s]
        assert float((R.scan_steps(x, lam, rev) - want).abs().max()) < 1e-12


def test_refusals():
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.RWKVTokenMixer(0, 4, 8, 12, 16)
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.RWKVTokenMixer(0, 4, 8, 16, 20)
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.RWKVChannelMixer(0, 4, 16, 12, 0.0)
    tm = C.RWKVTokenMixer(1, 4, 8, 16, 24)
    cm = C.RWKVChannelMixer(1, 4, 16, 24, 0.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        tm(torch.zeros(2, 8, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        cm(torch.zeros(2, 8, 16))
    with pytest.raises(ValueError, match="num_tokens = 8, got T = 9"):
        tm(torch.zeros(2, 9, 16))
    with pytest.raises(ValueError, match=r"\[B, T, 16\] expected"):
        tm(torch.zeros(2, 8, 24))
    with pytest.raises(ValueError, match=r"\[B, T, 16\] expected"):
        cm(torch.zeros(8, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rwkv_time_mix(torch.zeros(1, 2, 8), torch.zeros(8), None, torch.zeros(8))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rwkv_wkv(torch.zeros(1, 2, 8), torch.zeros(1, 2, 8), torch.zeros(1, 2, 8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rwkv_relu2(torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rwkv_gate(torch.zeros(4), torch.zeros(4))


def test_entries_declared_cited_and_built():
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, len(_lib.SIGNATURES[name][1]))
    assert sum(name.startswith("cfhip_rwkv_") for name in _lib.SIGNATURES) == len(ENTRIES)
    assert ops.RWKV_CHUNK == _lib.DEFINES["CFHIP_RWKV_CHUNK"] and ops.RWKV_MAX_WAVES == _lib.DEFINES["CFHIP_RWKV_MAX_WAVES"]
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("RWKV mixers (csrc/rwkv.hip)"):header.index("cfhip_rwkv_gate_bwd(")]
    for cite in ("token_mixers.py:107-206", "channel_mixers.py:69-113", "token_mixers.py:179-182", "token_mixers.py:184-203", "channel_mixers.py:111",
                 "channel_mixers.py:113"):
        assert cite in block, cite
    import __graft_entry__ as G

    assert "rwkv" in G.SOURCES
    script = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert re.search(r"^for f in .*\brwkv\b.*; do$", script, flags=re.M)
    source = open(os.path.join(ROOT, "carefree-learn_amd", "csrc", "rwkv.hip")).read()
    assert "atomic" not in source.replace("No floating-point atomics", "")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme


def _refused(rc, needle):
    assert rc == -1, rc
    msg = _lib.load().cfhip_last_error().decode()
    assert needle in msg, msg


def test_c_refusals_fire_before_any_launch():
    """no device is touched: the pointers are made-up addresses, every call must return before its launch"""
    lib = _lib.load()
    p = 4096
    _refused(lib.cfhip_rwkv_time_mix_fwd(None, 1, p, p, p, p, p, p, 1, 1, 8, None), "null operand")
    _refused(lib.cfhip_rwkv_time_mix_fwd(p, 1, p, None, p, p, p, p, 1, 1, 8, None), "mv and out_v together")
    _refused(lib.cfhip_rwkv_time_mix_fwd(p, 1, p, p, p, p, p, p, 0, 1, 8, None), "B = 0")
    _refused(lib.cfhip_rwkv_time_mix_fwd(p, 1, p, p, p, p, p, p, 1, 0, 8, None), "T = 0")
    _refused(lib.cfhip_rwkv_time_mix_fwd(p + 2, 1, p, p, p, p, p, p, 1, 1, 8, None), "misaligned")

    def tmb(dk=p, dx=p, dmk=p, ws=p, ws_bytes=1 << 20, acc=0, x=p):
        return lib.cfhip_rwkv_time_mix_bwd(dk, p, p, 0, x, 1, p, p, p, dx, dmk, None, None, acc, ws, ws_bytes, 2, 3, 8, None)

    _refused(tmb(dk=None), "null operand")
    _refused(tmb(x=None), "x for the mix gradients")
    _refused(tmb(dx=None, dmk=None), "nothing to compute")
    _refused(tmb(acc=8), "`accumulate` = 8")
    _refused(tmb(ws_bytes=4), "cfhip_rwkv_time_mix_bwd_workspace says")
    _refused(tmb(ws=None), "cfhip_rwkv_time_mix_bwd_workspace says")
    assert lib.cfhip_rwkv_time_mix_bwd_workspace(2, 3, 8) == 6 * 3 * 8 * 4 and lib.cfhip_rwkv_time_mix_bwd_workspace(0, 3, 8) == 0
    assert 0 < lib.cfhip_rwkv_time_mix_bwd_workspace(10 ** 4, 100, 256) <= 2048 * 3 * 256 * 4  # bounded: at most 2048 partial records

    def fwd(k=p, a=None, b=None, bsz=1, t=4, l=8, waves=0):
        return lib.cfhip_rwkv_wkv_fwd(k, p, p, p, p, a, b, bsz, t, l, waves, None)

    _refused(fwd(k=None), "null operand")
    _refused(fwd(a=p), "a and b together")
    _refused(fwd(l=0), "L = 0")
    _refused(fwd(waves=17), "waves = 17")
    _refused(fwd(waves=-1), "waves = -1")
    _refused(fwd(bsz=65536), "past the grid")

    def bwd(dy=p, dd=p, ws=p, ws_bytes=1 << 20, acc=0, waves=0):
        return lib.cfhip_rwkv_wkv_bwd(dy, 0, p, p, p, p, p, p, p, p, p, dd, acc, ws, ws_bytes, 2, 4, 8, waves, None)

    _refused(bwd(dy=None), "null operand")
    _refused(bwd(ws_bytes=8), "cfhip_rwkv_wkv_bwd_workspace says")
    _refused(bwd(ws=None), "cfhip_rwkv_wkv_bwd_workspace says")
    _refused(bwd(acc=2), "`accumulate` = 2")
    _refused(bwd(waves=99), "waves = 99")
    assert lib.cfhip_rwkv_wkv_bwd_workspace(2, 8) == 64 and lib.cfhip_rwkv_wkv_bwd_workspace(0, 8) == 0
    _refused(lib.cfhip_rwkv_relu2_fwd(None, 1, p, 4, None), "null operand")
    _refused(lib.cfhip_rwkv_relu2_fwd(p, 1, p, 0, None), "n = 0")
    _refused(lib.cfhip_rwkv_relu2_bwd(p, 0, None, 1, p, 4, None), "null operand")
    _refused(lib.cfhip_rwkv_gate_fwd(p, None, None, 0, p, 0, 4, None), "null operand")
    _refused(lib.cfhip_rwkv_gate_fwd(p, p, p + 2, 1, p, 0, 4, None), "misaligned")
    _refused(lib.cfhip_rwkv_gate_bwd(p, 1, p, p, None, p, 4, None), "null operand")
    _refused(lib.cfhip_rwkv_gate_bwd(p, 1, p, p, p, p, -1, None), "n = -1")
