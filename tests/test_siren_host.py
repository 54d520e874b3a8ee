"""Siren / ImgSiren without a GPU: state-dict parity with the reference's recorded keys, bit-equal initial parameters and grid, every
refusal and quirk, the C-ABI declarations, refusals and build lists, `build_activation("sine")`, and the float64 replica of
tests/siren_replay.py (with every bf16 rounding switched off) against the reference's recorded fp32 outputs and gradients."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops

import siren_replay as R
from helpers import rel_l2
from siren_weights import fill_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> number of arguments
ENTRIES = {"cfhip_siren_pack_workspace": 3, "cfhip_siren_pack": 7, "cfhip_siren_fwd": 19, "cfhip_siren_bwd_workspace": 6, "cfhip_siren_bwd": 23,
           "cfhip_siren_reduce": 13, "cfhip_sine_fwd": 5, "cfhip_sine_bwd": 6, "cfhip_relu_f32_fwd": 4, "cfhip_relu_f32_bwd": 5}
CLASSES = {"siren": C.Siren, "img": C.ImgSiren}
N_CONFIGS = 5


@pytest.fixture(scope="module")
def fx(golden):
    return golden("siren_small.pt")


def build(rec):
    torch.manual_seed(rec["seed"])
    return CLASSES[rec["kind"]](*rec["args"], **rec["kwargs"])


def test_export():
    for name in ("make_grid", "img_siren_head", "SirenLayer", "Modulator", "Siren", "ImgSiren", "Sine"):
        assert hasattr(C, name), name
    m = C.Siren(4, 2, 1, 32, num_layers=2)
    assert all(not list(blk.children()) or isinstance(blk.activation, (C.Sine, torch.nn.Identity)) for blk in [*m.blocks, m.head])


@pytest.mark.parametrize("index", range(N_CONFIGS))
def test_state_dict_matches_reference(fx, index):
    rec = fx["configs"][index]
    state = build(rec).state_dict()
    assert [(k, tuple(v.shape), str(v.dtype)) for k, v in state.items()] == [tuple(e) for e in rec["state"]], rec["name"]


@pytest.mark.parametrize("index", range(N_CONFIGS))
def test_checkpoint_round_trip_strict(fx, index):
    rec = fx["configs"][index]
    m = build(rec)
    state = {k: torch.randn(s, generator=torch.Generator().manual_seed(i)) for i, (k, s, _) in enumerate(rec["state"])}
    m.load_state_dict(state, strict=True)
    back = m.state_dict()
    assert list(back) == list(state) and all(torch.equal(back[k], state[k]) for k in state)


@pytest.mark.parametrize("index", range(N_CONFIGS))
def test_initial_parameters_are_the_references_bits(fx, index):
    rec = fx["configs"][index]
    m = build(rec)
    h = hashlib.sha256()
    for _, p in m.named_parameters():
        h.update(p.detach().contiguous().numpy().tobytes())
    assert h.hexdigest() == rec["init_sha"], rec["name"]


@pytest.mark.parametrize("index", range(N_CONFIGS))
def test_grid_is_bit_equal(fx, index):
    rec = fx["configs"][index]
    m = build(rec)
    siren = m.siren if rec["kind"] == "img" else m
    if "grid" not in rec:
        assert siren.grid is None
        return
    assert torch.equal(siren.grid, rec["grid"])
    size, in_dim = (rec["args"][0], 2) if rec["kind"] == "img" else rec["args"][:2]
    assert torch.equal(C.make_grid(size, in_dim), rec["grid"])
    assert C.img_siren_head(3, 2)(torch.arange(36.0).view(2, 9, 2)).shape == (2, 2, 3, 3)


def _front64(state, rec):
    """the part in front of the layer stack in torch float64 with autograd: (leaves, mods [L, B, latent], siren prefix)"""
    leaves = {k: v.detach().double().requires_grad_(True) for k, v in state.items() if v.is_floating_point() and not k.endswith("grid")}
    if "mods" in rec:
        mods = rec["mods"].double().requires_grad_(True)
        leaves["__mods"] = mods
        return leaves, mods, ""
    prefix = "siren." if rec["kind"] == "img" else ""
    z = rec["z"].double().requires_grad_(True)
    leaves["__z"] = z
    net = z
    if rec["kind"] == "img":
        pad = leaves["cond_padding.channel_padding"][rec["labels"]].view(z.shape[0], -1)
        key = [k for k in leaves if k.startswith("cond_padding.mapping")][0]
        net = torch.cat([z, pad], 1) @ leaves[key].t()
    zc, mods, i = net, [], 0
    while f"{prefix}modulator.blocks.{i}.0.weight" in leaves:
        net = torch.relu(net @ leaves[f"{prefix}modulator.blocks.{i}.0.weight"].t() + leaves[f"{prefix}modulator.blocks.{i}.0.bias"])
        mods.append(net)
        net = torch.cat((net, zc), 1)
        i += 1
    return leaves, torch.stack(mods), prefix


@pytest.mark.parametrize("index", range(N_CONFIGS))
def test_replica_reproduces_the_reference(fx, index):
    """ties tests/siren_replay.py (float64, hand-written adjoints) to the reference's fp32 run: with the bf16 roundings off it is the
    reference's arithmetic"""
    rec = fx["configs"][index]
    model = build(rec)
    fill_parameters(model, rec["seed"])
    state = model.state_dict()
    siren = model.siren if rec["kind"] == "img" else model
    leaves, mods, prefix = _front64(state, rec)
    rep = R.from_state(state, prefix, siren.num_layers, siren.has_bias, rounded=False)
    b = mods.shape[1]
    if "init" in rec:
        x = rec["init"].double().numpy().reshape(-1, siren.in_dim)
    else:
        x = np.tile(siren.grid[0].double().numpy(), (b, 1))
    n = x.shape[0] // b
    samp = np.repeat(np.arange(b), n)
    y, _ = rep.forward(x, samp, mods.detach().numpy())
    want = rec["y"].double()
    if rec["kind"] == "img":
        want = want.permute(0, 2, 3, 1)
    dy = rec["dy"].double().permute(0, 2, 3, 1) if rec["kind"] == "img" else rec["dy"].double()
    assert rel_l2(torch.from_numpy(y).view(-1), want.reshape(-1)) < 1e-5
    g = rep.backward(dy.reshape(-1, siren.out_dim).numpy())
    got = {}
    for l in range(siren.num_layers):
        got[f"{prefix}blocks.{l}.weight"] = g[f"w{l}"][0]
        if siren.has_bias:
            got[f"{prefix}blocks.{l}.bias"] = g[f"b{l}"][0]
    got[f"{prefix}head.weight"] = g["wh"][0]
    if siren.has_bias:
        got[f"{prefix}head.bias"] = g["bh"][0]
    got = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in got.items()}
    dm = torch.from_numpy(g["dmods"][0])
    if "mods" in rec:
        assert rel_l2(dm, rec["dmods"].double()) < 1e-5
        assert rel_l2(torch.from_numpy(g["dx"][0]).view(-1), rec["dinit"].double().view(-1)) < 1e-5
    else:
        names = [k for k in leaves if k not in got]
        outs = torch.autograd.grad(mods, [leaves[k] for k in names], grad_outputs=dm, allow_unused=True)
        for k, v in zip(names, outs):
            if k == "__z":
                assert rel_l2(v, rec["dz"].double()) < 1e-5
            else:
                got[k] = v
    assert set(got) == set(rec["grads"])
    for k, want_g in rec["grads"].items():
        have = got[k][::rec["grad_rows"][k]] if k in rec["grad_rows"] else got[k]
        assert rel_l2(have, want_g.double()) < 1e-5, (k, rel_l2(have, want_g.double()))


def test_replica_rounding_and_flip_bound():
    x = np.array([1.0, 1.00390625, 1.0 + 2.0 ** -8, -3.1415926, 0.0, 2.0 ** -130])
    want = torch.tensor(x, dtype=torch.float32).bfloat16().double().numpy()
    assert np.array_equal(R.rb(x), want)
    # exactly representable and far from a boundary: no flip within a small e; on a tie any e flips
    assert R.flip(np.array([1.5]), np.array([1e-6]))[0] == 0.0
    assert R.flip(np.array([1.0 + 2.0 ** -8]), np.array([1e-9]))[0] >= 2.0 ** -7
    # just above a power of two the lower boundary is a quarter spacing away
    assert R.flip(np.array([1.0]), np.array([2.0 ** -9 * 1.01]))[0] > 0.0 and R.flip(np.array([1.0]), np.array([2.0 ** -9 * 0.99]))[0] == 0.0


def test_refusals_and_quirks():
    for kw, needle in ((dict(latent_dim=48), "latent_dim = 48"), (dict(latent_dim=288), "latent_dim = 288"), (dict(in_dim=9), "in_dim = 9"),
                       (dict(in_dim=0), "in_dim = 0"), (dict(out_dim=17), "out_dim = 17"), (dict(num_layers=0), "num_layers = 0"),
                       (dict(final_activation="tanh"), "final_activation = 'tanh'")):
        base = dict(in_dim=2, out_dim=3, latent_dim=32, num_layers=2, final_activation=None)
        base.update(kw)
        with pytest.raises(NotImplementedError, match="DESIGN §8") as e:
            C.Siren(4, base.pop("in_dim"), base.pop("out_dim"), base.pop("latent_dim"), **base)
        assert needle in str(e.value)
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.ImgSiren(8, 3, 40)
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.ImgSiren(8, 17, 64)
    m = C.Siren(4, 2, 3, 32, num_layers=2, keep_edge=False)
    z = torch.zeros(2, 32)
    with pytest.raises(NotImplementedError, match=r"siren\.py:181-182.*DESIGN §8"):
        m(z, size=6)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(z)
    with pytest.raises(ValueError, match=r"\[B, 32\] latent expected"):
        m(torch.zeros(2, 16))
    d = C.Siren(None, 1, 2, 32, num_layers=2, bias=False, use_modulator=False)
    assert d.grid is None and d.modulator is None and d.head.bias is None and "grid" not in d.state_dict()
    mods = (torch.zeros(5, 32), torch.zeros(5, 32))
    with pytest.raises(ValueError, match="`init` should be provided"):
        d(mods)
    with pytest.raises(NotImplementedError, match=r"siren\.py:183.*DESIGN §8"):
        d(mods, size=4)
    with pytest.raises(ValueError, match="1 modulations for 2 layers"):
        d(mods[:1], init=torch.zeros(5, 7, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        d(mods, init=torch.zeros(5, 7, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        d(mods + (torch.zeros(5, 32),), init=torch.zeros(5, 7, 1))  # the first num_layers modulations are used, as zip does
    with pytest.raises(ValueError, match=r"`init` must be \[5, N, 1\]"):
        d(mods, init=torch.zeros(4, 7, 1))
    img = C.ImgSiren(8, 3, 64, num_classes=4)
    with pytest.raises(ValueError, match="`labels` should be provided"):
        img.decode(torch.zeros(2, 64), labels=None)
    with pytest.raises(NotImplementedError, match="latent_dim = 40"):
        ops.SirenShape(1, 1, 2, 40, 3, 2, 30.0, 1.0)


def test_ops_want_the_hip_device():
    sh = ops.SirenShape(2, 4, 2, 32, 3, 2, 30.0, 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.siren_pack([torch.zeros(32, 32)], torch.zeros(3, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.siren_fwd(sh, torch.zeros(8, 2), False, torch.zeros(32, 2), torch.zeros(8, dtype=torch.bfloat16), None, torch.zeros(2, 2, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sine_fwd(torch.zeros(4), 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sine_bwd(torch.zeros(4), torch.zeros(4), 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.siren_reduce(sh, torch.zeros(8), "dw0", torch.zeros(64))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.relu_f32_fwd(torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.relu_f32_bwd(torch.zeros(4), torch.zeros(4))


def test_build_activation_sine():
    act = C.modules.build_activation("sine", {"w": 30.0})
    assert isinstance(act, C.Sine) and act.w == 30.0 and not list(act.parameters()) and not act.state_dict()
    assert C.modules.build_activation("sine").w == 1.0
    with pytest.raises(RuntimeError, match="HIP device"):
        act(torch.zeros(3))
    for other in ("h_swish", "mish", "Tanh"):
        with pytest.raises(NotImplementedError, match="not on the accelerated hot path"):
            C.modules.build_activation(other)


def test_entries_declared_cited_and_built():
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, len(_lib.SIGNATURES[name][1]))
    assert sum(name.startswith(("cfhip_siren_", "cfhip_sine_", "cfhip_relu_f32_")) for name in _lib.SIGNATURES) == len(ENTRIES)
    assert ops.SIREN_MAX_LATENT == _lib.DEFINES["CFHIP_SIREN_MAX_LATENT"] == 256
    assert ops.SIREN_MAX_IN == _lib.DEFINES["CFHIP_SIREN_MAX_IN"] == 8 and ops.SIREN_MAX_OUT == _lib.DEFINES["CFHIP_SIREN_MAX_OUT"] == 16
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("(csrc/siren.hip)"):header.index("cfhip_relu_f32_bwd(")]
    for cite in ("siren.py:156-187", "siren.py:67-70", "siren.py:185-186", "siren.py:187", "siren.py:21-24", "siren.py:183", "siren.py:65"):
        assert cite in block, cite
    import __graft_entry__ as G

    assert "siren" in G.SOURCES
    script = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert re.search(r"^for f in .*\bsiren\b.*; do$", script, flags=re.M)
    source = open(os.path.join(ROOT, "carefree-learn_amd", "csrc", "siren.hip")).read()
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
    assert lib.cfhip_siren_pack_workspace(32, 32, 1) == 16 * 64 * 2 * 2 and lib.cfhip_siren_pack_workspace(3, 256, 1) == 16 * 64 * (8 + 16)
    assert lib.cfhip_siren_pack_workspace(32, 32, 0) == 16 * 64 * 2 and lib.cfhip_siren_pack_workspace(3, 256, 0) == 16 * 64 * 8  # the forward pack alone
    for t in (0, 1):
        assert lib.cfhip_siren_pack_workspace(32, 48, t) == 0 and lib.cfhip_siren_pack_workspace(0, 32, t) == 0
        assert lib.cfhip_siren_pack_workspace(257, 256, t) == 0
    _refused(lib.cfhip_siren_pack(p, p, 8, 32, 48, 1, None), "K = 48")
    _refused(lib.cfhip_siren_pack(None, p, 4096, 32, 32, 1, None), "null operand")
    _refused(lib.cfhip_siren_pack(p, p, 8, 32, 32, 1, None), "cfhip_siren_pack_workspace says")
    _refused(lib.cfhip_siren_pack(p, p, 4096, 32, 32, 0, None), "cfhip_siren_pack_workspace says")  # the size of the other form
    _refused(lib.cfhip_siren_pack(p, p + 8, 4096, 32, 32, 1, None), "misaligned")

    def fwd(x=p, ss=None, sc=None, b=2, n=4, din=2, h=32, dout=3, layers=2, packed=p):
        return lib.cfhip_siren_fwd(x, 0, p, packed, 0, None, p, p, ss, sc, b, n, din, h, dout, layers, 30.0, 1.0, None)

    _refused(fwd(x=None), "null operand")
    _refused(fwd(ss=p), "save_sin and save_cos together")
    _refused(fwd(h=48), "latent = 48")
    _refused(fwd(h=288), "latent = 288")
    _refused(fwd(din=9), "in_dim = 9")
    _refused(fwd(dout=17), "out_dim = 17")
    _refused(fwd(layers=0), "num_layers = 0")
    _refused(fwd(b=0), "B = 0")
    _refused(fwd(b=2 ** 20, n=2 ** 20), "M = B N")
    _refused(fwd(packed=p + 8), "16-byte aligned")
    _refused(fwd(x=p + 2), "misaligned")
    need = lib.cfhip_siren_bwd_workspace(2, 4, 2, 32, 3, 2)
    assert need == 4 * (1 * (2 * 32 + 32 * 2 + 3 * 32 + 16) + (1 + 2) * 2 * 32)
    assert lib.cfhip_siren_bwd_workspace(2, 4, 2, 48, 3, 2) == 0 and lib.cfhip_siren_bwd_workspace(0, 4, 2, 32, 3, 2) == 0

    def bwd(dy=p, ss=p, ws=p, ws_bytes=need, h=32):
        return lib.cfhip_siren_bwd(dy, p, 0, p, p, p, p, ss, p, None, None, None, ws, ws_bytes, 2, 4, 2, h, 3, 2, 30.0, 1.0, None)

    _refused(bwd(dy=None), "null operand")
    _refused(bwd(ss=None), "null operand")
    _refused(bwd(h=40), "latent = 40")
    _refused(bwd(ws_bytes=need - 4), "cfhip_siren_bwd_workspace says")
    _refused(bwd(ws=None), "cfhip_siren_bwd_workspace says")
    _refused(bwd(ws=p + 4), "16-byte aligned")

    def red(kind=0, layer=0, dest=p, acc=0, ws_bytes=need):
        return lib.cfhip_siren_reduce(p, ws_bytes, kind, layer, dest, acc, 2, 4, 2, 32, 3, 2, None)

    _refused(red(kind=5), "kind = 5")
    _refused(red(kind=-1), "kind = -1")
    _refused(red(layer=2), "layer = 2 of 2")
    _refused(red(dest=None), "null or misaligned destination")
    _refused(red(acc=2), "`accumulate` = 2")
    _refused(red(ws_bytes=8), "cfhip_siren_bwd_workspace says")
    _refused(lib.cfhip_sine_fwd(None, p, 4, 1.0, None), "null operand")
    _refused(lib.cfhip_sine_fwd(p, p, 0, 1.0, None), "n = 0")
    _refused(lib.cfhip_sine_bwd(p, p, None, 4, 1.0, None), "null operand")
    _refused(lib.cfhip_sine_bwd(p, p + 2, p, 4, 1.0, None), "misaligned")
    _refused(lib.cfhip_relu_f32_fwd(p, None, 4, None), "null operand")
    _refused(lib.cfhip_relu_f32_fwd(p, p, -1, None), "n = -1")
    _refused(lib.cfhip_relu_f32_bwd(p, None, p, 4, None), "null operand")
    _refused(lib.cfhip_relu_f32_bwd(p + 1, p, p, 4, None), "misaligned")
