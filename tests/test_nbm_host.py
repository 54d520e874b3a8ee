"""nbm without a GPU: the registry entry, state-dict parity with the reference's recorded keys, checkpoint round trips, nn.Conv1d's
init bounds, every refusal by name, the C-ABI declarations, build lists and host-side argument checks, the float64 replica of
tests/nbm_replay.py (roundings off) against the reference's recorded fp32 logits and gradients, and the condition the per-element GPU
cases rest on: the share of hidden units inside the zero band, computed from the replica alone, is below 1 %."""
import math
import os
import re

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops

import nbm_replay as R
from helpers import rel_l2
from nbm_weights import KERNEL_CASES, fill_parameters, kernel_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cfhip_nbm_pack_workspace", "cfhip_nbm_pack", "cfhip_nbm_bases_fwd", "cfhip_nbm_bases_bwd_workspace", "cfhip_nbm_bases_bwd",
           "cfhip_nbm_featurize_fwd", "cfhip_nbm_featurize_bwd_workspace", "cfhip_nbm_featurize_bwd")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("nbm_small.pt")


def test_registry_and_export():
    assert C.module_dict["nbm"] is C.NBM
    m = C.build_module("nbm", input_dim=6, output_dim=2, num_bases=4, hidden_units=[8, 8], unknown_keyword=1)
    assert isinstance(m, C.NBM) and m.latent_dim == 6 and m.nary == {"1": [(i,) for i in range(6)]}
    assert all(p.dtype == torch.float32 for p in m.parameters())
    assert C.NBM(68, 2).bases["1"].hidden == 136 and C.NBM(4, 2).bases["1"].hidden == 32  # 2 * [max(32, min(1024, 2 input_dim))]


@pytest.mark.parametrize("index", range(4))
def test_state_dict_matches_reference(fx, index):
    rec = fx["states"][index]
    m = C.NBM(**rec["kwargs"])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in rec["state"]], rec["name"]


@pytest.mark.parametrize("index", range(4))
def test_checkpoint_round_trip(fx, index):
    rec = fx["states"][index]
    m = C.NBM(**rec["kwargs"])
    state = {k: torch.randn(s, generator=torch.Generator().manual_seed(i)) for i, (k, s) in enumerate(rec["state"])}
    m.load_state_dict(state, strict=True)
    back = m.state_dict()
    assert list(back) == list(state) and all(torch.equal(back[k], state[k]) for k in state)
    # the other way: torch's own layers (what the reference's blocks hold) take this module's tensors
    for order, block in m.bases.items():
        o, nb, h = int(order), m.num_bases, block.hidden
        for i, (cin, cout) in enumerate(((o, h), (h, h), (h, 1))):
            torch.nn.Conv1d(cin * nb, cout * nb, 1, groups=nb).load_state_dict(block.net[i].conv.state_dict(), strict=True)
    torch.nn.Conv1d(m.latent_dim * m.num_bases, m.latent_dim, 1, groups=m.latent_dim).load_state_dict(m.featurizer.state_dict(), strict=True)
    torch.nn.Linear(m.latent_dim, m.output_dim).load_state_dict(m.head.state_dict(), strict=True)


def test_init_is_conv1d_and_linear_default():
    torch.manual_seed(5)
    m = C.NBM(6, 3, nary={"1": [(0,), (5,)], "2": [(1, 2)]}, num_bases=16, hidden_units=[24, 24])
    seen = 0
    for name, p in m.named_parameters():
        if ".conv." in name:
            block = m.bases[name.split(".")[1]]
            fan_in = block.net[int(name.split(".")[3])].in_dim  # the inputs of one output unit inside its group
        elif name.startswith("featurizer"):
            fan_in = m.num_bases
        else:
            fan_in = m.latent_dim
        bound = 1.0 / math.sqrt(fan_in)
        assert float(p.abs().max()) <= bound, (name, float(p.abs().max()), bound)
        assert p.numel() < 32 or float(p.abs().max()) > 0.5 * bound, name
        seen += 1
    assert seen == 16


def test_constructor_refusals():
    cases = [
        (dict(batch_norm=True), "batch_norm = True"),
        (dict(dropout=0.1), "dropout = 0.1 inside the bases"),
        (dict(activation="GELU"), "activation 'GELU'"),
        (dict(bias=False), "bias = False"),
        (dict(hidden_units=[32, 64]), "exactly two equal widths"),
        (dict(hidden_units=[32, 32, 32]), "exactly two equal widths"),
        (dict(hidden_units=[32]), "exactly two equal widths"),
        (dict(hidden_units=[12, 12]), "exactly two equal widths"),
        (dict(hidden_units=[264, 264]), "exactly two equal widths"),
        (dict(nary={"5": [(0, 1, 2, 3, 4)]}), "order 5"),
    ]
    for kw, needle in cases:
        with pytest.raises(NotImplementedError, match=re.escape(needle)) as info:
            C.NBM(8, 2, **kw)
        assert "DESIGN §8" in str(info.value), kw
    with pytest.raises(NotImplementedError, match="DESIGN §8"):
        C.NBM(200, 2)  # the default width 2 * 200 = 400 is past the kernels
    with pytest.raises(ValueError, match="length of every tuple"):
        C.NBM(8, 2, nary={"2": [(0, 1, 2)]})
    with pytest.raises(ValueError, match="outside"):
        C.NBM(4, 2, nary={"1": [(4,)]})
    C.NBM(8, 2, dropout=0.0, bases_dropout=0.3, hidden_units=[256, 256])  # what IS built
    with pytest.raises(RuntimeError, match="HIP device"):
        C.NBM(8, 2)(torch.zeros(2, 8))
    with pytest.raises(ValueError, match="not in the pre-defined nary"):
        C.NBM(8, 2).inspect(torch.zeros(2, 8), (0, 1), 0)


def test_entries_declared_cited_and_built():
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("NBM, the neural basis model"):header.index("cfhip_nbm_featurize_bwd(")]
    for cite in ("ml/nbm.py:54-120", "ml/nbm.py:18-51", "ml/nbm.py:168-174"):
        assert cite in block, cite
    import __graft_entry__ as G

    assert "nbm" in G.SOURCES
    script = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert re.search(r"^for f in .*\bnbm\b.*; do$", script, flags=re.M)
    source = open(os.path.join(ROOT, "carefree-learn_amd", "csrc", "nbm.hip")).read()
    assert "atomic" not in source.replace("No floating-point atomics", "")


def _refused(rc, needle):
    assert rc == -1, rc
    msg = _lib.load().cfhip_last_error().decode()
    assert needle in msg, msg


def test_c_refusals_fire_before_any_launch():
    """no device is touched: the pointers are made-up addresses (16-byte aligned), every call must return before its launch"""
    lib = _lib.load()
    p = 4096

    def fwd(x=p, h=8, o=1, nb=2, b=1, d=1):
        return lib.cfhip_nbm_bases_fwd(x, 4, p, p, p, p, p, p, p, p, b, d, nb, h, o, None)

    def bwd(dbases=p, h=8, o=1, ws=p, ws_bytes=1 << 30, acc=0):
        return lib.cfhip_nbm_bases_bwd(dbases, p, 4, p, p, p, p, p, p, None, None, p, None, None, None, None, acc, ws, ws_bytes, 1, 1, 4, 2, h, o, None)

    for h in (0, 12, 264):
        _refused(fwd(h=h), f"H = {h}")
        _refused(bwd(h=h), f"H = {h}")
        _refused(lib.cfhip_nbm_pack(p, p, 0, 2, h, None), f"H = {h}")
        assert lib.cfhip_nbm_pack_workspace(2, h) == 0 and lib.cfhip_nbm_bases_bwd_workspace(16, 2, h, 1, 0) == 0
    _refused(fwd(o=5), "order = 5")
    _refused(bwd(o=5), "order = 5")
    _refused(fwd(o=0), "order = 0")
    assert lib.cfhip_nbm_bases_bwd_workspace(16, 2, 8, 5, 0) == 0
    _refused(fwd(x=None), "null operand")
    _refused(bwd(dbases=None), "null operand")
    _refused(bwd(ws=None), "null operand")
    _refused(fwd(nb=0), "NB = 0")
    _refused(fwd(b=0), "B = 0")
    _refused(fwd(b=2 ** 20, d=2 ** 11), "rows")
    _refused(bwd(ws_bytes=16), "cfhip_nbm_bases_bwd_workspace says")
    _refused(bwd(acc=64), "`accumulate` = 64")
    _refused(lib.cfhip_nbm_pack(None, p, 0, 2, 8, None), "null operand")
    _refused(lib.cfhip_nbm_pack(p, p, 16, 2, 8, None), "cfhip_nbm_pack_workspace says")
    _refused(lib.cfhip_nbm_featurize_fwd(None, p, p, p, 1, 1, 1, None), "null operand")
    _refused(lib.cfhip_nbm_featurize_fwd(p, p, p, p, 0, 1, 1, None), "B = 0")
    _refused(lib.cfhip_nbm_featurize_bwd(None, p, p, p, p, p, 0, p, 1 << 20, 1, 1, 1, None), "null operand")
    _refused(lib.cfhip_nbm_featurize_bwd(p, None, p, p, p, p, 0, p, 1 << 20, 1, 1, 1, None), "bases for dwf")
    _refused(lib.cfhip_nbm_featurize_bwd(p, p, p, p, p, p, 0, p, 4, 1, 1, 1, None), "cfhip_nbm_featurize_bwd_workspace says")
    # two packs (forward and transposed) of NB * Np * Kp bf16 each
    assert lib.cfhip_nbm_pack_workspace(3, 40) == 2 * 2 * 3 * 48 * 64
    assert lib.cfhip_nbm_pack_workspace(64, 256) == 2 * 2 * 64 * 256 * 256


def test_workspace_grows_with_rows_and_is_never_zero():
    lib = _lib.load()
    for nb, h, o in ((1, 8, 1), (3, 40, 2), (64, 32, 1), (64, 256, 4)):
        for dx in (0, 1):
            sizes = [lib.cfhip_nbm_bases_bwd_workspace(m, nb, h, o, dx) for m in (1, 17, 65, 300, 4096, 65536)]
            assert all(s > 0 for s in sizes), sizes
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], (nb, h, o, dx, sizes)
            if dx:
                assert sizes[-1] >= 4 * nb * 65536 * o
            # nothing of M NB H elements: the row chunks stop growing (at most 4096 / NB and 2048 / (NB NT) of them, reached by
            # M = 2^19), past that the only growth is the [NB][M][o] partial of dx
            big, bigger = (lib.cfhip_nbm_bases_bwd_workspace(2 ** e, nb, h, o, dx) for e in (21, 22))
            assert 0 <= bigger - big <= dx * 4 * nb * 2 ** 21 * o + 256, (nb, h, o, dx)
    assert lib.cfhip_nbm_featurize_bwd_workspace(1, 1, 1) > 0
    assert lib.cfhip_nbm_featurize_bwd_workspace(10 ** 6, 12, 64) == lib.cfhip_nbm_featurize_bwd_workspace(10 ** 5, 12, 64)


def test_ops_refuse_before_the_library():
    with pytest.raises(ValueError, match=r"feature columns must lie in \[0, 3\)"):
        ops.nbm_index([(0,), (3,)], 1, 3, "cpu")
    idx = ops.nbm_index([(0, 2), (1, 1)], 2, 3, "cpu")
    assert idx.table.dtype == torch.int32 and idx.table.tolist() == [[0, 2], [1, 1]] and idx.features == 3 and tuple(idx.shape) == (2, 2)
    with pytest.raises(ValueError, match="int32"):
        ops.NbmIndex(torch.zeros(2, 2, dtype=torch.int64), 3)
    with pytest.raises(TypeError, match="NbmIndex"):
        ops.nbm_bases(torch.zeros(1, 3), idx.table, *([torch.zeros(1)] * 6))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.nbm_pack(torch.zeros(2, 8, 8))
    assert ops.nbm_hidden_ok(8) and ops.nbm_hidden_ok(256) and not ops.nbm_hidden_ok(12) and not ops.nbm_hidden_ok(264)


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_zero_band_share_of_the_kernel_cases(name):
    """the per-element GPU cases check every element with the flipped-mask magnitude inside the bound; that bound stays sharp only
    while few units sit in the zero band.  From the replica alone: below 1 % in every case (seeds chosen for it)."""
    h, nb, b, f, idx, seed = KERNEL_CASES[name]
    case = kernel_case(h, nb, b, f, idx, seed)
    rp = R.Replay(case)
    share = rp.zero_band_share()
    live1, live2 = float((rp.pre1 > 0).double().mean()), float((rp.pre2 > 0).double().mean())
    print(f"{name}: zero-band share {share:.2e}, live {live1:.2f} / {live2:.2f}, bases std {float(rp.bases.std()) if rp.bases.numel() > 1 else 0:.2f}")
    assert share < 0.01, share
    assert 0.25 < live1 < 0.75 and 0.25 < live2 < 0.75, (live1, live2)
    # dyadic layer-1 operands: pre1 is exact in f32 (the replica's float64 value is an f32 value)
    assert torch.equal(rp.pre1.float().double(), rp.pre1)
    dp2 = case["dbases"].double().reshape(rp.m, nb)[:, :, None] * rp.w3
    assert torch.equal(dp2.float().double(), dp2)


# ---- the float64 replica, roundings off, against the reference's fp32 record ------------------------------------------------------------


def module_replay(model, rec, rounding: bool):
    """float64 logits, features and gradients of `model` for the record's x / dy through tests/nbm_replay.py"""
    x, dy = rec["x"], rec["dy"].double()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    nb = model.num_bases
    plays, outs = [], []
    for order, indices in model.nary.items():
        pre = f"bases.{order}.net."
        h = sd[pre + "0.conv.bias"].numel() // nb
        case = dict(x=x, idx=indices, w1=sd[pre + "0.conv.weight"].view(nb, h, int(order)), b1=sd[pre + "0.conv.bias"].view(nb, h),
                    w2=sd[pre + "1.conv.weight"].view(nb, h, h), b2=sd[pre + "1.conv.bias"].view(nb, h),
                    w3=sd[pre + "2.conv.weight"].view(nb, h), b3=sd[pre + "2.conv.bias"])
        rp = R.Replay(case, round_h1=rounding, round_w2=rounding, round_dp2=rounding)
        plays.append((order, rp))
        outs.append(rp.bases.view(rp.b, rp.d, nb))
    bases = torch.cat(outs, 1)
    wf, bf = sd["featurizer.weight"].double().view(-1, nb), sd["featurizer.bias"].double()
    feat, _ = R.featurize(bases, wf, bf)
    wh, bh = sd["head.weight"].double(), sd["head.bias"].double()
    y = feat @ wh.t() + bh
    grads = {"head.weight": dy.t() @ feat, "head.bias": dy.sum(0)}
    fg, _ = R.featurize_backward(dy @ wh, bases, wf)
    grads["featurizer.weight"], grads["featurizer.bias"] = fg["dwf"].view(-1, nb, 1), fg["dbf"]
    dx, at = torch.zeros_like(x, dtype=torch.float64), 0
    for order, rp in plays:
        g, _ = rp.backward(fg["dbases"][:, at:at + rp.d])
        at += rp.d
        pre = f"bases.{order}.net."
        for i, (w, b) in enumerate((("dw1", "db1"), ("dw2", "db2"), ("dw3", "db3"))):
            grads[f"{pre}{i}.conv.weight"] = g[w].reshape(sd[f"{pre}{i}.conv.weight"].shape)
            grads[f"{pre}{i}.conv.bias"] = g[b].reshape(-1)
        dx += g["dx"]
    return y, feat, grads, dx


@pytest.mark.parametrize("index", range(4))
def test_replica_without_roundings_reproduces_the_reference(fx, index):
    rec = fx["configs"][index]
    model = C.NBM(**rec["kwargs"])
    fill_parameters(model, rec["seed"])
    y, feat, grads, dx = module_replay(model, rec, rounding=False)
    assert rel_l2(y, rec["y"]) < 1e-5 and rel_l2(feat, rec["feat"]) < 1e-5 and rel_l2(dx, rec["dx"]) < 1e-5
    assert set(grads) == set(rec["grads"])
    for k, want in rec["grads"].items():
        got = grads[k][::rec["grad_rows"][k]] if k in rec["grad_rows"] else grads[k]
        assert rel_l2(got, want) < 1e-5, (k, rel_l2(got, want))
    # and with the kernels' three bf16 roundings on it stays inside the reference's own bf16 distance
    y16, _, _, _ = module_replay(model, rec, rounding=True)
    assert rel_l2(y16, rec["y"]) <= rec["y_dist"], (rel_l2(y16, rec["y"]), rec["y_dist"])
