"""ml_rnn without a GPU: the registry entry, state-dict parity with the reference's recorded keys, checkpoint round trips, the C-ABI
declarations and build lists, every refusal that must fire before a launch, and the float64 one-step replica of tests/rnn_replay.py
against torch.nn.GRU / nn.LSTM and torch.autograd.gradcheck."""
import os
import re

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops

import rnn_replay as R
from rnn_weights import fill_parameters, seeded_state, step_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cfhip_rnn_pack_workspace", "cfhip_rnn_pack", "cfhip_rnn_fwd", "cfhip_rnn_bwd")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rnn_small.pt")


def test_registry_and_export():
    assert C.module_dict["ml_rnn"] is C.RNN
    m = C.build_module("ml_rnn", input_dim=6, output_dim=2, hidden_size=8, hidden_units=[16], unknown_keyword=1)
    assert isinstance(m, C.RNN) and isinstance(m.head, C.FCNN)
    assert all(p.dtype == torch.float32 for p in m.parameters())


@pytest.mark.parametrize("index", range(4))
def test_state_dict_matches_reference(fx, index):
    rec = fx["states"][index]
    m = C.RNN(**rec["kwargs"])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in rec["state"]], rec["name"]


@pytest.mark.parametrize("index", range(4))
def test_checkpoint_round_trip(fx, index):
    rec = fx["states"][index]
    m = C.RNN(**rec["kwargs"])
    state = {k: torch.randn(s, generator=torch.Generator().manual_seed(i)) for i, (k, s) in enumerate(rec["state"])}
    m.load_state_dict(state, strict=True)
    back = m.state_dict()
    assert list(back) == list(state) and all(torch.equal(back[k], state[k]) for k in state)
    # the other way: torch's own layers (what the reference's rnn_list holds) take this module's tensors
    kw = rec["kwargs"]
    ref = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM}[kw.get("cell", "GRU")](
        kw["input_dim"], kw.get("hidden_size", 256), batch_first=True, bidirectional=kw.get("bidirectional", False))
    ref.load_state_dict(m.rnn_list[0].state_dict(), strict=True)


def test_init_is_orthogonal_weights_zero_biases():
    torch.manual_seed(3)
    m = C.RNN(12, 2, cell="LSTM", hidden_size=16, bidirectional=True)
    for name, p in m.rnn_list.named_parameters():
        if "bias" in name:
            assert not p.any(), name
        else:
            q = p if p.shape[0] <= p.shape[1] else p.t()
            assert torch.allclose(q @ q.t(), torch.eye(q.shape[0]), atol=1e-5), name


def test_entries_declared_cited_and_built():
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    block = header[header.index("GRU / LSTM recurrence"):header.index("cfhip_rnn_bwd(")]
    for cite in ("ml/rnn.py:13-17", "ml/rnn.py:53-80", "ml/rnn.py:82-85"):
        assert cite in block, cite
    import __graft_entry__ as G

    assert "rnn" in G.SOURCES
    script = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert re.search(r"^for f in .*\brnn\b.*; do$", script, flags=re.M)
    assert os.path.isfile(os.path.join(ROOT, "carefree-learn_amd", "csrc", "rnn.hip"))


def _refused(rc, needle):
    assert rc != 0
    msg = _lib.load().cfhip_last_error().decode()
    assert needle in msg, msg


def test_c_refusals_fire_before_any_launch():
    """no device is touched: the pointers are made-up addresses (16-byte aligned), every call must return before its launch"""
    lib = _lib.load()
    p = 4096

    def fwd(gx=p, cell=0, h=8, ldy=8, b=1, t=1):
        return lib.cfhip_rnn_fwd(gx, p, p, None, None, p, ldy, None, None, None, None, None, cell, b, t, h, 0, None)

    for h in (0, 12, 264):
        _refused(fwd(h=h, ldy=512), f"H = {h}")
        _refused(lib.cfhip_rnn_pack(p, p, 0, 0, h, None), f"H = {h}")
        _refused(lib.cfhip_rnn_bwd(None, 0, None, None, p, p, 512, None, None, p, None, p, p, None, None, 0, 1, 1, h, 0, None), f"H = {h}")
        assert lib.cfhip_rnn_pack_workspace(0, h) == 0
    _refused(fwd(gx=None), "null operand")
    _refused(fwd(cell=2), "unknown cell id 2")
    _refused(lib.cfhip_rnn_pack(p, p, 0, 7, 8, None), "unknown cell id 7")
    _refused(fwd(h=16, ldy=8), "smaller than H")
    _refused(fwd(b=0), "B = 0")
    _refused(fwd(t=0), "T = 0")
    _refused(lib.cfhip_rnn_pack(p, p, 16, 0, 8, None), "cfhip_rnn_pack_workspace says")
    _refused(lib.cfhip_rnn_bwd(None, 0, None, None, p, p, 8, None, None, None, None, p, p, None, None, 0, 1, 1, 8, 0, None), "null operand")
    _refused(lib.cfhip_rnn_bwd(None, 0, None, None, p, None, 0, None, None, p, None, p, None, None, None, 1, 1, 1, 8, 0, None), "LSTM needs cseq")
    # two packs (forward and transposed), G * Np * Kp bf16 each
    assert lib.cfhip_rnn_pack_workspace(0, 40) == 2 * 2 * 3 * 48 * 64
    assert lib.cfhip_rnn_pack_workspace(1, 256) == 2 * 2 * 4 * 256 * 256


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="tanh cell"):
        C.RNN(8, 2, cell="RNN")
    for h in (4, 12, 264):
        with pytest.raises(NotImplementedError, match="outside the recurrent kernels"):
            C.RNN(8, 2, hidden_size=h)
    with pytest.raises((KeyError, ValueError)):
        C.RNN(8, 2, cell="QRNN")
    with pytest.raises(NotImplementedError, match="mapping type"):
        C.RNN(8, 2, hidden_size=8, mapping_type="highway")
    with pytest.raises(RuntimeError, match="HIP device"):
        C.RNN(8, 2, hidden_size=8)(torch.zeros(2, 3, 8))
    with pytest.raises(NotImplementedError):
        C.rnn.GRU(8, 12)


def test_only_the_first_layer_takes_two_word_input():
    m = C.RNN(10, 2, num_layers=3, hidden_size=8, bidirectional=True)
    assert [layer.two_word_input for layer in m.rnn_list] == [True, False, False]
    assert C.rnn.GRU(10, 8).two_word_input is False


def test_seeded_state_loads(fx):
    rec = fx["configs"][3]
    m = C.RNN(**rec["kwargs"])
    m.load_state_dict(seeded_state(m, rec["seed"]))
    ref = C.RNN(**rec["kwargs"])
    fill_parameters(ref, rec["seed"])
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))


# ---- the float64 replica --------------------------------------------------------------------------------------------------------------


def _step_case(fx, cell):
    st = fx["steps"][cell]
    layer, x, h0, c0 = step_tensors(cell, st["seed"])
    assert torch.equal(x, st["x"]) and torch.equal(h0, st["h0"]) and torch.equal(c0, st["c0"])
    gx = st["x"][:, 0] @ layer.weight_ih_l0.detach().t() + layer.bias_ih_l0.detach()
    return layer, st["x"], st["h0"], st["c0"], gx, layer.weight_hh_l0.detach(), layer.bias_hh_l0.detach()


def test_replica_gru_step_matches_torch(fx):
    layer, x, h0, _, gx, w, b = _step_case(fx, "GRU")
    h0g = h0.clone().requires_grad_(True)
    out, hn = layer(x, h0g[None])
    got, gates = R.gru_step(gx, h0, w, b)
    assert (got - out[:, 0].detach()).abs().max() < 1e-11 and (got - hn[0].detach()).abs().max() < 1e-11
    dh = torch.randn(got.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gxg = gx.clone().requires_grad_(True)
    hg = h0.clone().requires_grad_(True)
    R.gru_step(gxg, hg, w, b)[0].backward(dh)
    dgx, dgh, dhp = R.gru_step_bwd(dh, h0, w, gates)
    assert (dgx - gxg.grad).abs().max() < 1e-11 and (dhp - hg.grad).abs().max() < 1e-11
    (out[:, 0] * dh).sum().backward()
    assert (dhp - h0g.grad).abs().max() < 1e-11
    assert (dgh.t() @ h0 - layer.weight_hh_l0.grad).abs().max() < 1e-11 and (dgh.sum(0) - layer.bias_hh_l0.grad).abs().max() < 1e-11
    assert (dgx.sum(0) - layer.bias_ih_l0.grad).abs().max() < 1e-11


def test_replica_lstm_step_matches_torch(fx):
    layer, x, h0, c0, gx, w, b = _step_case(fx, "LSTM")
    h0g, c0g = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    out, (hn, cn) = layer(x, (h0g[None], c0g[None]))
    got_h, got_c, gates = R.lstm_step(gx, h0, c0, w, b)
    assert (got_h - out[:, 0].detach()).abs().max() < 1e-11 and (got_c - cn[0].detach()).abs().max() < 1e-11
    gen = torch.Generator().manual_seed(2)
    dh = torch.randn(got_h.shape, generator=gen, dtype=torch.float64)
    dc = torch.randn(got_h.shape, generator=gen, dtype=torch.float64)
    ((hn[0] * dh).sum() + (cn[0] * dc).sum()).backward()
    dgx, dgh, dhp, dcp = R.lstm_step_bwd(dh, dc, c0, got_c, w, gates)
    assert dgh is dgx
    assert (dhp - h0g.grad).abs().max() < 1e-11 and (dcp - c0g.grad).abs().max() < 1e-11
    assert (dgh.t() @ h0 - layer.weight_hh_l0.grad).abs().max() < 1e-11 and (dgx.sum(0) - layer.bias_ih_l0.grad).abs().max() < 1e-11


class _GruStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gx, h, w, b):
        out, gates = R.gru_step(gx, h, w, b)
        ctx.save_for_backward(h, w, *gates)
        return out

    @staticmethod
    def backward(ctx, dh):
        h, w, *gates = ctx.saved_tensors
        dgx, dgh, dhp = R.gru_step_bwd(dh, h, w, gates)
        return dgx, dhp, dgh.t() @ h, dgh.sum(0)


class _LstmStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gx, h, c, w, b):
        hn, cn, gates = R.lstm_step(gx, h, c, w, b)
        ctx.save_for_backward(h, c, cn, w, *gates)
        return hn, cn

    @staticmethod
    def backward(ctx, dh, dc):
        h, c, cn, w, *gates = ctx.saved_tensors
        dgx, dgh, dhp, dcp = R.lstm_step_bwd(dh, dc, c, cn, w, gates)
        return dgx, dhp, dcp, dgh.t() @ h, dgh.sum(0)


def test_replica_backward_passes_gradcheck(fx):
    _, _, h0, _, gx, w, b = _step_case(fx, "GRU")
    args = [t.clone().requires_grad_(True) for t in (gx, h0, w, b)]
    assert torch.autograd.gradcheck(_GruStep.apply, args, eps=1e-6, atol=1e-7)
    _, _, h0, c0, gx, w, b = _step_case(fx, "LSTM")
    args = [t.clone().requires_grad_(True) for t in (gx, h0, c0, w, b)]
    assert torch.autograd.gradcheck(_LstmStep.apply, args, eps=1e-6, atol=1e-7)
