"""The recurrent kernels of csrc/rnn.hip and the ml_rnn module on the GPU.

Single steps (T = 1) are checked per element against the float64 replica of tests/rnn_replay.py, fed the operands the kernel multiplies
(bf16(h0), bf16(W_hh)).  The forward bound is the replica's `gru_bound` / `lstm_bound`: the error model written out of the operation
order in the header of csrc/rnn.hip ((H + 2) u on the pre-activations' absolute sums, 4 u per sigmoid, 9 u per tanh, one u per
remaining operation), handed to helpers.assert_elementwise as `cond` with k = 1, plus one ulp of the f32 result.  The backward step is
fed the gate values the forward kernel saved, so its bound covers the backward arithmetic alone: at most 10 (GRU) / 29 (LSTM) f32
roundings on the product of the operands' absolute values before the one bf16 rounding of dgx / dgh (k = 12 / 32, one bf16 ulp), and
for the carry dh0 the bf16 rounding of the dgh operand (2^-9 relative = 2^15 u) and a chain of G Kp additions on |dgh| |W_hh|.
Everything longer than one step is checked bit for bit: one launch of T steps against T chained one-step launches."""
import pytest
import torch

from helpers import assert_elementwise, bf16_round, guarded_ops, rel_l2
import rnn_replay as R
from rnn_weights import fill_parameters

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CELLS = {"GRU": ops.RNN_GRU, "LSTM": ops.RNN_LSTM}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rnn_small.pt")


def _case(cell, b, t, h, seed=0):
    """device operands of one direction: gx [B, T, G H], W_hh, b_hh, h0, c0, dy [B, T, H], dhT, dcT (f32)"""
    gen = torch.Generator().manual_seed(1000 * h + 10 * b + t + seed)
    g = ops.RNN_GATES[CELLS[cell]]
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    out = dict(gx=rn(b, t, g * h), w=rn(g * h, h) * (1.5 / h ** 0.5), bias=rn(g * h) * 0.3, h0=rn(b, h) * 0.5, c0=rn(b, h),
               dy=rn(b, t, h), dhT=rn(b, h), dcT=rn(b, h))
    return {k: v.to(DEV) for k, v in out.items()}


def _d(t):
    return t.detach().cpu().double()


def _kp(h):
    return (h + 31) // 32 * 32


@pytest.mark.parametrize("b", [1, 17, 33])
@pytest.mark.parametrize("h", [8, 40, 256])
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_single_step_per_element(cell, h, b):
    cid, lstm = CELLS[cell], cell == "LSTM"
    g = ops.RNN_GATES[cid]
    c = _case(cell, b, 1, h)
    packed = ops.rnn_pack(c["w"], cid)
    w64, b64, gx64 = _d(bf16_round(c["w"])), _d(c["bias"]), _d(c["gx"][:, 0])
    for given in (True, False):
        for reverse in (False, True):
            tag = f"{cell} H={h} B={b} {'h0' if given else 'null'} {'rev' if reverse else 'fwd'}"
            h0 = c["h0"] if given else None
            c0 = c["c0"] if given and lstm else None
            y, hT, cT, saved = ops.rnn_fwd(c["gx"], packed, c["bias"], cid, h0=h0, c0=c0, reverse=reverse, save=True, want_state=True)
            gates, cseq, hprev = saved
            h64 = _d(h0) if given else torch.zeros(b, h, dtype=torch.float64)
            c64 = _d(c0) if c0 is not None else torch.zeros(b, h, dtype=torch.float64)
            hmat = _d(bf16_round(h64.float()))
            assert torch.equal(hprev[:, 0].cpu(), h64.float().to(BF16)), tag
            assert torch.equal(y[:, 0], hT), tag
            if not lstm:
                want, gw = R.gru_step(gx64, h64, w64, b64, h_mat=hmat)
                assert_elementwise(hT, want, out_dtype=F32, ulps=1, cond=R.gru_bound(gx64, h64, w64, b64, hmat, gw), k=1, what=f"{tag} hT")
            else:
                want, want_c, gw = R.lstm_step(gx64, h64, c64, w64, b64, h_mat=hmat)
                bh, bc = R.lstm_bound(gx64, c64, w64, b64, hmat, gw)
                assert_elementwise(cT, want_c, out_dtype=F32, ulps=1, cond=bc, k=1, what=f"{tag} cT")
                assert_elementwise(hT, want, out_dtype=F32, ulps=1, cond=bh, k=1, what=f"{tag} hT")
                assert torch.equal(cseq[:, 0], cT), tag
            # the saved gates against the replica's (the widest of the gate bounds: a tanh on an (H + 2) u pre-activation)
            pre = (h + 2) * (gx64.abs() + hmat.abs() @ w64.abs().t() + b64.abs())
            if not lstm:
                pre_n = pre[:, 2 * h:] + gw[3].abs() * (pre[:, :h] / 4 + R.SIG_U) + gx64[:, 2 * h:].abs() + (gw[0] * gw[3]).abs()
                gate_bound = torch.cat([pre[:, :h] / 4, pre[:, h:2 * h] / 4, pre_n, pre[:, 2 * h:]], 1) + R.TANH_U
            else:
                gate_bound = pre + R.TANH_U
            assert_elementwise(gates[:, 0], torch.cat(gw, 1), out_dtype=F32, ulps=1, cond=gate_bound, k=1, what=f"{tag} gates")

            # ---- the backward step, on the gates the kernel saved ----
            dgx, dgh, dh0, dc0 = ops.rnn_bwd(c["dy"], packed, cid, saved, y, h0=h0, c0=c0, dhT=c["dhT"], dcT=c["dcT"] if lstm else None,
                                             reverse=reverse, want_dstate=True)
            gk = [_d(gates[:, 0, i * h:(i + 1) * h]) for i in range(4)]
            dh = _d(c["dy"][:, 0]) + _d(c["dhT"])
            kchain = 2 ** 15 + g * _kp(h)
            if not lstm:
                wgx, wgh, wdh0 = R.gru_step_bwd(dh, h64, w64, gk)
                cond = (dh.abs() * (1 + h64.abs() + gk[2].abs()) * (1 + gk[3].abs())).repeat(1, 3)
                assert_elementwise(dgx[:, 0], wgx, out_dtype=BF16, ulps=1, cond=cond, k=12, what=f"{tag} dgx")
                assert_elementwise(dgh[:, 0], wgh, out_dtype=BF16, ulps=1, cond=cond, k=12, what=f"{tag} dgh")
                assert_elementwise(dh0, wdh0, out_dtype=F32, ulps=1, cond=dh.abs() + cond @ w64.abs(), k=kchain + 16, what=f"{tag} dh0")
                assert dc0 is None
            else:
                dc = _d(c["dcT"])
                wgx, _, wdh0, wdc0 = R.lstm_step_bwd(dh, dc, c64, _d(cseq[:, 0]), w64, gk)
                base = dc.abs() + dh.abs()
                cond = (base * (1 + c64.abs())).repeat(1, 4)
                assert dgh is dgx
                assert_elementwise(dgx[:, 0], wgx, out_dtype=BF16, ulps=1, cond=cond, k=32, what=f"{tag} dgx")
                assert_elementwise(dc0, wdc0, out_dtype=F32, ulps=1, cond=base, k=32, what=f"{tag} dc0")
                assert_elementwise(dh0, wdh0, out_dtype=F32, ulps=1, cond=cond @ w64.abs(), k=kchain + 32, what=f"{tag} dh0")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("t", [2, 7])
@pytest.mark.parametrize("b,h", [(17, 40), (33, 256)])
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_one_launch_equals_chained_steps(cell, b, h, t, reverse):
    cid, lstm = CELLS[cell], cell == "LSTM"
    c = _case(cell, b, t, h, seed=5)
    packed = ops.rnn_pack(c["w"], cid)
    c0, dcT = (c["c0"], c["dcT"]) if lstm else (None, None)
    y, hT, cT, saved = ops.rnn_fwd(c["gx"], packed, c["bias"], cid, h0=c["h0"], c0=c0, reverse=reverse, save=True, want_state=True)
    dgx, dgh, dh0, dc0 = ops.rnn_bwd(c["dy"], packed, cid, saved, y, h0=c["h0"], c0=c0, dhT=c["dhT"], dcT=dcT, reverse=reverse,
                                     want_dstate=True)
    step = lambda x, i: x[:, i:i + 1].contiguous()  # noqa: E731
    hs, cs, kept = [c["h0"]], [c0], []
    for s in range(t):
        i = t - 1 - s if reverse else s
        y1, hn, cn, sv = ops.rnn_fwd(step(c["gx"], i), packed, c["bias"], cid, h0=hs[-1], c0=cs[-1], reverse=reverse, save=True,
                                     want_state=True)
        assert torch.equal(y1[:, 0], y[:, i]), (s, "y")
        for a, full in zip(sv, saved):
            assert (a is None and full is None) or torch.equal(a[:, 0], full[:, i]), (s, "saved")
        hs.append(hn)
        cs.append(cn)
        kept.append(sv)
    assert torch.equal(hs[-1], hT) and (not lstm or torch.equal(cs[-1], cT))
    dh, dc = c["dhT"], dcT
    for s in reversed(range(t)):
        i = t - 1 - s if reverse else s
        g1, gh1, dh, dc = ops.rnn_bwd(step(c["dy"], i), packed, cid, kept[s], None, h0=hs[s], c0=cs[s], dhT=dh, dcT=dc, reverse=reverse,
                                      want_dstate=True)
        assert torch.equal(g1[:, 0], dgx[:, i]) and torch.equal(gh1[:, 0], dgh[:, i]), (s, "dgx / dgh")
    assert torch.equal(dh, dh0) and (not lstm or torch.equal(dc, dc0))


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_two_directions_share_one_buffer(cell, monkeypatch):
    """each direction writes its half of a [B, T, 2 H] buffer and nothing else; operands sit in poisoned, guarded buffers"""
    cid, lstm = CELLS[cell], cell == "LSTM"
    b, t, h = 17, 3, 40
    c = _case(cell, b, t, h, seed=9)
    want = [ops.rnn_fwd(c["gx"], ops.rnn_pack(c["w"], cid), c["bias"], cid, h0=c["h0"], c0=c["c0"] if lstm else None, reverse=r)[0]
            for r in (False, True)]
    G = guarded_ops(monkeypatch)
    gx, w, bias, h0 = (G.poisoned(c[k]) for k in ("gx", "w", "bias", "h0"))
    c0 = G.poisoned(c["c0"]) if lstm else None
    packed = ops.rnn_pack(w, cid)
    for d, reverse in enumerate((False, True)):
        (half,) = G.region((b, t, 2 * h), F32, DEV, lambda whole: [whole[:, :, d * h:(d + 1) * h]])
        ops.rnn_fwd(gx, packed, bias, cid, h0=h0, c0=c0, y=half, reverse=reverse, save=True, want_state=True)
        assert torch.equal(half, want[d]), (cell, d)
    G.check()


def _module(rec):
    model = C.RNN(**rec["kwargs"])
    fill_parameters(model, rec["seed"])
    return model.to(DEV)


def _run(model, rec, x_grad=True):
    for p in model.parameters():
        p.grad = None
    x = rec["x"].to(DEV).requires_grad_(x_grad)
    y = model(x)
    assert y.dtype == F32
    (y * rec["dy"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad


def _check_grads(model, rec, names, tag):
    for k, p in model.named_parameters():
        if k not in names:
            assert p.grad is None, f"{tag}: frozen {k} received a gradient"
            continue
        assert p.grad is not None, f"{tag}: {k} has no gradient"
        got = p.grad[::rec["grad_rows"][k]] if k in rec["grad_rows"] else p.grad
        if not rec["grads"][k].any():  # (dW_hh of the last layer's reverse direction: its one useful step starts from the zero state)
            assert not got.any(), f"{tag}: {k} is exactly zero in the reference"
            continue
        err = rel_l2(got, rec["grads"][k])
        print(f"{tag} {k}: rel-L2 {err:.3e} (reference under bf16 autocast {rec['grad_dist'][k]:.3e})")
        assert err <= 1.1 * rec["grad_dist"][k], f"{tag} {k}: rel-L2 {err:.3e} > 1.1 x {rec['grad_dist'][k]:.3e}"


@pytest.mark.parametrize("index", range(4))
def test_module_logits_vs_reference(fx, index):
    """logits within 1.1 x the reference's own bf16-autocast distance from its fp32 run (the fixture's record).

    The first layer reads the f32 features as two bf16 words (rnn.InputProjFn).  With one word the LSTM configuration missed this
    bound on an MI355X (2.58e-3 against 1.1 x 1.99e-3); a float64 replay of the module with the bf16 roundings switched on one group at
    a time gave 1.70e-3 for the head alone, 1.58e-3 for the rounding of x in the input projection alone and 0.27e-3 for the operands
    of the recurrent product alone, and 1.36e-3 with x kept whole."""
    rec = fx["configs"][index]
    model = _module(rec)
    with torch.no_grad():
        y = model(rec["x"].to(DEV))
    err = rel_l2(y, rec["y"])
    print(f"{rec['name']} logits: rel-L2 {err:.3e} (reference under bf16 autocast {rec['y_dist']:.3e})")
    assert err <= 1.1 * rec["y_dist"], f"{rec['name']} logits: rel-L2 {err:.3e} > 1.1 x {rec['y_dist']:.3e}"


@pytest.mark.parametrize("index", range(4))
def test_module_gradients_vs_reference(fx, index):
    """every parameter gradient and dx within 1.1 x the reference's own bf16-autocast distance from its fp32 gradients"""
    rec = fx["configs"][index]
    model = _module(rec)
    y, dx = _run(model, rec)
    _check_grads(model, rec, set(rec["grads"]), rec["name"])
    err = rel_l2(dx, rec["dx"])
    print(f"{rec['name']} dx: rel-L2 {err:.3e} (reference under bf16 autocast {rec['dx_dist']:.3e})")
    assert err <= 1.1 * rec["dx_dist"], f"{rec['name']} dx: rel-L2 {err:.3e} > 1.1 x {rec['dx_dist']:.3e}"


@pytest.mark.parametrize("index", range(4))
def test_module_gradients_under_partial_freezing(fx, index, monkeypatch):
    rec = fx["configs"][index]
    model = _module(rec)
    target = "rnn_list.0.weight_hh_l0"
    calls = {"colsum": 0, "tn": 0}
    colsum, gemm = ops.colsum, ops.gemm
    monkeypatch.setattr(ops, "colsum", lambda *a, **k: (calls.__setitem__("colsum", calls["colsum"] + 1), colsum(*a, **k))[1])
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: (calls.__setitem__("tn", calls["tn"] + bool(k.get("a_trans"))), gemm(*a, **k))[1])
    # frozen: every other gradient is what it was, weight_hh_l0 gets none
    dict(model.named_parameters())[target].requires_grad_(False)
    _, dx = _run(model, rec)
    _check_grads(model, rec, set(rec["grads"]) - {target}, f"{rec['name']} (weight_hh_l0 frozen)")
    assert rel_l2(dx, rec["dx"]) <= 1.1 * rec["dx_dist"]
    # only it trainable: one tn GEMM, no column sum, no other gradient
    for k, p in model.named_parameters():
        p.requires_grad_(k == target)
    calls.update(colsum=0, tn=0)
    _, dx = _run(model, rec, x_grad=False)
    assert dx is None
    _check_grads(model, rec, {target}, f"{rec['name']} (only weight_hh_l0)")
    assert calls == {"colsum": 0, "tn": 1}, calls


def test_training_reduces_the_loss_and_is_reproducible(fx):
    from cflearn_amd.engine import TrainStep

    rec = fx["configs"][3]
    labels = torch.tensor([0, 2, 1], device=DEV)
    runs = []
    for _ in range(2):
        model = _module(rec).train()
        ts = TrainStep(model, lr=2e-3, loss="focal")
        x = rec["x"].to(DEV)
        losses = [ts.step(x, labels).item() for _ in range(8)]
        torch.cuda.synchronize()
        with torch.no_grad():
            logits = model(x).clone()
        runs.append((losses, [p.detach().clone() for p in model.parameters()] + [logits]))
    losses = runs[0][0]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    # what the runs computed — every parameter after the last step and the logits they give — is the same bit for bit.  The REPORTED
    # loss is the focal kernel's sum over the batch rows, one f32 atomic add per row in whatever order the waves arrive (it feeds
    # nothing back: the logit gradients are per row), so the two runs' figures may differ by the reordering of three addends
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert all(abs(a - b) <= 2 * 2.0 ** -23 * abs(a) for a, b in zip(runs[0][0], runs[1][0])), (runs[0][0], runs[1][0])


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_inference_saves_nothing(fx, cell, monkeypatch):
    rec = fx["configs"][0 if cell == "GRU" else 1]
    model = _module(rec)
    x = rec["x"].to(DEV)
    y_train = model(x)
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = model(x)
    assert y_eval.grad_fn is None and torch.equal(y_eval, y_train.detach())
    # the module level: a no_grad forward keeps no recurrent state alive
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y_eval = model(x)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert grown <= y_eval.numel() * 4 + 512, grown
    # the kernel level: without `save` the forward allocates its output and nothing else (and nothing when the caller owns y)
    cid = CELLS[cell]
    c = _case(cell, 17, 3, 40)
    packed = ops.rnn_pack(c["w"], cid)
    G = guarded_ops(monkeypatch)
    y, hT, cT, saved = ops.rnn_fwd(c["gx"], packed, c["bias"], cid)
    assert saved is None and hT is None and cT is None and len(G.allocs) == 1 and tuple(G.allocs[0].view.shape) == (17, 3, 40)
    ops.rnn_fwd(c["gx"], packed, c["bias"], cid, y=y)
    assert len(G.allocs) == 1
    ops.rnn_fwd(c["gx"], packed, c["bias"], cid, save=True)
    assert len(G.allocs) == (5 if cell == "LSTM" else 4)
    G.check()
