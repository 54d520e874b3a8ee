"""The kernels of csrc/rwkv.hip and the RWKV mixers on the GPU.

Per-element cases compare the scan (y, the saved a and b, dk, dv, dr, d info_decay) and the time mix (the mixed rows, dx, d time_mix)
with the float64 replica of tests/rwkv_replay.py.  Every bound is the replica's: the count of f32 roundings on the path
x 2^-24 x the same recurrence on absolute values, plus half an ulp of the output dtype.  NO element is left out of a bound: the cap on
excluded cases is zero (`_inside` counts them).  Inputs keep |k| <= 4 and |r| <= 4, where the replica is finite everywhere.

Time mix: B in {1, 3}, T in {1, 2, 24, 63, 64, 65, 197}, C in {8, 72, 264}, and B = 3, T = 1025 at C = 8 and 264, where a thread
of the backward walks several rows and a chunk holds a sample boundary.  Scan shapes: B in {1, 3}, L in {8, 72, 200} (a partial wave, two waves with a partial one, four), T in {1, 2, 7, 8, 9, 63, 64, 65, 127, 128,
129, 197}: around the chunk length (8 steps) and the pass length of a 16-wave workgroup (128 steps), and more than one pass.

Causality, sample independence, determinism and the independence from the launch's chunking are exact comparisons.  The modules are
checked against the fixture recorded from the reference: within 1.1 x the reference's own bf16-autocast distance, per tensor."""
import itertools

import pytest
import torch

from helpers import guarded_ops, rel_l2
import rwkv_replay as R
from rwkv_weights import fill_parameters

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops, optim  # noqa: E402
from cflearn_amd import rwkv as RW  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.25
MAX_EXCLUDED = 0  # elements allowed outside their bound
SCAN_T = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 197)
SCAN_CASES = list(itertools.product((1, 3), SCAN_T, (8, 72, 200)))
CLASSES = {"token": C.RWKVTokenMixer, "channel": C.RWKVChannelMixer, "encoder": C.MixedStackedEncoder}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rwkv_small.pt")


def _inside(got, want, bound, what):
    g = got.detach().double().cpu().reshape(-1)
    w, b = want.reshape(-1), bound.reshape(-1)
    assert g.numel() == w.numel() == b.numel(), what
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()), f"{what}: the replica is not finite"
    err = (g - w).abs()
    bad = ~(err <= b)  # (a NaN is bad)
    worst = float((err / b.clamp_min(1e-300)).max()) if g.numel() else 0.0
    print(f"{what}: max |err| / bound {worst:.3f} over {g.numel()} elements")
    assert int(bad.sum()) <= MAX_EXCLUDED, f"{what}: {int(bad.sum())} of {g.numel()} elements outside their bound (worst ratio {worst:.3f})"


def scan_case(b, t, l, seed=0):
    gen = torch.Generator().manual_seed(1000 * t + 10 * l + b + seed)
    k = (torch.randn((b, t, l), generator=gen) * 1.5).clamp(-4.0, 4.0)
    v = torch.randn((b, t, l), generator=gen)
    r = (torch.randn((b, t, l), generator=gen) * 2.0).clamp(-4.0, 4.0)
    # decays exp(w) from 0.01 to 3.5: lam from 0.99 to 0.03, the range of the reference's closed form
    w = torch.linspace(-4.6, 1.25, l)[torch.randperm(l, generator=gen)].contiguous()
    dy = torch.randn((b, t, l), generator=gen)  # f32 as inside the token mixer for B = 1, bf16 for B = 3
    return k, v, r, w, dy if b == 1 else dy.to(BF16)


def _scan_run(case, G=None, waves=0, d_decay="write"):
    put = (lambda x: G.poisoned(x.to(DEV))) if G is not None else (lambda x: x.to(DEV))
    k, v, r, w, dy = (put(x) for x in case)
    y, sa, sb = ops.rwkv_wkv(k, v, r, w, save=True, waves=waves)
    dd = None if d_decay is None else torch.full((w.numel(),), SENTINEL, dtype=F32, device=DEV)
    dk, dv, dr = ops.rwkv_wkv_grad(dy, k, v, r, w, sa, sb, d_decay=dd, accumulate=False, waves=waves)
    torch.cuda.synchronize()
    return dict(y=y, a=sa, b=sb, dk=dk, dv=dv, dr=dr, d_decay=dd)


@pytest.mark.parametrize("b,t,l", SCAN_CASES)
def test_scan_per_element(b, t, l, monkeypatch):
    case = scan_case(b, t, l)
    fw = R.wkv_forward(*case[:4])
    bw = R.wkv_backward(case[4], fw)
    G = guarded_ops(monkeypatch)
    out = _scan_run(case, G)
    G.check()
    tag = f"B{b} T{t} L{l}"
    for name in ("y", "a", "b"):
        _inside(out[name], fw[name], fw[name + "_bound"], f"{tag} {name}")
    for name in ("dk", "dv", "dr", "d_decay"):
        _inside(out[name], bw[name], bw[name + "_bound"], f"{tag} {name}")
    assert out["y"].dtype == BF16 and out["dk"].dtype == BF16 and out["a"].dtype == F32
    # the bits do not depend on how many chunks a workgroup takes per pass
    for waves in (1, 3, 16):
        other = _scan_run(case, waves=waves)
        for name, val in out.items():
            assert torch.equal(val, other[name]), f"{tag} {name}: waves = {waves} changed the bits"


def test_scan_no_grad_output_only_and_destinations(monkeypatch):
    """without `save` the forward allocates y alone; d info_decay written, accumulated into, or frozen.  What is checked for a frozen
    one: the wrapper allocates no workspace for partials and hands the C entry a null destination (which then skips partials and
    reduce: csrc/rwkv.hip, `if (d_decay)`), and dk, dv, dr keep their bits.  The launch count itself is not observed."""
    case = scan_case(3, 65, 72)
    G = guarded_ops(monkeypatch)
    k, v, r, w, dy = (G.poisoned(x.to(DEV)) for x in case)
    n0 = len(G.allocs)
    y = ops.rwkv_wkv(k, v, r, w)
    assert len(G.allocs) == n0 + 1 and isinstance(y, torch.Tensor)
    y2, sa, sb = ops.rwkv_wkv(k, v, r, w, save=True)
    assert len(G.allocs) == n0 + 4 and torch.equal(y, y2)
    wrote = torch.full((72,), SENTINEL, dtype=F32, device=DEV)
    n1 = len(G.allocs)
    grads = ops.rwkv_wkv_grad(dy, k, v, r, w, sa, sb, d_decay=wrote)
    assert len(G.allocs) == n1 + 4  # the workspace of the partials, dk, dv, dr
    prior = torch.randn(72, device=DEV)
    added = prior.clone()
    again = ops.rwkv_wkv_grad(dy, k, v, r, w, sa, sb, d_decay=added, accumulate=True)
    n2 = len(G.allocs)
    frozen = ops.rwkv_wkv_grad(dy, k, v, r, w, sa, sb)
    assert len(G.allocs) == n2 + 3  # dk, dv, dr: no workspace
    G.check()
    assert not bool((wrote == SENTINEL).any()) and torch.equal(added, prior + wrote)
    for a, b, c in zip(grads, again, frozen):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_scan_causality_and_sample_independence():
    b, t, l, t0 = 3, 197, 72, 131
    case = scan_case(b, t, l)
    k, v, r, w, dy = (x.to(DEV) for x in case)
    y = ops.rwkv_wkv(k, v, r, w)
    gen = torch.Generator().manual_seed(5)
    k2, v2, r2 = (x.clone() for x in (k, v, r))
    for x in (k2, v2, r2):
        x[:, t0:] = torch.randn((b, t - t0, l), generator=gen).to(DEV)
    y2 = ops.rwkv_wkv(k2, v2, r2, w)
    assert torch.equal(y[:, :t0], y2[:, :t0]) and not torch.equal(y[:, t0:], y2[:, t0:])
    # a batch of 3 = its three samples alone, forward and backward (d info_decay sums over the batch: not compared)
    full = _scan_run(case)
    for i in range(b):
        one = _scan_run(tuple(x[i:i + 1].contiguous() if x.dim() == 3 else x for x in case))
        for name in ("y", "a", "b", "dk", "dv", "dr"):
            assert torch.equal(full[name][i:i + 1], one[name]), (name, i)


# ---- time mix ------------------------------------------------------------------------------------------------------------------


def mix_case(b, t, c, three, dtype):
    """x and the incoming gradients in `dtype`"""
    gen = torch.Generator().manual_seed(100 * t + c + b + int(three))
    x = torch.randn((b, t, c), generator=gen).to(dtype)
    mixes = [torch.rand(c, generator=gen) * 1.3 for _ in range(3 if three else 2)]
    ds = [torch.randn((b, t, c), generator=gen).to(dtype) for _ in mixes]
    return x, mixes, ds


def _mix_args(mixes):
    return (mixes[0], mixes[1] if len(mixes) == 3 else None, mixes[-1])


def _mix_names(mixes):
    return ("dmk", "dmv", "dmr") if len(mixes) == 3 else ("dmk", "dmr")


# the backward walks `per_chunk` rows per thread (one while B T <= 2048 / ceil(C / 256)): the long cases put several rows, a
# sample boundary inside a chunk and fewer chunks than rows in front of the reduce; per_chunk (2 at C = 8, 4 at C = 264) does
# not divide T = 1025, so the chunks straddle the samples at different offsets
MIX_LONG = [(3, 1025, 8), (3, 1025, 264)]
MIX_CASES = list(itertools.product((1, 3), (1, 2, 24, 63, 64, 65, 197), (8, 72, 264))) + MIX_LONG


def _rows_per_chunk(b, t, c):
    chunks = C._lib.load().cfhip_rwkv_time_mix_bwd_workspace(b, t, c) // (3 * c * 4)
    return -(-(b * t) // chunks), chunks


def _assert_rows_share_a_chunk(b, t, c):
    per, chunks = _rows_per_chunk(b, t, c)
    assert per > 1 and t % per != 0 and chunks < b * t, (per, chunks)


def _mix_run(x, mixes, ds, G=None, dests="write"):
    put = (lambda q: G.poisoned(q.to(DEV))) if G is not None else (lambda q: q.to(DEV))
    xd, md, dd = put(x), [put(m) for m in mixes], [put(d) for d in ds]
    outs = ops.rwkv_time_mix(xd, *_mix_args(md))
    names = _mix_names(mixes)
    dst = {n: torch.full((x.shape[-1],), SENTINEL, dtype=F32, device=DEV) for n in names}
    dargs = (dd[0], dd[1] if len(dd) == 3 else None, dd[-1])
    dx = ops.rwkv_time_mix_grad(*dargs, xd, *_mix_args(md), dests=dst)
    torch.cuda.synchronize()
    return outs, dx, [dst[n] for n in names]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("three", [True, False], ids=["kvr", "kr"])
@pytest.mark.parametrize("b,t,c", MIX_CASES)
def test_time_mix_per_element(b, t, c, three, dtype, monkeypatch):
    if (b, t, c) in MIX_LONG:
        _assert_rows_share_a_chunk(b, t, c)
    x, mixes, ds = mix_case(b, t, c, three, dtype)
    want, bounds = R.time_mix(x, mixes)
    back = R.time_mix_backward(ds, x, mixes, out_bf16=dtype == BF16)
    G = guarded_ops(monkeypatch)
    outs, dx, dms = _mix_run(x, mixes, ds, G)
    G.check()
    tag = f"B{b} T{t} C{c}"
    assert len(outs) == len(mixes) and dx.dtype == dtype
    for j, out in enumerate(outs):
        assert out.dtype == BF16
        _inside(out, want[j], bounds[j], f"{tag} in_{j}")
    _inside(dx, back["dx"], back["dx_bound"], f"{tag} dx")
    for j, dm in enumerate(dms):
        _inside(dm, back["dm"][j], back["dm_bound"][j], f"{tag} dm_{j}")


@pytest.mark.parametrize("b,t,c", [(3, 65, 72)] + MIX_LONG)
def test_time_mix_destinations_and_sample_independence(b, t, c, monkeypatch):
    """write / accumulate / null destinations of the mix gradients (a null one is neither computed nor given a workspace), and a
    batch of 3 against its samples alone, bit for bit; also where several rows and a sample boundary share a chunk"""
    if (b, t, c) in MIX_LONG:
        _assert_rows_share_a_chunk(b, t, c)
    x, mixes, ds = mix_case(b, t, c, True, F32)
    G = guarded_ops(monkeypatch)
    xd, md, dd = G.poisoned(x.to(DEV)), [G.poisoned(m.to(DEV)) for m in mixes], [G.poisoned(d.to(DEV)) for d in ds]
    wrote = {n: torch.full((c,), SENTINEL, dtype=F32, device=DEV) for n in ("dmk", "dmv", "dmr")}
    dx = ops.rwkv_time_mix_grad(*dd, xd, *md, dests=wrote)
    prior = {n: torch.randn(c, device=DEV) for n in wrote}
    # dmk added to, dmv frozen, dmr written
    mixed = {"dmk": prior["dmk"].clone(), "dmv": None, "dmr": torch.full((c,), SENTINEL, dtype=F32, device=DEV)}
    dx2 = ops.rwkv_time_mix_grad(*dd, xd, *md, dests=mixed, accumulate=("dmk",))
    n0 = len(G.allocs)
    dx3 = ops.rwkv_time_mix_grad(*dd, xd, *md, dests={})  # everything frozen: dx is the only allocation, no workspace for partials
    assert len(G.allocs) == n0 + 1
    assert ops.rwkv_time_mix_grad(*dd, xd, *md, dests={}, want_dx=False) is None and len(G.allocs) == n0 + 1
    only = {"dmv": torch.full((c,), SENTINEL, dtype=F32, device=DEV)}
    assert ops.rwkv_time_mix_grad(*dd, xd, *md, dests=only, want_dx=False) is None
    G.check()
    assert torch.equal(dx, dx2) and torch.equal(dx, dx3)
    assert torch.equal(mixed["dmk"], prior["dmk"] + wrote["dmk"]) and torch.equal(mixed["dmr"], wrote["dmr"])
    assert torch.equal(only["dmv"], wrote["dmv"]) and not any(bool((v == SENTINEL).any()) for v in wrote.values())
    # a batch of 3 = its three samples alone: the shift never crosses a sample boundary, forward or backward
    outs = ops.rwkv_time_mix(xd, *md)
    for i in range(3):
        one = ops.rwkv_time_mix(xd[i:i + 1].contiguous(), *md)
        assert all(torch.equal(a[i:i + 1], o) for a, o in zip(outs, one)), i
        dxi = ops.rwkv_time_mix_grad(*(d[i:i + 1].contiguous() for d in dd), xd[i:i + 1].contiguous(), *md, dests={})
        assert torch.equal(dx[i:i + 1], dxi), i


# ---- the channel mixer's elementwise kernels ---------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 255, 257, 3 * 65 * 72])
def test_relu2_and_gate_per_element(n, monkeypatch):
    gen = torch.Generator().manual_seed(n)
    G = guarded_ops(monkeypatch)
    U, HB = R.U, R.HALF_BF16
    d = torch.randn(n, generator=gen).to(BF16)
    for dtype in (F32, BF16):
        h = (torch.randn(n, generator=gen) * 2.0).to(dtype)
        hd = G.poisoned(h.to(DEV))
        h64 = torch.relu(h.double())
        _inside(ops.rwkv_relu2(hd), h64 ** 2, (U + HB) * h64 ** 2 * (1.0 + U), f"relu2 {dtype}")
        d = torch.randn(n, generator=gen).to(dtype)
        want = 2.0 * h64 * d.double()
        _inside(ops.rwkv_relu2_grad(G.poisoned(d.to(DEV)), hd), want, (U + HB) * want.abs() * (1.0 + U), f"relu2 grad {dtype}")
    r = (torch.randn(n, generator=gen) * 2.0).clamp(-4.0, 4.0)
    kv = torch.randn(n, generator=gen)
    rd, kd = G.poisoned(r.to(DEV)), G.poisoned(kv.to(DEV))
    sig = torch.sigmoid(r.double())
    val = sig * kv.double()
    out = ops.rwkv_gate(rd, kd)
    assert out.dtype == BF16
    _inside(out, val, val.abs() * (5.0 * U + HB) * (1.0 + 5.0 * U), "gate")
    for dtype in (F32, BF16):
        res = torch.randn(n, generator=gen).to(dtype)
        out = ops.rwkv_gate(rd, kd, G.poisoned(res.to(DEV)))
        assert out.dtype == dtype
        want = val + res.double()
        err = 5.0 * U * val.abs() + U * (val.abs() + res.double().abs())
        _inside(out, want, err + (U if dtype == F32 else HB) * (want.abs() + err), f"gate + residual {dtype}")
        g = torch.randn(n, generator=gen).to(dtype)
        dr, dkv = ops.rwkv_gate_grad(G.poisoned(g.to(DEV)), rd, kd)
        want_r, want_kv = g.double() * kv.double() * sig * (1.0 - sig), g.double() * sig
        _inside(dr, want_r, want_r.abs() * (14.0 * U + HB) * (1.0 + 14.0 * U), f"gate dr {dtype}")
        _inside(dkv, want_kv, want_kv.abs() * (5.0 * U + HB) * (1.0 + 5.0 * U), f"gate dkv {dtype}")
    G.check()


# ---- the modules against the fixture -----------------------------------------------------------------------------------------------


def _module(rec):
    torch.manual_seed(rec["seed"])
    model = CLASSES[rec["kind"]](**rec["kwargs"])
    fill_parameters(model, rec["seed"])
    return model.to(DEV)


def _run(model, rec, x_grad=True, clear=True):
    if clear:
        for p in model.parameters():
            p.grad = None
    x = rec["x"].to(DEV).requires_grad_(x_grad)
    y = model(x)
    (y.float() * rec["dy"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad


def _within(got, want, dist, what):
    err = rel_l2(got, want)
    print(f"{what}: rel-L2 {err:.3e} (reference under bf16 autocast {dist:.3e})")
    assert err <= 1.1 * dist, f"{what}: rel-L2 {err:.3e} > 1.1 x {dist:.3e}"


def _check_grads(model, rec, names, tag):
    """every named gradient is measured and printed before the first assertion fires"""
    late = []
    for k, p in model.named_parameters():
        if k not in names:
            assert p.grad is None or not p.requires_grad, f"{tag}: frozen {k} received a gradient"
            continue
        assert p.grad is not None, f"{tag}: {k} has no gradient"
        got = p.grad[::rec["grad_rows"][k]] if k in rec["grad_rows"] else p.grad
        try:
            _within(got, rec["grads"][k], rec["grad_dist"][k], f"{tag} {k}")
        except AssertionError as e:
            late.append(str(e))
    assert not late, f"{len(late)} of {len(names)} gradients outside 1.1 x their yardstick:\n" + "\n".join(late)


@pytest.mark.parametrize("index", range(5))
def test_module_vs_reference(fx, index):
    """output, dx and every parameter gradient within 1.1 x the reference's own bf16-autocast distance from its fp32 run.

    The tightest tensors are the encoder's LayerNorm biases (64 numbers, each a sum over the 96 rows).  With the Linear layers as
    separate autograd nodes around the bf16 rows `mixing_blocks.0.channel_norm.bias` measures up to 1.125 x its yardstick (6.73e-03
    against 5.98e-03); with every projection inside the Function next to it (f32 gradients between GEMM and kernel, `rwkv.py`) it is
    inside 1.1 x."""
    rec = fx["configs"][index]
    model = _module(rec)
    with torch.no_grad():
        y0 = model(rec["x"].to(DEV))
    _within(y0, rec["y"], rec["y_dist"], f"{rec['name']} output")
    y, dx = _run(model, rec)
    assert torch.equal(y, y0)
    _check_grads(model, rec, set(rec["grads"]), rec["name"])
    _within(dx, rec["dx"], rec["dx_dist"], f"{rec['name']} dx")


@pytest.mark.parametrize("index", range(5))
def test_module_under_partial_freezing(fx, index, monkeypatch):
    """info_decay and the time mixes frozen: the Linear weights get what they got, the scan's backward takes no destination and the
    time mix's none either; then only those trainable and no dx wanted"""
    rec = fx["configs"][index]
    model = _module(rec)
    small = {k for k in rec["grads"] if k.endswith("info_decay") or "time_mix_" in k}
    calls = []
    scan_grad, mix_grad = ops.rwkv_wkv_grad, ops.rwkv_time_mix_grad
    monkeypatch.setattr(ops, "rwkv_wkv_grad", lambda *a, **k: (calls.append(("wkv", k.get("d_decay") is not None)), scan_grad(*a, **k))[1])
    monkeypatch.setattr(ops, "rwkv_time_mix_grad",
                        lambda *a, **k: (calls.append(("mix", sorted(n for n, d in k["dests"].items() if d is not None))), mix_grad(*a, **k))[1])
    for k, p in model.named_parameters():
        p.requires_grad_(k not in small)
    _, dx = _run(model, rec)
    _check_grads(model, rec, set(rec["grads"]) - small, f"{rec['name']} (decay and mixes frozen)")
    _within(dx, rec["dx"], rec["dx_dist"], f"{rec['name']} dx (decay and mixes frozen)")
    assert calls and all(c in (("wkv", False), ("mix", [])) for c in calls), calls
    for k, p in model.named_parameters():
        p.requires_grad_(k in small)
    calls.clear()
    _, dx = _run(model, rec, x_grad=rec["kind"] == "encoder")
    _check_grads(model, rec, small, f"{rec['name']} (only decay and mixes)")
    assert all(c[1] for c in calls), calls


@pytest.mark.parametrize("index", [0, 2, 4])
def test_module_through_the_arena(fx, index):
    """direct `.grad` writes into an optim.ParamArena after a lazy zero-grad: every gradient is overwritten (the sentinel is gone),
    stays in the arena, and a second backward without zeroing doubles it"""
    rec = fx["configs"][index]
    model = _module(rec)
    arena = optim.ParamArena(list(model.parameters()))
    arena.flat_g.fill_(SENTINEL)
    arena.zero_grad(lazy=True)
    _, dx = _run(model, rec, clear=False)
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == arena.grad_view(p).data_ptr(), k
    _check_grads(model, rec, set(rec["grads"]), f"{rec['name']} (arena)")
    _within(dx, rec["dx"], rec["dx_dist"], f"{rec['name']} dx (arena)")
    once = {k: p.grad.clone() for k, p in model.named_parameters()}
    _run(model, rec, clear=False)
    for k, p in model.named_parameters():
        assert torch.allclose(p.grad, 2 * once[k], rtol=1e-5, atol=1e-9), k


@pytest.mark.parametrize("index", range(5))
def test_reference_keyed_state_dict_loads_strictly(fx, index):
    rec = fx["configs"][index]
    source = _module(rec)
    state = {k: v.detach().cpu().clone() for k, v in source.state_dict().items()}
    assert [k for k, _, _ in rec["state"]] == list(state)
    torch.manual_seed(1)
    model = CLASSES[rec["kind"]](**rec["kwargs"])
    model.load_state_dict(state, strict=True)
    model = model.to(DEV)
    with torch.no_grad():
        y = model(rec["x"].to(DEV))
    _within(y, rec["y"], rec["y_dist"], f"{rec['name']} output after load_state_dict")


@pytest.mark.parametrize("index", range(4))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_residual_is_added_on_the_way_out(fx, index, dtype):
    """mixer(x, residual=res) = res + mixer(x) to the rounding of the one add: the call without a residual leaves in bf16 (half an ulp
    of its value), the sum is rounded once to the residual's dtype"""
    rec = fx["configs"][index]
    model = _module(rec)
    x = rec["x"].to(DEV)
    res = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    with torch.no_grad():
        plain = model(x)
        summed = model(x, residual=res)
    assert plain.dtype == BF16 and summed.dtype == dtype
    want = res.double().cpu() + plain.double().cpu()
    bound = R.HALF_BF16 * 1.01 * plain.double().cpu().abs() + (R.U if dtype == F32 else R.HALF_BF16) * want.abs() * 1.01 + 1e-30
    _inside(summed, want, bound, f"{rec['name']} + residual {dtype}")
    # and the gradient reaches the residual unchanged
    resg = res.clone().requires_grad_(True)
    model(x, residual=resg).float().sum().backward()
    assert torch.equal(resg.grad, torch.ones_like(resg))


def test_mixers_are_causal_and_samples_independent(fx):
    """changing x at t >= t0 leaves every output at t < t0 bit-identical (token mixer, channel mixer, the encoder); changing one
    sample leaves the others bit-identical, forward and dx"""
    t0 = 13
    for index in (0, 2, 4):
        rec = fx["configs"][index]
        model = _module(rec)
        x = rec["x"].to(DEV)
        gen = torch.Generator().manual_seed(index)
        x2 = x.clone()
        x2[:, t0:] = torch.randn(x2[:, t0:].shape, generator=gen).to(DEV)
        with torch.no_grad():
            y, y2 = model(x), model(x2)
        assert torch.equal(y[:, :t0], y2[:, :t0]) and not torch.equal(y[:, t0:], y2[:, t0:]), rec["name"]
        x3 = x.clone()
        x3[1] = torch.randn(x3[1].shape, generator=gen).to(DEV)
        outs = []
        for inp in (x, x3):
            xg = inp.clone().requires_grad_(True)
            out = model(xg)
            (out.float() * rec["dy"].to(DEV)).sum().backward()
            outs.append((out.detach(), xg.grad))
        for i in (0, 2, 3):
            assert torch.equal(outs[0][0][i], outs[1][0][i]) and torch.equal(outs[0][1][i], outs[1][1][i]), (rec["name"], i)
        assert not torch.equal(outs[0][0][1], outs[1][0][1])


def test_two_runs_are_bit_identical(fx):
    for index in (0, 2, 4):
        rec = fx["configs"][index]
        model = _module(rec)
        runs = []
        for _ in range(2):
            y, dx = _run(model, rec)
            runs.append((y, dx, {k: p.grad.clone() for k, p in model.named_parameters()}))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        for k in runs[0][2]:
            assert torch.equal(runs[0][2][k], runs[1][2][k]), (rec["name"], k)


def test_no_grad_forward_saves_no_scan_state():
    b, t, l = 8, 256, 256
    k, v, r, w, _ = (x.to(DEV) for x in scan_case(b, t, l))
    state = b * t * l * 4  # one f32 scan state
    peaks = []
    for grad in (False, True):
        kk = k.clone().requires_grad_(grad)
        for _ in range(2):  # the first pass loads code objects and sizes the allocator's pools
            with torch.set_grad_enabled(grad):
                y = RW.wkv(kk, v, r, w)
            del y
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rest = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(grad):
            y = RW.wkv(kk, v, r, w)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - rest)
        del y
    print(f"peak above rest: {peaks[0]} bytes without grad, {peaks[1]} with; one f32 state is {state}")
    assert peaks[0] < state, peaks  # y alone (bf16: half a state)
    assert peaks[1] >= 2 * state, peaks  # a and b


def test_training_is_reproducible(fx):
    """three optimizer steps on the encoder, twice: the same bits"""
    rec = fx["configs"][4]
    x, dy = rec["x"].to(DEV), rec["dy"].to(DEV)
    runs = []
    for _ in range(2):
        model = _module(rec)
        opt = C.FusedAdamOptimizer(model.parameters(), lr=2e-3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = (model(x).float() * dy).sum()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        runs.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert not torch.equal(runs[0][0][0], runs[0][0][2])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
