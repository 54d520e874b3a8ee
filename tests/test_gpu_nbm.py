"""The basis and featurizer kernels of csrc/nbm.hip and the nbm module on the GPU.

Per-element cases (nbm_weights.KERNEL_CASES: a pruned cross of H in {8, 40, 256}, NB in {1, 3, 64}, M in {1, 17, 65, 300}, order in
{1, 2, 4} and an index table with a feature in several tuples and twice in one) compare `bases` and every backward output with the
float64 replica of tests/nbm_replay.py, fed the operands the kernel multiplies.  The bounds are the replica's, written out of the
operation order in the header of csrc/nbm.hip; for the gradients they include the magnitude of every hidden unit whose float64
pre-activation lies within the forward bound of zero, so a ReLU mask that flips is inside the bound and no element is left out
(tests/test_nbm_host.py checks, from the replica alone, that fewer than 1 % of the units are in that band).  Everything runs under
guard bytes; write / accumulate, null destinations, determinism and row chunking are exact comparisons.  The module is checked against
the fixture recorded from the reference: within 1.1 x the reference's own bf16-autocast distance from its fp32 run."""
import pytest
import torch

from helpers import assert_elementwise, guarded_ops, rel_l2
import nbm_replay as R
from nbm_weights import KERNEL_CASES, fill_parameters, kernel_case

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops, optim  # noqa: E402

DEV = "cuda"
F32 = torch.float32
GRADS = ops.NBM_GRADS
SENTINEL = -7.25


@pytest.fixture(scope="module")
def fx(golden):
    return golden("nbm_small.pt")


def _device_case(case, G=None):
    put = (lambda t: G.poisoned(t.to(DEV))) if G is not None else (lambda t: t.to(DEV))
    c = {k: put(v) for k, v in case.items() if k != "idx"}
    idx = ops.nbm_index(case["idx"], len(case["idx"][0]), case["x"].shape[1], DEV)
    if G is not None:
        idx = ops.NbmIndex(G.index(idx.table), idx.features)
    c["idx"] = idx
    return c


def _dests(c, fill=None, only=GRADS):
    shapes = {"dw1": c["w1"].shape, "db1": c["b1"].shape, "dw2": c["w2"].shape, "db2": c["b2"].shape, "dw3": c["w3"].shape, "db3": c["b3"].shape}
    return {k: (torch.empty(shapes[k], dtype=F32, device=DEV) if fill is None else torch.full(shapes[k], fill, dtype=F32, device=DEV))
            for k in only}


def _grad(c, dests, accumulate=(), want_dx=True, packed=None):
    packed = ops.nbm_pack(c["w2"]) if packed is None else packed
    return ops.nbm_bases_grad(c["dbases"], c["x"], c["idx"], c["w1"], c["b1"], packed, c["b2"], c["w3"], dests=dests, accumulate=accumulate,
                              want_dx=want_dx)


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_bases_per_element(name, monkeypatch):
    h, nb, b, f, idx, seed = KERNEL_CASES[name]
    case = kernel_case(h, nb, b, f, idx, seed)
    rp = R.Replay(case)
    G = guarded_ops(monkeypatch)
    c = _device_case(case, G)
    packed = ops.nbm_pack(c["w2"])
    bases = ops.nbm_bases(c["x"], c["idx"], c["w1"], c["b1"], packed, c["b2"], c["w3"], c["b3"])
    assert tuple(bases.shape) == (b, len(idx), nb)
    assert_elementwise(bases.view(-1, nb), rp.bases, out_dtype=F32, ulps=1, cond=rp.bases_bound(), k=1, what=f"{name} bases")
    # ---- the backward: every destination written (NaN-filled before), dx returned ----
    want, bound = rp.backward(case["dbases"])
    dests = {k: G.empty(v.shape, dtype=F32, device=DEV) for k, v in _dests(c).items()}
    dx = _grad(c, dests, packed=packed)
    for k in GRADS:
        print(f"{name} {k}: max |err| {float((dests[k].cpu().double().reshape(-1) - want[k].reshape(-1)).abs().max()):.3e}")
        assert_elementwise(dests[k].reshape(-1), want[k].reshape(-1), out_dtype=F32, ulps=1, cond=bound[k].reshape(-1), k=1, what=f"{name} {k}")
    assert_elementwise(dx, want["dx"], out_dtype=F32, ulps=1, cond=bound["dx"], k=1, what=f"{name} dx")
    # a feature no tuple reads gets an exact zero
    unread = [col for col in range(f) if all(col not in pack for pack in idx)]
    assert not dx[:, unread].any()
    # ---- determinism: a second identical call, bit for bit ----
    again = {k: G.empty(v.shape, dtype=F32, device=DEV) for k, v in dests.items()}
    dx2 = _grad(c, again, packed=packed)
    assert torch.equal(dx, dx2) and all(torch.equal(dests[k], again[k]) for k in GRADS)
    assert torch.equal(bases, ops.nbm_bases(c["x"], c["idx"], c["w1"], c["b1"], packed, c["b2"], c["w3"], c["b3"]))
    G.check()


@pytest.mark.parametrize("name", ["h40_nb3_m300_o2_repeat", "h256_nb3_m65_o4", "h8_nb64_m1_o4"])
def test_write_accumulate_and_null_destinations(name, monkeypatch):
    h, nb, b, f, idx, seed = KERNEL_CASES[name]
    c = _device_case(kernel_case(h, nb, b, f, idx, seed))
    plain = _dests(c)
    dx = _grad(c, plain)
    G = guarded_ops(monkeypatch)
    # accumulate every second destination into a sentinel-filled buffer, overwrite the others
    acc = GRADS[::2]
    mixed = {k: G.empty(v.shape, dtype=F32, device=DEV) for k, v in plain.items()}
    for k in GRADS:
        mixed[k].fill_(SENTINEL)
    assert torch.equal(_grad(c, mixed, accumulate=acc), dx)
    for k in GRADS:
        assert torch.equal(mixed[k], plain[k] + SENTINEL if k in acc else plain[k]), k
    # null destinations: one destination at a time, nothing else is written (every allocation of the call sits between guards)
    for k in GRADS:
        one = {k: G.empty(plain[k].shape, dtype=F32, device=DEV)}
        assert _grad(c, one, want_dx=False) is None
        assert torch.equal(one[k], plain[k]), k
    # dx alone
    assert torch.equal(_grad(c, {}), dx)
    G.check()


@pytest.mark.parametrize("name", ["h40_nb3_m300_o2_repeat", "h256_nb3_m300_o2_repeat", "h8_nb1_m300_o1"])
def test_row_chunks(name):
    """one call on all rows against two calls on the halves of the batch: `bases` and dx (per row) bit for bit, the parameter
    gradients as the f32 sum of the halves up to the reordering of the row sums"""
    h, nb, b, f, idx, seed = KERNEL_CASES[name]
    case = kernel_case(h, nb, b, f, idx, seed)
    c = _device_case(case)
    packed = ops.nbm_pack(c["w2"])
    run = lambda x: ops.nbm_bases(x, c["idx"], c["w1"], c["b1"], packed, c["b2"], c["w3"], c["b3"])  # noqa: E731
    whole = run(c["x"])
    cut = b // 2 + 1
    assert torch.equal(torch.cat([run(c["x"][:cut]), run(c["x"][cut:])]), whole)
    full = _dests(c)
    dx = _grad(c, full, packed=packed)
    halves, dxs = [], []
    for sl in (slice(0, cut), slice(cut, b)):
        part = dict(c, x=c["x"][sl], dbases=c["dbases"][sl].contiguous())
        d = _dests(c)
        dxs.append(_grad(part, d, packed=packed))
        halves.append(d)
    assert torch.equal(torch.cat(dxs), dx)
    _, bound = R.Replay(case).backward(case["dbases"])
    for k in GRADS:
        both = (halves[0][k] + halves[1][k]).cpu().double().reshape(-1)
        # each side is within its own bound of the exact sum, so the two differ by at most twice the bound (plus the f32 addition)
        assert_elementwise(full[k].reshape(-1), both, out_dtype=F32, ulps=2, cond=bound[k].reshape(-1), k=2, what=f"{name} {k}")


@pytest.mark.parametrize("b,d,nb", [(1, 1, 1), (17, 5, 3), (130, 12, 64), (4100, 2, 5)])
def test_featurizer_per_element(b, d, nb, monkeypatch):
    gen = torch.Generator().manual_seed(100 * b + d)
    G = guarded_ops(monkeypatch)
    bases, wf, bf, dfeat = (G.poisoned(torch.randn(s, generator=gen).to(DEV)) for s in ((b, d, nb), (d, nb), (d,), (b, d)))
    feat = ops.nbm_featurize(bases, wf, bf)
    want, bound = R.featurize(bases, wf, bf)
    assert_elementwise(feat, want, out_dtype=F32, ulps=1, cond=bound, k=1, what="feat")
    gw, gbound = R.featurize_backward(dfeat, bases, wf)
    dwf, dbf = G.empty((d, nb), dtype=F32, device=DEV), G.empty((d,), dtype=F32, device=DEV)
    dbases = ops.nbm_featurize_grad(dfeat, bases, wf, dwf=dwf, dbf=dbf)
    for got, k in ((dbases, "dbases"), (dwf, "dwf"), (dbf, "dbf")):
        assert_elementwise(got, gw[k], out_dtype=F32, ulps=1, cond=gbound[k], k=1, what=k)
    # accumulate / write per destination, null destinations, determinism
    dwf2, dbf2 = torch.full_like(dwf, SENTINEL), torch.full_like(dbf, SENTINEL)
    assert torch.equal(ops.nbm_featurize_grad(dfeat, bases, wf, dwf=dwf2, dbf=dbf2, accumulate=("dbf",)), dbases)
    assert torch.equal(dwf2, dwf) and torch.equal(dbf2, dbf + SENTINEL)
    dwf3 = G.empty((d, nb), dtype=F32, device=DEV)
    assert ops.nbm_featurize_grad(dfeat, bases, wf, dwf=dwf3, want_dbases=False) is None and torch.equal(dwf3, dwf)
    assert torch.equal(ops.nbm_featurize_grad(dfeat, None, wf), dbases)
    G.check()


# ---- the module against the fixture --------------------------------------------------------------------------------------------------


def _module(rec):
    model = C.NBM(**rec["kwargs"])
    fill_parameters(model, rec["seed"])
    return model.to(DEV)


def _run(model, rec, x_grad=True, clear=True):
    if clear:
        for p in model.parameters():
            p.grad = None
    x = rec["x"].to(DEV).requires_grad_(x_grad)
    y = model(x)
    assert y.dtype == F32
    (y * rec["dy"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad


def _within(got, want, dist, what):
    err = rel_l2(got, want)
    print(f"{what}: rel-L2 {err:.3e} (reference under bf16 autocast {dist:.3e})")
    assert err <= 1.1 * dist, f"{what}: rel-L2 {err:.3e} > 1.1 x {dist:.3e}"


def _check_grads(model, rec, names, tag):
    for k, p in model.named_parameters():
        if k not in names:
            assert p.grad is None or not p.requires_grad, f"{tag}: frozen {k} received a gradient"
            continue
        assert p.grad is not None, f"{tag}: {k} has no gradient"
        got = p.grad[::rec["grad_rows"][k]] if k in rec["grad_rows"] else p.grad
        _within(got, rec["grads"][k], rec["grad_dist"][k], f"{tag} {k}")


@pytest.mark.parametrize("index", range(4))
def test_module_vs_reference(fx, index):
    """logits, features, dx and every gradient within 1.1 x the reference's own bf16-autocast distance from its fp32 run"""
    rec = fx["configs"][index]
    model = _module(rec)
    with torch.no_grad():
        y0 = model(rec["x"].to(DEV))
        feat = model(rec["x"].to(DEV), return_features=True)
    _within(y0, rec["y"], rec["y_dist"], f"{rec['name']} logits")
    _within(feat, rec["feat"], rec["feat_dist"], f"{rec['name']} features")
    y, dx = _run(model, rec)
    assert torch.equal(y, y0)
    _check_grads(model, rec, set(rec["grads"]), rec["name"])
    _within(dx, rec["dx"], rec["dx_dist"], f"{rec['name']} dx")


@pytest.mark.parametrize("index", range(4))
def test_module_under_partial_freezing(fx, index, monkeypatch):
    rec = fx["configs"][index]
    model = _module(rec)
    calls = []
    grad = ops.nbm_bases_grad
    monkeypatch.setattr(ops, "nbm_bases_grad", lambda *a, **k: (calls.append((sorted(k["dests"]), k["want_dx"])), grad(*a, **k))[1])
    # the bases frozen: the featurizer and the head get what they got, dx still flows through one launch per order with no destination
    for k, p in model.named_parameters():
        p.requires_grad_(not k.startswith("bases."))
    _, dx = _run(model, rec)
    _check_grads(model, rec, {k for k in rec["grads"] if not k.startswith("bases.")}, f"{rec['name']} (bases frozen)")
    _within(dx, rec["dx"], rec["dx_dist"], f"{rec['name']} dx (bases frozen)")
    assert calls == [([], True)] * len(model.nary), calls
    # only the hidden matrix of the first order trainable: one destination, no dx
    first = next(iter(model.nary))
    target = f"bases.{first}.net.1.conv.weight"
    for k, p in model.named_parameters():
        p.requires_grad_(k == target)
    calls.clear()
    _, dx = _run(model, rec, x_grad=False)
    assert dx is None
    _check_grads(model, rec, {target}, f"{rec['name']} (only {target})")
    assert calls == [(["dw2"], False)], calls


@pytest.mark.parametrize("index", [0, 2])
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


def test_head_fn_per_element(monkeypatch):
    """nbm.HeadFn alone: logits, dX, dW and db against float64; f32 fma chains of latent_dim + 1 (the bias column) / out / B terms"""
    from cflearn_amd.nbm import HeadFn

    b, d, out = 37, 13, 3
    gen = torch.Generator().manual_seed(41)
    feat, w, bias, dy = (torch.randn(s, generator=gen) for s in ((b, d), (out, d), (out,), (b, out)))
    G = guarded_ops(monkeypatch)
    for direct in (True, False):
        f = feat.to(DEV).requires_grad_(True)
        wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(bias.to(DEV))
        y = HeadFn.apply(f, wp if direct else wp * 1, bp if direct else bp * 1)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
        f64, w64, b64, dy64 = feat.double(), w.double(), bias.double(), dy.double()
        assert_elementwise(y, f64 @ w64.t() + b64, out_dtype=F32, ulps=1, cond=f64.abs() @ w64.abs().t() + b64.abs(), k=d + 2, what="head y")
        assert_elementwise(f.grad, dy64 @ w64, out_dtype=F32, ulps=1, cond=dy64.abs() @ w64.abs(), k=out + 1, what="head dX")
        assert_elementwise(wp.grad, dy64.t() @ f64, out_dtype=F32, ulps=1, cond=dy64.abs().t() @ f64.abs(), k=b + 1, what="head dW")
        assert_elementwise(bp.grad, dy64.sum(0), out_dtype=F32, ulps=1, cond=dy64.abs().sum(0), k=b + 8, what="head db")
    G.check()
    # frozen weight and bias: dX only
    f = feat.to(DEV).requires_grad_(True)
    wp, bp = torch.nn.Parameter(w.to(DEV), requires_grad=False), torch.nn.Parameter(bias.to(DEV), requires_grad=False)
    HeadFn.apply(f, wp, bp).backward(dy.to(DEV))
    assert wp.grad is None and bp.grad is None and f.grad is not None


def test_bases_dropout_runs_in_training_only(fx):
    """`bases_dropout` goes through functional.dropout: identity in eval mode, a mask in training mode that the backward applies too"""
    rec = fx["configs"][2]
    model = C.NBM(**dict(rec["kwargs"], bases_dropout=0.5))
    fill_parameters(model, rec["seed"])
    model = model.to(DEV)
    x = rec["x"].to(DEV)
    with torch.no_grad():
        plain = _module(rec)(x)
        assert torch.equal(model.eval()(x), plain)
    model.train()
    xg = x.clone().requires_grad_(True)
    y = model(xg)
    assert y.shape == plain.shape and torch.isfinite(y).all() and not torch.equal(y.detach(), plain)
    y.sum().backward()
    assert torch.isfinite(xg.grad).all() and xg.grad.any()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_inputs_are_flattened_and_cast(fx):
    """more than 2 dimensions are flattened, a non-f32 input is cast to f32 (modules/ml/nbm.py:181-183)"""
    rec = fx["configs"][0]
    model = _module(rec)
    x = rec["x"].to(DEV)
    with torch.no_grad():
        want = model(x)
        assert torch.equal(model(x.view(x.shape[0], 3, 2, 2)), want)
        assert torch.equal(model(x.double()), want)
        x16 = x.to(torch.bfloat16)
        assert torch.equal(model(x16), model(x16.float()))


def test_inspect_vs_reference(fx):
    for rec in fx["inspect"]:
        cfg = fx["configs"][rec["config"]]
        model = _module(cfg).train()
        out = model.inspect(rec["input"].to(DEV), rec["x_dims"], rec["y_dim"], already_extracted=rec["already_extracted"])
        assert model.training and tuple(out.shape) == tuple(rec["out"].shape)
        _within(out, rec["out"], cfg["y_dist"], f"inspect {rec['x_dims']}")


def test_no_grad_allocates_the_bases_and_the_pack(monkeypatch):
    h, nb, b, f, idx, seed = KERNEL_CASES["h40_nb3_m17_o2"]
    c = _device_case(kernel_case(h, nb, b, f, idx, seed))
    G = guarded_ops(monkeypatch)
    packed = ops.nbm_pack(c["w2"])
    ops.nbm_bases(c["x"], c["idx"], c["w1"], c["b1"], packed, c["b2"], c["w3"], c["b3"])
    assert [tuple(a.view.shape) for a in G.allocs] == [(packed.numel(),), (b, len(idx), nb)]
    G.check()


def test_peak_memory_is_below_one_hidden_activation():
    """forward + backward at B = 64, D = 12, NB = 64, H = 32 peaks below the bytes of ONE bf16 [M, NB, H] tensor above the resting
    level (the reference keeps two f32 ones)"""
    b, d, nb, h = 64, 12, 64, 32
    model = C.NBM(d, 3, num_bases=nb, hidden_units=[h, h]).to(DEV)
    x = torch.randn(b, d, device=DEV)
    for _ in range(2):  # the first pass loads code objects and sizes the allocator's pools
        model(x).sum().backward()
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    rest = torch.cuda.memory_allocated()
    model(x).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - rest
    limit = b * d * nb * h * 2
    print(f"peak {peak} bytes above rest, one bf16 [M, NB, H] is {limit}")
    assert peak < limit, (peak, limit)


def test_training_is_reproducible(fx):
    from cflearn_amd.engine import TrainStep

    rec = fx["configs"][2]
    labels = (torch.arange(rec["x"].shape[0]) % rec["kwargs"]["output_dim"]).to(DEV)
    runs = []
    for _ in range(2):
        model = _module(rec).train()
        ts = TrainStep(model, lr=2e-3)
        x = rec["x"].to(DEV)
        losses = [ts.step(x, labels).item() for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in model.parameters()]))
    assert all(l == l for l in runs[0][0]), runs[0][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    start = [p.detach() for p in _module(rec).parameters()]
    assert all(not torch.equal(p, q) for p, q in zip(runs[0][1], start))
