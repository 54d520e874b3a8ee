"""Generate tests/golden/lora_linear.pt: the reference's own `LoRALinearHook` (modules/core/hijacks.py) on the CPU in fp32.

    python tools/gen_lora_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * layers: the reference's `HijackLinear` and `HijackCustomLinear` with a hook attached (dropout 0), (in, out, rank) in
    {(40, 24, 1), (64, 64, 4), (96, 200, 16)}, input [2, 7, in].  Both classes get the same numbers as inputs; their results differ
    (the reference runs the hook of a HijackCustomLinear twice in training mode: see the note in main()).  Recorded per class
    (`results`): the output and the gradients of x, lora_down.weight (`ga`) and lora_up.weight (`gbm`), run with the base unfrozen and
    frozen (the same bits, asserted; stored once); per shape: the gradients of the base weight and bias (unfrozen), and in eval mode
    the injected weight, the output, and that `cleanup()` restored the weight bit for bit (asserted here);
  * ff: the reference's `FeedForward(GELU)` with both layers hooked: output and input gradient.  The low-rank term of the first
    layer enters BEFORE the activation; `wrong_order_rel` is how far an add after the activation lands from it;
  * keys: the state-dict keys and the hook names of a tiny model after `LoRAManager.prepare` + `inject`, and the constructor
    signature / parameter shapes / init statistics of a fresh hook.
Single-threaded and seeded: a second run writes the same bytes.

To keep the file small every tensor the tests feed in lies on a coarse grid and is stored as int8 codes (decode q as
q.float() * <name>_scale; all of them exact in bf16), `lora_up.weight` gets seeded non-zero codes (its zero init would hide the
adapter), alpha is 0.8, and the two [out, in]-sized results (injected weight, base weight gradient) keep every `row_step`-th row."""
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lora_linear.pt")
SHAPES = ((40, 24, 1), (64, 64, 4), (96, 200, 16))
W_SCALE, X_SCALE, A_SCALE, ALPHA = 1.0 / 512, 1.0 / 32, 1.0 / 256, 0.8


def grid(gen, shape, scale, bound=127):
    q = torch.randint(-bound, bound + 1, shape, generator=gen)
    return q.to(torch.int8), q.float() * scale


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def main() -> None:
    torch.set_num_threads(1)
    import_cflearn()
    import importlib

    hj = importlib.import_module("cflearn.modules.core.hijacks")
    cm = importlib.import_module("cflearn.modules.core.mixed_stacks.channel_mixers")
    out: dict = {"layers": [], "scales": dict(w=W_SCALE, x=X_SCALE, a=A_SCALE), "alpha": ALPHA}

    def hooked(cls, nin, nout, rank, w, b, a, bm):
        m = cls(nin, nout)
        inner = m.linear if hasattr(m, "linear") else m
        with torch.no_grad():
            inner.weight.copy_(w)
            inner.bias.copy_(b)
        hook = hj.LoRALinearHook.create_with(m, rank)
        hook.dropout.p = 0.0
        with torch.no_grad():
            hook.lora_down.weight.copy_(a)
            hook.lora_up.weight.copy_(bm)
            hook.alpha.fill_(ALPHA)
        m.hook = hook
        return m, inner, hook

    for si, (nin, nout, rank) in enumerate(SHAPES):
        gen = torch.Generator().manual_seed(400 + si)
        wq, w = grid(gen, (nout, nin), W_SCALE)
        bq, b = grid(gen, (nout,), W_SCALE)
        aq, a = grid(gen, (rank, nin), A_SCALE)
        bmq, bm = grid(gen, (nout, rank), A_SCALE)
        xq, x = grid(gen, (2, 7, nin), X_SCALE, 96)
        gyq, gy = grid(gen, (2, 7, nout), X_SCALE, 96)
        step = max(1, nout // 12)
        rec = dict(shape=(nin, nout, rank), wq=wq, bq=bq, aq=aq, bmq=bmq, xq=xq, gyq=gyq, row_step=step)
        per_cls = []
        for cls in (hj.HijackLinear, hj.HijackCustomLinear):
            r: dict = {}
            for frozen in (False, True):
                m, inner, hook = hooked(cls, nin, nout, rank, w, b, a, bm)
                m.train()
                inner.weight.requires_grad_(not frozen)
                inner.bias.requires_grad_(not frozen)
                xi = x.clone().requires_grad_(True)
                y = m(xi)
                y.backward(gy)
                got = dict(y=y.detach().clone(), gx=xi.grad.clone(), ga=hook.lora_down.weight.grad.clone(),
                           gbm=hook.lora_up.weight.grad.clone())
                if frozen:  # freezing the base changes none of these: stored once
                    assert all(torch.equal(got[k], r[k]) for k in got)
                r.update(got)
                assert hook.alpha.grad is None  # `alpha.item()`: no gradient in the reference either
                if frozen:
                    assert inner.weight.grad is None and inner.bias.grad is None
                else:
                    r["gw_rows"] = inner.weight.grad[::step].clone()
                    r["gb"] = inner.bias.grad.clone()
            m, inner, hook = hooked(cls, nin, nout, rank, w, b, a, bm)
            m.eval()
            with torch.no_grad():
                r["y_eval"] = m(x).clone()
                assert hook.injected
                r["w_injected_rows"] = inner.weight.detach()[::step].clone()
                hook.cleanup()
                assert torch.equal(inner.weight.detach(), w)
            r["restored"] = True
            per_cls.append(r)
        rec["results"] = {"HijackLinear": per_cls[0], "HijackCustomLinear": per_cls[1]}
        # the reference applies the hook of a HijackCustomLinear TWICE in training mode (IBasicHijackMixin.forward, hijacks.py:42-49,
        # wraps customs.Linear.forward, customs.py:81-100, which reads the same `self.hook`): base + 2 s up(down(x)); the eval-mode
        # injection adds s Bm A once.  Recorded as it is; checked here so that a change of the reference shows.
        with torch.no_grad():
            low = (ALPHA / rank) * (x @ a.t() @ bm.t())
            base = x @ w.t() + b
        assert rel(base + low, per_cls[0]["y"]) < 1e-5 and rel(base + 2 * low, per_cls[1]["y"]) < 1e-5
        for k in ("y_eval", "w_injected_rows", "gw_rows", "gb"):  # the same for both classes: stored once
            assert torch.equal(per_cls[0][k], per_cls[1][k])
            rec[k] = per_cls[0][k]
            del per_cls[0][k], per_cls[1][k]
        out["layers"].append(rec)

    # ---- FeedForward(GELU), both layers hooked: pins where the low-rank term of the first layer enters
    nin, lat, rank = 40, 64, 4
    gen = torch.Generator().manual_seed(450)
    ff = cm.FeedForward(nin, lat, 0.0, "GELU")
    ffrec: dict = dict(shape=(nin, lat, rank))
    hooks = {}
    for idx, (i, o) in ((0, (nin, lat)), (3, (lat, nin))):
        layer = ff.net[idx]
        wq, w = grid(gen, (o, i), W_SCALE)
        bq, b = grid(gen, (o,), W_SCALE)
        aq, a = grid(gen, (rank, i), A_SCALE)
        bmq, bm = grid(gen, (o, rank), A_SCALE)
        with torch.no_grad():
            layer.linear.weight.copy_(w)
            layer.linear.bias.copy_(b)
        hook = hj.LoRALinearHook.create_with(layer, rank)
        hook.dropout.p = 0.0
        with torch.no_grad():
            hook.lora_down.weight.copy_(a)
            hook.lora_up.weight.copy_(bm)
            hook.alpha.fill_(ALPHA)
        layer.hook = hook
        hooks[idx] = hook
        ffrec[f"net{idx}"] = dict(wq=wq, bq=bq, aq=aq, bmq=bmq)
    xq, x = grid(gen, (2, 7, nin), X_SCALE, 96)
    gyq, gy = grid(gen, (2, 7, nin), X_SCALE, 96)
    ff.train()
    xi = x.clone().requires_grad_(True)
    y = ff(xi)
    y.backward(gy)
    ffrec.update(xq=xq, gyq=gyq, y=y.detach().clone(), gx=xi.grad.clone())
    with torch.no_grad():  # the low-rank term of net.0 added AFTER the activation instead
        s = 2 * ALPHA / rank  # HijackCustomLinear: the hook runs twice (see above)
        h0, l0, l3 = hooks[0], ff.net[0].linear, ff.net[3].linear
        t = torch.nn.functional.gelu(l0(x) + s * h0.lora_up(h0.lora_down(x)))
        assert rel(l3(t) + s * hooks[3].lora_up(hooks[3].lora_down(t)), y.detach()) < 1e-5
        t = torch.nn.functional.gelu(l0(x)) + s * h0.lora_up(h0.lora_down(x))
        wrong = l3(t) + s * hooks[3].lora_up(hooks[3].lora_down(t))
    ffrec["wrong_order_rel"] = rel(wrong, y.detach())
    out["ff"] = ffrec

    # ---- names: a prepared + injected tiny model, and a fresh hook
    class Tiny(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.ff = cm.FeedForward(16, 32, 0.0, "GELU")
            self.head = hj.HijackLinear(16, 8)

    torch.manual_seed(460)
    tiny = Tiny()
    mgr = hj.LoRAManager()
    mgr.prepare(tiny, key="a", rank=2, target_ancestors={"FeedForward"})
    mgr.inject(tiny, "a")
    fresh = hj.LoRALinearHook(64, 48, rank=8)
    sig = inspect.signature(hj.LoRALinearHook.__init__)
    out["keys"] = dict(
        state_dict=list(tiny.state_dict().keys()), hooks=sorted(mgr.lora_packs["a"].hooks),
        ctor=[(n, None if p.default is inspect.Parameter.empty else p.default, str(p.kind)) for n, p in sig.parameters.items() if n != "self"],
        param_shapes={n: tuple(p.shape) for n, p in fresh.named_parameters()},
        init=dict(down_std_times_rank=float(fresh.lora_down.weight.std()) * 8, up_abs_max=float(fresh.lora_up.weight.abs().max()),
                  alpha=float(fresh.alpha), dropout=fresh.dropout.p))
    try:
        hj.LoRALinearHook(8, 8, rank=9)
        raise AssertionError("rank > min(in, out) must raise")
    except ValueError as e:
        out["keys"]["rank_error"] = str(e)

    torch.save(out, OUT)
    print(f"FeedForward: low-rank term after the activation lands at rel-L2 {ffrec['wrong_order_rel']:.3f} of the reference's output")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
