"""Generate tests/golden/lora_conv.pt: the reference's own `HijackConv2d` + `LoRAConvHook` (modules/core/hijacks.py:208-266) on the
CPU in fp32.

    python tools/gen_lora_conv_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * layers: cases (Cin, Cout, k, stride, pad, rank, H, W) of CASES, batch 2, hook attached (dropout 0).  Recorded: the training
    output `y` and the gradients of x (`gx`), lora_down.weight (`ga`) and lora_up.weight (`gbm`), run with the base unfrozen and
    frozen (the same bits, asserted; stored once); the gradients of the base weight (every `row_step`-th output channel) and bias;
    for the 1x1 case the eval-mode output and the injected weight (the reference's `get_updown` is exact there); for the 3x3 cases
    `eval_ref_rel`, the rel-L2 distance of the reference's OWN eval-mode output from its training-mode output: its `get_updown`
    (hijacks.py:143) takes tap [0, 0] of `lora_down` and broadcasts it over all nine taps.  The eval target of a 3x3 case is `y`.
    Asserted here: a plain F.conv2d with the exactly merged filter W + s sum_c up[o][c] down[c][i][ky][kx] reproduces `y` to 1e-5.
  * keys: the hook names of a tiny module (a block of one HijackConv2d and one HijackLinear) after `LoRAManager.prepare` + `inject`, its state-dict
    keys, and the constructor signature / parameter shapes / init statistics of a fresh hook.
Single-threaded and seeded: a second run writes the same bytes.

Every tensor the tests feed in lies on a coarse grid and is stored as int8 codes (decode q as q.float() * <name>_scale; all of them
exact in bf16), `lora_up.weight` gets seeded non-zero codes (its zero init would hide the adapter), alpha is 0.8."""
import inspect
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lora_conv.pt")
CASES = ((8, 16, 1, 1, 0, 4, 5, 7), (32, 40, 3, 1, 1, 4, 5, 7), (32, 64, 3, 2, 1, 17, 6, 9), (64, 32, 3, 1, 1, 16, 8, 8))
BATCH = 2
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
    out: dict = {"layers": [], "scales": dict(w=W_SCALE, x=X_SCALE, a=A_SCALE), "alpha": ALPHA, "batch": BATCH}

    def hooked(cin, cout, k, stride, pad, rank, w, b, a, bm):
        m = hj.HijackConv2d(cin, cout, k, stride, pad)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        hook = hj.LoRAConvHook.create_with(m, rank)
        hook.dropout.p = 0.0
        with torch.no_grad():
            hook.lora_down.weight.copy_(a)
            hook.lora_up.weight.copy_(bm)
            hook.alpha.fill_(ALPHA)
        m.hook = hook
        return m, hook

    for si, (cin, cout, k, stride, pad, rank, h, w_) in enumerate(CASES):
        gen = torch.Generator().manual_seed(500 + si)
        wq, w = grid(gen, (cout, cin, k, k), W_SCALE)
        bq, b = grid(gen, (cout,), W_SCALE)
        aq, a = grid(gen, (rank, cin, k, k), A_SCALE)
        bmq, bm = grid(gen, (cout, rank, 1, 1), A_SCALE)
        xq, x = grid(gen, (BATCH, cin, h, w_), X_SCALE, 96)
        ho, wo = (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1
        gyq, gy = grid(gen, (BATCH, cout, ho, wo), X_SCALE, 96)
        step = max(1, cout // 6)
        rec = dict(case=(cin, cout, k, stride, pad, rank, h, w_), wq=wq, bq=bq, aq=aq, bmq=bmq, xq=xq, gyq=gyq, row_step=step)
        r: dict = {}
        for frozen in (False, True):
            m, hook = hooked(cin, cout, k, stride, pad, rank, w, b, a, bm)
            m.train()
            m.weight.requires_grad_(not frozen)
            m.bias.requires_grad_(not frozen)
            xi = x.clone().requires_grad_(True)
            y = m(xi)
            y.backward(gy)
            got = dict(y=y.detach().clone(), gx=xi.grad.clone(), ga=hook.lora_down.weight.grad.clone(),
                       gbm=hook.lora_up.weight.grad.clone())
            if frozen:  # freezing the base changes none of these: stored once
                assert all(torch.equal(got[key], r[key]) for key in got)
                assert m.weight.grad is None and m.bias.grad is None
            else:
                r["gw_rows"] = m.weight.grad[::step].clone()
                r["gb"] = m.bias.grad.clone()
            r.update(got)
            assert hook.alpha.grad is None  # `alpha.item()`: no gradient in the reference either
        # the exactly merged filter reproduces the training output
        s = ALPHA / rank
        with torch.no_grad():
            merged = w + s * torch.einsum("oc,cikl->oikl", bm[:, :, 0, 0], a)
            merged_rel = rel(F.conv2d(x, merged, b, stride, pad), r["y"])
        assert merged_rel < 1e-5, merged_rel
        rec["merged_rel"] = merged_rel
        m, hook = hooked(cin, cout, k, stride, pad, rank, w, b, a, bm)
        m.eval()
        with torch.no_grad():
            y_eval = m(x).clone()
            assert hook.injected
            w_inj = m.weight.detach().clone()
            hook.cleanup()
            assert torch.equal(m.weight.detach(), w)
        if k == 1:
            assert rel(y_eval, r["y"]) < 1e-5 and rel(w_inj, merged) < 1e-6
            r["y_eval"], r["w_injected"] = y_eval, w_inj
        else:  # hijacks.py:143: tap [0, 0] of lora_down, broadcast over the nine taps
            with torch.no_grad():
                bcast = w + s * (bm[:, :, 0, 0] @ a[:, :, 0, 0])[..., None, None]
            assert torch.allclose(w_inj, bcast, atol=1e-6)
            r["eval_ref_rel"] = rel(y_eval, r["y"])
        rec.update(r)
        out["layers"].append(rec)
        print(f"case {rec['case']}: merged filter vs training output {merged_rel:.1e}"
              + (f", the reference's eval output vs its training output {r['eval_ref_rel']:.3f}" if k == 3 else ""))

    # ---- names: a prepared + injected tiny module, and a fresh hook
    class Block(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.conv = hj.HijackConv2d(8, 16, 3, 1, 1)
            self.head = hj.HijackLinear(16, 8)

    class Tiny(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.block = Block()

    torch.manual_seed(560)
    tiny = Tiny()
    mgr = hj.LoRAManager()
    mgr.prepare(tiny, key="a", rank=2, target_ancestors={"Block"})
    mgr.inject(tiny, "a")
    fresh = hj.LoRAConvHook(32, 40, 3, 1, 1, rank=4)
    sig = inspect.signature(hj.LoRAConvHook.__init__)
    out["keys"] = dict(
        state_dict=list(tiny.state_dict().keys()), hooks=sorted(mgr.lora_packs["a"].hooks),
        hook_classes={name: type(hk).__name__ for name, hk in mgr.lora_packs["a"].hooks.items()},
        ctor=[(n, None if p.default is inspect.Parameter.empty else p.default, str(p.kind)) for n, p in sig.parameters.items() if n != "self"],
        param_shapes={n: tuple(p.shape) for n, p in fresh.named_parameters()},
        init=dict(down_std_times_rank=float(fresh.lora_down.weight.detach().std()) * 4, up_abs_max=float(fresh.lora_up.weight.abs().max()),
                  alpha=float(fresh.alpha), dropout=fresh.dropout.p))
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
