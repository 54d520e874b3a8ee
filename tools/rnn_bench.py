"""A/B of one recurrent layer on the MI355X: this package's `rnn.GRU` / `rnn.LSTM` (one `functional.linear` for the input projection,
the persistent recurrent kernels of csrc/rnn.hip, one tn GEMM and one column sum for the recurrent parameters) against
`torch.nn.GRU` / `torch.nn.LSTM` on the same device with the same f32 parameters — the reference's own path (modules/ml/rnn.py) on
this GPU —, forward + backward, alternating in one process.

    python tools/rnn_bench.py [--out profiles/r11/rnn_ab.txt] [--rounds 7] [--inner 40]

Sizes: B = 128, T = 64, H = 256 and B = 512, T = 32, H = 128, input width = H, both cells, one direction.  A call is forward, the loss
sum(y * dy) and backward (dx and every parameter gradient).  Every figure is the median over `rounds` alternating rounds of `inner`
back-to-back calls between device events (per call), with the min .. max of the rounds as its spread; the shader clock and socket
power averaged over each variant's timed rounds come from tools/gpu_telemetry.py.  Also printed: the recurrent kernels alone (forward
with saving, backward) and the bytes of packed W_hh they stream from L2 per step and workgroup.  If torch's layer cannot run on the
machine, that is recorded instead of a ratio.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402
from cflearn_amd.functional import SideStream  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402

DEV = "cuda"
WORKLOADS = [(128, 64, 256), (512, 32, 128)]  # (B, T, H)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(variants, rounds, inner, tel):
    """{name: dict(ms=(median, min, max), sclk_mhz, power_w)} of callables run in alternating rounds (two warm-up calls each first)"""
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    spans = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            ms[name].append(timed(fn, inner))
            spans[name].append((t0, time.perf_counter()))
    out = {}
    for name, v in ms.items():
        sums = [tel.summary(t0, t1) for t0, t1 in spans[name]] if tel.available else []
        avg = lambda key: (lambda xs: round(sum(xs) / len(xs), 1) if xs else None)([s[key] for s in sums if s.get(key) is not None])  # noqa: E731
        out[name] = dict(ms=(statistics.median(v), min(v), max(v)), sclk_mhz=avg("sclk_mhz_avg"), power_w=avg("power_w_avg"))
    return out


def fmt(name, r):
    m, lo, hi = r["ms"]
    return f"{name} {m:8.3f} ms ({lo:.3f} .. {hi:.3f}) sclk {r['sclk_mhz']} MHz {r['power_w']} W"


def step_of(layer, x, dy, ours):
    params = list(layer.parameters())

    def go():
        for p in params:
            p.grad = None
        x.grad = None
        y = layer(x) if ours else layer(x)[0]
        y.backward(dy)
        if ours:
            SideStream.join()

    return go


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "rnn_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; one layer, one direction, input width = H; forward + "
             f"backward per call; rounds {args.rounds} x inner {args.inner}; ms per call: median (min .. max over the alternating rounds); "
             f"telemetry: {tel.source.name if tel.available else 'unavailable (' + str(tel.error) + ')'}"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shown = 0

    def flush() -> None:  # (after every section: a later failure keeps what was measured)
        nonlocal shown
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")

    for b, t, h in WORKLOADS:
        for cell in ("GRU", "LSTM"):
            torch.manual_seed(0)
            key = f"{cell}_B{b}_T{t}_H{h}"
            ours = {"GRU": C.rnn.GRU, "LSTM": C.rnn.LSTM}[cell](h, h).to(DEV)
            x = torch.randn(b, t, h, device=DEV, requires_grad=True)
            dy = torch.randn(b, t, h, device=DEV)
            variants = {"hip": step_of(ours, x, dy, True)}
            note = ""
            try:
                ref = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM}[cell](h, h, batch_first=True).to(DEV)
                ref.load_state_dict(ours.state_dict())
                y_ref = ref(x)[0]
                rel = float((ours(x).detach() - y_ref.detach()).norm() / y_ref.detach().norm())
                variants["torch"] = step_of(ref, x, dy, False)
                note = f"   rel-L2(hip, torch f32) {rel:.2e}"
            except Exception as e:  # torch's layer cannot run here: recorded, not hidden
                note = f"   torch.nn.{cell} cannot run on this machine: {type(e).__name__}: {str(e)[:160]}"
            r = alternate(variants, args.rounds, args.inner, tel)
            ratio = f"   torch / hip {r['torch']['ms'][0] / r['hip']['ms'][0]:.2f}x" if "torch" in r else ""
            lines.append(f"{cell} B={b} T={t} H={h}   " + "   ".join(fmt(n, v) for n, v in r.items()) + ratio + note)
            results[key] = r
            # the recurrent kernels alone
            cid = C.rnn.CELL_IDS[cell]
            g = ops.RNN_GATES[cid]
            with torch.no_grad():
                gx = torch.randn(b, t, g * h, device=DEV)
                packed = ops.rnn_pack(ours.weight_hh_l0.detach(), cid)
                bias = ours.bias_hh_l0.detach()
                y, _, _, saved = ops.rnn_fwd(gx, packed, bias, cid, save=True)
                k = alternate({"fwd": lambda: ops.rnn_fwd(gx, packed, bias, cid, y=y, save=True),
                               "bwd": lambda: ops.rnn_bwd(dy, packed, cid, saved, y)}, args.rounds, max(args.inner, 100), tel)
            stream = packed.numel()  # bf16 elements of both packs = bytes of one pack
            lines.append(f"   kernels alone: {fmt('rnn_fwd', k['fwd'])}   {fmt('rnn_bwd', k['bwd'])}   = {k['fwd']['ms'][0] / t * 1e3:.1f} / "
                         f"{k['bwd']['ms'][0] / t * 1e3:.1f} us per step; W_hh pack streamed from L2 per step and workgroup: {stream} B "
                         f"({(b + 15) // 16} workgroups)")
            results[key + "_kernels"] = dict(k, pack_bytes_per_step=stream, workgroups=(b + 15) // 16)
            flush()
            del ours, x, dy
            torch.cuda.empty_cache()
    tel.stop()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
