"""A/B of Siren on the MI355X: this package's `Siren` (the fused kernels of csrc/siren.hip) against the same module composed HERE from
torch ops as the reference composes it (siren.py:185-187: F.linear -> sin(w .) -> * mod per layer over a [B, N, latent] tensor, then
the head), in f32 and under torch.autocast(bfloat16), on the same device with the same parameters, alternating in one process.

    python tools/siren_bench.py [--out profiles/r15/siren_ab.txt] [--rounds 3] [--inner 5]

Shapes: ImgSiren's stack at 64^2 x 16 and at 256^2 x 1 (latent 256, 4 layers, in 2, out 3, the grid shared by the samples) and the DDR
form B = 512, N = 16 (latent 128, 2 layers, in 1, out 2, a tuple of modulations and per-row coordinates).  Measured: the forward alone
(no gradient wanted) and forward + loss sum(y * dy) + backward (every parameter, the latent or the modulations, and `init` in the DDR
form).  Every figure is the median over `rounds` alternating rounds of back-to-back calls between device events, with the min .. max
of the rounds; the shader clock and socket power averaged over each variant's timed rounds come from tools/gpu_telemetry.py.  Also
printed: the peak memory of one call of each variant above the resting level and the rel-L2 distance of the fused output from the
composed f32 one.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd.functional import SideStream  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402
from tools.nbm_bench import peak_of  # noqa: E402
from tools.rnn_bench import alternate, fmt, timed  # noqa: E402

DEV = "cuda"
# (name, size, in_dim, out_dim, latent, layers, B, N for the tuple form or None)
WORKLOADS = [("img_64x64_x16", 64, 2, 3, 256, 4, 16, None), ("img_256x256_x1", 256, 2, 3, 256, 4, 1, None), ("ddr_B512_N16", None, 1, 2, 128, 2, 512, 16)]


class TorchSiren(nn.Module):
    """the reference's Siren.forward in torch ops: its composition, restated; parameters under the reference's names"""

    def __init__(self, ours: "C.Siren"):
        super().__init__()
        self.ours = ours

    def forward(self, inp, *, init=None):
        o = self.ours
        if o.modulator is None:
            mods = inp
        else:
            net, mods = inp, []
            for block in o.modulator.blocks:
                net = F.relu(F.linear(net, block[0].weight, block[0].bias))
                mods.append(net)
                net = torch.cat((net, inp), dim=1)
        net = init if init is not None else o.grid.repeat(mods[0].shape[0], 1, 1)
        for i, (block, mod) in enumerate(zip(o.blocks, mods)):
            net = torch.sin((o.w_sin_initial if i == 0 else o.w_sin) * F.linear(net, block.weight, block.bias)) * mod[:, None]
        return F.linear(net, o.head.weight, o.head.bias)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "siren_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("siren_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; Siren, fused (hip) against the composed module in f32 (torch_f32) "
             f"and under bf16 autocast (torch_bf16); rounds {args.rounds} of >= {args.inner} calls and >= 0.2 s; ms per call: median (min .. max "
             f"over the alternating rounds); telemetry: {tel.source.name if tel.available else 'unavailable (' + str(tel.error) + ')'}"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shown = 0

    def flush() -> None:  # (after every section: a later failure keeps what was measured)
        nonlocal shown
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")

    for name, size, din, dout, latent, layers, b, n in WORKLOADS:
        torch.manual_seed(0)
        tuple_form = n is not None
        ours = C.Siren(size, din, dout, latent, num_layers=layers, bias=not tuple_form, use_modulator=not tuple_form).to(DEV)
        ref = TorchSiren(ours)
        params = list(ours.parameters())
        if tuple_form:
            mods = tuple(torch.randn(b, latent, device=DEV, requires_grad=True) for _ in range(layers))
            init = (torch.rand(b, n, din, device=DEV) * 2.0 - 1.0).requires_grad_(True)
            leaves, call = [*mods, init], lambda m: m(mods, init=init)  # noqa: E731
        else:
            z = torch.randn(b, latent, device=DEV, requires_grad=True)
            leaves, call, n = [z], lambda m: m(z), size * size  # noqa: E731
        dy = torch.randn(b, n, dout, device=DEV)

        def autocast(fn):
            def go():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return fn()
            return go

        def fwd_of(m):
            def go():
                with torch.no_grad():
                    return call(m)
            return go

        def step_of(m, is_ours):
            def go():
                for p in params + leaves:
                    p.grad = None
                (call(m).float() * dy).sum().backward()
                if is_ours:
                    SideStream.join()
            return go

        with torch.no_grad():
            y_ref = call(ref)
            rel = float((call(ours).float() - y_ref).norm() / y_ref.norm())
            with torch.autocast("cuda", dtype=torch.bfloat16):
                rel16 = float((call(ref).float() - y_ref).norm() / y_ref.norm())
        sections = {"forward": {"hip": fwd_of(ours), "torch_f32": fwd_of(ref), "torch_bf16": autocast(fwd_of(ref))},
                    "forward + backward": {"hip": step_of(ours, True), "torch_f32": step_of(ref, False), "torch_bf16": autocast(step_of(ref, False))}}
        lines.append(f"{name}: M = {b * n} rows, latent {latent}, {layers} layers, in {din}, out {dout}; rel-L2 from the composed f32 output: "
                     f"hip {rel:.2e}, torch_bf16 {rel16:.2e}")
        results[name] = dict(rel_l2=rel, rel_l2_bf16=rel16)
        for what, variants in sections.items():
            peaks = {k: peak_of(fn) for k, fn in variants.items()}
            inner = max(args.inner, int(200.0 / max(max(timed(fn, 2) for fn in variants.values()), 1e-3)))
            r = alternate(variants, args.rounds, inner, tel)
            lines.append(f"   {what}: " + "   ".join(fmt(k, v) for k, v in r.items()))
            lines.append(f"      torch_f32 / hip {r['torch_f32']['ms'][0] / r['hip']['ms'][0]:.2f}x   torch_bf16 / hip "
                         f"{r['torch_bf16']['ms'][0] / r['hip']['ms'][0]:.2f}x   peak bytes above rest: " + ", ".join(f"{k} {v}" for k, v in peaks.items()))
            results[name][what] = dict(r, peak_bytes=peaks, inner=inner)
            flush()
        del ours, ref, leaves, dy, sections
        torch.cuda.empty_cache()
    tel.stop()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
