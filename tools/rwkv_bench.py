"""A/B of the RWKV token mixer on the MI355X: this package's `RWKVTokenMixer` (time-mix and WKV scan kernels of csrc/rwkv.hip, bf16
GEMMs) against a torch restatement of the reference's formula (mixed_stacks/token_mixers.py:170-206) written out HERE in f32 — the
time shift by padding, three mixes, nn.Linear layers, and the WKV term as two grouped conv1d calls with T-tap kernels — on the same
device with the same parameters, forward + backward, alternating in one process.

    python tools/rwkv_bench.py [--out profiles/r14/rwkv_ab.txt] [--rounds 3] [--inner 3]

Shapes: B = 128, T = 197, C = L = 768 and B = 8, T = 1024, C = L = 256.  A call is forward, the loss sum(y * dy) and backward (dx and
every parameter gradient).  Every figure is the median over `rounds` alternating rounds of back-to-back calls between device events
(per call; at least `inner` calls and at least 0.4 s per round, so that both variants have telemetry samples), with the min .. max
of the rounds as its spread; the shader clock and socket power averaged over each variant's timed rounds come from
tools/gpu_telemetry.py.  Also printed: the scan launches alone (forward with and without saving, backward with
and without d info_decay) and the peak memory of one call of each variant above the resting level.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402
from cflearn_amd.functional import SideStream  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402
from tools.nbm_bench import peak_of  # noqa: E402
from tools.rnn_bench import alternate, fmt, timed  # noqa: E402

DEV = "cuda"
WORKLOADS = [(128, 197, 768, 768), (8, 1024, 256, 256)]  # (B, T, C, L)


class TorchRWKV(nn.Module):
    """the reference's token mixer in torch ops, f32: its formula, restated"""

    def __init__(self, num_tokens: int, in_dim: int, latent_dim: int):
        super().__init__()
        self.ci = latent_dim
        self.key = nn.Linear(in_dim, latent_dim, bias=False)
        self.value = nn.Linear(in_dim, latent_dim, bias=False)
        self.receptance = nn.Linear(in_dim, latent_dim, bias=False)
        self.output = nn.Linear(latent_dim, in_dim, bias=False)
        self.info_decay = nn.Parameter(torch.zeros(latent_dim, 1))
        self.register_buffer("time_curve", torch.arange(-num_tokens + 1, 1)[None])
        self.time_mix_k = nn.Parameter(torch.zeros(1, 1, in_dim))
        self.time_mix_v = nn.Parameter(torch.zeros(1, 1, in_dim))
        self.time_mix_r = nn.Parameter(torch.zeros(1, 1, in_dim))

    def forward(self, net):
        t = net.shape[1]
        shifted = F.pad(net, (0, 0, 1, -1))
        net_k = net * self.time_mix_k + shifted * (1.0 - self.time_mix_k)
        net_v = net * self.time_mix_v + shifted * (1.0 - self.time_mix_v)
        net_r = net * self.time_mix_r + shifted * (1.0 - self.time_mix_r)
        net_k = self.key(net_k).transpose(1, 2)
        net_v = self.value(net_v).transpose(1, 2)
        exp_w = (self.info_decay.exp() * self.time_curve).exp()[:, None]
        exp_k = net_k.exp()
        net_kv = exp_k * net_v
        wk = F.conv1d(F.pad(exp_k, (t - 1, 0, 0, 0)), exp_w, groups=self.ci)
        net_kv = net_kv / (wk + 1.0e-6)
        wkv = F.conv1d(F.pad(net_kv, (t - 1, 0, 0, 0)), exp_w, groups=self.ci).transpose(1, 2)
        return self.output(torch.sigmoid(self.receptance(net_r)) * wkv).contiguous()


def step_of(model, x, dy, ours):
    params = list(model.parameters())

    def go():
        for p in params:
            p.grad = None
        x.grad = None
        (model(x).float() * dy).sum().backward()
        if ours:
            SideStream.join()

    return go


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "rwkv_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rwkv_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; rwkv token mixer, layer 1 of 4; forward + backward per call; "
             f"rounds {args.rounds} of >= {args.inner} calls and >= 0.4 s; ms per call: median (min .. max over the alternating rounds); "
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

    for b, t, c, l in WORKLOADS:
        torch.manual_seed(0)
        key = f"B{b}_T{t}_C{c}_L{l}"
        ours = C.RWKVTokenMixer(1, 4, t, c, l)
        with torch.no_grad():
            for m in (ours.key, ours.value, ours.receptance, ours.output):
                m.weight.normal_(0.0, 0.03)
        ours = ours.to(DEV)
        x = torch.randn(b, t, c, device=DEV, requires_grad=True)
        dy = torch.randn(b, t, c, device=DEV)
        # the scan launches alone
        with torch.no_grad():
            kk, vv, rr = (torch.randn(b, t, l, device=DEV) for _ in range(3))
            w = ours.info_decay.detach().reshape(-1)
            y, sa, sb = ops.rwkv_wkv(kk, vv, rr, w, save=True)
            dyb = torch.randn(b, t, l, device=DEV).bfloat16()
            dd = torch.empty(l, device=DEV)
            alone = {"fwd": lambda: ops.rwkv_wkv(kk, vv, rr, w), "fwd_save": lambda: ops.rwkv_wkv(kk, vv, rr, w, save=True),
                     "bwd": lambda: ops.rwkv_wkv_grad(dyb, kk, vv, rr, w, sa, sb, d_decay=dd),
                     "bwd_frozen": lambda: ops.rwkv_wkv_grad(dyb, kk, vv, rr, w, sa, sb)}
            k = {}
            for name, fn in alone.items():
                fn()
                k.update(alternate({name: fn}, args.rounds, max(20, int(200.0 / max(timed(fn, 5), 1e-3))), tel))
        gb = b * t * l / 1e9
        lines.append(f"B={b} T={t} C={c} L={l}   scan alone: {fmt('fwd', k['fwd'])}   {fmt('fwd + save', k['fwd_save'])}")
        lines.append(f"   {fmt('bwd', k['bwd'])}   {fmt('bwd, info_decay frozen', k['bwd_frozen'])}   "
                     f"(bytes moved: fwd {14 * gb:.3f} GB, fwd + save {22 * gb:.3f} GB, bwd {28 * gb:.3f} GB)")
        results[key + "_scan"] = k
        flush()
        del kk, vv, rr, y, sa, sb, dyb, alone
        torch.cuda.empty_cache()
        ref = TorchRWKV(t, c, l).to(DEV)
        ref.load_state_dict(ours.state_dict())
        with torch.no_grad():
            y_ref = ref(x)
            rel = float((ours(x).float() - y_ref).norm() / y_ref.norm())
        variants = {"hip": step_of(ours, x, dy, True), "torch": step_of(ref, x, dy, False)}
        peaks = {name: peak_of(fn) for name, fn in variants.items()}
        # each variant's round lasts at least 0.4 s, so that the telemetry has samples beside both (the fused call is ~20 x shorter)
        r = {}
        order = list(variants)
        inner = {}
        for name, fn in variants.items():
            fn()
            inner[name] = max(args.inner, int(400.0 / max(timed(fn, 3), 1e-3)))
        spans = {name: [] for name in order}
        ms = {name: [] for name in order}
        for _ in range(args.rounds):
            for name in order:
                t0 = time.perf_counter()
                ms[name].append(timed(variants[name], inner[name]))
                spans[name].append((t0, time.perf_counter()))
        for name in order:
            sums = [tel.summary(t0, t1) for t0, t1 in spans[name]] if tel.available else []
            avg = lambda key: (lambda xs: round(sum(xs) / len(xs), 1) if xs else None)([s[key] for s in sums if s.get(key) is not None])  # noqa: E731
            r[name] = dict(ms=(statistics.median(ms[name]), min(ms[name]), max(ms[name])), sclk_mhz=avg("sclk_mhz_avg"),
                           power_w=avg("power_w_avg"), inner=inner[name])
        lines.append(f"   module, forward + backward: " + "   ".join(fmt(n, v) for n, v in r.items())
                     + f"   torch / hip {r['torch']['ms'][0] / r['hip']['ms'][0]:.2f}x   rel-L2(hip, torch f32) {rel:.2e}   "
                     f"peak bytes above rest: hip {peaks['hip']}, torch {peaks['torch']}")
        results[key] = dict(r, peak_bytes=peaks, rel_l2=rel)
        flush()
        del ours, ref, variants, x, dy
        torch.cuda.empty_cache()
    tel.stop()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
