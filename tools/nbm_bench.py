"""A/B of the nbm module on the MI355X: this package's `NBM` (fused basis kernels of csrc/nbm.hip, featurizer kernels, the f32 head of
`nbm.HeadFn`) against the reference's construction — grouped nn.Conv1d(k = 1, groups = num_bases) layers over [B, num_bases H, D] tensors, a
grouped featurizer convolution and an nn.Linear head (modules/ml/nbm.py), rebuilt HERE from torch layers in f32 — on the same device
with the same parameters, forward + backward, alternating in one process.

    python tools/nbm_bench.py [--out profiles/r13/nbm_ab.txt] [--rounds 5] [--inner 10]

Shapes: B = 512, input_dim = 32 (H = 64), B = 256, input_dim = 64 (H = 128) and B = 128, input_dim = 128 (H = 256), the default order-1 `nary`, 64 bases.  A call is
forward, the loss sum(y * dy) and backward (dx and every parameter gradient).  Every figure is the median over `rounds` alternating
rounds of `inner` back-to-back calls between device events (per call), with the min .. max of the rounds as its spread; the shader
clock and socket power averaged over each variant's timed rounds come from tools/gpu_telemetry.py.  Also printed: the peak memory of one
call of each variant above the resting level, and the basis kernels alone (forward, backward, and the backward as its dW2 launch and the rest).  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402
from cflearn_amd.functional import SideStream  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402
from tools.rnn_bench import alternate, fmt, timed  # noqa: E402

DEV = "cuda"
WORKLOADS = [(512, 32), (256, 64), (128, 128)]  # (B, input_dim); H = 2 * input_dim
NUM_BASES = 64


class TorchNBM(nn.Module):
    """the reference's construction for the default order-1 `nary`: three grouped 1x1 convolutions with ReLU between them, the bases
    transposed to [B, D, NB], a grouped featurizer convolution and a Linear head"""

    def __init__(self, input_dim: int, output_dim: int, num_bases: int, hidden: int):
        super().__init__()
        nb = num_bases
        self.nb, self.d = nb, input_dim
        self.convs = nn.ModuleList([nn.Conv1d(nb, hidden * nb, 1, groups=nb), nn.Conv1d(hidden * nb, hidden * nb, 1, groups=nb),
                                    nn.Conv1d(hidden * nb, nb, 1, groups=nb)])
        self.featurizer = nn.Conv1d(input_dim * nb, input_dim, 1, groups=input_dim)
        self.head = nn.Linear(input_dim, output_dim)

    def load_from(self, m) -> None:
        block = m.bases["1"]
        for mine, theirs in zip(self.convs, block.net):
            mine.load_state_dict(theirs.conv.state_dict())
        self.featurizer.load_state_dict(m.featurizer.state_dict())
        self.head.load_state_dict(m.head.state_dict())

    def forward(self, x):
        b = len(x)
        net = x.view(b, 1, 1, self.d).repeat_interleave(self.nb, 1).contiguous().view(b, self.nb, self.d)
        net = torch.relu(self.convs[0](net))
        net = torch.relu(self.convs[1](net))
        net = self.convs[2](net).transpose(1, 2).contiguous()
        net = self.featurizer(net.view(b, self.d * self.nb, 1)).squeeze(2)
        return self.head(net)


def step_of(model, x, dy, ours):
    params = list(model.parameters())

    def go():
        for p in params:
            p.grad = None
        x.grad = None
        model(x).backward(dy)
        if ours:
            SideStream.join()

    return go


def peak_of(fn) -> int:
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    rest = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - rest


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "nbm_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbm_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; nbm, order-1 nary, {NUM_BASES} bases, H = 2 input_dim; forward "
             f"+ backward per call; rounds {args.rounds} x inner {args.inner}; ms per call: median (min .. max over the alternating rounds); "
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

    for b, f in WORKLOADS:
        torch.manual_seed(0)
        h = 2 * f
        key = f"B{b}_F{f}_H{h}"
        ours = C.NBM(f, 8, num_bases=NUM_BASES).to(DEV)
        ref = TorchNBM(f, 8, NUM_BASES, h).to(DEV)
        ref.load_from(ours)
        x = torch.randn(b, f, device=DEV, requires_grad=True)
        dy = torch.randn(b, 8, device=DEV)
        with torch.no_grad():
            y_ref = ref(x)
            rel = float((ours(x) - y_ref).norm() / y_ref.norm())
        variants = {"hip": step_of(ours, x, dy, True), "torch": step_of(ref, x, dy, False)}
        peaks = {name: peak_of(fn) for name, fn in variants.items()}
        r = alternate(variants, args.rounds, args.inner, tel)
        lines.append(f"B={b} F={f} H={h}   " + "   ".join(fmt(n, v) for n, v in r.items()) + f"   torch / hip {r['torch']['ms'][0] / r['hip']['ms'][0]:.2f}x"
                     f"   rel-L2(hip, torch f32) {rel:.2e}   peak bytes above rest: hip {peaks['hip']}, torch {peaks['torch']}")
        results[key] = dict(r, peak_bytes=peaks, rel_l2=rel)
        del ref, variants
        torch.cuda.empty_cache()
        # the basis kernels alone
        block = ours.bases["1"]
        with torch.no_grad():
            w1, b1, w2, b2, w3, b3 = (t.detach() for conv in (m.conv for m in block.net) for t in (conv.weight, conv.bias))
            w1, b1, w2, b2, w3 = w1.view(NUM_BASES, h, 1), b1.view(NUM_BASES, h), w2.view(NUM_BASES, h, h), b2.view(NUM_BASES, h), w3.view(NUM_BASES, h)
            idx = ops.nbm_index([(i,) for i in range(f)], 1, f, DEV)
            xd = x.detach()
            packed = ops.nbm_pack(w2)
            bases = ops.nbm_bases(xd, idx, w1, b1, packed, b2, w3, b3)
            dbases = torch.randn_like(bases)
            dests = {n: torch.empty_like(t) for n, t in (("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2), ("dw3", w3), ("db3", b3))}
            alone = {"fwd": lambda: ops.nbm_bases(xd, idx, w1, b1, packed, b2, w3, b3, out=bases),
                     "bwd": lambda: ops.nbm_bases_grad(dbases, xd, idx, w1, b1, packed, b2, w3, dests=dests, want_dx=True),
                     "bwd_rest": lambda: ops.nbm_bases_grad(dbases, xd, idx, w1, b1, packed, b2, w3, want_dx=True,
                                                            dests={n: t for n, t in dests.items() if n != "dw2"}),
                     "bwd_dw2": lambda: ops.nbm_bases_grad(dbases, xd, idx, w1, b1, packed, b2, w3, dests={"dw2": dests["dw2"]})}
            k = {}
            for name, fn in alone.items():  # rounds of at least 0.4 s each, so that every figure has telemetry samples beside it
                fn()
                k.update(alternate({name: fn}, args.rounds, max(50, int(400.0 / max(timed(fn, 5), 1e-3))), tel))
        lines.append(f"   kernels alone: {fmt('nbm_bases', k['fwd'])}   {fmt('nbm_bases_grad', k['bwd'])}")
        lines.append(f"   of the backward: {fmt('all but dW2', k['bwd_rest'])}   {fmt('dW2 alone', k['bwd_dw2'])}")
        results[key + "_kernels"] = k
        flush()
        del ours, x, dy
        torch.cuda.empty_cache()
    tel.stop()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
