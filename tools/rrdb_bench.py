"""A/B of the RRDB upscaler on the MI355X: `modules.RRDBNet` (the dense-block convolution of csrc/conv_dense.hip, 15 L + 6 launches)
against the same net composed from what the package offered before it — `modules.Conv2d` on the route `functional.conv_route` gives
each layer, `torch.cat` for the dense blocks, `ops.leaky_relu_fwd`, `functional.upsample2` (ops.upsample2_nhwc) and torch's
element-wise `* 0.2 + inp` on bf16 channels-last activations —, alternating in one process.

    python tools/rrdb_bench.py [--out profiles/r10/rrdb_ab.txt] [--rounds 5] [--inner 2] [--layers 23]

  1. the whole forward, scale 4, 23 layers: 512^2 x 1 and 128^2 x 4, both paths, and the rel-L2 between their outputs;
  2. one dense block's five launches alone (64 -> 32, 96 -> 32, 128 -> 32, 160 -> 32 with LeakyReLU, 192 -> 64 with `* 0.2 + inp`) at
     both sizes: achieved TFLOP/s over the COUNTED FLOPs, 2 x 9 x 26 624 per pixel (no padded channel or MFMA tile counts), and the
     block's least traffic, 1 664 B per pixel (prefixes of 64 .. 192 channels read, 192 channels written), over the same time.
Every figure is the median over `rounds` alternating rounds of `inner` back-to-back calls between device events (per call), with
the min .. max of the rounds as its spread.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
WORKLOADS = [(1, 512), (4, 128)]  # (batch, input side)
RDB_FLOP_PER_PIXEL = 2 * 9 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64)
RDB_BYTES_PER_PIXEL = 2 * (64 + 96 + 128 + 160 + 192) + 2 * 192


def _lrelu(x):
    b, c, h, w = x.shape
    return HF.rows_to_nhwc(ops.leaky_relu_fwd(HF.nhwc_rows(x), 0.2), b, c, h, w)


class _ComposedRDB(torch.nn.Module):
    def __init__(self):
        super().__init__()
        for i in range(4):
            setattr(self, f"conv{i + 1}", C.Conv2d(64 + 32 * i, 32, kernel_size=3))
        self.conv5 = C.Conv2d(192, 64, kernel_size=3)

    def forward(self, net):
        feats = [net]
        for i in range(4):
            feats.append(_lrelu(getattr(self, f"conv{i + 1}")(torch.cat(feats, 1) if i else net)))
        return self.conv5(torch.cat(feats, 1)) * 0.2 + net


class _ComposedRRDB(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _ComposedRDB(), _ComposedRDB(), _ComposedRDB()

    def forward(self, net):
        return self.rdb3(self.rdb2(self.rdb1(net))) * 0.2 + net


class ComposedRRDBNet(torch.nn.Module):
    """rrdb.py:58-102 at scale 4 from the pieces the package had before the dense-block kernel; the state-dict keys of RRDBNet"""

    def __init__(self, num_layers):
        super().__init__()
        self.conv_first = C.Conv2d(3, 64, kernel_size=3)
        self.body = torch.nn.Sequential(*[_ComposedRRDB() for _ in range(num_layers)])
        for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
            setattr(self, name, C.Conv2d(64, 64, kernel_size=3))
        self.conv_last = C.Conv2d(64, 3, kernel_size=3)

    def forward(self, x):
        prev = HF.NHWC[0]
        HF.NHWC[0] = True
        try:
            net = self.conv_first(HF.to_nhwc(x))
            net = net + self.conv_body(self.body(net))
            net = _lrelu(self.conv_up1(HF.upsample2(net)))
            net = _lrelu(self.conv_up2(HF.upsample2(net)))
            return HF.to_nchw(self.conv_last(_lrelu(self.conv_hr(net)))).float()
        finally:
            HF.NHWC[0] = prev


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(variants, rounds, inner):
    """{name: (median, min, max)} ms per call of callables run in alternating rounds (one warm-up call each first)"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(timed(fn, inner))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def fmt(r):
    return "  ".join(f"{name} {m:9.3f} ms ({lo:.3f} .. {hi:.3f})" for name, (m, lo, hi) in r.items())


def rdb_alone(net, batch, side, rounds, inner):
    rows = batch * side * side
    src = torch.randn((rows, 192), device=DEV).to(torch.bfloat16)
    dst = torch.empty((rows, 192), dtype=torch.bfloat16, device=DEV)
    block = net.body[0].rdb1
    packs = [net._packed(getattr(block, f"conv{i + 1}")) for i in range(5)]

    def go():
        for i in range(4):
            cin = 64 + 32 * i
            ops.conv3x3_dense(src[:, :cin], packs[i][0], packs[i][1], src[:, cin:cin + 32], batch, side, side, epilogue="lrelu")
        ops.conv3x3_dense(src, packs[4][0], packs[4][1], dst[:, :64], batch, side, side, epilogue="res1", s1=0.2, r1=src[:, :64])

    return alternate({"rdb": go}, rounds, inner)["rdb"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "rrdb_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--layers", type=int, default=23)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrdb_bench.py measures on the MI355X: no HIP device here")
    torch.manual_seed(0)
    net = C.RRDBNet(num_layers=args.layers).to(DEV).eval()
    old = ComposedRRDBNet(args.layers)
    old.load_state_dict(net.state_dict())
    old = old.to(DEV).eval()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; RRDBNet scale 4, {args.layers} layers; rounds {args.rounds} x "
             f"inner {args.inner}; ms per call: median (min .. max over the alternating rounds)"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shown = 0

    def flush() -> None:  # (after every section: a later failure keeps what was measured)
        nonlocal shown
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")

    with torch.no_grad():
        for batch, side in WORKLOADS:
            x = torch.rand((batch, 3, side, side), device=DEV)
            a, b = net(x), old(x)
            rel = float((a - b).norm() / b.norm())
            del a, b
            r = alternate({"dense": lambda: net(x), "composed": lambda: old(x)}, args.rounds, args.inner)
            lines.append(f"forward {side}^2 x {batch} -> {4 * side}^2   {fmt(r)}   composed / dense {r['composed'][0] / r['dense'][0]:.2f}x   "
                         f"rel-L2(dense, composed) {rel:.2e}")
            results[f"forward_{side}x{batch}"] = dict(r, rel_l2=rel)
            flush()
        for batch, side in WORKLOADS:
            m, lo, hi = rdb_alone(net, batch, side, args.rounds, max(args.inner, 20))
            px = batch * side * side
            lines.append(f"one dense block, 5 launches, {side}^2 x {batch}   {m:8.3f} ms ({lo:.3f} .. {hi:.3f})   "
                         f"{RDB_FLOP_PER_PIXEL * px / m / 1e9:.1f} TFLOP/s counted   {RDB_BYTES_PER_PIXEL * px / m / 1e9:.2f} TB/s least traffic")
            results[f"rdb_{side}x{batch}"] = dict(ms=(m, lo, hi), flop=RDB_FLOP_PER_PIXEL * px, bytes=RDB_BYTES_PER_PIXEL * px)
            flush()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
