"""The first grouped weight-gradient launch of a ViT-B/16 backward (blocks 11 + 10) alone: dense table against the row-periodic
table of fused.HEAD_ROW_DW.

    python tools/head_row_dw_bench.py [--batch 128] [--rounds 7] [--seconds 2.0] [--out profiles/head_row_dw/launch_alone.txt]
Seeded operands with the zero structure the head-only last block leaves: d2, dpre, dx1 and the Q third of dqkv of block 11 are
zero outside rows b * 197.  Dense table = 8 problems as the parent builds them; periodic table = 9 problems (in_w of block 11 cut
into its Q rows, period 197, and its K / V rows, dense).  The two tables alternate in one process, `--seconds` of back-to-back
launches each per round (HIP events around the window; socket power of its second half when telemetry is available, energy per
launch = (power - idle) x time, as tools/energy_table.py measures it); medians over the rounds.  Results are compared bit for bit."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cflearn_amd import ops  # noqa: E402
from tools.energy_table import loop  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda")
    t, d, ff = 197, 768, 3072
    k = args.batch * t
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda r, c: (torch.randn(r, c, generator=g, device=dev) * 0.5).to(torch.bfloat16)  # noqa: E731

    def head_rows(x, cols=None):  # zero outside rows b * t (in the first `cols` columns)
        keep = torch.zeros(k, 1, dtype=torch.bool, device=dev)
        keep[::t] = True
        if cols is None:
            return x * keep
        x[:, :cols] *= keep
        return x

    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    shapes = ((d, ff), (ff, d), (d, d), (3 * d, d))  # w2, w1, out_w, in_w: (M, N)
    last = [(head_rows(rnd(k, d)), rnd(k, ff)), (head_rows(rnd(k, ff)), rnd(k, d)), (head_rows(rnd(k, d)), rnd(k, d)), (head_rows(rnd(k, 3 * d), d), rnd(k, d))]
    prev = [(rnd(k, m), rnd(k, n)) for m, n in shapes]

    def table(periodic: bool):
        probs, outs = [], []
        for i, (dy, x) in enumerate(last + prev):
            m, n = dy.shape[1], x.shape[1]
            w, b = f32(m, n), f32(m)
            outs += [w, b]
            if not periodic or i >= 4:
                probs.append((dy, x, w, False, b, False))
            elif i == 3:
                probs.append((dy[:, :d], x, w[:d], False, b[:d], False, t))
                probs.append((dy[:, d:], x, w[d:], False, b[d:], False))
            else:
                probs.append((dy, x, w, False, b, False, t))
        return probs, outs

    dense, dense_out = table(False)
    rows, rows_out = table(True)
    ops.gemm_grouped_tn(dense)
    ops.gemm_grouped_tn(rows)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(dense_out, rows_out))
    lines = []

    def out(s: str = "") -> None:
        print(s, flush=True)
        lines.append(s)

    tel = GpuTelemetry(0, hz=10.0).start()
    w_idle = None
    if tel.available:
        time.sleep(1.0)
        t0 = time.perf_counter()
        time.sleep(3.0)
        w_idle = tel.summary(t0, time.perf_counter())["power_w_avg"]
    out(f"# first grouped dW launch of the step (blocks 11 + 10), batch {args.batch}, K = {k}: dense table ({len(dense)} problems) vs "
        f"row-periodic table ({len(rows)} problems, period {t}); results bit-equal: {same}")
    out(f"# {args.rounds} rounds, tables alternating, {args.seconds} s of back-to-back launches each; "
        + (f"idle {w_idle} W" if w_idle is not None else f"no power telemetry ({tel.error}): time only"))
    res = {"dense": [], "rows": []}
    for r in range(args.rounds):
        for name, probs in (("dense", dense), ("rows", rows)):
            time.sleep(0.3)
            n, sec, s = loop(lambda: ops.gemm_grouped_tn(probs), args.seconds, tel)
            w = s.get("power_w_avg") if w_idle is not None else None
            mj = (w - w_idle) * sec * 1e3 if w else None
            res[name].append((sec * 1e6, mj))
            out(f"  round {r} {name:5s} {sec * 1e6:8.1f} us / launch over {n} launches" + (f"  {w:7.1f} W  {s['sclk_mhz_avg'] or 0:6.0f} MHz  {mj:7.1f} mJ / launch" if mj is not None else ""))
    for name in ("dense", "rows"):
        us = statistics.median(u for u, _ in res[name])
        mjs = [m for _, m in res[name] if m is not None]
        out(f"median {name:5s} {us:8.1f} us / launch" + (f"  {statistics.median(mjs):7.1f} mJ / launch" if mjs else ""))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
