"""The fused nearest-code search (cfhip_vq_nearest, csrc/vq.hip) against the reference's formula written in torch on the same GPU:
python tools/vq_bench.py [--out FILE]      (default profiles/r07/vq_nearest.txt)

The formula is VQCodebook.forward's (modules/cv/common.py:378-386): sum, einsum, add, argmin, gather over a materialised
[rows, num_codes] f32 distance matrix.  Shapes: the zoo's ae/vq.f4 (32 768 rows = 256^2 images x 8 at 1/4 resolution, 8 192 codes
of 3 channels) and ae/vq.f8 (8 192 rows, 16 384 codes of 4).  Both forms are given the pixels in the layout that suits them best
(the kernel: the bf16 NCHW tensor `to_embedding` leaves; the formula: f32 pixel-major rows, the permute not counted).

Timing: device events around windows of at least 0.2 s after a warm-up of every shape; five rounds, the two forms alternating
inside each round in one process; the median and the spread over the rounds are printed.  Peak transient memory: the high-water
mark of torch's allocator during one call over what was allocated before it.  The FMA rate is computed from the shapes:
rows x codes x (D + 1) fused multiply-adds (D for the dot product, one for sq - 2 dot).  Needs the GPU: there is no fallback."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cflearn_amd import ops  # noqa: E402

SHAPES = [("ae/vq.f4", (8, 3, 64, 64), 8192), ("ae/vq.f8", (8, 4, 32, 32), 16384)]
ROUNDS = 5


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def formula(z_rows, codebook):
    distances = (torch.sum(z_rows ** 2, dim=1, keepdim=True) + torch.sum(codebook ** 2, dim=1)
                 - 2.0 * torch.einsum("bd,dn->bn", z_rows, codebook.t()))
    indices = torch.argmin(distances, dim=1)
    return indices, codebook[indices]


def peak_transient(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    out_path = os.path.join(ROOT, "profiles", "r07", "vq_nearest.txt")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    if not torch.cuda.is_available():
        raise SystemExit("vq_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lines = [f"# tools/vq_bench.py on {torch.cuda.get_device_name(0)}: cfhip_vq_nearest vs the reference's formula in torch; us per call, "
             f"{ROUNDS} rounds alternating in one process"]
    cases = []
    for name, (b, d, h, w), n in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + d)
        z = torch.randn((b, d, h, w), device=dev, generator=g).bfloat16()
        codebook = torch.randn((n, d), device=dev, generator=g)
        sq = ops.vq_code_sqnorm(codebook)
        z_rows = z.float().permute(0, 2, 3, 1).reshape(-1, d).contiguous()
        fused = lambda z=z, codebook=codebook, sq=sq: ops.vq_nearest(z, codebook, code_sq=sq)  # noqa: E731
        torch_form = lambda z_rows=z_rows, codebook=codebook: formula(z_rows, codebook)  # noqa: E731
        for fn in (fused, torch_form):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        idx_a, idx_b = fused()[0].reshape(-1), torch_form()[0]
        agree = float((idx_a == idx_b).float().mean())
        reps = {k: max(10, int(0.2e6 / max(window(fn, 5), 1.0))) for k, fn in (("fused", fused), ("torch", torch_form))}
        cases.append(dict(name=name, rows=b * h * w, codes=n, D=d, fused=fused, torch=torch_form, reps=reps, agree=agree, us=dict(fused=[], torch=[])))
    for _ in range(ROUNDS):
        for case in cases:
            for key in ("fused", "torch"):
                case["us"][key].append(window(case[key], case["reps"][key]))
    for case in cases:
        rec = dict(shape=case["name"], rows=case["rows"], codes=case["codes"], D=case["D"], indices_agree=round(case["agree"], 6))
        for key in ("fused", "torch"):
            us = sorted(case["us"][key])
            rec[key] = dict(reps=case["reps"][key], us_min=round(us[0], 1), us_median=round(us[len(us) // 2], 1), us_max=round(us[-1], 1),
                            peak_transient_mb=round(peak_transient(case[key]) / 2 ** 20, 2))
        fma = case["rows"] * case["codes"] * (case["D"] + 1)
        rec["fused_gfma_per_s"] = round(fma / rec["fused"]["us_median"] / 1e3, 1)
        rec["speedup_median"] = round(rec["torch"]["us_median"] / rec["fused"]["us_median"], 2)
        rec["distance_matrix_mb"] = round(case["rows"] * case["codes"] * 4 / 2 ** 20, 1)
        lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
