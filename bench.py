"""bench.py — ViT-B/16 224^2 bf16 training step on N MI355X (one process per GPU, RCCL all-reduce).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path over one synthetic batch that is already resident in HBM:
patch embedding -> 12 pre-norm transformer blocks -> head LN + Linear -> softmax-CE -> full backward
-> (N > 1: bucketed gradient all-reduce) -> fused AdamW update of all 86.6 M parameters.
Rank 0 prints ONE JSON line (metric = BASELINE.json's: train samples/sec + step ms).
`--dump-outputs DIR` also writes what the last timed step handed back (its loss and the updated parameters, sampled) as
DIR/<name>.npy: the inputs are seeded, so two builds run with the same arguments can be compared output for output.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs and the line.  Every
measurement that runs work of its own behind the timed steps (`calibration`, `roofline` / `hbm`, `other_workloads`,
`cpu_baseline`; with --workload unet | clip the FLOP-counted `roofline` step) comes with `--full`; the --no-* options
drop single ones from a --full run.

Extra fields / objects (* = --full only):
  host_issue_ms_per_step   wall time the host needed to ISSUE the timed steps (it never waits for the device inside): the device is
                the bound when this is well below ms_per_step (ViT: 10.3 of 18.0 ms), the Python path when it is not.
  step_ms       median / p10 / p90 / min / max of per-step HIP-event timings;  other_workloads*: UNet 64^2 x 8, UNet 256^2 x 1 (BASELINE
                config 4 as stated) and CLIP b256 steps.
  streams       did every helper stream (batch slices, weight-gradient lane, comm stream) get a hardware queue of its own
                (functional.stream_report)?  `distinct: false` = a serialised step; a multi-GPU run then exits non-zero.
  rccl          (N > 1 / --force-ddp) who launches the collectives, ncclCommCount / ncclCommUserRank of the C-ABI communicator,
                NCCL_MAX_NCHANNELS (--nchannels), buckets, wire dtype, the all-reduce self-test.
  roofline*     dominant kernel family = the MFMA GEMM (`gemm_grouped_tn_kernel<*>` / `gemm_bf16_kernel<*>`, 96 % of the step's
                FLOPs).  `achieved` = algorithmic FLOPs of every GEMM launch of one step (2*M*N*K each, the per-sample
                figure of SURVEY §8d x the batch) / the SUM OF THEIR IN-STEP DURATIONS: HIP-event pairs around every
                GEMM launch of real training steps, on the stream each one is launched on (`ops.GemmTimer`) — the same
                quantity a `rocprofv3 --kernel-trace --stats` run of this command reports (profiles/).  Because three
                streams overlap, that sum exceeds the wall time of the step; two more views are carried next to it:
                `isolated` (each shape timed alone, random operands) and `wall` (GEMM FLOPs / measured step time — the
                lower bound nobody can argue with).  peak = 2500 TFLOP/s dense bf16.
                `dominant_kernel`: `by_kernel` = in-step timings summed per kernel INSTANTIATION (cfhip_gemm_kernel_name: the row a
                rocprofv3 --stats summary lists first), `by_launch_shape` = the single launch shape with the most time.
                `traffic` = HBM-side bytes of the family from PMC passes (tools/gpu/run.sh pmc): only reported when
                the committed pass was taken on THIS kernel source (sha256 of the GEMM sources recorded in the JSON),
                otherwise null with `traffic_stale`.
  cpu_baseline* the same step (fwd + CE + bwd + AdamW) on the host cores, bounded sample.  kind "reference": the
                reference's own modules imported from /root/reference (build container); kind "port": the oracle
                restatement (oracle/vit_oracle.py) where the reference tree is absent (the GPU box).  fp32 and
                bf16-autocast, all host cores.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FLOP_PER_SAMPLE = 105.38e9  # fwd + bwd, SURVEY §8d (17 563 828 224 MAC fwd x 2 x 3)
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)


def gemm_shapes(batch: int, t: int = 197, d: int = 768, dff: int = 3072, layers: int = 12, classes: int = 1000,
                grouped=None):
    """(count, layout, M, N, K, epilogue) of every GEMM launch in one training step.  The forward of the block stack runs
    as `fused.FWD_HALVES` batch slices (one launch per slice and operator); the backward is one pass over the batch.
    The weight gradients of the blocks are grouped launches (`fused.DW_GROUP_BLOCKS` blocks each; `grouped=False`: the
    per-GEMM rows): (count, "tn-grouped", ((M, N, K), ...), 0, 0, "none")."""
    from cflearn_amd import fused

    m = batch * t
    mp = batch * (t - 1)
    L = layers
    nsl = fused.FWD_HALVES if batch >= 2 * fused.FWD_HALVES else 1
    fwd = []
    for i in range(nsl):
        ms = (batch * (i + 1) // nsl - batch * i // nsl) * t
        fwd += [(L, "nt", ms, 3 * d, d, "bias"), (L, "nt", ms, d, d, "residual"), (L, "nt", ms, dff, d, "gelu"),
                (L, "nt", ms, d, dff, "residual")]
    merged = {}
    for c, lay, mm, n, k, e in fwd:  # equal slices are one shape with twice the count
        merged[(lay, mm, n, k, e)] = merged.get((lay, mm, n, k, e), 0) + c
    # backward dX = dY W (W read n-major through the transposing LDS read): `fused.BWD_HALVES` batch slices as well
    nbs = fused.BWD_HALVES if batch >= 2 * fused.BWD_HALVES else 1
    bwd = {}
    for i in range(nbs):
        ms = (batch * (i + 1) // nbs - batch * i // nbs) * t
        for key in (("nn", ms, dff, d, "dgelu"), ("nn", ms, d, dff, "none"), ("nn", ms, d, d, "none"), ("nn", ms, d, 3 * d, "none")):
            bwd[key] = bwd.get(key, 0) + L
    return [(c,) + key for key, c in merged.items()] + [(c,) + key for key, c in bwd.items()] + [
        (1, "nt", mp, d, d, "bias"), (1, "nt", batch, classes, d, "bias"), (1, "nn", batch, d, classes, "none"),
        # backward dW = dY^T X (both operands token-major)
        (1, "tn", d, d, mp, "none"), (1, "tn", classes, d, batch, "none"),
    ] + _dw_rows(L, d, dff, m, fused.DW_GROUP_BLOCKS if grouped is None else (fused.DW_GROUP_BLOCKS if grouped else 0))


def _dw_rows(L: int, d: int, dff: int, m: int, nb: int):
    per_block = ((d, dff, m), (dff, d, m), (d, d, m), (3 * d, d, m))
    if nb <= 0:  # round-1/2 path: one split-K GEMM (+ reduce) per weight gradient
        return [(L, "tn") + sh + ("none",) for sh in per_block]
    rows = []
    if L // nb:
        rows.append((L // nb, "tn-grouped", per_block * nb, 0, 0, "none"))
    if L % nb:
        rows.append((1, "tn-grouped", per_block * (L % nb), 0, 0, "none"))
    return rows


def gemm_launchers(batch: int):
    """Every GEMM launch shape of the step as (row description, launch closure, count per step, FLOPs, algorithmic bytes): seeded
    random operands resident in HBM, the epilogue operands of the model (f32 residual stream, saved pre-activation).  Shared by
    `time_gemms` (isolated timings) and tools/energy_table.py (joules per launch)."""
    from cflearn_amd import ops

    dev = torch.device("cuda", torch.cuda.current_device())
    bf = torch.bfloat16
    for count, layout, m, n, k, epi in gemm_shapes(batch):
        if layout == "tn-grouped":
            g = torch.Generator(device=dev).manual_seed(len(m))
            rnd = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.5).to(bf)  # noqa: E731
            probs = [(rnd(kk, mm), rnd(kk, nn), torch.empty(mm, nn, dtype=torch.float32, device=dev), False,
                      torch.empty(mm, dtype=torch.float32, device=dev), False) for mm, nn, kk in m]
            flops = sum(2.0 * mm * nn * kk for mm, nn, kk in m)
            nbytes = sum(2.0 * (mm * kk + nn * kk) + 4.0 * mm * nn for mm, nn, kk in m)
            yield (dict(layout=layout, problems=[list(x) for x in m], count=count), (lambda probs=probs: ops.gemm_grouped_tn(probs)),
                   count, flops, nbytes)
            del probs
            continue
        g = torch.Generator(device=dev).manual_seed(m + n + k)
        rnd = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.5).to(bf)  # noqa: E731
        if layout == "nt":
            a, b, kw = rnd(m, k), rnd(n, k), {}
        elif layout == "nn":
            a, b, kw = rnd(m, k), rnd(k, n), dict(b_trans=True)
        else:
            a, b, kw = rnd(k, m), rnd(k, n), dict(a_trans=True, b_trans=True, out_dtype=torch.float32,
                                                  split_k=ops.pick_split_k(m, n, k))
        bias = torch.zeros(n, device=dev) if epi in ("bias", "residual", "gelu") else None
        # algorithmic HBM bytes of one launch: both operands once, the output once, epilogue operands once
        nbytes = 2.0 * (m * k + n * k) + 2.0 * m * n
        if epi == "gelu":
            kw.update(epilogue=ops.EPI_GELU, aux_out=torch.empty(m, n, dtype=bf, device=dev))
            nbytes += 2.0 * m * n  # the saved pre-activation
        elif epi == "residual":  # f32 residual stream in and out, as in the model
            kw.update(epilogue=ops.EPI_RESIDUAL, aux_in=torch.randn(m, n, generator=g, device=dev), out_dtype=torch.float32)
            nbytes += 2.0 * m * n + 4.0 * m * n
        elif epi == "dgelu":
            kw.update(epilogue=ops.EPI_DGELU, aux_in=rnd(m, n))
            nbytes += 2.0 * m * n
        if layout == "tn":
            nbytes += 2.0 * m * n  # f32 gradient output
        out = torch.empty(m, n, dtype=kw.pop("out_dtype", bf), device=dev)
        yield (dict(layout=layout, M=m, N=n, K=k, epilogue=epi, count=count),
               (lambda a=a, b=b, bias=bias, out=out, kw=kw: ops.gemm(a, b, bias=bias, out=out, **kw)), count, 2.0 * m * n * k, nbytes)


def time_gemms(batch: int, reps: int):
    """Event-timed duration of every GEMM shape of the step (steady state, same stream)."""
    rows = []
    tot_flops = tot_time = tot_bytes = 0.0
    for desc, fn, count, flops, nbytes in gemm_launchers(batch):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        dur = e0.elapsed_time(e1) * 1e-3 / reps
        rows.append(dict(desc, us=round(dur * 1e6, 1), tflops=round(flops / dur / 1e12, 1), algorithmic_mb=round(nbytes / 1e6, 1)))
        tot_flops += count * flops
        tot_time += count * dur
        tot_bytes += count * nbytes
    return tot_flops, tot_time, rows, tot_bytes


GEMM_SOURCES = ("gemm.hip", "gemm_device.h", "gemm_grouped.hip", "common.h")  # what a PMC pass of the GEMM family is valid for


def _gemm_source_hash() -> str:
    import hashlib

    hsh = hashlib.sha256()
    for name in GEMM_SOURCES:
        with open(os.path.join(ROOT, "carefree-learn_amd", "csrc", name), "rb") as f:
            hsh.update(f.read())
    return hsh.hexdigest()[:16]


def pmc_traffic(batch: int):
    """HBM bytes per step of the GEMM family from the newest committed PMC passes (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE over this script, tools/gpu/run.sh pmc -> tools/pmc_step_summary.py).  A pass is only valid for the
    kernel sources it was taken on (GEMM_SOURCES): returns (bytes or None, source path, whole-step bytes or None, stale note or None)."""
    best = None
    for rnd in sorted(os.listdir(os.path.join(ROOT, "profiles")), reverse=True):
        path = os.path.join(ROOT, "profiles", rnd, f"pmc_step_b{batch}.json")
        if os.path.isfile(path):
            best = path
            break
    if best is None:
        return None, None, None, "no PMC pass committed for this batch"
    with open(best) as f:
        doc = json.load(f)
    rel = os.path.relpath(best, ROOT)
    if doc.get("gemm_source_sha256_16") != _gemm_source_hash():
        return None, rel, None, (f"{rel} was taken on other GEMM sources "
                                 f"({doc.get('gemm_source_sha256_16', 'unrecorded')} != {_gemm_source_hash()})")
    fam = doc["families"].get("gemm")
    return (fam["total"] if fam else None), rel, doc.get("all_kernels", {}).get("total"), None


def time_gemms_in_step(ts, batch_fn, steps: int):
    """In-step GEMM durations: event pairs around every GEMM launch of `steps` real training steps."""
    from cflearn_amd import ops

    timer = ops.GemmTimer()
    ops.GEMM_TIMER = timer
    try:
        ts.step(*batch_fn())  # one step with the event pairs that does not count (event objects, allocator)
        torch.cuda.synchronize()
        timer.records.clear()
        for _ in range(steps):
            ts.step(*batch_fn())
        torch.cuda.synchronize()
    finally:
        ops.GEMM_TIMER = None
    rows, tot_t, tot_f = [], 0.0, 0.0
    for (layout, m, n, k, epi), (count, secs) in sorted(timer.durations().items(), key=lambda kv: -kv[1][1]):
        if layout == "tn-grouped":  # m = ((M, N, K), ...) of one grouped weight-gradient launch
            flops = sum(2.0 * mm * nn * kk for mm, nn, kk in m) * count
            row = dict(layout=layout, problems=len(m), tiles=sum(((mm + 255) // 256) * ((nn + 255) // 256) for mm, nn, _ in m),
                       K=m[0][2])
        else:
            flops = 2.0 * m * n * k * count
            row = dict(layout=layout, M=m, N=n, K=k, epilogue=epi)
        tot_t += secs
        tot_f += flops
        row.update(launches_per_step=round(count / steps, 2), us=round(secs / count * 1e6, 1), tflops=round(flops / secs / 1e12, 1),
                   ms_per_step=round(secs / steps * 1e3, 3))
        rows.append(row)
    return tot_f / steps, tot_t / steps, rows


def _kernel_of(row: dict) -> str:
    """the kernel instantiation behind an in-step timing row, as rocprofv3 names it (asked from the library: cfhip_gemm_kernel_name)"""
    import ctypes

    from cflearn_amd import _lib, fused, ops

    if row["layout"] == "tn-grouped":
        return (f"gemm_grouped_tn_kernel<Cfg<256, 256, 2, 4, 5, 32>, 3, true> ({row.get('problems')} weight gradients, {row.get('tiles')} "
                f"tiles per launch: DW_GROUP_BLOCKS {fused.DW_GROUP_BLOCKS}, DW_GROUP_TILES {fused.DW_GROUP_TILES})")
    epi = {"none": ops.EPI_NONE, "bias": ops.EPI_NONE, "gelu": ops.EPI_GELU, "residual": ops.EPI_RESIDUAL, "dgelu": ops.EPI_DGELU,
           "qgelu": ops.EPI_QGELU, "dqgelu": ops.EPI_DQGELU}.get(str(row.get("epilogue")), row.get("epilogue"))
    epi = epi if isinstance(epi, int) else 0
    buf = ctypes.create_string_buffer(128)
    lay = row["layout"]
    rc = _lib.load().cfhip_gemm_kernel_name(int(row["M"]), int(row["N"]), int(row["K"]), int(lay == "tn"), int(lay in ("nn", "tn")), epi, buf, 128)
    return buf.value.decode() if rc == 0 else f"gemm_bf16_kernel {lay}"


def _dominant(rows: list) -> dict:
    """The dominant kernel of the step, both ways of counting.  `by_kernel`: in-step timings summed per kernel INSTANTIATION —
    the first row of a `rocprofv3 --kernel-trace --stats` summary of the same command (several launch shapes share one
    instantiation: the three N = 768 dX GEMMs are one kernel).  `by_launch_shape`: the single launch shape with the most
    kernel time per step.  Fractions are in-step rates over the dense bf16 peak: three queues overlap, so every kernel that
    shares the chip reads lower here than alone."""
    if not rows:
        return {}
    groups: dict = {}
    for r in rows:
        g = groups.setdefault(_kernel_of(r), dict(ms_per_step=0.0, launches_per_step=0.0, flops_ms=0.0, shapes=[]))
        g["ms_per_step"] += r["ms_per_step"]
        g["launches_per_step"] += r["launches_per_step"]
        g["flops_ms"] += r["tflops"] * r["ms_per_step"]  # TFLOP/s x ms = GFLOP
        g["shapes"].append(f"{r.get('M', '')}x{r.get('N', '')}x{r.get('K', '')}" if r["layout"] != "tn-grouped" else f"K={r.get('K')}")
    name, g = max(groups.items(), key=lambda kv: kv[1]["ms_per_step"])
    tf = g["flops_ms"] / g["ms_per_step"]
    by_kernel = {"kernel": name, "launches_per_step": round(g["launches_per_step"], 2), "ms_per_step": round(g["ms_per_step"], 3),
                 "avg_us": round(g["ms_per_step"] / g["launches_per_step"] * 1e3, 1), "shapes": g["shapes"],
                 "achieved": round(tf, 1), "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4)}
    top = max(rows, key=lambda r: r.get("ms_per_step", 0.0))
    by_shape = {"kernel": _kernel_of(top), "launches_per_step": top["launches_per_step"], "avg_us": top["us"], "ms_per_step": top["ms_per_step"],
                "achieved": top["tflops"], "unit": "TFLOP/s", "frac": round(top["tflops"] / PEAK_BF16_TFLOPS, 4)}
    return {"by_kernel": by_kernel, "by_launch_shape": by_shape}


def _cpu_step_port(batch: int):
    """One step of the oracle restatement (oracle/vit_oracle.py): returns a closure and the kind string."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vit_oracle as O

    import cflearn_amd as C

    torch.manual_seed(0)
    model = C.vit_b16_classifier(1000)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    del model
    g = torch.Generator().manual_seed(1234)
    img = torch.randn(batch, 3, 224, 224, generator=g)
    labels = torch.randint(0, 1000, (batch, 1), generator=g)
    m = {k: torch.zeros_like(v) for k, v in sd.items()}
    v2 = {k: torch.zeros_like(v) for k, v in sd.items()}

    def one(step: int) -> None:
        _, _, grads = O.loss_and_grads(img, labels, sd, 12, 12)
        for k in sd:
            O.adamw_step(sd[k], grads[k], m[k], v2[k], step, 1e-4, weight_decay=0.0)

    return one, "port"


def _cpu_step_reference(batch: int):
    """One step of the REFERENCE'S OWN modules (ViTEncoder + Linear head from /root/reference through
    oracle/refharness), torch AdamW; raises when the tree is absent."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import warnings

    import refharness

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = refharness.load_reference()
    torch.manual_seed(0)
    enc = ref.ViTEncoder(img_size=224, patch_size=16, in_channels=3, latent_dim=768)
    head = ref.Linear(768, 1000)
    params = list(enc.parameters()) + list(head.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.0)
    g = torch.Generator().manual_seed(1234)
    img = torch.randn(batch, 3, 224, 224, generator=g)
    labels = torch.randint(0, 1000, (batch,), generator=g)

    def one(step: int) -> None:
        opt.zero_grad()
        # (the reference's `cv_clf` wrapper calls a method its ViTEncoder lacks — SURVEY F6 — so the encoder and the
        # head are driven directly, as the survey's probe did)
        logits = head(enc(img))
        torch.nn.functional.cross_entropy(logits, labels).backward()
        opt.step()

    return one, "reference"


def _cpu_child(mode: str, batch: int, steps: int, threads: int) -> None:
    """Runs in a child process (so that a slow host cannot stall the benchmark: the parent enforces a wall-clock
    limit): times `steps` steps and prints one JSON line."""
    torch.set_num_threads(threads)
    try:
        one, kind = _cpu_step_reference(batch)
    except Exception:  # /root/reference is absent (GPU box): the restatement
        one, kind = _cpu_step_port(batch)

    def run(n: int) -> float:
        one(1)
        t0 = time.perf_counter()
        for s_ in range(n):
            one(s_ + 2)
        return (time.perf_counter() - t0) / n

    if mode == "bf16":
        with torch.autocast("cpu", dtype=torch.bfloat16):
            dt = run(steps)
    else:
        dt = run(steps)
    print(json.dumps(dict(kind=kind, ms_per_step=dt * 1e3, value=batch / dt)))


def cpu_baseline(batch: int, steps: int, limit_s: float = 45.0):
    """The reference's PyTorch-CPU step on the host cores, bounded in WORK (batch x steps) and in WALL time (each
    variant runs in a child process with a time limit): fp32 and bf16-autocast, all host cores."""
    import subprocess

    logical = os.cpu_count() or 1
    # One thread per PHYSICAL core, at most 64: measured on the 2 x 64-core (256 logical CPUs) host of the GPU box,
    # 256 threads did not finish 8 batch-4 steps in 75 s where 64 threads take 1.4 s / step (round 1) — the
    # batch-4 GEMMs do not have 256-way parallelism, the surplus is OpenMP barrier time.
    cores = max(1, min(64, logical // 2 if logical >= 16 else logical))

    def child(mode: str, n: int):
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-child", mode, "--cpu-batch", str(batch),
               "--cpu-steps", str(n), "--cpu-threads", str(cores)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
            line = [ln for ln in res.stdout.strip().split("\n") if ln.startswith("{")]
            return json.loads(line[-1]) if line else dict(note=f"child failed: {res.stderr.strip()[-200:]}")
        except subprocess.TimeoutExpired:
            return dict(note=f"did not finish {n} steps within {limit_s:.0f} s")

    fp32 = child("fp32", steps)
    out = dict(value=None if "value" not in fp32 else round(fp32["value"], 3), unit="samples/s", cores=cores,
               host_logical_cpus=logical, kind=fp32.get("kind", "port"),
               sample=f"{steps} timed steps (+1 warm-up) of fwd+CE+bwd+AdamW, fp32, batch {batch}, torch CPU with "
                      f"{cores} threads, ViT-B/16 224^2 (child process, {limit_s:.0f} s limit)",
               ms_per_step=None if "ms_per_step" not in fp32 else round(fp32["ms_per_step"], 1))
    if "note" in fp32:
        out["note"] = fp32["note"]
    b16 = child("bf16", max(2, steps // 2))
    out["bf16_autocast"] = ({"value": round(b16["value"], 3), "ms_per_step": round(b16["ms_per_step"], 1)}
                            if "value" in b16 else {"value": None, "note": b16.get("note")})
    return out


def bench_other_workload(args) -> None:
    """`--workload unet | clip`: one JSON line for BASELINE config 3 / 4 on ONE GPU."""
    print(json.dumps(run_other_workload(args)))


def build_other_workload(args):
    """model + step engine + synthetic batch of `--workload unet | clip`: (step closure, model, name, batch, loss divisor)"""
    import cflearn_amd as C

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1234)
    if args.workload == "unet":
        from cflearn_amd.diffusion import DDPMTrainStep, NoiseSchedule

        batch = args.batch if args.batch != 128 else (8 if args.img <= 64 else 1)
        cfg = dict(in_channels=3, out_channels=3, start_channels=320, num_heads=8, use_spatial_transformer=True,
                   num_transformer_layers=1, num_res_blocks=2, attention_downsample_rates=(1, 2, 4),
                   channel_multipliers=(1, 2, 4, 4), context_dim=None)
        m = C.build_module("unet_diffuser", config=cfg).to(dev)
        ts = DDPMTrainStep(m, NoiseSchedule(device=dev), lr=1.0e-4, use_graph=bool(getattr(args, "graph", False)),
                           step_in_backward=not getattr(args, "no_step_in_backward", False))
        x = torch.randn(batch, 3, args.img, args.img, generator=g).clamp_(-1, 1).to(dev)
        t = torch.randint(0, 1000, (batch,), generator=g).to(dev)
        eps = torch.randn(x.shape, generator=g).to(dev)
        step = lambda: ts.step(x, None, timesteps=t, noise=eps)  # noqa: E731
        name = (f"DDPM UNet (zoo diffusion/ddpm: start 320, multipliers 1/2/4/4, SpatialTransformer at rates 1/2/4) "
                f"{args.img}^2, q_sample + fwd + MSE + bwd + fused AdamW")
        loss_div = batch
    else:
        from cflearn_amd.engine import LossTrainStep

        batch = args.batch if args.batch != 128 else 256
        m = C.build_module("clip", config={}).to(dev)
        ts = LossTrainStep(m, lambda mod, b_: mod.contrastive_loss(b_["image"], b_["text"]), lr=1.0e-4,
                           step_in_backward=not getattr(args, "no_step_in_backward", False))
        img = torch.randn(batch, 3, 224, 224, generator=g)
        txt = torch.randint(1, 49407, (batch, 77), generator=g)
        eot = torch.randint(8, 77, (batch,), generator=g)
        for i in range(batch):
            txt[i, eot[i]] = 49407
            txt[i, eot[i] + 1:] = 0
        data = dict(image=img.to(dev), text=txt.to(dev))
        step = lambda: ts.step(data)  # noqa: E731
        name = "CLIP (ViT-B/32 + 12 x 512 causal text tower) symmetric InfoNCE step, fwd + bwd + fused AdamW"
        loss_div = 1
    step.engine = ts  # (run_other_workload reports how many optimizer ranges were updated inside backward)
    return step, m, name, batch, loss_div


def run_other_workload(args) -> dict:
    """BASELINE configs 3 / 4 on ONE GPU (the multi-GPU path of these models is the same `BucketedAllReduce`; their
    default batch follows SURVEY §8d).  A dict with the keys of the headline line; `roofline` is the MFMA roofline of the
    whole step: counted MFMA-class FLOPs (ops.FlopCounter: GEMMs, implicit convolutions, attention) / wall time."""
    from cflearn_amd import ops

    step, m, name, batch, loss_div = build_other_workload(args)
    n_params = sum(p.numel() for p in m.parameters())
    first = None
    for i in range(args.warmup):
        loss = step()
        if i == 0:
            first = loss.item() / loss_div
            note(f"first step done, loss {first:.4f}")
    torch.cuda.synchronize()
    import gc

    gc.collect()
    gc.freeze()  # model, arena and warm-up survivors leave the collector's generations: its passes inside the timed steps stay short
    start_telemetry(torch.cuda.current_device())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    host_dt = (time.perf_counter() - t0) / args.steps  # the host's share: all launches of a step issued (no device wait inside)
    torch.cuda.synchronize()
    t_end = time.perf_counter()
    dt = (t_end - t0) / args.steps
    tel = telemetry_summary(t0, t_end)
    note(f"{args.workload}: {dt * 1e3:.3f} ms/step, host issue time {host_dt * 1e3:.3f} ms/step")
    if getattr(args, "dump_outputs", None):  # before the FLOP-counting step below
        dump_outputs(args.dump_outputs, loss, m)
    inb = getattr(step.engine.optimizer, "in_backward", None)
    in_bwd = None if inb is None else {"ranges": len(inb.ranges), "updated_inside_backward_last_step": int(inb.launched_in_backward)}
    full = getattr(args, "full", False)
    if full:  # one more step with the FLOP counter (a plain run stops at the timed steps)
        counter = ops.FlopCounter()
        ops.FLOP_COUNTER = counter
        try:
            step()
            torch.cuda.synchronize()
        finally:
            ops.FLOP_COUNTER = None
        tf = counter.total() / dt / 1e12
    gc.unfreeze()
    roofline = None
    if full:
        gemm_rows = None
        if getattr(args, "gemm_table", False):  # in-step event pairs around every GEMM launch, by shape
            class _Step:
                step = staticmethod(lambda: step())
            f_step, t_step, rows = time_gemms_in_step(_Step, lambda: (), 2)
            gemm_rows = {"flops_per_step": f_step, "kernel_ms_per_step": round(t_step * 1e3, 3), "rows": rows[:40]}
        roofline = {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": None,
                    "frac_at_sustained_clock": _frac_at_clock(tf, tel),
                    "definition": "algorithmic MFMA-class FLOPs of one step (ops.FlopCounter) / measured wall time of the step",
                    "flops_per_step": {k: v for k, v in counter.flops.items()}, "gemm_table": gemm_rows}
    return {
        "metric": f"train samples/sec + step ms, {args.workload}", "value": round(batch / dt, 3), "unit": "samples/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "host_issue_ms_per_step": round(host_dt * 1e3, 3),
        "telemetry": tel,
        "optimizer_in_backward": in_bwd,
        "config": {"workload": name, "per_gpu_batch": batch, "parameters": n_params,
                   "loss_first_step": None if first is None else round(first, 5),
                   "loss_last_step": round(loss.item() / loss_div, 5)},
        "roofline": roofline,
        "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2),
    }


NOMINAL_SCLK_MHZ = 2400.0  # the shader clock PEAK_BF16_TFLOPS is quoted at (MI355X_MICROARCH.md)


def _frac_at_clock(tflops: float, tel: dict):
    """fraction of the MFMA peak AT THE CLOCK THE CHIP SUSTAINED in the window: peak x sclk / 2400 MHz (null without a clock sample)"""
    sclk = (tel or {}).get("sclk_mhz_avg")
    if not sclk:
        return None
    return round(tflops / (PEAK_BF16_TFLOPS * sclk / NOMINAL_SCLK_MHZ), 4)


def _pct(sorted_vals: list, q: float) -> float:
    """q-quantile of an ascending list (linear interpolation)"""
    if not sorted_vals:
        return float("nan")
    pos = q * (len(sorted_vals) - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(sorted_vals) - 1)
    return sorted_vals[lo] + (sorted_vals[hi] - sorted_vals[lo]) * (pos - lo)


def launch_command(n: int, argv: list, port: int) -> list:
    """The command line of `python -m torch.distributed.run` that starts `n` ranks of this script on this node."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n: int, argv: list) -> int:
    """Re-execute this script as `n` ranks under torch.distributed.run (one per GPU; with `--backend gloo --all-on-gpu0`
    the ranks share cuda:0 — the dry run of the N > 1 path on a 1-GPU box).  Returns the launcher's exit code."""
    import subprocess

    visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if "--all-on-gpu0" not in argv and visible < n:
        print(f"[bench] --gpus {n} needs {n} visible GPUs, this node shows {visible} (dry run of the distributed path on one "
              "GPU: add --backend gloo --all-on-gpu0)", file=sys.stderr)
        return 2
    env = dict(os.environ, CFHIP_BENCH_LAUNCHER="self", MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL peer buffers)
    for i, a in enumerate(argv):  # --nchannels N: RCCL reads the variable when the communicator is created
        if a == "--nchannels" and i + 1 < len(argv) and int(argv[i + 1]) > 0:
            env["NCCL_MAX_NCHANNELS"] = argv[i + 1]
        elif a.startswith("--nchannels=") and int(a.split("=", 1)[1]) > 0:
            env["NCCL_MAX_NCHANNELS"] = a.split("=", 1)[1]
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = launch_command(n, argv, free_port())
    print(f"[bench] starting {n} ranks: {' '.join(cmd[1:10])} ...", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def sweep_launch(n: int, argv: list) -> int:
    """`python bench.py --gpus N --sweep` from a plain shell: one set of ranks per NCCL_MAX_NCHANNELS candidate (0 = RCCL's own
    choice), each sweeping bucket size x wire dtype in-process; the best line (by `value`) is printed with every table attached."""
    import subprocess

    visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if "--all-on-gpu0" not in argv and visible < n:
        print(f"[bench] --gpus {n} needs {n} visible GPUs, this node shows {visible}", file=sys.stderr)
        return 2
    best, tables, rc_last = None, {}, 0
    for nch in (0, 8, 16):
        env = dict(os.environ, CFHIP_BENCH_LAUNCHER="self", MASTER_ADDR="127.0.0.1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        env.pop("NCCL_MAX_NCHANNELS", None)
        extra = []
        if nch > 0:
            env["NCCL_MAX_NCHANNELS"] = str(nch)
            extra = ["--nchannels", str(nch)]
        cmd = launch_command(n, list(argv) + extra + ["--no-cpu-baseline", "--no-roofline"], free_port())
        print(f"[bench] sweep: {n} ranks with NCCL_MAX_NCHANNELS={nch or 'default'} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        rc_last = r.returncode
        line = None
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                try:
                    line = json.loads(ln)
                except ValueError:
                    pass
        if r.returncode != 0 or line is None:
            tables[str(nch)] = {"error": f"exit code {r.returncode}"}
            continue
        tables[str(nch)] = {"value": line["value"], "ms_per_step": line["ms_per_step"], "bucket_mb": line.get("rccl", {}).get("bucket_mb"),
                            "sweep": line.get("rccl", {}).get("sweep")}
        if best is None or line["value"] > best["value"]:
            best = line
    if best is None:
        print("[bench] sweep: no candidate produced a line", file=sys.stderr)
        return rc_last or 1
    best.setdefault("rccl", {})["nchannels_sweep"] = tables
    print(json.dumps(best))
    return 0


def time_exchange_settings(ts, next_batch, sync, dev, distributed: bool, bucket_mbs, wires, steps: int) -> list:
    """Time the live job with the reducer re-cut / re-wired between passes: [{bucket_mb, wire, buckets, ms_per_step}] (max over
    ranks).  Two untimed steps per setting first (launch plans re-record nothing: the notifications are replayed live)."""
    rows = []
    for wire in wires:
        for mb in bucket_mbs:
            ts.reducer.set_wire_bf16(wire)
            nbk = ts.reducer.rebucket(mb << 20)
            for _ in range(2):
                ts.step(*next_batch())
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                ts.step(*next_batch())
            sync()
            dt = time.perf_counter() - t0
            if distributed:
                tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                dt = tmax.item()
            rows.append({"bucket_mb": mb, "wire": "bf16" if wire else "fp32", "buckets": nbk, "ms_per_step": round(dt / steps * 1e3, 3)})
    return rows


_T0 = time.perf_counter()


def note(msg: str) -> None:
    """progress line on stderr (stdout carries only the JSON result)"""
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


DUMP_BUDGET_BYTES = 32 << 20  # the parameter samples of --dump-outputs (the cap on the whole directory is 64 MB)


def dump_outputs(out_dir: str, loss: torch.Tensor, model: torch.nn.Module) -> None:
    """--dump-outputs: what the timed path handed its caller after the LAST timed step, as float32 .npy files —
    `loss.npy` (the tensor `step()` returned) and `param.<name>.npy` for every parameter the step updated: the whole
    tensor when it is small, otherwise a fixed sample (torch.Generator seeded 0, indices drawn in `named_parameters`
    order), so two builds run with the same arguments can be compared file by file."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().float().cpu().numpy())
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    per = max(256, DUMP_BUDGET_BYTES // 4 // max(1, len(params)))
    g = torch.Generator().manual_seed(0)
    total = 0
    for name, p in params:
        flat = p.detach().reshape(-1)
        if flat.numel() > per:
            idx = torch.randint(0, flat.numel(), (per,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        arr = flat.float().cpu().numpy()
        np.save(os.path.join(out_dir, f"param.{name}.npy"), arr)
        total += arr.nbytes
    note(f"dumped loss + {len(params)} parameter tensors ({total / 2**20:.1f} MB) to {out_dir}")


TELEMETRY = None  # tools.gpu_telemetry.GpuTelemetry of this rank's GPU (started in main / bench_other_workload)


def start_telemetry(device_index: int):
    """sclk / socket power / junction temperature of this rank's GPU at 25 Hz from a side thread (tools/gpu_telemetry.py: amdsmi
    in-process, rocm-smi as fallback).  A line without clock and power cannot be compared with a line from another box: the step
    runs against the socket's power cap and boxes differ by +-3 % in the clock they sustain."""
    global TELEMETRY
    if TELEMETRY is None:
        try:
            from tools.gpu_telemetry import GpuTelemetry

            TELEMETRY = GpuTelemetry(device_index, hz=25.0).start()
            if not TELEMETRY.available:
                note(f"telemetry: no source ({TELEMETRY.error})")
        except Exception as e:  # never fatal
            note(f"telemetry unavailable: {type(e).__name__}: {e}")
            TELEMETRY = None
    return TELEMETRY


def telemetry_summary(t0: float, t1: float) -> dict:
    if TELEMETRY is None or not TELEMETRY.available:
        return {"sclk_mhz_avg": None, "power_w_avg": None, "power_cap_w": None, "samples": 0,
                "source": None if TELEMETRY is None else TELEMETRY.error}
    return TELEMETRY.summary(t0, t1)


def calibration_launch(min_seconds: float = 0.25) -> dict:
    """ONE fixed launch, the same on every box and in every round, timed right AFTER the timed region (the chip is hot and at the
    clock it sustains): the grouped weight-gradient kernel of two ViT-B/16 blocks at batch 128 (8 problems, K = 25 216, 216 tiles of
    256 x 256, 1.43 TFLOP per launch) on seeded random operands, back to back for >= `min_seconds`.  Its TFLOP/s is this box's
    yardstick: `ms_per_step x calibration rate` compares steps across boxes."""
    from cflearn_amd import ops

    dev = torch.device("cuda", torch.cuda.current_device())
    k = 128 * 197
    g = torch.Generator(device=dev).manual_seed(20260930)
    rnd = lambda r, c: (torch.randn(r, c, generator=g, device=dev) * 0.5).to(torch.bfloat16)  # noqa: E731
    shapes = ((768, 3072), (3072, 768), (768, 768), (2304, 768))
    probs = [(rnd(k, m), rnd(k, n), torch.empty(m, n, dtype=torch.float32, device=dev), False,
              torch.empty(m, dtype=torch.float32, device=dev), False) for _ in range(2) for m, n in shapes]
    flops = 2.0 * sum(2.0 * m * n * k for m, n in shapes)
    for _ in range(3):
        ops.gemm_grouped_tn(probs)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launches, t0 = 0, time.perf_counter()
    e0.record()
    while True:
        for _ in range(40):
            ops.gemm_grouped_tn(probs)
        launches += 40
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= min_seconds:
            break
    e1.record()
    e1.synchronize()
    t1 = time.perf_counter()
    us = e0.elapsed_time(e1) * 1e3 / launches
    tel = telemetry_summary(t0, t1)
    return {"kernel": "gemm_grouped_tn_kernel<Cfg<256,256,2,4,5,32>>: the weight gradients of two ViT-B/16 blocks at batch 128 "
                      "(8 problems, K = 25 216, 216 tiles), seeded random bf16 operands",
            "launches": launches, "us_per_launch": round(us, 2), "tflops": round(flops / us / 1e6, 1),
            "frac_of_peak": round(flops / us / 1e6 / PEAK_BF16_TFLOPS, 4), "sclk_mhz_avg": tel.get("sclk_mhz_avg"),
            "power_w_avg": tel.get("power_w_avg"), "when": "right after the timed region"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="per-GPU batch (weak scaling; SURVEY §8a: 64 or 128)")
    ap.add_argument("--set-option", action="append", default=[], metavar="NAME=VALUE",
                    help="cfhip_set_option before anything runs (A/B runs: e.g. gemm_heuristic=9); recorded in config.options")
    ap.add_argument("--batches", type=int, default=8, help="HBM-resident synthetic batches the steps rotate through (1: one fixed batch, which the model memorises)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step from a captured hipGraph (single GPU).  Default is eager multi-stream "
                         "launches: with the parameter-gradient kernels on side streams the eager step measured "
                         "faster than the graph replay (profiles/r01)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement behind the timed steps: calibration launch, roofline, other workloads, CPU "
                         "baseline (a plain run: set-up, warm-up, timed steps, --dump-outputs, the line)")
    ap.add_argument("--gemm-table", action="store_true", help="--full --workload unet | clip: add the in-step per-shape GEMM table")
    ap.add_argument("--no-graph", action="store_true", help="(default now) kept for compatibility")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the ViT roofline steps")
    ap.add_argument("--no-calibration", action="store_true", help="--full: skip the fixed calibration launch behind the timed region")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="--full: skip the bounded UNet 64^2 x 8 / CLIP b256 runs (BASELINE configs 3 / 4) appended to an N = 1 line")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--workload", default="vit", choices=["vit", "unet", "clip"],
                    help="vit (default: the headline metric, BASELINE configs[1/2]); unet / clip: configs 3 / 4 on one GPU")
    ap.add_argument("--img", type=int, default=64, help="--workload unet: image side (64 or 256)")
    ap.add_argument("--cpu-steps", type=int, default=6)
    ap.add_argument("--cpu-child", default=None, help="(internal) run the CPU baseline in this process: fp32 | bf16")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--gemm-reps", type=int, default=10)
    ap.add_argument("--bucket-mb", type=int, default=64, help="gradient bucket size of the RCCL exchange (sweep on an 8-GPU node)")
    ap.add_argument("--wire-bf16", action="store_true", help="all-reduce bf16 copies of the gradient buckets (half the xGMI bytes)")
    ap.add_argument("--nchannels", type=int, default=0,
                    help="NCCL_MAX_NCHANNELS for the ranks (RCCL's kernels take one workgroup per channel: fewer channels leave more "
                         "CUs to a step whose kernels already share the chip; 0 = RCCL's default).  Sweep on an 8-GPU node.")
    ap.add_argument("--sweep", action="store_true",
                    help="N > 1: tune the gradient exchange inside ONE launch — --bucket-mb {32,64,128} x --wire-bf16 {0,1} on the live "
                         "job (the reducer is re-cut between passes; 10 steps each), and, when bench.py starts its own ranks, once per "
                         "--nchannels {0,8,16} (RCCL reads NCCL_MAX_NCHANNELS when the communicator is created: a new set of ranks "
                         "each).  Prints the best line (timed on the best fp32-wire setting) with the table in `rccl.sweep`")
    ap.add_argument("--tune-buckets", default="auto", choices=["auto", "on", "off"],
                    help="before the warm-up of an N > 1 run, time --bucket-mb {32,64,128} for a few steps each on the live job and "
                         "keep the fastest (auto: on for N > 1 unless --bucket-mb was given); the table goes to `rccl.bucket_sweep`")
    ap.add_argument("--sweep-steps", type=int, default=10)
    ap.add_argument("--strict-streams", action="store_true",
                    help="exit with code 3 (after printing the line) when a helper stream had to share a hardware queue on any rank; "
                         "by default the line carries `streams.distinct_on_every_rank: false` and a `warnings` entry instead")
    ap.add_argument("--allow-aliased-streams", action="store_true", help=argparse.SUPPRESS)  # (round-4 spelling of the default)
    ap.add_argument("--no-step-in-backward", action="store_true",
                    help="A/B: one fused Adam(W) launch at the end of the step instead of range updates inside backward")
    ap.add_argument("--range-mb", type=int, default=32, help="arena range of one in-backward optimizer update")
    ap.add_argument("--comm", default="auto", choices=["auto", "torch", "cfhip"],
                    help="who launches the RCCL collectives: the cfhip_comm_* C-ABI on this package's own, queue-checked "
                         "comm stream (auto with the nccl backend: measured 22.4 ms vs 23.0 ms for the torch.distributed "
                         "launch at 1 rank, 22.3 ms without any exchange — profiles/r02/rccl_1rank_comm_*.json), or "
                         "torch.distributed (auto with gloo; fallback when the communicator cannot be created)")
    ap.add_argument("--profile-steps", type=int, default=6, help="extra (untimed) steps with event pairs around every GEMM launch (an event pair spans the launch from the moment its stream is ready for it: it includes the wait for free CUs, which a profiler's kernel duration does not)")
    ap.add_argument("--watchdog", type=int, default=0, help="dump all Python stacks every N seconds")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl == RCCL; gloo for the "
                                                      "single-GPU dry run of the N > 1 code path)")
    ap.add_argument("--all-on-gpu0", action="store_true", help="dry run: every rank uses cuda:0")
    ap.add_argument("--force-ddp", action="store_true",
                    help="dry run: take the distributed code path (process group, bucketed all-reduce, barrier) even "
                         "with WORLD_SIZE=1 -- exercises the RCCL calls on a 1-GPU box")
    ap.add_argument("--input", default="device", choices=["device", "host"],
                    help="device (default, the headline number): the batch is resident in HBM.  host: every step "
                         "pulls a fresh host batch through cflearn_amd.data.TensorBatcher (copy stream, one batch "
                         "ahead) — the PCIe-inclusive rate, reported in DESIGN.md only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the loss and (samples of) the parameters of the last timed step "
                         "as DIR/<name>.npy (float32, < 64 MB; rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gemm_table and not args.full:
        ap.error("--gemm-table is part of the roofline: add --full")
    if args.cpu_child is not None:
        _cpu_child(args.cpu_child, args.cpu_batch, args.cpu_steps, args.cpu_threads or (os.cpu_count() or 1))
        return
    if args.set_option:
        from cflearn_amd import ops as _ops

        for item in args.set_option:
            name, _, val = item.partition("=")
            _ops.set_option(name, int(val))
    if args.workload != "vit":
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
        bench_other_workload(args)
        return
    if args.watchdog > 0:
        import faulthandler

        faulthandler.dump_traceback_later(args.watchdog, repeat=True, file=sys.stderr)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` from a plain shell: start the N ranks ourselves (the reference launches its own ranks
        # too: api/api.py:269-293 run_accelerate -> `accelerate launch`); rank 0's JSON line passes through
        if args.sweep and args.nchannels == 0:
            raise SystemExit(sweep_launch(args.gpus, sys.argv[1:]))
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    # The result line must be the ONLY thing on stdout (the driver reads it from there): RCCL prints a version banner to the C-level
    # stdout of every rank when its first communicator is created (seen in the 1-rank RCCL runs: it lands AFTER the JSON line because C
    # stdio flushes at exit).  So file descriptor 1 is pointed at stderr for the whole run — Python's and every library's stdout text
    # goes there — and rank 0 writes the JSON line to the saved descriptor at the very end.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if "--all-on-gpu0" in sys.argv else int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    start_telemetry(local_rank)  # every rank samples its own GPU (RCCL's kernels draw from the same power cap: VERDICT r5 #8)
    distributed = world > 1 or args.force_ddp
    if args.nchannels > 0:  # (also when an external launcher started the ranks; RCCL reads it at communicator creation)
        os.environ["NCCL_MAX_NCHANNELS"] = str(args.nchannels)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # "nccl" == RCCL on ROCm
        else:
            dist.init_process_group(args.backend)
    if args.gpus != world and not args.force_ddp:
        raise SystemExit(f"bench.py --gpus {args.gpus} was started by an external launcher with WORLD_SIZE={world}: the "
                         "two must agree (plain `python bench.py --gpus N` starts its own N ranks)")
    if distributed:
        assert dist.get_world_size() == world

    import cflearn_amd as C
    from cflearn_amd.engine import TrainStep

    if args.comm == "auto":
        args.comm = "cfhip" if (distributed and args.backend == "nccl" and not args.all_on_gpu0) else "torch"
    torch.manual_seed(0)  # identical init on every rank (and rank 0 is broadcast anyway)
    model = C.vit_b16_classifier(1000).to(dev)
    def make_step(comm: str):
        return TrainStep(model, lr=1.0e-4, weight_decay=0.0, decoupled=True, use_graph=args.graph and not args.no_graph,
                         distributed=distributed, bucket_bytes=args.bucket_mb << 20, wire_bf16=args.wire_bf16, comm=comm,
                         step_in_backward=not args.no_step_in_backward, range_bytes=args.range_mb << 20)

    comm_selftest = None
    if args.comm == "cfhip":
        # The C-ABI communicator has only ever run with one rank on the builder's 1-GPU boxes: check it before trusting it.
        # (1) a watchdog ends the process loudly if its creation / first collective does not come back (a hang here must
        # not look like a slow benchmark); (2) one all-reduce of known values; (3) the ranks agree — through the torch
        # process group — whether everybody passed, otherwise ALL of them let torch.distributed launch the collectives.
        import threading

        def _stuck() -> None:
            print(f"[bench] rank {rank}: the cfhip communicator did not answer within 180 s (creation or first all-reduce); "
                  "rerun with --comm torch", file=sys.stderr, flush=True)
            os._exit(17)

        dog = threading.Timer(180.0, _stuck)
        dog.daemon = True
        dog.start()
        ok, why = 1, ""
        try:
            ts = make_step("cfhip")
            if ts.reducer is not None and ts.reducer.comm is not None:
                probe = torch.full((1024,), float(rank + 1), device=dev)
                ts.reducer.comm_stream.wait_stream(torch.cuda.current_stream())
                ts.reducer.comm.all_reduce_(probe, ts.reducer.comm_stream)
                torch.cuda.current_stream().wait_stream(ts.reducer.comm_stream)
                torch.cuda.synchronize()
                want = world * (world + 1) / 2.0
                if not bool((probe == want).all()):
                    ok, why = 0, f"all-reduce self-test gave {probe[0].item()} instead of {want}"
        except RuntimeError as e:  # the RCCL communicator could not be created
            ok, why = 0, str(e)
        dog.cancel()
        comm_selftest = "all-reduce of (rank + 1) over the cfhip communicator == W (W + 1) / 2: ok" if ok else f"failed: {why}"
        if distributed:
            flag = torch.tensor([ok], device=dev, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            everybody = int(flag.item())
        else:
            everybody = ok
        if not everybody:
            print(f"[bench] rank {rank}: cfhip communicator not usable ({why or 'another rank failed'}); "
                  "all ranks fall back to --comm torch", file=sys.stderr)
            args.comm = "torch"
            torch.manual_seed(0)
            model = C.vit_b16_classifier(1000).to(dev)  # a fresh model: the first arena / reducer hooks stay with the old one
            ts = make_step("torch")
    else:
        ts = make_step(args.comm)
    if ts.reducer is not None:
        ts.reducer.time_exposed = True
    g = torch.Generator().manual_seed(1234 + rank)
    # A RING of HBM-resident batches with fresh labels (round 5): one fixed batch is memorised within the
    # warm-up (loss 7.1 -> 0.006), after which the backward GEMMs see the gradients of a collapsed loss; the MFMA rate of this
    # chip depends on operand values (profiles/r04/hipblaslt_and_zero_operand_probe.log), so the timed steps must see
    # full-entropy activations and gradients.  `--batches 1` is the old behaviour (A/B in profiles/r05/).
    nb = max(1, args.batches)
    ring = [(torch.randn(args.batch, 3, 224, 224, generator=g).to(dev), torch.randint(0, 1000, (args.batch,), generator=g).to(dev))
            for _ in range(nb)]
    img, labels = ring[0]
    ring_pos = [0]

    def sync() -> None:
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    feed = None
    if args.input == "host":
        import itertools

        from cflearn_amd.data import TensorBatcher

        host = [dict(input=torch.randn(args.batch, 3, 224, 224, generator=g).numpy(),
                     labels=torch.randint(0, 1000, (args.batch,), generator=g).numpy()) for _ in range(4)]

        class _Endless:
            def __len__(self):
                return 1 << 30

            def __iter__(self):
                return itertools.cycle(host)

        feed = iter(TensorBatcher(_Endless(), dev, depth=1))

    def next_batch():
        if feed is None:
            ring_pos[0] += 1
            return ring[ring_pos[0] % nb]
        b = next(feed)
        return b["input"], b["labels"]

    note(f"model + arena ready on {dev}, launch={'graph' if ts.use_graph else 'eager'}, input={args.input}")
    # ---- the exchange settings of a multi-GPU run, tuned on the live job BEFORE the warm-up (untimed; the timed region below is
    # still exactly --steps steps on ONE setting).  Every rank takes the same decisions: the timings are all-reduced (MAX).
    sweep_rows, first_loss = None, None
    bucket_given = any(a == "--bucket-mb" or a.startswith("--bucket-mb=") for a in sys.argv[1:])
    tune = ts.reducer is not None and not ts.use_graph and (
        args.sweep or args.tune_buckets == "on" or (args.tune_buckets == "auto" and world > 1 and not bucket_given))
    if tune:
        try:
            for i in range(3):  # lazy initialisations, launch-plan recording, allocator
                loss = ts.step(*next_batch())
                if i == 0:
                    first_loss = loss.item() / args.batch
            sync()
            wires = (False, True) if (args.sweep and not args.wire_bf16) else (args.wire_bf16,)
            sweep_rows = time_exchange_settings(ts, next_batch, sync, dev, distributed, (32, 64, 128), wires,
                                                max(3, args.sweep_steps if args.sweep else 6))
            same_wire = [r for r in sweep_rows if (r["wire"] == "bf16") == bool(args.wire_bf16)]
            # the fastest bucket size on the wire dtype that was asked for (bf16 on the wire is a numerics trade: reported, never picked);
            # within 0.5 % of the default the default stays
            pick = min(same_wire, key=lambda r: r["ms_per_step"])
            dflt = next((r for r in same_wire if r["bucket_mb"] == args.bucket_mb), None)
            if dflt is not None and dflt["ms_per_step"] <= pick["ms_per_step"] * 1.005:
                pick = dflt
            args.bucket_mb = pick["bucket_mb"]
            note("exchange sweep: " + ", ".join(f"{r['bucket_mb']} MB/{r['wire']} {r['ms_per_step']:.2f} ms" for r in sweep_rows)
                 + f" -> {args.bucket_mb} MB buckets")
        except Exception as e:  # the headline run must survive a failed sweep: back to the defaults
            note(f"exchange sweep failed ({type(e).__name__}: {e}); default settings")
            sweep_rows = [{"error": f"{type(e).__name__}: {e}"[:200]}]
        ts.reducer.set_wire_bf16(args.wire_bf16)
        ts.reducer.rebucket(args.bucket_mb << 20)
    for i in range(args.warmup):
        loss = ts.step(*next_batch())
        if first_loss is None:
            first_loss = loss.item() / args.batch
            note(f"first step done, loss {first_loss:.4f}")
    if ts.reducer is not None:
        ts.reducer.exposed_ms()  # drop the warm-up records
    sync()
    note("warm-up done, timing")
    # per-step durations: one HIP event between steps on the stream the step is issued on (the side streams join it
    # before the optimizer kernel, so consecutive events bracket whole steps) — SURVEY §8d: median, p10, p90
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        loss = ts.step(*next_batch())
        marks[i + 1].record()
    host_dt = time.perf_counter() - t0  # every launch of the timed steps issued (the host never waits for the device inside)
    sync()
    t_end = time.perf_counter()
    dt = t_end - t0
    tel = telemetry_summary(t0, t_end)
    # the fixed calibration launch, on every rank at the same time (the ranks share nothing but the node's power delivery)
    try:
        calib = calibration_launch() if args.full and not args.no_calibration else None
    except Exception as e:  # the headline line must survive
        calib = {"error": f"{type(e).__name__}: {e}"[:200]}
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    if distributed:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = tmax.item()
    last_loss = loss.item() / args.batch
    if args.dump_outputs and rank == 0:  # before the untimed profiling steps below move the weights on
        dump_outputs(args.dump_outputs, loss, model)
    note(f"timed region: {dt / args.steps * 1e3:.3f} ms/step (host issue time {host_dt / args.steps * 1e3:.3f} ms/step)")
    samples_per_s = world * args.batch * args.steps / dt

    result = {
        "metric": "train samples/sec + step ms, ViT-B/16 bf16 DDP at 1/2/4/8 MI355X",
        "value": round(samples_per_s, 2),
        "unit": "samples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "host_issue_ms_per_step": round(host_dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic",
        "config": {
            "workload": "ViT-B/16 224^2 classifier (1000 classes), fwd + softmax-CE + bwd + AdamW, bf16 "
                        "activations / MFMA operands, fp32 master weights, grads and optimizer state",
            "per_gpu_batch": args.batch,
            "global_batch": world * args.batch,
            "seq_len": 197,
            "parallelism": f"dp{world}",
            "launch": "hipGraph replay" if ts.use_graph else "eager",
            "options": list(args.set_option),
            "batches_in_rotation": nb if feed is None else 4,
            "input": f"resident in HBM ({nb} synthetic batches in rotation, each with its own labels)" if feed is None else "host numpy -> TensorBatcher (copy stream, 1 batch ahead, device buffer ring)",
            "grad_exchange": "none" if not distributed else (
                f"bucketed {'RCCL' if args.backend == 'nccl' else args.backend} all-reduce {'bf16 wire' if args.wire_bf16 else 'fp32'}, "
                f"{args.bucket_mb} MB buckets ({len(ts.reducer.buckets)}), comm stream, launched by {args.comm}"),
            "optimizer": ("fused AdamW, arena ranges updated inside backward" + (" behind each bucket's all-reduce" if distributed else "")
                          if (ts.optimizer.in_backward is not None or (ts.reducer is not None and ts.reducer.step_in_backward))
                          else "fused AdamW, one launch at the end of the step"),
            "loss_first_step": None if first_loss is None else round(first_loss, 4),
            "loss_last_step": round(last_loss, 4),
        },
        "mfma_frac_whole_step": round(samples_per_s * FLOP_PER_SAMPLE / world / (PEAK_BF16_TFLOPS * 1e12), 4),
        "mfma_frac_whole_step_at_sustained_clock": _frac_at_clock(samples_per_s * FLOP_PER_SAMPLE / world / 1e12, tel),
        # this rank's GPU over the timed region (10 Hz side thread) and the fixed calibration launch right behind it: what makes
        # this line comparable with a line from another box or round (`ms_per_step x calibration.tflops` is box-independent to
        # first order)
        "telemetry": tel,
        "calibration": calib,
        "step_ms": {"median": round(_pct(per_step, 0.5), 3), "p10": round(_pct(per_step, 0.1), 3),
                    "p90": round(_pct(per_step, 0.9), 3), "min": round(per_step[0], 3), "max": round(per_step[-1], 3),
                    "n": len(per_step), "definition": "HIP events between consecutive steps on the issuing stream (this rank)"},
        "launcher": ("bench.py started its own ranks (torch.distributed.run)" if os.environ.get("CFHIP_BENCH_LAUNCHER") == "self"
                     else "external torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "single process"),
    }
    from cflearn_amd.functional import stream_report

    result["streams"] = stream_report()  # helper streams on hardware queues of their own? (False = a serialised step)
    if distributed:
        # clock / power / calibration of EVERY rank (rank order): the first multi-GPU line shows what RCCL's kernels cost the cap
        mine = {"rank": rank, "sclk_mhz_avg": tel.get("sclk_mhz_avg"), "power_w_avg": tel.get("power_w_avg"),
                "junction_c_avg": tel.get("junction_c_avg"), "calibration_tflops": (calib or {}).get("tflops")}
        allr = [None] * world
        try:
            dist.all_gather_object(allr, mine)  # (object form: the same call under nccl and gloo)
        except Exception as e:  # never fatal: the line keeps rank 0's figures
            allr = [mine, {"error": f"{type(e).__name__}: {e}"[:120]}]
        result["telemetry"]["per_rank"] = allr
        result["rccl"] = {
            "ranks": dist.get_world_size(), "backend": args.backend, "collectives_launched_by": args.comm,
            # what RCCL itself reports for the C-ABI communicator (ncclCommCount / ncclCommUserRank), not this script's bookkeeping
            "communicator_ranks": (ts.reducer.comm.count()[0] if (ts.reducer is not None and ts.reducer.comm is not None) else None),
            "communicator_rank": (ts.reducer.comm.count()[1] if (ts.reducer is not None and ts.reducer.comm is not None) else None),
            "max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS", "default"),
            "self_test": comm_selftest, "buckets": len(ts.reducer.buckets) if ts.reducer is not None else 0,
            "bucket_mb": args.bucket_mb, "wire": "bf16" if args.wire_bf16 else "fp32",
            # (round 5) bucket size x wire dtype timed on this job before the warm-up (ms per step, max over ranks); the timed region
            # ran on `bucket_mb`.  `sweep` = the full --sweep table, `bucket_sweep` = the default short one.
            ("sweep" if args.sweep else "bucket_sweep"): sweep_rows,
        }
    if ts.reducer is not None:
        ex = ts.reducer.exposed_ms()
        if ex:
            # time the compute stream waited for the exchange at the end of backward (BASELINE.md §4 column)
            result["allreduce_exposed_ms"] = {"mean": round(sum(ex) / len(ex), 3), "max": round(max(ex), 3),
                                              "per_step": [round(v, 3) for v in ex[:32]]}
    want_roofline = args.full and not args.no_roofline and not ts.use_graph
    if want_roofline:
        # every rank runs the profiling steps (the exchange is collective); rank 0 reports
        flops_step, gemm_sec, in_step_rows = time_gemms_in_step(ts, next_batch, max(1, args.profile_steps))
    if rank == 0 and want_roofline:
        iso_flops, iso_sec, iso_rows, algo_bytes = time_gemms(args.batch, args.gemm_reps)
        traffic, traffic_src, step_bytes, stale = pmc_traffic(args.batch)
        achieved = flops_step / gemm_sec / 1e12
        wall = flops_step / (dt / args.steps) / 1e12
        isolated = iso_flops / iso_sec / 1e12
        note(f"GEMM roofline: in-step {achieved:.1f} TFLOP/s over {gemm_sec * 1e3:.2f} ms of GEMM kernel time per step; "
             f"isolated {isolated:.1f}; FLOPs / wall step {wall:.1f}")
        result["roofline"] = {
            "bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
            "frac_at_sustained_clock": _frac_at_clock(achieved, tel),
            "definition": "GEMM FLOPs of one step / sum of the in-step durations of its GEMM launches (HIP events on the "
                          "launch streams, 3 overlapping streams: the sum exceeds the wall step)",
            "wall": {"achieved": round(wall, 1), "frac": round(wall / PEAK_BF16_TFLOPS, 4), "frac_at_sustained_clock": _frac_at_clock(wall, tel),
                     "definition": "GEMM FLOPs of one step / measured wall time of the step"},
            "isolated": {"achieved": round(isolated, 1), "frac": round(isolated / PEAK_BF16_TFLOPS, 4),
                         "gemm_ms_per_step": round(iso_sec * 1e3, 3),
                         "definition": "each launch shape timed alone on random operands, weighted by count"},
            "traffic": traffic,
            "traffic_unit": "HBM-side bytes per step over all GEMM launches (PMC FETCH_SIZE x2 + WRITE_SIZE)",
            "traffic_source": traffic_src, "traffic_stale": stale, "algorithmic_bytes": round(algo_bytes),
            "kernel": "gemm_bf16_kernel<AT,BT,EPI,Cfg<192,128,2,2,2,64>> (forward, dX: four waves of 96x64, gemm_heuristic 9) + "
                      "gemm_grouped_tn_kernel<Cfg<256,256,2,4,5,32>,3,BG> (weight gradients): all GEMM launches of one step",
            "dominant_kernel": _dominant(in_step_rows),
            "gemm_ms_per_step": round(gemm_sec * 1e3, 3), "gemm_flops_per_step": flops_step,
            "shapes": in_step_rows, "shapes_isolated": iso_rows,
        }
        if step_bytes:
            # whole-step HBM-side bytes (every kernel, PMC passes) over the measured step time
            gbps = step_bytes / (dt / args.steps) / 1e9
            result["hbm"] = {"bytes_per_step": step_bytes, "achieved": round(gbps, 1), "peak": 8000.0, "unit": "GB/s",
                             "frac": round(gbps / 8000.0, 4), "source": traffic_src}
    if distributed:
        dist.barrier()
    if args.full and rank == 0 and world == 1 and not args.no_other_workloads and not args.force_ddp:
        # BASELINE configs 3 and 4 ride on a --full run (a few steps each), so that one command times every configuration
        import copy
        import gc

        del ts, model
        from cflearn_amd import fused as _fused

        _fused._plans.clear()  # the ViT stack's launch plan pins every buffer of its recorded step (and a large Python object graph)
        gc.collect()
        torch.cuda.empty_cache()
        others = {}
        # (unet256: BASELINE config 4 AS STATED — the zoo DDPM UNet at 256^2, batch 1 — next to the 64^2 x 8 line)
        for name, wl, kw in (("unet", "unet", dict(img=64, steps=5, warmup=3)), ("unet256", "unet", dict(img=256, steps=3, warmup=2)),
                             ("clip", "clip", dict(steps=8, warmup=3))):  # (warm-up >= 3: a block stack records its launch plan on call 2)
            a2 = copy.copy(args)
            a2.workload, a2.batch = wl, 128  # 128 = "the workload's default batch" (8 for the 64^2 UNet, 1 at 256^2, 256 for CLIP)
            a2.dump_outputs = None  # --dump-outputs covers the headline step only
            for k_, v_ in kw.items():
                setattr(a2, k_, v_)
            note(f"other workload: {name} ...")
            wl = name
            try:
                r = run_other_workload(a2)
                others[wl] = {k_: r[k_] for k_ in ("value", "unit", "ms_per_step", "host_issue_ms_per_step", "telemetry", "optimizer_in_backward", "steps", "warmup", "roofline", "peak_mem_gb")}
                others[wl]["workload"] = r["config"]["workload"]
                others[wl]["per_gpu_batch"] = r["config"]["per_gpu_batch"]
            except Exception as e:  # the headline line must survive a failure here
                others[wl] = {"error": f"{type(e).__name__}: {e}"[:300]}
            _fused._plans.clear()
            gc.collect()
            torch.cuda.empty_cache()
        result["other_workloads"] = others
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        note("cpu baseline (the reference's PyTorch-CPU step on the host cores) ...")
        result["cpu_baseline"] = cpu_baseline(args.cpu_batch, args.cpu_steps)
        note("cpu baseline done")
    # a helper stream that shares a hardware queue turns the overlapped step into a serialised one: every rank looks at its own
    # check and the line SAYS so (`streams.distinct_on_every_rank`, `warnings`) — the first scaling curve must not silently be
    # the serialised one; the measurement itself stays valid (it is what that node delivers), so the run only fails on request
    aliased = not result["streams"]["distinct"]
    if distributed:
        flag = torch.tensor([1 if aliased else 0], device=dev, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        aliased = bool(flag.item())
        result["streams"]["distinct_on_every_rank"] = not aliased
    if aliased:
        result.setdefault("warnings", []).append(
            "a helper stream (batch slice / weight-gradient lane / comm) shares a hardware queue with a stream it should overlap "
            "with on at least one rank: this step ran partly serialised (GPU_MAX_HW_QUEUES, --nchannels)")
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    if TELEMETRY is not None:
        TELEMETRY.stop()
    sys.stdout.flush()
    if rank == 0:  # after everything that could still print: the one line on the real stdout
        os.write(result_fd, (json.dumps(result) + "\n").encode())
    os.close(result_fd)
    if aliased:
        print("[bench] WARNING: a helper stream had to share a hardware queue (see `streams` / `warnings` in the line): the step ran "
              "partly serialised", file=sys.stderr)
        if args.strict_streams:
            raise SystemExit(3)


if __name__ == "__main__":
    main()
