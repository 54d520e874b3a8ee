"""Token merging (csrc/tome.hip) A/B on the GPU: what `setup_hooks(tome_info=dict(ratio=0.5))` does to the time of
  * a SpatialTransformer inference forward at C 320 / 8 heads, N = 4 096 (64^2, batch 8) and N = 16 384 (128^2, batch 2),
  * one DDIM step of the zoo UNet at 64^2 x 8 (eager sampling, 4 steps per window),
with and without merging, alternating in one process, HIP events, warm-up first; and the four ToMe launches on their own.

python tools/tome_bench.py [--out FILE]      (default profiles/r09/tome_ab.txt)

Merging is set as the reference's default (`merge_attn` only, max_downsample 1) with a fixed seed, so both arms repeat the same work."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops, tome  # noqa: E402

ROUNDS = 5
TOME = dict(ratio=0.5, seed=1)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def ab(name, plain, merged, extra=None):
    """alternate the two arms ROUNDS times; reps sized to ~0.3 s a window"""
    for fn in (plain, merged):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {k: max(3, int(0.3e6 / max(window(fn, 2), 1.0))) for k, fn in (("plain", plain), ("tome", merged))}
    us = dict(plain=[], tome=[])
    for _ in range(ROUNDS):
        for key, fn in (("plain", plain), ("tome", merged)):
            us[key].append(window(fn, reps[key]))
    rec = dict(case=name)
    for key in ("plain", "tome"):
        v = sorted(us[key])
        rec[key] = dict(reps=reps[key], us_min=round(v[0], 1), us_median=round(v[len(v) // 2], 1), us_max=round(v[-1], 1))
    rec["tome_over_plain"] = round(rec["tome"]["us_median"] / rec["plain"]["us_median"], 3)
    rec.update(extra or {})
    return rec


def transformer_case(dev, b, side):
    st = C.SpatialTransformer(320, 8, 40).to(dev).eval()
    with torch.no_grad():  # (from_latent is zero-initialised: irrelevant to the time, but give the blocks ordinary weights)
        for p in st.parameters():
            if p.dim() > 1:
                p.normal_(0.0, p.shape[1] ** -0.5)
    x = torch.randn((b, 320, side, side), device=dev, generator=torch.Generator(device=dev).manual_seed(side)).bfloat16()

    def run(info):
        st.setup_hooks(tome_info=info)
        for block in st.blocks:
            if block.tome_info is not None:
                block.tome_info["size"] = (side, side)
        with torch.no_grad():
            return st(x, None)

    rec = ab(f"SpatialTransformer C320 h8 B{b} N{side * side}", lambda: run(None), lambda: run(TOME))
    st.setup_hooks()
    return rec


def launches_case(dev, b, side):
    n, c = side * side, 320
    x = torch.randn((b, n, c), device=dev, generator=torch.Generator(device=dev).manual_seed(n)).bfloat16()
    info = tome.setup_tome_info(dict(TOME))
    info["size"] = (side, side)
    sizes = tome.merge_sizes(n, info)
    tm = tome.TokenMerge(x, info, sizes)
    y = tm.merge(x)
    fns = dict(match=lambda: ops.tome_match(x, tm.src_idx, tm.dst_idx),
               select=lambda: ops.tome_select(tm.node_max, tm.node_idx, tm.src_idx, tm.dst_idx, tm.r),
               merge=lambda: tm.merge(x), unmerge_add=lambda: tm.unmerge_add(y, x))
    rec = dict(case=f"ToMe launches alone C320 B{b} N{n} r{tm.r}")
    for key, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps = max(5, int(0.1e6 / max(window(fn, 3), 1.0)))
        v = sorted(window(fn, reps) for _ in range(ROUNDS))
        rec[key] = dict(reps=reps, us_min=round(v[0], 1), us_median=round(v[len(v) // 2], 1), us_max=round(v[-1], 1))
    rec["sum_us_median"] = round(sum(rec[k]["us_median"] for k in fns), 1)
    return rec


def unet_case(dev):
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    torch.manual_seed(0)
    cfg = dict(in_channels=3, out_channels=3, start_channels=320, num_heads=8, use_spatial_transformer=True, num_transformer_layers=1,
               num_res_blocks=2, attention_downsample_rates=(1, 2, 4), channel_multipliers=(1, 2, 4, 4), context_dim=None)
    unet = C.build_module("unet_diffuser", config=cfg).to(dev).eval()
    s = make_sampler("ddim", unet, NoiseSchedule(device=dev))
    z = torch.randn((8, 3, 64, 64), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    steps = 4

    def run(info):
        unet.setup_hooks(tome_info=info)
        return s.sample(z, num_steps=steps, seed=1)

    rec = ab("zoo UNet 64^2 x 8, DDIM, eager, per 4-step sample", lambda: run(None), lambda: run(TOME), dict(steps_per_call=steps))
    for key in ("plain", "tome"):
        rec[key]["ms_per_step_median"] = round(rec[key]["us_median"] / steps / 1e3, 3)
    unet.setup_hooks()
    return rec


def main():
    out_path = os.path.join(ROOT, "profiles", "r09", "tome_ab.txt")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    if not torch.cuda.is_available():
        raise SystemExit("tome_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lines = [f"# tools/tome_bench.py on {torch.cuda.get_device_name(0)}: tome_info=dict(ratio=0.5, seed=1) against the plain path; us per "
             f"call, {ROUNDS} rounds alternating in one process"]
    for b, side in ((8, 64), (2, 128)):
        lines.append(json.dumps(transformer_case(dev, b, side)))
        print(lines[-1], flush=True)
        lines.append(json.dumps(launches_case(dev, b, side)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(unet_case(dev)))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
