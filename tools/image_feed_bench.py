"""A/B of the image input path on the MI355X: one ViT-shaped batch (128 x 224 x 224 x 3 out of 256 x 256 sources) fed end to end on
the copy stream, alternating in one process:

    uint8    `data.ImageBatcher`: the uint8 HWC batch (25.2 MB) crosses PCIe, cfhip_image_transform crops / resizes / normalizes it
    float32  `data.TensorBatcher`: the finished float32 NCHW batch (77.1 MB) crosses PCIe (what the host had to prepare in numpy)

    python tools/image_feed_bench.py [--out profiles/r16/image_feed_ab.txt] [--rounds 7] [--batches 8]

A timed call iterates a batcher over `batches` host batches with an idle consumer, so the figure is what the feed itself takes per
batch (copy, and transform where there is one) between device events on the consuming stream; the host preparation of the float32
batch is NOT in its figure.  Then the transform launch alone, the batch already on the device, on each route, for the random-crop
boxes of training and for the centre crop (the identity path), with the bytes it moves over its time.  Every figure is the median
over `rounds` alternating rounds with their min .. max; shader clock and socket power come from tools/gpu_telemetry.py.  Needs the
GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cflearn_amd import ops  # noqa: E402
from cflearn_amd.data import DeviceImageTransform, ImageBatcher, TensorBatcher  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402
from tools.rnn_bench import alternate, fmt, timed  # noqa: E402

DEV = "cuda"
B, HS, WS, C, SIZE = 128, 256, 256, 3, 224
IMAGENET = ("imagenet", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "image_feed_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_feed_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    rng = np.random.default_rng(0)
    u8 = [{"input": rng.integers(0, 256, (B, HS, WS, C), dtype=np.uint8)} for _ in range(args.batches)]
    f32 = [{"input": rng.random((B, C, SIZE, SIZE), dtype=np.float32)} for _ in range(args.batches)]
    tf = DeviceImageTransform(SIZE, mode="random_resized_crop", flip=0.5, normalize=IMAGENET, out_dtype=torch.float32, seed=1)
    feeds = {"uint8": ImageBatcher(u8, DEV, tf), "float32": TensorBatcher(f32, DEV)}

    def feed_of(batcher):
        def go():
            for _ in batcher:
                pass
        return go

    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; image feed of one ViT batch ({B} x {SIZE} x {SIZE} x {C} from "
             f"{HS} x {WS} sources); rounds {args.rounds}; ms: median (min .. max over the alternating rounds); telemetry: "
             f"{tel.source.name if tel.available else 'unavailable (' + str(tel.error) + ')'}"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    shown = 0

    def flush() -> None:  # (after every section: a later failure keeps what was measured)
        nonlocal shown
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")

    bytes_u8, bytes_f32 = B * HS * WS * C + 17 * B, 4 * B * C * SIZE * SIZE
    r = alternate({k: feed_of(v) for k, v in feeds.items()}, args.rounds, 1, tel)
    for k in r:
        r[k]["ms"] = tuple(x / args.batches for x in r[k]["ms"])
    lines.append(f"feed, per batch of {args.batches} in a row (idle consumer): " + "   ".join(fmt(k, v) for k, v in r.items()))
    ratio = r["float32"]["ms"][0] / r["uint8"]["ms"][0]
    lines.append(f"   bytes over PCIe per batch: uint8 {bytes_u8} ({bytes_u8 / 1e6:.1f} MB), float32 {bytes_f32} ({bytes_f32 / 1e6:.1f} MB); "
                 f"float32 / uint8 time {ratio:.2f}x" + ("" if ratio >= 1.0 else "   (the uint8 path is SLOWER at this shape)"))
    results["feed"] = dict(r, bytes=dict(uint8=bytes_u8, float32=bytes_f32))
    flush()

    src = torch.from_numpy(u8[0]["input"]).to(DEV)
    table = ops.image_scale_bias(tf.scale_bias(C), DEV)
    out = torch.empty((B, C, SIZE, SIZE), dtype=torch.float32, device=DEV)
    centre = DeviceImageTransform(SIZE, mode="center_crop", normalize=IMAGENET)
    for name, (boxes, flips) in (("random_resized_crop", tf.boxes(0, B, HS, WS)), ("center_crop", centre.boxes(0, B, HS, WS))):
        dev_boxes, dev_flips = torch.from_numpy(boxes).to(DEV), torch.from_numpy(flips).to(DEV)
        variants = {route: (lambda route=route: ops.image_transform(src, boxes, SIZE, table, flips=flips, out=out, route=route, dev_boxes=dev_boxes,
                                                                   dev_flips=dev_flips)) for route in ("lds", "gather")}
        inner = max(5, int(200.0 / max(max(timed(fn, 2) for fn in variants.values()), 1e-3)))
        r = alternate(variants, args.rounds, inner, tel)
        moved = B * HS * WS * C + out.numel() * 4  # at most: the whole source once, the destination once
        lines.append(f"transform alone, {name} (planned route: {ops.image_transform_plan(boxes, HS, WS, C, SIZE, SIZE)}; {inner} launches per round): "
                     + "   ".join(fmt(k, v) for k, v in r.items()))
        lines.append("   " + "   ".join(f"{k}: <= {moved / v['ms'][0] / 1e6:.0f} GB/s of source + destination" for k, v in r.items()))
        results[name] = dict(r, inner=inner, bytes_at_most=moved)
        flush()
    tel.stop()


if __name__ == "__main__":
    main()
