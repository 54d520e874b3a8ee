"""cfhip_image_transform on the device, per element against the float64 restatement of its sampling rule (tests/image_replay.py),
under guard bytes; the two routes against each other and the identity path bit for bit; ImageBatcher against ops.image_transform."""
import functools

import numpy as np
import pytest
import torch

from cflearn_amd import ops
from cflearn_amd.data import DeviceImageTransform, ImageBatcher

from helpers import assert_elementwise, guarded_ops
import image_replay as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (Hs, Ws) -> (Ho, Wo): a small tile; both 32-wide tile edges crossed; past the LDS budget (planned: gather); an upscale.  Rows of 51 and 87 bytes are in the set.
SHAPES = [((13, 17), (8, 8)), ((37, 29), (33, 35)), ((40, 40), (9, 9)), ((7, 5), (33, 20))]
SHAPE_ID = lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}"  # noqa: E731
SCALE_BIAS = np.array([[1 / 255 / 0.229, -0.485 / 0.229], [1 / 255 / 0.224, -0.456 / 0.224], [0.0123, 1.75], [-1 / 127.5, 1.0]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case(c, hs, ws, ho, wo, bilinear, flip):
    # shared by a case's f32 and bf16 forms; 3 samples: a box over the top and left edges, one over the bottom and right edges, one inside
    rng = np.random.default_rng(1000 * hs + 10 * ws + c)
    src = rng.integers(0, 256, (3, hs, ws, c), dtype=np.uint8)
    boxes = np.float32([[-1.3, -2.6, 0.71 * hs, 0.83 * ws], [0.37 * hs, 0.29 * ws, 0.93 * hs, 0.81 * ws], [0.21, 0.43, 0.77 * hs, 0.69 * ws]])
    flips = np.array([1, 0, 1], dtype=np.uint8) if flip else None
    return src, boxes, flips, R.transform(src, boxes, flips, SCALE_BIAS[:c], (ho, wo), bilinear)


def check(got, ref, cond, bilinear):
    """The bound, from the arithmetic of the rule.  The coordinates and the four axis weights are f32 values the reference shares
    exactly.  Bilinear: w_ij = wy wx (1 rounding), v_ij w_ij (1), three sums (3), the product with a (1), the sum with b (1): 7
    roundings of at most 2^-24 relative to quantities bounded by cond = blend |a| + |b|; 8 covers the second-order terms.  Nearest:
    the tap is exact, 2 roundings.  A bf16 destination adds one rounding of the result: 1 ulp of bf16."""
    assert_elementwise(got, torch.from_numpy(ref), out_dtype=got.dtype, ulps=float(got.dtype == torch.bfloat16), cond=torch.from_numpy(cond),
                       k=8 if bilinear else 2, what="image_transform")


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("interpolation", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("c", [1, 3, 4])
def test_against_replica_per_element(c, shape, interpolation, dtype, flip, monkeypatch):
    (hs, ws), (ho, wo), bilinear = *shape, interpolation == "bilinear"
    src, boxes, flips, (ref, cond) = case(c, hs, ws, ho, wo, bilinear, flip)
    g = guarded_ops(monkeypatch)
    got = ops.image_transform(g.index(torch.from_numpy(src).to(DEV)), boxes, (ho, wo), SCALE_BIAS[:c], flips=flips, interpolation=interpolation, out_dtype=dtype)
    assert got.shape == (3, c, ho, wo) and got.dtype == dtype
    g.check()
    check(got, ref, cond, bilinear)


@pytest.mark.parametrize("interpolation", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", SHAPES + [((150, 160), (9, 9))], ids=SHAPE_ID)
@pytest.mark.parametrize("c", [1, 3, 4])
def test_routes_are_bit_identical(c, shape, interpolation, monkeypatch):
    # forced LDS route: the 40 x 40 source is staged whole; the 150 x 160 tile exceeds LDS and gathers inside the LDS kernel
    (hs, ws), (ho, wo) = shape
    src, boxes, flips, _ = case(c, hs, ws, ho, wo, interpolation == "bilinear", True)
    assert ops.image_transform_plan(boxes, hs, ws, c, ho, wo) == ("gather" if (ho, wo) == (9, 9) else "lds")
    g = guarded_ops(monkeypatch)
    dev = g.index(torch.from_numpy(src).to(DEV))
    lds, gather = (ops.image_transform(dev, boxes, (ho, wo), SCALE_BIAS[:c], flips=flips, interpolation=interpolation, route=r) for r in ("lds", "gather"))
    g.check()
    assert torch.equal(lds, gather)


@pytest.mark.parametrize("route", ["lds", "gather"])
@pytest.mark.parametrize("interpolation", ["bilinear", "nearest"])
def test_identity_box_is_value_times_a_plus_b_bit_for_bit(interpolation, route):
    src = np.random.default_rng(5).integers(0, 256, (2, 45, 41, 3), dtype=np.uint8)
    boxes = np.float32([[3, 2, 40, 37], [5, 4, 40, 37]])  # integer origin, h == Ho, w == Wo, two tiles each way: the weights are 1, 0, 0, 0
    got = ops.image_transform(torch.from_numpy(src).to(DEV), boxes, (40, 37), SCALE_BIAS[:3], interpolation=interpolation, route=route)
    for b, (y0, x0) in enumerate(((3, 2), (5, 4))):
        crop = src[b, y0:y0 + 40, x0:x0 + 37].astype(np.float32).transpose(2, 0, 1)
        want = crop * SCALE_BIAS[:3, 0, None, None] + SCALE_BIAS[:3, 1, None, None]  # numpy float32: one rounding per operation
        assert want.dtype == np.float32 and np.array_equal(got[b].cpu().numpy(), want)


def test_row_and_batch_strides_are_honoured():
    src, boxes, flips, _ = case(3, 37, 29, 33, 35, True, True)
    want = ops.image_transform(torch.from_numpy(src).to(DEV), boxes, (33, 35), SCALE_BIAS[:3], flips=flips)
    wide = torch.full((3, 37 + 2, 29 + 3, 3), 255, dtype=torch.uint8, device=DEV)  # rows 96 bytes apart, samples two rows further
    view = wide[:, :37, :29].copy_(torch.from_numpy(src))
    assert not view.is_contiguous() and view.stride() == (39 * 96, 96, 3, 1)
    assert all(torch.equal(ops.image_transform(view, boxes, (33, 35), SCALE_BIAS[:3], flips=flips, route=r), want) for r in ("lds", "gather"))
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_transform(wide[:, :, ::2], boxes, (33, 35), SCALE_BIAS[:3])


def test_image_batcher_equals_ops_and_repeats_with_the_seed():
    rng = np.random.default_rng(11)
    loader = [{"input": rng.integers(0, 256, (n, 20, 24, 3), dtype=np.uint8), "labels": np.arange(n)} for n in (4, 4, 2)]  # ragged last batch
    make = lambda: DeviceImageTransform(16, mode="random_resized_crop", flip=0.5, normalize=("affine", 0.5, 0.5), out_dtype=torch.bfloat16, seed=3)  # noqa: E731
    tf, first = make(), []
    for i, batch in enumerate(ImageBatcher(loader, DEV, tf)):
        boxes, flips = tf.boxes(i, len(loader[i]["labels"]), 20, 24, epoch=0)
        want = ops.image_transform(torch.from_numpy(loader[i]["input"]).to(DEV), boxes, 16, tf.scale_bias(3), flips=flips, out_dtype=torch.bfloat16)
        assert batch["input"].dtype == torch.bfloat16 and torch.equal(batch["input"], want)
        assert batch["labels"].dtype == torch.int64 and batch["labels"].tolist() == list(range(len(boxes)))  # other keys: the base class
        first.append(want.clone())
    again = ImageBatcher(loader, DEV, make(), depth=2)
    assert all(torch.equal(batch["input"], want) for batch, want in zip(again, first))
    assert [b["input"].shape[0] for b in again] == [4, 4, 2] and again.epoch == 2  # the same batcher's next epoch
