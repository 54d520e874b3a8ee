"""The uint8 image input path without a GPU: the numpy restatement of its sampling rule, the boxes drawn, the route plan, the refusals."""
import numpy as np
import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops
from cflearn_amd.data import DeviceImageTransform, ImageBatcher

import image_replay as R

IMG = (10 * np.arange(4)[:, None] + np.arange(4)[None, :] + 5).astype(np.uint8)[None, :, :, None]  # value 10 y + x + 5


@pytest.mark.parametrize("box, flip, at, want", [
    ((0, 0, 4, 4), 0, (0, 1), 12.5),    # interior: sy = 0.5, sx = 2.5 -> the mean of rows 0, 1 x columns 2, 3
    ((-1, -1, 4, 4), 0, (0, 0), 5.0),   # clamped corner: sy = sx = -0.5 -> taps -1 and 0 both become pixel (0, 0)
    ((0, 0, 4, 4), 1, (0, 0), 12.5),    # flipped: output column 0 samples where column 1 did (unflipped it would be 10.5)
])
def test_replica_against_hand_computed_pixels(box, flip, at, want):
    ref, cond = R.transform(IMG, np.array([box], dtype=np.float32), [flip], [[1.0, 0.0]], (2, 2))
    assert ref[0, 0][at] == want and cond[0, 0][at] == want


def test_replica_identity_is_value_times_a_plus_b():
    src = np.random.default_rng(0).integers(0, 256, (2, 9, 7, 3), dtype=np.uint8)
    sb = np.array([[1 / 255 / 0.229, -0.485 / 0.229], [0.5, 3.0], [-2.0, 0.25]], dtype=np.float32)
    boxes = np.array([[2, 1, 5, 4], [4, 3, 5, 4]], dtype=np.float32)
    for bilinear in (True, False):
        ref, _ = R.transform(src, boxes, None, sb, (5, 4), bilinear)
        for b, (y0, x0) in enumerate(((2, 1), (4, 3))):
            crop = src[b, y0:y0 + 5, x0:x0 + 4].astype(np.float64).transpose(2, 0, 1)
            assert np.array_equal(ref[b], crop * sb[:, 0, None, None].astype(np.float64) + sb[:, 1, None, None])


def test_boxes_are_deterministic_inside_the_image_and_respect_scale_and_ratio():
    mk = lambda seed: DeviceImageTransform(16, mode="random_resized_crop", scale=(0.2, 0.7), ratio=(0.5, 2.0), flip=0.5, seed=seed)  # noqa: E731
    tf, args = mk(7), (512, 40, 56)
    box, flips = tf.boxes(3, *args)
    assert box.dtype == np.float32 and box.shape == (512, 4) and flips.dtype == np.uint8 and flips.shape == (512,)
    assert all(np.array_equal(a, b) for a, b in zip(mk(7).boxes(3, *args, epoch=0), (box, flips)))
    assert not any(np.array_equal(o[0], box) for o in (tf.boxes(4, *args), tf.boxes(3, *args, epoch=1), mk(8).boxes(3, *args)))
    tf.set_epoch(1)
    assert np.array_equal(tf.boxes(3, *args)[0], mk(7).boxes(3, *args, epoch=1)[0])
    (y0, x0, h, w), eps = box.astype(np.float64).T, 1e-4  # the boxes are float32
    assert (y0 >= 0).all() and (x0 >= 0).all() and (y0 + h <= 40 + eps).all() and (x0 + w <= 56 + eps).all()
    area, ratio = h * w / (40 * 56), w / h
    assert (area >= 0.2 - eps).all() and (area <= 0.7 + eps).all() and (ratio >= 0.5 - eps).all() and (ratio <= 2.0 + eps).all()
    assert area.max() - area.min() > 0.3 and 0.3 < flips.mean() < 0.7
    tall = DeviceImageTransform(16, mode="random_resized_crop", scale=(0.9, 1.0), ratio=(3.0, 4.0)).boxes(0, 4, 40, 40)[0]
    assert np.allclose(tall, [[(40 - 40 / 3) / 2, 0, 40 / 3, 40]] * 4)  # no try fits: the centred fallback of an allowed ratio


def test_center_crop_resize_and_inference_boxes():
    box, flips = DeviceImageTransform((8, 12), mode="center_crop", flip=1.0).boxes(0, 2, 20, 21)
    assert np.array_equal(box, [[6, 4.5, 8, 12]] * 2) and flips.tolist() == [1, 1]
    assert np.array_equal(DeviceImageTransform(8, mode="resize").boxes(5, 2, 20, 21)[0], [[0, 0, 20, 21]] * 2)
    inf = DeviceImageTransform(8, mode="random_resized_crop", flip=1.0, for_inference=True)
    box, flips = inf.boxes(0, 2, 20, 22)  # inference: the centre crop, no flip
    assert inf.mode == "center_crop" and np.array_equal(box, [[6, 7, 8, 8]] * 2) and flips.tolist() == [0, 0]


def test_normalisations_fold_into_scale_and_bias():
    sb = lambda n, c=3: np.array(DeviceImageTransform(8, normalize=n).scale_bias(c))  # noqa: E731
    v, mean, std = np.array([0.0, 17.0, 255.0])[:, None], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for n, want in ((("static", 255.0), v / 255.0), (("affine", 0.5, 0.25), (v / 255.0 - 0.5) / 0.25),
                    (("imagenet", mean, std), (v / 255.0 - np.array(mean)) / np.array(std)), (None, v + 0 * np.ones(3))):
        assert np.allclose(v * sb(n)[:, 0] + sb(n)[:, 1], want), n
    with pytest.raises(ValueError, match="3 / 3 channels for 1-channel"):
        sb(("imagenet", mean, std), 1)


def test_plan_takes_the_gather_route_past_the_lds_budget():
    whole = lambda hs, ws: np.array([[0, 0, hs, ws]], dtype=np.float32)  # noqa: E731
    for c in (1, 3, 4):
        assert ops.image_transform_plan(whole(40, 40), 40, 40, c, 9, 9) == "gather"
        assert ops.image_transform_plan(whole(37, 29), 37, 29, c, 33, 35) == "lds"
        assert ops.image_transform_plan(whole(256, 256), 256, 256, c, 224, 224) == "lds"
    assert ops.IMAGE_LDS_BYTES == 16384  # the bound: (ceil(32 ky) + 2) rows of (ceil(32 kx) + 2) C + 15 bytes rounded up to 16
    assert ops.image_transform_plan(np.array([[0, 0, 126, 32]], dtype=np.float32), 128, 32, 3, 32, 32) == "lds"      # 128 rows of 128 bytes
    assert ops.image_transform_plan(np.array([[0, 0, 127, 32]], dtype=np.float32), 128, 32, 3, 32, 32) == "gather"   # 129 rows
    assert ops.image_transform_plan(np.array([[0, 0, 8, 8], [0, 0, 40, 40]], dtype=np.float32), 40, 40, 3, 9, 9) == "gather"  # the largest scale decides


def test_refusals_fire_before_any_launch():
    lib, p = _lib.load(), 4096  # made-up device addresses: every call must return before its launch
    assert len(_lib.SIGNATURES["cfhip_image_transform"][1]) == 17 and len(_lib.SIGNATURES["cfhip_image_transform_plan"][1]) == 8
    call = lambda C=3, Ho=8, Wo=8, interp=1, route=0, row=51: lib.cfhip_image_transform(  # noqa: E731
        p, 51 * 13, row, 2, 13, 17, C, p, None, p, p, 0, Ho, Wo, interp, route, None)
    for kwargs, needle in ((dict(C=5), "C = 5"), (dict(C=0), "C = 0"), (dict(Ho=0), "output size"), (dict(Wo=0), "output size"),
                           (dict(interp=2), "interp = 2"), (dict(route=2), "route = 2"), (dict(row=50), "strides")):
        assert call(**kwargs) == -1 and needle in lib.cfhip_last_error().decode(), kwargs
    good = np.array([[0, 0, 4, 4]], dtype=np.float32)
    for bad, needle in (([0, 0, 0, 4], "empty"), ([0, 0, 4, -1], "empty"), ([np.nan, 0, 4, 4], "not finite"), ([0, 0, np.inf, 4], "not finite")):
        with pytest.raises(RuntimeError, match=needle):
            ops.image_transform_plan(np.array([good[0], bad], dtype=np.float32), 13, 17, 3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.image_transform(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), good, 8, [[1, 0]] * 3)
    for kwargs, needle in ((dict(mode="pad"), "mode"), (dict(interpolation="area"), "interpolation"), (dict(out_dtype=torch.float16), "out_dtype"),
                           (dict(scale=(0.0, 1.0)), "scale"), (dict(flip=1.5), "flip"), (dict(normalize=("static",)), "normalize")):
        with pytest.raises((ValueError, TypeError), match=needle):
            DeviceImageTransform(8, **kwargs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ImageBatcher([], "cpu", DeviceImageTransform(8))
    assert C.DeviceImageTransform is DeviceImageTransform and C.ImageBatcher is ImageBatcher and issubclass(ImageBatcher, C.data.TensorBatcher)
