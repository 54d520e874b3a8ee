"""cfhip_image_transform's sampling rule (include/cfhip.h) in numpy: coordinates and axis weights in f32 as the rule names them, the blend in float64."""
import numpy as np

F = np.float32


def _axis(origin, extent, out, idx, n, bilinear):
    """taps i0, i1 (clamped to [0, n - 1]) and the f32 weight of i1 for the output indices `idx` (already mirrored)"""
    k = F(extent) / F(out)
    s = (F(origin) + (idx.astype(F) + F(0.5)) * k) - F(0.5)
    i = np.floor(s) if bilinear else np.floor(s + F(0.5))
    w1 = (s - i) if bilinear else np.zeros_like(s)
    i = i.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1 if bilinear else i, 0, n - 1), w1


def transform(src, boxes, flips, scale_bias, size, bilinear=True):
    """src uint8 [B, Hs, Ws, C], boxes [B, 4] (y0, x0, h, w), flips [B] or None, scale_bias [C, 2] -> (ref, cond) float64
    [B, C, Ho, Wo]: ref = blend * a + b, cond = blend * |a| + |b| (what an f32 evaluation's rounding errors scale with)"""
    B, Hs, Ws, C = src.shape
    Ho, Wo = size
    sb = np.asarray(scale_bias, dtype=F).astype(np.float64)
    ref, cond = np.empty((B, C, Ho, Wo)), np.empty((B, C, Ho, Wo))
    for b in range(B):
        y0, x0, h, w = (F(v) for v in boxes[b])
        iy0, iy1, wy1 = _axis(y0, h, Ho, np.arange(Ho), Hs, bilinear)
        ix0, ix1, wx1 = _axis(x0, w, Wo, np.arange(Wo)[::-1] if flips is not None and flips[b] else np.arange(Wo), Ws, bilinear)
        wy0, wx0 = (F(1) - wy1).astype(np.float64)[:, None, None], (F(1) - wx1).astype(np.float64)[None, :, None]
        wy1, wx1 = wy1.astype(np.float64)[:, None, None], wx1.astype(np.float64)[None, :, None]
        img = src[b].astype(np.float64)
        tap = lambda iy, ix: img[iy[:, None], ix[None, :]]  # noqa: E731  [Ho, Wo, C]
        blend = tap(iy0, ix0) * (wy0 * wx0) + tap(iy0, ix1) * (wy0 * wx1) + tap(iy1, ix0) * (wy1 * wx0) + tap(iy1, ix1) * (wy1 * wx1)
        blend = blend.transpose(2, 0, 1)
        ref[b] = blend * sb[:, 0, None, None] + sb[:, 1, None, None]
        cond[b] = blend * np.abs(sb[:, 0, None, None]) + np.abs(sb[:, 1, None, None])
    return ref, cond
