"""Token merging (tomesd) for the SpatialTransformer blocks: the host side of the reference's SpatialTransformerHooks
(modules/core/mixed_stacks/api.py:473-618, 645-685) — the `tome_info` dictionary, the gate and size arithmetic of `compute_merge`,
the src / dst split of `bipartite_soft_matching_random2d` — and `TokenMerge`, which runs the match and select kernels of
csrc/tome.hip once per block forward and hands out `merge` / `unmerge_add` on their tables.  Forward only.

The split is built on the host exactly as the reference builds it on the CPU (`torch.randint(sy * sx, (h // sy, w // sx, 1))` from a
CPU generator seeded with `seed`), cached per (h, w, sx, sy, seed, use_rand) and kept on the device as two int32 tables of token
ids, each ascending.  The order inside the merged rows is defined here (the reference's comes from unstable sorts and is invisible
after `unmerge`): unmerged src rows in ascending token order, then dst rows in ascending token order."""
import functools
import math
import random
from typing import Any, Dict, Optional, Tuple

import torch
from torch import Tensor

from . import ops

TOME_DEFAULTS: Dict[str, Any] = dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=True, merge_attn=True, merge_crossattn=False,
                                     merge_mlp=False)
TOME_KEYS = frozenset(TOME_DEFAULTS) | {"seed", "size"}


def setup_tome_info(tome_info: Optional[Dict[str, Any]]) -> Optional[Dict[str, Any]]:
    """SpatialTransformerHooks.setup (api.py:654-672): a shallow copy with the reference's defaults; None switches merging off"""
    if tome_info is None:
        return None
    unknown = sorted(set(tome_info) - TOME_KEYS)
    if unknown:
        raise TypeError(f"tome_info: unknown keys {unknown} (known: {sorted(TOME_KEYS)})")
    info = dict(tome_info)
    for k, v in TOME_DEFAULTS.items():
        info.setdefault(k, v)
    return info


def new_seed() -> int:
    return random.randint(0, 2 ** 31 - 1)


def merge_sizes(num_tokens: int, info: Dict[str, Any]) -> Optional[Tuple[int, int, int]]:
    """compute_merge's arithmetic (api.py:592-602) and the two early returns of bipartite_soft_matching_random2d (:485, :542):
    (h, w, r) of the token grid this block sees and the number of tokens to merge, or None when nothing is merged"""
    if "size" not in info:
        raise RuntimeError("tome_info['size'] is missing: it is written by the forward of the UNet / ControlNet that owns the block "
                           "(a block used on its own: put the (H, W) of the token grid at downsample 1 there)")
    h0, w0 = (int(s) for s in info["size"])
    downsample = int(math.ceil(math.sqrt((h0 * w0) // num_tokens)))
    if downsample > info["max_downsample"]:
        return None
    w = int(math.ceil(w0 / downsample))
    h = int(math.ceil(h0 / downsample))
    r = int(num_tokens * info["ratio"])
    if r <= 0:
        return None
    n_dst = (h // info["sy"]) * (w // info["sx"])
    r = min(num_tokens - n_dst, r)
    if r <= 0 or n_dst <= 0:
        return None
    return h, w, r


@functools.lru_cache(maxsize=64)
def split_tables(h: int, w: int, sx: int, sy: int, seed: Optional[int], use_rand: bool) -> Tuple[Tensor, Tensor]:
    """(src_idx, dst_idx): int32 CPU tensors of token ids, each ascending (api.py:490-528): one token of every sy x sx cell of the
    top-left (h // sy * sy) x (w // sx * sx) region is dst, everything else (the margin included) src"""
    hsy, wsx = h // sy, w // sx
    if not use_rand:
        rand_idx = torch.zeros(hsy, wsx, 1, dtype=torch.int64)
    else:
        generator = torch.Generator("cpu").manual_seed(int(seed))
        rand_idx = torch.randint(sy * sx, size=(hsy, wsx, 1), generator=generator)
    view = torch.zeros(hsy, wsx, sy * sx, dtype=torch.int64)
    view.scatter_(dim=2, index=rand_idx, src=-torch.ones_like(rand_idx))
    view = view.view(hsy, wsx, sy, sx).transpose(1, 2).reshape(hsy * sy, wsx * sx)
    buf = torch.zeros(h, w, dtype=torch.int64)
    buf[: hsy * sy, : wsx * sx] = view
    flat = buf.reshape(-1)
    dst = torch.nonzero(flat == -1).view(-1).to(torch.int32)
    src = torch.nonzero(flat == 0).view(-1).to(torch.int32)
    return src, dst


_DEVICE_TABLES: Dict[Tuple[Any, ...], Tuple[Tensor, Tensor]] = {}


def device_tables(key: Tuple[int, int, int, int, Optional[int], bool], device: torch.device) -> Tuple[Tensor, Tensor]:
    """the split of `key` on `device`; a fixed split (seed given, or use_rand off) is uploaded once and kept"""
    fixed = key[4] is not None or not key[5]
    full = key + (str(device),)
    if fixed and full in _DEVICE_TABLES:
        return _DEVICE_TABLES[full]
    if not fixed:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise ValueError("token merging under graph capture needs a fixed split: give tome_info a `seed` or `use_rand=False` "
                             "(a fresh split per forward cannot be replayed)")
        key = key[:4] + (new_seed(), True)  # (api.py:610: a fresh seed per block forward)
        src, dst = split_tables.__wrapped__(*key)
    else:
        src, dst = split_tables(*key)
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise ValueError("token merging under graph capture: the split tables of this shape were not uploaded by a warm-up pass")
    out = (src.to(device), dst.to(device))
    if fixed:
        if len(_DEVICE_TABLES) >= 256:
            _DEVICE_TABLES.clear()
        _DEVICE_TABLES[full] = out
    return out


class TokenMerge:
    """One block forward's merge: the matching of `net` (bf16 [B, N, C], the metric, api.py:603-604) on the split of `info`, as the
    tables of cfhip_tome_select.  `merge(x)` -> bf16 [B, N - r, C]; `unmerge_add(y, residual)` -> residual + unmerge(y)."""

    def __init__(self, net: Tensor, info: Dict[str, Any], sizes: Tuple[int, int, int]):
        h, w, r = sizes
        key = (h, w, int(info["sx"]), int(info["sy"]), None if info.get("seed") is None else int(info["seed"]), bool(info["use_rand"]))
        self.src_idx, self.dst_idx = device_tables(key, net.device)
        self.r = r
        metric = net if net.dtype == torch.bfloat16 else ops.to_bf16(net.float().contiguous())
        if not metric.is_contiguous():
            metric = metric.contiguous()
        self.node_max, self.node_idx = ops.tome_match(metric, self.src_idx, self.dst_idx)
        self.row_of_token, self.token_of_row, self.member_off, self.members = ops.tome_select(
            self.node_max, self.node_idx, self.src_idx, self.dst_idx, r)

    def merge(self, x: Tensor) -> Tensor:
        if x.dtype != torch.bfloat16:
            x = ops.to_bf16(x.float().contiguous())
        return ops.tome_merge(x.contiguous(), self.token_of_row, self.member_off, self.members)

    def unmerge_add(self, y: Tensor, residual: Optional[Tensor]) -> Tensor:
        if y.dtype != torch.bfloat16:
            y = ops.to_bf16(y.float().contiguous())
        return ops.tome_unmerge_add(y.contiguous(), self.row_of_token, None if residual is None else residual.contiguous())
