"""Generate the token-merging fixture from the reference's own code on the CPU (modules/core/mixed_stacks/api.py:473-685):

    python tools/gen_tome_golden.py

  tests/golden/tome_small.pt
    "splits"  the src / dst token sets of bipartite_soft_matching_random2d for a table of (h, w, sx, sy, seed, use_rand), read out
              of the closures it returns (a_idx / b_idx), sorted;
    "sizes"   what compute_merge decides for a table of (H0, W0, downsample, ratio, max_downsample, sx, sy): merged or not, the r
              it merges and the number of dst tokens;
    "blocks"  the reference's fp32 SpatialTransformerBlock (query_dim 64, 2 heads of 32, context_dim 32) with `tome_info` on
              constructed inputs, for three flag sets and two shapes: the input, the context, the merged (src token, dst token)
              pairs, the fp32 output `y`, the reference's own output under torch.autocast("cpu", bfloat16) `y_bf16`, and the
              margins asserted below.

The block inputs are built so that the merge decision cannot depend on precision: dst tokens are orthogonal prototypes (plus small
noise), r src tokens sit close to one prototype each (at distinct distances), the rest of the src tokens live in the channels no
prototype uses.  Two margins are ASSERTED here, each at least 8 x the largest |score difference| between the reference's fp32
metric and its bf16-autocast metric: the top-2 gap of every merged row, and the gap between the r-th and (r+1)-th node_max.

Needs the reference tree (oracle/refharness finds it); writes data only, no parameters (every block is filled by `seeded_state` of
tools/gen_first_stage_golden.py, which the tests repeat).  Single-threaded and seeded: a second run writes the same values."""
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from refharness import import_cflearn  # noqa: E402
from gen_first_stage_golden import _fill  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# (h, w, sx, sy, seed, use_rand)
SPLIT_CASES = [(h, w, 2, 2, seed, rand) for (h, w) in ((8, 8), (16, 12), (9, 7)) for seed in (3, 1234) for rand in (True, False)]
SPLIT_CASES += [(8, 6, 1, 2, 3, True), (8, 6, 1, 2, 1234, True), (8, 6, 1, 2, 3, False)]
# (H0, W0) x downsample x ratio x max_downsample, sx = sy = 2, plus a few other cells
SIZE_CASES = [(h0, w0, d, ratio, md, 2, 2) for (h0, w0) in ((8, 8), (16, 12), (9, 7), (15, 13), (32, 32)) for d in (1, 2, 4)
              for ratio in (0.5, 0.25, 0.9, 0.0) for md in (1, 2)]
SIZE_CASES += [(8, 6, 1, 0.5, 1, 1, 2), (9, 7, 1, 0.75, 1, 3, 3), (5, 5, 1, 0.5, 1, 4, 4), (3, 3, 1, 0.5, 1, 4, 4)]

BLOCK_CFG = dict(query_dim=64, num_heads=2, head_dim=32, context_dim=32)
BLOCK_SEED = 2207
BLOCK_SHAPES = [(8, 8), (9, 7)]
BLOCK_FLAGS = {
    "attn": dict(merge_attn=True, merge_crossattn=False, merge_mlp=False),
    "all": dict(merge_attn=True, merge_crossattn=True, merge_mlp=True),
    "cross_mlp": dict(merge_attn=False, merge_crossattn=True, merge_mlp=True),
}
SPLIT_SEED = 11
MARGIN_FACTOR = 8.0


def _api():
    import importlib

    return importlib.import_module("cflearn.modules.core.mixed_stacks.api")


def _closure(fn, name):
    return inspect.getclosurevars(fn).nonlocals[name]


def ref_split(api, h, w, sx, sy, seed, use_rand):
    """(src tokens, dst tokens), sorted, from the closures of the reference's matching on a dummy metric"""
    x = torch.randn((1, h * w, 8), generator=torch.Generator().manual_seed(0))
    merge, _ = api.bipartite_soft_matching_random2d(x, w, h, sx, sy, 1, seed, not use_rand)
    split = _closure(merge, "split")
    src = _closure(split, "a_idx").reshape(-1).sort().values
    dst = _closure(split, "b_idx").reshape(-1).sort().values
    return src.to(torch.int32), dst.to(torch.int32)


def ref_sizes(api, h0, w0, d, ratio, md, sx, sy):
    n = -(-h0 // d) * -(-w0 // d)
    x = torch.randn((1, n, 8), generator=torch.Generator().manual_seed(0))
    info = dict(ratio=ratio, max_downsample=md, sx=sx, sy=sy, use_rand=False, merge_attn=True, merge_crossattn=False, merge_mlp=False,
                size=(h0, w0))
    hsy, wsx = -(-h0 // d) // sy, -(-w0 // d) // sx
    if hsy * wsx == 0 and d <= md and int(n * ratio) > 0:  # (the reference takes a max over an empty axis there: no record)
        return dict(num_tokens=n, merged=False, r=0, n_dst=0, reference_raises=True)
    m = api.compute_merge(x, info)[0]
    if m is api.do_nothing:
        return dict(num_tokens=n, merged=False, r=0, n_dst=0)
    return dict(num_tokens=n, merged=True, r=int(_closure(m, "r")), n_dst=int(_closure(_closure(m, "split"), "num_dst")))


def block_input(src, dst, n, c, r, batch, seed):
    """[batch, n, c]: prototypes on the dst tokens, r src tokens near one prototype each, the others in the unused channels"""
    g = torch.Generator().manual_seed(seed)
    n_dst, n_src = dst.numel(), src.numel()
    assert n_dst <= c // 2
    x = torch.zeros(batch, n, c)
    for b in range(batch):
        proto = 4.0 * torch.eye(n_dst, c)
        x[b, dst.long()] = proto + 0.02 * torch.randn((n_dst, c), generator=g)
        order = torch.randperm(n_src, generator=g)
        for k in range(n_src):
            tok = int(src[order[k]])
            if k < r:  # near prototype p, at a distance that grows with k: distinct node_max values, a clear top-2 gap
                p = 0 if k % 3 == 0 else (k * 5 + b) % n_dst
                noise = torch.zeros(c)
                noise[c // 2:] = torch.randn((c - c // 2,), generator=g)
                x[b, tok] = proto[p] + (0.2 + 0.01 * k) * noise / noise.norm() * 4.0 * 0.25
            else:  # far from every prototype
                v = torch.zeros(c)
                v[c // 2:] = torch.randn((c - c // 2,), generator=g)
                x[b, tok] = 3.0 * v / v.norm() + 0.02 * torch.randn((c,), generator=g)
    return x


def _scores(x, src, dst):
    m = x / x.norm(dim=-1, keepdim=True)
    return m[:, src.long()] @ m[:, dst.long()].transpose(-1, -2)


def block_fixture(api, h, w, flags):
    n, c = h * w, BLOCK_CFG["query_dim"]
    src, dst = ref_split(api, h, w, 2, 2, SPLIT_SEED, True)
    r = min(src.numel(), int(n * 0.5))
    x = block_input(src, dst, n, c, r, 2, BLOCK_SEED + h * 100 + w)
    context = torch.randn((2, 5, BLOCK_CFG["context_dim"]), generator=torch.Generator().manual_seed(BLOCK_SEED + 7))
    # the two margins against the reference's own precision spread on the metric
    full = _scores(x, src, dst)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        low = _scores(x, src, dst).float()
    spread = float((full - low).abs().max())
    top2 = full.topk(2, dim=-1).values
    node_max = top2[..., 0]
    ranked = node_max.sort(dim=-1, descending=True)
    merged_rows = ranked.indices[:, :r]
    gap_top2 = float(torch.gather(top2[..., 0] - top2[..., 1], 1, merged_rows).min())
    gap_r = float((ranked.values[:, r - 1] - ranked.values[:, r]).min()) if r < src.numel() else float("inf")
    assert gap_top2 >= MARGIN_FACTOR * spread, (h, w, gap_top2, spread)
    assert gap_r >= MARGIN_FACTOR * spread, (h, w, gap_r, spread)

    block = api.SpatialTransformerBlock(**BLOCK_CFG)
    _fill(block, BLOCK_SEED)
    block.eval()
    info = dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=True, seed=SPLIT_SEED, size=(h, w), **flags)
    block.setup_hooks(tome_info=info)
    with torch.no_grad():
        y = block(x, context).float().clone()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y_bf16 = block(x, context).float().clone()
        # the pairs the reference merges: (src token, dst token) per sample, sorted by src token
        merge, _ = api.bipartite_soft_matching_random2d(x, w, h, 2, 2, int(n * 0.5), SPLIT_SEED, False)
    a_idx = _closure(_closure(merge, "split"), "a_idx").reshape(-1)
    b_idx = _closure(_closure(merge, "split"), "b_idx").reshape(-1)
    src_pos, dst_pos = _closure(merge, "src_idx")[..., 0], _closure(merge, "dst_idx")[..., 0]
    pairs = []
    for b in range(x.shape[0]):
        p = sorted((int(a_idx[i]), int(b_idx[j])) for i, j in zip(src_pos[b].tolist(), dst_pos[b].tolist()))
        pairs.append(torch.tensor(p, dtype=torch.int32))
    return dict(h=h, w=w, tome_info={k: v for k, v in info.items() if k != "size"}, x=x, context=context, y=y, y_bf16=y_bf16, r=r,
                pairs=torch.stack(pairs), src=src, dst=dst, score_spread=spread, gap_top2=gap_top2, gap_r=gap_r,
                margin_factor=MARGIN_FACTOR)


def generate():
    torch.set_num_threads(1)
    import_cflearn()
    api = _api()
    splits = []
    for case in SPLIT_CASES:
        src, dst = ref_split(api, *case)
        splits.append(dict(case=case, src=src, dst=dst))
    sizes = [dict(case=case, **ref_sizes(api, *case)) for case in SIZE_CASES]
    blocks = {}
    for (h, w) in BLOCK_SHAPES:
        for name, flags in BLOCK_FLAGS.items():
            blocks[f"{h}x{w}-{name}"] = block_fixture(api, h, w, flags)
    return dict(splits=splits, sizes=sizes, blocks=blocks, block_cfg=dict(BLOCK_CFG), block_seed=BLOCK_SEED)


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "tome_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for key, rec in data["blocks"].items():
        print(f"  {key}: r {rec['r']}, score spread {rec['score_spread']:.3e}, top-2 gap {rec['gap_top2']:.3e}, r-th gap {rec['gap_r']:.3e}")


if __name__ == "__main__":
    main()
