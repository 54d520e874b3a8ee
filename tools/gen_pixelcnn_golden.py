"""Generate the PixelCNN fixture from the reference's own code on the CPU (cflearn/modules/cv/ar/pixel_cnn.py):

    python tools/gen_pixelcnn_golden.py

  tests/golden/pixelcnn_small.pt: "configs", one record for each of
    (a) num_codes = 32, latent_channels = 32, num_layers = 3, the default channel padding;
    (b) as (a) with need_embedding = True, num_classes = 4;
    (c) latent_channels = 64, num_layers = 2, norm_type = None, channel_padding = None
  holding: `kwargs`; `state`, the (name, shape) of every entry of the reference's state dict, in order; `seed` of the parameters
  (tests/pixelcnn_weights.fill_parameters rebuilds them, BatchNorm's running statistics included); `codes` int64 [2, 1, 9, 11] and
  `labels` (None when unconditional); `dy`, the gradient of the logits; `eval_logits` and `train_logits`, fp32 [2, K, 9, 11];
  `grads`: per parameter name the gradient of sum(train logits * dy) at the flat positions `pixelcnn_weights.grad_positions(numel)`;
  and the reference's own rel-L2 distance under torch.autocast("cpu", bfloat16) from each of those: `eval_dist`, `train_dist`,
  `grad_dist` per name.  The distance of a masked filter's gradient is taken over the kept positions that fall on LIVE taps: on the
  masked ones the reference hands back values that never reach the function, this package zeros.

ASSERTED here: every logit distance is at least 1e-3 (the yardstick of the module and sampler tests is not vacuous).

Needs the reference tree (oracle/refharness finds it); writes data only.  Single-threaded and seeded: a second run writes the same values."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from refharness import import_cflearn  # noqa: E402
from pixelcnn_weights import fill_parameters, grad_positions  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 7411
SHAPE = (2, 1, 9, 11)
CONFIGS = [
    ("plain", dict(num_codes=32, in_channels=1, latent_channels=32, num_layers=3)),
    ("embedding_conditional", dict(num_codes=32, in_channels=1, latent_channels=32, num_layers=3, need_embedding=True, num_classes=4)),
    ("no_norm_no_padding", dict(num_codes=32, in_channels=1, latent_channels=64, num_layers=2, norm_type=None, channel_padding=None)),
]
MIN_BF16_REL = 1e-3


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run(net, codes, labels, dy, autocast, train):
    """(logits, {name: grad}) — gradients only in training mode.  The running statistics a training forward moves are put back."""
    buffers = {k: v.clone() for k, v in net.named_buffers()}
    net.train(train)
    net.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast), torch.set_grad_enabled(train):
        y = net(codes, labels)
    grads = {}
    if train:
        (y.float() * dy).sum().backward()
        grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    with torch.no_grad():
        for k, v in net.named_buffers():
            v.copy_(buffers[k])
    return y.detach().float().clone(), grads


def config_fixture(mod, index, name, kw):
    seed = SEED + index
    net = mod.PixelCNN(**kw)
    state = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    fill_parameters(net, seed)
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, kw["num_codes"], SHAPE, generator=gen)
    labels = torch.randint(0, kw["num_classes"], (SHAPE[0],), generator=gen) if kw.get("num_classes") else None
    dy = torch.randn((SHAPE[0], kw["num_codes"], *SHAPE[2:]), generator=gen)
    ev, _ = run(net, codes, labels, dy, False, False)
    ev16, _ = run(net, codes, labels, dy, True, False)
    tr, grads = run(net, codes, labels, dy, False, True)
    tr16, grads16 = run(net, codes, labels, dy, True, True)
    eval_dist, train_dist = rel_l2(ev16, ev), rel_l2(tr16, tr)
    assert eval_dist >= MIN_BF16_REL and train_dist >= MIN_BF16_REL, (name, eval_dist, train_dist)
    masks = {k[:-len("mask")] + "weight": v.reshape(-1) for k, v in net.named_buffers() if k.endswith(".mask")}
    kept, grad_dist = {}, {}
    for k, g in grads.items():
        pos = grad_positions(g.numel())
        a, b = grads16[k].reshape(-1)[pos], g.reshape(-1)[pos]
        kept[k] = b.clone()
        if k in masks:
            live = masks[k][pos] != 0
            a, b = a[live], b[live]
        grad_dist[k] = rel_l2(a, b)
    return dict(name=name, kwargs=kw, state=state, seed=seed, codes=codes, labels=labels, dy=dy, eval_logits=ev, train_logits=tr,
                grads=kept, eval_dist=eval_dist, train_dist=train_dist, grad_dist=grad_dist)


def generate():
    torch.set_num_threads(1)
    import_cflearn()
    mod = importlib.import_module("cflearn.modules.cv.ar.pixel_cnn")
    return dict(configs=[config_fixture(mod, i, name, kw) for i, (name, kw) in enumerate(CONFIGS)])


def main() -> None:
    data = generate()
    path = os.path.join(GOLDEN, "pixelcnn_small.pt")
    torch.save(data, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for rec in data["configs"]:
        gd = rec["grad_dist"]
        print(f"  {rec['name']}: eval logits std {float(rec['eval_logits'].std()):.3f}, eval_dist {rec['eval_dist']:.3e}, train_dist "
              f"{rec['train_dist']:.3e}, grad_dist {min(gd.values()):.3e} .. {max(gd.values()):.3e}")


if __name__ == "__main__":
    main()
