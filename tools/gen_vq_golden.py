"""Generate the fixtures of the VQ-autoencoder first stage from the reference's own classes on the CPU:

    python tools/gen_vq_golden.py

  tests/golden/ae_vq_keys.pt    state-dict names and shapes of the small `ae_vq` (names and shapes only)
  tests/golden/ae_vq_small.pt   two records of the reference's `ae_vq` (cv/ae/vq.py) on one input [2, 3, 16, 16]:
                                "e4": the KL fixture's SMALL configuration (tools/gen_first_stage_golden.py) plus num_codes 64,
                                      embedding_channels 4;
                                "e3": the same with embedding_channels 3 and latent_channels 3, the form of the zoo's ae/vq.f4.
                                Each holds z_e (the `to_embedding` output), indices, z_q, decoded = decode(z_q) and z_q_g =
                                embedding.weight[indices].view_as(z_e), from the fp32 run (`*`) and from the reference's own run
                                under `torch.autocast("cpu", dtype=torch.bfloat16)` (`*_bf16`), and flips_bf16: the number of
                                pixels where those two runs chose different codes — the yardstick of the HIP path's own flips.

Needs the reference tree (oracle/refharness finds it); writes data only.  No fixture stores parameters: every model is filled by
`seeded_state` of tools/gen_first_stage_golden.py (1-D `weight`s 1 + 0.1 n, other 1-D tensors 0.1 n, filters n / sqrt(fan_in), in
the sorted order of the names from one CPU generator), which the tests repeat.  The codebook `codebook.embedding.weight` is a 2-D
tensor [num_codes, D] and so falls under the filter rule: n / sqrt(D).  Single-threaded and seeded: a second run writes the same
values.  `generate()` returns the fixtures in memory (tests/test_vq_host.py compares them with the committed files).

Seeds.  The parameter seed of a record is chosen so that 1 <= flips_bf16 <= 5 % of the 128 pixels (6): a fixture whose two runs
agree everywhere could not tell a path that flips nothing from one that is never compared.  The input always comes from
seed + 1.  Seeds tried (SEED_TRIALS below, seed -> flip count): 1701 was the first tried for both records and gave 2 flips
("e4") and 6 flips ("e3") of 128 pixels, both inside [1, 6]; no other seed was tried.  `--search` repeats the search."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from refharness import import_cflearn  # noqa: E402
from gen_first_stage_golden import SMALL, _both, _fill  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIGS = {
    "e4": dict(SMALL, num_codes=64, embedding_channels=4),
    "e3": dict(SMALL, num_codes=64, embedding_channels=3, latent_channels=3),
}
# seed -> flips_bf16 it gave, in the order tried (python tools/gen_vq_golden.py --search prints such a table)
SEED_TRIALS = {"e4": {1701: 2}, "e3": {1701: 6}}
SEEDS = {"e4": 1701, "e3": 1701}


def vq_fixture(cfg, seed):
    import importlib

    vq = importlib.import_module("cflearn.modules.cv.ae.vq")
    common = importlib.import_module("cflearn.modules.cv.common")
    m = vq.AttentionAutoEncoderVQ(**cfg)
    shapes = _fill(m, seed)
    m.eval()
    size = cfg["img_size"]
    x = torch.randn((2, 3, size, size), generator=torch.Generator().manual_seed(seed + 1))

    def run():
        with torch.no_grad():
            out = m.encode(x, return_z_q_g=True)
            return out.z_e, out.indices, out.z_q, m.decode(common.DecoderInputs(z=out.z_q)), out.z_q_g

    full, low = _both(run)
    names = ("z_e", "indices", "z_q", "decoded", "z_q_g")
    rec = dict(cfg=dict(cfg), seed=seed, x=x)
    for name, a, b in zip(names, full, low):
        if name == "indices":  # (_both stores floats; the indices are small integers, exact in f32)
            a, b = a.long(), b.long()
        rec[name], rec[name + "_bf16"] = a, b
    rec["flips_bf16"] = int((rec["indices"] != rec["indices_bf16"]).sum())
    return rec, shapes


def generate():
    torch.set_num_threads(1)
    import_cflearn()
    small = {}
    shapes = None
    for key, cfg in CONFIGS.items():
        small[key], sh = vq_fixture(cfg, SEEDS[key])
        if key == "e4":
            shapes = sh
    keys = dict(cfg=dict(CONFIGS["e4"]), keys=[(k, tuple(v)) for k, v in shapes.items()])
    return {"ae_vq_keys.pt": keys, "ae_vq_small.pt": small}


def search(first=1701, tries=12):
    torch.set_num_threads(1)
    import_cflearn()
    for key, cfg in CONFIGS.items():
        for seed in range(first, first + tries):
            rec, _ = vq_fixture(cfg, seed)
            pixels = rec["indices"].numel()
            print(f"{key}: seed {seed} -> flips_bf16 {rec['flips_bf16']} of {pixels}", flush=True)
            if 1 <= rec["flips_bf16"] <= pixels * 5 // 100:
                break


def main() -> None:
    if "--search" in sys.argv:
        return search()
    for name, data in generate().items():
        path = os.path.join(GOLDEN, name)
        torch.save(data, path)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
        if name == "ae_vq_small.pt":
            for key, rec in data.items():
                print(f"  {key}: seed {rec['seed']}, flips_bf16 {rec['flips_bf16']} of {rec['indices'].numel()} pixels")


if __name__ == "__main__":
    main()
