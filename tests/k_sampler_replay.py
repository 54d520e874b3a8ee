"""The step records of tests/golden/k_samplers.pt, decoded: the model outputs and noises from their int8 codes, and the
reference's intermediate images rebuilt from `step_z` and the reference's per-evaluation scalars (`table`) with the K step
kernel's operation order (csrc/sample.hip: k_sample_step_kernel), each step's image checked bit for bit against the SHA-256 the
generator (tools/gen_k_sampler_golden.py) stored for the reference's own.  The rebuild runs in numpy f32: one IEEE rounding per
operation whatever the host's vector units."""
import numpy as np
import torch

from sampler_replay import guided, sha256

COL = {n: i for i, n in enumerate(("t", "sigma", "c_out", "c_skip", "c_in_next", "dt", "sigma_up", "sigma_ratio", "expm1_neg_h",
                                   "r_plus", "r_minus", "flag"))}
EVALS_PER_STEP = {"k_euler_a": 1, "k_heun": 2, "k_dpmpp_2m": 1}


def k_eval_formula(kind, par, row, x, aux, m, xi):
    """one model evaluation, per element, in the kernel's order on numpy f32 arrays -> (x, aux, next input): `aux` is heun's d /
    dpmpp_2m's old_denoised (returned as it came where the kernel does not write it), `next input` the image the next
    evaluation's UNet input is made of (xin = bf16(next input * c_in_next))"""
    c = {n: np.float32(row[i]) for n, i in COL.items()}
    flag = c["flag"] != 0
    img = x + aux * c["dt"] if kind == "k_heun" and flag else x
    den = img * c["c_skip"] - m * c["c_out"] if par == "v" else img - m * c["c_out"]
    if kind == "k_euler_a":
        d = (img - den) / c["sigma"]
        y = img + d * c["dt"]
        if flag:
            y = y + xi * c["sigma_up"]
        return y, aux, y
    if kind == "k_heun":
        d = (img - den) / c["sigma"]
        if not flag:
            return x, d, x + d * c["dt"]
        y = x + ((aux + d) / np.float32(2.0)) * c["dt"]
        return y, aux, y
    dd = c["r_plus"] * den - c["r_minus"] * aux if flag else den
    y = c["sigma_ratio"] * img - c["expm1_neg_h"] * dd
    return y, den, y


def decode(fx, r) -> dict:
    """{table, outputs [evals, G B, ...], noises [evals, B, ...] | None, images [steps + 1, ...] (after each reference step),
    states / auxs [evals + 1, ...] (x and aux in front of each evaluation and after the last), nexts [evals, ...]} of one record"""
    table = r["table"].numpy()
    outputs = r["outputs_q"].float() * r["outputs_scale"]
    noises = r["noises_q"].float() * r["noises_scale"] if "noises_q" in r else None
    z = fx["step_z"].numpy().copy()
    x = z * np.float32(r["sigmas"][0].item())  # `image * self.sigmas[0]`
    aux = np.zeros_like(x)
    states, auxs, nexts, images = [x], [aux], [], [z]
    per = EVALS_PER_STEP[r["kind"]]
    for e in range(table.shape[0]):
        xi = None if noises is None else noises[e].numpy()
        x, aux, nxt = k_eval_formula(r["kind"], r["parameterization"], table[e], x, aux, guided(r, outputs[e].numpy()), xi)
        assert x.dtype == aux.dtype == nxt.dtype == np.float32
        states.append(x)
        auxs.append(aux)
        nexts.append(nxt)
        if (e + 1) % per == 0:
            images.append(x)
    images.append(x)  # the last step returns the image as it is (k_samplers.py:149-150)
    assert len(images) == r["steps"] + 1 == len(r["image_sha256"])
    for k, im in enumerate(images):
        assert sha256(torch.from_numpy(im)) == r["image_sha256"][k], \
            f"{r['kind']} {r['parameterization']} scale {r['scale']}: image {k} is not the reference's"
    st = lambda a: torch.from_numpy(np.stack(a))  # noqa: E731
    return dict(table=r["table"].clone(), outputs=outputs, noises=noises, images=st(images), states=st(states), auxs=st(auxs),
                nexts=st(nexts))
