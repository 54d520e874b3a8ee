"""The step records of tests/golden/ddpm_samplers.pt, decoded: the model outputs and noises from their int8 codes, and the
reference's intermediate images rebuilt from `step_z` and the reference's per-step scalars (`table`) with the step kernel's
operation order, each one checked bit for bit against the SHA-256 the generator (tools/gen_sampler_golden.py) stored for the
reference's own image.  The rebuild runs in numpy f32: one IEEE rounding per operation whatever the host's vector units."""
import hashlib

import numpy as np
import torch

from cflearn_amd import ops


def sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def step_formula(kind, par, row, x, m, xi, temperature):
    """the step kernel's per-element arithmetic (csrc/sample.hip), in its order, on numpy f32 arrays"""
    c = [np.float32(row[i]) for i in range(ops.SAMPLE_ROW)]
    temperature = np.float32(temperature)
    if kind == "ddim":
        if par == "v":
            eps, x0 = c[6] * m + c[7] * x, c[6] * x - c[7] * m
        else:
            eps = m
            x0 = (x - c[2] * eps) / c[1]
        return c[3] * x0 + c[4] * eps + c[5] * xi * temperature
    mean = m if par == "x0" else c[1] * (x - c[2] * m)
    return mean + c[3] * (xi * temperature)


def guided(r, out):
    """the model output the step sees: out, or out_u + s (out_c - out_u) of a [2B] output (schema.py:263)"""
    if r["scale"] is None:
        return out
    b = out.shape[0] // 2
    return out[b:] + np.float32(r["scale"]) * (out[:b] - out[b:])


def decode(fx, r) -> dict:
    """{table, outputs [steps, G B, ...], noises [steps, B, ...], images [steps + 1, B, ...]} of one record"""
    table = r["table"].numpy()
    outputs = r["outputs_q"].float() * r["outputs_scale"]
    noises = r["noises_q"].float() * r["noises_scale"]
    images = [fx["step_z"].numpy().copy()]
    for k in range(r["steps"]):
        y = step_formula(r["kind"], r["parameterization"], table[k], images[k], guided(r, outputs[k].numpy()),
                         noises[k].numpy(), r["temperature"])
        assert y.dtype == np.float32
        images.append(y)
    for k, im in enumerate(images):
        assert sha256(torch.from_numpy(im)) == r["image_sha256"][k], \
            f"{r['kind']} {r['parameterization']} scale {r['scale']}: image {k} is not the reference's"
    return dict(table=r["table"].clone(), outputs=outputs, noises=noises, images=torch.from_numpy(np.stack(images)))
