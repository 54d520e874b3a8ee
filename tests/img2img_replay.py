"""The numpy f32 replica of the sampler step WITH A REFERENCE (csrc/sample.hip: the merge of merge_ref inside the ddim / basic
step launch and on its own, the merged `denoised` of the K rules), in the kernel's operation order, and the step records of
tests/golden/img2img_samplers.pt decoded with it: every image the reference produced (tools/gen_img2img_golden.py stored the
SHA-256 of its f32 bytes) is rebuilt from `step_z` and checked bit for bit.  numpy f32: one IEEE rounding per operation whatever
the host's vector units."""
import numpy as np
import torch

from k_sampler_replay import COL, EVALS_PER_STEP
from sampler_replay import guided, sha256, step_formula

ONE = np.float32(1.0)
K_KINDS = ("k_euler_a", "k_heun", "k_dpmpp_2m")


def merge_formula(x, ref, mask, w_net, w_noise, nz):
    """merge_ref (basic.py:33-34 over DDPMQSampler.q_sample): mask * (w_net * ref + w_noise * nz) + (1 - mask) * x; the mask
    broadcasts as it stands ([B or 1, 1 or C, H, W])"""
    noisy = np.float32(w_net) * ref + np.float32(w_noise) * nz
    y = mask * noisy + (ONE - mask) * x
    assert y.dtype == np.float32
    return y


def clamp(x):
    """torch.clip(x, -1, 1) the kernel's way: NaN stays NaN"""
    return np.where(x < -ONE, -ONE, np.where(x > ONE, ONE, x)).astype(np.float32)


def k_eval_ref_formula(kind, par, row, x, aux, m, xi, ref=None, mask=None):
    """k_sampler_replay.k_eval_formula with get_denoised_with_reference (k_samplers.py:185-190): denoised = mask * ref +
    (1 - mask) * denoised -> (x, aux, next input, the merged denoised)"""
    c = {n: np.float32(row[i]) for n, i in COL.items()}
    flag = c["flag"] != 0
    img = x + aux * c["dt"] if kind == "k_heun" and flag else x
    den = img * c["c_skip"] - m * c["c_out"] if par == "v" else img - m * c["c_out"]
    if ref is not None:
        den = mask * ref + (ONE - mask) * den
    den = den.astype(np.float32)
    if kind == "k_euler_a":
        d = (img - den) / c["sigma"]
        y = img + d * c["dt"]
        if flag:
            y = y + xi * c["sigma_up"]
        return y, aux, y, den
    if kind == "k_heun":
        d = (img - den) / c["sigma"]
        if not flag:
            return x, d, x + d * c["dt"], den
        y = x + ((aux + d) / np.float32(2.0)) * c["dt"]
        return y, aux, y, den
    dd = c["r_plus"] * den - c["r_minus"] * aux if flag else den
    y = c["sigma_ratio"] * img - c["expm1_neg_h"] * dd
    return y, den, y, den


def record_operands(fx, r):
    """(ref, mask, unified reference noise) of a record as numpy arrays, or (None, None, None)"""
    if r["mask"] is None:
        return None, None, None
    return fx["step_ref"].numpy(), fx["step_masks"][r["mask"]].numpy(), fx["step_ref_noise"].numpy()


def decode(fx, r) -> dict:
    """One step record rebuilt with the replica, every image checked against the reference's hash.  Per executed launch j (row
    row0 + j of the full table):  outputs[j] [G B, ...], step_noise[j] / merge_noise[j] (the draws, where there are any),
    pre[j] / pre_aux[j]: x and aux in front of the launch, post[j] / post_aux[j] / nexts[j]: what it leaves (`nexts`: the image of
    the next model evaluation, before c_in), images: the reference's images (in front of the run, after every executed step)."""
    kind, par, start, steps = r["kind"], r["parameterization"], r["start_step"], r["steps"]
    ref, mask, unified_noise = record_operands(fx, r)
    outputs = (r["outputs_q"].float() * r["outputs_scale"]).numpy()
    draws = iter((r["draws_q"].float() * r["draws_scale"]).numpy()) if "draws_q" in r else iter(())
    z = fx["step_z"].numpy().copy()
    images, pre, post, pre_aux, post_aux, nexts, step_noise, merge_noise, dens = [z], [], [], [], [], [], [], [], []
    table = r["table"].numpy()
    if kind not in K_KINDS:
        side = r["side"].numpy()
        launches = steps - start
        assert table.shape[0] == launches == outputs.shape[0]

        def merge_draw():
            return unified_noise if r["unified"] else next(draws)

        x = z
        first_merge_noise = None
        if ref is not None:  # the stand-alone merge in front of the first executed step
            first_merge_noise = merge_draw()
            x = merge_formula(x, ref, mask, side[0, 0], side[0, 1], first_merge_noise)
        for j in range(launches):
            xi = next(draws)
            last = j == launches - 1
            # (the reference's order of draws: this step's noise, then — at the top of the next step — that step's merge noise)
            y = step_formula(kind, par, table[j], x, guided(r, outputs[j]), xi, r["temperature"])
            assert y.dtype == np.float32
            images.append(y)
            left, nz = y, None
            if ref is not None and not last:
                nz = merge_draw()
                left = merge_formula(y, ref, mask, side[j + 1, 0], side[j + 1, 1], nz)
            pre.append(x)
            post.append(left)
            nexts.append(left)
            step_noise.append(xi)
            merge_noise.append(nz)
            x = left
        extra = dict(side=r["side"].clone(), first_merge_noise=first_merge_noise, row0=start)
    else:
        per = EVALS_PER_STEP[kind]
        row0 = start * per
        x = z * np.float32(r["sigmas"][0].item()) if start == 0 else z  # `image * self.sigmas[0]`: at step 0 only
        aux = np.zeros_like(x)
        assert table.shape[0] - row0 == outputs.shape[0]
        for j, e in enumerate(range(row0, table.shape[0])):
            xi = None
            if kind == "k_euler_a" or (kind == "k_heun" and table[e, COL["flag"]] == 0):
                xi = next(draws)  # (k_heun draws once per step and never uses it)
            pre.append(x)
            pre_aux.append(aux)
            x, aux, nxt, den = k_eval_ref_formula(kind, par, table[e], x, aux, guided(r, outputs[j]), xi, ref, mask)
            assert x.dtype == aux.dtype == nxt.dtype == np.float32
            post.append(x)
            post_aux.append(aux)
            nexts.append(nxt)
            dens.append(den)
            step_noise.append(xi)
            if (j + 1) % per == 0:
                images.append(x)
        images.append(x)  # the last step returns the image as it is (k_samplers.py:149-150)
        extra = dict(row0=row0)
    assert next(draws, None) is None, "the record holds draws the replica did not consume"
    assert len(images) == steps - start + 1 == len(r["image_sha256"])
    for k, im in enumerate(images):
        assert sha256(torch.from_numpy(np.ascontiguousarray(im))) == r["image_sha256"][k], \
            f"{kind} {par} start {start} mask {r['mask']} scale {r['scale']}: image {k} is not the reference's"
    return dict(table=r["table"].clone(), outputs=outputs, images=images, pre=pre, post=post, pre_aux=pre_aux, post_aux=post_aux,
                nexts=nexts, step_noise=step_noise, merge_noise=merge_noise, denoised=dens, ref=ref, mask=mask, **extra)


def record_id(r) -> str:
    return f"{r['kind']}-{r['parameterization']}-s{r['start_step']}-{r['mask'] or 'noref'}-{'g' if r['scale'] is not None else 'u'}"
