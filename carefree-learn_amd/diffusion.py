"""DDPM training step around `modules.UNetDiffuser` (reference modules/multimodal/diffusion/ddpm.py:51-89,599-640;
samplers/schema.py:90-112; models/cv/diffusion.py:44-94): the float64 beta schedule (host, numpy, bit-exact with the
reference's arithmetic), the forward process `q_sample` and the epsilon-prediction MSE objective as kernels, and a
step engine on the flat arena + fused Adam like `engine.TrainStep`.

Every objective of `DDPMStep.loss_fn` is built: parameterization "eps" / "x0" / "v", loss "l2" / "l1", a fixed or learned
per-timestep `log_var`, `l_simple_weight` and the `original_elbo_weight * lvlb_weights[t]` term; the zoo `diffusion/ddpm`
defaults are eps / l2 / log_var 0 / weights 1 and 0.

Latent diffusion (multimodal/diffusion/ldm.py:154-202): with a frozen `first_stage` (modules.AttentionAutoEncoderKL) the train step
takes images, encodes them and draws the scaled latent in one posterior kernel (`LDM.preprocess`), and the sampler decodes the
latent it ends with (`LDM.decode`).  With modules.AttentionAutoEncoderVQ the scaled latent comes out of the one nearest-code launch.

Sampling (`make_sampler`): the reference's `ddim` and `basic` samplers (`DiffusionSampler`) and its sigma-space `k_euler_a`, `k_heun`
and `k_dpmpp_2m` (`KDiffusionSampler`, samplers/k_samplers.py), each one fused kernel launch and one counter launch per model
evaluation on per-evaluation scalars formed here, on the host, with the reference's f32 operations.  Image-to-image and
inpainting (`ISampler.sample`'s ref / ref_mask / ref_noise / start_step; the API's `_q_sample`, `_img2img`, raw inpainting):
`sample_with_reference`, `img2img`, `inpaint` of every sampler, the merge inside the same step launch."""
import contextlib
import math
from typing import Any, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import functional as HF
from . import ops
from .functional import SideStream
from .optim import FusedAdam, ParamArena


class NoiseSchedule:
    """`make_beta_schedule` + `_register_noise_schedule` (ddpm.py:51-89,599-640): float64 on the host, fp32 buffers"""

    def __init__(self, timesteps: int = 1000, beta_schedule: str = "linear", linear_start: float = 8.5e-4,
                 linear_end: float = 1.2e-2, device: Any = "cpu", *, cosine_s: float = 8.0e-3,
                 given_betas: Optional[np.ndarray] = None, parameterization: str = "eps", v_posterior: float = 0.0):
        if given_betas is not None:
            betas = np.asarray(given_betas, dtype=np.float64)
            timesteps = len(betas)
        elif beta_schedule == "linear":
            betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
        elif beta_schedule == "cosine":
            steps = np.arange(timesteps + 1, dtype=np.float64) / timesteps + cosine_s
            alphas_c = np.cos(steps / (1 + cosine_s) * np.pi / 2) ** 2
            alphas_c = alphas_c / alphas_c[0]
            betas = np.clip(1.0 - alphas_c[1:] / alphas_c[:-1], 0.0, 0.999)
        elif beta_schedule == "sqrt_linear":
            betas = np.linspace(linear_start, linear_end, timesteps, dtype=np.float64)
        elif beta_schedule == "sqrt":
            betas = np.linspace(linear_start, linear_end, timesteps, dtype=np.float64) ** 0.5
        else:
            raise ValueError(f"unrecognized schedule '{beta_schedule}' occurred")
        if parameterization not in ("eps", "x0", "v"):
            raise NotImplementedError(f"unrecognized parameterization '{parameterization}' occurred")
        alphas = 1.0 - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1.0, alphas_cumprod[:-1])
        one_m_cumprod = 1.0 - alphas_cumprod
        to_t = lambda a: torch.from_numpy(a.astype(np.float32)).to(device)  # noqa: E731  (cftool.array.to_torch)
        self.t = timesteps
        self.parameterization = parameterization
        self.betas = to_t(betas)
        self.alphas_cumprod = to_t(alphas_cumprod)
        self.sqrt_alphas_cumprod = to_t(np.sqrt(alphas_cumprod))
        self.sqrt_one_minus_alphas_cumprod = to_t(np.sqrt(one_m_cumprod))
        self.neg_sqrt_one_minus_alphas_cumprod = -self.sqrt_one_minus_alphas_cumprod
        # q(x_{t-1} | x_t, x_0) and the variational-bound weights (ddpm.py:636-679): the reference forms them from the
        # fp32 buffers with torch arithmetic — same operations, same order, here
        posterior_variance64 = v_posterior * betas + (1.0 - v_posterior) * betas * (1.0 - alphas_cumprod_prev) / one_m_cumprod
        posterior_variance = to_t(posterior_variance64)
        self.posterior_variance = posterior_variance
        # the rest of `_register_noise_schedule` (ddpm.py:611,630-635): what the reverse process reads
        self.alphas_cumprod_prev = to_t(alphas_cumprod_prev)
        self.posterior_log_variance_clipped = to_t(np.log(np.maximum(posterior_variance64, 1e-20)))
        self.posterior_coef1 = to_t(1.0 / np.sqrt(alphas))
        self.posterior_coef2 = to_t((1.0 - alphas) / np.sqrt(one_m_cumprod))
        if parameterization == "eps":
            lvlb = 0.5 * self.betas ** 2 / (posterior_variance * to_t(alphas) * (1.0 - self.alphas_cumprod))
        elif parameterization == "x0":
            lvlb = to_t(0.25 * np.sqrt(alphas_cumprod) / one_m_cumprod)
        else:
            lvlb = torch.ones_like(self.betas ** 2 / (2 * posterior_variance * to_t(alphas) * (1.0 - self.alphas_cumprod)))
        lvlb[0] = lvlb[1]
        self.lvlb_weights = lvlb

    def q_sample(self, x: Tensor, timesteps: Tensor, noise: Tensor, out_dtype: torch.dtype = torch.float32) -> Tensor:
        return ops.q_sample(x.float(), noise.float(), timesteps, self.sqrt_alphas_cumprod,
                            self.sqrt_one_minus_alphas_cumprod, out_dtype)

    def v_target(self, x: Tensor, timesteps: Tensor, noise: Tensor) -> Tensor:
        """`DDPMStep.get_v` (models/cv/diffusion.py:96-101): sqrt(ac[t]) noise - sqrt(1 - ac[t]) x, the same kernel as
        q_sample with the operands' roles exchanged"""
        return ops.q_sample(noise.float(), x.float(), timesteps, self.sqrt_alphas_cumprod,
                            self.neg_sqrt_one_minus_alphas_cumprod, torch.float32)


class DDPMTrainStep:
    """One optimisation step of `DDPMStep.loss_fn` (models/cv/diffusion.py:44-94): x_t = q_sample(x, t, noise);
    out = unet(x_t, t, context); target = noise | x | v by `parameterization`; per sample loss_b = mean_chw f(out - target)
    (f = square | abs); loss = l_simple_weight * mean_b(loss_b / exp(log_var[t_b]) + log_var[t_b]) +
    original_elbo_weight * mean_b(lvlb_weights[t_b] * loss_b); backward; fused AdamW over the arena.  `log_var` is a
    per-timestep table (`log_var_init`), a trained parameter of the arena with `learn_log_var`.  `t` and `noise` are
    drawn on the device when not given (torch's generator: input sampling, not part of the arithmetic path).

    `first_stage` (an `AttentionAutoEncoderKL`; reference LDM, ldm.py:154-190): `step(x)` then takes IMAGES.  Inside the step's body
    (so inside the recorded graph with `use_graph`) the first stage encodes them in eval mode under no_grad and the posterior kernel
    draws `first_stage_scale_factor * sample` (or, with `deterministic=True`, `* mode`) into the f32 latent the rest of the step
    takes.  The normals of step k are the Philox stream at (seed, k * ceil(latent elements / 4)) — `latent_draw(k)` —, `seed` being
    `step(seed=...)` or `first_stage_seed`: different per step, reproducible with `ops.gaussian_posterior` / `ops.randn`.  The first
    stage is frozen as the reference's `to_eval` freezes it (eval mode, requires_grad off): its parameters are outside the arena,
    get no gradient and are never updated.  `timesteps` and `noise` then have the latent's batch and shape.

    With an `AttentionAutoEncoderVQ` first stage (LDM.preprocess's other branch, ldm.py:183-190) the latent is
    `first_stage_scale_factor * z_q` of `first_stage.encode(x, return_z_q_g=False)`, scaled inside the one nearest-code launch
    (`cfhip_vq_nearest`).  Nothing is drawn: `deterministic` and `seed` are accepted and change nothing, no normals are generated
    in front of a recorded graph, and `steps_done` counts as before."""

    def __init__(self, unet: torch.nn.Module, schedule: Optional[NoiseSchedule] = None, *, lr: float = 1.0e-4,
                 betas: Any = (0.9, 0.999), eps: float = 1.0e-8, weight_decay: float = 0.0, decoupled: bool = True,
                 distributed: bool = False, bucket_bytes: int = 256 << 20, loss_type: str = "l2",
                 l_simple_weight: float = 1.0, original_elbo_weight: float = 0.0, learn_log_var: bool = False,
                 log_var_init: float = 0.0, use_graph: bool = False, step_in_backward: bool = True,
                 range_bytes: int = 64 << 20, first_stage: Optional[torch.nn.Module] = None, first_stage_scale_factor: float = 1.0,
                 first_stage_seed: int = 0):
        if loss_type not in ("l1", "l2"):
            raise ValueError(f"unrecognized loss '{loss_type}' occurred")
        self.unet = unet
        self.first_stage = first_stage
        self.first_stage_scale_factor = float(first_stage_scale_factor)
        self.first_stage_seed = int(first_stage_seed)
        self.steps_done = 0  # the counter the posterior draws follow
        self._draw: Tuple[int, int, bool] = (0, 0, False)
        self._vq = False
        if first_stage is not None:  # `to_eval` (ldm.py:157)
            from .modules import AttentionAutoEncoderVQ

            self._vq = isinstance(first_stage, AttentionAutoEncoderVQ)
            first_stage.eval()
            for p in first_stage.parameters():
                p.requires_grad_(False)
        params = [p for p in unet.parameters() if p.requires_grad]
        dev = params[0].device
        self.schedule = schedule or NoiseSchedule(device=dev)
        self.loss_type, self.l_simple_weight = loss_type, float(l_simple_weight)
        self.original_elbo_weight = float(original_elbo_weight)
        self.learn_log_var = learn_log_var
        self.log_var = torch.full((self.schedule.t,), float(log_var_init), dtype=torch.float32, device=dev)
        if learn_log_var:  # ddpm.py:231-236: an nn.Parameter trained with the UNet
            self.log_var = torch.nn.Parameter(self.log_var, requires_grad=True)
            params = params + [self.log_var]
        self.arena = ParamArena(params, with_shadow=True)
        self.optimizer = FusedAdam(None, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled,
                                   arena=self.arena)
        self.optimizer.lazy_zero = True
        self.reducer = None
        # the optimizer update inside backward (optim.StepInBackward): 865 M parameters x 30 bytes is 4.5 ms of HBM traffic that
        # used to run alone at the end of a 62 ms step
        in_bwd = bool(step_in_backward) and not use_graph and dev.type == "cuda"
        if distributed:  # 3.46 GB of fp32 gradients per step: 256 MB buckets, overlapped with the backward
            from .ddp import BucketedAllReduce

            self.reducer = BucketedAllReduce(self.arena, bucket_bytes=bucket_bytes, optimizer=self.optimizer, step_in_backward=in_bwd)
            self.reducer.broadcast_parameters(0)
        elif in_bwd:
            self.optimizer.enable_step_in_backward(range_bytes)
        self.loss_sum: Optional[Tensor] = None
        self.losses: dict = {}
        self.use_graph = bool(use_graph) and not distributed
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._static: dict = {}
        self._graph_loss: Optional[Tensor] = None

    def target(self, x: Tensor, timesteps: Tensor, noise: Tensor) -> Tensor:
        p = self.schedule.parameterization
        if p == "eps":
            return noise.float()
        if p == "x0":
            return x.float()
        return self.schedule.v_target(x, timesteps, noise)

    def objective(self, pred: Tensor, target: Tensor, timesteps: Tensor, want_grad: bool = True):
        """Returns (loss f32 scalar tensor, dpred bf16, dict of the reference's loss entries as device tensors);
        writes the gradient of a learned `log_var`."""
        from .functional import write_param_grad

        b = pred.shape[0]
        log_var_t = self.log_var.detach()[timesteps]
        inv = torch.exp(-log_var_t)
        weight = self.l_simple_weight * inv / b
        if self.original_elbo_weight > 0:
            weight = weight + self.original_elbo_weight * self.schedule.lvlb_weights[timesteps] / b
        per_sample, dpred = ops.diffusion_loss(pred, target, weight.float().contiguous(), self.loss_type, want_grad)
        loss_simple = per_sample / torch.exp(log_var_t) + log_var_t
        losses = {"simple": per_sample.mean()}
        if self.learn_log_var:
            losses["gamma"] = loss_simple.mean()
            losses["log_var"] = self.log_var.detach().mean()
            if want_grad:  # d/d log_var[t_b] of l_simple_weight * mean_b(loss_b exp(-lv) + lv)
                g = self.l_simple_weight * (1.0 - per_sample * inv) / b

                def scatter(out: Tensor, acc: bool) -> None:
                    if not acc:
                        out.zero_()
                    out.index_add_(0, timesteps, g)

                write_param_grad(self.log_var, scatter)
        loss = self.l_simple_weight * loss_simple.mean()
        if self.original_elbo_weight > 0:
            vlb = (self.schedule.lvlb_weights[timesteps] * per_sample).mean()
            losses["vlb"] = vlb
            loss = loss + self.original_elbo_weight * vlb
        losses["loss"] = loss
        return loss, dpred, losses

    def latent_shape(self, x: Tensor) -> Tuple[int, ...]:
        """the latent the first stage makes of the images `x`"""
        fs = self.first_stage
        f = 2 ** (len(fs.channel_multipliers) - 1)
        return (x.shape[0], fs.embedding_channels, x.shape[2] // f, x.shape[3] // f)

    def latent_draw(self, k: int, latent_elements: int, seed: Optional[int] = None) -> Tuple[int, int]:
        """(seed, offset) of the posterior normals of step k (k = 0 for the first `step` call)"""
        return (self.first_stage_seed if seed is None else int(seed)), int(k) * ((int(latent_elements) + 3) // 4)

    def encode(self, x: Tensor, *, seed: int = 0, offset: int = 0, noise: Optional[Tensor] = None, deterministic: bool = False) -> Tensor:
        """`LDM.preprocess` (ldm.py:183-190): images -> the scaled f32 latent, first stage in eval mode under no_grad"""
        with torch.no_grad():
            if self._vq:  # (vq.py:63-67: no posterior, so no draw; the scale rides in the lookup launch)
                return self.first_stage.encode(x, return_z_q_g=False, scale_factor=self.first_stage_scale_factor).z_q
            dist = self.first_stage.encode(x)
            return ops.gaussian_posterior(dist.net, scale_factor=self.first_stage_scale_factor, seed=seed, offset=offset, noise=noise,
                                          deterministic=deterministic)[0]

    def step(self, x: Tensor, context: Optional[Tensor] = None, *, timesteps: Optional[Tensor] = None,
             noise: Optional[Tensor] = None, labels: Optional[Tensor] = None, deterministic: bool = False,
             seed: Optional[int] = None) -> Tensor:
        """Returns the device tensor holding the loss of this step (`self.losses`: the reference's other entries).  With a first
        stage `x` holds images; `deterministic` takes the posterior's mode, `seed` names the stream of its draw."""
        b = x.shape[0]
        shape = x.shape if self.first_stage is None else self.latent_shape(x)
        if timesteps is None:
            timesteps = torch.randint(0, self.schedule.t, (b,), device=x.device, dtype=torch.int64)
        if noise is None:
            noise = torch.randn(shape, device=x.device, dtype=torch.float32)
        fs_noise = None
        if self.first_stage is not None:
            n = int(np.prod(shape))
            self._draw = (*self.latent_draw(self.steps_done, n, seed), bool(deterministic))
            if self.use_graph and not deterministic and not self._vq:
                # a recorded launch replays its arguments: the step's normals are drawn here, in front of the graph, from the same
                # stream, and the posterior kernel inside it reads them (bit-equal to drawing them itself)
                fs_noise = ops.randn(n, self._draw[0], self._draw[1], x.device).view(shape)
        elif deterministic or seed is not None:
            raise ValueError("DDPMTrainStep: `deterministic` / `seed` belong to a first stage; this step has none")
        self.steps_done += 1
        if self.use_graph:
            return self._graph_step(x, context, timesteps, noise, labels, fs_noise)
        self.optimizer.prepare_step()
        return self._body(x, context, timesteps, noise, labels)

    def _body(self, x: Tensor, context: Optional[Tensor], timesteps: Tensor, noise: Tensor, labels: Optional[Tensor],
              fs_noise: Optional[Tensor] = None) -> Tensor:
        """All device work of one step, no host synchronisation (what a hipGraph records)."""
        b = x.shape[0]
        self.optimizer.zero_grad()
        if self.first_stage is not None:
            seed, offset, deterministic = self._draw
            x = self.encode(x, seed=seed, offset=offset, noise=fs_noise, deterministic=deterministic)
        x_t = self.schedule.q_sample(x, timesteps, noise, torch.bfloat16)
        pred = self._predict(x_t, timesteps, context, {} if labels is None else {"labels": labels})
        loss, dpred, self.losses = self.objective(pred, self.target(x, timesteps, noise), timesteps)
        self.loss_sum = loss * b  # (round-1 name: sum over the batch of the per-sample objective)
        pred.backward(dpred)
        SideStream.join()
        if self.reducer is not None:
            self.reducer.finish()
        self.optimizer.launch_step()
        return loss

    def _predict(self, x_t: Tensor, timesteps: Tensor, context: Optional[Tensor], kw: dict) -> Tensor:
        """the model's prediction for x_t (what the objective differentiates)"""
        return self.unet(x_t, timesteps=timesteps, context=context, **kw)

    def _graph_step(self, x: Tensor, context: Optional[Tensor], timesteps: Tensor, noise: Tensor,
                    labels: Optional[Tensor], fs_noise: Optional[Tensor] = None) -> Tensor:
        """`use_graph`: the step is recorded ONCE into a hipGraph (after two eager passes for the allocator, the side streams
        and the lazy initialisations, whose updates are rolled back) and replayed; the ~2 900 launches of a UNet step then cost the host one call (the eager step at
        64^2 x 8 is bound by the host's issue rate: 65 ms of Python per 69 ms step).  Inputs are copied into the recorded
        buffers; shapes (and the presence of context / labels) must not change between steps."""
        ins = dict(x=x, context=context, timesteps=timesteps, noise=noise, labels=labels, fs_noise=fs_noise)
        if self._graph is None:
            self._static = {k: (None if v is None else v.clone()) for k, v in ins.items()}
            snap = self.optimizer.snapshot()  # the two warm-up passes below are not training steps
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    self.optimizer.prepare_step()
                    self._body(**self._static)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.optimizer.restore(snap)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):  # records, does not execute: this call goes on to replay it once
                self._graph_loss = self._body(**self._static)
        for k, v in ins.items():
            st = self._static[k]
            if (v is None) != (st is None) or (v is not None and v.shape != st.shape):
                raise ValueError(f"DDPMTrainStep(use_graph=True): '{k}' changed its shape / presence after the recording")
            if v is not None and v.data_ptr() != st.data_ptr():
                st.copy_(v, non_blocking=True)
        self.optimizer.prepare_step()
        self._graph.replay()
        return self._graph_loss.clone()  # (the recorded tensor is overwritten by every replay)


class ControlNetTrainStep(DDPMTrainStep):
    """One optimisation step of a `ControlNet` against a FROZEN UNet (reference ddpm.py:392-459 inside DDPMStep.loss_fn):
    x_t = q_sample(x, t, noise); ctrl = control_net(x_t, hint, t, context) * control_scales; pred = unet(x_t, t, context,
    control=ctrl, only_mid_control=...); the parent's objective; backward; fused AdamW.  The UNet's parameters have requires_grad
    off and stay outside the arena: its backward computes input gradients only (the autograd functions honour needs_input_grad),
    no `.grad` appears on it and nothing updates it.  The arena, the optimizer step inside backward and the bucketed all-reduce
    cover the ControlNet's parameters (and a learned log-variance).  `step(x, hint, context, ...)`: hint [B, hint_channels, 8 H, 8 W].
    Graph capture of this step is not built: there is no `use_graph`."""

    def __init__(self, unet: torch.nn.Module, control_net: torch.nn.Module, schedule: Optional[NoiseSchedule] = None, *,
                 control_scales: Optional[Sequence[float]] = None, only_mid_control: bool = False, **config: Any):
        if "use_graph" in config:
            raise TypeError("ControlNetTrainStep takes no `use_graph`: graph capture of the ControlNet step is not built")
        n = getattr(control_net, "num_control_scales", None)
        if control_scales is not None and n is not None and len(control_scales) != n:
            raise ValueError(f"`control_scales` must hold {n} floats, got {len(control_scales)}")
        for p in unet.parameters():
            p.requires_grad_(False)
        super().__init__(control_net, schedule, **config)
        self.control_net, self.unet = control_net, unet
        self.control_scales = None if control_scales is None else [float(v) for v in control_scales]
        self.only_mid_control = bool(only_mid_control)
        self._hint: Optional[Tensor] = None

    def step(self, x: Tensor, hint: Tensor, context: Optional[Tensor] = None, **kwargs: Any) -> Tensor:  # type: ignore[override]
        """the parent's `step` with the hint of this batch (keywords: timesteps, noise, labels, deterministic, seed)"""
        self._hint = hint
        try:
            return super().step(x, context, **kwargs)
        finally:
            self._hint = None

    def _predict(self, x_t: Tensor, timesteps: Tensor, context: Optional[Tensor], kw: dict) -> Tensor:
        ctrl = self.control_net(x_t, self._hint, timesteps=timesteps, context=context, scales=self.control_scales, **kw)
        return self.unet(x_t, timesteps=timesteps, context=context, control=ctrl, only_mid_control=self.only_mid_control, **kw)


# ---------------------------------------------------------------------------------------------
# Reverse process: DDIM and ancestral ("basic") sampling (reference samplers/ddim.py, basic.py, schema.py:153-263)
# ---------------------------------------------------------------------------------------------

# the reference's other samplers and options: not built here
UNBUILT_SAMPLERS = ("plms", "klms", "k_euler", "k_dpmpp_2m_sde", "solver", "lcm")


def ddim_q_timesteps(total: int, total_step: int, discretize: str = "uniform") -> np.ndarray:
    """`DDIMQSampler.reset_buffers` (ddim.py:37-53): the q-timesteps of a `total_step` run over a `total`-step schedule, with
    the reference's quirks (`uniform` yields one more entry than `total_step`; `quad` can repeat timesteps)"""
    if not 0 < total_step <= total:
        raise ValueError(f"num_steps must lie in [1, {total}], got {total_step}")
    if discretize == "uniform":
        span = total // (total_step + int(total % total_step == 0) - 1)
        q = np.array(list(range(0, total, span)) + [total - 1])
    elif discretize == "quad":
        end = math.sqrt(total * 0.8)
        q = (np.linspace(0, end, total_step) ** 2).astype(int)
    else:
        raise ValueError(f"unrecognized discretize method '{discretize}' occurred")
    q += 1
    return np.minimum(q, total - 1)


def ddim_tables(schedule: NoiseSchedule, total_step: int, discretize: str = "uniform", eta: float = 0.0) -> dict:
    """`DDIMMixin._reset_buffers` (ddim.py:241-268) on the CPU in f32: timesteps, alphas, alphas_prev, sigmas,
    sqrt_one_minus_alphas; index them with t_index = total_step - step - 1"""
    q = ddim_q_timesteps(schedule.t, total_step, discretize)
    alphas = schedule.alphas_cumprod.cpu()
    a = alphas[q]
    a_prev = torch.tensor([float(alphas[0])] + alphas[q[:-1]].tolist(), dtype=alphas.dtype)
    sigmas = eta * torch.sqrt((1.0 - a_prev) / (1.0 - a) * (1.0 - a / a_prev))
    return dict(timesteps=q.tolist(), alphas=a, alphas_prev=a_prev, sigmas=sigmas, sqrt_one_minus_alphas=torch.sqrt(1.0 - a))


def sampler_table(kind: str, schedule: NoiseSchedule, num_steps: int, *, discretize: str = "uniform",
                  eta: float = 0.0) -> Tensor:
    """[num_steps, ops.SAMPLE_ROW] f32 (CPU): row k = the per-step scalars of step k, formed with the reference's f32
    operations in its order (column layout: csrc/sample.hip).  DDIM: t, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev),
    sqrt(1 - a_prev - sigma^2), sigma, sqrt(ac[t]), sqrt(1 - ac[t]) (ddim.py:167-181,195-239); basic (t = num_steps - k - 1,
    basic.py:61-92): t, posterior_coef1[t], posterior_coef2[t], [t > 0] exp(0.5 posterior_log_variance_clipped[t])."""
    rows = torch.zeros((num_steps, ops.SAMPLE_ROW), dtype=torch.float32)
    if kind == "ddim":
        tb = ddim_tables(schedule, num_steps, discretize, eta)
        sac, s1mac = schedule.sqrt_alphas_cumprod.cpu(), schedule.sqrt_one_minus_alphas_cumprod.cpu()
        for k in range(num_steps):
            i = num_steps - k - 1
            t = tb["timesteps"][i]
            at, ap, sg = tb["alphas"][i:i + 1], tb["alphas_prev"][i:i + 1], tb["sigmas"][i:i + 1]
            cols = [torch.tensor([float(t)]), at.sqrt(), tb["sqrt_one_minus_alphas"][i:i + 1], ap.sqrt(),
                    (1.0 - ap - sg ** 2).sqrt(), sg, sac[t:t + 1], s1mac[t:t + 1]]
            rows[k] = torch.cat(cols)
    elif kind == "basic":
        if num_steps > schedule.t:
            raise ValueError(f"num_steps must lie in [1, {schedule.t}], got {num_steps}")
        c1, c2 = schedule.posterior_coef1.cpu(), schedule.posterior_coef2.cpu()
        lv = schedule.posterior_log_variance_clipped.cpu()
        for k in range(num_steps):
            t = num_steps - k - 1
            mask = torch.tensor([0.0 if t == 0 else 1.0])
            rows[k, :4] = torch.cat([torch.tensor([float(t)]), c1[t:t + 1], c2[t:t + 1], mask * (0.5 * lv[t:t + 1]).exp()])
    else:
        raise ValueError(f"unrecognized sampler '{kind}'")
    return rows


def _q_weights(kind: str, schedule: NoiseSchedule, num_steps: int, discretize: str = "uniform") -> Tuple[Tensor, Tensor]:
    """(sqrt_alphas, sqrt_one_minus_alphas) of the sampler's own q-sampler (CPU f32), indexed by its timestep index: DDIMQSampler's
    torch.sqrt(alphas[q]) / torch.sqrt(1 - alphas[q]) (ddim.py:50-53), or the schedule's DDPMQSampler buffers for `basic`"""
    if kind == "ddim":
        a = schedule.alphas_cumprod.cpu()[ddim_q_timesteps(schedule.t, num_steps, discretize)]
        return torch.sqrt(a), torch.sqrt(1.0 - a)
    if kind == "basic":
        if num_steps > schedule.t:
            raise ValueError(f"num_steps must lie in [1, {schedule.t}], got {num_steps}")
        return schedule.sqrt_alphas_cumprod.cpu(), schedule.sqrt_one_minus_alphas_cumprod.cpu()
    raise ValueError(f"unrecognized sampler '{kind}'")


def sampler_side_table(kind: str, schedule: NoiseSchedule, num_steps: int, *, discretize: str = "uniform") -> Tensor:
    """[num_steps, 2] f32 (CPU), the sibling of `sampler_table` for a run with a reference: row k = (w_net, w_noise) of the merge IN
    FRONT OF step k, `q_sample(ref, t_prev = num_steps - k - 1)` of merge_ref (basic.py:29-33) through the sampler's q-sampler."""
    w_net, w_noise = _q_weights(kind, schedule, num_steps, discretize)
    idx = torch.arange(num_steps - 1, -1, -1)
    return torch.stack([w_net[idx], w_noise[idx]], dim=1).to(torch.float32).contiguous()


def sampler_philox_ranges(total: int, rows: int, row0: int = 0) -> dict:
    """The half-open Philox counter ranges [lo, hi) a run on a state of `total` elements (rows = the table's rows, row0 = the first
    one executed) draws from under one seed, as csrc/sample.hip documents them; four normals per counter, total4 = total / 4:
    `start` the starting noise (offset - total4 = 0), `steps[row]` the draw of row `row` (offset + row * total4), `merges[row]` the
    noise of the merge in front of row `row` of a ddim / basic run with a reference (offset + (rows + row) * total4)."""
    total4 = int(total) // 4
    offset = total4
    span = lambda lo: (lo, lo + total4)  # noqa: E731
    return dict(start=span(0), steps={r: span(offset + r * total4) for r in range(row0, rows)},
                merges={r: span(offset + (rows + r) * total4) for r in range(row0, rows)})


class DiffusionSampler:
    """`ISampler.sample` (schema.py:153-195) of the reference's `ddim` / `basic` samplers around the HIP UNet.  Each step is
    three device operations: the UNet forward (no_grad; one 2B-batch forward with [cond; uncond] under classifier-free
    guidance, or two B-batch forwards when the context lengths differ), `cfhip_diffusion_sample_step` (every element-wise
    operation of the step, the guidance mix and the final clamp) and `cfhip_diffusion_sample_advance` (the device step
    counter and the UNet's timesteps).  `use_graph`: the first two steps run eagerly (they are the warm-up), the step is
    recorded once and replayed for the remaining ones; no host-to-device copy after the first step.  The filter matrices of the UNet's 3x3
    convolutions are packed once per `sample` call (`functional.frozen_conv_packs`)."""

    def __init__(self, kind: str, unet: torch.nn.Module, schedule: Optional[NoiseSchedule] = None, *, eta: float = 0.0,
                 discretize: str = "uniform", unconditional_cond: Optional[Tensor] = None,
                 unconditional_guidance_scale: float = 1.0, temperature: float = 1.0, default_steps: Optional[int] = None,
                 noise_dropout: float = 0.0, quantize_denoised: bool = False, first_stage: Optional[torch.nn.Module] = None,
                 first_stage_scale_factor: float = 1.0, control_model: Optional[torch.nn.Module] = None,
                 control_scales: Optional[Sequence[float]] = None, only_mid_control: bool = False):
        if kind not in ops.SAMPLERS:
            raise ValueError(f"unrecognized sampler '{kind}'")
        dev = next(unet.parameters()).device
        self.kind, self.unet = kind, unet
        self.schedule = schedule or NoiseSchedule(device=dev)
        par = self.schedule.parameterization
        if kind == "ddim" and par not in ("eps", "v"):
            raise ValueError("only `v` / `eps` parameterization is supported in `ddim`")
        if kind == "basic" and par not in ("eps", "x0"):
            raise NotImplementedError(f"unrecognized parameterization '{par}' occurred")
        if noise_dropout > 0:
            raise NotImplementedError("`noise_dropout` > 0 is not built")
        if quantize_denoised:
            raise NotImplementedError("`quantize_denoised` (a VQ first stage) is not built")
        if kind == "basic" and (eta != 0.0 or discretize != "uniform" or unconditional_cond is not None
                                or unconditional_guidance_scale != 1.0):
            raise NotImplementedError("the `basic` sampler takes `temperature` and `default_steps` only (basic.py:39-52)")
        if default_steps is None:
            default_steps = 50 if kind == "ddim" else self.schedule.t
        self._configure(unconditional_cond, unconditional_guidance_scale, default_steps, first_stage, first_stage_scale_factor)
        self._configure_control(control_model, control_scales, only_mid_control)
        if discretize not in ("uniform", "quad"):
            raise ValueError(f"unrecognized discretize method '{discretize}' occurred")
        self.eta, self.discretize, self.temperature = float(eta), discretize, float(temperature)

    def _configure(self, unconditional_cond: Optional[Tensor], unconditional_guidance_scale: float, default_steps: int,
                   first_stage: Optional[torch.nn.Module], first_stage_scale_factor: float) -> None:
        """what every sampler takes: the guidance condition and scale, the default step count, the first stage, the graph slot"""
        if unconditional_cond is not None:
            if not isinstance(unconditional_cond, Tensor):
                raise NotImplementedError("a dict condition (concat / ControlNet hint keys) is not built")
            if unconditional_cond.dim() != 3 or unconditional_cond.shape[0] != 1:
                raise ValueError("`unconditional_cond` must be [1, L, D]")
        self.unconditional_cond = unconditional_cond
        self.unconditional_guidance_scale = float(unconditional_guidance_scale)
        self.default_steps = int(default_steps)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.first_stage = first_stage
        self.first_stage_scale_factor = float(first_stage_scale_factor)
        if first_stage is not None:
            first_stage.eval()

    control_model: Optional[torch.nn.Module] = None

    def _configure_control(self, control_model: Optional[torch.nn.Module], control_scales: Optional[Sequence[float]],
                           only_mid_control: bool) -> None:
        """one `ControlNet` beside the UNet (`DDPM.control_model`, ddpm.py:392-419, 457-458); `sample(hint=...)` feeds it"""
        if control_model is not None and not hasattr(control_model, "input_hint_block"):
            raise NotImplementedError("`control_model` must be one ControlNet (a dict of several is not built)")
        n = getattr(control_model, "num_control_scales", None)
        if control_scales is not None and (control_model is None or len(control_scales) != n):
            raise ValueError(f"`control_scales` needs a `control_model` and one float per output ({n})")
        self.control_model = control_model
        self.control_scales = None if control_scales is None else [float(v) for v in control_scales]
        self.only_mid_control = bool(only_mid_control)

    def table(self, num_steps: int) -> Tensor:
        return sampler_table(self.kind, self.schedule, num_steps, discretize=self.discretize, eta=self.eta)

    def sample(self, z: Optional[Tensor] = None, *, num_samples: Optional[int] = None, shape: Optional[Tuple[int, ...]] = None,
               cond: Optional[Tensor] = None, labels: Optional[Tensor] = None, num_steps: Optional[int] = None, seed: int = 0,
               noise: Optional[Tensor] = None, clip_output: bool = True, use_graph: bool = False, return_latent: bool = False,
               hint: Optional[Tensor] = None, **kwargs: Any) -> Tensor:
        """Returns the f32 [B, C, H, W] sample; with a `first_stage` (LDM.decode, ldm.py:192-202) that is the LATENT, which is
        returned as it is with `return_latent=True` and otherwise decoded: `first_stage.decode(latent / first_stage_scale_factor)`,
        after the last step and outside the recorded graph (`clip_output` acts on the latent, as in the reference).
        z: the starting noise (else B = num_samples normals of `shape` (C, H, W) from
        Philox at (seed, 0)); cond: the UNet's context [B, L, D]; noise: an explicit f32 bank [num_steps, B, C, H, W] in place
        of the Philox normals (seed, B C H W / 4 * (1 + step)) of each step.  hint: [B, hint_channels, 8 H, 8 W] for the sampler's
        `control_model`, which then runs in front of every UNet forward (with that forward's context; repeated for both halves of
        a batched [cond; uncond] forward), inside the recorded step and inside the frozen filter packs of both models."""
        for key in ("ref", "ref_mask", "ref_noise"):
            if kwargs.get(key) is not None:
                raise NotImplementedError("`sample` takes no reference (`ref` / `ref_mask` / `ref_noise`, merge_ref of basic.py:15-36): "
                                          "call `sample_with_reference`, `img2img` or `inpaint`")
        for key in ("control", "control_hint", "step_callback"):
            if kwargs.get(key) is not None:
                raise NotImplementedError(f"`{key}` is not built")
        self._check_hint(z, num_samples, shape, hint)
        if kwargs.get("start_step") not in (None, 0):
            raise NotImplementedError("`sample` starts at step 0: `start_step` > 0 is `sample_with_reference(start_step=...)` or `img2img`")
        rest = set(kwargs) - {"ref", "ref_mask", "ref_noise", "control", "control_hint", "step_callback", "start_step", "verbose"}
        if rest:
            raise TypeError(f"unexpected arguments {sorted(rest)}")
        return self._run(z, num_samples=num_samples, shape=shape, cond=cond, labels=labels, num_steps=num_steps, seed=seed, noise=noise,
                         clip_output=clip_output, use_graph=use_graph, return_latent=return_latent, hint=hint)

    def _check_hint(self, z: Optional[Tensor], num_samples: Optional[int], shape: Optional[Tuple[int, ...]], hint: Optional[Tensor]) -> None:
        if (hint is None) != (self.control_model is None):
            raise ValueError("`hint` and the sampler's `control_model` go together: one was given without the other")
        if hint is not None:  # (host-side, like the noise bank below)
            zs = tuple(z.shape) if z is not None else ((int(num_samples), *shape) if num_samples is not None and shape is not None else None)
            if zs is not None and len(zs) == 4 and tuple(hint.shape) != (zs[0], self.control_model.hint_channels, 8 * zs[2], 8 * zs[3]):
                raise ValueError(f"`hint` must be [B, hint_channels, 8 H, 8 W] = {[zs[0], self.control_model.hint_channels, 8 * zs[2], 8 * zs[3]]}, "
                                 f"got {list(hint.shape)}")

    def _run(self, z: Optional[Tensor], *, num_samples: Optional[int], shape: Optional[Tuple[int, ...]], cond: Optional[Tensor],
             labels: Optional[Tensor], num_steps: Optional[int], seed: int, noise: Optional[Tensor], clip_output: bool, use_graph: bool,
             return_latent: bool, hint: Optional[Tensor], start_step: int = 0, ref: Optional[dict] = None,
             z_is_state: bool = False) -> Tensor:
        """The run every public entry shares (`sample`, `sample_with_reference`, `img2img`, `inpaint`): steps start_step .. of a
        `num_steps` run from z.  ref: the checked reference pack of `_ref_pack` (host tensors) or None.  z_is_state: see
        `sample_with_reference`."""
        steps = self.default_steps if num_steps is None else int(num_steps)
        start_step = int(start_step)
        if not 0 <= start_step <= steps:
            raise ValueError(f"`start_step` must lie in [0, num_steps = {steps}], got {start_step}")
        if noise is not None:  # (host-side: checked before anything touches the device)
            if z is None and (num_samples is None or shape is None):
                raise ValueError("give `z`, or `num_samples` and `shape` = (C, H, W)")
            bank = self._bank_shape(steps, tuple(z.shape) if z is not None else (int(num_samples), *shape))
            if tuple(noise.shape) != bank:
                raise ValueError(f"the noise bank must be {self._bank_doc} = {list(bank)}, got {list(noise.shape)}")
        unet = self.unet
        dev = next(unet.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the sampler runs on the HIP device: move the UNet there first")
        if isinstance(cond, dict):
            raise NotImplementedError("a dict condition (concat / ControlNet hint keys) is not built")
        if z is None:
            if num_samples is None or shape is None:
                raise ValueError("give `z`, or `num_samples` and `shape` = (C, H, W)")
            b, n = int(num_samples), int(np.prod(shape))
            z = ops.randn(b * n, seed, 0, dev).view(b, *shape)
        if z.dim() != 4 or z.shape[1] != getattr(unet, "in_channels", z.shape[1]):
            raise ValueError("`z` must be [B, C, H, W] with the UNet's input channels")
        b = z.shape[0]
        total = z.numel()
        if (total // b) % 4 != 0:
            raise ValueError("C * H * W must be a multiple of 4")
        if cond is not None and (cond.dim() != 3 or cond.shape[0] != b):
            raise ValueError("`cond` must be [B, L, D]")
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
        cm = self.control_model
        uncond = self.unconditional_cond
        guided = cond is not None and uncond is not None and self.unconditional_guidance_scale != 1.0
        batched = guided and cond.shape[1] == uncond.shape[1]
        g = 2 if batched else 1
        st, first_in = self._begin(z.to(device=dev, dtype=torch.float32).contiguous(), steps, g * b, start_step, z_is_state)
        row0 = st["row0"]  # the first row of the table this run executes
        st.update(noise=noise, k=torch.full((1,), row0, dtype=torch.int32, device=dev))
        evals = st["table"].shape[0] - row0  # model evaluations of the run: the rows of the table from row0 on
        xin = torch.empty((g * b, *z.shape[1:]), dtype=torch.bfloat16, device=dev)
        for i in range(g):
            xin[i * b:(i + 1) * b].copy_(first_in)
        st["xin"] = xin
        ctx = None if cond is None else cond.to(device=dev, dtype=torch.float32).contiguous()
        ctx_u = None
        if guided:
            ctx_u = uncond.to(device=dev, dtype=torch.float32).repeat_interleave(b, dim=0)  # schema.py:225
            if batched:
                ctx, ctx_u = torch.cat([ctx, ctx_u]).contiguous(), None
        st.update(ctx=ctx, ctx_u=ctx_u, guided=guided, batched=batched, b=b, clip=bool(clip_output), seed=int(seed),
                  offset=total // 4)
        if labels is not None:
            labels = labels.to(dev).reshape(-1)
            st["labels"] = torch.cat([labels, labels]) if batched else labels
        else:
            st["labels"] = None
        st["hint"] = None
        if hint is not None:
            hint = hint.to(device=dev, dtype=torch.float32).contiguous()
            st["hint"] = torch.cat([hint, hint]).contiguous() if batched else hint
        st["ref"] = None
        if ref is not None and evals > 0:
            st["ref"] = self._ref_operands(ref, steps, row0, dev)
            self._first_merge(st)  # (in front of the warm-up: the recorded unit stays forward(s), one step launch, advance)
        with torch.no_grad(), HF.frozen_conv_packs(unet), (HF.frozen_conv_packs(cm) if cm is not None else contextlib.nullcontext()):
            if not use_graph:
                for _ in range(evals):
                    self._step(st)
            else:
                warm = min(2, evals)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):  # the warm-up passes (allocator, side lanes, lazy state) are real steps
                    for _ in range(warm):
                        self._step(st)
                torch.cuda.current_stream().wait_stream(side)
                if evals > warm:
                    torch.cuda.synchronize()
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph):  # recorded, not executed
                        self._step(st)
                    for _ in range(evals - warm):
                        self.graph.replay()
                    torch.cuda.synchronize()
                    self.graph = None  # (its buffers and the frozen packs it reads go with the call)
        if evals <= 0 and st["clip"]:  # (a sigma-space run of one step evaluates nothing: the clamp of ddpm.py:298-300 still acts)
            st["x"].clamp_(-1.0, 1.0)
        if self.first_stage is None or return_latent:
            return st["x"]
        from .modules import DecoderInputs

        with torch.no_grad():
            return self.first_stage.decode(DecoderInputs(z=st["x"] / self.first_stage_scale_factor))

    _bank_doc = "[num_steps, B, C, H, W]"

    def _bank_shape(self, steps: int, z_shape: Tuple[int, ...]) -> Tuple[int, ...]:
        return (steps, *z_shape)

    def _begin(self, x: Tensor, steps: int, gb: int, start_step: int = 0, z_is_state: bool = False) -> Tuple[dict, Tensor]:
        """(the run's state: x, the device table, the first row to execute, the UNet's timesteps buffer; the first UNet input) from
        the f32 z on the device.  The table is the full run's whatever `start_step`: the step counter stays absolute."""
        table = self.table(steps)
        row0 = min(start_step, steps)
        st = dict(x=x.clone(), table=table.to(x.device), row0=row0,
                  ts=torch.full((gb,), int(table[min(row0, steps - 1), 0]), dtype=torch.int64, device=x.device))
        return st, st["x"]

    # ---- sampling with a reference: image-to-image and inpainting ------------------------------

    takes_ref_noise = True  # DDIM / basic noise the reference (merge_ref); the K samplers merge it into `denoised` as it is

    def side_table(self, num_steps: int) -> Tensor:
        return sampler_side_table(self.kind, self.schedule, num_steps, discretize=self.discretize)

    def _ref_pack(self, z_shape: Tuple[int, ...], steps: int, start_step: int, ref: Optional[Tensor], ref_mask: Optional[Tensor],
                  ref_noise: Optional[Tensor], use_unified_ref_noise: bool, ref_noise_bank: Optional[Tensor]) -> Optional[dict]:
        """The reference operands of a run, checked on the host before anything touches the device -> dict(ref, mask, noise, mode)
        or None.  As in the reference (basic.py:27-32) `ref_noise` is read only with `use_unified_ref_noise`."""
        if ref is None and ref_mask is None:
            if ref_noise_bank is not None or use_unified_ref_noise:
                raise ValueError("`ref_noise_bank` / `use_unified_ref_noise` need a reference (`ref` and `ref_mask`)")
            return None
        if ref is None or ref_mask is None:
            raise ValueError("`ref` and `ref_mask` go together: one was given without the other")
        if len(z_shape) != 4:
            raise ValueError("`z` must be [B, C, H, W]")
        b, c, h, w = z_shape
        if tuple(ref.shape) != (b, c, h, w):
            raise ValueError(f"`ref` must have the shape of the state {[b, c, h, w]}, got {list(ref.shape)}")
        if ref_mask.dim() != 4 or ref_mask.shape[0] not in (1, b) or ref_mask.shape[1] not in (1, c) or tuple(ref_mask.shape[2:]) != (h, w):
            raise ValueError(f"`ref_mask` must be [{b} or 1, 1 or {c}, {h}, {w}], got {list(ref_mask.shape)}")
        mode, noise = "philox", None
        if not self.takes_ref_noise:
            if ref_noise is not None or ref_noise_bank is not None or use_unified_ref_noise:
                raise ValueError(f"the '{self.kind}' sampler merges the reference without noise (k_samplers.py:185-190): it takes no "
                                 "`ref_noise` / `use_unified_ref_noise` / `ref_noise_bank`")
        elif ref_noise_bank is not None:
            if use_unified_ref_noise:
                raise ValueError("give `ref_noise_bank` or `use_unified_ref_noise`, not both")
            merges = max(steps - start_step, 0)
            if tuple(ref_noise_bank.shape) != (merges, b, c, h, w):
                raise ValueError(f"`ref_noise_bank` must be [num_steps - start_step, B, C, H, W] = {[merges, b, c, h, w]}, "
                                 f"got {list(ref_noise_bank.shape)}")
            mode, noise = "bank", ref_noise_bank
        elif use_unified_ref_noise:
            if ref_noise is None:
                raise ValueError("`use_unified_ref_noise` needs `ref_noise`")
            if tuple(ref_noise.shape) != (b, c, h, w):
                raise ValueError(f"`ref_noise` must have the shape of the state {[b, c, h, w]}, got {list(ref_noise.shape)}")
            mode, noise = "unified", ref_noise
        return dict(ref=ref, mask=ref_mask, noise=noise, mode=mode)

    def _ref_operands(self, ref: dict, steps: int, row0: int, dev: Any) -> dict:
        """the pack of `_ref_pack` on the device, as the `_ref` entry points take it (the mask keeps its shape: never expanded)"""
        f = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        out = dict(ref=f(ref["ref"]), mask=f(ref["mask"]))
        if self.takes_ref_noise:
            out.update(side=self.side_table(steps).to(dev), merge_noise=f(ref["noise"]), merge_noise_mode=ref["mode"], merge_row0=row0)
        return out

    def _first_merge(self, st: dict) -> None:
        """the merge in front of the first executed step: it has no preceding step launch to ride in"""
        ops.diffusion_sample_merge(st["x"], st["xin"], st["k"], seed=st["seed"], offset=st["offset"], **st["ref"])

    def sample_with_reference(self, z: Optional[Tensor] = None, *, ref: Optional[Tensor] = None, ref_mask: Optional[Tensor] = None,
                              ref_noise: Optional[Tensor] = None, start_step: Optional[int] = 0, use_unified_ref_noise: bool = False,
                              ref_noise_bank: Optional[Tensor] = None, num_samples: Optional[int] = None,
                              shape: Optional[Tuple[int, ...]] = None, cond: Optional[Tensor] = None, labels: Optional[Tensor] = None,
                              num_steps: Optional[int] = None, seed: int = 0, noise: Optional[Tensor] = None, clip_output: bool = True,
                              use_graph: bool = False, return_latent: bool = False, hint: Optional[Tensor] = None,
                              z_is_state: bool = False, **kwargs: Any) -> Tensor:
        """`ISampler.sample` (schema.py:153-194) with its reference: steps start_step .. num_steps - 1 of a `num_steps` run from `z`
        (the state IN FRONT OF step start_step: with start_step > 0 it is taken as it stands), everything else as `sample`.
        ref [B, C, H, W] and ref_mask [B or 1, 1 or C, H, W] (1 = keep the reference), both or neither:
          ddim / basic (merge_ref, basic.py:16-35): in front of every executed step the state becomes ref_mask * q_sample(ref, t) +
            (1 - ref_mask) * state, inside the preceding step's launch (the first one in a launch of its own).  The noise of
            q_sample is a fresh draw per merge (Philox at (seed, B C H W / 4 * (1 + num_steps + step)), disjoint from the starting
            noise and the step draws), `ref_noise` [B, C, H, W] for every merge with `use_unified_ref_noise`, or entry j of
            `ref_noise_bank` [num_steps - start_step, B, C, H, W] for the merge in front of step start_step + j.
          k samplers (get_denoised_with_reference, k_samplers.py:185-190): every denoised value becomes ref_mask * ref +
            (1 - ref_mask) * denoised; no noise is involved and the two noise options are refused.
        The step counter, the timesteps and the step draws are those of the full run at the same steps; start_step >= num_steps (K:
        >= num_steps - 1) evaluates nothing and returns z.  z_is_state (K samplers, start_step = 0): z already is the sigma-space
        state, as `_q_sample` leaves it (its `_reset_buffers` sets `initialized`, so k_samplers.py:140-148 does not scale again)."""
        for key in ("control", "control_hint", "step_callback"):
            if kwargs.get(key) is not None:
                raise NotImplementedError(f"`{key}` is not built")
        rest = set(kwargs) - {"control", "control_hint", "step_callback", "verbose"}
        if rest:
            raise TypeError(f"unexpected arguments {sorted(rest)}")
        if isinstance(cond, dict):
            raise NotImplementedError("a dict condition (concat-conditioned inpainting UNets / ControlNet hint keys) is not built")
        self._check_hint(z, num_samples, shape, hint)
        steps = self.default_steps if num_steps is None else int(num_steps)
        start_step = 0 if start_step is None else int(start_step)
        if not 0 <= start_step <= steps:
            raise ValueError(f"`start_step` must lie in [0, num_steps = {steps}], got {start_step}")
        zs = tuple(z.shape) if z is not None else ((int(num_samples), *shape) if num_samples is not None and shape is not None else ())
        pack = self._ref_pack(zs, steps, start_step, ref, ref_mask, ref_noise, use_unified_ref_noise, ref_noise_bank)
        return self._run(z, num_samples=num_samples, shape=shape, cond=cond, labels=labels, num_steps=steps, seed=seed, noise=noise,
                         clip_output=clip_output, use_graph=use_graph, return_latent=return_latent, hint=hint, start_step=start_step,
                         ref=pack, z_is_state=z_is_state)

    def img2img_start(self, fidelity: float, num_steps: int) -> Tuple[int, int]:
        """(t, start_step) of `DiffusionAPI._q_sample` (api/multimodal/diffusion.py:1586-1593) for this sampler's family"""
        t = int(min(1.0 - fidelity, 0.999) * num_steps)
        return t, num_steps - t

    def _q_sample_start(self, z_ref: Tensor, t: int, start_step: int, num_steps: int, noise: Tensor) -> Tensor:
        """the sampler's own q-sampler at index t: sqrt(a) z_ref + sqrt(1 - a) noise (DDPMQSampler.q_sample, schema.py:94-108), a of
        the DDIM q-timesteps (ddim) or of the schedule (basic)"""
        w = _q_weights(self.kind, self.schedule, num_steps, self.discretize)
        ts = torch.full((z_ref.shape[0],), int(t), dtype=torch.int64, device=z_ref.device)
        return ops.q_sample(z_ref, noise, ts, w[0].to(z_ref.device).contiguous(), w[1].to(z_ref.device).contiguous())

    def _encode_ref(self, z_ref: Tensor, dev: Any, is_image: Optional[bool] = None) -> Tensor:
        """The reference latent: `z_ref` as it is, or, with a KL first stage, of the image [B, 3, 8 H, 8 W] in [-1, 1] (what the train
        step's `encode` takes): the posterior's mode times the scale factor (`_get_z` -> LDM.preprocess(deterministic=True)).
        is_image None: an image iff its channels are the first stage's and not the UNet's."""
        fs = self.first_stage
        z_ref = z_ref.to(dev)
        if z_ref.dim() != 4:
            raise ValueError(f"`z_ref` must be [B, C, H, W], got {list(z_ref.shape)}")
        cu = getattr(self.unet, "in_channels", None)
        if is_image is None:
            is_image = fs is not None and z_ref.shape[1] == getattr(fs, "in_channels", None) and z_ref.shape[1] != cu
        if not is_image:
            return z_ref.to(torch.float32).contiguous()
        if fs is None:
            raise ValueError("an image reference needs the sampler's `first_stage`")
        with torch.no_grad():
            enc = fs.encode(z_ref)
            if not hasattr(enc, "net"):
                raise NotImplementedError("an image reference needs a KL first stage (the posterior's mode); give a latent")
            return ops.gaussian_posterior(enc.net, scale_factor=self.first_stage_scale_factor, deterministic=True)[0]

    def _img2img_z(self, z_ref: Tensor, fidelity: float, steps: int, seed: int, noise: Optional[Tensor]) -> Tuple[Tensor, Tensor, int]:
        """`_q_sample` (api/multimodal/diffusion.py:1568-1613) -> (z, its noise, start_step); the noise is the Philox stream the
        starting noise would have used, (seed, 0), or the given tensor"""
        if not 0.0 <= float(fidelity) <= 1.0:
            raise ValueError(f"`fidelity` must lie in [0, 1], got {fidelity}")
        if noise is not None and tuple(noise.shape) != tuple(z_ref.shape):
            raise ValueError(f"the start's `noise` must have the latent's shape {list(z_ref.shape)}, got {list(noise.shape)}")
        if z_ref.dim() != 4 or (z_ref.numel() // z_ref.shape[0]) % 4 != 0:
            raise ValueError("`z_ref` must be [B, C, H, W] with C * H * W a multiple of 4")
        t, start_step = self.img2img_start(float(fidelity), steps)
        dev = z_ref.device
        noise = ops.randn(z_ref.numel(), seed, 0, dev).view(z_ref.shape) if noise is None else noise.to(device=dev, dtype=torch.float32).contiguous()
        return self._q_sample_start(z_ref, t, start_step, steps, noise), noise, start_step

    def img2img(self, z_ref: Tensor, *, fidelity: float, num_steps: Optional[int] = None, seed: int = 0, noise: Optional[Tensor] = None,
                **kwargs: Any) -> Tensor:
        """`DiffusionAPI._q_sample` + `_img2img` (api/multimodal/diffusion.py:1568-1647): noise the reference latent `z_ref` to the
        step `fidelity` names (1: keep it, 0: nearly pure noise) and run the remaining steps.  With a KL `first_stage`, `z_ref` may
        be the image [B, 3, 8 H, 8 W]; the result is decoded as `sample` decodes it (`return_latent=True`: the latent).  `noise`:
        the start's noise, else Philox at (seed, 0); the other keywords are `sample_with_reference`'s (its `noise` bank is
        `step_noise` here; `ref_is_image` overrides the channel-count rule that tells an image from a latent)."""
        steps = self.default_steps if num_steps is None else int(num_steps)
        dev = next(self.unet.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the sampler runs on the HIP device: move the UNet there first")
        z, _, start_step = self._img2img_z(self._encode_ref(z_ref, dev, kwargs.pop("ref_is_image", None)), fidelity, steps, seed, noise)
        return self.sample_with_reference(z, start_step=start_step, num_steps=steps, seed=seed, noise=kwargs.pop("step_noise", None),
                                          z_is_state=True, **kwargs)

    def inpaint(self, z_ref: Tensor, z_ref_mask: Tensor, *, fidelity: Optional[float] = None, use_background_reference: bool = False,
                num_steps: Optional[int] = None, seed: int = 0, noise: Optional[Tensor] = None, **kwargs: Any) -> Tensor:
        """`DiffusionAPI._get_z_ref_pack` + the raw-inpainting path (api/multimodal/diffusion.py:793-810, 1463-1478): the region
        where `z_ref_mask` [B or 1, 1 or C, H, W] is 1 keeps the reference through every step (fractional values blend).  The
        start: pure noise from step 0 (fidelity None), or `img2img`'s start at `fidelity` from z_ref — with `use_background_reference`
        from z_ref * mask + noise * (1 - mask).  `noise` (else Philox at (seed, 0)) is the start's noise and also the `ref_noise`
        handed on, which the merges use with `use_unified_ref_noise=True` (ddim / basic).  Image references, decoding and the other
        keywords as `img2img`."""
        steps = self.default_steps if num_steps is None else int(num_steps)
        dev = next(self.unet.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the sampler runs on the HIP device: move the UNet there first")
        if use_background_reference and fidelity is None:
            raise ValueError("`use_background_reference` shapes the start of a `fidelity` run: give `fidelity`")
        z_ref = self._encode_ref(z_ref, dev, kwargs.pop("ref_is_image", None))
        if (z_ref_mask.dim() != 4 or z_ref_mask.shape[0] not in (1, z_ref.shape[0]) or z_ref_mask.shape[1] not in (1, z_ref.shape[1])
                or tuple(z_ref_mask.shape[2:]) != tuple(z_ref.shape[2:])):
            raise ValueError(f"`z_ref_mask` must be [B or 1, 1 or C, H, W] of the latent {list(z_ref.shape)}, got {list(z_ref_mask.shape)}")
        mask = z_ref_mask.to(device=dev, dtype=torch.float32).contiguous()
        if noise is not None and tuple(noise.shape) != tuple(z_ref.shape):
            raise ValueError(f"the start's `noise` must have the latent's shape {list(z_ref.shape)}, got {list(noise.shape)}")
        noise = ops.randn(z_ref.numel(), seed, 0, dev).view(z_ref.shape) if noise is None else noise.to(device=dev, dtype=torch.float32).contiguous()
        if fidelity is None:
            z, start_step, prepared = noise, 0, False
        else:
            prepared = True
            src = z_ref * mask + noise * (1.0 - mask) if use_background_reference else z_ref
            z, _, start_step = self._img2img_z(src, fidelity, steps, seed, noise)
        return self.sample_with_reference(z, ref=z_ref, ref_mask=mask, ref_noise=noise if self.takes_ref_noise else None, start_step=start_step,
                                          num_steps=steps, seed=seed, noise=kwargs.pop("step_noise", None), z_is_state=prepared, **kwargs)

    def _forward(self, st: dict) -> Tuple[Tensor, Optional[Tensor]]:
        """the UNet forward(s) of one model evaluation -> (out, out_u | None)"""
        unet, cm, b = self.unet, self.control_model, st["b"]
        kw = {} if st["labels"] is None else {"labels": st["labels"]}

        def model(ctx: Optional[Tensor]) -> Tensor:
            if cm is None:
                return unet(st["xin"], timesteps=st["ts"], context=ctx, **kw)
            ctrl = cm(st["xin"], st["hint"], timesteps=st["ts"], context=ctx, scales=self.control_scales, **kw)  # ddpm.py:412-419
            return unet(st["xin"], timesteps=st["ts"], context=ctx, control=ctrl, only_mid_control=self.only_mid_control, **kw)

        out = model(st["ctx"])
        out_u = None
        if st["batched"]:
            out, out_u = out[:b], out[b:]
        elif st["guided"]:
            out_u = model(st["ctx_u"])
        return out, out_u

    def _step(self, st: dict) -> None:
        """UNet forward(s), sample_step, advance: all device work of one step, no host synchronisation"""
        out, out_u = self._forward(st)
        step = ops.diffusion_sample_step if st["ref"] is None else ops.diffusion_sample_step_ref  # (the same launch, with the merge)
        step(st["x"], st["xin"], out.contiguous(), st["table"], st["k"], kind=self.kind, parameterization=self.schedule.parameterization,
             out_u=None if out_u is None else out_u.contiguous(), scale=self.unconditional_guidance_scale, noise=st["noise"],
             temperature=self.temperature, clip_last=st["clip"], seed=st["seed"], offset=st["offset"], **(st["ref"] or {}))
        ops.diffusion_sample_advance(st["k"], st["table"], st["ts"])


# ---------------------------------------------------------------------------------------------
# The sigma-space "K" samplers: k_euler_a, k_heun, k_dpmpp_2m (reference samplers/k_samplers.py)
# ---------------------------------------------------------------------------------------------


def get_ancestral_step(sigma_from: float, sigma_to: float, eta: float = 1.0) -> Tuple[float, float]:
    """The ancestral split of a step sigma_from -> sigma_to into a deterministic part down to sigma_down and fresh noise of
    scale sigma_up (sigma_down^2 + sigma_up^2 = sigma_to^2), in Python floats: the reference's call site (k_samplers.py:387-391)
    hands its function `.item()`s, so the table must not form these in f32.  Operation order as k_samplers.py:35-48."""
    if not eta:
        return sigma_to, 0.0
    var_from, var_to = sigma_from ** 2, sigma_to ** 2
    sigma_up = min(sigma_to, eta * (var_to * (var_from - var_to) / var_from) ** 0.5)
    return (var_to - sigma_up ** 2) ** 0.5, sigma_up


def k_sigma_to_t(sigmas: Tensor, log_sigmas_base: Tensor, quantize: bool) -> Tensor:
    """The timestep of each sigma on the schedule's log-sigma axis (`IKSampler._sigma_to_t`, k_samplers.py:213-230, whose f32
    operations these are): with `quantize` the int64 index of the nearest base sigma, else the f32 position between the two
    base sigmas around it, linear in log sigma and clamped to the axis"""
    log_sigma = sigmas.log()
    dist = log_sigma - log_sigmas_base[:, None]  # [T, N]
    if quantize:
        return dist.abs().argmin(dim=0).view(sigmas.shape)
    below = dist.ge(0.0).cumsum(dim=0).argmax(dim=0).clamp(max=log_sigmas_base.shape[0] - 2)  # the last base sigma <= sigma
    above = below + 1
    lo, hi = log_sigmas_base[below], log_sigmas_base[above]
    w = ((lo - log_sigma) / (lo - hi)).clamp(0.0, 1.0)
    return ((1.0 - w) * below + w * above).view(sigmas.shape)


def k_sigma_tables(schedule: NoiseSchedule, total_step: int, sigmas_scheduler: Optional[str] = None, quantize: bool = False) -> dict:
    """`IKSampler._reset_buffers` / `_get_sigmas` / `_t_to_sigma` (k_samplers.py:207-269) on the CPU with the reference's dtypes
    and operation order: sigmas_base, log_sigmas_base, sigmas [total_step + 1] (the appended zero included) and the timestep
    `_sigma_to_t` makes of each of the first total_step sigmas (f32, or int64 with `quantize`)"""
    if total_step < 1:
        raise ValueError(f"num_steps must be at least 1, got {total_step}")
    alphas = schedule.alphas_cumprod.cpu()
    sigmas_base = ((1.0 - alphas) / alphas) ** 0.5
    log_base = sigmas_base.log()
    if sigmas_scheduler == "karras":
        rho = 7.0
        sigma_min, sigma_max = sigmas_base[0].item(), sigmas_base[-1].item()
        ramp = torch.linspace(0, 1, total_step)
        min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        sig = (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho
    elif sigmas_scheduler is None:
        ts = torch.linspace(len(sigmas_base) - 1, 0, total_step)
        low_idx, high_idx, w = ts.floor().long(), ts.ceil().long(), ts.frac()
        sig = ((1.0 - w) * log_base[low_idx] + w * log_base[high_idx]).exp()
    else:
        raise ValueError(f"unrecognized sigmas scheduler '{sigmas_scheduler}' occurred (None | 'karras')")
    sigmas = torch.cat([sig, sig.new_zeros([1])]).to(alphas.dtype)
    # (one sigma at a time, as `get_denoised` asks: `sigma * s_in` is a [B] tensor of equal entries)
    timesteps = torch.cat([k_sigma_to_t(sigmas[i:i + 1], log_base, quantize) for i in range(total_step)])
    return dict(sigmas_base=sigmas_base, log_sigmas_base=log_base, sigmas=sigmas, timesteps=timesteps)


K_COLUMNS = ("t", "sigma", "c_out", "c_skip", "c_in_next", "dt", "sigma_up", "sigma_ratio", "expm1_neg_h", "r_plus", "r_minus", "flag")


def k_sampler_table(kind: str, schedule: NoiseSchedule, num_steps: int, *, sigmas_scheduler: Optional[str] = None,
                    quantize: bool = False, start_step: int = 0) -> Tensor:
    """[evaluations, ops.KSAMPLE_ROW] f32 (CPU): row e = the scalars of model evaluation e of a `num_steps` run (num_steps - 1
    evaluating steps; two rows per step for k_heun), every one formed with the reference's own operations on 0-dim f32 tensors
    (Python floats inside `get_ancestral_step`) in its order.  Columns (K_COLUMNS; csrc/sample.hip): t, sigma, c_out, c_skip of
    this evaluation (k_samplers.py:152-183), c_in of the next evaluation's input, dt (euler_a: sigma_down - sigma; heun:
    next_sigma - sigma), sigma_up (euler_a), sigma_next / sigma, expm1(-h), 1 + 1 / (2 r), 1 / (2 r) (dpmpp_2m), flag.
    start_step: the rows stay those of the full run (the step counter is absolute); for k_dpmpp_2m the row of step `start_step`, the
    first one executed, has flag 0, which is what `old_denoised is None` after `_reset_buffers` gives the reference there."""
    if kind not in ops.KSAMPLERS:
        raise ValueError(f"unrecognized sampler '{kind}'")
    par = schedule.parameterization
    if par not in ("eps", "v"):
        raise ValueError("only `v` / `eps` parameterization is supported in `k_samplers`")
    return _k_rows(kind, par, k_sigma_tables(schedule, num_steps, sigmas_scheduler, quantize), start_step)


def _k_rows(kind: str, par: str, tb: dict, start_step: int = 0) -> Tensor:
    """the rows of `k_sampler_table` from the sigma tables `tb` of the run"""
    sigmas, ts = tb["sigmas"], tb["timesteps"]
    num_steps = ts.shape[0]
    sigma_data = 1.0

    def c_in(sigma: Tensor) -> Tensor:
        return 1.0 / (sigma ** 2 + sigma_data ** 2) ** 0.5

    def head(i: int, nxt: int) -> list:
        """t, sigma, c_out, c_skip of an evaluation at sigmas[i]; c_in of sigmas[nxt]"""
        sigma = sigmas[i]
        if par == "eps":
            c_out, c_skip = sigma, torch.tensor(1.0)
        else:
            c_out = sigma * sigma_data / (sigma ** 2 + sigma_data ** 2) ** 0.5
            c_skip = sigma_data ** 2 / (sigma ** 2 + sigma_data ** 2)
        return [ts[i].to(torch.float32), sigma, c_out, c_skip, c_in(sigmas[nxt])]

    zero, one = torch.tensor(0.0), torch.tensor(1.0)
    t_fn = lambda sg: sg.log().neg()  # noqa: E731  (KDPMpp2MSampler.t_fn)
    rows = []
    for step in range(num_steps - 1):
        sigma, nxt = sigmas[step], sigmas[step + 1]
        if kind == "k_euler_a":
            sigma_down, sigma_up = get_ancestral_step(sigma.item(), nxt.item(), eta=1.0)
            dt = sigma_down - sigma
            flag = one if nxt.item() > 0 else zero
            rows.append(head(step, step + 1) + [dt, torch.tensor(sigma_up, dtype=torch.float32), zero, zero, zero, zero, flag])
        elif kind == "k_heun":
            dt = nxt - sigma * (0.0 + 1)  # sigma_hat = sigma * (gamma + 1) with s_churn = 0
            rows.append(head(step, step + 1) + [dt, zero, zero, zero, zero, zero, zero])
            rows.append(head(step + 1, step + 1) + [dt, zero, zero, zero, zero, zero, one])
        else:
            t, t_next = t_fn(sigma), t_fn(nxt)
            h = t_next - t
            ratio, em1 = nxt / sigma, (-h).expm1()
            if step == 0 or step == start_step:  # (old_denoised is None: k_samplers.py:470-471)
                r_plus, r_minus, flag = zero, zero, zero
            else:
                h_last = t - t_fn(sigmas[step - 1])
                r = h_last / h
                r_plus, r_minus, flag = 1 + 1 / (2 * r), 1 / (2 * r), one
            rows.append(head(step, step + 1) + [zero, zero, ratio, em1, r_plus, r_minus, flag])
    if not rows:
        return torch.zeros((0, ops.KSAMPLE_ROW), dtype=torch.float32)
    out = torch.stack([torch.stack([v.to(torch.float32).reshape(()) for v in r]) for r in rows])
    assert out.shape[1] == ops.KSAMPLE_ROW == len(K_COLUMNS)
    return out


class KDiffusionSampler(DiffusionSampler):
    """`IKSampler` (samplers/k_samplers.py:73-269) with `KEulerAncestralSampler`, `KHeunSampler`, `KDPMpp2MSampler` around the
    HIP UNet.  The state is x = z * sigmas[0]; a run of `num_steps` makes num_steps - 1 steps that evaluate the model (k_heun
    twice per step) and the last step returns the image as it is (:149-150), so the sample ends at sigma_min; num_steps = 1
    returns z * sigmas[0].  Each model evaluation is three device operations: the UNet forward(s) on xin = bf16(image * c_in)
    with the evaluation's timestep (f32 and fractional, or int64 with `default_quantize`), `cfhip_k_sample_step` and
    `cfhip_k_sample_advance`; `use_graph` records one evaluation.  noise: an f32 bank [num_steps - 1, B, C, H, W] for k_euler_a
    (else Philox at (seed, B C H W / 4 * (1 + evaluation))); the other two kinds draw nothing and refuse one."""

    _bank_doc = "[num_steps - 1, B, C, H, W]"

    def __init__(self, kind: str, unet: torch.nn.Module, schedule: Optional[NoiseSchedule] = None, *, default_quantize: bool = False,
                 unconditional_cond: Optional[Tensor] = None, unconditional_guidance_scale: float = 1.0,
                 sigmas_scheduler: Optional[str] = None, default_steps: int = 25, first_stage: Optional[torch.nn.Module] = None,
                 first_stage_scale_factor: float = 1.0, control_model: Optional[torch.nn.Module] = None,
                 control_scales: Optional[Sequence[float]] = None, only_mid_control: bool = False):
        if kind not in ops.KSAMPLERS:
            raise ValueError(f"unrecognized sampler '{kind}'")
        dev = next(unet.parameters()).device
        self.kind, self.unet = kind, unet
        self.schedule = schedule or NoiseSchedule(device=dev)
        if self.schedule.parameterization not in ("eps", "v"):
            raise ValueError("only `v` / `eps` parameterization is supported in `k_samplers`")
        self._configure(unconditional_cond, unconditional_guidance_scale, default_steps, first_stage, first_stage_scale_factor)
        self._configure_control(control_model, control_scales, only_mid_control)
        if sigmas_scheduler not in (None, "karras"):
            raise ValueError(f"unrecognized sigmas scheduler '{sigmas_scheduler}' occurred (None | 'karras')")
        self.default_quantize = bool(default_quantize)
        self.sigmas_scheduler = sigmas_scheduler

    def table(self, num_steps: int) -> Tensor:
        return k_sampler_table(self.kind, self.schedule, num_steps, sigmas_scheduler=self.sigmas_scheduler,
                               quantize=self.default_quantize)

    def _bank_shape(self, steps: int, z_shape: Tuple[int, ...]) -> Tuple[int, ...]:
        if self.kind != "k_euler_a":
            raise ValueError(f"the '{self.kind}' sampler draws no noise: it takes no noise bank")
        return (steps - 1, *z_shape)

    def _begin(self, x: Tensor, steps: int, gb: int, start_step: int = 0, z_is_state: bool = False) -> Tuple[dict, Tensor]:
        tb = k_sigma_tables(self.schedule, steps, self.sigmas_scheduler, self.default_quantize)
        table = _k_rows(self.kind, self.schedule.parameterization, tb, start_step)
        per = 2 if self.kind == "k_heun" else 1
        row0 = min(start_step * per, table.shape[0])  # the counter is absolute: evaluation row of step `start_step`
        sigma0 = tb["sigmas"][min(start_step, steps - 1)]  # sigma of the first evaluation's input
        if start_step == 0 and not z_is_state:
            x = x * sigma0.to(x.device)  # `image * self.sigmas[0]` (k_samplers.py:148: at step 0 of a run `_q_sample` did not prepare)
        else:
            x = x.clone()
        c_in0 = 1.0 / (sigma0 ** 2 + 1.0 ** 2) ** 0.5
        ts_dtype = torch.int64 if self.default_quantize else torch.float32
        t0 = table[row0, 0].item() if row0 < table.shape[0] else 0.0
        st = dict(x=x, table=table.to(x.device), row0=row0,
                  ts=torch.full((gb,), int(t0) if self.default_quantize else t0, dtype=ts_dtype, device=x.device),
                  aux=None if self.kind == "k_euler_a" else torch.zeros_like(x))
        return st, x * c_in0.to(x.device)

    takes_ref_noise = False

    def _first_merge(self, st: dict) -> None:
        """nothing: the K samplers merge the reference inside every evaluation's launch"""

    def img2img_start(self, fidelity: float, num_steps: int) -> Tuple[int, int]:
        t = min(num_steps, round((1.0 - fidelity) * (num_steps + 1))) - 1
        return t, num_steps - t - 1

    def _q_sample_start(self, z_ref: Tensor, t: int, start_step: int, num_steps: int, noise: Tensor) -> Tensor:
        """KQSampler.q_sample (k_samplers.py:56-67) at index t + 1 of the flipped sigmas: z_ref + sigmas[start_step] * noise"""
        sigmas = k_sigma_tables(self.schedule, num_steps, self.sigmas_scheduler, self.default_quantize)["sigmas"]
        return z_ref + sigmas[start_step].to(z_ref.device) * noise

    def _step(self, st: dict) -> None:
        """UNet forward(s), k_sample_step, k_sample_advance: all device work of one model evaluation, no host synchronisation"""
        out, out_u = self._forward(st)
        step = ops.k_sample_step if st["ref"] is None else ops.k_sample_step_ref
        step(st["x"], st["aux"], st["xin"], out.contiguous(), st["table"], st["k"], kind=self.kind,
             parameterization=self.schedule.parameterization, out_u=None if out_u is None else out_u.contiguous(),
             scale=self.unconditional_guidance_scale, noise=st["noise"], clip_last=st["clip"], seed=st["seed"], offset=st["offset"],
             **(st["ref"] or {}))
        ops.k_sample_advance(st["k"], st["table"], st["ts"])


def make_sampler(kind: str, unet: torch.nn.Module, schedule: Optional[NoiseSchedule] = None, **config: Any) -> DiffusionSampler:
    """the reference's `ISampler.make(kind, model, **config)` for "ddim" and "basic"; config keys as there (eta,
    discretize, unconditional_cond, unconditional_guidance_scale, temperature, default_steps, noise_dropout,
    quantize_denoised), plus `first_stage` / `first_stage_scale_factor` of a latent model.  "k_euler_a" | "k_heun" |
    "k_dpmpp_2m": the keys of `IKSampler.__init__` (default_quantize, unconditional_cond, unconditional_guidance_scale,
    sigmas_scheduler, default_steps) and the same two first-stage keys.  All five kinds: `control_model` (one ControlNet),
    `control_scales`, `only_mid_control` (`DDPM.control_model` / `.control_scales` / `.only_mid_control`); `sample(hint=...)`."""
    if kind in UNBUILT_SAMPLERS:
        raise NotImplementedError(f"the '{kind}' sampler is not built (ddim, basic, k_euler_a, k_heun and k_dpmpp_2m are)")
    if kind in ops.KSAMPLERS:
        return KDiffusionSampler(kind, unet, schedule, **config)
    if kind not in ops.SAMPLERS:
        raise ValueError(f"unrecognized sampler '{kind}'")
    return DiffusionSampler(kind, unet, schedule, **config)
