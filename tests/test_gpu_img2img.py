"""Image-to-image and inpainting sampling on the GPU (csrc/sample.hip: sample_step_kernel<Rule, REF>, sample_merge_kernel;
diffusion.sample_with_reference / img2img / inpaint) against the numpy f32 replica of tests/img2img_replay.py (whose operation order
the host test pins to the reference's images) and the reference's own runs (tests/golden/img2img_samplers.pt): the step kernel
and the stand-alone merge per element, the step records teacher-forced and free-running, the Philox merge draw, start_step = 0
without a reference == `sample`, the tail of a run, end to end on the small UNet with the reference's bf16-autocast distance
as the yardstick, the inpainting invariant, graph == eager, the first stage and a ControlNet hint."""
import numpy as np
import pytest
import torch

import cflearn_amd as C
from cflearn_amd import ops
from cflearn_amd.diffusion import NoiseSchedule, k_sampler_table, make_sampler, sampler_philox_ranges
from helpers import guarded_ops
from img2img_replay import K_KINDS, clamp, decode, k_eval_ref_formula, merge_formula, record_id
from k_sampler_replay import COL
from sampler_replay import sha256, step_formula

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
KINDS = ("ddim", "basic") + K_KINDS
PARS = {"ddim": ("eps", "v"), "basic": ("eps", "x0"), **{k: ("eps", "v") for k in K_KINDS}}
GUIDANCE = np.float32(3.0)
TEMPERATURE = 0.9
# (B, C, H, W): H W = 9 (vectors straddle channels and samples), one vector in all, H W = 10 with an odd sample size in
# vectors, and 527 878 groups of four: past the 2048 x 256 groups one pass of the kernel's stride loop covers, H W odd
SHAPES = [(2, 4, 3, 3), (1, 4, 1, 1), (3, 2, 2, 5), (2, 4, 257, 1027)]
MASK_LAYOUTS = ("b1", "1c", "11", "bc")  # [B, 1, H, W], [1, C, H, W], [1, 1, H, W], [B, C, H, W]
# row flags of the synthetic 3-row K tables (tests/test_gpu_k_sampler.py): euler_a draw / no draw / draw; heun stage 1, 2, 2;
# dpmpp_2m without history, with, with
FLAGS = {"k_euler_a": (1.0, 0.0, 1.0), "k_heun": (0.0, 1.0, 1.0), "k_dpmpp_2m": (0.0, 1.0, 1.0)}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("img2img_samplers.pt")


@pytest.fixture(scope="module")
def decoded(fx):
    """every step record decoded once with the numpy replica (each image checked against the reference's hash)"""
    return [(r, decode(fx, r)) for r in fx["steps"]]


@pytest.fixture(scope="module")
def small(golden):
    u = golden("unet_small.pt")
    m = C.build_module("unet_diffuser", config=dict(u["cfg"]))
    m.load_state_dict(u["sd"])
    return m.to(DEV)


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _dev(a):
    return None if a is None else _t(a).to(DEV).contiguous()


def _mask(layout, shape, gen):
    """a mask of the layout with exact 0s, exact 1s and fractional values"""
    b, c, h, w = shape
    ms = (b if layout[0] == "b" else 1, c if layout[1] == "c" else 1, h, w)
    m = torch.rand(ms, generator=gen)
    pick = torch.rand(ms, generator=gen)
    m = torch.where(pick < 0.3, torch.zeros(()), torch.where(pick > 0.7, torch.ones(()), m))
    flat = m.view(-1)
    flat[0] = 1.0  # (the one-pixel shapes too hold a kept element)
    if flat.numel() > 1:
        flat[-1] = 0.0
    return m


def _table(kind):
    """3 rows: a timestep and coefficients in [0.2, 1.5] (K: dt negative, the flags of FLAGS)"""
    row = ops.KSAMPLE_ROW if kind in K_KINDS else ops.SAMPLE_ROW
    t = torch.rand((3, row), generator=torch.Generator().manual_seed(13)) * 1.3 + 0.2
    t[:, 0] = torch.tensor([900.0, 500.0, 100.0])
    if kind in K_KINDS:
        t[:, COL["dt"]] = -t[:, COL["dt"]]
        t[:, COL["flag"]] = torch.tensor(FLAGS[kind])
    return t


def _inputs(shape, kind, guided, seed=0):
    g = torch.Generator().manual_seed(1000 * shape[0] + shape[2] * shape[3] + seed)
    x = torch.randn(shape, generator=g) * 1.5
    ref = torch.randn(shape, generator=g)
    oc = torch.randn(shape, generator=g).to(BF16)
    ou = torch.randn(shape, generator=g).to(BF16) if guided else None
    draws = kind != "k_heun" and kind != "k_dpmpp_2m"
    bank = torch.randn((3, *shape), generator=g) if draws else None
    aux = None if kind in ("ddim", "basic", "k_euler_a") else torch.randn(shape, generator=g)
    return dict(x=x, ref=ref, oc=oc, ou=ou, bank=bank, aux=aux, gen=g)


def _mix(oc, ou):
    """the guided model output in the kernel's order: u + s (m - u)"""
    m = oc.float().numpy()
    if ou is None:
        return m
    u = ou.float().numpy()
    return u + GUIDANCE * (m - u)


def _want(kind, par, table, k, i, mask, *, side=None, nz=None, row0=0, clip=False):
    """one launch in numpy f32, the kernel's order -> dict(x, aux | None, xin as a bf16 tensor, writes_x, writes_aux)"""
    m = _mix(i["oc"], i["ou"])
    x, ref, msk = i["x"].numpy(), i["ref"].numpy(), mask.numpy()
    xi = None if i["bank"] is None else i["bank"][k].numpy()
    row = table[k].numpy()
    last = k == table.shape[0] - 1
    if kind not in K_KINDS:
        y = step_formula(kind, par, row, x, m, xi, TEMPERATURE)
        if not last and k + 1 >= row0:  # the merge in front of row k + 1; never after the last row
            y = merge_formula(y, ref, msk, side[k + 1, 0].item(), side[k + 1, 1].item(), nz)
        if clip and last:
            y = clamp(y)
        return dict(x=y, aux=None, xin=_t(y).bfloat16(), writes_x=True, writes_aux=False)
    aux = None if i["aux"] is None else i["aux"].numpy()
    flag = row[COL["flag"]] != 0
    y, a, nxt, _ = k_eval_ref_formula(kind, par, row, x, np.zeros_like(x) if aux is None else aux, m, xi, ref, msk)
    writes_x = not (kind == "k_heun" and not flag)
    if clip and last and writes_x:
        y = nxt = clamp(y)
    writes_aux = kind == "k_dpmpp_2m" or (kind == "k_heun" and not flag)
    return dict(x=y, aux=a, xin=_t(nxt * np.float32(row[COL["c_in_next"]])).bfloat16(), writes_x=writes_x, writes_aux=writes_aux)


def _launch(G, kind, par, table, k, i, mask, dup, clip, *, side=None, merge_noise=None, mode="philox", row0=0, seed=0, offset=0,
            philox_step=False):
    """one `_ref` launch on poisoned inputs and a guarded NaN xin -> (x, aux, xin) on the device"""
    shape = i["x"].shape
    xd = G.poisoned(i["x"].to(DEV))
    ad = None if i["aux"] is None else G.poisoned(i["aux"].to(DEV))
    xin = G.empty((dup * shape[0], *shape[1:]), dtype=BF16, device=DEV)
    common = dict(ref=G.poisoned(i["ref"].to(DEV)), mask=G.poisoned(mask.to(DEV)), kind=kind, parameterization=par,
                  out_u=None if i["ou"] is None else G.poisoned(i["ou"].to(DEV)), scale=float(GUIDANCE) if i["ou"] is not None else 1.0,
                  noise=None if (i["bank"] is None or philox_step) else G.poisoned(i["bank"].to(DEV)), clip_last=clip, seed=seed, offset=offset)
    kd = G.index(torch.tensor([k], dtype=torch.int32, device=DEV))
    td = G.poisoned(table.to(DEV))
    if kind in K_KINDS:
        ops.k_sample_step_ref(xd, ad, xin, G.poisoned(i["oc"].to(DEV)), td, kd, **common)
    else:
        ops.diffusion_sample_step_ref(xd, xin, G.poisoned(i["oc"].to(DEV)), td, kd, side=G.poisoned(side.to(DEV)), temperature=TEMPERATURE,
                                      merge_noise=None if merge_noise is None else G.poisoned(merge_noise.to(DEV)), merge_noise_mode=mode,
                                      merge_row0=row0, **common)
    return xd, ad, xin


def _same(got, want, tag):
    got = got.cpu()
    want = want if isinstance(want, torch.Tensor) else _t(want)
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    assert not bool(bad.any()), (tag, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


# ---------------------------------------------------------------------------------------------
# the step kernel and the stand-alone merge, per element
# ---------------------------------------------------------------------------------------------


def _combos(shape):
    """(mask layout, dup, guided, row, clip, ddim / basic merge-noise mode): every layout with every row and both guidance forms,
    the copies of xin and the noise modes cycling through them, the last row with and without the clamp; the large shape: two"""
    if int(np.prod(shape)) > 100000:
        return [("b1", 2, True, 0, True, "bank"), ("1c", 1, False, 2, True, "unified")]
    out, n = [], 0
    for layout in MASK_LAYOUTS:
        for guided in (False, True):
            for k in (0, 1, 2):
                out.append((layout, 1 + n % 2, guided, k, True, ("bank", "unified")[(n // 2) % 2]))
                n += 1
        out.append((layout, 2, False, 2, False, "bank"))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,par", [(k, p) for k in KINDS for p in PARS[k]])
def test_step_kernel_with_reference_per_element(G, shape, kind, par):
    """x, aux and xin after one `_ref` launch == the numpy f32 replica, bit for bit: both mask layouts and both batch strides
    (the mask is handed over unexpanded, inside NaN guards: a wrong index reads NaN), xin in one and two copies, guided and not,
    first / middle / last row.  ddim / basic: rows 0 and 1 merge with the NEXT row's side scalars and noise (bank entry
    row - merge_row0 with merge_row0 = 1, or the unified tensor), the last row does not merge and clamps (values beyond +-1
    present); a row whose next row lies below merge_row0 does not merge.  K: the merged denoised inside the rule; dpmpp_2m's aux is
    the merged value.  Guard words behind every operand stay untouched.  A counter outside the table writes nothing."""
    table = _table(kind)
    is_k = kind in K_KINDS
    side = None if is_k else torch.rand((3, 2), generator=torch.Generator().manual_seed(17)) * 0.9 + 0.1
    b = shape[0]
    for layout, dup, guided, k, clip, mode in _combos(shape):
        i = _inputs(shape, kind, guided)
        mask = _mask(layout, shape, i["gen"])
        tag = f"{kind}/{par} {shape} mask={layout} dup={dup} guided={guided} k={k} clip={clip} mode={mode}"
        if i["aux"] is not None and FLAGS[kind][k] == 0:  # an aux the row does not read is NaN on entry
            i["aux"] = torch.full_like(i["aux"], float("nan"))
        mn, nz, row0 = None, None, 0
        if not is_k:
            row0 = 1 if mode == "bank" else 0
            mn = torch.randn(((3 - row0, *shape) if mode == "bank" else shape), generator=i["gen"])
            if k < 2:
                nz = (mn[k + 1 - row0] if mode == "bank" else mn).numpy()
        want = _want(kind, par, table, k, i, mask, side=side, nz=nz, row0=row0, clip=clip)
        if clip and k == 2 and int(np.prod(shape)) >= 72 and want["writes_x"]:
            raw = _want(kind, par, table, k, i, mask, side=side, nz=nz, row0=row0, clip=False)["x"]
            assert (raw > 1).any() and (raw < -1).any() and np.abs(want["x"]).max() <= 1.0, tag
        xd, ad, xin = _launch(G, kind, par, table, k, i, mask, dup, clip, side=side, merge_noise=mn, mode=mode, row0=row0)
        _same(xd, want["x"] if want["writes_x"] else i["x"], tag + " x")
        if ad is not None:
            _same(ad, want["aux"] if want["writes_aux"] else i["aux"], tag + " aux")
        for c in range(dup):
            _same(xin[c * b:(c + 1) * b].float(), want["xin"].float(), tag + f" xin copy {c}")
        G.check()
    if not is_k:  # a merge in front of a row below merge_row0 does not happen: row 0 with merge_row0 = 2 is the plain step
        i = _inputs(shape, kind, False)
        mask = _mask("b1", shape, i["gen"])
        mn = torch.randn((1, *shape), generator=i["gen"])
        xd, _, xin = _launch(G, kind, par, table, 0, i, mask, 1, True, side=side, merge_noise=mn, mode="bank", row0=2)
        plain = step_formula(kind, par, table[0].numpy(), i["x"].numpy(), _mix(i["oc"], None), i["bank"][0].numpy(), TEMPERATURE)
        _same(xd, plain, f"{kind}/{par} {shape} below merge_row0")
        G.check()
    i = _inputs(shape, kind, True)
    mask = _mask("1c", shape, i["gen"])
    mn = None if is_k else torch.randn(shape, generator=i["gen"])
    for k in (-1, 3):  # outside the table: nothing is written
        xd, ad, xin = _launch(G, kind, par, table, k, i, mask, 2, True, side=side, merge_noise=mn, mode="unified")
        assert torch.equal(xd.cpu().view(torch.int32), i["x"].view(torch.int32)), (kind, par, k)
        if ad is not None:
            assert torch.equal(ad.cpu().view(torch.int32), i["aux"].view(torch.int32)), (kind, par, k)
        fill = torch.full(tuple(xin.shape), float("nan"), dtype=BF16)
        assert torch.equal(xin.cpu().view(torch.int16), fill.view(torch.int16)), (kind, par, k)
        G.check()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stand_alone_merge_per_element(G, shape):
    """`diffusion_sample_merge`: x and both copies of xin == the replica's merge in front of row k, for every mask layout, the
    three noise modes (Philox: the replica fed `ops.randn` at the documented counters) and every row; a k below merge_row0 or
    outside the table writes nothing"""
    side = torch.rand((3, 2), generator=torch.Generator().manual_seed(19)) * 0.9 + 0.1
    b, total = shape[0], int(np.prod(shape))
    big = total > 100000
    seed, offset = 0x0FEDCBA987654321, 5
    n = 0
    for layout in (("b1", "1c") if big else MASK_LAYOUTS):
        for mode in (("philox",) if big else ("philox", "unified", "bank")):
            for k in ((1,) if big else (0, 1, 2)):
                i = _inputs(shape, "ddim", False, seed=n)
                mask = _mask(layout, shape, i["gen"])
                dup = 1 + n % 2
                n += 1
                row0 = 1 if mode == "bank" and k >= 1 else 0
                mn = None
                if mode == "philox":
                    nz = ops.randn(total, seed, offset + (3 + k) * (total // 4), DEV).cpu().view(shape).numpy()
                else:
                    mn = torch.randn(((3 - row0, *shape) if mode == "bank" else shape), generator=i["gen"])
                    nz = (mn[k - row0] if mode == "bank" else mn).numpy()
                want = merge_formula(i["x"].numpy(), i["ref"].numpy(), mask.numpy(), side[k, 0].item(), side[k, 1].item(), nz)
                xd = G.poisoned(i["x"].to(DEV))
                xin = G.empty((dup * b, *shape[1:]), dtype=BF16, device=DEV)
                ops.diffusion_sample_merge(xd, xin, G.index(torch.tensor([k], dtype=torch.int32, device=DEV)), ref=G.poisoned(i["ref"].to(DEV)),
                                           mask=G.poisoned(mask.to(DEV)), side=G.poisoned(side.to(DEV)), seed=seed, offset=offset,
                                           merge_noise=None if mn is None else G.poisoned(mn.to(DEV)), merge_noise_mode=mode, merge_row0=row0)
                tag = f"merge {shape} mask={layout} mode={mode} k={k} dup={dup}"
                _same(xd, want, tag)
                for c in range(dup):
                    _same(xin[c * b:(c + 1) * b].float(), _t(want).bfloat16().float(), tag + f" xin copy {c}")
                G.check()
    i = _inputs(shape, "ddim", False)
    mask = _mask("b1", shape, i["gen"])
    for k, row0 in ((-1, 0), (3, 0), (0, 1)):
        xd = G.poisoned(i["x"].to(DEV))
        xin = G.empty((2 * b, *shape[1:]), dtype=BF16, device=DEV)
        ops.diffusion_sample_merge(xd, xin, G.index(torch.tensor([k], dtype=torch.int32, device=DEV)), ref=G.poisoned(i["ref"].to(DEV)),
                                   mask=G.poisoned(mask.to(DEV)), side=G.poisoned(side.to(DEV)), merge_row0=row0)
        assert torch.equal(xd.cpu().view(torch.int32), i["x"].view(torch.int32)), (k, row0)
        assert bool(torch.isnan(xin.float()).all()), (k, row0)
        G.check()


@pytest.mark.parametrize("kind", ["ddim", "basic"])
def test_philox_merge_draw_is_the_replica_on_randn(G, kind):
    """without a merge-noise tensor the noise of the merge in front of row k + 1 is `ops.randn(total, seed, offset + (rows + k + 1) *
    total / 4)` (the stream test_gpu_philox.py pins to the host): x equals the replica fed those normals and the step's own
    draw `ops.randn(total, seed, offset + k * total / 4)`; and the step's draw does not depend on the reference being there: with
    an all-zero mask the `_ref` launch equals the plain launch bit for bit"""
    par = "eps"
    table = _table(kind)
    side = torch.rand((3, 2), generator=torch.Generator().manual_seed(17)) * 0.9 + 0.1
    seed = 0x123456789ABCDEF0
    for shape, offset in (((2, 4, 3, 3), 7), ((3, 2, 2, 5), 2 ** 32 - 2)):
        total = int(np.prod(shape))
        ranges = sampler_philox_ranges(total, 3)
        for k in (0, 1):
            i = _inputs(shape, kind, True)
            mask = _mask("b1", shape, i["gen"])
            xi = ops.randn(total, seed, offset + k * (total // 4), DEV).cpu().view(shape)
            nz = ops.randn(total, seed, offset + (3 + k + 1) * (total // 4), DEV).cpu().view(shape)
            assert ranges["merges"][k + 1][0] - ranges["steps"][0][0] == (3 + k + 1) * (total // 4)  # (the documented layout)
            fed = dict(i, bank=torch.stack([xi] * 3))
            want = _want(kind, par, table, k, fed, mask, side=side, nz=nz.numpy())
            xd, _, xin = _launch(G, kind, par, table, k, i, mask, 1, True, side=side, seed=seed, offset=offset, philox_step=True)
            _same(xd, want["x"], f"{kind} {shape} k={k} philox merge")
            _same(xin.float(), want["xin"].float(), f"{kind} {shape} k={k} philox merge xin")
            zero = torch.zeros_like(mask)
            xr, _, _ = _launch(G, kind, par, table, k, i, zero, 1, True, side=side, seed=seed, offset=offset, philox_step=True)
            xp = G.poisoned(i["x"].to(DEV))
            ops.diffusion_sample_step(xp, G.empty(shape, dtype=BF16, device=DEV), i["oc"].to(DEV), table.to(DEV),
                                      torch.tensor([k], dtype=torch.int32, device=DEV), kind=kind, parameterization=par, out_u=i["ou"].to(DEV),
                                      scale=float(GUIDANCE), temperature=TEMPERATURE, clip_last=True, seed=seed, offset=offset)
            assert torch.equal(xr, xp), f"{kind} {shape} k={k}: a zero mask must leave the plain step"
    G.check()


# ---------------------------------------------------------------------------------------------
# the reference's step records
# ---------------------------------------------------------------------------------------------


def _record_operands(fx, r, d):
    """the device operands of a record's launches: the full-run table (and side table), the step-noise bank and the reference pack"""
    steps, start, is_k = r["steps"], r["start_step"], r["kind"] in K_KINDS
    z_shape = tuple(fx["step_z"].shape)
    if is_k:
        table = d["table"].to(DEV)
    else:
        table = torch.zeros((steps, ops.SAMPLE_ROW))
        table[start:] = d["table"]
        table = table.to(DEV)
    rows, row0 = table.shape[0], d["row0"]
    bank = None
    if any(v is not None for v in d["step_noise"]) and r["kind"] != "k_heun":
        bank = torch.zeros((rows, *z_shape))
        for j, v in enumerate(d["step_noise"]):
            bank[row0 + j] = _t(v)
        bank = bank.to(DEV)
    ref = None
    if r["mask"] is not None:
        ref = dict(ref=_dev(d["ref"]), mask=_dev(d["mask"]))
        if not is_k:
            side = torch.zeros((steps, 2))
            side[start:] = d["side"]
            if r["unified"]:
                mn, mode = fx["step_ref_noise"].to(DEV), "unified"
            else:
                mn, mode = torch.stack([_t(d["first_merge_noise"])] + [_t(v) for v in d["merge_noise"][:-1]]).to(DEV), "bank"
            ref.update(side=side.to(DEV), merge_noise=mn.contiguous(), merge_noise_mode=mode, merge_row0=row0)
    return table, bank, ref


def _record_step(r, x, aux, xin, oc, ou, table, k, bank, ref):
    kw = dict(kind=r["kind"], parameterization=r["parameterization"], out_u=ou, scale=r["scale"] or 1.0, noise=bank, **(ref or {}))
    if r["kind"] in K_KINDS:
        (ops.k_sample_step_ref if ref else ops.k_sample_step)(x, aux, xin, oc, table, k, **kw)
    else:
        (ops.diffusion_sample_step_ref if ref else ops.diffusion_sample_step)(x, xin, oc, table, k, temperature=r["temperature"], **kw)


def _record_outs(r, d, j, b):
    o = _t(d["outputs"][j]).to(DEV).bfloat16()
    assert torch.equal(o.float().cpu(), _t(d["outputs"][j]))  # the recorded outputs are bf16 values
    return (o, None) if r["scale"] is None else (o[:b].contiguous(), o[b:].contiguous())


def test_step_records_teacher_forced_bit_for_bit(fx, decoded):
    """every launch of every record with the replica's state in front of it (the reference's image, merged): x, aux and both
    copies of xin equal the replica, whose images carry the reference's hashes.  The counter is the absolute row."""
    assert len(decoded) == 120
    b = fx["step_z"].shape[0]
    for r, d in decoded:
        table, bank, ref = _record_operands(fx, r, d)
        is_k = r["kind"] in K_KINDS
        for j in range(len(d["pre"])):
            x = _dev(d["pre"][j]).clone()
            aux = None if (not is_k or r["kind"] == "k_euler_a") else _dev(d["pre_aux"][j]).clone()
            xin = torch.empty((2 * b, *x.shape[1:]), dtype=BF16, device=DEV)
            oc, ou = _record_outs(r, d, j, b)
            _record_step(r, x, aux, xin, oc, ou, table, torch.tensor([d["row0"] + j], dtype=torch.int32, device=DEV), bank, ref)
            tag = (record_id(r), j)
            assert torch.equal(x.cpu(), _t(d["post"][j])), tag
            if aux is not None:
                assert torch.equal(aux.cpu(), _t(d["post_aux"][j])), tag
            nxt = d["nexts"][j] * np.float32(d["table"][d["row0"] + j, COL["c_in_next"]].item()) if is_k else d["nexts"][j]
            want_in = _t(nxt).bfloat16()
            assert torch.equal(xin[:b].cpu(), want_in) and torch.equal(xin[b:].cpu(), want_in), tag


def test_step_records_free_run_reproduce_every_image_hash(fx, decoded):
    """all launches chained on the device from `step_z` as `_run` chains them (the stand-alone merge in front of the first ddim /
    basic step, then step + advance from the absolute row of start_step), the outputs fed as recorded: the state after every
    launch equals the replica's bit for bit, the image after every step whose image the state IS (every K step; a ddim / basic
    step that no merge follows) hashes to the reference's, and the timesteps buffer holds what the reference's `denoise` received"""
    b = fx["step_z"].shape[0]
    for r, d in decoded:
        table, bank, ref = _record_operands(fx, r, d)
        is_k, kind = r["kind"] in K_KINDS, r["kind"]
        per = 2 if kind == "k_heun" else 1
        x = _dev(d["pre"][0] if is_k else fx["step_z"].numpy()).clone()
        aux = None if (not is_k or kind == "k_euler_a") else torch.zeros_like(x)
        xin = torch.empty_like(x, dtype=BF16)
        k = torch.full((1,), d["row0"], dtype=torch.int32, device=DEV)
        ts = torch.full((b,), -1, dtype=torch.int64 if (not is_k or r["quantize"]) else F32, device=DEV)
        if ref is not None and not is_k:
            ops.diffusion_sample_merge(x, xin, k, **ref)
            assert torch.equal(x.cpu(), _t(d["pre"][0])), record_id(r)
        launches = len(d["pre"])
        for j in range(launches):
            oc, ou = _record_outs(r, d, j, b)
            _record_step(r, x, aux, xin, oc, ou, table, k, bank, ref)
            (ops.k_sample_advance if is_k else ops.diffusion_sample_advance)(k, table, ts)
            tag = (record_id(r), j)
            assert torch.equal(x.cpu(), _t(d["post"][j])), tag
            if j + 1 < launches:
                assert torch.equal(ts.cpu().to(r["timesteps"].dtype), r["timesteps"][j + 1].expand(b)), tag
            if is_k and (j + 1) % per == 0:
                assert sha256(x.cpu()) == r["image_sha256"][(j + 1) // per], tag
            elif not is_k and (ref is None or j == launches - 1):
                assert sha256(x.cpu()) == r["image_sha256"][j + 1], tag
        assert k.item() == table.shape[0]
        assert sha256(x.cpu()) == r["image_sha256"][-1], record_id(r)


def test_inpainting_invariant_through_aux(fx, decoded):
    """where the mask is exactly 1 the merged denoised IS the reference, bit for bit: k_dpmpp_2m leaves it in `aux` (the replica
    holds the same for every K kind and evaluation, tests/test_img2img_host.py, and the kernel equals the replica above)"""
    b = fx["step_z"].shape[0]
    n = 0
    for r, d in decoded:
        if r["kind"] != "k_dpmpp_2m" or r["mask"] is None:
            continue
        table, bank, ref = _record_operands(fx, r, d)
        keep = torch.from_numpy(np.broadcast_to(d["mask"] == 1, d["ref"].shape).copy())
        assert bool(keep.any()) and not bool(keep.all())
        j = len(d["pre"]) - 1  # the last evaluation of the run
        x, aux = _dev(d["pre"][j]).clone(), _dev(d["pre_aux"][j]).clone()
        xin = torch.empty_like(x, dtype=BF16)
        oc, ou = _record_outs(r, d, j, b)
        _record_step(r, x, aux, xin, oc, ou, table, torch.tensor([d["row0"] + j], dtype=torch.int32, device=DEV), bank, ref)
        assert torch.equal(aux.cpu()[keep], _t(d["ref"])[keep]), record_id(r)
        assert not torch.equal(aux.cpu()[~keep], _t(d["ref"])[~keep])
        n += 1
    assert n == 16


# ---------------------------------------------------------------------------------------------
# the samplers around the small UNet
# ---------------------------------------------------------------------------------------------


def _sampler(kind, small, e, guided=True, **cfg):
    if guided and kind != "basic":  # (the basic sampler takes no guidance: basic.py:39-52)
        cfg.update(unconditional_cond=e["uncond"], unconditional_guidance_scale=e["scale"])
    return make_sampler(kind, small, NoiseSchedule(device=DEV), **cfg)


def _half_plane(h=16, w=16):
    col = torch.zeros(w)
    col[:7], col[7] = 1.0, 0.5
    return col.repeat(h, 1).view(1, 1, h, w).contiguous()


@pytest.mark.parametrize("kind", KINDS)
def test_start_step_zero_without_reference_is_sample(fx, small, kind):
    """the same z, seed and num_steps: `sample_with_reference` with start_step = 0 and no reference == `sample`, bit for bit
    (Philox step draws included), and so is the run from `num_samples` / `shape`"""
    e = fx["e2e"]
    s = _sampler(kind, small, e)
    z = torch.randn((2, 3, 16, 16), generator=torch.Generator().manual_seed(31)).to(DEV)
    kw = dict(cond=e["cond"].to(DEV), num_steps=5, seed=11)
    assert torch.equal(s.sample_with_reference(z, start_step=0, **kw), s.sample(z, **kw))
    assert torch.equal(s.sample_with_reference(z, **kw), s.sample(z, **kw))
    assert torch.equal(s.sample_with_reference(num_samples=2, shape=(3, 16, 16), start_step=None, **kw),
                       s.sample(num_samples=2, shape=(3, 16, 16), **kw))
    # nothing left to run: z comes back (clamped with clip_output), no forward
    end = 5 if kind in ("ddim", "basic") else 4
    for start in (end, 5):
        assert torch.equal(s.sample_with_reference(z, start_step=start, clip_output=False, **kw), z)
        assert torch.equal(s.sample_with_reference(z, start_step=start, **kw), z.clamp(-1.0, 1.0))


# (the basic sampler takes no guidance: basic.py:39-52)
@pytest.mark.parametrize("kind,guided", [("ddim", False), ("ddim", True), ("basic", False), ("k_euler_a", False), ("k_euler_a", True),
                                         ("k_dpmpp_2m", False), ("k_dpmpp_2m", True)])
def test_tail_of_a_run_is_the_replica_chain(fx, small, kind, guided):
    """a run with start_step = 2 of 5 steps, a reference, a fractional mask and explicit banks (rows 2.. of the step noise; one
    entry per merge) equals the numpy replica chained from the same state on the model outputs the UNet actually produced (caught
    by a hook), bit for bit: the counter, the side table, both banks and the first executed dpmpp_2m row are the full run's"""
    e = fx["e2e"]
    s = _sampler(kind, small, e, guided=guided, **({"eta": 0.7} if kind == "ddim" else {}))
    gen = torch.Generator().manual_seed(41)
    shape, steps, start = (2, 3, 16, 16), 5, 2
    z, ref = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    mask = _half_plane()
    is_k = kind in K_KINDS
    kw = dict(cond=e["cond"].to(DEV), num_steps=steps, start_step=start, ref=ref.to(DEV), ref_mask=mask.to(DEV), clip_output=True)
    if kind != "k_dpmpp_2m":
        bank = torch.randn((steps - 1 if is_k else steps, *shape), generator=gen)
        kw["noise"] = bank.to(DEV)
    if not is_k:
        mbank = torch.randn((steps - start, *shape), generator=gen)
        kw["ref_noise_bank"] = mbank.to(DEV)
    outs = []
    hook = small.register_forward_hook(lambda mod, args, out: outs.append(out.detach().float().cpu().clone()))
    try:
        got = s.sample_with_reference(z.to(DEV), **kw)
    finally:
        hook.remove()
    table = s.table(steps)
    rows = table.shape[0]
    assert len(outs) == rows - start

    def mixed(o):
        o = o.numpy()
        return o if not guided else o[2:] + np.float32(e["scale"]) * (o[:2] - o[2:])

    x, rf, mk = z.numpy(), ref.numpy(), mask.numpy()
    if is_k:
        if kind == "k_dpmpp_2m":  # `table()` is the full run's; a run from `start` has no old_denoised at its first row
            assert table[start, COL["flag"]].item() == 1.0
            table = k_sampler_table(kind, s.schedule, steps, start_step=start)
            assert table[start, COL["flag"]].item() == 0.0
        aux = np.zeros_like(x)
        for j, row in enumerate(range(start, rows)):
            xi = bank[row].numpy() if kind == "k_euler_a" else None
            x, aux, _, _ = k_eval_ref_formula(kind, "eps", table[row].numpy(), x, aux, mixed(outs[j]), xi, rf, mk)
    else:
        side = s.side_table(steps)
        for j, row in enumerate(range(start, rows)):
            x = merge_formula(x, rf, mk, side[row, 0].item(), side[row, 1].item(), mbank[j].numpy())
            x = step_formula(kind, "eps", table[row].numpy(), x, mixed(outs[j]), bank[row].numpy(), s.temperature)
    x = clamp(x)
    _same(got, x, f"{kind} tail from step {start}")


def _per_sample(a, ref):
    a, ref = a.float().cpu().flatten(1), ref.float().flatten(1)
    return ((a - ref).norm(dim=1) / ref.norm(dim=1)).tolist()


def _bank(e, run, kind, steps, start):
    """the recorded step draws of an e2e run as the full-run bank the sampler takes (rows below start_step are never read)"""
    if "noise_q" not in run:
        return None
    draws = run["noise_q"].float() * run["noise_scale"]
    rows = steps - 1 if kind in K_KINDS else steps
    bank = torch.zeros((rows, *draws.shape[1:]))
    bank[start:start + draws.shape[0]] = draws
    assert start + draws.shape[0] == rows
    return bank


E2E_RUNS = [(k, "img2img") for k in KINDS] + [(k, "inpaint") for k in ("ddim", "k_euler_a", "k_dpmpp_2m")]


@pytest.mark.parametrize("kind,job", E2E_RUNS)
def test_end_to_end_small_unet_within_the_reference_bf16_distance(fx, small, kind, job):
    """Per-sample relative L2 against the reference's fp32 run <= 1.1 x the reference's own bf16-autocast distance (the margin
    test_gpu_sampler.py and test_gpu_k_sampler.py hold), for every image-to-image record (`img2img` from the recorded reference,
    fidelity and start noise: start_step 4 of 12) and every inpainting record (`inpaint` from pure noise, the half-plane mask
    with a fractional edge, unified reference noise), with the recorded step noise."""
    e = fx["e2e"]
    name = f"{kind}_{job}"
    assert sorted(e["runs"]) == sorted(f"{k}_{j}" for k, j in E2E_RUNS)  # every record of the fixture is covered
    run = e["runs"][name]
    s = _sampler(kind, small, e)
    steps = e["steps"]
    kw = dict(cond=e["cond"].to(DEV), num_steps=steps, noise=e["start_noise"].to(DEV), clip_output=False,
              step_noise=_bank(e, run, kind, steps, run["start_step"]))
    if job == "img2img":
        assert s.img2img_start(e["fidelity"][kind], steps)[1] == run["start_step"] == 4
        y = s.img2img(e["z_ref"].to(DEV), fidelity=e["fidelity"][kind], **kw)
    else:
        assert torch.equal(e["mask"], _half_plane())
        extra = dict(use_unified_ref_noise=True) if kind == "ddim" else {}
        y = s.inpaint(e["z_ref"].to(DEV), e["mask"].to(DEV), **extra, **kw)
    mine, yard = _per_sample(y, run["fp32"]), _per_sample(run["autocast"], run["fp32"])
    print(f"{name} e2e per-sample rel-L2 vs fp32: HIP {mine}, reference bf16 autocast {yard}, "
          f"ratio {[a / b for a, b in zip(mine, yard)]}")
    for a, b in zip(mine, yard):
        assert a <= 1.1 * b, (mine, yard)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("kind", ["ddim", "k_heun"])
def test_graph_equals_eager_with_a_reference(fx, small, kind, guided):
    """ref + mask + (ddim) a fresh Philox draw per merge inside the recorded launch + start_step: the recorded unit is unchanged
    (forward(s), one step launch, advance; the first merge runs in front of the warm-up), and replaying it equals the eager
    run bit for bit; another seed gives another image for ddim (the merge noise is drawn)"""
    e = fx["e2e"]
    s = _sampler(kind, small, e, guided=guided, **({"eta": 0.5} if kind == "ddim" else {}))
    gen = torch.Generator().manual_seed(51)
    z, ref = torch.randn((2, 3, 16, 16), generator=gen).to(DEV), torch.randn((2, 3, 16, 16), generator=gen).to(DEV)
    kw = dict(cond=e["cond"].to(DEV), num_steps=8, start_step=2, ref=ref, ref_mask=_half_plane().to(DEV), seed=5)
    eager = s.sample_with_reference(z, **kw)
    graph = s.sample_with_reference(z, **kw, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), (eager - graph).abs().max().item()
    assert not torch.equal(eager, s.sample_with_reference(z, **dict(kw, ref=None, ref_mask=None)))
    if kind == "ddim":
        assert not torch.equal(s.sample_with_reference(z, **dict(kw, seed=6)), eager)


@pytest.mark.parametrize("kind", ["ddim", "k_dpmpp_2m"])
def test_first_stage_image_in_image_out(kind):
    """`img2img` / `inpaint` with the small KL first stage: an image goes in (encoded to the posterior's mode times the scale
    factor), an image comes out (the decode of latent / scale); `return_latent=True` gives the latent; a latent reference gives
    the same as the image it was encoded from"""
    from test_gpu_first_stage import SCALE, _small_ae, _small_unet

    ae, _ = _small_ae()
    unet = _small_unet().eval()
    img = torch.tanh(torch.randn((2, 3, 16, 16), generator=torch.Generator().manual_seed(61))).to(DEV)
    s = make_sampler(kind, unet, NoiseSchedule(device=DEV), first_stage=ae, first_stage_scale_factor=SCALE)
    with torch.no_grad():
        z_ref = ops.gaussian_posterior(ae.encode(img).net, scale_factor=SCALE, deterministic=True)[0]
    assert tuple(z_ref.shape) == (2, 4, 8, 8)
    kw = dict(fidelity=0.5, num_steps=6, seed=9)
    out = s.img2img(img, **kw)
    latent = s.img2img(img, return_latent=True, **kw)
    assert tuple(out.shape) == (2, 3, 16, 16) and tuple(latent.shape) == (2, 4, 8, 8) and latent.dtype == F32
    with torch.no_grad():
        assert torch.equal(out, ae.decode(C.DecoderInputs(z=latent / SCALE)))
    assert torch.equal(s.img2img(z_ref, return_latent=True, **kw), latent)
    mask = _half_plane(8, 8).to(DEV)
    pic = s.inpaint(img, mask, num_steps=6, seed=9)
    lat = s.inpaint(img, mask, num_steps=6, seed=9, return_latent=True)
    assert tuple(pic.shape) == (2, 3, 16, 16) and tuple(lat.shape) == (2, 4, 8, 8)
    assert torch.equal(lat, s.inpaint(z_ref, mask, num_steps=6, seed=9, return_latent=True))
    assert not torch.equal(lat, s.sample(num_samples=2, shape=(4, 8, 8), num_steps=6, seed=9, return_latent=True))
    bg = s.inpaint(img, mask, num_steps=6, seed=9, fidelity=0.2, use_background_reference=True, return_latent=True)
    assert torch.isfinite(bg).all() and not torch.equal(bg, lat)


@pytest.mark.parametrize("kind", ["ddim", "k_euler_a"])
def test_controlnet_hint_together_with_a_reference(kind):
    """a ControlNet `hint` and a reference in one run: it runs (eager and recorded alike) and differs from the run without the
    reference and from the run without the ControlNet"""
    from test_gpu_controlnet import GOLDEN, _inputs as cn_inputs, _models

    g = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    unet, cn = _models(g)
    i = cn_inputs(g)
    gen = torch.Generator().manual_seed(71)
    shape = tuple(i["x_t"].shape)
    z, ref = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
    mask = _half_plane(shape[2], shape[3]).to(DEV)
    sch = NoiseSchedule(device=DEV)
    s = make_sampler(kind, unet, sch, control_model=cn, control_scales=g["scales"])
    kw = dict(cond=i["context"], num_steps=5, seed=3, start_step=1)
    both = s.sample_with_reference(z, ref=ref, ref_mask=mask, hint=i["hint"], **kw)
    assert torch.isfinite(both).all()
    assert torch.equal(both, s.sample_with_reference(z, ref=ref, ref_mask=mask, hint=i["hint"], use_graph=True, **kw))
    assert not torch.equal(both, s.sample_with_reference(z, hint=i["hint"], **kw))
    assert not torch.equal(both, make_sampler(kind, unet, sch).sample_with_reference(z, ref=ref, ref_mask=mask, **kw))
    with pytest.raises(ValueError, match="go together"):
        s.sample_with_reference(z, ref=ref, ref_mask=mask, **kw)
