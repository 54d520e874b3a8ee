"""The VQ first stage on the HIP path: the fused nearest-code kernel (cfhip_vq_nearest / cfhip_vq_code_sqnorm, csrc/vq.hip) per row
against exact float64 arithmetic on the same inputs, AttentionAutoEncoderVQ against the reference's fp32 CPU run
(tests/golden/ae_vq_small.pt — tools/gen_vq_golden.py), and the VQ paths of DDPMTrainStep and DiffusionSampler.

Error model of one score (exact arithmetic in float64 on the same inputs): score_j = sq_j - 2 dot_j with sq_j and dot_j f32 fmaf
chains of D terms (D roundings each) and one rounding for the subtraction (2 dot_j is exact):
    tol_j = (D + 1) 2^-24 (|e_j|^2 + 2 sum_d |z_d e_jd|).
A row whose best and second-best float64 distances lie within tol_best + tol_second of each other is "in the band": there an f32
evaluation may legitimately pick either.  Outside the band the index must be the float64 argmin."""
import functools
import os

import pytest
import torch

from helpers import guarded_ops, rel_l2

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import _lib, functional as HF, ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------


def _scores64(z, e):
    """(score [rows, N], tol [rows, N]) in float64 for z [rows, D], e [N, D]: |e_j|^2 - 2 z . e_j (|z|^2 is the same for every j
    of a row) and the error bound of its f32 evaluation"""
    z64, e64 = z.double(), e.double()
    d = z.shape[1]
    sq = (e64 * e64).sum(1)
    score = sq[None, :] - 2.0 * (z64 @ e64.t())
    tol = (d + 1) * U * (sq[None, :] + 2.0 * (z64.abs() @ e64.abs().t()))
    return score, tol


def _reference(z, e):
    """dict: argmin [rows], in_band [rows] (best and second best within tol_best + tol_second), score / tol matrices"""
    score, tol = _scores64(z, e)
    arg = score.argmin(1)
    rows = torch.arange(z.shape[0])
    if e.shape[0] > 1:
        two, at = torch.topk(score, 2, dim=1, largest=False)
        band = (two[:, 1] - two[:, 0]) <= tol[rows, at[:, 0]] + tol[rows, at[:, 1]]
    else:
        band = torch.zeros(z.shape[0], dtype=torch.bool)
    return dict(argmin=arg, band=band, score=score, tol=tol)


def _assert_d64_bound(idx, ref, what):
    """every row, none excused: d64(idx) <= min d64 + tol_idx + tol_best"""
    rows = torch.arange(idx.numel())
    idx = idx.reshape(-1).cpu()
    got, best = ref["score"][rows, idx], ref["score"][rows, ref["argmin"]]
    bound = best + ref["tol"][rows, idx] + ref["tol"][rows, ref["argmin"]]
    bad = torch.nonzero(got > bound).view(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows beyond the float64 bound, first {bad[:5].tolist()}"


def _device_z(G, z_rows, shape, channels_last, dtype):
    """z rows [B h w, D] (pixel-major) as the [B, D, h, w] device tensor of that memory layout, inside a poisoned buffer"""
    b, h, w = shape
    d = z_rows.shape[1]
    pix = z_rows.view(b, h, w, d).to(dtype)
    if channels_last:
        return G.poisoned(pix.to(DEV)).permute(0, 3, 1, 2)
    return G.poisoned(pix.permute(0, 3, 1, 2).contiguous().to(DEV))


def _rows_of(t):
    """[B, D, h, w] -> pixel-major rows [B h w, D] on the CPU"""
    return t.detach().cpu().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---------------------------------------------------------------------------------------------
# kernel level: random cases
# ---------------------------------------------------------------------------------------------

# (D, N, (B, h, w), seed): six base cases (the zoo's f4 / f8 codebooks on 512 rows, odd sizes, D = 1, the widest
# code, one code), then D = 2 / 12 / 24 (the padded widths 16 and 32 with one row per lane), then the sizes around the threshold
# where a lane takes two rows (TWO_ROWS rows: 65535 is the largest one-row launch; 257 x 257 leaves one row in the last
# workgroup) for every padded width that is compiled
TWO_ROWS = 2 * 64 * _lib.DEFINES["CFHIP_VQ_TWO_ROWS_MIN_GROUPS"]
RANDOM_CASES = [
    (3, 8192, (2, 16, 16), 1), (4, 16384, (2, 16, 16), 2), (8, 1000, (3, 7, 5), 3), (1, 17, (4, 4, 4), 4), (64, 300, (2, 13, 5), 5),
    (4, 1, (1, 3, 3), 6),
    (2, 40, (1, 9, 7), 7), (12, 90, (2, 5, 7), 8), (24, 90, (2, 5, 7), 9),
    (3, 130, (1, 255, 257), 10), (3, 130, (1, 257, 257), 11), (4, 50, (1, 256, 256), 12), (1, 9, (1, 256, 256), 13),
    (2, 9, (1, 256, 256), 14), (6, 50, (1, 256, 256), 15), (12, 50, (1, 256, 256), 16), (24, 50, (1, 256, 256), 17),
    (64, 70, (1, 256, 256), 18),
]
assert TWO_ROWS == 65536 and 255 * 257 == TWO_ROWS - 1


BASE_CASES = 6  # the first six: no row of theirs is in the band (checked on the CPU beforehand; asserted below)


@functools.lru_cache(maxsize=None)
def _random_case(d, n, shape, seed):
    """inputs and the float64 reference of one case, computed once and shared by its runs (never modified): the argmin of every
    row, and for the rows in the band their whole float64 score / tol rows"""
    b, h, w = shape
    g = _gen(seed)
    z = torch.randn(b * h * w, d, generator=g).to(BF16).float()
    e = torch.randn(n, d, generator=g)
    ref = _reference(z, e)
    band = torch.nonzero(ref["band"]).view(-1)
    return z, e, ref["argmin"], band, ref["score"][band].clone(), ref["tol"][band].clone()


def _check_indices(idx, case, what):
    """the float64 argmin on every row outside the band; d64(idx) <= min d64 + tol_idx + tol_best on the rows inside it"""
    _, _, want, band, score, tol = case
    idx = idx.reshape(-1).cpu()
    outside = torch.ones(idx.numel(), dtype=torch.bool)
    outside[band] = False
    bad = torch.nonzero((idx != want) & outside).view(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows differ from the float64 argmin, first {bad[:5].tolist()}"
    if band.numel():
        k = torch.arange(band.numel())
        got, best = idx[band], want[band]
        assert bool((score[k, got] <= score[k, best] + tol[k, got] + tol[k, best]).all()), f"{what}: a row in the band is beyond the float64 bound"
    return idx


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("d,n,shape,seed", RANDOM_CASES, ids=[f"D{c[0]}-N{c[1]}-{c[2][0] * c[2][1] * c[2][2]}rows" for c in RANDOM_CASES])
def test_nearest_random(G, d, n, shape, seed, dtype):
    """The six base cases have no row in the band (asserted), so there indices == float64 argmin on every row with nothing
    left out; the cases added here (tens of thousands of rows) may have a handful, which must meet the float64 bound.  NCHW and
    channels-last memory give identical indices; z_q is the codebook row bit for bit at scale 1 and float32(scale) * row, one
    f32 product, at scale 0.18215; nothing around the outputs is written."""
    case = _random_case(d, n, shape, seed)
    z, e, _, band = case[:4]
    if RANDOM_CASES.index((d, n, shape, seed)) < BASE_CASES:
        assert band.numel() == 0, f"{band.numel()} rows of this case are in the band"
    assert band.numel() <= 16, band.numel()
    b, h, w = shape
    ed = G.poisoned(e.to(DEV))
    sq = ops.vq_code_sqnorm(ed)
    sq_want = torch.zeros(n)
    for k in range(d):  # the fmaf chain in d order from 0: the exact product and sum in float64, rounded to f32 once per step
        sq_want = (sq_want.double() + e[:, k].double() * e[:, k].double()).float()
    assert torch.equal(sq.cpu(), sq_want), "code_sq is not the fmaf chain in d order"
    got = {}
    for channels_last in (False, True):
        zd = _device_z(G, z, shape, channels_last, dtype)
        assert zd.is_contiguous() or zd.is_contiguous(memory_format=torch.channels_last)
        idx, z_q = ops.vq_nearest(zd, ed, code_sq=sq)
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (b, h, w)
        assert z_q.dtype == F32 and tuple(z_q.shape) == (b, d, h, w) and z_q.is_contiguous()
        flat = _check_indices(idx, case, f"channels_last={channels_last}")
        assert torch.equal(_rows_of(z_q), e[flat]), "z_q at scale 1 is not the codebook row bit for bit"
        got[channels_last] = idx
    assert torch.equal(got[False], got[True])
    flat = got[False].reshape(-1).cpu()
    scale = 0.18215
    idx2, z_q2 = ops.vq_nearest(_device_z(G, z, shape, False, dtype), ed, scale_factor=scale)  # (code_sq computed inside)
    assert torch.equal(idx2, got[False])
    assert torch.equal(_rows_of(z_q2), torch.tensor(scale, dtype=F32) * e[flat]), "z_q is not one f32 product scale * row"
    idx3, none = ops.vq_nearest(_device_z(G, z, shape, True, dtype), ed, code_sq=sq, want_z_q=False)
    assert none is None and torch.equal(idx3, got[False])


# ---------------------------------------------------------------------------------------------
# kernel level: adversarial codebooks, chunk boundaries, NaN
# ---------------------------------------------------------------------------------------------

ADV_SHAPE = (2, 10, 5)  # 100 rows
ADV_N = 1000


def _run(G, z, e, shape=ADV_SHAPE, channels_last=False, dtype=BF16):
    idx, z_q = ops.vq_nearest(_device_z(G, z, shape, channels_last, dtype), G.poisoned(e.to(DEV)))
    assert torch.equal(_rows_of(z_q), e[idx.reshape(-1).cpu()])
    return idx.reshape(-1).cpu()


def test_identical_nearest_rows_give_the_lower_index(G):
    """rows 5 and 900 of the codebook are the same vector and the nearest of every pixel: index 5 (for D = 4 they are scanned by
    different waves of the workgroup, 900 first in time or not)"""
    g = _gen(31)
    c = torch.randn(4, generator=g)
    z = (c + 0.01 * torch.randn(100, 4, generator=g)).to(BF16).float()
    e = c + 3.0 + torch.randn(ADV_N, 4, generator=g).abs()  # every other code is far on one side
    e[5] = c
    e[900] = c
    assert bool((_reference(z, e)["score"].argmin(1) == 5).all())
    for channels_last in (False, True):
        assert bool((_run(G, z, e, channels_last=channels_last) == 5).all())
    e[3] = c  # and within one wave's range
    assert bool((_run(G, z, e) == 3).all())


def test_all_rows_identical_give_index_zero(G):
    g = _gen(32)
    z = torch.randn(100, 4, generator=g).to(BF16).float()
    e = torch.randn(4, generator=g).expand(ADV_N, 4).contiguous()
    for dtype in (BF16, F32):
        assert bool((_run(G, z, e, dtype=dtype) == 0).all())


def test_neighbouring_codes_stay_within_the_float64_bound(G):
    """row b of the codebook is nextafter(row a): the two scores differ by less than one rounding, so either index is an f32
    answer; what must hold for every row is d64(idx) <= min d64 + tol_idx + tol_best"""
    g = _gen(33)
    c = torch.randn(4, generator=g)
    z = (c + 0.01 * torch.randn(100, 4, generator=g)).to(BF16).float()
    e = c + 3.0 + torch.randn(ADV_N, 4, generator=g).abs()
    e[700] = c
    e[40] = torch.nextafter(c, torch.full_like(c, float("inf")))
    ref = _reference(z, e)
    assert int(ref["band"].sum()) == 100  # every row is in the band: this case is about the bound, not about equality
    idx = _run(G, z, e)
    assert bool(((idx == 40) | (idx == 700)).all())
    _assert_d64_bound(idx, ref, "nextafter codes")


def test_default_initialised_codebook(G):
    """the module's own uniform(-1 / N, 1 / N) codebook: codes three orders of magnitude smaller than the pixels"""
    torch.manual_seed(34)
    e = C.VQCodebook(ADV_N, 4).embedding.weight.detach().clone()
    assert float(e.abs().max()) <= 1.0 / ADV_N
    z = torch.randn(100, 4, generator=_gen(34)).to(BF16).float()
    ref = _reference(z, e)
    idx = _run(G, z, e)
    _assert_d64_bound(idx, ref, "default-initialised codebook")
    out = ~ref["band"]
    assert torch.equal(idx[out], ref["argmin"][out])


VQ_CHUNK_D4 = 1024  # codes of a D = 4 codebook the kernel holds in LDS at once (cfhip_vq_chunk(4): 8192 floats / stride 8)


@pytest.mark.parametrize("n", [VQ_CHUNK_D4 + 1, VQ_CHUNK_D4 - 1, 2 * VQ_CHUNK_D4 + 52], ids=["chunk+1", "chunk-1", "2chunks+52"])
def test_chunk_boundaries(G, n):
    """N one past, one short of, and beyond twice what the kernel holds at once; the last code (alone in its chunk when N =
    chunk + 1) and the middle one are made the exact nearest of two rows"""
    assert ops.vq_chunk(4) == VQ_CHUNK_D4
    shape = (2, 7, 5)
    g = _gen(35 + n)
    z = torch.randn(70, 4, generator=g).to(BF16).float()
    e = torch.randn(n, 4, generator=g)
    e[n - 1] = z[3]
    e[(n - 1) // 2] = z[4]
    ref = _reference(z, e)
    assert int(ref["band"].sum()) == 0 and int(ref["argmin"][3]) == n - 1 and int(ref["argmin"][4]) == (n - 1) // 2
    for channels_last in (False, True):
        idx = _run(G, z, e, shape=shape, channels_last=channels_last)
        assert torch.equal(idx, ref["argmin"])
    assert len(set(ref["argmin"].tolist())) > 20 and int(ref["argmin"].max()) >= min(n - 1, VQ_CHUNK_D4)


def test_a_nan_row_stays_in_range_and_alone(G):
    g = _gen(36)
    z = torch.randn(100, 4, generator=g).to(BF16).float()
    e = torch.randn(ADV_N, 4, generator=g)
    clean = _run(G, z, e)
    assert torch.equal(clean, _reference(z, e)["argmin"])
    z_nan = z.clone()
    z_nan[17] = float("nan")
    for dtype in (BF16, F32):
        idx = ops.vq_nearest(_device_z(G, z_nan, ADV_SHAPE, False, dtype), G.poisoned(e.to(DEV)))[0].reshape(-1).cpu()
        assert 0 <= int(idx[17]) < ADV_N
        keep = torch.arange(100) != 17
        assert torch.equal(idx[keep], clean[keep])


def test_wrapper_refusals():
    e = torch.zeros(8, 4, device=DEV)
    with pytest.raises(NotImplementedError, match="64"):
        ops.vq_nearest(torch.zeros(1, 65, 2, 2, device=DEV), torch.zeros(8, 65, device=DEV))
    with pytest.raises(ValueError, match="for this codebook"):
        ops.vq_nearest(torch.zeros(1, 3, 2, 2, device=DEV), e)
    with pytest.raises(TypeError):
        ops.vq_nearest(torch.zeros(1, 4, 2, 2, device=DEV, dtype=torch.float16), e)
    with pytest.raises(ValueError, match="NCHW or channels-last"):
        ops.vq_nearest(torch.zeros(1, 4, 2, 4, device=DEV)[..., ::2], e)
    with pytest.raises(ValueError, match="code_sq"):
        ops.vq_nearest(torch.zeros(1, 4, 2, 2, device=DEV), e, code_sq=torch.zeros(7, device=DEV))


# ---------------------------------------------------------------------------------------------
# model level, against the reference's fp32 CPU run; yardstick = the reference's own bf16-autocast run
# ---------------------------------------------------------------------------------------------

YARDSTICK = 1.1


def seeded_state(shapes, seed):
    """tools/gen_first_stage_golden.py::seeded_state, line for line: the parameters no fixture stores (the 2-D codebook falls
    under the filter rule)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        n = torch.randn(shape, generator=g)
        if len(shape) == 1:
            out[name] = 1.0 + 0.1 * n if name.endswith("weight") else 0.1 * n
        else:
            out[name] = n / float(torch.Size(shape[1:]).numel()) ** 0.5
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    return torch.load(os.path.join(GOLDEN, "ae_vq_small.pt"), map_location="cpu", weights_only=False)


def _small_vq(key):
    g = _golden()[key]
    m = C.AttentionAutoEncoderVQ(**g["cfg"])
    state = seeded_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, g["seed"])
    m.load_state_dict(state, strict=True)
    return m.to(DEV).eval(), g, state


def _yardstick(got, want, ref_bf16, what):
    ours, theirs = rel_l2(got, want), rel_l2(ref_bf16, want)
    print(f"{what}: ours {ours:.3e}, reference bf16 {theirs:.3e}, ratio {ours / theirs:.2f}")
    assert ours <= YARDSTICK * theirs, f"{what}: rel-L2 {ours:.3e} vs fp32 > {YARDSTICK} x the reference's bf16 {theirs:.3e} (ratio {ours / theirs:.2f})"


@pytest.mark.parametrize("key", ["e4", "e3"])
def test_ae_vq_against_reference(key):
    m, g, state = _small_vq(key)
    e = state["codebook.embedding.weight"]
    with torch.no_grad():
        out = m.encode(g["x"].to(DEV))
    assert out.z_q_g is not None and tuple(out.z_q_g.shape) == tuple(g["z_q_g"].shape)
    # (a) z_e
    z_e = HF.to_nchw(out.z_e)
    assert tuple(z_e.shape) == tuple(g["z_e"].shape)
    _yardstick(z_e, g["z_e"], g["z_e_bf16"], f"ae_vq {key} z_e")
    # (b) the indices on HIP's own z_e: inside the float64 bound on every row, the float64 argmin outside the band
    ref = _reference(_rows_of(z_e.float()), e)
    idx = out.indices.reshape(-1).cpu()
    assert tuple(out.indices.shape) == tuple(g["indices"].shape) and out.indices.dtype == torch.int64
    _assert_d64_bound(idx, ref, f"ae_vq {key} indices")
    outside = ~ref["band"]
    assert torch.equal(idx[outside], ref["argmin"][outside]), f"{int(ref['band'].sum())} rows in the band"
    assert torch.equal(_rows_of(out.z_q), e[idx])
    assert torch.equal(out.z_q_g.cpu(), e[idx].view(out.z_q_g.shape))
    # (c) pixels whose code differs from the fp32 reference's, against the reference's own mixed-precision run
    flips = int((idx != g["indices"].reshape(-1)).sum())
    print(f"ae_vq {key}: HIP flips {flips}, reference bf16 flips {g['flips_bf16']} of {idx.numel()} pixels")
    assert flips <= 2 * g["flips_bf16"] + 2
    # (d) decode of the fixture's z_q
    with torch.no_grad():
        decoded = HF.to_nchw(m.decode(C.DecoderInputs(z=g["z_q"].to(DEV))))
        rec = m.reconstruct(g["x"].to(DEV))
        again = m.decode(C.DecoderInputs(z=out.z_q))
    _yardstick(decoded, g["decoded"], g["decoded_bf16"], f"ae_vq {key} decode(z_q)")
    assert torch.equal(rec, again)


def test_ae_vq_loading_z_q_g_and_refusals():
    """strict loading of the seeded state; the codebook fed the reference's z_q (f32 NCHW, every pixel an exact codebook row)
    finds the reference's indices again, and z_q_g is then the reference's pixel-major reshape; the forward's dictionary; a
    grad-requiring input raises"""
    m, g, state = _small_vq("e4")
    m2 = C.AttentionAutoEncoderVQ(**g["cfg"])
    with pytest.raises(RuntimeError):
        m2.load_state_dict({k: v for k, v in state.items() if k != "codebook.embedding.weight"}, strict=True)
    with torch.no_grad():
        out = m.codebook(g["z_q"].to(DEV), return_z_q_g=True)
        plain = m.codebook(g["z_q"].to(DEV).contiguous(memory_format=torch.channels_last))
    assert torch.equal(out.indices.cpu(), g["indices"]) and torch.equal(plain.indices, out.indices) and plain.z_q_g is None
    # the reference's z_q is its straight-through expression z_e + (z_q - z_e), two f32 roundings away from the codebook row that
    # the kernel returns bit for bit; its z_q_g is the plain gather
    e = state["codebook.embedding.weight"]
    assert torch.equal(out.z_q.cpu(), e[g["indices"]].permute(0, 3, 1, 2))
    assert bool(((out.z_q.cpu() - g["z_q"]).abs() <= 2 * U * (g["z_e"].abs() + 2 * g["z_q"].abs())).all())
    assert torch.equal(out.z_q_g.cpu(), g["z_q_g"])
    assert not torch.equal(out.z_q_g.cpu(), g["z_q"])  # (the reshape is not the permute)
    sq = m.codebook.code_sqnorm()
    assert m.codebook.code_sqnorm() is sq  # cached ...
    with torch.no_grad():
        m.codebook.embedding.weight.mul_(1.0)
    assert m.codebook.code_sqnorm() is not sq and torch.equal(m.codebook.code_sqnorm(), sq)  # ... until the weight's version moves
    with torch.no_grad():
        res = m(g["x"].to(DEV), return_z_q_g=False)
        z = m.generate_z(3)
    assert sorted(res) == ["indices", "predictions", "z_e", "z_q", "z_q_g"] and res["z_q_g"] is None
    assert tuple(res["predictions"].shape) == (2, 3, 16, 16) and tuple(z.shape) == (3, 4, 8, 8) and z.dtype == F32
    with pytest.raises(NotImplementedError, match="§8"):
        m.encode(g["x"].to(DEV).requires_grad_(True))
    with pytest.raises(NotImplementedError, match="apply_tanh"):
        m.decode(C.DecoderInputs(z=out.z_q, apply_tanh=True))


# ---------------------------------------------------------------------------------------------
# the latent path: DDPMTrainStep / DiffusionSampler with a VQ first stage
# ---------------------------------------------------------------------------------------------

SCALE = 0.5


def _small_unet():
    """the small UNet of test_gpu_first_stage.py (4 latent channels in and out), zero-initialised convolutions filled"""
    from cflearn_amd import modules as M

    torch.manual_seed(7)
    unet = M.UNetDiffuser(4, 4, num_head_channels=32, use_spatial_transformer=True, start_channels=32, num_res_blocks=1,
                          attention_downsample_rates=(1,), channel_multipliers=(1, 2))
    gen = _gen(8)
    with torch.no_grad():
        for p in unet.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=gen) * (0.5 / max(1, p[0].numel()) ** 0.5))
    return unet.to(DEV)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_vq_latent_train_step(use_graph):
    """three steps on images through the VQ first stage against three steps of an engine without a first stage fed
    ops.vq_nearest's scaled latent: the same loss and the same parameters, bit for bit; the first stage stays frozen"""
    from cflearn_amd.diffusion import DDPMTrainStep, NoiseSchedule

    vq, g, _ = _small_vq("e4")
    before = {k: v.clone() for k, v in vq.state_dict().items()}
    img = g["x"].to(DEV)
    gen = _gen(41)
    batches = [(torch.randint(0, 1000, (2,), generator=gen).to(DEV), torch.randn((2, 4, 8, 8), generator=gen).to(DEV)) for _ in range(3)]
    ts = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3, use_graph=use_graph, first_stage=vq, first_stage_scale_factor=SCALE)
    assert not vq.training and all(not p.requires_grad for p in vq.parameters())
    arena_ids = {id(p) for p in ts.arena.params}
    assert arena_ids and not any(id(p) in arena_ids for p in vq.parameters())
    with torch.no_grad():
        z_e = vq.to_embedding(vq.generator.encoder.encode(img))
        _, latent = ops.vq_nearest(z_e, vq.codebook.embedding.weight.detach(), scale_factor=SCALE)
    assert tuple(latent.shape) == (2, 4, 8, 8) and latent.dtype == F32 and tuple(ts.latent_shape(img)) == (2, 4, 8, 8)
    plain = DDPMTrainStep(_small_unet(), NoiseSchedule(device=DEV), lr=1e-3, use_graph=use_graph)
    kwargs = [dict(), dict(deterministic=True), dict(seed=5)]  # accepted, and without effect: nothing is drawn
    losses, losses_plain = [], []
    for (t, eps), kw in zip(batches, kwargs):
        losses.append(ts.step(img, timesteps=t, noise=eps, **kw).item())
        losses_plain.append(plain.step(latent, timesteps=t, noise=eps).item())
    HF.SideStream.join()
    torch.cuda.synchronize()
    assert ts.steps_done == 3 and len(set(losses)) == 3
    assert losses == losses_plain, (losses, losses_plain)
    for (n, p), (_, q) in zip(ts.unet.named_parameters(), plain.unet.named_parameters()):
        assert torch.equal(p, q), f"{n}: the updated parameters differ from the step fed the hand-made latent"
    for k, v in vq.state_dict().items():
        assert torch.equal(v, before[k]), f"first stage {k} changed"
    assert all(p.grad is None for p in vq.parameters())
    if use_graph:
        assert ts._static["fs_noise"] is None  # no normals in front of the recorded graph


def test_vq_latent_sampler_decodes():
    from cflearn_amd.diffusion import NoiseSchedule, make_sampler

    vq, _, _ = _small_vq("e4")
    unet = _small_unet().eval()
    z = torch.randn((2, 4, 8, 8), generator=_gen(43)).to(DEV)
    sampler = make_sampler("ddim", unet, NoiseSchedule(device=DEV), first_stage=vq, first_stage_scale_factor=SCALE)
    img = sampler.sample(z, num_steps=4)
    latent = sampler.sample(z, num_steps=4, return_latent=True)
    assert tuple(latent.shape) == (2, 4, 8, 8) and latent.dtype == F32 and tuple(img.shape) == (2, 3, 16, 16)
    with torch.no_grad():
        want = vq.decode(C.DecoderInputs(z=latent / SCALE))  # LDM.decode: the latent is not quantised
    assert torch.equal(img, want)
