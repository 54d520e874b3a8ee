"""HIP kernels at their edges, per element against float64 CPU references, with guarded outputs and poisoned inputs.

Every case runs under `guarded_ops` (outputs the wrappers allocate start as NaN between byte guards), reads floating
inputs from NaN-surrounded buffers (`poisoned`), compares each output element with a float64 reference on the same
bf16-rounded inputs (`assert_elementwise`, or `torch.equal` where the code documents bit-exactness) and ends with the
guard check.  Shapes sit at the edges: the 4-wide loops' scalar tails, the last partial slice / tile / row, N around
multiples of 8.  Error models (one line each at the call):
  * "one rounding": the kernel computes in f32 and rounds once to the output type -> ulps = 1.
  * "f32 sum of depth d": a reduction whose longest dependent chain of f32 additions is d -> k = d, cond = sum |terms|.
  * "fast intrinsics": v_exp_f32 / v_rcp_f32 (1 ulp each) and their argument roundings -> a few units of k with cond
    = |result| * (1 + |argument|); the A&S erf of the GELU adds 1.5e-7 |x| (~1.3 units of 2^-24 |x|)."""
import math

import pytest
import torch

from helpers import _gelu64, _gelu_grad64, _gemm_ref, _sig64, assert_elementwise, attn_ref, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# every n % 4; the last two lie beyond one pass of the capped grid (2048 blocks x 256 threads x 4 elements = 1 << 21): second and third trip
EDGE_N = [1, 2, 3, 4, 5, 6, 63, 64, 65, 66, 255, 257, (1 << 20) + 2, (1 << 20) + 3, (1 << 21) + 1024 + 3, 2 * (1 << 21) + 5]


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=_gen(seed), dtype=torch.float64) * scale).to(dtype)


def _dev(g, t):
    """a poisoned device copy of a floating CPU tensor"""
    return g.poisoned(t.to(DEV))


# ---------------------------------------------------------------------------------------------
# casts and element-wise
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", EDGE_N)
def test_casts_split_join_bit_exact(G, n):
    x = _randn(n, n, 3.0)
    xd = _dev(G, x)
    assert torch.equal(ops.to_bf16(xd).cpu(), x.to(BF16))  # RNE, bit-exact
    xb = x.to(BF16)
    assert torch.equal(ops.to_f32(_dev(G, xb)).cpu(), xb.float())
    hi, lo = ops.split_f32(xd)
    want_hi = x.to(BF16)
    assert torch.equal(hi.cpu(), want_hi) and torch.equal(lo.cpu(), (x - want_hi.float()).to(BF16))
    assert torch.equal(ops.join_bf16x2(_dev(G, want_hi), _dev(G, lo.cpu())).cpu(), want_hi.float() + lo.cpu().float())
    # out= into a guarded destination
    out = G.empty((n,), dtype=BF16, device=DEV)
    ops.to_bf16(xd, out=out)
    assert torch.equal(out.cpu(), x.to(BF16))
    G.check()


@pytest.mark.parametrize("n", EDGE_N)
def test_bf16_elementwise(G, n):
    a = _randn(n, 10 + n, 2.0).clamp(-6, 6).to(BF16)
    b = _randn(n, 20 + n, 2.0).clamp(-6, 6).to(BF16)
    ad, bd = _dev(G, a), _dev(G, b)
    a64, b64 = a.double(), b.double()
    # add: one rounding of an exact f32 sum
    assert_elementwise(ops.add(ad, bd), a64 + b64, out_dtype=BF16, what=f"add n={n}")
    # GELU: fast intrinsics + A&S erf; cond = |x| (1 + x^2) bounds the erf, exp-argument and rcp errors
    c = a64.abs() * (1 + a64 * a64)
    assert_elementwise(ops.gelu_fwd(ad), _gelu64(a64), out_dtype=BF16, cond=c, k=8, what=f"gelu n={n}")
    cb = b64.abs() * (1 + b64 * b64) * (1 + a64.abs())
    assert_elementwise(ops.gelu_bwd(ad, bd), a64 * _gelu_grad64(b64), out_dtype=BF16, cond=cb, k=8, what=f"gelu_bwd n={n}")
    q = 1.702 * a64
    assert_elementwise(ops.quick_gelu_fwd(ad), a64 * _sig64(q), out_dtype=BF16, cond=a64.abs() * (1 + q.abs()), k=8,
                       what=f"quick_gelu n={n}")
    qb = 1.702 * b64
    s = _sig64(qb)
    assert_elementwise(ops.quick_gelu_bwd(ad, bd), a64 * s * (1 + qb * (1 - s)), out_dtype=BF16,
                       cond=a64.abs() * (1 + qb.abs()) ** 2, k=8, what=f"quick_gelu_bwd n={n}")
    # leaky ReLU: one rounding
    assert_elementwise(ops.leaky_relu_fwd(ad, 0.2), torch.where(a64 > 0, a64, 0.2 * a64), out_dtype=BF16, what="leaky fwd")
    assert_elementwise(ops.leaky_relu_bwd(bd, ad, 0.2), torch.where(a64 > 0, b64, 0.2 * b64), out_dtype=BF16, what="leaky bwd")
    G.check()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 65, 66, 257, (1 << 20) + 3, (1 << 21) + 1024 + 3, 2 * (1 << 21) + 5])
def test_f32_silu_ema(G, n):
    x = _randn(n, 30 + n, 3.0)
    dy = _randn(n, 40 + n)
    xd, dyd = _dev(G, x), _dev(G, dy)
    x64, dy64 = x.double(), dy.double()
    s = _sig64(x64)
    # SiLU f32: fast intrinsics (exp2 / rcp, 1 ulp each, and the rounded exp2 argument)
    assert_elementwise(ops.silu_f32_fwd(xd), x64 * s, out_dtype=F32, ulps=2, cond=(x64 * s).abs() * (1 + x64.abs()), k=8,
                       what=f"silu f32 n={n}")
    assert_elementwise(ops.silu_f32_bwd(dyd, xd), dy64 * s * (1 + x64 * (1 - s)), out_dtype=F32, ulps=2,
                       cond=dy64.abs() * (1 + x64.abs()) ** 2, k=8, what=f"silu_bwd f32 n={n}")
    # EMA: two rounded products and a rounded sum, bit-exact with the torch expression
    ema = _randn(n, 50 + n)
    emad = G.poisoned(ema.to(DEV))
    ops.ema_update(emad, xd, 0.999)
    omd, dec = torch.tensor(1.0 - 0.999, dtype=F32), torch.tensor(0.999, dtype=F32)
    assert torch.equal(emad.cpu(), omd * x + dec * ema)
    G.check()


def test_q_sample_bit_exact(G):
    b, inner = 5, 65
    x, noise = _randn((b, inner), 1), _randn((b, inner), 2)
    sac, s1m = torch.rand(1000, generator=_gen(3)), torch.rand(1000, generator=_gen(4))
    t = torch.tensor([0, 999, 3, 500, 999])
    xt = ops.q_sample(_dev(G, x), _dev(G, noise), G.index(t.to(DEV)), _dev(G, sac), _dev(G, s1m))
    want = sac[t][:, None] * x + s1m[t][:, None] * noise
    assert torch.equal(xt.cpu(), want)
    xt16 = ops.q_sample(_dev(G, x), _dev(G, noise), G.index(t.to(DEV)), _dev(G, sac), _dev(G, s1m), out_dtype=BF16)
    assert torch.equal(xt16.cpu(), want.to(BF16))
    G.check()


@pytest.mark.parametrize("r,c", [(1, 1), (3, 5), (63, 65), (64, 64), (65, 257), (257, 63)])
def test_transposes_and_strided_copies(G, r, c):
    x = _randn((r, c), r * c).to(BF16)
    assert torch.equal(ops.transpose(_dev(G, x)).cpu(), x.t().contiguous())
    xb = _randn((3, r, c), r + c)
    assert torch.equal(ops.transpose_batched(_dev(G, xb)).cpu(), xb.transpose(1, 2).to(BF16))
    assert torch.equal(ops.transpose_batched(_dev(G, xb.to(BF16))).cpu(), xb.to(BF16).transpose(1, 2))
    # copy_strided: the concatenation of a skip connection, into a guarded destination
    batch, na, nb = 3, 4 * c, 4 * r
    src_a, src_b = _randn((batch, na), 7).to(BF16), _randn((batch, nb), 8).to(BF16)
    dst = G.empty((batch, na + nb), dtype=BF16, device=DEV)
    ops.copy_strided2(_dev(G, src_a), dst, na, na, na + nb, _dev(G, src_b), dst, nb, nb, na + nb, batch, dst_b_off=na)
    assert torch.equal(dst.cpu(), torch.cat([src_a, src_b], 1))
    dst2 = G.empty((batch, na + nb), dtype=BF16, device=DEV)
    ops.copy_strided(_dev(G, src_a), dst2, batch, na, na, na + nb)
    ops.copy_strided(_dev(G, src_b), dst2, batch, nb, nb, na + nb, dst_off=na)
    assert torch.equal(dst2.cpu(), torch.cat([src_a, src_b], 1))
    G.check()


def test_misaligned_views_are_refused():
    """The 4-wide kernels need 8 / 16-byte aligned pointers: a view one element into its storage is refused by the
    C-side checks before any launch, never computed."""
    xf = torch.randn(65, device=DEV)
    xb = xf.to(BF16)
    for call in (lambda: ops.to_bf16(xf[1:]), lambda: ops.to_f32(xb[1:]), lambda: ops.gelu_fwd(xb[1:]),
                 lambda: ops.add(xb[1:], xb[:-1]), lambda: ops.split_f32(xf[1:]), lambda: ops.leaky_relu_fwd(xb[1:], 0.1),
                 lambda: ops.ema_update(xf[1:], xf[:-1], 0.9)):
        with pytest.raises(RuntimeError, match="misaligned|aligned"):
            call()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# reductions and losses
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 257, 258, (1 << 20) + 3])
def test_sumsq_and_dot(G, n):
    a, b = _randn(n, 60 + n), _randn(n, 70 + n)
    a[-3:], b[-3:] = 100.0, -100.0  # a heavy tail: leaving out any element of the 4-wide loop's tail exceeds the bound at every n
    a64, b64 = a.double(), b.double()
    blocks = min(max(1, -(-n // 2048)), 1024)
    depth = -(-n // (blocks * 256)) + 8 + blocks  # per-thread chain + wave/workgroup tree + one atomic per workgroup
    assert_elementwise(ops.sumsq(_dev(G, a)), (a64 * a64).sum(), out_dtype=F32, cond=(a64 * a64).sum(), k=depth + 1,
                       what=f"sumsq n={n}")
    dot = ops.dot_f32(_dev(G, a), _dev(G, b))
    blocks_d = min(-(-n // 256), 1024)  # embed.hip: cfhip_dot_f32's grid
    depth_d = -(-n // (blocks_d * 256)) + 8 + blocks_d
    assert_elementwise(dot, (a64 * b64).sum(), out_dtype=F32, cond=(a64 * b64).abs().sum(), k=depth_d + 1,
                       what=f"dot n={n}")
    G.check()


@pytest.mark.parametrize("m,n", [(1, 8), (3, 16), (31, 8), (33, 64), (255, 520), (257, 1000), (5000, 72), (77, 13)])
def test_colsum_every_slice(G, m, n):
    """colsum's partial kernel cuts the rows into slices of >= 32 rows; the last one is short.  Rows get distinct
    magnitudes so that a missing / repeated row of any slice shows per column."""
    x = (_randn((m, n), m + n) * torch.linspace(1, 3, m, dtype=F32)[:, None]).to(BF16)
    x64 = x.double()
    slices = min(max(1, -(-m // 32)), 256)
    depth = -(-m // slices) + 4 + slices  # a wave's rows of one slice + 4 waves + the column reduce over slices
    want, cond = x64.sum(0), x64.abs().sum(0)
    assert_elementwise(ops.colsum(_dev(G, x)), want, out_dtype=F32, cond=cond, k=depth, what=f"colsum {m}x{n}")
    # out= inside a guarded buffer, accumulating onto 1.5
    out = G.out2d(1, n, n, F32, DEV, fill=1.5)
    ops.colsum(_dev(G, x), out=out.view(n), accumulate=True)
    assert_elementwise(out.view(n), want + 1.5, out_dtype=F32, cond=cond + 1.5, k=depth + 1, what=f"colsum acc {m}x{n}")
    # colreduce over f32 rows
    xf = _randn((m, n), 3 * m + n)
    depth_r = -(-m // 128) + 2 + 32
    assert_elementwise(ops.colreduce_f32(_dev(G, xf)), xf.double().sum(0), out_dtype=F32, cond=xf.double().abs().sum(0),
                       k=depth_r, what=f"colreduce {m}x{n}")
    oa, ob = G.out2d(1, n, n, F32, DEV, fill=0.25), G.out2d(1, n, n, F32, DEV, fill=-0.5)
    xf2 = _randn((m, n), 5 * m + n)
    ops.colreduce2_f32(_dev(G, xf), _dev(G, xf2), oa.view(n), ob.view(n), True)
    assert_elementwise(oa.view(n), xf.double().sum(0) + 0.25, out_dtype=F32, cond=xf.double().abs().sum(0) + 1, k=depth_r + 1,
                       what="colreduce2 a")
    assert_elementwise(ob.view(n), xf2.double().sum(0) - 0.5, out_dtype=F32, cond=xf2.double().abs().sum(0) + 1, k=depth_r + 1,
                       what="colreduce2 b")
    G.check()


@pytest.mark.parametrize("b,inner", [(1, 1), (3, 5), (4, 63), (5, 257), (2, (1 << 16) + 3)])
def test_mse_and_diffusion_losses(G, b, inner):
    pred = _randn((b, inner), b + inner).to(BF16)
    target = _randn((b, inner), 2 * b + inner)
    w = torch.rand(b, generator=_gen(b)) + 0.5
    d = pred.double() - target.double()
    blocks = min(max(1, -(-b * inner // 256)), 1024)
    depth = -(-b * inner // (blocks * 256)) + 8 + blocks
    loss, dpred = ops.mse_loss(_dev(G, pred), _dev(G, target), 0.5)
    # loss: f32 sum of the squares (and one division per workgroup); dpred: one rounding of an f32 product chain
    assert_elementwise(loss, (d * d).mean(1).sum(), out_dtype=F32, cond=(d * d).sum() / inner * 2, k=depth + 2, what="mse loss")
    assert_elementwise(dpred, 2 * 0.5 * d / inner, out_dtype=BF16, cond=d.abs() / inner, k=4, what="mse dpred")
    for lt in ("l2", "l1"):
        per, dp = ops.diffusion_loss(_dev(G, pred), _dev(G, target), _dev(G, w), lt)
        f = d * d if lt == "l2" else d.abs()
        blocks_d = min(max(1, -(-inner // 256)), 256)
        depth_d = -(-inner // (blocks_d * 256)) + 8 + blocks_d
        assert_elementwise(per, f.mean(1), out_dtype=F32, cond=f.mean(1) * 2, k=depth_d + 2, what=f"diffusion {lt} per-sample")
        wd = w.double()[:, None] / inner
        want = 2 * wd * d if lt == "l2" else wd * torch.sign(d)
        assert_elementwise(dp, want, out_dtype=BF16, cond=want.abs(), k=4, what=f"diffusion {lt} dpred")
    G.check()


@pytest.mark.parametrize("b,c", [(1, 1), (3, 2), (5, 63), (4, 64), (7, 65), (9, 1000)])
def test_softmax_xent_labels_at_both_ends(G, b, c):
    logits = (torch.rand((b, c), generator=_gen(c), dtype=torch.float64) * 160 - 80).float()  # spread over +-80
    labels = torch.tensor([(0 if i % 2 == 0 else c - 1) for i in range(b)])
    loss, dl = ops.softmax_xent(_dev(G, logits), G.index(labels.to(DEV)), 0.25)
    l64 = logits.double()
    lse = torch.logsumexp(l64, 1)
    want_loss = (lse - l64[torch.arange(b), labels]).sum()
    p = torch.softmax(l64, 1)
    want_d = (p - torch.nn.functional.one_hot(labels, c).double()) * 0.25
    # fast intrinsics: __expf of an argument up to 160 in magnitude (its rounding: |arg| * 2^-24 relative), __logf,
    # rcp; the loss is an f32 sum over the batch of lse terms of size <= 160
    assert_elementwise(loss, want_loss, out_dtype=F32, cond=(lse.abs() + 160).sum(), k=b + 64, what=f"xent loss {b}x{c}")
    assert_elementwise(dl, want_d, out_dtype=F32, ulps=4, cond=0.25 * p * (1 + 160) + 0.25 * 2 ** -20, k=c + 64,
                       what=f"xent dlogits {b}x{c}")
    G.check()


@pytest.mark.parametrize("m,d", [(1, 1), (3, 5), (5, 63), (4, 64), (7, 65), (2, 1000)])
def test_l2norm(G, m, d):
    x = _randn((m, d), m * d + 1)
    y, inv = ops.l2norm_fwd(_dev(G, x))
    x64 = x.double()
    nrm = x64.norm(dim=1, keepdim=True)
    # f32 sum of squares of depth <= d, a rsqrt / division, one multiply
    assert_elementwise(y, x64 / nrm, out_dtype=F32, ulps=4, cond=(x64 / nrm).abs(), k=d + 16, what=f"l2norm y {m}x{d}")
    dy = _randn((m, d), 7 * m + d)
    dx = ops.l2norm_bwd(_dev(G, dy), y, inv)
    y64 = x64 / nrm
    want = (dy.double() - y64 * (dy.double() * y64).sum(1, keepdim=True)) / nrm
    cond = (dy.double().abs() + y64.abs() * (dy.double() * y64).abs().sum(1, keepdim=True)) / nrm
    assert_elementwise(dx, want, out_dtype=F32, ulps=4, cond=cond, k=2 * d + 32, what=f"l2norm dx {m}x{d}")
    G.check()


@pytest.mark.parametrize("scale", ["alpha", "alpha_dev", "both"])
@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (15, 17, 16), (16, 16, 17), (33, 31, 50), (5, 70, 3)])
@pytest.mark.parametrize("a_trans,b_trans", [(False, False), (False, True), (True, False), (True, True)])
def test_sgemm_f32_layouts_tiles_and_scales(G, a_trans, b_trans, m, n, k, scale):
    """cfhip_sgemm_f32 (the CLIP similarity products): the four operand layouts, sizes at, below and across its 16 x 16 LDS tiles
    (partial tiles in M, N and K, one element, a reduction shorter than a tile), the host scale, the device scale and their product"""
    a = _randn((k, m) if a_trans else (m, k), 1000 * m + k)
    b = _randn((k, n) if b_trans else (n, k), 1000 * n + k + 1)
    alpha = float(torch.tensor(0.37, dtype=F32)) if scale != "alpha_dev" else 1.0
    adev = torch.tensor([-1.7], dtype=F32) if scale != "alpha" else None
    out = ops.sgemm_f32(_dev(G, a), _dev(G, b), a_trans=a_trans, b_trans=b_trans, alpha=alpha,
                        alpha_dev=None if adev is None else _dev(G, adev))
    A = a.double().t() if a_trans else a.double()
    B = b.double() if b_trans else b.double().t()
    s = alpha * (1.0 if adev is None else float(adev.double()))
    assert tuple(out.shape) == (m, n) and out.dtype == F32
    # an f32 FMA chain of depth K, then two products with the scale (alpha_dev * alpha, and that with the sum)
    assert_elementwise(out, s * (A @ B), out_dtype=F32, cond=abs(s) * (A.abs() @ B.abs()), k=k + 2,
                       what=f"sgemm_f32 {'t' if a_trans else 'n'}{'t' if b_trans else 'n'} {m}x{n}x{k} {scale}")
    G.check()


# ---------------------------------------------------------------------------------------------
# LayerNorm rows
# ---------------------------------------------------------------------------------------------


def _ln_ref(x64, g64, b64, eps):
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    return mu, rs, (x64 - mu) * rs * g64 + b64


@pytest.mark.parametrize("m,d,kind", [(1, 8, "bf16"), (3, 64, "bf16"), (5, 72, "f32"), (65, 256, "bf16"), (7, 768, "f32"),
                                      (4, 1000, "bf16"), (257, 520, "f32"), (3, 256, "offset_f32"), (5, 768, "offset_bf16")])
def test_layernorm_fwd_bwd_per_element(G, m, d, kind):
    eps = 1e-5
    if kind == "offset_f32":  # a large common offset against the spread: what f32 rows can carry
        x = 1e3 + _randn((m, d), d + m, 1e-2)
    elif kind == "offset_bf16":
        x = (100.0 + _randn((m, d), d + m, 4.0)).to(BF16)
    else:
        x = _randn((m, d), d + m, 2.0)
        x = x if kind == "f32" else x.to(BF16)
    g, b = _randn(d, 1, 0.3) + 1, _randn(d, 2, 0.3)
    x64, g64, b64 = x.double(), g.double(), b.double()
    mu, rs, y64 = _ln_ref(x64, g64, b64, eps)
    xd = _dev(G, x)
    y, mean, rstd = ops.layernorm_fwd(xd, _dev(G, g), _dev(G, b), eps)
    depth = -(-d // 64) + 16  # one wave per row: a lane's chain over its d / 64 columns plus the wave tree
    cx = rs * (x64.abs() + mu.abs())  # bounds the error of xhat from an f32 mean of the row
    assert_elementwise(mean, mu.view(-1), out_dtype=F32, cond=x64.abs().mean(1), k=depth, what=f"ln mean {m}x{d} {kind}")
    # two-pass variance: first order in its f32 sums, second order in the error of the mean (k u |mean| rstd)^2
    rsm = (rs * mu.abs()).view(-1)
    assert_elementwise(rstd, rs.view(-1), out_dtype=F32, ulps=2, cond=rs.view(-1) * (1 + depth * 2.0 ** -24 * rsm * rsm), k=depth,
                       what=f"ln rstd {m}x{d} {kind}")
    assert_elementwise(y, y64, out_dtype=BF16, cond=cx * g64.abs() + b64.abs(), k=depth, what=f"ln y {m}x{d} {kind}")
    dy = _randn((m, d), 3 * d + m).to(BF16)
    dxa = _randn((m, d), 5 * d + m).to(BF16)
    dx, dg, db = ops.layernorm_bwd(_dev(G, dy), xd, _dev(G, g), mean, rstd, dx_add=_dev(G, dxa))
    xh = (x64 - mu) * rs
    dn = dy.double() * g64
    want_dx = rs * (dn - dn.mean(1, keepdim=True) - xh * (dn * xh).mean(1, keepdim=True)) + dxa.double()
    cond_dx = rs * (dn.abs() + dn.abs().mean(1, keepdim=True) + cx * (dn.abs() * cx).mean(1, keepdim=True)) + dxa.double().abs()
    assert_elementwise(dx, want_dx, out_dtype=BF16, cond=cond_dx, k=depth, what=f"ln dx {m}x{d} {kind}")
    cdy = dy.double().abs()
    assert_elementwise(dg, (dy.double() * xh).sum(0), out_dtype=F32, cond=(cdy * cx).sum(0), k=m + 16,
                       what=f"ln dgamma {m}x{d} {kind}")
    assert_elementwise(db, dy.double().sum(0), out_dtype=F32, cond=cdy.sum(0), k=m + 16, what=f"ln dbeta {m}x{d} {kind}")
    # accumulate into guarded caller-owned parameter gradients
    dga, dba = G.out2d(1, d, d, F32, DEV, fill=0.5), G.out2d(1, d, d, F32, DEV, fill=-0.5)
    ops.layernorm_bwd(_dev(G, dy), xd, _dev(G, g), mean, rstd, dgamma=dga.view(d), dbeta=dba.view(d), accumulate=True)
    assert_elementwise(dga.view(d), (dy.double() * xh).sum(0) + 0.5, out_dtype=F32, cond=(cdy * cx).sum(0) + 1, k=m + 17,
                       what="ln dgamma acc")
    assert_elementwise(dba.view(d), dy.double().sum(0) - 0.5, out_dtype=F32, cond=cdy.sum(0) + 1, k=m + 17, what="ln dbeta acc")
    G.check()


# ---------------------------------------------------------------------------------------------
# GroupNorm, every form
# ---------------------------------------------------------------------------------------------


def _gn_ref(x64, add64, g64, b64, groups, eps, silu, dy64):
    """float64 forward and backward of [SiLU](GN(x + add) * gamma + beta) by hand, plus per-element cond terms"""
    bsz, c = x64.shape[:2]
    xs = x64 + add64[:, :, None]
    xg = xs.reshape(bsz, groups, -1)
    mu = xg.mean(2, keepdim=True)
    rs = 1.0 / torch.sqrt(((xg - mu) ** 2).mean(2, keepdim=True) + eps)
    xh = ((xg - mu) * rs).reshape(xs.shape)
    ga = g64.view(-1, c, 1) if g64.dim() == 1 else g64[:, :, None]
    be = b64.view(-1, c, 1) if b64.dim() == 1 else b64[:, :, None]
    pre = xh * ga + be
    s = _sig64(pre)
    y = pre * s if silu else pre
    dn = dy64 * (s * (1 + pre * (1 - s))) if silu else dy64
    dg, db = (dn * xh).sum(2), dn.sum(2)
    dng = (dn * ga).reshape(bsz, groups, -1)
    xhg = xh.reshape(bsz, groups, -1)
    dx = (rs * (dng - dng.mean(2, keepdim=True) - xhg * (dng * xhg).mean(2, keepdim=True))).reshape(xs.shape)
    cx = (rs * (xg.abs() + mu.abs())).reshape(xs.shape)  # error of xhat from f32 group statistics
    # (the factor 2 on the cond terms below: xhat = (x - mean) * rstd takes k u cx from the mean's error and k u |xhat| <= k u cx
    # from rstd's relative error — two contributions of the same bound)
    # with SiLU the error of xhat reaches dn through silu'' (|silu''| <= 1/2) times gamma
    cdn = dy64.abs() * (1 + ga.abs() * cx) if silu else dy64.abs()
    cdng = dng.abs()
    cxg = cx.reshape(bsz, groups, -1)
    cond_dx = (rs * (cdng + cdng.mean(2, keepdim=True) + cxg * (cdng * cxg).mean(2, keepdim=True))).reshape(xs.shape)
    return dict(mean=mu.view(-1), rstd=rs.view(-1), y=y, dx=dx, dg=dg, db=db, dadd=dx.sum(2),
                cond_mean=xg.abs().mean(2).view(-1), cond_rstd_mean=(rs * xg.abs().mean(2, keepdim=True)).view(-1), cond_rstd=rs.view(-1), cond_y=(cx * ga.abs() + be.abs()) * 2,
                cond_dx=cond_dx * 2, cond_dg=(dy64.abs() * cx + cdn * xh.abs()).sum(2) * 2, cond_db=cdn.sum(2) * 2,
                cond_dadd=cond_dx.sum(2) * 2)


GN_CASES = [
    # b, c, groups, inner, dtype, form: "scalar" (inner % 8 != 0), "vector" (one workgroup), "split"
    (2, 6, 6, 15, "bf16", "scalar"),     # one channel per group, odd inner
    (3, 9, 3, 13, "f32", "scalar"),      # three channels per group
    (2, 8, 4, 64, "bf16", "vector"),
    (1, 10, 2, 72, "f32", "vector"),     # five channels per group
    (1, 4, 4, 8 * 97, "bf16", "split"),  # 97 vectors per channel: the last slice is short
    (2, 6, 2, 8 * 65, "f32", "split"),
    (1, 32, 32, 8 * 3, "bf16", "split"),  # one vector per slice
    (2, 8, 2, 8 * 130, "offset_f32", "split"),
    (1, 8, 4, 8 * 40, "offset_bf16", "vector"),
    (1, 136, 1, 8 * 3, "bf16", "split"),  # 136 channels per group > CFHIP_GN_MAX_CG: forward in 3 slices, backward falls to the scalar kernel
    (2, 4, 2, 16, "shifted_bf16", "vector"),  # x starts one element (2 bytes) into its storage: both ways through the scalar kernels
]


@pytest.mark.parametrize("b,c,groups,inner,kind,form", GN_CASES)
@pytest.mark.parametrize("silu,per_sample", [(False, False), (True, True)])
def test_groupnorm_nchw_forms(G, monkeypatch, b, c, groups, inner, kind, form, silu, per_sample):
    monkeypatch.setattr(ops, "GN_TARGET_WORKGROUPS", 1 << 20 if form == "split" else 0)
    monkeypatch.setattr(ops, "GN_MIN_SLICE", 8)
    splits = ops.gn_splits(b, c, groups, inner)
    assert (splits > 1) == (form == "split"), splits
    # a ramp along `inner`: every slice has a mean of its own, so that a slice left out of a merge moves the statistics
    ramp = torch.linspace(0, 4, inner, dtype=torch.float64)
    base = _randn((b, c, inner), b * c + inner, 1.0).double() + ramp
    if kind == "offset_f32":
        x = (1e3 + base * 1e-2).float()
    elif kind == "offset_bf16":
        x = (100.0 + base * 4).to(BF16)
    else:
        x = base.float() if kind == "f32" else base.to(BF16)
    add = _randn((b, c), 11, 0.5)
    gshape = (b, c) if per_sample else (c,)
    gamma, beta = _randn(gshape, 12, 0.3) + 1, _randn(gshape, 13, 0.3)
    dy = _randn((b, c, inner), 14).to(BF16)
    r = _gn_ref(x.double(), add.double(), gamma.double(), beta.double(), groups, 1e-6, silu, dy.double())
    if kind == "shifted_bf16":  # a contiguous view that is only 2-byte aligned (the element in front of it is NaN)
        xd = _dev(G, torch.cat([torch.full((1,), float("nan"), dtype=BF16), x.flatten()]))[1:].view(x.shape)
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 2
    else:
        xd = _dev(G, x)
    y, mean, rstd = ops.groupnorm_fwd(xd, _dev(G, gamma), _dev(G, beta), groups, 1e-6, add=_dev(G, add), silu=silu)
    n = c // groups * inner
    depth = -(-n // 256) + 16 + 64  # a thread's chain over its share of the group + the workgroup tree + <= 64 slice merges
    tag = f"gn {form} {kind} b{b} c{c} g{groups} i{inner} silu={silu}"
    assert_elementwise(mean, r["mean"], out_dtype=F32, cond=r["cond_mean"], k=depth, what=f"{tag} mean")
    # two-pass variance (and Chan's merge of slice pairs): first order in the f32 sums, second order in the mean's error
    rsm = r["cond_rstd_mean"]
    assert_elementwise(rstd, r["rstd"], out_dtype=F32, ulps=2, cond=r["cond_rstd"] * (1 + depth * 2.0 ** -24 * rsm * rsm), k=depth,
                       what=f"{tag} rstd")
    assert_elementwise(y, r["y"], out_dtype=BF16, cond=r["cond_y"], k=depth, what=f"{tag} y")
    dx, dg, db, dadd = ops.groupnorm_bwd(_dev(G, dy), xd, _dev(G, gamma), _dev(G, beta), mean, rstd, groups, add=_dev(G, add),
                                         silu=silu, reduce=False)
    assert_elementwise(dx, r["dx"], out_dtype=BF16, cond=r["cond_dx"], k=depth, what=f"{tag} dx")
    assert_elementwise(dg, r["dg"], out_dtype=F32, cond=r["cond_dg"], k=depth, what=f"{tag} dgamma part")
    assert_elementwise(db, r["db"], out_dtype=F32, cond=r["cond_db"], k=depth, what=f"{tag} dbeta part")
    # dadd sums the f32 dx values (before their bf16 rounding)
    assert_elementwise(dadd, r["dadd"], out_dtype=F32, cond=r["cond_dadd"], k=depth, what=f"{tag} dadd")
    G.check()


GN_NHWC_CASES = [
    # b, hw, c, groups, form ("groups": one workgroup per (sample, group); "slices": row slices per sample)
    (2, 15, 8, 4, "groups"),
    (1, 65, 64, 32, "groups"),
    (3, 7, 24, 6, "groups"),    # four channels per group
    (1, 257, 8, 4, "slices"),   # rows not a multiple of the slice count
    (2, 33, 24, 8, "slices"),   # odd channels per group
    (1, 17, 16, 16, "slices"),  # one channel per group
]


@pytest.mark.parametrize("b,hw,c,groups,form", GN_NHWC_CASES)
@pytest.mark.parametrize("silu,per_sample", [(False, False), (True, True)])
def test_groupnorm_nhwc_forms(G, monkeypatch, b, hw, c, groups, form, silu, per_sample):
    monkeypatch.setattr(ops, "GN_NHWC_GROUP_MIN_WORKGROUPS", 1 if form == "groups" else 1 << 30)
    monkeypatch.setattr(ops, "GN_NHWC_MIN_ROWS", 4)
    cpg = c // groups
    if form == "groups" and cpg % 2:
        pytest.fail("the group form needs an even number of channels per group")
    assert (ops.gn_nhwc_splits(b, hw, c, groups) == 0) == (form == "groups")
    ramp = torch.linspace(0, 4, hw, dtype=torch.float64)[None, :, None]
    x = (_randn((b, hw, c), b * hw + c).double() + ramp).to(BF16)  # NHWC rows
    add = _randn((b, c), 21, 0.5)
    gshape = (b, c) if per_sample else (c,)
    gamma, beta = _randn(gshape, 22, 0.3) + 1, _randn(gshape, 23, 0.3)
    dy = _randn((b, hw, c), 24).to(BF16)
    nchw = lambda t: t.double().permute(0, 2, 1)  # noqa: E731
    r = _gn_ref(nchw(x), add.double(), gamma.double(), beta.double(), groups, 1e-6, silu, nchw(dy))
    back = lambda t: t.permute(0, 2, 1).reshape(b * hw, c)  # noqa: E731
    rows = _dev(G, x.reshape(b * hw, c))
    y, mean, rstd = ops.groupnorm_nhwc_fwd(rows, b, _dev(G, gamma), _dev(G, beta), groups, 1e-6, add=_dev(G, add), silu=silu)
    depth = -(-cpg * hw // 16) + 16 + 64  # (>= 16 lanes per group row set) + the workgroup tree + slice merges
    tag = f"gn nhwc {form} b{b} hw{hw} c{c} g{groups} silu={silu}"
    assert_elementwise(mean, r["mean"], out_dtype=F32, cond=r["cond_mean"], k=depth, what=f"{tag} mean")
    rsm = r["cond_rstd_mean"]
    assert_elementwise(rstd, r["rstd"], out_dtype=F32, ulps=2, cond=r["cond_rstd"] * (1 + depth * 2.0 ** -24 * rsm * rsm), k=depth,
                       what=f"{tag} rstd")
    assert_elementwise(y, back(r["y"]), out_dtype=BF16, cond=back(r["cond_y"]), k=depth, what=f"{tag} y")
    dx, dg, db, dadd = ops.groupnorm_nhwc_bwd(_dev(G, dy.reshape(b * hw, c)), rows, b, _dev(G, gamma), _dev(G, beta), mean, rstd,
                                              groups, add=_dev(G, add), silu=silu)
    assert_elementwise(dx, back(r["dx"]), out_dtype=BF16, cond=back(r["cond_dx"]), k=depth, what=f"{tag} dx")
    assert_elementwise(dg, r["dg"], out_dtype=F32, cond=r["cond_dg"], k=depth, what=f"{tag} dgamma part")
    assert_elementwise(db, r["db"], out_dtype=F32, cond=r["cond_db"], k=depth, what=f"{tag} dbeta part")
    assert_elementwise(dadd, r["dadd"], out_dtype=F32, cond=r["cond_dadd"], k=depth, what=f"{tag} dadd")
    G.check()


# ---------------------------------------------------------------------------------------------
# resampling and embeddings
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (3, 1), (3, 5), (4, 6)])
def test_resampling_exact(G, h, w):
    x = _randn((2, 3, h, w), h * w).to(BF16)
    up = ops.upsample2_fwd(_dev(G, x))
    assert torch.equal(up.cpu(), x.repeat_interleave(2, 2).repeat_interleave(2, 3))
    dy = _randn((2, 3, 2 * h, 2 * w), 2 * h * w).to(BF16)
    want = dy.double().reshape(2, 3, h, 2, w, 2).sum((3, 5))
    # the sum of 4 bf16 values in f32 (exact up to 2^-24 relative per add), one rounding
    assert_elementwise(ops.upsample2_bwd(_dev(G, dy)), want, out_dtype=BF16, cond=dy.double().abs().reshape(2, 3, h, 2, w, 2).sum((3, 5)),
                       k=3, what="upsample2 bwd")
    assert_elementwise(ops.avgpool2_fwd(_dev(G, dy)), want / 4, out_dtype=BF16,
                       cond=dy.double().abs().reshape(2, 3, h, 2, w, 2).sum((3, 5)) / 4, k=4, what="avgpool2 fwd")
    assert_elementwise(ops.avgpool2_bwd(_dev(G, x)), (x.double() / 4).repeat_interleave(2, 2).repeat_interleave(2, 3), out_dtype=BF16,
                       what="avgpool2 bwd")
    xr = _randn((2, h, w, 8), 3 * h * w).to(BF16)  # NHWC rows (C % 8 == 0)
    upn = ops.upsample2_nhwc(_dev(G, xr.reshape(2 * h * w, 8)), 2, h, w)
    assert torch.equal(upn.cpu(), xr.repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(-1, 8))
    dyr = _randn((2 * 2 * h * 2 * w, 8), 4 * h * w).to(BF16)
    dxr = ops.upsample2_nhwc(_dev(G, dyr), 2, h, w, backward=True)
    d4 = dyr.double().reshape(2, h, 2, w, 2, 8)
    assert_elementwise(dxr, d4.sum((2, 4)).reshape(-1, 8), out_dtype=BF16, cond=d4.abs().sum((2, 4)).reshape(-1, 8), k=3,
                       what="upsample2_nhwc bwd")
    G.check()


@pytest.mark.parametrize("h,w,pads", [(2, 2, (1, 1, 1, 1)), (3, 5, (2, 4, 2, 0)), (5, 3, (0, 2, 4, 1)), (1, 4, (3, 3, 0, 0))])
def test_reflect_pad_at_the_extent_limit(G, h, w, pads):
    x = _randn((2, 3, h, w), h + w)
    xb = x.to(BF16)
    want = torch.nn.functional.pad(x.double(), pads, mode="reflect")
    assert_elementwise(ops.reflect_pad2d_fwd(_dev(G, x), pads), want, out_dtype=BF16, what=f"reflect fwd f32 {h}x{w} {pads}")
    assert torch.equal(ops.reflect_pad2d_fwd(_dev(G, xb), pads).cpu(), torch.nn.functional.pad(xb.float(), pads, mode="reflect").to(BF16))
    dy = _randn(want.shape, 9).to(BF16)
    xr = x.double().requires_grad_(True)
    torch.nn.functional.pad(xr, pads, mode="reflect").backward(dy.double())
    # each input element gathers <= 4 output gradients: an f32 sum of depth 3, one rounding
    assert_elementwise(ops.reflect_pad2d_bwd(_dev(G, dy), pads), xr.grad, out_dtype=BF16, cond=4 * dy.double().abs().max(), k=3,
                       what=f"reflect bwd {h}x{w} {pads}")
    G.check()


@pytest.mark.parametrize("dim", [2, 3, 65, 320, 321])
def test_timestep_embedding(G, dim):
    t = torch.tensor([0, 1, 999, 500, 37])
    out = ops.timestep_embedding(G.index(t.to(DEV)), dim)
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    arg = t.double()[:, None] * freqs[None]
    want = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    if dim % 2:
        want = torch.cat([want, torch.zeros(len(t), 1, dtype=torch.float64)], 1)
    cond = torch.cat([arg, arg], 1)
    if dim % 2:
        cond = torch.cat([cond, torch.zeros(len(t), 1, dtype=torch.float64)], 1)
    # the f32 argument t * exp(-ln(P) k / half): the exponent (<= 9.21 in magnitude) carries ~3 roundings, so the argument is
    # off by up to ~32 units of 2^-24 of itself, and sin / cos move by as much
    assert_elementwise(out, want, out_dtype=F32, ulps=4, cond=cond, k=32, what=f"timestep embedding dim {dim}")
    G.check()


@pytest.mark.parametrize("v,d,n", [(1, 4, 3), (7, 8, 64), (50, 64, 257), (9, 4, 65)])
def test_embedding_fwd_bwd_duplicates_and_padding(G, v, d, n):
    table = _randn((v, d), v * d)
    idx = torch.randint(0, v, (n,), generator=_gen(n))
    idx[: min(n, 3)] = v - 1  # duplicates of the last row
    idx[-1] = 0
    out = ops.embedding_fwd(_dev(G, table), G.index(idx.to(DEV)))
    assert torch.equal(out.cpu(), table[idx])
    dy = _randn((n, d), 3 * n).to(BF16)
    for pad in (-1, 0, v - 1):
        dtable_dense = G.out2d(v, d, d, F32, DEV, fill=0.0)  # guard rows above and below: no row past V is touched
        ops.embedding_bwd(_dev(G, dy), G.index(idx.to(DEV)), dtable_dense, padding_idx=pad)
        want = torch.zeros(v, d, dtype=torch.float64).index_add_(0, idx, dy.double())
        cond = torch.zeros(v, d, dtype=torch.float64).index_add_(0, idx, dy.double().abs())
        if pad >= 0:
            want[pad] = 0
            cond[pad] = 0
        # atomic f32 adds in any order: depth <= the number of duplicates (n)
        assert_elementwise(dtable_dense, want, out_dtype=F32, cond=cond, k=n, what=f"embedding bwd v{v} d{d} n{n} pad {pad}")
    G.check()


# ---------------------------------------------------------------------------------------------
# MFMA output edges
# ---------------------------------------------------------------------------------------------


def _mk(shape, seed):
    return _randn(shape, seed).to(BF16)


@pytest.mark.parametrize("cfg", list(range(17)))
def test_gemm_out_view_every_config(G, cfg):
    """every tile configuration, M / N = tile +- 1 and N around multiples of 8, into an `out=` view with ldc > N whose
    padding columns and guard rows hold a sentinel: bf16 and f32 outputs, bias + residual and GELU epilogues"""
    ops.set_option("gemm_config", cfg)
    try:
        bm = (128, 128, 128, 128, 128, 128, 128, 256, 256, 256, 128, 256, 256, 256, 192, 192, 128)[cfg]
        bn = (128, 128, 128, 64, 128, 64, 64, 256, 128, 128, 256, 128, 256, 256, 128, 128, 256)[cfg]
        for (m, n, k) in ((bm + 1, bn - 8, 72), (bm - 8, bn + 8, 136), (8, 16, 40)):
            for layout in ("nt", "nn", "tn"):
                a_trans, b_trans = layout == "tn", layout in ("nn", "tn")
                if a_trans and m % 8:
                    continue
                a = _mk((k, m) if a_trans else (m, k), m + k)
                b = _mk((k, n) if b_trans else (n, k), n + k)
                want, cond = _gemm_ref(a, b, a_trans, b_trans)
                ad, bd = _dev(G, a), _dev(G, b)
                tag = f"cfg{cfg} {layout} {m}x{n}x{k}"
                out32 = G.out2d(m, n, n + 8, F32, DEV)
                ops.gemm(ad, bd, a_trans=a_trans, b_trans=b_trans, out=out32)
                # f32 sum of K products (exact in f32) with a chain of depth <= K, one rounding
                assert_elementwise(out32, want, out_dtype=F32, cond=cond, k=k, what=f"{tag} f32")
                out16 = G.out2d(m, n, n + 16, BF16, DEV)
                ops.gemm(ad, bd, a_trans=a_trans, b_trans=b_trans, out=out16)
                assert_elementwise(out16, want, out_dtype=BF16, cond=cond, k=k, what=f"{tag} bf16")
        # epilogues (nt, the forward layout): bias + residual, bias + GELU with its pre-activation
        m, n, k = bm + 1, bn + 8, 72
        a, w = _mk((m, k), 1), _mk((n, k), 2)
        bias, res = _randn(n, 3), _mk((m, n), 4)
        want, cond = _gemm_ref(a, w, False, False)
        want, cond = want + bias.double(), cond + bias.double().abs()
        ld = n + 8
        out = G.out2d(m, n, ld, BF16, DEV)
        resd = G.out2d(m, n, ld, BF16, DEV)
        resd.copy_(res.to(DEV))
        ops.gemm(_dev(G, a), _dev(G, w), bias=_dev(G, bias), epilogue=ops.EPI_RESIDUAL, aux_in=resd, out=out)
        assert_elementwise(out, want + res.double(), out_dtype=BF16, cond=cond + res.double().abs(), k=k + 2, what=f"cfg{cfg} residual")
        out = G.out2d(m, n, ld, BF16, DEV)
        pre = G.out2d(m, n, ld, BF16, DEV)
        ops.gemm(_dev(G, a), _dev(G, w), bias=_dev(G, bias), epilogue=ops.EPI_GELU, aux_out=pre, out=out)
        assert_elementwise(pre, want, out_dtype=BF16, cond=cond, k=k + 1, what=f"cfg{cfg} pre-activation")
        # the epilogue applies the GELU to the bf16-rounded pre-activation it stores (as the backward's dGELU sees it):
        # fast intrinsics + A&S erf, one rounding
        p64 = pre.cpu().double()
        assert_elementwise(out, _gelu64(p64), out_dtype=BF16, cond=p64.abs() * (1 + p64 * p64), k=8, what=f"cfg{cfg} gelu")
    finally:
        ops.set_option("gemm_config", -1)
    G.check()


@pytest.mark.parametrize("split", [1, 3, 7])
def test_gemm_split_k_accumulate_into_view(G, split):
    kd, n, k = 1000, 136, 72  # dW[n, k] = dY[kd, n]^T X[kd, k], bias gradient colsum(dY)
    dy, x = _mk((kd, n), 5), _mk((kd, k), 6)
    want, cond = _gemm_ref(dy, x, True, True)
    out = G.out2d(n, k, k + 8, F32, DEV, fill=2.0)
    bg = G.out2d(1, n, n, F32, DEV, fill=-1.0)
    ops.gemm(_dev(G, dy), _dev(G, x), a_trans=True, b_trans=True, out=out, accumulate=True, split_k=split,
             bias_grad=bg.view(n), bias_grad_accumulate=True)
    assert_elementwise(out, want + 2.0, out_dtype=F32, cond=cond + 2.0, k=kd + 1, what=f"split {split} dW acc")
    assert_elementwise(bg.view(n), dy.double().sum(0) - 1.0, out_dtype=F32, cond=dy.double().abs().sum(0) + 1.0, k=kd + 1,
                       what=f"split {split} db acc")
    G.check()


@pytest.mark.parametrize("variant", [0, 16, 32])
def test_gemm_grouped_with_sentinel_gaps(G, variant):
    """several dW problems whose C blocks share one buffer with sentinel rows between them: no problem writes into its
    neighbour's gradient"""
    specs = [(591, 264, 72), (40, 8, 8), (333, 257 // 8 * 8 + 8, 136), (96, 256, 264)]  # (K, M, N)
    ops.set_option("grouped_variant", variant)
    try:
        ld = max(n for _, _, n in specs) + 8
        offs, r = [], 2
        for (_, m, _) in specs:
            offs.append(r)
            r += m + 3  # three sentinel rows between blocks
        outs = G.region((r + 2, ld), F32, DEV, lambda w: [w[o:o + m, :n] for o, (_, m, n) in zip(offs, specs)])
        probs, wants = [], []
        for i, ((k, m, n), out) in enumerate(zip(specs, outs)):
            dy, x = _mk((k, m), 100 + i), _mk((k, n), 200 + i)
            acc = bool(i % 2)
            out.fill_(3.0)
            bg = G.out2d(1, m, m, F32, DEV, fill=5.0)
            probs.append((_dev(G, dy), _dev(G, x), out, acc, bg.view(m), acc))
            w, c = _gemm_ref(dy, x, True, True)
            wants.append((w + (3.0 if acc else 0.0), c + 3.0, dy.double().sum(0) + (5.0 if acc else 0.0), dy.double().abs().sum(0) + 5, k))
        ops.gemm_grouped_tn(probs)
        for i, (p, (w, c, bw, bc, k)) in enumerate(zip(probs, wants)):
            assert_elementwise(p[2], w, out_dtype=F32, cond=c, k=k + 1, what=f"variant {variant} problem {i} dW")
            assert_elementwise(p[4], bw, out_dtype=F32, cond=bc, k=k + 1, what=f"variant {variant} problem {i} db")
    finally:
        ops.set_option("grouped_variant", 0)
    G.check()


# ---------------------------------------------------------------------------------------------
# more row norms: refused widths, the split backward, the two-word gradient stream, 4-D LN, BatchNorm
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", [2, 6, 2052])
def test_layernorm_refuses_unsupported_widths(d):
    """D must be a multiple of 4 and at most 2048: refused by the C-side checks before any launch"""
    x = torch.randn(3, d, device=DEV).to(BF16)
    g, b = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.layernorm_fwd(x, g, b, 1e-5)
    mean, rstd = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.layernorm_bwd(x, x, g, mean, rstd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("m,d", [(1, 4), (5, 68), (65, 256), (257, 1000), (3, 2048)])
def test_layernorm_bwd_partials_reduce_and_two_words(G, m, d):
    eps = 1e-5
    x = _randn((m, d), m + d, 2.0).to(BF16)
    g, b = _randn(d, 3, 0.3) + 1, _randn(d, 4, 0.3)
    x64, g64 = x.double(), g.double()
    mu, rs, _ = _ln_ref(x64, g64, b.double(), eps)
    xd = _dev(G, x)
    _, mean, rstd = ops.layernorm_fwd(xd, _dev(G, g), _dev(G, b), eps)
    dy = _randn((m, d), 5 * m + d).to(BF16)
    dxa32 = _randn((m, d), 7 * m + d)  # an f32 residual gradient carried as two bf16 words
    hi = dxa32.to(BF16)
    lo = (dxa32 - hi.float()).to(BF16)
    xh = (x64 - mu) * rs
    dn = dy.double() * g64
    depth = -(-d // 64) + 16
    cx = rs * (x64.abs() + mu.abs())
    core = rs * (dn - dn.mean(1, keepdim=True) - xh * (dn * xh).mean(1, keepdim=True))
    cond_core = rs * (dn.abs() + dn.abs().mean(1, keepdim=True) + cx * (dn.abs() * cx).mean(1, keepdim=True))
    # the split form: the row kernel writes dx and per-workgroup partial sums, the reduce kernel sums them
    dx, ws, rows = ops.layernorm_bwd_partials(_dev(G, dy), xd, _dev(G, g), mean, rstd, dx_add=_dev(G, hi))
    assert_elementwise(dx, core + hi.double(), out_dtype=BF16, cond=cond_core + hi.double().abs(), k=depth, what=f"partials dx {m}x{d}")
    dga, dba = G.out2d(1, d, d, F32, DEV, fill=0.5), G.out2d(1, d, d, F32, DEV, fill=-0.5)
    ops.layernorm_bwd_reduce(ws, rows, d, dga.view(d), dba.view(d), True)
    cdy = dy.double().abs()
    assert_elementwise(dga.view(d), (dy.double() * xh).sum(0) + 0.5, out_dtype=F32, cond=(cdy * cx).sum(0) + 1, k=m + 17,
                       what=f"reduce dgamma {m}x{d}")
    assert_elementwise(dba.view(d), dy.double().sum(0) - 0.5, out_dtype=F32, cond=cdy.sum(0) + 1, k=m + 17, what=f"reduce dbeta {m}x{d}")
    # two words in, two words out: hi + lo carries the f32 value to ~16 bits (the second word's own rounding)
    lo_out = G.empty((m, d), dtype=BF16, device=DEV)
    dx2, _, _ = ops.layernorm_bwd(_dev(G, dy), xd, _dev(G, g), mean, rstd, dx_add=_dev(G, hi), dx_add_lo=_dev(G, lo),
                                  dx_lo_out=lo_out, want_param_grads=False)
    want = core + hi.double() + lo.double()
    joined = dx2.cpu().double() + lo_out.cpu().double()
    assert_elementwise(joined, want, out_dtype=BF16, ulps=2.0 ** -7, cond=cond_core + dxa32.double().abs(), k=depth,
                       what=f"bwd2 hi+lo {m}x{d}")
    G.check()


@pytest.mark.parametrize("b,c,h,w", [(1, 1, 1, 3), (2, 3, 5, 7), (3, 8, 16, 17), (1, 4, 65, 63)])
def test_layernorm4d_workspace_and_per_element(G, b, c, h, w):
    """the reference's 4-D LN (unbiased std, y = (x - mean) / (std + eps) * w[c] + b[c]); its workspace is sized by
    cfhip_layernorm4d_workspace and sits between guards"""
    eps = 1e-5
    x = (_randn((b, c, h, w), b * c + h * w, 2.0) + torch.linspace(0, 3, h * w).view(1, 1, h, w)).to(BF16)
    wt, bs = _randn(c, 5, 0.3) + 1, _randn(c, 6, 0.3)
    x64 = x.double().requires_grad_(True)
    wt64, bs64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    n = c * h * w
    mu = x64.reshape(b, -1).mean(1)
    sd = x64.reshape(b, -1).std(1)
    y64 = (x64 - mu.view(b, 1, 1, 1)) / (sd.view(b, 1, 1, 1) + eps) * wt64.view(1, c, 1, 1) + bs64.view(1, c, 1, 1)
    dy = _randn((b, c, h, w), 9).to(BF16)
    y64.backward(dy.double())
    xd = _dev(G, x)
    y, mean, std = ops.layernorm4d_fwd(xd, _dev(G, wt), _dev(G, bs), eps)
    depth = -(-n // 64) + 64  # a thread's chain over its share of the sample + the workgroup tree + the partial-sum merge
    rs = (1.0 / (sd + eps)).detach().view(b, 1, 1, 1)
    cx = rs * (x.double().abs() + mu.detach().abs().view(b, 1, 1, 1))
    assert_elementwise(mean, mu.detach(), out_dtype=F32, cond=x.double().abs().reshape(b, -1).mean(1), k=depth, what="ln4d mean")
    rsm = (rs.view(b) * mu.detach().abs())
    assert_elementwise(std, sd.detach(), out_dtype=F32, ulps=2, cond=sd.detach() * (1 + depth * 2.0 ** -24 * rsm * rsm), k=depth,
                       what="ln4d std")
    # (the factor 2: the mean's error and std's relative error each move xhat by up to k u cx)
    assert_elementwise(y, y64.detach(), out_dtype=BF16, cond=2 * cx * wt.double().abs().view(1, c, 1, 1) + bs.double().abs().view(1, c, 1, 1),
                       k=depth, what="ln4d y")
    dwt, dbs = G.out2d(1, c, c, F32, DEV, fill=1.0), G.out2d(1, c, c, F32, DEV, fill=-1.0)
    dx = ops.layernorm4d_bwd(_dev(G, dy), xd, _dev(G, wt), mean, std, eps, dweight=dwt.view(c), dbias=dbs.view(c), accumulate=True)
    dn = (dy.double() * wt.double().view(1, c, 1, 1)).reshape(b, -1)
    cxr = cx.reshape(b, -1)
    cond_dx = 2 * rs.view(b, 1) * (dn.abs() + dn.abs().mean(1, keepdim=True) + cxr * (dn.abs() * cxr).mean(1, keepdim=True))
    assert_elementwise(dx, x64.grad, out_dtype=BF16, cond=cond_dx.view(b, c, h, w), k=depth, what="ln4d dx")
    cdy = dy.double().abs()
    assert_elementwise(dwt.view(c), wt64.grad + 1.0, out_dtype=F32, cond=2 * (cdy * cx).sum((0, 2, 3)) + 1, k=depth + b * h * w,
                       what="ln4d dweight acc")
    assert_elementwise(dbs.view(c), bs64.grad - 1.0, out_dtype=F32, cond=cdy.sum((0, 2, 3)) + 1, k=depth + b * h * w, what="ln4d dbias acc")
    G.check()


@pytest.mark.parametrize("b,c,inner,xdt", [(1, 1, 3, F32), (3, 5, 7, BF16), (2, 64, 65, BF16), (5, 3, 257, F32)])
def test_batchnorm_train_and_eval(G, b, c, inner, xdt):
    eps, mom = 1e-5, 0.1
    x = (_randn((b, c, inner), b + c + inner, 2.0) + 3.0).to(xdt)
    gm, bt = _randn(c, 1, 0.3) + 1, _randn(c, 2, 0.3)
    rm0, rv0 = _randn(c, 3, 0.1), torch.rand(c, generator=_gen(4)) + 0.5
    rm, rv = G.poisoned(rm0.to(DEV)), G.poisoned(rv0.to(DEV))
    xd = _dev(G, x)
    y, mean, rstd = ops.batchnorm_fwd(xd, _dev(G, gm), _dev(G, bt), rm, rv, eps, mom, True)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    mu = x64.mean((0, 2))
    var = x64.var((0, 2), unbiased=False)
    rs = 1.0 / torch.sqrt(var + eps)
    y64 = (x64 - mu.view(1, c, 1)) * rs.view(1, c, 1) * g64.view(1, c, 1) + b64.view(1, c, 1)
    n = b * inner
    depth = -(-n // 64) + 64
    cx = (rs.view(1, c, 1) * (x.double().abs() + mu.abs().view(1, c, 1))).detach()
    assert_elementwise(mean, mu.detach(), out_dtype=F32, cond=x.double().abs().mean((0, 2)), k=depth, what="bn mean")
    rsm = (rs * mu.abs()).detach()
    assert_elementwise(rstd, rs.detach(), out_dtype=F32, ulps=2, cond=rs.detach() * (1 + depth * 2.0 ** -24 * rsm * rsm), k=depth,
                       what="bn rstd")
    # (factor 2: the mean's and rstd's errors each move xhat by up to k u cx)
    assert_elementwise(y, y64.detach(), out_dtype=BF16, cond=2 * cx * gm.double().abs().view(1, c, 1) + bt.double().abs().view(1, c, 1),
                       k=depth, what="bn y train")
    # running statistics: (1 - momentum) * running + momentum * batch statistic (unbiased variance)
    want_rm = (1 - mom) * rm0.double() + mom * mu.detach()
    want_rv = (1 - mom) * rv0.double() + mom * x64.detach().var((0, 2), unbiased=True)
    assert_elementwise(rm, want_rm, out_dtype=F32, ulps=2, cond=rm0.double().abs() + x.double().abs().mean((0, 2)), k=depth + 4,
                       what="bn running mean")
    assert_elementwise(rv, want_rv, out_dtype=F32, ulps=2, cond=rv0.double().abs() + want_rv * (1 + depth * 2.0 ** -24 * rsm * rsm),
                       k=depth + 4, what="bn running var")
    dy = _randn((b, c, inner), 8).to(BF16)
    y64.backward(dy.double())
    dx, dg, db = ops.batchnorm_bwd(_dev(G, dy), xd, _dev(G, gm), mean, rstd, training=True)
    dn = (dy.double() * gm.double().view(1, c, 1)).transpose(0, 1).reshape(c, -1)
    cxc = cx.transpose(0, 1).reshape(c, -1)
    cond_dx = 2 * rs.detach().view(c, 1) * (dn.abs() + dn.abs().mean(1, keepdim=True) + cxc * (dn.abs() * cxc).mean(1, keepdim=True))
    assert_elementwise(dx, x64.grad, out_dtype=BF16, cond=cond_dx.view(c, b, inner).transpose(0, 1), k=depth, what="bn dx train")
    cdy = dy.double().abs()
    assert_elementwise(dg, g64.grad, out_dtype=F32, cond=2 * (cdy * cx).sum((0, 2)), k=depth, what="bn dgamma")
    assert_elementwise(db, b64.grad, out_dtype=F32, cond=cdy.sum((0, 2)), k=depth, what="bn dbeta")
    # eval: the running statistics normalise, backward is the per-channel affine map
    rme, rve = G.poisoned(rm0.to(DEV)), G.poisoned(rv0.to(DEV))
    ye, me, rse = ops.batchnorm_fwd(xd, _dev(G, gm), _dev(G, bt), rme, rve, eps, mom, False)
    rs_e = 1.0 / torch.sqrt(rv0.double() + eps)
    want_e = (x.double() - rm0.double().view(1, c, 1)) * (rs_e * gm.double()).view(1, c, 1) + bt.double().view(1, c, 1)
    cond_e = (x.double().abs() + rm0.double().abs().view(1, c, 1)) * (rs_e * gm.double().abs()).view(1, c, 1) + bt.double().abs().view(1, c, 1)
    assert_elementwise(ye, want_e, out_dtype=BF16, cond=cond_e, k=6, what="bn y eval")
    assert torch.equal(rme.cpu(), rm0) and torch.equal(rve.cpu(), rv0)  # eval leaves the running statistics alone
    dxe, dge, dbe = ops.batchnorm_bwd(_dev(G, dy), xd, _dev(G, gm), me, rse, training=False)
    assert_elementwise(dxe, dy.double() * (rs_e * gm.double()).view(1, c, 1), out_dtype=BF16,
                       cond=dy.double().abs() * (rs_e * gm.double().abs()).view(1, c, 1), k=4, what="bn dx eval")
    xh_e = (x.double() - rm0.double().view(1, c, 1)) * rs_e.view(1, c, 1)
    assert_elementwise(dge, (dy.double() * xh_e).sum((0, 2)), out_dtype=F32,
                       cond=(cdy * (x.double().abs() + rm0.double().abs().view(1, c, 1)) * rs_e.view(1, c, 1)).sum((0, 2)), k=depth + 4,
                       what="bn dgamma eval")
    assert_elementwise(dbe, dy.double().sum((0, 2)), out_dtype=F32, cond=cdy.sum((0, 2)), k=depth, what="bn dbeta eval")
    G.check()


# ---------------------------------------------------------------------------------------------
# focal loss, GEGLU, global average pooling, the grouped time projection, the tabular encoder
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("b,c", [(1, 1), (3, 2), (5, 63), (4, 64), (7, 65), (9, 1000)])
def test_softmax_focal_labels_at_both_ends(G, b, c):
    gamma, eps, gs = 2.0, 1e-6, 0.5
    logits = (torch.rand((b, c), generator=_gen(c + 1), dtype=torch.float64) * 40 - 20).float()
    labels = torch.tensor([(0 if i % 2 == 0 else c - 1) for i in range(b)])
    loss, dl = ops.softmax_focal(_dev(G, logits), G.index(labels.to(DEV)), gs, gamma=gamma, eps=eps)
    z = logits.double()
    s = torch.softmax(z, 1)
    sy = s[torch.arange(b), labels]
    p = sy + eps
    om = 1 - p
    want_loss = (-torch.log(p) * om ** gamma).sum()
    dldp = -om ** gamma / p + gamma * om ** (gamma - 1) * torch.log(p)
    want_d = gs * (dldp * sy)[:, None] * (torch.nn.functional.one_hot(labels, c).double() - s)
    # libm expf / logf / powf (a few ulps each) of arguments up to 40: relative errors ~ (1 + |z|) 2^-24 in every
    # softmax term, amplified by |d log p / d p| = 1 / p in the loss; an f32 sum over the batch
    amp = (1 + 40.0) * (1 + 1 / p)
    # 1 - p is formed from the f32 p = s_y + eps: it carries u (1 + p) absolutely (all of it when s_y -> 1, e.g. C = 1)
    dom = (1 + p)
    cond_l = (torch.log(p).abs() * om.abs() ** gamma * amp + torch.log(p).abs() * gamma * om.abs() ** (gamma - 1) * dom).sum()
    assert_elementwise(loss, want_loss, out_dtype=F32, cond=cond_l, k=b + 64,
                       what=f"focal loss {b}x{c}")
    ddom = gamma * om.abs() ** (gamma - 1) / p + gamma * (gamma - 1) * om.abs() ** (gamma - 2) * torch.log(p).abs()
    cond_d = gs * ((dldp.abs() + gamma * om.abs() ** (gamma - 1) + 1 / p) * sy * amp + ddom * dom * sy)[:, None] * (1 + s)
    assert_elementwise(dl, want_d, out_dtype=F32, ulps=4, cond=cond_d, k=c + 64, what=f"focal dlogits {b}x{c}")
    G.check()


@pytest.mark.parametrize("m,l", [(1, 4), (3, 8), (5, 12), (65, 64), (257, 36)])
def test_geglu(G, m, l):
    vg = _randn((m, 2 * l), m + l, 2.0).clamp(-6, 6).to(BF16)
    v, g = vg.double()[:, :l], vg.double()[:, l:]
    out = ops.geglu_fwd(_dev(G, vg))
    # one rounding of v * gelu(g): fast intrinsics + A&S erf as in test_bf16_elementwise
    cg = g.abs() * (1 + g * g)
    assert_elementwise(out, v * _gelu64(g), out_dtype=BF16, cond=v.abs() * cg, k=8, what=f"geglu fwd {m}x{l}")
    dy = _randn((m, l), 3 * m + l).to(BF16)
    dvg = ops.geglu_bwd(_dev(G, dy), _dev(G, vg))
    d = dy.double()
    want = torch.cat([d * _gelu64(g), d * v * _gelu_grad64(g)], 1)
    cond = torch.cat([d.abs() * cg, (d * v).abs() * cg * (1 + g.abs())], 1)
    assert_elementwise(dvg, want, out_dtype=BF16, cond=cond, k=8, what=f"geglu bwd {m}x{l}")
    G.check()


@pytest.mark.parametrize("b,c,h,w", [(1, 1, 1, 1), (2, 3, 1, 5), (3, 5, 7, 9), (2, 64, 16, 17)])
def test_global_avgpool(G, b, c, h, w):
    x = _randn((b, c, h, w), b * c * h + w).to(BF16)
    y = ops.avgpool_fwd(_dev(G, x))
    # an f32 sum over H W (chain depth <= H W), one division, one rounding
    assert_elementwise(y, x.double().mean((2, 3)), out_dtype=BF16, cond=x.double().abs().mean((2, 3)), k=h * w + 2, what="avgpool fwd")
    dy = _randn((b, c), 7).to(BF16)
    dx = ops.avgpool_bwd(_dev(G, dy), (b, c, h, w))
    assert_elementwise(dx, (dy.double() / (h * w)).view(b, c, 1, 1).expand(b, c, h, w), out_dtype=BF16, what="avgpool bwd")
    G.check()


@pytest.mark.parametrize("b,k,ns", [(1, 32, (64,)), (3, 2048, (64, 136)), (9, 96, (8, 65, 200)), (17, 2048, (320,))])
def test_time_projection_at_the_k_limit(G, b, k, ns):
    """cfhip_time_proj_fwd / _bwd up to K = 2048 (eight bf16 rows of it fill the 32 KB of staged LDS), N not a multiple of 64,
    batches around the chunk of 8; outputs and the partial-sum workspace between guards"""
    emb = _randn((b, k), b + k)
    ws = [(_randn((n, k), n, 0.05)).to(BF16) for n in ns]
    bs = [_randn(n, n + 1, 0.1) for n in ns]
    t16 = G.empty((b, k), dtype=BF16, device=DEV)
    outs = ops.time_proj_fwd(_dev(G, emb), [_dev(G, w) for w in ws], [_dev(G, x) for x in bs], t16)
    e64 = emb.double()
    sil = e64 * _sig64(e64)
    # t16 = bf16(SiLU(emb)), SiLU by fast intrinsics
    assert_elementwise(t16, sil, out_dtype=BF16, cond=sil.abs() * (1 + e64.abs()), k=8, what="time_proj t16")
    t = t16.cpu().double()
    for i, (o, w, x) in enumerate(zip(outs, ws, bs)):
        want = t @ w.double().t() + x.double()
        cond = t.abs() @ w.double().abs().t() + x.double().abs()
        # an f32 sum of K exact products (chain depth <= K) and the bias
        assert_elementwise(o, want, out_dtype=F32, cond=cond, k=k + 1, what=f"time_proj out {i} (N = {ns[i]})")
    dys = [_randn((b, n), 2 * n) for n in ns]
    d_emb = ops.time_proj_bwd(_dev(G, emb), [_dev(G, w) for w in ws], [_dev(G, d) for d in dys], [None] * len(ns))
    s = _sig64(e64)
    g = sum(d.to(BF16).double() @ w.double() for d, w in zip(dys, ws))
    gc = sum(d.to(BF16).double().abs() @ w.double().abs() for d, w in zip(dys, ws))
    sg = s * (1 + e64 * (1 - s))
    # SiLU' by fast intrinsics times an f32 sum over every N_i (depth <= sum N + the per-64-column partials)
    assert_elementwise(d_emb, sg * g, out_dtype=F32, ulps=2, cond=gc * sg.abs() * (1 + e64.abs()), k=sum(ns) + 64, what="time_proj d_emb")
    G.check()


def test_ml_encoder_under_guards(G, golden):
    """the tabular encoder's gather / one-hot / scatter kernels (cfhip_ml_encode_*) with guarded outputs and a poisoned input,
    bit for bit against the reference's results already frozen in tests/golden/ml_encoder.pt"""
    from cflearn_amd.modules import MLEncoder

    for case in ("mixed", "all_embedding_oob"):
        g = golden("ml_encoder.pt")[case]
        enc = MLEncoder(g["settings"])
        enc.load_state_dict(g["sd"])
        enc = enc.to(DEV).eval()
        x = G.poisoned(g["x"].to(DEV))
        assert torch.equal(enc(x).cpu(), g["merged_all"])
        indices, _, embedding = enc.encode_result(x)
        assert torch.equal(indices.cpu(), g["indices"]) and torch.equal(embedding.cpu(), g["embedding"])
    G.check()


# ---------------------------------------------------------------------------------------------
# implicit-GEMM 3x3 convolution and attention
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("b,cin,cout,h,w", [(1, 32, 24, 5, 7), (2, 64, 136, 13, 9), (1, 32, 120, 3, 2), (3, 32, 128, 11, 11)])
@pytest.mark.parametrize("split", [1, 3])
def test_conv3x3_fwd_and_wgrad_edges(G, b, cin, cout, h, w, split):
    """H W not a multiple of the tile rows, Cout at and around tile boundaries, split reductions: outputs and the
    cfhip_conv3x3_*_workspace-sized workspaces between guards, inputs poisoned"""
    x = _randn((b, cin, h, w), b + cin + h).to(BF16)
    wt = (_randn((cout, cin, 3, 3), cout + cin) / (3.0 * cin ** 0.5)).to(BF16)
    bias = _randn(cout, 5)
    x64, w64 = x.double(), wt.double()
    want = torch.nn.functional.conv2d(x64, w64, bias.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    cond = torch.nn.functional.conv2d(x64.abs(), w64.abs(), bias.double().abs(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    x_rows = _dev(G, x.permute(0, 2, 3, 1).reshape(b * h * w, cin).contiguous())
    wk = ops.conv3x3_pack_filters(_dev(G, wt), False)
    ops.set_option("conv_split", split)
    try:
        y = ops.conv3x3_nhwc(x_rows, wk, _dev(G, bias), b, h, w)
    finally:
        ops.set_option("conv_split", -1)
    # an f32 sum of 9 Cin exact products (chain depth <= 9 Cin) and the bias, one rounding
    assert_elementwise(y, want, out_dtype=BF16, cond=cond, k=9 * cin + 1, what=f"conv3x3 {b}x{cin}->{cout} {h}x{w} split {split}")
    if ops.conv3x3_wgrad_ok(b, h, w):
        dy = _randn((b, cout, h, w), 11).to(BF16)
        dy_rows = _dev(G, dy.permute(0, 2, 3, 1).reshape(b * h * w, cout).contiguous())
        dw = G.out2d(1, cout * cin * 9, cout * cin * 9, F32, DEV, fill=0.25).view(cout, cin, 3, 3)
        db = G.out2d(1, cout, cout, F32, DEV, fill=-0.25).view(cout)
        ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split_k=split, out=dw, accumulate=True, bias_grad=db, bias_grad_accumulate=True)
        want_w = torch.nn.grad.conv2d_weight(x64, (cout, cin, 3, 3), dy.double(), padding=1)
        cond_w = torch.nn.grad.conv2d_weight(x64.abs(), (cout, cin, 3, 3), dy.double().abs(), padding=1)
        # an f32 sum of B H W exact products per filter tap (chain depth <= B H W)
        assert_elementwise(dw, want_w + 0.25, out_dtype=F32, cond=cond_w + 0.25, k=b * h * w + 1, what="conv3x3 wgrad dW acc")
        assert_elementwise(db, dy.double().sum((0, 2, 3)) - 0.25, out_dtype=F32, cond=dy.double().abs().sum((0, 2, 3)) + 0.25,
                           k=b * h * w + 1, what="conv3x3 wgrad db acc")
    G.check()


@pytest.mark.parametrize("t", [1, 63, 65, 129, 197])
@pytest.mark.parametrize("dh", [40, 64, 80])
@pytest.mark.parametrize("mode", ["plain", "causal", "mask"])
def test_attention_fwd_bwd_edges(G, t, dh, mode):
    """O, lse, dQ, dK, dV per element at token counts around the tiles and head widths of both kernel families; every
    partial tile's masked slots read NaN-surrounded operands"""
    bsz, heads = 2, 2
    d = heads * dh
    q, k, v = (_randn((bsz, t, d), 100 * i + t + dh).to(BF16) for i in range(3))
    causal = mode == "causal"
    mask = None
    if mode == "mask":
        mask = torch.rand((t, t), generator=_gen(t)) > 0.3
        mask[:, 0] = True  # every row keeps one slot
    Q, K, V, p, lse = attn_ref(q, k, v, heads, dh, mask, causal)
    qd, kd, vd = _dev(G, q), _dev(G, k), _dev(G, v)
    md = None if mask is None else G.index(mask.to(torch.uint8).to(DEV))
    o, lse_d = ops.attn_fwd(qd, kd, vd, heads, mask=md, causal=causal, head_dim=dh)
    back = lambda z: z.transpose(1, 2).reshape(bsz, -1, d)  # noqa: E731
    tag = f"attn T={t} dh={dh} {mode}"
    # P is rounded to bf16 before the PV product (half an ulp: 2^-8 relative per p, k = 2^16 on cond = sum p |v|), scores
    # are f32 sums of dh exact products, exp2 by the intrinsic
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) / math.sqrt(dh)
    kp = 2 ** 16 + 2 * dh + 64
    assert_elementwise(o, back(p @ V), out_dtype=BF16, cond=back(p @ V.abs()), k=kp, what=f"{tag} O")
    # lse = max + log(sum exp): its error is that of the scores (cond = the absolute-value scores) and the log.  Where
    # head_dim = 8 mod 16 without mask / causal the row sum comes out of the PV MFMA's spare ones-column (attn.hip SUMCOL):
    # a sum of the bf16-rounded p, 2^-8 relative, i.e. 2^-8 absolute on lse (cond 1, k 2^16)
    sumcol = dh % 16 == 8 and mode == "plain"
    lse_cond = (p * sabs).sum(-1) + lse.abs() + 1
    lse_k = 2 * dh + 64
    if sumcol:
        lse_k += 2 ** 16  # (lse_cond >= 1)
    assert_elementwise(lse_d, lse, out_dtype=F32, ulps=4, cond=lse_cond, k=lse_k, what=f"{tag} lse")
    do = _randn((bsz, t, d), 7 * t + dh).to(BF16)
    dO = do.double().view(bsz, t, heads, dh).transpose(1, 2)
    dq, dk, dv = (G.empty((bsz, t, d), dtype=BF16, device=DEV) for _ in range(3))
    ops.attn_bwd(qd, kd, vd, o, _dev(G, do), lse_d, heads, dq=dq, dk=dk, dv=dv, mask=md, causal=causal, head_dim=dh)
    O = p @ V
    dP = dO @ V.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    scale = 1.0 / math.sqrt(dh)
    # dV = P^T dO and dS = P (dP - delta) are rounded to bf16 before their products (2^-8 relative), delta is taken from
    # the bf16 O; cond = the same products on absolute values
    cdS = p * ((dO.abs() @ V.abs().transpose(-1, -2)) + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    assert_elementwise(dv, back(p.transpose(-1, -2) @ dO), out_dtype=BF16, cond=back(p.transpose(-1, -2) @ dO.abs()), k=kp,
                       what=f"{tag} dV")
    assert_elementwise(dq, back(dS @ K * scale), out_dtype=BF16, cond=back(cdS @ K.abs() * scale), k=2 * kp, what=f"{tag} dQ")
    assert_elementwise(dk, back(dS.transpose(-1, -2) @ Q * scale), out_dtype=BF16, cond=back(cdS.transpose(-1, -2) @ Q.abs() * scale),
                       k=2 * kp, what=f"{tag} dK")
    G.check()
