"""GroupNorm on NHWC rows: every kernel instantiation cfhip_groupnorm_nhwc_fwd / _bwd can select, per element against float64.

The table (tests/gn_nhwc_cases.py) names for each case the instantiation it is meant to hit, forward and backward; the test
asserts `ops.gn_nhwc_plan` — the function the launchers themselves consult — says exactly that BEFORE anything is launched, so
a case that drifts onto another kernel fails instead of silently re-testing a covered one.  Outputs are allocated under
`guarded_ops` (NaN interiors between byte guards), inputs are `poisoned`, every output (mean, rstd, y, dx, dgamma_part,
dbeta_part, dadd) is compared per element with `_gn_ref` on the same bf16-rounded inputs.

Error model: `gn_nhwc_cases.chains` derives k per case from the planned path's geometry (not fitted).

Every row matters: x and dy are noise + a ramp along the rows + a step on the rows of the last, partly filled row-lane pass,
with amplitudes sized from k so that, in the float64 reference alone, leaving any of those rows out of the sums moves mean,
rstd, dgamma and dbeta by at least 8x the bound they are compared with (`_assert_rows_matter`, on the CPU, every case)."""
import functools

import pytest
import torch

from gn_nhwc_cases import ALIGN_CASES, ALL_BWD, ALL_FWD, CASES, COVERED_BWD, COVERED_FWD, GROUP_CASES, SLICE_CASES, chains, geometry
from helpers import F32_EPS_HALF, _gn_ref, assert_elementwise, guarded_ops, ulp_out

pytestmark = pytest.mark.gpu

from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
SETTINGS = [(False, False), (True, True)]  # (silu, per_sample), as test_groupnorm_nhwc_forms


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _steer(monkeypatch, case):
    """the form and slice count through the knobs of ops.gn_nhwc_splits"""
    if case.splits == 0:
        monkeypatch.setattr(ops, "GN_NHWC_GROUP_MIN_WORKGROUPS", 1)
        monkeypatch.setattr(ops, "GN_NHWC_GROUP_MAX_ROWS", 1 << 30)
    else:
        monkeypatch.setattr(ops, "GN_NHWC_GROUP_MIN_WORKGROUPS", 1 << 30)
        monkeypatch.setattr(ops, "GN_NHWC_MIN_ROWS", 1)
        monkeypatch.setattr(ops, "GN_NHWC_TARGET_WORKGROUPS", case.splits * case.b)
    for backward in (False, True):
        assert ops.gn_nhwc_splits(case.b, case.inner, case.c, case.g, backward) == case.splits


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(x, dy) bf16 [B, inner, C], add, gamma / beta per sample [B, C] (row 0 = the shared affine): computed once per case.
    The step's amplitude follows the sensitivity a dropped row must reach: the bounds of mean / dbeta / dgamma grow like k u inner
    (k roundings over sums of `inner` terms per channel), so the step is 4 + 256 k u inner (x) and 4 + 1024 k u inner (dy)."""
    case = next(c for c in CASES if c.name == name)
    b, inner, c = case.b, case.inner, case.c
    _, _, first = geometry(case)
    kb = chains(case)[1]
    grow = kb * F32_EPS_HALF * inner
    seed = sum(map(ord, name))
    ramp = torch.linspace(0, 4, inner, dtype=torch.float64)[None, :, None]
    x = _randn((b, inner, c), seed) + ramp
    dy = _randn((b, inner, c), seed + 1)
    x[:, first:] += 4 + 256 * grow
    dy[:, first:] = dy[:, first:].abs() + 4 + 1024 * grow
    add = _randn((b, c), seed + 2, 0.5).float()
    gamma = (_randn((b, c), seed + 3, 0.3) + 1).clamp_min(0.4).float()  # (positive: the step rows stay on SiLU's rising side)
    beta = _randn((b, c), seed + 4, 0.3).float()
    return x.to(BF16), dy.to(BF16), add, gamma, beta


def _nchw(t):
    return t.double().permute(0, 2, 1)


def _bounds(case, r):
    """the bounds mean / rstd / dgamma / dbeta are compared with (as assert_elementwise forms them)"""
    kf, kb, _ = chains(case)
    u = F32_EPS_HALF
    rsm = r["cond_rstd_mean"]
    cond_rstd = r["cond_rstd"] * (1 + kf * u * rsm * rsm)
    return dict(mean=ulp_out(r["mean"].abs(), F32) + kf * u * r["cond_mean"],
                rstd=2 * ulp_out(r["rstd"].abs(), F32) + kf * u * cond_rstd,
                dg=ulp_out(r["dg"].abs(), F32) + kb * u * r["cond_dg"],
                db=ulp_out(r["db"].abs(), F32) + kb * u * r["cond_db"]), cond_rstd


def _assert_rows_matter(case, r, x64, add64, g64, b64, silu, dy64, bounds):
    """From the float64 reference alone: a kernel that left row j (any row of the last row-lane pass) out of its sums — dividing by the
    full count, as the kernels do — would miss mean, rstd, dgamma and dbeta by >= 8x the bound of the comparison."""
    _, _, first = geometry(case)
    bsz, c, inner = x64.shape
    g, cpg = case.g, c // case.g
    xs = (x64 + add64[:, :, None]).reshape(bsz, g, cpg, inner)
    n = cpg * inner
    mu = r["mean"].view(bsz, g, 1, 1)
    rows = xs[..., first:]  # [B, G, cpg, rows of the last pass]
    delta = rows.sum(2) / n  # [B, G, rows]: what the mean loses with row j
    d_mean = delta.abs()
    # the centred sum without row j around the mean without row j:  sum_all (x - m')^2 = Q + n (m - m')^2,  Q = n (1 / rstd^2 - eps)
    q_all = n * (1.0 / r["rstd"].view(bsz, g, 1) ** 2 - EPS) + n * delta ** 2
    q_drop = q_all - ((rows - (mu - delta[:, :, None, :])) ** 2).sum(2)
    d_rstd = (1.0 / torch.sqrt(q_drop / n + EPS) - r["rstd"].view(bsz, g, 1)).abs()
    bm, br = bounds["mean"].view(bsz, g, 1), bounds["rstd"].view(bsz, g, 1)
    assert (d_mean >= 8 * bm).all(), f"{case.name}: a dropped row moves mean by {(d_mean / bm).min():.2f}x its bound"
    assert (d_rstd >= 8 * br).all(), f"{case.name}: a dropped row moves rstd by {(d_rstd / br).min():.2f}x its bound"
    # dgamma / dbeta: the row's own term of every channel
    xh = ((xs - mu) * r["rstd"].view(bsz, g, 1, 1)).reshape(bsz, c, inner)[..., first:]
    ga = g64.view(-1, c, 1) if g64.dim() == 1 else g64[:, :, None]
    be = b64.view(-1, c, 1) if b64.dim() == 1 else b64[:, :, None]
    dn = dy64[..., first:]
    if silu:
        pre = xh * ga + be
        s = torch.sigmoid(pre)
        dn = dn * (s * (1 + pre * (1 - s)))
    t_dg, t_db = (dn * xh).abs(), dn.abs()
    assert (t_dg >= 8 * bounds["dg"][:, :, None]).all(), f"{case.name}: dgamma {(t_dg / bounds['dg'][:, :, None]).min():.2f}x"
    assert (t_db >= 8 * bounds["db"][:, :, None]).all(), f"{case.name}: dbeta {(t_db / bounds['db'][:, :, None]).min():.2f}x"


def _shifted(G, t, off):
    """a poisoned, contiguous device view of `t` that starts `off` elements into its storage (NaN in front of it)"""
    if not off:
        return G.poisoned(t.to(DEV))
    flat = torch.cat([torch.full((off,), float("nan"), dtype=t.dtype), t.flatten()])
    v = G.poisoned(flat.to(DEV))[off:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 2 * off
    return v


def reference(case, silu, per_sample):
    x, dy, add, gamma, beta = _inputs(case.name)
    ga, be = (gamma, beta) if per_sample else (gamma[0], beta[0])
    add64 = add.double() if case.add else torch.zeros_like(add, dtype=torch.float64)
    r = _gn_ref(_nchw(x), add64, ga.double(), be.double(), case.g, EPS, silu, _nchw(dy))
    return r, (x, dy, add if case.add else None, ga, be), add64


@pytest.mark.parametrize("silu,per_sample", SETTINGS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_groupnorm_nhwc_every_instantiation(G, monkeypatch, case, silu, per_sample):
    _steer(monkeypatch, case)
    b, inner, c, g = case.b, case.inner, case.c, case.g
    r, (x, dy, add, gamma, beta), add64 = reference(case, silu, per_sample)
    kf, kb, kd = chains(case)
    bounds, cond_rstd = _bounds(case, r)
    _assert_rows_matter(case, r, _nchw(x), add64, gamma.double(), beta.double(), silu, _nchw(dy), bounds)
    rows, dyr = _shifted(G, x.reshape(b * inner, c), case.off), _shifted(G, dy.reshape(b * inner, c), case.off)
    aligned = rows.data_ptr() % 16 == 0 and dyr.data_ptr() % 16 == 0  # (the outputs the wrappers allocate are 256-byte aligned)
    assert aligned == (case.off == 0)
    # the plan, before any launch
    assert ops.gn_nhwc_plan(False, c, g, inner, case.splits, aligned) == case.fwd, f"{case.name}: forward plan"
    assert ops.gn_nhwc_plan(True, c, g, inner, case.splits, aligned) == case.bwd, f"{case.name}: backward plan"
    dev = lambda t: None if t is None else G.poisoned(t.to(DEV))  # noqa: E731
    gd, bd, ad = dev(gamma), dev(beta), dev(add)
    back = lambda t: t.permute(0, 2, 1).reshape(b * inner, c)  # noqa: E731
    tag = f"gn nhwc {case.name} silu={silu}"
    y, mean, rstd = ops.groupnorm_nhwc_fwd(rows, b, gd, bd, g, EPS, add=ad, silu=silu)
    assert_elementwise(mean, r["mean"], out_dtype=F32, cond=r["cond_mean"], k=kf, what=f"{tag} mean")
    # two-pass variance (and Chan's merge of slice pairs): first order in the f32 sums, second order in the mean's error
    assert_elementwise(rstd, r["rstd"], out_dtype=F32, ulps=2, cond=cond_rstd, k=kf, what=f"{tag} rstd")
    assert_elementwise(y, back(r["y"]), out_dtype=BF16, cond=back(r["cond_y"]), k=kf, what=f"{tag} y")
    dx, dg, db, dadd = ops.groupnorm_nhwc_bwd(dyr, rows, b, gd, bd, mean, rstd, g, add=ad, silu=silu)
    assert_elementwise(dx, back(r["dx"]), out_dtype=BF16, cond=back(r["cond_dx"]), k=kb, what=f"{tag} dx")
    assert_elementwise(dg, r["dg"], out_dtype=F32, cond=r["cond_dg"], k=kb, what=f"{tag} dgamma part")
    assert_elementwise(db, r["db"], out_dtype=F32, cond=r["cond_db"], k=kb, what=f"{tag} dbeta part")
    if case.add:
        # dadd sums the f32 dx values (before their bf16 rounding)
        assert_elementwise(dadd, r["dadd"], out_dtype=F32, cond=r["cond_dadd"], k=kd, what=f"{tag} dadd")
    else:
        assert dadd is None
    G.check()


def test_every_instantiation_has_a_case():
    """12 forward + 9 backward group-form instantiations (VW 1 / 2 / 4 x the register tiers) and 2 + 2 slice-form ones (KC 1 / 2):
    the table's asserted plans cover the full set; the alignment cases run VW 1 where aligned rows would get 4."""
    assert len(ALL_FWD) == 12 + 2 and len(ALL_BWD) == 9 + 2
    assert ALL_FWD - COVERED_FWD == set() and COVERED_FWD <= ALL_FWD, sorted(ALL_FWD - COVERED_FWD)
    assert ALL_BWD - COVERED_BWD == set() and COVERED_BWD <= ALL_BWD, sorted(ALL_BWD - COVERED_BWD)
    assert {c.fwd for c in GROUP_CASES} == {p for p in ALL_FWD if p[0] == 0} and {c.bwd for c in GROUP_CASES} == {p for p in ALL_BWD if p[0] == 0}
    assert {c.fwd[3] for c in SLICE_CASES} == {1, 2}
    for case in ALIGN_CASES:
        assert case.off in (2, 4) and case.fwd[1] == 1
        assert ops.gn_nhwc_plan(False, case.c, case.g, case.inner, 0, True)[1] == 4
    # both sides of every tier boundary, for every vector width: rpt = rows per thread x VW at the limit and at the limit + VW
    rpt = {(c.fwd[1], geometry(c)[0] * c.fwd[1]) for c in GROUP_CASES}
    for vw in (1, 2, 4):
        for limit in (48, 88, 96, 176):
            assert (vw, limit) in rpt and (vw, limit + vw) in rpt, (vw, limit)
    for case in GROUP_CASES + ALIGN_CASES:  # the last row lane is partly empty
        assert case.inner % geometry(case)[1] != 0, case.name


@pytest.mark.parametrize("form,off", [("groups", 1), ("slices", 1), ("slices", 2), ("slices", 4)])
def test_rows_below_the_access_width_are_refused(G, monkeypatch, form, off):
    """The group form reads and writes dwords, the slice form 16 bytes at a time: row views that are only 2-byte (group form) or
    2- / 4- / 8-byte (slice form) aligned are refused by the C-side check before any launch — return code and message — and the
    outputs the wrapper had allocated keep their NaN fill."""
    b, inner, c, g = 1, 12, 16, 2
    monkeypatch.setattr(ops, "GN_NHWC_GROUP_MIN_WORKGROUPS", 1 if form == "groups" else 1 << 30)
    monkeypatch.setattr(ops, "GN_NHWC_MIN_ROWS", 4)
    assert (ops.gn_nhwc_splits(b, inner, c, g) == 0) == (form == "groups")
    x = _randn((b * inner, c), 5).to(BF16)
    rows, dy = _shifted(G, x, off), _shifted(G, x, off)
    ok = G.poisoned(x.to(DEV))
    gamma, beta = G.poisoned(torch.ones(c, device=DEV)), G.poisoned(torch.zeros(c, device=DEV))
    stats = G.poisoned(torch.ones(b * g, device=DEV))
    calls = [lambda: ops.groupnorm_nhwc_fwd(rows, b, gamma, beta, g, EPS),
             lambda: ops.groupnorm_nhwc_bwd(dy, ok, b, gamma, beta, stats, stats, g),
             lambda: ops.groupnorm_nhwc_bwd(ok, rows, b, gamma, beta, stats, stats, g)]
    for call in calls:
        n_before = len(G.allocs)
        with pytest.raises(RuntimeError, match=r"code -1\).*misaligned rows.*-byte aligned rows expected"):
            call()
        outs = [a.view for a in G.allocs[n_before:]]
        assert outs and all(torch.isnan(o).all() for o in outs if o.is_floating_point())
    torch.cuda.synchronize()
    G.check()
