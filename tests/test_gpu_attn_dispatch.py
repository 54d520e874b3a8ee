"""Every attention kernel the dispatcher of csrc/attn.hip can select (its own kernels and those of
csrc/attn_resident.hip and attn_one_pass.hip), per element against float64, inside guarded buffers.

Each case names the branch of plan_fwd / plan_bwd (the dispatcher's selection) it is meant to take in its pytest id
(docs/ATTN_DISPATCH.md lists, per compiled instantiation, the ids that launched it under a kernel trace).  Operands are
bf16 in NaN-surrounded buffers, masks in zero-guarded buffers, outputs start as NaN between byte guards; O, lse, dQ, dK
and dV are compared element by element with `helpers.attn_ref` and the guards are checked at the end.

Error model (an extension of test_gpu_kernel_edges.test_attention_fwd_bwd_edges; every term is named where it is used):
  * P (and dS) are rounded to bf16 before their MFMA products: half a bf16 ulp = 2^-9 relative per term, written as
    k = 2^16 units of 2^-24 on cond = the same product on absolute values (2^-8: the rounding of P plus that of the
    operand it was derived from, e.g. the bf16 O inside delta);
  * scores are f32 sums of dh exact products: 2 dh; exp2 / rcp / log by the 1-ulp intrinsics and their argument
    roundings: 64;
  * online softmax: a kernel rescales O and the row sum once per key block (64 keys in the two-tile kernels, 128 / 256
    in the general ones): one exp2 and one product rounding each on O and on l per block -> 4 ceil(Tk / 64);
  * the row sum itself is an f32 chain of about Tk / 4 additions per lane plus the cross-lane fold -> Tk / 4 + 8 on lse;
  * the ones-column row sum (plain head widths 40 and 56 on Fwd2<3 / 4>) adds the bf16-rounded p: 2^-8 on lse;
  * dropout: one more f32 product (P * 1 / (1 - p) before the bf16 rounding; 1 / (1 - p) / l in the forward): 2."""
import math
import os
import time

import pytest
import torch

from helpers import assert_attn_backward, assert_attn_forward, assert_elementwise, attn_mask as make_mask, attn_ref, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DEFAULTS = dict(attn_two_tiles=511, attn_one_pass=2, attn_persistent=7, attn_short_max=256, attn_pers_ctas=256)


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


@pytest.fixture
def options():
    """set(name=value, ...) for this test; the library's defaults come back afterwards, also on failure (the options are
    process-wide)"""
    def _set(**kw):
        for name, value in kw.items():
            assert name in DEFAULTS, name
            ops.set_option(name, value)
    try:
        yield _set
    finally:
        for name, value in DEFAULTS.items():
            ops.set_option(name, value)


@pytest.fixture(autouse=True)
def _census_window(request):
    """with CFHIP_ATTN_CENSUS_LOG set, append this test's CLOCK_MONOTONIC window (the time base of a rocprofv3 kernel
    trace): tools/attn_kernel_census.py joins the windows with the trace of the same run"""
    path = os.environ.get("CFHIP_ATTN_CENSUS_LOG")
    t0 = time.clock_gettime_ns(time.CLOCK_MONOTONIC)
    yield
    if path:
        torch.cuda.synchronize()
        with open(path, "a") as f:
            f.write(f"{request.node.name}\tmonotonic\t{t0}\t{time.clock_gettime_ns(time.CLOCK_MONOTONIC)}\n")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed):
    return torch.randn(shape, generator=_gen(seed), dtype=torch.float64).to(BF16)


# ---------------------------------------------------------------------------------------------
# one case: forward + backward against float64
# ---------------------------------------------------------------------------------------------


def run_attention(G, *, dh, tq, tk, mode="plain", mask_kind=None, heads=2, bsz=2, packed=False, parts=(3,), scale=None,
                  dropout=0.0, opt=None, tag=""):
    """forward, then the backward as the calls in `parts` ((3,), (1, 2) or (2,)); returns the device outputs"""
    opt = opt or {}
    d = heads * dh
    seed0 = 7 * dh + 3 * tq + tk
    if packed:
        assert tq == tk
        qkv = _randn((bsz, tq, 3, d), seed0)
        qkv_d = G.poisoned(qkv.to(DEV))
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        qd, kd, vd = qkv_d[:, :, 0], qkv_d[:, :, 1], qkv_d[:, :, 2]
    else:
        q, k, v = _randn((bsz, tq, d), seed0), _randn((bsz, tk, d), seed0 + 1), _randn((bsz, tk, d), seed0 + 2)
        qd, kd, vd = (G.poisoned(t.to(DEV)) for t in (q, k, v))
    causal = mode == "causal"
    mask = make_mask(mask_kind, bsz, heads, tq, tk) if mask_kind else None
    md = None if mask is None else G.index(mask.to(torch.uint8).to(DEV))
    sc = 1.0 / math.sqrt(dh) if scale is None else scale
    drop = None
    dkw = {}
    if dropout:
        dkw = dict(dropout_p=dropout, seed=1234 + dh, offset=40 + tq)
        m1 = ops.attn_dropout_mask(bsz, heads, tq, tk, dropout, dkw["seed"], dkw["offset"])
        m2 = ops.attn_dropout_mask(bsz, heads, tq, tk, dropout, dkw["seed"], dkw["offset"])
        assert torch.equal(m1, m2), f"{tag}: the dropout mask of one (seed, offset) differs between two calls"
        assert int(m1.max()) <= 1
        drop = (m1.cpu().bool(), ops.attn_dropout_p(dropout))
    ref = attn_ref(q, k, v, heads, dh, mask, causal, sc, drop)
    o = G.empty((bsz, tq, d), dtype=BF16, device=DEV)
    lse_d = G.empty((bsz, heads, tq), dtype=F32, device=DEV)
    ops.attn_fwd(qd, kd, vd, heads, mask=md, causal=causal, scale=sc, head_dim=dh, out=o, lse=lse_d, **dkw)
    # the forward's row sum comes out of the PV MFMA's ones column on the SUMCOL instantiations: ask the dispatcher's plan
    (fwd_kernel,) = ops.attn_plan(tq, tk, mask=md, causal=causal, head_dim=dh, dropout_p=dropout)
    sumcol = fwd_kernel.startswith("attn_fwd2_kernel<") and fwd_kernel.endswith(",true>")
    assert_attn_forward(o, lse_d, ref, sc, drop=bool(dropout), sumcol=sumcol, tag=tag)

    # backward
    do = _randn((bsz, tq, d), seed0 + 3)
    dod = G.poisoned(do.to(DEV))
    sentinel = 1.5
    if packed:
        dq, dk, dv = G.region((bsz, tq, 3, d), BF16, DEV, lambda w: [w[:, :, 0], w[:, :, 1], w[:, :, 2]])
        for t in (dq, dk, dv):
            t.fill_(float("nan"))
    else:
        dq = G.empty((bsz, tq, d), dtype=BF16, device=DEV)
        dk, dv = (G.empty((bsz, tk, d), dtype=BF16, device=DEV) for _ in range(2))
    if 1 not in parts and 3 not in parts:
        dq.fill_(sentinel)
    delta = G.empty((bsz, heads, tq), dtype=F32, device=DEV)  # starts as NaN
    for part in parts:
        ops.attn_bwd(qd, kd, vd, o, dod, lse_d, heads, dq=dq, dk=dk, dv=dv, mask=md, causal=causal, scale=sc, parts=part,
                     delta=delta, head_dim=dh, **dkw)
    has_dq = 1 in parts or 3 in parts
    assert_attn_backward(dq if has_dq else None, dk, dv, ref, do, sc, drop=drop, tag=tag)
    if not has_dq:
        assert bool((dq == sentinel).all()), f"{tag}: the dK / dV pass alone wrote dq"
    G.check()
    return dict(o=o, lse=lse_d, dq=dq, dk=dk, dv=dv)


# ---------------------------------------------------------------------------------------------
# the case table: (id, keyword arguments of run_attention, options)
# ---------------------------------------------------------------------------------------------

CASES = []


def case(cid, opt=None, **kw):
    CASES.append(pytest.param(kw, opt or {}, id=cid))


def _form(dh):
    """the general-path kernels a head width takes at the default options: forward, dQ, dK / dV (plain | masked)"""
    if dh <= 48:
        return ("Fwd2<3>" + ("+sumcol" if dh == 40 else ""), "dq3" + ("+fold" if dh == 40 else ""), "dkv2<3>" + ("+fold" if dh == 40 else "")), \
               ("Fwd2<3>m", "dq2<3>m", "dkv2<3>m")
    if dh <= 64:
        return ("Fwd2<4>" + ("+sumcol" if dh == 56 else ""), "dq2<4>", "dkv2<4>"), ("Fwd2<4>m", "dq2<4>m", "dkv2<4>m")
    if dh <= 80:
        return ("Fwd2<5>", "dq2<5>", "dkv2<5>"), ("gen_fwd<2>m", "gen_dq<2>m", "dkv2<5>m")
    if dh <= 96:
        return ("Fwd2<6>", "dq2<6>", "dkv2<6>"), ("gen_fwd<2>m", "gen_dq<2>m", "dkv2<6>m")
    nh = (dh + 63) // 64
    return (f"gen_fwd<{nh}>", f"gen_dq<{nh}>", f"gen_dkv<{nh}>"), (f"gen_fwd<{nh}>m", f"gen_dq<{nh}>m", f"gen_dkv<{nh}>m")


# all 24 head widths: plain / masked / causal at a ragged cross shape, and one shape across a chunk boundary
for _dh in range(8, 200, 8):
    _pl, _mk = _form(_dh)
    if _dh == 64:  # (37, 53) is the resident path here: its instantiations are listed below; the general forms at 257+
        _pl37, _mk37 = ("fwd<2,plain>", "dq", "dkv"), ("fwd<2,masked>", "dq_m", "dkv_m")
    else:
        _pl37, _mk37 = _pl, _mk
    case(f"dh{_dh}-37x53-plain-{'-'.join(_pl37)}", dh=_dh, tq=37, tk=53)
    case(f"dh{_dh}-37x53-mask-rand-{'-'.join(_mk37)}", dh=_dh, tq=37, tk=53, mask_kind="rand", mode="mask")
    case(f"dh{_dh}-37x53-causal-{'-'.join(_mk37)}", dh=_dh, tq=37, tk=53, mode="causal")
    _tk = 257 if _dh <= 64 else 129  # one key past the first staged chunk (256 keys for one 64-column half, else 128)
    case(f"dh{_dh}-70x{_tk}-plain-chunk-boundary-{'-'.join(_pl)}", dh=_dh, tq=70, tk=_tk, bsz=1)
    case(f"dh{_dh}-70x{_tk}-mask-full-chunk-boundary-{'-'.join(_mk)}", dh=_dh, tq=70, tk=_tk, bsz=1, mask_kind="full", mode="mask")

# head width 64, resident path, forward instantiations attn_fwd_kernel<NB, plain | masked> (Tq <= 128 keeps the plain
# forms off the persistent kernel) at Tk = 32 NB - 31, 32 NB - 1, 32 NB; the backward of these shapes is the two-pass pair
for _nb in range(1, 9):
    for _tk in (32 * _nb - 31, 32 * _nb - 1, 32 * _nb):
        case(f"dh64-fwd<{_nb},plain>-bwd_dq<plain>-bwd_dkv<plain>-33x{_tk}", dh=64, tq=33, tk=_tk, bsz=1)
    case(f"dh64-fwd<{_nb},masked>-bwd_dq<masked>-bwd_dkv<masked>-mask-rand-33x{32 * _nb - 1}", dh=64, tq=33, tk=32 * _nb - 1, bsz=1,
         mask_kind="rand", mode="mask")
    case(f"dh64-fwd<{_nb},masked>-causal-130x{32 * _nb - 1}", dh=64, tq=130, tk=32 * _nb - 1, bsz=1, mode="causal")
# persistent forward / dQ / dK-dV (Tq != Tk keeps the one-pass backward away): NB = ceil(Tk / 32), NBQ = ceil(Tq / 32)
for _nb, _tq, _tk in ((5, 160, 129), (6, 129, 191), (7, 255, 193), (8, 200, 256), (8, 256, 255), (5, 129, 160)):
    _nbq = -(-_tq // 32)
    case(f"dh64-fwd_pers<{_nb}>-dq_pers<{_nb}>-dkv_pers<{_nbq}>-{_tq}x{_tk}", dh=64, tq=_tq, tk=_tk)
case("dh64-fwd_pers<7>-dq_pers<7>-dkv_pers<6>-packed-unequal-heads-192x192-one_pass0", dict(attn_one_pass=0), dh=64, tq=192, tk=192,
     packed=True, heads=3)
case("dh64-fwd_pers<8>-dq_pers<8>-dkv_pers<8>-self-255", dh=64, tq=255, tk=255, packed=True)
case("dh64-fwd_pers<8>-dq_pers<8>-dkv_pers<8>-self-256", dh=64, tq=256, tk=256)
# one-pass backward: attn_bwd_one_kernel<2..4> (plain), <3..5, causal>, attn_bwd_one2_kernel<5..7>
for _nb, _t in ((2, 33), (2, 63), (2, 64), (3, 65), (3, 96), (4, 97), (4, 127), (4, 128)):
    case(f"dh64-bwd_one<{_nb}>-self-{_t}", dh=64, tq=_t, tk=_t, packed=_t in (33, 97))
for _nb, _t in ((3, 65), (3, 77), (4, 128), (5, 129), (5, 160)):
    case(f"dh64-bwd_one<{_nb},causal>-self-{_t}", dh=64, tq=_t, tk=_t, mode="causal", packed=_t == 77)
for _nb, _t in ((5, 129), (5, 145), (5, 160), (6, 161), (6, 177), (6, 192), (7, 193), (7, 197), (7, 224)):
    case(f"dh64-bwd_one2<{_nb}>-self-{_t}", dh=64, tq=_t, tk=_t, packed=_t == 197)
    if _t in (129, 177, 224):
        case(f"dh64-bwd_one<{_nb}>-self-{_t}-one_pass1", dict(attn_one_pass=1), dh=64, tq=_t, tk=_t)
# causal self-attention outside NB 3..5 and short plain sequences: the two-pass kernels
for _t in (1, 15, 16, 17, 31, 32):
    case(f"dh64-fwd<1,plain>-bwd_dq<plain>-bwd_dkv<plain>-self-{_t}", dh=64, tq=_t, tk=_t, packed=_t == 17)
for _t in (33, 64, 161, 255, 256):
    case(f"dh64-bwd_dq<masked>-bwd_dkv<masked>-causal-self-{_t}", dh=64, tq=_t, tk=_t, mode="causal")
# two-pass short kernels behind the one-pass backward and the persistent forms
for _t in (63, 127, 197):
    case(f"dh64-two-pass-bwd_dq<plain>-bwd_dkv<plain>-self-{_t}-one_pass0-persistent0", dict(attn_one_pass=0, attn_persistent=0),
         dh=64, tq=_t, tk=_t, packed=_t == 197)
case("dh64-fwd<8,plain>-bwd_dq<plain>-bwd_dkv<plain>-self-255-persistent0", dict(attn_persistent=0), dh=64, tq=255, tk=255)
# the short cross forms at the UNet's context length and around it
for _tq, _tk in ((128, 129), (100, 256), (16, 255)):
    case(f"dh64-fwd<{-(-_tk // 32)},plain>-short-cross-{_tq}x{_tk}", dh=64, tq=_tq, tk=_tk)
case("dh64-fwd<3,plain>-cross-256x77", dh=64, tq=256, tk=77)
# head width 64 beyond 256 tokens: the two-tile kernels with NDT = 4 (forward, dQ, dK / dV)
for _t in (257, 383, 385):
    case(f"dh64-Fwd2<4>-dq2<4>-dkv2<4>-self-{_t}", dh=64, tq=_t, tk=_t, bsz=1, packed=_t == 257)
    case(f"dh64-Fwd2<4>m-dq2<4>m-dkv2<4>m-causal-self-{_t}", dh=64, tq=_t, tk=_t, bsz=1, mode="causal")
case("dh64-Fwd2<4>-dq2<4>-dkv2<4>-cross-600x77", dh=64, tq=600, tk=77, bsz=1)
case("dh64-Fwd2<4>m-key-padding-600x77", dh=64, tq=600, tk=77, bsz=2, mask_kind="pad", mode="mask")
case("dh64-Fwd2<4>-dq2<4>-dkv2<4>-self-33-short_max32", dict(attn_short_max=32), dh=64, tq=33, tk=33)
case("dh64-Fwd2<4>m-dq2<4>m-dkv2<4>m-mask-rand-self-129-short_max0", dict(attn_short_max=0), dh=64, tq=129, tk=129, mask_kind="rand",
     mode="mask")
# token counts around tiles and chunks on the general families (40: three column tiles; 80 and 96: two halves; 160: three)
for _t in (1, 15, 16, 17, 31, 33, 127, 128, 129, 255, 256, 257, 383, 385):
    for _dh in (40, 96, 160):
        _pl, _mk = _form(_dh)
        case(f"dh{_dh}-self-{_t}-plain-{'-'.join(_pl)}", dh=_dh, tq=_t, tk=_t, bsz=1, packed=_t in (17, 129, 385))
    case(f"dh80-self-{_t}-causal-{'-'.join(_form(80)[1])}", dh=80, tq=_t, tk=_t, bsz=1, mode="causal")
    case(f"dh24-self-{_t}-causal-{'-'.join(_form(24)[1])}", dh=24, tq=_t, tk=_t, bsz=1, mode="causal", packed=_t in (33, 257))
for _dh in (40, 80, 160):
    case(f"dh{_dh}-cross-600x77-plain-{'-'.join(_form(_dh)[0])}", dh=_dh, tq=600, tk=77, bsz=1)
    case(f"dh{_dh}-cross-600x77-causal-{'-'.join(_form(_dh)[1])}", dh=_dh, tq=600, tk=77, bsz=1, mode="causal")
case("dh56-self-130-plain-Fwd2<4>+sumcol-dq2<4>-dkv2<4>-packed", dh=56, tq=130, tk=130, packed=True)
case("dh88-self-130-plain-Fwd2<6>-dq2<6>-dkv2<6>-packed", dh=88, tq=130, tk=130, packed=True)
case("dh72-self-130-plain-Fwd2<5>-dq2<5>-dkv2<5>-packed", dh=72, tq=130, tk=130, packed=True)
case("dh192-self-130-mask-gen<3>m-packed", dh=192, tq=130, tk=130, packed=True, mask_kind="rand", mode="mask")
case("dh128-self-130-plain-gen<2>-packed", dh=128, tq=130, tk=130, packed=True)
case("dh40-explicit-scale-0.3-70x129", dh=40, tq=70, tk=129, scale=0.3)
case("dh64-explicit-scale-0.05-70x129", dh=64, tq=70, tk=129, scale=0.05)
# masks: the three broadcast layouts, the wholly masked first chunks (m_use), the blanked last chunk
for _dh in (24, 64, 80, 160):
    _mk = "-".join(_form(_dh)[1])
    for _kind in ("rand", "pad", "full"):
        case(f"dh{_dh}-mask-{_kind}-100x140-{_mk if _dh != 64 else 'resident'}", dh=_dh, tq=100, tk=140, mask_kind=_kind, mode="mask")
    case(f"dh{_dh}-mask-prefix-m_use-70x385-{_mk}", dh=_dh, tq=70, tk=385, bsz=1, mask_kind="prefix", mode="mask")
    case(f"dh{_dh}-mask-band-70x385-{_mk}", dh=_dh, tq=70, tk=385, bsz=1, mask_kind="band", mode="mask")
    case(f"dh{_dh}-mask-band-causal-385x385-{_mk}", dh=_dh, tq=385, tk=385, bsz=1, mask_kind="band", mode="causal")
case("dh64-mask-band-resident-70x200", dh=64, tq=70, tk=200, mask_kind="band", mode="mask")
# a row with no kept key, on every masked family
for _dh, _tq, _tk in ((64, 70, 100), (64, 70, 300), (40, 70, 300), (80, 70, 300), (160, 70, 300)):
    _mk = "resident" if (_dh, _tk) == (64, 100) else "-".join(_form(_dh)[1])
    case(f"dh{_dh}-mask-dead-row-{_tq}x{_tk}-{_mk}", dh=_dh, tq=_tq, tk=_tk, mask_kind="dead", mode="mask")
# option-selected fallbacks (attn_two_tiles bits)
for _dh, _bit, _what in (
        (40, 1, "gen_fwd<1>"), (64, 1, "gen_fwd<1>"), (40, 2, "gen_dq<1>"), (64, 4, "gen_dq<1>"), (40, 8, "gen_dkv<1>"),
        (80, 8, "gen_dkv<2>"), (40, 16, "Fwd2<3>-no-sumcol"), (56, 16, "Fwd2<4>-no-sumcol"), (80, 32, "gen_dkv<2>"),
        (96, 32, "gen_dkv<2>"), (40, 64, "dq2<3>"), (24, 64, "dq2<3>"), (40, 128, "dq3-nofold-dkv2<3>-nofold"),
        (80, 256, "gen_fwd<2>-gen_dq<2>"), (96, 256, "gen_fwd<2>-gen_dq<2>")):
    for _tq, _tk in ((37, 53), (300, 300)):
        case(f"dh{_dh}-two_tiles-without-{_bit}-{_what}-{_tq}x{_tk}", dict(attn_two_tiles=511 & ~_bit), dh=_dh, tq=_tq, tk=_tk, bsz=1,
             packed=_tq == _tk)
    if _bit in (1, 2, 8, 32):
        case(f"dh{_dh}-two_tiles-without-{_bit}-{_what}-masked-prefix-70x385", dict(attn_two_tiles=511 & ~_bit), dh=_dh, tq=70, tk=385,
             bsz=1, mask_kind="prefix", mode="mask")


# persistent and one-pass kernels walking SEVERAL heads per workgroup (attn_pers_ctas 1 / 2: the next head's DMA into the
# other LDS buffer, LDS reuse), odd and even head counts per workgroup
for _ctas in (1, 2):
    for _b, _h in ((1, 3), (2, 2), (1, 5)):
        _o = dict(attn_pers_ctas=_ctas)
        _s = f"ctas{_ctas}-{_b * _h}heads"
        case(f"dh64-fwd_pers<5>-dq_pers<5>-dkv_pers<5>-160x129-{_s}", _o, dh=64, tq=160, tk=129, bsz=_b, heads=_h)
        case(f"dh64-fwd_pers<8>-dq_pers<8>-dkv_pers<8>-self-250-{_s}", _o, dh=64, tq=250, tk=250, bsz=_b, heads=_h)
        case(f"dh64-bwd_one2<7>-self-197-{_s}", _o, dh=64, tq=197, tk=197, bsz=_b, heads=_h, packed=True)
        case(f"dh64-bwd_one2<5>-self-130-{_s}", _o, dh=64, tq=130, tk=130, bsz=_b, heads=_h)
        case(f"dh64-bwd_one<2>-self-50-{_s}", _o, dh=64, tq=50, tk=50, bsz=_b, heads=_h)
        case(f"dh64-bwd_one<4>-self-100-{_s}", _o, dh=64, tq=100, tk=100, bsz=_b, heads=_h)
        case(f"dh64-bwd_one<3,causal>-self-77-{_s}", _o, dh=64, tq=77, tk=77, bsz=_b, heads=_h, mode="causal")
        case(f"dh64-bwd_one<6>-self-180-one_pass1-{_s}", dict(attn_pers_ctas=_ctas, attn_one_pass=1), dh=64, tq=180, tk=180, bsz=_b, heads=_h)
# a row with no kept key on the remaining masked backward kernels: gen<2> (head widths 104 .. 128) and the gen<1> fallbacks
case("dh128-mask-dead-row-70x300-gen_fwd<2>m-gen_dq<2>m-gen_dkv<2>m", dh=128, tq=70, tk=300, mask_kind="dead", mode="mask")
case("dh40-mask-dead-row-70x300-gen<1>m-two_tiles-500", dict(attn_two_tiles=511 & ~11), dh=40, tq=70, tk=300, mask_kind="dead", mode="mask")
case("dh64-mask-dead-row-70x300-gen<1>m-two_tiles-500", dict(attn_two_tiles=511 & ~11), dh=64, tq=70, tk=300, mask_kind="dead", mode="mask")
case("dh64-mask-dead-row-packed-130x130-resident", dh=64, tq=130, tk=130, mask_kind="dead", mode="mask", packed=True)


@pytest.mark.parametrize("kw,opt", CASES)
def test_dispatch(G, options, kw, opt, request):
    options(**opt)
    run_attention(G, opt=opt, tag=request.node.callspec.id, **kw)


# ---------------------------------------------------------------------------------------------
# parts: 3, 1 then 2, 2 alone (delta starts as NaN; dq must stay as it was)
# ---------------------------------------------------------------------------------------------

PARTS_SHAPES = [
    # id, kwargs, options: one per backward family
    ("dh64-two-pass-33x40", dict(dh=64, tq=33, tk=40), {}),
    ("dh64-two-pass-masked-130x130", dict(dh=64, tq=130, tk=130, mask_kind="rand", mode="mask"), {}),
    ("dh64-one2<5>|dq_pers<5>+bwd_dkv<plain>-160x160", dict(dh=64, tq=160, tk=160), {}),
    ("dh64-dq_pers<7>-197x197-packed", dict(dh=64, tq=197, tk=197, packed=True), {}),
    ("dh64-dq_pers<8>-129x256", dict(dh=64, tq=129, tk=256), {}),
    ("dh64-dq2<4>-delta-dkv2<4>-300x300", dict(dh=64, tq=300, tk=300, bsz=1), {}),
    ("dh40-dq3-fold-delta-dkv2<3>-fold-70x129", dict(dh=40, tq=70, tk=129), {}),
    ("dh24-dq3-delta-dkv2<3>-70x129", dict(dh=24, tq=70, tk=129), {}),
    ("dh48-dq2<3>m-delta-dkv2<3>m-causal-130x130", dict(dh=48, tq=130, tk=130, mode="causal"), {}),
    ("dh80-dq2<5>-delta-dkv2<5>-70x129", dict(dh=80, tq=70, tk=129), {}),
    ("dh96-dq2<6>-delta-dkv2<6>-130x130-packed", dict(dh=96, tq=130, tk=130, packed=True), {}),
    ("dh80-gen_dq<2>m-delta-dkv2<5>m-mask-70x129", dict(dh=80, tq=70, tk=129, mask_kind="full", mode="mask"), {}),
    ("dh128-gen_dq<2>-gen_dkv<2>-70x129", dict(dh=128, tq=70, tk=129), {}),
    ("dh160-gen_dq<3>-gen_dkv<3>-70x129", dict(dh=160, tq=70, tk=129), {}),
    ("dh160-gen_dq<3>m-gen_dkv<3>m-causal-130x130", dict(dh=160, tq=130, tk=130, mode="causal"), {}),
    ("dh40-gen_dq<1>-gen_dkv<1>-70x129-two_tiles-501", dict(dh=40, tq=70, tk=129), dict(attn_two_tiles=511 & ~10)),
    ("dh80-dq2<5>-gen_dkv<2>-70x129-two_tiles-without-32", dict(dh=80, tq=70, tk=129), dict(attn_two_tiles=511 & ~32)),
]


@pytest.mark.parametrize("parts", [(3,), (1, 2), (2,)], ids=["parts3", "parts1then2", "parts2alone"])
@pytest.mark.parametrize("cid,kw,opt", PARTS_SHAPES, ids=[c[0] for c in PARTS_SHAPES])
def test_backward_parts(G, options, cid, kw, opt, parts):
    options(**opt)
    run_attention(G, opt=opt, parts=parts, tag=f"{cid} parts {parts}", **kw)


# ---------------------------------------------------------------------------------------------
# kernels documented as bit-identical
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("t", [129, 160, 161, 197, 224])
def test_one2_equals_one_bit_for_bit(G, options, t):
    """attn_bwd_one2_kernel (8 waves, two key tiles per wave) keeps the reduction order of attn_bwd_one_kernel"""
    options(attn_one_pass=2)
    a = run_attention(G, dh=64, tq=t, tk=t, tag=f"one2 T={t}")
    options(attn_one_pass=1)
    b = run_attention(G, dh=64, tq=t, tk=t, opt=dict(attn_one_pass=1), tag=f"one T={t}")
    for name in ("dq", "dk", "dv"):
        assert torch.equal(a[name], b[name]), f"T={t}: {name} of the one2 and one kernels differ"


@pytest.mark.parametrize("tq,tk", [(129, 129), (160, 191), (255, 200), (256, 256)])
def test_persistent_forward_equals_one_shot_bit_for_bit(G, options, tq, tk):
    """attn_fwd_pers_kernel: same instruction order as attn_fwd_kernel<NB, plain>, O and lse bit-identical"""
    a = run_attention(G, dh=64, tq=tq, tk=tk, tag=f"fwd_pers {tq}x{tk}")
    options(attn_persistent=0)
    b = run_attention(G, dh=64, tq=tq, tk=tk, opt=dict(attn_persistent=0), tag=f"fwd one-shot {tq}x{tk}")
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["lse"], b["lse"])


# ---------------------------------------------------------------------------------------------
# dropout forms: attn_gen_{fwd,bwd_dq,bwd_dkv}<NH, plain | masked, DROP>
# ---------------------------------------------------------------------------------------------


DROP_CASES = []
for _dh, _tq, _tk in ((8, 37, 53), (64, 70, 129), (64, 130, 130), (80, 37, 53), (128, 70, 129), (160, 37, 53), (192, 70, 257)):
    for _mode in ("plain", "mask", "causal"):
        # the split backward calls at one shape per NH
        for _parts in ((3,), (1, 2), (2,)) if (_tq, _tk) == (70, 129) else ((3,),):
            _nh = (_dh + 63) // 64
            DROP_CASES.append(pytest.param(_dh, _tq, _tk, _mode, _parts,
                                           id=f"gen<{_nh},{_mode},DROP>-dh{_dh}-{_tq}x{_tk}-parts{''.join(map(str, _parts))}"))


for _dh in (40, 96, 136):  # the packed [B, T, 3, H, dh] buffer in place, one per NH
    for _mode in ("plain", "causal"):
        DROP_CASES.append(pytest.param(_dh, 130, 130, _mode, (3,), id=f"gen<{(_dh + 63) // 64},{_mode},DROP>-dh{_dh}-packed-130x130-parts3"))


@pytest.mark.parametrize("dh,tq,tk,mode,parts", DROP_CASES)
def test_dropout_forms(G, dh, tq, tk, mode, parts, request):
    run_attention(G, dh=dh, tq=tq, tk=tk, mode=mode, mask_kind="full" if mode == "mask" else None, dropout=0.3, parts=parts,
                  bsz=1 if tk > 200 else 2, packed="packed" in request.node.callspec.id, tag=request.node.callspec.id)


# ---------------------------------------------------------------------------------------------
# attn_probs / attn_probs_bwd
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["mask", "causal"])
@pytest.mark.parametrize("dh", [8, 64, 80, 192])
@pytest.mark.parametrize("tq,tk", [(37, 53), (17, 300)])
def test_attn_probs_and_bwd(G, dh, tq, tk, mode):
    bsz, heads = 2, 2
    d = heads * dh
    q, k = _randn((bsz, tq, d), dh + tq), _randn((bsz, tk, d), dh + tk + 1)
    causal = mode == "causal"
    mask = make_mask("full", bsz, heads, tq, tk) if mode == "mask" else None
    md = None if mask is None else G.index(mask.to(torch.uint8).to(DEV))
    Q, K, _, p, lse = attn_ref(q, k, k, heads, dh, mask, causal)
    # the kernel takes lse as an input: feed it the f32-rounded reference and compare with exp(s - that)
    lse32 = lse.float()
    s = (Q @ K.transpose(-1, -2)) / math.sqrt(dh)
    keep = p > 0
    want_p = torch.where(keep, torch.exp(s - lse32.double()[..., None]), torch.zeros_like(s))
    qd, kd = G.poisoned(q.to(DEV)), G.poisoned(k.to(DEV))
    lsed = G.poisoned(lse32.to(DEV))
    probs = ops.attn_probs(qd, kd, lsed, heads, mask=md, causal=causal, head_dim=dh)
    tag = f"attn_probs dh={dh} {tq}x{tk} {mode}"
    assert bool((probs.cpu()[~keep] == 0).all()), f"{tag}: a masked slot is not exactly 0"
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) / math.sqrt(dh)
    # an f32 fma chain of depth dh for the score, the scale product and the subtraction of lse, __expf (2 ulp and the
    # rounding of its argument): the argument's error times p
    cond_p = want_p * (sabs + lse32.double().abs()[..., None] + 1)
    assert_elementwise(probs, want_p, out_dtype=F32, ulps=4, cond=cond_p, k=dh + 8, what=tag)
    dp = torch.randn((bsz, heads, tq, tk), generator=_gen(dh + tq + tk), dtype=torch.float64).float()
    dq, dk = ops.attn_probs_bwd(qd, kd, lsed, G.poisoned(dp.to(DEV)), heads, mask=md, causal=causal, head_dim=dh)
    sc = 1.0 / math.sqrt(dh)
    dp64 = dp.double()
    t = (dp64 * want_p).sum(-1, keepdim=True)
    ds = sc * want_p * (dp64 - t)
    # dS in f32: P's error (cond_p), the f32 chain of t (depth <= Tk / 256 + 8 per thread and fold); then f32 fma chains
    # of depth Tk (dq) / Tq (dk) and one bf16 rounding
    ct = (dp64.abs() * want_p).sum(-1, keepdim=True)
    cds = sc * (want_p * (dp64.abs() + ct) + cond_p * (dp64.abs() + ct))
    back = lambda z: z.transpose(1, 2).reshape(bsz, -1, d)  # noqa: E731
    kk = dh + 8 + tk // 256 + 8
    assert_elementwise(dq, back(ds @ K), out_dtype=BF16, cond=back(cds @ K.abs()), k=kk + tk, what=f"{tag} bwd dq")
    assert_elementwise(dk, back(ds.transpose(-1, -2) @ Q), out_dtype=BF16, cond=back(cds.transpose(-1, -2) @ Q.abs()), k=kk + tq,
                       what=f"{tag} bwd dk")
    G.check()  # the [B, H, Tq, Tk] workspace and both outputs came from the guarded allocator
