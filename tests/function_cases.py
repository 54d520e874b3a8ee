"""The case table of the autograd-Function tests: one entry (or several, one per route) for every `torch.autograd.Function`
of the package, whatever module defines it (the host test walks every module of `cflearn_amd`: `functional`, `contrastive`,
`fused`, `rnn`, `nbm`, `rwkv`, `siren`, `pixelcnn` hold Functions today).  Imports without a GPU.

A `Case` holds
  * `make()`        the inputs on the CPU, in the dtypes the device gets (bf16 activations, f32 parameters, integer indices);
  * `diff`          the inputs that can ask for a gradient, `params` those of them that are parameters;
  * `call(t)`       the call through the public wrapper on the device tensors `t` (a dict by name) -> tensor or tuple;
  * `ref(v)`        the same operation in plain torch on float64 CPU values `v` — the values the kernels see: an input listed in
                    `seen` is rounded to that dtype first (the bf16 shadow of an f32 weight, the bf16 copy of an f32 activation);
  * `obvious(v)`    the torch call the reference restates (F.linear, F.conv2d, ...): the host test compares the two forwards;
  * `err`           the error model of every output (`y0`, `y1`, ...) and every gradient (by input name), in `assert_elementwise`'s
                    terms: |got - ref| <= ulps * ulp(dtype, |ref|) + 2^-24 * units(c).  `units` is written in units of one f32
                    rounding (2^-24) on a quantity computed from absolute values; one bf16 rounding of an intermediate is
                    BF = 2^16 such units on ITS absolute value (the unit roundoff of bf16 is 2^-8: half a spacing of 2^-7
                    relative to the lower end of the binade — the same figure helpers.attn_k_product uses).
                    No constant here was fitted to what a GPU returned: each follows from the line written at the case.
The conditioning context `c` carries `c.v` (float64 inputs), `c.y` (reference outputs), `c.dy` (output gradients) and `c.g`
(reference gradients); `ABS` asks the harness for the reference evaluated on absolute values (|x| @ |w|^T + |b|, and its gradients with
|dy|): the exact first-order bound of any sum of products with non-negative structure.
"""
import math
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from cflearn_amd import contrastive as HC
from cflearn_amd import functional as HF
from cflearn_amd import fused as HU
from cflearn_amd import nbm as HN
from cflearn_amd import ops
from cflearn_amd import pixelcnn as HP
from cflearn_amd import rnn as HR
from cflearn_amd import rwkv as HW
from cflearn_amd import siren as HS

import nbm_replay as NR
import nbm_weights as NW
import pixelcnn_replay as PR
import rnn_replay as RR
import rwkv_replay as WR
import siren_replay as SR

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BF = 2.0 ** 16  # one bf16 rounding (2^-8 relative) in units of 2^-24
ABS = "abs"


@dataclass
class Err:
    ulps: Any = 1.0                         # roundings to the output type itself (a callable c -> tensor: per element)
    units: Any = None                       # None, (k, ABS), ("self", k): k units on |ref| itself, or a callable c -> tensor of 2^-24 units
    dtype: Optional[torch.dtype] = None     # the type the value was last rounded to (default: bf16 activations, f32 parameters)


@dataclass
class Case:
    name: str
    fns: Tuple[Any, ...]
    make: Callable[[], Dict[str, Any]]
    diff: Tuple[str, ...]
    call: Callable[[Dict[str, Any]], Any]
    ref: Callable[[Dict[str, Any]], Any]
    err: Dict[str, Err]
    out: Tuple[torch.dtype, ...] = (BF16,)
    params: Tuple[str, ...] = ()
    seen: Dict[str, torch.dtype] = field(default_factory=dict)
    obvious: Optional[Callable[[Dict[str, Any]], Any]] = None
    nhwc: bool = False                       # run under functional.NHWC[0] (the UNet's channels_last hand-over)
    nhwc_in: Tuple[str, ...] = ()            # inputs handed over as channels_last views
    scope: Optional[Callable[[], Any]] = None  # a context manager factory around the call (fanin_links)
    modes: Optional[Tuple[str, ...]] = None  # parameter modes (default: all three when there are parameters)
    refused: Optional[Tuple[Any, str]] = None  # (exception type, why): the call must raise
    family: str = ""                         # one case per family also runs the dy forms
    dy_forms: bool = False
    nondiff_out: Tuple[int, ...] = ()        # outputs that take no gradient
    fast_gradcheck: bool = False
    dy_f32: bool = False                     # output gradients with a full f32 mantissa (f32 outputs whose dy must come back unrounded)


CASES: Dict[str, Case] = {}


def case(**kw: Any) -> Case:
    c = Case(**kw)
    assert c.name not in CASES, c.name
    CASES[c.name] = c
    return c


def _g(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def R(shape: Any, seed: int, scale: float = 1.0, dtype: torch.dtype = F32) -> torch.Tensor:
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return (torch.randn(shape, generator=_g(seed), dtype=F64) * scale).to(dtype)


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def sig64(x):
    return 1.0 / (1.0 + torch.exp(-x))


# =============================================================================================
# Linear family
# =============================================================================================


def _lin_ref(v, act=0, res=None):
    y = v["x"] @ v["w"].t()
    if v.get("b") is not None:
        y = y + v["b"]
    if act == 1:
        y = gelu64(y)
    elif act == 2:
        y = y * sig64(1.702 * y)
    if res is not None:
        y = y + v[res]
    return y


def _lin_obvious(v, act=0, res=None):
    y = F.linear(v["x"], v["w"], v.get("b"))
    if act == 1:
        y = F.gelu(y)
    elif act == 2:
        y = y * torch.sigmoid(1.702 * y)
    return y if res is None else y + v[res]


def _lin_make(rows, k, n, seed, x_dtype=BF16, res=None, bias=True):
    def make():
        d = {"x": R(rows + (k,), seed, 1.0, x_dtype), "w": R((n, k), seed + 1, 1.0 / math.sqrt(k))}
        if bias:
            d["b"] = R(n, seed + 2, 0.5)
        if res is not None:
            d["r"] = R(rows + (n,), seed + 3, 1.0, res)
        return d
    return make


def _lin_pre(c):
    v = c.v
    pre = v["x"] @ v["w"].t() + (v["b"] if v.get("b") is not None else 0.0)
    apre = v["x"].abs() @ v["w"].abs().t() + (v["b"].abs() if v.get("b") is not None else 0.0)
    return pre, apre


def _lin_err(k, n, rows, act=0, res=False, bias=True):
    """plain / residual: y = one rounding of an f32 sum of K exact products, the bias (and the residual): K + 2 roundings on ABS.
    dx: an f32 sum of N products of bf16 dy and bf16 w, one rounding.  dW: an f32 sum over the M rows (split-K adds a few partial
    sums: M + 8), stored in f32.  db: an f32 column sum of depth M."""
    m = int(math.prod(rows))
    if act == 0:
        e = {"y0": Err(1, (k + 2, ABS)), "x": Err(1, (n + 1, ABS)), "w": Err(1, (m + 8, ABS))}
        if bias:
            e["b"] = Err(1, (m + 8, ABS))
        if res:
            e["r"] = Err(1, None)  # dY handed on as it came: exact in bf16
        return e

    # GELU / quick-GELU epilogue: the activation by fast intrinsics (8 units on |pre| (1 + pre^2), as test_bf16_elementwise) of the
    # pre-activation THE KERNEL STORED, i.e. rounded to bf16 (test_gpu_gemm_epilogues: "of the pre-activation the kernel stored"): one
    # bf16 rounding of pre through |act'(pre)|, after the K + 1 roundings of the accumulator, which |act'| <= 1.13 carries over.
    # Backward: dpre = bf16(dy * act'(bf16 pre)): the derivative is taken at the ROUNDED pre-activation (one bf16 rounding of pre
    # times |act''| <= 0.8 for GELU, <= 0.86 for quick-GELU: 0.9), 8 units of intrinsics, then one bf16 rounding of dpre itself; every
    # gradient is a product with that dpre (depth N for dx, M for dW / db).
    def dact(p):
        if act == 1:
            return gelu_grad64(p)
        s = sig64(1.702 * p)
        return s * (1 + 1.702 * p * (1 - s))

    def y_units(c):
        pre, apre = _lin_pre(c)
        return 1.13 * (k + 2) * apre + 8 * pre.abs() * (1 + pre * pre) + BF * dact(pre).abs() * pre.abs()

    def dpre_abs(c):
        pre, apre = _lin_pre(c)
        dy = c.dy[0].abs()
        first = dy * dact(pre).abs()
        # error of dpre in 2^-24 units: rounding of dpre, intrinsics, the rounding of pre and the accumulator's own roundings
        e = BF * first + 8 * first * (1 + pre.abs()) ** 2 + dy * 0.9 * (BF * pre.abs() + (k + 2) * apre)
        return first, e

    def dx_units(c):
        first, e = dpre_abs(c)
        wa = c.v["w"].abs()
        return (n + 1) * (first @ wa) + e @ wa

    def dw_units(c):
        first, e = dpre_abs(c)
        xa = c.v["x"].abs().reshape(-1, k)
        f2, e2 = first.reshape(-1, n), e.reshape(-1, n)
        return (m + 8) * (f2.t() @ xa) + e2.t() @ xa

    def db_units(c):
        first, e = dpre_abs(c)
        return (m + 8) * first.reshape(-1, n).sum(0) + e.reshape(-1, n).sum(0)

    e = {"y0": Err(1, y_units), "x": Err(1, dx_units), "w": Err(1, dw_units)}
    if bias:
        e["b"] = Err(1, db_units)
    return e


def _linear_cases():
    for tag, rows, k, n in (("mfma", (2, 5), 24, 40), ("narrow", (2, 5), 10, 3)):
        for act_name, act in (("plain", 0), ("gelu", 1), ("qgelu", 2)):
            case(name=f"linear_{act_name}_{tag}", fns=(HF.LinearFn,), family="linear", dy_forms=(tag == "mfma" and act == 0),
                 make=_lin_make(rows, k, n, 100 + act), diff=("x", "w", "b"), params=("w", "b"), seen={"w": BF16},
                 call=lambda t, act=act: HF.linear(t["x"], t["w"], t["b"], act=act),
                 ref=lambda v, act=act: _lin_ref(v, act), obvious=lambda v, act=act: _lin_obvious(v, act),
                 err=_lin_err(k, n, rows, act))
        # residual operand bf16 (bf16 sum) and f32 (f32 sum: the residual stream keeps its type), and the f32 output
        case(name=f"linear_res_bf16_{tag}", fns=(HF.LinearFn,), make=_lin_make(rows, k, n, 110, res=BF16), diff=("x", "w", "b", "r"),
             params=("w", "b"), seen={"w": BF16}, call=lambda t: HF.linear(t["x"], t["w"], t["b"], residual=t["r"]),
             ref=lambda v: _lin_ref(v, 0, "r"), obvious=lambda v: _lin_obvious(v, 0, "r"), err=_lin_err(k, n, rows, res=True))
        e = _lin_err(k, n, rows, res=True)
        e["y0"] = Err(1, (k + 2, ABS), F32)
        e["r"] = Err(1, None, BF16)  # the f32 dy of the f32 sum is rounded once to bf16 for the GEMMs and handed on so
        for key in ("x", "w", "b"):  # ... which every other gradient of this case sees too: one bf16 rounding of dy, on ABS
            e[key] = Err(1, (e[key].units[0] + BF, ABS))
        case(name=f"linear_res_f32_{tag}", fns=(HF.LinearFn,), make=_lin_make(rows, k, n, 111, res=F32), diff=("x", "w", "b", "r"),
             params=("w", "b"), seen={"w": BF16}, out=(F32,), call=lambda t: HF.linear(t["x"], t["w"], t["b"], residual=t["r"]),
             ref=lambda v: _lin_ref(v, 0, "r"), obvious=lambda v: _lin_obvious(v, 0, "r"), err=e)
        e = _lin_err(k, n, rows)
        e["y0"] = Err(1, (k + 2, ABS), F32)
        for key in ("x", "w", "b"):
            e[key] = Err(1, (e[key].units[0] + BF, ABS))  # the f32 dy is rounded to bf16 first
        case(name=f"linear_out_f32_{tag}", fns=(HF.LinearFn,), make=_lin_make(rows, k, n, 112), diff=("x", "w", "b"),
             params=("w", "b"), seen={"w": BF16}, out=(F32,), call=lambda t: HF.linear(t["x"], t["w"], t["b"], out_f32=True),
             ref=_lin_ref, obvious=_lin_obvious, err=e)
    # an f32 activation is rounded to bf16 on the way in
    case(name="linear_f32_in", fns=(HF.LinearFn,), make=_lin_make((2, 5), 24, 40, 113, x_dtype=F32), diff=("x", "w", "b"),
         params=("w", "b"), seen={"w": BF16, "x": BF16}, call=lambda t: HF.linear(t["x"], t["w"], t["b"]),
         ref=_lin_ref, obvious=_lin_obvious, err=_lin_err(24, 40, (2, 5)))
    case(name="linear_no_bias", fns=(HF.LinearFn,), make=_lin_make((2, 5), 24, 40, 114, bias=False), diff=("x", "w"),
         params=("w",), seen={"w": BF16}, call=lambda t: HF.linear(t["x"], t["w"], None),
         ref=_lin_ref, obvious=_lin_obvious, err=_lin_err(24, 40, (2, 5), bias=False))


_linear_cases()


# ---- LoRA linear: y = x W^T + b + s (x A^T) Bm^T ------------------------------------------------------------------------------------------
LORA_S = 0.75


def _lora_lin_ref(v):
    h = v["x"] @ v["A"].t()
    return v["x"] @ v["w"].t() + v["b"] + LORA_S * (h @ v["Bm"].t())


def _lora_units(depth):
    """base as LinearFn; the low-rank path rounds h = x A^T (and dh = s dy Bm) to bf16 between its two products, and the
    read-modify-write of lora_up_add rounds the base result to bf16 before the adapter's share is added: two bf16 roundings on ABS
    besides the f32 chains (K or N or M deep, plus r = 4 for the adapter)"""
    return (depth + 4 + 8 + 2 * BF, ABS)


def _lora_linear_cases():
    rows, k, n, r = (2, 5), 24, 40, 4
    m = 10

    def make():
        d = _lin_make(rows, k, n, 120)()
        d["A"] = R((r, k), 123, 1.0 / math.sqrt(k))
        d["Bm"] = R((n, r), 124, 0.5)
        return d

    case(name="lora_linear", fns=(HF.LoRALinearFn,), family="lora", dy_forms=True, make=make, diff=("x", "w", "b", "A", "Bm"),
         params=("w", "b", "A", "Bm"), seen={"w": BF16, "A": BF16, "Bm": BF16},
         call=lambda t: HF.lora_linear(t["x"], t["w"], t["b"], t["A"], t["Bm"], LORA_S),
         ref=_lora_lin_ref, obvious=lambda v: F.linear(v["x"], v["w"] + LORA_S * v["Bm"] @ v["A"], v["b"]),
         err={"y0": Err(1, _lora_units(k)), "x": Err(1, _lora_units(n)), "w": Err(1, (m + 8, ABS)), "b": Err(1, (m + 8, ABS)),
              "A": Err(1, _lora_units(m + n)), "Bm": Err(1, _lora_units(m + k))})


_lora_linear_cases()


# ---- QKV: three bias-free projections as one GEMM when their weights are adjacent in one arena ---------------------------------------------


def _qkv_call(t):
    if HF.qkv_weights_adjacent(t["wq"], t["wk"], t["wv"]):
        return HF.qkv_linear(t["x"], t["wq"], t["wk"], t["wv"])
    return torch.cat([HF.linear(t["x"], t[n]) for n in ("wq", "wk", "wv")], -1)  # what modules.Attention does otherwise


def _qkv_cases():
    rows, c, d = (2, 5), 24, 16
    # as LinearFn; dx sums the three projections' shares: depth 3 D (one GEMM) or three rounded parts and two bf16 adds by
    # autograd on the fall-back path: 2 BF on ABS
    case(name="qkv_linear", fns=(HF.QKVLinearFn,), family="qkv", dy_forms=True, modes=("arena", "direct", "returned"),
         make=lambda: {"x": R(rows + (c,), 130, 1.0, BF16), "wq": R((d, c), 131, 0.2), "wk": R((d, c), 132, 0.2), "wv": R((d, c), 133, 0.2)},
         diff=("x", "wq", "wk", "wv"), params=("wq", "wk", "wv"), seen={"wq": BF16, "wk": BF16, "wv": BF16}, call=_qkv_call,
         ref=lambda v: torch.cat([v["x"] @ v[n].t() for n in ("wq", "wk", "wv")], -1),
         obvious=lambda v: F.linear(v["x"], torch.cat([v["wq"], v["wk"], v["wv"]], 0)),
         err={"y0": Err(1, (c + 2, ABS)), "x": Err(1, (3 * d + 1 + 2 * BF, ABS)), "wq": Err(1, (18, ABS)), "wk": Err(1, (18, ABS)),
              "wv": Err(1, (18, ABS))})


_qkv_cases()


# =============================================================================================
# Norms
# =============================================================================================


def _ln_ref(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _ln_ctx(c, eps, xkey="x"):
    x, w = c.v[xkey], c.v["w"]
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return x, w, (x - mu) * rstd, rstd


def _ln_err(d, rows, eps, out=BF16, extra_dy=0.0, link=False):
    """forward: two f32 sums of depth D (mean, variance), rsqrt, and the affine: the error of xhat is (D + 8) units on
    (|x| + |mu|) rstd plus the variance's relative (2 D + 8) units on |xhat| / 2 — taken together as (3 D + 16)(|x - mu| + |mu| + |x|) rstd |w|
    — plus 2 units on |w xhat| + |b|.
    dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w: three f32 sums of depth D on their absolute values, and the forward's
    error in xhat / rstd again: (3 D + 16) units on rstd (|g| + mean|g| + (|xhat| + 1) mean|g xhat|) (1 + |xhat|).
    dgamma = sum_rows dy xhat, dbeta = sum_rows dy: f32 sums of depth M (+ 8 for partial sums), xhat carrying (3 D + 16) units."""
    m = int(math.prod(rows))

    def y_units(c):
        x, w, xhat, rstd = _ln_ctx(c, eps)
        mu = x.mean(-1, keepdim=True)
        return (3 * d + 16) * ((x - mu).abs() + mu.abs() + x.abs()) * rstd * w.abs() + 2 * ((w * xhat).abs() + c.v["b"].abs())

    def dx_units(c):
        x, w, xhat, rstd = _ln_ctx(c, eps)
        dy = c.dy[0]
        ga = (dy * w).abs()
        base = rstd * (ga + ga.mean(-1, keepdim=True) + (xhat.abs() + 1) * (ga * xhat.abs()).mean(-1, keepdim=True)) * (1 + xhat.abs())
        u = (3 * d + 16 + extra_dy) * base
        if link:  # the fan-in gradient rides in as dx_add (bf16, exact) and is added in f32 before the one rounding: 1 unit
            u = u + c.dy[0].abs()
        return u

    def dg_units(c):
        x, w, xhat, rstd = _ln_ctx(c, eps)
        dy = c.dy[0].abs().reshape(-1, d)
        xa = xhat.abs().reshape(-1, d)
        return (m + 8 + extra_dy) * (dy * xa).sum(0) + (3 * d + 16) * (dy * (xa + 1)).sum(0)

    def db_units(c):
        return (m + 8 + extra_dy) * c.dy[0].abs().reshape(-1, d).sum(0)

    return {"y0": Err(1, y_units, out), "x": Err(1, dx_units, BF16), "w": Err(1, dg_units), "b": Err(1, db_units)}


def _ln_cases():
    eps = 1e-5
    for d in (8, 256):
        for xd, of32 in ((BF16, False), (F32, False), (F32, True)):
            name = f"layernorm_d{d}_{'bf16' if xd == BF16 else 'f32'}{'_outf32' if of32 else ''}"
            rows = (2, 3)
            # an f32 output's dy arrives in f32 and is rounded to bf16 first: BF more on the same quantities
            e = _ln_err(d, rows, eps, F32 if of32 else BF16, extra_dy=BF if of32 else 0.0)
            case(name=name, fns=(HF.LayerNormFn,), family="layernorm", dy_forms=(d == 256 and xd == BF16),
                 make=lambda d=d, xd=xd: {"x": R(rows + (d,), 200 + d, 1.5, xd), "w": 1.0 + R(d, 201, 0.3), "b": R(d, 202, 0.3)},
                 diff=("x", "w", "b"), params=("w", "b"), out=(F32 if of32 else BF16,),
                 call=lambda t, of32=of32: HF.layer_norm(t["x"], t["w"], t["b"], eps, out_f32=of32),
                 ref=lambda v: _ln_ref(v["x"], v["w"], v["b"], eps),
                 obvious=lambda v, d=d: F.layer_norm(v["x"], (d,), v["w"], v["b"], eps), err=e)

    # fan-in links: y = Linear(LN(x)) + x with the add in the GEMM's epilogue.  Inside fanin_links() the GEMM's dY reaches x through
    # the LayerNorm backward's dx_add (one rounding of the f32 sum); outside, autograd adds two bf16 gradients (two roundings).
    d, rows, n = 24, (2, 5), 24

    def make():
        return {"x": R(rows + (d,), 210, 1.5, BF16), "w": 1.0 + R(d, 211, 0.3), "b": R(d, 212, 0.3), "lw": R((n, d), 213, 0.2),
                "lb": R(n, 214, 0.3)}

    def call(t):
        h = HF.layer_norm(t["x"], t["w"], t["b"], eps)
        return HF.linear(h, t["lw"], t["lb"], residual=t["x"])

    def call_untaken(t):  # a link is offered (the scope is active) but the GEMM adds ANOTHER tensor back: nobody takes it
        h = HF.layer_norm(t["x"], t["w"], t["b"], eps)
        return HF.linear(h, t["lw"], t["lb"], residual=t["x"].detach() * 1)

    def ref(v, res=True):
        h = _ln_ref(v["x"], v["w"], v["b"], eps)
        return h @ v["lw"].t() + v["lb"] + (v["x"] if res else R(rows + (d,), 210, 1.5, BF16).double())  # (a constant: the same values)

    def chain_err(taken):
        """the LayerNorm's bf16 output h feeds the GEMM: BF on |h| through |lw|; backward: dh = bf16(dy lw) (BF) is the LayerNorm's
        dy.  Stated on ABS-free quantities: every term below is the LayerNorm / Linear model with the one extra bf16 rounding."""
        def ctx2(c):
            x, w, xhat, rstd = _ln_ctx(c, eps)
            h = xhat * w + c.v["b"]
            dh = c.dy[0] @ c.v["lw"]
            dha = c.dy[0].abs() @ c.v["lw"].abs()
            return x, w, xhat, rstd, h, dh, dha

        def y_units(c):
            x, w, xhat, rstd, h, dh, dha = ctx2(c)
            mu = x.mean(-1, keepdim=True)
            eh = (3 * d + 16) * ((x - mu).abs() + mu.abs() + x.abs()) * rstd * w.abs() + 2 * h.abs() + BF * h.abs()
            return eh @ c.v["lw"].abs().t() + (d + 3) * (h.abs() @ c.v["lw"].abs().t() + c.v["lb"].abs() + x.abs())

        def dx_units(c):
            x, w, xhat, rstd, h, dh, dha = ctx2(c)
            ga = dha * w.abs()
            base = rstd * (ga + ga.mean(-1, keepdim=True) + (xhat.abs() + 1) * (ga * xhat.abs()).mean(-1, keepdim=True)) * (1 + xhat.abs())
            u = (3 * d + 16 + BF + n + 1) * base + c.dy[0].abs()
            if not taken:
                u = u + BF * rstd * (ga + ga.mean(-1, keepdim=True) + xhat.abs() * (ga * xhat.abs()).mean(-1, keepdim=True))  # dx rounded before autograd's add
            return u

        def dg_units(c):
            x, w, xhat, rstd, h, dh, dha = ctx2(c)
            xa = xhat.abs().reshape(-1, d)
            da = dha.reshape(-1, d)
            return (10 + 8 + BF + n + 1) * (da * xa).sum(0) + (3 * d + 16) * (da * (xa + 1)).sum(0)

        def db_units(c):
            x, w, xhat, rstd, h, dh, dha = ctx2(c)
            return (10 + 8 + BF + n + 1) * dha.reshape(-1, d).sum(0)

        def dlw_units(c):
            x, w, xhat, rstd, h, dh, dha = ctx2(c)
            mu = x.mean(-1, keepdim=True)
            eh = (3 * d + 16) * ((x - mu).abs() + mu.abs() + x.abs()) * rstd * w.abs() + (2 + BF) * h.abs()
            dy2 = c.dy[0].abs().reshape(-1, n)
            return (10 + 8) * (dy2.t() @ h.abs().reshape(-1, d)) + dy2.t() @ eh.reshape(-1, d)

        return {"y0": Err(1, y_units), "x": Err(1, dx_units, BF16), "w": Err(1, dg_units), "b": Err(1, db_units),
                "lw": Err(1, dlw_units), "lb": Err(1, (18, ABS))}

    common = dict(fns=(HF.LayerNormFn, HF.LinearFn), make=make, diff=("x", "w", "b", "lw", "lb"), params=("w", "b", "lw", "lb"),
                  seen={"lw": BF16})
    obv = lambda v: F.linear(F.layer_norm(v["x"], (d,), v["w"], v["b"], eps), v["lw"], v["lb"]) + v["x"]  # noqa: E731
    case(name="layernorm_fanin_taken", call=call, ref=ref, obvious=obv, scope=HF.fanin_links, err=chain_err(True), **common)
    case(name="layernorm_fanin_plain", call=call, ref=ref, obvious=obv, err=chain_err(False), **common)
    e = chain_err(True)
    case(name="layernorm_fanin_untaken", call=call_untaken, ref=lambda v: ref(v, False),
         obvious=lambda v: F.linear(F.layer_norm(v["x"], (d,), v["w"], v["b"], eps), v["lw"], v["lb"]) + R(rows + (d,), 210, 1.5, BF16).double(),
         scope=HF.fanin_links, err=e, **common)


_ln_cases()


def _ln4d_ref(v, eps=1e-5):
    x = v["x"]
    b = x.shape[0]
    flat = x.reshape(b, -1)
    mu = flat.mean(1).view(b, 1, 1, 1)
    std = torch.sqrt(((flat - flat.mean(1, keepdim=True)) ** 2).sum(1) / (flat.shape[1] - 1)).view(b, 1, 1, 1)
    y = (x - mu) / (std + eps)
    if v.get("w") is not None:
        y = y * v["w"].view(1, -1, 1, 1) + v["b"].view(1, -1, 1, 1)
    return y


def _ln4d_cases():
    eps = 1e-5
    b, ch, h, w = 2, 3, 4, 5
    n = ch * h * w

    def stats(c):
        x = c.v["x"]
        flat = x.reshape(b, -1)
        mu = flat.mean(1).view(b, 1, 1, 1)
        std = torch.sqrt(((flat - flat.mean(1, keepdim=True)) ** 2).sum(1) / (n - 1)).view(b, 1, 1, 1)
        g = c.v["w"].view(1, -1, 1, 1) if c.v.get("w") is not None else torch.ones(1, ch, 1, 1, dtype=F64)
        return x, mu, std, (x - mu) / (std + eps), g

    # as LayerNorm with D = C H W per sample (sums of depth N, a square root and a division); the parameter sums run over B H W
    def y_units(c):
        x, mu, std, xhat, g = stats(c)
        u = (3 * n + 16) * ((x - mu).abs() + mu.abs() + x.abs()) / (std + eps) * g.abs() + 2 * (g * xhat).abs()
        return u + (2 * c.v["b"].abs().view(1, -1, 1, 1) if c.v.get("b") is not None else 0.0)

    def dx_units(c):
        x, mu, std, xhat, g = stats(c)
        ga = (c.dy[0] * g).abs()
        mean = lambda t: t.reshape(b, -1).mean(1).view(b, 1, 1, 1)  # noqa: E731
        return (3 * n + 16) * (ga + mean(ga) + (xhat.abs() + 1) * mean(ga * xhat.abs()) * n / (n - 1)) / (std + eps) * (1 + xhat.abs())

    def dw_units(c):
        x, mu, std, xhat, g = stats(c)
        dy = c.dy[0].abs()
        return (b * h * w + 8) * (dy * xhat.abs()).sum((0, 2, 3)) + (3 * n + 16) * (dy * (xhat.abs() + 1)).sum((0, 2, 3))

    def db_units(c):
        return (b * h * w + 8) * c.dy[0].abs().sum((0, 2, 3))

    def make(aff):
        def f():
            d = {"x": R((b, ch, h, w), 220, 1.5, BF16)}
            if aff:
                d["w"], d["b"] = 1.0 + R(ch, 221, 0.3), R(ch, 222, 0.3)
            return d
        return f

    case(name="layernorm4d_affine", fns=(HF.LayerNorm4dFn,), family="layernorm4d", dy_forms=True, make=make(True),
         diff=("x", "w", "b"), params=("w", "b"), call=lambda t: HF.layer_norm_4d(t["x"], t["w"], t["b"], eps), ref=_ln4d_ref,
         obvious=lambda v: (v["x"] - v["x"].mean((1, 2, 3), keepdim=True)) / (v["x"].reshape(b, -1).std(1).view(b, 1, 1, 1) + eps)
         * v["w"].view(1, -1, 1, 1) + v["b"].view(1, -1, 1, 1),
         err={"y0": Err(1, y_units), "x": Err(1, dx_units), "w": Err(1, dw_units), "b": Err(1, db_units)})
    case(name="layernorm4d_none", fns=(HF.LayerNorm4dFn,), make=make(False), diff=("x",),
         call=lambda t: HF.layer_norm_4d(t["x"], None, None, eps), ref=_ln4d_ref,
         obvious=lambda v: (v["x"] - v["x"].mean((1, 2, 3), keepdim=True)) / (v["x"].reshape(b, -1).std(1).view(b, 1, 1, 1) + eps),
         err={"y0": Err(1, y_units), "x": Err(1, dx_units)})
    # a weight without a bias: the kernel takes the affine pair or nothing, and says so (ops.layernorm4d_fwd)
    case(name="layernorm4d_weight_only", fns=(HF.LayerNorm4dFn,), make=lambda: {"x": R((b, ch, h, w), 220, 1.5, BF16), "w": 1.0 + R(ch, 221, 0.3)},
         diff=("x", "w"), params=("w",), call=lambda t: HF.layer_norm_4d(t["x"], t["w"], None, eps),
         ref=lambda v: _ln4d_ref({"x": v["x"]}) * v["w"].view(1, -1, 1, 1),
         obvious=lambda v: (v["x"] - v["x"].mean((1, 2, 3), keepdim=True)) / (v["x"].reshape(b, -1).std(1).view(b, 1, 1, 1) + eps)
         * v["w"].view(1, -1, 1, 1),
         err={"y0": Err(1, y_units), "x": Err(1, dx_units), "w": Err(1, dw_units)},
         refused=(ValueError, "weight and bias come together"))


_ln4d_cases()


def _gn_ref(v, groups, eps, silu, add=None, per_sample=False):
    x = v["x"]
    b, c = x.shape[:2]
    if add is not None:
        x = x + v[add][:, :, None, None]
    xg = x.reshape(b, groups, -1)
    mu = xg.mean(-1, keepdim=True)
    var = ((xg - mu) ** 2).mean(-1, keepdim=True)
    xhat = ((xg - mu) / torch.sqrt(var + eps)).reshape(x.shape)
    if per_sample:
        ge, be = v["ge"], v["be"]
        y = xhat * ge[:, :, None, None] + be[:, :, None, None]
    else:
        y = xhat * v["w"].view(1, -1, 1, 1) + v["b"].view(1, -1, 1, 1)
    return y * sig64(y) if silu else y


def _gn_err(groups, eps, silu, shape, add=None):
    """as LayerNorm with D = (C / G) H W per (sample, group); SiLU by fast intrinsics on the f32 result (8 units on |y| (1 + |z|)),
    its derivative (|silu'| <= 1.1, |silu''| <= 0.5) taken at the f32 pre-activation z recomputed in backward: the forward model's
    units on z through 0.5 |dy|.  dgamma / dbeta: f32 sums over H W then over B (depth H W + B + 8).  dadd: the sum of dx over H W."""
    b, ch, h, w = shape
    n = ch // groups * h * w

    def stats(c):
        x = c.v["x"] + (c.v[add][:, :, None, None] if add is not None else 0.0)
        xg = x.reshape(b, groups, -1)
        mu = xg.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xg - mu) ** 2).mean(-1, keepdim=True) + eps)
        xhat = ((xg - mu) * rstd).reshape(x.shape)
        gam, bet = c.v["w"].view(1, -1, 1, 1), c.v["b"].view(1, -1, 1, 1)
        z = xhat * gam + bet
        ez = ((3 * n + 16) * ((xg - mu).abs() + mu.abs() + xg.abs()) * rstd).reshape(x.shape) * gam.abs() + 2 * ((gam * xhat).abs() + bet.abs())
        gmean = lambda t: t.reshape(b, groups, -1).mean(-1, keepdim=True).expand(b, groups, n).reshape(x.shape)  # noqa: E731
        rs = rstd.expand(b, groups, n).reshape(x.shape)
        return x, xhat, rs, gam, z, ez, gmean

    def dz_of(c, z, ez):
        dy = c.dy[0]
        if not silu:
            return dy.abs(), torch.zeros_like(z)
        s = sig64(z)
        d1 = (s * (1 + z * (1 - s))).abs()
        return dy.abs() * d1, dy.abs() * (8 * d1 * (1 + z.abs()) ** 2 + 0.5 * ez)

    def y_units(c):
        x, xhat, rs, gam, z, ez, gmean = stats(c)
        if not silu:
            return ez
        return 1.1 * ez + 8 * (z * sig64(z)).abs() * (1 + z.abs())

    def dx_base(c):
        x, xhat, rs, gam, z, ez, gmean = stats(c)
        dz, edz = dz_of(c, z, ez)
        ga, ega = dz * gam.abs(), edz * gam.abs()
        bound = lambda q: rs * (q + gmean(q) + (xhat.abs() + 1) * gmean(q * xhat.abs())) * (1 + xhat.abs())  # noqa: E731
        return (3 * n + 16) * bound(ga) + bound(ega)

    def dg_units(c):
        x, xhat, rs, gam, z, ez, gmean = stats(c)
        dz, edz = dz_of(c, z, ez)
        return ((h * w + b + 8) * dz * xhat.abs() + (3 * n + 16) * dz * (xhat.abs() + 1) + edz * xhat.abs()).sum((0, 2, 3))

    def db_units(c):
        x, xhat, rs, gam, z, ez, gmean = stats(c)
        dz, edz = dz_of(c, z, ez)
        return ((h * w + b + 8) * dz + edz).sum((0, 2, 3))

    e = {"y0": Err(1, y_units), "x": Err(1, dx_base), "w": Err(1, dg_units), "b": Err(1, db_units)}
    if add is not None:
        # dadd[b, c] = sum over H W of the f32 dx (before its rounding): depth H W more on the same bound, stored in f32
        e[add] = Err(1, lambda c: (h * w + 9) * dx_base(c).sum((2, 3)), F32)
    return e


def _gn_cases():
    eps = 1e-5
    for tag, nhwc, shape, groups in (("nchw", False, (2, 6, 3, 5), 3), ("nhwc", True, (2, 16, 3, 5), 4)):
        for silu in (False, True):
            for with_add in (False, True):
                name = f"groupnorm_{tag}{'_silu' if silu else ''}{'_add' if with_add else ''}"
                b, ch, h, w = shape

                def make(shape=shape, with_add=with_add, ch=ch, b=b):
                    d = {"x": R(shape, 230, 1.5, BF16), "w": 1.0 + R(ch, 231, 0.3), "b": R(ch, 232, 0.3)}
                    if with_add:
                        d["add"] = R((b, ch), 233, 0.5)
                    return d

                diff = ("x", "w", "b") + (("add",) if with_add else ())
                case(name=name, fns=(HF.GroupNormFn,), family="groupnorm", dy_forms=(silu and with_add), make=make, diff=diff,
                     params=("w", "b"), nhwc=nhwc, nhwc_in=("x",) if nhwc else (),
                     call=lambda t, groups=groups, silu=silu, with_add=with_add: HF.group_norm(
                         t["x"], t["w"], t["b"], groups, eps, t["add"] if with_add else None, silu),
                     ref=lambda v, groups=groups, silu=silu, with_add=with_add: _gn_ref(v, groups, eps, silu, "add" if with_add else None),
                     obvious=lambda v, groups=groups, silu=silu, with_add=with_add: (lambda y: F.silu(y) if silu else y)(F.group_norm(
                         v["x"] + (v["add"][:, :, None, None] if with_add else 0.0), groups, v["w"], v["b"], eps)),
                     err=_gn_err(groups, eps, silu, shape, "add" if with_add else None))


_gn_cases()


def _ssa_cases():
    """ScaleShiftAffineFn feeding GroupNormFn's per-sample affine: gamma_eff = gamma (1 + scale), beta_eff = beta (1 + scale) + shift"""
    eps, groups, shape = 1e-5, 3, (2, 6, 3, 5)
    b, ch, h, w = shape
    n = ch // groups * h * w

    def call(t):
        ge, be = HF.scale_shift_affine(t["w"], t["b"], t["scale"], t["shift"])
        return HF.group_norm(t["x"], ge, be, groups, eps)

    def ref(v):
        ge = v["w"][None, :] * (1 + v["scale"])
        be = v["b"][None, :] * (1 + v["scale"]) + v["shift"]
        return _gn_ref({"x": v["x"], "ge": ge, "be": be}, groups, eps, False, per_sample=True)

    def obvious(v):
        y = F.group_norm(v["x"], groups, None, None, eps)
        return y * (v["w"].view(1, -1, 1, 1) * (1 + v["scale"][:, :, None, None])) + (v["b"].view(1, -1, 1, 1) * (1 + v["scale"][:, :, None, None])
                                                                                     + v["shift"][:, :, None, None])

    def stats(c):
        x = c.v["x"]
        xg = x.reshape(b, groups, -1)
        mu = xg.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xg - mu) ** 2).mean(-1, keepdim=True) + eps)
        xhat = ((xg - mu) * rstd).reshape(x.shape)
        op = (1 + c.v["scale"])
        ge = (c.v["w"][None, :] * op)[:, :, None, None]
        be = (c.v["b"][None, :] * op + c.v["shift"])[:, :, None, None]
        exh = ((3 * n + 16) * ((xg - mu).abs() + mu.abs() + xg.abs()) * rstd).reshape(x.shape)
        gmean = lambda t: t.reshape(b, groups, -1).mean(-1, keepdim=True).expand(b, groups, n).reshape(x.shape)  # noqa: E731
        return x, xhat, rstd.expand(b, groups, n).reshape(x.shape), ge, be, exh, gmean, op

    # the effective affine is formed in f32 torch arithmetic (2 roundings each), then GroupNorm's model with it
    def y_units(c):
        x, xhat, rs, ge, be, exh, gmean, op = stats(c)
        return exh * ge.abs() + 4 * ((ge * xhat).abs() + be.abs() + c.v["shift"].abs()[:, :, None, None])

    def dx_units(c):
        x, xhat, rs, ge, be, exh, gmean, op = stats(c)
        ga = (c.dy[0] * ge).abs()
        return (3 * n + 16 + 4) * rs * (ga + gmean(ga) + (xhat.abs() + 1) * gmean(ga * xhat.abs())) * (1 + xhat.abs())

    def dge(c):  # |dgamma_eff| [B, C] and its units: an f32 sum over H W of dy xhat
        x, xhat, rs, ge, be, exh, gmean, op = stats(c)
        dy = c.dy[0].abs()
        return (dy * xhat.abs()).sum((2, 3)), ((h * w + 8) * dy * xhat.abs() + (3 * n + 16) * dy * (xhat.abs() + 1)).sum((2, 3)), \
            dy.sum((2, 3)), (h * w + 8) * dy.sum((2, 3)), op

    def dw_units(c):
        a, ua, bb, ub, op = dge(c)
        return (ua * op.abs() + (b + 3) * a * op.abs()).sum(0)

    def db_units(c):
        a, ua, bb, ub, op = dge(c)
        return (ub * op.abs() + (b + 3) * bb * op.abs()).sum(0)

    def dscale_units(c):
        a, ua, bb, ub, op = dge(c)
        return ua * c.v["w"].abs()[None, :] + ub * c.v["b"].abs()[None, :] + 4 * (a * c.v["w"].abs()[None, :] + bb * c.v["b"].abs()[None, :])

    def dshift_units(c):
        a, ua, bb, ub, op = dge(c)
        return ub

    case(name="scale_shift_groupnorm", fns=(HF.ScaleShiftAffineFn, HF.GroupNormFn), family="scale_shift", dy_forms=True,
         make=lambda: {"x": R(shape, 240, 1.5, BF16), "w": 1.0 + R(ch, 241, 0.3), "b": R(ch, 242, 0.3), "scale": R((b, ch), 243, 0.3),
                       "shift": R((b, ch), 244, 0.3)},
         diff=("x", "w", "b", "scale", "shift"), params=("w", "b"), call=call, ref=ref, obvious=obvious,
         err={"y0": Err(1, y_units), "x": Err(1, dx_units), "w": Err(1, dw_units), "b": Err(1, db_units),
              "scale": Err(1, dscale_units, F32), "shift": Err(1, dshift_units, F32)})


_ssa_cases()


def _bn_cases():
    eps, mom = 1e-5, 0.1

    def ref(v, training, rm=None, rv=None):
        x = v["x"]
        dims = (0,) if x.dim() == 2 else (0, 2, 3)
        shp = (1, -1) if x.dim() == 2 else (1, -1, 1, 1)
        if training:
            mu = x.mean(dims, keepdim=True)
            var = ((x - mu) ** 2).mean(dims, keepdim=True)
        else:
            mu, var = rm.double().view(shp), rv.double().view(shp)
        y = (x - mu) / torch.sqrt(var + eps)
        if v.get("w") is not None:
            y = y * v["w"].view(shp) + v["b"].view(shp)
        return y

    for tag, shape in (("4d", (3, 4, 2, 3)), ("2d", (5, 4))):
        ch = shape[1]
        n = int(math.prod(shape)) // ch
        rm, rv = R(ch, 250, 0.3), 0.5 + R(ch, 251, 0.5).abs()
        for training in (True, False):
            for aff in (True, False):
                name = f"batchnorm_{tag}_{'train' if training else 'eval'}{'' if aff else '_noaffine'}"
                dims = (0,) if len(shape) == 2 else (0, 2, 3)
                shp = (1, -1) if len(shape) == 2 else (1, -1, 1, 1)

                def stats(c, training=training, dims=dims, shp=shp, rm=rm, rv=rv):
                    x = c.v["x"]
                    if training:
                        mu = x.mean(dims, keepdim=True)
                        var = ((x - mu) ** 2).mean(dims, keepdim=True)
                    else:
                        mu, var = rm.double().view(shp), rv.double().view(shp)
                    rstd = 1.0 / torch.sqrt(var + eps)
                    g = c.v["w"].view(shp) if c.v.get("w") is not None else torch.ones(1, dtype=F64).view((1,) * len(shp))
                    return x, mu, rstd, (x - mu) * rstd, g

                # as LayerNorm with the statistics over B H W per channel (depth N); eval: the running statistics are constants
                # (an rsqrt, a subtraction, the affine: 8 units), dx = dy gamma rstd (3 roundings)
                def y_units(c, stats=stats, n=n, shp=shp):
                    x, mu, rstd, xhat, g = stats(c)
                    u = (3 * n + 16) * ((x - mu).abs() + mu.abs() + x.abs()) * rstd * g.abs() + 2 * (g * xhat).abs()
                    return u + (2 * c.v["b"].abs().view(shp) if c.v.get("b") is not None else 0.0)

                def dx_units(c, stats=stats, n=n, dims=dims, training=training):
                    x, mu, rstd, xhat, g = stats(c)
                    ga = (c.dy[0] * g).abs()
                    if not training:
                        return 8 * ga * rstd
                    mean = lambda t: t.mean(dims, keepdim=True)  # noqa: E731
                    return (3 * n + 16) * rstd * (ga + mean(ga) + (xhat.abs() + 1) * mean(ga * xhat.abs())) * (1 + xhat.abs())

                def dw_units(c, stats=stats, n=n, dims=dims):
                    x, mu, rstd, xhat, g = stats(c)
                    dy = c.dy[0].abs()
                    return (n + 8) * (dy * xhat.abs()).sum(dims) + (3 * n + 16) * (dy * (xhat.abs() + 1)).sum(dims)

                def db_units(c, n=n, dims=dims):
                    return (n + 8) * c.dy[0].abs().sum(dims)

                def make(shape=shape, aff=aff, ch=ch):
                    d = {"x": R(shape, 252, 1.5, BF16)}
                    if aff:
                        d["w"], d["b"] = 1.0 + R(ch, 253, 0.3), R(ch, 254, 0.3)
                    return d

                def call(t, training=training, rm=rm, rv=rv):
                    dev = t["x"].device
                    return HF.batch_norm(t["x"], t.get("w"), t.get("b"), rm.clone().to(dev), rv.clone().to(dev), eps, mom, training)

                e = {"y0": Err(1, y_units), "x": Err(1, dx_units)}
                if aff:
                    e["w"], e["b"] = Err(1, dw_units), Err(1, db_units)
                case(name=name, fns=(HF.BatchNormFn,), family="batchnorm", dy_forms=(tag == "4d" and training and aff), make=make,
                     diff=("x", "w", "b") if aff else ("x",), params=("w", "b") if aff else (), call=call,
                     ref=lambda v, training=training, rm=rm, rv=rv: ref(v, training, rm, rv),
                     obvious=lambda v, training=training, rm=rm, rv=rv: F.batch_norm(v["x"], rm.double().clone(), rv.double().clone(), v.get("w"),
                                                                                    v.get("b"), training, mom, eps),
                     err=e)


_bn_cases()


# =============================================================================================
# Convolutions
# =============================================================================================


def _conv_err(taps, cin, cout, m):
    """y: an f32 sum of taps * Cin exact products and the bias, one rounding (assert_conv3x3_rows' model).  dx: a sum over
    taps * Cout products (depth taps * Cp with the zero filters), rounded once (row2im sums up to `taps` bf16-rounded GEMM rows'
    worth in f32 and rounds once on the im2row route: the [M, Kp] GEMM result is bf16 first — BF on ABS there).
    dW: an f32 sum over the M output positions (+ 8 partials); db: a column sum of depth M."""
    return {"y0": Err(1, (taps * cin + 2, ABS)), "x": Err(1, (taps * (cout + 32) + taps + 1 + BF, ABS)), "w": Err(1, (m + 8, ABS)),
            "b": Err(1, (m + 8, ABS))}


def _conv_cases():
    def mk(shape, wshape, seed, bias=True, x_dtype=BF16):
        def make():
            fan = wshape[1] * wshape[2] * wshape[3]
            d = {"x": R(shape, seed, 1.0, x_dtype), "w": R(wshape, seed + 1, 1.0 / math.sqrt(fan))}
            if bias:
                d["b"] = R(wshape[0], seed + 2, 0.3)
            return d
        return make

    def add(name, shape, wshape, stride, pad, seed, fns=(HF.Conv2dFn,), nhwc=False, groups=1, pad_hi=None, dy_forms=False, bias=True,
            x_dtype=BF16, diff=None):
        b, cin, h, w = shape
        cout, cin_g, kh, kw = wshape
        ho = (h + pad + (pad if pad_hi is None else pad_hi) - kh) // stride + 1
        wo = (w + pad + (pad if pad_hi is None else pad_hi) - kw) // stride + 1
        m = b * ho * wo

        def ref(v):
            x = v["x"]
            if pad_hi is not None:
                x = F.pad(x, (pad, pad_hi, pad, pad_hi))
                return F.conv2d(x, v["w"], v.get("b"), stride, 0, 1, groups)
            return F.conv2d(x, v["w"], v.get("b"), stride, pad, 1, groups)

        def explicit(v):  # unfold + matrix product: the restatement the host test holds against F.conv2d
            x = v["x"]
            p_lo, p_hi = pad, pad if pad_hi is None else pad_hi
            x = F.pad(x, (p_lo, p_hi, p_lo, p_hi))
            cols = F.unfold(x, (kh, kw), stride=stride)  # [B, Cin kh kw, L]
            cols = cols.view(b, groups, cin // groups * kh * kw, -1)
            wm = v["w"].view(groups, cout // groups, -1)
            y = torch.einsum("gok,bgkl->bgol", wm, cols).reshape(b, cout, ho, wo)
            return y if v.get("b") is None else y + v["b"].view(1, -1, 1, 1)

        e = _conv_err(kh * kw, cin_g, cout // groups, m)
        if not bias:
            e.pop("b")
        seen = {"w": BF16}
        if x_dtype != BF16:
            seen["x"] = BF16
        case(name=name, fns=fns, family="conv", dy_forms=dy_forms, make=mk(shape, wshape, seed, bias, x_dtype),
             diff=diff or (("x", "w", "b") if bias else ("x", "w")), params=("w", "b") if bias else ("w",), seen=seen, nhwc=nhwc,
             nhwc_in=("x",) if nhwc else (),
             call=lambda t: HF.conv2d(t["x"], t["w"], t.get("b"), stride, pad, 1, groups, pad_hi),
             ref=explicit, obvious=ref, err=e)

    add("conv_implicit", (2, 32, 5, 7), (32, 32, 3, 3), 1, 1, 300, dy_forms=True)
    add("conv_implicit_nhwc", (2, 32, 5, 7), (32, 32, 3, 3), 1, 1, 301, nhwc=True)
    add("conv_implicit_cout36", (1, 32, 5, 7), (40, 32, 3, 3), 1, 1, 302)  # Cp % 32 != 0: dX through GEMM + row2im
    add("conv_thin_head", (1, 32, 5, 7), (3, 32, 3, 3), 1, 1, 303)         # cp = 32 != cout = 3
    add("conv_pointwise", (2, 16, 3, 5), (24, 16, 1, 1), 1, 0, 304)
    add("conv_pointwise_nhwc", (2, 16, 3, 5), (24, 16, 1, 1), 1, 0, 305, nhwc=True)
    add("conv_pointwise_cout36", (2, 16, 3, 5), (36, 16, 1, 1), 1, 0, 306)  # cp = 40 != cout
    add("conv_im2row", (2, 3, 5, 7), (8, 3, 3, 3), 1, 1, 307)
    add("conv_im2row_f32_in", (2, 3, 5, 7), (8, 3, 3, 3), 1, 1, 308, x_dtype=F32)
    add("conv_im2row_stride2", (2, 3, 6, 7), (8, 3, 3, 3), 2, 1, 309)
    add("conv_im2row_no_bias", (2, 3, 5, 7), (8, 3, 3, 3), 1, 1, 310, bias=False)
    add("conv_pad_hi", (2, 8, 6, 7), (8, 8, 3, 3), 2, 0, 311, fns=(HF.Conv2dPadFn,), pad_hi=1)
    add("conv_depthwise", (2, 6, 5, 7), (6, 1, 3, 3), 1, 1, 312, fns=(HF.GroupedConv2dFn,), groups=6)
    add("conv_groups2", (2, 4, 5, 7), (6, 2, 3, 3), 1, 1, 313, fns=(HF.GroupedConv2dFn,), groups=2)


_conv_cases()


def _convT_cases():
    for cin in (8, 6):
        b, h, w, cout, k, stride, pad = 2, 3, 4, 5, 4, 2, 1
        m = b * h * w
        # forward: x_rows wt2 (depth Cin) rounded to bf16, then row2im sums up to (k / s)^2 = 4 of them in f32 and rounds once;
        # dx: a sum over Cout k k products; dW: over the B h w input positions
        case(name=f"conv_transpose_cin{cin}", fns=(HF.ConvTranspose2dFn,), family="conv_transpose", dy_forms=(cin == 8),
             make=lambda cin=cin: {"x": R((b, cin, h, w), 320 + cin, 1.0, BF16), "w": R((cin, cout, k, k), 321 + cin, 0.2)},
             diff=("x", "w"), params=("w",), seen={"w": BF16},
             call=lambda t: HF.conv_transpose2d(t["x"], t["w"], stride, pad),
             ref=lambda v: F.conv_transpose2d(v["x"], v["w"], None, stride, pad),
             obvious=lambda v: torch.autograd.functional.vjp(lambda z: F.conv2d(z, v["w"].detach(), None, stride, pad),
                                                             torch.zeros(b, cout, 2 * h, 2 * w, dtype=F64), v["x"].detach())[1],
             err={"y0": Err(1, (cin + 8 + BF, ABS)), "x": Err(1, (cout * k * k + 9, ABS)), "w": Err(1, (m + 8, ABS))})


_convT_cases()


def _direct_conv_cases():
    for stride in (1, 2):
        b, cin, h, w, cout = 2, 8, 5, 6, 16
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        case(name=f"direct_conv3x3_s{stride}", fns=(HF.DirectConv3x3Fn,), family="direct_conv", dy_forms=(stride == 1),
             make=lambda: {"x": R((b, cin, h, w), 330, 1.0, BF16), "w": R((cout, cin, 3, 3), 331, 0.1), "b": R(cout, 332, 0.3)},
             diff=("x", "w", "b"), params=("w", "b"), seen={"w": BF16},
             call=lambda t, stride=stride: HF.direct_conv3x3(t["x"], t["w"], t["b"], stride),
             ref=lambda v, stride=stride: F.conv2d(v["x"], v["w"], v["b"], stride, 1),
             obvious=lambda v, stride=stride: F.conv2d(F.pad(v["x"], (1, 1, 1, 1)), v["w"], v["b"], stride, 0),
             err={"y0": Err(1, (9 * cin + 2, ABS)), "x": Err(1, (9 * cout + 2, ABS)), "w": Err(1, (b * ho * wo + 8, ABS)),
                  "b": Err(1, (b * ho * wo + 8, ABS))})


_direct_conv_cases()


def _lora_conv_cases():
    for k in (1, 3):
        b, cin, h, w, cout, r = 2, 32 if k == 3 else 16, 4, 5, 32 if k == 3 else 24, 4
        pad = 1 if k == 3 else 0
        m = b * h * w

        def ref(v, pad=pad):
            hm = F.conv2d(v["x"], v["A"], None, 1, pad)
            return F.conv2d(v["x"], v["w"], v["b"], 1, pad) + LORA_S * F.conv2d(hm, v["Bm"])

        # as lora_linear, the base being the convolution's route
        u = lambda depth: (depth + r + 8 + 2 * BF, ABS)  # noqa: E731
        case(name=f"lora_conv_k{k}", fns=(HF.LoRAConv2dFn,), family="lora_conv", dy_forms=(k == 3),
             make=lambda k=k, cin=cin, cout=cout: {"x": R((b, cin, h, w), 340 + k, 1.0, BF16), "w": R((cout, cin, k, k), 341, 0.1),
                                                  "b": R(cout, 342, 0.3), "A": R((r, cin, k, k), 343, 0.1), "Bm": R((cout, r, 1, 1), 344, 0.5)},
             diff=("x", "w", "b", "A", "Bm"), params=("w", "b", "A", "Bm"), seen={"w": BF16, "A": BF16, "Bm": BF16},
             call=lambda t, pad=pad: HF.lora_conv2d(t["x"], t["w"], t["b"], 1, pad, 1, t["A"], t["Bm"], LORA_S),
             ref=ref, obvious=lambda v, pad=pad: F.conv2d(v["x"], v["w"] + LORA_S * torch.einsum("or,rckl->ockl", v["Bm"][:, :, 0, 0], v["A"]),
                                                         v["b"], 1, pad),
             err={"y0": Err(1, u(k * k * cin)), "x": Err(1, u(k * k * (cout + 32))), "w": Err(1, (m + 8, ABS)), "b": Err(1, (m + 8, ABS)),
                  "A": Err(1, u(m + cout)), "Bm": Err(1, u(m + k * k * cin))})


_lora_conv_cases()


# =============================================================================================
# Attention
# =============================================================================================


def _attn64(q, k, v, heads, dh, keep=None, causal=False, scale=None):
    b, tq, _ = q.shape
    tk = k.shape[1]
    sh = lambda t, n: t.reshape(b, n, heads, dh).transpose(1, 2)  # noqa: E731
    Q, K, V = sh(q, tq), sh(k, tk), sh(v, tk)
    s = Q @ K.transpose(-1, -2) * (1.0 / math.sqrt(dh) if scale is None else scale)
    m = torch.ones(tq, tk, dtype=torch.bool)
    if causal:
        m = torch.tril(m)
    if keep is not None:
        m = m & keep
    s = s.masked_fill(~m, -math.inf)
    p = torch.softmax(s, -1)
    return (p @ V).transpose(1, 2).reshape(b, tq, heads * dh), p


def _attn_err(heads, dh, tq, tk, keep, causal, names=("q", "k", "v"), packed=False, scale=None):
    """helpers.attn_k_product's model (P and dS rounded to bf16 before their products, f32 scores of depth dh, the online
    softmax's rescales): its units on P |V| for O, on P^T |dO| for dV, twice on |dS|^T |Q| scale / |dS| |K| scale for dK / dQ"""
    from helpers import attn_k_product

    kp = attn_k_product(dh, tk)
    sc = 1.0 / math.sqrt(dh) if scale is None else scale

    def parts(c):
        if packed:
            d = heads * dh
            q, k, v = c.v["qkv"][..., :d], c.v["qkv"][..., d:2 * d], c.v["qkv"][..., 2 * d:]
        else:
            q, k, v = (c.v[n] for n in names)
        b = q.shape[0]
        sh = lambda t, n: t.reshape(b, n, heads, dh).transpose(1, 2)  # noqa: E731
        Q, K, V = sh(q, tq), sh(k, tk), sh(v, tk)
        _, p = _attn64(q, k, v, heads, dh, keep, causal, scale)
        dO = sh(c.dy[0], tq)
        O = p @ V
        cdP = dO.abs() @ V.abs().transpose(-1, -2)
        cdS = p * (cdP + (dO.abs() * O.abs()).sum(-1, keepdim=True))
        back = lambda z: z.transpose(1, 2).reshape(b, -1, heads * dh)  # noqa: E731
        return Q, K, V, p, dO, cdS, back

    def o_units(c):
        Q, K, V, p, dO, cdS, back = parts(c)
        return kp * back(p @ V.abs())

    def dq_units(c):
        Q, K, V, p, dO, cdS, back = parts(c)
        return 2 * kp * back(cdS @ K.abs() * sc)

    def dk_units(c):
        Q, K, V, p, dO, cdS, back = parts(c)
        return 2 * kp * back(cdS.transpose(-1, -2) @ Q.abs() * sc)

    def dv_units(c):
        Q, K, V, p, dO, cdS, back = parts(c)
        return kp * back(p.transpose(-1, -2) @ dO.abs())

    if packed:
        return {"y0": Err(1, o_units), "qkv": Err(1, lambda c: torch.cat([dq_units(c), dk_units(c), dv_units(c)], -1))}
    return {"y0": Err(1, o_units), names[0]: Err(1, dq_units), names[1]: Err(1, dk_units), names[2]: Err(1, dv_units)}


def _attn_cases():
    b, heads = 2, 2
    for t in (5, 65):
        for dh in (40, 64):
            for kind in ("plain", "mask", "causal"):
                d = heads * dh
                keep = None
                if kind == "mask":
                    keep = torch.rand((t, t), generator=_g(400 + t)) > 0.3
                    keep[:, 0] = True
                causal = kind == "causal"
                big = t == 65
                # packed self-attention (the kernels of head width 64 by default, the `_dh` kernels otherwise)
                case(name=f"attn_packed_t{t}_dh{dh}_{kind}", fns=(HF.PackedSelfAttentionFn,), family="attn_packed",
                     dy_forms=(t == 5 and dh == 64 and kind == "plain"), fast_gradcheck=big,
                     make=lambda t=t, d=d: {"qkv": R((b, t, 3 * d), 401 + t + d, 1.0, BF16)}, diff=("qkv",),
                     call=lambda tt, keep=keep, causal=causal, dh=dh: HF.packed_self_attention(
                         tt["qkv"], heads, None if keep is None else keep.to(tt["qkv"].device), causal, 0.0, dh),
                     ref=lambda v, keep=keep, causal=causal, dh=dh, d=d: _attn64(v["qkv"][..., :d], v["qkv"][..., d:2 * d], v["qkv"][..., 2 * d:],
                                                                                heads, dh, keep, causal)[0],
                     obvious=lambda v, keep=keep, causal=causal, dh=dh, d=d, t=t: _sdpa(v["qkv"][..., :d], v["qkv"][..., d:2 * d],
                                                                                      v["qkv"][..., 2 * d:], heads, dh, keep, causal),
                     err=_attn_err(heads, dh, t, t, keep, causal, packed=True))
                case(name=f"attn_core_self_t{t}_dh{dh}_{kind}", fns=(HF.AttentionCoreFn,), family="attn_core",
                     dy_forms=(t == 5 and dh == 40 and kind == "plain"), fast_gradcheck=big,
                     make=lambda t=t, d=d: {"q": R((b, t, d), 402 + t, 1.0, BF16), "k": R((b, t, d), 403 + t, 1.0, BF16),
                                            "v": R((b, t, d), 404 + t, 1.0, BF16)}, diff=("q", "k", "v"),
                     call=lambda tt, keep=keep, causal=causal, dh=dh: HF.attention_core(
                         tt["q"], tt["k"], tt["v"], heads, None if keep is None else keep.to(tt["q"].device), causal, dh),
                     ref=lambda v, keep=keep, causal=causal, dh=dh: _attn64(v["q"], v["k"], v["v"], heads, dh, keep, causal)[0],
                     obvious=lambda v, keep=keep, causal=causal, dh=dh: _sdpa(v["q"], v["k"], v["v"], heads, dh, keep, causal),
                     err=_attn_err(heads, dh, t, t, keep, causal))
    # cross attention, Tq != Tk
    for tq, tk, dh, kind in ((5, 65, 40, "plain"), (65, 5, 64, "mask"), (5, 7, 64, "causal")):
        d = heads * dh
        keep = None
        if kind == "mask":
            keep = torch.rand((tq, tk), generator=_g(410)) > 0.3
            keep[:, 0] = True
        causal = kind == "causal"
        mk = lambda tq=tq, tk=tk, d=d: {"q": R((b, tq, d), 411, 1.0, BF16), "k": R((b, tk, d), 412, 1.0, BF16),  # noqa: E731
                                        "v": R((b, tk, d), 413, 1.0, BF16)}
        case(name=f"attn_core_cross_{tq}x{tk}_dh{dh}_{kind}", fns=(HF.AttentionCoreFn,), fast_gradcheck=True, make=mk, diff=("q", "k", "v"),
             call=lambda tt, keep=keep, causal=causal, dh=dh: HF.attention_core(
                 tt["q"], tt["k"], tt["v"], heads, None if keep is None else keep.to(tt["q"].device), causal, dh),
             ref=lambda v, keep=keep, causal=causal, dh=dh: _attn64(v["q"], v["k"], v["v"], heads, dh, keep, causal)[0],
             obvious=lambda v, keep=keep, causal=causal, dh=dh: _sdpa(v["q"], v["k"], v["v"], heads, dh, keep, causal),
             err=_attn_err(heads, dh, tq, tk, keep, causal))
    # output and weights: the weights f32 [B, H, Tq, Tk] rebuilt from the saved log-sum-exp; a gradient on them reaches q and k
    def weights_case(tq, tk, dh, kind):
        d = heads * dh
        keep = None
        if kind == "mask":
            keep = torch.rand((tq, tk), generator=_g(420)) > 0.3
            keep[:, 0] = True
        scale = 0.2
        e = _attn_err(heads, dh, tq, tk, keep, False, scale=scale)
        from helpers import attn_k_lse, attn_k_product

        # head_dim = 8 mod 16 without mask / causal: the forward's row sum comes out of the PV MFMA's ones column (attn.hip SUMCOL,
        # test_attention_edges): 2^-8 absolute on the saved lse, which the weights and their backward are rebuilt from
        sumcol = dh % 16 == 8 and kind == "plain"
        kl, kp = attn_k_lse(dh, tk, sumcol), attn_k_product(dh, tk)

        def pstuff(c, keep=keep, dh=dh, tq=tq, tk=tk):
            q, k = c.v["q"], c.v["k"]
            sh = lambda t, n: t.reshape(b, n, heads, dh).transpose(1, 2)  # noqa: E731
            Q, K = sh(q, tq), sh(k, tk)
            _, p = _attn64(q, k, c.v["v"], heads, dh, keep, False, scale)
            sabs = Q.abs() @ K.abs().transpose(-1, -2) * scale
            return Q, K, p, sabs

        # weights = exp(s - lse): the score's f32 chain (2 dh) and the lse's model (attn_k_lse) on p (|s| + |lse| + 1) <= p (2 sabs + 1)
        def p_units(c, pstuff=pstuff):
            Q, K, p, sabs = pstuff(c)
            return (2 * dh + 16 + kl) * p * (2 * sabs + (p * sabs).sum(-1, keepdim=True) + 1)

        # through the weights: dS = p (dP - sum p dP) in f32, rounded to bf16 for the products with K / Q (attn_probs_bwd): the
        # product model's units on |dS| |K| scale; the two shares of dq / dk are added by one more bf16 rounding (ops.add)
        def w_share(c, which, pstuff=pstuff, dh=dh, tq=tq, tk=tk):
            Q, K, p, sabs = pstuff(c)
            dP = c.dy[1].abs()
            cdS = p * (dP + (p * dP).sum(-1, keepdim=True))
            back = lambda z: z.transpose(1, 2).reshape(b, -1, heads * dh)  # noqa: E731
            return back(cdS @ K.abs() * scale) if which == "q" else back(cdS.transpose(-1, -2) @ Q.abs() * scale)

        def with_w(base, which):
            return lambda c: base(c) + (2 * kp + BF + (BF if sumcol else 0)) * w_share(c, which) + BF * c.g[which].abs()

        e2 = {"y0": e["y0"], "y1": Err(4, p_units, F32), "q": Err(1, with_w(e["q"].units, "q")), "k": Err(1, with_w(e["k"].units, "k")),
              "v": e["v"]}
        case(name=f"attn_weights_{tq}x{tk}_dh{dh}_{kind}", fns=(HF.AttentionWeightsFn,), family="attn_weights", dy_forms=(kind == "plain"),
             fast_gradcheck=True, out=(BF16, F32),
             make=lambda tq=tq, tk=tk, d=d: {"q": R((b, tq, d), 421, 1.0, BF16), "k": R((b, tk, d), 422, 1.0, BF16), "v": R((b, tk, d), 423, 1.0, BF16)},
             diff=("q", "k", "v"),
             call=lambda tt, keep=keep, dh=dh: HF.attention_with_weights(tt["q"], tt["k"], tt["v"], heads,
                                                                        None if keep is None else keep.to(tt["q"].device), False, dh, scale),
             ref=lambda v, keep=keep, dh=dh: _attn64(v["q"], v["k"], v["v"], heads, dh, keep, False, scale),
             obvious=lambda v, keep=keep, dh=dh: _sdpa(v["q"], v["k"], v["v"], heads, dh, keep, False, scale, True), err=e2)

    for args in ((5, 7, 40, "plain"), (65, 5, 64, "mask")):
        weights_case(*args)
    # the wide head (192 < head_dim <= 512) is forward only: an input that asks for a gradient is refused by name
    dh = 256
    mkw = lambda: {"q": R((1, 5, dh), 431, 1.0, BF16), "k": R((1, 7, dh), 432, 1.0, BF16), "v": R((1, 7, dh), 433, 1.0, BF16)}  # noqa: E731
    from helpers import attn_k_product as _kp
    case(name="attn_wide_forward", fns=(HF.AttentionWideFn,), family="attn_wide", make=mkw, diff=(), fast_gradcheck=True,
         call=lambda tt: HF.attention_wide(tt["q"], tt["k"], tt["v"], 1), ref=lambda v: _attn64(v["q"], v["k"], v["v"], 1, dh)[0],
         obvious=lambda v: _sdpa(v["q"], v["k"], v["v"], 1, dh, None, False),
         err={"y0": Err(1, lambda c: _kp(dh, 7) * (_attn64(c.v["q"], c.v["k"], c.v["v"], 1, dh)[1] @ c.v["v"].abs().view(1, 1, 7, dh)).transpose(1, 2).reshape(1, 5, dh))})
    case(name="attn_wide_refuses_grad", fns=(HF.AttentionWideFn,), make=mkw, diff=("q", "k", "v"), fast_gradcheck=True,
         call=lambda tt: HF.attention_wide(tt["q"], tt["k"], tt["v"], 1), ref=lambda v: _attn64(v["q"], v["k"], v["v"], 1, dh)[0],
         obvious=lambda v: _sdpa(v["q"], v["k"], v["v"], 1, dh, None, False),
         err={"y0": Err(), "q": Err(), "k": Err(), "v": Err()}, refused=(NotImplementedError, "forward-only"))


def _sdpa(q, k, v, heads, dh, keep, causal, scale=None, weights=False):
    b, tq, _ = q.shape
    tk = k.shape[1]
    sh = lambda t, n: t.reshape(b, n, heads, dh).transpose(1, 2)  # noqa: E731
    m = torch.ones(tq, tk, dtype=torch.bool)
    if causal:
        m = torch.tril(m)
    if keep is not None:
        m = m & keep
    o = F.scaled_dot_product_attention(sh(q, tq), sh(k, tk), sh(v, tk), attn_mask=m, scale=scale)
    o = o.transpose(1, 2).reshape(b, tq, heads * dh)
    if not weights:
        return o
    s = (sh(q, tq) @ sh(k, tk).transpose(-1, -2)) * scale
    return o, F.softmax(s.masked_fill(~m, -math.inf), -1)


_attn_cases()


# =============================================================================================
# Element-wise, layout and pooling Functions
# =============================================================================================


def _small_cases():
    sh4, sh3 = (2, 8, 3, 5), (2, 5, 16)
    x4 = lambda seed, dt=BF16: (lambda: {"x": R(sh4, seed, 1.5, dt)})  # noqa: E731

    # add: one rounding of an exact sum; both gradients are dy itself
    for tag, nhwc in (("nchw", False), ("nhwc", True)):
        case(name=f"add_{tag}", fns=(HF.AddFn,), family="add", dy_forms=not nhwc, nhwc=nhwc, nhwc_in=("a",) if nhwc else (),
             make=lambda: {"a": R(sh4, 500, 1.0, BF16), "b": R(sh4, 501, 1.0, BF16)}, diff=("a", "b"),
             call=lambda t: HF.add(t["a"], t["b"]), ref=lambda v: v["a"] + v["b"], obvious=lambda v: torch.add(v["a"], v["b"]),
             err={"y0": Err(1), "a": Err(0), "b": Err(0)})
    # GELU: test_bf16_elementwise's model (fast intrinsics, A&S erf): 8 units on |x| (1 + x^2) [(1 + |dy|...) for the derivative]
    case(name="gelu", fns=(HF.GeluFn,), family="gelu", dy_forms=True, make=lambda: {"x": R(sh3, 502, 2.0, BF16).clamp(-6, 6)}, diff=("x",),
         call=lambda t: HF.gelu(t["x"]), ref=lambda v: gelu64(v["x"]), obvious=lambda v: F.gelu(v["x"]),
         err={"y0": Err(1, lambda c: 8 * c.v["x"].abs() * (1 + c.v["x"] ** 2)),
              "x": Err(1, lambda c: 8 * c.v["x"].abs() * (1 + c.v["x"] ** 2) * (1 + c.dy[0].abs()))})
    # SiLU bf16: silu_f32's model (exp2 / rcp): 8 units on |y| (1 + |x|), |dy| (1 + |x|)^2
    for tag, nhwc in (("nchw", False), ("nhwc", True)):
        case(name=f"silu_bf16_{tag}", fns=(HF.SiLUBf16Fn,), family="silu_bf16", dy_forms=not nhwc, nhwc=nhwc, nhwc_in=("x",) if nhwc else (),
             make=x4(503), diff=("x",), call=lambda t: HF.silu_bf16(t["x"]), ref=lambda v: v["x"] * sig64(v["x"]),
             obvious=lambda v: F.silu(v["x"]),
             err={"y0": Err(1, lambda c: 8 * c.y[0].abs() * (1 + c.v["x"].abs())), "x": Err(1, lambda c: 8 * c.dy[0].abs() * (1 + c.v["x"].abs()) ** 2)})
    # scale: one product, one rounding
    case(name="scale_bf16", fns=(HF.ScaleBf16Fn,), family="scale", dy_forms=True, make=x4(504), diff=("x",),
         call=lambda t: HF.scale_bf16(t["x"], 0.37), ref=lambda v: v["x"] * float(torch.tensor(0.37, dtype=F32)),
         obvious=lambda v: torch.mul(v["x"], float(torch.tensor(0.37, dtype=F32))), err={"y0": Err(1, ("self", 2)), "x": Err(1, ("self", 2))})
    case(name="leaky_relu", fns=(HF.LeakyReLUFn,), family="leaky", dy_forms=True, make=x4(505), diff=("x",),
         call=lambda t: HF.leaky_relu(t["x"], 0.2), ref=lambda v: torch.where(v["x"] > 0, v["x"], float(torch.tensor(0.2, dtype=F32)) * v["x"]),
         obvious=lambda v: F.leaky_relu(v["x"], float(torch.tensor(0.2, dtype=F32))), err={"y0": Err(1, ("self", 2)), "x": Err(1, ("self", 2))})
    # global average pool: an f32 sum of depth H W, a division, one rounding; dx = dy / (H W): one rounding
    case(name="global_avg_pool", fns=(HF.GlobalAvgPoolFn,), family="gap", dy_forms=True, make=x4(506), diff=("x",),
         call=lambda t: HF.global_avg_pool(t["x"]), ref=lambda v: v["x"].sum((2, 3)) / 15.0, obvious=lambda v: F.adaptive_avg_pool2d(v["x"], 1)[:, :, 0, 0],
         err={"y0": Err(1, (17, ABS)), "x": Err(1, ("self", 2))})
    case(name="l2_normalize", fns=(HF.L2NormalizeFn,), family="l2norm", dy_forms=True, out=(F32,), make=lambda: {"x": R((5, 24), 507, 1.0)},
         diff=("x",), call=lambda t: HF.l2_normalize(t["x"]), ref=lambda v: v["x"] / torch.sqrt((v["x"] ** 2).sum(-1, keepdim=True)),
         obvious=lambda v: F.normalize(v["x"], dim=-1, eps=0.0),
         # an f32 sum of D squares, rsqrt, a product: D + 8 units on |y|; dx = inv (dy - y <dy, y>): a sum of depth D on its absolute values
         err={"y0": Err(1, lambda c: (24 + 8) * c.y[0].abs(), F32),
              "x": Err(1, lambda c: (2 * 24 + 16) * (c.dy[0].abs() + c.y[0].abs() * (c.dy[0].abs() * c.y[0].abs()).sum(-1, keepdim=True))
                       / torch.sqrt((c.v["x"] ** 2).sum(-1, keepdim=True)), F32)})
    case(name="silu_f32", fns=(HF.SiLUF32Fn,), family="silu_f32", dy_forms=True, out=(F32,), make=lambda: {"x": R((3, 32), 508, 2.0)}, diff=("x",),
         call=lambda t: HF.silu_f32(t["x"]), ref=lambda v: v["x"] * sig64(v["x"]), obvious=lambda v: F.silu(v["x"]),
         err={"y0": Err(2, lambda c: 8 * c.y[0].abs() * (1 + c.v["x"].abs()), F32),
              "x": Err(2, lambda c: 8 * c.dy[0].abs() * (1 + c.v["x"].abs()) ** 2, F32)})  # test_f32_silu_ema's model
    for tag, nhwc in (("nchw", False), ("nhwc", True)):
        # nearest up-sampling copies; its backward sums 4 bf16 values in f32 and rounds once
        case(name=f"upsample2_{tag}", fns=(HF.Upsample2Fn,), family="upsample", dy_forms=not nhwc, nhwc=nhwc, nhwc_in=("x",) if nhwc else (),
             make=x4(509), diff=("x",), call=lambda t: HF.upsample2(t["x"]),
             ref=lambda v: v["x"].repeat_interleave(2, 2).repeat_interleave(2, 3), obvious=lambda v: F.interpolate(v["x"], scale_factor=2, mode="nearest"),
             err={"y0": Err(0), "x": Err(1, (4, ABS))})
        # 2x2 average pooling: an f32 sum of 4 and a product with 1/4, one rounding; dx = dy / 4: exact in bf16 short of underflow
        case(name=f"avg_pool2_{tag}", fns=(HF.AvgPool2Fn,), family="avgpool2", dy_forms=not nhwc, nhwc=nhwc, nhwc_in=("x",) if nhwc else (),
             make=lambda: {"x": R((2, 8, 4, 6), 510, 1.5, BF16)}, diff=("x",), call=lambda t: HF.avg_pool2(t["x"]),
             ref=lambda v: v["x"].reshape(2, 8, 2, 2, 3, 2).sum((3, 5)) / 4.0, obvious=lambda v: F.avg_pool2d(v["x"], 2, 2),
             err={"y0": Err(1, (5, ABS)), "x": Err(1)})
    # reflection padding copies; its backward sums the up to 4 images of an element in f32 and rounds once
    case(name="reflect_pad2d", fns=(HF.ReflectPad2dFn,), family="reflect", dy_forms=True, make=x4(511), diff=("x",),
         call=lambda t: HF.reflect_pad2d(t["x"], (1, 2, 2, 1)),
         ref=lambda v: v["x"][:, :, [2, 1, 0, 1, 2, 1], :][:, :, :, [1, 0, 1, 2, 3, 4, 3, 2]], obvious=lambda v: F.pad(v["x"], (1, 2, 2, 1), mode="reflect"),
         err={"y0": Err(0), "x": Err(1, (4, ABS))})
    case(name="reflect_pad2d_f32_in", fns=(HF.ReflectPad2dFn,), make=x4(512, F32), diff=("x",), seen={"x": BF16},
         call=lambda t: HF.reflect_pad2d(t["x"], 1), ref=lambda v: v["x"][:, :, [1, 0, 1, 2, 1], :][:, :, :, [1, 0, 1, 2, 3, 4, 3]],
         obvious=lambda v: F.pad(v["x"], (1, 1, 1, 1), mode="reflect"), err={"y0": Err(0), "x": Err(1, (4, ABS))})
    # GEGLU: test_geglu's model
    def geglu_parts(c):
        v, g = c.v["x"][..., :8], c.v["x"][..., 8:]
        return v, g, g.abs() * (1 + g * g)

    case(name="geglu", fns=(HF.GegluFn,), family="geglu", dy_forms=True, make=lambda: {"x": R(sh3, 513, 2.0, BF16).clamp(-6, 6)}, diff=("x",),
         call=lambda t: HF.geglu(t["x"]), ref=lambda v: v["x"][..., :8] * gelu64(v["x"][..., 8:]),
         obvious=lambda v: v["x"][..., :8] * F.gelu(v["x"][..., 8:]),
         err={"y0": Err(1, lambda c: 8 * geglu_parts(c)[0].abs() * geglu_parts(c)[2]),
              "x": Err(1, lambda c: 8 * torch.cat([c.dy[0].abs() * geglu_parts(c)[2],
                                                   (c.dy[0] * geglu_parts(c)[0]).abs() * geglu_parts(c)[2] * (1 + geglu_parts(c)[1].abs())], -1))})
    # layout hops: copies
    for tag, nhwc in (("nchw", False), ("nhwc", True)):
        case(name=f"nchw_to_tokens_{tag}", fns=(HF.NchwToTokensFn,), family="to_tokens", dy_forms=not nhwc, nhwc=nhwc,
             nhwc_in=("x",) if nhwc else (), make=x4(514), diff=("x",), call=lambda t: HF.nchw_to_tokens(t["x"]),
             ref=lambda v: v["x"].permute(0, 2, 3, 1).reshape(2, 15, 8), obvious=lambda v: v["x"].flatten(2).transpose(1, 2), err={"y0": Err(0), "x": Err(0)})
        case(name=f"tokens_to_nchw_{tag}", fns=(HF.TokensToNchwFn,), family="to_nchw", dy_forms=not nhwc, nhwc=nhwc,
             make=lambda: {"x": R((2, 15, 8), 515, 1.0, BF16)}, diff=("x",), call=lambda t: HF.tokens_to_nchw(t["x"], 3, 5),
             ref=lambda v: v["x"].reshape(2, 3, 5, 8).permute(0, 3, 1, 2), obvious=lambda v: v["x"].transpose(1, 2).reshape(2, 8, 3, 5),
             err={"y0": Err(0), "x": Err(0)})
        case(name=f"concat_channels_{tag}", fns=(HF.ConcatChannelsFn,), family="concat", dy_forms=not nhwc, nhwc=nhwc,
             nhwc_in=("a",) if nhwc else (), make=lambda: {"a": R(sh4, 516, 1.0, BF16), "b": R((2, 16, 3, 5), 517, 1.0, BF16)}, diff=("a", "b"),
             call=lambda t: HF.concat_channels(t["a"], t["b"]), ref=lambda v: torch.cat([v["a"], v["b"]], 1),
             obvious=lambda v: torch.cat((v["a"], v["b"]), dim=1), err={"y0": Err(0), "a": Err(0), "b": Err(0)})
    # dropout / DropPath with the mask injected: x / (1 - p) where kept: one f32 product, one rounding
    p = 0.25
    keep = (torch.rand(sh3, generator=_g(518)) > p).to(torch.uint8)
    inv = 1.0 / float(torch.tensor(1.0 - p, dtype=F32))
    case(name="dropout_mask", fns=(HF.DropoutFn,), family="dropout", dy_forms=True, make=lambda: {"x": R(sh3, 519, 1.0, BF16)}, diff=("x",),
         call=lambda t: HF.dropout(t["x"], p, True, keep.to(t["x"].device)), ref=lambda v: v["x"] * keep.double() * inv,
         obvious=lambda v: torch.where(keep.bool(), v["x"] / (1 - p), torch.zeros_like(v["x"])), err={"y0": Err(1, ("self", 3)), "x": Err(1, ("self", 3))})
    pmask = torch.tensor([1.0, 0.0, 1.0])
    kp_ = float(torch.tensor(0.8, dtype=F32))
    case(name="drop_path_mask", fns=(HF.DropPathFn,), family="drop_path", dy_forms=True, make=lambda: {"x": R((3, 5, 16), 520, 1.0, BF16)},
         diff=("x",), call=lambda t: HF.drop_path(t["x"], 1.0 - kp_, True, pmask.to(t["x"].device)),
         ref=lambda v: v["x"] / (1.0 - (1.0 - kp_)) * pmask.double().view(3, 1, 1), obvious=lambda v: v["x"].div(1.0 - (1.0 - kp_)) * pmask.double().view(3, 1, 1),
         err={"y0": Err(1, ("self", 3)), "x": Err(1, ("self", 3))})


_small_cases()


def _patch_tokens_cases():
    b, ch, hw, patch, d = 2, 3, 8, 4, 16
    np_ = (hw // patch) ** 2
    k = ch * patch * patch

    def ref(v):
        cols = F.unfold(v["img"], patch, stride=patch).transpose(1, 2)  # [B, Np, C P P] in (c, ph, pw) order
        patches = cols @ v["w"].reshape(d, -1).t() + v["b"]
        x0 = torch.cat([v["head"].reshape(1, 1, d).expand(b, 1, d), patches], 1)
        return x0 + v["pos"].reshape(1, np_ + 1, d)

    def obvious(v):
        patches = F.conv2d(v["img"], v["w"], v["b"], stride=patch).flatten(2).transpose(1, 2)
        return torch.cat([v["head"].reshape(1, 1, d).expand(b, -1, -1), patches], 1) + v["pos"].reshape(1, np_ + 1, d)

    # patches = bf16(GEMM of depth K + bias), then + pos in f32: BF + K + 2 units on ABS; dpatches = bf16(dx0) (BF), dW / db sums over
    # the B Np rows; d head = sum over B of dx0[:, 0], d pos = sum over B of dx0 (f32 sums of the bf16-rounded dx0: B + BF units)
    case(name="patch_tokens", fns=(HF.PatchTokensFn,), family="patch_tokens", dy_forms=True, out=(F32,),
         make=lambda: {"img": R((b, ch, hw, hw), 600, 1.0), "w": R((d, ch, patch, patch), 601, 0.15), "b": R(d, 602, 0.3),
                       "head": R((1, 1, d), 603, 0.5), "pos": R((1, np_ + 1, d), 604, 0.5)},
         diff=("w", "b", "head", "pos"), params=("w", "b", "head", "pos"), seen={"img": BF16, "w": BF16},
         call=lambda t: HF.patch_tokens(t["img"], t["w"], t["b"], t["head"], t["pos"]), ref=ref, obvious=obvious,
         err={"y0": Err(1, (k + 3 + BF, ABS), F32), "w": Err(1, (b * np_ + 8 + BF, ABS)), "b": Err(1, (b * np_ + 8 + BF, ABS)),
              "head": Err(1, (b + 2 + BF, ABS)), "pos": Err(1, (b + 2 + BF, ABS))})


_patch_tokens_cases()


def _focal_case():
    b, c, gamma, eps = 5, 7, 2.0, 1e-6
    labels = torch.tensor([0, 6, 3, 3, 1])

    def ref(v):
        s = torch.softmax(v["x"], 1)
        p = s[torch.arange(b), labels] + eps
        return (-(torch.log(p)) * (1 - p) ** gamma).mean()

    def parts(c_):
        z = c_.v["x"]
        s = torch.softmax(z, 1)
        sy = s[torch.arange(b), labels]
        p = sy + eps
        om = 1 - p
        amp = (1 + z.abs().max()) * (1 + 1 / p)
        dom = 1 + p
        return s, sy, p, om, amp, dom

    # test_softmax_focal_labels_at_both_ends' models, with the 1 / B of the mean and the product with the incoming gradient (2 units)
    def loss_units(c_):
        s, sy, p, om, amp, dom = parts(c_)
        lp = torch.log(p).abs()
        return (b + 66) * (lp * om.abs() ** gamma * amp + lp * gamma * om.abs() ** (gamma - 1) * dom).sum() / b

    def d_units(c_):
        s, sy, p, om, amp, dom = parts(c_)
        dldp = -om ** gamma / p + gamma * om ** (gamma - 1) * torch.log(p)
        ddom = gamma * om.abs() ** (gamma - 1) / p + gamma * (gamma - 1) * om.abs() ** (gamma - 2) * torch.log(p).abs()
        cd = ((dldp.abs() + gamma * om.abs() ** (gamma - 1) + 1 / p) * sy * amp + ddom * dom * sy)[:, None] * (1 + s) / b
        return (c + 66) * cd * c_.dy[0].abs()

    case(name="focal_loss", fns=(HF.FocalLossFn,), family="focal", dy_forms=True, out=(F32,), make=lambda: {"x": R((b, c), 610, 2.0), "labels": labels},
         diff=("x",), call=lambda t: HF.focal_loss(t["x"], t["labels"], gamma, eps), ref=ref,
         obvious=lambda v: (-(torch.log(F.softmax(v["x"], 1).gather(1, labels[:, None])[:, 0] + eps))
                            * (1 - (F.softmax(v["x"], 1).gather(1, labels[:, None])[:, 0] + eps)) ** gamma).mean(),
         err={"y0": Err(1, loss_units, F32), "x": Err(5, d_units, F32)})


_focal_case()


def _embedding_cases():
    vocab, d, b, t = 7, 8, 2, 5
    idx = torch.tensor([[0, 3, 6, 3, 2], [2, 2, 5, 0, 3]])
    for tag, with_pos, pad_idx in (("plain", False, -1), ("pos", True, -1), ("pos_padding", True, 3)):
        def ref(v, with_pos=with_pos):
            y = v["w"][idx]
            return y + v["pos"].reshape(-1, d)[:t][None] if with_pos else y

        def mask_rows(c_, pad_idx=pad_idx):
            return (idx != pad_idx).double()[..., None]

        # the lookup copies f32 rows (+ one f32 add of the positional row); d table = a scatter-add of up to B T f32 rows (atomics,
        # any order): B T units on the absolute sum, rows of the padding index left out; d pos = a column sum over B of bf16(dy): BF + B + 8
        def dw_units(c_, pad_idx=pad_idx):
            dy = c_.dy[0].abs() * (idx != pad_idx).double()[..., None]
            out = torch.zeros(vocab, d, dtype=F64)
            out.index_add_(0, idx.reshape(-1), dy.reshape(-1, d))
            return (b * t) * out

        def ref_padded(v, with_pos=with_pos, pad_idx=pad_idx, ref=ref):
            # the forward reads the padding row like any other; only its gradient is withheld
            w = v["w"]
            if pad_idx >= 0:
                keep = torch.ones(vocab, 1, dtype=F64)
                keep[pad_idx] = 0
                w = w * keep + R((vocab, d), 620, 1.0).double() * (1 - keep)  # (the row as a constant: the values `make` gives it)
            return ref({**v, "w": w})

        def dpos_units(c_):
            full = torch.zeros_like(c_.v["pos"]).reshape(-1, d)
            full[:t] = (b + 8 + BF) * c_.dy[0].abs().sum(0)
            return full.reshape(c_.v["pos"].shape)

        def make(with_pos=with_pos):
            dd = {"idx": idx, "w": R((vocab, d), 620, 1.0)}
            if with_pos:
                dd["pos"] = R((1, t + 2, d), 621, 0.5)
            return dd

        e = {"y0": Err(1, None, F32), "w": Err(1, dw_units)}
        if with_pos:
            e["pos"] = Err(1, dpos_units)
        case(name=f"embedding_{tag}", fns=(HF.EmbeddingFn,), family="embedding", dy_forms=(tag == "pos"), out=(F32,), make=make,
             diff=("w", "pos") if with_pos else ("w",), params=("w", "pos") if with_pos else ("w",),
             call=lambda tt, with_pos=with_pos, pad_idx=pad_idx: HF.embedding(tt["idx"], tt["w"], tt["pos"] if with_pos else None, pad_idx),
             ref=ref_padded, obvious=lambda v, with_pos=with_pos, pad_idx=pad_idx: F.embedding(idx, v["w"], padding_idx=pad_idx if pad_idx >= 0 else None)
             + (v["pos"].reshape(-1, d)[:t][None] if with_pos else 0.0), err=e)
    # EOT pooling: x[arange(B), index] on the f32 stream; dx = a scatter of dy rows into zeros
    gi = torch.tensor([4, 0])
    case(name="gather_rows", fns=(HF.GatherRowsFn,), family="gather_rows", dy_forms=True, out=(F32,), make=lambda: {"x": R((2, 5, 8), 622, 1.0), "index": gi},
         diff=("x",), call=lambda tt: HF.gather_rows(tt["x"], tt["index"]), ref=lambda v: v["x"][torch.arange(2), gi],
         obvious=lambda v: v["x"].gather(1, gi.view(2, 1, 1).expand(2, 1, 8))[:, 0], err={"y0": Err(0, None, F32), "x": Err(0, None, F32)})


_embedding_cases()


def _time_proj_cases():
    b, k, ns = 3, 32, (8, 24)

    class _Lin:
        def __init__(self, w, bb):
            self.weight, self.bias = w, bb

    class _Blk:
        def __init__(self, w, bb):
            self.time_embedding = _Lin(w, bb)

    def call(t):
        blocks = [_Blk(t["w0"], t["b0"]), _Blk(t["w1"], t["b1"])]
        assert HF.time_proj_all(t["emb"], blocks), "the grouped time projection did not take this input"
        try:
            outs = tuple(HF.time_pre_lookup(blk, t["emb"]) for blk in blocks)
        finally:
            HF.time_pre_clear()
        assert all(o is not None for o in outs)
        return outs

    def ref(v):
        s = v["emb"] * sig64(v["emb"])
        return tuple(s @ v[f"w{i}"].t() + v[f"b{i}"] for i in range(2))

    # t16 = bf16(SiLU(emb)) (fast intrinsics: 8 units, then BF) feeds an f32 sum of depth K + the bias (test_time_projection's model);
    # d emb = SiLU'(emb) sum_i bf16(dy_i) W_i: BF on dy, depth sum N + 64; dW_i = bf16(dy_i)^T t16 over B rows: 2 BF + B + 8; db: BF + B + 8
    def silu_abs(c):
        e = c.v["emb"]
        s = sig64(e)
        return (e * s).abs(), (s * (1 + e * (1 - s))).abs()

    def y_units(i):
        def f(c):
            sa, _ = silu_abs(c)
            wa = c.v[f"w{i}"].abs()
            return (k + 2 + BF) * (sa @ wa.t() + c.v[f"b{i}"].abs()) + 8 * ((sa * (1 + c.v["emb"].abs())) @ wa.t())
        return f

    def demb_units(c):
        sa, da = silu_abs(c)
        gc = sum(c.dy[i].abs() @ c.v[f"w{i}"].abs() for i in range(2))
        return (sum(ns) + 64 + BF + 8) * gc * da * (1 + c.v["emb"].abs())

    def dw_units(i):
        def f(c):
            sa, _ = silu_abs(c)
            return (b + 8 + 2 * BF) * (c.dy[i].abs().t() @ sa) + 8 * (c.dy[i].abs().t() @ (sa * (1 + c.v["emb"].abs())))
        return f

    case(name="time_proj", fns=(HF.TimeProjAllFn, HF.TimeProjTapFn), family="time_proj", dy_forms=True, out=(F32, F32),
         make=lambda: {"emb": R((b, k), 630, 1.5), "w0": R((ns[0], k), 631, 0.2), "b0": R(ns[0], 632, 0.3), "w1": R((ns[1], k), 633, 0.2),
                       "b1": R(ns[1], 634, 0.3)},
         diff=("emb", "w0", "b0", "w1", "b1"), params=("w0", "b0", "w1", "b1"), seen={"w0": BF16, "w1": BF16}, call=call, ref=ref,
         obvious=lambda v: tuple(F.linear(F.silu(v["emb"]), v[f"w{i}"], v[f"b{i}"]) for i in range(2)),
         err={"y0": Err(1, y_units(0), F32), "y1": Err(1, y_units(1), F32), "emb": Err(2, demb_units, F32), "w0": Err(1, dw_units(0)),
              "w1": Err(1, dw_units(1)), "b0": Err(1, lambda c: (b + 8 + BF) * c.dy[0].abs().sum(0)),
              "b1": Err(1, lambda c: (b + 8 + BF) * c.dy[1].abs().sum(0))})


_time_proj_cases()


def _ml_encode_case():
    # columns: 0 numerical, 1 one-hot (3 values), 2 embedded (4 values -> 2 wide), 3 numerical
    b = 5
    plan = torch.tensor([[0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [1, 1, 0, 0, 3, 0], [1, 1, 1, 0, 3, 0], [1, 1, 2, 0, 3, 0],
                         [2, 2, 0, 0, 4, 2], [2, 2, 1, 0, 4, 2]], dtype=torch.int32)
    cat1 = torch.tensor([0., 2., 1., 5., 2.])   # 5 >= 3: imputed to 0
    cat2 = torch.tensor([3., 0., 0., 2., 1.])

    def make():
        x = R((b, 4), 640, 1.0)
        x[:, 1], x[:, 2] = cat1, cat2
        return {"x": x, "table": R((4, 2), 641, 1.0), "plan": plan}

    i1 = torch.where(cat1 >= 3, torch.zeros_like(cat1), cat1).long()
    i2 = cat2.long()

    def ref(v):
        return torch.cat([v["x"][:, [0, 3]], F.one_hot(i1, 3).double() + 0.0 * v["x"][:, 1:2], v["table"][i2] + 0.0 * v["x"][:, 2:3]], 1)

    def call(t):
        ptrs = torch.tensor([t["table"].data_ptr()], dtype=torch.int64).to(t["x"].device)
        return HF.MLEncodeFn.apply(t["x"], t["plan"], ptrs, 7, t["table"])

    # copies; d table = a scatter-add of B f32 rows (B units on the absolute sum); dx = dout on the numerical columns, 0 elsewhere
    def dt_units(c):
        out = torch.zeros(4, 2, dtype=F64)
        out.index_add_(0, i2, c.dy[0][:, 5:7].abs())
        return b * out

    case(name="ml_encode", fns=(HF.MLEncodeFn,), family="ml_encode", dy_forms=True, out=(F32,), make=make, diff=("x", "table"), params=("table",),
         call=call, ref=ref, obvious=lambda v: torch.cat([v["x"][:, [0, 3]], F.one_hot(i1, 3).double(), F.embedding(i2, v["table"])], 1),
         err={"y0": Err(0, None, F32), "x": Err(0, None, F32), "table": Err(1, dt_units)})


_ml_encode_case()


# =============================================================================================
# contrastive.py
# =============================================================================================


def _clip_cases():
    b, d = 5, 24

    def feats(seed):
        x = R((b, d), seed, 1.0)
        return x / x.norm(dim=-1, keepdim=True)

    def sim_ref(v):
        return torch.exp(v["ls"]) * (v["img"] @ v["txt"].t())

    # s = exp(logit_scale) in f32 torch arithmetic (2 units), then cfhip_sgemm_f32's model: an FMA chain of depth D and two products
    # with the scale: D + 4 units on s |I| |T|^T; the backward products have depth B (d img, d txt) and B D (d logit_scale)
    case(name="similarity", fns=(HC.SimilarityFn,), family="similarity", dy_forms=True, out=(F32,),
         make=lambda: {"img": feats(700), "txt": feats(701), "ls": torch.tensor(1.3)}, diff=("img", "txt", "ls"), params=("ls",),
         call=lambda t: HC.similarity_logits(t["img"], t["txt"], t["ls"]), ref=sim_ref,
         obvious=lambda v: v["ls"].exp() * v["img"] @ v["txt"].t(),
         err={"y0": Err(1, (d + 4, ABS), F32), "img": Err(1, (b + 4, ABS), F32), "txt": Err(1, (b + 4, ABS), F32),
              "ls": Err(1, (b * b + d + 8, ABS))})

    def loss_ref(v):
        s = torch.exp(v["ls"])
        li, lt = s * v["img"] @ v["txt"].t(), s * v["txt"] @ v["img"].t()
        lab = torch.arange(b)
        pick = lambda l: -(torch.log_softmax(l, 1)[lab, lab]).mean()  # noqa: E731
        return ((pick(li) + pick(lt)) / 2).reshape(1)

    def loss_ctx(c):
        s = torch.exp(c.v["ls"])
        I, T = c.v["img"], c.v["txt"]
        li, lt = s * I @ T.t(), s * T @ I.t()
        ali = s * (I.abs() @ T.abs().t())
        pi, pt = torch.softmax(li, 1), torch.softmax(lt, 1)
        eye = torch.eye(b, dtype=F64)
        return s, I, T, li, lt, ali, pi, pt, eye

    # logits carry (D + 4) units on their absolute products; log-softmax: libm exp / log of arguments up to |l|: (1 + |l|) units, and an
    # f32 row sum of depth B; the loss is a sum over 2 B rows.  Every logit error moves the loss by <= |p - onehot| / (2 B).
    def loss_units(c):
        s, I, T, li, lt, ali, pi, pt, eye = loss_ctx(c)
        per = lambda l, p, al: ((p - eye).abs() * ((d + 4) * al + 8 * (1 + l.abs()))).sum() + (b + 16) * (l.abs().max() + math.log(b))  # noqa: E731
        return (per(li, pi, ali) + per(lt, pt, ali.t())) / (2 * b) + (2 * b + 8) * c.y[0].abs()

    # dlogits = (p - onehot) / (2 B), each p with (1 + |l|) (B + 16) units and the logit's own error through |dp / dl| <= p;
    # then a product of depth B with the features and the scale s g (4 more)
    def dl_units(c, l, p, al):
        return ((b + 16 + 8) * (1 + l.abs()) * p + p * (d + 4) * al + 4 * (p - c_eye(b)).abs()) / (2 * b)

    def c_eye(n):
        return torch.eye(n, dtype=F64)

    def dimg_units(c):
        s, I, T, li, lt, ali, pi, pt, eye = loss_ctx(c)
        g = c.dy[0].abs() * s
        ui, ut = dl_units(c, li, pi, ali), dl_units(c, lt, pt, ali.t())
        di, dt = (pi - eye).abs() / (2 * b), (pt - eye).abs() / (2 * b)
        return g * ((ui + (b + 6) * di) @ T.abs() + (ut.t() + (b + 6) * dt.t()) @ T.abs()) + 2 * c.g["img"].abs()

    def dtxt_units(c):
        s, I, T, li, lt, ali, pi, pt, eye = loss_ctx(c)
        g = c.dy[0].abs() * s
        ui, ut = dl_units(c, li, pi, ali), dl_units(c, lt, pt, ali.t())
        di, dt = (pi - eye).abs() / (2 * b), (pt - eye).abs() / (2 * b)
        return g * ((ut + (b + 6) * dt) @ I.abs() + (ui.t() + (b + 6) * di.t()) @ I.abs()) + 2 * c.g["txt"].abs()

    def dls_units(c):
        s, I, T, li, lt, ali, pi, pt, eye = loss_ctx(c)
        ui, ut = dl_units(c, li, pi, ali), dl_units(c, lt, pt, ali.t())
        di, dt = (pi - eye).abs() / (2 * b), (pt - eye).abs() / (2 * b)
        tot = (ui * li.abs() + di * ((d + 4) * ali + (b * b + 8) * li.abs())).sum() + (ut * lt.abs() + dt * ((d + 4) * ali.t() + (b * b + 8) * lt.abs())).sum()
        return (tot * c.dy[0].abs()).reshape(())

    case(name="clip_loss", fns=(HC.ClipLossFn,), family="clip_loss", dy_forms=True, out=(F32,),
         make=lambda: {"img": feats(702), "txt": feats(703), "ls": torch.tensor(1.3)}, diff=("img", "txt", "ls"), params=("ls",),
         call=lambda t: HC.clip_contrastive_loss(t["img"], t["txt"], t["ls"]), ref=loss_ref,
         obvious=lambda v: ((F.cross_entropy(v["ls"].exp() * v["img"] @ v["txt"].t(), torch.arange(b))
                             + F.cross_entropy(v["ls"].exp() * v["txt"] @ v["img"].t(), torch.arange(b))) / 2).reshape(1),
         err={"y0": Err(2, loss_units, F32), "img": Err(2, dimg_units, F32), "txt": Err(2, dtxt_units, F32), "ls": Err(2, dls_units)})

    # the gather over ranks, in a one-process group: forward a copy, backward this rank's slice of the sum: a copy again
    def gather_call(t):
        import torch.distributed as dist

        assert dist.is_initialized(), "the harness initialises a one-process group for this case"
        return HC.gather_rows_with_grad(t["x"])

    case(name="gather_rows_with_grad", fns=(HC.GatherRowsWithGradFn,), family="gather_with_grad", dy_forms=True, out=(F32,),
         make=lambda: {"x": R((3, 8), 704, 1.0)}, diff=("x",), call=gather_call, ref=lambda v: v["x"] * 1.0, obvious=lambda v: v["x"].clone(),
         err={"y0": Err(0, None, F32), "x": Err(0, None, F32)})


_clip_cases()


# =============================================================================================
# fused.py: one pre-norm transformer block as one node (and a one-block stack)
# =============================================================================================

MIX = dict(b=2, t=5, d=64, heads=1, hid=128, eps=1e-5)
MIX_PARAMS = ("ln1_w", "ln1_b", "in_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")


def _mix_make():
    d, hid = MIX["d"], MIX["hid"]
    return {"x": R((MIX["b"], MIX["t"], d), 800, 1.0, BF16), "ln1_w": 1.0 + R(d, 801, 0.2), "ln1_b": R(d, 802, 0.2),
            "in_w": R((3 * d, d), 803, 1.0 / math.sqrt(d)), "qkv_b": R(3 * d, 804, 0.2), "out_w": R((d, d), 805, 1.0 / math.sqrt(d)),
            "out_b": R(d, 806, 0.2), "ln2_w": 1.0 + R(d, 807, 0.2), "ln2_b": R(d, 808, 0.2), "w1": R((hid, d), 809, 1.0 / math.sqrt(d)),
            "b1": R(hid, 810, 0.2), "w2": R((d, hid), 811, 1.0 / math.sqrt(hid)), "b2": R(d, 812, 0.2)}


def _mix_ref(v):
    """x1 = x + out(attn(LN1(x) in_w^T + qkv_b)); y = x1 + W2 gelu(W1 LN2(x1) + b1) + b2.  On the GPU the block is walked link by link
    on the intermediates it stored (test_gpu_function_grads.test_mixing_block_and_stack): `Err(1, "mix")` names that model."""
    r = lambda name, t: t  # noqa: E731  (the names of what the block stores in bf16)
    d, eps = MIX["d"], MIX["eps"]
    ln1 = r("ln1", _ln_ref(v["x"], v["ln1_w"], v["ln1_b"], eps))
    qkv = r("qkv", ln1 @ v["in_w"].t() + v["qkv_b"])
    o = r("o", _attn64(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], MIX["heads"], d // MIX["heads"])[0])
    x1 = r("x1", v["x"] + o @ v["out_w"].t() + v["out_b"])
    ln2 = r("ln2", _ln_ref(x1, v["ln2_w"], v["ln2_b"], eps))
    h = r("h", gelu64(r("pre", ln2 @ v["w1"].t() + v["b1"])))
    return x1 + h @ v["w2"].t() + v["b2"]


def _mix_obvious(v):
    d, eps = MIX["d"], MIX["eps"]
    ln1 = F.layer_norm(v["x"], (d,), v["ln1_w"], v["ln1_b"], eps)
    qkv = F.linear(ln1, v["in_w"], v["qkv_b"])
    o = _sdpa(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], MIX["heads"], d // MIX["heads"], None, False)
    x1 = v["x"] + F.linear(o, v["out_w"], v["out_b"])
    return x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, (d,), v["ln2_w"], v["ln2_b"], eps), v["w1"], v["b1"])), v["w2"], v["b2"])


def _mixing_cases():
    seen = {n: BF16 for n in ("in_w", "out_w", "w1", "w2")}
    common = dict(make=_mix_make, diff=("x",) + MIX_PARAMS, params=MIX_PARAMS, seen=seen, ref=_mix_ref, obvious=_mix_obvious, fast_gradcheck=True,
                  modes=("direct", "arena"),  # every gradient of a fused block is written straight into `.grad` (modules._fusable)
                  err={k: Err(1, "mix") for k in ("y0", "x") + MIX_PARAMS})
    case(name="mixing_block", fns=(HU.MixingBlockFn,), family="mixing_block", dy_forms=True,
         call=lambda t: HU.mixing_block(t["x"], *[t[n] for n in MIX_PARAMS], MIX["heads"], MIX["eps"], MIX["eps"], None, False, False), **common)
    case(name="mixing_stack", fns=(HU.MixingStackFn,), family="mixing_stack", dy_forms=True,
         call=lambda t: HU.mixing_stack(t["x"], ((MIX["heads"], MIX["eps"], MIX["eps"], False),), None, False, [t[n] for n in MIX_PARAMS]), **common)


_mixing_cases()


# =============================================================================================
# rnn: the recurrence of one GRU / LSTM layer and the two-word input projection
# =============================================================================================
# Shapes: B = 17 (two workgroups of 16 rows, the second ragged), T = 3 (T = 1 would make dW_hh identically zero: the Function has no
# initial-state input), H = 40 (padded to Kp = 64 / Np = 48 in the pack) and H = 8; W_hh at the layer's own initial deviation
# (uniform(-1, 1) / sqrt(H): 0.58 / sqrt(H)), since every step of the worst-case carry below multiplies a bound by sum_k |W_hh|, which
# the random signs of the values do not follow: at 1.5 / sqrt(H) the bound of db_hh (H = 40) reached the gradient's own size and
# would have held nothing to account.  The float64 side is the one-step replica of
# tests/rnn_replay.py chained over the steps with NO rounding (`h_mat` = h); the kernels round the state to bf16 as the matrix operand
# and W_hh once (`seen`).
#
# The bound, written out (all in units of u = 2^-24, first order).  E_h(s) is the bound of the state after step s, E_h(-1) = 0.
#   forward, step s: the matrix operand is bf16 of the kernel's state: d_mat = E_h(s-1) + BF |h|, so the pre-activations move by
#     d_a = d_mat |W_hh|^T; through the gates on absolute values (|sig'| = g (1 - g), |tanh'| = 1 - g^2):
#       GRU   e_r = r (1-r) d_a_r, e_z = z (1-z) d_a_z, e_n = (1 - n^2) (|gh_n| e_r + r d_a_n),
#             E_h(s) = gru_bound + |h - n| e_z + (1 - z) e_n + z E_h(s-1)                 (h' = (1 - z) n + z h)
#       LSTM  E_c(s) = bound_c + |c| f (1-f) d_a_f + f E_c(s-1) + |g| i (1-i) d_a_i + i (1 - g^2) d_a_g,
#             E_h(s) = bound_h + |tanh c'| o (1-o) d_a_o + o (1 - tanh^2 c') (E_c(s) - bound_c)
#     `gru_bound` / `lstm_bound` are the replica's own step models.  The SAVED gate values carry the same propagated terms plus the
#     gate bounds of tests/test_gpu_rnn.py ((H + 2) u on the pre-activations' absolute sums, / 4 through a sigmoid, + 9 u).
#   backward, step s (from the last): dh = dy + carry.  Every product of the header of csrc/rnn.hip is carried by the product rule on
#     absolute values with the errors of its factors (dh: the carry's; the gates': above; h_prev = y[s-1]: E_h(s-1); c: E_c), plus
#     the step's own arithmetic: 12 (GRU) / 32 (LSTM) u on test_gpu_rnn's conditioning.  dgx is then rounded to bf16 once (its
#     `ulps`); as the operand of the carry product and of dW_hh / db_hh, dgh carries that rounding as BF |dgh|:
#       carry = direct + bf16(dgh) bf16(W_hh): the operand's error through |W_hh| + (G Kp + 16 [32]) u on |direct| + |dgh| |W_hh|
#       dW_hh = sum over the B T rows of bf16(dgh)^T bf16(h_prev): operand errors (h_prev: E_h(s-1) + BF |h_prev|) + (B T + 8) u
#       db_hh = the column sum of bf16(dgh): operand errors + (B T + 8) u.


def _rnn_dirs(v):
    out = [(v["gx_f"], v["w_hh_f"], v["b_hh_f"], False)]
    if v.get("gx_r") is not None:
        out.append((v["gx_r"], v["w_hh_r"], v["b_hh_r"], True))
    return out


def _rnn_order(steps, reverse):
    return list(range(steps - 1, -1, -1)) if reverse else list(range(steps))


def _rnn_ref(v, lstm):
    ys = []
    for gx, w, b, reverse in _rnn_dirs(v):
        h = gx.new_zeros((gx.shape[0], w.shape[1]))
        c = h
        outs = [None] * gx.shape[1]
        for t in _rnn_order(gx.shape[1], reverse):
            if lstm:
                h, c, _ = RR.lstm_step(gx[:, t], h, c, w, b)
            else:
                h, _ = RR.gru_step(gx[:, t], h, w, b)
            outs[t] = h
        ys.append(torch.stack(outs, 1))
    return torch.cat(ys, -1)


def _rnn_obvious(v, lstm):
    """nn.GRU / nn.LSTM in float64 fed [gx_f, gx_r] through identity input weights and a zero input bias"""
    dirs = _rnn_dirs(v)
    gh, hd, nd = dirs[0][0].shape[-1], dirs[0][1].shape[1], len(dirs)
    net = (torch.nn.LSTM if lstm else torch.nn.GRU)(nd * gh, hd, batch_first=True, bidirectional=nd == 2).double()
    with torch.no_grad():
        for d, (_, w, b, _) in enumerate(dirs):
            sfx = "_reverse" if d else ""
            w_ih = torch.zeros(gh, nd * gh, dtype=F64)
            w_ih[:, d * gh:(d + 1) * gh] = torch.eye(gh, dtype=F64)
            getattr(net, "weight_ih_l0" + sfx).copy_(w_ih)
            getattr(net, "bias_ih_l0" + sfx).zero_()
            getattr(net, "weight_hh_l0" + sfx).copy_(w)
            getattr(net, "bias_hh_l0" + sfx).copy_(b)
    return net(torch.cat([d[0] for d in dirs], -1))[0]


def _rnn_units_dir(gx, w, b, dy, reverse, lstm):
    """(units of y, of dgx, of dW_hh, of db_hh) of one direction: the bound written out above"""
    bsz, steps, hd = gx.shape[0], gx.shape[1], w.shape[1]
    kp = (hd + 31) // 32 * 32
    wa = w.abs()
    zero = gx.new_zeros((bsz, hd))
    sl = lambda t, i: t[:, i * hd:(i + 1) * hd]  # noqa: E731
    h, c, e_h, e_c = zero, zero, zero, zero
    u_y = torch.zeros_like(dy)
    rec = []
    for t in _rnn_order(steps, reverse):
        g_in = gx[:, t]
        d_a = (e_h + BF * h.abs()) @ wa.t()
        pre = RR._pre_bound(g_in, h, w, b)
        if lstm:
            hn, cn, (i, f, g, o) = RR.lstm_step(g_in, h, c, w, b)
            b_h, b_c = RR.lstm_bound(g_in, c, w, b, h, (i, f, g, o))
            e_i = i * (1 - i) * sl(d_a, 0) + sl(pre, 0) / 4 + RR.SIG_U
            e_f = f * (1 - f) * sl(d_a, 1) + sl(pre, 1) / 4 + RR.SIG_U
            e_g = (1 - g * g) * sl(d_a, 2) + sl(pre, 2) + RR.TANH_U
            e_o = o * (1 - o) * sl(d_a, 3) + sl(pre, 3) / 4 + RR.SIG_U
            prop_c = c.abs() * f * (1 - f) * sl(d_a, 1) + f * e_c + g.abs() * i * (1 - i) * sl(d_a, 0) + i * (1 - g * g) * sl(d_a, 2)
            tc = torch.tanh(cn)
            e_cn = b_c + prop_c
            e_hn = b_h + tc.abs() * o * (1 - o) * sl(d_a, 3) + o * (1 - tc * tc) * prop_c
            rec.append(dict(t=t, h=h, c=c, cn=cn, e_h=e_h, e_c=e_c, e_cn=e_cn, gates=(i, f, g, o), eg=(e_i, e_f, e_g, e_o)))
            h, c, e_h, e_c = hn, cn, e_hn, e_cn
        else:
            hn, (r, z, n, ghn) = RR.gru_step(g_in, h, w, b)
            own = RR.gru_bound(g_in, h, w, b, h, (r, z, n, ghn))
            p_r, p_z, p_n = r * (1 - r) * sl(d_a, 0), z * (1 - z) * sl(d_a, 1), sl(d_a, 2)
            p_nn = (1 - n * n) * (ghn.abs() * p_r + r * p_n)
            # the saved gates: test_gpu_rnn's gate bounds and the propagated terms
            own_n = sl(pre, 2) + ghn.abs() * (sl(pre, 0) / 4 + RR.SIG_U) + sl(g_in, 2).abs() + (r * ghn).abs()
            e_r, e_z = p_r + sl(pre, 0) / 4 + RR.TANH_U, p_z + sl(pre, 1) / 4 + RR.TANH_U
            e_n, e_ghn = p_nn + own_n + RR.TANH_U, p_n + sl(pre, 2) + RR.TANH_U
            e_hn = own + (h - n).abs() * p_z + (1 - z) * p_nn + z * e_h
            rec.append(dict(t=t, h=h, e_h=e_h, gates=(r, z, n, ghn), eg=(e_r, e_z, e_n, e_ghn)))
            h, e_h = hn, e_hn
        u_y[:, t] = e_h
    # ---- backward, from the last step
    u_gx = torch.zeros_like(gx)
    u_w, s_w = torch.zeros_like(w), torch.zeros_like(w)
    u_b, s_b = torch.zeros_like(b), torch.zeros_like(b)
    carry, e_carry, dc, e_dc = zero, zero, zero, zero
    for st in reversed(rec):
        t, hp, e_hp = st["t"], st["h"], st["e_h"]
        dh = dy[:, t] + carry
        e_dh = e_carry + dy[:, t].abs() + carry.abs()
        a = dh.abs()
        if lstm:
            (i, f, g, o), (e_i, e_f, e_g, e_o) = st["gates"], st["eg"]
            cp, e_cp = st["c"], st["e_c"]
            tc = torch.tanh(st["cn"])
            e_tc = (1 - tc * tc) * st["e_cn"] + RR.TANH_U
            dcc = dc + dh * o * (1 - tc * tc)
            e_dcc = e_dc + e_dh * o * (1 - tc * tc) + a * e_o * (1 - tc * tc) + a * o * 2 * tc.abs() * e_tc
            q = dcc.abs()
            parts = [dcc * g * i * (1 - i), dcc * cp * f * (1 - f), dcc * i * (1 - g * g), dh * tc * o * (1 - o)]
            errs = [e_dcc * g.abs() * i * (1 - i) + q * (e_g * i * (1 - i) + g.abs() * e_i),
                    e_dcc * cp.abs() * f * (1 - f) + q * (e_cp * f * (1 - f) + cp.abs() * e_f),
                    e_dcc * i * (1 - g * g) + q * (e_i * (1 - g * g) + i * 2 * g.abs() * e_g),
                    e_dh * tc.abs() * o * (1 - o) + a * (e_tc * o * (1 - o) + tc.abs() * e_o)]
            base = dc.abs() + a
            own = 32 * base * (1 + cp.abs())
            dgx = torch.cat(parts, 1)
            e_dgx = torch.cat([e + own for e in errs], 1)
            dgh, e_dgh = dgx, e_dgx
            direct, e_direct = zero, zero
            e_dc = e_dcc * f + q * e_f + 32 * base
            dc = dcc * f
            chain = 4 * kp + 32
        else:
            (r, z, n, ghn), (e_r, e_z, e_n, e_ghn) = st["gates"], st["eg"]
            dn, dz = dh * (1 - z), dh * (hp - n)
            dnp, dzp = dn * (1 - n * n), dz * z * (1 - z)
            rr = r * (1 - r)
            drp = dnp * ghn * rr
            e_dn = e_dh * (1 - z) + a * e_z
            e_dz = e_dh * (hp - n).abs() + a * (e_hp + e_n)
            e_dnp = e_dn * (1 - n * n) + dn.abs() * 2 * n.abs() * e_n
            e_dzp = e_dz * z * (1 - z) + dz.abs() * e_z
            e_drp = e_dnp * (ghn * rr).abs() + dnp.abs() * (e_ghn * rr + ghn.abs() * e_r)
            own = 12 * a * (1 + hp.abs() + n.abs()) * (1 + ghn.abs())
            dgx = torch.cat([drp, dzp, dnp], 1)
            e_dgx = torch.cat([e_drp + own, e_dzp + own, e_dnp + own], 1)
            dgh = torch.cat([drp, dzp, dnp * r], 1)
            e_dgh = torch.cat([e_drp + own, e_dzp + own, e_dnp * r + dnp.abs() * e_r + own], 1)
            direct, e_direct = dh * z, e_dh * z + a * e_z
            chain = 3 * kp + 16
        e_mat = e_dgh + BF * dgh.abs()
        u_gx[:, t] = e_dgx
        u_w += e_mat.t() @ hp.abs() + dgh.abs().t() @ (e_hp + BF * hp.abs())
        s_w += dgh.abs().t() @ hp.abs()
        u_b += e_mat.sum(0)
        s_b += dgh.abs().sum(0)
        carry = direct + dgh @ w
        e_carry = e_direct + e_mat @ wa + chain * (direct.abs() + dgh.abs() @ wa)
    m = bsz * steps
    return u_y, u_gx, u_w + (m + 8) * s_w, u_b + (m + 8) * s_b


def _rnn_units(lstm):
    def model(c):
        hit = getattr(c, "_rnn_units", None)
        if hit is None:
            hit = {}
            ys = []
            for d, (gx, w, b, reverse) in enumerate(_rnn_dirs(c.v)):
                hd = w.shape[1]
                sfx = "_r" if d else "_f"
                u_y, hit["gx" + sfx], hit["w_hh" + sfx], hit["b_hh" + sfx] = _rnn_units_dir(
                    gx, w, b, c.dy[0][:, :, d * hd:(d + 1) * hd], reverse, lstm)
                ys.append(u_y)
            hit["y0"] = torch.cat(ys, -1)
            c._rnn_units = hit
        return hit
    return lambda key: (lambda c: model(c)[key])


def _rnn_cases():
    bsz, steps = 17, 3
    for cell, ndir, hd in (("GRU", 1, 40), ("GRU", 2, 8), ("LSTM", 1, 8), ("LSTM", 2, 40)):
        lstm = cell == "LSTM"
        gates = 4 if lstm else 3
        sfxs = ("_f", "_r")[:ndir]

        def make(gates=gates, hd=hd, sfxs=sfxs, seed=600 + 10 * gates + hd):
            d = {}
            for j, s in enumerate(sfxs):
                d["gx" + s] = R((bsz, steps, gates * hd), seed + 3 * j, 1.0)
                d["w_hh" + s] = R((gates * hd, hd), seed + 3 * j + 1, 0.6 / math.sqrt(hd))  # the layer's own initial deviation
                d["b_hh" + s] = R(gates * hd, seed + 3 * j + 2, 0.3)
            return d

        def call(t, cell=cell, sfxs=sfxs):
            args = [t[k + s] for s in sfxs for k in ("gx", "w_hh", "b_hh")]
            return HR.recurrence(HR.CELL_IDS[cell], *args)

        units = _rnn_units(lstm)
        names = tuple(k + s for s in sfxs for k in ("gx", "w_hh", "b_hh"))
        err = {"y0": Err(1, units("y0"), F32)}
        for s in sfxs:
            err["gx" + s] = Err(1, units("gx" + s), BF16)  # dgx leaves the kernel as bf16; autograd casts it to the f32 of gx
            err["w_hh" + s] = Err(1, units("w_hh" + s))
            err["b_hh" + s] = Err(1, units("b_hh" + s))
        case(name=f"rnn_{cell.lower()}_d{ndir}_h{hd}", fns=(HR.RecurrentFn,), family="rnn", dy_forms=(cell == "GRU" and ndir == 2),
             make=make, diff=names, params=tuple(n for n in names if not n.startswith("gx")), out=(F32,),
             seen={"w_hh" + s: BF16 for s in sfxs}, call=call, ref=lambda v, lstm=lstm: _rnn_ref(v, lstm),
             obvious=lambda v, lstm=lstm: _rnn_obvious(v, lstm), err=err)

    # InputProjFn: gx = x W_ih^T + b_ih with the f32 x as two bf16 words.  x of order 1e3 with fractional parts needs the second
    # word (one word would lose everything below 4 .. 8); F = 5 is the narrow GEMM, 15 rows are no multiple of 8.
    #   hi + lo = x to 2^-8 2^-8 |x| (two bf16 roundings, the second of the first's remainder): 2^8 u on ABS;
    #   y: two f32 chains of F products, the bias, the f32 store of the first GEMM and the add of the second: 2 F + 4;
    #   dX = bf16 dgx W_ih (depth G H + 1) leaves as bf16: autograd casts it to the f32 of x;
    #   dW_ih: two tn GEMMs over the M rows into ONE destination (each M + 8, one add between them) + the residue of x again;
    #   db_ih: the column sum of depth M.
    rows, f, gh = (3, 5), 5, 24
    m = 15
    case(name="rnn_input_proj", fns=(HR.InputProjFn,), family="rnn_input_proj", dy_forms=True, out=(F32,),
         make=lambda: {"x": R(rows + (f,), 640, 1.0e3), "w": R((gh, f), 641, 1.0 / math.sqrt(f)), "b": R(gh, 642, 0.3)},
         diff=("x", "w", "b"), params=("w", "b"), seen={"w": BF16}, call=lambda t: HR.InputProjFn.apply(t["x"], t["w"], t["b"]),
         ref=lambda v: v["x"] @ v["w"].t() + v["b"], obvious=lambda v: F.linear(v["x"], v["w"], v["b"]),
         err={"y0": Err(1, (2 * f + 4 + 2 ** 8, ABS), F32), "x": Err(1, (gh + 1, ABS), BF16),
              "w": Err(1, (2 * (m + 8) + 1 + 2 ** 8, ABS)), "b": Err(1, (m + 8, ABS))})


_rnn_cases()


# =============================================================================================
# nbm: the per-basis MLPs, the featurizer and the f32 head
# =============================================================================================


def _nbm_mats(v, order):
    """the conv-shaped parameters as the matrices of nbm_replay: w1 [NB, H, o], b1 [NB, H], w2 [NB, H, H], b2, w3 [NB, H], b3 [NB]"""
    nb = v["b3"].numel()
    h = v["b1"].numel() // nb
    return (v["w1"].reshape(nb, h, order), v["b1"].reshape(nb, h), v["w2"].reshape(nb, h, h), v["b2"].reshape(nb, h),
            v["w3"].reshape(nb, h), v["b3"].reshape(nb))


def _nbm_pre(v):
    idx = v["idx"]
    w1, b1, w2, b2, w3, b3 = _nbm_mats(v, len(idx[0]))
    u = v["x"][:, torch.as_tensor(idx, dtype=torch.long)]                      # [B, D, o]
    pre1 = torch.einsum("bdo,gko->bdgk", u, w1) + b1
    pre2 = torch.einsum("bdgk,gjk->bdgj", pre1.clamp_min(0), w2) + b2
    return pre1, pre2, w3, b3


def _nbm_ref(v):
    pre1, pre2, w3, b3 = _nbm_pre(v)
    return torch.einsum("bdgj,gj->bdg", pre2.clamp_min(0), w3) + b3


def _nbm_obvious(v):
    """basis by basis: Linear(o, H), ReLU, Linear(H, H), ReLU, Linear(H, 1) on the gathered tuples"""
    idx = v["idx"]
    w1, b1, w2, b2, w3, b3 = _nbm_mats(v, len(idx[0]))
    u = v["x"][:, torch.as_tensor(idx, dtype=torch.long)]
    outs = []
    for g in range(b3.numel()):
        hid = F.relu(F.linear(F.relu(F.linear(u, w1[g], b1[g])), w2[g], b2[g]))
        outs.append(F.linear(hid, w3[g:g + 1], b3[g:g + 1]))
    return torch.cat(outs, -1)


def _nbm_units():
    """The replica of tests/nbm_replay.py runs the kernels' operation order WITH their bf16 roundings (h1 as two words, dpre2 as the
    MFMA operand; W2's is `seen`) and bounds the f32 arithmetic around ITS values, zero-band mask flips of layer 2 included: no element
    is left out.  The reference here is plain, so each bound is the replica's plus the float64 distance between the replica and the
    reference: what those roundings do to this case's values, computed on the CPU.  The operands are nbm_weights.kernel_case's dyadic
    ones, for which pre1 and dbases w3 are exact in f32 (dy is bf16-valued, w3 a 7-bit code: 15 bits)."""
    def model(c):
        hit = getattr(c, "_nbm_units", None)
        if hit is None:
            v = c.v
            idx = v["idx"]
            w1, b1, w2, b2, w3, b3 = _nbm_mats(v, len(idx[0]))
            rp = NR.Replay(dict(x=v["x"], idx=idx, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3))
            got, bd = rp.backward(c.dy[0])
            hit = {"y0": rp.bases_bound() + (rp.bases - c.y[0].reshape(rp.bases.shape)).abs() / NR.U}
            for name, key in (("x", "dx"), ("w1", "dw1"), ("b1", "db1"), ("w2", "dw2"), ("b2", "db2"), ("w3", "dw3"), ("b3", "db3")):
                ref = c.g[name]
                hit[name] = (bd[key].reshape(ref.shape) + (got[key].reshape(ref.shape) - ref).abs() / NR.U)
            hit["y0"] = hit["y0"].reshape(c.y[0].shape)
            c._nbm_units = hit
        return hit
    return lambda key: (lambda c: model(c)[key])


# (seeds: the first from 21 on for which no pre-activation of the reference is exactly zero; the host test asserts it)
NBM_CASES = {"nbm_bases_o1": (40, 3, 17, 3, [(0,), (1,), (2,)], 31), "nbm_bases_o2_repeat": (40, 3, 17, 4, NW.REPEAT, 22)}


def _nbm_make(h, nb, b, f, idx, seed):
    def make():
        k = NW.kernel_case(h, nb, b, f, idx, seed)
        o = len(idx[0])
        return {"x": k["x"], "idx": [tuple(t) for t in idx], "w1": k["w1"].reshape(nb * h, o, 1), "b1": k["b1"].reshape(nb * h),
                "w2": k["w2"].reshape(nb * h, h, 1), "b2": k["b2"].reshape(nb * h), "w3": k["w3"].reshape(nb, h, 1), "b3": k["b3"].reshape(nb)}
    return make


def nbm_relu_margin(name):
    """the smallest |pre-activation| of a bases case: the host test asserts that no hidden unit of the reference sits ON its kink
    (the dyadic operands could produce an exact zero, where gradcheck's difference quotient and the mask disagree)"""
    c = CASES[name]
    pre1, pre2, _, _ = _nbm_pre(values64(c, c.make(), grad=False))
    return float(torch.minimum(pre1.abs().min(), pre2.abs().min()))


def _nbm_cases():
    units = _nbm_units()
    pnames = ("w1", "b1", "w2", "b2", "w3", "b3")
    for name, (h, nb, b, f, idx, seed) in NBM_CASES.items():
        def call(t, idx=idx, f=f):
            table = ops.nbm_index(t["idx"], len(idx[0]), f, t["x"].device)
            return HN.BasesFn.apply(t["x"], table, *(t[k] for k in pnames))

        err = {"y0": Err(1, units("y0"), F32), "x": Err(1, units("x"), F32)}
        err.update({k: Err(1, units(k)) for k in pnames})
        case(name=name, fns=(HN.BasesFn,), family="nbm_bases", dy_forms=name.endswith("repeat"), make=_nbm_make(h, nb, b, f, idx, seed),
             diff=("x",) + pnames, params=pnames, seen={"w2": BF16}, out=(F32,), call=call, ref=_nbm_ref, obvious=_nbm_obvious, err=err)

    # FeaturizeFn: feat[b, d] = sum_g bases[b, d, g] w[d, g] + bias[d]: one fma chain over the NB bases and the bias (NB + 1);
    # dbases = dfeat w: one product; dw / dbias: sums over the B samples in a fixed order of at most B + 64 additions (nbm_replay)
    b, d, nb = 17, 5, 3
    case(name="nbm_featurize", fns=(HN.FeaturizeFn,), family="nbm_featurize", dy_forms=True, out=(F32,),
         make=lambda: {"bases": R((b, d, nb), 650), "w": R((d, nb, 1), 651, 0.6), "b": R(d, 652, 0.3)},
         diff=("bases", "w", "b"), params=("w", "b"), call=lambda t: HN.featurize(t["bases"], t["w"], t["b"]),
         ref=lambda v: torch.einsum("bdg,dg->bd", v["bases"], v["w"].reshape(d, nb)) + v["b"],
         obvious=lambda v: F.conv1d(v["bases"].reshape(b, d * nb, 1), v["w"], v["b"], groups=d)[:, :, 0],
         err={"y0": Err(1, (nb + 1, ABS), F32), "bases": Err(1, ("self", 1), F32), "w": Err(1, (b + 64, ABS)), "b": Err(1, (b + 64, ABS))})
    # HeadFn: f32 end to end (test_head_fn_per_element's counts): y an fma chain of latent + 1 terms (the bias column), dX of `out`
    # terms, dW of B terms, db the column sum (B + 8)
    lat, out = 5, 3
    case(name="nbm_head", fns=(HN.HeadFn,), family="nbm_head", dy_forms=True, out=(F32,),
         make=lambda: {"feat": R((b, lat), 655), "w": R((out, lat), 656, 0.5), "b": R(out, 657, 0.3)},
         diff=("feat", "w", "b"), params=("w", "b"), call=lambda t: HN.head(t["feat"], t["w"], t["b"]),
         ref=lambda v: v["feat"] @ v["w"].t() + v["b"], obvious=lambda v: F.linear(v["feat"], v["w"], v["b"]),
         err={"y0": Err(1, (lat + 2, ABS), F32), "feat": Err(1, (out + 1, ABS), F32), "w": Err(1, (b + 1, ABS)), "b": Err(1, (b + 8, ABS))})


_nbm_cases()


# =============================================================================================
# pixelcnn: the masked 7x7 convolution on the live taps
# =============================================================================================


def _masked_conv_cases():
    """(B, H, W) = (2, 5, 7), (Cin, Cout) = (64, 32): the smallest entries of test_gpu_pixelcnn's CHANNELS with Cin != Cout; the map is
    narrower than the halo on both sides.  test_gpu_pixelcnn's models: y and dX are one f32 chain of T Ci (T Co) exact products and
    the bias, rounded to bf16 once; dW the tn GEMM's f32 sum over the B H W = 70 rows (one row chunk: + 1, + 1); db a column sum.
    The reference reads the live taps only, so its gradient of a masked tap is exactly zero, and so must the device's be: `ulps` is
    0 there and the ABS units vanish with the reference."""
    b, cin, cout, h, w = 2, 64, 32, 5, 7
    m = b * h * w

    def add(name, mask_type, bias, nhwc=False, dy_forms=False):
        taps = ops.MASKED_TAPS[mask_type]
        live = PR.mask_of(mask_type).expand(cout, cin, 7, 7)

        def make():
            d = {"x": R((b, cin, h, w), 660 + taps, 1.0, BF16), "w": R((cout, cin, 7, 7), 662 + taps, 2.0 / math.sqrt(25 * cin))}
            if bias:
                d["b"] = R(cout, 664 + taps, 0.3)
            return d

        def ref(v):
            y = PR.masked_conv64(v["x"], v["w"], mask_type)[0]
            return y if v.get("b") is None else y + v["b"].view(1, -1, 1, 1)

        err = {"y0": Err(1, (taps * cin + 2, ABS)), "x": Err(1, (taps * cout + 1, ABS)), "w": Err(lambda c: live.clone(), (m + 2, ABS))}
        if bias:
            err["b"] = Err(1, (m + 8, ABS))
        case(name=name, fns=(HP.MaskedConv2dFn,), family="masked_conv", dy_forms=dy_forms, make=make,
             diff=("x", "w", "b") if bias else ("x", "w"), params=("w", "b") if bias else ("w",), seen={"w": BF16}, nhwc=nhwc,
             nhwc_in=("x",) if nhwc else (), call=lambda t: HP.masked_conv2d(t["x"], t["w"], t.get("b"), taps), ref=ref,
             obvious=lambda v: F.conv2d(v["x"], v["w"] * PR.mask_of(mask_type), v.get("b"), padding=3), err=err, fast_gradcheck=True)

    add("masked_conv_a", "A", True, dy_forms=True)
    add("masked_conv_b_no_bias", "B", False)
    add("masked_conv_b_nhwc", "B", True, nhwc=True)


_masked_conv_cases()


# =============================================================================================
# rwkv: the time mix with its projections, the WKV scan with the output layer, relu^2 with the value layer, the gate
# =============================================================================================
_WU = WR.U


def _time_mix_cases():
    """(B, T, C) = (3, 5, 72): C is no multiple of 64, N_j != C.  rows_j = bf16(x m_j + shift(x) (1 - m_j)) (rwkv_replay.time_mix:
    3 u on the two products' magnitudes and the bf16 rounding), out_j = rows_j bf16(W_j)^T in f32: the rows' bound through |W_j| and
    a chain of C + 1.  Backward: d_j arrives bf16-valued; ds_j = d_j W_j in f32 (chain N_j + 1) enters the time-mix backward
    (rwkv_replay.time_mix_backward, exact inputs) and carries its own error through it: |m|, |1 - m| on the next row for dx,
    |x - shift(x)| summed over the rows for dm.  dW_j = d_j^T rows_j over the M = 15 rows (M + 8) with the rows' bound."""
    bsz, steps, ch = 3, 5, 72
    m = bsz * steps

    def add(name, three, x_dtype, dy_forms=False):
        js = ("k", "v", "r") if three else ("k", "r")
        width = {"k": 40, "v": 48, "r": 56}

        def make():
            d = {"x": R((bsz, steps, ch), 670, 1.0, x_dtype)}
            for i, j in enumerate(("k", "v", "r")):
                on = j in js
                d["m" + j] = torch.rand((1, 1, ch), generator=_g(671 + i), dtype=F64).to(F32) if on else None
                d["w" + j] = R((width[j], ch), 675 + i, 1.0 / math.sqrt(ch)) if on else None
            return d

        mixes = lambda v: [v["m" + j].reshape(-1) for j in js]  # noqa: E731

        def ref(v):
            return tuple(WR.mixed(v["x"], v["m" + j]) @ v["w" + j].t() for j in js)

        def obvious(v):
            xs = F.pad(v["x"], (0, 0, 1, -1))  # nn.ZeroPad2d((0, 0, 1, -1)): the reference's time shift
            return tuple(F.linear(torch.lerp(xs, v["x"], v["m" + j]), v["w" + j]) for j in js)

        def model(c):
            hit = getattr(c, "_tm", None)
            if hit is None:
                v = c.v
                vals, bnds = WR.time_mix(v["x"], mixes(v))
                ds, e_ds, hit = [], [], {}
                for i, j in enumerate(js):
                    wa, dya = v["w" + j].abs(), c.dy[i].abs().reshape(m, -1)
                    hit[f"y{i}"] = (bnds[i] / _WU) @ wa.t() + (ch + 2) * (vals[i].abs() @ wa.t())
                    hit["w" + j] = dya.t() @ (bnds[i].reshape(m, ch) / _WU) + (m + 8) * (dya.t() @ vals[i].abs().reshape(m, ch))
                    ds.append(c.dy[i] @ v["w" + j])
                    e_ds.append((width[j] + 1) * (c.dy[i].abs() @ wa))
                bw = WR.time_mix_backward(ds, v["x"], mixes(v), x_dtype == BF16)
                diff = (v["x"] - WR.shift(v["x"])).abs()
                u_x = bw["dx_bound"] / _WU
                for i, j in enumerate(js):
                    mj = v["m" + j].reshape(-1)
                    nxt = torch.cat([e_ds[i][:, 1:], torch.zeros_like(e_ds[i][:, :1])], 1)
                    u_x = u_x + e_ds[i] * mj.abs() + nxt * (1 - mj).abs()
                    hit["m" + j] = (bw["dm_bound"][i] / _WU + (e_ds[i] * diff).sum((0, 1))).reshape(1, 1, ch)
                hit["x"] = u_x
                c._tm = hit
            return hit

        u = lambda key: (lambda c: model(c)[key])  # noqa: E731
        names = ("x",) + tuple("m" + j for j in js) + tuple("w" + j for j in js)
        err = {f"y{i}": Err(1, u(f"y{i}"), F32) for i in range(len(js))}
        # (dx_bound and dm_bound hold their own output rounding; one more ulp stands for the f32 -> x.dtype hand-over)
        err["x"] = Err(1, u("x"), x_dtype)
        err.update({k: Err(1, u(k)) for k in names[1:]})
        case(name=name, fns=(HW.TimeMixFn,), family="rwkv_time_mix", dy_forms=dy_forms, make=make, diff=names, params=names[1:],
             seen={"w" + j: BF16 for j in js}, out=(F32,) * len(js),
             call=lambda t: HW.time_mix(t["x"], t["mk"], t["mv"], t["mr"], t["wk"], t["wv"], t["wr"]), ref=ref, obvious=obvious, err=err)

    add("rwkv_time_mix_kvr_bf16", True, BF16, dy_forms=True)
    add("rwkv_time_mix_kvr_f32", True, F32)
    add("rwkv_time_mix_kr_bf16", False, BF16)
    add("rwkv_time_mix_kr_f32", False, F32)


_time_mix_cases()


def _wkv_explicit(k, v, r, decay):
    """the explicit causal sums: wk[t] = sum_{s <= t} lam^(t-s) exp(k[s]), wkv[t] = sum_{s <= t} lam^(t-s) exp(k[s]) v[s] / (wk[s] + 1e-6)"""
    lam = torch.exp(-torch.exp(decay.reshape(-1)))
    steps = k.shape[1]
    t = torch.arange(steps, dtype=F64)
    gap = t[:, None] - t[None, :]
    kern = torch.where((gap >= 0)[:, :, None], lam[None, None, :] ** gap.clamp_min(0)[:, :, None], torch.zeros((), dtype=F64))  # [t, s, L]
    e = torch.exp(k)
    wk = torch.einsum("tsl,bsl->btl", kern, e)
    wkv = torch.einsum("tsl,bsl->btl", kern, e * v / (wk + WR.EPS))
    return torch.sigmoid(r) * wkv


def _wkv_abs_backward(e_dy, fw):
    """the scan's backward is linear in dy: a bound e_dy of dy reaches dk, dv, dr and d_decay through the same recurrences on
    absolute values (the magnitudes of rwkv_replay.wkv_backward)"""
    lam, ew, e, v, a, n, sig = fw["lam"], fw["ew"], fw["e"], fw["v"], fw["a"], fw["n"], fw["sig"]
    q = 1.0 / (a + WR.EPS)
    big_g = WR.scan(e_dy * sig, lam, True)
    big_h = WR.scan(big_g * n.abs() * q, lam, True)
    prev = lambda t: torch.cat([torch.zeros_like(t[:, :1]), t[:, :-1]], 1)  # noqa: E731
    dlam = (big_g * prev(fw["b_abs"]) + big_h * prev(a)).sum((0, 1))
    return dict(dk=(big_g * v.abs() * q + big_h) * e, dv=big_g * e * q, dr=e_dy * fw["b_abs"] * sig * (1 - sig), d_decay=dlam * lam * ew)


def _wkv_cases():
    """(B, T, L) = (3, 11, 40): csrc/rwkv.hip cuts time into chunks of CFHIP_RWKV_CHUNK = 8 steps at fixed positions, so T = 11
    crosses one chunk boundary (the carry between chunks runs); L = 40 leaves a wave's lanes ragged.  The float64 side is
    rwkv_replay.Wkv (the recurrence with its hand-written adjoints, which gradcheck holds to account), `obvious` the explicit sums.
    Bare: y = bf16 of the scan: rwkv_replay's y_bound (its own bf16 rounding inside, so `ulps` = 0), dk / dv / dr / d_decay its
    backward bounds.  With `w_out`: out = bf16(y) bf16(W)^T (+ residual), a chain of L + 2 behind y's bound through |W|; the scan's
    dy = d W in f32 (chain N + 1) is no longer exact: its error runs through the scan's backward on absolute values
    (`_wkv_abs_backward`); dW_out = d^T bf16(y) over the M = 33 rows.  The residual's gradient is d itself, handed back as it came:
    exact in either dtype (`ulps` = 0, no units)."""
    bsz, steps, lat, n_out = 3, 11, 40, 56
    m = bsz * steps

    def add(name, with_out, res_dtype, dy_forms=False):
        def make():
            d = {"k": R((bsz, steps, lat), 680, 0.7), "v": R((bsz, steps, lat), 681), "r": R((bsz, steps, lat), 682),
                 "decay": R((lat, 1), 683, 0.5), "w_out": R((n_out, lat), 684, 1.0 / math.sqrt(lat)) if with_out else None,
                 "res": R((bsz, steps, n_out), 685, 1.0, res_dtype) if res_dtype is not None else None}
            return d

        def tail(y, v):
            if v.get("w_out") is not None:
                y = y @ v["w_out"].t()
            return y if v.get("res") is None else y + v["res"]

        # an f32 residual makes the output f32 and its dy f32-valued (`dy_f32`): the GEMMs read d2 = bf16(d), one bf16 rounding of d
        # (BF on |d|) in front of dy = d2 W and dW_out = d2^T y, while the residual's own gradient must come back unrounded
        bf_dy = BF if res_dtype == F32 else 0.0

        def model(c):
            hit = getattr(c, "_wkv", None)
            if hit is None:
                v = c.v
                fw = WR.wkv_forward(v["k"], v["v"], v["r"], v["decay"])
                dy, e_dy, hit = c.dy[0], torch.zeros_like(fw["y"]), {}
                if with_out:
                    wa = v["w_out"].abs()
                    res = v["res"].abs() if res_dtype is not None else 0.0
                    hit["y0"] = (fw["y_bound"] / _WU) @ wa.t() + (lat + 3) * (fw["y"].abs() @ wa.t() + res)
                    dya = dy.abs().reshape(m, n_out)
                    hit["w_out"] = dya.t() @ (fw["y_bound"].reshape(m, lat) / _WU) + (m + 8) * (dya.t() @ fw["y"].abs().reshape(m, lat))
                    e_dy = (n_out + 1 + bf_dy) * (dy.abs() @ wa)
                    hit["w_out"] = hit["w_out"] + bf_dy * (dya.t() @ fw["y"].abs().reshape(m, lat))
                    dy = dy @ v["w_out"]
                else:
                    hit["y0"] = fw["y_bound"] / _WU
                bw = WR.wkv_backward(dy, fw)
                carried = _wkv_abs_backward(e_dy * (1 + WR.HALF_BF16), fw)
                for key, name_ in (("k", "dk"), ("v", "dv"), ("r", "dr")):
                    hit[key] = bw[name_ + "_bound"] / _WU + carried[name_]
                hit["decay"] = (bw["d_decay_bound"] / _WU + carried["d_decay"]).reshape(lat, 1)
                c._wkv = hit
            return hit

        u = lambda key: (lambda c: model(c)[key])  # noqa: E731
        names = ("k", "v", "r", "decay") + (("w_out",) if with_out else ()) + (("res",) if res_dtype is not None else ())
        out_dtype = res_dtype if res_dtype is not None else BF16
        err = {"y0": Err(1 if with_out else 0, u("y0"), out_dtype), "decay": Err(0, u("decay"))}
        err.update({key: Err(0, u(key), BF16) for key in ("k", "v", "r")})  # (the bounds hold the bf16 rounding of dk, dv, dr)
        if with_out:
            err["w_out"] = Err(1, u("w_out"))
        if res_dtype is not None:
            err["res"] = Err(0, None, res_dtype)
        case(name=name, fns=(HW.WkvFn,), family="rwkv_wkv", dy_forms=dy_forms, make=make, diff=names,
             params=("decay",) + (("w_out",) if with_out else ()), seen={"w_out": BF16} if with_out else {}, out=(out_dtype,),
             call=lambda t: HW.wkv(t["k"], t["v"], t["r"], t["decay"], t["w_out"], t["res"]),
             ref=lambda v: tail(WR.Wkv.apply(v["k"], v["v"], v["r"], v["decay"]), v),
             obvious=lambda v: tail(_wkv_explicit(v["k"], v["v"], v["r"], v["decay"]), v), err=err, dy_f32=res_dtype == F32)

    add("rwkv_wkv_bare", False, None)
    add("rwkv_wkv_out", True, None)
    add("rwkv_wkv_out_res_bf16", True, BF16, dy_forms=True)
    add("rwkv_wkv_out_res_f32", True, F32)


_wkv_cases()


def _rwkv_small_cases():
    bsz, steps, hid, ch = 3, 5, 40, 72
    m = bsz * steps
    # relu(h)^2 from the exact f32 h (the mask needs no band): one product and the bf16 rounding; dh = bf16(2 relu(h) d): the
    # doubling is exact, one product.  With `w_value`: out = kk bf16(W)^T in f32 behind kk's rounding (BF + 1 on |kk|) and a chain
    # of HID + 1; the d reaching relu^2's backward is d W in f32 (chain C + 1); dW = d^T kk over M = 15 rows.
    relu2 = lambda v: v["h"].clamp_min(0) ** 2  # noqa: E731
    case(name="rwkv_squared_relu", fns=(HW.SquaredReluFn,), family="rwkv_relu2", dy_forms=True,
         make=lambda: {"h": R((bsz, steps, hid), 690)}, diff=("h",), call=lambda t: HW.squared_relu(t["h"]), ref=relu2,
         obvious=lambda v: torch.square(F.relu(v["h"])), err={"y0": Err(1, ("self", 1)), "h": Err(1, ("self", 1), BF16)})

    def value_units(key):
        def units(c):
            v = c.v
            kk, wa, dya = relu2(v).abs(), v["w"].abs(), c.dy[0].abs()
            if key == "y0":
                return (BF + 1 + hid + 1) * (kk @ wa.t())
            if key == "w":
                return (BF + 1 + m + 8) * (dya.reshape(m, ch).t() @ kk.reshape(m, hid))
            return 2 * v["h"].clamp_min(0) * (ch + 2) * (dya @ wa)
        return units

    case(name="rwkv_squared_relu_value", fns=(HW.SquaredReluFn,), family="rwkv_relu2", out=(F32,),
         make=lambda: {"h": R((bsz, steps, hid), 691), "w": R((ch, hid), 692, 1.0 / math.sqrt(hid))}, diff=("h", "w"), params=("w",),
         seen={"w": BF16}, call=lambda t: HW.squared_relu(t["h"], t["w"]), ref=lambda v: relu2(v) @ v["w"].t(),
         obvious=lambda v: F.linear(torch.square(F.relu(v["h"])), v["w"]),
         err={"y0": Err(1, value_units("y0"), F32), "h": Err(1, value_units("h"), BF16), "w": Err(1, value_units("w"))})

    # the gate: s = 1 / (1 + expf(-r)) (4 u, rwkv_replay), s kv one product, the residual one add; dr = d kv (s (x s)), x = expf(-r):
    # 1 - sigmoid = expf(-r) sigmoid at 7 u, three more products; dkv = d s.  The residual's gradient is d as it came.
    gate_ref = lambda v: torch.sigmoid(v["r"]) * v["kv"] + (v["res"] if v.get("res") is not None else 0.0)  # noqa: E731

    def gate_units(key):
        def units(c):
            s = torch.sigmoid(c.v["r"])
            if key == "y0":
                return 6 * (s * c.v["kv"]).abs() + (c.v["res"].abs() if c.v.get("res") is not None else 0.0)
            if key == "r":
                return 16 * (c.dy[0] * c.v["kv"]).abs() * s * (1 - s)
            return 6 * c.dy[0].abs() * s
        return units

    for tag, res_dtype in (("plain", None), ("res_bf16", BF16), ("res_f32", F32)):
        def make(res_dtype=res_dtype):
            return {"r": R((bsz, steps, ch), 693), "kv": R((bsz, steps, ch), 694),
                    "res": R((bsz, steps, ch), 695, 1.0, res_dtype) if res_dtype is not None else None}

        out_dtype = res_dtype if res_dtype is not None else BF16
        err = {"y0": Err(1, gate_units("y0"), out_dtype), "r": Err(1, gate_units("r"), BF16), "kv": Err(1, gate_units("kv"), BF16)}
        if res_dtype is not None:
            err["res"] = Err(0, None, res_dtype)
        case(name=f"rwkv_gate_{tag}", fns=(HW.GateFn,), family="rwkv_gate", dy_forms=(tag == "res_bf16"), make=make,
             diff=("r", "kv") + (("res",) if res_dtype is not None else ()), out=(out_dtype,),
             call=lambda t: HW.gate(t["r"], t["kv"], t["res"]), ref=gate_ref,
             obvious=lambda v: (lambda y: y if v.get("res") is None else torch.add(v["res"], y))(torch.mul(1.0 / (1.0 + torch.exp(-v["r"])), v["kv"])),
             err=err, dy_f32=res_dtype == F32)  # (the gate's backward reads the f32 d as it is: the same products, no rounding of d)


_rwkv_small_cases()


# =============================================================================================
# siren: the stand-alone sine, the modulator's f32 ReLU and the fused coordinate MLP
# =============================================================================================


def _siren_cases():
    sh = (5, 24)
    # sin(w x): the product w x rounds once (u |w x| on the argument), the library's sine 2 ulp at 1 (4 u): siren_replay / test_sine_per_element;
    # dx = dy w cos(w x): the same on the cosine through |dy w|, and two products
    for w in (30.0, 1.0):
        case(name=f"siren_sine_w{int(w)}", fns=(HS.SineFn,), family="siren_sine", dy_forms=(w == 30.0), out=(F32,),
             make=lambda: {"x": R(sh, 700, 1.0)}, diff=("x",), call=lambda t, w=w: HS.Sine(w=w)(t["x"]),
             ref=lambda v, w=w: torch.sin(w * v["x"]), obvious=lambda v, w=w: torch.sin(torch.mul(v["x"], w)),
             err={"y0": Err(1, lambda c, w=w: (w * c.v["x"]).abs() + 4, F32),
                  "x": Err(1, lambda c, w=w: (c.dy[0] * w).abs() * ((w * c.v["x"]).abs() + 4) + 2 * c.g["x"].abs(), F32)})
    # the f32 ReLU: copies and zeros; the mask comes from the exact f32 input (the saved output), so no band is needed
    case(name="siren_relu_f32", fns=(HS.ReluF32Fn,), family="siren_relu", dy_forms=True, out=(F32,), make=lambda: {"x": R(sh, 701, 1.0)},
         diff=("x",), call=lambda t: HS.ReluF32Fn.apply(t["x"]), ref=lambda v: v["x"].clamp_min(0), obvious=lambda v: F.relu(v["x"]),
         err={"y0": Err(0, None, F32), "x": Err(0, None, F32)})

    # SirenFn: layers = 2, latent = 32, (B, N) = (3, 25): M = 75 rows are no multiple of the kernel's row tile and straddle the
    # samples (test_gpu_siren's ROWS).  The replica of tests/siren_replay.py runs the kernel's operation order with its bf16 words
    # (h, sin, cos, dpre, the packed hidden and head weights) and bounds the f32 arithmetic around ITS values, `flip` terms for a
    # re-rounded word included.  The reference here is the plain layer loop, so each bound is the replica's plus the float64
    # distance between the replica and the reference: what those roundings do to this case's values, computed on the CPU.
    # No weight is `seen` in bf16: the head weight enters the forward as its bf16 pack, but the backward's dh = dy Wh reads the f32
    # parameter (as the replica does).  A first version of this case rounded `wh` on both sides through `seen` and missed dmods, dx
    # and the layer gradients behind dh by that one rounding of Wh (2^-9 relative) on an MI355X; the kernel is as documented.
    b, n, lat, din, dout, layers = 3, 25, 32, 2, 3, 2

    def add(name, shared, bias, dy_forms=False):
        def make():
            hb = math.sqrt(6.0 / lat)
            uni = lambda shape, seed, bound: ((torch.rand(shape, generator=_g(seed), dtype=F64) * 2 - 1) * bound).to(F32)  # noqa: E731
            d = {"x": uni((n, din) if shared else (b, n, din), 710, 1.0), "mods": R((layers, b, lat), 711),
                 "w0": uni((lat, din), 712, 1.0 / din), "w1": uni((lat, lat), 713, hb), "wh": uni((dout, lat), 714, hb)}
            if bias:
                d.update(b0=uni((lat,), 715, 1.0 / din), b1=uni((lat,), 716, hb), bh=uni((dout,), 717, hb))
            return d

        pnames = ("w0", "w1", "wh") + (("b0", "b1", "bh") if bias else ())

        def call(t):
            shape = ops.SirenShape(b, n, din, lat, dout, layers, 30.0, 1.0)
            params = [t[k] for k in pnames]
            save = torch.is_grad_enabled() and any(p.requires_grad for p in (t["x"], t["mods"], *params))
            return HS.SirenFn.apply(shape, shared, bias, save, t["x"], t["mods"], *params)

        def rows(v):
            return v["x"].unsqueeze(0).expand(b, n, din) if shared else v["x"]

        def ref(v):
            net = rows(v)
            for l, w in enumerate((30.0, 1.0)):
                pre = torch.einsum("bni,oi->bno", net, v[f"w{l}"]) + (v[f"b{l}"] if bias else 0.0)
                net = torch.sin(w * pre) * v["mods"][l][:, None, :]
            return torch.einsum("bni,oi->bno", net, v["wh"]) + (v["bh"] if bias else 0.0)

        def obvious(v):  # the reference's loop: net = block(net); net = net * mod
            net = rows(v)
            for l, w in enumerate((30.0, 1.0)):
                net = torch.sin(w * F.linear(net, v[f"w{l}"], v[f"b{l}"] if bias else None))
                net = net * v["mods"][l].unsqueeze(1)
            return F.linear(net, v["wh"], v["bh"] if bias else None)

        def model(c):
            hit = getattr(c, "_siren", None)
            if hit is None:
                v = c.v
                np64 = lambda t: t.detach().numpy()  # noqa: E731
                rep = SR.Replica([np64(v["w0"]), np64(v["w1"])], np64(v["wh"]), [np64(v[k]) for k in ("b0", "b1", "bh")] if bias else None,
                                 30.0, 1.0)
                y, ey = rep.forward(np64(rows(v).reshape(b * n, din)), np.repeat(np.arange(b), n), np64(v["mods"]))
                back = rep.backward(np64(c.dy[0].reshape(b * n, dout)))
                both = lambda val, bound, ref_: (torch.from_numpy(bound) + (torch.from_numpy(val) - ref_.reshape(val.shape)).abs()).reshape(ref_.shape) / SR.U  # noqa: E731
                hit = {"y0": both(y, ey, c.y[0]), "mods": both(*back["dmods"], c.g["mods"])}
                if not shared:
                    hit["x"] = both(*back["dx"], c.g["x"])
                for k in pnames:
                    hit[k] = both(*back[k], c.g[k])
                c._siren = hit
            return hit

        u = lambda key: (lambda c: model(c)[key])  # noqa: E731
        names = (() if shared else ("x",)) + ("mods",) + pnames  # (the shared grid is a buffer: the Function returns no gradient for it)
        err = {"y0": Err(1, u("y0"), F32), "mods": Err(1, u("mods"), F32)}
        if not shared:
            err["x"] = Err(1, u("x"), F32)
        err.update({k: Err(1, u(k)) for k in pnames})
        case(name=name, fns=(HS.SirenFn,), family="siren", dy_forms=dy_forms, make=make, diff=names, params=pnames, out=(F32,),
             call=call, ref=ref, obvious=obvious, err=err)

    add("siren_grid_bias", True, True, dy_forms=True)
    add("siren_init_no_bias", False, False)


_siren_cases()


# =============================================================================================
# Wrappers: LayerNorm -> Linear(GELU) -> Linear(residual) plain, as one taped node, and checkpointed: bit-equal gradients
# =============================================================================================

WRAP = dict(rows=(2, 5), d=24, hid=40, eps=1e-5)
WRAP_PARAMS = ("ln_w", "ln_b", "w1", "b1", "w2", "b2")


def wrap_make():
    d, hid = WRAP["d"], WRAP["hid"]
    return {"x": R(WRAP["rows"] + (d,), 900, 1.0, BF16), "ln_w": 1.0 + R(d, 901, 0.2), "ln_b": R(d, 902, 0.2), "w1": R((hid, d), 903, 0.2),
            "b1": R(hid, 904, 0.2), "w2": R((d, hid), 905, 0.2), "b2": R(d, 906, 0.2)}


def wrap_chain(x, ln_w, ln_b, w1, b1, w2, b2):
    with HF.fanin_links():  # (the taped node folds x's two gradients inside the LayerNorm backward kernel; so does the link)
        h = HF.layer_norm(x, ln_w, ln_b, WRAP["eps"])
        h = HF.linear(h, w1, b1, act=HF.ACT_GELU)
        return HF.linear(h, w2, b2, residual=x)


def wrap_call(kind: str, t: Dict[str, Any]) -> Any:
    args = [t["x"]] + [t[n] for n in WRAP_PARAMS]
    if kind == "plain":
        return wrap_chain(*args)
    if kind == "taped":
        return HF.run_taped(lambda: wrap_chain(*args), tuple(args))
    if kind == "checkpoint":
        return HF.gradient_checkpoint(lambda x: wrap_chain(x, *args[1:]), (t["x"],), args[1:], True)
    raise ValueError(kind)


def wrap_ref(v):
    h = _ln_ref(v["x"], v["ln_w"], v["ln_b"], WRAP["eps"])
    h = gelu64(h @ v["w1"].t() + v["b1"])
    return h @ v["w2"].t() + v["b2"] + v["x"]


# the three forms launch the same kernels on the same operands: their results are compared with each other, bit for bit (the value
# checks of the chain's links are the cases above)
WRAPPER_FNS = (HF.TapedFn, HF._CheckpointFn)


def covered_functions():
    out = set(WRAPPER_FNS)
    for c in CASES.values():
        out.update(c.fns)
    return out


# =============================================================================================
# The float64 side of a case: values, outputs, gradients and the error bounds (shared by the host and the GPU tests)
# =============================================================================================


class Ctx:
    """what an error model's `units` callable sees"""

    def __init__(self, v, y, dy, g):
        self.v, self.y, self.dy, self.g = v, y, dy, g


def as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def values64(c: Case, vals: Dict[str, Any], grad: bool = True) -> Dict[str, Any]:
    """the values the kernels see, as float64 leaves (integer inputs pass through)"""
    out = {}
    for k, t in vals.items():
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            t = t.to(c.seen.get(k, t.dtype)).double().detach().clone()
            if grad and k in c.diff:
                t.requires_grad_(True)
        out[k] = t
    return out


def make_dys(c: Case, ys: Sequence[torch.Tensor], seed: int):
    """one bf16-representable output gradient per differentiable output (every dy form then carries the same values); with `dy_f32`
    the values need the whole f32 mantissa, so that a rounding of dy to bf16 on its way back shows"""
    dt = F32 if c.dy_f32 else BF16
    return [None if i in c.nondiff_out else R(tuple(y.shape), seed + 17 * i, 1.0, dt).double() for i, y in enumerate(ys)]


def grads64(c: Case, vals: Dict[str, Any], dys) -> Tuple[tuple, Dict[str, torch.Tensor]]:
    v = values64(c, vals)
    ys = as_tuple(c.ref(v))
    loss = sum((y * d.reshape(y.shape)).sum() for y, d in zip(ys, dys) if d is not None)
    wrt = [k for k in c.diff]
    gs = torch.autograd.grad(loss, [v[k] for k in wrt], allow_unused=True) if wrt else ()
    return tuple(y.detach() for y in ys), {k: (torch.zeros_like(v[k]) if g is None else g) for k, g in zip(wrt, gs)}


def _abs_pass(c: Case, vals: Dict[str, Any], dys):
    """the reference on absolute values: for a sum of products the exact first-order condition of outputs and gradients"""
    v = values64(c, vals)
    va = {k: (t.detach().abs().requires_grad_(k in c.diff) if isinstance(t, torch.Tensor) and t.is_floating_point() else t) for k, t in v.items()}
    ys = as_tuple(c.ref(va))
    loss = sum((y * d.abs().reshape(y.shape)).sum() for y, d in zip(ys, dys) if d is not None)
    wrt = [k for k in c.diff]
    gs = torch.autograd.grad(loss, [va[k] for k in wrt], allow_unused=True) if wrt else ()
    out = {f"y{i}": y.detach() for i, y in enumerate(ys)}
    out.update({k: (torch.zeros_like(va[k]) if g is None else g) for k, g in zip(wrt, gs)})
    return out


def err_dtype(c: Case, key: str) -> torch.dtype:
    e = c.err[key]
    if e.dtype is not None:
        return e.dtype
    if key.startswith("y") and key[1:].isdigit():
        return c.out[int(key[1:])]
    return F32 if key in c.params else BF16


def bounds(c: Case, vals: Dict[str, Any], dys, ys, gs) -> Dict[str, Tuple[float, Optional[torch.Tensor], torch.dtype]]:
    """{key: (ulps, units tensor or None, dtype)} for every output and gradient of the case"""
    v = {k: (t.detach() if isinstance(t, torch.Tensor) else t) for k, t in values64(c, vals, grad=False).items()}
    ctx = Ctx(v, ys, dys, gs)
    ab = None
    out = {}
    for key, e in c.err.items():
        ref = ys[int(key[1:])] if key.startswith("y") and key[1:].isdigit() else gs[key]
        u = e.units
        if u is None:
            units = None
        elif isinstance(u, tuple) and u[1] == ABS:
            ab = ab if ab is not None else _abs_pass(c, vals, dys)
            units = u[0] * ab[key]
        elif isinstance(u, tuple) and u[0] == "self":
            units = u[1] * ref.abs()
        elif callable(u):
            units = u(ctx)
        else:
            raise TypeError(f"{c.name}: error model of {key}: {u!r}")
        out[key] = (e.ulps(ctx) if callable(e.ulps) else e.ulps, units, err_dtype(c, key))
    return out
