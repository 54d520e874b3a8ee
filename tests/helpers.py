"""Shared comparison helpers for the parity tests."""
import math

import torch


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def max_abs(a: torch.Tensor, b: torch.Tensor) -> float:
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item()


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


def assert_close(a, b, rel, what="", abs_floor=0.0):
    err = rel_l2(a, b)
    if err > rel and max_abs(a, b) > abs_floor:
        raise AssertionError(f"{what}: rel-L2 {err:.3e} > {rel:.1e} (max-abs {max_abs(a, b):.3e})")
    return err


# ---------------------------------------------------------------------------------------------
# Per-element comparison against a float64 reference
# ---------------------------------------------------------------------------------------------

_MANT_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23, torch.float64: 52}
_MIN_NORMAL_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126, torch.float64: -1022}
F32_EPS_HALF = 2.0 ** -24  # unit roundoff of one f32 operation


def ulp_out(ref_abs: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` at |ref| (float64), floored at the spacing of the smallest normal: 2^(e - 7) for bf16,
    2^(e - 23) for f32, where 2^e <= |ref| < 2^(e + 1)."""
    mant, emin = _MANT_BITS[dtype], _MIN_NORMAL_EXP[dtype]
    a = ref_abs.double().clamp_min(2.0 ** emin)
    a = torch.where(torch.isfinite(a), a, torch.full_like(a, 2.0 ** emin))
    _, e = torch.frexp(a)  # a = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), (e - 1 - mant).to(torch.int32))


def assert_elementwise(got, ref64, *, out_dtype, ulps=1.0, cond=None, k=0.0, what=""):
    """Every element: |got - ref| <= ulps * ulp_out(|ref|) + k * 2^-24 * cond, with NaN and +-Inf at the same positions.

    `ref64` is a float64 reference computed from the same (bf16-rounded) inputs the kernel saw; `cond` is the same
    computation on absolute values (|A| @ |B|, sum |x|, ...), which bounds the rounding error of an f32 evaluation:
    `k` is the number of f32 roundings the error model allows along the longest dependent chain."""
    g = got.detach().cpu().double().reshape(-1)
    r = torch.as_tensor(ref64).detach().cpu().double().expand(got.shape).reshape(-1)
    if g.numel() != r.numel():
        raise AssertionError(f"{what}: {g.numel()} elements, reference has {r.numel()}")
    bound = ulps * ulp_out(r.abs(), out_dtype)
    if cond is not None and k:
        c = torch.as_tensor(cond).detach().cpu().double().expand(got.shape).reshape(-1)
        bound = bound + k * F32_EPS_HALF * c
    r_nan, g_nan = torch.isnan(r), torch.isnan(g)
    r_inf, g_inf = torch.isinf(r), torch.isinf(g)
    special_bad = (r_nan != g_nan) | (r_inf != g_inf) | (r_inf & g_inf & (r != g))
    finite = ~(r_nan | r_inf) & ~(g_nan | g_inf)
    err = torch.zeros_like(r)
    err[finite] = (g[finite] - r[finite]).abs()
    bad = special_bad | (finite & (err > bound))
    nbad = int(bad.sum())
    if nbad:
        idx = torch.nonzero(bad).view(-1)[:8].tolist()
        lines = [f"  [{i}] got {g[i].item():.9g} ref {r[i].item():.9g} |err| {abs(g[i].item() - r[i].item()):.3g} "
                 f"bound {bound[i].item():.3g}" for i in idx]
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements out of bound (ulps={ulps}, k={k}); first flat indices:\n"
                             + "\n".join(lines))


# ---------------------------------------------------------------------------------------------
# float64 references shared by the GEMM epilogue tests and the element-wise kernel tests
# ---------------------------------------------------------------------------------------------


def _gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _sig64(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _gemm_ref(a, b, a_trans, b_trans):
    """float64 A @ B of bf16 operands in the layout of ops.gemm -> (want, cond): cond is the product of the absolute values"""
    A = a.double().t() if a_trans else a.double()
    B = b.double() if b_trans else b.double().t()
    return A @ B, A.abs() @ B.abs()


# ---------------------------------------------------------------------------------------------
# float64 3x3 convolution on NHWC rows (the reference of the implicit-GEMM convolution tests)
# ---------------------------------------------------------------------------------------------


def conv3x3_rows_ref(x, w, bias):
    """float64 3x3 / stride 1 / padding 1 convolution of x [B, Cin, H, W] with w [Cout, Cin, 3, 3] (bf16-valued) and an f32
    bias or None, as NHWC rows [B H W, Cout] -> (want, cond): cond is the same convolution on absolute values."""
    conv = torch.nn.functional.conv2d
    x64, w64 = x.double(), w.double()
    b64 = None if bias is None else bias.double()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, w.shape[0])  # noqa: E731
    return rows(conv(x64, w64, b64, padding=1)), rows(conv(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), padding=1))


def assert_conv3x3_rows(y_rows, ref, cin, what=""):
    """bf16 rows [B H W, Cout] of a 3x3 convolution against `ref` = conv3x3_rows_ref(...), every element: an f32 sum of
    9 Cin exact products (bf16 x bf16 fits f32) and the bias — 9 Cin additions in any order — rounded once to bf16."""
    want, cond = ref
    assert tuple(y_rows.shape) == tuple(want.shape), f"{what}: shape {tuple(y_rows.shape)}, expected {tuple(want.shape)}"
    assert_elementwise(y_rows, want, out_dtype=torch.bfloat16, ulps=1, cond=cond, k=9 * cin + 1, what=what)


# ---------------------------------------------------------------------------------------------
# float64 softmax attention (the reference of the attention kernel tests)
# ---------------------------------------------------------------------------------------------


def attn_ref(q, k, v, heads, dh, mask=None, causal=False, scale=None, drop=None):
    """float64 attention on bf16 operands q [B, Tq, H dh], k / v [B, Tk, H dh] -> Q, K, V ([B, H, T, dh]), P and lse (for
    the backward and the cond terms).  `mask`: a bool keep mask broadcastable to [B, H, Tq, Tk]; `causal` masks j > i
    (also when Tq != Tk); `scale` defaults to 1 / sqrt(dh).  A row without a kept key has P = 0 and lse = -inf.
    `drop` = (keep [B, H, Tq, Tk] bool, p_eff): a sixth value, the dropped probabilities P * keep / (1 - p_eff)."""
    bsz, tq, _ = q.shape
    tk = k.shape[1]
    sh = lambda t, n: t.double().view(bsz, n, heads, dh).transpose(1, 2)  # noqa: E731
    Q, K, V = sh(q, tq), sh(k, tk), sh(v, tk)
    s = Q @ K.transpose(-1, -2) * (1.0 / math.sqrt(dh) if scale is None else scale)
    keep = torch.ones(tq, tk, dtype=torch.bool)
    if causal:
        keep = torch.tril(keep)
    if mask is not None:
        keep = keep & mask
    s = s.masked_fill(~keep, -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    p = torch.where(torch.isinf(lse)[..., None], torch.zeros_like(p), p)
    if drop is None:
        return Q, K, V, p, lse
    dkeep, p_eff = drop
    return Q, K, V, p, lse, p * dkeep.double() / (1.0 - p_eff)


def attn_mask(kind, bsz, heads, tq, tk):
    """bool keep masks.  rand: [Tq, Tk] (ms_b = ms_h = 0); pad: [B, 1, 1, Tk] key padding (ms_h = ms_q = 0); full:
    [B, H, Tq, Tk], different per head; prefix: every third row loses keys 0 .. 255 (whole first chunks) and keeps the
    later ones; band: every third row loses the whole last 128-key chunk; dead: `rand` with rows 1 and Tq - 2 empty."""
    g = torch.Generator().manual_seed(1000 * tq + tk)
    if kind in ("rand", "dead"):
        m = torch.rand((tq, tk), generator=g) > 0.3
        m[:, 0] = True  # every row keeps one slot
        if kind == "dead":
            m[1 % tq] = False
            m[max(tq - 2, 0)] = False
        return m
    if kind == "pad":
        m = torch.ones((bsz, 1, 1, tk), dtype=torch.bool)
        for b in range(bsz):
            m[b, 0, 0, max(1, tk - 1 - (b + 1) * max(1, tk // 5)):] = False  # a different padded tail per sample
        return m
    if kind == "full":
        m = torch.rand((bsz, heads, tq, tk), generator=g) > 0.3
        m[..., 0] = True
        return m
    if kind == "prefix":
        assert tk > 256
        m = torch.ones((tq, tk), dtype=torch.bool)
        m[::3, :256] = False
        return m
    if kind == "band":
        assert tk > 128
        m = torch.ones((tq, tk), dtype=torch.bool)
        m[1::3, (tk - 1) // 128 * 128:] = False
        return m
    raise ValueError(kind)


def attn_k_product(dh, tk, drop=False):
    """units of 2^-24 on cond for O and dV (twice that for dQ / dK): the error model of the attention kernel tests"""
    k = 2 ** 16 + 2 * dh + 64  # P / dS rounded to bf16 before their products; f32 scores of depth dh; exp2 / rcp / log
    k += 4 * -(-tk // 64)      # online softmax: one exp2 and one product rounding on O and on l per 64-key block
    if drop:
        k += 2                 # the f32 product with 1 / (1 - p)
    return k


def attn_k_lse(dh, tk, sumcol=False):
    """units of 2^-24 on cond (>= 1) for lse = max + log(row sum)"""
    k = 2 * dh + 64 + 4 * -(-tk // 64)  # scores, intrinsics, the rescales of the row sum
    k += tk // 4 + 8                    # the row sum: an f32 chain of Tk / 4 additions per lane and the cross-lane fold
    if sumcol:
        k += 2 ** 16                    # row sum out of the PV MFMA's ones column: a sum of the bf16-rounded p, 2^-8 on lse
    return k


def assert_attn_forward(o, lse_got, ref, scale, *, drop=False, sumcol=False, tag=""):
    """O [B, Tq, H dh] and lse [B, H, Tq] against `ref` = attn_ref(...)'s tuple, per element.  A row without a kept key
    (reference lse = -inf) has 1 / l with l = 0 in the kernels: its own O and lse are unspecified and left out."""
    Q, K, V, p, lse = ref[:5]
    pd = ref[5] if len(ref) > 5 else p
    bsz, heads, tq, dh = Q.shape
    tk = K.shape[2]
    back = lambda z: z.transpose(1, 2).reshape(bsz, tq, heads * dh)  # noqa: E731
    alive = torch.isfinite(lse)
    alive_o = back(alive[..., None].expand(bsz, heads, tq, dh))
    want_o = back(pd @ V)
    got_o = torch.where(alive_o, o.detach().cpu().double(), want_o)
    assert_elementwise(got_o, want_o, out_dtype=torch.bfloat16, cond=back(pd @ V.abs()), k=attn_k_product(dh, tk, drop), what=f"{tag} O")
    # lse = max + log(sum exp): its error is that of the scores (cond = the absolute-value scores) and the log
    sabs = (Q.abs() @ K.abs().transpose(-1, -2)) * scale
    want_lse = torch.where(alive, lse, torch.zeros_like(lse))
    lse_cond = (p * sabs).sum(-1) + want_lse.abs() + 1
    got_lse = torch.where(alive, lse_got.detach().cpu().double(), want_lse)
    assert_elementwise(got_lse, want_lse, out_dtype=torch.float32, ulps=4, cond=lse_cond, k=attn_k_lse(dh, tk, sumcol), what=f"{tag} lse")


def assert_attn_backward(dq, dk, dv, ref, do, scale, *, drop=None, tag=""):
    """dQ (or None), dK, dV [B, T, H dh] against the float64 backward of `ref` = attn_ref(...)'s tuple for the output
    gradient `do` [B, Tq, H dh]; `drop` = (keep, p_eff) as given to attn_ref.  dV = Pd^T dO and dS = P (dP - delta) are
    rounded to bf16 before their products (the 2^16 term of attn_k_product), delta is taken from the bf16 O; cond = the
    same products on absolute values.  dQ and dK chain two such roundings (dS, then its product): twice the units.
    The dQ of a row without a kept key is unspecified and left out; dK and dV are checked in full."""
    Q, K, V, p, lse = ref[:5]
    pd = ref[5] if len(ref) > 5 else p
    bsz, heads, tq, dh = Q.shape
    tk = K.shape[2]
    back = lambda z: z.transpose(1, 2).reshape(bsz, -1, heads * dh)  # noqa: E731
    dO = do.double().view(bsz, tq, heads, dh).transpose(1, 2)
    kp = attn_k_product(dh, tk, drop is not None)
    O = pd @ V
    dP = dO @ V.transpose(-1, -2)
    cdP = dO.abs() @ V.abs().transpose(-1, -2)
    if drop is not None:
        f = drop[0].double() / (1.0 - drop[1])
        dP, cdP = dP * f, cdP * f
    dS = p * (dP - (dO * O).sum(-1, keepdim=True))
    cdS = p * (cdP + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    bf16 = torch.bfloat16
    assert_elementwise(dv, back(pd.transpose(-1, -2) @ dO), out_dtype=bf16, cond=back(pd.transpose(-1, -2) @ dO.abs()), k=kp,
                       what=f"{tag} dV")
    assert_elementwise(dk, back(dS.transpose(-1, -2) @ Q * scale), out_dtype=bf16, cond=back(cdS.transpose(-1, -2) @ Q.abs() * scale),
                       k=2 * kp, what=f"{tag} dK")
    if dq is not None:
        want_dq = back(dS @ K * scale)
        alive_o = back(torch.isfinite(lse)[..., None].expand(bsz, heads, tq, dh))
        got_dq = torch.where(alive_o, dq.detach().cpu().double(), want_dq)
        assert_elementwise(got_dq, want_dq, out_dtype=bf16, cond=back(cdS @ K.abs() * scale), k=2 * kp, what=f"{tag} dQ")


# ---------------------------------------------------------------------------------------------
# Guarded allocations: overruns, unwritten outputs and reads past an input
# ---------------------------------------------------------------------------------------------

GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
ALIGN = 256
_INT_OF_SIZE = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _site() -> str:
    import traceback

    for fr in reversed(traceback.extract_stack()[:-2]):
        if not fr.filename.endswith("helpers.py"):
            return f"{fr.filename.rsplit('/', 1)[-1]}:{fr.lineno} {fr.name}"
    return "?"


class _Guarded:
    """One buffer: [guard >= 4 KB][interior, 256-byte aligned][guard >= 4 KB].  Bytes outside `view` must keep
    the content they had when the buffer was made."""

    def __init__(self, buf, start, view, label):
        self.buf, self.start, self.view, self.label = buf, start, view, label
        mark = torch.zeros(buf.numel(), dtype=torch.uint8)
        isz = view.element_size()
        as_int = mark.view(_INT_OF_SIZE[isz])
        off = (view.data_ptr() - buf.data_ptr()) // isz
        if view.numel():
            as_int.as_strided(view.shape, view.stride(), off).fill_(-1)
        self.keep = mark == 0
        self.expect = buf.detach().cpu().clone()

    def clobbered(self):
        now = self.buf.detach().cpu()
        diff = torch.nonzero(self.keep & (now != self.expect)).view(-1)
        if diff.numel() == 0:
            return None
        first = int(diff[0])
        return int(diff.numel()), first - self.start, int(now[first]), int(self.expect[first])


def _raw_buffer(nbytes: int, device, fill_byte: int):
    """uint8 buffer with >= GUARD_BYTES on each side of an ALIGN-aligned interior of `nbytes` -> (buf, start)."""
    body = (nbytes + ALIGN - 1) // ALIGN * ALIGN
    buf = torch.full((GUARD_BYTES + ALIGN + body + GUARD_BYTES,), fill_byte, dtype=torch.uint8, device=device)
    start = GUARD_BYTES + (-(buf.data_ptr() + GUARD_BYTES)) % ALIGN
    assert (buf.data_ptr() + start) % ALIGN == 0
    return buf, start


def _interior(buf, start, shape, dtype):
    nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    t = buf[start:start + nbytes].view(dtype).view(shape)
    assert t.data_ptr() % ALIGN == 0, "guarded interior lost its 256-byte alignment"
    return t


def _fill_like_nan(t):
    if t.is_floating_point():
        t.fill_(float("nan"))
    return t


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = size[0]
    return tuple(int(s) for s in size)


class GuardedOps:
    """Replaces `ops.torch` with a proxy whose empty / empty_like / zeros return views into guarded buffers:
    floating `empty` interiors start as NaN (an element a kernel skips cannot inherit a right value from the
    caching allocator), `zeros` interiors as 0, and every byte around them as GUARD_BYTE.  `check()` finds any
    guard byte a kernel changed.  Also the home of guarded inputs (`poisoned`, `index`) and `out=` views (`out2d`)."""

    def __init__(self, monkeypatch=None):
        self.allocs = []
        if monkeypatch is not None:
            from cflearn_amd import ops

            monkeypatch.setattr(ops, "torch", _TorchProxy(self))

    # -- allocation -------------------------------------------------------------------------------
    def _new(self, shape, dtype, device, fill):
        dtype = dtype or torch.get_default_dtype()
        shape = tuple(shape)
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        buf, start = _raw_buffer(nbytes, device, GUARD_BYTE)
        t = _interior(buf, start, shape, dtype)
        if fill == "nan":
            _fill_like_nan(t)
        elif fill == "zero":
            t.zero_()
        self.allocs.append(_Guarded(buf, start, t, f"{tuple(shape)} {dtype} from {_site()}"))
        return t

    def empty(self, *size, dtype=None, device=None):
        return self._new(_shape_of(size), dtype, device, "nan")

    def zeros(self, *size, dtype=None, device=None):
        return self._new(_shape_of(size), dtype, device, "zero")

    def empty_like(self, x, *, dtype=None, device=None):
        return self._new(tuple(x.shape), dtype or x.dtype, device or x.device, "nan")

    # -- inputs -----------------------------------------------------------------------------------
    def poisoned(self, t):
        """Contiguous copy of a floating input inside a NaN-filled buffer (guards included): a read past either
        end that reaches a result shows as NaN.  The NaN guards are checked for writes too."""
        assert t.is_floating_point(), "poison only floating inputs; use index() for integer ones"
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        buf, start = _raw_buffer(nbytes, t.device, 0)
        total = buf.numel() // t.element_size() * t.element_size()
        buf[:total].view(t.dtype).fill_(float("nan"))
        v = _interior(buf, start, tuple(t.shape), t.dtype)
        v.copy_(t)
        self.allocs.append(_Guarded(buf, start, v, f"input {tuple(t.shape)} {t.dtype} from {_site()}"))
        return v

    def index(self, t):
        """Integer input (indices, labels, timesteps) in a guarded buffer whose guards hold 0, a valid index:
        a read past the end can never become an out-of-range address."""
        assert not t.is_floating_point()
        t = t.contiguous()
        buf, start = _raw_buffer(t.numel() * t.element_size(), t.device, 0)
        v = _interior(buf, start, tuple(t.shape), t.dtype)
        v.copy_(t)
        self.allocs.append(_Guarded(buf, start, v, f"index {tuple(t.shape)} {t.dtype} from {_site()}"))
        return v

    def out2d(self, m, n, ld, dtype, device, *, fill=float("nan"), pad=float("-7.25"), guard_rows=2):
        """[m, n] output view with leading dimension ld > n: padding columns hold `pad`, `guard_rows` rows of
        `pad` above and below, all inside a byte-guarded buffer; the view itself starts as `fill`."""
        assert ld >= n
        rows = m + 2 * guard_rows
        isz = torch.empty((), dtype=dtype).element_size()
        buf, start = _raw_buffer(rows * ld * isz, device, GUARD_BYTE)
        whole = _interior(buf, start, (rows, ld), dtype)
        whole.fill_(pad)
        v = whole[guard_rows:guard_rows + m, :n]
        v.fill_(fill)
        self.allocs.append(_Guarded(buf, start, v, f"out2d {m}x{n} ld {ld} {dtype} from {_site()}"))
        return v

    def region(self, shape, dtype, device, views, *, pad=float("-7.25")):
        """One guarded buffer of `shape` filled with `pad`, in which only the sub-views `views(whole)` returns may
        change (e.g. several problems' C blocks with sentinel gaps between them)."""
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        buf, start = _raw_buffer(nbytes, device, GUARD_BYTE)
        whole = _interior(buf, start, tuple(shape), dtype)
        whole.fill_(pad)
        parts = views(whole)
        mark = _Guarded(buf, start, whole, f"region {tuple(shape)} {dtype} from {_site()}")
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for p in parts:
            g = _Guarded(buf, start, p, "")
            keep &= g.keep
        mark.keep = keep
        self.allocs.append(mark)
        return parts

    # -- verification -----------------------------------------------------------------------------
    def check(self):
        if any(a.buf.is_cuda for a in self.allocs):
            torch.cuda.synchronize()
        msgs = []
        for a in self.allocs:
            c = a.clobbered()
            if c is not None:
                n, off, now, was = c
                msgs.append(f"{a.label}: {n} guard byte(s) changed, first at byte offset {off} from the interior start "
                            f"(0x{now:02x}, was 0x{was:02x})")
        self.allocs.clear()
        if msgs:
            raise AssertionError("guard check failed:\n  " + "\n  ".join(msgs))


class _TorchProxy:
    """`torch` for ops.py: everything passes through except the three allocators GuardedOps replaces."""

    def __init__(self, g):
        self._g = g

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None):
        return self._g.empty(*size, dtype=dtype, device=device)

    def empty_like(self, x, *, dtype=None, device=None):
        return self._g.empty_like(x, dtype=dtype, device=device)

    def zeros(self, *size, dtype=None, device=None):
        return self._g.zeros(*size, dtype=dtype, device=device)


def guarded_ops(monkeypatch) -> GuardedOps:
    """GuardedOps patched into `cflearn_amd.ops` for the rest of the test (monkeypatch restores `ops.torch`)."""
    return GuardedOps(monkeypatch)


def poisoned(t, g: GuardedOps = None):
    """Module-level form of GuardedOps.poisoned (without a GuardedOps the guards are not checked for writes)."""
    return (g or GuardedOps()).poisoned(t)
