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
