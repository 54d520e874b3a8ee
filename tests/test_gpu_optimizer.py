"""The fused Adam / AdamW step (csrc/elementwise.hip: adam_kernel, adam_dev_kernel) and `optim.FusedAdam` around it, per
element against the float64 reference of adam_ref.py.

Conventions as in test_gpu_kernel_edges.py: buffers come from `guarded_ops` (inputs inside NaN, outputs between byte guards, all
checked for overruns at the end), tolerances are `ulps = 1` plus `k * 2^-24 * cond` with the rounding counts K_P / K_M / K_V
derived at the top of adam_ref.py, and the bf16 shadow is compared bit for bit with torch's round-to-nearest-even cast of the
parameters the kernel returned.  Sizes go past one pass of the grid-stride loop (2048 blocks x 256 threads x 4 elements = 2^21):
the arenas the optimizer really runs on are almost entirely beyond it.  Every comparison prints `ratio`, its largest
error / bound, before it asserts."""
import functools

import pytest
import torch

import adam_ref as A
from helpers import assert_elementwise, guarded_ops, ulp_out

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402
from cflearn_amd.optim import (FusedAdam, FusedAdamOptimizer, FusedAdamWOptimizer, ParamArena, _HYPER_RING,  # noqa: E402
                               clip_grad_norm_)

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PASS = 1 << 21  # elements one pass of the capped grid covers
SMALL_N = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025]
LARGE_N = [PASS - 1, PASS, PASS + 1, PASS + 1024 + 3, 2 * PASS + 5 * 1024 + 3]
BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)]
# (betas, eps, grad_scale, with shadow): every beta pair with both eps, every grad_scale twice, no shadow twice
SCALAR_MIX = [(BETAS[0], 1e-8, 1.0, True), (BETAS[1], 1e-3, 0.5, True), (BETAS[2], 1e-8, 1.0 / 3.0, False),
              (BETAS[0], 1e-3, 1.0 / 3.0, True), (BETAS[1], 1e-8, 1.0, False), (BETAS[2], 1e-3, 0.5, True)]
# the two scalar sets of the large sizes, one per decay form: (decoupled, wd, step, betas, eps, grad_scale)
LARGE_SETS = [(1, 0.05, 2, BETAS[0], 1e-8, 0.5), (0, 0.05, 1000, BETAS[1], 1e-3, 1.0 / 3.0)]
LR = 1e-2


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def _step_dev(p, g, m, v, p16, n, hyper, decoupled, off=0):
    """cfhip_adam_step_dev on elements [off, off + n) of the buffers -> return code (no check)"""
    return _lib.load().cfhip_adam_step_dev(_ptr(p, off), _ptr(g, off), _ptr(m, off), _ptr(v, off), _ptr(p16, off), n,
                                           hyper.data_ptr(), int(decoupled), _stream())


def _step_capi(p, g, m, v, p16, n, h, decoupled, step):
    """cfhip_adam_step with the float arguments of the record `h` -> return code (no check)"""
    return _lib.load().cfhip_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), n, h.lr, h.beta1, h.beta2, h.eps, h.wd,
                                       int(decoupled), int(step), h.gscale, _stream())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(got, want_cond, k, what):
    """assert_elementwise(ulps = 1, k) after printing the largest error / bound"""
    want, cond = want_cond
    g64 = got.detach().cpu().double().reshape(-1)
    bound = ulp_out(want.abs(), F32) + k * 2.0 ** -24 * cond
    ratio = ((g64 - want).abs() / bound).nan_to_num(nan=float("inf")).max().item() if g64.numel() else 0.0
    print(f"ratio {what}: {ratio:.3f} (k = {k})")
    assert_elementwise(got, want, out_dtype=F32, ulps=1, cond=cond, k=k, what=what)


def _check_step(got_p, got_m, got_v, got_p16, state, h, decoupled, tag):
    """p', m', v' of one launch against the float64 reference on the state it started from; the shadow against the cast of p'"""
    ref_p, ref_m, ref_v = A.adam_ref(*(t.double() for t in state), h, decoupled)
    _check(got_p, ref_p, A.K_P, f"{tag} p")  # 15 roundings reach p' (table in adam_ref.py)
    _check(got_m, ref_m, A.K_M, f"{tag} m")  # 5 roundings reach m'
    _check(got_v, ref_v, A.K_V, f"{tag} v")  # 8 roundings reach v'
    if got_p16 is not None:
        assert torch.equal(got_p16.cpu(), got_p.cpu().to(BF16)), f"{tag}: bf16 shadow is not the RNE cast of p'"


@functools.lru_cache(maxsize=2)
def _state(n, seed=0):
    return A.mixed_state(n, 1000 * seed + n % 997)


def _launch_both(G, state, h, betas, decoupled, step, shadow):
    """the same state through ops.adam_step (with the unrounded `betas` that `h` = hyper_capi(...) was made from) and through
    cfhip_adam_step_dev (with the record `h`) -> two (p, m, v, p16) tuples; g must stay as it was"""
    n = state[0].numel()
    outs = []
    for entry in ("capi", "dev"):
        p, g, m, v = (G.poisoned(t.to(DEV)) for t in state)
        p16 = G.empty((n,), dtype=BF16, device=DEV) if shadow else None
        if entry == "capi":
            ops.adam_step(p, g, m, v, p16, lr=h.lr, beta1=betas[0], beta2=betas[1], eps=h.eps, weight_decay=h.wd,
                          decoupled=bool(decoupled), step=step, grad_scale=h.gscale)
        else:
            _lib.check(_step_dev(p, g, m, v, p16, n, G.poisoned(h.tensor().to(DEV)), decoupled), "adam_step_dev")
        assert _same_bits(g, state[1]), f"{entry}: the gradient buffer changed"
        outs.append((p, m, v, p16))
    return outs


def _assert_entries_equal(a, b, tag):
    for name, x, y in zip(("p", "m", "v", "p16"), a, b):
        assert (x is None and y is None) or _same_bits(x, y), f"{tag}: {name} differs between cfhip_adam_step and cfhip_adam_step_dev"


# ---------------------------------------------------------------------------------------------
# the kernels per element
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("decoupled,wd", [(0, 0.0), (0, 0.05), (1, 0.0), (1, 0.05)])
def test_small_sizes_every_scalar(G, decoupled, wd, step):
    """n around the 4-wide body / scalar tail and one block; both decay forms with and without decay (wd == 0 skips the branch),
    bias corrections from step 1 to where they are 1, three beta pairs (beta1 = 0: bc1 = 1), two eps, three grad_scale, shadow
    present and absent.  The five regimes of `mixed_state` share every vector."""
    for n in SMALL_N:
        state = _state(n)
        zero = torch.arange(n) % 5 == 2  # g = m = v = 0
        for betas, eps, gscale, shadow in SCALAR_MIX:
            h = A.hyper_capi(LR, betas[0], betas[1], eps, wd, step, gscale)
            tag = f"n={n} dec={decoupled} wd={wd} t={step} betas={betas} eps={eps} gs={gscale:.3g}"
            capi, dev = _launch_both(G, state, h, betas, decoupled, step, shadow)
            _check_step(*capi, state, h, decoupled, tag)
            _assert_entries_equal(capi, dev, tag)
            p, m, v, _ = (None if t is None else t.cpu() for t in capi)
            if wd == 0.0 or decoupled:  # nothing reaches the moments of an element without gradient or state: 0 / eps, not NaN
                assert not m[zero].any() and not v[zero].any(), tag
            if wd == 0.0:
                assert _same_bits(p[zero], state[0][zero]), f"{tag}: p moved without gradient, state or decay"
        G.check()


@pytest.mark.parametrize("decoupled,wd,step,betas,eps,gscale", LARGE_SETS)
@pytest.mark.parametrize("n", LARGE_N)
def test_sizes_past_one_grid_pass(G, n, decoupled, wd, step, betas, eps, gscale):
    """2^21 - 1 ... 2^21 + 1027 and a third trip: every element of the `i += stride` trips and of the tail behind them"""
    state = _state(n)
    h = A.hyper_capi(LR, betas[0], betas[1], eps, wd, step, gscale)
    tag = f"n={n} dec={decoupled} t={step}"
    capi, dev = _launch_both(G, state, h, betas, decoupled, step, True)
    _check_step(*capi, state, h, decoupled, tag)
    _assert_entries_equal(capi, dev, tag)


def _tie_patterns():
    """f32 values around bf16 rounding: exact ties (low half 0x8000) over an odd and an even kept mantissa, one f32 ulp below and
    above a tie, a tie that carries into the exponent, the smallest normal's binade; both signs; -0.0, 0.0, +-largest finite bf16"""
    bits = []
    for lo in (0x8000, 0x7FFF, 0x8001):
        for hi in (0x3F81, 0x3F80, 0x4049, 0x4048, 0x3FFF, 0x0080):
            for sign in (0, 1):
                bits.append((sign << 31) | (hi << 16) | lo)
    bits += [0x80000000, 0x00000000, 0x7F7F0000, 0xFF7F0000]
    t = torch.tensor(bits, dtype=torch.int64)
    return torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32).view(F32)


@pytest.mark.parametrize("n", [41, 42, 43, 1024 + 3])
def test_shadow_rounds_to_nearest_even_in_body_and_tail(G, n):
    """lr = 0, wd = 0: p comes back bit for bit (g, m > 0, so that -0.0 keeps its sign through p - 0 * x), and the shadow must be
    torch's RNE cast of it.  The patterns are rotated so that ties over odd and even mantissas of both signs fall into the
    scalar tail (n % 4 = 1, 2, 3) as well as into the vectors."""
    pat = _tie_patterns()
    _, g, m, v = _state(n)
    g, m, v = g.abs() + 0.25, m.abs() + 0.25, v + 0.25
    for shift in range(4):
        p = torch.roll(pat.repeat(n // pat.numel() + 1)[:n], n - n % 4 - shift)  # the tail starts at pattern `shift`
        assert ((_bits(p[n - n % 4:]) & 0xFFFF) == 0x8000).all(), "the tail holds something else than ties"
        h = A.hyper_capi(0.0, 0.9, 0.999, 1e-8, 0.0, 3, 1.0)
        for decoupled in (0, 1):
            for out in _launch_both(G, (p, g, m, v), h, (0.9, 0.999), decoupled, 3, True):
                assert _same_bits(out[0], p), f"n={n} shift={shift}: p changed under lr = 0"
                assert _same_bits(out[3], p.to(BF16)), f"n={n} shift={shift}: shadow is not the RNE cast"
    G.check()


@pytest.mark.parametrize("cnt", [1, 5, 1023, PASS + 3])
@pytest.mark.parametrize("lo", [4, 8, 1028])
def test_interior_range_equals_whole_launch_and_leaves_the_rest(G, lo, cnt):
    """`FusedAdam.launch_range` hands the kernel interior pointers: inside [lo, hi) the result is the whole-buffer launch's bit
    for bit (an element may sit in a vector there and in the tail here), outside it no bit of p, m, v or the shadow changes"""
    hi = lo + cnt
    total = hi + 12
    state = tuple(t[:total] for t in _state(PASS + 1028 + 3 + 12))
    decoupled, step = 1, 7
    h = A.hyper_capi(LR, 0.9, 0.999, 1e-8, 0.05, step, 0.5)
    hd = G.poisoned(h.tensor().to(DEV))
    whole = [G.poisoned(t.to(DEV)) for t in state] + [G.empty((total,), dtype=BF16, device=DEV)]
    _lib.check(_step_dev(*whole, total, hd, decoupled), "adam_step_dev")
    part = [G.poisoned(t.to(DEV)) for t in state] + [G.empty((total,), dtype=BF16, device=DEV)]
    before16 = _bits(part[4]).clone()
    _lib.check(_step_dev(*part, cnt, hd, decoupled, off=lo), "adam_step_dev")
    views = [G.poisoned(t.to(DEV)) for t in state] + [G.empty((total,), dtype=BF16, device=DEV)]
    ops.adam_step(*(t[lo:hi] for t in views), lr=h.lr, beta1=0.9, beta2=0.999, eps=h.eps, weight_decay=h.wd,
                  decoupled=True, step=step, grad_scale=h.gscale)
    for name, i in (("p", 0), ("m", 2), ("v", 3), ("p16", 4)):
        w = _bits(whole[i])
        before = before16 if i == 4 else _bits(state[i])
        for entry, bufs in (("adam_step_dev", part), ("adam_step", views)):
            got = _bits(bufs[i])
            assert torch.equal(got[lo:hi], w[lo:hi]), f"{entry} [{lo}, {hi}) {name}: differs from the whole-buffer launch"
            assert torch.equal(got[:lo], before[:lo]) and torch.equal(got[hi:], before[hi:]), f"{entry} [{lo}, {hi}) {name}: written outside"
    for bufs in (whole, part, views):
        assert _same_bits(bufs[1], state[1])
    if cnt <= 1023:  # (what the bits are compared with is right; the large range's values: test_sizes_past_one_grid_pass)
        _check_step(whole[0], whole[2], whole[3], whole[4], state, h, decoupled, f"range base total={total}")


SHAPES = [(1,), (7,), (8,), (9,), (3, 5), (1025,)]  # arena offsets 0, 8, 16, 24, 40, 56: padding after all but the (8,)


def _make(cls=FusedAdam, seed=5, **kw):
    """-> (optimizer, FusedAdam, arena) over fresh parameters of SHAPES (unit scale, the same for one seed)"""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(s, generator=gen, dtype=F64) * 1.5).float().to(DEV)) for s in SHAPES]
    opt = cls(params, **kw)
    fused = opt.fused if hasattr(opt, "fused") else opt
    return opt, fused, fused.arena


def _grads(arena, seed, scale=1.0):
    """fixed synthetic gradients, written through the parameters' `.grad` views (the padding of flat_g stays zero)"""
    gen = torch.Generator().manual_seed(100 + seed)
    for p in arena.params:
        p.grad.copy_((torch.randn(p.shape, generator=gen, dtype=F64) * scale).float())


def _flat(fused):
    a = fused.arena
    return a.flat_p.cpu(), a.flat_g.cpu(), fused.exp_avg.cpu(), fused.exp_avg_sq.cpu()


def _all_bits(fused):
    a = fused.arena
    return [_bits(t) for t in (a.flat_p, fused.exp_avg, fused.exp_avg_sq, a.flat_p16)]


def _assert_same_state(x, y, tag):
    for name, s, t in zip(("p", "m", "v", "p16"), _all_bits(x), _all_bits(y)):
        assert torch.equal(s, t), f"{tag}: {name} differs"
    assert x.step_count == y.step_count, tag


PIECES = {
    "first at 0": [(0, 16)],
    "last ends at total": [(1080, 1088)],
    "two adjacent": [(16, 40), (40, 64)],
    "one of 8 elements": [(24, 32)],
    "none": [],
    "all kinds": [(0, 8), (16, 40), (40, 64), (512, 520), (1000, 1088)],
    "open at both ends": [(8, 16), (64, 1080)],
}


@pytest.mark.parametrize("name", list(PIECES))
def test_partitions_through_fused_adam(name):
    """launch_range pieces after prepare_step(), the rest by launch_step()'s complement walk: the same bits as one launch, in
    the given order and shuffled.  State and gradients fill the whole arena here, padding included, so that every element tells."""
    results = []
    pieces = PIECES[name]
    orders = [None, pieces, pieces[::-1], pieces[1::2] + pieces[0::2]]
    for order in orders:
        _, fused, arena = _make(lr=LR, weight_decay=0.05, decoupled=True)
        assert arena.total == 1088 and arena.offsets == [0, 8, 16, 24, 40, 56]
        p, g, m, v = (t.to(DEV) for t in A.mixed_state(arena.total, 77))
        arena.flat_p.copy_(p), arena.flat_g.copy_(g), fused.exp_avg.copy_(m), fused.exp_avg_sq.copy_(v)
        fused.step_count = 4
        fused.prepare_step()
        for lo, hi in order or []:
            fused.launch_range(lo, hi)
        fused.launch_step()
        assert not fused._done and torch.equal(arena.flat_g.cpu(), g.cpu())
        results.append(_all_bits(fused))
    for r in results[1:]:
        for nm, s, t in zip(("p", "m", "v", "p16"), results[0], r):
            bad = torch.nonzero(s != t).view(-1)
            assert bad.numel() == 0, f"pieces '{name}': {nm} differs from one launch at {bad.numel()} elements, first {int(bad[0])}"
    assert not torch.equal(results[0][0], _bits(p))  # (and the launch did something)


def test_refusals_write_nothing_and_empty_launch_succeeds(G):
    n = 64
    state = _state(n + 4)
    h = A.hyper_capi(LR, 0.9, 0.999, 1e-8, 0.05, 1, 1.0)
    hd = G.poisoned(h.tensor().to(DEV))
    bufs = [G.poisoned(t.to(DEV)) for t in state] + [G.poisoned(state[0].to(BF16).to(DEV))]
    before = [_bits(t).clone() for t in bufs]
    lib = _lib.load()
    for i, name in enumerate(("p", "g", "m", "v", "p16")):  # one element into the buffer: 4 bytes (2 for the shadow) off alignment
        shifted = [t[1:n + 1] if j == i else t[:n] for j, t in enumerate(bufs)]
        with pytest.raises(RuntimeError, match="aligned"):
            ops.adam_step(*shifted, lr=h.lr, beta1=h.beta1, beta2=h.beta2, eps=h.eps, weight_decay=h.wd, decoupled=True, step=1)
        with pytest.raises(RuntimeError, match="aligned"):
            _lib.check(lib.cfhip_adam_step_dev(*(_ptr(t) for t in shifted), n, hd.data_ptr(), 1, _stream()), f"adam_step_dev {name}")
    with pytest.raises(RuntimeError, match="bad arguments"):
        ops.adam_step(*(t[:n] for t in bufs), lr=h.lr, beta1=h.beta1, beta2=h.beta2, eps=h.eps, weight_decay=h.wd, decoupled=True, step=0)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _lib.check(_step_capi(*bufs, -1, h, 1, 1), "adam_step n < 0")
    with pytest.raises(RuntimeError, match="bad arguments"):
        _lib.check(_step_dev(*bufs, -1, hd, 1), "adam_step_dev n < 0")
    assert _step_capi(*bufs, 0, h, 1, 1) == 0 and _step_dev(*bufs, 0, hd, 1) == 0  # n = 0: success, no launch
    torch.cuda.synchronize()
    for name, t, b in zip(("p", "g", "m", "v", "p16"), bufs, before):
        assert torch.equal(_bits(t), b), f"a refused or empty launch wrote {name}"


# ---------------------------------------------------------------------------------------------
# FusedAdam end to end, without a model
# ---------------------------------------------------------------------------------------------


def _padding_mask(arena):
    pad = torch.ones(arena.total, dtype=torch.bool)
    for p, o in zip(arena.params, arena.offsets):
        pad[o:o + p.numel()] = False
    return pad


def _teacher_forced_step(fused, do_step, lr, t, gscale, tag):
    """the state before the step, the step, then p', m', v' against the reference on that state: one step's bound at every step"""
    before = _flat(fused)
    do_step()
    g = fused.param_groups[0]
    h = A.hyper_fused(lr, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], t, gscale)
    a = fused.arena
    assert fused.step_count == t and torch.equal(a.flat_g.cpu(), before[1])
    _check_step(a.flat_p, fused.exp_avg, fused.exp_avg_sq, a.flat_p16, before, h, fused.decoupled, tag)


@pytest.mark.parametrize("cls", [FusedAdamOptimizer, FusedAdamWOptimizer])
def test_six_steps_under_a_scheduler(cls):
    """a LambdaLR writes `param_groups[0]["lr"]` every step; the record must carry that rate and this step's bias corrections;
    the arena's padding (and that of the moments and the shadow) stays exactly zero"""
    opt, fused, arena = _make(cls, lr=LR, weight_decay=0.05, betas=(0.9, 0.99), eps=1e-7)
    assert fused.decoupled == (cls is FusedAdamWOptimizer) and _padding_mask(arena).sum() == 1088 - 1065
    factor = lambda e: 1.0 / (1.0 + 0.7 * e)  # noqa: E731
    sched = torch.optim.lr_scheduler.LambdaLR(opt, factor)
    for t in range(1, 7):
        _grads(arena, t)
        lr = opt.param_groups[0]["lr"]
        assert lr == LR * factor(t - 1)
        _teacher_forced_step(fused, opt.step, lr, t, 1.0, f"{cls.__name__} step {t}")
        sched.step()
    pad = _padding_mask(arena)
    for name, t in (("flat_p", arena.flat_p), ("exp_avg", fused.exp_avg), ("exp_avg_sq", fused.exp_avg_sq), ("shadow", arena.flat_p16)):
        assert not _bits(t)[pad].any(), f"padding of {name} is not zero"


def test_grad_scale_persists_and_step_clip_lasts_one_step():
    _, fused, arena = _make(lr=LR, weight_decay=0.05, decoupled=False)
    fused.grad_scale = 0.25
    clip = torch.tensor(0.3, dtype=F32)
    for t in (1, 2, 3):
        _grads(arena, t)

        def do_step():
            fused.prepare_step()
            if t == 2:
                fused.set_step_clip(clip.to(DEV))
            fused.launch_step()

        gscale = float(clip * 0.25) if t == 2 else 0.25  # f32(0.3) * 0.25 is exact in f32
        _teacher_forced_step(fused, do_step, LR, t, gscale, f"grad_scale step {t}")
        assert fused.grad_scale == 0.25 and fused._step_clip is None


def _norm_check(total, g_flat, base):
    """sqrt(sumsq) * base: sumsq by test_sumsq_and_dot's model (k = depth + 1 on sum g^2), halved by the square root, plus the
    rounding of the root and of the product"""
    n = g_flat.numel()
    blocks = min(max(1, -(-n // 2048)), 1024)
    depth = -(-n // (blocks * 256)) + 8 + blocks
    want = g_flat.double().norm() * base
    _check(total, (want.reshape(1), want.reshape(1)), (depth + 1) / 2 + 2, f"clip norm n={n}")


def _coef(norm_got, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in f32 from the device's own norm"""
    return (float(max_norm) / (norm_got.cpu().float() + 1.0e-6)).clamp(max=1.0)


@pytest.mark.parametrize("max_norm,clips", [(0.5, True), (1.0e4, False)])
def test_clip_grad_norm_with_an_optimizer(max_norm, clips):
    _, fused, arena = _make(lr=LR, weight_decay=0.0, decoupled=True)
    fused.grad_scale = 0.5
    _grads(arena, 1)
    fused.step()
    _grads(arena, 2, scale=2.0)
    g0 = arena.flat_g.cpu()
    total = clip_grad_norm_(arena, max_norm, fused)
    assert tuple(total.shape) == (1,) and total.is_cuda
    _norm_check(total, g0, 0.5)
    coef = _coef(total, max_norm)
    assert (coef.item() < 1.0) == clips
    _teacher_forced_step(fused, fused.step, LR, 2, float(coef * 0.5), f"clipped step max_norm={max_norm}")
    assert torch.equal(arena.flat_g.cpu(), g0) and fused.grad_scale == 0.5  # with an optimizer the arena itself is not scaled
    _grads(arena, 3)
    _teacher_forced_step(fused, fused.step, LR, 3, 0.5, "the step after the clipped one")


@pytest.mark.parametrize("max_norm,clips", [(0.5, True), (1.0e4, False)])
def test_clip_grad_norm_scales_the_arena_in_place(max_norm, clips):
    _, fused, arena = _make(lr=LR)
    _grads(arena, 4, scale=3.0)
    g0 = arena.flat_g.cpu()
    total = clip_grad_norm_(arena, max_norm)
    _norm_check(total, g0, 1.0)
    coef = _coef(total, max_norm)
    got = arena.flat_g.cpu()
    if not clips:
        assert coef.item() == 1.0 and _same_bits(got, g0)
        return
    assert coef.item() < 1.0
    # one rounding per element: g * coef (the coefficient itself an f32 value)
    assert_elementwise(got, g0.double() * coef.double(), out_dtype=F32, ulps=1, what="clipped arena")


def test_resume_from_state_dict_is_bit_identical():
    _, a, arena_a = _make(lr=LR, weight_decay=0.05, decoupled=True)
    for t in (1, 2, 3):
        if t == 2:
            a.param_groups[0]["lr"] = 4e-3  # a scheduler's rate travels in the state dict's param_groups
        _grads(arena_a, t)
        a.step()
    flat_p = arena_a.flat_p.clone()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    _, b, arena_b = _make(seed=6, lr=LR, weight_decay=0.0, decoupled=True)
    arena_b.flat_p.copy_(flat_p)
    arena_b.refresh_shadow()
    b.load_state_dict(sd)
    assert b.step_count == 3 and b.param_groups[0]["lr"] == 4e-3 and b.param_groups[0]["weight_decay"] == 0.05
    _assert_same_state(a, b, "after load_state_dict")
    for t in (4, 5, 6):
        for f, ar in ((a, arena_a), (b, arena_b)):
            _grads(ar, t)
            f.step()
        _assert_same_state(a, b, f"resumed, step {t}")
    assert a.step_count == 6


def test_snapshot_restore_replays_the_same_steps():
    _, f, arena = _make(lr=LR, weight_decay=0.05, decoupled=False)
    arena.double_buffer_shadows()
    _grads(arena, 1)
    f.step()
    snap = f.snapshot()
    want0 = [t.clone() for t in _all_bits(f)]
    for t in (2, 3):
        _grads(arena, t)
        f.step()
    after = [t.clone() for t in _all_bits(f)]
    assert f.step_count == 3 and not torch.equal(after[0], want0[0])
    f.restore(snap)
    assert f.step_count == 1
    for name, s, t in zip(("p", "m", "v", "p16"), _all_bits(f), want0):
        assert torch.equal(s, t), f"restore: {name}"
    assert torch.equal(_bits(arena.flat_p16_alt), want0[3]), "restore: the second shadow arena does not hold the pre-step values"
    for t in (2, 3):
        _grads(arena, t)
        f.step()
    for name, s, t in zip(("p", "m", "v", "p16"), _all_bits(f), after):
        assert torch.equal(s, t), f"replayed after restore: {name}"
    for p in arena.params:  # the views the forward reads are those of the current shadow arena
        assert torch.equal(p._cfhip_shadow, p.detach().to(BF16))


def test_graph_replay_follows_eager_over_the_hyper_ring():
    """`launch_step()` alone in a captured graph (one stream: no parallel branches), `prepare_step()` and a new learning rate in
    front of each of ten replays — more than the 8 slots of the pinned hyper ring"""
    _, e, arena_e = _make(lr=LR, weight_decay=0.05, decoupled=True)
    _, g, arena_g = _make(lr=LR, weight_decay=0.05, decoupled=True)
    snap = g.snapshot()
    g.step()  # warm-up outside the capture (library and allocator), rolled back
    g.restore(snap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    g.prepare_step()
    with torch.cuda.graph(graph):
        g.launch_step()
    g.step_count = 0
    torch.cuda.synchronize()
    _assert_same_state(e, g, "capture must not step")
    steps = _HYPER_RING + 2
    for t in range(1, steps + 1):
        lr = LR / t
        for f, ar in ((e, arena_e), (g, arena_g)):
            f.param_groups[0]["lr"] = lr
            _grads(ar, t)
        e.step()
        g.prepare_step()
        graph.replay()
        _assert_same_state(e, g, f"graph replay {t}")
    assert e.step_count == steps
