"""Every convolution kernel the router can select, per element against float64, with guarded outputs and poisoned inputs.

The implicit-GEMM 3x3 convolution (cfhip_conv3x3_nhwc_bf16) in each of its four tile forms and with whole and split reductions
(forced through the `conv_form` / `conv_split` options, and as `conv_plan` in csrc/gemm.hip chooses by itself), its use as the input
gradient (rotated filters) and as the thin head (zero filters up to 32 channels), the 3x3 weight gradient at the channel widths its
C entry admits, the three grouped-convolution kernels of csrc/conv_grouped.hip through `ops`, and the im2row / row2im gathers with
their `_pad` forms.  Every case: floating inputs are poisoned device copies, outputs (and workspaces) the wrappers allocate lie
between guards and start as NaN, every output element is compared, the guard check runs at the end.

Error models — none is measured, each follows from the length of the sum and holds for any summation order (n terms take n - 1
additions, each rounding at most 2^-24 of the sum of the absolute values; bf16 x bf16 products are exact in f32):
  * bf16 output of an f32 sum of n products plus bias: ulps = 1 (the one rounding to bf16), k = n + 1, cond = the same
    convolution on absolute values.
  * f32 output (weight / bias gradients, also accumulated onto a pre-filled destination): ulps = 1, k = n + 1.
  * pure gathers: torch.equal."""
import contextlib
import functools

import pytest
import torch

from helpers import assert_conv3x3_rows, assert_elementwise, conv3x3_rows_ref, guarded_ops

pytestmark = pytest.mark.gpu

from cflearn_amd import _lib, ops  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
conv2d = torch.nn.functional.conv2d


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _randn(shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)


def _dev(g, t):
    """a poisoned device copy of a floating CPU tensor"""
    return g.poisoned(t.to(DEV))


def _rows(t):
    """[B, C, H, W] -> NHWC rows [B H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


@contextlib.contextmanager
def _conv_options(form, split):
    """`conv_form` / `conv_split` for the duration of a block; both back at -1 afterwards, whatever happens inside"""
    try:
        ops.set_option("conv_form", form)
        ops.set_option("conv_split", split)
        yield
    finally:
        ops.set_option("conv_form", -1)
        ops.set_option("conv_split", -1)


def _forced_split(cin, split):
    """the number of K slices conv_plan makes of a forced `conv_split`: 64-wide steps, equal slices, no empty one"""
    steps = -(-9 * cin // 64)
    per = -(-steps // min(split, steps))
    return -(-steps // per)


def _workspace(b, cin, cout, h, w):
    return _lib.load().cfhip_conv3x3_workspace(b, h, w, cin, cout)


# ---------------------------------------------------------------------------------------------
# 1. forward: every tile form, whole-K and split
# ---------------------------------------------------------------------------------------------

FWD_SHAPES = [
    (3, 64, 152, 7, 5),     # 105 pixels: one partial M tile; Cout ends inside the second wave's 80 columns (forms 2, 3), crosses the 128-column tile (0, 1)
    (2, 64, 168, 13, 11),   # 286 pixels: a second, 30-row tile in form 0, three tiles in the others; the second 160-column tile has 8 columns
    (1, 128, 320, 9, 15),   # two full 160-column tiles, 18 K-steps of 64 (two per tap), three slices of three taps
    (2, 96, 160, 1, 9),     # H = 1: every off-centre row is padding, pixels p +- 1 of a row end belong to the next image; Cin % 64 != 0: form 3 -> 2
    (2, 32, 160, 6, 1),     # W = 1: the same along x
    (1, 32, 8, 1, 1),       # one pixel, 8 of the 9 taps padding, the smallest Cout
]


@functools.lru_cache(maxsize=None)
def _fwd_case(b, cin, cout, h, w):
    """operands and float64 references of one shape, made once (with bias, without)"""
    x = _randn((b, cin, h, w), b + cin + h + 3 * w, dtype=BF16)
    wt = _randn((cout, cin, 3, 3), cout + cin, 1.0 / (3.0 * cin ** 0.5), BF16)
    bias = _randn(cout, 5)
    return x, wt, bias, conv3x3_rows_ref(x, wt, bias), conv3x3_rows_ref(x, wt, None)


@pytest.mark.parametrize("b,cin,cout,h,w", FWD_SHAPES)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_conv3x3_forward_every_form_and_split(G, form, split, b, cin, cout, h, w):
    """forms 0 .. 3 (256x128x32, 128x128x32, 128x160x32, 128x160x64; 3 falls back to 2 where Cin % 64 != 0), the whole reduction
    and three K slices (f32 slabs in the guarded workspace, then the ordered reduce), with and without bias"""
    x, wt, bias, ref_b, ref_n = _fwd_case(b, cin, cout, h, w)
    x_rows = _dev(G, _rows(x))
    wk = ops.conv3x3_pack_filters(_dev(G, wt), False)
    bias_d = _dev(G, bias)
    slices = _forced_split(cin, split)
    with _conv_options(form, split):
        # the split is in force: the workspace the wrapper is about to allocate has one f32 slab per slice
        assert _workspace(b, cin, cout, h, w) == (slices * b * h * w * cout * 4 if slices > 1 else 0)
        y_b = ops.conv3x3_nhwc(x_rows, wk, bias_d, b, h, w)
        y_n = ops.conv3x3_nhwc(x_rows, wk, None, b, h, w)
    tag = f"conv3x3 form {form} split {split} {(b, cin, cout, h, w)}"
    assert_conv3x3_rows(y_b, ref_b, cin, tag + " bias")
    assert_conv3x3_rows(y_n, ref_n, cin, tag + " no bias")
    if split == 1 and form != 1:
        # whole-K results do not depend on the tile form: the K order inside a tile is the same in every form
        with _conv_options(1, 1):
            assert torch.equal(ops.conv3x3_nhwc(x_rows, wk, bias_d, b, h, w), y_b), tag + ": differs from form 1 (bias)"
            assert torch.equal(ops.conv3x3_nhwc(x_rows, wk, None, b, h, w), y_n), tag + ": differs from form 1 (no bias)"
    G.check()


# ---------------------------------------------------------------------------------------------
# 2. the plan's own choice
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("b,cin,cout,h,w,split", [
    (1, 128, 160, 5, 7, 2),    # form 3: one 160-column tile, 18 steps -> 2 slices
    (1, 256, 160, 4, 4, 4),    # form 3: 36 steps -> 4 slices
    (1, 32, 24, 32, 33, 1),    # form 0 (1056 pixels, Cout too narrow for 160-column tiles), 5 steps: no split
    (2, 96, 160, 1, 9, 1),     # form 2 (Cin % 64 != 0), 14 steps: no split
])
def test_conv3x3_forward_as_planned(G, b, cin, cout, h, w, split):
    """both options at -1: the K split (the one part of the plan a caller can see, through the workspace size) is the one worked
    out by hand from conv_plan, and the result holds per element"""
    x, wt, bias, ref_b, _ = _fwd_case(b, cin, cout, h, w)
    assert _workspace(b, cin, cout, h, w) == (split * b * h * w * cout * 4 if split > 1 else 0)
    y = ops.conv3x3_nhwc(_dev(G, _rows(x)), ops.conv3x3_pack_filters(_dev(G, wt), False), _dev(G, bias), b, h, w)
    assert_conv3x3_rows(y, ref_b, cin, f"conv3x3 planned {(b, cin, cout, h, w)}")
    G.check()


# ---------------------------------------------------------------------------------------------
# 3. the input gradient (rotated filters) and the thin head
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("b,cin,cout,h,w,forms", [
    (2, 40, 96, 5, 6, (-1,)),                # the kernel sees Cin 96, Cout 40
    (1, 160, 128, 7, 9, (-1, 0, 1, 2, 3)),   # the kernel sees Cin 128, Cout 160: form 3 with two K slices by the plan
])
def test_conv3x3_input_gradient_through_rotated_filters(G, b, cin, cout, h, w, forms):
    wt = _randn((cout, cin, 3, 3), cout + cin, 1.0 / (3.0 * cin ** 0.5), BF16)
    dy = _randn((b, cout, h, w), 17 + cout, dtype=BF16)
    w16 = _dev(G, wt)
    wk, wr = ops.conv3x3_pack_filters(w16, False), ops.conv3x3_pack_filters(w16, True)
    assert torch.equal(wk.cpu(), wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin))
    assert torch.equal(wr.cpu(), wt.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, 9 * cout))
    conv_in = torch.nn.grad.conv2d_input
    want = _rows(conv_in((b, cin, h, w), wt.double(), dy.double(), padding=1))
    cond = _rows(conv_in((b, cin, h, w), wt.double().abs(), dy.double().abs(), padding=1))
    dy_rows = _dev(G, _rows(dy))
    if (b, cin, cout, h, w) == (1, 160, 128, 7, 9):
        assert _workspace(b, cout, cin, h, w) == 2 * b * h * w * cin * 4
    for form in forms:
        with _conv_options(form, -1):
            dx_rows = ops.conv3x3_nhwc(dy_rows, wr, None, b, h, w)
        # an f32 sum of 9 Cout exact products, one rounding to bf16
        assert_elementwise(dx_rows, want, out_dtype=BF16, ulps=1, cond=cond, k=9 * cout + 1, what=f"conv3x3 dX {(b, cin, cout, h, w)} form {form}")
    G.check()


@pytest.mark.parametrize("cout", [3, 5])
def test_conv3x3_thin_head_per_element(G, cout):
    """a 3x3 convolution onto a few channels runs the implicit kernel on zero filters up to 32 channels (forward, dX, dW, db); the
    zero filters' products are exact zeros, so the sums are those of `cout` channels.  The second backward accumulates: the f32
    gradients add one rounding for the sum of the two passes (n - 1 additions each and one more: still within k = n + 1 on the
    doubled cond), and the bf16 dX of two identical passes is exactly twice that of one."""
    b, cin, h, w = 2, 32, 6, 5
    assert HF.conv_route(cin, cout, 3, 3, 1, 1, 1, h, w) == ("implicit", 32)
    x = _randn((b, cin, h, w), 31 + cout, dtype=BF16)
    wt = _randn((cout, cin, 3, 3), 32 + cout, 1.0 / (3.0 * cin ** 0.5), BF16)
    bias = _randn(cout, 33 + cout)
    dy = _randn((b, cout, h, w), 34 + cout, dtype=BF16)
    x64, w64, dy64, n = x.double(), wt.double(), dy.double(), b * h * w
    xd = _dev(G, x).requires_grad_(True)
    wd, bd = _dev(G, wt.float()).requires_grad_(True), _dev(G, bias).requires_grad_(True)
    dyd = _dev(G, dy)
    want_dx = torch.nn.grad.conv2d_input(x.shape, w64, dy64, padding=1)
    cond_dx = torch.nn.grad.conv2d_input(x.shape, w64.abs(), dy64.abs(), padding=1)
    want_w = torch.nn.grad.conv2d_weight(x64, wt.shape, dy64, padding=1)
    cond_w = torch.nn.grad.conv2d_weight(x64.abs(), wt.shape, dy64.abs(), padding=1)
    dx_first = None
    for rep in (1, 2):
        y = HF.conv2d(xd, wd, bd, 1, 1, 1)
        y.backward(dyd)
        HF.SideStream.join()
        assert y.dtype == BF16 and tuple(y.shape) == (b, cout, h, w)
        assert_elementwise(y, conv2d(x64, w64, bias.double(), padding=1), out_dtype=BF16, ulps=1,
                           cond=conv2d(x64.abs(), w64.abs(), bias.double().abs(), padding=1), k=9 * cin + 1, what=f"thin head {cout} y")
        if rep == 1:
            assert_elementwise(xd.grad, want_dx, out_dtype=BF16, ulps=1, cond=cond_dx, k=9 * cout + 1, what=f"thin head {cout} dX")
            dx_first = xd.grad.clone()
        else:
            assert torch.equal(xd.grad, 2 * dx_first), f"thin head {cout}: dX of the second pass differs from the first"
        assert wd.grad.dtype == F32 and bd.grad.dtype == F32
        assert_elementwise(wd.grad, rep * want_w, out_dtype=F32, ulps=1, cond=rep * cond_w, k=n + 1, what=f"thin head {cout} dW pass {rep}")
        assert_elementwise(bd.grad, rep * dy64.sum((0, 2, 3)), out_dtype=F32, ulps=1, cond=rep * dy64.abs().sum((0, 2, 3)), k=n + 1,
                           what=f"thin head {cout} db pass {rep}")
    G.check()


# ---------------------------------------------------------------------------------------------
# 4. the 3x3 weight gradient at the widths its C entry admits
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("b,cin,cout,h,w", [
    (2, 8, 16, 5, 7),      # Cin % 8 == 0, not a multiple of 32
    (1, 24, 40, 4, 4),     # the same, Cout past one 32-row block
    (2, 64, 160, 9, 7),
])
@pytest.mark.parametrize("split", [1, 3])
def test_conv3x3_weight_gradient_widths(G, b, cin, cout, h, w, split):
    assert ops.conv3x3_wgrad_ok(b, h, w)
    x = _randn((b, cin, h, w), b + cin + h, dtype=BF16)
    dy = _randn((b, cout, h, w), 11 + cout, dtype=BF16)
    x64, dy64, n = x.double(), dy.double(), b * h * w
    x_rows, dy_rows = _dev(G, _rows(x)), _dev(G, _rows(dy))
    want_w = torch.nn.grad.conv2d_weight(x64, (cout, cin, 3, 3), dy64, padding=1)
    cond_w = torch.nn.grad.conv2d_weight(x64.abs(), (cout, cin, 3, 3), dy64.abs(), padding=1)
    # accumulated onto pre-filled destinations: an f32 sum of B H W exact products per filter tap and the value that was there
    dw = G.out2d(1, cout * cin * 9, cout * cin * 9, F32, DEV, fill=0.25).view(cout, cin, 3, 3)
    db = G.out2d(1, cout, cout, F32, DEV, fill=-0.25).view(cout)
    ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split_k=split, out=dw, accumulate=True, bias_grad=db, bias_grad_accumulate=True)
    tag = f"conv3x3 wgrad {(b, cin, cout, h, w)} split {split}"
    assert_elementwise(dw, want_w + 0.25, out_dtype=F32, ulps=1, cond=cond_w + 0.25, k=n + 1, what=tag + " dW acc")
    assert_elementwise(db, dy64.sum((0, 2, 3)) - 0.25, out_dtype=F32, ulps=1, cond=dy64.abs().sum((0, 2, 3)) + 0.25, k=n + 1, what=tag + " db acc")
    # written, without the bias gradient: the NaN the destination starts with is gone from every element
    dw2 = G.out2d(1, cout * cin * 9, cout * cin * 9, F32, DEV).view(cout, cin, 3, 3)
    ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split_k=split, out=dw2, accumulate=False, bias_grad=None)
    assert_elementwise(dw2, want_w, out_dtype=F32, ulps=1, cond=cond_w, k=n + 1, what=tag + " dW written, no db")
    G.check()


@pytest.mark.parametrize("b,cin,cout,h,w", [s for s in FWD_SHAPES if s[3] == 1 or s[4] == 1])
def test_conv3x3_weight_gradient_refuses_one_pixel_wide_images(G, b, cin, cout, h, w):
    """H = 1 or W = 1: `conv3x3_wgrad_ok` sends Conv2dFn to the im2row GEMM, and the C entry refuses before it launches anything"""
    assert not ops.conv3x3_wgrad_ok(b, h, w)
    x_rows = _dev(G, _rows(_randn((b, cin, h, w), 1, dtype=BF16)))
    dy_rows = _dev(G, _rows(_randn((b, cout, h, w), 2, dtype=BF16)))
    dw = G.out2d(1, cout * cin * 9, cout * cin * 9, F32, DEV, fill=0.25).view(cout, cin, 3, 3)
    db = G.out2d(1, cout, cout, F32, DEV, fill=-0.25).view(cout)
    with pytest.raises(RuntimeError, match="bad image shape"):
        ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split_k=1, out=dw, accumulate=True, bias_grad=db, bias_grad_accumulate=True)
    assert bool((dw == 0.25).all()) and bool((db == -0.25).all())  # the second pass of a launch would have added to both
    G.check()


# ---------------------------------------------------------------------------------------------
# 5. grouped convolution through `ops`
# ---------------------------------------------------------------------------------------------

GROUPED = [
    # b, cin, cout, h, w, k, stride, pad, dil, groups
    (2, 16, 16, 14, 14, 3, 1, 1, 1, 16),   # depthwise
    (3, 32, 64, 9, 11, 3, 2, 1, 1, 4),     # strided, 8 -> 16 channels per group
    (2, 24, 24, 13, 10, 5, 1, 2, 1, 24),   # depthwise 5x5
    (1, 12, 6, 8, 8, 3, 1, 2, 2, 3),       # dilated
    (2, 8, 8, 7, 7, 7, 1, 3, 1, 2),        # 49 taps
    (2, 6, 10, 5, 6, 1, 1, 0, 1, 2),       # 1x1
    (2, 12, 6, 9, 11, 2, 2, 1, 2, 3),      # 4 taps in the 9-tap template, stride and dilation together, odd sizes
    (1, 8, 8, 6, 6, 4, 1, 1, 1, 4),        # 16 taps: the 25-tap template
    (1, 4, 4, 7, 8, 6, 1, 2, 1, 2),        # 36 taps: the 49-tap template
    (3, 6, 6, 3, 3, 3, 1, 0, 1, 6),        # Ho = Wo = 1: three terms per sum, 253 threads idle
]


@pytest.mark.parametrize("b,cin,cout,h,w,k,s,p,d,g", GROUPED)
def test_grouped_convolution_kernels_per_element(G, b, cin, cout, h, w, k, s, p, d, g):
    cgi, cgo = cin // g, cout // g
    x = _randn((b, cin, h, w), b + cin + k, dtype=BF16)
    wt = _randn((cout, cgi, k, k), cout + k, 1.0 / (cgi * k * k) ** 0.5, BF16)
    bias = _randn(cout, 7)
    ho, wo = ops.conv_out_hw(h, w, k, k, s, p, d)
    dy = _randn((b, cout, ho, wo), 9 + ho, dtype=BF16)
    x64, w64, dy64 = x.double(), wt.double(), dy.double()
    geom = dict(stride=s, padding=p, dilation=d, groups=g)
    tag = f"grouped {(b, cin, cout, h, w, k, s, p, d, g)}"
    xd, wd, dyd = _dev(G, x), _dev(G, wt), _dev(G, dy)

    # forward: an f32 sum of (Cin / g) k k exact products and the bias
    for bi in (bias, None):
        b64 = None if bi is None else bi.double()
        y = ops.conv2d_grouped_fwd(xd, wd, None if bi is None else _dev(G, bi), s, p, d, g)
        assert tuple(y.shape) == (b, cout, ho, wo)
        assert_elementwise(y, conv2d(x64, w64, b64, **geom), out_dtype=BF16, ulps=1,
                           cond=conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), **geom), k=cgi * k * k + 1,
                           what=f"{tag} y bias {bi is not None}")

    # input gradient: an f32 sum of at most (Cout / g) k k exact products
    dx = ops.conv2d_grouped_bwd_input(dyd, wd, x.shape, s, p, d, g)
    assert_elementwise(dx, torch.nn.grad.conv2d_input(x.shape, w64, dy64, **geom), out_dtype=BF16, ulps=1,
                       cond=torch.nn.grad.conv2d_input(x.shape, w64.abs(), dy64.abs(), **geom), k=cgo * k * k, what=f"{tag} dX")

    # weight and bias gradients: f32 sums of B Ho Wo terms, added to or written over pre-filled destinations
    want_w = torch.nn.grad.conv2d_weight(x64, wt.shape, dy64, **geom)
    cond_w = torch.nn.grad.conv2d_weight(x64.abs(), wt.shape, dy64.abs(), **geom)
    want_b, cond_b = dy64.sum((0, 2, 3)), dy64.abs().sum((0, 2, 3))
    n = b * ho * wo
    for acc_w, acc_b, with_db in ((True, False, True), (False, True, True), (True, False, False)):
        dw = G.out2d(1, wt.numel(), wt.numel(), F32, DEV, fill=0.25).view(wt.shape)
        db = G.out2d(1, cout, cout, F32, DEV, fill=-0.25).view(cout)
        ops.conv2d_grouped_bwd_weight(dyd, xd, dw, acc_w, db if with_db else None, acc_b, s, p, d, g)
        flags = f"acc_w {acc_w} acc_b {acc_b} db {with_db}"
        assert_elementwise(dw, want_w + 0.25 * acc_w, out_dtype=F32, ulps=1, cond=cond_w + 0.25 * acc_w, k=n + 1, what=f"{tag} dW {flags}")
        if with_db:
            assert_elementwise(db, want_b - 0.25 * acc_b, out_dtype=F32, ulps=1, cond=cond_b + 0.25 * acc_b, k=n + 1, what=f"{tag} db {flags}")
        else:
            assert bool((db == -0.25).all()), f"{tag}: bias_grad=None, yet something wrote the bias gradient"
    G.check()


# ---------------------------------------------------------------------------------------------
# 6. the gathers
# ---------------------------------------------------------------------------------------------


def _gather_ref(x64, c, k, s, d, pads):
    """float64 im2row of x64 [B, C, H, W] through one-hot filters after F.pad(x, pads) (pads = (left, right, top, bottom)): rows
    [B Ho Wo, C k k] (k = (c, ky, kx)) -> (rows, Ho, Wo)"""
    kk = c * k * k
    eye = torch.eye(kk, dtype=torch.float64).view(kk, c, k, k)
    y = conv2d(torch.nn.functional.pad(x64, pads), eye, None, stride=s, padding=0, dilation=d)
    return y.permute(0, 2, 3, 1).reshape(-1, kk), y.shape[2], y.shape[3]


def _scatter_ref(r64, shape, c, k, s, d, pads):
    """the transpose of `_gather_ref` applied to r64 [B Ho Wo, C k k]: float64 [B, C, H, W]"""
    xg = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    _gather_ref(xg, c, k, s, d, pads)[0].backward(r64)
    return xg.grad


@pytest.mark.parametrize("b,c,h,w,k,s,p,d,pad_hi", [
    (2, 3, 9, 11, 3, 1, 1, 1, None), (3, 1, 28, 28, 7, 1, 3, 1, None), (2, 16, 14, 14, 3, 2, 1, 1, None), (1, 5, 13, 10, 3, 2, 2, 2, None),
    (2, 8, 7, 7, 1, 1, 0, 1, None),
    (2, 8, 9, 7, 3, 2, 0, 1, 1),   # F.pad(x, (0, 1, 0, 1)) and a stride-2 convolution: the encoder's down-sampling
])
def test_im2row_row2im_under_guards(G, b, c, h, w, k, s, p, d, pad_hi):
    x = _randn((b, c, h, w), b + c + h + k, dtype=BF16)
    hi = p if pad_hi is None else pad_hi
    pads = (p, hi, p, hi)
    want, ho, wo = _gather_ref(x.double(), c, k, s, d, pads)
    kk, m = c * k * k, b * ho * wo
    rows = {}
    for dt in (F32, BF16):
        r = ops.conv_im2row(_dev(G, x.to(dt)), k, k, s, p, d, pad_hi)
        assert r.dtype == BF16 and tuple(r.shape) == (m, (kk + 7) // 8 * 8)
        assert torch.equal(r[:, :kk].cpu().double(), want), f"im2row from {dt}"
        assert bool((r[:, kk:] == 0).all()), f"im2row from {dt}: the padding columns are not zero"
        rows[dt] = r
    kp = rows[F32].shape[1]
    r = _randn((m, kp), 3 + m, 0.25, BF16)
    r[:, kk:] = 0
    got = ops.conv_row2im(_dev(G, r), (b, c, h, w), k, k, s, p, d, pad_hi)
    # a sum of at most k k bf16 values in f32, one rounding to bf16
    assert_elementwise(got, _scatter_ref(r[:, :kk].double(), x.shape, c, k, s, d, pads), out_dtype=BF16, ulps=1,
                       cond=_scatter_ref(r[:, :kk].double().abs(), x.shape, c, k, s, d, pads), k=k * k, what="row2im")
    G.check()


def test_im2row_row2im_with_four_different_paddings(G):
    """cfhip_conv_im2row_pad / _row2im_pad take the padding above and left of the image separately (ConvGeom.pad, .pad_x): no rows
    above, one below, two columns to the left, none to the right — F.pad(x, (2, 0, 0, 1)) and a padding-0 convolution"""
    b, c, h, w, k, s, d = 2, 3, 6, 7, 3, 2, 1
    pad_t, pad_b, pad_l, pad_r = 0, 1, 2, 0
    x = _randn((b, c, h, w), 41, dtype=BF16)
    want, ho, wo = _gather_ref(x.double(), c, k, s, d, (pad_l, pad_r, pad_t, pad_b))
    assert (ho, wo) == (3, 4)
    kk, kp, m = c * k * k, (c * k * k + 7) // 8 * 8, b * ho * wo
    lib = _lib.load()
    for dt in (F32, BF16):
        rows = G.empty((m, kp), dtype=BF16, device=DEV)
        _lib.check(lib.cfhip_conv_im2row_pad(_dev(G, x.to(dt)).data_ptr(), int(dt == F32), rows.data_ptr(), b, c, h, w, k, k, s,
                                             pad_t, pad_b, pad_l, pad_r, d, kp, ops._stream()), "conv_im2row_pad")
        assert torch.equal(rows[:, :kk].cpu().double(), want), f"im2row_pad from {dt}"
        assert bool((rows[:, kk:] == 0).all())
    r = _randn((m, kp), 43, 0.25, BF16)
    r[:, kk:] = 0
    dx = G.empty((b, c, h, w), dtype=BF16, device=DEV)
    _lib.check(lib.cfhip_conv_row2im_pad(_dev(G, r).data_ptr(), dx.data_ptr(), b, c, h, w, k, k, s, pad_t, pad_b, pad_l, pad_r, d, kp,
                                         ops._stream()), "conv_row2im_pad")
    pads = (pad_l, pad_r, pad_t, pad_b)
    assert_elementwise(dx, _scatter_ref(r[:, :kk].double(), x.shape, c, k, s, d, pads), out_dtype=BF16, ulps=1,
                       cond=_scatter_ref(r[:, :kk].double().abs(), x.shape, c, k, s, d, pads), k=k * k, what="row2im_pad")
    G.check()
