"""The RRDB upscaler on the HIP path (csrc/conv_dense.hip, cflearn_amd.modules.RRDBNet).

1. `ops.conv3x3_dense` per element against float64 on the same bf16-rounded operands (helpers.assert_elementwise): ulps = 1, cond = the
   same computation on absolute values (residual terms included), k = 9 Cin + 1 + e with e the f32 roundings of the epilogue (0 none,
   1 lrelu, 2 res1, 4 res2) - the error model of helpers.assert_conv3x3_rows, no new constant.  Operands sit in guarded, poisoned
   buffers; every byte of the output buffer outside the written slice and every byte of the input and residual buffers is compared
   bit for bit with its value before the call.  Also the filter pack against a host restatement of its layout and the input kernel
   against the reference's pixel_unshuffle (tests/golden/rrdb_small.pt).
2. One whole dense block and one whole RRDB built from kernel calls on the dense buffers: every slice the fifteen launches wrote against
   float64 of the reference's expression (rrdb.py:22-29, :39-44) on the bf16 values the buffers hold - a rounding wherever the kernel
   stores one - on the same per-element terms: a wrong slice table or residual operand fails its own layer.
3. The module against the reference's fp32 CPU run for the three fixture configurations: rel_l2(out, y) <= 1.1 rel_l2(y_bf16, y), the
   reference's own bf16-autocast run being the yardstick (the factor of the sampler and img2img tests).
4. Launch discipline: bit-identical runs, eager against a captured graph, no torch.cat, 15 num_layers + 6 convolution launches, filter
   packs cached per parameter version, load_state_dict."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_elementwise, guarded_ops, rel_l2
from rrdb_weights import fill_parameters, seeded_state

pytestmark = pytest.mark.gpu

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YARDSTICK = 1.1
S = float(torch.tensor(0.2, dtype=F32))  # the f32 value of 0.2 the kernel multiplies by
EPI_ROUNDINGS = dict(none=0, lrelu=1, res1=2, res2=4)
TH, TW = ops.DENSE_TILE
IMAGES = [(1, 5, 7), (2, 9, 17), (1, 33, 18), (1, TH + 1, TW + 1), (1, TH - 1, TW - 1)]
# (Cin, ld_in, output offset, N, ld_out, real input channels, real output channels, f32 NCHW store); ld_out None: another buffer is
# not needed because the slice lies in the input's buffer
CASES = {
    "64-32": (64, 192, 64, 32, 192, 64, 32, False),
    "96-32": (96, 192, 96, 32, 192, 96, 32, False),
    "160-32": (160, 192, 160, 32, 192, 160, 32, False),
    "192-64": (192, 192, 0, 64, 192, 192, 64, False),
    "64-64": (64, 64, 0, 64, 64, 64, 64, False),
    "8-64": (8, 8, 0, 64, 64, 3, 64, False),
    "48-64": (48, 48, 0, 64, 64, 48, 64, False),
    "64-3": (64, 64, 0, 16, None, 64, 3, True),
}


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


@pytest.fixture(scope="module")
def fixture():
    return torch.load(os.path.join(GOLDEN, "rrdb_small.pt"), weights_only=False)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_ref(x_rows, b, h, w, wt, up2=False):
    """float64 (acc, cond) rows of the 3x3 / pad 1 convolution of bf16 rows [b h w, Cp] with wt [N, c <= Cp, 3, 3] (bf16-valued)"""
    x = x_rows.detach().cpu().double().view(b, h, w, -1).permute(0, 3, 1, 2)
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w64 = torch.zeros((wt.shape[0], x.shape[1], 3, 3), dtype=torch.float64)
    w64[:, :wt.shape[1]] = wt.detach().cpu().double()
    return _rows(F.conv2d(x, w64, padding=1)), _rows(F.conv2d(x.abs(), w64.abs(), padding=1))


def epilogue_ref(acc, cond, bias, epilogue, r1=None, r2=None):
    """float64 (want, cond) of the fused epilogue in the reference's operation order"""
    if bias is not None:
        acc, cond = acc + bias.detach().cpu().double(), cond + bias.detach().cpu().double().abs()
    if epilogue == "lrelu":
        acc = torch.where(acc > 0, acc, S * acc)
    if epilogue in ("res1", "res2"):
        r = r1.detach().cpu().double()
        acc, cond = S * acc + r, S * cond + r.abs()
    if epilogue == "res2":
        r = r2.detach().cpu().double()
        acc, cond = acc * S + r, cond * S + r.abs()
    return acc, cond


def check_dense(got, want, cond, cin, epilogue, what, out_dtype=BF16):
    assert_elementwise(got, want, out_dtype=out_dtype, ulps=1, cond=cond, k=9 * cin + 1 + EPI_ROUNDINGS[epilogue], what=what)


def _filters(n_real, cin_real, seed):
    gen = _gen(seed)
    wt = (torch.randn((n_real, cin_real, 3, 3), generator=gen) * (9 * cin_real) ** -0.5).to(BF16).float()
    return wt, torch.randn((n_real,), generator=gen)


def run_case(G, case, image, epilogue, with_bias, up2=False):
    cin, ld_in, off, n, ld_out, cin_real, n_real, f32_out = CASES[case]
    b, h, w = image
    ho, wo = (2 * h, 2 * w) if up2 else (h, w)
    p_in, p_out = b * h * w, b * ho * wo
    gen = _gen(1000 * h + w + 7 * cin)
    wt, bias = _filters(n_real, cin_real, cin * 100 + n)
    wp = ops.conv3x3_dense_pack(wt.to(DEV))
    bias_d = bias.to(DEV) if with_bias else None
    xbuf = G.poisoned(torch.randn((p_in, ld_in), generator=gen).to(BF16).to(DEV))
    same = off > 0
    assert not (same and up2)
    if f32_out:
        ybuf = y = ops.torch.empty((b, n_real, ho, wo), dtype=F32, device=DEV)  # guarded, NaN-filled
    else:
        ybuf = xbuf if same else G.poisoned(torch.randn((p_out, ld_out), generator=gen).to(BF16).to(DEV))
        y = ybuf[:, off:off + n_real]
    r1buf = G.poisoned(torch.randn((p_out, 96), generator=gen).to(BF16).to(DEV))
    r2buf = G.poisoned(torch.randn((p_out, 72), generator=gen).to(BF16).to(DEV))
    r1 = r1buf[:, 8:8 + n_real] if epilogue in ("res1", "res2") else None
    r2 = r2buf[:, :n_real] if epilogue == "res2" else None
    x_rows = xbuf[:, :cin].detach().cpu().clone()
    before = {name: _bits(t) for name, t in (("x", xbuf), ("y", ybuf), ("r1", r1buf), ("r2", r2buf))}
    out = ops.conv3x3_dense(xbuf[:, :cin], wp, bias_d, y, b, h, w, epilogue=epilogue, slope=0.2, r1=r1, s1=0.2, r2=r2, s2=0.2, up2=up2)
    assert out is y
    what = f"{case} {image} {epilogue} bias={with_bias} up2={up2}"
    acc, cond = conv_ref(x_rows, b, h, w, wt, up2)
    want, cond = epilogue_ref(acc, cond, bias if with_bias else None, epilogue, r1, r2)
    if f32_out:
        got = _rows(y.detach().cpu())
        check_dense(got, want, cond, cin, epilogue, what, out_dtype=F32)
    else:
        check_dense(y.detach().cpu().float(), want, cond, cin, epilogue, what)
        keep = torch.ones(ybuf.shape, dtype=torch.bool)
        keep[:, off:off + n_real] = False
        assert torch.equal(_bits(ybuf)[keep], before["y"][keep]), f"{what}: bytes outside the written slice changed"
    for name, t in (("x", xbuf), ("r1", r1buf), ("r2", r2buf)):
        if t is ybuf:
            continue
        assert torch.equal(_bits(t), before[name]), f"{what}: the {name} buffer changed"


@pytest.mark.parametrize("image", IMAGES, ids=lambda i: "x".join(map(str, i)))
@pytest.mark.parametrize("case", list(CASES))
def test_dense_kernel_per_element(G, case, image):
    for epilogue in EPI_ROUNDINGS:
        for with_bias in (True, False):
            run_case(G, case, image, epilogue, with_bias)


@pytest.mark.parametrize("image", [(1, 5, 7), (2, 9, 17)], ids=lambda i: "x".join(map(str, i)))
def test_dense_kernel_upsampled_input(G, image):
    """64 -> 64 behind the nearest 2x upsampling that is never built, odd H and W"""
    for epilogue in EPI_ROUNDINGS:
        for with_bias in (True, False):
            run_case(G, "64-64", image, epilogue, with_bias, up2=True)
    run_case(G, "64-3", image, "none", True, up2=True)


@pytest.mark.parametrize("cout,cin", [(32, 64), (32, 160), (64, 192), (64, 3), (64, 12), (64, 48), (3, 64), (5, 64)])
def test_pack_layout(G, cout, cin):
    """wp[n][tap Cp + c] = bf16(w[n][c][ky][kx]), Cp = Cin rounded up to 8, N = Cout rounded up to 16 / 32 / 64, Kp = 9 Cp rounded up
    to 32; every other position an exact zero"""
    w = torch.randn((cout, cin, 3, 3), generator=_gen(cout * 1000 + cin))
    wp = ops.conv3x3_dense_pack(w.to(DEV))
    cp, n = (cin + 7) // 8 * 8, 16 if cout <= 16 else 32 if cout <= 32 else 64
    kp = (9 * cp + 31) // 32 * 32
    want = torch.zeros((n, kp), dtype=BF16)
    for tap in range(9):
        want[:cout, tap * cp:tap * cp + cin] = w[:, :, tap // 3, tap % 3].to(BF16)
    assert wp.dtype == BF16 and tuple(wp.shape) == (n, kp)
    assert torch.equal(_bits(wp), _bits(want))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_input_kernel_is_the_references_unshuffle(G, fixture, dtype):
    ramp, outs = fixture["unshuffle"]["ramp"], fixture["unshuffle"]["out"]
    for s, want in outs.items():  # the reference's own result (a ramp: bf16 keeps it up to 256, rounds above)
        got = ops.pixel_unshuffle_nhwc(G.poisoned(ramp.to(dtype).to(DEV)), s)
        c2 = want.shape[1]
        assert got.dtype == BF16 and tuple(got.shape) == (1, want.shape[2], want.shape[3], (c2 + 7) // 8 * 8)
        assert torch.equal(got[..., :c2].cpu(), want.to(dtype).to(BF16).permute(0, 2, 3, 1))
        assert not bool(got[..., c2:].cpu().float().abs().any()), "padding channels must be zero"
    for s, (b, c, h, w) in ((1, (2, 3, 5, 7)), (2, (2, 3, 6, 10)), (4, (1, 5, 8, 12)), (1, (1, 8, 3, 3))):
        x = torch.randn((b, c, h, w), generator=_gen(s * 10 + c)).to(dtype)
        got = ops.pixel_unshuffle_nhwc(G.poisoned(x.to(DEV)), s).cpu()
        m = ops.pixel_unshuffle_map(c, h, w, s)  # (pinned to the reference by tests/test_rrdb_host.py)
        want = x.reshape(b, -1)[:, m].to(BF16)
        assert torch.equal(got[..., :c * s * s], want) and not bool(got[..., c * s * s:].float().abs().any())


# ---------------------------------------------------------------------------------------------
# one dense block, one RRDB
# ---------------------------------------------------------------------------------------------

LAT, GROW, WIDE = 64, 32, 192


def _rdb_filters(seed):
    out = []
    for i in range(5):
        cin, cout = LAT + i * GROW, GROW if i < 4 else LAT
        gen = _gen(seed * 10 + i)
        wt = (torch.randn((cout, cin, 3, 3), generator=gen) * 1.2 * (9 * cin) ** -0.5).to(BF16).float()
        out.append((wt, torch.randn((cout,), generator=gen) * 0.1, ops.conv3x3_dense_pack(wt.to(DEV))))
    return out


def _launch_rdb(filters, src, dst, outer, b, h, w):
    """the five launches of rrdb.py:22-29 on the dense buffers: src[:, :64] is the input, src[:, 64:] receives net1 .. net4, the
    result goes to dst[:, :64]; `outer`: the RRDB's input, for the third block (rrdb.py:44)"""
    for i in range(4):
        cin = LAT + i * GROW
        ops.conv3x3_dense(src[:, :cin], filters[i][2], filters[i][1].to(DEV), src[:, cin:cin + GROW], b, h, w, epilogue="lrelu", slope=0.2)
    if outer is None:
        ops.conv3x3_dense(src, filters[4][2], filters[4][1].to(DEV), dst[:, :LAT], b, h, w, epilogue="res1", s1=0.2, r1=src[:, :LAT])
    else:
        ops.conv3x3_dense(src, filters[4][2], filters[4][1].to(DEV), dst[:, :LAT], b, h, w, epilogue="res2", s1=0.2, r1=src[:, :LAT],
                          s2=0.2, r2=outer[:, :LAT])


def _check_rdb(filters, src, dst, outer, b, h, w, what):
    """every slice the five launches wrote, from the bf16 values the buffers hold now"""
    src_c, dst_c = src.detach().cpu(), dst.detach().cpu()
    for i in range(4):
        cin = LAT + i * GROW
        acc, cond = conv_ref(src_c[:, :cin], b, h, w, filters[i][0])
        want, cond = epilogue_ref(acc, cond, filters[i][1], "lrelu")
        check_dense(src_c[:, cin:cin + GROW].float(), want, cond, cin, "lrelu", f"{what} conv{i + 1}")
    acc, cond = conv_ref(src_c, b, h, w, filters[4][0])
    epilogue = "res1" if outer is None else "res2"
    want, cond = epilogue_ref(acc, cond, filters[4][1], epilogue, src_c[:, :LAT], None if outer is None else outer.detach().cpu()[:, :LAT])
    check_dense(dst_c[:, :LAT].float(), want, cond, WIDE, epilogue, f"{what} conv5")


def test_one_dense_block_and_one_rrdb(G):
    b, h, w = 2, TH + 3, TW + 5  # 2 x 2 tiles per image, two images
    rows = b * h * w
    inp = torch.randn((rows, LAT), generator=_gen(5)).to(BF16)
    bufs = [G.poisoned(torch.randn((rows, WIDE), generator=_gen(6 + i)).to(BF16).to(DEV)) for i in range(3)]
    bufs[0][:, :LAT] = inp.to(DEV)
    blocks = [_rdb_filters(seed) for seed in (1, 2, 3)]
    # one dense block: buffer 0 -> buffer 1
    _launch_rdb(blocks[0], bufs[0], bufs[1], None, b, h, w)
    _check_rdb(blocks[0], bufs[0], bufs[1], None, b, h, w, "rdb1")
    assert torch.equal(bufs[0][:, :LAT].cpu(), inp), "the block's input changed"
    # the rest of the RRDB: 1 -> 2, then 2 -> 1 with the RRDB's input (buffer 0) as the second residual
    _launch_rdb(blocks[1], bufs[1], bufs[2], None, b, h, w)
    _check_rdb(blocks[1], bufs[1], bufs[2], None, b, h, w, "rdb2")
    tail1 = _bits(bufs[1][:, LAT:])
    _launch_rdb(blocks[2], bufs[2], bufs[1], bufs[0], b, h, w)
    _check_rdb(blocks[2], bufs[2], bufs[1], bufs[0], b, h, w, "rdb3")
    assert torch.equal(bufs[0][:, :LAT].cpu(), inp), "the RRDB's input changed"
    assert torch.equal(_bits(bufs[1][:, LAT:]), tail1), "the third block wrote past the first 64 channels of its output buffer"
    # and against the reference's expression end to end in fp64, as a whole.  The bound is one bf16 spacing, 2^-8 relative: the last
    # store alone rounds by up to 2^-9 of each element, and what the fourteen earlier stores add reaches the output through
    # `* 0.2` once (the outputs of blocks 1 and 2) or twice and a convolution (net1 .. net4), so it stays below a second 2^-9.
    x = inp.double().view(b, h, w, LAT).permute(0, 3, 1, 2)
    net = x
    for filters in blocks:
        feats = [net]
        for i in range(4):
            feats.append(F.leaky_relu(F.conv2d(torch.cat(feats, 1), filters[i][0].double(), filters[i][1].double(), padding=1), 0.2))
        net = F.conv2d(torch.cat(feats, 1), filters[4][0].double(), filters[4][1].double(), padding=1) * 0.2 + net
    want = _rows(net * 0.2 + x)
    assert rel_l2(bufs[1][:, :LAT].float(), want) < 2.0 ** -8, "the RRDB as a whole is off by more than one bf16 rounding"


# ---------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------


def _module(rec):
    net = C.RRDBNet(**rec["kwargs"])
    fill_parameters(net, rec["seed"])
    return net.to(DEV).eval()


@pytest.mark.parametrize("index", [0, 1, 2], ids=["x4", "x2", "x1"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_module_against_the_reference(fixture, index, dtype):
    rec = fixture["configs"][index]
    net = _module(rec)
    x = rec["x"].to(DEV).to(dtype)
    out = net.upscale(x)
    assert out.dtype == F32 and tuple(out.shape) == tuple(rec["y"].shape)
    yard = rel_l2(rec["y_bf16"], rec["y"])
    got = rel_l2(out, rec["y"])
    print(f"{rec['name']} {dtype}: rel_l2(out, y) {got:.3e}, rel_l2(y_bf16, y) {yard:.3e}")
    if dtype == F32:
        assert got <= YARDSTICK * yard, f"{rec['name']}: rel-L2 {got:.3e} > {YARDSTICK} x {yard:.3e}"
    else:  # a bf16 input is the same net on the rounded image: the bound holds against the reference's run on what it was given
        same = net.upscale(x.float())
        assert torch.equal(out, same), "a bf16 input and the same values as f32 must give the same bits"


def test_launch_discipline_and_determinism(fixture, monkeypatch):
    rec = fixture["configs"][0]
    net = _module(rec)
    layers = rec["kwargs"]["num_layers"]
    x = rec["x"].to(DEV)
    calls = dict(conv=0, pack=0)
    real_conv, real_pack, real_cat = ops.conv3x3_dense, ops.conv3x3_dense_pack, torch.cat

    def conv(*a, **k):
        calls["conv"] += 1
        return real_conv(*a, **k)

    def pack(*a, **k):
        calls["pack"] += 1
        return real_pack(*a, **k)

    def no_cat(*a, **k):
        raise AssertionError("torch.cat called during RRDBNet.forward")

    monkeypatch.setattr(ops, "conv3x3_dense", conv)
    monkeypatch.setattr(ops, "conv3x3_dense_pack", pack)
    monkeypatch.setattr(torch, "cat", no_cat)
    first = net.upscale(x)
    assert calls == dict(conv=15 * layers + 6, pack=15 * layers + 6)
    calls.update(conv=0, pack=0)
    second = net.upscale(x)
    assert calls == dict(conv=15 * layers + 6, pack=0), "a second forward with unchanged weights must not repack"
    assert torch.equal(first, second), "two runs differ"
    monkeypatch.setattr(torch, "cat", real_cat)

    # eager against a captured graph
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.upscale(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = net.upscale(static_x)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, first), "the graph replay differs from the eager run"

    # an in-place change of one body convolution repacks that layer and changes the output
    calls.update(conv=0, pack=0)
    with torch.no_grad():
        net.body[1].rdb2.conv3.weight.mul_(0.5)
    third = net.upscale(x)
    assert calls["pack"] == 1 and not torch.equal(third, first)

    # load_state_dict of the seeded state into a fresh module reproduces the first output bit for bit
    fresh = C.RRDBNet(**rec["kwargs"])
    fresh.load_state_dict(seeded_state(fresh, rec["seed"]))
    fresh = fresh.to(DEV)
    assert torch.equal(fresh.upscale(x), first)
    # ... and into the changed module: every layer whose version moved is repacked
    calls.update(conv=0, pack=0)
    net.load_state_dict(seeded_state(fresh, rec["seed"]))
    assert torch.equal(net.upscale(x), first) and calls["pack"] == 15 * layers + 6
