"""Host-side checks of the RRDB upscaler (no device): the registry entry, the default net's state-dict names and shapes against
what tools/gen_rrdb_golden.py recorded from the reference (tests/golden/rrdb_small.pt), the refusals of the C entry points of
csrc/conv_dense.hip (each before any launch, each with its message), the host statement of the reference's pixel_unshuffle, and the
constructor's and the forward's refusals."""
import os

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MB = 1 << 20  # non-null, aligned "pointers" a megabyte apart: every call below is refused before anything could read them
X, WP, BIAS, Y, R1, R2 = (k * 64 * MB for k in range(1, 7))
NONE, LRELU, RES1, RES2 = (ops.DENSE_EPILOGUES[k] for k in ("none", "lrelu", "res1", "res2"))


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(GOLDEN, "rrdb_small.pt"), weights_only=False)


def test_registry_builds_the_module():
    net = C.build_module("rrdb", config=dict(in_channels=3, scale=2, num_layers=1))
    assert isinstance(net, C.RRDBNet) and net.scale == 2 and net.num_layers == 1 and len(net.body) == 1
    assert net.conv_first.weight.shape == (64, 12, 3, 3) and net.conv_last.weight.shape == (3, 64, 3, 3)
    assert all(p.dtype == torch.float32 for p in net.parameters())
    assert C.build_module("rrdb", config=dict(out_channels=5, num_layers=1)).conv_last.bias.shape == (5,)


def test_default_state_dict_is_the_references(G):
    got = [(k, tuple(v.shape)) for k, v in C.RRDBNet().state_dict().items()]
    assert len(got) == 2 * (15 * 23 + 6) and got == [(k, tuple(s)) for k, s in G["default_state"]]
    assert got[2][0] == "body.0.rdb1.conv1.weight" and got[-1] == ("conv_last.bias", (3,))


def test_entry_points_are_declared_built_and_cited():
    lib = _lib.load()
    for name, nargs in (("cfhip_conv3x3_dense_bf16", 23), ("cfhip_pixel_unshuffle_nhwc", 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None and not _lib.ctypes_only(name)
    assert ops.DENSE_EPILOGUES == dict(none=0, lrelu=1, res1=2, res2=3)
    assert ops.DENSE_TILE == (_lib.DEFINES["CFHIP_DENSE_TILE_H"], _lib.DEFINES["CFHIP_DENSE_TILE_W"])
    header = open(_lib.HEADER_PATH).read()
    for cite in ("translator/rrdb.py:15-29", "rrdb.py:39-44", "rrdb.py:77-85", "rrdb.py:47-55", "rrdb.py:88"):
        assert cite in header, f"cfhip.h does not cite {cite}"
    assert " conv_dense " in open(os.path.join(ROOT, "build_lib.sh")).read()
    import __graft_entry__ as entry

    assert "conv_dense" in entry.SOURCES and os.path.isfile(os.path.join(entry.CSRC, "conv_dense.hip"))


def _refused(rc, *words):
    msg = _lib.load().cfhip_last_error()
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"], rc
    assert msg and all(w.encode() in msg for w in words), msg


def _dense(x=X, wp=WP, bias=BIAS, y=Y, r1=None, r2=None, b=1, h=8, w=8, cin=64, n=32, n_store=None, ld_in=192, ld_out=192, ld_r1=64,
           ld_r2=64, epi=NONE, up2=0, f32_out=0):
    return _lib.load().cfhip_conv3x3_dense_bf16(x, wp, bias, y, r1, r2, b, h, w, cin, n, n if n_store is None else n_store, ld_in, ld_out,
                                                ld_r1, ld_r2, epi, 0.2, 0.2, 0.2, up2, f32_out, None)


def test_dense_entry_refuses_bad_arguments_before_any_launch():
    for k in ("x", "wp", "y"):
        _refused(_dense(**{k: None}), "conv3x3_dense_bf16", "null")
    _refused(_dense(cin=60), "Cin = 60", "multiple of 8")
    _refused(_dense(cin=200, ld_in=200), "Cin = 200", "192")
    _refused(_dense(ld_in=196), "ld_in = 196", "multiple of 8")
    _refused(_dense(ld_out=100), "ld_out = 100", "multiple of 8")
    _refused(_dense(cin=96, ld_in=64), "ld_in = 64 < Cin = 96")
    for n in (0, 8, 48, 128):
        _refused(_dense(n=n, n_store=1), f"N = {n}", "16, 32 or 64")
    _refused(_dense(n=16, n_store=17), "n_store = 17", "N = 16")
    _refused(_dense(n=16, n_store=0), "n_store = 0")
    _refused(_dense(epi=4), "unknown epilogue 4")
    _refused(_dense(epi=-1), "unknown epilogue -1")
    _refused(_dense(epi=RES1), "res1", "without its operand r1")
    _refused(_dense(epi=RES2, r1=R1), "res2", "without its operand r2")
    _refused(_dense(epi=RES2, r2=R2), "without its operand r1")
    _refused(_dense(epi=RES1, r1=R1, ld_r1=60), "ld_r1 = 60")
    _refused(_dense(x=X + 8), "misaligned")
    _refused(_dense(y=Y + 2), "misaligned")
    _refused(_dense(b=0), "bad image")
    _refused(_dense(h=1 << 15), "too large")


def test_dense_entry_refuses_overlap_before_any_launch():
    """the output's bytes against everything the call reads.  The dense block's own case — another column range of the same row grid
    — is the one meeting of byte ranges that is let through; it launches, so tests/test_gpu_rrdb.py exercises it, not this file"""
    el = 2
    # the same buffer, columns [32, 64) written while [0, 64) is read
    _refused(_dense(y=X + 32 * el), "output range overlaps the channels [0, 64)")
    # columns [176, 208) wrap into the next row's [0, 16)
    _refused(_dense(y=X + 176 * el), "output range overlaps")
    # y = x
    _refused(_dense(y=X, ld_in=64, ld_out=64, n=64), "output range overlaps")
    # another stride over the same bytes
    _refused(_dense(y=X + 64 * el, ld_out=96), "output range overlaps")
    # the upsampled form has another row grid: any meeting of the byte ranges is refused
    _refused(_dense(y=X + 64 * el, up2=1), "output range overlaps")
    # the f32 NCHW store inside the input buffer
    _refused(_dense(y=X + 4096, n=16, n_store=3, f32_out=1), "output range overlaps")
    # residuals aliasing y, exactly and by a column overlap of the same grid
    _refused(_dense(epi=RES1, r1=Y, ld_r1=192), "overlaps the residual r1")
    _refused(_dense(epi=RES1, r1=Y + 16 * el, ld_r1=192), "overlaps the residual r1")
    _refused(_dense(epi=RES2, r1=R1, r2=Y, ld_r2=192), "overlaps the residual r2")
    _refused(_dense(epi=RES2, r1=R1, r2=Y - 64 * el, ld_r2=96), "overlaps the residual r2")


def test_unshuffle_entry_refuses_bad_arguments():
    lib = _lib.load()
    _refused(lib.cfhip_pixel_unshuffle_nhwc(None, 1, Y, 1, 3, 8, 8, 2, None), "pixel_unshuffle_nhwc", "null")
    _refused(lib.cfhip_pixel_unshuffle_nhwc(X, 1, Y, 1, 3, 8, 8, 3, None), "s = 3")
    _refused(lib.cfhip_pixel_unshuffle_nhwc(X, 1, Y, 1, 3, 8, 6, 4, None), "not divisible")
    _refused(lib.cfhip_pixel_unshuffle_nhwc(X, 1, Y, 0, 3, 8, 8, 2, None), "bad shape")
    _refused(lib.cfhip_pixel_unshuffle_nhwc(X, 1, Y + 4, 1, 3, 8, 8, 2, None), "misaligned")


def test_host_unshuffle_map_is_the_references(G):
    ramp, outs = G["unshuffle"]["ramp"], G["unshuffle"]["out"]
    assert sorted(outs) == [2, 4]
    _, c, h, w = ramp.shape
    for s, want in outs.items():
        m = ops.pixel_unshuffle_map(c, h, w, s)
        assert m.dtype == torch.int64 and tuple(m.shape) == (h // s, w // s, c * s * s)
        got = ramp[0].reshape(-1)[m].permute(2, 0, 1)  # [c s^2, h / s, w / s]
        assert torch.equal(got, want[0]), s
    assert torch.equal(ops.pixel_unshuffle_map(3, 4, 6, 1), torch.arange(72).view(3, 4, 6).permute(1, 2, 0))
    with pytest.raises(ValueError, match="divide"):
        ops.pixel_unshuffle_map(3, 6, 8, 4)


def test_ops_refuse_cpu_tensors_and_bad_operands():
    bf = torch.bfloat16
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.conv3x3_dense_pack(torch.zeros(32, 64, 3, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.pixel_unshuffle_nhwc(torch.zeros(1, 3, 8, 8), 2)
    buf = torch.zeros(64, 192, dtype=bf)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.conv3x3_dense(buf[:, :64], torch.zeros(32, 576, dtype=bf), None, buf[:, 64:96], 1, 8, 8)
    with pytest.raises(ValueError, match="unknown epilogue"):
        ops.conv3x3_dense(buf[:, :64], torch.zeros(32, 576, dtype=bf), None, buf[:, 64:96], 1, 8, 8, epilogue="relu")


def test_constructor_refuses_other_widths():
    with pytest.raises(NotImplementedError, match="latent_channels = 64 with grow_channels = 32"):
        C.RRDBNet(latent_channels=32)
    with pytest.raises(NotImplementedError, match="§8"):
        C.RRDBNet(grow_channels=16)
    with pytest.raises(NotImplementedError, match="192 input"):
        C.RRDBNet(in_channels=16, scale=1, num_layers=1)
    with pytest.raises(ValueError, match="scale = 3"):
        C.RRDBNet(scale=3)
    with pytest.raises(ValueError, match="num_layers"):
        C.RRDBNet(num_layers=0)


def test_forward_refusals_on_the_host():
    net = C.RRDBNet(scale=2, num_layers=1)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="§8"):
        net(x)  # grad mode on, parameters require grad
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="§8"):
        net(x.clone().requires_grad_(True))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP device"):
            net(x)
        with pytest.raises(ValueError, match="divisible by 2"):
            net(torch.zeros(1, 3, 9, 8))
        with pytest.raises(ValueError, match="expected"):
            net(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        net.upscale(x)
    with pytest.raises(ValueError, match="divisible by 4"):
        C.RRDBNet(scale=1, num_layers=1).upscale(torch.zeros(1, 3, 8, 6))
    assert net.training  # upscale restores the mode


def test_fixture_records_what_the_generator_asserted(G):
    assert [r["name"] for r in G["configs"]] == ["x4", "x2", "x1"]
    shapes = {"x4": (2, 3, 12, 20), "x2": (1, 3, 16, 12), "x1": (1, 3, 16, 16)}
    for rec in G["configs"]:
        s = rec["kwargs"]["scale"]
        b, c, h, w = shapes[rec["name"]]
        assert tuple(rec["x"].shape) == (b, c, h, w) and tuple(rec["y"].shape) == tuple(rec["y_bf16"].shape) == (b, 3, h * s, w * s)
        assert rec["kwargs"]["num_layers"] == 2 and 0.25 <= rec["conv_std_min"] <= rec["conv_std_max"] <= 4.0
        assert float((rec["y_bf16"] - rec["y"]).norm() / rec["y"].norm()) >= 1e-3


def test_fixture_matches_a_regeneration(G):
    """the committed fixture against tools/gen_rrdb_golden.py run now, in memory, through oracle.refharness"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refharness

    if not refharness.reference_available():
        pytest.skip("the reference tree is not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rrdb_golden as gen

    threads = torch.get_num_threads()
    try:
        fresh = gen.generate()  # (single-threaded)
    finally:
        torch.set_num_threads(threads)
    assert fresh["default_state"] == G["default_state"]
    assert torch.equal(fresh["unshuffle"]["ramp"], G["unshuffle"]["ramp"])
    for s in (2, 4):
        assert torch.equal(fresh["unshuffle"]["out"][s], G["unshuffle"]["out"][s])
    for now, rec in zip(fresh["configs"], G["configs"]):
        assert now["name"] == rec["name"] and now["kwargs"] == rec["kwargs"] and now["seed"] == rec["seed"]
        assert torch.equal(now["x"], rec["x"])
        assert torch.allclose(now["y"], rec["y"], rtol=1e-4, atol=1e-5), rec["name"]
        # (the reference's bf16 run: another CPU's kernels may round a bf16 intermediate the other way)
        assert float((now["y_bf16"] - rec["y_bf16"]).norm() / rec["y_bf16"].norm()) < 5e-3, rec["name"]
