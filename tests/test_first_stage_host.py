"""Host-side checks of the first-stage path (no device): the new C entry points and their argument checks, the registry names
and state-dict keys of the KL autoencoder, and the fixtures of tools/gen_first_stage_golden.py against a regeneration."""
import os
import sys

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = ("cfhip_attn_wide_fwd", "cfhip_gaussian_posterior", "cfhip_conv_im2row_pad", "cfhip_conv_row2im_pad")
P = 4096  # a non-null, aligned "pointer": every call below is refused before anything could read it


def test_new_entry_points_are_exported_and_declared():
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert not _lib.ctypes_only(name)  # served by the vectorcall module like the other launches
    assert _lib.DEFINES["CFHIP_ATTN_WIDE_MAX_HEAD_DIM"] == 512 and _lib.DEFINES["CFHIP_ATTN_WIDE_CHUNK"] == 64
    header = open(_lib.HEADER_PATH).read()
    for cite in ("attentions.py:330-370", "cv/ae/kl.py", "cv/encoder/attn.py:14-28", "ldm.py:183-190"):
        assert cite in header, f"cfhip.h does not cite {cite}"


def _wide(q=P, k=P, v=P, o=P, lse=None, b=1, h=1, tq=4, tk=4, dh=256, st=None):
    st = h * dh if st is None else st
    return _lib.load().cfhip_attn_wide_fwd(q, k, v, o, lse, b, h, tq, tk, dh, tq * st, st, tk * st, st, tq * st, st, 0.0625, None)


def _refused(rc, *words):
    msg = _lib.load().cfhip_last_error()
    assert rc == -1, rc
    assert msg and all(w.encode() in msg for w in words), msg


def test_attn_wide_argument_checks():
    for null in ("q", "k", "v", "o"):
        _refused(_wide(**{null: None}), "null")
    for dh in (192, 520, 260):
        _refused(_wide(dh=dh), "head_dim", str(dh))
    for zero in ("b", "h", "tq", "tk"):
        _refused(_wide(**{zero: 0}), "empty")
    _refused(_wide(st=252), "stride")       # not a multiple of 8 elements
    _refused(_wide(h=2, st=256), "stride")  # a token stride below H * head_dim
    _refused(_wide(q=P + 8), "aligned")
    # the dispatcher's entry keeps its own limit (tests/test_capi.py::test_version_and_error_string) and the plan keeps raising
    with pytest.raises(RuntimeError):
        C.ops.attn_plan(16, 16, head_dim=20)
    with pytest.raises(RuntimeError):
        C.ops.attn_plan(16, 16, head_dim=256)


def test_gaussian_posterior_argument_checks():
    f = _lib.load().cfhip_gaussian_posterior
    _refused(f(None, 0, P, None, None, 0, 1, 4, 16, 1.0, 0, 0, None), "null")
    _refused(f(P, 0, None, None, None, 0, 1, 4, 16, 1.0, 0, 0, None), "neither")
    for b, e, hw in ((0, 4, 16), (1, 0, 16), (1, 4, 0)):
        _refused(f(P, 0, P, None, None, 0, b, e, hw, 1.0, 0, 0, None), "empty")
    _refused(f(P, 0, P, None, P, 1, 1, 4, 16, 1.0, 0, 0, None), "deterministic")
    _refused(f(P, 0, P + 2, None, None, 0, 1, 4, 16, 1.0, 0, 0, None), "misaligned")


def test_padded_gather_argument_checks():
    lib = _lib.load()
    for name in ("cfhip_conv_im2row_pad", "cfhip_conv_row2im_pad"):
        f = getattr(lib, name)
        lead = (None, 0, P) if name.endswith("im2row_pad") else (None, P)
        _refused(f(*lead, 1, 8, 8, 8, 3, 3, 2, 0, 1, 0, 1, 1, 72, None), "null")
        lead = (P, 0, P) if name.endswith("im2row_pad") else (P, P)
        _refused(f(*lead, 0, 8, 8, 8, 3, 3, 2, 0, 1, 0, 1, 1, 72, None), "geometry")    # zero batch
        _refused(f(*lead, 1, 8, 8, 8, 3, 3, 2, 0, -1, 0, 1, 1, 72, None), "geometry")   # negative high padding
        _refused(f(*lead, 1, 8, 1, 1, 3, 3, 2, 0, 1, 0, 1, 1, 72, None), "empty output")
        _refused(f(*lead, 1, 8, 8, 8, 3, 3, 2, 0, 1, 0, 1, 1, 64, None), "padded K")


SMALL = dict(img_size=16, in_channels=3, out_channels=3, inner_channels=32, latent_channels=4, channel_multipliers=(1, 2),
             embedding_channels=4, num_res_blocks=1, attention_resolutions=(8,))


def test_registry_names_and_state_dict_keys():
    reg = C.registry
    assert reg.generators.has("ae_kl") and reg.encoders.has("attention") and reg.decoders.has("attention")
    assert not reg.generators.has("ae_vq")
    m = reg.generators.build("ae_kl", config=dict(SMALL, no_such_keyword=1))  # safe_execute drops what the constructor does not take
    assert isinstance(m, C.AttentionAutoEncoderKL) and m.z_size == 8 and m.embedding_channels == 4
    assert isinstance(m.generator.encoder, C.AttentionEncoder) and isinstance(m.generator.decoder, C.AttentionDecoder)
    assert all(p.device.type == "cpu" for p in m.parameters())
    g = torch.load(os.path.join(GOLDEN, "ae_kl_keys.pt"), weights_only=False)
    assert g["cfg"] == SMALL
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in g["keys"]]
    attn = C.make_attention(64, "spatial", num_groups=16, no_such_keyword=1)
    assert isinstance(attn, C.SpatialAttention) and attn.group_norm.num_groups == 16
    assert sorted(attn.state_dict()) == sorted(f"{n}.{p}" for n in ("group_norm", "to_q", "to_k", "to_v", "to_out") for p in ("weight", "bias"))
    assert tuple(attn.to_q.weight.shape) == (64, 64, 1, 1)
    assert isinstance(C.make_attention(64, "none"), torch.nn.Identity)
    for kind in ("cross", "multi_head_spatial", "linear_depth_wise"):
        with pytest.raises(NotImplementedError, match=kind):
            C.make_attention(64, kind)
    with pytest.raises(ValueError):
        C.make_attention(64, "no_such_attention")
    enc = reg.encoders.build("attention", config=dict(img_size=16, in_channels=3, inner_channels=32, latent_channels=8, channel_multipliers=(1, 2),
                                                       num_res_blocks=1, downsample_with_conv=False, out_channels=3))
    assert any(isinstance(b, C.modules.Downsample) and b.conv is None for b in enc.encoder)


def test_fixtures_match_a_regeneration():
    """the committed fixtures against tools/gen_first_stage_golden.py run now, in memory, through oracle.refharness — a stale fixture
    shows up here"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refharness

    if not refharness.reference_available():
        pytest.skip("the reference tree is not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_first_stage_golden as gen

    def same(a, b, where):
        if isinstance(a, dict):
            assert isinstance(b, dict) and sorted(map(str, a)) == sorted(map(str, b)), where
            for k in a:
                same(a[k], b[k], f"{where}.{k}")
        elif isinstance(a, torch.Tensor):
            assert a.shape == b.shape, where
            if "_bf16" in where:  # the reference's bf16 run: another CPU's kernels may round a bf16 intermediate the other way
                assert float((a - b).norm() / b.norm()) < 5e-3, where
            else:
                assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), where
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), where
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{where}[{i}]")
        else:
            assert a == b, where

    threads = torch.get_num_threads()
    try:
        fresh = gen.generate()  # (single-threaded)
    finally:
        torch.set_num_threads(threads)
    for name, data in fresh.items():
        same(data, torch.load(os.path.join(GOLDEN, name), weights_only=False), name)


def test_gaussian_distribution_plain_torch_forms():
    """what stays plain torch, off the training path: the moments' views, `kl(other)` and `nll`, against the formulas in float64
    (reference cv/ae/kl.py:18-63); a deterministic distribution has zero spread and zero kl / nll"""
    g = torch.Generator().manual_seed(5)
    a, b = (C.GaussianDistribution((torch.randn((2, 8, 3, 3), generator=g) * 3).bfloat16()) for _ in range(2))
    m1, l1 = a.net[:, :4].double(), a.net[:, 4:].double().clamp(-30, 20)
    m2, l2 = b.net[:, :4].double(), b.net[:, 4:].double().clamp(-30, 20)
    assert torch.equal(a.mean.double(), m1) and torch.equal(a.log_var.double(), l1)
    assert torch.allclose(a.std.double(), (0.5 * l1).exp(), rtol=1e-6) and torch.allclose(a.var.double(), l1.exp(), rtol=1e-6)
    want = 0.5 * ((m1 - m2) ** 2 / l2.exp() + l1.exp() / l2.exp() - 1 - l1 + l2).sum(dim=(1, 2, 3))
    assert torch.allclose(a.kl(b).double(), want, rtol=1e-5)
    x = torch.randn((2, 4, 3, 3), generator=g)
    want = 0.5 * (torch.log(torch.tensor(2 * torch.pi, dtype=torch.float64)) + l1 + (x.double() - m1) ** 2 / l1.exp()).sum(dim=(1, 2, 3))
    assert torch.allclose(a.nll(x).double(), want, rtol=1e-5)
    d = C.GaussianDistribution(a.net, deterministic=True)
    assert float(d.std.abs().max()) == 0.0 and float(d.kl()) == 0.0 and float(d.nll(x)) == 0.0
