"""Host-side checks of the VQ first stage (no device): the C entry points of csrc/vq.hip and their refusals, the state-dict keys
of AttentionAutoEncoderVQ (and that the KL class kept its own), and the fixtures of tools/gen_vq_golden.py against a regeneration."""
import os
import sys

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = ("cfhip_vq_code_sqnorm", "cfhip_vq_nearest", "cfhip_vq_chunk")
P = 4096  # a non-null, aligned "pointer": every call below is refused before anything could read it


def _refused(rc, *words):
    msg = _lib.load().cfhip_last_error()
    assert rc == _lib.DEFINES["CFHIP_ERR_INVALID"], rc
    assert msg and all(w.encode() in msg for w in words), msg


def test_vq_entry_points_are_exported_and_declared():
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert not _lib.ctypes_only(name)
    assert _lib.DEFINES["CFHIP_VQ_MAX_DIM"] == 64 and C.ops.VQ_MAX_DIM == 64
    header = open(_lib.HEADER_PATH).read()
    for cite in ("modules/cv/common.py:362-400", "cv/ae/vq.py:63-67", "ldm.py:183-190"):
        assert cite in header, f"cfhip.h does not cite {cite}"
    sources = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert " vq;" in sources or " vq " in sources
    import __graft_entry__ as entry

    assert "vq" in entry.SOURCES


def test_vq_chunk_query():
    """codes held in LDS at once: CFHIP_VQ_LDS_FLOATS floats of [sq, e_0 .. e_(D'-1)] records on a stride rounded up to 4 floats
    (D' = D up to 4, else the next power of two), rounded down to a multiple of the four waves that share a chunk"""
    lib = _lib.load()
    floats = _lib.DEFINES["CFHIP_VQ_LDS_FLOATS"]
    assert floats == 8192
    for d, stride in ((1, 4), (2, 4), (3, 4), (4, 8), (5, 12), (8, 12), (9, 20), (16, 20), (17, 36), (32, 36), (33, 68), (64, 68)):
        assert lib.cfhip_vq_chunk(d) == C.ops.vq_chunk(d) == floats // stride // 4 * 4, d
    assert lib.cfhip_vq_chunk(0) == 0 and lib.cfhip_vq_chunk(65) == 0 and lib.cfhip_vq_chunk(-3) == 0


def _nearest(z=P, cb=P, sq=P, idx=P, zq=P, b=1, d=4, hw=16, n=8):
    return _lib.load().cfhip_vq_nearest(z, 0, 0, cb, sq, idx, zq, b, d, hw, n, 1.0, None)


def test_vq_nearest_refusals():
    for null in ("z", "cb", "sq", "idx"):
        _refused(_nearest(**{null: None}), "vq_nearest", "null")
    _refused(_nearest(n=0), "vq_nearest", "N = 0")
    _refused(_nearest(n=-1), "vq_nearest", "N = -1")
    _refused(_nearest(d=0), "vq_nearest", "D = 0")
    _refused(_nearest(d=65), "vq_nearest", "D = 65", "64")
    _refused(_nearest(b=0), "vq_nearest", "empty")
    _refused(_nearest(hw=0), "vq_nearest", "empty")
    _refused(_nearest(idx=P + 4), "vq_nearest", "misaligned")
    _refused(_nearest(z=P + 1), "vq_nearest", "misaligned")
    _refused(_nearest(zq=P + 2), "vq_nearest", "misaligned")


def test_vq_code_sqnorm_refusals():
    f = _lib.load().cfhip_vq_code_sqnorm
    _refused(f(None, P, 8, 4, None), "vq_code_sqnorm", "null")
    _refused(f(P, None, 8, 4, None), "vq_code_sqnorm", "null")
    _refused(f(P, P, 0, 4, None), "vq_code_sqnorm", "N = 0")
    _refused(f(P, P, 8, 0, None), "vq_code_sqnorm", "D = 0")
    _refused(f(P, P, 8, 65, None), "vq_code_sqnorm", "D = 65")
    _refused(f(P + 2, P, 8, 4, None), "vq_code_sqnorm", "misaligned")


def test_ops_refuse_before_any_launch():
    """the host wrappers' own checks need no device: a CPU tensor is refused by name"""
    with pytest.raises(RuntimeError, match="HIP device"):
        C.ops.vq_nearest(torch.zeros(1, 4, 2, 2), torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        C.ops.vq_code_sqnorm(torch.zeros(8, 4))


SMALL_KL = dict(img_size=16, in_channels=3, out_channels=3, inner_channels=32, latent_channels=4, channel_multipliers=(1, 2),
                embedding_channels=4, num_res_blocks=1, attention_resolutions=(8,))
SMALL_VQ = dict(SMALL_KL, num_codes=64)


def test_state_dict_keys_and_construction():
    g = torch.load(os.path.join(GOLDEN, "ae_vq_keys.pt"), weights_only=False)
    assert g["cfg"] == SMALL_VQ
    m = C.AttentionAutoEncoderVQ(**SMALL_VQ)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in g["keys"]]
    assert "codebook.embedding.weight" in m.state_dict() and tuple(m.codebook.embedding.weight.shape) == (64, 4)
    assert tuple(m.to_embedding.weight.shape) == (4, 4, 1, 1)  # enc_double_channels = False: no doubled moments
    assert m.z_size == 8 and m.embedding_channels == 4 and not m.enc_double_channels
    assert isinstance(m.codebook, C.VQCodebook) and m.codebook.num_codes == 64 and m.codebook.code_dimension == 4
    w = m.codebook.embedding.weight
    assert float(w.detach().abs().max()) <= 1.0 / 64 and float(w.detach().std()) > 0.25 / 64  # uniform(-1 / N, 1 / N)
    assert all(p.device.type == "cpu" for p in m.parameters())
    out = C.VQCodebookOut(torch.zeros(1), torch.ones(1), torch.zeros(1, dtype=torch.int64))
    assert out.z_q_g is None and list(out.to_dict()) == ["z_e", "z_q", "indices", "z_q_g"]
    # one constructor body for both autoencoders
    assert C.AttentionAutoEncoderKL.__init__ is C.modules._AttentionAutoEncoder.__init__
    assert issubclass(C.AttentionAutoEncoderVQ, C.modules._AttentionAutoEncoder)


def test_kl_class_keeps_its_keys():
    g = torch.load(os.path.join(GOLDEN, "ae_kl_keys.pt"), weights_only=False)
    assert g["cfg"] == SMALL_KL
    m = C.AttentionAutoEncoderKL(**SMALL_KL)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in g["keys"]]
    assert m.enc_double_channels and tuple(m.to_embedding.weight.shape) == (8, 8, 1, 1)
    vq_keys = [k for k, _ in torch.load(os.path.join(GOLDEN, "ae_vq_keys.pt"), weights_only=False)["keys"]]
    assert sorted(set(vq_keys) - set(m.state_dict())) == ["codebook.embedding.weight"] and not set(m.state_dict()) - set(vq_keys)


def test_codebook_refuses_a_grad_requiring_input_before_any_launch():
    cb = C.VQCodebook(8, 4)
    with pytest.raises(NotImplementedError, match="§8"):
        cb(torch.zeros(1, 4, 2, 2, requires_grad=True))


def test_fixtures_match_a_regeneration():
    """the committed fixtures against tools/gen_vq_golden.py run now, in memory, through oracle.refharness"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refharness

    if not refharness.reference_available():
        pytest.skip("the reference tree is not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_vq_golden as gen

    def same(a, b, where, skip=()):
        if isinstance(a, dict):
            assert isinstance(b, dict) and sorted(map(str, a)) == sorted(map(str, b)), where
            for k in a:
                if k not in skip:
                    same(a[k], b[k], f"{where}.{k}")
        elif isinstance(a, torch.Tensor):
            assert a.shape == b.shape and a.dtype == b.dtype, where
            if not a.is_floating_point():
                assert torch.equal(a, b), where
            elif "_bf16" in where:  # the reference's bf16 run: another CPU's kernels may round a bf16 intermediate the other way
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
    assert sorted(fresh) == ["ae_vq_keys.pt", "ae_vq_small.pt"]
    same(fresh["ae_vq_keys.pt"], torch.load(os.path.join(GOLDEN, "ae_vq_keys.pt"), weights_only=False), "ae_vq_keys.pt")
    committed = torch.load(os.path.join(GOLDEN, "ae_vq_small.pt"), weights_only=False)
    assert sorted(fresh["ae_vq_small.pt"]) == sorted(committed) == ["e3", "e4"]
    # what follows the bf16 run's choice of codes (another CPU's bf16 kernels may move a pixel or two of that run across a code
    # boundary; the fp32 run's indices are pinned exactly): compared only where that choice came out the same
    follows = ("indices_bf16", "z_q_bf16", "decoded_bf16", "z_q_g_bf16", "flips_bf16")
    for key, rec in committed.items():
        now = fresh["ae_vq_small.pt"][key]
        moved = int((now["indices_bf16"] != rec["indices_bf16"]).sum())
        assert moved <= 2, (key, moved)
        same(now, rec, f"ae_vq_small.pt.{key}", skip=follows if moved else ())
        pixels = rec["indices"].numel()
        assert rec["flips_bf16"] == int((rec["indices"] != rec["indices_bf16"]).sum()) == gen.SEED_TRIALS[key][gen.SEEDS[key]]
        assert 1 <= rec["flips_bf16"] <= pixels * 5 // 100, (key, rec["flips_bf16"])
        assert rec["seed"] == gen.SEEDS[key] and rec["cfg"] == gen.CONFIGS[key]
