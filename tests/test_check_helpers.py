"""CPU self-tests of the per-element and guard helpers (tests/helpers.py): they show the gap a whole-tensor
rel-L2 leaves and that the per-element check and the guarded allocations close it.  No GPU needed."""
import pytest
import torch

from helpers import GuardedOps, assert_close, assert_elementwise, guarded_ops, ulp_out


def test_one_wrong_element_passes_rel_l2_but_not_elementwise():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1_000_000, generator=g, dtype=torch.float64)
    got = ref.to(torch.bfloat16)
    got[654_321] += 1.0
    assert_close(got, ref, 4e-3, "one wrong element")  # the whole-tensor norm does not see it
    with pytest.raises(AssertionError, match=r"(?s)1 of 1000000 elements out of bound.*\[654321\]"):
        assert_elementwise(got, ref, out_dtype=torch.bfloat16, what="one wrong element")


def test_correctly_rounded_bf16_passes_at_one_ulp():
    g = torch.Generator().manual_seed(1)
    ref = torch.cat([torch.randn(100_000, generator=g, dtype=torch.float64) * 10.0 ** e for e in (-30, -3, 0, 3, 30)])
    ref = torch.cat([ref, torch.tensor([0.0, -0.0, 1e-40, 2.0 ** -126, 65504.0, 3.3e38])])
    assert_elementwise(ref.to(torch.bfloat16), ref, out_dtype=torch.bfloat16, ulps=1.0, what="bf16 RNE")
    assert_elementwise(ref.to(torch.float32), ref, out_dtype=torch.float32, ulps=1.0, what="f32 RNE")
    # ... and one ulp more than that does not
    bad = ref.to(torch.bfloat16).double()
    bad[7] += 2 * ulp_out(ref[7:8].abs(), torch.bfloat16)[0]
    with pytest.raises(AssertionError, match=r"\[7\]"):
        assert_elementwise(bad, ref, out_dtype=torch.bfloat16, ulps=1.0)


def test_ulp_spacing():
    u = ulp_out(torch.tensor([1.0, 1.5, 2.0, 3.99, 0.0, 1e-300]), torch.bfloat16)
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133]
    assert ulp_out(torch.tensor([1.0]), torch.float32).item() == 2.0 ** -23


def test_accumulation_term():
    ref = torch.tensor([0.0], dtype=torch.float64)
    got = torch.tensor([3e-6])
    with pytest.raises(AssertionError):
        assert_elementwise(got, ref, out_dtype=torch.float32)
    # an f32 sum of 100 terms of size 1 may be off by ~100 * 2^-24
    assert_elementwise(got, ref, out_dtype=torch.float32, cond=torch.tensor([100.0]), k=100)


def test_nan_and_inf_positions_must_match():
    ref = torch.tensor([1.0, 2.0, float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
    assert_elementwise(ref.float(), ref, out_dtype=torch.float32)
    for i, v in ((0, float("nan")), (2, 3.0), (3, -float("inf")), (4, 1e30), (1, float("inf"))):
        got = ref.float().clone()
        got[i] = v
        with pytest.raises(AssertionError, match=rf"\[{i}\]"):
            assert_elementwise(got, ref, out_dtype=torch.float32)


def _past(t, at):
    """a one-element view of t's storage at flat element `at` (may lie outside t itself)"""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + at)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("where", [-1, "end"])
def test_write_outside_a_guarded_allocation_fails_check(dtype, where):
    g = GuardedOps()
    t = g.empty((5, 3), dtype=dtype)
    assert t.data_ptr() % 256 == 0
    if t.is_floating_point():
        assert torch.isnan(t.float()).all()
    t.fill_(1)
    g.check()  # writing the interior is fine
    t = g.empty(5, 3, dtype=dtype)
    _past(t, t.numel() if where == "end" else -1).fill_(1)
    with pytest.raises(AssertionError, match=r"(?s)\(5, 3\).*first at byte offset " + ("-" if where == -1 else "")):
        g.check()


def test_unwritten_element_of_a_guarded_empty_shows_as_nan():
    g = GuardedOps()
    out = g.empty((1000,), dtype=torch.float32)
    ref = torch.arange(1000, dtype=torch.float64)
    out[:999] = ref[:999].float()  # a kernel that forgets its last element
    g.check()
    with pytest.raises(AssertionError, match=r"(?s)1 of 1000 elements out of bound.*\[999\] got nan"):
        assert_elementwise(out, ref, out_dtype=torch.float32)


def test_zeros_and_empty_like():
    g = GuardedOps()
    z = g.zeros((7,), dtype=torch.float32)
    assert torch.equal(z, torch.zeros(7))
    e = g.empty_like(torch.ones(3, 4, dtype=torch.bfloat16))
    assert e.shape == (3, 4) and e.dtype == torch.bfloat16 and torch.isnan(e.float()).all()
    g.check()


def test_poisoned_input_reads_past_the_end_see_nan():
    g = GuardedOps()
    x = g.poisoned(torch.arange(10, dtype=torch.float32))
    assert torch.equal(x, torch.arange(10, dtype=torch.float32)) and x.data_ptr() % 256 == 0
    assert torch.isnan(_past(x, 10)).all() and torch.isnan(_past(x, -1)).all()
    idx = g.index(torch.tensor([3, 1, 2]))
    assert _past(idx, 3).item() == 0 and _past(idx, -1).item() == 0
    g.check()
    x = g.poisoned(torch.arange(10, dtype=torch.float32))
    _past(x, 11).fill_(0.0)  # an input's guards are checked for writes as well
    with pytest.raises(AssertionError, match="input"):
        g.check()


def test_out2d_padding_and_guard_rows():
    g = GuardedOps()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    assert out.shape == (4, 5) and out.stride() == (8, 1)
    out.fill_(0.5)
    g.check()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    _past(out, 5).fill_(0.5)  # a column store past N (ldc > N)
    with pytest.raises(AssertionError, match="out2d 4x5 ld 8"):
        g.check()
    out = g.out2d(4, 5, 8, torch.float32, "cpu")
    _past(out, 4 * 8).fill_(0.5)  # the row after the last
    with pytest.raises(AssertionError, match="out2d"):
        g.check()


def test_region_with_sentinel_gaps():
    g = GuardedOps()
    a, b = g.region((10, 4), torch.float32, "cpu", lambda w: (w[1:4], w[6:9]))
    a.fill_(1.0)
    b.fill_(2.0)
    g.check()
    a, b = g.region((10, 4), torch.float32, "cpu", lambda w: (w[1:4], w[6:9]))
    _past(a, 12).fill_(1.0)  # problem a writes one row into the gap
    with pytest.raises(AssertionError, match="region"):
        g.check()


def test_guarded_ops_patches_only_ops_torch(monkeypatch):
    from cflearn_amd import functional, ops

    g = guarded_ops(monkeypatch)
    assert ops.torch.empty is not torch.empty and ops.torch.bfloat16 is torch.bfloat16
    assert functional.torch is torch
    t = ops.torch.empty((2, 3), dtype=torch.float32, device="cpu")
    assert torch.isnan(t).all() and len(g.allocs) == 1
    g.check()
