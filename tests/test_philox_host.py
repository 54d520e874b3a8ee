"""The host reference of the random stream (tests/philox_ref.py) against what is known from outside this project, on the
CPU: the Random123 known-answer vectors of Philox4x32-10, the edge counters the GPU tests use (they hold the words they
are named for), the error bound of the normal test (an f32 evaluation of the Box-Muller formula stays inside it), and the
stream helpers' own consistency.  test_gpu_philox.py then pins every Philox-drawing kernel to this reference."""
import numpy as np
import torch

import philox_ref as R
from helpers import assert_elementwise
from philox_ref import ONES_WORDS, SEED, ZERO_WORDS, ZERO_WORDS_A


def test_known_answer_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter words, key words -> output words"""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in kat:
        got = R.philox4x32_10_words(*ctr, *key)
        assert got.dtype == np.uint32 and got.shape == (1, 4)
        assert tuple(int(v) for v in got[0]) == want, (ctr, key, [hex(int(v)) for v in got[0]])
    # the 64-bit entry is the same function with the device's word mapping
    assert np.array_equal(R.philox4x32_10([0], 0), R.philox4x32_10_words(0, 0, 0, 0, 0, 0))
    ctr = np.array([5, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 64 - 1], dtype=np.uint64)
    want = R.philox4x32_10_words(ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), 0, 0, SEED & 0xFFFFFFFF, SEED >> 32)
    assert np.array_equal(R.philox4x32_10(ctr, SEED), want)
    assert not np.array_equal(R.philox4x32_10([2 ** 32], SEED), R.philox4x32_10([0], SEED))  # the counter's high word counts
    assert not np.array_equal(R.philox4x32_10([0], SEED), R.philox4x32_10([0], SEED & 0xFFFFFFFF))  # and the key's


def test_edge_counters_hold_what_they_are_named_for():
    for c, w in ZERO_WORDS + ZERO_WORDS_A:
        assert int(R.philox4x32_10([c], SEED)[0, w]) >> 8 == 0, (c, w)
    for c, w in ONES_WORDS:
        assert int(R.philox4x32_10([c], SEED)[0, w]) >> 8 == 0xFFFFFF, (c, w)
    assert all(w in (0, 2) for _, w in ZERO_WORDS_A)
    assert {w % 2 for _, w in ONES_WORDS} == {0, 1}  # u = 1 both as u_a (radius 0) and as u_b (angle 2 pi)
    # what the helpers make of them
    for c, w in ZERO_WORDS + ZERO_WORDS_A:
        assert R.dropout_keep(4, 0.0, SEED, c)[w] == 1 and R.dropout_keep(4, 2.0 ** -24, SEED, c)[w] == 0
    for c, w in ONES_WORDS:
        assert R.dropout_keep(4, 0.999, SEED, c)[w] == 1
        z, rad = R.normals64(4, SEED, c)
        if w % 2 == 0:
            assert rad[w] == 0.0 and z[w] == 0.0 and z[w + 1] == 0.0
        else:
            assert abs(z[w]) <= 1e-15 * rad[w] and z[w - 1] == rad[w]
    z, rad = R.normals64(4, SEED, ZERO_WORDS_A[0][0])
    assert rad[ZERO_WORDS_A[0][1]] == np.sqrt(-2.0 * np.log(2.0 ** -24)) and np.isfinite(z).all()


def test_f32_box_muller_stays_inside_the_gpu_tests_bound():
    """The bound of test_gpu_philox's normal test, |z - z64| <= ulp_f32(|z64|) + 8 * 2^-24 * rad, holds for a plain numpy
    float32 evaluation of the same formula whose angle 2 pi u is ROUNDED to f32 (the kernel's sincospif never forms it):
    the bound asks nothing a careful f32 implementation cannot give."""
    n = 4 << 20
    z64, rad = R.normals64(n, SEED, 0)
    w = R.philox4x32_10(R.counters(0, n // 4), SEED)
    u = (((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)  # exact
    z = np.empty(u.shape, dtype=np.float32)
    for a in (0, 2):
        r = np.sqrt(np.float32(-2.0) * np.log(u[:, a]))
        ang = np.float32(2.0 * np.pi) * u[:, a + 1]
        assert r.dtype == np.float32 and ang.dtype == np.float32
        z[:, a], z[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
    z = z.reshape(-1)
    units = (np.abs(z.astype(np.float64) - z64) - np.spacing(np.abs(z64).astype(np.float32)).astype(np.float64)) / (2.0 ** -24 * np.maximum(rad, 1e-300))
    print(f"f32 Box-Muller over {n} normals: worst excess over 1 ulp = {units.max():.2f} units of 2^-24 rad (8 allowed)")
    assert_elementwise(torch.from_numpy(z), torch.from_numpy(z64), out_dtype=torch.float32, ulps=1, cond=torch.from_numpy(rad), k=8,
                       what="numpy f32 Box-Muller")


def test_stream_helpers_are_self_consistent():
    for off in (0, 7, 2 ** 32 - 2, 2 ** 40 + 5):
        for p in (0.0, 0.3, 0.9):
            full = R.dropout_keep(23, p, SEED, off)
            assert np.array_equal(full[4:], R.dropout_keep(19, p, SEED, off + 1))
            assert np.array_equal(full[:5], R.dropout_keep(5, p, SEED, off))
        assert R.dropout_keep(4096, 0.0, SEED, off).all()
        assert np.array_equal(R.drop_path_mask(9, 0.5, SEED, off)[4:], R.drop_path_mask(5, 0.5, SEED, off + 1))
        assert (R.drop_path_mask(64, 1.0, SEED, off) == 1.0).all()
        z, rad = R.normals64(11, SEED, off)
        z1, rad1 = R.normals64(7, SEED, off + 1)
        assert np.array_equal(z[4:], z1) and np.array_equal(rad[4:], rad1) and np.array_equal(R.rad64(11, SEED, off), rad)
    m = R.drop_path_mask(4096, 0.8, SEED, 0)
    assert set(np.unique(m)) == {0.0, 1.0} and abs(m.mean() - 0.8) < 5 * np.sqrt(0.16 / 4096)
    # dropout and DropPath read the same word of the same counter: keep (u >= p) and floor(keep_prob + u) agree where exact
    assert np.array_equal(R.drop_path_mask(4096, 0.5, SEED, 3), R.dropout_keep(4096, 0.5, SEED, 3).astype(np.float32))
    # attention: a Tq x Tk that is no multiple of 4 is the corner of the padded one, per (b, h)
    assert [R.attn_thresh(p) for p in (0.001, 0.1, 0.25, 0.5, 0.998, 0.999)] == [1, 26, 64, 128, 255, 255]
    for p in (0.1, 0.5):
        pad = R.attn_keep(2, 3, 8, 12, p, SEED, 7)
        cut = R.attn_keep(2, 3, 5, 10, p, SEED, 7)
        assert pad.shape == (2, 3, 8, 12) and cut.shape == (2, 3, 5, 10)
        # the padded one has the same blocks per row of blocks only when ceil(Tk / 4) agrees: 12 and 10 both give 3
        assert np.array_equal(cut, pad[:, :, :5, :10])
    # entry (b, h, i, j) from first principles
    B, H, Tq, Tk, off = 2, 3, 5, 7, 2 ** 32 - 2
    m = R.attn_keep(B, H, Tq, Tk, 0.25, SEED, off)
    for (b, h, i, j) in ((0, 0, 0, 0), (1, 2, 4, 6), (0, 1, 3, 5), (1, 0, 2, 4)):
        ctr = off + ((b * H + h) * 2 + i // 4) * 2 + j // 4
        word = int(R.philox4x32_10([ctr], SEED)[0, i % 4])
        assert m[b, h, i, j] == int(((word >> (8 * (j % 4))) & 255) >= 64)
