"""Host reference of the library's random stream: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
3", SC'11; the Random123 known-answer vectors are in test_philox_host.py) in 64-bit integer numpy arithmetic, and the
mapping from its words to every random decision the kernels make (csrc/common.h philox4x32_10, csrc/random.hip,
csrc/attn.hip drop_block / attn_dropout_mask_kernel, csrc/sample.hip normal4).  Plain numpy: nothing of the project is
imported, so the GPU tests compare the kernels with an independent statement of what the stream has to be."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF
TWO_M24 = 2.0 ** -24

# Edge words of the stream keyed by SEED, as (counter, word): w >> 8 == 0 (u = 0 for the masks, u = 2^-24 for the normals)
# and w >> 8 == 0xFFFFFF (u = 1 - 2^-24, and u = 1 for the normals), every one there is among counters 0 .. 2^24 - 1, found
# once by a numpy search over that range.  ZERO_WORDS_A: a zero in an even word, the u_a of a Box-Muller pair and so the
# largest radius sqrt(-2 ln 2^-24), the first among counters 2^24 .. 2^25.  test_philox_host.py recomputes each of them.
SEED = 0x123456789ABCDEF0
ZERO_WORDS = [(3967492, 3), (7162423, 3), (9163692, 1)]
ONES_WORDS = [(1040478, 0), (4634497, 2), (5952133, 1), (10075381, 3), (16149446, 3)]
ZERO_WORDS_A = [(22212599, 2)]


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32_10_words(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter words (c0, c1, c2, c3) under the key words (k0, k1): arrays (or scalars) of 32-bit
    values held in uint64 -> uint32 [n, 4].  Every product is a 32 x 32 -> 64 bit one: it fits uint64 exactly."""
    c0, c1, c2, c3 = (_u64(c) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def philox4x32_10(ctr_u64, seed_u64):
    """the device function's mapping: counter words (ctr & 0xffffffff, ctr >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32)
    -> uint32 [n, 4]"""
    ctr = _u64(ctr_u64)
    seed = int(seed_u64) & MASK64
    return philox4x32_10_words(ctr & np.uint64(MASK32), ctr >> np.uint64(32), 0, 0, seed & MASK32, seed >> 32)


def counters(first, count):
    """uint64 [count]: first, first + 1, ... modulo 2^64 (the device adds in unsigned long long)"""
    return (np.arange(count, dtype=np.uint64) + np.uint64(int(first) & MASK64)) & np.uint64(MASK64)


def _stream_words(n, seed, offset):
    """element i of a flat stream: word i % 4 of counter offset + i // 4 -> uint32 [n]"""
    return philox4x32_10(counters(offset, (n + 3) // 4), seed).reshape(-1)[:n]


def dropout_keep(n, p, seed, offset):
    """uint8 [n]: keep iff (w >> 8) * 2^-24 >= float32(p).  Both sides are exact in float64."""
    u = (_stream_words(n, seed, offset) >> np.uint32(8)).astype(np.float64) * TWO_M24
    return (u >= np.float64(np.float32(p))).astype(np.uint8)


def drop_path_mask(B, keep_prob, seed, offset):
    """float32 [B]: floor(f32(keep_prob) + u) with the f32 addition's rounding, u = (w >> 8) * 2^-24 (exact in f32)"""
    u = ((_stream_words(B, seed, offset) >> np.uint32(8)).astype(np.float64) * TWO_M24).astype(np.float32)
    return np.floor(np.float32(keep_prob) + u).astype(np.float32)


def attn_thresh(p):
    """the byte threshold of attention dropout: clamp(round_half_even(256 * f32(p)), 1, 255); 256 * f32(p) is exact"""
    return int(min(max(int(np.rint(np.float64(np.float32(p)) * 256.0)), 1), 255))


def attn_keep(B, H, Tq, Tk, p, seed, offset):
    """uint8 [B, H, Tq, Tk]: entry (b, h, i, j) is byte j % 4 (little end first) of word i % 4 of counter
    offset + ((b H + h) ceil(Tq / 4) + i // 4) ceil(Tk / 4) + j // 4; keep iff byte >= thresh"""
    bq, bk = (Tq + 3) // 4, (Tk + 3) // 4
    words = philox4x32_10(counters(offset, B * H * bq * bk), seed).reshape(B, H, bq, bk, 4)  # [.., block row, block col, word]
    shifts = (np.arange(4, dtype=np.uint32) * np.uint32(8)).reshape(1, 1, 1, 1, 1, 4)
    by = (words[..., None] >> shifts) & np.uint32(255)  # [B, H, bq, bk, word = i % 4, byte = j % 4]
    by = by.transpose(0, 1, 2, 4, 3, 5).reshape(B, H, bq * 4, bk * 4)
    return (by[:, :, :Tq, :Tk] >= np.uint32(attn_thresh(p))).astype(np.uint8)


def rad64(n, seed, offset):
    """float64 [n]: the Box-Muller radius sqrt(-2 ln u_a) of each element's pair, u = ((w >> 8) + 1) * 2^-24 in (0, 1]"""
    return normals64(n, seed, offset)[1]


def normals64(n, seed, offset):
    """(z, rad), float64 [n] each: four normals per counter, Box-Muller on the word pairs (w0, w1) and (w2, w3):
    z = sqrt(-2 ln u_a) * (cos(2 pi u_b), sin(2 pi u_b)), evaluated in float64 with u exact"""
    w = philox4x32_10(counters(offset, (n + 3) // 4), seed)
    u = ((w >> np.uint32(8)).astype(np.float64) + 1.0) * TWO_M24
    z = np.empty(u.shape, dtype=np.float64)
    rad = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        ang = 2.0 * np.pi * u[:, a + 1]
        z[:, a], z[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
        rad[:, a] = rad[:, a + 1] = r
    return z.reshape(-1)[:n], rad.reshape(-1)[:n]
