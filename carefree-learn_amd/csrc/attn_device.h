// Device parts shared by the attention kernels of csrc/attn.hip, of its family files (csrc/attn_resident.hip,
// attn_one_pass.hip) and of csrc/attn_wide.hip: the swizzled [rows][64] bf16 LDS tile, its LDS-DMA fill, the MFMA
// operand fragments read from it or from global memory, the row stores, the mask / dropout predicates, the group reductions of the
// online softmax, the LDS-space pointer types of the kernels that build their own addresses, and the geometry of a staged chunk.
#pragma once
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int DH = CFHIP_ATTN_HEAD_DIM;  // 64

// XOR key of the 16-byte slots of a tile row (128 B per row: two rows per 256-byte LDS bank row).  The key moves whole
// 32-byte chunks (bit 0 clear) and takes four values over the row pairs of an 8-row block: the 16 lanes of a
// ds_read_b128 group (8 rows on each half of the bank row, two adjacent slots) land on 8 distinct slots per half, and the
// 8 rows x 32 bytes a half-wave of ds_read_b64_tr_b16 touches land on 4 distinct chunks per half — both conflict-free.
// (The first version, key (row >> 1) & 7, differed only in bit 0 between rows r and r + 2: the two slots of a 32-byte
// chunk swapped places and every transposing read was a 2-way conflict — SQ_LDS_BANK_CONFLICT 26 % of the LDS cycles.)
__device__ __forceinline__ int swz(int row) { return ((row >> 1) & 3) << 1; }

// byte offset of element (row, col) in a swizzled [rows][64] bf16 tile (128 B per row)
__device__ __forceinline__ int tile_off(int row, int col) {
  return row * 128 + ((((col >> 3) ^ swz(row))) << 4) + ((col & 7) << 1);
}

// row-operand fragment: lane (i = l&15, g = l>>4) <- tile[row0 + i][ks*32 + 8g .. +8]
__device__ __forceinline__ bf16x8 frag_rows(const char* tile, int row0, int ks, int lane) {
  const int row = row0 + (lane & 15);
  const int slot = ks * 4 + (lane >> 4);
  return *reinterpret_cast<const bf16x8*>(tile + row * 128 + ((slot ^ swz(row)) << 4));
}

// two transposing reads (four k-slots each) -> one MFMA operand
__device__ __forceinline__ bf16x8 join8(const s16x4& lo, const s16x4& hi) {
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// the 64-deep product of the 16 tile rows from `row0` with a row operand held as two 32-deep fragments f0, f1
__device__ __forceinline__ f32x4 product64(const char* tile, int row0, const bf16x8& f0, const bf16x8& f1, int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(tile, row0, 0, lane), f0, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(tile, row0, 1, lane), f1, acc, 0, 0, 0);
}

// column-operand fragment over the 32-row block starting at `r32`, columns c0..c0+15:
// lane (n = l&15, g = l>>4) <- { tile[r32 + 4g + e][c0 + n], e = 0..3 ; tile[r32 + 16 + 4g + e][c0 + n] }
// (the k-slot order that the packed S^T / P registers have).
__device__ __forceinline__ bf16x8 frag_cols(const char* tile, int r32, int c0, int lane) {
  const int g = lane >> 4, s = lane & 15;
  const int r_lo = r32 + 4 * g + (s >> 2);
  const int col = c0 + 4 * (s & 3);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + tile_off(r_lo, col)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + tile_off(r_lo + 16, col)));
  return join8(lo, hi);
}

__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  union { bf16x8 v; unsigned w[4]; } u;
  u.w[0] = pack_bf16x2(a[0], a[1]); u.w[1] = pack_bf16x2(a[2], a[3]);
  u.w[2] = pack_bf16x2(b[0], b[1]); u.w[3] = pack_bf16x2(b[2], b[3]);
  return u.v;
}

__device__ __forceinline__ float group_max(float v) {  // across the 4 lanes sharing l & 15
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}

__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// The row walk of every tile fill.  One LDS-DMA instruction (buffer_load_dwordx4 ... lds) = 8 rows x 128 B, no VGPR staging; the LDS
// image of the DMA is lane-linear, so the 16-byte-slot swizzle is applied to the SOURCE address; rows past the end (and everything
// when `live` is false) are range-checked to zero by the buffer descriptor.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dma_rsrc(const bf16_t* base, long stride_t, int rows_valid, int dh, bool live = true) {
  long bytes = ((long)(rows_valid - 1) * stride_t + dh) * 2;
  if (bytes > 0x7fffffffL) bytes = 0x7fffffffL;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, live ? (int)bytes : 0, 0x00020000);
}
// instruction `inst` of the walk: rows 8 inst .. 8 inst + 7 of 64-column half `half` of a head_dim-dh operand
template <bool SKIP_PAD = false>
__device__ __forceinline__ void dma_rows8(const __amdgpu_buffer_rsrc_t& rsrc, char* tile, int inst, long stride_t, int rows_valid,
                                          int half, int dh, int lane, bool live = true) {
  const int r8 = lane >> 3, slot = lane & 7;
  const int row = inst * 8 + r8;
  const int chunk = slot ^ swz(row);
  const bool ok = live && row < rows_valid && half * 64 + chunk * 8 < dh;
  const unsigned off = ok ? (unsigned)(row * stride_t * 2 + half * 128 + chunk * 16) : 0x80000000u;
  if (SKIP_PAD) {
    if (half * 64 + chunk * 8 < dh) lds_dma16(rsrc, tile + inst * 1024, off);  // (rows beyond rows_valid still fetch zeros)
  } else {
    lds_dma16(rsrc, tile + inst * 1024, off);
  }
}

// one 64-column half of `rows_pad` rows -> swizzled [rows][64] tile; columns >= dh and rows >= rows_valid are zero.
// SKIP_PAD: the lanes whose 16-byte chunk lies beyond dh are switched off (EXEC) instead of fetching zeros, so the DMA never
// writes the pad columns of the tile: whatever the kernel put there once (zeros; attn_fwd2_kernel's column of ones) stays.
template <bool SKIP_PAD = false>
__device__ __forceinline__ void dma_half(char* tile, const bf16_t* base, long stride_t, int rows_valid, int rows_pad,
                                         int half, int dh, int wave, int nwaves, int lane) {
  const __amdgpu_buffer_rsrc_t rsrc = dma_rsrc(base, stride_t, rows_valid, dh);
  for (int inst = wave; inst < rows_pad / 8; inst += nwaves) dma_rows8<SKIP_PAD>(rsrc, tile, inst, stride_t, rows_valid, half, dh, lane);
}

// Cooperative asynchronous load of `rows_pad` rows (zero beyond rows_valid) of one head_dim-64 head into a swizzled tile.
// Completion = the issuing wave's vmcnt, then a workgroup barrier.  (The walk is dma_rows8's with half 0 and dh 64, written out:
// through dma_rows8 one wait of attn_bwd_dkv_kernel<false>'s prologue moves behind the barrier.)
__device__ __forceinline__ void dma_tile(char* tile, const bf16_t* base, long stride_t, int rows_valid,
                                         int rows_pad, int wave, int nwaves, int lane) {
  const __amdgpu_buffer_rsrc_t rsrc = dma_rsrc(base, stride_t, rows_valid, DH);
  const int r8 = lane >> 3, slot = lane & 7;
  for (int inst = wave; inst < rows_pad / 8; inst += nwaves) {
    const int row = inst * 8 + r8;
    const int chunk = slot ^ swz(row);
    const unsigned off = row < rows_valid ? (unsigned)(row * stride_t * 2 + chunk * 16) : 0x80000000u;
    lds_dma16(rsrc, tile + inst * 1024, off);
  }
}

// row-operand fragment ks (32 columns) of the wave's own 16 rows straight from global memory, zero beyond dh
__device__ __forceinline__ bf16x8 frag_global_dh(const bf16_t* base, long stride_t, int row0, int rows_valid, int ks,
                                                 int lane, int dh) {
  const int row = row0 + (lane & 15);
  const int col = ks * 32 + (lane >> 4) * 8;
  bf16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < rows_valid && col < dh) r = *reinterpret_cast<const bf16x8*>(base + (long)row * stride_t + col);
  return r;
}

// LDS-space pointers for the kernels that build the lane-constant part of their LDS addresses once (attn_bwd_one_kernel,
// attn_bwd_one2_kernel, attn_bwd_dkv2_kernel, attn_bwd_dq3_kernel; the reasons are told there).  CFHIP_OPAQUE_LDS hides a pointer's
// value from the optimiser (so that it stays one register instead of being rebuilt at every use), CFHIP_LDS_XOR flips address bits.
typedef __attribute__((address_space(3))) const char* lds_cp;
typedef __attribute__((address_space(3))) char* lds_p;
typedef __attribute__((address_space(3))) const bf16x8* lds_v8;
typedef __attribute__((address_space(3))) const f32x4* lds_f4;
typedef __attribute__((address_space(3))) s16x4* lds_s4;
typedef __attribute__((address_space(3))) const s16x4* lds_cs4;
#define CFHIP_OPAQUE_LDS(ptr, T) { unsigned u_ = (unsigned)(uintptr_t)(ptr); asm volatile("" : "+v"(u_)); (ptr) = (T)(uintptr_t)u_; }
#define CFHIP_LDS_XOR(ptr, bits) ((lds_cp)(uintptr_t)((unsigned)(uintptr_t)(ptr) ^ (unsigned)(bits)))

// row-operand fragment straight from global memory (one 16-row tile owned by this wave)
__device__ __forceinline__ bf16x8 frag_global(const bf16_t* base, long stride_t, int row0, int rows_valid,
                                              int ks, int lane) {
  const int row = row0 + (lane & 15);
  bf16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < rows_valid)
    r = *reinterpret_cast<const bf16x8*>(base + (long)row * stride_t + ks * 32 + (lane >> 4) * 8);
  return r;
}

// Packed f32 VALU, measured twice in round 6 (profiles/r06/attn_packed_f32_rejected.txt): (1) the softmax math of the long-sequence backward
// passes written on vectors (16 fma + 16 mul -> 8 v_pk_fma_f32 + 8 v_pk_mul_f32 per block) made dQ 2.5 % and dK / dV 4-5 % SLOWER — the
// packed instructions are no bargain beside MFMAs (MI355X_MICROARCH.md prices one v_pk_fma_f32 at +22 cycles against two v_fma_f32);
// (2) the other direction — the v_pk_mul_f32 hipcc's SLP pass makes of the one-pass backward's `pr * (dP - delta)` pinned to single
// v_mul_f32 through inline asm — was 3.4 % slower too (12 more conversions).  And inline asm must never READ an MFMA result: hipcc's
// hazard recogniser does not see the asm as a VALU consumer and omits the wait states (the persistent forward with asm fma / max3
// on the scores returned NaN).  So: scalar source, the compiler's own choice of packing, asm only on VALU results (max_nn).

// One 64-column output row per lane group: lane (n = l & 15, g = l >> 4) holds columns 16 dt + 4 g .. + 3 of row n for the
// four 16-column tiles dt.  Written as they are, that is four 8-byte stores per lane, 32-byte runs per row and
// instruction — the store tail of these kernels is issue-bound (dK/dV: 34 of 105 us).  Lanes g and g ^ 1 swap half of
// their values instead (two ds_bpermute per tile pair), so that every lane owns 8 consecutive columns of ONE tile and
// the row goes out as two 16-byte stores per lane, 64-byte runs per row and instruction.  Call with all lanes active.
__device__ __forceinline__ void store_row64(bf16_t* row, const f32x4 (&t)[4], float mul, int g, bool valid) {
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const f32x4 a = t[2 * pr] * mul, b = t[2 * pr + 1] * mul;
    const unsigned a0 = pack_bf16x2(a[0], a[1]), a1 = pack_bf16x2(a[2], a[3]);
    const unsigned b0 = pack_bf16x2(b[0], b[1]), b1 = pack_bf16x2(b[2], b[3]);
    const bool odd = (g & 1) != 0;
    const unsigned r0 = (unsigned)__shfl_xor((int)(odd ? a0 : b0), 16, 64);  // even g sends tile 2pr+1, odd g tile 2pr
    const unsigned r1 = (unsigned)__shfl_xor((int)(odd ? a1 : b1), 16, 64);
    // even g: own tile-2pr columns 4g..4g+3, then the partner's (g + 1); odd g: the partner's (g - 1) tile-(2pr+1)
    // columns, then its own
    const u32x4 w = odd ? u32x4{r0, r1, b0, b1} : u32x4{a0, a1, r0, r1};
    const int col = (2 * pr + (odd ? 1 : 0)) * 16 + 4 * (g & 2);
    if (valid) *reinterpret_cast<u32x4*>(row + col) = w;
  }
}

// the same for ONE pair of 16-column tiles (2 pr, 2 pr + 1) of the row: one 16-byte store per lane
__device__ __forceinline__ void store_row32(bf16_t* row, const f32x4& ta, const f32x4& tb, float mul, int g, bool valid, int pr) {
  const f32x4 a = ta * mul, b = tb * mul;
  const unsigned a0 = pack_bf16x2(a[0], a[1]), a1 = pack_bf16x2(a[2], a[3]);
  const unsigned b0 = pack_bf16x2(b[0], b[1]), b1 = pack_bf16x2(b[2], b[3]);
  const bool odd = (g & 1) != 0;
  const unsigned r0 = (unsigned)__shfl_xor((int)(odd ? a0 : b0), 16, 64);
  const unsigned r1 = (unsigned)__shfl_xor((int)(odd ? a1 : b1), 16, 64);
  const u32x4 w = odd ? u32x4{r0, r1, b0, b1} : u32x4{a0, a1, r0, r1};
  const int col = (2 * pr + (odd ? 1 : 0)) * 16 + 4 * (g & 2);
  if (valid) *reinterpret_cast<u32x4*>(row + col) = w;
}
// (store_row64 stays written out beside store_row32: as two calls of it, hipcc orders the shuffles of the dK and dV rows of
// attn_bwd_dkv_pers_kernel differently and one wait of that kernel's store tail moves.)

// (`Params`: the AttnParams of csrc/attn_host.h — a template so that this header needs no host-side type)
template <typename Params>
__device__ __forceinline__ bool keep_at(const Params& p, int b, int h, int i, int j) {
  if (j >= p.Tk) return false;
  if (p.causal && j > i) return false;
  if (p.mask != nullptr) return p.mask[(long)b * p.ms_b + (long)h * p.ms_h + (long)i * p.ms_q + j] != 0;
  return true;
}

// A query row without a kept key (mask only) has l = 0 in the forward: its O — and so its delta = rowsum(dO * O) — is not
// finite.  Every p of such a row is 0 by the keep select, but 0 * (dP - NaN) would carry the NaN into dK of every key
// through dS^T Q: the masked backward kernels take delta = 0 for such a row (its dS is then exactly 0).
__device__ __forceinline__ float finite_or_zero(float x) { return fabsf(x) < INFINITY ? x : 0.f; }

template <typename Params>
__device__ __forceinline__ Philox drop_block(const Params& p, int b, int h, int block_row, int block_col) {
  const unsigned long long ctr =
      p.drop_offset + ((unsigned long long)(b * p.H + h) * p.drop_bq + block_row) * p.drop_bk + block_col;
  return philox4x32_10(ctr, p.drop_seed);
}
__device__ __forceinline__ unsigned pick_word(const Philox& r, int w) {  // r.c[w & 3] without a private-memory array
  const unsigned lo = (w & 1) ? r.c[1] : r.c[0], hi = (w & 1) ? r.c[3] : r.c[2];
  return (w & 2) ? hi : lo;
}

// The same through gfx950's lane swaps (round 6): `__shfl_xor` is a ds_bpermute — an LDS round trip behind ~6 VALU of address arithmetic,
// twice in a row on the critical path of every 64-key block of the long-sequence forward.  v_permlane16_swap(v, v) leaves the two halves of
// every 32-lane pair of rows side by side (result 0: the even rows' values in both rows, result 1: the odd rows'), v_permlane32_swap(v, v)
// the two 32-lane halves: one max each.
// max of two values that are never NaN (scores, running maxima: finite or -inf): fmaxf() on values that come out of a lane swap
// (integers to the compiler) is preceded by a quieting v_max_f32 v, v, v per operand — three instructions for one; the med3(x, y, +inf)
// builtin is folded back into the same maxnum.  The instruction itself, then.
__device__ __forceinline__ float max_nn(float x, float y) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ float group_max_swap(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float m1 = max_nn(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const unsigned w = __float_as_uint(m1);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return max_nn(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// Round 3 measured a TWO-slot chunk ring for head_dim <= 64 (chunk c + 1 streaming into the other slot while chunk c is
// computed, 128-row chunks, one barrier per chunk; the code path is still here: NSLOT = 2): UNet shape B1 H8 T65536 dh40 forward
// 12.47 -> 13.86 ms, dQ 12.84 -> 13.21, dK/dV after a dQ pass 17.5 -> 20.2; 256^2 step 611 -> 645 ms
// (profiles/r03/attn_long_bench_{r02kernels,two_slot_ring}.log).  The load was already covered by the second workgroup of
// the CU; what the ring costs is twice the online-softmax steps per key (128- instead of 256-key chunks) and every wave of
// the workgroup in lock-step on one barrier.  Kept: NSLOT = 1, 256-row chunks for head_dim <= 64.
template <int NH>
struct Gen {
  static constexpr int CH = NH == 1 ? 256 : 128;  // rows per staged chunk (LDS: 2 operands x NH halves x CH x 128 B per slot)
  static constexpr int CHB = CH / 32;
  static constexpr int HALF_BYTES = CH * 128;
  static constexpr int OPER_BYTES = NH * HALF_BYTES;
  static constexpr int SLOT_BYTES = 2 * OPER_BYTES;
  static constexpr int NSLOT = 1;
};

template <int NH, bool SKIP_PAD = false>
__device__ __forceinline__ void dma_oper(char* tiles, const bf16_t* base, long stride_t, int rows_valid, int dh,
                                         int wave, int nwaves, int lane) {
#pragma unroll
  for (int hf = 0; hf < NH; ++hf)
    dma_half<SKIP_PAD>(tiles + hf * Gen<NH>::HALF_BYTES, base, stride_t, rows_valid, Gen<NH>::CH, hf, dh, wave, nwaves, lane);
}

}  // namespace
