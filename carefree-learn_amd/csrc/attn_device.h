// Device parts shared by the attention kernels of csrc/attn.hip and csrc/attn_wide.hip: the swizzled [rows][64] bf16 LDS tile,
// its LDS-DMA fill, the MFMA operand fragments read from it, and the group reductions of the online softmax.
#pragma once
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

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
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
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

// one 64-column half of `rows_pad` rows -> swizzled [rows][64] tile; columns >= dh and rows >= rows_valid are zero.
// SKIP_PAD: the lanes whose 16-byte chunk lies beyond dh are switched off (EXEC) instead of fetching zeros, so the DMA never
// writes the pad columns of the tile: whatever the kernel put there once (zeros; attn_fwd2_kernel's column of ones) stays.
template <bool SKIP_PAD = false>
__device__ __forceinline__ void dma_half(char* tile, const bf16_t* base, long stride_t, int rows_valid, int rows_pad,
                                         int half, int dh, int wave, int nwaves, int lane) {
  long bytes = ((long)(rows_valid - 1) * stride_t + dh) * 2;
  if (bytes > 0x7fffffffL) bytes = 0x7fffffffL;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, (int)bytes, 0x00020000);
  const int r8 = lane >> 3, slot = lane & 7;
  for (int inst = wave; inst < rows_pad / 8; inst += nwaves) {
    const int row = inst * 8 + r8;
    const int chunk = slot ^ swz(row);
    const bool ok = row < rows_valid && half * 64 + chunk * 8 < dh;
    const unsigned off = ok ? (unsigned)(row * stride_t * 2 + half * 128 + chunk * 16) : 0x80000000u;
    if (SKIP_PAD) {
      if (half * 64 + chunk * 8 < dh) lds_dma16(rsrc, tile + inst * 1024, off);  // (rows beyond rows_valid still fetch zeros)
    } else {
      lds_dma16(rsrc, tile + inst * 1024, off);
    }
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

}  // namespace
