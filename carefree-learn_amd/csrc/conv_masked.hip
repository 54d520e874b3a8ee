// Masked 7x7 convolution of the PixelCNN for gfx950 (reference modules/cv/ar/pixel_cnn.py:20-65: MaskedConv2d, stride 1, padding 3):
// only the T live taps (24 for mask "A", 25 for "B": the first T row-major positions of the 7x7 window) are packed, read and
// multiplied; the [B H W, 49 Cin] im2row matrix is never formed.
//
// conv_masked_kernel<NTL>: bf16 NHWC rows in and out.  A workgroup (256 threads, 4 waves) owns a 16 x 16 tile of output pixels of one
// image and NTL 16-channel output tiles.  The halo of the tile is one-sided: 3 rows above (mirror = 0) or below (mirror = 1: the
// input gradient, the same kernel on the mirrored tap set with the transposed pack) and 3 columns either side, 19 x 22 pixels, staged
// in LDS 32 input channels at a time (zero outside the image).  Wave w computes the tile's rows 4 w .. 4 w + 3 (one MFMA M-tile of 16
// pixels each); the filter fragments come from the row-major pack [Co][T Ci] in global memory, one 16-byte load per lane.
// Operation order, per output element: f32 MFMA accumulation (v_mfma_f32_16x16x32_bf16) from 0 over the input-channel chunks of 32 in
// ascending order and, inside a chunk, over the taps t = 0 .. T - 1; then + bias (optional), one rounding to bf16.  Fixed order, no
// atomics: bit-identical between runs.
//
// conv_masked_gather_kernel: rows [row0, row0 + nrows) of the live-tap matrix G[row][t Ci + c] = x[b][i + t / 7 - 3][j + t % 7 - 3][c]
// (zero outside the image), the B operand of the weight gradient dWpack = dy_rows^T G (a `tn` GEMM per row chunk).
// conv_masked_pack_kernel: f32 weight [Cout][Cin][7][7] -> bf16 [Cout][T Cin] (k = t Cin + c) or, transposed, [Cin][T Cout]
// (k = t Cout + n); masked taps are never read.
#include "common.h"

namespace {

constexpr int CM_TILE = 16;
constexpr int CM_HROWS = CM_TILE + 3, CM_HCOLS = CM_TILE + 6;
constexpr int CM_LDP = 40;  // bf16 per staged pixel: 32 channels + 8 of padding (80 bytes: 16-byte aligned, spreads the banks)

template <int NTL>
__global__ __launch_bounds__(256) void conv_masked_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ pack,
                                                          const float* __restrict__ bias, bf16_t* __restrict__ y, int H, int W, int Ci,
                                                          int Co, int T, int mirror, int tiles_x) {
  __shared__ __attribute__((aligned(16))) bf16_t halo[CM_HROWS * CM_HCOLS * CM_LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int ty0 = blockIdx.x / tiles_x, i0 = ty0 * CM_TILE, j0 = (blockIdx.x - ty0 * tiles_x) * CM_TILE;
  const long b = blockIdx.y;
  const int n0 = blockIdx.z * NTL * 16;
  const long ldk = (long)T * Ci;
  const int row_org = mirror ? i0 : i0 - 3, col_org = j0 - 3;
  f32x4 acc[4][NTL];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < NTL; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* wrow = pack + (long)(n0 + lr) * ldk + lq * 8;
  for (int c0 = 0; c0 < Ci; c0 += 32) {
    __syncthreads();
    for (int idx = tid; idx < CM_HROWS * CM_HCOLS * 4; idx += 256) {
      const int pix = idx >> 2, part = idx & 3, hr = pix / CM_HCOLS, hc = pix - hr * CM_HCOLS;
      const int ii = row_org + hr, jj = col_org + hc;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (ii >= 0 && ii < H && jj >= 0 && jj < W) v = *reinterpret_cast<const u32x4*>(x + (((b * H + ii) * W + jj) * (long)Ci + c0 + part * 8));
      *reinterpret_cast<u32x4*>(halo + pix * CM_LDP + part * 8) = v;
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const int ty = t / 7, tx = t - ty * 7;
      const int dr = mirror ? 3 - ty : ty, dc = mirror ? 6 - tx : tx;
      bf16x8 wf[NTL];
#pragma unroll
      for (int n = 0; n < NTL; ++n) wf[n] = *reinterpret_cast<const bf16x8*>(wrow + (long)n * 16 * ldk + (long)t * Ci + c0);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(halo + ((wave * 4 + m + dr) * CM_HCOLS + lr + dc) * CM_LDP + lq * 8);
#pragma unroll
        for (int n = 0; n < NTL; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf[n], acc[m][n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NTL; ++n) {
    const int ch = n0 + n * 16 + lr;
    const float bv = bias ? bias[ch] : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int ii = i0 + wave * 4 + m;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int jj = j0 + lq * 4 + r4;
        if (ii < H && jj < W) y[((b * H + ii) * W + jj) * (long)Co + ch] = f32_to_bf16(bias ? acc[m][n][r4] + bv : acc[m][n][r4]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv_masked_gather_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, long row0,
                                                                 long nrows, int H, int W, int Ci, int T) {
  const int c8 = Ci >> 3;
  const long per_row = (long)T * c8, idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nrows * per_row) return;
  const long r = idx / per_row, row = row0 + r;
  const int rem = (int)(idx - r * per_row), t = rem / c8, c = (rem - t * c8) * 8;
  const long b = row / ((long)H * W);
  const int p = (int)(row - b * (long)H * W), i = p / W, j = p - i * W;
  const int ii = i + t / 7 - 3, jj = j + t % 7 - 3;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (ii >= 0 && jj >= 0 && jj < W) v = *reinterpret_cast<const u32x4*>(x + (((b * H + ii) * W + jj) * (long)Ci + c));
  *reinterpret_cast<u32x4*>(out + (r * T + t) * (long)Ci + c) = v;
}

__global__ __launch_bounds__(256) void conv_masked_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cout, int Cin,
                                                               int T, int transposed) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Cout * Cin * T) return;
  int n, c, t;
  if (!transposed) {  // out[n][t Cin + c]
    c = (int)(idx % Cin);
    t = (int)((idx / Cin) % T);
    n = (int)(idx / ((long)Cin * T));
  } else {  // out[c][t Cout + n]
    n = (int)(idx % Cout);
    t = (int)((idx / Cout) % T);
    c = (int)(idx / ((long)Cout * T));
  }
  out[idx] = f32_to_bf16(w[((long)n * Cin + c) * 49 + t]);
}

bool cm_shape_ok(int Ci, int Co, int T, const char* who) {
  if (T != 24 && T != 25) {
    cfhip_set_error("%s: %d live taps (24 = mask A, 25 = mask B of a 7x7 filter)", who, T);
    return false;
  }
  if (Ci < 32 || Co < 32 || Ci % 32 != 0 || Co % 32 != 0) {
    cfhip_set_error("%s: channels %d -> %d are outside the masked kernels (multiples of 32 on both sides)", who, Ci, Co);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int cfhip_conv_masked_pack(const float* w, void* pack, int Cout, int Cin, int taps, int transposed, void* stream) {
  if (!cm_shape_ok(Cin, Cout, taps, "conv_masked_pack")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(w && pack, "conv_masked_pack: null operand");
  CFHIP_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)pack & 15) == 0, "conv_masked_pack: misaligned operand");
  const long total = (long)Cout * Cin * taps;
  hipLaunchKernelGGL(conv_masked_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     reinterpret_cast<bf16_t*>(pack), Cout, Cin, taps, transposed != 0);
  CFHIP_CHECK_LAUNCH("conv_masked_pack");
  return CFHIP_OK;
}

extern "C" int cfhip_conv_masked_bf16(const void* x, const void* pack, const float* bias, void* y, int B, int H, int W, int Ci, int Co,
                                      int taps, int mirror, void* stream) {
  if (!cm_shape_ok(Ci, Co, taps, "conv_masked")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(x && pack && y, "conv_masked: null operand");
  CFHIP_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W <= 0x3fffffffL, "conv_masked: B = %d, H = %d, W = %d", B, H, W);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)pack) & 15) == 0 && ((uintptr_t)y & 1) == 0 && ((uintptr_t)bias & 3) == 0,
                "conv_masked: misaligned operand");
  const int tiles_x = (W + CM_TILE - 1) / CM_TILE, tiles_y = (H + CM_TILE - 1) / CM_TILE, nt = Co / 16;
  const int ntl = nt % 8 == 0 ? 8 : nt % 4 == 0 ? 4 : 2;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B, (unsigned)(nt / ntl));
  CFHIP_REQUIRE(nt / ntl <= 65535, "conv_masked: Co = %d", Co);
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  const bf16_t* pp = reinterpret_cast<const bf16_t*>(pack);
  bf16_t* yp = reinterpret_cast<bf16_t*>(y);
  const int mr = mirror != 0;
  if (ntl == 8) hipLaunchKernelGGL(conv_masked_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, xp, pp, bias, yp, H, W, Ci, Co, taps, mr, tiles_x);
  else if (ntl == 4) hipLaunchKernelGGL(conv_masked_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, xp, pp, bias, yp, H, W, Ci, Co, taps, mr, tiles_x);
  else hipLaunchKernelGGL(conv_masked_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, xp, pp, bias, yp, H, W, Ci, Co, taps, mr, tiles_x);
  CFHIP_CHECK_LAUNCH("conv_masked");
  return CFHIP_OK;
}

extern "C" int cfhip_conv_masked_gather(const void* x, void* out, int64_t row0, int64_t nrows, int B, int H, int W, int Ci, int taps,
                                        void* stream) {
  if (!cm_shape_ok(Ci, 32, taps, "conv_masked_gather")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(x && out, "conv_masked_gather: null operand");
  CFHIP_REQUIRE(B >= 1 && H >= 1 && W >= 1 && row0 >= 0 && nrows >= 1 && row0 + nrows <= (int64_t)B * H * W,
                "conv_masked_gather: rows [%lld, %lld) are not inside the %lld rows of the input", (long long)row0, (long long)(row0 + nrows),
                (long long)B * H * W);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "conv_masked_gather: misaligned operand");
  const long total = (long)nrows * taps * (Ci / 8);
  CFHIP_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "conv_masked_gather: %lld rows in one launch", (long long)nrows);
  hipLaunchKernelGGL(conv_masked_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(out), (long)row0, (long)nrows, H, W, Ci, taps);
  CFHIP_CHECK_LAUNCH("conv_masked_gather");
  return CFHIP_OK;
}
