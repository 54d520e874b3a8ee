// LoRA adapters of Linear layers (reference modules/core/hijacks.py:157-166: `out + scale * dropout(lora_up(lora_down(inp)))`,
// and the autograd backward of those four ATen ops) as three kernel forms around a factor of rank r <= 64:
//
//   lora_down     h [M, r]  = s * (mask . X) F^T        X [M, K] read once, the factor resident in LDS          (skinny-N product)
//   lora_up_add   Y [M, N] += s * mask . (H F^T)        one read-modify-write pass over Y                       (rank-r update in place)
//   lora_wgrad    G [J, r]  (+)= s * (mask . T)^T U     reduction over M in row splits: f32 partials, then a    (tall reduction)
//                                                       second kernel that adds them in split order
//
// All three run on mfma_f32_16x16x32_bf16 with the rank padded to the MFMA width in LDS / registers only (nothing padded in
// HBM), accumulate in f32, use plain vector stores and no atomics: the same inputs give the same bits.  `mask` is the keep mask
// of csrc/random.hip's dropout over the contiguous [M, N] index space (element i: Philox4x32-10 keyed by `seed`, counter
// offset + i / 4, word i % 4, keep = u >= p), regenerated wherever it is needed and never stored; p == 0 skips the generator.
// The kept values' factor here is s / (1 - p) formed in f32, not cfhip_dropout's 1.0f / (float)(1.0 - p): the two can differ in the last bit.
// Fragment maps (lane l, g = l >> 4): A[row l & 15][k = 8 g + e], B[k = 8 g + e][col l & 15], e = 0..7; D[row 4 g + i][col l & 15].
//
// LoRA adapters of Conv2d layers (reference hijacks.py:208-266: lora_down a k x k convolution Cin -> r with the base layer's
// stride and padding, lora_up a 1x1 convolution r -> Cout) on NHWC rows [B H W, C]: every 1x1 piece IS one of the three forms
// above; the 3x3 / pad 1 / stride 1 or 2 down factor adds three gather forms that read the factor in the parameter's own layout
// f[c][ci][ky][kx] and permute it to (ky, kx, ci) order on the way into LDS (no packed copy in HBM):
//
//   lora_conv_down   h [B Ho Wo, r] = s * sum_taps X[nbr] F_tap^T     a lane's A fragment = 8 channels of one tap (or zeros)
//   lora_conv_dx     dX [B H W, C] (+)= sum_(tap, c) dH[nbr][c] F     gather form of the transposed convolution, D^T = F dH^T
//   lora_conv_wgrad  G [r][C][3][3] (+)= s * dH^T im2row(X)           the tall reduction over a virtual [B Ho Wo, 9 C] matrix
#include "common.h"

namespace {

constexpr int MAX_RANK = 64;
constexpr int THREADS = 256;      // four waves
constexpr int LDS_BUDGET = 65536; // dynamic LDS of one workgroup (no opt-in needed, two workgroups per CU)

__device__ __forceinline__ float u01(unsigned r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }  // as csrc/random.hip

// 8 bf16 values of flat indices i0 .. i0 + 7 (i0 % 4 == 0): dropped ones become +0
__device__ __forceinline__ bf16x8 mask8(bf16x8 v, long i0, float p, unsigned long long seed, unsigned long long offset) {
  const Philox r0 = philox4x32_10(offset + (unsigned long long)(i0 >> 2), seed);
  const Philox r1 = philox4x32_10(offset + (unsigned long long)(i0 >> 2) + 1ull, seed);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!(u01(r0.c[e]) >= p)) v[e] = 0;
    if (!(u01(r1.c[e]) >= p)) v[4 + e] = 0;
  }
  return v;
}

__device__ __forceinline__ bf16x8 zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// ---- skinny-N product ----------------------------------------------------------------------------------------------------------
// One workgroup walks stripes of 64 rows (16 per wave) and runs the whole reduction of each.  The factor sits in LDS as
// Fs[j][k] (j < 16 nct, pitch KC + 8 elements = 16 m + 4 dwords: the 16 rows one ds_read_b128 lane group reads fall on 16
// different 4-dword bank slots); when all of it fits (K <= KC) it is staged once per workgroup, else per K chunk.
// FT: the factor is given as [K][r] (ldf) instead of [r][K].
template <bool FT>
__global__ __launch_bounds__(THREADS) void lora_down_kernel(const bf16_t* __restrict__ X, long ldx, const bf16_t* __restrict__ F,
                                                            long ldf, bf16_t* __restrict__ H, int M, int K, int r, int KC,
                                                            float scale, float p, unsigned long long seed,
                                                            unsigned long long offset) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Fs = reinterpret_cast<bf16_t*>(smem);
  const int pitch = KC + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int nct = (r + 15) >> 4, rows_f = nct << 4;
  const int chunks = (K + KC - 1) / KC;
  const int stripes = (M + 63) >> 6;
  for (int st = blockIdx.x; st < stripes; st += gridDim.x) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long row = (long)st * 64 + wave * 16 + lr;
    const bool row_ok = row < M;
    for (int c = 0; c < chunks; ++c) {
      const int k0 = c * KC;
      const int kc = min(KC, K - k0);    // multiple of 8
      const int kcp = (kc + 31) & ~31;   // MFMA steps of 32: the tail is zero in LDS
      if (chunks > 1 || st == (int)blockIdx.x) {
        __syncthreads();
        if (FT) {
          for (int idx = threadIdx.x; idx < rows_f * kcp; idx += THREADS) {
            const int j = idx % rows_f, k = idx / rows_f;
            Fs[j * pitch + k] = (j < r && k < kc) ? F[(long)(k0 + k) * ldf + j] : (bf16_t)0;
          }
        } else {
          const int k8n = kcp >> 3;
          for (int idx = threadIdx.x; idx < rows_f * k8n; idx += THREADS) {
            const int j = idx / k8n, k = (idx % k8n) << 3;
            bf16x8 v = zero8();
            if (j < r && k < kc) v = *reinterpret_cast<const bf16x8*>(F + (long)j * ldf + k0 + k);
            *reinterpret_cast<bf16x8*>(Fs + j * pitch + k) = v;
          }
        }
        __syncthreads();
      }
      for (int ks = 0; ks < kcp; ks += 32) {
        const int k = ks + 8 * g;
        bf16x8 a = zero8();
        if (row_ok && k < kc) {
          a = *reinterpret_cast<const bf16x8*>(X + row * ldx + k0 + k);
          if (p > 0.f) a = mask8(a, row * (long)K + k0 + k, p, seed, offset);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < nct) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(Fs + (t * 16 + lr) * pitch + k);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = t * 16 + lr;
      if (t < nct && col < r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long rr = (long)st * 64 + wave * 16 + 4 * g + i;
          if (rr < M) H[rr * r + col] = f32_to_bf16(acc[t][i] * scale);
        }
      }
    }
  }
}

// ---- rank-r update in place ----------------------------------------------------------------------------------------------------
// D^T = F H^T: the factor is the A operand (rows = output columns n), H the B operand (columns = rows m of Y), so a lane ends up
// with FOUR CONSECUTIVE n of one row m: one 8-byte (bf16) / 16-byte (f32) read-modify-write and exactly one Philox counter.
// blockIdx.y owns 256 output columns whose factor rows sit in LDS as Fs[n][c] (pitch kp + 8 = 40 / 72 elements = 20 / 36
// dwords: conflict-free for a 16-lane group); blockIdx.x walks stripes of 64 rows.  FT: the factor is [r][N] (ldf), not [N][r].
constexpr int UP_NC = 256;

template <bool FT, bool YF32>
__global__ __launch_bounds__(THREADS) void lora_up_add_kernel(const bf16_t* __restrict__ H, const bf16_t* __restrict__ F, long ldf,
                                                              void* __restrict__ Y, long ldy, int M, int N, int r, float scale,
                                                              float p, unsigned long long seed, unsigned long long offset) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Fs = reinterpret_cast<bf16_t*>(smem);
  const int kp = (r + 31) & ~31, pitch = kp + 8, ksteps = kp >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int n_base = blockIdx.y * UP_NC;
  const int nc = min(UP_NC, N - n_base);   // multiple of 4
  const int ntiles = (nc + 15) >> 4;
  for (int idx = threadIdx.x; idx < ntiles * 16 * kp; idx += THREADS) {
    int n, c;
    if (FT) { n = idx % (ntiles * 16); c = idx / (ntiles * 16); } else { n = idx / kp; c = idx % kp; }
    bf16_t v = 0;
    if (n < nc && c < r) v = FT ? F[(long)c * ldf + n_base + n] : F[(long)(n_base + n) * ldf + c];
    Fs[n * pitch + c] = v;
  }
  __syncthreads();
  const int stripes = (M + 63) >> 6;
  for (int st = blockIdx.x; st < stripes; st += gridDim.x) {
    const long m = (long)st * 64 + wave * 16 + lr;
    bf16x8 hb[2] = {zero8(), zero8()};
    if (m < M) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int c0 = ks * 32 + 8 * g;
        if (ks < ksteps && c0 < r) {
          if ((r & 7) == 0) {
            hb[ks] = *reinterpret_cast<const bf16x8*>(H + m * r + c0);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (c0 + e < r) hb[ks][e] = (short)H[m * r + c0 + e];
          }
        }
      }
    }
    for (int nt = 0; nt < ntiles; ++nt) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (ks < ksteps) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(Fs + (nt * 16 + lr) * pitch + ks * 32 + 8 * g);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, hb[ks], acc, 0, 0, 0);
        }
      }
      const int n = nt * 16 + 4 * g;  // this lane: Y[m][n_base + n .. + 3]
      if (m < M && n < nc) {
        bool keep[4] = {true, true, true, true};
        if (p > 0.f) {
          const Philox rnd = philox4x32_10(offset + (unsigned long long)((m * (long)N + n_base + n) >> 2), seed);
#pragma unroll
          for (int e = 0; e < 4; ++e) keep[e] = u01(rnd.c[e]) >= p;
        }
        if (YF32) {
          float* yp = reinterpret_cast<float*>(Y) + m * ldy + n_base + n;
          f32x4 y = *reinterpret_cast<const f32x4*>(yp);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (keep[e]) y[e] = fmaf(scale, acc[e], y[e]);
          *reinterpret_cast<f32x4*>(yp) = y;
        } else {
          bf16_t* yp = reinterpret_cast<bf16_t*>(Y) + m * ldy + n_base + n;
          s16x4 y = *reinterpret_cast<const s16x4*>(yp);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (keep[e]) y[e] = (short)f32_to_bf16(fmaf(scale, acc[e], bf16_to_f32((bf16_t)y[e])));
          *reinterpret_cast<s16x4*>(yp) = y;
        }
      }
    }
  }
}

// ---- tall reduction ------------------------------------------------------------------------------------------------------------
// G[j][c] = sum_m T[m][j] U[m][c]: both MFMA operands want the reduction index (m) contiguous per lane, T has it strided, so a
// [32 m][64 j] tile of T goes through LDS (16-byte global reads along j, masked on the way; pitch 68 elements = 34 dwords: the four
// lane groups of the column read sit 16 banks apart) and U through LDS transposed (Us[c][m], pitch 40).  blockIdx.x owns 64
// columns j (16 per wave, every c), blockIdx.y a row split; partial sums go to ws[split][j][c] (f32) and lora_wgrad_reduce adds
// the splits in order.
constexpr int WG_ROWS = 32, WG_COLS = 64, WG_TPITCH = 68, WG_UPITCH = 40;

__global__ __launch_bounds__(THREADS) void lora_wgrad_kernel(const bf16_t* __restrict__ T, long ldt, const bf16_t* __restrict__ U,
                                                             float* __restrict__ ws, int M, int J, int r, int rows_per_split,
                                                             float p, unsigned long long seed, unsigned long long offset) {
  __shared__ __attribute__((aligned(16))) bf16_t Ts[WG_ROWS * WG_TPITCH];
  __shared__ __attribute__((aligned(16))) bf16_t Us[MAX_RANK * WG_UPITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int nct = (r + 15) >> 4, rows_u = nct << 4;
  const int j_base = blockIdx.x * WG_COLS;
  const long m_begin = (long)blockIdx.y * rows_per_split;
  const long m_end = min((long)M, m_begin + rows_per_split);
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tm = threadIdx.x >> 3, tj = (threadIdx.x & 7) << 3;  // this thread's 8 elements of the T tile
  for (long m0 = m_begin; m0 < m_end; m0 += WG_ROWS) {
    __syncthreads();
    {
      const long m = m0 + tm;
      const int j = j_base + tj;
      bf16x8 v = zero8();
      if (m < m_end && j < J) {
        v = *reinterpret_cast<const bf16x8*>(T + m * ldt + j);
        if (p > 0.f) v = mask8(v, m * (long)J + j, p, seed, offset);
      }
      s16x4* dst = reinterpret_cast<s16x4*>(Ts + tm * WG_TPITCH + tj);
      dst[0] = s16x4{v[0], v[1], v[2], v[3]};
      dst[1] = s16x4{v[4], v[5], v[6], v[7]};
    }
    for (int idx = threadIdx.x; idx < WG_ROWS * rows_u; idx += THREADS) {
      const int mm = idx / rows_u, c = idx % rows_u;
      const long m = m0 + mm;
      Us[c * WG_UPITCH + mm] = (m < m_end && c < r) ? U[m * r + c] : (bf16_t)0;
    }
    __syncthreads();
    bf16x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (short)Ts[(8 * g + e) * WG_TPITCH + wave * 16 + lr];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nct) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(Us + (t * 16 + lr) * WG_UPITCH + 8 * g);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = t * 16 + lr;
    if (t < nct && c < r) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = j_base + wave * 16 + 4 * g + i;
        if (j < J) ws[((long)blockIdx.y * J + j) * r + c] = acc[t][i];
      }
    }
  }
}

// out (+)= scale * (ws[0] + ws[1] + ... in split order); out is [J][r], or [r][J] when out_trans
__global__ void lora_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int splits, int J, int r,
                                         int out_trans, int accumulate, float scale) {
  const long total = (long)J * r;
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  float s = ws[idx];
  for (int k = 1; k < splits; ++k) s += ws[(long)k * total + idx];
  s *= scale;
  const long o = out_trans ? (idx % r) * (long)J + idx / r : idx;
  out[o] = accumulate ? out[o] + s : s;
}

// ---- 3x3 convolution adapters: the down factor ---------------------------------------------------------------------------------
// Geometry of a 3x3 / pad 1 / stride s (1 or 2) convolution over NHWC rows: Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1.
struct ConvGeom {
  int B, H, W, Ho, Wo, C, s;
};

// Skinny product over K = (tap, ci): stripes of 64 output pixels, 16 per wave, as lora_down_kernel.  The factor is staged in chunks
// of CC channels x 9 taps as Fs[j][tap * cc + cl] (pitch = 9 CC rounded up to 32, + 8 elements = 16 m + 4 dwords: the bank rule
// of lora_down_kernel); the global reads of a chunk run along (cl, tap), 9 cc contiguous elements per factor row.  A lane's A
// fragment at k = tap * cc + cl is x[(b, oy s + ky - 1, ox s + kx - 1)][c0 + cl .. + 7]: cc % 8 == 0, so the 8 never straddle a tap.
__global__ __launch_bounds__(THREADS) void lora_conv_down_kernel(const bf16_t* __restrict__ X, long ldx, const bf16_t* __restrict__ F,
                                                                 bf16_t* __restrict__ Hout, ConvGeom q, int M, int r, int CC,
                                                                 float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Fs = reinterpret_cast<bf16_t*>(smem);
  const int pitch = ((9 * CC + 31) & ~31) + 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int nct = (r + 15) >> 4, rows_f = nct << 4;
  const int chunks = (q.C + CC - 1) / CC;
  const int stripes = (M + 63) >> 6;
  for (int st = blockIdx.x; st < stripes; st += gridDim.x) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = st * 64 + wave * 16 + lr;
    const bool row_ok = row < M;
    const int ox = row % q.Wo, oy = (row / q.Wo) % q.Ho, b = row / (q.Wo * q.Ho);
    const int iy0 = oy * q.s - 1, ix0 = ox * q.s - 1;
    for (int c = 0; c < chunks; ++c) {
      const int c0 = c * CC;
      const int cc = min(CC, q.C - c0);   // multiple of 8
      const int kc = 9 * cc;
      const int kcp = (kc + 31) & ~31;    // MFMA steps of 32: the tail is zero in LDS
      if (chunks > 1 || st == (int)blockIdx.x) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < rows_f * kcp; idx += THREADS) {
          const int j = idx / kcp, e = idx % kcp;
          int dst = e;
          bf16_t v = 0;
          if (e < kc) {
            const int cl = e / 9, tap = e - 9 * cl;
            dst = tap * cc + cl;
            if (j < r) v = F[((long)j * q.C + c0 + cl) * 9 + tap];
          }
          Fs[j * pitch + dst] = v;
        }
        __syncthreads();
      }
      int tap = 0, cl = 8 * g;  // this lane's k = ks + 8 g as (tap, channel of the chunk)
      while (cl >= cc) { cl -= cc; ++tap; }
      for (int ks = 0; ks < kcp; ks += 32) {
        bf16x8 a = zero8();
        if (row_ok && tap < 9) {
          const int ky = tap / 3, kx = tap - 3 * ky;
          const int iy = iy0 + ky, ix = ix0 + kx;
          if ((unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W)
            a = *reinterpret_cast<const bf16x8*>(X + ((long)(b * q.H + iy) * q.W + ix) * ldx + c0 + cl);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < nct) {
            const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(Fs + (t * 16 + lr) * pitch + ks + 8 * g);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, acc[t], 0, 0, 0);
          }
        }
        cl += 32;
        while (cl >= cc) { cl -= cc; ++tap; }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = t * 16 + lr;
      if (t < nct && col < r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long rr = (long)st * 64 + wave * 16 + 4 * g + i;
          if (rr < M) Hout[rr * r + col] = f32_to_bf16(acc[t][i] * scale);
        }
      }
    }
  }
}

// Input gradient of the 3x3 down factor, gather form: D^T = F dH^T as in lora_up_add_kernel — the factor is the A operand (rows =
// input channels ci), the B operand's column is an input pixel and its k runs over (tap, c) JOINTLY, 9 r padded once to a multiple
// of 32: element (tap, c) is dh[(b, (iy + 1 - ky) / s, (ix + 1 - kx) / s)][c] where that output pixel exists, else zero.  A lane
// gathers the B fragments of DX_KSTEPS K-steps at a time (registers) and reuses them for every channel tile; it ends up with
// four consecutive channels of one pixel: one 8-byte store, or one 8-byte read-modify-write when accumulating.  blockIdx.y owns NC
// channels (at most DX_TILES tiles of 16, each with its own accumulator) whose factor rows sit in LDS as Fs[n][tap * r + c]
// (pitch 9 r rounded up to 32, + 8: 16 m + 4 dwords).
constexpr int DX_KSTEPS = 4, DX_TILES = UP_NC / 16;

__global__ __launch_bounds__(THREADS) void lora_conv_dx_kernel(const bf16_t* __restrict__ DH, const bf16_t* __restrict__ F,
                                                               bf16_t* __restrict__ DX, long lddx, ConvGeom q, int M, int r, int NC,
                                                               int accumulate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Fs = reinterpret_cast<bf16_t*>(smem);
  const int kt = 9 * r, kp = (kt + 31) & ~31, pitch = kp + 8, ksteps = kp >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int n_base = blockIdx.y * NC;
  const int nc = min(NC, q.C - n_base);  // multiple of 8
  const int ntiles = (nc + 15) >> 4;
  for (int idx = threadIdx.x; idx < ntiles * 16 * pitch; idx += THREADS) Fs[idx] = 0;
  __syncthreads();
  for (int idx = threadIdx.x; idx < r * nc * 9; idx += THREADS) {  // global reads along (n, tap): 9 nc contiguous elements per c
    const int c = idx / (nc * 9), rem = idx - c * nc * 9;
    const int n = rem / 9, tap = rem - 9 * n;
    Fs[n * pitch + tap * r + c] = F[((long)c * q.C + n_base + n) * 9 + tap];
  }
  __syncthreads();
  const int stripes = (M + 63) >> 6;
  for (int st = blockIdx.x; st < stripes; st += gridDim.x) {
    const int m = st * 64 + wave * 16 + lr;
    const bool ok = m < M;
    const int ix = m % q.W, iy = (m / q.W) % q.H, b = m / (q.W * q.H);
    // row of dh that tap (ky, kx) of this input pixel reads, -1 when there is none
    auto nbr = [&](int tap) -> long {
      const int ky = tap / 3, kx = tap - 3 * ky;
      int ty = iy + 1 - ky, tx = ix + 1 - kx;
      if (ty < 0 || tx < 0) return -1;
      if (q.s == 2) {
        if ((ty | tx) & 1) return -1;
        ty >>= 1;
        tx >>= 1;
      }
      if (ty >= q.Ho || tx >= q.Wo) return -1;
      return (long)(b * q.Ho + ty) * q.Wo + tx;
    };
    f32x4 acc[DX_TILES];
#pragma unroll
    for (int nt = 0; nt < DX_TILES; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kp; k0 += 32 * DX_KSTEPS) {  // DX_KSTEPS K-steps at a time: gather their B fragments, then every tile
      bf16x8 hb[DX_KSTEPS];
#pragma unroll
      for (int ks = 0; ks < DX_KSTEPS; ++ks) {
        hb[ks] = zero8();
        const int k = k0 + ks * 32 + 8 * g;
        if (ok && k < kt) {
          if ((r & 7) == 0) {  // the 8 ranks of one tap: one 16-byte load
            const int tap = k / r, c = k - tap * r;
            const long row = nbr(tap);
            if (row >= 0) hb[ks] = *reinterpret_cast<const bf16x8*>(DH + row * r + c);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              if (k + e < kt) {
                const int tap = (k + e) / r, c = k + e - tap * r;
                const long row = nbr(tap);
                if (row >= 0) hb[ks][e] = (short)DH[row * r + c];
              }
            }
          }
        }
      }
#pragma unroll
      for (int nt = 0; nt < DX_TILES; ++nt) {
        if (nt < ntiles) {
#pragma unroll
          for (int ks = 0; ks < DX_KSTEPS; ++ks) {
            if (k0 + ks * 32 < kp) {
              const bf16x8 a = *reinterpret_cast<const bf16x8*>(Fs + (nt * 16 + lr) * pitch + k0 + ks * 32 + 8 * g);
              acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, hb[ks], acc[nt], 0, 0, 0);
            }
          }
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < DX_TILES; ++nt) {
      const int n = nt * 16 + 4 * g;  // this lane: dx[m][n_base + n .. + 3]
      if (nt < ntiles && ok && n < nc) {
        bf16_t* dp = DX + (long)m * lddx + n_base + n;
        s16x4 d;
        if (accumulate) {
          d = *reinterpret_cast<const s16x4*>(dp);
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = (short)f32_to_bf16(acc[nt][e] + bf16_to_f32((bf16_t)d[e]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = (short)f32_to_bf16(acc[nt][e]);
        }
        *reinterpret_cast<s16x4*>(dp) = d;
      }
    }
  }
}

// Weight gradient of the 3x3 down factor: lora_wgrad_kernel over the VIRTUAL matrix T[m][j = tap * C + ci] = x[nbr(m, tap)][ci]
// (m an output pixel), never materialised: a thread's 8 columns of the T tile are 8 channels of one tap (C % 8 == 0) of its row's
// neighbour pixel, one 16-byte load or zeros.  Same tiles, pitches and row splits as lora_wgrad_kernel; partial sums go to
// ws[split][j][c] and lora_conv_wgrad_reduce_kernel adds the splits in order, writing out[c][ci][ky][kx] directly.
__global__ __launch_bounds__(THREADS) void lora_conv_wgrad_kernel(const bf16_t* __restrict__ X, long ldx, const bf16_t* __restrict__ U,
                                                                  float* __restrict__ ws, ConvGeom q, int M, int r,
                                                                  int rows_per_split) {
  __shared__ __attribute__((aligned(16))) bf16_t Ts[WG_ROWS * WG_TPITCH];
  __shared__ __attribute__((aligned(16))) bf16_t Us[MAX_RANK * WG_UPITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
  const int nct = (r + 15) >> 4, rows_u = nct << 4;
  const int J = 9 * q.C;
  const int j_base = blockIdx.x * WG_COLS;
  const int m_begin = blockIdx.y * rows_per_split;
  const int m_end = min(M, m_begin + rows_per_split);
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tm = threadIdx.x >> 3, tj = (threadIdx.x & 7) << 3;  // this thread's 8 elements of the T tile
  const int j_t = j_base + tj;
  const int tap_t = j_t / q.C, ci_t = j_t - tap_t * q.C;        // fixed for the whole reduction
  const int ky_t = tap_t / 3, kx_t = tap_t - 3 * ky_t;
  for (int m0 = m_begin; m0 < m_end; m0 += WG_ROWS) {
    __syncthreads();
    {
      const int m = m0 + tm;
      bf16x8 v = zero8();
      if (m < m_end && j_t < J) {
        const int ox = m % q.Wo, oy = (m / q.Wo) % q.Ho, b = m / (q.Wo * q.Ho);
        const int iy = oy * q.s + ky_t - 1, ix = ox * q.s + kx_t - 1;
        if ((unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W)
          v = *reinterpret_cast<const bf16x8*>(X + ((long)(b * q.H + iy) * q.W + ix) * ldx + ci_t);
      }
      s16x4* dst = reinterpret_cast<s16x4*>(Ts + tm * WG_TPITCH + tj);
      dst[0] = s16x4{v[0], v[1], v[2], v[3]};
      dst[1] = s16x4{v[4], v[5], v[6], v[7]};
    }
    for (int idx = threadIdx.x; idx < WG_ROWS * rows_u; idx += THREADS) {
      const int mm = idx / rows_u, c = idx % rows_u;
      const int m = m0 + mm;
      Us[c * WG_UPITCH + mm] = (m < m_end && c < r) ? U[(long)m * r + c] : (bf16_t)0;
    }
    __syncthreads();
    bf16x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (short)Ts[(8 * g + e) * WG_TPITCH + wave * 16 + lr];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nct) {
        const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(Us + (t * 16 + lr) * WG_UPITCH + 8 * g);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = t * 16 + lr;
    if (t < nct && c < r) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = j_base + wave * 16 + 4 * g + i;
        if (j < J) ws[((long)blockIdx.y * J + j) * r + c] = acc[t][i];
      }
    }
  }
}

// out[c][ci][tap] (+)= scale * (ws[0] + ws[1] + ... in split order)[j = tap * C + ci][c]
__global__ void lora_conv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int splits, int C, int r,
                                              int accumulate, float scale) {
  const long total = 9l * C * r;
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  float s = ws[idx];
  for (int k = 1; k < splits; ++k) s += ws[(long)k * total + idx];
  s *= scale;
  const int c = (int)(idx % r), j = (int)(idx / r);
  const int tap = j / C, ci = j - tap * C;
  const long o = ((long)c * C + ci) * 9 + tap;
  out[o] = accumulate ? out[o] + s : s;
}

inline int round_up(int v, int to) { return (v + to - 1) / to * to; }

// rows of one split of the tall reduction: about 1 024 workgroups in all, never fewer than 128 rows each
inline int wgrad_rows_per_split(int M, int J) {
  const int col_tiles = (J + WG_COLS - 1) / WG_COLS;
  const int want = 1024 / col_tiles < 1 ? 1 : 1024 / col_tiles;
  int rows = round_up((M + want - 1) / want, WG_ROWS);
  return rows < 128 ? 128 : rows;
}

inline bool bad_p(float p) { return !(p >= 0.f && p < 1.f); }

// shared argument checks of the three convolution-adapter entry points; fills the geometry
inline int conv_geom(const char* name, int B, int H, int W, int C, int r, int stride, ConvGeom* q) {
  CFHIP_REQUIRE(B > 0 && H > 0 && W > 0, "%s: B = %d, H = %d, W = %d must be positive", name, B, H, W);
  CFHIP_REQUIRE(C > 0 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", name, C);
  CFHIP_REQUIRE(r >= 1 && r <= MAX_RANK, "%s: rank %d outside 1 .. %d", name, r, MAX_RANK);
  CFHIP_REQUIRE(stride == 1 || stride == 2, "%s: stride %d (3x3 / pad 1 adapters run at stride 1 or 2)", name, stride);
  CFHIP_REQUIRE((long)B * H * W < (1l << 31) && 9l * C < (1l << 31), "%s: B H W = %ld rows do not fit 31 bits", name, (long)B * H * W);
  *q = ConvGeom{B, H, W, (H - 1) / stride + 1, (W - 1) / stride + 1, C, stride};
  return CFHIP_OK;
}

}  // namespace

extern "C" int cfhip_lora_down(const void* x, const void* f, void* h, int M, int K, int r, int64_t ldx, int64_t ldf, int f_trans,
                               float scale, float p, uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(x && f && h, "lora_down: null pointer");
  CFHIP_REQUIRE(M > 0 && K > 0 && K % 8 == 0, "lora_down: M = %d, K = %d (K must be a positive multiple of 8)", M, K);
  CFHIP_REQUIRE(r >= 1 && r <= MAX_RANK, "lora_down: rank %d outside 1 .. %d", r, MAX_RANK);
  CFHIP_REQUIRE(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "lora_down: x must be 16-byte aligned with a row stride that is a multiple of 8");
  if (f_trans) CFHIP_REQUIRE(ldf >= r, "lora_down: factor [K][r] with ldf = %ld < r", (long)ldf);
  else CFHIP_REQUIRE(ldf >= K && ldf % 8 == 0 && ((uintptr_t)f & 15) == 0, "lora_down: factor [r][K] must be 16-byte aligned with ldf %% 8 == 0");
  CFHIP_REQUIRE(!bad_p(p), "lora_down: p = %f must be in [0, 1)", (double)p);
  const int rows_f = round_up(r, 16);
  const int kc_max = LDS_BUDGET / (rows_f * 2) - 8;  // elements of K one LDS image holds
  const int kp = round_up(K, 32);
  const int KC = kp <= kc_max ? kp : kc_max / 128 * 128;
  const size_t lds = (size_t)rows_f * (KC + 8) * 2;
  const int stripes = (M + 63) / 64;
  const int grid = stripes < 1024 ? stripes : 1024;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float sc = p > 0.f ? scale / (1.0f - p) : scale;
  if (f_trans)
    hipLaunchKernelGGL(lora_down_kernel<true>, dim3(grid), dim3(THREADS), lds, s, (const bf16_t*)x, (long)ldx, (const bf16_t*)f,
                       (long)ldf, (bf16_t*)h, M, K, r, KC, sc, p, (unsigned long long)seed, (unsigned long long)offset);
  else
    hipLaunchKernelGGL(lora_down_kernel<false>, dim3(grid), dim3(THREADS), lds, s, (const bf16_t*)x, (long)ldx, (const bf16_t*)f,
                       (long)ldf, (bf16_t*)h, M, K, r, KC, sc, p, (unsigned long long)seed, (unsigned long long)offset);
  CFHIP_CHECK_LAUNCH("lora_down");
  return CFHIP_OK;
}

extern "C" int cfhip_lora_up_add(const void* h, const void* f, void* y, int y_is_f32, int M, int N, int r, int64_t ldf, int64_t ldy,
                                 int f_trans, float scale, float p, uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(h && f && y, "lora_up_add: null pointer");
  CFHIP_REQUIRE(M > 0 && N > 0 && N % 8 == 0, "lora_up_add: M = %d, N = %d (N must be a positive multiple of 8)", M, N);
  CFHIP_REQUIRE(r >= 1 && r <= MAX_RANK, "lora_up_add: rank %d outside 1 .. %d", r, MAX_RANK);
  CFHIP_REQUIRE(ldy >= N && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0, "lora_up_add: y must be 16-byte aligned with a row stride that is a multiple of 4");
  CFHIP_REQUIRE(ldf >= (f_trans ? N : r), "lora_up_add: ldf = %ld too small", (long)ldf);
  CFHIP_REQUIRE((r & 7) != 0 || ((uintptr_t)h & 15) == 0, "lora_up_add: h must be 16-byte aligned");
  CFHIP_REQUIRE(!bad_p(p), "lora_up_add: p = %f must be in [0, 1)", (double)p);
  const int kp = round_up(r, 32);
  const int col_blocks = (N + UP_NC - 1) / UP_NC;
  const size_t lds = (size_t)UP_NC * (kp + 8) * 2;
  const int stripes = (M + 63) / 64;
  int gx = 1024 / col_blocks < 1 ? 1 : 1024 / col_blocks;
  if (gx > stripes) gx = stripes;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float sc = p > 0.f ? scale / (1.0f - p) : scale;
#define CFHIP_LORA_UP(FT, YF)                                                                                                       \
  hipLaunchKernelGGL((lora_up_add_kernel<FT, YF>), dim3(gx, col_blocks), dim3(THREADS), lds, s, (const bf16_t*)h, (const bf16_t*)f, \
                     (long)ldf, y, (long)ldy, M, N, r, sc, p, (unsigned long long)seed, (unsigned long long)offset)
  if (f_trans) {
    if (y_is_f32) CFHIP_LORA_UP(true, true);
    else CFHIP_LORA_UP(true, false);
  } else {
    if (y_is_f32) CFHIP_LORA_UP(false, true);
    else CFHIP_LORA_UP(false, false);
  }
#undef CFHIP_LORA_UP
  CFHIP_CHECK_LAUNCH("lora_up_add");
  return CFHIP_OK;
}

extern "C" size_t cfhip_lora_wgrad_workspace(int M, int J, int r) {
  if (M <= 0 || J <= 0 || r <= 0) return 0;
  const int rows = wgrad_rows_per_split(M, J);
  const size_t splits = (size_t)((M + rows - 1) / rows);
  return splits * (size_t)J * (size_t)r * sizeof(float);
}

extern "C" int cfhip_lora_wgrad(const void* t, const void* u, float* out, int M, int J, int r, int64_t ldt, int out_trans,
                                int accumulate, float scale, float p, uint64_t seed, uint64_t offset, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CFHIP_REQUIRE(t && u && out, "lora_wgrad: null pointer");
  CFHIP_REQUIRE(M > 0 && J > 0 && J % 8 == 0, "lora_wgrad: M = %d, J = %d (J must be a positive multiple of 8)", M, J);
  CFHIP_REQUIRE(r >= 1 && r <= MAX_RANK, "lora_wgrad: rank %d outside 1 .. %d", r, MAX_RANK);
  CFHIP_REQUIRE(ldt >= J && ldt % 8 == 0 && ((uintptr_t)t & 15) == 0, "lora_wgrad: t must be 16-byte aligned with a row stride that is a multiple of 8");
  CFHIP_REQUIRE(!bad_p(p), "lora_wgrad: p = %f must be in [0, 1)", (double)p);
  const size_t need = cfhip_lora_wgrad_workspace(M, J, r);
  if (workspace == nullptr || workspace_bytes < need) {
    cfhip_set_error("lora_wgrad: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    return CFHIP_ERR_WORKSPACE;
  }
  const int rows = wgrad_rows_per_split(M, J);
  const int splits = (M + rows - 1) / rows;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lora_wgrad_kernel, dim3((J + WG_COLS - 1) / WG_COLS, splits), dim3(THREADS), 0, s, (const bf16_t*)t, (long)ldt,
                     (const bf16_t*)u, (float*)workspace, M, J, r, rows, p, (unsigned long long)seed, (unsigned long long)offset);
  CFHIP_CHECK_LAUNCH("lora_wgrad");
  const long total = (long)J * r;
  const float sc = p > 0.f ? scale / (1.0f - p) : scale;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)workspace, out,
                     splits, J, r, out_trans, accumulate, sc);
  CFHIP_CHECK_LAUNCH("lora_wgrad_reduce");
  return CFHIP_OK;
}

extern "C" int cfhip_lora_conv_down(const void* x, const void* f, void* h, int B, int H, int W, int C, int r, int stride, int64_t ldx,
                                    float scale, void* stream) {
  CFHIP_REQUIRE(x && f && h, "lora_conv_down: null pointer");
  ConvGeom q;
  if (int rc = conv_geom("lora_conv_down", B, H, W, C, r, stride, &q)) return rc;
  CFHIP_REQUIRE(ldx >= C && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "lora_conv_down: x must be 16-byte aligned with a row stride that is a multiple of 8");
  const int M = B * q.Ho * q.Wo;
  const int rows_f = round_up(r, 16);
  const int kc_max = LDS_BUDGET / (rows_f * 2) - 8;  // elements of K = (tap, channel) one LDS image holds
  const int CC = round_up(9 * C, 32) <= kc_max ? C : kc_max / 9 / 32 * 32;  // channels per chunk: all, or a multiple of 32 (>= 32)
  const size_t lds = (size_t)rows_f * (round_up(9 * CC, 32) + 8) * 2;
  const int stripes = (M + 63) / 64;
  const int grid = stripes < 1024 ? stripes : 1024;
  hipLaunchKernelGGL(lora_conv_down_kernel, dim3(grid), dim3(THREADS), lds, reinterpret_cast<hipStream_t>(stream), (const bf16_t*)x,
                     (long)ldx, (const bf16_t*)f, (bf16_t*)h, q, M, r, CC, scale);
  CFHIP_CHECK_LAUNCH("lora_conv_down");
  return CFHIP_OK;
}

extern "C" int cfhip_lora_conv_dx(const void* dh, const void* f, void* dx, int B, int H, int W, int C, int r, int stride,
                                  int64_t lddx, int accumulate, void* stream) {
  CFHIP_REQUIRE(dh && f && dx, "lora_conv_dx: null pointer");
  ConvGeom q;
  if (int rc = conv_geom("lora_conv_dx", B, H, W, C, r, stride, &q)) return rc;
  CFHIP_REQUIRE(lddx >= C && lddx % 8 == 0 && ((uintptr_t)dx & 15) == 0, "lora_conv_dx: dx must be 16-byte aligned with a row stride that is a multiple of 8");
  CFHIP_REQUIRE((r & 7) != 0 || ((uintptr_t)dh & 15) == 0, "lora_conv_dx: dh must be 16-byte aligned");
  const int M = B * H * W;
  const int pitch = round_up(9 * r, 32) + 8;
  int NC = LDS_BUDGET / (2 * pitch) / 16 * 16;  // channels whose factor rows one LDS image holds (>= 48)
  if (NC > UP_NC) NC = UP_NC;
  const int col_blocks = (C + NC - 1) / NC;
  const size_t lds = (size_t)(C < NC ? round_up(C, 16) : NC) * pitch * 2;
  const int stripes = (M + 63) / 64;
  int gx = 1024 / col_blocks < 1 ? 1 : 1024 / col_blocks;
  if (gx > stripes) gx = stripes;
  hipLaunchKernelGGL(lora_conv_dx_kernel, dim3(gx, col_blocks), dim3(THREADS), lds, reinterpret_cast<hipStream_t>(stream),
                     (const bf16_t*)dh, (const bf16_t*)f, (bf16_t*)dx, (long)lddx, q, M, r, NC, accumulate);
  CFHIP_CHECK_LAUNCH("lora_conv_dx");
  return CFHIP_OK;
}

extern "C" size_t cfhip_lora_conv_wgrad_workspace(int B, int H, int W, int C, int r, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || r <= 0 || (stride != 1 && stride != 2)) return 0;
  const long M = (long)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  if (M >= (1l << 31) || 9l * C >= (1l << 31)) return 0;
  const int rows = wgrad_rows_per_split((int)M, 9 * C);
  const size_t splits = (size_t)((M + rows - 1) / rows);
  return splits * 9 * (size_t)C * (size_t)r * sizeof(float);
}

extern "C" int cfhip_lora_conv_wgrad(const void* dh, const void* x, float* out, int B, int H, int W, int C, int r, int stride,
                                     int64_t ldx, int accumulate, float scale, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  CFHIP_REQUIRE(dh && x && out, "lora_conv_wgrad: null pointer");
  ConvGeom q;
  if (int rc = conv_geom("lora_conv_wgrad", B, H, W, C, r, stride, &q)) return rc;
  CFHIP_REQUIRE(ldx >= C && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "lora_conv_wgrad: x must be 16-byte aligned with a row stride that is a multiple of 8");
  const size_t need = cfhip_lora_conv_wgrad_workspace(B, H, W, C, r, stride);
  if (workspace == nullptr || workspace_bytes < need) {
    cfhip_set_error("lora_conv_wgrad: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    return CFHIP_ERR_WORKSPACE;
  }
  const int M = B * q.Ho * q.Wo, J = 9 * C;
  const int rows = wgrad_rows_per_split(M, J);
  const int splits = (M + rows - 1) / rows;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lora_conv_wgrad_kernel, dim3((J + WG_COLS - 1) / WG_COLS, splits), dim3(THREADS), 0, s, (const bf16_t*)x, (long)ldx,
                     (const bf16_t*)dh, (float*)workspace, q, M, r, rows);
  CFHIP_CHECK_LAUNCH("lora_conv_wgrad");
  const long total = (long)J * r;
  hipLaunchKernelGGL(lora_conv_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)workspace, out,
                     splits, C, r, accumulate, scale);
  CFHIP_CHECK_LAUNCH("lora_conv_wgrad_reduce");
  return CFHIP_OK;
}
