// Vector quantisation: the nearest-code search of VQCodebook.forward (modules/cv/common.py:362-400) without the
// rows x num_codes distance matrix the reference materialises (sum, einsum, add, argmin, gather: 1 GB of f32 at the zoo's
// ae/vq.f4 shape, written and read several times per step only to take an argmin).
//
//   score_j = sq_j - 2 dot_j,   dot_j = fmaf chain over d = 0 .. D - 1 from 0 of z_d e_jd,   sq_j = fmaf chain of e_jd^2
//   (|z|^2 is the same for every j of a row and left out); idx = the lowest j with the least score; z_q = scale * e_idx.
//
// How the codebook reaches the lanes: a workgroup of four waves holds 64 R rows (R = 1 or 2 per lane, all four
// waves hold the SAME rows in registers) and streams the codebook through LDS in chunks of cfhip_vq_chunk(D) codes, each code
// stored as [sq_j, e_j0 .. e_j(D'-1), 0 ..] on a stride of S floats (S a multiple of 4: 16-byte reads).  Wave w scans quarter w
// of every chunk; all 64 lanes read the same LDS address (a broadcast: one bank row, no conflict), so one 16-byte read feeds
// 4 R FMAs per lane.  The next chunk's global loads are in flight while the current one is scanned.  Each wave scans its
// codes in ascending j with a strict <; the four candidates of a row meet in LDS and the least (score, index) pair wins, which
// is the lowest index among the least scores: what one ascending scan of all N codes gives.
//
// D' = D for D <= 4, else the next power of two up to 64: the padding columns hold 0 in the registers and in LDS, and
// fmaf(0, 0, acc) = acc leaves every chain's value as it was.
#include "common.h"

namespace {

constexpr int VQ_THREADS = 256;
constexpr int VQ_WAVES = VQ_THREADS / 64;

constexpr int vq_padded_dim(int D) { return D <= 4 ? D : (D <= 8 ? 8 : (D <= 16 ? 16 : (D <= 32 ? 32 : 64))); }
constexpr int vq_stride(int DP) { return (DP + 1 + 3) / 4 * 4; }                                   // floats per code in LDS
constexpr int vq_chunk(int DP) { return CFHIP_VQ_LDS_FLOATS / vq_stride(DP) / VQ_WAVES * VQ_WAVES; }  // codes per chunk

__global__ void vq_code_sqnorm_kernel(const float* __restrict__ cb, float* __restrict__ out, int N, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const float* e = cb + (long)j * D;
  float sq = 0.f;
  for (int d = 0; d < D; ++d) sq = fmaf(e[d], e[d], sq);
  out[j] = sq;
}

template <int DP, int R>
__global__ __launch_bounds__(VQ_THREADS) void vq_nearest_kernel(const void* __restrict__ z, int z_is_f32, int channels_last,
                                                                 const float* __restrict__ cb, const float* __restrict__ code_sq,
                                                                 int64_t* __restrict__ indices, float* __restrict__ z_q, long rows,
                                                                 int D, long hw, int N, float scale) {
  constexpr int S = vq_stride(DP), CH = vq_chunk(DP), QUARTER = CH / VQ_WAVES;
  constexpr int PF = (CH * S + VQ_THREADS - 1) / VQ_THREADS;  // floats of a chunk each thread stages
  constexpr int UNR = S <= 4 ? 8 : (S <= 8 ? 4 : (S <= 20 ? 2 : 1));
  constexpr bool PIPE = S <= 20;
  __shared__ __attribute__((aligned(16))) float lds[(CH + 2 * UNR) * S];
  __shared__ float cand_s[VQ_WAVES][64 * R];
  __shared__ int cand_i[VQ_WAVES][64 * R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)blockIdx.x * (64 * R);

  // this lane's rows, padded with zeros to DP columns (a row past the end: all zeros, nothing is written for it)
  float zr[R][DP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long row = row0 + r * 64 + lane;
    const long b = row / hw, p = row - b * hw;
    const long at0 = channels_last ? row * D : b * D * hw + p, step = channels_last ? 1 : hw;
    if (z_is_f32) {  // (no branch around a load: a dead element reads z[0] and is replaced by 0)
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const bool live = row < rows && d < D;
        const float v = reinterpret_cast<const float*>(z)[live ? at0 + d * step : 0];
        zr[r][d] = live ? v : 0.f;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const bool live = row < rows && d < D;
        const float v = bf16_to_f32(reinterpret_cast<const bf16_t*>(z)[live ? at0 + d * step : 0]);
        zr[r][d] = live ? v : 0.f;
      }
    }
  }

  // element i of the chunk that starts at code j0: [sq | e_0 .. e_(D-1) | 0 ..] of code j0 + i / S; 0 past the last code
  auto fetch = [&](float (&pf)[PF], int j0) {
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int i = tid + t * VQ_THREADS;
      const int j = j0 + i / S, k = i % S;
      // no branch around the load (a dead element reads code_sq[0] and is replaced by 0): all PF loads are in flight together
      const bool live = i < CH * S && j < N && k <= D;
      const float* src = k == 0 ? code_sq + j : cb + ((long)j * D + (k - 1));
      const float v = *(live ? src : code_sq);
      pf[t] = live ? v : 0.f;
    }
  };

  float best[R];
  int best_j[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    best[r] = __builtin_inff();
    best_j[r] = 0;
  }

  float pf[PF];
  fetch(pf, 0);
  for (int j0 = 0; j0 < N; j0 += CH) {
    __syncthreads();  // every wave has finished with the previous chunk
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int i = tid + t * VQ_THREADS;
      if (i < CH * S) lds[i] = pf[t];
    }
    __syncthreads();
    if (j0 + CH < N) fetch(pf, j0 + CH);  // in flight during the scan
    const int left = N - j0;
    const int lo = wave * QUARTER;
    const int hi = min(lo + QUARTER, left);
    // UNR codes per group; with short records two groups alternate in registers so that the LDS reads of the next group are in
    // flight while the current one is scored (one wave per SIMD has nobody else to hide the read latency behind).  A group read
    // may start at `hi` and run past it: it stays inside the UNR spare records behind the chunk and is never scored.
    auto load = [&](float (&e)[UNR][S], int c) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
#pragma unroll
        for (int q = 0; q < S / 4; ++q) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(&lds[(c + u) * S + 4 * q]);
          e[u][4 * q] = v[0];
          e[u][4 * q + 1] = v[1];
          e[u][4 * q + 2] = v[2];
          e[u][4 * q + 3] = v[3];
        }
      }
    };
    auto score = [&](const float (&e)[UNR][S], int c, int count) {  // codes c .. c + count - 1, ascending
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (u < count) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) dot = fmaf(zr[r][d], e[u][1 + d], dot);
            const float sc = fmaf(-2.0f, dot, e[u][0]);
            if (sc < best[r]) {
              best[r] = sc;
              best_j[r] = j0 + c + u;
            }
          }
        }
      }
    };
    int c = lo;
    float ea[UNR][S];
    if constexpr (PIPE) {
      float eb[UNR][S];
      load(ea, c);
      for (;;) {
        if (c + UNR > hi) break;
        load(eb, c + UNR);
        score(ea, c, UNR);
        c += UNR;
        if (c + UNR > hi) break;
        load(ea, c + UNR);
        score(eb, c, UNR);
        c += UNR;
      }
    } else {
      for (; c + UNR <= hi; c += UNR) {
        load(ea, c);
        score(ea, c, UNR);
      }
    }
    if (c < hi) {  // fewer than UNR codes left
      load(ea, c);
      score(ea, c, hi - c);
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    cand_s[wave][r * 64 + lane] = best[r];
    cand_i[wave][r * 64 + lane] = best_j[r];
  }
  __syncthreads();
  if (tid < 64 * R) {
    const long row = row0 + tid;
    if (row < rows) {
      float bs = cand_s[0][tid];
      int bj = cand_i[0][tid];
#pragma unroll
      for (int w = 1; w < VQ_WAVES; ++w) {
        const float s = cand_s[w][tid];
        const int j = cand_i[w][tid];
        if (s < bs || (s == bs && j < bj)) {
          bs = s;
          bj = j;
        }
      }
      indices[row] = (int64_t)bj;
      if (z_q != nullptr) {  // contiguous NCHW
        const long b = row / hw, p = row - b * hw;
        for (int d = 0; d < D; ++d) z_q[(b * D + d) * hw + p] = scale * cb[(long)bj * D + d];
      }
    }
  }
}

template <int DP>
void vq_launch(bool two_rows, long rows, hipStream_t stream, const void* z, int z_is_f32, int channels_last, const float* cb,
               const float* code_sq, int64_t* indices, float* z_q, int D, long hw, int N, float scale) {
  if (two_rows) {
    hipLaunchKernelGGL((vq_nearest_kernel<DP, 2>), dim3((unsigned)((rows + 127) / 128)), dim3(VQ_THREADS), 0, stream, z, z_is_f32,
                       channels_last, cb, code_sq, indices, z_q, rows, D, hw, N, scale);
  } else {
    hipLaunchKernelGGL((vq_nearest_kernel<DP, 1>), dim3((unsigned)((rows + 63) / 64)), dim3(VQ_THREADS), 0, stream, z, z_is_f32,
                       channels_last, cb, code_sq, indices, z_q, rows, D, hw, N, scale);
  }
}

}  // namespace

extern "C" int cfhip_vq_chunk(int D) {
  if (D < 1 || D > CFHIP_VQ_MAX_DIM) return 0;
  return vq_chunk(vq_padded_dim(D));
}

extern "C" int cfhip_vq_code_sqnorm(const float* codebook, float* out, int N, int D, void* stream) {
  CFHIP_REQUIRE(codebook && out, "vq_code_sqnorm: null codebook or output");
  CFHIP_REQUIRE(N >= 1, "vq_code_sqnorm: N = %d codes (at least 1)", N);
  CFHIP_REQUIRE(D >= 1 && D <= CFHIP_VQ_MAX_DIM, "vq_code_sqnorm: D = %d outside [1, %d]", D, CFHIP_VQ_MAX_DIM);
  CFHIP_REQUIRE(((uintptr_t)codebook & 3) == 0 && ((uintptr_t)out & 3) == 0, "vq_code_sqnorm: misaligned operand");
  hipLaunchKernelGGL(vq_code_sqnorm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codebook, out, N, D);
  CFHIP_CHECK_LAUNCH("vq_code_sqnorm");
  return CFHIP_OK;
}

extern "C" int cfhip_vq_nearest(const void* z, int z_is_f32, int channels_last, const float* codebook, const float* code_sq,
                                int64_t* indices, float* z_q, int64_t B, int D, int64_t hw, int N, float scale_factor,
                                void* stream) {
  CFHIP_REQUIRE(z && codebook && code_sq && indices, "vq_nearest: null z, codebook, code_sq or indices");
  CFHIP_REQUIRE(B > 0 && hw > 0, "vq_nearest: empty tensor");
  CFHIP_REQUIRE(N >= 1, "vq_nearest: N = %d codes (at least 1)", N);
  CFHIP_REQUIRE(D >= 1 && D <= CFHIP_VQ_MAX_DIM, "vq_nearest: D = %d outside [1, %d]", D, CFHIP_VQ_MAX_DIM);
  CFHIP_REQUIRE(B * hw <= ((int64_t)1 << 36) / D, "vq_nearest: B * hw = %lld rows of D = %d is beyond the supported size",
                (long long)(B * hw), D);
  CFHIP_REQUIRE(((uintptr_t)z & (z_is_f32 ? 3 : 1)) == 0 && ((uintptr_t)codebook & 3) == 0 && ((uintptr_t)code_sq & 3) == 0 &&
                    ((uintptr_t)indices & 7) == 0 && ((uintptr_t)z_q & 3) == 0,
                "vq_nearest: misaligned operand");
  const long rows = (long)(B * hw);
  // two rows per lane halve the LDS reads per FMA; one row per lane while that is what it takes to give every CU two workgroups
  const bool two = rows >= 2L * 64 * CFHIP_VQ_TWO_ROWS_MIN_GROUPS;
  const hipStream_t s = (hipStream_t)stream;
#define VQ_CASE(DP)                                                                                                    \
  case DP:                                                                                                             \
    vq_launch<DP>(two, rows, s, z, z_is_f32, channels_last, codebook, code_sq, indices, z_q, D, (long)hw, N, scale_factor); \
    break;
  switch (vq_padded_dim(D)) {
    VQ_CASE(1)
    VQ_CASE(2)
    VQ_CASE(3)
    VQ_CASE(4)
    VQ_CASE(8)
    VQ_CASE(16)
    VQ_CASE(32)
    VQ_CASE(64)
  }
#undef VQ_CASE
  CFHIP_CHECK_LAUNCH("vq_nearest");
  return CFHIP_OK;
}
