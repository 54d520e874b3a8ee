// Head poolers of the mixed stacks (reference mixed_stacks/poolers.py:27-39 `SequencePooler`, api.py:369-402 the "mean" Lambda and the
// PreNorm head around either): out[b, :] = sum_t p[b, t] * y[b, t, :] over the rows of one sample, with y = LayerNorm(x) (NORM form) or
// y = x (plain form) and p = 1 / T (mean) or p = softmax_t(y . w_p + b_p) (sequence).  One pass over the residual stream: the
// normalised tensor and the probabilities never reach memory.
//
// Work split.  Forward: one workgroup of four waves per (sample, chunk of rows); wave w takes rows w, w + 4, ... of the chunk.  The 64
// lanes span D in groups of four consecutive elements (one 16-byte load of f32, one 8-byte load of bf16), NV = ceil(D / 256) groups per
// lane, so a whole row lives in 4 NV registers of each lane (D <= 2048: 32).  gamma, beta and w_p are staged in LDS once per workgroup
// and read back with 16-byte LDS loads for every row.  Per row: mean and variance (two-pass, from the registers) by wave reductions, the
// logit by a third, then the online-softmax update of the wave's (max, denominator, accumulator[D]) — the accumulator is another 4 NV
// registers.  The four waves then meet in LDS (the staging area is dead by then and is reused) and are merged in wave order.  A sample
// that is one chunk is finished there; otherwise (max, denominator, accumulator) goes to the workspace and pool_merge_kernel folds the
// chunks of a sample in chunk order.  Mean mode is the same walk with every logit 0: max 0, denominator = rows, lse = log T.
// Backward: workgroups walk the same (sample, chunk) items, recompute y from x, mean, rstd, form p from the saved lse, and push
// dy = p dout + dlogit w_p through the LayerNorm backward of the row; parameter gradients stay in registers over all rows of a workgroup,
// are merged across waves in LDS, written as one partial per workgroup and summed by pool_reduce_kernel in workgroup order.
// Every sum has a fixed order: no atomics, results repeat bit for bit.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int WAVES = 4, THREADS = 64 * WAVES;
// the CU count of the MI355X as a compile-time constant: the chunking must not depend on the device a call happens to run on (the
// workspace query takes no device; results are bit-identical from box to box)
constexpr int CUS = 256;
constexpr int MIN_CHUNK = 4 * WAVES;  // automatic chunks keep four rows per wave
constexpr int MAX_D = 2048;
constexpr int BWD_GROUPS = 4 * CUS;   // most workgroups (= partial rows of the parameter gradients) a backward launches
constexpr int HEAD = 4;               // floats in front of a chunk's accumulator in the workspace: max, denominator, two unused

struct PoolFwd {
  const void* x;
  const float *gamma, *beta, *w, *bp;
  float *out, *lse, *mean, *rstd, *ws;
  long ld_x;
  int B, T, D, seq, chunk, chunks;
  float eps;
};

struct PoolBwd {
  const float *dout, *out, *lse;
  const void* x;
  const float *gamma, *beta, *w, *bp, *mean, *rstd;
  void* dx;
  float* part;
  float* dest[4];  // dgamma, dbeta, dw_p, db_p (null: not wanted)
  long ld_x, ld_dx;
  int B, T, D, seq, chunk, chunks, items, groups, want_ln, want_w, acc_mask;
};

template <bool XF32>
__device__ __forceinline__ f32x4 ld_row4(const void* row, int col) {
  if (XF32) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(row) + col);
  const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(row) + col);
  return f32x4{bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
}
template <bool XF32>
__device__ __forceinline__ void st_row4(void* row, int col, f32x4 v) {
  if (XF32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(row) + col) = v;
  else *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(row) + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}
__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ const f32x4& lds4(const float* s, int col) { return *reinterpret_cast<const f32x4*>(s + col); }

// gamma | beta | w_p -> smem[0, D) | [D, 2 D) | [2 D, 3 D) (only what the form and the mode read)
__device__ __forceinline__ void stage_params(float* smem, const float* gamma, const float* beta, const float* w, int D) {
  for (int c = threadIdx.x * 4; c < D; c += THREADS * 4) {
    if (gamma != nullptr) {
      *reinterpret_cast<f32x4*>(smem + c) = *reinterpret_cast<const f32x4*>(gamma + c);
      *reinterpret_cast<f32x4*>(smem + D + c) = *reinterpret_cast<const f32x4*>(beta + c);
    }
    if (w != nullptr) *reinterpret_cast<f32x4*>(smem + 2 * D + c) = *reinterpret_cast<const f32x4*>(w + c);
  }
  __syncthreads();
}

template <int NV, bool XF32>
__global__ __launch_bounds__(THREADS) void pool_fwd_kernel(PoolFwd p) {
  extern __shared__ __align__(16) float smem[];  // 4 D floats: the staged parameters, then one accumulator per wave
  __shared__ float s_m[WAVES], s_l[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.D;
  const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
  const bool norm = p.gamma != nullptr, seq = p.seq != 0;
  stage_params(smem, p.gamma, p.beta, seq ? p.w : nullptr, D);
  const float *s_g = smem, *s_b = smem + D, *s_w = smem + 2 * D;
  const int t0 = chunk * p.chunk, t1 = min(p.T, t0 + p.chunk);
  const float bp = seq && p.bp != nullptr ? *p.bp : 0.f, inv_d = 1.0f / (float)D;
  float m = seq ? -INFINITY : 0.f, l = 0.f;
  f32x4 acc[NV];
#pragma unroll
  for (int g = 0; g < NV; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = t0 + wave; t < t1; t += WAVES) {
    const long r = (long)b * p.T + t;
    const char* row = reinterpret_cast<const char*>(p.x) + r * p.ld_x * (XF32 ? 4 : 2);
    f32x4 v[NV];
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int col = (g * 64 + lane) * 4;
      v[g] = col < D ? ld_row4<XF32>(row, col) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (norm) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < NV; ++g) s += sum4(v[g]);
      const float mean = wave_sum(s) * inv_d;
      float q = 0.f;
#pragma unroll
      for (int g = 0; g < NV; ++g) {
        const f32x4 d = v[g] - mean;
        if ((g * 64 + lane) * 4 < D) q += sum4(d * d);
      }
      const float rstd = rsqrtf(wave_sum(q) * inv_d + p.eps);
      if (lane == 0) {
        p.mean[r] = mean;
        p.rstd[r] = rstd;
      }
#pragma unroll
      for (int g = 0; g < NV; ++g) {
        const int col = (g * 64 + lane) * 4;
        if (col < D) v[g] = (v[g] - mean) * rstd * lds4(s_g, col) + lds4(s_b, col);
      }
    }
    float pr = 1.0f;
    if (seq) {
      float d = 0.f;
#pragma unroll
      for (int g = 0; g < NV; ++g) {
        const int col = (g * 64 + lane) * 4;
        if (col < D) d += sum4(v[g] * lds4(s_w, col));
      }
      const float logit = wave_sum(d) + bp;
      if (logit > m) {  // the max moves: what the wave holds is rescaled to it
        const float sc = expf(m - logit);
        l *= sc;
#pragma unroll
        for (int g = 0; g < NV; ++g) acc[g] *= sc;
        m = logit;
      }
      pr = expf(logit - m);
    }
    l += pr;
#pragma unroll
    for (int g = 0; g < NV; ++g) acc[g] += v[g] * pr;
  }
  __syncthreads();  // every wave is done with the staged parameters
#pragma unroll
  for (int g = 0; g < NV; ++g) {
    const int col = (g * 64 + lane) * 4;
    if (col < D) *reinterpret_cast<f32x4*>(smem + wave * D + col) = acc[g];
  }
  if (lane == 0) {
    s_m[wave] = m;
    s_l[wave] = l;
  }
  __syncthreads();
  float M = s_m[0];  // wave 0 always has a row
  for (int w = 1; w < WAVES; ++w) M = fmaxf(M, s_m[w]);
  float sc[WAVES], L = 0.f;
  for (int w = 0; w < WAVES; ++w) {
    sc[w] = expf(s_m[w] - M);  // a wave without a row: exp(-inf) = 0 (mean mode: its denominator is 0)
    L += s_l[w] * sc[w];
  }
  float* ws = p.ws + (long)blockIdx.x * (D + HEAD);
  for (int c = threadIdx.x * 4; c < D; c += THREADS * 4) {
    f32x4 o = lds4(smem, c) * sc[0];
    for (int w = 1; w < WAVES; ++w) o += lds4(smem + w * D, c) * sc[w];
    if (p.chunks == 1) *reinterpret_cast<f32x4*>(p.out + (long)b * D + c) = o / L;
    else *reinterpret_cast<f32x4*>(ws + HEAD + c) = o;
  }
  if (threadIdx.x == 0) {
    if (p.chunks == 1) {
      p.lse[b] = M + logf(L);
    } else {
      ws[0] = M;
      ws[1] = L;
    }
  }
}

// the chunks of one sample, in chunk order: (max, denominator, accumulator) -> out, lse
__global__ __launch_bounds__(THREADS) void pool_merge_kernel(PoolFwd p) {
  const int b = blockIdx.x, D = p.D;
  const float* ws = p.ws + (long)b * p.chunks * (D + HEAD);
  float M = ws[0];
  for (int c = 1; c < p.chunks; ++c) M = fmaxf(M, ws[(long)c * (D + HEAD)]);
  const int c0 = threadIdx.x * 4, c1 = c0 + THREADS * 4;  // D <= 2048: two column groups per thread at most
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
  float L = 0.f;
  for (int c = 0; c < p.chunks; ++c) {
    const float* part = ws + (long)c * (D + HEAD);
    const float sc = expf(part[0] - M);
    L += part[1] * sc;
    if (c0 < D) o0 += *reinterpret_cast<const f32x4*>(part + HEAD + c0) * sc;
    if (c1 < D) o1 += *reinterpret_cast<const f32x4*>(part + HEAD + c1) * sc;
  }
  if (c0 < D) *reinterpret_cast<f32x4*>(p.out + (long)b * D + c0) = o0 / L;
  if (c1 < D) *reinterpret_cast<f32x4*>(p.out + (long)b * D + c1) = o1 / L;
  if (threadIdx.x == 0) p.lse[b] = M + logf(L);
}

// one register array of per-wave parameter-gradient sums -> the workgroup's partial (waves added in wave order)
template <int NV>
__device__ __forceinline__ void fold_waves(float* smem, const f32x4 (&a)[NV], float* dst, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int g = 0; g < NV; ++g) {
    const int col = (g * 64 + lane) * 4;
    if (col < D) *reinterpret_cast<f32x4*>(smem + wave * D + col) = a[g];
  }
  __syncthreads();
  for (int c = threadIdx.x * 4; c < D; c += THREADS * 4) {
    f32x4 s = lds4(smem, c);
    for (int w = 1; w < WAVES; ++w) s += lds4(smem + w * D, c);
    *reinterpret_cast<f32x4*>(dst + c) = s;
  }
}

template <int NV, bool XF32>
__global__ __launch_bounds__(THREADS) void pool_bwd_kernel(PoolBwd p) {
  extern __shared__ __align__(16) float smem[];  // 4 D floats, as in the forward
  __shared__ float s_bp[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.D;
  const bool norm = p.gamma != nullptr, seq = p.seq != 0;
  stage_params(smem, p.gamma, p.beta, seq ? p.w : nullptr, D);
  const float *s_g = smem, *s_b = smem + D, *s_w = smem + 2 * D;
  const float bp = seq && p.bp != nullptr ? *p.bp : 0.f, inv_d = 1.0f / (float)D, p_mean = 1.0f / (float)p.T;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 a_g[NV], a_b[NV], a_w[NV];
  float a_bp = 0.f;
#pragma unroll
  for (int g = 0; g < NV; ++g) a_g[g] = a_b[g] = a_w[g] = zero;
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int b = item / p.chunks, chunk = item - b * p.chunks;
    f32x4 go[NV];
    float cb = 0.f;
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int col = (g * 64 + lane) * 4;
      go[g] = col < D ? *reinterpret_cast<const f32x4*>(p.dout + (long)b * D + col) : zero;
      if (seq && col < D) cb += sum4(go[g] * *reinterpret_cast<const f32x4*>(p.out + (long)b * D + col));
    }
    cb = wave_sum(cb);  // c_b = out[b] . dout[b]: every wave forms it the same way
    const float lse = seq ? p.lse[b] : 0.f;
    const int t0 = chunk * p.chunk, t1 = min(p.T, t0 + p.chunk);
    for (int t = t0 + wave; t < t1; t += WAVES) {
      const long r = (long)b * p.T + t;
      const char* row = reinterpret_cast<const char*>(p.x) + r * p.ld_x * (XF32 ? 4 : 2);
      f32x4 xh[NV], y[NV];
      float rstd = 1.0f;
#pragma unroll
      for (int g = 0; g < NV; ++g) xh[g] = y[g] = zero;
      if (norm || seq) {  // (mean mode of the plain form reads no x: dx = dout / T)
        const float mean = norm ? p.mean[r] : 0.f;
        if (norm) rstd = p.rstd[r];
#pragma unroll
        for (int g = 0; g < NV; ++g) {
          const int col = (g * 64 + lane) * 4;
          if (col < D) {
            y[g] = ld_row4<XF32>(row, col);
            if (norm) {
              xh[g] = (y[g] - mean) * rstd;
              y[g] = xh[g] * lds4(s_g, col) + lds4(s_b, col);
            }
          }
        }
      }
      float pr = p_mean, dl = 0.f;
      if (seq) {
        float d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int g = 0; g < NV; ++g) {
          const int col = (g * 64 + lane) * 4;
          if (col < D) d1 += sum4(y[g] * lds4(s_w, col));
          d2 += sum4(y[g] * go[g]);
        }
        pr = expf(wave_sum(d1) + bp - lse);
        dl = pr * (wave_sum(d2) - cb);
        a_bp += dl;
      }
      f32x4 dy[NV];
      float r1 = 0.f, r2 = 0.f;
#pragma unroll
      for (int g = 0; g < NV; ++g) {
        const int col = (g * 64 + lane) * 4;
        dy[g] = go[g] * pr;
        if (seq && col < D) {
          dy[g] += lds4(s_w, col) * dl;
          a_w[g] += y[g] * dl;
        }
        if (norm && col < D) {
          a_g[g] += dy[g] * xh[g];
          a_b[g] += dy[g];
          dy[g] *= lds4(s_g, col);  // from here on: the gradient of xhat
          r1 += sum4(dy[g]);
          r2 += sum4(dy[g] * xh[g]);
        }
      }
      if (p.dx == nullptr) continue;
      if (norm) {
        r1 = wave_sum(r1) * inv_d;
        r2 = wave_sum(r2) * inv_d;
      }
      char* drow = reinterpret_cast<char*>(p.dx) + r * p.ld_dx * (XF32 ? 4 : 2);
#pragma unroll
      for (int g = 0; g < NV; ++g) {
        const int col = (g * 64 + lane) * 4;
        if (col < D) st_row4<XF32>(drow, col, norm ? (dy[g] - r1 - xh[g] * r2) * rstd : dy[g]);
      }
    }
  }
  if (!p.want_ln && !p.want_w) return;
  float* dst = p.part + (long)blockIdx.x * (3 * D + HEAD);
  if (p.want_ln) {
    fold_waves<NV>(smem, a_g, dst, D);
    fold_waves<NV>(smem, a_b, dst + D, D);
  }
  if (p.want_w) {
    fold_waves<NV>(smem, a_w, dst + 2 * D, D);
    if (lane == 0) s_bp[wave] = a_bp;
    __syncthreads();
    if (threadIdx.x == 0) dst[3 * D] = ((s_bp[0] + s_bp[1]) + s_bp[2]) + s_bp[3];
  }
}

// partials [groups][3 D + HEAD] -> dgamma | dbeta | dw_p | db_p, workgroups added in workgroup order; a null destination is skipped
__global__ __launch_bounds__(THREADS) void pool_reduce_kernel(PoolBwd p) {
  const int i = blockIdx.x * THREADS + threadIdx.x, D = p.D;
  if (i > 3 * D) return;
  const int k = i / D;  // 0 .. 2: the [D] vectors; 3 (i == 3 D): db_p
  float* dest = p.dest[k];
  if (dest == nullptr) return;
  float s = 0.f;
  for (int g = 0; g < p.groups; ++g) s += p.part[(long)g * (3 * D + HEAD) + i];
  dest += i - k * D;
  *dest = (p.acc_mask >> k) & 1 ? *dest + s : s;
}

// rows per chunk: the caller's, or the smallest that still gives every CU a workgroup (never fewer than MIN_CHUNK rows)
int pick_chunk(int B, int T, int chunk_rows) {
  if (chunk_rows > 0) return chunk_rows < T ? chunk_rows : T;
  const int want = (CUS + B - 1) / B;
  int rows = (T + want - 1) / want;
  if (rows < MIN_CHUNK) rows = MIN_CHUNK;
  return rows < T ? rows : T;
}

bool misaligned(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) != 0; }

// two byte ranges share a byte (a null operand is absent)
bool meets(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (a == nullptr || b == nullptr) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int geometry(const char* who, int B, int T, int D, int mode, int chunk_rows) {
  CFHIP_REQUIRE(B > 0 && T > 0 && D > 0, "%s: empty problem (B %d, T %d, D %d)", who, B, T, D);
  CFHIP_REQUIRE(D % 4 == 0, "%s: D = %d is not a multiple of 4 (lanes hold groups of four elements)", who, D);
  CFHIP_REQUIRE(D <= MAX_D, "%s: D = %d exceeds %d (a row is held in registers)", who, D, MAX_D);
  CFHIP_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d (0 mean, 1 sequence)", who, mode);
  CFHIP_REQUIRE(chunk_rows >= 0, "%s: chunk_rows = %d (0 = automatic)", who, chunk_rows);
  CFHIP_REQUIRE((long)B * T <= (long)INT_MAX, "%s: B * T = %ld rows exceed the 31-bit row index", who, (long)B * T);
  return CFHIP_OK;
}

int check_rows(const char* who, const char* name, const void* ptr, int64_t ld, int D) {
  CFHIP_REQUIRE(ptr != nullptr, "%s: %s is null", who, name);
  CFHIP_REQUIRE(!misaligned(ptr), "%s: %s is not 16-byte aligned", who, name);
  CFHIP_REQUIRE(ld >= D && ld % 4 == 0, "%s: ld_%s = %ld must be a multiple of 4 and at least D = %d", who, name, (long)ld, D);
  return CFHIP_OK;
}

size_t rows_bytes(int B, int T, int D, int64_t ld, int is_f32) { return (size_t)(((long)B * T - 1) * ld + D) * (is_f32 ? 4 : 2); }

// kernel<NV, XF32> for this D and row type, on 4 D floats of dynamic LDS
#define POOL_LAUNCH(kernel, p, x_is_f32, grid, stream)                                                                      \
  do {                                                                                                                      \
    const int nv__ = ((p).D + 255) / 256;                                                                                   \
    const size_t lds__ = (size_t)WAVES * (p).D * sizeof(float);                                                             \
    const dim3 g__(grid), b__(THREADS);                                                                                     \
    if (x_is_f32) {                                                                                                         \
      if (nv__ <= 1) hipLaunchKernelGGL((kernel<1, true>), g__, b__, lds__, stream, p);                                     \
      else if (nv__ <= 2) hipLaunchKernelGGL((kernel<2, true>), g__, b__, lds__, stream, p);                                \
      else if (nv__ <= 4) hipLaunchKernelGGL((kernel<4, true>), g__, b__, lds__, stream, p);                                \
      else hipLaunchKernelGGL((kernel<8, true>), g__, b__, lds__, stream, p);                                               \
    } else {                                                                                                                \
      if (nv__ <= 1) hipLaunchKernelGGL((kernel<1, false>), g__, b__, lds__, stream, p);                                    \
      else if (nv__ <= 2) hipLaunchKernelGGL((kernel<2, false>), g__, b__, lds__, stream, p);                               \
      else if (nv__ <= 4) hipLaunchKernelGGL((kernel<4, false>), g__, b__, lds__, stream, p);                               \
      else hipLaunchKernelGGL((kernel<8, false>), g__, b__, lds__, stream, p);                                              \
    }                                                                                                                       \
  } while (0)

}  // namespace

extern "C" size_t cfhip_pool_rows_workspace(int B, int T, int D, int chunk_rows, int backward) {
  if (B <= 0 || T <= 0 || D <= 0 || D % 4 != 0 || D > MAX_D || chunk_rows < 0 || (long)B * T > (long)INT_MAX) return 0;
  const int rows = pick_chunk(B, T, chunk_rows);
  const long items = (long)B * ((T + rows - 1) / rows);
  if (backward) return (size_t)(items < BWD_GROUPS ? items : BWD_GROUPS) * (size_t)(3 * D + HEAD) * sizeof(float);
  return items == B ? 0 : (size_t)items * (size_t)(D + HEAD) * sizeof(float);
}

extern "C" int cfhip_pool_rows_fwd(const void* x, int x_is_f32, int64_t ld_x, const float* gamma, const float* beta, const float* w_p,
                                   const float* b_p, float* out, float* lse, float* mean, float* rstd, int B, int T, int D, int mode,
                                   float eps, int chunk_rows, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pool_rows_fwd";
  int rc = geometry(who, B, T, D, mode, chunk_rows);
  if (rc == CFHIP_OK) rc = check_rows(who, "x", x, ld_x, D);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(out != nullptr && lse != nullptr && !misaligned(out), "%s: out (16-byte aligned) and lse must be given", who);
  CFHIP_REQUIRE((gamma == nullptr) == (beta == nullptr), "%s: gamma and beta come together (both null: the plain form)", who);
  CFHIP_REQUIRE(gamma == nullptr || (mean != nullptr && rstd != nullptr), "%s: the NORM form saves mean and rstd", who);
  CFHIP_REQUIRE(mode == 0 || w_p != nullptr, "%s: sequence mode needs w_p", who);
  CFHIP_REQUIRE(!misaligned(gamma) && !misaligned(beta) && !misaligned(w_p), "%s: gamma, beta and w_p must be 16-byte aligned", who);
  const size_t xb = rows_bytes(B, T, D, ld_x, x_is_f32), need = cfhip_pool_rows_workspace(B, T, D, chunk_rows, 0);
  CFHIP_REQUIRE(!meets(out, (size_t)B * D * 4, x, xb) && !meets(lse, (size_t)B * 4, x, xb) && !meets(mean, (size_t)B * T * 4, x, xb) &&
                    !meets(rstd, (size_t)B * T * 4, x, xb) && !meets(workspace, need, x, xb) && !meets(workspace, need, out, (size_t)B * D * 4),
                "%s: out, lse, mean, rstd or the workspace overlaps x (or the workspace overlaps out)", who);
  CFHIP_REQUIRE(need == 0 || (workspace != nullptr && !misaligned(workspace) && workspace_bytes >= need),
                "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", who, need, workspace_bytes);
  PoolFwd p = {};
  p.x = x; p.gamma = gamma; p.beta = beta; p.w = w_p; p.bp = mode ? b_p : nullptr;
  p.out = out; p.lse = lse; p.mean = mean; p.rstd = rstd; p.ws = reinterpret_cast<float*>(workspace);
  p.ld_x = ld_x; p.B = B; p.T = T; p.D = D; p.seq = mode; p.eps = eps;
  p.chunk = pick_chunk(B, T, chunk_rows);
  p.chunks = (T + p.chunk - 1) / p.chunk;
  CFHIP_REQUIRE((long)B * p.chunks <= (long)INT_MAX, "%s: B * chunks = %ld workgroups", who, (long)B * p.chunks);
  POOL_LAUNCH(pool_fwd_kernel, p, x_is_f32, (unsigned)(B * p.chunks), (hipStream_t)stream);
  CFHIP_CHECK_LAUNCH(who);
  if (p.chunks > 1) {
    hipLaunchKernelGGL(pool_merge_kernel, dim3((unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, p);
    CFHIP_CHECK_LAUNCH("pool_rows_fwd (merge)");
  }
  return CFHIP_OK;
}

extern "C" int cfhip_pool_rows_bwd(const float* dout, const float* out, const float* lse, const void* x, int x_is_f32, int64_t ld_x,
                                   const float* gamma, const float* beta, const float* w_p, const float* b_p, const float* mean,
                                   const float* rstd, void* dx, int64_t ld_dx, float* dgamma, float* dbeta, float* dw_p, float* db_p,
                                   int accumulate_mask, int B, int T, int D, int mode, int chunk_rows, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const char* who = "pool_rows_bwd";
  int rc = geometry(who, B, T, D, mode, chunk_rows);
  if (rc == CFHIP_OK) rc = check_rows(who, "x", x, ld_x, D);
  if (rc == CFHIP_OK && dx != nullptr) rc = check_rows(who, "dx", dx, ld_dx, D);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(dout != nullptr && !misaligned(dout), "%s: dout must be given, 16-byte aligned", who);
  CFHIP_REQUIRE((gamma == nullptr) == (beta == nullptr), "%s: gamma and beta come together (both null: the plain form)", who);
  CFHIP_REQUIRE(gamma == nullptr || (mean != nullptr && rstd != nullptr), "%s: the NORM form reads the saved mean and rstd", who);
  CFHIP_REQUIRE(gamma != nullptr || (dgamma == nullptr && dbeta == nullptr), "%s: the plain form has no dgamma / dbeta", who);
  CFHIP_REQUIRE(mode == 1 || (dw_p == nullptr && db_p == nullptr), "%s: mean mode has no dw_p / db_p", who);
  CFHIP_REQUIRE(mode == 0 || (w_p != nullptr && out != nullptr && lse != nullptr && !misaligned(out)),
                "%s: sequence mode needs w_p, out (16-byte aligned) and lse", who);
  CFHIP_REQUIRE(!misaligned(gamma) && !misaligned(beta) && !misaligned(w_p), "%s: gamma, beta and w_p must be 16-byte aligned", who);
  CFHIP_REQUIRE(dx != nullptr || dgamma != nullptr || dbeta != nullptr || dw_p != nullptr || db_p != nullptr, "%s: no output asked for", who);
  PoolBwd p = {};
  p.want_ln = dgamma != nullptr || dbeta != nullptr;
  p.want_w = dw_p != nullptr || db_p != nullptr;
  p.chunk = pick_chunk(B, T, chunk_rows);
  p.chunks = (T + p.chunk - 1) / p.chunk;
  CFHIP_REQUIRE((long)B * p.chunks <= (long)INT_MAX, "%s: B * chunks = %ld work items", who, (long)B * p.chunks);
  p.items = B * p.chunks;
  p.groups = p.items < BWD_GROUPS ? p.items : BWD_GROUPS;
  const size_t xb = rows_bytes(B, T, D, ld_x, x_is_f32), need = (size_t)p.groups * (size_t)(3 * D + HEAD) * sizeof(float);
  if (dx != nullptr) {
    const size_t db = rows_bytes(B, T, D, ld_dx, x_is_f32);
    CFHIP_REQUIRE(!meets(dx, db, x, xb) && !meets(dx, db, dout, (size_t)B * D * 4) && !meets(dx, db, out, (size_t)B * D * 4),
                  "%s: dx overlaps x, dout or out", who);
  }
  if (p.want_ln || p.want_w) {
    CFHIP_REQUIRE(workspace != nullptr && !misaligned(workspace) && workspace_bytes >= need,
                  "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", who, need, workspace_bytes);
    float* dests[4] = {dgamma, dbeta, dw_p, db_p};
    const void* ins[4] = {x, dx, dout, workspace};
    const size_t in_bytes[4] = {xb, dx != nullptr ? rows_bytes(B, T, D, ld_dx, x_is_f32) : 0, (size_t)B * D * 4, need};
    for (int k = 0; k < 4; ++k)
      for (int i = 0; i < 4; ++i)
        CFHIP_REQUIRE(!meets(dests[k], k < 3 ? (size_t)D * 4 : 4, ins[i], in_bytes[i]),
                      "%s: a parameter gradient overlaps x, dx, dout or the workspace", who);
    CFHIP_REQUIRE(!meets(workspace, need, x, xb) && !meets(workspace, need, dx, in_bytes[1]) && !meets(workspace, need, dout, in_bytes[2]),
                  "%s: the workspace overlaps x, dx or dout", who);
    p.part = reinterpret_cast<float*>(workspace);
    for (int k = 0; k < 4; ++k) p.dest[k] = dests[k];
  }
  p.dout = dout; p.out = out; p.lse = lse; p.x = x; p.gamma = gamma; p.beta = beta; p.w = w_p; p.bp = mode ? b_p : nullptr;
  p.mean = mean; p.rstd = rstd; p.dx = dx; p.ld_x = ld_x; p.ld_dx = ld_dx;
  p.B = B; p.T = T; p.D = D; p.seq = mode; p.acc_mask = accumulate_mask;
  POOL_LAUNCH(pool_bwd_kernel, p, x_is_f32, (unsigned)p.groups, (hipStream_t)stream);
  CFHIP_CHECK_LAUNCH(who);
  if (p.want_ln || p.want_w) {
    hipLaunchKernelGGL(pool_reduce_kernel, dim3((unsigned)((3 * D + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, p);
    CFHIP_CHECK_LAUNCH("pool_rows_bwd (reduce)");
  }
  return CFHIP_OK;
}
