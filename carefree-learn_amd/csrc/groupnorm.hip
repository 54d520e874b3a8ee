// GroupNorm (+ a per-(b, c) additive term in front, + SiLU behind) of the UNet's residual blocks (convs/residual.py:154-253):
//   net = conv1(..) + Linear(SiLU(t))[:, :, None, None];  net = SiLU(GroupNorm32(net)).
// x' = x + add[b][c] is what gets normalised; two-pass statistics (mean, then centred sum of squares) in fp32.
//
//   NCHW, x [B][C][inner]:  scalar kernels  — one workgroup per (b, group), any `inner`, any alignment, any channel count;
//                           vector kernels  — the same workgroup, 8 elements per lane per access;
//                           split kernels   — the (b, group) cut into slices along `inner`, one workgroup each.
//     The vector and split kernels are ONE set of loops over (channel of the group, 8-element vector of a range [j0, j1)):
//     the gn_slice_* functions below; the per-element arithmetic of all three forms is gn_norm_act / gn_xhat_dn / gn_dx.
//   NHWC, x [B][inner][C]:  group and slice kernels, further down.
#include "common.h"
#include <type_traits>

namespace {

constexpr int GN_MAX_CG = CFHIP_GN_MAX_CG;  // channels per group the backward vector / split kernels hold partial sums for in LDS

// ---- the arithmetic of one element ---------------------------------------------------------------------------------
__device__ __forceinline__ float gn_norm_act(float v, float ad, float mean, float rstd, float ga, float be, int silu) {
  float r = ((v + ad) - mean) * rstd * ga + be;
  if (silu) r = silu_f(r);
  return r;
}
// xhat, and dL/d(normalised value): dy, times SiLU'(xhat * gamma + beta) when the forward applied SiLU
__device__ __forceinline__ void gn_xhat_dn(float v, float dyv, float ad, float mu, float rs, float ga, float be, int silu, float& xh,
                                           float& dn) {
  xh = (v + ad - mu) * rs;
  dn = dyv;
  if (silu) dn *= silu_grad_f(xh * ga + be);
}
// dx = rstd * (dn * gamma - s1 / n - xhat * s2 / n),  s1 = sum(dn * gamma), s2 = sum(dn * gamma * xhat) over the group
__device__ __forceinline__ float gn_dx(float xh, float dn, float rs, float ga, float s1, float s2, float inv_n) {
  return rs * (dn * ga - s1 * inv_n - xh * s2 * inv_n);
}
__device__ __forceinline__ float gn_fold4(const float (&p)[4]) { return (p[0] + p[1]) + (p[2] + p[3]); }  // the four waves' partials

// ---- scalar kernels: a flat walk over the group's cg * inner elements, block_sum per reduction ----------------------
template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_fwd_kernel(const void* __restrict__ x, const float* __restrict__ add,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, int C, int G, int inner, float eps,
                                                     int silu, int affine_bs) {
  __shared__ float red[4];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  gamma += (long)b * affine_bs;  // per-sample affine (scale-shift norm): gamma / beta are [B][C] when affine_bs == C
  beta += (long)b * affine_bs;
  const int cg = C / G;
  const long base = ((long)b * C + (long)g * cg) * inner;
  const long n = (long)cg * inner;
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = (int)(i / inner);
    s += ld_act(x, base + i, IN_F32) + (add != nullptr ? add[(long)b * C + g * cg + c] : 0.f);
  }
  const float mean = block_sum(s, red) / (float)n;
  float q = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = (int)(i / inner);
    const float d = ld_act(x, base + i, IN_F32) + (add != nullptr ? add[(long)b * C + g * cg + c] : 0.f) - mean;
    q += d * d;
  }
  const float rstd = rsqrtf(block_sum(q, red) / (float)n + eps);
  if (threadIdx.x == 0) {
    mean_out[blockIdx.x] = mean;
    rstd_out[blockIdx.x] = rstd;
  }
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = g * cg + (int)(i / inner);
    const float ad = add != nullptr ? add[(long)b * C + c] : 0.f;
    y[base + i] = f32_to_bf16(gn_norm_act(ld_act(x, base + i, IN_F32), ad, mean, rstd, gamma[c], beta[c], silu));
  }
}

// dx (bf16), partial dgamma / dbeta per (b, group) block [B][C] (reduced over b by the caller's column reduce),
// dadd[b][c] = sum_inner dx (when the forward had an additive term)
template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_bwd_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                     const float* __restrict__ add, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                     float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                                     float* __restrict__ dadd, int C, int G, int inner, int silu, int affine_bs) {
  __shared__ float red[4];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  const int cg = C / G;
  const long base = ((long)b * C + (long)g * cg) * inner;
  const long n = (long)cg * inner;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  // pass 1: per-channel dgamma / dbeta partials and the two group sums
  float s1 = 0.f, s2 = 0.f;
  for (int cl = 0; cl < cg; ++cl) {
    const int c = g * cg + cl;
    const float ad = add != nullptr ? add[(long)b * C + c] : 0.f;
    const float ga = gamma[c], be = beta[c];
    float sg = 0.f, sb = 0.f;
    for (int j = threadIdx.x; j < inner; j += blockDim.x) {
      const long o = base + (long)cl * inner + j;
      float xh, dn;
      gn_xhat_dn(ld_act(x, o, IN_F32), bf16_to_f32(dy[o]), ad, mu, rs, ga, be, silu, xh, dn);
      sg += dn * xh;
      sb += dn;
    }
    sg = block_sum(sg, red);
    sb = block_sum(sb, red);
    if (threadIdx.x == 0) {
      dgamma_part[(long)b * C + c] = sg;
      dbeta_part[(long)b * C + c] = sb;
    }
    s1 += sb * ga;
    s2 += sg * ga;
  }
  const float inv_n = 1.f / (float)n;
  // pass 2: dx
  for (int cl = 0; cl < cg; ++cl) {
    const int c = g * cg + cl;
    const float ad = add != nullptr ? add[(long)b * C + c] : 0.f;
    const float ga = gamma[c], be = beta[c];
    float sd = 0.f;
    for (int j = threadIdx.x; j < inner; j += blockDim.x) {
      const long o = base + (long)cl * inner + j;
      float xh, dn;
      gn_xhat_dn(ld_act(x, o, IN_F32), bf16_to_f32(dy[o]), ad, mu, rs, ga, be, silu, xh, dn);
      const float d = gn_dx(xh, dn, rs, ga, s1, s2, inv_n);
      dx[o] = f32_to_bf16(d);
      sd += d;
    }
    if (dadd != nullptr) {
      sd = block_sum(sd, red);
      if (threadIdx.x == 0) dadd[(long)b * C + c] = sd;
    }
  }
}

// ---- vector and split kernels: inner % 8 == 0, 16-byte aligned rows ---------------------------------------------------
// Same arithmetic as the scalar kernels, 8 elements per lane per load (one 16-byte load of bf16, two of f32) and no integer
// division in the loops; the second and third pass over a group (80 KB - 1.3 MB) come out of L2.  UNet 64^2 x 8: the scalar
// forms took 74 / 116 us per call, 11.5 ms of a 101 ms step (profiles/r01/prof_unet64_b8_implicit_summary.txt).
//
// Split form: the vector kernels run ONE workgroup per (sample, group): B * G = 32 workgroups for the batch-1 256^2 UNet step (a
// tenth of the chip: 61 + 61 launches took 11.7 + 17.8 ms of a 533 ms step, profiles/r03/prof_unet256_b1_summary.txt) and
// one 4-wave workgroup per CU at 64^2 x 8.  There the (sample, group) is cut into S slices along `inner`: the statistics kernel
// writes one (mean, M2) pair per slice — a local two-pass over the slice (second pass out of L2) — and every workgroup of the
// apply kernel merges the S pairs of its group in slice order (Chan's parallel-variance update: deterministic, no cancellation)
// before it normalises its own slice.  Backward: per-slice per-channel sums (dn * xhat, dn) -> merged per channel by the apply
// kernel, which also leaves per-slice sums of dx for the time-embedding gradient (reduced by gn_split_dadd_kernel).

// What one workgroup works on: the 8-element vectors [j0, j1) of every channel of group g of sample b — slice sl of S; the
// one-workgroup kernels are the slice (0, 1), all inner / 8 vectors.
struct GnSlice {
  int b, cg, c0, inner, j0, j1;  // c0 = g * cg: the group's first channel
  long row, base;                // of the group's first channel in the [B][C] arrays / first element in x, y, dy, dx
};
__device__ __forceinline__ int gn_slice_begin(int sl, int S, int inner8) { return (int)((long)sl * inner8 / S); }
__device__ __forceinline__ GnSlice gn_slice(int bg, int C, int G, int inner, int sl, int S) {
  GnSlice s;
  s.b = bg / G;
  s.cg = C / G;
  s.c0 = (bg - s.b * G) * s.cg;
  s.inner = inner;
  s.j0 = gn_slice_begin(sl, S, inner >> 3);
  s.j1 = gn_slice_begin(sl + 1, S, inner >> 3);
  s.row = (long)s.b * C + s.c0;
  s.base = s.row * inner;
  return s;
}
__device__ __forceinline__ float gn_slice_inv_n(const GnSlice& s) { return 1.f / ((float)s.cg * (float)(s.j1 - s.j0) * 8.f); }

// (mean, M2 = centred sum of squares) of the slice: two passes, the second out of L2
template <bool IN_F32>
__device__ __forceinline__ void gn_slice_stats(const void* __restrict__ x, const float* __restrict__ add, const GnSlice& s, float* red,
                                               float& mean, float& m2) {
  const float inv_n = gn_slice_inv_n(s);
  float sum = 0.f;
  for (int cl = 0; cl < s.cg; ++cl) {
    const float ad = add != nullptr ? add[s.row + cl] : 0.f;
    for (int j = s.j0 + threadIdx.x; j < s.j1; j += 256) {
      float v[8];
      ld_act8<IN_F32>(x, s.base + (long)cl * s.inner + (long)j * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[e] + ad;
    }
  }
  mean = block_sum(sum, red) * inv_n;
  float q = 0.f;
  for (int cl = 0; cl < s.cg; ++cl) {
    const float ad = (add != nullptr ? add[s.row + cl] : 0.f) - mean;
    for (int j = s.j0 + threadIdx.x; j < s.j1; j += 256) {
      float v[8];
      ld_act8<IN_F32>(x, s.base + (long)cl * s.inner + (long)j * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[e] + ad;
        q += d * d;
      }
    }
  }
  m2 = block_sum(q, red);
}

// y = [SiLU](normalised slice)
template <bool IN_F32>
__device__ __forceinline__ void gn_slice_normalize(const void* __restrict__ x, const float* __restrict__ add,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   bf16_t* __restrict__ y, const GnSlice& s, float mean, float rstd, int silu) {
  for (int cl = 0; cl < s.cg; ++cl) {
    const float ad = add != nullptr ? add[s.row + cl] : 0.f;
    const float ga = gamma[s.c0 + cl], be = beta[s.c0 + cl];
    for (int j = s.j0 + threadIdx.x; j < s.j1; j += 256) {
      float v[8];
      const long o = s.base + (long)cl * s.inner + (long)j * 8;
      ld_act8<IN_F32>(x, o, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = gn_norm_act(v[e], ad, mean, rstd, ga, be, silu);
      st_bf16x8(y, o, v);
    }
  }
}

// Backward.  The per-channel sums are reduced per WAVE inside the channel loop (shuffles only) and parked in LDS; the workgroup
// synchronises once per pass instead of 4-6 times per channel, so the loads of the next channel overlap the arithmetic of this
// one.  Channels per group <= GN_MAX_CG (the UNet's widest: 2560 / 32).
// part[0 / 1][cl][wave] = the wave's sum(dn * xhat) / sum(dn) over the slice's elements of channel cl
template <bool IN_F32>
__device__ __forceinline__ void gn_slice_bwd_sums(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                  const float* __restrict__ add, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const GnSlice& s, float mu, float rs, int silu,
                                                  float (&part)[2][GN_MAX_CG][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int cl = 0; cl < s.cg; ++cl) {
    const float ad = add != nullptr ? add[s.row + cl] : 0.f;
    const float ga = gamma[s.c0 + cl], be = beta[s.c0 + cl];
    float sg = 0.f, sb = 0.f;
    for (int j = s.j0 + threadIdx.x; j < s.j1; j += 256) {
      const long o = s.base + (long)cl * s.inner + (long)j * 8;
      float v[8], d[8];
      ld_act8<IN_F32>(x, o, v);
      ld_act8<false>(dy, o, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float xh, dn;
        gn_xhat_dn(v[e], d[e], ad, mu, rs, ga, be, silu, xh, dn);
        sg += dn * xh;
        sb += dn;
      }
    }
    sg = wave_sum(sg);
    sb = wave_sum(sb);
    if (lane == 0) {
      part[0][cl][wave] = sg;
      part[1][cl][wave] = sb;
    }
  }
}
// dx of the slice; with want_dadd, dsum[cl][wave] = the wave's sum of dx over the slice's elements of channel cl — of the fp32
// values, as in the scalar kernel (the bf16 rounding happens at the store only)
template <bool IN_F32>
__device__ __forceinline__ void gn_slice_bwd_dx(const bf16_t* __restrict__ dy, const void* __restrict__ x, const float* __restrict__ add,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, bf16_t* __restrict__ dx,
                                                const GnSlice& s, float mu, float rs, float s1, float s2, int silu, bool want_dadd,
                                                float (&dsum)[GN_MAX_CG][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_n = 1.f / ((float)s.cg * (float)s.inner);
  for (int cl = 0; cl < s.cg; ++cl) {
    const float ad = add != nullptr ? add[s.row + cl] : 0.f;
    const float ga = gamma[s.c0 + cl], be = beta[s.c0 + cl];
    float sd = 0.f;
    for (int j = s.j0 + threadIdx.x; j < s.j1; j += 256) {
      const long o = s.base + (long)cl * s.inner + (long)j * 8;
      float v[8], d[8];
      ld_act8<IN_F32>(x, o, v);
      ld_act8<false>(dy, o, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float xh, dn;
        gn_xhat_dn(v[e], d[e], ad, mu, rs, ga, be, silu, xh, dn);
        d[e] = gn_dx(xh, dn, rs, ga, s1, s2, inv_n);
        sd += d[e];
      }
      st_bf16x8(dx, o, d);
    }
    if (want_dadd) {
      sd = wave_sum(sd);
      if (lane == 0) dsum[cl][wave] = sd;
    }
  }
}
// Thread t < cg holds its channel's group-wide (sg, sb) = (sum(dn * xhat), sum(dn)): the parameter-gradient partials go out (from
// one workgroup of the group: `write`), and every thread gets s1 = sum(sb * gamma), s2 = sum(sg * gamma) over the group.
__device__ __forceinline__ void gn_bwd_group_sums(float sg, float sb, const float* __restrict__ gamma, const GnSlice& s, bool write,
                                                  float* __restrict__ dgamma_part, float* __restrict__ dbeta_part, float* red, float& s1,
                                                  float& s2) {
  float t1 = 0.f, t2 = 0.f;
  if ((int)threadIdx.x < s.cg) {
    if (write) {
      dgamma_part[s.row + threadIdx.x] = sg;
      dbeta_part[s.row + threadIdx.x] = sb;
    }
    t1 = sb * gamma[s.c0 + threadIdx.x];
    t2 = sg * gamma[s.c0 + threadIdx.x];
  }
  s1 = block_sum(t1, red);
  s2 = block_sum(t2, red);
}

template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_fwd_vec_kernel(const void* __restrict__ x, const float* __restrict__ add,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                         float* __restrict__ rstd_out, int C, int G, int inner, float eps,
                                                         int silu, int affine_bs) {
  __shared__ float red[4];
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, 0, 1);
  gamma += (long)s.b * affine_bs;
  beta += (long)s.b * affine_bs;
  float mean, m2;
  gn_slice_stats<IN_F32>(x, add, s, red, mean, m2);
  const float rstd = rsqrtf(m2 * gn_slice_inv_n(s) + eps);
  if (threadIdx.x == 0) {
    mean_out[blockIdx.x] = mean;
    rstd_out[blockIdx.x] = rstd;
  }
  gn_slice_normalize<IN_F32>(x, add, gamma, beta, y, s, mean, rstd, silu);
}

template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_bwd_vec_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                         const float* __restrict__ add, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                         float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                                         float* __restrict__ dadd, int C, int G, int inner, int silu, int affine_bs) {
  __shared__ float red[4];
  __shared__ float part[2][GN_MAX_CG][4];
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, 0, 1);
  gamma += (long)s.b * affine_bs;
  beta += (long)s.b * affine_bs;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  gn_slice_bwd_sums<IN_F32>(dy, x, add, gamma, beta, s, mu, rs, silu, part);
  __syncthreads();
  float sg = 0.f, sb = 0.f, s1, s2;
  if ((int)threadIdx.x < s.cg) {
    sg = gn_fold4(part[0][threadIdx.x]);
    sb = gn_fold4(part[1][threadIdx.x]);
  }
  gn_bwd_group_sums(sg, sb, gamma, s, true, dgamma_part, dbeta_part, red, s1, s2);
  // (part[0] is free again: its pass-1 contents were consumed before the block_sum barriers)
  gn_slice_bwd_dx<IN_F32>(dy, x, add, gamma, beta, dx, s, mu, rs, s1, s2, silu, dadd != nullptr, part[0]);
  if (dadd != nullptr) {
    __syncthreads();
    if ((int)threadIdx.x < s.cg) dadd[s.row + threadIdx.x] = gn_fold4(part[0][threadIdx.x]);
  }
}

// forward workspace: [bg][slice] (mean, M2) pairs
template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_split_stats_kernel(const void* __restrict__ x, const float* __restrict__ add,
                                                             float* __restrict__ part, int C, int G, int inner, int S) {
  __shared__ float red[4];
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, blockIdx.y, S);
  float mean, m2;
  gn_slice_stats<IN_F32>(x, add, s, red, mean, m2);
  if (threadIdx.x == 0) {
    part[((long)blockIdx.x * S + blockIdx.y) * 2] = mean;
    part[((long)blockIdx.x * S + blockIdx.y) * 2 + 1] = m2;
  }
}

// (mean, rstd) of group `bg` from its S slice pairs; every thread computes the same values (S <= 64 pairs: 512 bytes)
__device__ __forceinline__ void gn_merge_slices(const float* __restrict__ part, int bg, int S, int cg, int inner8, float eps,
                                                float& mean, float& rstd) {
  float n = 0.f, mu = 0.f, m2 = 0.f;
  for (int sl = 0; sl < S; ++sl) {
    const float nb = (float)cg * (float)(gn_slice_begin(sl + 1, S, inner8) - gn_slice_begin(sl, S, inner8)) * 8.f;
    const float mb = part[((long)bg * S + sl) * 2], qb = part[((long)bg * S + sl) * 2 + 1];
    const float nt = n + nb, d = mb - mu;
    mu += d * (nb / nt);
    m2 += qb + d * d * (n * nb / nt);
    n = nt;
  }
  mean = mu;
  rstd = rsqrtf(m2 / n + eps);
}

template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_split_apply_kernel(const void* __restrict__ x, const float* __restrict__ add,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ part, bf16_t* __restrict__ y,
                                                             float* __restrict__ mean_out, float* __restrict__ rstd_out, int C,
                                                             int G, int inner, float eps, int silu, int affine_bs, int S) {
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, blockIdx.y, S);
  gamma += (long)s.b * affine_bs;
  beta += (long)s.b * affine_bs;
  float mean, rstd;
  gn_merge_slices(part, blockIdx.x, S, s.cg, inner >> 3, eps, mean, rstd);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    mean_out[blockIdx.x] = mean;
    rstd_out[blockIdx.x] = rstd;
  }
  gn_slice_normalize<IN_F32>(x, add, gamma, beta, y, s, mean, rstd, silu);
}

// backward workspace: [bg][slice][3][cg]: sum(dn * xhat), sum(dn), sum(dx) per channel of the slice
template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_split_bwd_stats_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                                 const float* __restrict__ add, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ part, int C,
                                                                 int G, int inner, int silu, int affine_bs, int S) {
  __shared__ float wpart[2][GN_MAX_CG][4];
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, blockIdx.y, S);
  gamma += (long)s.b * affine_bs;
  beta += (long)s.b * affine_bs;
  gn_slice_bwd_sums<IN_F32>(dy, x, add, gamma, beta, s, mean[blockIdx.x], rstd[blockIdx.x], silu, wpart);
  __syncthreads();
  if ((int)threadIdx.x < s.cg) {
    float* dst = part + ((long)blockIdx.x * S + blockIdx.y) * 3 * s.cg;
    dst[threadIdx.x] = gn_fold4(wpart[0][threadIdx.x]);
    dst[s.cg + threadIdx.x] = gn_fold4(wpart[1][threadIdx.x]);
  }
}

template <bool IN_F32>
__global__ __launch_bounds__(256) void gn_split_bwd_apply_kernel(const bf16_t* __restrict__ dy, const void* __restrict__ x,
                                                                 const float* __restrict__ add, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ part,
                                                                 bf16_t* __restrict__ dx, float* __restrict__ dgamma_part,
                                                                 float* __restrict__ dbeta_part, int want_dadd, int C, int G,
                                                                 int inner, int silu, int affine_bs, int S) {
  __shared__ float red[4];
  __shared__ float wpart[GN_MAX_CG][4];
  const GnSlice s = gn_slice(blockIdx.x, C, G, inner, blockIdx.y, S);
  gamma += (long)s.b * affine_bs;
  beta += (long)s.b * affine_bs;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  float sg = 0.f, sb = 0.f, s1, s2;
  if ((int)threadIdx.x < s.cg) {  // this thread's channel: the S slice sums in slice order
    for (int k = 0; k < S; ++k) {
      const float* src = part + ((long)blockIdx.x * S + k) * 3 * s.cg;
      sg += src[threadIdx.x];
      sb += src[s.cg + threadIdx.x];
    }
  }
  gn_bwd_group_sums(sg, sb, gamma, s, blockIdx.y == 0, dgamma_part, dbeta_part, red, s1, s2);
  gn_slice_bwd_dx<IN_F32>(dy, x, add, gamma, beta, dx, s, mu, rs, s1, s2, silu, want_dadd, wpart);
  if (want_dadd) {
    __syncthreads();
    if ((int)threadIdx.x < s.cg)
      part[((long)blockIdx.x * S + blockIdx.y) * 3 * s.cg + 2 * s.cg + threadIdx.x] = gn_fold4(wpart[threadIdx.x]);
  }
}

__global__ __launch_bounds__(128) void gn_split_dadd_kernel(const float* __restrict__ part, float* __restrict__ dadd, int C, int G,
                                                            int S) {
  const int bg = blockIdx.x;
  const int b = bg / G, g = bg - b * G;
  const int cg = C / G;
  if ((int)threadIdx.x < cg) {
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[((long)bg * S + k) * 3 * cg + 2 * cg + threadIdx.x];
    dadd[(long)b * C + g * cg + threadIdx.x] = s;
  }
}

// ---- GroupNorm on NHWC rows (round 5) ------------------------------------------------------------------------------------------
// x, y, dy, dx: bf16 [B][inner = H * W][C] — the layout the implicit-GEMM convolutions read and write, so a residual block that keeps
// its activations in it needs no NCHW <-> NHWC hop around every convolution (318 transposes per 64^2 x 8 UNet step).  Same
// arithmetic as the split NCHW kernels above (two-pass statistics per slice in fp32, Chan's merge in slice order, the additive
// per-(b, c) term in front, SiLU behind, per-sample partial sums of dgamma / dbeta, deterministic: no atomics), other indexing:
// a workgroup owns a slice of ROWS of one sample and all C channels; a thread owns KC slots of 8 consecutive channels (one
// 16-byte access per row and slot: rows are read and written as whole contiguous lines) and walks the rows rl, rl + RPP, ...;
// per-channel partial sums of the RPP row lanes meet in LDS in a fixed order, 32 threads fold channels into groups.
struct GnNhwcMap {
  int cg8, rpp, rl, nslot;  // 8-channel slots per row, row lanes, this thread's row lane, its number of slots (0: idle)
  int slot[2];              // its slots (channel = slot * 8)
};
__device__ __forceinline__ GnNhwcMap gn_nhwc_map(int C) {
  GnNhwcMap m;
  m.cg8 = C >> 3;
  const int t = threadIdx.x;
  if (m.cg8 >= 256) {
    m.rpp = 1; m.rl = 0;
    m.slot[0] = t; m.slot[1] = t + 256;
    m.nslot = (t < m.cg8 ? 1 : 0) + (t + 256 < m.cg8 ? 1 : 0);
  } else {
    m.rpp = 256 / m.cg8;
    m.rl = t / m.cg8;
    m.slot[0] = t - m.rl * m.cg8; m.slot[1] = 0;
    m.nslot = m.rl < m.rpp ? 1 : 0;
  }
  return m;
}
// rows [r0, r1) of slice sl of S over `inner` rows
__device__ __forceinline__ void gn_nhwc_rows(int inner, int S, int sl, int& r0, int& r1) {
  r0 = (int)((long)sl * inner / S);
  r1 = (int)((long)(sl + 1) * inner / S);
}
// The row walk of a thread: rows r0 + rl, r0 + rl + rpp, ... of the slice.  An idle thread (no slot) gets an EMPTY range instead of a
// branch around the body, and the loop is unrolled by 4: the four 16-byte loads of an unrolled body are independent and issue back
// to back (one load in flight per thread left these kernels at ~1.3 TB/s).
#define GN_NHWC_ROW_LOOP(r) _Pragma("unroll 4") for (int r = (m.nslot > 0 ? r0 + m.rl : r1); r < r1; r += m.rpp)
// per-channel values of all row lanes (acc[k][e] of every thread) -> chan[c] in LDS, summed over the row lanes in lane order
template <int KC>
__device__ __forceinline__ void gn_nhwc_fold(const GnNhwcMap& m, const float (&acc)[KC][8], float* lanes, float* chan, int C) {
  __syncthreads();  // (the buffers may still be read from a previous use)
#pragma unroll
  for (int k = 0; k < KC; ++k)
    if (k < m.nslot) {
#pragma unroll
      for (int e = 0; e < 8; ++e) lanes[m.rl * C + m.slot[k] * 8 + e] = acc[k][e];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int l = 0; l < m.rpp; ++l) s += lanes[l * C + c];
    chan[c] = s;
  }
  __syncthreads();
}

// ---- group form: one workgroup per (sample, group), ONE launch each way --------------------------------------------------------------
// With enough samples (B G >= ~128 workgroups: the 64^2 x 8 step has 256) a workgroup takes all rows of one group: its cpg
// channels are a 2 cpg-byte chunk of every row (20 .. 160 bytes), read as dwords — thread (rl, dw) owns the channel pair dw of the
// rows rl, rl + RPP, ... — so statistics, normalisation and the parameter-gradient sums all stay inside the workgroup: no slices,
// no workspace, no merge.  The 32 workgroups of a sample share every row's cache lines in L2.  cpg even, cpg <= 256.
// VW (round 5): a thread owns VW consecutive dwords (2 VW channels) of the chunk and reads them with ONE 4 VW-byte access — 4 when the
// chunk is a multiple of 16 bytes (cpg = 40, 80: C = 1 280, 2 560), 2 for multiples of 8 (cpg = 20, 60), else 1: a quarter / half of
// the memory instructions for the same bytes (the chunked accesses are what these kernels spend their time on, twice as much
// inside the step as alone).
template <int VW> struct GnVecT;
template <> struct GnVecT<1> { typedef unsigned T; };
template <> struct GnVecT<2> { typedef u32x2 T; };
template <> struct GnVecT<4> { typedef u32x4 T; };
template <int VW> struct GnWords {
  unsigned w[VW];
};
template <int VW> __device__ __forceinline__ GnWords<VW> gn_ldw(const bf16_t* p) {
  union { typename GnVecT<VW>::T v; GnWords<VW> w; } u;
  u.v = *reinterpret_cast<const typename GnVecT<VW>::T*>(p);
  return u.w;
}
template <int VW> __device__ __forceinline__ void gn_stw(bf16_t* p, const GnWords<VW>& w) {
  union { typename GnVecT<VW>::T v; GnWords<VW> w; } u;
  u.w = w;
  *reinterpret_cast<typename GnVecT<VW>::T*>(p) = u.v;
}
struct GnGroupMap {
  int vpr, rpp, rl, vs;  // vector slots per row chunk, row lanes, this thread's row lane / slot
  bool active;
};
template <int VW> __device__ __forceinline__ GnGroupMap gn_group_map(int cpg) {
  GnGroupMap m;
  m.vpr = (cpg >> 1) / VW;
  m.rpp = 256 / m.vpr;
  m.rl = threadIdx.x / m.vpr;
  m.vs = threadIdx.x - m.rl * m.vpr;
  m.active = m.rl < m.rpp;
  return m;
}

// RPT > 0: the thread's rows (at most RPT / VW of them, chosen by the launcher) stay in REGISTERS between the passes — one global read
// and one write per element instead of three reads and a write; RPT = 0: every pass re-reads (out of L2).
template <int RPT, int VW>
__global__ __launch_bounds__(256) void gn_nhwc_group_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ add,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                                float* __restrict__ rstd_out, int C, int G, int inner, float eps, int silu,
                                                                int affine_bs) {
  __shared__ float red[4];
  constexpr int NC = RPT > 0 ? RPT / VW : 1;
  constexpr int CH = 2 * VW;  // channels per thread
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int cpg = C / G;
  const GnGroupMap m = gn_group_map<VW>(cpg);
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  const int c0 = g * cpg + CH * m.vs;
  const long base = (long)b * inner * C + c0;
  float a[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) a[e] = (m.active && add != nullptr) ? add[(long)b * C + c0 + e] : 0.f;
  const float n = (float)cpg * (float)inner;
  auto row_sum = [&](const GnWords<VW>& w) {
    float t = 0.f;
#pragma unroll
    for (int v = 0; v < VW; ++v) t += (bf16lo(w.w[v]) + a[2 * v]) + (bf16hi(w.w[v]) + a[2 * v + 1]);
    return t;
  };
  GnWords<VW> cache[NC];
  float s = 0.f;
  if (RPT > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int r = m.rl + i * m.rpp;
#pragma unroll
      for (int v = 0; v < VW; ++v) cache[i].w[v] = 0u;
      if (m.active && r < inner) {
        cache[i] = gn_ldw<VW>(x + base + (long)r * C);
        s += row_sum(cache[i]);
      }
    }
  } else if (m.active) {
    for (int r = m.rl; r < inner; r += m.rpp) s += row_sum(gn_ldw<VW>(x + base + (long)r * C));
  }
  const float mean = block_sum(s, red) / n;
  auto row_sq = [&](const GnWords<VW>& w) {
    float t = 0.f;
#pragma unroll
    for (int v = 0; v < VW; ++v) {
      const float d0 = bf16lo(w.w[v]) + a[2 * v] - mean, d1 = bf16hi(w.w[v]) + a[2 * v + 1] - mean;
      t += d0 * d0 + d1 * d1;
    }
    return t;
  };
  float q = 0.f;
  if (RPT > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int r = m.rl + i * m.rpp;
      if (m.active && r < inner) q += row_sq(cache[i]);
    }
  } else if (m.active) {
    for (int r = m.rl; r < inner; r += m.rpp) q += row_sq(gn_ldw<VW>(x + base + (long)r * C));
  }
  const float rstd = rsqrtf(block_sum(q, red) / n + eps);
  if (threadIdx.x == 0) {
    mean_out[blockIdx.x] = mean;
    rstd_out[blockIdx.x] = rstd;
  }
  if (!m.active) return;
  float k[CH], o[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    k[e] = rstd * gamma[c0 + e];
    o[e] = beta[c0 + e] + (a[e] - mean) * k[e];
  }
  auto emit = [&](int r, const GnWords<VW>& w) {
    GnWords<VW> out;
#pragma unroll
    for (int v = 0; v < VW; ++v) {
      float v0 = fmaf(bf16lo(w.w[v]), k[2 * v], o[2 * v]), v1 = fmaf(bf16hi(w.w[v]), k[2 * v + 1], o[2 * v + 1]);
      if (silu) {
        v0 = silu_f(v0);
        v1 = silu_f(v1);
      }
      out.w[v] = pack_bf16x2(v0, v1);
    }
    gn_stw<VW>(y + base + (long)r * C, out);
  };
  if (RPT > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int r = m.rl + i * m.rpp;
      if (r < inner) emit(r, cache[i]);
    }
  } else {
    for (int r = m.rl; r < inner; r += m.rpp) emit(r, gn_ldw<VW>(x + base + (long)r * C));
  }
}

// LDS: lanes [rpp][cpg] (<= 512 VW floats) + ch [2][cpg]
template <int RPT, int VW>
__global__ __launch_bounds__(256) void gn_nhwc_group_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                const float* __restrict__ add, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                                float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                                                float* __restrict__ dadd, int C, int G, int inner, int silu, int affine_bs) {
  __shared__ float lanes[512 * VW];
  __shared__ float chA[256], chB[256], sums[2];
  constexpr int NC = RPT > 0 ? RPT / VW : 1;
  constexpr int CH = 2 * VW;
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int cpg = C / G;
  const GnGroupMap m = gn_group_map<VW>(cpg);
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  const int c0 = g * cpg + CH * m.vs;
  const long base = (long)b * inner * C + c0;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  float sh[CH], ga[CH], be[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    sh[e] = -mu;
    ga[e] = be[e] = 0.f;
    if (m.active) {
      if (add != nullptr) sh[e] += add[(long)b * C + c0 + e];
      ga[e] = gamma[c0 + e];
      be[e] = beta[c0 + e];
    }
  }
  // a per-channel quantity of every row lane -> ch[c], summed over the row lanes in lane order
  auto fold = [&](const float (&v)[CH], float* ch) {
    __syncthreads();
    if (m.active) {
#pragma unroll
      for (int e = 0; e < CH; ++e) lanes[m.rl * cpg + CH * m.vs + e] = v[e];
    }
    __syncthreads();
    if ((int)threadIdx.x < cpg) {
      float t = 0.f;
      for (int l = 0; l < m.rpp; ++l) t += lanes[l * cpg + threadIdx.x];
      ch[threadIdx.x] = t;
    }
    __syncthreads();
  };
  // (xhat, dn) of the thread's 2 VW elements of a row from the raw words
  auto terms = [&](const GnWords<VW>& wx, const GnWords<VW>& wd, float (&xh)[CH], float (&d)[CH]) {
#pragma unroll
    for (int v = 0; v < VW; ++v) {
      xh[2 * v] = (bf16lo(wx.w[v]) + sh[2 * v]) * rs;
      xh[2 * v + 1] = (bf16hi(wx.w[v]) + sh[2 * v + 1]) * rs;
      d[2 * v] = bf16lo(wd.w[v]);
      d[2 * v + 1] = bf16hi(wd.w[v]);
    }
    if (silu) {
#pragma unroll
      for (int e = 0; e < CH; ++e) d[e] *= silu_grad_f(fmaf(xh[e], ga[e], be[e]));
    }
  };
  GnWords<VW> cx[NC], cd[NC];
  float A[CH], Bs[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) A[e] = Bs[e] = 0.f;
  auto accumulate = [&](const GnWords<VW>& wx, const GnWords<VW>& wd) {
    float xh[CH], d[CH];
    terms(wx, wd, xh, d);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      A[e] += d[e] * xh[e];
      Bs[e] += d[e];
    }
  };
  if (RPT > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int r = m.rl + i * m.rpp;
#pragma unroll
      for (int v = 0; v < VW; ++v) cx[i].w[v] = cd[i].w[v] = 0u;
      if (m.active && r < inner) {
        cx[i] = gn_ldw<VW>(x + base + (long)r * C);
        cd[i] = gn_ldw<VW>(dy + base + (long)r * C);
        accumulate(cx[i], cd[i]);
      }
    }
  } else if (m.active) {
    for (int r = m.rl; r < inner; r += m.rpp) accumulate(gn_ldw<VW>(x + base + (long)r * C), gn_ldw<VW>(dy + base + (long)r * C));
  }
  fold(A, chA);
  fold(Bs, chB);
  if ((int)threadIdx.x < cpg) {
    dgamma_part[(long)b * C + g * cpg + threadIdx.x] = chA[threadIdx.x];
    dbeta_part[(long)b * C + g * cpg + threadIdx.x] = chB[threadIdx.x];
  }
  if (threadIdx.x == 0) {
    float s1 = 0.f, s2 = 0.f;  // sum dn gamma, sum dn gamma xhat
    for (int c = 0; c < cpg; ++c) {
      s1 += chB[c] * gamma[g * cpg + c];
      s2 += chA[c] * gamma[g * cpg + c];
    }
    const float inv_n = 1.f / ((float)cpg * (float)inner);
    sums[0] = s1 * inv_n;
    sums[1] = s2 * inv_n;
  }
  __syncthreads();
  const float m1 = sums[0], m2 = sums[1];
  float D[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) D[e] = 0.f;
  auto emit = [&](int r, const GnWords<VW>& wx, const GnWords<VW>& wd) {
    float xh[CH], d[CH];
    terms(wx, wd, xh, d);
    GnWords<VW> out;
#pragma unroll
    for (int v = 0; v < VW; ++v) {
      const float o0 = rs * (d[2 * v] * ga[2 * v] - m1 - xh[2 * v] * m2);
      const float o1 = rs * (d[2 * v + 1] * ga[2 * v + 1] - m1 - xh[2 * v + 1] * m2);
      out.w[v] = pack_bf16x2(o0, o1);
      D[2 * v] += o0;
      D[2 * v + 1] += o1;
    }
    gn_stw<VW>(dx + base + (long)r * C, out);
  };
  if (RPT > 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int r = m.rl + i * m.rpp;
      if (m.active && r < inner) emit(r, cx[i], cd[i]);
    }
  } else if (m.active) {
    for (int r = m.rl; r < inner; r += m.rpp) emit(r, gn_ldw<VW>(x + base + (long)r * C), gn_ldw<VW>(dy + base + (long)r * C));
  }
  if (dadd != nullptr) {
    fold(D, chA);
    if ((int)threadIdx.x < cpg) dadd[(long)b * C + g * cpg + threadIdx.x] = chA[threadIdx.x];
  }
}

// ---- slice form (few samples: B G too small to fill the chip, e.g. 256^2 x 1) --------------------------------------------------------
// LDS: lanes [rpp][C] + chan [C] + grp [2 G] floats (rpp * C <= 2048 + C: at most 4 C floats)
template <int KC>
__global__ __launch_bounds__(256) void gn_nhwc_stats_kernel(const bf16_t* __restrict__ x, const float* __restrict__ add,
                                                            float* __restrict__ part, int C, int G, int inner, int S) {
  extern __shared__ float gsm[];
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S;
  const GnNhwcMap m = gn_nhwc_map(C);
  float* lanes = gsm;
  float* chan = gsm + m.rpp * C;
  float* grp = chan + C;
  const int cpg = C / G;
  int r0, r1;
  gn_nhwc_rows(inner, S, sl, r0, r1);
  const bf16_t* xb = x + (long)b * inner * C;
  float ad[KC][8], acc[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ad[k][e] = (add != nullptr && k < m.nslot) ? add[(long)b * C + m.slot[k] * 8 + e] : 0.f;
      acc[k][e] = 0.f;
    }
  GN_NHWC_ROW_LOOP(r) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k == 0 || k < m.nslot) {
        float v[8];
        ld_act8<false>(xb, (long)r * C + m.slot[k] * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] += v[e] + ad[k][e];
      }
  }
  gn_nhwc_fold<KC>(m, acc, lanes, chan, C);
  const float cnt = (float)cpg * (float)(r1 - r0);
  if ((int)threadIdx.x < G) {
    float s = 0.f;
    for (int c = threadIdx.x * cpg; c < (int)(threadIdx.x + 1) * cpg; ++c) s += chan[c];
    grp[threadIdx.x] = cnt > 0.f ? s / cnt : 0.f;
  }
  __syncthreads();
  float mu[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mu[k][e] = k < m.nslot ? ad[k][e] - grp[(m.slot[k] * 8 + e) / cpg] : 0.f;  // v + add - mean
      acc[k][e] = 0.f;
    }
  GN_NHWC_ROW_LOOP(r) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k == 0 || k < m.nslot) {
        float v[8];
        ld_act8<false>(xb, (long)r * C + m.slot[k] * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[e] + mu[k][e];
          acc[k][e] += d * d;
        }
      }
  }
  gn_nhwc_fold<KC>(m, acc, lanes, chan, C);
  if ((int)threadIdx.x < G) {
    float q = 0.f;
    for (int c = threadIdx.x * cpg; c < (int)(threadIdx.x + 1) * cpg; ++c) q += chan[c];
    float* o = part + (((long)b * S + sl) * G + threadIdx.x) * 2;
    o[0] = grp[threadIdx.x];
    o[1] = q;
  }
}

// (mean, rstd) of every group of sample b from the S slice pairs, by threads 0 .. G - 1, into grp[0 .. G) / grp[G .. 2 G)
__device__ __forceinline__ void gn_nhwc_merge(const float* __restrict__ part, int b, int S, int G, int cpg, int inner, float eps,
                                              float* grp) {
  if ((int)threadIdx.x < G) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    // (no branch in the body and unrolled: the S pair loads of a thread are independent and issue ahead of the serial merge)
#pragma unroll 8
    for (int sl = 0; sl < S; ++sl) {
      int r0, r1;
      gn_nhwc_rows(inner, S, sl, r0, r1);
      const float nb = (float)cpg * (float)(r1 - r0);
      const float* o = part + (((long)b * S + sl) * G + threadIdx.x) * 2;
      const float o0 = o[0], o1 = o[1];
      const bool some = nb > 0.f;  // (an empty slice wrote (0, 0))
      const float nt = n + nb, d = o0 - mean;
      const float w = some ? nb / nt : 0.f;
      mean += d * w;
      m2 += some ? o1 + d * d * (n * w) : 0.f;
      n = nt;
    }
    grp[threadIdx.x] = mean;
    grp[G + threadIdx.x] = rsqrtf(m2 / n + eps);
  }
  __syncthreads();
}

// one workgroup per sample merges the slice pairs ONCE (the apply kernels read the result: merging inside every apply workgroup was
// S^2 G loads per sample — 268 MB of L2 reads per call at 256^2 x 1)
__global__ void gn_nhwc_merge_kernel(const float* __restrict__ part, float* __restrict__ mean_out, float* __restrict__ rstd_out, int G,
                                     int cpg, int inner, float eps, int S) {
  __shared__ float grp[2 * 64];
  const int b = blockIdx.x;
  gn_nhwc_merge(part, b, S, G, cpg, inner, eps, grp);
  if ((int)threadIdx.x < G) {
    mean_out[b * G + threadIdx.x] = grp[threadIdx.x];
    rstd_out[b * G + threadIdx.x] = grp[G + threadIdx.x];
  }
}

template <int KC>
__global__ __launch_bounds__(256) void gn_nhwc_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ add,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            bf16_t* __restrict__ y, const float* __restrict__ mean_in,
                                                            const float* __restrict__ rstd_in, int C, int G, int inner, int silu,
                                                            int affine_bs, int S) {
  __shared__ float grp[2 * 64];
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S;
  const GnNhwcMap m = gn_nhwc_map(C);
  const int cpg = C / G;
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  if ((int)threadIdx.x < G) {
    grp[threadIdx.x] = mean_in[b * G + threadIdx.x];
    grp[G + threadIdx.x] = rstd_in[b * G + threadIdx.x];
  }
  __syncthreads();
  float a[KC][8], bb[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a[k][e] = bb[k][e] = 0.f;
      if (k < m.nslot) {
        const int c = m.slot[k] * 8 + e, g = c / cpg;
        const float ad = add != nullptr ? add[(long)b * C + c] : 0.f;
        a[k][e] = grp[G + g] * gamma[c];
        bb[k][e] = beta[c] + (ad - grp[g]) * a[k][e];
      }
    }
  int r0, r1;
  gn_nhwc_rows(inner, S, sl, r0, r1);
  const bf16_t* xb = x + (long)b * inner * C;
  bf16_t* yb = y + (long)b * inner * C;
  GN_NHWC_ROW_LOOP(r) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k == 0 || k < m.nslot) {
        float v[8];
        const long off = (long)r * C + m.slot[k] * 8;
        ld_act8<false>(xb, off, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float o = fmaf(v[e], a[k][e], bb[k][e]);
          v[e] = silu ? silu_f(o) : o;
        }
        st_bf16x8(yb, off, v);
      }
  }
}

// backward, statistics: per slice and channel  A_c = sum dn * xhat,  B_c = sum dn  (dn = dy [* SiLU'(xhat gamma + beta)])
// part: [B][S][2][C]
template <int KC>
__global__ __launch_bounds__(256) void gn_nhwc_bwd_stats_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                const float* __restrict__ add, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ part, int C, int G,
                                                                int inner, int silu, int affine_bs, int S) {
  extern __shared__ float gsm[];
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S;
  const GnNhwcMap m = gn_nhwc_map(C);
  float* lanes = gsm;
  float* chan = gsm + m.rpp * C;
  const int cpg = C / G;
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  float sh[KC][8], rs[KC][8], ga[KC][8], be[KC][8], accA[KC][8], accB[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sh[k][e] = rs[k][e] = ga[k][e] = be[k][e] = accA[k][e] = accB[k][e] = 0.f;
      if (k < m.nslot) {
        const int c = m.slot[k] * 8 + e, g = c / cpg;
        rs[k][e] = rstd[b * G + g];
        sh[k][e] = (add != nullptr ? add[(long)b * C + c] : 0.f) - mean[b * G + g];  // xhat = (x + sh) * rs
        ga[k][e] = gamma[c];
        be[k][e] = beta[c];
      }
    }
  int r0, r1;
  gn_nhwc_rows(inner, S, sl, r0, r1);
  const bf16_t* xb = x + (long)b * inner * C;
  const bf16_t* dyb = dy + (long)b * inner * C;
  GN_NHWC_ROW_LOOP(r) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k == 0 || k < m.nslot) {
        float v[8], d[8];
        const long off = (long)r * C + m.slot[k] * 8;
        ld_act8<false>(xb, off, v);
        ld_act8<false>(dyb, off, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = (v[e] + sh[k][e]) * rs[k][e];
          float dn = d[e];
          if (silu) dn *= silu_grad_f(fmaf(xh, ga[k][e], be[k][e]));
          accA[k][e] += dn * xh;
          accB[k][e] += dn;
        }
      }
  }
  float* o = part + ((long)b * S + sl) * 2 * C;
  gn_nhwc_fold<KC>(m, accA, lanes, chan, C);
  for (int c = threadIdx.x; c < C; c += 256) o[c] = chan[c];
  gn_nhwc_fold<KC>(m, accB, lanes, chan, C);
  for (int c = threadIdx.x; c < C; c += 256) o[C + c] = chan[c];
}

// backward, apply: merges the slices per channel (slice order), writes the per-sample dgamma / dbeta partial rows (slice 0's
// workgroup), dx = rstd (dn gamma - s1 / n - xhat s2 / n), and per slice and channel sum(dx) for the time-embedding gradient
// LDS: lanes [rpp][C] + chA [C] + chB [C] + grp [2 G]
template <int KC>
__global__ __launch_bounds__(256) void gn_nhwc_bwd_apply_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                const float* __restrict__ add, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ part,
                                                                bf16_t* __restrict__ dx, const float* __restrict__ dgamma_part,
                                                                const float* __restrict__ dbeta_part, float* __restrict__ dadd_part, int C,
                                                                int G, int inner, int silu, int affine_bs, int S) {
  extern __shared__ float gsm[];
  const int b = blockIdx.x / S, sl = blockIdx.x - b * S;
  const GnNhwcMap m = gn_nhwc_map(C);
  float* lanes = gsm;
  float* chA = gsm + m.rpp * C;
  float* chB = chA + C;
  float* grp = chB + C;
  const int cpg = C / G;
  gamma += (long)b * affine_bs;
  beta += (long)b * affine_bs;
  (void)part;
  for (int c = threadIdx.x; c < C; c += 256) {  // the per-sample sums gn_nhwc_bwd_merge_kernel left in dgamma_part / dbeta_part
    chA[c] = dgamma_part[(long)b * C + c];
    chB[c] = dbeta_part[(long)b * C + c];
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    float s1 = 0.f, s2 = 0.f;  // sum dn gamma, sum dn gamma xhat
    for (int c = threadIdx.x * cpg; c < (int)(threadIdx.x + 1) * cpg; ++c) {
      s1 += chB[c] * gamma[c];
      s2 += chA[c] * gamma[c];
    }
    const float inv_n = 1.f / ((float)cpg * (float)inner);
    grp[threadIdx.x] = s1 * inv_n;
    grp[G + threadIdx.x] = s2 * inv_n;
  }
  __syncthreads();
  float sh[KC][8], rs[KC][8], ga[KC][8], be[KC][8], m1[KC][8], m2[KC][8], accD[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sh[k][e] = rs[k][e] = ga[k][e] = be[k][e] = m1[k][e] = m2[k][e] = accD[k][e] = 0.f;
      if (k < m.nslot) {
        const int c = m.slot[k] * 8 + e, g = c / cpg;
        rs[k][e] = rstd[b * G + g];
        sh[k][e] = (add != nullptr ? add[(long)b * C + c] : 0.f) - mean[b * G + g];
        ga[k][e] = gamma[c];
        be[k][e] = beta[c];
        m1[k][e] = grp[g];
        m2[k][e] = grp[G + g];
      }
    }
  int r0, r1;
  gn_nhwc_rows(inner, S, sl, r0, r1);
  const bf16_t* xb = x + (long)b * inner * C;
  const bf16_t* dyb = dy + (long)b * inner * C;
  bf16_t* dxb = dx + (long)b * inner * C;
  GN_NHWC_ROW_LOOP(r) {
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (k == 0 || k < m.nslot) {
        float v[8], d[8];
        const long off = (long)r * C + m.slot[k] * 8;
        ld_act8<false>(xb, off, v);
        ld_act8<false>(dyb, off, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = (v[e] + sh[k][e]) * rs[k][e];
          float dn = d[e];
          if (silu) dn *= silu_grad_f(fmaf(xh, ga[k][e], be[k][e]));
          const float o = rs[k][e] * (dn * ga[k][e] - m1[k][e] - xh * m2[k][e]);
          v[e] = o;
          accD[k][e] += o;
        }
        st_bf16x8(dxb, off, v);
      }
  }
  if (dadd_part != nullptr) {
    gn_nhwc_fold<KC>(m, accD, lanes, chA, C);  // (chA / chB are no longer needed: every thread holds its coefficients in registers)
    float* o = dadd_part + ((long)b * S + sl) * C;
    for (int c = threadIdx.x; c < C; c += 256) o[c] = chA[c];
  }
}

#undef GN_NHWC_ROW_LOOP

// dgamma_part[b][c] / dbeta_part[b][c] = the slice sums of A_c / B_c added in slice order, once per sample (S C loads per sample)
__global__ void gn_nhwc_bwd_merge_kernel(const float* __restrict__ part, float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                         int C, int S) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float sa = 0.f, sb = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < S; ++sl) {  // (same order of additions; unrolled so that the loads run ahead of them)
    const float* o = part + ((long)b * S + sl) * 2 * C;
    sa += o[c];
    sb += o[C + c];
  }
  dgamma_part[(long)b * C + c] = sa;
  dbeta_part[(long)b * C + c] = sb;
}

// dadd[b][c] = sum over the slices of sum(dx), slice order
__global__ void gn_nhwc_dadd_kernel(const float* __restrict__ part, float* __restrict__ dadd, int C, int S) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
#pragma unroll 8
  for (int sl = 0; sl < S; ++sl) s += part[((long)b * S + sl) * C + c];
  dadd[(long)b * C + c] = s;
}

}  // namespace

// f(std::bool_constant<flag>): a kernel's template argument chosen at run time, written once per entry point
template <class F>
static inline void gn_dispatch(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// ---- GroupNorm on NCHW: entry points ------------------------------------------------------------------------------------------
extern "C" int cfhip_groupnorm_fwd(const void* x, int x_is_f32, const float* add, const float* gamma, const float* beta, void* y,
                                   float* mean, float* rstd, int B, int C, int G, int inner, float eps, int silu,
                                   int affine_batch_stride, int splits, float* workspace, void* stream) {
  CFHIP_REQUIRE(affine_batch_stride == 0 || affine_batch_stride == C, "groupnorm_fwd: affine batch stride must be 0 or C");
  CFHIP_REQUIRE(x && gamma && beta && y && mean && rstd && B > 0 && C > 0 && G > 0 && inner > 0, "groupnorm_fwd: bad arguments");
  CFHIP_REQUIRE(C % G == 0, "groupnorm_fwd: %d channels do not split into %d groups", C, G);
  const bool vec = inner % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
  if (splits > 1) {
    CFHIP_REQUIRE(vec, "groupnorm_fwd: the split form needs inner %% 8 == 0 and 16-byte aligned x / y (pass splits = 1)");
    CFHIP_REQUIRE(splits <= 64 && splits <= inner / 8, "groupnorm_fwd: split form: %d slices for inner = %d", splits, inner);
    CFHIP_REQUIRE(workspace, "groupnorm_fwd: the split form needs a workspace");
  }
  hipStream_t s = (hipStream_t)stream;
  gn_dispatch(x_is_f32 != 0, [&](auto f32) {
    constexpr bool F32 = decltype(f32)::value;
    if (splits > 1) {
      const dim3 grid(B * G, splits);
      hipLaunchKernelGGL((gn_split_stats_kernel<F32>), grid, dim3(256), 0, s, x, add, workspace, C, G, inner, splits);
      hipLaunchKernelGGL((gn_split_apply_kernel<F32>), grid, dim3(256), 0, s, x, add, gamma, beta, workspace, (bf16_t*)y, mean, rstd,
                         C, G, inner, eps, silu, affine_batch_stride, splits);
    } else {
      hipLaunchKernelGGL(vec ? gn_fwd_vec_kernel<F32> : gn_fwd_kernel<F32>, dim3(B * G), dim3(256), 0, s, x, add, gamma, beta,
                         (bf16_t*)y, mean, rstd, C, G, inner, eps, silu, affine_batch_stride);
    }
  });
  CFHIP_CHECK_LAUNCH("groupnorm_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_groupnorm_bwd(const void* dy, const void* x, int x_is_f32, const float* add, const float* gamma, const float* beta,
                                   const float* mean, const float* rstd, void* dx, float* dgamma_part, float* dbeta_part, float* dadd,
                                   int B, int C, int G, int inner, int silu, int affine_batch_stride, int splits, float* workspace,
                                   void* stream) {
  CFHIP_REQUIRE(affine_batch_stride == 0 || affine_batch_stride == C, "groupnorm_bwd: affine batch stride must be 0 or C");
  CFHIP_REQUIRE(dy && x && gamma && beta && mean && rstd && dx && dgamma_part && dbeta_part, "groupnorm_bwd: null pointer");
  CFHIP_REQUIRE(B > 0 && C > 0 && G > 0 && inner > 0 && C % G == 0, "groupnorm_bwd: bad geometry");
  CFHIP_REQUIRE(dadd == nullptr || add != nullptr, "groupnorm_bwd: dadd without add");
  const bool vec = inner % 8 == 0 && C / G <= GN_MAX_CG && ((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0 &&
                   ((uintptr_t)dx & 15) == 0;
  if (splits > 1) {
    CFHIP_REQUIRE(vec, "groupnorm_bwd: the split form needs inner %% 8 == 0, <= %d channels per group and 16-byte aligned x / dy / dx (pass splits = 1)",
                  GN_MAX_CG);
    CFHIP_REQUIRE(splits <= 64 && splits <= inner / 8, "groupnorm_bwd: split form: %d slices for inner = %d", splits, inner);
    CFHIP_REQUIRE(workspace, "groupnorm_bwd: the split form needs a workspace");
  }
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* dyp = (const bf16_t*)dy;
  gn_dispatch(x_is_f32 != 0, [&](auto f32) {
    constexpr bool F32 = decltype(f32)::value;
    if (splits > 1) {
      const dim3 grid(B * G, splits);
      const int want = dadd != nullptr;
      hipLaunchKernelGGL((gn_split_bwd_stats_kernel<F32>), grid, dim3(256), 0, s, dyp, x, add, gamma, beta, mean, rstd, workspace, C, G,
                         inner, silu, affine_batch_stride, splits);
      hipLaunchKernelGGL((gn_split_bwd_apply_kernel<F32>), grid, dim3(256), 0, s, dyp, x, add, gamma, beta, mean, rstd, workspace,
                         (bf16_t*)dx, dgamma_part, dbeta_part, want, C, G, inner, silu, affine_batch_stride, splits);
      if (want) hipLaunchKernelGGL(gn_split_dadd_kernel, dim3(B * G), dim3(128), 0, s, workspace, dadd, C, G, splits);
    } else {
      hipLaunchKernelGGL(vec ? gn_bwd_vec_kernel<F32> : gn_bwd_kernel<F32>, dim3(B * G), dim3(256), 0, s, dyp, x, add, gamma, beta,
                         mean, rstd, (bf16_t*)dx, dgamma_part, dbeta_part, dadd, C, G, inner, silu, affine_batch_stride);
    }
  });
  CFHIP_CHECK_LAUNCH("groupnorm_bwd");
  return CFHIP_OK;
}

// ---- GroupNorm on NHWC rows: entry points ---------------------------------------------------------------------------------------
static int gn_nhwc_check(const char* who, int B, int C, int G, int inner, int splits) {
  CFHIP_REQUIRE(B > 0 && C > 0 && G > 0 && inner > 0, "%s: empty problem (B=%d C=%d G=%d inner=%d)", who, B, C, G, inner);
  CFHIP_REQUIRE(C % 8 == 0 && C % G == 0 && G <= 64 && C <= 4096, "%s: C = %d must be a multiple of 8 and of G = %d (<= 64), at most 4096", who, C, G);
  if (splits == 0) {
    const int cpg = C / G;
    CFHIP_REQUIRE(cpg % 2 == 0 && cpg <= 256, "%s: the group form (splits = 0) needs an even number of channels per group, at most 256 (got %d)", who, cpg);
    return CFHIP_OK;
  }
  CFHIP_REQUIRE(splits >= 1 && splits <= inner && splits <= 4096, "%s: splits = %d outside 1 .. min(inner, 4096)", who, splits);
  return CFHIP_OK;
}
static inline int gn_nhwc_rpp(int C) { return (C >> 3) >= 256 ? 1 : 256 / (C >> 3); }
// dwords a thread of the group form reads with one access: the largest of 4 / 2 / 1 that divides the chunk's cpg / 2 dwords
// (the chunk then starts on a 4 VW-byte boundary in every row: C * 2 is a multiple of 16)
static inline int gn_group_vw(int cpg) { const int d = cpg >> 1; return d % 4 == 0 ? 4 : d % 2 == 0 ? 2 : 1; }

extern "C" size_t cfhip_groupnorm_nhwc_workspace(int B, int C, int G, int splits, int backward, int with_add) {
  if (B <= 0 || C <= 0 || G <= 0 || splits <= 0) return 0;
  if (!backward) return (size_t)B * splits * G * 2 * sizeof(float);
  return ((size_t)B * splits * 2 * C + (with_add ? (size_t)B * splits * C : 0)) * sizeof(float);
}

extern "C" int cfhip_groupnorm_nhwc_fwd(const void* x, const float* add, const float* gamma, const float* beta, void* y, float* mean,
                                        float* rstd, int B, int C, int G, int inner, float eps, int silu, int affine_batch_stride,
                                        int splits, float* workspace, void* stream) {
  CFHIP_REQUIRE(x && gamma && beta && y && mean && rstd && (workspace || splits == 0), "groupnorm_nhwc_fwd: null argument");
  const int rc = gn_nhwc_check("groupnorm_nhwc_fwd", B, C, G, inner, splits);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(affine_batch_stride == 0 || affine_batch_stride == C, "groupnorm_nhwc_fwd: affine_batch_stride must be 0 or C");
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* xp = (const bf16_t*)x;
  if (splits == 0) {  // group form: one workgroup per (sample, group), one launch
    // dwords per thread (rows x vector width): kept in registers when they fit
    const int vw = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 ? gn_group_vw(C / G) : 1;  // (rows of an odd view: dword accesses)
    const int rpp = 256 / ((C / G / 2) / vw);
    const int rpt = ((inner + rpp - 1) / rpp) * vw;
#define CFHIP_GN_GROUP_FWD_V(RPT, VW)                                                                                                  \
  hipLaunchKernelGGL((gn_nhwc_group_fwd_kernel<RPT, VW>), dim3(B * G), dim3(256), 0, s, xp, add, gamma, beta, (bf16_t*)y, mean, rstd, C, G, \
                     inner, eps, silu, affine_batch_stride)
#define CFHIP_GN_GROUP_FWD(RPT)                  \
  do {                                           \
    if (vw == 4) CFHIP_GN_GROUP_FWD_V(RPT, 4);   \
    else if (vw == 2) CFHIP_GN_GROUP_FWD_V(RPT, 2); \
    else CFHIP_GN_GROUP_FWD_V(RPT, 1);           \
  } while (0)
    if (rpt <= 48) CFHIP_GN_GROUP_FWD(48);  // (a 24-row instantiation came out of hipcc with 254 VGPRs and 132 B of scratch: not built)
    else if (rpt <= 96) CFHIP_GN_GROUP_FWD(96);
    else if (rpt <= 176) CFHIP_GN_GROUP_FWD(176);
    else CFHIP_GN_GROUP_FWD(0);
#undef CFHIP_GN_GROUP_FWD
#undef CFHIP_GN_GROUP_FWD_V
    CFHIP_CHECK_LAUNCH("groupnorm_nhwc_fwd");
    return CFHIP_OK;
  }
  const size_t lds = ((size_t)gn_nhwc_rpp(C) * C + C + 2 * 64) * sizeof(float);
  const int cpg = C / G;
  gn_dispatch((C >> 3) > 256, [&](auto two) {  // 8-channel slots per thread
    constexpr int KC = decltype(two)::value ? 2 : 1;
    hipLaunchKernelGGL((gn_nhwc_stats_kernel<KC>), dim3(B * splits), dim3(256), lds, s, xp, add, workspace, C, G, inner, splits);
    hipLaunchKernelGGL(gn_nhwc_merge_kernel, dim3(B), dim3(64), 0, s, workspace, mean, rstd, G, cpg, inner, eps, splits);
    hipLaunchKernelGGL((gn_nhwc_apply_kernel<KC>), dim3(B * splits), dim3(256), 0, s, xp, add, gamma, beta, (bf16_t*)y, mean, rstd, C, G, inner,
                       silu, affine_batch_stride, splits);
  });
  CFHIP_CHECK_LAUNCH("groupnorm_nhwc_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_groupnorm_nhwc_bwd(const void* dy, const void* x, const float* add, const float* gamma, const float* beta,
                                        const float* mean, const float* rstd, void* dx, float* dgamma_part, float* dbeta_part, float* dadd,
                                        int B, int C, int G, int inner, int silu, int affine_batch_stride, int splits, float* workspace,
                                        void* stream) {
  CFHIP_REQUIRE(dy && x && gamma && beta && mean && rstd && dx && dgamma_part && dbeta_part && (workspace || splits == 0), "groupnorm_nhwc_bwd: null argument");
  const int rc = gn_nhwc_check("groupnorm_nhwc_bwd", B, C, G, inner, splits);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(affine_batch_stride == 0 || affine_batch_stride == C, "groupnorm_nhwc_bwd: affine_batch_stride must be 0 or C");
  CFHIP_REQUIRE((dadd != nullptr) == (add != nullptr), "groupnorm_nhwc_bwd: dadd goes with add");
  hipStream_t s = (hipStream_t)stream;
  if (splits == 0) {  // group form
    const int vw = (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0 ? gn_group_vw(C / G) : 1;
    const int rpp = 256 / ((C / G / 2) / vw);
    const int rpt = ((inner + rpp - 1) / rpp) * vw;
#define CFHIP_GN_GROUP_BWD_V(RPT, VW)                                                                                                   \
  hipLaunchKernelGGL((gn_nhwc_group_bwd_kernel<RPT, VW>), dim3(B * G), dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)x, add, gamma, beta, \
                     mean, rstd, (bf16_t*)dx, dgamma_part, dbeta_part, dadd, C, G, inner, silu, affine_batch_stride)
#define CFHIP_GN_GROUP_BWD(RPT)                  \
  do {                                           \
    if (vw == 4) CFHIP_GN_GROUP_BWD_V(RPT, 4);   \
    else if (vw == 2) CFHIP_GN_GROUP_BWD_V(RPT, 2); \
    else CFHIP_GN_GROUP_BWD_V(RPT, 1);           \
  } while (0)
    if (rpt <= 48) CFHIP_GN_GROUP_BWD(48);
    else if (rpt <= 88) CFHIP_GN_GROUP_BWD(88);
    else CFHIP_GN_GROUP_BWD(0);
#undef CFHIP_GN_GROUP_BWD
#undef CFHIP_GN_GROUP_BWD_V
    CFHIP_CHECK_LAUNCH("groupnorm_nhwc_bwd");
    return CFHIP_OK;
  }
  const size_t lds_a = ((size_t)gn_nhwc_rpp(C) * C + C) * sizeof(float);
  const size_t lds_b = ((size_t)gn_nhwc_rpp(C) * C + 2 * C + 2 * 64) * sizeof(float);
  float* part = workspace;
  float* dpart = dadd != nullptr ? workspace + (size_t)B * splits * 2 * C : nullptr;
  const bf16_t* dyp = (const bf16_t*)dy;
  const bf16_t* xp = (const bf16_t*)x;
  gn_dispatch((C >> 3) > 256, [&](auto two) {
    constexpr int KC = decltype(two)::value ? 2 : 1;
    hipLaunchKernelGGL((gn_nhwc_bwd_stats_kernel<KC>), dim3(B * splits), dim3(256), lds_a, s, dyp, xp, add, gamma, beta, mean, rstd, part, C, G,
                       inner, silu, affine_batch_stride, splits);
    hipLaunchKernelGGL(gn_nhwc_bwd_merge_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, part, dgamma_part, dbeta_part, C, splits);
    hipLaunchKernelGGL((gn_nhwc_bwd_apply_kernel<KC>), dim3(B * splits), dim3(256), lds_b, s, dyp, xp, add, gamma, beta, mean, rstd, part,
                       (bf16_t*)dx, dgamma_part, dbeta_part, dpart, C, G, inner, silu, affine_batch_stride, splits);
  });
  if (dadd != nullptr)
    hipLaunchKernelGGL(gn_nhwc_dadd_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, dpart, dadd, C, splits);
  CFHIP_CHECK_LAUNCH("groupnorm_nhwc_bwd");
  return CFHIP_OK;
}
