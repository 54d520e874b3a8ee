// Token merging (tomesd) of the SpatialTransformer hooks: bipartite_soft_matching_random2d of the reference
// (modules/core/mixed_stacks/api.py:473-589) without the [B, N_src, N_dst] cosine matrix it forms only to take a row maximum, and
// without its sort / three gathers / scatter_reduce / three scatter_ calls.  Four entries:
//
//   match        rinv_t = 1 / |x_t| (f32 sum of squares; 0 for a zero row), then per src row i
//                  node_max_i, node_idx_i = max / lowest arg-max over j of  (dot(src_i, dst_j) * rinv_src_i) * rinv_dst_j
//                dot on v_mfma_f32_16x16x32_bf16 over the RAW bf16 rows (products exact in f32, f32 accumulation); the two inverse
//                norms are applied in f32 afterwards, never rounded into a bf16 operand.
//   select       the r largest node_max of a sample (ties: lowest src position) by a four-pass radix select on the order-preserving
//                integer image of the float and prefix-sum compactions: one workgroup per sample, everything streamed from global
//                memory (N_src reaches 49 152), integer atomics for COUNTS only, so two runs are bit-identical.
//   merge        [unmerged src rows, ascending token | dst rows, ascending token]; dst = (dst + sum members) / (1 + count), the members
//                added in ascending token order in f32, one rounding.
//   unmerge_add  out[t] = residual[t] + y[row_of_token[t]]: one f32 add, one rounding.
//
// Match layout: a workgroup of four waves takes 64 src rows (16 per wave), each wave holds ITS rows' MFMA B-operand fragments
// for the whole channel extent in registers (KS k-steps of 32 channels, 4 VGPRs each) and the dst rows stream through LDS DT rows
// at a time, shared by the four waves.  A lane's accumulator holds four dst rows of one src column, scanned in ascending j with a
// strict >; the four lanes of a column meet through two shuffles, the lower j winning a tie: what one ascending scan gives.
#include "common.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TS_THREADS = 1024;

__global__ __launch_bounds__(256) void tome_rinv_kernel(const bf16_t* __restrict__ x, float* __restrict__ rinv, long rows, int C) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* p = x + row * C;
  float sq = 0.f;
  for (int c8 = lane; c8 < C / 8; c8 += 64) {
    float v[8];
    ld_act8<false>(p, c8 * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) sq = fmaf(v[e], v[e], sq);
  }
  sq = wave_sum(sq);
  if (lane == 0) rinv[row] = sq > 0.f ? 1.0f / sqrtf(sq) : 0.f;
}

template <int KS, int DT>
__global__ __launch_bounds__(TM_THREADS) void tome_match_kernel(const bf16_t* __restrict__ x, const int* __restrict__ src_idx,
                                                                 const int* __restrict__ dst_idx, const float* __restrict__ rinv,
                                                                 float* __restrict__ node_max, int* __restrict__ node_idx, int N, int C,
                                                                 int n_src, int n_dst) {
  constexpr int STRIDE = KS * 64 + 16;  // bytes of a dst row in LDS: an odd number of 16-byte slots
  __shared__ __attribute__((aligned(16))) unsigned char tile[DT * STRIDE];
  __shared__ float tile_rinv[DT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4;
  const int b = blockIdx.y;
  const bf16_t* xb = x + (long)b * N * C;
  const float* rb = rinv + (long)b * N;
  const int chunks = C / 8;

  // this lane's src row (a row past the end repeats the last one; nothing is written for it)
  const int i = blockIdx.x * 64 + wave * 16 + (lane & 15);
  const int tok = min((unsigned)src_idx[min(i, n_src - 1)], (unsigned)(N - 1));
  bf16x8 sf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int ch = ks * 4 + q;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xb + (long)tok * C + (ch < chunks ? ch : 0) * 8);
    sf[ks] = ch < chunks ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};  // the C tail of the last k-step: zeros
  }
  const float rs = rb[tok];
  float best = -__builtin_inff();
  int best_j = 0;

  // 16-byte chunk e of the tile that starts at dst row j0: row e / (4 KS), chunk e % (4 KS); zeros past the last row / channel
  static_assert((DT * KS * 4) % TM_THREADS == 0 && DT <= TM_THREADS, "a tile is a whole number of chunks per thread");
  constexpr int PF = DT * KS * 4 / TM_THREADS;
  auto fetch = [&](u32x4 (&pf)[PF], float& pr, int j0) {
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int e = tid + t * TM_THREADS;
      const int rr = e / (KS * 4), ch = e % (KS * 4);
      const int j = j0 + rr;
      const bool live = j < n_dst && ch < chunks;
      // (no branch around the load: a dead chunk reads the tile's first row and is replaced by zeros; all PF loads in flight together)
      const int tk = min((unsigned)dst_idx[live ? j : j0], (unsigned)(N - 1));
      const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (long)tk * C + (live ? ch : 0) * 8);
      pf[t] = live ? v : u32x4{0u, 0u, 0u, 0u};
    }
    pr = 0.f;
    if (tid < DT && j0 + tid < n_dst) pr = rb[min((unsigned)dst_idx[j0 + tid], (unsigned)(N - 1))];
  };
  u32x4 pf[PF];
  float pr;
  fetch(pf, pr, 0);

  for (int j0 = 0; j0 < n_dst; j0 += DT) {
    __syncthreads();  // every wave has finished with the previous tile
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int e = tid + t * TM_THREADS;
      *reinterpret_cast<u32x4*>(&tile[(e / (KS * 4)) * STRIDE + (e % (KS * 4)) * 16]) = pf[t];
    }
    if (tid < DT) tile_rinv[tid] = pr;
    __syncthreads();
    if (j0 + DT < n_dst) fetch(pf, pr, j0 + DT);  // in flight while this tile is scored
#pragma unroll 1
    for (int st = 0; st < DT / 16; ++st) {
      if (j0 + st * 16 >= n_dst) break;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const unsigned char* rowp = &tile[(st * 16 + (lane & 15)) * STRIDE + q * 16];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks * 32 < C) {
          const bf16x8 df = *reinterpret_cast<const bf16x8*>(rowp + ks * 64);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, sf[ks], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {  // dst rows j ascending within the lane
        const int jl = st * 16 + q * 4 + reg;
        const float s = (acc[reg] * rs) * tile_rinv[jl];
        if (j0 + jl < n_dst && s > best) {
          best = s;
          best_j = j0 + jl;
        }
      }
    }
  }
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float os = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(best_j, off, 64);
    if (os > best || (os == best && oj < best_j)) {
      best = os;
      best_j = oj;
    }
  }
  if (lane < 16 && i < n_src) {
    node_max[(long)b * n_src + i] = best;
    node_idx[(long)b * n_src + i] = best_j;
  }
}

// ---- select ---------------------------------------------------------------------------------------------------------------

// larger float <-> larger unsigned (-0 < +0; NaNs land at the two ends, wherever: deterministically)
__device__ __forceinline__ unsigned tome_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A value another wave of THIS workgroup stored or counted in global memory, read after a __syncthreads(): a workgroup-scope atomic
// load.  One workgroup runs on one CU, so workgroup scope is all the phases of the select kernel need, and the fences inside
// __syncthreads() are all their ordering (an agent-scope fence or load goes past the L2: tens of microseconds over the kernel).
__device__ __forceinline__ int ld_wg(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// exclusive prefix sum of v over the workgroup (TS_THREADS threads, thread order); total = the sum
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  __syncthreads();  // wsum is free again
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < TS_THREADS / 64; ++w) {
    const int s = wsum[w];
    base += w < wave ? s : 0;
    tot += s;
  }
  total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(TS_THREADS) void tome_select_kernel(const float* __restrict__ node_max, const int* __restrict__ node_idx,
                                                                  const int* __restrict__ src_idx, const int* __restrict__ dst_idx,
                                                                  int* row_of_token, int* token_of_row, int* member_off, int* members,
                                                                  int* cursor, int N, int n_src, int n_dst, int r) {
  __shared__ __attribute__((aligned(16))) int hist[256];
  __shared__ int wsum[TS_THREADS / 64];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_rem;
  __shared__ __attribute__((aligned(16))) int keys[TS_THREADS];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const float* nm = node_max + b * n_src;
  const int* ni = node_idx + b * n_src;
  int* rot = row_of_token + b * N;
  int* tor = token_of_row + b * (N - r);
  int* moff = member_off + b * (n_dst + 1);
  int* mem = members + b * r;
  int* cur = cursor + b * n_dst;
  const int n_unm = n_src - r;

  // the key of the r-th largest value, eight bits per pass from the top; `rem` = how many of the keys equal to it are taken
  unsigned prefix = 0u;
  int rem = r;
  if (tid == 0) {
    sh_prefix = 0u;
    sh_rem = r;
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n_src; i += TS_THREADS) {
      const unsigned key = tome_key(nm[i]);
      if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid < 64) {  // the digit d with count(digits > d) < rem <= count(digits >= d): lane l owns digits 4 l .. 4 l + 3
      const int4 h = reinterpret_cast<const int4*>(hist)[tid];
      const int own = h.x + h.y + h.z + h.w;
      int suf = own;  // keys in this lane's digits and all higher ones
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(suf, off, 64);
        if (tid + off < 64) suf += t;
      }
      const int above = suf - own;
      if (above < rem && rem <= suf) {  // exactly one lane (rem <= the keys that carry the prefix)
        int rm = rem - above, d = 4 * tid + 3;
        if (rm > h.w) {
          rm -= h.w;
          d = 4 * tid + 2;
          if (rm > h.z) {
            rm -= h.z;
            d = 4 * tid + 1;
            if (rm > h.y) {
              rm -= h.y;
              d = 4 * tid;
            }
          }
        }
        sh_prefix = prefix | ((unsigned)d << shift);
        sh_rem = rm;
      }
    }
    __syncthreads();
    prefix = sh_prefix;
    rem = sh_rem;
  }
  const unsigned T = prefix;
  const int need_eq = rem;

  for (int j = tid; j <= n_dst; j += TS_THREADS) {
    moff[j] = 0;
    if (j < n_dst) cur[j] = 0;
  }
  __syncthreads();

  // src positions in ascending order (= ascending token order), TS_THREADS at a time: taken or not, and the rank among the rest
  int eq_base = 0, unm_base = 0;
  for (int c0 = 0; c0 < n_src; c0 += TS_THREADS) {
    const int i = c0 + tid;
    const bool live = i < n_src;
    const unsigned key = live ? tome_key(nm[i]) : 0u;
    const bool iseq = live && key == T;
    int tot;
    const int eqx = eq_base + block_excl_scan(iseq ? 1 : 0, wsum, tot);
    eq_base += tot;
    const bool sel = live && (key > T || (iseq && eqx < need_eq));
    const bool unm = live && !sel;
    const int ux = unm_base + block_excl_scan(unm ? 1 : 0, wsum, tot);
    unm_base += tot;
    if (live) {
      const int tok = min((unsigned)src_idx[i], (unsigned)(N - 1));
      if (unm) {
        if (ux < n_unm) {
          rot[tok] = ux;
          tor[ux] = tok;
        }
      } else {
        const int j = min((unsigned)ni[i], (unsigned)(n_dst - 1));
        rot[tok] = n_unm + j;
        atomicAdd(&moff[j + 1], 1);
      }
    }
  }
  for (int j = tid; j < n_dst; j += TS_THREADS) {
    const int tok = min((unsigned)dst_idx[j], (unsigned)(N - 1));
    rot[tok] = n_unm + j;
    tor[n_unm + j] = tok;
  }
  __syncthreads();

  // member_off[j] = members of the dst rows before j: the inclusive scan of [0, count_0, count_1, ..] in place
  int carry = 0;
  for (int c0 = 0; c0 <= n_dst; c0 += TS_THREADS) {
    const int j = c0 + tid;
    const int v = j <= n_dst ? ld_wg(&moff[j]) : 0;
    int tot;
    const int ex = block_excl_scan(v, wsum, tot);
    if (j <= n_dst) moff[j] = carry + ex + v;
    carry += tot;
  }
  __syncthreads();

  // member lists in ascending src position: a taken row's slot = the members its dst already has from earlier chunks
  // (cursor) + the taken rows of the same dst before it in this chunk
  for (int c0 = 0; c0 < n_src; c0 += TS_THREADS) {
    const int i = c0 + tid;
    int j = -1, tok = 0;
    if (i < n_src) {
      tok = min((unsigned)src_idx[i], (unsigned)(N - 1));
      const int row = ld_wg(&rot[tok]);
      if (row >= n_unm) j = row - n_unm;
    }
    __syncthreads();  // the previous chunk's keys have been read, its cursor updates have landed
    keys[tid] = j;
    __syncthreads();
    if (j >= 0) {
      int rank = 0;
#pragma unroll 8  // (independent LDS reads: eight in flight instead of one)
      for (int k4 = 0; k4 * 4 < tid; ++k4) {
        const int4 v = reinterpret_cast<const int4*>(keys)[k4];
        const int k = k4 * 4;
        rank += (v.x == j ? 1 : 0) + ((v.y == j && k + 1 < tid) ? 1 : 0) + ((v.z == j && k + 2 < tid) ? 1 : 0) +
                ((v.w == j && k + 3 < tid) ? 1 : 0);
      }
      const int slot = ld_wg(&moff[j]) + ld_wg(&cur[j]) + rank;
      if (slot < r) mem[slot] = tok;
    }
    __syncthreads();  // every cursor of this chunk has been read
    if (j >= 0) atomicAdd(&cur[j], 1);
  }
}

// ---- merge / unmerge ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, const int* __restrict__ token_of_row,
                                                          const int* __restrict__ member_off, const int* __restrict__ members,
                                                          bf16_t* __restrict__ out, int N, int C, int n_unm, int n_dst, int r) {
  const int lane = threadIdx.x & 63;
  const int rows = N - r;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const long b = blockIdx.y;
  if (row >= rows) return;
  const bf16_t* xb = x + b * N * C;
  bf16_t* o = out + (b * rows + row) * C;
  const int tok = min((unsigned)token_of_row[b * rows + row], (unsigned)(N - 1));
  const bf16_t* self = xb + (long)tok * C;
  if (row < n_unm) {
    for (int c8 = lane; c8 < C / 8; c8 += 64) reinterpret_cast<u32x4*>(o)[c8] = reinterpret_cast<const u32x4*>(self)[c8];
    return;
  }
  const int j = row - n_unm;
  const int m0 = max(member_off[b * (n_dst + 1) + j], 0), m1 = min(member_off[b * (n_dst + 1) + j + 1], r);
  const int* mem = members + b * r;
  const float count = (float)(1 + m1 - m0);
  for (int c8 = lane; c8 < C / 8; c8 += 64) {
    float acc[8];
    ld_act8<false>(self, c8 * 8, acc);
    for (int m = m0; m < m1; ++m) {  // ascending token order
      const int t = min((unsigned)mem[m], (unsigned)(N - 1));
      float v[8];
      ld_act8<false>(xb + (long)t * C, c8 * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] / count;
    st_bf16x8(o, c8 * 8, acc);
  }
}

template <bool RES, bool F32>
__global__ __launch_bounds__(256) void tome_unmerge_add_kernel(const bf16_t* __restrict__ y, const int* __restrict__ row_of_token,
                                                                const void* __restrict__ residual, void* __restrict__ out, int N, int C,
                                                                int rows) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const long b = blockIdx.y;
  if (t >= N) return;
  const int row = min((unsigned)row_of_token[b * N + t], (unsigned)(rows - 1));
  const bf16_t* yr = y + (b * rows + row) * C;
  const long at = (b * N + t) * C;
  for (int c8 = lane; c8 < C / 8; c8 += 64) {
    float v[8];
    ld_act8<false>(yr, c8 * 8, v);
    if (RES) {
      float res[8];
      ld_act8<F32>(residual, at + c8 * 8, res);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = res[e] + v[e];
    }
    if (F32) {
      float* o = reinterpret_cast<float*>(out) + at + c8 * 8;
      *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
      st_bf16x8(reinterpret_cast<bf16_t*>(out), at + c8 * 8, v);
    }
  }
}

bool tome_shape_ok(int64_t B, int N, int C, const char* who) {
  if (B < 1 || B > 65535 || N < 1 || N > CFHIP_TOME_MAX_TOKENS || C < 8 || C > CFHIP_TOME_MAX_CHANNELS || C % 8 != 0) {
    cfhip_set_error("%s: B = %lld, N = %d, C = %d outside 1 <= B <= 65535, 1 <= N <= %d, C %% 8 == 0, 8 <= C <= %d", who, (long long)B, N,
                    C, CFHIP_TOME_MAX_TOKENS, CFHIP_TOME_MAX_CHANNELS);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int cfhip_tome_match(const void* x, const int* src_idx, const int* dst_idx, float* rinv, float* node_max, int* node_idx,
                                int64_t B, int N, int C, int n_src, int n_dst, void* stream) {
  CFHIP_REQUIRE(x && src_idx && dst_idx && rinv && node_max && node_idx, "tome_match: null operand");
  if (!tome_shape_ok(B, N, C, "tome_match")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src + n_dst == N, "tome_match: n_src = %d, n_dst = %d do not split N = %d", n_src, n_dst, N);
  CFHIP_REQUIRE(((uintptr_t)x & 15) == 0 && (((uintptr_t)src_idx | (uintptr_t)dst_idx | (uintptr_t)rinv | (uintptr_t)node_max |
                                              (uintptr_t)node_idx) & 3) == 0,
                "tome_match: misaligned operand");
  const hipStream_t s = (hipStream_t)stream;
  const bf16_t* xp = reinterpret_cast<const bf16_t*>(x);
  const long rows = (long)B * N;
  hipLaunchKernelGGL(tome_rinv_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, xp, rinv, rows, C);
  CFHIP_CHECK_LAUNCH("tome_match (norms)");
  const dim3 grid((unsigned)((n_src + 63) / 64), (unsigned)B);
#define TOME_MATCH(KS, DT)                                                                                                        \
  hipLaunchKernelGGL((tome_match_kernel<KS, DT>), grid, dim3(TM_THREADS), 0, s, xp, src_idx, dst_idx, rinv, node_max, node_idx, N, C, \
                     n_src, n_dst)
  if (C <= 64) TOME_MATCH(2, 64);
  else if (C <= 320) TOME_MATCH(10, 64);
  else if (C <= 640) TOME_MATCH(20, 32);
  else TOME_MATCH(40, 16);
#undef TOME_MATCH
  CFHIP_CHECK_LAUNCH("tome_match");
  return CFHIP_OK;
}

extern "C" int cfhip_tome_select(const float* node_max, const int* node_idx, const int* src_idx, const int* dst_idx, int* row_of_token,
                                 int* token_of_row, int* member_off, int* members, int* cursor, int64_t B, int N, int n_src, int n_dst,
                                 int r, void* stream) {
  CFHIP_REQUIRE(node_max && node_idx && src_idx && dst_idx && row_of_token && token_of_row && member_off && members && cursor,
                "tome_select: null operand");
  if (!tome_shape_ok(B, N, 8, "tome_select")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src + n_dst == N, "tome_select: n_src = %d, n_dst = %d do not split N = %d", n_src, n_dst, N);
  CFHIP_REQUIRE(r >= 1 && r <= n_src, "tome_select: r = %d outside [1, n_src = %d]", r, n_src);
  hipLaunchKernelGGL(tome_select_kernel, dim3((unsigned)B), dim3(TS_THREADS), 0, (hipStream_t)stream, node_max, node_idx, src_idx, dst_idx,
                     row_of_token, token_of_row, member_off, members, cursor, N, n_src, n_dst, r);
  CFHIP_CHECK_LAUNCH("tome_select");
  return CFHIP_OK;
}

extern "C" int cfhip_tome_merge(const void* x, const int* token_of_row, const int* member_off, const int* members, void* out, int64_t B,
                                int N, int C, int n_src, int n_dst, int r, void* stream) {
  CFHIP_REQUIRE(x && token_of_row && member_off && members && out, "tome_merge: null operand");
  if (!tome_shape_ok(B, N, C, "tome_merge")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src + n_dst == N, "tome_merge: n_src = %d, n_dst = %d do not split N = %d", n_src, n_dst, N);
  CFHIP_REQUIRE(r >= 1 && r <= n_src, "tome_merge: r = %d outside [1, n_src = %d]", r, n_src);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "tome_merge: misaligned operand");
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)((N - r + 3) / 4), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const bf16_t*>(x), token_of_row, member_off, members, reinterpret_cast<bf16_t*>(out), N, C,
                     n_src - r, n_dst, r);
  CFHIP_CHECK_LAUNCH("tome_merge");
  return CFHIP_OK;
}

extern "C" int cfhip_tome_unmerge_add(const void* y, const int* row_of_token, const void* residual, void* out, int out_is_f32, int64_t B,
                                      int N, int C, int r, void* stream) {
  CFHIP_REQUIRE(y && row_of_token && out, "tome_unmerge_add: null operand");
  if (!tome_shape_ok(B, N, C, "tome_unmerge_add")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(r >= 1 && r < N, "tome_unmerge_add: r = %d outside [1, N = %d)", r, N);
  CFHIP_REQUIRE((((uintptr_t)y | (uintptr_t)residual | (uintptr_t)out) & 15) == 0, "tome_unmerge_add: misaligned operand");
  const dim3 grid((unsigned)((N + 3) / 4), (unsigned)B);
  const hipStream_t s = (hipStream_t)stream;
  const bf16_t* yp = reinterpret_cast<const bf16_t*>(y);
#define TOME_UNMERGE(RES, F32) \
  hipLaunchKernelGGL((tome_unmerge_add_kernel<RES, F32>), grid, dim3(256), 0, s, yp, row_of_token, residual, out, N, C, N - r)
  if (residual != nullptr) {
    if (out_is_f32) TOME_UNMERGE(true, true);
    else TOME_UNMERGE(true, false);
  } else {
    if (out_is_f32) TOME_UNMERGE(false, true);
    else TOME_UNMERGE(false, false);
  }
#undef TOME_UNMERGE
  CFHIP_CHECK_LAUNCH("tome_unmerge_add");
  return CFHIP_OK;
}
