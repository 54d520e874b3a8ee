// NBM (neural basis model) for gfx950: the per-basis MLPs and the featurizer of reference modules/ml/nbm.py.
//
// For every row m = (b, d) (sample b, feature tuple d; M = B D rows) the reference evaluates NB independent MLPs order -> H -> H -> 1
// (ReLU) on the same `order` scalars, as grouped nn.Conv1d(k = 1, groups = NB) over [B, NB H, D] tensors (nbm.py:18-51 SeparableMapping,
// nbm.py:54-120 NBMBlock).  Here the whole basis network is one launch: nothing of size M NB H exists in either pass.
//
// Padding: Kp = H rounded up to 32 (a reduction), Np = H rounded up to 16 (a width), KC = Kp / 32, NT = Np / 16.  Every staged small
// vector is zero past H, the packs are zero past H: a padded unit has pre-activation exactly 0, is not live and contributes exactly 0.
//
// cfhip_nbm_pack: W2 f32 [NB, H, H] -> bf16 in v_mfma_f32_16x16x32_bf16 B-fragment order, twice:
//   forward pack    basis g, fragment (j KC + kk), lane l: W2[g][16 j + (l & 15)][32 kk + 8 (l >> 4) + e], e = 0 .. 7
//   transposed pack (after all NB forward packs) basis g, fragment (kt KC + jj), lane l: W2[g][32 jj + 8 (l >> 4) + e][16 kt + (l & 15)]
//
// Operation order of the forward (cfhip_nbm_bases_fwd), per row m and basis g -- what the per-element tests derive their bounds from:
//   u_j     = x[b][idx[d][j]]                                           f32, never rounded
//   pre1_k  = fma(u_{o-1}, w1[k][o-1], ... fma(u_0, w1[k][0], b1[k]))   f32 VALU, o roundings
//   h1_k    = max(pre1_k, 0) as TWO bf16 words, hi = bf16(h1), lo = bf16(h1 - hi): the matrix operand, hi + lo = h1 to 2^-17.  With
//             one word the ReLU masks of layer 2 flipped where pre2 is small, and single flipped units of large gradient put the
//             parameter gradients up to 4 x past the reference's own bf16-autocast distance
//   a_j     = sum_k (hi_k + lo_k) * bf16(W2[j][k])                      one f32 MFMA accumulation chain over 2 KC instructions (hi, lo
//                                                                        per 32 k), from 0
//   pre2_j  = a_j + b2[j]                                               1 rounding;  h2_j = max(pre2_j, 0)
//   p       = fma(h2_j, w3[j], p)  over j = lr, lr + 16, ...            per lane lr = 0 .. 15, NT roundings, from 0
//   s       = the 16 lanes' p folded by xor 1, 2, 4, 8                  4 roundings
//   bases   = s + b3                                                    1 rounding
// One workgroup (256 threads) stages the forward pack of ONE basis in LDS once (Np Kp bf16: 128 KB at H = 256) and loops over its row
// tiles, 16 rows per wave and step; each lane builds its own 8 elements of every A fragment in registers, layer 1 needs no LDS.
//
// The backward saves nothing: it recomputes pre1, h1 and pre2 with the arithmetic above (the same bits, hence the same ReLU masks).
//   nbm_bwd_main_kernel (one wave per workgroup, a basis and a chunk of 16-row tiles):
//     dpre2_j = [pre2_j > 0] dbases w3[j] (1 rounding);  db3 += dbases;  db2_j += dpre2_j;  dw3_j = fma(dbases, h2_j, dw3_j)
//     dh1_k   = sum_j bf16(dpre2_j) * bf16(W2[j][k])       one MFMA chain over KC instructions on the transposed pack
//     dpre1_k = [pre1_k > 0] dh1_k;  db1_k += dpre1_k;  dw1_kj = fma(dpre1_k, u_j, dw1_kj);  du_j = fma(dpre1_k, w1[k][j], du_j)
//     sums over the rows of a tile: 4 rows per lane in row order, then a fold over the 4 lane groups (xor 16, 32); over the tiles of a
//     workgroup in tile order (an f32 LDS accumulator); the workgroup's sums go to a workspace.  du (folded over the 16 lanes of a row by
//     xor 1, 2, 4, 8) goes to a [NB][M][o] f32 partial.
//   nbm_bwd_dw2_kernel (one wave per workgroup: a basis, ONE 16-row block of dW2 and a chunk of 32-row steps):
//     dW2[j][k] = sum_m bf16(dpre2_mj) * (hi + lo)_mk, rows as the MFMA reduction, 32 per instruction pair, f32 accumulators.  The whole
//     dW2[g] is H^2 f32 = 256 KB at H = 256 (256 VGPRs per lane of a 256-thread workgroup), so it is split over workgroups by blocks
//     of 16 rows j: 16 column tiles x 4 = 64 accumulator VGPRs per lane.  A workgroup needs pre2 only for its 16 columns (layer 2 is
//     computed once in total, not once per block); what is repeated per block is layer 1 (VALU).  Both MFMA operands are built in
//     registers: A is the dpre2 accumulator of two 16-row tiles (k-slot 8 q + e <-> row 4 q + e of the first tile for e < 4, row
//     4 q + e - 4 of the second otherwise), B is h1 computed by the lane for the same eight rows.
//   nbm_reduce_kernel: destination = [accumulate ? destination : 0] + (partial 0 + partial 1 + ...), chunks in ascending order.
//   nbm_dx_kernel: dx[b][f] = sum over the (d, j) with idx[d][j] == f, ascending, of (sum_g du partial, g ascending).
// No floating-point atomics anywhere: two identical calls are bit-identical.
#include "common.h"

namespace {

constexpr int NBM_HMAX = CFHIP_NBM_MAX_HIDDEN;
constexpr int NBM_OMAX = CFHIP_NBM_MAX_ORDER;
constexpr int NBM_KCMAX = NBM_HMAX / 32;
constexpr int NBM_NTMAX = NBM_HMAX / 16;
constexpr int NBM_LDP = NBM_HMAX + 8;  // bf16 elements per row of the dpre2 tile (rows 16 bytes apart mod 32 banks)

struct NbmArgs {
  const float* x;       // [B][ldx]
  const int* idx;       // [D][o]
  const float* w1;      // [NB][H][o]
  const float* b1;      // [NB][H]
  const bf16x8* wp;     // forward pack
  const bf16x8* wpt;    // transposed pack
  const float* b2;      // [NB][H]
  const float* w3;      // [NB][H]
  const float* b3;      // [NB]
  float* bases;         // [M][NB] (forward)
  const float* dbases;  // [M][NB] (backward)
  float* part;          // the launch's partial sums
  float* dupart;        // [NB][M][o] or null
  long ldx;
  int M, D, NB, H, o;
  int chunks, tiles_per_chunk;  // row chunks and 16-row tiles (forward, main) / 32-row steps (dW2) per chunk
  int need_h1;                  // main: the part behind dpre2 (dh1, dpre1, dw1, db1, du) is wanted
};

__global__ __launch_bounds__(256) void nbm_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ out, int NB, int H) {
  const int KC = (H + 31) >> 5, NT = (H + 15) >> 4;
  const long per = (long)NB * NT * KC * 64;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= 2 * per) return;
  const bool tr = id >= per;
  const long f = tr ? id - per : id;
  const int lane = (int)(f & 63);
  long frag = f >> 6;
  const int inner = (int)(frag % KC);
  frag /= KC;
  const int outer = (int)(frag % NT);
  const long g = frag / NT;
  const int n = outer * 16 + (lane & 15), k0 = inner * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float x = 0.f;
    if (n < H && k < H) x = tr ? w[(g * H + k) * H + n] : w[(g * H + n) * H + k];
    v[e] = x;
  }
  out[id] = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

// the small vectors of basis g as f32 in LDS, zero past H: w1s [o][P] (transposed: 8 consecutive k are 8 consecutive words), b1s, b2s, w3s [P]
__device__ __forceinline__ void nbm_stage_smalls(const NbmArgs& a, int g, int P, float* w1s, float* b1s, float* b2s, float* w3s, int tid,
                                                 int nthreads) {
  const int H = a.H, o = a.o;
  for (int k = tid; k < P; k += nthreads) {
    const bool in = k < H;
    b1s[k] = in ? a.b1[(long)g * H + k] : 0.f;
    b2s[k] = in ? a.b2[(long)g * H + k] : 0.f;
    w3s[k] = in ? a.w3[(long)g * H + k] : 0.f;
    for (int j = 0; j < o; ++j) w1s[j * P + k] = in ? a.w1[((long)g * H + k) * o + j] : 0.f;
  }
}

// u of row `row` (zeros for a row past M)
__device__ __forceinline__ void nbm_load_u(const NbmArgs& a, long row, float (&u)[NBM_OMAX]) {
#pragma unroll
  for (int j = 0; j < NBM_OMAX; ++j) u[j] = 0.f;
  if (row < a.M) {
    const unsigned b = (unsigned)row / (unsigned)a.D;  // (row < M < 2^31: a 32-bit division)
    const int d = (int)((unsigned)row - b * (unsigned)a.D);
#pragma unroll
    for (int j = 0; j < NBM_OMAX; ++j)
      if (j < a.o) u[j] = a.x[(long)b * a.ldx + a.idx[d * a.o + j]];
  }
}

__device__ __forceinline__ float nbm_pre1(const float (&u)[NBM_OMAX], const float* w1s, const float* b1s, int P, int o, int k) {
  float pre = b1s[k];
#pragma unroll
  for (int j = 0; j < NBM_OMAX; ++j)
    if (j < o) pre = fmaf(u[j], w1s[j * P + k], pre);
  return pre;
}

// eight f32 values as two bf16 words each: hi = bf16(h), lo = bf16(h - hi) (the subtraction is exact; h = hi + lo to 2^-17 relative)
__device__ __forceinline__ void nbm_two_words(const float (&h)[8], bf16x8& hi, bf16x8& lo) {
  const u32x4 w{pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3]), pack_bf16x2(h[4], h[5]), pack_bf16x2(h[6], h[7])};
  float r[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[2 * e] = h[2 * e] - bf16lo(w[e]);
    r[2 * e + 1] = h[2 * e + 1] - bf16hi(w[e]);
  }
  const u32x4 v{pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
  hi = __builtin_bit_cast(bf16x8, w);
  lo = __builtin_bit_cast(bf16x8, v);
}

// the lane's 8 elements of the A fragment of h1 at k0 = 32 kk + 8 (lane >> 4), row (lane & 15), as two words
__device__ __forceinline__ void nbm_h1_frag(const float (&u)[NBM_OMAX], const float* w1s, const float* b1s, int P, int o, int k0, bf16x8& hi,
                                            bf16x8& lo) {
  float h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = fmaxf(nbm_pre1(u, w1s, b1s, P, o, k0 + e), 0.f);
  nbm_two_words(h, hi, lo);
}

__global__ __launch_bounds__(256) void nbm_fwd_kernel(const NbmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = a.H, o = a.o, P = (H + 31) & ~31, KC = P >> 5, NT = (H + 15) >> 4;
  bf16x8* wl = reinterpret_cast<bf16x8*>(smem);
  float* w1s = reinterpret_cast<float*>(smem + (size_t)NT * KC * 64 * 16);
  float* b1s = w1s + NBM_OMAX * P;
  float* b2s = b1s + P;
  float* w3s = b2s + P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int g = blockIdx.x % a.NB, chunk = blockIdx.x / a.NB;
  const bf16x8* src = a.wp + (long)g * NT * KC * 64;
  for (int i = tid; i < NT * KC * 64; i += 256) wl[i] = src[i];
  nbm_stage_smalls(a, g, P, w1s, b1s, b2s, w3s, tid, 256);
  __syncthreads();
  const float b3 = a.b3[g];
  const int tiles = (a.M + 15) >> 4;
  const int t_end = min(tiles, (chunk + 1) * a.tiles_per_chunk);
  for (int t = chunk * a.tiles_per_chunk + wave; t < t_end; t += 4) {
    const long row0 = (long)t * 16;
    float u[NBM_OMAX];
    nbm_load_u(a, row0 + lr, u);
    bf16x8 af[NBM_KCMAX], al[NBM_KCMAX];
#pragma unroll
    for (int kk = 0; kk < NBM_KCMAX; ++kk)
      if (kk < KC) nbm_h1_frag(u, w1s, b1s, P, o, kk * 32 + lq * 8, af[kk], al[kk]);
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < NT; ++j) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NBM_KCMAX; ++kk)
        if (kk < KC) {
          const bf16x8 wf = wl[(j * KC + kk) * 64 + lane];
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], wf, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[kk], wf, acc, 0, 0, 0);
        }
      const int col = j * 16 + lr;
      const float bj = b2s[col], wj = w3s[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = fmaf(fmaxf(acc[i] + bj, 0.f), wj, p[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) p[i] += __shfl_xor(p[i], off, 64);
      const long row = row0 + lq * 4 + i;
      if (lr == 0 && row < a.M) a.bases[row * a.NB + g] = p[i] + b3;
    }
  }
}

// layout of one (chunk, basis) record of the main kernel's partials, (4 + o) P floats: [db2 P][dw3 P][db1 P][db3, then unused, P][dw1 o P ([j][P])]
__global__ __launch_bounds__(64) void nbm_bwd_main_kernel(const NbmArgs a) {
  __shared__ float w1s[NBM_OMAX * NBM_HMAX], b1s[NBM_HMAX], b2s[NBM_HMAX], w3s[NBM_HMAX];
  __shared__ float acc_s[(4 + NBM_OMAX) * NBM_HMAX];  // the record below
  __shared__ float ut[16 * NBM_OMAX];
  __shared__ __attribute__((aligned(16))) bf16_t dpt[16 * NBM_LDP];
  const int H = a.H, o = a.o, P = (H + 31) & ~31, KC = P >> 5, NT = (H + 15) >> 4;
  const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
  const int g = blockIdx.x % a.NB, chunk = blockIdx.x / a.NB;
  nbm_stage_smalls(a, g, P, w1s, b1s, b2s, w3s, lane, 64);
  for (int i = lane; i < (4 + o) * P; i += 64) acc_s[i] = 0.f;
  for (int i = lane; i < 16 * NBM_LDP; i += 64) dpt[i] = 0;
  __syncthreads();
  float* db2a = acc_s;
  float* dw3a = acc_s + P;
  float* db1a = acc_s + 2 * P;
  float* dw1a = acc_s + 4 * P;
  const bf16x8* wg = a.wp + (long)g * NT * KC * 64 + lane;
  const bf16x8* wtg = a.wpt + (long)g * NT * KC * 64 + lane;
  float db3 = 0.f;
  const int tiles = (a.M + 15) >> 4;
  const int t_end = min(tiles, (chunk + 1) * a.tiles_per_chunk);
  for (int t = chunk * a.tiles_per_chunk; t < t_end; ++t) {
    const long row0 = (long)t * 16;
    float u[NBM_OMAX];
    nbm_load_u(a, row0 + lr, u);
    if (lq == 0) {
#pragma unroll
      for (int j = 0; j < NBM_OMAX; ++j) ut[lr * NBM_OMAX + j] = u[j];
    }
    float dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + lq * 4 + i;
      dv[i] = row < a.M ? a.dbases[row * a.NB + g] : 0.f;
    }
    {
      float s = (dv[0] + dv[1]) + (dv[2] + dv[3]);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      db3 += s;
    }
    bf16x8 af[NBM_KCMAX], al[NBM_KCMAX];
#pragma unroll
    for (int kk = 0; kk < NBM_KCMAX; ++kk)
      if (kk < KC) nbm_h1_frag(u, w1s, b1s, P, o, kk * 32 + lq * 8, af[kk], al[kk]);
    for (int j = 0; j < NT; ++j) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NBM_KCMAX; ++kk)
        if (kk < KC) {
          const bf16x8 wf = wg[(j * KC + kk) * 64];
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], wf, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[kk], wf, acc, 0, 0, 0);
        }
      const int col = j * 16 + lr;
      const float bj = b2s[col], wj = w3s[col];
      float s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pre2 = acc[i] + bj;
        const float dp = pre2 > 0.f ? dv[i] * wj : 0.f;
        s2 += dp;
        s3 = fmaf(dv[i], fmaxf(pre2, 0.f), s3);
        dpt[(lq * 4 + i) * NBM_LDP + col] = f32_to_bf16(dp);
      }
      s2 += __shfl_xor(s2, 16, 64);
      s2 += __shfl_xor(s2, 32, 64);
      s3 += __shfl_xor(s3, 16, 64);
      s3 += __shfl_xor(s3, 32, 64);
      if (lq == 0) {
        db2a[col] += s2;
        dw3a[col] += s3;
      }
    }
    __syncthreads();
    if (a.need_h1) {
      float du[4][NBM_OMAX];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NBM_OMAX; ++j) du[i][j] = 0.f;
      for (int kt = 0; kt < NT; ++kt) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jj = 0; jj < NBM_KCMAX; ++jj)
          if (jj < KC) {
            const bf16x8 da = *reinterpret_cast<const bf16x8*>(dpt + lr * NBM_LDP + jj * 32 + lq * 8);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, wtg[(kt * KC + jj) * 64], acc, 0, 0, 0);
          }
        const int k = kt * 16 + lr;
        float sb = 0.f, sw[NBM_OMAX];
#pragma unroll
        for (int j = 0; j < NBM_OMAX; ++j) sw[j] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float ur[NBM_OMAX];
#pragma unroll
          for (int j = 0; j < NBM_OMAX; ++j) ur[j] = ut[(lq * 4 + i) * NBM_OMAX + j];
          const float dp1 = nbm_pre1(ur, w1s, b1s, P, o, k) > 0.f ? acc[i] : 0.f;
          sb += dp1;
#pragma unroll
          for (int j = 0; j < NBM_OMAX; ++j)
            if (j < o) {
              sw[j] = fmaf(dp1, ur[j], sw[j]);
              du[i][j] = fmaf(dp1, w1s[j * P + k], du[i][j]);
            }
        }
        sb += __shfl_xor(sb, 16, 64);
        sb += __shfl_xor(sb, 32, 64);
        if (lq == 0) db1a[k] += sb;
#pragma unroll
        for (int j = 0; j < NBM_OMAX; ++j)
          if (j < o) {
            float s = sw[j];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lq == 0) dw1a[j * P + k] += s;
          }
      }
      if (a.dupart) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long row = row0 + lq * 4 + i;
#pragma unroll
          for (int j = 0; j < NBM_OMAX; ++j)
            if (j < o) {
              float s = du[i][j];
#pragma unroll
              for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
              if (lr == 0 && row < a.M) a.dupart[((long)g * a.M + row) * o + j] = s;
            }
        }
      }
    }
    __syncthreads();
  }
  float* rec = a.part + ((long)chunk * a.NB + g) * ((4L + o) * P);
  for (int i = lane; i < (4 + o) * P; i += 64) rec[i] = i == 3 * P ? db3 : acc_s[i];
}

// two waves per SIMD (256 registers, accumulators included): the second wave is what hides this kernel's LDS and VALU latencies
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void nbm_bwd_dw2_kernel(const NbmArgs a) {
  __shared__ float w1s[NBM_OMAX * NBM_HMAX], b1s[NBM_HMAX], b2s[NBM_HMAX], w3s[NBM_HMAX];
  // u and dbases of the step's 32 rows: gathered ONCE per step (lane r < 32 owns row r) and read from LDS in both fragment layouts;
  // the gather of the next step is issued before this step's arithmetic, so its latency runs under it
  __shared__ float ut[32 * NBM_OMAX], dvs[32];
  const int H = a.H, o = a.o, P = (H + 31) & ~31, KC = P >> 5, NT = (H + 15) >> 4;
  const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
  int bid = blockIdx.x;
  const int jz = bid % NT;
  bid /= NT;
  const int g = bid % a.NB, chunk = bid / a.NB;
  nbm_stage_smalls(a, g, P, w1s, b1s, b2s, w3s, lane, 64);
  __syncthreads();
  bf16x8 wf[NBM_KCMAX];
#pragma unroll
  for (int kk = 0; kk < NBM_KCMAX; ++kk)
    if (kk < KC) wf[kk] = a.wp[((long)g * NT * KC + jz * KC + kk) * 64 + lane];
  const int col = jz * 16 + lr;
  const float bj = b2s[col], wj = w3s[col];
  f32x4 accw[NBM_NTMAX];
#pragma unroll
  for (int kt = 0; kt < NBM_NTMAX; ++kt) accw[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = (a.M + 31) >> 5;
  const int s_end = min(steps, (chunk + 1) * a.tiles_per_chunk);
  float un[NBM_OMAX], dvn = 0.f;
#pragma unroll
  for (int j = 0; j < NBM_OMAX; ++j) un[j] = 0.f;
  auto gather = [&](int step) {
    const long row = (long)step * 32 + lane;
    if (lane < 32) {
      nbm_load_u(a, row, un);
      dvn = row < a.M ? a.dbases[row * a.NB + g] : 0.f;
    }
  };
  if (chunk * a.tiles_per_chunk < s_end) gather(chunk * a.tiles_per_chunk);
  for (int s = chunk * a.tiles_per_chunk; s < s_end; ++s) {
    __syncthreads();  // the previous step has read ut / dvs
    if (lane < 32) {
#pragma unroll
      for (int j = 0; j < NBM_OMAX; ++j) ut[lane * NBM_OMAX + j] = un[j];
      dvs[lane] = dvn;
    }
    __syncthreads();
    if (s + 1 < s_end) gather(s + 1);
    float dp[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float u[NBM_OMAX];
#pragma unroll
      for (int j = 0; j < NBM_OMAX; ++j) u[j] = ut[(t * 16 + lr) * NBM_OMAX + j];
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NBM_KCMAX; ++kk)
        if (kk < KC) {
          bf16x8 hi, lo;
          nbm_h1_frag(u, w1s, b1s, P, o, kk * 32 + lq * 8, hi, lo);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, wf[kk], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, wf[kk], acc, 0, 0, 0);
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dp[t * 4 + i] = acc[i] + bj > 0.f ? dvs[t * 16 + lq * 4 + i] * wj : 0.f;
      }
    }
    const u32x4 dw{pack_bf16x2(dp[0], dp[1]), pack_bf16x2(dp[2], dp[3]), pack_bf16x2(dp[4], dp[5]), pack_bf16x2(dp[6], dp[7])};
    const bf16x8 da = __builtin_bit_cast(bf16x8, dw);
    float ub[8][NBM_OMAX];  // u of the eight rows behind the lane's k-slots
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int j = 0; j < NBM_OMAX; ++j) ub[e][j] = ut[((e >> 2) * 16 + lq * 4 + (e & 3)) * NBM_OMAX + j];
#pragma unroll
    for (int kt = 0; kt < NBM_NTMAX; ++kt)
      if (kt < NT) {
        const int k = kt * 16 + lr;
        float h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = fmaxf(nbm_pre1(ub[e], w1s, b1s, P, o, k), 0.f);
        bf16x8 hi, lo;
        nbm_two_words(h, hi, lo);
        accw[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, hi, accw[kt], 0, 0, 0);
        accw[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, lo, accw[kt], 0, 0, 0);
      }
  }
  float* rec = a.part + ((long)chunk * a.NB + g) * ((long)H * H);
#pragma unroll
  for (int kt = 0; kt < NBM_NTMAX; ++kt)
    if (kt < NT) {
      const int k = kt * 16 + lr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = jz * 16 + lq * 4 + i;
        if (j < H && k < H) rec[(long)j * H + k] = accw[kt][i];
      }
    }
}

// out[g][c] (c < per_group) = [accumulate ? out : 0] + sum over chunks, ascending, of part[(chunk groups + g) stride + off + (c % inner) P + c / inner]
__global__ __launch_bounds__(256) void nbm_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long groups, long per_group,
                                                         long stride, long off, int inner, int P, int chunks, int accumulate) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= groups * per_group) return;
  const long g = id / per_group, c = id - g * per_group;
  const long src = off + (c % inner) * P + c / inner;
  float s = part[g * stride + src];
  for (int r = 1; r < chunks; ++r) s += part[((long)r * groups + g) * stride + src];
  out[id] = accumulate ? out[id] + s : s;
}

__global__ __launch_bounds__(256) void nbm_dx_kernel(const float* __restrict__ dupart, const int* __restrict__ idx, float* __restrict__ dx,
                                                     long B, int F, int D, int o, int NB) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= B * F) return;
  const long b = id / F;
  const int f = (int)(id - b * F);
  const long M = B * D;
  float s = 0.f;
  for (int e = 0; e < D * o; ++e) {
    if (idx[e] != f) continue;
    const long at = (b * D + e / o) * o + e % o;
    float v = dupart[at];
    for (int g = 1; g < NB; ++g) v += dupart[(long)g * M * o + at];
    s += v;
  }
  dx[id] = s;
}

__global__ __launch_bounds__(256) void nbm_featurize_fwd_kernel(const float* __restrict__ bases, const float* __restrict__ wf,
                                                                const float* __restrict__ bf, float* __restrict__ feat, long M, int D, int NB) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int d = (int)(m % D);
  const float* br = bases + m * NB;
  const float* wr = wf + (long)d * NB;
  float s = 0.f;
  for (int g = 0; g < NB; ++g) s = fmaf(br[g], wr[g], s);
  feat[m] = s + bf[d];
}

// thread (d, g) of chunk c walks its samples b in order: dbases = dfeat wf;  dwf partial = fma(dfeat, bases, .);  dbf partial (g == 0) += dfeat
__global__ __launch_bounds__(256) void nbm_featurize_bwd_kernel(const float* __restrict__ dfeat, const float* __restrict__ bases,
                                                                const float* __restrict__ wf, float* __restrict__ dbases, float* __restrict__ part,
                                                                long B, int D, int NB, long per_chunk) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const long DN = (long)D * NB;
  if (id >= DN) return;
  const long d = id / NB;
  const int g = (int)(id - d * NB);
  const long b0 = (long)blockIdx.y * per_chunk, b1 = min(B, b0 + per_chunk);
  const float w = wf[id];
  float sw = 0.f, sb = 0.f;
  for (long b = b0; b < b1; ++b) {
    const float df = dfeat[b * D + d];
    if (dbases) dbases[b * DN + id] = df * w;
    if (bases) sw = fmaf(df, bases[b * DN + id], sw);
    sb += df;
  }
  float* rec = part + (long)blockIdx.y * (DN + D);
  rec[id] = sw;
  if (g == 0) rec[DN + d] = sb;
}

bool nbm_shape_ok(int64_t M, int NB, int H, int o, const char* who) {
  if (H < 8 || H > NBM_HMAX || H % 8 != 0) {
    cfhip_set_error("%s: H = %d is outside the basis kernels (H %% 8 == 0, 8 <= H <= %d)", who, H, NBM_HMAX);
    return false;
  }
  if (o < 1 || o > NBM_OMAX) {
    cfhip_set_error("%s: order = %d is outside the basis kernels (1 <= order <= %d)", who, o, NBM_OMAX);
    return false;
  }
  if (NB < 1 || NB > CFHIP_NBM_MAX_BASES || M < 1 || M >= 0x7fffffffLL) {
    cfhip_set_error("%s: M = B D = %lld rows (1 .. 2^31 - 2), NB = %d (1 .. %d)", who, (long long)M, NB, CFHIP_NBM_MAX_BASES);
    return false;
  }
  return true;
}

// row chunks of a launch with `units` row units per basis and `groups` one-wave workgroups per chunk: `waves` workgroups in all when the
// rows allow it (the kernels hide the latency of their L2 reads only behind other waves), at least `min_units` units per chunk (every
// chunk costs a record of partials in the workspace, which must stay small against the rows it sums)
int nbm_chunks(long units, long groups, long waves, long min_units) {
  const long want = (waves + groups - 1) / groups;
  return (int)max(1L, min(units / min_units, want));
}

struct NbmPlan {
  int chunks1, tpc1;  // main: chunks of 16-row tiles
  int chunks2, tpc2;  // dW2: chunks of 32-row steps
  size_t off2, offdu, bytes;
};

NbmPlan nbm_plan(int64_t M, int NB, int H, int o, int want_dx) {
  NbmPlan p;
  const long P = (H + 31) / 32 * 32, NT = (H + 15) / 16;
  const long tiles = (M + 15) / 16, steps = (M + 31) / 32;
  p.chunks1 = nbm_chunks(tiles, NB, 4096, 4);
  p.tpc1 = (int)((tiles + p.chunks1 - 1) / p.chunks1);
  p.chunks1 = (int)((tiles + p.tpc1 - 1) / p.tpc1);
  p.chunks2 = nbm_chunks(steps, (long)NB * NT, 2048, 8);
  p.tpc2 = (int)((steps + p.chunks2 - 1) / p.chunks2);
  p.chunks2 = (int)((steps + p.tpc2 - 1) / p.tpc2);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  p.off2 = up(sizeof(float) * p.chunks1 * NB * (4 + o) * P);
  p.offdu = p.off2 + up(sizeof(float) * p.chunks2 * NB * H * H);
  p.bytes = p.offdu + (want_dx ? up(sizeof(float) * NB * M * o) : 0);
  return p;
}

int nbm_fwd_lds(int H) {
  const int P = (H + 31) / 32 * 32, Np = (H + 15) / 16 * 16;
  return Np * P * 2 + (NBM_OMAX + 3) * P * 4;
}

}  // namespace

extern "C" size_t cfhip_nbm_pack_workspace(int NB, int H) {
  if (H < 8 || H > NBM_HMAX || H % 8 != 0 || NB < 1 || NB > CFHIP_NBM_MAX_BASES) return 0;
  return 2 * sizeof(bf16_t) * (size_t)NB * ((H + 15) / 16 * 16) * ((H + 31) / 32 * 32);
}

extern "C" int cfhip_nbm_pack(const float* w2, void* packed, size_t packed_bytes, int NB, int H, void* stream) {
  if (!nbm_shape_ok(1, NB, H, 1, "nbm_pack")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(w2 && packed, "nbm_pack: null operand");
  CFHIP_REQUIRE(packed_bytes == cfhip_nbm_pack_workspace(NB, H), "nbm_pack: `packed` holds %zu bytes, cfhip_nbm_pack_workspace says %zu",
                packed_bytes, cfhip_nbm_pack_workspace(NB, H));
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)w2 & 3) == 0, "nbm_pack: misaligned operand");
  const long lanes = (long)(packed_bytes / 16);
  hipLaunchKernelGGL(nbm_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w2,
                     reinterpret_cast<u32x4*>(packed), NB, H);
  CFHIP_CHECK_LAUNCH("nbm_pack");
  return CFHIP_OK;
}

extern "C" int cfhip_nbm_bases_fwd(const float* x, int64_t ldx, const int* idx, const float* w1, const float* b1, const void* packed,
                                   const float* b2, const float* w3, const float* b3, float* bases, int64_t B, int D, int NB, int H,
                                   int order, void* stream) {
  CFHIP_REQUIRE(B >= 1 && B < 0x7fffffffLL && D >= 1, "nbm_bases_fwd: B = %lld, D = %d", (long long)B, D);
  const int64_t M = B * D;
  if (!nbm_shape_ok(M, NB, H, order, "nbm_bases_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(x && idx && w1 && b1 && packed && b2 && w3 && b3 && bases, "nbm_bases_fwd: null operand");
  CFHIP_REQUIRE(ldx >= 1, "nbm_bases_fwd: row stride %lld of x", (long long)ldx);
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0, "nbm_bases_fwd: `packed` must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)idx | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)w3 | (uintptr_t)b3 |
                  (uintptr_t)bases) & 3) == 0, "nbm_bases_fwd: misaligned operand");
  const long tiles = (M + 15) / 16;
  const int want = max(1, 2048 / NB);
  int chunks = (int)max(1L, min((tiles + 3) / 4, (long)want));
  const int tpc = (int)((tiles + chunks - 1) / chunks);
  chunks = (int)((tiles + tpc - 1) / tpc);
  const int lds = nbm_fwd_lds(H);
  // more than 64 KB of dynamic LDS needs the attribute; set on every call (a host-side setting of the current device, no launch)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(nbm_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  CFHIP_REQUIRE(e == hipSuccess, "nbm_bases_fwd: cannot reserve %d bytes of LDS: %s", lds, hipGetErrorString(e));
  const size_t fwd_frags = cfhip_nbm_pack_workspace(NB, H) / 32;
  NbmArgs a{};
  a.x = x, a.idx = idx, a.w1 = w1, a.b1 = b1, a.wp = reinterpret_cast<const bf16x8*>(packed), a.wpt = a.wp + fwd_frags;
  a.b2 = b2, a.w3 = w3, a.b3 = b3, a.bases = bases, a.ldx = (long)ldx;
  a.M = (int)M, a.D = D, a.NB = NB, a.H = H, a.o = order, a.chunks = chunks, a.tiles_per_chunk = tpc;
  hipLaunchKernelGGL(nbm_fwd_kernel, dim3((unsigned)chunks * NB), dim3(256), lds, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("nbm_bases_fwd");
  return CFHIP_OK;
}

// bytes of the backward's workspace (0 for a shape the kernels refuse, never 0 otherwise)
extern "C" size_t cfhip_nbm_bases_bwd_workspace(int64_t M, int NB, int H, int order, int want_dx) {
  if (H < 8 || H > NBM_HMAX || H % 8 != 0 || order < 1 || order > NBM_OMAX || NB < 1 || NB > CFHIP_NBM_MAX_BASES || M < 1 ||
      M >= 0x7fffffffLL)
    return 0;
  return nbm_plan(M, NB, H, order, want_dx).bytes;
}

extern "C" int cfhip_nbm_bases_bwd(const float* dbases, const float* x, int64_t ldx, const int* idx, const float* w1, const float* b1,
                                   const void* packed, const float* b2, const float* w3, float* dw1, float* db1, float* dw2, float* db2,
                                   float* dw3, float* db3, float* dx, int accumulate, void* workspace, size_t workspace_bytes, int64_t B,
                                   int D, int F, int NB, int H, int order, void* stream) {
  CFHIP_REQUIRE(B >= 1 && B < 0x7fffffffLL && D >= 1, "nbm_bases_bwd: B = %lld, D = %d", (long long)B, D);
  const int64_t M = B * D;
  if (!nbm_shape_ok(M, NB, H, order, "nbm_bases_bwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(dbases && x && idx && w1 && b1 && packed && b2 && w3 && workspace, "nbm_bases_bwd: null operand");
  CFHIP_REQUIRE(ldx >= 1 && (!dx || (F >= 1 && B * (int64_t)F < 0x7fffffffLL * 256)), "nbm_bases_bwd: ldx = %lld, F = %d", (long long)ldx, F);
  CFHIP_REQUIRE((accumulate & ~63) == 0, "nbm_bases_bwd: `accumulate` = %d has bits past the six destinations", accumulate);
  const NbmPlan p = nbm_plan(M, NB, H, order, dx != nullptr);
  CFHIP_REQUIRE(workspace_bytes >= p.bytes, "nbm_bases_bwd: the workspace holds %zu bytes, cfhip_nbm_bases_bwd_workspace says %zu",
                workspace_bytes, p.bytes);
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "nbm_bases_bwd: `packed` and the workspace must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)dbases | (uintptr_t)x | (uintptr_t)idx | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)w3 |
                  (uintptr_t)dw1 | (uintptr_t)db1 | (uintptr_t)dw2 | (uintptr_t)db2 | (uintptr_t)dw3 | (uintptr_t)db3 | (uintptr_t)dx) & 3) == 0,
                "nbm_bases_bwd: misaligned operand");
  const int P = (H + 31) / 32 * 32, NT = (H + 15) / 16;
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  const size_t fwd_frags = cfhip_nbm_pack_workspace(NB, H) / 32;
  NbmArgs a{};
  a.x = x, a.idx = idx, a.w1 = w1, a.b1 = b1, a.wp = reinterpret_cast<const bf16x8*>(packed), a.wpt = a.wp + fwd_frags;
  a.b2 = b2, a.w3 = w3, a.dbases = dbases, a.ldx = (long)ldx;
  a.M = (int)M, a.D = D, a.NB = NB, a.H = H, a.o = order;
  auto reduce = [&](const float* part, float* out, long per_group, long stride, long off, int inner, int chunks, int acc) {
    const long n = (long)NB * per_group;
    hipLaunchKernelGGL(nbm_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, out, (long)NB, per_group, stride, off,
                       inner, P, chunks, acc);
  };
  const bool need_h1 = dw1 || db1 || dx;
  if (need_h1 || db2 || dw3 || db3) {
    float* part = reinterpret_cast<float*>(ws);
    a.part = part, a.dupart = dx ? reinterpret_cast<float*>(ws + p.offdu) : nullptr;
    a.chunks = p.chunks1, a.tiles_per_chunk = p.tpc1, a.need_h1 = need_h1;
    hipLaunchKernelGGL(nbm_bwd_main_kernel, dim3((unsigned)p.chunks1 * NB), dim3(64), 0, s, a);
    CFHIP_CHECK_LAUNCH("nbm_bases_bwd");
    const long stride = (4L + order) * P;
    if (db2) reduce(part, db2, H, stride, 0, 1, p.chunks1, accumulate >> 3 & 1);
    if (dw3) reduce(part, dw3, H, stride, P, 1, p.chunks1, accumulate >> 4 & 1);
    if (db1) reduce(part, db1, H, stride, 2L * P, 1, p.chunks1, accumulate >> 1 & 1);
    if (dw1) reduce(part, dw1, (long)H * order, stride, 4L * P, order, p.chunks1, accumulate & 1);
    if (db3) reduce(part, db3, 1, stride, 3L * P, 1, p.chunks1, accumulate >> 5 & 1);
    if (dx) {
      const long n = B * F;
      hipLaunchKernelGGL(nbm_dx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.dupart, idx, dx, (long)B, F, D, order, NB);
    }
  }
  if (dw2) {
    float* part = reinterpret_cast<float*>(ws + p.off2);
    a.part = part, a.dupart = nullptr, a.chunks = p.chunks2, a.tiles_per_chunk = p.tpc2;
    hipLaunchKernelGGL(nbm_bwd_dw2_kernel, dim3((unsigned)p.chunks2 * NB * NT), dim3(64), 0, s, a);
    CFHIP_CHECK_LAUNCH("nbm_bases_bwd");
    reduce(part, dw2, (long)H * H, (long)H * H, 0, 1, p.chunks2, accumulate >> 2 & 1);
  }
  CFHIP_CHECK_LAUNCH("nbm_bases_bwd");
  return CFHIP_OK;
}

namespace {
int nbm_feat_chunks(int64_t B) { return (int)max((int64_t)1, min((int64_t)64, (B + 63) / 64)); }
bool nbm_feat_ok(int64_t B, int D, int NB, const char* who) {
  if (B < 1 || D < 1 || NB < 1 || NB > CFHIP_NBM_MAX_BASES || B * D >= 0x7fffffffLL || (int64_t)D * NB >= 0x7fffffffLL) {
    cfhip_set_error("%s: B = %lld, D = %d, NB = %d", who, (long long)B, D, NB);
    return false;
  }
  return true;
}
}  // namespace

extern "C" int cfhip_nbm_featurize_fwd(const float* bases, const float* wf, const float* bf, float* feat, int64_t B, int D, int NB,
                                       void* stream) {
  if (!nbm_feat_ok(B, D, NB, "nbm_featurize_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(bases && wf && bf && feat, "nbm_featurize_fwd: null operand");
  CFHIP_REQUIRE((((uintptr_t)bases | (uintptr_t)wf | (uintptr_t)bf | (uintptr_t)feat) & 3) == 0, "nbm_featurize_fwd: misaligned operand");
  const long M = B * D;
  hipLaunchKernelGGL(nbm_featurize_fwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bases, wf, bf, feat, M,
                     D, NB);
  CFHIP_CHECK_LAUNCH("nbm_featurize_fwd");
  return CFHIP_OK;
}

extern "C" size_t cfhip_nbm_featurize_bwd_workspace(int64_t B, int D, int NB) {
  if (B < 1 || D < 1 || NB < 1 || NB > CFHIP_NBM_MAX_BASES || B * D >= 0x7fffffffLL || (int64_t)D * NB >= 0x7fffffffLL) return 0;
  return sizeof(float) * (size_t)nbm_feat_chunks(B) * ((size_t)D * NB + D);
}

extern "C" int cfhip_nbm_featurize_bwd(const float* dfeat, const float* bases, const float* wf, float* dbases, float* dwf, float* dbf,
                                       int accumulate, void* workspace, size_t workspace_bytes, int64_t B, int D, int NB, void* stream) {
  if (!nbm_feat_ok(B, D, NB, "nbm_featurize_bwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(dfeat && wf && workspace && (bases || !dwf), "nbm_featurize_bwd: null operand (dfeat, wf and the workspace; bases for dwf)");
  CFHIP_REQUIRE((accumulate & ~3) == 0, "nbm_featurize_bwd: `accumulate` = %d has bits past the two destinations", accumulate);
  CFHIP_REQUIRE(workspace_bytes >= cfhip_nbm_featurize_bwd_workspace(B, D, NB),
                "nbm_featurize_bwd: the workspace holds %zu bytes, cfhip_nbm_featurize_bwd_workspace says %zu", workspace_bytes,
                cfhip_nbm_featurize_bwd_workspace(B, D, NB));
  CFHIP_REQUIRE((((uintptr_t)dfeat | (uintptr_t)bases | (uintptr_t)wf | (uintptr_t)dbases | (uintptr_t)dwf | (uintptr_t)dbf |
                  (uintptr_t)workspace) & 3) == 0, "nbm_featurize_bwd: misaligned operand");
  if (!dbases && !dwf && !dbf) return CFHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = nbm_feat_chunks(B);
  const long per_chunk = (B + chunks - 1) / chunks, DN = (long)D * NB;
  float* part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(nbm_featurize_bwd_kernel, dim3((unsigned)((DN + 255) / 256), (unsigned)chunks), dim3(256), 0, s, dfeat,
                     dwf ? bases : nullptr, wf, dbases, part, (long)B, D, NB, per_chunk);
  CFHIP_CHECK_LAUNCH("nbm_featurize_bwd");
  if (dwf)
    hipLaunchKernelGGL(nbm_reduce_kernel, dim3((unsigned)((DN + 255) / 256)), dim3(256), 0, s, part, dwf, 1L, DN, DN + D, 0L, 1, 0, chunks,
                       accumulate & 1);
  if (dbf)
    hipLaunchKernelGGL(nbm_reduce_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, part, dbf, 1L, (long)D, DN + D, DN, 1, 0, chunks,
                       accumulate >> 1 & 1);
  CFHIP_CHECK_LAUNCH("nbm_featurize_bwd");
  return CFHIP_OK;
}
