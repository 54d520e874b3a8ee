// K3/K4: fused scaled-dot-product attention (forward + backward) for gfx950, head_dim 64,
// sequence lengths up to 256 (the whole K / V of one head is resident in LDS: ViT-B/16 has T = 197).
//
// Replaces F.scaled_dot_product_attention reached through sdp_attn (reference toolkit.py:953-963)
// from Attention.forward (attentions.py:254), including the head split / merge permute copies
// (attentions.py:180-185, 270-275): q / k / v are read in place from the packed [B,T,3,H,64]
// projection output and o is written directly as [B,T,H*64].
//
// Structure (all on v_mfma_f32_16x16x32_bf16, one 16-row tile per wave):
//   * "swapped" products: S^T = K Q^T, so that a lane holds 4 consecutive kv positions of ONE query
//     row (row = lane & 15) -> the row softmax is lane-local plus two xor-shuffles (16, 32), and the
//     bf16-packed probabilities are directly the register operand of the P·V MFMA (the k-slot
//     permutation this implies is matched on the V side, a dot product does not care about order).
//   * K / V / Q / dO tiles sit in LDS as [rows][64] bf16 with an XOR swizzle of the 16-byte slots;
//     row-operand fragments are ds_read_b128, column-operand fragments (V in P·V, K in dS·K,
//     dO and Q in the dK/dV pass) are ds_read_b64_tr_b16 hardware-transpose reads.
//   * backward = two passes without atomics: pass A (wave = query tile) recomputes S and dP and
//     accumulates dQ; pass B (wave = kv tile) recomputes them transposed and accumulates dK, dV.
//     Deterministic; costs 7 instead of 5 GEMM units, attention is 3.4 % of the ViT FLOPs.
#include "common.h"
#include "attn_device.h"
#include "attn_host.h"
#include <math.h>

using namespace cfhip_attn;

namespace {

// ------------------------------------------------------------------------------------------------
// The per-tile arithmetic a one-shot kernel and its persistent twin share, stated once where hipcc lets it be: the 64-deep
// products (product64, csrc/attn_device.h), the PLAIN max / exp2 / sum pass, the row delta and the dS operand of the dQ pass.
// Tried and NOT kept (profiles/r14/attn_split_isa.txt: registers, scratch, occupancy and the wait / LDS / MFMA sequence of every
// instantiation must not move): any helper that takes a kernel's accumulator or score ARRAY by reference — the score tiles (one
// wait of attn_fwd_kernel<7, true> moves), the tail masking (attn_fwd_kernel<1, true>: 49 -> 57 registers), the P·V, dQ and
// dK / dV accumulations (registers and schedules of most instantiations) — and the P / dS operands of the dK / dV pass, which
// return values as the dQ one does (attn_bwd_dkv_kernel<true>: 112 -> 114 registers).  Those bodies stay written out in both
// kernels of a pair; edit them together.
// ------------------------------------------------------------------------------------------------

// PLAIN softmax of the masked scores in place (st <- exp2(s * sl2 - mx)): mx (-inf on entry) = the row maximum (scaled, log2 domain), l = the row sum
template <int NB>
__device__ __forceinline__ void softmax_plain(f32x4 (&st)[2 * NB], float sl2, float& mx, float& l) {
  // (sl2 > 0: the maximum commutes with the scaling, so the pass over the 8 NB scores per lane is max only and the
  // scaling rides in the FMA of the exponent: e = exp2(s * sl2 - max * sl2), two scores per v_pk_fma_f32 / v_pk_add_f32)
#pragma unroll
  for (int jt = 0; jt < 2 * NB; ++jt) mx = fmaxf(mx, fmaxf(fmaxf(st[jt][0], st[jt][1]), fmaxf(st[jt][2], st[jt][3])));
  mx = group_max(mx) * sl2;
  const f32x4 sc4 = {sl2, sl2, sl2, sl2}, nm4 = {-mx, -mx, -mx, -mx};
  f32x4 l4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jt = 0; jt < 2 * NB; ++jt) {
    const f32x4 x = __builtin_elementwise_fma(st[jt], sc4, nm4);
    f32x4 e;
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(x[r]);  // raw v_exp_f32: arguments are <= 0
    st[jt] = e;
    l4 += e;
  }
  l = group_sum((l4[0] + l4[1]) + (l4[2] + l4[3]));
}

// delta_i = sum_d dO[i][d] * O[i][d] from the row fragments of a query tile
__device__ __forceinline__ float row_delta(const bf16x8& dof0, const bf16x8& dof1, const bf16x8& of0, const bf16x8& of1) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s += bf16_to_f32((bf16_t)dof0[e]) * bf16_to_f32((bf16_t)of0[e]);
    s += bf16_to_f32((bf16_t)dof1[e]) * bf16_to_f32((bf16_t)of1[e]);
  }
  return group_sum(s);
}

// dS of one query tile against the 32 keys of block a, packed as an MFMA operand: dS = exp2(s * sl2 - lse2) (dP - delta); the mask
// predicate (!PLAIN, row `qrow` of the mask) acts on the probability
template <bool PLAIN>
__device__ __forceinline__ bf16x8 dq_ds(const char* Ks, const char* Vs, int a, const bf16x8& qf0, const bf16x8& qf1, const bf16x8& dof0,
                                        const bf16x8& dof1, float sl2, float lse2, float delta, const AttnParams& p, int b, int h,
                                        int qrow, int lane) {
  const int g = lane >> 4;
  f32x4 ds[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int jt = 2 * a + t;
    const f32x4 s = product64(Ks, jt * 16, qf0, qf1, lane), dp = product64(Vs, jt * 16, dof0, dof1, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pr = __builtin_amdgcn_exp2f(s[r] * sl2 - lse2);
      if (!PLAIN) pr = keep_at(p, b, h, qrow, jt * 16 + 4 * g + r) ? pr : 0.f;
      ds[t][r] = pr * (dp[r] - delta);
    }
  }
  return pack8(ds[0], ds[1]);
}

// ------------------------------------------------------------------------------------------------
// forward: workgroup = (query chunk of nwaves*16 rows, head, batch); NB = ceil(Tk / 32)
// ------------------------------------------------------------------------------------------------
// PLAIN = no mask, not causal (the ViT path): the only masking is the kv tail (j >= Tk), decided per
// 16-wide tile with wave-uniform branches — no per-element predicate registers.
template <int NB, bool PLAIN>
__global__ __launch_bounds__(512, 4) void attn_fwd_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + NB * 32 * 128;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * DH;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * DH;
  if (!ATTN_ABL(1)) {
    dma_tile(Ks, kb, p.kv_st, p.Tk, NB * 32, wave, nwaves, lane);
    dma_tile(Vs, vb, p.kv_st, p.Tk, NB * 32, wave, nwaves, lane);
  }
  lds_dma_wait_all();
  __syncthreads();  // (drains the DMA: vmcnt(0) + barrier)
  if (ATTN_ABL(2)) return;

  const int i = lane & 15, g = lane >> 4;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * DH;
  // K / V are loaded once per (batch, head); the waves walk the query tiles
  for (int row0 = (blockIdx.x * nwaves + wave) * 16; row0 < p.Tq; row0 += gridDim.x * nwaves * 16) {
  const int qi = row0 + i;
  const bf16x8 qf0 = frag_global(qb, p.q_st, row0, p.Tq, 0, lane);
  const bf16x8 qf1 = frag_global(qb, p.q_st, row0, p.Tq, 1, lane);

  f32x4 st[2 * NB];
#pragma unroll
  for (int jt = 0; jt < 2 * NB; ++jt) {
    st[jt] = product64(Ks, jt * 16, qf0, qf1, lane);
    if (jt & 1) __builtin_amdgcn_sched_barrier(0);  // at most 4 K fragments in flight: 128 VGPRs, 4 waves / SIMD
  }
  // row max / sum of the scaled scores in the log2 domain, masked
  const float sl2 = p.scale * LOG2E;
  float mx = -INFINITY;
  float l = 0.f;
  if (PLAIN) {
    // (sl2 > 0: the maximum commutes with the scaling, so the pass over the 8 NB scores per lane is max only and the
    // scaling rides in the FMA of the exponent: e = exp2(s * sl2 - max * sl2), two scores per v_pk_fma_f32 / v_pk_add_f32)
#pragma unroll
    for (int jt = 2 * NB - 2; jt < 2 * NB; ++jt) {  // nb = ceil(Tk / 32): only the last two tiles can touch the kv tail
      if (jt * 16 >= p.Tk) {                         // tile entirely past the end (wave-uniform)
        st[jt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      } else if (jt * 16 + 15 >= p.Tk) {             // the tile straddling Tk
#pragma unroll
        for (int r = 0; r < 4; ++r) st[jt][r] = (jt * 16 + 4 * g + r < p.Tk) ? st[jt][r] : -INFINITY;
      }
    }
    softmax_plain<NB>(st, sl2, mx, l);
  } else {
#pragma unroll
    for (int jt = 0; jt < 2 * NB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jt * 16 + 4 * g + r;
        const float x = keep_at(p, b, h, qi < p.Tq ? qi : p.Tq - 1, j) ? st[jt][r] * sl2 : -INFINITY;
        st[jt][r] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = group_max(mx);
#pragma unroll
    for (int jt = 0; jt < 2 * NB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(st[jt][r] - mx);  // raw v_exp_f32: arguments are <= 0
        st[jt][r] = e;
        l += e;
      }
    }
    l = group_sum(l);
  }

  // O^T[d][i] = sum_j V^T[d][j] P^T[j][i]   (operands swapped: lane ends with 4 consecutive d of row i)
  f32x4 ot[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < NB; ++a) {
    const bf16x8 pa = pack8(st[2 * a], st[2 * a + 1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Vs, a * 32, dt * 16, lane), pa, ot[dt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  {
    const bool valid = qi < p.Tq && !ATTN_ABL(4);
    const float inv = 1.0f / l;
    store_row64(p.o + (long)b * p.o_sb + (long)qi * p.o_st + h * DH, ot, inv, g, valid);
    if (valid && g == 0 && p.lse != nullptr)
      p.lse[((long)b * p.H + h) * p.Tq + qi] = (mx + log2f(l)) * (1.0f / LOG2E);
  }
  }  // query-tile loop
}

// ------------------------------------------------------------------------------------------------
// backward pass A: dQ (and delta = rowsum(dO * O)).  workgroup as in forward; K, V in LDS.
// ------------------------------------------------------------------------------------------------
// PLAIN (no mask, not causal): no predicate at all — kv rows past Tk are ZERO in LDS (DMA range check),
// so their dS (finite: s = 0, dP = 0) meets K = 0 in the dQ product; padded query rows carry lse = +inf.
template <bool PLAIN>
__global__ __launch_bounds__(512, 4) void attn_bwd_dq_kernel(AttnParams p, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + nb * 32 * 128;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  dma_tile(Ks, p.k + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, nb * 32, wave, nwaves, lane);
  dma_tile(Vs, p.v + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, nb * 32, wave, nwaves, lane);
  lds_dma_wait_all();
  __syncthreads();

  const int i = lane & 15, g = lane >> 4;
  for (int row0 = (blockIdx.x * nwaves + wave) * 16; row0 < p.Tq; row0 += gridDim.x * nwaves * 16) {
  const int qi = row0 + i;
  const bool qvalid = qi < p.Tq;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * DH;
  const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * DH;
  const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * DH;
  const bf16x8 qf0 = frag_global(qb, p.q_st, row0, p.Tq, 0, lane);
  const bf16x8 qf1 = frag_global(qb, p.q_st, row0, p.Tq, 1, lane);
  const bf16x8 dof0 = frag_global(dob, p.o_st, row0, p.Tq, 0, lane);
  const bf16x8 dof1 = frag_global(dob, p.o_st, row0, p.Tq, 1, lane);
  float delta = row_delta(dof0, dof1, frag_global(ob, p.o_st, row0, p.Tq, 0, lane), frag_global(ob, p.o_st, row0, p.Tq, 1, lane));
  if (!PLAIN) delta = finite_or_zero(delta);
  const long stat = ((long)b * p.H + h) * p.Tq + qi;
  if (qvalid && g == 0) p.delta[stat] = delta;
  const float lse2 = qvalid ? p.lse[stat] * LOG2E : INFINITY;  // +inf -> p = 0 for padded rows
  const float sl2 = p.scale * LOG2E;

  f32x4 dqt[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dqt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int a = 0; a < nb; ++a) {
    const bf16x8 dsp = dq_ds<PLAIN>(Ks, Vs, a, qf0, qf1, dof0, dof1, sl2, lse2, delta, p, b, h, qvalid ? qi : p.Tq - 1, lane);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dqt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Ks, a * 32, dt * 16, lane), dsp, dqt[dt], 0, 0, 0);
  }
  store_row64(p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * DH, dqt, p.scale, g, qvalid);
  }  // query-tile loop
}

// ------------------------------------------------------------------------------------------------
// backward pass B: dK, dV.  workgroup = (kv chunk of nwaves*16 rows, head, batch); Q, dO, lse,
// delta of the whole head in LDS; nbq = ceil(Tq / 32).
// ------------------------------------------------------------------------------------------------
// PLAIN: no predicate — a kv row past Tk only pollutes its own (never stored) dK / dV row, padded query
// rows carry lse = +inf (p = 0).
template <bool PLAIN>
__global__ __launch_bounds__(512, PLAIN ? 4 : 2) void attn_bwd_dkv_kernel(AttnParams p, int nbq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = smem + nbq * 32 * 128;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * nbq * 32 * 128);
  float* delta_s = lse_s + nbq * 32;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  if (!ATTN_ABL(1)) {
  dma_tile(Qs, p.q + (long)b * p.q_sb + h * DH, p.q_st, p.Tq, nbq * 32, wave, nwaves, lane);
  dma_tile(dOs, p.d_o + (long)b * p.o_sb + h * DH, p.o_st, p.Tq, nbq * 32, wave, nwaves, lane);
  // lse and delta_i = sum_d dO[i][d] * O[i][d] of every query row (delta is recomputed here from the
  // L2-resident dO / O rows so that this pass does not depend on the dQ pass: the two kernels run
  // concurrently on two streams).  8 consecutive lanes own the 8 16-byte slots of one row.
  for (int idx = threadIdx.x; idx < nbq * 32 * 8; idx += blockDim.x) {
    const int t = idx >> 3, slot = idx & 7;
    float s = 0.f;
    if (p.delta_ready) {
      if (slot == 0 && t < p.Tq) s = p.delta[((long)b * p.H + h) * p.Tq + t];
    } else if (t < p.Tq) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(p.d_o + (long)b * p.o_sb + (long)t * p.o_st + h * DH + slot * 8);
      const u32x4 c = *reinterpret_cast<const u32x4*>(p.o_in + (long)b * p.o_sb + (long)t * p.o_st + h * DH + slot * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += bf16lo(a[e]) * bf16lo(c[e]) + bf16hi(a[e]) * bf16hi(c[e]);
    }
    if (!p.delta_ready) {
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
    }
    if (slot == 0) {
      delta_s[t] = PLAIN ? s : finite_or_zero(s);
      lse_s[t] = t < p.Tq ? p.lse[((long)b * p.H + h) * p.Tq + t] * LOG2E : INFINITY;
    }
  }
  }
  lds_dma_wait_all();
  __syncthreads();
  if (ATTN_ABL(2)) return;

  const int n = lane & 15, g = lane >> 4;
  for (int row0 = (blockIdx.x * nwaves + wave) * 16; row0 < p.Tk; row0 += gridDim.x * nwaves * 16) {
  const int kj = row0 + n;  // kv rows of this wave
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * DH;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * DH;
  const bf16x8 kf0 = frag_global(kb, p.kv_st, row0, p.Tk, 0, lane);
  const bf16x8 kf1 = frag_global(kb, p.kv_st, row0, p.Tk, 1, lane);
  const bf16x8 vf0 = frag_global(vb, p.kv_st, row0, p.Tk, 0, lane);
  const bf16x8 vf1 = frag_global(vb, p.kv_st, row0, p.Tk, 1, lane);
  const float sl2 = p.scale * LOG2E;

  f32x4 dkt[4], dvt[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int a = 0; a < nbq; ++a) {
    f32x4 pp[2], ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int it = 2 * a + t;
      // S[i][j] with lane <- rows i = it*16 + 4g + r, column j = kj
      const f32x4 s = product64(Qs, it * 16, kf0, kf1, lane), dp = product64(dOs, it * 16, vf0, vf1, lane);
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + it * 16 + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_s + it * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pr = __builtin_amdgcn_exp2f(s[r] * sl2 - l4[r]);
        if (!PLAIN) {
          const int qi = it * 16 + 4 * g + r;
          pr = (qi < p.Tq && keep_at(p, b, h, qi, kj)) ? pr : 0.f;
        }
        pp[t][r] = pr;
        ds[t][r] = pr * (dp[r] - d4[r]);
      }
    }
    const bf16x8 ppk = pack8(pp[0], pp[1]);
    const bf16x8 dsk = pack8(ds[0], ds[1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(dOs, a * 32, dt * 16, lane), ppk, dvt[dt], 0, 0, 0);
      dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Qs, a * 32, dt * 16, lane), dsk, dkt[dt], 0, 0, 0);
    }
  }
  {
    const bool valid = kj < p.Tk && !ATTN_ABL(4);
    store_row64(p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dkt, p.scale, g, valid);
    store_row64(p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dvt, 1.0f, g, valid);
  }
  }  // kv-tile loop
}

// ------------------------------------------------------------------------------------------------
// Persistent form of the dK/dV pass (PLAIN only, sequence lengths 129 .. 256 = the ViT step).
// One 16-wave workgroup per CU walks (batch, head) pairs; the operands of the NEXT head stream into a second LDS buffer
// while the waves work on the current one.  In the one-shot kernels above the prologue DMA (57 KB per head) is not
// covered by anything: every workgroup of a launch sits in it at the same time.  Worth 8 % on this pass alone and 40 us of
// its in-step duration, nothing on the wall clock of the step (profiles/r02/attn_vit_ablation.log); the same form of the
// forward and dQ passes was built, measured (no gain alone or in the step) and removed.  The DMA / statistics loads of the next head are issued UNCONDITIONALLY (out of
// range offsets when there is no next head), right after this head's own fragment loads, so that the compiler's vmcnt
// bookkeeping can wait for the fragments while the younger DMA stays in flight.
// ------------------------------------------------------------------------------------------------

// 2 instructions per wave cover up to 256 rows (32 instructions of 8 rows)
__device__ __forceinline__ void dma_tile_pers(char* tile, const bf16_t* base, long stride_t, int rows_valid, bool live,
                                              int wave, int lane) {
  const __amdgpu_buffer_rsrc_t rsrc = dma_rsrc(base, stride_t, rows_valid, DH, live);
#pragma unroll
  for (int j = 0; j < 2; ++j) dma_rows8(rsrc, tile, wave + j * PERS_WAVES, stride_t, rows_valid, 0, DH, lane, live);
}

template <int NBQ>
__global__ __launch_bounds__(PERS_WAVES * 64, 4) void attn_bwd_dkv_pers_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // every wave issues 2 DMA instructions per operand whatever NBQ is (a fixed count the compiler can wait on): the tile
  // slot is 256 rows, the instructions beyond ROWS write zeros into its padding
  constexpr int ROWS = NBQ * 32, TILE = 256 * 128, BUF = 2 * TILE + 2 * ROWS * 4;
  static_assert(ROWS <= 256 && ROWS * 8 <= 2 * PERS_WAVES * 64, "two DMA instructions / two statistics slots per thread");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int heads = p.B * p.H;
  const float sl2 = p.scale * LOG2E;

  auto issue = [&](int hh, char* buf, bool live) {
    const int b = hh / p.H, h = hh - b * p.H;
    dma_tile_pers(buf, p.q + (long)b * p.q_sb + h * DH, p.q_st, p.Tq, live, wave, lane);
    dma_tile_pers(buf + TILE, p.d_o + (long)b * p.o_sb + h * DH, p.o_st, p.Tq, live, wave, lane);
  };
  // lse (log2 domain) and delta of row t = idx (thread-per-row, 2 slots per thread); needs p.delta from the dQ pass
  auto stats_load = [&](int hh, bool live, float (&lv)[2], float (&dv)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = (int)threadIdx.x + j * PERS_WAVES * 64;
      const bool ok = live && t < p.Tq;
      const long at = (long)hh * p.Tq + (ok ? t : 0);
      const float l = p.lse[ok ? at : 0], d = p.delta[ok ? at : 0];
      lv[j] = ok ? l * LOG2E : INFINITY;
      dv[j] = ok ? d : 0.f;
    }
  };
  auto stats_store = [&](char* buf, const float (&lv)[2], const float (&dv)[2]) {
    float* lse_s = reinterpret_cast<float*>(buf + 2 * TILE);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = (int)threadIdx.x + j * PERS_WAVES * 64;
      if (t < ROWS) {
        lse_s[t] = lv[j];
        lse_s[ROWS + t] = dv[j];
      }
    }
  };

  int hh = blockIdx.x;
  int cur = 0;
  {
    float lv[2], dv[2];
    issue(hh, smem, hh < heads);
    stats_load(hh, hh < heads, lv, dv);
    stats_store(smem, lv, dv);
  }
  lds_dma_wait_all();
  __syncthreads();
  for (; hh < heads; hh += gridDim.x) {
    const int b = hh / p.H, h = hh - b * p.H;
    char* Qs = smem + cur * BUF;
    char* dOs = Qs + TILE;
    const float* lse_s = reinterpret_cast<const float*>(Qs + 2 * TILE);
    const float* delta_s = lse_s + ROWS;
    const int row0 = wave * 16;
    const int kj = row0 + n;
    const bf16_t* kb = p.k + (long)b * p.kv_sb + h * DH;
    const bf16_t* vb = p.v + (long)b * p.kv_sb + h * DH;
    // this head's own fragments first: older than the DMA below in the vmcnt order
    const bf16x8 kf0 = frag_global(kb, p.kv_st, row0, p.Tk, 0, lane);
    const bf16x8 kf1 = frag_global(kb, p.kv_st, row0, p.Tk, 1, lane);
    const bf16x8 vf0 = frag_global(vb, p.kv_st, row0, p.Tk, 0, lane);
    const bf16x8 vf1 = frag_global(vb, p.kv_st, row0, p.Tk, 1, lane);
    const int nxt = hh + gridDim.x;
    float lv[2], dv[2];
    issue(nxt < heads ? nxt : hh, smem + (cur ^ 1) * BUF, nxt < heads);
    stats_load(nxt < heads ? nxt : hh, nxt < heads, lv, dv);

    f32x4 dkt[4], dvt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (row0 < p.Tk) {
      for (int a = 0; a < NBQ; ++a) {
        f32x4 pp[2], ds[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int it = 2 * a + t;
          const f32x4 sc = product64(Qs, it * 16, kf0, kf1, lane), dp = product64(dOs, it * 16, vf0, vf1, lane);
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + it * 16 + 4 * g);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_s + it * 16 + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = __builtin_amdgcn_exp2f(sc[r] * sl2 - l4[r]);
            pp[t][r] = pr;
            ds[t][r] = pr * (dp[r] - d4[r]);
          }
        }
        const bf16x8 ppk = pack8(pp[0], pp[1]);
        const bf16x8 dsk = pack8(ds[0], ds[1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(dOs, a * 32, dt * 16, lane), ppk, dvt[dt], 0, 0, 0);
          dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Qs, a * 32, dt * 16, lane), dsk, dkt[dt], 0, 0, 0);
        }
      }
    }
    {
      const bool valid = kj < p.Tk;
      store_row64(p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dkt, p.scale, g, valid);
      store_row64(p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dvt, 1.0f, g, valid);
    }
    stats_store(smem + (cur ^ 1) * BUF, lv, dv);
    lds_dma_wait_all();
    __syncthreads();  // the next head's operands have landed (vmcnt 0) and nobody reads this head's buffer any more
    cur ^= 1;
  }
}

// The forward in the persistent form (round 4; PLAIN only — the ViT path): wave w owns query rows 16 w .. 16 w + 15 of every
// head its workgroup visits, the next head's K / V stream into the second buffer.  The per-tile arithmetic is attn_fwd_kernel's
// (same instruction order: outputs and log-sum-exp are bit-identical).  Option "attn_persistent" bit 2.
template <int NB>
__global__ __launch_bounds__(PERS_WAVES * 64, 4) void attn_fwd_pers_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 256 * 128, BUF = 2 * TILE;
  static_assert(NB * 32 <= 256, "K / V of one head fit the 256-row tile slot");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int heads = p.B * p.H;
  const float sl2 = p.scale * LOG2E;
  auto issue = [&](int hh, char* buf, bool live) {
    const int b = hh / p.H, h = hh - b * p.H;
    dma_tile_pers(buf, p.k + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, live, wave, lane);
    dma_tile_pers(buf + TILE, p.v + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, live, wave, lane);
  };
  int hh = blockIdx.x;
  int cur = 0;
  issue(hh, smem, hh < heads);
  lds_dma_wait_all();
  __syncthreads();
  const int row0 = wave * 16;
  const int qi = row0 + i;
  // this wave's Q fragments: of the first head here, of every later head right behind the S products of the head before (their
  // global-memory latency used to sit in front of the first MFMA of every head)
  bf16x8 qf0 = {0, 0, 0, 0, 0, 0, 0, 0}, qf1 = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hh < heads) {
    const int b = hh / p.H, h = hh - b * p.H;
    const bf16_t* qb = p.q + (long)b * p.q_sb + h * DH;
    qf0 = frag_global(qb, p.q_st, row0, p.Tq, 0, lane);
    qf1 = frag_global(qb, p.q_st, row0, p.Tq, 1, lane);
  }
  for (; hh < heads; hh += gridDim.x) {
    const int b = hh / p.H, h = hh - b * p.H;
    const char* Ks = smem + cur * BUF;
    const char* Vs = Ks + TILE;
    const int nxt = hh + gridDim.x;
    issue(nxt < heads ? nxt : hh, smem + (cur ^ 1) * BUF, nxt < heads);
    if (row0 < p.Tq) {
      f32x4 st[2 * NB];
#pragma unroll
      for (int jt = 0; jt < 2 * NB; ++jt) {
        st[jt] = product64(Ks, jt * 16, qf0, qf1, lane);
        if (jt & 1) __builtin_amdgcn_sched_barrier(0);
      }
      if (nxt < heads) {
        const int bn = nxt / p.H, hn = nxt - bn * p.H;
        const bf16_t* qn = p.q + (long)bn * p.q_sb + hn * DH;
        qf0 = frag_global(qn, p.q_st, row0, p.Tq, 0, lane);
        qf1 = frag_global(qn, p.q_st, row0, p.Tq, 1, lane);
      }
#pragma unroll
      for (int jt = 2 * NB - 2; jt < 2 * NB; ++jt) {
        if (jt * 16 >= p.Tk) {
          st[jt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        } else if (jt * 16 + 15 >= p.Tk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) st[jt][r] = (jt * 16 + 4 * g + r < p.Tk) ? st[jt][r] : -INFINITY;
        }
      }
      float mx = -INFINITY, l;
      softmax_plain<NB>(st, sl2, mx, l);
      f32x4 ot[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        const bf16x8 pa = pack8(st[2 * a], st[2 * a + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Vs, a * 32, dt * 16, lane), pa, ot[dt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      const bool valid = qi < p.Tq;
      const float inv = 1.0f / l;
      store_row64(p.o + (long)b * p.o_sb + (long)qi * p.o_st + h * DH, ot, inv, g, valid);
      if (valid && g == 0 && p.lse != nullptr) p.lse[(long)hh * p.Tq + qi] = (mx + log2f(l)) * (1.0f / LOG2E);
    }
    lds_dma_wait_all();
    __syncthreads();
    cur ^= 1;
  }
}

// The dQ pass in the same persistent form (round 4): one 16-wave workgroup per CU walks (batch, head) pairs, wave w owns query
// rows 16 w .. 16 w + 15 of every head, K / V of the NEXT head stream into the second LDS buffer behind the current head's
// work.  In the round-4 stream plan the persistent dK / dV pass is worth 0.12 ms of the ViT step against the one-shot form
// (it was neutral in round 2); this is the dQ pass given the same treatment.  Option "attn_persistent" bit 1.
template <int NB>
__global__ __launch_bounds__(PERS_WAVES * 64, 4) void attn_bwd_dq_pers_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 256 * 128, BUF = 2 * TILE;  // K tile + V tile, 256-row slots (rows beyond Tk are zero)
  static_assert(NB * 32 <= 256, "K / V of one head fit the 256-row tile slot");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int heads = p.B * p.H;
  const float sl2 = p.scale * LOG2E;

  auto issue = [&](int hh, char* buf, bool live) {
    const int b = hh / p.H, h = hh - b * p.H;
    dma_tile_pers(buf, p.k + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, live, wave, lane);
    dma_tile_pers(buf + TILE, p.v + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, live, wave, lane);
  };

  int hh = blockIdx.x;
  int cur = 0;
  issue(hh, smem, hh < heads);
  lds_dma_wait_all();
  __syncthreads();
  const int row0 = wave * 16;
  const int qi = row0 + i;
  const bool qvalid = qi < p.Tq;
  for (; hh < heads; hh += gridDim.x) {
    const int b = hh / p.H, h = hh - b * p.H;
    const char* Ks = smem + cur * BUF;
    const char* Vs = Ks + TILE;
    const bf16_t* qb = p.q + (long)b * p.q_sb + h * DH;
    const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * DH;
    const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * DH;
    // this head's own fragments first: older than the DMA below in the vmcnt order
    const bf16x8 qf0 = frag_global(qb, p.q_st, row0, p.Tq, 0, lane);
    const bf16x8 qf1 = frag_global(qb, p.q_st, row0, p.Tq, 1, lane);
    const bf16x8 dof0 = frag_global(dob, p.o_st, row0, p.Tq, 0, lane);
    const bf16x8 dof1 = frag_global(dob, p.o_st, row0, p.Tq, 1, lane);
    const bf16x8 of0 = frag_global(ob, p.o_st, row0, p.Tq, 0, lane);
    const bf16x8 of1 = frag_global(ob, p.o_st, row0, p.Tq, 1, lane);
    const long stat = (long)hh * p.Tq + (qvalid ? qi : 0);
    const float lse_raw = p.lse[stat];
    const int nxt = hh + gridDim.x;
    issue(nxt < heads ? nxt : hh, smem + (cur ^ 1) * BUF, nxt < heads);

    const float delta = row_delta(dof0, dof1, of0, of1);
    if (qvalid && g == 0) p.delta[stat] = delta;
    const float lse2 = qvalid ? lse_raw * LOG2E : INFINITY;  // +inf -> p = 0 for padded rows

    f32x4 dqt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dqt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row0 < p.Tq) {
      for (int a = 0; a < NB; ++a) {
        const bf16x8 dsp = dq_ds<true>(Ks, Vs, a, qf0, qf1, dof0, dof1, sl2, lse2, delta, p, b, h, qi, lane);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dqt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Ks, a * 32, dt * 16, lane), dsp, dqt[dt], 0, 0, 0);
      }
    }
    store_row64(p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * DH, dqt, p.scale, g, qvalid);
    lds_dma_wait_all();
    __syncthreads();  // the next head's K / V have landed (vmcnt 0) and nobody reads this head's buffer any more
    cur ^= 1;
  }
}

// waves per workgroup: ONE workgroup per (batch, head) (the resident K / V — or Q / dO — tiles are
// loaded once), its waves walk the 16-row tiles in rounds; pick the wave count that leaves the
// fewest idle slots in the last round (at most 8 waves).
inline int pick_waves(int T) {
  const int tiles = (T + 15) / 16;
  const int rounds = (tiles + 7) / 8;
  return (tiles + rounds - 1) / rounds;
}

}  // namespace

int cfhip_attn::launch_resident(const Step& st, const AttnParams& p, int pers_ctas, hipStream_t s) {
  const int heads = p.B * p.H;
  const dim3 per_head(1, p.H, p.B);                                       // one workgroup per (batch, head)
  const dim3 persistent(heads < pers_ctas ? heads : pers_ctas);  // workgroups walking the heads
  const size_t pers_lds = (size_t)2 * 2 * 256 * 128;  // two buffers of 256 K and V rows
  switch (st.family) {
    case FWD:
      return with_args<1, 2, 3, 4, 5, 6, 7, 8>(st, "attn_fwd", [&](auto NB, auto PLAIN, auto) {
        return launch<attn_fwd_kernel<NB(), PLAIN()>>(per_head, pick_waves(p.Tq) * 64, (size_t)2 * NB() * 32 * 128, s, "attn_fwd", p);
      });
    case FWD_PERS:
      return with_args<5, 6, 7, 8>(st, "attn_fwd", [&](auto NB, auto, auto) {
        return launch<attn_fwd_pers_kernel<NB()>>(persistent, PERS_WAVES * 64, pers_lds, s, "attn_fwd(persistent)", p);
      });
    case DQ: {
      const size_t lds = (size_t)2 * st.n * 32 * 128;
      return st.plain ? launch<attn_bwd_dq_kernel<true>>(per_head, pick_waves(p.Tq) * 64, lds, s, "attn_bwd_dq", p, st.n)
                      : launch<attn_bwd_dq_kernel<false>>(per_head, pick_waves(p.Tq) * 64, lds, s, "attn_bwd_dq", p, st.n);
    }
    case DQ_PERS:
      return with_args<5, 6, 7, 8>(st, "attn_bwd", [&](auto NB, auto, auto) {
        return launch<attn_bwd_dq_pers_kernel<NB()>>(persistent, PERS_WAVES * 64, pers_lds, s, "attn_bwd_dq(persistent)", p);
      });
    case DKV: {
      const size_t lds = (size_t)2 * st.n * 32 * 128 + (size_t)2 * st.n * 32 * sizeof(float);
      return st.plain ? launch<attn_bwd_dkv_kernel<true>>(per_head, pick_waves(p.Tk) * 64, lds, s, "attn_bwd_dkv", p, st.n)
                      : launch<attn_bwd_dkv_kernel<false>>(per_head, pick_waves(p.Tk) * 64, lds, s, "attn_bwd_dkv", p, st.n);
    }
    case DKV_PERS:
      return with_args<5, 6, 7, 8>(st, "attn_bwd", [&](auto NBQ, auto, auto) {
        return launch<attn_bwd_dkv_pers_kernel<NBQ()>>(persistent, PERS_WAVES * 64, 2 * ((size_t)2 * 256 * 128 + (size_t)2 * NBQ() * 32 * sizeof(float)),
                                                       s, "attn_bwd_dkv(persistent)", p);
      });
    default:
      return no_kernel(st);
  }
}
