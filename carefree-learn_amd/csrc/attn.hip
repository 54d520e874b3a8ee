// Fused scaled-dot-product attention (forward + backward) for gfx950: the options, the plan of a call, the launch of its steps
// and the C ABI, and the kernels that stage their operands chunk by chunk: the general forms (any length, head_dim up to 192, dropout)
// and the two-tiles-per-wave forms for long sequences.  The kernels that keep a head resident in LDS live in their own files, each
// behind one launcher (csrc/attn_host.h):
//   attn_resident.hip   head_dim 64, T <= 256, K / V (or Q / dO) of a head resident in LDS: one-shot and persistent forms
//   attn_one_pass.hip   dQ, dK and dV of a short self-attention from one evaluation of S and dP
// All share csrc/attn_device.h.  The general and the long-sequence kernels stay in ONE translation unit: hipcc takes the value ranges
// of a shared inline helper's arguments (frag_cols, ...) over every caller of a translation unit, and compiled apart 22 of their
// forward instantiations change registers and two start to spill (profiles/r14/attn_split_isa.txt).
#include "common.h"
#include "attn_device.h"
#include "attn_host.h"
#include <math.h>

using namespace cfhip_attn;

namespace {

// Timing ablations exist only in -DCFHIP_ABLATE builds (tools/build_variant.sh); the product library has none.
#ifdef CFHIP_ABLATE
int g_attn_ablate = 0;
#endif

// ------------------------------------------------------------------------------------------------
// General form: any sequence length, head_dim = any multiple of 8 up to 192 (UNet cross-attention heads of 40 / 80 /
// 160 channels, convs / mixed_stacks/api.py:766-893).  The same three kernels with (1) an outer loop over CHUNKS of
// the operand that the short form keeps resident in LDS and (2) the head dimension handled as NH = ceil(dh / 64)
// zero-padded 64-column HALVES, each an ordinary swizzled [rows][64] tile (columns >= dh are range-checked to zero
// by the DMA / never loaded into fragments / never stored).  Workgroup = (128-row chunk of the walking operand,
// head, batch), one 16-row tile per wave.  Forward: online softmax across chunks (running max m, sum l, rescaled O);
// backward: p = exp2(s * scale - lse) with the saved lse, so chunks just accumulate.  The chunked operand is re-read
// once per 128-row workgroup, from L2.
// ------------------------------------------------------------------------------------------------
// (DROP: the Philox state and the keep bytes need registers beyond the 128 of four waves per SIMD — two per SIMD, no scratch)
template <int NH, bool PLAIN, bool DROP = false>
__global__ __launch_bounds__(512, (NH == 1 && !DROP) ? 4 : 2) void attn_gen_fwd_kernel(AttnParams p) {
  using G = Gen<NH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + G::OPER_BYTES;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * dh;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * dh;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * dh;
  const int row0 = (blockIdx.x * nwaves + wave) * 16;
  const bool active = row0 < p.Tq;  // inactive waves still stage and hit the barriers
  const int qi = row0 + i;
  bf16x8 qf[2 * NH];
#pragma unroll
  for (int ks = 0; ks < 2 * NH; ++ks) qf[ks] = frag_global_dh(qb, p.q_st, row0, active ? p.Tq : 0, ks, lane, dh);
  const float sl2 = p.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x4 ot[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int k0, char* slot) {
    const int rows_ = min(G::CH, p.Tk - k0);
    int ln = lane;  // opaque copy: the per-lane DMA offsets are recomputed per chunk (a few VALU) instead of being hoisted out
    asm volatile("" : "+v"(ln));  // of the chunk loop and spilled around it
    dma_oper<NH>(slot, kb + (long)k0 * p.kv_st, p.kv_st, rows_, dh, wave, nwaves, ln);
    dma_oper<NH>(slot + G::OPER_BYTES, vb + (long)k0 * p.kv_st, p.kv_st, rows_, dh, wave, nwaves, ln);
  };
  if (G::NSLOT == 2) issue(0, smem);
  for (int kv0 = 0, c = 0; kv0 < p.Tk; kv0 += G::CH, ++c) {
    if (G::NSLOT == 2) {
      lds_dma_wait_all();
      __syncthreads();  // chunk c has landed everywhere; every wave is done with chunk c - 1 (the other slot)
      if (kv0 + G::CH < p.Tk) issue(kv0 + G::CH, smem + ((c + 1) & 1) * G::SLOT_BYTES);
      Ks = smem + (c & 1) * G::SLOT_BYTES;
      Vs = Ks + G::OPER_BYTES;
    } else {
      __syncthreads();  // every wave is done with the previous chunk
      issue(kv0, smem);
      lds_dma_wait_all();
      __syncthreads();
    }
    if (!active) continue;
    if (p.causal && kv0 > row0 + 15) continue;  // chunk entirely in the future of this tile (wave-uniform)
    f32x4 st[2 * G::CHB];
#pragma unroll
    for (int jt = 0; jt < 2 * G::CHB; ++jt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2 * NH; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(Ks + (ks >> 1) * G::HALF_BYTES, jt * 16, ks & 1, lane),
                                                      qf[ks], acc, 0, 0, 0);
      st[jt] = acc;
      if (jt & 1) __builtin_amdgcn_sched_barrier(0);
    }
    float mx = -INFINITY;
    const bool tail = kv0 + G::CH > p.Tk;  // wave-uniform: only the last chunk needs the j < Tk test
#pragma unroll
    for (int jt = 0; jt < 2 * G::CHB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kv0 + jt * 16 + 4 * g + r;
        float x = st[jt][r] * sl2;
        if (PLAIN) {
          if (tail) x = j < p.Tk ? x : -INFINITY;
        } else {
          x = keep_at(p, b, h, qi < p.Tq ? qi : p.Tq - 1, j) ? x : -INFINITY;
        }
        st[jt][r] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = group_max(mx);
    const float m_new = fmaxf(m, mx);
    // rows whose every position so far is masked (m_new = -inf) must not produce NaN from (-inf) - (-inf): use 0
    // as the reference point for them (all their terms are exp2(-inf) = 0 anyway); no divergent branch around MFMAs
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_use);  // m = -inf on the first chunk: 0
    float ls = 0.f;
#pragma unroll
    for (int jt = 0; jt < 2 * G::CHB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(st[jt][r] - m_use);
        st[jt][r] = e;
        ls += e;
      }
    }
    l = l * alpha + group_sum(ls);
    m = m_new;
    if (DROP) {  // the row sum above is the softmax denominator: dropout acts on the normalised probabilities
#pragma unroll
      for (int jt = 0; jt < 2 * G::CHB; ++jt) {
        const unsigned w = pick_word(drop_block(p, b, h, qi >> 2, (kv0 >> 2) + jt * 4 + g), qi);
#pragma unroll
        for (int r = 0; r < 4; ++r) st[jt][r] = ((w >> (8 * r)) & 255u) >= p.drop_thresh ? st[jt][r] : 0.f;
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) ot[dt] *= alpha;
#pragma unroll
    for (int a = 0; a < G::CHB; ++a) {
      const bf16x8 pa = pack8(st[2 * a], st[2 * a + 1]);
#pragma unroll
      for (int dt = 0; dt < 4 * NH; ++dt)
        ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            frag_cols(Vs + (dt >> 2) * G::HALF_BYTES, a * 32, (dt & 3) * 16, lane), pa, ot[dt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (active && qi < p.Tq) {
    const float inv = (DROP ? p.drop_scale : 1.0f) / l;
    bf16_t* orow = p.o + (long)b * p.o_sb + (long)qi * p.o_st + h * dh;
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) {
      const int col = dt * 16 + 4 * g;
      if (col >= dh) continue;  // dh % 8 == 0: a 4-column group is entirely inside or outside
      const f32x4 v = ot[dt] * inv;
      *reinterpret_cast<u32x2*>(orow + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    }
    if (g == 0 && p.lse != nullptr) p.lse[((long)b * p.H + h) * p.Tq + qi] = (m + log2f(l)) * (1.0f / LOG2E);
  }
}

template <int NH, bool PLAIN, bool DROP = false>
__global__ __launch_bounds__(512, NH == 1 ? 4 : 2) void attn_gen_bwd_dq_kernel(AttnParams p) {
  using G = Gen<NH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + G::OPER_BYTES;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const int row0 = (blockIdx.x * nwaves + wave) * 16;
  const bool active = row0 < p.Tq;
  const int qi = row0 + i;
  const bool qvalid = active && qi < p.Tq;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * dh;
  const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * dh;
  const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * dh;
  bf16x8 qf[2 * NH], dof[2 * NH];
  float sacc = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2 * NH; ++ks) {
    qf[ks] = frag_global_dh(qb, p.q_st, row0, active ? p.Tq : 0, ks, lane, dh);
    dof[ks] = frag_global_dh(dob, p.o_st, row0, active ? p.Tq : 0, ks, lane, dh);
    const bf16x8 of = frag_global_dh(ob, p.o_st, row0, active ? p.Tq : 0, ks, lane, dh);
#pragma unroll
    for (int e = 0; e < 8; ++e) sacc += bf16_to_f32((bf16_t)dof[ks][e]) * bf16_to_f32((bf16_t)of[e]);
  }
  const float delta = PLAIN ? group_sum(sacc) : finite_or_zero(group_sum(sacc));
  const long stat = ((long)b * p.H + h) * p.Tq + qi;
  if (qvalid && g == 0) p.delta[stat] = delta;
  const float lse2 = qvalid ? p.lse[stat] * LOG2E : INFINITY;
  const float sl2 = p.scale * LOG2E;
  f32x4 dqt[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) dqt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int k0, char* slot) {
    const int rows_ = min(G::CH, p.Tk - k0);
    int ln = lane;  // opaque copy: the per-lane DMA offsets are recomputed per chunk (a few VALU) instead of being hoisted out
    asm volatile("" : "+v"(ln));  // of the chunk loop and spilled around it
    dma_oper<NH>(slot, p.k + (long)b * p.kv_sb + (long)k0 * p.kv_st + h * dh, p.kv_st, rows_, dh, wave, nwaves, ln);
    dma_oper<NH>(slot + G::OPER_BYTES, p.v + (long)b * p.kv_sb + (long)k0 * p.kv_st + h * dh, p.kv_st, rows_, dh, wave, nwaves, ln);
  };
  if (G::NSLOT == 2) issue(0, smem);
  for (int kv0 = 0, c = 0; kv0 < p.Tk; kv0 += G::CH, ++c) {
    const int rows = min(G::CH, p.Tk - kv0);
    if (G::NSLOT == 2) {
      lds_dma_wait_all();
      __syncthreads();  // chunk c has landed everywhere; every wave is done with chunk c - 1 (the other slot)
      if (kv0 + G::CH < p.Tk) issue(kv0 + G::CH, smem + ((c + 1) & 1) * G::SLOT_BYTES);
      Ks = smem + (c & 1) * G::SLOT_BYTES;
      Vs = Ks + G::OPER_BYTES;
    } else {
      __syncthreads();
      issue(kv0, smem);
      lds_dma_wait_all();
      __syncthreads();
    }
    if (!active) continue;
    if (p.causal && kv0 > row0 + 15) continue;
    const int nbl = (rows + 31) / 32;
    for (int a = 0; a < nbl; ++a) {
      f32x4 ds[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int jt = 2 * a + t;
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2 * NH; ++ks) {
          sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(Ks + (ks >> 1) * G::HALF_BYTES, jt * 16, ks & 1, lane),
                                                       qf[ks], sc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(Vs + (ks >> 1) * G::HALF_BYTES, jt * 16, ks & 1, lane),
                                                       dof[ks], dp, 0, 0, 0);
        }
        unsigned w = 0u;
        if (DROP) w = pick_word(drop_block(p, b, h, qi >> 2, (kv0 >> 2) + jt * 4 + g), qi);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pr = __builtin_amdgcn_exp2f(sc[r] * sl2 - lse2);
          if (!PLAIN) pr = keep_at(p, b, h, qvalid ? qi : p.Tq - 1, kv0 + jt * 16 + 4 * g + r) ? pr : 0.f;
          float dpr = dp[r];  // d loss / d (dropped probability)
          if (DROP) dpr = ((w >> (8 * r)) & 255u) >= p.drop_thresh ? dpr * p.drop_scale : 0.f;
          ds[t][r] = pr * (dpr - delta);
        }
      }
      const bf16x8 dsp = pack8(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 4 * NH; ++dt) {
        dqt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            frag_cols(Ks + (dt >> 2) * G::HALF_BYTES, a * 32, (dt & 3) * 16, lane), dsp, dqt[dt], 0, 0, 0);
      }
    }
  }
  if (qvalid) {
    bf16_t* dqrow = p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * dh;
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) {
      const int col = dt * 16 + 4 * g;
      if (col >= dh) continue;
      const f32x4 v = dqt[dt] * p.scale;
      *reinterpret_cast<u32x2*>(dqrow + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    }
  }
}

template <int NH, bool PLAIN, bool DROP = false>
__global__ __launch_bounds__(512, NH == 1 ? 4 : 2) void attn_gen_bwd_dkv_kernel(AttnParams p) {
  using G = Gen<NH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = smem + G::OPER_BYTES;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * G::OPER_BYTES);
  float* delta_s = lse_s + G::CH;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = blockDim.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const int row0 = (blockIdx.x * nwaves + wave) * 16;
  const bool active = row0 < p.Tk;
  const int kj = row0 + n;
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * dh;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * dh;
  bf16x8 kf[2 * NH], vf[2 * NH];
#pragma unroll
  for (int ks = 0; ks < 2 * NH; ++ks) {
    kf[ks] = frag_global_dh(kb, p.kv_st, row0, active ? p.Tk : 0, ks, lane, dh);
    vf[ks] = frag_global_dh(vb, p.kv_st, row0, active ? p.Tk : 0, ks, lane, dh);
  }
  const float sl2 = p.scale * LOG2E;
  f32x4 dkt[4 * NH], dvt[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int dslots = dh / 8;  // 16-byte slots of one row of dO / O

  // lse (log2 domain) and delta_i = sum_d dO[i][d] * O[i][d] of a chunk's rows: thread t of the first CH threads owns row t
  auto stats_load = [&](int q0_, float& lv, float& dv) {
    const int t = threadIdx.x;
    lv = INFINITY;
    dv = 0.f;
    if (t >= G::CH) return;
    const int tq = q0_ + t;
    if (tq >= p.Tq) return;
    if (G::NSLOT == 2 || p.delta_ready) {  // (the two-slot launches always find delta filled: attn_delta_kernel)
      dv = p.delta[((long)b * p.H + h) * p.Tq + tq];
    } else {
      const bf16_t* dor = p.d_o + (long)b * p.o_sb + (long)tq * p.o_st + h * dh;
      const bf16_t* orr = p.o_in + (long)b * p.o_sb + (long)tq * p.o_st + h * dh;
      for (int sl = 0; sl < dslots; ++sl) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(dor + sl * 8);
        const u32x4 c = *reinterpret_cast<const u32x4*>(orr + sl * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) dv += bf16lo(a[e]) * bf16lo(c[e]) + bf16hi(a[e]) * bf16hi(c[e]);
      }
    }
    if (!PLAIN) dv = finite_or_zero(dv);
    lv = p.lse[((long)b * p.H + h) * p.Tq + tq] * LOG2E;
  };
  auto stats_store = [&](char* slot, float lv, float dv) {
    if ((int)threadIdx.x < G::CH) {
      float* ls = reinterpret_cast<float*>(slot + G::SLOT_BYTES);
      ls[threadIdx.x] = lv;
      ls[G::CH + threadIdx.x] = dv;
    }
  };
  auto issue = [&](int q0_, char* slot) {
    const int rows_ = min(G::CH, p.Tq - q0_);
    int ln = lane;  // opaque copy: see attn_gen_fwd_kernel
    asm volatile("" : "+v"(ln));
    dma_oper<NH>(slot, p.q + (long)b * p.q_sb + (long)q0_ * p.q_st + h * dh, p.q_st, rows_, dh, wave, nwaves, ln);
    dma_oper<NH>(slot + G::OPER_BYTES, p.d_o + (long)b * p.o_sb + (long)q0_ * p.o_st + h * dh, p.o_st, rows_, dh, wave, nwaves, ln);
  };
  constexpr int RING = G::SLOT_BYTES + 2 * G::CH * (int)sizeof(float);  // operands + statistics of one chunk
  float nlv = INFINITY, ndv = 0.f;  // statistics of the NEXT chunk: loaded before this chunk's MFMAs, stored after them
  if (G::NSLOT == 2) {
    stats_load(0, nlv, ndv);
    issue(0, smem);
    stats_store(smem, nlv, ndv);
  }
  for (int q0 = 0, c = 0; q0 < p.Tq; q0 += G::CH, ++c) {
    const int rows = min(G::CH, p.Tq - q0);
    const bool more = q0 + G::CH < p.Tq;
    if (G::NSLOT == 2) {
      lds_dma_wait_all();
      __syncthreads();  // chunk c (operands and statistics) is visible; every wave is done with chunk c - 1 (the other slot)
      if (more) {
        stats_load(q0 + G::CH, nlv, ndv);  // (issued BEFORE the DMA: the compiler's wait for these loads at the store below
        issue(q0 + G::CH, smem + ((c + 1) & 1) * RING);  //  comes after this chunk's MFMAs, when the DMA has landed anyway)
      }
    } else {
      __syncthreads();
      issue(q0, smem);
      stats_load(q0, nlv, ndv);
      stats_store(smem, nlv, ndv);
      lds_dma_wait_all();
      __syncthreads();
    }
    const bool skip = !active || (p.causal && q0 + G::CH - 1 < row0);  // inactive tile / every query of the chunk precedes it
    if (skip) {
      if (G::NSLOT == 2 && more) stats_store(smem + ((c + 1) & 1) * RING, nlv, ndv);
      continue;
    }
    // the chunk's MFMA work, once per ring slot with COMPILE-TIME LDS addresses (a run-time slot base costs an address
    // register per fragment read: the 128-register budget of two workgroups per CU does not have them)
    auto body = [&](auto slot_tag) {
      constexpr int S = decltype(slot_tag)::value;
      const char* Qs_ = smem + S * RING;
      const char* dOs_ = Qs_ + G::OPER_BYTES;
      const float* lse_ = reinterpret_cast<const float*>(Qs_ + G::SLOT_BYTES);
      const float* delta_ = lse_ + G::CH;
      const int nbl = (rows + 31) / 32;
#pragma unroll 1
      for (int a = 0; a < nbl; ++a) {
        f32x4 pp[2], ds[2];
  #pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int it = 2 * a + t;
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
          for (int ks = 0; ks < 2 * NH; ++ks) {
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(Qs_ + (ks >> 1) * G::HALF_BYTES, it * 16, ks & 1, lane),
                                                         kf[ks], sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(dOs_ + (ks >> 1) * G::HALF_BYTES, it * 16, ks & 1, lane),
                                                         vf[ks], dp, 0, 0, 0);
          }
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_ + it * 16 + 4 * g);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_ + it * 16 + 4 * g);
          Philox rb = {{0u, 0u, 0u, 0u}};
          if (DROP) rb = drop_block(p, b, h, (q0 >> 2) + it * 4 + g, kj >> 2);  // rows 4g .. 4g + 3 = words 0 .. 3
  #pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = __builtin_amdgcn_exp2f(sc[r] * sl2 - l4[r]);
            if (!PLAIN) {
              const int qi = q0 + it * 16 + 4 * g + r;
              pr = (qi < p.Tq && keep_at(p, b, h, qi, kj)) ? pr : 0.f;
            }
            float keep_scale = 1.0f;
            if (DROP) keep_scale = ((rb.c[r] >> (8 * (kj & 3))) & 255u) >= p.drop_thresh ? p.drop_scale : 0.f;
            pp[t][r] = pr * keep_scale;
            ds[t][r] = pr * (dp[r] * keep_scale - d4[r]);
          }
        }
        const bf16x8 ppk = pack8(pp[0], pp[1]);
        const bf16x8 dsk = pack8(ds[0], ds[1]);
  #pragma unroll
        for (int dt = 0; dt < 4 * NH; ++dt) {
          dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              frag_cols(dOs_ + (dt >> 2) * G::HALF_BYTES, a * 32, (dt & 3) * 16, lane), ppk, dvt[dt], 0, 0, 0);
          dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              frag_cols(Qs_ + (dt >> 2) * G::HALF_BYTES, a * 32, (dt & 3) * 16, lane), dsk, dkt[dt], 0, 0, 0);
        }
      }
    };
    if (G::NSLOT == 2 && (c & 1)) body(std::integral_constant<int, 1>{});
    else body(std::integral_constant<int, 0>{});
    if (G::NSLOT == 2 && more) stats_store(smem + ((c + 1) & 1) * RING, nlv, ndv);
  }
  if (active && kj < p.Tk) {
    bf16_t* dkrow = p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * dh;
    bf16_t* dvrow = p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * dh;
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) {
      const int col = dt * 16 + 4 * g;
      if (col >= dh) continue;
      const f32x4 kk = dkt[dt] * p.scale;
      const f32x4 vv = dvt[dt];
      *reinterpret_cast<u32x2*>(dkrow + col) = u32x2{pack_bf16x2(kk[0], kk[1]), pack_bf16x2(kk[2], kk[3])};
      *reinterpret_cast<u32x2*>(dvrow + col) = u32x2{pack_bf16x2(vv[0], vv[1]), pack_bf16x2(vv[2], vv[3])};
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Round 3, head_dim <= 64 without dropout: TWO 16-row tiles per wave.
// In the kernels above every wave reads the WHOLE staged chunk from LDS for its 16 rows: per 256-key chunk 32 ds_read_b128
// + 64 ds_read_b64_tr_b16 per wave = 256 LDS cycles, sixteen waves per CU = 4096 — exactly the matrix time of the chunk
// (64 MFMAs x 16 cycles x 4 waves per SIMD): LDS bandwidth and the matrix pipe are co-bottlenecks and neither gets above
// half.  Here a wave owns 32 query rows (forward, dQ) / 32 key rows (dK, dV): every K / V (Q / dO) fragment read from LDS
// feeds two MFMAs, a workgroup covers 256 rows per staged chunk instead of 128 (half the L2 -> LDS bytes per FLOP), and
// the two tiles are independent dependency chains inside the wave.  Scores live in registers for 64 keys at a time (32
// registers for both tiles; the 256-key form would need 128), online softmax per 64-key block; the row sum is kept per
// lane and folded across the four lanes of a row once, at the end.  Output columns beyond head_dim are not computed:
// NDT = 3 column tiles for head_dim <= 48 (the UNet's 40-channel heads), 4 otherwise.
// ------------------------------------------------------------------------------------------------
// Tried and NOT kept: columns 32 .. 47 of a head_dim <= 48 product through ONE v_mfma_f32_16x16x16_bf16 instead of the second,
// three-quarters-empty 16x16x32.  hipcc schedules the 16-deep MFMA directly behind the 32-deep one whose result it accumulates
// onto, with a DIFFERENT destination register and no wait states; the results are wrong (tools/micro/mfma_chain.hip shows the
// in-place chain is fine, tools/micro/mfma16_layout.hip that the operand layout is what one expects).  The gain would have been
// 2-5 % on the backward passes and nothing on the VALU-bound forward; a hand-padded chain is not worth a silent-corruption risk.
constexpr int A2_ROWS = 256;   // rows of the walking operand per workgroup (8 waves x 32)
constexpr int A2_CH = 256;     // rows of the staged operand per chunk (64 KB: K + V, or Q + dO)
constexpr int A2_TILE = A2_CH * 128;

// SUMCOL (head_dim = 8 mod 16, e.g. the UNet's 40: the last column tile has free columns): the softmax row sum comes out of
// the matrix pipe.  Column dh of the staged V tile is a column of ONES (written once: the chunk DMAs skip the pad columns,
// dma_half<SKIP_PAD>), so O[:, dh] = sum_j p_ij accumulates — and is rescaled by alpha — with the output it normalises,
// and the 32 adds per 64-key block (16 v_pk_add_f32 per wave in a VALU-bound loop: 163 VALU per 28 MFMAs) disappear.  The sum
// is then that of the bf16-rounded probabilities, i.e. of exactly what multiplied V.
// Both forms skip the rescale of O when no row of the wave raised its running maximum in this block (alpha == 1 for all 32
// rows — the common case after the first few blocks of a long sequence): a wave-uniform branch around 12-16 v_pk_mul_f32.
#ifndef CFHIP_ATTN_NDT4_WAVES
#define CFHIP_ATTN_NDT4_WAVES 4  // waves per SIMD of the head_dim-64 (NDT = 4) long-sequence forms: 4 keeps 12-36 B of scratch, 3 has none (A/B: profiles/r05)
#endif
// NDT = 5 / 6 (head_dim 72 .. 96: the UNet's 80-channel heads; round 6, late): the same loop over KS = 3 reduction steps and two
// 64-column halves of the staged K / V — as attn_bwd_dkv2_kernel does it: 4 waves, 128-key chunks (64 KB of LDS), two workgroups per CU
// at 256 registers.  The one-tile general kernel ran this head_dim's forward at 527 TFLOP/s against 1 020 for its dK / dV pass.
template <int NDT>
struct Fwd2 {
  static constexpr int NH = (NDT + 3) / 4;  // 64-column halves of a staged operand
  static constexpr int KS = (NDT + 1) / 2;  // 32-deep steps of the reduction over head_dim
  static constexpr int NW = NH == 1 ? 8 : 4;
  static constexpr int CH = Gen<NH>::CH;    // keys per staged chunk: 256 / 128
  static constexpr int HB = Gen<NH>::HALF_BYTES;
  static constexpr int WAVES_PER_SIMD = NH == 1 ? (NDT == 4 ? CFHIP_ATTN_NDT4_WAVES : 4) : 2;
};
template <bool PLAIN, int NDT, bool SUMCOL = false>
__global__ __launch_bounds__(Fwd2<NDT>::NW * 64, Fwd2<NDT>::WAVES_PER_SIMD) void attn_fwd2_kernel(AttnParams p) {
  using F = Fwd2<NDT>;
  constexpr int NH = F::NH, KS = F::KS, NW = F::NW, CH = F::CH, HB = F::HB;
  static_assert(!SUMCOL || NH == 1, "the ones column: single-half forms only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + NH * HB;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  if (SUMCOL) {
    // pad chunks of both tiles, once: zeros, and 1.0 in column dh of V (dh % 16 == 8: element 0 of its 16-byte chunk)
    for (int idx = threadIdx.x; idx < CH * 8; idx += NW * 64) {
      const int row = idx >> 3, chunk = idx & 7;
      if (chunk * 8 >= dh) {
        const int off = row * 128 + ((chunk ^ swz(row)) << 4);
        *reinterpret_cast<u32x4*>(Ks + off) = u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(Vs + off) = u32x4{chunk * 8 == dh ? 0x3F80u : 0u, 0u, 0u, 0u};
      }
    }
  }
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * dh;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * dh;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * dh;
  const int row0 = (blockIdx.x * NW + wave) * 32;
  const bool active = row0 < p.Tq;  // inactive waves still stage and hit the barriers
  bf16x8 qf[2][KS];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[t][ks] = frag_global_dh(qb, p.q_st, row0 + 16 * t, active ? p.Tq : 0, ks, lane, dh);
  const float sl2 = p.scale * LOG2E;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};  // l: this LANE's share of the row sum
  f32x4 ot[2][NDT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) ot[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kv0 = 0; kv0 < p.Tk; kv0 += CH) {
    const int rows = min(CH, p.Tk - kv0);
    __syncthreads();  // every wave is done with the previous chunk
    {
      int ln = lane;  // opaque copy: the per-lane DMA offsets are recomputed per chunk instead of hoisted and spilled
      asm volatile("" : "+v"(ln));
      dma_oper<NH, SUMCOL>(Ks, kb + (long)kv0 * p.kv_st, p.kv_st, rows, dh, wave, NW, ln);
      dma_oper<NH, SUMCOL>(Vs, vb + (long)kv0 * p.kv_st, p.kv_st, rows, dh, wave, NW, ln);
    }
    lds_dma_wait_all();
    __syncthreads();
    if (!active) continue;
    if (p.causal && kv0 > row0 + 31) continue;  // chunk entirely in the future of both tiles (wave-uniform)
    const int nsb = (rows + 63) >> 6;
#pragma unroll 1
    for (int sb = 0; sb < nsb; ++sb) {
      const int k0 = sb * 64;
      if (p.causal && kv0 + k0 > row0 + 31) break;
      f32x4 st[2][4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        bf16x8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = frag_rows(Ks + (ks >> 1) * HB, k0 + jt * 16, ks & 1, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[t][ks], acc, 0, 0, 0);
          st[t][jt] = acc;
        }
      }
      // Key positions >= Tk (zero rows of the staged chunk) exist only in the last 64-key block of a sequence whose length
      // is not a multiple of 64: a REAL wave-uniform branch around a masking pass.  Written as `if (tail) x = j < Tk ? x :
      // -inf` inside the softmax loop, hipcc if-converted the test into two v_cndmask + index arithmetic for every score of
      // every block: 104 of the loop's ~250 VALU instructions, in a kernel that is VALU-bound (10.9 VALU per MFMA:
      // profiles/r03/pmc_attn_fwd2_first.txt); an empty asm inside the branch was not enough either (the selects were
      // hoisted above it), the compared bound has to be opaque.
      if (PLAIN && kv0 + k0 + 64 > p.Tk) {
        int lim = p.Tk - (kv0 + k0);    // valid keys of this block
        asm volatile("" : "+s"(lim));  // opaque and produced INSIDE the branch: the selects cannot be hoisted above it
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              st[t][jt][r] = jt * 16 + 4 * g + r < lim ? st[t][jt][r] : -INFINITY;
      }
      float alpha[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qi = row0 + 16 * t + i;
        float mx = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = st[t][jt][r];  // raw score: the scale is folded into the exponent below (scale > 0)
            if (!PLAIN) {
              x = keep_at(p, b, h, qi < p.Tq ? qi : p.Tq - 1, kv0 + k0 + jt * 16 + 4 * g + r) ? x : -INFINITY;
              st[t][jt][r] = x;
            }
            mx = fmaxf(mx, x);
          }
        }
        mx = group_max_swap(mx) * sl2;
        const float m_new = max_nn(m[t], mx);
        // rows whose every position so far is masked (m_new = -inf) must not produce NaN from (-inf) - (-inf): use 0
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        alpha[t] = __builtin_amdgcn_exp2f(m[t] - m_use);  // m = -inf on the first block: 0; unchanged maximum: exactly 1
        float ls = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(st[t][jt][r], sl2, -m_use));
            st[t][jt][r] = e;
            if (!SUMCOL) ls += e;
          }
        }
        if (!SUMCOL) l[t] = l[t] * alpha[t] + ls;
        m[t] = m_new;
      }
      if (__builtin_amdgcn_ballot_w64(alpha[0] != 1.f || alpha[1] != 1.f) != 0) {  // wave-uniform
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) ot[t][dt] *= alpha[t];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const bf16x8 pa0 = pack8(st[0][2 * a], st[0][2 * a + 1]);
        const bf16x8 pa1 = pack8(st[1][2 * a], st[1][2 * a + 1]);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const bf16x8 vf = frag_cols(Vs + (dt >> 2) * HB, k0 + a * 32, (dt & 3) * 16, lane);
          ot[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa0, ot[0][dt], 0, 0, 0);
          ot[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa1, ot[1][dt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qi = row0 + 16 * t + i;
    // SUMCOL: the row sum is column dh = (NDT - 1) * 16 + 8 of O: register 0 of the lanes with g = 2
    const float lsum = SUMCOL ? __shfl(ot[t][NDT - 1][0], 32 + i) : group_sum(l[t]);
    if (active && qi < p.Tq) {
      const float inv = 1.0f / lsum;
      bf16_t* orow = p.o + (long)b * p.o_sb + (long)qi * p.o_st + h * dh;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * g;
        if (col >= dh) continue;  // dh % 8 == 0: a 4-column group is entirely inside or outside
        const f32x4 v = ot[t][dt] * inv;
        *reinterpret_cast<u32x2*>(orow + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      }
      if (g == 0 && p.lse != nullptr) p.lse[((long)b * p.H + h) * p.Tq + qi] = (m[t] + log2f(lsum)) * (1.0f / LOG2E);
    }
  }
}

// dQ pass, two query tiles per wave (see attn_fwd2_kernel): per 32-key block the four K / V row fragments and the NDT K column
// fragments are read once for both tiles: 22 MFMAs per 8 ds_read_b128 + 6 ds_read_b64_tr_b16 (NDT = 3) against 12 per 8 + 8.
// Key rows beyond Tk are zero rows of the staged chunk: their p is finite, their dP and their K are zero, they add nothing.
// (masked / causal instantiations: the predicate registers do not fit beside two 16-row tiles at 128 registers — two waves per
// SIMD for them, no scratch; PLAIN, the UNet's and the ViT's path, keeps four)
// NDT = 5 / 6 (head_dim 72 .. 96; round 6, late): KS = 3 reduction steps and two 64-column halves per staged operand, 4 waves, 128-key
// chunks, two workgroups per CU — the geometry of Fwd2<NDT> (the general one-tile kernel ran the UNet's 80-channel dQ at 746 TFLOP/s).
template <bool PLAIN, int NDT>
__global__ __launch_bounds__(Fwd2<NDT>::NW * 64, PLAIN ? Fwd2<NDT>::WAVES_PER_SIMD : 2) void attn_bwd_dq2_kernel(AttnParams p) {
  using F = Fwd2<NDT>;
  constexpr int NH = F::NH, KS = F::KS, NW = F::NW, CH = F::CH, HB = F::HB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + NH * HB;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const int row0 = (blockIdx.x * NW + wave) * 32;
  const bool active = row0 < p.Tq;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * dh;
  const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * dh;
  const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * dh;
  bf16x8 qf[2][KS], dof[2][KS];
  float delta[2], lse2[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float sacc = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[t][ks] = frag_global_dh(qb, p.q_st, row0 + 16 * t, active ? p.Tq : 0, ks, lane, dh);
      dof[t][ks] = frag_global_dh(dob, p.o_st, row0 + 16 * t, active ? p.Tq : 0, ks, lane, dh);
      const bf16x8 of = frag_global_dh(ob, p.o_st, row0 + 16 * t, active ? p.Tq : 0, ks, lane, dh);
#pragma unroll
      for (int e = 0; e < 8; ++e) sacc += bf16_to_f32((bf16_t)dof[t][ks][e]) * bf16_to_f32((bf16_t)of[e]);
    }
    delta[t] = PLAIN ? group_sum(sacc) : finite_or_zero(group_sum(sacc));
    const int qi = row0 + 16 * t + i;
    const bool qvalid = active && qi < p.Tq;
    const long stat = ((long)b * p.H + h) * p.Tq + qi;
    if (qvalid && g == 0) p.delta[stat] = delta[t];
    lse2[t] = qvalid ? p.lse[stat] * LOG2E : INFINITY;
  }
  const float sl2 = p.scale * LOG2E;
  f32x4 dqt[2][NDT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dqt[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kv0 = 0; kv0 < p.Tk; kv0 += CH) {
    const int rows = min(CH, p.Tk - kv0);
    __syncthreads();
    {
      int ln = lane;  // opaque copy: see attn_fwd2_kernel
      asm volatile("" : "+v"(ln));
      dma_oper<NH>(Ks, p.k + (long)b * p.kv_sb + (long)kv0 * p.kv_st + h * dh, p.kv_st, rows, dh, wave, NW, ln);
      dma_oper<NH>(Vs, p.v + (long)b * p.kv_sb + (long)kv0 * p.kv_st + h * dh, p.kv_st, rows, dh, wave, NW, ln);
    }
    lds_dma_wait_all();
    __syncthreads();
    if (!active) continue;
    if (p.causal && kv0 > row0 + 31) continue;
    const int nbl = (rows + 31) / 32;
#pragma unroll 1
    for (int a = 0; a < nbl; ++a) {
      f32x4 ds[2][2];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int r16 = a * 32 + jt * 16;
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          kf[ks] = frag_rows(Ks + (ks >> 1) * HB, r16, ks & 1, lane);
          vf[ks] = frag_rows(Vs + (ks >> 1) * HB, r16, ks & 1, lane);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[t][ks], sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[ks], dof[t][ks], dp, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = __builtin_amdgcn_exp2f(fmaf(sc[r], sl2, -lse2[t]));
            if (!PLAIN) {
              const int qi = row0 + 16 * t + i;
              pr = keep_at(p, b, h, qi < p.Tq ? qi : p.Tq - 1, kv0 + r16 + 4 * g + r) ? pr : 0.f;
            }
            ds[t][jt][r] = pr * (dp[r] - delta[t]);
          }
        }
      }
      const bf16x8 dsp0 = pack8(ds[0][0], ds[0][1]);
      const bf16x8 dsp1 = pack8(ds[1][0], ds[1][1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const bf16x8 kc = frag_cols(Ks + (dt >> 2) * HB, a * 32, (dt & 3) * 16, lane);
        dqt[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc, dsp0, dqt[0][dt], 0, 0, 0);
        dqt[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc, dsp1, dqt[1][dt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qi = row0 + 16 * t + i;
    if (active && qi < p.Tq) {
      bf16_t* dqrow = p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * dh;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * g;
        if (col >= dh) continue;
        const f32x4 v = dqt[t][dt] * p.scale;
        *reinterpret_cast<u32x2*>(dqrow + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      }
    }
  }
}

// dK / dV pass, two key tiles per wave: 4-wave workgroups of 128 key rows over 128-row chunks of Q / dO (33 KB of LDS: three to
// four workgroups per CU).  Per 32-query block the eight Q / dO row fragments, the statistics and the 2 NDT column fragments are
// read once for both key tiles: 28 MFMAs per 12 ds_read_b128 + 12 ds_read_b64_tr_b16 (NDT = 3) against 16 per 12 + 16 — the
// one-tile kernel is LDS-bandwidth-bound (80 LDS cycles per wave and block x 16 waves = 1 280 per CU against 1 024 matrix cycles
// per SIMD).  ~165 registers: three waves per SIMD.  delta must be ready (the dQ pass, or attn_delta_kernel).
constexpr int A2D_CH = 128;
constexpr int A2D_TILE = A2D_CH * 128;

// NDT = 5 / 6 (head_dim 72 .. 96, the UNet's 80-channel heads; round 3b): the same loop over KS = 3 reduction steps and two
// 64-column halves of the staged operands (66 KB of LDS, ~215 registers: two workgroups per CU) — the general one-tile kernel
// ran this head_dim at 342 TFLOP/s against 800 for head_dim 40 here.
// FOLD (round 6; plain, head_dim 40): dP - delta from the matrix pipe, as in attn_bwd_dq3_kernel — ones in columns 40 / 41 of the V
// fragments, -bf16(delta) / -bf16(delta - hi) in columns 40 / 41 of the staged dO rows (written by the thread that owns the row's
// statistics; the dO DMAs skip the pad columns).
template <bool PLAIN, int NDT, bool FOLD = false>
__global__ __launch_bounds__(256, (NDT == 3 && PLAIN) ? 3 : 2) void attn_bwd_dkv2_kernel(AttnParams p) {
  static_assert(!FOLD || (PLAIN && NDT == 3), "the folded delta: plain head_dim-40 form only");
  constexpr int KS = (NDT + 1) / 2;     // 32-deep steps of the reductions over head_dim
  constexpr int NHALF = (NDT + 3) / 4;  // 64-column halves of a staged operand
  extern __shared__ __attribute__((aligned(128))) char smem[];  // 128: the XOR-derived addresses below need whole tile rows
  char* Qs = smem;
  char* dOs = smem + NHALF * A2D_TILE;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * NHALF * A2D_TILE);
  float* delta_s = lse_s + A2D_CH;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const int row0 = (blockIdx.x * 4 + wave) * 32;
  const bool active = row0 < p.Tk;
  const bf16_t* kb = p.k + (long)b * p.kv_sb + h * dh;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + h * dh;
  bf16x8 kf[2][KS], vf[2][KS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      kf[u][ks] = frag_global_dh(kb, p.kv_st, row0 + 16 * u, active ? p.Tk : 0, ks, lane, dh);
      vf[u][ks] = frag_global_dh(vb, p.kv_st, row0 + 16 * u, active ? p.Tk : 0, ks, lane, dh);
    }
  if (FOLD) {
    if (g == 1) {  // dh == 40: the (ks = 1, g = 1) fragment is columns 40 .. 47
      vf[0][KS - 1][0] = vf[0][KS - 1][1] = (short)0x3F80;
      vf[1][KS - 1][0] = vf[1][KS - 1][1] = (short)0x3F80;
    }
    for (int idx = threadIdx.x; idx < A2D_CH * 8; idx += 256) {  // the pad chunks of the dO tile, once (columns 40 / 41 are rewritten per chunk)
      const int row = idx >> 3, chunk = idx & 7;
      if (chunk * 8 >= dh) *reinterpret_cast<u32x4*>(dOs + row * 128 + ((chunk ^ swz(row)) << 4)) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  const float sl2 = p.scale * LOG2E;
  f32x4 dkt[2][NDT], dvt[2][NDT];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { dkt[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  // Lane-constant parts of the LDS addresses of a block as opaque LDS-space pointers (see attn_bwd_dq3_kernel / attn_bwd_one_kernel):
  // the other reduction half of a row fragment and the other column tiles are an XOR of bits 5..6 away, halves / dO / the second
  // transposing read / the second 16-row tile are immediates; a block adds its a * 4 096 (statistics: a * 128) bytes to three of them.
  lds_cp qr0, qc0, sp;
  {
    const lds_cp q3 = (lds_cp)LDS_PTR(Qs);
    qr0 = q3 + n * 128 + ((g ^ swz(n)) << 4);
    qc0 = q3 + tile_off(4 * g + (n >> 2), 4 * (n & 3));
    sp = (lds_cp)LDS_PTR(lse_s) + 16 * g;
    CFHIP_OPAQUE_LDS(qr0, lds_cp)
    CFHIP_OPAQUE_LDS(qc0, lds_cp)
    CFHIP_OPAQUE_LDS(sp, lds_cp)
  }
  constexpr int DO_OFF = NHALF * A2D_TILE;  // the dO tile(s) behind the Q tile(s)
  for (int q0 = 0; q0 < p.Tq; q0 += A2D_CH) {
    const int rows = min(A2D_CH, p.Tq - q0);
    __syncthreads();
    {
      int ln = lane;  // opaque copy: see attn_fwd2_kernel
      asm volatile("" : "+v"(ln));
#pragma unroll
      for (int hf = 0; hf < NHALF; ++hf) {
        dma_half(Qs + hf * A2D_TILE, p.q + (long)b * p.q_sb + (long)q0 * p.q_st + h * dh, p.q_st, rows, A2D_CH, hf, dh, wave, 4, ln);
        dma_half<FOLD>(dOs + hf * A2D_TILE, p.d_o + (long)b * p.o_sb + (long)q0 * p.o_st + h * dh, p.o_st, rows, A2D_CH, hf, dh, wave, 4, ln);
      }
    }
    if ((int)threadIdx.x < A2D_CH) {  // thread t owns the statistics of row t of the chunk
      const int tq = q0 + (int)threadIdx.x;
      const long at = ((long)b * p.H + h) * p.Tq + tq;
      lse_s[threadIdx.x] = tq < p.Tq ? p.lse[at] * LOG2E : INFINITY;
      const float dl = tq < p.Tq ? (PLAIN ? p.delta[at] : finite_or_zero(p.delta[at])) : 0.f;
      if (FOLD) {
        const bf16_t hi = f32_to_bf16(-dl);
        const bf16_t lo = f32_to_bf16(-dl - bf16_to_f32(hi));
        *reinterpret_cast<unsigned*>(dOs + tile_off((int)threadIdx.x, 40)) = (unsigned)hi | ((unsigned)lo << 16);
      } else {
        delta_s[threadIdx.x] = dl;
      }
    }
    lds_dma_wait_all();
    __syncthreads();
    if (!active) continue;
    if (p.causal && q0 + A2D_CH - 1 < row0) continue;  // every query of the chunk precedes both kv tiles
    const int nbl = (rows + 31) / 32;
#pragma unroll 1
    for (int a = 0; a < nbl; ++a) {
      f32x4 pp[2][2], ds[2][2];  // [kv tile][query 16-row tile]
      const int aoff = a * (32 * 128);
      const lds_cp ra = qr0 + aoff, rb = CFHIP_LDS_XOR(qr0 + aoff, 64), spa = sp + a * 128;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int r16 = a * 32 + it * 16;
        bf16x8 qf[KS], of[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const lds_cp rp = ((ks & 1) ? rb : ra) + (ks >> 1) * A2D_TILE + it * 2048;  // rows r16 + n, reduction half ks
          qf[ks] = *(lds_v8)rp;
          of[ks] = *(lds_v8)(rp + DO_OFF);
        }
        const f32x4 l4 = *(lds_f4)(spa + it * 64);
        f32x4 d4 = {0.f, 0.f, 0.f, 0.f};
        if (!FOLD) d4 = *(lds_f4)(spa + it * 64 + A2D_CH * 4);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[ks], kf[u][ks], sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(of[ks], vf[u][ks], dp, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = __builtin_amdgcn_exp2f(fmaf(sc[r], sl2, -l4[r]));
            if (!PLAIN) {
              const int qi = q0 + r16 + 4 * g + r;
              pr = (qi < p.Tq && keep_at(p, b, h, qi, row0 + 16 * u + n)) ? pr : 0.f;
            }
            pp[u][it][r] = pr;
            ds[u][it][r] = pr * (FOLD ? dp[r] : dp[r] - d4[r]);
          }
        }
      }
      const bf16x8 ppk0 = pack8(pp[0][0], pp[0][1]), ppk1 = pack8(pp[1][0], pp[1][1]);
      const bf16x8 dsk0 = pack8(ds[0][0], ds[0][1]), dsk1 = pack8(ds[1][0], ds[1][1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const lds_cp cp = CFHIP_LDS_XOR(qc0 + aoff, (dt & 3) * 32) + (dt >> 2) * A2D_TILE;  // rows 32 a + 4 g + (n >> 2) (+16: 2 048 bytes on)
        const s16x4 olo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + DO_OFF));
        const s16x4 ohi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + DO_OFF + 2048));
        const bf16x8 oc = join8(olo, ohi);
        dvt[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oc, ppk0, dvt[0][dt], 0, 0, 0);
        dvt[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oc, ppk1, dvt[1][dt], 0, 0, 0);
        const s16x4 qlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)cp);
        const s16x4 qhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + 2048));
        const bf16x8 qc = join8(qlo, qhi);
        dkt[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qc, dsk0, dkt[0][dt], 0, 0, 0);
        dkt[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qc, dsk1, dkt[1][dt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int kj = row0 + 16 * u + n;
    if (active && kj < p.Tk) {
      bf16_t* dkrow = p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * dh;
      bf16_t* dvrow = p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * dh;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * g;
        if (col >= dh) continue;
        const f32x4 kk = dkt[u][dt] * p.scale;
        const f32x4 vv = dvt[u][dt];
        *reinterpret_cast<u32x2*>(dkrow + col) = u32x2{pack_bf16x2(kk[0], kk[1]), pack_bf16x2(kk[2], kk[3])};
        *reinterpret_cast<u32x2*>(dvrow + col) = u32x2{pack_bf16x2(vv[0], vv[1]), pack_bf16x2(vv[2], vv[3])};
      }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Round 6: the backward passes of head_dim <= 48 (the UNet's 40-channel heads: 333 of the 256^2 step's 474 ms of kernel time) with the
// two reductions over head_dim — S = Q K^T and dP = dO V^T — on v_mfma_f32_32x32x16_bf16.  The kernels above run them on 16x16x32
// MFMAs: head_dim 40 is padded to 64 there (two 32-deep steps, the second three quarters empty) and the passes sit at their MFMA-issue
// bound (dK / dV: 1.6 + 1.6 + 1.2 + 1.2 = 5.6 padded units, 1 166 TFLOP/s issued).  A 32x32 tile takes the reduction in 16-deep steps:
// three of them (48) instead of 64 — 3.6 units instead of 4.4 for dQ.  (The 16-deep 16x16 MFMA costs what the 32-deep one does on gfx950
// — measured, profiles/r06/attn_k48_mfma16_rejected.txt — the 32x32x16 one is the double-rate instruction of its shape.)
// MEASURED (profiles/r06/attn_s32x32_ab.txt): dQ at T = 65 536 10.38 -> 9.79 ms (-5.6 %), at T = 4 096 x 8 410 -> 391 us: a quarter of
// what the MFMA count promised — the passes turn out to sit at ~50 % of the matrix pipe with the VALU (exp2, two multiplies, a subtract
// and the packing per score) about as busy, so removing matrix cycles returns a fraction.  The same form of the dK / dV pass (eight
// statistics loads and two swaps per block instead of four and none) was 1.8 % SLOWER (13.60 -> 13.84 ms) and is not in the tree.
// The price is the result layout: lane l holds ONE column (l & 31) and the 16 rows 8 j + 4 (l >> 5) + r, where the products that consume
// dS as an operand (dQ: output width head_dim, 48 on 16-column tiles — a 32-wide tile would pad it to 64 again) want 8
// reduction slots of one of 16 columns per lane.  v_permlane16_swap does that conversion: with X = the packed rows of j in {0, 1} and
// Y = those of j in {2, 3}, swapping X's odd 16-lane rows with Y's even ones leaves in X the complete 16x16x32 operand of columns 0..15
// and in Y that of columns 16..31, k-slot group g = lane >> 4 holding rows base(g) + {0..3, 8..11}, base = {0, 16, 4, 20}: the
// transposing LDS reads of the other operand take their four-row runs from exactly those rows (frag_cols32).  tools/micro/mfma32_swap.hip
// checks the chain bit for bit.  No mask / causal / dropout forms: the UNet's path (PLAIN); everything else stays on the kernels above.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;

// A operand of a 32x32x16 MFMA from a swizzled tile: lane (rho = l & 31, hk = l >> 5) <- tile[row0 + rho][ks*16 + 8 hk .. +8]
__device__ __forceinline__ bf16x8 frag_rows32(const char* tile, int row0, int ks, int lane) {
  const int row = row0 + (lane & 31);
  const int slot = ks * 2 + (lane >> 5);
  return *reinterpret_cast<const bf16x8*>(tile + row * 128 + ((slot ^ swz(row)) << 4));
}

// the same straight from global memory for the wave's own 32 rows, zero beyond dh / rows_valid
__device__ __forceinline__ bf16x8 frag_global32_dh(const bf16_t* base, long stride_t, int row0, int rows_valid, int ks, int lane, int dh) {
  const int row = row0 + (lane & 31);
  const int col = ks * 16 + (lane >> 5) * 8;
  bf16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < rows_valid && col < dh) r = *reinterpret_cast<const bf16x8*>(base + (long)row * stride_t + col);
  return r;
}

// column-operand fragment over the 32-row block at `r32`, columns c0..c0+15, in the k-slot order of swap32_operands' results
__device__ __forceinline__ bf16x8 frag_cols32(const char* tile, int r32, int c0, int lane) {
  const int g = lane >> 4, s = lane & 15;
  const int r_lo = r32 + (g & 1) * 16 + (g >> 1) * 4 + (s >> 2);
  const int col = c0 + 4 * (s & 3);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + tile_off(r_lo, col)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + tile_off(r_lo + 8, col)));
  return join8(lo, hi);
}

// 32x32 MFMA result (16 f32 per lane: column l & 31, rows 8 j + 4 (l >> 5) + r) -> the bf16 B operands of two 16x16x32 MFMAs:
// `lo` for columns 0..15, `hi` for columns 16..31 (lane n = l & 15 in both), 32 reduction slots in frag_cols32's order
__device__ __forceinline__ void swap32_operands(const f32x16& t, bf16x8& lo, bf16x8& hi) {
  union { bf16x8 v; unsigned w[4]; } x, y;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    x.w[w] = pack_bf16x2(t[2 * w], t[2 * w + 1]);
    y.w[w] = pack_bf16x2(t[8 + 2 * w], t[8 + 2 * w + 1]);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const auto r = __builtin_amdgcn_permlane16_swap(x.w[w], y.w[w], false, false);
    x.w[w] = r[0];
    y.w[w] = r[1];
  }
  lo = x.v;
  hi = y.v;
}

// FOLD (head_dim 40: the reduction is padded to 48, columns 40 / 41 are free): dP - delta comes out of the matrix pipe.  The staged V tile
// carries ones in columns 40 and 41 (written once; the chunk DMAs skip the pad columns), the dO fragment -bf16(delta) and -bf16(delta - hi)
// (16 mantissa bits of delta): 16 subtractions per lane and 32 x 32 block leave a loop whose VALU is as busy as its matrix pipe.
template <int NDT, bool FOLD>
__global__ __launch_bounds__(512, 4) void attn_bwd_dq3_kernel(AttnParams p) {
  static_assert(NDT == 3, "head_dim <= 48: three 16-deep reduction steps, three 16-column output tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + A2_TILE;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const int row0 = (blockIdx.x * 8 + wave) * 32;
  const bool active = row0 < p.Tq;
  const bf16_t* qb = p.q + (long)b * p.q_sb + h * dh;
  const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * dh;
  const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * dh;
  bf16x8 qf[3], dof[3];
  float sacc = 0.f;
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    qf[ks] = frag_global32_dh(qb, p.q_st, row0, active ? p.Tq : 0, ks, lane, dh);
    dof[ks] = frag_global32_dh(dob, p.o_st, row0, active ? p.Tq : 0, ks, lane, dh);
    const bf16x8 of = frag_global32_dh(ob, p.o_st, row0, active ? p.Tq : 0, ks, lane, dh);
#pragma unroll
    for (int e = 0; e < 8; ++e) sacc += bf16_to_f32((bf16_t)dof[ks][e]) * bf16_to_f32((bf16_t)of[e]);
  }
  const float delta = sacc + __shfl_xor(sacc, 32, 64);  // the two halves of a row's reduction sit in lanes l and l ^ 32
  if (FOLD) {  // dh == 40: element 0 / 1 of the (ks = 2, hk = 1) fragment are columns 40 / 41
    const bf16_t hi = f32_to_bf16(-delta);
    const bf16_t lo = f32_to_bf16(-delta - bf16_to_f32(hi));
    if (lane >= 32) { dof[2][0] = (short)hi; dof[2][1] = (short)lo; }
    for (int idx = threadIdx.x; idx < A2_CH * 8; idx += 512) {  // the pad chunks of the V tile, once: ones in columns 40 / 41
      const int row = idx >> 3, chunk = idx & 7;
      if (chunk * 8 >= dh)
        *reinterpret_cast<u32x4*>(Vs + row * 128 + ((chunk ^ swz(row)) << 4)) = u32x4{chunk * 8 == dh ? 0x3F803F80u : 0u, 0u, 0u, 0u};
    }
  }
  const int qrow = row0 + (lane & 31);
  const bool qvalid = active && qrow < p.Tq;
  const long stat = ((long)b * p.H + h) * p.Tq + qrow;
  if (qvalid && lane < 32) p.delta[stat] = delta;
  const float lse2 = qvalid ? p.lse[stat] * LOG2E : INFINITY;
  const float sl2 = p.scale * LOG2E;
  f32x4 dqt[2][NDT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dqt[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Lane-constant parts of the twelve LDS addresses of a block (the swizzle key of row a*32 + r is that of r; the V tile sits A2_TILE
  // bytes behind the K tile, the second transposing read 8 rows = 1 024 bytes behind the first): a block adds its a * 4 096 bytes to SIX
  // of them — the compiler's own form added it to all twelve, 12 of the loop's 72 VALU instructions.
  // (kept as LDS-space pointers: through generic pointers every load paid a `v_add_u32 v, 0, v` for the address-space cast)
  lds_cp kr[3], kc[NDT];
  {
    const lds_cp ks3 = (lds_cp)LDS_PTR(Ks);
    const int r = lane & 31;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) kr[ks] = ks3 + r * 128 + (((ks * 2 + (lane >> 5)) ^ swz(r)) << 4);
    const int s16 = lane & 15;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) kc[dt] = ks3 + tile_off((g & 1) * 16 + (g >> 1) * 4 + (s16 >> 2), dt * 16 + 4 * (s16 & 3));
    // opaque: the tile's base is a link-time constant that hipcc otherwise adds at every USE (`v_add_u32 v, 0, v`) beside the loop's increments
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) { unsigned u = (unsigned)(uintptr_t)kr[ks]; asm volatile("" : "+v"(u)); kr[ks] = (lds_cp)(uintptr_t)u; }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { unsigned u = (unsigned)(uintptr_t)kc[dt]; asm volatile("" : "+v"(u)); kc[dt] = (lds_cp)(uintptr_t)u; }
  }
  for (int kv0 = 0; kv0 < p.Tk; kv0 += A2_CH) {
    const int rows = min(A2_CH, p.Tk - kv0);
    __syncthreads();
    {
      int ln = lane;  // opaque copy: see attn_fwd2_kernel
      asm volatile("" : "+v"(ln));
      dma_oper<1>(Ks, p.k + (long)b * p.kv_sb + (long)kv0 * p.kv_st + h * dh, p.kv_st, rows, dh, wave, 8, ln);
      dma_oper<1, FOLD>(Vs, p.v + (long)b * p.kv_sb + (long)kv0 * p.kv_st + h * dh, p.kv_st, rows, dh, wave, 8, ln);
    }
    lds_dma_wait_all();
    __syncthreads();
    if (!active) continue;
    const int nbl = (rows + 31) / 32;
#pragma unroll 1
    for (int a = 0; a < nbl; ++a) {
      f32x16 sc, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { sc[e] = 0.f; dp[e] = 0.f; }
      const int aoff = a * (32 * 128);
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const lds_cp kp = kr[ks] + aoff;
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(lds_v8)kp, qf[ks], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(lds_v8)(kp + A2_TILE), dof[ks], dp, 0, 0, 0);
      }
      // lane: query row0 + (l & 31), keys a*32 + 8 j + 4 (l >> 5) + r.  Key rows beyond Tk are zero rows of the chunk: p finite, dP = 0
#pragma unroll
      for (int e = 0; e < 16; ++e) sc[e] = __builtin_amdgcn_exp2f(fmaf(sc[e], sl2, -lse2)) * (FOLD ? dp[e] : dp[e] - delta);
      bf16x8 ds0, ds1;
      swap32_operands(sc, ds0, ds1);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const lds_cp cp = kc[dt] + aoff;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)cp);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(cp + 8 * 128));
        const bf16x8 kcf = join8(lo, hi);
        dqt[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kcf, ds0, dqt[0][dt], 0, 0, 0);
        dqt[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kcf, ds1, dqt[1][dt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qi = row0 + 16 * t + i;
    if (active && qi < p.Tq) {
      bf16_t* dqrow = p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * dh;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int col = dt * 16 + 4 * g;
        if (col >= dh) continue;
        const f32x4 v = dqt[t][dt] * p.scale;
        *reinterpret_cast<u32x2*>(dqrow + col) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      }
    }
  }
}

int check_common(const char* who, const void* q, const void* k, const void* v, int B, int H, int Tq, int Tk,
                 int64_t q_sb, int64_t q_st, int64_t kv_sb, int64_t kv_st, int64_t o_sb, int64_t o_st) {
  CFHIP_REQUIRE(q && k && v, "%s: null q/k/v", who);
  CFHIP_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "%s: empty problem", who);
  CFHIP_REQUIRE((long)B * 1 <= 65535 && H <= 65535, "%s: B = %d / H = %d exceed the grid limits", who, B, H);
  CFHIP_REQUIRE(q_sb % 8 == 0 && q_st % 8 == 0 && kv_sb % 8 == 0 && kv_st % 8 == 0 && o_sb % 8 == 0 &&
                    o_st % 8 == 0,
                "%s: strides must be multiples of 8 elements", who);
  CFHIP_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0,
                "%s: q/k/v must be 16-byte aligned", who);
  return CFHIP_OK;
}

// delta[b][h][t] = sum_d dO[b][t][h][d] * O[b][t][h][d]: what the dQ pass leaves behind for the dK / dV pass; launched on its
// own when the dK / dV pass of the two-slot kernels runs without a dQ pass in front of it (one thread per row).
__global__ void attn_delta_kernel(AttnParams p) {
  const long total = (long)p.B * p.H * p.Tq;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int t = (int)(idx % p.Tq);
    const long bh = idx / p.Tq;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    const bf16_t* dor = p.d_o + (long)b * p.o_sb + (long)t * p.o_st + h * p.dh;
    const bf16_t* orr = p.o_in + (long)b * p.o_sb + (long)t * p.o_st + h * p.dh;
    float s = 0.f;
    for (int sl = 0; sl < p.dh / 8; ++sl) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(dor + sl * 8);
      const u32x4 c = *reinterpret_cast<const u32x4*>(orr + sl * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += bf16lo(a[e]) * bf16lo(c[e]) + bf16hi(a[e]) * bf16hi(c[e]);
    }
    p.delta[idx] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// Host side.  A call is planned first (plan_fwd / plan_bwd: which kernels, from the shape, the mode and the options
// alone), then launched step by step (launch_step: the family file's launcher, which holds each grid, block and LDS byte count; launch,
// csrc/attn_host.h: the one place that reserves LDS, launches and checks).  cfhip_attn_plan prints the same plan without touching a device.
// ---------------------------------------------------------------------------------------------

enum : int {  // "attn_two_tiles" bits (the numeric values are the public option interface: include/cfhip.h)
  TT_FWD = 1,         // forward of head_dim <= 64 on attn_fwd2_kernel
  TT_DQ = 2,          // dQ pass of head_dim <= 48 on attn_bwd_dq2_kernel / attn_bwd_dq3_kernel
  TT_DQ_WIDE = 4,     // with TT_DQ: also head_dim 56 / 64 (the 4-column-tile form)
  TT_DKV = 8,         // dK / dV pass of head_dim <= 64 on attn_bwd_dkv2_kernel
  TT_SUMCOL = 16,     // plain forward row sums through the ones column when head_dim = 8 mod 16
  TT_DKV_96 = 32,     // with TT_DKV: dK / dV pass of head_dim 72 .. 96 on attn_bwd_dkv2_kernel<.., 5 / 6>
  TT_DQ3 = 64,        // plain head_dim <= 48 dQ pass with S / dP on 32x32x16 MFMAs (attn_bwd_dq3_kernel)
  TT_FOLD = 128,      // head_dim 40, plain: dP - delta out of the matrix pipe in that dQ pass and in the dK / dV pass
  TT_PLAIN_96 = 256,  // head_dim 72 .. 96 without a mask: forward and dQ pass on the two-tile kernels (Fwd2<5 / 6>)
};
enum : int {  // "attn_persistent" bits: persistent 16-wave workgroups when 128 < T <= 256 (the ViT shape)
  PERS_DKV = 1,  // dK / dV pass
  PERS_DQ = 2,   // dQ pass
  PERS_FWD = 4,  // forward
};
enum : int {  // "attn_one_pass" values: dQ, dK and dV of a short self-attention from one evaluation of S and dP
  ONE_PASS_OFF = 0,   // the two-pass kernels
  ONE_PASS_ONE = 1,   // attn_bwd_one_kernel at every length 32 < T <= 224
  ONE_PASS_ONE2 = 2,  // that, with 128 < T <= 224 without a mask on attn_bwd_one2_kernel (bit-identical results)
};

struct AttnOptions {
  int short_max = CFHIP_ATTN_MAX_T;  // "attn_short_max": head_dim-64 sequences up to this length take the LDS-resident kernels
  int two_tiles = TT_FWD | TT_DQ | TT_DQ_WIDE | TT_DKV | TT_SUMCOL | TT_DKV_96 | TT_DQ3 | TT_FOLD | TT_PLAIN_96;
  int pers_ctas = 256;  // "attn_pers_ctas": workgroups of a persistent launch (one per CU; fewer leave CUs to the other queues)
  int one_pass = ONE_PASS_ONE2;
  int persistent = PERS_DKV | PERS_DQ | PERS_FWD;
};
AttnOptions g_opt;

// ---- plan ----------------------------------------------------------------------------------


struct Plan {  // the steps of one call, in launch order
  int count = 0;
  Step steps[3];
  void add(Family family, int n = 0, bool plain = false, bool flag = false) { steps[count++] = Step{family, n, plain, flag}; }
};

struct PlanInput {  // everything the selection depends on, next to the options
  int dh, Tq, Tk;
  bool mask, causal, dropout;
  int parts;  // backward: 1 dQ pass, 2 dK / dV pass, 3 both
  bool lse;   // forward: lse is asked for
  bool plain() const { return !mask && !causal; }
  bool delta_ready() const { return (parts & 3) == 3; }  // the dQ pass of the same call writes delta in front of the dK / dV pass
  int halves() const { return (dh + 63) / 64; }  // NH of the general kernels (head_dim <= 192: at most 3)
  // the LDS-resident kernels: head_dim 64, both lengths up to attn_short_max; otherwise the chunked general forms
  bool resident(const AttnOptions& o) const { return dh == CFHIP_ATTN_HEAD_DIM && Tq <= o.short_max && Tk <= o.short_max; }
};


Plan plan_fwd(const PlanInput& in, const AttnOptions& o) {
  Plan plan;
  const bool plain = in.plain();
  const int nh = in.halves(), tt = o.two_tiles;
  if (in.dropout) {  // dropout on the probabilities: the general kernels' DROP forms
    plan.add(GEN_FWD, nh, plain, true);
  } else if (!in.resident(o)) {  // chunked K / V with online softmax, head_dim as zero-padded 64-column halves
    if (nh == 1 && (tt & TT_FWD)) {
      const int ndt = in.dh <= 48 ? 3 : 4;
      plan.add(FWD2, ndt, plain, plain && in.dh == (ndt - 1) * 16 + 8 && (tt & TT_SUMCOL));  // a free column in the last tile
    } else if (nh == 2 && plain && in.dh <= 96 && (tt & TT_PLAIN_96)) {  // (masked / causal sequences of that width stay general)
      plan.add(FWD2, in.dh <= 80 ? 5 : 6, true);
    } else {
      plan.add(GEN_FWD, nh, plain);
    }
  } else if (plain && (o.persistent & PERS_FWD) && in.Tq > 128 && in.Tq <= PERS_WAVES * 16 && in.Tk > 128 && in.Tk <= 256 && in.lse) {
    plan.add(FWD_PERS, (in.Tk + 31) / 32);
  } else {
    plan.add(FWD, (in.Tk + 31) / 32, plain);
  }
  return plan;
}

Plan plan_bwd(const PlanInput& in, const AttnOptions& o) {
  Plan plan;
  const bool plain = in.plain(), want_dq = in.parts & 1, want_dkv = in.parts & 2;
  const int nh = in.halves(), tt = o.two_tiles, dh = in.dh;
  if (in.dropout) {
    if (want_dq) plan.add(GEN_DQ, nh, plain, true);
    if (want_dkv) plan.add(GEN_DKV, nh, plain, true);
    return plan;
  }
  if (!in.resident(o)) {
    // the two-tile dK / dV pass reads delta: without a dQ pass in front of it, attn_delta_kernel fills it
    const bool dkv2 = want_dkv && (tt & TT_DKV) && (nh == 1 || (nh == 2 && dh <= 96 && (tt & TT_DKV_96)));
    if (dkv2 && !in.delta_ready()) plan.add(DELTA);
    if (want_dq) {
      if (nh == 1 && (tt & TT_DQ) && (dh <= 48 || (tt & TT_DQ_WIDE))) {
        if (dh > 48) plan.add(DQ2, 4, plain);
        else if (plain && (tt & TT_DQ3)) plan.add(DQ3, 3, true, dh == 40 && (tt & TT_FOLD));
        else plan.add(DQ2, 3, plain);
      } else if (nh == 2 && plain && dh <= 96 && (tt & TT_PLAIN_96)) {
        plan.add(DQ2, dh <= 80 ? 5 : 6, true);
      } else {
        plan.add(GEN_DQ, nh, plain);
      }
    }
    if (dkv2) {
      const int ndt = dh <= 48 ? 3 : dh <= 64 ? 4 : dh <= 80 ? 5 : 6;
      plan.add(DKV2, ndt, plain, plain && dh == 40 && (tt & TT_FOLD));
    } else if (want_dkv) {
      static_assert(Gen<1>::NSLOT == 1 && Gen<2>::NSLOT == 1 && Gen<3>::NSLOT == 1, "a two-slot ring reads delta: plan DELTA for it");
      plan.add(GEN_DKV, nh, plain);
    }
    return plan;
  }
  const int nbq = (in.Tq + 31) / 32, nb = (in.Tk + 31) / 32;
  if (in.delta_ready() && !in.mask && o.one_pass != ONE_PASS_OFF && in.Tq == in.Tk && in.Tq > 32 && in.Tq <= 224 &&
      (!in.causal || (nbq >= 3 && nbq <= 5))) {
    // dQ, dK and dV of a head from one evaluation of S and dP: 16-wave workgroups, one per CU, for the ViT lengths; 4 / 8 waves
    // and several workgroups per CU for the short sequences (ViT-B/32 in CLIP: T = 50; its causal text tower: T = 77).  Causal
    // instantiations exist for 64 < T <= 160 (the others would spill two registers: the two-pass kernels take them).
    if (in.causal) plan.add(ONE, nbq, false, true);
    else if (nbq >= 5 && o.one_pass >= ONE_PASS_ONE2) plan.add(ONE2, nbq);  // two key tiles per wave: 8 waves
    else plan.add(ONE, nbq);
    return plan;
  }
  const bool vit = plain && in.Tq > 128;  // persistent workgroups, the next head's operands streaming in behind the current one
  if (want_dq && vit && (o.persistent & PERS_DQ) && in.Tq <= PERS_WAVES * 16 && in.Tk > 128 && in.Tk <= 256) plan.add(DQ_PERS, nb);
  else if (want_dq) plan.add(DQ, nb, plain);
  if (want_dkv && vit && in.delta_ready() && (o.persistent & PERS_DKV) && in.Tk <= PERS_WAVES * 16) plan.add(DKV_PERS, nbq);
  else if (want_dkv) plan.add(DKV, nbq, plain);
  return plan;
}

// the instantiation of a step as a profiler prints it, spaces removed: "attn_fwd2_kernel<true,3,false>"
int step_name(const Step& st, char* out, size_t bytes) {
  const char* pl = st.plain ? "true" : "false";
  const char* fl = st.flag ? "true" : "false";
  switch (st.family) {
    case FWD: return snprintf(out, bytes, "attn_fwd_kernel<%d,%s>", st.n, pl);
    case FWD_PERS: return snprintf(out, bytes, "attn_fwd_pers_kernel<%d>", st.n);
    case FWD2: return snprintf(out, bytes, "attn_fwd2_kernel<%s,%d,%s>", pl, st.n, fl);
    case GEN_FWD: return snprintf(out, bytes, "attn_gen_fwd_kernel<%d,%s,%s>", st.n, pl, fl);
    case DELTA: return snprintf(out, bytes, "attn_delta_kernel");
    case DQ: return snprintf(out, bytes, "attn_bwd_dq_kernel<%s>", pl);
    case DQ_PERS: return snprintf(out, bytes, "attn_bwd_dq_pers_kernel<%d>", st.n);
    case DQ2: return snprintf(out, bytes, "attn_bwd_dq2_kernel<%s,%d>", pl, st.n);
    case DQ3: return snprintf(out, bytes, "attn_bwd_dq3_kernel<%d,%s>", st.n, fl);
    case GEN_DQ: return snprintf(out, bytes, "attn_gen_bwd_dq_kernel<%d,%s,%s>", st.n, pl, fl);
    case DKV: return snprintf(out, bytes, "attn_bwd_dkv_kernel<%s>", pl);
    case DKV_PERS: return snprintf(out, bytes, "attn_bwd_dkv_pers_kernel<%d>", st.n);
    case DKV2: return snprintf(out, bytes, "attn_bwd_dkv2_kernel<%s,%d,%s>", pl, st.n, fl);
    case GEN_DKV: return snprintf(out, bytes, "attn_gen_bwd_dkv_kernel<%d,%s,%s>", st.n, pl, fl);
    case ONE: return snprintf(out, bytes, "attn_bwd_one_kernel<%d,%d,%s>", st.n, one_pass_waves(st.n), fl);
    case ONE2: return snprintf(out, bytes, "attn_bwd_one2_kernel<%d>", st.n);
  }
  return 0;
}

// ---- launch --------------------------------------------------------------------------------

int launch_step(const Step& st, const AttnParams& p, hipStream_t s) {
  const dim3 q128((p.Tq + 127) / 128, p.H, p.B), k128((p.Tk + 127) / 128, p.H, p.B);
  switch (st.family) {
    case FWD: case FWD_PERS: case DQ: case DQ_PERS: case DKV: case DKV_PERS:
      return launch_resident(st, p, g_opt.pers_ctas, s);
    case ONE: case ONE2:
      return launch_one_pass(st, p, g_opt.pers_ctas, s);
    case FWD2:
      return with_args<3, 4, 5, 6>(st, "attn_fwd", [&](auto NDT, auto PLAIN, auto SUMCOL) {
        using F = Fwd2<NDT()>;  // head_dim 72 .. 96 (two halves): the plain form only; the ones column: plain, one half
        if constexpr (PLAIN() ? (SUMCOL() && F::NH == 2) : (SUMCOL() || F::NH == 2)) return no_kernel(st);
        else return launch<attn_fwd2_kernel<PLAIN(), NDT(), SUMCOL()>>(dim3((p.Tq + F::NW * 32 - 1) / (F::NW * 32), p.H, p.B), F::NW * 64,
                                                                          (size_t)2 * F::NH * F::HB, s, "attn_fwd2", p);
      });
    case GEN_FWD:
      return with_args<1, 2, 3>(st, "attn_fwd", [&](auto NH, auto PLAIN, auto DROP) {
        return launch<attn_gen_fwd_kernel<NH(), PLAIN(), DROP()>>(q128, 512, (size_t)Gen<NH()>::NSLOT * Gen<NH()>::SLOT_BYTES, s, "attn_gen_fwd", p);
      });
    case DQ2:
      return with_args<3, 4, 5, 6>(st, "attn_bwd", [&](auto NDT, auto PLAIN, auto) {
        using F = Fwd2<NDT()>;
        if constexpr (!PLAIN() && F::NH == 2) return no_kernel(st);  // head_dim 72 .. 96: the plain form only
        else return launch<attn_bwd_dq2_kernel<PLAIN(), NDT()>>(dim3((p.Tq + F::NW * 32 - 1) / (F::NW * 32), p.H, p.B), F::NW * 64,
                                                                  (size_t)2 * F::NH * F::HB, s, "attn_bwd_dq2", p);
      });
    case DQ3:
      return with_args<3>(st, "attn_bwd", [&](auto NDT, auto, auto FOLD) {
        return launch<attn_bwd_dq3_kernel<NDT(), FOLD()>>(dim3((p.Tq + A2_ROWS - 1) / A2_ROWS, p.H, p.B), 512, (size_t)2 * A2_TILE, s, "attn_bwd_dq3", p);
      });
    case GEN_DQ:
      return with_args<1, 2, 3>(st, "attn_bwd", [&](auto NH, auto PLAIN, auto DROP) {
        return launch<attn_gen_bwd_dq_kernel<NH(), PLAIN(), DROP()>>(q128, 512, (size_t)Gen<NH()>::NSLOT * Gen<NH()>::SLOT_BYTES, s, "attn_gen_bwd_dq", p);
      });
    case DKV2:
      return with_args<3, 4, 5, 6>(st, "attn_bwd", [&](auto NDT, auto PLAIN, auto FOLD) {
        if constexpr (FOLD() && !(PLAIN() && NDT() == 3)) return no_kernel(st);  // the folded delta: plain head_dim 40 only
        else return launch<attn_bwd_dkv2_kernel<PLAIN(), NDT(), FOLD()>>(k128, 256, (size_t)2 * ((NDT() + 3) / 4) * A2D_TILE + (size_t)2 * A2D_CH * sizeof(float),
                                                                           s, "attn_bwd_dkv2", p);
      });
    case GEN_DKV:
      return with_args<1, 2, 3>(st, "attn_bwd", [&](auto NH, auto PLAIN, auto DROP) {
        using G = Gen<NH()>;
        return launch<attn_gen_bwd_dkv_kernel<NH(), PLAIN(), DROP()>>(k128, 512, (size_t)G::NSLOT * (G::SLOT_BYTES + (size_t)2 * G::CH * sizeof(float)), s,
                                                                       "attn_gen_bwd_dkv", p);
      });
    case DELTA: {  // one thread per row
      const long blocks = ((long)p.B * p.H * p.Tq + 255) / 256;
      return launch<attn_delta_kernel>(dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), 256, 0, s, "attn_delta", p);
    }
  }
  return no_kernel(st);
}

int launch_plan(const Plan& plan, const AttnParams& p, hipStream_t s) {
  for (int i = 0; i < plan.count; ++i) {
    const int rc = launch_step(plan.steps[i], p, s);
    if (rc != CFHIP_OK) return rc;
  }
  return CFHIP_OK;
}

// fills the dropout fields; false = no dropout (p <= 0).  The probability is quantised to 1/256 (as flash attention
// implementations do): thresh = round(256 p), kept values are scaled by 1 / (1 - thresh / 256).
bool set_dropout(AttnParams& p, float dropout_p, uint64_t seed, uint64_t offset) {
  if (!(dropout_p > 0.f)) return false;
  int t = (int)lrintf(dropout_p * 256.0f);
  t = t < 1 ? 1 : (t > 255 ? 255 : t);
  p.drop_thresh = (unsigned)t;
  p.drop_scale = 256.0f / (float)(256 - t);
  p.drop_seed = seed;
  p.drop_offset = offset;
  p.drop_bq = (p.Tq + 3) / 4;
  p.drop_bk = (p.Tk + 3) / 4;
  return true;
}

int check_head_dim(const char* who, int head_dim) {
  CFHIP_REQUIRE(head_dim >= 8 && head_dim <= 192 && head_dim % 8 == 0,
                "%s: head_dim %d is not a multiple of 8 in [8, 192]", who, head_dim);
  return CFHIP_OK;
}

}  // namespace

int cfhip_internal_set_attn_short_max(int v) {
  g_opt.short_max = v < 0 ? 0 : (v > CFHIP_ATTN_MAX_T ? CFHIP_ATTN_MAX_T : v);
  return CFHIP_OK;
}

int cfhip_internal_set_attn_two_tiles(int v) {
  g_opt.two_tiles = v;
  return CFHIP_OK;
}

int cfhip_internal_set_attn_pers_ctas(int v) {
  g_opt.pers_ctas = v < 1 ? 1 : v;
  return CFHIP_OK;
}

int cfhip_internal_set_attn_one_pass(int v) {
  g_opt.one_pass = v;
  return CFHIP_OK;
}
int cfhip_internal_set_attn_persistent(int v) {
  g_opt.persistent = v;
  return CFHIP_OK;
}

#ifdef CFHIP_ABLATE
int cfhip_internal_set_attn_ablate(int v) {
  g_attn_ablate = v;
  return CFHIP_OK;
}
#endif

static int attn_fwd_impl(const void* q, const void* k, const void* v, void* o, float* lse,
                         const uint8_t* mask, int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b,
                         int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                         int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                         int64_t ms_q, float scale, int causal, void* stream, float dropout_p = 0.f,
                         uint64_t seed = 0, uint64_t offset = 0) {
  int rc = check_head_dim("attn_fwd", head_dim);
  if (rc != CFHIP_OK) return rc;
  rc = check_common("attn_fwd", q, k, v, B, H, Tq, Tk, q_stride_b, q_stride_t, kv_stride_b,
                        kv_stride_t, o_stride_b, o_stride_t);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(o && ((uintptr_t)o & 7) == 0, "attn_fwd: o must be non-null and 8-byte aligned");
  AttnParams p = {};
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o;
  p.lse = lse; p.mask = mask;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk;
  p.q_sb = q_stride_b; p.q_st = q_stride_t; p.kv_sb = kv_stride_b; p.kv_st = kv_stride_t;
  p.o_sb = o_stride_b; p.o_st = o_stride_t;
  p.ms_b = ms_b; p.ms_h = ms_h; p.ms_q = ms_q;
  p.scale = scale; p.causal = causal;
#ifdef CFHIP_ABLATE
  p.ablate = g_attn_ablate;
#endif
  p.dh = head_dim;
  const bool dropout = set_dropout(p, dropout_p, seed, offset);
  const PlanInput in = {head_dim, Tq, Tk, mask != nullptr, causal != 0, dropout, 0, lse != nullptr};
  return launch_plan(plan_fwd(in, g_opt), p, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int cfhip_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                              const uint8_t* mask, int B, int H, int Tq, int Tk, int64_t q_stride_b,
                              int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                              int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                              int64_t ms_q, float scale, int causal, void* stream) {
  return attn_fwd_impl(q, k, v, o, lse, mask, B, H, Tq, Tk, CFHIP_ATTN_HEAD_DIM, q_stride_b, q_stride_t, kv_stride_b,
                       kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal, stream);
}

extern "C" int cfhip_attn_fwd_dh(const void* q, const void* k, const void* v, void* o, float* lse,
                                 const uint8_t* mask, int B, int H, int Tq, int Tk, int head_dim,
                                 int64_t q_stride_b, int64_t q_stride_t, int64_t kv_stride_b,
                                 int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b,
                                 int64_t ms_h, int64_t ms_q, float scale, int causal, void* stream) {
  return attn_fwd_impl(q, k, v, o, lse, mask, B, H, Tq, Tk, head_dim, q_stride_b, q_stride_t, kv_stride_b,
                       kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal, stream);
}

static int attn_bwd_impl(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                         const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk,
                         void* dv, int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b,
                         int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                         int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                         int64_t ms_q, float scale, int causal, int parts, void* stream, float dropout_p = 0.f,
                         uint64_t seed = 0, uint64_t offset = 0) {
  int rc = check_head_dim("attn_bwd", head_dim);
  if (rc != CFHIP_OK) return rc;
  rc = check_common("attn_bwd", q, k, v, B, H, Tq, Tk, q_stride_b, q_stride_t, kv_stride_b,
                        kv_stride_t, o_stride_b, o_stride_t);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(o && d_o && lse && delta && dq && dk && dv, "attn_bwd: null pointer");
  CFHIP_REQUIRE(((uintptr_t)o & 15) == 0 && ((uintptr_t)d_o & 15) == 0 && ((uintptr_t)dq & 7) == 0 &&
                    ((uintptr_t)dk & 7) == 0 && ((uintptr_t)dv & 7) == 0,
                "attn_bwd: misaligned tensors");
  CFHIP_REQUIRE((parts & 3) != 0, "attn_bwd: parts must select the dQ pass (1), the dK/dV pass (2) or both (3)");
  AttnParams p = {};
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.o_in = (const bf16_t*)o; p.d_o = (const bf16_t*)d_o;
  p.lse = const_cast<float*>(lse); p.delta = delta; p.mask = mask;
  p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk;
  p.q_sb = q_stride_b; p.q_st = q_stride_t; p.kv_sb = kv_stride_b; p.kv_st = kv_stride_t;
  p.o_sb = o_stride_b; p.o_st = o_stride_t;
  p.ms_b = ms_b; p.ms_h = ms_h; p.ms_q = ms_q;
  p.scale = scale; p.causal = causal;
#ifdef CFHIP_ABLATE
  p.ablate = g_attn_ablate;
#endif
  p.dh = head_dim;
  const bool dropout = set_dropout(p, dropout_p, seed, offset);
  const PlanInput in = {head_dim, Tq, Tk, mask != nullptr, causal != 0, dropout, parts, true};
  p.delta_ready = in.delta_ready();
  return launch_plan(plan_bwd(in, g_opt), p, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int cfhip_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                              const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk,
                              void* dv, int B, int H, int Tq, int Tk, int64_t q_stride_b,
                              int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                              int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                              int64_t ms_q, float scale, int causal, int parts, void* stream) {
  return attn_bwd_impl(q, k, v, o, d_o, lse, delta, mask, dq, dk, dv, B, H, Tq, Tk, CFHIP_ATTN_HEAD_DIM, q_stride_b,
                       q_stride_t, kv_stride_b, kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal,
                       parts, stream);
}

extern "C" int cfhip_attn_bwd_dh(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                                 const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk,
                                 void* dv, int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b,
                                 int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                                 int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                                 int64_t ms_q, float scale, int causal, int parts, void* stream) {
  return attn_bwd_impl(q, k, v, o, d_o, lse, delta, mask, dq, dk, dv, B, H, Tq, Tk, head_dim, q_stride_b, q_stride_t,
                       kv_stride_b, kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal, parts, stream);
}

extern "C" int cfhip_attn_fwd_dropout(const void* q, const void* k, const void* v, void* o, float* lse,
                                      const uint8_t* mask, int B, int H, int Tq, int Tk, int head_dim,
                                      int64_t q_stride_b, int64_t q_stride_t, int64_t kv_stride_b,
                                      int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b,
                                      int64_t ms_h, int64_t ms_q, float scale, int causal, float dropout_p,
                                      uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "attn_fwd_dropout: p = %f is not in [0, 1)", (double)dropout_p);
  return attn_fwd_impl(q, k, v, o, lse, mask, B, H, Tq, Tk, head_dim, q_stride_b, q_stride_t, kv_stride_b,
                       kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal, stream, dropout_p, seed, offset);
}

extern "C" int cfhip_attn_bwd_dropout(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                                      const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk,
                                      void* dv, int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b,
                                      int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                                      int64_t o_stride_b, int64_t o_stride_t, int64_t ms_b, int64_t ms_h,
                                      int64_t ms_q, float scale, int causal, int parts, float dropout_p,
                                      uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "attn_bwd_dropout: p = %f is not in [0, 1)", (double)dropout_p);
  return attn_bwd_impl(q, k, v, o, d_o, lse, delta, mask, dq, dk, dv, B, H, Tq, Tk, head_dim, q_stride_b, q_stride_t,
                       kv_stride_b, kv_stride_t, o_stride_b, o_stride_t, ms_b, ms_h, ms_q, scale, causal, parts, stream,
                       dropout_p, seed, offset);
}

extern "C" int cfhip_attn_plan(int backward, int head_dim, int Tq, int Tk, int has_mask, int causal, int dropout, int parts,
                               int has_lse, char* out, size_t out_bytes) {
  const int rc = check_head_dim("attn_plan", head_dim);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(Tq > 0 && Tk > 0, "attn_plan: empty problem");
  CFHIP_REQUIRE(!backward || (parts & 3) != 0, "attn_plan: parts must select the dQ pass (1), the dK/dV pass (2) or both (3)");
  CFHIP_REQUIRE(out != nullptr && out_bytes >= 128, "attn_plan: buffer of at least 128 bytes");
  const PlanInput in = {head_dim, Tq, Tk, has_mask != 0, causal != 0, dropout != 0, parts, has_lse != 0};
  const Plan plan = backward ? plan_bwd(in, g_opt) : plan_fwd(in, g_opt);
  size_t at = 0;
  for (int i = 0; i < plan.count; ++i) {
    if (i) out[at++] = '\n';
    at += (size_t)step_name(plan.steps[i], out + at, out_bytes - at);  // three names of at most 38 characters
  }
  return CFHIP_OK;
}

/* the keep mask the DROP kernels use, one byte per (b, h, i, j): for tests and for callers that need the mask itself */
namespace {
__global__ void attn_dropout_mask_kernel(AttnParams p, unsigned char* out) {
  const long total = (long)p.B * p.H * p.Tq * p.Tk;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int j = (int)(idx % p.Tk);
    long t = idx / p.Tk;
    const int i = (int)(t % p.Tq);
    t /= p.Tq;
    const int h = (int)(t % p.H), b = (int)(t / p.H);
    const unsigned w = pick_word(drop_block(p, b, h, i >> 2, j >> 2), i);
    out[idx] = ((w >> (8 * (j & 3))) & 255u) >= p.drop_thresh ? 1 : 0;
  }
}
}  // namespace

extern "C" int cfhip_attn_dropout_mask(void* mask_out, int B, int H, int Tq, int Tk, float dropout_p, uint64_t seed,
                                       uint64_t offset, void* stream) {
  CFHIP_REQUIRE(mask_out && B > 0 && H > 0 && Tq > 0 && Tk > 0, "attn_dropout_mask: bad arguments");
  CFHIP_REQUIRE(dropout_p > 0.f && dropout_p < 1.f, "attn_dropout_mask: p = %f is not in (0, 1)", (double)dropout_p);
  AttnParams p = {};
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk;
  set_dropout(p, dropout_p, seed, offset);
  const long total = (long)B * H * Tq * Tk;
  hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p,
                     (unsigned char*)mask_out);
  CFHIP_CHECK_LAUNCH("attn_dropout_mask");
  return CFHIP_OK;
}
