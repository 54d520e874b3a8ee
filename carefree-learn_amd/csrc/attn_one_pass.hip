#include "common.h"
#include "attn_device.h"
#include "attn_host.h"
#include <math.h>

using namespace cfhip_attn;

namespace {

// The prologue both one-pass kernels share: Q and dO of head `hx` into their LDS tiles (DMA: no registers) ...
__device__ __forceinline__ void stage_q_do(char* Qs, char* dOs, const AttnParams& p, int hx, int rows, int wave, int nwaves, int lane) {
  const int b = hx / p.H, h = hx - b * p.H;
  dma_tile(Qs, p.q + (long)b * p.q_sb + h * DH, p.q_st, p.Tq, rows, wave, nwaves, lane);
  dma_tile(dOs, p.d_o + (long)b * p.o_sb + h * DH, p.o_st, p.Tq, rows, wave, nwaves, lane);
}
// ... and its K
__device__ __forceinline__ void stage_k_tile(char* Ks, const AttnParams& p, int hx, int rows, int wave, int nwaves, int lane) {
  const int b = hx / p.H, h = hx - b * p.H;
  dma_tile(Ks, p.k + (long)b * p.kv_sb + h * DH, p.kv_st, p.Tk, rows, wave, nwaves, lane);
}

// ------------------------------------------------------------------------------------------------
// ONE-PASS backward for the ViT shape (round 6; PLAIN, self-attention, 128 < T <= 224, head_dim 64): dQ, dK and dV of a head from
// ONE evaluation of S and dP.  The two-pass form (csrc/attn_resident.hip) recomputes S = Q K^T and dP = dO V^T in both passes (2 548 MFMAs per head at
// T = 197); the energy table of round 6 ranks attention first in joules per FLOP (2.4-2.9 J/TFLOP against 1.04-1.16 for the GEMMs,
// profiles/r06/energy_table.txt), which is what decided that this experiment gets built.
//   * a 16-wave workgroup owns a CU and walks (batch, head) pairs; Q, dO and K of the head sit in LDS (K / V fragments of a wave's own
//     key tile come from global memory into registers, as in the persistent dK / dV kernel);
//   * phase 1 (waves own KEY tiles): for every query tile of the current half — S, P = exp2(S - lse), dP, dS = P (dP - delta);
//     dV += P^T dO and dK += dS^T Q accumulate in registers over both halves; dS (bf16, the rounding the MFMAs of both passes of the
//     two-pass form use) goes to an LDS buffer [query][key];
//   * barrier; phase 2 (waves own (QUERY tile, half of the 64 columns)): dQ = dS K with the whole key range as the reduction, the
//     dS operand read back from LDS in exactly the k-slot order a packed register operand has; barrier;
//   * queries in two halves so that Q + dO + K + dS + statistics fit 160 KB (T <= 224: 147 KB); delta = rowsum(dO o O) is computed in
//     the prologue (four lanes per row) and also written to p.delta for callers that read it.
// 1 716 MFMAs per head (-33 %), one launch instead of two; what it gives up: the next head's operands no longer stream in behind
// the current head (the LDS is full), and two more barriers per head.
// ------------------------------------------------------------------------------------------------
// CAUSAL: key j attends only to queries i >= j (the CLIP text tower's triu(1) mask as a flag): P = 0 above the diagonal (a predicate on
// the probability; skipping the tiles above the diagonal costs more registers than it saves at T = 77), their zero dS is not read in
// phase 2.
template <int NB, int PW, bool CAUSAL = false>  // NB pairs of 16-row tiles (T <= 32 NB); PW waves per workgroup (>= 2 NB key tiles, >= 4 ceil(NB / 2) phase-2 items)
__global__ __launch_bounds__(PW * 64, 4) void attn_bwd_one_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(128))) char smem[];  // 128: the XOR-derived addresses below need whole tile rows
  constexpr int ROWS = NB * 32, TILE = ROWS * 128;
  constexpr int HA = (NB + 1) / 2;          // query pair-tiles per half
  constexpr int DSROW = ROWS * 2 + 16;      // bytes per dS row (ROWS keys, bf16) + 16: rows 4 apart start 16 banks apart
  static_assert(3 * TILE + 2 * ROWS * 4 + HA * 32 * DSROW <= 160 * 1024, "Q + dO + K + statistics + dS must fit the LDS");
  static_assert(2 * NB <= PW && 4 * HA <= PW && ROWS * 4 <= PW * 64, "a wave per key tile; a wave per (query tile, column half); four lanes per row");
  char* Qs = smem;
  char* dOs = Qs + TILE;
  char* Ks = dOs + TILE;
  float* lse_s = reinterpret_cast<float*>(Ks + TILE);
  float* delta_s = lse_s + ROWS;
  char* dSs = reinterpret_cast<char*>(delta_s + ROWS);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int heads = p.B * p.H;
  const float sl2 = p.scale * LOG2E;
  const int row0 = wave * 16;  // phase 1: this wave's key tile
  const int qt = wave >> 1, ch = wave & 1;  // phase 2: query tile of the half, column half
  const int kq = row0 + n - 4 * g;  // CAUSAL: key (row0 + n) is masked for query (16 it + 4 g + r) when kq > 16 it + r

  // Q and dO of head `hx` into the LDS (DMA: no registers) ...
  auto stage_q = [&](int hx) { stage_q_do(Qs, dOs, p, hx, ROWS, wave, PW, lane); };
  // ... and its statistics (log-sum-exp in the log2 domain, delta = rowsum(dO o O)): four lanes per row, 16 columns each
  auto stage_stats = [&](int hx) {
    const int b = hx / p.H, h = hx - b * p.H;
    const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * DH;
    const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * DH;
    const int t = (int)threadIdx.x >> 2, part = (int)threadIdx.x & 3;
    float sacc = 0.f;
    if (t < p.Tq) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(dob + (long)t * p.o_st + part * 16 + j * 8);
        const bf16x8 c = *reinterpret_cast<const bf16x8*>(ob + (long)t * p.o_st + part * 16 + j * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) sacc += bf16_to_f32((bf16_t)a[e]) * bf16_to_f32((bf16_t)c[e]);
      }
    }
    sacc += __shfl_xor(sacc, 1, 64);
    sacc += __shfl_xor(sacc, 2, 64);
    if (part == 0 && t < ROWS) {
      const bool ok = t < p.Tq;
      lse_s[t] = ok ? p.lse[(long)hx * p.Tq + t] * LOG2E : INFINITY;  // +inf -> p = 0 for padded query rows
      delta_s[t] = ok ? sacc : 0.f;
      if (ok && p.delta != nullptr) p.delta[(long)hx * p.Tq + t] = sacc;
    }
  };
  auto stage_k = [&](int hx) { stage_k_tile(Ks, p, hx, ROWS, wave, PW, lane); };

  // Lane-constant parts of the LDS addresses of both phases, kept as LDS-space pointers and made opaque once (see attn_bwd_dq3_kernel):
  // through generic pointers every access paid a `v_add_u32 v, 0, v` for the link-time base, and the statistics / dS regions sit beyond
  // the 64 KB an instruction's offset field reaches, so each of their twelve accesses per block paid an add of its own — 28 of the 65
  // VALU instructions of the phase-1 block.  With the region's base inside the pointer the rest are immediates: 8 adds per block.
  lds_cp qr0, qc0, sp;
  lds_p dsw;
  {
    // (the tiles start on 128-byte boundaries — the first one at the dynamic LDS base — so the other reduction half of a row fragment and
    // the other column tiles are one XOR of bits 5..6 away: slot ^ key with the key in bits 1..2 of the slot)
    const lds_cp q3 = (lds_cp)LDS_PTR(Qs);
    qr0 = q3 + n * 128 + ((g ^ swz(n)) << 4);
    qc0 = q3 + tile_off(4 * g + (n >> 2), 4 * (n & 3));
    sp = (lds_cp)LDS_PTR(lse_s) + 16 * g;
    dsw = (lds_p)LDS_PTR(dSs) + (row0 + n) * 2 + 4 * g * DSROW;
    CFHIP_OPAQUE_LDS(qr0, lds_cp)
    CFHIP_OPAQUE_LDS(qc0, lds_cp)
    CFHIP_OPAQUE_LDS(sp, lds_cp)
    CFHIP_OPAQUE_LDS(dsw, lds_p)
  }
  int hh = blockIdx.x;
  if (hh < heads) {
    stage_q(hh);
    stage_k(hh);
    stage_stats(hh);
  }
  for (; hh < heads; hh += gridDim.x) {
    const int b = hh / p.H, h = hh - b * p.H;
    const bf16_t* kb = p.k + (long)b * p.kv_sb + h * DH;
    const bf16_t* vb = p.v + (long)b * p.kv_sb + h * DH;
    // this wave's key tile: K / V fragments in registers (rows beyond Tk are zero)
    const bf16x8 kf0 = frag_global(kb, p.kv_st, row0, p.Tk, 0, lane);
    const bf16x8 kf1 = frag_global(kb, p.kv_st, row0, p.Tk, 1, lane);
    const bf16x8 vf0 = frag_global(vb, p.kv_st, row0, p.Tk, 0, lane);
    const bf16x8 vf1 = frag_global(vb, p.kv_st, row0, p.Tk, 1, lane);
    lds_dma_wait_all();
    __syncthreads();
    const int nxt = hh + gridDim.x;

    f32x4 dkt[4], dvt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      const int a0 = hf * HA, a1 = hf == 0 ? HA : NB;
      // ---- phase 1: key tile x the query tiles of this half
      if (row0 < ROWS) {
        for (int a = a0; a < a1; ++a) {
          f32x4 pp[2], ds[2];
          const int aoff = a * (32 * 128);
          const lds_cp spa = sp + a * 128;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int it = 2 * a + t;
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const lds_cp r0 = qr0 + aoff + t * 2048, r1 = CFHIP_LDS_XOR(qr0 + aoff, 64) + t * 2048;  // rows 16 it + n of Q; dO sits TILE bytes behind
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(lds_v8)r0, kf0, sc, 0, 0, 0);
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(lds_v8)r1, kf1, sc, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(lds_v8)(r0 + TILE), vf0, dp, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(lds_v8)(r1 + TILE), vf1, dp, 0, 0, 0);
            const f32x4 l4 = *(lds_f4)(spa + t * 64);
            const f32x4 d4 = *(lds_f4)(spa + t * 64 + ROWS * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float pr = __builtin_amdgcn_exp2f(sc[r] * sl2 - l4[r]);
              if (CAUSAL && kq > it * 16 + r) pr = 0.f;
              pp[t][r] = pr;
              ds[t][r] = pr * (dp[r] - d4[r]);
            }
          }
          const bf16x8 ppk = pack8(pp[0], pp[1]);
          const bf16x8 dsk = pack8(ds[0], ds[1]);
          // dS[query 16 (2a + t) + 4g + r][key row0 + n] -> LDS [query][key]
          {
            const lds_p col = dsw + (a - a0) * (32 * DSROW);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                *(__attribute__((address_space(3))) short*)(col + (t * 16 + r) * DSROW) = dsk[4 * t + r];
          }
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const lds_cp cp = CFHIP_LDS_XOR(qc0 + aoff, dt * 32);  // rows 32 a + 4 g + (n >> 2) of Q (+16: 2 048 bytes on); dO TILE bytes behind
            const s16x4 qlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)cp);
            const s16x4 qhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + 2048));
            const s16x4 olo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + TILE));
            const s16x4 ohi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + TILE + 2048));
            const bf16x8 dof = join8(olo, ohi);
            const bf16x8 qf = join8(qlo, qhi);
            dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof, ppk, dvt[dt], 0, 0, 0);
            dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, dsk, dkt[dt], 0, 0, 0);
          }
        }
      }
      __syncthreads();
      // Q and dO of this head are done with after the second half's phase 1: the NEXT head's stream in behind the last dQ phase
      // (which reads K and dS only); its statistics follow at the end of the head, when the dK / dV accumulators are dead
      if (hf == 1 && nxt < heads) stage_q(nxt);
      // ---- phase 2: dQ of the query tiles of this half, 32 columns per wave, reduction over every key
      if (qt < 2 * (a1 - a0)) {
        f32x4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = {0.f, 0.f, 0.f, 0.f};
        const int a_end = CAUSAL ? min(NB, ((2 * a0 + qt) * 16 + 15) / 32 + 1) : NB;  // keys beyond the tile's last query: dS = 0
        // (phase 2's three pointers are rebuilt per half: kept across phase 1 they push the CAUSAL forms into scratch)
        lds_cp kc2[2], drow = (lds_cp)LDS_PTR(dSs) + (qt * 16 + n) * DSROW + 8 * g;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          kc2[j] = (lds_cp)LDS_PTR(Ks) + tile_off(4 * g + (n >> 2), (2 * ch + j) * 16 + 4 * (n & 3));
          CFHIP_OPAQUE_LDS(kc2[j], lds_cp)
        }
        CFHIP_OPAQUE_LDS(drow, lds_cp)
#pragma unroll 1
        for (int a = 0; a < a_end; ++a) {
          const s16x4 lo = *(lds_cs4)(drow + a * 64);
          const s16x4 hi = *(lds_cs4)(drow + a * 64 + 32);
          const bf16x8 dsp = join8(lo, hi);
          const lds_cp c0 = kc2[0] + a * (32 * 128), c1 = kc2[1] + a * (32 * 128);
          const s16x4 k0l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)c0), k0h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(c0 + 2048));
          const s16x4 k1l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)c1), k1h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(c1 + 2048));
          const bf16x8 kf0c = join8(k0l, k0h);
          const bf16x8 kf1c = join8(k1l, k1h);
          dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0c, dsp, dq0, 0, 0, 0);
          dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1c, dsp, dq1, 0, 0, 0);
        }
        const int qi = (2 * a0 + qt) * 16 + n;
        store_row32(p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * DH, dq0, dq1, p.scale, g, qi < p.Tq, ch);
      }
      __syncthreads();  // the dS buffer (and, after the second half, K) may be overwritten
    }
    if (nxt < heads) stage_k(nxt);
    {
      const int kj = row0 + n;
      const bool valid = kj < p.Tk;
      store_row64(p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dkt, p.scale, g, valid);
      store_row64(p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dvt, 1.0f, g, valid);
    }
    if (nxt < heads) stage_stats(nxt);
  }
}

// ------------------------------------------------------------------------------------------------
// The one-pass backward with TWO key tiles per wave (round 6, late; non-causal, 128 < T <= 224).  The 16-wave form above sits at 13 %
// of the matrix pipe and 26 % of the LDS: at 128 registers per wave hipcc issues the LDS reads of a block two at a time and waits for
// each pair (twelve exposed LDS latencies per 16 MFMAs).  Here a workgroup is 8 waves at 256 registers: a wave owns 32 keys, so every
// Q / dO fragment read from LDS (row form for S and dP, column form for dV and dK) feeds two MFMAs — half the LDS reads per FLOP,
// 32 MFMAs per block — and all fragments of a block are in flight before the first MFMA needs one.  Phase 2: a wave per 16-query tile
// of the half, all 64 columns (four accumulators per dS operand read instead of two).  Same LDS layout, same arithmetic per element
// (the reduction order over queries / keys inside an accumulator is unchanged): results are bit-identical to the 16-wave form.
// ------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(512, 2) void attn_bwd_one2_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(128))) char smem[];  // 128: the XOR-derived addresses below need whole tile rows
  constexpr int PW = 8;
  constexpr int ROWS = NB * 32, TILE = ROWS * 128;
  constexpr int HA = (NB + 1) / 2;          // query pair-tiles per half
  constexpr int DSROW = ROWS * 2 + 16;      // bytes per dS row (ROWS keys, bf16) + 16: rows 4 apart start 16 banks apart
  static_assert(3 * TILE + 2 * ROWS * 4 + HA * 32 * DSROW <= 160 * 1024, "Q + dO + K + statistics + dS must fit the LDS");
  static_assert(NB <= PW && 2 * HA <= PW, "a wave per 32 keys; a wave per query tile of a half");
  char* Qs = smem;
  char* dOs = Qs + TILE;
  char* Ks = dOs + TILE;
  float* lse_s = reinterpret_cast<float*>(Ks + TILE);
  float* delta_s = lse_s + ROWS;
  char* dSs = reinterpret_cast<char*>(delta_s + ROWS);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int heads = p.B * p.H;
  const float sl2 = p.scale * LOG2E;
  const int row0 = wave * 32;  // phase 1: this wave's keys
  const int qt = wave;         // phase 2: query tile of the half

  auto stage_q = [&](int hx) { stage_q_do(Qs, dOs, p, hx, ROWS, wave, PW, lane); };
  // statistics of a head (log-sum-exp in the log2 domain, delta = rowsum(dO o O)): four lanes per row, two sweeps of 128 rows.  The
  // global loads (load_stats) are issued a whole dQ phase before their values are folded and written to the LDS (finish_stats).
  bf16x8 st_a[2][2], st_c[2][2];
  float st_l[2];
  auto load_stats = [&](int hx) {
    const int b = hx / p.H, h = hx - b * p.H;
    const bf16_t* dob = p.d_o + (long)b * p.o_sb + h * DH;
    const bf16_t* ob = p.o_in + (long)b * p.o_sb + h * DH;
    const int part = (int)threadIdx.x & 3;
#pragma unroll
    for (int sw = 0; sw < 2; ++sw) {
      const int t = ((int)threadIdx.x >> 2) + sw * (PW * 16);
      const bool ok = t < p.Tq && !ATTN_ABL(32);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        st_a[sw][j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        st_c[sw][j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) {
          st_a[sw][j] = *reinterpret_cast<const bf16x8*>(dob + (long)t * p.o_st + part * 16 + j * 8);
          st_c[sw][j] = *reinterpret_cast<const bf16x8*>(ob + (long)t * p.o_st + part * 16 + j * 8);
        }
      }
      st_l[sw] = (ok && part == 0) ? p.lse[(long)hx * p.Tq + t] * LOG2E : INFINITY;  // +inf -> p = 0 for padded query rows
    }
  };
  auto finish_stats = [&](int hx) {
    const int part = (int)threadIdx.x & 3;
#pragma unroll
    for (int sw = 0; sw < 2; ++sw) {
      const int t = ((int)threadIdx.x >> 2) + sw * (PW * 16);
      float sacc = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) sacc += bf16_to_f32((bf16_t)st_a[sw][j][e]) * bf16_to_f32((bf16_t)st_c[sw][j][e]);
      sacc += __shfl_xor(sacc, 1, 64);
      sacc += __shfl_xor(sacc, 2, 64);
      if (part == 0 && t < ROWS) {
        lse_s[t] = st_l[sw];
        delta_s[t] = sacc;  // (rows beyond Tq: zero operands)
        if (t < p.Tq && p.delta != nullptr) p.delta[(long)hx * p.Tq + t] = sacc;
      }
    }
  };
  auto stage_k = [&](int hx) { stage_k_tile(Ks, p, hx, ROWS, wave, PW, lane); };

  lds_cp qr0, qc0, sp, drow, kc0;
  lds_p dsw;
  {
    const lds_cp q3 = (lds_cp)LDS_PTR(Qs);
    qr0 = q3 + n * 128 + ((g ^ swz(n)) << 4);
    qc0 = q3 + tile_off(4 * g + (n >> 2), 4 * (n & 3));
    kc0 = qc0 + 2 * TILE;
    sp = (lds_cp)LDS_PTR(lse_s) + 16 * g;
    dsw = (lds_p)LDS_PTR(dSs) + (row0 + n) * 2 + 4 * g * DSROW;
    drow = (lds_cp)LDS_PTR(dSs) + (qt * 16 + n) * DSROW + 8 * g;
    CFHIP_OPAQUE_LDS(qr0, lds_cp)
    CFHIP_OPAQUE_LDS(qc0, lds_cp)
    CFHIP_OPAQUE_LDS(kc0, lds_cp)
    CFHIP_OPAQUE_LDS(sp, lds_cp)
    CFHIP_OPAQUE_LDS(dsw, lds_p)
    CFHIP_OPAQUE_LDS(drow, lds_cp)
  }
  // K / V fragments of this wave's two key tiles (rows beyond Tk are zero): loaded for the NEXT head behind the last phase 1 of a head
  bf16x8 kf[2][2], vf[2][2];
  auto load_kv = [&](int hx) {
    const int b = hx / p.H, h = hx - b * p.H;
    const bf16_t* kb = p.k + (long)b * p.kv_sb + h * DH;
    const bf16_t* vb = p.v + (long)b * p.kv_sb + h * DH;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        kf[kt][ks] = frag_global(kb, p.kv_st, row0 + 16 * kt, ATTN_ABL(128) ? 0 : p.Tk, ks, lane);
        vf[kt][ks] = frag_global(vb, p.kv_st, row0 + 16 * kt, ATTN_ABL(128) ? 0 : p.Tk, ks, lane);
      }
  };
  int hh = blockIdx.x;
  if (hh < heads) {
    stage_q(hh);
    load_kv(hh);
    load_stats(hh);
    finish_stats(hh);
  }
  for (; hh < heads; hh += gridDim.x) {
    const int b = hh / p.H, h = hh - b * p.H;
    const int nxt = hh + gridDim.x;
    // Q, dO and the statistics of this head are in the LDS (staged behind the previous head's last phase 1); the previous head's last
    // dQ phase is over, so its K tile may go: this head's K streams in under phase 1, which takes K from registers
    lds_dma_wait_all();
    __syncthreads();
    if (!ATTN_ABL(256)) stage_k(hh);

    f32x4 dkt[2][4], dvt[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { dkt[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int a0 = hf * HA, a1 = hf == 0 ? HA : NB;
      // ---- phase 1: 32 keys x the query tiles of this half
      if (row0 < ROWS && !ATTN_ABL(8)) {
#pragma unroll 1
        for (int a = a0; a < a1; ++a) {
          const int aoff = a * (32 * 128);
          const lds_cp spa = sp + a * 128;
          bf16x8 qf[2][2], dof[2][2];
          f32x4 l4[2], d4[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const lds_cp r0 = qr0 + aoff + t * 2048, r1 = CFHIP_LDS_XOR(qr0 + aoff, 64) + t * 2048;  // rows 32 a + 16 t + n of Q; dO TILE bytes behind
            qf[t][0] = *(lds_v8)r0;
            qf[t][1] = *(lds_v8)r1;
            dof[t][0] = *(lds_v8)(r0 + TILE);
            dof[t][1] = *(lds_v8)(r1 + TILE);
            l4[t] = *(lds_f4)(spa + t * 64);
            d4[t] = *(lds_f4)(spa + t * 64 + ROWS * 4);
          }
          bf16x8 ppk[2], dsk[2];
          const lds_p col = dsw + (a - a0) * (32 * DSROW);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            f32x4 pp[2], ds[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
              sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[t][0], kf[kt][0], sc, 0, 0, 0);
              sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[t][1], kf[kt][1], sc, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof[t][0], vf[kt][0], dp, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof[t][1], vf[kt][1], dp, 0, 0, 0);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float pr = __builtin_amdgcn_exp2f(sc[r] * sl2 - l4[t][r]);
                pp[t][r] = pr;
                ds[t][r] = pr * (dp[r] - d4[t][r]);
              }
            }
            ppk[kt] = pack8(pp[0], pp[1]);
            dsk[kt] = pack8(ds[0], ds[1]);
            // dS[query 16 (2 (a - a0) + t) + 4g + r][key row0 + 16 kt + n] -> LDS [query][key]
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                *(__attribute__((address_space(3))) short*)(col + kt * 32 + (t * 16 + r) * DSROW) = dsk[kt][4 * t + r];
          }
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const lds_cp cp = CFHIP_LDS_XOR(qc0 + aoff, dt * 32);  // rows 32 a + 4 g + (n >> 2) of Q (+16: 2 048 bytes on); dO TILE bytes behind
            const s16x4 qlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)cp);
            const s16x4 qhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + 2048));
            const s16x4 olo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + TILE));
            const s16x4 ohi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + TILE + 2048));
            const bf16x8 doc = join8(olo, ohi);
            const bf16x8 qcf = join8(qlo, qhi);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
              dvt[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(doc, ppk[kt], dvt[kt][dt], 0, 0, 0);
              dkt[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qcf, dsk[kt], dkt[kt][dt], 0, 0, 0);
            }
          }
        }
      }
      if (hf == 0) {
        lds_dma_wait_all();  // this head's K tile (issued a phase ago)
      } else {
        // dK / dV are complete: out now, behind the dQ phase, not at the end of the head
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const int kj = row0 + 16 * kt + n;
          const bool valid = kj < p.Tk && !ATTN_ABL(64);
          store_row64(p.dk + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dkt[kt], p.scale, g, valid);
          store_row64(p.dv + (long)b * p.kv_sb + (long)kj * p.kv_st + h * DH, dvt[kt], 1.0f, g, valid);
        }
      }
      __syncthreads();
      // Q, dO and the statistics of this head are done with after the second half's phase 1: the NEXT head's stream in behind the last
      // dQ phase — tiles by DMA, the wave's K / V fragments and the statistics' inputs into registers
      if (hf == 1 && nxt < heads) {
        if (!ATTN_ABL(256)) stage_q(nxt);
        load_kv(nxt);
        load_stats(nxt);
      }
      // ---- phase 2: dQ of the query tiles of this half, reduction over every key
      if (qt < 2 * (a1 - a0) && !ATTN_ABL(16)) {
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int a = 0; a < NB; ++a) {
          const s16x4 lo = *(lds_cs4)(drow + a * 64);
          const s16x4 hi = *(lds_cs4)(drow + a * 64 + 32);
          const bf16x8 dsp = join8(lo, hi);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const lds_cp cp = CFHIP_LDS_XOR(kc0 + a * (32 * 128), dt * 32);
            const s16x4 kl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)cp), kh = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(cp + 2048));
            const bf16x8 kcf = join8(kl, kh);
            dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kcf, dsp, dq[dt], 0, 0, 0);
          }
        }
        const int qi = (2 * a0 + qt) * 16 + n;
        store_row64(p.dq + (long)b * p.q_sb + (long)qi * p.q_st + h * DH, dq, p.scale, g, qi < p.Tq);
      }
      if (hf == 0) __syncthreads();  // the dS buffer may be overwritten (after the second half: the barrier at the top of the next head)
    }
    if (nxt < heads) finish_stats(nxt);
  }
}


}  // namespace

int cfhip_attn::launch_one_pass(const Step& st, const AttnParams& p, int pers_ctas, hipStream_t s) {
  const int heads = p.B * p.H;
  switch (st.family) {
    case ONE:
    case ONE2:
      return with_args<2, 3, 4, 5, 6, 7>(st, "attn_bwd", [&](auto NB_, auto, auto CAUSAL) {
        constexpr int NB = NB_(), PW = one_pass_waves(NB);
        const size_t lds = (size_t)3 * NB * 32 * 128 + (size_t)2 * NB * 32 * 4 + (size_t)((NB + 1) / 2) * 32 * (NB * 64 + 16);
        const int ctas = pers_ctas * one_pass_per_cu(NB);
        const dim3 grid(heads < ctas ? heads : ctas);
        if (st.family == ONE2) {
          if constexpr (NB < 5 || CAUSAL()) return no_kernel(st);
          else return launch<attn_bwd_one2_kernel<NB>>(grid, 512, lds, s, "attn_bwd(one pass)", p);
        } else {
          if constexpr (CAUSAL() && (NB < 3 || NB > 5)) return no_kernel(st);
          else return launch<attn_bwd_one_kernel<NB, PW, CAUSAL()>>(grid, PW * 64, lds, s, "attn_bwd(one pass)", p);
        }
      });
    default:
      return no_kernel(st);
  }
}
