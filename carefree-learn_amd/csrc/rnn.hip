// GRU / LSTM recurrence for gfx950 (reference modules/ml/rnn.py:13-17, 53-80, 82-85: single-layer nn.GRU / nn.LSTM, batch_first).
//
// The input projection gx = x W_ih^T + b_ih of all time steps is a GEMM outside this file; what is here is the chain of T dependent
// steps.  Samples are independent, so ONE workgroup (256 threads, 4 waves) owns 16 batch rows for all T steps of one direction and
// loops over time inside the launch: no grid-wide barrier, no cooperative launch, no wait on another workgroup.
//
// Residency: the state lives in LDS for the whole launch (h and c as f32 [16][256], h once more as the bf16 MFMA operand in two
// buffers that alternate per step, so one __syncthreads per step).  W_hh is NOT resident: it is packed once per forward into MFMA
// fragment order (cfhip_rnn_pack; H padded with zeros to Kp = 32-multiples in the reduction and Np = 16-multiples in the width) and
// every step streams the whole pack from L2 with one 16-byte load per lane and fragment: 2 G Np Kp bytes per workgroup and step.
//
// Operation order of one forward step (what the per-element tests derive their bounds from), per row and hidden unit j:
//   a_g  = sum_k bf16(h[k]) * bf16(W_hh[g H + j][k])     one f32 MFMA accumulation chain over Kp / 32 instructions, from 0
//   gh_g = a_g + b_hh[g H + j]                            1 rounding
//   GRU:  r = sig(gx_r + gh_r), z = sig(gx_z + gh_z)      1 add, then sig(x) = rcp(1 + exp2(-x log2 e)): 4 roundings
//         n = tanh(gx_n + r * gh_n)                       1 fma, then tanh(x) = 1 - 2 rcp(1 + exp2(2 x log2 e)): 5 roundings
//         h' = (1 - z) * n + z * h                        1 sub, 1 mul, 1 fma
//   LSTM: i, f, o = sig(gx + gh), g = tanh(gx + gh);  c' = f * c + i * g (1 mul, 1 fma);  h' = o * tanh(c')
// Nothing in a step depends on its index in the launch: T steps in one launch equal T chained launches of one step, bit for bit.
//
// The backward walks the steps in the opposite order.  Per step, thread `col` owns hidden unit col of all 16 rows (dc stays in its
// registers): dh = dy_t + carry;
//   GRU:  dn = dh (1 - z), dz = dh (h_prev - n);  dn' = dn (1 - n^2), dz' = dz z (1 - z), dr' = dn' gh_n r (1 - r)
//         dgx = [dr', dz', dn'], dgh = [dr', dz', dn' r], direct carry = dh z
//   LSTM: tc = tanh(c'), do = dh tc, dc = dc_carry + dh o (1 - tc^2);  di' = dc g i (1 - i), df' = dc c_prev f (1 - f),
//         dg' = dc i (1 - g^2), do' = do o (1 - o);  dc_carry = dc f, direct carry = 0;  dgh = dgx
// dgx / dgh are rounded to bf16 (the operand of the weight-gradient GEMMs and of the carry product alike), then
//   carry = direct + sum_k bf16(dgh[k]) * bf16(W_hh[k][j])   one MFMA chain over G Kp / 32 instructions on the transposed pack.
// The forward saves the gate values in training mode (gates f32 [B T, 4 H]: r, z, n, gh_n or i, f, g, o; LSTM also c' per step);
// the backward recomputes nothing but tanh(c').
#include "common.h"

namespace {

constexpr int RNN_ROWS = 16;
constexpr int RNN_THREADS = 256;
constexpr int RNN_HMAX = CFHIP_RNN_MAX_HIDDEN;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float sig_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x)); }
__device__ __forceinline__ float tanh_f(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((2.0f * LOG2E) * x)); }

struct RnnFwd {
  const float* gx;        // [B T, G H]
  const bf16x8* wp;       // forward pack
  const float* b_hh;      // [G H]
  const float* h0;        // [B, H] or null
  const float* c0;
  float* y;               // row (b T + t) at y + row * ldy
  long ldy;
  float* hT;
  float* cT;
  float* gates;           // [B T, 4 H] or null
  float* cseq;            // [B T, H] or null (LSTM)
  bf16_t* hprev16;        // [B T, H] or null
  long B;
  int T, H, reverse;
};

struct RnnBwd {
  const float* dy;        // row (b T + t) at dy + row * lddy, or null (zero)
  long lddy;
  const float* dhT;
  const float* dcT;
  const bf16x8* wpt;      // transposed pack
  const float* y;
  long ldy;
  const float* h0;
  const float* c0;
  const float* gates;
  const float* cseq;
  bf16_t* dgx;            // [B T, G H]
  bf16_t* dgh;            // [B T, G H] (GRU; the LSTM's is dgx)
  float* dh0;
  float* dc0;
  long B;
  int T, H, reverse;
};

// packed W_hh (f32 [G H, H] -> bf16 fragments).  Forward pack: fragment ((j KC + kk) G + g), lane l holds W[g H + 16 j + (l & 15)][32 kk +
// 8 (l >> 4) + e]; transposed pack (after the forward one): fragment (j G KC + g KC + kk), lane l holds W[g H + 32 kk + 8 (l >> 4) + e]
// [16 j + (l & 15)]; zero outside H.
__global__ __launch_bounds__(256) void rnn_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ out, int G, int H) {
  const int KC = (H + 31) >> 5, NT = (H + 15) >> 4;
  const int per = NT * KC * G * 64;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const bool tr = idx >= per;
  const int f = tr ? idx - per : idx;
  const int lane = f & 63;
  int frag = f >> 6, j, kk, g;
  if (!tr) {
    g = frag % G;
    frag /= G;
    kk = frag % KC;
    j = frag / KC;
  } else {
    kk = frag % KC;
    frag /= KC;
    g = frag % G;
    j = frag / G;
  }
  const int n = j * 16 + (lane & 15), k0 = kk * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float x = 0.f;
    if (n < H && k < H) x = tr ? w[((long)g * H + k) * H + n] : w[((long)g * H + n) * H + k];
    v[e] = x;
  }
  out[idx] = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

template <int G>
__global__ __launch_bounds__(RNN_THREADS) void rnn_fwd_kernel(const RnnFwd a) {
  constexpr bool LSTM = G == 4;
  constexpr int LDB_MAX = RNN_HMAX + 8;
  __shared__ float hf[RNN_ROWS * RNN_HMAX];
  __shared__ float cf[LSTM ? RNN_ROWS * RNN_HMAX : 1];
  __shared__ __attribute__((aligned(16))) bf16_t hb[2][RNN_ROWS * LDB_MAX];
  const int H = a.H, T = a.T, Kp = (H + 31) & ~31, NT = (H + 15) >> 4, KC = Kp >> 5, ldb = Kp + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)blockIdx.x * RNN_ROWS;
  const int nrows = (int)min((long)RNN_ROWS, a.B - row0);
  for (int idx = tid; idx < RNN_ROWS * Kp; idx += RNN_THREADS) {
    const int r = idx / Kp, c = idx - r * Kp;
    float h = 0.f, cc = 0.f;
    if (r < nrows && c < H) {
      if (a.h0) h = a.h0[(row0 + r) * H + c];
      if (LSTM && a.c0) cc = a.c0[(row0 + r) * H + c];
    }
    hf[r * RNN_HMAX + c] = h;
    if (LSTM) cf[r * RNN_HMAX + c] = cc;
    hb[0][r * ldb + c] = f32_to_bf16(h);
    hb[1][r * ldb + c] = 0;
  }
  __syncthreads();
  const int lr = lane & 15, lq = lane >> 4;
  for (int s = 0; s < T; ++s) {
    const int t = a.reverse ? T - 1 - s : s;
    const bf16_t* cur = hb[s & 1];
    bf16_t* nxt = hb[(s & 1) ^ 1];
    if (a.hprev16) {
      for (int idx = tid; idx < nrows * H; idx += RNN_THREADS) {
        const int r = idx / H, c = idx - r * H;
        a.hprev16[((row0 + r) * T + t) * H + c] = cur[r * ldb + c];
      }
    }
    for (int j = wave; j < NT; j += RNN_THREADS / 64) {
      f32x4 acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16x8* wj = a.wp + (long)j * KC * G * 64 + lane;
      for (int kk = 0; kk < KC; ++kk) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(cur + lr * ldb + kk * 32 + lq * 8);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wj[(kk * G + g) * 64], acc[g], 0, 0, 0);
      }
      const int col = j * 16 + lr;
      if (col < H) {
        float bh[G];
#pragma unroll
        for (int g = 0; g < G; ++g) bh[g] = a.b_hh[g * H + col];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = lq * 4 + i;
          if (r < nrows) {
            const long grow = (row0 + r) * T + t;
            const float* gxp = a.gx + grow * (G * H) + col;
            float hnew;
            if (!LSTM) {
              const float ghr = acc[0][i] + bh[0], ghz = acc[1][i] + bh[1], ghn = acc[2][i] + bh[2];
              const float rg = sig_f(gxp[0] + ghr), zg = sig_f(gxp[H] + ghz);
              const float ng = tanh_f(fmaf(rg, ghn, gxp[2 * H]));
              hnew = fmaf(zg, hf[r * RNN_HMAX + col], (1.0f - zg) * ng);
              if (a.gates) {
                float* gp = a.gates + grow * (4 * H) + col;
                gp[0] = rg;
                gp[H] = zg;
                gp[2 * H] = ng;
                gp[3 * H] = ghn;
              }
            } else {
              const float ig = sig_f(gxp[0] + (acc[0][i] + bh[0])), fg = sig_f(gxp[H] + (acc[1][i] + bh[1]));
              const float gg = tanh_f(gxp[2 * H] + (acc[2][i] + bh[2])), og = sig_f(gxp[3 * H] + (acc[3][i] + bh[3]));
              const float cnew = fmaf(fg, cf[r * RNN_HMAX + col], ig * gg);
              cf[r * RNN_HMAX + col] = cnew;
              hnew = og * tanh_f(cnew);
              if (a.gates) {
                float* gp = a.gates + grow * (4 * H) + col;
                gp[0] = ig;
                gp[H] = fg;
                gp[2 * H] = gg;
                gp[3 * H] = og;
              }
              if (a.cseq) a.cseq[grow * H + col] = cnew;
            }
            hf[r * RNN_HMAX + col] = hnew;
            nxt[r * ldb + col] = f32_to_bf16(hnew);
            a.y[grow * a.ldy + col] = hnew;
          }
        }
      }
    }
    __syncthreads();
  }
  if (a.hT || (LSTM && a.cT)) {
    for (int idx = tid; idx < nrows * H; idx += RNN_THREADS) {
      const int r = idx / H, c = idx - r * H;
      if (a.hT) a.hT[(row0 + r) * H + c] = hf[r * RNN_HMAX + c];
      if (LSTM && a.cT) a.cT[(row0 + r) * H + c] = cf[r * RNN_HMAX + c];
    }
  }
}

template <int G>
__global__ __launch_bounds__(RNN_THREADS) void rnn_bwd_kernel(const RnnBwd a) {
  constexpr bool LSTM = G == 4;
  constexpr int LDA_MAX = G * RNN_HMAX + 8;
  __shared__ float carry[RNN_ROWS * RNN_HMAX];
  __shared__ __attribute__((aligned(16))) bf16_t at[RNN_ROWS * LDA_MAX];
  const int H = a.H, T = a.T, Kp = (H + 31) & ~31, NT = (H + 15) >> 4, KC = Kp >> 5, lda = G * Kp + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)blockIdx.x * RNN_ROWS;
  const int nrows = (int)min((long)RNN_ROWS, a.B - row0);
  for (int idx = tid; idx < RNN_ROWS * lda; idx += RNN_THREADS) at[idx] = 0;
  const int col = tid;  // the hidden unit this thread owns in the gate phase
  float dc[RNN_ROWS];
#pragma unroll
  for (int r = 0; r < RNN_ROWS; ++r) {
    float dh = 0.f;
    dc[r] = 0.f;
    if (r < nrows && col < H) {
      if (a.dhT) dh = a.dhT[(row0 + r) * H + col];
      if (LSTM && a.dcT) dc[r] = a.dcT[(row0 + r) * H + col];
    }
    carry[r * RNN_HMAX + col] = dh;
  }
  __syncthreads();
  const int lr = lane & 15, lq = lane >> 4;
  for (int sb = 0; sb < T; ++sb) {
    const int sf = T - 1 - sb;                       // the forward step this undoes
    const int t = a.reverse ? T - 1 - sf : sf;
    const int tp = a.reverse ? t + 1 : t - 1;        // the time of the forward's previous step (sf > 0)
    if (col < H) {
#pragma unroll
      for (int r = 0; r < RNN_ROWS; ++r) {
        if (r < nrows) {
          const long b = row0 + r, grow = b * T + t;
          float dh = carry[r * RNN_HMAX + col];
          if (a.dy) dh = a.dy[grow * a.lddy + col] + dh;
          const float* gp = a.gates + grow * (4 * H) + col;
          float d[G], direct;
          if (!LSTM) {
            const float rg = gp[0], zg = gp[H], ng = gp[2 * H], ghn = gp[3 * H];
            float hprev = 0.f;
            if (sf > 0) hprev = a.y[(b * T + tp) * a.ldy + col];
            else if (a.h0) hprev = a.h0[b * H + col];
            const float dn = dh * (1.0f - zg), dz = dh * (hprev - ng);
            const float dnp = dn * (1.0f - ng * ng), dzp = dz * zg * (1.0f - zg), drp = dnp * ghn * rg * (1.0f - rg);
            d[0] = drp;
            d[1] = dzp;
            d[2] = dnp * rg;
            direct = dh * zg;
            bf16_t* gxo = a.dgx + grow * (G * H) + col;
            gxo[0] = f32_to_bf16(drp);
            gxo[H] = f32_to_bf16(dzp);
            gxo[2 * H] = f32_to_bf16(dnp);
            bf16_t* gho = a.dgh + grow * (G * H) + col;
#pragma unroll
            for (int g = 0; g < G; ++g) gho[g * H] = f32_to_bf16(d[g]);
          } else {
            const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
            float cprev = 0.f;
            if (sf > 0) cprev = a.cseq[(b * T + tp) * H + col];
            else if (a.c0) cprev = a.c0[b * H + col];
            const float tc = tanh_f(a.cseq[grow * H + col]);
            const float dout = dh * tc;
            const float dcc = fmaf(dh * og, 1.0f - tc * tc, dc[r]);
            d[0] = dcc * gg * ig * (1.0f - ig);
            d[1] = dcc * cprev * fg * (1.0f - fg);
            d[2] = dcc * ig * (1.0f - gg * gg);
            d[3] = dout * og * (1.0f - og);
            dc[r] = dcc * fg;
            direct = 0.f;
            bf16_t* gxo = a.dgx + grow * (G * H) + col;
#pragma unroll
            for (int g = 0; g < G; ++g) gxo[g * H] = f32_to_bf16(d[g]);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) at[r * lda + g * Kp + col] = f32_to_bf16(d[g]);
          carry[r * RNN_HMAX + col] = direct;
        }
      }
    }
    __syncthreads();
    for (int j = wave; j < NT; j += RNN_THREADS / 64) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16x8* wj = a.wpt + (long)j * (G * KC) * 64 + lane;
      for (int kq = 0; kq < G * KC; ++kq) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(at + lr * lda + kq * 32 + lq * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wj[kq * 64], acc, 0, 0, 0);
      }
      const int c = j * 16 + lr;
      if (c < H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = lq * 4 + i;
          if (r < nrows) carry[r * RNN_HMAX + c] += acc[i];
        }
      }
    }
    __syncthreads();
  }
  if (col < H) {
#pragma unroll
    for (int r = 0; r < RNN_ROWS; ++r) {
      if (r < nrows) {
        if (a.dh0) a.dh0[(row0 + r) * H + col] = carry[r * RNN_HMAX + col];
        if (LSTM && a.dc0) a.dc0[(row0 + r) * H + col] = dc[r];
      }
    }
  }
}

bool rnn_shape_ok(int cell, int64_t B, int T, int H, const char* who) {
  if (cell != CFHIP_RNN_GRU && cell != CFHIP_RNN_LSTM) {
    cfhip_set_error("%s: unknown cell id %d (0 = GRU, 1 = LSTM)", who, cell);
    return false;
  }
  if (H < 8 || H > RNN_HMAX || H % 8 != 0) {
    cfhip_set_error("%s: H = %d is outside the recurrent kernels (H %% 8 == 0, 8 <= H <= %d)", who, H, RNN_HMAX);
    return false;
  }
  if (B < 1 || T < 1 || (B + RNN_ROWS - 1) / RNN_ROWS > 0x7fffffffLL) {
    cfhip_set_error("%s: B = %lld, T = %d", who, (long long)B, T);
    return false;
  }
  return true;
}

}  // namespace

// bytes of the two packs of one W_hh (0 for a shape the kernels refuse)
extern "C" size_t cfhip_rnn_pack_workspace(int cell, int H) {
  if (cell != CFHIP_RNN_GRU && cell != CFHIP_RNN_LSTM) return 0;
  if (H < 8 || H > RNN_HMAX || H % 8 != 0) return 0;
  const size_t G = cell == CFHIP_RNN_GRU ? 3 : 4;
  return 2 * sizeof(bf16_t) * G * ((H + 15) / 16 * 16) * ((H + 31) / 32 * 32);
}

extern "C" int cfhip_rnn_pack(const float* w_hh, void* packed, size_t packed_bytes, int cell, int H, void* stream) {
  if (!rnn_shape_ok(cell, 1, 1, H, "rnn_pack")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(w_hh && packed, "rnn_pack: null operand");
  CFHIP_REQUIRE(packed_bytes == cfhip_rnn_pack_workspace(cell, H), "rnn_pack: `packed` holds %zu bytes, cfhip_rnn_pack_workspace says %zu",
                packed_bytes, cfhip_rnn_pack_workspace(cell, H));
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)w_hh & 3) == 0, "rnn_pack: misaligned operand");
  const int G = cell == CFHIP_RNN_GRU ? 3 : 4;
  const int lanes = (int)(packed_bytes / 16);
  hipLaunchKernelGGL(rnn_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_hh,
                     reinterpret_cast<u32x4*>(packed), G, H);
  CFHIP_CHECK_LAUNCH("rnn_pack");
  return CFHIP_OK;
}

extern "C" int cfhip_rnn_fwd(const float* gx, const void* packed, const float* b_hh, const float* h0, const float* c0, float* y,
                             int64_t ldy, float* hT, float* cT, float* gates, float* cseq, void* hprev16, int cell, int64_t B, int T,
                             int H, int reverse, void* stream) {
  if (!rnn_shape_ok(cell, B, T, H, "rnn_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(gx && packed && b_hh && y, "rnn_fwd: null operand (gx, packed, b_hh and y are required)");
  CFHIP_REQUIRE(ldy >= H, "rnn_fwd: output row stride %lld is smaller than H = %d", (long long)ldy, H);
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0, "rnn_fwd: `packed` must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)gx | (uintptr_t)b_hh | (uintptr_t)h0 | (uintptr_t)c0 | (uintptr_t)y | (uintptr_t)hT | (uintptr_t)cT |
                  (uintptr_t)gates | (uintptr_t)cseq) & 3) == 0 && ((uintptr_t)hprev16 & 1) == 0, "rnn_fwd: misaligned operand");
  const bool lstm = cell == CFHIP_RNN_LSTM;
  CFHIP_REQUIRE(lstm || (!c0 && !cT && !cseq), "rnn_fwd: c0 / cT / cseq belong to the LSTM");
  CFHIP_REQUIRE(!lstm || !gates || cseq, "rnn_fwd: an LSTM that saves its gates saves its cell states too");
  RnnFwd a{gx, reinterpret_cast<const bf16x8*>(packed), b_hh, h0, c0, y, (long)ldy, hT, cT, gates, cseq,
           reinterpret_cast<bf16_t*>(hprev16), (long)B, T, H, reverse != 0};
  const dim3 grid((unsigned)((B + RNN_ROWS - 1) / RNN_ROWS));
  if (lstm) hipLaunchKernelGGL(rnn_fwd_kernel<4>, grid, dim3(RNN_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rnn_fwd_kernel<3>, grid, dim3(RNN_THREADS), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("rnn_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_rnn_bwd(const float* dy, int64_t lddy, const float* dhT, const float* dcT, const void* packed, const float* y,
                             int64_t ldy, const float* h0, const float* c0, const float* gates, const float* cseq, void* dgx, void* dgh,
                             float* dh0, float* dc0, int cell, int64_t B, int T, int H, int reverse, void* stream) {
  if (!rnn_shape_ok(cell, B, T, H, "rnn_bwd")) return CFHIP_ERR_INVALID;
  const bool lstm = cell == CFHIP_RNN_LSTM;
  CFHIP_REQUIRE(packed && gates && dgx, "rnn_bwd: null operand (packed, gates and dgx are required)");
  CFHIP_REQUIRE(lstm ? cseq != nullptr : dgh != nullptr, "rnn_bwd: the %s", lstm ? "LSTM needs cseq" : "GRU needs dgh");
  CFHIP_REQUIRE(lstm || (y != nullptr && ldy >= H) || T == 1, "rnn_bwd: the GRU reads h_{t-1} from y (row stride %lld, H = %d)",
                (long long)ldy, H);
  CFHIP_REQUIRE(dy == nullptr || lddy >= H, "rnn_bwd: gradient row stride %lld is smaller than H = %d", (long long)lddy, H);
  CFHIP_REQUIRE(lstm || (!c0 && !dcT && !dc0), "rnn_bwd: c0 / dcT / dc0 belong to the LSTM");
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0, "rnn_bwd: `packed` must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)dhT | (uintptr_t)dcT | (uintptr_t)y | (uintptr_t)h0 | (uintptr_t)c0 | (uintptr_t)gates |
                  (uintptr_t)cseq | (uintptr_t)dh0 | (uintptr_t)dc0) & 3) == 0 && (((uintptr_t)dgx | (uintptr_t)dgh) & 1) == 0,
                "rnn_bwd: misaligned operand");
  const size_t fwd_elems = cfhip_rnn_pack_workspace(cell, H) / 4;
  RnnBwd a{dy, (long)lddy, dhT, dcT, reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(packed) + fwd_elems), y, (long)ldy,
           h0, c0, gates, cseq, reinterpret_cast<bf16_t*>(dgx), reinterpret_cast<bf16_t*>(dgh), dh0, dc0, (long)B, T, H, reverse != 0};
  const dim3 grid((unsigned)((B + RNN_ROWS - 1) / RNN_ROWS));
  if (lstm) hipLaunchKernelGGL(rnn_bwd_kernel<4>, grid, dim3(RNN_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rnn_bwd_kernel<3>, grid, dim3(RNN_THREADS), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("rnn_bwd");
  return CFHIP_OK;
}
