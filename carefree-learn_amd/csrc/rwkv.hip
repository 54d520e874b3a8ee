// RWKV mixers for gfx950: the time shift and mixes, the WKV scan and the gates of reference mixed_stacks/token_mixers.py:107-206 and
// mixed_stacks/channel_mixers.py:69-113.  include/cfhip.h states the C-ABI; this file states the f32 operation order.
//
// The WKV scan.  The reference computes wk = conv1d(pad(exp(k)), exp_w) and wkv = conv1d(pad(exp(k) v / (wk + 1e-6)), exp_w) with
// T-tap kernels exp_w[c][j] = lam_c^(T-1-j): O(T^2) per channel.  Both are first-order recurrences,
//     a[t] = lam a[t-1] + e[t],   b[t] = lam b[t-1] + n[t],   e = exp(k),  n = e v / (a + 1e-6),  lam = exp(-exp(info_decay)).
// Layout [B][T][L]: lane = channel (64 consecutive channels of one sample per wave: every load and store of a wave is one
// contiguous row segment), time runs in registers.  Time is cut into chunks of TC = CFHIP_RWKV_CHUNK steps at fixed positions
// (chunk j = steps [j TC, (j+1) TC)); the W waves of a workgroup take W consecutive chunks per pass.  A recurrence s[t] = lam s[t-1] + u[t]
// is affine in its state, so inside chunk j, with carry = s[j TC - 1],
//     s[t] = fma(lam^(i+1), carry, local[i]),   local[i] = fma(lam, local[i-1], u[t]),  local[-1] = 0,   i = t - j TC,
// lam^(i+1) by i multiplications by lam, and the carries run chunk by chunk:  carry(j+1) = fma(lam^TC, carry(j), local[TC-1] of j).
// Each wave posts its last local value in LDS and walks the chunks before its own from the pass's incoming carry, so the VALUE of
// every carry is the same chain of fmas whatever W is: the result's bits depend on TC alone (a compile-time constant), not on the
// launch.  b needs the finished a, hence two carry rounds (two barriers) per pass.  All loads of a chunk (3 TC per lane forward,
// 6 TC + 2 backward) are issued before the first dependent fma.
//
// Backward, given dy (g = dy sigmoid(r), q = 1 / (a + 1e-6)); the same chunking, walked from the last chunk to the first:
//     G[t] = g[t] + lam G[t+1];   da[t] = -G[t] n[t] q[t];   H[t] = da[t] + lam H[t+1];
//     dv = G e q;   dk = (G v q + H) e;   dr = dy b s (1 - s), with 1 - s = exp(-r) s (no cancellation);
//     dlam = sum_{b, t >= 1} (G[t] b[t-1] + H[t] a[t-1]):  per chunk from the last step down, the chunks of a sample from the last
//     down (one partial per workgroup), then over the samples in order;  d info_decay = dlam * (-(lam exp(info_decay))).
// exp is expf (<= 1 ulp), divisions are IEEE: the error model of DESIGN §3.18 counts on it.  No floating-point atomics.
#include "common.h"

namespace {

constexpr int TC = CFHIP_RWKV_CHUNK;
constexpr int WMAX = CFHIP_RWKV_MAX_WAVES;
constexpr float WKV_EPS = 1.0e-6f;

__device__ __forceinline__ void st_act(void* p, long i, bool f32, float v) {
  if (f32) reinterpret_cast<float*>(p)[i] = v;
  else reinterpret_cast<bf16_t*>(p)[i] = f32_to_bf16(v);
}

// ---- time shift + mixes --------------------------------------------------------------------------------------------------------

// thread = one element of x; rows = B T
__global__ __launch_bounds__(256) void time_mix_fwd_kernel(const void* __restrict__ x, int x_f32, const float* __restrict__ mk,
                                                           const float* __restrict__ mv, const float* __restrict__ mr,
                                                           bf16_t* __restrict__ ok, bf16_t* __restrict__ ov, bf16_t* __restrict__ orr,
                                                           long rows, int T, int C) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const long row = blockIdx.x;
  if (c >= C || row >= rows) return;
  const long at = row * C + c;
  const float xv = ld_act(x, at, x_f32 != 0);
  const float xp = (row % T) > 0 ? ld_act(x, at - C, x_f32 != 0) : 0.f;
  const float m0 = mk[c], m2 = mr[c];
  ok[at] = f32_to_bf16(fmaf(xv, m0, xp * (1.0f - m0)));
  if (mv) {
    const float m1 = mv[c];
    ov[at] = f32_to_bf16(fmaf(xv, m1, xp * (1.0f - m1)));
  }
  orr[at] = f32_to_bf16(fmaf(xv, m2, xp * (1.0f - m2)));
}

// thread = channel c of row chunk blockIdx.y: walks its rows in order.  dx = ((((dk m_k + dk' (1-m_k)) + dv m_v) + dv' (1-m_v)) ...
// as one fma chain in the order k, k', v, v', r, r' (' = row t+1 of the same sample); partial of dm_j = fma chain of d_j (x - x').
__global__ __launch_bounds__(256) void time_mix_bwd_kernel(const void* __restrict__ dk, const void* __restrict__ dv,
                                                           const void* __restrict__ dr, int d_f32, const void* __restrict__ x, int x_f32,
                                                           const float* __restrict__ mk, const float* __restrict__ mv,
                                                           const float* __restrict__ mr, void* __restrict__ dx, int want,
                                                           float* __restrict__ part, long rows, int T, int C, long per_chunk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const long r0 = (long)blockIdx.y * per_chunk, r1 = min(rows, r0 + per_chunk);
  const bool f32 = x_f32 != 0, df = d_f32 != 0;
  const float m0 = mk[c], m1 = mv ? mv[c] : 0.f, m2 = mr[c];
  const float n0 = 1.0f - m0, n1 = 1.0f - m1, n2 = 1.0f - m2;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (long row = r0; row < r1; ++row) {
    const long at = row * C + c;
    const int t = (int)(row % T);
    const float a0 = ld_act(dk, at, df), a2 = ld_act(dr, at, df);
    const float a1 = dv ? ld_act(dv, at, df) : 0.f;
    if (dx) {
      const bool nx = t + 1 < T;
      float s = a0 * m0;
      if (nx) s = fmaf(ld_act(dk, at + C, df), n0, s);
      if (dv) {
        s = fmaf(a1, m1, s);
        if (nx) s = fmaf(ld_act(dv, at + C, df), n1, s);
      }
      s = fmaf(a2, m2, s);
      if (nx) s = fmaf(ld_act(dr, at + C, df), n2, s);
      st_act(dx, at, f32, s);
    }
    if (want) {
      const float diff = ld_act(x, at, f32) - (t > 0 ? ld_act(x, at - C, f32) : 0.f);
      if (want & 1) s0 = fmaf(a0, diff, s0);
      if (want & 2) s1 = fmaf(a1, diff, s1);
      if (want & 4) s2 = fmaf(a2, diff, s2);
    }
  }
  if (want) {
    float* rec = part + (long)blockIdx.y * 3 * C;
    rec[c] = s0;
    rec[C + c] = s1;
    rec[2 * C + c] = s2;
  }
}

// thread = channel c of mix j: the chunks in order
__global__ __launch_bounds__(256) void time_mix_reduce_kernel(const float* __restrict__ part, float* __restrict__ d0, float* __restrict__ d1,
                                                              float* __restrict__ d2, int accumulate, int chunks, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  float* dst = j == 0 ? d0 : j == 1 ? d1 : d2;
  if (c >= C || !dst) return;
  float s = 0.f;
  for (int i = 0; i < chunks; ++i) s += part[((long)i * 3 + j) * C + c];
  dst[c] = ((accumulate >> j) & 1) ? dst[c] + s : s;
}

// ---- the WKV scan ----------------------------------------------------------------------------------------------------------------

// lam^(i+1), i < TC, by repeated multiplication
__device__ __forceinline__ void lam_powers(float lam, float (&p)[TC]) {
  p[0] = lam;
#pragma unroll
  for (int i = 1; i < TC; ++i) p[i] = p[i - 1] * lam;
}

template <bool SAVE>
__global__ __launch_bounds__(64 * WMAX) void wkv_fwd_kernel(const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ r,
                                                            const float* __restrict__ decay, bf16_t* __restrict__ y, float* __restrict__ sa,
                                                            float* __restrict__ sb, int T, int L) {
  __shared__ float post[2][WMAX][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool live = c < L;
  const long base = (long)blockIdx.y * T * L + (live ? c : L - 1);  // a lane past L reads channel L - 1 and stores nothing
  const float lam = expf(-expf(decay[live ? c : L - 1]));
  float p[TC];
  lam_powers(lam, p);
  const float pT = p[TC - 1];
  float ga = 0.f, gb = 0.f;  // a, b at the step before this pass
  for (int g0 = 0; g0 < T; g0 += W * TC) {
    const int t0 = g0 + w * TC;
    float e[TC], vv[TC], rr[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      const long at = base + (long)min(t0 + i, T - 1) * L;  // a step past T reads step T - 1 and counts as zero
      e[i] = k[at];
      vv[i] = v[at];
      rr[i] = r[at];
    }
    float la[TC], s = 0.f;
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      e[i] = t0 + i < T ? expf(e[i]) : 0.f;
      s = fmaf(lam, s, e[i]);
      la[i] = s;
    }
    post[0][w][lane] = s;
    __syncthreads();
    float ca = ga;
    for (int j = 0; j < w; ++j) ca = fmaf(pT, ca, post[0][j][lane]);
    ga = ca;
    for (int j = w; j < W; ++j) ga = fmaf(pT, ga, post[0][j][lane]);
    float lb[TC];
    s = 0.f;
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      la[i] = fmaf(p[i], ca, la[i]);
      const float n = e[i] * vv[i] / (la[i] + WKV_EPS);
      s = fmaf(lam, s, n);
      lb[i] = s;
    }
    post[1][w][lane] = s;
    __syncthreads();
    float cb = gb;
    for (int j = 0; j < w; ++j) cb = fmaf(pT, cb, post[1][j][lane]);
    gb = cb;
    for (int j = w; j < W; ++j) gb = fmaf(pT, gb, post[1][j][lane]);
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      if (live && t0 + i < T) {
        const long at = base + (long)(t0 + i) * L;
        const float b = fmaf(p[i], cb, lb[i]);
        const float sig = 1.0f / (1.0f + expf(-rr[i]));
        y[at] = f32_to_bf16(sig * b);
        if (SAVE) {
          sa[at] = la[i];
          sb[at] = b;
        }
      }
    }
  }
}

__global__ __launch_bounds__(64 * WMAX) void wkv_bwd_kernel(const void* __restrict__ dy, int dy_f32, const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ r, const float* __restrict__ decay,
                                                            const float* __restrict__ sa, const float* __restrict__ sb, bf16_t* __restrict__ dk,
                                                            bf16_t* __restrict__ dv, bf16_t* __restrict__ dr, float* __restrict__ part, int T, int L) {
  __shared__ float post[3][WMAX][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool live = c < L;
  const long base = (long)blockIdx.y * T * L + (live ? c : L - 1);
  const float lam = expf(-expf(decay[live ? c : L - 1]));
  float p[TC];
  lam_powers(lam, p);
  const float pT = p[TC - 1];
  const int span = W * TC;
  float gG = 0.f, gH = 0.f, dl = 0.f;  // G, H at the step after this pass; the running sum of dlam
  for (int g0 = (T - 1) / span * span; g0 >= 0; g0 -= span) {
    const int t0 = g0 + w * TC;
    float e[TC], vv[TC], sg[TC], om[TC], dyv[TC], av[TC], bv[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      const long at = base + (long)min(t0 + i, T - 1) * L;
      e[i] = k[at];
      vv[i] = v[at];
      sg[i] = r[at];
      dyv[i] = ld_act(dy, at, dy_f32 != 0);
      av[i] = sa[at];
      bv[i] = sb[at];
    }
    const long prev = base + (long)min(max(t0 - 1, 0), T - 1) * L;
    const float ap = sa[prev], bp = sb[prev];  // a, b at t0 - 1 (used for t0 >= 1 only)
    float lg[TC], s = 0.f;
#pragma unroll
    for (int i = TC - 1; i >= 0; --i) {
      const bool on = t0 + i < T;
      const float x = expf(-sg[i]);
      sg[i] = 1.0f / (1.0f + x);
      om[i] = x * sg[i];
      e[i] = on ? expf(e[i]) : 0.f;
      s = fmaf(lam, s, on ? dyv[i] * sg[i] : 0.f);
      lg[i] = s;
    }
    post[0][w][lane] = s;
    __syncthreads();
    float cg = gG;
    for (int j = W - 1; j > w; --j) cg = fmaf(pT, cg, post[0][j][lane]);
    gG = cg;
    for (int j = w; j >= 0; --j) gG = fmaf(pT, gG, post[0][j][lane]);
    float lh[TC], q[TC];
    s = 0.f;
#pragma unroll
    for (int i = TC - 1; i >= 0; --i) {
      lg[i] = fmaf(p[TC - 1 - i], cg, lg[i]);  // G[t]
      q[i] = 1.0f / (av[i] + WKV_EPS);
      const float n = e[i] * vv[i] * q[i];
      s = fmaf(lam, s, -(lg[i] * n) * q[i]);
      lh[i] = s;
    }
    post[1][w][lane] = s;
    __syncthreads();
    float ch = gH;
    for (int j = W - 1; j > w; --j) ch = fmaf(pT, ch, post[1][j][lane]);
    gH = ch;
    for (int j = w; j >= 0; --j) gH = fmaf(pT, gH, post[1][j][lane]);
    float dls = 0.f;
#pragma unroll
    for (int i = TC - 1; i >= 0; --i) {
      const int t = t0 + i;
      const float h = fmaf(p[TC - 1 - i], ch, lh[i]);  // H[t]
      if (t < T) {
        if (live) {
          const long at = base + (long)t * L;
          dv[at] = f32_to_bf16(lg[i] * e[i] * q[i]);
          dk[at] = f32_to_bf16(fmaf(lg[i] * vv[i], q[i], h) * e[i]);
          dr[at] = f32_to_bf16(dyv[i] * bv[i] * (sg[i] * om[i]));
        }
        if (part && t >= 1) dls += fmaf(lg[i], i > 0 ? bv[i ? i - 1 : 0] : bp, h * (i > 0 ? av[i ? i - 1 : 0] : ap));
      }
    }
    if (part) {  // (uniform over the workgroup)
      post[2][w][lane] = dls;
      __syncthreads();
      for (int j = W - 1; j >= 0; --j) dl += post[2][j][lane];
    }
  }
  if (part && w == 0 && live) part[(long)blockIdx.y * L + c] = dl;
}

// thread = channel: the samples in order, then the factor d lam / d info_decay = -(lam exp(info_decay))
__global__ __launch_bounds__(256) void wkv_decay_reduce_kernel(const float* __restrict__ part, const float* __restrict__ decay,
                                                               float* __restrict__ dst, int accumulate, long B, int L) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= L) return;
  float s = 0.f;
  for (long b = 0; b < B; ++b) s += part[b * L + c];
  const float ew = expf(decay[c]);
  const float val = __fmul_rn(s, -(expf(-ew) * ew));  // (its own rounding: an accumulated result is the written one added)
  dst[c] = accumulate ? dst[c] + val : val;
}

// ---- the channel mixer's elementwise kernels ---------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void relu2_fwd_kernel(const void* __restrict__ h, int h_f32, bf16_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = fmaxf(ld_act(h, i, h_f32 != 0), 0.f);
  out[i] = f32_to_bf16(x * x);
}

__global__ __launch_bounds__(256) void relu2_bwd_kernel(const void* __restrict__ d, int d_f32, const void* __restrict__ h, int h_f32,
                                                        bf16_t* __restrict__ dh, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = fmaxf(ld_act(h, i, h_f32 != 0), 0.f);
  dh[i] = f32_to_bf16((x + x) * ld_act(d, i, d_f32 != 0));
}

__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ r, const float* __restrict__ kv, const void* __restrict__ res,
                                                       int res_f32, void* __restrict__ out, int out_f32, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float s = 1.0f / (1.0f + expf(-r[i]));
  float o = s * kv[i];
  if (res) o += ld_act(res, i, res_f32 != 0);
  st_act(out, i, out_f32 != 0, o);
}

__global__ __launch_bounds__(256) void gate_bwd_kernel(const void* __restrict__ d, int d_f32, const float* __restrict__ r,
                                                       const float* __restrict__ kv, bf16_t* __restrict__ dr, bf16_t* __restrict__ dkv, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = expf(-r[i]);
  const float s = 1.0f / (1.0f + x);
  const float g = ld_act(d, i, d_f32 != 0);
  dr[i] = f32_to_bf16(g * kv[i] * (s * (x * s)));
  dkv[i] = f32_to_bf16(g * s);
}

constexpr int64_t RWKV_MAX_ELEMS = (int64_t)1 << 38;  // (256 per workgroup: below the 2^31 workgroups of a grid's x)
constexpr int TM_MAX_CHUNKS = 2048;

bool rwkv_shape_ok(int64_t B, int T, int C, const char* who, const char* cname) {
  if (B < 1 || T < 1 || C < 1 || B > RWKV_MAX_ELEMS / T / C || B * T > 0x7fffffffLL) {
    cfhip_set_error("%s: B = %lld, T = %d, %s = %d (each >= 1, B T below 2^31, B T %s below 2^38)", who, (long long)B, T, cname, C, cname);
    return false;
  }
  return true;
}

// rows per chunk and chunks of the time-mix backward: enough workgroups to fill the chip, at most TM_MAX_CHUNKS partial records
void time_mix_chunks(int64_t rows, int C, long* per_chunk, int* chunks) {
  const int64_t col_groups = (C + 255) / 256;
  int64_t want = TM_MAX_CHUNKS / col_groups;
  if (want < 1) want = 1;
  if (want > rows) want = rows;
  *per_chunk = (long)((rows + want - 1) / want);
  *chunks = (int)((rows + *per_chunk - 1) / *per_chunk);
}

int wkv_waves(int64_t B, int T, int L, int waves) {
  const int chunks = (T + TC - 1) / TC;
  int w = waves;
  if (w == 0) w = B * ((L + 63) / 64) >= 1024 ? 4 : WMAX;  // enough workgroups: fewer barriers' worth of waiting per workgroup
  return w < chunks ? w : chunks;
}

bool aligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 3) == 0;
}

}  // namespace

extern "C" int cfhip_rwkv_time_mix_fwd(const void* x, int x_f32, const float* mk, const float* mv, const float* mr, void* out_k, void* out_v,
                                       void* out_r, int64_t B, int T, int C, void* stream) {
  if (!rwkv_shape_ok(B, T, C, "rwkv_time_mix_fwd", "C")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(x && mk && mr && out_k && out_r && (!mv == !out_v), "rwkv_time_mix_fwd: null operand (x, mk, mr, out_k, out_r; mv and out_v together)");
  CFHIP_REQUIRE(aligned4(mk, mv, mr) && (((uintptr_t)x | (uintptr_t)out_k | (uintptr_t)out_v | (uintptr_t)out_r) & 1) == 0 &&
                    (!x_f32 || aligned4(x)), "rwkv_time_mix_fwd: misaligned operand");
  const int64_t rows = B * T;
  hipLaunchKernelGGL(time_mix_fwd_kernel, dim3((unsigned)rows, (unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, x_f32, mk,
                     mv, mr, (bf16_t*)out_k, (bf16_t*)out_v, (bf16_t*)out_r, (long)rows, T, C);
  CFHIP_CHECK_LAUNCH("rwkv_time_mix_fwd");
  return CFHIP_OK;
}

extern "C" size_t cfhip_rwkv_time_mix_bwd_workspace(int64_t B, int T, int C) {
  if (B < 1 || T < 1 || C < 1 || B > RWKV_MAX_ELEMS / T / C || B * T > 0x7fffffffLL) return 0;
  long per;
  int chunks;
  time_mix_chunks(B * T, C, &per, &chunks);
  return (size_t)chunks * 3 * C * sizeof(float);
}

extern "C" int cfhip_rwkv_time_mix_bwd(const void* dk, const void* dv, const void* dr, int d_f32, const void* x, int x_f32, const float* mk,
                                       const float* mv, const float* mr, void* dx, float* dmk, float* dmv, float* dmr, int accumulate,
                                       void* workspace, size_t workspace_bytes, int64_t B, int T, int C, void* stream) {
  if (!rwkv_shape_ok(B, T, C, "rwkv_time_mix_bwd", "C")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(dk && dr && mk && mr && (!mv == !dv) && (mv || !dmv),
                "rwkv_time_mix_bwd: null operand (dk, dr, mk, mr; mv and dv together; dmv needs them)");
  const int want = (dmk ? 1 : 0) | (dmv ? 2 : 0) | (dmr ? 4 : 0);
  CFHIP_REQUIRE(x || !want, "rwkv_time_mix_bwd: null operand (x for the mix gradients)");
  CFHIP_REQUIRE(dx || want, "rwkv_time_mix_bwd: nothing to compute (dx and every mix gradient are NULL)");
  CFHIP_REQUIRE((accumulate & ~7) == 0, "rwkv_time_mix_bwd: `accumulate` = %d has bits past the three destinations", accumulate);
  CFHIP_REQUIRE(!want || (workspace && workspace_bytes >= cfhip_rwkv_time_mix_bwd_workspace(B, T, C)),
                "rwkv_time_mix_bwd: the workspace holds %zu bytes, cfhip_rwkv_time_mix_bwd_workspace says %zu", workspace ? workspace_bytes : (size_t)0,
                cfhip_rwkv_time_mix_bwd_workspace(B, T, C));
  CFHIP_REQUIRE(aligned4(mk, mv, mr, workspace) && aligned4(dmk, dmv, dmr) && (!x_f32 || aligned4(x, dx)) && (!d_f32 || aligned4(dk, dv, dr)) &&
                    (((uintptr_t)dk | (uintptr_t)dv | (uintptr_t)dr | (uintptr_t)x | (uintptr_t)dx) & 1) == 0,
                "rwkv_time_mix_bwd: misaligned operand");
  const int64_t rows = B * T;
  long per;
  int chunks;
  time_mix_chunks(rows, C, &per, &chunks);
  hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)((C + 255) / 256);
  hipLaunchKernelGGL(time_mix_bwd_kernel, dim3(gx, (unsigned)chunks), dim3(256), 0, s, dk, dv, dr, d_f32, x,
                     x_f32, mk, mv, mr, dx, want, (float*)workspace, (long)rows, T, C, per);
  CFHIP_CHECK_LAUNCH("rwkv_time_mix_bwd");
  if (want) {
    hipLaunchKernelGGL(time_mix_reduce_kernel, dim3(gx, 3), dim3(256), 0, s, (const float*)workspace, dmk, dmv, dmr, accumulate, chunks, C);
    CFHIP_CHECK_LAUNCH("rwkv_time_mix_bwd");
  }
  return CFHIP_OK;
}

extern "C" int cfhip_rwkv_wkv_fwd(const float* k, const float* v, const float* r, const float* info_decay, void* y, float* a, float* b,
                                  int64_t B, int T, int L, int waves, void* stream) {
  if (!rwkv_shape_ok(B, T, L, "rwkv_wkv_fwd", "L")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(k && v && r && info_decay && y && (!a == !b), "rwkv_wkv_fwd: null operand (k, v, r, info_decay, y; a and b together)");
  CFHIP_REQUIRE(waves >= 0 && waves <= WMAX, "rwkv_wkv_fwd: waves = %d (0 .. %d)", waves, WMAX);
  CFHIP_REQUIRE(B <= 65535, "rwkv_wkv_fwd: B = %lld is past the grid (65535 samples per launch)", (long long)B);
  CFHIP_REQUIRE(aligned4(k, v, r, info_decay) && aligned4(a, b) && ((uintptr_t)y & 1) == 0, "rwkv_wkv_fwd: misaligned operand");
  const int W = wkv_waves(B, T, L, waves);
  const dim3 grid((unsigned)((L + 63) / 64), (unsigned)B), block(64 * W);
  if (a)
    hipLaunchKernelGGL(wkv_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, k, v, r, info_decay, (bf16_t*)y, a, b, T, L);
  else
    hipLaunchKernelGGL(wkv_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, k, v, r, info_decay, (bf16_t*)y, a, b, T, L);
  CFHIP_CHECK_LAUNCH("rwkv_wkv_fwd");
  return CFHIP_OK;
}

extern "C" size_t cfhip_rwkv_wkv_bwd_workspace(int64_t B, int L) {
  if (B < 1 || L < 1 || B > 65535) return 0;
  return (size_t)B * L * sizeof(float);
}

extern "C" int cfhip_rwkv_wkv_bwd(const void* dy, int dy_f32, const float* k, const float* v, const float* r, const float* info_decay, const float* a,
                                  const float* b, void* dk, void* dv, void* dr, float* d_decay, int accumulate, void* workspace,
                                  size_t workspace_bytes, int64_t B, int T, int L, int waves, void* stream) {
  if (!rwkv_shape_ok(B, T, L, "rwkv_wkv_bwd", "L")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(dy && k && v && r && info_decay && a && b && dk && dv && dr, "rwkv_wkv_bwd: null operand (only d_decay and its workspace may be NULL)");
  CFHIP_REQUIRE(waves >= 0 && waves <= WMAX, "rwkv_wkv_bwd: waves = %d (0 .. %d)", waves, WMAX);
  CFHIP_REQUIRE(B <= 65535, "rwkv_wkv_bwd: B = %lld is past the grid (65535 samples per launch)", (long long)B);
  CFHIP_REQUIRE((accumulate & ~1) == 0, "rwkv_wkv_bwd: `accumulate` = %d has bits past the one destination", accumulate);
  CFHIP_REQUIRE(!d_decay || (workspace && workspace_bytes >= cfhip_rwkv_wkv_bwd_workspace(B, L)),
                "rwkv_wkv_bwd: the workspace holds %zu bytes, cfhip_rwkv_wkv_bwd_workspace says %zu", workspace ? workspace_bytes : (size_t)0,
                cfhip_rwkv_wkv_bwd_workspace(B, L));
  CFHIP_REQUIRE(aligned4(k, v, r, info_decay) && aligned4(a, b, d_decay, workspace) &&
                    (((uintptr_t)dy | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)dr) & 1) == 0 && (!dy_f32 || aligned4(dy)),
                "rwkv_wkv_bwd: misaligned operand");
  const int W = wkv_waves(B, T, L, waves);
  hipStream_t s = (hipStream_t)stream;
  float* part = d_decay ? (float*)workspace : nullptr;
  hipLaunchKernelGGL(wkv_bwd_kernel, dim3((unsigned)((L + 63) / 64), (unsigned)B), dim3(64 * W), 0, s, dy, dy_f32, k, v, r, info_decay,
                     a, b, (bf16_t*)dk, (bf16_t*)dv, (bf16_t*)dr, part, T, L);
  CFHIP_CHECK_LAUNCH("rwkv_wkv_bwd");
  if (d_decay) {
    hipLaunchKernelGGL(wkv_decay_reduce_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, (const float*)part, info_decay, d_decay,
                       accumulate, (long)B, L);
    CFHIP_CHECK_LAUNCH("rwkv_wkv_bwd");
  }
  return CFHIP_OK;
}

namespace {
bool elems_ok(int64_t n, const char* who) {
  if (n < 1 || n > RWKV_MAX_ELEMS) {
    cfhip_set_error("%s: n = %lld elements (1 .. 2^38)", who, (long long)n);
    return false;
  }
  return true;
}
unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" int cfhip_rwkv_relu2_fwd(const void* h, int h_f32, void* out, int64_t n, void* stream) {
  if (!elems_ok(n, "rwkv_relu2_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(h && out, "rwkv_relu2_fwd: null operand");
  CFHIP_REQUIRE((((uintptr_t)h | (uintptr_t)out) & 1) == 0 && (!h_f32 || aligned4(h)), "rwkv_relu2_fwd: misaligned operand");
  hipLaunchKernelGGL(relu2_fwd_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, h, h_f32, (bf16_t*)out, (long)n);
  CFHIP_CHECK_LAUNCH("rwkv_relu2_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_rwkv_relu2_bwd(const void* d, int d_f32, const void* h, int h_f32, void* dh, int64_t n, void* stream) {
  if (!elems_ok(n, "rwkv_relu2_bwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(d && h && dh, "rwkv_relu2_bwd: null operand");
  CFHIP_REQUIRE((((uintptr_t)d | (uintptr_t)h | (uintptr_t)dh) & 1) == 0 && (!h_f32 || aligned4(h)) && (!d_f32 || aligned4(d)),
                "rwkv_relu2_bwd: misaligned operand");
  hipLaunchKernelGGL(relu2_bwd_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, d, d_f32, h, h_f32, (bf16_t*)dh, (long)n);
  CFHIP_CHECK_LAUNCH("rwkv_relu2_bwd");
  return CFHIP_OK;
}

extern "C" int cfhip_rwkv_gate_fwd(const float* r, const float* kv, const void* residual, int residual_f32, void* out, int out_f32, int64_t n,
                                   void* stream) {
  if (!elems_ok(n, "rwkv_gate_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(r && kv && out, "rwkv_gate_fwd: null operand");
  CFHIP_REQUIRE(aligned4(r, kv) && (((uintptr_t)residual | (uintptr_t)out) & 1) == 0 && (!residual_f32 || aligned4(residual)) &&
                    (!out_f32 || aligned4(out)), "rwkv_gate_fwd: misaligned operand");
  hipLaunchKernelGGL(gate_fwd_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, r, kv, residual, residual_f32, out, out_f32, (long)n);
  CFHIP_CHECK_LAUNCH("rwkv_gate_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_rwkv_gate_bwd(const void* d, int d_f32, const float* r, const float* kv, void* dr, void* dkv, int64_t n, void* stream) {
  if (!elems_ok(n, "rwkv_gate_bwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(d && r && kv && dr && dkv, "rwkv_gate_bwd: null operand");
  CFHIP_REQUIRE(aligned4(r, kv) && (((uintptr_t)d | (uintptr_t)dr | (uintptr_t)dkv) & 1) == 0 && (!d_f32 || aligned4(d)),
                "rwkv_gate_bwd: misaligned operand");
  hipLaunchKernelGGL(gate_bwd_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, d, d_f32, r, kv, (bf16_t*)dr, (bf16_t*)dkv, (long)n);
  CFHIP_CHECK_LAUNCH("rwkv_gate_bwd");
  return CFHIP_OK;
}
