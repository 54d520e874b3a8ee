// Siren (sine-activated coordinate MLP) for gfx950: the layer stack of reference modules/implicit/siren.py:156-187.
//
// Rows r = b N + n (M = B N), sample b = r / N; a 16-row tile may straddle samples.  The reference runs L times F.linear -> sin -> * mod
// over a [B, N, latent] tensor (siren.py:185-186) and then the head (siren.py:187); here one launch walks all layers and the head with
// the tile's activations in LDS, so no [M, latent] tensor exists in HBM unless a gradient is wanted.
//
// H = latent (a multiple of 32, 32 .. 256), KC = H / 32, NT = H / 16, in_dim <= 8, out_dim <= 16.
//
// cfhip_siren_pack: W f32 [R][K] -> bf16 in v_mfma_f32_16x16x32_bf16 B-fragment order, once or (with_transposed: a hidden weight whose layer
// will be differentiated; the head's backward reads the f32 weight) twice:
//   forward pack    fragment (j KC + kk), lane l: W[16 j + (l & 15)][32 kk + 8 (l >> 4) + e], e = 0 .. 7, zero past row R
//   transposed pack (after the forward pack) fragment (kt RC + jj), lane l: W[32 jj + 8 (l >> 4) + e][16 kt + (l & 15)], RC = ceil(R / 32)
//
// Operation order of the forward (cfhip_siren_fwd), per row r of sample b -- what the per-element tests derive their bounds from:
//   pre0_k  = fma(x_{d-1}, W0[k][d-1], ... fma(x_0, W0[k][0], b0[k]))   f32 VALU from the f32 coordinates, in_dim roundings
//   s0_k    = sin(w0 pre0_k), c0_k = cos(w0 pre0_k)                     the product rounded once, then the accurate library sine (full
//                                                                        range reduction: |w0 pre0| reaches ~60 rad)
//   h_l,k   = bf16(s_l,k * mod_l[b][k])                                 one f32 product, one rounding to the matrix operand
//   pre_l,j = (sum_k h_{l-1},k * bf16(W_l[j][k])) + b_l[j]              one f32 MFMA accumulation chain over KC instructions from 0, then 1 rounding
//   s_l,j   = sin(w pre_l,j), c_l,j = cos(w pre_l,j)
//   out_o   = (sum_k h_{L-1},k * bf16(Wh[o][k])) + bh[o]                the same chain
// With `save`, s_l and c_l go to HBM as bf16 [L][M][H] for the backward.
//
// The backward (cfhip_siren_bwd, one wave per 16-row tile, top layer first), dh in f32 accumulator registers:
//   dh_{L-1},k = fma chain over o ascending of dy[o] * Wh[o][k]          f32 VALU on the f32 head weight
//   q_l      = dh_l * S_l                      (S, C: the saved bf16 words)             d mod_l[b] = sum over the rows of b of q_l
//   dpre_l   = ((dh_l * mod_l[b]) * w) * C_l                                            db_l = sum over rows of dpre_l
//   dh_{l-1} = sum_j bf16(dpre_l,j) * bf16(W_l[j][k])  one MFMA chain on the transposed pack
//   (S_l, C_l reach the lanes through LDS: 16-byte rows in, the accumulator layout out; bf16(dpre_l) and bf16(S_l mod_l) leave the same way)
//   dW_l (l >= 1) = the caller's tn GEMM over the stored bf16(dpre_l) [M][H] and bf16(S_{l-1} * mod_{l-1}) [M][H]
//   dW_0[k][d] = sum over rows of dpre_0,k * x_d;  dx_d = fma chain over k = lr, lr + 16, ... then a fold over the 16 lanes (xor 1, 2, 4, 8)
//   dWh[o][k] = sum over rows of dy_o * (S_{L-1},k * mod);  dbh = sum over rows of dy
//   Row sums: 4 rows per lane in row order ((r0 + r1) + (r2 + r3)), a fold over the 4 lane groups (xor 16, 32): one record per TILE in the
//   workspace.  d mod: one record per (tile, sample) pair, record index tile + sample (unique: both are monotone in the row).
// cfhip_siren_reduce: destination = [accumulate ? destination : 0] + the records' sum: G lanes per element, lane i takes records i, i + G, ...
//   ascending, then a xor-fold 32, 16, .. 1 (G = 64), or one lane in ascending order (G = 1).  The split into tiles depends on M alone.
// No floating-point atomics anywhere: two identical calls are bit-identical.
#include "common.h"

namespace {

constexpr int SR_HMAX = CFHIP_SIREN_MAX_LATENT;
constexpr int SR_IMAX = CFHIP_SIREN_MAX_IN;
constexpr int SR_OMAX = CFHIP_SIREN_MAX_OUT;
constexpr int SR_KCMAX = SR_HMAX / 32;
constexpr int SR_NTMAX = SR_HMAX / 16;
constexpr int SR_LD = SR_HMAX + 8;  // bf16 elements per row of a wave's activation tile (rows 16 bytes apart mod 32 banks)

struct SirenArgs {
  const float* x;      // [M][in_dim], or [N][in_dim] with x_shared (the grid buffer: row r reads its row r - b N)
  const float* w0;     // [H][in_dim]
  const float* bias;   // [L H + out_dim] or null
  const float* mods;   // [L][B][H]
  const bf16x8* pack;  // L - 1 hidden packs, `hid` fragment lanes apart, then the head's forward pack
  long hid;
  float* out;          // [M][out_dim]
  bf16_t* ss;          // [L][M][H] sin words (written by the forward, read by the backward) or null
  bf16_t* sc;          // cos words
  const float* dy;     // [M][out_dim]
  const float* wh;     // [out_dim][H] f32
  float* part;         // [tiles][rec]
  float* pm;           // [tiles + B][L][H]
  float* dx;           // [M][in_dim] or null
  bf16_t* dpre;        // [L - 1][M][H] or null
  bf16_t* hp;          // [L - 1][M][H] or null
  long M, N, B;
  int in_dim, H, out_dim, L, x_shared;
  float w_first, w_hidden;
};

__device__ __forceinline__ float sr_bf(bf16_t v) { return __uint_as_float((unsigned)v << 16); }
__host__ __device__ __forceinline__ long sr_rec(int L, int H, int in_dim, int out_dim) { return (long)L * H + (long)H * in_dim + (long)out_dim * H + 16; }
// bf16x8 fragments-times-lanes of one pack of W [R][K]: the forward part and the whole
__host__ __device__ __forceinline__ long sr_pack_fwd(int R, int K) { return (long)((R + 15) / 16) * (K / 32) * 64; }
__host__ __device__ __forceinline__ long sr_pack_all(int R, int K) { return sr_pack_fwd(R, K) + (long)(K / 16) * ((R + 31) / 32) * 64; }

__global__ __launch_bounds__(256) void siren_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ out, int R, int K, int with_t) {
  const int KC = K >> 5, RC = (R + 31) >> 5;
  const long fwd = sr_pack_fwd(R, K), all = with_t ? sr_pack_all(R, K) : fwd;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= all) return;
  const bool tr = id >= fwd;
  const long f = tr ? id - fwd : id;
  const int lane = (int)(f & 63);
  const long frag = f >> 6;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int r, k;
    if (!tr) {
      r = (int)(frag / KC) * 16 + (lane & 15), k = (int)(frag % KC) * 32 + (lane >> 4) * 8 + e;
    } else {
      r = (int)(frag % RC) * 32 + (lane >> 4) * 8 + e, k = (int)(frag / RC) * 16 + (lane & 15);
    }
    v[e] = r < R ? w[(long)r * K + k] : 0.f;
  }
  out[id] = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

__global__ __launch_bounds__(256) void siren_fwd_kernel(const SirenArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t tile_s[4][16 * SR_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int H = a.H, KC = H >> 5, NT = H >> 4, din = a.in_dim;
  const long M = a.M;
  bf16_t* tile = tile_s[wave];
  const long row0 = ((long)blockIdx.x * 4 + wave) * 16;
  long bc[4];  // the samples of the lane's four accumulator rows (a row past M stands for the last row: computed, never stored)
#pragma unroll
  for (int i = 0; i < 4; ++i) bc[i] = min(row0 + lq * 4 + i, M - 1) / a.N;
  {
    // layer 0 in the A-fragment layout: the lane owns row lr and 8 consecutive units per 32
    const long ra = min(row0 + lr, M - 1), ba = ra / a.N;
    const float* xr = a.x + (a.x_shared ? ra - ba * a.N : ra) * din;
    float u[SR_IMAX];
#pragma unroll
    for (int j = 0; j < SR_IMAX; ++j) u[j] = j < din ? xr[j] : 0.f;
    const float* m0 = a.mods + ba * H;
    const bool keep = a.ss && row0 + lr < M;
    for (int kk = 0; kk < KC; ++kk) {
      const int k0 = kk * 32 + lq * 8;
      float s[8], c[8], h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        float pre = a.bias ? a.bias[k] : 0.f;
#pragma unroll
        for (int j = 0; j < SR_IMAX; ++j)
          if (j < din) pre = fmaf(u[j], a.w0[k * din + j], pre);
        sincosf(a.w_first * pre, &s[e], &c[e]);
        h[e] = s[e] * m0[k];
      }
      st_bf16x8(tile, lr * SR_LD + k0, h);
      if (keep) {
        st_bf16x8(a.ss, (row0 + lr) * H + k0, s);
        st_bf16x8(a.sc, (row0 + lr) * H + k0, c);
      }
    }
  }
  __syncthreads();
  const long hid = a.hid;
  bf16x8 af[SR_KCMAX];
  for (int l = 1; l < a.L; ++l) {
    const bf16x8* wp = a.pack + (l - 1) * hid + lane;
#pragma unroll
    for (int kk = 0; kk < SR_KCMAX; ++kk)
      if (kk < KC) af[kk] = *reinterpret_cast<const bf16x8*>(tile + lr * SR_LD + kk * 32 + lq * 8);
    __syncthreads();
    for (int j = 0; j < NT; ++j) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < SR_KCMAX; ++kk)
        if (kk < KC) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], wp[(j * KC + kk) * 64], acc, 0, 0, 0);
      const int col = j * 16 + lr;
      const float bj = a.bias ? a.bias[(long)l * H + col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s, c;
        sincosf(a.w_hidden * (acc[i] + bj), &s, &c);
        const float m = a.mods[((long)l * a.B + bc[i]) * H + col];
        tile[(lq * 4 + i) * SR_LD + col] = f32_to_bf16(s * m);
        const long row = row0 + lq * 4 + i;
        if (a.ss && row < M) {
          a.ss[((long)l * M + row) * H + col] = f32_to_bf16(s);
          a.sc[((long)l * M + row) * H + col] = f32_to_bf16(c);
        }
      }
    }
    __syncthreads();
  }
  {
    const bf16x8* wp = a.pack + (a.L - 1) * hid + lane;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < SR_KCMAX; ++kk)
      if (kk < KC) {
        const bf16x8 f = *reinterpret_cast<const bf16x8*>(tile + lr * SR_LD + kk * 32 + lq * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, wp[kk * 64], acc, 0, 0, 0);
      }
    if (lr < a.out_dim) {
      const float bo = a.bias ? a.bias[(long)a.L * H + lr] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long row = row0 + lq * 4 + i;
        if (row < M) a.out[row * a.out_dim + lr] = acc[i] + bo;
      }
    }
  }
}

__device__ __forceinline__ float sr_fold_groups(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// two waves per workgroup: three bf16 tiles per wave (dpre, and the layer's saved sine and cosine words, which arrive and leave as 16-byte
// rows and are read in the accumulator layout from LDS) stay below 64 KB of static LDS
__global__ __launch_bounds__(128) void siren_bwd_kernel(const SirenArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t tile_s[2][16 * SR_LD], stile_s[2][16 * SR_LD], ctile_s[2][16 * SR_LD];
  __shared__ float dys_s[2][16 * SR_OMAX], xs_s[2][16 * SR_IMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int H = a.H, KC = H >> 5, NT = H >> 4, din = a.in_dim, dout = a.out_dim, L = a.L;
  const long M = a.M, tiles = (M + 15) >> 4;
  bf16_t* tile = tile_s[wave];
  bf16_t* stile = stile_s[wave];
  bf16_t* ctile = ctile_s[wave];
  float* dys = dys_s[wave];
  float* xs = xs_s[wave];
  const long t = (long)blockIdx.x * 2 + wave, row0 = t * 16;
  const bool live = t < tiles;  // (a dead wave of the last workgroup walks the code for the barriers: all its rows are past M)
  const long rec = sr_rec(L, H, din, dout);
  float* part = a.part + (live ? t : 0) * rec;
  const long off_w0 = (long)L * H, off_wh = off_w0 + (long)H * din, off_bh = off_wh + (long)dout * H;
  long rc[4], bc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rc[i] = min(row0 + lq * 4 + i, M - 1);
    bc[i] = rc[i] / a.N;
  }
  const long b_lo = min(row0, M - 1) / a.N, b_hi = min(row0 + 15, M - 1) / a.N;
  for (int i = lane; i < 16 * SR_OMAX; i += 64) {
    const long row = row0 + (i >> 4);
    const int o = i & 15;
    dys[i] = row < M && o < dout ? a.dy[row * dout + o] : 0.f;
  }
  for (int i = lane; i < 16 * SR_IMAX; i += 64) {
    const long r = min(row0 + (i >> 3), M - 1), b = r / a.N;
    const int j = i & 7;
    xs[i] = j < din ? a.x[(a.x_shared ? r - b * a.N : r) * din + j] : 0.f;
  }
  __syncthreads();
  if (live && lane < dout) {
    float s = 0.f;
    for (int r = 0; r < 16; ++r) s += dys[r * 16 + lane];
    part[off_bh + lane] = s;
  }
  float dh[SR_NTMAX][4];
#pragma unroll
  for (int j = 0; j < SR_NTMAX; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dh[j][i] = 0.f;
    if (j < NT) {
      for (int o = 0; o < dout; ++o) {
        const float w = a.wh[(long)o * H + j * 16 + lr];
#pragma unroll
        for (int i = 0; i < 4; ++i) dh[j][i] = fmaf(dys[(lq * 4 + i) * 16 + o], w, dh[j][i]);
      }
    }
  }
  float du[4][SR_IMAX];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < SR_IMAX; ++j) du[i][j] = 0.f;
  const long hid = a.hid, hid_fwd = sr_pack_fwd(H, H);
  for (int l = L - 1; l >= 0; --l) {
    const float wl = l == 0 ? a.w_first : a.w_hidden;
    const bf16_t* ssl = a.ss + (long)l * M * H;
    const bf16_t* scl = a.sc + (long)l * M * H;
    const float* ml = a.mods + (long)l * a.B * H;
    {
      const long ra = min(row0 + lr, M - 1);
      for (int kk = 0; kk < KC; ++kk) {
        const int k0 = kk * 32 + lq * 8;
        *reinterpret_cast<u32x4*>(stile + lr * SR_LD + k0) = *reinterpret_cast<const u32x4*>(ssl + ra * H + k0);
        *reinterpret_cast<u32x4*>(ctile + lr * SR_LD + k0) = *reinterpret_cast<const u32x4*>(scl + ra * H + k0);
      }
    }
    __syncthreads();
    const bool put_dpre = l >= 1 && a.dpre, put_hp = l <= L - 2 && a.hp;
#pragma unroll
    for (int j = 0; j < SR_NTMAX; ++j)
      if (j < NT) {
        const int col = j * 16 + lr;
        float q[4], dp[4], hh[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int at = (lq * 4 + i) * SR_LD + col;
          const float s = sr_bf(stile[at]), c = sr_bf(ctile[at]), m = ml[bc[i] * H + col];
          q[i] = dh[j][i] * s;
          dp[i] = ((dh[j][i] * m) * wl) * c;
          hh[i] = s * m;
          tile[at] = f32_to_bf16(dp[i]);
          if (put_hp) stile[at] = f32_to_bf16(hh[i]);  // (the lane that read the word replaces it)
        }
        const float sb = sr_fold_groups((dp[0] + dp[1]) + (dp[2] + dp[3]));
        if (live && lq == 0) part[(long)l * H + col] = sb;
        if (l == L - 1) {
          for (int o = 0; o < dout; ++o) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) s = fmaf(dys[(lq * 4 + i) * 16 + o], hh[i], s);
            s = sr_fold_groups(s);
            if (live && lq == 0) part[off_wh + (long)o * H + col] = s;
          }
        }
        for (long bb = b_lo; bb <= b_hi; ++bb) {
          float v = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) v += bc[i] == bb ? q[i] : 0.f;
          v = sr_fold_groups(v);
          if (live && lq == 0) a.pm[((t + bb) * L + l) * H + col] = v;
        }
        if (l == 0) {
#pragma unroll
          for (int jj = 0; jj < SR_IMAX; ++jj)
            if (jj < din) {
              float s = 0.f;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                s = fmaf(dp[i], xs[(lq * 4 + i) * 8 + jj], s);
                du[i][jj] = fmaf(dp[i], a.w0[col * din + jj], du[i][jj]);
              }
              s = sr_fold_groups(s);
              if (live && lq == 0) part[off_w0 + (long)col * din + jj] = s;
            }
        }
      }
    __syncthreads();
    if ((put_dpre || put_hp) && row0 + lr < M) {
      for (int kk = 0; kk < KC; ++kk) {
        const int k0 = kk * 32 + lq * 8;
        if (put_dpre)
          *reinterpret_cast<u32x4*>(a.dpre + ((long)(l - 1) * M + row0 + lr) * H + k0) = *reinterpret_cast<const u32x4*>(tile + lr * SR_LD + k0);
        if (put_hp)
          *reinterpret_cast<u32x4*>(a.hp + ((long)l * M + row0 + lr) * H + k0) = *reinterpret_cast<const u32x4*>(stile + lr * SR_LD + k0);
      }
    }
    if (l >= 1) {
      const bf16x8* wpt = a.pack + (l - 1) * hid + hid_fwd + lane;
      bf16x8 af[SR_KCMAX];
#pragma unroll
      for (int jj = 0; jj < SR_KCMAX; ++jj)
        if (jj < KC) af[jj] = *reinterpret_cast<const bf16x8*>(tile + lr * SR_LD + jj * 32 + lq * 8);
#pragma unroll
      for (int kt = 0; kt < SR_NTMAX; ++kt)
        if (kt < NT) {
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int jj = 0; jj < SR_KCMAX; ++jj)
            if (jj < KC) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[jj], wpt[(kt * KC + jj) * 64], acc, 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) dh[kt][i] = acc[i];
        }
      __syncthreads();
    }
  }
  if (a.dx) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + lq * 4 + i;
#pragma unroll
      for (int jj = 0; jj < SR_IMAX; ++jj)
        if (jj < din) {
          float s = du[i][jj];
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
          if (lr == 0 && row < M) a.dx[row * din + jj] = s;
        }
    }
  }
}

// mode 0: dst[e] (+)= sum over tiles t of src[t rec + e] (src already points at the section)
// mode 1: dst[(l B + b) H + col] (+)= sum over the tiles t of sample b of src[((t + b) L + l) H + col]
__global__ __launch_bounds__(256) void siren_reduce_kernel(const float* __restrict__ src, float* __restrict__ dst, long n, int G, int mode,
                                                           long tiles, long rec, long B, long N, int L, int H, int accumulate) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  const long e = G == 64 ? id >> 6 : id;
  const int sub = G == 64 ? (int)(id & 63) : 0;
  if (e >= n) return;  // (whole waves leave together: 256 % 64 == 0)
  long t0 = 0, t1 = tiles - 1, base = e, stride = rec;
  if (mode == 1) {
    const int col = (int)(e % H);
    const long lb = e / H, b = lb % B, l = lb / B;
    t0 = (b * N) >> 4, t1 = ((b + 1) * N - 1) >> 4;
    stride = (long)L * H;
    base = (b * L + l) * H + col;
  }
  float s = 0.f;
  for (long t = t0 + sub; t <= t1; t += G) s += src[t * stride + base];
  if (G == 64) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  }
  if (sub == 0) dst[e] = accumulate ? dst[e] + s : s;
}

__global__ __launch_bounds__(256) void sine_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float w) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id < n) y[id] = sinf(w * x[id]);
}

__global__ __launch_bounds__(256) void sine_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long n,
                                                       float w) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id < n) dx[id] = (dy[id] * w) * cosf(w * x[id]);
}

// the modulator's ReLU on f32 rows (siren.py:80-83): y = max(x, 0); dx = y > 0 ? dy : 0 (the mask read from the saved output)
__global__ __launch_bounds__(256) void relu_f32_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id < n) y[id] = fmaxf(x[id], 0.f);
}

__global__ __launch_bounds__(256) void relu_f32_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long n) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id < n) dx[id] = y[id] > 0.f ? dy[id] : 0.f;
}

bool siren_shape_ok(int64_t B, int64_t N, int in_dim, int H, int out_dim, int L, const char* who) {
  if (H < 32 || H > SR_HMAX || H % 32 != 0) {
    cfhip_set_error("%s: latent = %d is outside the kernel (a multiple of 32, 32 .. %d)", who, H, SR_HMAX);
    return false;
  }
  if (in_dim < 1 || in_dim > SR_IMAX || out_dim < 1 || out_dim > SR_OMAX || L < 1 || L > 65536) {
    cfhip_set_error("%s: in_dim = %d (1 .. %d), out_dim = %d (1 .. %d), num_layers = %d (1 .. 65536)", who, in_dim, SR_IMAX, out_dim, SR_OMAX, L);
    return false;
  }
  if (B < 1 || N < 1 || B >= 0x7fffffffLL || N >= 0x7fffffffLL || B * N >= 0x7fffffffLL) {
    cfhip_set_error("%s: B = %lld, N = %lld (M = B N in 1 .. 2^31 - 2)", who, (long long)B, (long long)N);
    return false;
  }
  return true;
}

}  // namespace

extern "C" size_t cfhip_siren_pack_workspace(int rows, int K, int with_transposed) {
  if (K < 32 || K > SR_HMAX || K % 32 != 0 || rows < 1 || rows > SR_HMAX) return 0;
  return 16 * (size_t)(with_transposed ? sr_pack_all(rows, K) : sr_pack_fwd(rows, K));
}

extern "C" int cfhip_siren_pack(const float* w, void* packed, size_t packed_bytes, int rows, int K, int with_transposed, void* stream) {
  CFHIP_REQUIRE(K >= 32 && K <= SR_HMAX && K % 32 == 0 && rows >= 1 && rows <= SR_HMAX,
                "siren_pack: rows = %d (1 .. %d), K = %d (a multiple of 32, 32 .. %d)", rows, SR_HMAX, K, SR_HMAX);
  CFHIP_REQUIRE(w && packed, "siren_pack: null operand");
  CFHIP_REQUIRE(packed_bytes == cfhip_siren_pack_workspace(rows, K, with_transposed),
                "siren_pack: `packed` holds %zu bytes, cfhip_siren_pack_workspace says %zu", packed_bytes,
                cfhip_siren_pack_workspace(rows, K, with_transposed));
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)w & 3) == 0, "siren_pack: misaligned operand");
  const long lanes = with_transposed ? sr_pack_all(rows, K) : sr_pack_fwd(rows, K);
  hipLaunchKernelGGL(siren_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     reinterpret_cast<u32x4*>(packed), rows, K, with_transposed != 0);
  CFHIP_CHECK_LAUNCH("siren_pack");
  return CFHIP_OK;
}

extern "C" int cfhip_siren_fwd(const float* x, int x_shared, const float* w0, const void* packed, int packed_transposed, const float* bias, const float* mods, float* out,
                               void* save_sin, void* save_cos, int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers,
                               float w_first, float w_hidden, void* stream) {
  if (!siren_shape_ok(B, N, in_dim, latent, out_dim, num_layers, "siren_fwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(x && w0 && packed && mods && out, "siren_fwd: null operand");
  CFHIP_REQUIRE(!save_sin == !save_cos, "siren_fwd: save_sin and save_cos together");
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)save_sin & 15) == 0 && ((uintptr_t)save_cos & 15) == 0,
                "siren_fwd: `packed` and the saved words must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)w0 | (uintptr_t)bias | (uintptr_t)mods | (uintptr_t)out) & 3) == 0, "siren_fwd: misaligned operand");
  SirenArgs a{};
  a.x = x, a.x_shared = x_shared != 0, a.w0 = w0, a.pack = reinterpret_cast<const bf16x8*>(packed), a.bias = bias, a.mods = mods, a.out = out;
  a.ss = reinterpret_cast<bf16_t*>(save_sin), a.sc = reinterpret_cast<bf16_t*>(save_cos);
  a.hid = packed_transposed ? sr_pack_all(latent, latent) : sr_pack_fwd(latent, latent);
  a.M = B * N, a.N = N, a.B = B, a.in_dim = in_dim, a.H = latent, a.out_dim = out_dim, a.L = num_layers, a.w_first = w_first, a.w_hidden = w_hidden;
  const long tiles = (a.M + 15) / 16;
  hipLaunchKernelGGL(siren_fwd_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("siren_fwd");
  return CFHIP_OK;
}

// bytes of the backward's workspace (0 for a refused shape)
extern "C" size_t cfhip_siren_bwd_workspace(int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers) {
  if (latent < 32 || latent > SR_HMAX || latent % 32 != 0 || in_dim < 1 || in_dim > SR_IMAX || out_dim < 1 || out_dim > SR_OMAX ||
      num_layers < 1 || num_layers > 65536 || B < 1 || N < 1 || B >= 0x7fffffffLL || N >= 0x7fffffffLL || B * N >= 0x7fffffffLL)
    return 0;
  const size_t tiles = (size_t)((B * N + 15) / 16);
  return sizeof(float) * (tiles * (size_t)sr_rec(num_layers, latent, in_dim, out_dim) + (tiles + (size_t)B) * num_layers * latent);
}

extern "C" int cfhip_siren_bwd(const float* dy, const float* x, int x_shared, const float* w0, const void* packed, const float* head_w,
                               const float* mods, const void* save_sin, const void* save_cos, float* dx, void* dpre, void* hprev,
                               void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers,
                               float w_first, float w_hidden, void* stream) {
  if (!siren_shape_ok(B, N, in_dim, latent, out_dim, num_layers, "siren_bwd")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(dy && x && w0 && packed && head_w && mods && save_sin && save_cos, "siren_bwd: null operand");
  const size_t need = cfhip_siren_bwd_workspace(B, N, in_dim, latent, out_dim, num_layers);
  CFHIP_REQUIRE(workspace && workspace_bytes >= need, "siren_bwd: the workspace holds %zu bytes, cfhip_siren_bwd_workspace says %zu",
                workspace ? workspace_bytes : (size_t)0, need);
  CFHIP_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "siren_bwd: `packed` and the workspace must be 16-byte aligned");
  CFHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)w0 | (uintptr_t)head_w | (uintptr_t)mods | (uintptr_t)dx) & 3) == 0 &&
                    (((uintptr_t)save_sin | (uintptr_t)save_cos | (uintptr_t)dpre | (uintptr_t)hprev) & 15) == 0,
                "siren_bwd: misaligned operand");
  SirenArgs a{};
  a.dy = dy, a.x = x, a.x_shared = x_shared != 0, a.w0 = w0, a.pack = reinterpret_cast<const bf16x8*>(packed), a.wh = head_w, a.mods = mods;
  a.ss = reinterpret_cast<bf16_t*>(const_cast<void*>(save_sin)), a.sc = reinterpret_cast<bf16_t*>(const_cast<void*>(save_cos));
  a.dx = dx, a.dpre = reinterpret_cast<bf16_t*>(dpre), a.hp = reinterpret_cast<bf16_t*>(hprev), a.hid = sr_pack_all(latent, latent);
  a.M = B * N, a.N = N, a.B = B, a.in_dim = in_dim, a.H = latent, a.out_dim = out_dim, a.L = num_layers, a.w_first = w_first, a.w_hidden = w_hidden;
  const long tiles = (a.M + 15) / 16;
  a.part = reinterpret_cast<float*>(workspace);
  a.pm = a.part + tiles * sr_rec(num_layers, latent, in_dim, out_dim);
  hipLaunchKernelGGL(siren_bwd_kernel, dim3((unsigned)((tiles + 1) / 2)), dim3(128), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("siren_bwd");
  return CFHIP_OK;
}

extern "C" int cfhip_siren_reduce(const void* workspace, size_t workspace_bytes, int kind, int layer, float* dest, int accumulate, int64_t B,
                                  int64_t N, int in_dim, int latent, int out_dim, int num_layers, void* stream) {
  if (!siren_shape_ok(B, N, in_dim, latent, out_dim, num_layers, "siren_reduce")) return CFHIP_ERR_INVALID;
  const size_t need = cfhip_siren_bwd_workspace(B, N, in_dim, latent, out_dim, num_layers);
  CFHIP_REQUIRE(workspace && workspace_bytes >= need, "siren_reduce: the workspace holds %zu bytes, cfhip_siren_bwd_workspace says %zu",
                workspace ? workspace_bytes : (size_t)0, need);
  CFHIP_REQUIRE(dest && ((uintptr_t)dest & 3) == 0 && ((uintptr_t)workspace & 15) == 0, "siren_reduce: null or misaligned destination");
  CFHIP_REQUIRE(kind >= CFHIP_SIREN_DB && kind <= CFHIP_SIREN_DMODS, "siren_reduce: kind = %d", kind);
  CFHIP_REQUIRE(kind != CFHIP_SIREN_DB || (layer >= 0 && layer < num_layers), "siren_reduce: layer = %d of %d", layer, num_layers);
  CFHIP_REQUIRE(accumulate == 0 || accumulate == 1, "siren_reduce: `accumulate` = %d", accumulate);
  const long M = B * N, tiles = (M + 15) / 16, rec = sr_rec(num_layers, latent, in_dim, out_dim);
  const float* part = reinterpret_cast<const float*>(workspace);
  const long off_w0 = (long)num_layers * latent, off_wh = off_w0 + (long)latent * in_dim, off_bh = off_wh + (long)out_dim * latent;
  const float* src = part;
  long n = 0;
  int G = 64, mode = 0;
  switch (kind) {
    case CFHIP_SIREN_DB: src = part + (long)layer * latent, n = latent; break;
    case CFHIP_SIREN_DW0: src = part + off_w0, n = (long)latent * in_dim; break;
    case CFHIP_SIREN_DWHEAD: src = part + off_wh, n = (long)out_dim * latent; break;
    case CFHIP_SIREN_DBHEAD: src = part + off_bh, n = out_dim; break;
    default: src = part + tiles * rec, n = (long)num_layers * B * latent, mode = 1, G = N > 256 ? 64 : 1; break;
  }
  const long threads = n * G;
  hipLaunchKernelGGL(siren_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dest, n, G, mode, tiles,
                     rec, (long)B, (long)N, num_layers, latent, accumulate);
  CFHIP_CHECK_LAUNCH("siren_reduce");
  return CFHIP_OK;
}

extern "C" int cfhip_sine_fwd(const float* x, float* y, int64_t n, float w, void* stream) {
  CFHIP_REQUIRE(x && y, "sine_fwd: null operand");
  CFHIP_REQUIRE(n >= 1 && n < 0x7fffffffLL * 256, "sine_fwd: n = %lld", (long long)n);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0, "sine_fwd: misaligned operand");
  hipLaunchKernelGGL(sine_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, w);
  CFHIP_CHECK_LAUNCH("sine_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_sine_bwd(const float* dy, const float* x, float* dx, int64_t n, float w, void* stream) {
  CFHIP_REQUIRE(dy && x && dx, "sine_bwd: null operand");
  CFHIP_REQUIRE(n >= 1 && n < 0x7fffffffLL * 256, "sine_bwd: n = %lld", (long long)n);
  CFHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx) & 3) == 0, "sine_bwd: misaligned operand");
  hipLaunchKernelGGL(sine_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, (long)n, w);
  CFHIP_CHECK_LAUNCH("sine_bwd");
  return CFHIP_OK;
}

extern "C" int cfhip_relu_f32_fwd(const float* x, float* y, int64_t n, void* stream) {
  CFHIP_REQUIRE(x && y, "relu_f32_fwd: null operand");
  CFHIP_REQUIRE(n >= 1 && n < 0x7fffffffLL * 256, "relu_f32_fwd: n = %lld", (long long)n);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0, "relu_f32_fwd: misaligned operand");
  hipLaunchKernelGGL(relu_f32_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n);
  CFHIP_CHECK_LAUNCH("relu_f32_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_relu_f32_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream) {
  CFHIP_REQUIRE(dy && y && dx, "relu_f32_bwd: null operand");
  CFHIP_REQUIRE(n >= 1 && n < 0x7fffffffLL * 256, "relu_f32_bwd: n = %lld", (long long)n);
  CFHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dx) & 3) == 0, "relu_f32_bwd: misaligned operand");
  hipLaunchKernelGGL(relu_f32_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, (long)n);
  CFHIP_CHECK_LAUNCH("relu_f32_bwd");
  return CFHIP_OK;
}
