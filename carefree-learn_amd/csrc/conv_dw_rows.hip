// Depthwise 3x3 convolution over TOKEN ROWS, with the GELU fused: the middle of the reference's MixFeedForward
// (mixed_stacks/channel_mixers.py:46-66: Linear -> permute -> DepthWiseConv2d (convs/basic.py:187-201) -> flatten / transpose ->
// GELU -> Linear).  The GEMMs on either side produce and consume bf16 rows [B * H * W][C]; on rows the channels are the contiguous
// axis, so the permutes of the reference are no data movement at all and a lane's 16-byte access is 8 channels of one pixel.
//
// A stencil, not a GEMM: 9 multiply-adds per output with a weight per CHANNEL — there is no shared K axis an MFMA tile could
// contract over.  The work is two passes over memory (read x, write y) and the kernels are built around that:
//   * a workgroup (256 threads) owns a TILE_H x 8 pixel tile of one sample times a 64-channel slab (128 bytes of every row it touches);
//     thread = (pixel lane 0..31, channel lane 0..7), 8 channels per lane;
//   * the tile plus its halo is read from memory ONCE into LDS (zeros outside the image: the padding, the sample boundary and the
//     row wrap are all the same `inside` test made where the tile is filled), the 9 taps are 16-byte LDS reads;
//   * TILE_H = 8 (halo factor 100 / 64) when that still gives every CU a workgroup, 4 otherwise (a 16 x 16 token grid at
//     C = 2048 has 128 tiles of 8 rows but 256 of 4).
// Backward, one launch + one reduce: x with a halo of 2 -> LDS; g = dy * act'(conv(x) + bias) in f32 on the tile plus a halo of 1 ->
// LDS (the pre-activation is recomputed, never stored, and g is never rounded); dx = transposed stencil of g; dw / db accumulate in
// registers over the tiles a workgroup walks, are folded across its pixel lanes in a fixed order and leave as ONE partial per
// workgroup; a second kernel adds the partials in workgroup order.  No atomics: results are reproducible bit for bit.
#include "common.h"

#include <limits.h>

namespace {

constexpr int TW = 8;          // tile width in pixels
constexpr int CS = 64;         // channel slab of a workgroup: 8 lanes x 8 channels
constexpr int PIX_LANES = 32;  // 256 threads / 8 channel lanes
constexpr int ROW_U4 = CS / 8; // 16-byte words per LDS pixel (bf16)
constexpr int NACC = 10;       // 9 taps + the bias gradient

struct DwRows {
  const bf16_t* x; const float* w; const float* bias; bf16_t* y;
  const bf16_t* dy; bf16_t* dx; float* part; float* dw; float* db;
  long ld_x, ld_y, ld_dy, ld_dx;
  int B, H, W, C, act;
  int tiles_x, tiles_y, n_tiles, groups;  // groups: workgroups per slab in the backward (each walks tiles g, g + groups, ...)
  int want_w, want_b, acc_w, acc_b;
};

__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = bf16lo(v[e]);
    f[2 * e + 1] = bf16hi(v[e]);
  }
}

// the lane's 8 x 9 filter taps, read as stored (f32 [C][1][3][3]: 72 consecutive floats, 16-byte aligned because c % 8 == 0)
__device__ __forceinline__ void load_taps(const float* w, int c, bool live, float (&wv)[72]) {
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const f32x4 v = live ? *reinterpret_cast<const f32x4*>(w + (long)c * 9 + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
    wv[4 * i] = v[0]; wv[4 * i + 1] = v[1]; wv[4 * i + 2] = v[2]; wv[4 * i + 3] = v[3];
  }
}
__device__ __forceinline__ void load_bias(const float* bias, int c, bool live, float (&bv)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) bv[e] = 0.f;
  if (bias != nullptr && live) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(bias + c), b = *reinterpret_cast<const f32x4*>(bias + c + 4);
    bv[0] = a[0]; bv[1] = a[1]; bv[2] = a[2]; bv[3] = a[3]; bv[4] = b[0]; bv[5] = b[1]; bv[6] = b[2]; bv[7] = b[3];
  }
}

// rows [y0 - HALO, y0 + TH + HALO) x columns [x0 - HALO, x0 + TW + HALO) of sample b, this slab's channels -> LDS, zeros outside
template <int TH, int HALO>
__device__ __forceinline__ void fill_tile(u32x4* xs, const bf16_t* x, long ld, int b, int y0, int x0, int H, int W, int c, bool live,
                                          int pl, int cl) {
  constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
  for (int i = pl; i < LW * LH; i += PIX_LANES) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gy = y0 - HALO + ly, gx = x0 - HALO + lx;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (live && gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const u32x4*>(x + ((long)b * H * W + (long)gy * W + gx) * ld + c);
    xs[i * ROW_U4 + cl] = v;
  }
}

// bias + the 9 taps around LDS pixel (ly, lx) of a tile LW pixels wide (the pixel itself at tap 4)
template <int LW>
__device__ __forceinline__ void stencil(const u32x4* xs, int ly, int lx, int cl, const float (&wv)[72], const float (&bv)[8], float (&acc)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = bv[e];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      float xv[8];
      unpack8(xs[((ly + ky - 1) * LW + (lx + kx - 1)) * ROW_U4 + cl], xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(wv[e * 9 + ky * 3 + kx], xv[e], acc[e]);
    }
  }
}

__device__ __forceinline__ void tile_origin(const DwRows& p, int tile, int TH, int& b, int& y0, int& x0) {
  const int per = p.tiles_x * p.tiles_y;
  b = tile / per;
  const int r = tile - b * per;
  const int ty = r / p.tiles_x;
  y0 = ty * TH;
  x0 = (r - ty * p.tiles_x) * TW;
}

template <int TH>
__global__ __launch_bounds__(256) void dw_rows_fwd_kernel(DwRows p) {
  constexpr int LW = TW + 2;
  __shared__ u32x4 xs[(TH + 2) * LW * ROW_U4];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int c = blockIdx.y * CS + cl * 8;
  const bool live = c < p.C;
  int b, y0, x0;
  tile_origin(p, blockIdx.x, TH, b, y0, x0);
  fill_tile<TH, 1>(xs, p.x, p.ld_x, b, y0, x0, p.H, p.W, c, live, pl, cl);
  float wv[72], bv[8];
  load_taps(p.w, c, live, wv);
  load_bias(p.bias, c, live, bv);
  __syncthreads();
  if (!live) return;
  for (int i = pl; i < TH * TW; i += PIX_LANES) {
    const int py = i / TW, px = i - py * TW;
    const int gy = y0 + py, gx = x0 + px;
    if (gy >= p.H || gx >= p.W) continue;
    float acc[8];
    stencil<LW>(xs, py + 1, px + 1, cl, wv, bv, acc);
    if (p.act) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = gelu_erf_f(acc[e]);
    }
    st_bf16x8(p.y, ((long)b * p.H * p.W + (long)gy * p.W + gx) * p.ld_y + c, acc);
  }
}

template <int TH>
__global__ __launch_bounds__(256) void dw_rows_bwd_kernel(DwRows p) {
  constexpr int XW = TW + 4, GW = TW + 2, GH = TH + 2;
  __shared__ u32x4 xs[(TH + 4) * XW * ROW_U4];
  __shared__ f32x4 gs[GH * GW * 2 * ROW_U4];  // f32: two 16-byte words per lane and pixel; after the walk, the fold across waves
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int c = blockIdx.y * CS + cl * 8;
  const bool live = c < p.C;
  const bool sums = p.want_w || p.want_b;
  float wv[72], bv[8];
  load_taps(p.w, c, live, wv);
  load_bias(p.bias, c, live, bv);
  float aw[72], ab[8];
#pragma unroll
  for (int i = 0; i < 72; ++i) aw[i] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ab[e] = 0.f;

  for (int tile = blockIdx.x; tile < p.n_tiles; tile += p.groups) {
    int b, y0, x0;
    tile_origin(p, tile, TH, b, y0, x0);
    __syncthreads();  // the previous tile's readers are done with xs / gs
    if (p.act || p.want_w) fill_tile<TH, 2>(xs, p.x, p.ld_x, b, y0, x0, p.H, p.W, c, live, pl, cl);
    __syncthreads();
    // g on the tile and a halo of one pixel; zero outside the image
    for (int i = pl; i < GH * GW; i += PIX_LANES) {
      const int ly = i / GW, lx = i - ly * GW;
      const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = 0.f;
      if (live && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
        unpack8(*reinterpret_cast<const u32x4*>(p.dy + ((long)b * p.H * p.W + (long)gy * p.W + gx) * p.ld_dy + c), g);
        if (p.act) {
          float pre[8];
          stencil<XW>(xs, ly + 1, lx + 1, cl, wv, bv, pre);
#pragma unroll
          for (int e = 0; e < 8; ++e) g[e] *= gelu_erf_grad_f(pre[e]);
        }
      }
      gs[(i * ROW_U4 + cl) * 2] = f32x4{g[0], g[1], g[2], g[3]};
      gs[(i * ROW_U4 + cl) * 2 + 1] = f32x4{g[4], g[5], g[6], g[7]};
    }
    __syncthreads();
    if (!live) continue;
    for (int i = pl; i < TH * TW; i += PIX_LANES) {
      const int py = i / TW, px = i - py * TW;
      const int gy = y0 + py, gx = x0 + px;
      if (gy >= p.H || gx >= p.W) continue;
      if (p.dx != nullptr) {  // y(q) = sum_k w[k] x(q + o_k)  =>  dx(r) = sum_k w[k] g(r - o_k)
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int j = (((py + 2 - ky) * GW + (px + 2 - kx)) * ROW_U4 + cl) * 2;
            const f32x4 a = gs[j], d = gs[j + 1];
            const float gv[8] = {a[0], a[1], a[2], a[3], d[0], d[1], d[2], d[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wv[e * 9 + ky * 3 + kx], gv[e], acc[e]);
          }
        }
        st_bf16x8(p.dx, ((long)b * p.H * p.W + (long)gy * p.W + gx) * p.ld_dx + c, acc);
      }
      if (sums) {
        const int j = (((py + 1) * GW + (px + 1)) * ROW_U4 + cl) * 2;
        const f32x4 a = gs[j], d = gs[j + 1];
        const float gv[8] = {a[0], a[1], a[2], a[3], d[0], d[1], d[2], d[3]};
        if (p.want_b) {
#pragma unroll
          for (int e = 0; e < 8; ++e) ab[e] += gv[e];
        }
        if (p.want_w) {
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              float xv[8];
              unpack8(xs[((py + 1 + ky) * XW + (px + 1 + kx)) * ROW_U4 + cl], xv);
#pragma unroll
              for (int e = 0; e < 8; ++e) aw[e * 9 + ky * 3 + kx] = fmaf(gv[e], xv[e], aw[e * 9 + ky * 3 + kx]);
            }
          }
        }
      }
    }
  }
  if (!sums) return;
  // fold the 32 pixel lanes of each channel lane: the 8 of a wave by xor shuffles (lane = cl + 8 * j), the 4 waves through LDS in
  // wave order; one partial [C][10] per workgroup
  __syncthreads();
  float* red = reinterpret_cast<float*>(gs);  // [4 waves][8 channel lanes][80]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 80; ++i) {
    float v = i < 72 ? aw[i] : ab[i - 72];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 8) red[(wave * 8 + lane) * 80 + i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 8 * 80; i += 256) {
    const int l = i / 80, k = i - l * 80;  // k < 72: channel e = k / 9, tap k % 9; else the bias gradient of channel k - 72
    const int ch = blockIdx.y * CS + l * 8 + (k < 72 ? k / 9 : k - 72);
    if (ch >= p.C) continue;
    const float v = (red[(0 * 8 + l) * 80 + k] + red[(1 * 8 + l) * 80 + k]) + (red[(2 * 8 + l) * 80 + k] + red[(3 * 8 + l) * 80 + k]);
    p.part[((long)blockIdx.x * p.C + ch) * NACC + (k < 72 ? k % 9 : 9)] = v;
  }
}

// dw[c][k] / db[c] (+)= the partials added in workgroup order; one thread per (c, k)
__global__ __launch_bounds__(256) void dw_rows_reduce_kernel(DwRows p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.C * NACC) return;
  const int c = i / NACC, k = i - c * NACC;
  if (k < 9 ? !p.want_w : !p.want_b) return;
  float s = 0.f;
  for (int g = 0; g < p.groups; ++g) s += p.part[(long)g * p.C * NACC + i];
  if (k < 9) {
    float* out = p.dw + c * 9 + k;
    *out = p.acc_w ? *out + s : s;
  } else {
    p.db[c] = p.acc_b ? p.db[c] + s : s;
  }
}

// the CU count of the MI355X as a compile-time constant: the library is built for gfx950 only, and the tile choice must not depend on
// the device a call happens to run on (the workspace query takes no device; results are bit-identical from box to box)
constexpr int CUS = 256;

bool misaligned(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) != 0; }

// [ptr, ptr + bytes of M rows of C used elements, ld apart) of two operands share a byte (conservative: two column slices of one
// buffer interleave without sharing one and are refused too)
bool overlaps(const void* a, long ld_a, const void* b, long ld_b, long M, int C) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + (uintptr_t)(((M - 1) * ld_a + C) * 2), b1 = b0 + (uintptr_t)(((M - 1) * ld_b + C) * 2);
  return a0 < b1 && b0 < a1;
}

// a flat f32 operand of `bytes` bytes (dw, db, the workspace; null: absent) shares a byte with a rows operand (null: absent)
bool meets(const void* flat, size_t bytes, const void* rows, long ld, long M, int C) {
  if (flat == nullptr || rows == nullptr) return false;
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(flat), r0 = reinterpret_cast<uintptr_t>(rows);
  return f0 < r0 + (uintptr_t)(((M - 1) * ld + C) * 2) && r0 < f0 + bytes;
}

int geometry(DwRows& p, const char* who, int B, int H, int W, int C, int act) {
  CFHIP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: empty problem (B %d, H %d, W %d, C %d)", who, B, H, W, C);
  CFHIP_REQUIRE(C % 8 == 0, "%s: C = %d is not a multiple of 8 (16-byte accesses of 8 channels)", who, C);
  CFHIP_REQUIRE(act == 0 || act == 1, "%s: act = %d (0 none, 1 GELU)", who, act);
  CFHIP_REQUIRE((long)B * H * W <= (long)INT_MAX, "%s: B * H * W = %ld rows exceed the 31-bit row index", who, (long)B * H * W);
  p.B = B; p.H = H; p.W = W; p.C = C; p.act = act;
  return CFHIP_OK;
}

// 8-row tiles when they still give every CU a workgroup, 4-row tiles otherwise
int pick_tile(DwRows& p) {
  const int slabs = (p.C + CS - 1) / CS;
  p.tiles_x = (p.W + TW - 1) / TW;
  int th = 8;
  if ((long)p.B * ((p.H + 7) / 8) * p.tiles_x * slabs < CUS) th = 4;
  p.tiles_y = (p.H + th - 1) / th;
  p.n_tiles = p.B * p.tiles_y * p.tiles_x;  // <= B * H * W
  return th;
}

// workgroups per slab in the backward: about four per CU over all slabs, never more than tiles
int bwd_groups(const DwRows& p) {
  const int slabs = (p.C + CS - 1) / CS;
  const int g = (4 * CUS + slabs - 1) / slabs;
  return g < p.n_tiles ? g : p.n_tiles;
}

int check_rows(const char* who, const char* name, const void* ptr, int64_t ld, int C) {
  CFHIP_REQUIRE(ptr != nullptr, "%s: %s is null", who, name);
  CFHIP_REQUIRE(!misaligned(ptr), "%s: %s is not 16-byte aligned", who, name);
  CFHIP_REQUIRE(ld >= C && ld % 8 == 0, "%s: ld_%s = %ld must be a multiple of 8 and at least C = %d", who, name, (long)ld, C);
  return CFHIP_OK;
}

}  // namespace

extern "C" int cfhip_dwconv3x3_rows_fwd(const void* x, int64_t ld_x, const float* w, const float* bias, void* y, int64_t ld_y, int B,
                                        int H, int W, int C, int act, void* stream) {
  const char* who = "dwconv3x3_rows_fwd";
  DwRows p = {};
  int rc = geometry(p, who, B, H, W, C, act);
  if (rc == CFHIP_OK) rc = check_rows(who, "x", x, ld_x, C);
  if (rc == CFHIP_OK) rc = check_rows(who, "y", y, ld_y, C);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(w != nullptr && !misaligned(w) && !misaligned(bias), "%s: w / bias must be 16-byte aligned (w not null)", who);
  CFHIP_REQUIRE(!overlaps(x, ld_x, y, ld_y, (long)B * H * W, C), "%s: y overlaps x (a tile's halo is read after its neighbour wrote)", who);
  p.x = reinterpret_cast<const bf16_t*>(x); p.w = w; p.bias = bias; p.y = reinterpret_cast<bf16_t*>(y);
  p.ld_x = ld_x; p.ld_y = ld_y;
  const int th = pick_tile(p);
  const dim3 grid((unsigned)p.n_tiles, (unsigned)((C + CS - 1) / CS));
  CFHIP_REQUIRE(grid.y <= 65535u, "%s: C = %d needs more than 65535 channel slabs", who, C);
  if (th == 8) hipLaunchKernelGGL(dw_rows_fwd_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(dw_rows_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  CFHIP_CHECK_LAUNCH(who);
  return CFHIP_OK;
}

extern "C" size_t cfhip_dwconv3x3_rows_bwd_workspace(int B, int H, int W, int C) {
  DwRows p = {};
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (long)B * H * W > (long)INT_MAX) return 0;
  p.B = B; p.H = H; p.W = W; p.C = C;
  pick_tile(p);
  return (size_t)bwd_groups(p) * (size_t)C * NACC * sizeof(float);
}

extern "C" int cfhip_dwconv3x3_rows_bwd(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, const float* w, const float* bias,
                                        void* dx, int64_t ld_dx, float* dw, int dw_accumulate, float* db, int db_accumulate, int B,
                                        int H, int W, int C, int act, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "dwconv3x3_rows_bwd";
  DwRows p = {};
  int rc = geometry(p, who, B, H, W, C, act);
  if (rc == CFHIP_OK) rc = check_rows(who, "dy", dy, ld_dy, C);
  if (rc == CFHIP_OK) rc = check_rows(who, "x", x, ld_x, C);
  if (rc == CFHIP_OK && dx != nullptr) rc = check_rows(who, "dx", dx, ld_dx, C);
  if (rc != CFHIP_OK) return rc;
  CFHIP_REQUIRE(w != nullptr && !misaligned(w) && !misaligned(bias), "%s: w / bias must be 16-byte aligned (w not null)", who);
  CFHIP_REQUIRE(dx != nullptr || dw != nullptr || db != nullptr, "%s: no output asked for", who);
  const long M = (long)B * H * W;
  CFHIP_REQUIRE(dx == nullptr || (!overlaps(x, ld_x, dx, ld_dx, M, C) && !overlaps(dy, ld_dy, dx, ld_dx, M, C)),
                "%s: dx overlaps x or dy (a tile's halo is read after its neighbour wrote)", who);
  p.dy = reinterpret_cast<const bf16_t*>(dy); p.x = reinterpret_cast<const bf16_t*>(x); p.w = w; p.bias = bias;
  p.dx = reinterpret_cast<bf16_t*>(dx); p.dw = dw; p.db = db;
  p.ld_dy = ld_dy; p.ld_x = ld_x; p.ld_dx = ld_dx;
  p.want_w = dw != nullptr; p.want_b = db != nullptr; p.acc_w = dw_accumulate; p.acc_b = db_accumulate;
  const int th = pick_tile(p);
  p.groups = bwd_groups(p);
  if (p.want_w || p.want_b) {
    const size_t need = (size_t)p.groups * (size_t)C * NACC * sizeof(float);
    CFHIP_REQUIRE(workspace != nullptr && !misaligned(workspace) && workspace_bytes >= need,
                  "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", who, need, workspace_bytes);
    p.part = reinterpret_cast<float*>(workspace);
    const void* rows[3] = {x, dy, dx};
    const long lds[3] = {(long)ld_x, (long)ld_dy, (long)ld_dx};
    for (int i = 0; i < 3; ++i)
      CFHIP_REQUIRE(!meets(dw, (size_t)C * 36, rows[i], lds[i], M, C) && !meets(db, (size_t)C * 4, rows[i], lds[i], M, C) &&
                        !meets(workspace, need, rows[i], lds[i], M, C),
                    "%s: dw, db or the workspace overlaps a rows operand (x, dy or dx)", who);
  }
  const dim3 grid((unsigned)p.groups, (unsigned)((C + CS - 1) / CS));
  CFHIP_REQUIRE(grid.y <= 65535u, "%s: C = %d needs more than 65535 channel slabs", who, C);
  if (th == 8) hipLaunchKernelGGL(dw_rows_bwd_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(dw_rows_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  CFHIP_CHECK_LAUNCH(who);
  if (p.want_w || p.want_b) {
    hipLaunchKernelGGL(dw_rows_reduce_kernel, dim3((unsigned)((C * NACC + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    CFHIP_CHECK_LAUNCH("dwconv3x3_rows_bwd (reduce)");
  }
  return CFHIP_OK;
}
