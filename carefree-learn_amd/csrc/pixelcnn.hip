// PixelCNN sampling for gfx950 (reference modules/cv/ar/pixel_cnn.py:142-165: img_size^2 full forwards, one softmax + multinomial per pixel).
//
// In eval mode the net (pixel_cnn.py:90-104, 130-134: masked 7x7 convolution -> BatchNorm / identity -> LeakyReLU(0.2), L times, then a
// 1x1 head) is strictly causal: the output of every layer at pixel (i, j) depends only on pixels before (i, j) in raster order (mask
// "A", the first layer) or up to and including it (mask "B").  One pixel therefore needs ONE output column per layer, a
// [rows, T Cin] x [T Cin, C] product over the T = 24 / 25 live taps, not a forward over the whole map.
//
// Samples are independent, so ONE workgroup (512 threads, 8 waves) owns 16 batch rows for the whole launch and walks the pixels
// first_pixel .. last_pixel - 1 in raster order: no grid-wide barrier, no wait on another workgroup.  The activations of every layer
// live in global memory as bf16 [B][H][W][C] (`in0`: the input of layer 0, [B][H][W][Cin0]; `act`: [L][B][H][W][C]); a workgroup
// reads only rows it wrote itself at this or an earlier pixel (of this or an earlier launch), so the ordering it needs is the
// workgroup's own: stores drained (s_waitcnt vmcnt(0)), then __syncthreads().  Zero padding is never USED: the loads are branch-free,
// an address outside the image is clamped into the workgroup's own rows of the buffer (possibly onto a slot no pixel has written yet)
// and the loaded value is replaced by zero; no value of an unwritten slot reaches a result.  The filter packs hold the live taps only and are streamed from L2 in MFMA fragment
// order, one 16-byte load per lane and fragment (as csrc/rnn.hip streams W_hh).
//
// Pack of a layer (built on the host): K index k = t Cin + c, t the row-major index of the tap in the 7x7 window (the live taps are
// exactly t < T: three whole rows above, then the centre row up to the centre), zero for k >= T Cin up to Kp = a multiple of 32;
// fragment (n, kk), lane l holds W[16 n + (l & 15)][32 kk + 8 (l >> 4) + e], e = 0 .. 7.
//
// Operation order of one pixel (what the per-element tests derive their bounds from), per row:
//   layer l, channel c:  a = sum_k bf16(x[k]) * bf16(W[c][k])       one f32 MFMA accumulation chain over Kp / 32 instructions, from 0,
//                                                                     k ascending
//                        v = fma(a, scale[l][c], shift[l][c])       BatchNorm's eval affine in f32 (1, 0 without a norm)
//                        v = v > 0 ? v : 0.2f * v;  y = bf16(v)     stored; the operand of the next layer
//   head, code k:        lg[k] = (sum_c y[c] * bf16(Wh[k][c])) + bh[k]   one chain over C / 32 instructions, 1 rounding for the bias
//   draw (one wave per row, lane q owns the S = ceil(K / 64) consecutive codes q S .. q S + S - 1):
//        m     = max_k lg[k]
//        e[k]  = exp2((lg[k] - m) * log2(e))                        v_exp_f32, 1 ulp
//        s_q   = e[q S] + e[q S + 1] + ...                          sequential f32 sum of the lane's codes, from 0
//        P_q   = inclusive scan of s over the lanes: for off = 1, 2, 4, 8, 16, 32: P_q += P_{q - off} (q >= off)
//        total = P_63;  target = u * total, u = (w >> 8) * 2^-24, w = word e % 4 of Philox4x32-10(offset + e / 4; seed),
//                                            e = (b H + i) W + j: the draw depends on (seed, offset, b, i, j) only
//        run   = P_q - s_q, then run += e[k] for the lane's codes in order; the lane's candidate is its first k with run > target
//        code  = the smallest candidate of all lanes, K - 1 when there is none
//   `forced` != 0: the code is read from `codes` instead (teacher forcing); the logits are computed and stored all the same.
//   in0[b][i][j][:] = in_table[label_row[b]][code][:]  (the module's own to_blocks + channel padding of that code, as bf16)
// Nothing in a pixel's arithmetic depends on the launch's pixel range or on B: one launch over all pixels equals chained launches over
// any split of them, bit for bit.
#include "common.h"

namespace {

constexpr int PC_ROWS = 16;
constexpr int PC_THREADS = 512;
constexpr int PC_WAVES = PC_THREADS / 64;
static_assert(CFHIP_PIXELCNN_MAX_CHANNELS / 16 <= 2 * PC_WAVES, "two output tiles of a layer per wave at most");
constexpr int PC_SEG = (CFHIP_PIXELCNN_MAX_CODES + 63) / 64;           // codes per lane in the draw, at most
constexpr int PC_DEPTH = 8;                                             // K-chunks of a layer whose loads are in flight together
constexpr int PC_KCH = CFHIP_PIXELCNN_MAX_CHANNELS / 32;                // K-chunks of the head, at most
constexpr float PC_LOG2E = 1.4426950408889634f;

struct PcArgs {
  long long* codes;         // [B][1][H][W]
  const int* label_row;     // [B]: row of in_table's first dim
  const bf16_t* in_table;   // [U][K][Cin0]
  bf16_t* in0;              // [B][H][W][Cin0]
  bf16_t* act;              // [L][B][H][W][C]
  const bf16x8* packs;      // layer 0 (Kp0 = pad32(24 Cin0)), then L - 1 layers of Kp = 25 C
  const float* scale;       // [L][C]
  const float* shift;       // [L][C]
  const bf16x8* head_pack;  // [Kt][C / 32][64]
  const float* head_bias;   // [K]
  float* logits;            // [B][H][W][K] (per_pixel) or [B][K]
  unsigned long long seed, offset;
  long B;
  int H, W, C, Cin0, L, K, first, last, forced, per_pixel;
};

// the A fragment of K-chunk `kk` of a layer whose input has cin % 32 == 0 channels: 8 channels of one causal neighbour.  Branch-free, so
// that the loads of a group of chunks are all in flight together: the address is clamped to a pixel inside the image of a row this
// workgroup owns (in bounds; on the first rows of the image it can be a slot that is not written yet) and the loaded value is dropped
// where the tap is padding, the row is past B or the chunk is past the end of the layer.
__device__ __forceinline__ bf16x8 pc_gather(const bf16_t* src, long b_or_row0, bool row_ok, int i, int j, int H, int W, int cin, int per_tap,
                                            int kk, int kc, int lq) {
  const int kq = min(kk, kc - 1), t = kq / per_tap, c0 = (kq - t * per_tap) * 32 + lq * 8;
  const int ii = i + t / 7 - 3, jj = j + t % 7 - 3;
  const bool ok = row_ok && kk < kc && ii >= 0 && jj >= 0 && jj < W;
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (((b_or_row0 * H + max(ii, 0)) * W + min(max(jj, 0), W - 1)) * (long)cin + c0));
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? v : z;
}

// the single A fragment of a one-channel layer 0: element e is tap 8 lq + e (24 live taps, mask "A")
__device__ __forceinline__ bf16x8 pc_gather1(const bf16_t* src, long b, bool row_ok, int i, int j, int H, int W, int lq) {
  bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int t = lq * 8 + e;
    const int ii = i + t / 7 - 3, jj = j + t % 7 - 3;
    if (row_ok && t < 24 && ii >= 0 && jj >= 0 && jj < W) v[e] = (short)src[(b * H + ii) * W + jj];
  }
  return v;
}

template <int TPW>  // output tiles of one layer per wave: 1 up to 128 channels, 2 above
__global__ __launch_bounds__(PC_THREADS) void pixelcnn_sample_kernel(const PcArgs a) {
  const int H = a.H, W = a.W, C = a.C, K = a.K, L = a.L, Cin0 = a.Cin0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const long row0 = (long)blockIdx.x * PC_ROWS;
  const int nrows = (int)min((long)PC_ROWS, a.B - row0);
  const long b_a = row0 + lr;  // the batch row of this lane's A fragments
  const bool a_ok = lr < nrows;
  const int NT = C >> 4;
  const int KC0 = (24 * Cin0 + 31) >> 5, KC = (25 * C) >> 5, KCH = C >> 5;
  const long plane = (long)a.B * H * W * C;
  const int KT = (K + 15) >> 4;
  const int S = (K + 63) >> 6;
  for (int p = a.first; p < a.last; ++p) {
    const int i = p / W, j = p - i * W;
    for (int l = 0; l < L; ++l) {
      const bf16_t* src = l == 0 ? a.in0 : a.act + (long)(l - 1) * plane;
      bf16_t* dst = a.act + (long)l * plane;
      const int cin = l == 0 ? Cin0 : C, kc = l == 0 ? KC0 : KC;
      const bf16x8* pack = a.packs + (l == 0 ? 0L : ((long)NT * KC0 + (long)(l - 1) * NT * KC) * 64) + lane;
      f32x4 acc[TPW];
#pragma unroll
      for (int q = 0; q < TPW; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wave < NT) {
        // a wave whose second tile is past the layer's width computes its last tile again and drops it
        const bf16x8* wq[TPW];
#pragma unroll
        for (int q = 0; q < TPW; ++q) wq[q] = pack + (long)min(wave + q * PC_WAVES, NT - 1) * kc * 64;
        if (cin == 1) {
          const bf16x8 af = pc_gather1(src, b_a, a_ok, i, j, H, W, lq);
#pragma unroll
          for (int q = 0; q < TPW; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wq[q][0], acc[q], 0, 0, 0);
        } else {
          // PC_DEPTH K-chunks in flight: every load of a group is issued before its first MFMA (a plain loop pays one round trip to
          // L2 or beyond per chunk).  A chunk past the end multiplies a zero A fragment: exact zeros, the chain stays k ascending.
          const int per_tap = cin >> 5;
          const long b_ld = a_ok ? b_a : row0;
          for (int k0 = 0; k0 < kc; k0 += PC_DEPTH) {
            bf16x8 af[PC_DEPTH], wf[TPW][PC_DEPTH];
#pragma unroll
            for (int d = 0; d < PC_DEPTH; ++d) {
              af[d] = pc_gather(src, b_ld, a_ok, i, j, H, W, cin, per_tap, k0 + d, kc, lq);
#pragma unroll
              for (int q = 0; q < TPW; ++q) wf[q][d] = wq[q][(long)min(k0 + d, kc - 1) * 64];
            }
#pragma unroll
            for (int d = 0; d < PC_DEPTH; ++d) {
#pragma unroll
              for (int q = 0; q < TPW; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[d], wf[q][d], acc[q], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
          const int n = wave + q * PC_WAVES;
          if (n < NT) {
            const int c = n * 16 + lr;
            const float sc = a.scale[l * C + c], sh = a.shift[l * C + c];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
              const int r = lq * 4 + r4;
              if (r < nrows) {
                float v = fmaf(acc[q][r4], sc, sh);
                v = v > 0.f ? v : 0.2f * v;
                dst[(((row0 + r) * H + i) * W + j) * (long)C + c] = f32_to_bf16(v);
              }
            }
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    // head: f32 logits of the 16 rows
    {
      const bf16_t* top = a.act + (long)(L - 1) * plane;
      bf16x8 af[PC_KCH];  // the top layer's 16 rows at this pixel: the A operand of every head tile
#pragma unroll
      for (int kk = 0; kk < PC_KCH; ++kk) {
        af[kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (a_ok && kk < KCH) af[kk] = *reinterpret_cast<const bf16x8*>(top + (((b_a * H + i) * W + j) * (long)C + kk * 32 + lq * 8));
      }
      for (int n = wave; n < KT; n += PC_WAVES) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        bf16x8 wf[PC_KCH];
#pragma unroll
        for (int kk = 0; kk < PC_KCH; ++kk) {
          wf[kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          if (kk < KCH) wf[kk] = a.head_pack[((long)n * KCH + kk) * 64 + lane];
        }
#pragma unroll
        for (int kk = 0; kk < PC_KCH; ++kk)
          if (kk < KCH) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], wf[kk], acc, 0, 0, 0);
        const int k = n * 16 + lr;
        if (k < K) {
          const float bh = a.head_bias[k];
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int r = lq * 4 + r4;
            if (r < nrows) {
              const long b = row0 + r;
              float* lg = a.per_pixel ? a.logits + ((b * H + i) * W + j) * (long)K : a.logits + b * (long)K;
              lg[k] = acc[r4] + bh;
            }
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // draw: wave w takes rows w and w + 8
    for (int r = wave; r < nrows; r += PC_WAVES) {
      const long b = row0 + r;
      const long e = (b * H + i) * W + j;
      long long code;
      if (a.forced) {
        code = a.codes[e];
      } else {
        const float* lg = a.per_pixel ? a.logits + e * (long)K : a.logits + b * (long)K;
        float ev[PC_SEG];
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < PC_SEG; ++q) {
          const int k = lane * S + q;
          ev[q] = (q < S && k < K) ? lg[k] : -INFINITY;
          m = fmaxf(m, ev[q]);
        }
        m = wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < PC_SEG; ++q) {
          const int k = lane * S + q;
          ev[q] = (q < S && k < K) ? __builtin_amdgcn_exp2f((ev[q] - m) * PC_LOG2E) : 0.f;
          if (q < S && k < K) s += ev[q];
        }
        float P = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float up = __shfl_up(P, off, 64);
          if (lane >= off) P += up;
        }
        const float total = __shfl(P, 63, 64);
        const Philox ph = philox4x32_10(a.offset + (unsigned long long)(e >> 2), a.seed);
        const float u = (float)(ph.c[e & 3] >> 8) * 5.9604644775390625e-8f;  // 2^-24, exact
        const float target = u * total;
        float run = P - s;
        int cand = K - 1;
        bool found = false;
#pragma unroll
        for (int q = 0; q < PC_SEG; ++q) {
          const int k = lane * S + q;
          if (q < S && k < K) {
            run += ev[q];
            if (!found && run > target) {
              found = true;
              cand = k;
            }
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off, 64));
        code = cand;
        if (lane == 0) a.codes[e] = code;
      }
      const bf16_t* trow = a.in_table + ((long)a.label_row[b] * K + code) * Cin0;
      bf16_t* irow = a.in0 + e * (long)Cin0;
      for (int c = lane; c < Cin0; c += 64) irow[c] = trow[c];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

}  // namespace

extern "C" int cfhip_pixelcnn_sample(void* codes, const int* label_row, const void* in_table, void* in0, void* act, const void* packs,
                                     const float* scale, const float* shift, const void* head_pack, const float* head_bias,
                                     float* logits, int logits_per_pixel, int64_t B, int H, int W, int C, int Cin0, int L, int K,
                                     int first_pixel, int last_pixel, int forced, uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(C >= 32 && C <= CFHIP_PIXELCNN_MAX_CHANNELS && C % 32 == 0,
                "pixelcnn_sample: latent_channels = %d is outside the sampler (a multiple of 32, 32 .. %d)", C, CFHIP_PIXELCNN_MAX_CHANNELS);
  CFHIP_REQUIRE(Cin0 == 1 || Cin0 == C, "pixelcnn_sample: the first layer reads %d channels, expected 1 or latent_channels = %d", Cin0, C);
  CFHIP_REQUIRE(K >= 2 && K <= CFHIP_PIXELCNN_MAX_CODES, "pixelcnn_sample: num_codes = %d is outside the sampler (2 .. %d)", K,
                CFHIP_PIXELCNN_MAX_CODES);
  CFHIP_REQUIRE(L >= 1, "pixelcnn_sample: num_layers = %d", L);
  CFHIP_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffffLL && (B + PC_ROWS - 1) / PC_ROWS <= 0x7fffffffLL,
                "pixelcnn_sample: B = %lld, H = %d, W = %d", (long long)B, H, W);
  CFHIP_REQUIRE(first_pixel >= 0 && first_pixel <= last_pixel && last_pixel <= H * W,
                "pixelcnn_sample: pixel range [%d, %d) is not inside [0, %d)", first_pixel, last_pixel, H * W);
  CFHIP_REQUIRE(codes && label_row && in_table && in0 && act && packs && scale && shift && head_pack && head_bias && logits,
                "pixelcnn_sample: null operand");
  CFHIP_REQUIRE((((uintptr_t)packs | (uintptr_t)head_pack | (uintptr_t)act) & 15) == 0 && (Cin0 == 1 || ((uintptr_t)in0 & 15) == 0),
                "pixelcnn_sample: packs, head_pack, act and in0 must be 16-byte aligned");
  CFHIP_REQUIRE(((uintptr_t)codes & 7) == 0 && (((uintptr_t)label_row | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)head_bias |
                                                  (uintptr_t)logits) & 3) == 0 && (((uintptr_t)in_table | (uintptr_t)in0) & 1) == 0,
                "pixelcnn_sample: misaligned operand");
  if (first_pixel == last_pixel) return CFHIP_OK;
  PcArgs a{reinterpret_cast<long long*>(codes), label_row, reinterpret_cast<const bf16_t*>(in_table), reinterpret_cast<bf16_t*>(in0),
           reinterpret_cast<bf16_t*>(act), reinterpret_cast<const bf16x8*>(packs), scale, shift,
           reinterpret_cast<const bf16x8*>(head_pack), head_bias, logits, (unsigned long long)seed, (unsigned long long)offset, (long)B,
           H, W, C, Cin0, L, K, first_pixel, last_pixel, forced != 0, logits_per_pixel != 0};
  const dim3 grid((unsigned)((B + PC_ROWS - 1) / PC_ROWS));
  if (C <= 16 * PC_WAVES) hipLaunchKernelGGL(pixelcnn_sample_kernel<1>, grid, dim3(PC_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pixelcnn_sample_kernel<2>, grid, dim3(PC_THREADS), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("pixelcnn_sample");
  return CFHIP_OK;
}
