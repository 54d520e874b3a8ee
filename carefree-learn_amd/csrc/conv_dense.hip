// 3x3 / stride 1 / padding 1 convolution on bf16 NHWC rows WITH ROW STRIDES on both sides, for the dense blocks of the RRDB upscaler
// (reference cflearn/modules/cv/translator/rrdb.py:12-29: five convolutions over torch.cat((inp, net1, ...), 1)): the input is the
// channel prefix [0, Cin) of a buffer [B H W][ld_in], the output a slice of N channels of a buffer [B H W][ld_out], so a dense block
// reads and writes slices of ONE buffer and never concatenates.  Also the small input kernel in front of the net (rrdb.py:47-55).
//
// One workgroup (4 waves) computes a spatial tile of TH x TW = 8 x 32 output pixels and all N output channels.  Per chunk of <= 64
// input channels the tile with its one-pixel halo (10 x 34 pixels) is staged in LDS ONCE and read by all nine taps: a pixel is
// fetched from memory 1.33 times per launch instead of 9 times.  Rows of the LDS image are 128 bytes (64 channels); the 16-byte slot
// of a pixel is XOR-ed with the low three bits of the pixel's index, so the 16 consecutive pixels x 4 slots a ds_read_b128 wave
// access touches spread over the 64 banks.  A chunk travels global -> registers (11 x 16 bytes per thread, every load in flight at
// once) -> LDS; the loads of the NEXT chunk are issued before the current one is multiplied and land behind its MFMAs.
//
// One v_mfma_f32_16x16x32_bf16 per (16 output channels) x (16 pixels) x (32 channels of one tap), FILTERS as the A operand (one
// predicated 16-byte global load per lane out of wp[N][Kp], k = tap Cin + c: the layout of cfhip_conv3x3_direct_pack; <= 110 KB per
// layer, cache resident), PIXELS as the B operand (one ds_read_b128 per lane), as in conv_direct.hip.  A wave owns two rows of the
// tile = four 16-pixel groups, so one A fragment feeds four MFMAs and one B fragment feeds N / 16: per MFMA (16 cycles) a wave asks
// the LDS array for 4 / (N / 16) cycles, four waves for 16 of 32 at N = 32.  The loop over (K-step, tap) is rolled and fetches the
// filters of the next group of steps while the current group is multiplied (3 steps per group at N <= 32, 1 at N = 64: what the
// registers allow at 3 and 2 waves per SIMD).  A channel chunk that is no multiple of 32 (Cin = 8, 16, 48) is zero-filled in LDS up
// to the K-step and its filter lanes are predicated to zero.
// The accumulator (col = lane & 15 = pixel, row = 4 (lane >> 4) + reg = channel) leaves a lane four consecutive output channels of one
// pixel: the epilogue (bias, LeakyReLU, one or two scaled residuals: f32, the reference's operation order, not contracted) and one
// 8-byte bf16 store, or four f32 stores into [B][n_store][H][W] for the net's last layer.
// f32 accumulation in a fixed order, no split reduction, no atomics: bit-identical between runs.
#include "common.h"

namespace {

constexpr int TH = CFHIP_DENSE_TILE_H, TW = CFHIP_DENSE_TILE_W, HALO_W = TW + 2, HALO = (TH + 2) * HALO_W;
constexpr int NPIECE = (HALO * 8 + 255) / 256;  // 16-byte pieces of a 64-channel halo tile per thread

struct DenseArgs {
  const bf16_t* x;
  const bf16_t* wp;
  const float* bias;
  void* y;
  const bf16_t* r1;
  const bf16_t* r2;
  int B, H, W, Ho, Wo, Cin, Kp, n_store, epilogue, up2, out_f32_nchw;
  long ld_in, ld_out, ld_r1, ld_r2;
  float slope, s1, s2;
};

template <int NT>
__global__ __launch_bounds__(256) void conv3x3_dense_kernel(const DenseArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[HALO * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
  int t = blockIdx.x;
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y, b = t / tiles_y;
  const int ox0 = tx * TW, oy0 = ty * TH;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  f32x4 acc[4][NT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[g][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the 16-byte pieces of one chunk's halo tile this thread moves: global -> registers (all loads in flight at once) -> LDS
  u32x4 piece[NPIECE];
  auto stage_load = [&](int c0) {
    const int cw = min(64, a.Cin - c0), sshift = ((cw + 31) >> 5) + 1;  // 4 or 8 slots of 8 channels per pixel
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int i = tid + 256 * j, p = i >> sshift, sl = i - (p << sshift);
      const int hy = p / HALO_W, hx = p - hy * HALO_W;
      const int oy = oy0 - 1 + hy, ox = ox0 - 1 + hx;
      piece[j] = u32x4{0u, 0u, 0u, 0u};
      if (p < HALO && oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo && sl * 8 < cw) {
        const int sy = a.up2 ? oy >> 1 : oy, sx = a.up2 ? ox >> 1 : ox;
        piece[j] = *reinterpret_cast<const u32x4*>(a.x + (((long)b * a.H + sy) * a.W + sx) * a.ld_in + c0 + sl * 8);
      }
    }
  };
  auto stage_store = [&](int c0) {
    const int cw = min(64, a.Cin - c0), sshift = ((cw + 31) >> 5) + 1;
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
      const int i = tid + 256 * j, p = i >> sshift, sl = i - (p << sshift);
      if (p < HALO) *reinterpret_cast<u32x4*>(tile + p * 64 + ((sl ^ (p & 7)) << 3)) = piece[j];
    }
  };
  // the A fragments (filters) of one GROUP of PF steps; step = 9 s + tap: K-step s of 32 channels, tap = 3 ky + kx (PF divides 9)
  constexpr int PF = NT <= 2 ? 3 : 1;  // steps fetched ahead: what keeps N <= 32 at three and N = 64 at two waves per SIMD of registers
  auto load_a = [&](int c0, int group, bf16x8 (&af)[PF][NT]) {
    const int s = group * PF >= 9, c = c0 + 32 * s + 8 * q;  // this lane's 8 channels of the K-step
#pragma unroll
    for (int t = 0; t < PF; ++t)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        af[t][nt] = c < a.Cin ? *reinterpret_cast<const bf16x8*>(a.wp + (long)(16 * nt + col) * a.Kp + (group * PF + t - 9 * s) * a.Cin + c)
                              : zero;
  };

  stage_load(0);
  for (int c0 = 0; c0 < a.Cin; c0 += 64) {
    const int groups = 9 / PF * ((min(64, a.Cin - c0) + 31) >> 5);  // (K-steps of 32 channels) x taps / PF
    __syncthreads();  // the previous chunk has been read
    stage_store(c0);
    __syncthreads();
    bf16x8 af[PF][NT], an[PF][NT];
    load_a(c0, 0, af);
    if (c0 + 64 < a.Cin) stage_load(c0 + 64);  // in flight while this chunk is multiplied
#pragma unroll 1  // (fully unrolled, the compiler hoists the filter loads of all nine taps: 144 registers at N = 64)
    for (int group = 0; group < groups; ++group) {
      if (group + 1 < groups) load_a(c0, group + 1, an);  // the next group's filters, behind this group's 4 PF N / 16 MFMAs
      const int s = group * PF >= 9, tap0 = group * PF - 9 * s, sl = 4 * s + q;
#pragma unroll
      for (int t = 0; t < PF; ++t) {
        const int ky = (tap0 + t) / 3, kx = tap0 + t - 3 * ky;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int p = (2 * wave + (g >> 1) + ky) * HALO_W + (g & 1) * 16 + col + kx;
          const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(tile + p * 64 + ((sl ^ (p & 7)) << 3));
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[g][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t][nt], bfrag, acc[g][nt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < PF; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) af[t][nt] = an[t][nt];
    }
  }

#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int oy = oy0 + 2 * wave + (g >> 1), ox = ox0 + (g & 1) * 16 + col;
    if (oy >= a.Ho || ox >= a.Wo) continue;
    const long pix = ((long)b * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n0 = 16 * nt + 4 * q;
      if (n0 >= a.n_store) continue;
      const bool whole = n0 + 4 <= a.n_store;  // all four channels of this lane are stored
      float v[4] = {acc[g][nt][0], acc[g][nt][1], acc[g][nt][2], acc[g][nt][3]};
      float r1v[4] = {0.f, 0.f, 0.f, 0.f}, r2v[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.bias != nullptr) {
        if (whole) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n0);
          v[0] += bv[0], v[1] += bv[1], v[2] += bv[2], v[3] += bv[3];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n0 + e < a.n_store) v[e] += a.bias[n0 + e];
        }
      }
      if (a.epilogue >= CFHIP_DENSE_EPI_RES1) {
        const bf16_t* rp = a.r1 + pix * a.ld_r1 + n0;
        if (whole) {
          const u32x2 w = *reinterpret_cast<const u32x2*>(rp);
          r1v[0] = bf16lo(w[0]), r1v[1] = bf16hi(w[0]), r1v[2] = bf16lo(w[1]), r1v[3] = bf16hi(w[1]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n0 + e < a.n_store) r1v[e] = bf16_to_f32(rp[e]);
        }
      }
      if (a.epilogue == CFHIP_DENSE_EPI_RES2) {
        const bf16_t* rp = a.r2 + pix * a.ld_r2 + n0;
        if (whole) {
          const u32x2 w = *reinterpret_cast<const u32x2*>(rp);
          r2v[0] = bf16lo(w[0]), r2v[1] = bf16hi(w[0]), r2v[2] = bf16lo(w[1]), r2v[3] = bf16hi(w[1]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n0 + e < a.n_store) r2v[e] = bf16_to_f32(rp[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = v[e];
        if (a.epilogue == CFHIP_DENSE_EPI_LRELU) u = u > 0.f ? u : __fmul_rn(a.slope, u);
        if (a.epilogue >= CFHIP_DENSE_EPI_RES1) u = __fadd_rn(__fmul_rn(a.s1, u), r1v[e]);    // net * 0.2 + inp (rrdb.py:29)
        if (a.epilogue == CFHIP_DENSE_EPI_RES2) u = __fadd_rn(__fmul_rn(u, a.s2), r2v[e]);    // net * 0.2 + inp (rrdb.py:44)
        v[e] = u;
      }
      if (a.out_f32_nchw) {
        float* yp = reinterpret_cast<float*>(a.y) + (((long)b * a.n_store + n0) * a.Ho + oy) * a.Wo + ox;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n0 + e < a.n_store) yp[(long)e * a.Ho * a.Wo] = v[e];
      } else {
        bf16_t* yp = reinterpret_cast<bf16_t*>(a.y) + pix * a.ld_out + n0;
        if (whole) {
          *reinterpret_cast<u32x2*>(yp) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n0 + e < a.n_store) yp[e] = f32_to_bf16(v[e]);
        }
      }
    }
  }
}

// one thread per 8 output channels of one output pixel
template <bool IN_F32>
__global__ __launch_bounds__(256) void unshuffle_nhwc_kernel(const void* __restrict__ x, bf16_t* __restrict__ y, long B, int C, int H,
                                                             int W, int s, int Cp) {
  const int Hs = H / s, Ws = W / s, slots = Cp >> 3, C2 = C * s * s;
  const long total = B * Hs * Ws * slots;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int sl = (int)(i % slots);
    const long pix = i / slots;
    const int ox = (int)(pix % Ws), oy = (int)((pix / Ws) % Hs);
    const long b = pix / ((long)Ws * Hs);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int oc = sl * 8 + e;  // = c s^2 + dy s + dx (rrdb.py:53-54)
      v[e] = 0.f;
      if (oc < C2) {
        const int c = oc / (s * s), r = oc - c * s * s, dy = r / s, dx = r - dy * s;
        v[e] = ld_act(x, ((b * C + c) * H + oy * s + dy) * W + ox * s + dx, IN_F32);
      }
    }
    st_bf16x8(y, i << 3, v);
  }
}

typedef void (*dense_kernel_t)(const DenseArgs);

// [lo, hi) in bytes of `rows` rows of `width` elements with row stride `ld`
struct Span {
  uintptr_t lo, hi;
};
inline Span span_of(const void* p, long rows, long ld, long width, int elem) {
  return Span{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(((rows - 1) * ld + width) * elem)};
}
inline bool spans_meet(Span u, Span v) { return u.lo < v.hi && v.lo < u.hi; }
// A bf16 output slice [.., n_out) of rows with stride ld_out against a bf16 operand that reads [0, n_read) of rows with stride ld_read:
// disjoint byte ranges, or the SAME row grid (equal strides, equal row count) with the columns apart — the dense block's normal case.
inline bool slice_clear(Span out, long ld_out, long n_out, Span read, long ld_read, long n_read, bool same_rows) {
  if (!spans_meet(out, read)) return true;
  if (!same_rows || ld_out != ld_read) return false;
  const long d = ((long)out.lo - (long)read.lo) / 2;  // elements (both 16-byte aligned)
  const long off = ((d % ld_read) + ld_read) % ld_read;
  return off >= n_read && off + n_out <= ld_read;
}

}  // namespace

extern "C" int cfhip_conv3x3_dense_bf16(const void* x, const void* wp, const float* bias, void* y, const void* r1, const void* r2, int B,
                                        int H, int W, int Cin, int N, int n_store, int64_t ld_in, int64_t ld_out, int64_t ld_r1,
                                        int64_t ld_r2, int epilogue, float slope, float s1, float s2, int up2, int out_f32_nchw,
                                        void* stream) {
  CFHIP_REQUIRE(x && wp && y, "conv3x3_dense_bf16: null x, wp or y");
  CFHIP_REQUIRE(B > 0 && H > 0 && W > 0, "conv3x3_dense_bf16: bad image B = %d, H = %d, W = %d", B, H, W);
  CFHIP_REQUIRE(Cin >= 8 && Cin <= 192 && Cin % 8 == 0, "conv3x3_dense_bf16: Cin = %d (a multiple of 8 up to 192)", Cin);
  CFHIP_REQUIRE(ld_in % 8 == 0, "conv3x3_dense_bf16: ld_in = %lld (a multiple of 8)", (long long)ld_in);
  CFHIP_REQUIRE(ld_in >= Cin, "conv3x3_dense_bf16: ld_in = %lld < Cin = %d", (long long)ld_in, Cin);
  CFHIP_REQUIRE(N == 16 || N == 32 || N == 64, "conv3x3_dense_bf16: N = %d (16, 32 or 64)", N);
  CFHIP_REQUIRE(n_store >= 1 && n_store <= N, "conv3x3_dense_bf16: n_store = %d (1 .. N = %d)", n_store, N);
  CFHIP_REQUIRE(epilogue >= CFHIP_DENSE_EPI_NONE && epilogue <= CFHIP_DENSE_EPI_RES2,
                "conv3x3_dense_bf16: unknown epilogue %d (0 none, 1 lrelu, 2 res1, 3 res2)", epilogue);
  const bool res1 = epilogue >= CFHIP_DENSE_EPI_RES1, res2 = epilogue == CFHIP_DENSE_EPI_RES2;
  CFHIP_REQUIRE(!res1 || r1, "conv3x3_dense_bf16: epilogue res1 / res2 without its operand r1");
  CFHIP_REQUIRE(!res2 || r2, "conv3x3_dense_bf16: epilogue res2 without its operand r2");
  CFHIP_REQUIRE(!res1 || (ld_r1 % 8 == 0 && ld_r1 >= n_store), "conv3x3_dense_bf16: ld_r1 = %lld (a multiple of 8, >= n_store)",
                (long long)ld_r1);
  CFHIP_REQUIRE(!res2 || (ld_r2 % 8 == 0 && ld_r2 >= n_store), "conv3x3_dense_bf16: ld_r2 = %lld (a multiple of 8, >= n_store)",
                (long long)ld_r2);
  const int Ho = up2 ? 2 * H : H, Wo = up2 ? 2 * W : W;
  CFHIP_REQUIRE(H <= (1 << 14) && W <= (1 << 14), "conv3x3_dense_bf16: image %d x %d too large", H, W);
  const long tiles = (long)B * ((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW);
  CFHIP_REQUIRE(tiles < (1L << 31), "conv3x3_dense_bf16: %ld tiles (B too large)", tiles);
  if (!out_f32_nchw)
    CFHIP_REQUIRE(ld_out % 8 == 0 && ld_out >= n_store, "conv3x3_dense_bf16: ld_out = %lld (a multiple of 8, >= n_store = %d)",
                  (long long)ld_out, n_store);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)wp | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)(res1 ? r1 : nullptr) |
                  (uintptr_t)(res2 ? r2 : nullptr)) & 15) == 0, "conv3x3_dense_bf16: misaligned operand");
  // neighbouring pixels' taps would race with a store into what they read: refuse before anything is launched
  const long Pin = (long)B * H * W, Pout = (long)B * Ho * Wo;
  const Span in = span_of(x, Pin, ld_in, Cin, 2);
  const Span out = out_f32_nchw ? span_of(y, 1, 0, Pout * n_store, 4) : span_of(y, Pout, ld_out, n_store, 2);
  const bool rows = !out_f32_nchw;
  CFHIP_REQUIRE(rows ? slice_clear(out, ld_out, n_store, in, ld_in, Cin, !up2) : !spans_meet(out, in),
                "conv3x3_dense_bf16: the output range overlaps the channels [0, %d) it reads", Cin);
  if (res1) {
    const Span r = span_of(r1, Pout, ld_r1, n_store, 2);
    CFHIP_REQUIRE(rows ? slice_clear(out, ld_out, n_store, r, ld_r1, n_store, true) : !spans_meet(out, r),
                  "conv3x3_dense_bf16: the output range overlaps the residual r1");
  }
  if (res2) {
    const Span r = span_of(r2, Pout, ld_r2, n_store, 2);
    CFHIP_REQUIRE(rows ? slice_clear(out, ld_out, n_store, r, ld_r2, n_store, true) : !spans_meet(out, r),
                  "conv3x3_dense_bf16: the output range overlaps the residual r2");
  }
  DenseArgs a;
  a.x = (const bf16_t*)x, a.wp = (const bf16_t*)wp, a.bias = bias, a.y = y;
  a.r1 = res1 ? (const bf16_t*)r1 : nullptr, a.r2 = res2 ? (const bf16_t*)r2 : nullptr;
  a.B = B, a.H = H, a.W = W, a.Ho = Ho, a.Wo = Wo, a.Cin = Cin, a.Kp = (9 * Cin + 31) / 32 * 32, a.n_store = n_store;
  a.epilogue = epilogue, a.up2 = up2 != 0, a.out_f32_nchw = out_f32_nchw != 0;
  a.ld_in = ld_in, a.ld_out = ld_out, a.ld_r1 = ld_r1, a.ld_r2 = ld_r2;
  a.slope = slope, a.s1 = s1, a.s2 = s2;
  const dense_kernel_t kernel = N == 16 ? conv3x3_dense_kernel<1> : N == 32 ? conv3x3_dense_kernel<2> : conv3x3_dense_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("conv3x3_dense_bf16");
  return CFHIP_OK;
}

extern "C" int cfhip_pixel_unshuffle_nhwc(const void* x, int x_is_f32, void* y, int64_t B, int C, int H, int W, int s, void* stream) {
  CFHIP_REQUIRE(x && y, "pixel_unshuffle_nhwc: null x or y");
  CFHIP_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "pixel_unshuffle_nhwc: bad shape B = %lld, C = %d, H = %d, W = %d", (long long)B, C, H, W);
  CFHIP_REQUIRE(s == 1 || s == 2 || s == 4, "pixel_unshuffle_nhwc: s = %d (1, 2 or 4)", s);
  CFHIP_REQUIRE(H % s == 0 && W % s == 0, "pixel_unshuffle_nhwc: H = %d, W = %d not divisible by s = %d", H, W, s);
  CFHIP_REQUIRE((long)C * s * s <= 4096, "pixel_unshuffle_nhwc: C s^2 = %ld (up to 4096)", (long)C * s * s);
  CFHIP_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)x & (x_is_f32 ? 3 : 1)) == 0, "pixel_unshuffle_nhwc: misaligned operand");
  const int Cp = (C * s * s + 7) / 8 * 8;
  const long total = (long)B * (H / s) * (W / s) * (Cp / 8);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (x_is_f32)
    hipLaunchKernelGGL((unshuffle_nhwc_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, (long)B, C,
                       H, W, s, Cp);
  else
    hipLaunchKernelGGL((unshuffle_nhwc_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, (long)B, C,
                       H, W, s, Cp);
  CFHIP_CHECK_LAUNCH("pixel_unshuffle_nhwc");
  return CFHIP_OK;
}
