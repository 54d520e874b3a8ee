// Direct 3x3 convolution for FEW channels (the ControlNet hint block, reference multimodal/diffusion/unet.py:441-457: hint -> 16 -> 16
// -> 32 (stride 2) -> 32 -> 96 (stride 2) at 8x the latent's side) and the bf16 SiLU between those convolutions.
//
// These layers have 8 .. 96 channels on 512^2 images: the im2row route writes a [B H W, 9 Cin] matrix that is 9x the activation, reads
// it back in the GEMM, and repeats both for the input gradient.  Here the taps are gathered straight from the NHWC activation.
//
// One v_mfma_f32_16x16x32_bf16 per (16 output channels) x (16 pixels) x (32 of K), FILTERS as the A operand, PIXELS as the B operand:
//   K is ordered k = tap * Cp + c with Cp (the input channels) a multiple of 8, so the 8 consecutive k a lane holds of either operand
//   (A[row lane & 15][8 (lane >> 4) + j], B[8 (lane >> 4) + j][col lane & 15]) are 8 consecutive channels of ONE tap of ONE pixel, or
//   8 consecutive k of one filter row: each fragment is one predicated 16-byte global load, no LDS, no barrier.  A pixel (or tap, or
//   padded k) that is predicated off is ZERO in the register — a padded filter zero never meets an unloaded value.
//   The accumulator (col = lane & 15 = pixel, row = 4 (lane >> 4) + reg = channel) leaves a lane four consecutive output channels
//   of one pixel: one 8-byte store after bias and rounding.
// A wave takes 16 consecutive output pixels of one image row and all N output channels (<= 6 accumulators), a workgroup is 4
// independent waves, the grid strides over the 16-pixel groups.  The filter fragments stay in registers across groups where they fit
// (N / 16 * Kp / 32 <= 18 fragments = 72 VGPRs), else they are re-read per group (<= 166 KB of filters: L2 / L1 resident).
//
// mode 0: y[b, oy, ox, n] = bias[n] + sum_k x[b, oy s - 1 + ky, ox s - 1 + kx, c] wp[n][k], Ho = (H - 1) / s + 1.
// mode 1: the input gradient.  x is dY [B, Ho, Wo, Cp], y is dX [B, H, W, N]; wp holds the filter's tap (ky, kx) at position
//   (2 - ky, 2 - kx) (cfhip_conv3x3_direct_pack mode 1), so position (py, px) of pixel (iy, ix) reads dY at
//   ((iy - 1 + py) / s, (ix - 1 + px) / s) = ((iy + 1 - ky) / s, (ix + 1 - kx) / s): only where both numerators are non-negative and
//   divisible by s and the quotients lie inside dY.
#include "common.h"

namespace {

inline int grid_for(long work_items, int per_block, int cap = 2048) {
  long b = (work_items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

template <bool BWD>
__global__ __launch_bounds__(256) void silu_bf16_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ x,
                                                        bf16_t* __restrict__ out, long n) {
  const long n8 = n >> 3;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < n8; i += stride) {
    float v[8];
    ld_act8<false>(x, i << 3, v);
    if (BWD) {
      float d[8];
      ld_act8<false>(a, i << 3, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = d[e] * silu_grad_f(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
    }
    st_bf16x8(out, i << 3, v);
  }
  for (long i = (n8 << 3) + tid; i < n; i += stride) {  // the scalar tail (n % 8 elements)
    const float xv = bf16_to_f32(x[i]);
    out[i] = f32_to_bf16(BWD ? bf16_to_f32(a[i]) * silu_grad_f(xv) : silu_f(xv));
  }
}

// y = bf16(s * x): a ControlNet output times its control scale (ddpm.py:419), and the same launch for its gradient
__global__ __launch_bounds__(256) void scale_bf16_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, long n, float s) {
  const long n8 = n >> 3;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < n8; i += stride) {
    float v[8];
    ld_act8<false>(x, i << 3, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= s;
    st_bf16x8(out, i << 3, v);
  }
  for (long i = (n8 << 3) + tid; i < n; i += stride) out[i] = f32_to_bf16(bf16_to_f32(x[i]) * s);
}

// one thread per element of wp[N][Kp]
__global__ void direct_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int Cout, int Cin, int N, int Cp, int Kp,
                                   int mode) {
  const long total = (long)N * Kp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / Kp), k = (int)(i - (long)n * Kp);
    const int tap = k / Cp, c = k - tap * Cp;
    float v = 0.f;
    if (tap < 9) {
      if (mode == 0) {
        if (c < Cin) v = w[((long)n * Cin + c) * 9 + tap];
      } else if (n < Cin && c < Cout) {
        v = w[((long)c * Cin + n) * 9 + (8 - tap)];  // (2 - ky) * 3 + (2 - kx) = 8 - tap
      }
    }
    wp[i] = f32_to_bf16(v);
  }
}

template <int CP, int NT>
__global__ __launch_bounds__(256) void conv3x3_direct_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                             const float* __restrict__ bias, bf16_t* __restrict__ y, int B,
                                                             int Hin, int Win, int Hout, int Wout, int N, int stride, int mode) {
  constexpr int KP = (9 * CP + 31) / 32 * 32, KS = KP / 32;
  constexpr bool HOIST = NT * KS <= 18;
  const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // the A fragment of k-step s, channel tile nt: filter row 16 nt + col, k = 32 s + 8 q ..
  auto load_a = [&](int nt, int s) -> bf16x8 {
    const int n = 16 * nt + col;
    return n < N ? *reinterpret_cast<const bf16x8*>(wp + (long)n * KP + 32 * s + 8 * q) : zero;
  };
  bf16x8 af[HOIST ? NT * KS : 1];
  if constexpr (HOIST) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int s = 0; s < KS; ++s) af[nt * KS + s] = load_a(nt, s);
  }
  const int gpr = (Wout + 15) >> 4;  // 16-pixel groups per output row
  const long groups = (long)B * Hout * gpr;
  for (long g = blockIdx.x * 4L + (threadIdx.x >> 6); g < groups; g += gridDim.x * 4L) {
    const long r = g / gpr;
    const int ox = (int)(g - r * gpr) * 16 + col, oy = (int)(r % Hout);
    const long b = r / Hout;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k0 = 32 * s + 8 * q, tap = k0 / CP, c0 = k0 - tap * CP;
      const int ty = tap / 3, tx = tap - 3 * ty;
      bool ok = tap < 9 && ox < Wout;
      int sy, sx;
      if (mode == 0) {
        sy = oy * stride - 1 + ty;
        sx = ox * stride - 1 + tx;
      } else {
        const int ny = oy - 1 + ty, nx = ox - 1 + tx;
        ok = ok && ny >= 0 && nx >= 0 && (stride == 1 || ((ny | nx) & 1) == 0);
        sy = stride == 2 ? ny >> 1 : ny;
        sx = stride == 2 ? nx >> 1 : nx;
      }
      ok = ok && sy >= 0 && sy < Hin && sx >= 0 && sx < Win;
      bf16x8 bfrag = zero;
      if (ok) bfrag = *reinterpret_cast<const bf16x8*>(x + ((b * Hin + sy) * Win + sx) * CP + c0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        bf16x8 afrag;
        if constexpr (HOIST) {
          afrag = af[nt * KS + s];
        } else {
          afrag = load_a(nt, s);
        }
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc[nt], 0, 0, 0);
      }
    }
    if (ox < Wout) {
      bf16_t* yp = y + ((b * Hout + oy) * Wout + ox) * N;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n0 = 16 * nt + 4 * q;
        if (n0 < N) {
          f32x4 v = acc[nt];
          if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + n0);
          *reinterpret_cast<u32x2*>(yp + n0) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
      }
    }
  }
}

typedef void (*direct_kernel_t)(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, int, int, int, int);

template <int CP>
direct_kernel_t direct_kernel_for(int nt) {
  switch (nt) {
    case 1: return conv3x3_direct_kernel<CP, 1>;
    case 2: return conv3x3_direct_kernel<CP, 2>;
    case 3: return conv3x3_direct_kernel<CP, 3>;
    case 4: return conv3x3_direct_kernel<CP, 4>;
    case 5: return conv3x3_direct_kernel<CP, 5>;
    default: return conv3x3_direct_kernel<CP, 6>;
  }
}

}  // namespace

extern "C" int cfhip_silu_bf16_fwd(const void* x, void* y, int64_t n, void* stream) {
  CFHIP_REQUIRE(n >= 0 && (n == 0 || (x && y)), "silu_bf16_fwd: bad arguments");
  if (n == 0) return CFHIP_OK;  // an empty tensor: nothing to launch
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "silu_bf16_fwd: misaligned operand");
  hipLaunchKernelGGL((silu_bf16_kernel<false>), dim3(grid_for((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (const bf16_t*)x, (bf16_t*)y, (long)n);
  CFHIP_CHECK_LAUNCH("silu_bf16_fwd");
  return CFHIP_OK;
}

extern "C" int cfhip_silu_bf16_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream) {
  CFHIP_REQUIRE(n >= 0 && (n == 0 || (dy && x && dx)), "silu_bf16_bwd: bad arguments");
  if (n == 0) return CFHIP_OK;  // an empty tensor: nothing to launch
  CFHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx) & 15) == 0, "silu_bf16_bwd: misaligned operand");
  hipLaunchKernelGGL((silu_bf16_kernel<true>), dim3(grid_for((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx, (long)n);
  CFHIP_CHECK_LAUNCH("silu_bf16_bwd");
  return CFHIP_OK;
}

extern "C" int cfhip_scale_bf16(const void* x, void* y, int64_t n, float scale, void* stream) {
  CFHIP_REQUIRE(n >= 0 && (n == 0 || (x && y)), "scale_bf16: bad arguments");
  if (n == 0) return CFHIP_OK;  // an empty tensor: nothing to launch
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "scale_bf16: misaligned operand");
  hipLaunchKernelGGL(scale_bf16_kernel, dim3(grid_for((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (bf16_t*)y, (long)n, scale);
  CFHIP_CHECK_LAUNCH("scale_bf16");
  return CFHIP_OK;
}

extern "C" int cfhip_conv3x3_direct_pack(const float* w, void* wp, int Cout, int Cin, int mode, void* stream) {
  CFHIP_REQUIRE(w && wp && Cout > 0 && Cin > 0, "conv3x3_direct_pack: bad arguments");
  CFHIP_REQUIRE(mode == 0 || mode == 1, "conv3x3_direct_pack: mode %d (0 forward, 1 input gradient)", mode);
  const int N = mode == 0 ? Cout : (Cin + 7) / 8 * 8;
  const int Cp = ((mode == 0 ? Cin : Cout) + 7) / 8 * 8;
  const int Kp = (9 * Cp + 31) / 32 * 32;
  hipLaunchKernelGGL(direct_pack_kernel, dim3(grid_for((long)N * Kp, 256)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)wp,
                     Cout, Cin, N, Cp, Kp, mode);
  CFHIP_CHECK_LAUNCH("conv3x3_direct_pack");
  return CFHIP_OK;
}

extern "C" int cfhip_conv3x3_direct_bf16(const void* x, const void* wp, const float* bias, void* y, int B, int H, int W, int Cp,
                                         int N, int stride, int mode, void* stream) {
  CFHIP_REQUIRE(x && wp && y && B > 0 && H > 0 && W > 0, "conv3x3_direct_bf16: bad arguments");
  CFHIP_REQUIRE(stride == 1 || stride == 2, "conv3x3_direct_bf16: stride %d (1 or 2)", stride);
  CFHIP_REQUIRE(mode == 0 || mode == 1, "conv3x3_direct_bf16: mode %d (0 forward, 1 input gradient)", mode);
  CFHIP_REQUIRE(Cp == 8 || Cp == 16 || Cp == 24 || Cp == 32 || Cp == 48 || Cp == 64 || Cp == 80 || Cp == 96,
                "conv3x3_direct_bf16: Cp = %d (8, 16, 24, 32, 48, 64, 80 or 96)", Cp);
  CFHIP_REQUIRE(N >= 8 && N <= 96 && N % 8 == 0, "conv3x3_direct_bf16: N = %d (a multiple of 8 up to 96)", N);
  CFHIP_REQUIRE(H < (1 << 24) && W < (1 << 24), "conv3x3_direct_bf16: image %d x %d too large", H, W);
  CFHIP_REQUIRE((((uintptr_t)x | (uintptr_t)wp | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, "conv3x3_direct_bf16: misaligned operand");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  // (Hin, Win): the image `x` holds; (Hout, Wout): the image `y` receives
  const int Hin = mode == 0 ? H : Ho, Win = mode == 0 ? W : Wo, Hout = mode == 0 ? Ho : H, Wout = mode == 0 ? Wo : W;
  const int nt = (N + 15) / 16;
  const direct_kernel_t kernel = Cp == 8    ? direct_kernel_for<8>(nt)
                                 : Cp == 16 ? direct_kernel_for<16>(nt)
                                 : Cp == 24 ? direct_kernel_for<24>(nt)
                                 : Cp == 32 ? direct_kernel_for<32>(nt)
                                 : Cp == 48 ? direct_kernel_for<48>(nt)
                                 : Cp == 64 ? direct_kernel_for<64>(nt)
                                 : Cp == 80 ? direct_kernel_for<80>(nt)
                                            : direct_kernel_for<96>(nt);
  const long groups = (long)B * Hout * ((Wout + 15) / 16);
  hipLaunchKernelGGL(kernel, dim3(grid_for(groups, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)wp, bias,
                     (bf16_t*)y, B, Hin, Win, Hout, Wout, N, stride, mode);
  CFHIP_CHECK_LAUNCH("conv3x3_direct_bf16");
  return CFHIP_OK;
}
