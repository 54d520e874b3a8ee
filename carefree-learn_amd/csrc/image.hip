// The uint8 image input path for gfx950: crop + resize + flip + normalize + HWC -> CHW in ONE launch.  Replaces the per-item CPU blocks of the
// reference's data/blocks/cv/ (resize.py, crop.py, normalize.py: static_normalize / affine_normalize / imagenet_normalize, hwc_to_chw.py)
// for batches that cross PCIe as uint8 [B][Hs][Ws][C] and leave this kernel as the f32 / bf16 [B][C][Ho][Wo] tensor the model takes.
//
// Sampling rule, per output pixel (oy, ox) of sample b with box (y0, x0, h, w) -- every operation below is ONE f32 operation, rounded to
// nearest, never contracted into an fma (the file is compiled with fp contraction off), so that a host restatement in f32 reproduces the
// coordinates bit for bit and the two routes below agree bit for bit:
//   ky = h / Ho, kx = w / Wo                                        (IEEE division)
//   oxf = flip ? Wo - 1 - ox : ox
//   sy = (y0 + (oy + 0.5) * ky) - 0.5,  sx = (x0 + (oxf + 0.5) * kx) - 0.5        half-pixel centres
//   bilinear: iy = floor(sy), fy = sy - iy, taps iy and iy + 1 clamped to [0, Hs - 1] of the WHOLE image (replicate border, not the
//             box), weights wy1 = fy, wy0 = 1 - fy; the same in x;
//             w00 = wy0 wx0, w01 = wy0 wx1, w10 = wy1 wx0, w11 = wy1 wx1;  v = ((v00 w00 + v01 w01) + v10 w10) + v11 w11
//   nearest:  iy = floor(sy + 0.5) clamped, ix likewise; v = the tap
//   out = v * a[c] + b[c]   (one product, one sum), then ONE rounding to bf16 when the destination is bf16.
// A box with integer origin and h == Ho, w == Wo has ky = kx = 1, fy = fx = 0 and the weights 1, 0, 0, 0 exactly: out = value * a + b.
//
// Work split.  One workgroup (256 lanes) = one (sample, 32 x 32 output tile) for all C channels; lane t owns column t & 31 and rows
// (t >> 5) + 8 p, p = 0 .. 3: lanes run along x, every store to an NCHW plane is a 32-pixel row segment.
//   route 0 (LDS tiled): the workgroup maps the tile's four corner pixels through the rule above -- the coordinates are monotone in oy and
//     ox, so their taps bound every tap of the tile --, and stages the footprint rows [ty0 .. ty1] x bytes [tx0 C .. (tx1 + 1) C) into LDS.
//     A footprint row is contiguous in HWC: it moves as 16-byte chunks aligned in GLOBAL memory (consecutive lanes take consecutive chunks);
//     the row sits in LDS at the same offset mod 16 as in global memory, so the LDS side of each chunk is aligned as well; the chunks that
//     hold the row's first and last bytes (Ws C = 51 bytes per row puts them anywhere) move byte by byte, and only the bytes of the
//     footprint are ever read.  Then each lane takes its 4 (or 1) taps per channel from LDS.  A tile whose footprint does not fit in
//     IMG_LDS bytes takes its taps from global memory instead (a workgroup-uniform branch): whatever boxes the device buffer holds, LDS
//     is never overrun.
//   route 1 (direct gather): no LDS at all, every tap is a global byte load through the same device function.  For strong downscales,
//     where a 32 x 32 tile covers more source than LDS holds and most of it is never sampled.
// The route is chosen per launch, on the host, from the boxes the host drew (cfhip_image_transform_plan): the bound is what a full tile
// can cover at the largest scale of the batch, (ceil(32 ky) + 2) rows of (ceil(32 kx) + 2) C + 15 bytes rounded up to 16.
// No atomics, no scratch, no grid-wide synchronisation.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int IMG_TILE = 32;
constexpr int IMG_LDS = CFHIP_IMAGE_LDS_BYTES;

struct ImageArgs {
  const uint8_t* src;
  long stride_b, stride_row;  // bytes
  int B, Hs, Ws, C;
  const float* boxes;
  const uint8_t* flips;
  const float* scale_bias;
  void* dst;
  int dst_bf16, Ho, Wo, interp;
  int tiles_x, tiles_y;
};

// one axis of the rule: output index o (already mirrored) -> taps i0 <= i1 in [0, n - 1] and the weight of i1
__device__ __forceinline__ void img_axis(float origin, float k, int o, int n, int interp, int& i0, int& i1, float& w1) {
  const float s = (origin + ((float)o + 0.5f) * k) - 0.5f;
  // clamped as a float first (a NaN becomes -1): the conversion to int below is then defined whatever the box holds
  const float fl = fminf(fmaxf(floorf(interp ? s : s + 0.5f), -1.0f), (float)n);
  const int i = (int)fl;
  i0 = min(max(i, 0), n - 1);
  i1 = interp ? min(max(i + 1, 0), n - 1) : i0;
  w1 = interp ? s - floorf(s) : 0.0f;
  if (!(w1 >= 0.0f && w1 <= 1.0f)) w1 = 0.0f;  // a non-finite coordinate (refused on the host; a device buffer can hold anything)
}

// the pixel's C values from taps at byte offsets o00 .. o11 of `base` (LDS or global: the SAME arithmetic either way)
template <typename P>
__device__ __forceinline__ void img_blend(P base, long o00, long o01, long o10, long o11, float wy1, float wx1, int interp, int C, float (&v)[4]) {
  if (interp) {
    const float wy0 = 1.0f - wy1, wx0 = 1.0f - wx1;
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        const float v00 = (float)base[o00 + c], v01 = (float)base[o01 + c], v10 = (float)base[o10 + c], v11 = (float)base[o11 + c];
        v[c] = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
      }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) v[c] = (float)base[o00 + c];
  }
}

template <bool LDS>
__global__ __launch_bounds__(256) void image_transform_kernel(const ImageArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[LDS ? IMG_LDS : 16];
  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int oy0 = (t / a.tiles_x) * IMG_TILE, ox0 = (t % a.tiles_x) * IMG_TILE;
  const int C = a.C, Hs = a.Hs, Ws = a.Ws, Ho = a.Ho, Wo = a.Wo, interp = a.interp;
  const float by = a.boxes[4 * b], bx = a.boxes[4 * b + 1];
  const float ky = a.boxes[4 * b + 2] / (float)Ho, kx = a.boxes[4 * b + 3] / (float)Wo;
  const bool flip = a.flips != nullptr && a.flips[b] != 0;
  const uint8_t* img = a.src + (long)b * a.stride_b;

  // the footprint from the tile's corner pixels
  bool staged = false;
  int ty0 = 0, tx0 = 0, pitch = 0, fh = 1, fw = 1;
  if (LDS) {
    const int oy1 = min(oy0 + IMG_TILE, Ho) - 1, ox1 = min(ox0 + IMG_TILE, Wo) - 1;
    int p0, p1, q0, q1;
    float w;
    img_axis(by, ky, oy0, Hs, interp, p0, p1, w);
    img_axis(by, ky, oy1, Hs, interp, q0, q1, w);
    ty0 = min(p0, q0);
    const int ty1 = max(p1, q1);
    img_axis(bx, kx, flip ? Wo - 1 - ox0 : ox0, Ws, interp, p0, p1, w);
    img_axis(bx, kx, flip ? Wo - 1 - ox1 : ox1, Ws, interp, q0, q1, w);
    tx0 = min(p0, q0);
    const int tx1 = max(p1, q1);
    fh = ty1 - ty0 + 1, fw = tx1 - tx0 + 1;
    const int fbytes = fw * C;
    pitch = (fbytes + 15 + 15) & ~15;
    staged = (long)fh * pitch <= IMG_LDS;
    if (staged) {
      const int chunks = pitch >> 4;
      for (int i = tid; i < fh * chunks; i += 256) {
        const int r = i / chunks, j = i - r * chunks;
        const uint8_t* g0 = img + (long)(ty0 + r) * a.stride_row + (long)tx0 * C;  // the row's first footprint byte
        const int sh = (int)((uintptr_t)g0 & 15);
        const int lo = j * 16 - sh;  // the chunk's first byte, relative to g0
        if (lo >= fbytes) continue;
        uint8_t* l = tile + r * pitch + j * 16;
        if (lo >= 0 && lo + 16 <= fbytes) {
          *reinterpret_cast<u32x4*>(l) = *reinterpret_cast<const u32x4*>(g0 + lo);
        } else {
          for (int e = max(lo, 0); e < min(lo + 16, fbytes); ++e) l[e - lo] = g0[e];  // head or tail: only bytes of the footprint
        }
      }
    }
    __syncthreads();
  }

  const int ox = ox0 + (tid & 31);
  if (ox >= Wo) return;
  int x0i, x1i;
  float wx1;
  img_axis(bx, kx, flip ? Wo - 1 - ox : ox, Ws, interp, x0i, x1i, wx1);
  float sa[4], sb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sa[c] = c < C ? a.scale_bias[2 * c] : 0.0f;
    sb[c] = c < C ? a.scale_bias[2 * c + 1] : 0.0f;
  }
  const long plane = (long)Ho * Wo;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int oy = oy0 + (tid >> 5) + 8 * p;
    if (oy >= Ho) break;
    int y0i, y1i;
    float wy1;
    img_axis(by, ky, oy, Hs, interp, y0i, y1i, wy1);
    float v[4];
    if (LDS && staged) {
      // row r of the footprint starts at the offset its first byte has mod 16 in global memory
      // (every tap lies inside the footprint by monotonicity; the clamps make that independent of the argument)
      const int r0 = min(max(y0i - ty0, 0), fh - 1), r1 = min(max(y1i - ty0, 0), fh - 1);
      const int s0 = (int)((uintptr_t)(img + (long)y0i * a.stride_row + (long)tx0 * C) & 15);
      const int s1 = (int)((uintptr_t)(img + (long)y1i * a.stride_row + (long)tx0 * C) & 15);
      const int c0 = min(max(x0i - tx0, 0), fw - 1) * C, c1 = min(max(x1i - tx0, 0), fw - 1) * C;
      const uint8_t* lt = tile;
      img_blend(lt, (long)(r0 * pitch + s0 + c0), (long)(r0 * pitch + s0 + c1), (long)(r1 * pitch + s1 + c0), (long)(r1 * pitch + s1 + c1), wy1,
                wx1, interp, C, v);
    } else {
      const long rb0 = (long)y0i * a.stride_row, rb1 = (long)y1i * a.stride_row;
      img_blend(img, rb0 + (long)x0i * C, rb0 + (long)x1i * C, rb1 + (long)x0i * C, rb1 + (long)x1i * C, wy1, wx1, interp, C, v);
    }
    const long at = (long)b * C * plane + (long)oy * Wo + ox;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        const float o = v[c] * sa[c] + sb[c];
        if (a.dst_bf16)
          reinterpret_cast<bf16_t*>(a.dst)[at + c * plane] = f32_to_bf16(o);
        else
          reinterpret_cast<float*>(a.dst)[at + c * plane] = o;
      }
  }
}

bool image_shape_ok(int B, int Hs, int Ws, int C, int Ho, int Wo, int interp, const char* who) {
  if (C < 1 || C > CFHIP_IMAGE_MAX_CHANNELS) {
    cfhip_set_error("%s: C = %d channels is outside the kernel (1 .. %d)", who, C, CFHIP_IMAGE_MAX_CHANNELS);
    return false;
  }
  if (Ho < 1 || Wo < 1 || Ho > 32768 || Wo > 32768) {
    cfhip_set_error("%s: output size %d x %d (1 .. 32768 each)", who, Ho, Wo);
    return false;
  }
  if (B < 1 || Hs < 1 || Ws < 1 || Hs > 32768 || Ws > 32768) {
    cfhip_set_error("%s: B = %d, source size %d x %d (B >= 1, 1 .. 32768 each)", who, B, Hs, Ws);
    return false;
  }
  const long tiles = (long)((Ho + IMG_TILE - 1) / IMG_TILE) * ((Wo + IMG_TILE - 1) / IMG_TILE);
  if (tiles * B >= 0x7fffffffL) {
    cfhip_set_error("%s: B = %d times %ld tiles does not fit one launch", who, B, tiles);
    return false;
  }
  if (interp != 0 && interp != 1) {
    cfhip_set_error("%s: interp = %d (0 nearest, 1 bilinear)", who, interp);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int cfhip_image_transform_plan(const float* host_boxes, int B, int Hs, int Ws, int C, int Ho, int Wo, int interp) {
  if (!image_shape_ok(B, Hs, Ws, C, Ho, Wo, interp, "image_transform_plan")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(host_boxes != nullptr, "image_transform_plan: null boxes");
  float ky = 0.f, kx = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* q = host_boxes + 4 * b;
    CFHIP_REQUIRE(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && isfinite(q[3]), "image_transform_plan: box %d is not finite", b);
    CFHIP_REQUIRE(q[2] > 0.f && q[3] > 0.f, "image_transform_plan: box %d is empty (h = %g, w = %g)", b, (double)q[2], (double)q[3]);
    ky = fmaxf(ky, q[2] / (float)Ho);
    kx = fmaxf(kx, q[3] / (float)Wo);
  }
  // what a full tile can cover at the batch's largest scale: rows, and bytes per row as LDS holds them
  const double rows = ceil((double)IMG_TILE * ky) + 2.0, cols = ceil((double)IMG_TILE * kx) + 2.0;
  const double pitch = floor((cols * C + 30.0) / 16.0) * 16.0;
  return rows * pitch <= (double)IMG_LDS ? CFHIP_IMAGE_ROUTE_LDS : CFHIP_IMAGE_ROUTE_GATHER;
}

extern "C" int cfhip_image_transform(const uint8_t* src, int64_t src_stride_b, int64_t src_stride_row, int B, int Hs, int Ws, int C,
                                     const float* boxes, const uint8_t* flips, const float* scale_bias, void* dst, int dst_bf16, int Ho, int Wo,
                                     int interp, int route, void* stream) {
  if (!image_shape_ok(B, Hs, Ws, C, Ho, Wo, interp, "image_transform")) return CFHIP_ERR_INVALID;
  CFHIP_REQUIRE(src && boxes && scale_bias && dst, "image_transform: null operand");
  CFHIP_REQUIRE(route == CFHIP_IMAGE_ROUTE_LDS || route == CFHIP_IMAGE_ROUTE_GATHER, "image_transform: route = %d (0 LDS tiled, 1 gather)", route);
  CFHIP_REQUIRE(dst_bf16 == 0 || dst_bf16 == 1, "image_transform: dst_bf16 = %d", dst_bf16);
  CFHIP_REQUIRE(src_stride_row >= (int64_t)Ws * C && (B == 1 || src_stride_b >= (Hs - 1) * src_stride_row + (int64_t)Ws * C),
                "image_transform: strides %lld / %lld bytes overlap rows of %d x %d bytes", (long long)src_stride_b, (long long)src_stride_row,
                Ws, C);
  CFHIP_REQUIRE((((uintptr_t)boxes | (uintptr_t)scale_bias) & 3) == 0 && ((uintptr_t)dst & (dst_bf16 ? 1 : 3)) == 0,
                "image_transform: misaligned operand");
  ImageArgs a{};
  a.src = src, a.stride_b = src_stride_b, a.stride_row = src_stride_row, a.B = B, a.Hs = Hs, a.Ws = Ws, a.C = C;
  a.boxes = boxes, a.flips = flips, a.scale_bias = scale_bias, a.dst = dst, a.dst_bf16 = dst_bf16, a.Ho = Ho, a.Wo = Wo, a.interp = interp;
  a.tiles_x = (Wo + IMG_TILE - 1) / IMG_TILE, a.tiles_y = (Ho + IMG_TILE - 1) / IMG_TILE;
  const unsigned grid = (unsigned)((long)B * a.tiles_x * a.tiles_y);
  if (route == CFHIP_IMAGE_ROUTE_LDS)
    hipLaunchKernelGGL(image_transform_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(image_transform_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  CFHIP_CHECK_LAUNCH("image_transform");
  return CFHIP_OK;
}
