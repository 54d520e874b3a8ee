// Wide-head attention forward: one head of 192 < head_dim <= 512 channels — the single-head SpatialAttention at the bottleneck
// of the KL autoencoder (reference attentions.py:330-370; the zoo autoencoder has C = 512 there).  No mask, not causal, no
// dropout, no backward: the first stage of a latent-diffusion model is frozen.
//
// The general forward of csrc/attn.hip (`attn_gen_fwd_kernel`) with the head dimension carried on to NH = ceil(dh / 64) = 4..8
// zero-padded 64-column halves, built from the same parts (csrc/attn_device.h): workgroup = (128-row query chunk, head, batch),
// eight waves, one 16-row query tile per wave; K and V stream through LDS in chunks of 64 keys (32 at NH = 8), each half an ordinary
// swizzled [64][64] tile (2 x NH x 8 KiB: 112 KiB at NH = 7, 64 KiB at NH = 8; one workgroup per CU); online softmax across the chunks; the same
// operand order, the same roundings (S in f32 from bf16 products, P rounded to bf16 before P V) as the general kernels, so the
// error model of their tests holds unchanged.
//
// Registers are what shapes it: the f32 accumulator of a 16 x 512 tile is 128 registers per lane and the Q fragments another
// 64, so the kernels are built for two waves per SIMD (256 registers per lane) instead of the four of the 64-wide forward, and
// the key chunk is 64 or 32 rows (16 / 8 score registers) instead of 128 / 256.  No scratch.
#include "common.h"
#include "attn_device.h"

namespace {

// keys per staged chunk: 64 (16 score registers per lane), 32 at NH = 8, where 64 leaves the compiler 9 registers short of the 256
template <int NH>
constexpr int WIDE_CH = NH == 8 ? CFHIP_ATTN_WIDE_CHUNK / 2 : CFHIP_ATTN_WIDE_CHUNK;
constexpr int WIDE_WAVES = 8;                   // 16-row query tiles per workgroup

struct WideParams {
  const bf16_t* q; const bf16_t* k; const bf16_t* v;
  bf16_t* o;
  float* lse;
  int B, H, Tq, Tk;
  long q_sb, q_st, kv_sb, kv_st, o_sb, o_st;
  float scale;
  int dh;
};

template <int NH>
__global__ __launch_bounds__(WIDE_WAVES * 64, 2) void wide_attn_fwd_kernel(WideParams p) {
  constexpr int CH = WIDE_CH<NH>;
  constexpr int HALF_BYTES = CH * 128;
  constexpr int OPER_BYTES = NH * HALF_BYTES;
  constexpr int CHB = CH / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + OPER_BYTES;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int dh = p.dh;
  const bf16_t* kb = p.k + (long)b * p.kv_sb + (long)h * dh;
  const bf16_t* vb = p.v + (long)b * p.kv_sb + (long)h * dh;
  const bf16_t* qb = p.q + (long)b * p.q_sb + (long)h * dh;
  const int row0 = (blockIdx.x * WIDE_WAVES + wave) * 16;
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

  for (int kv0 = 0; kv0 < p.Tk; kv0 += CH) {
    __syncthreads();  // every wave is done with the previous chunk
    {
      const int rows_ = min(CH, p.Tk - kv0);
      int ln = lane;  // opaque copy: the per-lane DMA offsets are recomputed per chunk instead of being kept alive across it
      asm volatile("" : "+v"(ln));
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) {
        dma_half(Ks + hf * HALF_BYTES, kb + (long)kv0 * p.kv_st, p.kv_st, rows_, CH, hf, dh, wave, WIDE_WAVES, ln);
        dma_half(Vs + hf * HALF_BYTES, vb + (long)kv0 * p.kv_st, p.kv_st, rows_, CH, hf, dh, wave, WIDE_WAVES, ln);
      }
    }
    lds_dma_wait_all();
    __syncthreads();
    if (!active) continue;
    f32x4 st[2 * CHB];
#pragma unroll
    for (int jt = 0; jt < 2 * CHB; ++jt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2 * NH; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(Ks + (ks >> 1) * HALF_BYTES, jt * 16, ks & 1, lane), qf[ks], acc, 0, 0, 0);
      st[jt] = acc;
    }
    float mx = -INFINITY;
    const bool tail = kv0 + CH > p.Tk;  // wave-uniform: only the last chunk needs the j < Tk test
#pragma unroll
    for (int jt = 0; jt < 2 * CHB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kv0 + jt * 16 + 4 * g + r;
        float x = st[jt][r] * sl2;
        if (tail) x = j < p.Tk ? x : -INFINITY;
        st[jt][r] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = group_max(mx);
    const float m_new = fmaxf(m, mx);
    // a row without a finite score so far (m_new = -inf) must not produce NaN from (-inf) - (-inf): the guard of the general forward
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_use);  // m = -inf on the first chunk: 0
    float ls = 0.f;
#pragma unroll
    for (int jt = 0; jt < 2 * CHB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(st[jt][r] - m_use);
        st[jt][r] = e;
        ls += e;
      }
    }
    l = l * alpha + group_sum(ls);
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) ot[dt] *= alpha;
#pragma unroll
    for (int a = 0; a < CHB; ++a) {
      const bf16x8 pa = pack8(st[2 * a], st[2 * a + 1]);
#pragma unroll
      for (int dt = 0; dt < 4 * NH; ++dt)
        ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols(Vs + (dt >> 2) * HALF_BYTES, a * 32, (dt & 3) * 16, lane), pa,
                                                         ot[dt], 0, 0, 0);
    }
  }
  if (active && qi < p.Tq) {
    const float inv = 1.0f / l;
    bf16_t* orow = p.o + (long)b * p.o_sb + (long)qi * p.o_st + (long)h * dh;
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

template <int NH>
int launch_wide(const WideParams& p, hipStream_t s) {
  const size_t lds = (size_t)2 * NH * WIDE_CH<NH> * 128;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(wide_attn_fwd_kernel<NH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      cfhip_set_error("attn_wide_fwd: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
      return CFHIP_ERR_LAUNCH;
    }
  }
  const dim3 grid((p.Tq + WIDE_WAVES * 16 - 1) / (WIDE_WAVES * 16), p.H, p.B);
  hipLaunchKernelGGL(wide_attn_fwd_kernel<NH>, grid, dim3(WIDE_WAVES * 64), lds, s, p);
  CFHIP_CHECK_LAUNCH("attn_wide_fwd");
  return CFHIP_OK;
}

}  // namespace

extern "C" int cfhip_attn_wide_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Tq,
                                   int Tk, int head_dim, int64_t q_stride_b, int64_t q_stride_t, int64_t kv_stride_b,
                                   int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t, float scale, void* stream) {
  CFHIP_REQUIRE(head_dim > 192 && head_dim <= CFHIP_ATTN_WIDE_MAX_HEAD_DIM && head_dim % 8 == 0,
                "attn_wide_fwd: head_dim %d is not a multiple of 8 in (192, %d] (up to 192: cfhip_attn_fwd_dh)", head_dim,
                CFHIP_ATTN_WIDE_MAX_HEAD_DIM);
  CFHIP_REQUIRE(q && k && v && o, "attn_wide_fwd: null q/k/v/o");
  CFHIP_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "attn_wide_fwd: empty problem");
  CFHIP_REQUIRE(B <= 65535 && H <= 65535, "attn_wide_fwd: B = %d / H = %d exceed the grid limits", B, H);
  CFHIP_REQUIRE(q_stride_b % 8 == 0 && q_stride_t % 8 == 0 && kv_stride_b % 8 == 0 && kv_stride_t % 8 == 0 &&
                    o_stride_b % 8 == 0 && o_stride_t % 8 == 0,
                "attn_wide_fwd: strides must be multiples of 8 elements");
  CFHIP_REQUIRE(q_stride_t >= (int64_t)H * head_dim && kv_stride_t >= (int64_t)H * head_dim && o_stride_t >= (int64_t)H * head_dim,
                "attn_wide_fwd: a token stride is smaller than H * head_dim = %lld", (long long)H * head_dim);
  // the DMA addresses a chunk's rows with 32-bit byte offsets from the chunk's first row
  CFHIP_REQUIRE(kv_stride_t * 2 * CFHIP_ATTN_WIDE_CHUNK < 0x7fffffffLL, "attn_wide_fwd: kv token stride %lld too large", (long long)kv_stride_t);
  CFHIP_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)o & 7) == 0 &&
                    ((uintptr_t)lse & 3) == 0,
                "attn_wide_fwd: q/k/v must be 16-byte, o 8-byte, lse 4-byte aligned");
  WideParams p = {};
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o;
  p.lse = lse;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk;
  p.q_sb = q_stride_b; p.q_st = q_stride_t; p.kv_sb = kv_stride_b; p.kv_st = kv_stride_t;
  p.o_sb = o_stride_b; p.o_st = o_stride_t;
  p.scale = scale;
  p.dh = head_dim;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch ((head_dim + 63) / 64) {
    case 4: return launch_wide<4>(p, s);
    case 5: return launch_wide<5>(p, s);
    case 6: return launch_wide<6>(p, s);
    case 7: return launch_wide<7>(p, s);
    default: return launch_wide<8>(p, s);
  }
}
