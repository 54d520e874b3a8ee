// Reverse diffusion: the per-step arithmetic of the reference's DDIM and ancestral ("basic") samplers
// (multimodal/diffusion/samplers/ddim.py:195-239, basic.py:61-92, schema.py:197-263 for classifier-free guidance,
// ddpm.py:298-300 for the final clamp) as ONE launch per step, plus the standard-normal generator of the starting noise
// (ddpm.py:264-266).
//
// Every scalar a step needs (sqrt(a_t), the DDIM direction coefficient, the posterior coefficients, ...) is formed once on the
// host with the reference's f32 operation order and stored as row k of a [steps][8] f32 table; the step counter k lives in
// device memory, so a recorded step (hipGraph) replays unchanged: `advance` bumps k and writes the next row's timestep into
// the UNet's int64 timesteps buffer.  The arithmetic below keeps the reference's roundings (no FMA contraction, IEEE
// division): given the same model output and noise the f32 state matches the reference's CPU run.
//
// Noise xi: Philox4x32-10 at counter (seed, offset + k * total4 + i / 4), Box-Muller, four normals per counter; or an
// explicit f32 bank [steps][B * n] (the parity tests' hook).  The starting noise z is the same stream at "step -1": the
// host draws it with cfhip_randn_f32 at `offset - total4`.
//
// The sigma-space "K" samplers (samplers/k_samplers.py: k_euler_a, k_heun, k_dpmpp_2m) run on the same step kernel and advance:
// one launch per MODEL EVALUATION, rows of CFHIP_KSAMPLE_ROW scalars, an f32 auxiliary buffer, xin = bf16(next input * c_in).
#include "common.h"

namespace {

inline int grid_for(long work_items, int per_block, int cap = 2048) {
  long b = (work_items + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// uniform in (0, 1] with 24 random bits: log(u) is finite
__device__ __forceinline__ float u01_open0(unsigned r) { return (float)((r >> 8) + 1u) * (1.0f / 16777216.0f); }

// four standard normals out of one Philox call: Box-Muller on (c0, c1) and on (c2, c3)
__device__ __forceinline__ f32x4 normal4(unsigned long long ctr, unsigned long long seed) {
  const Philox r = philox4x32_10(ctr, seed);
  f32x4 z;
  {
    const float rad = sqrtf(-2.0f * logf(u01_open0(r.c[0])));
    float s, c;
    sincospif(2.0f * u01_open0(r.c[1]), &s, &c);
    z[0] = rad * c;
    z[1] = rad * s;
  }
  {
    const float rad = sqrtf(-2.0f * logf(u01_open0(r.c[2])));
    float s, c;
    sincospif(2.0f * u01_open0(r.c[3]), &s, &c);
    z[2] = rad * c;
    z[3] = rad * s;
  }
  return z;
}

__global__ void randn_kernel(float* __restrict__ out, long n, unsigned long long seed, unsigned long long offset) {
  const long n4 = (n + 3) >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < n4; i4 += stride) {
    const f32x4 z = normal4(offset + (unsigned long long)i4, seed);
    const long base = i4 << 2;
    if (base + 3 < n) {
      *reinterpret_cast<f32x4*>(out + base) = z;
    } else {
      for (int e = 0; e < 4 && base + e < n; ++e) out[base + e] = z[e];
    }
  }
}

// z = scale_factor * (mean + exp(0.5 clamp(log_var, -30, 20)) * n) from the moments [B][2E][hw] (NCHW) or [B][hw][2E] (channels
// last) of the KL autoencoder's posterior (cv/ae/kl.py:18-36 with the scale_factor of ldm.py:183-190); n: an explicit f32
// tensor, nothing (`deterministic`: the mode), or the normal of randn_kernel at the same flat output index (counter offset +
// index / 4, component index % 4).  grid = (blocks, B): the blocks of sample b walk the groups of four flat indices that
// overlap the sample (a group that straddles two samples is drawn by both, each taking its own elements).  kl (optional):
// kl[b] = 0.5 sum (mean^2 + var - 1 - log_var) (kl.py:38-45), reduced in a fixed order by the ONE block per sample that the
// host launches when it is asked for: deterministic.
__global__ __launch_bounds__(256) void gaussian_posterior_kernel(const bf16_t* __restrict__ mom, int channels_last,
                                                                  float* __restrict__ z, float* __restrict__ kl,
                                                                  const float* __restrict__ noise, int deterministic, int E,
                                                                  long hw, float scale_factor, unsigned long long seed,
                                                                  unsigned long long offset) {
  __shared__ float part[4];
  const long b = blockIdx.y;
  const long n = (long)E * hw;
  const long lo = b * n, hi = lo + n;
  const long g_lo = lo >> 2, g_hi = (hi - 1) >> 2;
  const bool draw = !deterministic && noise == nullptr && z != nullptr;
  float acc = 0.f;
  for (long g4 = g_lo + blockIdx.x * (long)blockDim.x + threadIdx.x; g4 <= g_hi; g4 += (long)gridDim.x * blockDim.x) {
    f32x4 xi = {0.f, 0.f, 0.f, 0.f};
    if (draw) xi = normal4(offset + (unsigned long long)g4, seed);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long idx = (g4 << 2) + e;
      if (idx < lo || idx >= hi) continue;
      const long j = idx - lo;
      const long c = j / hw, pix = j - c * hw;
      const long at = channels_last ? (b * hw + pix) * (2 * E) + c : (b * 2 * E + c) * hw + pix;
      const float mean = bf16_to_f32(mom[at]);
      float lv = bf16_to_f32(mom[at + (channels_last ? (long)E : (long)E * hw)]);
      lv = fminf(fmaxf(lv, -30.0f), 20.0f);
      if (z != nullptr) {
        if (deterministic) {
          z[idx] = scale_factor * mean;
        } else {
          const float nrm = noise != nullptr ? noise[idx] : xi[e];
          z[idx] = scale_factor * (mean + expf(0.5f * lv) * nrm);
        }
      }
      if (kl != nullptr) acc += mean * mean + expf(lv) - 1.0f - lv;
    }
  }
  if (kl != nullptr) {  // (gridDim.x == 1)
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) kl[b] = 0.5f * (((part[0] + part[1]) + part[2]) + part[3]);
  }
}

// ---- the sampler step: one kernel walk, one rule per sampler ----------------------------------
// No FMA contraction from here on: the reference's f32 roundings (normal4, parsed above, keeps its own options when inlined).
#pragma clang fp contract(off)

// the operands of one step launch
struct StepParams {
  float *x, *aux;
  bf16_t* xin;
  const bf16_t *out_c, *out_u;
  const float *table, *bank;
  const int* kp;
  float scale, temperature;
  int rows, param, clip_last, dup;
  unsigned long long seed, offset;
  long total4;
};

// A rule is one sampler's update.  It is built from row k of the table (ROW scalars; column 0, the timestep, is the advance
// kernel's), says what this row does, and maps one element: apply(x, aux, next, m, xi) takes the state, the auxiliary value,
// the guided model output and the draw, and leaves the new state, the new auxiliary value and `next`, the image of the next
// model evaluation.  SCALES_INPUT: xin = bf16(next * c_in) instead of bf16(next).
struct RowActs { bool draws = false, reads_aux = false, writes_aux = false, writes_x = true; };

// DDIM and basic: one row per step, every row draws
struct StepRule : RowActs {
  static constexpr int ROW = CFHIP_SAMPLE_ROW;
  static constexpr bool SCALES_INPUT = false;
  float c1, c2, c3, c4, c5, c6, c7, temperature;
  int param;
  __device__ StepRule(const float* r, const StepParams& p)
      : c1(r[1]), c2(r[2]), c3(r[3]), c4(r[4]), c5(r[5]), c6(r[6]), c7(r[7]), temperature(p.temperature), param(p.param) {
    draws = true;
  }
};

// ddim.py:195-239.  c1 sqrt(a_t), c2 sqrt(1 - a_t), c3 sqrt(a_prev), c4 sqrt(1 - a_prev - sigma^2), c5 sigma, c6 / c7 sqrt(ac[t]) /
// sqrt(1 - ac[t]) of the DDPM schedule (v-parameterization, ddpm.py:461-484)
struct DdimRule : StepRule {
  using StepRule::StepRule;
  __device__ void apply(float& x, float&, float& next, float m, float xi) const {
    float eps, x0;
    if (param == CFHIP_PARAM_V) {
      eps = c6 * m + c7 * x;
      x0 = c6 * x - c7 * m;
    } else {
      eps = m;
      x0 = (x - c2 * eps) / c1;
    }
    const float dir = c4 * eps;
    const float noise = c5 * xi * temperature;
    x = next = c3 * x0 + dir + noise;
  }
};

// basic.py:61-92.  c1 / c2 posterior_coef1 / 2 [t], c3 [t > 0] exp(0.5 posterior_log_variance_clipped[t])
struct BasicRule : StepRule {
  using StepRule::StepRule;
  __device__ void apply(float& x, float&, float& next, float m, float xi) const {
    const float mean = param == CFHIP_PARAM_X0 ? m : c1 * (x - c2 * m);
    const float noise = xi * temperature;
    x = next = mean + c3 * noise;
  }
};

// The sigma-space ("K") rules (samplers/k_samplers.py): one row per MODEL EVALUATION (Heun spends two rows per step).
//   1 sigma      of this evaluation's input           2 c_out, 3 c_skip   of get_denoised at sigma (k_samplers.py:152-183)
//   4 c_in       of the NEXT evaluation's input
//   5 dt         sigma_down - sigma (euler_a), next_sigma - sigma (heun, both rows of a step)
//   6 sigma_up   (euler_a)                            7 sigma_next / sigma, 8 expm1(-h), 9 1 + 1 / (2 r), 10 1 / (2 r) (dpmpp_2m)
//   11 flag      euler_a: next_sigma > 0 (the draw is added); heun: 0 = stage 1, 1 = stage 2; dpmpp_2m: 1 = old_denoised exists
// aux: heun's d between its two stages, dpmpp_2m's old_denoised; euler_a does not touch it.
struct KRule : RowActs {
  static constexpr int ROW = CFHIP_KSAMPLE_ROW;
  static constexpr bool SCALES_INPUT = true;
  float sigma, c_out, c_skip, c_in, dt, sigma_up, ratio, em1, r1, r2;
  bool flag, v;
  __device__ KRule(const float* r, const StepParams& p)
      : sigma(r[1]), c_out(r[2]), c_skip(r[3]), c_in(r[4]), dt(r[5]), sigma_up(r[6]), ratio(r[7]), em1(r[8]), r1(r[9]), r2(r[10]),
        flag(r[11] != 0.0f), v(p.param == CFHIP_PARAM_V) {}
  __device__ float denoised(float img, float m) const { return v ? img * c_skip - m * c_out : img - m * c_out; }
};

struct EulerARule : KRule {  // k_samplers.py:384-397
  __device__ EulerARule(const float* r, const StepParams& p) : KRule(r, p) { draws = flag; }
  __device__ void apply(float& x, float&, float& next, float m, float xi) const {
    const float d = (x - denoised(x, m)) / sigma;
    x = x + d * dt;
    if (flag) x = x + xi * sigma_up;
    next = x;
  }
};

struct HeunRule : KRule {  // k_samplers.py:429-440; stage 1 writes no state (so there is nothing to clamp), stage 2 no aux
  __device__ HeunRule(const float* r, const StepParams& p) : KRule(r, p) {
    reads_aux = writes_x = flag;
    writes_aux = !flag;
  }
  __device__ void apply(float& x, float& aux, float& next, float m, float) const {
    const float img = flag ? x + aux * dt : x;  // stage 2 evaluates stage 1's `next`, rebuilt from the saved d: the same bits
    const float d = (img - denoised(img, m)) / sigma;
    if (!flag) {
      aux = d;
      next = x + d * dt;
    } else {
      const float dp = (aux + d) / 2.0f;
      x = next = x + dp * dt;
    }
  }
};

struct Dpmpp2mRule : KRule {  // k_samplers.py:464-477
  __device__ Dpmpp2mRule(const float* r, const StepParams& p) : KRule(r, p) {
    reads_aux = flag;
    writes_aux = true;
  }
  __device__ void apply(float& x, float& aux, float& next, float m, float) const {
    const float den = denoised(x, m);
    const float dd = flag ? r1 * den - r2 * aux : den;
    x = next = ratio * x - em1 * dd;
    aux = den;
  }
};

// one step (DDIM, basic) or model evaluation (K) on x[total] (total = B * n, total % 4 == 0); the row of the table is the
// counter's, and a counter outside the table makes the launch a no-op
template <class Rule>
__global__ void sample_step_kernel(const StepParams p) {
  const int k = *p.kp;
  if (k < 0 || k >= p.rows) return;
  const Rule rule(p.table + (long)k * Rule::ROW, p);
  const bool clamp = p.clip_last && k == p.rows - 1 && rule.writes_x;
  const long total = p.total4 << 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < p.total4; i4 += stride) {
    const long base = i4 << 2;
    f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + base);
    const u32x2 wc = *reinterpret_cast<const u32x2*>(p.out_c + base);
    f32x4 m = {bf16lo(wc[0]), bf16hi(wc[0]), bf16lo(wc[1]), bf16hi(wc[1])};
    if (p.out_u != nullptr) {  // eps_uncond + s * (eps - eps_uncond)   (schema.py:255-263)
      const u32x2 wu = *reinterpret_cast<const u32x2*>(p.out_u + base);
      const f32x4 u = {bf16lo(wu[0]), bf16hi(wu[0]), bf16lo(wu[1]), bf16hi(wu[1])};
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = u[e] + p.scale * (m[e] - u[e]);
    }
    f32x4 xi = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f}, nxt;
    if (rule.draws)
      xi = p.bank != nullptr ? *reinterpret_cast<const f32x4*>(p.bank + (long)k * total + base)
                             : normal4(p.offset + (unsigned long long)k * (unsigned long long)p.total4 + (unsigned long long)i4, p.seed);
    if (rule.reads_aux) av = *reinterpret_cast<const f32x4*>(p.aux + base);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = xv[e], a = av[e], next;
      rule.apply(x, a, next, m[e], xi[e]);
      if (clamp) x = next = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);  // torch.clip: NaN stays NaN
      if constexpr (Rule::SCALES_INPUT) next = next * rule.c_in;
      xv[e] = x;
      av[e] = a;
      nxt[e] = next;
    }
    if (rule.writes_x) *reinterpret_cast<f32x4*>(p.x + base) = xv;
    if (rule.writes_aux) *reinterpret_cast<f32x4*>(p.aux + base) = av;
    const u32x2 w = {pack_bf16x2(nxt[0], nxt[1]), pack_bf16x2(nxt[2], nxt[3])};
    *reinterpret_cast<u32x2*>(p.xin + base) = w;
    if (p.dup == 2) *reinterpret_cast<u32x2*>(p.xin + total + base) = w;
  }
}

// k += 1; the UNet's timesteps[0 .. gb) = t of the new row (while there is one): int64 of it, or f32 as it stands (the K
// samplers' fractional timesteps).  One thread, a launch of its own: every workgroup of the step kernel has read k before
// this launch starts.
__global__ void sample_advance_kernel(int* __restrict__ kp, const float* __restrict__ table, int rows, int row,
                                      void* __restrict__ ts, int ts_is_int64, int gb) {
  const int kn = *kp + 1;
  *kp = kn;
  if (kn >= 0 && kn < rows) {
    const float t = table[(long)kn * row];
    for (int j = 0; j < gb; ++j) {
      if (ts_is_int64) {
        static_cast<int64_t*>(ts)[j] = (int64_t)t;
      } else {
        static_cast<float*>(ts)[j] = t;
      }
    }
  }
}

// what both step entry points require of their operands (`who` names the entry point in the messages), then the launch
int run_step(const char* who, void (*kernel)(StepParams), StepParams p, int64_t B, int64_t n, void* stream) {
  CFHIP_REQUIRE(p.x && p.xin && p.out_c && p.table && p.kp && B > 0 && n > 0 && p.rows > 0, "%s: bad arguments", who);
  CFHIP_REQUIRE(n % 4 == 0, "%s: n = %lld is not a multiple of 4", who, (long long)n);
  CFHIP_REQUIRE(p.param == CFHIP_PARAM_EPS || p.param == CFHIP_PARAM_X0 || p.param == CFHIP_PARAM_V, "%s: parameterization %d", who, p.param);
  CFHIP_REQUIRE(p.dup == 1 || p.dup == 2, "%s: dup %d (1 or 2)", who, p.dup);
  CFHIP_REQUIRE(((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.aux & 15) == 0 && ((uintptr_t)p.xin & 7) == 0 &&
                    ((uintptr_t)p.out_c & 7) == 0 && ((uintptr_t)p.out_u & 7) == 0 && ((uintptr_t)p.bank & 15) == 0,
                "%s: misaligned operand", who);
  p.total4 = (long)(B * n / 4);
  hipLaunchKernelGGL(kernel, dim3(grid_for(p.total4, 256)), dim3(256), 0, (hipStream_t)stream, p);
  CFHIP_CHECK_LAUNCH(who);
  return CFHIP_OK;
}

}  // namespace

extern "C" int cfhip_randn_f32(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(out && n > 0, "randn_f32: bad arguments");
  hipLaunchKernelGGL(randn_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, out, (long)n,
                     (unsigned long long)seed, (unsigned long long)offset);
  CFHIP_CHECK_LAUNCH("randn_f32");
  return CFHIP_OK;
}

extern "C" int cfhip_gaussian_posterior(const void* moments, int channels_last, float* z, float* kl, const float* noise,
                                        int deterministic, int64_t B, int E, int64_t hw, float scale_factor, uint64_t seed,
                                        uint64_t offset, void* stream) {
  CFHIP_REQUIRE(moments && (z || kl), "gaussian_posterior: null moments, or neither z nor kl asked for");
  CFHIP_REQUIRE(B > 0 && E > 0 && hw > 0, "gaussian_posterior: empty tensor");
  CFHIP_REQUIRE(B <= 65535, "gaussian_posterior: B = %lld exceeds the grid limit", (long long)B);
  CFHIP_REQUIRE(!(deterministic && noise), "gaussian_posterior: deterministic takes no noise");
  CFHIP_REQUIRE(((uintptr_t)moments & 1) == 0 && ((uintptr_t)z & 3) == 0 && ((uintptr_t)kl & 3) == 0 && ((uintptr_t)noise & 3) == 0,
                "gaussian_posterior: misaligned operand");
  const long groups = ((long)E * hw + 3) / 4 + 1;
  const dim3 grid(kl ? 1 : grid_for(groups, 256), (unsigned)B);
  hipLaunchKernelGGL(gaussian_posterior_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)moments, channels_last != 0,
                     z, kl, noise, deterministic != 0, E, (long)hw, scale_factor, (unsigned long long)seed,
                     (unsigned long long)offset);
  CFHIP_CHECK_LAUNCH("gaussian_posterior");
  return CFHIP_OK;
}

extern "C" int cfhip_diffusion_sample_step(float* x, void* xin, const void* out_c, const void* out_u, float scale,
                                           const float* table, int steps, const int* k, const float* noise, int64_t B,
                                           int64_t n, int kind, int param, float temperature, int clip_last, int dup,
                                           uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(kind == CFHIP_SAMPLER_DDIM || kind == CFHIP_SAMPLER_BASIC, "diffusion_sample_step: kind %d", kind);
  CFHIP_REQUIRE(!(kind == CFHIP_SAMPLER_DDIM && param == CFHIP_PARAM_X0) && !(kind == CFHIP_SAMPLER_BASIC && param == CFHIP_PARAM_V),
                "diffusion_sample_step: parameterization %d is not defined for sampler %d", param, kind);
  const StepParams p = {x, nullptr, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                        scale, temperature, steps, param, clip_last, dup, seed, offset};
  return run_step("diffusion_sample_step", kind == CFHIP_SAMPLER_DDIM ? sample_step_kernel<DdimRule> : sample_step_kernel<BasicRule>,
                  p, B, n, stream);
}

extern "C" int cfhip_k_sample_step(float* x, float* aux, void* xin, const void* out_c, const void* out_u, float scale,
                                   const float* table, int rows, const int* k, const float* noise, int64_t B, int64_t n,
                                   int kind, int param, int clip_last, int dup, uint64_t seed, uint64_t offset, void* stream) {
  CFHIP_REQUIRE(kind == CFHIP_KSAMPLER_EULER_A || kind == CFHIP_KSAMPLER_HEUN || kind == CFHIP_KSAMPLER_DPMPP_2M,
                "k_sample_step: kind %d", kind);
  CFHIP_REQUIRE(param != CFHIP_PARAM_X0, "k_sample_step: parameterization %d (only eps and v are defined for the k samplers)", param);
  CFHIP_REQUIRE(aux || kind == CFHIP_KSAMPLER_EULER_A, "k_sample_step: sampler %d needs the auxiliary buffer", kind);
  CFHIP_REQUIRE(!noise || kind == CFHIP_KSAMPLER_EULER_A, "k_sample_step: sampler %d draws no noise", kind);
  const StepParams p = {x, aux, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                        scale, 1.0f, rows, param, clip_last, dup, seed, offset};
  return run_step("k_sample_step",
                  kind == CFHIP_KSAMPLER_EULER_A ? sample_step_kernel<EulerARule>
                  : kind == CFHIP_KSAMPLER_HEUN  ? sample_step_kernel<HeunRule>
                                                 : sample_step_kernel<Dpmpp2mRule>,
                  p, B, n, stream);
}

extern "C" int cfhip_diffusion_sample_advance(int* k, const float* table, int steps, int64_t* timesteps, int gb,
                                              void* stream) {
  CFHIP_REQUIRE(k && table && timesteps && steps > 0 && gb > 0, "diffusion_sample_advance: bad arguments");
  hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, k, table, steps, CFHIP_SAMPLE_ROW,
                     (void*)timesteps, 1, gb);
  CFHIP_CHECK_LAUNCH("diffusion_sample_advance");
  return CFHIP_OK;
}

extern "C" int cfhip_k_sample_advance(int* k, const float* table, int rows, void* timesteps, int timesteps_int64, int gb,
                                      void* stream) {
  CFHIP_REQUIRE(k && table && timesteps && rows > 0 && gb > 0, "k_sample_advance: bad arguments");
  CFHIP_REQUIRE(((uintptr_t)timesteps & (timesteps_int64 ? 7 : 3)) == 0, "k_sample_advance: misaligned timesteps");
  hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, k, table, rows, CFHIP_KSAMPLE_ROW, timesteps,
                     timesteps_int64 != 0, gb);
  CFHIP_CHECK_LAUNCH("k_sample_advance");
  return CFHIP_OK;
}
