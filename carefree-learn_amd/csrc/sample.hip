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
//
// With a reference (image-to-image and inpainting: ISampler.sample's ref / ref_mask / ref_noise / start_step, schema.py:153-194)
// the same kernel, instantiated with REF, merges inside the step launch: DDIM / basic merge the state row k leaves with the
// noised reference (merge_ref of basic.py:16-35, which the reference runs at the top of step k + 1), the K rules merge the
// reference into their denoised value (k_samplers.py:185-190).  The counter stays absolute: a run from start_step s starts k at
// row s and draws what a full run draws there.  The entry points without a reference instantiate the kernel without it.
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

// The optional reference of a launch (image-to-image / inpainting; merge_ref of samplers/basic.py:16-35, get_denoised_with_reference
// of k_samplers.py:185-190).  ref f32 [B][n]; mask f32 [B or 1][C or 1][hw], never expanded: element (b, c, pix) is
// mask[b * mask_bs + c * mask_cs + pix] with a stride of 0 where the mask has extent 1.  DDIM / basic only: side f32 [rows][2] =
// (w_net, w_noise) of the merge IN FRONT OF each row, and its noise by `noise_mode`: Philox at counter (seed, offset + (rows + row)
// * total4 + i4) (disjoint from the starting noise at offset - total4 and from the step draws at offset + row * total4, row < rows),
// one f32 [B][n] tensor for every merge (unified), or a bank whose entry 0 is the merge in front of row `row0`.  No merge happens
// in front of a row below row0, the first row the run executes.
struct RefParams {
  const float *ref, *mask, *side, *noise;
  long mask_bs, mask_cs, n, hw;
  int noise_mode, row0;
};

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
  RefParams r;
};

// one element's reference operands inside a rule (`on` is a compile-time false in the kernels without a reference)
struct RefElem {
  bool on;
  float ref, mask;
};

// the mask values of the four flat indices from `base` on: a vector straddles two channels or two samples when hw % 4 != 0
__device__ __forceinline__ f32x4 mask4(const RefParams& r, long base) {
  long b = base / r.n;
  const long j = base - b * r.n;
  long c = j / r.hw, pix = j - c * r.hw;
  f32x4 mv;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mv[e] = r.mask[b * r.mask_bs + c * r.mask_cs + pix];
    if (++pix == r.hw) {
      pix = 0;
      if (++c * r.hw == r.n) {
        c = 0;
        ++b;
      }
    }
  }
  return mv;
}

// merge_ref (basic.py:33-34 over DDPMQSampler.q_sample, schema.py:107), in the reference's operand order
__device__ __forceinline__ float merge_ref(float x, float ref, float mask, float w_net, float w_noise, float nz) {
  const float noisy = w_net * ref + w_noise * nz;
  return mask * noisy + (1.0f - mask) * x;
}

// the noise of the merge in front of `row` for the vector i4
__device__ __forceinline__ f32x4 merge_noise4(const StepParams& p, int row, long i4) {
  const RefParams& r = p.r;
  const long base = i4 << 2;
  if (r.noise_mode == CFHIP_MERGE_NOISE_UNIFIED) return *reinterpret_cast<const f32x4*>(r.noise + base);
  if (r.noise_mode == CFHIP_MERGE_NOISE_BANK) return *reinterpret_cast<const f32x4*>(r.noise + (long)(row - r.row0) * (p.total4 << 2) + base);
  return normal4(p.offset + ((unsigned long long)p.rows + (unsigned long long)row) * (unsigned long long)p.total4 + (unsigned long long)i4, p.seed);
}

// A rule is one sampler's update.  It is built from row k of the table (ROW scalars; column 0, the timestep, is the advance
// kernel's), says what this row does, and maps one element: apply(x, aux, next, m, xi, g) takes the state, the auxiliary value,
// the guided model output, the draw and the element's reference operands (the K rules merge them into `denoised`), and leaves the new state, the new auxiliary value and `next`, the image of the next
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
  __device__ void apply(float& x, float&, float& next, float m, float xi, const RefElem&) const {
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
  __device__ void apply(float& x, float&, float& next, float m, float xi, const RefElem&) const {
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
  __device__ float denoised(float img, float m, const RefElem& g) const {
    const float den = v ? img * c_skip - m * c_out : img - m * c_out;
    return g.on ? g.mask * g.ref + (1.0f - g.mask) * den : den;  // get_denoised_with_reference (k_samplers.py:185-190)
  }
};

struct EulerARule : KRule {  // k_samplers.py:384-397
  __device__ EulerARule(const float* r, const StepParams& p) : KRule(r, p) { draws = flag; }
  __device__ void apply(float& x, float&, float& next, float m, float xi, const RefElem& g) const {
    const float d = (x - denoised(x, m, g)) / sigma;
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
  __device__ void apply(float& x, float& aux, float& next, float m, float, const RefElem& g) const {
    const float img = flag ? x + aux * dt : x;  // stage 2 evaluates stage 1's `next`, rebuilt from the saved d: the same bits
    const float d = (img - denoised(img, m, g)) / sigma;
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
  __device__ void apply(float& x, float& aux, float& next, float m, float, const RefElem& g) const {
    const float den = denoised(x, m, g);
    const float dd = flag ? r1 * den - r2 * aux : den;
    x = next = ratio * x - em1 * dd;
    aux = den;
  }
};

// one step (DDIM, basic) or model evaluation (K) on x[total] (total = B * n, total % 4 == 0); the row of the table is the
// counter's, and a counter outside the table makes the launch a no-op.  REF: the launch has a reference.  The K rules merge it
// into their denoised value; DDIM / basic merge the state row k leaves with the noised reference, which is the merge the
// reference performs at the top of step k + 1 (so not after the last row, whose image is returned unmerged and clamped).
template <class Rule, bool REF>
__global__ void sample_step_kernel(const StepParams p) {
  const int k = *p.kp;
  if (k < 0 || k >= p.rows) return;
  const Rule rule(p.table + (long)k * Rule::ROW, p);
  const bool clamp = p.clip_last && k == p.rows - 1 && rule.writes_x;
  const bool merge_after = REF && !Rule::SCALES_INPUT && k + 1 < p.rows && k + 1 >= p.r.row0;
  float w_net = 0.f, w_noise = 0.f;
  if (merge_after) {
    w_net = p.r.side[2 * (k + 1)];
    w_noise = p.r.side[2 * (k + 1) + 1];
  }
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
    f32x4 rv = {0.f, 0.f, 0.f, 0.f}, mv = {0.f, 0.f, 0.f, 0.f}, nz = {0.f, 0.f, 0.f, 0.f};
    if constexpr (REF) {
      if (Rule::SCALES_INPUT || merge_after) {
        rv = *reinterpret_cast<const f32x4*>(p.r.ref + base);
        mv = mask4(p.r, base);
      }
      if (merge_after) nz = merge_noise4(p, k + 1, i4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = xv[e], a = av[e], next;
      rule.apply(x, a, next, m[e], xi[e], RefElem{REF && Rule::SCALES_INPUT, rv[e], mv[e]});
      if (merge_after) x = next = merge_ref(x, rv[e], mv[e], w_net, w_noise, nz[e]);
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

// the merge in front of row k on its own (x and xin = the merged state): the first executed DDIM / basic step of a run has no
// preceding step launch to ride in.  A counter outside the table, or below row0, makes the launch a no-op.
__global__ void sample_merge_kernel(const StepParams p) {
  const int k = *p.kp;
  if (k < 0 || k >= p.rows || k < p.r.row0) return;
  const float w_net = p.r.side[2 * k], w_noise = p.r.side[2 * k + 1];
  const long total = p.total4 << 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < p.total4; i4 += stride) {
    const long base = i4 << 2;
    f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + base);
    const f32x4 rv = *reinterpret_cast<const f32x4*>(p.r.ref + base);
    const f32x4 mv = mask4(p.r, base);
    const f32x4 nz = merge_noise4(p, k, i4);
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = merge_ref(xv[e], rv[e], mv[e], w_net, w_noise, nz[e]);
    *reinterpret_cast<f32x4*>(p.x + base) = xv;
    const u32x2 w = {pack_bf16x2(xv[0], xv[1]), pack_bf16x2(xv[2], xv[3])};
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

// what every step entry point requires of its operands (`who` names the entry point in the messages), then the launch
int run_step(const char* who, void (*kernel)(StepParams), StepParams p, int64_t B, int64_t n, void* stream, bool merge_only = false) {
  CFHIP_REQUIRE(p.x && p.xin && (merge_only || (p.out_c && p.table)) && p.kp && B > 0 && n > 0 && p.rows > 0, "%s: bad arguments", who);
  CFHIP_REQUIRE(n % 4 == 0, "%s: n = %lld is not a multiple of 4", who, (long long)n);
  CFHIP_REQUIRE(p.param == CFHIP_PARAM_EPS || p.param == CFHIP_PARAM_X0 || p.param == CFHIP_PARAM_V, "%s: parameterization %d", who, p.param);
  CFHIP_REQUIRE(p.dup == 1 || p.dup == 2, "%s: dup %d (1 or 2)", who, p.dup);
  CFHIP_REQUIRE(((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.aux & 15) == 0 && ((uintptr_t)p.xin & 7) == 0 &&
                    ((uintptr_t)p.out_c & 7) == 0 && ((uintptr_t)p.out_u & 7) == 0 && ((uintptr_t)p.bank & 15) == 0 &&
                    ((uintptr_t)p.r.ref & 15) == 0 && ((uintptr_t)p.r.mask & 3) == 0 && ((uintptr_t)p.r.side & 3) == 0 &&
                    ((uintptr_t)p.r.noise & 15) == 0,
                "%s: misaligned operand", who);
  p.total4 = (long)(B * n / 4);
  hipLaunchKernelGGL(kernel, dim3(grid_for(p.total4, 256)), dim3(256), 0, (hipStream_t)stream, p);
  CFHIP_CHECK_LAUNCH(who);
  return CFHIP_OK;
}

// the reference operands of a `_ref` entry point, checked; `noised`: DDIM / basic (a side table and a merge noise), else K
int ref_params(const char* who, RefParams& r, const float* ref, const float* mask, int64_t mask_bstride, int64_t mask_cstride, int64_t n,
               int64_t hw, const float* side, const float* merge_noise, int merge_noise_mode, int merge_row0, int rows, bool noised) {
  CFHIP_REQUIRE(ref && mask, "%s: needs `ref` and `mask`", who);
  CFHIP_REQUIRE(hw > 0 && n > 0 && n % hw == 0, "%s: hw = %lld does not divide n = %lld", who, (long long)hw, (long long)n);
  CFHIP_REQUIRE((mask_bstride == 0 || mask_bstride == hw || mask_bstride == n) && (mask_cstride == 0 || mask_cstride == hw) &&
                    !(mask_bstride == hw && mask_cstride == hw && n != hw) && !(mask_bstride == n && mask_cstride == 0 && n != hw),
                "%s: mask strides (%lld, %lld) are not those of a contiguous [B or 1][C or 1][hw] mask", who, (long long)mask_bstride,
                (long long)mask_cstride);
  if (noised) {
    CFHIP_REQUIRE(side, "%s: needs the side table", who);
    CFHIP_REQUIRE(merge_noise_mode == CFHIP_MERGE_NOISE_PHILOX || merge_noise_mode == CFHIP_MERGE_NOISE_UNIFIED ||
                      merge_noise_mode == CFHIP_MERGE_NOISE_BANK,
                  "%s: merge noise mode %d", who, merge_noise_mode);
    CFHIP_REQUIRE((merge_noise_mode == CFHIP_MERGE_NOISE_PHILOX) == (merge_noise == nullptr),
                  "%s: the merge noise tensor goes with the unified and bank modes only", who);
    CFHIP_REQUIRE(merge_row0 >= 0 && merge_row0 < rows, "%s: merge_row0 %d outside [0, %d)", who, merge_row0, rows);
  }
  r = {ref, mask, side, merge_noise, (long)mask_bstride, (long)mask_cstride, (long)n, (long)hw, merge_noise_mode, merge_row0};
  return CFHIP_OK;
}

int check_step_kind(const char* who, int kind, int param) {
  CFHIP_REQUIRE(kind == CFHIP_SAMPLER_DDIM || kind == CFHIP_SAMPLER_BASIC, "%s: kind %d", who, kind);
  CFHIP_REQUIRE(!(kind == CFHIP_SAMPLER_DDIM && param == CFHIP_PARAM_X0) && !(kind == CFHIP_SAMPLER_BASIC && param == CFHIP_PARAM_V),
                "%s: parameterization %d is not defined for sampler %d", who, param, kind);
  return CFHIP_OK;
}

int check_k_kind(const char* who, int kind, int param, const float* aux, const float* noise) {
  CFHIP_REQUIRE(kind == CFHIP_KSAMPLER_EULER_A || kind == CFHIP_KSAMPLER_HEUN || kind == CFHIP_KSAMPLER_DPMPP_2M, "%s: kind %d", who, kind);
  CFHIP_REQUIRE(param != CFHIP_PARAM_X0, "%s: parameterization %d (only eps and v are defined for the k samplers)", who, param);
  CFHIP_REQUIRE(aux || kind == CFHIP_KSAMPLER_EULER_A, "%s: sampler %d needs the auxiliary buffer", who, kind);
  CFHIP_REQUIRE(!noise || kind == CFHIP_KSAMPLER_EULER_A, "%s: sampler %d draws no noise", who, kind);
  return CFHIP_OK;
}

template <bool REF>
auto step_kernel(int kind) {
  return kind == CFHIP_SAMPLER_DDIM ? sample_step_kernel<DdimRule, REF> : sample_step_kernel<BasicRule, REF>;
}

template <bool REF>
auto k_step_kernel(int kind) {
  return kind == CFHIP_KSAMPLER_EULER_A ? sample_step_kernel<EulerARule, REF>
         : kind == CFHIP_KSAMPLER_HEUN  ? sample_step_kernel<HeunRule, REF>
                                        : sample_step_kernel<Dpmpp2mRule, REF>;
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
  if (int rc = check_step_kind("diffusion_sample_step", kind, param)) return rc;
  const StepParams p = {x, nullptr, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                        scale, temperature, steps, param, clip_last, dup, seed, offset};
  return run_step("diffusion_sample_step", step_kernel<false>(kind), p, B, n, stream);
}

extern "C" int cfhip_diffusion_sample_step_ref(float* x, void* xin, const void* out_c, const void* out_u, float scale,
                                               const float* table, int steps, const int* k, const float* noise, int64_t B,
                                               int64_t n, int kind, int param, float temperature, int clip_last, int dup,
                                               uint64_t seed, uint64_t offset, const float* ref, const float* mask,
                                               int64_t mask_bstride, int64_t mask_cstride, int64_t hw, const float* side,
                                               const float* merge_noise, int merge_noise_mode, int merge_row0, void* stream) {
  if (int rc = check_step_kind("diffusion_sample_step_ref", kind, param)) return rc;
  StepParams p = {x, nullptr, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                  scale, temperature, steps, param, clip_last, dup, seed, offset};
  if (int rc = ref_params("diffusion_sample_step_ref", p.r, ref, mask, mask_bstride, mask_cstride, n, hw, side, merge_noise,
                          merge_noise_mode, merge_row0, steps, true))
    return rc;
  return run_step("diffusion_sample_step_ref", step_kernel<true>(kind), p, B, n, stream);
}

extern "C" int cfhip_diffusion_sample_merge(float* x, void* xin, int steps, const int* k, int64_t B, int64_t n, int dup, uint64_t seed,
                                            uint64_t offset, const float* ref, const float* mask, int64_t mask_bstride,
                                            int64_t mask_cstride, int64_t hw, const float* side, const float* merge_noise,
                                            int merge_noise_mode, int merge_row0, void* stream) {
  StepParams p = {x, nullptr, (bf16_t*)xin, nullptr, nullptr, nullptr, nullptr, k, 1.0f, 1.0f, steps, CFHIP_PARAM_EPS, 0, dup, seed, offset};
  CFHIP_REQUIRE(steps > 0, "diffusion_sample_merge: bad arguments");
  if (int rc = ref_params("diffusion_sample_merge", p.r, ref, mask, mask_bstride, mask_cstride, n, hw, side, merge_noise,
                          merge_noise_mode, merge_row0, steps, true))
    return rc;
  return run_step("diffusion_sample_merge", sample_merge_kernel, p, B, n, stream, true);
}

extern "C" int cfhip_k_sample_step(float* x, float* aux, void* xin, const void* out_c, const void* out_u, float scale,
                                   const float* table, int rows, const int* k, const float* noise, int64_t B, int64_t n,
                                   int kind, int param, int clip_last, int dup, uint64_t seed, uint64_t offset, void* stream) {
  if (int rc = check_k_kind("k_sample_step", kind, param, aux, noise)) return rc;
  const StepParams p = {x, aux, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                        scale, 1.0f, rows, param, clip_last, dup, seed, offset};
  return run_step("k_sample_step", k_step_kernel<false>(kind), p, B, n, stream);
}

extern "C" int cfhip_k_sample_step_ref(float* x, float* aux, void* xin, const void* out_c, const void* out_u, float scale,
                                       const float* table, int rows, const int* k, const float* noise, int64_t B, int64_t n,
                                       int kind, int param, int clip_last, int dup, uint64_t seed, uint64_t offset,
                                       const float* ref, const float* mask, int64_t mask_bstride, int64_t mask_cstride, int64_t hw,
                                       void* stream) {
  if (int rc = check_k_kind("k_sample_step_ref", kind, param, aux, noise)) return rc;
  StepParams p = {x, aux, (bf16_t*)xin, (const bf16_t*)out_c, (const bf16_t*)out_u, table, noise, k,
                  scale, 1.0f, rows, param, clip_last, dup, seed, offset};
  if (int rc = ref_params("k_sample_step_ref", p.r, ref, mask, mask_bstride, mask_cstride, n, hw, nullptr, nullptr,
                          CFHIP_MERGE_NOISE_PHILOX, 0, rows, false))
    return rc;
  return run_step("k_sample_step_ref", k_step_kernel<true>(kind), p, B, n, stream);
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
