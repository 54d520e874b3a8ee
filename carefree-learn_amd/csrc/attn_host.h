// Internal to the attention sources (never installed): what crosses the boundary between csrc/attn.hip — options, plan, C ABI —
// and the kernel-family files csrc/attn_resident.hip and attn_one_pass.hip.  The kernels keep
// internal linkage in their own file; each family file exports ONE launcher, declared at the end of this header.  The types in
// the launchers' signatures live in a named namespace: an anonymous-namespace type there would be a different type per file.
#pragma once
#include "common.h"
#include <type_traits>

namespace cfhip_attn {

struct AttnParams {
  const bf16_t* q; const bf16_t* k; const bf16_t* v;
  bf16_t* o; const bf16_t* o_in; const bf16_t* d_o;
  float* lse; float* delta;
  const uint8_t* mask;
  bf16_t* dq; bf16_t* dk; bf16_t* dv;
  int B, H, Tq, Tk;
  long q_sb, q_st, kv_sb, kv_st, o_sb, o_st;
  long ms_b, ms_h, ms_q;
  float scale;
  int causal;
  int dh;           // head_dim of the general kernels (the resident fast kernels are head_dim 64 only)
  int delta_ready;  // dK/dV pass: p.delta was already written by the dQ pass of the same call
  // dropout on the attention probabilities (general kernels, DROP instantiations): keep(b, h, i, j) = byte (j & 3) of word
  // (i & 3) of philox(drop_offset + ((b H + h) drop_bq + (i >> 2)) drop_bk + (j >> 2), drop_seed) >= drop_thresh, i.e. one
  // Philox call per 4 x 4 block of the score matrix, the same bits whichever way a kernel walks it; kept values are
  // scaled by drop_scale = 1 / (1 - drop_thresh / 256)
  unsigned long long drop_seed, drop_offset;
  int drop_bq, drop_bk;
  unsigned drop_thresh;
  float drop_scale;
#ifdef CFHIP_ABLATE
  int ablate;       // benchmarking only (forward): bit0 skip the K/V DMA, bit1 skip the tile loop, bit2 skip stores; attn_bwd_one2_kernel: 8 no phase 1, 16 no phase 2, 32 no statistics, 64 no dK / dV stores, 128 no K / V fragments, 256 no staging of the next head
#endif
};

// Timing ablations exist only in -DCFHIP_ABLATE builds (tools/build_variant.sh); the product library has none.
#ifdef CFHIP_ABLATE
#define ATTN_ABL(bit) (p.ablate & (bit))
#else
#define ATTN_ABL(bit) false
#endif

constexpr int PERS_WAVES = 16;  // waves of a persistent workgroup (csrc/attn_resident.hip): a wave per 16-row tile, T <= 256

constexpr int one_pass_waves(int NB) { return NB <= 2 ? 4 : NB <= 4 ? 8 : 16; }    // PW of attn_bwd_one_kernel<NB, PW, ..>
constexpr int one_pass_per_cu(int NB) { return NB <= 2 ? 4 : NB <= 4 ? 2 : 1; }  // workgroups per CU at that size

enum Family : int {  // one per __global__ template; a step's n / plain / flag are its template arguments
  FWD,       // attn_fwd_kernel<n = NB, plain>
  FWD_PERS,  // attn_fwd_pers_kernel<n = NB>
  FWD2,      // attn_fwd2_kernel<plain, n = NDT, flag = SUMCOL>
  GEN_FWD,   // attn_gen_fwd_kernel<n = NH, plain, flag = DROP>
  DELTA,     // attn_delta_kernel
  DQ,        // attn_bwd_dq_kernel<plain>(p, n = nb)
  DQ_PERS,   // attn_bwd_dq_pers_kernel<n = NB>
  DQ2,       // attn_bwd_dq2_kernel<plain, n = NDT>
  DQ3,       // attn_bwd_dq3_kernel<n = 3, flag = FOLD>
  GEN_DQ,    // attn_gen_bwd_dq_kernel<n = NH, plain, flag = DROP>
  DKV,       // attn_bwd_dkv_kernel<plain>(p, n = nbq)
  DKV_PERS,  // attn_bwd_dkv_pers_kernel<n = NBQ>
  DKV2,      // attn_bwd_dkv2_kernel<plain, n = NDT, flag = FOLD>
  GEN_DKV,   // attn_gen_bwd_dkv_kernel<n = NH, plain, flag = DROP>
  ONE,       // attn_bwd_one_kernel<n = NB, PW of NB, flag = CAUSAL>
  ONE2,      // attn_bwd_one2_kernel<n = NB>
};

struct Step {
  Family family;
  int n;
  bool plain, flag;
};

// ---- launch --------------------------------------------------------------------------------

// the one launcher: dynamic LDS above 64 KiB is reserved on the kernel that is launched
template <auto Kernel, typename... Args>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const char* who, Args... args) {
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      cfhip_set_error("%s: cannot reserve %zu bytes of LDS: %s", who, lds, hipGetErrorString(e));
      return CFHIP_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  CFHIP_CHECK_LAUNCH(who);
  return CFHIP_OK;
}

template <int N>
using Int = std::integral_constant<int, N>;

// f(Int<n>, plain, flag) with the step's arguments as compile-time constants; an n outside Ns... is a bad nb
template <int... Ns, typename F>
int with_args(const Step& st, const char* who, F f) {
  int rc = CFHIP_ERR_INVALID;
  auto call = [&](auto n) {
    rc = st.plain ? (st.flag ? f(n, std::true_type{}, std::true_type{}) : f(n, std::true_type{}, std::false_type{}))
                  : (st.flag ? f(n, std::false_type{}, std::true_type{}) : f(n, std::false_type{}, std::false_type{}));
    return true;
  };
  if (!((st.n == Ns && call(Int<Ns>{})) || ...)) cfhip_set_error("%s: bad nb %d", who, st.n);
  return rc;
}

inline int no_kernel(const Step& st) {  // a step the plan never makes: not every argument combination is instantiated
  cfhip_set_error("attention: no kernel for step %d<%d,%d,%d>", (int)st.family, st.n, (int)st.plain, (int)st.flag);
  return CFHIP_ERR_INVALID;
}

// One launcher per family file (the chunked families are launched from csrc/attn.hip itself): the cases of the step's family with their grids, blocks and LDS byte counts.  `pers_ctas` is the
// "attn_pers_ctas" option (the options themselves stay private to csrc/attn.hip).
int launch_resident(const Step& st, const AttnParams& p, int pers_ctas, hipStream_t s);  // FWD, DQ, DKV and their _PERS forms
int launch_one_pass(const Step& st, const AttnParams& p, int pers_ctas, hipStream_t s);  // ONE, ONE2

}  // namespace cfhip_attn
