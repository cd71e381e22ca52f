// post_kernels.hip -- posterior marginals and posterior draws of the enumerated latent states (gfx950).
//
// After a step-2/3 fit the decode (pert_enum_pass, PERT_MODE_DECODE) gives the joint MAP state of
// every (bin, cell).  This pass gives the probabilities that call is made from: at the fitted
// parameters the posterior over the 2P joint states of an element is gamma = softmax_{c,r} s(c, r)
// (pert_math.h), and the kernel writes its marginals P(rep = 1) and P(cn = k).
//
// One wave per (64-cell tile, bin tile), lanes are cells (as enum3_kernel): per-cell u, tau and
// betas live in registers, per-bin rho and GC features are wave-uniform loads, the P logits of a
// bin are P coalesced 256-byte rows of the z_pi wave tile.  Plain global loads: this runs once
// after a fit, not in the SVI loop.  Nothing is reduced across lanes and nothing is added to
// atomically, so reruns are bit-identical.  Nothing of pert_state is written.
#include "../../include/pert_hip.h"
#include "pert_math.h"
#include "sim_math.h"

#include <math.h>
#include <stddef.h>

namespace {

using namespace pert;

constexpr int kPostDefaultLT = 32;   // bins per tile when the state names none (as the passes)
constexpr int kPostMaxLT = 64;

// its own case list: every supported P
#define PERT_POST_P_CASES                                                                       \
  PERT_CASE(2) PERT_CASE(3) PERT_CASE(4) PERT_CASE(5) PERT_CASE(6) PERT_CASE(7) PERT_CASE(8)    \
  PERT_CASE(9) PERT_CASE(10) PERT_CASE(11) PERT_CASE(12) PERT_CASE(13) PERT_CASE(14)            \
  PERT_CASE(15) PERT_CASE(16)

template <int P>
__global__ void __launch_bounds__(64, 4) enum_posterior_kernel(pert_problem pr, pert_state st, int LT,
                                                               const uint8_t* __restrict__ cn_state,
                                                               float* __restrict__ rep_prob,
                                                               float* __restrict__ cn_prob,
                                                               float* __restrict__ cn_marg) {
  const int lane = threadIdx.x;
  const int wt = blockIdx.x, bt = blockIdx.y;
  const int N = pr.N, K1 = pr.K1, ldn = pr.ldn, L = pr.L;
  const int n = wt * 64 + lane;                 // < ldn: ldn is N rounded up to a multiple of 256
  const bool valid = n < N;
  const int l0 = bt * LT;
  const int l1 = min(L, l0 + LT);
  const bool frozen = pr.kind == PERT_KIND_STEP3;
  const pert_layout lay = st.lay;
  const float* __restrict__ params = st.params;

  // cell parameters (padded lanes: u = 0, so D = 0 and every chain is clamped; never stored)
  const float a_val = frozen ? pr.a_fixed : fexp(params[lay.off_a]);
  const float c0 = (1.0f - pr.lamb) / pr.lamb;
  const float log1m_lam = pr.log1m_lam;
  float u = 0.0f, tau = 0.5f;
  float beta[PERT_MAX_K1];
#pragma unroll
  for (int k = 0; k < PERT_MAX_K1; ++k) beta[k] = 0.0f;
  if (valid) {
    u = params[lay.off_u + n];
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k)
      if (k < K1) beta[k] = params[lay.off_beta + k * N + n];
    float dm;
    tau = clipped_sigmoid(params[lay.off_tau + n], &dm);
  }
  const float ucc = u * c0;
  const float* __restrict__ zt = st.z_pi + (size_t)wt * L * P * 64 + lane;   // this wave tile's logits
  const size_t plane = (size_t)L * ldn;

  for (int l = l0; l < l1; ++l) {
    // per-bin constants, wave-uniform
    float rho;
    if (frozen) {
      rho = pr.rho_fixed[l];
    } else {
      float dm;
      rho = clipped_sigmoid(params[lay.off_rho + l], &dm);
    }
    const float* __restrict__ gl = pr.gcf + (size_t)l * K1;
    float dot = 0.0f;
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k) dot += (k < K1) ? beta[k] * gl[k] : 0.0f;

    const size_t e = (size_t)l * ldn + n;
    const float x = pr.reads[e];
    float z[P];
#pragma unroll
    for (int k = 0; k < P; ++k) z[k] = zt[((size_t)l * P + k) * 64];

    // omega, D and phi in the operations and order of the enumerated passes
    const float invx = x > 0.0f ? frcp(x) : 0.0f;
    const float omega = fexp(dot);                         // pert_model.py:633
    const float D = ucc * omega;                           // :636-640 (delta = chi D)
    const float t = tau - rho;                             // :616
    const float phi = frcp(1.0f + fexp(-a_val * t));       // :619
    float p_cn[P];
    const float p_rep = enum_posterior<P>(x, invx, z, log1m_lam, D, phi, p_cn);

    if (valid) {
      rep_prob[e] = p_rep;
      if (cn_prob) {
        // the marginal at the caller's state (select chain: no indexed local array); a state
        // outside [0, P) has probability 0
        const int cs = cn_state[e];
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k) v = (cs == k) ? p_cn[k] : v;
        cn_prob[e] = v;
      }
      if (cn_marg) {
#pragma unroll
        for (int k = 0; k < P; ++k) cn_marg[(size_t)k * plane + e] = p_cn[k];
      }
    }
  }
}

template <int P>
int selftest_posterior_host(int64_t n, const float* x, const float* z, float log1m_lam, const float* D,
                            const float* phi, float* p_rep, float* p_cn) {
  for (int64_t i = 0; i < n; ++i) {
    float zz[P], pc[P];
    for (int k = 0; k < P; ++k) zz[k] = z[i * P + k];
    const float xi = x[i];
    p_rep[i] = enum_posterior<P>(xi, xi > 0.0f ? 1.0f / xi : 0.0f, zz, log1m_lam, D[i], phi[i], pc);
    for (int k = 0; k < P; ++k) p_cn[i * P + k] = pc[k];
  }
  return PERT_OK;
}

// Posterior draws (pert_enum_draw): the launch shape, loads and per-element inputs of
// enum_posterior_kernel; the element's scores, weights and running sums are formed once
// (enum_draw_cdf) and n_draws draws are then taken from registers.  Draw g = first_draw + d of
// (bin l, global cell cell0 + n) uses word g & 3 of philox({l, cell low, g >> 2, cell high}) under
// the key of (seed, PERT_TAG_DRAWS): one Philox call serves four consecutive draws, and a draw
// depends on nothing but (seed, bin, global cell, g).  Stores are one byte per lane per draw
// plane: a wave writes one 64-byte row segment (layouts measured: DESIGN.md 6k).
template <int P>
__global__ void __launch_bounds__(64, 4) enum_draw_kernel(pert_problem pr, pert_state st, int LT, uint64_t seed,
                                                          int64_t cell0, int first_draw, int n_draws,
                                                          uint8_t* __restrict__ rep_draw,
                                                          uint8_t* __restrict__ cn_draw) {
  const int lane = threadIdx.x;
  const int wt = blockIdx.x, bt = blockIdx.y;
  const int N = pr.N, K1 = pr.K1, ldn = pr.ldn, L = pr.L;
  const int n = wt * 64 + lane;                 // < ldn: ldn is N rounded up to a multiple of 256
  const bool valid = n < N;
  const int l0 = bt * LT;
  const int l1 = min(L, l0 + LT);
  const bool frozen = pr.kind == PERT_KIND_STEP3;
  const pert_layout lay = st.lay;
  const float* __restrict__ params = st.params;

  // cell parameters, as enum_posterior_kernel
  const float a_val = frozen ? pr.a_fixed : fexp(params[lay.off_a]);
  const float c0 = (1.0f - pr.lamb) / pr.lamb;
  const float log1m_lam = pr.log1m_lam;
  float u = 0.0f, tau = 0.5f;
  float beta[PERT_MAX_K1];
#pragma unroll
  for (int k = 0; k < PERT_MAX_K1; ++k) beta[k] = 0.0f;
  if (valid) {
    u = params[lay.off_u + n];
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k)
      if (k < K1) beta[k] = params[lay.off_beta + k * N + n];
    float dm;
    tau = clipped_sigmoid(params[lay.off_tau + n], &dm);
  }
  const float ucc = u * c0;
  const float* __restrict__ zt = st.z_pi + (size_t)wt * L * P * 64 + lane;   // this wave tile's logits
  const size_t plane = (size_t)L * ldn;
  const pert_sim::Key key = pert_sim::make_key(seed, PERT_TAG_DRAWS);
  const uint64_t cell = (uint64_t)cell0 + (uint64_t)n;
  const int g_end = first_draw + n_draws;

  for (int l = l0; l < l1; ++l) {
    float rho;
    if (frozen) {
      rho = pr.rho_fixed[l];
    } else {
      float dm;
      rho = clipped_sigmoid(params[lay.off_rho + l], &dm);
    }
    const float* __restrict__ gl = pr.gcf + (size_t)l * K1;
    float dot = 0.0f;
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k) dot += (k < K1) ? beta[k] * gl[k] : 0.0f;

    const size_t e = (size_t)l * ldn + n;
    const float x = pr.reads[e];
    float z[P];
#pragma unroll
    for (int k = 0; k < P; ++k) z[k] = zt[((size_t)l * P + k) * 64];

    const float invx = x > 0.0f ? frcp(x) : 0.0f;
    const float omega = fexp(dot);
    const float D = ucc * omega;
    const float t = tau - rho;
    const float phi = frcp(1.0f + fexp(-a_val * t));
    float C[2 * P];
    const int jlast = enum_draw_cdf<P>(x, invx, z, log1m_lam, D, phi, C);

    if (valid) {
      uint8_t* __restrict__ rp = rep_draw + e;
      uint8_t* __restrict__ cp = cn_draw ? cn_draw + e : nullptr;
      for (int grp = first_draw >> 2; grp <= (g_end - 1) >> 2; ++grp) {
        const pert_sim::Words w = pert_sim::draw(key, (uint32_t)l, cell, (uint32_t)grp);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int g = grp * 4 + k;
          if (g >= first_draw && g < g_end) {
            const int j = enum_draw_pick<P>(C, jlast, pert_sim::u01(word[k]));
            const size_t o = (size_t)(g - first_draw) * plane;
            rp[o] = (uint8_t)(j & 1);
            if (cp) cp[o] = (uint8_t)(j >> 1);
          }
        }
      }
    }
  }
}

template <int P>
int selftest_draw_host(int64_t n, const float* x, const float* z, float log1m_lam, const float* D, const float* phi,
                       int32_t n_draws, const float* u, uint8_t* cn, uint8_t* rep) {
  for (int64_t i = 0; i < n; ++i) {
    float zz[P], C[2 * P];
    for (int k = 0; k < P; ++k) zz[k] = z[i * P + k];
    const float xi = x[i];
    const int jlast = enum_draw_cdf<P>(xi, xi > 0.0f ? 1.0f / xi : 0.0f, zz, log1m_lam, D[i], phi[i], C);
    for (int32_t d = 0; d < n_draws; ++d) {
      const int j = enum_draw_pick<P>(C, jlast, u[i * n_draws + d]);
      cn[i * n_draws + d] = (uint8_t)(j >> 1);
      rep[i * n_draws + d] = (uint8_t)(j & 1);
    }
  }
  return PERT_OK;
}

}  // namespace

extern "C" {

int pert_enum_posterior(const pert_problem* prob, const pert_state* st, const uint8_t* cn_state, float* rep_prob,
                        float* cn_prob, float* cn_marg, hipStream_t stream) {
  if (!prob || !st || !rep_prob) return PERT_E_ARG;
  if (prob->kind != PERT_KIND_STEP2 && prob->kind != PERT_KIND_STEP3) return PERT_E_ARG;
  if ((cn_state == nullptr) != (cn_prob == nullptr)) return PERT_E_ARG;
  if (prob->L < 1 || prob->N < 1 || prob->ldn < prob->N || prob->ldn % PERT_BLOCK != 0) return PERT_E_ARG;
  if (prob->P < PERT_MIN_P || prob->P > PERT_MAX_P) return PERT_E_UNSUPPORTED_P;
  if (prob->K1 < 1 || prob->K1 > PERT_MAX_K1) return PERT_E_UNSUPPORTED_K;
  if (!prob->reads || !prob->gcf || !st->params || !st->z_pi) return PERT_E_ARG;
  if (prob->kind == PERT_KIND_STEP3 && !prob->rho_fixed) return PERT_E_ARG;
  int lt = st->bins_per_tile > 0 ? st->bins_per_tile : kPostDefaultLT;
  lt = lt > kPostMaxLT ? kPostMaxLT : lt;
  const dim3 grid((unsigned)((prob->N + 63) / 64), (unsigned)((prob->L + lt - 1) / lt));
  if (grid.y > 65535u) return PERT_E_ARG;
  switch (prob->P) {
#define PERT_CASE(PP)                                                                                      \
  case PP:                                                                                                 \
    hipLaunchKernelGGL(enum_posterior_kernel<PP>, grid, dim3(64), 0, stream, *prob, *st, lt, cn_state,     \
                       rep_prob, cn_prob, cn_marg);                                                        \
    break;
    PERT_POST_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

int pert_selftest_enum_posterior_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                      const float* D, const float* phi, float* p_rep, float* p_cn) {
  if (n < 0 || (n > 0 && (!x || !z || !D || !phi || !p_rep || !p_cn))) return PERT_E_ARG;
  switch (P) {
#define PERT_CASE(PP) \
  case PP: return selftest_posterior_host<PP>(n, x, z, log1m_lam, D, phi, p_rep, p_cn);
    PERT_POST_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
}

int pert_enum_draw(const pert_problem* prob, const pert_state* st, uint64_t seed, int64_t cell0, int32_t first_draw,
                   int32_t n_draws, uint8_t* rep_draw, uint8_t* cn_draw, hipStream_t stream) {
  if (!prob || !st || !rep_draw) return PERT_E_ARG;
  if (prob->kind != PERT_KIND_STEP2 && prob->kind != PERT_KIND_STEP3) return PERT_E_ARG;
  if (prob->L < 1 || prob->N < 1 || prob->ldn < prob->N || prob->ldn % PERT_BLOCK != 0) return PERT_E_ARG;
  if (prob->P < PERT_MIN_P || prob->P > PERT_MAX_P) return PERT_E_UNSUPPORTED_P;
  if (prob->K1 < 1 || prob->K1 > PERT_MAX_K1) return PERT_E_UNSUPPORTED_K;
  if (!prob->reads || !prob->gcf || !st->params || !st->z_pi) return PERT_E_ARG;
  if (prob->kind == PERT_KIND_STEP3 && !prob->rho_fixed) return PERT_E_ARG;
  if (n_draws < 1 || n_draws > PERT_MAX_DRAWS || first_draw < 0 || first_draw > INT32_MAX - n_draws) return PERT_E_ARG;
  if (cell0 < 0) return PERT_E_ARG;
  int lt = st->bins_per_tile > 0 ? st->bins_per_tile : kPostDefaultLT;
  lt = lt > kPostMaxLT ? kPostMaxLT : lt;
  const dim3 grid((unsigned)((prob->N + 63) / 64), (unsigned)((prob->L + lt - 1) / lt));
  if (grid.y > 65535u) return PERT_E_ARG;
  switch (prob->P) {
#define PERT_CASE(PP)                                                                                      \
  case PP:                                                                                                 \
    hipLaunchKernelGGL(enum_draw_kernel<PP>, grid, dim3(64), 0, stream, *prob, *st, lt, seed, cell0,       \
                       first_draw, n_draws, rep_draw, cn_draw);                                            \
    break;
    PERT_POST_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

int pert_selftest_enum_draw_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                 const float* D, const float* phi, int32_t n_draws, const float* u, uint8_t* cn,
                                 uint8_t* rep) {
  if (n < 0 || n_draws < 1 || (n > 0 && (!x || !z || !D || !phi || !u || !cn || !rep))) return PERT_E_ARG;
  switch (P) {
#define PERT_CASE(PP) \
  case PP: return selftest_draw_host<PP>(n, x, z, log1m_lam, D, phi, n_draws, u, cn, rep);
    PERT_POST_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
}

}  // extern "C"
