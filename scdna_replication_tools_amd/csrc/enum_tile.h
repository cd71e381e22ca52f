// enum_tile.h -- the wave-tile walk of the post-fit passes over every (bin, cell) (gfx950).
//
// pert_enum_posterior, pert_enum_draw (post_kernels.hip) and pert_enum_evidence (curve_kernels.hip)
// launch one wave per (64-cell tile, bin tile), lanes are cells (as enum3_kernel): per-cell u, tau
// and betas live in registers, per-bin rho and GC features are wave-uniform loads, the P logits
// of a bin are P coalesced 256-byte rows of the z_pi wave tile.  This header is the one place
// where an element's inputs (x, 1/x, z, D, phi) are formed, in the operations and order of the
// enumerated passes: the three passes agree bit for bit on them because they share this code.
// It also owns what their entry points share on the host: the list of P, the argument checks,
// the tile length, the grid and the launch status.
#pragma once

#include "../../include/pert_hip.h"
#include "pert_math.h"

#include <stddef.h>

namespace pert {

// every supported P
#define PERT_ENUM_P_CASES                                                                       \
  PERT_CASE(2) PERT_CASE(3) PERT_CASE(4) PERT_CASE(5) PERT_CASE(6) PERT_CASE(7) PERT_CASE(8)    \
  PERT_CASE(9) PERT_CASE(10) PERT_CASE(11) PERT_CASE(12) PERT_CASE(13) PERT_CASE(14)            \
  PERT_CASE(15) PERT_CASE(16)

// the fitted parameters phi = sigmoid(a (tau - rho)) is formed from (tau_curve_kernel's too)
__device__ __forceinline__ float fitted_a(const pert_problem& pr, const pert_state& st) {
  return pr.kind == PERT_KIND_STEP3 ? pr.a_fixed : fexp(st.params[st.lay.off_a]);
}
__device__ __forceinline__ float cell_tau(const pert_state& st, int n) {
  float dm;
  return clipped_sigmoid(st.params[st.lay.off_tau + n], &dm);
}
__device__ __forceinline__ float bin_rho(const pert_problem& pr, const pert_state& st, int l) {
  if (pr.kind == PERT_KIND_STEP3) return pr.rho_fixed[l];
  float dm;
  return clipped_sigmoid(st.params[st.lay.off_rho + l], &dm);
}

// the inputs of one element: e indexes [L][ldn] planes; phi is formed only where wanted
template <int P>
struct EnumElem {
  size_t e;
  float x, invx, z[P], D, phi;
};

// One wave's tile: cell n = 64 wt + lane, bins l0 .. l1 - 1.  PHI = false loads and computes
// nothing of a, tau or rho.
template <int P, bool PHI>
struct EnumTile {
  int n, l0, l1;
  bool valid;                                   // n < N: padded lanes compute and never store
  float a_val, log1m_lam, ucc, tau;
  float beta[PERT_MAX_K1];
  const float* zt;                              // this wave tile's logits
  size_t plane;                                 // L * ldn

  __device__ __forceinline__ EnumTile(const pert_problem& pr, const pert_state& st, int LT) {
    const int lane = threadIdx.x;
    const int wt = blockIdx.x, bt = blockIdx.y;
    const int N = pr.N, K1 = pr.K1, L = pr.L;
    n = wt * 64 + lane;                         // < ldn: ldn is N rounded up to a multiple of 256
    valid = n < N;
    l0 = bt * LT;
    l1 = min(L, l0 + LT);
    const float* __restrict__ params = st.params;

    // cell parameters (padded lanes: u = 0, so D = 0 and every chain is clamped; never stored)
    if constexpr (PHI) a_val = fitted_a(pr, st);
    const float c0 = (1.0f - pr.lamb) / pr.lamb;
    log1m_lam = pr.log1m_lam;
    float u = 0.0f;
    tau = 0.5f;
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k) beta[k] = 0.0f;
    if (valid) {
      u = params[st.lay.off_u + n];
#pragma unroll
      for (int k = 0; k < PERT_MAX_K1; ++k)
        if (k < K1) beta[k] = params[st.lay.off_beta + k * N + n];
      if constexpr (PHI) tau = cell_tau(st, n);
    }
    ucc = u * c0;
    zt = st.z_pi + (size_t)wt * L * P * 64 + lane;
    plane = (size_t)L * pr.ldn;
  }

  __device__ __forceinline__ void load(const pert_problem& pr, const pert_state& st, int l, EnumElem<P>& el) const {
    // per-bin constants, wave-uniform
    float rho = 0.0f;
    if constexpr (PHI) rho = bin_rho(pr, st, l);
    const int K1 = pr.K1;
    const float* __restrict__ gl = pr.gcf + (size_t)l * K1;
    float dot = 0.0f;
#pragma unroll
    for (int k = 0; k < PERT_MAX_K1; ++k) dot += (k < K1) ? beta[k] * gl[k] : 0.0f;

    el.e = (size_t)l * pr.ldn + n;
    el.x = pr.reads[el.e];
#pragma unroll
    for (int k = 0; k < P; ++k) el.z[k] = zt[((size_t)l * P + k) * 64];

    // omega, D and phi in the operations and order of the enumerated passes
    el.invx = el.x > 0.0f ? frcp(el.x) : 0.0f;
    const float omega = fexp(dot);                           // pert_model.py:633
    el.D = ucc * omega;                                      // :636-640 (delta = chi D)
    if constexpr (PHI) {
      const float t = tau - rho;                             // :616
      el.phi = frcp(1.0f + fexp(-a_val * t));                // :619
    }
  }
};

// ---------------------------------------------------------------------------- host side
// The checks the three passes share, in this order (out: the pass's first output).
inline int check_enum_args(const pert_problem* prob, const pert_state* st, const void* out) {
  if (!prob || !st || !out) return PERT_E_ARG;
  if (prob->kind != PERT_KIND_STEP2 && prob->kind != PERT_KIND_STEP3) return PERT_E_ARG;
  if (prob->L < 1 || prob->N < 1 || prob->ldn < prob->N || prob->ldn % PERT_BLOCK != 0) return PERT_E_ARG;
  if (prob->P < PERT_MIN_P || prob->P > PERT_MAX_P) return PERT_E_UNSUPPORTED_P;
  if (prob->K1 < 1 || prob->K1 > PERT_MAX_K1) return PERT_E_UNSUPPORTED_K;
  if (!prob->reads || !prob->gcf || !st->params || !st->z_pi) return PERT_E_ARG;
  if (prob->kind == PERT_KIND_STEP3 && !prob->rho_fixed) return PERT_E_ARG;
  return PERT_OK;
}

// bins per tile: the state's, 32 when it names none (as the passes), at most 64
inline int enum_tile_len(const pert_state* st) {
  const int lt = st->bins_per_tile > 0 ? st->bins_per_tile : 32;
  return lt > 64 ? 64 : lt;
}

// one wave per (64-cell tile, bin tile); false when the bin tiles exceed a grid's y extent
inline bool enum_grid(const pert_problem* prob, int lt, dim3& grid) {
  grid = dim3((unsigned)((prob->N + 63) / 64), (unsigned)((prob->L + lt - 1) / lt));
  return grid.y <= 65535u;
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

}  // namespace pert
