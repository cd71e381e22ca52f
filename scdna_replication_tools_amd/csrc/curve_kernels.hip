// curve_kernels.hip -- per-cell likelihood curves over S-phase time tau (gfx950).
//
// After a step-2/3 fit every other consumer conditions on one number per cell, the fitted tau.
// tau enters an element's 2P joint scores through the Bernoulli term alone (pert_math.h), so with
// pi, u, beta, rho and a held at the fit the log marginal of (bin l, cell n) at ANY tau is
//   m_ln(tau) = log((1 - phi) exp(e_0) + phi exp(e_1)),  phi = clamp(sigmoid(a (tau - rho_l)))
// with the two branch evidences e_r = log sum_c exp(log pi~_c + NB'(c (1 + r))) independent of tau.
//
//   pert_enum_evidence  one pass in pert_enum_posterior's shape (one wave per 64-cell tile x bin
//                       tile, lanes are cells): the P logits and the 2P - 1 NB terms once per
//                       element, written as the two planes of ev.  The walk and the inputs of
//                       an element are enum_tile.h's, the posterior pass's own.
//   pert_tau_curve      curve[g][n] = sum_l m_ln(grid[g]) and at_fit[n] = sum_l m_ln(tau_n): a wave
//                       owns a 64-cell tile and kCurveChunk grid points, keeps their fp64 sums in
//                       registers and walks ALL bins in order l = 0 .. L-1.  So a sum depends on
//                       nothing but (ev, the parameters, the grid value): not on the launch
//                       geometry and not on how a caller chunks the grid; no workspace, no
//                       cross-wave reduction, no atomics, reruns bit-identical.
//
// Neither kernel writes anything of pert_state, and neither touches a column n >= N of an output.
#include "enum_tile.h"

#include <math.h>

namespace {

using namespace pert;

constexpr int kCurveChunk = 4;        // grid points per wave of tau_curve_kernel
constexpr int kBinBlock = 8;          // bins per block of its walk (loads in flight: 2 kBinBlock rows)

// enum_posterior_kernel's walk (enum_tile.h), so its launch shape, loads and the same x, z and D
// of an element; a, tau and rho are not read and phi is not formed.
template <int P>
__global__ void __launch_bounds__(64, 4) enum_evidence_kernel(pert_problem pr, pert_state st, int LT,
                                                              float* __restrict__ ev) {
  const EnumTile<P, false> t(pr, st, LT);
  for (int l = t.l0; l < t.l1; ++l) {
    EnumElem<P> el;
    t.load(pr, st, l, el);
    float e0, e1;
    enum_evidence<P>(el.x, el.invx, el.z, t.log1m_lam, el.D, e0, e1);
    if (t.valid) {
      ev[el.e] = e0;
      ev[t.plane + el.e] = e1;
    }
  }
}

// One wave: cells wt * 64 .. + 63, grid points g0 .. g0 + kCurveChunk - 1 (those < G), every bin.
// The waves of one cell tile are neighbours in the launch (the chunk index runs fastest), so the
// re-reads of the tile's evidences by its other chunks find them in the caches.
// The bins are walked in blocks of kBinBlock.  A wave's loads are two 256-byte rows per bin, a
// row stride apart, so the whole next block (2 kBinBlock rows) is requested before the current
// block's arithmetic: one bin's arithmetic is far shorter than a load's latency.
// phi of a (bin, grid point), and the two logarithms tau_mix takes of it, do not depend on the
// cell: per block, lane i * kCurveChunk + j forms them for bin i of the block and grid point j of
// the chunk, and each is then broadcast from that lane -- one evaluation per (bin, grid point) and
// wave, not one per element.  The broadcast copies a value; nothing is summed across lanes, and
// each (g, n) still adds its bins in the order l = 0 .. L-1.  The first wave of a cell tile
// (chunk 0) also sums the cells' own fitted tau into at_fit, with a per-lane phi.
__global__ void __launch_bounds__(64) tau_curve_kernel(pert_problem pr, pert_state st, const float* __restrict__ ev,
                                                       const float* __restrict__ grid, int G, int n_chunks,
                                                       double* __restrict__ curve, double* __restrict__ at_fit) {
  static_assert(kBinBlock * kCurveChunk <= 64, "one lane per (bin of the block, grid point of the chunk)");
  const int lane = threadIdx.x;
  const int wt = blockIdx.x / n_chunks;
  const int chunk = blockIdx.x - wt * n_chunks;
  const int g0 = chunk * kCurveChunk;
  const int N = pr.N, ldn = pr.ldn, L = pr.L;
  const int n = wt * 64 + lane;                 // < ldn
  const bool valid = n < N;
  const bool own = chunk == 0;
  const float a_val = fitted_a(pr, st);

  // this lane's (bin of a block, grid point of the chunk); lanes past kBinBlock * kCurveChunk repeat
  const int bi = (lane / kCurveChunk) % kBinBlock;
  const float tg = grid[min(g0 + lane % kCurveChunk, G - 1)];   // (the repeats past G are never stored)
  const float tau = valid ? cell_tau(st, n) : 0.5f;
  double acc[kCurveChunk];
#pragma unroll
  for (int j = 0; j < kCurveChunk; ++j) acc[j] = 0.0;
  double acc_fit = 0.0;

  const float* __restrict__ p0 = ev + n;
  const float* __restrict__ p1 = ev + (size_t)L * ldn + n;
  float c0[kBinBlock], c1[kBinBlock];
#pragma unroll
  for (int i = 0; i < kBinBlock; ++i) {
    const size_t o = (size_t)min(i, L - 1) * ldn;
    c0[i] = p0[o];
    c1[i] = p1[o];
  }
  for (int lb = 0; lb < L; lb += kBinBlock) {
    float n0[kBinBlock], n1[kBinBlock];           // the next block (rows past the last bin repeat it, unused)
#pragma unroll
    for (int i = 0; i < kBinBlock; ++i) {
      const size_t o = (size_t)min(lb + kBinBlock + i, L - 1) * ldn;
      n0[i] = p0[o];
      n1[i] = p1[o];
    }
    const int lm = min(lb + bi, L - 1);
    const float rho = bin_rho(pr, st, lm);
    float l1mphi, lphi;
    tau_mix_phi(frcp(1.0f + fexp(-a_val * (tg - rho))), l1mphi, lphi);   // the passes' own operations
#pragma unroll
    for (int i = 0; i < kBinBlock; ++i) {
      if (lb + i < L) {                           // (wave-uniform)
#pragma unroll
        for (int j = 0; j < kCurveChunk; ++j) {
          const float a0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l1mphi), i * kCurveChunk + j));
          const float a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lphi), i * kCurveChunk + j));
          acc[j] += (double)tau_mix_logs(c0[i], c1[i], a0, a1);
        }
        if (own) {
          const float rho_i = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rho), i * kCurveChunk));
          const float phi = frcp(1.0f + fexp(-a_val * (tau - rho_i)));
          acc_fit += (double)tau_mix(c0[i], c1[i], phi);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBinBlock; ++i) {
      c0[i] = n0[i];
      c1[i] = n1[i];
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < kCurveChunk; ++j)
      if (g0 + j < G) curve[(size_t)(g0 + j) * N + n] = acc[j];
    if (own) at_fit[n] = acc_fit;
  }
}

template <int P>
int selftest_evidence_host(int64_t n, const float* x, const float* z, float log1m_lam, const float* D, float* ev0,
                           float* ev1) {
  for (int64_t i = 0; i < n; ++i) {
    float zz[P];
    for (int k = 0; k < P; ++k) zz[k] = z[i * P + k];
    const float xi = x[i];
    enum_evidence<P>(xi, xi > 0.0f ? 1.0f / xi : 0.0f, zz, log1m_lam, D[i], ev0[i], ev1[i]);
  }
  return PERT_OK;
}

}  // namespace

extern "C" {

int pert_enum_evidence(const pert_problem* prob, const pert_state* st, float* ev, hipStream_t stream) {
  const int rc = check_enum_args(prob, st, ev);
  if (rc != PERT_OK) return rc;
  const int lt = enum_tile_len(st);
  dim3 grid;
  if (!enum_grid(prob, lt, grid)) return PERT_E_ARG;
  switch (prob->P) {
#define PERT_CASE(PP)                                                                                 \
  case PP:                                                                                            \
    hipLaunchKernelGGL(enum_evidence_kernel<PP>, grid, dim3(64), 0, stream, *prob, *st, lt, ev);      \
    break;
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
  return launch_status();
}

int pert_tau_curve(const pert_problem* prob, const pert_state* st, const float* ev, const float* grid, int32_t G,
                   double* curve, double* at_fit, hipStream_t stream) {
  if (!prob || !st || !ev || !grid || !curve || !at_fit) return PERT_E_ARG;
  if (prob->kind != PERT_KIND_STEP2 && prob->kind != PERT_KIND_STEP3) return PERT_E_ARG;
  if (G < 1 || G > PERT_TAU_MAX_GRID) return PERT_E_ARG;
  if (prob->L < 1 || prob->N < 1 || prob->ldn < prob->N || prob->ldn % PERT_BLOCK != 0) return PERT_E_ARG;
  if (!st->params) return PERT_E_ARG;
  if (prob->kind == PERT_KIND_STEP3 && !prob->rho_fixed) return PERT_E_ARG;
  const int n_chunks = (G + kCurveChunk - 1) / kCurveChunk;                 // <= 256
  const int64_t waves = ((int64_t)prob->N + 63) / 64 * n_chunks;
  if (waves > INT32_MAX) return PERT_E_ARG;
  hipLaunchKernelGGL(tau_curve_kernel, dim3((unsigned)waves), dim3(64), 0, stream, *prob, *st, ev, grid, (int)G,
                     n_chunks, curve, at_fit);
  return launch_status();
}

int pert_selftest_enum_evidence_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                     const float* D, float* ev0, float* ev1) {
  if (n < 0 || (n > 0 && (!x || !z || !D || !ev0 || !ev1))) return PERT_E_ARG;
  switch (P) {
#define PERT_CASE(PP) \
  case PP: return selftest_evidence_host<PP>(n, x, z, log1m_lam, D, ev0, ev1);
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
}

int pert_selftest_tau_mix_host(int64_t n, const float* ev0, const float* ev1, const float* phi, float* m) {
  if (n < 0 || (n > 0 && (!ev0 || !ev1 || !phi || !m))) return PERT_E_ARG;
  for (int64_t i = 0; i < n; ++i) m[i] = tau_mix(ev0[i], ev1[i], phi[i]);
  return PERT_OK;
}

}  // extern "C"
