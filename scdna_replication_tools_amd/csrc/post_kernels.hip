// post_kernels.hip -- posterior marginals and posterior draws of the enumerated latent states (gfx950).
//
// After a step-2/3 fit the decode (pert_enum_pass, PERT_MODE_DECODE) gives the joint MAP state of
// every (bin, cell).  This pass gives the probabilities that call is made from: at the fitted
// parameters the posterior over the 2P joint states of an element is gamma = softmax_{c,r} s(c, r)
// (pert_math.h), and the kernel writes its marginals P(rep = 1) and P(cn = k).
//
// One wave per (64-cell tile, bin tile), lanes are cells; the walk, its loads and the inputs of an
// element (x, z, D, phi) are enum_tile.h's, shared with pert_enum_evidence.  Plain global loads:
// this runs once after a fit, not in the SVI loop.  Nothing is reduced across lanes and nothing
// is added to atomically, so reruns are bit-identical.  Nothing of pert_state is written.
#include "enum_tile.h"
#include "sim_math.h"

#include <math.h>

namespace {

using namespace pert;

template <int P>
__global__ void __launch_bounds__(64, 4) enum_posterior_kernel(pert_problem pr, pert_state st, int LT,
                                                               const uint8_t* __restrict__ cn_state,
                                                               float* __restrict__ rep_prob,
                                                               float* __restrict__ cn_prob,
                                                               float* __restrict__ cn_marg) {
  const EnumTile<P, true> t(pr, st, LT);
  for (int l = t.l0; l < t.l1; ++l) {
    EnumElem<P> el;
    t.load(pr, st, l, el);
    float p_cn[P];
    const float p_rep = enum_posterior<P>(el.x, el.invx, el.z, t.log1m_lam, el.D, el.phi, p_cn);

    if (t.valid) {
      rep_prob[el.e] = p_rep;
      if (cn_prob) {
        // the marginal at the caller's state (select chain: no indexed local array); a state
        // outside [0, P) has probability 0
        const int cs = cn_state[el.e];
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < P; ++k) v = (cs == k) ? p_cn[k] : v;
        cn_prob[el.e] = v;
      }
      if (cn_marg) {
#pragma unroll
        for (int k = 0; k < P; ++k) cn_marg[(size_t)k * t.plane + el.e] = p_cn[k];
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

// Posterior draws (pert_enum_draw): the same walk (enum_tile.h), so the launch shape, loads and
// per-element inputs of enum_posterior_kernel; the element's scores, weights and running sums are
// formed once (enum_draw_cdf) and n_draws draws are then taken from registers.  Draw g = first_draw + d of
// (bin l, global cell cell0 + n) uses word g & 3 of philox({l, cell low, g >> 2, cell high}) under
// the key of (seed, PERT_TAG_DRAWS): one Philox call serves four consecutive draws, and a draw
// depends on nothing but (seed, bin, global cell, g).  Stores are one byte per lane per draw
// plane: a wave writes one 64-byte row segment (layouts measured: DESIGN.md 6k).
template <int P>
__global__ void __launch_bounds__(64, 4) enum_draw_kernel(pert_problem pr, pert_state st, int LT, uint64_t seed,
                                                          int64_t cell0, int first_draw, int n_draws,
                                                          uint8_t* __restrict__ rep_draw,
                                                          uint8_t* __restrict__ cn_draw) {
  const EnumTile<P, true> t(pr, st, LT);
  const pert_sim::Key key = pert_sim::make_key(seed, PERT_TAG_DRAWS);
  const uint64_t cell = (uint64_t)cell0 + (uint64_t)t.n;
  const int g_end = first_draw + n_draws;

  for (int l = t.l0; l < t.l1; ++l) {
    EnumElem<P> el;
    t.load(pr, st, l, el);
    float C[2 * P];
    const int jlast = enum_draw_cdf<P>(el.x, el.invx, el.z, t.log1m_lam, el.D, el.phi, C);

    if (t.valid) {
      uint8_t* __restrict__ rp = rep_draw + el.e;
      uint8_t* __restrict__ cp = cn_draw ? cn_draw + el.e : nullptr;
      for (int grp = first_draw >> 2; grp <= (g_end - 1) >> 2; ++grp) {
        const pert_sim::Words w = pert_sim::draw(key, (uint32_t)l, cell, (uint32_t)grp);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int g = grp * 4 + k;
          if (g >= first_draw && g < g_end) {
            const int j = enum_draw_pick<P>(C, jlast, pert_sim::u01(word[k]));
            const size_t o = (size_t)(g - first_draw) * t.plane;
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
  // the pair check reads nothing and returns what the shared checks before P's return
  if ((cn_state == nullptr) != (cn_prob == nullptr)) return PERT_E_ARG;
  const int rc = check_enum_args(prob, st, rep_prob);
  if (rc != PERT_OK) return rc;
  const int lt = enum_tile_len(st);
  dim3 grid;
  if (!enum_grid(prob, lt, grid)) return PERT_E_ARG;
  switch (prob->P) {
#define PERT_CASE(PP)                                                                                      \
  case PP:                                                                                                 \
    hipLaunchKernelGGL(enum_posterior_kernel<PP>, grid, dim3(64), 0, stream, *prob, *st, lt, cn_state,     \
                       rep_prob, cn_prob, cn_marg);                                                        \
    break;
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
  return launch_status();
}

int pert_selftest_enum_posterior_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                      const float* D, const float* phi, float* p_rep, float* p_cn) {
  if (n < 0 || (n > 0 && (!x || !z || !D || !phi || !p_rep || !p_cn))) return PERT_E_ARG;
  switch (P) {
#define PERT_CASE(PP) \
  case PP: return selftest_posterior_host<PP>(n, x, z, log1m_lam, D, phi, p_rep, p_cn);
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
}

int pert_enum_draw(const pert_problem* prob, const pert_state* st, uint64_t seed, int64_t cell0, int32_t first_draw,
                   int32_t n_draws, uint8_t* rep_draw, uint8_t* cn_draw, hipStream_t stream) {
  const int rc = check_enum_args(prob, st, rep_draw);
  if (rc != PERT_OK) return rc;
  if (n_draws < 1 || n_draws > PERT_MAX_DRAWS || first_draw < 0 || first_draw > INT32_MAX - n_draws) return PERT_E_ARG;
  if (cell0 < 0) return PERT_E_ARG;
  const int lt = enum_tile_len(st);
  dim3 grid;
  if (!enum_grid(prob, lt, grid)) return PERT_E_ARG;
  switch (prob->P) {
#define PERT_CASE(PP)                                                                                      \
  case PP:                                                                                                 \
    hipLaunchKernelGGL(enum_draw_kernel<PP>, grid, dim3(64), 0, stream, *prob, *st, lt, seed, cell0,       \
                       first_draw, n_draws, rep_draw, cn_draw);                                            \
    break;
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
  return launch_status();
}

int pert_selftest_enum_draw_host(int32_t P, int64_t n, const float* x, const float* z, float log1m_lam,
                                 const float* D, const float* phi, int32_t n_draws, const float* u, uint8_t* cn,
                                 uint8_t* rep) {
  if (n < 0 || n_draws < 1 || (n > 0 && (!x || !z || !D || !phi || !u || !cn || !rep))) return PERT_E_ARG;
  switch (P) {
#define PERT_CASE(PP) \
  case PP: return selftest_draw_host<PP>(n, x, z, log1m_lam, D, phi, n_draws, u, cn, rep);
    PERT_ENUM_P_CASES
#undef PERT_CASE
    default: return PERT_E_UNSUPPORTED_P;
  }
}

}  // extern "C"
