// bin_kernels.hip -- gfx950 kernel of the threshold binarisation of RT profiles (binarize.py).
//
// Reference: binarize_rt_profiles.py:44-117 (Dileep & Gilbert): per cell a 2-component
// GaussianMixture(random_state=0) on the raw float64 profile (sklearn: KMeans tolerance from the
// uncentred data, centring, k-means++ with 2 + floor(log 2) local trials, Lloyd, EM, fit_predict's
// final E step), the two binary levels (the GMM means, or percentiles chosen by the biased skew
// when the means are closer than MEAN_GAP_THRESH), then the 100 fixed thresholds
// np.linspace(-3, 3, 100): the first one of least sum |X - where(X > t, b1, b0)|.
//
// The stage is the same algorithm as tau_kernels.hip's (one 256-thread workgroup per cell runs
// every loop to its own stopping iteration, fp64, fixed-order block sums: reruns are
// bit-identical), on the double profile itself instead of the standardised fp32 reads, with the
// reference's outputs (covariances, GMM labels, binary states, the whole distance table) and
// with the margins of an fp64-vs-fp64 comparison, all passed in pert_bin_params.  The stages the
// two kernels share are in gmm2_stages.h.  The scan sums each threshold's distance directly (10
// thresholds per pass over the profile): the tau kernel's 2^-32 fixed-point histogram is too
// coarse for a distance table compared at rounding level.

#include "gmm2_stages.h"

namespace {

using namespace gmm2;
using namespace gmm2::f64;   // Cell, assign2, lloyd

constexpr int kNT = PERT_BIN_THRESHOLDS;
constexpr int kTG = 10;                 // thresholds per scan pass
enum { kEmTol, kRegCovar, kMeanGap, kEarly, kLate, kEmMargin, kGapMargin, kSkewMargin, kRespMargin, kThreshMargin,
       kDistMargin, kNPar };   // slots of the kernel's LDS copy of the late-stage parameters

// em2's constants, from the kernel's LDS copy
struct EmConsts {
  const double* s_par;
  __device__ __forceinline__ double em_tol() const { return s_par[kEmTol]; }
  __device__ __forceinline__ double em_margin() const { return s_par[kEmMargin]; }
  __device__ __forceinline__ double reg_covar() const { return s_par[kRegCovar]; }
};

__global__ __launch_bounds__(kT) void rt_binarize_kernel(int L, int N, const double* __restrict__ x,
                                                            pert_bin_params p, double* __restrict__ means,
                                                            double* __restrict__ covs,
                                                            int8_t* __restrict__ gmm_state,
                                                            uint8_t* __restrict__ rt_state,
                                                            double* __restrict__ dist, int32_t* __restrict__ best,
                                                            int32_t* __restrict__ n_rep,
                                                            int32_t* __restrict__ flags) {
  __shared__ double sm[2 * kTG * kTW];
  __shared__ double sval[2];
  __shared__ int smi[kTW];
  __shared__ SelectLds s_sel;
  __shared__ double s_th[kNT];
  __shared__ double s_d[kNT];
  __shared__ int s_cnt[kNT];
  __shared__ double s_par[kNPar];
  const int n = blockIdx.x;
  if (n >= N) return;
  const size_t row = (size_t)n * (size_t)L;
  int8_t* lab1 = gmm_state + row;                                   // Lloyd's labels until the final E step
  int8_t* lab_old = reinterpret_cast<int8_t*>(rt_state + row);      // Lloyd's previous labels until the scan
  Cell c;
  c.x = x + row;
  c.L = L;
  if (threadIdx.x < kNT) s_th[threadIdx.x] = p.thresh[threadIdx.x];
  // the parameters of the later stages wait in LDS, not in scalar registers held through the
  // k-means and EM loops (the first block sum's barrier orders these writes before any read)
  if (threadIdx.x == 0) {
    s_par[kEmTol] = p.em_tol;
    s_par[kRegCovar] = p.reg_covar;
    s_par[kMeanGap] = p.mean_gap;
    s_par[kEarly] = p.early_skew;
    s_par[kLate] = p.late_skew;
    s_par[kEmMargin] = p.em_margin;
    s_par[kGapMargin] = p.gap_margin;
    s_par[kSkewMargin] = p.skew_margin;
    s_par[kRespMargin] = p.resp_margin;
    s_par[kThreshMargin] = p.thresh_margin;
    s_par[kDistMargin] = p.dist_margin;
  }

  // ---- KMeans: tolerance from the uncentred data (mean variance x 1e-4), then centring
  double sumXc, tol;
  {
    double a[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) a[0] += c.X(i);
    block_sums<1>(a, sm);
    c.mX = a[0] / (double)L;
    double q[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double d = c.Xc(i);
      q[0] += d;
      q[1] += d * d;
    }
    block_sums<2>(q, sm);
    sumXc = q[0];
    tol = q[1] / (double)L * 1e-4;
  }

  // ---- k-means++ for 2 centres, then Lloyd
  int flag = 0;
  {
    double cen0, cen1;
    int cand[2];
    if (kmeans_pp2(c, p, &cen0, &cen1, cand, sm, smi, sval)) flag |= PERT_BIN_F_PP;
    bool fr = false;
    lloyd(c, cen0, cen1, tol, sumXc, p, lab_old, lab1, &fr, sm);
    if (fr) flag |= PERT_BIN_F_LLOYD;
  }

  // ---- EM of the 2-component 1-D mixture from the k-means labels
  Mix fit;
  em2(c, lab1, p.em_max_iter, EmConsts{s_par}, &fit, &flag, (int)PERT_BIN_F_EM, sm);
  const double mu0 = fit.mu0, mu1 = fit.mu1;

  // ---- fit_predict's final E step with the fitted parameters: gmm_state = argmax (first on a tie)
  {
    const LogProb e(fit);
    const double resp_margin = s_par[kRespMargin];
    double nr[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      double l0, l1;
      e.weighted(X, &l0, &l1);
      lab1[i] = l1 > l0 ? 1 : 0;
      nr[0] += (fabs(l1 - l0) <= resp_margin * (1.0 + fabs(l0) + fabs(l1))) ? 1.0 : 0.0;
    }
    block_sums<1>(nr, sm);
    if (nr[0] > 0.0) flag |= PERT_BIN_F_RESP;
  }

  // ---- levels (binarize_rt_profiles.py:59-85): the GMM means, or percentiles of the profile
  // chosen by its biased skew when the means are closer than MEAN_GAP_THRESH
  double b0, b1;
  if (levels2(c, p, mu0, mu1,
              LevelTests{s_par[kMeanGap], s_par[kGapMargin] * fmax(1.0, fabs(mu0) + fabs(mu1)), s_par[kEarly],
                         s_par[kLate], s_par[kSkewMargin]},
              &b0, &b1, sm, &s_sel))
    flag |= PERT_BIN_F_LEVELS;

  // ---- the scan (:89-101): per threshold the Manhattan distance and the count above it, kTG
  // thresholds per pass over the profile, each a fixed-order block sum
  for (int g = 0; g < kNT / kTG; ++g) {
    double acc[2 * kTG];
#pragma unroll
    for (int k = 0; k < 2 * kTG; ++k) acc[k] = 0.0;
    double th[kTG];
#pragma unroll
    for (int k = 0; k < kTG; ++k) th[k] = s_th[g * kTG + k];
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double e0 = fabs(X - b0), e1 = fabs(X - b1);
#pragma unroll
      for (int k = 0; k < kTG; ++k) {
        const bool hi = X > th[k];
        acc[k] += hi ? e1 : e0;
        acc[kTG + k] += hi ? 1.0 : 0.0;
      }
    }
    block_sums<2 * kTG>(acc, sm);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kTG; ++k) {
        s_d[g * kTG + k] = acc[k];
        s_cnt[g * kTG + k] = (int)acc[kTG + k];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int bi = 0;
    for (int i = 1; i < kNT; ++i)
      if (s_d[i] < s_d[bi]) bi = i;                                     // first strict minimum
    smi[0] = bi;
  }
  __syncthreads();
  const int bi = smi[0];
  const double dmin = s_d[bi], tbest = s_th[bi];
  const int cbest = s_cnt[bi];
  __syncthreads();                                                      // smi is reused below
  bool other = false;
  if (threadIdx.x < kNT) {
    const int i = threadIdx.x;
    const double slack = s_par[kDistMargin] * (dmin + (double)L * fmax(fabs(b0), fabs(b1)));
    other = s_cnt[i] != cbest && s_d[i] - dmin <= slack;
    dist[(size_t)n * kNT + i] = s_d[i];
  }
  bool point = false;
  const double thresh_margin = s_par[kThreshMargin];
  uint8_t* rs = rt_state + row;
  for (int i = threadIdx.x; i < L; i += kT) {
    const double X = c.X(i);
    rs[i] = X > tbest ? 1 : 0;
    point = point || (thresh_margin > 0.0 && fabs(X - tbest) <= thresh_margin);
  }
  if (block_min_i(other ? 0 : 1, smi) == 0) flag |= PERT_BIN_F_SCAN;
  if (block_min_i(point ? 0 : 1, smi) == 0) flag |= PERT_BIN_F_POINT;

  if (threadIdx.x == 0) {
    means[2 * n] = mu0;
    means[2 * n + 1] = mu1;
    covs[2 * n] = fit.var0;
    covs[2 * n + 1] = fit.var1;
    best[n] = bi;
    n_rep[n] = cbest;
    flags[n] = flag;
  }
}

}  // namespace

extern "C" int pert_rt_binarize(int32_t L, int32_t N, const double* x, const pert_bin_params* p, double* means,
                                double* covs, int8_t* gmm_state, uint8_t* rt_state, double* dist, int32_t* best,
                                int32_t* n_rep, int32_t* flags, hipStream_t stream) {
  if (L < 2 || N < 1 || !x || !p || !means || !covs || !gmm_state || !rt_state || !dist || !best || !n_rep || !flags)
    return PERT_E_ARG;
  if (!gmm2::params_ok(L, *p)) return PERT_E_ARG;
  hipLaunchKernelGGL(rt_binarize_kernel, dim3(N), dim3(gmm2::kT), 0, stream, L, N, x, *p, means, covs, gmm_state,
                     rt_state, dist, best, n_rep, flags);
  return gmm2::launch_status();
}
