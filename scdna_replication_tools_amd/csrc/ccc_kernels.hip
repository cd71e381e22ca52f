// ccc_kernels.hip -- gfx950 kernel of the cell-cycle-classifier features (ccc_features.py).
//
// Reference: compute_ccc_features.py:18-56, per cell: the log likelihood ratio statistic of a
// 1-component against a 2-component GaussianMixture of the cell's float64 profile (both with
// random_state=None: the draws are the caller's, per cell), the median absolute difference of
// adjacent bins, and the copy-number breakpoints counted within chromosomes.
//
// One 256-thread workgroup per cell runs every loop to its own stopping iteration, in fp64 with
// fixed-order block sums (reruns are bit-identical), as rt_binarize_kernel does; the k-means++ /
// Lloyd / EM stages are the ones of gmm2_stages.h with this kernel's margins, and a decision
// within its margin sets the PERT_BIN_F_* bit of its stage (the caller recomputes that cell's
// scores on the host).  The median is exact: a radix select of the two middle order statistics
// over a view of the differences.

#include "gmm2_stages.h"

namespace {

using namespace gmm2;
using namespace gmm2::f64;   // Cell, assign2, lloyd

// kmeans_pp2's parameters for one cell: its own draws, the launch's margin
struct CellDraws {
  int first;
  double u[2];
  double pp_margin;
};

// em2's constants, from the kernel's parameter struct
struct EmConsts {
  double tol, margin, reg;
  __device__ __forceinline__ double em_tol() const { return tol; }
  __device__ __forceinline__ double em_margin() const { return margin; }
  __device__ __forceinline__ double reg_covar() const { return reg; }
};

// select4's view of the L - 1 absolute differences of adjacent bins
struct AbsDiffs {
  const double* x;
  int L;               // the number of differences
  __device__ __forceinline__ double X(int i) const { return fabs(x[i + 1] - x[i]); }
};

__global__ __launch_bounds__(kT) void ccc_features_kernel(int L, int N, const double* __restrict__ x,
                                                             const int32_t* __restrict__ first2,
                                                             const double* __restrict__ u,
                                                             const int32_t* __restrict__ state,
                                                             const int32_t* __restrict__ chrom, pert_ccc_params p,
                                                             int8_t* __restrict__ scratch,
                                                             double* __restrict__ score1,
                                                             double* __restrict__ score2, double* __restrict__ lrs,
                                                             double* __restrict__ madn,
                                                             int32_t* __restrict__ breakpoints,
                                                             int32_t* __restrict__ flags) {
  __shared__ double sm[5 * kTW];
  __shared__ double sval[2];
  __shared__ int smi[kTW];
  __shared__ SelectLds s_sel;
  const int n = blockIdx.x;
  if (n >= N) return;
  const size_t row = (size_t)n * (size_t)L;
  int8_t* lab_old = scratch + row;                                   // Lloyd's previous labels
  int8_t* lab1 = scratch + (size_t)N * (size_t)L + row;              // Lloyd's labels, EM's start
  Cell c;
  c.x = x + row;
  c.L = L;

  // ---- the sum of the profile: KMeans' centring mean and the 1-component mean
  double sumX;
  {
    double a[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) a[0] += c.X(i);
    block_sums<1>(a, sm);
    sumX = a[0];
  }
  c.mX = sumX / (double)L;

  // ---- one component (sklearn's M step of all-one responsibilities): the mean log density
  double s1;
  {
    const double nk = (double)L + kEps10;
    const double mean = sumX / nk;
    double q[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double d = c.X(i) - mean;
      q[0] += d * d;
    }
    block_sums<1>(q, sm);
    const double var = q[0] / nk + p.reg_covar;
    const double pr = 1.0 / sqrt(var), lp = log(pr);
    double a[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double y = (c.X(i) - mean) * pr;
      a[0] += -0.5 * (kLog2Pi + y * y) + lp;
    }
    block_sums<1>(a, sm);
    s1 = a[0] / (double)L;
  }

  // ---- KMeans: tolerance from the uncentred data (mean variance x 1e-4), on the centred data
  double sumXc, tol;
  {
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

  // ---- k-means++ for 2 centres from this cell's draws, then Lloyd
  int flag = 0;
  {
    const CellDraws dr{first2[n], {u[2 * n], u[2 * n + 1]}, p.pp_margin};
    double cen0, cen1;
    int cand[2];
    if (kmeans_pp2(c, dr, &cen0, &cen1, cand, sm, smi, sval)) flag |= PERT_BIN_F_PP;
    bool fr = false;
    lloyd(c, cen0, cen1, tol, sumXc, p, lab_old, lab1, &fr, sm);
    if (fr) flag |= PERT_BIN_F_LLOYD;
  }

  // ---- EM from the k-means labels, then score(): the mean log probability under the final
  // parameters (after the last M step), not the loop's lower bound
  Mix fit;
  em2(c, lab1, p.em_max_iter, EmConsts{p.em_tol, p.em_margin, p.reg_covar}, &fit, &flag, (int)PERT_BIN_F_EM, sm);
  double s2;
  {
    const LogProb e(fit);
    double a[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      double lpn, r0, r1;
      e.resp(c.X(i), &lpn, &r0, &r1);
      a[0] += lpn;
    }
    block_sums<1>(a, sm);
    s2 = a[0] / (double)L;
  }

  // ---- madn: np.median of the L - 1 absolute differences (the middle order statistic, or the
  // mean of the two middle ones)
  double med;
  {
    const AbsDiffs d{c.x, L - 1};
    const int m = L - 1, lo = (m - 1) / 2, hi = m / 2;
    const int rank[4] = {lo, hi, lo, hi};
    double v[4];
    select4(d, rank, v, s_sel.hist, s_sel.pref, s_sel.k);
    med = lo == hi ? v[0] : (v[0] + v[1]) / 2.0;
  }

  // ---- breakpoints: state changes between adjacent rows of one chromosome
  int bk = 0;
  if (state != nullptr) {
    const int32_t* st = state + row;
    const int32_t* ch = chrom + row;
    double a[1] = {0.0};
    for (int i = 1 + threadIdx.x; i < L; i += kT) a[0] += (st[i] != st[i - 1] && ch[i] == ch[i - 1]) ? 1.0 : 0.0;
    block_sums<1>(a, sm);
    bk = (int)a[0];
  }

  if (threadIdx.x == 0) {
    score1[n] = s1;
    score2[n] = s2;
    lrs[n] = -2.0 * (s1 - s2);
    madn[n] = med;
    breakpoints[n] = bk;
    flags[n] = flag;
  }
}

}  // namespace

extern "C" int pert_ccc_features(int32_t L, int32_t N, const double* x, const int32_t* first1, const int32_t* first2,
                                 const double* u, const int32_t* state, const int32_t* chrom,
                                 const pert_ccc_params* p, int8_t* scratch, double* score1, double* score2,
                                 double* lrs, double* madn, int32_t* breakpoints, int32_t* flags,
                                 hipStream_t stream) {
  if (L < 2 || N < 1 || !x || !first1 || !first2 || !u || !p || !scratch || !score1 || !score2 || !lrs || !madn ||
      !breakpoints || !flags)
    return PERT_E_ARG;
  if ((state == nullptr) != (chrom == nullptr)) return PERT_E_ARG;
  if (p->lloyd_max_iter < 1 || p->em_max_iter < 1) return PERT_E_ARG;
  hipLaunchKernelGGL(ccc_features_kernel, dim3(N), dim3(gmm2::kT), 0, stream, L, N, x, first2, u, state, chrom, *p,
                     scratch, score1, score2, lrs, madn, breakpoints, flags);
  return gmm2::launch_status();
}
