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
// with the margins of an fp64-vs-fp64 comparison, all passed in pert_bin_params.  The block-sum,
// prefix-scan and radix-select helpers are tau_kernels.hip's, restated here so that kernel and
// its instantiation stay as they are.  The scan sums each threshold's distance directly (10
// thresholds per pass over the profile): the tau kernel's 2^-32 fixed-point histogram is too
// coarse for a distance table compared at rounding level.

#include "../../include/pert_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kT = 256;                 // threads per workgroup
constexpr int kTW = kT / 64;            // waves per workgroup
constexpr int kNT = PERT_BIN_THRESHOLDS;
constexpr int kTG = 10;                 // thresholds per scan pass
enum { kEmTol, kRegCovar, kMeanGap, kEarly, kLate, kEmMargin, kGapMargin, kSkewMargin, kRespMargin, kThreshMargin,
       kDistMargin, kNPar };   // slots of the kernel's LDS copy of the late-stage parameters
constexpr double kLog2Pi = 1.8378770664093454836;
constexpr double kEps10 = 10.0 * 2.220446049250313e-16;   // 10 * finfo(float64).eps

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Fixed-order block sums of NV values; every thread receives the sums.
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], double* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();                      // earlier readers of sm are done
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sm[k * kTW + w] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double t = 0.0;
#pragma unroll
    for (int ww = 0; ww < kTW; ++ww) t += sm[k * kTW + ww];
    v[k] = t;
  }
}

__device__ __forceinline__ int block_min_i(int v, int* smi) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if (lane == 0) smi[w] = v;
  __syncthreads();
  int t = smi[0];
#pragma unroll
  for (int ww = 1; ww < kTW; ++ww) t = min(t, smi[ww]);
  return t;
}

struct Cell {
  const double* x;     // the cell's profile, [L]
  int L;
  double mX;           // its mean (KMeans centres its data first)
  __device__ __forceinline__ double X(int i) const { return x[i]; }
  __device__ __forceinline__ double Xc(int i) const { return x[i] - mX; }
};

// sklearn's label rule for 2 centres: centre 1 where ||c1||^2 - 2 x c1 < ||c0||^2 - 2 x c0.
// *near: the two sides are within `tie` of each other, relative to their magnitude.
__device__ __forceinline__ int assign2(double X, double c0, double c1, double tie, bool* near) {
  const double d1 = c1 * c1 - 2.0 * X * c1;
  const double d0 = c0 * c0 - 2.0 * X * c0;
  const double scale = c0 * c0 + c1 * c1 + 2.0 * fabs(X) * (fabs(c0) + fabs(c1));
  *near = fabs(d1 - d0) <= tie * scale;
  return d1 < d0 ? 1 : 0;
}

// Lloyd's k-means for 2 centres (sklearn _kmeans_single_lloyd: at most max_iter iterations, stop
// on unchanged labels or a centre shift <= tol, then the final re-assignment).  lab_old: scratch
// row; out: the final labels.  *fragile: the shift test within lloyd_margin of tol, or a point
// of an iteration within tie_margin of the assignment boundary.
__device__ void lloyd(const Cell& c, double c0, double c1, double tol, double sumXc, const pert_bin_params& p,
                      int8_t* lab_old, int8_t* out, bool* fragile, double* sm) {
  const int L = c.L;
  for (int i = threadIdx.x; i < L; i += kT) lab_old[i] = -1;
  bool strict = false;
  for (int it = 0; it < p.lloyd_max_iter; ++it) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};       // w1, s1, changed labels, points on the boundary
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.Xc(i);
      bool near;
      const int l = assign2(X, c0, c1, p.tie_margin, &near);
      acc[0] += (double)l;
      acc[1] += l ? X : 0.0;
      acc[2] += (l != lab_old[i]) ? 1.0 : 0.0;
      acc[3] += near ? 1.0 : 0.0;
      lab_old[i] = (int8_t)l;
    }
    block_sums<4>(acc, sm);
    const double w1 = acc[0], w0 = (double)L - w1;
    const double s1 = acc[1], s0 = sumXc - s1;
    const double n0 = w0 > 0.0 ? s0 / fmax(w0, 1.0) : c0;
    const double n1 = w1 > 0.0 ? s1 / fmax(w1, 1.0) : c1;
    const double shift = (n0 - c0) * (n0 - c0) + (n1 - c1) * (n1 - c1);
    const bool same = acc[2] == 0.0;
    if (acc[3] > 0.0) *fragile = true;
    if (!same && fabs(shift - tol) <= p.lloyd_margin * tol) *fragile = true;
    c0 = n0;
    c1 = n1;
    if (same) {
      strict = true;
      break;
    }
    if (shift <= tol) break;
  }
  double nr[1] = {0.0};
  for (int i = threadIdx.x; i < L; i += kT) {
    bool near = false;
    out[i] = strict ? lab_old[i] : (int8_t)assign2(c.Xc(i), c0, c1, p.tie_margin, &near);
    nr[0] += near ? 1.0 : 0.0;
  }
  block_sums<1>(nr, sm);
  if (nr[0] > 0.0) *fragile = true;
}

// Inclusive prefix sums of one 256-element chunk: this thread's cumulative value (carry + the
// chunk's elements up to and including this thread's); *total the carry plus the whole chunk.
__device__ __forceinline__ double chunk_scan(double v, double carry, double* total, double* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  __syncthreads();
  if (lane == 63) sm[w] = v;
  __syncthreads();
  double pre = carry;
  for (int ww = 0; ww < w; ++ww) pre += sm[ww];
  double tot = carry;
#pragma unroll
  for (int ww = 0; ww < kTW; ++ww) tot += sm[ww];
  *total = tot;
  return pre + v;
}

// Order-preserving map of a double onto uint64 (radix select) and back.
__device__ __forceinline__ uint64_t okey(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ikey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// Order statistics rank[0..3] (0-based) of the profile by 8-bit radix select, MSB first (8
// passes, one 256-bin integer histogram per target in LDS: deterministic).
__device__ void select4(const Cell& c, const int (&rank)[4], double (&out)[4], uint32_t* hist, uint64_t* s_pref,
                        long long* s_k) {
  const int L = c.L;
  if (threadIdx.x < 4) {
    s_pref[threadIdx.x] = 0;
    s_k[threadIdx.x] = rank[threadIdx.x];
  }
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    for (int i = threadIdx.x; i < 4 * 256; i += kT) hist[i] = 0;
    __syncthreads();
    uint64_t pref[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pref[j] = s_pref[j];
    for (int i = threadIdx.x; i < L; i += kT) {
      const uint64_t key = okey(c.X(i));
      const uint32_t dig = (uint32_t)(key >> shift) & 255u;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (pass == 0 || (key >> (shift + 8)) == (pref[j] >> (shift + 8))) atomicAdd(&hist[j * 256 + dig], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      const int j = threadIdx.x;
      long long cum = 0;
      for (int d = 0; d < 256; ++d) {
        const long long h = hist[j * 256 + d];
        if (cum + h > s_k[j]) {
          s_pref[j] = pref[j] | ((uint64_t)d << shift);
          s_k[j] -= cum;
          break;
        }
        cum += h;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = ikey(s_pref[j]);
}

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
  __shared__ uint32_t s_hist[4 * 256];
  __shared__ uint64_t s_pref[4];
  __shared__ long long s_k[4];
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
  const double invL = 1.0 / (double)L;
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

  // ---- k-means++ for 2 centres: first centre from the data-free RandomState(0) draw, two local
  // trials at u * potential on the cumulative sum
  const int first = min(max(p.first, 0), L - 1);
  const double cen0 = c.Xc(first);
  double pot;
  {
    double a[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double d = c.Xc(i) - cen0;
      a[0] += d * d;
    }
    block_sums<1>(a, sm);
    pot = a[0];
  }
  const double rv[2] = {p.u[0] * pot, p.u[1] * pot};
  int cand[2] = {-1, -1};
  double cum_at[2] = {0.0, 0.0}, cum_prev[2] = {0.0, 0.0};
  {
    double carry = 0.0;
    for (int base = 0; base < L && (cand[0] < 0 || cand[1] < 0); base += kT) {
      const int i = base + threadIdx.x;
      double v = 0.0;
      if (i < L) {
        const double d = c.Xc(i) - cen0;
        v = d * d;
      }
      double total;
      const double cum = chunk_scan(v, carry, &total, sm);
      const bool last = base + kT >= L;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (cand[t] >= 0) continue;                                   // uniform
        const int hit = block_min_i((i < L && cum >= rv[t]) ? i : 0x7fffffff, smi);
        if (hit == 0x7fffffff && !last) continue;                     // uniform
        const int ci = hit != 0x7fffffff ? hit : L - 1;               // searchsorted, clamped
        __syncthreads();
        if (i == ci) sval[0] = cum;
        if (i == ci - 1) sval[1] = cum;
        __syncthreads();
        cand[t] = ci;
        cum_at[t] = sval[0];
        cum_prev[t] = ci == base ? carry : sval[1];
      }
      carry = total;
    }
  }
  const double xc[2] = {c.Xc(cand[0]), c.Xc(cand[1])};
  double pots[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < L; i += kT) {
    const double X = c.Xc(i);
    const double d0 = (X - cen0) * (X - cen0);
    pots[0] += fmin(d0, (X - xc[0]) * (X - xc[0]));
    pots[1] += fmin(d0, (X - xc[1]) * (X - xc[1]));
  }
  block_sums<2>(pots, sm);
  const double cen1 = pots[1] < pots[0] ? xc[1] : xc[0];               // first minimum
  int flag = 0;
  for (int t = 0; t < 2; ++t) {
    if (fabs(cum_at[t] - rv[t]) <= p.pp_margin * pot) flag |= PERT_BIN_F_PP;
    if (cand[t] > 0 && fabs(cum_prev[t] - rv[t]) <= p.pp_margin * pot) flag |= PERT_BIN_F_PP;
  }
  if (xc[0] != xc[1] && fabs(pots[0] - pots[1]) <= p.pp_margin * fmax(fabs(pots[0]), fabs(pots[1])))
    flag |= PERT_BIN_F_PP;

  {
    bool fr = false;
    lloyd(c, cen0, cen1, tol, sumXc, p, lab_old, lab1, &fr, sm);
    if (fr) flag |= PERT_BIN_F_LLOYD;
  }

  // ---- EM of the 2-component 1-D mixture from the k-means labels (sklearn fit_predict: at most
  // em_max_iter iterations, |lower-bound change| < em_tol)
  double w0, w1, mu0, mu1, var0, var1;
  const double reg_covar = s_par[kRegCovar];
  {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double r1 = (double)lab1[i], r0 = 1.0 - r1;
      a[0] += r0;
      a[1] += r1;
      a[2] += r0 * X;
      a[3] += r1 * X;
    }
    block_sums<4>(a, sm);
    const double nk0 = a[0] + kEps10, nk1 = a[1] + kEps10;
    mu0 = a[2] / nk0;
    mu1 = a[3] / nk1;
    double q[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double r1 = (double)lab1[i], r0 = 1.0 - r1;
      q[0] += r0 * (X - mu0) * (X - mu0);
      q[1] += r1 * (X - mu1) * (X - mu1);
    }
    block_sums<2>(q, sm);
    var0 = q[0] / nk0 + reg_covar;
    var1 = q[1] / nk1 + reg_covar;
    w0 = nk0 * invL;
    w1 = nk1 * invL;
    const double ws = w0 + w1;
    w0 /= ws;
    w1 /= ws;
  }
  double lb = -INFINITY;
  for (int it = 0; it < p.em_max_iter; ++it) {
    const double pr0 = 1.0 / sqrt(var0), pr1 = 1.0 / sqrt(var1);
    const double lp0 = log(pr0), lp1 = log(pr1), lw0 = log(w0), lw1 = log(w1);
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double y0 = (X - mu0) * pr0, y1 = (X - mu1) * pr1;
      const double l0 = (-0.5 * (kLog2Pi + y0 * y0) + lp0) + lw0, l1 = (-0.5 * (kLog2Pi + y1 * y1) + lp1) + lw1;
      const double m = fmax(l0, l1);
      const double lpn = m + log(exp(l0 - m) + exp(l1 - m));
      const double r0 = exp(l0 - lpn), r1 = exp(l1 - lpn);
      a[0] += r0;
      a[1] += r1;
      a[2] += r0 * X;
      a[3] += r1 * X;
      a[4] += lpn;
    }
    block_sums<5>(a, sm);
    const double nk0 = a[0] + kEps10, nk1 = a[1] + kEps10;
    const double m0 = a[2] / nk0, m1 = a[3] / nk1;
    double q[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double y0 = (X - mu0) * pr0, y1 = (X - mu1) * pr1;
      const double l0 = (-0.5 * (kLog2Pi + y0 * y0) + lp0) + lw0, l1 = (-0.5 * (kLog2Pi + y1 * y1) + lp1) + lw1;
      const double m = fmax(l0, l1);
      const double lpn = m + log(exp(l0 - m) + exp(l1 - m));
      const double r0 = exp(l0 - lpn), r1 = exp(l1 - lpn);
      q[0] += r0 * (X - m0) * (X - m0);
      q[1] += r1 * (X - m1) * (X - m1);
    }
    block_sums<2>(q, sm);
    double nw0 = nk0 * invL, nw1 = nk1 * invL;
    const double ws = nw0 + nw1;
    w0 = nw0 / ws;
    w1 = nw1 / ws;
    mu0 = m0;
    mu1 = m1;
    var0 = q[0] / nk0 + reg_covar;
    var1 = q[1] / nk1 + reg_covar;
    const double lb2 = a[4] * invL;
    const double change = lb2 - lb;
    lb = lb2;
    if (fabs(fabs(change) - s_par[kEmTol]) <= s_par[kEmMargin]) flag |= PERT_BIN_F_EM;
    if (fabs(change) < s_par[kEmTol]) break;
  }

  // ---- fit_predict's final E step with the fitted parameters: gmm_state = argmax (first on a tie)
  {
    const double pr0 = 1.0 / sqrt(var0), pr1 = 1.0 / sqrt(var1);
    const double lp0 = log(pr0), lp1 = log(pr1), lw0 = log(w0), lw1 = log(w1);
    const double resp_margin = s_par[kRespMargin];
    double nr[1] = {0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double y0 = (X - mu0) * pr0, y1 = (X - mu1) * pr1;
      const double l0 = (-0.5 * (kLog2Pi + y0 * y0) + lp0) + lw0, l1 = (-0.5 * (kLog2Pi + y1 * y1) + lp1) + lw1;
      lab1[i] = l1 > l0 ? 1 : 0;
      nr[0] += (fabs(l1 - l0) <= resp_margin * (1.0 + fabs(l0) + fabs(l1))) ? 1.0 : 0.0;
    }
    block_sums<1>(nr, sm);
    if (nr[0] > 0.0) flag |= PERT_BIN_F_RESP;
  }

  // ---- levels (binarize_rt_profiles.py:59-85): the GMM means, or percentiles of the profile
  // chosen by its biased skew when the means are closer than MEAN_GAP_THRESH
  double b0 = fmin(mu0, mu1), b1 = fmax(mu0, mu1);
  const double gap = fabs(mu0 - mu1);
  if (fabs(gap - s_par[kMeanGap]) <= s_par[kGapMargin] * fmax(1.0, fabs(mu0) + fabs(mu1))) flag |= PERT_BIN_F_LEVELS;
  if (gap < s_par[kMeanGap]) {
    double m[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double d = c.Xc(i);
      m[0] += d * d;
      m[1] += d * d * d;
    }
    block_sums<2>(m, sm);
    const double m2 = m[0] / (double)L, m3 = m[1] / (double)L;
    const double sk = m3 / pow(m2, 1.5);
    const double early_skew = s_par[kEarly], late_skew = s_par[kLate];
    if (fabs(sk - early_skew) <= s_par[kSkewMargin] || fabs(sk - late_skew) <= s_par[kSkewMargin]) flag |= PERT_BIN_F_LEVELS;
    const bool early = sk > early_skew, late = !early && sk < late_skew;
    const int qa = early ? 2 : (late ? 0 : 1), qb = early ? 4 : (late ? 2 : 3);   // (50, 95) / (5, 50) / (25, 75)
    const int rank[4] = {p.q_lo[qa], p.q_hi[qa], p.q_lo[qb], p.q_hi[qb]};
    double v[4];
    select4(c, rank, v, s_hist, s_pref, s_k);
    // np.percentile 'linear' with numpy's two-sided lerp
    const double ta = p.q_t[qa], tb = p.q_t[qb];
    const double da = v[1] - v[0], dbq = v[3] - v[2];
    b0 = ta >= 0.5 ? v[1] - da * (1.0 - ta) : v[0] + da * ta;
    b1 = tb >= 0.5 ? v[3] - dbq * (1.0 - tb) : v[2] + dbq * tb;
  }

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
    covs[2 * n] = var0;
    covs[2 * n + 1] = var1;
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
  if (p->first < 0 || p->first >= L || p->lloyd_max_iter < 1 || p->em_max_iter < 1) return PERT_E_ARG;
  for (int j = 0; j < 5; ++j)
    if (p->q_lo[j] < 0 || p->q_lo[j] >= L || p->q_hi[j] < 0 || p->q_hi[j] >= L) return PERT_E_ARG;
  hipLaunchKernelGGL(rt_binarize_kernel, dim3(N), dim3(kT), 0, stream, L, N, x, *p, means, covs, gmm_state, rt_state,
                     dist, best, n_rep, flags);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}
