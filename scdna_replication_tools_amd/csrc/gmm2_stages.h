// gmm2_stages.h -- the stages tau_kernels.hip, bin_kernels.hip and ccc_kernels.hip share: sklearn's
// GaussianMixture(n_components=2) on one 1-D profile per 256-thread workgroup, from the caller's draws
// (k-means++ for two centres, EM from the k-means labels, the mixture's per-point log
// probabilities), the two binary levels (the GMM means, or np.percentile order statistics chosen
// by the skew), and the fixed-order block reductions, prefix scan and radix select under them.
//
// Every stage is in fp64 and every sum a fixed-order block sum, so reruns are bit-identical; the
// decisions are sklearn's / numpy's, and each reports whether it sat within the caller's rounding
// margin (the caller routes such a cell to its exact host path).  Each kernel keeps what differs
// in substance: its prologue and what it does with the fit (a threshold scan, or
// ccc_kernels.hip's scores); tau_kernels.hip also its own Cell, assign2 and lloyd, while the two
// fp64 row kernels share those of namespace f64 below.  The stage functions are plain __device__
// templates: every one has a single call site per kernel and is inlined there.
//
// Cell: c.L bins, c.X(i) the profile the mixture is fitted to, c.Xc(i) the centred profile
// k-means runs on.  Params: pert_tau_params, pert_bin_params or a kernel's per-cell view (the
// fields used here carry the same names in all).  sm: LDS of at least the widest block sum's
// NV * kTW doubles.

#pragma once

#include "../../include/pert_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gmm2 {

constexpr int kT = 256;                 // threads per workgroup
constexpr int kTW = kT / 64;            // waves per workgroup
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

// Inclusive prefix sums of one 256-element chunk: returns this thread's cumulative value
// (carry + the chunk's elements up to and including this thread's), *total the carry plus
// the whole chunk -- both sums in one fixed order.
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

// Order statistics rank[0..3] (0-based) of c.X by 8-bit radix select, MSB first (8 passes, one
// 256-bin integer histogram per target in LDS: deterministic).  hist: 4 * 256 words.
template <class Cell>
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

// k-means++ for 2 centres on c.Xc (sklearn _kmeans_plusplus; tau_init._kmeans_pp): the first
// centre from the data-free RandomState(0) draw p.first, two local trials at p.u * potential on
// the cumulative sum, the trial of least potential (first on a tie) becomes the second centre.
// cand: the two trials' indices.  Returns whether a draw or the choice between the trials sat
// within p.pp_margin (relative to the potential) of a rounding boundary.  sval: 2 doubles of LDS.
template <class Cell, class Params>
__device__ bool kmeans_pp2(const Cell& c, const Params& p, double* cen0_out, double* cen1_out, int (&cand)[2],
                           double* sm, int* smi, double* sval) {
  const int L = c.L;
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
  cand[0] = cand[1] = -1;
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
  *cen0_out = cen0;
  *cen1_out = pots[1] < pots[0] ? xc[1] : xc[0];                       // first minimum
  bool frag = false;
  for (int t = 0; t < 2; ++t) {
    if (fabs(cum_at[t] - rv[t]) <= p.pp_margin * pot) frag = true;
    if (cand[t] > 0 && fabs(cum_prev[t] - rv[t]) <= p.pp_margin * pot) frag = true;
  }
  if (xc[0] != xc[1] && fabs(pots[0] - pots[1]) <= p.pp_margin * fmax(fabs(pots[0]), fabs(pots[1]))) frag = true;
  return frag;
}

// The 2-component 1-D mixture: weights, means, variances (reg_covar included), sklearn's
// component order.
struct Mix {
  double w0, w1, mu0, mu1, var0, var1;
};

// The per-point weighted log probabilities of a Mix (sklearn _estimate_weighted_log_prob) and,
// from them, the point's log probability and responsibilities (_estimate_log_prob_resp).
struct LogProb {
  double mu0, mu1, pr0, pr1, lp0, lp1, lw0, lw1;
  __device__ __forceinline__ explicit LogProb(const Mix& g)
      : mu0(g.mu0), mu1(g.mu1), pr0(1.0 / sqrt(g.var0)), pr1(1.0 / sqrt(g.var1)), lp0(log(pr0)), lp1(log(pr1)),
        lw0(log(g.w0)), lw1(log(g.w1)) {}
  __device__ __forceinline__ void weighted(double X, double* l0, double* l1) const {
    const double y0 = (X - mu0) * pr0, y1 = (X - mu1) * pr1;
    *l0 = (-0.5 * (kLog2Pi + y0 * y0) + lp0) + lw0;
    *l1 = (-0.5 * (kLog2Pi + y1 * y1) + lp1) + lw1;
  }
  __device__ __forceinline__ void resp(double X, double* lpn, double* r0, double* r1) const {
    double l0, l1;
    weighted(X, &l0, &l1);
    const double m = fmax(l0, l1);
    *lpn = m + log(exp(l0 - m) + exp(l1 - m));
    *r0 = exp(l0 - *lpn);
    *r1 = exp(l1 - *lpn);
  }
};

// EM of the mixture on c.X from the k-means labels lab (tau_init._gmm_fit; sklearn fit_predict:
// the M step of the one-hot labels, then at most em_max_iter iterations until |lower-bound
// change| < em_tol).  k supplies em_tol(), em_margin() and reg_covar() from wherever the kernel
// keeps them (its parameter struct, or LDS).  Sets `bit` in *flag when a stopping test was within
// em_margin of em_tol -- in the caller's own flag word: a separate boolean carried through the
// loop costs the RT kernel a dozen scalar registers.
template <class Cell, class Consts, class Flag>
__device__ void em2(const Cell& c, const int8_t* lab, int em_max_iter, const Consts& k, Mix* out, Flag* flag,
                    Flag bit, double* sm) {
  const int L = c.L;
  const double invL = 1.0 / (double)L;
  const double reg_covar = k.reg_covar();
  Mix g;
  {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double r1 = (double)lab[i], r0 = 1.0 - r1;
      a[0] += r0;
      a[1] += r1;
      a[2] += r0 * X;
      a[3] += r1 * X;
    }
    block_sums<4>(a, sm);
    const double nk0 = a[0] + kEps10, nk1 = a[1] + kEps10;
    g.mu0 = a[2] / nk0;
    g.mu1 = a[3] / nk1;
    double q[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      const double r1 = (double)lab[i], r0 = 1.0 - r1;
      q[0] += r0 * (X - g.mu0) * (X - g.mu0);
      q[1] += r1 * (X - g.mu1) * (X - g.mu1);
    }
    block_sums<2>(q, sm);
    g.var0 = q[0] / nk0 + reg_covar;
    g.var1 = q[1] / nk1 + reg_covar;
    g.w0 = nk0 * invL;
    g.w1 = nk1 * invL;
    const double ws = g.w0 + g.w1;
    g.w0 /= ws;
    g.w1 /= ws;
  }
  double lb = -INFINITY;
  for (int it = 0; it < em_max_iter; ++it) {
    const LogProb e(g);
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double X = c.X(i);
      double lpn, r0, r1;
      e.resp(X, &lpn, &r0, &r1);
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
      double lpn, r0, r1;
      e.resp(X, &lpn, &r0, &r1);
      q[0] += r0 * (X - m0) * (X - m0);
      q[1] += r1 * (X - m1) * (X - m1);
    }
    block_sums<2>(q, sm);
    double nw0 = nk0 * invL, nw1 = nk1 * invL;
    const double ws = nw0 + nw1;
    g.w0 = nw0 / ws;
    g.w1 = nw1 / ws;
    g.mu0 = m0;
    g.mu1 = m1;
    g.var0 = q[0] / nk0 + reg_covar;
    g.var1 = q[1] / nk1 + reg_covar;
    const double lb2 = a[4] * invL;
    const double change = lb2 - lb;
    lb = lb2;
    if (fabs(fabs(change) - k.em_tol()) <= k.em_margin()) *flag |= bit;
    if (fabs(change) < k.em_tol()) break;
  }
  *out = g;
}

// LDS of levels2's radix select.
struct SelectLds {
  uint32_t hist[4 * 256];
  uint64_t pref[4];
  long long k[4];
};

// The mean-gap / skew thresholds of the levels with the caller's slacks (absolute): a test
// within its slack of its threshold makes the levels fragile.
struct LevelTests {
  double mean_gap, gap_slack, early_skew, late_skew, skew_slack;
};

// The two binary levels b0 <= b1 (pert_model.py:377-400, binarize_rt_profiles.py:59-85;
// tau_init._levels_scan): the GMM means, or, when they are closer than mean_gap, np.percentile
// 'linear' (50, 95) / (5, 50) / (25, 75) of c.X chosen by the biased skew of c.Xc, at the
// positions p.q_lo / p.q_hi / p.q_t.  Returns whether a test sat within its slack.
template <class Cell, class Params>
__device__ bool levels2(const Cell& c, const Params& p, double mu0, double mu1, const LevelTests& t, double* b0,
                        double* b1, double* sm, SelectLds* sel) {
  const int L = c.L;
  *b0 = fmin(mu0, mu1);
  *b1 = fmax(mu0, mu1);
  const double gap = fabs(mu0 - mu1);
  bool fragile = fabs(gap - t.mean_gap) <= t.gap_slack;
  if (gap < t.mean_gap) {
    double m[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < L; i += kT) {
      const double xc = c.Xc(i);
      m[0] += xc * xc;
      m[1] += xc * xc * xc;
    }
    block_sums<2>(m, sm);
    const double m2 = m[0] / (double)L, m3 = m[1] / (double)L;
    const double sk = m3 / pow(m2, 1.5);
    if (fabs(sk - t.early_skew) <= t.skew_slack || fabs(sk - t.late_skew) <= t.skew_slack) fragile = true;
    const bool early = sk > t.early_skew, late = !early && sk < t.late_skew;
    const int qa = early ? 2 : (late ? 0 : 1), qb = early ? 4 : (late ? 2 : 3);   // (50, 95) / (5, 50) / (25, 75)
    const int rank[4] = {p.q_lo[qa], p.q_hi[qa], p.q_lo[qb], p.q_hi[qb]};
    double v[4];
    select4(c, rank, v, sel->hist, sel->pref, sel->k);
    // np.percentile 'linear' with numpy's two-sided lerp (tau_init._percentiles)
    const double ta = p.q_t[qa], tb = p.q_t[qb];
    const double da = v[1] - v[0], dbq = v[3] - v[2];
    *b0 = ta >= 0.5 ? v[1] - da * (1.0 - ta) : v[0] + da * ta;
    *b1 = tb >= 0.5 ? v[3] - dbq * (1.0 - tb) : v[2] + dbq * tb;
  }
  return fragile;
}

// The argument check of both entry points: first centre, iteration counts, percentile ranks.
template <class Params>
inline bool params_ok(int L, const Params& p) {
  if (p.first < 0 || p.first >= L || p.lloyd_max_iter < 1 || p.em_max_iter < 1) return false;
  for (int j = 0; j < 5; ++j)
    if (p.q_lo[j] < 0 || p.q_lo[j] >= L || p.q_hi[j] < 0 || p.q_hi[j] >= L) return false;
  return true;
}

// The fp64 row kernels' (bin_kernels.hip, ccc_kernels.hip) Cell, label rule and Lloyd.  In a
// namespace of their own: tau_kernels.hip keeps a Cell / assign2 / lloyd of the same names on its
// standardised fp32 reads.
namespace f64 {

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
// of an iteration within tie_margin of the assignment boundary.  Params: pert_bin_params or
// pert_ccc_params (lloyd_max_iter, tie_margin, lloyd_margin).
template <class Params>
__device__ void lloyd(const Cell& c, double c0, double c1, double tol, double sumXc, const Params& p,
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

}  // namespace f64

// The status of the launch just made.
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

}  // namespace gmm2
