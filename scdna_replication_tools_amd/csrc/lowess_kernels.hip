// lowess_kernels.hip -- gfx950 kernels of the bulk G1 GC correction's LOWESS curve (gc_correction.py).
//
// Reference: bulk_gc_correction.py:60-72, statsmodels' lowess(rpm, gc, xvals=unique gc) over every
// (G1/2 cell, bin) point of a library, frac = 2/3, it = 3, delta = 0.  GC is a property of the bin:
// x takes U <= L distinct values, each repeated once per cell, and the tricube weight depends on x
// alone, so a fit needs two sums per distinct x, S0 = sum delta and S1 = sum delta y (delta the
// robustness weights).  A robustness round is
//   sums     one streaming pass over y (C, L): delta recomputed from fit[inv[l]] and the median m,
//            per-bin partial sums of fixed 32-cell chunks, added in chunk order, then per distinct
//            x in bin order;
//   regress  a U x U local regression, one workgroup per fit point: the k-th neighbour distance
//            over the weighted multiset (counts per x), then the three fixed-order block sums;
//   absmed   the exact median of |y - fit[inv]|: a radix select on the uint64 pattern of the
//            non-negative doubles, 11 bits a pass (6 passes), LDS histograms, one integer atomic
//            per non-empty bucket per workgroup; both middle order statistics.
// Everything is fp64; no floating-point atomics; every floating-point sum has one fixed order, so
// reruns are bit-identical.  pert_lowess_curve queues every round and the final evaluation on the
// caller's stream; nothing comes back to the host in between.

#include "gmm2_stages.h"

namespace {

using gmm2::block_sums;
using gmm2::chunk_scan;
using gmm2::kT;
using gmm2::kTW;
using gmm2::wave_sum;

constexpr int kChunk = 32;                 // cells per partial sum of the sums pass (fixed: part of the result)
constexpr int kBuckets = 2048;             // 11-bit digits
constexpr int kPasses = 6;
constexpr int kHistWords = 2 * kBuckets + 4;   // the two histograms, and the word that records a NaN residual
constexpr int kHistBlocks = 1024;          // the histogram passes' grid, about

__host__ __device__ inline int pass_shift(int pass) { return pass < 5 ? 52 - 11 * pass : 0; }
__host__ __device__ inline int pass_width(int pass) { return pass < 5 ? 11 : 8; }

// the select's state between passes
struct SelState {
  unsigned long long pref[2];              // the bits found so far of the two order statistics
  long long krem[2];                       // their ranks among the keys sharing pref
  long long n;                             // the number of finite points
};

__device__ __forceinline__ bool finite64(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// np.median of the two middle order statistics
__device__ __forceinline__ double median_of(const double* med) {
  const double lo = med[0], hi = med[1];
  return lo == hi ? lo : (lo + hi) / 2.0;
}

// ---- the sums: per (chunk of cells, bin) partial sums of delta and delta y
__global__ __launch_bounds__(kT) void lowess_sums_kernel(int C, int L, int first, const double* __restrict__ y,
                                                          const int32_t* __restrict__ inv,
                                                          const double* __restrict__ fit,
                                                          const double* __restrict__ med,
                                                          double* __restrict__ part0, double* __restrict__ part1) {
  const int l = blockIdx.x * kT + threadIdx.x;
  if (l >= L) return;
  const int chunk = blockIdx.y;
  const int c0 = chunk * kChunk, c1 = min(C, c0 + kChunk);
  double f = 0.0, m = 0.0, six = 0.0;
  if (!first) {
    f = fit[inv[l]];
    m = median_of(med);
    six = 6.0 * m;
  }
  double s0 = 0.0, s1 = 0.0;
  for (int c = c0; c < c1; ++c) {
    const double v = y[(size_t)c * (size_t)L + (size_t)l];
    if (!finite64(v)) continue;
    double d = 1.0;
    if (!first) {
      const double r = fabs(v - f);
      const double u = m == 0.0 ? (r > 0.0 ? 1.0 : 0.0) : fmin(r / six, 1.0);
      const double q = 1.0 - u * u;
      d = q * q;
    }
    s0 += d;
    s1 += d * v;
  }
  part0[(size_t)chunk * (size_t)L + (size_t)l] = s0;
  part1[(size_t)chunk * (size_t)L + (size_t)l] = s1;
}

// per bin: the chunks' partial sums in chunk order
__global__ __launch_bounds__(kT) void lowess_bin_kernel(int L, int n_chunks, const double* __restrict__ part0,
                                                         const double* __restrict__ part1, double* __restrict__ b0,
                                                         double* __restrict__ b1) {
  const int l = blockIdx.x * kT + threadIdx.x;
  if (l >= L) return;
  double s0 = 0.0, s1 = 0.0;
  for (int c = 0; c < n_chunks; ++c) {
    s0 += part0[(size_t)c * (size_t)L + (size_t)l];
    s1 += part1[(size_t)c * (size_t)L + (size_t)l];
  }
  b0[l] = s0;
  b1[l] = s1;
}

// per distinct x: one wave adds the bins mapped to it, lane by lane in bin order, then across lanes
__global__ __launch_bounds__(kT) void lowess_group_kernel(int L, int U, const int32_t* __restrict__ inv,
                                                           const double* __restrict__ b0,
                                                           const double* __restrict__ b1, double* __restrict__ S0,
                                                           double* __restrict__ S1) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * kTW + (threadIdx.x >> 6);
  if (u >= U) return;                                     // whole waves leave: no barrier below
  double s0 = 0.0, s1 = 0.0;
  for (int l = lane; l < L; l += 64) {
    if (inv[l] == u) {
      s0 += b0[l];
      s1 += b1[l];
    }
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (lane == 0) {
    S0[u] = s0;
    S1[u] = s1;
  }
}

// P[0] = 0, P[j + 1] = cnt[0] + .. + cnt[j]: the first round's S0 are the points per distinct x
// (sums of ones: whole numbers below 2^53, exact in any order).  One workgroup.
__global__ __launch_bounds__(kT) void lowess_prefix_kernel(int U, const double* __restrict__ cnt,
                                                            double* __restrict__ P) {
  __shared__ double sm[kTW];
  double carry = 0.0;
  if (threadIdx.x == 0) P[0] = 0.0;
  for (int base = 0; base < U; base += kT) {
    const int j = base + threadIdx.x;
    double tot;
    const double c = chunk_scan(j < U ? cnt[j] : 0.0, carry, &tot, sm);
    if (j < U) P[j + 1] = c;
    carry = tot;
    __syncthreads();
  }
}

__device__ __forceinline__ double block_min_d(double v, double* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if (lane == 0) sm[w] = v;
  __syncthreads();
  double t = sm[0];
#pragma unroll
  for (int ww = 1; ww < kTW; ++ww) t = fmin(t, sm[ww]);
  return t;
}

__device__ __forceinline__ double tricube(double d, double h) {
  if (!(d < h)) return 0.0;
  const double t = d / h;
  const double q = 1.0 - t * t * t;
  return q * q * q;
}

// ---- the local regression at x0s[blockIdx.x]
__global__ __launch_bounds__(kT) void lowess_regress_kernel(int U, const double* __restrict__ ux,
                                                             const double* __restrict__ P,
                                                             const double* __restrict__ S0,
                                                             const double* __restrict__ S1,
                                                             const double* __restrict__ x0s, double k,
                                                             double* __restrict__ out) {
  __shared__ double sm[2 * kTW];
  const double x0 = x0s[blockIdx.x];
  // p: the first distinct x not below x0.  |ux[j] - x0| falls (weakly) with j below p and rises from p on.
  int p;
  {
    int lo = 0, hi = U;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ux[mid] < x0) lo = mid + 1; else hi = mid;
    }
    p = lo;
  }
  // h: the least distance d_j with at least k points at distance <= d_j
  double hmin = INFINITY;
  for (int j = threadIdx.x; j < U; j += kT) {
    const double dj = fabs(ux[j] - x0);
    int lo = 0, hi = p;                                   // a: the first index below p with d <= dj
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (fabs(ux[mid] - x0) <= dj) hi = mid; else lo = mid + 1;
    }
    const int a = lo;
    lo = p;
    hi = U;                                               // b: the first index from p on with d > dj
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (fabs(ux[mid] - x0) <= dj) lo = mid + 1; else hi = mid;
    }
    if (P[lo] - P[a] >= k) hmin = fmin(hmin, dj);
  }
  const double h = block_min_d(hmin, sm);

  double W;
  {
    double a[1] = {0.0};
    for (int j = threadIdx.x; j < U; j += kT) a[0] += tricube(fabs(ux[j] - x0), h) * S0[j];
    block_sums<1>(a, sm);
    W = a[0];
  }
  // h = 0, a window of zero (or NaN) weights only, or k beyond the number of points (h = inf)
  if (!(W > 0.0) || h == INFINITY) {
    if (threadIdx.x == 0) out[blockIdx.x] = NAN;
    return;
  }
  double xb;
  {
    double a[1] = {0.0};
    for (int j = threadIdx.x; j < U; j += kT) a[0] += tricube(fabs(ux[j] - x0), h) * S0[j] / W * ux[j];
    block_sums<1>(a, sm);
    xb = a[0];
  }
  double v;
  {
    double a[1] = {0.0};
    for (int j = threadIdx.x; j < U; j += kT) {
      const double e = ux[j] - xb;
      a[0] += tricube(fabs(ux[j] - x0), h) * S0[j] / W * e * e;
    }
    block_sums<1>(a, sm);
    v = a[0];
  }
  {
    const double dx = x0 - xb;
    double a[1] = {0.0};
    for (int j = threadIdx.x; j < U; j += kT) {
      const double t = tricube(fabs(ux[j] - x0), h) / W;
      const double lev = v > 0.0 ? 1.0 + dx * (ux[j] - xb) / v : 1.0;
      a[0] += t * lev * S1[j];
    }
    block_sums<1>(a, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = a[0];
  }
}

// ---- the exact median: one pass of the radix select over |y - fit[inv]|
__global__ __launch_bounds__(kT) void lowess_hist_kernel(int C, int L, int cells_per_block,
                                                          const double* __restrict__ y,
                                                          const int32_t* __restrict__ inv,
                                                          const double* __restrict__ fit,
                                                          const SelState* __restrict__ st, int pass,
                                                          uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[2 * kBuckets];
  for (int i = threadIdx.x; i < 2 * kBuckets; i += kT) h[i] = 0;
  __syncthreads();
  const int shift = pass_shift(pass);
  const int hs = pass == 0 ? 63 : shift + pass_width(pass);   // the sign bit of |.| is 0
  const uint32_t mask = (1u << pass_width(pass)) - 1u;
  const unsigned long long p0 = pass == 0 ? 0ull : st->pref[0] >> hs;
  const unsigned long long p1 = pass == 0 ? 0ull : st->pref[1] >> hs;
  const bool same = p0 == p1;
  const int l = blockIdx.x * kT + threadIdx.x;
  if (l < L) {
    const double f = fit[inv[l]];
    const int c0 = blockIdx.y * cells_per_block, c1 = min(C, c0 + cells_per_block);
    uint32_t cur = 0, run = 0;                            // a run of equal digits is one LDS add
    for (int c = c0; c < c1; ++c) {
      const double v = y[(size_t)c * (size_t)L + (size_t)l];
      if (!finite64(v)) continue;
      const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(v - f));
      // a NaN residual (a NaN fit) makes the median NaN, as np.median does: the word after the
      // histograms records it
      if (pass == 0 && key > 0x7ff0000000000000ull) atomicOr(&ghist[2 * kBuckets], 1u);
      const uint32_t dig = (uint32_t)(key >> shift) & mask;
      const unsigned long long top = key >> hs;
      if (top == p0) {
        if (run != 0 && dig == cur) {
          ++run;
        } else {
          if (run != 0) atomicAdd(&h[cur], run);
          cur = dig;
          run = 1;
        }
      }
      if (!same && top == p1) atomicAdd(&h[kBuckets + dig], 1u);
    }
    if (run != 0) atomicAdd(&h[cur], run);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kBuckets; i += kT) {
    const uint32_t c = h[i];
    if (c != 0) atomicAdd(&ghist[i], c);
  }
}

// One workgroup: the digit of each of the two order statistics from the pass's histogram, which is
// cleared for the next pass.  The last pass writes the two values (NaN without points).
__global__ __launch_bounds__(kT) void lowess_select_kernel(SelState* st, uint32_t* ghist, int pass, double* med,
                                                            long long* n_out) {
  __shared__ unsigned long long sc[kT];
  __shared__ unsigned long long fin[2];
  constexpr int kPer = kBuckets / kT;                    // 8 buckets a thread
  const int shift = pass_shift(pass);
  const bool same = pass == 0 || st->pref[0] == st->pref[1];
  unsigned long long pref[2] = {pass == 0 ? 0ull : st->pref[0], pass == 0 ? 0ull : st->pref[1]};
  long long krem[2] = {pass == 0 ? 0ll : st->krem[0], pass == 0 ? 0ll : st->krem[1]};
  long long n = pass == 0 ? 0ll : st->n;
  __syncthreads();                                        // the state is read before anyone writes it
  for (int j = 0; j < 2; ++j) {
    const uint32_t* g = ghist + ((same || j == 0) ? 0 : kBuckets);
    unsigned long long s = 0;
    for (int i = 0; i < kPer; ++i) s += g[threadIdx.x * kPer + i];
    sc[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < kT; off <<= 1) {             // inclusive scan of the 256 partial counts
      const unsigned long long t = threadIdx.x >= off ? sc[threadIdx.x - off] : 0ull;
      __syncthreads();
      sc[threadIdx.x] += t;
      __syncthreads();
    }
    const unsigned long long incl = sc[threadIdx.x], excl = incl - s;
    if (pass == 0 && j == 0) {
      n = (long long)sc[kT - 1];
      krem[0] = (n - 1) / 2;
      krem[1] = n / 2;
    }
    const long long kk = krem[j];
    if (n > 0 && (long long)excl <= kk && kk < (long long)incl) {
      long long cum = (long long)excl;
      for (int i = 0; i < kPer; ++i) {
        const long long c = g[threadIdx.x * kPer + i];
        if (cum + c > kk) {
          fin[j] = pref[j] | ((unsigned long long)(threadIdx.x * kPer + i) << shift);
          st->pref[j] = fin[j];
          st->krem[j] = kk - cum;
          break;
        }
        cum += c;
      }
    }
    __syncthreads();
  }
  if (pass == 0 && threadIdx.x == 0) st->n = n;
  for (int i = threadIdx.x; i < 2 * kBuckets; i += kT) ghist[i] = 0;
  if (pass == kPasses - 1) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const bool ok = n > 0 && ghist[2 * kBuckets] == 0;  // points, and no NaN residual among them
      med[0] = ok ? __longlong_as_double((long long)fin[0]) : NAN;
      med[1] = ok ? __longlong_as_double((long long)fin[1]) : NAN;
      if (n_out != nullptr) *n_out = n;
      ghist[2 * kBuckets] = 0;
    }
  }
}

// ---- the workspace
struct Workspace {
  int32_t* inv;
  double *ux, *xv, *part0, *part1, *b0, *b1, *S0, *S1, *P, *fit, *med;
  SelState* st;
  uint32_t* hist;
  int64_t bytes;
};

inline int n_chunks_of(int C) { return (C + kChunk - 1) / kChunk; }

inline Workspace carve(void* base, int C, int L, int U, int M) {
  Workspace w;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += (bytes + 15) & ~(size_t)15;
    return q;
  };
  const size_t nc = (size_t)n_chunks_of(C);
  w.inv = (int32_t*)take(sizeof(int32_t) * (size_t)L);
  w.ux = (double*)take(8 * (size_t)U);
  w.xv = (double*)take(8 * (size_t)(M > 0 ? M : 1));
  w.part0 = (double*)take(8 * nc * (size_t)L);
  w.part1 = (double*)take(8 * nc * (size_t)L);
  w.b0 = (double*)take(8 * (size_t)L);
  w.b1 = (double*)take(8 * (size_t)L);
  w.S0 = (double*)take(8 * (size_t)U);
  w.S1 = (double*)take(8 * (size_t)U);
  w.P = (double*)take(8 * ((size_t)U + 1));
  w.fit = (double*)take(8 * (size_t)U);
  w.med = (double*)take(16);
  w.st = (SelState*)take(sizeof(SelState));
  w.hist = (uint32_t*)take(sizeof(uint32_t) * kHistWords);
  w.bytes = (int64_t)(p - (char*)base);
  return w;
}

// C: the sums pass puts the 32-cell chunks on grid.y (at most 65,535)
inline bool shape_ok(int32_t C, int32_t L, int32_t U) {
  return C >= 1 && C <= kChunk * 65535 && L >= 1 && U >= 1 && U <= L &&
         (int64_t)C * (int64_t)L < ((int64_t)1 << 31);
}

inline bool inv_ok(const int32_t* inv, int32_t L, int32_t U) {
  for (int32_t l = 0; l < L; ++l)
    if (inv[l] < 0 || inv[l] >= U) return false;
  return true;
}

#define LW_HIP(call)                                             \
  do {                                                           \
    const hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return PERT_E_HIP_BASE + (int)e_;      \
  } while (0)
#define LW_LAUNCHED()                                            \
  do {                                                           \
    const int s_ = gmm2::launch_status();                        \
    if (s_ != PERT_OK) return s_;                                \
  } while (0)

// the six passes of the select over |y - fit[inv]|, on device arrays; the histogram is zero on
// entry and on exit
int queue_absmed(int C, int L, const double* y, const int32_t* inv, const double* fit, const Workspace& w,
                 double* med, long long* n_out, hipStream_t stream) {
  const int gx = (L + kT - 1) / kT;
  int gy = kHistBlocks / gx;
  gy = gy < 1 ? 1 : (gy > C ? C : gy);
  const int cpb = (C + gy - 1) / gy;
  gy = (C + cpb - 1) / cpb;
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(lowess_hist_kernel, dim3(gx, gy), dim3(kT), 0, stream, C, L, cpb, y, inv, fit, w.st, pass,
                       w.hist);
    LW_LAUNCHED();
    hipLaunchKernelGGL(lowess_select_kernel, dim3(1), dim3(kT), 0, stream, w.st, w.hist, pass, med, n_out);
    LW_LAUNCHED();
  }
  return PERT_OK;
}

// sums of one round into w.S0 / w.S1
int queue_sums(int C, int L, int U, int first, const double* y, const Workspace& w, hipStream_t stream) {
  const int gx = (L + kT - 1) / kT, nc = n_chunks_of(C);
  hipLaunchKernelGGL(lowess_sums_kernel, dim3(gx, nc), dim3(kT), 0, stream, C, L, first, y, w.inv, w.fit, w.med,
                     w.part0, w.part1);
  LW_LAUNCHED();
  hipLaunchKernelGGL(lowess_bin_kernel, dim3(gx), dim3(kT), 0, stream, L, nc, w.part0, w.part1, w.b0, w.b1);
  LW_LAUNCHED();
  hipLaunchKernelGGL(lowess_group_kernel, dim3((U + kTW - 1) / kTW), dim3(kT), 0, stream, L, U, w.inv, w.b0, w.b1,
                     w.S0, w.S1);
  LW_LAUNCHED();
  return PERT_OK;
}

}  // namespace

extern "C" int pert_lowess_workspace(int32_t C, int32_t L, int32_t U, int32_t M, int64_t* bytes) {
  if (!bytes || !shape_ok(C, L, U) || M < 0) return PERT_E_ARG;
  *bytes = carve(nullptr, C, L, U, M).bytes;
  return PERT_OK;
}

extern "C" int pert_lowess_absmed(int32_t C, int32_t L, int32_t U, const double* y, const int32_t* inv,
                                  const double* fit, double* med, int64_t* n_out, void* workspace,
                                  int64_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(C, L, U) || !y || !inv || !fit || !med || !workspace) return PERT_E_ARG;
  if (((uintptr_t)workspace & 15u) != 0) return PERT_E_ARG;
  const Workspace w = carve(workspace, C, L, U, 0);
  if (workspace_bytes < w.bytes) return PERT_E_ARG;
  if (!inv_ok(inv, L, U)) return PERT_E_ARG;
  LW_HIP(hipMemcpyAsync(w.inv, inv, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, stream));
  LW_HIP(hipMemsetAsync(w.hist, 0, sizeof(uint32_t) * kHistWords, stream));
  return queue_absmed(C, L, y, w.inv, fit, w, med, (long long*)n_out, stream);
}

extern "C" int pert_lowess_curve(int32_t C, int32_t L, int32_t U, int32_t M, const double* y, const int32_t* inv,
                                 const double* ux, const double* xv, int64_t k, int32_t it, double* out,
                                 void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(C, L, U) || M < 1 || !y || !inv || !ux || !xv || !out || !workspace) return PERT_E_ARG;
  if (k < 1 || k > (int64_t)C * (int64_t)L || it < 0) return PERT_E_ARG;
  if (((uintptr_t)workspace & 15u) != 0) return PERT_E_ARG;
  const Workspace w = carve(workspace, C, L, U, M);
  if (workspace_bytes < w.bytes) return PERT_E_ARG;
  if (!inv_ok(inv, L, U)) return PERT_E_ARG;
  for (int32_t j = 0; j < U; ++j)
    if (!isfinite(ux[j]) || (j > 0 && !(ux[j] > ux[j - 1]))) return PERT_E_ARG;
  for (int32_t j = 0; j < M; ++j)
    if (!isfinite(xv[j])) return PERT_E_ARG;

  LW_HIP(hipMemcpyAsync(w.inv, inv, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, stream));
  LW_HIP(hipMemcpyAsync(w.ux, ux, 8 * (size_t)U, hipMemcpyHostToDevice, stream));
  LW_HIP(hipMemcpyAsync(w.xv, xv, 8 * (size_t)M, hipMemcpyHostToDevice, stream));
  LW_HIP(hipMemsetAsync(w.hist, 0, sizeof(uint32_t) * kHistWords, stream));
  const double kd = (double)k;
  for (int round = 0; round <= it; ++round) {
    int s = queue_sums(C, L, U, round == 0, y, w, stream);
    if (s != PERT_OK) return s;
    if (round == 0) {
      hipLaunchKernelGGL(lowess_prefix_kernel, dim3(1), dim3(kT), 0, stream, U, w.S0, w.P);
      LW_LAUNCHED();
    }
    hipLaunchKernelGGL(lowess_regress_kernel, dim3(U), dim3(kT), 0, stream, U, w.ux, w.P, w.S0, w.S1, w.ux, kd,
                       w.fit);
    LW_LAUNCHED();
    s = queue_absmed(C, L, y, w.inv, w.fit, w, w.med, nullptr, stream);
    if (s != PERT_OK) return s;
  }
  const int s = queue_sums(C, L, U, 0, y, w, stream);
  if (s != PERT_OK) return s;
  hipLaunchKernelGGL(lowess_regress_kernel, dim3(M), dim3(kT), 0, stream, U, w.ux, w.P, w.S0, w.S1, w.xv, kd, out);
  LW_LAUNCHED();
  return PERT_OK;
}
