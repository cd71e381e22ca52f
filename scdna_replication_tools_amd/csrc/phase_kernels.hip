// phase_kernels.hip -- gfx950 kernels of the per-cell quality features behind the phase calls
// (phase_matrix.py): what predict_cycle_phase.py:54-88 computes per cell from the long table,
// computed from the decode's uint8 [L][ldn] state matrices and the shard's reads in place.
//
// Reference: predict_cycle_phase.py:23-30 (autocorr = mean of acf lags 9..50, breakpoints = number
// of adjacent changes), :33-39 (cell_frac_rep) and :54-88 (the per-cell feature table).
//
// pert_phase_counts.  The replication state is 0 / 1, so its autocorrelation follows from integer
// counts: T = sum x_t, S_k = #{t : x_t = x_{t+k} = 1} and the sums of the first and last k states
// (phase_matrix.py turns them into the exact rational acf).  One lane owns one cell: it packs 64
// consecutive states of its column into a 64-bit word w and keeps the word before it, p; bit j of
// (w << k) | (p >> (64 - k)) is the state k bins before bin j of w, so a word's contribution to S_k
// is one popcount per lag and the 64 counters S_1..S_64 stay in registers.  The bins are split into
// chunks of whole words (grid y); a chunk owns the pairs whose LATER bin it holds and reads the one
// word before its first as the halo.  Integer adds only (register sums, then one global integer
// atomic per counter and chunk): chunk order is irrelevant, and runs repeat bit for bit.
//
// pert_phase_acf.  The read depth is a float series: two passes in fp64.  Pass 1 sums each cell
// over each chunk (sequentially, four interleaved partial sums), pass 2 forms the mean from the
// chunk sums in chunk order and accumulates c_k = sum (x_t - m)(x_{t+k} - m) for k = 0..max_lag
// over the pairs whose later bin the chunk holds; a last kernel adds the chunks' partials in chunk
// order.  No floating-point atomics: two runs agree bit for bit.  A lane owns a cell (coalesced
// rows); the last 64 centred values of its cell sit in an LDS ring [slot][lane] (consecutive lanes
// = consecutive 8-byte words: conflict free), the max_lag + 1 accumulators in registers.  Four
// bins are processed per ring sweep, so one ring read feeds four multiply-adds.
//
// Both: columns n >= N are never read.  Lanes are independent, so a NaN stays in its cell.

#include "../../include/pert_hip.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kLanes = 64;              // cells per workgroup: one wave, no barriers
constexpr int kWord = 64;               // bins per packed word = slots of the acf ring
constexpr int kMinChunkWords = 2;       // a chunk holds at least two words (128 bins)
constexpr int kTargetWaves = 1024;      // chunks are cut so that about this many waves exist
constexpr int kStep = 4;                // bins per ring sweep of the acf kernel
static_assert(PERT_PHASE_MAX_LAG == kWord, "the halo is one word; the ring holds one word");
static_assert((kMinChunkWords * kWord) % kStep == 0, "chunks start on a sweep boundary");

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Bins per chunk: whole words, at least kMinChunkWords, long enough that the grid has about
// kTargetWaves waves (`groups` = 64-cell groups x planes).
inline int chunk_bins(int L, int64_t groups) {
  const int words = ceil_div(L, kWord);
  const int max_chunks = (int)std::max<int64_t>(1, kTargetWaves / std::max<int64_t>(groups, 1));
  return kWord * std::max(kMinChunkWords, ceil_div(words, max_chunks));
}

// Bit j = (col[(b + j) * ldn] != 0) for j < cnt (cnt <= 64), higher bits 0.
__device__ __forceinline__ uint64_t load_word(const uint8_t* __restrict__ col, int ldn, int b, int cnt) {
  uint64_t w = 0;
  if (cnt >= kWord) {
#pragma unroll
    for (int j = 0; j < kWord; ++j) w |= (uint64_t)(col[(size_t)(b + j) * ldn] != 0) << j;
  } else {
    for (int j = 0; j < cnt; ++j) w |= (uint64_t)(col[(size_t)(b + j) * ldn] != 0) << j;
  }
  return w;
}

// Grid (64-cell groups, chunks, planes), one wave per workgroup.
template <bool HAS_CN>
__global__ __launch_bounds__(kLanes) void phase_counts_kernel(
    int L, int N, int ldn, int64_t plane_stride, const uint8_t* __restrict__ rep, const uint8_t* __restrict__ cn,
    int max_lag, int chunk, uint32_t* __restrict__ rep_sum, uint32_t* __restrict__ rep_bk,
    uint32_t* __restrict__ cn_bk, uint32_t* __restrict__ cn0, uint32_t* __restrict__ rep_lag,
    uint32_t* __restrict__ rep_head, uint32_t* __restrict__ rep_tail) {
  const int n = blockIdx.x * kLanes + threadIdx.x;
  if (n >= N) return;
  const size_t plane = blockIdx.z;
  const uint8_t* col = rep + plane * (size_t)plane_stride + n;
  const int t0 = blockIdx.y * chunk, t1 = min(L, t0 + chunk);

  uint32_t s[kWord];
#pragma unroll
  for (int k = 0; k < kWord; ++k) s[k] = 0u;
  uint32_t total = 0u, bk = 0u;
  uint64_t p = t0 > 0 ? load_word(col, ldn, t0 - kWord, kWord) : 0ull;    // the halo: bins [t0 - 64, t0)
  uint64_t first = 0ull;
  for (int b = t0; b < t1; b += kWord) {
    const int cnt = min(kWord, L - b);
    const uint64_t w = load_word(col, ldn, b, cnt);
    if (b == 0) first = w;
    total += (uint32_t)__popcll(w);
    uint64_t pairs = cnt >= kWord ? ~0ull : (1ull << cnt) - 1ull;          // bins of this word that exist
    if (b == 0) pairs &= ~1ull;                                            // bin 0 has no bin before it
    bk += (uint32_t)__popcll((w ^ ((w << 1) | (p >> 63))) & pairs);
#pragma unroll
    for (int k = 1; k <= kWord; ++k) {
      if (k <= max_lag) {
        const uint64_t before = k == kWord ? p : (w << (k & 63)) | (p >> ((kWord - k) & 63));
        s[k - 1] += (uint32_t)__popcll(w & before);
      }
    }
    p = w;
  }

  const size_t o = plane * (size_t)N + n;
  if (total) atomicAdd(&rep_sum[o], total);
  if (bk) atomicAdd(&rep_bk[o], bk);
  const size_t ol = plane * (size_t)max_lag * N + n;
#pragma unroll
  for (int k = 1; k <= kWord; ++k)
    if (k <= max_lag && s[k - 1]) atomicAdd(&rep_lag[ol + (size_t)(k - 1) * N], s[k - 1]);

  if (blockIdx.y == 0) {                                                   // the two ends, once per cell
    uint64_t last = 0ull;                                                  // bit j = bin L - 64 + j
    if (L >= kWord) {
      last = load_word(col, ldn, L - kWord, kWord);
    } else {
      last = load_word(col, ldn, 0, L) << (kWord - L);
    }
#pragma unroll
    for (int k = 1; k <= kWord; ++k) {
      if (k <= max_lag) {
        const uint32_t h = (uint32_t)__popcll(k == kWord ? first : first & ((1ull << (k & 63)) - 1ull));
        const uint32_t t = (uint32_t)__popcll(last >> ((kWord - k) & 63));
        if (h) atomicAdd(&rep_head[ol + (size_t)(k - 1) * N], h);
        if (t) atomicAdd(&rep_tail[ol + (size_t)(k - 1) * N], t);
      }
    }
  }

  if (HAS_CN) {
    const uint8_t* ccol = cn + plane * (size_t)plane_stride + n;
    uint32_t zeros = 0u, cbk = 0u;
    uint8_t prev = ccol[(size_t)(t0 > 0 ? t0 - 1 : 0) * ldn];
#pragma unroll 8
    for (int t = t0; t < t1; ++t) {
      const uint8_t c = ccol[(size_t)t * ldn];
      zeros += c == 0;
      cbk += c != prev;
      prev = c;
    }
    if (zeros) atomicAdd(&cn0[o], zeros);
    if (cbk) atomicAdd(&cn_bk[o], cbk);
  }
}

// part[chunk][n] = sum of cell n over the chunk's bins, fp64, in a fixed order.
template <typename T>
__global__ __launch_bounds__(kLanes) void phase_sum_kernel(int L, int N, int ldn, const T* __restrict__ x, int chunk,
                                                           double* __restrict__ part) {
  const int n = blockIdx.x * kLanes + threadIdx.x;
  if (n >= N) return;
  const T* col = x + n;
  const int t0 = blockIdx.y * chunk, t1 = min(L, t0 + chunk);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int t = t0;
#pragma unroll 4
  for (; t + 4 <= t1; t += 4) {
    a0 += (double)col[(size_t)t * ldn];
    a1 += (double)col[(size_t)(t + 1) * ldn];
    a2 += (double)col[(size_t)(t + 2) * ldn];
    a3 += (double)col[(size_t)(t + 3) * ldn];
  }
  for (; t < t1; ++t) a0 += (double)col[(size_t)t * ldn];
  part[(size_t)blockIdx.y * N + n] = (a0 + a1) + (a2 + a3);
}

// part_c[chunk][k][n] = sum over the pairs (t - k, t), t in the chunk, of the centred products.
template <typename T>
__global__ __launch_bounds__(kLanes) void phase_prod_kernel(int L, int N, int ldn, const T* __restrict__ x,
                                                            int max_lag, int chunk, int n_chunks,
                                                            const double* __restrict__ part_sum,
                                                            double* __restrict__ mean, double* __restrict__ part_c) {
  __shared__ double ring[kWord * kLanes];                                  // [bin & 63][lane]
  const int lane = threadIdx.x, n = blockIdx.x * kLanes + lane;
  if (n >= N) return;
  double m = 0.0;
  for (int c = 0; c < n_chunks; ++c) m += part_sum[(size_t)c * N + n];
  m /= (double)L;
  if (!isfinite(m)) m = __builtin_nan("");                                 // an Inf in the series: every output NaN
  if (blockIdx.y == 0) mean[n] = m;

  const T* col = x + n;
  const int t0 = blockIdx.y * chunk, t1 = min(L, t0 + chunk);
#pragma unroll 8
  for (int j = 1; j <= kWord; ++j) {                                       // the halo: bins [t0 - 64, t0)
    const int sb = t0 - j;
    ring[(sb & (kWord - 1)) * kLanes + lane] = sb >= 0 ? (double)col[(size_t)sb * ldn] - m : 0.0;
  }
  double acc[kWord + kStep];                                               // lags above max_lag are never stored
#pragma unroll
  for (int k = 0; k < kWord + kStep; ++k) acc[k] = 0.0;

  for (int t = t0; t < t1; t += kStep) {
    double d[kStep];
#pragma unroll
    for (int i = 0; i < kStep; ++i) d[i] = t + i < t1 ? (double)col[(size_t)(t + i) * ldn] - m : 0.0;
#pragma unroll
    for (int i = 0; i < kStep; ++i)                                        // pairs inside these four bins
#pragma unroll
      for (int e = 0; e <= i; ++e) acc[i - e] += d[e] * d[i];
#pragma unroll
    for (int j = 1; j <= kWord; ++j) {                                     // the bin j before the first of them
      if (j <= max_lag) {
        const double e = ring[((t - j) & (kWord - 1)) * kLanes + lane];
#pragma unroll
        for (int i = 0; i < kStep; ++i) acc[j + i] += e * d[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kStep; ++i) ring[((t + i) & (kWord - 1)) * kLanes + lane] = d[i];
  }
#pragma unroll
  for (int k = 0; k <= kWord; ++k)
    if (k <= max_lag) part_c[((size_t)blockIdx.y * (max_lag + 1) + k) * N + n] = acc[k];
}

// c[k][n] = the chunks' partials added in chunk order.
__global__ __launch_bounds__(256) void phase_reduce_kernel(int64_t count, int n_chunks,
                                                           const double* __restrict__ part_c, double* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  double a = 0.0;
  for (int ch = 0; ch < n_chunks; ++ch) a += part_c[(size_t)ch * count + i];
  c[i] = a;
}

inline bool bad_series(int L, int N, int ldn, int max_lag, const void* base) {
  return N < 1 || ldn < N || (ldn % 16) != 0 || !base || (reinterpret_cast<uintptr_t>(base) % 16) != 0 ||
         max_lag < 1 || max_lag > PERT_PHASE_MAX_LAG || L <= max_lag || L >= (1 << 20);
}

inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

template <typename T>
int launch_acf(int L, int N, int ldn, const void* x, int max_lag, int chunk, int n_chunks, double* mean, double* c,
               double* ws, hipStream_t stream) {
  const T* xs = static_cast<const T*>(x);
  double* part_sum = ws;                                                   // [n_chunks][N]
  double* part_c = ws + (size_t)n_chunks * N;                              // [n_chunks][max_lag + 1][N]
  const dim3 grid(ceil_div(N, kLanes), n_chunks);
  hipLaunchKernelGGL(phase_sum_kernel<T>, grid, dim3(kLanes), 0, stream, L, N, ldn, xs, chunk, part_sum);
  hipLaunchKernelGGL(phase_prod_kernel<T>, grid, dim3(kLanes), 0, stream, L, N, ldn, xs, max_lag, chunk, n_chunks,
                     part_sum, mean, part_c);
  const int64_t count = (int64_t)(max_lag + 1) * N;
  hipLaunchKernelGGL(phase_reduce_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, count,
                     n_chunks, part_c, c);
  return last_error();
}

}  // namespace

extern "C" int pert_phase_counts(int32_t L, int32_t N, int32_t ldn, int32_t n_planes, int64_t plane_stride,
                                 const uint8_t* rep, const uint8_t* cn, int32_t max_lag, uint32_t* rep_sum,
                                 uint32_t* rep_bk, uint32_t* cn_bk, uint32_t* cn0, uint32_t* rep_lag,
                                 uint32_t* rep_head, uint32_t* rep_tail, hipStream_t stream) {
  if (bad_series(L, N, ldn, max_lag, rep) || n_planes < 1 || n_planes > 65535 || !rep_sum || !rep_bk || !rep_lag ||
      !rep_head || !rep_tail)
    return PERT_E_ARG;
  if (cn && ((reinterpret_cast<uintptr_t>(cn) % 16) != 0 || !cn_bk || !cn0)) return PERT_E_ARG;
  if (n_planes > 1 && (plane_stride < (int64_t)L * ldn || (plane_stride % 16) != 0)) return PERT_E_ARG;
  const int gx = ceil_div(N, kLanes);
  const int chunk = chunk_bins(L, (int64_t)gx * n_planes);
  const dim3 grid(gx, ceil_div(L, chunk), n_planes);
  if (cn)
    hipLaunchKernelGGL(phase_counts_kernel<true>, grid, dim3(kLanes), 0, stream, L, N, ldn, plane_stride, rep, cn,
                       max_lag, chunk, rep_sum, rep_bk, cn_bk, cn0, rep_lag, rep_head, rep_tail);
  else
    hipLaunchKernelGGL(phase_counts_kernel<false>, grid, dim3(kLanes), 0, stream, L, N, ldn, plane_stride, rep, cn,
                       max_lag, chunk, rep_sum, rep_bk, cn_bk, cn0, rep_lag, rep_head, rep_tail);
  return last_error();
}

extern "C" int pert_phase_acf_workspace(int32_t L, int32_t N, int32_t max_lag, int64_t* bytes) {
  if (!bytes || N < 1 || max_lag < 1 || max_lag > PERT_PHASE_MAX_LAG || L <= max_lag || L >= (1 << 20))
    return PERT_E_ARG;
  const int n_chunks = ceil_div(L, chunk_bins(L, ceil_div(N, kLanes)));
  *bytes = (int64_t)sizeof(double) * n_chunks * (max_lag + 2) * N;
  return PERT_OK;
}

extern "C" int pert_phase_acf(int32_t L, int32_t N, int32_t ldn, const void* x, int32_t is_f64, int32_t max_lag,
                              double* mean, double* c, void* workspace, int64_t workspace_bytes,
                              hipStream_t stream) {
  if (bad_series(L, N, ldn, max_lag, x) || !mean || !c || !workspace ||
      (reinterpret_cast<uintptr_t>(workspace) % 8) != 0)
    return PERT_E_ARG;
  int64_t need = 0;
  if (pert_phase_acf_workspace(L, N, max_lag, &need) != PERT_OK || workspace_bytes < need) return PERT_E_ARG;
  const int chunk = chunk_bins(L, ceil_div(N, kLanes));
  const int n_chunks = ceil_div(L, chunk);
  double* ws = static_cast<double*>(workspace);
  return is_f64 ? launch_acf<double>(L, N, ldn, x, max_lag, chunk, n_chunks, mean, c, ws, stream)
                : launch_acf<float>(L, N, ldn, x, max_lag, chunk, n_chunks, mean, c, ws, stream);
}
