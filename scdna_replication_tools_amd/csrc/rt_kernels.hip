// rt_kernels.hip -- gfx950 kernels of the downstream replication-timing analyses
// (rt_profiles.py): pseudobulk counts and the time-from-scheduled-replication histogram,
// both computed from the decode's uint8 [L][ldn] replication states without the long table.
//
// Reference: compute_pseudobulk_rt_profiles.py:16-38 (the per-locus mean over cells, whole
// population and per clone) and calculate_twidth.py:37-71 (for each of 200 intervals of
// t = hours[locus] - 10 frac[cell], the rows inside it and how many of them are replicated).
// Every row's t is rank-1 (a per-(group, bin) value minus a per-cell value), so both are
// streaming passes over one byte per (bin, cell) that produce integer counts; the host
// turns the counts into the reference's fractions with the reference's own operations.
//
// Exactness: integer adds only (LDS and global integer atomics, register sums), so results do
// not depend on arrival order and repeat bit for bit.  t is one subtraction in the caller's
// type; its interval is decided by comparisons against the edge table alone (an arithmetic
// guess picks where the comparisons start, never the answer).
//
// Access: a lane reads 16 consecutive cells of one bin as one 16-byte load; cells >= N are
// masked by index (the padding bytes of a row are undefined).  Outputs are added to: the
// caller zeroes them (launches over cell or group subsets then sum by themselves).

#include "../../include/pert_hip.h"
#include "rt_interval.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kT = 256;                 // threads per workgroup
constexpr int kCV = 16;                 // cells per lane: one 16-byte load
constexpr int kCountRows = 32;          // bins per tile of the counts kernel (8 per wave, in registers)
constexpr int kCountRPW = kCountRows / (kT / 64);
constexpr int kCountCells = 64 * kCV;   // cells per workgroup of the counts kernel
constexpr int kHistRows = 64;           // bins per tile of the histogram kernel (hours rows staged in LDS)
using pert_rt::find_interval;           // rt_interval.h: shared with boot_kernels.hip
using pert_rt::kEdgeSlots;
constexpr int kTileCells = 64;          // cells per workgroup of the per-cell LDS tile

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}

__device__ __forceinline__ uint32_t dword_of(const uint4& v, int d) {
  return d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
}

// bin_count[g][l] += replicated cells of group g in bin l; cell_count[n] += replicated bins of cell n.
// Grid (cell chunks of 1024, bin slices); a wave owns whole bins of its chunk (8 per tile, loaded
// together), so a bin's per-group sum is one wave reduction and one global add per non-zero sum.
__global__ __launch_bounds__(kT) void rt_counts_kernel(int L, int N, int ldn, int G, const uint8_t* __restrict__ rep,
                                                       const int32_t* __restrict__ group,
                                                       uint32_t* __restrict__ bin_count,
                                                       uint32_t* __restrict__ cell_count, int n_tiles) {
  __shared__ uint32_t s_cell[kCountCells];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 64 + lane) * kCV;
  const bool have = n0 < N;
  int grp[kCV];
  uint32_t live[4] = {0u, 0u, 0u, 0u};  // byte mask of the cells < N
  uint32_t acc[kCV];
#pragma unroll
  for (int j = 0; j < kCV; ++j) {
    const bool ok = n0 + j < N;
    grp[j] = ok ? group[n0 + j] : -1;
    if (ok) live[j >> 2] |= 0xFFu << (8 * (j & 3));
    acc[j] = 0u;
  }
  for (int i = threadIdx.x; i < kCountCells; i += kT) s_cell[i] = 0u;
  __syncthreads();

  for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const int l0 = tile * kCountRows + wave * kCountRPW;
    uint32_t v[kCountRPW][4];
#pragma unroll
    for (int r = 0; r < kCountRPW; ++r) {
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (have && l0 + r < L) q = *reinterpret_cast<const uint4*>(rep + (size_t)(l0 + r) * ldn + n0);
#pragma unroll
      for (int d = 0; d < 4; ++d) v[r][d] = dword_of(q, d) & live[d];
    }
#pragma unroll
    for (int r = 0; r < kCountRPW; ++r)
#pragma unroll
      for (int j = 0; j < kCV; ++j) acc[j] += (v[r][j >> 2] >> (8 * (j & 3))) & 0xFFu;
    for (int g = 0; g < G; ++g) {
      uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < kCV; ++j)
        if (grp[j] == g) m[j >> 2] |= 0xFFu << (8 * (j & 3));
      if (!__any((m[0] | m[1] | m[2] | m[3]) != 0u)) continue;      // no cell of g in this wave's chunk
#pragma unroll
      for (int r = 0; r < kCountRPW; ++r) {
        uint32_t s = 0u;
#pragma unroll
        for (int d = 0; d < 4; ++d) s = __builtin_amdgcn_sad_u8(v[r][d] & m[d], 0u, s);   // sum of the 4 bytes
        s = wave_sum_u32(s);
        if (lane == 0 && s != 0u && l0 + r < L) atomicAdd(&bin_count[(size_t)g * L + l0 + r], s);
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kCV; ++j)
    if (acc[j] != 0u) atomicAdd(&s_cell[lane * kCV + j], acc[j]);
  __syncthreads();
  for (int i = threadIdx.x; i < kCountCells; i += kT) {
    const int n = blockIdx.x * kCountCells + i;
    const uint32_t c = s_cell[i];
    if (n < N && c != 0u) atomicAdd(&cell_count[n], c);
  }
}

// MODE 0: one histogram over all cells, privatised in LDS.  MODE 1: per-cell histograms, a
// 64-cell x nb x 2 tile in LDS per workgroup (CPR = 4 lanes across the cells, 64 bins per pass).
// MODE 2: per-cell histograms added straight to global memory (the mapping of MODE 0).
// Grid (cell chunks of 16 CPR cells, bin slices); tiles of 64 bins, whose hours rows are in LDS.
template <typename T, int CPR, int MODE>
__global__ __launch_bounds__(kT) void rt_hist_kernel(int L, int N, int ldn, int G, const uint8_t* __restrict__ rep,
                                                     const int32_t* __restrict__ group, const T* __restrict__ hours,
                                                     const T* __restrict__ f10, const T* __restrict__ edges, int nb,
                                                     uint32_t* __restrict__ hist_n, uint32_t* __restrict__ hist_rep,
                                                     int n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* s_edges = reinterpret_cast<T*>(smem);                                  // [nb + 1]
  T* s_hours = s_edges + kEdgeSlots;                                        // [G][64]
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(s_hours + (size_t)G * kHistRows);
  constexpr int RPP = kT / CPR;                                             // bins per pass
  constexpr int kSlots = MODE == 0 ? 2 : MODE == 1 ? 2 * kTileCells : 0;    // x nb histogram words
  static_assert(MODE != 1 || CPR * kCV == kTileCells, "the LDS tile holds the workgroup's cells");

  const int cq = threadIdx.x % CPR, rs = threadIdx.x / CPR;
  const int n0 = (blockIdx.x * CPR + cq) * kCV;
  for (int i = threadIdx.x; i <= nb; i += kT) s_edges[i] = edges[i];
  for (int i = threadIdx.x; i < kSlots * nb; i += kT) s_hist[i] = 0u;

  int grp[kCV];
  T f[kCV];
  bool any = false;
#pragma unroll
  for (int j = 0; j < kCV; ++j) {
    const bool ok = n0 + j < N;
    int g = ok ? group[n0 + j] : -1;
    if (g < 0 || g >= G) g = -1;                                            // excluded; keeps s_hours in bounds
    grp[j] = g;
    f[j] = ok ? f10[n0 + j] : (T)0;
    any = any || g >= 0;
  }
  __syncthreads();
  const T e0 = s_edges[0];
  const float inv_width = (float)nb / (float)(s_edges[nb] - e0);

  for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const int l0 = tile * kHistRows;
    __syncthreads();                                                        // the last tile's hours are read
    for (int i = threadIdx.x; i < G * kHistRows; i += kT) {
      const int l = l0 + (i & (kHistRows - 1));
      s_hours[i] = l < L ? hours[(size_t)(i / kHistRows) * L + l] : (T)0;
    }
    __syncthreads();
    for (int r = rs; r < kHistRows; r += RPP) {
      const int l = l0 + r;
      if (!any || l >= L) continue;
      const uint4 q = *reinterpret_cast<const uint4*>(rep + (size_t)l * ldn + n0);
#pragma unroll
      for (int j = 0; j < kCV; ++j) {
        if (grp[j] < 0) continue;
        const T t = s_hours[grp[j] * kHistRows + r] - f[j];
        const int i = find_interval<T>(t, s_edges, nb, e0, inv_width);
        if (i < 0) continue;
        const uint32_t b = (dword_of(q, j >> 2) >> (8 * (j & 3))) & 0xFFu;
        if (MODE == 0) {
          atomicAdd(&s_hist[i], 1u);
          if (b) atomicAdd(&s_hist[nb + i], b);
        } else if (MODE == 1) {
          const int c = cq * kCV + j;
          atomicAdd(&s_hist[c * nb + i], 1u);
          if (b) atomicAdd(&s_hist[(kTileCells + c) * nb + i], b);
        } else {
          const size_t o = (size_t)(n0 + j) * nb + i;
          atomicAdd(&hist_n[o], 1u);
          if (b) atomicAdd(&hist_rep[o], b);
        }
      }
    }
  }

  if (MODE == 2) return;
  __syncthreads();
  if (MODE == 0) {                                                          // one global add per non-zero slot
    for (int i = threadIdx.x; i < 2 * nb; i += kT) {
      const uint32_t c = s_hist[i];
      if (c != 0u) atomicAdd(i < nb ? &hist_n[i] : &hist_rep[i - nb], c);
    }
  } else {
    const int cells = min(kTileCells, N - (int)blockIdx.x * kTileCells);
    for (int i = threadIdx.x; i < cells * nb; i += kT) {
      const size_t o = (size_t)blockIdx.x * kTileCells * nb + i;
      const uint32_t c = s_hist[i], b = s_hist[kTileCells * nb + i];
      if (c != 0u) atomicAdd(&hist_n[o], c);
      if (b != 0u) atomicAdd(&hist_rep[o], b);
    }
  }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

inline bool bad_matrix(int L, int N, int ldn, int G, const void* rep, const void* group) {
  return L < 1 || N < 1 || ldn < N || (ldn % kCV) != 0 || G < 1 || !rep || !group ||
         (reinterpret_cast<uintptr_t>(rep) % 16) != 0;
}

template <typename T, int CPR, int MODE>
int launch_hist(int L, int N, int ldn, int G, const uint8_t* rep, const int32_t* group, const void* hours,
                const void* f10, const void* edges, int nb, uint32_t* hist_n, uint32_t* hist_rep, int target,
                hipStream_t stream) {
  const int n_tiles = ceil_div(L, kHistRows);
  const int gx = ceil_div(ceil_div(N, kCV), CPR);
  const int gy = std::min(n_tiles, std::max(1, ceil_div(target, gx)));
  const int slots = MODE == 0 ? 2 : MODE == 1 ? 2 * kTileCells : 0;
  const size_t lds = sizeof(T) * ((size_t)kEdgeSlots + (size_t)G * kHistRows) + sizeof(uint32_t) * (size_t)slots * nb;
  auto kern = rt_hist_kernel<T, CPR, MODE>;
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return PERT_E_HIP_BASE + (int)ea;
  }
  hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(kT), lds, stream, L, N, ldn, G, rep, group,
                     static_cast<const T*>(hours), static_cast<const T*>(f10), static_cast<const T*>(edges), nb,
                     hist_n, hist_rep, n_tiles);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

template <typename T>
int launch_hist_mode(int mode, int L, int N, int ldn, int G, const uint8_t* rep, const int32_t* group,
                     const void* hours, const void* f10, const void* edges, int nb, uint32_t* hist_n,
                     uint32_t* hist_rep, hipStream_t stream) {
  if (mode == 0)
    return launch_hist<T, 64, 0>(L, N, ldn, G, rep, group, hours, f10, edges, nb, hist_n, hist_rep, 2048, stream);
  if (mode == 1)   // one workgroup per CU (its LDS): about three rounds of the 256 CUs
    return launch_hist<T, kTileCells / kCV, 1>(L, N, ldn, G, rep, group, hours, f10, edges, nb, hist_n, hist_rep, 768,
                                              stream);
  return launch_hist<T, 64, 2>(L, N, ldn, G, rep, group, hours, f10, edges, nb, hist_n, hist_rep, 2048, stream);
}

}  // namespace

extern "C" int pert_rt_counts(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep, const int32_t* group,
                              uint32_t* bin_count, uint32_t* cell_count, hipStream_t stream) {
  if (bad_matrix(L, N, ldn, G, rep, group) || !bin_count || !cell_count) return PERT_E_ARG;
  const int n_tiles = ceil_div(L, kCountRows);
  const int gx = ceil_div(N, kCountCells);
  const int gy = std::min(n_tiles, std::max(1, 1024 / gx));
  hipLaunchKernelGGL(rt_counts_kernel, dim3(gx, gy), dim3(kT), 0, stream, L, N, ldn, G, rep, group, bin_count,
                     cell_count, n_tiles);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

extern "C" int pert_rt_tfs_hist(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep,
                                const int32_t* group, const void* hours, const void* f10, const void* edges,
                                int32_t n_edges, int32_t is_f64, int32_t per_cell, uint32_t* hist_n,
                                uint32_t* hist_rep, hipStream_t stream) {
  if (bad_matrix(L, N, ldn, G, rep, group) || G > PERT_RT_MAX_GROUPS || !hours || !f10 || !edges || !hist_n ||
      !hist_rep || n_edges < 2 || n_edges > PERT_RT_MAX_EDGES || per_cell < 0 || per_cell > 2)
    return PERT_E_ARG;
  if ((int64_t)L * (int64_t)N >= ((int64_t)1 << 32)) return PERT_E_ARG;     // a counter could wrap
  const int nb = n_edges - 1;
  return is_f64 ? launch_hist_mode<double>(per_cell, L, N, ldn, G, rep, group, hours, f10, edges, nb, hist_n,
                                           hist_rep, stream)
                : launch_hist_mode<float>(per_cell, L, N, ldn, G, rep, group, hours, f10, edges, nb, hist_n,
                                          hist_rep, stream);
}
