// boot_kernels.hip -- gfx950 kernels of the cell bootstrap (cell_bootstrap.py): the pseudobulk
// counts and the time-from-scheduled-replication histogram of rt_kernels.hip for B resampled
// sets of cells at once.  A replicate is an integer weight per cell (how often the resampling
// picked it), so its per-bin counts are rep . w and its histogram is the rank-1 histogram with
// every (bin, cell) row counted w[n] times: all replicates share one read of the one byte per
// (bin, cell), instead of one read per replicate.
//
// Exactness (the rule of rt_kernels.hip): integer adds only (LDS and global integer atomics,
// register sums and dot products), so results do not depend on arrival order and repeat bit for
// bit.  The interval of t is decided by rt_interval.h's find_interval, the routine of
// pert_rt_tfs_hist.  Outputs are added to: the caller zeroes them.
//
// Access: a lane reads 16 consecutive cells of one bin, and of one weight row, as one 16-byte
// load each; cells >= N are masked by index in both operands (padding bytes are undefined).

#include "../../include/pert_hip.h"
#include "rt_interval.h"
#include "sim_math.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>

namespace {

using pert_rt::guess_interval;
using pert_rt::kEdgeSlots;
using pert_rt::settle_interval;

constexpr int kT = 256;                 // threads per workgroup
constexpr int kCV = 16;                 // cells per lane: one 16-byte load
constexpr int kChunkCells = 64 * kCV;   // cells of one wave-wide load
constexpr int kHistRows = 64;           // bins per tile of the histogram kernel (as rt_hist_kernel)
constexpr int kHistCPR = 16;            // histogram kernel: lanes across the cells (256 cells per workgroup)
constexpr int kDotRows = 8;             // counts kernel: weight rows per workgroup (register tile)
constexpr int kDotBins = 8;             // counts kernel: bins per workgroup (register tile)

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}

__device__ __forceinline__ uint32_t dword_of(const uint4& v, int d) {
  return d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
}

// ---- the resampler ----------------------------------------------------------------------------

// Draw (b, j): scratch[b - b0][cell picked] += 1.  Grid (positions / 256, replicates).
__global__ __launch_bounds__(kT) void boot_draw_kernel(int N, const int32_t* __restrict__ pos_lo,
                                                       const int32_t* __restrict__ pos_n,
                                                       const int32_t* __restrict__ order, pert_sim::Key key,
                                                       uint64_t b0, uint32_t* __restrict__ scratch,
                                                       uint32_t* __restrict__ flag) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= N) return;
  const uint64_t b = b0 + blockIdx.y;
  const pert_sim::Words w = pert_sim::philox4x32_10(
      pert_sim::Words{(uint32_t)j, (uint32_t)b, PERT_TAG_BOOT, (uint32_t)(b >> 32)}, key.k0, key.k1);
  const uint64_t word = ((uint64_t)w.y << 32) | (uint64_t)w.x;
  const int lo = pos_lo[j], n_g = pos_n[j];
  if (lo < 0 || n_g < 1 || lo > j || (int64_t)lo + n_g > N || (int64_t)lo + n_g <= j) {   // not a stratum layout
    atomicOr(flag, 2u);
    return;
  }
  const int cell = order[lo + (int)__umul64hi(word, (uint64_t)n_g)];
  if (cell < 0 || cell >= N) {
    atomicOr(flag, 2u);
    return;
  }
  atomicAdd(&scratch[(size_t)blockIdx.y * N + cell], 1u);
}

// w[b][n] = the 32-bit count as a byte (columns [N, ldw) zero); flag bit 0 if a count exceeds 255.
__global__ __launch_bounds__(kT) void boot_narrow_kernel(int N, int ldw, const uint32_t* __restrict__ scratch,
                                                         uint8_t* __restrict__ w, uint32_t* __restrict__ flag) {
  const int n = blockIdx.x * kT + threadIdx.x;
  if (n >= ldw) return;
  uint32_t c = n < N ? scratch[(size_t)blockIdx.y * N + n] : 0u;
  if (c > 255u) {
    atomicOr(flag, 1u);
    c = 255u;
  }
  w[(size_t)blockIdx.y * ldw + n] = (uint8_t)c;
}

// ---- counts: count[c][l] += sum_n wg[c][n] rep[l][n] -----------------------------------------------

// Grid (weight-row tiles of 8, bin tiles of 8): neighbouring workgroups share a rep tile in the
// L2.  A wave takes every fourth 1024-cell chunk; a lane keeps the 8 x 8 sums of its 16 cells in
// registers (v_dot4_u32_u8), a loaded rep fragment serving 8 weight rows and a weight fragment
// 8 bins.  One wave reduction per sum at the end, the four waves meet in LDS, one global add per
// non-zero sum.
__global__ __launch_bounds__(kT) void boot_counts_kernel(int L, int N, int ldn, const uint8_t* __restrict__ rep,
                                                         int C, int ldw, const uint8_t* __restrict__ wg,
                                                         uint32_t* __restrict__ count) {
  __shared__ uint32_t s_acc[kDotRows * kDotBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.x * kDotRows, l0 = blockIdx.y * kDotBins;
  if (threadIdx.x < kDotRows * kDotBins) s_acc[threadIdx.x] = 0u;
  __syncthreads();

  uint32_t acc[kDotRows][kDotBins];
#pragma unroll
  for (int c = 0; c < kDotRows; ++c)
#pragma unroll
    for (int r = 0; r < kDotBins; ++r) acc[c][r] = 0u;

  const int n_chunks = (N + kChunkCells - 1) / kChunkCells;
  for (int chunk = wave; chunk < n_chunks; chunk += kT / 64) {
    const int n0 = (chunk * 64 + lane) * kCV;
    if (n0 >= N) continue;
    uint32_t live[4] = {0u, 0u, 0u, 0u};  // byte mask of the cells < N
#pragma unroll
    for (int j = 0; j < kCV; ++j)
      if (n0 + j < N) live[j >> 2] |= 0xFFu << (8 * (j & 3));
    uint32_t rv[kDotBins][4];
#pragma unroll
    for (int r = 0; r < kDotBins; ++r) {
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (l0 + r < L) q = *reinterpret_cast<const uint4*>(rep + (size_t)(l0 + r) * ldn + n0);
#pragma unroll
      for (int d = 0; d < 4; ++d) rv[r][d] = dword_of(q, d) & live[d];
    }
#pragma unroll
    for (int c = 0; c < kDotRows; ++c) {
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (c0 + c < C) q = *reinterpret_cast<const uint4*>(wg + (size_t)(c0 + c) * ldw + n0);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t wv = dword_of(q, d) & live[d];
#pragma unroll
        for (int r = 0; r < kDotBins; ++r) acc[c][r] = __builtin_amdgcn_udot4(wv, rv[r][d], acc[c][r], false);
      }
    }
  }

#pragma unroll
  for (int c = 0; c < kDotRows; ++c)
#pragma unroll
    for (int r = 0; r < kDotBins; ++r) {
      const uint32_t s = wave_sum_u32(acc[c][r]);
      if (lane == 0 && s != 0u) atomicAdd(&s_acc[c * kDotBins + r], s);
    }
  __syncthreads();
  if (threadIdx.x < kDotRows * kDotBins) {
    const int c = c0 + threadIdx.x / kDotBins, l = l0 + threadIdx.x % kDotBins;
    const uint32_t s = s_acc[threadIdx.x];
    if (s != 0u && c < C && l < L) atomicAdd(&count[(size_t)c * L + l], s);
  }
}

// ---- the weighted histogram ---------------------------------------------------------------------

// Grid (cell chunks of 256 = 16 CPR cells, bin slices); tiles of 64 bins.  Thread (cq, rs) =
// (tid % CPR, tid / CPR), CPR = 16, owns cells [n0, n0 + 16) and the tile's bins rs, rs + RG, ...
// (RG = 256 / CPR = 16 row groups, 4 bins each).  Measured against CPR = 64 (1024 cells per
// workgroup, 16 bins per thread) the narrow shape was faster at 2,000 and at 10,000 cells
// (DESIGN.md 6p): more workgroups, and a flush per 16 K rather than 64 K decisions still pays.
// A thread reads its bytes of the tile once and keeps them as one bit each (a replicated state
// is any non-zero byte): 16 registers, bit k of cb[j] = bin rs + RG k of cell j.
// Then the replicates walk over the tile: a replicate's hours[g][tile bins] rows are staged in
// LDS, its weights come as one 16-byte load, each (bin, cell) with a non-zero weight adds that
// weight to hist_n / hist_rep [G][nb] in LDS, and the non-zero slots are flushed to [Bc][G][nb]
// with global integer atomics.  A lane whose 16 weights are all zero (cells the resampling left
// out, or outside the groups) does nothing for that replicate but the barriers.  Decisions go
// four at a time: four t, four guesses and their eight edge loads are issued before the first
// comparison (the LDS latency of a decision's chain is paid once per four).  Workgroups start at
// different replicates, so that their flushes do not all meet on one replicate's slots.
//
// LDS: sizeof(T) (264 + 64 G) + 8 G nb bytes.  The usual call (G <= 4, nb = 200, fp32) takes at
// most 8.3 KiB, and the registers, not the LDS, set the occupancy there: 132 VGPRs in fp32 and
// 162 in fp64, 3 waves per SIMD = 3 workgroups per CU, 25 KiB of its 160 KiB.  The LDS becomes
// the limit past 53 KiB per workgroup (G >= 29 at nb = 200 in fp32); the largest call (G = 32,
// nb = 256, fp64) takes 82 KiB: one workgroup per CU, 1 wave per SIMD.
template <typename T>
__global__ __launch_bounds__(kT) void boot_hist_kernel(int L, int N, int ldn, int G, const uint8_t* __restrict__ rep,
                                                       const int32_t* __restrict__ group, int Bc, int ldw,
                                                       const uint8_t* __restrict__ w, const T* __restrict__ hours,
                                                       const T* __restrict__ f10, const T* __restrict__ edges,
                                                       int nb, uint32_t* __restrict__ hist_n,
                                                       uint32_t* __restrict__ hist_rep, int n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* s_edges = reinterpret_cast<T*>(smem);                                  // [nb + 1]
  T* s_hours = s_edges + kEdgeSlots;                                        // [G][64]
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(s_hours + (size_t)G * kHistRows);   // [2][G][nb]
  const int n_slots = G * nb;

  constexpr int CPR = kHistCPR;
  constexpr int RG = kT / CPR;                 // row groups: bins rs, rs + RG, ... of the tile
  constexpr int kRows = kHistRows / RG;        // bins of the tile per thread
  constexpr int kU = 4;                        // decisions in flight
  static_assert(kRows % kU == 0 && kRows <= 32, "whole groups of decisions; one bit per bin in cb");

  const int cq = threadIdx.x % CPR, rs = threadIdx.x / CPR;
  const int n0 = (blockIdx.x * CPR + cq) * kCV;
  for (int i = threadIdx.x; i <= nb; i += kT) s_edges[i] = edges[i];
  for (int i = threadIdx.x; i < 2 * n_slots; i += kT) s_hist[i] = 0u;

  int grp[kCV];
  T f[kCV];
  uint32_t live[4] = {0u, 0u, 0u, 0u};    // byte mask of the cells < N that belong to a group
#pragma unroll
  for (int j = 0; j < kCV; ++j) {
    const bool ok = n0 + j < N;
    int g = ok ? group[n0 + j] : -1;
    if (g < 0 || g >= G) g = -1;                                            // excluded; keeps s_hours in bounds
    grp[j] = g < 0 ? 0 : g;
    f[j] = ok ? f10[n0 + j] : (T)0;
    if (g >= 0) live[j >> 2] |= 0xFFu << (8 * (j & 3));
  }
  const bool any = (live[0] | live[1] | live[2] | live[3]) != 0u;           // then n0 < N: loads stay in the row
  __syncthreads();
  const T e0 = s_edges[0];
  const float inv_width = (float)nb / (float)(s_edges[nb] - e0);

  for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const int l0 = tile * kHistRows;
    const int rows = min(kHistRows, L - l0);
    const int k_end = rows > rs ? (rows - rs + RG - 1) / RG : 0;            // this thread's bins of the tile
    uint32_t cb[kCV];
#pragma unroll
    for (int j = 0; j < kCV; ++j) cb[j] = 0u;
    if (any) {
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        if (k >= k_end) continue;
        const uint4 q = *reinterpret_cast<const uint4*>(rep + (size_t)(l0 + rs + RG * k) * ldn + n0);
#pragma unroll
        for (int j = 0; j < kCV; ++j)
          if ((dword_of(q, j >> 2) >> (8 * (j & 3))) & 0xFFu) cb[j] |= 1u << k;
      }
    }

    const int b_first = (int)((blockIdx.x * 7u + blockIdx.y * 13u) % (uint32_t)Bc);
    for (int bi = 0; bi < Bc; ++bi) {
      const int b = bi + b_first < Bc ? bi + b_first : bi + b_first - Bc;
      __syncthreads();                                   // the last replicate's hours are read, its flush is done
      for (int i = threadIdx.x; i < G * kHistRows; i += kT) {
        const int l = l0 + (i & (kHistRows - 1));
        s_hours[i] = l < L ? hours[((size_t)b * G + i / kHistRows) * L + l] : (T)0;
      }
      uint32_t wv[4] = {0u, 0u, 0u, 0u};
      if (any) {
        const uint4 q = *reinterpret_cast<const uint4*>(w + (size_t)b * ldw + n0);
#pragma unroll
        for (int d = 0; d < 4; ++d) wv[d] = dword_of(q, d) & live[d];
      }
      __syncthreads();
      if ((wv[0] | wv[1] | wv[2] | wv[3]) != 0u) {
#pragma unroll
        for (int j = 0; j < kCV; ++j) {
          const uint32_t wj = (wv[j >> 2] >> (8 * (j & 3))) & 0xFFu;
          if (wj == 0u) continue;
          const T* h = s_hours + grp[j] * kHistRows + rs;
          uint32_t* hn = s_hist + grp[j] * nb;
          for (int k0 = 0; k0 < k_end; k0 += kU) {
            T t[kU], lo[kU], hi[kU];
            int i[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {               // bins past the tile's end repeat its last: not counted below
              t[u] = h[RG * min(k0 + u, k_end - 1)] - f[j];
              i[u] = guess_interval<T>(t[u], nb, e0, inv_width);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
              lo[u] = s_edges[i[u]];
              hi[u] = s_edges[i[u] + 1];
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
              if (k0 + u >= k_end) continue;
              const int ii = settle_interval<T>(t[u], i[u], lo[u], hi[u], s_edges, nb);
              if (ii < 0) continue;
              atomicAdd(&hn[ii], wj);
              if ((cb[j] >> (k0 + u)) & 1u) atomicAdd(&hn[n_slots + ii], wj);
            }
          }
        }
      }
      __syncthreads();
      for (int i = threadIdx.x; i < 2 * n_slots; i += kT) {   // one global add per non-zero slot
        const uint32_t c = s_hist[i];
        if (c != 0u) {
          s_hist[i] = 0u;
          atomicAdd(i < n_slots ? &hist_n[(size_t)b * n_slots + i] : &hist_rep[(size_t)b * n_slots + i - n_slots], c);
        }
      }
    }
  }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) != 0; }

inline bool bad_operands(int L, int N, int ldn, const void* rep, int rows, int ldw, const void* w) {
  return L < 1 || N < 1 || ldn < N || (ldn % kCV) != 0 || !rep || misaligned(rep) || rows < 1 || ldw < N ||
         (ldw % kCV) != 0 || !w || misaligned(w);
}

inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

template <typename T>
int launch_boot_hist(int L, int N, int ldn, int G, const uint8_t* rep, const int32_t* group, int Bc, int ldw,
                     const uint8_t* w, const void* hours, const void* f10, const void* edges, int nb,
                     uint32_t* hist_n, uint32_t* hist_rep, hipStream_t stream) {
  const int n_tiles = ceil_div(L, kHistRows);
  const int gx = ceil_div(N, kHistCPR * kCV);
  const int gy = std::min(n_tiles, std::max(1, ceil_div(4096, gx)));
  const size_t lds = sizeof(T) * ((size_t)kEdgeSlots + (size_t)G * kHistRows) + sizeof(uint32_t) * 2 * (size_t)G * nb;
  auto kern = boot_hist_kernel<T>;
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return PERT_E_HIP_BASE + (int)ea;
  }
  hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(kT), lds, stream, L, N, ldn, G, rep, group, Bc, ldw, w,
                     static_cast<const T*>(hours), static_cast<const T*>(f10), static_cast<const T*>(edges), nb,
                     hist_n, hist_rep, n_tiles);
  return last_error();
}

}  // namespace

extern "C" int pert_boot_weights(int32_t N, int32_t ldw, const int32_t* pos_lo, const int32_t* pos_n,
                                 const int32_t* order, uint64_t seed, int64_t b0, int32_t Bc, uint32_t* scratch,
                                 uint8_t* w, uint32_t* flag, hipStream_t stream) {
  if (N < 1 || ldw < N || (ldw % kCV) != 0 || !pos_lo || !pos_n || !order || b0 < 0 || Bc < 1 ||
      Bc > PERT_BOOT_MAX_LAUNCH || !scratch || !w || misaligned(w) || !flag)
    return PERT_E_ARG;
  hipLaunchKernelGGL(boot_draw_kernel, dim3(ceil_div(N, kT), Bc), dim3(kT), 0, stream, N, pos_lo, pos_n, order,
                     pert_sim::make_key(seed, PERT_TAG_BOOT), (uint64_t)b0, scratch, flag);
  int rc = last_error();
  if (rc != PERT_OK) return rc;
  hipLaunchKernelGGL(boot_narrow_kernel, dim3(ceil_div(ldw, kT), Bc), dim3(kT), 0, stream, N, ldw, scratch, w, flag);
  return last_error();
}

extern "C" int pert_boot_counts(int32_t L, int32_t N, int32_t ldn, const uint8_t* rep, int32_t C, int32_t ldw,
                                const uint8_t* wg, uint32_t* count, hipStream_t stream) {
  if (bad_operands(L, N, ldn, rep, C, ldw, wg) || !count) return PERT_E_ARG;
  if ((int64_t)N * 255 >= ((int64_t)1 << 32)) return PERT_E_ARG;             // a counter could wrap
  const int gy = ceil_div(L, kDotBins);
  if (gy > 65535) return PERT_E_ARG;
  hipLaunchKernelGGL(boot_counts_kernel, dim3(ceil_div(C, kDotRows), gy), dim3(kT), 0, stream, L, N, ldn, rep, C, ldw,
                     wg, count);
  return last_error();
}

extern "C" int pert_boot_tfs_hist(int32_t L, int32_t N, int32_t ldn, int32_t G, const uint8_t* rep,
                                  const int32_t* group, int32_t Bc, int32_t ldw, const uint8_t* w, const void* hours,
                                  const void* f10, const void* edges, int32_t n_edges, int32_t is_f64,
                                  uint32_t* hist_n, uint32_t* hist_rep, hipStream_t stream) {
  if (bad_operands(L, N, ldn, rep, Bc, ldw, w) || !group || G < 1 || G > PERT_RT_MAX_GROUPS || !hours || !f10 ||
      !edges || !hist_n || !hist_rep || n_edges < 2 || n_edges > PERT_RT_MAX_EDGES)
    return PERT_E_ARG;
  const int nb = n_edges - 1;
  return is_f64 ? launch_boot_hist<double>(L, N, ldn, G, rep, group, Bc, ldw, w, hours, f10, edges, nb, hist_n,
                                           hist_rep, stream)
                : launch_boot_hist<float>(L, N, ldn, G, rep, group, Bc, ldw, w, hours, f10, edges, nb, hist_n,
                                          hist_rep, stream);
}
