// cpd_kernels.hip -- gfx950 kernels of the cell level's change-point search (normalize_cell.py).
//
// Reference: normalize_by_cell.py:45-46 and :73-74, ruptures' KernelCPD(kernel='linear',
// min_size=2).fit(Y).predict(n_bkps) with n_bkps = 2 and 1: the breakpoints that minimise the sum of
// the segments' costs sum y^2 - (sum y)^2 / len, that is, that maximise the sum of (segment sum)^2 / len.
// The definition this file computes, for a profile Y[0..n):
//   S[0] = 0, S[i] = S[i-1] + Y[i-1]        sequential fp64, in bin order
//   rinv[k] = 1.0 / k                       correctly rounded
//   two breakpoints, over 2 <= a, a + 2 <= b, b <= n - 2:
//     G(a, b) = (S[a] S[a]) rinv[a] + ((S[b] - S[a]) (S[b] - S[a])) rinv[b - a]
//               + ((S[n] - S[b]) (S[n] - S[b])) rinv[n - b]
//   one breakpoint, over 2 <= a <= n - 2:
//     G(a) = (S[a] S[a]) rinv[a] + ((S[n] - S[a]) (S[n] - S[a])) rinv[n - a]
// every operation one IEEE fp64 operation, the terms added left to right, nothing fused; the largest
// G wins, a tie goes to the smallest a, then the smallest b.
//
// Three launches a call:
//   prefix   one wave per cell: 64 values at a time through LDS, lane 0 adds them in order
//   search   grid (tiles of a, cells), 1024 threads: S and rinv of the cell staged in LDS; tile t takes
//            a = 2 + t, 2 + t + T, ... (interleaved: every tile gets long and short b ranges), its waves
//            take every 16th of those, the lanes stride b; a thread keeps its first maximum, the
//            workgroup reduces by (gain, -a, -b) and writes one winner per (cell, tile)
//   reduce   one wave per cell over its tiles' winners, same order
// The order (gain, -a, -b) is total on distinct candidates, so the result does not depend on the
// tiling, needs no atomics and two runs agree bit for bit.

#include "gmm2_stages.h"

// no fused multiply-add anywhere in this file: the gains are compared for exact ties and with the
// numpy twin bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;                   // lanes of a wave

constexpr int kThreads = 1024;             // the search's workgroup: 16 waves, 4 a SIMD
constexpr int kWaves = kThreads / kWave;
constexpr int kTargetGroups = 1024;        // the search's grid, about (four rounds of the 256 CUs)
constexpr int kRedBytes = kWaves * 16;     // the winners of a workgroup's waves

struct Winner {
  double gain;
  int32_t a, b;
};

// (gain, -a, -b) lexicographic: is y ahead of x?  A cell without a candidate holds a = -1, gain = -1.
__device__ __forceinline__ bool ahead(double gy, int ay, int by, double gx, int ax, int bx) {
  if (ay < 0) return false;
  if (ax < 0) return true;
  if (gy != gx) return gy > gx;
  if (ay != ax) return ay < ax;
  return by < bx;
}

__device__ __forceinline__ void wave_best(double& g, int& a, int& b) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double g2 = __shfl_xor(g, off);
    const int a2 = __shfl_xor(a, off);
    const int b2 = __shfl_xor(b, off);
    if (ahead(g2, a2, b2, g, a, b)) {
      g = g2;
      a = a2;
      b = b2;
    }
  }
}

__host__ __device__ inline bool feasible(int n, int mode) { return mode == 2 ? n >= 6 : n >= 4; }

// ---- S[c][0..n]: the prefix sums in bin order
__global__ __launch_bounds__(kWave) void cpd_prefix_kernel(int ld, const double* __restrict__ y,
                                                          const int32_t* __restrict__ len,
                                                          const int32_t* __restrict__ active,
                                                          double* __restrict__ S) {
  __shared__ double buf[kWave];
  const int c = blockIdx.x, lane = threadIdx.x;
  if (!active[c]) return;
  const int n = len[c];
  const double* yc = y + (size_t)c * ld;
  double* Sc = S + (size_t)c * (ld + 1);
  double run = 0.0;
  if (lane == 0) Sc[0] = 0.0;
  for (int i0 = 0; i0 < n; i0 += kWave) {
    const int m = min(kWave, n - i0);
    if (lane < m) buf[lane] = yc[i0 + lane];
    __syncthreads();
    if (lane == 0) {
      for (int i = 0; i < m; ++i) {
        run = run + buf[i];
        buf[i] = run;
      }
    }
    __syncthreads();
    if (lane < m) Sc[i0 + 1 + lane] = buf[lane];
    __syncthreads();
  }
}

// ---- the search of one (cell, tile of a)
__global__ __launch_bounds__(kThreads) void cpd_search_kernel(int ld, int T, const double* __restrict__ S,
                                                               const int32_t* __restrict__ len,
                                                               const int32_t* __restrict__ mode,
                                                               const int32_t* __restrict__ active,
                                                               Winner* __restrict__ tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cpd_lds[];
  const int c = blockIdx.y, t = blockIdx.x;
  if (!active[c]) return;
  const int n = len[c], md = mode[c];
  if (!feasible(n, md)) return;                  // the reduce kernel reports it
  Winner* red = reinterpret_cast<Winner*>(cpd_lds);
  double* s = reinterpret_cast<double*>(cpd_lds + kRedBytes);          // [n + 1]
  double* rinv = s + (n + 1);                                           // [n + 1], entry 0 unused
  const double* Sc = S + (size_t)c * (ld + 1);
  for (int i = threadIdx.x; i <= n; i += kThreads) {
    s[i] = Sc[i];
    rinv[i] = i > 0 ? 1.0 / (double)i : 0.0;
  }
  __syncthreads();

  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const double Sn = s[n];
  double bg = -1.0;
  int ba = -1, bb = -1;
  // a ascending per thread, then b ascending: a strict > keeps the first maximum in (a, b) order
  for (int a = 2 + t + wave * T; a <= n - 2 - (md == 2 ? 2 : 0); a += kWaves * T) {
    const double Sa = s[a];
    const double t1 = (Sa * Sa) * rinv[a];
    if (md == 2) {
      for (int b = a + 2 + lane; b <= n - 2; b += kWave) {
        const double Sb = s[b];
        const double d = Sb - Sa, e = Sn - Sb;
        const double g = (t1 + (d * d) * rinv[b - a]) + (e * e) * rinv[n - b];
        if (g > bg) {
          bg = g;
          ba = a;
          bb = b;
        }
      }
    } else if (lane == 0) {
      const double e = Sn - Sa;
      const double g = t1 + (e * e) * rinv[n - a];
      if (g > bg) {
        bg = g;
        ba = a;
        bb = n;
      }
    }
  }
  wave_best(bg, ba, bb);
  if (lane == 0) red[wave] = Winner{bg, ba, bb};
  __syncthreads();
  if (wave == 0) {
    bg = -1.0, ba = -1, bb = -1;
    if (lane < kWaves) {
      bg = red[lane].gain;
      ba = red[lane].a;
      bb = red[lane].b;
    }
    wave_best(bg, ba, bb);
    if (lane == 0) tiles[(size_t)c * T + t] = Winner{bg, ba, bb};
  }
}

// ---- the cell's winner among its tiles'
__global__ __launch_bounds__(kWave) void cpd_reduce_kernel(int T, const int32_t* __restrict__ len,
                                                          const int32_t* __restrict__ mode,
                                                          const int32_t* __restrict__ active,
                                                          const Winner* __restrict__ tiles, int32_t* __restrict__ a_out,
                                                          int32_t* __restrict__ b_out, double* __restrict__ gain_out) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (!active[c]) return;                        // an inactive cell's outputs are left as they are
  double bg = -1.0;
  int ba = -1, bb = -1;
  if (feasible(len[c], mode[c])) {
    for (int t = lane; t < T; t += kWave) {
      const Winner w = tiles[(size_t)c * T + t];
      if (ahead(w.gain, w.a, w.b, bg, ba, bb)) {
        bg = w.gain;
        ba = w.a;
        bb = w.b;
      }
    }
    wave_best(bg, ba, bb);
  }
  if (lane == 0) {
    a_out[c] = ba;
    b_out[c] = bb;
    gain_out[c] = ba < 0 ? 0.0 : bg;
  }
}

struct Workspace {
  double* S;
  Winner* tiles;
  int32_t *len, *mode, *active;
  int T;
  int64_t bytes;
};

inline bool shape_ok(int32_t N, int32_t ld) {
  return N >= 1 && N <= 65535 && ld >= 1 && ld <= PERT_CPD_MAX_N;
}

// the tiles of a per cell: enough workgroups for the chip from a handful of cells, never more than
// there are values of a
inline int tiles_of(int N, int ld) {
  const int most = ld - 3 > 1 ? ld - 3 : 1;
  const int want = (kTargetGroups + N - 1) / N;
  return want < most ? want : most;
}

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

Workspace carve(void* base, int N, int ld) {
  Workspace w;
  w.T = tiles_of(N, ld);
  char* p = static_cast<char*>(base);
  int64_t off = 0;
  w.S = reinterpret_cast<double*>(p + off);
  off += up16(8 * (int64_t)N * (ld + 1));
  w.tiles = reinterpret_cast<Winner*>(p + off);
  off += up16((int64_t)sizeof(Winner) * N * w.T);
  w.len = reinterpret_cast<int32_t*>(p + off);
  off += up16(4 * (int64_t)N);
  w.mode = reinterpret_cast<int32_t*>(p + off);
  off += up16(4 * (int64_t)N);
  w.active = reinterpret_cast<int32_t*>(p + off);
  off += up16(4 * (int64_t)N);
  w.bytes = off;
  return w;
}

#define CPD_HIP(call)                                            \
  do {                                                           \
    const hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return PERT_E_HIP_BASE + (int)e_;      \
  } while (0)
#define CPD_LAUNCHED()                                           \
  do {                                                           \
    const int s_ = gmm2::launch_status();                        \
    if (s_ != PERT_OK) return s_;                                \
  } while (0)

}  // namespace

extern "C" int pert_cpd_workspace(int32_t N, int32_t ld, int64_t* bytes) {
  if (!bytes || !shape_ok(N, ld)) return PERT_E_ARG;
  *bytes = carve(nullptr, N, ld).bytes;
  return PERT_OK;
}

extern "C" int pert_cpd_search(int32_t N, int32_t ld, const double* y, const int32_t* len, const int32_t* mode,
                               const int32_t* active, int32_t* a, int32_t* b, double* gain, void* workspace,
                               int64_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(N, ld) || !y || !len || !mode || !active || !a || !b || !gain || !workspace) return PERT_E_ARG;
  if (((uintptr_t)workspace & 15u) != 0 || ((uintptr_t)y & 7u) != 0) return PERT_E_ARG;
  const Workspace w = carve(workspace, N, ld);
  if (workspace_bytes < w.bytes) return PERT_E_ARG;
  int n_max = 0, n_active = 0;
  for (int32_t c = 0; c < N; ++c) {
    if (len[c] < 0 || len[c] > ld) return PERT_E_ARG;
    if (mode[c] != 1 && mode[c] != 2) return PERT_E_ARG;
    if (active[c] != 0 && active[c] != 1) return PERT_E_ARG;
    if (active[c]) {
      ++n_active;
      if (len[c] > n_max) n_max = len[c];
    }
  }
  if (n_active == 0) return PERT_OK;

  CPD_HIP(hipMemcpyAsync(w.len, len, 4 * (size_t)N, hipMemcpyHostToDevice, stream));
  CPD_HIP(hipMemcpyAsync(w.mode, mode, 4 * (size_t)N, hipMemcpyHostToDevice, stream));
  CPD_HIP(hipMemcpyAsync(w.active, active, 4 * (size_t)N, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(cpd_prefix_kernel, dim3(N), dim3(kWave), 0, stream, ld, y, w.len, w.active, w.S);
  CPD_LAUNCHED();
  // S and rinv of the longest active cell, and the waves' winners (n_max <= PERT_CPD_MAX_N: within 160 KiB)
  const size_t lds = (size_t)kRedBytes + 16 * ((size_t)n_max + 1);
  if (lds > 64 * 1024)
    CPD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cpd_search_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(cpd_search_kernel, dim3(w.T, N), dim3(kThreads), lds, stream, ld, w.T, w.S, w.len, w.mode,
                     w.active, w.tiles);
  CPD_LAUNCHED();
  hipLaunchKernelGGL(cpd_reduce_kernel, dim3(N), dim3(kWave), 0, stream, w.T, w.len, w.mode, w.active, w.tiles, a, b,
                     gain);
  CPD_LAUNCHED();
  return PERT_OK;
}
