// sim_kernels.hip -- gfx950 kernels of the read-count simulator (pert_simulator.py).
//
// Reference: scdna_replication_tools/pert_simulator.py -- model_s (:38-124) with its global
// sites conditioned (simulate_s_cells, :201-249), model_g1 (:128-174, simulate_g_cells
// :252-282).  Per cell: tau ~ Beta(1, 1) (:77) and the GC coefficients
// betas ~ Normal(beta_means[lib], beta_stds[lib]) (:83).  Per (bin, cell): rep ~ Bernoulli(phi)
// (:98-104), chi = cn (1 + rep), delta = max(u chi omega (1 - lamb) / lamb, 1) (:107-122),
// reads ~ NegativeBinomial(delta, probs = lamb) (:124), which torch draws as
// Poisson(Gamma(delta, scale = lamb / (1 - lamb))).  Then reads_norm =
// int64(reads / sum(reads) * num_reads) (:245-247).
//
// Every (bin, cell) is independent, so the reads kernel is one fused pass: a lane owns a
// cell, walks a strided set of bins, and writes 5 to 9 bytes per element against a Philox
// block or more and some dozens of transcendentals -- it is bound by vector ALU issue, not by
// memory.  A cell's column sum is kept in a register and added once per lane with an integer
// atomic, so the sums are exact and do not depend on arrival order.
//
// The random numbers of an element are a function of (seed, bin, global cell, draw round)
// alone (sim_math.h), so a launch over any subset of the cells, with any grid, draws the same
// numbers for them as one launch over all cells.

#include "../../include/pert_hip.h"
#include "sim_math.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

namespace {

using namespace pert_sim;

constexpr int kT = PERT_BLOCK;   // cells per workgroup, one per lane

inline int status_of_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PERT_OK : PERT_E_HIP_BASE + (int)e;
}

// out[i] = the four words of counter (c + i, as a 128-bit integer) under key (k0, k1).
__global__ __launch_bounds__(kT) void sim_raw_kernel(uint32_t k0, uint32_t k1, Words c, int64_t n,
                                                     uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const uint64_t lo = ((uint64_t)c.y << 32 | c.x) + (uint64_t)i;
  const uint64_t hi = ((uint64_t)c.w << 32 | c.z) + (lo < (uint64_t)i ? 1u : 0u);
  const Words w = philox4x32_10(Words{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}, k0, k1);
  *reinterpret_cast<uint4*>(out + 4 * i) = make_uint4(w.x, w.y, w.z, w.w);
}

// Per-cell draws, stream PERT_SIM_TAG_CELLS, bin word 0: draw round 0 word 0 is tau; draw
// round 1 + k words 0, 1 are the Box-Muller pair of beta k.  In fp64: there are N (K1 + 1)
// draws against L N of the reads kernel, and a beta that nearly cancels (mean + std z close
// to 0) keeps its relative accuracy only if z has more digits than the fp32 it is stored in.
__global__ __launch_bounds__(kT) void sim_cells_kernel(int N, int K1, int n_libs, uint64_t cell0, Key key,
                                                       const int32_t* __restrict__ libs,
                                                       const float* __restrict__ beta_means,
                                                       const float* __restrict__ beta_stds, float* __restrict__ tau,
                                                       float* __restrict__ betas) {
  const int n = blockIdx.x * kT + threadIdx.x;
  if (n >= N) return;
  const uint64_t cell = cell0 + (uint64_t)n;
  if (tau) tau[n] = u01(draw(key, 0u, cell, 0u).x);
  int lib = libs[n];
  lib = lib < 0 ? 0 : (lib >= n_libs ? n_libs - 1 : lib);          // keeps the tables in bounds
  for (int k = 0; k < K1; ++k) {
    const Words w = draw(key, 0u, cell, 1u + (uint32_t)k);
    const double u1 = ((double)(w.x >> 8) + 0.5) * 0x1p-24, u2 = ((double)(w.y >> 8) + 0.5) * 0x1p-24;
    const double z = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    betas[(size_t)k * N + n] =
        (float)((double)beta_means[lib * K1 + k] + (double)beta_stds[lib * K1 + k] * z);
  }
}

struct ReadsArgs {
  int L, N, ldn, K1;
  uint64_t cell0;
  Key key;
  const float* cn;
  const float* gc;
  const float* rho;
  const float* tau;
  const float* betas;
  float u_ratio;        // u (1 - lamb) / lamb
  float a;
  float scale;          // lamb / (1 - lamb)
  uint32_t* counts;
  uint8_t* rep;
  float* p_rep;
  unsigned long long* colsum;
  uint32_t* exhausted;
};

// Grid (ldn / 256 cell blocks, bin slices): lane = cell, bins l = blockIdx.y, + gridDim.y, ...
// S_MODE: the S-phase model (tau given); else rep = 0 (model_g1).
template <bool S_MODE>
__global__ __launch_bounds__(kT) void sim_reads_kernel(ReadsArgs p) {
  const int n = blockIdx.x * kT + threadIdx.x;          // < ldn: the grid has ldn / 256 blocks
  if (n >= p.N) {                                       // padding columns [N, ldn) are zero
    for (int l = blockIdx.y; l < p.L; l += gridDim.y) {
      const size_t o = (size_t)l * p.ldn + n;
      p.counts[o] = 0u;
      p.rep[o] = 0;
      if (p.p_rep) p.p_rep[o] = 0.0f;
    }
    return;
  }
  const uint64_t cell = p.cell0 + (uint64_t)n;
  float beta[PERT_MAX_K1];                              // right aligned: leading zeros leave Horner's sum alone
#pragma unroll
  for (int j = 0; j < PERT_MAX_K1; ++j) {
    const int k = j - (PERT_MAX_K1 - p.K1);
    beta[j] = k >= 0 ? p.betas[(size_t)k * p.N + n] : 0.0f;
  }
  const float tau = S_MODE ? p.tau[n] : 0.0f;
  unsigned long long sum = 0ull;
  uint32_t exhausted = 0u;

  for (int l = blockIdx.y; l < p.L; l += gridDim.y) {
    const size_t o = (size_t)l * p.ldn + n;
    const float gc = p.gc[l];
    float poly = 0.0f;                                   // sum_k beta[k] gc^(K - k), Horner
#pragma unroll
    for (int j = 0; j < PERT_MAX_K1; ++j) poly = fmaf(poly, gc, beta[j]);
    const float omega = expf(poly);
    const Words w = draw(p.key, (uint32_t)l, cell, 0u);
    uint32_t r = 0u;
    float phi = 0.0f;
    if (S_MODE) {
      phi = 1.0f / (1.0f + expf(-p.a * (tau - p.rho[l])));
      r = u01(w.x) < phi ? 1u : 0u;
    }
    const float chi = p.cn[o] * (1.0f + (float)r);
    const float delta = fmaxf(p.u_ratio * chi * omega, 1.0f);        // also takes a NaN to 1
    const float rate = sample_gamma(delta, p.key, (uint32_t)l, cell, w, exhausted) * p.scale;
    const float k = sample_poisson(rate, p.key, (uint32_t)l, cell, exhausted);
    const uint32_t count = k >= 4294967040.0f ? 0xFFFFFFFFu : (uint32_t)fmaxf(k, 0.0f);
    sum += count;
    p.counts[o] = count;
    p.rep[o] = (uint8_t)r;
    if (p.p_rep) p.p_rep[o] = phi;
  }
  if (sum != 0ull) atomicAdd(&p.colsum[n], sum);
  if (exhausted != 0u) atomicAdd(p.exhausted, exhausted);
}

// out = float(int64(raw / colsum * num_reads)), the three operations in fp64 as torch's.
__global__ __launch_bounds__(kT) void sim_normalise_kernel(int L, int N, int ldn, double num_reads,
                                                           const uint32_t* __restrict__ counts,
                                                           const unsigned long long* __restrict__ colsum,
                                                           float* __restrict__ out) {
  const int n = blockIdx.x * kT + threadIdx.x;
  const bool live = n < N;
  const double total = live ? (double)colsum[n] : 0.0;
  for (int l = blockIdx.y; l < L; l += gridDim.y) {
    const size_t o = (size_t)l * ldn + n;
    float v = 0.0f;
    if (live && total > 0.0) v = (float)(long long)((double)counts[o] / total * num_reads);
    out[o] = v;
  }
}

inline bool bad_shape(int L, int N, int ldn) { return L < 1 || N < 1 || ldn < N || (ldn % kT) != 0; }

inline dim3 matrix_grid(int L, int ldn) {
  const int gx = ldn / kT;
  const int gy = std::min(L, std::max(1, (4096 + gx - 1) / gx));     // some 16 workgroups per CU
  return dim3(gx, gy);
}

}  // namespace

extern "C" int pert_sim_raw(uint32_t key0, uint32_t key1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                            int64_t n, uint32_t* out, hipStream_t stream) {
  if (n < 1 || n > ((int64_t)1 << 31) || !out || (reinterpret_cast<uintptr_t>(out) % 16) != 0) return PERT_E_ARG;
  hipLaunchKernelGGL(sim_raw_kernel, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, stream, key0, key1,
                     Words{c0, c1, c2, c3}, n, out);
  return status_of_launch();
}

extern "C" int pert_sim_cells(int32_t N, int32_t K1, int32_t n_libs, int64_t cell0, uint64_t seed,
                              const int32_t* libs, const float* beta_means, const float* beta_stds, float* tau,
                              float* betas, hipStream_t stream) {
  if (N < 1 || K1 < 1 || K1 > PERT_MAX_K1 || n_libs < 1 || cell0 < 0 || !libs || !beta_means || !beta_stds || !betas)
    return PERT_E_ARG;
  hipLaunchKernelGGL(sim_cells_kernel, dim3((N + kT - 1) / kT), dim3(kT), 0, stream, N, K1, n_libs, (uint64_t)cell0,
                     make_key(seed, PERT_SIM_TAG_CELLS), libs, beta_means, beta_stds, tau, betas);
  return status_of_launch();
}

extern "C" int pert_sim_reads(int32_t L, int32_t N, int32_t ldn, int32_t K1, int64_t cell0, uint64_t seed,
                              const float* cn, const float* gc, const float* rho, const float* tau,
                              const float* betas, float u, float a, float lamb, uint32_t* counts, uint8_t* rep,
                              float* p_rep, uint64_t* colsum, uint32_t* exhausted, hipStream_t stream) {
  if (bad_shape(L, N, ldn) || K1 < 1 || K1 > PERT_MAX_K1 || cell0 < 0 || !cn || !gc || !betas || !counts || !rep ||
      !colsum || !exhausted || (tau && !rho) || !(lamb > 0.0f && lamb < 1.0f) || !(u >= 0.0f))
    return PERT_E_ARG;
  ReadsArgs p;
  p.L = L, p.N = N, p.ldn = ldn, p.K1 = K1;
  p.cell0 = (uint64_t)cell0;
  p.key = make_key(seed, PERT_SIM_TAG_READS);
  p.cn = cn, p.gc = gc, p.rho = rho, p.tau = tau, p.betas = betas;
  p.u_ratio = (float)((double)u * (1.0 - (double)lamb) / (double)lamb);
  p.a = a;
  p.scale = (float)((double)lamb / (1.0 - (double)lamb));
  p.counts = counts, p.rep = rep, p.p_rep = p_rep;
  p.colsum = reinterpret_cast<unsigned long long*>(colsum);
  p.exhausted = exhausted;
  if (tau)
    hipLaunchKernelGGL(sim_reads_kernel<true>, matrix_grid(L, ldn), dim3(kT), 0, stream, p);
  else
    hipLaunchKernelGGL(sim_reads_kernel<false>, matrix_grid(L, ldn), dim3(kT), 0, stream, p);
  return status_of_launch();
}

extern "C" int pert_sim_normalise(int32_t L, int32_t N, int32_t ldn, double num_reads, const uint32_t* counts,
                                  const uint64_t* colsum, float* reads_norm, hipStream_t stream) {
  if (bad_shape(L, N, ldn) || !counts || !colsum || !reads_norm || !(num_reads >= 0.0) ||
      !(num_reads < 16777216.0))
    return PERT_E_ARG;
  hipLaunchKernelGGL(sim_normalise_kernel, matrix_grid(L, ldn), dim3(kT), 0, stream, L, N, ldn, num_reads, counts,
                     reinterpret_cast<const unsigned long long*>(colsum), reads_norm);
  return status_of_launch();
}
