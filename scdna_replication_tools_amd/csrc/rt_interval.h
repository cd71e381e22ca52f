// rt_interval.h -- the interval decision of the time-from-scheduled-replication histograms,
// shared by rt_kernels.hip (pert_rt_tfs_hist) and boot_kernels.hip (pert_boot_tfs_hist) so that
// both place every t by the same comparisons against the edge table.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace pert_rt {

constexpr int kEdgeSlots = 264;         // LDS slots of the edge table (>= 257, keeps what follows 16-byte aligned)

// Where the comparisons start: the scaled offset of t, clamped into [0, nb - 1] (NaN gives 0).
template <typename T>
__device__ __forceinline__ int guess_interval(T t, int nb, T e0, float inv_width) {
  float q = (float)(t - e0) * inv_width;
  q = fminf(fmaxf(q, 0.0f), (float)(nb - 1));           // fmaxf(NaN, 0) = 0
  return (int)q;
}

// The interval i with edges[i] <= t < edges[i + 1], or -1 (t outside the edges, or NaN), walking
// from interval i in [0, nb - 1]: the answer comes from comparisons against the edges alone.
template <typename T>
__device__ __forceinline__ int walk_interval(T t, int i, const T* s_edges, int nb) {
  while (i > 0 && t < s_edges[i]) --i;
  while (i < nb - 1 && t >= s_edges[i + 1]) ++i;
  return (t >= s_edges[i] && t < s_edges[i + 1]) ? i : -1;
}

template <typename T>
__device__ __forceinline__ int find_interval(T t, const T* s_edges, int nb, T e0, float inv_width) {
  return walk_interval<T>(t, guess_interval<T>(t, nb, e0, inv_width), s_edges, nb);
}

// walk_interval with the two edges of the start interval already loaded (lo = edges[i],
// hi = edges[i + 1]): when they hold t the walk would not move and would return i.  Lets a
// caller issue the edge loads of several decisions before the first comparison.
template <typename T>
__device__ __forceinline__ int settle_interval(T t, int i, T lo, T hi, const T* s_edges, int nb) {
  return (t >= lo && t < hi) ? i : walk_interval<T>(t, i, s_edges, nb);
}

}  // namespace pert_rt
