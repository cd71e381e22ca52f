// sim_math.h -- the random-number generator and the samplers of the read-count simulator
// (sim_kernels.hip), written so that the host compiles them too (a CPU program can check a
// sampler's distribution without a device).
//
// Generator: Philox4x32-10 (Salmon et al., SC'11), counter based: four output words are a pure
// function of a 128-bit counter and a 64-bit key.  Nothing is carried from draw to draw, so an
// element's random numbers depend only on the seed and on which element it is (the counter
// rule: include/pert_hip.h, "Read-count simulator").
//
// Samplers (torch.distributions.NegativeBinomial.sample is Poisson(Gamma(shape, scale))):
//   Gamma(shape >= 1)  Marsaglia & Tsang (2000), no small-shape boost
//   Poisson(rate < 10) inversion by sequential search, one uniform
//   Poisson(rate >= 10) PTRS, Hoermann (1993) transformed rejection with squeeze; the
//                      log-pmf of its exact test is evaluated in a cancellation-free form
// Every rejection loop runs at most kSimMaxRounds rounds; a lane that uses them up takes the
// rounded mean and is counted, so a sampler bug gives a wrong number, never an endless loop.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SIM_HD __host__ __device__ __forceinline__

namespace pert_sim {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr uint32_t kTagMul = 0x9E3779B9u;    // key[1] = high word of the seed ^ tag * kTagMul
constexpr int kSimMaxRounds = 64;            // rounds of every rejection loop
constexpr uint32_t kRoundPoisson = 64u;      // first draw round of the Poisson sampler
constexpr float kPoissonSwitch = 10.0f;      // inversion below, PTRS from here on (as torch)
constexpr int kInversionMax = 64;            // Poisson(10) has 4e-30 of its mass at and above 64

struct Words {
  uint32_t x, y, z, w;
};

SIM_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

SIM_HD Words philox4x32_10(Words c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
    const uint32_t hi1 = mulhi32(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
    c = Words{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

struct Key {
  uint32_t k0, k1;
};

SIM_HD Key make_key(uint64_t seed, uint32_t tag) {
  return Key{(uint32_t)seed, (uint32_t)(seed >> 32) ^ (tag * kTagMul)};
}

// The words of (bin, global cell, draw round) under a key.
SIM_HD Words draw(Key key, uint32_t bin, uint64_t cell, uint32_t round) {
  return philox4x32_10(Words{bin, (uint32_t)cell, round, (uint32_t)(cell >> 32)}, key.k0, key.k1);
}

// ((w >> 8) + 0.5) 2^-24 rounded to fp32 once (ties to even), then kept below 1: of the 2^24
// values only the last rounds to 1.0, and it becomes 1 - 2^-24.  Strictly inside (0, 1).
SIM_HD float u01(uint32_t w) {
  return fminf(fmaf((float)(w >> 8), 0x1p-24f, 0x1p-25f), 0x1.fffffep-1f);
}

SIM_HD float cospi_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return cospif(x);
#else
  return cosf(3.14159265358979323846f * x);
#endif
}

// Box-Muller, the cosine branch: sqrt(-2 log u1) cos(2 pi u2).
SIM_HD float normal_f(uint32_t w1, uint32_t w2) {
  return sqrtf(-2.0f * logf(u01(w1))) * cospi_f(2.0f * u01(w2));
}

// Gamma(shape, 1), shape >= 1.  first = the words of draw round 0, whose .y .z .w serve attempt
// 0 (.x is the element's Bernoulli word); attempt j > 0 takes .y .z .w of draw round j.
SIM_HD float sample_gamma(float shape, Key key, uint32_t bin, uint64_t cell, Words first, uint32_t& exhausted) {
  const float d = shape - (1.0f / 3.0f);
  const float c = 1.0f / sqrtf(9.0f * d);
  Words w = first;
  for (int j = 0; j < kSimMaxRounds; ++j) {
    if (j > 0) w = draw(key, bin, cell, (uint32_t)j);
    const float x = normal_f(w.y, w.z);
    const float uu = u01(w.w);
    const float t = 1.0f + c * x;
    if (t > 0.0f) {
      const float v = t * t * t, x2 = x * x;
      if (uu < 1.0f - 0.0331f * x2 * x2 || logf(uu) < 0.5f * x2 + d * (1.0f - v + logf(v))) return d * v;
    }
  }
  ++exhausted;
  return shape;
}

// log of the Poisson pmf at integer k >= 0: -rate + k log(rate) - lgamma(k + 1).  For k >= 10,
// Stirling's series with the two large terms merged, (k - rate) - k log1p((k - rate) / rate):
// its terms are O(|k - rate|), not O(k log k), so fp32 keeps about 1e-4 absolute at rate 1e4.
SIM_HD float poisson_logpmf(float k, float rate, float lograte) {
  if (k >= 10.0f) {
    const float dk = k - rate, ik = 1.0f / k, ik2 = ik * ik;
    const float series = ik * (0.0833333333f - ik2 * (0.00277777778f - ik2 * 0.000793650794f));
    return (dk - k * log1pf(dk / rate)) - 0.5f * logf(6.28318530718f * k) - series;
  }
  float fact = 1.0f;
#pragma unroll
  for (int i = 2; i < 10; ++i) fact *= ((float)i <= k) ? (float)i : 1.0f;
  return k * lograte - rate - logf(fact);
}

// Poisson(rate), rate >= 0, as a float holding an integer.  Inversion takes .x of draw round
// kRoundPoisson; PTRS attempt j takes .x and .y of draw round kRoundPoisson + j.
SIM_HD float sample_poisson(float rate, Key key, uint32_t bin, uint64_t cell, uint32_t& exhausted) {
  Words w = draw(key, bin, cell, kRoundPoisson);
  if (rate < kPoissonSwitch) {
    float u = u01(w.x);
    float p = expf(-rate), k = 0.0f;
    // u keeps what is left of it above the cumulated mass; once the pmf falls under fp32's
    // resolution of that remainder (1e-12 is far under it) the search has arrived
    for (int i = 0; i < kInversionMax && u > p && p >= 1e-12f; ++i) {
      u -= p;
      k += 1.0f;
      p *= rate / k;
    }
    return k;
  }
  const float slam = sqrtf(rate), lograte = logf(rate);
  const float b = 0.931f + 2.53f * slam;
  const float a = -0.059f + 0.02483f * b;
  const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f);
  const float vr = 0.9277f - 3.6224f / (b - 2.0f);
  for (int j = 0; j < kSimMaxRounds; ++j) {
    if (j > 0) w = draw(key, bin, cell, kRoundPoisson + (uint32_t)j);
    const float U = u01(w.x) - 0.5f, V = u01(w.y);
    const float us = 0.5f - fabsf(U);
    const float k = floorf((2.0f * a / us + b) * U + rate + 0.43f);
    if (us >= 0.07f && V <= vr) return k;
    if (k < 0.0f || (us < 0.013f && V > us)) continue;
    if (logf(V * inv_alpha / (a / (us * us) + b)) <= poisson_logpmf(k, rate, lograte)) return k;
  }
  ++exhausted;
  return rintf(rate);
}

}  // namespace pert_sim
