// Counter-based generator of the stochastic structure sampler
// (fold_sample.hip): draw number `draw` of sample `sample` of sequence `seq`
// under `seed` is a pure function of those four keys, so a sampled structure
// does not depend on wave scheduling, on how a call is split into batches or
// on how many samples were asked for.  Host and device run the same code
// (sk_fold_sample_uniform is the host entry).
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define SK_RNG_HD __host__ __device__
#else
#define SK_RNG_HD
#endif

namespace sk {

// splitmix64's output function (Steele, Lea, Flood 2014): a bijection of 64 bits
SK_RNG_HD inline uint64_t rng_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

constexpr uint64_t kRngGamma = 0x9e3779b97f4a7c15ull;

// the stream of one (seed, sequence, sample): distinct (seq, sample) give
// distinct keys under one seed (rng_mix is a bijection)
SK_RNG_HD inline uint64_t rng_stream(uint64_t seed, int32_t seq, int32_t sample) {
  const uint64_t k = rng_mix(seed + kRngGamma);
  return rng_mix(k ^ ((uint64_t)(uint32_t)seq << 32 | (uint64_t)(uint32_t)sample));
}

// uniform double in [0, 1) with 53 bits: draw number `draw` of a stream
SK_RNG_HD inline double rng_uniform(uint64_t stream, int32_t draw) {
  const uint64_t x = rng_mix(stream + kRngGamma * ((uint64_t)(uint32_t)draw + 1));
  return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace sk
