// kernels_rng.h — the counter-based generator of the resampling and simulation kernels (kernels_rell.h, kernels_simulate.h): the
// SplitMix64 finaliser and the stream of a (seed, replicate, gene).  Written out in kernels_rell.h; no state lives anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace paml_amd {

#define RELL_GAMMA 0x9E3779B97F4A7C15ULL

__host__ __device__ __forceinline__ unsigned long long rell_mix(unsigned long long z)
{
   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ULL;
   z = (z ^ z >> 27) * 0x94D049BB133111EBULL;
   return z ^ z >> 31;
}

__host__ __device__ __forceinline__ unsigned long long rell_stream(unsigned long long seed, unsigned r, unsigned g)
{
   return rell_mix(seed + RELL_GAMMA * ((((unsigned long long)r << 32) | g) + 1ULL));
}

}  // namespace paml_amd
