// Counter-based RNG shared bit for bit with ops_ref.crng (NumPy): stream i, draw j ->
// splitmix64(splitmix64((i << 32) | j) ^ seed) >> 32.  No state: every thread computes
// its own draw, so the random image ops and the dropout masks run entirely on the device.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace csa {

__device__ __forceinline__ uint64_t smix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t crng(uint64_t seed, uint64_t i, uint64_t j) {
  return (uint32_t)(smix(smix((i << 32) | j) ^ seed) >> 32);
}

}  // namespace csa
