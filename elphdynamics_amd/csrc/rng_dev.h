// rng_dev.h — the build's counter-based generator (elphdynamics_amd/synth.py), shared by hmc.hip and greens_noise.hip:
// SplitMix64 -> uniform(0,1) -> Box-Muller.  Element i of a batch of n normals uses uniforms i/2 and ceil(n/2) + i/2; even i takes the
// cosine, odd i the sine.  Counter-based: any split of the pairs over threads, on the host or the device, gives the same numbers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

__host__ __device__ inline uint64_t sm64(uint64_t seed, uint64_t idx1) {
    uint64_t z = seed + idx1 * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline double u01(uint64_t seed, uint64_t i) {
    return ((double)(sm64(seed, i + 1) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
