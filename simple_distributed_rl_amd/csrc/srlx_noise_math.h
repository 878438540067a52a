// srlx_noise_math.h -- the Gaussian noise of the NoisyLinear layers (srl/rl/torch_/modules/noisy_linear.py:44-52), one definition for the image Q-network
// (srlx_noisy.hip) and the MLP Q-network (srlx_mlpq.hip): eps(seed, draw, tensor, element) is a pure function of its four keys, so a backward pass
// regenerates the noise of the forward pass it belongs to instead of storing it.
#pragma once

#include "srlx_common.h"

namespace srlx {

// two independent standard normals from one 64-bit draw (Box-Muller on two 24-bit uniforms; u1 in (0, 1])
__device__ __forceinline__ float2 normal_pair(u64 x) {
    const float u1 = (float)((unsigned)(x >> 40) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)((unsigned)(x >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    return make_float2(r * c, r * s);
}

// the normals of elements 2 p and 2 p + 1 of tensor `t` under draw `id` (a tensor of odd length leaves the last pair's second half unused)
__device__ __forceinline__ float2 noisy_eps_pair(u64 seed, u64 id, int t, u64 p) { return normal_pair(rng_u64(seed + 0x9E37ull * (u64)(t + 1), id, p)); }

}  // namespace srlx
