// srlx_sacd_math.h -- the closed forms of the discrete soft actor-critic update (srl/algorithms/sac/sac_tf_discrete.py:158-243), written once
// for the kernels of srlx_sacd.hip.  The update's forms are all float32, every sum over the A <= 16 actions in action order; the acting pass's forms at the end
//  are float64.  The library is built with -ffp-contract=off: a fused
// multiply-add is written fmaf where one is meant, everything else rounds after every operation.
#pragma once
#include <hip/hip_runtime.h>

namespace srlxs {

constexpr int kMaxActions = 16;
constexpr float kClipLo = 1e-7f;  // the reference writes 10e-8 (:44)

// z - logsumexp(z): finite for any finite logits (the stated departure: the reference takes log(softmax(z)), -inf once a probability underflows)
__device__ __forceinline__ void log_softmax(const float *z, int A, float *logp) {
    float mx = z[0];
    for (int a = 1; a < A; a++) mx = z[a] > mx ? z[a] : mx;
    float s = 0.f;
    for (int a = 0; a < A; a++) s += expf(z[a] - mx);
    const float lse = mx + logf(s);
    for (int a = 0; a < A; a++) logp[a] = z[a] - lse;
}

__device__ __forceinline__ void softmax(const float *z, int A, float *p) {
    float mx = z[0];
    for (int a = 1; a < A; a++) mx = z[a] > mx ? z[a] : mx;
    float s = 0.f;
    for (int a = 0; a < A; a++) {
        p[a] = expf(z[a] - mx);
        s += p[a];
    }
    for (int a = 0; a < A; a++) p[a] = p[a] / s;
}

// :179-191: y = r + (1 - done) * discount * sum_a p'[a] (qmin'[a] - alpha logp'[a])
// (`logp`: A floats of the caller's, as every row array here: a private array indexed by a run-time action number would live in scratch memory)
__device__ __forceinline__ float soft_target(const float *z_next, const float *qmin_next, int A, float alpha, float reward, float done, float discount, float *logp) {
    log_softmax(z_next, A, logp);
    float v = 0.f;
    for (int a = 0; a < A; a++) v += expf(logp[a]) * (qmin_next[a] - alpha * logp[a]);
    return reward + ((1.f - done) * discount) * v;
}

// :41-51 for one row: p = softmax(z), L = log(clip(p, 1e-7, 1)), entropy = -sum p L, loss = sum p (alpha L - qv), and d (loss / B) / d z.  With
// c[a] = d loss / d p[a] = (alpha L[a] - qv[a]) + alpha [p[a] inside the clip] (the clip passes no gradient where it is active), the softmax gives
// d loss / d z[j] = p[j] (c[j] - sum_a p[a] c[a]).
__device__ __forceinline__ void policy_row(const float *z, const float *qv, int A, float alpha, float inv_batch, float *entropy, float *loss, float *dz, float *p,
                                           float *c) {
    softmax(z, A, p);
    float ent = 0.f, ls = 0.f, pc = 0.f;
    for (int a = 0; a < A; a++) {
        const bool inside = p[a] >= kClipLo;  // (p <= 1 always)
        const float L = logf(inside ? p[a] : kClipLo);
        const float e = alpha * L - qv[a];
        ent += p[a] * L;
        ls += p[a] * e;
        c[a] = inside ? e + alpha : e;
        pc += p[a] * c[a];
    }
    *entropy = -ent;
    *loss = ls;
    for (int a = 0; a < A; a++) dz[a] = (p[a] * (c[a] - pc)) * inv_batch;
}

// helper.model_soft_sync per element: (1 - tau) is rounded to float32 from double by the caller; two products and one add
__device__ __forceinline__ float soft_sync(float target, float online, float one_minus_tau, float tau) { return one_minus_tau * target + tau * online; }

// ---- the Worker's action (srlx_sacd_act).  All float64, as numpy computes algorithms/sac.py:gumbel_max_sample; U is a keyed uniform in [0, 1).
// Host-compilable: nothing here needs a device.

// rng.uniform(1e-6, 1.0): low + (high - low) * U, the product and the sum rounded separately
__host__ __device__ __forceinline__ double gumbel_uniform(double U) { return 1e-6 + (1.0 - 1e-6) * U; }

// logits - log(-log(u)) for one action: the logit is exact in float64
__host__ __device__ __forceinline__ double gumbel_score(float z, double u) { return (double)z - log(-log(u)); }

// np.argmax: the FIRST maximum
__host__ __device__ __forceinline__ int first_argmax(const double *score, int A) {
    int best = 0;
    for (int a = 1; a < A; a++) best = score[a] > score[best] ? a : best;
    return best;
}

// the Worker's sample_action() while start_steps last: uniform over the A actions from one uniform
__host__ __device__ __forceinline__ int random_action(double U, int A) {
    const int a = (int)floor(U * (double)A);
    return a < A - 1 ? a : A - 1;
}

}  // namespace srlxs
