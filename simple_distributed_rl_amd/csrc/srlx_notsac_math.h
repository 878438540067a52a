// srlx_notsac_math.h -- the per-row closed forms of NoT_SAC's update (srl/algorithms/sac_not/torch_model.py:150-189 and the two distribution blocks it uses:
// srl/rl/torch_/distributions/normal_dist_block.py:52-54, categorical_gumbel_dist_block.py:10-12,45-60).  Inputs and results are float32; every function
// evaluates in float64 and rounds once.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

#include "srlx_mlp_rows.h"
#include "srlx_ppo_math.h"

namespace srlxn {

using srlxm::kHeadCols;  // a row's head outputs, actions and their gradients: 16 logits, or 8 locs at 0.. and 8 log-scales at kNormalLs..
using srlxm::kNormalLs;
using srlxp::clampf;
constexpr double kGumbelEps = 1e-6;

// SiLU and its derivative at the pre-activation z
__device__ __forceinline__ float silu(float z) {
    const double x = (double)z;
    return (float)(x / (1.0 + exp(-x)));
}
__device__ __forceinline__ double silu_grad(float z) {
    const double x = (double)z, s = 1.0 / (1.0 + exp(-x));
    return s * (1.0 + x * (1.0 - s));
}

// -log(-log(u + eps) + eps) of a uniform u in [0, 1)
__device__ __forceinline__ double gumbel(float u) { return -log(-log((double)u + kGumbelEps) + kGumbelEps); }

// One element of the Normal head's action from a standard normal e: loc + exp(clamp(ls)) e, through tanh when squashed.
__device__ __forceinline__ float normal_action(float loc, float ls_raw, float lo, float hi, float e, int squashed) {
    const double x = (double)loc + exp((double)clampf(ls_raw, lo, hi)) * (double)e;
    return (float)(squashed ? tanh(x) : x);
}

// d loss / d (loc, raw log-scale) of that element from d loss / d action = g and the action a it gave: through 1 - a^2 when squashed; the log-scale takes
// g exp(ls) e on the clamp's closed interval and nothing outside it (torch.clamp).
__device__ __forceinline__ void normal_action_grad(float g, float a, float ls_raw, float lo, float hi, float e, int squashed, float &dloc, float &dls) {
    const double gx = squashed ? (double)g * (1.0 - (double)a * (double)a) : (double)g;
    dloc = (float)gx;
    dls = (ls_raw >= lo && ls_raw <= hi) ? (float)(gx * exp((double)ls_raw) * (double)e) : 0.f;
}

// The first maximum of logits + gumbel(u) over A actions: the one-hot next action (a positive temperature divides both sides of every comparison).
__device__ __forceinline__ int gumbel_argmax(const float *z, const float *u, int A) {
    int best = 0;
    double vb = (double)z[0] + gumbel(u[0]);
    for (int k = 1; k < A; k++) {
        const double v = (double)z[k] + gumbel(u[k]);
        if (v > vb) vb = v, best = k;
    }
    return best;
}

// softmax(logits + gumbel(u)) of one row into a[0..A)
__device__ __forceinline__ void gumbel_softmax(const float *z, const float *u, int A, float *a) {
    // (three passes that each form z + gumbel(u) again: a local array indexed by k would live in scratch memory)
    double m = -INFINITY, tot = 0.0;
    for (int k = 0; k < A; k++) {
        const double v = (double)z[k] + gumbel(u[k]);
        m = v > m ? v : m;
    }
    for (int k = 0; k < A; k++) tot += exp((double)z[k] + gumbel(u[k]) - m);
    for (int k = 0; k < A; k++) a[k] = (float)(exp((double)z[k] + gumbel(u[k]) - m) / tot);
}

// The softmax Jacobian: d logits_j = a_j (g_j - sum_i a_i g_i)
__device__ __forceinline__ void softmax_grad(const float *a, const float *g, int A, float *dz) {
    double dot = 0.0;
    for (int k = 0; k < A; k++) dot = fma((double)a[k], (double)g[k], dot);
    for (int k = 0; k < A; k++) dz[k] = (float)((double)a[k] * ((double)g[k] - dot));
}

// One row of the Q step (:160-167): the target, the Huber and MSE terms (the target is the first argument, q takes the gradient) and the seed d loss / d q.
struct QRow {
    float target, huber, align, dq;
};
__device__ __forceinline__ QRow q_row(float q, float n_q, float reward, float not_term, float total, float discount, float coeff, double inv_b) {
    QRow r;
    r.target = reward + (not_term * discount) * n_q;
    const double d = (double)r.target - (double)q, ad = fabs(d);
    r.huber = (float)(ad < 1.0 ? 0.5 * d * d : ad - 0.5);
    const double e = (double)total - (double)q;
    r.align = (float)(e * e);
    const double gh = -(d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d));  // clamp(q - target, -1, 1)
    r.dq = (float)((gh + (double)coeff * (-2.0 * e)) * inv_b);
    return r;
}

}  // namespace srlxn
