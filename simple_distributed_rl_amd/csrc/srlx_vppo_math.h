// srlx_vppo_math.h -- the per-row arithmetic of V-PPO's update (srl/algorithms/ppo_v/torch_model.py:136-171), shared by the kernels of srlx_vppo.hip.  The
// categorical log-softmax and the Normal constants are srlx_ppo_math.h's (cat_lse, cat_logp, kHalfLog2Pi, clampf): the same arithmetic, one definition.
// Everything here is one row's float32 arithmetic; sums over the batch and over a layer's inputs live in the kernels (float64, rounded once).  DESIGN.md 7o.
//
// One row b with K log-probabilities (K = 1: categorical, K = k: Normal), N = B K, v = v(s_b), q = r + not_terminated discount v(s'_b), adv = q - v:
//   ratio_j = expf(lp_j - old_j)
//   Huber (delta 1) of d = ratio_j q - v: 0.5 d^2 where |d| < 1, |d| - 0.5 elsewhere; v is the TARGET, d huber / d v = -d or -sign(d)
//   align: (ratio_j tr - v)^2, d / d v = -2 (ratio_j tr - v)
//   surrogate: min(ratio_j adv, clamp(ratio_j, lo, hi) adv); torch.minimum halves the gradient between its arguments at a tie and clamp passes it on the
//           closed interval, so inside [lo, hi] (always a tie) d / d ratio = adv; outside, adv where the unclipped product is the smaller one and 0 elsewhere
//   entropy (entropy_weight > 0 only): -expf(lp_j) lp_j per element; loss_e = mean_b sum_j expf(lp_j) lp_j
#pragma once
#include <cmath>

#include "srlx_mlp_rows.h"
#include "srlx_ppo_math.h"

namespace srlxv {

using srlxp::clampf;

using srlxm::kHeadCols;  // columns of a head row in LDS and in the seed table: A logits, or k locs at 0.. and k log-scales at kNormalLs..
using srlxm::kNormalLs;
constexpr float kProbFloor = 1e-7f;  // categorical_dist_block.py:53-54 (written 10e-8)
constexpr double kSquashFloor = 1e-10;  // normal_dist_block.py:20-29

struct Cfg {
    float discount, clip_lo, clip_hi, entropy_w, align_c;
    float inv_n, inv_b;  // 1 / (B K), 1 / B
    float ls_lo, ls_hi;  // the log-scale clamp (-inf / +inf: none)
    int squashed;
};

struct RowSums {
    float huber, align, policy, ent;  // sums over the row's K elements: Huber terms, squared alignment errors, surrogate terms, expf(lp) lp
    float dv;                         // d loss / d v of the row
};

// one element of the value losses; adds its part of d loss / d v (the means' 1 / N and the alignment coefficient included)
__device__ __forceinline__ void value_terms(const Cfg &c, float ratio, float q, float tr, float v, RowSums &s) {
    const float d = ratio * q - v, ad = fabsf(d);
    s.huber += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
    const float dh = ad < 1.f ? -d : (d > 0.f ? -1.f : 1.f);
    const float e = ratio * tr - v;
    s.align += e * e;
    s.dv += c.inv_n * (dh + c.align_c * (-2.f * e));
}

// one element of the policy losses given its log-probability; returns d loss / d lp
__device__ __forceinline__ float policy_terms(const Cfg &c, float lp, float ratio, float adv, RowSums &s) {
    const float rc = clampf(ratio, c.clip_lo, c.clip_hi);
    const float lu = ratio * adv, lc = rc * adv;
    s.policy += fminf(lu, lc);
    const bool inside = ratio >= c.clip_lo && ratio <= c.clip_hi;
    const float g_ratio = (inside || lu < lc) ? adv : 0.f;
    float g = -c.inv_n * g_ratio * ratio;
    if (c.entropy_w > 0.f) {
        const float elp = expf(lp);
        s.ent += elp * lp;
        g += c.entropy_w * c.inv_b * (elp * lp + elp);
    }
    return g;
}

// lp = log(clamp(p_a, 1e-7, 1)) with p = softmax(z), float32: inside the clamp (`pass`) the log-softmax itself, below it log(1e-7).  The update's new_logpi and the
// acting kernel's log-probability are both this function: with unchanged parameters they agree to the bit.
__device__ __forceinline__ float categorical_logp(const float *z, int A, int a, float &m, float &lse, bool &pass) {
    srlxp::cat_lse(z, A, m, lse);
    const float xa = srlxp::cat_logp(z[a], m, lse);
    pass = expf(xa) >= kProbFloor;
    return pass ? xa : logf(kProbFloor);
}

// Categorical row: z [A] logits (LDS) -> lp of action a, the row's sums, d loss / d z_k into dz [A].  Below the clamp lp has no gradient.
__device__ __forceinline__ float categorical_row(const Cfg &c, const float *z, int A, int a, float old_lp, float q, float tr, float v, RowSums &s, float *dz) {
    float m, lse;
    bool pass;
    const float lp = categorical_logp(z, A, a, m, lse, pass);
    const float ratio = expf(lp - old_lp);
    value_terms(c, ratio, q, tr, v, s);
    const float g_lp = policy_terms(c, lp, ratio, q - v, s);
    for (int k = 0; k < A; k++) dz[k] = pass ? g_lp * ((k == a ? 1.f : 0.f) - expf(srlxp::cat_logp(z[k], m, lse))) : 0.f;
    return lp;
}

// the squashing correction of one row, sum_i log(clamp(1 - tanh(a_i)^2, 1e-10, 1)), in float64 (1 - tanh^2 cancels in float32); constant in the parameters
__device__ __forceinline__ float squash_correction(const float *act, int k) {
    double s = 0.0;
    for (int i = 0; i < k; i++) {
        const double th = tanh((double)act[i]);
        const double x = 1.0 - th * th;
        s += log(x < kSquashFloor ? kSquashFloor : (x > 1.0 ? 1.0 : x));
    }
    return (float)s;
}

// One element's Normal log-probability, float32: u = (a - loc) / sd comes back, lp = (-0.5 log 2 pi - ls - 0.5 u^2) - corr, with corr the row's squashing
// correction (0 when plain).  The update's new_logpi and the Normal acting kernel's log-probability are both this function: with unchanged parameters they agree
// to the bit on every element.
__device__ __forceinline__ float normal_logp(float a, float loc, float ls, float sd, float corr, float &u) {
    u = (a - loc) / sd;
    return (-srlxp::kHalfLog2Pi - ls - 0.5f * (u * u)) - corr;
}

// Normal row: z = k locs at 0.. and k raw log-scales at kNormalLs.. (LDS) -> lp [k] (global), the row's sums, the seeds into dz in the same layout
__device__ __forceinline__ void normal_row(const Cfg &c, const float *z, int k, const float *act, const float *old_lp, float q, float tr, float v, RowSums &s,
                                           float *dz, float *lp_out) {
    const float corr = c.squashed ? squash_correction(act, k) : 0.f;
    for (int j = 0; j < k; j++) {
        const float loc = z[j], lsr = z[kNormalLs + j];
        const float ls = clampf(lsr, c.ls_lo, c.ls_hi);
        const float sd = expf(ls);
        float u;
        const float lp = normal_logp(act[j], loc, ls, sd, corr, u);
        lp_out[j] = lp;
        const float ratio = expf(lp - old_lp[j]);
        value_terms(c, ratio, q, tr, v, s);
        const float g_lp = policy_terms(c, lp, ratio, q - v, s);
        dz[j] = g_lp * (u / sd);
        dz[kNormalLs + j] = (lsr >= c.ls_lo && lsr <= c.ls_hi) ? g_lp * (u * u - 1.f) : 0.f;
    }
}

// ---- the Worker's action on the categorical head (srlx_vppo_act; algorithms/ppo_v.py: Worker.policy, discrete branch).  U0, U1 are keyed uniforms
// in [0, 1); everything is float64 and host arithmetic as well, so the mirror of the tests restates it line by line.
__host__ __device__ __forceinline__ bool act_is_random(double u0, double epsilon) { return u0 < epsilon; }  // random.random() < epsilon
__host__ __device__ __forceinline__ int act_uniform_action(double u1, int A) {                             // sample_action()
    const int a = (int)floor(u1 * (double)A);
    return a < A - 1 ? a : A - 1;
}
__host__ __device__ __forceinline__ float act_uniform_logp(int A) { return (float)log(1.0 / (double)A); }
// the softmax weight of one logit beside the row's maximum, and the inverse CDF over the running sums c_0 <= .. <= c_{A-1} of those weights in action order:
// the first k with U1 c_{A-1} < c_k (A - 1 if rounding leaves none).  Categorical.sample in distribution.
__host__ __device__ __forceinline__ double act_weight(float z, float zmax) { return exp((double)z - (double)zmax); }
__host__ __device__ __forceinline__ int act_inverse_cdf(const double *c, int A, double u1) {
    const double thr = u1 * c[A - 1];
    for (int k = 0; k < A; k++)
        if (thr < c[k]) return k;
    return A - 1;
}

// ---- the Worker's action on the Normal head (srlx_vppo_act_normal; algorithms/ppo_v.py: Worker.policy, NpArraySpace branch, training).  Row r of a
// k-element head reads 2 k + 1 keyed uniforms: U0 at (2 k + 1) r, element j's pair at + 1 + 2 j and + 2 + 2 j.  Everything is float64 and host arithmetic as well.
__host__ __device__ __forceinline__ double act_box_muller(double ua, double ub) {  // one standard normal: 1 - Ua is in (0, 1], the log is finite
    return sqrt(-2.0 * log(1.0 - ua)) * cos(6.283185307179586 * ub);
}
// np.random.normal(loc, scale): the value BEFORE tanh, rounded to the float32 the item holds
__host__ __device__ __forceinline__ float act_normal_action(float loc, float sd, double z) { return (float)((double)loc + (double)sd * z); }
// NpArraySpace.rescale_from of tanh(a) (squashed) or of a (plain) from [-1, 1] onto [low, high] in float64, rounded to float32, then sanitize's clip
__host__ __device__ __forceinline__ float act_env_action(float a, float low, float high, int squashed) {
    const double x = squashed ? tanh((double)a) : (double)a;
    const float e = (float)((double)low + (x + 1.0) / 2.0 * ((double)high - (double)low));
    return e < low ? low : (e > high ? high : e);
}

}  // namespace srlxv
