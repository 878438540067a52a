// srlx_ppo_math.h -- the per-sample arithmetic of the PPO path, shared by the one-purpose kernels of srlx_ppo.hip (policy sampling, loss + gradient seeds,
// the Pendulum-shaped environment, the self-resetting CartPole) and the fused network kernels of srlx_ppo_net.hip (whole rollout / whole minibatch in one launch):
// one definition, same bits.  The CartPole step is srlx_mlpq.hip's k_cartpole as well.
// Reference lines: srl/algorithms/ppo/ppo.py:102-169 (compute_train_loss), :316-339 (policy), srl/rl/tf/distributions/normal_dist_block.py:13-20,64-74,144-149,
// srl/rl/tf/distributions/categorical_dist_block.py (CategoricalDist: log_softmax of the logits, sample, mode = argmax).
//
// The categorical head, exactly (tests/ppo_cat_reference.py restates it):
//   log-softmax, float32: m = max_k logit_k; s = sum_k expf(logit_k - m), k ascending from 0.f; lse = logf(s); logp_k = (logit_k - m) - lse.
//   sample: ONE keyed uniform per row, u = u53(rng_u64(seed, counter, row)) (a double in [0, 1)); p_k = expf(logp_k) in float32; cum = 0.f; cum += p_k for k
//           ascending; the action is the first k with (double)cum > u, and n_actions - 1 when no k qualifies (cum may end a few ulp short of 1).
//   deterministic: the first k whose logit equals the maximum (CategoricalDist.mode; torch.argmax).
//   the taken action's log-probability is floored at kLogFloor (ppo.py:324).
//   loss seeds: lp = logp_a (not floored: the graph's log_softmax, ppo.py:117-119), g_lp = policy_lp_terms at K = 1 (entropy term -exp(lp) lp of the taken action
//           only, :166), d loss / d logit_k = g_lp * ((k == a) - p_k).  Unimix is not offered.
//
// The adaptive-KL surrogate (surrogate_type "kl": ppo.py:138-146, :279-287; tests/ppo_kl_reference.py restates it in float64):
//   policy term of an element = ratio * adv - beta * kl, no ratio clip; beta is a float32 in device memory that the update adapts after every minibatch
//           (kl_adapt_beta: kl_mean < target / 1.5 halves it, kl_mean > target * 1.5 doubles it while it is below 10; the comparison in double).
//   categorical (srl/rl/tf/functions.py:86-92): q = clip(old_probs, 1e-10, 1), p = clip(new_probs, 1e-10, 1), kl = sum_k q_k logf(q_k / p_k), k ascending from 0.f;
//           new_probs_k = expf(logp_k) (cat_act_one<true> records the same values as the NEXT update's old_probs).  tf.clip_by_value passes the gradient where
//           1e-10 <= p_k <= 1, bounds included: g_k = -q_k / p_k there and 0 elsewhere, d kl / d logit_j = g_j P_j - P_j sum_k g_k P_k with P the unclipped softmax.
//   Normal (functions.py:95-103: tfp's Normal.kl_divergence, closed form per dimension): kl = (ls2 - ls1) + (exp(2 ls1) + (m1 - m2)^2) * 0.5 * exp(-2 ls2) - 0.5,
//           old mean m1 and old log-scale ls1 as clamped at acting time, new mean m2, ls2 = the new log-scale clamped to the stable-gradient range;
//           d kl / d m2 = (m2 - m1) exp(-2 ls2); d kl / d ls2 = 1 - (exp(2 ls1) + (m1 - m2)^2) exp(-2 ls2), passed to the raw log-scale inside the clamp range only.
#pragma once
#include "srlx_common.h"

namespace srlxp {

using i64 = int64_t;
using u8 = unsigned char;
using u64 = unsigned long long;

constexpr float kHalfLog2Pi = 0.91893853320467274178f;  // 0.5 * log(2 pi)
constexpr float kLogFloor = -13.815510557964274f;      // math.log(1e-6), ppo.py:322

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// action = loc + exp(log_scale) * N(0,1) (Box-Muller on two keyed uniforms); log_prob per dimension, floored at log(1e-6).  i = flat index of (environment, dimension).
// The standard-normal draw depends on (seed, counter, index) only -- a rollout kernel draws all T steps' values up front (normal_z) and applies them per step
// (normal_act_from_z): the same expression, the same bits as normal_act_one.
__device__ __forceinline__ float normal_z(u64 seed, u64 c, i64 i) {
    const double u1 = 1.0 - srlx::u53(srlx::rng_u64(seed, c, (u64)(2 * i)));  // (0, 1]
    const double u2 = srlx::u53(srlx::rng_u64(seed, c, (u64)(2 * i + 1)));
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

__device__ __forceinline__ void normal_act_from_z(float loc, float log_scale, float ls_lo, float ls_hi, float z, int deterministic, float &action, float &logprob) {
    const float ls = clampf(log_scale, ls_lo, ls_hi);  // enable_stable_gradients clip, normal_dist_block.py:144-149
    const float sd = expf(ls);
    float a = loc;
    if (!deterministic) a = loc + sd * z;
    const float q = (a - loc) / sd;
    action = a;
    logprob = fmaxf(-kHalfLog2Pi - ls - 0.5f * (q * q), kLogFloor);
}

__device__ __forceinline__ void normal_act_one(float loc, float log_scale, float ls_lo, float ls_hi, u64 seed, u64 c, i64 i, int deterministic, float &action, float &logprob) {
    normal_act_from_z(loc, log_scale, ls_lo, ls_hi, deterministic ? 0.f : normal_z(seed, c, i), deterministic, action, logprob);
}

struct LossCfg {
    float ls_lo, ls_hi;
    int baseline_advantage, surrogate_clip, value_clip;
    float policy_clip, value_clip_range, value_w, entropy_w;
    float inv_b, inv_bk;  // 1 / B, 1 / (B * K)
};

// One (sample, dimension) of the policy loss given the log-probability lp of the taken action: surrogate term, entropy term, d loss / d lp
__device__ __forceinline__ float policy_lp_terms(const LossCfg &a, float lp, float old_lp, float adv, float &term, float &ent) {
    const float ratio = expf(lp - old_lp);  // :126
    float g_ratio;                          // d policy_term / d ratio
    if (a.surrogate_clip) {                 // :127-137
        const float rc = clampf(ratio, 1.0f - a.policy_clip, 1.0f + a.policy_clip);
        const float lu = ratio * adv, lc = rc * adv;
        term = fminf(lu, lc);
        g_ratio = lu <= lc ? adv : 0.f;  // tf.minimum routes the gradient to its first argument on ties
    } else {  // surrogate_type == "" (:148-149)
        term = ratio * adv;
        g_ratio = adv;
    }
    const float elp = expf(lp);
    ent = -elp * lp;  // :166
    // d loss / d lp: policy (-mean over B*K), entropy (weight * -mean over B of the per-sample sum)
    return -a.inv_bk * g_ratio * ratio + a.entropy_w * a.inv_b * (elp * lp + elp);
}

// Normal head: log-probability of `action` and the seeds d loss / d loc, d loss / d log_scale
__device__ __forceinline__ void policy_normal(const LossCfg &a, float loc, float ls_raw, float action, float old_lp, float adv, float &term, float &ent, float &d_loc, float &d_ls) {
    const float ls = clampf(ls_raw, a.ls_lo, a.ls_hi);
    const float q = (action - loc) / expf(ls);
    const float lp = -kHalfLog2Pi - ls - 0.5f * (q * q);  // normal_dist_block.py:13-20
    const float g_lp = policy_lp_terms(a, lp, old_lp, adv, term, ent);
    const bool pass = ls_raw >= a.ls_lo && ls_raw <= a.ls_hi;  // clip_by_value passes the gradient inside the range
    d_loc = g_lp * (q / expf(clampf(ls_raw, a.ls_lo, a.ls_hi)));
    d_ls = pass ? g_lp * (q * q - 1.0f) : 0.f;
}

// ---- the adaptive-KL surrogate (the head comment has the formulas) ------------------------------------------------------------------------------------------
constexpr float kKlProbFloor = 1e-10f;  // functions.py:88-89

// beta after one minibatch whose mean KL is kl_mean; lo = target / 1.5, hi = target * 1.5 (formed on the host, in double).  Halving and doubling are exact in float32
// as long as beta stays a normal number, so the halving stops at the smallest one (1.18e-38: 125 consecutive halvings from 0.5): below it the reference's Python
// float goes on halving (with no effect on a float32 loss: beta * kl is gone long before), but a float32 would lose bits and then reach 0, from which no doubling
// returns -- measured: 16 updates per iteration on a KL far below the target put it there within ten iterations.
constexpr float kKlBetaMin = 1.17549435e-38f;  // FLT_MIN
__device__ __forceinline__ float kl_adapt_beta(float beta, float kl_mean, double lo, double hi) {
    if ((double)kl_mean < lo) return beta * 0.5f >= kKlBetaMin ? beta * 0.5f : beta;
    if ((double)kl_mean > hi && beta < 10.0f) return beta * 2.0f;
    return beta;
}

// Normal head, one (sample, dimension): KL(old || new) and its derivatives at the new mean and the new CLAMPED log-scale
__device__ __forceinline__ float kl_normal(float m1, float ls1, float m2, float ls2, float &d_m2, float &d_ls2) {
    const float e = expf(-2.0f * ls2), dm = m1 - m2;
    const float s = expf(2.0f * ls1) + dm * dm;
    d_m2 = (m2 - m1) * e;
    d_ls2 = 1.0f - s * e;
    return (ls2 - ls1) + s * 0.5f * e - 0.5f;
}

// policy_normal under the "kl" surrogate (a.surrogate_clip == 0): term = ratio * adv - beta * kl, the seeds gain beta * inv_bk * d kl
__device__ __forceinline__ void policy_normal_kl(const LossCfg &a, float beta, float loc, float ls_raw, float action, float old_lp, float old_loc, float old_ls, float adv, float &term,
                                                 float &ent, float &kl, float &d_loc, float &d_ls) {
    policy_normal(a, loc, ls_raw, action, old_lp, adv, term, ent, d_loc, d_ls);
    float k_m, k_ls;
    kl = kl_normal(old_loc, old_ls, loc, clampf(ls_raw, a.ls_lo, a.ls_hi), k_m, k_ls);
    const bool pass = ls_raw >= a.ls_lo && ls_raw <= a.ls_hi;
    term -= beta * kl;
    d_loc += beta * a.inv_bk * k_m;
    d_ls += pass ? beta * a.inv_bk * k_ls : 0.f;
}

// value loss :152-158: returns the summand, g_v = d loss / d v
__device__ __forceinline__ float value_term(const LossCfg &a, float v, float vt, float ov, float &g_v) {
    const float e1 = v - vt;
    float s, g;
    if (a.value_clip) {
        const float vc = clampf(v, ov - a.value_clip_range, ov + a.value_clip_range);
        const float e2 = vc - vt;
        const float l1 = e1 * e1, l2 = e2 * e2;
        s = fmaxf(l1, l2);
        // tf.maximum routes the gradient to its first argument on ties; the clipped branch only inside the range
        g = l1 >= l2 ? 2.0f * e1 : ((v >= ov - a.value_clip_range && v <= ov + a.value_clip_range) ? 2.0f * e2 : 0.f);
    } else {
        s = e1 * e1;
        g = 2.0f * e1;
    }
    g_v = a.value_w * a.inv_b * g;
    return s;
}

// Pendulum dynamics (the classic-control task config 5 is shaped on): th'' = 3g/(2l) sin th + 3/(m l^2) u; time limit = truncation with auto-reset
__device__ __forceinline__ void pendulum_one(float &th, float &thd, int &t, float action, i64 episode_len, u64 seed, u64 c, i64 e, float &o0, float &o1, float &o2, float &reward,
                                             u8 &done) {
    const float g = 10.0f, m = 1.0f, l = 1.0f, dt = 0.05f, max_speed = 8.0f, max_torque = 2.0f;
    const float u = clampf(action, -max_torque, max_torque);
    const float pi = 3.14159265358979323846f;
    float an = fmodf(th + pi, 2.0f * pi);
    if (an < 0.f) an += 2.0f * pi;
    an -= pi;  // angle_normalize
    reward = -(an * an + 0.1f * thd * thd + 0.001f * u * u);
    thd = clampf(thd + (3.0f * g / (2.0f * l) * sinf(th) + 3.0f / (m * l * l) * u) * dt, -max_speed, max_speed);
    th = th + thd * dt;
    t = t + 1;
    const bool end = t >= episode_len;  // a time limit: truncation, not termination
    done = end ? 1 : 0;
    if (end) {  // auto-reset: th ~ U(-pi, pi), thdot ~ U(-1, 1)
        th = (float)((2.0 * srlx::u53(srlx::rng_u64(seed ^ 0x70656e64ull, c, (u64)(2 * e))) - 1.0) * 3.14159265358979323846);
        thd = (float)(2.0 * srlx::u53(srlx::rng_u64(seed ^ 0x70656e64ull, c, (u64)(2 * e + 1))) - 1.0);
        t = 0;
    }
    o0 = cosf(th);
    o1 = sinf(th);
    o2 = thd;
}

// ---- categorical head ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int kCatMax = 8;  // n_actions the fused network covers (its heads table has 8 policy slots per row)

__device__ __forceinline__ void cat_lse(const float *__restrict__ logits, int n, float &m, float &lse) {
    m = logits[0];
    for (int k = 1; k < n; k++) m = fmaxf(m, logits[k]);
    float s = 0.f;
    for (int k = 0; k < n; k++) s += expf(logits[k] - m);
    lse = logf(s);
}
__device__ __forceinline__ float cat_logp(float logit, float m, float lse) { return (logit - m) - lse; }

// logits [n] (memory: global or LDS) -> action + its log-probability; row = the index the uniform is keyed with.
// PROBS: probs [n] also receives the probabilities the sampler sums (what the "kl" surrogate records as old_probs); false: the function as it was
template <bool PROBS = false>
__device__ __forceinline__ void cat_act_one(const float *__restrict__ logits, int n, u64 seed, u64 c, i64 row, int deterministic, int &action, float &logprob,
                                            float *__restrict__ probs = nullptr) {
    float m, lse;
    cat_lse(logits, n, m, lse);
    int a;
    if (deterministic) {
        a = 0;
        for (int k = n - 1; k >= 0; k--)
            if (logits[k] == m) a = k;  // the first maximum
        if constexpr (PROBS) {
            for (int k = 0; k < n; k++) probs[k] = expf(cat_logp(logits[k], m, lse));
        }
    } else {
        const double u = srlx::u53(srlx::rng_u64(seed, c, (u64)row));
        a = n - 1;
        float cum = 0.f;
        bool found = false;
        for (int k = 0; k < n; k++) {
            const float p = expf(cat_logp(logits[k], m, lse));
            if constexpr (PROBS) probs[k] = p;
            cum += p;
            if (!found && (double)cum > u) a = k, found = true;
        }
    }
    action = a;
    logprob = fmaxf(cat_logp(logits[a], m, lse), kLogFloor);
}

// Categorical head: log-probability of `action` and the seeds d loss / d logit_k (fixed extent kCatMax, zero beyond n: no run-time register index)
__device__ __forceinline__ void policy_categorical(const LossCfg &a, const float *__restrict__ logits, int n, int action, float old_lp, float adv, float &term, float &ent,
                                                   float (&d_logit)[kCatMax]) {
    float m, lse;
    cat_lse(logits, n, m, lse);
    const float lp = cat_logp(logits[action], m, lse);
    const float g_lp = policy_lp_terms(a, lp, old_lp, adv, term, ent);
#pragma unroll
    for (int k = 0; k < kCatMax; k++) d_logit[k] = k < n ? g_lp * ((k == action ? 1.0f : 0.0f) - expf(cat_logp(logits[k], m, lse))) : 0.f;
}

// policy_categorical under the "kl" surrogate (a.surrogate_clip == 0): term = ratio * adv - beta * kl, the seeds gain beta * inv_b * d kl / d logit
__device__ __forceinline__ void policy_categorical_kl(const LossCfg &a, float beta, const float *__restrict__ logits, int n, int action, float old_lp, const float *__restrict__ old_probs,
                                                      float adv, float &term, float &ent, float &kl, float (&d_logit)[kCatMax]) {
    float m, lse;
    cat_lse(logits, n, m, lse);
    const float lp = cat_logp(logits[action], m, lse);
    const float g_lp = policy_lp_terms(a, lp, old_lp, adv, term, ent);
    float P[kCatMax], g[kCatMax], s_kl = 0.f, s_gp = 0.f;
#pragma unroll
    for (int k = 0; k < kCatMax; k++) {
        P[k] = 0.f, g[k] = 0.f;
        if (k < n) {
            P[k] = expf(cat_logp(logits[k], m, lse));
            const float q = clampf(old_probs[k], kKlProbFloor, 1.0f), p = clampf(P[k], kKlProbFloor, 1.0f);
            s_kl += q * logf(q / p);
            g[k] = (P[k] >= kKlProbFloor && P[k] <= 1.0f) ? -q / p : 0.f;
            s_gp = fmaf(g[k], P[k], s_gp);
        }
    }
    kl = s_kl;
    term -= beta * kl;
    const float w = beta * a.inv_b;
#pragma unroll
    for (int k = 0; k < kCatMax; k++) d_logit[k] = k < n ? g_lp * ((k == action ? 1.0f : 0.0f) - P[k]) + w * (g[k] * P[k] - P[k] * s_gp) : 0.f;
}

// ---- CartPole (envs/cartpole.py), float64 state x, x_dot, theta, theta_dot ------------------------------------------------------------------------------------
constexpr double kCpGravity = 9.8, kCpMassCart = 1.0, kCpMassPole = 0.1, kCpHalfLength = 0.5, kCpForce = 10.0, kCpTau = 0.02;
constexpr double kCpPi = 3.141592653589793;

// the lane's next episode: uniform in [-0.05, 0.05]^4 from (seed, lane, episode of the lane); the episode count advances, the step count restarts
__device__ __forceinline__ void cartpole_reset(double (&s)[4], int &steps, int &episode, u64 seed, i64 lane) {
    const u64 key = (u64)lane * 0x100000000ull + (u64)(uint32_t)episode;
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = -0.05 + 0.1 * srlx::u53(srlx::rng_u64(seed ^ 0xCA27901Eull, key, (u64)k));
    episode += 1;
    steps = 0;
}

// one explicit-Euler step (envs/cartpole.py:step): action 1 pushes right, anything else left
__device__ __forceinline__ void cartpole_dynamics(double (&s)[4], int &steps, int action, i64 max_steps, bool &terminated, bool &truncated) {
    const double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
    const double force = action == 1 ? kCpForce : -kCpForce;
    const double cos_t = cos(theta), sin_t = sin(theta);
    const double total_mass = kCpMassCart + kCpMassPole, pole_ml = kCpMassPole * kCpHalfLength;
    const double temp = (force + pole_ml * theta_dot * theta_dot * sin_t) / total_mass;
    const double theta_acc = (kCpGravity * sin_t - cos_t * temp) / (kCpHalfLength * (4.0 / 3.0 - kCpMassPole * cos_t * cos_t / total_mass));
    const double x_acc = temp - pole_ml * theta_acc * cos_t / total_mass;
    const double nx = x + kCpTau * x_dot, nx_dot = x_dot + kCpTau * x_acc;
    const double nth = theta + kCpTau * theta_dot, nth_dot = theta_dot + kCpTau * theta_acc;
    s[0] = nx, s[1] = nx_dot, s[2] = nth, s[3] = nth_dot;
    steps += 1;
    const double theta_limit = 12 * 2 * kCpPi / 360, x_limit = 2.4;
    terminated = nx < -x_limit || nx > x_limit || nth < -theta_limit || nth > theta_limit;
    truncated = !terminated && steps >= max_steps;
}

// step + auto-reset, as pendulum_one: the call that ends an episode (termination or the step limit) returns that step's reward and done = 1, and the NEXT
// episode's first observation
__device__ __forceinline__ void cartpole_one(double (&s)[4], int &steps, int &episode, int action, i64 max_steps, u64 seed, i64 lane, float (&obs)[4], float &reward, u8 &done) {
    bool term, trunc;
    cartpole_dynamics(s, steps, action, max_steps, term, trunc);
    reward = 1.f;
    done = (term || trunc) ? 1 : 0;
    if (done) cartpole_reset(s, steps, episode, seed, lane);
#pragma unroll
    for (int k = 0; k < 4; k++) obs[k] = (float)s[k];
}

}  // namespace srlxp
