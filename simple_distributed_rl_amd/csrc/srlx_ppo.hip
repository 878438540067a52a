// srlx_ppo.hip -- PPO on the vectorised path (BASELINE config 5):
//   srlx_ppo_normal_act   : Normal policy head -> action sample + log-probability for E environments in one
//                           launch (srl/algorithms/ppo/ppo.py:316-339, srl/rl/tf/distributions/normal_dist_block.py:13-20,64-74)
//   srlx_ppo_loss_normal  : the whole of compute_train_loss (ppo.py:102-169) for a Normal policy, forward AND the
//                           gradient seeds d loss / d (loc, log_scale, v) in one launch; the host backpropagates the
//                           seeds through the network (same scheme as the Huber seed of the DQN family)
//   srlx_ppo_loss_logpi   : the same for an arbitrary policy head given its log-probabilities (Categorical):
//                           seeds d loss / d (new_logpi, v)
//   srlx_pendulum_step    : the Pendulum-shaped synthetic workload of BASELINE config 5 (obs (cos, sin, thdot),
//                           one torque) for E lock-stepped environments
//   srlx_ppo_categorical_act     : Categorical policy head -> action sample + its log-probability, one keyed uniform per row
//                                  (ppo.py:316-324, CategoricalDist.sample / mode)
//   srlx_cartpole_autoreset_step : CartPole (envs/cartpole.py:step) that starts its next episode in the call that ends one, like
//                                  srlx_pendulum_step -- the discrete-action workload of the PPO engine
//   srlx_ppo_loss_categorical_kl / srlx_ppo_loss_normal_kl : compute_train_loss under surrogate_type "kl" (ppo.py:138-146): the KL term against the recorded old
//                                  distribution, its gradient in the seeds, and the adaptation of beta (:279-287) in device memory, one launch
//   srlx_ppo_categorical_act_dist / srlx_ppo_normal_act_dist : the two samplers, which also write the acting distribution the "kl" surrogate compares with
// The reference module imports TensorFlow and cannot be imported in the build container: these follow the source
// lines only (parity UNPINNED, like srlx_gae_scan); tests check them against oracle/hot_path_oracle.py and
// against torch autograd of the same formula.
// All of them are tiny elementwise/reduction kernels (B x action_dim floats): their point is launch count --
// one launch instead of ~40 framework kernels per minibatch.
#include "srlx_common.h"
#include "srlx_ppo_math.h"

namespace {

using i64 = int64_t;
using u8 = unsigned char;
using srlxp::LossCfg;

__device__ __forceinline__ float block_sum(float v, float *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(256) k_normal_act(i64 n, const float *loc, const float *log_scale, float ls_lo, float ls_hi, unsigned long long seed,
                                                    const i64 *counter, int deterministic, float *action, float *logprob) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    srlxp::normal_act_one(loc[i], log_scale[i], ls_lo, ls_hi, seed, deterministic ? 0ull : (unsigned long long)counter[0], i, deterministic, action[i], logprob[i]);
}

struct PpoArgs {
    i64 B;
    int K;  // action dimensions (log-probabilities per sample)
    const float *loc, *log_scale, *action;  // normal variant
    const float *new_logpi;                 // logpi variant
    const float *old_logpi, *advantage, *v, *v_target, *old_v;
    float ls_lo, ls_hi;
    int baseline_advantage, surrogate_clip, value_clip;
    float policy_clip, value_clip_range, value_w, entropy_w;
    float *losses;  // [3] policy, value, entropy (weighted, as the reference reports them)
    float *d_loc, *d_log_scale, *d_logpi, *d_v;
};

// One workgroup per launch slice; partial sums are accumulated with float atomics into losses[] (zeroed by the host
// side memset) -- the three scalars are reporting values, the gradient seeds do not depend on them.
template <bool NORMAL>
__global__ void __launch_bounds__(256) k_ppo_loss(PpoArgs a) {
    __shared__ float red[256];
    LossCfg c{a.ls_lo, a.ls_hi, a.baseline_advantage, a.surrogate_clip, a.value_clip, a.policy_clip, a.value_clip_range, a.value_w, a.entropy_w,
              1.0f / (float)a.B, 1.0f / (float)(a.B * a.K)};
    float s_pol = 0.f, s_val = 0.f, s_ent = 0.f;
    for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += (i64)gridDim.x * blockDim.x) {
        const float v = a.v[b], vt = a.v_target[b];
        const float adv = a.baseline_advantage ? a.advantage[b] - v : a.advantage[b];  // ppo.py:121-122 (v is a stop_gradient there)
        float ent = 0.f;
        for (int k = 0; k < a.K; k++) {
            const i64 i = b * a.K + k;
            float term, e1;
            if (NORMAL)
                srlxp::policy_normal(c, a.loc[i], a.log_scale[i], a.action[i], a.old_logpi[i], adv, term, e1, a.d_loc[i], a.d_log_scale[i]);
            else
                a.d_logpi[i] = srlxp::policy_lp_terms(c, a.new_logpi[i], a.old_logpi[i], adv, term, e1);
            s_pol += term;
            ent += e1;
        }
        s_ent += ent;
        float g_v;
        s_val += srlxp::value_term(c, v, vt, a.value_clip ? a.old_v[b] : 0.f, g_v);
        a.d_v[b] = g_v;
    }
    const float p = block_sum(s_pol, red), vl = block_sum(s_val, red), en = block_sum(s_ent, red);
    if (threadIdx.x == 0) {
        atomicAdd(&a.losses[0], -c.inv_bk * p);
        atomicAdd(&a.losses[1], a.value_w * c.inv_b * vl);
        atomicAdd(&a.losses[2], a.entropy_w * -c.inv_b * en);
    }
}

// The "kl" surrogate.  ONE workgroup of 1024 threads walks the batch: the sums meet in a fixed tree (deterministic, no atomics), and the thread that forms kl_mean
// adapts beta behind every other thread's read of it -- no second launch, no counter.  losses [5]: policy, value, entropy, kl_mean, beta as adapted.
struct KlLossArgs {
    i64 B;
    int K;                                           // NORMAL: action dimensions; else the number of actions (<= kCatMax)
    const float *loc, *log_scale, *action;           // NORMAL: loc = [B][K]; else loc = the logits [B][K]
    const int32_t *action_index;                     // categorical: [B]
    const float *old_logpi, *old0, *old1;            // NORMAL: old loc, old clamped log_scale [B][K]; else old0 = old probs [B][K]
    const float *advantage, *v, *v_target, *old_v;
    LossCfg cfg;
    double kl_lo, kl_hi;  // target / 1.5, target * 1.5
    float *beta, *losses, *d_loc, *d_log_scale, *d_v;
};

__device__ __forceinline__ float block_sum_kl(float v, float *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

template <bool NORMAL>
__global__ void __launch_bounds__(1024) k_ppo_loss_kl(KlLossArgs a) {
    __shared__ float red[1024];
    const LossCfg &c = a.cfg;
    const float beta = a.beta[0];
    float s_pol = 0.f, s_val = 0.f, s_ent = 0.f, s_kl = 0.f;
    for (i64 b = threadIdx.x; b < a.B; b += 1024) {
        const float v = a.v[b], vt = a.v_target[b];
        const float adv = c.baseline_advantage ? a.advantage[b] - v : a.advantage[b];
        float ent = 0.f;
        if constexpr (NORMAL) {
            for (int k = 0; k < a.K; k++) {
                const i64 i = b * a.K + k;
                float term, e1, kl;
                srlxp::policy_normal_kl(c, beta, a.loc[i], a.log_scale[i], a.action[i], a.old_logpi[i], a.old0[i], a.old1[i], adv, term, e1, kl, a.d_loc[i], a.d_log_scale[i]);
                s_pol += term, ent += e1, s_kl += kl;
            }
        } else {
            float term, kl, dl[srlxp::kCatMax];
            const int act = min(max(a.action_index[b], 0), a.K - 1);
            srlxp::policy_categorical_kl(c, beta, a.loc + b * a.K, a.K, act, a.old_logpi[b], a.old0 + b * a.K, adv, term, ent, kl, dl);
            s_pol += term, s_kl += kl;
#pragma unroll
            for (int k = 0; k < srlxp::kCatMax; k++)
                if (k < a.K) a.d_loc[b * a.K + k] = dl[k];
        }
        s_ent += ent;
        float g_v;
        s_val += srlxp::value_term(c, v, vt, c.value_clip ? a.old_v[b] : 0.f, g_v);
        a.d_v[b] = g_v;
    }
    const float p = block_sum_kl(s_pol, red), vl = block_sum_kl(s_val, red), en = block_sum_kl(s_ent, red), kl = block_sum_kl(s_kl, red);  // (every thread has read beta by now)
    if (threadIdx.x == 0) {
        const float kl_mean = c.inv_bk * kl, nb = srlxp::kl_adapt_beta(beta, kl_mean, a.kl_lo, a.kl_hi);
        a.losses[0] = -c.inv_bk * p, a.losses[1] = c.value_w * c.inv_b * vl, a.losses[2] = c.entropy_w * -c.inv_b * en, a.losses[3] = kl_mean, a.losses[4] = nb;
        a.beta[0] = nb;
    }
}

__global__ void __launch_bounds__(256) k_normal_act_dist(i64 n, const float *loc, const float *log_scale, float ls_lo, float ls_hi, unsigned long long seed, const i64 *counter,
                                                         int deterministic, float *action, float *logprob, float *old_loc, float *old_ls) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    srlxp::normal_act_one(loc[i], log_scale[i], ls_lo, ls_hi, seed, deterministic ? 0ull : (unsigned long long)counter[0], i, deterministic, action[i], logprob[i]);
    old_loc[i] = loc[i];
    old_ls[i] = srlxp::clampf(log_scale[i], ls_lo, ls_hi);
}

__global__ void __launch_bounds__(256) k_categorical_act_dist(i64 rows, int n, const float *__restrict__ logits, unsigned long long seed, const i64 *counter, int deterministic,
                                                              int32_t *__restrict__ action, float *__restrict__ logprob, float *__restrict__ probs) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int a;
    srlxp::cat_act_one<true>(logits + r * n, n, seed, deterministic ? 0ull : (unsigned long long)counter[0], r, deterministic, a, logprob[r], probs + r * n);
    action[r] = a;
}

__global__ void __launch_bounds__(256) k_pendulum(i64 E, float *state /*[E][2] th, thdot*/, int32_t *t_in_ep, const float *action, i64 episode_len,
                                                  unsigned long long seed, const i64 *counter, float *obs /*[E][3]*/, float *reward, u8 *done) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float th = state[2 * e], thd = state[2 * e + 1];
    int t = t_in_ep[e];
    srlxp::pendulum_one(th, thd, t, action[e], episode_len, seed, (unsigned long long)counter[0], e, obs[3 * e], obs[3 * e + 1], obs[3 * e + 2], reward[e], done[e]);
    state[2 * e] = th;
    state[2 * e + 1] = thd;
    t_in_ep[e] = t;
}

__global__ void k_advance1(i64 *c) { c[0] += 1; }

__global__ void __launch_bounds__(256) k_categorical_act(i64 rows, int n, const float *__restrict__ logits, unsigned long long seed, const i64 *counter, int deterministic,
                                                         int32_t *__restrict__ action, float *__restrict__ logprob) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int a;
    srlxp::cat_act_one(logits + r * n, n, seed, deterministic ? 0ull : (unsigned long long)counter[0], r, deterministic, a, logprob[r]);
    action[r] = a;
}

__global__ void __launch_bounds__(256) k_cartpole_auto(i64 E, double *__restrict__ state, int32_t *__restrict__ steps, int32_t *__restrict__ episodes,
                                                       const int32_t *__restrict__ actions, i64 max_steps, unsigned long long seed, float *__restrict__ obs,
                                                       float *__restrict__ reward, u8 *__restrict__ done) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double s[4] = {state[4 * e], state[4 * e + 1], state[4 * e + 2], state[4 * e + 3]};
    int st = steps[e], ep = episodes[e];
    float o[4];
    srlxp::cartpole_one(s, st, ep, actions[e], max_steps, seed, e, o, reward[e], done[e]);
    for (int k = 0; k < 4; k++) state[4 * e + k] = s[k], obs[4 * e + k] = o[k];
    steps[e] = st, episodes[e] = ep;
}

}  // namespace

extern "C" {

int srlx_ppo_normal_act(int64_t n, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max, uint64_t seed,
                        int64_t *d_counter, int deterministic, float *d_action, float *d_logprob, void *stream) {
    SRLX_REQUIRE(n > 0 && d_loc && d_log_scale && d_action && d_logprob && (deterministic || d_counter), "ppo_normal_act: bad argument");
    hipLaunchKernelGGL(k_normal_act, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n, d_loc, d_log_scale, (float)log_scale_min,
                       (float)log_scale_max, (unsigned long long)seed, (const i64 *)d_counter, deterministic, d_action, d_logprob);
    if (!deterministic) hipLaunchKernelGGL(k_advance1, dim3(1), dim3(1), 0, (hipStream_t)stream, d_counter);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

static int ppo_loss_common(PpoArgs &a, bool normal, void *stream) {
    SRLX_REQUIRE(a.B > 0 && a.K > 0 && a.old_logpi && a.advantage && a.v && a.v_target && a.losses && a.d_v, "ppo_loss: bad argument");
    SRLX_REQUIRE(!a.value_clip || a.old_v, "ppo_loss: enable_value_clip needs old_v");
    SRLX_HIP(hipMemsetAsync(a.losses, 0, 3 * sizeof(float), (hipStream_t)stream));
    i64 blocks = (a.B + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (normal)
        hipLaunchKernelGGL(k_ppo_loss<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_ppo_loss<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_ppo_loss_normal(int64_t batch, int action_dim, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max,
                         const float *d_action, const float *d_old_logpi, const float *d_advantage, const float *d_v, const float *d_v_target,
                         const float *d_old_v, int baseline_advantage, int surrogate_clip, double policy_clip_range, int enable_value_clip,
                         double value_clip_range, double value_loss_weight, double entropy_weight, float *d_losses, float *d_grad_loc,
                         float *d_grad_log_scale, float *d_grad_v, void *stream) {
    SRLX_REQUIRE(d_loc && d_log_scale && d_action && d_grad_loc && d_grad_log_scale, "ppo_loss_normal: NULL argument");
    PpoArgs a{};
    a.B = batch;
    a.K = action_dim;
    a.loc = d_loc;
    a.log_scale = d_log_scale;
    a.action = d_action;
    a.old_logpi = d_old_logpi;
    a.advantage = d_advantage;
    a.v = d_v;
    a.v_target = d_v_target;
    a.old_v = d_old_v;
    a.ls_lo = (float)log_scale_min;
    a.ls_hi = (float)log_scale_max;
    a.baseline_advantage = baseline_advantage;
    a.surrogate_clip = surrogate_clip;
    a.value_clip = enable_value_clip;
    a.policy_clip = (float)policy_clip_range;
    a.value_clip_range = (float)value_clip_range;
    a.value_w = (float)value_loss_weight;
    a.entropy_w = (float)entropy_weight;
    a.losses = d_losses;
    a.d_loc = d_grad_loc;
    a.d_log_scale = d_grad_log_scale;
    a.d_v = d_grad_v;
    return ppo_loss_common(a, true, stream);
}

int srlx_ppo_loss_logpi(int64_t batch, int n_logpi, const float *d_new_logpi, const float *d_old_logpi, const float *d_advantage, const float *d_v,
                        const float *d_v_target, const float *d_old_v, int baseline_advantage, int surrogate_clip, double policy_clip_range,
                        int enable_value_clip, double value_clip_range, double value_loss_weight, double entropy_weight, float *d_losses,
                        float *d_grad_logpi, float *d_grad_v, void *stream) {
    SRLX_REQUIRE(d_new_logpi && d_grad_logpi, "ppo_loss_logpi: NULL argument");
    PpoArgs a{};
    a.B = batch;
    a.K = n_logpi;
    a.new_logpi = d_new_logpi;
    a.old_logpi = d_old_logpi;
    a.advantage = d_advantage;
    a.v = d_v;
    a.v_target = d_v_target;
    a.old_v = d_old_v;
    a.baseline_advantage = baseline_advantage;
    a.surrogate_clip = surrogate_clip;
    a.value_clip = enable_value_clip;
    a.policy_clip = (float)policy_clip_range;
    a.value_clip_range = (float)value_clip_range;
    a.value_w = (float)value_loss_weight;
    a.entropy_w = (float)entropy_weight;
    a.losses = d_losses;
    a.d_logpi = d_grad_logpi;
    a.d_v = d_grad_v;
    return ppo_loss_common(a, false, stream);
}

int srlx_ppo_categorical_act(int64_t rows, int n_actions, const float *d_logits, uint64_t seed, int64_t *d_counter, int deterministic, int32_t *d_action,
                             float *d_logprob, void *stream) {
    SRLX_REQUIRE(rows > 0 && n_actions >= 1 && d_logits && d_action && d_logprob && (deterministic || d_counter), "ppo_categorical_act: bad argument");
    hipLaunchKernelGGL(k_categorical_act, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)rows, n_actions, d_logits, (unsigned long long)seed,
                       (const i64 *)d_counter, deterministic, d_action, d_logprob);
    if (!deterministic) hipLaunchKernelGGL(k_advance1, dim3(1), dim3(1), 0, (hipStream_t)stream, d_counter);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_ppo_normal_act_dist(int64_t n, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max, uint64_t seed, int64_t *d_counter,
                             int deterministic, float *d_action, float *d_logprob, float *d_old_loc, float *d_old_log_scale, void *stream) {
    SRLX_REQUIRE(n > 0 && d_loc && d_log_scale && d_action && d_logprob && d_old_loc && d_old_log_scale && (deterministic || d_counter), "ppo_normal_act_dist: bad argument");
    hipLaunchKernelGGL(k_normal_act_dist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n, d_loc, d_log_scale, (float)log_scale_min, (float)log_scale_max,
                       (unsigned long long)seed, (const i64 *)d_counter, deterministic, d_action, d_logprob, d_old_loc, d_old_log_scale);
    if (!deterministic) hipLaunchKernelGGL(k_advance1, dim3(1), dim3(1), 0, (hipStream_t)stream, d_counter);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_ppo_categorical_act_dist(int64_t rows, int n_actions, const float *d_logits, uint64_t seed, int64_t *d_counter, int deterministic, int32_t *d_action, float *d_logprob,
                                  float *d_probs, void *stream) {
    SRLX_REQUIRE(rows > 0 && n_actions >= 1 && d_logits && d_action && d_logprob && d_probs && (deterministic || d_counter), "ppo_categorical_act_dist: bad argument");
    hipLaunchKernelGGL(k_categorical_act_dist, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)rows, n_actions, d_logits, (unsigned long long)seed,
                       (const i64 *)d_counter, deterministic, d_action, d_logprob, d_probs);
    if (!deterministic) hipLaunchKernelGGL(k_advance1, dim3(1), dim3(1), 0, (hipStream_t)stream, d_counter);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

static int ppo_loss_kl_common(const char *name, KlLossArgs &a, bool normal, int baseline_advantage, int enable_value_clip, double value_clip_range, double value_loss_weight,
                              double entropy_weight, double ls_lo, double ls_hi, double kl_target, void *stream) {
    SRLX_REQUIRE(a.B > 0 && a.K > 0 && a.loc && a.old_logpi && a.old0 && a.advantage && a.v && a.v_target && a.beta && a.losses && a.d_loc && a.d_v, "%s: bad argument", name);
    SRLX_REQUIRE(!enable_value_clip || a.old_v, "%s: enable_value_clip needs old_v", name);
    SRLX_REQUIRE(kl_target > 0, "%s: adaptive_kl_target must be positive", name);
    a.cfg = LossCfg{(float)ls_lo, (float)ls_hi, baseline_advantage, 0, enable_value_clip, 0.f, (float)value_clip_range, (float)value_loss_weight, (float)entropy_weight,
                    1.0f / (float)a.B, 1.0f / (float)(normal ? a.B * a.K : a.B)};
    a.kl_lo = kl_target / 1.5, a.kl_hi = kl_target * 1.5;
    if (normal)
        hipLaunchKernelGGL(k_ppo_loss_kl<true>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_ppo_loss_kl<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_ppo_loss_normal_kl(int64_t batch, int action_dim, const float *d_loc, const float *d_log_scale, double log_scale_min, double log_scale_max, const float *d_action,
                            const float *d_old_logpi, const float *d_old_loc, const float *d_old_log_scale, const float *d_advantage, const float *d_v, const float *d_v_target,
                            const float *d_old_v, int baseline_advantage, int enable_value_clip, double value_clip_range, double value_loss_weight, double entropy_weight,
                            double adaptive_kl_target, float *d_kl_beta, float *d_losses, float *d_grad_loc, float *d_grad_log_scale, float *d_grad_v, void *stream) {
    SRLX_REQUIRE(d_log_scale && d_action && d_old_log_scale && d_grad_log_scale, "ppo_loss_normal_kl: NULL argument");
    KlLossArgs a{};
    a.B = batch, a.K = action_dim;
    a.loc = d_loc, a.log_scale = d_log_scale, a.action = d_action;
    a.old_logpi = d_old_logpi, a.old0 = d_old_loc, a.old1 = d_old_log_scale;
    a.advantage = d_advantage, a.v = d_v, a.v_target = d_v_target, a.old_v = d_old_v;
    a.beta = d_kl_beta, a.losses = d_losses, a.d_loc = d_grad_loc, a.d_log_scale = d_grad_log_scale, a.d_v = d_grad_v;
    return ppo_loss_kl_common("ppo_loss_normal_kl", a, true, baseline_advantage, enable_value_clip, value_clip_range, value_loss_weight, entropy_weight, log_scale_min, log_scale_max,
                              adaptive_kl_target, stream);
}

int srlx_ppo_loss_categorical_kl(int64_t batch, int n_actions, const float *d_logits, const int32_t *d_action, const float *d_old_logpi, const float *d_old_probs,
                                 const float *d_advantage, const float *d_v, const float *d_v_target, const float *d_old_v, int baseline_advantage, int enable_value_clip,
                                 double value_clip_range, double value_loss_weight, double entropy_weight, double adaptive_kl_target, float *d_kl_beta, float *d_losses,
                                 float *d_grad_logits, float *d_grad_v, void *stream) {
    SRLX_REQUIRE(d_action && n_actions >= 2 && n_actions <= srlxp::kCatMax, "ppo_loss_categorical_kl: 2 <= n_actions <= 8, an action index per row");
    KlLossArgs a{};
    a.B = batch, a.K = n_actions;
    a.loc = d_logits, a.action_index = d_action;
    a.old_logpi = d_old_logpi, a.old0 = d_old_probs;
    a.advantage = d_advantage, a.v = d_v, a.v_target = d_v_target, a.old_v = d_old_v;
    a.beta = d_kl_beta, a.losses = d_losses, a.d_loc = d_grad_logits, a.d_v = d_grad_v;
    return ppo_loss_kl_common("ppo_loss_categorical_kl", a, false, baseline_advantage, enable_value_clip, value_clip_range, value_loss_weight, entropy_weight, 0.0, 0.0,
                              adaptive_kl_target, stream);
}

int srlx_cartpole_autoreset_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const int32_t *d_actions, int64_t max_steps, uint64_t seed,
                                 float *d_obs, float *d_reward, uint8_t *d_done, void *stream) {
    SRLX_REQUIRE(n_envs > 0 && d_state && d_steps && d_episodes && d_actions && d_obs && d_reward && d_done && max_steps > 0, "cartpole_autoreset_step: bad argument");
    hipLaunchKernelGGL(k_cartpole_auto, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n_envs, d_state, d_steps, d_episodes, d_actions,
                       (i64)max_steps, (unsigned long long)seed, d_obs, d_reward, d_done);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_pendulum_step(int64_t n_envs, float *d_state, int32_t *d_step_in_episode, const float *d_action, int64_t episode_len, uint64_t seed,
                       int64_t *d_counter, float *d_obs, float *d_reward, uint8_t *d_done, void *stream) {
    SRLX_REQUIRE(n_envs > 0 && d_state && d_step_in_episode && d_action && d_counter && d_obs && d_reward && d_done && episode_len > 0,
                 "pendulum_step: bad argument");
    hipLaunchKernelGGL(k_pendulum, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n_envs, d_state, d_step_in_episode, d_action,
                       (i64)episode_len, (unsigned long long)seed, (const i64 *)d_counter, d_obs, d_reward, d_done);
    hipLaunchKernelGGL(k_advance1, dim3(1), dim3(1), 0, (hipStream_t)stream, d_counter);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
