// srlx_ppo_net.hip -- PPO's actor-critic (srl/algorithms/ppo/ppo.py:55-99 with the default blocks: in -> 64 -> 64 -> {64 -> V, 64 -> (loc, log_scale)}) as four kernels:
//   k_ppo_rollout   : the WHOLE rollout of an iteration in one launch -- T steps of E environments: network forward, policy sample + log-probability
//                     (ppo.py:316-339), environment step with auto-reset, the [T][E] buffers, episode returns, V(s_T) and the GAE scan (:389-404).  A template over
//                     its Task -- a policy head on its built-in environment: PendulumNormal, CartPoleCategorical -- which holds all that differs between them.
//                     One workgroup owns 16 environments for all T steps (an environment's steps depend on each other, the environments do not): weights and
//                     activations live in LDS (the 64 x 64 layers as v_mfma_f32_16x16x4_f32 tiles), nothing but the buffers goes to HBM.
//   k_ppo_minibatch : one minibatch of the update in one launch -- gather of the permuted samples, forward, compute_train_loss + gradient seeds (:102-169), the whole
//                     backward pass; every workgroup walks tiles of 64 samples (the three 64 x 64 layers on v_mfma_f32_32x32x2_f32) and keeps ITS sum of the
//                     12 931 parameter gradients in registers; per-workgroup partial gradients go to HBM once.
//   k_ppo_reduce    : partial gradients -> the flat gradient (fixed order: deterministic) + the three reported losses.
//   k_ppo_adam      : global-norm clip (:240-241, torch.nn.utils.clip_grad_norm_) + Adam (torch.optim.Adam) over the flat parameter vector, one workgroup; between
//                     k_ppo_reduce and k_ppo_adam sits the data-parallel job's ONE all-reduce of the flat gradient (device/ppo.py).
//   k_ppo_adv_baseline : baseline_type "ave" / "std" / "normal" (:222-233) over one minibatch's advantages, in front of k_ppo_minibatch: one workgroup, two float64 passes.
// What a ppo.Config asks beyond the network is compiled in on demand: k_ppo_adam<SCHED> evaluates a learning-rate schedule (srlx_lr_math.h) from the step count it reads
// from device memory, k_ppo_rollout<Task, EX> clips rewards / observations and rescales the action (srlx_ppo_env_opts_t); the <false> instantiations are the kernels
// as they were, and what a constant schedule / an all-off options struct launches.  surrogate_type "kl" is a third such switch (KL): k_ppo_rollout<Task, EX, true> also
// records the acting distribution, k_ppo_minibatch<CAT, true> gathers it, adds the KL seeds and a fourth loss sum, and k_ppo_reduce_kl forms kl_mean and adapts beta in
// device memory (srlx_ppo_math.h: kl_adapt_beta) -- the captured update graph follows beta as it follows the schedule.
// The same four kernels serve a CATEGORICAL head (template parameter CAT; discrete actions, ppo.py:316-324): in -> 64 -> 64 -> {64 -> V, 64 -> n logits}, parameters
// ... wp, bp, wlogit [n][64], blogit [n].  The n <= 8 logit rows take the 2 * A_MAX = 8 policy-head slots the Normal head's loc / log_scale rows take (slot k: k < 4
// in wloc's place, else in wls's), so the LDS image, the heads / seeds tables and the whole backward pass are shared; what differs is the parameter layout, the
// loss seeds and the rollout's Task: CartPoleCategorical steps CartPole (float64 state, srlx_ppo_math.h: cartpole_one) under a categorical sample.
// float32 throughout, fmaf accumulation in ascending input order; the per-sample policy / loss / environment arithmetic is srlx_ppo_math.h, shared with the
// one-purpose kernels of srlx_ppo.hip.  Parameters are ONE flat float32 vector in torch's `ActorCritic.parameters()` order (weights [out][in]).
// Bounds: VALU (f32 FMA) -- about 76 kFLOP per sample and update (forward + backward), 25 kFLOP per environment step; HBM traffic is the buffers only.
#include <type_traits>

#include "srlx_adam_math.h"
#include "srlx_common.h"
#include "srlx_lr_math.h"
#include "srlx_ppo_math.h"

namespace {

using i64 = int64_t;
using u8 = unsigned char;
using u64 = unsigned long long;
using srlxp::LossCfg;

constexpr int H = 64;       // width of every hidden layer (the reference's default blocks)
constexpr int OBS_MAX = 8;  // observation dimensions
constexpr int A_MAX = 4;    // action dimensions
constexpr int RE = 16;      // environments per workgroup in the rollout / forward kernels
constexpr int S = 64;       // samples per tile in the minibatch kernel

struct NetOff {
    int w1, b1, w2, b2, wv, bv, wvo, bvo, wp, bp, wloc, bloc, wls, bls, total;
};
__host__ __device__ inline NetOff net_off(int obs, int A) {
    NetOff o;
    int p = 0;
    o.w1 = p, p += H * obs;
    o.b1 = p, p += H;
    o.w2 = p, p += H * H;
    o.b2 = p, p += H;
    o.wv = p, p += H * H;
    o.bv = p, p += H;
    o.wvo = p, p += H;
    o.bvo = p, p += 1;
    o.wp = p, p += H * H;
    o.bp = p, p += H;
    o.wloc = p, p += A * H;
    o.bloc = p, p += A;
    o.wls = p, p += A * H;
    o.bls = p, p += A;
    o.total = p;
    return o;
}

// categorical head: wlogit / blogit stand where wloc / bloc do; there is no second head tensor
__host__ __device__ inline NetOff net_off_cat(int obs, int n) {
    NetOff o = net_off(obs, 0);
    int p = o.wloc;
    o.wloc = p, p += n * H;
    o.bloc = p, p += n;
    o.wls = o.bls = o.total = p;
    return o;
}
template <bool CAT>
__host__ __device__ inline NetOff net_off_of(int obs, int A) {
    return CAT ? net_off_cat(obs, A) : net_off(obs, A);
}
static_assert(srlxp::kCatMax == 2 * A_MAX, "the logit rows take the loc + log_scale slots");

// LDS image of the small tensors (everything but the three 64 x 64 matrices)
struct Small {
    float w1[H * OBS_MAX], b1[H], b2[H], bv[H], bp[H], wvo[H], wloc[A_MAX * H], wls[A_MAX * H], bvo[4], bloc[A_MAX], bls[A_MAX];  // (a multiple of 16 bytes)
};

template <bool CAT = false>
__device__ __forceinline__ void load_small(Small &sm, const float *__restrict__ p, const NetOff &o, int obs, int A) {
    const int t = threadIdx.x, n = blockDim.x;
    for (int i = t; i < H * obs; i += n) sm.w1[i] = p[o.w1 + i];
    for (int i = t; i < H; i += n) {
        sm.b1[i] = p[o.b1 + i];
        sm.b2[i] = p[o.b2 + i];
        sm.bv[i] = p[o.bv + i];
        sm.bp[i] = p[o.bp + i];
        sm.wvo[i] = p[o.wvo + i];
    }
    if constexpr (CAT) {  // logit row k: slot k of the eight policy-head rows
        for (int i = t; i < A * H; i += n) {
            if (i < A_MAX * H)
                sm.wloc[i] = p[o.wloc + i];
            else
                sm.wls[i - A_MAX * H] = p[o.wloc + i];
        }
        if (t < A) {
            if (t < A_MAX)
                sm.bloc[t] = p[o.bloc + t];
            else
                sm.bls[t - A_MAX] = p[o.bloc + t];
        }
    } else {
        for (int i = t; i < A * H; i += n) {
            sm.wloc[i] = p[o.wloc + i];
            sm.wls[i] = p[o.wls + i];
        }
        if (t < A) {
            sm.bloc[t] = p[o.bloc + t];
            sm.bls[t] = p[o.bls + t];
        }
    }
    if (t == 0) sm.bvo[0] = p[o.bvo];
}

// W [j][k] in HBM -> Wt [k][j] in LDS (the forward's operand: a thread reads four consecutive units of one input)
__device__ __forceinline__ void load_transposed(float *__restrict__ wt, const float *__restrict__ w) {
    for (int i = threadIdx.x; i < H * H; i += blockDim.x) {
        const int j = i >> 6, k = i & 63;
        wt[k * H + j] = w[i];
    }
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }
__device__ __forceinline__ float4 fma4(float s, float4 w, float4 a) { return make_float4(fmaf(s, w.x, a.x), fmaf(s, w.y, a.y), fmaf(s, w.z, a.z), fmaf(s, w.w, a.w)); }

// first layer: out[j0 .. j0 + 3] = b1 + sum_o x[o] * w1[j][o]
__device__ __forceinline__ float4 first_row(const float *__restrict__ x, const Small &sm, int obs, int j0) {
    float acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float a = sm.b1[j0 + i];
        for (int o = 0; o < obs; o++) a = fmaf(x[o], sm.w1[(j0 + i) * obs + o], a);
        acc[i] = a;
    }
    return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__device__ __forceinline__ float dot64(const float *__restrict__ a, const float *__restrict__ b, float bias) {
    float acc = bias;
#pragma unroll 8
    for (int k = 0; k < H; k++) acc = fmaf(a[k], b[k], acc);
    return acc;
}

// The forward of RE = 16 rows held in LDS (x [RE][OBS_MAX]) by 256 threads.  The first layer and the heads on the vector pipe; the three 64 x 64 layers as
// v_mfma_f32_16x16x4_f32 tiles: wave w owns units 16 w .. 16 w + 15 of all 16 rows, 16 chained MFMAs per layer (lane l supplies in[row l & 15][k] and
// Wt[k][unit l & 15] for k = (l >> 4) + 4 q; D[4 (l >> 4) + i][l & 15] = acc[i]) -- a layer is 0.5 k clocks of matrix pipe instead of ~3 k clocks of LDS-latency-
// bound FMAs (one workgroup per CU, one wave per SIMD).  Activation rows are 65 floats long ("lane i reads row i" without bank conflicts).
// heads [RE][1 + 2 A]: v, loc, log_scale (CAT: [RE][1 + n]: v, logits).  value_only: the policy branch is skipped (V(s_T)).  Ends behind a barrier.
constexpr int LDF = 65;
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct FwdLds {
    float wt2[H * H], wtv[H * H], wtp[H * H];
    Small sm;
    float x[RE * OBS_MAX], h1[RE * LDF], h2[RE * LDF], hv[RE * LDF], hp[RE * LDF], heads[RE * (1 + 2 * A_MAX)];
};

__device__ __forceinline__ void mfma16_dense(const float *__restrict__ in, const float *__restrict__ wt, const float *__restrict__ bias, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, n0 = (threadIdx.x >> 6) * 16, c = lane & 15, g = lane >> 4;
    const float b = bias[n0 + c];
    f32x4 acc = {b, b, b, b};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int k = g + 4 * q;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(in[c * LDF + k], wt[k * H + n0 + c], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[(4 * g + i) * LDF + n0 + c] = fmaxf(acc[i], 0.f);
}

template <bool CAT = false>
__device__ __forceinline__ void forward_rows(FwdLds &L, int obs, int A, bool value_only) {
    const int tid = threadIdx.x, e = tid >> 4, j0 = (tid & 15) * 4;
    {
        const float4 h = relu4(first_row(L.x + e * OBS_MAX, L.sm, obs, j0));
        float *o = L.h1 + e * LDF + j0;
        o[0] = h.x, o[1] = h.y, o[2] = h.z, o[3] = h.w;
    }
    __syncthreads();
    mfma16_dense(L.h1, L.wt2, L.sm.b2, L.h2);
    __syncthreads();
    mfma16_dense(L.h2, L.wtv, L.sm.bv, L.hv);
    if (!value_only) mfma16_dense(L.h2, L.wtp, L.sm.bp, L.hp);
    __syncthreads();
    const int n_out = CAT ? 1 + A : 1 + 2 * A;
    if (tid < RE * n_out) {
        const int r = tid % RE, o = tid / RE;  // (consecutive lanes: consecutive rows)
        float v;
        if (o == 0)
            v = dot64(L.hv + r * LDF, L.sm.wvo, L.sm.bvo[0]);
        else if (value_only)
            v = 0.f;
        else if (CAT)
            v = o <= A_MAX ? dot64(L.hp + r * LDF, L.sm.wloc + (o - 1) * H, L.sm.bloc[o - 1]) : dot64(L.hp + r * LDF, L.sm.wls + (o - 1 - A_MAX) * H, L.sm.bls[o - 1 - A_MAX]);
        else if (o <= A)
            v = dot64(L.hp + r * LDF, L.sm.wloc + (o - 1) * H, L.sm.bloc[o - 1]);
        else
            v = dot64(L.hp + r * LDF, L.sm.wls + (o - 1 - A) * H, L.sm.bls[o - 1 - A]);
        L.heads[r * (1 + 2 * A_MAX) + o] = v;
    }
    __syncthreads();
}

template <bool CAT = false>
__device__ __forceinline__ void load_forward_weights(FwdLds &L, const float *__restrict__ params, const NetOff &o, int obs, int A) {
    load_transposed(L.wt2, params + o.w2);
    load_transposed(L.wtv, params + o.wv);
    load_transposed(L.wtp, params + o.wp);
    load_small<CAT>(L.sm, params, o, obs, A);
}

// ---- plain forward (evaluation, tests, rollouts of environments other than the built-in one) -----------------------------------------------------------------------
// (CAT: loc [n][A] receives the logits, ls is not written)
template <bool CAT>
__global__ void __launch_bounds__(256) k_ppo_forward(i64 n, int obs, int A, const float *__restrict__ params, const float *__restrict__ x, float *__restrict__ v, float *__restrict__ loc,
                                                     float *__restrict__ ls) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    FwdLds &L = *reinterpret_cast<FwdLds *>(lds_raw);
    const NetOff o = net_off_of<CAT>(obs, A);
    load_forward_weights<CAT>(L, params, o, obs, A);
    const int tid = threadIdx.x;
    for (i64 r0 = (i64)blockIdx.x * RE; r0 < n; r0 += (i64)gridDim.x * RE) {
        __syncthreads();
        if (tid < RE * obs) {
            const int r = tid / obs, c = tid % obs;
            L.x[r * OBS_MAX + c] = r0 + r < n ? x[(r0 + r) * obs + c] : 0.f;
        }
        __syncthreads();
        forward_rows<CAT>(L, obs, A, false);
        if (tid < RE && r0 + tid < n) {
            const float *hd = L.heads + tid * (1 + 2 * A_MAX);
            v[r0 + tid] = hd[0];
            for (int a = 0; a < A; a++) {
                loc[(r0 + tid) * A + a] = hd[1 + a];
                if (!CAT) ls[(r0 + tid) * A + a] = hd[1 + A + a];
            }
        }
    }
}

// ---- the rollout -------------------------------------------------------------------------------------------------------------------------------------------------------
// k_ppo_rollout<Task> is the scaffold -- LDS, weights, the T-step loop, the record tables, episode returns, V(s_T), GAE; a Task (below) is a policy head on its
// built-in environment: everything the scaffold does not know.
template <class Task>
struct RolloutArgs {
    i64 E, T;
    int A;  // action dimensions (CAT: actions)
    const float *params;
    float *env_obs;   // [E][OBS]: the observation the rollout starts from / ends at
    i64 episode_len;  // (CartPole: max_steps)
    u64 env_seed, act_seed;
    i64 *act_counter;  // advances by T per rollout (Task::advance, behind this kernel)
    typename Task::Env env;
    double discount, lam;
    float *b_obs /*[T+1][E][OBS]*/;
    typename Task::Act *b_act /*[T][E][A]; CAT: [T][E]*/;
    float *b_logp, *b_val /*[T][E]*/, *b_rew;
    u8 *b_done;
    float *b_adv, *last_v /*[E]*/, *episode_return /*[E]*/, *finished /*[2] sum, count*/;
    srlx_ppo_env_opts_t opts;  // reward / state clips, action rescale (srlx.h); all off: the arithmetic of the plain entry points
};
// surrogate_type "kl": where the rollout records the acting distribution -- CAT: d0 = b_probs [T][E][n]; Normal: d0 = b_loc, d1 = b_ls (clamped) [T][E][A]
struct RolloutKl {
    float *d0, *d1;
};
template <class Task, bool KL>
struct RolloutArgsOf;
template <class Task>
struct RolloutArgsOf<Task, false> : RolloutArgs<Task> {};  // (an empty base: the arguments as they were)
template <class Task>
struct RolloutArgsOf<Task, true> : RolloutArgs<Task> {
    RolloutKl kl;
};
constexpr srlx_ppo_env_opts_t kEnvOptsOff = {0, 0.f, 0.f, 0, 0.f, 0.f, 1.f, 0.f};
__host__ __device__ inline bool rescales(const srlx_ppo_env_opts_t &o) { return o.action_scale != 1.f || o.action_offset != 0.f; }

__global__ void k_advance2(i64 *c0, i64 *c1, i64 n) {
    c0[0] += n;
    c1[0] += n;
}
__global__ void k_advance(i64 *c, i64 n) { c[0] += n; }

// The Normal head on the Pendulum-shaped environment (float32 state; a reset is keyed with the environment counter)
struct PendulumNormal {
    static constexpr bool CAT = false;
    static constexpr int OBS = 3;
    using Act = float;
    struct Env {
        float *state;      // [E][2] th, thdot
        int32_t *t_in_ep;  // [E]
        i64 *counter;      // advances by T per rollout, like the action counter
        float ls_lo, ls_hi;
    };
    static bool env_ok(const Env &v) { return v.state && v.t_in_ep && v.counter; }
    static constexpr int records(int A) { return 3 + A; }  // LDS floats per step and environment: reward, value, done + the A draws of zbuf
    static void advance(const Env &v, i64 *act_counter, i64 n, hipStream_t s) { hipLaunchKernelGGL(k_advance2, dim3(1), dim3(1), 0, s, v.counter, act_counter, n); }
    struct Lane {
        float th = 0.f, thd = 0.f;
        int tstep = 0;
        const u64 c_env;  // (uniform)
        __device__ explicit Lane(const Env &v) : c_env((u64)v.counter[0]) {}
        __device__ void load(const Env &v, i64 eg) { th = v.state[2 * eg], thd = v.state[2 * eg + 1], tstep = v.t_in_ep[eg]; }
        __device__ void store(const Env &v, i64 eg) const { v.state[2 * eg] = th, v.state[2 * eg + 1] = thd, v.t_in_ep[eg] = tstep; }
    };
    // zbuf [T][RE][A]: the policy's standard-normal draws of the whole rollout, made up front by all threads (double-precision log / cos off the step loop)
    static __device__ __forceinline__ void draw(const RolloutArgs<PendulumNormal> &a, float *zbuf, u64 c_act, i64 e0) {
        const int A = a.A;
        for (i64 w = threadIdx.x; w < a.T * RE * A; w += 256) {
            const i64 t = w / (RE * A);
            const int rem = (int)(w % (RE * A)), e = rem / A, d = rem % A;
            zbuf[w] = srlxp::normal_z(a.act_seed, c_act + (u64)t, (e0 + e) * A + d);
        }
    }
    // policy sample + log-probability (ppo.py:316-339) -> b_act / b_logp [t][eg]; then the environment's step
    // KL: kl-> also receives the acting distribution of this step: the mean, and the log-scale as normal_act_from_z clamps it
    template <bool EX, bool KL>
    static __device__ __forceinline__ void step(const RolloutArgs<PendulumNormal> &a, const RolloutKl *kl, Lane &s, const float *hd, const float *zbuf, i64 t, u64, i64 eg, float (&ob)[OBS],
                                                float &rw, u8 &dn) {
        const int A = a.A, tid = threadIdx.x;
        float act0 = 0.f;
        for (int d = 0; d < A; d++) {
            float ac, lp;
            srlxp::normal_act_from_z(hd[1 + d], hd[1 + A + d], a.env.ls_lo, a.env.ls_hi, zbuf[(t * RE + tid) * A + d], 0, ac, lp);
            a.b_act[(t * a.E + eg) * A + d] = ac;
            a.b_logp[(t * a.E + eg) * A + d] = lp;
            if constexpr (KL) {
                kl->d0[(t * a.E + eg) * A + d] = hd[1 + d];
                kl->d1[(t * a.E + eg) * A + d] = srlxp::clampf(hd[1 + A + d], a.env.ls_lo, a.env.ls_hi);
            }
            if (d == 0) act0 = ac;
        }
        if (EX && rescales(a.opts)) act0 = act0 * a.opts.action_scale + a.opts.action_offset;  // ppo.py:336: [-1, 1] onto the environment's bounds (no contraction: two roundings)
        srlxp::pendulum_one(s.th, s.thd, s.tstep, act0, a.episode_len, a.env_seed, s.c_env + (u64)t, eg, ob[0], ob[1], ob[2], rw, dn);
    }
};

// The categorical head on CartPole: the environment is float64 (cartpole_one: about 40 f64 operations, one sin and one cos per step on 16 of the workgroup's 256
// lanes) and keeps no counter: a reset is keyed with (lane, episode of the lane).
struct CartPoleCategorical {
    static constexpr bool CAT = true;
    static constexpr int OBS = 4;
    using Act = int32_t;
    struct Env {
        double *state;              // [E][4]
        int32_t *steps, *episodes;  // [E]
    };
    static bool env_ok(const Env &v) { return v.state && v.steps && v.episodes; }
    static constexpr int records(int) { return 3; }  // reward, value, done
    static void advance(const Env &, i64 *act_counter, i64 n, hipStream_t s) { hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, act_counter, n); }
    struct Lane {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        int steps = 0, episode = 0;
        __device__ explicit Lane(const Env &) {}
        __device__ void load(const Env &v, i64 eg) {
#pragma unroll
            for (int c = 0; c < 4; c++) s[c] = v.state[4 * eg + c];
            steps = v.steps[eg], episode = v.episodes[eg];
        }
        __device__ void store(const Env &v, i64 eg) const {
#pragma unroll
            for (int c = 0; c < 4; c++) v.state[4 * eg + c] = s[c];
            v.steps[eg] = steps, v.episodes[eg] = episode;
        }
    };
    static __device__ __forceinline__ void draw(const RolloutArgs<CartPoleCategorical> &, float *, u64, i64) {}  // (one uniform per step, drawn in it)
    // categorical sample + log-probability (ppo.py:316-324), the environment's step; then b_act / b_logp [t][eg]
    // KL: kl->d0 also receives the acting distribution of this step: the probabilities the sampler sums (cat_act_one<true>)
    template <bool EX, bool KL>
    static __device__ __forceinline__ void step(const RolloutArgs<CartPoleCategorical> &a, const RolloutKl *kl, Lane &s, const float *hd, const float *, i64 t, u64 c_act, i64 eg,
                                                float (&ob)[OBS], float &rw, u8 &dn) {
        int ac;
        float lp;
        if constexpr (KL)
            srlxp::cat_act_one<true>(hd + 1, a.A, a.act_seed, c_act + (u64)t, eg, 0, ac, lp, kl->d0 + (t * a.E + eg) * a.A);
        else
            srlxp::cat_act_one(hd + 1, a.A, a.act_seed, c_act + (u64)t, eg, 0, ac, lp);
        srlxp::cartpole_one(s.s, s.steps, s.episode, ac, a.episode_len, a.env_seed, eg, ob, rw, dn);
        a.b_act[t * a.E + eg] = ac;
        a.b_logp[t * a.E + eg] = lp;
    }
};

// The GAE scan of one environment (thread tid < RE) over the rollout's LDS records (the arithmetic of k_gae_scan, srlx_train.hip)
__device__ __forceinline__ void gae_rows(const float *t_rew, const float *t_val, const float *t_done, i64 T, i64 E, i64 eg, int tid, float lv, double discount, double lam,
                                         float *__restrict__ b_adv) {
    const float g = (float)discount, gl = (float)(discount * lam);
    float gae = 0.f;
    for (i64 i = T - 1; i >= 0; i--) {
        const float r = t_rew[i * RE + tid], v = t_val[i * RE + tid];
        float delta;
        if (t_done[i * RE + tid] != 0.f) {
            delta = r - v;
            gae = 0.f;
        } else if (i == T - 1) {
            delta = (r + g * lv) - v;
        } else {
            delta = (r + g * t_val[(i + 1) * RE + tid]) - v;
        }
        gae = delta + gl * gae;
        b_adv[i * E + eg] = gae;
    }
}

// EX: with the options of a.opts (reward / state clips, action rescale); false: no trace of them in the code -- the rollout as it was before they existed
// KL: the step also writes the acting distribution, from the heads row it samples from; false: no trace of it in the code or the arguments
template <class Task, bool EX, bool KL = false>
__global__ void __launch_bounds__(256) k_ppo_rollout(RolloutArgsOf<Task, KL> a) {
    constexpr int OBS = Task::OBS;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    FwdLds &L = *reinterpret_cast<FwdLds *>(lds_raw);
    float *t_rew = reinterpret_cast<float *>(lds_raw + sizeof(FwdLds));  // [T][RE]
    float *t_val = t_rew + a.T * RE;
    float *t_done = t_val + a.T * RE;
    float *zbuf = t_done + a.T * RE;  // (the records a Task asks for beyond these three)
    const int A = a.A, tid = threadIdx.x;
    const NetOff o = net_off_of<Task::CAT>(OBS, A);
    load_forward_weights<Task::CAT>(L, a.params, o, OBS, A);
    const i64 e0 = (i64)blockIdx.x * RE, eg = e0 + tid;  // (tid < RE: this thread's environment)
    typename Task::Lane lane(a.env);
    float er = 0.f, fin_sum = 0.f, fin_cnt = 0.f;
    if (tid < RE) {
        lane.load(a.env, eg);
        er = a.episode_return[eg];
        for (int c = 0; c < OBS; c++) {
            float v = a.env_obs[OBS * eg + c];
            if (EX && a.opts.state_clip) v = srlxp::clampf(v, a.opts.state_lo, a.opts.state_hi);
            L.x[tid * OBS_MAX + c] = v;
            a.b_obs[OBS * eg + c] = v;
        }
    }
    const u64 c_act = (u64)a.act_counter[0];
    Task::draw(a, zbuf, c_act, e0);
    __syncthreads();
    for (i64 t = 0; t < a.T; t++) {
        forward_rows<Task::CAT>(L, OBS, A, false);
        if (tid < RE) {
            const float *hd = L.heads + tid * (1 + 2 * A_MAX);
            float ob[OBS], rw;
            u8 dn;
            const RolloutKl *kl = nullptr;
            if constexpr (KL) kl = &a.kl;
            Task::template step<EX, KL>(a, kl, lane, hd, zbuf, t, c_act, eg, ob, rw, dn);
            const float raw = rw;  // (the episode's return counts the raw reward)
            if constexpr (EX) {
                if (a.opts.reward_clip) rw = srlxp::clampf(rw, a.opts.reward_lo, a.opts.reward_hi);
                if (a.opts.state_clip) {
#pragma unroll
                    for (int c = 0; c < OBS; c++) ob[c] = srlxp::clampf(ob[c], a.opts.state_lo, a.opts.state_hi);
                }
            }
            const i64 k = t * a.E + eg;
            a.b_val[k] = hd[0];
            a.b_rew[k] = rw;
            a.b_done[k] = dn;
            float *bo = a.b_obs + ((t + 1) * a.E + eg) * OBS;
#pragma unroll
            for (int c = 0; c < OBS; c++) bo[c] = ob[c], L.x[tid * OBS_MAX + c] = ob[c];
            t_rew[t * RE + tid] = rw, t_val[t * RE + tid] = hd[0], t_done[t * RE + tid] = dn ? 1.f : 0.f;
            er += raw;
            if (dn) fin_sum += er, fin_cnt += 1.f, er = 0.f;
        }
        __syncthreads();
    }
    forward_rows<Task::CAT>(L, OBS, A, true);  // V(s_T): a horizon cut inside an episode bootstraps from it, an episode end never does (ppo.py:396-397)
    if (tid < RE) {
        const float lv = L.heads[tid * (1 + 2 * A_MAX)];
        a.last_v[eg] = lv;
        gae_rows(t_rew, t_val, t_done, a.T, a.E, eg, tid, lv, a.discount, a.lam, a.b_adv);
        lane.store(a.env, eg);
        a.episode_return[eg] = er;
        for (int c = 0; c < OBS; c++) a.env_obs[OBS * eg + c] = L.x[tid * OBS_MAX + c];
        if (fin_cnt > 0.f) {
            atomicAdd(&a.finished[0], fin_sum);
            atomicAdd(&a.finished[1], fin_cnt);
        }
    }
}

// ---- one minibatch: forward + loss + backward ----------------------------------------------------------------------------------------------------------------------
struct MbArgs {
    i64 mb;           // samples in this minibatch
    const i64 *perm;  // [mb] rows of the [T * E] buffers
    int obs, A;
    const float *params;
    const float *b_obs, *b_act /*CAT: int32 [n]*/, *b_logp, *b_adv, *b_vt, *b_val;
    LossCfg cfg;
    float *partials;  // [gridDim.x][stride]: per-workgroup gradient sums (parameter order) + 3 loss sums (KL: 4)
    int stride;
};
// surrogate_type "kl": the old distribution's buffers, rows as b_logp's (CAT: b_old0 = b_probs [n]; Normal: b_old0 = b_loc, b_old1 = b_ls [A]) and the beta state
struct MbKl {
    const float *b_old0, *b_old1, *beta;
};
template <bool KL>
struct MbArgsOf;
template <>
struct MbArgsOf<false> : MbArgs {};
template <>
struct MbArgsOf<true> : MbArgs {
    MbKl kl;
};

// The three 64 x 64 layers run on the matrix cores: v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: an fmaf chain per output, the f32 MFMA peak equals the vector
// peak -- the gain is that an operand element is read from LDS once per 32 outputs instead of once per 4, and that 32 chained MFMAs keep a SIMD busy where the
// vector loop waited for LDS).  A tile is 64 samples; each of the four waves owns one 32 x 32 block of every 64 x 64 product (forward: [sample][unit], data
// gradient: [sample][input], weight gradient: [unit][input] with the SAMPLES as the K dimension -- accumulated in registers across the workgroup's tiles).
// LDS rows are 65 floats long: "lane i reads row i" and "lane i reads column i" are both conflict-free, so no matrix is kept twice.
constexpr int LD = 65;
static_assert(S == 64 && H == 64 && RE == 16, "mfma_block: K = 64 for every product; mfma16_dense: 16 rows");
constexpr int HS = 12;  // floats per row of the heads / seeds tables (16-byte rows)
constexpr int kVecs = 6 + 2 * A_MAX + OBS_MAX;  // vectors of 64 partial sums a thread row keeps (b1, b2, bv, bp, wvo, head biases, wloc[], wls[], w1[][c])
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MbLds {
    float w2[H * LD], wv[H * LD], wp[H * LD];  // [unit][input]
    Small sm;
    float x[S * OBS_MAX], h1[S * LD], h2[S * LD], hv[S * LD], hp[S * LD], d2[S * LD];
    float heads[S * HS], seeds[S * HS];
    float red[3 * S];
};

// acc[r] <-> D[(r & 3) + 8 (r >> 2) + 4 h][i] of this lane (i = lane & 31, h = lane >> 5); lane supplies A[i][k], B[k][i] for k = h, h + 2, ...
template <class FA, class FB>
__device__ __forceinline__ f32x16 mfma_block(f32x16 acc, FA a_at, FB b_at) {  // K = 64: 32 chained MFMAs (measured: two interleaved chains, a 16-deep unroll or
    // straight-line code with all operands fetched first are slower or spill -- about 100 clocks per MFMA against the pipe's 64)
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
#pragma unroll 8
    for (int q = 0; q < 32; q++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_at(i, h + 2 * q), b_at(h + 2 * q, i), acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ int acc_row(int r) { return (r & 3) + 8 * (r >> 2) + 4 * ((threadIdx.x & 63) >> 5); }

// out[s][j] = relu(bias[j] + sum_k in[s][k] W[j][k]) for this wave's block (samples m0.., units n0..)
__device__ __forceinline__ void mfma_dense(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ out, int m0, int n0) {
    const int i = threadIdx.x & 31;
    f32x16 acc;
    const float b = bias[n0 + i];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = b;
    acc = mfma_block(acc, [&](int row, int k) { return in[(m0 + row) * LD + k]; }, [&](int k, int col) { return w[(n0 + col) * LD + k]; });
#pragma unroll
    for (int r = 0; r < 16; r++) out[(m0 + acc_row(r)) * LD + n0 + i] = fmaxf(acc[r], 0.f);
}

// acc += dz[s][j] W[j][k] for this wave's block (samples m0.., inputs n0..)
__device__ __forceinline__ f32x16 mfma_dgrad(f32x16 acc, const float *__restrict__ dz, const float *__restrict__ w, int m0, int n0) {
    return mfma_block(acc, [&](int row, int j) { return dz[(m0 + row) * LD + j]; }, [&](int j, int col) { return w[j * LD + n0 + col]; });
}

// acc += sum_s dz[s][j] h[s][k] for this wave's block (units m0.., inputs n0..)
__device__ __forceinline__ f32x16 mfma_wgrad(f32x16 acc, const float *__restrict__ dz, const float *__restrict__ h, int m0, int n0) {
    return mfma_block(acc, [&](int row, int s) { return dz[s * LD + m0 + row]; }, [&](int s, int col) { return h[s * LD + n0 + col]; });
}

// CAT: A = the number of actions; logit k lives in policy-head slot k (seeds column 1 + k; weights wloc[k] for k < 4, wls[k - 4] beyond)
// KL: the "kl" surrogate (a.cfg.surrogate_clip == 0): a sample's old distribution is gathered with its other loss inputs and waits in the sample's row of the seeds
// table (free until the loss writes it: no register is held across the forward), the seeds gain beta * d kl, and a fourth loss sum (kl) joins the three.
template <bool CAT, bool KL = false>
__global__ void __launch_bounds__(256) k_ppo_minibatch(MbArgsOf<KL> a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    MbLds &L = *reinterpret_cast<MbLds *>(lds_raw);
    const int obs = a.obs, A = a.A, tid = threadIdx.x, n_out = CAT ? 1 + A : 1 + 2 * A;
    const NetOff o = net_off_of<CAT>(obs, A);
#pragma unroll 4
    for (int i = tid; i < H * H; i += 256) {
        const int j = i >> 6, k = i & 63;
        L.w2[j * LD + k] = a.params[o.w2 + i];
        L.wv[j * LD + k] = a.params[o.wv + i];
        L.wp[j * LD + k] = a.params[o.wp + i];
    }
    load_small<CAT>(L.sm, a.params, o, obs, A);
    const int wave = tid >> 6, m0 = (wave >> 1) * 32, n0 = (wave & 1) * 32, li = tid & 31;
    // the matrices: this wave's block of W [m0 + acc_row(r)][n0 + li], summed over the workgroup's tiles
    f32x16 g_w2, g_wv, g_wp;
#pragma unroll
    for (int r = 0; r < 16; r++) g_w2[r] = 0.f, g_wv[r] = 0.f, g_wp[r] = 0.f;
    // the vectors: thread (unit u = tid & 63, part = tid >> 6) works on samples 16 part .. 16 part + 15 of every tile; the four parts meet once, behind the tile loop.
    // Fixed extents (8 observation dimensions, 4 action dimensions, zero-padded): no run-time trip counts in the per-sample loops
    const int u = tid & 63, part = tid >> 6, s_lo = 16 * part;
    float g_w1[OBS_MAX] = {}, g_b1 = 0.f, g_b2 = 0.f, g_bv = 0.f, g_bp = 0.f, g_wvo = 0.f, g_wloc[A_MAX] = {}, g_wls[A_MAX] = {};
    float g_head_b = 0.f;                         // u < 12: the seeds' column u (0: bvo, 1 + d: bloc[d], 5 + d: bls[d])
    float s_pol = 0.f, s_val = 0.f, s_ent = 0.f;  // tid < S: loss sums
    [[maybe_unused]] float s_kl = 0.f;            // (KL)
    __syncthreads();
    float w1u[OBS_MAX], wloc_u[A_MAX], wls_u[A_MAX];
#pragma unroll
    for (int c = 0; c < OBS_MAX; c++) w1u[c] = c < obs ? L.sm.w1[u * obs + c] : 0.f;
#pragma unroll
    for (int d = 0; d < A_MAX; d++) wloc_u[d] = d < A ? L.sm.wloc[d * H + u] : 0.f, wls_u[d] = (CAT ? A_MAX + d : d) < A ? L.sm.wls[d * H + u] : 0.f;
    const float b1u = L.sm.b1[u], wvo_u = L.sm.wvo[u];
    const i64 tiles = (a.mb + S - 1) / S;
    for (i64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();
        const i64 row = tile * S + tid;  // (tid < S)
        i64 idx = -1;
        float in_vt = 0.f, in_adv = 0.f, in_val = 0.f, in_act[A_MAX], in_logp[A_MAX];  // this sample's loss inputs: gathered now, used behind the forward
        int in_a = 0;                                                                    // (CAT: the action, and in_logp[0])
        if (tid < S) {
            idx = row < a.mb ? a.perm[row] : -1;
            for (int c = 0; c < OBS_MAX; c++) L.x[tid * OBS_MAX + c] = (idx >= 0 && c < obs) ? a.b_obs[idx * obs + c] : 0.f;
            if (idx >= 0) {
                in_vt = a.b_vt[idx], in_adv = a.b_adv[idx], in_val = a.b_val[idx];
                if constexpr (CAT) {
                    in_a = min(max(reinterpret_cast<const int32_t *>(a.b_act)[idx], 0), A - 1);
                    in_logp[0] = a.b_logp[idx];
                } else {
                    for (int d = 0; d < A; d++) in_act[d] = a.b_act[idx * A + d], in_logp[d] = a.b_logp[idx * A + d];
                }
                if constexpr (KL) {  // columns 1 .. 8 of this sample's seeds row, where its seeds will go
                    float *od = L.seeds + tid * HS;
                    if constexpr (CAT) {
                        for (int k = 0; k < A; k++) od[1 + k] = a.kl.b_old0[idx * A + k];
                    } else {
                        for (int d = 0; d < A; d++) od[1 + d] = a.kl.b_old0[idx * A + d], od[5 + d] = a.kl.b_old1[idx * A + d];
                    }
                }
            }
        }
        __syncthreads();
        // ---- forward ----
#pragma unroll 4
        for (int s = s_lo; s < s_lo + 16; s++) {
            const float4 x0 = ld4(L.x + s * OBS_MAX), x1 = ld4(L.x + s * OBS_MAX + 4);
            float acc = b1u;
            acc = fmaf(x0.x, w1u[0], acc), acc = fmaf(x0.y, w1u[1], acc), acc = fmaf(x0.z, w1u[2], acc), acc = fmaf(x0.w, w1u[3], acc);
            acc = fmaf(x1.x, w1u[4], acc), acc = fmaf(x1.y, w1u[5], acc), acc = fmaf(x1.z, w1u[6], acc), acc = fmaf(x1.w, w1u[7], acc);
            L.h1[s * LD + u] = fmaxf(acc, 0.f);
        }
        __syncthreads();
        mfma_dense(L.h1, L.w2, L.sm.b2, L.h2, m0, n0);
        __syncthreads();
        mfma_dense(L.h2, L.wv, L.sm.bv, L.hv, m0, n0);
        mfma_dense(L.h2, L.wp, L.sm.bp, L.hp, m0, n0);
        __syncthreads();
        for (int w = tid; w < S * n_out; w += 256) {
            const int r = w % S, oo = w / S;  // (consecutive lanes: consecutive rows of an LD = 65 matrix: conflict-free)
            const float *hrow = (oo == 0 ? L.hv : L.hp) + r * LD;
            const int split = CAT ? A_MAX : A;  // heads 1 .. split from wloc / bloc, the rest from wls / bls
            const float *wrow = oo == 0 ? L.sm.wvo : (oo <= split ? L.sm.wloc + (oo - 1) * H : L.sm.wls + (oo - 1 - split) * H);
            L.heads[r * HS + oo] = dot64(hrow, wrow, oo == 0 ? L.sm.bvo[0] : (oo <= split ? L.sm.bloc[oo - 1] : L.sm.bls[oo - 1 - split]));
        }
        __syncthreads();
        // ---- loss + gradient seeds (compute_train_loss, ppo.py:102-169): one thread per sample; seeds row: [0] d/dv, [1 + d] d/dloc, [5 + d] d/dlog_scale ----
        if (tid < S) {
            float sd[HS] = {};
            const float *hd = L.heads + tid * HS;
            if (idx >= 0) {
                const float v = hd[0];
                const float adv = a.cfg.baseline_advantage ? in_adv - v : in_adv;
                float ent = 0.f;
                if constexpr (CAT) {
                    float term, dl[srlxp::kCatMax];
                    if constexpr (KL) {
                        float kl;
                        srlxp::policy_categorical_kl(a.cfg, a.kl.beta[0], hd + 1, A, in_a, in_logp[0], L.seeds + tid * HS + 1, adv, term, ent, kl, dl);
                        s_kl += kl;
                    } else {
                        srlxp::policy_categorical(a.cfg, hd + 1, A, in_a, in_logp[0], adv, term, ent, dl);
                    }
                    s_pol += term;
#pragma unroll
                    for (int k = 0; k < srlxp::kCatMax; k++) sd[1 + k] = dl[k];
                } else {
                    for (int d = 0; d < A; d++) {
                        float term, e1;
                        if constexpr (KL) {
                            const float *od = L.seeds + tid * HS;
                            float kl;
                            srlxp::policy_normal_kl(a.cfg, a.kl.beta[0], hd[1 + d], hd[1 + A + d], in_act[d], in_logp[d], od[1 + d], od[5 + d], adv, term, e1, kl, sd[1 + d], sd[5 + d]);
                            s_kl += kl;
                        } else {
                            srlxp::policy_normal(a.cfg, hd[1 + d], hd[1 + A + d], in_act[d], in_logp[d], adv, term, e1, sd[1 + d], sd[5 + d]);
                        }
                        s_pol += term;
                        ent += e1;
                    }
                }
                s_ent += ent;
                s_val += srlxp::value_term(a.cfg, v, in_vt, a.cfg.value_clip ? in_val : 0.f, sd[0]);
            }
#pragma unroll
            for (int q = 0; q < HS; q += 4) st4(L.seeds + tid * HS + q, make_float4(sd[q], sd[q + 1], sd[q + 2], sd[q + 3]));
        }
        __syncthreads();
        // ---- the heads' gradients, and the gradients at the value / policy blocks' pre-activations in place of their activations ----
#pragma unroll 4
        for (int s = s_lo; s < s_lo + 16; s++) {
            const float4 q0 = ld4(L.seeds + s * HS), q1 = ld4(L.seeds + s * HS + 4), q2 = ld4(L.seeds + s * HS + 8);
            const float sloc[4] = {q0.y, q0.z, q0.w, q1.x}, sls[4] = {q1.y, q1.z, q1.w, q2.x};
            const float hv = L.hv[s * LD + u], hp = L.hp[s * LD + u];
            g_wvo = fmaf(q0.x, hv, g_wvo);
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < A_MAX; d++) {
                g_wloc[d] = fmaf(sloc[d], hp, g_wloc[d]);
                g_wls[d] = fmaf(sls[d], hp, g_wls[d]);
                acc = fmaf(sloc[d], wloc_u[d], acc);
                acc = fmaf(sls[d], wls_u[d], acc);
            }
            if (u < HS) g_head_b += L.seeds[s * HS + u];
            const float zv = hv > 0.f ? q0.x * wvo_u : 0.f, zp = hp > 0.f ? acc : 0.f;
            g_bv += zv, g_bp += zp;
            L.hv[s * LD + u] = zv, L.hp[s * LD + u] = zp;  // (this thread read them, this thread replaces them)
        }
        __syncthreads();
        // ---- value / policy blocks: weight gradients, and the gradient at the trunk's second pre-activation ----
        g_wv = mfma_wgrad(g_wv, L.hv, L.h2, m0, n0);
        g_wp = mfma_wgrad(g_wp, L.hp, L.h2, m0, n0);
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            acc = mfma_dgrad(acc, L.hv, L.wv, m0, n0);
            acc = mfma_dgrad(acc, L.hp, L.wp, m0, n0);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int at = (m0 + acc_row(r)) * LD + n0 + li;
                L.d2[at] = L.h2[at] > 0.f ? acc[r] : 0.f;
            }
        }
        __syncthreads();
        // ---- trunk, second layer: weight gradient; the gradient at the first pre-activation goes where hv was ----
        g_w2 = mfma_wgrad(g_w2, L.d2, L.h1, m0, n0);
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            acc = mfma_dgrad(acc, L.d2, L.w2, m0, n0);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int at = (m0 + acc_row(r)) * LD + n0 + li;
                L.hv[at] = L.h1[at] > 0.f ? acc[r] : 0.f;
            }
        }
        __syncthreads();
        // ---- trunk, first layer ----
#pragma unroll 4
        for (int s = s_lo; s < s_lo + 16; s++) {
            const float d = L.hv[s * LD + u];
            const float4 x0 = ld4(L.x + s * OBS_MAX), x1 = ld4(L.x + s * OBS_MAX + 4);
            g_b1 += d;
            g_b2 += L.d2[s * LD + u];
            g_w1[0] = fmaf(d, x0.x, g_w1[0]), g_w1[1] = fmaf(d, x0.y, g_w1[1]), g_w1[2] = fmaf(d, x0.z, g_w1[2]), g_w1[3] = fmaf(d, x0.w, g_w1[3]);
            g_w1[4] = fmaf(d, x1.x, g_w1[4]), g_w1[5] = fmaf(d, x1.y, g_w1[5]), g_w1[6] = fmaf(d, x1.z, g_w1[6]), g_w1[7] = fmaf(d, x1.w, g_w1[7]);
        }
    }
    // ---- the four parts of every vector meet (part 0 + 1 + 2 + 3, in that order), through the activations' LDS ----
    __syncthreads();
    {
        static_assert(4 * kVecs * H <= 2 * S * LD, "the partial sums' scratch spans h1 and h2");
        float *sc = L.h1 + part * kVecs * H;  // [part][vector][unit] (h1 and h2 are adjacent and dead by now)
        int q = 0;
        sc[(q++) * H + u] = g_b1, sc[(q++) * H + u] = g_b2, sc[(q++) * H + u] = g_bv, sc[(q++) * H + u] = g_bp, sc[(q++) * H + u] = g_wvo, sc[(q++) * H + u] = g_head_b;
        for (int d = 0; d < A_MAX; d++) sc[(q++) * H + u] = g_wloc[d], sc[(q++) * H + u] = g_wls[d];
        for (int c = 0; c < OBS_MAX; c++) sc[(q++) * H + u] = g_w1[c];
    }
    __syncthreads();
    if (part == 0) {
        const int per = kVecs * H;
        auto total = [&](int q) { return ((L.h1[q * H + u] + L.h1[per + q * H + u]) + L.h1[2 * per + q * H + u]) + L.h1[3 * per + q * H + u]; };
        int q = 0;
        g_b1 = total(q++), g_b2 = total(q++), g_bv = total(q++), g_bp = total(q++), g_wvo = total(q++), g_head_b = total(q++);
        for (int d = 0; d < A_MAX; d++) g_wloc[d] = total(q++), g_wls[d] = total(q++);
        for (int c = 0; c < OBS_MAX; c++) g_w1[c] = total(q++);
    }
    // ---- this workgroup's sums -> HBM ----
    float *out = a.partials + (i64)blockIdx.x * a.stride;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int at = (m0 + acc_row(r)) * H + n0 + li;
        out[o.w2 + at] = g_w2[r], out[o.wv + at] = g_wv[r], out[o.wp + at] = g_wp[r];
    }
    if (tid < H) {
        for (int c = 0; c < obs; c++) out[o.w1 + tid * obs + c] = g_w1[c];
        out[o.b1 + tid] = g_b1, out[o.b2 + tid] = g_b2, out[o.bv + tid] = g_bv, out[o.bp + tid] = g_bp, out[o.wvo + tid] = g_wvo;
        if (tid == 0) out[o.bvo] = g_head_b;
        if constexpr (CAT) {
#pragma unroll
            for (int d = 0; d < A_MAX; d++) {
                if (d < A) out[o.wloc + d * H + tid] = g_wloc[d];
                if (A_MAX + d < A) out[o.wloc + (A_MAX + d) * H + tid] = g_wls[d];
            }
            if (tid >= 1 && tid <= A) out[o.bloc + tid - 1] = g_head_b;
        } else {
            for (int d = 0; d < A; d++) out[o.wloc + d * H + tid] = g_wloc[d], out[o.wls + d * H + tid] = g_wls[d];
            if (tid >= 1 && tid <= A) out[o.bloc + tid - 1] = g_head_b;
            if (tid >= 5 && tid < 5 + A) out[o.bls + tid - 5] = g_head_b;
        }
    }
    __syncthreads();
    if (tid < S) L.red[tid] = s_pol, L.red[S + tid] = s_val, L.red[2 * S + tid] = s_ent;
    if constexpr (KL) {
        if (tid < S) L.seeds[tid] = s_kl;  // (the seeds table is dead by now)
    }
    __syncthreads();
    if (tid < 3) {
        float acc = 0.f;
        for (int s = 0; s < S; s++) acc += L.red[tid * S + s];
        out[o.total + tid] = acc;
    }
    if constexpr (KL) {
        if (tid == 3) {
            float acc = 0.f;
            for (int s = 0; s < S; s++) acc += L.seeds[s];
            out[o.total + 3] = acc;
        }
    }
}

// partial[w][p] -> grad[p]: four lanes per parameter, each sums every fourth partial in ascending order, then (s0 + s1) + (s2 + s3) -- a fixed order: deterministic.
// The three loss sums -> the values the reference reports (weighted means).
// KL (k_ppo_reduce_kl): a fourth loss sum, kl; the lane that forms kl_mean adapts beta (ppo.py:279-287) -- the minibatch launch in front of this one has read beta, the
// next one reads what this lane writes: stream order.  losses [5]: policy, value, entropy, kl_mean, beta as adapted.
struct ReduceKl {
    float *beta;
    double lo, hi;  // target / 1.5, target * 1.5
};
struct NoKl {};
template <bool KL>
__device__ __forceinline__ void reduce_partials(int n_wg, int P, int stride, const float *__restrict__ partials, float *__restrict__ grad, float *__restrict__ losses, const LossCfg &cfg,
                                                const std::conditional_t<KL, ReduceKl, NoKl> &kl) {
    constexpr int NL = KL ? 4 : 3;
    const int t = blockIdx.x * 256 + threadIdx.x, p = t >> 2, q = t & 3;
    float acc = 0.f;
    if (p < P + NL) {
#pragma unroll 8
        for (int w = q; w < n_wg; w += 4) acc += partials[(i64)w * stride + p];
    }
    const float a1 = __shfl_xor(acc, 1);
    acc = (q & 1) ? a1 + acc : acc + a1;  // (both lanes of a pair hold s_even + s_odd, added in that order)
    const float a2 = __shfl_xor(acc, 2);
    acc = (q & 2) ? a2 + acc : acc + a2;
    if (q != 0 || p >= P + NL) return;
    if constexpr (KL) {
        if (p == P + 3) {
            const float kl_mean = cfg.inv_bk * acc, nb = srlxp::kl_adapt_beta(kl.beta[0], kl_mean, kl.lo, kl.hi);
            kl.beta[0] = nb;
            if (losses) losses[3] = kl_mean, losses[4] = nb;
            return;
        }
    }
    if (p < P)
        grad[p] = acc;
    else if (losses)
        losses[p - P] = p - P == 0 ? -cfg.inv_bk * acc : (p - P == 1 ? cfg.value_w * cfg.inv_b * acc : cfg.entropy_w * -cfg.inv_b * acc);
}
__global__ void __launch_bounds__(256) k_ppo_reduce(int n_wg, int P, int stride, const float *__restrict__ partials, float *__restrict__ grad, float *__restrict__ losses, LossCfg cfg) {
    reduce_partials<false>(n_wg, P, stride, partials, grad, losses, cfg, NoKl{});
}
__global__ void __launch_bounds__(256) k_ppo_reduce_kl(int n_wg, int P, int stride, const float *__restrict__ partials, float *__restrict__ grad, float *__restrict__ losses, LossCfg cfg,
                                                       ReduceKl kl) {
    reduce_partials<true>(n_wg, P, stride, partials, grad, losses, cfg, kl);
}

// The gradient scaled by grad_scale (1 / world size behind the data-parallel all-reduce); global-norm clip; Adam.
// SCHED: the rate is lr * factor(schedule, steps taken) (srlx_lr_math.h); false: lr as it is, and no trace of the schedule in the code or the arguments.
struct NoSchedule {};
template <bool SCHED>
__global__ void __launch_bounds__(1024) k_ppo_adam(int P, float *__restrict__ params, const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v, i64 *__restrict__ step,
                                                    double lr, std::conditional_t<SCHED, srlx_lr_schedule_t, NoSchedule> sched, double b1, double b2, double eps, float max_norm, float grad_scale) {
    // ceil(P / 1024) workgroups: every one computes the WHOLE vector's norm (52 KB out of L2, the same sums in the same order everywhere), then steps its own 1 024
    // parameters -- no grid-wide exchange for the clip factor; the last workgroup out (step[1]: an arrival counter) advances the step count.
    __shared__ float red[1024];
    constexpr int kPer = 16;  // elements per thread of the norm pass (>= the largest geometry's 14.3 K / 1024), fully unrolled: every load in flight at once
    const int tid = threadIdx.x, mine = blockIdx.x * 1024 + tid;
    const i64 steps_taken = step[0];
    const bool in_mine = mine < P;
    float pp = 0.f, mm = 0.f, vv = 0.f;
    if (in_mine) pp = params[mine], mm = m[mine], vv = v[mine];
    // The rate of THIS step, evaluated by one lane beside the norm pass and handed over through LDS behind the reduction's barriers -- a captured graph follows the
    // schedule from the step count alone.
    __shared__ double lr_shared;  // (SCHED only)
    if constexpr (SCHED) {
        if (tid == 1023) lr_shared = lr * srlx::lr_factor(sched, steps_taken, lr);
    }
    float g[kPer];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int p = tid + 1024 * k;
        g[k] = p < P ? grad[p] * grad_scale : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kPer; k++) ss = fmaf(g[k], g[k], ss);
    red[tid] = ss;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float clip = max_norm > 0.f ? fminf(max_norm / (sqrtf(red[0]) + 1e-6f), 1.0f) : 1.0f;  // torch.nn.utils.clip_grad_norm_
    if (in_mine) {
        double lr_now = lr;
        if constexpr (SCHED) lr_now = lr_shared;
        const srlx::AdamCoef c = srlx::adam_coef(lr_now, b1, b2, eps, steps_taken);
        float gc = 0.f;
#pragma unroll
        for (int k = 0; k < kPer; k++)
            if (k == (int)blockIdx.x) gc = g[k] * clip;  // (this thread's own element is g[blockIdx.x]: selected without a run-time register index)
        srlx::adam_one(pp, gc, mm, vv, c);  // (`grad` itself stays as it is: every workgroup reads all of it for the norm)
        params[mine] = pp, m[mine] = mm, v[mine] = vv;
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long *>(step + 1), 1ull);
        if (old == gridDim.x - 1) {  // every workgroup has read step[0] (it arrives behind that read)
            step[1] = 0;
            step[0] = steps_taken + 1;
        }
    }
}

// baseline_type "ave" / "std" / "normal" (ppo.py:222-233) over one minibatch of at most E T / minibatches elements.  Up to 16 workgroups, and EVERY one computes the
// whole minibatch's statistics (the same sums in the same order everywhere: no grid-wide exchange, as k_ppo_adam does for the norm), then transforms its own
// slice -- measured at 32 768 elements: one workgroup making every pass from HBM 90.5 us, with the gather staged in LDS 63.6 us, and what is left is one CU's
// address pipe working through 32 768 scattered reads and 32 768 scattered writes plus the float64 divisions; the slices divide the writes and the divisions.
// The gather adv[rows[i]] is made ONCE per workgroup, 16 elements per lane in flight at a time, into LDS (the
// first kBaseStage = 32 768 elements: 128 KiB; what a larger minibatch has beyond them is read again from HBM in every pass), and the three passes -- the sum, the sum
// of squared deviations from the mean (no cancellation at mean >> spread), the transform -- read it there.  Each lane adds its elements i = tid, tid + 1024, ... in
// ascending order into a float64, the 1 024 lane sums meet in a fixed tree: deterministic.  The population deviation, and 1e-8 beside it, as numpy's in the
// reference.  The quotient is formed in float64 and rounded to float32 once.
constexpr i64 kBaseStage = 32 * 1024;
__device__ __forceinline__ double block_sum_1024(double x, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();  // (the previous use of `red` is over; the staged values are written)
    red[tid] = x;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(1024) k_ppo_adv_baseline(i64 mb, const i64 *__restrict__ rows, const float *__restrict__ adv, int mode, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float *xs = reinterpret_cast<float *>(lds_raw);  // [min(mb, kBaseStage)]
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    const i64 staged = mb < kBaseStage ? mb : kBaseStage;
    for (i64 base = 0; base < staged; base += 16 * 1024) {
        i64 r[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const i64 i = base + tid + 1024 * k;
            r[k] = i < staged ? rows[i] : -1;
        }
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (r[k] >= 0) xs[base + tid + 1024 * k] = adv[r[k]];
    }
    __syncthreads();  // (the last pass reads what other lanes staged)
    auto at = [&](i64 i) { return i < staged ? xs[i] : adv[rows[i]]; };
    double s = 0.0;
    for (i64 i = tid; i < mb; i += 1024) s += (double)at(i);
    const double mean = block_sum_1024(s, red) / (double)mb;
    double q = 0.0;
    for (i64 i = tid; i < mb; i += 1024) {
        const double d = (double)at(i) - mean;
        q += d * d;
    }
    const double sd = sqrt(block_sum_1024(q, red) / (double)mb) + 1e-8;
    for (i64 i = (i64)blockIdx.x * 1024 + tid; i < mb; i += (i64)gridDim.x * 1024) {  // this workgroup's slice
        const double a = (double)at(i);
        out[rows[i]] = (float)(mode == SRLX_PPO_BASELINE_AVE ? a - mean : (mode == SRLX_PPO_BASELINE_STD ? a / sd : (a - mean) / sd));
    }
}

static_assert(H * OBS_MAX + 3 * H * H + 2 * A_MAX * H + 5 * H + 1 + 2 * A_MAX <= 16 * 1024, "k_ppo_adam: sixteen elements per thread");
// categorical: 2 .. 8 actions -- the heads table's eight policy slots per row; more would widen the tables and the backward's fixed extents
template <bool CAT>
bool geometry_ok(int obs, int A) {
    return obs >= 1 && obs <= OBS_MAX && (CAT ? A >= 2 && A <= srlxp::kCatMax : A >= 1 && A <= A_MAX);
}
template <bool CAT>
int param_count(int obs, int A) {
    return geometry_ok<CAT>(obs, A) ? net_off_of<CAT>(obs, A).total : -1;
}
constexpr int partials_stride(int params) { return (params + 3 + 3) & ~3; }  // per-workgroup gradient sums + 3 loss sums, 16-byte rows
template <bool CAT>
int partials_floats(int obs, int A) {
    return geometry_ok<CAT>(obs, A) ? 256 * partials_stride(net_off_of<CAT>(obs, A).total) : -1;
}
constexpr int partials_stride_kl(int params) { return (params + 4 + 3) & ~3; }  // ... + 4 loss sums
template <bool CAT>
int partials_floats_kl(int obs, int A) {
    return geometry_ok<CAT>(obs, A) ? 256 * partials_stride_kl(net_off_of<CAT>(obs, A).total) : -1;
}
constexpr size_t kLdsMax = 160 * 1024;  // a workgroup's LDS (gfx950)

template <class Task>
int rollout_max_horizon(int A) {  // what fits the workgroup's LDS beside weights and activations
    if (!geometry_ok<Task::CAT>(Task::OBS, A)) return -1;
    const long long t = ((long long)kLdsMax - (long long)sizeof(FwdLds)) / ((long long)RE * Task::records(A) * (long long)sizeof(float));
    return (int)(t < 1024 ? t : 1024);
}

template <class Task, bool EX, bool KL>
int launch_rollout_kernel(const RolloutArgsOf<Task, KL> &a, size_t lds, void *stream) {
    static size_t lds_set = 0;
    if (lds > lds_set) {
        SRLX_HIP(hipFuncSetAttribute((const void *)k_ppo_rollout<Task, EX, KL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set = lds;
    }
    hipLaunchKernelGGL((k_ppo_rollout<Task, EX, KL>), dim3((unsigned)(a.E / RE)), dim3(256), lds, (hipStream_t)stream, a);
    return SRLX_OK;
}

// name: the entry point's, for its error texts
// kl: NULL = the rollout as it is; else the "kl" surrogate's record of the acting distribution
template <class Task>
int launch_rollout(const char *name, const RolloutArgs<Task> &a, void *stream, const RolloutKl *kl = nullptr) {
    SRLX_REQUIRE(a.E > 0 && a.E % RE == 0, "%s: the environment count must be a multiple of 16", name);
    SRLX_REQUIRE(a.T > 0 && geometry_ok<Task::CAT>(Task::OBS, a.A) && a.T <= rollout_max_horizon<Task>(a.A) && a.episode_len > 0,
                 "%s: bad geometry (horizon <= srlx_%s_max_horizon)", name, name);
    SRLX_REQUIRE(a.params && Task::env_ok(a.env) && a.env_obs && a.act_counter && a.b_obs && a.b_act && a.b_logp && a.b_val && a.b_rew && a.b_done && a.b_adv && a.last_v &&
                     a.episode_return && a.finished,
                 "%s: NULL argument", name);
    SRLX_REQUIRE((!a.opts.reward_clip || a.opts.reward_lo <= a.opts.reward_hi) && (!a.opts.state_clip || a.opts.state_lo <= a.opts.state_hi), "%s: a clip's lower bound exceeds its upper bound",
                 name);
    SRLX_REQUIRE(!Task::CAT || !rescales(a.opts), "%s: the action rescale belongs to the Normal head", name);
    const size_t lds = sizeof(FwdLds) + (size_t)a.T * RE * Task::records(a.A) * sizeof(float);
    SRLX_REQUIRE(lds <= kLdsMax, "%s: horizon too long for the workgroup's LDS", name);
    const bool ex = a.opts.reward_clip || a.opts.state_clip || rescales(a.opts);  // all off: the kernel without the options' code
    int st;
    if (kl) {
        SRLX_REQUIRE(kl->d0 && (Task::CAT || kl->d1), "%s: NULL buffer for the acting distribution", name);
        RolloutArgsOf<Task, true> k;
        static_cast<RolloutArgs<Task> &>(k) = a;
        k.kl = *kl;
        st = ex ? launch_rollout_kernel<Task, true, true>(k, lds, stream) : launch_rollout_kernel<Task, false, true>(k, lds, stream);
    } else {
        RolloutArgsOf<Task, false> k;
        static_cast<RolloutArgs<Task> &>(k) = a;
        st = ex ? launch_rollout_kernel<Task, true, false>(k, lds, stream) : launch_rollout_kernel<Task, false, false>(k, lds, stream);
    }
    if (st != SRLX_OK) return st;
    Task::advance(a.env, a.act_counter, a.T, (hipStream_t)stream);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

template <bool CAT>
int launch_forward(i64 n, int obs, int A, const float *params, const float *x, float *v, float *h0, float *h1, void *stream) {
    static bool attr = false;
    if (!attr) {
        SRLX_HIP(hipFuncSetAttribute((const void *)k_ppo_forward<CAT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(FwdLds)));
        attr = true;
    }
    i64 wgs = (n + RE - 1) / RE;
    if (wgs > 1024) wgs = 1024;
    hipLaunchKernelGGL(k_ppo_forward<CAT>, dim3((unsigned)wgs), dim3(256), sizeof(FwdLds), (hipStream_t)stream, (i64)n, obs, A, params, x, v, h0, h1);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

template <bool CAT>
int launch_minibatch(MbArgs &a, float *d_grad, float *d_losses, void *stream) {
    static bool attr = false;
    if (!attr) {
        SRLX_HIP(hipFuncSetAttribute((const void *)k_ppo_minibatch<CAT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MbLds)));
        attr = true;
    }
    const NetOff o = net_off_of<CAT>(a.obs, a.A);
    a.stride = partials_stride(o.total);
    const i64 tiles = (a.mb + S - 1) / S;
    const int wgs = (int)(tiles < 256 ? tiles : 256);
    MbArgsOf<false> k;
    static_cast<MbArgs &>(k) = a;
    hipLaunchKernelGGL(k_ppo_minibatch<CAT>, dim3((unsigned)wgs), dim3(256), sizeof(MbLds), (hipStream_t)stream, k);
    hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)((4 * (o.total + 3) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wgs, o.total, a.stride, a.partials, d_grad, d_losses, a.cfg);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

// the "kl" surrogate's two launches: the same shape, the KL instantiations; partials [srlx_ppo_*_kl_partials_floats]
template <bool CAT>
int launch_minibatch_kl(const char *name, MbArgs &a, const float *b_old0, const float *b_old1, double kl_target, float *d_kl_beta, float *d_grad, float *d_losses, void *stream) {
    SRLX_REQUIRE(b_old0 && (CAT || b_old1) && d_kl_beta && kl_target > 0, "%s: the old distribution's buffers, the beta state and a positive adaptive_kl_target", name);
    static bool attr = false;
    if (!attr) {
        SRLX_HIP(hipFuncSetAttribute((const void *)k_ppo_minibatch<CAT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MbLds)));
        attr = true;
    }
    const NetOff o = net_off_of<CAT>(a.obs, a.A);
    a.stride = partials_stride_kl(o.total);
    const i64 tiles = (a.mb + S - 1) / S;
    const int wgs = (int)(tiles < 256 ? tiles : 256);
    MbArgsOf<true> k;
    static_cast<MbArgs &>(k) = a;
    k.kl = MbKl{b_old0, b_old1, d_kl_beta};
    hipLaunchKernelGGL((k_ppo_minibatch<CAT, true>), dim3((unsigned)wgs), dim3(256), sizeof(MbLds), (hipStream_t)stream, k);
    hipLaunchKernelGGL(k_ppo_reduce_kl, dim3((unsigned)((4 * (o.total + 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wgs, o.total, a.stride, a.partials, d_grad, d_losses, a.cfg,
                       ReduceKl{d_kl_beta, kl_target / 1.5, kl_target * 1.5});
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

constexpr srlx_lr_schedule_t kLrConstant = {SRLX_LR_CONSTANT, 0, 0, 0.0, 0.0, {}, {}};

int launch_adam(const char *name, int P, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step, double lr, const srlx_lr_schedule_t *sched, double beta1,
                double beta2, double eps, double max_grad_norm, double grad_scale, void *stream) {
    SRLX_REQUIRE(sched && srlx::lr_schedule_ok(*sched) && (sched->kind == SRLX_LR_CONSTANT || lr > 0), "%s: bad learning-rate schedule", name);
    const dim3 grid((unsigned)((P + 1023) / 1024)), block(1024);
    if (sched->kind == SRLX_LR_CONSTANT)  // the kernel without the schedule's code and arguments
        hipLaunchKernelGGL(k_ppo_adam<false>, grid, block, 0, (hipStream_t)stream, P, d_params, d_grad, d_exp_avg, d_exp_avg_sq, (i64 *)d_step, lr, NoSchedule{}, beta1, beta2, eps,
                           (float)max_grad_norm, (float)grad_scale);
    else
        hipLaunchKernelGGL(k_ppo_adam<true>, grid, block, 0, (hipStream_t)stream, P, d_params, d_grad, d_exp_avg, d_exp_avg_sq, (i64 *)d_step, lr, *sched, beta1, beta2, eps,
                           (float)max_grad_norm, (float)grad_scale);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // namespace

extern "C" {

int srlx_ppo_net_param_count(int obs_dim, int action_dim) { return param_count<false>(obs_dim, action_dim); }

int srlx_ppo_net_forward(int64_t n, int obs_dim, int action_dim, const float *d_params, const float *d_obs, float *d_v, float *d_loc, float *d_log_scale, void *stream) {
    SRLX_REQUIRE(n > 0 && geometry_ok<false>(obs_dim, action_dim) && d_params && d_obs && d_v && d_loc && d_log_scale, "ppo_net_forward: bad argument");
    return launch_forward<false>(n, obs_dim, action_dim, d_params, d_obs, d_v, d_loc, d_log_scale, stream);
}

int srlx_ppo_net_rollout_max_horizon(int action_dim) { return rollout_max_horizon<PendulumNormal>(action_dim); }

int srlx_ppo_net_rollout_ex(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state, int32_t *d_step_in_episode, float *d_env_obs,
                            int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter, uint64_t act_seed, int64_t *d_act_counter, double log_scale_min,
                            double log_scale_max, double discount, double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                            uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished, const srlx_ppo_env_opts_t *opts, void *stream) {
    const RolloutArgs<PendulumNormal> a{n_envs, horizon, action_dim, d_params, d_env_obs, episode_len, (u64)env_seed, (u64)act_seed, d_act_counter,
                                        {d_env_state, d_step_in_episode, d_env_counter, (float)log_scale_min, (float)log_scale_max}, discount, gae_lambda, d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv,
                                        d_last_v, d_episode_return, d_finished, opts ? *opts : kEnvOptsOff};
    return launch_rollout("ppo_net_rollout", a, stream);
}

int srlx_ppo_net_rollout(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state, int32_t *d_step_in_episode, float *d_env_obs,
                         int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter, uint64_t act_seed, int64_t *d_act_counter, double log_scale_min,
                         double log_scale_max, double discount, double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                         uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished, void *stream) {
    return srlx_ppo_net_rollout_ex(n_envs, horizon, action_dim, d_params, d_env_state, d_step_in_episode, d_env_obs, episode_len, env_seed, d_env_counter, act_seed, d_act_counter,
                                   log_scale_min, log_scale_max, discount, gae_lambda, d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv, d_last_v, d_episode_return,
                                   d_finished, nullptr, stream);
}

int srlx_ppo_net_minibatch(int64_t minibatch, const int64_t *d_rows, int obs_dim, int action_dim, const float *d_params, const float *d_b_obs, const float *d_b_act,
                           const float *d_b_logp, const float *d_b_adv, const float *d_b_v_target, const float *d_b_val, double log_scale_min, double log_scale_max,
                           int baseline_advantage, int surrogate_clip, double policy_clip_range, int enable_value_clip, double value_clip_range, double value_loss_weight,
                           double entropy_weight, float *d_partials, float *d_grad, float *d_losses, void *stream) {
    SRLX_REQUIRE(minibatch > 0 && geometry_ok<false>(obs_dim, action_dim), "ppo_net_minibatch: bad geometry");
    SRLX_REQUIRE(d_rows && d_params && d_b_obs && d_b_act && d_b_logp && d_b_adv && d_b_v_target && d_b_val && d_partials && d_grad, "ppo_net_minibatch: NULL argument");
    MbArgs a{};
    a.mb = minibatch;
    a.perm = d_rows;
    a.obs = obs_dim, a.A = action_dim;
    a.params = d_params;
    a.b_obs = d_b_obs, a.b_act = d_b_act, a.b_logp = d_b_logp, a.b_adv = d_b_adv, a.b_vt = d_b_v_target, a.b_val = d_b_val;
    a.cfg = LossCfg{(float)log_scale_min, (float)log_scale_max, baseline_advantage, surrogate_clip, enable_value_clip, (float)policy_clip_range, (float)value_clip_range,
                    (float)value_loss_weight, (float)entropy_weight, 1.0f / (float)minibatch, 1.0f / (float)(minibatch * action_dim)};
    a.partials = d_partials;
    return launch_minibatch<false>(a, d_grad, d_losses, stream);
}

int srlx_ppo_net_partials_floats(int obs_dim, int action_dim) { return partials_floats<false>(obs_dim, action_dim); }

int srlx_ppo_net_kl_partials_floats(int obs_dim, int action_dim) { return partials_floats_kl<false>(obs_dim, action_dim); }

int srlx_ppo_net_rollout_kl(int64_t n_envs, int64_t horizon, int action_dim, const float *d_params, float *d_env_state, int32_t *d_step_in_episode, float *d_env_obs,
                            int64_t episode_len, uint64_t env_seed, int64_t *d_env_counter, uint64_t act_seed, int64_t *d_act_counter, double log_scale_min,
                            double log_scale_max, double discount, double gae_lambda, float *d_b_obs, float *d_b_act, float *d_b_logp, float *d_b_val, float *d_b_rew,
                            uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished, float *d_b_loc, float *d_b_log_scale,
                            const srlx_ppo_env_opts_t *opts, void *stream) {
    const RolloutArgs<PendulumNormal> a{n_envs, horizon, action_dim, d_params, d_env_obs, episode_len, (u64)env_seed, (u64)act_seed, d_act_counter,
                                        {d_env_state, d_step_in_episode, d_env_counter, (float)log_scale_min, (float)log_scale_max}, discount, gae_lambda, d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv,
                                        d_last_v, d_episode_return, d_finished, opts ? *opts : kEnvOptsOff};
    const RolloutKl kl{d_b_loc, d_b_log_scale};
    return launch_rollout("ppo_net_rollout_kl", a, stream, &kl);
}

int srlx_ppo_net_minibatch_kl(int64_t minibatch, const int64_t *d_rows, int obs_dim, int action_dim, const float *d_params, const float *d_b_obs, const float *d_b_act,
                              const float *d_b_logp, const float *d_b_adv, const float *d_b_v_target, const float *d_b_val, const float *d_b_loc, const float *d_b_log_scale,
                              double log_scale_min, double log_scale_max, int baseline_advantage, int enable_value_clip, double value_clip_range, double value_loss_weight,
                              double entropy_weight, double adaptive_kl_target, float *d_kl_beta, float *d_partials, float *d_grad, float *d_losses, void *stream) {
    SRLX_REQUIRE(minibatch > 0 && geometry_ok<false>(obs_dim, action_dim), "ppo_net_minibatch_kl: bad geometry");
    SRLX_REQUIRE(d_rows && d_params && d_b_obs && d_b_act && d_b_logp && d_b_adv && d_b_v_target && d_b_val && d_partials && d_grad, "ppo_net_minibatch_kl: NULL argument");
    MbArgs a{};
    a.mb = minibatch;
    a.perm = d_rows;
    a.obs = obs_dim, a.A = action_dim;
    a.params = d_params;
    a.b_obs = d_b_obs, a.b_act = d_b_act, a.b_logp = d_b_logp, a.b_adv = d_b_adv, a.b_vt = d_b_v_target, a.b_val = d_b_val;
    a.cfg = LossCfg{(float)log_scale_min, (float)log_scale_max, baseline_advantage, 0, enable_value_clip, 0.f, (float)value_clip_range, (float)value_loss_weight, (float)entropy_weight,
                    1.0f / (float)minibatch, 1.0f / (float)(minibatch * action_dim)};
    a.partials = d_partials;
    return launch_minibatch_kl<false>("ppo_net_minibatch_kl", a, d_b_loc, d_b_log_scale, adaptive_kl_target, d_kl_beta, d_grad, d_losses, stream);
}

int srlx_ppo_net_adam(int obs_dim, int action_dim, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step, double lr, double beta1, double beta2,
                      double eps, double max_grad_norm, double grad_scale, void *stream) {
    SRLX_REQUIRE(geometry_ok<false>(obs_dim, action_dim) && d_params && d_grad && d_exp_avg && d_exp_avg_sq && d_step, "ppo_net_adam: bad argument");
    return launch_adam("ppo_net_adam", param_count<false>(obs_dim, action_dim), d_params, d_grad, d_exp_avg, d_exp_avg_sq, d_step, lr, &kLrConstant, beta1, beta2, eps, max_grad_norm,
                       grad_scale, stream);
}

int srlx_ppo_net_adam_sched(int obs_dim, int action_dim, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step, double lr,
                            const srlx_lr_schedule_t *schedule, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale, void *stream) {
    SRLX_REQUIRE(geometry_ok<false>(obs_dim, action_dim) && d_params && d_grad && d_exp_avg && d_exp_avg_sq && d_step, "ppo_net_adam_sched: bad argument");
    return launch_adam("ppo_net_adam_sched", param_count<false>(obs_dim, action_dim), d_params, d_grad, d_exp_avg, d_exp_avg_sq, d_step, lr, schedule, beta1, beta2, eps, max_grad_norm,
                       grad_scale, stream);
}

int srlx_lr_factor(const srlx_lr_schedule_t *schedule, int64_t step, double lr, double *out) {
    SRLX_REQUIRE(schedule && out && srlx::lr_schedule_ok(*schedule) && step >= 0 && lr > 0, "lr_factor: bad argument (kind, decay_steps > 0, at most 8 boundaries, step >= 0, lr > 0)");
    *out = srlx::lr_factor(*schedule, step, lr);
    return SRLX_OK;
}

int srlx_ppo_adv_baseline(int64_t minibatch, const int64_t *d_rows, const float *d_b_adv, int mode, float *d_out, void *stream) {
    SRLX_REQUIRE(minibatch > 0 && d_rows && d_b_adv && d_out && d_out != d_b_adv, "ppo_adv_baseline: bad argument (the output is a second buffer)");
    SRLX_REQUIRE(mode >= SRLX_PPO_BASELINE_AVE && mode <= SRLX_PPO_BASELINE_NORMAL, "ppo_adv_baseline: mode is SRLX_PPO_BASELINE_AVE / _STD / _NORMAL");
    const size_t lds = (size_t)(minibatch < kBaseStage ? minibatch : kBaseStage) * sizeof(float);
    static size_t lds_set = 0;
    if (lds > lds_set) {
        SRLX_HIP(hipFuncSetAttribute((const void *)k_ppo_adv_baseline, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set = lds;
    }
    const int64_t wgs = (minibatch + 1023) / 1024;
    hipLaunchKernelGGL(k_ppo_adv_baseline, dim3((unsigned)(wgs < 16 ? wgs : 16)), dim3(1024), lds, (hipStream_t)stream, (i64)minibatch, d_rows, d_b_adv, mode, d_out);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

// ---- the categorical head ---------------------------------------------------------------------------------------------------------------------------------------------
int srlx_ppo_cat_param_count(int obs_dim, int n_actions) { return param_count<true>(obs_dim, n_actions); }

int srlx_ppo_cat_partials_floats(int obs_dim, int n_actions) { return partials_floats<true>(obs_dim, n_actions); }

int srlx_ppo_cat_rollout_max_horizon(int n_actions) { return rollout_max_horizon<CartPoleCategorical>(n_actions); }

int srlx_ppo_cat_kl_partials_floats(int obs_dim, int n_actions) { return partials_floats_kl<true>(obs_dim, n_actions); }

int srlx_ppo_cat_rollout_kl(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps, int32_t *d_episodes, float *d_env_obs,
                            int64_t max_steps, uint64_t env_seed, uint64_t act_seed, int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act,
                            float *d_b_logp, float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished,
                            float *d_b_probs, const srlx_ppo_env_opts_t *opts, void *stream) {
    const RolloutArgs<CartPoleCategorical> a{n_envs, horizon, n_actions, d_params, d_env_obs, max_steps, (u64)env_seed, (u64)act_seed, d_act_counter,
                                             {d_env_state, d_steps, d_episodes}, discount, gae_lambda, d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv, d_last_v, d_episode_return, d_finished,
                                             opts ? *opts : kEnvOptsOff};
    const RolloutKl kl{d_b_probs, nullptr};
    return launch_rollout("ppo_cat_rollout_kl", a, stream, &kl);
}

int srlx_ppo_cat_minibatch_kl(int64_t minibatch, const int64_t *d_rows, int obs_dim, int n_actions, const float *d_params, const float *d_b_obs, const int32_t *d_b_act,
                              const float *d_b_logp, const float *d_b_adv, const float *d_b_v_target, const float *d_b_val, const float *d_b_probs, int baseline_advantage,
                              int enable_value_clip, double value_clip_range, double value_loss_weight, double entropy_weight, double adaptive_kl_target, float *d_kl_beta,
                              float *d_partials, float *d_grad, float *d_losses, void *stream) {
    SRLX_REQUIRE(minibatch > 0 && geometry_ok<true>(obs_dim, n_actions), "ppo_cat_minibatch_kl: bad geometry");
    SRLX_REQUIRE(d_rows && d_params && d_b_obs && d_b_act && d_b_logp && d_b_adv && d_b_v_target && d_b_val && d_partials && d_grad, "ppo_cat_minibatch_kl: NULL argument");
    MbArgs a{};
    a.mb = minibatch;
    a.perm = d_rows;
    a.obs = obs_dim, a.A = n_actions;
    a.params = d_params;
    a.b_obs = d_b_obs, a.b_act = reinterpret_cast<const float *>(d_b_act), a.b_logp = d_b_logp, a.b_adv = d_b_adv, a.b_vt = d_b_v_target, a.b_val = d_b_val;
    a.cfg = LossCfg{0.f, 0.f, baseline_advantage, 0, enable_value_clip, 0.f, (float)value_clip_range, (float)value_loss_weight, (float)entropy_weight, 1.0f / (float)minibatch,
                    1.0f / (float)minibatch};
    a.partials = d_partials;
    return launch_minibatch_kl<true>("ppo_cat_minibatch_kl", a, d_b_probs, nullptr, adaptive_kl_target, d_kl_beta, d_grad, d_losses, stream);
}

int srlx_ppo_cat_forward(int64_t n, int obs_dim, int n_actions, const float *d_params, const float *d_obs, float *d_v, float *d_logits, void *stream) {
    SRLX_REQUIRE(n > 0 && geometry_ok<true>(obs_dim, n_actions) && d_params && d_obs && d_v && d_logits, "ppo_cat_forward: bad argument");
    return launch_forward<true>(n, obs_dim, n_actions, d_params, d_obs, d_v, d_logits, nullptr, stream);
}

int srlx_ppo_cat_rollout_ex(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps, int32_t *d_episodes, float *d_env_obs,
                            int64_t max_steps, uint64_t env_seed, uint64_t act_seed, int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act,
                            float *d_b_logp, float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished,
                            const srlx_ppo_env_opts_t *opts, void *stream) {
    const RolloutArgs<CartPoleCategorical> a{n_envs, horizon, n_actions, d_params, d_env_obs, max_steps, (u64)env_seed, (u64)act_seed, d_act_counter,
                                             {d_env_state, d_steps, d_episodes}, discount, gae_lambda, d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv, d_last_v, d_episode_return, d_finished,
                                             opts ? *opts : kEnvOptsOff};
    return launch_rollout("ppo_cat_rollout", a, stream);
}

int srlx_ppo_cat_rollout(int64_t n_envs, int64_t horizon, int n_actions, const float *d_params, double *d_env_state, int32_t *d_steps, int32_t *d_episodes, float *d_env_obs,
                         int64_t max_steps, uint64_t env_seed, uint64_t act_seed, int64_t *d_act_counter, double discount, double gae_lambda, float *d_b_obs, int32_t *d_b_act,
                         float *d_b_logp, float *d_b_val, float *d_b_rew, uint8_t *d_b_done, float *d_b_adv, float *d_last_v, float *d_episode_return, float *d_finished,
                         void *stream) {
    return srlx_ppo_cat_rollout_ex(n_envs, horizon, n_actions, d_params, d_env_state, d_steps, d_episodes, d_env_obs, max_steps, env_seed, act_seed, d_act_counter, discount, gae_lambda,
                                   d_b_obs, d_b_act, d_b_logp, d_b_val, d_b_rew, d_b_done, d_b_adv, d_last_v, d_episode_return, d_finished, nullptr, stream);
}

int srlx_ppo_cat_minibatch(int64_t minibatch, const int64_t *d_rows, int obs_dim, int n_actions, const float *d_params, const float *d_b_obs, const int32_t *d_b_act,
                           const float *d_b_logp, const float *d_b_adv, const float *d_b_v_target, const float *d_b_val, int baseline_advantage, int surrogate_clip,
                           double policy_clip_range, int enable_value_clip, double value_clip_range, double value_loss_weight, double entropy_weight, float *d_partials,
                           float *d_grad, float *d_losses, void *stream) {
    SRLX_REQUIRE(minibatch > 0 && geometry_ok<true>(obs_dim, n_actions), "ppo_cat_minibatch: bad geometry");
    SRLX_REQUIRE(d_rows && d_params && d_b_obs && d_b_act && d_b_logp && d_b_adv && d_b_v_target && d_b_val && d_partials && d_grad, "ppo_cat_minibatch: NULL argument");
    MbArgs a{};
    a.mb = minibatch;
    a.perm = d_rows;
    a.obs = obs_dim, a.A = n_actions;
    a.params = d_params;
    a.b_obs = d_b_obs, a.b_act = reinterpret_cast<const float *>(d_b_act), a.b_logp = d_b_logp, a.b_adv = d_b_adv, a.b_vt = d_b_v_target, a.b_val = d_b_val;
    a.cfg = LossCfg{0.f, 0.f, baseline_advantage, surrogate_clip, enable_value_clip, (float)policy_clip_range, (float)value_clip_range, (float)value_loss_weight,
                    (float)entropy_weight, 1.0f / (float)minibatch, 1.0f / (float)minibatch};
    a.partials = d_partials;
    return launch_minibatch<true>(a, d_grad, d_losses, stream);
}

int srlx_ppo_cat_adam(int obs_dim, int n_actions, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step, double lr, double beta1, double beta2,
                      double eps, double max_grad_norm, double grad_scale, void *stream) {
    SRLX_REQUIRE(geometry_ok<true>(obs_dim, n_actions) && d_params && d_grad && d_exp_avg && d_exp_avg_sq && d_step, "ppo_cat_adam: bad argument");
    return launch_adam("ppo_cat_adam", param_count<true>(obs_dim, n_actions), d_params, d_grad, d_exp_avg, d_exp_avg_sq, d_step, lr, &kLrConstant, beta1, beta2, eps, max_grad_norm,
                       grad_scale, stream);
}

int srlx_ppo_cat_adam_sched(int obs_dim, int n_actions, float *d_params, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t *d_step, double lr,
                            const srlx_lr_schedule_t *schedule, double beta1, double beta2, double eps, double max_grad_norm, double grad_scale, void *stream) {
    SRLX_REQUIRE(geometry_ok<true>(obs_dim, n_actions) && d_params && d_grad && d_exp_avg && d_exp_avg_sq && d_step, "ppo_cat_adam_sched: bad argument");
    return launch_adam("ppo_cat_adam_sched", param_count<true>(obs_dim, n_actions), d_params, d_grad, d_exp_avg, d_exp_avg_sq, d_step, lr, schedule, beta1, beta2, eps, max_grad_norm,
                       grad_scale, stream);
}

}  // extern "C"
