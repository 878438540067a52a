// srlx_vppo_lanes.hip -- V-PPO's episode store for E lock-stepped lanes (contract in include/srlx.h): the Worker's trackings and the ReplayBuffer
// of algorithms/ppo_v.py as two structures in HBM.
//   tracking ring  time-major [R][E], R = max_episode_steps + 2: row p holds the observation every lane acted on at lock-step p and that step's action,
//                  log-probability, reward, not-terminated and done; s' of row p is row p + 1.  Per lane: the running episode length and the needs_reset byte.
//   item ring      `capacity` items, struct of arrays (s, s', action, old log-probability, reward, not-terminated, total reward); the item with sequence number q
//                  lives in slot q % capacity, as ReplayBuffer.add leaves it; the write count is device-resident and ping-ponged between two words.
//   k_vppo_lanes_store   one thread per observation element: the lock-step's fields, next_obs into the next row, the lanes' lengths, needs_reset, the policy counter
//   k_vppo_lanes_close   one workgroup per lane whose step was done: the returns walked backwards (one float64 chain), the items appended in that order
//   k_vppo_lanes_pick    one wave: Floyd's algorithm on keyed uniforms, B distinct slots
//   k_vppo_lanes_gather  one workgroup per drawn item: the update's dense tensors
//   k_pendulum_lanes     one thread per lane: Pendulum-v1 in float64 under the needs_reset protocol (the Normal head's device environment)
// A push is TWO launches: the close reads every lane's length and done flag to place its items (an exclusive prefix in lane order), and only a launch boundary
// orders those reads behind all lanes' stores.  No atomics: equal inputs give equal bits.
// Two kinds of handle share every kernel: the categorical one keeps one int32 action and one log-probability per step, the Normal one K float32
// action elements and K log-probabilities (K = 1..8).  The kernels take K and move an action as K 32-bit words -- they never read its value, so an int32 and a
// float32 travel alike, bit for bit -- and floor each of the K log-probabilities.
#include "srlx_common.h"
#include "srlx_ppo_math.h"

namespace {

using i64 = int64_t;
using u8 = unsigned char;
using srlx::u64;

constexpr int kThreads = 256;
constexpr int kMaxRing = 4096;  // rows of the tracking ring: the close keeps one lane's rewards and returns in LDS
constexpr int kViews = 16;

struct Ring {
    float *obs;  // [R][E][D]
    int32_t *action;  // [R][E][K] words: int32 actions (K = 1) or float32 action elements
    float *logp;      // [R][E][K]
    float *reward, *nterm;
    u8 *done;  // [R][E]
    int32_t *len;
    u8 *needs_reset;  // [E]
};

struct Items {
    float *s, *s2;  // [capacity][D]
    int32_t *action;  // [capacity][K] words
    float *logp;      // [capacity][K]
    float *reward, *nterm, *total;  // [capacity]
};

}  // namespace

struct srlx_vppo_lanes {
    int E, D, R, device;
    int K;        // words of an action and log-probabilities of a step
    bool normal;  // the words are float32 action elements (srlx_vppo_lanes_create_normal)
    i64 capacity;
    double discount;
    i64 lock_steps;  // pushes since the reset: the current row is lock_steps % R, the count that holds is word lock_steps & 1
    i64 draws;       // samples since the reset: the key of the next draw's uniforms
    Ring r;
    Items it;
    i64 *count;      // [2]
    int32_t *error;  // sticky: 1 an episode outlived the ring, 2 a draw asked for more items than the ring holds
};

namespace {

struct StoreArgs {
    int E, D, R, K;
    i64 row, next_row;
    const int32_t *actions;
    const float *logp, *rewards;
    const u8 *terminated, *done;
    const float *next_obs;
    i64 *policy_counter;  // NULL: none
    int32_t *error;
};

// A lane whose previous step ended an episode (needs_reset) only receives the new episode's first observation: nothing is stored for it and its length
// restarts at 0.  The length of a closed episode stays until then: k_vppo_lanes_close reads it.  A lane that outlived the ring keeps the length -1 until
// that restart, so what is left of its episode never closes: no item with a return cut short at the drop reaches the item ring.
__global__ void __launch_bounds__(kThreads) k_vppo_lanes_store(StoreArgs a, Ring r) {
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    const i64 ED = (i64)a.E * a.D;
    if (i < ED) r.obs[a.next_row * ED + i] = a.next_obs[i];
    if (i < a.E) {
        const bool first = r.needs_reset[i] != 0;
        int n = 0;
        if (!first) {
            const i64 k = a.row * a.E + i;
            for (int j = 0; j < a.K; j++) {
                r.action[k * a.K + j] = a.actions[i * a.K + j];
                r.logp[k * a.K + j] = fmaxf(a.logp[i * a.K + j], srlxp::kLogFloor);  // the Worker floors in on_step, not in policy(); per element
            }
            r.reward[k] = a.rewards[i];
            r.nterm[k] = a.terminated[i] ? 0.f : 1.f;
            r.done[k] = a.done[i] ? 1 : 0;
            n = r.len[i] < 0 ? -1 : r.len[i] + 1;
            if (n > a.R - 2) {  // more steps than max_episode_steps: the next row would reach the episode's first one
                a.error[0] = 1;
                n = -1;
            }
        }
        r.len[i] = n;
        r.needs_reset[i] = a.done[i] ? 1 : 0;
    }
    if (i == 0 && a.policy_counter) a.policy_counter[0] += 1;
}

struct CloseArgs {
    int E, D, R, K;
    i64 row, capacity;
    double discount;
    const u8 *done;
    const i64 *count_in;
    i64 *count_out;
};

// Lane e closes when its step was done (and it stored one: length > 0).  Sequence numbers: count_in + (lengths of the closing lanes before e) + j for the j-th
// item, j = 0 the LAST step -- the Worker's reversed walk.  Of the S items the lock-step adds only the last `capacity` are written: what a sequential ring would
// still hold, and no two workgroups write one slot.  Every closing workgroup recomputes prefix and total from the lanes' lengths, which this launch only reads;
// the count goes from one word to the other, so no workgroup reads what another advances.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_vppo_lanes_close(CloseArgs a, Ring r, Items it) {
    __shared__ i64 red[2][kThreads];
    __shared__ float rw[kMaxRing], tot[kMaxRing];
    const int t = threadIdx.x, e = blockIdx.x;
    const bool closing = a.done[e] && r.len[e] > 0;
    if (!closing && e != 0) return;  // (lane 0's workgroup always runs: it carries the count over)
    i64 before = 0, all = 0;
    for (int k = t; k < a.E; k += kThreads)
        if (a.done[k] && r.len[k] > 0) {
            all += r.len[k];
            if (k < e) before += r.len[k];
        }
    red[0][t] = before, red[1][t] = all;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) red[0][t] += red[0][t + w], red[1][t] += red[1][t + w];
        __syncthreads();
    }
    const i64 count = a.count_in[0];
    const i64 S = red[1][0];
    if (e == 0 && t == 0) a.count_out[0] = count + S;
    if (!closing) return;
    const int n = r.len[e];
    const i64 base = count + red[0][0];
    const i64 keep_from = count + S - a.capacity;  // the first sequence number that survives the lock-step
    for (int j = t; j < n; j += kThreads) rw[j] = r.reward[(i64)((a.row - j + a.R) % a.R) * a.E + e];
    __syncthreads();
    if (t == 0) {
        double total = 0.0;  // total = reward + discount * total, the Worker's order, one chain; rounded to float32 once, at the store
        for (int j = 0; j < n; j++) {
            total = (double)rw[j] + a.discount * total;
            tot[j] = (float)total;
        }
    }
    __syncthreads();
    for (int j = t; j < n; j += kThreads) {
        if (base + j < keep_from) continue;
        const i64 slot = (base + j) % a.capacity;
        const i64 k = (i64)((a.row - j + a.R) % a.R) * a.E + e;
        for (int q = 0; q < a.K; q++) it.action[slot * a.K + q] = r.action[k * a.K + q], it.logp[slot * a.K + q] = r.logp[k * a.K + q];
        it.reward[slot] = r.reward[k], it.nterm[slot] = r.nterm[k], it.total[slot] = tot[j];
    }
    const int DV = VEC ? a.D / 4 : a.D;
    for (i64 p = t; p < (i64)n * DV; p += kThreads) {
        const int j = (int)(p / DV), d = (int)(p % DV);
        if (base + j < keep_from) continue;
        const i64 slot = (base + j) % a.capacity;
        const i64 rj = (a.row - j + a.R) % a.R, rn = (rj + 1) % a.R;
        const i64 src = (rj * a.E + e) * DV + d, src2 = (rn * a.E + e) * DV + d, dst = slot * DV + d;
        if constexpr (VEC) {
            ((float4 *)it.s)[dst] = ((const float4 *)r.obs)[src];
            ((float4 *)it.s2)[dst] = ((const float4 *)r.obs)[src2];
        } else {
            it.s[dst] = r.obs[src];
            it.s2[dst] = r.obs[src2];
        }
    }
}

// Floyd's algorithm: B distinct values of [0, N), N = min(capacity, added).  Step i: j = N - B + i, t = min(j, floor(U_i (j + 1))), U_i the keyed uniform
// (seed, draw, i); take t, or j when t is already chosen.  One wave: the B steps are sequential, the membership test runs across the lanes.
__global__ void __launch_bounds__(64) k_vppo_lanes_pick(const i64 *count, i64 capacity, int B, u64 seed, u64 draw, i64 *slots, int32_t *error) {
    __shared__ i64 ch[kThreads];
    const int lane = threadIdx.x;
    const i64 added = count[0];
    const i64 N = added < capacity ? added : capacity;
    if (N < B) {
        if (lane == 0) error[0] = 2;
        for (int i = lane; i < B; i += 64) slots[i] = 0;
        return;
    }
    for (int i = 0; i < B; i++) {
        const i64 j = N - B + i;
        i64 tt = (i64)floor(srlx::u53(srlx::rng_u64(seed, draw, (u64)i)) * (double)(j + 1));
        tt = tt < j ? tt : j;
        int hit = 0;
        for (int k = lane; k < i; k += 64) hit |= ch[k] == tt;
        const i64 pick = __any(hit) ? j : tt;
        if (lane == 0) ch[i] = pick;  // (slot i: no step has read it yet)
        __syncthreads();
    }
    for (int i = lane; i < B; i += 64) slots[i] = ch[i];
}

struct GatherArgs {
    int D, K;
    const i64 *slots;
    float *s, *s2;
    int32_t *action;
    float *logp, *reward, *nterm, *total;
};

template <bool VEC>
__global__ void __launch_bounds__(64) k_vppo_lanes_gather(GatherArgs a, Items it) {
    const int b = blockIdx.x, t = threadIdx.x;
    const i64 slot = a.slots[b];
    const int DV = VEC ? a.D / 4 : a.D;
    for (int d = t; d < DV; d += 64) {
        if constexpr (VEC) {
            ((float4 *)a.s)[(i64)b * DV + d] = ((const float4 *)it.s)[slot * DV + d];
            ((float4 *)a.s2)[(i64)b * DV + d] = ((const float4 *)it.s2)[slot * DV + d];
        } else {
            a.s[(i64)b * DV + d] = it.s[slot * DV + d];
            a.s2[(i64)b * DV + d] = it.s2[slot * DV + d];
        }
    }
    if (t < a.K) a.action[(i64)b * a.K + t] = it.action[slot * a.K + t], a.logp[(i64)b * a.K + t] = it.logp[slot * a.K + t];
    if (t == 0) a.reward[b] = it.reward[slot], a.nterm[b] = it.nterm[slot], a.total[b] = it.total[slot];
}

// ---- Pendulum-v1 (envs/pendulum.py) for E lanes under the needs_reset protocol, float64 state (th, thdot) -------------------------------------------------------
// The step is envs/pendulum.py:step line for line: u = clip(torque, -2, 2); ang = ((th + pi) % (2 pi)) - pi with Python's sign-of-the-divisor remainder;
// reward = -(ang ang + 0.1 thdot thdot + 0.001 u u) from the state BEFORE the step; thdot = clip(thdot + (15 sin th + 3 u) 0.05, -8, 8); th += thdot 0.05.
// A lane whose needs_reset byte is set only receives its next episode's first observation: th = -pi + 2 pi U_0, thdot = -1 + 2 U_1 (random.uniform's a + (b - a) U)
// from uniforms keyed by (seed ^ kPendulumKey, lane << 32 | episode, k).
constexpr u64 kPendulumKey = 0x50454E44554C554Dull;  // "PENDULUM"
constexpr double kPi = 3.141592653589793;

__global__ void __launch_bounds__(256) k_pendulum_lanes(i64 E, double *__restrict__ state, int32_t *__restrict__ steps, int32_t *__restrict__ episodes,
                                                        const u8 *__restrict__ needs_reset, const float *__restrict__ torques, i64 max_steps, u64 seed,
                                                        float *__restrict__ obs, float *__restrict__ reward, u8 *__restrict__ terminated, u8 *__restrict__ done) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double th = state[2 * e], thdot = state[2 * e + 1];
    if (!torques || !needs_reset || needs_reset[e]) {  // (no torques or no bytes: every lane's next episode)
        const int ep = episodes[e];
        const u64 key = (u64)e * 0x100000000ull + (u64)(uint32_t)ep;
        th = -kPi + (2.0 * kPi) * srlx::u53(srlx::rng_u64(seed ^ kPendulumKey, key, 0));
        thdot = -1.0 + 2.0 * srlx::u53(srlx::rng_u64(seed ^ kPendulumKey, key, 1));
        episodes[e] = ep + 1;
        steps[e] = 0;
        if (reward) reward[e] = 0.f, terminated[e] = 0, done[e] = 0;
    } else {
        const double t = (double)torques[e];
        const double u = t < -2.0 ? -2.0 : (t > 2.0 ? 2.0 : t);
        double ang = fmod(th + kPi, 2.0 * kPi);
        if (ang < 0.0) ang += 2.0 * kPi;  // Python's %: the remainder takes the divisor's sign
        ang -= kPi;
        reward[e] = (float)-(ang * ang + 0.1 * thdot * thdot + 0.001 * u * u);
        const double nd = thdot + (15.0 * sin(th) + 3.0 * u) * 0.05;
        thdot = nd < -8.0 ? -8.0 : (nd > 8.0 ? 8.0 : nd);
        th = th + thdot * 0.05;
        const int st = steps[e] + 1;
        steps[e] = st;
        terminated[e] = 0;
        done[e] = st >= max_steps ? 1 : 0;
    }
    state[2 * e] = th, state[2 * e + 1] = thdot;
    obs[3 * e] = (float)cos(th), obs[3 * e + 1] = (float)sin(th), obs[3 * e + 2] = (float)thdot;
}

int check_shape(const char *who, i64 E, int D, i64 max_episode_steps, i64 capacity) {
    SRLX_REQUIRE(E >= 1 && E <= 4096, "%s: %lld lanes (1..4096)", who, (long long)E);
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(max_episode_steps >= 1 && max_episode_steps <= kMaxRing - 2, "%s: max_episode_steps %lld (1..%d)", who, (long long)max_episode_steps, kMaxRing - 2);
    SRLX_REQUIRE(capacity >= 1 && capacity <= (i64)1 << 24, "%s: capacity %lld (1..2^24)", who, (long long)capacity);
    return SRLX_OK;
}

// both kinds of handle: K = 1 words per action and `normal` false for the categorical store
int create(const char *who, srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int K, bool normal,
           int device) {
    SRLX_REQUIRE(out, "%s: NULL handle pointer", who);
    *out = nullptr;
    SRLX_TRY(check_shape(who, n_lanes, obs_dim, max_episode_steps, capacity));
    SRLX_REQUIRE(discount >= 0.0 && discount <= 1.0, "%s: discount %g (0..1)", who, discount);
    SRLX_REQUIRE(K >= 1 && K <= 8, "%s: %d action elements (1..8)", who, K);
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "%s: device %d unavailable", who, device);
    srlx_vppo_lanes *h = new srlx_vppo_lanes();
    h->E = (int)n_lanes, h->D = obs_dim, h->R = (int)max_episode_steps + 2, h->device = device, h->capacity = capacity, h->discount = discount;
    h->K = K, h->normal = normal;
    const size_t E = (size_t)h->E, D = (size_t)h->D, RE = (size_t)h->R * E, C = (size_t)capacity, W = (size_t)K;
    hipError_t e = hipMalloc((void **)&h->r.obs, sizeof(float) * RE * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.action, sizeof(int32_t) * RE * W);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.logp, sizeof(float) * RE * W);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.reward, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.nterm, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.done, RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.len, sizeof(int32_t) * E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.needs_reset, E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.s, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.s2, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.action, sizeof(int32_t) * C * W);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.logp, sizeof(float) * C * W);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.reward, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.nterm, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.total, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->count, sizeof(i64) * 2);
    if (e == hipSuccess) e = hipMalloc((void **)&h->error, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->r.obs, 0, sizeof(float) * RE * D);
    if (e == hipSuccess) e = hipMemset(h->r.action, 0, sizeof(int32_t) * RE * W);
    if (e == hipSuccess) e = hipMemset(h->r.logp, 0, sizeof(float) * RE * W);
    if (e == hipSuccess) e = hipMemset(h->r.reward, 0, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.nterm, 0, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.done, 0, RE);
    if (e == hipSuccess) e = hipMemset(h->r.len, 0, sizeof(int32_t) * E);
    if (e == hipSuccess) e = hipMemset(h->r.needs_reset, 0, E);
    if (e == hipSuccess) e = hipMemset(h->it.s, 0, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMemset(h->it.s2, 0, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMemset(h->it.action, 0, sizeof(int32_t) * C * W);
    if (e == hipSuccess) e = hipMemset(h->it.logp, 0, sizeof(float) * C * W);
    if (e == hipSuccess) e = hipMemset(h->it.reward, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->it.nterm, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->it.total, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->count, 0, sizeof(i64) * 2);
    if (e == hipSuccess) e = hipMemset(h->error, 0, sizeof(int32_t));
    if (e != hipSuccess) {
        srlx_vppo_lanes_destroy(h);
        srlx::set_error("%s: device set-up failed: %s", who, hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    *out = h;
    return SRLX_OK;
}

// one lock-step of either kind: `actions` as words [E][K], `logp` [E][K]
int push(srlx_vppo_lanes *h, const int32_t *d_actions, const float *d_logp, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done,
         const float *d_next_obs, int64_t *d_policy_counter, void *stream) {
    srlx::DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const i64 row = h->lock_steps % h->R, next_row = (h->lock_steps + 1) % h->R;
    const int par = (int)(h->lock_steps & 1);
    StoreArgs sa{h->E, h->D, h->R, h->K, row, next_row, d_actions, d_logp, d_rewards, d_terminated, d_done, d_next_obs, (i64 *)d_policy_counter, h->error};
    const i64 ED = (i64)h->E * h->D;
    hipLaunchKernelGGL(k_vppo_lanes_store, dim3((unsigned)((ED + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sa, h->r);
    CloseArgs ca{h->E, h->D, h->R, h->K, row, h->capacity, h->discount, d_done, h->count + par, h->count + (par ^ 1)};
    if (h->D % 4 == 0)
        hipLaunchKernelGGL(k_vppo_lanes_close<true>, dim3((unsigned)h->E), dim3(kThreads), 0, st, ca, h->r, h->it);
    else
        hipLaunchKernelGGL(k_vppo_lanes_close<false>, dim3((unsigned)h->E), dim3(kThreads), 0, st, ca, h->r, h->it);
    SRLX_HIP(hipGetLastError());
    h->lock_steps++;
    return SRLX_OK;
}

// one draw of either kind: `d_actions` as words [B][K], `d_old_logpi` [B][K]
int sample(srlx_vppo_lanes *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, int32_t *d_actions, float *d_old_logpi, float *d_rewards,
           float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream) {
    srlx::DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = h->D % 4 == 0 && (((uintptr_t)d_states | (uintptr_t)d_next_states) & 15) == 0;
    hipLaunchKernelGGL(k_vppo_lanes_pick, dim3(1), dim3(64), 0, st, (const i64 *)(h->count + (h->lock_steps & 1)), h->capacity, (int)batch, (u64)seed, (u64)h->draws,
                       (i64 *)d_slots, h->error);
    GatherArgs ga{h->D, h->K, (const i64 *)d_slots, d_states, d_next_states, d_actions, d_old_logpi, d_rewards, d_not_terminated, d_total_rewards};
    if (vec)
        hipLaunchKernelGGL(k_vppo_lanes_gather<true>, dim3((unsigned)batch), dim3(64), 0, st, ga, h->it);
    else
        hipLaunchKernelGGL(k_vppo_lanes_gather<false>, dim3((unsigned)batch), dim3(64), 0, st, ga, h->it);
    SRLX_HIP(hipGetLastError());
    h->draws++;
    return SRLX_OK;
}

}  // namespace

extern "C" {

int srlx_vppo_lanes_create(srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int device) {
    return create("vppo_lanes_create", out, n_lanes, obs_dim, max_episode_steps, capacity, discount, 1, false, device);
}

int srlx_vppo_lanes_create_normal(srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int action_dim,
                                  int device) {
    return create("vppo_lanes_create_normal", out, n_lanes, obs_dim, max_episode_steps, capacity, discount, action_dim, true, device);
}

int srlx_vppo_lanes_destroy(srlx_vppo_lanes_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (void *p : {(void *)h->r.obs, (void *)h->r.action, (void *)h->r.logp, (void *)h->r.reward, (void *)h->r.nterm, (void *)h->r.done, (void *)h->r.len,
                    (void *)h->r.needs_reset, (void *)h->it.s, (void *)h->it.s2, (void *)h->it.action, (void *)h->it.logp, (void *)h->it.reward, (void *)h->it.nterm,
                    (void *)h->it.total, (void *)h->count, (void *)h->error})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_vppo_lanes_reset(srlx_vppo_lanes_t *h, const float *d_first_obs, void *stream) {
    SRLX_REQUIRE(h && d_first_obs, "vppo_lanes_reset: NULL handle or observations");
    srlx::DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    SRLX_HIP(hipMemsetAsync(h->r.len, 0, sizeof(int32_t) * h->E, st));
    SRLX_HIP(hipMemsetAsync(h->r.needs_reset, 0, (size_t)h->E, st));
    SRLX_HIP(hipMemsetAsync(h->count, 0, sizeof(i64) * 2, st));
    SRLX_HIP(hipMemsetAsync(h->error, 0, sizeof(int32_t), st));
    SRLX_HIP(hipMemcpyAsync(h->r.obs, d_first_obs, sizeof(float) * (size_t)h->E * h->D, hipMemcpyDeviceToDevice, st));
    h->lock_steps = 0, h->draws = 0;
    return SRLX_OK;
}

int srlx_vppo_lanes_push(srlx_vppo_lanes_t *h, const int32_t *d_actions, const float *d_logp, const float *d_rewards, const uint8_t *d_terminated, const uint8_t *d_done,
                         const float *d_next_obs, int64_t *d_policy_counter, void *stream) {
    SRLX_REQUIRE(h, "vppo_lanes_push: NULL handle");
    SRLX_REQUIRE(!h->normal, "vppo_lanes_push: a Normal store takes float32 actions [E][K] (srlx_vppo_lanes_push_normal)");
    SRLX_REQUIRE(d_actions && d_logp && d_rewards && d_terminated && d_done && d_next_obs, "vppo_lanes_push: NULL argument");
    return push(h, d_actions, d_logp, d_rewards, d_terminated, d_done, d_next_obs, d_policy_counter, stream);
}

int srlx_vppo_lanes_push_normal(srlx_vppo_lanes_t *h, const float *d_actions, const float *d_logp, const float *d_rewards, const uint8_t *d_terminated,
                                const uint8_t *d_done, const float *d_next_obs, int64_t *d_policy_counter, void *stream) {
    SRLX_REQUIRE(h, "vppo_lanes_push_normal: NULL handle");
    SRLX_REQUIRE(h->normal, "vppo_lanes_push_normal: a categorical store takes int32 actions [E] (srlx_vppo_lanes_push)");
    SRLX_REQUIRE(d_actions && d_logp && d_rewards && d_terminated && d_done && d_next_obs, "vppo_lanes_push_normal: NULL argument");
    return push(h, (const int32_t *)d_actions, d_logp, d_rewards, d_terminated, d_done, d_next_obs, d_policy_counter, stream);
}

int srlx_vppo_lanes_sample(srlx_vppo_lanes_t *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, int32_t *d_actions, float *d_old_logpi,
                           float *d_rewards, float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream) {
    SRLX_REQUIRE(h, "vppo_lanes_sample: NULL handle");
    SRLX_REQUIRE(batch >= 1 && batch <= kThreads && batch <= h->capacity, "vppo_lanes_sample: batch %lld (1..%d, at most the capacity %lld)", (long long)batch, kThreads,
                 (long long)h->capacity);
    SRLX_REQUIRE(!h->normal, "vppo_lanes_sample: a Normal store gives float32 actions [B][K] (srlx_vppo_lanes_sample_normal)");
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_old_logpi && d_rewards && d_not_terminated && d_total_rewards && d_slots, "vppo_lanes_sample: NULL argument");
    return sample(h, batch, seed, d_states, d_next_states, d_actions, d_old_logpi, d_rewards, d_not_terminated, d_total_rewards, d_slots, stream);
}

int srlx_vppo_lanes_sample_normal(srlx_vppo_lanes_t *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, float *d_actions, float *d_old_logpi,
                                  float *d_rewards, float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream) {
    SRLX_REQUIRE(h, "vppo_lanes_sample_normal: NULL handle");
    SRLX_REQUIRE(batch >= 1 && batch <= kThreads && batch <= h->capacity, "vppo_lanes_sample_normal: batch %lld (1..%d, at most the capacity %lld)", (long long)batch,
                 kThreads, (long long)h->capacity);
    SRLX_REQUIRE(h->normal, "vppo_lanes_sample_normal: a categorical store gives int32 actions [B] (srlx_vppo_lanes_sample)");
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_old_logpi && d_rewards && d_not_terminated && d_total_rewards && d_slots,
                 "vppo_lanes_sample_normal: NULL argument");
    return sample(h, batch, seed, d_states, d_next_states, (int32_t *)d_actions, d_old_logpi, d_rewards, d_not_terminated, d_total_rewards, d_slots, stream);
}

int srlx_pendulum_lane_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const uint8_t *d_needs_reset, const float *d_torques,
                            int64_t max_steps, uint64_t seed, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_done, void *stream) {
    SRLX_REQUIRE(n_envs > 0 && n_envs <= 65536 && d_state && d_steps && d_episodes && d_obs && max_steps > 0, "pendulum_lane_step: bad argument");
    SRLX_REQUIRE(!d_torques || !d_needs_reset || (d_reward && d_terminated && d_done), "pendulum_lane_step: a step needs the scalar outputs");
    SRLX_REQUIRE(!d_reward == !d_terminated && !d_reward == !d_done, "pendulum_lane_step: the scalar outputs come together");
    hipLaunchKernelGGL(k_pendulum_lanes, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n_envs, d_state, d_steps, d_episodes, d_needs_reset,
                       d_torques, (i64)max_steps, (u64)seed, d_obs, d_reward, d_terminated, d_done);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_vppo_lanes_count(srlx_vppo_lanes_t *h, int64_t *added, int32_t *error, void *stream) {
    SRLX_REQUIRE(h && added && error, "vppo_lanes_count: NULL argument");
    srlx::DeviceGuard g(h->device);
    SRLX_HIP(hipStreamSynchronize((hipStream_t)stream));
    SRLX_HIP(hipMemcpy(added, h->count + (h->lock_steps & 1), sizeof(i64), hipMemcpyDeviceToHost));
    SRLX_HIP(hipMemcpy(error, h->error, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SRLX_OK;
}

int srlx_vppo_lanes_views(srlx_vppo_lanes_t *h, void **views, int64_t *current_row) {
    SRLX_REQUIRE(h && views && current_row, "vppo_lanes_views: NULL argument");
    void *v[kViews] = {h->r.obs, h->r.action, h->r.logp, h->r.reward, h->r.nterm, h->r.done, h->r.len, h->r.needs_reset, h->it.s, h->it.s2, h->it.action, h->it.logp,
                       h->it.reward, h->it.nterm, h->it.total, h->count};
    for (int i = 0; i < kViews; i++) views[i] = v[i];
    *current_row = h->lock_steps % h->R;
    return SRLX_OK;
}

int srlx_vppo_lanes_read(srlx_vppo_lanes_t *h, int view, int64_t bytes, void *host_dst, void *stream) {
    SRLX_REQUIRE(h && host_dst, "vppo_lanes_read: NULL argument");
    SRLX_REQUIRE(view >= 0 && view < kViews, "vppo_lanes_read: view %d (0..%d)", view, kViews - 1);
    const size_t E = (size_t)h->E, D = (size_t)h->D, RE = (size_t)h->R * E, C = (size_t)h->capacity, W = (size_t)h->K;
    const size_t size[kViews] = {4 * RE * D, 4 * RE * W, 4 * RE * W, 4 * RE, 4 * RE, RE, 4 * E, E, 4 * C * D, 4 * C * D, 4 * C * W, 4 * C * W, 4 * C, 4 * C, 4 * C, 16};
    SRLX_REQUIRE(bytes >= 0 && (size_t)bytes == size[view], "vppo_lanes_read: view %d holds %lld bytes, not %lld", view, (long long)size[view], (long long)bytes);
    void *views[kViews];
    int64_t row;
    SRLX_TRY(srlx_vppo_lanes_views(h, views, &row));
    srlx::DeviceGuard g(h->device);
    SRLX_HIP(hipStreamSynchronize((hipStream_t)stream));
    SRLX_HIP(hipMemcpy(host_dst, views[view], (size_t)bytes, hipMemcpyDeviceToHost));
    return SRLX_OK;
}

}  // extern "C"
