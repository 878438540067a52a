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
// A push is TWO launches: the close reads every lane's length and done flag to place its items (an exclusive prefix in lane order), and only a launch boundary
// orders those reads behind all lanes' stores.  No atomics: equal inputs give equal bits.
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
    int32_t *action;
    float *logp, *reward, *nterm;
    u8 *done;  // [R][E]
    int32_t *len;
    u8 *needs_reset;  // [E]
};

struct Items {
    float *s, *s2;  // [capacity][D]
    int32_t *action;
    float *logp, *reward, *nterm, *total;  // [capacity]
};

}  // namespace

struct srlx_vppo_lanes {
    int E, D, R, device;
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
    int E, D, R;
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
            r.action[k] = a.actions[i];
            r.logp[k] = fmaxf(a.logp[i], srlxp::kLogFloor);  // the Worker floors in on_step, not in policy()
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
    int E, D, R;
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
        it.action[slot] = r.action[k], it.logp[slot] = r.logp[k], it.reward[slot] = r.reward[k], it.nterm[slot] = r.nterm[k], it.total[slot] = tot[j];
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
    int D;
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
    if (t == 0) a.action[b] = it.action[slot], a.logp[b] = it.logp[slot], a.reward[b] = it.reward[slot], a.nterm[b] = it.nterm[slot], a.total[b] = it.total[slot];
}

int check_shape(const char *who, i64 E, int D, i64 max_episode_steps, i64 capacity) {
    SRLX_REQUIRE(E >= 1 && E <= 4096, "%s: %lld lanes (1..4096)", who, (long long)E);
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(max_episode_steps >= 1 && max_episode_steps <= kMaxRing - 2, "%s: max_episode_steps %lld (1..%d)", who, (long long)max_episode_steps, kMaxRing - 2);
    SRLX_REQUIRE(capacity >= 1 && capacity <= (i64)1 << 24, "%s: capacity %lld (1..2^24)", who, (long long)capacity);
    return SRLX_OK;
}

}  // namespace

extern "C" {

int srlx_vppo_lanes_create(srlx_vppo_lanes_t **out, int64_t n_lanes, int obs_dim, int64_t max_episode_steps, int64_t capacity, double discount, int device) {
    SRLX_REQUIRE(out, "vppo_lanes_create: NULL handle pointer");
    *out = nullptr;
    SRLX_TRY(check_shape("vppo_lanes_create", n_lanes, obs_dim, max_episode_steps, capacity));
    SRLX_REQUIRE(discount >= 0.0 && discount <= 1.0, "vppo_lanes_create: discount %g (0..1)", discount);
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "vppo_lanes_create: device %d unavailable", device);
    srlx_vppo_lanes *h = new srlx_vppo_lanes();
    h->E = (int)n_lanes, h->D = obs_dim, h->R = (int)max_episode_steps + 2, h->device = device, h->capacity = capacity, h->discount = discount;
    const size_t E = (size_t)h->E, D = (size_t)h->D, RE = (size_t)h->R * E, C = (size_t)capacity;
    hipError_t e = hipMalloc((void **)&h->r.obs, sizeof(float) * RE * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.action, sizeof(int32_t) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.logp, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.reward, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.nterm, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.done, RE);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.len, sizeof(int32_t) * E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->r.needs_reset, E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.s, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.s2, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.action, sizeof(int32_t) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.logp, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.reward, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.nterm, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->it.total, sizeof(float) * C);
    if (e == hipSuccess) e = hipMalloc((void **)&h->count, sizeof(i64) * 2);
    if (e == hipSuccess) e = hipMalloc((void **)&h->error, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->r.obs, 0, sizeof(float) * RE * D);
    if (e == hipSuccess) e = hipMemset(h->r.action, 0, sizeof(int32_t) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.logp, 0, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.reward, 0, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.nterm, 0, sizeof(float) * RE);
    if (e == hipSuccess) e = hipMemset(h->r.done, 0, RE);
    if (e == hipSuccess) e = hipMemset(h->r.len, 0, sizeof(int32_t) * E);
    if (e == hipSuccess) e = hipMemset(h->r.needs_reset, 0, E);
    if (e == hipSuccess) e = hipMemset(h->it.s, 0, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMemset(h->it.s2, 0, sizeof(float) * C * D);
    if (e == hipSuccess) e = hipMemset(h->it.action, 0, sizeof(int32_t) * C);
    if (e == hipSuccess) e = hipMemset(h->it.logp, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->it.reward, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->it.nterm, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->it.total, 0, sizeof(float) * C);
    if (e == hipSuccess) e = hipMemset(h->count, 0, sizeof(i64) * 2);
    if (e == hipSuccess) e = hipMemset(h->error, 0, sizeof(int32_t));
    if (e != hipSuccess) {
        srlx_vppo_lanes_destroy(h);
        srlx::set_error("vppo_lanes_create: device set-up failed: %s", hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    *out = h;
    return SRLX_OK;
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
    SRLX_REQUIRE(d_actions && d_logp && d_rewards && d_terminated && d_done && d_next_obs, "vppo_lanes_push: NULL argument");
    srlx::DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const i64 row = h->lock_steps % h->R, next_row = (h->lock_steps + 1) % h->R;
    const int par = (int)(h->lock_steps & 1);
    StoreArgs sa{h->E, h->D, h->R, row, next_row, d_actions, d_logp, d_rewards, d_terminated, d_done, d_next_obs, (i64 *)d_policy_counter, h->error};
    const i64 ED = (i64)h->E * h->D;
    hipLaunchKernelGGL(k_vppo_lanes_store, dim3((unsigned)((ED + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sa, h->r);
    CloseArgs ca{h->E, h->D, h->R, row, h->capacity, h->discount, d_done, h->count + par, h->count + (par ^ 1)};
    if (h->D % 4 == 0)
        hipLaunchKernelGGL(k_vppo_lanes_close<true>, dim3((unsigned)h->E), dim3(kThreads), 0, st, ca, h->r, h->it);
    else
        hipLaunchKernelGGL(k_vppo_lanes_close<false>, dim3((unsigned)h->E), dim3(kThreads), 0, st, ca, h->r, h->it);
    SRLX_HIP(hipGetLastError());
    h->lock_steps++;
    return SRLX_OK;
}

int srlx_vppo_lanes_sample(srlx_vppo_lanes_t *h, int64_t batch, uint64_t seed, float *d_states, float *d_next_states, int32_t *d_actions, float *d_old_logpi,
                           float *d_rewards, float *d_not_terminated, float *d_total_rewards, int64_t *d_slots, void *stream) {
    SRLX_REQUIRE(h, "vppo_lanes_sample: NULL handle");
    SRLX_REQUIRE(batch >= 1 && batch <= kThreads && batch <= h->capacity, "vppo_lanes_sample: batch %lld (1..%d, at most the capacity %lld)", (long long)batch, kThreads,
                 (long long)h->capacity);
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_old_logpi && d_rewards && d_not_terminated && d_total_rewards && d_slots, "vppo_lanes_sample: NULL argument");
    srlx::DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = h->D % 4 == 0 && (((uintptr_t)d_states | (uintptr_t)d_next_states) & 15) == 0;
    hipLaunchKernelGGL(k_vppo_lanes_pick, dim3(1), dim3(64), 0, st, (const i64 *)(h->count + (h->lock_steps & 1)), h->capacity, (int)batch, (u64)seed, (u64)h->draws,
                       (i64 *)d_slots, h->error);
    GatherArgs ga{h->D, (const i64 *)d_slots, d_states, d_next_states, d_actions, d_old_logpi, d_rewards, d_not_terminated, d_total_rewards};
    if (vec)
        hipLaunchKernelGGL(k_vppo_lanes_gather<true>, dim3((unsigned)batch), dim3(64), 0, st, ga, h->it);
    else
        hipLaunchKernelGGL(k_vppo_lanes_gather<false>, dim3((unsigned)batch), dim3(64), 0, st, ga, h->it);
    SRLX_HIP(hipGetLastError());
    h->draws++;
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
    const size_t E = (size_t)h->E, D = (size_t)h->D, RE = (size_t)h->R * E, C = (size_t)h->capacity;
    const size_t size[kViews] = {4 * RE * D, 4 * RE, 4 * RE, 4 * RE, 4 * RE, RE, 4 * E, E, 4 * C * D, 4 * C * D, 4 * C, 4 * C, 4 * C, 4 * C, 4 * C, 16};
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
