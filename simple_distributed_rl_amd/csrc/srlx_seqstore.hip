// srlx_seqstore.hip -- Agent57's sequence replay in HBM (include/srlx.h, "Agent57 sequence store"): one launch assembles a sampled batch of sequences from the
// frame ring and the per-sequence records into the tensors the trainer feeds its networks.  The kernel moves data and computes nothing: no atomics, no LDS, no
// scratch.  Rows are copied with 16-byte accesses when the frame length allows it and with dword accesses otherwise; the path is a property of the launch.
//
// The lane ring of the E-lane engine (srlx.h, "Agent57 lane sequence ring") lives here too: srlx_seq_lane_push writes one lock-step of all lanes into time-major
// rings, srlx_seq_lane_gather builds the same eleven tensors from (lane, position, flush offset) descriptors.  A window there is a view of the rings, and its
// padding (before the episode's start, after its end) is decided per entry from the position's age; pad actions come from the keyed generator.
//
// R2D2's lane ring (srlx.h, "R2D2 lane sequence ring") follows it: srlx_r2d2_policy (the roulette draw over the epsilon-greedy probabilities, with the drawn
// probability), srlx_r2d2_lane_push and srlx_r2d2_lane_gather (the tensors of r2d2.SequenceBatch).
#include "srlx_common.h"

namespace {

using i64 = long long;
using u8 = unsigned char;

constexpr int kThreads = 256;
constexpr int kInFlight = 4;                      // loads a lane issues before its first store
constexpr int kChunk = kThreads * kInFlight;      // copy units (float4 or float) one workgroup moves

struct SeqGatherArgs {
    i64 B;
    int L, S, A, H;
    i64 frame_elems, frame_stride, frame_capacity, seq_capacity, record_stride;
    const int64_t *slots;
    const float *ring;
    const int32_t *records;
    float *states;
    int64_t *actions;
    float *r_ext, *r_int, *dones;
    u8 *invalid;
    int64_t *actor;
    float *h_ext, *c_ext, *h_int, *c_int;
};

template <typename V>
__device__ __forceinline__ V zero_of();
template <>
__device__ __forceinline__ float zero_of<float>() {
    return 0.f;
}
template <>
__device__ __forceinline__ float4 zero_of<float4>() {
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// workgroups [0, B L) x chunks: frame l of batch row b; workgroups [B L, B L + B) (chunk 0 only): the small fields of batch row b
template <typename V>
__global__ __launch_bounds__(kThreads) void k_seq_gather(SeqGatherArgs a) {
    const i64 row = blockIdx.x;
    const i64 n_frames = a.B * a.L;
    const int tid = threadIdx.x;
    if (row < n_frames) {
        const i64 b = row / a.L;
        const int l = (int)(row - b * a.L);
        const i64 s = a.slots[b];
        i64 f = -1;
        if (s >= 0 && s < a.seq_capacity) f = a.records[s * a.record_stride + l];
        const bool zero = f < 0 || f >= a.frame_capacity;  // -1: an all-zero frame; anything else outside the ring is never dereferenced
        constexpr int kPer = (int)(sizeof(V) / sizeof(float));
        const i64 units = a.frame_elems / kPer;  // (the vector path runs only when frame_elems is a multiple of 4)
        const V *src = (const V *)(a.ring + (zero ? 0 : f) * a.frame_stride);
        V *dst = (V *)(a.states + row * a.frame_elems);
        const i64 base = (i64)blockIdx.y * kChunk + tid;
        V v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            v[k] = zero_of<V>();
            if (!zero && i < units) v[k] = src[i];
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            if (i < units) dst[i] = v[k];
        }
        return;
    }
    if (blockIdx.y != 0) return;
    const i64 b = row - n_frames;
    const i64 s = a.slots[b];
    const bool live = s >= 0 && s < a.seq_capacity;
    const int32_t *rec = a.records + (live ? s : 0) * a.record_stride;
    const int L = a.L, S = a.S, A = a.A, H = a.H;
    const int32_t *rec_act = rec + L;
    const float *rec_rext = (const float *)(rec + 2 * L), *rec_rint = (const float *)(rec + 3 * L), *rec_undone = (const float *)(rec + 4 * L);
    const float *rec_hid = (const float *)(rec + 4 * L + S + 1);
    const u8 *rec_inv = (const u8 *)(rec + 4 * L + S + 1 + 4 * H);
    for (int i = tid; i < L; i += kThreads) {
        a.actions[b * L + i] = live ? (int64_t)rec_act[i] : 0;
        a.r_ext[b * L + i] = live ? rec_rext[i] : 0.f;
        a.r_int[b * L + i] = live ? rec_rint[i] : 0.f;
    }
    for (int i = tid; i < S; i += kThreads) a.dones[b * S + i] = live ? rec_undone[i] : 0.f;
    for (int i = tid; i < S * A; i += kThreads) a.invalid[b * (i64)S * A + i] = live ? rec_inv[i] : (u8)0;
    if (tid == 0) a.actor[b] = live ? (int64_t)rec[4 * L + S] : 0;
    for (int i = tid; i < H; i += kThreads) {
        a.h_ext[b * H + i] = live ? rec_hid[i] : 0.f;
        a.c_ext[b * H + i] = live ? rec_hid[H + i] : 0.f;
        a.h_int[b * H + i] = live ? rec_hid[2 * H + i] : 0.f;
        a.c_int[b * H + i] = live ? rec_hid[3 * H + i] : 0.f;
    }
}

// ---- the lane ring ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kScal = 8;  // dwords per (position, lane) of the scalar ring: action, r_ext, r_int, undone, actor, age, 0, 0
enum { kAction = 0, kRExt = 1, kRInt = 2, kUndone = 3, kActor = 4, kAge = 5 };

__device__ __forceinline__ int pad_action(srlx::u64 seed, int e, i64 p, int A) { return (int)(srlx::rng_u64(seed, (srlx::u64)e, (srlx::u64)p) % (srlx::u64)A); }

struct LanePushArgs {
    int E, A, H;
    i64 frame_elems, frame_stride, T, t;
    srlx::u64 seed;
    const float *frames;
    const int32_t *action;
    const float *r_ext, *r_int, *undone;
    const int32_t *actor;
    const u8 *invalid;  // may be NULL: no invalid action
    const float *h_ext, *c_ext, *h_int, *c_int;
    const u8 *first;
    float *ring_frames;
    int32_t *ring_scal;
    u8 *ring_invalid;
    float *ring_hidden;
};

// workgroup (e, chunk): the chunk of lane e's frame row; chunk 0 also writes the lane's small fields
template <typename V>
__global__ __launch_bounds__(kThreads) void k_seq_lane_push(LanePushArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const i64 row = (a.t % a.T) * a.E + e;
    constexpr int kPer = (int)(sizeof(V) / sizeof(float));
    const i64 units = a.frame_elems / kPer;
    const V *src = (const V *)(a.frames + (i64)e * a.frame_elems);
    V *dst = (V *)(a.ring_frames + row * a.frame_stride);
    const i64 base = (i64)blockIdx.y * kChunk + tid;
    V v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        const i64 i = base + (i64)k * kThreads;
        v[k] = zero_of<V>();
        if (i < units) v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        const i64 i = base + (i64)k * kThreads;
        if (i < units) dst[i] = v[k];
    }
    if (blockIdx.y != 0) return;
    const bool first = a.t == 0 || a.first[e] != 0;  // an episode's first observation: it reads like the padding before it, but for its frame
    const int A = a.A, H = a.H;
    if (tid == 0) {
        int32_t *sc = a.ring_scal + row * kScal;
        float *scf = (float *)sc;
        int age = 0;
        if (!first) age = a.ring_scal[(((a.t - 1) % a.T) * a.E + e) * kScal + kAge] + 1;
        sc[kAction] = first ? pad_action(a.seed, e, a.t, A) : a.action[e];
        scf[kRExt] = first ? 0.f : a.r_ext[e];
        scf[kRInt] = first ? 0.f : a.r_int[e];
        scf[kUndone] = first ? 1.f : a.undone[e];
        sc[kActor] = a.actor[e];
        sc[kAge] = age;
        sc[6] = 0;
        sc[7] = 0;
    }
    for (int i = tid; i < A; i += kThreads) a.ring_invalid[row * A + i] = (first || !a.invalid) ? (u8)0 : a.invalid[(i64)e * A + i];
    float *hid = a.ring_hidden + row * 4 * H;
    for (int i = tid; i < H; i += kThreads) {
        hid[i] = first ? 0.f : a.h_ext[(i64)e * H + i];
        hid[H + i] = first ? 0.f : a.c_ext[(i64)e * H + i];
        hid[2 * H + i] = first ? 0.f : a.h_int[(i64)e * H + i];
        hid[3 * H + i] = first ? 0.f : a.c_int[(i64)e * H + i];
    }
}

struct LaneGatherArgs {
    i64 B;
    int L, S, A, H, E;
    i64 T, frame_elems, frame_stride;
    srlx::u64 seed;
    const int64_t *desc;
    const float *ring_frames;
    const int32_t *ring_scal;
    const u8 *ring_invalid;
    const float *ring_hidden;
    float *states;
    int64_t *actions;
    float *r_ext, *r_int, *dones;
    u8 *invalid;
    int64_t *actor;
    float *h_ext, *c_ext, *h_int, *c_int;
};

struct LaneWindow {
    bool live;  // the descriptor names a lane, a position and a flush offset the rings have room for
    int e, age;
    i64 t, k;
};

__device__ __forceinline__ LaneWindow lane_window(const LaneGatherArgs &a, i64 b) {
    LaneWindow w;
    const i64 e = a.desc[3 * b], t = a.desc[3 * b + 1], k = a.desc[3 * b + 2];
    w.live = e >= 0 && e < a.E && t >= 0 && k >= 0 && k < a.L;
    w.e = w.live ? (int)e : 0;
    w.t = w.live ? t : 0;
    w.k = w.live ? k : 0;
    w.age = w.live ? a.ring_scal[((w.t % a.T) * a.E + w.e) * kScal + kAge] : 0;
    return w;
}

enum { kRing = 0, kBefore = 1, kAfter = 2 };
// entry l of the window is lane position p = t - (L - 1) + l + k: after the end (p > t), before the episode's start (t - p > age), or the ring's entry
__device__ __forceinline__ int lane_entry(const LaneGatherArgs &a, const LaneWindow &w, int l, i64 *p) {
    *p = w.t - (a.L - 1) + l + w.k;
    if (*p > w.t) return kAfter;
    if (w.t - *p > (i64)w.age || *p < 0) return kBefore;  // (p < 0 cannot be inside an episode: never dereferenced)
    return kRing;
}

// workgroups [0, B L) x chunks: frame l of batch row b; workgroups [B L, B L + B) (chunk 0 only): the small fields of batch row b
template <typename V>
__global__ __launch_bounds__(kThreads) void k_seq_lane_gather(LaneGatherArgs a) {
    const i64 row = blockIdx.x;
    const i64 n_frames = a.B * a.L;
    const int tid = threadIdx.x;
    if (row < n_frames) {
        const i64 b = row / a.L;
        const int l = (int)(row - b * a.L);
        const LaneWindow w = lane_window(a, b);
        i64 p;
        const bool zero = !w.live || lane_entry(a, w, l, &p) != kRing;
        constexpr int kPer = (int)(sizeof(V) / sizeof(float));
        const i64 units = a.frame_elems / kPer;
        const V *src = (const V *)(a.ring_frames + (zero ? 0 : (p % a.T) * a.E + w.e) * a.frame_stride);
        V *dst = (V *)(a.states + row * a.frame_elems);
        const i64 base = (i64)blockIdx.y * kChunk + tid;
        V v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            v[k] = zero_of<V>();
            if (!zero && i < units) v[k] = src[i];
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            if (i < units) dst[i] = v[k];
        }
        return;
    }
    if (blockIdx.y != 0) return;
    const i64 b = row - n_frames;
    const LaneWindow w = lane_window(a, b);
    const int L = a.L, S = a.S, A = a.A, H = a.H;
    for (int i = tid; i < L; i += kThreads) {
        i64 p;
        const int kind = w.live ? lane_entry(a, w, i, &p) : kAfter;
        const int32_t *sc = a.ring_scal + (kind == kRing ? (p % a.T) * a.E + w.e : 0) * kScal;
        const float *scf = (const float *)sc;
        a.actions[b * L + i] = !w.live ? 0 : kind == kRing ? (int64_t)sc[kAction] : (int64_t)pad_action(a.seed, w.e, p, A);
        a.r_ext[b * L + i] = kind == kRing ? scf[kRExt] : 0.f;
        a.r_int[b * L + i] = kind == kRing ? scf[kRInt] : 0.f;
        if (i >= L - S) a.dones[b * S + (i - (L - S))] = kind == kRing ? scf[kUndone] : (w.live && kind == kBefore) ? 1.f : 0.f;
    }
    for (int i = tid; i < S * A; i += kThreads) {
        i64 p;
        const int kind = w.live ? lane_entry(a, w, L - S + i / A, &p) : kAfter;
        a.invalid[b * (i64)S * A + i] = kind == kRing ? a.ring_invalid[((p % a.T) * a.E + w.e) * A + i % A] : (u8)0;
    }
    if (tid == 0) a.actor[b] = w.live ? (int64_t)a.ring_scal[((w.t % a.T) * a.E + w.e) * kScal + kActor] : 0;
    i64 p0;
    const bool head = w.live && lane_entry(a, w, 0, &p0) == kRing;  // (the window's head is never after the end: k <= L - 1)
    const float *hid = a.ring_hidden + (head ? (p0 % a.T) * a.E + w.e : 0) * 4 * H;
    for (int i = tid; i < H; i += kThreads) {
        a.h_ext[b * H + i] = head ? hid[i] : 0.f;
        a.c_ext[b * H + i] = head ? hid[H + i] : 0.f;
        a.h_int[b * H + i] = head ? hid[2 * H + i] : 0.f;
        a.c_int[b * H + i] = head ? hid[3 * H + i] : 0.f;
    }
}

// ---- R2D2's lane ring (srlx.h, "R2D2 lane sequence ring") ------------------------------------------------------------------------------------------------------
// The same time-major rings with R2D2's fields: the scalar row carries the acting probability, two recurrent vectors instead of four, the invalid mask belongs to
// the position's OWN observation (an episode's first entry keeps it), and a window has S transitions and S + 1 masks.  The row copy (kInFlight loads before the
// first store), zero_of and the keyed pad action are the Agent57 kernels' own; those kernels are not touched.
enum { kRAction = 0, kRMu = 1, kRReward = 2, kRDone = 3, kRAge = 4 };  // dwords 5..7 stay zero

// srlx_r2d2_policy: one work-item per row.  The roulette walk is a serial double sum in action order (its rounding is the contract), A <= 64 and E is a lane
// count, so a wave per row would leave 63 lanes waiting on lane 0's walk.
__global__ __launch_bounds__(kThreads) void k_r2d2_policy(i64 E, int A, const float *__restrict__ q, const float *__restrict__ eps, const double *__restrict__ u,
                                                          const u8 *__restrict__ invalid, int32_t *__restrict__ actions, float *__restrict__ mu) {
    const i64 e = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const float *qe = q + e * A;
    const u8 *inv = invalid ? invalid + e * A : nullptr;
    int n_valid = 0, n_max = 0;
    float q_max = 0.f;
    for (int a = 0; a < A; ++a) {
        if (inv && inv[a]) continue;
        const float v = qe[a];
        if (n_valid == 0 || v > q_max) {
            q_max = v;
            n_max = 1;
        } else if (v == q_max) {
            ++n_max;
        }
        ++n_valid;
    }
    if (n_valid == 0) {  // (the reference divides by zero here)
        actions[e] = 0;
        mu[e] = 1.f;
        return;
    }
    const double epsilon = (double)eps[e];
    const double p_any = epsilon / (double)n_valid, p_top = p_any + (1.0 - epsilon) / (double)n_max;
    double total = 0.0;
    for (int a = 0; a < A; ++a) {
        if (inv && inv[a]) continue;
        total += qe[a] == q_max ? p_top : p_any;
    }
    const double r = u[e] * total;
    double acc = 0.0, p_act = 0.0;
    int act = 0;
    for (int a = 0; a < A; ++a) {
        if (inv && inv[a]) continue;  // (a zero weight: the reference would return an invalid action 0 at u = 0)
        p_act = qe[a] == q_max ? p_top : p_any;
        act = a;
        acc += p_act;
        if (r <= acc) break;
    }
    actions[e] = act;  // (acc ends at `total`, summed in the same order, and r <= total: the walk always breaks; the last valid action otherwise)
    mu[e] = (float)p_act;
}

struct R2d2PushArgs {
    int E, A, H;
    i64 frame_elems, frame_stride, T, t;
    srlx::u64 seed;
    const float *frames;
    const int32_t *action;
    const float *mu, *reward;
    const u8 *done;
    const u8 *invalid;  // may be NULL: no invalid action
    const float *h, *c;
    const u8 *first;
    float *ring_frames;
    int32_t *ring_scal;
    u8 *ring_invalid;
    float *ring_hidden;
};

// workgroup (e, chunk): the chunk of lane e's frame row; chunk 0 also writes the lane's small fields
template <typename V>
__global__ __launch_bounds__(kThreads) void k_r2d2_lane_push(R2d2PushArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const i64 row = (a.t % a.T) * a.E + e;
    constexpr int kPer = (int)(sizeof(V) / sizeof(float));
    const i64 units = a.frame_elems / kPer;
    const V *src = (const V *)(a.frames + (i64)e * a.frame_elems);
    V *dst = (V *)(a.ring_frames + row * a.frame_stride);
    const i64 base = (i64)blockIdx.y * kChunk + tid;
    V v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        const i64 i = base + (i64)k * kThreads;
        v[k] = zero_of<V>();
        if (i < units) v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        const i64 i = base + (i64)k * kThreads;
        if (i < units) dst[i] = v[k];
    }
    if (blockIdx.y != 0) return;
    const bool first = a.t == 0 || a.first[e] != 0;  // an episode's first observation: a pad transition, but its own frame and its own mask
    const int A = a.A, H = a.H;
    if (tid == 0) {
        int32_t *sc = a.ring_scal + row * kScal;
        float *scf = (float *)sc;
        int age = 0;
        if (!first) age = a.ring_scal[(((a.t - 1) % a.T) * a.E + e) * kScal + kRAge] + 1;
        sc[kRAction] = first ? pad_action(a.seed, e, a.t, A) : a.action[e];
        scf[kRMu] = first ? (float)(1.0 / (double)A) : a.mu[e];
        scf[kRReward] = first ? 0.f : a.reward[e];
        sc[kRDone] = first ? 0 : (a.done[e] != 0 ? 1 : 0);
        sc[kRAge] = age;
        sc[5] = 0;
        sc[6] = 0;
        sc[7] = 0;
    }
    for (int i = tid; i < A; i += kThreads) a.ring_invalid[row * A + i] = a.invalid ? a.invalid[(i64)e * A + i] : (u8)0;
    float *hid = a.ring_hidden + row * 2 * H;
    for (int i = tid; i < H; i += kThreads) {
        hid[i] = first ? 0.f : a.h[(i64)e * H + i];
        hid[H + i] = first ? 0.f : a.c[(i64)e * H + i];
    }
}

struct R2d2GatherArgs {
    i64 B;
    int L, S, A, H, E;
    i64 T, frame_elems, frame_stride;
    srlx::u64 seed;
    const int64_t *desc;
    const float *ring_frames;
    const int32_t *ring_scal;
    const u8 *ring_invalid;
    const float *ring_hidden;
    float *states;
    int32_t *actions;
    float *probs, *rewards;
    u8 *dones, *invalid;
    float *h, *c;
};

__device__ __forceinline__ LaneWindow r2d2_window(const R2d2GatherArgs &a, i64 b) {
    LaneWindow w;
    const i64 e = a.desc[3 * b], t = a.desc[3 * b + 1], k = a.desc[3 * b + 2];
    w.live = e >= 0 && e < a.E && t >= 0 && k >= 0 && k < a.S;
    w.e = w.live ? (int)e : 0;
    w.t = w.live ? t : 0;
    w.k = w.live ? k : 0;
    w.age = w.live ? a.ring_scal[((w.t % a.T) * a.E + w.e) * kScal + kRAge] : 0;
    return w;
}

// entry l of the window is lane position p = t - (L - 1) + l + k; a position is reduced mod T only once it is known to be >= 0 (kRing)
__device__ __forceinline__ int r2d2_entry(const R2d2GatherArgs &a, const LaneWindow &w, int l, i64 *p) {
    *p = w.t - (a.L - 1) + l + w.k;
    if (*p > w.t) return kAfter;
    if (w.t - *p > (i64)w.age || *p < 0) return kBefore;
    return kRing;
}

// workgroups [0, B L) x chunks: frame l of batch row b; workgroups [B L, B L + B) (chunk 0 only): the small fields of batch row b
template <typename V>
__global__ __launch_bounds__(kThreads) void k_r2d2_lane_gather(R2d2GatherArgs a) {
    const i64 row = blockIdx.x;
    const i64 n_frames = a.B * a.L;
    const int tid = threadIdx.x;
    if (row < n_frames) {
        const i64 b = row / a.L;
        const int l = (int)(row - b * a.L);
        const LaneWindow w = r2d2_window(a, b);
        i64 p;
        const bool zero = !w.live || r2d2_entry(a, w, l, &p) != kRing;
        constexpr int kPer = (int)(sizeof(V) / sizeof(float));
        const i64 units = a.frame_elems / kPer;
        const V *src = (const V *)(a.ring_frames + (zero ? 0 : (p % a.T) * a.E + w.e) * a.frame_stride);
        V *dst = (V *)(a.states + row * a.frame_elems);
        const i64 base = (i64)blockIdx.y * kChunk + tid;
        V v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            v[k] = zero_of<V>();
            if (!zero && i < units) v[k] = src[i];
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            if (i < units) dst[i] = v[k];
        }
        return;
    }
    if (blockIdx.y != 0) return;
    const i64 b = row - n_frames;
    const LaneWindow w = r2d2_window(a, b);
    const int L = a.L, S = a.S, A = a.A, H = a.H;
    const float pad_mu = (float)(1.0 / (double)A);
    for (int i = tid; i < S; i += kThreads) {  // the S transitions: entries L - S .. L - 1
        i64 p;
        const int kind = w.live ? r2d2_entry(a, w, L - S + i, &p) : kAfter;
        const int32_t *sc = a.ring_scal + (kind == kRing ? (p % a.T) * a.E + w.e : 0) * kScal;
        const float *scf = (const float *)sc;
        a.actions[b * S + i] = !w.live ? 0 : kind == kRing ? sc[kRAction] : pad_action(a.seed, w.e, p, A);
        a.probs[b * S + i] = !w.live ? 0.f : kind == kRing ? scf[kRMu] : pad_mu;
        a.rewards[b * S + i] = kind == kRing ? scf[kRReward] : 0.f;
        a.dones[b * S + i] = !w.live ? (u8)0 : kind == kRing ? (u8)(sc[kRDone] != 0) : (u8)(kind == kAfter);
    }
    for (int i = tid; i < (S + 1) * A; i += kThreads) {  // the S + 1 masks: entries L - S - 1 .. L - 1
        i64 p;
        const int kind = w.live ? r2d2_entry(a, w, L - S - 1 + i / A, &p) : kAfter;
        a.invalid[b * (i64)(S + 1) * A + i] = kind == kRing ? a.ring_invalid[((p % a.T) * a.E + w.e) * A + i % A] : (u8)0;
    }
    i64 p0;
    const bool head = w.live && r2d2_entry(a, w, 0, &p0) == kRing;  // (the window's head is never after the end: k <= S - 1 < L - 1)
    const float *hid = a.ring_hidden + (head ? (p0 % a.T) * a.E + w.e : 0) * 2 * H;
    for (int i = tid; i < H; i += kThreads) {
        a.h[b * H + i] = head ? hid[i] : 0.f;
        a.c[b * H + i] = head ? hid[H + i] : 0.f;
    }
}

bool in_envelope(int64_t L, int64_t S, int64_t A, int64_t H) {
    return L >= 2 && L <= SRLX_SEQ_MAX_L && S >= 1 && S < L && A >= 1 && A <= SRLX_SEQ_MAX_A && H >= 1 && H <= SRLX_SEQ_MAX_H;
}

i64 record_dwords(int64_t L, int64_t S, int64_t A, int64_t H) { return (4 * L + S + 1 + 4 * H + (S * A + 3) / 4 + 3) / 4 * 4; }

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t srlx_seq_record_dwords(int64_t L, int64_t S, int64_t A, int64_t H) { return in_envelope(L, S, A, H) ? record_dwords(L, S, A, H) : -1; }

int srlx_seq_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t frame_capacity, int64_t seq_capacity,
                    int64_t record_stride, const int64_t *d_slots, const float *d_ring, const int32_t *d_records, float *d_states, int64_t *d_actions,
                    float *d_r_ext, float *d_r_int, float *d_dones, uint8_t *d_invalid, int64_t *d_actor, float *d_h_ext, float *d_c_ext, float *d_h_int,
                    float *d_c_int, void *stream) {
    SRLX_REQUIRE(B >= 1 && B <= SRLX_SEQ_MAX_B, "srlx_seq_gather: batch %lld outside 1..%d", (long long)B, SRLX_SEQ_MAX_B);
    SRLX_REQUIRE(L >= 2 && L <= SRLX_SEQ_MAX_L, "srlx_seq_gather: window L %lld outside 2..%d", (long long)L, SRLX_SEQ_MAX_L);
    SRLX_REQUIRE(S >= 1 && S < L, "srlx_seq_gather: sequence length S %lld must be in 1..L-1 (L %lld)", (long long)S, (long long)L);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_seq_gather: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_seq_gather: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_seq_gather: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_seq_gather: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(frame_capacity >= 1 && frame_capacity <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_seq_gather: frame_capacity %lld outside 1..2^31-1",
                 (long long)frame_capacity);
    SRLX_REQUIRE(seq_capacity >= 1, "srlx_seq_gather: seq_capacity %lld must be positive", (long long)seq_capacity);
    SRLX_REQUIRE(record_stride >= record_dwords(L, S, A, H), "srlx_seq_gather: record_stride %lld below the record's %lld dwords", (long long)record_stride,
                 (long long)record_dwords(L, S, A, H));
    SRLX_REQUIRE(d_slots && d_ring && d_records, "srlx_seq_gather: an input pointer is NULL");
    SRLX_REQUIRE(d_states && d_actions && d_r_ext && d_r_int && d_dones && d_invalid && d_actor && d_h_ext && d_c_ext && d_h_int && d_c_int,
                 "srlx_seq_gather: an output pointer is NULL");
    SeqGatherArgs a{};
    a.B = B;
    a.L = (int)L;
    a.S = (int)S;
    a.A = (int)A;
    a.H = (int)H;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.frame_capacity = frame_capacity;
    a.seq_capacity = seq_capacity;
    a.record_stride = record_stride;
    a.slots = d_slots;
    a.ring = d_ring;
    a.records = d_records;
    a.states = d_states;
    a.actions = d_actions;
    a.r_ext = d_r_ext;
    a.r_int = d_r_int;
    a.dones = d_dones;
    a.invalid = d_invalid;
    a.actor = d_actor;
    a.h_ext = d_h_ext;
    a.c_ext = d_c_ext;
    a.h_int = d_h_int;
    a.c_int = d_c_int;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_ring) && aligned16(d_states);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)(B * L + B), (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_seq_gather<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_seq_gather<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_seq_lane_push(int64_t E, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t T, int64_t t, uint64_t seed, const float *d_frames,
                       const int32_t *d_action, const float *d_r_ext, const float *d_r_int, const float *d_undone, const int32_t *d_actor, const uint8_t *d_invalid,
                       const float *d_h_ext, const float *d_c_ext, const float *d_h_int, const float *d_c_int, const uint8_t *d_first, float *d_ring_frames,
                       int32_t *d_ring_scalars, uint8_t *d_ring_invalid, float *d_ring_hidden, void *stream) {
    SRLX_REQUIRE(E >= 1 && E <= SRLX_SEQ_MAX_LANES, "srlx_seq_lane_push: lanes E %lld outside 1..%d", (long long)E, SRLX_SEQ_MAX_LANES);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_seq_lane_push: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_seq_lane_push: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_seq_lane_push: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_seq_lane_push: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(T >= 2 && T * E <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_seq_lane_push: ring length T %lld outside 2..(2^31-1)/E", (long long)T);
    SRLX_REQUIRE(t >= 0, "srlx_seq_lane_push: position t %lld is negative", (long long)t);
    SRLX_REQUIRE(d_frames && d_action && d_r_ext && d_r_int && d_undone && d_actor && d_h_ext && d_c_ext && d_h_int && d_c_int && d_first,
                 "srlx_seq_lane_push: an input pointer is NULL (only the invalid mask may be)");
    SRLX_REQUIRE(d_ring_frames && d_ring_scalars && d_ring_invalid && d_ring_hidden, "srlx_seq_lane_push: a ring pointer is NULL");
    LanePushArgs a{};
    a.E = (int)E;
    a.A = (int)A;
    a.H = (int)H;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.T = T;
    a.t = t;
    a.seed = seed;
    a.frames = d_frames;
    a.action = d_action;
    a.r_ext = d_r_ext;
    a.r_int = d_r_int;
    a.undone = d_undone;
    a.actor = d_actor;
    a.invalid = d_invalid;
    a.h_ext = d_h_ext;
    a.c_ext = d_c_ext;
    a.h_int = d_h_int;
    a.c_int = d_c_int;
    a.first = d_first;
    a.ring_frames = d_ring_frames;
    a.ring_scal = d_ring_scalars;
    a.ring_invalid = d_ring_invalid;
    a.ring_hidden = d_ring_hidden;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_frames) && aligned16(d_ring_frames);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)E, (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_seq_lane_push<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_seq_lane_push<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_seq_lane_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t E, int64_t T, int64_t frame_elems, int64_t frame_stride, uint64_t seed,
                         const int64_t *d_desc, const float *d_ring_frames, const int32_t *d_ring_scalars, const uint8_t *d_ring_invalid, const float *d_ring_hidden,
                         float *d_states, int64_t *d_actions, float *d_r_ext, float *d_r_int, float *d_dones, uint8_t *d_invalid, int64_t *d_actor, float *d_h_ext,
                         float *d_c_ext, float *d_h_int, float *d_c_int, void *stream) {
    SRLX_REQUIRE(B >= 1 && B <= SRLX_SEQ_MAX_B, "srlx_seq_lane_gather: batch %lld outside 1..%d", (long long)B, SRLX_SEQ_MAX_B);
    SRLX_REQUIRE(L >= 2 && L <= SRLX_SEQ_MAX_L, "srlx_seq_lane_gather: window L %lld outside 2..%d", (long long)L, SRLX_SEQ_MAX_L);
    SRLX_REQUIRE(S >= 1 && S < L, "srlx_seq_lane_gather: sequence length S %lld must be in 1..L-1 (L %lld)", (long long)S, (long long)L);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_seq_lane_gather: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_seq_lane_gather: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(E >= 1 && E <= SRLX_SEQ_MAX_LANES, "srlx_seq_lane_gather: lanes E %lld outside 1..%d", (long long)E, SRLX_SEQ_MAX_LANES);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_seq_lane_gather: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_seq_lane_gather: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(T >= L && T * E <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_seq_lane_gather: ring length T %lld outside L..(2^31-1)/E", (long long)T);
    SRLX_REQUIRE(d_desc && d_ring_frames && d_ring_scalars && d_ring_invalid && d_ring_hidden, "srlx_seq_lane_gather: an input pointer is NULL");
    SRLX_REQUIRE(d_states && d_actions && d_r_ext && d_r_int && d_dones && d_invalid && d_actor && d_h_ext && d_c_ext && d_h_int && d_c_int,
                 "srlx_seq_lane_gather: an output pointer is NULL");
    LaneGatherArgs a{};
    a.B = B;
    a.L = (int)L;
    a.S = (int)S;
    a.A = (int)A;
    a.H = (int)H;
    a.E = (int)E;
    a.T = T;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.seed = seed;
    a.desc = d_desc;
    a.ring_frames = d_ring_frames;
    a.ring_scal = d_ring_scalars;
    a.ring_invalid = d_ring_invalid;
    a.ring_hidden = d_ring_hidden;
    a.states = d_states;
    a.actions = d_actions;
    a.r_ext = d_r_ext;
    a.r_int = d_r_int;
    a.dones = d_dones;
    a.invalid = d_invalid;
    a.actor = d_actor;
    a.h_ext = d_h_ext;
    a.c_ext = d_c_ext;
    a.h_int = d_h_int;
    a.c_int = d_c_int;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_ring_frames) && aligned16(d_states);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)(B * L + B), (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_seq_lane_gather<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_seq_lane_gather<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_r2d2_policy(int64_t n_envs, int64_t n_actions, const float *d_q, const float *d_eps, const double *d_u, const uint8_t *d_invalid, int32_t *d_actions,
                     float *d_mu, void *stream) {
    SRLX_REQUIRE(n_envs >= 1 && n_envs <= SRLX_SEQ_MAX_LANES, "srlx_r2d2_policy: rows n_envs %lld outside 1..%d", (long long)n_envs, SRLX_SEQ_MAX_LANES);
    SRLX_REQUIRE(n_actions >= 1 && n_actions <= SRLX_SEQ_MAX_A, "srlx_r2d2_policy: actions n_actions %lld outside 1..%d", (long long)n_actions, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(d_q && d_eps && d_u, "srlx_r2d2_policy: an input pointer is NULL (only the invalid mask may be)");
    SRLX_REQUIRE(d_actions && d_mu, "srlx_r2d2_policy: an output pointer is NULL");
    hipLaunchKernelGGL(k_r2d2_policy, dim3((unsigned)((n_envs + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (i64)n_envs, (int)n_actions, d_q,
                       d_eps, d_u, d_invalid, d_actions, d_mu);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_r2d2_lane_push(int64_t E, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t T, int64_t t, uint64_t seed, const float *d_frames,
                        const int32_t *d_action, const float *d_mu, const float *d_reward, const uint8_t *d_done, const uint8_t *d_invalid, const float *d_h,
                        const float *d_c, const uint8_t *d_first, float *d_ring_frames, int32_t *d_ring_scalars, uint8_t *d_ring_invalid, float *d_ring_hidden,
                        void *stream) {
    SRLX_REQUIRE(E >= 1 && E <= SRLX_SEQ_MAX_LANES, "srlx_r2d2_lane_push: lanes E %lld outside 1..%d", (long long)E, SRLX_SEQ_MAX_LANES);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_r2d2_lane_push: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_r2d2_lane_push: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_r2d2_lane_push: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_r2d2_lane_push: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(T >= 2 && T * E <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_r2d2_lane_push: ring length T %lld outside 2..(2^31-1)/E", (long long)T);
    SRLX_REQUIRE(t >= 0, "srlx_r2d2_lane_push: position t %lld is negative", (long long)t);
    SRLX_REQUIRE(d_frames && d_action && d_mu && d_reward && d_done && d_h && d_c && d_first,
                 "srlx_r2d2_lane_push: an input pointer is NULL (only the invalid mask may be)");
    SRLX_REQUIRE(d_ring_frames && d_ring_scalars && d_ring_invalid && d_ring_hidden, "srlx_r2d2_lane_push: a ring pointer is NULL");
    R2d2PushArgs a{};
    a.E = (int)E;
    a.A = (int)A;
    a.H = (int)H;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.T = T;
    a.t = t;
    a.seed = seed;
    a.frames = d_frames;
    a.action = d_action;
    a.mu = d_mu;
    a.reward = d_reward;
    a.done = d_done;
    a.invalid = d_invalid;
    a.h = d_h;
    a.c = d_c;
    a.first = d_first;
    a.ring_frames = d_ring_frames;
    a.ring_scal = d_ring_scalars;
    a.ring_invalid = d_ring_invalid;
    a.ring_hidden = d_ring_hidden;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_frames) && aligned16(d_ring_frames);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)E, (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_r2d2_lane_push<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_r2d2_lane_push<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_r2d2_lane_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t E, int64_t T, int64_t frame_elems, int64_t frame_stride, uint64_t seed,
                          const int64_t *d_desc, const float *d_ring_frames, const int32_t *d_ring_scalars, const uint8_t *d_ring_invalid,
                          const float *d_ring_hidden, float *d_states, int32_t *d_actions, float *d_probs, float *d_rewards, uint8_t *d_dones, uint8_t *d_invalid,
                          float *d_h, float *d_c, void *stream) {
    SRLX_REQUIRE(B >= 1 && B <= SRLX_SEQ_MAX_B, "srlx_r2d2_lane_gather: batch %lld outside 1..%d", (long long)B, SRLX_SEQ_MAX_B);
    SRLX_REQUIRE(L >= 2 && L <= SRLX_SEQ_MAX_L, "srlx_r2d2_lane_gather: window L %lld outside 2..%d", (long long)L, SRLX_SEQ_MAX_L);
    SRLX_REQUIRE(S >= 1 && S < L, "srlx_r2d2_lane_gather: sequence length S %lld must be in 1..L-1 (L %lld)", (long long)S, (long long)L);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_r2d2_lane_gather: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_r2d2_lane_gather: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(E >= 1 && E <= SRLX_SEQ_MAX_LANES, "srlx_r2d2_lane_gather: lanes E %lld outside 1..%d", (long long)E, SRLX_SEQ_MAX_LANES);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_r2d2_lane_gather: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_r2d2_lane_gather: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(T >= L && T * E <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_r2d2_lane_gather: ring length T %lld outside L..(2^31-1)/E", (long long)T);
    SRLX_REQUIRE(d_desc && d_ring_frames && d_ring_scalars && d_ring_invalid && d_ring_hidden, "srlx_r2d2_lane_gather: an input pointer is NULL");
    SRLX_REQUIRE(d_states && d_actions && d_probs && d_rewards && d_dones && d_invalid && d_h && d_c, "srlx_r2d2_lane_gather: an output pointer is NULL");
    R2d2GatherArgs a{};
    a.B = B;
    a.L = (int)L;
    a.S = (int)S;
    a.A = (int)A;
    a.H = (int)H;
    a.E = (int)E;
    a.T = T;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.seed = seed;
    a.desc = d_desc;
    a.ring_frames = d_ring_frames;
    a.ring_scal = d_ring_scalars;
    a.ring_invalid = d_ring_invalid;
    a.ring_hidden = d_ring_hidden;
    a.states = d_states;
    a.actions = d_actions;
    a.probs = d_probs;
    a.rewards = d_rewards;
    a.dones = d_dones;
    a.invalid = d_invalid;
    a.h = d_h;
    a.c = d_c;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_ring_frames) && aligned16(d_states);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)(B * L + B), (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_r2d2_lane_gather<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_r2d2_lane_gather<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
