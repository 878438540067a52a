// srlx_sacd.hip -- the whole update of discrete soft actor-critic (srl/algorithms/sac/sac_tf_discrete.py:158-243) on flat observations in five launches, and a
// forward-only pass.  Five small MLPs: the policy (in -> policy_block -> out_layer, A logits) and two Q-networks with their targets
// (concat(state, one-hot action) -> q_block -> Linear(1)).  The arithmetic contract is DESIGN.md 7m; its closed forms are srlx_sacd_math.h.
//
// The work is srlx_mlpq.hip's, not a GEMM's (<= 256 x 16 rows through layers of <= 512 units), and so is the shape: 256 threads over <= 16 rows, each layer's
// weight staged through LDS in tiles of whole rows (srlx_mlp_rows.h, which both files share: here with float64 accumulators), hidden rows and their gradients
// kept in per-layer planes, one thread per parameter for the weight gradient (a sum over the batch in item order) with torch's Adam in the same thread.  A <= 16, so the A
// one-hot rows of one item are rows of one workgroup: 16 / A items per workgroup wherever every action is evaluated.
//   k_sacd_target   policy(s') and both TARGET Q-networks over every action of s', then y (soft_target)
//   k_sacd_q_rows   blockIdx.y = q1 | q2: forward over (s, e_a), the squared error against y, the backward chain d loss / d h_l
//   k_sacd_grad     one thread per parameter of the segments it is given: gradient, Adam, and for a Q-network the target element's hard or soft sync.
//                   Launched for q1 + q2, then for the policy; the policy's launch also reduces the four losses and takes the temperature's Adam step
//   k_sacd_policy   both ONLINE Q-networks (as the Q step left them) over every action of s, policy(s), policy_row, the backward chain
//   k_sacd_forward  logits and min(q1, q2) over every action of n rows, online or target
// and, for the device engine, outside the update:
//   k_sacd_act         the policy's logits of ring rows and the Worker's action (uniform while start_steps last, Gumbel-max after), one launch per lock-step
//   k_sacd_ring_batch  the drawn items' rows out of the ring as the update's dense tensors
// No atomics and a fixed order in every sum: equal inputs give equal bits.
#include "srlx_param_tail.h"
#include "srlx_sacd_math.h"
#include <cmath>

namespace {

using i64 = int64_t;
using u8 = unsigned char;

using srlxm::kRows;
using srlxm::kThreads;
constexpr int kNets = 5;      // policy, q1_online, q1_target, q2_online, q2_target
constexpr int kMaxSegs = 16;  // q1 + q2: 2 networks x 4 layers x (weight, bias)

// one network in device memory: the policy has In = D and Out = A, a Q-network In = D + A and Out = 1
using NetD = srlxm::Layers;

struct Seg {  // one parameter tensor of a trained network
    i64 end;       // running element count
    int out, in;   // in = 0: a bias
    int opt, pad;  // whose Adam step: 0 policy, 1 q1, 2 q2
    const float *dout, *xin;  // [B][out] d loss / d (layer output), [B][in] the layer's input rows
    float *p, *g, *m, *v;
    float *tgt;  // the target network's tensor (Q-networks), NULL for the policy
};

}  // namespace

struct srlx_sacd {
    int D, A, Lp, Lq, device;
    int Wp[3], Wq[3];
    int wmax;  // the widest row in LDS: max(D + A, every width)
    int wmax_policy;  // the same over the policy alone: max(D, its widths) -- k_sacd_act's rows
    i64 max_batch;
    float *p[kNets][8];
    float *log_alpha;
    float *g[3][8], *g_log_alpha;  // policy, q1, q2
    float *m[3][8], *v[3][8], *m_la, *v_la;
    double beta1, beta2, eps;
    i64 steps[4];  // optimiser steps taken: policy, q1, q2, alpha
    bool bound, grads_bound, adam_bound, table_ok, nets_ok;
    // device scratch
    NetD *d_nets;
    Seg *d_segs;  // [0, nq): q1 then q2; [kMaxSegs, kMaxSegs + np): the policy
    float *x0;    // [max_batch][D + A]: the Q step's input rows
    float *h, *dh;  // planes [net 0..2][layer 0..2][max_batch][wmax]
    float *dlast;   // [3][max_batch][16]: d loss / d (out layer output)
    float *rows;    // [3][max_batch]: squared errors of q1, q2; the policy loss rows
};

namespace {

int n_tensors_policy(const srlx_sacd *h) { return 2 * (h->Lp + 1); }
int n_tensors_q(const srlx_sacd *h) { return 2 * (h->Lq + 1); }
int lds_stride(const srlx_sacd *h) { return h->wmax + 1; }
size_t lds_bytes(const srlx_sacd *h) { return srlxt::row_lds_bytes(2, h->wmax); }
int act_lds_stride(const srlx_sacd *h) { return h->wmax_policy + 1; }
size_t act_lds_bytes(const srlx_sacd *h) { return srlxt::row_lds_bytes(2, h->wmax_policy); }

// the whole network over the rows in buf0; returns the buffer that holds the output rows, behind a barrier (srlx_mlp_rows.h: the kept planes)
__device__ __forceinline__ float *forward_rows(const NetD &n, int rows, float *buf0, float *buf1, int S, float *wl, float *keep, i64 keep_plane, i64 keep_row0,
                                               int kept) {
    return srlxm::forward_rows<double>(n, n.L + 1, rows, buf0, buf1, S, wl, keep, keep_plane, keep_row0, kept);
}

// rows r * A + a of buf = concat(state of item i0 + r, e_a), for r < nb
__device__ __forceinline__ void load_all_action_rows(const float *__restrict__ states, i64 i0, int nb, int D, int A, float *buf, int S) {
    const int In = D + A;
    for (int p = threadIdx.x; p < nb * A * In; p += kThreads) {
        const int rr = p / In, k = p % In, r = rr / A, a = rr % A;
        buf[rr * S + k] = k < D ? states[(i0 + r) * D + k] : (k - D == a ? 1.f : 0.f);
    }
}

// min(qa, qb)(state, e_a) for every action of items i0..i0+nb-1 into qm[r * A + a] (LDS).  Begins and ends behind a barrier.
__device__ __forceinline__ void min_q_all_actions(const NetD &qa, const NetD &qb, const float *__restrict__ states, i64 i0, int nb, int D, int A, float *b0, float *b1,
                                                  int S, float *wl, float *qm) {
    const int t = threadIdx.x;
    __syncthreads();
    load_all_action_rows(states, i0, nb, D, A, b0, S);
    __syncthreads();
    const float *q = forward_rows(qa, nb * A, b0, b1, S, wl, nullptr, 0, 0, 0);
    if (t < nb * A) qm[t] = q[t * S];
    __syncthreads();
    load_all_action_rows(states, i0, nb, D, A, b0, S);
    __syncthreads();
    q = forward_rows(qb, nb * A, b0, b1, S, wl, nullptr, 0, 0, 0);
    if (t < nb * A) {
        const float v = q[t * S];
        qm[t] = v < qm[t] ? v : qm[t];
    }
    __syncthreads();
}

// the policy's logits of items i0..i0+nb-1 into lg[r * A + a] (LDS).  Begins and ends behind a barrier.
__device__ __forceinline__ void policy_logits(const NetD &pol, const float *__restrict__ states, i64 i0, int nb, int D, int A, float *b0, float *b1, int S, float *wl,
                                              float *lg, float *keep, i64 keep_plane) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int p = t; p < nb * D; p += kThreads) b0[(p / D) * S + p % D] = states[(i0 + p / D) * D + p % D];
    __syncthreads();
    const float *z = forward_rows(pol, nb, b0, b1, S, wl, keep, keep_plane, i0, nb);
    if (t < nb * A) lg[t] = z[(t / A) * S + t % A];
    __syncthreads();
}

struct Batch {
    i64 B;
    const float *s, *s2, *reward;
    const int32_t *action;
    const u8 *done;
    float *y;
};

__global__ void __launch_bounds__(kThreads) k_sacd_target(const NetD *__restrict__ nets, const float *__restrict__ log_alpha, Batch a, float discount, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    __shared__ float lg[kRows], qm[kRows], tmp[kRows];
    const int ipw = kRows / A;
    const i64 i0 = (i64)blockIdx.x * ipw;
    const int nb = (int)(a.B - i0 < ipw ? a.B - i0 : ipw);
    policy_logits(nets[0], a.s2, i0, nb, D, A, b0, b1, S, wl, lg, nullptr, 0);
    min_q_all_actions(nets[2], nets[4], a.s2, i0, nb, D, A, b0, b1, S, wl, qm);
    const int t = threadIdx.x;
    if (t < nb) {
        const float alpha = expf(log_alpha[0]);
        const i64 b = i0 + t;
        a.y[b] = srlxs::soft_target(lg + t * A, qm + t * A, A, alpha, a.reward[b], a.done[b] ? 1.f : 0.f, discount, tmp + t * A);
    }
}

struct QStep {
    float *x0, *h, *dh, *dlast, *rows;
    float *q1, *q2;
    i64 plane, max_batch;
};

__global__ void __launch_bounds__(kThreads) k_sacd_q_rows(const NetD *__restrict__ nets, Batch a, QStep w, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    const int t = threadIdx.x, which = blockIdx.y;  // 0: q1, 1: q2
    const NetD &n = nets[which == 0 ? 1 : 3];
    const i64 i0 = (i64)blockIdx.x * kRows;
    const int nb = (int)(a.B - i0 < kRows ? a.B - i0 : kRows);
    const int In = D + A;
    for (int p = t; p < nb * In; p += kThreads) {
        const int r = p / In, k = p % In;
        const float x = k < D ? a.s[(i0 + r) * D + k] : (k - D == a.action[i0 + r] ? 1.f : 0.f);
        b0[r * S + k] = x;
        if (which == 0) w.x0[(i0 + r) * In + k] = x;
    }
    __syncthreads();
    const i64 net_planes = (i64)(1 + which) * 3 * w.plane;
    float *q = forward_rows(n, nb, b0, b1, S, wl, w.h + net_planes, w.plane, i0, nb);
    float *other = q == b0 ? b1 : b0;
    float dq = 0.f;
    if (t < nb) {
        const i64 b = i0 + t;
        const float qv = q[t * S];
        (which == 0 ? w.q1 : w.q2)[b] = qv;
        const float diff = qv - a.y[b];
        w.rows[(i64)which * w.max_batch + b] = diff * diff;
        dq = (2.f * diff) / (float)a.B;  // d mean_b (y - q)^2 / d q_b
        w.dlast[((i64)(1 + which) * w.max_batch + b) * kRows] = dq;
    }
    __syncthreads();
    if (t < nb) q[t * S] = dq;
    __syncthreads();
    srlxm::backward_rows<double>(n, n.L - 1, nb, i0, other, q, S, w.h + net_planes, w.dh + net_planes, w.plane);  // (q: the rows' d loss / d q in column 0)
}

struct PStep {
    float *h, *dh, *dlast, *rows, *entropy;
    i64 plane, max_batch;
};

__global__ void __launch_bounds__(kThreads) k_sacd_policy(const NetD *__restrict__ nets, const float *__restrict__ log_alpha, Batch a, PStep w, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    __shared__ float lg[kRows], qm[kRows], dz[kRows], tp[kRows], tc[kRows];
    const int t = threadIdx.x;
    const int ipw = kRows / A;
    const i64 i0 = (i64)blockIdx.x * ipw;
    const int nb = (int)(a.B - i0 < ipw ? a.B - i0 : ipw);
    min_q_all_actions(nets[1], nets[3], a.s, i0, nb, D, A, b0, b1, S, wl, qm);
    policy_logits(nets[0], a.s, i0, nb, D, A, b0, b1, S, wl, lg, w.h, w.plane);
    if (t < nb) {
        const float alpha = expf(log_alpha[0]);
        const i64 b = i0 + t;
        float ent, ls;
        srlxs::policy_row(lg + t * A, qm + t * A, A, alpha, 1.f / (float)a.B, &ent, &ls, dz + t * A, tp + t * A, tc + t * A);
        w.entropy[b] = ent;
        w.rows[2 * w.max_batch + b] = ls;
    }
    __syncthreads();
    if (t < nb * A) {
        b0[(t / A) * S + t % A] = dz[t];
        w.dlast[(i0 + t / A) * kRows + t % A] = dz[t];
    }
    __syncthreads();
    srlxm::backward_rows<double>(nets[0], nets[0].L - 1, nb, i0, b1, b0, S, w.h, w.dh, w.plane);  // (b0: the rows' d loss / d logits)
}

__global__ void __launch_bounds__(kThreads) k_sacd_forward(const NetD *__restrict__ nets, int target, i64 n, const float *__restrict__ states, float *__restrict__ logits,
                                                           float *__restrict__ qmin, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    __shared__ float lg[kRows], qm[kRows];
    const int t = threadIdx.x;
    const int ipw = kRows / A;
    const i64 i0 = (i64)blockIdx.x * ipw;
    const int nb = (int)(n - i0 < ipw ? n - i0 : ipw);
    if (logits) {
        policy_logits(nets[0], states, i0, nb, D, A, b0, b1, S, wl, lg, nullptr, 0);
        if (t < nb * A) logits[i0 * A + t] = lg[t];
    }
    if (qmin) {
        min_q_all_actions(nets[target ? 2 : 1], nets[target ? 4 : 3], states, i0, nb, D, A, b0, b1, S, wl, qm);
        if (t < nb * A) qmin[i0 * A + t] = qm[t];
    }
}

// The Worker's policy() for the lanes of a lock-step (algorithms/sac.py:334-338): the policy's logits of `rpw` <= 16 rows per workgroup (rows from a
// ring through an offset table), then one thread per (row, action) for the keyed uniform, the rescaled uniform and the Gumbel score in float64, then one
// thread per row for the first maximum -- or, while *counter < random_until, the uniform random action.  A row's logits are the same fma chains whatever rows
// share its workgroup, so `rpw` changes the launch shape and never a bit.  The scores stand in the weight tile once the network is done with it.
struct ActArgs {
    i64 n;
    const float *obs;
    const i64 *off;  // NULL: row r at obs + r * D
    srlx::u64 seed;
    const i64 *counter;
    i64 random_until;
    int32_t *actions;
    float *logits;   // NULL: not wanted
    double *scores;  // NULL: not wanted
};

__global__ void __launch_bounds__(kThreads) k_sacd_act(const NetD *__restrict__ nets, ActArgs a, int rpw, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    double *sc = (double *)wl;  // [rpw][A] (2 * kRows * S floats in front of it: a multiple of 16 bytes)
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(a.n - i0 < rpw ? a.n - i0 : rpw);
    const srlx::u64 c = (srlx::u64)a.counter[0];
    const bool random = a.counter[0] < a.random_until;
    if (!random || a.logits || a.scores) {  // (the same answer in every thread of the launch)
        for (int p = t; p < nb * D; p += kThreads) {
            const int r = p / D, k = p % D;
            b0[r * S + k] = (a.off ? a.obs + a.off[i0 + r] : a.obs + (i0 + r) * D)[k];
        }
        __syncthreads();
        const float *z = forward_rows(nets[0], nb, b0, b1, S, wl, nullptr, 0, 0, 0);
        if (t < nb * A) {
            const int r = t / A, j = t % A;
            const i64 e = (i0 + r) * A + j;
            const float zv = z[r * S + j];
            const double s = srlxs::gumbel_score(zv, srlxs::gumbel_uniform(srlx::u53(srlx::rng_u64(a.seed, c, (srlx::u64)e))));
            sc[t] = s;
            if (a.logits) a.logits[e] = zv;
            if (a.scores) a.scores[e] = s;
        }
        __syncthreads();
    }
    if (t < nb) {
        const i64 r = i0 + t;
        a.actions[r] = random ? srlxs::random_action(srlx::u53(srlx::rng_u64(a.seed, c, (srlx::u64)(r * A))), A) : srlxs::first_argmax(sc + t * A, A);
    }
}

// The items a uniform draw named, as srlx_sacd_update's tensors: one workgroup per item copies s and s' out of the ring (16 bytes per access where the
// rows allow), one-hot encodes the action and turns `terminated` into the update's done byte.
struct RingBatchArgs {
    const float *obs;
    const i64 *off;  // [B][2]: s, s'
    const int32_t *actions;
    const float *terminated;
    float *states, *next_states, *onehot;
    u8 *done;
    int D, A, vec;
};

__global__ void __launch_bounds__(128) k_sacd_ring_batch(RingBatchArgs a) {
    const i64 b = blockIdx.x;
    const int t = threadIdx.x, D = a.D;
    const i64 o0 = a.off[2 * b], o1 = a.off[2 * b + 1];
    const float *s0 = a.obs + o0, *s1 = a.obs + o1;
    float *d0 = a.states + b * D, *d1 = a.next_states + b * D;
    if (a.vec && ((o0 | o1) & 3) == 0) {
        const int q = D / 4;
        for (int i = t; i < 2 * q; i += 128) {
            const bool nx = i >= q;
            const int k = nx ? i - q : i;
            ((float4 *)(nx ? d1 : d0))[k] = ((const float4 *)(nx ? s1 : s0))[k];
        }
    } else {
        for (int i = t; i < 2 * D; i += 128) {
            const bool nx = i >= D;
            const int k = nx ? i - D : i;
            (nx ? d1 : d0)[k] = (nx ? s1 : s0)[k];
        }
    }
    if (t < a.A) a.onehot[b * a.A + t] = t == a.actions[b] ? 1.f : 0.f;
    if (t == 0) a.done[b] = a.terminated[b] != 0.f ? 1 : 0;
}

struct GradArgs {
    const Seg *segs;
    int nseg;
    i64 B;
    const float *xin0;  // the input rows of a first layer whose segment names none (the policy's: the caller's states)
    double lr0, lr1, lr2, beta1, beta2, eps;  // lr of opt 0 (policy), 1 (q1), 2 (q2)
    i64 st0, st1, st2;                        // their steps taken
    int sync;                                 // Q-networks: 1 = hard (copy), 2 = soft
    float one_minus_tau, tau;
};

struct Tail {  // rides on the policy's launch: the loss reduction and the temperature
    const float *rows, *entropy;
    i64 max_batch;
    float *log_alpha, *g_la, *m_la, *v_la;
    int auto_scale;
    float target_entropy;
    double lr_alpha;
    i64 st_alpha;
    float *out;  // q1_loss, q2_loss, policy_loss, alpha_loss, alpha
};

__device__ __forceinline__ void tail_body(const GradArgs &a, const Tail &z, int t) {
    if (t < 3) {
        double s = 0.0;
        for (i64 b = 0; b < a.B; b++) s += (double)z.rows[t * z.max_batch + b];
        z.out[t] = (float)(s / (double)a.B);
        return;
    }
    // :226-233: alpha_loss = -mean_b(alpha (target_entropy - entropy_b)); d alpha_loss / d log_alpha is the same number
    const float alpha = expf(z.log_alpha[0]);
    z.out[4] = alpha;
    if (!z.auto_scale) {
        z.out[3] = 0.f;
        if (z.g_la) z.g_la[0] = 0.f;
        return;
    }
    double s = 0.0;
    for (i64 b = 0; b < a.B; b++) s += (double)(alpha * (z.target_entropy - z.entropy[b]));
    const float g = -(float)(s / (double)a.B);
    z.out[3] = g;
    if (z.g_la) z.g_la[0] = g;
    const srlx::AdamCoef c = srlx::adam_coef(z.lr_alpha, a.beta1, a.beta2, a.eps, z.st_alpha);
    float p = z.log_alpha[0], m = z.m_la[0], v = z.v_la[0];
    srlx::adam_one_foreach(p, g, m, v, c);
    z.log_alpha[0] = p, z.m_la[0] = m, z.v_la[0] = v;
}

template <bool TAIL>
__global__ void __launch_bounds__(kThreads) k_sacd_grad(GradArgs a, Tail z) {
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    if constexpr (TAIL) {
        // (the last block's last four threads: the launch rounds the element count + 4 up, so they exist and own no element)
        const i64 last = (i64)gridDim.x * kThreads;
        if (i >= last - 4) {
            tail_body(a, z, (int)(i - (last - 4)));
            return;
        }
    }
    const Seg *segs = a.segs;
    if (i >= segs[a.nseg - 1].end) return;
    int s = 0;
    while (i >= segs[s].end) s++;
    const Seg sg = segs[s];
    const i64 e = i - (s ? segs[s - 1].end : 0);
    const int Out = sg.out, In = sg.in;
    double acc = 0.0;
    if (In) {
        const int u = (int)(e / In), k = (int)(e % In);
        const float *dout = sg.dout + u, *xin = (sg.xin ? sg.xin : a.xin0) + k;
#pragma unroll 8
        for (int b = 0; b < (int)a.B; b++) acc = fma((double)dout[(i64)b * Out], (double)xin[(i64)b * In], acc);
    } else {
        const float *dout = sg.dout + e;
#pragma unroll 8
        for (int b = 0; b < (int)a.B; b++) acc += (double)dout[(i64)b * Out];
    }
    const float g = (float)acc;
    sg.g[e] = g;
    const double lr = sg.opt == 0 ? a.lr0 : (sg.opt == 1 ? a.lr1 : a.lr2);
    const i64 st = sg.opt == 0 ? a.st0 : (sg.opt == 1 ? a.st1 : a.st2);
    const srlx::AdamCoef c = srlx::adam_coef(lr, a.beta1, a.beta2, a.eps, st);
    float p = sg.p[e], m = sg.m[e], v = sg.v[e];
    srlx::adam_one_foreach(p, g, m, v, c);
    sg.p[e] = p, sg.m[e] = m, sg.v[e] = v;
    if (sg.tgt) sg.tgt[e] = a.sync == 1 ? p : srlxs::soft_sync(sg.tgt[e], p, a.one_minus_tau, a.tau);
}

int set_lds(const void *fn, size_t bytes) {
    if (bytes > 65536) SRLX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return SRLX_OK;
}

int check_shape(const char *who, int D, int A, int n_policy, const int *pw, int n_q, const int *qw, i64 max_batch) {
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(A >= 2 && A <= 16, "%s: %d actions (2..16)", who, A);
    SRLX_REQUIRE(srlxt::widths_ok(n_policy, 1, 3, pw), "%s: the policy block is 1..3 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(srlxt::widths_ok(n_q, 1, 3, qw), "%s: the q block is 1..3 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(max_batch >= 1 && max_batch <= 256, "%s: max_batch %lld (1..256)", who, (long long)max_batch);
    return SRLX_OK;
}

int wmax_of(int D, int A, int n_policy, const int *pw, int n_q, const int *qw) {
    int w = D + A;
    for (int l = 0; l < n_policy; l++) w = pw[l] > w ? pw[l] : w;
    for (int l = 0; l < n_q; l++) w = qw[l] > w ? qw[l] : w;
    return w;
}

// (out, in) of tensor pair l of a network with `L` hidden layers
void layer_shape(int In, int L, const int *W, int Out, int l, int *out, int *in) {
    *in = l == 0 ? In : W[l - 1];
    *out = l < L ? W[l] : Out;
}

NetD net_of(const srlx_sacd *h, int k) {
    return k == 0 ? srlxt::chain(h->D, h->Lp, h->Wp, h->A, h->p[0]) : srlxt::chain(h->D + h->A, h->Lq, h->Wq, 1, h->p[k]);
}

// the segment tables of the two gradient launches, from everything that is bound
int upload_tables(srlx_sacd *h) {
    NetD nets[kNets];
    for (int k = 0; k < kNets; k++) nets[k] = net_of(h, k);
    SRLX_HIP(hipMemcpy(h->d_nets, nets, sizeof(nets), hipMemcpyHostToDevice));
    Seg segs[2 * kMaxSegs];
    memset(segs, 0, sizeof(segs));
    const i64 plane = h->max_batch * h->wmax;
    i64 end = 0;
    int s = 0;
    for (int q = 0; q < 2; q++) {  // q1, q2
        const int net = 1 + 2 * q, t = 1 + q;
        for (int l = 0; l <= h->Lq; l++) {
            int out, in;
            layer_shape(h->D + h->A, h->Lq, h->Wq, 1, l, &out, &in);
            const float *dout = l < h->Lq ? h->dh + ((i64)t * 3 + l) * plane : h->dlast + (i64)t * h->max_batch * kRows;
            const float *xin = l == 0 ? h->x0 : h->h + ((i64)t * 3 + l - 1) * plane;
            for (int k = 0; k < 2; k++, s++) {
                Seg &g = segs[s];
                end += k == 0 ? (i64)out * in : out;
                g.end = end, g.out = l < h->Lq ? out : kRows, g.in = k == 0 ? in : 0, g.opt = t;
                g.dout = dout, g.xin = xin;
                g.p = h->p[net][2 * l + k], g.g = h->g[t][2 * l + k], g.m = h->m[t][2 * l + k], g.v = h->v[t][2 * l + k];
                g.tgt = h->p[net + 1][2 * l + k];
            }
        }
    }
    end = 0, s = kMaxSegs;
    for (int l = 0; l <= h->Lp; l++) {
        int out, in;
        layer_shape(h->D, h->Lp, h->Wp, h->A, l, &out, &in);
        const float *dout = l < h->Lp ? h->dh + (i64)l * plane : h->dlast;
        for (int k = 0; k < 2; k++, s++) {
            Seg &g = segs[s];
            end += k == 0 ? (i64)out * in : out;
            g.end = end, g.out = l < h->Lp ? out : kRows, g.in = k == 0 ? in : 0, g.opt = 0;
            g.dout = dout, g.xin = l == 0 ? nullptr : h->h + (i64)(l - 1) * plane;  // (layer 0 reads the caller's states: GradArgs.xin0)
            g.p = h->p[0][2 * l + k], g.g = h->g[0][2 * l + k], g.m = h->m[0][2 * l + k], g.v = h->v[0][2 * l + k];
            g.tgt = nullptr;
        }
    }
    SRLX_HIP(hipMemcpy(h->d_segs, segs, sizeof(segs), hipMemcpyHostToDevice));
    h->table_ok = h->nets_ok = true;
    return SRLX_OK;
}

i64 elements(int In, int L, const int *W, int Out) {
    i64 n = 0;
    for (int l = 0; l <= L; l++) {
        int out, in;
        layer_shape(In, L, W, Out, l, &out, &in);
        n += (i64)out * in + out;
    }
    return n;
}

}  // namespace

extern "C" {

int64_t srlx_sacd_scratch_floats(int obs_dim, int n_actions, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int64_t max_batch) {
    if (check_shape("sacd_scratch_floats", obs_dim, n_actions, n_policy, policy_widths, n_q, q_widths, max_batch) != SRLX_OK) return -1;
    const i64 wmax = wmax_of(obs_dim, n_actions, n_policy, policy_widths, n_q, q_widths);
    return max_batch * (obs_dim + n_actions) + 2 * 9 * max_batch * wmax + 3 * max_batch * kRows + 3 * max_batch;
}

int srlx_sacd_create(srlx_sacd_t **out, int obs_dim, int n_actions, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int64_t max_batch,
                     int device) {
    SRLX_REQUIRE(out, "sacd_create: NULL handle pointer");
    *out = nullptr;
    SRLX_TRY(check_shape("sacd_create", obs_dim, n_actions, n_policy, policy_widths, n_q, q_widths, max_batch));
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "sacd_create: device %d unavailable", device);
    srlx_sacd *h = new srlx_sacd();
    h->D = obs_dim, h->A = n_actions, h->Lp = n_policy, h->Lq = n_q, h->device = device, h->max_batch = max_batch;
    for (int l = 0; l < n_policy; l++) h->Wp[l] = policy_widths[l];
    for (int l = 0; l < n_q; l++) h->Wq[l] = q_widths[l];
    h->wmax = wmax_of(obs_dim, n_actions, n_policy, policy_widths, n_q, q_widths);
    h->wmax_policy = wmax_of(obs_dim, 0, n_policy, policy_widths, 0, nullptr);
    const size_t plane = (size_t)max_batch * h->wmax;
    hipError_t e = hipMalloc((void **)&h->d_nets, sizeof(NetD) * kNets);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_segs, sizeof(Seg) * 2 * kMaxSegs);
    if (e == hipSuccess) e = hipMalloc((void **)&h->x0, sizeof(float) * max_batch * (obs_dim + n_actions));
    if (e == hipSuccess) e = hipMalloc((void **)&h->h, sizeof(float) * 9 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dh, sizeof(float) * 9 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dlast, sizeof(float) * 3 * max_batch * kRows);
    if (e == hipSuccess) e = hipMalloc((void **)&h->rows, sizeof(float) * 3 * max_batch);
    if (e == hipSuccess) e = hipMemset(h->dlast, 0, sizeof(float) * 3 * max_batch * kRows);
    if (e != hipSuccess) {
        srlx_sacd_destroy(h);
        srlx::set_error("sacd_create: hipMalloc failed: %s", hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    const size_t lds = lds_bytes(h);
    int st = set_lds((const void *)k_sacd_target, lds);
    if (st == SRLX_OK) st = set_lds((const void *)k_sacd_q_rows, lds);
    if (st == SRLX_OK) st = set_lds((const void *)k_sacd_policy, lds);
    if (st == SRLX_OK) st = set_lds((const void *)k_sacd_forward, lds);
    if (st == SRLX_OK) st = set_lds((const void *)k_sacd_act, srlxt::kLdsCap2);
    if (st != SRLX_OK) {
        srlx_sacd_destroy(h);
        return st;
    }
    *out = h;
    return SRLX_OK;
}

int srlx_sacd_destroy(srlx_sacd_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (void *p : {(void *)h->d_nets, (void *)h->d_segs, (void *)h->x0, (void *)h->h, (void *)h->dh, (void *)h->dlast, (void *)h->rows})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_sacd_bind(srlx_sacd_t *h, float *const *d_params, float *d_log_alpha) {
    SRLX_REQUIRE(h && d_params && d_log_alpha, "sacd_bind: NULL argument");
    int i = 0;
    for (int k = 0; k < kNets; k++)
        for (int t = 0; t < (k == 0 ? n_tensors_policy(h) : n_tensors_q(h)); t++, i++) {
            SRLX_REQUIRE(d_params[i], "sacd_bind: parameter %d is NULL", i);
            h->p[k][t] = d_params[i];
        }
    h->log_alpha = d_log_alpha;
    h->bound = true, h->table_ok = h->nets_ok = false;
    return SRLX_OK;
}

int srlx_sacd_bind_grads(srlx_sacd_t *h, float *const *d_grads, float *d_grad_log_alpha) {
    SRLX_REQUIRE(h && d_grads && d_grad_log_alpha, "sacd_bind_grads: NULL argument");
    int i = 0;
    for (int k = 0; k < 3; k++)
        for (int t = 0; t < (k == 0 ? n_tensors_policy(h) : n_tensors_q(h)); t++, i++) {
            SRLX_REQUIRE(d_grads[i], "sacd_bind_grads: gradient tensor %d is NULL", i);
            h->g[k][t] = d_grads[i];
        }
    h->g_log_alpha = d_grad_log_alpha;
    h->grads_bound = true, h->table_ok = false;
    return SRLX_OK;
}

int srlx_sacd_bind_adam(srlx_sacd_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, const int64_t *steps_taken, double beta1, double beta2, double eps) {
    SRLX_REQUIRE(h && d_exp_avg && d_exp_avg_sq && steps_taken, "sacd_bind_adam: NULL argument");
    SRLX_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0, "sacd_bind_adam: betas in [0, 1) and eps > 0");
    int i = 0;
    for (int k = 0; k < 3; k++)
        for (int t = 0; t < (k == 0 ? n_tensors_policy(h) : n_tensors_q(h)); t++, i++) {
            SRLX_REQUIRE(d_exp_avg[i] && d_exp_avg_sq[i], "sacd_bind_adam: state %d is NULL", i);
            h->m[k][t] = d_exp_avg[i], h->v[k][t] = d_exp_avg_sq[i];
        }
    SRLX_REQUIRE(d_exp_avg[i] && d_exp_avg_sq[i], "sacd_bind_adam: log_alpha's state is NULL");
    h->m_la = d_exp_avg[i], h->v_la = d_exp_avg_sq[i];
    for (int k = 0; k < 4; k++) {
        SRLX_REQUIRE(steps_taken[k] >= 0, "sacd_bind_adam: step counts are non-negative");
        h->steps[k] = steps_taken[k];
    }
    h->beta1 = beta1, h->beta2 = beta2, h->eps = eps;
    h->adam_bound = true, h->table_ok = false;
    return SRLX_OK;
}

int srlx_sacd_steps(const srlx_sacd_t *h, int64_t *steps_taken) {
    SRLX_REQUIRE(h && steps_taken, "sacd_steps: NULL argument");
    for (int k = 0; k < 4; k++) steps_taken[k] = h->steps[k];
    return SRLX_OK;
}

int srlx_sacd_forward(srlx_sacd_t *h, int64_t n, const float *d_states, int target, float *d_logits, float *d_qmin, void *stream) {
    SRLX_REQUIRE(h && d_states, "sacd_forward: NULL handle or states");
    SRLX_REQUIRE(h->bound, "sacd_forward: unbound handle (srlx_sacd_bind)");
    SRLX_REQUIRE(n >= 1 && n <= (int64_t)1 << 24, "sacd_forward: %lld rows (1..2^24)", (long long)n);
    SRLX_REQUIRE(d_logits || d_qmin, "sacd_forward: nothing to write");
    SRLX_REQUIRE(target == 0 || target == 1, "sacd_forward: target is 0 (online) or 1");
    srlx::DeviceGuard g(h->device);
    if (!h->nets_ok) {
        NetD nets[kNets];
        for (int k = 0; k < kNets; k++) nets[k] = net_of(h, k);
        SRLX_HIP(hipMemcpy(h->d_nets, nets, sizeof(nets), hipMemcpyHostToDevice));
        h->nets_ok = true;
    }
    const int ipw = kRows / h->A;
    hipLaunchKernelGGL(k_sacd_forward, dim3((unsigned)((n + ipw - 1) / ipw)), dim3(kThreads), lds_bytes(h), (hipStream_t)stream, (const NetD *)h->d_nets, target, (i64)n,
                       d_states, d_logits, d_qmin, h->D, h->A, lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_sacd_act(srlx_sacd_t *h, int64_t n_rows, const float *d_obs_base, const int64_t *d_row_offsets, uint64_t seed, const int64_t *d_counter,
                  int64_t random_until, int32_t *d_actions, float *d_logits, double *d_scores, void *stream) {
    SRLX_REQUIRE(h, "sacd_act: NULL handle");
    SRLX_REQUIRE(h->bound, "sacd_act: unbound handle (srlx_sacd_bind)");
    SRLX_REQUIRE(n_rows >= 1 && n_rows <= 65536, "sacd_act: %lld rows (1..65536)", (long long)n_rows);
    SRLX_REQUIRE(random_until >= 0, "sacd_act: random_until %lld is negative", (long long)random_until);
    SRLX_REQUIRE(d_obs_base && d_counter && d_actions, "sacd_act: NULL observations, counter or actions");
    srlx::DeviceGuard g(h->device);
    if (!h->nets_ok) {
        NetD nets[kNets];
        for (int k = 0; k < kNets; k++) nets[k] = net_of(h, k);
        SRLX_HIP(hipMemcpy(h->d_nets, nets, sizeof(nets), hipMemcpyHostToDevice));
        h->nets_ok = true;
    }
    const int rpw = srlxt::rows_per_workgroup(n_rows);
    ActArgs a{(i64)n_rows, d_obs_base, (const i64 *)d_row_offsets, (srlx::u64)seed, (const i64 *)d_counter, (i64)random_until, d_actions, d_logits, d_scores};
    hipLaunchKernelGGL(k_sacd_act, dim3((unsigned)((n_rows + rpw - 1) / rpw)), dim3(kThreads), act_lds_bytes(h), (hipStream_t)stream, (const NetD *)h->d_nets, a, rpw,
                       h->D, h->A, act_lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_sacd_ring_batch(int64_t B, int D, int A, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions, const float *d_rewards,
                         const float *d_terminated, float *d_states, float *d_next_states, float *d_onehot, uint8_t *d_done, void *stream) {
    SRLX_REQUIRE(B >= 1 && B <= 256, "sacd_ring_batch: batch %lld (1..256)", (long long)B);
    SRLX_REQUIRE(D >= 1 && D <= 256, "sacd_ring_batch: observation length %d (1..256)", D);
    SRLX_REQUIRE(A >= 2 && A <= 16, "sacd_ring_batch: %d actions (2..16)", A);
    // (d_rewards is the gather's [B][1] column, already the update's [B] tensor: required like the rest, handed on by the caller, not copied)
    SRLX_REQUIRE(d_obs_base && d_offsets && d_actions && d_rewards && d_terminated && d_states && d_next_states && d_onehot && d_done,
                 "sacd_ring_batch: NULL argument");
    const bool vec = D % 4 == 0 && (((uintptr_t)d_obs_base | (uintptr_t)d_states | (uintptr_t)d_next_states) & 15) == 0;
    RingBatchArgs a{d_obs_base, (const i64 *)d_offsets, d_actions, d_terminated, d_states, d_next_states, d_onehot, d_done, D, A, vec ? 1 : 0};
    hipLaunchKernelGGL(k_sacd_ring_batch, dim3((unsigned)B), dim3(128), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_sacd_update(srlx_sacd_t *h, int64_t batch, const float *d_states, const int32_t *d_actions, const float *d_next_states, const float *d_rewards,
                     const uint8_t *d_dones, double lr_policy, double lr_q, double lr_alpha, double discount, double tau, int hard_sync, int auto_scale,
                     double target_entropy, float *d_y, float *d_q1, float *d_q2, float *d_entropy, float *d_scalars, void *stream) {
    SRLX_REQUIRE(h, "sacd_update: NULL handle");
    SRLX_REQUIRE(h->bound && h->grads_bound && h->adam_bound, "sacd_update: bind the parameters, the gradient tensors and the Adam state first");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "sacd_update: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_states && d_actions && d_next_states && d_rewards && d_dones && d_y && d_q1 && d_q2 && d_entropy && d_scalars, "sacd_update: NULL argument");
    SRLX_REQUIRE(lr_policy >= 0 && lr_q >= 0 && lr_alpha >= 0, "sacd_update: learning rates are non-negative");
    SRLX_REQUIRE(tau >= 0 && tau <= 1, "sacd_update: tau %g (0..1)", tau);
    SRLX_REQUIRE((hard_sync == 0 || hard_sync == 1) && (auto_scale == 0 || auto_scale == 1), "sacd_update: hard_sync and auto_scale are 0 or 1");
    srlx::DeviceGuard g(h->device);
    if (!h->table_ok) SRLX_TRY(upload_tables(h));
    hipStream_t st = (hipStream_t)stream;
    const int S = lds_stride(h), D = h->D, A = h->A;
    const size_t lds = lds_bytes(h);
    const int ipw = kRows / A;
    const unsigned item_blocks = (unsigned)((batch + ipw - 1) / ipw);
    const i64 plane = h->max_batch * h->wmax;
    const NetD *nets = h->d_nets;
    Batch b{(i64)batch, d_states, d_next_states, d_rewards, d_actions, d_dones, d_y};
    hipLaunchKernelGGL(k_sacd_target, dim3(item_blocks), dim3(kThreads), lds, st, nets, (const float *)h->log_alpha, b, (float)discount, D, A, S);
    QStep qs{h->x0, h->h, h->dh, h->dlast, h->rows, d_q1, d_q2, plane, h->max_batch};
    hipLaunchKernelGGL(k_sacd_q_rows, dim3((unsigned)((batch + kRows - 1) / kRows), 2), dim3(kThreads), lds, st, nets, b, qs, D, A, S);
    GradArgs ga{};
    ga.B = batch;
    ga.lr0 = lr_policy, ga.lr1 = lr_q, ga.lr2 = lr_q, ga.beta1 = h->beta1, ga.beta2 = h->beta2, ga.eps = h->eps;
    ga.st0 = h->steps[0], ga.st1 = h->steps[1], ga.st2 = h->steps[2];
    ga.sync = hard_sync ? 1 : 2;
    ga.one_minus_tau = (float)(1.0 - tau), ga.tau = (float)tau;
    Tail tl{};
    ga.segs = h->d_segs, ga.nseg = 2 * n_tensors_q(h);
    const i64 nq = 2 * elements(D + A, h->Lq, h->Wq, 1);
    hipLaunchKernelGGL(k_sacd_grad<false>, dim3((unsigned)((nq + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ga, tl);
    PStep ps{h->h, h->dh, h->dlast, h->rows, d_entropy, plane, h->max_batch};
    hipLaunchKernelGGL(k_sacd_policy, dim3(item_blocks), dim3(kThreads), lds, st, nets, (const float *)h->log_alpha, b, ps, D, A, S);
    ga.segs = h->d_segs + kMaxSegs, ga.nseg = n_tensors_policy(h), ga.xin0 = d_states;
    tl.rows = h->rows, tl.entropy = d_entropy, tl.max_batch = h->max_batch;
    tl.log_alpha = h->log_alpha, tl.g_la = h->g_log_alpha, tl.m_la = h->m_la, tl.v_la = h->v_la;
    tl.auto_scale = auto_scale, tl.target_entropy = (float)target_entropy, tl.lr_alpha = lr_alpha, tl.st_alpha = h->steps[3];
    tl.out = d_scalars;
    const i64 np = elements(D, h->Lp, h->Wp, A);
    hipLaunchKernelGGL(k_sacd_grad<true>, dim3((unsigned)((np + 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ga, tl);
    SRLX_HIP(hipGetLastError());
    h->steps[0]++, h->steps[1]++, h->steps[2]++;
    if (auto_scale) h->steps[3]++;
    return SRLX_OK;
}

}  // extern "C"
