// srlx_mlpq.hip -- DQN's Q-network for flat observations (srl/algorithms/dqn/model_torch.py:17-29: in_block -> hidden_block (MLP) -> out_layer), its
// acting pass with the fused epsilon-greedy selection, the whole learner step in two launches, the online -> target / actor copy, and a batch CartPole.
//
// Every dense layer is Linear (+ ReLU except out_layer), weights in torch's [out][in] layout, plain float32 on the VALU: at D <= 256 inputs, <= 3 layers of
// <= 512 units and <= 32 actions a pass is a few thousand dependent multiply-adds per row, so launch count and the layer chain bound it, not throughput.
// The layer descriptor, dense(), the plain-layer forward loop and the hidden-layer backward chain are srlx_mlp_rows.h's, instantiated with float32 sums
// (srlx_sacd.hip runs the same code with float64 sums); the dueling head, narrow_rows() and the sparse seeds of the chain's top layer are this file's,
// and so is one kept copy of the forward loop, for k_mlpq_learn_rows and the n-step learner kernels (forward_rows<true>: why, there).
//   k_mlpq_actor      16 rows per workgroup: rows -> LDS, layer by layer through two LDS buffers (each layer's weight staged in LDS by coalesced loads, in
//                     tiles of whole rows), Q rows out, epsilon-greedy on each row (= k_head's rule).
//   k_mlpq_learn_rows 8 sampled items per workgroup: online pass over s_0 and s_1, target pass over s_1, the 1-step (double) DQN target / Huber / priority of
//                     srlx_td_math.h:td_rows, then the backward chain d loss / d h_l of every layer for these rows (the chain is row-local).  Writes the
//                     s_0 activations and the d h_l rows.
//   k_mlpq_learn_nstep<n>  Rainbow's update (rainbow/model_torch.py:15-29, rainbow.py:185-287) on the same layers: 16 / (n + 1) items per workgroup, online pass
//                     over s_0..s_n, target pass over s_1..s_n, the n-step retrace target, then the backward chain -- through out_layer, or through the
//                     dueling head (forward_rows: MLP trunk of 0..2 layers, then v_layers / adv_layers; srl/rl/torch_/blocks/dueling_network.py:8-59).
//   k_mlpq_grad_adam  one thread per parameter: the gradient as a sum over the batch in item order (no atomics: bit-reproducible), then torch's Adam
//                     (srlx_adam_math.h) in the same thread; block 0 reduces the loss.
//
// NoisyLinear layers (srl/rl/torch_/modules/noisy_linear.py:8-52; rainbow.Config(enable_noisy_dense=True)) on a dueling handle, srlx_mlpq_bind_noisy: the
// bound tensors are the mu tensors, and ONE launch per call (k_mlpq_noisy_eff) writes mu + sigma * eps of every noisy tensor into the handle's effective
// tensors, which dense / narrow_rows / the backward chain read like plain weights -- srlx_noisy.hip:1-16's argument: inside dense() every workgroup would
// regenerate every normal of the layer, on the VALU that the multiply-adds need.  eps(seed, draw, tensor, element) is a pure function (srlx_noise_math.h), the
// draw ids come from a device-resident counter (srlx.h: the draw-id contract), and k_mlpq_grad_adam_noisy regenerates the s_0 pass's eps for d loss / d sigma.
//   k_mlpq_noisy_eff        up to three draws in one launch (the learner: the online handle's s_1..s_n and s_0 draws and the target's)
//   k_mlpq_learn_nstep_noisy<n>  k_mlpq_learn_nstep<n> with the online pass split: rows of s_0 under one draw, rows of s_1..s_n under the other
//   k_mlpq_grad_adam_noisy  k_mlpq_grad_adam; for a noisy tensor the thread also writes g_sigma = g * eps and takes sigma's Adam step
//
// The categorical head (C51; srl/algorithms/c51/c51.py:23-42, :70-142) on a srlx_mlpq_create_categorical handle: a plain network whose out_layer has A * N rows,
// row a * N + j = atom j of action a on the support linspace(v_min, v_max, N); the arithmetic is srlx_c51_math.h's, shared with the plugin trainer's kernel.
//   k_mlpq_actor_c51  k_mlpq_actor with one thread per (row, action) turning the logit rows into expectations before the same selection
//   k_mlpq_learn_c51  8 items per workgroup: ONE online pass over s_0 and s_1 (no target network), the item arithmetic on the logit rows in LDS, then
//                     k_mlpq_learn_rows's backward chain seeded through the N out_layer rows of a_0; k_mlpq_grad_adam follows unchanged
//   k_c51_loss        the same item arithmetic on logits torch produced (srlx_c51_loss), one workgroup walking the batch
#include "srlx_adam_math.h"
#include "srlx_c51_math.h"
#include "srlx_common.h"
#include "srlx_mlp_rows.h"
#include "srlx_noise_math.h"
#include "srlx_ppo_math.h"
#include "srlx_td_math.h"
#include <cmath>

struct srlx_mlpq {
    int D, L, A, device;  // L: the Linear + ReLU layers in front of the head (plain: 1..3, then out_layer; dueling: the trunk, 0..2)
    int W[3];
    int H, head;  // dueling: units of each branch; head 0 = out_layer, 1 = dueling "average", 2 = dueling "", 3 = categorical (out_layer with A * atoms rows)
    int atoms;    // categorical: atoms per action, on the support v_min..v_max
    double v_min, v_max;
    int max_nstep;
    int64_t max_rows, max_batch;
    float *p[12];  // layer 0 weight, bias, ..., then out_layer weight, bias -- or v_layers.0, v_layers.2, adv_layers.0, adv_layers.2 (weight, bias each)
    bool bound;
    float *grads[12];
    float *m[12], *v[12];
    double lr, beta1, beta2, eps;
    bool adam;
    // learner scratch (max_batch > 0)
    float *x0, *h, *dh, *q_on_next, *q_tg_next, *grad_q, *grad_v;
    double *loss_rows;
    int wmax;
    void *d_net;  // the descriptor of the bound parameters in device memory (the learner step's launch reads it)
    // NoisyLinear (srlx_mlpq_bind_noisy): p[] are the mu tensors; sig[i] != NULL marks a noisy tensor.  eff[0]: the effective tensors of srlx_mlpq_forward, of
    // the learner's s_1..s_n pass and of a target handle's pass; eff[1] (training handles): those of the learner's s_0 pass.  d_net describes set 0, d_net0 set 1.
    bool noisy, noisy_adam;
    float *sig[12], *gsig[12], *msig[12], *vsig[12];
    float *eff[2][12];
    unsigned long long noisy_seed;
    int64_t *d_draw;  // [0] the id the next pass will use, [1] the id set 0 holds, [2] the id set 1 holds
    void *d_net0;
};

namespace {

using i64 = int64_t;
using u64 = unsigned long long;
using u8 = unsigned char;

using srlxm::kRows;  // rows of one acting workgroup, and of the learner's online pass (s_0 and s_1 of kItems items)
using srlxm::kThreads;
using srlxm::kWTile;
constexpr int kItems = kRows / 2;
constexpr int kMaxParams = 12;  // two trunk layers and the dueling head's four
constexpr int kMaxNstep = 7;    // kRows / (n + 1) >= 2 items per workgroup

struct Net : srlxm::Layers {  // In = D; Out = A, or A * atoms on a categorical handle; L = the layers in front of the head
    const float *wout;  // out_layer's weight (= the weight of layer L)
    // the dueling head (head != 0; srl/rl/torch_/blocks/dueling_network.py:8-59) behind the L trunk layers: v_layers.0 [H][in], v_layers.2 [1][H],
    // adv_layers.0 [H][in], adv_layers.2 [A][H]; head 1 = "average", 2 = ""
    int H, head;
    const float *vw0, *vb0, *vw1, *vb1, *aw0, *ab0, *aw1, *ab1;
};

bool dueling(const srlx_mlpq *h) { return h->head == 1 || h->head == 2; }
bool categorical(const srlx_mlpq *h) { return h->head == 3; }
int out_cols(const srlx_mlpq *h) { return categorical(h) ? h->A * h->atoms : h->A; }  // rows of out_layer / of adv_layers.2

// the tensors a pass reads: the bound ones, or for a noisy tensor the effective one of `set`
const float *read_ptr(const srlx_mlpq *h, int i, int set) { return h->sig[i] ? h->eff[set][i] : h->p[i]; }

Net net_of(const srlx_mlpq *h, int set = 0) {
    Net n;
    n.In = h->D, n.L = h->L, n.Out = out_cols(h);  // (a categorical handle's network is a plain one whose out_layer has A * atoms rows)
    n.W0 = h->W[0], n.W1 = h->L > 1 ? h->W[1] : 0, n.W2 = h->L > 2 ? h->W[2] : 0;
    const float *w[4] = {nullptr, nullptr, nullptr, nullptr}, *b[4] = {nullptr, nullptr, nullptr, nullptr};
    const int plain_layers = dueling(h) ? h->L : h->L + 1;
    for (int l = 0; l < plain_layers; l++) w[l] = read_ptr(h, 2 * l, set), b[l] = read_ptr(h, 2 * l + 1, set);
    n.w0 = w[0], n.w1 = w[1], n.w2 = w[2], n.w3 = w[3], n.b0 = b[0], n.b1 = b[1], n.b2 = b[2], n.b3 = b[3];
    n.wout = dueling(h) ? nullptr : w[h->L];
    n.H = h->H, n.head = dueling(h) ? h->head : 0;
    const float *q[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (dueling(h))
        for (int k = 0; k < 8; k++) q[k] = read_ptr(h, 2 * h->L + k, set);
    n.vw0 = q[0], n.vb0 = q[1], n.vw1 = q[2], n.vb1 = q[3], n.aw0 = q[4], n.ab0 = q[5], n.aw1 = q[6], n.ab1 = q[7];
    return n;
}

int n_params(const srlx_mlpq *h) { return dueling(h) ? 2 * h->L + 8 : 2 * (h->L + 1); }

int lds_stride(const srlx_mlpq *h) { return h->wmax + 1; }  // (odd: rows of different row groups fall on different banks)

// The head's second layers (v_layers.2: 1 output, adv_layers.2: A <= 32 outputs, H inputs each): y[r][u] = sum_k W[u][k] x[r][k] + b[u] with 16 lanes per
// row (kThreads = 16 * kRows) -- every lane a strided partial sum, then a butterfly over the 16.  dense() would leave all but `rows` threads idle on a chain
// of H dependent multiply-adds per output.  The weight is read from memory as it is ([out][in] rows, 16 consecutive floats per row group).  No barrier inside.
__device__ __forceinline__ void narrow_rows(const float *__restrict__ Wt, const float *__restrict__ bias, int In, int Out, int rows, const float *x, int sx, float *y,
                                            int sy) {
    const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
    for (int u = 0; u < Out; u++) {
        float acc = 0.f;
        if (r < rows)
            for (int k = j; k < In; k += 16) acc = __builtin_fmaf(Wt[u * In + k], x[r * sx + k], acc);
        for (int d = 8; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 16);
        if (j == 0 && r < rows) y[r * sy + u] = acc + bias[u];
    }
}

// the whole network over the rows in buf0 (inputs, D columns); returns the buffer that holds the Q rows, behind a barrier: srlx_mlp_rows.h's plain-layer loop
// (a plain net: all L + 1 layers; a dueling one: the L trunk layers), then the dueling head.  `keep`: the kept planes of the hidden layers, NULL: not kept.
// OWN: the plain-layer loop written out here, a kept copy for the learner kernels that run two networks (k_mlpq_learn_rows, learn_nstep_body).  They sit at the
// SGPR limit, and behind the shared loop the compiler placed their scalar spills differently (k_mlpq_learn_nstep<3>: 150 reloads against 113), which cost
// the Rainbow and DQN updates 0.4 to 0.7 %; with the loop in this function their instructions are, up to register numbers, within three of
// what they were before the header.  Same layers, same dense(), same bits.
template <bool OWN = false>
__device__ __forceinline__ float *forward_rows(const Net &n, int rows, float *buf0, float *buf1, int S, float *wl, float *keep, i64 keep_plane, i64 keep_row0,
                                               int kept) {
    float *cur = buf0, *nxt = buf1;
    if constexpr (OWN) {
        const int plain_layers = n.head ? n.L : n.L + 1;
        for (int l = 0; l < plain_layers; l++) {
            const int In = n.in_of(l), Out = n.out_of(l);
            srlxm::dense<float>(n.weight(l), n.bias(l), In, Out, rows, cur, S, nxt, S, l < n.L, wl);
            __syncthreads();
            if (keep && l < n.L)
                for (int p = threadIdx.x; p < kept * Out; p += kThreads) keep[l * keep_plane + (keep_row0 + p / Out) * Out + p % Out] = nxt[(p / Out) * S + p % Out];
            float *tmp = cur;
            cur = nxt, nxt = tmp;
        }
    } else {
        cur = srlxm::forward_rows<float>(n, n.head ? n.L : n.L + 1, rows, buf0, buf1, S, wl, keep, keep_plane, keep_row0, kept);
        nxt = cur == buf0 ? buf1 : buf0;
    }
    if (!n.head) return cur;
    // the dueling head on the trunk's output rows in `cur` (the observation rows when there is no trunk).  Both branches' hidden rows go through `nxt`, one after
    // the other: the value branch's row is reduced to its scalar before the advantage branch overwrites it, so the row stride stays max width + 1.  Kept planes:
    // L = the value branch's hidden rows, L + 1 = the advantage branch's.
    __shared__ float vrow[kRows], mrow[kRows];
    const int t = threadIdx.x, In = n.in_of(n.L), H = n.H, A = n.Out;
    srlxm::dense<float>(n.vw0, n.vb0, In, H, rows, cur, S, nxt, S, true, wl);
    __syncthreads();
    if (keep)
        for (int p = t; p < kept * H; p += kThreads) keep[n.L * keep_plane + (keep_row0 + p / H) * H + p % H] = nxt[(p / H) * S + p % H];
    narrow_rows(n.vw1, n.vb1, H, 1, rows, nxt, S, vrow, 1);
    srlxm::dense<float>(n.aw0, n.ab0, In, H, rows, cur, S, nxt, S, true, wl);  // (its first barrier is behind every read of the value rows above)
    __syncthreads();
    if (keep)
        for (int p = t; p < kept * H; p += kThreads) keep[(n.L + 1) * keep_plane + (keep_row0 + p / H) * H + p % H] = nxt[(p / H) * S + p % H];
    narrow_rows(n.aw1, n.ab1, H, A, rows, nxt, S, cur, S);  // (the barrier above is behind every read of the trunk rows in `cur`)
    __syncthreads();
    if (t < rows) {  // torch.mean(adv, dim=-1)
        float s = 0.f;
        for (int a = 0; a < A; a++) s += cur[t * S + a];
        mrow[t] = n.head == 1 ? s / (float)A : 0.f;
    }
    __syncthreads();
    for (int p = t; p < rows * A; p += kThreads) {  // v + adv - mean (dueling_network.py:51); "": v + adv
        const int r = p / A, a = p % A;
        const float q = vrow[r] + cur[r * S + a];
        cur[r * S + a] = n.head == 1 ? q - mrow[r] : q;
    }
    __syncthreads();
    return cur;
}

struct Policy {
    u64 seed;
    const i64 *counter;
    const float *eps;
    int32_t *actions;
};

// k_head's selection (srlx_qnet.hip: fused_policy; rainbow.py:301-329): u53(rng_u64(seed, counter, 2 m)) < eps[m] -> the uniform draw
// u53(rng_u64(seed, counter, 2 m + 1)) picks one of the A actions, else the first maximum of the row (np.argmax).  The counter is only read here.
__device__ __forceinline__ int select_action(const Policy &pol, i64 m, int A, const float *q) {
    const u64 c = (u64)pol.counter[0];
    int act = 0;
    if (srlx::u53(srlx::rng_u64(pol.seed, c, (u64)(2 * m))) < (double)pol.eps[m]) {
        int pick = (int)(srlx::u53(srlx::rng_u64(pol.seed, c, (u64)(2 * m + 1))) * (double)A);
        if (pick >= A) pick = A - 1;
        act = pick;
    } else {
        float bv = -INFINITY;
        bool have = false;
        for (int a = 0; a < A; a++)
            if (!have || q[a] > bv) act = a, bv = q[a], have = true;
    }
    return act;
}

__device__ __forceinline__ const float *row_ptr(const float *base, const i64 *off, i64 row, int D) { return off ? base + off[row] : base + row * D; }

// the categorical head's shape behind a Net whose out_layer has A * N rows
struct Cat {
    int A, N;
    double v_min, v_max;
};

// CAT: the rows forward_rows returns are logits [A][N]; one thread per (row, action) turns them into the expectations E[Z] (srlx_c51_math.h; c51.py:165-168),
// which go where the Q rows go and into select_action unchanged.
template <bool CAT>
__device__ __forceinline__ void actor_body(const Net &n, i64 rows_total, const float *__restrict__ obs, const i64 *__restrict__ off, int S, float *__restrict__ q,
                                           const Policy &pol, i64 *draw, const Cat &cat) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    const int t = threadIdx.x;
    const i64 r0 = (i64)blockIdx.x * kRows;
    const int rows = (int)(rows_total - r0 < kRows ? rows_total - r0 : kRows);
    if (draw && blockIdx.x == 0 && t == 0) draw[0] += 1;  // NoisyLinear: this pass's draw is spent (every reader of draw[0] ran in the launch before)
    for (int p = t; p < rows * n.In; p += kThreads) {
        const int r = p / n.In, k = p % n.In;
        b0[r * S + k] = row_ptr(obs, off, r0 + r, n.In)[k];
    }
    __syncthreads();
    const float *qs = forward_rows(n, rows, b0, b1, S, wl, nullptr, 0, 0, 0);
    if constexpr (CAT) {
        __shared__ float qe[kRows * srlxc::kMaxActions];
        const int A = cat.A;
        for (int p = t; p < rows * A; p += kThreads) {
            const int r = p / A, c = p % A;
            const float e = srlxc::expectation(qs + r * S + c * cat.N, cat.N, cat.v_min, cat.v_max);
            qe[r * srlxc::kMaxActions + c] = e;
            if (q) q[(r0 + r) * A + c] = e;
        }
        __syncthreads();
        if (pol.actions && t < rows) pol.actions[r0 + t] = select_action(pol, r0 + t, A, qe + t * srlxc::kMaxActions);
    } else {
        if (q)
            for (int p = t; p < rows * n.Out; p += kThreads) q[(r0 + p / n.Out) * n.Out + p % n.Out] = qs[(p / n.Out) * S + p % n.Out];
        if (pol.actions && t < rows) pol.actions[r0 + t] = select_action(pol, r0 + t, n.Out, qs + t * S);
    }
}

__global__ void __launch_bounds__(kThreads) k_mlpq_actor(Net n, i64 rows_total, const float *__restrict__ obs, const i64 *__restrict__ off, int S, float *__restrict__ q,
                                                         Policy pol, i64 *draw) {
    actor_body<false>(n, rows_total, obs, off, S, q, pol, draw, Cat{});
}

__global__ void __launch_bounds__(kThreads) k_mlpq_actor_c51(Net n, i64 rows_total, const float *__restrict__ obs, const i64 *__restrict__ off, int S,
                                                             float *__restrict__ q, Policy pol, Cat cat) {
    actor_body<true>(n, rows_total, obs, off, S, q, pol, nullptr, cat);
}

// srl/rl/functions.py:10-17 in float64 (one evaluation per item)
__device__ __forceinline__ double rescaling64(double x) {
    const double s = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    return s * (sqrt(fabs(x) + 1.0) - 1.0) + 0.001 * x;
}
__device__ __forceinline__ double inverse_rescaling64(double x) {
    const double s = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    const double n = (sqrt(1.0 + 4.0 * 0.001 * (fabs(x) + 1.0 + 0.001)) - 1.0) / (2.0 * 0.001);
    return s * (n * n - 1.0);
}

// srlx_td_math.h:td_rows at n = 1, written out (its per-step arrays, indexed by the run-time n, would live in scratch memory): dqn.py:144-176 -- the retrace sum
// is the single term float32(gain * float32(discount ** 0)) * 1.0 = gain -- and model_torch.py:89-131.  With `rescale` the two value transforms run in float64.
// Returns the item's Huber term (float64).
__device__ __forceinline__ double td_one(const srlx::TdArgs &a, i64 b) {
    const int A = a.A;
    const float *qon = a.q_on_next + b * A, *qtg = a.q_tg_next + b * A;
    const int nact = srlx::argmax_masked(a.double_dqn ? qon : qtg, nullptr, A);
    const float maxq = qtg[nact];
    float gain;
    if (a.rescale) {
        // (float64: in float32, sqrt(1 + 0.004 (|x| + 1.001)) - 1 of the inverse cancels to ~3e-5 relative, 5e-5 absolute on the target at |Q| ~ 1)
        const double inv = inverse_rescaling64((double)maxq);
        gain = (float)rescaling64((double)a.rewards[b] + ((1.0 - (double)a.terminated[b]) * a.discount) * inv);
    } else {
        gain = a.rewards[b] + ((1.0f - a.terminated[b]) * (float)a.discount) * maxq;
    }
    const float target = gain;
    a.target[b] = target;
    const int a0 = a.actions[b];
    const float q0 = a.q_on_0[b * A + a0];
    const float w = a.weights[b];
    const float tw = target * w, qw = q0 * w;
    const float diff = tw - qw;
    const float z = fabsf(diff);
    const double huber = (z < 1.0f) ? 0.5 * (double)z * (double)z : (double)z - 0.5;
    const float dclamp = diff > 1.0f ? 1.0f : (diff < -1.0f ? -1.0f : diff);
    const float gsel = -(w * dclamp) / (float)a.B;
    for (int k = 0; k < A; k++) a.grad_q0[b * A + k] = k == a0 ? gsel : 0.f;
    a.priorities[b] = fabsf(target - q0);
    return huber;
}

struct Learn {
    i64 B;
    const float *obs;
    const i64 *off;  // [B][2]: element offsets of s_0 and s_1 (srlx_per_sample_gather_train's frame_off_all with window 1, n_step 1)
    float *x0, *h, *dh, *q0, *grad_q;
    double *loss_rows;
    int hstride;  // floats between the per-layer planes of h / dh (max_batch * wmax)
    srlx::TdArgs td;
};

__global__ void __launch_bounds__(kThreads) k_mlpq_learn_rows(const Net *__restrict__ onp, const Net *__restrict__ tgp, Learn a, int S) {
    // (the two networks' descriptors are read from memory: as kernel arguments, held in scalar registers through both passes, they spilled to scratch)
    const Net &on = *onp, &tg = *tgp;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *d0 = sm + 2 * kRows * S, *d1 = d0 + kItems * S, *wl = d1 + kItems * S;
    __shared__ float gsel[kItems];
    __shared__ int act0[kItems];
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * kItems;
    const int nb = (int)(a.B - i0 < kItems ? a.B - i0 : kItems);
    const int D = on.In, A = on.Out, L = on.L;
    // rows 0..kItems-1: s_0 of the items, kItems..: s_1 (missing items: zero rows, never stored)
    for (int p = t; p < kRows * D; p += kThreads) {
        const int r = p / D, k = p % D, it = r % kItems, which = r / kItems;
        const float x = it < nb ? a.obs[a.off[(i0 + it) * 2 + which] + k] : 0.f;
        b0[r * S + k] = x;
        if (which == 0 && it < nb) a.x0[(i0 + it) * D + k] = x;
    }
    __syncthreads();
    const float *qs = forward_rows<true>(on, kRows, b0, b1, S, wl, a.h, a.hstride, i0, nb);  // (the kept planes are [B][W_l] dense)
    for (int p = t; p < nb * A; p += kThreads) {
        const int r = p / A, c = p % A;
        a.q0[(i0 + r) * A + c] = qs[r * S + c];
        const_cast<float *>(a.td.q_on_next)[(i0 + r) * A + c] = qs[(kItems + r) * S + c];
    }
    __syncthreads();
    // target pass over s_1
    for (int p = t; p < kItems * D; p += kThreads) {
        const int r = p / D, k = p % D;
        b0[r * S + k] = r < nb ? a.obs[a.off[(i0 + r) * 2 + 1] + k] : 0.f;
    }
    __syncthreads();
    const float *qt = forward_rows<true>(tg, kItems, b0, b1, S, wl, nullptr, 0, 0, 0);
    for (int p = t; p < nb * A; p += kThreads) const_cast<float *>(a.td.q_tg_next)[(i0 + p / A) * A + p % A] = qt[(p / A) * S + p % A];
    __threadfence_block();
    __syncthreads();
    // dqn.py:144-176 + model_torch.py:89-131 for these items (td_rows with n = 1: target, Huber term, d loss / d q, priority)
    if (t < nb) {
        const i64 b = i0 + t;
        a.loss_rows[b] = td_one(a.td, b);
        act0[t] = a.td.actions[b];
        gsel[t] = a.td.grad_q0[b * A + act0[t]];
    }
    __syncthreads();
    // the backward chain, row by row: d h_{L-1} from the Q seed (one non-zero column of out_layer's weight per row), then through every hidden layer's weight
    srlxm::backward_rows<float>(on, L - 1, nb, i0, d0, d1, S, a.h, a.dh, a.hstride, [&](int r, int k, int Wl) { return gsel[r] * on.wout[act0[r] * Wl + k]; });
}


// ---- the n-step learner step (Rainbow on flat observations) -------------------------------------------------------------------------------------------------
struct LearnN {
    i64 B;
    const float *obs;
    const i64 *off;  // [B][n + 1]: element offsets of s_0..s_n (the store's frame_off_all at window 1)
    const int32_t *actions;              // [B][n]
    const float *rewards, *terminated;   // [B][n]
    const float *weights;                // [B]
    float *x0, *h, *dh, *q0, *grad_q, *grad_v;
    double *loss_rows;
    int hstride;
    float *target, *priorities;
    double discount, retrace_h;
    int double_dqn, rescale;
    float dm[kMaxNstep];  // float32(discount ** m), filled on the host (srlx_td_math.h: multi_discounts)
};

// srlx_td_math.h:td_rows for one item with the step count a compile-time bound (its per-step values stay in registers): rainbow.py:226-287 and
// model_torch.py:103-113 in numpy's float32 order.  qon: the online Q rows of s_1.. (step stride qstep floats), qtg: the target's.  With `rescale` the two value
// transforms run in float64, like td_one.  Returns the Huber term; gsel = d loss / d q[a_0].
template <int NS>
__device__ __forceinline__ double td_item(const LearnN &a, i64 b, int A, const float *qon, const float *qtg, int qstep, const float *q0row, float &gsel, int &a0_out) {
    double c = 1.0;
    float target = 0.f;
#pragma unroll
    for (int m = 0; m < NS; m++) {
        const float *qo = qon + m * qstep, *qt = qtg + m * qstep;
        const int na = srlx::argmax_masked(a.double_dqn ? qo : qt, nullptr, A);  // :245-253
        const float maxq = qt[na];
        const float r = a.rewards[b * NS + m], term = a.terminated[b * NS + m];
        float gain;
        if (a.rescale)
            gain = (float)rescaling64((double)r + ((1.0 - (double)term) * a.discount) * inverse_rescaling64((double)maxq));
        else
            gain = r + ((1.0f - term) * (float)a.discount) * maxq;  // :258
        const int am = a.actions[b * NS + m];
        const float qsel = m == 0 ? 0.f : (qon + (m - 1) * qstep)[am];  // :231-233
        const float td = gain - qsel;
        if (m > 0) c *= a.retrace_h * (am == na ? 1.0 : 0.0);  // :267-280
        target = target + (float)((double)(td * a.dm[m]) * c);  // :285
    }
    a.target[b] = target;
    const int a0 = a.actions[b * NS];
    const float q0 = q0row[a0];
    const float w = a.weights[b];
    const float tw = target * w, qw = q0 * w;
    const float diff = tw - qw;
    const float z = fabsf(diff);
    const double huber = (z < 1.0f) ? 0.5 * (double)z * (double)z : (double)z - 0.5;
    const float dclamp = diff > 1.0f ? 1.0f : (diff < -1.0f ? -1.0f : diff);
    gsel = -(w * dclamp) / (float)a.B;
    a0_out = a0;
    a.priorities[b] = fabsf(target - q0);
    return huber;
}

// kRows / (NS + 1) items per workgroup, rows step-major (row s * P + item): the online pass over s_0..s_n, the target pass over s_1..s_n, td_item, then the
// row-local backward chain -- through out_layer as in k_mlpq_learn_rows, or through the dueling head's two branches into the trunk.  At NS = 1 on a plain net the
// row layout, every sum and every store are k_mlpq_learn_rows's.
//
// NZ (NoisyLinear handles): `on` describes the effective tensors of the s_0 draw, `on_next` those of the s_1..s_n draw, and the online pass runs as two calls
// of forward_rows -- rows 0..P-1 under `on` with their kept planes, rows P.. under `on_next`.  dense() and narrow_rows() give a row the same sums whichever
// rows share the call, so with every sigma 0 the results are the plain kernel's bits.  The backward chain reads `on`.
template <int NS, bool NZ>
__device__ __forceinline__ void learn_nstep_body(const Net &on, const Net &on_next, const Net &tg, const LearnN &a, int S) {
    constexpr int P = kRows / (NS + 1), R = P * (NS + 1);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *d0 = sm + 2 * kRows * S, *d1 = d0 + kItems * S, *wl = d1 + kItems * S;
    __shared__ float qon_s[kRows * 32], qtg_s[kRows * 32];  // Q rows of s_1..s_n: row (s - 1) * P + item, A floats each
    __shared__ float gsel[kItems];
    __shared__ int act0[kItems];
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * P;
    const int nb = (int)(a.B - i0 < P ? a.B - i0 : P);
    const int D = on.In, A = on.Out, L = on.L;
    for (int p = t; p < R * D; p += kThreads) {  // (missing items: zero rows, never stored)
        const int r = p / D, k = p % D, it = r % P, st = r / P;
        const float x = it < nb ? a.obs[a.off[(i0 + it) * (NS + 1) + st] + k] : 0.f;
        b0[r * S + k] = x;
        if (st == 0 && it < nb) a.x0[(i0 + it) * D + k] = x;
    }
    __syncthreads();
    if constexpr (NZ) {
        // (forward_rows writes rows < `rows` of either buffer only: the s_1..s_n inputs in rows P.. of b0 outlive the s_0 pass)
        const float *qs = forward_rows<true>(on, P, b0, b1, S, wl, a.h, a.hstride, i0, nb);
        for (int p = t; p < nb * A; p += kThreads) a.q0[(i0 + p / A) * A + p % A] = qs[(p / A) * S + p % A];
        __syncthreads();
        const float *qn = forward_rows<true>(on_next, NS * P, b0 + P * S, b1 + P * S, S, wl, nullptr, 0, 0, 0);
        for (int p = t; p < NS * P * A; p += kThreads) qon_s[p] = qn[(p / A) * S + p % A];
    } else {
        const float *qs = forward_rows<true>(on, R, b0, b1, S, wl, a.h, a.hstride, i0, nb);
        for (int p = t; p < nb * A; p += kThreads) a.q0[(i0 + p / A) * A + p % A] = qs[(p / A) * S + p % A];
        for (int p = t; p < NS * P * A; p += kThreads) qon_s[p] = qs[(P + p / A) * S + p % A];
    }
    __syncthreads();
    for (int p = t; p < NS * P * D; p += kThreads) {
        const int r = p / D, k = p % D, it = r % P, st = r / P + 1;
        b0[r * S + k] = it < nb ? a.obs[a.off[(i0 + it) * (NS + 1) + st] + k] : 0.f;
    }
    __syncthreads();
    const float *qt = forward_rows<true>(tg, NS * P, b0, b1, S, wl, nullptr, 0, 0, 0);
    for (int p = t; p < NS * P * A; p += kThreads) qtg_s[p] = qt[(p / A) * S + p % A];
    __threadfence_block();  // (q0 rows are read back from memory below)
    __syncthreads();
    if (t < nb) {
        const i64 b = i0 + t;
        float g;
        int a0;
        a.loss_rows[b] = td_item<NS>(a, b, A, qon_s + t * A, qtg_s + t * A, P * A, a.q0 + b * A, g, a0);
        gsel[t] = g, act0[t] = a0;
        if (!on.head)
            for (int k = 0; k < A; k++) a.grad_q[b * A + k] = k == a0 ? g : 0.f;
    }
    __syncthreads();
    if (!on.head) {
        // the backward chain as in k_mlpq_learn_rows: the Q seed has one non-zero column per row
        srlxm::backward_rows<float>(on, on.L - 1, nb, i0, d0, d1, S, a.h, a.dh, a.hstride, [&](int r, int k, int Wl) { return gsel[r] * on.wout[act0[r] * Wl + k]; });
        return;
    }
    // the dueling head: d adv_k = g ((k == a_0) - 1/A) ("": g (k == a_0)), d v = g; through adv_layers.2 / v_layers.2 into the two hidden rows (d0: value branch,
    // d1: advantage branch), then through both first layers into the trunk's last output, and down the trunk
    const int H = on.H;
    const float sub = on.head == 1 ? 1.0f / (float)A : 0.f;
    for (int p = t; p < nb * A; p += kThreads) {
        const int r = p / A, k = p % A;
        a.grad_q[(i0 + r) * A + k] = gsel[r] * ((k == act0[r] ? 1.0f : 0.f) - sub);
    }
    if (t < nb) a.grad_v[i0 + t] = gsel[t];
    {
        const float *hv = a.h + (i64)L * a.hstride, *ha = a.h + (i64)(L + 1) * a.hstride;
        float *dhv = a.dh + (i64)L * a.hstride, *dha = a.dh + (i64)(L + 1) * a.hstride;
        for (int p = t; p < nb * H; p += kThreads) {
            const int r = p / H, k = p % H;
            const float g = gsel[r];
            const int a0 = act0[r];
            float gv = g * on.vw1[k];
            gv = hv[(i0 + r) * H + k] > 0.f ? gv : 0.f;
            float ga = 0.f;
            for (int c = 0; c < A; c++) ga = __builtin_fmaf(g * ((c == a0 ? 1.0f : 0.f) - sub), on.aw1[c * H + k], ga);
            ga = ha[(i0 + r) * H + k] > 0.f ? ga : 0.f;
            d0[r * S + k] = gv, dhv[(i0 + r) * H + k] = gv;
            d1[r * S + k] = ga, dha[(i0 + r) * H + k] = ga;
        }
    }
    __syncthreads();
    if (L > 0) {
        const int Wl = on.width(L - 1);
        const float *hl = a.h + (i64)(L - 1) * a.hstride;
        float *dhl = a.dh + (i64)(L - 1) * a.hstride;
        for (int p = t; p < nb * Wl; p += kThreads) {
            const int r = p / Wl, k = p % Wl;
            float g = 0.f;
#pragma unroll 8
            for (int u = 0; u < H; u++) g = __builtin_fmaf(d0[r * S + u], on.vw0[(i64)u * Wl + k], g);
#pragma unroll 8
            for (int u = 0; u < H; u++) g = __builtin_fmaf(d1[r * S + u], on.aw0[(i64)u * Wl + k], g);
            g = hl[(i0 + r) * Wl + k] > 0.f ? g : 0.f;
            b0[r * S + k] = g;
            dhl[(i0 + r) * Wl + k] = g;
        }
        __syncthreads();
    }
    if (L > 1) {
        const int W0 = on.W0, W1 = on.W1;
        for (int p = t; p < nb * W0; p += kThreads) {
            const int r = p / W0, k = p % W0;
            float g = 0.f;
#pragma unroll 8
            for (int u = 0; u < W1; u++) g = __builtin_fmaf(b0[r * S + u], on.w1[(i64)u * W0 + k], g);
            a.dh[(i0 + r) * W0 + k] = a.h[(i0 + r) * W0 + k] > 0.f ? g : 0.f;
        }
    }
}

template <int NS>
__global__ void __launch_bounds__(kThreads) k_mlpq_learn_nstep(const Net *__restrict__ onp, const Net *__restrict__ tgp, LearnN a, int S) {
    learn_nstep_body<NS, false>(*onp, *onp, *tgp, a, S);
}

// draw_on / draw_tg: the two handles' draw counters.  k_mlpq_noisy_eff, the launch before this one, was their last reader: the three ids are spent here.
template <int NS>
__global__ void __launch_bounds__(kThreads) k_mlpq_learn_nstep_noisy(const Net *__restrict__ on0p, const Net *__restrict__ onp, const Net *__restrict__ tgp, LearnN a,
                                                                     int S, i64 *draw_on, i64 *draw_tg) {
    if (blockIdx.x == 0 && threadIdx.x == 0) draw_on[0] += 2, draw_tg[0] += 1;
    learn_nstep_body<NS, true>(*on0p, *onp, *tgp, a, S);
}

const void *learn_nstep_noisy_fn(int n) {
    switch (n) {
    case 1: return (const void *)k_mlpq_learn_nstep_noisy<1>;
    case 2: return (const void *)k_mlpq_learn_nstep_noisy<2>;
    case 3: return (const void *)k_mlpq_learn_nstep_noisy<3>;
    case 4: return (const void *)k_mlpq_learn_nstep_noisy<4>;
    case 5: return (const void *)k_mlpq_learn_nstep_noisy<5>;
    case 6: return (const void *)k_mlpq_learn_nstep_noisy<6>;
    default: return (const void *)k_mlpq_learn_nstep_noisy<7>;
    }
}

const void *learn_nstep_fn(int n) {
    switch (n) {
    case 1: return (const void *)k_mlpq_learn_nstep<1>;
    case 2: return (const void *)k_mlpq_learn_nstep<2>;
    case 3: return (const void *)k_mlpq_learn_nstep<3>;
    case 4: return (const void *)k_mlpq_learn_nstep<4>;
    case 5: return (const void *)k_mlpq_learn_nstep<5>;
    case 6: return (const void *)k_mlpq_learn_nstep<6>;
    default: return (const void *)k_mlpq_learn_nstep<7>;
    }
}

// ---- the categorical learner step (C51 on flat observations) ------------------------------------------------------------------------------------------------
struct LearnC {
    const float *obs;
    const i64 *off;  // [B][2]: element offsets of s_0 and s_1
    float *x0, *h, *dh;
    double *loss_rows;
    int hstride;
    srlxc::Items it;
};

// c51.py:70-142 for kItems sampled items per workgroup: ONE online pass over s_0 (rows 0..kItems-1, kept planes) and s_1 (rows kItems..) -- there is no target
// network (:91) -- then srlx_c51_math.h:items_step on the logit rows where they lie in LDS, then k_mlpq_learn_rows's row-local backward chain, seeded through
// the N rows of out_layer that belong to a_0.  The item arrays (next distribution, p_0 / seeds, m) take the weight tile's place: after the pass it is free.
__global__ void __launch_bounds__(kThreads) k_mlpq_learn_c51(const Net *__restrict__ onp, LearnC a, int S) {
    const Net &on = *onp;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *d0 = sm + 2 * kRows * S, *d1 = d0 + kItems * S, *wl = d1 + kItems * S;
    static_assert(3 * kItems * srlxc::kMaxAtoms <= kWTile, "the item arrays live in the weight tile");
    float *pn = wl, *seed = wl + kItems * srlxc::kMaxAtoms, *ms = wl + 2 * kItems * srlxc::kMaxAtoms;
    __shared__ int act0[kItems];
    __shared__ double row_loss[kItems];
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * kItems;
    const int nb = (int)(a.it.B - i0 < kItems ? a.it.B - i0 : kItems);
    const int D = on.In, N = a.it.N;
    for (int p = t; p < kRows * D; p += kThreads) {  // (missing items: zero rows, never stored)
        const int r = p / D, k = p % D, it = r % kItems, which = r / kItems;
        const float x = it < nb ? a.obs[a.off[(i0 + it) * 2 + which] + k] : 0.f;
        b0[r * S + k] = x;
        if (which == 0 && it < nb) a.x0[(i0 + it) * D + k] = x;
    }
    __syncthreads();
    const float *lg = forward_rows(on, kRows, b0, b1, S, wl, a.h, a.hstride, i0, nb);  // (returns behind a barrier: every read of the weight tile is done)
    srlxc::items_step<kItems>(a.it, i0, nb, lg, lg + kItems * S, S, pn, seed, ms, act0, row_loss);
    if (t < nb) a.loss_rows[i0 + t] = row_loss[t];
    srlxm::backward_rows<float>(on, on.L - 1, nb, i0, d0, d1, S, a.h, a.dh, a.hstride, [&](int r, int k, int Wl) {
        const float *wa = on.wout + (i64)act0[r] * N * Wl + k, *sr = seed + r * srlxc::kMaxAtoms;
        float g = 0.f;
#pragma unroll 8
        for (int j = 0; j < N; j++) g = __builtin_fmaf(sr[j], wa[(i64)j * Wl], g);
        return g;
    });
}

// srlx_c51_loss: the same item arithmetic on logits torch produced, one workgroup walking the batch kItems items at a time; thread 0 reduces the row terms in
// item order as k_mlpq_grad_adam does.
__global__ void __launch_bounds__(kThreads) k_c51_loss(srlxc::Items a, const float *__restrict__ lg_next, const float *__restrict__ lg_0, float *__restrict__ loss) {
    __shared__ float pn[kItems * srlxc::kMaxAtoms], seed[kItems * srlxc::kMaxAtoms], ms[kItems * srlxc::kMaxAtoms];
    __shared__ int act0[kItems];
    __shared__ double row_loss[kItems];
    const i64 cols = (i64)a.A * a.N;
    double s = 0.0;
    for (i64 i0 = 0; i0 < a.B; i0 += kItems) {
        const int nb = (int)(a.B - i0 < kItems ? a.B - i0 : kItems);
        srlxc::items_step<kItems>(a, i0, nb, lg_0 + i0 * cols, lg_next + i0 * cols, cols, pn, seed, ms, act0, row_loss);
        if (threadIdx.x == 0)
            for (int r = 0; r < nb; r++) s += row_loss[r];
    }
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)a.B);
}

struct GradAdam {
    i64 B;
    int nseg;
    i64 seg_end[kMaxParams];  // running element counts of the parameter tensors
    int seg_out[kMaxParams], seg_in[kMaxParams];  // in = 0: a bias
    const float *dout[kMaxParams];  // [B][out]: d loss / d (layer output) rows
    const float *xin[kMaxParams];   // [B][in]: the layer's input rows
    float *p[kMaxParams], *g[kMaxParams], *m[kMaxParams], *v[kMaxParams];
    int adam;
    double lr, beta1, beta2, eps;
    const i64 *steps_taken;
    const double *loss_rows;
    float *loss;
};

// the sigma side of a noisy handle's update (NULL sig[s]: a plain tensor)
struct NoisyGrad {
    float *sig[kMaxParams], *g[kMaxParams], *m[kMaxParams], *v[kMaxParams];
    u64 seed;
    const i64 *draw;  // draw[2]: the id of the s_0 pass whose gradient this is
};

template <bool NZ>
__device__ __forceinline__ void grad_adam_body(const GradAdam &a, const NoisyGrad *z) {
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.loss) {
        double s = 0.0;
        for (i64 b = 0; b < a.B; b++) s += a.loss_rows[b];
        a.loss[0] = (float)(s / (double)a.B);
    }
    if (i >= a.seg_end[a.nseg - 1]) return;
    int s = 0;
    while (i >= a.seg_end[s]) s++;
    const i64 e = i - (s ? a.seg_end[s - 1] : 0);
    const int Out = a.seg_out[s], In = a.seg_in[s];
    float g = 0.f;
    if (In) {
        const int u = (int)(e / In), k = (int)(e % In);
        const float *dout = a.dout[s] + u, *xin = a.xin[s] + k;
#pragma unroll 8
        for (int b = 0; b < (int)a.B; b++) g = __builtin_fmaf(dout[(i64)b * Out], xin[(i64)b * In], g);
    } else {
        const float *dout = a.dout[s] + e;
#pragma unroll 8
        for (int b = 0; b < (int)a.B; b++) g += dout[(i64)b * Out];
    }
    if (a.g[s]) a.g[s][e] = g;
    if (a.adam) {
        const srlx::AdamCoef c = srlx::adam_coef(a.lr, a.beta1, a.beta2, a.eps, a.steps_taken[0]);
        float p = a.p[s][e], m = a.m[s][e], v = a.v[s][e];
        srlx::adam_one(p, g, m, v, c);
        a.p[s][e] = p, a.m[s][e] = m, a.v[s][e] = v;
    }
    if constexpr (NZ) {
        // noisy_linear.py:50-52: W = w_mu + w_sigma * eps, so d loss / d w_sigma = d loss / d W * eps of the pass the gradient belongs to
        if (!z->sig[s]) return;
        const float2 n2 = srlx::noisy_eps_pair(z->seed, (u64)z->draw[2], s, (u64)(e >> 1));
        const float gs = g * ((e & 1) ? n2.y : n2.x);
        if (z->g[s]) z->g[s][e] = gs;
        if (a.adam) {
            const srlx::AdamCoef c = srlx::adam_coef(a.lr, a.beta1, a.beta2, a.eps, a.steps_taken[0]);
            float p = z->sig[s][e], m = z->m[s][e], v = z->v[s][e];
            srlx::adam_one(p, gs, m, v, c);
            z->sig[s][e] = p, z->m[s][e] = m, z->v[s][e] = v;
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_mlpq_grad_adam(GradAdam a) { grad_adam_body<false>(a, nullptr); }

__global__ void __launch_bounds__(kThreads) k_mlpq_grad_adam_noisy(GradAdam a, NoisyGrad z) { grad_adam_body<true>(a, &z); }

// ---- NoisyLinear: the effective tensors of a draw -------------------------------------------------------------------------------------------------------------
struct EffJob {  // one draw of one handle
    const float *mu[kMaxParams], *sig[kMaxParams];  // sig NULL: a plain tensor (no elements in `begin`)
    float *out[kMaxParams];
    i64 *draw;  // the handle's counter block: the id is draw[0] + add, recorded in draw[rec]
    int add, rec;
    u64 seed;
};
struct EffArgs {
    EffJob job[3];  // blockIdx.y
    i64 begin[kMaxParams + 1];  // prefix sums of the noisy tensors' element PAIR counts (one Box-Muller evaluation yields elements 2 j, 2 j + 1)
    i64 n[kMaxParams];
};

__device__ __forceinline__ int find_segment(const i64 *begin, i64 j) {
    int t = 0;
#pragma unroll
    for (int k = 1; k < kMaxParams; k++) t += j >= begin[k] ? 1 : 0;
    return t;
}

// out = mu + sigma * eps(seed, id, tensor, element) for every noisy tensor of up to three draws.  The counters are only read here (the call's next launch
// advances them); block (0, y) records the id its job used.
__global__ void __launch_bounds__(kThreads) k_mlpq_noisy_eff(EffArgs s) {
    const EffJob &jb = s.job[blockIdx.y];
    const i64 id = jb.draw[0] + jb.add;
    if (blockIdx.x == 0 && threadIdx.x == 0) jb.draw[jb.rec] = id;
    const i64 total = s.begin[kMaxParams];
    for (i64 j = (i64)blockIdx.x * kThreads + threadIdx.x; j < total; j += (i64)gridDim.x * kThreads) {
        const int t = find_segment(s.begin, j);
        const i64 p = j - s.begin[t], e = 2 * p;
        const float2 z = srlx::noisy_eps_pair(jb.seed, (u64)id, t, (u64)p);
        jb.out[t][e] = jb.mu[t][e] + jb.sig[t][e] * z.x;
        if (e + 1 < s.n[t]) jb.out[t][e + 1] = jb.mu[t][e + 1] + jb.sig[t][e + 1] * z.y;
    }
}

// eps of one tensor under a given draw (tests: the noise of a step, known before it runs)
__global__ void __launch_bounds__(kThreads) k_mlpq_noisy_eps(u64 seed, i64 id, int t, i64 n, float *__restrict__ out) {
    const i64 pairs = (n + 1) / 2;
    for (i64 p = (i64)blockIdx.x * kThreads + threadIdx.x; p < pairs; p += (i64)gridDim.x * kThreads) {
        const float2 z = srlx::noisy_eps_pair(seed, (u64)id, t, (u64)p);
        out[2 * p] = z.x;
        if (2 * p + 1 < n) out[2 * p + 1] = z.y;
    }
}

__global__ void __launch_bounds__(kThreads) k_mlpq_copy(int nseg, GradAdam segs /* p = src, g = dst */) {
    const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (i >= segs.seg_end[nseg - 1]) return;
    int s = 0;
    while (i >= segs.seg_end[s]) s++;
    const i64 e = i - (s ? segs.seg_end[s - 1] : 0);
    segs.g[s][e] = segs.p[s][e];
}

// ---- CartPole (envs/cartpole.py:step) for E lanes, float64 state -------------------------------------------------------------------------------------------
// (the step and the reset are srlx_ppo_math.h's: one definition with the self-resetting step of the PPO path)
__global__ void __launch_bounds__(256) k_cartpole(i64 E, double *__restrict__ state, int32_t *__restrict__ steps, int32_t *__restrict__ episodes,
                                                  const u8 *__restrict__ needs_reset, const int32_t *__restrict__ actions, i64 max_steps, u64 seed,
                                                  float *__restrict__ obs, float *__restrict__ reward, u8 *__restrict__ terminated, u8 *__restrict__ done) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double s[4] = {state[4 * e], state[4 * e + 1], state[4 * e + 2], state[4 * e + 3]};
    int st = steps[e];
    if (!needs_reset || needs_reset[e]) {  // the lane's next episode: uniform in [-0.05, 0.05]^4 from (seed, lane, episode of the lane)
        int ep = episodes[e];
        srlxp::cartpole_reset(s, st, ep, seed, e);
        episodes[e] = ep;
        steps[e] = st;
        for (int k = 0; k < 4; k++) state[4 * e + k] = s[k], obs[4 * e + k] = (float)s[k];
        if (reward) reward[e] = 0.f, terminated[e] = 0, done[e] = 0;
        return;
    }
    bool term, trunc;
    srlxp::cartpole_dynamics(s, st, actions[e], max_steps, term, trunc);
    steps[e] = st;
    for (int k = 0; k < 4; k++) state[4 * e + k] = s[k], obs[4 * e + k] = (float)s[k];
    reward[e] = 1.f;
    terminated[e] = term ? 1 : 0;
    done[e] = (term || trunc) ? 1 : 0;
}

int set_lds(const void *fn, size_t bytes) {
    if (bytes > 65536) SRLX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return SRLX_OK;
}

// (Out, In) of the handle's n_params / 2 Linear layers in binding order
int layer_shapes(const srlx_mlpq *h, int *outs, int *ins) {
    const int last = h->L == 0 ? h->D : h->W[h->L - 1];
    int n = 0;
    for (int l = 0; l < h->L; l++) outs[n] = h->W[l], ins[n] = l == 0 ? h->D : h->W[l - 1], n++;
    if (dueling(h)) {
        outs[n] = h->H, ins[n] = last, n++;
        outs[n] = 1, ins[n] = h->H, n++;
        outs[n] = h->H, ins[n] = last, n++;
        outs[n] = h->A, ins[n] = h->H, n++;
    } else {
        outs[n] = out_cols(h), ins[n] = last, n++;
    }
    return n;
}

GradAdam segments(const srlx_mlpq *h) {
    GradAdam a{};
    int outs[kMaxParams / 2], ins[kMaxParams / 2];
    const int layers = layer_shapes(h, outs, ins);
    a.nseg = 2 * layers;
    i64 run = 0;
    for (int l = 0; l < layers; l++) {
        const int In = ins[l], Out = outs[l];
        run += (i64)Out * In;
        a.seg_end[2 * l] = run, a.seg_out[2 * l] = Out, a.seg_in[2 * l] = In;
        run += Out;
        a.seg_end[2 * l + 1] = run, a.seg_out[2 * l + 1] = Out, a.seg_in[2 * l + 1] = 0;
    }
    return a;
}

// the descriptors the learner's launch reads from memory: set 0, and on a noisy training handle set 1 (the s_0 pass)
int upload_nets(srlx_mlpq *h) {
    if (!h->d_net) SRLX_HIP(hipMalloc(&h->d_net, sizeof(Net)));
    const Net n = net_of(h, 0);
    SRLX_HIP(hipMemcpy(h->d_net, &n, sizeof(Net), hipMemcpyHostToDevice));
    if (h->noisy && h->eff[1][n_params(h) - 1]) {
        if (!h->d_net0) SRLX_HIP(hipMalloc(&h->d_net0, sizeof(Net)));
        const Net n0 = net_of(h, 1);
        SRLX_HIP(hipMemcpy(h->d_net0, &n0, sizeof(Net), hipMemcpyHostToDevice));
    }
    return SRLX_OK;
}

// begin / n of EffArgs for this handle's shapes; returns the pair count of one draw
i64 eff_shapes(const srlx_mlpq *h, EffArgs &a) {
    const GradAdam seg = segments(h);
    a.begin[0] = 0;
    for (int t = 0; t < kMaxParams; t++) {
        const i64 n = t < seg.nseg ? seg.seg_end[t] - (t ? seg.seg_end[t - 1] : 0) : 0;
        a.n[t] = n;
        a.begin[t + 1] = a.begin[t] + (t < seg.nseg && h->sig[t] ? (n + 1) / 2 : 0);
    }
    return a.begin[kMaxParams];
}

EffJob eff_job(const srlx_mlpq *h, int set, int add) {
    EffJob j{};
    for (int t = 0; t < n_params(h); t++) j.mu[t] = h->p[t], j.sig[t] = h->sig[t], j.out[t] = h->eff[set][t];
    j.draw = h->d_draw, j.add = add, j.rec = 1 + set, j.seed = h->noisy_seed;
    return j;
}

void launch_eff(const EffArgs &a, int jobs, hipStream_t st) {
    const i64 total = a.begin[kMaxParams];
    const i64 blocks = (total + 4 * kThreads - 1) / (4 * kThreads);  // (about four pairs per thread)
    hipLaunchKernelGGL(k_mlpq_noisy_eff, dim3((unsigned)(blocks < 1 ? 1 : blocks), (unsigned)jobs), dim3(kThreads), 0, st, a);
}

bool same_noisy_layers(const srlx_mlpq *a, const srlx_mlpq *b) {
    for (int t = 0; t < n_params(a); t++)
        if ((a->sig[t] != nullptr) != (b->sig[t] != nullptr)) return false;
    return true;
}

}  // namespace

extern "C" {

static int create_checked(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int dueling_units, int head, int n_actions, int64_t max_rows,
                          int64_t max_batch, int max_nstep, int device, int n_atoms = 0, double v_min = 0.0, double v_max = 0.0);

int srlx_mlpq_create(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int n_actions, int64_t max_rows, int64_t max_batch, int device) {
    SRLX_REQUIRE(out && widths, "mlpq_create: NULL argument");
    *out = nullptr;
    SRLX_REQUIRE(obs_dim >= 1 && obs_dim <= 256, "mlpq_create: %d observation elements (covered: 1..256)", obs_dim);
    SRLX_REQUIRE(n_layers >= 1 && n_layers <= 3, "mlpq_create: %d dense layers (covered: 1..3)", n_layers);
    for (int l = 0; l < n_layers; l++)
        SRLX_REQUIRE(widths[l] >= 32 && widths[l] <= 512 && widths[l] % 32 == 0, "mlpq_create: layer width %d (covered: 32..512, multiples of 32)", widths[l]);
    SRLX_REQUIRE(n_actions >= 2 && n_actions <= 32, "mlpq_create: %d actions (covered: 2..32)", n_actions);
    SRLX_REQUIRE(max_rows >= 1 && max_batch >= 0 && max_batch <= 256, "mlpq_create: max_rows %lld, max_batch %lld (learner batches <= 256)", (long long)max_rows,
                 (long long)max_batch);
    return create_checked(out, obs_dim, n_layers, widths, 0, 0, n_actions, max_rows, max_batch, kMaxNstep, device);
}

int srlx_mlpq_create_dueling(srlx_mlpq_t **out, int obs_dim, int n_trunk, const int *trunk_widths, int dueling_units, int dueling_type, int n_actions,
                             int64_t max_rows, int64_t max_batch, int max_nstep, int device) {
    SRLX_REQUIRE(out && (trunk_widths || n_trunk == 0), "mlpq_create_dueling: NULL argument");
    *out = nullptr;
    SRLX_REQUIRE(obs_dim >= 1 && obs_dim <= 256, "mlpq_create_dueling: %d observation elements (covered: 1..256)", obs_dim);
    SRLX_REQUIRE(n_trunk >= 0 && n_trunk <= 2, "mlpq_create_dueling: %d trunk layers (covered: 0..2)", n_trunk);
    for (int l = 0; l < n_trunk; l++)
        SRLX_REQUIRE(trunk_widths[l] >= 32 && trunk_widths[l] <= 512 && trunk_widths[l] % 32 == 0,
                     "mlpq_create_dueling: trunk layer width %d (covered: 32..512, multiples of 32)", trunk_widths[l]);
    SRLX_REQUIRE(dueling_units >= 32 && dueling_units <= 512 && dueling_units % 32 == 0, "mlpq_create_dueling: %d dueling units (covered: 32..512, multiples of 32)",
                 dueling_units);
    SRLX_REQUIRE(dueling_type == 0 || dueling_type == 1, "mlpq_create_dueling: dueling type %d (covered: 0 \"average\", 1 \"\")", dueling_type);
    SRLX_REQUIRE(n_actions >= 2 && n_actions <= 32, "mlpq_create_dueling: %d actions (covered: 2..32)", n_actions);
    SRLX_REQUIRE(max_rows >= 1 && max_batch >= 0 && max_batch <= 256, "mlpq_create_dueling: max_rows %lld, max_batch %lld (learner batches <= 256)",
                 (long long)max_rows, (long long)max_batch);
    SRLX_REQUIRE(max_nstep >= 1 && max_nstep <= kMaxNstep, "mlpq_create_dueling: max_nstep %d (covered: 1..%d)", max_nstep, kMaxNstep);
    return create_checked(out, obs_dim, n_trunk, trunk_widths, dueling_units, dueling_type + 1, n_actions, max_rows, max_batch, max_nstep, device);
}

int srlx_mlpq_create_categorical(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int n_actions, int n_atoms, double v_min, double v_max,
                                 int64_t max_rows, int64_t max_batch, int device) {
    SRLX_REQUIRE(out && widths, "mlpq_create_categorical: NULL argument");
    *out = nullptr;
    SRLX_REQUIRE(obs_dim >= 1 && obs_dim <= 256, "mlpq_create_categorical: %d observation elements (covered: 1..256)", obs_dim);
    SRLX_REQUIRE(n_layers >= 1 && n_layers <= 3, "mlpq_create_categorical: %d dense layers (covered: 1..3)", n_layers);
    for (int l = 0; l < n_layers; l++)
        SRLX_REQUIRE(widths[l] >= 32 && widths[l] <= 512 && widths[l] % 32 == 0, "mlpq_create_categorical: layer width %d (covered: 32..512, multiples of 32)",
                     widths[l]);
    SRLX_REQUIRE(n_actions >= 2 && n_actions <= srlxc::kMaxActions, "mlpq_create_categorical: %d actions (covered: 2..32)", n_actions);
    SRLX_REQUIRE(n_atoms >= 2 && n_atoms <= srlxc::kMaxAtoms, "mlpq_create_categorical: %d atoms (covered: 2..256)", n_atoms);
    SRLX_REQUIRE(n_actions * n_atoms <= 512, "mlpq_create_categorical: %d actions x %d atoms = %d out_layer rows (covered: <= 512)", n_actions, n_atoms,
                 n_actions * n_atoms);
    SRLX_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "mlpq_create_categorical: support %g..%g (v_min < v_max, both finite)", v_min, v_max);
    SRLX_REQUIRE(max_rows >= 1 && max_batch >= 0 && max_batch <= 256, "mlpq_create_categorical: max_rows %lld, max_batch %lld (learner batches <= 256)",
                 (long long)max_rows, (long long)max_batch);
    return create_checked(out, obs_dim, n_layers, widths, 0, 3, n_actions, max_rows, max_batch, 1, device, n_atoms, v_min, v_max);
}

// (the arguments are inside the envelope; no device call has been made yet)
static int create_checked(srlx_mlpq_t **out, int obs_dim, int n_layers, const int *widths, int dueling_units, int head, int n_actions, int64_t max_rows,
                          int64_t max_batch, int max_nstep, int device, int n_atoms, double v_min, double v_max) {
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "mlpq_create: device %d unavailable", device);
    srlx_mlpq *h = new srlx_mlpq();
    h->D = obs_dim, h->L = n_layers, h->A = n_actions, h->device = device;
    h->H = dueling_units, h->head = head, h->max_nstep = max_nstep;
    h->max_rows = max_rows, h->max_batch = max_batch;
    h->atoms = n_atoms, h->v_min = v_min, h->v_max = v_max;
    const int cols = out_cols(h);  // (categorical: the logit rows are A * atoms wide, in LDS and in the out_layer's gradient seeds)
    h->wmax = obs_dim > cols ? obs_dim : cols;
    if (dueling_units > h->wmax) h->wmax = dueling_units;
    for (int l = 0; l < n_layers; l++) {
        h->W[l] = widths[l];
        if (widths[l] > h->wmax) h->wmax = widths[l];
    }
    if (max_batch > 0) {
        const size_t plane = (size_t)max_batch * h->wmax;
        const size_t planes = dueling(h) ? n_layers + 2 : 3;  // (dueling: the trunk's, then the value and the advantage branch's hidden rows)
        hipError_t e = hipMalloc((void **)&h->x0, sizeof(float) * max_batch * obs_dim);
        if (e == hipSuccess) e = hipMalloc((void **)&h->h, sizeof(float) * planes * plane);
        if (e == hipSuccess) e = hipMalloc((void **)&h->dh, sizeof(float) * planes * plane);
        if (e == hipSuccess && dueling(h)) e = hipMalloc((void **)&h->grad_v, sizeof(float) * max_batch);
        if (e == hipSuccess && !categorical(h)) e = hipMalloc((void **)&h->q_on_next, sizeof(float) * max_batch * n_actions);
        if (e == hipSuccess && !categorical(h)) e = hipMalloc((void **)&h->q_tg_next, sizeof(float) * max_batch * n_actions);
        if (e == hipSuccess) e = hipMalloc((void **)&h->grad_q, sizeof(float) * max_batch * cols);
        if (e == hipSuccess) e = hipMalloc((void **)&h->loss_rows, sizeof(double) * max_batch);
        if (e != hipSuccess) {
            srlx_mlpq_destroy(h);
            srlx::set_error("mlpq_create: hipMalloc failed: %s", hipGetErrorString(e));
            return SRLX_ERR_NOMEM;
        }
    }
    const int S = lds_stride(h);
    int st = set_lds((const void *)k_mlpq_actor, sizeof(float) * (2 * kRows * S + kWTile));
    if (st == SRLX_OK && categorical(h)) st = set_lds((const void *)k_mlpq_actor_c51, sizeof(float) * (2 * kRows * S + kWTile));
    if (st == SRLX_OK && categorical(h)) st = set_lds((const void *)k_mlpq_learn_c51, sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile));
    if (st == SRLX_OK) st = set_lds((const void *)k_mlpq_learn_rows, sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile));
    for (int n = 1; n <= kMaxNstep && st == SRLX_OK; n++) st = set_lds(learn_nstep_fn(n), sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile));
    for (int n = 1; n <= kMaxNstep && st == SRLX_OK && dueling(h); n++)
        st = set_lds(learn_nstep_noisy_fn(n), sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile));
    if (st != SRLX_OK) {
        srlx_mlpq_destroy(h);
        return st;
    }
    *out = h;
    return SRLX_OK;
}

int srlx_mlpq_destroy(srlx_mlpq_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (int set = 0; set < 2; set++)
        for (int t = 0; t < kMaxParams; t++)
            if (h->eff[set][t]) (void)hipFree(h->eff[set][t]);
    for (void *p : {h->d_net0, (void *)h->d_draw, h->d_net, (void *)h->x0, (void *)h->h, (void *)h->dh, (void *)h->q_on_next, (void *)h->q_tg_next, (void *)h->grad_q, (void *)h->grad_v,
                    (void *)h->loss_rows})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_mlpq_bind(srlx_mlpq_t *h, float *const *d_params) {
    SRLX_REQUIRE(h && d_params, "mlpq_bind: NULL argument");
    for (int i = 0; i < n_params(h); i++) {
        SRLX_REQUIRE(d_params[i], "mlpq_bind: parameter %d is NULL", i);
        h->p[i] = d_params[i];
    }
    h->bound = true;
    srlx::DeviceGuard g(h->device);
    return upload_nets(h);
}

int srlx_mlpq_bind_noisy(srlx_mlpq_t *h, float *const *d_sigma, uint64_t seed) {
    SRLX_REQUIRE(h && d_sigma, "mlpq_bind_noisy: NULL argument");
    SRLX_REQUIRE(!categorical(h), "mlpq_bind_noisy: a categorical handle has no NoisyLinear form (c51.py builds plain Dense layers)");
    SRLX_REQUIRE(h->head, "mlpq_bind_noisy: a plain (out_layer) handle has no NoisyLinear form; noisy layers belong to srlx_mlpq_create_dueling handles");
    SRLX_REQUIRE(h->bound, "mlpq_bind_noisy: bind the parameters first (srlx_mlpq_bind: a noisy layer's entries are its mu tensors)");
    const int np = n_params(h);
    bool seen = false;
    for (int l = 0; l < np / 2; l++) {
        const bool w = d_sigma[2 * l] != nullptr, b = d_sigma[2 * l + 1] != nullptr;
        SRLX_REQUIRE(w == b, "mlpq_bind_noisy: layer %d has one of its two sigma tensors (weight and bias sigma come together)", l);
        SRLX_REQUIRE(w || l < h->L, "mlpq_bind_noisy: head layer %d has no sigma tensors (the four head layers are noisy)", l - h->L);
        SRLX_REQUIRE(w || !seen, "mlpq_bind_noisy: plain trunk layer %d behind a noisy one (plain layers form a prefix: the input value block)", l);
        seen |= w;
    }
    srlx::DeviceGuard g(h->device);
    SRLX_REQUIRE(g.ok, "mlpq_bind_noisy: device %d unavailable", h->device);
    const GradAdam seg = segments(h);
    for (int t = 0; t < np; t++) {
        const size_t n = (size_t)(seg.seg_end[t] - (t ? seg.seg_end[t - 1] : 0));
        for (int set = 0; set < (h->max_batch > 0 ? 2 : 1); set++) {
            if (d_sigma[t] && !h->eff[set][t]) SRLX_HIP(hipMalloc((void **)&h->eff[set][t], n * sizeof(float)));
            if (!d_sigma[t] && h->eff[set][t]) {
                SRLX_HIP(hipFree(h->eff[set][t]));
                h->eff[set][t] = nullptr;
            }
        }
        h->sig[t] = d_sigma[t];
    }
    if (!h->d_draw) {
        SRLX_HIP(hipMalloc((void **)&h->d_draw, 4 * sizeof(int64_t)));
        const int64_t init[4] = {0, -1, -1, 0};
        SRLX_HIP(hipMemcpy(h->d_draw, init, sizeof(init), hipMemcpyHostToDevice));
    }
    h->noisy = true, h->noisy_seed = seed;
    return upload_nets(h);  // from now on every pass reads the effective tensors of the noisy layers
}

int srlx_mlpq_bind_noisy_grads(srlx_mlpq_t *h, float *const *d_grad_sigma) {
    SRLX_REQUIRE(h && h->noisy, "mlpq_bind_noisy_grads: not a noisy handle (srlx_mlpq_bind_noisy)");
    for (int t = 0; t < n_params(h); t++) {
        SRLX_REQUIRE(!d_grad_sigma || !h->sig[t] || d_grad_sigma[t], "mlpq_bind_noisy_grads: gradient tensor %d is NULL", t);
        h->gsig[t] = d_grad_sigma && h->sig[t] ? d_grad_sigma[t] : nullptr;
    }
    return SRLX_OK;
}

int srlx_mlpq_bind_noisy_adam(srlx_mlpq_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq) {
    SRLX_REQUIRE(h && h->noisy && d_exp_avg && d_exp_avg_sq, "mlpq_bind_noisy_adam: not a noisy handle (srlx_mlpq_bind_noisy), or a NULL argument");
    SRLX_REQUIRE(h->adam, "mlpq_bind_noisy_adam: bind the mu tensors' Adam state first (srlx_mlpq_bind_adam: its hyper-parameters serve mu and sigma alike)");
    for (int t = 0; t < n_params(h); t++) {
        SRLX_REQUIRE(!h->sig[t] || (d_exp_avg[t] && d_exp_avg_sq[t]), "mlpq_bind_noisy_adam: state %d is NULL", t);
        h->msig[t] = h->sig[t] ? d_exp_avg[t] : nullptr, h->vsig[t] = h->sig[t] ? d_exp_avg_sq[t] : nullptr;
    }
    h->noisy_adam = true;
    return SRLX_OK;
}

int srlx_mlpq_noisy_draw(srlx_mlpq_t *h, const int64_t *set_next, int64_t *next_out) {
    SRLX_REQUIRE(h && h->noisy, "mlpq_noisy_draw: not a noisy handle (srlx_mlpq_bind_noisy)");
    SRLX_REQUIRE(!set_next || *set_next >= 0, "mlpq_noisy_draw: draw ids are non-negative");
    srlx::DeviceGuard g(h->device);
    SRLX_HIP(hipDeviceSynchronize());
    if (set_next) SRLX_HIP(hipMemcpy(h->d_draw, set_next, sizeof(int64_t), hipMemcpyHostToDevice));
    if (next_out) SRLX_HIP(hipMemcpy(next_out, h->d_draw, sizeof(int64_t), hipMemcpyDeviceToHost));
    return SRLX_OK;
}

int srlx_mlpq_noisy_eps(srlx_mlpq_t *h, int64_t draw, int param_index, float *d_out, void *stream) {
    SRLX_REQUIRE(h && h->noisy && d_out, "mlpq_noisy_eps: not a noisy handle (srlx_mlpq_bind_noisy), or NULL output");
    SRLX_REQUIRE(param_index >= 0 && param_index < n_params(h) && h->sig[param_index], "mlpq_noisy_eps: tensor %d is not a noisy tensor of this handle", param_index);
    SRLX_REQUIRE(draw >= 0, "mlpq_noisy_eps: draw ids are non-negative");
    srlx::DeviceGuard g(h->device);
    const GradAdam seg = segments(h);
    const i64 n = seg.seg_end[param_index] - (param_index ? seg.seg_end[param_index - 1] : 0);
    const i64 blocks = ((n + 1) / 2 + 4 * kThreads - 1) / (4 * kThreads);
    hipLaunchKernelGGL(k_mlpq_noisy_eps, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (u64)h->noisy_seed, (i64)draw, param_index, n, d_out);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_mlpq_bind_grads(srlx_mlpq_t *h, float *const *d_grads) {
    SRLX_REQUIRE(h, "mlpq_bind_grads: NULL handle");
    for (int i = 0; i < n_params(h); i++) h->grads[i] = d_grads ? d_grads[i] : nullptr;
    return SRLX_OK;
}

int srlx_mlpq_bind_adam(srlx_mlpq_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, double lr, double beta1, double beta2, double eps) {
    SRLX_REQUIRE(h && d_exp_avg && d_exp_avg_sq, "mlpq_bind_adam: NULL argument");
    for (int i = 0; i < n_params(h); i++) {
        SRLX_REQUIRE(d_exp_avg[i] && d_exp_avg_sq[i], "mlpq_bind_adam: state %d is NULL", i);
        h->m[i] = d_exp_avg[i], h->v[i] = d_exp_avg_sq[i];
    }
    h->lr = lr, h->beta1 = beta1, h->beta2 = beta2, h->eps = eps;
    h->adam = true;
    return SRLX_OK;
}

int srlx_mlpq_forward(srlx_mlpq_t *h, int64_t rows, const float *d_obs, const int64_t *d_row_offsets, float *d_q, const float *d_eps, uint64_t seed,
                      const int64_t *d_counter, int32_t *d_actions, void *stream) {
    SRLX_REQUIRE(h && h->bound && d_obs, "mlpq_forward: unbound handle or NULL observations");
    SRLX_REQUIRE(rows >= 1 && rows <= h->max_rows, "mlpq_forward: %lld rows (handle sized for %lld)", (long long)rows, (long long)h->max_rows);
    SRLX_REQUIRE(!d_actions || (d_eps && d_counter), "mlpq_forward: the policy needs eps and the counter");
    SRLX_REQUIRE(d_q || d_actions, "mlpq_forward: nothing to write");
    srlx::DeviceGuard g(h->device);
    const int S = lds_stride(h);
    Policy pol{(u64)seed, (const i64 *)d_counter, d_eps, d_actions};
    if (h->noisy) {  // a fresh draw for this call's rows (noisy_linear.py:44-52), then the pass spends it
        EffArgs ea{};
        eff_shapes(h, ea);
        ea.job[0] = eff_job(h, 0, 0);
        launch_eff(ea, 1, (hipStream_t)stream);
    }
    if (categorical(h))
        hipLaunchKernelGGL(k_mlpq_actor_c51, dim3((unsigned)((rows + kRows - 1) / kRows)), dim3(kThreads), sizeof(float) * (2 * kRows * S + kWTile), (hipStream_t)stream,
                           net_of(h), (i64)rows, d_obs, (const i64 *)d_row_offsets, S, d_q, pol, Cat{h->A, h->atoms, h->v_min, h->v_max});
    else
        hipLaunchKernelGGL(k_mlpq_actor, dim3((unsigned)((rows + kRows - 1) / kRows)), dim3(kThreads), sizeof(float) * (2 * kRows * S + kWTile), (hipStream_t)stream,
                           net_of(h), (i64)rows, d_obs, (const i64 *)d_row_offsets, S, d_q, pol, h->noisy ? (i64 *)h->d_draw : (i64 *)nullptr);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_mlpq_train_step(srlx_mlpq_t *h, const srlx_mlpq_t *target, int64_t batch, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions,
                         const float *d_rewards, const float *d_terminated, const float *d_weights, double discount, int double_dqn, int rescale,
                         const int64_t *d_steps_taken, float *d_q0, float *d_target, float *d_loss, float *d_priorities, void *stream) {
    SRLX_REQUIRE(h && target && h->bound && target->bound, "mlpq_train_step: unbound handle");
    SRLX_REQUIRE(!categorical(h) && !categorical(target), "mlpq_train_step: a categorical handle trains through srlx_mlpq_train_categorical");
    SRLX_REQUIRE(!h->noisy && !target->noisy, "mlpq_train_step: a noisy handle trains through srlx_mlpq_train_nstep");
    SRLX_REQUIRE(!h->head && !target->head, "mlpq_train_step: a dueling handle trains through srlx_mlpq_train_nstep");
    SRLX_REQUIRE(h->D == target->D && h->L == target->L && h->A == target->A, "mlpq_train_step: online and target shapes differ");
    for (int l = 0; l < h->L; l++) SRLX_REQUIRE(h->W[l] == target->W[l], "mlpq_train_step: online and target layer widths differ");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "mlpq_train_step: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_obs_base && d_offsets && d_actions && d_rewards && d_terminated && d_weights && d_q0 && d_target && d_loss && d_priorities,
                 "mlpq_train_step: NULL argument");
    SRLX_REQUIRE(!h->adam || d_steps_taken, "mlpq_train_step: Adam needs the step count");
    bool any_grad = false;
    for (int i = 0; i < 2 * (h->L + 1); i++) any_grad |= h->grads[i] != nullptr;
    SRLX_REQUIRE(h->adam || any_grad, "mlpq_train_step: neither gradients nor Adam bound");
    srlx::DeviceGuard g(h->device);
    const int S = lds_stride(h);
    Learn a{};
    a.B = batch, a.obs = d_obs_base, a.off = (const i64 *)d_offsets;
    a.x0 = h->x0, a.h = h->h, a.dh = h->dh, a.q0 = d_q0, a.grad_q = h->grad_q, a.loss_rows = h->loss_rows;
    a.hstride = (int)(h->max_batch * h->wmax);
    srlx::TdArgs &td = a.td;
    td.B = batch, td.n = 1, td.A = h->A;
    td.q_on_next = h->q_on_next, td.q_tg_next = h->q_tg_next, td.q_on_0 = d_q0;
    td.actions = d_actions, td.rewards = d_rewards, td.terminated = d_terminated, td.invalid_next = nullptr, td.weights = d_weights;
    td.discount = discount, td.retrace_h = 1.0, td.double_dqn = double_dqn, td.rescale = rescale;
    td.target = d_target, td.loss = d_loss, td.grad_q0 = h->grad_q, td.priorities = d_priorities;
    td.on_next_stride = h->A, td.on_0_stride = h->A;
    td.disc_ps = nullptr, td.td_signed = nullptr;
    hipLaunchKernelGGL(k_mlpq_learn_rows, dim3((unsigned)((batch + kItems - 1) / kItems)), dim3(kThreads), sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile),
                       (hipStream_t)stream, (const Net *)h->d_net, (const Net *)target->d_net, a, S);
    GradAdam ga = segments(h);
    ga.B = batch;
    for (int l = 0; l <= h->L; l++) {
        const i64 plane = h->max_batch * h->wmax;
        const float *dout = l < h->L ? h->dh + l * plane : h->grad_q;
        const float *xin = l == 0 ? h->x0 : h->h + (l - 1) * plane;
        for (int k = 0; k < 2; k++) {
            const int s = 2 * l + k;
            ga.dout[s] = dout, ga.xin[s] = xin;
            ga.p[s] = h->p[s], ga.g[s] = h->grads[s], ga.m[s] = h->m[s], ga.v[s] = h->v[s];
        }
    }
    ga.adam = h->adam ? 1 : 0;
    ga.lr = h->lr, ga.beta1 = h->beta1, ga.beta2 = h->beta2, ga.eps = h->eps;
    ga.steps_taken = (const i64 *)d_steps_taken;
    ga.loss_rows = h->loss_rows, ga.loss = d_loss;
    const i64 total = ga.seg_end[ga.nseg - 1];
    hipLaunchKernelGGL(k_mlpq_grad_adam, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ga);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_mlpq_train_nstep(srlx_mlpq_t *h, const srlx_mlpq_t *target, int64_t batch, int n, const float *d_obs_base, const int64_t *d_offsets,
                          const int32_t *d_actions, const float *d_rewards, const float *d_terminated, const float *d_weights, double discount, double retrace_h,
                          int double_dqn, int rescale, const int64_t *d_steps_taken, float *d_q0, float *d_target, float *d_loss, float *d_priorities, void *stream) {
    SRLX_REQUIRE(h && target && h->bound && target->bound, "mlpq_train_nstep: unbound handle");
    SRLX_REQUIRE(!categorical(h) && !categorical(target), "mlpq_train_nstep: a categorical handle trains through srlx_mlpq_train_categorical");
    SRLX_REQUIRE(h->D == target->D && h->L == target->L && h->A == target->A && h->head == target->head && h->H == target->H,
                 "mlpq_train_nstep: online and target shapes differ");
    for (int l = 0; l < h->L; l++) SRLX_REQUIRE(h->W[l] == target->W[l], "mlpq_train_nstep: online and target layer widths differ");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "mlpq_train_nstep: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(n >= 1 && n <= h->max_nstep, "mlpq_train_nstep: %d steps (handle sized for %d)", n, h->max_nstep);
    SRLX_REQUIRE(d_obs_base && d_offsets && d_actions && d_rewards && d_terminated && d_weights && d_q0 && d_target && d_loss && d_priorities,
                 "mlpq_train_nstep: NULL argument");
    SRLX_REQUIRE(!h->adam || d_steps_taken, "mlpq_train_nstep: Adam needs the step count");
    bool any_grad = false;
    for (int i = 0; i < n_params(h); i++) any_grad |= h->grads[i] != nullptr;
    SRLX_REQUIRE(h->adam || any_grad, "mlpq_train_nstep: neither gradients nor Adam bound");
    SRLX_REQUIRE(h->noisy == target->noisy && (!h->noisy || same_noisy_layers(h, target)),
                 "mlpq_train_nstep: a noisy online handle needs a noisy target with the same noisy layers, a plain one a plain target");
    if (h->noisy) {
        bool any_sigma_grad = false;
        for (int i = 0; i < n_params(h); i++) any_sigma_grad |= h->gsig[i] != nullptr;
        SRLX_REQUIRE(h->noisy_adam || any_sigma_grad, "mlpq_train_nstep: neither sigma gradients nor sigma Adam state bound (srlx_mlpq_bind_noisy_grads / _adam)");
        SRLX_REQUIRE(h->adam == h->noisy_adam, "mlpq_train_nstep: Adam steps mu and sigma alike: bind the state of both (srlx_mlpq_bind_adam, srlx_mlpq_bind_noisy_adam)");
        SRLX_REQUIRE(h != target && h->d_net0, "mlpq_train_nstep: the online handle was not created for training");
    }
    srlx::DeviceGuard g(h->device);
    const int S = lds_stride(h);
    LearnN a{};
    a.B = batch, a.obs = d_obs_base, a.off = (const i64 *)d_offsets;
    a.actions = d_actions, a.rewards = d_rewards, a.terminated = d_terminated, a.weights = d_weights;
    a.x0 = h->x0, a.h = h->h, a.dh = h->dh, a.q0 = d_q0, a.grad_q = h->grad_q, a.grad_v = h->grad_v, a.loss_rows = h->loss_rows;
    a.hstride = (int)(h->max_batch * h->wmax);
    a.target = d_target, a.priorities = d_priorities;
    a.discount = discount, a.retrace_h = retrace_h, a.double_dqn = double_dqn, a.rescale = rescale;
    for (int m = 0; m < kMaxNstep; m++) a.dm[m] = m < n ? (float)pow(discount, (double)m) : 0.f;  // (srlx_td_math.h:td_fill_discounts)
    const int P = kRows / (n + 1);
    const Net *onp = (const Net *)h->d_net, *tgp = (const Net *)target->d_net;
    if (h->noisy) {
        // three draws in one launch: the online handle's id (s_1..s_n pass, set 0) and id + 1 (s_0 pass, set 1), the target handle's id (set 0)
        EffArgs ea{};
        eff_shapes(h, ea);
        ea.job[0] = eff_job(h, 0, 0), ea.job[1] = eff_job(h, 1, 1), ea.job[2] = eff_job(target, 0, 0);
        launch_eff(ea, 3, (hipStream_t)stream);
        const Net *on0p = (const Net *)h->d_net0;
        i64 *draw_on = (i64 *)h->d_draw, *draw_tg = (i64 *)target->d_draw;
        void *args[] = {(void *)&on0p, (void *)&onp, (void *)&tgp, (void *)&a, (void *)&S, (void *)&draw_on, (void *)&draw_tg};
        SRLX_HIP(hipLaunchKernel(learn_nstep_noisy_fn(n), dim3((unsigned)((batch + P - 1) / P)), dim3(kThreads), args,
                                 sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile), (hipStream_t)stream));
    } else {
        void *args[] = {(void *)&onp, (void *)&tgp, (void *)&a, (void *)&S};
        SRLX_HIP(hipLaunchKernel(learn_nstep_fn(n), dim3((unsigned)((batch + P - 1) / P)), dim3(kThreads), args,
                                 sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile), (hipStream_t)stream));
    }
    GradAdam ga = segments(h);
    ga.B = batch;
    const i64 plane = h->max_batch * h->wmax;
    const float *trunk_out = h->L == 0 ? h->x0 : h->h + (h->L - 1) * plane;
    for (int l = 0; l < ga.nseg / 2; l++) {
        const float *dout, *xin;
        if (l < h->L) {
            dout = h->dh + l * plane, xin = l == 0 ? h->x0 : h->h + (l - 1) * plane;
        } else if (!dueling(h)) {
            dout = h->grad_q, xin = trunk_out;
        } else {
            const int k = l - h->L;  // v_layers.0, v_layers.2, adv_layers.0, adv_layers.2
            dout = k == 0 ? h->dh + h->L * plane : (k == 1 ? h->grad_v : (k == 2 ? h->dh + (h->L + 1) * plane : h->grad_q));
            xin = k == 0 || k == 2 ? trunk_out : (k == 1 ? h->h + h->L * plane : h->h + (h->L + 1) * plane);
        }
        for (int k = 0; k < 2; k++) {
            const int s = 2 * l + k;
            ga.dout[s] = dout, ga.xin[s] = xin;
            ga.p[s] = h->p[s], ga.g[s] = h->grads[s], ga.m[s] = h->m[s], ga.v[s] = h->v[s];
        }
    }
    ga.adam = h->adam ? 1 : 0;
    ga.lr = h->lr, ga.beta1 = h->beta1, ga.beta2 = h->beta2, ga.eps = h->eps;
    ga.steps_taken = (const i64 *)d_steps_taken;
    ga.loss_rows = h->loss_rows, ga.loss = d_loss;
    const i64 total = ga.seg_end[ga.nseg - 1];
    if (h->noisy) {
        NoisyGrad z{};
        for (int s = 0; s < ga.nseg; s++) z.sig[s] = h->sig[s], z.g[s] = h->gsig[s], z.m[s] = h->msig[s], z.v[s] = h->vsig[s];
        z.seed = h->noisy_seed, z.draw = (const i64 *)h->d_draw;
        hipLaunchKernelGGL(k_mlpq_grad_adam_noisy, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ga, z);
    } else {
        hipLaunchKernelGGL(k_mlpq_grad_adam, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ga);
    }
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_mlpq_train_categorical(srlx_mlpq_t *h, int64_t batch, const float *d_obs_base, const int64_t *d_offsets, const int32_t *d_actions, const float *d_rewards,
                                const float *d_terminated, double discount, const int64_t *d_steps_taken, float *d_q0, float *d_p0, float *d_m, float *d_loss,
                                float *d_item_loss, void *stream) {
    SRLX_REQUIRE(h && h->bound, "mlpq_train_categorical: unbound handle");
    SRLX_REQUIRE(categorical(h), "mlpq_train_categorical: not a categorical handle (srlx_mlpq_create_categorical); a %s handle trains through %s",
                 dueling(h) ? "dueling" : "plain", dueling(h) ? "srlx_mlpq_train_nstep" : "srlx_mlpq_train_step");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "mlpq_train_categorical: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_obs_base && d_offsets && d_actions && d_rewards && d_terminated && d_q0 && d_p0 && d_m && d_loss && d_item_loss,
                 "mlpq_train_categorical: NULL argument");
    SRLX_REQUIRE(std::isfinite(discount), "mlpq_train_categorical: discount %g", discount);
    SRLX_REQUIRE(!h->adam || d_steps_taken, "mlpq_train_categorical: Adam needs the step count");
    bool any_grad = false;
    for (int i = 0; i < n_params(h); i++) any_grad |= h->grads[i] != nullptr;
    SRLX_REQUIRE(h->adam || any_grad, "mlpq_train_categorical: neither gradients nor Adam bound");
    srlx::DeviceGuard g(h->device);
    const int S = lds_stride(h);
    LearnC a{};
    a.obs = d_obs_base, a.off = (const i64 *)d_offsets;
    a.x0 = h->x0, a.h = h->h, a.dh = h->dh, a.loss_rows = h->loss_rows;
    a.hstride = (int)(h->max_batch * h->wmax);
    srlxc::Items &it = a.it;
    it.B = batch, it.A = h->A, it.N = h->atoms, it.v_min = h->v_min, it.v_max = h->v_max, it.discount = discount;
    it.actions = d_actions, it.rewards = d_rewards, it.terminated = d_terminated;
    it.q0 = d_q0, it.p0 = d_p0, it.m = d_m, it.grad = h->grad_q, it.item_loss = d_item_loss;
    hipLaunchKernelGGL(k_mlpq_learn_c51, dim3((unsigned)((batch + kItems - 1) / kItems)), dim3(kThreads), sizeof(float) * ((2 * kRows + 2 * kItems) * S + kWTile),
                       (hipStream_t)stream, (const Net *)h->d_net, a, S);
    GradAdam ga = segments(h);  // (the out_layer segment has seg_out = A * atoms)
    ga.B = batch;
    const i64 plane = h->max_batch * h->wmax;
    for (int l = 0; l <= h->L; l++) {
        const float *dout = l < h->L ? h->dh + l * plane : h->grad_q;
        const float *xin = l == 0 ? h->x0 : h->h + (l - 1) * plane;
        for (int k = 0; k < 2; k++) {
            const int s = 2 * l + k;
            ga.dout[s] = dout, ga.xin[s] = xin;
            ga.p[s] = h->p[s], ga.g[s] = h->grads[s], ga.m[s] = h->m[s], ga.v[s] = h->v[s];
        }
    }
    ga.adam = h->adam ? 1 : 0;
    ga.lr = h->lr, ga.beta1 = h->beta1, ga.beta2 = h->beta2, ga.eps = h->eps;
    ga.steps_taken = (const i64 *)d_steps_taken;
    ga.loss_rows = h->loss_rows, ga.loss = d_loss;
    const i64 total = ga.seg_end[ga.nseg - 1];
    hipLaunchKernelGGL(k_mlpq_grad_adam, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ga);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_c51_loss(int64_t batch, int n_actions, int n_atoms, double v_min, double v_max, double discount, const float *d_logits_next, const float *d_logits_0,
                  const int32_t *d_actions, const float *d_rewards, const float *d_terminated, float *d_m, float *d_p0, float *d_grad_logits, float *d_loss,
                  void *stream) {
    SRLX_REQUIRE(batch >= 1, "c51_loss: batch %lld", (long long)batch);
    SRLX_REQUIRE(n_actions >= 1 && n_actions <= srlxc::kMaxActions, "c51_loss: %d actions (covered: 1..32)", n_actions);
    SRLX_REQUIRE(n_atoms >= 2 && n_atoms <= srlxc::kMaxAtoms, "c51_loss: %d atoms (covered: 2..256)", n_atoms);
    SRLX_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max && std::isfinite(discount), "c51_loss: support %g..%g, discount %g", v_min, v_max, discount);
    SRLX_REQUIRE(d_logits_next && d_logits_0 && d_actions && d_rewards && d_terminated && d_m && d_p0 && d_grad_logits && d_loss, "c51_loss: NULL argument");
    srlxc::Items it{};
    it.B = batch, it.A = n_actions, it.N = n_atoms, it.v_min = v_min, it.v_max = v_max, it.discount = discount;
    it.actions = d_actions, it.rewards = d_rewards, it.terminated = d_terminated;
    it.q0 = nullptr, it.p0 = d_p0, it.m = d_m, it.grad = d_grad_logits, it.item_loss = nullptr;
    hipLaunchKernelGGL(k_c51_loss, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, it, d_logits_next, d_logits_0, d_loss);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_mlpq_publish(const srlx_mlpq_t *src, srlx_mlpq_t *dst, void *stream) {
    SRLX_REQUIRE(src && dst && src->bound && dst->bound, "mlpq_publish: unbound handle");
    SRLX_REQUIRE(src->D == dst->D && src->L == dst->L && src->A == dst->A && src->head == dst->head && src->H == dst->H && src->atoms == dst->atoms,
                 "mlpq_publish: shapes differ");
    for (int l = 0; l < src->L; l++) SRLX_REQUIRE(src->W[l] == dst->W[l], "mlpq_publish: shapes differ");
    SRLX_REQUIRE(src->noisy == dst->noisy && (!src->noisy || same_noisy_layers(src, dst)),
                 "mlpq_publish: a noisy source needs a noisy destination with the same noisy layers, a plain one a plain destination");
    srlx::DeviceGuard g(src->device);
    GradAdam c = segments(src);
    for (int s = 0; s < c.nseg; s++) c.p[s] = src->p[s], c.g[s] = dst->p[s];
    const i64 total = c.seg_end[c.nseg - 1];
    hipLaunchKernelGGL(k_mlpq_copy, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, c.nseg, c);
    if (src->noisy) {  // the sigmas (model_torch.py:125-127 copies the whole state_dict): the noisy tensors' segments, compacted
        GradAdam z{};
        i64 run = 0;
        for (int s = 0; s < c.nseg; s++) {
            if (!src->sig[s]) continue;
            run += c.seg_end[s] - (s ? c.seg_end[s - 1] : 0);
            z.seg_end[z.nseg] = run, z.p[z.nseg] = src->sig[s], z.g[z.nseg] = dst->sig[s], z.nseg++;
        }
        hipLaunchKernelGGL(k_mlpq_copy, dim3((unsigned)((run + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, z.nseg, z);
    }
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_cartpole_step(int64_t n_envs, double *d_state, int32_t *d_steps, int32_t *d_episodes, const uint8_t *d_needs_reset, const int32_t *d_actions,
                       int64_t max_steps, uint64_t seed, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_done, void *stream) {
    SRLX_REQUIRE(n_envs > 0 && d_state && d_steps && d_episodes && d_obs && max_steps > 0, "cartpole_step: bad argument");
    SRLX_REQUIRE(!d_needs_reset || (d_actions && d_reward && d_terminated && d_done), "cartpole_step: a step needs actions and the scalar outputs");
    hipLaunchKernelGGL(k_cartpole, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (i64)n_envs, d_state, d_steps, d_episodes,
                       d_needs_reset, d_actions, (i64)max_steps, (u64)seed, d_obs, d_reward, d_terminated, d_done);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
