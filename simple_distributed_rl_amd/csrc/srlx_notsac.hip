// srlx_notsac.hip -- the whole update of NoT_SAC (srl/algorithms/sac_not/torch_model.py:131-191) on flat observations in six launches, and a forward-only pass.
// Two networks: the policy (1..3 ReLU layers + the head: Linear(A) logits, or Linear(K) locs and Linear(K) log-scales) and the Q-network (act_block =
// Linear(A or K, E) + SiLU beside the observation, the two concatenated, 1..3 ReLU layers + Linear(1)).  The arithmetic contract is DESIGN.md 7r and
// include/srlx.h; its per-row closed forms are srlx_notsac_math.h.
//
// The work is srlx_vppo.hip's, not a GEMM's (<= 256 rows through <= 4 layers of <= 512 units), and so is the shape: 256 threads over <= 16 rows, each layer's
// weight staged through LDS in tiles of whole rows (srlx_mlp_rows.h with float64 accumulators), hidden rows and their gradients kept in per-layer planes.
//   k_notsac_q_rows   up to 16 rows per workgroup (rows_per_workgroup: one row each while the launch fits the machine, so an update of B <= 256 runs one row per
//                     workgroup unless srlx_notsac_set_rows_per_workgroup says otherwise): the policy on s' (nothing kept), the next action from noise plane 0,
//                     Q(s', a') and the target; Q(s, a) with the
//                     planes kept; the row's Huber and MSE terms and the seed d loss / d q; the backward chain down q_block, through the embedding columns of
//                     its first weight and the SiLU derivative into the act_block
//   k_notsac_grad     one thread per parameter of ONE network (a segment table each): the gradient before the clip, a sum over the batch in row order; every
//                     workgroup leaves the sum of its squares; the last threads of the launch reduce the network's losses
//   k_notsac_step     every workgroup sums the same partial squares in the same order (the norm), then one thread per parameter: the clipped gradient and Adam
//   k_notsac_pi_rows  the policy on s with the planes kept, the action from noise plane 1, the STEPPED Q-network's forward with its masks kept, the seed -1 / B
//                     down q_out and q_block, through the embedding columns, the SiLU derivative and the act_block's weight transposed (d loss / d action),
//                     through the head's Jacobian and down the policy's chain
//   k_notsac_forward  the head's outputs of n rows and, for given actions, q(s, a)
// One update: q_rows, grad (Q), step (Q), pi_rows, grad (policy), step (policy); the stream orders them and nothing synchronises the host.
// LDS: three row buffers of 16 x (widest row + 1) floats (the act_block's pre-activations have to outlive q_block's chains) and the 32 KB weight tile:
// 131 264 bytes at a widest row of 512 -- the concatenated row of D + E floats is held to that.
// No atomics and a fixed order in every sum: equal inputs give equal bits.
#include "srlx_notsac_math.h"
#include "srlx_param_tail.h"
#include <cmath>

namespace {

using i64 = int64_t;

using srlxm::kRows;
using srlxm::kThreads;
using srlxm::Layers;
using srlxm::Src;
using srlxm::SumSeed;
using srlxn::kHeadCols;
using srlxn::kNormalLs;
using srlxt::Seg;
constexpr int kNetTensors = 10;  // policy: 2 x (3 layers + 2 heads); Q: 2 x (act_block + 3 layers + q_out)
static_assert(2 * kNetTensors <= srlxt::kMaxTensors, "the policy's tensors, then the Q-network's, in one ParamSet");
constexpr int kMaxWidth = 512;   // of a hidden layer and of the concatenated row

struct Net {  // (in device memory: the kernels read it through a pointer)
    Layers pi, q;
    const float *w_ls, *b_ls;  // the Normal head's second Linear (NULL: the Gumbel head)
    const float *wa, *ba;      // act_block's Linear [E][A]
};

}  // namespace

struct srlx_notsac {
    int D, head, A, Lp, Lq, E, device;  // head 0: Gumbel with A actions; 1: Normal with A = K elements
    int Wp[3], Wq[3];
    int wmax, ntp, ntq;
    int rpw;  // rows per workgroup of the row kernels; 0: rows_per_workgroup's own choice
    i64 max_batch, elements_p, elements_q, blocks_p, blocks_q;
    srlxt::ParamSet ps;  // the policy's tensors, then the Q-network's
    Net *d_net;
    Seg *d_segs;        // [2][kNetTensors]: policy, Q
    float *hp, *dhp;    // planes [3][max_batch][wmax]: the policy's hidden rows and their gradients
    float *hq, *dhq;    // the same of q_block
    float *xcat;        // [max_batch][D + E]: q_block's input rows
    float *zact, *dact; // [max_batch][E]: act_block's pre-activations and their gradients
    float *ain;         // [max_batch][A]: act_block's input rows
    float *dlast_q;     // [max_batch]: d loss / d q
    float *dlast_p;     // [max_batch][kHeadCols]: d loss / d (head outputs)
    float *rows;        // [3][max_batch]: the rows' Huber terms, MSE terms and q(s, pi(s))
    double *partials;   // [max(blocks_p, blocks_q)]: sums of squared gradients
};

namespace {

int lds_stride(const srlx_notsac *h) { return h->wmax + 1; }
size_t lds_bytes(const srlx_notsac *h) { return srlxt::row_lds_bytes(3, h->wmax); }

struct Bufs {
    float *b0, *b1, *b2, *wl;
    int S;
};

// The head's outputs of rows i0..i0+nb-1 of `states`: zs[r][kHeadCols] = logits, or locs at 0.. and RAW log-scales at kNormalLs...  `keep`: the planes of the
// hidden rows (NULL: not kept).  The same chains whatever rows share the workgroup.  Begins and ends behind a barrier.
__device__ __forceinline__ void pi_forward(const Net &n, const float *__restrict__ states, i64 i0, int nb, int D, Bufs B, float *keep, i64 plane, float *zs) {
    const int t = threadIdx.x, S = B.S;
    __syncthreads();
    for (int p = t; p < nb * D; p += kThreads) B.b0[(p / D) * S + p % D] = states[(i0 + p / D) * D + p % D];
    __syncthreads();
    const float *z = srlxm::forward_rows<double>(n.pi, n.pi.L + 1, nb, B.b0, B.b1, S, B.wl, keep, plane, i0, keep ? nb : 0);
    srlxm::head_rows(n.pi, n.w_ls, n.b_ls, nb, z, z == B.b0 ? B.b1 : B.b0, B.b2, S, B.wl, zs);
}

struct QKeep {  // what the Q-network's forward leaves in global memory (NULL: not kept)
    float *hq, *xcat, *zact, *ain;
    i64 plane;
};

// q of the rows: the observations from `states`, the actions from the LDS rows `acts` [kRows][kHeadCols] (A columns).  act_block's Linear, SiLU in float64,
// the concatenated row, q_block and q_out.  Returns the buffer whose column 0 holds q; b2 keeps act_block's pre-activations.  Begins and ends behind a barrier.
__device__ __forceinline__ float *q_forward(const Net &n, const float *__restrict__ states, i64 i0, int nb, int D, int A, int E, const float *acts, Bufs B, QKeep kp) {
    const int t = threadIdx.x, S = B.S, W = D + E;
    __syncthreads();
    for (int p = t; p < nb * A; p += kThreads) {
        const float a = acts[(p / A) * kHeadCols + p % A];
        B.b1[(p / A) * S + p % A] = a;
        if (kp.ain) kp.ain[(i0 + p / A) * A + p % A] = a;
    }
    __syncthreads();
    srlxm::dense<double>(n.wa, n.ba, A, E, nb, B.b1, S, B.b2, S, false, B.wl);
    __syncthreads();
    for (int p = t; p < nb * W; p += kThreads) {
        const int r = p / W, k = p % W;
        const float x = k < D ? states[(i0 + r) * D + k] : srlxn::silu(B.b2[r * S + k - D]);
        B.b0[r * S + k] = x;
        if (kp.xcat) kp.xcat[(i0 + r) * W + k] = x;
    }
    if (kp.zact)
        for (int p = t; p < nb * E; p += kThreads) kp.zact[(i0 + p / E) * E + p % E] = B.b2[(p / E) * S + p % E];
    __syncthreads();
    return srlxm::forward_rows<double>(n.q, n.q.L + 1, nb, B.b0, B.b1, S, B.wl, kp.hq, kp.plane, i0, kp.hq ? nb : 0);
}

// From the rows' d loss / d q in column 0 of `dn`: d loss / d h down q_block (written to the planes of dhq), then d loss / d (act_block pre-activation)
// through the embedding columns of q_block's first weight and the SiLU derivative at the pre-activations in `z` (LDS rows).  Returns the buffer that holds those
// rows (E columns), behind a barrier; `dact` (global, NULL: not kept) receives them too.
__device__ __forceinline__ float *q_backward(const Net &n, int nb, i64 i0, int D, int E, float *dn, float *dc, const float *z, int S, const float *hq, float *dhq,
                                             i64 plane, float *dact) {
    srlxm::backward_rows<double>(n.q, n.q.L - 1, nb, i0, dc, dn, S, hq, dhq, plane);
    const float *d0 = (n.q.L & 1) ? dc : dn;  // the rows of d loss / d h_0
    float *out = (n.q.L & 1) ? dn : dc;
    const int W0 = n.q.W0, W = D + E;
    const float *w0 = n.q.w0 + D;
    for (int p = threadIdx.x; p < nb * E; p += kThreads) {
        const int r = p / E, j = p % E;
        double acc = 0.0;
#pragma unroll 8
        for (int u = 0; u < W0; u++) acc = srlxm::fma_acc((double)d0[r * S + u], (double)w0[(i64)u * W + j], acc);
        const float g = (float)(acc * srlxn::silu_grad(z[r * S + j]));
        out[r * S + j] = g;
        if (dact) dact[(i0 + r) * E + j] = g;
    }
    __syncthreads();
    return out;
}

struct Batch {
    i64 B;
    const float *s, *s2, *reward, *not_term, *total_reward;
    const int32_t *action_i;  // Gumbel head
    const float *action_f;    // Normal head
    const float *noise;       // [2][B][A]
    float *q, *target, *next_action, *pi_action;
};

struct Work {
    float *hp, *dhp, *hq, *dhq, *xcat, *zact, *dact, *ain, *dlast_q, *dlast_p, *rows;
    i64 plane, max_batch;
};

struct Cfg {
    float discount, coeff, ls_lo, ls_hi;
    double inv_b;
    int squashed;
};

// The row kernels' arguments wait in LDS: held in scalar registers through the network passes they spilled (the first barrier of pi_forward publishes them).
struct RowArgs {
    Batch a;
    Work w;
    Cfg c;
};

__global__ void __launch_bounds__(kThreads) k_notsac_q_rows(const Net *__restrict__ net, RowArgs args, int rpw, int D, int A, int E, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const Bufs B{sm, sm + kRows * S, sm + 2 * kRows * S, sm + 3 * kRows * S, S};
    __shared__ RowArgs held;
    if (threadIdx.x == 0) held = args;
    const Batch &a = held.a;
    const Work &w = held.w;
    const Cfg &c = held.c;
    __shared__ float zs[kRows * kHeadCols], acts[kRows * kHeadCols], nqs[kRows];
    const Net &n = *net;
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(args.a.B - i0 < rpw ? args.a.B - i0 : rpw);
    const bool normal = n.w_ls != nullptr;
    // ---- the target: a' from the policy on s' and noise plane 0, then Q(s', a')
    pi_forward(n, args.a.s2, i0, nb, D, B, nullptr, 0, zs);
    if (normal) {
        if (t < nb * A) {
            const int r = t / A, j = t % A;
            const float x = srlxn::normal_action(zs[r * kHeadCols + j], zs[r * kHeadCols + kNormalLs + j], c.ls_lo, c.ls_hi, a.noise[(i0 + r) * A + j], c.squashed);
            acts[r * kHeadCols + j] = x;
            a.next_action[(i0 + r) * A + j] = x;
        }
    } else if (t < nb) {
        const int best = srlxn::gumbel_argmax(zs + t * kHeadCols, a.noise + (i0 + t) * A, A);
        for (int k = 0; k < A; k++) {
            acts[t * kHeadCols + k] = k == best ? 1.f : 0.f;
            a.next_action[(i0 + t) * A + k] = k == best ? 1.f : 0.f;
        }
    }
    const float *qo = q_forward(n, a.s2, i0, nb, D, A, E, acts, B, QKeep{nullptr, nullptr, nullptr, nullptr, 0});
    if (t < nb) nqs[t] = qo[t * S];
    __syncthreads();
    // ---- Q(s, a) of the stored action, everything kept
    if (normal) {
        if (t < nb * A) acts[(t / A) * kHeadCols + t % A] = a.action_f[(i0 + t / A) * A + t % A];
    } else if (t < nb) {
        const int act = a.action_i[i0 + t];
        const int ac = act < 0 ? 0 : (act >= A ? A - 1 : act);
        for (int k = 0; k < A; k++) acts[t * kHeadCols + k] = k == ac ? 1.f : 0.f;
    }
    qo = q_forward(n, a.s, i0, nb, D, A, E, acts, B, QKeep{w.hq, w.xcat, w.zact, w.ain, w.plane});
    const float qv = t < nb ? qo[t * S] : 0.f;
    __syncthreads();
    if (t < nb) {
        const i64 b = i0 + t;
        const srlxn::QRow r = srlxn::q_row(qv, nqs[t], a.reward[b], a.not_term[b], a.total_reward[b], c.discount, c.coeff, c.inv_b);
        a.q[b] = qv, a.target[b] = r.target;
        w.rows[b] = r.huber, w.rows[w.max_batch + b] = r.align;
        w.dlast_q[b] = r.dq;
        B.b0[t * S] = r.dq;  // the rows of d loss / d (q_out's output), column 0
    }
    __syncthreads();
    q_backward(n, nb, i0, D, E, B.b0, B.b1, B.b2, S, w.hq, w.dhq, w.plane, w.dact);
}

__global__ void __launch_bounds__(kThreads) k_notsac_pi_rows(const Net *__restrict__ net, RowArgs args, int rpw, int D, int A, int E, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const Bufs B{sm, sm + kRows * S, sm + 2 * kRows * S, sm + 3 * kRows * S, S};
    __shared__ RowArgs held;
    if (threadIdx.x == 0) held = args;
    const Batch &a = held.a;
    const Work &w = held.w;
    const Cfg &c = held.c;
    __shared__ float zs[kRows * kHeadCols], acts[kRows * kHeadCols], ga[kRows * kHeadCols], dzs[kRows * kHeadCols];
    const Net &n = *net;
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(args.a.B - i0 < rpw ? args.a.B - i0 : rpw);
    const bool normal = n.w_ls != nullptr;
    pi_forward(n, args.a.s, i0, nb, D, B, args.w.hp, args.w.plane, zs);
    const float *noise = a.noise + a.B * A;  // plane 1
    dzs[t] = 0.f;  // (kRows * kHeadCols = kThreads: srlx_mlp_rows.h asserts it)
    if (normal) {
        if (t < nb * A) {
            const int r = t / A, j = t % A;
            const float x = srlxn::normal_action(zs[r * kHeadCols + j], zs[r * kHeadCols + kNormalLs + j], c.ls_lo, c.ls_hi, noise[(i0 + r) * A + j], c.squashed);
            acts[r * kHeadCols + j] = x;
            a.pi_action[(i0 + r) * A + j] = x;
        }
    } else if (t < nb) {
        srlxn::gumbel_softmax(zs + t * kHeadCols, noise + (i0 + t) * A, A, acts + t * kHeadCols);
        for (int k = 0; k < A; k++) a.pi_action[(i0 + t) * A + k] = acts[t * kHeadCols + k];
    }
    // ---- the stepped Q-network on (s, pi(s)): its masks kept, the seed -1 / B
    const float *qo = q_forward(n, a.s, i0, nb, D, A, E, acts, B, QKeep{w.hq, nullptr, nullptr, nullptr, w.plane});
    const float qv = t < nb ? qo[t * S] : 0.f;
    __syncthreads();
    if (t < nb) {
        w.rows[2 * w.max_batch + i0 + t] = qv;
        B.b0[t * S] = (float)(-c.inv_b);
    }
    __syncthreads();
    const float *dz = q_backward(n, nb, i0, D, E, B.b0, B.b1, B.b2, S, w.hq, w.dhq, w.plane, nullptr);
    // ---- d loss / d action through act_block's weight transposed, then through the head
    if (t < nb * A) {
        const int r = t / A, i = t % A;
        double acc = 0.0;
        for (int j = 0; j < E; j++) acc = srlxm::fma_acc((double)dz[r * S + j], (double)n.wa[(i64)j * A + i], acc);
        ga[r * kHeadCols + i] = (float)acc;
    }
    __syncthreads();
    if (normal) {
        if (t < nb * A) {
            const int r = t / A, j = t % A;
            float dloc, dls;
            srlxn::normal_action_grad(ga[r * kHeadCols + j], acts[r * kHeadCols + j], zs[r * kHeadCols + kNormalLs + j], c.ls_lo, c.ls_hi, noise[(i0 + r) * A + j],
                                      c.squashed, dloc, dls);
            dzs[r * kHeadCols + j] = dloc, dzs[r * kHeadCols + kNormalLs + j] = dls;
        }
    } else if (t < nb) {
        srlxn::softmax_grad(acts + t * kHeadCols, ga + t * kHeadCols, A, dzs + t * kHeadCols);
    }
    __syncthreads();
    if (t < nb * kHeadCols) w.dlast_p[i0 * kHeadCols + t] = dzs[t];
    const int Lp = n.pi.L;
    // the policy's top hidden layer is read by the head's one or two Linear layers: one float64 chain over both
    const int HO = n.pi.Out;
    const Src none{nullptr, 0, 0, nullptr};
    const Src head{dzs, kHeadCols, HO, n.pi.weight(Lp)};
    const Src head_ls = normal ? Src{dzs + kNormalLs, kHeadCols, HO, n.w_ls} : none;
    srlxm::backward_rows<double>(n.pi, Lp - 1, nb, i0, B.b0, B.b1, S, w.hp, w.dhp, w.plane, SumSeed{head, head_ls, none});
}

__global__ void __launch_bounds__(kThreads) k_notsac_forward(const Net *__restrict__ net, i64 rows, const float *__restrict__ states, const float *__restrict__ actions,
                                                             float *__restrict__ head0, float *__restrict__ head1, float *__restrict__ q, float ls_lo, float ls_hi, int rpw,
                                                             int D, int A, int E, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const Bufs B{sm, sm + kRows * S, sm + 2 * kRows * S, sm + 3 * kRows * S, S};
    __shared__ float zs[kRows * kHeadCols], acts[kRows * kHeadCols];
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(rows - i0 < rpw ? rows - i0 : rpw);
    const Net &n = *net;
    if (head0) {
        pi_forward(n, states, i0, nb, D, B, nullptr, 0, zs);
        if (t < nb * A) {
            const int r = t / A, j = t % A;
            head0[(i0 + r) * A + j] = zs[r * kHeadCols + j];
            if (head1) head1[(i0 + r) * A + j] = srlxn::clampf(zs[r * kHeadCols + kNormalLs + j], ls_lo, ls_hi);
        }
    }
    if (q) {
        if (t < nb * A) acts[(t / A) * kHeadCols + t % A] = actions[(i0 + t / A) * A + t % A];
        const float *qo = q_forward(n, states, i0, nb, D, A, E, acts, B, QKeep{nullptr, nullptr, nullptr, nullptr, 0});
        if (t < nb) q[i0 + t] = qo[t * S];
    }
}

// The loss sums of k_notsac_grad's last n threads, one scale for all: out[k] = scale * sum of rows[k]
struct LossSums {
    int n;  // <= 2
    i64 B;
    const float *rows;  // [n][max_batch]
    i64 max_batch;
    double scale;
    float *out;  // [n]
    __device__ void operator()(int k) const {
        double s = 0.0;
        for (i64 b = 0; b < B; b++) s += (double)rows[k * max_batch + b];
        out[k] = (float)(s * scale);
    }
};

struct GradArgs {
    const Seg *segs;
    int nseg;
    const float *xin0;  // the caller's states: the input rows of the policy's first layer
    double *partials;
    LossSums sums;
};

__global__ void __launch_bounds__(kThreads) k_notsac_grad(GradArgs a) { srlxt::grad_body(a.segs, a.nseg, a.sums.B, a.xin0, a.partials, a.sums); }

__global__ void __launch_bounds__(kThreads) k_notsac_step(srlxt::StepArgs a) { srlxt::step_body(a); }

int check_shape(const char *who, int D, int head, int A, int np, const int *pw, int nq, const int *qw, int E, i64 max_batch) {
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(head == 0 || head == 1, "%s: head kind %d (0 Gumbel, 1 Normal)", who, head);
    SRLX_REQUIRE(head == 1 || (A >= 2 && A <= 16), "%s: %d actions (2..16)", who, A);
    SRLX_REQUIRE(head == 0 || (A >= 1 && A <= 8), "%s: %d action elements (1..8)", who, A);
    SRLX_REQUIRE(srlxt::widths_ok(np, 1, 3, pw), "%s: the policy block is 1..3 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(srlxt::widths_ok(nq, 1, 3, qw), "%s: the q block is 1..3 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(E >= 32 && E <= kMaxWidth && E % 32 == 0, "%s: %d action-embedding units (32..512 in multiples of 32)", who, E);
    SRLX_REQUIRE(D + E <= kMaxWidth, "%s: the concatenated row of %d + %d floats is wider than %d (the row buffers in LDS)", who, D, E, kMaxWidth);
    SRLX_REQUIRE(max_batch >= 1 && max_batch <= 256, "%s: max_batch %lld (1..256)", who, (long long)max_batch);
    return SRLX_OK;
}

// (out, in) of every Linear of one network in parameters() order
int policy_shapes(const srlx_notsac *h, int (*shape)[2]) {
    int n = 0, in = h->D;
    for (int l = 0; l < h->Lp; l++) shape[n][0] = h->Wp[l], shape[n][1] = in, in = h->Wp[l], n++;
    shape[n][0] = h->A, shape[n][1] = in, n++;
    if (h->head) shape[n][0] = h->A, shape[n][1] = in, n++;
    return n;
}

int q_shapes(const srlx_notsac *h, int (*shape)[2]) {
    int n = 0, in = h->D + h->E;
    shape[n][0] = h->E, shape[n][1] = h->A, n++;
    for (int l = 0; l < h->Lq; l++) shape[n][0] = h->Wq[l], shape[n][1] = in, in = h->Wq[l], n++;
    shape[n][0] = 1, shape[n][1] = in, n++;
    return n;
}

i64 elements_of(int n, const int (*shape)[2]) {
    i64 e = 0;
    for (int l = 0; l < n; l++) e += (i64)shape[l][0] * shape[l][1] + shape[l][0];
    return e;
}

int upload_net(srlx_notsac *h) {
    Net n;
    float *const *p = h->ps.p;
    n.pi = srlxt::chain(h->D, h->Lp, h->Wp, h->A, p);
    n.w_ls = h->head ? p[2 * (h->Lp + 1)] : nullptr;
    n.b_ls = h->head ? p[2 * (h->Lp + 1) + 1] : nullptr;
    float *const *q = p + h->ntp;
    n.wa = q[0], n.ba = q[1];
    n.q = srlxt::chain(h->D + h->E, h->Lq, h->Wq, 1, q + 2);
    SRLX_HIP(hipMemcpy(h->d_net, &n, sizeof(n), hipMemcpyHostToDevice));
    h->ps.net_ok = true;
    return SRLX_OK;
}

int upload_table(srlx_notsac *h) {
    Seg segs[2 * kNetTensors];
    memset(segs, 0, sizeof(segs));
    int shape[kNetTensors / 2][2];
    const i64 plane = h->max_batch * h->wmax;
    // ---- the policy
    int nl = policy_shapes(h, shape);
    i64 end = 0;
    for (int l = 0; l < nl; l++) {
        const float *dout, *xin;
        int stride = shape[l][0];
        if (l < h->Lp) {
            dout = h->dhp + (i64)l * plane, xin = l ? h->hp + (i64)(l - 1) * plane : nullptr;
        } else {  // 0: logits or locs, 1: log-scales
            dout = h->dlast_p + (l - h->Lp ? kNormalLs : 0), stride = kHeadCols, xin = h->hp + (i64)(h->Lp - 1) * plane;
        }
        srlxt::push_linear(segs + 2 * l, end, shape[l][0], shape[l][1], stride, dout, xin, h->ps, 2 * l);
    }
    // ---- the Q-network
    nl = q_shapes(h, shape);
    end = 0;
    for (int l = 0; l < nl; l++) {
        const float *dout, *xin;
        const int k = l - 1;  // q_block's layer
        if (l == 0) {
            dout = h->dact, xin = h->ain;
        } else if (k < h->Lq) {
            dout = h->dhq + (i64)k * plane, xin = k ? h->hq + (i64)(k - 1) * plane : h->xcat;
        } else {
            dout = h->dlast_q, xin = h->hq + (i64)(h->Lq - 1) * plane;
        }
        srlxt::push_linear(segs + kNetTensors + 2 * l, end, shape[l][0], shape[l][1], shape[l][0], dout, xin, h->ps, h->ntp + 2 * l);
    }
    SRLX_HIP(hipMemcpy(h->d_segs, segs, sizeof(segs), hipMemcpyHostToDevice));
    h->ps.table_ok = true;
    return SRLX_OK;
}

void fill(srlx_notsac *h, int D, int head, int A, int np, const int *pw, int nq, const int *qw, int E, i64 max_batch, int device) {
    h->D = D, h->head = head, h->A = A, h->Lp = np, h->Lq = nq, h->E = E, h->device = device, h->max_batch = max_batch;
    int w = D + E > kHeadCols ? D + E : kHeadCols;
    for (int l = 0; l < np; l++) h->Wp[l] = pw[l], w = pw[l] > w ? pw[l] : w;
    for (int l = 0; l < nq; l++) h->Wq[l] = qw[l], w = qw[l] > w ? qw[l] : w;
    h->wmax = w;
    int shape[kNetTensors / 2][2];
    int n = policy_shapes(h, shape);
    h->ntp = 2 * n, h->elements_p = elements_of(n, shape);
    n = q_shapes(h, shape);
    h->ntq = 2 * n, h->elements_q = elements_of(n, shape);
    h->blocks_p = (h->elements_p + 2 + kThreads - 1) / kThreads;
    h->blocks_q = (h->elements_q + 2 + kThreads - 1) / kThreads;
}

// rows per workgroup of the row kernels: what srlx_notsac_set_rows_per_workgroup asked for, or the shared rule
int rows_per_workgroup(const srlx_notsac *h, i64 n) { return h->rpw ? h->rpw : srlxt::rows_per_workgroup(n); }

i64 scratch_floats(const srlx_notsac *h) {
    const i64 mb = h->max_batch, blocks = h->blocks_p > h->blocks_q ? h->blocks_p : h->blocks_q;
    return 12 * mb * h->wmax + mb * (h->D + h->E) + 2 * mb * h->E + mb * h->A + mb + mb * kHeadCols + 3 * mb + 2 * blocks;
}

}  // namespace

extern "C" {

int64_t srlx_notsac_scratch_floats(int obs_dim, int head, int n_out, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int act_emb_units,
                                   int64_t max_batch) {
    if (check_shape("notsac_scratch_floats", obs_dim, head, n_out, n_policy, policy_widths, n_q, q_widths, act_emb_units, max_batch) != SRLX_OK) return -1;
    srlx_notsac h{};
    fill(&h, obs_dim, head, n_out, n_policy, policy_widths, n_q, q_widths, act_emb_units, max_batch, 0);
    return scratch_floats(&h);
}

int srlx_notsac_create(srlx_notsac_t **out, int obs_dim, int head, int n_out, int n_policy, const int *policy_widths, int n_q, const int *q_widths, int act_emb_units,
                       int64_t max_batch, int device) {
    SRLX_REQUIRE(out, "notsac_create: NULL handle pointer");
    *out = nullptr;
    SRLX_TRY(check_shape("notsac_create", obs_dim, head, n_out, n_policy, policy_widths, n_q, q_widths, act_emb_units, max_batch));
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "notsac_create: device %d unavailable", device);
    srlx_notsac *h = new srlx_notsac();
    fill(h, obs_dim, head, n_out, n_policy, policy_widths, n_q, q_widths, act_emb_units, max_batch, device);
    const size_t mb = (size_t)max_batch, plane = mb * h->wmax;
    const size_t blocks = (size_t)(h->blocks_p > h->blocks_q ? h->blocks_p : h->blocks_q);
    hipError_t e = hipMalloc((void **)&h->d_segs, sizeof(Seg) * 2 * kNetTensors);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_net, sizeof(Net));
    if (e == hipSuccess) e = hipMalloc((void **)&h->hp, sizeof(float) * 3 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dhp, sizeof(float) * 3 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->hq, sizeof(float) * 3 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dhq, sizeof(float) * 3 * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->xcat, sizeof(float) * mb * (h->D + h->E));
    if (e == hipSuccess) e = hipMalloc((void **)&h->zact, sizeof(float) * mb * h->E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dact, sizeof(float) * mb * h->E);
    if (e == hipSuccess) e = hipMalloc((void **)&h->ain, sizeof(float) * mb * h->A);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dlast_q, sizeof(float) * mb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dlast_p, sizeof(float) * mb * kHeadCols);
    if (e == hipSuccess) e = hipMalloc((void **)&h->rows, sizeof(float) * 3 * mb);
    if (e == hipSuccess) e = hipMalloc((void **)&h->partials, sizeof(double) * blocks);
    if (e == hipSuccess) e = hipMemset(h->dlast_p, 0, sizeof(float) * mb * kHeadCols);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_notsac_q_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap3);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_notsac_pi_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap3);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_notsac_forward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap3);
    if (e != hipSuccess) {
        srlx_notsac_destroy(h);
        srlx::set_error("notsac_create: device set-up failed: %s", hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    *out = h;
    return SRLX_OK;
}

int srlx_notsac_destroy(srlx_notsac_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (void *p : {(void *)h->d_net, (void *)h->d_segs, (void *)h->hp, (void *)h->dhp, (void *)h->hq, (void *)h->dhq, (void *)h->xcat, (void *)h->zact, (void *)h->dact,
                    (void *)h->ain, (void *)h->dlast_q, (void *)h->dlast_p, (void *)h->rows, (void *)h->partials})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_notsac_bind(srlx_notsac_t *h, int n_tensors, float *const *d_params) {
    SRLX_REQUIRE(h && d_params, "notsac_bind: NULL argument");
    SRLX_REQUIRE(n_tensors == h->ntp + h->ntq, "notsac_bind: %d tensors (this shape has %d policy tensors, then %d Q tensors)", n_tensors, h->ntp, h->ntq);
    return h->ps.bind_params("notsac_bind", n_tensors, d_params);
}

int srlx_notsac_bind_grads(srlx_notsac_t *h, int n_tensors, float *const *d_grads, float *const *d_raw_grads) {
    SRLX_REQUIRE(h && d_grads && d_raw_grads, "notsac_bind_grads: NULL argument");
    SRLX_REQUIRE(n_tensors == h->ntp + h->ntq, "notsac_bind_grads: %d tensors (this shape has %d + %d)", n_tensors, h->ntp, h->ntq);
    return h->ps.bind_grads("notsac_bind_grads", n_tensors, d_grads, d_raw_grads);
}

int srlx_notsac_bind_adam(srlx_notsac_t *h, int n_tensors, float *const *d_exp_avg, float *const *d_exp_avg_sq, int64_t steps_taken, double beta1, double beta2,
                          double eps) {
    SRLX_REQUIRE(h && d_exp_avg && d_exp_avg_sq, "notsac_bind_adam: NULL argument");
    SRLX_REQUIRE(n_tensors == h->ntp + h->ntq, "notsac_bind_adam: %d tensors (this shape has %d + %d)", n_tensors, h->ntp, h->ntq);
    return h->ps.bind_adam("notsac_bind_adam", n_tensors, d_exp_avg, d_exp_avg_sq, steps_taken, beta1, beta2, eps);
}

int srlx_notsac_set_rows_per_workgroup(srlx_notsac_t *h, int rows) {
    SRLX_REQUIRE(h, "notsac_set_rows_per_workgroup: NULL handle");
    SRLX_REQUIRE(rows == 0 || rows == 1 || rows == 2 || rows == 4 || rows == 8 || rows == kRows, "notsac_set_rows_per_workgroup: %d rows (0 for the default, or 1, 2, 4, 8, 16)", rows);
    h->rpw = rows;
    return SRLX_OK;
}

int64_t srlx_notsac_steps(const srlx_notsac_t *h) {
    if (!h) {
        srlx::set_error("notsac_steps: NULL handle");
        return -1;
    }
    return h->ps.steps;
}

int srlx_notsac_forward(srlx_notsac_t *h, int64_t n, const float *d_states, double log_scale_lo, double log_scale_hi, float *d_head0, float *d_head1,
                        const float *d_actions, float *d_q, void *stream) {
    SRLX_REQUIRE(h && d_states, "notsac_forward: NULL handle or states");
    SRLX_REQUIRE(h->ps.bound, "notsac_forward: unbound handle (srlx_notsac_bind)");
    SRLX_REQUIRE(n >= 1 && n <= (int64_t)1 << 24, "notsac_forward: %lld rows (1..2^24)", (long long)n);
    SRLX_REQUIRE(d_head0 || d_q, "notsac_forward: nothing to write");
    SRLX_REQUIRE(!d_head1 || (d_head0 && h->head == 1), "notsac_forward: log-scales go with locs, on a Normal head");
    SRLX_REQUIRE(!(h->head == 1 && d_head0 && !d_head1), "notsac_forward: a Normal head writes locs and log-scales");
    SRLX_REQUIRE((d_q != nullptr) == (d_actions != nullptr), "notsac_forward: q goes with actions");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "notsac_forward: the log-scale clamp's ends are ordered");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    const int rpw = rows_per_workgroup(h, n);
    hipLaunchKernelGGL(k_notsac_forward, dim3((unsigned)((n + rpw - 1) / rpw)), dim3(kThreads), lds_bytes(h), (hipStream_t)stream, (const Net *)h->d_net, (i64)n, d_states,
                       d_actions, d_head0, d_head1, d_q, (float)log_scale_lo, (float)log_scale_hi, rpw, h->D, h->A, h->E, lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_notsac_update(srlx_notsac_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_rewards,
                       const float *d_not_terminated, const float *d_total_rewards, const float *d_noise, double lr, double discount, double loss_align_coeff,
                       double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_q, float *d_target_q, float *d_next_action,
                       float *d_pi_action, float *d_scalars, void *stream) {
    SRLX_REQUIRE(h, "notsac_update: NULL handle");
    SRLX_REQUIRE(h->ps.ready(), "notsac_update: bind the parameters, the gradient tensors and the Adam state first");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "notsac_update: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_rewards && d_not_terminated && d_total_rewards && d_noise && d_q && d_target_q && d_next_action &&
                     d_pi_action && d_scalars,
                 "notsac_update: NULL argument");
    SRLX_REQUIRE(lr >= 0 && max_grad_norm > 0, "notsac_update: lr is non-negative, max_grad_norm positive");
    SRLX_REQUIRE(squashed == 0 || squashed == 1, "notsac_update: squashed is 0 or 1");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "notsac_update: the log-scale clamp's ends are ordered");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    if (!h->ps.table_ok) SRLX_TRY(upload_table(h));
    hipStream_t st = (hipStream_t)stream;
    const double inv_b = 1.0 / (double)batch;
    const Cfg c{(float)discount, (float)loss_align_coeff, (float)log_scale_lo, (float)log_scale_hi, inv_b, squashed};
    const Batch b{(i64)batch, d_states, d_next_states, d_rewards, d_not_terminated, d_total_rewards, h->head ? nullptr : (const int32_t *)d_actions,
                  h->head ? (const float *)d_actions : nullptr, d_noise, d_q, d_target_q, d_next_action, d_pi_action};
    const Work w{h->hp, h->dhp, h->hq, h->dhq, h->xcat, h->zact, h->dact, h->ain, h->dlast_q, h->dlast_p, h->rows, h->max_batch * h->wmax, h->max_batch};
    const RowArgs ra{b, w, c};
    const int rpw = rows_per_workgroup(h, batch);
    const dim3 row_grid((unsigned)((batch + rpw - 1) / rpw));
    const Seg *segs_p = h->d_segs, *segs_q = h->d_segs + kNetTensors;
    // ---- the Q step
    hipLaunchKernelGGL(k_notsac_q_rows, row_grid, dim3(kThreads), lds_bytes(h), st, (const Net *)h->d_net, ra, rpw, h->D, h->A, h->E, lds_stride(h));
    const GradArgs gq{segs_q, h->ntq, d_states, h->partials, LossSums{2, (i64)batch, h->rows, h->max_batch, inv_b, d_scalars}};
    hipLaunchKernelGGL(k_notsac_grad, dim3((unsigned)h->blocks_q), dim3(kThreads), 0, st, gq);
    const srlxt::StepArgs sq = h->ps.step_args(segs_q, h->ntq, h->partials, h->blocks_q, max_grad_norm, lr, d_scalars + 3);
    hipLaunchKernelGGL(k_notsac_step, dim3((unsigned)((h->elements_q + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sq);
    // ---- the policy step, through the Q-network as it stands now
    hipLaunchKernelGGL(k_notsac_pi_rows, row_grid, dim3(kThreads), lds_bytes(h), st, (const Net *)h->d_net, ra, rpw, h->D, h->A, h->E, lds_stride(h));
    const GradArgs gp{segs_p, h->ntp, d_states, h->partials, LossSums{1, (i64)batch, h->rows + 2 * h->max_batch, h->max_batch, -inv_b, d_scalars + 2}};
    hipLaunchKernelGGL(k_notsac_grad, dim3((unsigned)h->blocks_p), dim3(kThreads), 0, st, gp);
    const srlxt::StepArgs sp = h->ps.step_args(segs_p, h->ntp, h->partials, h->blocks_p, max_grad_norm, lr, d_scalars + 4);
    hipLaunchKernelGGL(k_notsac_step, dim3((unsigned)((h->elements_p + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sp);
    SRLX_HIP(hipGetLastError());
    h->ps.steps++;
    return SRLX_OK;
}

}  // extern "C"
