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
//   k_mlp_walk        (srlx_mlp_walk.h) the head's outputs for the plugin's acting: 16 rows per workgroup through the policy on the float64
//                     matrix cores, the activations in LDS
// One update: q_rows, grad (Q), step (Q), pi_rows, grad (policy), step (policy); the stream orders them and nothing synchronises the host.
// LDS: three row buffers of 16 x (widest row + 1) floats (the act_block's pre-activations have to outlive q_block's chains) and the 32 KB weight tile:
// 131 264 bytes at a widest row of 512 -- the concatenated row of D + E floats is held to that.
// No atomics and a fixed order in every sum: equal inputs give equal bits.
//
// srlx_notsac_update_gemm is the same update layer by layer: every Linear of both networks over the whole batch as one job of srlx_mlp_gemm.h's
// tile on the float64 matrix cores, jobs of equal depth in one launch, and between those launches
//   k_notsac_gemm_action     one thread per row (Gumbel) or per row and element (Normal): the action from the head rows and one noise plane, act_block's input rows
//   k_notsac_gemm_embed      one thread per (row set, row, column of the concatenated row): the state copied, act_block's Linear (A <= 16 terms) and SiLU
//   k_notsac_gemm_q_loss     one thread per row: the target, the Huber and MSE terms, the seed d loss / d q
//   k_notsac_gemm_bwd        srlx_mlp_gemm.h's backward tile with NoT_SAC's three epilogues: the ReLU mask, the SiLU derivative behind a column range of
//                            q_block's first weight, none (d loss / d action)
//   k_notsac_gemm_head_grad  one thread per row or per row and element: the head's Jacobian
// with k_notsac_grad and k_notsac_step as the tail of each half.  upload_gemm builds these steps on srlxg::Plan, the handle keeps them in a srlxg::GemmPath
//  and update walks them; GemmScratch is the one statement of the path's scratch layout.
#include "srlx_mlp_gemm.h"
#include "srlx_mlp_walk.h"
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

// The gemm path's plan (srlxg::Plan): a list of steps, each a launch of jobs from the device table (srlxg::kFwd; srlxg::kBwd, here through
// k_notsac_gemm_bwd) or one of the pointwise kernels between them.
enum StepKind { kNextAction = srlxg::kBwd + 1, kEmbedBoth, kQLoss, kTailQ, kPiAction, kEmbedOne, kHeadGrad, kTailP };
constexpr int kGemmSteps = 40;  // target half: 3 + 1 policy, 2 pointwise, 3 + 1 Q, 1 pointwise, 3 + 1 backward, the tail; policy half: 20
constexpr int kGemmJobs = 40;   // target half: 3 + 2, 2 x (3 + 1), 3 + 1; policy half: 3 + 2, 3 + 1, 3 + 1 + 1, 3
enum Epilogue { kEpiRelu = 0, kEpiSilu = 1, kEpiNone = 2 };  // of a k_notsac_gemm_bwd job, in Job::relu

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
    // srlx_notsac_update_gemm's own, allocated at its first call; scratch: GemmScratch
    srlxg::GemmPath<kGemmJobs, kGemmSteps> path;
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

// ---- the gemm path's own kernels (srlx_notsac_update_gemm).  The closed forms are the lines the row kernels run, on the same float32 values.

// The backward tile of srlx_mlp_gemm.h with the epilogue the job names in Job::relu:
//   kEpiRelu  dH = H > 0 ? sum : 0, H = aux [M][N] (k_mlp_gemm_bwd's)
//   kEpiSilu  the columns c0..N-1 of the weight only (q_block's first [H][D + E] matrix from its embedding column on: the tile starts at column c0 of the whole
//             matrix, so the row stride stays N and nothing below c0 is computed): d z = (float)(sum * silu_grad(z)), z = aux [M][N - c0], as q_backward
//   kEpiNone  the rounded sum (d loss / d action through act_block's weight)
// grid (column tiles of the launch's widest output, row tiles, jobs).
SRLXG_KERNEL void __launch_bounds__(srlxg::kThreads) k_notsac_gemm_bwd(const srlxg::Job *__restrict__ jobs, int M, int c0) {
    using namespace srlxg;
    __shared__ __attribute__((aligned(16))) float As[2 * kTile * kLdK], Bs[2 * kChunk * kLdN];
    const Job &job = jobs[blockIdx.z];
    const int epi = job.relu, first = epi == kEpiSilu ? c0 : 0, width = job.N - first;
    const int n0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile;
    if (n0 >= width) return;
    const f64x4 acc = tile_sums<true>(job, M, m0, first + n0, nullptr, nullptr, As, Bs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = n0 + (wave & 1) * 16 + (lane & 15);
    if (col >= width) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = m0 + (wave >> 1) * 16 + 4 * r + (lane >> 4);
        if (row >= M) continue;
        float g = (float)acc[r];
        if (epi == kEpiRelu) g = job.aux[(i64)row * width + col] > 0.f ? g : 0.f;
        else if (epi == kEpiSilu) g = (float)(acc[r] * srlxn::silu_grad(job.aux[(i64)row * width + col]));
        job.y[(i64)row * job.ldy + col] = g;
    }
}

constexpr int kRowThreads = 64;  // of the one-thread-per-row kernels

// One row set of k_notsac_gemm_embed: states [B][D] and actions [B][A] in, the concatenated rows [B][D + E] and (NULL: not kept) act_block's pre-activations out
struct EmbedSet {
    const float *s, *act;
    float *xcat, *zact;
};

// q_block's input rows: one thread per (row set, row, column).  Columns below D copy the state; column D + j is SiLU of act_block's Linear, an A-term float64
// chain in dense<double>'s order, rounded once.  blockIdx.y: the row set (the target half runs (s, a) and (s', a') in one launch).
SRLXG_KERNEL void __launch_bounds__(kThreads) k_notsac_gemm_embed(EmbedSet s0, EmbedSet s1, i64 B, const float *__restrict__ wa, const float *__restrict__ ba, int D, int A,
                                                                  int E) {
    const int W = D + E;
    const i64 p = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (p >= B * W) return;
    const bool second = blockIdx.y != 0;
    const float *s = second ? s1.s : s0.s, *act = second ? s1.act : s0.act;
    float *xcat = second ? s1.xcat : s0.xcat, *zact = second ? s1.zact : s0.zact;
    const i64 r = p / W;
    const int k = (int)(p % W);
    if (k < D) {
        xcat[p] = s[r * D + k];
        return;
    }
    const int j = k - D;
    double acc = 0.0;
    for (int i = 0; i < A; i++) acc = srlxm::fma_acc((double)wa[j * A + i], (double)act[r * A + i], acc);
    const float z = (float)(acc + (double)ba[j]);
    if (zact) zact[r * E + j] = z;
    xcat[p] = srlxn::silu(z);
}

// The action of every row from its head row `z` [B][kHeadCols] and one noise plane, and act_block's input rows `ain`.
//   half 0 (the target): a' = normal_action / the one-hot of gumbel_argmax into `out` (next_action); `ain` takes the STORED actions
//   half 1 (the policy): a = normal_action / gumbel_softmax into `out` (pi_action) and `ain`; dlast_q takes the seed -1 / B of q(s, pi(s))
// One thread per row and element (Normal) or per row (Gumbel).
struct ActionArgs {
    i64 B;
    const float *z, *noise;
    float *out, *ain, *dlast_q;
    const int32_t *action_i;
    const float *action_f;
    float ls_lo, ls_hi, seed;
    int squashed, A, normal, half;
};
SRLXG_KERNEL void __launch_bounds__(kRowThreads) k_notsac_gemm_action(ActionArgs a) {
    const i64 p = (i64)blockIdx.x * kRowThreads + threadIdx.x;
    const int A = a.A;
    if (a.normal) {
        if (p >= a.B * A) return;
        const i64 r = p / A;
        const int j = (int)(p % A);
        const float x = srlxn::normal_action(a.z[r * kHeadCols + j], a.z[r * kHeadCols + kNormalLs + j], a.ls_lo, a.ls_hi, a.noise[p], a.squashed);
        a.out[p] = x;
        a.ain[p] = a.half ? x : a.action_f[p];
        if (a.half && j == 0) a.dlast_q[r] = a.seed;
        return;
    }
    if (p >= a.B) return;
    if (a.half) {
        srlxn::gumbel_softmax(a.z + p * kHeadCols, a.noise + p * A, A, a.out + p * A);
        for (int k = 0; k < A; k++) a.ain[p * A + k] = a.out[p * A + k];
        a.dlast_q[p] = a.seed;
    } else {
        const int best = srlxn::gumbel_argmax(a.z + p * kHeadCols, a.noise + p * A, A);
        const int act = a.action_i[p];
        const int ac = act < 0 ? 0 : (act >= A ? A - 1 : act);
        for (int k = 0; k < A; k++) a.out[p * A + k] = k == best ? 1.f : 0.f, a.ain[p * A + k] = k == ac ? 1.f : 0.f;
    }
}

// The Q step's rows: `qv` [2][max_batch] holds q(s', a') and q(s, a)
SRLXG_KERNEL void __launch_bounds__(kRowThreads) k_notsac_gemm_q_loss(Batch a, const float *__restrict__ qv, float *__restrict__ rows, float *__restrict__ dlast_q,
                                                                     i64 max_batch, Cfg c) {
    const i64 b = (i64)blockIdx.x * kRowThreads + threadIdx.x;
    if (b >= a.B) return;
    const float qn = qv[b], q = qv[max_batch + b];
    const srlxn::QRow r = srlxn::q_row(q, qn, a.reward[b], a.not_term[b], a.total_reward[b], c.discount, c.coeff, c.inv_b);
    a.q[b] = q, a.target[b] = r.target;
    rows[b] = r.huber, rows[max_batch + b] = r.align;
    dlast_q[b] = r.dq;
}

// d loss / d (head outputs) from d loss / d action `ga` [B][kHeadCols], the actions `act` [B][A] they belong to, the head rows and noise plane 1.  The columns of
// dlast_p no head writes stay the zeros srlx_notsac_create left.
SRLXG_KERNEL void __launch_bounds__(kRowThreads) k_notsac_gemm_head_grad(i64 B, const float *__restrict__ ga, const float *__restrict__ act, const float *__restrict__ z,
                                                                        const float *__restrict__ noise, float *__restrict__ dlast_p, float ls_lo, float ls_hi,
                                                                        int squashed, int A, int normal) {
    const i64 p = (i64)blockIdx.x * kRowThreads + threadIdx.x;
    if (normal) {
        if (p >= B * A) return;
        const i64 r = p / A;
        const int j = (int)(p % A);
        float dloc, dls;
        srlxn::normal_action_grad(ga[r * kHeadCols + j], act[p], z[r * kHeadCols + kNormalLs + j], ls_lo, ls_hi, noise[p], squashed, dloc, dls);
        dlast_p[r * kHeadCols + j] = dloc, dlast_p[r * kHeadCols + kNormalLs + j] = dls;
        return;
    }
    if (p >= B) return;
    srlxn::softmax_grad(act + p * A, ga + p * kHeadCols, A, dlast_p + p * kHeadCols);
}

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
    h->path.ok = false;  // (whatever made this table stale made the gemm path's jobs stale)
    return SRLX_OK;
}

// the gemm path's scratch: upload_gemm and update share this layout
struct GemmScratch {
    float *sp[2];  // two planes [max_batch][wmax]: the layers nothing keeps, in turn
    float *xcat2;  // [max_batch][D + E]: the s' rows of xcat
    float *z, *ga; // [max_batch][kHeadCols] each: the head rows and d loss / d action
    float *qv;     // [2][max_batch]: q(s', a') and q(s, a)
    static size_t floats(const srlx_notsac *h) {
        const size_t mb = (size_t)h->max_batch;
        return 2 * mb * h->wmax + mb * (h->D + h->E) + 2 * mb * kHeadCols + 2 * mb;
    }
    GemmScratch(const srlx_notsac *h) {
        const i64 mb = h->max_batch, plane = mb * h->wmax;
        float *g = h->path.scratch;
        sp[0] = g, sp[1] = g + plane, xcat2 = g + 2 * plane, z = xcat2 + mb * (h->D + h->E), ga = z + mb * kHeadCols, qv = ga + mb * kHeadCols;
    }
};

// The gemm path's plan: every Linear with a reduction length worth a tile is one job, jobs of equal depth share a launch, the pointwise kernels
// stand between them.  The planes, and the layout upload_table hands to the tail, are the row path's; what the row path keeps in LDS only (the s' rows, the
// head rows, d loss / d action) goes through the path's own scratch, allocated at its first call.
int upload_gemm(const char *who, srlx_notsac *h) {
    using srlxg::Job;
    const i64 mb = h->max_batch, plane = mb * h->wmax;
    const int D = h->D, A = h->A, E = h->E, Lp = h->Lp, Lq = h->Lq, W = D + E;
    SRLX_TRY(h->path.ensure(GemmScratch::floats(h)));
    const GemmScratch sc(h);
    float *const *sp = sc.sp, *xcat2 = sc.xcat2, *z = sc.z, *ga = sc.ga, *qv = sc.qv;
    auto &p = h->path.plan;
    p.clear();
    float *const *P = h->ps.p, *const *Q = h->ps.p + h->ntp;  // Q: act_block, q_block's layers, q_out
    auto fwd = [&](const float *x, int sel, int K, float *const *lin, int N, float *y, int ldy, int relu) { p.fwd(x, sel, K, lin[0], lin[1], K, N, y, ldy, relu); };
    // the policy's hidden layers and head on the rows of launch argument `sel`: kept in hp's planes, or through the two scratch planes in turn
    auto plan_policy = [&](int sel, bool keep) {
        const float *x = nullptr;
        int in = D;
        for (int l = 0; l < Lp; in = h->Wp[l], l++) {
            float *y = keep ? h->hp + l * plane : sp[l & 1];
            p.begin(srlxg::kFwd);
            fwd(x, l ? srlxg::kFromJob : sel, in, P + 2 * l, h->Wp[l], y, h->Wp[l], 1);
            p.end();
            x = y;
        }
        p.begin(srlxg::kFwd);
        fwd(x, 0, in, P + 2 * Lp, A, z, kHeadCols, 0);
        if (h->head) fwd(x, 0, in, P + 2 * (Lp + 1), A, z + kNormalLs, kHeadCols, 0);
        p.end();
    };
    // q_block and q_out on the kept rows (xcat -> hq's planes -> q_kept) and, `both`, on the s' rows (xcat2 -> the scratch planes -> qv[0])
    auto plan_q = [&](bool both, float *q_kept) {
        const float *x = h->xcat, *x2 = xcat2;
        int in = W;
        for (int l = 0; l < Lq; in = h->Wq[l], l++) {
            p.begin(srlxg::kFwd);
            fwd(x, 0, in, Q + 2 + 2 * l, h->Wq[l], h->hq + l * plane, h->Wq[l], 1);
            if (both) fwd(x2, 0, in, Q + 2 + 2 * l, h->Wq[l], sp[l & 1], h->Wq[l], 1);
            p.end();
            x = h->hq + l * plane, x2 = sp[l & 1];
        }
        p.begin(srlxg::kFwd);
        fwd(x, 0, in, Q + 2 + 2 * Lq, 1, q_kept, 1, 0);
        if (both) fwd(x2, 0, in, Q + 2 + 2 * Lq, 1, qv, 1, 0);
        p.end();
    };
    // from dlast_q down q_block (the masks of hq's planes, into dhq's), then through the embedding columns of its first weight and the SiLU derivative into dact
    auto plan_q_back = [&]() {
        for (int l = Lq - 1; l >= 0; l--) {
            p.begin(srlxg::kBwd);
            Job &j = p.bwd(h->dhq + l * plane, h->Wq[l], h->hq + l * plane, h->Wq[l], h->Wq[l], kEpiRelu);
            if (l == Lq - 1) p.src(j, h->dlast_q, 1, 1, Q[2 + 2 * Lq]);
            else p.src(j, h->dhq + (l + 1) * plane, h->Wq[l + 1], h->Wq[l + 1], Q[2 + 2 * (l + 1)]);
            p.end();
        }
        p.begin(srlxg::kBwd);
        p.src(p.bwd(h->dact, E, h->zact, W, E, kEpiSilu), h->dhq, h->Wq[0], h->Wq[0], Q[2]);
        p.end();
    };
    // ---- the target half and the Q step
    plan_policy(srlxg::kArg1, false);
    p.point(kNextAction);
    p.point(kEmbedBoth);
    plan_q(true, qv + mb);
    p.point(kQLoss);
    plan_q_back();
    p.point(kTailQ);
    // ---- the policy half, through the Q-network as it stands now: its planes, xcat, zact and dact are free again
    plan_policy(srlxg::kArg0, true);
    p.point(kPiAction);
    p.point(kEmbedOne);
    plan_q(false, h->rows + 2 * mb);
    plan_q_back();
    p.begin(srlxg::kBwd);
    p.src(p.bwd(ga, kHeadCols, nullptr, A, A, kEpiNone), h->dact, E, E, Q[0]);
    p.end();
    p.point(kHeadGrad);
    for (int l = Lp - 1; l >= 0; l--) {
        p.begin(srlxg::kBwd);
        Job &j = p.bwd(h->dhp + l * plane, h->Wp[l], h->hp + l * plane, h->Wp[l], h->Wp[l], kEpiRelu);
        if (l < Lp - 1) {
            p.src(j, h->dhp + (l + 1) * plane, h->Wp[l + 1], h->Wp[l + 1], P[2 * (l + 1)]);
        } else {
            p.src(j, h->dlast_p, kHeadCols, A, P[2 * Lp]);  // SumSeed's order: the head, then the log-scale head
            if (h->head) p.src(j, h->dlast_p + kNormalLs, kHeadCols, A, P[2 * (Lp + 1)]);
        }
        p.end();
    }
    p.point(kTailP);
    return h->path.upload(who);  // (at most 16 + 20 steps and 17 + 17 jobs, at three layers everywhere and a Normal head)
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

// srlx_notsac_update (gemm = false: the two row kernels) and srlx_notsac_update_gemm (upload_gemm's plan): one contract, one set of planes, one gradient, clip
// and Adam tail behind each half.  `who` names the entry point in every message.
int update(const char *who, bool gemm, srlx_notsac *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_rewards,
           const float *d_not_terminated, const float *d_total_rewards, const float *d_noise, double lr, double discount, double loss_align_coeff, double max_grad_norm,
           int squashed, double log_scale_lo, double log_scale_hi, float *d_q, float *d_target_q, float *d_next_action, float *d_pi_action, float *d_scalars,
           void *stream) {
    SRLX_REQUIRE(h, "%s: NULL handle", who);
    SRLX_REQUIRE(h->ps.ready(), "%s: bind the parameters, the gradient tensors and the Adam state first", who);
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "%s: batch %lld (handle sized for %lld)", who, (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_rewards && d_not_terminated && d_total_rewards && d_noise && d_q && d_target_q && d_next_action &&
                     d_pi_action && d_scalars,
                 "%s: NULL argument", who);
    SRLX_REQUIRE(lr >= 0 && max_grad_norm > 0, "%s: lr is non-negative, max_grad_norm positive", who);
    SRLX_REQUIRE(squashed == 0 || squashed == 1, "%s: squashed is 0 or 1", who);
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "%s: the log-scale clamp's ends are ordered", who);
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    if (!h->ps.table_ok) SRLX_TRY(upload_table(h));
    if (gemm && !h->path.ok) SRLX_TRY(upload_gemm(who, h));
    hipStream_t st = (hipStream_t)stream;
    const double inv_b = 1.0 / (double)batch;
    const Cfg c{(float)discount, (float)loss_align_coeff, (float)log_scale_lo, (float)log_scale_hi, inv_b, squashed};
    const Batch b{(i64)batch, d_states, d_next_states, d_rewards, d_not_terminated, d_total_rewards, h->head ? nullptr : (const int32_t *)d_actions,
                  h->head ? (const float *)d_actions : nullptr, d_noise, d_q, d_target_q, d_next_action, d_pi_action};
    const Seg *segs_p = h->d_segs, *segs_q = h->d_segs + kNetTensors;
    // the tail of each half: the network's gradient before the clip with its loss sums, then the norm, the clip and Adam
    auto tail_q = [&]() {
        const GradArgs gq{segs_q, h->ntq, d_states, h->partials, LossSums{2, (i64)batch, h->rows, h->max_batch, inv_b, d_scalars}};
        hipLaunchKernelGGL(k_notsac_grad, dim3((unsigned)h->blocks_q), dim3(kThreads), 0, st, gq);
        const srlxt::StepArgs sq = h->ps.step_args(segs_q, h->ntq, h->partials, h->blocks_q, max_grad_norm, lr, d_scalars + 3);
        hipLaunchKernelGGL(k_notsac_step, dim3((unsigned)((h->elements_q + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sq);
    };
    auto tail_p = [&]() {
        const GradArgs gp{segs_p, h->ntp, d_states, h->partials, LossSums{1, (i64)batch, h->rows + 2 * h->max_batch, h->max_batch, -inv_b, d_scalars + 2}};
        hipLaunchKernelGGL(k_notsac_grad, dim3((unsigned)h->blocks_p), dim3(kThreads), 0, st, gp);
        const srlxt::StepArgs sp = h->ps.step_args(segs_p, h->ntp, h->partials, h->blocks_p, max_grad_norm, lr, d_scalars + 4);
        hipLaunchKernelGGL(k_notsac_step, dim3((unsigned)((h->elements_p + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sp);
    };
    if (!gemm) {
        const Work w{h->hp, h->dhp, h->hq, h->dhq, h->xcat, h->zact, h->dact, h->ain, h->dlast_q, h->dlast_p, h->rows, h->max_batch * h->wmax, h->max_batch};
        const RowArgs ra{b, w, c};
        const int rpw = rows_per_workgroup(h, batch);
        const dim3 row_grid((unsigned)((batch + rpw - 1) / rpw));
        // ---- the Q step
        hipLaunchKernelGGL(k_notsac_q_rows, row_grid, dim3(kThreads), lds_bytes(h), st, (const Net *)h->d_net, ra, rpw, h->D, h->A, h->E, lds_stride(h));
        tail_q();
        // ---- the policy step, through the Q-network as it stands now
        hipLaunchKernelGGL(k_notsac_pi_rows, row_grid, dim3(kThreads), lds_bytes(h), st, (const Net *)h->d_net, ra, rpw, h->D, h->A, h->E, lds_stride(h));
        tail_p();
    } else {
        const i64 mb = h->max_batch;
        const int D = h->D, A = h->A, E = h->E, W = D + E, M = (int)batch;
        const GemmScratch sc(h);
        float *xcat2 = sc.xcat2, *z = sc.z, *ga = sc.ga, *qv = sc.qv;
        const float *wa = h->ps.p[h->ntp], *ba = h->ps.p[h->ntp + 1];
        const i64 heads = h->head ? batch * A : batch;  // threads of the kernels that run one per row and element (Normal) or per row (Gumbel)
        const dim3 head_grid((unsigned)((heads + kRowThreads - 1) / kRowThreads)), row_grid((unsigned)((batch + kRowThreads - 1) / kRowThreads));
        const unsigned embed_blocks = (unsigned)((batch * W + kThreads - 1) / kThreads);
        const EmbedSet kept{d_states, h->ain, h->xcat, h->zact}, next{d_next_states, d_next_action, xcat2, nullptr};
        for (int i = 0; i < h->path.plan.ns; i++) {
            const srlxg::Step &s = h->path.plan.steps[i];
            const srlxg::Grid gr = srlxg::grid_of(s.l, M);
            switch (s.kind) {
            case srlxg::kFwd:
                srlxg::launch(s.l, h->path.d_jobs, M, d_states, d_next_states, st);
                break;
            case srlxg::kBwd:
                hipLaunchKernelGGL(k_notsac_gemm_bwd, dim3((unsigned)gr.x, (unsigned)gr.y, (unsigned)gr.z), dim3(srlxg::kThreads), 0, st,
                                   (const srlxg::Job *)h->path.d_jobs + s.l.first, M, D);
                break;
            case kNextAction:
                hipLaunchKernelGGL(k_notsac_gemm_action, head_grid, dim3(kRowThreads), 0, st,
                                   ActionArgs{(i64)batch, z, d_noise, d_next_action, h->ain, h->dlast_q, b.action_i, b.action_f, c.ls_lo, c.ls_hi, 0.f, squashed, A, h->head, 0});
                break;
            case kPiAction:
                hipLaunchKernelGGL(k_notsac_gemm_action, head_grid, dim3(kRowThreads), 0, st,
                                   ActionArgs{(i64)batch, z, d_noise + batch * A, d_pi_action, h->ain, h->dlast_q, nullptr, nullptr, c.ls_lo, c.ls_hi, (float)(-inv_b),
                                              squashed, A, h->head, 1});
                break;
            case kEmbedBoth:
            case kEmbedOne:
                hipLaunchKernelGGL(k_notsac_gemm_embed, dim3(embed_blocks, s.kind == kEmbedBoth ? 2u : 1u), dim3(kThreads), 0, st, kept, next, (i64)batch, wa, ba, D, A, E);
                break;
            case kQLoss:
                hipLaunchKernelGGL(k_notsac_gemm_q_loss, row_grid, dim3(kRowThreads), 0, st, b, (const float *)qv, h->rows, h->dlast_q, mb, c);
                break;
            case kHeadGrad:
                hipLaunchKernelGGL(k_notsac_gemm_head_grad, head_grid, dim3(kRowThreads), 0, st, (i64)batch, (const float *)ga, (const float *)d_pi_action, (const float *)z,
                                   d_noise + batch * A, h->dlast_p, c.ls_lo, c.ls_hi, squashed, A, h->head);
                break;
            case kTailQ:
                tail_q();
                break;
            case kTailP:
                tail_p();
                break;
            }
        }
    }
    SRLX_HIP(hipGetLastError());
    h->ps.steps++;
    return SRLX_OK;
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
    if (e == hipSuccess) e = srlxw::raise_lds_limit();
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
    h->path.release();
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

int srlx_notsac_walk(srlx_notsac_t *h, int64_t n_rows, const float *d_states, double log_scale_lo, double log_scale_hi, float *d_head0, float *d_head1,
                     void *stream) {
    SRLX_REQUIRE(n_rows >= 1 && n_rows <= srlxw::kMaxRows, "notsac_walk: n_rows %lld (1..%lld)", (long long)n_rows, (long long)srlxw::kMaxRows);
    SRLX_REQUIRE(h, "notsac_walk: NULL handle");
    SRLX_REQUIRE(h->ps.bound, "notsac_walk: bind the parameters first (srlx_notsac_bind)");
    SRLX_REQUIRE(d_states && d_head0, "notsac_walk: NULL d_states or d_head0");
    SRLX_REQUIRE((d_head1 != nullptr) == (h->head == 1), "notsac_walk: d_head1 takes the log-scales of a Normal head and is NULL on a Gumbel one");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "notsac_walk: the log-scale clamp's ends are ordered");
    // the policy alone, layer by layer; its head in the kernel's last round
    float *const *P = h->ps.p;
    srlxw::WalkPlan w;
    int v = 0, K = h->D;
    for (int l = 0; l < h->Lp; K = h->Wp[l], l++) v = w.pass(v, K, P[2 * l], P[2 * l + 1], h->Wp[l]);
    float *const *hd = P + 2 * h->Lp;
    w.dist_head(v, K, h->A, hd[0], hd[1], h->head ? hd[2] : nullptr, h->head ? hd[3] : nullptr);
    SRLX_REQUIRE(w.finish(h->D), "notsac_walk: the network's planes do not fit the kernel's LDS");
    srlx::DeviceGuard g(h->device);
    srlxw::launch(w, n_rows, d_states, (float)log_scale_lo, (float)log_scale_hi, nullptr, d_head0, d_head1, (hipStream_t)stream);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_notsac_update(srlx_notsac_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_rewards,
                       const float *d_not_terminated, const float *d_total_rewards, const float *d_noise, double lr, double discount, double loss_align_coeff,
                       double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_q, float *d_target_q, float *d_next_action,
                       float *d_pi_action, float *d_scalars, void *stream) {
    return update("notsac_update", false, h, batch, d_states, d_next_states, d_actions, d_rewards, d_not_terminated, d_total_rewards, d_noise, lr, discount,
                  loss_align_coeff, max_grad_norm, squashed, log_scale_lo, log_scale_hi, d_q, d_target_q, d_next_action, d_pi_action, d_scalars, stream);
}

int srlx_notsac_update_gemm(srlx_notsac_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_rewards,
                            const float *d_not_terminated, const float *d_total_rewards, const float *d_noise, double lr, double discount, double loss_align_coeff,
                            double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_q, float *d_target_q, float *d_next_action,
                            float *d_pi_action, float *d_scalars, void *stream) {
    return update("notsac_update_gemm", true, h, batch, d_states, d_next_states, d_actions, d_rewards, d_not_terminated, d_total_rewards, d_noise, lr, discount,
                  loss_align_coeff, max_grad_norm, squashed, log_scale_lo, log_scale_hi, d_q, d_target_q, d_next_action, d_pi_action, d_scalars, stream);
}

}  // extern "C"
