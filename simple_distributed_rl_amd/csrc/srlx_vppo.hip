// srlx_vppo.hip -- the whole update of V-PPO (srl/algorithms/ppo_v/torch_model.py:111-178) on flat observations in three launches, and a forward-only pass.
// One actor-critic MLP: a trunk (input value block + hidden block, 1..3 ReLU layers), a value branch (0..2 ReLU layers + Linear(1)) and a policy branch
// (0..2 ReLU layers + the head: Linear(A) logits, or Linear(k) locs and Linear(k) log-scales).  The arithmetic contract is DESIGN.md 7o and include/srlx.h; its
// per-row closed forms are srlx_vppo_math.h.
//
// The work is srlx_sacd.hip's, not a GEMM's (<= 256 rows through <= 8 layers of <= 512 units), and so is the shape: 256 threads over <= 16 rows, each layer's
// weight staged through LDS in tiles of whole rows (srlx_mlp_rows.h with float64 accumulators), hidden rows and their gradients kept in per-layer planes.
//   k_vppo_rows     16 rows per workgroup: v(s'), then trunk, value branch and policy branch of s with the hidden rows kept, the row's losses and seeds
//                   (the means are known factors 1 / (B K): no cross-row reduction), then the backward chains of both branches and of the trunk, whose
//                   top layer sums what the two branches send down
//   k_vppo_grad     one thread per parameter: the gradient before the clip, a sum over the batch in row order; every workgroup leaves the sum of its squares;
//                   the last four threads of the launch reduce the four losses
//   k_vppo_step     every workgroup sums the same partial squares in the same order (the norm), then one thread per parameter: the clipped gradient and Adam
//   k_vppo_forward  v and the head's outputs of n rows
//   k_vppo_act      the Worker's policy() for the lanes of a device engine: trunk and policy branch of up to 16 rows per workgroup, keyed uniforms, the action and
//                   its log-probability (two row buffers, 98 432 bytes of LDS at most)
//   k_vppo_act_normal  the same on the Normal head: Box-Muller on keyed uniforms, the action before tanh, every element's log-probability, the environment's
//                   action (the same two row buffers)
// LDS: three row buffers of 16 x (widest row + 1) floats (the trunk's output has to outlive the value branch) and the 32 KB weight tile: 131 264 bytes at
// widths of 512, one workgroup per compute unit, which is all these launches (<= 16 workgroups) ask for.
// No atomics and a fixed order in every sum: equal inputs give equal bits.
#include "srlx_param_tail.h"
#include "srlx_vppo_math.h"
#include <cmath>

namespace {

using i64 = int64_t;

using srlxm::kRows;
using srlxm::kThreads;
using srlxm::Layers;
using srlxm::Src;
using srlxm::SumSeed;
using srlxt::kMaxTensors;  // 2 x (3 trunk + 2 value + value_out + 2 policy + 2 heads)
using srlxt::Seg;
using srlxv::kHeadCols;
using srlxv::kNormalLs;
constexpr int kPlanes = 7;  // trunk 0..2, value 3..4, policy 5..6

struct Net {  // the three chains as the kernels read them; the Normal head's second Linear beside the policy chain (NULL: categorical)
    Layers trunk, value, policy;
    const float *w_ls, *b_ls;
};

}  // namespace

struct srlx_vppo {
    int D, head, A, Lt, Lv, Lp, device;  // head 0: categorical with A actions; 1: Normal with A = k elements
    int Wt[3], Wv[2], Wp[2];
    int wmax, nt;
    int wmax_act;  // max(D, trunk widths, policy widths): k_vppo_act's rows
    i64 max_batch, elements, grad_blocks;
    srlxt::ParamSet ps;
    Net *d_net;  // (in device memory: a by-value kernel argument of this size was copied to scratch)
    Seg *d_segs;
    float *h, *dh;    // planes [kPlanes][max_batch][wmax]
    float *dlast_v;   // [max_batch]: d loss / d v
    float *dlast_p;   // [max_batch][kHeadCols]: d loss / d (head outputs)
    float *rows;      // [4][max_batch]: the rows' loss sums
    double *partials; // [grad_blocks]: sums of squared gradients
};

namespace {

int n_tensors(const srlx_vppo *h) { return 2 * (h->Lt + h->Lv + 1 + h->Lp + (h->head ? 2 : 1)); }
int lds_stride(const srlx_vppo *h) { return h->wmax + 1; }
size_t lds_bytes(const srlx_vppo *h) { return srlxt::row_lds_bytes(3, h->wmax); }
int act_lds_stride(const srlx_vppo *h) { return h->wmax_act + 1; }
size_t act_lds_bytes(const srlx_vppo *h) { return srlxt::row_lds_bytes(2, h->wmax_act); }

struct Keep {  // planes of the hidden rows (NULL: not kept)
    float *ht, *hv, *hp;
    i64 plane;
};

// v (and, with `policy`, the head's outputs) of rows i0..i0+nb-1 of `states`: vs[r]; zs[r][kHeadCols] = logits, or locs at 0.. and RAW log-scales at kNormalLs...
// The same chains whatever rows share the workgroup and whether the policy is asked for: k_vppo_forward and k_vppo_rows give the same bits.  Begins and ends
// behind a barrier.
__device__ __forceinline__ void forward_heads(const Net &n, const float *__restrict__ states, i64 i0, int nb, int D, float *b0, float *b1, float *b2, int S, float *wl,
                                              Keep kp, bool policy, float *vs, float *zs) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int p = t; p < nb * D; p += kThreads) b0[(p / D) * S + p % D] = states[(i0 + p / D) * D + p % D];
    __syncthreads();
    float *T = srlxm::forward_rows<double>(n.trunk, n.trunk.L, nb, b0, b1, S, wl, kp.ht, kp.plane, i0, kp.ht ? nb : 0);
    const int Wtop = n.trunk.width(n.trunk.L - 1);
    if (policy)
        for (int p = t; p < nb * Wtop; p += kThreads) b2[(p / Wtop) * S + p % Wtop] = T[(p / Wtop) * S + p % Wtop];
    const float *vo = srlxm::forward_rows<double>(n.value, n.value.L + 1, nb, T, T == b0 ? b1 : b0, S, wl, kp.hv, kp.plane, i0, kp.hv ? nb : 0);
    if (t < nb) vs[t] = vo[t * S];
    __syncthreads();
    if (!policy) return;
    for (int p = t; p < nb * Wtop; p += kThreads) b0[(p / Wtop) * S + p % Wtop] = b2[(p / Wtop) * S + p % Wtop];
    __syncthreads();
    const float *z = srlxm::forward_rows<double>(n.policy, n.policy.L + 1, nb, b0, b1, S, wl, kp.hp, kp.plane, i0, kp.hp ? nb : 0);
    srlxm::head_rows(n.policy, n.w_ls, n.b_ls, nb, z, z == b0 ? b1 : b0, b2, S, wl, zs);
}

struct Batch {
    i64 B;
    const float *s, *s2, *old_lp, *reward, *not_term, *total_reward;
    const int32_t *action_i;  // categorical
    const float *action_f;    // Normal
    float *v, *n_v, *new_lp;
};

struct Work {
    float *h, *dh, *dlast_v, *dlast_p, *rows;
    i64 plane, max_batch;
};

__global__ void __launch_bounds__(kThreads) k_vppo_rows(const Net *__restrict__ net, Batch a, Work w, srlxv::Cfg c, int D, int K, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *b2 = sm + 2 * kRows * S, *wl = sm + 3 * kRows * S;
    __shared__ float vs[kRows], nvs[kRows], zs[kRows * kHeadCols], dzs[kRows * kHeadCols];
    const Net &n = *net;
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * kRows;
    const int nb = (int)(a.B - i0 < kRows ? a.B - i0 : kRows);
    const i64 plane = w.plane;
    float *ht = w.h, *hv = w.h + 3 * plane, *hp = w.h + 5 * plane;
    float *dht = w.dh, *dhv = w.dh + 3 * plane, *dhp = w.dh + 5 * plane;
    forward_heads(n, a.s2, i0, nb, D, b0, b1, b2, S, wl, Keep{nullptr, nullptr, nullptr, 0}, false, nvs, nullptr);
    forward_heads(n, a.s, i0, nb, D, b0, b1, b2, S, wl, Keep{ht, hv, hp, plane}, true, vs, zs);
    const bool normal = n.w_ls != nullptr;
    for (int p = t; p < nb * kHeadCols; p += kThreads) dzs[p] = 0.f;
    __syncthreads();
    if (t < nb) {
        const i64 b = i0 + t;
        const float v = vs[t], nv = nvs[t];
        const float q = a.reward[b] + (a.not_term[b] * c.discount) * nv;
        srlxv::RowSums s{0.f, 0.f, 0.f, 0.f, 0.f};
        if (normal) {
            srlxv::normal_row(c, zs + t * kHeadCols, K, a.action_f + b * K, a.old_lp + b * K, q, a.total_reward[b], v, s, dzs + t * kHeadCols, a.new_lp + b * K);
        } else {
            const int A = n.policy.Out, act = a.action_i[b];
            a.new_lp[b] = srlxv::categorical_row(c, zs + t * kHeadCols, A, act < 0 ? 0 : (act >= A ? A - 1 : act), a.old_lp[b], q, a.total_reward[b], v, s, dzs + t * kHeadCols);
        }
        a.v[b] = v, a.n_v[b] = nv;
        w.rows[b] = s.huber, w.rows[w.max_batch + b] = s.align, w.rows[2 * w.max_batch + b] = s.policy, w.rows[3 * w.max_batch + b] = s.ent;
        w.dlast_v[b] = s.dv;
        b0[t * S] = s.dv;  // the value branch's rows of d loss / d (out layer output), column 0
    }
    __syncthreads();
    for (int p = t; p < nb * kHeadCols; p += kThreads) w.dlast_p[i0 * kHeadCols + p] = dzs[p];
    // ---- value branch: the bottom rows (what the trunk's top layer reads) end in buffer vb
    const int Lv = n.value.L, Lp = n.policy.L;
    int vb = 0;
    if (Lv >= 1) {
        srlxm::backward_rows<double>(n.value, Lv - 1, nb, i0, b1, b0, S, hv, dhv, plane);
        vb = (Lv & 1) ? 1 : 0;
    }
    float *VB = vb == 0 ? b0 : b1;
    float *P = vb == 0 ? b1 : b0, *Q = b2;  // the two other buffers
    const int HO = n.policy.Out;
    const Src none{nullptr, 0, 0, nullptr};
    const Src head{dzs, kHeadCols, HO, n.policy.weight(Lp)};
    const Src head_ls = normal ? Src{dzs + kNormalLs, kHeadCols, HO, n.w_ls} : none;
    const Src val{VB, S, Lv >= 1 ? n.value.W0 : 1, n.value.w0};  // (Lv = 0: column 0, through the out layer itself)
    if (Lp >= 1) {
        srlxm::backward_rows<double>(n.policy, Lp - 1, nb, i0, P, Q, S, hp, dhp, plane, SumSeed{head, head_ls, none});
        float *PB = (Lp & 1) ? P : Q, *F = (Lp & 1) ? Q : P;
        srlxm::backward_rows<double>(n.trunk, n.trunk.L - 1, nb, i0, F, VB, S, ht, dht, plane, SumSeed{val, Src{PB, S, n.policy.W0, n.policy.w0}, none});
    } else {
        srlxm::backward_rows<double>(n.trunk, n.trunk.L - 1, nb, i0, P, Q, S, ht, dht, plane, SumSeed{val, head, head_ls});
    }
}

__global__ void __launch_bounds__(kThreads) k_vppo_forward(const Net *__restrict__ net, i64 rows, const float *__restrict__ states, float *__restrict__ v, float *__restrict__ head0,
                                                           float *__restrict__ head1, float ls_lo, float ls_hi, int D, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *b2 = sm + 2 * kRows * S, *wl = sm + 3 * kRows * S;
    __shared__ float vs[kRows], zs[kRows * kHeadCols];
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * kRows;
    const int nb = (int)(rows - i0 < kRows ? rows - i0 : kRows);
    const Net &n = *net;
    forward_heads(n, states, i0, nb, D, b0, b1, b2, S, wl, Keep{nullptr, nullptr, nullptr, 0}, head0 != nullptr, vs, zs);
    if (v && t < nb) v[i0 + t] = vs[t];
    const int HO = n.policy.Out;
    if (head0 && t < nb * HO) {
        const int r = t / HO, j = t % HO;
        head0[(i0 + r) * HO + j] = zs[r * kHeadCols + j];
        if (head1) head1[(i0 + r) * HO + j] = srlxv::clampf(zs[r * kHeadCols + kNormalLs + j], ls_lo, ls_hi);
    }
}

// The Worker's policy() for the lanes of a lock-step (algorithms/ppo_v.py: Worker.policy, discrete branch, training): trunk and policy branch of
// `rpw` <= 16 dense rows per workgroup -- the value branch is skipped, the Worker throws v away -- then one thread per (row, action) for the softmax weight in
// float64, then one thread per row for the running sums, the two keyed uniforms, the action and its log-probability.  A row's logits are forward_heads' fma
// chains whatever rows share its workgroup, so `rpw` changes the launch shape and never a bit.  The weights stand in the weight tile once the network is done
// with it.  Two row buffers: nothing has to outlive a branch here.
struct ActArgs {
    i64 n;
    const float *obs;  // [n][D] dense
    srlx::u64 seed;
    const i64 *counter;  // read, not advanced
    double epsilon;
    float uniform_logp;  // act_uniform_logp(A), formed on the host
    int32_t *actions;
    float *logp;
    float *logits;  // NULL: not wanted
    double *cdf;    // NULL: not wanted
};

__global__ void __launch_bounds__(kThreads) k_vppo_act(const Net *__restrict__ net, ActArgs a, int rpw, int D, int A, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    double *cd = (double *)wl;  // [rpw][A] (2 * kRows * S floats in front of it: a multiple of 16 bytes)
    const Net &n = *net;
    const int t = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(a.n - i0 < rpw ? a.n - i0 : rpw);
    for (int p = t; p < nb * D; p += kThreads) b0[(p / D) * S + p % D] = a.obs[(i0 + p / D) * D + p % D];
    __syncthreads();
    float *T = srlxm::forward_rows<double>(n.trunk, n.trunk.L, nb, b0, b1, S, wl, nullptr, 0, 0, 0);
    const float *z = srlxm::forward_rows<double>(n.policy, n.policy.L + 1, nb, T, T == b0 ? b1 : b0, S, wl, nullptr, 0, 0, 0);
    if (t < nb * A) {
        const int r = t / A, j = t % A;
        const float *zr = z + r * S;
        float m = zr[0];
        for (int k = 1; k < A; k++) m = fmaxf(m, zr[k]);
        cd[t] = srlxv::act_weight(zr[j], m);
        if (a.logits) a.logits[(i0 + r) * A + j] = zr[j];
    }
    __syncthreads();
    if (t < nb) {
        const i64 r = i0 + t;
        double *c = cd + t * A;
        for (int k = 1; k < A; k++) c[k] = c[k - 1] + c[k];
        if (a.cdf)
            for (int k = 0; k < A; k++) a.cdf[r * A + k] = c[k];
        const srlx::u64 ctr = (srlx::u64)a.counter[0];
        const double u0 = srlx::u53(srlx::rng_u64(a.seed, ctr, (srlx::u64)(2 * r)));
        const double u1 = srlx::u53(srlx::rng_u64(a.seed, ctr, (srlx::u64)(2 * r + 1)));
        int act;
        float lp;
        if (srlxv::act_is_random(u0, a.epsilon)) {
            act = srlxv::act_uniform_action(u1, A);
            lp = a.uniform_logp;
        } else {
            act = srlxv::act_inverse_cdf(c, A, u1);
            float m, lse;
            bool pass;
            lp = srlxv::categorical_logp(z + t * S, A, act, m, lse, pass);
        }
        a.actions[r] = act;
        a.logp[r] = lp;
    }
}

// The Worker's policy() on the Normal head (algorithms/ppo_v.py: Worker.policy, NpArraySpace branch, training), k_vppo_act's launch shape and
// network pass: trunk and policy branch of `rpw` <= 16 dense rows per workgroup, the locs kept in `zs`, then the log-scale Linear on the head's input rows into
// the buffer the locs leave free -- forward_heads' fma chains, so a row's loc and clamped log-scale are srlx_vppo_forward's bits whatever rows share its
// workgroup.  Then one thread per (row, element): the keyed uniforms, Box-Muller in float64, the epsilon branch, the float32 action before tanh; behind a barrier
// the row's squashing correction from the row's stored actions, the log-probability through normal_logp (the update's own lines) and the environment's action.
struct ActNormalDraw {  // what the epilogue reads
    srlx::u64 seed;
    const i64 *counter;  // read, not advanced
    double epsilon;
    float noise_sd, noise_ls;  // policy_noise_normal_scale and (float)log of it, formed on the host
    float ls_lo, ls_hi;
    int squashed;
    const float *low, *high;  // [K]
    float *actions, *logp, *env_actions;  // [n][K]
    float *loc, *log_scale;  // [n][K]; NULL: not wanted
    double *z;               // [n][K]; NULL: not wanted
};
struct ActNormalArgs {
    i64 n;
    const float *obs;  // [n][D] dense
    ActNormalDraw draw;
};

__global__ void __launch_bounds__(kThreads) k_vppo_act_normal(const Net *__restrict__ net, ActNormalArgs args, int rpw, int D, int K, int S) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *b0 = sm, *b1 = sm + kRows * S, *wl = sm + 2 * kRows * S;
    __shared__ float zs[kRows * kHeadCols], acts[kRows * kNormalLs];
    // the epilogue's arguments wait in LDS: held in scalar registers through the network pass they spilled (the first barrier below publishes them)
    __shared__ ActNormalDraw draw;
    const Net &n = *net;
    const int t = threadIdx.x;
    if (t == 0) draw = args.draw;
    const i64 i0 = (i64)blockIdx.x * rpw;
    const int nb = (int)(args.n - i0 < rpw ? args.n - i0 : rpw);
    for (int p = t; p < nb * D; p += kThreads) b0[(p / D) * S + p % D] = args.obs[(i0 + p / D) * D + p % D];
    __syncthreads();
    float *T = srlxm::forward_rows<double>(n.trunk, n.trunk.L, nb, b0, b1, S, wl, nullptr, 0, 0, 0);
    float *z = srlxm::forward_rows<double>(n.policy, n.policy.L + 1, nb, T, T == b0 ? b1 : b0, S, wl, nullptr, 0, 0, 0);
    const float *hin = z == b0 ? b1 : b0;  // the head's input rows
    const bool mine = t < nb * K;
    const int r = t / K, j = t % K;
    if (mine) zs[r * kHeadCols + j] = z[r * S + j];
    __syncthreads();
    srlxm::dense<double>(n.w_ls, n.b_ls, n.policy.in_of(n.policy.L), K, nb, hin, S, z, S, false, wl);
    __syncthreads();
    const ActNormalDraw &a = draw;
    const i64 row = i0 + r;
    float loc = 0.f, ls = 0.f, sd = 0.f, act = 0.f;
    if (mine) {
        const float h_loc = zs[r * kHeadCols + j], h_ls = srlxv::clampf(z[r * S + j], a.ls_lo, a.ls_hi);
        const srlx::u64 ctr = (srlx::u64)a.counter[0], base = (srlx::u64)(2 * K + 1) * (srlx::u64)row;
        const double u0 = srlx::u53(srlx::rng_u64(a.seed, ctr, base));
        const double ua = srlx::u53(srlx::rng_u64(a.seed, ctr, base + 1 + 2 * j));
        const double ub = srlx::u53(srlx::rng_u64(a.seed, ctr, base + 2 + 2 * j));
        const double zn = srlxv::act_box_muller(ua, ub);
        const bool random = srlxv::act_is_random(u0, a.epsilon);
        loc = random ? 0.f : h_loc, ls = random ? a.noise_ls : h_ls, sd = random ? a.noise_sd : expf(h_ls);
        act = srlxv::act_normal_action(loc, sd, zn);
        acts[r * kNormalLs + j] = act;
        a.actions[row * K + j] = act;
        if (a.loc) a.loc[row * K + j] = h_loc, a.log_scale[row * K + j] = h_ls;
        if (a.z) a.z[row * K + j] = zn;
    }
    __syncthreads();
    if (mine) {
        const float corr = a.squashed ? srlxv::squash_correction(acts + r * kNormalLs, K) : 0.f;
        float u;
        a.logp[row * K + j] = srlxv::normal_logp(act, loc, ls, sd, corr, u);
        a.env_actions[row * K + j] = srlxv::act_env_action(act, a.low[j], a.high[j], a.squashed);
    }
}

// The four loss sums of k_vppo_grad's last four threads: loss_value, loss_v_align, loss_policy, loss_e into out[0..3]
struct LossSums {
    static constexpr int n = 4;
    i64 B;
    const float *rows;  // [4][max_batch]
    i64 max_batch;
    double inv_n, inv_b;
    int entropy;
    float *out;
    __device__ void operator()(int k) const {
        double s = 0.0;
        for (i64 b = 0; b < B; b++) s += (double)rows[k * max_batch + b];
        out[k] = k == 0 || k == 1 ? (float)(s * inv_n) : (k == 2 ? (float)(-s * inv_n) : (entropy ? (float)(s * inv_b) : 0.f));
    }
};

struct GradArgs {
    const Seg *segs;
    int nseg;
    const float *xin0;  // the caller's states: the input rows of the first layer
    double *partials;
    LossSums sums;
};

__global__ void __launch_bounds__(kThreads) k_vppo_grad(GradArgs a) { srlxt::grad_body(a.segs, a.nseg, a.sums.B, a.xin0, a.partials, a.sums); }

__global__ void __launch_bounds__(kThreads) k_vppo_step(srlxt::StepArgs a) { srlxt::step_body(a); }

int check_shape(const char *who, int D, int head, int A, int nt, const int *tw, int nv, const int *vw, int np, const int *pw, i64 max_batch) {
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(head == 0 || head == 1, "%s: head kind %d (0 categorical, 1 Normal)", who, head);
    SRLX_REQUIRE(head == 1 || (A >= 2 && A <= 16), "%s: %d actions (2..16)", who, A);
    SRLX_REQUIRE(head == 0 || (A >= 1 && A <= 8), "%s: %d action elements (1..8)", who, A);
    SRLX_REQUIRE(srlxt::widths_ok(nt, 1, 3, tw), "%s: the trunk is 1..3 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(srlxt::widths_ok(nv, 0, 2, vw), "%s: the value block is 0..2 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(srlxt::widths_ok(np, 0, 2, pw), "%s: the policy block is 0..2 layers of 32..512 units in multiples of 32", who);
    SRLX_REQUIRE(max_batch >= 1 && max_batch <= 256, "%s: max_batch %lld (1..256)", who, (long long)max_batch);
    return SRLX_OK;
}

int wmax_of(int D, int nt, const int *tw, int nv, const int *vw, int np, const int *pw) {
    int w = D > kHeadCols ? D : kHeadCols;
    for (int l = 0; l < nt; l++) w = tw[l] > w ? tw[l] : w;
    for (int l = 0; l < nv; l++) w = vw[l] > w ? vw[l] : w;
    for (int l = 0; l < np; l++) w = pw[l] > w ? pw[l] : w;
    return w;
}

// (out, in) of every Linear in state-dict order
int linear_shapes(const srlx_vppo *h, int (*shape)[2]) {
    int n = 0, in = h->D;
    for (int l = 0; l < h->Lt; l++) shape[n][0] = h->Wt[l], shape[n][1] = in, in = h->Wt[l], n++;
    const int top = in;
    for (int l = 0; l < h->Lv; l++) shape[n][0] = h->Wv[l], shape[n][1] = in, in = h->Wv[l], n++;
    shape[n][0] = 1, shape[n][1] = in, n++;
    in = top;
    for (int l = 0; l < h->Lp; l++) shape[n][0] = h->Wp[l], shape[n][1] = in, in = h->Wp[l], n++;
    shape[n][0] = h->A, shape[n][1] = in, n++;
    if (h->head) shape[n][0] = h->A, shape[n][1] = in, n++;
    return n;
}

i64 elements_of(const srlx_vppo *h) {
    int shape[kMaxTensors / 2][2];
    const int n = linear_shapes(h, shape);
    i64 e = 0;
    for (int l = 0; l < n; l++) e += (i64)shape[l][0] * shape[l][1] + shape[l][0];
    return e;
}

Net net_of(const srlx_vppo *h) {
    Net n;
    float *tr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 2 * h->Lt; i++) tr[i] = h->ps.p[i];  // (the trunk has no layer of its own behind its hidden ones: slot Lt stays NULL)
    n.trunk = srlxt::chain(h->D, h->Lt, h->Wt, 0, tr);
    const int top = h->Wt[h->Lt - 1];
    n.value = srlxt::chain(top, h->Lv, h->Wv, 1, h->ps.p + 2 * h->Lt);
    float *const *pp = h->ps.p + 2 * (h->Lt + h->Lv + 1);
    n.policy = srlxt::chain(top, h->Lp, h->Wp, h->A, pp);
    n.w_ls = h->head ? pp[2 * (h->Lp + 1)] : nullptr;
    n.b_ls = h->head ? pp[2 * (h->Lp + 1) + 1] : nullptr;
    return n;
}

int upload_net(srlx_vppo *h) {
    const Net n = net_of(h);
    SRLX_HIP(hipMemcpy(h->d_net, &n, sizeof(n), hipMemcpyHostToDevice));
    h->ps.net_ok = true;
    return SRLX_OK;
}

int upload_table(srlx_vppo *h) {
    Seg segs[kMaxTensors];
    memset(segs, 0, sizeof(segs));
    int shape[kMaxTensors / 2][2];
    const int nl = linear_shapes(h, shape);
    const i64 plane = h->max_batch * h->wmax;
    const float *ht = h->h, *hv = h->h + 3 * plane, *hp = h->h + 5 * plane;
    const float *dht = h->dh, *dhv = h->dh + 3 * plane, *dhp = h->dh + 5 * plane;
    const float *top = ht + (i64)(h->Lt - 1) * plane;
    i64 end = 0;
    for (int l = 0; l < nl; l++) {
        const float *dout, *xin;
        int stride = shape[l][0];
        int k = l;
        if (k < h->Lt) {
            dout = dht + (i64)k * plane, xin = k ? ht + (i64)(k - 1) * plane : nullptr;
        } else if ((k -= h->Lt) < h->Lv) {
            dout = dhv + (i64)k * plane, xin = k ? hv + (i64)(k - 1) * plane : top;
        } else if ((k -= h->Lv) == 0) {
            dout = h->dlast_v, xin = h->Lv ? hv + (i64)(h->Lv - 1) * plane : top;
        } else if ((k -= 1) < h->Lp) {
            dout = dhp + (i64)k * plane, xin = k ? hp + (i64)(k - 1) * plane : top;
        } else {
            k -= h->Lp;  // 0: logits or locs, 1: log-scales
            dout = h->dlast_p + (k ? kNormalLs : 0), stride = kHeadCols, xin = h->Lp ? hp + (i64)(h->Lp - 1) * plane : top;
        }
        srlxt::push_linear(segs + 2 * l, end, shape[l][0], shape[l][1], stride, dout, xin, h->ps, 2 * l);
    }
    SRLX_HIP(hipMemcpy(h->d_segs, segs, sizeof(segs), hipMemcpyHostToDevice));
    h->ps.table_ok = true;
    return SRLX_OK;
}

void fill(srlx_vppo *h, int D, int head, int A, int nt, const int *tw, int nv, const int *vw, int np, const int *pw, i64 max_batch, int device) {
    h->D = D, h->head = head, h->A = A, h->Lt = nt, h->Lv = nv, h->Lp = np, h->device = device, h->max_batch = max_batch;
    for (int l = 0; l < nt; l++) h->Wt[l] = tw[l];
    for (int l = 0; l < nv; l++) h->Wv[l] = vw[l];
    for (int l = 0; l < np; l++) h->Wp[l] = pw[l];
    h->wmax = wmax_of(D, nt, tw, nv, vw, np, pw);
    h->wmax_act = D;
    for (int l = 0; l < nt; l++) h->wmax_act = tw[l] > h->wmax_act ? tw[l] : h->wmax_act;
    for (int l = 0; l < np; l++) h->wmax_act = pw[l] > h->wmax_act ? pw[l] : h->wmax_act;
    h->nt = n_tensors(h);
    h->elements = elements_of(h);
    h->grad_blocks = (h->elements + 4 + kThreads - 1) / kThreads;
}

}  // namespace

extern "C" {

int64_t srlx_vppo_scratch_floats(int obs_dim, int head, int n_out, int n_trunk, const int *trunk_widths, int n_value, const int *value_widths, int n_policy,
                                 const int *policy_widths, int64_t max_batch) {
    if (check_shape("vppo_scratch_floats", obs_dim, head, n_out, n_trunk, trunk_widths, n_value, value_widths, n_policy, policy_widths, max_batch) != SRLX_OK)
        return -1;
    srlx_vppo h{};
    fill(&h, obs_dim, head, n_out, n_trunk, trunk_widths, n_value, value_widths, n_policy, policy_widths, max_batch, 0);
    return 2 * kPlanes * max_batch * h.wmax + max_batch + max_batch * kHeadCols + 4 * max_batch + 2 * h.grad_blocks;
}

int srlx_vppo_create(srlx_vppo_t **out, int obs_dim, int head, int n_out, int n_trunk, const int *trunk_widths, int n_value, const int *value_widths, int n_policy,
                     const int *policy_widths, int64_t max_batch, int device) {
    SRLX_REQUIRE(out, "vppo_create: NULL handle pointer");
    *out = nullptr;
    SRLX_TRY(check_shape("vppo_create", obs_dim, head, n_out, n_trunk, trunk_widths, n_value, value_widths, n_policy, policy_widths, max_batch));
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "vppo_create: device %d unavailable", device);
    srlx_vppo *h = new srlx_vppo();
    fill(h, obs_dim, head, n_out, n_trunk, trunk_widths, n_value, value_widths, n_policy, policy_widths, max_batch, device);
    const size_t plane = (size_t)max_batch * h->wmax;
    hipError_t e = hipMalloc((void **)&h->d_segs, sizeof(Seg) * kMaxTensors);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_net, sizeof(Net));
    if (e == hipSuccess) e = hipMalloc((void **)&h->h, sizeof(float) * kPlanes * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dh, sizeof(float) * kPlanes * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dlast_v, sizeof(float) * max_batch);
    if (e == hipSuccess) e = hipMalloc((void **)&h->dlast_p, sizeof(float) * max_batch * kHeadCols);
    if (e == hipSuccess) e = hipMalloc((void **)&h->rows, sizeof(float) * 4 * max_batch);
    if (e == hipSuccess) e = hipMalloc((void **)&h->partials, sizeof(double) * h->grad_blocks);
    if (e == hipSuccess) e = hipMemset(h->dlast_p, 0, sizeof(float) * max_batch * kHeadCols);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_vppo_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap3);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_vppo_forward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap3);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_vppo_act, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap2);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_vppo_act_normal, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srlxt::kLdsCap2);
    if (e != hipSuccess) {
        srlx_vppo_destroy(h);
        srlx::set_error("vppo_create: device set-up failed: %s", hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    *out = h;
    return SRLX_OK;
}

int srlx_vppo_destroy(srlx_vppo_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (void *p : {(void *)h->d_net, (void *)h->d_segs, (void *)h->h, (void *)h->dh, (void *)h->dlast_v, (void *)h->dlast_p, (void *)h->rows, (void *)h->partials})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_vppo_bind(srlx_vppo_t *h, float *const *d_params) {
    SRLX_REQUIRE(h && d_params, "vppo_bind: NULL argument");
    return h->ps.bind_params("vppo_bind", h->nt, d_params);
}

int srlx_vppo_bind_grads(srlx_vppo_t *h, float *const *d_grads, float *const *d_raw_grads) {
    SRLX_REQUIRE(h && d_grads && d_raw_grads, "vppo_bind_grads: NULL argument");
    return h->ps.bind_grads("vppo_bind_grads", h->nt, d_grads, d_raw_grads);
}

int srlx_vppo_bind_adam(srlx_vppo_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, int64_t steps_taken, double beta1, double beta2, double eps) {
    SRLX_REQUIRE(h && d_exp_avg && d_exp_avg_sq, "vppo_bind_adam: NULL argument");
    return h->ps.bind_adam("vppo_bind_adam", h->nt, d_exp_avg, d_exp_avg_sq, steps_taken, beta1, beta2, eps);
}

int64_t srlx_vppo_steps(const srlx_vppo_t *h) {
    if (!h) {
        srlx::set_error("vppo_steps: NULL handle");
        return -1;
    }
    return h->ps.steps;
}

int srlx_vppo_forward(srlx_vppo_t *h, int64_t n, const float *d_states, double log_scale_lo, double log_scale_hi, float *d_v, float *d_head0, float *d_head1,
                      void *stream) {
    SRLX_REQUIRE(h && d_states, "vppo_forward: NULL handle or states");
    SRLX_REQUIRE(h->ps.bound, "vppo_forward: unbound handle (srlx_vppo_bind)");
    SRLX_REQUIRE(n >= 1 && n <= (int64_t)1 << 24, "vppo_forward: %lld rows (1..2^24)", (long long)n);
    SRLX_REQUIRE(d_v || d_head0, "vppo_forward: nothing to write");
    SRLX_REQUIRE(!d_head1 || (d_head0 && h->head == 1), "vppo_forward: log-scales go with locs, on a Normal head");
    SRLX_REQUIRE(!(h->head == 1 && d_head0 && !d_head1), "vppo_forward: a Normal head writes locs and log-scales");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "vppo_forward: the log-scale clamp's ends are ordered");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    hipLaunchKernelGGL(k_vppo_forward, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), lds_bytes(h), (hipStream_t)stream, (const Net *)h->d_net, (i64)n, d_states, d_v,
                       d_head0, d_head1, (float)log_scale_lo, (float)log_scale_hi, h->D, lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_vppo_act(srlx_vppo_t *h, int64_t n_rows, const float *d_obs, uint64_t seed, const int64_t *d_counter, double epsilon, int32_t *d_actions, float *d_logp,
                  float *d_logits, double *d_cdf, void *stream) {
    SRLX_REQUIRE(h, "vppo_act: NULL handle");
    SRLX_REQUIRE(h->ps.bound, "vppo_act: unbound handle (srlx_vppo_bind)");
    SRLX_REQUIRE(h->head == 0, "vppo_act: the acting kernel serves the categorical head");
    SRLX_REQUIRE(n_rows >= 1 && n_rows <= 65536, "vppo_act: %lld rows (1..65536)", (long long)n_rows);
    SRLX_REQUIRE(epsilon >= 0.0 && epsilon <= 1.0, "vppo_act: epsilon %g (0..1)", epsilon);
    SRLX_REQUIRE(d_obs && d_counter && d_actions && d_logp, "vppo_act: NULL observations, counter, actions or log-probabilities");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    const int rpw = srlxt::rows_per_workgroup(n_rows);
    ActArgs a{(i64)n_rows, d_obs, (srlx::u64)seed, (const i64 *)d_counter, epsilon, srlxv::act_uniform_logp(h->A), d_actions, d_logp, d_logits, d_cdf};
    hipLaunchKernelGGL(k_vppo_act, dim3((unsigned)((n_rows + rpw - 1) / rpw)), dim3(kThreads), act_lds_bytes(h), (hipStream_t)stream, (const Net *)h->d_net, a, rpw, h->D, h->A,
                       act_lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_vppo_act_normal(srlx_vppo_t *h, int64_t n_rows, const float *d_obs, uint64_t seed, const int64_t *d_counter, double epsilon, double noise_scale, int squashed,
                         double log_scale_lo, double log_scale_hi, const float *d_low, const float *d_high, float *d_actions, float *d_logp, float *d_env_actions,
                         float *d_loc, float *d_log_scale, double *d_z, void *stream) {
    SRLX_REQUIRE(h, "vppo_act_normal: NULL handle");
    SRLX_REQUIRE(h->ps.bound, "vppo_act_normal: unbound handle (srlx_vppo_bind)");
    SRLX_REQUIRE(h->head == 1, "vppo_act_normal: the acting kernel serves the Normal head (srlx_vppo_act serves the categorical one)");
    SRLX_REQUIRE(n_rows >= 1 && n_rows <= 65536, "vppo_act_normal: %lld rows (1..65536)", (long long)n_rows);
    SRLX_REQUIRE(epsilon >= 0.0 && epsilon <= 1.0, "vppo_act_normal: epsilon %g (0..1)", epsilon);
    SRLX_REQUIRE(noise_scale > 0.0 && std::isfinite(noise_scale), "vppo_act_normal: noise scale %g (positive and finite)", noise_scale);
    SRLX_REQUIRE(squashed == 0 || squashed == 1, "vppo_act_normal: squashed is 0 or 1");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "vppo_act_normal: the log-scale clamp's ends are ordered");
    SRLX_REQUIRE(d_obs && d_counter && d_low && d_high && d_actions && d_logp && d_env_actions,
                 "vppo_act_normal: NULL observations, counter, bounds, actions, log-probabilities or environment actions");
    SRLX_REQUIRE((d_loc != nullptr) == (d_log_scale != nullptr), "vppo_act_normal: locs and log-scales are written together or not at all");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    const int rpw = srlxt::rows_per_workgroup(n_rows);
    ActNormalArgs a{(i64)n_rows, d_obs, ActNormalDraw{(srlx::u64)seed, (const i64 *)d_counter, epsilon, (float)noise_scale, (float)log(noise_scale), (float)log_scale_lo,
                                                      (float)log_scale_hi, squashed, d_low, d_high, d_actions, d_logp, d_env_actions, d_loc, d_log_scale, d_z}};
    hipLaunchKernelGGL(k_vppo_act_normal, dim3((unsigned)((n_rows + rpw - 1) / rpw)), dim3(kThreads), act_lds_bytes(h), (hipStream_t)stream, (const Net *)h->d_net, a, rpw,
                       h->D, h->A, act_lds_stride(h));
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_vppo_update(srlx_vppo_t *h, int64_t batch, const float *d_states, const float *d_next_states, const void *d_actions, const float *d_old_logpi,
                     const float *d_rewards, const float *d_not_terminated, const float *d_total_rewards, double lr, double discount, double clip_range,
                     double entropy_weight, double loss_align_coeff, double max_grad_norm, int squashed, double log_scale_lo, double log_scale_hi, float *d_v,
                     float *d_n_v, float *d_new_logpi, float *d_scalars, void *stream) {
    SRLX_REQUIRE(h, "vppo_update: NULL handle");
    SRLX_REQUIRE(h->ps.ready(), "vppo_update: bind the parameters, the gradient tensors and the Adam state first");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "vppo_update: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_states && d_next_states && d_actions && d_old_logpi && d_rewards && d_not_terminated && d_total_rewards && d_v && d_n_v && d_new_logpi && d_scalars,
                 "vppo_update: NULL argument");
    SRLX_REQUIRE(lr >= 0 && clip_range >= 0 && max_grad_norm > 0, "vppo_update: lr and clip_range are non-negative, max_grad_norm positive");
    SRLX_REQUIRE(squashed == 0 || squashed == 1, "vppo_update: squashed is 0 or 1");
    SRLX_REQUIRE(log_scale_lo <= log_scale_hi, "vppo_update: the log-scale clamp's ends are ordered");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.net_ok) SRLX_TRY(upload_net(h));
    if (!h->ps.table_ok) SRLX_TRY(upload_table(h));
    hipStream_t st = (hipStream_t)stream;
    const int K = h->head ? h->A : 1;
    const double N = (double)batch * K;
    srlxv::Cfg c{(float)discount, (float)(1.0 - clip_range), (float)(1.0 + clip_range), (float)entropy_weight, (float)loss_align_coeff, (float)(1.0 / N),
                 (float)(1.0 / (double)batch), (float)log_scale_lo, (float)log_scale_hi, squashed};
    Batch b{(i64)batch, d_states, d_next_states, d_old_logpi, d_rewards, d_not_terminated, d_total_rewards, h->head ? nullptr : (const int32_t *)d_actions,
            h->head ? (const float *)d_actions : nullptr, d_v, d_n_v, d_new_logpi};
    Work w{h->h, h->dh, h->dlast_v, h->dlast_p, h->rows, h->max_batch * h->wmax, h->max_batch};
    hipLaunchKernelGGL(k_vppo_rows, dim3((unsigned)((batch + kRows - 1) / kRows)), dim3(kThreads), lds_bytes(h), st, (const Net *)h->d_net, b, w, c, h->D, K, lds_stride(h));
    GradArgs ga{h->d_segs, h->nt, d_states, h->partials, LossSums{(i64)batch, h->rows, h->max_batch, 1.0 / N, 1.0 / (double)batch, entropy_weight > 0 ? 1 : 0, d_scalars}};
    hipLaunchKernelGGL(k_vppo_grad, dim3((unsigned)h->grad_blocks), dim3(kThreads), 0, st, ga);
    const srlxt::StepArgs sa = h->ps.step_args(h->d_segs, h->nt, h->partials, h->grad_blocks, max_grad_norm, lr, d_scalars + 4);
    hipLaunchKernelGGL(k_vppo_step, dim3((unsigned)((h->elements + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sa);
    SRLX_HIP(hipGetLastError());
    h->ps.steps++;
    return SRLX_OK;
}

}  // extern "C"
