// srlx_param_tail.h -- what stands around the row-blocked passes (srlx_mlp_rows.h) in every update that ends in clip_grad_norm_ and one Adam step: V-PPO
// (srlx_vppo.hip) and NoT_SAC (srlx_notsac.hip).  An algorithm's file keeps its row kernels, its loss sums and which rows feed which tensor; the rest is here.
//   Seg, push_linear   the segment table: one entry per parameter tensor, a weight + bias pair per Linear
//   grad_body          one thread per parameter: the gradient before the clip, a sum over the batch in row order; every workgroup leaves the sum of its squares;
//                      the last threads of the launch own no element and run the caller's loss sums instead
//   step_body          every workgroup sums the same partial squares in the same order (the norm), then one thread per parameter: the clipped gradient and Adam
//   ParamSet           the host's side of the table: the bound tensors, Adam's constants, the step count and what is stale
//   chain, widths_ok, rows_per_workgroup, row_lds_bytes   the shape rules of a handle (srlx_sacd.hip reads these too; its gradient kernel, which has no norm
//                      clip, steps Adam in the gradient thread and syncs the target, is its own)
// No atomics and a fixed order in every sum: equal inputs give equal bits.
#pragma once
#include "srlx_adam_math.h"
#include "srlx_common.h"
#include "srlx_mlp_rows.h"

namespace srlxt {

using i64 = int64_t;
using srlxm::kRows;
using srlxm::kThreads;
using srlxm::kWTile;
using srlxm::Layers;

constexpr int kMaxTensors = 20;  // the most of any handle (V-PPO: 2 x (3 trunk + 2 value + value_out + 2 policy + 2 heads))

struct Seg {  // one parameter tensor
    i64 end;          // running element count (within its network)
    int stride, in;   // row stride of dout; in = 0: a bias
    const float *dout, *xin;  // [B][stride] d loss / d (layer output), [B][in] the layer's input rows (NULL: the caller's states)
    float *p, *g, *graw, *m, *v;
};

// the sum of every thread's `mine`, in sq[0] behind a barrier
__device__ __forceinline__ void block_sum(double *sq, double mine) {
    const int t = threadIdx.x;
    sq[t] = mine;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) sq[t] += sq[t + w];
        __syncthreads();
    }
}

// `tail`: tail.n loss sums and tail(k), which reduces and writes sum k.  The launch rounds the element count + tail.n up to whole workgroups, so the last
// tail.n threads of the last workgroup exist and own no element.
template <typename Tail>
__device__ __forceinline__ void grad_body(const Seg *segs, int nseg, i64 B, const float *xin0, double *partials, Tail tail) {
    __shared__ double sq[kThreads];
    const int t = threadIdx.x;
    const i64 i = (i64)blockIdx.x * kThreads + t;
    const i64 last = (i64)gridDim.x * kThreads;
    double mine = 0.0;
    if (i >= last - tail.n) {
        tail((int)(i - (last - tail.n)));
    } else if (i < segs[nseg - 1].end) {
        int s = 0;
        while (i >= segs[s].end) s++;
        const Seg sg = segs[s];
        const i64 e = i - (s ? segs[s - 1].end : 0);
        const int St = sg.stride, In = sg.in;
        double acc = 0.0;
        if (In) {
            const int u = (int)(e / In), k = (int)(e % In);
            const float *dout = sg.dout + u, *xin = (sg.xin ? sg.xin : xin0) + k;
#pragma unroll 8
            for (int b = 0; b < (int)B; b++) acc = fma((double)dout[(i64)b * St], (double)xin[(i64)b * In], acc);
        } else {
            const float *dout = sg.dout + e;
#pragma unroll 8
            for (int b = 0; b < (int)B; b++) acc += (double)dout[(i64)b * St];
        }
        const float g = (float)acc;
        sg.graw[e] = g;
        mine = (double)g * (double)g;
    }
    block_sum(sq, mine);
    if (t == 0) partials[blockIdx.x] = sq[0];
}

struct StepArgs {
    const Seg *segs;
    int nseg;
    const double *partials;
    i64 n_partials;
    float max_norm;
    double lr, beta1, beta2, eps;
    i64 steps_taken;
    float *norm_out;
};

__device__ __forceinline__ void step_body(const StepArgs &a) {
    __shared__ double sq[kThreads];
    const int t = threadIdx.x;
    double mine = 0.0;
    for (i64 k = t; k < a.n_partials; k += kThreads) mine += a.partials[k];
    block_sum(sq, mine);
    // clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6)) in float32, and the gradients are always multiplied by it
    const float norm = (float)sqrt(sq[0]);
    const float coef = fminf(1.f, a.max_norm / (norm + 1e-6f));
    const i64 i = (i64)blockIdx.x * kThreads + t;
    if (i == 0) a.norm_out[0] = norm;
    if (i >= a.segs[a.nseg - 1].end) return;
    int s = 0;
    while (i >= a.segs[s].end) s++;
    const Seg sg = a.segs[s];
    const i64 e = i - (s ? a.segs[s - 1].end : 0);
    const float g = sg.graw[e] * coef;
    sg.g[e] = g;
    const srlx::AdamCoef c = srlx::adam_coef(a.lr, a.beta1, a.beta2, a.eps, a.steps_taken);
    float p = sg.p[e], m = sg.m[e], v = sg.v[e];
    srlx::adam_one_foreach(p, g, m, v, c);
    sg.p[e] = p, sg.m[e] = m, sg.v[e] = v;
}

// What a handle has been given.  Binding anything makes the segment table stale; binding parameters makes the network's device copy stale too.  `who` is the
// entry point's name, `n` the handle's tensor count; the entry point has checked its own pointers.
struct ParamSet {
    float *p[kMaxTensors], *g[kMaxTensors], *graw[kMaxTensors], *m[kMaxTensors], *v[kMaxTensors];
    double beta1, beta2, eps;
    i64 steps;
    bool bound, grads_bound, adam_bound, table_ok, net_ok;

    int bind_params(const char *who, int n, float *const *d_params) {
        for (int i = 0; i < n; i++) SRLX_REQUIRE(d_params[i], "%s: parameter %d is NULL", who, i);
        for (int i = 0; i < n; i++) p[i] = d_params[i];
        bound = true, table_ok = net_ok = false;
        return SRLX_OK;
    }
    int bind_grads(const char *who, int n, float *const *d_grads, float *const *d_raw_grads) {
        for (int i = 0; i < n; i++) SRLX_REQUIRE(d_grads[i] && d_raw_grads[i], "%s: gradient tensor %d is NULL", who, i);
        for (int i = 0; i < n; i++) g[i] = d_grads[i], graw[i] = d_raw_grads[i];
        grads_bound = true, table_ok = false;
        return SRLX_OK;
    }
    int bind_adam(const char *who, int n, float *const *d_exp_avg, float *const *d_exp_avg_sq, i64 steps_taken, double b1, double b2, double e) {
        SRLX_REQUIRE(b1 >= 0 && b1 < 1 && b2 >= 0 && b2 < 1 && e > 0, "%s: betas in [0, 1) and eps > 0", who);
        SRLX_REQUIRE(steps_taken >= 0, "%s: the step count is non-negative", who);
        for (int i = 0; i < n; i++) SRLX_REQUIRE(d_exp_avg[i] && d_exp_avg_sq[i], "%s: state %d is NULL", who, i);
        for (int i = 0; i < n; i++) m[i] = d_exp_avg[i], v[i] = d_exp_avg_sq[i];
        steps = steps_taken, beta1 = b1, beta2 = b2, eps = e;
        adam_bound = true, table_ok = false;
        return SRLX_OK;
    }
    bool ready() const { return bound && grads_bound && adam_bound; }
    StepArgs step_args(const Seg *segs, int nseg, const double *partials, i64 n_partials, double max_norm, double lr, float *norm_out) const {
        return StepArgs{segs, nseg, partials, n_partials, (float)max_norm, lr, beta1, beta2, eps, steps, norm_out};
    }
};

// The weight and bias entries of one Linear [out][in] at pair[0], pair[1]: tensors ti and ti + 1 of `ps`.  `end` runs on.
inline void push_linear(Seg *pair, i64 &end, int out, int in, int stride, const float *dout, const float *xin, const ParamSet &ps, int ti) {
    for (int j = 0; j < 2; j++) {
        Seg &g = pair[j];
        end += j == 0 ? (i64)out * in : out;
        g.end = end, g.stride = stride, g.in = j == 0 ? in : 0;
        g.dout = dout, g.xin = xin;
        g.p = ps.p[ti + j], g.g = ps.g[ti + j], g.graw = ps.graw[ti + j], g.m = ps.m[ti + j], g.v = ps.v[ti + j];
    }
}

// L hidden layers of widths W and the Linear behind them, from (weight, bias) pairs in `p`.  L = 0: the out layer alone.  A NULL slot: no such layer (a trunk
// has none behind its hidden ones).
inline Layers chain(int In, int L, const int *W, int Out, float *const *p) {
    Layers n;
    n.In = In, n.L = L, n.Out = Out;
    n.W0 = L > 0 ? W[0] : 0, n.W1 = L > 1 ? W[1] : 0, n.W2 = L > 2 ? W[2] : 0;
    const float *w[4] = {nullptr, nullptr, nullptr, nullptr}, *b[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l <= L && l < 4; l++)
        if (p[2 * l]) w[l] = p[2 * l], b[l] = p[2 * l + 1];
    n.w0 = w[0], n.w1 = w[1], n.w2 = w[2], n.w3 = w[3], n.b0 = b[0], n.b1 = b[1], n.b2 = b[2], n.b3 = b[3];
    return n;
}

// lo..hi layers of 32..512 units in multiples of 32
inline bool widths_ok(int n, int lo, int hi, const int *w) {
    if (n < lo || n > hi || (n && !w)) return false;
    for (int l = 0; l < n; l++)
        if (w[l] < 32 || w[l] > 512 || w[l] % 32) return false;
    return true;
}

// rows per workgroup of a row kernel over n rows: the smallest of 1, 2, 4, 8, 16 that keeps the launch within one workgroup for each of the MI355X's 256
// compute units (a workgroup's time grows with its rows, and every workgroup of a launch that fits the machine runs at once: DESIGN.md 7n).  A row's chains
// are the same whatever rows share its workgroup, so this changes the launch shape and never a bit.
inline int rows_per_workgroup(i64 n) {
    int rpw = 1;
    while (rpw < kRows && (n + rpw - 1) / rpw > 256) rpw *= 2;
    return rpw;
}

// dynamic LDS of a row kernel: `buffers` row buffers of kRows x (widest row + 1) floats and the weight tile.  The caps are the most any handle asks for: a
// kernel's limit is set to its cap at every create, so that creating a narrow handle never lowers it under a wide one that is still alive.
constexpr size_t row_lds_bytes(int buffers, int wmax) { return sizeof(float) * ((size_t)buffers * kRows * (wmax + 1) + kWTile); }
constexpr size_t kLdsCap3 = row_lds_bytes(3, 512);  // 131 264 bytes
constexpr size_t kLdsCap2 = row_lds_bytes(2, 512);  //  98 432 bytes

}  // namespace srlxt
