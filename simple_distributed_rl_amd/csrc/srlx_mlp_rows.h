// srlx_mlp_rows.h -- the row-blocked MLP passes shared by the flat-observation kernels: DQN / Rainbow / C51's Q-network (srlx_mlpq.hip, float32 sums), discrete
// SAC's five networks (srlx_sacd.hip), V-PPO's actor-critic (srlx_vppo.hip) and NoT_SAC's policy and Q-network (srlx_notsac.hip; float64 sums).  The work is not a GEMM's (<= 16 rows through <= 4 layers of <= 512 units), so launch count and the layer
// chain bound it: one workgroup of kThreads threads takes up to kRows rows through the whole network, and back.
//   Layers         one network as the kernels read it
//   dense<Acc>     one Linear (+ ReLU) layer over the rows
//   forward_rows   the first `layers` layers, with the hidden rows kept for the backward pass
//   backward_rows  d loss / d h_l down the hidden layers, row by row; the top layer through the next weight, or from a seed the caller gives
//   SumSeed        that seed for a layer which up to three Linear layers read
//   head_rows      a policy head's output rows in kHeadCols columns: logits, or locs and log-scales
// Acc = float: one float32 fused multiply-add per term.  Acc = double: the same chain in float64, rounded to float32 once per sum.  Either way every sum runs
// in k order with no atomics, so equal inputs give equal bits.
//
// LDS layout (dynamic, floats): two row buffers of kRows * S each, S = (widest row of the handle) + 1 -- odd on purpose: rows of different row groups fall on
// different banks -- then whatever the kernel adds, then the weight tile of kWTile floats.  A plain acting kernel asks for 2 * kRows * S + kWTile floats.
#pragma once
#include <stdint.h>

#include <type_traits>

#include <hip/hip_runtime.h>

namespace srlxm {
using i64 = int64_t;

constexpr int kThreads = 256;
constexpr int kRows = 16;     // rows of one workgroup
constexpr int kWTile = 8192;  // floats of the weight tile in LDS (32 KB)
constexpr int kHeadCols = 16;  // a head row in LDS and in the seed tables: A <= 16 logits, or k <= 8 locs at 0.. and k log-scales at kNormalLs..
constexpr int kNormalLs = 8;
static_assert(kRows * kHeadCols == kThreads, "one thread per column of a workgroup's head rows (k_notsac_pi_rows zeroes them so)");

// Linear + ReLU layers 0..L-1, then Linear layer L; weights in torch's [out][in] layout.  Scalar fields and selects, no arrays: a kernel-argument array indexed by
// a run-time layer number is copied to scratch memory.
struct Layers {
    int In, L, Out;  // inputs of layer 0, hidden layers, outputs of layer L
    int W0, W1, W2;
    const float *w0, *w1, *w2, *w3, *b0, *b1, *b2, *b3;
    __device__ int width(int l) const { return l == 0 ? W0 : (l == 1 ? W1 : W2); }
    __device__ int in_of(int l) const { return l == 0 ? In : width(l - 1); }
    __device__ int out_of(int l) const { return l < L ? width(l) : Out; }
    __device__ const float *weight(int l) const { return l == 0 ? w0 : (l == 1 ? w1 : (l == 2 ? w2 : w3)); }
    __device__ const float *bias(int l) const { return l == 0 ? b0 : (l == 1 ? b1 : (l == 2 ? b2 : b3)); }
};

__device__ __forceinline__ float fma_acc(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_acc(double a, double b, double c) { return __builtin_fma(a, b, c); }

// one k step of dense(): acc[j] += w * x[row j of this thread's row group][k]
template <typename Acc>
__device__ __forceinline__ void dense_step(Acc (&acc)[kRows], Acc w, const float *x, int sx, int k, int g, int G, int nr) {
#pragma unroll
    for (int j = 0; j < kRows; j++)
        if (j < nr) acc[j] = fma_acc(w, (Acc)x[(g + j * G) * sx + k], acc[j]);
}

// y[r][u] = act(sum_k W[u][k] x[r][k] + b[u]) for rows r < rows (<= kRows), both in LDS with row strides sx / sy.  The weight goes through LDS: a tile of whole
// [out][in] rows (as many units as kWTile floats hold, row stride In + 1) is loaded by the whole workgroup with coalesced reads, then thread -> (unit, row group):
// a tile narrower than the workgroup runs kThreads / units row groups side by side; each thread keeps its rows' sums in registers.  Every thread of the
// workgroup must call this (it holds barriers).
//
// Acc = double: tensors stay float32; every sum ACCUMULATES in float64 (a product of two float32 values is exact there) and is rounded to float32 once, here, in
// backward_rows and in the batch sum of k_sacd_grad.  Why: Adam's first steps are lr g / (|g| + eps), so a gradient entry that cancels to about eps (1e-8 beside
// terms of 1e-3) turns its relative error into a parameter error of up to lr; with float32 chains of 272 and 512 terms in front of it such an entry was 30 % off
// (DESIGN.md 7m).
template <typename Acc>
__device__ __forceinline__ void dense(const float *__restrict__ Wt, const float *__restrict__ bias, int In, int Out, int rows, const float *x, int sx, float *y, int sy,
                                      bool relu, float *wl) {
    const int t = threadIdx.x;
    const int ws = In + 1;
    const int tu_max = kWTile / ws < Out ? kWTile / ws : Out;
    for (int u0 = 0; u0 < Out; u0 += tu_max) {
        const int tu = Out - u0 < tu_max ? Out - u0 : tu_max;
        __syncthreads();  // (the previous tile's readers are done)
        const float *src = Wt + (i64)u0 * In;
        for (int i = t; i < tu * In; i += kThreads) wl[(i / In) * ws + i % In] = src[i];
        __syncthreads();
        const int uc = tu < kThreads ? tu : kThreads;
        const int G = kThreads / uc;
        const int g = t / uc, ul = t % uc;
        if (g >= G) continue;
        const int nr = g < rows ? (rows - g + G - 1) / G : 0;
        for (int u = ul; u < tu; u += uc) {
            Acc acc[kRows];
#pragma unroll
            for (int j = 0; j < kRows; j++) acc[j] = (Acc)0;
            const float *wr = wl + u * ws;
            if constexpr (sizeof(Acc) == sizeof(double)) {
#pragma unroll 4  // (four steps' LDS reads in flight; each row's chain of fused multiply-adds keeps its order)
                for (int k = 0; k < In; k++) dense_step<Acc>(acc, (Acc)wr[k], x, sx, k, g, G, nr);
            } else {
                for (int k = 0; k < In; k++) dense_step<Acc>(acc, (Acc)wr[k], x, sx, k, g, G, nr);
            }
            const Acc bu = (Acc)bias[u0 + u];
#pragma unroll
            for (int j = 0; j < kRows; j++)
                if (j < nr) {
                    const float z = (float)(acc[j] + bu);
                    y[(g + j * G) * sy + u0 + u] = relu ? (z > 0.f ? z : 0.f) : z;
                }
        }
    }
}

// layers 0..layers-1 (layers <= L + 1) over the rows in buf0 (In columns); returns the buffer that holds the last layer's output rows, behind a barrier.
// `keep` (global; plane l: [max_batch][W_l] dense, NULL: not kept) receives rows 0..kept-1 of every hidden layer's output as rows keep_row0.. of the plane.
template <typename Acc>
__device__ __forceinline__ float *forward_rows(const Layers &n, int layers, int rows, float *buf0, float *buf1, int S, float *wl, float *keep, i64 keep_plane,
                                               i64 keep_row0, int kept) {
    float *cur = buf0, *nxt = buf1;
    for (int l = 0; l < layers; l++) {
        const int In = n.in_of(l), Out = n.out_of(l);
        dense<Acc>(n.weight(l), n.bias(l), In, Out, rows, cur, S, nxt, S, l < n.L, wl);
        __syncthreads();
        if (keep && l < n.L)
            for (int p = threadIdx.x; p < kept * Out; p += kThreads) keep[l * keep_plane + (keep_row0 + p / Out) * Out + p % Out] = nxt[(p / Out) * S + p % Out];
        float *tmp = cur;
        cur = nxt, nxt = tmp;
    }
    return cur;
}

// d loss / d h_l for l = top..0 and rows i0..i0+nb-1, row by row; every step takes its ReLU mask from the kept plane, writes the LDS rows `dcur` and the plane
// of dh, synchronises and swaps the two buffers.  Layers below `top` read the `dnext` rows (stride S) through weight(l + 1).  So does layer `top` with the
// default Seed: `dnext` then holds the rows' d loss / d (output of layer top + 1) (SAC: top = L - 1, the out layer's rows).  With a callable,
// d h_top[r][k] = seed(r, k, W_top) before the mask: a head whose gradient is sparse in a way only the caller knows (srlx_mlpq.hip).
struct ThroughWeight {
    __device__ float operator()(int, int, int) const { return 0.f; }
};
template <typename Acc, typename Seed = ThroughWeight>
__device__ __forceinline__ void backward_rows(const Layers &n, int top, int nb, i64 i0, float *dcur, float *dnext, int S, const float *h, float *dh, i64 plane,
                                              Seed seed = Seed()) {
    constexpr bool seeded = !std::is_same<Seed, ThroughWeight>::value;
    for (int l = top; l >= 0; l--) {
        const int Wl = n.width(l);
        const float *hl = h + (i64)l * plane;
        float *dhl = dh + (i64)l * plane;
        for (int p = threadIdx.x; p < nb * Wl; p += kThreads) {
            const int r = p / Wl, k = p % Wl;
            float g;
            if (seeded && l == top) {
                g = seed(r, k, Wl);
            } else {
                const int Wn = n.out_of(l + 1);
                const float *wn = n.weight(l + 1);
                Acc acc = (Acc)0;
#pragma unroll 8
                for (int u = 0; u < Wn; u++) acc = fma_acc((Acc)dnext[r * S + u], (Acc)wn[(i64)u * Wl + k], acc);
                g = (float)acc;
            }
            g = hl[(i0 + r) * Wl + k] > 0.f ? g : 0.f;
            dcur[r * S + k] = g;
            dhl[(i0 + r) * Wl + k] = g;
        }
        __syncthreads();
        float *tmp = dcur;
        dcur = dnext, dnext = tmp;
    }
}

// d loss / d h of a layer that up to three Linear layers read: sum over their output rows' seeds through their weights, one float64 chain
struct Src {
    const float *d;  // [rows][stride]
    int stride, n;   // n = 0: none
    const float *w;  // [n][W of the layer below]
};
struct SumSeed {
    Src a, b, c;
    __device__ float operator()(int r, int k, int Wl) const {
        double acc = 0.0;
#pragma unroll 4
        for (int u = 0; u < a.n; u++) acc = fma_acc((double)a.d[r * a.stride + u], (double)a.w[(i64)u * Wl + k], acc);
        for (int u = 0; u < b.n; u++) acc = fma_acc((double)b.d[r * b.stride + u], (double)b.w[(i64)u * Wl + k], acc);
        for (int u = 0; u < c.n; u++) acc = fma_acc((double)c.d[r * c.stride + u], (double)c.w[(i64)u * Wl + k], acc);
        return (float)acc;
    }
};

// The head rows of a policy chain `pol` whose out layer's rows are `z` and whose head reads the rows `hin` (both LDS, stride S): zs[r][kHeadCols] = logits, or
// locs at 0.. and, through the Normal head's second Linear (w_ls NULL: none) and the free buffer b2, RAW log-scales at kNormalLs...  Ends behind a barrier.
__device__ __forceinline__ void head_rows(const Layers &pol, const float *w_ls, const float *b_ls, int nb, const float *z, const float *hin, float *b2, int S, float *wl,
                                          float *zs) {
    const int t = threadIdx.x, HO = pol.Out;
    if (t < nb * HO) zs[(t / HO) * kHeadCols + t % HO] = z[(t / HO) * S + t % HO];
    if (w_ls) {
        dense<double>(w_ls, b_ls, pol.in_of(pol.L), HO, nb, hin, S, b2, S, false, wl);
        __syncthreads();
        if (t < nb * HO) zs[(t / HO) * kHeadCols + kNormalLs + t % HO] = b2[(t / HO) * S + t % HO];
    }
    __syncthreads();
}

}  // namespace srlxm
