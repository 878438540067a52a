// srlx_mlp_walk.h -- a whole MLP forward of 16 rows in ONE workgroup on v_mfma_f64_16x16x4_f64, the activations in LDS.
// The device pieces are k_dqnnot_act's (srlx_dqnnot.hip), lifted here unchanged: a plane's layout (act_slot, ld), the tile loop that takes the weights from L2
// straight into the B fragment (act_tiles) and one pass of Linear + ReLU over 1 or 2 weight matrices (act_layer).  On top of them k_mlp_walk walks ANY network
// that a small pass table in its kernel arguments describes, and WalkPlan is the host function that writes that table: which pass reads and writes which
// plane, and how many planes the network needs.  srlx_vppo_walk and srlx_notsac_walk are its two callers.
//
// The contract is srlx_mlp_gemm.h's: float32 operands widened at the fragment read, exact products, float64 sums in a fixed order, ONE rounding per Linear in
// the epilogue that adds the bias in float64 (and applies ReLU on the way into LDS).  No atomics; a row's result knows neither n nor the row's place.
#pragma once
#include "srlx_mlp_gemm.h"

namespace srlxw {

using i64 = int64_t;

constexpr int kWaves = 16, kThreads = 64 * kWaves;
constexpr int kRows = 16;   // rows of a workgroup: the M of one MFMA tile
constexpr int kStep = 32;   // reduction indices per step
constexpr i64 kMaxRows = 65536;
constexpr int kLdsLimit = 163840;  // gfx950's LDS per workgroup

constexpr int ld(int K) { return (K + kStep - 1) / kStep * kStep + 4; }  // a plane's row stride in floats: 4 * odd

// where a plane keeps reduction index k of a row
__device__ __forceinline__ int act_slot(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

__device__ __forceinline__ float quad_at(const float4 &q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }

// kT column tiles over the K reduction indices of one plane: acc[i] += sum_k plane[row][k] w[i][k].  `a`: the plane at this lane's row and lane group;
// w[i]: this lane's weight row of tile i.  live[i] false: the lane's column does not exist; w[i] is then the weight's first row, the lane computes a column
// nobody stores (a column's B operand reaches that column's sums only), and only the masked last step asks.
// The K / 32 full steps load WITHOUT a condition: a branch around a load makes the compiler wait for every load in flight where the branch ends, which put
// each quad's latency in front of the MFMAs (measured: 128 us per call at U 512 against 80 us without).  Two steps per trip on two sets of registers; a
// step's quads are requested before the MFMAs of the step in front of it, and the request behind the last full step repeats that step's.  What is left of K
// (the first layer's D, where it is no multiple of 32) is one more step on load_quad, masked at K.
template <int kT, bool kVec>
__device__ __forceinline__ void act_tiles(const float *a, int K, const float *const (&w)[kT], const bool (&live)[kT], srlxg::f64x4 (&acc)[kT]) {
    const int g4 = ((threadIdx.x & 63) >> 4) << 2;
    float4 q0[kT][2], q1[kT][2];
    auto fetch = [&](float4(&q)[kT][2], int k0) {
#pragma unroll
        for (int i = 0; i < kT; i++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const float *p = w[i] + k0 + 16 * s + g4;
                if constexpr (kVec) q[i][s] = *reinterpret_cast<const float4 *>(p);
                else q[i][s] = make_float4(p[0], p[1], p[2], p[3]);
            }
    };
    auto step = [&](const float4(&q)[kT][2], int k0) {
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double av = (double)a[k0 + 16 * s + 4 * j];
#pragma unroll
                for (int i = 0; i < kT; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, (double)quad_at(q[i][s], j), acc[i], 0, 0, 0);
            }
    };
    const int full = K / kStep;
    if (full > 0) {
        const int last = (full - 1) * kStep;
        int k0 = 0;
        fetch(q0, 0);
        for (; k0 < last; k0 += 2 * kStep) {  // (nothing conditional inside: the compiler moves a load whose values one branch reads into that branch)
            fetch(q1, k0 + kStep);
            step(q0, k0);
            fetch(q0, min(k0 + 2 * kStep, last));
            step(q1, k0 + kStep);
        }
        if (k0 == last) step(q0, last);  // an odd number of steps: q0 holds the last one's quads
    }
    if (K % kStep) {
        const int k0 = full * kStep;
#pragma unroll
        for (int i = 0; i < kT; i++)
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int k = k0 + 16 * s + g4;
                q0[i][s] = srlxg::load_quad(w[i] + k, live[i] ? K - k : 0, kVec);
            }
        step(q0, k0);
    }
}

// One pass of Linear + ReLU from the plane `in` (K reduction indices, row stride ldin): column tiles 0..UT-1 are (w0, b0) into out0, tiles UT.. (w1, b1) into
// out1 -- U = 16 UT output columns of the first matrix, 16 (NT - UT) of the second, which need not be as many.  Every wave takes its tiles two at a time; no
// barrier inside.
__device__ __forceinline__ void act_layer(const float *in, int ldin, int K, int U, int NT, const float *w0, const float *b0, float *out0, const float *w1,
                                          const float *b1, float *out1, int ldout) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, g = lane >> 4;
    const int UT = U / 16;
    const bool vec = K % 4 == 0 && srlxg::aligned16(w0) && srlxg::aligned16(w1);
    const float *a = in + fr * ldin + g;
    for (int t = wave; t < NT; t += 2 * kWaves) {
        const float *w[2], *b[2];
        float *o[2];
        int col[2];
        bool live[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int ti = t + i * kWaves;
            const bool second = ti >= UT;
            col[i] = (ti - (second ? UT : 0)) * 16 + fr;
            const float *base = second ? w1 : w0;
            live[i] = ti < NT;
            w[i] = base + (live[i] ? (i64)col[i] * K : 0);
            b[i] = second ? b1 : b0, o[i] = second ? out1 : out0;
        }
        srlxg::f64x4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        if (vec) act_tiles<2, true>(a, K, w, live, acc);
        else act_tiles<2, false>(a, K, w, live, acc);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (!live[i]) continue;
            const double bias = (double)b[i][col[i]];
            float *dst = o[i] + act_slot(col[i]);
#pragma unroll
            for (int r = 0; r < 4; r++) {  // (D layout: register r is row 4 r + l / 16)
                const float z = (float)(acc[i][r] + bias);
                dst[(4 * r + g) * ldout] = z > 0.f ? z : 0.f;
            }
        }
    }
}

// ---- the general walk ------------------------------------------------------------------------------------------------------------------------
// k_mlp_walk.  Grid ceil(n / 16); a workgroup of kWaves waves owns 16 rows and walks `np` passes of act_layer, one barrier behind each, then the heads.  Dynamic
// LDS: x as [16][ld(D)] and `planes` planes [16][ldu], ldu = ld(widest hidden layer); plane -1 is x.  Rows >= n are zero on load and never stored; no thread
// leaves before the last barrier.
// The heads are one more round of act_tiles without ReLU, written straight to global memory: wave 0 runs the value head (one live column) when there is one,
// wave 1 the distribution head -- n_out logit columns, or n_out loc columns and behind them n_out log-scale columns in ONE tile (2 n_out <= 16; a lane's weight
// row is its own, so the two Linears share the tile).  A log-scale is rounded once and then clamped to [ls_lo, ls_hi] in float32, srlx_vppo_forward's rule.
constexpr int kMaxPasses = 6;  // V-PPO: 3 trunk layers, value_block.0 || policy_block.0, value_block.1, policy_block.1
constexpr int kMaxPlanes = 3;  // what WalkPlan ever hands out (7za: the trunk's output and one more per branch, or the trunk's ping-pong pair)

struct Pass {
    const float *w0, *b0, *w1, *b1;  // a one-matrix pass: w1 = w0, b1 = b0
    int in, out0, out1;              // planes; in -1: x
    int K, U, NT;                    // reduction length, the first matrix's columns, column tiles of both
};
struct Heads {
    const float *wv, *bv;            // value_out_layer [1][Kv], NULL: no value head
    const float *w0, *b0, *w1, *b1;  // [n_out][Kp]: logits or locs; log-scales (NULL: a logit head)
    int in_v, Kv, in_p, Kp, n_out;
    float ls_lo, ls_hi;
};
struct WalkArgs {
    i64 n;
    int D, ldu, np;
    const float *x;            // [n][D]
    float *v, *head0, *head1;  // [n], [n][n_out], [n][n_out]
    Heads h;
    Pass pass[kMaxPasses];
};

static SRLXG_KERNEL void __launch_bounds__(kThreads) k_mlp_walk(WalkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float walk_lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fr = lane & 15, g = lane >> 4;
    const int D = a.D, Dp = ld(D) - 4, ldx = ld(D), ldu = a.ldu;
    float *xs = walk_lds, *planes = xs + kRows * ldx;
    const i64 row0 = (i64)blockIdx.x * kRows;

    for (int i = t; i < kRows * Dp; i += kThreads) {  // rows >= n and the padding behind D: zero
        const int r = i / Dp, k = i - r * Dp;
        xs[r * ldx + act_slot(k)] = row0 + r < a.n && k < D ? a.x[(row0 + r) * D + k] : 0.f;
    }
    __syncthreads();
    for (int p = 0; p < a.np; p++) {  // (uniform: every thread meets every barrier)
        const Pass &ps = a.pass[p];
        const bool from_x = ps.in < 0;
        act_layer(from_x ? xs : planes + ps.in * kRows * ldu, from_x ? ldx : ldu, ps.K, ps.U, ps.NT, ps.w0, ps.b0, planes + ps.out0 * kRows * ldu, ps.w1, ps.b1,
                  planes + ps.out1 * kRows * ldu, ldu);
        __syncthreads();  // (the last pass's is the workgroup's last barrier)
    }
    const Heads &h = a.h;
    const bool isv = wave == 0;
    if (isv ? h.wv != nullptr : wave == 1) {  // (wave-uniform; no barrier inside)
        const bool normal = h.w1 != nullptr;
        const int K = isv ? h.Kv : h.Kp, cols = isv ? 1 : (normal ? 2 * h.n_out : h.n_out);
        const bool ls = !isv && fr >= h.n_out;  // (a live column behind the locs)
        const int col = ls ? fr - h.n_out : fr;
        const float *hw = isv ? h.wv : (ls ? h.w1 : h.w0), *hb = isv ? h.bv : (ls ? h.b1 : h.b0);
        const bool live[1] = {fr < cols};
        const float *w[1] = {live[0] ? hw + (i64)col * K : (isv ? h.wv : h.w0)};
        srlxg::f64x4 acc[1] = {{0.0, 0.0, 0.0, 0.0}};
        const float *ha = planes + (isv ? h.in_v : h.in_p) * kRows * ldu + fr * ldu + g;
        if (isv ? srlxg::aligned16(h.wv) : srlxg::aligned16(h.w0) && srlxg::aligned16(h.w1)) act_tiles<1, true>(ha, K, w, live, acc);  // (K is a multiple of 32)
        else act_tiles<1, false>(ha, K, w, live, acc);
        if (live[0]) {
            const double bias = (double)hb[col];
            float *dst = isv ? a.v : (ls ? a.head1 : a.head0);
            const int stride = isv ? 1 : h.n_out;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const i64 row = row0 + 4 * r + g;
                const float z = (float)(acc[0][r] + bias);
                if (row < a.n) dst[row * stride + col] = ls ? fminf(fmaxf(z, h.ls_lo), h.ls_hi) : z;
            }
        }
    }
}

// ---- the host's plan -----------------------------------------------------------------------------------------------------------------------------------------
// WalkPlan writes the pass table.  A caller adds its passes in walk order with VALUES for activations (0 is x, `pass` returns the new ones), names the values
// the heads read, and `finish` gives every value a plane: a value keeps its plane up to its last reader, a pass's outputs take the lowest planes that are free
// while the pass runs (its own input's is not).  So the trunk ping-pongs on two planes, a branch moves into whatever its sibling has let go, and no network of
// the envelope needs more than kMaxPlanes.  `lds_bytes` is the launch's dynamic LDS; `finish` refuses what does not fit kMaxPlanes or gfx950's LDS.
struct WalkPlan {
    WalkArgs a{};
    int planes = 0, umax = 0;
    int vin[kMaxPasses], vout[kMaxPasses][2], v_value = -1, v_dist = -1, nval = 1;
    bool overflow = false;  // more passes than the table holds

    // Linear(K, U) + ReLU from value `in`; with w1: Linear(K, U1) + ReLU beside it on the same read of `in`.  Returns the first output's value; the second's is
    // the next one.
    int pass(int in, int K, const float *w0, const float *b0, int U, const float *w1 = nullptr, const float *b1 = nullptr, int U1 = 0) {
        if (a.np == kMaxPasses) {
            overflow = true;
            return 0;
        }
        Pass &p = a.pass[a.np];
        p = Pass{w0, b0, w1 ? w1 : w0, w1 ? b1 : b0, 0, 0, 0, K, U, (U + U1) / 16};
        vin[a.np] = in, vout[a.np][0] = nval++, vout[a.np][1] = w1 ? nval++ : -1;
        umax = U > umax ? U : umax, umax = U1 > umax ? U1 : umax;
        return vout[a.np++][0];
    }
    void value_head(int in, int K, const float *w, const float *b) { v_value = in, a.h.Kv = K, a.h.wv = w, a.h.bv = b; }
    void dist_head(int in, int K, int n_out, const float *w0, const float *b0, const float *w1, const float *b1) {
        v_dist = in, a.h.Kp = K, a.h.n_out = n_out, a.h.w0 = w0, a.h.b0 = b0, a.h.w1 = w1, a.h.b1 = b1;
    }
    size_t lds_bytes() const { return sizeof(float) * kRows * ((size_t)ld(a.D) + (size_t)planes * a.ldu); }

    bool finish(int D) {
        if (overflow) return false;
        a.D = D, a.ldu = ld(umax);
        int last[2 * kMaxPasses + 1], plane_of[2 * kMaxPasses + 1], holder[kMaxPlanes];  // a value's last reader (a.np: a head) and plane; a plane's value
        for (int v = 0; v < nval; v++) last[v] = -1, plane_of[v] = -1;
        for (int p = 0; p < a.np; p++) last[vin[p]] = p;
        if (v_value > 0) last[v_value] = a.np;
        if (v_dist > 0) last[v_dist] = a.np;
        for (int k = 0; k < kMaxPlanes; k++) holder[k] = -1;
        for (int p = 0; p < a.np; p++) {
            for (int k = 0; k < kMaxPlanes; k++)
                if (holder[k] >= 0 && last[holder[k]] < p) holder[k] = -1;
            for (int o = 0; o < 2; o++) {
                const int v = vout[p][o];
                if (v < 0) continue;
                int k = 0;
                while (k < kMaxPlanes && holder[k] >= 0) k++;
                if (k == kMaxPlanes) return false;
                holder[k] = v, plane_of[v] = k, planes = k + 1 > planes ? k + 1 : planes;
            }
            a.pass[p].in = plane_of[vin[p]], a.pass[p].out0 = plane_of[vout[p][0]], a.pass[p].out1 = plane_of[vout[p][vout[p][1] < 0 ? 0 : 1]];
        }
        if (v_dist <= 0 || (a.h.wv && v_value <= 0)) return false;  // (a head reads a hidden plane, never x)
        a.h.in_v = a.h.wv ? plane_of[v_value] : 0, a.h.in_p = plane_of[v_dist];
        return lds_bytes() <= (size_t)kLdsLimit;
    }
};

// the envelope's corner: D 256 and three planes of 512 units (115 712 bytes); every create raises the kernel's limit to it
constexpr size_t kLdsCap = sizeof(float) * kRows * ((size_t)ld(256) + (size_t)kMaxPlanes * ld(512));
static_assert(kLdsCap <= (size_t)kLdsLimit, "the corner fits gfx950's LDS");

inline hipError_t raise_lds_limit() { return hipFuncSetAttribute((const void *)k_mlp_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap); }

// `plan` finished; the outputs and the clamp are the call's
inline void launch(WalkPlan &plan, i64 n, const float *x, float ls_lo, float ls_hi, float *v, float *head0, float *head1, hipStream_t st) {
    WalkArgs &a = plan.a;
    a.n = n, a.x = x, a.v = v, a.head0 = head0, a.head1 = head1, a.h.ls_lo = ls_lo, a.h.ls_hi = ls_hi;
    hipLaunchKernelGGL(k_mlp_walk, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), plan.lds_bytes(), st, a);
}

}  // namespace srlxw
