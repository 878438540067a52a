// srlx_c51_math.h -- the arithmetic of Categorical DQN (C51; srl/algorithms/c51/c51.py:64-142, :150-174), held once: the fused learner kernel and the
// categorical actor tail of srlx_mlpq.hip and the one-purpose loss kernel behind the plugin trainer (srlx_c51_loss) call these functions, so they give one set of
// bits.  tests/c51_reference.py restates the same lines in float64 as a different program (a scatter where this is a gather).
//
// The head, exactly:
//   support     z_j = v_min + j * ((v_max - v_min) / (N - 1)) in float64, two roundings, as np.linspace computes it (c51.py:67); the last atom is v_max itself.
//               Expectations multiply by float32(z_j): TensorFlow casts Z to the probabilities' float32 (:93, :167).
//   softmax     float32: mx = max_j x_j; s = sum_j expf(x_j - mx), j ascending from 0.f; p_j = expf(x_j - mx) / s.
//   expectation q = sum_j p_j * float32(z_j), j ascending; the products and their sum in float64, rounded to float32 once (a float32 sum over atoms of +-v_max
//               would carry about N ulp of v_max into a mean that is often near 0).
//   next action the first maximum of the float32 expectations of s' (:94; tf.argmax).
//   projection  (:102-121) TZ_j = clip(r + ((1 - done) * discount) * z_j, v_min, v_max), b_j = (TZ_j - v_min) / delta_z, (ratio_j, idx_j) = modf(b_j), all in
//               float64 from the float32 reward, as numpy does there.  Written as a GATHER: the thread of target atom i walks j = 0..N-1 in ascending order and adds
//               p_j * (1 - ratio_j) when idx_j == i, p_j * ratio_j when idx_j + 1 == i and ratio_j != 0, in float64.  One j never feeds the same i twice, so per
//               destination this is the reference's scatter order: no atomics, bit-reproducible.  m_i is rounded to float32 once at the end (TensorFlow casts
//               target_dists).  GUARD: idx_j >= N - 1 puts the whole mass p_j on atom N - 1 -- TZ_j = v_max lands there with ratio 0 anyway, and where the
//               division rounds b_j a hair above N - 1 the reference would index target_dists[N] out of range.
//   loss        (:130-135) per item -sum_i m_i * logf(clip(p_i, 1e-6, 1)), the terms and their sum in float64, i ascending; the mean over the batch is taken by
//               whoever reduces the row terms (k_mlpq_grad_adam; k_c51_loss's thread 0), in item order.
//   seeds       tf.clip_by_value passes the gradient where 1e-6 <= p_i <= 1, bounds included.  With u_i = m_i there and 0 elsewhere, the softmax backward in its
//               division-free form: d loss / d logit[a_0][k] = (p_k * sum_i u_i - u_k) / B (float64, rounded once); m_i / p_i is never formed.  Every other
//               action's logits get 0.
#pragma once
#include "srlx_common.h"

namespace srlxc {

using i64 = int64_t;

constexpr int kMaxAtoms = 256;   // n_atoms of a handle (item rows in LDS have this stride)
constexpr int kMaxActions = 32;
constexpr float kClipLo = 1e-6f;  // c51.py:131

__device__ __forceinline__ double delta_z(double v_min, double v_max, int N) { return (v_max - v_min) / (double)(N - 1); }

__device__ __forceinline__ double atom64(double v_min, double v_max, double dz, int N, int j) { return j == N - 1 ? v_max : (double)j * dz + v_min; }

__device__ __forceinline__ void softmax_stats(const float *x, int N, float &mx, float &s) {
    float m = x[0];
    for (int j = 1; j < N; j++) m = fmaxf(m, x[j]);
    float sum = 0.f;
    for (int j = 0; j < N; j++) sum += expf(x[j] - m);
    mx = m, s = sum;
}

__device__ __forceinline__ float prob(float x, float mx, float s) { return expf(x - mx) / s; }

// E[Z] of one action's N logits
__device__ __forceinline__ float expectation(const float *x, int N, double v_min, double v_max) {
    float mx, s;
    softmax_stats(x, N, mx, s);
    const double dz = delta_z(v_min, v_max, N);
    double q = 0.0;
    for (int j = 0; j < N; j++) q += (double)prob(x[j], mx, s) * (double)(float)atom64(v_min, v_max, dz, N, j);
    return (float)q;
}

__device__ __forceinline__ int first_max(const float *q, int A) {
    int act = 0;
    float best = q[0];
    for (int a = 1; a < A; a++)
        if (q[a] > best) act = a, best = q[a];
    return act;
}

// m_i of one item: the mass the projected next distribution `pn` puts on atom i
__device__ __forceinline__ float project_atom(const float *pn, int N, int i, float reward, float terminated, double discount, double v_min, double v_max) {
    const double dz = delta_z(v_min, v_max, N);
    const double r = (double)reward, g = (1.0 - (double)terminated) * discount;
    double acc = 0.0;
    for (int j = 0; j < N; j++) {
        double tz = r + g * atom64(v_min, v_max, dz, N, j);
        tz = fmin(v_max, fmax(v_min, tz));
        const double b = (tz - v_min) / dz;
        double whole;
        double ratio = modf(b, &whole);
        int idx = (int)whole;
        if (idx >= N - 1) idx = N - 1, ratio = 0.0;  // the guard above
        const double p = (double)pn[j];
        if (idx == i) acc += p * (1.0 - ratio);
        if (idx + 1 == i && ratio != 0.0) acc += p * ratio;
    }
    return (float)acc;
}

struct Items {
    i64 B;
    int A, N;
    double v_min, v_max, discount;
    const int32_t *actions;             // [B]
    const float *rewards, *terminated;  // [B]
    float *q0;         // [B][A] expectations of s (NULL: not written)
    float *p0, *m;     // [B][N]: softmax of a_0's logits, the projected target
    float *grad;       // [B][A * N]: d loss / d logits of s
    float *item_loss;  // [B] (NULL: not written)
};

// The update's item arithmetic for items i0..i0+nb-1 (nb <= ITEMS) by the whole workgroup: lg0 / lg1 = the items' logit rows of s and s' ([A][N] each, `stride`
// floats from one item to the next; LDS or global memory).  pn / p0 / ms: ITEMS * kMaxAtoms floats of LDS each; on return p0 holds the seeds of a_0's N logits,
// act0[r] the item's action and row_loss[r] its float64 loss term (act0, row_loss: LDS).  Every thread of the workgroup must call this (it holds barriers).
template <int ITEMS>
__device__ __forceinline__ void items_step(const Items &a, i64 i0, int nb, const float *lg0, const float *lg1, i64 stride, float *pn, float *p0, float *ms, int *act0,
                                           double *row_loss) {
    __shared__ float qn[ITEMS * kMaxActions];
    __shared__ float mx[2 * ITEMS], sum[2 * ITEMS];
    __shared__ int anext[ITEMS];
    __shared__ double usum[ITEMS];
    const int t = threadIdx.x, nt = blockDim.x, A = a.A, N = a.N;
    for (int p = t; p < 2 * nb * A; p += nt) {  // one thread per (row, action): the expectations of s (out) and of s' (the greedy next action)
        const int which = p / (nb * A), r = (p % (nb * A)) / A, c = p % A;
        const float q = expectation((which ? lg1 : lg0) + r * stride + c * N, N, a.v_min, a.v_max);
        if (which)
            qn[r * kMaxActions + c] = q;
        else if (a.q0)
            a.q0[(i0 + r) * A + c] = q;
    }
    __syncthreads();
    if (t < 2 * nb) {  // a* = argmax E[Z(s', .)] (:94), a_0; the softmax statistics of the two selected rows
        const int which = t / nb, r = t % nb;
        int act;
        if (which) {
            act = first_max(qn + r * kMaxActions, A);
            anext[r] = act;
        } else {
            act = a.actions[i0 + r];
            act = act < 0 ? 0 : (act >= A ? A - 1 : act);  // (an action outside the space must not become an address)
            act0[r] = act;
        }
        softmax_stats((which ? lg1 : lg0) + r * stride + act * N, N, mx[which * ITEMS + r], sum[which * ITEMS + r]);
    }
    __syncthreads();
    for (int p = t; p < 2 * nb * N; p += nt) {
        const int which = p / (nb * N), r = (p % (nb * N)) / N, j = p % N;
        if (which) {
            pn[r * kMaxAtoms + j] = prob(lg1[r * stride + anext[r] * N + j], mx[ITEMS + r], sum[ITEMS + r]);
        } else {
            const float pr = prob(lg0[r * stride + act0[r] * N + j], mx[r], sum[r]);
            p0[r * kMaxAtoms + j] = pr;
            a.p0[(i0 + r) * N + j] = pr;
        }
    }
    __syncthreads();
    for (int p = t; p < nb * N; p += nt) {  // one thread per (item, target atom)
        const int r = p / N, i = p % N;
        const float mi = project_atom(pn + r * kMaxAtoms, N, i, a.rewards[i0 + r], a.terminated[i0 + r], a.discount, a.v_min, a.v_max);
        ms[r * kMaxAtoms + i] = mi;
        a.m[(i0 + r) * N + i] = mi;
    }
    __syncthreads();
    if (t < nb) {
        double l = 0.0, u = 0.0;
        for (int i = 0; i < N; i++) {
            const float pi = p0[t * kMaxAtoms + i], mi = ms[t * kMaxAtoms + i];
            const float pc = pi < kClipLo ? kClipLo : (pi > 1.0f ? 1.0f : pi);
            l += (double)mi * (double)logf(pc);
            if (pi >= kClipLo && pi <= 1.0f) u += (double)mi;
        }
        row_loss[t] = -l;
        usum[t] = u;
        if (a.item_loss) a.item_loss[i0 + t] = (float)(-l);
    }
    __syncthreads();
    for (int p = t; p < nb * N; p += nt) {
        const int r = p / N, k = p % N;
        const float pk = p0[r * kMaxAtoms + k];
        const double uk = (pk >= kClipLo && pk <= 1.0f) ? (double)ms[r * kMaxAtoms + k] : 0.0;
        p0[r * kMaxAtoms + k] = (float)(((double)pk * usum[r] - uk) / (double)a.B);
    }
    __syncthreads();
    for (int p = t; p < nb * A * N; p += nt) {
        const int r = p / (A * N), c = p % (A * N), blk = c / N;
        a.grad[(i0 + r) * A * N + c] = blk == act0[r] ? p0[r * kMaxAtoms + c - blk * N] : 0.f;
    }
    __syncthreads();
}

}  // namespace srlxc
