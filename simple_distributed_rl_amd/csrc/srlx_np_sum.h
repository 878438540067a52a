// srlx_np_sum.h -- numpy's float32 pairwise summation, shared by every kernel that restates an np.sum / np.mean of the reference
// (srlx_ngu.hip: the pseudo-count formula and the RND error; srlx_td_math.h: the n-step discounted sum).
#pragma once
#include <stdint.h>

namespace srlx {

// One leaf of numpy's float32 pairwise summation (numpy/_core/src/umath/loops_utils.h.src), n <= 128 terms f(lo) .. f(lo + n - 1): a plain loop below 8
// terms, 8 partial sums and then the tail from 8 up.  No call, no stack: it inlines into its caller.  f is evaluated once per index, in increasing order
// of the index, so it may carry state from one term to the next.
template <typename F>
__device__ __forceinline__ float np_sum_leaf(F &&f, int64_t lo, int64_t n) {
    if (n < 8) {
        float acc = 0.f;  // numpy starts from -0.0; the same bits unless every term is -0.0
        for (int64_t i = 0; i < n; i++) acc = acc + f(lo + i);
        return acc;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = f(lo + j);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = r[j] + f(lo + i + j);
    }
    float acc = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) acc = acc + f(lo + i);
    return acc;
}

// The same leaf, the same order of additions, with ONE copy of f's body: a single rolled loop in which term i joins partial sum i mod 8 (a select over the
// eight registers, no indexed array), for callers whose f is large -- td_rows' term is a masked argmax, two rescalings and a retrace product, and seventeen
// inlined copies of it cost the backward pass's head kernels a wave of occupancy.  Below 8 terms the loop body is acc = acc + f(i) and nothing else.
template <typename F>
__device__ __forceinline__ float np_sum_leaf_rolled(F &&f, int n) {
    const int nb = n < 8 ? 0 : n - (n % 8);  // terms that go through the 8 partial sums
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f, r4 = 0.f, r5 = 0.f, r6 = 0.f, r7 = 0.f, acc = 0.f;  // numpy starts a short sum from -0.0: see np_sum_leaf
    for (int i = 0; i < n; i++) {
        const float t = f(i);
        if (i < nb) {
            const int j = i & 7;
            const bool first = i < 8;  // the partial sums START as terms 0..7 (no 0 + t)
            r0 = j == 0 ? (first ? t : r0 + t) : r0;
            r1 = j == 1 ? (first ? t : r1 + t) : r1;
            r2 = j == 2 ? (first ? t : r2 + t) : r2;
            r3 = j == 3 ? (first ? t : r3 + t) : r3;
            r4 = j == 4 ? (first ? t : r4 + t) : r4;
            r5 = j == 5 ? (first ? t : r5 + t) : r5;
            r6 = j == 6 ? (first ? t : r6 + t) : r6;
            r7 = j == 7 ? (first ? t : r7 + t) : r7;
            if (i + 1 == nb) acc = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        } else {
            acc = acc + t;  // every term below 8 terms; the tail behind the partial sums from 8 up
        }
    }
    return acc;
}

// The whole summation over f(lo) .. f(lo + n - 1): the leaf up to 128 terms, recursive halving above (a real call with a stack: for kernels whose sums can be
// that long; a kernel that knows n <= 128 calls np_sum_leaf itself).
template <typename F>
__device__ float np_pairwise_sum(const F &f, int64_t lo, int64_t n) {
    if (n <= 128) return np_sum_leaf(f, lo, n);
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(f, lo, n2) + np_pairwise_sum(f, lo + n2, n - n2);
}

}  // namespace srlx
