// srlx_r2d2.hip -- R2D2's learner arithmetic after the forwards, in one entry point (contract: include/srlx.h, srlx_r2d2_seq_td):
//   srl/algorithms/r2d2/r2d2.py:152-209 (double-DQN gains with invalid-action masks, value rescaling, retrace with the stored acting
//   probability, backward target recursion, Huber loss of the weighted selected Q) and the per-sequence mean TD error of :204.
//
// One workgroup per batch row, three phases over LDS:
//   1. parallel over the row's S steps: the masked argmax of the selecting row, the gain, q_t[a_t] and the retrace factor
//      discount * (retrace_h * min(1, pi_t[a_t] / mu_t)) -- everything that does not depend on another step;
//   2. one thread walks t = S-1 .. 0 over those S values in LDS (the only serial part: 3 dependent double operations per step),
//      summing the row's Huber terms and TD errors in walk order;
//   3. all threads write the row's grad_q block, every entry once, as consecutive dwords.
// A second launch of one workgroup adds the B per-row loss terms in a fixed tree and clears the slot they travelled in (the first
// entry of each row's last grad_q step, which the contract wants zero).  No atomics: two calls on the same inputs give the same bits.
//
// The reference evaluates the per-(row, step) chain on Python floats; so does this file, in double, and rounds on output only.
#include "srlx_common.h"

namespace {

using i64 = int64_t;
using u8 = unsigned char;

constexpr int kThreads = 256;
constexpr int kMaxS = SRLX_SEQ_MAX_L - 1;

// srl/rl/functions.py:10-17 on doubles, in the reference's order of operations
__device__ __forceinline__ double sign_d(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }
__device__ __forceinline__ double rescaling_d(double x) { return sign_d(x) * (sqrt(fabs(x) + 1.0) - 1.0) + 0.001 * x; }
__device__ __forceinline__ double inverse_rescaling_d(double x) {
    double n = sqrt(1.0 + 4.0 * 0.001 * (fabs(x) + 1.0 + 0.001)) - 1.0;
    n = n / (2.0 * 0.001);
    return sign_d(x) * ((n * n) - 1.0);
}

struct R2d2Args {
    int B, S, A;
    const float *q, *q_target;  // [B][S+1][A]
    const int32_t *actions;     // [B][S]
    const float *mu, *rewards;  // [B][S]
    const u8 *dones;            // [B][S]
    const u8 *invalid;          // [B][S+1][A] or NULL
    const float *weights;       // [B]
    double discount, retrace_h;
    int retrace, double_dqn, rescale;
    float *target;   // [B][S]
    float *grad_q;   // [B][S+1][A]
    float *td_mean;  // [B]
};

__global__ void __launch_bounds__(kThreads) k_r2d2_seq_td(R2d2Args a) {
    __shared__ double s_gain[kMaxS];  // the gain; after the walk, the gradient seed of q_t[a_t]
    __shared__ double s_aq[kMaxS];    // q_t[a_t]
    __shared__ double s_coef[kMaxS];  // discount * (retrace_h * min(1, pi / mu))
    __shared__ int s_act[kMaxS];
    const int S = a.S, A = a.A, b = blockIdx.x;
    const i64 row = (i64)b * (S + 1) * A;
    const float *q = a.q + row, *qt = a.q_target + row;
    const u8 *inv = a.invalid ? a.invalid + row : nullptr;

    for (int t = threadIdx.x; t < S; t += kThreads) {
        const i64 bt = (i64)b * S + t;
        const int act = min(max(a.actions[bt], 0), A - 1);  // (the contract wants 0 <= action < A; nothing is read outside the row either way)
        double gain = (double)a.rewards[bt];
        if (!a.dones[bt]) {  // r2d2.py:172-182
            const float *sel = (a.double_dqn ? q : qt) + (t + 1) * A;
            const u8 *ninv = inv ? inv + (t + 1) * A : nullptr;
            int best = 0;
            float bv = 0.f;
            for (int k = 0; k < A; k++) {  // np.argmax: the first maximum
                const float v = (ninv && ninv[k]) ? -INFINITY : sel[k];
                if (k == 0 || v > bv) {
                    best = k;
                    bv = v;
                }
            }
            double maxq = (double)qt[(t + 1) * A + best];
            if (a.rescale) maxq = inverse_rescaling_d(maxq);
            gain = gain + a.discount * maxq;
        }
        if (a.rescale) gain = rescaling_d(gain);
        double coef = 0.0;
        if (a.retrace) {  // :194-202: the greedy distribution over the valid actions of q_t
            const float *cur = q + t * A;
            const u8 *cinv = inv ? inv + t * A : nullptr;
            float mx = -INFINITY;
            int n_max = 0;
            for (int k = 0; k < A; k++) {
                const float v = (cinv && cinv[k]) ? -INFINITY : cur[k];
                if (v > mx) {
                    mx = v;
                    n_max = 1;
                } else if (v == mx) {
                    n_max++;
                }
            }
            const bool greedy = !(cinv && cinv[act]) && cur[act] == mx;
            const double pi = greedy ? 1.0 / (double)n_max : 0.0;
            coef = a.discount * (a.retrace_h * fmin(1.0, pi / (double)a.mu[bt]));
        }
        s_gain[t] = gain;
        s_aq[t] = (double)q[t * A + act];
        s_coef[t] = coef;
        s_act[t] = act;
    }
    __syncthreads();

    if (threadIdx.x == 0) {  // :161-203, walking back
        const double w = (double)a.weights[b], inv_n = 1.0 / ((double)a.B * (double)S);
        double retrace = 1.0, next_td = 0.0, loss = 0.0, td_sum = 0.0;
        for (int t = S - 1; t >= 0; t--) {
            const double gain = s_gain[t], aq = s_aq[t];
            const double tq = gain + retrace * next_td;
            const double td = gain - aq;
            td_sum = td_sum + td;
            if (a.retrace) {
                next_td = td;
                retrace = retrace * s_coef[t];
            }
            a.target[(i64)b * S + t] = (float)tq;
            const double d = aq * w - tq * w;  // Huber(delta 1) of target * w against q[a] * w (:209)
            const double ad = fabs(d);
            loss = loss + (ad <= 1.0 ? 0.5 * d * d : ad - 0.5);
            s_gain[t] = inv_n * ((ad <= 1.0 ? d : sign_d(d)) * w);
        }
        a.td_mean[b] = (float)(td_sum / (double)S);
        s_aq[0] = loss;
    }
    __syncthreads();

    float *gq = a.grad_q + row;
    const int n = S * A;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int t = i / A;
        gq[i] = (i - t * A == s_act[t]) ? (float)s_gain[t] : 0.f;
    }
    for (int k = threadIdx.x; k < A; k += kThreads) gq[n + k] = k == 0 ? (float)s_aq[0] : 0.f;  // the row's loss term, until k_r2d2_loss takes it
}

// loss = (sum of the B row terms) / (B * S), in double, in a fixed order: thread i adds rows i, i + 256, ...; then a halving tree.
__global__ void __launch_bounds__(kThreads) k_r2d2_loss(int B, int S, int A, float *grad_q, float *loss) {
    __shared__ double red[kThreads];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += kThreads) {
        float *slot = grad_q + ((i64)b * (S + 1) + S) * A;
        acc = acc + (double)*slot;
        *slot = 0.f;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] / ((double)B * (double)S));
}

}  // namespace

int srlx_r2d2_seq_td(int64_t batch, int seq_len, int n_actions, const float *d_q, const float *d_q_target, const int32_t *d_actions, const float *d_mu,
                     const float *d_rewards, const uint8_t *d_dones, const uint8_t *d_invalid, const float *d_weights, double discount, double retrace_h,
                     int enable_retrace, int enable_double_dqn, int enable_rescale, float *d_target, float *d_loss, float *d_grad_q, float *d_td_mean,
                     void *stream) {
    SRLX_REQUIRE(batch >= 1 && batch <= SRLX_SEQ_MAX_B, "r2d2_seq_td: batch %lld outside 1..%d", (long long)batch, SRLX_SEQ_MAX_B);
    SRLX_REQUIRE(seq_len >= 1 && seq_len <= kMaxS, "r2d2_seq_td: seq_len %d outside 1..%d", seq_len, kMaxS);
    SRLX_REQUIRE(n_actions >= 1 && n_actions <= SRLX_SEQ_MAX_A, "r2d2_seq_td: n_actions %d outside 1..%d", n_actions, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(d_q && d_q_target && d_actions && d_mu && d_rewards && d_dones && d_weights && d_target && d_loss && d_grad_q && d_td_mean,
                 "r2d2_seq_td: NULL argument (only invalid may be NULL)");
    SRLX_REQUIRE(discount >= 0.0 && discount <= 1.7976931348623157e308, "r2d2_seq_td: discount must be finite and >= 0");
    SRLX_REQUIRE(retrace_h >= 0.0 && retrace_h <= 1.7976931348623157e308, "r2d2_seq_td: retrace_h must be finite and >= 0");
    R2d2Args a{};
    a.B = (int)batch;
    a.S = seq_len;
    a.A = n_actions;
    a.q = d_q;
    a.q_target = d_q_target;
    a.actions = d_actions;
    a.mu = d_mu;
    a.rewards = d_rewards;
    a.dones = d_dones;
    a.invalid = d_invalid;
    a.weights = d_weights;
    a.discount = discount;
    a.retrace_h = retrace_h;
    a.retrace = enable_retrace != 0;
    a.double_dqn = enable_double_dqn != 0;
    a.rescale = enable_rescale != 0;
    a.target = d_target;
    a.grad_q = d_grad_q;
    a.td_mean = d_td_mean;
    hipLaunchKernelGGL(k_r2d2_seq_td, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_r2d2_loss, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (int)batch, seq_len, n_actions, d_grad_q, d_loss);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}
