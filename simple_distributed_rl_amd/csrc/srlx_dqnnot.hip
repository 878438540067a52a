// srlx_dqnnot.hip -- the whole update of NoTarget_DQN (srl/algorithms/dqn_not/trainer.py:33-87 over parameter.py:17-46) on flat observations in six launches
// (DESIGN.md 7x).  One dueling Q-network: hidden_block Linear(D, U) + ReLU, v_block Linear(U, U) + ReLU + Linear(U, 1), adv_block Linear(U, U) + ReLU +
// Linear(U, A), q = v + adv - mean(adv).  The target comes from the SAME network on the next states, so one forward serves 2B rows: rows 0..B-1 are the states
// and take the gradient, rows B..2B-1 are the next states and take none.
//   k_mlp_gemm_fwd    M = 2B: h = relu(X W0^T + b0)
//   k_mlp_gemm_fwd    M = 2B, two jobs: hv = relu(h Wv1^T + bv1), ha = relu(h Wa1^T + ba1)
//   k_dqnnot_head     one wave per item: the head's 2 (1 + A) dot products, q of both rows, the target, both loss terms, the head's gradient row and the data
//                     gradients dhv, dha of the item's row
//   k_mlp_gemm_bwd    M = B, one job with two sources: dh = h > 0 ? dhv Wv1 + dha Wa1 : 0
//   k_mlp_gemm_wgrad  the five Linears' weight and bias gradients as 32 x 32 tiles; its last workgroup reduces the two loss means
//   k_dqnnot_step     srlxt::step_body with max_norm = +inf (the reference does not clip: coef is exactly 1) and Adam
// The layer launches are srlx_mlp_gemm.h's on v_mfma_f64_16x16x4_f64, their four jobs and the weight gradient's tile table srlx_gemm_plan.h's,
// the segment table and the tail srlx_param_tail.h's; the head kernel is this file's.
//
// k_dqnnot_head.  A workgroup of 4 waves stages the (1 + A) x U head weights (v_block.2's row, then adv_block.2's A rows) ONCE in LDS as float32, at most
// 33 x 512 x 4 = 67 584 bytes of dynamic LDS, and its four waves take one item each.  A lane keeps the strips u = lane + 64 j of hv[b], ha[b], hv[B + b] and
// ha[B + b] in registers, widened to float64 (the last strip masked where U is no multiple of 64); a head row's two dot products -- the item's and its next
// state's, on one read of the weight from LDS, consecutive lanes on consecutive banks -- are per-lane partial sums in u order and one xor butterfly over the 64
// lanes, the same tree for every product.  Lane r keeps row r's pair: lane 0 the value, lanes 1..A the advantages, so the mean and the maximum are one more
// butterfly each and everything after them is lane-uniform float64.  The gradient row is rounded to float32 BEFORE the data gradients read it (the weight
// gradient launch reads the same floats), lane r's element broadcast by a uniform read.  No atomics, a fixed order in every sum: equal inputs give equal bits.
#include "srlx_mlp_gemm.h"
#include "srlx_mlp_walk.h"
#include "srlx_param_tail.h"
#include <cmath>

namespace {

using i64 = int64_t;
using srlxt::kThreads;
using srlxt::Seg;

constexpr int kTensors = 10, kLinears = 5;   // hidden_block.0, v_block.0, v_block.2, adv_block.0, adv_block.2: weight then bias each
constexpr int kJobs = 4;                     // forward: hidden; v_block.0 and adv_block.0 side by side; backward: the hidden layer's data gradient
constexpr int kItems = 4;                    // items of a head workgroup, one per wave
constexpr i64 kMaxBatch = 4096;
constexpr int kMaxUnits = 512, kMaxActions = 32;
constexpr size_t kHeadLdsCap = sizeof(float) * (1 + kMaxActions) * kMaxUnits;  // 67 584 bytes

}  // namespace

struct srlx_dqnnot {
    int D, U, A, device;
    i64 max_batch, elements;
    int wgrad_tiles;
    srlxt::ParamSet ps;
    Seg *d_segs;              // [kTensors]
    srlxg::WgradLin *d_lins;  // [kLinears]
    srlxg::Job *d_jobs;       // [kJobs]
    float *h, *hv, *ha;       // [2 max_batch][U]: rows B.. of an update are the next states'
    float *dh, *dhv, *dha;    // [max_batch][U]
    float *zrow;              // [max_batch][1 + A]: d loss / d (v, adv)
    float *terms;             // [2][max_batch]: the items' weighted Huber and alignment terms
    float *norm;              // [1]: step_body's gradient norm (nobody clips by it)
    double *partials;         // [wgrad_tiles]
};

namespace {

struct HeadArgs {
    int B, U, A;
    const float *hv, *ha;                     // [2B][U]
    const float *wv2, *bv2, *wa2, *ba2;       // [U], [1], [A][U], [A]
    const int32_t *action;
    const float *reward, *not_term, *total_reward, *weights;  // [B]; weights NULL: 1
    double discount, align_coeff;
    float *out_q, *out_target, *terms;        // [B], [B], [2][max_batch]
    i64 max_batch;
    float *zrow, *dhv, *dha;                  // [B][1 + A], [B][U], [B][U]
};

// the same xor tree on every lane: both partners of a step add the same two values, so all 64 lanes end with equal bits
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = fmax(x, __shfl_xor(x, m));
    return x;
}

// kStrips: strips of 64 units a lane holds (U <= 64 kStrips)
template <int kStrips>
__global__ void __launch_bounds__(kThreads) k_dqnnot_head(HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wl[];  // [1 + A][U]: row 0 v_block.2, rows 1.. adv_block.2
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int U = a.U, A = a.A;
    for (int i = t; i < U; i += kThreads) wl[i] = a.wv2[i];
    for (int i = t; i < A * U; i += kThreads) wl[U + i] = a.wa2[i];
    __syncthreads();
    const int b = (int)blockIdx.x * kItems + wave;
    if (b >= a.B) return;  // (behind the workgroup's only barrier)

    double hv[kStrips], ha[kStrips], nhv[kStrips], nha[kStrips];
    {
        const float *pv = a.hv + (i64)b * U, *pa = a.ha + (i64)b * U, *pnv = a.hv + (i64)(a.B + b) * U, *pna = a.ha + (i64)(a.B + b) * U;
#pragma unroll
        for (int j = 0; j < kStrips; j++) {
            const int u = lane + 64 * j;
            const bool ok = u < U;
            hv[j] = ok ? (double)pv[u] : 0.0, ha[j] = ok ? (double)pa[u] : 0.0;
            nhv[j] = ok ? (double)pnv[u] : 0.0, nha[j] = ok ? (double)pna[u] : 0.0;
        }
    }
    // head row r of the item (z) and of its next state (nz), kept by lane r
    const double bias = lane == 0 ? (double)a.bv2[0] : (lane <= A ? (double)a.ba2[lane - 1] : 0.0);
    double z = 0.0, nz = 0.0;
    {
        double p = 0.0, np = 0.0;
#pragma unroll
        for (int j = 0; j < kStrips; j++) {
            const int u = lane + 64 * j;
            const double w = u < U ? (double)wl[u] : 0.0;
            p += w * hv[j], np += w * nhv[j];
        }
        p = wave_sum(p), np = wave_sum(np);
        if (lane == 0) z = p + bias, nz = np + bias;
    }
    for (int r = 1; r <= A; r++) {
        const float *w_r = wl + r * U;
        double p = 0.0, np = 0.0;
#pragma unroll
        for (int j = 0; j < kStrips; j++) {
            const int u = lane + 64 * j;
            const double w = u < U ? (double)w_r[u] : 0.0;
            p += w * ha[j], np += w * nha[j];
        }
        p = wave_sum(p), np = wave_sum(np);
        if (lane == r) z = p + bias, nz = np + bias;
    }

    // the scalar part: lane-uniform from here on but for q / nq, lane r's own
    const bool is_adv = lane >= 1 && lane <= A;
    const double v = __shfl(z, 0), n_v = __shfl(nz, 0);
    const double mean = wave_sum(is_adv ? z : 0.0) / (double)A, n_mean = wave_sum(is_adv ? nz : 0.0) / (double)A;
    const double q = v + z - mean, nq = n_v + nz - n_mean;
    const double n_maxq = wave_max(is_adv ? nq : -INFINITY);
    const int act = a.action[b];
    const double qa = __shfl(q, (act + 1) & 63);
    const double target = (double)a.reward[b] + (double)a.not_term[b] * a.discount * (n_maxq + n_v) / 2.0;
    const double d = target - qa, e = (double)a.total_reward[b] - qa;
    const double w = a.weights ? (double)a.weights[b] : 1.0;
    const double huber = fabs(d) < 1.0 ? 0.5 * d * d : fabs(d) - 0.5;
    const double dq = w / (double)a.B * (-fmin(fmax(d, -1.0), 1.0) - 2.0 * a.align_coeff * e);
    const float dvf = (float)dq;
    const float gf = lane == 0 ? dvf : (float)(dq * ((lane - 1 == act ? 1.0 : 0.0) - 1.0 / (double)A));  // (lanes 0..A: the gradient row)
    if (lane <= A) a.zrow[(i64)b * (1 + A) + lane] = gf;
    if (lane == 0) {
        a.out_q[b] = (float)qa, a.out_target[b] = (float)target;
        a.terms[b] = (float)(w * huber), a.terms[a.max_batch + b] = (float)(w * (e * e));
    }

    // the data gradients of the item's row, from the rounded gradient row
    double acc[kStrips];
#pragma unroll
    for (int j = 0; j < kStrips; j++) acc[j] = 0.0;
    for (int r = 1; r <= A; r++) {
        const double g = (double)__shfl(gf, r);
        const float *w_r = wl + r * U;
#pragma unroll
        for (int j = 0; j < kStrips; j++) {
            const int u = lane + 64 * j;
            if (u < U) acc[j] += g * (double)w_r[u];
        }
    }
    float *pdv = a.dhv + (i64)b * U, *pda = a.dha + (i64)b * U;
#pragma unroll
    for (int j = 0; j < kStrips; j++) {
        const int u = lane + 64 * j;
        if (u >= U) continue;
        pdv[u] = hv[j] > 0.0 ? (float)((double)dvf * (double)wl[u]) : 0.f;
        pda[u] = ha[j] > 0.0 ? (float)acc[j] : 0.f;
    }
}

// ---- acting: the whole forward of 16 rows in one workgroup ------------------------------------------------------------------------------------------
// k_dqnnot_act.  Grid ceil(n / 16); a workgroup of kActWaves waves owns 16 rows -- the M of one v_mfma_f64_16x16x4_f64 tile -- and walks hidden_block.0, then
// v_block.0 and adv_block.0 as ONE pass of 2 U output columns, then the head.  x, h, hv and ha live in dynamic LDS as float32 planes [16][K + 4] (K padded to
// kActStep) and never touch HBM; rows >= n are zero on load and never stored, and no thread leaves before the last barrier.
// Weights go from L2 straight into the B fragment.  A wave owns the column tiles w, w + kActWaves, ... of a pass and runs two of them at a time on one read
// of A.  Per step of kActStep = 32 reduction indices, lane l (column l % 16, lane group g = l / 16) loads the quads k0 + 4 g.. and k0 + 16 + 4 g.. of its
// column's weight row -- the four lane groups of a column cover 128 contiguous bytes -- one step ahead of the matrix cores; element by element where the
// pointer or K do not allow 16-byte loads (load_quad's rule).  MFMA j of a quad therefore reduces k = k0 + 4 g + j in lane group g, and A has to agree: a plane stores reduction index k of a row at act_slot(k), the 4 x 4 transpose inside each group of 16, so the lane's A read of that MFMA is
// plane[row][k0 + 4 j + g] -- row l % 16, consecutive floats across the lane groups -- and with a row stride of 4 * odd floats the 64 reads of one MFMA fall on
// banks 4 (l % 16) stride + l / 16: 64 different ones, srlx_mlp_gemm.h's argument.  The epilogue adds the bias in float64, rounds ONCE, applies ReLU and
// writes the next plane at act_slot(column).  One barrier per layer.
// The head: wave 0 runs v_block.2 (one live column) over hv, waves 1.. the ceil(A / 16) tiles of adv_block.2 over ha, through the same tile loop; sums and
// biases stay float64 in LDS.  Then thread r finishes row r in float64 -- the mean in action order, q = v + adv - mean -- rounds q and v once and takes the
// first maximum of the ROUNDED q.  Fixed order everywhere, no atomics; a row's arithmetic does not know its place or n.
// The plane layout, the tile loop and the pass (act_slot, quad_at, act_tiles, act_layer) are srlx_mlp_walk.h's since DESIGN.md 7za: this kernel's own, lifted
// there unchanged for k_mlp_walk to share.
using srlxw::act_layer;
using srlxw::act_slot;
using srlxw::act_tiles;
constexpr int kActThreads = srlxw::kThreads;  // kActWaves = 16 waves
constexpr int kActRows = srlxw::kRows;        // rows of a workgroup
constexpr i64 kActMaxRows = srlxw::kMaxRows;

constexpr int act_ld(int K) { return srlxw::ld(K); }  // a plane's row stride in floats: 4 * odd
constexpr size_t act_lds_bytes(int D, int U, int A) { return sizeof(float) * kActRows * (act_ld(D) + 3 * act_ld(U)) + sizeof(double) * kActRows * (1 + A); }
constexpr size_t kActLdsCap = act_lds_bytes(256, kMaxUnits, kMaxActions);  // 119 936 bytes

struct ActArgs {
    i64 n;
    int D, U, A;
    const float *x;  // [n][D]
    const float *w0, *b0, *wv1, *bv1, *wv2, *bv2, *wa1, *ba1, *wa2, *ba2;
    float *q, *v;     // [n][A], [n][1]; NULL: not wanted
    int32_t *action;  // [n]
};

SRLXG_KERNEL void __launch_bounds__(kActThreads) k_dqnnot_act(ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float act_lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fr = lane & 15, g = lane >> 4;
    const int D = a.D, U = a.U, A = a.A, Z = 1 + A;
    const int Dp = act_ld(D) - 4, ldx = act_ld(D), ldu = act_ld(U);
    float *xs = act_lds, *hs = xs + kActRows * ldx, *hvs = hs + kActRows * ldu, *has = hvs + kActRows * ldu;
    double *zs = reinterpret_cast<double *>(has + kActRows * ldu);  // [16][1 + A]: v, then adv, bias added (the float planes are a multiple of 256 bytes)
    const i64 row0 = (i64)blockIdx.x * kActRows;

    for (int i = t; i < kActRows * Dp; i += kActThreads) {  // rows >= n and the padding behind D: zero
        const int r = i / Dp, k = i - r * Dp;
        xs[r * ldx + act_slot(k)] = row0 + r < a.n && k < D ? a.x[(row0 + r) * D + k] : 0.f;
    }
    __syncthreads();
    act_layer(xs, ldx, D, U, U / 16, a.w0, a.b0, hs, a.w0, a.b0, hs, ldu);
    __syncthreads();
    act_layer(hs, ldu, U, U, 2 * (U / 16), a.wv1, a.bv1, hvs, a.wa1, a.ba1, has, ldu);
    __syncthreads();
    if (wave < 1 + (A + 15) / 16) {  // (wave-uniform; no barrier inside)
        const bool isv = wave == 0;
        const int col = isv ? fr : (wave - 1) * 16 + fr;
        const float *hw = isv ? a.wv2 : a.wa2;
        const bool live[1] = {col < (isv ? 1 : A)};
        const float *w[1] = {hw + (live[0] ? (i64)col * U : 0)};
        srlxg::f64x4 acc[1] = {{0.0, 0.0, 0.0, 0.0}};
        const float *ha = (isv ? hvs : has) + fr * ldu + g;
        if (srlxg::aligned16(a.wv2) && srlxg::aligned16(a.wa2)) act_tiles<1, true>(ha, U, w, live, acc);  // (U is a multiple of 4)
        else act_tiles<1, false>(ha, U, w, live, acc);
        if (live[0]) {
            const double bias = isv ? (double)a.bv2[0] : (double)a.ba2[col];
#pragma unroll
            for (int r = 0; r < 4; r++) zs[(4 * r + g) * Z + (isv ? 0 : 1 + col)] = acc[0][r] + bias;
        }
    }
    __syncthreads();  // (the workgroup's last barrier)
    if (t < kActRows && row0 + t < a.n) {
        const double *z = zs + t * Z;
        const i64 row = row0 + t;
        double sum = 0.0;
        for (int j = 1; j <= A; j++) sum += z[j];
        const double v = z[0], mean = sum / (double)A;
        float best = 0.f;
        int arg = 0;
        for (int j = 0; j < A; j++) {
            const float q = (float)(v + z[1 + j] - mean);
            if (a.q) a.q[row * A + j] = q;
            if (j == 0 || (best == best && (q > best || q != q))) best = q, arg = j;  // numpy.argmax: the first maximum, a NaN counting as one
        }
        if (a.v) a.v[row] = (float)v;
        a.action[row] = arg;
    }
}

// The two loss means in the last workgroup of k_mlp_gemm_wgrad's launch: every thread takes the items t, t + 256, ... of a term in item order, then block_sum's
// tree -- a fixed order in float64, rounded once.
struct LossMeans {
    i64 B, max_batch;
    const float *terms;  // [2][max_batch]
    float *out;          // [2]: loss_q, loss_align
    __device__ __forceinline__ void operator()(double *sq) const {
        for (int k = 0; k < 2; k++) {
            double mine = 0.0;
            for (i64 b = threadIdx.x; b < B; b += kThreads) mine += (double)terms[k * max_batch + b];
            srlxt::block_sum(sq, mine);
            const double sum = sq[0];
            __syncthreads();  // (every thread has read sq[0] before the next sum's first write)
            if (threadIdx.x == 0) out[k] = (float)(sum / (double)B);
        }
    }
};

__global__ void __launch_bounds__(kThreads) k_dqnnot_step(srlxt::StepArgs a) { srlxt::step_body(a); }

int check_shape(const char *who, int D, int U, int A, i64 max_batch) {
    SRLX_REQUIRE(D >= 1 && D <= 256, "%s: observation length %d (1..256)", who, D);
    SRLX_REQUIRE(U >= 32 && U <= kMaxUnits && U % 32 == 0, "%s: %d units (32..512 in multiples of 32)", who, U);
    SRLX_REQUIRE(A >= 2 && A <= kMaxActions, "%s: %d actions (2..32)", who, A);
    SRLX_REQUIRE(max_batch >= 1 && max_batch <= kMaxBatch, "%s: max_batch %lld (1..%lld)", who, (long long)max_batch, (long long)kMaxBatch);
    return SRLX_OK;
}

// (out, in) of the five Linears in state-dict order
void linear_shapes(const srlx_dqnnot *h, int (*shape)[2]) {
    const int s[kLinears][2] = {{h->U, h->D}, {h->U, h->U}, {1, h->U}, {h->U, h->U}, {h->A, h->U}};
    memcpy(shape, s, sizeof(s));
}

// The segment table, the weight gradient's tile prefix and the four layer jobs, from the bound tensors.
int upload_table(srlx_dqnnot *h) {
    int shape[kLinears][2];
    linear_shapes(h, shape);
    const int U = h->U, Z = 1 + h->A;
    const float *dout[kLinears] = {h->dh, h->dhv, h->zrow, h->dha, h->zrow + 1};
    const float *xin[kLinears] = {nullptr, h->h, h->hv, h->h, h->ha};
    const int stride[kLinears] = {U, U, Z, U, Z};
    Seg segs[kTensors];
    srlxg::WgradLin lins[kLinears];
    memset(segs, 0, sizeof(segs));
    memset(lins, 0, sizeof(lins));
    i64 end = 0;
    for (int l = 0; l < kLinears; l++) srlxt::push_linear(segs + 2 * l, end, shape[l][0], shape[l][1], stride[l], dout[l], xin[l], h->ps, 2 * l);
    srlxg::wgrad_table(shape, kLinears, lins);
    float *const *P = h->ps.p;
    srlxg::Plan<kJobs, 1> plan;  // (for the job table alone: srlx_dqnnot_update writes its four launches out, so the one step is begun and never read)
    plan.clear();
    plan.begin(srlxg::kFwd);
    plan.fwd(nullptr, srlxg::kArg0, h->D, P[0], P[1], h->D, U, h->h, U, 1);
    plan.fwd(h->h, srlxg::kFromJob, U, P[2], P[3], U, U, h->hv, U, 1);
    plan.fwd(h->h, srlxg::kFromJob, U, P[6], P[7], U, U, h->ha, U, 1);
    srlxg::Job &bw = plan.bwd(h->dh, U, h->h, U, U, 0);
    plan.src(bw, h->dhv, U, U, P[2]);  // the value branch first, then the advantage branch: SumSeed's order
    plan.src(bw, h->dha, U, U, P[6]);
    SRLX_REQUIRE(!plan.overflow && plan.nj == kJobs, "dqnnot_update: the layer jobs do not fill their table of %d", kJobs);
    SRLX_HIP(hipMemcpy(h->d_segs, segs, sizeof(segs), hipMemcpyHostToDevice));
    SRLX_HIP(hipMemcpy(h->d_lins, lins, sizeof(lins), hipMemcpyHostToDevice));
    SRLX_HIP(hipMemcpy(h->d_jobs, plan.jobs, sizeof(plan.jobs), hipMemcpyHostToDevice));
    h->ps.table_ok = h->ps.net_ok = true;
    return SRLX_OK;
}

typedef void (*HeadKernel)(HeadArgs);
const HeadKernel kHeadKernels[4] = {k_dqnnot_head<1>, k_dqnnot_head<2>, k_dqnnot_head<4>, k_dqnnot_head<8>};

// the instantiation with the fewest strips that hold U units
int head_kernel_of(int U) {
    int k = 0;
    while ((64 << k) < U) k++;
    return k;
}

}  // namespace

extern "C" {

int srlx_dqnnot_create(srlx_dqnnot_t **out, int obs_dim, int units, int n_actions, int64_t max_batch, int device) {
    SRLX_REQUIRE(out, "dqnnot_create: NULL handle pointer");
    *out = nullptr;
    SRLX_TRY(check_shape("dqnnot_create", obs_dim, units, n_actions, max_batch));
    srlx::DeviceGuard g(device);
    SRLX_REQUIRE(g.ok, "dqnnot_create: device %d unavailable", device);
    srlx_dqnnot *h = new srlx_dqnnot();
    h->D = obs_dim, h->U = units, h->A = n_actions, h->device = device, h->max_batch = max_batch;
    int shape[kLinears][2];
    linear_shapes(h, shape);
    for (int l = 0; l < kLinears; l++) h->elements += (i64)shape[l][0] * shape[l][1] + shape[l][0];
    h->wgrad_tiles = srlxg::wgrad_table(shape, kLinears, nullptr);
    const size_t plane = sizeof(float) * (size_t)max_batch * units;
    hipError_t e = hipMalloc((void **)&h->d_segs, sizeof(Seg) * kTensors);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_lins, sizeof(srlxg::WgradLin) * kLinears);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_jobs, sizeof(srlxg::Job) * kJobs);
    for (float **p : {&h->h, &h->hv, &h->ha})
        if (e == hipSuccess) e = hipMalloc((void **)p, 2 * plane);
    for (float **p : {&h->dh, &h->dhv, &h->dha})
        if (e == hipSuccess) e = hipMalloc((void **)p, plane);
    if (e == hipSuccess) e = hipMalloc((void **)&h->zrow, sizeof(float) * max_batch * (1 + n_actions));
    if (e == hipSuccess) e = hipMalloc((void **)&h->terms, sizeof(float) * 2 * max_batch);
    if (e == hipSuccess) e = hipMalloc((void **)&h->norm, sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&h->partials, sizeof(double) * h->wgrad_tiles);
    // (every instantiation's limit at its cap, at every create: a narrow handle never lowers it under a wide one that is still alive)
    for (HeadKernel k : kHeadKernels)
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadLdsCap);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_dqnnot_act, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kActLdsCap);
    if (e != hipSuccess) {
        srlx_dqnnot_destroy(h);
        srlx::set_error("dqnnot_create: device set-up failed: %s", hipGetErrorString(e));
        return SRLX_ERR_NOMEM;
    }
    *out = h;
    return SRLX_OK;
}

int srlx_dqnnot_destroy(srlx_dqnnot_t *h) {
    if (!h) return SRLX_OK;
    srlx::DeviceGuard g(h->device);
    for (void *p : {(void *)h->d_segs, (void *)h->d_lins, (void *)h->d_jobs, (void *)h->h, (void *)h->hv, (void *)h->ha, (void *)h->dh, (void *)h->dhv, (void *)h->dha,
                    (void *)h->zrow, (void *)h->terms, (void *)h->norm, (void *)h->partials})
        if (p) (void)hipFree(p);
    delete h;
    return SRLX_OK;
}

int srlx_dqnnot_bind_params(srlx_dqnnot_t *h, float *const *d_params) {
    SRLX_REQUIRE(h && d_params, "dqnnot_bind_params: NULL argument");
    return h->ps.bind_params("dqnnot_bind_params", kTensors, d_params);
}

int srlx_dqnnot_bind_grads(srlx_dqnnot_t *h, float *const *d_grads, float *const *d_raw_grads) {
    SRLX_REQUIRE(h && d_grads && d_raw_grads, "dqnnot_bind_grads: NULL argument");
    return h->ps.bind_grads("dqnnot_bind_grads", kTensors, d_grads, d_raw_grads);
}

int srlx_dqnnot_bind_adam(srlx_dqnnot_t *h, float *const *d_exp_avg, float *const *d_exp_avg_sq, int64_t steps_taken, double beta1, double beta2, double eps) {
    SRLX_REQUIRE(h && d_exp_avg && d_exp_avg_sq, "dqnnot_bind_adam: NULL argument");
    return h->ps.bind_adam("dqnnot_bind_adam", kTensors, d_exp_avg, d_exp_avg_sq, steps_taken, beta1, beta2, eps);
}

int64_t srlx_dqnnot_steps(const srlx_dqnnot_t *h) {
    if (!h) {
        srlx::set_error("dqnnot_steps: NULL handle");
        return -1;
    }
    return h->ps.steps;
}

int srlx_dqnnot_update(srlx_dqnnot_t *h, const float *d_states, const int32_t *d_actions, const float *d_rewards, const float *d_not_terminated,
                       const float *d_total_rewards, const float *d_weights, int64_t batch, double discount, double align_coeff, double lr, float *d_q,
                       float *d_target, float *d_losses, void *stream) {
    SRLX_REQUIRE(h, "dqnnot_update: NULL handle");
    SRLX_REQUIRE(h->ps.ready(), "dqnnot_update: bind the parameters, the gradient tensors and the Adam state first");
    SRLX_REQUIRE(batch >= 1 && batch <= h->max_batch, "dqnnot_update: batch %lld (handle sized for %lld)", (long long)batch, (long long)h->max_batch);
    SRLX_REQUIRE(d_states && d_actions && d_rewards && d_not_terminated && d_total_rewards && d_q && d_target && d_losses, "dqnnot_update: NULL argument");
    SRLX_REQUIRE(lr >= 0 && std::isfinite(lr) && std::isfinite(discount) && std::isfinite(align_coeff), "dqnnot_update: lr is non-negative; lr, discount and align_coeff are finite");
    srlx::DeviceGuard g(h->device);
    if (!h->ps.table_ok) SRLX_TRY(upload_table(h));
    hipStream_t st = (hipStream_t)stream;
    const int B = (int)batch, U = h->U, A = h->A;
    srlxg::launch(srlxg::Launch{0, 1, U, 0}, h->d_jobs, 2 * B, d_states, nullptr, st);
    srlxg::launch(srlxg::Launch{1, 2, U, 0}, h->d_jobs, 2 * B, nullptr, nullptr, st);
    float *const *P = h->ps.p;
    const HeadArgs ha{B, U, A, h->hv, h->ha, P[4], P[5], P[8], P[9], d_actions, d_rewards, d_not_terminated, d_total_rewards, d_weights, discount, align_coeff,
                      d_q, d_target, h->terms, h->max_batch, h->zrow, h->dhv, h->dha};
    hipLaunchKernelGGL(kHeadKernels[head_kernel_of(U)], dim3((unsigned)((B + kItems - 1) / kItems)), dim3(kThreads), sizeof(float) * (size_t)(1 + A) * U, st, ha);
    srlxg::launch(srlxg::Launch{3, 1, U, 1}, h->d_jobs, B, nullptr, nullptr, st);
    const srlxg::WgradArgs wa{h->d_segs, h->d_lins, kLinears, B, d_states, h->partials};
    hipLaunchKernelGGL(srlxg::k_mlp_gemm_wgrad<LossMeans>, dim3((unsigned)h->wgrad_tiles + 1), dim3(kThreads), 0, st, wa, LossMeans{(i64)B, h->max_batch, h->terms, d_losses});
    const srlxt::StepArgs sa = h->ps.step_args(h->d_segs, kTensors, h->partials, h->wgrad_tiles, (double)INFINITY, lr, h->norm);
    hipLaunchKernelGGL(k_dqnnot_step, dim3((unsigned)((h->elements + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sa);
    SRLX_HIP(hipGetLastError());
    h->ps.steps++;
    return SRLX_OK;
}

int srlx_dqnnot_act(srlx_dqnnot_t *h, int64_t n_rows, const float *d_states, float *d_q, float *d_v, int32_t *d_actions, void *stream) {
    SRLX_REQUIRE(n_rows >= 1 && n_rows <= kActMaxRows, "dqnnot_act: n_rows %lld (1..%lld)", (long long)n_rows, (long long)kActMaxRows);
    SRLX_REQUIRE(h, "dqnnot_act: NULL handle");
    SRLX_REQUIRE(h->ps.bound, "dqnnot_act: bind the parameters first (srlx_dqnnot_bind_params)");
    SRLX_REQUIRE(d_states && d_actions, "dqnnot_act: NULL d_states or d_actions (d_q and d_v alone are optional)");
    srlx::DeviceGuard g(h->device);
    float *const *P = h->ps.p;
    const ActArgs aa{n_rows, h->D, h->U, h->A, d_states, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], P[9], d_q, d_v, d_actions};
    hipLaunchKernelGGL(k_dqnnot_act, dim3((unsigned)((n_rows + kActRows - 1) / kActRows)), dim3(kActThreads), act_lds_bytes(h->D, h->U, h->A), (hipStream_t)stream, aa);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
