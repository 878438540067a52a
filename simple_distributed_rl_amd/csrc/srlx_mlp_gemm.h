// srlx_mlp_gemm.h -- the layer passes of an MLP update over the WHOLE batch, one tiled GEMM per Linear on gfx950's float64 matrix cores
// (v_mfma_f64_16x16x4_f64).  The row-blocked passes of srlx_mlp_rows.h walk at most 16 rows through every layer in one workgroup; at wide layers and full batches
// that is a GEMM-sized problem walked as chains, and this header is the other way to run it: V-PPO is the first consumer
// (srlx_vppo.hip: srlx_vppo_update_gemm), NoT_SAC the second (srlx_notsac.hip: srlx_notsac_update_gemm, DESIGN.md 7u: k_mlp_gemm_fwd and a backward
// kernel of its own on tile_sums), SAC-Discrete the third (srlx_sacd.hip: srlx_sacd_update_gemm, DESIGN.md 7v: both kernels and a first-layer kernel of its own
// on tile_sums<false>, which hands it the two operands swapped), NoTarget_DQN the fourth (srlx_dqnnot.hip).  What the host needs to drive the kernels
// is one piece of code for all of them: srlx_gemm_plan.h holds Job, Src, Launch, the plan builder and the weight gradient's table, and GemmPath
// at the end of this header the path's device state.
//   Job, Src          (srlx_gemm_plan.h) one GEMM of a launch: up to three (rows, weight) sources summed into one output tile, in the order a, b, c
//   k_mlp_gemm_fwd    Y[M][N] = act(X[M][K] W[N][K]^T + b): the weight in torch's [out][in] layout, both operands contiguous along k
//   k_mlp_gemm_bwd    dH[M][N] = H[M][N] > 0 ? sum_s dOut_s[M][n_s] W_s[n_s][N] : 0: the weight read untransposed, coalesced along the output column
//   k_mlp_gemm_wgrad  dW[N][K] = dOut[M][N]^T X[M][K] and db[N] = sum_m dOut[m][N] of every Linear of a srlxt::Seg table in one launch, the batch the reduction
//                     index: the gradient launch of a handle of srlx_vppo_create_gemm (its own comment stands in front of it below)
// Numeric contract (dense<double>'s, on the matrix cores): tensors are float32 in memory; a lane widens its operand to float64 when it reads its fragment, a product
// of two float32 values is exact there, the sum accumulates in float64 and is rounded to float32 ONCE, in the epilogue.  Inside a group of 4 terms the matrix core's
// order is its own, so a sum may differ from dense<double>'s in the last bit of that one rounding.
//
// The tile.  A workgroup of 4 waves owns a 32 x 32 tile of the output, wave w the 16 x 16 quadrant (w / 2, w % 2): 4 float64 accumulators per lane.  The reduction
// index is walked in chunks of kChunk = 64 across the job's sources; a chunk of the rows operand (32 x 64) and of the weight (32 x 64, or 64 x 32 untransposed) is
// fetched into registers as float32 -- 16-byte loads where the operand's pointer, row stride and length allow, else element by element -- while the matrix cores
// work on the chunk before it, then written to the other half of a double-buffered LDS stage: one barrier per chunk.  16 MFMAs per chunk per wave.
// LDS rows are padded so that the 64 fragment reads of one MFMA operand fall on 64 different banks: stride 68 floats for a [row][k] stage (bank 4 (l % 16) +
// l / 16), stride 48 for the untransposed weight's [k][column] stage (bank 48 (l / 16) + l % 16 mod 64).  34 816 bytes forward, 41 984 bytes backward.
// Rows >= M, columns >= N and reduction indices past a source's length are zero on load and never stored.
//
// Operand layout of v_mfma_f64_16x16x4_f64 (one block, k reduced across the four 16-lane groups), lane l:
//   A: row l % 16, k = l / 16     B: k = l / 16, column l % 16     D: register r holds row 4 r + l / 16, column l % 16
// (D is NOT the float32 16x16x4's 4 (l / 16) + r: the float64 instruction has four groups of ONE row per lane group.)
//
// No atomics, no sum split across workgroups or waves, a fixed chunk order: equal inputs give equal bits.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "srlx_gemm_plan.h"
#include "srlx_param_tail.h"

namespace srlxg {
using i64 = int64_t;

constexpr int kThreads = 256;
constexpr int kChunk = 64;   // reduction indices per LDS stage
constexpr int kLdK = kChunk + 4;  // [row][k] stage: 68 floats (16-byte multiples: rows stay aligned for the float4 stores)
constexpr int kLdN = kTile + 16;  // [k][column] stage: 48 floats

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Kernels of this path are compiled without the packed float32 instructions (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32), whatever the translation unit's flags.
#if defined(__HIP_DEVICE_COMPILE__)
#define SRLXG_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__
#else  // (the host pass knows no such feature)
#define SRLXG_KERNEL __global__
#endif

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// 4 consecutive floats p[0..3] of which the first `left` exist (left <= 0: none); `vec`: one 16-byte load (the caller has checked alignment, and that
// the row's length is a multiple of 4, so a quad is whole or absent)
__device__ __forceinline__ float4 load_quad(const float *p, int left, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (left <= 0) return v;
    if (vec) return *reinterpret_cast<const float4 *>(p);
    v.x = p[0];
    if (left > 1) v.y = p[1];
    if (left > 2) v.z = p[2];
    if (left > 3) v.w = p[3];
    return v;
}

// One chunk of a [rows][k]-contiguous operand: rows r0.. (below `rows`), reduction indices k0.. (below `n`); 512 quads, two per thread.
__device__ __forceinline__ void fetch_rows_k(const float *base, i64 ld, int rows, int n, int r0, int k0, bool vec, float4 (&q)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int slot = threadIdx.x + i * kThreads, r = r0 + (slot >> 4), k = k0 + ((slot & 15) << 2);
        q[i] = load_quad(base + (i64)r * ld + k, r < rows ? n - k : 0, vec);
    }
}
__device__ __forceinline__ void stage_rows_k(float *lds, const float4 (&q)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int slot = threadIdx.x + i * kThreads;
        *reinterpret_cast<float4 *>(lds + (slot >> 4) * kLdK + ((slot & 15) << 2)) = q[i];
    }
}

// One chunk of an untransposed weight [n][N]: reduction rows k0.. (below `n`), columns c0.. (below `N`); 64 x 8 quads, two per thread.
__device__ __forceinline__ void fetch_k_cols(const float *w, int N, int n, int k0, int c0, bool vec, float4 (&q)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int slot = threadIdx.x + i * kThreads, k = k0 + (slot >> 3), c = c0 + ((slot & 7) << 2);
        q[i] = load_quad(w + (i64)k * N + c, k < n ? N - c : 0, vec);
    }
}
__device__ __forceinline__ void stage_k_cols(float *lds, const float4 (&q)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int slot = threadIdx.x + i * kThreads;
        *reinterpret_cast<float4 *>(lds + (slot >> 3) * kLdN + ((slot & 7) << 2)) = q[i];
    }
}

// The tile's accumulators: every chunk of every source of `job` through the matrix cores.  kBwd: the weight is read untransposed.  `x0` / `x1`: the launch's
// per-call row pointers (Sel).  Every thread of the workgroup must call this (it holds barriers); returns this lane's 4 sums (D layout above).
template <bool kBwd>
__device__ __forceinline__ f64x4 tile_sums(const Job &job, int M, int m0, int n0, const float *x0, const float *x1, float *As, float *Bs) {
    constexpr int kAStage = kTile * kLdK, kBStage = kBwd ? kChunk * kLdN : kTile * kLdK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fk = lane >> 4;  // this lane's row / column within the quadrant, and its k within a group of 4
    const int am = (wave >> 1) * 16 + fr, bn = (wave & 1) * 16 + fr;
    const int N = job.N;
    int chunks = 0;
    for (int s = 0; s < job.nsrc; s++) chunks += (job.s[s].n + kChunk - 1) / kChunk;

    // chunk c of the walk: its source and first reduction index (sources in order, each one's chunks in order)
    int s_next = 0, k_next = 0;
    const float *a = nullptr, *w = nullptr;
    int lda = 0, n = 0;
    bool avec = false, wvec = false;
    auto open_source = [&]() {
        const Src &sc = job.s[s_next];
        // (a job's own pointer is NULL where `sel` names an argument.  Bits, not a choice between pointers: the compiler turned `sel ? x0 : sc.a` into a choice
        // between the ADDRESSES of the three and put the two arguments into scratch for it)
        const uintptr_t bits = (uintptr_t)sc.a | (sc.sel == kArg0 ? (uintptr_t)x0 : 0) | (sc.sel == kArg1 ? (uintptr_t)x1 : 0);
        a = (const float *)bits, w = sc.w, lda = sc.lda, n = sc.n;
        avec = aligned16(a) && lda % 4 == 0 && n % 4 == 0;
        wvec = aligned16(w) && (kBwd ? N % 4 == 0 : n % 4 == 0);
    };
    float4 qa[2], qb[2];
    auto fetch = [&]() {  // the next chunk of the walk into registers
        if (k_next == 0) open_source();
        fetch_rows_k(a, lda, M, n, m0, k_next, avec, qa);
        if constexpr (kBwd) fetch_k_cols(w, N, n, k_next, n0, wvec, qb);
        else fetch_rows_k(w, n, N, n, n0, k_next, wvec, qb);
        k_next += kChunk;
        if (k_next >= n) s_next++, k_next = 0;
    };
    auto stage = [&](int half) {
        stage_rows_k(As + half * kAStage, qa);
        if constexpr (kBwd) stage_k_cols(Bs + half * kBStage, qb);
        else stage_rows_k(Bs + half * kBStage, qb);
    };

    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    fetch();
    stage(0);
    __syncthreads();
    for (int c = 0; c < chunks; c++) {
        const bool more = c + 1 < chunks;
        if (more) fetch();  // (in flight under this chunk's MFMAs)
        const float *A = As + (c & 1) * kAStage + am * kLdK + fk;
        const float *B = Bs + (c & 1) * kBStage + (kBwd ? fk * kLdN + bn : bn * kLdK + fk);
#pragma unroll
        for (int kk = 0; kk < kChunk; kk += 4) {
            const double av = (double)A[kk], bv = (double)(kBwd ? B[kk * kLdN] : B[kk]);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        if (more) stage((c + 1) & 1);  // (the half whose readers passed the barrier that ended chunk c - 1)
        __syncthreads();
    }
    return acc;
}

// grid (column tiles of the launch's widest job, row tiles, jobs); a job narrower than the grid leaves its spare workgroups idle
// (static: every translation unit that includes this header -- srlx_vppo.hip, srlx_notsac.hip -- holds the two kernels for its own launches)
static SRLXG_KERNEL void __launch_bounds__(kThreads) k_mlp_gemm_fwd(const Job *__restrict__ jobs, int M, const float *__restrict__ x0, const float *__restrict__ x1) {
    __shared__ __attribute__((aligned(16))) float As[2 * kTile * kLdK], Bs[2 * kTile * kLdK];
    const Job &job = jobs[blockIdx.z];
    const int n0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile;
    if (n0 >= job.N) return;
    const f64x4 acc = tile_sums<false>(job, M, m0, n0, x0, x1, As, Bs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = n0 + (wave & 1) * 16 + (lane & 15);
    if (col >= job.N) return;
    const double b = (double)job.aux[col];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = m0 + (wave >> 1) * 16 + 4 * r + (lane >> 4);
        if (row >= M) continue;
        const float z = (float)(acc[r] + b);
        job.y[(i64)row * job.ldy + col] = job.relu ? (z > 0.f ? z : 0.f) : z;
    }
}

static SRLXG_KERNEL void __launch_bounds__(kThreads) k_mlp_gemm_bwd(const Job *__restrict__ jobs, int M, const float *__restrict__ x0, const float *__restrict__ x1) {
    __shared__ __attribute__((aligned(16))) float As[2 * kTile * kLdK], Bs[2 * kChunk * kLdN];
    const Job &job = jobs[blockIdx.z];
    const int n0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile;
    if (n0 >= job.N) return;
    const f64x4 acc = tile_sums<true>(job, M, m0, n0, x0, x1, As, Bs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = n0 + (wave & 1) * 16 + (lane & 15);
    if (col >= job.N) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = m0 + (wave >> 1) * 16 + 4 * r + (lane >> 4);
        if (row >= M) continue;
        job.y[(i64)row * job.ldy + col] = job.aux[(i64)row * job.N + col] > 0.f ? (float)acc[r] : 0.f;
    }
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------------------
// Every weight / bias pair of a srlxt::Seg table in ONE launch: graw_w[u][k] = sum_b dout[b][u] xin[b][k], graw_b[u] = sum_b dout[b][u], the batch row the
// reduction index.  A workgroup owns a 32 (out) x 32 (in) tile of one Linear; the bias is column `in` of that Linear's X, a 1.0f the loader writes for rows < B, so
// a Linear has ceil((in + 1) / 32) tile columns.  Transposed A: BOTH operands are read as fetch_k_cols reads the backward pass's weight -- for each of the chunk's
// 64 batch rows, 32 consecutive columns -- and staged [k][column] at stride kLdN, so the A fragment of lane l (row l % 16, k = l / 16) and the B fragment
// (k = l / 16, column l % 16) are both As[(kk + l / 16) kLdN + quadrant + l % 16]: bank 48 (l / 16) + l % 16 mod 64, 64 different banks.  49 152 bytes of stage and
// 2 048 of block_sum.  The same numeric contract; every workgroup leaves the float64 sum of the squares of the float32 values it stored in partials[blockIdx.x].
// (WgradLin, the table's rows, and wgrad_table, which fills them: srlx_gemm_plan.h.)

// One chunk of a [k][ld]-strided operand: reduction rows k0.. (below `n`), columns c0.. (below `cols`); 64 x 8 quads, two per thread.  `one` >= 0: column `one`
// of every row below `n` reads 1.0f (the bias column; it lies at or behind `cols`).
__device__ __forceinline__ void fetch_k_cols_ld(const float *p, i64 ld, int cols, int n, int k0, int c0, bool vec, int one, float4 (&q)[2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int slot = threadIdx.x + i * kThreads, k = k0 + (slot >> 3), c = c0 + ((slot & 7) << 2);
        q[i] = load_quad(p + (i64)k * ld + c, k < n ? cols - c : 0, vec);
        const int j = one - c;
        if (k < n && one >= 0) {
            if (j == 0) q[i].x = 1.f;
            if (j == 1) q[i].y = 1.f;
            if (j == 2) q[i].z = 1.f;
            if (j == 3) q[i].w = 1.f;
        }
    }
}

// The tile's accumulators: sum_b dout[b][u0 + .] x[b][k0 + .] over b < B, chunk by chunk.  Every thread of the workgroup must call this (it holds barriers);
// returns this lane's 4 sums: register r is out row u0 + 16 (wave / 2) + 4 r + l / 16, in column k0 + 16 (wave % 2) + l % 16.
__device__ __forceinline__ f64x4 tile_sums_wgrad(const float *dout, int stride, int out, const float *x, int in, int B, int u0, int k0, float *As, float *Bs) {
    constexpr int kStage = kChunk * kLdN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    const int au = (wave >> 1) * 16 + fr, bn = (wave & 1) * 16 + fr;
    const bool avec = aligned16(dout) && stride % 4 == 0 && out % 4 == 0, xvec = aligned16(x) && in % 4 == 0;
    const int chunks = (B + kChunk - 1) / kChunk;
    float4 qa[2], qb[2];
    auto fetch = [&](int c) {
        fetch_k_cols_ld(dout, stride, out, B, c * kChunk, u0, avec, -1, qa);
        fetch_k_cols_ld(x, in, in, B, c * kChunk, k0, xvec, in, qb);
    };
    auto stage = [&](int half) {
        stage_k_cols(As + half * kStage, qa);
        stage_k_cols(Bs + half * kStage, qb);
    };
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < chunks; c++) {
        const bool more = c + 1 < chunks;
        if (more) fetch(c + 1);  // (in flight under this chunk's MFMAs)
        const float *A = As + (c & 1) * kStage + fk * kLdN + au;
        const float *Bp = Bs + (c & 1) * kStage + fk * kLdN + bn;
#pragma unroll
        for (int kk = 0; kk < kChunk; kk += 4) {
            const double av = (double)A[kk * kLdN], bv = (double)Bp[kk * kLdN];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        if (more) stage((c + 1) & 1);  // (the half whose readers passed the barrier that ended chunk c - 1)
        __syncthreads();
    }
    return acc;
}

struct WgradArgs {
    const srlxt::Seg *segs;
    const WgradLin *lins;  // [nlin]
    int nlin, B;
    const float *xin0;     // the caller's states: the input rows of a Linear whose xin is NULL
    double *partials;      // [lins[nlin - 1].tile_end]
};

// grid lins[nlin - 1].tile_end + 1: one workgroup per tile, and a last one that owns no tile and runs the caller's loss sums: tail(sq) with every thread of the
// workgroup, `sq` block_sum's buffer.  (A template: a translation unit holds the kernel for the tails it launches.)
template <typename Tail>
SRLXG_KERNEL void __launch_bounds__(kThreads) k_mlp_gemm_wgrad(WgradArgs a, Tail tail) {
    static_assert(kThreads == srlxt::kThreads, "block_sum reduces the tail's workgroup size");
    __shared__ __attribute__((aligned(16))) float As[2 * kChunk * kLdN], Bs[2 * kChunk * kLdN];
    __shared__ double sq[kThreads];
    const int tile = (int)blockIdx.x;
    if (tile >= a.lins[a.nlin - 1].tile_end) {
        tail(sq);
        return;
    }
    int l = 0;
    while (tile >= a.lins[l].tile_end) l++;
    const WgradLin ln = a.lins[l];
    const srlxt::Seg sw = a.segs[2 * l];
    float *graw_b = a.segs[2 * l + 1].graw;
    const int t = tile - (l ? a.lins[l - 1].tile_end : 0);
    const int u0 = (t / ln.ktiles) * kTile, k0 = (t % ln.ktiles) * kTile;
    const f64x4 acc = tile_sums_wgrad(sw.dout, sw.stride, ln.out, sw.xin ? sw.xin : a.xin0, ln.in, a.B, u0, k0, As, Bs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = k0 + (wave & 1) * 16 + (lane & 15);
    double mine = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int u = u0 + (wave >> 1) * 16 + 4 * r + (lane >> 4);
        if (u >= ln.out || k > ln.in) continue;
        const float g = (float)acc[r];
        if (k < ln.in) sw.graw[(i64)u * ln.in + k] = g;
        else graw_b[u] = g;
        mine += (double)g * (double)g;
    }
    srlxt::block_sum(sq, mine);
    if (threadIdx.x == 0) a.partials[tile] = sq[0];
}

inline void launch(const Launch &l, const Job *d_jobs, int M, const float *x0, const float *x1, hipStream_t st) {
    const Grid g = grid_of(l, M);
    const dim3 grid((unsigned)g.x, (unsigned)g.y, (unsigned)g.z);
    if (l.bwd) hipLaunchKernelGGL(k_mlp_gemm_bwd, grid, dim3(kThreads), 0, st, d_jobs + l.first, M, x0, x1);
    else hipLaunchKernelGGL(k_mlp_gemm_fwd, grid, dim3(kThreads), 0, st, d_jobs + l.first, M, x0, x1);
}

// The path's device state in a handle: the scratch the layer launches write beside the handle's planes, the device copy of the plan's jobs, and
// whether that copy holds the bound tensors (whatever makes the handle's segment table stale sets `ok` false).  `who` names the entry point in every message.
template <int MaxJobs, int MaxSteps>
struct GemmPath {
    float *scratch;  // zeroed when allocated, at the path's first call
    Job *d_jobs;     // [MaxJobs]: the plan's jobs, launch after launch
    Plan<MaxJobs, MaxSteps> plan;
    bool ok;

    int ensure(size_t scratch_floats) {
        if (scratch) return SRLX_OK;
        SRLX_HIP(hipMalloc((void **)&scratch, sizeof(float) * scratch_floats));
        SRLX_HIP(hipMemset(scratch, 0, sizeof(float) * scratch_floats));
        SRLX_HIP(hipMalloc((void **)&d_jobs, sizeof(Job) * MaxJobs));
        return SRLX_OK;
    }
    int upload(const char *who) {
        SRLX_REQUIRE(!plan.overflow, "%s: the gemm plan asked for more than %d jobs, %d steps or %d sources of a job", who, MaxJobs, MaxSteps, kMaxSrc);
        SRLX_HIP(hipMemcpy(d_jobs, plan.jobs, sizeof(Job) * plan.nj, hipMemcpyHostToDevice));
        ok = true;
        return SRLX_OK;
    }
    void release() {
        if (scratch) (void)hipFree(scratch);
        if (d_jobs) (void)hipFree(d_jobs);
        scratch = nullptr, d_jobs = nullptr, ok = false;
    }
};

}  // namespace srlxg
