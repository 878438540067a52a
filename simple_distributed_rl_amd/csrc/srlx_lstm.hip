// srlx_lstm.hip -- Agent57's recurrent layer (srl/algorithms/agent57/model_torch.py:39-46,74-75: one-layer, unidirectional, batch_first nn.LSTM) as libsrlx
// kernels: sequence forward and backward through time in float32 on the f32 matrix cores, every sum in a fixed order (no atomics, no split-K across
// workgroups), so a backward pass is bit-reproducible.
//
//   k_lstm_gemm       one dense LDS-tiled GEMM (128 x 128 x 16 block, four waves, 2 x 2 tiles of v_mfma_f32_32x32x2_f32 per wave) for every NON-recurrent
//                     product: Gx = X W_ih^T + b_ih + b_hh for all time steps at once, and after the backward scan dX = dG W_ih, dW_ih = dG^T X,
//                     dW_hh = dG^T Hprev.  Operands are addressed by two strides each; the template arguments say which index is the contiguous one (they
//                     pick the thread mapping of the staging loads, nothing else).  M, N and K tails are staged as zeros.  One wave owns an output
//                     element and walks K in order: the result is one k-ordered fmaf chain.
//   k_lstm_colsum     db_ih = db_hh = column sums of dG: 32 row slices per column, each summed in row order, combined in slice order.
//   k_lstm_fwd_step   one launch per time step: gates = Gx[:, t] + h_{t-1} W_hh^T on v_mfma_f32_16x16x4_f32, a workgroup per (16 units x 16 rows); a lane
//                     holds all four gates of its (row, unit), so the cell is pointwise in the epilogue.  The four waves split K in interleaved chunks of
//                     16 and combine their partial sums through LDS in wave order.
//   k_lstm_bwd_step   one launch per time step, t = T-1 .. 0: dh_t = dY[:, t] + dG_{t+1} W_hh (+ dh_n), the pointwise backward into dG_t and the dc carry;
//                     launched once more (t = -1) for dh0 = dG_0 W_hh when the caller asks for it.
//
// A time step is a launch, not a grid-wide barrier inside a persistent kernel: a launch ends on its own.
#include "srlx_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// dense GEMM
constexpr int GM = 128, GN = 128, GK = 16;
constexpr int GLD = GM + 4;  // LDS row of one k: 128 floats + 4 (a 32-lane ds_read_b32 of consecutive floats is conflict-free at any row stride; the pad
                             // spreads the k-major staging writes over the banks)
static_assert(GM == GN && GM * GK == 8 * 256, "k_lstm_gemm: eight staged elements per thread and operand");

struct GemmArgs {
    const float *A;  // A(m, k) = A[m * sam + k * sak]
    int64_t sam, sak;
    const float *B;  // B(k, n) = B[k * sbk + n * sbn]
    int64_t sbk, sbn;
    const float *B0;  // with T > 0, B is the "previous hidden state" matrix: row k = b * T + t is B0[b * sbk + n] at t = 0 and B[(k - 1) * sbk + n] beyond
    int T;
    float *C;  // C[m * ldc + n]
    int64_t ldc;
    const float *bias1, *bias2;  // both or neither: C += bias1[n] + bias2[n]
    int M, N, K;
};

template <bool AM, bool BN>
__global__ void __launch_bounds__(256) k_lstm_gemm(GemmArgs a) {
    __shared__ float As[GK * GLD], Bs[GK * GLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * GM, n0 = blockIdx.x * GN;
    const int wm = (w & 1) * 64, wn = (w >> 1) * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[x][y][r] = 0.f;
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int e = tid + 256 * j;
            const int am = AM ? e % GM : e / GK, ak = AM ? e / GM : e % GK;
            const int bn = BN ? e % GN : e / GK, bk = BN ? e / GN : e % GK;
            const int gm = m0 + am, gka = k0 + ak, gn = n0 + bn, gkb = k0 + bk;
            ra[j] = (gm < a.M && gka < a.K) ? a.A[(int64_t)gm * a.sam + (int64_t)gka * a.sak] : 0.f;
            float v = 0.f;
            if (gn < a.N && gkb < a.K) {
                if (a.T > 0) {
                    const int t = gkb % a.T;
                    v = t == 0 ? a.B0[(int64_t)(gkb / a.T) * a.sbk + (int64_t)gn * a.sbn] : a.B[(int64_t)(gkb - 1) * a.sbk + (int64_t)gn * a.sbn];
                } else {
                    v = a.B[(int64_t)gkb * a.sbk + (int64_t)gn * a.sbn];
                }
            }
            rb[j] = v;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += GK) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int e = tid + 256 * j;
            const int am = AM ? e % GM : e / GK, ak = AM ? e / GM : e % GK;
            const int bn = BN ? e % GN : e / GK, bk = BN ? e / GN : e % GK;
            As[ak * GLD + am] = ra[j];
            Bs[bk * GLD + bn] = rb[j];
        }
        __syncthreads();
        if (k0 + GK < a.K) fetch(k0 + GK);  // the next tile's loads fly while this one multiplies
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a0 = As[(kk + h) * GLD + wm + i], a1 = As[(kk + h) * GLD + wm + 32 + i];
            const float b0 = Bs[(kk + h) * GLD + wn + i], b1 = Bs[(kk + h) * GLD + wn + 32 + i];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // acc[.][.][r] <-> row (r & 3) + 8 (r >> 2) + 4 h, column i of its 32 x 32 tile
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) {
            const int n = n0 + wn + 32 * y + i;
            if (n >= a.N) continue;
            const float bias = a.bias1 ? a.bias1[n] + a.bias2[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < a.M) a.C[(int64_t)m * a.ldc + n] = a.bias1 ? acc[x][y][r] + bias : acc[x][y][r];
            }
        }
}

template <bool AM, bool BN>
int launch_gemm(const GemmArgs &a, hipStream_t s) {
    dim3 grid((a.N + GN - 1) / GN, (a.M + GM - 1) / GM);
    hipLaunchKernelGGL((k_lstm_gemm<AM, BN>), grid, dim3(256), 0, s, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

// out1[c] = out2[c] = sum over rows of g[row][c]: slice s takes rows s, s + 32, ... in order; the slices are added in order
constexpr int CS_COLS = 32, CS_SLICES = 32;
__global__ void __launch_bounds__(CS_COLS *CS_SLICES) k_lstm_colsum(const float *__restrict__ g, int64_t rows, int cols, float *__restrict__ out1,
                                                                    float *__restrict__ out2) {
    __shared__ float red[CS_SLICES][CS_COLS + 1];
    const int c = blockIdx.x * CS_COLS + (threadIdx.x % CS_COLS), s = threadIdx.x / CS_COLS;
    float sum = 0.f;
    if (c < cols) {
#pragma unroll 4
        for (int64_t r = s; r < rows; r += CS_SLICES) sum += g[r * cols + c];
    }
    red[s][threadIdx.x % CS_COLS] = sum;
    __syncthreads();
    if (s == 0 && c < cols) {
        float t = red[0][threadIdx.x];
        for (int k = 1; k < CS_SLICES; k++) t += red[k][threadIdx.x];
        out1[c] = t;
        out2[c] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// the recurrent steps.  A workgroup owns 16 rows (batch entries) x 16 units.  v_mfma_f32_16x16x4_f32: lane l supplies A[row l & 15][k = l >> 4] and
// B[k = l >> 4][column l & 15]; D[row 4 (l >> 4) + r][column l & 15] is register r.  Which four k a lane group feeds to an MFMA is free as long as A and B
// agree, so a lane loads FOUR consecutive k (one 16-byte load) and spends them on four MFMAs: of a chunk of 16 k, lane group q holds k = 4 q + j at MFMA j.
constexpr int ST = 16;  // rows and units of a step tile

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct FwdArgs {
    const float *gx;   // [B * T][4 H]
    const float *h0, *c0;  // [B][H]
    const float *whh;  // [4 H][H]
    float *y;          // [B * T][H]
    float *wsg, *wsc;  // training: gate activations [B * T][4 H] and cell states [B * T][H]; else NULL
    float *h_n, *c_n;  // [B][H]
    int B, T, H, t;
};

__global__ void __launch_bounds__(256) k_lstm_fwd_step(FwdArgs a) {
    __shared__ float part[4][4][4][64];  // [wave][gate][register][lane]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int u0 = blockIdx.x * ST, r0 = blockIdx.y * ST, H = a.H, T = a.T, t = a.t;
    const int arow = r0 + col;
    const bool aok = arow < a.B;
    const float *hp = !aok ? nullptr : t == 0 ? a.h0 + (int64_t)arow * H : a.y + ((int64_t)arow * T + t - 1) * H;
    const float *wp[4];
#pragma unroll
    for (int g = 0; g < 4; g++) wp[g] = a.whh + (int64_t)(g * H + u0 + col) * H;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = w * 16; kc < H; kc += 64) {
        const int k = kc + 4 * q;
        const f32x4 av = aok ? *(const f32x4 *)(hp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 bv[4];
#pragma unroll
        for (int g = 0; g < 4; g++) bv[g] = *(const f32x4 *)(wp[g] + k);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[g][j], acc[g], 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int r = 0; r < 4; r++) part[w][g][r][lane] = acc[g][r];
    __syncthreads();
    // thread (w, lane) finishes row 4 q + w, unit col of the tile: register w of every wave's partial sums
    const int row = r0 + 4 * q + w, u = u0 + col;
    if (row >= a.B) return;
    const int64_t bt = (int64_t)row * T + t;
    float x[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float s = ((part[0][g][w][lane] + part[1][g][w][lane]) + part[2][g][w][lane]) + part[3][g][w][lane];
        x[g] = a.gx[bt * 4 * H + g * H + u] + s;
    }
    const float gi = sigmoidf_(x[0]), gf = sigmoidf_(x[1]), gg = tanhf(x[2]), go = sigmoidf_(x[3]);
    const float cp = t == 0 ? a.c0[(int64_t)row * H + u] : a.wsc ? a.wsc[(bt - 1) * H + u] : a.c_n[(int64_t)row * H + u];
    const float c = gf * cp + gi * gg;
    const float hh = go * tanhf(c);
    a.y[bt * H + u] = hh;
    if (a.wsc) {
        a.wsg[bt * 4 * H + 0 * H + u] = gi;
        a.wsg[bt * 4 * H + 1 * H + u] = gf;
        a.wsg[bt * 4 * H + 2 * H + u] = gg;
        a.wsg[bt * 4 * H + 3 * H + u] = go;
        a.wsc[bt * H + u] = c;
        if (t == T - 1) a.c_n[(int64_t)row * H + u] = c;
    } else {
        a.c_n[(int64_t)row * H + u] = c;  // the running cell state lives in c_n: this thread alone reads and writes the element
    }
    if (t == T - 1) a.h_n[(int64_t)row * H + u] = hh;
}

struct BwdArgs {
    const float *dy;         // [B * T][H]
    const float *dh_n, *dc_n;  // [B][H] or NULL
    const float *whh;        // [4 H][H]
    const float *wsg, *wsc;  // the forward's gate activations and cell states
    const float *c0;         // [B][H]
    float *dg;               // [B * T][4 H]
    float *dcarry;           // [B][H]: d loss / d c_{t-1}, read at t < T - 1, written at every t
    float *dh0, *dc0;        // [B][H] or NULL
    int B, T, H, t;          // t = -1: dh0 = dG_0 W_hh only
};

__global__ void __launch_bounds__(256) k_lstm_bwd_step(BwdArgs a) {
    __shared__ float part[4][4][64];  // [wave][register][lane]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int u0 = blockIdx.x * ST, r0 = blockIdx.y * ST, H = a.H, T = a.T, t = a.t;
    const int arow = r0 + col;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < T - 1) {  // dG_{t+1} [rows][4 H] times W_hh [4 H][units]
        const bool aok = arow < a.B;
        const float *gp = aok ? a.dg + ((int64_t)arow * T + t + 1) * 4 * H : nullptr;
        const float *wp = a.whh + u0 + col;
        for (int kc = w * 16; kc < 4 * H; kc += 64) {
            const int k = kc + 4 * q;
            const f32x4 av = aok ? *(const f32x4 *)(gp + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            float bv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) bv[j] = wp[(int64_t)(k + j) * H];
#pragma unroll
            for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[w][r][lane] = acc[r];
    __syncthreads();
    const int row = r0 + 4 * q + w, u = u0 + col;
    if (row >= a.B) return;
    const int64_t bu = (int64_t)row * H + u;
    const float rec = ((part[0][w][lane] + part[1][w][lane]) + part[2][w][lane]) + part[3][w][lane];
    if (t < 0) {
        a.dh0[bu] = rec;
        return;
    }
    const int64_t bt = (int64_t)row * T + t;
    float dh = a.dy[bt * H + u] + rec;
    if (t == T - 1 && a.dh_n) dh += a.dh_n[bu];
    const float dc_in = t == T - 1 ? (a.dc_n ? a.dc_n[bu] : 0.f) : a.dcarry[bu];
    const float gi = a.wsg[bt * 4 * H + 0 * H + u], gf = a.wsg[bt * 4 * H + 1 * H + u], gg = a.wsg[bt * 4 * H + 2 * H + u], go = a.wsg[bt * 4 * H + 3 * H + u];
    const float c = a.wsc[bt * H + u], cp = t == 0 ? a.c0[bu] : a.wsc[(bt - 1) * H + u];
    const float tc = tanhf(c);
    const float dc = dh * go * (1.f - tc * tc) + dc_in;
    a.dg[bt * 4 * H + 0 * H + u] = dc * gg * (gi * (1.f - gi));
    a.dg[bt * 4 * H + 1 * H + u] = dc * cp * (gf * (1.f - gf));
    a.dg[bt * 4 * H + 2 * H + u] = dc * gi * (1.f - gg * gg);
    a.dg[bt * 4 * H + 3 * H + u] = dh * tc * (go * (1.f - go));
    const float dcp = dc * gf;
    a.dcarry[bu] = dcp;
    if (t == 0 && a.dc0) a.dc0[bu] = dcp;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
bool in_envelope(int64_t B, int64_t T, int64_t I, int64_t H) {
    return H >= 16 && H <= 512 && H % 16 == 0 && I >= 1 && I <= 16384 && B >= 1 && B <= 256 && T >= 1 && T <= 256;
}
int check_envelope(const char *who, int64_t B, int64_t T, int64_t I, int64_t H) {
    SRLX_REQUIRE(in_envelope(B, T, I, H),
                 "%s: lstm shape B=%lld T=%lld I=%lld H=%lld outside the envelope (B 1..256, T 1..256, I 1..16384, H a multiple of 16 in 16..512)", who,
                 (long long)B, (long long)T, (long long)I, (long long)H);
    return SRLX_OK;
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t srlx_lstm_workspace_floats(int64_t B, int64_t T, int64_t I, int64_t H, int training) {
    if (!in_envelope(B, T, I, H)) return -1;
    return training ? 5 * B * T * H : 0;  // gate activations [B * T][4 H] + cell states [B * T][H]
}

int64_t srlx_lstm_scratch_floats(int64_t B, int64_t T, int64_t I, int64_t H, int training) {
    if (!in_envelope(B, T, I, H)) return -1;
    (void)training;
    return 4 * B * T * H + B * H;  // Gx (forward) or dG (backward) [B * T][4 H], then the dc carry [B][H]
}

int srlx_lstm_forward(int64_t B, int64_t T, int64_t I, int64_t H, const float *x, const float *h0, const float *c0, const float *w_ih, const float *w_hh,
                      const float *b_ih, const float *b_hh, float *y, float *h_n, float *c_n, float *workspace, float *scratch, void *stream) {
    SRLX_TRY(check_envelope("srlx_lstm_forward", B, T, I, H));
    SRLX_REQUIRE(x && h0 && c0 && w_ih && w_hh && b_ih && b_hh && y && h_n && c_n && scratch, "srlx_lstm_forward: lstm: a required pointer is NULL");
    SRLX_REQUIRE(aligned16(h0) && aligned16(w_hh) && aligned16(y), "srlx_lstm_forward: lstm: h0, w_hh and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float *gx = scratch;
    GemmArgs g{};
    g.A = x, g.sam = I, g.sak = 1;
    g.B = w_ih, g.sbk = 1, g.sbn = I;
    g.C = gx, g.ldc = 4 * H;
    g.bias1 = b_ih, g.bias2 = b_hh;
    g.M = (int)(B * T), g.N = (int)(4 * H), g.K = (int)I;
    SRLX_TRY((launch_gemm<false, false>(g, s)));
    FwdArgs f{};
    f.gx = gx, f.h0 = h0, f.c0 = c0, f.whh = w_hh, f.y = y, f.h_n = h_n, f.c_n = c_n;
    f.wsg = workspace, f.wsc = workspace ? workspace + 4 * B * T * H : nullptr;
    f.B = (int)B, f.T = (int)T, f.H = (int)H;
    dim3 grid((unsigned)(H / ST), (unsigned)((B + ST - 1) / ST));
    for (int t = 0; t < (int)T; t++) {
        f.t = t;
        hipLaunchKernelGGL(k_lstm_fwd_step, grid, dim3(256), 0, s, f);
    }
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

int srlx_lstm_backward(int64_t B, int64_t T, int64_t I, int64_t H, const float *x, const float *h0, const float *c0, const float *w_ih, const float *w_hh,
                       const float *y, const float *workspace, const float *dy, const float *dh_n, const float *dc_n, float *dx, float *dw_ih, float *dw_hh,
                       float *db_ih, float *db_hh, float *dh0, float *dc0, float *scratch, void *stream) {
    SRLX_TRY(check_envelope("srlx_lstm_backward", B, T, I, H));
    SRLX_REQUIRE(x && h0 && c0 && w_ih && w_hh && y && workspace && dy && dw_ih && dw_hh && db_ih && db_hh && scratch,
                 "srlx_lstm_backward: lstm: a required pointer is NULL");
    SRLX_REQUIRE(aligned16(w_hh) && aligned16(scratch), "srlx_lstm_backward: lstm: w_hh and scratch must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float *dg = scratch;
    BwdArgs b{};
    b.dy = dy, b.dh_n = dh_n, b.dc_n = dc_n, b.whh = w_hh, b.wsg = workspace, b.wsc = workspace + 4 * B * T * H, b.c0 = c0;
    b.dg = dg, b.dcarry = scratch + 4 * B * T * H, b.dh0 = dh0, b.dc0 = dc0;
    b.B = (int)B, b.T = (int)T, b.H = (int)H;
    dim3 grid((unsigned)(H / ST), (unsigned)((B + ST - 1) / ST));
    for (int t = (int)T - 1; t >= (dh0 ? -1 : 0); t--) {
        b.t = t;
        hipLaunchKernelGGL(k_lstm_bwd_step, grid, dim3(256), 0, s, b);
    }
    SRLX_HIP(hipGetLastError());
    const int BT = (int)(B * T), G = (int)(4 * H);
    GemmArgs g{};
    if (dx) {  // dX [B T][I] = dG [B T][4 H] W_ih [4 H][I]
        g.A = dg, g.sam = G, g.sak = 1;
        g.B = w_ih, g.sbk = I, g.sbn = 1;
        g.C = dx, g.ldc = I;
        g.M = BT, g.N = (int)I, g.K = G;
        SRLX_TRY((launch_gemm<false, true>(g, s)));
    }
    g = GemmArgs{};  // dW_ih [4 H][I] = dG^T X
    g.A = dg, g.sam = 1, g.sak = G;
    g.B = x, g.sbk = I, g.sbn = 1;
    g.C = dw_ih, g.ldc = I;
    g.M = G, g.N = (int)I, g.K = BT;
    SRLX_TRY((launch_gemm<true, true>(g, s)));
    g = GemmArgs{};  // dW_hh [4 H][H] = dG^T Hprev, Hprev row b T + t = h0[b] at t = 0, y[b][t - 1] beyond
    g.A = dg, g.sam = 1, g.sak = G;
    g.B = y, g.sbk = H, g.sbn = 1, g.B0 = h0, g.T = (int)T;
    g.C = dw_hh, g.ldc = H;
    g.M = G, g.N = (int)H, g.K = BT;
    SRLX_TRY((launch_gemm<true, true>(g, s)));
    hipLaunchKernelGGL(k_lstm_colsum, dim3((G + CS_COLS - 1) / CS_COLS), dim3(CS_COLS * CS_SLICES), 0, s, dg, (int64_t)BT, G, db_ih, db_hh);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
