// srlx_gemm_plan.h -- the host side of a plan for srlx_mlp_gemm.h's kernels: the job and launch records the kernels read, a bounded builder
// for the list of launches and pointwise steps of one update, the launch grid and the weight gradient's tile table.  Plain C++17 and no HIP header, so a host
// compiler can exercise it alone (tests/host/gemm_plan_host.cpp).
//   Sel, Src, Job   one GEMM of a launch: up to three (rows, weight) sources summed into one output tile, in the order a, b, c (SumSeed's order)
//   Launch, Step    `njobs` jobs of the device table from `first` on, and a step of a plan: such a launch (kFwd, kBwd, or a kind of the algorithm's own kernel
//                   on the same table) or one of the algorithm's pointwise kernels between them
//   Plan            the jobs and steps of one update in fixed arrays whose sizes the algorithm states; a job or step too many sets `overflow` and writes nothing
//                   behind an array
//   grid_of         (column tiles of the launch's widest job, row tiles, jobs)
//   WgradLin, wgrad_table   the running tile count of every Linear of k_mlp_gemm_wgrad's launch
#pragma once
#include <stdint.h>
#include <string.h>

namespace srlxg {

constexpr int kTile = 32;  // rows and columns of a workgroup's output tile
constexpr int kMaxSrc = 3;

enum Sel { kFromJob = 0, kArg0 = 1, kArg1 = 2 };  // where a source's rows come from: the job's own pointer, or one of the launch's two per-call pointers

struct Src {
    const float *a;  // rows [M][lda]
    int lda, sel;
    const float *w;  // forward [N][n] (row stride n); backward [n][N] (row stride N)
    int n;           // reduction length
};

struct Job {
    Src s[kMaxSrc];
    int nsrc, N;        // sources in use; output columns
    const float *aux;   // forward: bias [N]; backward: the kept activations [M][N] whose sign is the ReLU mask
    float *y;           // [M][ldy]
    int ldy, relu;      // (relu: forward only; a kernel of an algorithm's own reads it as that kernel's epilogue or mode)
};
static_assert(sizeof(void *) != 8 || (sizeof(Src) == 32 && sizeof(Job) == 128), "the kernels index the device table by this layout");

// One launch of a plan: `njobs` jobs from `first` on in the device table, the widest of them `nmax` columns.
struct Launch {
    int first, njobs, nmax, bwd;
};

// A step's kind: these two are srlxg::launch's; an algorithm's own kinds (its pointwise kernels, its own kernels on the job table, its tails) start above them.
enum StepKind { kFwd = 0, kBwd = 1 };
struct Step {
    int kind;
    Launch l;  // (a pointwise step: zeros)
};

template <int MaxJobs, int MaxSteps>
struct Plan {
    Job jobs[MaxJobs];
    Step steps[MaxSteps];
    int nj, ns;
    bool overflow;   // a job, a step or a source too many was asked for: the plan is not to be uploaded
    Job spare_job;   // what such a request writes to instead
    Step spare_step;

    void clear() { memset(this, 0, sizeof(*this)); }
    bool full() const { return ns >= MaxSteps; }
    Step &open() { return full() ? spare_step : steps[ns]; }  // the step being built
    // (a launch nothing joins is no step and asks for none, on a full plan too: a step too many is raised by the job that joins it, or by point)
    void begin(int kind) { open() = Step{kind, Launch{nj, 0, 0, kind == kBwd}}; }
    void end() { ns += !full() && steps[ns].l.njobs ? 1 : 0; }
    void point(int kind) {
        overflow = overflow || full();
        open() = Step{kind, Launch{0, 0, 0, 0}};
        ns += full() ? 0 : 1;
    }
    Job &add(int width) {  // (width: the columns the job writes)
        Launch &l = open().l;
        l.njobs++, l.nmax = width > l.nmax ? width : l.nmax;
        if (!full() && nj < MaxJobs) return jobs[nj++];
        overflow = true;
        return spare_job = Job{};
    }
    // Y = act(X W^T + b): rows `x` (or the launch argument `sel` names) of stride `lda`, reduction length K
    void fwd(const float *x, int sel, int lda, const float *w, const float *bias, int K, int N, float *y, int ldy, int relu) {
        Job &j = add(N);
        j.s[0] = Src{x, lda, sel, w, K};
        j.nsrc = 1, j.N = N, j.aux = bias, j.y = y, j.ldy = ldy, j.relu = relu;
    }
    // a backward job of `width` written columns, its sources still to come (src)
    Job &bwd(float *y, int ldy, const float *aux, int N, int width, int epi) {
        Job &j = add(width);
        j.nsrc = 0, j.N = N, j.aux = aux, j.y = y, j.ldy = ldy, j.relu = epi;
        return j;
    }
    void src(Job &j, const float *a, int lda, int n, const float *w) {
        if (j.nsrc < kMaxSrc) j.s[j.nsrc++] = Src{a, lda, kFromJob, w, n};
        else overflow = true;
    }
};

struct Grid {
    int x, y, z;
};
inline Grid grid_of(const Launch &l, int M) { return Grid{(l.nmax + kTile - 1) / kTile, (M + kTile - 1) / kTile, l.njobs}; }

// ---- the weight gradient's table (k_mlp_gemm_wgrad)
struct WgradLin {  // one Linear of the table: segs[2 l] (weight) and segs[2 l + 1] (bias)
    int tile_end;  // running tile count: blockIdx.x is searched here as grad_body searches segs[].end
    int out, in, ktiles;  // ktiles = ceil((in + 1) / 32): tile t of the Linear is (t / ktiles, t % ktiles)
};

// tiles of one Linear (the bias is column `in` of its input rows)
inline int wgrad_tiles(int out, int in) { return ((out + kTile - 1) / kTile) * ((in + 1 + kTile - 1) / kTile); }

// The table of `n` Linears of shape[l] = (out, in) into lins[0..n-1] (NULL: not wanted); returns the launch's tiles.
inline int wgrad_table(const int (*shape)[2], int n, WgradLin *lins) {
    int tiles = 0;
    for (int l = 0; l < n; l++) {
        tiles += wgrad_tiles(shape[l][0], shape[l][1]);
        if (lins) lins[l] = WgradLin{tiles, shape[l][0], shape[l][1], (shape[l][1] + 1 + kTile - 1) / kTile};
    }
    return tiles;
}

}  // namespace srlxg
