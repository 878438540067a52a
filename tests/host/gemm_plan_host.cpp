// The host side of a gemm plan (csrc/srlx_gemm_plan.h) on a CPU: built and run by tests/test_gemm_plan_cpu.py, under AddressSanitizer and
// UndefinedBehaviorSanitizer where the machine links them.  Every CHECK that fails prints its line; the exit status is the number of failures.
#include <stdio.h>

#include "srlx_gemm_plan.h"

using namespace srlxg;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);  \
            failures++;                                              \
        }                                                            \
    } while (0)

enum { kPointA = kBwd + 1, kPointB, kOwnLaunch };

static bool same(const Launch &l, int first, int njobs, int nmax, int bwd) { return l.first == first && l.njobs == njobs && l.nmax == nmax && l.bwd == bwd; }

// field by field: a Src and a Job hold padding, which an assignment need not copy
static bool same(const Job &a, const Job &b) {
    bool eq = a.nsrc == b.nsrc && a.N == b.N && a.aux == b.aux && a.y == b.y && a.ldy == b.ldy && a.relu == b.relu;
    for (int s = 0; s < kMaxSrc; s++) eq = eq && a.s[s].a == b.s[s].a && a.s[s].lda == b.s[s].lda && a.s[s].sel == b.s[s].sel && a.s[s].w == b.s[s].w && a.s[s].n == b.s[s].n;
    return eq;
}

static void launches_and_points() {
    static float x[4], w[4], b[4], y[4];
    Plan<8, 8> p;
    p.clear();
    p.point(kPointA);
    p.begin(kFwd);  // mixed widths: nmax is the widest
    p.add(64);
    p.add(512);
    p.add(1);
    p.end();
    p.begin(kFwd);  // nothing joins: no step
    p.end();
    p.point(kPointB);
    p.begin(kBwd);
    p.add(33);
    p.end();
    p.begin(kOwnLaunch);  // an algorithm's own kind is a forward launch to `bwd`
    p.fwd(x, kArg1, 7, w, b, 9, 96, y, 100, 5);
    p.end();
    CHECK(!p.overflow && p.nj == 5 && p.ns == 5);
    CHECK(p.steps[0].kind == kPointA && same(p.steps[0].l, 0, 0, 0, 0));
    CHECK(p.steps[1].kind == kFwd && same(p.steps[1].l, 0, 3, 512, 0));
    CHECK(p.steps[2].kind == kPointB && same(p.steps[2].l, 0, 0, 0, 0));
    CHECK(p.steps[3].kind == kBwd && same(p.steps[3].l, 3, 1, 33, 1));
    CHECK(p.steps[4].kind == kOwnLaunch && same(p.steps[4].l, 4, 1, 96, 0));
    const Job &j = p.jobs[4];  // lda != K, and `relu` carried as the caller's code
    CHECK(j.nsrc == 1 && j.s[0].a == x && j.s[0].lda == 7 && j.s[0].sel == kArg1 && j.s[0].w == w && j.s[0].n == 9);
    CHECK(j.N == 96 && j.aux == b && j.y == y && j.ldy == 100 && j.relu == 5);
    p.clear();
    CHECK(p.nj == 0 && p.ns == 0 && !p.overflow && p.jobs[4].N == 0 && p.steps[1].l.njobs == 0);
}

static void sources() {
    static float a[4][2], w[4][2], aux[2], y[2];
    Plan<2, 2> p;
    p.clear();
    p.begin(kBwd);
    Job &j = p.bwd(y, 40, aux, 48, 16, 2);
    CHECK(j.nsrc == 0 && j.N == 48 && j.aux == aux && j.y == y && j.ldy == 40 && j.relu == 2);
    for (int s = 0; s < 3; s++) p.src(j, a[s], 10 + s, 20 + s, w[s]);
    p.end();
    CHECK(!p.overflow && j.nsrc == 3 && same(p.steps[0].l, 0, 1, 16, 1));
    for (int s = 0; s < 3; s++) CHECK(j.s[s].a == a[s] && j.s[s].lda == 10 + s && j.s[s].sel == kFromJob && j.s[s].n == 20 + s && j.s[s].w == w[s]);
    const Job before = j;
    p.src(j, a[3], 13, 23, w[3]);  // a fourth source is refused
    CHECK(p.overflow && same(before, j));
}

// A Plan<2, 2> with a guard word behind it: a third job or step sets `overflow` and touches neither the two it holds nor the guard.
struct Guarded {
    Plan<2, 2> p;
    uint64_t guard;
};

static void fill_two(Guarded &g) {
    static float x[1], w[1], b[1], y[1];
    g.p.clear();
    g.guard = 0x5ca1ab1e0ddba11ull;
    for (int i = 0; i < 2; i++) {
        g.p.begin(kFwd);
        g.p.fwd(x, kFromJob, 3 + i, w, b, 3 + i, 5 + i, y, 5 + i, 1);
        g.p.end();
    }
}

static void overflow() {
    Guarded g, full;
    fill_two(full);
    fill_two(g);
    CHECK(!g.p.overflow && g.p.nj == 2 && g.p.ns == 2);
    auto untouched = [&]() {
        return same(g.p.jobs[0], full.p.jobs[0]) && same(g.p.jobs[1], full.p.jobs[1]) && memcmp(g.p.steps, full.p.steps, sizeof(g.p.steps)) == 0 &&
               g.guard == full.guard && g.p.nj == 2 && g.p.ns == 2;
    };
    g.p.begin(kFwd);  // a launch nothing joins asks for no step, on a full plan too
    g.p.end();
    CHECK(!g.p.overflow && untouched());
    g.p.point(kPointA);  // a third step
    CHECK(g.p.overflow && untouched());
    fill_two(g);
    g.p.begin(kBwd);  // a third launch with a third job
    Job &j = g.p.bwd(nullptr, 1, nullptr, 1, 1, 0);
    g.p.src(j, nullptr, 1, 1, nullptr);
    g.p.end();
    CHECK(g.p.overflow && untouched());
    CHECK(&j < g.p.jobs || &j >= g.p.jobs + 2);  // the scratch job, inside the struct
    CHECK((const char *)&j >= (const char *)&g.p && (const char *)(&j + 1) <= (const char *)&g.p + sizeof(g.p));
    fill_two(g);
    g.p.ns = 1;  // room for a step, none for a job
    g.p.begin(kFwd);
    g.p.add(9);
    g.p.end();
    CHECK(g.p.overflow && g.p.nj == 2 && same(g.p.jobs[0], full.p.jobs[0]) && same(g.p.jobs[1], full.p.jobs[1]) && g.guard == full.guard);
}

static void grids() {
    const Grid a = grid_of(Launch{0, 3, 33, 0}, 33);
    CHECK(a.x == 2 && a.y == 2 && a.z == 3);
    const Grid b = grid_of(Launch{5, 1, 1, 1}, 1);
    CHECK(b.x == 1 && b.y == 1 && b.z == 1);
    const Grid c = grid_of(Launch{0, 2, 512, 0}, 4096);
    CHECK(c.x == 16 && c.y == 128 && c.z == 2);
}

static void wgrad() {
    const int shape[3][2] = {{32, 31}, {1, 32}, {33, 1}};
    WgradLin lins[3];
    memset(lins, 0xff, sizeof(lins));
    const int tiles = wgrad_table(shape, 3, lins);
    CHECK(tiles == 5 && wgrad_table(shape, 3, nullptr) == 5);
    const int ends[3] = {1, 3, 5}, ktiles[3] = {1, 2, 1};
    for (int l = 0; l < 3; l++) {
        CHECK(lins[l].tile_end == ends[l] && lins[l].ktiles == ktiles[l] && lins[l].out == shape[l][0] && lins[l].in == shape[l][1]);
        CHECK(wgrad_tiles(shape[l][0], shape[l][1]) == ends[l] - (l ? ends[l - 1] : 0));
    }
    CHECK(wgrad_table(shape, 0, nullptr) == 0);
}

int main() {
    launches_and_points();
    sources();
    overflow();
    grids();
    wgrad();
    printf(failures ? "%d checks failed\n" : "gemm plan: all checks passed\n", failures);
    return failures;
}
