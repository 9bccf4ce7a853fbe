// Stand-alone checker of the grouped merged-backward planner in dsrg_amd/csrc/igemm_plan.h (merged_groups_plan and what it is built
// from).  tests/test_igemm_merged_plan.py builds it with the address and undefined-behaviour sanitizers and runs it on the CPU.
// Without arguments it asserts the properties below and exits 0; with --print it also prints the model's prices per geometry.
#include "igemm_plan.h"

#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

using namespace dsrg;

struct Geom { const char *name; int B, H, W, cin, cout, k, ngroups, dil[4]; };
static const Geom kGeoms[] = {
    // the train step's two four-branch layers
    {"fc6 x4, step", 16, 41, 41, 512, 1024, 3, 4, {6, 12, 18, 24}},
    {"fc7 x4, step", 16, 41, 41, 1024, 1024, 1, 4, {1, 1, 1, 1}},
    // the shapes of tests/test_gpu_igemm_merged_groups.py
    {"fc7 form, 9x11", 2, 9, 11, 256, 256, 1, 4, {1, 1, 1, 1}},
    {"fc7 form, 26x29", 2, 26, 29, 256, 256, 1, 4, {1, 1, 1, 1}},
    {"fc6 form, 26x29", 2, 26, 29, 256, 256, 3, 4, {6, 12, 18, 24}},
    {"fc6 form, 13x17", 2, 13, 17, 256, 256, 3, 4, {6, 12, 18, 24}},
    // fewer groups, one pixel, an undilated 3x3 pair, a dilated single layer
    {"one pixel", 1, 1, 1, 256, 256, 1, 1, {1}},
    {"two groups 3x3", 2, 20, 20, 256, 256, 3, 2, {1, 2}},
    {"one group dil 12", 1, 13, 17, 256, 256, 3, 1, {12}},
    {"three groups 1x1", 3, 17, 5, 512, 256, 1, 3, {1, 1, 1}},
};
static const int kCus[] = {256, 304, 8};
static const int kVariants[] = {3, 6, 7, 8, 9};

static int g_failures = 0;
#define CHECK(cond, ...)                                                                                          \
    do {                                                                                                          \
        if (!(cond)) { g_failures++; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// every tile of the data gradient is some block's, no tile is two blocks'
static void check_dgrad_cover(const Geom &g, const DgradShape &d) {
    std::set<std::tuple<int, int, int>> seen;
    for (int id = 0; id < d.grid; id++) {
        int grp = -1, tm = -1, tn = -1;
        if (!dgrad_block_tile(d, id, grp, tm, tn)) continue;
        CHECK(grp >= 0 && grp < d.ngroups && tm >= 0 && tm < d.tiles_m && tn >= 0 && tn < d.tiles_n, "%s: block %d -> (%d, %d, %d)", g.name, id, grp, tm, tn);
        CHECK(seen.insert({grp, tm, tn}).second, "%s: data-gradient tile (%d, %d, %d) twice", g.name, grp, tm, tn);
    }
    CHECK((long long)seen.size() == (long long)d.ngroups * d.tiles_m * d.tiles_n, "%s: %zu data-gradient tiles of %d", g.name, seen.size(),
          d.ngroups * d.tiles_m * d.tiles_n);
    CHECK((int)dgrad_block_costs(d).size() == d.grid, "%s: cost list length", g.name);
}
// ... and every (group, split, output tile) of the weight gradient
static void check_wgrad_cover(const Geom &g, const WgradShape &w) {
    std::set<std::tuple<int, int, int>> seen;
    const int tiles = w.tiles_n * w.tiles_c;
    for (int id = 0; id < w.grid; id++) {
        int grp = -1, split = -1, ksp = -1, t = -1;
        if (!wgrad_block_unit(w, id, grp, split, ksp, t)) continue;
        CHECK(grp >= 0 && grp < w.ngroups && ksp >= 1 && split >= 0 && split < ksp && t >= 0 && t < tiles, "%s: block %d -> (%d, %d / %d, %d)", g.name,
              id, grp, split, ksp, t);
        CHECK(seen.insert({grp, split, t}).second, "%s: weight-gradient unit (%d, %d, %d) twice", g.name, grp, split, t);
    }
    long long want = (long long)w.ngroups * w.ksplit * tiles;
    if (w.plan) {
        want = 0;
        for (int i = 0; i < w.ngroups * 9; i++) want += (long long)w.plan[2 * i] * w.tiles_n * ((w.cin + 255) / 256);
    }
    CHECK((long long)seen.size() == want, "%s: %zu weight-gradient units of %lld", g.name, seen.size(), want);
    const std::vector<double> c = wgrad_block_costs(w);
    CHECK((int)c.size() == w.grid, "%s: cost list length", g.name);
    for (double v : c) CHECK(v >= 0.0, "%s: a negative cost would end an XCD's list", g.name);
}

// the grid [first | padding | second]: the halves' id ranges do not meet, both start at a multiple of 8
static void check_ranges(const char *name, int n_first, int n_second) {
    const int start = merged_second_half_start(n_first);
    CHECK(start % 8 == 0 && start >= n_first && start < n_first + 8, "%s: second half of (%d, %d) starts at %d", name, n_first, n_second, start);
    std::set<int> ids;
    for (int i = 0; i < n_first; i++) CHECK(ids.insert(i).second, "%s: id %d twice", name, i);
    for (int i = 0; i < n_second; i++) CHECK(ids.insert(start + i).second, "%s: id %d twice", name, start + i);
}

static void check_geometry(const Geom &g, int cus, int variant, bool print) {
    const IgemmVariant v = decode_igemm_variant(variant);
    const long long M = (long long)g.B * g.H * g.W;
    const DgradShape d = dgrad_shape_for(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k, g.dil, v);
    const WgradShape w0 = wgrad_shape_for(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k, g.dil, v, 0, cus);
    check_dgrad_cover(g, d);
    check_wgrad_cover(g, w0);
    const MergedGroupsPlan &p = merged_groups_plan(d, g.cin, g.cout, g.k, v, 0, cus);
    CHECK(&p == &merged_groups_plan(d, g.cin, g.cout, g.k, v, 0, cus), "%s: the plan is decided once", g.name);
    CHECK(p.merged_us <= p.separate_us + 1e-9, "%s: %.1f us chosen, %.1f us as two launches", g.name, p.merged_us, p.separate_us);
    CHECK(p.merge || p.merged_us == p.separate_us, "%s: two launches cost what two launches cost", g.name);
    CHECK(p.w_first == 0 || p.w_first == 1, "%s: w_first %d", g.name, p.w_first);
    // a work list stays the weight gradient's half (its bits are the launch's alone); a uniform split fits the workspace, leaves no
    // chunk empty, and is the launch's own where the halves run as two launches
    const int w_grid = p.ksplit > 0 ? wgrad_shape_for(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k, g.dil, v, p.ksplit, cus).grid : w0.grid;
    CHECK((p.ksplit == 0) == (w0.plan != nullptr), "%s: ksplit %d", g.name, p.ksplit);
    if (p.ksplit > 0) {
        CHECK(p.ksplit <= wgrad_ksplit_bound(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k), "%s: split %d beyond the workspace", g.name, p.ksplit);
        CHECK((long long)(p.ksplit - 1) * (((M + p.ksplit - 1) / p.ksplit + 63) / 64 * 64) < M, "%s: split %d leaves an empty chunk", g.name, p.ksplit);
        CHECK(p.merge || p.ksplit == w0.ksplit, "%s: two launches keep the split of the launch alone", g.name);
        CHECK(wgrad_wants_mix(g.dil, g.ngroups, g.k) ? p.ksplit == w0.ksplit : true, "%s: dilated kernels keep their split", g.name);
    }
    check_ranges(g.name, p.w_first ? w_grid : d.grid, p.w_first ? d.grid : w_grid);
    // a forced uniform split is taken where the launch runs one, it leaves no chunk empty and the workspace holds it
    if (!w0.plan) {
        const int bound = wgrad_ksplit_bound(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k);
        for (int ks = 1; ks <= bound + 1; ks++) {
            const bool fits = ks <= bound && (long long)(ks - 1) * (((M + ks - 1) / ks + 63) / 64 * 64) < M;
            const MergedGroupsPlan &f = merged_groups_plan(d, g.cin, g.cout, g.k, v, ks, cus);
            CHECK(f.ksplit == (fits ? ks : w0.ksplit), "%s: forced split %d -> %d", g.name, ks, f.ksplit);
            CHECK(f.merged_us <= f.separate_us + 1e-9, "%s: forced split %d: %.1f us chosen, %.1f us as two launches", g.name, ks, f.merged_us, f.separate_us);
            if (fits) check_wgrad_cover(g, wgrad_shape_for(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k, g.dil, v, ks, cus));
        }
    } else {
        CHECK(merged_groups_plan(d, g.cin, g.cout, g.k, v, 3, cus).ksplit == 0, "%s: a work list is not replaced by a forced split", g.name);
    }
    if (print)
        printf("%-18s cus %3d variant %d: data gradient %4d blocks, weight gradient %4d%s -> %s, w_first %d, ksplit %d: %.1f us merged, %.1f us as two launches\n",
               g.name, cus, variant, d.grid, w0.grid, w0.plan ? " (work list)" : "", p.merge ? "one grid" : "two launches", p.w_first, p.ksplit,
               p.merged_us, p.separate_us);
}

static bool near(double a, double b) { return a - b < 1e-9 && b - a < 1e-9; }
static void check_degenerate() {
    const std::vector<double> none, one = {40.7}, few = {262.2, 262.2, 10.0};
    for (int cus : kCus) {
        const MergedGroupsPlan e0 = merged_groups_decide(none, few, cus), e1 = merged_groups_decide(few, none, cus), e2 = merged_groups_decide(none, none, cus);
        CHECK(!e0.merge && !e1.merge && !e2.merge, "an empty half leaves nothing to merge (cus %d)", cus);
        CHECK(e0.merged_us == e0.separate_us && near(e0.separate_us, 262.2) && e2.separate_us == 0.0, "prices of an empty half (cus %d)", cus);
        // the second block has id 8: the XCD of the first — beside it where an XCD has two CUs, behind it where it has one
        const MergedGroupsPlan s = merged_groups_decide(one, one, cus);
        const double side = cus >= 16 ? 40.7 : 81.4;
        CHECK(s.merge && near(s.merged_us, side) && near(s.separate_us, 81.4), "two single blocks (cus %d): %.1f / %.1f", cus, s.merged_us, s.separate_us);
        // one CU per XCD: ids 0, 8 and 16 queue on XCD 0 in either order
        std::vector<double> nine(9, 5.0);
        CHECK(near(merged_grid_makespan(one, nine, 8), 50.7), "one CU per XCD: %.1f", merged_grid_makespan(one, nine, 8));
        CHECK(near(merged_grid_makespan(nine, one, 8), 50.7), "one CU per XCD, the long block last: %.1f", merged_grid_makespan(nine, one, 8));
        CHECK(near(merged_grid_makespan(one, nine, 256), 40.7), "32 CUs per XCD: %.1f", merged_grid_makespan(one, nine, 256));
        check_ranges("degenerate", 0, 3);
        check_ranges("degenerate", 1, 1);
        check_ranges("degenerate", 8, 0);
    }
}

int main(int argc, char **argv) {
    const bool print = argc > 1 && !strcmp(argv[1], "--print");
    for (const Geom &g : kGeoms)
        for (int cus : kCus)
            for (int variant : kVariants) check_geometry(g, cus, variant, print && variant == 3);
    check_degenerate();
    // the step's layers and the test shapes take the merged grid on the chip they are measured on
    for (int i = 0; i < 6; i++) {
        const Geom &g = kGeoms[i];
        const IgemmVariant v = decode_igemm_variant(3);
        const MergedGroupsPlan &p = merged_groups_plan(dgrad_shape_for(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k, g.dil, v), g.cin, g.cout, g.k, v, 0, 256);
        CHECK(p.merge, "%s: the planner declines (%.1f us against %.1f us)", g.name, p.merged_us, p.separate_us);
    }
    if (g_failures) { printf("%d checks failed\n", g_failures); return 1; }
    printf("all properties hold\n");
    return 0;
}
