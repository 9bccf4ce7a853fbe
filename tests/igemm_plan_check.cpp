// Stand-alone checker of dsrg_amd/csrc/igemm_plan.h (tests/test_igemm_plan.py builds it with the address and undefined-behaviour
// sanitizers and runs it on the CPU).  Without arguments it asserts the planners' properties over the geometry list below and
// exits 0; with --dump it prints every decision for that list (tests/golden/igemm_plan_decisions.txt).
#include "igemm_plan.h"

#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

using namespace dsrg;

struct Geom { int B, H, W, cin, cout, k, ngroups, dil[4]; };
static const Geom kGeoms[] = {
    // the train step's layers
    {16, 81, 81, 256, 256, 3, 1, {1}},
    {16, 41, 41, 512, 512, 3, 1, {1}},
    {16, 41, 41, 512, 512, 3, 1, {2}},
    {16, 41, 41, 512, 1024, 3, 4, {6, 12, 18, 24}},
    {16, 41, 41, 512, 1024, 3, 1, {6}},
    {16, 41, 41, 512, 1024, 3, 1, {12}},
    {16, 41, 41, 512, 1024, 3, 1, {18}},
    {16, 41, 41, 512, 1024, 3, 1, {24}},
    {16, 41, 41, 1024, 1024, 1, 1, {1}},
    // the ResNet mode's layers
    {10, 129, 129, 64, 256, 1, 1, {1}},
    {10, 129, 129, 256, 64, 1, 1, {1}},
    {10, 129, 129, 64, 64, 3, 1, {1}},
    {10, 129, 129, 256, 128, 1, 1, {1}},
    {10, 65, 65, 128, 128, 3, 1, {1}},
    {10, 65, 65, 128, 512, 1, 1, {1}},
    {10, 65, 65, 512, 256, 1, 1, {1}},
    {10, 65, 65, 256, 256, 3, 1, {2}},
    {10, 65, 65, 256, 1024, 1, 1, {1}},
    {10, 65, 65, 1024, 256, 1, 1, {1}},
    {10, 65, 65, 1024, 512, 1, 1, {1}},
    {10, 65, 65, 512, 512, 3, 1, {4}},
    {10, 65, 65, 512, 2048, 1, 1, {1}},
    {10, 65, 65, 2048, 512, 1, 1, {1}},
    // edge cases: eight taps that reach nothing, a small odd map, one pixel, W > kBM / 2, H beyond what a class rectangle encodes,
    // the 128-channel 3x3 weight gradient (two taps per tile, no work list)
    {1, 5, 7, 256, 256, 3, 1, {12}},
    {1, 13, 17, 256, 256, 3, 1, {12}},
    {1, 1, 1, 64, 64, 1, 1, {1}},
    {1, 3, 200, 256, 256, 3, 1, {6}},
    {2, 300, 9, 256, 256, 3, 1, {3}},
    {2, 20, 20, 128, 256, 3, 1, {1}},
    {2, 20, 20, 128, 256, 3, 1, {6}},
};
static const int kCus[] = {256, 304, 8};

static int g_failures = 0;
#define CHECK(cond, ...)                                                                                          \
    do {                                                                                                          \
        if (!(cond)) { g_failures++; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static long long chunk_of(long long M, int ks) { return ((M + ks - 1) / ks + 63) / 64 * 64; }
static bool last_split_live(long long M, int ks) { return (long long)(ks - 1) * chunk_of(M, ks) < M; }
static long long tap_pixels(const Geom &g, int q, int tap) {
    const int rh = g.H - abs((tap / 3 - 1) * g.dil[q]), rw = g.W - abs((tap % 3 - 1) * g.dil[q]);
    return rh > 0 && rw > 0 ? (long long)g.B * rh * rw : 0;
}
static bool mergeable(const Geom &g) { return g.ngroups == 1 && (g.k == 1 || g.dil[0] < 3); }
static int dgrad_tiles(const Geom &g) {      // the data gradient of a mergeable layer: flattened tiles, its outputs are the layer's inputs
    const long long M = (long long)g.B * g.H * g.W;
    return (int)((M + kBM - 1) / kBM) * ((g.cin + kBN - 1) / kBN);
}
static bool rows_ok(const Geom &g) { return g.W <= kBM && conv_igemm_row_tiles(g.H, g.W); }

static void check_classes(const Geom &g, int d, int gi) {
    HostClass c[kMaxClasses];
    const int n = build_classes(g.H, g.W, d, c);
    CHECK(n >= 1 && n <= kMaxClasses, "geometry %d: %d classes", gi, n);
    std::vector<int> owner((size_t)g.H * g.W, -1);
    long long pairs = 0;
    for (int i = 0; i < n; i++) {
        if (i) CHECK(__builtin_popcount(c[i].mask) <= __builtin_popcount(c[i - 1].mask), "geometry %d: class %d has more taps than class %d", gi, i, i - 1);
        for (int y = c[i].y0; y < c[i].y1; y++)
            for (int x = c[i].x0; x < c[i].x1; x++) {
                const bool fresh = y >= 0 && y < g.H && x >= 0 && x < g.W && owner[(size_t)y * g.W + x] < 0;
                CHECK(fresh, "geometry %d: pixel (%d, %d) twice or outside", gi, y, x);
                if (!fresh) continue;
                owner[(size_t)y * g.W + x] = i;
                uint32_t live = 0;
                for (int tap = 0; tap < 9; tap++) {
                    const int yy = y + (tap / 3 - 1) * d, xx = x + (tap % 3 - 1) * d;
                    if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) live |= 1u << tap;
                }
                CHECK(live == c[i].mask, "geometry %d: pixel (%d, %d) has taps %x, its class %x", gi, y, x, live, c[i].mask);
                pairs += __builtin_popcount(live);
            }
    }
    for (size_t p = 0; p < owner.size(); p++) CHECK(owner[p] >= 0, "geometry %d: pixel %zu in no class", gi, p);
    const long long ideal = (pairs * g.B + kBM - 1) / kBM, cls = tile_taps(g.B, g.H, g.W, d, 2);
    CHECK(cls >= ideal, "geometry %d dilation %d: %lld class-order steps below the ideal %lld", gi, d, cls, ideal);
}

static void check_geometry(const Geom &g, int gi, int cus) {
    const long long M = (long long)g.B * g.H * g.W;
    const IgemmVariant dflt = decode_igemm_variant(-1);
    if (g.k == 3) {
        for (int q = 0; q < g.ngroups; q++) check_classes(g, g.dil[q], gi);
        if (class_order_pays(g.B, g.H, g.W, g.dil, g.ngroups, rows_ok(g))) {
            long long cls = 0, flat = 0;
            for (int q = 0; q < g.ngroups; q++) { cls += tile_taps(g.B, g.H, g.W, g.dil[q], 2); flat += tile_taps(g.B, g.H, g.W, g.dil[q], 0); }
            CHECK(cls <= flat, "geometry %d: the class order pays with %lld steps against the flat order's %lld", gi, cls, flat);
        }
    }
    // uniform splits
    const int bound = wgrad_ksplit_bound(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k);
    const size_t ws = wgrad_workspace_bytes(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k);
    const size_t room = wgrad_plan_room(g.ngroups, bound, g.cin, g.k);
    const size_t gbytes = (size_t)g.cout * g.k * g.k * g.cin * sizeof(float);
    for (int mix = 0; mix < 2; mix++) {
        const int ks = wgrad_uniform_ksplit(g.ngroups, M, g.cin, g.cout, g.k, mix != 0);
        CHECK(ks >= 1 && last_split_live(M, ks), "geometry %d: uniform split %d leaves its last chunk empty", gi, ks);
        CHECK(wgrad_ksplit_cap(M, ks) >= ks, "geometry %d: cap below the split %d", gi, ks);
        CHECK(ws >= (size_t)g.ngroups * ks * gbytes + room, "geometry %d: workspace below the uniform launch's need", gi);
    }
    if (mergeable(g)) {
        const int ks0 = wgrad_uniform_ksplit(1, M, g.cin, g.cout, g.k, false);
        const std::pair<int, int> m = merged_backward_split(g.B, g.H, g.W, g.cin, g.cout, g.k, dgrad_tiles(g), cus);
        CHECK(m.first >= 1 && m.first <= wgrad_ksplit_cap(M, ks0) && last_split_live(M, m.first), "geometry %d: merged split %d", gi, m.first);
        CHECK(m.second == 0 || m.second == 1, "geometry %d: block order %d", gi, m.second);
        CHECK(ws >= (size_t)m.first * gbytes + room, "geometry %d: workspace below the merged launch's need", gi);
    }
    // the work list
    if (!wgrad_wants_plan(dflt, g.dil, g.ngroups, g.cin, g.k)) return;
    const WgradPlan &p = build_wgrad_plan(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.dil, cus);
    const int ntap = g.ngroups * 9;
    int planes = 0;
    for (int i = 0; i < ntap; i++) {
        const long long Kc = tap_pixels(g, i / 9, i % 9);
        const int cnt = (int)p.words[2 * i];
        CHECK((cnt >= 1) == (Kc > 0), "geometry %d tap %d: %d splits of %lld pixels", gi, i, cnt, Kc);
        if (cnt >= 1) CHECK(last_split_live(Kc, cnt), "geometry %d tap %d: split %d leaves its last chunk empty", gi, i, cnt);
        CHECK((int)p.words[2 * i + 1] == planes, "geometry %d tap %d: first plane %u, expected %d", gi, i, p.words[2 * i + 1], planes);
        planes += cnt;
    }
    for (int i = 2 * ntap; i < kPlanHdr; i++) CHECK(p.words[i] == 0, "geometry %d: table word %d of an absent group is %u", gi, i, p.words[i]);
    CHECK(p.planes == planes && planes <= ntap * bound, "geometry %d: %d planes, counts sum to %d, bound %d", gi, p.planes, planes, ntap * bound);
    CHECK(p.nent == planes && p.words.size() == (size_t)kPlanHdr + p.nent, "geometry %d: %d entries, %zu words", gi, p.nent, p.words.size());
    CHECK(p.words.size() * sizeof(uint32_t) <= room, "geometry %d: %zu words beyond the room of %zu bytes", gi, p.words.size(), room);
    CHECK(ws >= (size_t)planes * g.cout * g.cin * sizeof(float) + room, "geometry %d: workspace below the work list's need", gi);
    std::set<std::tuple<int, int, int>> seen;
    long long prev_steps = -1;
    for (int e = 0; e < p.nent; e++) {
        const uint32_t w = p.words[kPlanHdr + e];
        const int grp = (int)(w & 3u), tap = (int)((w >> 2) & 15u), split = (int)((w >> 6) & 255u), cnt = (int)((w >> 14) & 255u);
        CHECK(grp < g.ngroups && tap < 9 && split < cnt && cnt == (int)p.words[2 * (grp * 9 + tap)], "geometry %d entry %d: %x", gi, e, w);
        CHECK(seen.insert(std::make_tuple(grp, tap, split)).second, "geometry %d entry %d: (%d, %d, %d) twice", gi, e, grp, tap, split);
        const long long Kc = tap_pixels(g, grp, tap), ch = chunk_of(Kc, cnt), beg = split * ch, end = std::min(Kc, beg + ch);
        const long long steps = (end - beg + 63) / 64;
        CHECK(steps >= 1 && (prev_steps < 0 || steps <= prev_steps), "geometry %d entry %d: %lld steps behind %lld", gi, e, steps, prev_steps);
        prev_steps = steps;
    }
}

static void check_variants() {
    for (int v = -1; v <= 12; v++) {
        const int e = (v < 0 || v == 2 || v == 5) ? 3 : v;
        const IgemmVariant d = decode_igemm_variant(v);
        auto in = [e](std::initializer_list<int> s) { return std::find(s.begin(), s.end(), e) != s.end(); };
        CHECK(d.stagger == (e >= 3), "variant %d", v);
        CHECK(d.skip_dead_steps == (e != 6), "variant %d", v);
        CHECK(d.stream_k_where_it_wins == in({3, 8, 9}), "variant %d", v);
        CHECK(d.stream_k_forced == (e == 4), "variant %d", v);
        CHECK(d.class_tiles_allowed == (e != 8), "variant %d", v);
        CHECK(d.class_tiles_forced == (e == 9), "variant %d", v);
        CHECK(d.wgrad_work_list == !in({6, 7}), "variant %d", v);
        CHECK(d.wgrad_compact == (e != 7), "variant %d", v);
        CHECK(d.merged_backward == in({1, 3, 8, 9}), "variant %d", v);
    }
}

static void dump_geometry(const Geom &g) {
    const long long M = (long long)g.B * g.H * g.W;
    printf("geometry B=%d H=%d W=%d cin=%d cout=%d k=%d dil=", g.B, g.H, g.W, g.cin, g.cout, g.k);
    for (int q = 0; q < g.ngroups; q++) printf("%s%d", q ? "," : "", g.dil[q]);
    printf("\n  launchable fwd=%d wgrad=%d col_tiles=%d row_tiles=%d pixel_tiles=%zu\n", (int)conv_igemm_launchable(g.cin, g.cout, g.k),
           (int)conv_igemm_wgrad_launchable(g.cin, g.cout, g.k), wgrad_col_tiles(g.cin, g.k), (int)conv_igemm_row_tiles(g.H, g.W),
           conv_igemm_pixel_tiles(g.B, g.H, g.W));
    if (g.k == 3) {
        for (int q = 0; q < g.ngroups; q++) {
            HostClass c[kMaxClasses];
            const int n = build_classes(g.H, g.W, g.dil[q], c);
            printf("  dil %d classes", g.dil[q]);
            for (int i = 0; i < n; i++) printf(" [%d,%d)x[%d,%d):%03x", c[i].y0, c[i].y1, c[i].x0, c[i].x1, c[i].mask);
            printf("\n  dil %d tile_taps class=%lld rows=", g.dil[q], tile_taps(g.B, g.H, g.W, g.dil[q], 2));
            if (g.W <= kBM) printf("%lld", tile_taps(g.B, g.H, g.W, g.dil[q], 1));
            else printf("-");
            printf(" flat=%lld\n", tile_taps(g.B, g.H, g.W, g.dil[q], 0));
        }
        printf("  class order pays=%d (against %s tiles)\n", (int)class_order_pays(g.B, g.H, g.W, g.dil, g.ngroups, rows_ok(g)), rows_ok(g) ? "row" : "flat");
    }
    const int ks = wgrad_uniform_ksplit(g.ngroups, M, g.cin, g.cout, g.k, wgrad_wants_mix(g.dil, g.ngroups, g.k));
    const int bound = wgrad_ksplit_bound(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k);
    printf("  wgrad ksplit=%d cap=%d bound=%d room=%zu workspace=%zu\n", ks, wgrad_ksplit_cap(M, ks), bound,
           wgrad_plan_room(g.ngroups, bound, g.cin, g.k), wgrad_workspace_bytes(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.k));
    for (int cus : kCus) {
        if (mergeable(g)) {
            const std::pair<int, int> m = merged_backward_split(g.B, g.H, g.W, g.cin, g.cout, g.k, dgrad_tiles(g), cus);
            printf("  cus %d merged nd=%d ksplit=%d w_first=%d\n", cus, dgrad_tiles(g), m.first, m.second);
        }
        if (wgrad_wants_plan(decode_igemm_variant(-1), g.dil, g.ngroups, g.cin, g.k)) {
            const WgradPlan &p = build_wgrad_plan(g.ngroups, g.B, g.H, g.W, g.cin, g.cout, g.dil, cus);
            printf("  cus %d work list nent=%d planes=%d words=%zu\n    counts", cus, p.nent, p.planes, p.words.size());
            for (int i = 0; i < g.ngroups * 9; i++) printf(" %u", p.words[2 * i]);
            printf("\n    words");
            for (uint32_t w : p.words) printf(" %x", w);
            printf("\n");
        }
    }
}

int main(int argc, char **argv) {
    const int ngeom = (int)(sizeof(kGeoms) / sizeof(kGeoms[0]));
    if (argc > 1 && !strcmp(argv[1], "--dump")) {
        for (int gi = 0; gi < ngeom; gi++) dump_geometry(kGeoms[gi]);
        return 0;
    }
    check_variants();
    for (int cus : kCus)
        for (int gi = 0; gi < ngeom; gi++) check_geometry(kGeoms[gi], gi, cus);
    if (g_failures) { printf("%d checks failed\n", g_failures); return 1; }
    printf("igemm_plan: all properties hold for %d geometries\n", ngeom);
    return 0;
}
