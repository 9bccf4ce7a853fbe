// Host-side planning of the implicit-GEMM launches (conv_igemm.hip): which shapes a launch takes, how its pixels are tiled and
// ordered, how a weight gradient's pixels are split, the work list of a dilated launch, the split and block order of a merged
// backward grid (one layer, or 1 - 4 groups priced block by block), and what a debug variant number means.  Pure integer and double arithmetic on shapes: C++17 and the standard
// library only, no HIP — the CU count is an argument — so that every decision can be checked on a CPU
// (tests/igemm_plan_check.cpp, tests/golden/igemm_plan_decisions.txt; tests/igemm_merged_plan_check.cpp).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <queue>
#include <vector>

namespace dsrg {

// shared with the kernels
constexpr int kBM = 256, kBN = 256;                        // a tile: pixels x output channels
constexpr int kMaxClasses = 9;                             // rectangles of a map's class order (IgemmGroup::cls)
constexpr int kPlanHdr = 2 * 4 * 9;                        // words in front of a work list's entries

// ---- dsrg_debug_set_igemm_variant's integer, decoded once per public launch (INTEGRATION.md has the table).  Every integer
// decodes: negative values and the retired 2 / 5 (a ring of four 32-deep stages, an early barrier) are the default, 3
struct IgemmVariant {
    bool stagger;                   // IgemmArgs::stagger, IgemmWgradArgs::stagger
    bool skip_dead_steps;           // skip_taps / skip_rows, and with them xcd_mix and compact (off: 6 — every tap of every tile)
    bool stream_k_where_it_wins;    // the 60 % rule of prepare_igemm (3, and 8 / 9: 3 with one tiling forced)
    bool stream_k_forced;           // 4: wherever legal
    bool class_tiles_allowed;       // off: 8 — row-aligned tiles
    bool class_tiles_forced;        // 9: the class order wherever it is legal
    bool wgrad_work_list;           // off: 6 / 7 — one uniform split
    bool wgrad_compact;             // off: 7 — dead steps skipped in the flat pixel order
    bool merged_backward;           // 1, 3, 8, 9
};
inline IgemmVariant decode_igemm_variant(int v) {
    const int e = (v < 0 || v == 2 || v == 5) ? 3 : v;
    return IgemmVariant{e >= 3, e != 6, e == 3 || e == 8 || e == 9, e == 4, e != 8, e == 9, e != 6 && e != 7, e != 7, e == 3 || e == 1 || e == 8 || e == 9};
}

// a decision taken once per key.  Values live in the map's nodes, whose addresses never change: a reference handed out stays
// valid for the life of the process
template <class Key, class Value> struct PlanMemo {
    std::mutex mutex_;
    std::map<Key, Value> map_;
    template <class Make> const Value &get(const Key &key, Make &&make) {
        std::lock_guard<std::mutex> lock(mutex_);
        auto it = map_.find(key);
        if (it == map_.end()) it = map_.emplace(key, make()).first;
        return it->second;
    }
};

// when the last block of a grid ends: the chip is 8 XCDs, XCD x takes the blocks cost(x, 0), cost(x, 1), .. (a negative cost ends
// its list) and its CUs take them in that order as they free up
template <class Cost> double dispatch_makespan(int cus, Cost &&cost) {
    const int per_xcd = cus / 8 > 0 ? cus / 8 : 32;
    double worst = 0.0;
    for (int x = 0; x < 8; x++) {
        std::priority_queue<double, std::vector<double>, std::greater<double>> cu;
        for (int c = 0; c < per_xcd; c++) cu.push(0.0);
        double t;
        for (int b = 0; (t = cost(x, b)) >= 0.0; b++) {
            const double end = cu.top() + t;
            cu.pop();
            cu.push(end);
            worst = std::max(worst, end);
        }
    }
    return worst;
}

// ---- what the launches take.  Forward / data gradient: also a 64-channel output (a wave's 128 output columns half empty: rows
// of w past cout read zeros through the descriptor, the store skips them) — not the recommended route for a 3x3 layer
// (conv_direct.hip), but a 1x1 layer over many pixels is bandwidth-bound either way (ResNet res2: 256 -> 64 at 129 x 129 x 10 pixels)
inline bool conv_igemm_launchable(int cin, int cout, int k) {
    return (k == 1 || k == 3) && cin >= 64 && cin % 64 == 0 && (cout == 64 || (cout >= 128 && cout % 128 == 0));
}
// weight gradient (conv_igemm_wgrad_supported: where it is the recommended route): any multiples of 64 channels — a tile is 256
// outputs x (one tap x 256 inputs), narrower tensors leave part of it empty (ResNet res2 / res3: 64 / 128 channels over 42 - 166
// thousand pixels, bandwidth-bound either way)
inline bool conv_igemm_wgrad_launchable(int cin, int cout, int k) {
    return (k == 1 || k == 3) && cin >= 64 && cin % 64 == 0 && cout >= 64 && cout % 64 == 0;
}
inline int wgrad_col_tiles(int cin, int k) { return (cin == 128 && k == 3) ? (k * k + 1) / 2 : k * k * ((cin + 255) / 256); }

// row-aligned pixel tiles (IgemmArgs::row_tiles) when at least two rows fit a tile and the rows a band leaves empty cost less
// than a tenth of the tiles
inline bool conv_igemm_row_tiles(int H, int W) {
    if (W > kBM / 2) return false;
    const int r = kBM / W, bands = (H + r - 1) / r;
    return (long long)bands * kBM * 10 <= (long long)H * W * 11 + 10LL * kBM;
}
// most pixel tiles a launch over B maps of H x W can have per group (flattened or row-aligned): sizes the column-sum scratch
inline size_t conv_igemm_pixel_tiles(int B, int H, int W) {
    const long long M = (long long)B * H * W;
    size_t t = (size_t)((M + kBM - 1) / kBM);
    if (W <= kBM && conv_igemm_row_tiles(H, W)) {
        const int r = kBM / W;
        const size_t tr = (size_t)B * ((H + r - 1) / r);
        if (tr > t) t = tr;
    }
    return t;
}

// ---- class order of a dilated launch's pixels (IgemmArgs::cls_tiles)
inline uint32_t tap_mask_rect(int H, int W, int d, int y0, int y1, int x0, int x1) {      // the taps that reach a pixel of [y0, y1) x [x0, x1)
    uint32_t m = 0;
    for (int tap = 0; tap < 9; tap++) {
        const int dy = (tap / 3 - 1) * d, dx = (tap % 3 - 1) * d;
        if (std::max(y0, -dy) < std::min(y1, H - dy) && std::max(x0, -dx) < std::min(x1, W - dx)) m |= 1u << tap;
    }
    return m;
}
// the bands of an axis of n pixels inside each of which the taps -d / +d are either valid for every pixel or for none
inline int axis_bands(int n, int d, int (*out)[2]) {
    if (d >= n) { out[0][0] = 0; out[0][1] = n; return 1; }
    const int lo = std::min(d, n - d), hi = std::max(d, n - d), cut[4] = {0, lo, hi, n};
    int k = 0;
    for (int i = 0; i < 3; i++)
        if (cut[i + 1] > cut[i]) { out[k][0] = cut[i]; out[k][1] = cut[i + 1]; k++; }
    return k;
}
struct HostClass { int y0, y1, x0, x1; uint32_t mask; };
inline int build_classes(int H, int W, int d, HostClass *c) {      // most live taps first (ties: map order)
    int yb[3][2], xb[3][2];
    const int ny = axis_bands(H, d, yb), nx = axis_bands(W, d, xb);
    int n = 0;
    for (int i = 0; i < ny; i++)
        for (int j = 0; j < nx; j++) c[n++] = HostClass{yb[i][0], yb[i][1], xb[j][0], xb[j][1], tap_mask_rect(H, W, d, yb[i][0], yb[i][1], xb[j][0], xb[j][1])};
    std::stable_sort(c, c + n, [](const HostClass &a, const HostClass &b) { return __builtin_popcount(a.mask) > __builtin_popcount(b.mask); });
    return n;
}
// K-steps per 64-channel chunk (= live taps summed over the pixel tiles) of one group: class order / row-aligned / flattened tiles
inline long long tile_taps(int B, int H, int W, int d, int mode) {
    const long long M = (long long)B * H * W;
    long long tot = 0;
    if (mode == 1) {                                         // whole rows of one image
        const int r = kBM / W;
        for (int y0 = 0; y0 < H; y0 += r) tot += (long long)B * __builtin_popcount(tap_mask_rect(H, W, d, y0, std::min(H, y0 + r), 0, W));
        return tot;
    }
    HostClass c[kMaxClasses];
    const int n = mode == 2 ? build_classes(H, W, d, c) : 0;
    long long q0[kMaxClasses + 1] = {0};
    for (int k = 0; k < n; k++) q0[k + 1] = q0[k] + (long long)B * (c[k].y1 - c[k].y0) * (c[k].x1 - c[k].x0);
    for (long long t0 = 0; t0 < M; t0 += kBM) {              // 256 consecutive indices of the class order (2) or pixels (0)
        const long long t1 = std::min(M, t0 + kBM);
        uint32_t m = 0;
        for (int k = 0; k < n; k++)
            if (q0[k] < t1 && q0[k + 1] > t0) m |= c[k].mask;
        for (long long p = t0; mode == 0 && p < t1;) {       // row by row (a row piece is a rectangle)
            const int rem = (int)(p % ((long long)H * W)), y = rem / W, x = rem % W;
            const int x1 = (int)std::min<long long>(W, x + (t1 - p));
            m |= tap_mask_rect(H, W, d, y, y + 1, x, x1);
            p += x1 - x;
        }
        tot += __builtin_popcount(m);
    }
    return tot;
}
// the class order pays where its tiles run fewer K-steps than the tiling it replaces (row-aligned tiles when `rows`, else
// flattened ones; a map of few tiles has most of them straddle classes); decided once per geometry
inline bool class_order_pays(int B, int H, int W, const int *dil, int ngroups, bool rows) {
    static PlanMemo<std::array<int, 9>, bool> memo;
    std::array<int, 9> key = {B, H, W, 0, 0, 0, 0, ngroups, rows};
    for (int g = 0; g < ngroups; g++) key[3 + g] = dil[g];
    return memo.get(key, [&] {
        long long now = 0, then = 0;
        for (int g = 0; g < ngroups; g++) { now += tile_taps(B, H, W, dil[g], 2); then += tile_taps(B, H, W, dil[g], rows ? 1 : 0); }
        return now * 100 < then * 97;
    });
}

// ---- pixel splits of the weight gradient.
// The UNIFORM split of a launch (every launch but the dilated 3x3 ones in the compact pixel order, whose splits are per (group,
// tap): build_wgrad_plan; the debug variants 6 / 7 of those; the bound the workspace is sized by): the number of workgroups per
// output tile that minimises
// rounds of the chip x (K-steps per workgroup + a fixed cost per workgroup for prologue and the partial tile's write-out)
// out_bytes: the gradient tensors of all groups — every split writes and the reduction reads that much again, ~2.3 us (one
// K-step of a workgroup) per 9.2 MB at the rate the reduction kernel streams (the four fc6_k: 75 MB, 8 K-steps per split)
// xcd_mix_only: only the splits the XCD-interleaved workgroup map takes (a divisor or a multiple of 8)
inline int wgrad_ksplit(long long M, int tiles, int cus, double out_bytes = 0.0, bool xcd_mix_only = false) {
    long long best_cost = -1;
    int best = 1;
    for (int ks = 1; ks <= 128; ks++) {
        const long long chunk = ((M + ks - 1) / ks + 63) / 64 * 64;
        if ((long long)(ks - 1) * chunk >= M) continue;                 // an empty last split
        if (xcd_mix_only && ks % 8 != 0 && 8 % ks != 0) continue;
        const long long steps = chunk / 64, rounds = ((long long)tiles * ks + cus - 1) / cus;
        const long long cost = rounds * (steps + 8) + (long long)(ks * out_bytes / 9.2e6);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ks; }
    }
    return best;
}
// dilated kernels: workgroups of unequal length, which want the XCD-interleaved map (whatever the variant: tests compare them bit for bit)
inline bool wgrad_wants_mix(const int *dil, int ngroups, int k) {
    for (int q = 0; q < ngroups; q++)
        if (k == 3 && dil && dil[q] >= 3) return true;
    return false;
}
// ... of a launch of ngroups layers over M pixels (priced for a chip of 256 CUs, whatever the device: the workspace's size follows)
inline int wgrad_uniform_ksplit(int ngroups, long long M, int cin, int cout, int k, bool xcd_mix_only) {
    return wgrad_ksplit(M, ngroups * ((cout + 255) / 256) * wgrad_col_tiles(cin, k), 256, (double)ngroups * cout * k * k * cin * 4.0, xcd_mix_only);
}

// the finest pixel split the merged backward may pick for a layer whose stand-alone split is ks: twice as fine, never beyond
// one 64-pixel step per split
inline int wgrad_ksplit_cap(long long M, int ks) {
    const long long most = (M + 63) / 64;
    long long c = 2LL * ks;
    if (c > most) c = most;
    if (c > 128) c = 128;
    return (int)(c < ks ? ks : c);
}

// the most partial copies of the gradient any launch of this geometry writes, whatever its dilations
inline int wgrad_ksplit_bound(int ngroups, int B, int H, int W, int cin, int cout, int k) {
    const long long M = (long long)B * H * W;
    // (a launch of dilated kernels picks among the splits the XCD-interleaved map takes)
    int ks = std::max(wgrad_uniform_ksplit(ngroups, M, cin, cout, k, false), wgrad_uniform_ksplit(ngroups, M, cin, cout, k, true));
    if (ngroups == 1) ks = wgrad_ksplit_cap(M, ks);         // (the merged backward launch may cut a single layer's pixels finer)
    return ks;
}
// room for the work list of a dilated launch behind the partials: its table and one word per partial plane (a plan never holds
// more planes than the uniform bound: build_wgrad_plan)
inline size_t wgrad_plan_room(int ngroups, int ks_bound, int cin, int k) {
    if (k != 3 || cin == 128) return 0;
    return ((size_t)(kPlanHdr + ngroups * 9 * ks_bound) * sizeof(uint32_t) + 255) / 256 * 256;
}
// the weight gradient's workspace: the partials of the uniform bound, the work list's room behind them (0: not a geometry the launch takes)
inline size_t wgrad_workspace_bytes(int ngroups, int B, int H, int W, int cin, int cout, int k) {
    if (!conv_igemm_wgrad_launchable(cin, cout, k) || ngroups < 1 || ngroups > 4) return 0;
    const int ks = wgrad_ksplit_bound(ngroups, B, H, W, cin, cout, k);
    return (size_t)ngroups * ks * cout * k * k * cin * sizeof(float) + wgrad_plan_room(ngroups, ks, cin, k);
}

// ---- the work list of a dilated launch (IgemmWgradArgs::plan).  Split counts per (group, tap) from the tap's live pixels
// B (H - |dy|) (W - |dx|): for every target length L (K-steps per workgroup) the counts round(steps / L) — at least one, none for an
// empty rectangle, never so many that a split is empty — give a list of entries that is sorted longest first, dealt to the
// XCDs in turn and run through dispatch_makespan (a workgroup costs its K-steps + 8); every partial plane is priced as
// wgrad_ksplit prices it (one K-step per 9.2 MB written and read back).  The cheapest L wins; the planes never outnumber the
// uniform bound the workspace was sized for.
struct WgradPlan {
    std::vector<uint32_t> words;      // table + entries, as the kernels read them
    int nent = 0, planes = 0;
};
// does a launch of these kernels take a work list?  3x3 kernels of which one has dilation >= 3, in the compact pixel order (not
// the variants 6 / 7, not a 128-channel x).  (The weight-gradient half of a merged backward launch never does: its caller does not ask.)
inline bool wgrad_wants_plan(const IgemmVariant &v, const int *dil, int ngroups, int cin, int k) {
    if (k != 3 || cin == 128 || !dil || !v.wgrad_work_list) return false;
    for (int q = 0; q < ngroups; q++)
        if (dil[q] < 1) return false;
    return wgrad_wants_mix(dil, ngroups, k);
}
inline const WgradPlan &build_wgrad_plan(int ngroups, int B, int H, int W, int cin, int cout, const int *dil, int cus) {
    static PlanMemo<std::array<int, 11>, WgradPlan> memo;      // (launches hold pointers to the words)
    std::array<int, 11> key = {B, H, W, cin, cout, ngroups, 0, 0, 0, 0, cus};
    for (int q = 0; q < ngroups; q++) key[6 + q] = dil[q];
    return memo.get(key, [&] {
        const int ntap = ngroups * 9, tpe = ((cout + 255) / 256) * ((cin + 255) / 256);
        const int cap = ntap * wgrad_ksplit_bound(ngroups, B, H, W, cin, cout, 3);
        const double plane_price = (double)cout * cin * 4.0 / 9.2e6;
        std::vector<long long> Kc(ntap);
        long long max_steps = 1;
        for (int q = 0; q < ngroups; q++)
            for (int tap = 0; tap < 9; tap++) {
                const int rh = H - abs((tap / 3 - 1) * dil[q]), rw = W - abs((tap % 3 - 1) * dil[q]);
                Kc[q * 9 + tap] = (rh > 0 && rw > 0) ? (long long)B * rh * rw : 0;
                max_steps = std::max(max_steps, (Kc[q * 9 + tap] + 63) / 64);
            }
        struct Entry { int steps, grp, tap, split, count; };
        auto chunk_of = [&](int i, long long c) { return ((Kc[i] + c - 1) / c + 63) / 64 * 64; };
        auto count_for = [&](int i, long long L) -> int {                                       // tap i (not empty) at target length L
            const long long steps = (Kc[i] + 63) / 64;
            long long c = std::min<long long>(std::max<long long>((steps + L / 2) / L, 1), 128);
            while (c > 1 && (c - 1) * chunk_of(i, c) >= Kc[i]) c--;                             // (an empty last split)
            return (int)c;
        };
        auto entries_for = [&](std::vector<Entry> &out, const int *cnt) {
            out.clear();
            for (int i = 0; i < ntap; i++)
                for (int s = 0; s < cnt[i]; s++) {
                    const long long ch = chunk_of(i, cnt[i]), beg = s * ch, end = std::min(Kc[i], beg + ch);
                    out.push_back({(int)((end - beg + 63) / 64), i / 9, i % 9, s, cnt[i]});
                }
            std::stable_sort(out.begin(), out.end(), [](const Entry &x, const Entry &y) { return x.steps > y.steps; });
        };
        // entry e belongs to XCD e % 8, its tpe tiles side by side
        auto makespan = [&](const std::vector<Entry> &es) {
            return dispatch_makespan(cus, [&](int x, int b) {
                const size_t e = (size_t)x + 8 * (size_t)(b / tpe);
                return e < es.size() ? (double)(es[e].steps + 8) : -1.0;
            });
        };
        std::vector<Entry> es, best_es;
        std::array<int, 36> counts{}, prev_counts{}, best_counts{};
        double best = -1.0;
        auto counts_for = [&](long long L) -> int {                                             // -> planes, without the entries
            int planes = 0;
            for (int i = 0; i < ntap; i++) planes += (counts[i] = Kc[i] ? count_for(i, L) : 0);
            return planes;
        };
        // (from the longest workgroups down; ties: the longer workgroups.  An L that cuts every tap as the one before it did is the same
        // list and is not priced again; the counts grow as L falls, so the search ends at the first L whose planes outgrow the workspace)
        for (long long L = max_steps; L >= 1; L--) {
            const int planes = counts_for(L);
            if (planes > cap) break;
            if (L < max_steps && counts == prev_counts) continue;
            prev_counts = counts;
            entries_for(es, counts.data());
            const double cost = makespan(es) + planes * plane_price;
            if (best < 0.0 || cost < best) { best = cost; best_es = es; best_counts = counts; }
        }
        WgradPlan p;
        p.words.assign(kPlanHdr, 0u);
        for (int i = 0, plane = 0; i < ntap; i++) {
            p.words[2 * i] = (uint32_t)best_counts[i];
            p.words[2 * i + 1] = (uint32_t)plane;
            plane += best_counts[i];
            p.planes = plane;
        }
        for (const Entry &e : best_es)
            p.words.push_back((uint32_t)e.grp | (uint32_t)e.tap << 2 | (uint32_t)e.split << 6 | (uint32_t)e.count << 14);
        p.nent = (int)best_es.size();
        return p;
    });
}

// ---- the merged backward grid (conv_igemm_bwd_kernel) of one layer whose data gradient is nd tiles: the pixel split of the weight
// gradient half, chosen for THIS grid — its workgroups fill the CUs the data gradient's tiles leave idle and then the whole chip;
// what counts is when the last of them ends — and whether the weight gradient's workgroups take the first block ids.  Blocks go
// to the XCDs round-robin by id, the second half from the next multiple of 8.  -> (ksplit, w_first)
// The search simulates up to 2 x 128 grids of ~1 000 blocks — 0.25 - 0.5 ms of host time, as much as the launch runs on the
// GPU: decided once per geometry (a ResNet-101 step has 77 of these launches)
inline std::pair<int, int> merged_backward_split(int B, int H, int W, int cin, int cout, int k, int nd, int cus) {
    static PlanMemo<std::array<int, 8>, std::pair<int, int>> memo;
    return memo.get({B, H, W, cin, cout, k, nd, cus}, [&] {
        const long long M = (long long)B * H * W;
        const int tiles = ((cout + 255) / 256) * wgrad_col_tiles(cin, k), ks0 = wgrad_uniform_ksplit(1, M, cin, cout, k, false), cap = wgrad_ksplit_cap(M, ks0);
        const double td = ((cout / 64) * k * k + 6) * 1.85;                  // us per data-gradient tile: K-steps + prologue / epilogue
        auto makespan = [&](int n0, double t0, int n1, double t1) {          // n0 blocks of t0 us first, then n1 of t1
            return dispatch_makespan(cus, [&](int x, int b) {
                const int n0x = std::max((n0 - x + 7) / 8, 0), n1x = std::max((n1 - x + 7) / 8, 0);
                return b < n0x ? t0 : b < n0x + n1x ? t1 : -1.0;
            });
        };
        // (the block order is searched too for the shapes round 6 added — 1x1 layers, channel counts below 256: their data-gradient
        // tiles are a few K-steps long, and long weight-gradient workgroups dispatched LAST would run on alone; the 3x3 layers of
        // the VGG path keep the order they were tuned with)
        const bool order_free = k == 1 || cin < 256 || cout < 256;
        double best = -1.0;
        std::pair<int, int> pick(ks0, 0);
        for (int ks = 1; ks <= cap; ks++) {
            const long long chunk = ((M + ks - 1) / ks + 63) / 64 * 64;
            if ((long long)(ks - 1) * chunk >= M) continue;                  // an empty last split
            const double tw = (chunk / 64 + 8) * 2.3;                        // us per weight-gradient workgroup: steps + partial tile out
            const double tail = 3.0 + 2.4 * ks * ((double)cout * k * k * cin / (512.0 * 4608.0));
            const double t = makespan(nd, td, tiles * ks, tw) + tail;
            if (best < 0.0 || t < best) { best = t; pick = {ks, 0}; }
            if (order_free) {
                const double t2 = makespan(tiles * ks, tw, nd, td) + tail;
                if (t2 < best) { best = t2; pick = {ks, 1}; }
            }
        }
        return pick;
    });
}

// ---- the merged backward grid of a launch of 1 - 4 GROUPS (the four ASPP branches: fc7 x4, 1x1; fc6 x4, 3x3 with dilations 6 - 24).
// Its blocks do not cost the same — a class-ordered data-gradient tile runs its live taps only, a work-list entry its own K-steps —
// so both halves are priced block by block, in block-id order, exactly as the kernels decode their ids: the two shapes below
// hold what prepare_igemm / prepare_wgrad decided (conv_igemm.hip; dgrad_shape_for / wgrad_shape_for decide the same from the
// geometry alone, for the CPU check and cross-checked by the launcher), dgrad_block_costs / wgrad_block_costs turn them into us
// per block (a block that exits at once costs 0), merged_grid_makespan runs one order of the two lists through dispatch_makespan
// with the second half starting at the next multiple of 8, and merged_groups_plan picks.
struct DgradShape {
    int ngroups, B, H, W, kch, taps, tiles_m, tiles_n, xcd_mix, row_tiles, cls_tiles, skip_taps, grid, dil[4];      // kch: 64-channel chunks of g
};
struct WgradShape {
    int ngroups, B, H, W, cin, cout, taps, tiles_n, tiles_c, ksplit, compact, xcd_mix, nent, grid, dil[4];
    const uint32_t *plan;           // nullptr, or the work list's words (WgradPlan::words: host memory)
};

// live taps of every pixel tile of one group, in tile order (tile_taps's three tilings, tile by tile)
inline std::vector<int> tile_tap_list(int B, int H, int W, int d, int mode) {
    const long long M = (long long)B * H * W;
    std::vector<int> out;
    if (mode == 1) {
        const int r = kBM / W;
        for (int b = 0; b < B; b++)
            for (int y0 = 0; y0 < H; y0 += r) out.push_back(__builtin_popcount(tap_mask_rect(H, W, d, y0, std::min(H, y0 + r), 0, W)));
        return out;
    }
    HostClass c[kMaxClasses];
    const int n = mode == 2 ? build_classes(H, W, d, c) : 0;
    long long q0[kMaxClasses + 1] = {0};
    for (int k = 0; k < n; k++) q0[k + 1] = q0[k] + (long long)B * (c[k].y1 - c[k].y0) * (c[k].x1 - c[k].x0);
    for (long long t0 = 0; t0 < M; t0 += kBM) {
        const long long t1 = std::min(M, t0 + kBM);
        uint32_t m = 0;
        for (int k = 0; k < n; k++)
            if (q0[k] < t1 && q0[k + 1] > t0) m |= c[k].mask;
        for (long long p = t0; mode == 0 && p < t1;) {
            const int rem = (int)(p % ((long long)H * W)), y = rem / W, x = rem % W;
            const int x1 = (int)std::min<long long>(W, x + (t1 - p));
            m |= tap_mask_rect(H, W, d, y, y + 1, x, x1);
            p += x1 - x;
        }
        out.push_back(__builtin_popcount(m));
    }
    return out;
}

// the data gradient of a forward convolution cin -> cout: g has cout channels (the K axis), gx has cin (the output columns)
inline DgradShape dgrad_shape_for(int ngroups, int B, int H, int W, int cin, int cout, int k, const int *dil, const IgemmVariant &v) {
    DgradShape s{};
    const long long M = (long long)B * H * W;
    s.ngroups = ngroups; s.B = B; s.H = H; s.W = W; s.kch = cout / 64; s.taps = k * k;
    s.tiles_m = (int)((M + kBM - 1) / kBM);
    s.tiles_n = (cin + kBN - 1) / kBN;
    s.skip_taps = v.skip_dead_steps;
    for (int g = 0; g < ngroups; g++) {
        s.dil[g] = dil ? dil[g] : 1;
        if (s.skip_taps && k == 3 && s.dil[g] >= 3) s.xcd_mix = 1;
    }
    const bool rows_ok = s.xcd_mix && W <= kBM && conv_igemm_row_tiles(H, W);
    if (s.xcd_mix && v.class_tiles_allowed && H <= 255 && W <= 255 && (class_order_pays(B, H, W, s.dil, ngroups, rows_ok) || v.class_tiles_forced))
        s.cls_tiles = 1;
    if (!s.cls_tiles && rows_ok) {
        s.row_tiles = 1;
        s.tiles_m = B * ((H + kBM / W - 1) / (kBM / W));
    }
    s.grid = s.xcd_mix ? 8 * ngroups * ((s.tiles_m + 7) / 8) * s.tiles_n : s.tiles_m * s.tiles_n * ngroups;
    return s;
}
// the weight gradient of the same launch; forced_ksplit > 0: that uniform split, no work list (prepare_wgrad's rule)
inline WgradShape wgrad_shape_for(int ngroups, int B, int H, int W, int cin, int cout, int k, const int *dil, const IgemmVariant &v,
                                  int forced_ksplit, int cus) {
    WgradShape s{};
    const long long M = (long long)B * H * W;
    s.ngroups = ngroups; s.B = B; s.H = H; s.W = W; s.cin = cin; s.cout = cout; s.taps = k * k;
    s.tiles_n = (cout + 255) / 256;
    s.tiles_c = wgrad_col_tiles(cin, k);
    for (int q = 0; q < ngroups; q++) s.dil[q] = dil ? dil[q] : 1;
    const WgradPlan *p = (forced_ksplit <= 0 && wgrad_wants_plan(v, dil, ngroups, cin, k)) ? &build_wgrad_plan(ngroups, B, H, W, cin, cout, dil, cus) : nullptr;
    s.ksplit = forced_ksplit > 0 ? forced_ksplit : wgrad_uniform_ksplit(ngroups, M, cin, cout, k, wgrad_wants_mix(dil, ngroups, k));
    for (int q = 0; q < ngroups; q++) {
        if (v.skip_dead_steps && k == 3 && s.dil[q] >= 3 &&
            (s.ksplit % 8 == 0 || (8 % s.ksplit == 0 && (s.tiles_n * s.tiles_c) % (8 / s.ksplit) == 0))) s.xcd_mix = 1;
        if (v.skip_dead_steps && v.wgrad_compact && k == 3 && cin != 128 && s.dil[q] >= 1) s.compact = 1;
    }
    s.grid = s.tiles_n * s.tiles_c * s.ksplit * ngroups;
    if (p) {
        s.plan = p->words.data();
        s.nent = p->nent;
        s.grid = (s.nent + 7) / 8 * 8 * (s.tiles_n * ((cin + 255) / 256));
    }
    return s;
}

// conv_igemm_body's tile map: block id of the half -> (group, pixel tile, channel tile); false: the block exits at once
inline bool dgrad_block_tile(const DgradShape &s, int id, int &grp, int &tm, int &tn) {
    const int xcd = id & 7, k = id >> 3;
    if (s.xcd_mix) {
        const int cm = (s.tiles_m - xcd + 7) >> 3, per_group = cm * s.tiles_n;
        if (cm <= 0 || k >= per_group * s.ngroups) return false;
        grp = k / per_group;
        const int r = k - grp * per_group, tml = r / s.tiles_n;
        tn = r - tml * s.tiles_n;
        tm = xcd + 8 * tml;
        return true;
    }
    const int q = s.grid >> 3, r = s.grid & 7, per_group = s.tiles_m * s.tiles_n;
    int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    grp = t / per_group;
    t -= grp * per_group;
    tm = t / s.tiles_n;
    tn = t - tm * s.tiles_n;
    return true;
}
// conv_igemm_wgrad_body's three maps: block id of the half -> (group, pixel split of ksp, output tile t); false: the block exits at once
inline bool wgrad_block_unit(const WgradShape &s, int id, int &grp, int &split, int &ksp, int &t) {
    const int xcd = id & 7, k = id >> 3, tiles = s.tiles_n * s.tiles_c;
    ksp = s.ksplit;
    if (s.plan) {
        const int ncb = (s.cin + 255) >> 8, tpe = s.tiles_n * ncb, pos = k / tpe, te = k - pos * tpe, e = pos * 8 + xcd;
        if (e >= s.nent) return false;
        const uint32_t w = s.plan[kPlanHdr + e];
        grp = (int)(w & 3u);
        split = (int)((w >> 6) & 255u);
        ksp = (int)((w >> 14) & 255u);
        t = (te / ncb) * s.tiles_c + (int)((w >> 2) & 15u) * ncb + te % ncb;
    } else if (s.xcd_mix && s.ksplit >= 8) {
        const int per_group = (s.ksplit >> 3) * tiles;
        grp = k / per_group;
        const int r = k - grp * per_group;
        split = xcd + 8 * (r / tiles);
        t = r % tiles;
    } else if (s.xcd_mix) {
        const int xpc = 8 / s.ksplit, per_group = tiles / xpc;
        split = xcd / xpc;
        grp = k / per_group;
        t = xcd % xpc + xpc * (k - grp * per_group);
    } else {
        const int q = s.grid >> 3, r = s.grid & 7, tiles_per_group = tiles * s.ksplit;
        t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
        grp = t / tiles_per_group;
        t -= grp * tiles_per_group;
        split = t / tiles;
        t -= split * tiles;
    }
    return true;
}

// us per block, in block-id order: a tile costs its live K-steps + 6 at 1.85 us (merged_backward_split's price)
inline std::vector<double> dgrad_block_costs(const DgradShape &s) {
    std::vector<std::vector<int>> live(s.ngroups);
    for (int g = 0; g < s.ngroups; g++) {
        if (s.taps == 9 && s.skip_taps) live[g] = tile_tap_list(s.B, s.H, s.W, s.dil[g], s.cls_tiles ? 2 : s.row_tiles ? 1 : 0);
        else live[g].assign((size_t)s.tiles_m, s.taps);
    }
    std::vector<double> c((size_t)std::max(s.grid, 0), 0.0);
    for (int id = 0; id < s.grid; id++) {
        int grp, tm, tn;
        if (dgrad_block_tile(s, id, grp, tm, tn)) c[(size_t)id] = (s.kch * live[grp][(size_t)tm] + 6) * 1.85;
    }
    return c;
}
// ... conv_igemm_wgrad_body's three maps: a workgroup costs its K-steps + 8 at 2.3 us
inline std::vector<double> wgrad_block_costs(const WgradShape &s) {
    std::vector<double> c((size_t)std::max(s.grid, 0), 0.0);
    const long long M = (long long)s.B * s.H * s.W;
    const bool two = s.cin == 128 && s.taps == 9;
    const int ncb = two ? 1 : (s.cin + 255) >> 8;
    for (int id = 0; id < s.grid; id++) {
        int grp, split, ksp, t;
        if (!wgrad_block_unit(s, id, grp, split, ksp, t)) continue;
        const int tc = t % s.tiles_c, tap = two ? 2 * tc : tc / ncb;
        long long Kc = M, chunk = ((M + s.ksplit - 1) / s.ksplit + 63) / 64 * 64;
        if (s.compact && !two && s.taps == 9) {
            const int rh = s.H - abs((tap / 3 - 1) * s.dil[grp]), rw = s.W - abs((tap % 3 - 1) * s.dil[grp]);
            Kc = (rh > 0 && rw > 0) ? (long long)s.B * rh * rw : 0;
            chunk = ((Kc + ksp - 1) / ksp + 63) / 64 * 64;
        }
        const long long beg = split * chunk, end = std::min(Kc, beg + chunk);
        c[(size_t)id] = ((end > beg ? (end - beg + 63) / 64 : 0) + 8) * 2.3;
    }
    return c;
}

// when the last block of the grid [first | padding to a multiple of 8 | second] ends (an empty second: the first launched alone)
inline int merged_second_half_start(int n_first) { return (n_first + 7) & ~7; }      // both halves keep their block-id -> XCD relation
inline double merged_grid_makespan(const std::vector<double> &first, const std::vector<double> &second, int cus) {
    const size_t n0 = first.size(), pad = (size_t)merged_second_half_start((int)n0);
    return dispatch_makespan(cus, [&](int x, int b) {
        const size_t id = (size_t)x + 8 * (size_t)b;
        if (id < n0) return first[id];
        if (id < pad) return 0.0;
        return id - pad < second.size() ? second[id - pad] : -1.0;
    });
}

struct MergedGroupsPlan {
    bool merge;                     // one grid (conv_igemm_bwd_kernel) — else the two halves as two launches
    int w_first;                    // the weight gradient's workgroups take the first block ids
    int ksplit;                     // the weight gradient's uniform pixel split for this grid (0: it runs its work list, as it does alone)
    double merged_us, separate_us;  // the model's price of the choice and of the two launches (both with the reduction's share)
};
// one pair of cost lists: the cheaper block order — where the model prices both alike (it runs one workgroup per CU at a time,
// the chip two: fc7 x4's 256 weight-gradient workgroups are exactly one round of its 256 CUs, and every order comes out as the two
// launches one behind the other), the half with the longest block goes first, as list scheduling would have it: its blocks then
// run beside the other half's instead of alone at the end — merged where the model does not price it above the two launches.
// An empty half leaves nothing to merge
inline MergedGroupsPlan merged_groups_decide(const std::vector<double> &dcost, const std::vector<double> &wcost, int cus) {
    MergedGroupsPlan p{false, 0, 0, 0.0, 0.0};
    const std::vector<double> none;
    p.separate_us = merged_grid_makespan(dcost, none, cus) + merged_grid_makespan(wcost, none, cus);
    p.merged_us = p.separate_us;
    if (dcost.empty() || wcost.empty()) return p;
    const double d_first = merged_grid_makespan(dcost, wcost, cus), w_first = merged_grid_makespan(wcost, dcost, cus);
    p.w_first = w_first < d_first || (w_first == d_first && *std::max_element(wcost.begin(), wcost.end()) > *std::max_element(dcost.begin(), dcost.end()));
    p.merged_us = std::min(d_first, w_first);
    p.merge = p.merged_us <= p.separate_us;
    if (!p.merge) p.merged_us = p.separate_us;
    return p;
}
// The plan of a launch: d as prepared; the weight gradient either keeps its work list (fc6 x4: its bits stay those of the launch
// alone) or — a uniform split on the plain map (fc7 x4) — has its split searched for THIS grid among 1 .. the bound its workspace
// was sized for: fc7 x4's four splits are 256 workgroups of 106 K-steps, exactly one round of the chip with nothing to fill, two
// splits are 128 workgroups that take half the CUs for the whole launch while the 1 696 data-gradient tiles run on the other
// half.  Every split is priced with its share of the reduction as merged_backward_split prices it (3 us + 2.4 us per 512 x 4608
// floats of partials); the price of the two launches is that of the split the launch runs alone.  forced_ksplit > 0 (tests): that
// split only, where the workspace holds it.  Decided once per key
inline const MergedGroupsPlan &merged_groups_plan(const DgradShape &d, int cin, int cout, int k, const IgemmVariant &v, int forced_ksplit, int cus) {
    static PlanMemo<std::array<int, 20>, MergedGroupsPlan> memo;
    const int vbits = v.skip_dead_steps | v.class_tiles_allowed << 1 | v.class_tiles_forced << 2 | v.wgrad_work_list << 3 | v.wgrad_compact << 4;
    const std::array<int, 20> key = {d.ngroups, d.B, d.H, d.W, cin, cout, k, d.dil[0], d.dil[1], d.dil[2], d.dil[3], d.tiles_m, d.xcd_mix,
                                     d.row_tiles, d.cls_tiles, d.skip_taps, d.grid, vbits, forced_ksplit, cus};
    return memo.get(key, [&] {
        const long long M = (long long)d.B * d.H * d.W;
        const std::vector<double> dcost = dgrad_block_costs(d);
        const WgradShape w0 = wgrad_shape_for(d.ngroups, d.B, d.H, d.W, cin, cout, k, d.dil, v, 0, cus);
        auto priced = [&](const WgradShape &w) {
            double planes = (double)w.ksplit * w.taps * d.ngroups;
            if (w.plan) { planes = 0.0; for (int i = 0; i < d.ngroups * 9; i++) planes += (double)w.plan[2 * i]; }
            const double tail = 3.0 + 2.4 * planes * ((double)cout * cin / (512.0 * 4608.0));
            MergedGroupsPlan p = merged_groups_decide(dcost, wgrad_block_costs(w), cus);
            p.merged_us += tail;
            p.separate_us += tail;
            p.ksplit = w.plan ? 0 : w.ksplit;
            return p;
        };
        MergedGroupsPlan best = priced(w0);
        const double separate = best.separate_us;
        if (!w0.plan && (forced_ksplit > 0 || !wgrad_wants_mix(d.dil, d.ngroups, k))) {
            const int bound = wgrad_ksplit_bound(d.ngroups, d.B, d.H, d.W, cin, cout, k);
            for (int ks = 1; ks <= bound; ks++) {
                if ((long long)(ks - 1) * (((M + ks - 1) / ks + 63) / 64 * 64) >= M) continue;      // an empty last split
                if (forced_ksplit > 0 ? ks != forced_ksplit : ks == w0.ksplit) continue;
                const MergedGroupsPlan p = priced(wgrad_shape_for(d.ngroups, d.B, d.H, d.W, cin, cout, k, d.dil, v, ks, cus));
                if (forced_ksplit > 0 || (p.merge && p.merged_us < best.merged_us)) best = p;
            }
        }
        if (forced_ksplit <= 0) {
            best.separate_us = separate;
            best.merge = best.merge && best.merged_us <= separate;
            if (!best.merge) { best.merged_us = separate; best.ksplit = w0.plan ? 0 : w0.ksplit; }      // two launches: the split of the launch alone
        }
        return best;
    });
}

}  // namespace dsrg
