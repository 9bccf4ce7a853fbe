// Implicit-GEMM 3x3 (dilated) / 1x1 convolutions for the wide layers of the backbone: conv3_x at 81x81, conv4_x / conv5_x
// (dilation 1 / 2) and the four fc6_k (dilation 6 / 12 / 18 / 24) / fc7_k at 41x41 of train-s.prototxt:161-736 — backbone
// plumbing, no reference counterpart (Caffe's Convolution layer lives in the external framework).  One kernel serves the
// forward (bias + ReLU in the epilogue) and the data gradient (the same convolution of g with the flipped kernel, channel axes
// swapped: the caller packs the weights that way).
//
// Why it exists: the im2col route writes and re-reads a 9x copy of every activation (248 MB per 512-channel layer at batch 16,
// 1.2 ms per step in all) only so that a library GEMM can find its A operand contiguous.  Here the A operand is gathered:
//
//   out[m][n] = sum over (cc, tap, c) of  x[pixel(m) + tap offset][cc*64 + c] * w[n][cc][tap][c]
//
//   * tile 256 pixels x 256 output channels x 64 reduction elements (one tap of one 64-channel chunk per K-step), 8 waves
//     (2 across the channels x 4 across the pixels), product taken transposed (rows = output channels, columns = pixels) so
//     that a lane ends with runs of four consecutive channels of ONE pixel;
//   * the forward / data-gradient body multiplies with v_mfma_f32_16x16x32_bf16: a wave's 128 channels x 64 pixels are 8 x 4
//     blocks of 16 x 16 (128 accumulator registers, as before), a K-step is two 32-deep slices of 32 MFMAs; the four pixel
//     fragments of a slice are held, the eight channel fragments stream through a ring three fragments ahead of their MFMAs
//     (igemm_mma_step).  Same FLOPs, LDS bytes and DMA as on 32x32x16, bit-identical results, every layer 2-7 % faster
//     (profiles/mfma_shape_igemm_probe.txt: the shape is a lever on the clock the chip holds under this load).  The weight-gradient body is still on v_mfma_f32_32x32x16_bf16;
//   * both operand tiles go global -> LDS by `buffer_load_dwordx4 ... lds` (no staging registers, no ds_write pass): a wave
//     instruction moves 8 rows of 128 bytes; the per-lane SOURCE offset is free, so the gather of the pixel rows (one
//     128-byte line per pixel, shifted by the tap's offset) costs one v_add + one v_cndmask per load, and a pixel whose tap
//     falls outside the map gets an offset beyond the descriptor's range, which the hardware answers with zeros;
//   * LDS rows are 128 bytes = 8 chunks of 16 bytes; chunk c of row r is stored at chunk position c ^ ((r >> 1) & 7)
//     (permuting the SOURCE chunk per lane — the LDS destination of the DMA is lane-linear), which spreads the 16 rows a
//     ds_read_b128 lane group touches over all 64 banks;
//   * K order: 64-channel chunk outer, tap inner — the nine taps re-read the same (shifted) 128-byte lines of a pixel
//     neighbourhood back to back, so they hit the XCD's L2; weights are packed [n][cc][tap][64] to match;
//   * two LDS stages of 64 KB: the DMA of K-step s + 1 is in flight while step s is multiplied, one barrier per step;
//   * up to four independent problems (the four ASPP branches: same geometry, own input / weights / dilation / output) share
//     a launch, so that the 424 tiles of one fc6 become 1696 and fill 256 CUs to 95 % instead of 83 %;
//   * epilogue: bias (+ ReLU) on the fp32 accumulators, bf16 pack, through LDS for 16-byte coalesced NHWC stores.
//
// Host side (behind the kernels): every launch is PREPARED (prepare_igemm / prepare_wgrad: validate, fill the argument block,
// state the grid and the form; nothing is enqueued) and then RUN (run_igemm / run_wgrad, or the merged backward grid over both
// prepared halves); what a launch depends on is in those functions' parameters.  The decisions themselves — tile maps, class
// order, pixel splits, work lists, the merged grid's split and order, the debug variants — are plain C++ in igemm_plan.h (which
// also holds kBM, kBN, kMaxClasses and kPlanHdr), checked on the CPU by tests/test_igemm_plan.py.
#include "common.h"
#include "igemm_plan.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace dsrg {
namespace {
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(3))) void lds_void;

constexpr int kOutRow = 128 * 2 + 16;                      // epilogue: a wave's 64 pixels x 128 channels, padded rows
constexpr int kOutWave = 64 * kOutRow;
constexpr uint32_t kOob = 0x80000000u;                     // beyond any descriptor of this kernel: the load returns zeros
constexpr int kRowTab = 8 * kOutWave;                      // cls_tiles: the pixel of each of the tile's 256 rows (int32, -1 = none), behind
constexpr int kRowTabBytes = kBM * 4;                      // the stages and the epilogue's staging rows

// BK = reduction elements per K-step, NST = LDS stages: (64, 2) — one step in flight behind the one being multiplied.
template <int BK, int NST> struct ICfg {
    static constexpr int ROW = BK * 2;                     // bytes per LDS row
    static constexpr int CPR = ROW / 16;                   // 16-byte chunks per row (8 / 4)
    static constexpr int RPI = 1024 / ROW;                 // rows one wave DMA instruction moves (8 / 16)
    static constexpr int IPW = 256 / RPI / 8;              // DMA instructions per wave, tile and step (4 / 2)
    static constexpr int STAGE = (kBM + kBN) * ROW;        // pixel rows, then weight rows (64 / 32 KB)
    static constexpr int KS = BK / 16;                     // MFMA k-slices per step
    static constexpr int SPC = 64 / BK;                    // steps per 64-channel chunk of a tap
    static constexpr int AHEAD = NST - 1;
    static_assert(NST * STAGE <= kRowTab, "the row table sits behind the stages");
    static constexpr size_t LDS = (size_t)kRowTab + kRowTabBytes;
    // chunk c of row r is stored at chunk position c ^ swz(r): the 16 rows a ds_read_b128 lane group touches then cover
    // all 64 banks (rows of 128 B: 2 rows per 256-byte bank line -> 3 bits from r >> 1; rows of 64 B: 4 per line -> r >> 2)
    __device__ static constexpr int swz(int r) { return BK == 64 ? (r >> 1) & 7 : (r >> 2) & 3; }
};

// a rectangle [y0, y0 + h) x [x0, x0 + w) of every image of the batch; its pixels (image-major, raster order inside) take the
// indices q0 .. q0 + B h w - 1 of the launch's pixel order (IgemmArgs::cls_tiles)
struct IgemmClass {
    uint32_t rect;          // y0 | h << 8 | x0 << 16 | w << 24
    int q0;
};
struct IgemmGroup {
    const uint16_t *x;      // (B, H, W, Cin) bf16
    const uint16_t *w;      // (Cout, Cin / 64, taps, 64) bf16
    const float *bias;      // (Cout) or nullptr
    uint16_t *y;            // (B, H, W, Cout) bf16
    const uint16_t *mask;   // (B, H, W, Cout) bf16 or nullptr: outputs are kept where mask > 0 (times out_scale), else zeroed —
                            // the ReLU (+ Dropout) backward of the layer below, when this launch is a data gradient
    float *colsum;          // (tiles_m, Cout) fp32 or nullptr: per 256-row tile, the column sums of what was stored —
                            // the partial bias gradient of the layer below (summed in fixed order by igemm_colsum_kernel)
    const uint16_t *res;    // (B, H, W, Cout) bf16 or nullptr: added to the bf16-rounded result BEFORE the ReLU / the mask — the identity
                            // branch of a residual block in the forward launch (y = relu(bf16(conv + bias) + res): bit for bit what a separate
                            // add + ReLU pass over the stored convolution gives), the gradient that reaches the block's input past the
                            // convolutions in its first convolution's data gradient (gx = (bf16(conv) + res) where mask > 0)
    int dil, ncls;
    IgemmClass cls[kMaxClasses];    // cls_tiles: the group's pixel order, classes by ascending q0
};
struct IgemmArgs {
    IgemmGroup g[4];
    int ngroups, B, H, W, Cin, Cout, taps, relu, M, tiles_m, tiles_n, tiles_per_group;
    int stagger;            // 1: waves 4-7 issue their DMA behind the first MFMA cluster of a step (their SIMD partners 0-3 issue
                            // in front of theirs), so that no SIMD's matrix pipe waits for both of its waves to get through the issue code
    uint32_t drop_thresh;   // Dropout behind the ReLU, fused: keep an element iff its random byte >= drop_thresh (p = thresh / 256;
    float drop_scale;       // 0 = no dropout), kept elements times drop_scale = 1 / (1 - p)
    uint32_t seed_lo, seed_hi;
    float out_scale;        // every output times this (1 unless a mask carries a Dropout scale)
    int xcd_mix;            // 1: XCD-interleaved tile map (see the kernel); the grid is 8 * ngroups * ceil(tiles_m / 8) * tiles_n blocks
    int row_tiles, rows_per_tile, bands;      // 1: a pixel tile = rows_per_tile whole rows of one image (bands of them per image)
    int skip_taps;          // 1: a K-step whose tap reaches no pixel of the tile (a dilated kernel near the map's border: all of
                            // its operand rows would be the zeros of the padding) is not loaded and not multiplied
    int xrow;               // bytes per pixel row of x (Cin * 2 — or, split mode, the three bf16 planes of a float32 activation: 3 * cin * 2)
    int cpp;                // split mode (0 = off): 64-channel chunks per PLANE.  A float32 convolution as six bf16 products on the fp32
                            // accumulators: x = x0 + x1 + x2 and w = w0 + w1 + w2 (each term the bf16 rounding of what the terms before
                            // leave), the products x0 w0, x0 w1, x1 w0, x0 w2, x2 w0, x1 w1 carry 2^-24-grade relative error; the K loop
                            // runs over 6 * cpp VIRTUAL chunks — virtual chunk v reads plane kSplitXPlane[v / cpp] of x, and the packed
                            // kernel holds plane kSplitWPlane[v / cpp] of w there (the caller's packing)
    int out_f32;            // 1: y is float32 (B, H, W, Cout), written straight from the accumulators (split mode's prototype epilogue)
    int cls_tiles;          // 1: a pixel tile = 256 consecutive indices of the group's CLASS order (IgemmGroup::cls) instead of 256
                            // consecutive pixels: a dilated tap (dy, dx) d reaches exactly the pixels of a rectangle of the map, so the
                            // map falls into <= 3 x 3 rectangles inside each of which every pixel has the SAME live taps; ordered
                            // class by class (most taps first), a tile multiplies padding only where it straddles two classes
};

// the random bytes of the four consecutive channels starting at element 4 * e4 of a launch's output: a counter-based
// generator (two rounds of the murmur3 finaliser over the element counter and the 64-bit seed) — every element's decision is a
// pure function of (seed, position), so the mask needs no state, no extra pass and no storage (the backward pass reads it
// off the sign of the output, as with torch's dropout kernel before)
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t dropout_bytes(uint32_t e4, uint32_t seed_lo, uint32_t seed_hi) {
    return fmix32(fmix32(e4 ^ seed_lo) + seed_hi);
}

__device__ __forceinline__ uint32_t pack2(float lo, float hi) {   // v_cvt_pk_bf16_f32: round to nearest even
    f32x2 v = {lo, hi};
    bf16x2 b = __builtin_convertvector(v, bf16x2);
    return *reinterpret_cast<uint32_t *>(&b);
}

template <int N> __device__ __forceinline__ void wait_vm_barrier() {
    // this wave's DMA up to the step about to be read has landed (N younger loads may still fly), then the workgroup barrier:
    // everybody's has, and everybody is done reading the stage the next issue overwrites.  One asm statement with a memory
    // clobber: neither LDS reads nor the DMA issue may move across it.
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// One 64-deep K-step of a wave's 128 channels x 64 pixels on v_mfma_f32_16x16x32_bf16: 8 x 4 blocks of 16 x 16, two 32-deep slices of
// 32 MFMAs.  A fragment is one ds_read_b128: lane l reads row l & 15 of a 16-row block, chunk 4 * slice + (l >> 4) through the
// swizzle (choff[slice], IgemmFrag) — the 16 lanes of each of the instruction's four passes fall on 16 different 16-byte slots of
// the 256-byte bank line.  The four pixel fragments of a slice are held (those of slice 1 are read under the first
// four clusters of slice 0); the sixteen channel fragments stream through a ring, kAhead clusters (of 4 MFMAs = 64 cycles) ahead
// of their use — double-buffering whole slices as the 32x32x16 loop did would take 96 fragment registers beside the 128
// accumulators.  Order pinned by sched_barrier.  late_issue: called behind the fourth cluster (256 MFMA cycles into the step,
// where the 32x32x16 loop's first cluster ended) when `late` — the staggered DMA issue of waves 4-7.
constexpr int kAhead = 3;
struct IgemmFrag {
    uint32_t choff[2];
    __device__ __forceinline__ explicit IgemmFrag(int lane) {
        using C = ICfg<64, 2>;
        const int l15 = lane & 15, g4 = lane >> 4;          // (fragment bases are multiples of 16 rows: the swizzle term depends on the lane only)
#pragma unroll
        for (int sl = 0; sl < 2; sl++) choff[sl] = (uint32_t)l15 * C::ROW + (uint32_t)(((sl * 4 + g4) ^ C::swz(l15)) << 4);
    }
};
template <class LateIssue>
__device__ __forceinline__ void igemm_mma_step(const unsigned char *P, const unsigned char *Wt, const IgemmFrag &fr, f32x4 (&acc)[8][4],
                                               const bool late, LateIssue &&late_issue) {
    using C = ICfg<64, 2>;
    constexpr int RING = kAhead + 1;
    bf16x8 bq[2][4], ar[RING];
    auto read_w = [&](int u) { return *reinterpret_cast<const bf16x8 *>(Wt + (u & 7) * (16 * C::ROW) + fr.choff[u >> 3]); };
#pragma unroll
    for (int j = 0; j < 4; j++) bq[0][j] = *reinterpret_cast<const bf16x8 *>(P + j * (16 * C::ROW) + fr.choff[0]);
#pragma unroll
    for (int u = 0; u < kAhead; u++) ar[u] = read_w(u);
#pragma unroll
    for (int u = 0; u < 16; u++) {                          // cluster u: channel block u & 7 of slice u >> 3 against the slice's four pixel blocks
        if (u + kAhead < 16) ar[(u + kAhead) % RING] = read_w(u + kAhead);
        if (u < 4) bq[1][u] = *reinterpret_cast<const bf16x8 *>(P + u * (16 * C::ROW) + fr.choff[1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; j++)
            acc[u & 7][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ar[u % RING], bq[u >> 3][j], acc[u & 7][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (u == 3 && late) late_issue();
    }
}

__device__ __forceinline__ void conv_igemm_body(const IgemmArgs &a, const int bid, const int nblk) {      // block bid of nblk (a merged launch passes a sub-range)
    using C = ICfg<64, 2>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ig_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;
    const int wn = wv >> 2, wm = wv & 3;

    // tile of this workgroup: consecutive ids share an XCD (blockIdx % 8) in runs, n-tile fastest.
    // xcd_mix (launches that skip taps): tiles no longer cost the same — a dilation-24 tile runs 3 to 6 of its 9 taps, a
    // dilation-6 tile all of them — and an XCD only ever runs the blocks with its own id % 8: with runs of consecutive tiles
    // per XCD the two XCDs that hold fc6_1's tiles set the launch's duration while those with fc6_4's idle (measured: skipping
    // 15 % of the steps bought 0 %).  There XCD x takes the pixel tiles x, x + 8, .. of EVERY group (its blocks in the
    // order group, pixel tile, n-tile), so that all XCDs hold the same mix; blocks beyond an XCD's share exit at once.
    int grp, tm, tn;
    if (a.xcd_mix) {
        const int id = bid, xcd = id & 7, k = id >> 3;
        const int cm = (a.tiles_m - xcd + 7) >> 3, per_group = cm * a.tiles_n;
        if (cm <= 0 || k >= per_group * a.ngroups) return;
        grp = k / per_group;
        const int r = k - grp * per_group, tml = r / a.tiles_n;
        tn = r - tml * a.tiles_n;
        tm = xcd + 8 * tml;
    } else {
        const int total = nblk, id = bid;
        const int q = total >> 3, r = total & 7, xcd = id & 7, k = id >> 3;
        int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
        grp = t / a.tiles_per_group;
        t -= grp * a.tiles_per_group;
        tm = t / a.tiles_n;
        tn = t - tm * a.tiles_n;
    }
    // the tile's pixels: 256 consecutive ones — or (row_tiles: launches that skip taps) whole map rows of ONE image, as many as fit
    // 256: a tile that straddles two images reaches every vertical tap through one of them and skips nothing, a tile aligned to
    // rows skips more (41-wide map, six rows = 246 pixels per tile: 5 % fewer K-steps over the four fc6_k than flattened tiles)
    int m0 = tm * kBM, mvalid;
    if (a.row_tiles) {
        const int bimg = tm / a.bands, band = tm - bimg * a.bands, row0 = band * a.rows_per_tile;
        m0 = (bimg * a.H + row0) * a.W;
        mvalid = min(a.rows_per_tile, a.H - row0) * a.W;
    } else {
        mvalid = min(kBM, a.M - m0);
    }
    const int n0 = tn * kBN;
    const IgemmGroup &G = a.g[grp];
    const int taps = a.taps, Cin = a.Cin, W = a.W, H = a.H;
    const int ktot = taps * Cin;
    // cls_tiles: row r of the tile is index m0 + r of the group's class order; its pixel goes to the row table (one row per
    // thread: a search over <= 9 classes and two divisions), which the DMA geometry and the epilogue read
    volatile int32_t *rowpix = reinterpret_cast<volatile int32_t *>(ig_lds + kRowTab);
    const bool cls = a.cls_tiles != 0;
    if (cls) {
        if (tid < kBM) {
            const int q = m0 + tid;
            int m = -1;
            if (q < a.M) {
                uint32_t rect = G.cls[0].rect;
                int q0 = G.cls[0].q0;
#pragma unroll
                for (int k = 1; k < kMaxClasses; k++)
                    if (k < G.ncls && q >= G.cls[k].q0) { rect = G.cls[k].rect; q0 = G.cls[k].q0; }
                const int cy0 = (int)(rect & 255u), ch = (int)((rect >> 8) & 255u), cx0 = (int)((rect >> 16) & 255u), cw = (int)(rect >> 24);
                const int qq = q - q0, area = ch * cw, b = qq / area, rem = qq - b * area, yy = rem / cw, xx = rem - yy * cw;
                m = (b * H + cy0 + yy) * W + cx0 + xx;
            }
            rowpix[tid] = m;
        }
        __syncthreads();
    }
    auto row_pixel = [&](int r) -> int { return cls ? rowpix[r] : (r < mvalid ? m0 + r : -1); };      // -1: the tile has no such row

    const int xrow = a.xrow;
    const rsrc_t rx = make_rsrc(G.x, (size_t)a.M * xrow);
    const rsrc_t rw = make_rsrc(G.w, (size_t)a.Cout * ktot * 2);

    // ---- DMA geometry: per K-step a wave moves rows [wv*32 + i*RPI, +RPI) of both tiles; lane -> (row, 16-byte chunk)
    uint32_t pbase[C::IPW], pvalid[C::IPW], wbase[C::IPW];
#pragma unroll
    for (int i = 0; i < C::IPW; i++) {
        const int r = wv * 32 + i * C::RPI + lane / C::CPR;
        const int c = (lane % C::CPR) ^ C::swz(r);         // source chunk that lands at chunk position lane % CPR
        const int m = row_pixel(r);
        const bool in = m >= 0;
        const int mm = in ? m : 0;
        const int hw = H * W;
        const int b = mm / hw, rem = mm - b * hw, y = rem / W, x = rem - y * W;
        uint32_t valid = 0;
        if (in) {
            if (taps == 9) {
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    const int yy = y + (tap / 3 - 1) * G.dil, xx = x + (tap % 3 - 1) * G.dil;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) valid |= 1u << tap;
                }
            } else {
                valid = 1u;
            }
        }
        pbase[i] = (uint32_t)mm * (uint32_t)xrow + (uint32_t)c * 16u;
        pvalid[i] = valid;
        wbase[i] = (uint32_t)(n0 + r) * (uint32_t)(ktot * 2) + (uint32_t)c * 16u;   // rows past Cout lie beyond the descriptor
    }

    // ---- the taps this tile multiplies.  With a dilated kernel whole taps fall into the zero padding for every pixel of a tile
    // (fc6_4, dilation 24 on a 41-row map: the three upper taps reach a pixel only from row 24 on — for the tiles above they
    // are 64-deep K-steps of zeros times weights): the tile's taps are the OR of its pixels' validity bits, and the K loop runs
    // over those only — 15 % of the four fc6_k's steps at 16 images (30 % for dilation 24).  A skipped step adds exact zeros
    // to every accumulator, so results are bit-identical with and without (tests/test_gpu_igemm.py).  Taps stay in their
    // order, chunk outer / tap inner as before; a tile that reaches every tap runs the very same sequence.
    uint32_t tapmask = taps == 9 ? 0x1ffu : 1u;
    if (a.skip_taps && taps == 9 && G.dil >= 3) {           // (workgroup-uniform; below 3 no 256-pixel tile loses a tap)
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < C::IPW; i++) v |= pvalid[i];
#pragma unroll
        for (int o = 32; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
        volatile uint32_t *red = reinterpret_cast<volatile uint32_t *>(ig_lds);
        if (lane == 0) red[wv] = v;
        __syncthreads();
        v = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) v |= red[k];
        __syncthreads();                                    // the words are stage 0's first row again
        tapmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
    unsigned long long taplist = 0;                         // nibble k = the k-th live tap
    int nlive = 0;
#pragma unroll
    for (int tp = 0; tp < 9; tp++)
        if ((tapmask >> tp) & 1u) { taplist |= (unsigned long long)tp << (4 * nlive); nlive++; }
    const int nsteps = (Cin >> 6) * nlive * C::SPC;

    // issue(stage, s): the DMA of K-step s into `stage`; the steps are issued in order, so (chunk, live tap, half) advance as
    // counters instead of being divided out of s
    int it_cc = 0, it_tap = 0, it_h = 0;
    auto issue = [&](int stage, int) {
        const int tap = (int)((taplist >> (4 * it_tap)) & 15u);
        const int cc = it_cc, h = it_h;
        const uint32_t s_real = (uint32_t)((cc * taps + tap) * C::SPC + h);     // position of the step's weights in a packed row
        if (++it_h == C::SPC) { it_h = 0; if (++it_tap == nlive) { it_tap = 0; it_cc++; } }
        int dy = 0, dx = 0;
        if (taps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
        // (split mode: virtual chunk cc -> chunk cc % cpp of plane 0 0 1 0 2 1 [cc / cpp] of x; two bits per entry of 0x610)
        const int xc = a.cpp ? (int)((0x610u >> (2 * (cc / a.cpp))) & 3u) * a.cpp + cc % a.cpp : cc;
        const int toff = (dy * G.dil * W + dx * G.dil) * xrow + xc * 128 + h * C::ROW;      // wave-uniform
        unsigned char *P = ig_lds + stage * C::STAGE + wv * (32 * C::ROW);
        unsigned char *Wt = P + kBM * C::ROW;
#pragma unroll
        for (int i = 0; i < C::IPW; i++) {
            const uint32_t vo = ((pvalid[i] >> tap) & 1u) ? pbase[i] + (uint32_t)toff : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void *)(P + i * (C::RPI * C::ROW)), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < C::IPW; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void *)(Wt + i * (C::RPI * C::ROW)), 16, wbase[i], s_real * C::ROW, 0, 0);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[i][j][r] = 0.0f;

    const IgemmFrag fr(lane);
    // an output-channel count of 128 (mod 256) leaves the upper half of the last n-tile empty: its waves (4-7) only move data
    const bool active = n0 + wn * 128 < a.Cout;
    const bool late = a.stagger && wv >= 4 && active;
    if (nsteps > 0) issue(0, 0);
    // (two loops, not one with the multiply under `if (active)`: a loop in which the accumulators reach the back edge by two paths
    // makes the register allocator copy them around it — this MFMA shape's destination is not tied to its addend)
    if (!active) {                                          // a wave without output columns: it only moves data
        for (int s = 0; s < nsteps; s++) {
            wait_vm_barrier<0>();
            if (s + 1 < nsteps) issue((s & 1) ^ 1, s + 1);
        }
    } else {
        for (int s = 0; s < nsteps; s++) {
            const int stage = s & 1;
            wait_vm_barrier<0>();
            const bool more = s + 1 < nsteps;
            if (more && !late) issue(stage ^ 1, s + 1);
            igemm_mma_step(ig_lds + stage * C::STAGE + wm * (64 * C::ROW), ig_lds + stage * C::STAGE + kBM * C::ROW + wn * (128 * C::ROW), fr, acc,
                           more && late, [&]() { issue(stage ^ 1, s + 1); });
        }
    }
    __syncthreads();                                        // every wave is done reading the last stage
    if (!active) return;

    // ---- epilogue: C[row = channel][col = pixel]; a lane holds channels 16 i + 4 g4 + reg of pixel 16 j + l15 in acc[i][j][reg]
    unsigned char *O = ig_lds + wv * kOutWave;
    const int nw = n0 + wn * 128;
    if (a.out_f32) {
        // float32 result straight from the accumulators: 16 bytes per lane and (i, j) (the layer-level prototype of the split mode; a
        // production epilogue would stage through LDS as the bf16 one does)
        float *y32 = reinterpret_cast<float *>(G.y);
        const float floor32 = a.relu ? 0.0f : -__builtin_inff();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int m = row_pixel(wm * 64 + j * 16 + l15);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int n = nw + i * 16 + g4 * 4;
                float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (G.bias) b4 = *reinterpret_cast<const float4 *>(G.bias + n);
                const float4 v = make_float4(fmaxf(acc[i][j][0] + b4.x, floor32), fmaxf(acc[i][j][1] + b4.y, floor32),
                                             fmaxf(acc[i][j][2] + b4.z, floor32), fmaxf(acc[i][j][3] + b4.w, floor32));
                if (m >= 0) *reinterpret_cast<float4 *>(y32 + (size_t)m * a.Cout + n) = v;
            }
        }
        return;
    }
    const rsrc_t rb = make_rsrc(G.bias, G.bias ? (size_t)a.Cout * 4 : 0);      // no bias: every load is out of range = 0
    const float floor_ = (a.relu && !G.res) ? 0.0f : -__builtin_inff();        // ReLU without a branch per value (behind the residual, if any)
    const uint32_t seed_g = a.seed_lo + (uint32_t)grp * 0x9E3779B9u;              // every branch its own stream
    float bias_r[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int e = 0; e < 4; e++) bias_r[i][e] = ld_f32(rb, (uint32_t)(nw + i * 16 + g4 * 4 + e) * 4u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int nl = i * 16 + g4 * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float v0 = acc[i][j][0] + bias_r[i][0], v1 = acc[i][j][1] + bias_r[i][1];
            float v2 = acc[i][j][2] + bias_r[i][2], v3 = acc[i][j][3] + bias_r[i][3];
            v0 = fmaxf(v0, floor_) * a.out_scale; v1 = fmaxf(v1, floor_) * a.out_scale;
            v2 = fmaxf(v2, floor_) * a.out_scale; v3 = fmaxf(v3, floor_) * a.out_scale;
            if (a.drop_thresh) {                                             // uniform
                const uint32_t m = cls ? (uint32_t)rowpix[wm * 64 + j * 16 + l15] : (uint32_t)(m0 + wm * 64 + j * 16 + l15);
                const uint32_t h = dropout_bytes((m * (uint32_t)a.Cout + (uint32_t)(nw + nl)) >> 2, seed_g, a.seed_hi);
                v0 = (h & 0xffu) >= a.drop_thresh ? v0 * a.drop_scale : 0.0f;
                v1 = ((h >> 8) & 0xffu) >= a.drop_thresh ? v1 * a.drop_scale : 0.0f;
                v2 = ((h >> 16) & 0xffu) >= a.drop_thresh ? v2 * a.drop_scale : 0.0f;
                v3 = (h >> 24) >= a.drop_thresh ? v3 * a.drop_scale : 0.0f;
            }
            // (a 16-lane group of this 8-byte store: 16 pixel rows of 68 dwords, two per bank pair — 2-way, as the 32x32x16 mapping was)
            *reinterpret_cast<uint2 *>(O + (j * 16 + l15) * kOutRow + nl * 2) = make_uint2(pack2(v0, v1), pack2(v2, v3));
        }
    }
    // the wave reads back its own rows only: LDS operations of one wave complete in order
    const bool chv = nw + (lane & 15) * 8 < a.Cout;          // a 64-channel output: the upper half of the wave's 128 columns does not exist
    if (G.res) {                                             // (uniform) residual, then ReLU and / or the mask of the layer below
        const float floor2 = a.relu ? 0.0f : -__builtin_inff();
#pragma unroll
        for (int h = 0; h < 2; h++) {                        // two batches of eight rows: two latencies, half the registers
            uint4 rs[8], mk8[8];
#pragma unroll
            for (int it = 0; it < 8; it++) {
                const int m = row_pixel(wm * 64 + (h * 8 + it) * 4 + (lane >> 4));
                const size_t at = (size_t)m * a.Cout + nw + (lane & 15) * 8;
                rs[it] = (m >= 0 && chv) ? *reinterpret_cast<const uint4 *>(G.res + at) : make_uint4(0, 0, 0, 0);
                mk8[it] = !G.mask ? make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u)
                                  : ((m >= 0 && chv) ? *reinterpret_cast<const uint4 *>(G.mask + at) : make_uint4(0, 0, 0, 0));
            }
#pragma unroll
            for (int it = 0; it < 8; it++) {
                const int p = (h * 8 + it) * 4 + (lane >> 4), ch = lane & 15;
                const int m = row_pixel(wm * 64 + p);
                const uint4 v = *reinterpret_cast<const uint4 *>(O + p * kOutRow + ch * 16);
                uint32_t w4[4] = {v.x, v.y, v.z, v.w};
                const uint32_t r4[4] = {rs[it].x, rs[it].y, rs[it].z, rs[it].w};
                const uint32_t y4[4] = {mk8[it].x, mk8[it].y, mk8[it].z, mk8[it].w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float lo = fmaxf(__uint_as_float(w4[e] << 16) + __uint_as_float(r4[e] << 16), floor2);
                    const float hi = fmaxf(__uint_as_float(w4[e] & 0xffff0000u) + __uint_as_float(r4[e] & 0xffff0000u), floor2);
                    const uint32_t klo = (int16_t)(y4[e] & 0xffffu) > 0 ? 0x0000ffffu : 0u;
                    const uint32_t khi = (int32_t)y4[e] >= 0x10000 ? 0xffff0000u : 0u;
                    w4[e] = pack2(lo, hi) & (klo | khi);
                }
                if (m >= 0 && chv) *reinterpret_cast<uint4 *>(G.y + (size_t)m * a.Cout + nw + ch * 8) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
        }
        return;
    }
    if (!G.mask && !G.colsum) {
#pragma unroll 4
        for (int it = 0; it < 16; it++) {
            const int p = it * 4 + (lane >> 4), ch = lane & 15;
            const int m = row_pixel(wm * 64 + p);
            const uint4 v = *reinterpret_cast<const uint4 *>(O + p * kOutRow + ch * 16);
            if (m >= 0 && chv) *reinterpret_cast<uint4 *>(G.y + (size_t)m * a.Cout + nw + ch * 8) = v;
        }
        return;
    }
    // data gradient with the backward of the ReLU (+ Dropout) below it and that layer's bias gradient: keep a value where the
    // layer's OUTPUT was positive (bf16 halves compared as signed 16-bit integers: +0 and negatives drop), sum what is stored.
    // The accumulators are dead by now: all sixteen mask rows of the lane are fetched in one batch (one latency, not sixteen).
    uint4 mk[16];
    if (G.mask) {
#pragma unroll
        for (int it = 0; it < 16; it++) {
            const int m = row_pixel(wm * 64 + it * 4 + (lane >> 4));
            mk[it] = (m >= 0 && chv) ? *reinterpret_cast<const uint4 *>(G.mask + (size_t)m * a.Cout + nw + (lane & 15) * 8) : make_uint4(0, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int it = 0; it < 16; it++) mk[it] = make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
    }
    float cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int it = 0; it < 16; it++) {
        const int p = it * 4 + (lane >> 4), ch = lane & 15;
        const int m = row_pixel(wm * 64 + p);
        const uint4 v = *reinterpret_cast<const uint4 *>(O + p * kOutRow + ch * 16);
        uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        const uint32_t y4[4] = {mk[it].x, mk[it].y, mk[it].z, mk[it].w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t lo = (int16_t)(y4[e] & 0xffffu) > 0 ? 0x0000ffffu : 0u;
            const uint32_t hi = (int32_t)y4[e] >= 0x10000 ? 0xffff0000u : 0u;       // upper half positive and non-zero
            w4[e] &= lo | hi;                                                        // (rows past the end: mask 0 -> adds 0)
            cs[2 * e] += __uint_as_float(w4[e] << 16);
            cs[2 * e + 1] += __uint_as_float(w4[e] & 0xffff0000u);
        }
        if (m >= 0 && chv) *reinterpret_cast<uint4 *>(G.y + (size_t)m * a.Cout + nw + ch * 8) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
    if (G.colsum) {                                          // uniform for the workgroup
#pragma unroll
        for (int e = 0; e < 8; e++) {
            cs[e] += __shfl_xor(cs[e], 16);
            cs[e] += __shfl_xor(cs[e], 32);
        }
        // the four 64-row slabs of the tile are summed here (fixed order) so that the scratch holds one row per tile.  A wave's
        // own staging region is free again (its reads above have returned: their values were used)
        float *slab = reinterpret_cast<float *>(O);
        if (lane < 16) {
            *reinterpret_cast<float4 *>(slab + lane * 8) = make_float4(cs[0], cs[1], cs[2], cs[3]);
            *reinterpret_cast<float4 *>(slab + lane * 8 + 4) = make_float4(cs[4], cs[5], cs[6], cs[7]);
        }
        __syncthreads();                                     // (waves of a 128-wide n-tile's idle half have left: not counted)
        if (wm == 0) {
            const float *s0 = reinterpret_cast<const float *>(ig_lds + (wn * 4 + 0) * kOutWave);
            const float *s1 = reinterpret_cast<const float *>(ig_lds + (wn * 4 + 1) * kOutWave);
            const float *s2 = reinterpret_cast<const float *>(ig_lds + (wn * 4 + 2) * kOutWave);
            const float *s3 = reinterpret_cast<const float *>(ig_lds + (wn * 4 + 3) * kOutWave);
            float *dst = G.colsum + (size_t)tm * a.Cout + nw;
            dst[lane] = (s0[lane] + s1[lane]) + (s2[lane] + s3[lane]);
            if (nw + lane + 64 < a.Cout) dst[lane + 64] = (s0[lane + 64] + s1[lane + 64]) + (s2[lane + 64] + s3[lane + 64]);
        }
    }
}


__global__ __launch_bounds__(512, 2) void conv_igemm_kernel_64x2(IgemmArgs a) { conv_igemm_body(a, (int)blockIdx.x, (int)gridDim.x); }

// ------------------------------------------------------------------------------------------------------------------
// The same convolution with the K-steps of ALL tiles dealt out evenly ("stream-K"): the 41x41 layers have 212 tiles of 72
// K-steps for 256 CUs — one round with a sixth of the chip idle — and the data gradient of conv4_1 106.  Here the grid is one
// workgroup per CU and workgroup u takes the global K-steps [u T / U, (u + 1) T / U) of the T = tiles x steps of the launch:
// up to one tile it finishes for an earlier workgroup (its first segment), whole tiles, and up to one tile it starts (its last
// segment).  A tile cut this way is completed by the workgroup that holds its FIRST step — that segment is the last thing the
// workgroup does, so the other parts (the first segments of the following workgroups, written to a workspace with
// write-through stores and published by a flag: cdna_hip_programming.md Guideline 16, recipe R1) are there long before it
// looks; it adds them in workgroup order (deterministic) and runs the ordinary epilogue.  Dependencies point to higher
// workgroup ids only and nobody waits before having done all its own work, so the launch cannot deadlock however the
// dispatcher places the workgroups; every wait is bounded all the same (error word set, the tile is then filled with NaNs:
// a timeout under a debugger or profiler turns the step's loss into NaN instead of feeding stale memory to the next layer).
struct IgemmSkArgs {
    IgemmArgs base;
    float *ws;              // [units][32][512] float4: a workgroup's accumulators of its first segment
    uint32_t *flags;        // [units + 1]: published marker per workgroup (zeroed before every launch) + an error word
    int units, tiles_total;
};
constexpr int kSkParts = 4;        // most shares a cut tile can have besides its owner's: the launcher keeps a workgroup's
                                   // run of steps >= a third of a tile
using f32x4v = decltype(__builtin_amdgcn_raw_buffer_load_b128(rsrc_t(), 0, 0, 0));

__global__ __launch_bounds__(512, 2) void conv_igemm_sk_kernel(IgemmSkArgs k) {
    using C = ICfg<64, 2>;
    const IgemmArgs &a = k.base;
    extern __shared__ __attribute__((aligned(16))) unsigned char ig_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;
    const int wn = wv >> 2, wm = wv & 3;
    int unit;
    {
        const int total = (int)gridDim.x, id = (int)blockIdx.x;
        const int q = total >> 3, r = total & 7, xcd = id & 7, kk = id >> 3;
        unit = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + kk;       // neighbours in the step order share an XCD
    }
    const int taps = a.taps, Cin = a.Cin, W = a.W, H = a.H;
    const int ktot = taps * Cin;
    const int nsteps = (Cin >> 6) * taps;
    const long long total_steps = (long long)k.tiles_total * nsteps;
    auto unit_start = [&](int u) { return (long long)u * total_steps / k.units; };
    const long long g1 = unit_start(unit + 1);
    const IgemmFrag fr(lane);
    const rsrc_t rws = make_rsrc(k.ws, (size_t)k.units * 32 * 512 * 16);
    const float floor_ = a.relu ? 0.0f : -__builtin_inff();

    for (long long g = unit_start(unit); g < g1;) {
        const int tile = (int)(g / nsteps);
        const int sb = (int)(g - (long long)tile * nsteps);
        const int se = (int)min((long long)nsteps, sb + (g1 - g));
        int t = tile;
        const int grp = t / a.tiles_per_group;
        t -= grp * a.tiles_per_group;
        const int tm = t / a.tiles_n, tn = t - tm * a.tiles_n;
        const int m0 = tm * kBM, n0 = tn * kBN;
        const IgemmGroup G = a.g[grp];
        const rsrc_t rx = make_rsrc(G.x, (size_t)a.M * Cin * 2);
        const rsrc_t rw = make_rsrc(G.w, (size_t)a.Cout * ktot * 2);
        const bool active = n0 + wn * 128 < a.Cout;

        // DMA geometry, kept in few registers (this kernel's budget is tight): instruction i of a wave moves rows wv*32 + i*8 +
        // lane/8; row and source chunk of i follow from those of i = 0 — the pixel / weight row advances by 8 rows per i, and
        // the swizzle term ((r >> 1) & 7) flips bit 2 of the chunk for odd i, i.e. XORs the byte offset with 64
        uint32_t pbase0, wbase0, pvalid01 = 0, pvalid23 = 0;
        {
            const int r0 = wv * 32 + lane / C::CPR;
            const int c0 = (lane % C::CPR) ^ C::swz(r0);
            pbase0 = (uint32_t)(m0 + r0) * (uint32_t)(Cin * 2) + (uint32_t)c0 * 16u;       // rows past M are never valid: any offset does
            wbase0 = (uint32_t)(n0 + r0) * (uint32_t)(ktot * 2) + (uint32_t)c0 * 16u;     // rows past Cout lie beyond the descriptor
#pragma unroll
            for (int i = 0; i < C::IPW; i++) {
                const int m = m0 + r0 + i * C::RPI;
                uint32_t valid = 0;
                if (m < a.M) {
                    const int hw = H * W;
                    const int bimg = m / hw, rem = m - bimg * hw, y = rem / W, x = rem - y * W;
                    if (taps == 9) {
#pragma unroll
                        for (int tap = 0; tap < 9; tap++) {
                            const int yy = y + (tap / 3 - 1) * G.dil, xx = x + (tap % 3 - 1) * G.dil;
                            if (yy >= 0 && yy < H && xx >= 0 && xx < W) valid |= 1u << tap;
                        }
                    } else {
                        valid = 1u;
                    }
                }
                if (i < 2) pvalid01 |= valid << (16 * i); else pvalid23 |= valid << (16 * (i - 2));
            }
        }
        auto issue = [&](int stage, int s) {
            const int cc = s / taps, tap = s - cc * taps;
            int dy = 0, dx = 0;
            if (taps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
            const int toff = (dy * G.dil * W + dx * G.dil) * Cin * 2 + cc * 128;
            unsigned char *P = ig_lds + stage * C::STAGE + wv * (32 * C::ROW);
            unsigned char *Wt = P + kBM * C::ROW;
#pragma unroll
            for (int i = 0; i < C::IPW; i++) {
                const uint32_t bits = (i < 2 ? pvalid01 : pvalid23) >> (16 * (i & 1) + tap);
                const uint32_t off = ((pbase0 + (uint32_t)(i * C::RPI * Cin * 2)) ^ ((i & 1) ? 64u : 0u)) + (uint32_t)toff;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void *)(P + i * (C::RPI * C::ROW)), 16, (bits & 1u) ? off : kOob, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < C::IPW; i++)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void *)(Wt + i * (C::RPI * C::ROW)), 16, (i & 1) ? wbase0 ^ 64u : wbase0,
                                                         (uint32_t)s * C::ROW + (uint32_t)(i * C::RPI * ktot * 2), 0, 0);
        };

        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[i][j][r] = 0.0f;

        issue(0, sb);
        if (!active) {                                      // (two loops: see conv_igemm_body)
            for (int s = sb; s < se; s++) {
                wait_vm_barrier<0>();
                if (s + 1 < se) issue(((s - sb) & 1) ^ 1, s + 1);
            }
        } else {
            for (int s = sb; s < se; s++) {
                const int stage = (s - sb) & 1;
                wait_vm_barrier<0>();
                const bool more = s + 1 < se, late = wv >= 4;
                if (more && !late) issue(stage ^ 1, s + 1);
                igemm_mma_step(ig_lds + stage * C::STAGE + wm * (64 * C::ROW), ig_lds + stage * C::STAGE + kBM * C::ROW + wn * (128 * C::ROW), fr, acc,
                               more && late, [&]() { issue(stage ^ 1, s + 1); });
            }
        }
        __syncthreads();                                    // every wave is done reading the last stage

        if (sb != 0) {
            // ---- my first segment continues a tile an earlier workgroup starts: publish the accumulators (write-through), flag
            if (active) {
#pragma unroll
                for (int i = 0; i < 8; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        f32x4v v = {__float_as_uint(acc[i][j][0]), __float_as_uint(acc[i][j][1]), __float_as_uint(acc[i][j][2]), __float_as_uint(acc[i][j][3])};
                        __builtin_amdgcn_raw_buffer_store_b128(v, rws, (uint32_t)((i * 4 + j) * 512 + tid) * 16u,
                                                               (uint32_t)unit * (32u * 512u * 16u), 16);      // aux 16 = sc1
                    }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // every storing wave drains
            __syncthreads();
            if (tid == 0) __hip_atomic_store(k.flags + unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            bool ok = true;
            int nparts = 0;
            if (se != nsteps) {
                // ---- I hold the tile's first steps: the rest are the first segments of the following workgroups.  Wait for
                // their flags (one lane, relaxed polls, bounded), ONE acquire, barrier; the epilogue below then adds their
                // accumulators group by group, in workgroup order.
                const long long tile_end = (long long)(tile + 1) * nsteps;
                while (unit + 1 + nparts < k.units && unit_start(unit + 1 + nparts) < tile_end) nparts++;
                volatile int &sk_ok = *reinterpret_cast<volatile int *>(ig_lds);     // the stages are idle here (one LDS object only)
                if (tid == 0) {
                    int good = nparts <= kSkParts ? 1 : 0;          // (the launcher's rule makes more impossible; never drop a share silently)
                    for (int p = 0; p < nparts && good; p++) {
                        unsigned spins = 0;
                        while (__hip_atomic_load(k.flags + unit + 1 + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1u) {
                            __builtin_amdgcn_s_sleep(8);
                            if (++spins > (1u << 24)) { good = 0; break; }           // ~ seconds: give up, report
                        }
                    }
                    if (good) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    else __hip_atomic_store(k.flags + k.units, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sk_ok = good;
                }
                __syncthreads();
                ok = sk_ok != 0;
                __syncthreads();                              // the flag word is an epilogue row again
            }
            if (active) {
                // (a share that never arrived within the bounded wait — error word set — poisons the tile: every value gets a NaN
                // added, so the step's loss is NaN instead of stale memory feeding the next layer silently)
                const float poison = ok ? 0.0f : __builtin_nanf("");
                // ---- epilogue of the complete tile (as conv_igemm_body), the other workgroups' shares of a cut tile added group
                // by group in workgroup order: the up to kSkParts 16-byte loads of group gi + 1 are in flight while group gi is
                // finished (a share beyond nparts gets an out-of-range offset = zeros, so the code has no branch per share)
                unsigned char *O = ig_lds + wv * kOutWave;
                const int nw = n0 + wn * 128;
                const rsrc_t rb = make_rsrc(G.bias, G.bias ? (size_t)a.Cout * 4 : 0);
                const uint32_t seed_g = a.seed_lo + (uint32_t)grp * 0x9E3779B9u;
                f32x4v shares[2][kSkParts];
                float bq[2][4];
                auto fetch = [&](int gi, f32x4v (&dst)[kSkParts], float (&bias4)[4]) {
                    const int i = gi >> 2;                  // group gi = accumulator block (i, j) = (gi >> 2, gi & 3), as published above
                    const uint32_t off = (uint32_t)(gi * 512 + tid) * 16u;
#pragma unroll
                    for (int p = 0; p < kSkParts; p++)
                        dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rws, p < nparts ? off : kOob, (uint32_t)(unit + 1 + p) * (32u * 512u * 16u), 0);
#pragma unroll
                    for (int e = 0; e < 4; e++) bias4[e] = ld_f32(rb, (uint32_t)(nw + i * 16 + g4 * 4 + e) * 4u);
                };
                fetch(0, shares[0], bq[0]);
#pragma unroll
                for (int gi = 0; gi < 32; gi++) {
                    const int i = gi >> 2, j = gi & 3;
                    if (gi + 1 < 32) fetch(gi + 1, shares[(gi + 1) & 1], bq[(gi + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    const int nl = i * 16 + g4 * 4;
                    float s0 = acc[i][j][0], s1 = acc[i][j][1], s2 = acc[i][j][2], s3 = acc[i][j][3];
#pragma unroll
                    for (int p = 0; p < kSkParts; p++) {
                        const f32x4v pv = shares[gi & 1][p];
                        s0 += __uint_as_float(pv[0]); s1 += __uint_as_float(pv[1]); s2 += __uint_as_float(pv[2]); s3 += __uint_as_float(pv[3]);
                    }
                    float v0 = s0 + bq[gi & 1][0], v1 = s1 + bq[gi & 1][1], v2 = s2 + bq[gi & 1][2], v3 = s3 + bq[gi & 1][3];
                    v0 = fmaxf(v0, floor_) + poison; v1 = fmaxf(v1, floor_) + poison; v2 = fmaxf(v2, floor_) + poison; v3 = fmaxf(v3, floor_) + poison;
                    if (a.drop_thresh) {
                        const uint32_t m = (uint32_t)(m0 + wm * 64 + j * 16 + l15);
                        const uint32_t h = dropout_bytes((m * (uint32_t)a.Cout + (uint32_t)(nw + nl)) >> 2, seed_g, a.seed_hi);
                        v0 = (h & 0xffu) >= a.drop_thresh ? v0 * a.drop_scale : 0.0f;
                        v1 = ((h >> 8) & 0xffu) >= a.drop_thresh ? v1 * a.drop_scale : 0.0f;
                        v2 = ((h >> 16) & 0xffu) >= a.drop_thresh ? v2 * a.drop_scale : 0.0f;
                        v3 = (h >> 24) >= a.drop_thresh ? v3 * a.drop_scale : 0.0f;
                    }
                    *reinterpret_cast<uint2 *>(O + (j * 16 + l15) * kOutRow + nl * 2) = make_uint2(pack2(v0, v1), pack2(v2, v3));
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll 4
                for (int it = 0; it < 16; it++) {
                    const int p = it * 4 + (lane >> 4), ch = lane & 15;
                    const int m = m0 + wm * 64 + p;
                    const uint4 v = *reinterpret_cast<const uint4 *>(O + p * kOutRow + ch * 16);
                    if (m < a.M) *reinterpret_cast<uint4 *>(G.y + (size_t)m * a.Cout + nw + ch * 8) = v;
                }
            }
        }
        g += se - sb;
        __syncthreads();                                    // the epilogue's LDS rows are the next segment's stages
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Weight gradient of the same convolutions, again without an im2col matrix:
//
//   gw[n][tap][c] = sum over pixels m of  g[m][n] * x[pixel(m) + tap offset][c]
//
// A GEMM whose reduction runs over the pixels — the SLOW axis of both NHWC operands — so both MFMA operands are formed by
// gfx950's transposing LDS read (ds_read_b64_tr_b16: a 16-lane group reads a [4 pixels][16 channels] block and each lane
// receives one channel's four pixels), exactly as the direct kernels' weight gradient does (conv_direct.hip), but with the
// tiles DMA'd global -> LDS as in the forward kernel above:
//   * output tile 256 channels of g x 256 columns (one tap, 256 channels of x), K-step = 64 pixels: two tiles of 64 rows x
//     512 bytes per step; a DMA wave instruction moves 2 rows; the 64-byte piece (32 channels) p of row r is stored at piece
//     position p ^ (r & 3) so that the four pixel rows of a transposing read hit four different bank quarters;
//   * the x rows are the g rows' pixels shifted by the tile's tap (zero outside the map, per lane, by the descriptor's range
//     check); (row, column) of a lane's pixels advance incrementally by 64 pixels per step — no division in the loop;
//   * 9 * cin * cout / 65536 tiles are far fewer than CUs, so the pixel range of a tile is split over several workgroups
//     (chosen by the launcher to fill whole rounds of the chip); each writes its fp32 partial tile, and a second kernel sums
//     the partials in a fixed order (deterministic) into the gradient, laid out [n][tap][c] = a channels_last (cout, cin, k, k)
//     tensor, in fp32 (the master weights' gradient needs no further cast) or bf16.
//   * the number of splits is one `ksplit` for the whole launch — or, for a launch of dilated 3x3 kernels in the compact pixel
//     order, a property of the (group, tap): a tile's reduction length is the number of pixels its tap reaches (16 images of
//     41 x 41: 421 K-steps for a centre tap, 73 for a corner tap of dilation 24), so a uniform split leaves workgroups of 18 to
//     105 steps and writes four partial copies of a gradient of which many hold a handful of steps.  Such a launch takes a
//     WORK LIST (`plan`, built by the host once per geometry: build_wgrad_plan, igemm_plan.h) in device memory:
//       plan[2 (9 grp + tap)], plan[.. + 1] = the tap's split count (0: its rectangle is empty) and the index of its first partial
//                                             plane (planes of Cout x Cin floats, counted from g[0].part);
//       plan[72 + e]                        = entry e: grp | tap << 2 | split << 6 | split count << 14, longest entry first.
//     Entry e belongs to XCD e % 8; an XCD's blocks run through its entries in order, the tiles_n x (Cin / 256) tiles of an entry
//     (same rows of g and x) side by side.  Splits of one tap still take equal shares of its live pixels.
struct WgradGroup {
    const uint16_t *x;      // (B, H, W, Cin) bf16: the layer's input
    const uint16_t *g;      // (B, H, W, Cout) bf16: gradient of its output
    float *part;            // (ksplit, Cout, taps, Cin) f32 partials — with a work list: the planes (Cout, Cin) of all groups, the same pointer in every group
    int dil, pad_;
};
struct IgemmWgradArgs {
    WgradGroup g[4];
    int ngroups, B, H, W, Cin, Cout, taps, M, tiles_n, tiles_c, ksplit, kchunk, tiles_per_group;
    int stagger;            // as IgemmArgs::stagger
    int compact;            // 1: a tile sums over the pixels its tap reaches only (see the kernel); every split takes an equal share of THEM
    int xcd_mix;            // 1: XCD-interleaved map of the (group, pixel chunk, tile) workgroups (see the kernel); needs 8 | ksplit
    int skip_rows;          // 1: a K-step (64 pixels) whose rows the tile's tap shifts out of the map entirely is not loaded and
                            // not multiplied (its x rows would all be padding zeros)
    int nent;               // entries of the work list
    const uint32_t *plan;   // nullptr: `ksplit` splits for every tile; else the work list (needs compact, taps = 9, Cin != 128)
};
constexpr int kWRow = 512;                                 // bytes per LDS row: 256 channels
constexpr int kWTile = 64 * kWRow;                         // 64 pixels
constexpr int kWStage = 2 * kWTile;
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4v;
typedef __attribute__((address_space(3))) unsigned char lds_u8;

__device__ __forceinline__ bf16x8 tr_frag8(lds_u8 *p) {    // pixels 0-3 and 4-7 of a lane's k-range: two transposing reads
    bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(reinterpret_cast<__attribute__((address_space(3))) bf16x4v *>(p));
    bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(reinterpret_cast<__attribute__((address_space(3))) bf16x4v *>(p + 4 * kWRow));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ void conv_igemm_wgrad_body(const IgemmWgradArgs &a, const int bid, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ig_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kgrp = lane >> 5, i16 = lane & 15, gq = lane >> 4;
    const int wn = wv >> 2, wm = wv & 3;

    // all tiles of one pixel chunk are neighbours in t (they read the same rows of g and x): they share an XCD's L2.
    // xcd_mix (launches that skip rows; 8 | ksplit): workgroups no longer cost the same (a dilation-24 tile skips 37 % of its
    // steps, a dilation-6 one 7 %) and an XCD only runs the blocks with its id % 8 — XCD x takes the pixel chunks x, x + 8, ..
    // of EVERY group and tile (order: group, chunk, tile), which keeps a chunk's tiles on one XCD and gives all XCDs the same mix.
    const int tiles = a.tiles_n * a.tiles_c;
    int grp, split, t, ksp = a.ksplit;
    size_t plane = 0;                                       // work list: the tile's partial plane
    if (a.plan) {
        const int ncb_ = (a.Cin + 255) >> 8, tpe = a.tiles_n * ncb_;
        const int xcd = bid & 7, k = bid >> 3, pos = k / tpe, te = k - pos * tpe, e = pos * 8 + xcd;
        if (e >= a.nent) return;                            // (the grid is whole rows of 8 entries; workgroup-uniform)
        const uint32_t w = a.plan[kPlanHdr + e];
        grp = (int)(w & 3u);
        const int ptap = (int)((w >> 2) & 15u), tn_ = te / ncb_;
        split = (int)((w >> 6) & 255u);
        ksp = (int)((w >> 14) & 255u);
        t = tn_ * a.tiles_c + ptap * ncb_ + (te - tn_ * ncb_);
        plane = (size_t)a.plan[2 * (grp * 9 + ptap) + 1] + (size_t)split;
    } else if (a.xcd_mix) {
        const int id = bid, xcd = id & 7, k = id >> 3;
        if (a.ksplit >= 8) {                                // 8 | ksplit: XCD x owns the chunks x, x + 8, ..
            const int per_group = (a.ksplit >> 3) * tiles;
            grp = k / per_group;
            const int r = k - grp * per_group, sl = r / tiles;
            t = r - sl * tiles;
            split = xcd + 8 * sl;
        } else {                                            // ksplit | 8: a chunk belongs to 8 / ksplit XCDs, its tiles dealt out among them in turn
            const int xpc = 8 / a.ksplit, sub = xcd % xpc, per_group = tiles / xpc;      // (xpc | tiles: the launcher checked)
            split = xcd / xpc;
            grp = k / per_group;
            t = sub + xpc * (k - grp * per_group);
        }
    } else {
        const int total = nblk, id = bid;
        const int q = total >> 3, r = total & 7, xcd = id & 7, k = id >> 3;
        t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
        grp = t / a.tiles_per_group;
        t -= grp * a.tiles_per_group;
        split = t / tiles;
        t -= split * tiles;
    }
    const int tn = t / a.tiles_c, tc = t - tn * a.tiles_c;
    const WgradGroup G = a.g[grp];
    const int taps = a.taps, Cin = a.Cin, Cout = a.Cout, W = a.W, H = a.H;
    // the 256 columns of a tile: one tap x 256 channels of x — or, for a 128-channel x (conv3_1), two taps x 128 channels
    const bool two = Cin == 128 && taps == 9;
    const int ncb = two ? 1 : (Cin + 255) >> 8;             // 256-channel blocks of x per tap (the last one may be narrower)
    const int tap = two ? 2 * tc : tc / ncb, c0 = two ? 0 : (tc - tap * ncb) << 8, n0 = tn << 8;
    // ---- the pixels this tile sums over.  The reduction index q runs over the pixels of a RECTANGLE of every image, image-major,
    // raster order inside: the whole map — or (compact: dilated kernels) exactly the pixels whose tap lands inside the map: a tap of
    // dilation 24 on a 41 x 41 map reaches 17 x 17 (corner tap) or 17 x 41 (edge tap) pixels, everything else would multiply padding
    // zeros.  The K loop then holds no dead element at all (36 % of the four fc6_k's pixel x tap pairs are dead; skipping whole
    // 64-pixel steps of the flat order catches 22 %), and the terms that remain are summed in the order they had before.  Every
    // 3x3 layer takes this form: with dilation 1 / 2 the rectangle only loses the one or two border rows and columns (2-10 % of
    // the pixels), and every split of a tile gets an equal share of the LIVE pixels.
    const int tdy = (taps == 9 && !two) ? (tap / 3 - 1) * G.dil : 0, tdx = (taps == 9 && !two) ? (tap % 3 - 1) * G.dil : 0;
    const bool compact = a.compact && !two && taps == 9;
    const int ry0 = compact ? max(0, -tdy) : 0, rx0 = compact ? max(0, -tdx) : 0;
    const int rh_ = compact ? H - abs(tdy) : H, rw_ = compact ? W - abs(tdx) : W;
    const int rh = max(rh_, 1), rw = max(rw_, 1);                         // (an empty rectangle: no steps at all, see Kc)
    const int area = rh * rw;
    const int Kc = (rh_ > 0 && rw_ > 0) ? a.B * area : 0;
    const int kchunk = compact ? (((Kc + ksp - 1) / ksp + 63) >> 6) << 6 : a.kchunk;
    const int mbeg = split * kchunk, mend = min(Kc, mbeg + kchunk);      // [mbeg, mend) of the reduction index
    const int nsteps = mend > mbeg ? (mend - mbeg + 63) >> 6 : 0;

    const rsrc_t rx = make_rsrc(G.x, (size_t)a.M * Cin * 2);
    const rsrc_t rg = make_rsrc(G.g, (size_t)a.M * Cout * 2);

    // ---- DMA geometry: per step a wave moves rows [wv*8 + i*2, +2) of both tiles, i = 0..3; lane -> (row, 16-byte piece)
    int pm[4], pb[4], py[4], px[4], ldy[4], ldx[4], ltapoff[4];       // reduction index, image, row and column inside the rectangle
    uint32_t srcoff[4], xsrcoff[4];                         // byte offset of the lane's source piece inside a row of g / of x
    bool ltap[4];                                           // the lane's tap exists (a two-tap tile may hold the tenth)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = wv * 8 + i * 2 + (lane >> 5);
        const int q = lane & 31, p = (q >> 2) ^ (r & 3);    // 64-byte source piece that lands at piece position q >> 2
        srcoff[i] = (uint32_t)(p * 64 + (q & 3) * 16);
        const int mytap = two ? tap + (p >> 2) : tap;       // pieces 4-7 of a two-tap tile belong to the second tap
        xsrcoff[i] = two ? (uint32_t)((p & 3) * 64 + (q & 3) * 16) : srcoff[i];
        // channel counts that are no multiple of 256 (ResNet res2 / res3: 64, 128): the pieces of a 512-byte tile row past the tensor's
        // own row must read zeros — bit 31 of the piece offset pushes the lane's address beyond the descriptor (both tensors < 2^31 bytes)
        if (!two && (uint32_t)(c0 * 2) + xsrcoff[i] >= (uint32_t)(Cin * 2)) xsrcoff[i] |= 0x80000000u;
        if ((uint32_t)(n0 * 2) + srcoff[i] >= (uint32_t)(Cout * 2)) srcoff[i] |= 0x80000000u;
        ltap[i] = mytap < taps;
        ldy[i] = taps == 9 ? (mytap / 3 - 1) * G.dil : 0;
        ldx[i] = taps == 9 ? (mytap % 3 - 1) * G.dil : 0;
        ltapoff[i] = (ldy[i] * W + ldx[i]) * Cin * 2 + c0 * 2;
        const int m = mbeg + r;
        pm[i] = m;
        const int mm = m < Kc ? m : 0;
        pb[i] = mm / area;
        const int rem = mm - pb[i] * area;
        py[i] = rem / rw;
        px[i] = rem - py[i] * rw;
    }
    const int qW = 64 / rw, rW = 64 - qW * rw;              // a step advances every row by 64 elements of the reduction index

    auto advance = [&]() {                                   // the lanes' pixels move on by one step
#pragma unroll
        for (int i = 0; i < 4; i++) {
            pm[i] += 64;
            px[i] += rW;
            py[i] += qW;
            if (px[i] >= rw) { px[i] -= rw; py[i] += 1; }
            while (py[i] >= rh) { py[i] -= rh; pb[i] += 1; }
        }
    };
    auto issue = [&](int stage) {
        unsigned char *A = ig_lds + stage * kWStage + wv * (8 * kWRow);
        unsigned char *Bt = A + kWTile;
        int pix[4];
#pragma unroll
        for (int i = 0; i < 4; i++) pix[i] = compact ? (pb[i] * H + ry0 + py[i]) * W + rx0 + px[i] : pm[i];       // the pixel of the map
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool live = pm[i] < mend;
            const uint32_t vo = live ? (uint32_t)pix[i] * (uint32_t)(Cout * 2) + (uint32_t)(n0 * 2) + srcoff[i] : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (lds_void *)(A + i * (2 * kWRow)), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int yy = ry0 + py[i] + ldy[i], xx = rx0 + px[i] + ldx[i];
            const bool live = ltap[i] && pm[i] < mend && yy >= 0 && yy < H && xx >= 0 && xx < W;
            const uint32_t vo = live ? (uint32_t)(pix[i] * (Cin * 2) + ltapoff[i]) + xsrcoff[i] : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void *)(Bt + i * (2 * kWRow)), 16, vo, 0, 0, 0);
        }
        advance();                                           // the next step's pixels
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    // the address a lane supplies to a transposing read of fragment f (32 channels = one 64-byte piece), k-slice ks: pixel row
    // ks*16 + kgrp*8 + i16/4 (the second read 4 rows further), piece f ^ (row & 3), channels (gq & 1)*16 + 4 (i16 & 3) .. + 3
    const int swz = (i16 >> 2) & 3;
    const uint32_t lane_off = (uint32_t)((kgrp * 8 + (i16 >> 2)) * kWRow + (gq & 1) * 32 + (i16 & 3) * 8);
    uint32_t aoff[4], boff[2];
#pragma unroll
    for (int i = 0; i < 4; i++) aoff[i] = lane_off + (uint32_t)(((wn * 4 + i) ^ swz) * 64);
#pragma unroll
    for (int j = 0; j < 2; j++) boff[j] = lane_off + (uint32_t)(kWTile + ((wm * 2 + j) ^ swz) * 64);
    lds_u8 *lds = (lds_u8 *)ig_lds;

    // ---- the K-steps this tile multiplies.  A dilated tap shifts whole rows of the map into the padding: with dilation 24 on 41
    // rows the three upper taps see x only from rows >= 24 — for the 64-pixel steps that lie in rows 0..23 of an image every
    // x row is zero and the step adds exact zeros (22 % of the four fc6_k's steps at 16 images, 37 % for dilation 24).  Such
    // steps are skipped: the lanes' pixel counters run on, nothing is loaded, nothing multiplied; the partial sums are
    // bit-identical.  Decided per step from the rows its first and last pixel lie in (wave-uniform, scalar): a step inside one
    // image is dead when no row in [y_first, y_last] lands in [0, H) after the shift; a step that crosses into the next image
    // always holds live rows of one of the two (|shift| < H), and so does any tile without a vertical shift.
    // (a step of 64 pixels spans at least 64 / W rows: below that shift no step can be dead, and the test is not free)
    const bool may_skip = a.skip_rows && !compact && abs(tdy) * W >= 64 && tdy > -H && tdy < H;
    const int hw_ = H * W;
    auto step_dead = [&](int st) -> bool {
        const int p0 = mbeg + st * 64, p1 = min(p0 + 63, mend - 1);
        const int b0 = p0 / hw_, b1 = p1 / hw_;
        if (b0 != b1) return false;
        const int y0 = (p0 - b0 * hw_) / W, y1 = (p1 - b0 * hw_) / W;
        return y1 + tdy < 0 || y0 + tdy >= H;
    };
    int cur = 0;                                             // the step the lanes' counters stand at = the next one to issue
    auto seek = [&]() {
        if (may_skip)
            while (cur < nsteps && step_dead(cur)) { advance(); cur++; }
    };
    seek();
    bool have = cur < nsteps;
    if (have) { issue(0); cur++; }
    for (int s = 0; have; s++) {
        wait_vm_barrier<0>();
        seek();
        const bool more = cur < nsteps, late = a.stagger && wv >= 4;
        if (more && !late) { issue((s + 1) & 1); cur++; }
        lds_u8 *st = lds + (s & 1) * kWStage;
        bf16x8 af[2][4], bfr[2][2];
#pragma unroll
        for (int i = 0; i < 4; i++) af[0][i] = tr_frag8(st + aoff[i]);
#pragma unroll
        for (int j = 0; j < 2; j++) bfr[0][j] = tr_frag8(st + boff[j]);
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            if (ks + 1 < 4) {
#pragma unroll
                for (int i = 0; i < 4; i++) af[(ks + 1) & 1][i] = tr_frag8(st + (ks + 1) * (16 * kWRow) + aoff[i]);
#pragma unroll
                for (int j = 0; j < 2; j++) bfr[(ks + 1) & 1][j] = tr_frag8(st + (ks + 1) * (16 * kWRow) + boff[j]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks & 1][i], bfr[ks & 1][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks == 0 && more && late) { issue((s + 1) & 1); cur++; }
        }
        have = more;
    }
    // C[row = channel of g][col = channel of x]: lane holds column l31, rows (reg & 3) + 8 (reg >> 2) + 4 kgrp
    // (work list: the tile's own plane [n][c]; else split `split` of the whole gradient [n][tap][c])
    float *pp = a.plan ? G.part + plane * ((size_t)Cout * Cin) : G.part + (size_t)split * ((size_t)Cout * taps * Cin);
    const size_t prow = a.plan ? (size_t)Cin : (size_t)taps * Cin;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int col = wm * 64 + j * 32 + l31;
            const int etap = two ? tap + (col >> 7) : tap, c = two ? (col & 127) : c0 + col;
            if (etap < taps && c < Cin && n0 + wn * 128 + i * 32 < Cout) {      // (32-row / 32-column blocks: channel counts are multiples of 64)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + wn * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kgrp;
                    pp[(size_t)n * prow + (a.plan ? 0 : etap * Cin) + c] = acc[i][j][r];
                }
            }
        }
}

__global__ __launch_bounds__(512, 2) void conv_igemm_wgrad_kernel(IgemmWgradArgs a) { conv_igemm_wgrad_body(a, (int)blockIdx.x, (int)gridDim.x); }

// One launch for the whole backward of a layer's convolution: both gradients need nothing but the (masked) output gradient, and a
// 41x41 layer's data gradient is 212 tiles for 256 CUs — one round with a sixth of the chip idle — while its weight gradient is
// 252 workgroups.  Blocks [0, nd) are the data gradient's tiles, blocks [nd_pad, nd_pad + nw) the weight gradient's workgroups
// (nd_pad = nd rounded up to a multiple of 8, so that both halves keep their block-id -> XCD relation; the padding blocks exit):
// the dispatcher hands the weight gradient's first workgroups to the CUs the data gradient leaves idle, no stream, no join.
// (The two kernels on two streams lost: 1 761 -> 1 715 images/s, profiles/r05_wgrad_side_stream_ab.txt.)
struct IgemmBwdArgs {
    IgemmArgs d;
    IgemmWgradArgs w;
    int nd, nd_pad, nw;
    int w_first, nw_pad;    // 1: the weight gradient's workgroups take the first block ids (they are dispatched first): the order for a layer
                            // whose weight-gradient workgroups run longer than its data-gradient tiles (a 1x1 layer: tiles of 4 - 16 K-steps)
};
__global__ __launch_bounds__(512, 2) void conv_igemm_bwd_kernel(IgemmBwdArgs a) {
    const int id = (int)blockIdx.x;
    if (a.w_first) {
        if (id < a.nw_pad) {
            if (id < a.nw) conv_igemm_wgrad_body(a.w, id, a.nw);
        } else if (id - a.nw_pad < a.nd) {
            conv_igemm_body(a.d, id - a.nw_pad, a.nd);
        }
        return;
    }
    if (id < a.nd_pad) {
        if (id < a.nd) conv_igemm_body(a.d, id, a.nd);
    } else {
        conv_igemm_wgrad_body(a.w, id - a.nd_pad, a.nw);
    }
}

// gw[e] = sum over the splits of part[s][e], e over [n][tap][c], in split order; float4 per thread; blockIdx.y = the group
// (the four branches of a grouped launch share ONE reduction launch: 17 -> 11 reduction launches per train step).
// With a work list (IgemmWgradArgs::plan) the element's own tap says how many partials there are and where: plan[2 (9 grp + tap)]
// planes of (Cout, Cin) floats from plane plan[.. + 1] on, summed in split order; a tap without a split (its rectangle is
// empty: no workgroup ran) gets exact zeros.
struct WgradReduceArgs {
    const float *part[4];
    void *gw[4];
    int ksplit;
    int cin4;               // work list: float4s per (output channel, tap) = Cin / 4
    const uint32_t *plan;   // nullptr, or the work list's table
    size_t plane4;          // work list: float4s per partial plane = Cout * Cin / 4
    size_t n4;
    const float *scale;     // nullptr, or (cout) f32: output channel o's gradient times scale[o] (a constant per-channel factor folded into
    size_t per_o4;          // the kernel the convolution ran with: d/dw = scale * d/d(w scale)); per_o4 = float4s per output channel
};
template <bool BF16_OUT>
__global__ __launch_bounds__(256) void conv_igemm_wgrad_reduce_kernel(WgradReduceArgs a) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n4) return;
    const float4 *p = reinterpret_cast<const float4 *>(a.part[blockIdx.y]) + e;
    void *gw = a.gw[blockIdx.y];
    int ksplit = a.ksplit;
    size_t stride = a.n4;
    if (a.plan) {
        const size_t n = e / a.per_o4, rem = e - n * a.per_o4;
        const int tap = (int)(rem / (size_t)a.cin4), c4 = (int)(rem - (size_t)tap * a.cin4);
        const uint32_t *row = a.plan + 2 * ((int)blockIdx.y * 9 + tap);
        ksplit = (int)row[0];
        stride = a.plane4;
        p = reinterpret_cast<const float4 *>(a.part[0]) + (size_t)row[1] * a.plane4 + n * (size_t)a.cin4 + c4;
    }
    float4 s = ksplit > 0 ? p[0] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int k = 1;
    for (; k + 8 <= ksplit; k += 8) {                        // eight loads in flight, added in split order (the sum's bits do not change)
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; u++) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; k < ksplit; k++) {
        const float4 v = p[(size_t)k * stride];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (a.scale) {
        const float f = a.scale[e / a.per_o4];
        s.x *= f; s.y *= f; s.z *= f; s.w *= f;
    }
    if (BF16_OUT) reinterpret_cast<uint2 *>(gw)[e] = make_uint2(pack2(s.x, s.y), pack2(s.z, s.w));
    else reinterpret_cast<float4 *>(gw)[e] = s;
}


// ------------------------------------------------------------------------------------------------------------------
// Both packed forms of a kernel in one pass over the float32 master weights ([o][tap][c] = a channels_last (cout, cin, k, k)
// parameter): the forward form fwd[o][c / 64][tap][64] and the data-gradient form dg[c][o / 64][T - tap][64] (the kernel
// flipped, T = k*k - 1, and its channel axes swapped), both bf16.  One block per (64 outputs, 64 inputs, tap): the forward
// form is the tile as it is read; the data-gradient form is its transpose, taken through LDS.
// plain = 1: the layouts of the direct kernels (conv_direct.hip) instead — fwd[o][tap][c] (the parameter's own order, cast) and
// dg[c][T - tap][o] (a channels_last (cin, cout, k, k) tensor: the kernel flipped, channel axes swapped).
__global__ __launch_bounds__(256) void pack_conv_weight_kernel(const float *w, uint16_t *fwd, uint16_t *dg, int cout, int cin, int taps,
                                                               int plain, const float *scale) {      // scale: nullptr or (cout) — w[o] * scale[o] is packed
    __shared__ uint16_t tile[64][64 + 4];
    const int ob = blockIdx.x, cb = blockIdx.y, tap = blockIdx.z, t = threadIdx.x;
    const int r = t >> 4, q = t & 15;                        // 16 rows x 16 float4 per pass
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int o = r + 16 * i;
        const size_t src = ((size_t)(ob * 64 + o) * taps + tap) * cin + cb * 64 + q * 4;
        float4 v = *reinterpret_cast<const float4 *>(w + src);
        if (scale) {
            const float f = scale[ob * 64 + o];
            v.x *= f; v.y *= f; v.z *= f; v.w *= f;
        }
        const uint2 pk = make_uint2(pack2(v.x, v.y), pack2(v.z, v.w));
        if (fwd) *reinterpret_cast<uint2 *>(fwd + (plain ? src : (((size_t)(ob * 64 + o) * (cin >> 6) + cb) * taps + tap) * 64 + q * 4)) = pk;
        *reinterpret_cast<uint2 *>(&tile[o][q * 4]) = pk;
    }
    if (!dg) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c = r + 16 * i;                            // row of the transposed tile; q*4 .. q*4+3 = its outputs
        const uint32_t lo = (uint32_t)tile[q * 4 + 0][c] | ((uint32_t)tile[q * 4 + 1][c] << 16);
        const uint32_t hi = (uint32_t)tile[q * 4 + 2][c] | ((uint32_t)tile[q * 4 + 3][c] << 16);
        const size_t dst = plain ? ((size_t)(cb * 64 + c) * taps + (taps - 1 - tap)) * cout + ob * 64 + q * 4
                                 : (((size_t)(cb * 64 + c) * (cout >> 6) + ob) * taps + (taps - 1 - tap)) * 64 + q * 4;
        *reinterpret_cast<uint2 *>(dg + dst) = make_uint2(lo, hi);
    }
}

}  // namespace

bool conv_igemm_supported(int cin, int cout, int k) {
    return (k == 1 || k == 3) && cin >= 64 && cin % 64 == 0 && cout >= 128 && cout % 128 == 0;
}

std::atomic<int> g_igemm_variant{-1};      // dsrg_debug_set_igemm_variant (tests / tools); -1 = the default, 3
// read ONCE per public launch; the decoded struct is handed down (igemm_plan.h)
static IgemmVariant igemm_variant() { return decode_igemm_variant(g_igemm_variant.load(std::memory_order_relaxed)); }

static int igemm_cus() {
    static const int n = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 8) c = 256;
        return c;
    }();
    return n;
}
// device scratch of the stream-K form: one accumulator tile (256 KB) and one flag per workgroup (= per CU), an error word
size_t conv_igemm_workspace() { return (size_t)igemm_cus() * (32 * 512 * 16) + ((size_t)igemm_cus() + 1 + 63) / 64 * 256; }

// bias gradient from the per-tile column sums of a masked data gradient: fixed order (sixteen interleaved row streams, then
// a tree), one workgroup per 64 channels of a group
struct ColsumArgs {
    const float *part[4];
    float *out[4];
    int rows, cout;
};
__global__ __launch_bounds__(1024) void igemm_colsum_kernel(ColsumArgs a) {
    __shared__ float red[16][64];
    colsum_block(a.part[blockIdx.y], a.out[blockIdx.y], a.rows, a.cout, (int)blockIdx.x, red);
}

int launch_igemm_colsum(const float *const *parts, float *const *outs, int ngroups, int rows, int cout, hipStream_t stream) {
    if (ngroups < 1 || ngroups > 4 || cout % 64 || rows < 1) return set_error(DSRG_ERR_INVALID, "column sums: 1..4 groups, 64 | channels");
    if (defer_reduction(0, ngroups, parts, outs, rows, cout)) return DSRG_OK;      // all groups recorded; else none: sum now
    ColsumArgs c;
    memset(&c, 0, sizeof(c));
    for (int g = 0; g < ngroups; g++) { c.part[g] = parts[g]; c.out[g] = outs[g]; }
    c.rows = rows; c.cout = cout;
    hipLaunchKernelGGL(igemm_colsum_kernel, dim3(cout / 64, ngroups), dim3(1024), 0, stream, c);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

size_t conv_igemm_colsum_workspace(int ngroups, int B, int H, int W, int cout) {
    return (size_t)ngroups * conv_igemm_pixel_tiles(B, H, W) * (size_t)cout * sizeof(float);
}

// ---- forward / data gradient: prepare_igemm validates and decides, run_igemm launches what was prepared
namespace {
struct IgemmLaunch {
    IgemmSkArgs sk;         // sk.base: the argument block of either form; the rest is filled when stream_k
    int grid;
    bool stream_k;          // conv_igemm_sk_kernel instead of conv_igemm_kernel_64x2
};

// The request's fields: IgemmRequest (common.h).  Launches nothing, enqueues nothing
int prepare_igemm(const IgemmRequest &r, const IgemmVariant &v, IgemmLaunch &L) {
    const int ngroups = r.ngroups, B = r.s.B, H = r.s.H, W = r.s.W, cin = r.s.cin, cout = r.s.cout, k = r.s.k, split_cin = r.split_cin;
    const float drop_p = r.drop_p;
    if (ngroups < 1 || ngroups > 4) return set_error(DSRG_ERR_INVALID, "conv_igemm: 1..4 groups");
    if (r.colsums && (!r.colsum_ws || r.colsum_ws_bytes < conv_igemm_colsum_workspace(ngroups, B, H, W, cout)))
        return set_error(DSRG_ERR_INVALID, "conv_igemm: column-sum scratch missing or too small");
    if (!conv_igemm_launchable(cin, cout, k))
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm: cin %% 64 == 0, cout %% 128 == 0 (or cout = 64), k in (1, 3) required (got %d, %d, %d)",
                         cin, cout, k);
    const long long M = (long long)B * H * W;
    if (M <= 0 || M * cin * 2 >= 0x7fffffffLL || (long long)cout * k * k * cin * 2 >= 0x7fffffffLL || M * cout * 2 >= 0x7fffffff00LL)
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm: tensor too large for 32-bit buffer offsets");
    memset(&L, 0, sizeof(L));
    IgemmArgs &a = L.sk.base;
    for (int g = 0; g < ngroups; g++) {
        a.g[g].x = static_cast<const uint16_t *>(r.x[g]);
        a.g[g].w = static_cast<const uint16_t *>(r.w[g]);
        a.g[g].bias = r.bias[g];
        a.g[g].y = static_cast<uint16_t *>(r.y[g]);
        a.g[g].dil = r.dil[g];
        a.g[g].mask = r.masked ? static_cast<const uint16_t *>(r.mask[g]) : nullptr;
        a.g[g].colsum = r.colsums ? static_cast<float *>(r.colsum_ws) + (size_t)g * conv_igemm_pixel_tiles(B, H, W) * cout : nullptr;
        a.g[g].res = static_cast<const uint16_t *>(r.res);
        if (!a.g[g].x || !a.g[g].w || !a.g[g].y || (r.masked && !r.mask[g]) || (r.colsums && !r.colsum[g]))
            return set_error(DSRG_ERR_INVALID, "conv_igemm: null pointer");
    }
    a.out_scale = r.out_scale;
    a.xrow = cin * 2;
    if (split_cin > 0) {
        a.xrow = 3 * split_cin * 2;
        a.cpp = split_cin / 64;
        a.out_f32 = 1;
    }
    a.skip_taps = v.skip_dead_steps;
    const bool fused_bwd = r.masked || r.colsums || r.res;
    if (r.res && (r.colsums || ngroups != 1 || drop_p != 0.0f || split_cin))
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm: a residual goes with one group, no column sums, no dropout");
    a.ngroups = ngroups; a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.taps = k * k; a.relu = r.relu; a.M = (int)M;
    a.tiles_m = (int)((M + kBM - 1) / kBM);
    a.tiles_n = (cout + kBN - 1) / kBN;
    a.tiles_per_group = a.tiles_m * a.tiles_n;
    if (drop_p < 0.0f || drop_p >= 1.0f) return set_error(DSRG_ERR_INVALID, "conv_igemm: 0 <= dropout probability < 1");
    a.drop_thresh = (uint32_t)(drop_p * 256.0f + 0.5f);       // p is realised in steps of 1 / 256 (0.5 exactly)
    if (a.drop_thresh > 255) a.drop_thresh = 255;
    a.drop_scale = 256.0f / (float)(256 - (int)a.drop_thresh);
    a.seed_lo = (uint32_t)r.seed; a.seed_hi = (uint32_t)(r.seed >> 32);
    a.stagger = v.stagger;
    // stream-K only where it was measured to win (profiles/r04_igemm_stream_k.txt): a single round that fills at most 60 % of
    // the chip (conv4_1's data gradient: 106 tiles, 115 -> 88 us).  A cut tile costs its workgroups ~25 us (256 KB of
    // accumulators written through, read back, one acquire), which eats the sixth of the chip that 212 tiles leave idle (131 ->
    // 136 us), and launches of several rounds lose less to their last round than the round count suggests (workgroups of
    // different rounds overlap: fc6 x 4, 6.6 rounds, 810 us whole against 902 us dealt out).
    const int units = igemm_cus(), tiles_total = a.tiles_per_group * ngroups, nsteps = (cin / 64) * k * k;
    const bool sk_wins = tiles_total * 100 <= units * 60;
    if (r.may_stream_k && !fused_bwd && split_cin == 0 && cout % 128 == 0 && r.workspace && r.workspace_bytes >= conv_igemm_workspace() &&
        ((v.stream_k_where_it_wins && sk_wins) || v.stream_k_forced) && (long long)tiles_total * nsteps >= (long long)units * 8 &&
        tiles_total * 3 >= units) {
        L.stream_k = true; L.grid = units;
        a.stagger = 1;
        L.sk.ws = static_cast<float *>(r.workspace);
        L.sk.flags = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(r.workspace) + (size_t)units * (32 * 512 * 16));
        L.sk.units = units; L.sk.tiles_total = tiles_total;
        return DSRG_OK;
    }
    // tap skipping makes tiles unequal: spread every group's tiles over all XCDs (conv_igemm_body).  Only then: the layers
    // whose tiles all run the same steps keep the map they were tuned with (neighbouring pixel tiles share rows in one L2)
    int dils[4];
    for (int g = 0; g < ngroups; g++) {
        dils[g] = a.g[g].dil;
        if (a.skip_taps && k == 3 && dils[g] >= 3) a.xcd_mix = 1;
    }
    const bool rows_ok = a.xcd_mix && W <= kBM && conv_igemm_row_tiles(H, W);
    // the class order where it pays, or wherever it is legal when forced (a rectangle encodes coordinates below 256)
    if (a.xcd_mix && v.class_tiles_allowed && H <= 255 && W <= 255 && (class_order_pays(B, H, W, dils, ngroups, rows_ok) || v.class_tiles_forced)) {
        a.cls_tiles = 1;
        for (int g = 0; g < ngroups; g++) {
            HostClass c[kMaxClasses];
            const int n = build_classes(H, W, dils[g], c);
            long long q0 = 0;
            a.g[g].ncls = n;
            for (int i = 0; i < n; i++) {
                a.g[g].cls[i].rect = (uint32_t)c[i].y0 | (uint32_t)(c[i].y1 - c[i].y0) << 8 | (uint32_t)c[i].x0 << 16 | (uint32_t)(c[i].x1 - c[i].x0) << 24;
                a.g[g].cls[i].q0 = (int)q0;
                q0 += (long long)B * (c[i].y1 - c[i].y0) * (c[i].x1 - c[i].x0);
            }
        }
    }
    if (!a.cls_tiles && rows_ok) {
        // ... and cut them along map rows (see the kernel); tiles_m grows by the rows a band leaves empty (112 against 106 tiles
        // for sixteen 41x41 maps), which the skipped steps more than pay for
        a.row_tiles = 1;
        a.rows_per_tile = kBM / W;
        a.bands = (H + a.rows_per_tile - 1) / a.rows_per_tile;
        a.tiles_m = B * a.bands;
        a.tiles_per_group = a.tiles_m * a.tiles_n;
    }
    L.grid = a.xcd_mix ? 8 * ngroups * ((a.tiles_m + 7) / 8) * a.tiles_n : a.tiles_per_group * ngroups;
    return DSRG_OK;
}

// the column sums a data gradient's grid left per tile, summed into colsum (nullptr: it kept none)
int run_colsum(const IgemmArgs &a, float *const *colsum, hipStream_t stream) {
    if (!colsum) return DSRG_OK;
    const float *parts[4];
    for (int g = 0; g < a.ngroups; g++) parts[g] = a.g[g].colsum;
    return launch_igemm_colsum(parts, colsum, a.ngroups, a.tiles_m, a.Cout, stream);
}

// the prepared launch, then its column-sum pass
int run_igemm(const IgemmLaunch &L, float *const *colsum, hipStream_t stream) {
    static LdsGrant grant[2];
    constexpr size_t lds = ICfg<64, 2>::LDS;
    const IgemmArgs &a = L.sk.base;
    if (L.stream_k) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&conv_igemm_sk_kernel), lds, grant[1])) return rc;
        DSRG_HIP_CHECK(hipMemsetAsync(L.sk.flags, 0, sizeof(uint32_t) * ((size_t)L.sk.units + 1), stream));      // every launch (a graph replays it)
        hipLaunchKernelGGL(conv_igemm_sk_kernel, dim3(L.grid), dim3(512), lds, stream, L.sk);
        DSRG_LAUNCH_CHECK();
        return DSRG_OK;
    }
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&conv_igemm_kernel_64x2), lds, grant[0])) return rc;
    hipLaunchKernelGGL(conv_igemm_kernel_64x2, dim3(L.grid), dim3(512), lds, stream, a);
    DSRG_LAUNCH_CHECK();
    return run_colsum(a, colsum, stream);
}
}  // namespace

// A forward, a data gradient (the request's mask / colsum fields), or either with a residual in the single group's store: y =
// post(bf16(conv(x, w) + bias) + res), post = ReLU (relu) and / or zero where mask <= 0 — the forward of a residual block's last
// convolution, the data gradient of its first
int launch_conv_igemm(const IgemmRequest &r, hipStream_t stream) {
    IgemmLaunch L;
    if (int rc = prepare_igemm(r, igemm_variant(), L)) return rc;
    return run_igemm(L, r.colsums ? r.colsum : nullptr, stream);
}

// A float32 convolution on the bf16 MFMA (forward, one group; layer-level prototype of round 6): x3 = the three bf16 planes of the
// float32 activation, (B, H, W, 3 cin) with channel index plane * cin + c; w = the packed kernel over 6 cin VIRTUAL channels,
// (cout, 6 cin / 64, k k, 64), virtual chunk block q holding plane {0, 1, 0, 2, 0, 1}[q] of the split kernel; y float32 (B, H, W, cout)
int launch_conv_igemm_split(const void *x3, const void *w, const float *bias, float *y, int dil, const ConvGeom &s, int relu, hipStream_t stream) {
    if (!conv_igemm_supported(s.cin, s.cout, s.k) || (long long)s.B * s.H * s.W * 3 * s.cin * 2 >= 0x7fffffffLL)
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm_split: shape not supported");
    IgemmRequest r;
    r.x[0] = x3; r.w[0] = w; r.bias[0] = bias; r.y[0] = y; r.dil[0] = dil;
    r.s = {s.B, s.H, s.W, 6 * s.cin, s.cout, s.k};
    r.relu = relu;
    r.split_cin = s.cin;
    return launch_conv_igemm(r, stream);
}

bool conv_igemm_wgrad_supported(int cin, int cout, int k) {
    return (k == 1 || k == 3) && ((cin >= 256 && cin % 256 == 0) || (cin == 128 && k == 3)) && cout >= 256 && cout % 256 == 0;
}

size_t conv_igemm_wgrad_workspace(int ngroups, int B, int H, int W, int cin, int cout, int k) {
    return wgrad_workspace_bytes(ngroups, B, H, W, cin, cout, k);
}

int conv_igemm_wgrad_splits(int ngroups, int B, int H, int W, int cin, int cout, int k, const int *dil, int *splits) {
    if (ngroups < 1 || ngroups > 4 || !splits || !conv_igemm_wgrad_launchable(cin, cout, k) || (long long)B * H * W <= 0)
        return set_error(DSRG_ERR_INVALID, "conv_igemm_wgrad_splits: 1..4 groups of a geometry conv_igemm_wgrad takes");
    if (wgrad_wants_plan(igemm_variant(), dil, ngroups, cin, k)) {
        const WgradPlan &p = build_wgrad_plan(ngroups, B, H, W, cin, cout, dil, igemm_cus());
        for (int i = 0; i < ngroups * 9; i++) splits[i] = (int)p.words[2 * i];
        return DSRG_OK;
    }
    const int ks = wgrad_uniform_ksplit(ngroups, (long long)B * H * W, cin, cout, k, wgrad_wants_mix(dil, ngroups, k));
    for (int i = 0; i < ngroups * k * k; i++) splits[i] = ks;
    return DSRG_OK;
}

// The work list reaches its place behind the partials as kernel arguments, in front of EVERY launch that reads it: a store kernel
// in the launch's own stream (an ordinary kernel node under stream capture), kPlanChunk words per launch (fc6 x4 at batch 16: 132
// words, one launch of one workgroup).  The host keeps no record of what a workspace holds, so nothing the caller does to it
// between two calls matters.
constexpr int kPlanChunk = 960;                            // (a kernel's arguments hold 4 KB)
struct PlanChunkArgs { uint32_t *dst; int n, pad_; uint32_t w[kPlanChunk]; };
__global__ void __launch_bounds__(256) conv_igemm_wgrad_plan_kernel(const PlanChunkArgs c) {
    for (int i = threadIdx.x; i < c.n; i += 256) c.dst[i] = c.w[i];
}

// ---- weight gradient: prepare_wgrad validates and decides; upload_wgrad_plan, launch_wgrad and reduce_wgrad are the launch's steps
namespace {
struct WgradLaunch {
    IgemmWgradArgs a;
    const WgradPlan *plan;  // the work list a.plan will hold once uploaded (nullptr: a uniform split)
    int grid;
};

// The request's fields: WgradRequest (common.h); a forced split is a uniform one: such a launch takes no work list.  Launches
// nothing, enqueues nothing
int prepare_wgrad(const WgradRequest &r, const IgemmVariant &v, WgradLaunch &L) {
    const int ngroups = r.ngroups, B = r.s.B, H = r.s.H, W = r.s.W, cin = r.s.cin, cout = r.s.cout, k = r.s.k, forced_ksplit = r.forced_ksplit;
    const int *const dil = r.dil;
    void *const workspace = r.workspace;
    if (ngroups < 1 || ngroups > 4) return set_error(DSRG_ERR_INVALID, "conv_igemm_wgrad: 1..4 groups");
    if (!conv_igemm_wgrad_launchable(cin, cout, k))
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm_wgrad: cin %% 64 == 0, cout %% 64 == 0, k in (1, 3) required (got %d, %d, %d)", cin, cout, k);
    const long long M = (long long)B * H * W;
    if (M <= 0 || M * cin * 2 >= 0x7fffffffLL || M * cout * 2 >= 0x7fffffffLL)
        return set_error(DSRG_ERR_UNSUPPORTED, "conv_igemm_wgrad: tensor too large for 32-bit buffer offsets");
    const size_t need = wgrad_workspace_bytes(ngroups, B, H, W, cin, cout, k);
    if (!workspace || r.workspace_bytes < need) return set_error(DSRG_ERR_INVALID, "conv_igemm_wgrad: workspace of %zu bytes needed", need);
    memset(&L, 0, sizeof(L));
    IgemmWgradArgs &a = L.a;
    a.ngroups = ngroups; a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.taps = k * k; a.M = (int)M;
    a.tiles_n = (cout + 255) / 256;
    a.tiles_c = wgrad_col_tiles(cin, k);
    if (forced_ksplit <= 0 && wgrad_wants_plan(v, dil, ngroups, cin, k)) L.plan = &build_wgrad_plan(ngroups, B, H, W, cin, cout, dil, igemm_cus());
    a.ksplit = forced_ksplit > 0 ? forced_ksplit : wgrad_uniform_ksplit(ngroups, M, cin, cout, k, wgrad_wants_mix(dil, ngroups, k));
    a.kchunk = (int)(((M + a.ksplit - 1) / a.ksplit + 63) / 64 * 64);
    a.tiles_per_group = a.tiles_n * a.tiles_c * a.ksplit;
    a.stagger = v.stagger;
    a.skip_rows = v.skip_dead_steps;
    const size_t per_group = (size_t)a.ksplit * cout * k * k * cin;
    for (int q = 0; q < ngroups; q++) {
        a.g[q].x = static_cast<const uint16_t *>(r.x[q]);
        a.g[q].g = static_cast<const uint16_t *>(r.g[q]);
        a.g[q].part = static_cast<float *>(workspace) + (L.plan ? 0 : (size_t)q * per_group);
        a.g[q].dil = dil[q];
        if (!a.g[q].x || !a.g[q].g || !r.gw[q]) return set_error(DSRG_ERR_INVALID, "conv_igemm_wgrad: null pointer");
    }
    // (compact pixel order for every 3x3 layer, not the dilated ones only: 1 800-1 807 against 1 776-1 782 images/s)
    for (int q = 0; q < ngroups; q++) {
        if (a.skip_rows && k == 3 && a.g[q].dil >= 3 &&
            (a.ksplit % 8 == 0 || (8 % a.ksplit == 0 && (a.tiles_n * a.tiles_c) % (8 / a.ksplit) == 0))) a.xcd_mix = 1;
        if (a.skip_rows && v.wgrad_compact && k == 3 && cin != 128 && a.g[q].dil >= 1) a.compact = 1;
    }
    L.grid = a.tiles_per_group * ngroups;
    if (L.plan) {
        // the work list lies behind the partials any launch of this geometry may write
        const size_t room = wgrad_plan_room(ngroups, wgrad_ksplit_bound(ngroups, B, H, W, cin, cout, k), cin, k);
        if (L.plan->words.size() * sizeof(uint32_t) > room || (size_t)L.plan->planes * cout * cin * sizeof(float) > need - room)
            return set_error(DSRG_ERR_INVALID, "conv_igemm_wgrad: work list larger than its workspace");
        a.plan = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + (need - room));
        a.nent = L.plan->nent;
        L.grid = (a.nent + 7) / 8 * 8 * (a.tiles_n * ((cin + 255) / 256));      // whole rows of 8 entries, an entry's tiles side by side
    }
    return DSRG_OK;
}

int upload_wgrad_plan(const WgradLaunch &L, hipStream_t stream) {
    if (!L.plan) return DSRG_OK;
    for (size_t at = 0, n = L.plan->words.size(); at < n; at += kPlanChunk) {
        PlanChunkArgs c;
        c.dst = const_cast<uint32_t *>(L.a.plan) + at;
        c.n = (int)std::min<size_t>(kPlanChunk, n - at);
        c.pad_ = 0;
        memcpy(c.w, L.plan->words.data() + at, (size_t)c.n * sizeof(uint32_t));
        hipLaunchKernelGGL(conv_igemm_wgrad_plan_kernel, dim3(1), dim3(256), 0, stream, c);
        DSRG_LAUNCH_CHECK();
    }
    return DSRG_OK;
}

int launch_wgrad(const WgradLaunch &L, hipStream_t stream) {
    static LdsGrant grant;
    constexpr size_t lds = 2 * kWStage;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&conv_igemm_wgrad_kernel), lds, grant)) return rc;
    hipLaunchKernelGGL(conv_igemm_wgrad_kernel, dim3((unsigned)L.grid), dim3(512), lds, stream, L.a);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// scale: nullptr, or the per-output factor of the gradient (WgradReduceArgs::scale)
int reduce_wgrad(const IgemmWgradArgs &a, void *const *gw, const float *scale, int out_bf16, hipStream_t stream) {
    WgradReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.ksplit = a.ksplit;
    r.plan = a.plan;
    r.cin4 = a.Cin / 4;
    r.plane4 = (size_t)a.Cout * a.Cin / 4;
    r.n4 = (size_t)a.Cout * a.taps * a.Cin / 4;
    r.scale = scale;
    r.per_o4 = (size_t)a.taps * a.Cin / 4;
    for (int q = 0; q < a.ngroups; q++) { r.part[q] = a.g[q].part; r.gw[q] = gw[q]; }
    const dim3 rgrid((unsigned)((r.n4 + 255) / 256), (unsigned)a.ngroups);
    if (out_bf16) hipLaunchKernelGGL(conv_igemm_wgrad_reduce_kernel<true>, rgrid, dim3(256), 0, stream, r);
    else hipLaunchKernelGGL(conv_igemm_wgrad_reduce_kernel<false>, rgrid, dim3(256), 0, stream, r);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int run_wgrad(const WgradLaunch &L, void *const *gw, const float *scale, int out_bf16, hipStream_t stream) {
    if (int rc = upload_wgrad_plan(L, stream)) return rc;
    if (int rc = launch_wgrad(L, stream)) return rc;
    return reduce_wgrad(L.a, gw, scale, out_bf16, stream);
}
}  // namespace

int launch_conv_igemm_wgrad(const WgradRequest &r, int out_bf16, hipStream_t stream) {
    WgradLaunch L;
    if (int rc = prepare_wgrad(r, igemm_variant(), L)) return rc;
    return run_wgrad(L, r.gw, nullptr, out_bf16, stream);
}

// the merged grid of two prepared halves (a.nd / a.nw blocks, padded to multiples of 8; a.w_first: the order)
static int launch_bwd_grid(const IgemmBwdArgs &a, hipStream_t stream) {
    static LdsGrant grant;
    constexpr size_t lds = ICfg<64, 2>::LDS > (size_t)(2 * kWStage) ? ICfg<64, 2>::LDS : (size_t)(2 * kWStage);
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&conv_igemm_bwd_kernel), lds, grant)) return rc;
    hipLaunchKernelGGL(conv_igemm_bwd_kernel, dim3(a.w_first ? a.nw_pad + a.nd : a.nd_pad + a.nw), dim3(512), lds, stream, a);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// ---- a whole backward: prepare_backward (one convolution) or prepare_backward_groups decides, run_backward launches
namespace {
// Both halves prepared — whole tiles, no stream-K — and how they run: as one grid (conv_igemm_bwd_kernel) in the order w_first, or
// as two launches.  Same results either way: the two halves of the merged kernel run the very code of the separate kernels on the
// very argument blocks
struct Backward {
    IgemmLaunch d;
    WgradLaunch w;
    bool merge;
    int w_first;
};

// the data gradient of g with the flipped kernels wd (cout -> cin channels), with the ReLU / Dropout backward and the bias gradients
// of the layer below where masks are given, as launch_conv_igemm's fused form
IgemmRequest dgrad_half(const BackwardRequest &r) {
    IgemmRequest q;
    put_groups(q.x, r.g, 4); put_groups(q.w, r.wd, 4); put_groups(q.y, r.gx, 4); put_groups(q.mask, r.mask, 4);
    put_groups(q.colsum, r.bias_grad, 4); put_groups(q.dil, r.dil, 4);
    q.masked = r.masked; q.colsums = r.bias_grads; q.ngroups = r.ngroups;
    q.s = {r.s.B, r.s.H, r.s.W, r.s.cout, r.s.cin, r.s.k};
    q.out_scale = r.mask_scale;
    q.colsum_ws = r.colsum_ws; q.colsum_ws_bytes = r.colsum_ws_bytes;
    q.res = r.res;
    q.may_stream_k = false;
    return q;
}
// the weight gradient from (x, g): gw is (cout, cin, k, k) in float32
WgradRequest wgrad_half(const BackwardRequest &r, int forced_ksplit) {
    WgradRequest q;
    put_groups(q.x, r.x, 4); put_groups(q.g, r.g, 4); put_groups(q.gw, r.gw, 4); put_groups(q.dil, r.dil, 4);
    q.ngroups = r.ngroups;
    q.workspace = r.wgrad_ws; q.workspace_bytes = r.wgrad_ws_bytes;
    q.s = r.s;
    q.forced_ksplit = forced_ksplit;
    return q;
}

// ONE convolution: the split and block order of the merged grid come from merged_backward_split (igemm_plan.h).  Two launches where
// the merged kernel does not apply (a dilation >= 3: the XCD-interleaved forms; the variants without it).  Launches nothing
int prepare_backward(const BackwardRequest &r, const IgemmVariant &v, Backward &P) {
    if (int rc = prepare_igemm(dgrad_half(r), v, P.d)) return rc;
    const int dil = r.dil[0], k = r.s.k;
    const bool merge = ((k == 3 && dil < 3) || k == 1) && v.merged_backward && !P.d.sk.base.xcd_mix && P.d.grid >= 1;
    const std::pair<int, int> pick = merge ? merged_backward_split(r.s.B, r.s.H, r.s.W, r.s.cin, r.s.cout, k, P.d.grid, igemm_cus()) : std::make_pair(0, 0);
    if (int rc = prepare_wgrad(wgrad_half(r, pick.first), v, P.w)) return rc;
    P.merge = merge && P.w.grid >= 1;
    P.w_first = pick.second;
    return DSRG_OK;
}

// 1 - 4 convolutions of one geometry (the four ASPP branches), both halves in their GROUPED forms — the data gradient with its
// XCD-interleaved map and class-ordered or row tiles where the kernels are dilated (fc6 x4), mask and bias sums in its store where
// masks are given (fc7 x4); the weight gradient on its uniform split (fc7 x4: searched for this grid) or on its per-tap work list
// (fc6 x4: the list of the launch alone, so its bits are that launch's).  Both bodies decode group, tile and list entry from
// (arguments, block id, blocks of their half), so the kernel is conv_igemm_bwd_kernel as it is; the planner prices both halves block
// by block (merged_groups_plan, igemm_plan.h).  Where it declines, or the variant has no merged backward: two launches.
// r.forced_ksplit / r.forced_order: BackwardRequest.  Launches nothing
int prepare_backward_groups(const BackwardRequest &r, const IgemmVariant &v, Backward &P, MergedGroupsPlan &plan) {
    const int ngroups = r.ngroups, B = r.s.B, H = r.s.H, W = r.s.W, cin = r.s.cin, cout = r.s.cout, k = r.s.k;
    if (int rc = prepare_igemm(dgrad_half(r), v, P.d)) return rc;
    if (int rc = prepare_wgrad(wgrad_half(r, 0), v, P.w)) return rc;
    const IgemmArgs &a = P.d.sk.base;
    // the planner's own reading of the geometry must be what was prepared: its block costs follow the kernels' id decode
    const DgradShape ds = dgrad_shape_for(ngroups, B, H, W, cin, cout, k, r.dil, v);
    const WgradShape ws = wgrad_shape_for(ngroups, B, H, W, cin, cout, k, r.dil, v, 0, igemm_cus());
    if (ds.grid != P.d.grid || ds.tiles_m != a.tiles_m || ds.tiles_n != a.tiles_n || ds.xcd_mix != a.xcd_mix || ds.row_tiles != a.row_tiles ||
        ds.cls_tiles != a.cls_tiles || ws.grid != P.w.grid || ws.ksplit != P.w.a.ksplit || ws.xcd_mix != P.w.a.xcd_mix ||
        ws.compact != P.w.a.compact || ws.nent != P.w.a.nent || (ws.plan != nullptr) != (P.w.plan != nullptr))
        return set_error(DSRG_ERR_INVALID, "conv_igemm_backward_groups: the planner and the launcher disagree on the grid");
    plan = MergedGroupsPlan{false, 0, P.w.plan ? 0 : P.w.a.ksplit, 0.0, 0.0};
    if (v.merged_backward && P.d.grid >= 1 && P.w.grid >= 1) {
        plan = merged_groups_plan(ds, cin, cout, k, v, P.w.plan ? 0 : r.forced_ksplit, igemm_cus());
        if (plan.merge && r.forced_order > 0) plan.w_first = r.forced_order == 2;
        if (plan.ksplit > 0 && plan.ksplit != P.w.a.ksplit)
            if (int rc = prepare_wgrad(wgrad_half(r, plan.ksplit), v, P.w)) return rc;
    }
    P.merge = plan.merge;
    P.w_first = plan.w_first;
    return DSRG_OK;
}

// Merged: the work list (if the weight gradient runs one) is stored in front of the grid as in front of every launch that reads it
int run_backward(const Backward &P, void *const *gw, const float *gw_scale, float *const *bias_grad, hipStream_t stream) {
    if (!P.merge) {
        if (int rc = run_igemm(P.d, bias_grad, stream)) return rc;
        return run_wgrad(P.w, gw, gw_scale, 0, stream);
    }
    if (int rc = upload_wgrad_plan(P.w, stream)) return rc;
    IgemmBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.d = P.d.sk.base;
    a.w = P.w.a;
    a.nd = P.d.grid; a.nd_pad = merged_second_half_start(a.nd); a.nw = P.w.grid; a.nw_pad = merged_second_half_start(a.nw);
    a.w_first = P.w_first;
    if (int rc = launch_bwd_grid(a, stream)) return rc;
    if (int rc = run_colsum(a.d, bias_grad, stream)) return rc;
    return reduce_wgrad(a.w, gw, gw_scale, 0, stream);
}
}  // namespace

// The backward of one convolution: r.ngroups = 1, r.res and r.gw_scale as a ResNet bottleneck convolution wants them
int launch_conv_igemm_backward(const BackwardRequest &r, hipStream_t stream) {
    Backward P;
    if (int rc = prepare_backward(r, igemm_variant(), P)) return rc;
    return run_backward(P, r.gw, r.gw_scale, r.bias_grads ? r.bias_grad : nullptr, stream);
}

int launch_conv_igemm_backward_groups(const BackwardRequest &r, hipStream_t stream) {
    if (r.bias_grads && !r.masked) return set_error(DSRG_ERR_INVALID, "conv_igemm_backward_groups: bias gradients come with the masks");
    Backward P;
    MergedGroupsPlan plan;
    if (int rc = prepare_backward_groups(r, igemm_variant(), P, plan)) return rc;
    return run_backward(P, r.gw, nullptr, r.bias_grads ? r.bias_grad : nullptr, stream);
}

// host only: what launch_conv_igemm_backward_groups would do for this geometry under the current variant — out[0] merged grid or two
// launches, out[1] w_first, out[2] the weight gradient's uniform split (0: its work list), out[3] / out[4] blocks of the data /
// weight gradient half; us[0] / us[1] the model's price of the choice and of the two launches (0 where nothing was priced)
int conv_igemm_backward_groups_plan(int ngroups, const ConvGeom &s, const int *dil, int with_mask, int forced_ksplit, int forced_order, int *out,
                                    double *us) {
    if (ngroups < 1 || ngroups > 4 || !out || !us) return set_error(DSRG_ERR_INVALID, "conv_igemm_backward_groups_plan: 1..4 groups");
    // (nothing is launched: the prepared argument blocks only ever hold these stand-in addresses)
    void *const fake = reinterpret_cast<void *>(uintptr_t(256));
    BackwardRequest r;
    for (int q = 0; q < ngroups; q++) {
        r.g[q] = r.wd[q] = r.x[q] = r.gx[q] = r.gw[q] = fake;
        if (with_mask) { r.mask[q] = fake; r.bias_grad[q] = static_cast<float *>(fake); }
    }
    r.masked = r.bias_grads = with_mask != 0;
    put_groups(r.dil, dil, ngroups);
    r.ngroups = ngroups;
    r.s = s;
    r.colsum_ws = with_mask ? fake : nullptr;
    r.colsum_ws_bytes = conv_igemm_colsum_workspace(ngroups, s.B, s.H, s.W, s.cin);
    r.wgrad_ws = fake;
    r.wgrad_ws_bytes = wgrad_workspace_bytes(ngroups, s.B, s.H, s.W, s.cin, s.cout, s.k);
    r.forced_ksplit = forced_ksplit; r.forced_order = forced_order;
    Backward P;
    MergedGroupsPlan plan;
    if (int rc = prepare_backward_groups(r, igemm_variant(), P, plan)) return rc;
    out[0] = plan.merge; out[1] = plan.w_first; out[2] = plan.ksplit; out[3] = P.d.grid; out[4] = P.w.grid;
    us[0] = plan.merged_us; us[1] = plan.separate_us;
    return DSRG_OK;
}

int launch_pack_conv_weight(const float *w, void *fwd, void *dgrad, int cout, int cin, int k, hipStream_t stream, int plain, const float *scale) {
    if (!w || cout < 64 || cout % 64 || cin < 64 || cin % 64 || (k != 1 && k != 3))
        return set_error(DSRG_ERR_INVALID, "pack_conv_weight: 64 | cout, 64 | cin, k in (1, 3) required (got %d, %d, %d)", cout, cin, k);
    if (!fwd && !dgrad) return DSRG_OK;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(cout / 64, cin / 64, k * k), dim3(256), 0, stream, w, static_cast<uint16_t *>(fwd),
                       static_cast<uint16_t *>(dgrad), cout, cin, k * k, plain, scale);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// tests: the error word of the last stream-K launch that used this workspace (1 = a workgroup gave up waiting); synchronises
int conv_igemm_workspace_status(const void *workspace, hipStream_t stream, int *status) {
    uint32_t v = 0;
    const unsigned char *p = static_cast<const unsigned char *>(workspace) + (size_t)igemm_cus() * (32 * 512 * 16) + sizeof(uint32_t) * (size_t)igemm_cus();
    DSRG_HIP_CHECK(hipMemcpyAsync(&v, p, sizeof(v), hipMemcpyDeviceToHost, stream));
    DSRG_HIP_CHECK(hipStreamSynchronize(stream));
    *status = (int)v;
    return DSRG_OK;
}

}  // namespace dsrg
