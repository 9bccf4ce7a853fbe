// Softmax loss at label resolution in two launches: a batch of (B, C, h, w) logits and its (B, 1, H, W) label maps -> the mean loss
// over the valid pixels, its gradient with respect to the logits, and three counters.  The logits are zoomed to H x W on the fly; no
// zoomed score, probability or gradient of size B*C*H*W reaches memory.
//
// The zoom is eval.hip's / multiscale.hip's at K = 1, operation for operation (the score the loss sees at a pixel is the score
// dsrg_eval_confusion_batch ranks):
//   scale = (in - 1) / (out - 1) in double on the host (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
//   l1 = src - i0, l0 = 1 - l1, z = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11) in double, rounded once to f32
// (-ffp-contract=off: every product and sum rounded on its own).
// Per valid pixel (label exactly one of 0..C-1 and not ignore_label): m = max_c z_c (first maximum: strict > walking c upwards),
// e_c = expf(z_c - m), s = sum_c e_c in f32 with c ascending, r = 1 / s (one IEEE division), loss = logf(s) - (z_label - m),
// p_c = e_c * r.  The gradient is a GATHER: cell (i, j) of plane c sums (wy * wx) * (p_c - [c == label]) over the pixels whose taps
// touch it, wy = (i == y0 ? (float)l0h : 0) + (i == y1 ? (float)l1h : 0), wx alike, all in f32.
//
// seg_loss_zoom_main_kernel: a workgroup owns a tile of at most 4 x 8 low-resolution cells of one image (the map's sides split
// evenly: 41 columns are six tiles of 7, 7, 7, 7, 7, 6) and holds those cells plus a one-cell halo of all C planes in LDS ([c][cell],
// plane stride odd: lanes that differ in c hit different banks).  The tile is small so that many workgroups share a CU — at 21
// labels 39 KB of LDS each, four to a CU; the double-precision blends and the exponentials are dependent chains that want other
// waves to hide behind (8 x 8 cells with a tile's 73 x 73 pixels parked at once, 57 KB, and the columns' weights recomputed per
// pixel: 483 us against 376 us at 10 x 21 x 41 -> 321, profiles/seg_loss_probe.txt).  The pixels that can
// touch the tile — those whose (y0, x0) lies in the tile or in the halo row / column before it — are taken in chunks of at most
// kSlPark pixels and kSlChunkW columns (one chunk at 4 x 8 cells and factor 8: 41 x 73; larger factors take several, in raster
// order); the columns' taps and weights are tabulated in LDS once per chunk:
//   pass 1  one lane per pixel of the chunk: label, m, r and the argmax; m, r and the label (-1: nothing to add) are parked in LDS.
//           A pixel is OWNED by the tile that holds its (y0, x0) cell: only owned pixels add to the workgroup's loss and counters.
//   pass 2  one lane per (cell, class) of the tile: it walks the chunk's part of the cell's footprint (the pixels with y0 in
//           {i - 1, i} and x0 in {j - 1, j}) row by row, recomputes z_c and e_c from the LDS tile, sums a row's products from left
//           to right and adds the row's sum to its sum.  The sum
//           lives in grad_dev between chunks (the same lane reads back what it wrote: no other lane ever touches the cell).
// The order of every floating-point sum is fixed by the shapes alone: no floating-point atomics, neither on memory nor on LDS.
// The workgroup's loss (double) and counters go to its slot of the workspace; loss and counters are reduced over the lanes by a tree
// in LDS.  A cell with an empty footprint (shrinking) is written as 0.
//
// seg_loss_zoom_finish_kernel: every workgroup sums the slots' valid counts (integers), divides its share of grad_dev by
// (float)max(N, 1) — one IEEE division per element — and workgroup 0 also sums the losses in double in slot order (lane-strided,
// then the same tree), writes *loss_dev = (float)(sum / max(N, 1)) and adds the three counters.
#include "common.h"
#include "zoom_gather.h"

namespace dsrg {

constexpr int kSlThreads = 256;
constexpr int kSlTileH = 4, kSlTileW = 8;  // cells per tile side, at most
constexpr int kSlPark = 3072;              // pixels parked per chunk (>= 41 * 73: 4 x 8 cells at factor 8 in one chunk)
constexpr int kSlChunkW = 128;             // pixel columns per chunk, at most (the columns' taps and weights are tabulated once per chunk)
constexpr int kSlMaxBatch = 32;
constexpr int kSlFinishBlocks = 256;

struct SegLossPart {                       // a workgroup's slot of the workspace
    double loss;
    unsigned long long valid, correct, invalid;
};

__global__ __launch_bounds__(kSlThreads) void seg_loss_zoom_main_kernel(int C, const float *__restrict__ logits, int h, int w, double sh,
                                                                        double sw, const float *__restrict__ labels, int H, int W,
                                                                        float ignore_label, int TH, int TW, int nty, int ntx, int TP,
                                                                        float *grad, SegLossPart *__restrict__ parts) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    float *s_tile = reinterpret_cast<float *>(s_raw);                       // [C][TP]: (th + 2) x (tw + 2) cells per plane
    float *s_m = s_tile + (size_t)C * TP;                                   // [kSlPark]
    float *s_r = s_m + kSlPark;                                             // [kSlPark]
    signed char *s_lab = reinterpret_cast<signed char *>(s_r + kSlPark);    // [kSlPark]
    __shared__ int s_fy[kSlTileH + 2], s_fx[kSlTileW + 2];
    __shared__ double s_xl0[kSlChunkW], s_xl1[kSlChunkW];                   // a chunk's columns: l0w, l1w,
    __shared__ float s_xf0[kSlChunkW], s_xf1[kSlChunkW];                    // the two as float32,
    __shared__ int s_xo[kSlChunkW];                                         // and x0's column in the LDS tile
    __shared__ double s_redd[kSlThreads];
    __shared__ unsigned int s_redu[kSlThreads];

    const int tid = threadIdx.x;
    const int b = blockIdx.x / (nty * ntx);
    const int tix = blockIdx.x - b * (nty * ntx);
    const int ty = tix / ntx, tx = tix - ty * ntx;
    const int i_lo = ty * TH, j_lo = tx * TW;
    const int th = min(TH, h - i_lo), tw = min(TW, w - j_lo);               // the tile's cells: [i_lo, i_lo + th) x [j_lo, j_lo + tw)
    const int ti0 = i_lo - 1, tj0 = j_lo - 1;                               // the LDS tile's first row / column (may be -1)
    const int tcols = tw + 2;
    const int hw = h * w;
    const float *lg_b = logits + (size_t)b * C * hw;
    const float *lab_b = labels + (size_t)b * H * W;
    float *grad_b = grad + (size_t)b * C * hw;

    // the cells and their halo, all planes; cells off the map are never read by a blend
    const int tcells = (th + 2) * tcols;
    for (int e = tid; e < C * tcells; e += kSlThreads) {
        const int c = e / tcells, k = e - c * tcells;
        const int r = k / tcols, q = k - r * tcols;
        const int i = ti0 + r, j = tj0 + q;
        s_tile[c * TP + k] = (i >= 0 && i < h && j >= 0 && j < w) ? lg_b[(size_t)c * hw + i * w + j] : 0.0f;
    }
    // s_fy[k]: the first pixel row whose source row is >= ti0 + k; cell row r (1..th) is touched by rows [s_fy[r - 1], s_fy[r + 1])
    if (tid <= th + 1) s_fy[tid] = sl_first(sh, ti0 + tid, h, H);
    else if (tid >= 64 && tid - 64 <= tw + 1) s_fx[tid - 64] = sl_first(sw, tj0 + tid - 64, w, W);
    __syncthreads();

    const int ylo = s_fy[0], yhi = s_fy[th + 1], xlo = s_fx[0], xhi = s_fx[tw + 1];
    const int RH = yhi - ylo, RW = xhi - xlo;
    const int PW = min(RW, kSlChunkW), PH = PW > 0 ? min(RH, kSlPark / PW) : 0;
    const int ncx = PW > 0 ? (RW + PW - 1) / PW : 1, ncy = PH > 0 ? (RH + PH - 1) / PH : 1;

    double loss = 0.0;
    unsigned int n_valid = 0, n_correct = 0, n_invalid = 0;                 // (a tile's pixels: < 2^31 in all)
#pragma unroll 1
    for (int ck = 0; ck < ncy * ncx; ++ck) {
        const int cky = ck / ncx, ckx = ck - cky * ncx;
        const int cy0 = ylo + cky * PH, cy1 = min(yhi, cy0 + PH);
        const int cx0 = xlo + ckx * PW, cx1 = min(xhi, cx0 + PW);
        const int cw = cx1 - cx0, npix = (cy1 - cy0) * cw;                  // (0 where the tile has no pixel at all)
        if (ck) __syncthreads();                                            // pass 2 of the chunk before is done with the parked values
        if (tid < cw) {                                                     // the columns' table (read by pass 2, behind pass 1's barrier)
            const double sx = sw * (double)(cx0 + tid);
            const int x0 = min((int)sx, w - 1);
            const double l1w = sx - (double)x0, l0w = 1.0 - l1w;
            s_xl0[tid] = l0w, s_xl1[tid] = l1w;
            s_xf0[tid] = (float)l0w, s_xf1[tid] = (float)l1w;
            s_xo[tid] = x0 - tj0;
        }

        // ---- pass 1: a lane per pixel
#pragma unroll 1
        for (int t = tid; t < npix; t += kSlThreads) {
            const int yy = t / cw, y = cy0 + yy, x = cx0 + (t - yy * cw);
            const float l = lab_b[(size_t)y * W + x];
            const double sy = sh * (double)y, sx = sw * (double)x;
            const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
            const bool own = y0 >= i_lo && x0 >= j_lo && y0 < i_lo + th && x0 < j_lo + tw;
            int g = -1;
            if (l != ignore_label) {
                if (l >= 0.0f && l < (float)C) {
                    const int gi = (int)l;
                    if ((float)gi == l) g = gi;
                }
                if (g < 0 && own) ++n_invalid;
            }
            s_lab[t] = (signed char)g;
            if (g < 0) continue;
            const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
            const double l1h = sy - (double)y0, l1w = sx - (double)x0;
            const double l0h = 1.0 - l1h, l0w = 1.0 - l1w;
            const int o00 = (y0 - ti0) * tcols + (x0 - tj0), o01 = (y0 - ti0) * tcols + (x1 - tj0);
            const int o10 = (y1 - ti0) * tcols + (x0 - tj0), o11 = (y1 - ti0) * tcols + (x1 - tj0);
            float m = 0.0f;
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                const float *pl = s_tile + c * TP;
                const double v00 = pl[o00], v01 = pl[o01], v10 = pl[o10], v11 = pl[o11];
                const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
                if (c == 0 || z > m) { m = z; arg = c; }
            }
            float s = 0.0f, zl = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float *pl = s_tile + c * TP;
                const double v00 = pl[o00], v01 = pl[o01], v10 = pl[o10], v11 = pl[o11];
                const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
                s += expf(z - m);
                if (c == g) zl = z;
            }
            s_m[t] = m;
            s_r[t] = 1.0f / s;
            if (own) {
                ++n_valid;
                n_correct += arg == g ? 1u : 0u;
                loss += (double)(logf(s) - (zl - m));
            }
        }
        __syncthreads();

        // ---- pass 2: a lane per (cell, class)
#pragma unroll 1
        for (int q = tid; q < th * tw * C; q += kSlThreads) {
            const int cell = q / C, c = q - cell * C;
            const int r = cell / tw + 1, cc = cell - (r - 1) * tw + 1;      // the cell's row / column in the LDS tile
            const int i = ti0 + r, j = tj0 + cc;
            float *dst = grad_b + (size_t)c * hw + i * w + j;
            float acc = ck ? *dst : 0.0f;
            const float *pl = s_tile + c * TP;
            const int ya = max(s_fy[r - 1], cy0), yb = min(s_fy[r + 1], cy1);
            const int xa = max(s_fx[cc - 1], cx0), xb = min(s_fx[cc + 1], cx1);
#pragma unroll 1
            for (int y = ya; y < yb; ++y) {
                const double sy = sh * (double)y;
                const int y0 = min((int)sy, h - 1), y1 = y0 + (y0 < h - 1 ? 1 : 0);
                const double l1h = sy - (double)y0, l0h = 1.0 - l1h;
                const float wy = (y0 == i ? (float)l0h : 0.0f) + (y1 == i ? (float)l1h : 0.0f);
                const int t0 = (y - cy0) * cw - cx0;
                const int oy0 = (y0 - ti0) * tcols, oy1 = (y1 - ti0) * tcols;
                float row = 0.0f;                                           // a row's sum first: shorter chains of float32 additions
#pragma unroll 1
                for (int x = xa; x < xb; ++x) {
                    const int g = s_lab[t0 + x];
                    if (g < 0) continue;
                    const int k = x - cx0;
                    const int o0 = s_xo[k], x0 = o0 + tj0, step = x0 < w - 1 ? 1 : 0, o1 = o0 + step;
                    const double l0w = s_xl0[k], l1w = s_xl1[k];
                    const float wx = (x0 == j ? s_xf0[k] : 0.0f) + (x0 + step == j ? s_xf1[k] : 0.0f);
                    const double v00 = pl[oy0 + o0], v01 = pl[oy0 + o1], v10 = pl[oy1 + o0], v11 = pl[oy1 + o1];
                    const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
                    const float p = expf(z - s_m[t0 + x]) * s_r[t0 + x];
                    row += (wy * wx) * (p - (c == g ? 1.0f : 0.0f));
                }
                acc += row;
            }
            *dst = acc;
        }
    }

    // the workgroup's slot
    const double tl = sl_block_sum<kSlThreads>(loss, s_redd);
    const unsigned int tv = sl_block_sum<kSlThreads>(n_valid, s_redu);
    const unsigned int tc = sl_block_sum<kSlThreads>(n_correct, s_redu);
    const unsigned int ti = sl_block_sum<kSlThreads>(n_invalid, s_redu);
    if (tid == 0) {
        SegLossPart p;
        p.loss = tl, p.valid = tv, p.correct = tc, p.invalid = ti;
        parts[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(kSlThreads) void seg_loss_zoom_finish_kernel(int nparts, const SegLossPart *__restrict__ parts,
                                                                          unsigned int total, float *__restrict__ grad,
                                                                          float *__restrict__ loss_out,
                                                                          unsigned long long *__restrict__ counters) {
    __shared__ double s_redd[kSlThreads];
    __shared__ unsigned long long s_redu[kSlThreads];
    const int tid = threadIdx.x;
    unsigned long long nv = 0;
    for (int k = tid; k < nparts; k += kSlThreads) nv += parts[k].valid;
    const unsigned long long N = sl_block_sum<kSlThreads>(nv, s_redu);
    const unsigned long long D = N > 0 ? N : 1;
    if (blockIdx.x == 0) {
        double l = 0.0;
        unsigned long long nc = 0, ni = 0;
        for (int k = tid; k < nparts; k += kSlThreads) {
            l += parts[k].loss;
            nc += parts[k].correct;
            ni += parts[k].invalid;
        }
        const double L = sl_block_sum<kSlThreads>(l, s_redd);
        const unsigned long long NC = sl_block_sum<kSlThreads>(nc, s_redu);
        const unsigned long long NI = sl_block_sum<kSlThreads>(ni, s_redu);
        if (tid == 0) {
            *loss_out = (float)(L / (double)D);
            counters[0] += N;
            counters[1] += NC;
            counters[2] += NI;
        }
    }
    const float den = (float)D;
    const unsigned int stride = gridDim.x * kSlThreads;                     // (total < 2^31: e + stride stays inside 32 bits)
    for (unsigned int e = blockIdx.x * kSlThreads + tid; e < total; e += stride) grad[e] = grad[e] / den;
}

static int seg_loss_tiles(int n, int side) { return (n + side - 1) / side; }

// every argument of the pair below, checked by one routine: the workspace size function answers 0 for what the launch refuses
static int seg_loss_check_shapes(int B, int C, int h, int w, int H, int W) {
    if (B < 1 || B > kSlMaxBatch) return set_error(DSRG_ERR_INVALID, "seg loss zoom: 1..%d images, got %d", kSlMaxBatch, B);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "seg loss zoom: %d labels", C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_UNSUPPORTED, "seg loss zoom: at most %d labels, got %d", kMaxLabels, C);
    if (h < 1 || w < 1 || H < 1 || W < 1)
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: logit maps %dx%d, label maps %dx%d", h, w, H, W);
    // (each factor is < 2^31 and B * C <= 3072: the running products below stay far inside 64 bits)
    if ((long long)B * C * h >= (1LL << 31) || (long long)B * C * h * w >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: B*C*h*w >= 2^31");
    if ((long long)B * H >= (1LL << 31) || (long long)B * H * W >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: B*H*W >= 2^31");
    return DSRG_OK;
}

size_t seg_loss_zoom_workspace(int B, int C, int h, int w, int H, int W) {
    if (seg_loss_check_shapes(B, C, h, w, H, W) != DSRG_OK) return 0;
    return (size_t)B * seg_loss_tiles(h, kSlTileH) * seg_loss_tiles(w, kSlTileW) * sizeof(SegLossPart);
}

int launch_seg_loss_zoom_batch(int B, int C, const float *logits, int h, int w, const float *labels, int H, int W, float ignore_label,
                               float *loss, float *grad, unsigned long long *counters, void *workspace, size_t workspace_bytes,
                               hipStream_t stream) {
    if (!logits || !labels || !loss || !grad || !counters || !workspace)
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: NULL logits / labels / loss / grad / counters / workspace");
    if (int rc = seg_loss_check_shapes(B, C, h, w, H, W)) return rc;
    const int nty = seg_loss_tiles(h, kSlTileH), ntx = seg_loss_tiles(w, kSlTileW);
    const long long nparts = (long long)B * nty * ntx;                      // (<= B*h*w < 2^31)
    if (workspace_bytes < (size_t)nparts * sizeof(SegLossPart))
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: workspace of %zu B, %zu needed", workspace_bytes,
                         (size_t)nparts * sizeof(SegLossPart));
    if (reinterpret_cast<uintptr_t>(workspace) % alignof(SegLossPart))
        return set_error(DSRG_ERR_INVALID, "seg loss zoom: the workspace must be %zu-byte aligned", alignof(SegLossPart));
    const int TH = (h + nty - 1) / nty, TW = (w + ntx - 1) / ntx;           // the sides split evenly: <= 4 x 8 cells
    const int TP = ((TH + 2) * (TW + 2)) | 1;
    const double sh = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
    const double sw = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
    const size_t lds = (size_t)C * TP * sizeof(float) + (size_t)kSlPark * (2 * sizeof(float) + 1);     // <= 51 072 B at C = 96
    static LdsGrant grant;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(seg_loss_zoom_main_kernel), lds, grant)) return rc;
    hipLaunchKernelGGL(seg_loss_zoom_main_kernel, dim3((unsigned)nparts), dim3(kSlThreads), lds, stream, C, logits, h, w, sh, sw, labels, H,
                       W, ignore_label, TH, TW, nty, ntx, TP, grad, static_cast<SegLossPart *>(workspace));
    DSRG_LAUNCH_CHECK();
    const unsigned int total = (unsigned int)((long long)B * C * h * w);
    const unsigned int want = (total + kSlThreads - 1) / kSlThreads;
    hipLaunchKernelGGL(seg_loss_zoom_finish_kernel, dim3(want < (unsigned)kSlFinishBlocks ? want : (unsigned)kSlFinishBlocks),
                       dim3(kSlThreads), 0, stream, (int)nparts, static_cast<const SegLossPart *>(workspace), total, grad, loss, counters);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
