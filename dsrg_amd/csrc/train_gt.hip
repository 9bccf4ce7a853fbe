// The tail of the weakly supervised pseudo-label pass: scores -> the full-resolution probabilities / dense-CRF unary / restricted
// labels, for a group of G images, from M = K * (1 + flip) score maps per image — K sizes, each optionally with the map of the
// mirrored input; the maps are the slices of K batched forwards.  Per map m: P_m = softmax over labels per MAP pixel, z_m = the
// order-1 zoom of P_m (the PROBABILITIES) to the image; then acc = z_0, acc = acc + z_m in list order (scale 0 plain, scale 0
// mirror, scale 1 plain, ...), p = max(acc / (float)M, eps) (no division at M = 1); the unary is logf(p), the label the arg-max
// over background + the image-level labels.  K = 1 without flip (--mode gt, dsrg_train_gt_unary_batch) is what
// generate_train_gt.py:85-104 computes; the ensemble (--mode gt-ms) has no counterpart in the reference.  multiscale.hip zooms
// scores and then takes the softmax; this is the other order, which gives other numbers, so it is a sibling of
// multiscale_unary_body and not a mode of it.
//
// Two launches on one stream, whatever K is:
//   A. train_gt_ms_softmax_kernel: one thread per (map, slice, map pixel) over the used slices of all K maps (blockIdx.x -> map
//      through block prefix sums; a block never straddles two maps): m = max_c s, e_c = expf(s_c - m) (d = s - m in f32, as numpy
//      computes it on the float32 blob), sum in label order, p_c = e_c / sum -> probability planes (slices, C, h_k * w_k) per map,
//      map after map, in the caller's workspace
//   B. train_gt_ms_zoom_kernel<K, FLIP>: one workgroup owns 64 consecutive output pixels of one image (blockIdx.x -> (image, block)
//      through per-image block prefix sums, as multiscale_unary_batch_kernel)
//        1. per (pixel, scale): the two source rows / columns and the blend weights, fp64, in registers (the arithmetic
//           multiscale.hip documents for its step 2: scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src,
//           i1 = i0 + (i0 < in - 1), l1 = src - i0).  A mirror map is read as flip(map, last axis): rows, x0, x1 and the weights
//           come from the output pixel as for the plain map, only the four loads move to columns w - 1 - x0 and w - 1 - x1 (the
//           rule of multiscale_unary_body)
//        2. per (pixel, label): the M blends f32(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)), each rounded
//           once, summed in a register in list order, divided, clamped -> LDS tile [64][C], written once
//        3. per pixel: the restricted selection (select_label) -> labels
//        4. the block's 64 * C floats as float4 rows: the clamped probabilities, and / or their logf (the unary)
// -ffp-contract=off (Makefile) keeps every product and sum rounded on its own.  No atomics: results are bit-reproducible, and
// image g's outputs do not depend on the group it is in.
#include <math.h>
#include <string.h>
#include "common.h"

namespace dsrg {

constexpr int kTgMsMaxMaps = 8;        // M = K * (1 + flip) maps per image
constexpr int kTgMsMaxFlipBatch = 8;   // images per launch with flip: two slices each in a batch of at most 16

struct TgMsSoftmaxArgs {
    const float *s[kTgMsMaxMaps];      // (Gcap, C, h_k, w_k) score maps; the first `slices` slices are read
    size_t off[kTgMsMaxMaps];          // floats of the workspace before map k's planes
    int hw[kTgMsMaxMaps];
    int blk0[kTgMsMaxMaps + 1];        // the first block of map k (blk0[K] = the grid)
};

__global__ __launch_bounds__(256) void train_gt_ms_softmax_kernel(TgMsSoftmaxArgs a, float *__restrict__ planes, int K, int slices,
                                                                  int C) {
    const int blk = (int)blockIdx.x;
    int k = 0;
    while (k + 1 < K && blk >= a.blk0[k + 1]) ++k;          // (uniform over the block)
    const int hw = a.hw[k];
    const size_t idx = (size_t)(blk - a.blk0[k]) * blockDim.x + threadIdx.x;
    if (idx >= (size_t)slices * hw) return;
    const size_t g = idx / (size_t)hw, i = idx - g * (size_t)hw;
    const float *s = a.s[k] + g * (size_t)C * hw + i;
    float *o = planes + a.off[k] + g * (size_t)C * hw + i;
    float m = s[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, s[(size_t)c * hw]);
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum = sum + expf(s[(size_t)c * hw] - m);
    for (int c = 0; c < C; ++c) o[(size_t)c * hw] = expf(s[(size_t)c * hw] - m) / sum;
}

struct TgMsBatchArgs {                 // 2.9 KB by value (the kernel-argument segment holds 4 KB)
    const float *planes;               // pass A's workspace
    size_t off[kTgMsMaxMaps];          // floats before scale k's planes: (slices, C, h_k * w_k)
    int h[kTgMsMaxMaps], w[kTgMsMaxMaps];
    int H[kTgMaxBatch], W[kTgMaxBatch];
    int blk0[kTgMaxBatch + 1];
    float *unary[kTgMaxBatch];
    float *probs[kTgMaxBatch];
    int32_t *labels[kTgMaxBatch];
    int nsel[kTgMaxBatch];
    unsigned char sel[kTgMaxBatch][kMaxSelect];
};
static_assert(sizeof(TgMsBatchArgs) + 4 * sizeof(int) <= 4096, "the by-value arguments must fit the 4 KB kernel-argument segment");

// K scales; FLIP: image g reads slices 2g (plain) and 2g + 1 (mirrored) of every scale, otherwise slice g
template <int K, bool FLIP>
__global__ __launch_bounds__(kTgThreads) void train_gt_ms_zoom_kernel(TgMsBatchArgs b, int G, int C, float eps, float ignore_below) {
    __shared__ float s_tile[kTgPix * (kMaxLabels + 1)];     // [pixel][label], row stride Cs (odd: conflict-free columns)
    __shared__ int s_sel[kMaxSelect];
    constexpr int M = K * (FLIP ? 2 : 1);

    const int blk_all = (int)blockIdx.x;
    int g = 0;
    while (g + 1 < G && blk_all >= b.blk0[g + 1]) ++g;      // (uniform over the block)
    const int H = b.H[g], W = b.W[g];
    float *unary = b.unary[g], *probs = b.probs[g];
    int32_t *labels = b.labels[g];

    const int N = H * W;
    const int pix0 = (blk_all - b.blk0[g]) * kTgPix;
    const int npb = min(kTgPix, N - pix0);
    const int Cs = C | 1;
    const int tid = threadIdx.x;
    const int nsel = labels ? b.nsel[g] : 0;
    if (tid < nsel) s_sel[tid] = b.sel[g][tid];

    {
        // 1. this lane's pixel (lanes p, p + 64, p + 128, p + 192 share it and take every fourth label): per scale the taps and
        // weights, in registers
        const int p = tid % kTgPix, c0 = tid / kTgPix;
        const int i = pix0 + min(p, npb - 1);
        const int y = i / W, x = i - y * W;
        const float *base[K];                               // label 0 of the image's (plain) slice
        int o00[K], o01[K], o10[K], o11[K], hw[K];
        int m00[FLIP ? K : 1], m01[FLIP ? K : 1], m10[FLIP ? K : 1], m11[FLIP ? K : 1];     // the mirror slice's taps
        double l1h[K], l1w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int h = b.h[k], w = b.w[k];
            const double sh = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
            const double sw = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
            const double sy = sh * (double)y, sx = sw * (double)x;
            const int y0 = (int)sy, x0 = (int)sx;
            const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
            hw[k] = h * w;
            o00[k] = y0 * w + x0;
            o01[k] = y0 * w + x1;
            o10[k] = y1 * w + x0;
            o11[k] = y1 * w + x1;
            if constexpr (FLIP) {
                m00[k] = y0 * w + (w - 1 - x0);
                m01[k] = y0 * w + (w - 1 - x1);
                m10[k] = y1 * w + (w - 1 - x0);
                m11[k] = y1 * w + (w - 1 - x1);
            }
            l1h[k] = sy - (double)y0;
            l1w[k] = sx - (double)x0;
            base[k] = b.planes + b.off[k] + (size_t)(FLIP ? 2 * g : g) * C * hw[k];
        }
        // 2. the ensemble of every label: the M zoomed probabilities summed in list order, divided by M, clamped
#pragma unroll 1
        for (int c = c0; c < C; c += kTgThreads / kTgPix) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float *plane = base[k] + (size_t)c * hw[k];
                const double l0h = 1.0 - l1h[k], l0w = 1.0 - l1w[k];
                {
                    const double v00 = plane[o00[k]], v01 = plane[o01[k]], v10 = plane[o10[k]], v11 = plane[o11[k]];
                    const float z = (float)(l0h * (l0w * v00 + l1w[k] * v01) + l1h[k] * (l0w * v10 + l1w[k] * v11));
                    acc = k == 0 ? z : acc + z;
                }
                if constexpr (FLIP) {
                    const float *mplane = plane + (size_t)C * hw[k];           // the same label of the mirror slice, 2g + 1
                    const double v00 = mplane[m00[k]], v01 = mplane[m01[k]], v10 = mplane[m10[k]], v11 = mplane[m11[k]];
                    const float z = (float)(l0h * (l0w * v00 + l1w[k] * v01) + l1h[k] * (l0w * v10 + l1w[k] * v11));
                    acc = acc + z;
                }
            }
            if (M > 1) acc = acc / (float)M;
            s_tile[p * Cs + c] = fmaxf(acc, eps);
        }
    }
    __syncthreads();

    // 3. the restricted selection, one lane per pixel
    if (labels && tid < npb) {
        const float *row = s_tile + tid * Cs;
        int lab = select_label(row, 1, s_sel, nsel);
        if (ignore_below > 0.0f && max_label_value(row, 1, C) < ignore_below) lab = kIgnoreLabel;
        labels[pix0 + tid] = lab;
    }

    // 4. the block's output floats [pix0 * C, (pix0 + npb) * C) as float4 rows (pix0 * C is a multiple of 64)
    if (!unary && !probs) return;
    const int n = npb * C;
    const float invC = 1.0f / (float)C;
    const size_t out0 = (size_t)pix0 * C;
    for (int j4 = tid * 4; j4 < n; j4 += kTgThreads * 4) {
        float pv[4], uv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = min(j4 + r, n - 1);
            // j / C for j < 64 * 96: the quotient's fractional part is >= 0.5 / C away from the next integer, far above the error
            const int p = (int)(((float)j + 0.5f) * invC);
            const int c = j - p * C;
            pv[r] = s_tile[p * Cs + c];
            uv[r] = logf(pv[r]);
        }
        if (j4 + 4 <= n) {
            if (probs) *reinterpret_cast<float4 *>(probs + out0 + j4) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            if (unary) *reinterpret_cast<float4 *>(unary + out0 + j4) = make_float4(uv[0], uv[1], uv[2], uv[3]);
        } else {
            for (int r = 0; r < n - j4; ++r) {
                if (probs) probs[out0 + j4 + r] = pv[r];
                if (unary) unary[out0 + j4 + r] = uv[r];
            }
        }
    }
}

// one selection list of an entry point, checked on the host: 1..128 entries, each a label of [0, C)
int check_select_list(const char *who, int image, const int32_t *sel, int n, int stride, int C) {
    if (n < 1 || n > kMaxSelect)
        return set_error(DSRG_ERR_INVALID, "%s: a selection list holds 1..%d labels, image %d has %d", who, kMaxSelect, image, n);
    if (n > stride)
        return set_error(DSRG_ERR_INVALID, "%s: the list of image %d (%d labels) is longer than select_stride %d", who, image, n, stride);
    for (int j = 0; j < n; ++j)
        if (sel[j] < 0 || sel[j] >= C)
            return set_error(DSRG_ERR_INVALID, "%s: selection entry %d of image %d is label %d, outside [0, %d)", who, j, image,
                             (int)sel[j], C);
    return DSRG_OK;
}

// who: the entry point the messages name ("train-gt ensemble", "train-gt unary")
int launch_train_gt_ensemble_batch(const char *who, int G, int K, int flip, int C, const float *const *scores, const int32_t *h,
                                   const int32_t *w, const int32_t *H, const int32_t *W, float eps, const int32_t *select,
                                   const int32_t *nselect, int select_stride, float ignore_below, float *workspace,
                                   float *const *unary, float *const *probs, int32_t *const *labels, hipStream_t stream) {
    const int per = flip ? 2 : 1;
    const int maxG = flip ? kTgMsMaxFlipBatch : kTgMaxBatch, maxK = kTgMsMaxMaps / per;
    if (G < 1 || G > maxG)
        return set_error(DSRG_ERR_INVALID, "%s: 1..%d images%s, got %d", who, maxG, flip ? " with flip (two slices each)" : "", G);
    if (K < 1 || K > maxK)
        return set_error(DSRG_ERR_INVALID, "%s: 1..%d sizes%s (at most %d maps per image), got %d", who, maxK,
                         flip ? " with flip" : "", kTgMsMaxMaps, K);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "%s: %d labels", who, C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_INVALID, "%s: at most %d labels, got %d", who, kMaxLabels, C);
    if (!scores) return set_error(DSRG_ERR_INVALID, "%s: NULL score map array", who);
    if (!h || !w) return set_error(DSRG_ERR_INVALID, "%s: NULL score map size array", who);
    if (!H || !W) return set_error(DSRG_ERR_INVALID, "%s: NULL image size array", who);
    if (!workspace) return set_error(DSRG_ERR_INVALID, "%s: NULL workspace", who);
    const int slices = per * G;
    TgMsSoftmaxArgs a;
    TgMsBatchArgs b;
    memset(&a, 0, sizeof(a));
    memset(&b, 0, sizeof(b));
    size_t off = 0;
    for (int k = 0; k < K; ++k) {
        if (!scores[k]) return set_error(DSRG_ERR_INVALID, "%s: score map %d is NULL", who, k);
        if (h[k] < 1 || w[k] < 1) return set_error(DSRG_ERR_INVALID, "%s: score map %d is %dx%d", who, k, h[k], w[k]);
        if ((long long)h[k] * w[k] * C >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "%s: score map %d holds >= 2^31 values", who, k);
        a.s[k] = scores[k];
        a.off[k] = b.off[k] = off;
        a.hw[k] = h[k] * w[k];
        // (slices * h * w < 2^35: fewer than 2^27 blocks per map, 2^30 in all)
        a.blk0[k + 1] = a.blk0[k] + (int)(((size_t)slices * a.hw[k] + 255) / 256);
        b.h[k] = h[k];
        b.w[k] = w[k];
        off += (size_t)slices * C * a.hw[k];
    }
    const int cu = output_class((const void *const *)unary, G), cp = output_class((const void *const *)probs, G),
              cl = output_class((const void *const *)labels, G);
    if (cu < 0 || cp < 0 || cl < 0)
        return set_error(DSRG_ERR_INVALID, "%s: an output class must be NULL or set for every image", who);
    if (!cu && !cp && !cl) return set_error(DSRG_ERR_INVALID, "%s: no output requested", who);
    if (cl && (!select || !nselect)) return set_error(DSRG_ERR_INVALID, "%s: labels need the selection lists (NULL)", who);
    for (int g = 0; g < G; ++g) {
        if (H[g] < 1 || W[g] < 1) return set_error(DSRG_ERR_INVALID, "%s: output %d is %dx%d", who, g, H[g], W[g]);
        if ((long long)H[g] * W[g] * C >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "%s: H*W*C = %lld >= 2^31", who, (long long)H[g] * W[g] * C);
        if ((cu && ((uintptr_t)unary[g] & 15)) || (cp && ((uintptr_t)probs[g] & 15)))
            return set_error(DSRG_ERR_INVALID, "%s: unary / probs outputs must be 16-byte aligned", who);
        if (cl) {
            const int32_t *sel = select + (size_t)g * (select_stride > 0 ? select_stride : 0);
            int rc = check_select_list(who, g, sel, nselect[g], select_stride, C);
            if (rc) return rc;
            b.nsel[g] = nselect[g];
            for (int j = 0; j < nselect[g]; ++j) b.sel[g][j] = (unsigned char)sel[j];
        }
        b.H[g] = H[g];
        b.W[g] = W[g];
        b.blk0[g + 1] = b.blk0[g] + (H[g] * W[g] + kTgPix - 1) / kTgPix;      // < 2^25 blocks per image
        b.unary[g] = cu ? unary[g] : nullptr;
        b.probs[g] = cp ? probs[g] : nullptr;
        b.labels[g] = cl ? labels[g] : nullptr;
    }
    b.planes = workspace;
    hipLaunchKernelGGL(train_gt_ms_softmax_kernel, dim3((unsigned)a.blk0[K]), dim3(256), 0, stream, a, workspace, K, slices, C);
    DSRG_LAUNCH_CHECK();
    const dim3 grid((unsigned)b.blk0[G]), block(kTgThreads);
    switch (flip ? -K : K) {
#define DSRG_TGMS_CASE(k, f)                                                                                                     \
    case (f ? -k : k):                                                                                                           \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(train_gt_ms_zoom_kernel<k, f>), grid, block, 0, stream, b, G, C, eps, ignore_below);                 \
        break;
        DSRG_TGMS_CASE(1, false) DSRG_TGMS_CASE(2, false) DSRG_TGMS_CASE(3, false) DSRG_TGMS_CASE(4, false)
        DSRG_TGMS_CASE(5, false) DSRG_TGMS_CASE(6, false) DSRG_TGMS_CASE(7, false) DSRG_TGMS_CASE(8, false)
        DSRG_TGMS_CASE(1, true) DSRG_TGMS_CASE(2, true) DSRG_TGMS_CASE(3, true) DSRG_TGMS_CASE(4, true)
#undef DSRG_TGMS_CASE
    }
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// generate_train_gt.py:85-104: one map per image, the ensemble at K = 1 without flip (the same G*C*h*w floats of workspace)
int launch_train_gt_unary_batch(int G, int C, const float *scores, int h, int w, const int32_t *H, const int32_t *W, float eps,
                                const int32_t *select, const int32_t *nselect, int select_stride, float ignore_below,
                                float *workspace, float *const *unary, float *const *probs, int32_t *const *labels,
                                hipStream_t stream) {
    const int32_t h1[1] = {h}, w1[1] = {w};
    return launch_train_gt_ensemble_batch("train-gt unary", G, 1, 0, C, &scores, h1, w1, H, W, eps, select, nselect, select_stride,
                                          ignore_below, workspace, unary, probs, labels, stream);
}

}  // namespace dsrg
