// Single-scale scores -> the full-resolution probabilities / dense-CRF unary / restricted labels of the weakly supervised
// pseudo-label pass: the tail of generate_train_gt.py:85-104 (softmax over labels at MAP resolution, order-1 zoom of the
// PROBABILITIES to the image, clamp at eps, log; arg-max over background + the image-level labels) for a group of G <= 16 images
// whose score maps are the slices of one batched forward.  multiscale.hip zooms scores and then takes the softmax; this is the
// other order, which gives other numbers, so it is a sibling of multiscale_unary_body and not a mode of it.
//
// Two launches on one stream:
//   A. train_gt_softmax_kernel: one thread per (image, map pixel): m = max_c s, e_c = expf(s_c - m) (d = s - m in f32, as numpy
//      computes it on the float32 blob), sum in label order, p_c = e_c / sum -> (G, C, h * w) probability planes in the caller's
//      workspace
//   B. train_gt_zoom_kernel: one workgroup owns 64 consecutive output pixels of one image (blockIdx.x -> (image, block) through
//      per-image block prefix sums, as multiscale_unary_batch_kernel)
//        1. per pixel: the two source rows / columns and the blend weights, fp64 (the arithmetic multiscale.hip documents for
//           its step 2: scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0)
//        2. per (pixel, label): max(f32(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)), eps) -> LDS tile [64][C]
//        3. per pixel: the restricted selection (select_label below) -> labels
//        4. the block's 64 * C floats as float4 rows: the clamped probabilities, and / or their logf (the unary)
// -ffp-contract=off (Makefile) keeps every product and sum rounded on its own.  No atomics: results are bit-reproducible, and
// image g's outputs do not depend on the group it is in.
#include <math.h>
#include <string.h>
#include "common.h"

namespace dsrg {

struct TgBatchArgs {
    const float *planes;           // (G, C, h * w) probabilities of pass A
    int h, w;
    int H[kTgMaxBatch], W[kTgMaxBatch];
    int blk0[kTgMaxBatch + 1];
    float *unary[kTgMaxBatch];
    float *probs[kTgMaxBatch];
    int32_t *labels[kTgMaxBatch];
    int nsel[kTgMaxBatch];
    unsigned char sel[kTgMaxBatch][kMaxSelect];
};

__global__ __launch_bounds__(256) void train_gt_softmax_kernel(const float *__restrict__ scores, float *__restrict__ planes,
                                                               int G, int C, int hw) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)G * hw) return;
    const size_t g = idx / (size_t)hw, i = idx - g * (size_t)hw;
    const float *s = scores + g * (size_t)C * hw + i;
    float *o = planes + g * (size_t)C * hw + i;
    float m = s[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, s[(size_t)c * hw]);
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum = sum + expf(s[(size_t)c * hw] - m);
    for (int c = 0; c < C; ++c) o[(size_t)c * hw] = expf(s[(size_t)c * hw] - m) / sum;
}

__global__ __launch_bounds__(kTgThreads) void train_gt_zoom_kernel(TgBatchArgs b, int G, int C, float eps, float ignore_below) {
    __shared__ float s_tile[kTgPix * (kMaxLabels + 1)];     // [pixel][label], row stride Cs (odd: conflict-free columns)
    __shared__ int s_sel[kMaxSelect];

    const int blk_all = (int)blockIdx.x;
    int g = 0;
    while (g + 1 < G && blk_all >= b.blk0[g + 1]) ++g;      // (uniform over the block)
    const int H = b.H[g], W = b.W[g], h = b.h, w = b.w;
    const double sh = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
    const double sw = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
    const float *planes = b.planes + (size_t)g * C * h * w;
    float *unary = b.unary[g], *probs = b.probs[g];
    int32_t *labels = b.labels[g];

    const int N = H * W;
    const int pix0 = (blk_all - b.blk0[g]) * kTgPix;
    const int npb = min(kTgPix, N - pix0);
    const int Cs = C | 1;
    const int tid = threadIdx.x;
    const int nsel = labels ? b.nsel[g] : 0;
    if (tid < nsel) s_sel[tid] = b.sel[g][tid];

    // 1. this lane's pixel (lanes p, p + 64, p + 128, p + 192 share it and take every fourth label)
    {
        const int p = tid % kTgPix, c0 = tid / kTgPix;
        const int i = pix0 + min(p, npb - 1);
        const int y = i / W, x = i - y * W;
        const double sy = sh * (double)y, sx = sw * (double)x;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1, hw = h * w;
        const double l1h = sy - (double)y0, l1w = sx - (double)x0;
        const double l0h = 1.0 - l1h, l0w = 1.0 - l1w;
        // 2. the zoomed, clamped probability of every label
#pragma unroll 1
        for (int c = c0; c < C; c += kTgThreads / kTgPix) {
            const float *plane = planes + (size_t)c * hw;
            const double v00 = plane[o00], v01 = plane[o01], v10 = plane[o10], v11 = plane[o11];
            const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
            s_tile[p * Cs + c] = fmaxf(z, eps);
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
    const size_t base = (size_t)pix0 * C;
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
            if (probs) *reinterpret_cast<float4 *>(probs + base + j4) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            if (unary) *reinterpret_cast<float4 *>(unary + base + j4) = make_float4(uv[0], uv[1], uv[2], uv[3]);
        } else {
            for (int r = 0; r < n - j4; ++r) {
                if (probs) probs[base + j4 + r] = pv[r];
                if (unary) unary[base + j4 + r] = uv[r];
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

int launch_train_gt_unary_batch(int G, int C, const float *scores, int h, int w, const int32_t *H, const int32_t *W, float eps,
                                const int32_t *select, const int32_t *nselect, int select_stride, float ignore_below,
                                float *workspace, float *const *unary, float *const *probs, int32_t *const *labels,
                                hipStream_t stream) {
    static const char who[] = "train-gt unary";
    if (G < 1 || G > kTgMaxBatch) return set_error(DSRG_ERR_INVALID, "%s: 1..%d images, got %d", who, kTgMaxBatch, G);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "%s: %d labels", who, C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_INVALID, "%s: at most %d labels, got %d", who, kMaxLabels, C);
    if (!scores) return set_error(DSRG_ERR_INVALID, "%s: NULL score maps", who);
    if (!workspace) return set_error(DSRG_ERR_INVALID, "%s: NULL workspace", who);
    if (!H || !W) return set_error(DSRG_ERR_INVALID, "%s: NULL image size array", who);
    if (h < 1 || w < 1) return set_error(DSRG_ERR_INVALID, "%s: score map is %dx%d", who, h, w);
    if ((long long)h * w * C >= (1LL << 31))
        return set_error(DSRG_ERR_UNSUPPORTED, "%s: a score map holds >= 2^31 values", who);
    const int cu = output_class((const void *const *)unary, G), cp = output_class((const void *const *)probs, G),
              cl = output_class((const void *const *)labels, G);
    if (cu < 0 || cp < 0 || cl < 0)
        return set_error(DSRG_ERR_INVALID, "%s: an output class must be NULL or set for every image", who);
    if (!cu && !cp && !cl) return set_error(DSRG_ERR_INVALID, "%s: no output requested", who);
    if (cl && (!select || !nselect)) return set_error(DSRG_ERR_INVALID, "%s: labels need the selection lists (NULL)", who);
    TgBatchArgs b;
    memset(&b, 0, sizeof(b));
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
    b.h = h;
    b.w = w;
    const size_t nmap = (size_t)G * h * w;
    hipLaunchKernelGGL(train_gt_softmax_kernel, dim3((unsigned)((nmap + 255) / 256)), dim3(256), 0, stream, scores, workspace, G, C,
                       h * w);
    DSRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_gt_zoom_kernel, dim3((unsigned)b.blk0[G]), dim3(kTgThreads), 0, stream, b, G, C, eps, ignore_below);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
