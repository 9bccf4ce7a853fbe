// Validation scoring in one launch: a batch of score maps and its full-resolution label maps -> confusion counters.
//
// For every pixel (b, y, x) of B label maps (B, 1, Hz, Wz) — what dsrg_train_f_input_batch writes: the label byte as a float on the
// image, ignore_label off it — whose label passes the keep rule (rule_lt = 0: label != ignore_label, ConfusionMatrix.add;
// rule_lt = 1: label < C, generateM), the prediction is the first maximum over labels of slice b of the (>= B, C, h, w) scores
// zoomed to Hz x Wz, and hist[label * C + pred] += 1 (hist[C * C] for a kept label that is not one of 0..C-1).
//
// The zoom is multiscale.hip's at K = 1, operation for operation (so `pred` is what dsrg_multiscale_unary writes to argmax_dev):
//   scale = (in - 1) / (out - 1) in double on the host (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
//   l1 = src - i0, l0 = 1 - l1, v = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11) in double, rounded once to f32
// (-ffp-contract=off: every product and sum rounded on its own), strict > while walking the labels upwards.
//
// One grid covers the batch.  The B * Hz * Wz pixels are numbered through (image, then y * Wz + x); a workgroup of 256 lanes takes
// runs of 256 consecutive pixels, a lane one pixel of each (coalesced label reads), the runs gridDim.x apart: the grid is capped at
// kEvalMaxBlocks workgroups, so however many pixels there are, at most that many LDS histograms are added to the global counters
// (with a histogram of its own for every 256 pixels the launch took half as long again at 10 x 513 x 513).  A lane reads its label
// first; one that is dropped loads no score, and a wave none of whose labels is kept — the padded border of every image — skips
// the scores altogether.  Taps and weights are computed once per pixel in registers, the C planes are walked with a running first
// maximum (no LDS tile, no exp: only the argmax is wanted), counts go to an LDS histogram of C * C + 1 32-bit counters (a
// workgroup adds fewer than 2^31 in all) and at the end its non-zero counters to the 64-bit global ones.  Nothing but the counters
// is written.  Integer counters: the result does not depend on the order in which lanes or workgroups add.
#include "common.h"

namespace dsrg {

constexpr int kEvalThreads = 256;
constexpr int kEvalMaxBlocks = 1024;
constexpr int kEvalMaxBatch = 32;

__global__ __launch_bounds__(kEvalThreads) void eval_confusion_batch_kernel(int B, int C, const float *__restrict__ scores, int h, int w,
                                                                            double sh, double sw,
                                                                            const float *__restrict__ labels, int Hz, int Wz,
                                                                            float ignore_label, int rule_lt,
                                                                            unsigned long long *__restrict__ hist) {
    extern __shared__ unsigned int s_hist[];                  // [C * C + 1]
    const int nb = C * C + 1;
    const int tid = threadIdx.x;
    for (int i = tid; i < nb; i += kEvalThreads) s_hist[i] = 0u;
    __syncthreads();

    const unsigned N = (unsigned)(Hz * Wz), total = (unsigned)B * N;      // (< 2^31: p + stride below stays inside 32 bits)
    const unsigned stride = gridDim.x * kEvalThreads;
    const int hw = h * w;
#pragma unroll 1
    for (unsigned p = blockIdx.x * kEvalThreads + tid; p < total; p += stride) {
        const float l = labels[p];
        if (!(rule_lt ? l < (float)C : l != ignore_label)) continue;
        int g = -1;                                           // the row, or -1: a kept label that is not one of 0..C-1
        if (l >= 0.0f && l < (float)C) {
            const int gi = (int)l;
            if ((float)gi == l) g = gi;
        }
        if (g < 0) {
            atomicAdd(&s_hist[nb - 1], 1u);
            continue;
        }
        // taps and weights of this pixel (multiscale_unary_body, step 1)
        const unsigned b = p / N;
        const int i = (int)(p - b * N);
        const int y = i / Wz, x = i - y * Wz;
        const double sy = sh * (double)y, sx = sw * (double)x;
        const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);      // (the min never binds: src <= in - 1)
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
        const double l1h = sy - (double)y0, l1w = sx - (double)x0;
        const double l0h = 1.0 - l1h, l0w = 1.0 - l1w;
        // the first maximum over the labels
        const float *sc_b = scores + (size_t)b * C * hw;
        float m = 0.0f;
        int arg = 0;
#pragma unroll 2
        for (int c = 0; c < C; ++c) {
            const float *plane = sc_b + (size_t)c * hw;
            const double v00 = plane[o00], v01 = plane[o01], v10 = plane[o10], v11 = plane[o11];
            const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
            if (c == 0 || z > m) { m = z; arg = c; }
        }
        atomicAdd(&s_hist[g * C + arg], 1u);
    }
    __syncthreads();

    // the workgroup's non-zero counters out
    for (int i = tid; i < nb; i += kEvalThreads) {
        const unsigned int v = s_hist[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

int launch_eval_confusion_batch(int B, int C, const float *scores, int h, int w, const float *labels, int Hz, int Wz,
                                float ignore_label, int rule_lt, unsigned long long *hist, hipStream_t stream) {
    if (!scores || !labels || !hist) return set_error(DSRG_ERR_INVALID, "eval confusion batch: NULL scores / labels / hist");
    if (B < 1 || B > kEvalMaxBatch) return set_error(DSRG_ERR_INVALID, "eval confusion batch: 1..%d images, got %d", kEvalMaxBatch, B);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "eval confusion batch: %d labels", C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_UNSUPPORTED, "eval confusion batch: at most %d labels, got %d", kMaxLabels, C);
    if (h < 1 || w < 1 || Hz < 1 || Wz < 1)
        return set_error(DSRG_ERR_INVALID, "eval confusion batch: score maps %dx%d, label maps %dx%d", h, w, Hz, Wz);
    // (each factor is < 2^31 and B * C <= 3072: the running products below stay far inside 64 bits)
    if ((long long)B * C * h >= (1LL << 31) || (long long)B * C * h * w >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "eval confusion batch: B*C*h*w >= 2^31");
    if ((long long)B * Hz >= (1LL << 31) || (long long)B * Hz * Wz >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "eval confusion batch: B*Hz*Wz >= 2^31");
    const double sh = Hz > 1 ? (double)(h - 1) / (double)(Hz - 1) : 0.0;
    const double sw = Wz > 1 ? (double)(w - 1) / (double)(Wz - 1) : 0.0;
    const long long runs = ((long long)B * Hz * Wz + kEvalThreads - 1) / kEvalThreads;
    const unsigned grid = (unsigned)(runs < kEvalMaxBlocks ? runs : kEvalMaxBlocks);
    const size_t lds = ((size_t)C * C + 1) * sizeof(unsigned int);         // <= 36 868 B: inside the default dynamic-LDS limit
    hipLaunchKernelGGL(eval_confusion_batch_kernel, dim3(grid), dim3(kEvalThreads), lds, stream, B, C, scores, h, w, sh, sw, labels, Hz,
                       Wz, ignore_label, rule_lt, hist);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// ---- scoring finished label maps: a group of differently sized int32 label maps and their uint8 ground truth -> the same counters
//
// The label maps are what the dense CRF's map and the arg-max outputs of the multi-scale / pseudo-label tails leave on the device.
// The G images' pixels are numbered through the group (image g holds pixels off[g] .. off[g + 1]); the grid, the runs of 256
// consecutive pixels, the LDS histogram and the way it is added to the global counters are eval_confusion_batch_kernel's.  A run may
// straddle images: a lane finds its image by walking the prefix offsets upwards (its pixels only ever increase), and the reads of
// either side of a seam are still consecutive.  A lane reads its ground-truth byte first; one that is dropped loads no label — and a
// wave none of whose bytes is kept issues no label load — unless masks are wanted: then every pixel's label is read and written back
// as a byte, 255 standing for everything outside 0..255 (what astype(uint8) gives the label maps the project produces, whose only
// value outside 0..C-1 is the 255 of ignore_below).
constexpr int kScoreMaxGroup = 16;

struct ScoreLabelsArgs {
    const int32_t *labels[kScoreMaxGroup];
    const unsigned char *gt[kScoreMaxGroup];
    unsigned char *mask[kScoreMaxGroup];                      // all NULL: no masks wanted
    unsigned off[kScoreMaxGroup + 1];                         // off[G] = the group's pixels (< 2^31)
};

__global__ __launch_bounds__(kEvalThreads) void score_labels_batch_kernel(ScoreLabelsArgs a, int G, int C, int ignore_label, int rule_lt,
                                                                          int want_mask, unsigned long long *__restrict__ hist) {
    extern __shared__ unsigned int s_hist[];                  // [C * C + 1]
    const int nb = C * C + 1;
    const int tid = threadIdx.x;
    for (int i = tid; i < nb; i += kEvalThreads) s_hist[i] = 0u;
    __syncthreads();

    const unsigned total = a.off[G];                          // (< 2^31: p + stride below stays inside 32 bits)
    const unsigned stride = gridDim.x * kEvalThreads;
    int g = 0;
#pragma unroll 1
    for (unsigned p = blockIdx.x * kEvalThreads + tid; p < total; p += stride) {
        while (g + 1 < G && p >= a.off[g + 1]) ++g;
        const unsigned i = p - a.off[g];
        const int t = (int)a.gt[g][i];
        const bool keep = rule_lt ? t < C : t != ignore_label;
        if (!keep && !want_mask) continue;
        const int l = a.labels[g][i];
        if (want_mask) a.mask[g][i] = (unsigned char)((unsigned)l <= 255u ? l : 255);
        if (!keep) continue;
        const bool in_range = t < C && (unsigned)l < (unsigned)C;
        atomicAdd(&s_hist[in_range ? t * C + l : nb - 1], 1u);
    }
    __syncthreads();

    // the workgroup's non-zero counters out
    for (int i = tid; i < nb; i += kEvalThreads) {
        const unsigned int v = s_hist[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

int launch_score_labels_batch(int G, int C, const int32_t *const *labels, const unsigned char *const *gt, const int32_t *H,
                              const int32_t *W, int ignore_label, int rule_lt, unsigned long long *hist, unsigned char *const *mask,
                              hipStream_t stream) {
    if (!labels || !gt || !hist || !H || !W)
        return set_error(DSRG_ERR_INVALID, "score labels batch: NULL labels / gt / hist / size array");
    if (G < 1 || G > kScoreMaxGroup) return set_error(DSRG_ERR_INVALID, "score labels batch: 1..%d images, got %d", kScoreMaxGroup, G);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "score labels batch: %d labels", C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_UNSUPPORTED, "score labels batch: at most %d labels, got %d", kMaxLabels, C);
    ScoreLabelsArgs a = {};
    long long total = 0;
    for (int g = 0; g < G; ++g) {
        if (!labels[g] || !gt[g] || (mask && !mask[g]))
            return set_error(DSRG_ERR_INVALID, "score labels batch: image %d has a NULL label map, ground truth or mask", g);
        if (H[g] < 1 || W[g] < 1) return set_error(DSRG_ERR_INVALID, "score labels batch: image %d is %dx%d", g, H[g], W[g]);
        total += (long long)H[g] * W[g];                      // (each product < 2^62, checked before the next is added)
        if (total >= (1LL << 31)) return set_error(DSRG_ERR_INVALID, "score labels batch: the group holds >= 2^31 pixels");
        a.labels[g] = labels[g];
        a.gt[g] = gt[g];
        a.mask[g] = mask ? mask[g] : nullptr;
        a.off[g + 1] = (unsigned)total;
    }
    for (int g = G + 1; g <= kScoreMaxGroup; ++g) a.off[g] = (unsigned)total;
    const long long runs = (total + kEvalThreads - 1) / kEvalThreads;
    const unsigned grid = (unsigned)(runs < kEvalMaxBlocks ? runs : kEvalMaxBlocks);
    const size_t lds = ((size_t)C * C + 1) * sizeof(unsigned int);         // <= 36 868 B: inside the default dynamic-LDS limit
    hipLaunchKernelGGL(score_labels_batch_kernel, dim3(grid), dim3(kEvalThreads), lds, stream, a, G, C, ignore_label, rule_lt,
                       mask ? 1 : 0, hist);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
