// Every network input of a group of test images in one launch: inference.preprocess (test-ms.py:68-81) for G images at K sizes, and
// inference.preprocess_relative (test-ms-f.py:100-112) for G same-sized images at K relative scales.
// Image g, (H_g, W_g, 3) RGB uint8, is zoomed to h_k x w_k for every k, reordered to BGR and has the mean subtracted; the results
// are the slots g of K (Gcap, 3, h_k, w_k) f32 NCHW tensors: the batched inputs of the K forwards.  Slots g >= G are written as
// zeros, so a padded tail group is deterministic.  dsrg_preprocess_ms_batch is the square case h_k = w_k = S_k of
// dsrg_preprocess_rect_batch: one kernel and one launcher serve both.
//
// One thread owns one output pixel (its three channels) of one (scale, slot); blockIdx.x -> scale through per-scale block prefix
// sums.  The zoom is the order-1 align-corners zoom stated at the top of multiscale.hip (torch's upsample_bilinear2d on float64
// input, which is what inference._zoom runs): coordinate y * (H-1)/(h-1) (0 when h == 1; likewise x) and the two-tap blend
// l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11) in double, rounded once to f32; then the f32 subtraction of the
// mean.  At h_k == H_g and w_k == W_g the scale is 1, the weights are 1 and 0, and the pixel comes through exactly.  The four
// taps are loaded unconditionally from clamped indices.
// -ffp-contract=off (Makefile) keeps every product and sum rounded on its own.  No atomics: results are bit-reproducible.
//
// dsrg_preprocess_rect_mirror_batch (mirrored test-time augmentation) is preprocess_rect_mirror_batch_kernel: image g owns the slot
// pair (2 g, 2 g + 1), and the thread of output pixel (y, x) stores each of its three values twice, at column x of slot 2 g and
// at column w - 1 - x of slot 2 g + 1.  So slot 2 g is what the plain kernel writes for image g and slot 2 g + 1 is that tensor
// with its last axis reversed (the mirrored network input, not a second zoom of a mirrored image); slots 2 G.. are zeros.
#include <string.h>
#include "common.h"

namespace dsrg {

constexpr int kPpThreads = 256;
constexpr int kPpMaxScales = 8;
constexpr int kPpMaxBatch = 16;
constexpr int kPpMaxMirrorBatch = 8;  // images of the mirror form: two slots each

struct PpArgs {
    const unsigned char *im[kPpMaxBatch];
    int H[kPpMaxBatch], W[kPpMaxBatch];
    float *out[kPpMaxScales];
    int h[kPpMaxScales], w[kPpMaxScales];
    int blk0[kPpMaxScales + 1];       // first block of scale k (blk0[K] = the grid)
    float mean[3];                    // of the OUTPUT channels (B, G, R)
};

__global__ __launch_bounds__(kPpThreads) void preprocess_rect_batch_kernel(PpArgs a, int G, int Gcap, int K) {
    const int blk = (int)blockIdx.x;
    int k = 0;
    while (k + 1 < K && blk >= a.blk0[k + 1]) ++k;          // (uniform over the block)
    const int h = a.h[k], w = a.w[k], hw = h * w;
    const int idx = (blk - a.blk0[k]) * kPpThreads + (int)threadIdx.x;    // (slot, y, x) flattened: < Gcap * h * w < 2^31 / 3
    if (idx >= Gcap * hw) return;
    const int g = idx / hw, r = idx - g * hw;
    const int y = r / w, x = r - y * w;
    float *o = a.out[k] + (size_t)g * 3 * hw + r;
    if (g >= G) {
        o[0] = 0.0f;
        o[hw] = 0.0f;
        o[2 * hw] = 0.0f;
        return;
    }
    const int H = a.H[g], W = a.W[g];
    ZoomTaps t = zoom_taps(H, W, zoom_axis_scale(H, h), zoom_axis_scale(W, w), y, x);    // (common.h)
    zoom_point(t, a.im[g], W);
#pragma unroll
    for (int c = 0; c < 3; ++c)                             // output channel c = input channel 2 - c (BGR)
        o[c * hw] = zoom_blend(t, 2 - c) - a.mean[c];
}

// The mirror form.  The index space is (image or zero slot, y, x) with Gcap - G entries on its first axis: the G images (entry g
// -> slots 2 g and 2 g + 1), then the Gcap - 2 G zero slots behind the pairs (entry g -> slot g + G).  The arithmetic is the
// statements of preprocess_rect_batch_kernel, kept as a kernel of its own: sharing a body moved an operand order in that kernel's
// instructions, and it is to stay the code it was.
__global__ __launch_bounds__(kPpThreads) void preprocess_rect_mirror_batch_kernel(PpArgs a, int G, int Gcap, int K) {
    const int blk = (int)blockIdx.x;
    int k = 0;
    while (k + 1 < K && blk >= a.blk0[k + 1]) ++k;          // (uniform over the block)
    const int h = a.h[k], w = a.w[k], hw = h * w;
    const int idx = (blk - a.blk0[k]) * kPpThreads + (int)threadIdx.x;    // < (Gcap - G) * h * w < 2^31 / 3
    if (idx >= (Gcap - G) * hw) return;
    const int g = idx / hw, r = idx - g * hw;
    const int y = r / w, x = r - y * w;
    if (g >= G) {
        float *o = a.out[k] + (size_t)(g + G) * 3 * hw + r;
        o[0] = 0.0f;
        o[hw] = 0.0f;
        o[2 * hw] = 0.0f;
        return;
    }
    float *o = a.out[k] + (size_t)(2 * g) * 3 * hw + r;     // slot 2 g, (y, x)
    float *om = o + 3 * hw + (w - 1 - 2 * x);               // slot 2 g + 1, (y, w - 1 - x)
    const int H = a.H[g], W = a.W[g];
    const double sh = h > 1 ? (double)(H - 1) / (double)(h - 1) : 0.0;
    const double sw = w > 1 ? (double)(W - 1) / (double)(w - 1) : 0.0;
    const double sy = sh * (double)y, sx = sw * (double)x;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const double l1h = sy - (double)y0, l1w = sx - (double)x0;
    const double l0h = 1.0 - l1h, l0w = 1.0 - l1w;
    const unsigned char *im = a.im[g];
    const unsigned char *p00 = im + ((size_t)y0 * W + x0) * 3, *p01 = im + ((size_t)y0 * W + x1) * 3;
    const unsigned char *p10 = im + ((size_t)y1 * W + x0) * 3, *p11 = im + ((size_t)y1 * W + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                           // output channel c = input channel 2 - c (BGR)
        const double v00 = p00[2 - c], v01 = p01[2 - c], v10 = p10[2 - c], v11 = p11[2 - c];
        const float z = (float)(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11));
        const float v = z - a.mean[c];                      // computed once, stored twice
        o[c * hw] = v;
        om[c * hw] = v;
    }
}

// `what` names the entry point in the messages; oh / ow: the K target heights / widths (the same array for the square case);
// mirror: two slots per image (dsrg_preprocess_rect_mirror_batch)
static int launch_preprocess_batch(const char *what, bool mirror, int G, int Gcap, int K, const unsigned char *const *images, const int32_t *H,
                                   const int32_t *W, const int32_t *oh, const int32_t *ow, const float *mean, float *const *out,
                                   hipStream_t stream) {
    const int maxG = mirror ? kPpMaxMirrorBatch : kPpMaxBatch, per = mirror ? 2 : 1;
    if (G < 1 || G > maxG) return set_error(DSRG_ERR_INVALID, "%s: 1..%d images, got %d", what, maxG, G);
    if (K < 1 || K > kPpMaxScales) return set_error(DSRG_ERR_INVALID, "%s: 1..%d sizes, got %d", what, kPpMaxScales, K);
    if (Gcap < per * G)
        return set_error(DSRG_ERR_INVALID, "%s: capacity %d below the %d slots of %d images", what, Gcap, per * G, G);
    if (!images || !H || !W) return set_error(DSRG_ERR_INVALID, "%s: NULL image / image size array", what);
    if (!oh || !ow || !mean || !out) return set_error(DSRG_ERR_INVALID, "%s: NULL size / mean / output array", what);
    PpArgs a;
    memset(&a, 0, sizeof(a));
    for (int g = 0; g < G; ++g) {
        if (!images[g]) return set_error(DSRG_ERR_INVALID, "%s: image %d is NULL", what, g);
        if (H[g] < 1 || W[g] < 1) return set_error(DSRG_ERR_INVALID, "%s: image %d is %dx%d", what, g, H[g], W[g]);
        if ((long long)H[g] * W[g] * 3 >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "%s: image %d holds >= 2^31 values", what, g);
        a.im[g] = images[g];
        a.H[g] = H[g];
        a.W[g] = W[g];
    }
    long long blocks = 0;
    for (int k = 0; k < K; ++k) {
        if (oh[k] < 1 || ow[k] < 1) return set_error(DSRG_ERR_INVALID, "%s: size %d is %dx%d", what, k, oh[k], ow[k]);
        if (!out[k]) return set_error(DSRG_ERR_INVALID, "%s: output %d is NULL", what, k);
        if ((uintptr_t)out[k] & 3) return set_error(DSRG_ERR_INVALID, "%s: output %d is not aligned to a float", what, k);
        const long long n = (long long)Gcap * oh[k] * ow[k];
        if (n * 3 >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "%s: output %d holds %lld >= 2^31 values", what, k, n * 3);
        a.out[k] = out[k];
        a.h[k] = oh[k];
        a.w[k] = ow[k];
        a.blk0[k] = (int)blocks;
        const long long threads = (long long)(mirror ? Gcap - G : Gcap) * oh[k] * ow[k];    // (one per image pixel and zero-slot pixel)
        blocks += (threads + kPpThreads - 1) / kPpThreads;  // < 2^23 per scale
    }
    a.blk0[K] = (int)blocks;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c];
    if (mirror)
        hipLaunchKernelGGL(preprocess_rect_mirror_batch_kernel, dim3((unsigned)blocks), dim3(kPpThreads), 0, stream, a, G, Gcap, K);
    else
        hipLaunchKernelGGL(preprocess_rect_batch_kernel, dim3((unsigned)blocks), dim3(kPpThreads), 0, stream, a, G, Gcap, K);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_preprocess_ms_batch(int G, int Gcap, int K, const unsigned char *const *images, const int32_t *H, const int32_t *W,
                               const int32_t *sizes, const float *mean, float *const *out, hipStream_t stream) {
    return launch_preprocess_batch("preprocess batch", false, G, Gcap, K, images, H, W, sizes, sizes, mean, out, stream);
}

int launch_preprocess_rect_batch(int G, int Gcap, int K, const unsigned char *const *images, const int32_t *H, const int32_t *W,
                                 const int32_t *oh, const int32_t *ow, const float *mean, float *const *out, hipStream_t stream) {
    return launch_preprocess_batch("preprocess rect batch", false, G, Gcap, K, images, H, W, oh, ow, mean, out, stream);
}

int launch_preprocess_rect_mirror_batch(int G, int Gcap, int K, const unsigned char *const *images, const int32_t *H, const int32_t *W,
                                        const int32_t *oh, const int32_t *ow, const float *mean, float *const *out,
                                        hipStream_t stream) {
    return launch_preprocess_batch("preprocess rect mirror batch", true, G, Gcap, K, images, H, W, oh, ow, mean, out, stream);
}

}  // namespace dsrg
