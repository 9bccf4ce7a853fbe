// The training batches of both stages, assembled on the device from ONE staging buffer of raw bytes that the host fills and
// uploads with a single copy per batch: the training-side sibling of preprocess_rect_batch_kernel.  Per-image descriptors (byte
// offsets into the staging buffer, sizes, counts) ride by value in the argument block, at most 32 images (~1 KB).
//
// train_s_input_kernel (stage 1): Caffe's ImageData layer (train-s.prototxt:3-22: read, cv::resize to S x S, mean) followed by
// AnnotationLayer (pylayers.py:346-387).  One launch, two block ranges:
//   blocks [0, cue0): one thread owns one output pixel of one image (its three channels).  The resize is the 8-bit bilinear
//     resize stated in DESIGN.md (a restatement of OpenCV's INTER_LINEAR path for 8-bit images: coordinates through double, the
//     fraction in float, weights rounded half-even to 11 bits, horizontal pass in int32, vertical pass with the >> 4, >> 16, + 2,
//     >> 2 sequence), then RGB -> BGR, then float(pixel) - mean[c].  All of it is integer arithmetic up to the last subtraction,
//     so the result is exact or wrong.  KNOWN, ACCEPTED DEVIATION: OpenCV runs an exact 2x shrink (source = 2S on both axes) as
//     area averaging; this kernel blends bilinearly there as everywhere else.
//   blocks [cue0, cue0 + B*C): one workgroup owns one (image, class) plane of the cues: it zeroes the plane, passes a barrier,
//     then walks the image's K (class, row, column) int32 triplets and writes 1.0 for those of its class; thread 0 writes the
//     image-level label of the class (1.0 for class 0 and for the listed ids).  A triplet outside the planes writes nothing.
//   One flag per image reverses the last axis of its pixels and cue planes (pylayers.py:384-387) by writing to the mirrored column.
//
// train_f_input_kernel (stage 2): data.SimpleTransformer.preprocess (layer.py:169-236) for B images: one thread owns one pixel of
// one crop: (float(px) - mean[c]) * scale in BGR order (two separately rounded f32 operations) where the crop lies on the image and
// 0.0 off it; the label byte as float, ignore_label off the image; the mirror reverses both along x.
//
// train_f_input_scaled_kernel (stage 2 with `scale_factors`): the same crop taken from image b rescaled to Hs_b x Ws_b, a size the
// host computes (data.scaled_size); the rescaled image never exists in memory.  The thread of crop pixel (y, x) stands at
// (top + y, left + x) on the SCALED image and computes its own taps: the pixel by the 8-bit bilinear resize above with (n, S) =
// (W, Ws) on x and (H, Hs) on y — four clamped loads per channel — and the label by nearest neighbour, src = min((int)floor(d *
// scale), n - 1) with the resize's own double `scale` per axis (cv::resize INTER_NEAREST).  Then mean, scale, border values and
// mirror as in train_f_input_kernel.  Hs = H, Ws = W reproduces train_f_input_kernel bit for bit.  The two scales of an image ride
// in the argument block beside Hs and Ws (the launcher divides once per image; the threads would each divide four times).
//
// train_s_cuemap_input_kernel (stage 1 fed by cue MAPS): AnnotationLayerCOCO (pylayers.py:432-512) for B images: per image an
// (H, W, 3) RGB image and an (Hm, Wm) map of cue bytes, `ignore_label` = no cue.  One launch, three block ranges:
//   blocks [0, cue0): one thread owns one output pixel of one image (its three channels): the order-1 align-corners zoom of
//     preprocess_rect_batch_kernel to Sh x Sw (zoom_taps / zoom_blend of common.h, the code that kernel runs; the two scales of
//     an image are divided once by the launcher and ride in the argument block), minus the mean in f32.  Output channel c reads
//     source byte 2 - c with `bgr` (what every other pipeline of this project feeds the net) and byte c without (the layer's
//     own order).
//   blocks [cue0, lab0): one thread owns one map pixel of one image: it loads the byte v and walks the C planes, storing 1.0 to
//     plane v and 0.0 to the others (all 0.0 where v == ignore_label or v >= C), so a wave's stores run along x within a plane.
//   blocks [lab0, lab0 + B): one workgroup owns the image-level labels of one image: C flags in LDS, cleared, barrier, set by
//     plain same-value stores for every kept byte of the map, barrier, written out as C floats.  Class 0 is not forced on.
//   The mirror flag writes pixels and cue planes to the mirrored column; the labels do not depend on it.
//
// All: loads are issued unconditionally on clamped indices and selected afterwards; no atomics, no scratch, no dependence on the
// order of workgroups (every output element has exactly one owner; duplicate cue triplets write the same value behind the owner's
// barrier); LDS only for the C label flags of the cue-map kernel; -ffp-contract=off (Makefile).  Results are bit-reproducible.
#include "common.h"
#include "train_input_check.h"

namespace dsrg {

constexpr int kTiThreads = 256;

// source coordinates per output coordinate on an axis of n source and S output samples.  Two IEEE double divisions: the same bits
// from the host and from the device
__host__ __device__ __forceinline__ double axis_scale(int n, int S) { return 1.0 / ((double)S / (double)n); }

// source index and the two 11-bit weights of output coordinate d on an axis of n source samples and scale axis_scale(n, S);
// `zero_at_border`: the x axis' rule (fraction zeroed where the index is clamped), the y axis keeps its fraction and clamps the
// two rows instead
__device__ __forceinline__ void resize_tap(int d, int n, double scale, bool zero_at_border, int &s, int &w0, int &w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (zero_at_border) {
        if (s < 0) { s = 0; f = 0.0f; }
        if (s >= n - 1) { s = n - 1; f = 0.0f; }
    }
    const int r1 = (int)rintf(f * 2048.0f), r0 = (int)rintf((1.0f - f) * 2048.0f);        // round half even; saturate to int16
    w1 = min(max(r1, -32768), 32767);
    w0 = min(max(r0, -32768), 32767);
}

// nearest-neighbour source index of output coordinate d on the same axis, from the same scale (d >= 0, so the index is >= 0)
__device__ __forceinline__ int nearest_tap(int d, int n, double scale) { return min((int)floor((double)d * scale), n - 1); }

__global__ __launch_bounds__(kTiThreads) void train_s_input_kernel(const unsigned char *__restrict__ stage, TsArgs a, int B, int S, int C,
                                                                   int Hm, int Wm, int cue0, float *__restrict__ images,
                                                                   float *__restrict__ cues, float *__restrict__ labels) {
    const int blk = (int)blockIdx.x;
    if (blk < cue0) {                                                                       // (uniform over the block)
        const int SS = S * S;
        const int idx = blk * kTiThreads + (int)threadIdx.x;                                // (image, y, x) flattened: < B * S * S < 2^31 / 3
        if (idx >= B * SS) return;
        const int b = idx / SS, r = idx - b * SS;
        const int y = r / S, x = r - y * S;
        const int H = a.H[b], W = a.W[b];
        int sx, a0, a1, sy, b0, b1;
        resize_tap(x, W, axis_scale(W, S), true, sx, a0, a1);
        resize_tap(y, H, axis_scale(H, S), false, sy, b0, b1);
        const int x0 = sx, x1 = min(sx + 1, W - 1);
        const int y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
        const unsigned char *im = stage + a.img_off[b];
        const unsigned char *p00 = im + ((size_t)y0 * W + x0) * 3, *p01 = im + ((size_t)y0 * W + x1) * 3;
        const unsigned char *p10 = im + ((size_t)y1 * W + x0) * 3, *p11 = im + ((size_t)y1 * W + x1) * 3;
        const int xo = ((a.mirror >> b) & 1u) ? S - 1 - x : x;
        float *o = images + (size_t)b * 3 * SS + (size_t)y * S + xo;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                                       // output channel c = input channel 2 - c (BGR)
            const int D0 = (int)p00[2 - c] * a0 + (int)p01[2 - c] * a1;
            const int D1 = (int)p10[2 - c] * a0 + (int)p11[2 - c] * a1;
            const int v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2;
            o[c * SS] = (float)v - a.mean[c];
        }
        return;
    }
    const int plane = blk - cue0;                                                           // < B * C
    const int b = plane / C, c = plane - b * C;
    const int HW = Hm * Wm, tid = (int)threadIdx.x;
    float *p = cues + (size_t)plane * HW;
    for (int i = tid; i < HW; i += kTiThreads) p[i] = 0.0f;
    __syncthreads();                                                                        // the plane's zeros are complete before its ones
    const int K = a.ncue[b];
    const int *t = reinterpret_cast<const int *>(stage + a.cue_off[b]);
    const bool mir = (a.mirror >> b) & 1u;
    for (int k = tid; k < K; k += kTiThreads) {
        const int cls = t[k], yy = t[K + k], xx = t[2 * K + k];
        if (cls == c && yy >= 0 && yy < Hm && xx >= 0 && xx < Wm) p[yy * Wm + (mir ? Wm - 1 - xx : xx)] = 1.0f;
    }
    if (tid == 0) {
        const int L = a.nlab[b];
        const int *l = reinterpret_cast<const int *>(stage + a.lab_off[b]);
        bool present = c == 0;
        for (int k = 0; k < L; ++k) present = present || l[k] == c;
        labels[plane] = present ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(kTiThreads) void train_f_input_kernel(const unsigned char *__restrict__ stage, TfArgs a, int B, int ch, int cw,
                                                                   float *__restrict__ data, float *__restrict__ label) {
    const int P = ch * cw;
    const int idx = (int)blockIdx.x * kTiThreads + (int)threadIdx.x;                        // (image, y, x) flattened: < B * ch * cw < 2^31 / 3
    if (idx >= B * P) return;
    const int b = idx / P, r = idx - b * P;
    const int y = r / cw, x = r - y * cw;
    const int H = a.H[b], W = a.W[b];
    const int sy = a.top[b] + y, sx = a.left[b] + x;                                       // on the extended image (top, left >= 0)
    const bool on = sy < H && sx < W;
    const size_t src = (size_t)min(sy, H - 1) * W + min(sx, W - 1);                        // clamped: the loads below are unconditional
    const unsigned char *px = stage + a.img_off[b] + src * 3;
    const float lab = (float)stage[(size_t)a.lab_off[b] + src];
    const int xo = ((a.mirror >> b) & 1u) ? cw - 1 - x : x;
    const size_t at = (size_t)y * cw + xo;
    float *o = data + (size_t)b * 3 * P + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                                           // output channel c = input channel 2 - c (BGR)
        const float v = ((float)px[2 - c] - a.mean[c]) * a.scale;
        o[c * P] = on ? v : 0.0f;
    }
    label[(size_t)b * P + at] = on ? lab : a.ignore_label;
}

__global__ __launch_bounds__(kTiThreads) void train_f_input_scaled_kernel(const unsigned char *__restrict__ stage, TfScaledArgs sa, int B,
                                                                          int ch, int cw, float *__restrict__ data,
                                                                          float *__restrict__ label) {
    const TfArgs &a = sa.f;
    const int P = ch * cw;
    const int idx = (int)blockIdx.x * kTiThreads + (int)threadIdx.x;                        // (image, y, x) flattened: < B * ch * cw < 2^31 / 3
    if (idx >= B * P) return;
    const int b = idx / P, r = idx - b * P;
    const int y = r / cw, x = r - y * cw;
    const int H = a.H[b], W = a.W[b], Hs = sa.Hs[b], Ws = sa.Ws[b];
    const int sy = a.top[b] + y, sx = a.left[b] + x;                                       // on the extended SCALED image (top, left >= 0)
    const bool on = sy < Hs && sx < Ws;
    const int dy = min(sy, Hs - 1), dx = min(sx, Ws - 1);                                  // clamped: taps and loads below are unconditional
    const double ys = sa.ys[b], xs = sa.xs[b];
    int tx, a0, a1, ty, b0, b1;
    resize_tap(dx, W, xs, true, tx, a0, a1);
    resize_tap(dy, H, ys, false, ty, b0, b1);
    const int x0 = tx, x1 = min(tx + 1, W - 1);                                            // all four inside [0, W) x [0, H)
    const int y0 = min(max(ty, 0), H - 1), y1 = min(max(ty + 1, 0), H - 1);
    const unsigned char *im = stage + a.img_off[b];
    const unsigned char *p00 = im + ((size_t)y0 * W + x0) * 3, *p01 = im + ((size_t)y0 * W + x1) * 3;
    const unsigned char *p10 = im + ((size_t)y1 * W + x0) * 3, *p11 = im + ((size_t)y1 * W + x1) * 3;
    const float lab = (float)stage[(size_t)a.lab_off[b] + (size_t)nearest_tap(dy, H, ys) * W + nearest_tap(dx, W, xs)];
    const int xo = ((a.mirror >> b) & 1u) ? cw - 1 - x : x;
    const size_t at = (size_t)y * cw + xo;
    float *o = data + (size_t)b * 3 * P + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                                           // output channel c = input channel 2 - c (BGR)
        const int D0 = (int)p00[2 - c] * a0 + (int)p01[2 - c] * a1;
        const int D1 = (int)p10[2 - c] * a0 + (int)p11[2 - c] * a1;
        const int px = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2;
        const float v = ((float)px - a.mean[c]) * a.scale;
        o[c * P] = on ? v : 0.0f;
    }
    label[(size_t)b * P + at] = on ? lab : a.ignore_label;
}

__global__ __launch_bounds__(kTiThreads) void train_s_cuemap_input_kernel(const unsigned char *__restrict__ stage, TcArgs a, int B, int Sh,
                                                                          int Sw, int C, int Hm, int Wm, int ignore_label, int bgr,
                                                                          int cue0, int lab0, float *__restrict__ images,
                                                                          float *__restrict__ cues, float *__restrict__ labels) {
    __shared__ int present[kMaxLabels];
    const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int HW = Hm * Wm;
    if (blk < cue0) {                                                                       // (uniform over the block)
        const int SS = Sh * Sw;
        const int idx = blk * kTiThreads + tid;                                             // (image, y, x) flattened: < B * Sh * Sw < 2^31 / 3
        if (idx >= B * SS) return;
        const int b = idx / SS, r = idx - b * SS;
        const int y = r / Sw, x = r - y * Sw;
        ZoomTaps t = zoom_taps(a.H[b], a.W[b], a.sh[b], a.sw[b], y, x);
        zoom_point(t, stage + a.img_off[b], a.W[b]);
        const int xo = ((a.mirror >> b) & 1u) ? Sw - 1 - x : x;
        float *o = images + (size_t)b * 3 * SS + (size_t)y * Sw + xo;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * SS] = zoom_blend(t, bgr ? 2 - c : c) - a.mean[c];
        return;
    }
    if (blk < lab0) {
        const int idx = (blk - cue0) * kTiThreads + tid;                                    // (image, y, x) flattened: < B * Hm * Wm
        if (idx >= B * HW) return;
        const int b = idx / HW, r = idx - b * HW;
        const int y = r / Wm, x = r - y * Wm;
        const int v = (int)stage[(size_t)a.cue_off[b] + r];
        const int own = (v != ignore_label && v < C) ? v : -1;                              // the plane that takes this pixel's 1.0
        const int xo = ((a.mirror >> b) & 1u) ? Wm - 1 - x : x;
        float *o = cues + (size_t)b * C * HW + (size_t)y * Wm + xo;
        for (int c = 0; c < C; ++c) o[(size_t)c * HW] = c == own ? 1.0f : 0.0f;
        return;
    }
    const int b = blk - lab0;                                                               // < B
    for (int c = tid; c < C; c += kTiThreads) present[c] = 0;                               // (C <= kMaxLabels: checked by the launcher)
    __syncthreads();
    const unsigned char *m = stage + a.cue_off[b];
    for (int i = tid; i < HW; i += kTiThreads) {
        const int v = (int)m[i];
        if (v != ignore_label && v < C) present[v] = 1;                                     // same-value stores: any order gives the same flags
    }
    __syncthreads();
    for (int c = tid; c < C; c += kTiThreads) labels[(size_t)b * C + c] = present[c] ? 1.0f : 0.0f;
}

int launch_train_s_input_batch(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *H,
                               const int32_t *W, const int32_t *cue_off, const int32_t *ncues, const int32_t *label_off,
                               const int32_t *nlabels, const int32_t *mirror, int S, int C, int Hm, int Wm, const float *mean,
                               float *images, float *cues, float *labels, hipStream_t stream) {
    TsArgs a;
    if (int rc = check_train_s_input(B, stage, stage_bytes, image_off, H, W, cue_off, ncues, label_off, nlabels, mirror, S, C, Hm, Wm, mean,
                                     images, cues, labels, a)) return rc;
    const int cue0 = (int)(((long long)B * S * S + kTiThreads - 1) / kTiThreads);            // < 2^23
    const long long blocks = (long long)cue0 + (long long)B * C;                             // B * C < 2^31 / (Hm * Wm)
    if (blocks >= (1LL << 24))                                                               // a grid holds < 2^32 threads
        return set_error(DSRG_ERR_UNSUPPORTED, "train-s input: %lld workgroups >= 2^24 (pixel blocks + B * C planes)", blocks);
    hipLaunchKernelGGL(train_s_input_kernel, dim3((unsigned)blocks), dim3(kTiThreads), 0, stream, stage, a, B, S, C, Hm, Wm, cue0, images,
                       cues, labels);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_train_s_cuemap_input_batch(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *H,
                                      const int32_t *W, const int32_t *cue_off, const int32_t *mirror, int Sh, int Sw, int C, int Hm,
                                      int Wm, const float *mean, int ignore_label, int bgr, float *images, float *cues, float *labels,
                                      hipStream_t stream) {
    TcArgs a;
    if (int rc = check_train_s_cuemap_input(B, stage, stage_bytes, image_off, H, W, cue_off, mirror, Sh, Sw, C, kMaxLabels, Hm, Wm, mean,
                                            ignore_label, bgr, images, cues, labels, a)) return rc;
    for (int b = 0; b < B; ++b) a.sh[b] = zoom_axis_scale(H[b], Sh), a.sw[b] = zoom_axis_scale(W[b], Sw);
    const int cue0 = (int)(((long long)B * Sh * Sw + kTiThreads - 1) / kTiThreads);          // < 2^23
    const int lab0 = cue0 + (int)(((long long)B * Hm * Wm + kTiThreads - 1) / kTiThreads);   // < 2^24
    hipLaunchKernelGGL(train_s_cuemap_input_kernel, dim3((unsigned)(lab0 + B)), dim3(kTiThreads), 0, stream, stage, a, B, Sh, Sw, C, Hm, Wm,
                       ignore_label, bgr, cue0, lab0, images, cues, labels);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_train_f_input_batch(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *label_off,
                               const int32_t *H, const int32_t *W, const int32_t *top, const int32_t *left, const int32_t *mirror,
                               int ch, int cw, const float *mean, float scale, float ignore_label, float *data, float *label,
                               hipStream_t stream) {
    TfArgs a;
    if (int rc = check_train_f_input(B, stage, stage_bytes, image_off, label_off, H, W, NULL, NULL, top, left, mirror, ch, cw, mean, scale,
                                     ignore_label, data, label, a, NULL)) return rc;
    const unsigned blocks = (unsigned)(((long long)B * ch * cw + kTiThreads - 1) / kTiThreads);
    hipLaunchKernelGGL(train_f_input_kernel, dim3(blocks), dim3(kTiThreads), 0, stream, stage, a, B, ch, cw, data, label);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_train_f_input_scaled_batch(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off,
                                      const int32_t *label_off, const int32_t *H, const int32_t *W, const int32_t *Hs, const int32_t *Ws,
                                      const int32_t *top, const int32_t *left, const int32_t *mirror, int ch, int cw, const float *mean,
                                      float scale, float ignore_label, float *data, float *label, hipStream_t stream) {
    TfScaledArgs sa;
    if (int rc = check_train_f_input(B, stage, stage_bytes, image_off, label_off, H, W, Hs, Ws, top, left, mirror, ch, cw, mean, scale,
                                     ignore_label, data, label, sa.f, &sa)) return rc;
    for (int b = 0; b < B; ++b) sa.ys[b] = axis_scale(H[b], Hs[b]), sa.xs[b] = axis_scale(W[b], Ws[b]);
    const unsigned blocks = (unsigned)(((long long)B * ch * cw + kTiThreads - 1) / kTiThreads);
    hipLaunchKernelGGL(train_f_input_scaled_kernel, dim3(blocks), dim3(kTiThreads), 0, stream, stage, sa, B, ch, cw, data, label);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
