// Multi-scale scores -> dense-CRF unary in one launch: the full-resolution tail of test-ms.py:90-103 / test-ms-f.py:121-134
// (zoom every scale's fc8 scores to the image, sum over scales, softmax over labels, clamp at eps, log), written label-fastest
// (H, W, C) as CRF_device takes it.
//
// One workgroup owns 64 consecutive output pixels (flattened y * W + x), i.e. 64 * C consecutive output floats.
//   1. per (pixel, scale): the two source rows / columns and the two blend weights, fp64, in the registers of the four lanes that
//      serve the pixel (the scale count is a template parameter: every scale's 4 loads per label are issued together)
//   2. per (pixel, label): z_k = f32(align-corners bilinear in fp64) summed in scale order in f32 -> LDS tile [64][C]
//   3. per pixel (4 lanes each): max, first arg-max, sum of exp(S - max)
//   4. the block's 64 * C floats written as float4 rows: S (sum), log(max(exp(S - max) / sum, eps)) (unary)
// The arithmetic of step 2 is inference._zoom's (torch's upsample_bilinear2d, align_corners=True, on float64 input):
//   scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
//   l1 = src - i0, l0 = 1 - l1, v = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11), rounded once to f32.
// -ffp-contract=off (Makefile) keeps every product and sum rounded on its own.  No atomics: results are bit-reproducible.
//
// Two front ends share the body: multiscale_unary_kernel (one image) and multiscale_unary_batch_kernel (G images whose score maps
// are the slices of K batched maps, test-ms.py's fixed sizes: blockIdx.x -> (image, block) through per-image block prefix sums).
//
// Mirrored test-time augmentation (the scores of a mirrored input, mirrored back and summed with the plain ones) is the body's
// MIRROR instantiation behind two front ends of its own, multiscale_unary_mirror_kernel and multiscale_unary_mirror_batch_kernel:
// a map whose bit of `mirror` is set is read as flip(map, last axis).  y0, y1, x0, x1 and the blend weights of step 1 come from
// the output pixel exactly as for a plain map; only the four loads move, to columns w - 1 - x0 and w - 1 - x1.  The MIRROR = false
// instantiations are the kernels as they were.
#include <math.h>
#include <string.h>
#include "common.h"

namespace dsrg {

constexpr int kMsPix = 64;        // output pixels per workgroup
constexpr int kMsThreads = 256;
constexpr int kMsMaxScales = 8;
constexpr int kMsMaxBatch = 16;   // images per batched launch (multiscale_unary_batch_kernel, preprocess_rect_batch_kernel)
constexpr int kMsMaxMirrorBatch = 8;   // ... of the mirror forms: two slices per image in a batch of at most 16

struct MsArgs {
    const float *s[kMsMaxScales];  // (C, h_k, w_k) score maps
    int h[kMsMaxScales], w[kMsMaxScales];
    double sh[kMsMaxScales], sw[kMsMaxScales];   // (in - 1) / (out - 1), 0 for out == 1
};

// block `blk` of one image: output pixels [64 blk, 64 blk + 64) of the H x W map
// (mirror: bit k set = map k is read with its columns reversed; MIRROR = false ignores it)
template <int K, bool MIRROR>
__device__ __forceinline__ void multiscale_unary_body(const MsArgs &a, unsigned mirror, int C, int H, int W, float eps, int blk,
                                                      float *__restrict__ unary, int32_t *__restrict__ amax,
                                                      float *__restrict__ sum_out) {
    __shared__ float s_tile[kMsPix * (kMaxLabels + 1)];     // [pixel][label], row stride Cs (odd: conflict-free columns)
    __shared__ float s_max[kMsPix], s_sum[kMsPix];

    const int N = H * W;
    const int pix0 = blk * kMsPix;
    const int npb = min(kMsPix, N - pix0);
    const int Cs = C | 1;
    const int tid = threadIdx.x;

    // 1. this lane's pixel (lanes p, p + 64, p + 128, p + 192 share it and take every fourth label): its source rows / columns
    // and blend weights at every scale, in registers
    const int p = tid % kMsPix, c0 = tid / kMsPix;
    const int i = pix0 + min(p, npb - 1);
    const int y = i / W, x = i - y * W;
    int o00[K], o01[K], o10[K], o11[K], hw[K];
    double l1h[K], l1w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int h = a.h[k], w = a.w[k];
        const double sy = a.sh[k] * (double)y, sx = a.sw[k] * (double)x;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const bool rev = MIRROR && ((mirror >> k) & 1u);
        const int c0x = rev ? w - 1 - x0 : x0, c1x = rev ? w - 1 - x1 : x1;      // the columns the two taps are loaded from
        o00[k] = y0 * w + c0x;
        o01[k] = y0 * w + c1x;
        o10[k] = y1 * w + c0x;
        o11[k] = y1 * w + c1x;
        hw[k] = h * w;
        l1h[k] = sy - (double)y0;
        l1w[k] = sx - (double)x0;
    }

    // 2. S[p][c] = ((z_0 + z_1) + z_2) ... in f32
#pragma unroll 1
    for (int c = c0; c < C; c += kMsThreads / kMsPix) {
        float S = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float *plane = a.s[k] + (size_t)c * hw[k];
            const double v00 = plane[o00[k]], v01 = plane[o01[k]], v10 = plane[o10[k]], v11 = plane[o11[k]];
            const double l0h = 1.0 - l1h[k], l0w = 1.0 - l1w[k];
            const float z = (float)(l0h * (l0w * v00 + l1w[k] * v01) + l1h[k] * (l0w * v10 + l1w[k] * v11));
            S = k == 0 ? z : S + z;
        }
        s_tile[p * Cs + c] = S;
    }
    __syncthreads();

    // 3. per pixel: 4 lanes, labels q, q + 4, ...; partials combined by lane exchange in a fixed order
    {
        const int p = tid >> 2, q = tid & 3;                // (shadows the lane's pixel of steps 1-2)
        const float *row = s_tile + p * Cs;
        float m = -INFINITY;
        int arg = C;
        for (int c = q; c < C; c += 4) {
            const float v = row[c];
            if (v > m || arg == C) { m = v; arg = c; }
        }
#pragma unroll
        for (int d = 1; d <= 2; d <<= 1) {
            const float om = __shfl_xor(m, d, 64);
            const int oa = __shfl_xor(arg, d, 64);
            if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }
        }
        float e = 0.0f;
        for (int c = q; c < C; c += 4) e += expf(row[c] - m);
#pragma unroll
        for (int d = 1; d <= 2; d <<= 1) {
            const float oe = __shfl_xor(e, d, 64);
            e = (q & d) ? oe + e : e + oe;              // same operand order on both lanes: all four end with one value
        }
        if (q == 0) {
            s_max[p] = m;
            s_sum[p] = e;
            if (amax && p < npb) amax[pix0 + p] = arg;
        }
    }
    __syncthreads();

    // 4. the block's output floats [pix0 * C, (pix0 + npb) * C) as float4 rows (pix0 * C is a multiple of 64)
    if (!unary && !sum_out) return;
    const int n = npb * C;
    const float invC = 1.0f / (float)C;
    const size_t base = (size_t)pix0 * C;
    for (int j4 = tid * 4; j4 < n; j4 += kMsThreads * 4) {
        float sv[4], uv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = min(j4 + r, n - 1);
            // j / C for j < 64 * 96: the quotient's fractional part is >= 0.5 / C away from the next integer, far above the error
            const int p = (int)(((float)j + 0.5f) * invC);
            const int c = j - p * C;
            const float S = s_tile[p * Cs + c];
            sv[r] = S;
            const float pr = expf(S - s_max[p]) / s_sum[p];
            uv[r] = logf(fmaxf(pr, eps));
        }
        if (j4 + 4 <= n) {
            if (unary) *reinterpret_cast<float4 *>(unary + base + j4) = make_float4(uv[0], uv[1], uv[2], uv[3]);
            if (sum_out) *reinterpret_cast<float4 *>(sum_out + base + j4) = make_float4(sv[0], sv[1], sv[2], sv[3]);
        } else {
            for (int r = 0; r < n - j4; ++r) {
                if (unary) unary[base + j4 + r] = uv[r];
                if (sum_out) sum_out[base + j4 + r] = sv[r];
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(kMsThreads) void multiscale_unary_kernel(MsArgs a, int C, int H, int W, float eps,
                                                                      float *__restrict__ unary, int32_t *__restrict__ amax,
                                                                      float *__restrict__ sum_out) {
    multiscale_unary_body<K, false>(a, 0u, C, H, W, eps, (int)blockIdx.x, unary, amax, sum_out);
}

template <int K>
__global__ __launch_bounds__(kMsThreads) void multiscale_unary_mirror_kernel(MsArgs a, unsigned mirror, int C, int H, int W, float eps,
                                                                             float *__restrict__ unary, int32_t *__restrict__ amax,
                                                                             float *__restrict__ sum_out) {
    multiscale_unary_body<K, true>(a, mirror, C, H, W, eps, (int)blockIdx.x, unary, amax, sum_out);
}

// G images in one launch.  s[k]: (Gcap, C, h_k, w_k) batched maps, image g reads slice g; blk0[g]: the first block of image g
// (blk0[G] = the grid).  The scale factors are the doubles launch_multiscale_unary computes on the host ((in - 1) / (out - 1) is
// one correctly rounded IEEE division on either side), so image g's outputs are those of the single-image kernel bit for bit.
struct MsBatchArgs {
    const float *s[kMsMaxScales];
    int h[kMsMaxScales], w[kMsMaxScales];
    int H[kMsMaxBatch], W[kMsMaxBatch];
    int blk0[kMsMaxBatch + 1];
    float *unary[kMsMaxBatch];
    int32_t *amax[kMsMaxBatch];
    float *sum[kMsMaxBatch];
};

template <int K>
__global__ __launch_bounds__(kMsThreads) void multiscale_unary_batch_kernel(MsBatchArgs b, int G, int C, float eps) {
    const int blk = (int)blockIdx.x;
    int g = 0;
    while (g + 1 < G && blk >= b.blk0[g + 1]) ++g;          // (uniform over the block)
    const int H = b.H[g], W = b.W[g];
    MsArgs a;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int h = b.h[k], w = b.w[k];
        a.s[k] = b.s[k] + (size_t)g * C * h * w;
        a.h[k] = h;
        a.w[k] = w;
        a.sh[k] = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
        a.sw[k] = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
    }
    multiscale_unary_body<K, false>(a, 0u, C, H, W, eps, blk - b.blk0[g], b.unary[g], b.amax[g], b.sum[g]);
}

// G images at K scales, each with its mirror: s[k] is (Gcap >= 2 G, C, h_k, w_k), image g reads slice 2 g plain and slice 2 g + 1
// mirrored back.  The body runs on the 2 K maps in the order scale 0 plain, scale 0 mirror, scale 1 plain, ..., which is the
// list multiscale_unary_mirror_kernel<2 K> gets for those slices with the flags 0, 1, 0, 1, ...: bit for bit its outputs.
template <int K>
__global__ __launch_bounds__(kMsThreads) void multiscale_unary_mirror_batch_kernel(MsBatchArgs b, int G, int C, float eps) {
    const int blk = (int)blockIdx.x;
    int g = 0;
    while (g + 1 < G && blk >= b.blk0[g + 1]) ++g;          // (uniform over the block)
    const int H = b.H[g], W = b.W[g];
    MsArgs a;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int h = b.h[k], w = b.w[k];
        const size_t slice = (size_t)C * h * w;
        a.s[2 * k] = b.s[k] + (size_t)(2 * g) * slice;
        a.s[2 * k + 1] = b.s[k] + (size_t)(2 * g + 1) * slice;
        a.h[2 * k] = a.h[2 * k + 1] = h;
        a.w[2 * k] = a.w[2 * k + 1] = w;
        a.sh[2 * k] = a.sh[2 * k + 1] = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
        a.sw[2 * k] = a.sw[2 * k + 1] = W > 1 ? (double)(w - 1) / (double)(W - 1) : 0.0;
    }
    multiscale_unary_body<2 * K, true>(a, 0xAAu, C, H, W, eps, blk - b.blk0[g], b.unary[g], b.amax[g], b.sum[g]);
}

int check_multiscale_unary(int K, int C, const float *const *scores, const int32_t *h, const int32_t *w, int H, int W,
                           const float *unary, const int32_t *amax, const float *sum_out) {
    if (K < 1 || K > kMsMaxScales) return set_error(DSRG_ERR_INVALID, "multiscale unary: 1..%d scales, got %d", kMsMaxScales, K);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "multiscale unary: %d labels", C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_INVALID, "multiscale unary: at most %d labels, got %d", kMaxLabels, C);
    if (H < 1 || W < 1) return set_error(DSRG_ERR_INVALID, "multiscale unary: output %dx%d", H, W);
    if (!scores || !h || !w) return set_error(DSRG_ERR_INVALID, "multiscale unary: NULL score / size array");
    if (!unary && !amax && !sum_out) return set_error(DSRG_ERR_INVALID, "multiscale unary: no output requested");
    if ((long long)H * W * C >= (1LL << 31))
        return set_error(DSRG_ERR_UNSUPPORTED, "multiscale unary: H*W*C = %lld >= 2^31", (long long)H * W * C);
    for (int k = 0; k < K; ++k) {
        if (!scores[k]) return set_error(DSRG_ERR_INVALID, "multiscale unary: score map %d is NULL", k);
        if (h[k] < 1 || w[k] < 1) return set_error(DSRG_ERR_INVALID, "multiscale unary: score map %d is %dx%d", k, h[k], w[k]);
        if ((long long)h[k] * w[k] * C >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "multiscale unary: score map %d holds >= 2^31 values", k);
    }
    if ((unary && ((uintptr_t)unary & 15)) || (sum_out && ((uintptr_t)sum_out & 15)))
        return set_error(DSRG_ERR_INVALID, "multiscale unary: unary / sum outputs must be 16-byte aligned");
    return DSRG_OK;
}

// mirrored: dsrg_multiscale_unary_mirror (mirror: K flags, non-zero = map k is read with its columns reversed), else
// dsrg_multiscale_unary (mirror unused)
static int launch_multiscale_unary_any(bool mirrored, int K, int C, const float *const *scores, const int32_t *mirror, const int32_t *h,
                                       const int32_t *w, int H, int W, float eps, float *unary, int32_t *amax, float *sum_out,
                                       hipStream_t stream) {
    int rc = check_multiscale_unary(K, C, scores, h, w, H, W, unary, amax, sum_out);
    if (rc) return rc;
    if (mirrored && !mirror) return set_error(DSRG_ERR_INVALID, "multiscale unary mirror: NULL mirror flag array");
    MsArgs a;
    memset(&a, 0, sizeof(a));
    unsigned mask = 0;
    for (int k = 0; k < K; ++k) {
        a.s[k] = scores[k];
        a.h[k] = h[k];
        a.w[k] = w[k];
        a.sh[k] = H > 1 ? (double)(h[k] - 1) / (double)(H - 1) : 0.0;
        a.sw[k] = W > 1 ? (double)(w[k] - 1) / (double)(W - 1) : 0.0;
        if (mirrored && mirror[k]) mask |= 1u << k;
    }
    const dim3 grid((unsigned)((H * W + kMsPix - 1) / kMsPix)), block(kMsThreads);
    switch (K) {
#define DSRG_MS_CASE(k)                                                                                                          \
    case k:                                                                                                                      \
        if (mirrored)                                                                                                            \
            hipLaunchKernelGGL(multiscale_unary_mirror_kernel<k>, grid, block, 0, stream, a, mask, C, H, W, eps, unary, amax,    \
                               sum_out);                                                                                         \
        else                                                                                                                     \
            hipLaunchKernelGGL(multiscale_unary_kernel<k>, grid, block, 0, stream, a, C, H, W, eps, unary, amax, sum_out);       \
        break;
        DSRG_MS_CASE(1) DSRG_MS_CASE(2) DSRG_MS_CASE(3) DSRG_MS_CASE(4) DSRG_MS_CASE(5) DSRG_MS_CASE(6) DSRG_MS_CASE(7)
        DSRG_MS_CASE(8)
#undef DSRG_MS_CASE
    }
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_multiscale_unary(int K, int C, const float *const *scores, const int32_t *h, const int32_t *w, int H, int W, float eps,
                            float *unary, int32_t *amax, float *sum_out, hipStream_t stream) {
    return launch_multiscale_unary_any(false, K, C, scores, nullptr, h, w, H, W, eps, unary, amax, sum_out, stream);
}

int launch_multiscale_unary_mirror(int K, int C, const float *const *scores, const int32_t *mirror, const int32_t *h, const int32_t *w,
                                   int H, int W, float eps, float *unary, int32_t *amax, float *sum_out, hipStream_t stream) {
    return launch_multiscale_unary_any(true, K, C, scores, mirror, h, w, H, W, eps, unary, amax, sum_out, stream);
}

// mirrored: dsrg_multiscale_unary_mirror_batch (at most kMsMaxMirrorBatch images and kMsMaxScales / 2 scales, each scale's map
// holding two slices per image), else dsrg_multiscale_unary_batch; `what` names the entry point in the messages
static int launch_multiscale_unary_batch_any(bool mirrored, const char *what, int G, int K, int C, const float *const *scores,
                                             const int32_t *h, const int32_t *w, const int32_t *H, const int32_t *W, float eps,
                                             float *const *unary, int32_t *const *amax, float *const *sum_out, hipStream_t stream) {
    const int maxG = mirrored ? kMsMaxMirrorBatch : kMsMaxBatch;
    if (G < 1 || G > maxG) return set_error(DSRG_ERR_INVALID, "%s: 1..%d images, got %d", what, maxG, G);
    if (mirrored && (K < 1 || K > kMsMaxScales / 2))
        return set_error(DSRG_ERR_INVALID, "%s: 1..%d scales (each with its mirror), got %d", what, kMsMaxScales / 2, K);
    if (!H || !W) return set_error(DSRG_ERR_INVALID, "%s: NULL image size array", what);
    const int cu = output_class((const void *const *)unary, G), ca = output_class((const void *const *)amax, G),
              cs = output_class((const void *const *)sum_out, G);
    if (cu < 0 || ca < 0 || cs < 0)
        return set_error(DSRG_ERR_INVALID, "%s: an output class must be NULL or set for every image", what);
    MsBatchArgs b;
    memset(&b, 0, sizeof(b));
    for (int g = 0; g < G; ++g) {
        // the single-image checks, image by image (K, C, the score maps and "no output requested" among them)
        int rc = check_multiscale_unary(K, C, scores, h, w, H[g], W[g], cu ? unary[g] : nullptr, ca ? amax[g] : nullptr,
                                        cs ? sum_out[g] : nullptr);
        if (rc) return rc;
        b.H[g] = H[g];
        b.W[g] = W[g];
        b.blk0[g + 1] = b.blk0[g] + (H[g] * W[g] + kMsPix - 1) / kMsPix;      // < 2^25 blocks per image
        b.unary[g] = cu ? unary[g] : nullptr;
        b.amax[g] = ca ? amax[g] : nullptr;
        b.sum[g] = cs ? sum_out[g] : nullptr;
    }
    for (int k = 0; k < K; ++k) {
        b.s[k] = scores[k];
        b.h[k] = h[k];
        b.w[k] = w[k];
    }
    const dim3 grid((unsigned)b.blk0[G]), block(kMsThreads);
    if (mirrored) {
        switch (K) {
#define DSRG_MS_CASE(k) \
    case k: hipLaunchKernelGGL(multiscale_unary_mirror_batch_kernel<k>, grid, block, 0, stream, b, G, C, eps); break;
            DSRG_MS_CASE(1) DSRG_MS_CASE(2) DSRG_MS_CASE(3) DSRG_MS_CASE(4)
#undef DSRG_MS_CASE
        }
    } else {
        switch (K) {
#define DSRG_MS_CASE(k) \
    case k: hipLaunchKernelGGL(multiscale_unary_batch_kernel<k>, grid, block, 0, stream, b, G, C, eps); break;
            DSRG_MS_CASE(1) DSRG_MS_CASE(2) DSRG_MS_CASE(3) DSRG_MS_CASE(4) DSRG_MS_CASE(5) DSRG_MS_CASE(6) DSRG_MS_CASE(7)
            DSRG_MS_CASE(8)
#undef DSRG_MS_CASE
        }
    }
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_multiscale_unary_batch(int G, int K, int C, const float *const *scores, const int32_t *h, const int32_t *w,
                                  const int32_t *H, const int32_t *W, float eps, float *const *unary, int32_t *const *amax,
                                  float *const *sum_out, hipStream_t stream) {
    return launch_multiscale_unary_batch_any(false, "multiscale unary batch", G, K, C, scores, h, w, H, W, eps, unary, amax, sum_out,
                                             stream);
}

int launch_multiscale_unary_mirror_batch(int G, int K, int C, const float *const *scores, const int32_t *h, const int32_t *w,
                                         const int32_t *H, const int32_t *W, float eps, float *const *unary, int32_t *const *amax,
                                         float *const *sum_out, hipStream_t stream) {
    return launch_multiscale_unary_batch_any(true, "multiscale unary mirror batch", G, K, C, scores, h, w, H, W, eps, unary, amax,
                                             sum_out, stream);
}

}  // namespace dsrg
