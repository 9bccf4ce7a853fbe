// The stem of the DeepLab-v2 ResNet-101 at test time in ONE launch (no reference counterpart: the reference's networks are Caffe
// prototxts; dsrg_amd/retrain.py ResNet101DeepLab.stem is the module this restates):
//   conv 7x7 / 2, pad 3, 3 -> 64 (kernel x frozen BatchNorm scale, packed once)  ->  + shift  ->  ReLU  ->  max pool 3x3 / 2, pad 1, ceil
// x (B,3,H,W) float32 NCHW in, (B,PH,PW,64) bf16 NHWC out; the OHc x OWc x 64 convolution map lives in LDS only.
//
// A workgroup of 4 waves owns a tile of 4 x 8 pooled pixels = 9 x 17 convolution pixels = a 23 x 39 x 3 input patch:
//   1. the patch is read (unconditional loads on clamped indices, zero selected outside the image), rounded to bf16 (nearest even)
//      and laid in LDS as [c][23][40] (column 39 is a zero: the eighth tap of a kernel row, whose weight is zero, reads it);
//   2. an implicit GEMM on v_mfma_f32_16x16x32_bf16, M = 64 channels, N = 153 pixels (10 blocks of 16, dealt to the waves round robin),
//      K = 192: k = (ky * 3 + c) * 8 + kx — the 8 values of a pixel's fragment are 8 neighbours of one patch row (four 4-byte LDS
//      reads, stride 2 makes the start even), groups 21..23 and kx = 7 carry zero weights.  The 24 weight fragments of a wave
//      (4 channel blocks x 6 K-steps, 96 registers) are loaded once from the packed kernel (24 KiB, L2);
//   3. + shift, ReLU, and a pixel that is not on the OHc x OWc map (the tile's overhang, the pool's pad and ceil-mode overhang) is
//      written as 0 — NOT as a convolution over zero padding, which would be relu(shift) — into LDS [pixel][68] float32;
//   4. a thread takes the 3x3 window maximum of 8 channels of one pooled pixel (every real value is >= 0 and every window holds a
//      real pixel), rounds once to bf16 and stores 16 bytes.
// No scratch, no atomics; results do not depend on the tiling (fp32 accumulation order is fixed per output).
#include "common.h"

namespace dsrg {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int kStemCout = 64, kStemCin = 3, kStemTaps = 7;
constexpr int kStemGroups = kStemTaps * kStemCin;            // 21 (ky, c) kernel rows of 8 (7 taps + a zero)
constexpr int kStemK = 192;                                  // 24 groups x 8: six K-steps of 32
constexpr int kStemKSteps = kStemK / 32;
constexpr int kTPH = 4, kTPW = 8;                            // pooled pixels per tile
constexpr int kTCH = 2 * kTPH + 1, kTCW = 2 * kTPW + 1;      // 9 x 17 convolution pixels
constexpr int kTPix = kTCH * kTCW;                           // 153
constexpr int kPixBlocks = (kTPix + 15) / 16;                // 10
constexpr int kPRows = 2 * (kTCH - 1) + kStemTaps;           // 23 patch rows
constexpr int kPCols = 2 * (kTCW - 1) + kStemTaps + 1;       // 39 patch columns + the zero column
constexpr int kPWords = kPCols / 2;                          // 20 words of two bf16 per patch row
constexpr int kConvStride = 68;                              // floats per pixel row of the LDS map (64 + 4: 16-byte aligned, off the bank line)
constexpr int kStemThreads = 256;
static_assert(kPCols % 2 == 0 && kConvStride % 4 == 0, "patch rows are whole words, map rows whole float4s");
static_assert(kTPH * kTPW * (kStemCout / 8) == kStemThreads, "one thread per (pooled pixel, 8 channels)");

__device__ __forceinline__ uint32_t stem_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;      // NaN stays NaN
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// packed[o][k], k = (ky * 3 + c) * 8 + kx: bf16(w[o][c][ky][kx] * scale[o]) — one float32 product, one rounding; 0 where kx = 7 or
// the group is padding
__global__ __launch_bounds__(256) void resnet_stem_pack_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                               uint16_t *__restrict__ packed) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kStemCout * kStemK) return;
    const int o = idx / kStemK, k = idx - o * kStemK;
    const int g = k >> 3, kx = k & 7;
    const bool real = g < kStemGroups && kx < kStemTaps;
    const int ky = min(g, kStemGroups - 1) / kStemCin, c = min(g, kStemGroups - 1) % kStemCin;
    const float v = w[((o * kStemCin + c) * kStemTaps + ky) * kStemTaps + min(kx, kStemTaps - 1)] * scale[o];
    packed[idx] = real ? (uint16_t)stem_bf16_rne(v) : (uint16_t)0;
}

__global__ __launch_bounds__(kStemThreads) void resnet_stem_kernel(const float *__restrict__ x, const uint16_t *__restrict__ packed,
                                                                   const float *__restrict__ shift, uint4 *__restrict__ y, int H, int W,
                                                                   int OHc, int OWc, int PH, int PW, int ntx, int nty) {
    __shared__ __attribute__((aligned(16))) uint32_t patch[kStemCin * kPRows * kPWords];       // 5 520 B
    __shared__ __attribute__((aligned(16))) float cmap[kTPix * kConvStride];                   // 41 616 B
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l15 = lane & 15, g4 = lane >> 4;
    int t = blockIdx.x;
    const int tx = t % ntx;
    t /= ntx;
    const int ty = t % nty, b = t / nty;
    const int py0 = ty * kTPH, px0 = tx * kTPW;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;                     // first convolution pixel of the tile (-1: the pool's pad)
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;                     // first input pixel of the patch

    // ---- 1. the input patch, two neighbours per word
    const float *xb = x + (size_t)b * kStemCin * H * W;
    for (int i = tid; i < kStemCin * kPRows * kPWords; i += kStemThreads) {
        const int c = i / (kPRows * kPWords), r = (i / kPWords) % kPRows, q = (i % kPWords) * 2;
        const int iy = iy0 + r, ixa = ix0 + q, ixb = ixa + 1;
        const bool row_on = iy >= 0 && iy < H;
        const bool on_a = row_on && ixa >= 0 && ixa < W;
        const bool on_b = row_on && ixb >= 0 && ixb < W && q + 1 < kPCols - 1;         // the last column is the zero
        const float *row = xb + ((size_t)c * H + min(max(iy, 0), H - 1)) * W;
        const float va = row[min(max(ixa, 0), W - 1)], vb = row[min(max(ixb, 0), W - 1)];   // clamped: unconditional loads
        patch[i] = (on_a ? stem_bf16_rne(va) : 0u) | ((on_b ? stem_bf16_rne(vb) : 0u) << 16);
    }

    // ---- the wave's weight fragments: A[row = channel ct * 16 + l15][k = 32 s + 8 g4 + j]
    bf16x8 wf[4][kStemKSteps];
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int s = 0; s < kStemKSteps; s++)
            wf[ct][s] = *reinterpret_cast<const bf16x8 *>(packed + (ct * 16 + l15) * kStemK + s * 32 + g4 * 8);
    f32x4 sh[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) sh[ct] = *reinterpret_cast<const f32x4 *>(shift + ct * 16 + g4 * 4);
    __syncthreads();

    // ---- 2. + 3. implicit GEMM per block of 16 pixels, epilogue into the LDS map
    for (int nb = wv; nb < kPixBlocks; nb += kStemThreads / 64) {
        const int p = nb * 16 + l15, pc = min(p, kTPix - 1);            // (the padding pixels of the last block read pixel 152's data)
        const int cyl = pc / kTCW, cxl = pc - cyl * kTCW;
        f32x4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < kStemKSteps; s++) {
            // padding groups re-read the last one, and the eighth element of every fragment is the pixel's right-hand neighbour (or
            // the zero column): real data x zero weights.  So a NON-FINITE input value (0 x inf = NaN) also reaches the convolution
            // pixel whose row fragment ends on it, one column outside its receptive field — harmless for image data, which is finite.
            const int g = min(4 * s + g4, kStemGroups - 1);
            const int ky = g / kStemCin, c = g - ky * kStemCin;
            const uint32_t *src = patch + (c * kPRows + 2 * cyl + ky) * kPWords + cxl;      // element 2 cxl of the row
            const bf16x8 pf = __builtin_bit_cast(bf16x8, (u32x4{src[0], src[1], src[2], src[3]}));   // B[k = 32 s + 8 g4 + j][col = pixel l15]
#pragma unroll
            for (int ct = 0; ct < 4; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct][s], pf, acc[ct], 0, 0, 0);
        }
        // D[row = channel ct * 16 + 4 g4 + reg][col = pixel l15]
        const int cy = cy0 + cyl, cx = cx0 + cxl;
        const bool real = cy >= 0 && cy < OHc && cx >= 0 && cx < OWc;
        if (p < kTPix) {
#pragma unroll
            for (int ct = 0; ct < 4; ct++) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float a = acc[ct][r] + sh[ct][r];
                    v[r] = (real && a > 0.f) ? a : 0.f;
                }
                *reinterpret_cast<f32x4 *>(cmap + p * kConvStride + ct * 16 + g4 * 4) = v;
            }
        }
    }
    __syncthreads();

    // ---- 4. the pool: thread = (pooled pixel tid / 8, channels 8 (tid % 8) ..)
    const int pp = tid >> 3, cg = tid & 7;
    const int pi = pp / kTPW, pj = pp - pi * kTPW;
    const int py = py0 + pi, px = px0 + pj;
    if (py < PH && px < PW) {
        float m[8];
#pragma unroll
        for (int k = 0; k < 8; k++) m[k] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const float *src = cmap + ((2 * pi + dy) * kTCW + 2 * pj + dx) * kConvStride + cg * 8;
                const f32x4 a = *reinterpret_cast<const f32x4 *>(src), c = *reinterpret_cast<const f32x4 *>(src + 4);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    m[k] = a[k] > m[k] ? a[k] : m[k];
                    m[4 + k] = c[k] > m[4 + k] ? c[k] : m[4 + k];
                }
            }
        uint4 o;
        o.x = stem_bf16_rne(m[0]) | (stem_bf16_rne(m[1]) << 16);
        o.y = stem_bf16_rne(m[2]) | (stem_bf16_rne(m[3]) << 16);
        o.z = stem_bf16_rne(m[4]) | (stem_bf16_rne(m[5]) << 16);
        o.w = stem_bf16_rne(m[6]) | (stem_bf16_rne(m[7]) << 16);
        y[(((size_t)b * PH + py) * PW + px) * (kStemCout / 8) + cg] = o;
    }
}

// 3x3 / stride 2 / pad 1 ceil-mode pooling extent (Caffe's rule, torch's with ceil_mode: the last window starts on the map or its left pad)
int stem_pool_size(int n) {
    int o = (n + 2 - 3 + 1) / 2 + 1;
    if ((o - 1) * 2 >= n + 1) --o;
    return o;
}

}  // namespace

size_t resnet_stem_packed_bytes() { return (size_t)kStemCout * kStemK * sizeof(uint16_t); }

// (api.hip has refused NULL pointers and B, H, W < 1 before either launcher runs)
int launch_pack_resnet_stem(const float *w, const float *scale, void *packed, hipStream_t stream) {
    if (((uintptr_t)w | (uintptr_t)scale) & 3) return set_error(DSRG_ERR_INVALID, "resnet stem pack: kernel / scale not aligned to a float");
    if ((uintptr_t)packed & 15) return set_error(DSRG_ERR_INVALID, "resnet stem pack: packed kernel not aligned to 16 bytes");
    hipLaunchKernelGGL(resnet_stem_pack_kernel, dim3((kStemCout * kStemK + 255) / 256), dim3(256), 0, stream, w, scale,
                       static_cast<uint16_t *>(packed));
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

int launch_resnet_stem(const float *x, const void *packed, const float *shift, void *y, int B, int H, int W, hipStream_t stream) {
    if ((uintptr_t)x & 3) return set_error(DSRG_ERR_INVALID, "resnet stem: input not aligned to a float");
    if (((uintptr_t)packed | (uintptr_t)shift | (uintptr_t)y) & 15)
        return set_error(DSRG_ERR_INVALID, "resnet stem: packed kernel / shift / output not aligned to 16 bytes");
    if (H >= (1 << 28) || W >= (1 << 28)) return set_error(DSRG_ERR_UNSUPPORTED, "resnet stem: a %dx%d image (sides < 2^28)", H, W);
    const int OHc = (H - 1) / 2 + 1, OWc = (W - 1) / 2 + 1;
    const int PH = stem_pool_size(OHc), PW = stem_pool_size(OWc);
    const int nty = (PH + kTPH - 1) / kTPH, ntx = (PW + kTPW - 1) / kTPW;
    const long long tiles = (long long)B * nty * ntx;
    if (tiles >= (1LL << 31)) return set_error(DSRG_ERR_UNSUPPORTED, "resnet stem: %lld tiles >= 2^31", tiles);
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)tiles), dim3(kStemThreads), 0, stream, x, static_cast<const uint16_t *>(packed),
                       shift, static_cast<uint4 *>(y), H, W, OHc, OWc, PH, PW, ntx, nty);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
