// Multi-scale-input training with max fusion (DeepLab-v2's "MSC" recipe; the reference retrains at one scale and has no counterpart):
// the input pyramid in one launch, and the S + 1 softmax losses of S score maps with their gradients in three.
//
// msc_pyramid_kernel: one lane per pixel of every smaller copy.  (B, 3, H, W) NCHW -> up to three (B, 3, H_s, W_s) copies written
// channels-last (the three values of a pixel side by side), with the project's align-corners zoom (eval.hip / seg_loss.hip):
//   scale = (in - 1) / (out - 1) in double on the host (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
//   l1 = src - i0, l0 = 1 - l1, v = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11) in double, rounded once to f32
// (-ffp-contract=off: every product and sum rounded on its own).
//
// The loss.  Map 0 is the full scale; u_0 = z_0, u_s = z_s zoomed to h_0 x w_0 with the arithmetic above, f_c = max_s u_s,c and the
// winner k_c = the lowest s that attains it (strict > walking s upwards).  Map s is judged against the nearest sample of the label
// map at the align-corners position, in integers: y = (2 i (H - 1) + (h_s - 1)) / (2 (h_s - 1)), 0 when h_s == 1; the fused head
// shares map 0's labels.  Every head per valid pixel exactly as seg_loss.hip: m = first maximum, e_c = expf(z_c - m), s = sum e_c
// in f32 with c ascending, r = 1 / s, loss term logf(s) - (z_label - m), d_c = e_c * r - [c == label]; 0 where the pixel is not valid.
//
// msc_main_kernel    one lane per pixel of every map; a workgroup (one wave) belongs to one map.  The lane writes the
//                    unnormalised d_s to grad_s.  A map-0 lane also blends the other maps, picks the winners and runs the fused
//                    softmax: f_c is parked in the workspace while m and s are found (the lane reads back what it wrote), then
//                    replaced by d_f,c, with the winner byte beside it.  Loss and counts go to the workgroup's slot, reduced over the
//                    lanes by a fixed tree in LDS.
// msc_reduce_kernel  one workgroup: the slots of every map summed in slot order (lane-strided, then the same tree) -> the S valid
//                    counts (kept in the workspace's header), the S + 1 losses, the three counters of the fused head (added to).
// msc_finish_kernel  one lane per element of every grad_s.  Map 0: (d_0 + [k == 0] d_f) / (float)max(N_0, 1).  Map s > 0: the lane
//                    owns cell (a, b) of plane c and GATHERS G = sum over the map-0 pixels whose taps touch the cell of
//                    (wy * wx) * [k_c == s] * d_f,c — rows from the top, a row's products from the left, the row's sum added to
//                    the cell's (seg_loss.hip's order and its f32 weights: (float)l0 / (float)l1, their f32 sum where both taps
//                    are one cell) — and writes d_s / (float)max(N_s, 1) + G / (float)max(N_0, 1).
// Every floating-point sum has an order fixed by the shapes alone; there are no floating-point atomics, neither on memory nor on
// LDS: repeated calls give identical bits.
#include "common.h"
#include "zoom_gather.h"

namespace dsrg {

constexpr int kMscMaxMaps = 4;
constexpr int kMscMaxBatch = 32;
constexpr int kMscThreads = 64;            // main kernel: one wave per workgroup (16 810 map-0 pixels of the workload: 263 workgroups for 256 CUs)
constexpr int kMscWide = 256;              // reduce / finish / pyramid
constexpr size_t kMscHeadBytes = 64;       // the workspace's header: the S valid counts N_s, 64 bits each (left there for the caller)

struct MscPart {                           // a workgroup's slot of the workspace
    double loss, loss_fused;
    unsigned int valid, correct, invalid, pad;
};

struct MscMaps {
    const float *z[kMscMaxMaps];
    float *g[kMscMaxMaps];
    int h[kMscMaxMaps], w[kMscMaxMaps];
    double sh[kMscMaxMaps], sw[kMscMaxMaps];   // (h_s - 1) / (h_0 - 1): map 0's pixel -> map s's coordinate
    unsigned int blk0[kMscMaxMaps + 1];        // main kernel: map s owns the workgroups [blk0[s], blk0[s + 1])
    unsigned int el0[kMscMaxMaps + 1];         // finish kernel: map s owns the elements [el0[s], el0[s + 1])
};

struct MscView {                           // one map's entries of MscMaps (picked with constant indices: the struct stays in the kernel arguments)
    const float *z;
    float *g;
    int h, w;
    double sh, sw;
};

__device__ __forceinline__ MscView msc_view(const MscMaps &M, int s) {
    MscView v = {M.z[0], M.g[0], M.h[0], M.w[0], M.sh[0], M.sw[0]};
#pragma unroll
    for (int k = 1; k < kMscMaxMaps; ++k)
        if (k == s) v = MscView{M.z[k], M.g[k], M.h[k], M.w[k], M.sh[k], M.sw[k]};
    return v;
}

// the label of a pixel as a class, or -1; *invalid: neither a class nor ignore_label
__device__ __forceinline__ int msc_class(float l, int C, float ignore_label, bool *invalid) {
    int g = -1;
    *invalid = false;
    if (l != ignore_label) {
        if (l >= 0.0f && l < (float)C) {
            const int gi = (int)l;
            if ((float)gi == l) g = gi;
        }
        *invalid = g < 0;
    }
    return g;
}

// nearest sample of an axis of N labels for coordinate i of an axis of n
__device__ __forceinline__ int msc_label_coord(int i, int n, int N) {
    return n > 1 ? (int)((2LL * i * (N - 1) + (n - 1)) / (2LL * (n - 1))) : 0;
}

struct MscTaps {
    int o0, o1;
    double l0, l1;
};

__device__ __forceinline__ MscTaps msc_taps(double scale, int d, int n_in) {
    const double src = scale * (double)d;
    const int i0 = min((int)src, n_in - 1);                                   // (the min never binds: eval.hip)
    MscTaps t;
    t.o0 = i0, t.o1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (double)i0, t.l0 = 1.0 - t.l1;
    return t;
}

__global__ __launch_bounds__(kMscThreads) void msc_main_kernel(MscMaps M, int S, int B, int C, const float *__restrict__ labels, int H,
                                                                int W, float ignore_label, float *__restrict__ df,
                                                                unsigned char *__restrict__ win, MscPart *__restrict__ parts) {
    __shared__ double s_redd[kMscThreads];
    __shared__ unsigned int s_redu[kMscThreads];
    const int tid = threadIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 1; k < kMscMaxMaps; ++k)
        if (k < S && blockIdx.x >= M.blk0[k]) s = k;
    const MscView V = msc_view(M, s);
    unsigned int first = M.blk0[0];
#pragma unroll
    for (int k = 1; k < kMscMaxMaps; ++k)
        if (k == s) first = M.blk0[k];
    const int hw = V.h * V.w;
    const unsigned int t = (blockIdx.x - first) * kMscThreads + tid;          // the pixel among the map's B * h * w
    double loss = 0.0, loss_f = 0.0;
    unsigned int n_valid = 0, n_correct = 0, n_invalid = 0;
    if (t < (unsigned int)B * (unsigned int)hw) {
        const int b = t / hw, q = t - b * hw;
        const int i = q / V.w, j = q - i * V.w;
        const float l = labels[(size_t)b * H * W + (size_t)msc_label_coord(i, V.h, H) * W + msc_label_coord(j, V.w, W)];
        bool invalid;
        const int g = msc_class(l, C, ignore_label, &invalid);
        const float *zp = V.z + (size_t)b * C * hw + q;
        float *gp = V.g + (size_t)b * C * hw + q;
        if (g < 0) {
            for (int c = 0; c < C; ++c) gp[(size_t)c * hw] = 0.0f;
        } else {
            float m = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float z = zp[(size_t)c * hw];
                if (c == 0 || z > m) m = z;
            }
            float sum = 0.0f;
            for (int c = 0; c < C; ++c) sum += expf(zp[(size_t)c * hw] - m);
            const float r = 1.0f / sum;
            for (int c = 0; c < C; ++c) gp[(size_t)c * hw] = expf(zp[(size_t)c * hw] - m) * r - (c == g ? 1.0f : 0.0f);
            loss = (double)(logf(sum) - (zp[(size_t)g * hw] - m));
            n_valid = 1;
        }
        if (s == 0) {                                                         // (the whole workgroup: a workgroup belongs to one map)
            n_invalid = invalid ? 1u : 0u;
            float *fp = df + (size_t)b * C * hw + q;
            unsigned char *kp = win + (size_t)b * C * hw + q;
            if (g < 0) {
                for (int c = 0; c < C; ++c) fp[(size_t)c * hw] = 0.0f, kp[(size_t)c * hw] = 0;
            } else {
                MscTaps ty[kMscMaxMaps], tx[kMscMaxMaps];
#pragma unroll
                for (int k = 1; k < kMscMaxMaps; ++k)
                    if (k < S) ty[k] = msc_taps(M.sh[k], i, M.h[k]), tx[k] = msc_taps(M.sw[k], j, M.w[k]);
                float m = 0.0f;
                int arg = 0;
                for (int c = 0; c < C; ++c) {
                    float f = zp[(size_t)c * hw];
                    int k_win = 0;
#pragma unroll
                    for (int k = 1; k < kMscMaxMaps; ++k) {
                        if (k < S) {
                            const int wk = M.w[k];
                            const float *pl = M.z[k] + ((size_t)b * C + c) * M.h[k] * wk;
                            const double v00 = pl[ty[k].o0 * wk + tx[k].o0], v01 = pl[ty[k].o0 * wk + tx[k].o1];
                            const double v10 = pl[ty[k].o1 * wk + tx[k].o0], v11 = pl[ty[k].o1 * wk + tx[k].o1];
                            const float u = (float)(ty[k].l0 * (tx[k].l0 * v00 + tx[k].l1 * v01) + ty[k].l1 * (tx[k].l0 * v10 + tx[k].l1 * v11));
                            if (u > f) f = u, k_win = k;
                        }
                    }
                    fp[(size_t)c * hw] = f;
                    kp[(size_t)c * hw] = (unsigned char)k_win;
                    if (c == 0 || f > m) m = f, arg = c;
                }
                float sum = 0.0f;
                for (int c = 0; c < C; ++c) sum += expf(fp[(size_t)c * hw] - m);
                const float r = 1.0f / sum;
                const float fl = fp[(size_t)g * hw];
                for (int c = 0; c < C; ++c) fp[(size_t)c * hw] = expf(fp[(size_t)c * hw] - m) * r - (c == g ? 1.0f : 0.0f);
                loss_f = (double)(logf(sum) - (fl - m));
                n_correct = arg == g ? 1u : 0u;
            }
        }
    }
    const double tl = sl_block_sum<kMscThreads>(loss, s_redd);
    const double tf = sl_block_sum<kMscThreads>(loss_f, s_redd);
    const unsigned int tv = sl_block_sum<kMscThreads>(n_valid, s_redu);
    const unsigned int tc = sl_block_sum<kMscThreads>(n_correct, s_redu);
    const unsigned int ti = sl_block_sum<kMscThreads>(n_invalid, s_redu);
    if (tid == 0) {
        MscPart p;
        p.loss = tl, p.loss_fused = tf, p.valid = tv, p.correct = tc, p.invalid = ti, p.pad = 0;
        parts[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(kMscWide) void msc_reduce_kernel(MscMaps M, int S, const MscPart *__restrict__ parts,
                                                              unsigned long long *__restrict__ head, float *__restrict__ losses,
                                                              unsigned long long *__restrict__ counters) {
    __shared__ double s_redd[kMscWide];
    __shared__ unsigned long long s_redu[kMscWide];
    const int tid = threadIdx.x;
    unsigned long long n0 = 1;
#pragma unroll
    for (int s = 0; s < kMscMaxMaps; ++s) {
        if (s >= S) break;
        double l = 0.0, lf = 0.0;
        unsigned long long nv = 0, nc = 0, ni = 0;
        for (unsigned int k = M.blk0[s] + tid; k < M.blk0[s + 1]; k += kMscWide) {
            const MscPart p = parts[k];
            l += p.loss, lf += p.loss_fused;
            nv += p.valid, nc += p.correct, ni += p.invalid;
        }
        const unsigned long long N = sl_block_sum<kMscWide>(nv, s_redu);
        const unsigned long long D = N > 0 ? N : 1;
        const double L = sl_block_sum<kMscWide>(l, s_redd);
        if (s == 0) {
            const double LF = sl_block_sum<kMscWide>(lf, s_redd);
            const unsigned long long NC = sl_block_sum<kMscWide>(nc, s_redu);
            const unsigned long long NI = sl_block_sum<kMscWide>(ni, s_redu);
            n0 = D;
            if (tid == 0) {
                losses[0] = (float)(LF / (double)n0);
                counters[0] += N;
                counters[1] += NC;
                counters[2] += NI;
            }
        }
        if (tid == 0) {
            losses[1 + s] = (float)(L / (double)D);
            head[s] = N;
        }
    }
}

__global__ __launch_bounds__(kMscWide) void msc_finish_kernel(MscMaps M, int S, int C, const unsigned long long *__restrict__ head,
                                                              const float *__restrict__ df, const unsigned char *__restrict__ win) {
    const unsigned int e = blockIdx.x * kMscWide + threadIdx.x;
    if (e >= M.el0[S]) return;
    int s = 0;
#pragma unroll
    for (int k = 1; k < kMscMaxMaps; ++k)
        if (k < S && e >= M.el0[k]) s = k;
    unsigned int first = 0;
    unsigned long long ns = head[0];
#pragma unroll
    for (int k = 1; k < kMscMaxMaps; ++k)
        if (k == s) first = M.el0[k], ns = head[k];
    const unsigned long long n0 = head[0];
    const float den0 = (float)(n0 > 0 ? n0 : 1), den = (float)(ns > 0 ? ns : 1);
    const unsigned int r = e - first;                                         // (b, c, i, j) of the map, NCHW
    if (s == 0) {
        M.g[0][r] = (M.g[0][r] + (win[r] == 0 ? df[r] : 0.0f)) / den0;
        return;
    }
    const MscView V = msc_view(M, s);
    const int h0 = M.h[0], w0 = M.w[0], hw0 = h0 * w0;
    const int hw = V.h * V.w;
    const unsigned int bc = r / hw;
    const int q = r - bc * hw, a = q / V.w, bb = q - a * V.w;
    const int ya = sl_first(V.sh, a - 1, V.h, h0), yb = sl_first(V.sh, a + 1, V.h, h0);
    const int xa = sl_first(V.sw, bb - 1, V.w, w0), xb = sl_first(V.sw, bb + 1, V.w, w0);
    const float *dp = df + (size_t)bc * hw0;
    const unsigned char *kp = win + (size_t)bc * hw0;
    float acc = 0.0f;
#pragma unroll 1
    for (int y = ya; y < yb; ++y) {
        const MscTaps ty = msc_taps(V.sh, y, V.h);
        const float wy = (ty.o0 == a ? (float)ty.l0 : 0.0f) + (ty.o1 == a ? (float)ty.l1 : 0.0f);
        float row = 0.0f;
#pragma unroll 1
        for (int x = xa; x < xb; ++x) {
            if (kp[y * w0 + x] != s) continue;
            const MscTaps tx = msc_taps(V.sw, x, V.w);
            const float wx = (tx.o0 == bb ? (float)tx.l0 : 0.0f) + (tx.o1 == bb ? (float)tx.l1 : 0.0f);
            row += (wy * wx) * dp[y * w0 + x];
        }
        acc += row;
    }
    V.g[r] = V.g[r] / den + acc / den0;
}

struct MscPyramid {
    float *out[3];
    int h[3], w[3];
    double sh[3], sw[3];                   // (H - 1) / (h_s - 1): a copy's pixel -> the source coordinate
    unsigned int px0[4];                   // copy s owns the lanes [px0[s], px0[s + 1])
};

__global__ __launch_bounds__(kMscWide) void msc_pyramid_kernel(MscPyramid P, int n, const float *__restrict__ x, int H, int W) {
    const unsigned int e = blockIdx.x * kMscWide + threadIdx.x;
    if (e >= P.px0[n]) return;
    int s = 0;
#pragma unroll
    for (int k = 1; k < 3; ++k)
        if (k < n && e >= P.px0[k]) s = k;
    float *out = P.out[0];
    int h = P.h[0], w = P.w[0];
    double sh = P.sh[0], sw = P.sw[0];
    unsigned int first = 0;
#pragma unroll
    for (int k = 1; k < 3; ++k)
        if (k == s) out = P.out[k], h = P.h[k], w = P.w[k], sh = P.sh[k], sw = P.sw[k], first = P.px0[k];
    const unsigned int t = e - first;
    const int hw = h * w;
    const int b = t / hw, q = t - b * hw, i = q / w, j = q - i * w;
    const MscTaps ty = msc_taps(sh, i, H), tx = msc_taps(sw, j, W);
    const float *xb = x + (size_t)b * 3 * H * W;
    float *o = out + (size_t)t * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *pl = xb + (size_t)c * H * W;
        const double v00 = pl[(size_t)ty.o0 * W + tx.o0], v01 = pl[(size_t)ty.o0 * W + tx.o1];
        const double v10 = pl[(size_t)ty.o1 * W + tx.o0], v11 = pl[(size_t)ty.o1 * W + tx.o1];
        o[c] = (float)(ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11));
    }
}

static double msc_scale(int n_in, int n_out) { return n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 0.0; }

int launch_msc_pyramid_batch(int B, const float *images, int H, int W, int n, const int *h, const int *w, float *const *out,
                             hipStream_t stream) {
    if (!images || !h || !w || !out) return set_error(DSRG_ERR_INVALID, "msc pyramid: NULL images / sizes / outputs");
    if (n < 1 || n > 3) return set_error(DSRG_ERR_INVALID, "msc pyramid: 1..3 copies, got %d", n);
    if (B < 1 || B > kMscMaxBatch) return set_error(DSRG_ERR_INVALID, "msc pyramid: 1..%d images, got %d", kMscMaxBatch, B);
    if (H < 1 || W < 1) return set_error(DSRG_ERR_INVALID, "msc pyramid: images of %dx%d", H, W);
    // (each factor is < 2^31 and B * 3 <= 96: checked in stages, the running products stay far inside 64 bits)
    if ((long long)B * 3 * H >= (1LL << 31) || (long long)B * 3 * H * W >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "msc pyramid: B*3*H*W >= 2^31");
    MscPyramid P;
    long long px = 0;
    P.px0[0] = 0;
    for (int s = 0; s < 3; ++s) {
        if (s >= n) {
            P.out[s] = nullptr, P.h[s] = P.w[s] = 1, P.sh[s] = P.sw[s] = 0.0, P.px0[s + 1] = (unsigned int)px;
            continue;
        }
        if (!out[s]) return set_error(DSRG_ERR_INVALID, "msc pyramid: NULL output %d", s);
        if (h[s] < 1 || w[s] < 1) return set_error(DSRG_ERR_INVALID, "msc pyramid: copy %d of %dx%d", s, h[s], w[s]);
        if ((long long)h[s] * w[s] >= (1LL << 31)) return set_error(DSRG_ERR_INVALID, "msc pyramid: the copies hold >= 2^31 values");
        px += (long long)B * h[s] * w[s];                                     // (B <= 32, h * w < 2^31)
        if (px * 3 >= (1LL << 31)) return set_error(DSRG_ERR_INVALID, "msc pyramid: the copies hold >= 2^31 values");
        P.out[s] = out[s], P.h[s] = h[s], P.w[s] = w[s];
        P.sh[s] = msc_scale(H, h[s]), P.sw[s] = msc_scale(W, w[s]);
        P.px0[s + 1] = (unsigned int)px;
    }
    hipLaunchKernelGGL(msc_pyramid_kernel, dim3((unsigned)((px + kMscWide - 1) / kMscWide)), dim3(kMscWide), 0, stream, P, n, images, H, W);
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

// every shape argument of the pair below, checked by one routine: the workspace size function answers 0 for what the launch refuses
static int msc_check_shapes(int S, int B, int C, const int *h, const int *w, int H, int W, long long *blocks, long long *elements) {
    if (S < 2 || S > kMscMaxMaps) return set_error(DSRG_ERR_INVALID, "msc loss: 2..%d score maps, got %d", kMscMaxMaps, S);
    if (!h || !w) return set_error(DSRG_ERR_INVALID, "msc loss: NULL sizes");
    if (B < 1 || B > kMscMaxBatch) return set_error(DSRG_ERR_INVALID, "msc loss: 1..%d images, got %d", kMscMaxBatch, B);
    if (C < 1) return set_error(DSRG_ERR_INVALID, "msc loss: %d labels", C);
    if (C > kMaxLabels) return set_error(DSRG_ERR_UNSUPPORTED, "msc loss: at most %d labels, got %d", kMaxLabels, C);
    if (H < 1 || W < 1) return set_error(DSRG_ERR_INVALID, "msc loss: label maps %dx%d", H, W);
    if ((long long)B * H >= (1LL << 31) || (long long)B * H * W >= (1LL << 31)) return set_error(DSRG_ERR_INVALID, "msc loss: B*H*W >= 2^31");
    long long nb = 0, ne = 0;
    for (int s = 0; s < S; ++s) {
        if (h[s] < 1 || w[s] < 1) return set_error(DSRG_ERR_INVALID, "msc loss: score map %d is %dx%d", s, h[s], w[s]);
        // (each factor is < 2^31 and B * C <= 3072: the running products stay far inside 64 bits)
        if ((long long)B * C * h[s] >= (1LL << 31) || (long long)B * C * h[s] * w[s] >= (1LL << 31))
            return set_error(DSRG_ERR_INVALID, "msc loss: B*C*h*w >= 2^31 for score map %d", s);
        ne += (long long)B * C * h[s] * w[s];
        nb += ((long long)B * h[s] * w[s] + kMscThreads - 1) / kMscThreads;
    }
    if (ne >= (1LL << 31)) return set_error(DSRG_ERR_INVALID, "msc loss: the score maps hold >= 2^31 values");
    *blocks = nb, *elements = ne;
    return DSRG_OK;
}

static size_t msc_align(size_t n) { return (n + 63) / 64 * 64; }

size_t msc_loss_workspace(int S, int B, int C, const int *h, const int *w, int H, int W) {
    long long nb, ne;
    if (msc_check_shapes(S, B, C, h, w, H, W, &nb, &ne) != DSRG_OK) return 0;
    const size_t n0 = (size_t)B * C * h[0] * w[0];
    return kMscHeadBytes + msc_align((size_t)nb * sizeof(MscPart)) + msc_align(n0 * sizeof(float)) + msc_align(n0);
}

int launch_msc_loss_batch(int S, int B, int C, const float *const *maps, const int *h, const int *w, const float *labels, int H, int W,
                          float ignore_label, float *losses, float *const *grads, unsigned long long *counters, void *workspace,
                          size_t workspace_bytes, hipStream_t stream) {
    if (!maps || !labels || !losses || !grads || !counters || !workspace)
        return set_error(DSRG_ERR_INVALID, "msc loss: NULL maps / labels / losses / grads / counters / workspace");
    long long nb, ne;
    if (int rc = msc_check_shapes(S, B, C, h, w, H, W, &nb, &ne)) return rc;
    for (int s = 0; s < S; ++s)
        if (!maps[s] || !grads[s]) return set_error(DSRG_ERR_INVALID, "msc loss: NULL score map or gradient %d", s);
    const size_t need = msc_loss_workspace(S, B, C, h, w, H, W);
    if (workspace_bytes < need) return set_error(DSRG_ERR_INVALID, "msc loss: workspace of %zu B, %zu needed", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return set_error(DSRG_ERR_INVALID, "msc loss: the workspace must be 8-byte aligned");
    MscMaps M;
    M.blk0[0] = M.el0[0] = 0;
    for (int s = 0; s < kMscMaxMaps; ++s) {
        const int k = s < S ? s : 0;                                          // (entries beyond S are never used: copies of map 0)
        M.z[s] = maps[k], M.g[s] = grads[k], M.h[s] = h[k], M.w[s] = w[k];
        M.sh[s] = msc_scale(h[k], h[0]), M.sw[s] = msc_scale(w[k], w[0]);
        const long long px = s < S ? (long long)B * h[s] * w[s] : 0;
        M.blk0[s + 1] = M.blk0[s] + (unsigned int)((px + kMscThreads - 1) / kMscThreads);
        M.el0[s + 1] = M.el0[s] + (unsigned int)(px * C);
    }
    unsigned char *base = static_cast<unsigned char *>(workspace);
    unsigned long long *head = reinterpret_cast<unsigned long long *>(base);
    MscPart *parts = reinterpret_cast<MscPart *>(base + kMscHeadBytes);
    const size_t n0 = (size_t)B * C * h[0] * w[0];
    float *df = reinterpret_cast<float *>(base + kMscHeadBytes + msc_align((size_t)nb * sizeof(MscPart)));
    unsigned char *win = reinterpret_cast<unsigned char *>(df) + msc_align(n0 * sizeof(float));
    hipLaunchKernelGGL(msc_main_kernel, dim3((unsigned)nb), dim3(kMscThreads), 0, stream, M, S, B, C, labels, H, W, ignore_label, df, win, parts);
    DSRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(msc_reduce_kernel, dim3(1), dim3(kMscWide), 0, stream, M, S, static_cast<const MscPart *>(parts), head, losses, counters);
    DSRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(msc_finish_kernel, dim3((unsigned)((ne + kMscWide - 1) / kMscWide)), dim3(kMscWide), 0, stream, M, S, C,
                       static_cast<const unsigned long long *>(head), static_cast<const float *>(df), static_cast<const unsigned char *>(win));
    DSRG_LAUNCH_CHECK();
    return DSRG_OK;
}

}  // namespace dsrg
