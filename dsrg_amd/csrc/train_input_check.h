// Host-side argument checks of the four training-input launchers (train_input.hip) and the argument blocks they fill.  Integer
// arithmetic on sizes and byte offsets, no HIP, so that accepted inputs too can be checked on a CPU, under sanitizers
// (tests/train_input_check.cpp).  What needs HIP (the per-image scales, the grid) the launcher adds after a check returned DSRG_OK
#pragma once
#include <string.h>
#include "../../include/dsrg_hip.h"

namespace dsrg {
int set_error(int code, const char *fmt, ...);
constexpr int kTiMaxBatch = 32;

struct TsArgs {
    int img_off[kTiMaxBatch], H[kTiMaxBatch], W[kTiMaxBatch];       // (H, W, 3) RGB uint8 at stage + img_off
    int cue_off[kTiMaxBatch], ncue[kTiMaxBatch];                    // (3, K) int32 at stage + cue_off: classes, rows, columns
    int lab_off[kTiMaxBatch], nlab[kTiMaxBatch];                    // L int32 class ids at stage + lab_off
    unsigned mirror;                                                // bit b: image b is mirrored
    float mean[3];                                                  // of the OUTPUT channels (B, G, R)
};

struct TcArgs {
    int img_off[kTiMaxBatch], H[kTiMaxBatch], W[kTiMaxBatch];       // (H, W, 3) RGB uint8 at stage + img_off
    int cue_off[kTiMaxBatch];                                       // (Hm, Wm) uint8 cue bytes at stage + cue_off
    double sh[kTiMaxBatch], sw[kTiMaxBatch];                        // zoom_axis_scale(H, Sh), zoom_axis_scale(W, Sw): divided once, on the host
    unsigned mirror;                                                // bit b: image b is mirrored
    float mean[3];                                                  // of the OUTPUT channels
};

struct TfArgs {
    int img_off[kTiMaxBatch], lab_off[kTiMaxBatch];                 // (H, W, 3) RGB uint8 / (H, W) uint8
    int H[kTiMaxBatch], W[kTiMaxBatch], top[kTiMaxBatch], left[kTiMaxBatch];
    unsigned mirror;
    float mean[3], scale, ignore_label;
};
struct TfScaledArgs {
    TfArgs f;
    int Hs[kTiMaxBatch], Ws[kTiMaxBatch];                           // the size image b is rescaled to before the crop
    double ys[kTiMaxBatch], xs[kTiMaxBatch];                        // axis_scale(H, Hs), axis_scale(W, Ws): divided once, on the host
};

// `n` bytes at byte offset `off` lie inside the staging buffer?
inline bool inside(long long off, long long n, size_t stage_bytes) { return off >= 0 && n >= 0 && (unsigned long long)off + n <= stage_bytes; }

// What every entry checks, under its message prefix `name` and the code `big` that it answers the 2^31 limits with; `null`: its words for
// the first NULL array or output, if any; `outputs`: their addresses or-ed.  Clears `a`, fills its img_off, H, W, mirror and mean
template <class Args>
int check_ti_shared(const char *name, int big, const char *null, int B, const unsigned char *stage, size_t stage_bytes, uintptr_t outputs,
                    const int32_t *image_off, const int32_t *H, const int32_t *W, const int32_t *mirror, const float *mean, Args &a) {
    if (B < 1 || B > kTiMaxBatch) return set_error(DSRG_ERR_INVALID, "%s: 1..%d images, got %d", name, kTiMaxBatch, B);
    if (!stage || null) return set_error(DSRG_ERR_INVALID, "%s: NULL %s", name, stage ? null : "staging buffer");
    if (outputs & 3) return set_error(DSRG_ERR_INVALID, "%s: an output is not aligned to a float", name);
    if (stage_bytes >= ((size_t)1 << 31)) return set_error(big, "%s: staging buffer holds >= 2^31 bytes", name);
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < B; ++b) {
        if (H[b] < 1 || W[b] < 1) return set_error(DSRG_ERR_INVALID, "%s: image %d is %dx%d", name, b, H[b], W[b]);
        if ((long long)H[b] * W[b] * 3 >= (1LL << 31)) return set_error(big, "%s: image %d holds >= 2^31 values", name, b);
        if (!inside(image_off[b], (long long)H[b] * W[b] * 3, stage_bytes))
            return set_error(DSRG_ERR_INVALID, "%s: image %d lies outside the staging buffer", name, b);
        a.img_off[b] = image_off[b], a.H[b] = H[b], a.W[b] = W[b], a.mirror |= (mirror[b] ? 1u : 0u) << b;
    }
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c];
    return DSRG_OK;
}

inline int check_train_s_input(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *H, const int32_t *W,
                               const int32_t *cue_off, const int32_t *ncues, const int32_t *label_off, const int32_t *nlabels,
                               const int32_t *mirror, int S, int C, int Hm, int Wm, const float *mean, const float *images,
                               const float *cues, const float *labels, TsArgs &a) {
    const char *null = !image_off || !H || !W ? "image offset / image size array" : !cue_off || !ncues || !label_off || !nlabels
        ? "cue / label descriptor array" : !mirror || !mean ? "mirror / mean array" : !images || !cues || !labels ? "output" : NULL;
    if (S < 1 || C < 1 || Hm < 1 || Wm < 1) return set_error(DSRG_ERR_INVALID, "train-s input: size %d, %d classes, %dx%d planes", S, C, Hm, Wm);
    if ((long long)B * 3 * S * S >= (1LL << 31))
        return set_error(DSRG_ERR_UNSUPPORTED, "train-s input: images hold %lld >= 2^31 values", (long long)B * 3 * S * S);
    if ((long long)B * C * Hm * Wm >= (1LL << 31))
        return set_error(DSRG_ERR_UNSUPPORTED, "train-s input: cues hold %lld >= 2^31 values", (long long)B * C * Hm * Wm);
    if (int rc = check_ti_shared("train-s input", DSRG_ERR_UNSUPPORTED, null, B, stage, stage_bytes,
                                 (uintptr_t)images | (uintptr_t)cues | (uintptr_t)labels, image_off, H, W, mirror, mean, a)) return rc;
    for (int b = 0; b < B; ++b) {
        if (ncues[b] < 0 || nlabels[b] < 0) return set_error(DSRG_ERR_INVALID, "train-s input: image %d has a negative cue / label count", b);
        if (((uintptr_t)stage + (uintptr_t)(uint32_t)cue_off[b]) & 3 || ((uintptr_t)stage + (uintptr_t)(uint32_t)label_off[b]) & 3)
            return set_error(DSRG_ERR_INVALID, "train-s input: cues / labels of image %d are not aligned to an int32", b);
        if (!inside(cue_off[b], 12LL * ncues[b], stage_bytes))
            return set_error(DSRG_ERR_INVALID, "train-s input: cues of image %d lie outside the staging buffer", b);
        if (!inside(label_off[b], 4LL * nlabels[b], stage_bytes))
            return set_error(DSRG_ERR_INVALID, "train-s input: labels of image %d lie outside the staging buffer", b);
        a.cue_off[b] = cue_off[b], a.ncue[b] = ncues[b], a.lab_off[b] = label_off[b], a.nlab[b] = nlabels[b];
    }
    return DSRG_OK;
}

// `max_classes`: kMaxLabels, the flags of the kernel's LDS.  Answers its 2^31 limits with DSRG_ERR_INVALID (include/dsrg_hip.h)
inline int check_train_s_cuemap_input(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *H,
                                      const int32_t *W, const int32_t *cue_off, const int32_t *mirror, int Sh, int Sw, int C, int max_classes,
                                      int Hm, int Wm, const float *mean, int ignore_label, int bgr, const float *images, const float *cues,
                                      const float *labels, TcArgs &a) {
    const char *null = !image_off || !H || !W ? "image offset / image size array" : !cue_off ? "cue offset array" : !mirror || !mean
        ? "mirror / mean array" : !images ? "images output" : !cues ? "cues output" : !labels ? "labels output" : NULL;
    if (Sh < 1 || Sw < 1 || C < 1 || Hm < 1 || Wm < 1)
        return set_error(DSRG_ERR_INVALID, "train-s cue-map input: size %dx%d, %d classes, %dx%d maps", Sh, Sw, C, Hm, Wm);
    if (C > max_classes) return set_error(DSRG_ERR_UNSUPPORTED, "train-s cue-map input: %d classes, at most %d", C, max_classes);
    if (ignore_label < 0 || ignore_label > 255)
        return set_error(DSRG_ERR_INVALID, "train-s cue-map input: ignore_label %d is no byte value", ignore_label);
    if (bgr != 0 && bgr != 1) return set_error(DSRG_ERR_INVALID, "train-s cue-map input: bgr must be 0 or 1, got %d", bgr);
    if ((long long)Sh * Sw >= (1LL << 31) || (long long)B * 3 * Sh * Sw >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "train-s cue-map input: images hold >= 2^31 values (%d x 3 x %d x %d)", B, Sh, Sw);
    if ((long long)Hm * Wm >= (1LL << 31) || (long long)B * C * Hm * Wm >= (1LL << 31))
        return set_error(DSRG_ERR_INVALID, "train-s cue-map input: cues hold >= 2^31 values (%d x %d x %d x %d)", B, C, Hm, Wm);
    if (int rc = check_ti_shared("train-s cue-map input", DSRG_ERR_INVALID, null, B, stage, stage_bytes,
                                 (uintptr_t)images | (uintptr_t)cues | (uintptr_t)labels, image_off, H, W, mirror, mean, a)) return rc;
    for (int b = 0; b < B; ++b)
        if (!inside(cue_off[b], (long long)Hm * Wm, stage_bytes))
            return set_error(DSRG_ERR_INVALID, "train-s cue-map input: cue map %d lies outside the staging buffer", b);
    memcpy(a.cue_off, cue_off, B * sizeof(int32_t));
    return DSRG_OK;
}

// the two stage-2 entries.  `sa`: NULL, or the block of the scaled entry, whose `f` is `a`: then Hs and Ws are checked and filled too
inline int check_train_f_input(int B, const unsigned char *stage, size_t stage_bytes, const int32_t *image_off, const int32_t *label_off,
                               const int32_t *H, const int32_t *W, const int32_t *Hs, const int32_t *Ws, const int32_t *top,
                               const int32_t *left, const int32_t *mirror, int ch, int cw, const float *mean, float scale, float ignore_label,
                               const float *data, const float *label, TfArgs &a, TfScaledArgs *sa) {
    const char *null = !image_off || !label_off || !H || !W ? "offset / image size array" : !top || !left || !mirror || !mean
        ? "top / left / mirror / mean array" : !data || !label ? "output" : sa && (!Hs || !Ws) ? "scaled size array" : NULL;
    if (ch < 1 || cw < 1) return set_error(DSRG_ERR_INVALID, "train-f input: crop %dx%d", ch, cw);
    if ((long long)B * 3 * ch * cw >= (1LL << 31))
        return set_error(DSRG_ERR_UNSUPPORTED, "train-f input: data holds %lld >= 2^31 values", (long long)B * 3 * ch * cw);
    if (sa) memset(sa, 0, sizeof(*sa));
    if (int rc = check_ti_shared("train-f input", DSRG_ERR_UNSUPPORTED, null, B, stage, stage_bytes, (uintptr_t)data | (uintptr_t)label,
                                 image_off, H, W, mirror, mean, a)) return rc;
    for (int b = 0; b < B; ++b) {
        if (top[b] < 0 || left[b] < 0) return set_error(DSRG_ERR_INVALID, "train-f input: image %d has a negative offset (%d, %d)", b, top[b], left[b]);
        if ((long long)top[b] + ch >= (1LL << 31) || (long long)left[b] + cw >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "train-f input: image %d has an offset + crop >= 2^31", b);
        if (!inside(label_off[b], (long long)H[b] * W[b], stage_bytes))
            return set_error(DSRG_ERR_INVALID, "train-f input: label %d lies outside the staging buffer", b);
        a.lab_off[b] = label_off[b], a.top[b] = top[b], a.left[b] = left[b];
        if (!sa) continue;
        if (Hs[b] < 1 || Ws[b] < 1) return set_error(DSRG_ERR_INVALID, "train-f input: image %d is rescaled to %dx%d", b, Hs[b], Ws[b]);
        if ((long long)Hs[b] * Ws[b] >= (1LL << 31))
            return set_error(DSRG_ERR_UNSUPPORTED, "train-f input: image %d rescaled to %dx%d holds >= 2^31 pixels", b, Hs[b], Ws[b]);
        sa->Hs[b] = Hs[b], sa->Ws[b] = Ws[b];
    }
    a.scale = scale, a.ignore_label = ignore_label;
    return DSRG_OK;
}

}  // namespace dsrg
