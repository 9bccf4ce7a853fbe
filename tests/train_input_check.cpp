// The host argument checks of the training-input launchers (dsrg_amd/csrc/train_input_check.h) on what the library cannot show
// without a GPU: ACCEPTED inputs and the argument blocks they fill, and the extremes of offsets and sizes.  A stand-alone
// program built with -fsanitize=address,undefined by tests/test_train_input_refusals.py; includes nothing but that header.
// No device pointer is dereferenced: the checks only look at the addresses.
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "train_input_check.h"

static int g_code;
static char g_msg[512];
int dsrg::set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return g_code = code;
}

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "%s:%d: %s [%s] FAILED: %s (last message: %s)\n", __FILE__, __LINE__, g_entry, g_case, #cond, g_msg); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

using namespace dsrg;
typedef std::vector<int32_t> V;
static const char *g_entry = "", *g_case = "";
static const int kE = DSRG_ERR_INVALID, kU = DSRG_ERR_UNSUPPORTED;
static unsigned char *const kStage = (unsigned char *)(uintptr_t)256;          // made-up device pointers, 4-aligned
static float *const kOut = (float *)(uintptr_t)4096;
static const float kMean[3] = {104.0f, 117.0f, 123.0f};

// one call's inputs, for any of the four entries ('s', 'c', 'f', 'x' = f scaled); B images of 4 x 5 laid out as the argument
// tests of the library do: images 256 bytes apart from 0, second pieces 64 bytes apart from `second`, train-s label ids from 3/4
struct In {
    char entry;
    int B;
    size_t nbytes;
    V off, H, W, mir, coff, nc, loff, nl, top, left, Hs, Ws;
    int S = 5, Sw = 6, C = 21, Hm = 5, Wm = 7, ignore = 255, bgr = 1, ch = 17, cw = 13;
    In(char e, int B_, size_t n = 4096) : entry(e), B(B_), nbytes(n) {
        const int second = (int)n / 4, third = (int)n / 4 * 3;
        for (int b = 0; b < B; ++b) {
            off.push_back(256 * b), H.push_back(4), W.push_back(5), mir.push_back(b % 3 == 1 ? 7 : 0);
            coff.push_back(second + 64 * b), nc.push_back(b % 6), loff.push_back(e == 's' ? third + 16 * b : second + 64 * b);
            nl.push_back(b % 3), top.push_back(b), left.push_back(2 * b + 1), Hs.push_back(6 + b), Ws.push_back(3 + b);
        }
    }
};

static TsArgs g_s;
static TcArgs g_c;
static TfScaledArgs g_x;

static int run(const In &i) {
    g_code = DSRG_OK, g_msg[0] = 0;
    memset(&g_s, 0xEE, sizeof(g_s)), memset(&g_c, 0xEE, sizeof(g_c)), memset(&g_x, 0xEE, sizeof(g_x));    // the checks clear what they fill
    int rc;
    if (i.entry == 's')
        rc = check_train_s_input(i.B, kStage, i.nbytes, i.off.data(), i.H.data(), i.W.data(), i.coff.data(), i.nc.data(), i.loff.data(),
                                 i.nl.data(), i.mir.data(), i.S, i.C, i.Hm, i.Wm, kMean, kOut, kOut, kOut, g_s);
    else if (i.entry == 'c')
        rc = check_train_s_cuemap_input(i.B, kStage, i.nbytes, i.off.data(), i.H.data(), i.W.data(), i.coff.data(), i.mir.data(), i.S,
                                        i.Sw, i.C, 96, i.Hm, i.Wm, kMean, i.ignore, i.bgr, kOut, kOut, kOut, g_c);
    else if (i.entry == 'f')
        rc = check_train_f_input(i.B, kStage, i.nbytes, i.off.data(), i.loff.data(), i.H.data(), i.W.data(), NULL, NULL, i.top.data(),
                                 i.left.data(), i.mir.data(), i.ch, i.cw, kMean, 0.5f, 255.0f, kOut, kOut, g_x.f, NULL);
    else
        rc = check_train_f_input(i.B, kStage, i.nbytes, i.off.data(), i.loff.data(), i.H.data(), i.W.data(), i.Hs.data(), i.Ws.data(),
                                 i.top.data(), i.left.data(), i.mir.data(), i.ch, i.cw, kMean, 0.5f, 255.0f, kOut, kOut, g_x.f, &g_x);
    CHECK(rc == g_code);                                                     // a refusal went through set_error, an acceptance did not
    return rc;
}

static bool refused(const In &i, int code, const char *word) { return run(i) == code && strstr(g_msg, word) != NULL; }

// slots [0, B) of a block's array equal the input, slots [B, 32) are zero
static bool slots(const int *a, const V &v, int B) {
    for (int b = 0; b < kTiMaxBatch; ++b)
        if (a[b] != (b < B ? v[b] : 0)) return false;
    return true;
}
template <class Args> static bool shared_fields(const Args &a, const In &i) {
    unsigned bits = 0;
    for (int b = 0; b < i.B; ++b) bits |= i.mir[b] ? 1u << b : 0u;
    return slots(a.img_off, i.off, i.B) && slots(a.H, i.H, i.B) && slots(a.W, i.W, i.B) && a.mirror == bits && a.mean[0] == kMean[0] &&
           a.mean[1] == kMean[1] && a.mean[2] == kMean[2];
}

// an accepted call fills its block with the inputs, field by field
static void accepted(const In &i) {
    CHECK(run(i) == DSRG_OK);
    if (i.entry == 's') {
        CHECK(shared_fields(g_s, i));
        CHECK(slots(g_s.cue_off, i.coff, i.B) && slots(g_s.ncue, i.nc, i.B) && slots(g_s.lab_off, i.loff, i.B) && slots(g_s.nlab, i.nl, i.B));
    } else if (i.entry == 'c') {
        CHECK(shared_fields(g_c, i) && slots(g_c.cue_off, i.coff, i.B));
        for (int b = 0; b < kTiMaxBatch; ++b) CHECK(g_c.sh[b] == 0.0 && g_c.sw[b] == 0.0);         // the launcher's to fill
    } else {
        const TfArgs &f = g_x.f;
        CHECK(shared_fields(f, i) && slots(f.lab_off, i.loff, i.B) && slots(f.top, i.top, i.B) && slots(f.left, i.left, i.B));
        CHECK(f.scale == 0.5f && f.ignore_label == 255.0f);
        if (i.entry == 'x') {
            CHECK(slots(g_x.Hs, i.Hs, i.B) && slots(g_x.Ws, i.Ws, i.B));
            for (int b = 0; b < kTiMaxBatch; ++b) CHECK(g_x.ys[b] == 0.0 && g_x.xs[b] == 0.0);     // the launcher's to fill
        }
    }
}

// a piece of `bytes` bytes at v[1]: ending exactly at the buffer's end it is accepted, with the buffer one byte shorter it is
// refused as lying outside; the offsets INT32_MIN, -1 and INT32_MAX are refused
static void piece(const In &base, V In::*v, long long bytes, const char *what) {
    g_case = what;
    In i = base;
    (i.*v)[1] = (int32_t)((long long)i.nbytes - bytes);
    accepted(i);
    i.nbytes -= 1;
    CHECK(refused(i, kE, "outside"));
    const int32_t extremes[3] = {INT32_MIN, -1, INT32_MAX};
    for (int k = 0; k < 3; ++k) {
        i = base;
        (i.*v)[1] = extremes[k];
        CHECK(run(i) == kE && (strstr(g_msg, "outside") || strstr(g_msg, "aligned")));            // (an odd offset of int32 data is misaligned first)
    }
}

static void entry(char e, const char *name) {
    g_entry = name;
    const int big = e == 'c' ? kE : kU;                                      // what the entry answers its 2^31 limits with
    const In base(e, 3);
    g_case = "baseline";
    accepted(base);
    g_case = "32 images";
    In full(e, 32, 1 << 16);
    for (int b = 0; b < 32; ++b) full.mir[b] = 1 + b;
    accepted(full);
    CHECK((e == 's' ? g_s.mirror : e == 'c' ? g_c.mirror : g_x.f.mirror) == 0xFFFFFFFFu);
    In more = full;
    more.B = 33;
    CHECK(refused(more, kE, "1..32 images"));

    piece(base, &In::off, 4 * 5 * 3, "image");
    if (e == 's') {
        piece(base, &In::coff, 12LL * base.nc[1], "cue triplets");
        piece(base, &In::loff, 4LL * base.nl[1], "label ids");
    } else if (e == 'c') {
        piece(base, &In::coff, 5 * 7, "cue map");
    } else {
        piece(base, &In::loff, 4 * 5, "label");
    }

    g_case = "2^31 limits";
    In i = base;
    i.H[2] = i.W[2] = 32768;                                                 // 3 * 2^30 values: no int holds the product
    CHECK(refused(i, big, "image 2 holds >= 2^31 values"));
    i = base;
    i.nbytes = (size_t)1 << 31;
    CHECK(refused(i, big, "staging buffer holds >= 2^31 bytes"));
    i.nbytes -= 1;                                                           // the largest buffer taken
    accepted(i);
    i = full;
    if (e == 's' || e == 'c') i.S = i.Sw = 4800; else i.ch = i.cw = 4800;    // 32 * 3 * 4800^2
    CHECK(refused(i, big, "2^31 values"));
    if (e == 's' || e == 'c') {
        i = full, i.C = 64, i.Hm = i.Wm = 1024, i.nbytes = (size_t)1 << 30;                        // 32 * 64 * 2^20 = 2^31
        for (int b = 0; b < 32; ++b) i.coff[b] = (b + 1) << 20, i.nc[b] = 0;
        CHECK(refused(i, big, "cues hold"));
        i.C = 63;
        accepted(i);
    }
    if (e == 'c') {
        i = base, i.S = i.Sw = 46341;
        CHECK(refused(i, kE, "images hold"));
        i = base, i.C = 97;
        CHECK(refused(i, kU, "at most 96"));                                 // the one UNSUPPORTED of this entry
        i.C = 96;
        accepted(i);
    }
    if (e == 'f' || e == 'x') {
        i = base, i.top[1] = INT32_MAX - 17;                                 // top + ch = 2^31 - 1: the last one taken
        accepted(i);
        i.top[1] += 1;
        CHECK(refused(i, kU, "offset + crop >= 2^31"));
        i = base, i.left[2] = INT32_MAX;
        CHECK(refused(i, kU, "offset + crop >= 2^31"));
    }
    if (e == 'x') {
        i = base, i.Hs[1] = i.Ws[1] = 46340;                                 // 46340^2 < 2^31 <= 46341^2
        accepted(i);
        i.Hs[1] = i.Ws[1] = 46341;
        CHECK(refused(i, kU, "holds >= 2^31 pixels"));
        i.Hs[1] = i.Ws[1] = INT32_MAX;
        CHECK(refused(i, kU, "holds >= 2^31 pixels"));
    }
}

int main() {
    entry('s', "train-s");
    entry('c', "train-s cue-map");
    entry('f', "train-f");
    entry('x', "train-f scaled");
    printf("all properties hold\n");
    return 0;
}
