/*
 * dsrg_hip.h — C ABI of libdsrg_hip.so, the MI355X (gfx950) implementation of
 * the DSRG per-iteration supervision path.
 *
 * Every entry point replaces one interface of the reference (speedinghzl/DSRG);
 * the reference file:line it stands in for is cited on each declaration.  The
 * library has no CPU fallback: every compute entry point launches HIP kernels
 * and returns an error code when no device / too large a problem is given.
 *
 * Conventions
 *   - return value: 0 = DSRG_OK, negative = error (dsrg_last_error() has text)
 *   - "dev" pointers are device (HBM) pointers owned by the caller; "host"
 *     pointers are ordinary host memory
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); device
 *     entry points are stream-ordered and never synchronise the host
 *   - layouts: blobs are NCHW float32, C-contiguous, exactly like the Caffe
 *     blobs the reference's Python layers see (pylayers.py)
 *   - threads: a handle (dsrg_ctx_t, dsrg_crf_t) is used by one host thread at a
 *     time; different handles, and the handle-free entry points, may be called
 *     from different host threads concurrently (the library's shared tables are
 *     atomics; dsrg_last_error() is per thread).  Results do not depend on the
 *     interleaving (tests/test_gpu_parity.py::test_four_host_threads_four_contexts)
 */
#ifndef DSRG_HIP_H
#define DSRG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

#define DSRG_OK 0
#define DSRG_ERR_INVALID (-1)      /* bad argument */
#define DSRG_ERR_HIP (-2)          /* HIP runtime error (no device, launch failure, ...) */
#define DSRG_ERR_UNSUPPORTED (-3)  /* problem does not fit the implemented kernels */
#define DSRG_ERR_NOMEM (-4)

const char *dsrg_last_error(void);
/* number of visible HIP devices (0 when there is none); never fails */
int dsrg_device_count(void);
/* Page-lock `bytes` of ordinary host memory at `host` in place (hipHostRegister), so that the copies between a Caffe blob
 * (pylayers.py: bottom[i].data / top[i].data are host arrays the framework owns) and HBM run as DMA instead of through a
 * bounce buffer.  Returns 1 = registered by this call, 0 = left alone: memory HIP already knows (page-locked by its owner —
 * a hipHostMalloc'ed blob of a GPU-mode Caffe, a pinned torch tensor — or overlapping an earlier registration) or a refused
 * registration.  Never fails and never leaves a HIP error behind for the next launch check to trip over.
 * dsrg_host_unregister undoes a registration made here (call it only for pointers that returned 1); same guarantees. */
int dsrg_host_register(void *host, size_t bytes);
int dsrg_host_unregister(void *host);

/* ------------------------------------------------------------------------ */
/* 1. Single-image dense-CRF object: mirrors the C++ class DenseCRFWrapper     */
/*    (CRF/include/densecrf_wrapper.h:3-28) that the Cython class DenseCRF     */
/*    (CRF/krahenbuhl2013/wrapper.pyx:5-17,20-60) binds.  Host pointers, one   */
/*    image, synchronous — exactly the reference's calling convention.         */
/* ------------------------------------------------------------------------ */
typedef struct dsrg_crf_s *dsrg_crf_t;

/* DenseCRFWrapper::DenseCRFWrapper(int W, int H, int nlabels)  densecrf_wrapper.cpp:5-8 */
int dsrg_crf_create(int W, int H, int nlabels, dsrg_crf_t *out);
/* The same object for `nimages` (1 .. 8) same-sized images per call: what the reference's test-time loops do one image at
 * a time (training/tools/test-ms.py:84-111, generate_train_gt.py:78-106: CRF() per image over 10 582 images) as ONE set of
 * launches — the lattices of the batch are built together (every key carries its image's number, so images share no vertex)
 * and every splat / blur / slice launch of the mean-field loop carries all of them.  The unary, image, result and label
 * buffers of the calls below then hold the images back to back ((nimages, H, W, nlabels) / (nimages, H, W, 3) / (nimages, H,
 * W)); dsrg_crf_npixels returns nimages * W * H.  Results equal nimages single-image calls bit for bit.  Always the
 * global-memory path; DSRG_ERR_UNSUPPORTED at inference when a spatial kernel is so narrow that the image number does not fit
 * beside its lattice coordinates (theta_gamma below ~0.3 pixel at 500 pixels a side): filter such images one at a time. */
int dsrg_crf_create_batch(int W, int H, int nlabels, int nimages, dsrg_crf_t *out);
/* DenseCRFWrapper::~DenseCRFWrapper                             densecrf_wrapper.cpp:10-12 */
int dsrg_crf_destroy(dsrg_crf_t h);
/* The four data pointers of this object API (`unary_host`, `im_host`, `out_host`, `labels_host`) may be host OR device
 * pointers — the copies use hipMemcpyDefault — so a device-resident caller (dsrg_amd/inference.py) skips the PCIe trips.
 * DenseCRFWrapper::set_unary_energy(float*)                     densecrf_wrapper.cpp:32-37
 * unary_host: [W*H*nlabels], label-fastest (copied). */
int dsrg_crf_set_unary_energy(dsrg_crf_t h, const float *unary_host);
/* DenseCRFWrapper::add_pairwise_energy(...)                     densecrf_wrapper.cpp:19-30
 * Gaussian potential (w2, theta_gamma) first, then bilateral (w1, theta_alpha,
 * theta_beta), both Potts.  im_host: [W*H*3] uint8, not retained. */
int dsrg_crf_add_pairwise_energy(dsrg_crf_t h, float w1, float theta_alpha_1, float theta_alpha_2,
                                 float theta_beta_1, float theta_beta_2, float theta_beta_3,
                                 float w2, float theta_gamma_1, float theta_gamma_2,
                                 const unsigned char *im_host);
/* DenseCRFWrapper::inference(int, float*)                       densecrf_wrapper.cpp:45-50
 * out_host: [W*H*nlabels] label-fastest marginals. */
int dsrg_crf_inference(dsrg_crf_t h, int n_iters, float *out_host);
/* DenseCRFWrapper::map(int, int*)                               densecrf_wrapper.cpp:39-43 */
int dsrg_crf_map(dsrg_crf_t h, int n_iters, int32_t *labels_host);
/* dsrg_crf_map restricted to the labels known to be in the image — the selection of training/tools/generate_train_gt.py:98-104
 * (probs[:, :, [0] + labels], np.argmax, labels[...]) on the final marginals.  select_host: HOST array of one ordered list per
 * image of the object (one for dsrg_crf_create objects, `nimages` for batched ones), list b at select_host + b * select_stride,
 * nselect_host[b] entries (1..128, <= select_stride), each a label of [0, nlabels); duplicates and any order are allowed.  The
 * label of a pixel is sel[j], j the FIRST index that maximises Q[sel[j]].  ignore_below > 0: pixels whose largest marginal over
 * ALL labels is below it get 255 (the reference's commented-out line 104); <= 0: off.  The lists are copied before the call
 * returns.  Every argument is checked before the first device call.  Stream, async and labels_host (host or device pointer,
 * [npixels]) exactly as dsrg_crf_map. */
int dsrg_crf_map_select(dsrg_crf_t h, int n_iters, const int32_t *select_host, const int32_t *nselect_host, int select_stride,
                        float ignore_below, int32_t *labels_host);
/* Where an object's copies and kernels run (default: the null stream, every call synchronous as the reference's).  With
 * async != 0 the entry points enqueue and return: buffers passed in must be device (or pinned host) memory that stays valid,
 * results are final after dsrg_crf_synchronize.  Objects on different streams overlap their launches — how a test-time loop
 * (training/tools/test-ms.py:84-111) keeps several images in flight (dsrg_amd.crf.CRF_device_many). */
int dsrg_crf_set_stream(dsrg_crf_t crf, void *stream, int async);
int dsrg_crf_synchronize(dsrg_crf_t crf);
/* DenseCRFWrapper::npixels / nlabels                            densecrf_wrapper.cpp:14-15 */
int dsrg_crf_npixels(dsrg_crf_t h);
int dsrg_crf_nlabels(dsrg_crf_t h);
/* introspection (tests): vertex count of lattice k (0 Gaussian, 1 bilateral), -1 if not built */
int dsrg_crf_lattice_size(dsrg_crf_t h, int k);
/* introspection for the parity tests, objects on the global-memory path only (maps beyond DSRG_CTX_MAX_PIXELS, and every object of
 * dsrg_crf_create_batch): the counterparts of dsrg_ctx_lattice_dump / dsrg_ctx_lattice_norm / dsrg_ctx_filter_once in section 2,
 * for image b (0 for a one-image object) of the last add_pairwise_energy.  kind 0 = Gaussian, 1 = bilateral lattice.
 * DSRG_ERR_UNSUPPORTED for an object on the LDS-resident path, DSRG_ERR_INVALID before add_pairwise_energy.  They run on the
 * object's stream and return when done; the lattices are built here if no inference has run since add_pairwise_energy.
 *   dump: arrays as dsrg_ctx_lattice_dump, of ONE image: N = W * H pixels, *m_host = the image's vertex count (the vertices
 *         of the image's SSE padding pixels included), ids local to the image in first-occurrence order, the image number
 *         removed from the keys.  Any array may be NULL: call once for *m_host, then with arrays of that size.
 *   norm: norm_host [W*H].
 *   filter_once: x, out [W*H*nlabels] label-fastest, host or device pointers; out = norm . K (norm . x) through the splat,
 *         combine and blur launches of one mean-field iteration (same grids and buffers) and the slice.  The other images of
 *         a batched object filter zeros.  Overwrites the object's marginals (the next inference / map call recomputes them). */
int dsrg_crf_lattice_dump(dsrg_crf_t h, int kind, int b, int32_t *m_host, int16_t *keys_host, int32_t *vid_host,
                          float *bary_host, int32_t *n1_host, int32_t *n2_host);
int dsrg_crf_lattice_norm(dsrg_crf_t h, int kind, int b, float *norm_host);
int dsrg_crf_filter_once(dsrg_crf_t h, int kind, int b, const float *x, float *out);

/* measurement hook (no reference counterpart): while on, every launch of the dominant kernel of this object's path — the
 * splat of the global-memory path (full-resolution maps), the mean-field filter kernel of the LDS-resident path — is
 * bracketed by HIP events on its stream; _stop synchronises and returns the summed time and the launch count. */
int dsrg_crf_profile_start(dsrg_crf_t h, int max_launches);
int dsrg_crf_profile_stop(dsrg_crf_t h, double *total_ms_host, int32_t *launches_host);

/* ------------------------------------------------------------------------ */
/* 2. Batched device context: workspace for B images of (C,H,W) so that the    */
/*    per-iteration path runs without allocation or host synchronisation.      */
/* ------------------------------------------------------------------------ */
typedef struct dsrg_ctx_s *dsrg_ctx_t;

/* pairwise parameters of krahenbuhl2013.CRF (CRF/krahenbuhl2013/CRF.py:25-35);
 * the caller evaluates 80/scale_factor etc. in double and rounds to float, as
 * the Python->Cython call does. */
typedef struct {
    float w_bilateral;      /* 10 */
    float theta_alpha_x;    /* 80 / scale_factor */
    float theta_alpha_y;
    float theta_beta_r;     /* color_factor = 13 */
    float theta_beta_g;
    float theta_beta_b;
    float w_gaussian;       /* 3 */
    float theta_gamma_x;    /* 3 / scale_factor */
    float theta_gamma_y;
    int32_t n_iters;        /* maxiter = 10 */
} dsrg_crf_params;

/* Which maps a context takes is a function of N = H * W alone, never of the images: every lattice is provisioned for its worst
 * case (6 * 4 * ceil(N / 4) vertices for the bilateral kernel, whatever the colours), so that a training run cannot meet a
 * batch that does not fit.  Accepted: N <= DSRG_CTX_MAX_PIXELS (41x41, 65x65 — the maps of 321x321 and 513x513 inputs — up
 * to 66x68; 67x67 is the first square map beyond), C <= 96 labels; anything larger returns DSRG_ERR_UNSUPPORTED here, at
 * creation, with the reason in dsrg_last_error().  Larger maps run on the global-memory path: the object API (section 1,
 * dsrg_crf_create / dsrg_crf_create_batch) for the CRF and the stand-alone layer entry points below for the rest — which is
 * what the Python mirror's supervision_step does for them (dsrg_amd/ops.py). */
#define DSRG_CTX_MAX_PIXELS 4488
int dsrg_ctx_create(int max_batch, int C, int H, int W, dsrg_ctx_t *out);
int dsrg_ctx_destroy(dsrg_ctx_t ctx);

/* CRFLayer.forward (pylayers/pylayers/pylayers.py:63-88) and, identically,
 * DSRGLayer.refinement (pylayers.py:310-331):
 *   probs_dev   (B,C,H,W) f32   clipped IN PLACE to >= 1e-4 (pylayers.py:67,312)
 *   images_dev  (B,3,Hi,Wi) f32 mean-subtracted BGR (bottom[1]); resampled to
 *               (H,W) with the align-corners order-1 zoom, + mean pixel
 *               (104,117,123), round-half-even, cast to uint8 (pylayers.py:70-75)
 *   refined_dev (B,C,H,W) f64   clip(Q,1e-4)/sum  (pylayers.py:84-86) = self.result
 *   logq_dev    (B,C,H,W) f32   log(refined)      (pylayers.py:88); may be NULL
 * images_dev may be NULL when dsrg_crf_prepare_batch has been called for this batch (see below). */
int dsrg_crf_refine_batch(dsrg_ctx_t ctx, int B, float *probs_dev, const float *images_dev,
                          int img_h, int img_w, const dsrg_crf_params *params,
                          double *refined_dev, float *logq_dev, void *stream);
/* The image-dependent half of the CRF — resampling the images to (H,W) and building the bilateral
 * lattices (Permutohedral::init, CRF/src/permutohedral.cpp:140-321) — needs no network output, so a
 * trainer can run it on a side stream underneath the backbone forward.  After this call (and a
 * stream dependency set up by the caller) dsrg_supervision_step may be given images_dev = NULL.
 * The call overwrites the context's lattices: the caller also orders it BEHIND the last call that
 * reads them (the previous step's mean field), e.g. side stream waits on the main stream first.
 * One host synchronisation of `stream` happens on the FIRST call per (shape, kernel widths): the spatial lattice is built
 * once and its "pixel-local" flag is read back so that later filter launches leave its workgroups out of the grid; inside
 * a stream capture the read-back is postponed to the first later call outside one. */
int dsrg_crf_prepare_batch(dsrg_ctx_t ctx, int B, const float *images_dev, int img_h, int img_w,
                           const dsrg_crf_params *params, void *stream);

/* the same mean-field run on caller-prepared inputs (used by krahenbuhl2013.CRF
 * and by tests): unary_dev (B,C,H,W) f32 holds the NEGATED energies -U (i.e.
 * the `unary` argument of CRF.py:28), im_u8_dev (B,H*W,3) uint8, q_dev
 * (B,C,H,W) f32 receives the marginals. */
int dsrg_crf_meanfield_batch(dsrg_ctx_t ctx, int B, const float *neg_unary_dev,
                             const unsigned char *im_u8_dev, const dsrg_crf_params *params,
                             float *q_dev, void *stream);
/* vertex counts of the lattices built by the last refine/meanfield call:
 * m_gauss, and m_bilateral[b] for b < B (host arrays; synchronises the stream) */
int dsrg_ctx_lattice_sizes(dsrg_ctx_t ctx, int B, int32_t *m_gauss_host, int32_t *m_bilateral_host,
                           void *stream);

/* measurement: per lattice, the number of splat entries beyond the first entry of their vertex (the part of the splat that
 * goes through LDS products; bench.py's LDS traffic model).  Host arrays as for dsrg_ctx_lattice_sizes; synchronises. */
int dsrg_ctx_lattice_extras(dsrg_ctx_t ctx, int B, int32_t *x_gauss_host, int32_t *x_bilateral_host, void *stream);
/* measurement: the geometry of one mean-field filter launch over B images as the launcher plans it NOW (label planes per
 * bilateral / per Gaussian workgroup, workgroups in the grid, dynamic LDS bytes) — bench.py's LDS model reads it instead of
 * re-deriving the launcher's rules.  Host pointers, any may be NULL. */
int dsrg_ctx_filter_plan(dsrg_ctx_t ctx, int B, int32_t *planes_bilateral, int32_t *planes_gaussian, int32_t *workgroups,
                         int32_t *lds_bytes);

/* introspection for the parity tests: one lattice as the reference holds it.  kind 0 = the Gaussian lattice (b = 0),
 * kind 1 = the bilateral lattice of image b of the last refine / prepare / meanfield / supervision call.
 *   keys_host [M*d] int16   vertex keys in id order          (HashTable::getKeys, CRF/src/permutohedral.cpp:296-297)
 *   vid_host  [N*(d+1)]     offset_: vertex id of corner r of pixel i, pixel-major   (permutohedral.cpp:272)
 *   bary_host [N*(d+1)]     barycentric_                                             (permutohedral.cpp:274)
 *   n1_host / n2_host [(d+1)*M]  blur_neighbors_[j*M+i].n1 / .n2, -1 = none          (permutohedral.cpp:315-316)
 * Any array may be NULL; *m_host receives M (size the arrays with dsrg_ctx_lattice_sizes first).  Synchronises. */
int dsrg_ctx_lattice_dump(dsrg_ctx_t ctx, int kind, int b, int32_t *m_host, int16_t *keys_host, int32_t *vid_host,
                          float *bary_host, int32_t *n1_host, int32_t *n2_host, void *stream);
/* introspection for the parity tests: norm_host [N] = 1/sqrt(K 1 + 1e-20) of lattice (kind, b) as dsrg_ctx_lattice_dump
 * addresses it (DenseKernel::initLattice, CRF/src/pairwise.cpp:44,54-57).  Synchronises. */
int dsrg_ctx_lattice_norm(dsrg_ctx_t ctx, int kind, int b, float *norm_host, void *stream);
/* introspection for the parity tests: ONE application of the normalised kernel `kind` (0 Gaussian, 1 bilateral),
 * out = norm . K (norm . q)  (DenseKernel::filter, CRF/src/pairwise.cpp:63-80; splat / blur / slice of
 * CRF/src/permutohedral.cpp:529-589), through the kernels and lattices of the inference loop.  q_dev, out_dev (B,C,H,W) f32. */
int dsrg_ctx_filter_once(dsrg_ctx_t ctx, int kind, int B, const float *q_dev, float *out_dev, void *stream);
/* introspection for the parity tests: the float64 marginals (`self.result`, pylayers.py:84-86) the last
 * dsrg_supervision_step thresholded, copied to refined_dev (B,C,H,W) f64 in stream order. */
int dsrg_ctx_read_refined(dsrg_ctx_t ctx, int B, double *refined_dev, void *stream);

/* measurement hook (no reference counterpart): while profiling is on, every launch of the
 * mean-field filter kernel (splat/blur/slice, the dominant kernel) is bracketed by HIP events
 * on the launch stream; _stop synchronises and returns the summed kernel time and launch count. */
int dsrg_ctx_profile_start(dsrg_ctx_t ctx, int max_launches);
int dsrg_ctx_profile_stop(dsrg_ctx_t ctx, double *total_ms_host, int32_t *launches_host);

/* CRFLayer.backward (pylayers.py:90-92): bottom_diff = (1 - refined) * top_diff */
int dsrg_crf_layer_backward(size_t n, const double *refined_dev, const float *top_diff_dev,
                            float *bottom_diff_dev, void *stream);

/* DSRGLayer.forward -> generate_seed -> generate_seed_step (pylayers.py:237-275,
 * 297-304,333-344) incl. CC_lab (CC_labeling_8.py:112-197), given the refined
 * marginals:
 *   labels_dev (B,1,1,C) f32 0/1, cues_dev (B,C,H,W) f32 0/1,
 *   refined_dev (B,C,H,W) f64, seeds_dev (B,C,H,W) f32 0/1 (output),
 *   scratch_dev: B*H*W uint16 of device scratch (the per-pixel classification handed from the
 *   pixel-parallel pass to the per-image growth pass).  C <= 96. */
int dsrg_srg_grow_batch(int B, int C, int H, int W, const float *labels_dev, const float *cues_dev,
                        const double *refined_dev, double th1, double th2, float *seeds_dev,
                        void *scratch_dev, void *stream);

/* SoftmaxLayer.forward / backward (pylayers.py:30-51) */
int dsrg_softmax_forward(int B, int C, int HW, const float *x_dev, float *p_dev, void *stream);
int dsrg_softmax_backward(int B, int C, int HW, const float *x_dev, const float *top_diff_dev,
                          float *bottom_diff_dev, void *stream);

/* BalancedSeedLossLayer.forward / backward (pylayers.py:126-152).
 * loss_dev: one float.  grad_dev may be NULL (forward only). */
int dsrg_seed_loss(int B, int C, int HW, const float *probs_dev, const float *seeds_dev,
                   float *loss_dev, float *grad_dev, void *stream);
/* ConstrainLossLayer.forward / backward (pylayers.py:160-180); grads may be NULL. */
int dsrg_constrain_loss(int B, int C, int HW, const float *probs_dev, const float *logq_dev,
                        float *loss_dev, float *grad_probs_dev, float *grad_logq_dev, void *stream);

/* ---- the pylayers classes no seed_mc prototxt references, and the evaluation histogram ---------------- */
/* SeedLossLayer (pylayers/pylayers/pylayers.py:94-118): L = -mean_b[ sum S log p / sum S ]; loss and/or grad may be NULL. */
int dsrg_seed_loss_plain(int B, int C, int HW, const float *probs_dev, const float *seeds_dev, float *loss_dev,
                         float *grad_dev, void *stream);
/* ExpandLossLayer (pylayers.py:183-233): probs (B,C,HW), class 0 = background; stat (B,C) image-level labels (> 0.5 =
 * present; stat[:,0] ignored); q_fg / q_bg = 0.996 / 0.999 in the reference.  HW <= 8192.  scratch_dev: B*C doubles
 * (needed when loss_dev != NULL).  loss and/or grad may be NULL. */
int dsrg_expand_loss(int B, int C, int HW, const float *probs_dev, const float *stat_dev, double q_fg, double q_bg,
                     float *loss_dev, float *grad_dev, void *scratch_dev, void *stream);
/* ConfusionMatrix.add (rule_lt = 0: pixels with gt != 255) / generateM (rule_lt = 1: gt < nclass) of
 * training/tools/evaluate.py:25-30,61-68.  hist_dev: nclass*nclass + 1 unsigned 64-bit counters that are ADDED to
 * (row = ground truth, column = prediction); the last one counts kept pixels whose gt or prediction is >= nclass.
 * nclass <= 127. */
int dsrg_confusion_matrix(size_t n, const unsigned char *gt_dev, const unsigned char *pred_dev, int nclass, int rule_lt,
                          unsigned long long *hist_dev, void *stream);
/* The full-resolution tail of the multi-scale test (training/tools/test-ms.py:90-103, test-ms-f.py:121-134) in one launch:
 * K score maps (batch 1, (C, h_k, w_k) f32 NCHW, sizes may differ; scores_dev is a HOST array of K device pointers, h_host /
 * w_host host arrays of their sizes) are each zoomed to H x W (order-1 zoom, (in-1)/(out-1) mapping, blended in double and
 * rounded once to f32), summed in f32 in scale order (S), and turned into p = max(softmax_c(S), eps).  Outputs, each optional
 * (NULL = not written, at least one required), label-fastest:
 *   unary_dev  (H, W, C) f32: log(p), the unary CRF_device takes; 16-byte aligned
 *   argmax_dev (H, W) int32: the first maximum of S (a maximum of p: the smooth=False result)
 *   sum_dev    (H, W, C) f32: S itself (parity tests); 16-byte aligned
 * 1 <= K <= 8, 1 <= C <= 96, H, W, h_k, w_k >= 1, H*W*C < 2^31; every argument is checked before the first device call.
 * Stream-ordered, no host synchronisation, no handle (callable from any host thread); bit-reproducible (no atomics). */
int dsrg_multiscale_unary(int K, int C, const float *const *scores_dev, const int32_t *h_host, const int32_t *w_host, int H, int W,
                          float eps, float *unary_dev, int32_t *argmax_dev, float *sum_dev, void *stream);
/* dsrg_multiscale_unary for G images in one launch (the fixed sizes of test-ms.py give every image of a group the same score
 * map sizes): scores_dev is a HOST array of K device pointers to batched maps (Gcap, C, h_k, w_k) f32 NCHW, Gcap >= G, image g
 * reads slice g; H_host / W_host: host arrays of the G output sizes.  unary_dev / argmax_dev / sum_dev: HOST arrays of G device
 * pointers each (layouts and alignment as above), or NULL; a class of outputs is NULL (or all-NULL) or set for every image, and
 * at least one class is required.  Image g's outputs equal dsrg_multiscale_unary's on slice g and (H_g, W_g) bit for bit.
 * 1 <= G <= 16; otherwise the limits of dsrg_multiscale_unary, per image; every argument is checked before the first device
 * call.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_multiscale_unary_batch(int G, int K, int C, const float *const *scores_dev, const int32_t *h_host, const int32_t *w_host,
                                const int32_t *H_host, const int32_t *W_host, float eps, float *const *unary_dev,
                                int32_t *const *argmax_dev, float *const *sum_dev, void *stream);
/* dsrg_multiscale_unary with mirrored maps (horizontal-flip test-time augmentation: the scores of a mirrored network input are
 * mirrored back and summed with the plain ones): mirror_host is a HOST array of K flags, and a map whose flag is non-zero is read
 * with its columns reversed.  The result is defined as dsrg_multiscale_unary's on flip(map, last axis): the sampling
 * coordinates, x0, x1 and the blend weights come from the output pixel as there, only the four loads address columns w-1-x0
 * and w-1-x1; the f32 sum runs in list order.  All flags zero gives dsrg_multiscale_unary's outputs bit for bit.  Limits and
 * checks as there (K <= 8 maps: up to four scales with their mirrors), mirror_host must not be NULL.  Stream-ordered, no host
 * synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_multiscale_unary_mirror(int K, int C, const float *const *scores_dev, const int32_t *mirror_host, const int32_t *h_host,
                                 const int32_t *w_host, int H, int W, float eps, float *unary_dev, int32_t *argmax_dev,
                                 float *sum_dev, void *stream);
/* dsrg_multiscale_unary_mirror for G images at K scales in one launch: scores_dev is a HOST array of K device pointers to batched
 * maps (Gcap, C, h_k, w_k) f32 NCHW with Gcap >= 2 G (the outputs of batch-2G forwards on dsrg_preprocess_rect_mirror_batch's
 * inputs); image g reads slice 2g plain and slice 2g+1 mirrored back.  Per pixel the f32 sum runs scale-major: scale 0 plain,
 * scale 0 mirror, scale 1 plain, ...  Image g's outputs equal dsrg_multiscale_unary_mirror's on those 2K slices in that order
 * (flags 0, 1, 0, 1, ...) and (H_g, W_g) bit for bit.  H_host / W_host and the output arrays as dsrg_multiscale_unary_batch
 * takes them.  1 <= G <= 8, 1 <= K <= 4; otherwise the limits of dsrg_multiscale_unary, per image; every argument is checked
 * before the first device call.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_multiscale_unary_mirror_batch(int G, int K, int C, const float *const *scores_dev, const int32_t *h_host,
                                       const int32_t *w_host, const int32_t *H_host, const int32_t *W_host, float eps,
                                       float *const *unary_dev, int32_t *const *argmax_dev, float *const *sum_dev, void *stream);
/* The full-resolution tail of the weakly supervised pseudo-label pass (training/tools/generate_train_gt.py:85-104) for G images
 * whose score maps are the slices of one batched forward: scores_dev (Gcap >= G, C, h, w) f32 NCHW, image g reads slice g.  First
 * the softmax over labels per MAP pixel in f32 (s - max, expf, sum in label order, divide) into workspace_dev (G * C * h * w
 * floats, the caller's: nothing is allocated here), then the order-1 zoom of those probabilities to (H_g, W_g) ((in-1)/(out-1)
 * mapping, blended in double and rounded once to f32) and p = max(p, eps).  G = 1 is the single-image form.  Outputs: HOST arrays
 * of G device pointers each, or NULL; a class is NULL (or all-NULL) or set for every image, at least one class is required:
 *   unary_dev  (H, W, C) f32 label-fastest: logf(p), the unary CRF_device takes; 16-byte aligned
 *   probs_dev  (H, W, C) f32 label-fastest: p itself (parity tests); 16-byte aligned
 *   labels_dev (H, W) int32: the selection of dsrg_crf_map_select applied to p (the smooth=False result): select_host /
 *              nselect_host / select_stride / ignore_below as there, one list per image; may be NULL when labels_dev is
 * 1 <= G <= 16, 1 <= C <= 96, H_g, W_g, h, w >= 1, H_g*W_g*C < 2^31, h*w*C < 2^31; every argument is checked before the first
 * device call.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics), and image g's outputs do not
 * depend on the group.  It is dsrg_train_gt_ensemble_batch at K = 1, flip = 0 on this one map: the same two kernels, the same
 * workspace, the same return codes; its messages begin with "train-gt unary". */
int dsrg_train_gt_unary_batch(int G, int C, const float *scores_dev, int h, int w, const int32_t *H_host, const int32_t *W_host,
                              float eps, const int32_t *select_host, const int32_t *nselect_host, int select_stride,
                              float ignore_below, float *workspace_dev, float *const *unary_dev, float *const *probs_dev,
                              int32_t *const *labels_dev, void *stream);
/* dsrg_train_gt_unary_batch as a probability ensemble over K sizes, each optionally with its mirror (no counterpart in the
 * reference): scores_dev is a HOST array of K device pointers to batched maps (Gcap, C, h_k, w_k) f32 NCHW (h_host / w_host: host
 * arrays of their sizes).  flip = 0: Gcap >= G, image g reads slice g; flip != 0: Gcap >= 2 G, image g reads slice 2g plain and
 * slice 2g+1 mirrored (the slot layout of dsrg_preprocess_rect_mirror_batch).  The M = K * (1 + flip) maps of an image come in the
 * order scale 0 plain, scale 0 mirror, scale 1 plain, ...  Per map: the softmax over labels per MAP pixel and the order-1 zoom of
 * the probabilities to (H_g, W_g), both with the arithmetic stated at dsrg_train_gt_unary_batch (z_m: blended in double, rounded
 * once to f32); a mirror map is read as flip(map, last axis): coordinates and weights come from the output pixel as for a plain map, only
 * the four loads address columns w-1-x0 and w-1-x1.  Then in f32, in list order: acc = z_0, acc = acc + z_m; p = acc / (float)M
 * (no division at M = 1); p = max(p, eps).  workspace_dev: sum over k of G * (1 + flip) * C * h_k * w_k floats, the caller's
 * (nothing is allocated here).  Outputs (unary_dev = logf(p), probs_dev = p, labels_dev), their classes, alignment and the
 * selection lists as dsrg_train_gt_unary_batch takes them; K = 1 without flip is that entry point (one launcher, one kernel family).
 * 1 <= K, K * (1 + flip) <= 8; 1 <= G <= 16 without flip, <= 8 with it; 1 <= C <= 96; H_g, W_g, h_k, w_k >= 1, H_g*W_g*C < 2^31,
 * h_k*w_k*C < 2^31; every argument is checked before the first device call.  Two launches whatever K is.  Stream-ordered, no host
 * synchronisation, no handle; bit-reproducible (no atomics), and image g's outputs do not depend on the group. */
int dsrg_train_gt_ensemble_batch(int G, int K, int flip, int C, const float *const *scores_dev, const int32_t *h_host,
                                 const int32_t *w_host, const int32_t *H_host, const int32_t *W_host, float eps,
                                 const int32_t *select_host, const int32_t *nselect_host, int select_stride, float ignore_below,
                                 float *workspace_dev, float *const *unary_dev, float *const *probs_dev,
                                 int32_t *const *labels_dev, void *stream);
/* The network inputs of a group of test images in one launch (training/tools/test-ms.py:68-81 for G images at K sizes):
 * images_dev is a HOST array of G device pointers to (H_g, W_g, 3) RGB uint8 images (H_host / W_host: their sizes), sizes_host K
 * target sizes S_k, mean_host the 3 values subtracted from the B, G, R output channels, out_dev a HOST array of K device
 * pointers to (capacity, 3, S_k, S_k) f32 NCHW tensors.  Slot g < G of output k is image g zoomed to S_k x S_k (order-1 zoom,
 * (in-1)/(out-1) mapping, blended in double and rounded once to f32), in BGR order, minus the mean (in f32); slots G..capacity-1
 * are written as zeros.  1 <= G <= 16, G <= capacity, 1 <= K <= 8, all sizes >= 1, H_g*W_g*3 < 2^31, capacity*3*S_k^2 < 2^31,
 * outputs aligned to 4 bytes; every argument is checked before the first device call.  Stream-ordered, no host
 * synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_preprocess_ms_batch(int G, int capacity, int K, const unsigned char *const *images_dev, const int32_t *H_host,
                             const int32_t *W_host, const int32_t *sizes_host, const float *mean_host, float *const *out_dev,
                             void *stream);
/* dsrg_preprocess_ms_batch with a target (h_k, w_k) per scale instead of S_k x S_k: the network inputs of a group of SAME-SIZED
 * test images at K relative scales in one launch (training/tools/test-ms-f.py:100-112 for G images; the images' sizes may
 * differ here too).  out_h_host / out_w_host: the K target heights / widths, out_dev a HOST array of K device pointers to
 * (capacity, 3, h_k, w_k) f32 NCHW tensors.  Slot g < G of output k is image g zoomed to h_k x w_k: coordinate y*(H-1)/(h-1) (0
 * when h == 1), likewise x; the two-tap blend l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11) in double, rounded once to f32;
 * BGR order; minus the mean (in f32).  Slots G..capacity-1 are written as zeros.  With h_k = w_k = S_k the results equal
 * dsrg_preprocess_ms_batch's bit for bit (one kernel serves both).  1 <= G <= 16, G <= capacity, 1 <= K <= 8, all sizes >= 1,
 * H_g*W_g*3 < 2^31, capacity*3*h_k*w_k < 2^31, outputs aligned to 4 bytes; every argument is checked before the first device
 * call.  Nothing is allocated.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_preprocess_rect_batch(int G, int capacity, int K, const unsigned char *const *images_dev, const int32_t *H_host,
                               const int32_t *W_host, const int32_t *out_h_host, const int32_t *out_w_host, const float *mean_host,
                               float *const *out_dev, void *stream);
/* dsrg_preprocess_rect_batch for mirrored test-time augmentation: every image fills two slots.  Slot 2g of output k is what
 * dsrg_preprocess_rect_batch writes for image g, bit for bit; slot 2g+1 is the same tensor with its last axis reversed (the
 * mirrored network input, not a second zoom of a mirrored image: each value is computed once and stored twice); slots
 * 2G..capacity-1 are written as zeros.  With h_k = w_k = S_k this serves the fixed sizes of test-ms.py as well.  1 <= G <= 8,
 * 2G <= capacity; the other arguments, limits and checks as there.  Nothing is allocated.  Stream-ordered, no host
 * synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_preprocess_rect_mirror_batch(int G, int capacity, int K, const unsigned char *const *images_dev, const int32_t *H_host,
                                      const int32_t *W_host, const int32_t *out_h_host, const int32_t *out_w_host,
                                      const float *mean_host, float *const *out_dev, void *stream);
/* The stage-1 training batch in one launch: Caffe's ImageData layer (training/experiment/seed_mc/train-s.prototxt:3-22: read,
 * cv::resize to S x S, mean 104/117/123) followed by AnnotationLayer (pylayers/pylayers/pylayers.py:346-387), for B images.
 * stage_dev: ONE device buffer of stage_bytes raw bytes (uploaded by the caller with one copy per batch); the HOST arrays
 * describe image b in it by byte offsets: image_off (H_b, W_b, 3) RGB uint8; cue_off the (3, ncues_b) int32 array '<id>_cues'
 * (classes, rows, columns; 4-byte aligned; ncues_b may be 0); label_off the nlabels_b int32 class ids '<id>_labels' (4-byte
 * aligned); mirror_host[b] != 0 reverses the last axis of image b's pixels and cue planes (pylayers.py:384-387).  Outputs:
 *   images_dev (B, 3, S, S) f32 NCHW: the 8-bit bilinear resize of the image (the integer arithmetic stated in DESIGN.md, a
 *              restatement of OpenCV's INTER_LINEAR for 8-bit images; an exact 2x shrink is NOT switched to area averaging),
 *              reordered to BGR, float(pixel) - mean_host[c]
 *   cues_dev   (B, C, Hm, Wm) f32: zeros, 1.0 at every (class, row, column) triplet; a triplet outside the planes writes nothing
 *   labels_dev (B, 1, 1, C) f32: 1.0 for class 0 and the listed ids, else 0
 * 1 <= B <= 32, S, C, Hm, Wm >= 1, H_b, W_b >= 1, every offset + extent inside stage_bytes < 2^31, H_b*W_b*3, B*3*S*S and
 * B*C*Hm*Wm < 2^31, ceil(B*S*S / 256) + B*C < 2^24 workgroups, outputs aligned to 4 bytes; every argument is checked before the first device call.  Nothing is allocated.
 * Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_train_s_input_batch(int B, const unsigned char *stage_dev, size_t stage_bytes, const int32_t *image_off_host,
                             const int32_t *H_host, const int32_t *W_host, const int32_t *cue_off_host, const int32_t *ncues_host,
                             const int32_t *label_off_host, const int32_t *nlabels_host, const int32_t *mirror_host, int S, int C,
                             int Hm, int Wm, const float *mean_host, float *images_dev, float *cues_dev, float *labels_dev,
                             void *stream);
/* The stage-1 training batch of a run fed by cue MAPS, in one launch: AnnotationLayerCOCO (pylayers/pylayers/pylayers.py:432-512,
 * the feeder of the 81-class runs) for B images.  stage_dev / stage_bytes as above; image_off the (H_b, W_b, 3) RGB uint8 image,
 * cue_off its (Hm, Wm) map of cue bytes (a class per pixel, ignore_label = no cue); mirror_host[b] != 0 reverses the last axis
 * of image b's pixels and cue planes.  A byte v is KEPT iff v != ignore_label and v < C.  Outputs, every element written:
 *   images_dev (B, 3, Sh, Sw) f32 NCHW: the image zoomed to Sh x Sw as dsrg_preprocess_rect_batch zooms (scipy.ndimage.zoom,
 *              order 1: coordinate y*(H-1)/(Sh-1), 0 when Sh == 1, likewise x; i0 = (int)src, i1 = i0 + (i0 < in-1); the two-tap
 *              blend l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11) in double, rounded once to f32), minus mean_host[c] in
 *              f32.  Output channel c reads source byte 2 - c with bgr = 1 (the order of every other entry of this library:
 *              the values are then dsrg_preprocess_rect_batch's bit for bit) and byte c with bgr = 0 (the layer's own order)
 *   cues_dev   (B, C, Hm, Wm) f32: 1.0 at (v, y, x) for every kept byte v at (y, x), 0.0 elsewhere
 *   labels_dev (B, 1, 1, C) f32: 1.0 for every class some kept byte names, else 0.0 (class 0 is NOT forced on; a map without a
 *              kept byte gives all zeros)
 * 1 <= B <= 32, Sh, Sw, Hm, Wm >= 1, 1 <= C <= 96 (above: DSRG_ERR_UNSUPPORTED), 0 <= ignore_label <= 255, bgr 0 or 1, H_b, W_b
 * >= 1, every offset + extent inside stage_bytes < 2^31, H_b*W_b*3, B*3*Sh*Sw and B*C*Hm*Wm < 2^31, outputs aligned to 4 bytes
 * (otherwise DSRG_ERR_INVALID — the 2^31 limits included: an INCONSISTENCY with the three sibling entries, which answer theirs
 * with DSRG_ERR_UNSUPPORTED; kept, since callers may test the code); every argument is checked before the first device call.
 * Nothing is allocated.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_train_s_cuemap_input_batch(int B, const unsigned char *stage_dev, size_t stage_bytes, const int32_t *image_off_host,
                                    const int32_t *H_host, const int32_t *W_host, const int32_t *cue_off_host,
                                    const int32_t *mirror_host, int Sh, int Sw, int C, int Hm, int Wm, const float *mean_host,
                                    int ignore_label, int bgr, float *images_dev, float *cues_dev, float *labels_dev, void *stream);
/* The stage-2 training batch in one launch: SimpleTransformer.preprocess of ImageSegDataLayer (pylayers/pylayers/layer.py:17-251,
 * the arithmetic of layer.py:169-236; train-f.prototxt:3-14) for B images.  stage_dev / stage_bytes as above; image_off the
 * (H_b, W_b, 3) RGB uint8 image, label_off its (H_b, W_b) uint8 label; top_host / left_host: the crop's offsets on the image
 * extended to at least the crop size at its bottom / right edges (drawn or centred by the host, >= 0); mirror_host[b] != 0
 * reverses both outputs along x.  Outputs:
 *   data_dev  (B, 3, ch, cw) f32: (float(pixel) - mean_host[c]) * scale in BGR order (two separately rounded f32 operations)
 *             where the crop lies on the image, 0.0 off it
 *   label_dev (B, 1, ch, cw) f32: the label byte as float where the crop lies on the image, ignore_label off it
 * 1 <= B <= 32, ch, cw >= 1, H_b, W_b >= 1, every offset + extent inside stage_bytes < 2^31, H_b*W_b*3 and B*3*ch*cw < 2^31,
 * outputs aligned to 4 bytes; every argument is checked before the first device call.  Nothing is allocated.  Stream-ordered,
 * no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_train_f_input_batch(int B, const unsigned char *stage_dev, size_t stage_bytes, const int32_t *image_off_host,
                             const int32_t *label_off_host, const int32_t *H_host, const int32_t *W_host, const int32_t *top_host,
                             const int32_t *left_host, const int32_t *mirror_host, int ch, int cw, const float *mean_host, float scale,
                             float ignore_label, float *data_dev, float *label_dev, void *stream);
/* dsrg_train_f_input_batch with a per-image rescaling in front of the crop (Caffe-DeepLab's `scale_factors`: cv::resize
 * INTER_LINEAR for the image, INTER_NEAREST for the label), in one launch; the rescaled image is never stored.  Arguments as
 * above, plus Hs_host / Ws_host: the size image b is rescaled to (the host's max(1, round_half_even(H_b * s)); the factor itself
 * does not cross this boundary).  top_host / left_host are offsets on the RESCALED image extended to at least the crop size.  The
 * pixel at (r, c) of the rescaled image is, per axis with n source and S output samples (n, S) = (H_b, Hs_b) and (W_b, Ws_b):
 *   image: the 8-bit bilinear resize stated in DESIGN.md ("The resize contract": scale = 1.0 / ((double)S / (double)n), fraction
 *          in float, 11-bit weights rounded half-even; x zeroes the fraction at clamped indices, y clamps its two rows; vertical
 *          pass >> 4, >> 16, + 2, >> 2); an exact 2x shrink is NOT switched to area averaging
 *   label: the byte at src = min((int)floor((double)d * scale), n - 1) on each axis, with the same double `scale`
 * and the outputs are those of dsrg_train_f_input_batch on that image: (float(pixel) - mean_host[c]) * scale in BGR order / the
 * label byte as float where the crop lies on the rescaled image, 0.0 / ignore_label off it, mirrored along x where
 * mirror_host[b] != 0.  With Hs_b = H_b and Ws_b = W_b the outputs equal dsrg_train_f_input_batch's bit for bit.
 * Limits as above, and Hs_b, Ws_b >= 1, Hs_b*Ws_b < 2^31; every argument is checked before the first device call.  Nothing is
 * allocated.  Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
int dsrg_train_f_input_scaled_batch(int B, const unsigned char *stage_dev, size_t stage_bytes, const int32_t *image_off_host,
                                    const int32_t *label_off_host, const int32_t *H_host, const int32_t *W_host,
                                    const int32_t *Hs_host, const int32_t *Ws_host, const int32_t *top_host, const int32_t *left_host,
                                    const int32_t *mirror_host, int ch, int cw, const float *mean_host, float scale,
                                    float ignore_label, float *data_dev, float *label_dev, void *stream);
/* Validation scoring of a batch in one launch: the confusion counters of the network's score maps against full-resolution label
 * maps, with nothing else written (no zoomed scores, no argmax map).
 *   scores_dev (>= B, C, h, w) f32 contiguous NCHW: the first B slices are scored (the scores of B inputs of extent Hz x Wz)
 *   labels_dev (B, 1, Hz, Wz) f32: what dsrg_train_f_input_batch writes as label_dev (the label byte as a float on the image,
 *              ignore_label off it)
 *   hist_dev   C*C + 1 unsigned 64-bit counters that are ADDED to, dsrg_confusion_matrix's layout: row = ground truth, column =
 *              prediction, the last one the overflow counter
 * A pixel (b, y, x) is kept iff label != ignore_label (rule_lt = 0, ConfusionMatrix.add) or label < (float)C (rule_lt = 1,
 * generateM).  Its prediction is the value dsrg_multiscale_unary(K = 1, C, slice b, h, w, Hz, Wz) writes to
 * argmax_dev[y * Wz + x], bit for bit: scale (in-1)/(out-1) in double (0 when out == 1), i0 = (int)src, i1 = i0 + (i0 < in-1),
 * the two-tap blend l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11) in double rounded once to f32, the first maximum over the
 * labels.  A kept label that is one of 0..C-1 exactly adds 1 to hist[label * C + pred]; any other kept label (negative, >= C,
 * non-integral) adds 1 to hist[C*C].  The prediction is always in [0, C): scores are assumed finite, non-finite ones may give
 * any label in range and never index outside the counters.
 * 1 <= B <= 32, 1 <= C <= 96 (above: DSRG_ERR_UNSUPPORTED), h, w, Hz, Wz >= 1, B*C*h*w < 2^31, B*Hz*Wz < 2^31; every argument is
 * checked before the first device call (NULL pointers and bad shapes: DSRG_ERR_INVALID).  Nothing is allocated.  Stream-ordered,
 * no host synchronisation, no handle.  The counters are integers added with atomics: the result does not depend on the order in
 * which workgroups finish, and repeated calls give identical counters. */
int dsrg_eval_confusion_batch(int B, int C, const float *scores_dev, int h, int w, const float *labels_dev, int Hz, int Wz,
                              float ignore_label, int rule_lt, unsigned long long *hist_dev, void *stream);
/* Scoring of finished label maps in one launch: the confusion counters of a group of G differently sized label maps — what
 * dsrg_crf_map / dsrg_crf_map_select and the argmax / labels outputs of the multi-scale and pseudo-label tails write — against
 * their ground truth, and optionally the maps narrowed to bytes (the PNG payload).
 *   labels_dev, gt_dev  HOST arrays of G device pointers, as dsrg_multiscale_unary_batch takes its per-image pointers:
 *              labels_dev[g] the (H_g, W_g) int32 label map of image g, gt_dev[g] its (H_g, W_g) uint8 ground truth
 *   H_host, W_host      host arrays of the G sizes (they may all differ)
 *   hist_dev   C*C + 1 unsigned 64-bit counters that are ADDED to, dsrg_confusion_matrix's layout: row = ground truth, column =
 *              prediction, the last one the overflow counter
 *   mask_dev   NULL, or a HOST array of G device pointers to (H_g, W_g) uint8: EVERY pixel, kept or not, gets the byte p where
 *              the label p is one of 0..255, and 255 otherwise
 * A pixel is kept iff gt != ignore_label (rule_lt = 0, ConfusionMatrix.add) or gt < C (rule_lt = 1, generateM).  A kept pixel
 * with gt and label both in 0..C-1 adds 1 to hist[gt * C + label]; any other kept pixel (a 255 written by ignore_below, a
 * negative label, a ground truth of 254 under rule_lt = 0) adds 1 to hist[C*C].  Without mask_dev the label of a pixel that is
 * not kept is not read.
 * 1 <= G <= 16, 1 <= C <= 96 (above: DSRG_ERR_UNSUPPORTED), H_g, W_g >= 1, sum of H_g*W_g < 2^31; the arrays, hist_dev and every
 * entry of the pointer arrays must not be NULL (DSRG_ERR_INVALID); every argument is checked before the first device call.
 * Nothing is allocated.  Stream-ordered, no host synchronisation, no handle.  The counters are integers added with atomics: the
 * result does not depend on the order in which lanes or workgroups add, and repeated calls give identical counters. */
int dsrg_score_labels_batch(int G, int C, const int32_t *const *labels_dev, const unsigned char *const *gt_dev,
                            const int32_t *H_host, const int32_t *W_host, int ignore_label, int rule_lt,
                            unsigned long long *hist_dev, unsigned char *const *mask_dev, void *stream);
/* Softmax loss at label resolution (stage 2 with loss_at = "label"; the reference takes the loss on the 41 x 41 map against labels
 * shrunk by 8, train-f.prototxt:721-744, and has no counterpart): the logits are zoomed to the label maps' size on the fly and the
 * loss is taken against every label pixel; loss, gradient and counters in two launches, nothing of size B*C*H*W written.
 *   logits_dev (>= B, C, h, w) f32 contiguous NCHW: the first B slices are used, the rest is not read
 *   labels_dev (B, 1, H, W) f32: what dsrg_train_f_input_batch writes as label_dev
 *   loss_dev   one f32, written;  grad_dev (B, C, h, w) f32, WRITTEN (not added to): d loss / d logits
 *   counters_dev  three unsigned 64-bit counters that are ADDED to: valid pixels, valid pixels whose first-maximum argmax over c
 *              of z equals the label (what dsrg_eval_confusion_batch counts on its diagonal), invalid pixels
 *   workspace_dev  dsrg_seg_loss_zoom_workspace(B, C, h, w, H, W) bytes, 8-byte aligned (0 is returned for shapes the launch
 *              refuses): one slot of loss and counts per workgroup; too small: DSRG_ERR_INVALID
 * z(b, c, y, x) is the score dsrg_eval_confusion_batch ranks at that pixel, bit for bit: scale (in-1)/(out-1) in double (0 when
 * out == 1), i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1, l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11)
 * in double rounded once to f32.  A pixel is IGNORED iff its label equals ignore_label; otherwise VALID iff the label is exactly
 * one of 0..C-1, and INVALID if not (>= C, negative, non-integral).  Ignored and invalid pixels add nothing to loss or gradient.
 * Per valid pixel: m = max_c z_c, e_c = expf(z_c - m), s = sum_c e_c in f32 with c ascending, l = logf(s) - (z_label - m),
 * p_c = e_c * (1 / s) with r = 1 / s one IEEE division per pixel (two tied planes of a 2-label map give p = 0.5 exactly).
 * With N the valid pixels of the whole call (Caffe's VALID normalisation):
 *   *loss_dev = (float)((sum of l in double) / max(N, 1))
 *   grad[b,c,i,j] = S / (float)max(N, 1), one IEEE division, S = the f32 sum over the valid pixels (y, x) of image b of
 *     (wy(y,i) * wx(x,j)) * (p_c - [c == label]),  wy(y,i) = ((i == y0) ? (float)l0h : 0) + ((i == y1) ? (float)l1h : 0), wx alike
 * N == 0 gives loss 0 and an all-zero gradient, never NaN.  S is a gather, summed in an order fixed by the shapes alone (the
 * products of a cell's pixels row by row: a row's from left to right, then the rows' sums from the top); the workgroups' losses are summed in slot order; there are no floating-point atomics on memory or LDS:
 * repeated calls give identical bits in loss_dev and grad_dev.
 * 1 <= B <= 32, 1 <= C <= 96 (above: DSRG_ERR_UNSUPPORTED), h, w, H, W >= 1 (enlarging, shrinking, identity), B*C*h*w < 2^31,
 * B*H*W < 2^31; every argument is checked before the first device call (NULL pointers and bad shapes: DSRG_ERR_INVALID).  Nothing
 * is allocated.  Stream-ordered, no host synchronisation, no handle. */
size_t dsrg_seg_loss_zoom_workspace(int B, int C, int h, int w, int H, int W);
int dsrg_seg_loss_zoom_batch(int B, int C, const float *logits_dev, int h, int w, const float *labels_dev, int H, int W,
                             float ignore_label, float *loss_dev, float *grad_dev, unsigned long long *counters_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream);
/* Multi-scale-input training with max fusion (DeepLab-v2's "MSC" recipe for ResNet-101: the shared-weight network runs on the crop
 * and on smaller copies of it, the smaller score maps are zoomed to the full one, the element-wise maximum is taken, and the fused
 * map and every scale's own map are judged by a softmax loss of weight 1 each; the reference retrains at one scale and has no
 * counterpart).  All three entry points are stream-ordered, allocate nothing, keep no handle, never synchronise the host, and check
 * every argument before the first device call (NULL pointers and bad shapes: DSRG_ERR_INVALID; C > 96: DSRG_ERR_UNSUPPORTED).
 * h, w (and maps_dev, grads_dev, out_dev: arrays of device pointers) are HOST arrays, read before the call returns.
 *
 * The zoom of both is the project's align-corners zoom (dsrg_eval_confusion_batch, dsrg_seg_loss_zoom_batch): scale =
 * (in-1)/(out-1) in double (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1,
 * l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11) in double rounded once to f32.
 *
 * dsrg_msc_pyramid_batch, one launch: images_dev (B, 3, H, W) f32 NCHW -> n = 1..3 zoomed copies out_dev[s] of h[s] x w[s], each
 * WRITTEN CHANNELS-LAST (memory order B, h, w, 3: what a (B, 3, h, w) tensor of torch.channels_last holds).  1 <= B <= 32,
 * B*3*H*W < 2^31, the copies together < 2^31 values; a copy may be larger than the input.
 *
 * dsrg_msc_loss_batch, three launches: S = 2..4 score maps maps_dev[s] (B, C, h[s], w[s]) f32 NCHW contiguous, map 0 the full scale
 * (any sizes: a map may be as large as map 0 or larger), labels_dev (B, 1, H, W) f32 as dsrg_train_f_input_batch writes them.
 *   labels of map s: the nearest sample of the label map at the align-corners position, in integers:
 *       y = (2*i*(H-1) + (h[s]-1)) / (2*(h[s]-1)), 0 when h[s] == 1; columns alike (at H-1 = 8 (h-1): label[::8, ::8]).
 *       Validity as dsrg_seg_loss_zoom_batch: ignored iff == ignore_label, else valid iff exactly one of 0..C-1, else invalid.
 *   fused map: u_0 = z_0, u_s = z_s zoomed to h[0] x w[0]; f_c = max_s u_s,c; the winner k_c(i,j) = the LOWEST s attaining it.
 *   each of the S + 1 heads per valid pixel as dsrg_seg_loss_zoom_batch: m = first maximum over c, e_c = expf(z_c - m), s = sum
 *       of e_c in f32 with c ascending, r = 1/s, term = logf(s) - (z_label - m), d_c = e_c*r - [c == label]; d = 0 where the pixel is
 *       not valid.  N_s = valid pixels of map s; the fused head shares map 0's labels and N_0.
 *   losses_dev[S+1] f32, written: fused, map 0, map 1, ...: (float)((double sum of the head's terms) / max(N_head, 1))
 *   grads_dev[s] (B, C, h[s], w[s]) f32, WRITTEN: the gradient of the SUM of the S + 1 losses with respect to map s:
 *       grad_0 = (d_0 + [k == 0] * d_f) / (float)max(N_0, 1)
 *       grad_s = d_s / (float)max(N_s, 1) + G_s / (float)max(N_0, 1)  for s > 0, with
 *       G_s,c(a,b) = the f32 sum over the map-0 pixels (y, x) whose taps touch cell (a,b) of (wy*wx) * [k_c(y,x) == s] * d_f,c(y,x),
 *       wy = ((a == y0) ? (float)l0h : 0) + ((a == y1) ? (float)l1h : 0), wx alike — a GATHER per cell, rows from the top, a row's
 *       products from the left, the row's sum added to the cell's: an order fixed by the shapes alone.
 *   counters_dev: three unsigned 64-bit counters ADDED to, for the fused head: valid pixels, valid pixels whose first-maximum
 *       argmax of f equals the label, invalid labels of map 0's sampling.
 *   workspace_dev: dsrg_msc_loss_workspace(...) bytes (0 for what the launch refuses), 8-byte aligned: d_f and the winner bytes
 *       (5 bytes per element of map 0) plus a 32-byte slot per 64 pixels of the maps; too small: DSRG_ERR_INVALID.  After the call
 *       its first S unsigned 64-bit words hold N_0 .. N_{S-1}.
 * No floating-point atomics on memory or LDS: repeated calls give identical bits.  Nothing valid: losses 0, zero gradients.
 * 1 <= B <= 32, 1 <= C <= 96, every size >= 1, B*C*sum(h*w) < 2^31, B*H*W < 2^31. */
int dsrg_msc_pyramid_batch(int B, const float *images_dev, int H, int W, int n, const int *h, const int *w, float *const *out_dev,
                           void *stream);
size_t dsrg_msc_loss_workspace(int S, int B, int C, const int *h, const int *w, int H, int W);
int dsrg_msc_loss_batch(int S, int B, int C, const float *const *maps_dev, const int *h, const int *w, const float *labels_dev, int H,
                        int W, float ignore_label, float *losses_dev, float *const *grads_dev, unsigned long long *counters_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);
/* The stem of the DeepLab-v2 ResNet-101 at test time in one launch (backbone plumbing; the reference's networks are Caffe
 * prototxts): conv 7x7 / stride 2 / zero pad 3, 3 -> 64, with a frozen BatchNorm folded in -> ReLU -> max pool 3x3 / stride 2 /
 * pad 1, ceil mode.  The convolution map never reaches memory.
 *   dsrg_pack_resnet_stem_f32: w_dev (64, 3, 7, 7) f32 contiguous and scale_dev (64) f32 -> packed_dev,
 *     dsrg_resnet_stem_packed_bytes() bytes, 16-byte aligned: (64, 192) bf16, packed[o][(ky * 3 + c) * 8 + kx] =
 *     bf16(w[o][c][ky][kx] * scale[o]) — one f32 product, rounded once to nearest even — and 0 where kx = 7 or ky * 3 + c >= 21.
 *   dsrg_resnet_stem_bf16: x_dev (B, 3, H, W) f32 contiguous NCHW, each value rounded to bf16 (nearest even) as it is read;
 *     shift_dev (64) f32; y_dev (B, PH, PW, 64) bf16 (the memory of a channels_last (B, 64, PH, PW) tensor):
 *       conv[b,o,i,j] = max(0, shift[o] + sum_{c,ky,kx} packed(o,c,ky,kx) * bf16(x[b, c, 2i - 3 + ky, 2j - 3 + kx]))   (zero outside x)
 *     for i < OHc = (H - 1) / 2 + 1, j < OWc = (W - 1) / 2 + 1, products summed in f32, and
 *       y[b,p,q,o] = bf16(max of conv[b,o,i,j] over 2p - 1 <= i <= 2p + 1, 2q - 1 <= j <= 2q + 1 ON the OHc x OWc map)
 *     for p < PH = OHc / 2 + 1 less one if 2 (PH - 1) >= OHc + 1 (the 3x3 / 2 / pad 1 ceil-mode extent), PW likewise.  Window
 *     positions off the map do not exist (they are not convolutions over zero padding).  shift_dev, packed_dev, y_dev 16-byte aligned.
 * Both check every argument before the first device call (NULL pointers, B, H, W < 1: DSRG_ERR_INVALID).  Nothing is allocated.
 * Stream-ordered, no host synchronisation, no handle; bit-reproducible (no atomics). */
size_t dsrg_resnet_stem_packed_bytes(void);
int dsrg_pack_resnet_stem_f32(const float *w_dev, const float *scale_dev, void *packed_dev, void *stream);
int dsrg_resnet_stem_bf16(const float *x_dev, const void *packed_dev, const float *shift_dev, void *y_dev, int B, int H, int W,
                          void *stream);

/* Backbone plumbing (no reference counterpart; Caffe's im2col lives in the external framework): NHWC im2col
 * of a 3x3, stride-1, "same"-padded, dilated convolution for 2-byte elements (bf16/fp16), C % 8 == 0:
 *   out[(b,y,x)][tap][c] = in[b][y+(tap/3-1)*dil][x+(tap%3-1)*dil][c], zero outside the map. */
int dsrg_im2col3x3_nhwc16(const void *in_dev, void *out_dev, int B, int H, int W, int C, int dilation, void *stream);
/* Adjoint of dsrg_im2col3x3_nhwc16 for bf16: out[b,y,x,:] = sum over the 9 taps of cols[(b, y-dy*dil, x-dx*dil), tap, :]
 * (cols: (B*H*W, 9*C) row-major, f32 accumulation).  With cols = g @ W^T this is the data gradient of the convolution. */
int dsrg_col2im3x3_nhwc_bf16(const void *cols_dev, void *out_dev, int B, int H, int W, int C, int dilation, void *stream);
/* ReLU backward fused with the bias-gradient reduction of the convolution in front of it: g, y (the ReLU output) and
 * gm are (rows, C) bf16 row-major (NHWC activations), C % 8 == 0; gm = scale * g where y > 0 else 0; bias_grad[c] =
 * sum_r gm[r,c] (f32, summed in a fixed order).  scale = 1 for a plain ReLU; with y = dropout(relu(.)) and
 * scale = 1/(1-p) the same pass is the backward of ReLU + Dropout (y > 0 is both masks at once).  y_dev = gm_dev = NULL:
 * no ReLU, only the column sums of g (any C % 8 == 0 up to 2048; dsrg_bias_grad_bf16 covers the other widths).
 * partials: device scratch of partial_blocks * C floats. */
int dsrg_relu_bwd_bias_bf16(const void *g_dev, const void *y_dev, void *gm_dev, float *bias_grad_dev, float *partials_dev,
                            int partial_blocks, long rows, int C, float scale, void *stream);
/* Column sums of a (rows, C) bf16 matrix in f32, any C <= 256 (bias gradient of a convolution without a ReLU behind it,
 * e.g. the 21-channel fc8 outputs).  partials: device scratch of partial_blocks * C floats. */
int dsrg_bias_grad_bf16(const void *g_dev, float *bias_grad_dev, float *partials_dev, int partial_blocks, long rows, int C,
                        void *stream);
/* Layer-level prototype (round 6) of a FLOAT32 convolution on the bf16 MFMA — the arithmetic of the reference's Caffe
 * convolutions (train-s.prototxt:41-744) at six bf16 products per multiply-add: x = x0 + x1 + x2, w = w0 + w1 + w2 (each term the
 * bf16 rounding of what the terms before leave), products x0 w0, x0 w1, x1 w0, x0 w2, x2 w0, x1 w1 on the fp32 accumulators.
 *   x3_dev (B,H,W,3*cin) bf16: channel plane * cin + c;  w_dev (cout, 6*cin/64, k*k, 64) bf16: the dsrg_conv_igemm_bf16 packing of
 *   the six-block virtual kernel [w0 | w1 | w0 | w2 | w0 | w1];  y_dev (B,H,W,cout) float32.  Forward only, one group. */
int dsrg_conv_igemm_split_f32(const void *x3_dev, const void *w_dev, const float *bias_dev, float *y_dev, int dilation, int B, int H,
                              int W, int cin, int cout, int ksize, int relu, void *stream);
/* The tail of a ResNet bottleneck (the train-f stage on the DeepLab-v2 ResNet-101 of BASELINE.json configs[4]; the reference
 * trains VGG16 only, train-f.prototxt:15-720 — backbone plumbing): y = relu(a + b) over n bf16 elements (fp32 sum, one
 * rounding), n % 8 == 0; and its backward gm = (y > 0) ? g (+ g2) : 0 — g2_dev (may be NULL): a second gradient of y to be
 * added first (the sum autograd would otherwise take in a pass of its own). */
int dsrg_add_relu_bf16(const void *a_dev, const void *b_dev, void *y_dev, size_t n, void *stream);
int dsrg_relu_mask_bf16(const void *g_dev, const void *g2_dev, const void *y_dev, void *gm_dev, size_t n, void *stream);
/* 3x3 / stride 1 / pad 1 average pooling over padded windows (Caffe AVE pooling, pool5a of train-s.prototxt), NHWC bf16,
 * C % 8 == 0.  The stencil is symmetric: the backward pass is the same call on the output gradient. */
int dsrg_avgpool3x3_s1_bf16(const void *in_dev, void *out_dev, int B, int H, int W, int C, void *stream);
/* Direct 3x3 / stride 1 / pad 1 convolution for the narrow layers at the large resolutions: cin, cout in {64, 128}
 * (conv1_2 at 321x321, conv2_1 / conv2_2 at 161x161 of train-s.prototxt:65-160) and 3 -> 64 (conv1_1, :44-64), NHWC bf16 in and out, fp32
 * accumulation, optional bias (cout f32) and ReLU in the epilogue:
 *   y[b,y,x,o] = relu?( bias[o] + sum_{dy,dx,c} w[o][dy+1][dx+1][c] * x[b,y+dy,x+dx,c] )
 * w_dev: (cout, 3, 3, cin) bf16 = the memory of a channels_last (out, in, 3, 3) tensor.  With the kernel flipped and its
 * channel axes swapped the same call is the data gradient of that convolution.  Other channel counts: DSRG_ERR_INVALID.
 * Size limit (this call and dsrg_conv3x3_direct_dgrad_bf16): a launch with 64 / 128 channels whose B * H * W * max(cin, cout) * 2
 * bytes reach 2^31 is refused with DSRG_ERR_UNSUPPORTED, forward and masked alike; 3 -> 64 has no such limit. */
int dsrg_conv3x3_direct_bf16(const void *x_dev, const void *w_dev, const float *bias_dev, void *y_dev, int B, int H, int W,
                             int cin, int cout, int relu, void *stream);
/* The data-gradient form with the ReLU backward of the layer below in its store (cin, cout in {64, 128}): gx = conv(g, w) where
 * mask_dev (B,H,W,cout) bf16 — that layer's output — is positive, else 0; bias_grad_dev (cout f32) = sum over pixels of gx
 * (fixed summation order).  workspace_dev: dsrg_conv3x3_direct_dgrad_workspace(cout) bytes.  The size limit above applies. */
size_t dsrg_conv3x3_direct_dgrad_workspace(int cout);
int dsrg_conv3x3_direct_dgrad_bf16(const void *g_dev, const void *w_dev, const void *mask_dev, void *gx_dev, float *bias_grad_dev,
                                   void *workspace_dev, size_t workspace_bytes, int B, int H, int W, int cin, int cout, void *stream);
/* Weight gradient of the same convolution for (cin, cout) in {(3, 64), (64, 64), (64, 128), (128, 128)}:
 *   gw[o][dy+1][dx+1][c] = sum_{b,y,x} g[b,y,x,o] * x[b,y+dy,x+dx,c]      (zero padding)
 * x_dev (B,H,W,cin) and g_dev (B,H,W,cout) NHWC bf16; gw_dev (cout, 3, 3, cin) bf16 = the memory of a channels_last
 * (out, in, 3, 3) tensor; fp32 accumulation, summed in a fixed order (deterministic).  workspace_dev: device scratch of
 * dsrg_conv3x3_wgrad_workspace(B, H, W, cin, cout) bytes (0 = unsupported channel counts). */
size_t dsrg_conv3x3_wgrad_workspace(int B, int H, int W, int cin, int cout);
int dsrg_conv3x3_wgrad_bf16(const void *x_dev, const void *g_dev, void *gw_dev, void *workspace_dev, size_t workspace_bytes,
                            int B, int H, int W, int cin, int cout, void *stream);
/* The same with the gradient in float32 (the master parameters' dtype: no rounding, no cast pass). */
int dsrg_conv3x3_wgrad_f32(const void *x_dev, const void *g_dev, float *gw_dev, void *workspace_dev, size_t workspace_bytes, int B,
                           int H, int W, int cin, int cout, void *stream);
/* Both bf16 kernels dsrg_conv3x3_direct_bf16 reads, from the float32 master (cout, 3, 3, cin) in one pass (cin, cout in {64, 128}):
 * fwd_dev (cout, 3, 3, cin) — the parameter cast — and dgrad_dev (cin, 3, 3, cout) — flipped, channel axes swapped: the kernel of
 * the data gradient.  Either may be NULL. */
int dsrg_pack_conv_weight_direct_f32(const float *w_dev, void *fwd_dev, void *dgrad_dev, int cout, int cin, void *stream);
/* Implicit-GEMM convolution for the wide layers (conv3_x, conv4_x, conv5_x, fc6_k, fc7_k of train-s.prototxt:161-736): 3x3
 * with any dilation ('same' zero padding) or 1x1, stride 1, cin % 64 == 0, cout % 256 == 0, NHWC bf16 in and out, fp32
 * accumulation, optional bias (cout f32) and ReLU in the epilogue (the launch also takes cout = 64 — half-empty channel tiles, for
 * bandwidth-bound 1x1 layers; dsrg_conv_igemm_supported names the shapes it is the recommended route for); no im2col matrix is formed:
 *   y[b,y,x,o] = relu?( bias[o] + sum_{dy,dx,c} w[o][dy+1][dx+1][c] * x[b,y+dy*dil,x+dx*dil,c] )
 * Up to four independent problems of one geometry (the four ASPP branches) share a launch: x_dev, w_dev, bias_dev (may be
 * NULL, entries may be NULL), y_dev and dilation are HOST arrays of ngroups entries.  w_dev[g]: the kernel packed as
 * (cout, cin / 64, ksize * ksize, 64) bf16 — w_packed[o][cc][tap][c] = w[o][cc * 64 + c][tap / 3][tap % 3].  With the kernel
 * flipped and its channel axes swapped the same call is the data gradient.  dropout_p > 0: the Dropout layer behind the
 * ReLU (train-s.prototxt: drop6_k, drop7_k) in the same epilogue — y = relu(..) * keep / (1 - p), keep a pure function of
 * (dropout_seed, group, element position) from a counter-based generator, p realised in steps of 1/256; the backward pass
 * reads both masks off the sign of y.  dsrg_conv_igemm_supported: 1 if the channel counts / kernel size are served, else 0
 * (the call then returns DSRG_ERR_UNSUPPORTED).
 * workspace_dev (may be NULL): dsrg_conv_igemm_workspace() bytes of device scratch owned by the caller and used by ONE stream
 * at a time.  With it, a launch whose tiles do not fill whole rounds of the chip deals its K-steps out evenly instead
 * ("stream-K": one workgroup per CU, partial tiles handed over through the scratch, summed in a fixed order — results are
 * deterministic, equal to the whole-tile launch up to the fp32 summation order of a cut tile).
 * dsrg_conv_igemm_workspace_status (tests): 0, or 1 if a workgroup of the last launch on that scratch gave up waiting. */
int dsrg_conv_igemm_supported(int cin, int cout, int ksize);
int dsrg_conv_igemm_bf16(const void *const *x_dev, const void *const *w_dev, const float *const *bias_dev, void *const *y_dev,
                         const int *dilation, int ngroups, int B, int H, int W, int cin, int cout, int ksize, int relu,
                         float dropout_p, unsigned long long dropout_seed, void *workspace_dev, size_t workspace_bytes,
                         void *stream);
size_t dsrg_conv_igemm_workspace(void);
/* The same launch as the data gradient of a convolution whose INPUT was the output y_below of a ReLU (optionally followed by
 * Dropout) layer: gx = conv(g, w_dgrad) * mask_scale where mask = y_below > 0, else 0 — the ReLU / Dropout backward folded
 * into the store — and bias_grad[g][c] = sum over pixels of gx (the bias gradient of the layer below; fp32, fixed summation
 * order).  g: (B, H, W, cin) gradient of this layer's output; w: the flipped + transposed packing of dsrg_pack_conv_weight_f32
 * (cout = the layer's INPUT channels); mask, gx: (B, H, W, cout) bf16; bias_grad_dev: NULL or ngroups pointers to cout floats;
 * workspace_dev: dsrg_conv_igemm_dgrad_workspace(...) bytes when bias_grad_dev is given.  Replaces the separate
 * relu-backward + bias-sum pass over the gradient (mirror: torch.autograd of Conv -> ReLU -> Dropout in one step). */
size_t dsrg_conv_igemm_dgrad_workspace(int ngroups, int B, int H, int W, int cout);
int dsrg_conv_igemm_dgrad_bf16(const void *const *g_dev, const void *const *w_dev, const void *const *mask_dev, void *const *gx_dev,
                               float *const *bias_grad_dev, const int *dilation, int ngroups, int B, int H, int W, int cin,
                               int cout, int ksize, float mask_scale, void *workspace_dev, size_t workspace_bytes, void *stream);
/* One convolution of the same family with a RESIDUAL in its store (a ResNet bottleneck's shortcut; the reference's stage-2 networks
 * are DeepLab-v2 VGG16 / ResNet-101 — training/experiment/anti-noise/config/deeplabv2_weak.prototxt — where Caffe runs Eltwise SUM +
 * ReLU layers of their own):  y = post( bf16(conv(x, w) + bias) + res ),  post = ReLU (relu != 0) and / or zero where mask <= 0
 * (mask_dev may be NULL).  res, mask, y: (B, H, W, cout) bf16.  Bit for bit what dsrg_conv_igemm_bf16 followed by dsrg_add_relu_bf16
 * (forward: res = the shortcut) or by a bf16 add and dsrg_relu_mask_bf16 (data gradient of the block's first convolution: res = the
 * gradient that reaches the block input along the shortcut, mask = the block input, itself a ReLU output) gives, in one launch. */
int dsrg_conv_igemm_residual_bf16(const void *x_dev, const void *w_dev, const float *bias_dev, const void *res_dev, const void *mask_dev,
                                  void *y_dev, int dilation, int B, int H, int W, int cin, int cout, int ksize, int relu, void *stream);
/* The DeepLab-v2 ASPP head — J = branches x 9 (branch, tap) pairs of dilated 3x3 classifiers with `outputs` (21) channels each, all
 * reading ONE feature map and summed (deeplabv2 prototxt: fc1_voc12_c0..c3 + Eltwise SUM) — as one 1x1 convolution plus a shifted
 * gather: y = dsrg_conv_igemm_bf16(x, the (J outputs, rounded up to `channels`) x cin matrix of all kernels' taps, 1x1) and
 *   out[b,y,x,o] = bias[o] + sum_j y[b, y + dy_j, x + dx_j, j outputs + o]        (zero outside the map; j ascending; fp32)
 * (dsrg_aspp_shift_sum_f32; y (B,H,W,channels) bf16, out (B,H,W,outputs) f32, bias_dev (outputs) or NULL = the branches' biases
 * summed).  Backward: gp[b,y,x,j outputs + o] = bf16(g[b, y - dy_j, x - dx_j, o]) (dsrg_aspp_shift_gather_bf16; channels past
 * J outputs zero) is the gradient of y; the 1x1 layer's data / weight gradients follow.  offsets: HOST array of npairs (dy, dx)
 * pairs, npairs <= 36.  No output channel is padded to a 128-wide tile and the feature map is read once per pass. */
int dsrg_aspp_shift_sum_f32(const void *y_dev, const float *bias_dev, float *out_dev, const int *offsets, int npairs, int outputs,
                            int channels, int B, int H, int W, void *stream);
int dsrg_aspp_shift_gather_bf16(const float *g_dev, void *gp_dev, const int *offsets, int npairs, int outputs, int channels, int B, int H,
                                int W, void *stream);
/* Deferred bias-gradient reductions.  The launches that hand back a bias gradient (dsrg_conv_igemm_dgrad_bf16 / dsrg_conv_igemm_backward_bf16
 * with bias_grad_dev, dsrg_conv3x3_direct_dgrad_bf16, dsrg_heads_backward_relu_bf16, dsrg_relu_bwd_bias_bf16, dsrg_bias_grad_bf16,
 * dsrg_maxpool3x3_bwd_relu_bf16) end with a pass of 5-7 us that sums per-tile / per-block partial rows (fifteen such passes per
 * train-s step, 96 us) and nothing reads a bias gradient before the update.  dsrg_defer_reductions(1): from now on these passes
 * are RECORDED instead of launched (up to 48; beyond that they run as before — a launch's groups all or none);
 * dsrg_flush_reductions(stream) runs everything
 * recorded in ONE launch on `stream` — the same arithmetic in the same order, the gradients' bits do not change — and
 * dsrg_defer_reductions(0) stops recording.  Process-wide.  The caller's duties while recording: the partial-row scratch it passed
 * to each launch (workspace_dev / partial_dev) stays alive, and is not shared between launches, and the bias gradients' memory
 * stays allocated (the flush writes it), until the flush has been enqueued on the stream the launches ran on; nothing reads the
 * bias gradients before it. */
int dsrg_defer_reductions(int on);
int dsrg_flush_reductions(void *stream);
int dsrg_conv_igemm_workspace_status(const void *workspace_dev, void *stream, int *status_host);
/* The two packed forms dsrg_conv_igemm_bf16 reads, from the float32 master kernel in ONE pass (cast included): w_dev
 * (cout, ksize*ksize, cin) f32 = the memory of a channels_last (cout, cin, ksize, ksize) parameter; fwd_dev (may be NULL):
 * (cout, cin / 64, taps, 64) bf16 for the forward; dgrad_dev (may be NULL): (cin, cout / 64, taps, 64) bf16 for the data
 * gradient (kernel flipped, channel axes swapped).  64 | cout, 64 | cin. */
int dsrg_pack_conv_weight_f32(const float *w_dev, void *fwd_dev, void *dgrad_dev, int cout, int cin, int ksize, void *stream);
/* The same with a constant per-output-channel factor folded in: w[o] * scale_dev[o] is what is packed (scale_dev (cout) f32, may be
 * NULL = dsrg_pack_conv_weight_f32) — a frozen BatchNorm's scale behind the convolution (DeepLab-v2 ResNet-101, use_global_stats). */
int dsrg_pack_conv_weight_scaled_f32(const float *w_dev, const float *scale_dev, void *fwd_dev, void *dgrad_dev, int cout, int cin,
                                     int ksize, void *stream);
/* Caffe's SGDSolver update (solver-s.prototxt:5-14: momentum 0.9, weight_decay 5e-4, per-blob lr_mult / decay_mult of
 * train-s.prototxt) of n float32 parameters, sixteen per launch, in the form  B <- momentum B + (g + wd W);  W <- W - lr B
 * (B = Caffe's history / lr), WITH the packed bf16 kernels of the convolution routes written from the new values in the same
 * pass (the packs of dsrg_pack_conv_weight_f32 / dsrg_pack_conv_weight_direct_f32 — the next forward then reads no float32
 * weight).  Host arrays of n entries each: param_dev / grad_dev / momentum_dev device pointers (4-byte aligned; parameter and momentum of a packed kernel 16, same element
 * order; grad_dev[i] = NULL: tensor i is only packed); fwd_dev[i] / dgrad_dev[i] packed outputs or NULL (the arrays themselves
 * may be NULL: nothing packed); shape[4 i ..] = {cout, cin, taps (1 | 9), plain (1: the direct kernels' layouts)} of a packed
 * tensor, whose memory is (cout, taps, cin), 64 | cout, 64 | cin; numel[i]; lr[i] = base_lr * lr_mult, weight_decay[i] =
 * weight_decay * decay_mult.  Element-wise, one thread owns an element: deterministic. */
int dsrg_sgd_pack_f32(int n, float *const *param_dev, const float *const *grad_dev, float *const *momentum_dev, void *const *fwd_dev,
                      void *const *dgrad_dev, const int *shape, const long long *numel, const float *lr, const float *weight_decay,
                      float momentum, void *stream);
/* Weight gradient of the same convolutions, again without an im2col matrix (cin % 64 == 0, cout % 64 == 0, ksize 1 or 3; tiles of 256
 * outputs x 256 inputs of one tap — full, hence the recommended route, where cin % 256 == 0 (or cin = 128 with a 3x3 kernel) and
 * cout % 256 == 0; narrower tensors run partly empty tiles, which is fine where the layer is bandwidth-bound):
 *   gw[o][tap][c] = sum_{b,y,x} g[b,y,x,o] * x[b,y+dy*dil,x+dx*dil,c]      (zero padding; tap = 3 (dy+1) + dx+1)
 * x_dev[g] (B,H,W,cin) and g_dev[g] (B,H,W,cout) NHWC bf16; gw_dev[g] (cout, ksize*ksize, cin) = the memory of a channels_last
 * (cout, cin, ksize, ksize) tensor, float32 (out_bf16 = 0: the master weights' gradient, no cast behind it) or bf16; fp32
 * accumulation; the pixel range is split over workgroups whose partial tiles are summed in a fixed order (deterministic).
 * x_dev, g_dev, gw_dev, dilation: HOST arrays of ngroups (1..4) entries (the four ASPP branches in one launch).
 * A launch of 3x3 kernels of which one has dilation >= 3 splits the pixels per (group, tap), in proportion to the pixels the tap
 * reaches (a tap that reaches none runs no workgroup, its rows of the gradient are exact zeros); every other launch splits all
 * its tiles alike.
 * workspace_dev: dsrg_conv_igemm_wgrad_workspace(ngroups, B, H, W, cin, cout, ksize) bytes of device scratch (0 = unsupported;
 * the size holds for any dilations).  A launch with per-tap splits writes a small work list into the end of those bytes itself,
 * in the same stream, every time: the buffer's contents between calls do not matter. */
size_t dsrg_conv_igemm_wgrad_workspace(int ngroups, int B, int H, int W, int cin, int cout, int ksize);
/* Read-only query (host only, no launch): the number of pixel splits dsrg_conv_igemm_wgrad_bf16 runs for each (group, tap) of this
 * launch: splits_out[ksize*ksize * g + tap], 0 for a tap that reaches no pixel. */
int dsrg_conv_igemm_wgrad_splits(int ngroups, int B, int H, int W, int cin, int cout, int ksize, const int *dilation, int *splits_out);
int dsrg_conv_igemm_wgrad_bf16(const void *const *x_dev, const void *const *g_dev, void *const *gw_dev, const int *dilation,
                               int ngroups, void *workspace_dev, size_t workspace_bytes, int B, int H, int W, int cin, int cout,
                               int ksize, int out_bf16, void *stream);
/* The whole backward of ONE 3x3 convolution of the forward geometry cin -> cout as one launch: the data gradient gx (B,H,W,cin) of g
 * (B,H,W,cout) with the data-gradient packing w_dgrad_dev (dsrg_pack_conv_weight_f32) — with mask_dev (the layer's INPUT = the ReLU
 * output of the layer below, (B,H,W,cin) bf16) and bias_grad_dev given also that layer's ReLU (+ Dropout: mask_scale) backward and
 * bias gradient, as dsrg_conv_igemm_dgrad_bf16 — and the weight gradient gw (cout, cin, k, k; float32, channels_last) from x_dev
 * (B,H,W,cin) and g.  The data gradient's tiles and the weight gradient's workgroups share a grid, so the CUs a 212-tile data
 * gradient leaves idle take weight-gradient work; where that form does not apply (dilation >= 3, a 128-channel x) the two launches
 * run one after the other.  The data gradient equals dsrg_conv_igemm_dgrad_bf16 / dsrg_conv_igemm_bf16 bit for bit; the weight gradient
 * equals dsrg_conv_igemm_wgrad_bf16 up to fp32 reassociation (its pixel split is chosen for the merged grid); both deterministic.
 * Workspaces: dsrg_conv_igemm_dgrad_workspace(1, B, H, W, cin) bytes (only with bias_grad_dev) and
 * dsrg_conv_igemm_wgrad_workspace(1, B, H, W, cin, cout, ksize) bytes. */
int dsrg_conv_igemm_backward_bf16(const void *g_dev, const void *w_dgrad_dev, const void *x_dev, const void *mask_dev, void *gx_dev,
                                  float *gw_dev, int dilation, float *bias_grad_dev, float mask_scale, void *colsum_workspace_dev,
                                  size_t colsum_workspace_bytes, void *wgrad_workspace_dev, size_t wgrad_workspace_bytes, int B, int H,
                                  int W, int cin, int cout, int ksize, void *stream);
/* The same whole backward (3x3 with dilation < 3, or 1x1: merged grid; else two launches) for a convolution inside a residual block
 * with a folded constant scale: res_dev (may be NULL; (B,H,W,cin) bf16) is added to the bf16-rounded data gradient before the mask, as
 * dsrg_conv_igemm_residual_bf16; gw_scale_dev (may be NULL; (cout) f32): gw[o] = scale[o] * (the gradient of the scaled kernel the
 * forward ran with).  No bias gradient.  mask_dev may be NULL. */
int dsrg_conv_igemm_backward_residual_bf16(const void *g_dev, const void *w_dgrad_dev, const void *x_dev, const void *mask_dev,
                                           const void *res_dev, void *gx_dev, float *gw_dev, const float *gw_scale_dev, int dilation,
                                           void *wgrad_workspace_dev, size_t wgrad_workspace_bytes, int B, int H, int W, int cin, int cout,
                                           int ksize, void *stream);
/* dsrg_conv_igemm_backward_bf16 for 1 - 4 convolutions of one geometry (the four ASPP branches; 3x3 with any dilations, or 1x1): host
 * arrays of ngroups device pointers as dsrg_conv_igemm_dgrad_bf16 / dsrg_conv_igemm_wgrad_bf16 take them.  mask_dev / bias_grad_dev may
 * be NULL (both or neither: the layer's inputs are not ReLU outputs with a single consumer).  The grouped data gradient (XCD-interleaved,
 * class-ordered or row tiles for dilated kernels) and the grouped weight gradient (its per-tap work list for dilated kernels) share one
 * grid where the launch planner prices that below the two launches, else they run one after the other: the same bits either way.
 * Data and bias gradients equal dsrg_conv_igemm_dgrad_bf16 / dsrg_conv_igemm_bf16 bit for bit; a weight gradient that runs its work
 * list equals dsrg_conv_igemm_wgrad_bf16 bit for bit, one on a uniform split does wherever the split is that launch's (it is chosen
 * for the merged grid; force_ksplit > 0, for tests, sets it as far as the workspace holds it) and else up to fp32 reassociation.  force_order 1 / 2: a merged grid takes the data / weight gradient's
 * blocks first (0: the planner's order; for tests — the results do not depend on it).  Workspaces: dsrg_conv_igemm_dgrad_workspace(ngroups, B, H, W, cin)
 * bytes (only with bias_grad_dev) and dsrg_conv_igemm_wgrad_workspace(ngroups, B, H, W, cin, cout, ksize) bytes. */
int dsrg_conv_igemm_backward_groups_bf16(const void *const *g_dev, const void *const *w_dgrad_dev, const void *const *x_dev,
                                         const void *const *mask_dev, void *const *gx_dev, void *const *gw_dev, const int *dilation,
                                         int ngroups, float *const *bias_grad_dev, float mask_scale, void *colsum_workspace_dev,
                                         size_t colsum_workspace_bytes, void *wgrad_workspace_dev, size_t wgrad_workspace_bytes, int B,
                                         int H, int W, int cin, int cout, int ksize, int force_ksplit, int force_order, void *stream);
/* Read-only query (host only, no launch) of what that call does under the current variant: plan_out[0] 1 = one merged grid, 0 = two
 * launches; [1] 1 = the weight gradient's workgroups take the first block ids; [2] the weight gradient's uniform pixel split (0: it
 * runs its work list); [3], [4] blocks of the data- / weight-gradient half.  us_out[0], [1]: the dispatch model's price of the choice
 * and of the two launches, microseconds. */
int dsrg_conv_igemm_backward_groups_plan(int ngroups, int B, int H, int W, int cin, int cout, int ksize, const int *dilation, int with_mask,
                                         int force_ksplit, int force_order, int *plan_out, double *us_out);
/* The four fc8-SEC_k 1x1 classifiers and their Eltwise SUM (train-s.prototxt:461-744) in one pass with float32 weights,
 * float32 accumulation and a float32 NCHW result: out[b][o][hw] = sum_k ( x_k[(b,hw)][:] . w[k][o][:] + bias[k][o] ).
 * x_dev: host array of n_branches (<= 4) device pointers to (B*HW, K) bf16 row-major (NHWC) activations; w_dev
 * (n_branches, O, K) f32; bias_dev (n_branches, O) f32 or NULL; out_dev (B, O, HW) f32.  O <= 32, K % 256 == 0. */
int dsrg_heads_forward_bf16(const void *const *x_dev, int n_branches, const float *w_dev, const float *bias_dev,
                            float *out_dev, int B, int HW, int K, int O, void *stream);
/* Its backward from the float32 score gradient g_dev (B, O, HW):
 *   gx_dev (may be NULL): n_branches matrices (B*HW, K) bf16 row-major, branch k at byte offset k * gx_branch_stride_bytes:
 *                         gx_k[m][c] = sum_o g[m][o] w[k][o][c]                       (float32 accumulation)
 *   gw_dev (may be NULL): (n_branches, O, K) f32: gw[k][o][c] = sum_m g[m][o] x_k[m][c] (exact f32 fma chains, fixed order);
 *                         partial_dev: scratch of dsrg_heads_backward_chunks(B*HW) * n_branches * O * K floats. */
int dsrg_heads_backward_chunks(int M);
int dsrg_heads_backward_bf16(const void *const *x_dev, int n_branches, const float *w_dev, const float *g_dev,
                             void *gx_dev, size_t gx_branch_stride_bytes, float *gw_dev, float *partial_dev, int B,
                             int HW, int K, int O, void *stream);
/* The same with the backward of the ReLU (+ Dropout) layers that produced the x_k folded into the data gradient's store:
 * gx_k[m][c] = relu_scale * sum_o g[m][o] w[k][o][c] where x_k[m][c] > 0, else 0, and bias_grad_dev (n_branches, K) f32 =
 * sum over m of gx_k (the bias gradient of the layer below; fixed summation order).  workspace_dev:
 * dsrg_heads_backward_relu_workspace(n_branches, B*HW, K) bytes.  gw as above (from the unmasked x_k, g). */
size_t dsrg_heads_backward_relu_workspace(int n_branches, int M, int K);
int dsrg_heads_backward_relu_bf16(const void *const *x_dev, int n_branches, const float *w_dev, const float *g_dev,
                                  void *gx_dev, size_t gx_branch_stride_bytes, float *gw_dev, float *partial_dev,
                                  float relu_scale, float *bias_grad_dev, void *workspace_dev, size_t workspace_bytes, int B,
                                  int HW, int K, int O, void *stream);
/* 3x3 max pooling, pad 1, stride 1 or 2, NHWC bf16 (the Pooling layers of train-s.prototxt:69-80 etc.; OH/OW chosen by
 * the caller, ceil mode included).  code_dev: B*OH*OW*C bytes, the window position (3*dy+dx) of the first maximum. */
int dsrg_maxpool3x3_fwd_bf16(const void *in_dev, void *out_dev, void *code_dev, int B, int H, int W, int OH, int OW, int C,
                             int stride, void *stream);
/* The same pooling of a ReLU's OUTPUT when the pool's backward is to carry that ReLU's backward as well: windows whose maximum
 * is not positive get the code 0xfe, which names no window position — their gradient goes nowhere, which is what masking the
 * pooled-back gradient with (input > 0) does (a pixel receives gradient only as the argmax of a window, and its value is
 * that window's maximum).  Pooled values are the same as dsrg_maxpool3x3_fwd_bf16's. */
int dsrg_maxpool3x3_relu_fwd_bf16(const void *in_dev, void *out_dev, void *code_dev, int B, int H, int W, int OH, int OW, int C,
                                  int stride, void *stream);
int dsrg_maxpool3x3_bwd_bf16(const void *gout_dev, const void *code_dev, void *gin_dev, int B, int H, int W, int OH, int OW,
                             int C, int stride, void *stream);
/* Stride-2 pooling backward fused with the ReLU backward and the bias gradient of the convolution in front of the pool
 * (conv + ReLU + pool, train-s.prototxt:65-226): relu_out_dev = the pool's input = that ReLU's output (B,H,W,C) bf16;
 * gin = (relu_out > 0) ? pooled-back gradient : 0 (bit-identical to dsrg_maxpool3x3_bwd_bf16 followed by
 * dsrg_relu_bwd_bias_bf16), bias_grad_dev[c] = sum of gin over (b, y, x).  partials_dev: partial_blocks * C floats;
 * (C / 8) must divide 256.  relu_out_dev may be NULL when code_dev comes from dsrg_maxpool3x3_relu_fwd_bf16: the codes then
 * carry the mask, the pool's input (211 MB at pool1, batch 16) is not read again, and the result is the same bit for bit. */
int dsrg_maxpool3x3_bwd_relu_bf16(const void *gout_dev, const void *code_dev, const void *relu_out_dev, void *gin_dev,
                                  float *bias_grad_dev, float *partials_dev, int partial_blocks, int B, int H, int W, int OH,
                                  int OW, int C, void *stream);

/* The five Python layers of train-s.prototxt:746-810 as ONE stream-ordered
 * sequence (Softmax -> CRF -> DSRG -> BalancedSeedLoss + ConstrainLoss, then
 * the backward pass of A.3 down to d loss / d fc8), computing the CRF once
 * (SURVEY §0.2).  Outputs:
 *   losses_dev[2]   = {loss-Seed, loss-Constrain}
 *   grad_logits_dev = d(loss-Seed + loss-Constrain)/d fc8-SEC      (B,C,H,W)
 *   probs_dev / seeds_dev / logq_dev: optional (may be NULL) copies of the
 *   clipped softmax blob, the grown seeds and the CRF log-marginals.
 * images_dev may be NULL when dsrg_crf_prepare_batch has been called for this batch. */
int dsrg_supervision_step(dsrg_ctx_t ctx, int B, const float *logits_dev, const float *images_dev,
                          int img_h, int img_w, const float *labels_dev, const float *cues_dev,
                          double th1, double th2, const dsrg_crf_params *params,
                          float *losses_dev, float *grad_logits_dev,
                          float *probs_dev, float *seeds_dev, float *logq_dev, void *stream);
/* The same, and total_dev[0] (may be NULL) = losses_dev[0] + losses_dev[1], one float32 add in the kernel that finishes the two
 * losses: what a two-element float32 sum of losses_dev gives, without its launch. */
int dsrg_supervision_step_total(dsrg_ctx_t ctx, int B, const float *logits_dev, const float *images_dev,
                                int img_h, int img_w, const float *labels_dev, const float *cues_dev,
                                double th1, double th2, const dsrg_crf_params *params,
                                float *losses_dev, float *total_dev, float *grad_logits_dev,
                                float *probs_dev, float *seeds_dev, float *logq_dev, void *stream);

/* dsrg_heads_forward_bf16 / dsrg_heads_backward_bf16 / dsrg_heads_backward_relu_bf16 with the branches' kernels, biases and
 * weight gradients where they lie instead of stacked: w_dev / bias_dev / gw_dev are HOST arrays of n_branches device pointers
 * to (O, K) f32 kernels (the memory of a channels_last (O, K, 1, 1) parameter), (O) f32 biases and (O, K) f32 gradient
 * destinations (a parameter's gradient, a slot of a gradient bucket).  bias_dev may be NULL (no bias), gw_dev may be NULL (no
 * weight gradient).  relu_scale > 0: the _relu form (bias_grad_dev and workspace_dev as there), else the plain one.  The same
 * arithmetic in the same order as the stacked forms: identical bits. */
int dsrg_heads_forward_ptrs_bf16(const void *const *x_dev, int n_branches, const float *const *w_dev, const float *const *bias_dev,
                                 float *out_dev, int B, int HW, int K, int O, void *stream);
int dsrg_heads_backward_ptrs_bf16(const void *const *x_dev, int n_branches, const float *const *w_dev, const float *g_dev,
                                  void *gx_dev, size_t gx_branch_stride_bytes, float *const *gw_dev, float *partial_dev,
                                  float relu_scale, float *bias_grad_dev, void *workspace_dev, size_t workspace_bytes, int B,
                                  int HW, int K, int O, void *stream);
/* The network's input in one pass: x_dev (B, 3, H, W) f32 NCHW -> y_dev (B, H, W, 3) bf16 (the memory of a channels_last
 * (B, 3, H, W) tensor), round to nearest even, NaN -> 0x7fc0: the bits of a layout copy followed by a cast. */
int dsrg_image_nchw_to_nhwc_bf16(const float *x_dev, void *y_dev, int B, int H, int W, void *stream);
/* out = rne(rne(rne(g_0 + g_1) + g_2) + g_3) over n (2..4) bf16 tensors of numel elements (a multiple of 8, 16-byte aligned)
 * in one memory order: float32 adds with one bf16 rounding after each, in input order (NaN -> 0x7fc0) — what accumulating n
 * bf16 gradients of one tensor pairwise gives, in one pass.  g_dev: HOST array of n device pointers. */
int dsrg_sum_bf16(const void *const *g_dev, int n, void *out_dev, size_t numel, void *stream);
/* dsrg_sgd_pack_f32 with one more optional output per tensor: cast_dev[i] (may be NULL, as the array itself) receives the new
 * values of parameter i rounded to bf16 (nearest even) in the parameter's own element order — the kernel of a convolution
 * route that reads its weights unpacked (conv1_1).  Only for tensors without fwd_dev[i] / dgrad_dev[i]. */
int dsrg_sgd_pack_cast_f32(int n, float *const *param_dev, const float *const *grad_dev, float *const *momentum_dev,
                           void *const *fwd_dev, void *const *dgrad_dev, void *const *cast_dev, const int *shape,
                           const long long *numel, const float *lr, const float *weight_decay, float momentum, void *stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* DSRG_HIP_H */
