"""Torch-tensor front-end of libdsrg_hip.so: device pointers in, device pointers out.

PyTorch is plumbing here (HBM allocations, streams); all arithmetic happens in the
HIP kernels behind the C ABI (include/dsrg_hip.h).  Every function below names the
reference routine it replaces.
"""
import contextlib
import ctypes
import os
import threading
import weakref as _weakref

import torch

from . import _lib
from ._lib import CrfParams, check
from .crf import select_arrays


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32c(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
    return t


# ---- deferred bias-gradient reductions (dsrg_defer_reductions / dsrg_flush_reductions) -------------------------------------------
# Inside `with deferred_reductions():` the 5-7 us passes that finish a bias gradient (column sums of a data gradient's partial rows,
# the direct kernels' block partials: fifteen per train-s step) are recorded by the library and run in ONE launch when the block
# ends.  This module's part of the contract is to keep alive, until the flush is enqueued, everything that launch touches: every
# recording op takes the scratch its reduction reads from `_reduction_scratch` (inside a block a tensor of the launch's own) and
# the bias gradient it writes from `_bias_grad_dest`; both park what they hand out in `_defer_keep`.
_defer = [False]                       # [0]: inside deferred_reductions()
_defer_keep = []                       # what the flush reads and writes, held until it is enqueued


_scratch = {}


def _stream_scratch(kind, device, nbytes):
    """launch scratch of at least nbytes (uint8), cached per (kind, device index, torch's current stream) and replaced only when it
    is too small.  Launches are stream-ordered, so consecutive users of one buffer never overlap; replacing a buffer that earlier
    launches on the stream still use is safe as well, because torch's allocator hands a freed block only to later work on the
    stream that allocated it."""
    key = (kind, device.index, torch.cuda.current_stream().cuda_stream)
    ws = _scratch.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _scratch[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _reduction_scratch(device, nbytes, kind=None):
    """the scratch (uint8) a launch's bias-gradient reduction reads.  Inside deferred_reductions(): a tensor of the launch's own,
    held until the flush.  Outside: the per-stream buffer of `kind`, or a fresh tensor when no kind is named."""
    if kind is not None and not _defer[0]:
        return _stream_scratch(kind, device, nbytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if _defer[0]:
        _defer_keep.append(ws)
    return ws


def _dest(out, shape, dtype, device, channels_last=False):
    """`out` if it can take a kernel's result of this shape / dtype in place (a reducer's gradient slot: dense, the layout the
    kernel writes), else a fresh tensor"""
    if out is not None and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.device == device and (
            out.is_contiguous(memory_format=torch.channels_last) if channels_last else out.is_contiguous()):
        return out
    if channels_last:
        return torch.empty(shape, dtype=dtype, device=device, memory_format=torch.channels_last)
    return torch.empty(shape, dtype=dtype, device=device)


def _bias_grad_dest(out, shape, device):
    """the float32 destination of a bias gradient: `out` if it can take it (_dest), else a fresh tensor.  Inside deferred_reductions()
    the flush writes it, so its storage is held until then — through an alias, never the tensor itself: AccumulateGrad adopts a
    gradient without copying only while nobody else holds the tensor object (backbone._landed), and a copy made before the flush
    would be a copy of a gradient that is not final"""
    gb = _dest(out, shape, torch.float32, device)
    if _defer[0]:
        _defer_keep.append(gb.detach())
    return gb


@contextlib.contextmanager
def deferred_reductions(enabled=True):
    """inside: bias gradients returned by this module's launches are NOT final until the block ends (nothing may read them; autograd's
    AccumulateGrad adopting a gradient of a parameter whose .grad is None is no read); on exit one launch finishes them all"""
    if not enabled or _defer[0]:
        yield
        return
    L = _lib.lib()
    check(L.dsrg_defer_reductions(1))
    _defer[0] = True
    try:
        yield
    finally:
        rc = L.dsrg_flush_reductions(_stream())
        L.dsrg_defer_reductions(0)
        _defer[0] = False
        del _defer_keep[:]
        check(rc)


class Context(object):
    """dsrg_ctx_t: device workspace for up to max_batch images of shape (C,H,W)."""

    def __init__(self, max_batch, C, H, W):
        _lib.require_gpu()
        self.max_batch, self.C, self.H, self.W = int(max_batch), int(C), int(H), int(W)
        self.device = torch.cuda.current_device()
        h = ctypes.c_void_p()
        check(_lib.lib().dsrg_ctx_create(self.max_batch, self.C, self.H, self.W, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().dsrg_ctx_destroy(h)
            except Exception:                # interpreter teardown: the module globals may already be gone
                pass
            self._h = None

    def profile_start(self, max_launches=4096):
        """bracket every mean-field filter launch with HIP events on the launch stream"""
        check(_lib.lib().dsrg_ctx_profile_start(self._h, int(max_launches)))

    def profile_stop(self):
        """-> (summed filter-kernel milliseconds, number of launches); synchronises"""
        ms, n = ctypes.c_double(0.0), ctypes.c_int32(0)
        check(_lib.lib().dsrg_ctx_profile_stop(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def lattice_sizes(self, B):
        """(M_gaussian, [M_bilateral per image]) of the lattices built by the last CRF call."""
        mg = ctypes.c_int32(0)
        mb = (ctypes.c_int32 * max(B, 1))()
        check(_lib.lib().dsrg_ctx_lattice_sizes(self._h, B, ctypes.byref(mg), mb, _stream()))
        return mg.value, [mb[i] for i in range(B)]

    def lattice_extras(self, B):
        """(X_gaussian, [X_bilateral per image]): splat entries beyond the first of their vertex (bench.py's LDS model)"""
        xg = ctypes.c_int32(0)
        xb = (ctypes.c_int32 * max(B, 1))()
        check(_lib.lib().dsrg_ctx_lattice_extras(self._h, B, ctypes.byref(xg), xb, _stream()))
        return xg.value, [xb[i] for i in range(B)]

    def filter_plan(self, B):
        """(planes per bilateral workgroup, planes per Gaussian workgroup, workgroups, LDS bytes) of a filter launch over B
        images as the launcher plans it now (bench.py's LDS model)"""
        v = [ctypes.c_int32(0) for _ in range(4)]
        check(_lib.lib().dsrg_ctx_filter_plan(self._h, int(B), *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def lattice_dump(self, kind, b=0):
        """One lattice in the reference's own form (tests): kind 0 = Gaussian, 1 = bilateral lattice of image b.
        -> dict(M, keys (M,d) int16, vid (N,d+1) int32, bary (N,d+1) f32, n1 / n2 (d+1,M) int32 with -1 = none)."""
        import numpy as np
        d, N = (2, self.H * self.W) if kind == 0 else (5, self.H * self.W)
        m = ctypes.c_int32(0)
        L = _lib.lib()
        check(L.dsrg_ctx_lattice_dump(self._h, kind, b, ctypes.byref(m), None, None, None, None, None, _stream()))
        M = m.value
        keys = np.empty((M, d), np.int16)
        vid = np.empty((N, d + 1), np.int32)
        bary = np.empty((N, d + 1), np.float32)
        n1 = np.empty((d + 1, M), np.int32)
        n2 = np.empty((d + 1, M), np.int32)
        check(L.dsrg_ctx_lattice_dump(self._h, kind, b, ctypes.byref(m), keys.ctypes.data, vid.ctypes.data, bary.ctypes.data,
                                      n1.ctypes.data, n2.ctypes.data, _stream()))
        return dict(M=M, keys=keys, vid=vid, bary=bary, n1=n1, n2=n2)

    def lattice_norm(self, kind, b=0):
        """norm = 1/sqrt(K 1 + 1e-20) of one lattice (pairwise.cpp:44,54-57), (N,) float32 numpy (tests)"""
        import numpy as np
        out = np.empty(self.H * self.W, np.float32)
        check(_lib.lib().dsrg_ctx_lattice_norm(self._h, kind, b, out.ctypes.data, _stream()))
        return out

    def filter_once(self, kind, q):
        """one application of the normalised kernel `kind` (0 Gaussian, 1 bilateral) to q (B,C,H,W) with the lattices of
        the last CRF call on this context: DenseKernel::filter (pairwise.cpp:63-80) (tests)"""
        _f32c(q, "q")
        out = torch.empty_like(q)
        check(_lib.lib().dsrg_ctx_filter_once(self._h, kind, q.shape[0], _ptr(q), _ptr(out), _stream()))
        return out

    def read_refined(self, B):
        """float64 marginals (B,C,H,W) the last supervision_step on this context thresholded (tests)"""
        out = torch.empty((B, self.C, self.H, self.W), dtype=torch.float64, device="cuda")
        check(_lib.lib().dsrg_ctx_read_refined(self._h, B, _ptr(out), _stream()))
        return out


_CTX_CACHE = {}
_CTX_LOCK = threading.Lock()


# The LDS-resident path (contexts, the fused step) provisions every lattice for its WORST case — 6 * 4 * ceil(N / 4) vertices for
# N = H * W pixels, whatever the image — so which maps it takes is a function of N alone (include/dsrg_hip.h): N <= 4488, i.e.
# 41x41, 65x65, 66x68; 67x67 is the first square map beyond.  Larger maps take the global-memory path through the same Python
# entry points (crf_refine, supervision_step, dsrg_supervision_loss): the batched full-resolution CRF + the stand-alone
# kernels of the other layers, composed in the order of train-s.prototxt:746-810.
LDS_PATH_MAX_PIXELS = 4488


def lds_path_supports(H, W):
    return H * W <= LDS_PATH_MAX_PIXELS


def get_context(B, C, H, W):
    """the cached workspace of (device, host thread, C, H, W): a context is used by one host thread at a time
    (include/dsrg_hip.h), so every thread gets its own"""
    key = (torch.cuda.current_device(), threading.get_ident(), C, H, W)
    with _CTX_LOCK:
        ctx = _CTX_CACHE.get(key)
        if ctx is None or ctx.max_batch < B:
            ctx = Context(max(B, 1), C, H, W)
            _CTX_CACHE[key] = ctx
    return ctx


def softmax_forward(x):
    """SoftmaxLayer.forward (pylayers.py:46-47)."""
    _f32c(x, "x")
    B, C, H, W = x.shape
    p = torch.empty_like(x)
    check(_lib.lib().dsrg_softmax_forward(B, C, H * W, _ptr(x), _ptr(p), _stream()))
    return p


def softmax_backward(x, top_diff):
    """SoftmaxLayer.backward (pylayers.py:49-51)."""
    _f32c(x, "x"), _f32c(top_diff, "top_diff")
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().dsrg_softmax_backward(B, C, H * W, _ptr(x), _ptr(top_diff), _ptr(dx), _stream()))
    return dx


def crf_refine(probs, images, scale_factor=12.0, maxiter=10, ctx=None, want_log=True, prepared=False):
    """CRFLayer.forward / DSRGLayer.refinement (pylayers.py:63-88,310-331).

    probs (B,C,H,W) f32 is clipped IN PLACE (as the reference does to its bottom blob);
    returns (refined float64 (B,C,H,W), log-marginals float32 or None).  prepared: the lattices of `images` were built
    by crf_prepare on this context (e.g. on a side stream under the backbone forward)."""
    _f32c(probs, "probs"), _f32c(images, "images")
    B, C, H, W = probs.shape
    if images.shape[0] != B or images.shape[1] != 3:
        raise ValueError("images must be (B,3,Hi,Wi)")
    if not lds_path_supports(H, W):
        return _crf_refine_large(probs, images, scale_factor, maxiter, want_log)
    ctx = ctx or get_context(B, C, H, W)
    refined = torch.empty((B, C, H, W), dtype=torch.float64, device=probs.device)
    logq = torch.empty_like(probs) if want_log else None
    prm = CrfParams.from_crf_args(maxiter, scale_factor)
    check(_lib.lib().dsrg_crf_refine_batch(ctx._h, B, _ptr(probs), None if prepared else _ptr(images), images.shape[2],
                                           images.shape[3], ctypes.byref(prm), _ptr(refined), _ptr(logq), _stream()))
    return refined, logq


MEAN_PIXEL = (104.0, 117.0, 123.0)      # B, G, R (test-ms.py:79; inference.MEAN_PIXEL)


def _map_images_u8(images, H, W):
    """(B,3,Hi,Wi) mean-subtracted float images -> (B,H,W,3) uint8 at the map's size: zoom(order=1) with the (in-1)/(out-1)
    mapping evaluated in double, rounded once to float, + mean pixel, np.round, astype(ubyte) (pylayers.py:70-75) — what
    map_pixel_rgb (csrc/embed.h) does inside the LDS path's embedding kernel"""
    import torch.nn.functional as F
    x = images
    if x.shape[2] != H or x.shape[3] != W:
        x = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=True).float()
    mean = torch.tensor(MEAN_PIXEL, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)
    v = torch.round(x.double() + mean).to(torch.int64) & 0xff                    # half-even, then C's conversion to unsigned char
    return v.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _crf_refine_large(probs, images, scale_factor, maxiter, want_log):
    """crf_refine beyond the LDS path: the in-place clip, the mean field through the batched global-memory objects
    (crf.CRF_device_batch; one image per object when a batch's spatial kernel is too narrow for the image tag), then the
    reference's float64 clip / renormalisation / log (pylayers.py:84-88)"""
    from .crf import CRF_device, CRF_device_batch
    probs.clamp_(min=1e-4)                                                       # pylayers.py:65-67
    B, C, H, W = probs.shape
    im = _map_images_u8(images, H, W)
    un = probs.permute(0, 2, 3, 1).contiguous()
    try:
        q = CRF_device_batch(im, un, maxiter, scale_factor)
    except _lib.DsrgError as e:
        if e.code != _lib.ERR_UNSUPPORTED:                                       # out of memory, a HIP fault: not ours to retry
            raise
        q = torch.stack([CRF_device(im[b], un[b], maxiter, scale_factor) for b in range(B)])
    q64 = q.permute(0, 3, 1, 2).double().clamp_min(1e-4)
    refined = (q64 / q64.sum(1, keepdim=True)).contiguous()
    return refined, (torch.log(refined).float().contiguous() if want_log else None)


def crf_prepare(images, C, H, W, scale_factor=12.0, maxiter=10, ctx=None):
    """Image-dependent half of the CRF (image resampling + bilateral lattice build) on the current
    stream; a later supervision_step(..., prepared=True) on the same context skips it.  Lets a trainer
    hide the lattice build under the backbone forward (side stream).  It overwrites the context's lattices: on a side
    stream, order it behind the last mean field that reads them (`side.wait_stream(main)`, as DSRGTrainer.step does)."""
    _f32c(images, "images")
    B = images.shape[0]
    if not lds_path_supports(H, W):
        return None                      # the global-memory path builds its lattices inside the call that uses them
    ctx = ctx or get_context(B, C, H, W)
    prm = CrfParams.from_crf_args(maxiter, scale_factor)
    check(_lib.lib().dsrg_crf_prepare_batch(ctx._h, B, _ptr(images), images.shape[2], images.shape[3],
                                            ctypes.byref(prm), _stream()))
    return ctx


def crf_meanfield(unary, im_u8, maxiter=10, scale_factor=1.0, color_factor=13, ctx=None, params=None):
    """krahenbuhl2013.CRF on device blobs: unary (B,C,H,W) f32 (the `unary` argument of CRF.py:28,
    i.e. minus the energy), im_u8 (B,H,W,3) uint8 -> marginals (B,C,H,W) f32.  params: a ready CrfParams (kernel weights,
    widths and iteration count) instead of the ones CRF() derives from maxiter / scale_factor / color_factor."""
    _f32c(unary, "unary")
    if not (im_u8.is_cuda and im_u8.dtype == torch.uint8 and im_u8.is_contiguous()):
        raise ValueError("im_u8 must be a contiguous uint8 CUDA tensor")
    B, C, H, W = unary.shape
    ctx = ctx or get_context(B, C, H, W)
    q = torch.empty_like(unary)
    prm = params if params is not None else CrfParams.from_crf_args(maxiter, scale_factor, color_factor)
    check(_lib.lib().dsrg_crf_meanfield_batch(ctx._h, B, _ptr(unary), _ptr(im_u8), ctypes.byref(prm), _ptr(q),
                                              _stream()))
    return q


def crf_layer_backward(refined, top_diff):
    """CRFLayer.backward (pylayers.py:90-92)."""
    _f32c(top_diff, "top_diff")
    if not (refined.is_cuda and refined.dtype == torch.float64 and refined.is_contiguous()):
        raise ValueError("refined must be a contiguous float64 CUDA tensor")
    out = torch.empty_like(top_diff)
    check(_lib.lib().dsrg_crf_layer_backward(refined.numel(), _ptr(refined), _ptr(top_diff), _ptr(out), _stream()))
    return out


def srg_grow(labels, cues, refined, th1=0.99, th2=0.85):
    """DSRGLayer.generate_seed -> generate_seed_step (pylayers.py:237-275,333-344)."""
    _f32c(labels, "labels"), _f32c(cues, "cues")
    if not (refined.is_cuda and refined.dtype == torch.float64 and refined.is_contiguous()):
        raise ValueError("refined must be a contiguous float64 CUDA tensor")
    B, C, H, W = cues.shape
    if labels.numel() != B * C:
        raise ValueError("labels must hold B*C values")
    seeds = torch.empty_like(cues)
    scratch = torch.empty(B * H * W, dtype=torch.int16, device=cues.device)
    check(_lib.lib().dsrg_srg_grow_batch(B, C, H, W, _ptr(labels), _ptr(cues), _ptr(refined), float(th1), float(th2),
                                         _ptr(seeds), _ptr(scratch), _stream()))
    return seeds


def seed_loss(probs, seeds, want_grad=True, want_loss=True):
    """BalancedSeedLossLayer.forward/backward (pylayers.py:147-152) -> (loss[1] or None, grad or None)."""
    _f32c(probs, "probs"), _f32c(seeds, "seeds")
    B, C, H, W = probs.shape
    loss = torch.empty(1, dtype=torch.float32, device=probs.device) if want_loss else None
    grad = torch.empty_like(probs) if want_grad else None
    check(_lib.lib().dsrg_seed_loss(B, C, H * W, _ptr(probs), _ptr(seeds), _ptr(loss), _ptr(grad), _stream()))
    return loss, grad


def constrain_loss(probs, logq, want_grad=True, want_loss=True):
    """ConstrainLossLayer.forward/backward (pylayers.py:173-180) -> (loss[1] or None, grad_probs, grad_logq)."""
    _f32c(probs, "probs"), _f32c(logq, "logq")
    B, C, H, W = probs.shape
    loss = torch.empty(1, dtype=torch.float32, device=probs.device) if want_loss else None
    gp = torch.empty_like(probs) if want_grad else None
    gq = torch.empty_like(probs) if want_grad else None
    check(_lib.lib().dsrg_constrain_loss(B, C, H * W, _ptr(probs), _ptr(logq), _ptr(loss), _ptr(gp), _ptr(gq),
                                         _stream()))
    return loss, gp, gq


def seed_loss_plain(probs, seeds, want_grad=True):
    """SeedLossLayer forward/backward (pylayers.py:94-118) -> (loss (1,), grad or None)."""
    _f32c(probs, "probs"), _f32c(seeds, "seeds")
    B, C, H, W = probs.shape
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    grad = torch.empty_like(probs) if want_grad else None
    check(_lib.lib().dsrg_seed_loss_plain(B, C, H * W, _ptr(probs), _ptr(seeds), _ptr(loss), _ptr(grad), _stream()))
    return loss, grad


def expand_loss(probs, stat, want_grad=True, q_fg=0.996, q_bg=0.999):
    """ExpandLossLayer forward/backward (pylayers.py:183-233): probs (B,C,H,W), stat (B,1,1,C) image-level labels."""
    _f32c(probs, "probs"), _f32c(stat, "stat")
    B, C, H, W = probs.shape
    if stat.numel() != B * C:
        raise ValueError("stat must hold B*C values")
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    grad = torch.empty_like(probs) if want_grad else None
    scratch = torch.empty(B * C, dtype=torch.float64, device=probs.device)
    check(_lib.lib().dsrg_expand_loss(B, C, H * W, _ptr(probs), _ptr(stat), float(q_fg), float(q_bg), _ptr(loss), _ptr(grad),
                                      _ptr(scratch), _stream()))
    return loss, grad


def confusion_matrix(gt, pred, nclass, rule_lt=False, hist=None):
    """evaluate.py:25-30 (`add`: gt != 255) / :61-68 (`generateM`: gt < nclass) on uint8 CUDA tensors.
    Returns the (nclass*nclass + 1) int64 counters (added to `hist` when given); the last counts out-of-range labels."""
    if not (gt.is_cuda and pred.is_cuda and gt.dtype == torch.uint8 and pred.dtype == torch.uint8):
        raise ValueError("gt and pred must be uint8 CUDA tensors")
    gt, pred = gt.contiguous(), pred.contiguous()
    if gt.numel() != pred.numel():
        raise ValueError("gt and pred differ in size")
    if hist is None:
        hist = torch.zeros(nclass * nclass + 1, dtype=torch.int64, device=gt.device)
    check(_lib.lib().dsrg_confusion_matrix(gt.numel(), _ptr(gt), _ptr(pred), int(nclass), int(bool(rule_lt)), _ptr(hist),
                                           _stream()))
    return hist


def eval_confusion_batch(scores, labels, nclass, ignore_label=255, rule_lt=False, hist=None):
    """Validation scoring of a batch in one launch (dsrg_eval_confusion_batch): scores (>= B, nclass, h, w) and labels (B, 1, Hz, Wz),
    contiguous float32 CUDA tensors — the network's score maps and the label maps train_f_input_batch returns (ignore_label off the
    image).  The first B slices of scores are zoomed to Hz x Wz with multiscale_unary's arithmetic, their first maximum over the
    labels is the prediction, and the pixels whose label passes the rule (rule_lt False: label != ignore_label; True: label <
    nclass) are counted.  Returns the (nclass*nclass + 1) int64 counters of confusion_matrix (added to `hist` when given); the last
    counts kept labels that are not one of 0..nclass-1.  Nothing else is written.  Runs on torch's current stream."""
    for t, name in ((scores, "scores"), (labels, "labels")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
    nclass = int(nclass)
    if scores.dim() != 4 or scores.shape[1] != nclass:
        raise ValueError("scores must be (>= B, %d, h, w), got %s" % (nclass, tuple(scores.shape)))
    if labels.dim() != 4 or labels.shape[1] != 1:
        raise ValueError("labels must be (B, 1, Hz, Wz), got %s" % (tuple(labels.shape),))
    B, _, Hz, Wz = labels.shape
    if B > scores.shape[0]:
        raise ValueError("%d label maps for %d score maps" % (B, scores.shape[0]))
    if hist is None:
        hist = torch.zeros(nclass * nclass + 1, dtype=torch.int64, device=scores.device)
    elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == nclass * nclass + 1):
        raise ValueError("hist must be a contiguous int64 CUDA tensor of %d counters" % (nclass * nclass + 1))
    check(_lib.lib().dsrg_eval_confusion_batch(int(B), nclass, _ptr(scores), int(scores.shape[2]), int(scores.shape[3]), _ptr(labels),
                                               int(Hz), int(Wz), float(ignore_label), int(bool(rule_lt)), _ptr(hist), _stream()))
    return hist


def seg_loss_zoom(logits, labels, ignore_label=255, counters=None):
    """Softmax loss at label resolution in two launches (dsrg_seg_loss_zoom_batch): logits (>= B, C, h, w) and labels (B, 1, H, W),
    contiguous float32 CUDA tensors — the network's score maps and the label maps train_f_input_batch returns.  The first B slices
    of logits are zoomed to H x W with eval_confusion_batch's arithmetic and the loss is the mean of -log softmax(z)[label] over
    the valid pixels of the batch (label one of 0..C-1 and not ignore_label).  Returns (loss: 0-dim float32, grad: (B, C, h, w)
    float32 = d loss / d logits, counters: 3 int64 — valid pixels, valid pixels the argmax gets right, invalid labels — ADDED to
    `counters` when given).  No valid pixel: loss 0 and a zero gradient.  Bit-reproducible; runs on torch's current stream."""
    for t, name in ((logits, "logits"), (labels, "labels")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
    if logits.dim() != 4:
        raise ValueError("logits must be (>= B, C, h, w), got %s" % (tuple(logits.shape),))
    if labels.dim() != 4 or labels.shape[1] != 1:
        raise ValueError("labels must be (B, 1, H, W), got %s" % (tuple(labels.shape),))
    B, _, H, W = labels.shape
    C, h, w = (int(v) for v in logits.shape[1:])
    if B > logits.shape[0]:
        raise ValueError("%d label maps for %d logit maps" % (B, logits.shape[0]))
    dev = logits.device
    if counters is None:
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
    elif not (counters.is_cuda and counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 3):
        raise ValueError("counters must be a contiguous int64 CUDA tensor of 3 counters")
    L = _lib.lib()
    need = L.dsrg_seg_loss_zoom_workspace(int(B), C, h, w, int(H), int(W))        # (0 for a refused shape: the launch names it)
    ws = _stream_scratch("seg_loss_zoom", dev, max(int(need), 8))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((int(B), C, h, w), dtype=torch.float32, device=dev)
    check(L.dsrg_seg_loss_zoom_batch(int(B), C, _ptr(logits), h, w, _ptr(labels), int(H), int(W), float(ignore_label), _ptr(loss),
                                     _ptr(grad), _ptr(counters), _ptr(ws), ws.numel(), _stream()))
    return loss, grad, counters


class SegLossZoomFn(torch.autograd.Function):
    """seg_loss_zoom as a differentiable scalar: the launch runs in forward and leaves the gradient, backward returns grad * g —
    float32 NCHW contiguous, where the classifier heads' backward takes it.  apply(logits, labels, ignore_label, counters)"""

    @staticmethod
    def forward(ctx, logits, labels, ignore_label, counters):
        x = logits.detach()
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.float().contiguous()
        loss, grad, _ = seg_loss_zoom(x, labels, ignore_label, counters)
        ctx.save_for_backward(grad)
        ctx.full = logits.shape[0]
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        out = grad * g
        if ctx.full != out.shape[0]:                                              # (slices beyond the label maps took no part)
            out = torch.cat([out, out.new_zeros((ctx.full - out.shape[0],) + tuple(out.shape[1:]))])
        return out, None, None, None


def _int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def msc_pyramid(images, sizes):
    """The smaller inputs of a multi-scale step in one launch (dsrg_msc_pyramid_batch): images (B, 3, H, W) contiguous float32 NCHW
    (the loader's mean-subtracted crop), sizes 1..3 pairs (h, w) or single sides -> a list of (B, 3, h, w) float32 tensors in
    torch.channels_last, each the align-corners zoom of eval_confusion_batch (blend in double, rounded once)."""
    if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float32 and images.is_contiguous()):
        raise ValueError("images must be a contiguous float32 CUDA tensor")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("images must be (B, 3, H, W), got %s" % (tuple(images.shape),))
    sizes = [(int(s), int(s)) if isinstance(s, int) else (int(s[0]), int(s[1])) for s in sizes]
    if not 1 <= len(sizes) <= 3:
        raise ValueError("1..3 sizes, got %d" % len(sizes))
    B, _, H, W = (int(v) for v in images.shape)
    outs = [torch.empty((B, 3, max(h, 1), max(w, 1)), dtype=torch.float32, device=images.device, memory_format=torch.channels_last)
            for h, w in sizes]
    check(_lib.lib().dsrg_msc_pyramid_batch(B, _ptr(images), H, W, len(sizes), _int_array([h for h, _ in sizes]),
                                            _int_array([w for _, w in sizes]), _ptr_array(outs), _stream()))
    return outs


def msc_loss(maps, labels, ignore_label=255, counters=None):
    """The S + 1 softmax losses of a multi-scale step with max fusion in three launches (dsrg_msc_loss_batch): maps, a list of
    2..4 contiguous float32 CUDA score maps (B, C, h_s, w_s) with map 0 the full scale, and labels (B, 1, H, W) float32.  The other
    maps are zoomed to map 0 (eval_confusion_batch's arithmetic), the element-wise maximum is the fused map (ties go to the lowest
    scale index); the fused map and every map are judged against the nearest label sample at their own resolution.  Returns
    (losses: S + 1 float32 — fused, map 0, map 1, ... —, grads: a list of (B, C, h_s, w_s) float32 = d (sum of the losses) / d map s,
    counters: 3 int64 of the fused head — valid pixels, valid pixels the argmax gets right, invalid labels — ADDED to `counters`
    when given).  Nothing valid: losses 0 and zero gradients.  Bit-reproducible; runs on torch's current stream."""
    maps = list(maps)
    if not 2 <= len(maps) <= 4:
        raise ValueError("2..4 score maps, got %d" % len(maps))
    for t, name in [(m, "maps[%d]" % k) for k, m in enumerate(maps)] + [(labels, "labels")]:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
    if labels.dim() != 4 or labels.shape[1] != 1:
        raise ValueError("labels must be (B, 1, H, W), got %s" % (tuple(labels.shape),))
    B, _, H, W = (int(v) for v in labels.shape)
    if any(m.dim() != 4 or tuple(m.shape[:2]) != tuple(maps[0].shape[:2]) for m in maps) or maps[0].shape[0] != B:
        raise ValueError("score maps must be (%d, C, h, w) with one C, got %s" % (B, [tuple(m.shape) for m in maps]))
    C = int(maps[0].shape[1])
    dev = maps[0].device
    if counters is None:
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
    elif not (counters.is_cuda and counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 3):
        raise ValueError("counters must be a contiguous int64 CUDA tensor of 3 counters")
    L = _lib.lib()
    S = len(maps)
    hs, ws_ = _int_array([m.shape[2] for m in maps]), _int_array([m.shape[3] for m in maps])
    need = L.dsrg_msc_loss_workspace(S, B, C, hs, ws_, H, W)                      # (0 for a refused shape: the launch names it)
    ws = _stream_scratch("msc_loss", dev, max(int(need), 8))
    losses = torch.empty(S + 1, dtype=torch.float32, device=dev)
    grads = [torch.empty_like(m) for m in maps]
    check(L.dsrg_msc_loss_batch(S, B, C, _ptr_array(maps), hs, ws_, _ptr(labels), H, W, float(ignore_label), _ptr(losses),
                                _ptr_array(grads), _ptr(counters), _ptr(ws), ws.numel(), _stream()))
    return losses, grads, counters


class MscLossFn(torch.autograd.Function):
    """msc_loss as a differentiable scalar: the launch runs in forward and leaves the gradients of the SUM of the S + 1 heads (each
    of weight 1, as in the recipe); backward returns grad_s * g for every map — float32 NCHW contiguous, where the classifier
    heads' backward takes it.  apply(labels, ignore_label, counters, map_0, map_1, ...) -> (total: 0-dim, the sum of the losses in
    float32, differentiable; losses: S + 1 float32 — fused, map 0, map 1, ... —, not differentiable)"""

    @staticmethod
    def forward(ctx, labels, ignore_label, counters, *maps):
        xs = [m.detach() if (m.dtype == torch.float32 and m.is_contiguous()) else m.detach().float().contiguous() for m in maps]
        losses, grads, _ = msc_loss(xs, labels, ignore_label, counters)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(losses)
        return losses.sum(), losses

    @staticmethod
    def backward(ctx, g, _):
        return (None, None, None) + tuple(grad * g for grad in ctx.saved_tensors)


def score_labels_batch(labels, gts, nclass, ignore_label=255, rule_lt=False, hist=None, masks=None):
    """Scoring of a group of finished label maps in one launch (dsrg_score_labels_batch): labels, a list of 1..16 contiguous (H_g,
    W_g) int32 CUDA tensors (the CRF's map, the argmax / labels outputs of the multi-scale and pseudo-label tails; sizes may
    differ), and gts, as many contiguous uint8 CUDA tensors of the same sizes.  The pixels whose ground truth passes the rule
    (rule_lt False: gt != ignore_label; True: gt < nclass) are counted.  masks: None, or as many contiguous uint8 CUDA tensors of
    those sizes, which get every pixel's label as a byte (255 for a label outside 0..255).  Returns the (nclass*nclass + 1) int64
    counters of confusion_matrix (added to `hist` when given); the last counts kept pixels whose ground truth or label is not one
    of 0..nclass-1.  Runs on torch's current stream."""
    labels, gts = list(labels), list(gts)
    nclass = int(nclass)
    if not labels or len(gts) != len(labels) or (masks is not None and len(masks) != len(labels)):
        raise ValueError("%d label maps, %d ground truths%s" % (len(labels), len(gts),
                                                                "" if masks is None else ", %d masks" % len(masks)))
    for name, ts, dtype in (("labels", labels, torch.int32), ("gts", gts, torch.uint8), ("masks", masks, torch.uint8)):
        for g, t in enumerate(ts or ()):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
                raise ValueError("%s[%d] must be a contiguous %s CUDA tensor" % (name, g, str(dtype).split(".")[-1]))
            if t.dim() != 2 or t.shape != labels[g].shape:
                raise ValueError("%s[%d] is %s, label map %d is %s" % (name, g, tuple(t.shape), g, tuple(labels[g].shape)))
    if hist is None:
        hist = torch.zeros(nclass * nclass + 1, dtype=torch.int64, device=labels[0].device)
    elif not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == nclass * nclass + 1):
        raise ValueError("hist must be a contiguous int64 CUDA tensor of %d counters" % (nclass * nclass + 1))
    check(_lib.lib().dsrg_score_labels_batch(len(labels), nclass, _ptrs(labels), _ptrs(gts), _i32s([t.shape[0] for t in labels]),
                                             _i32s([t.shape[1] for t in labels]), int(ignore_label), int(bool(rule_lt)), _ptr(hist),
                                             _ptrs(masks), _stream()))
    return hist


_MS_OUTPUTS = ("unary", "argmax", "sum")
_TG_OUTPUTS = ("unary", "probs", "labels")
_INT_OUTPUTS = ("argmax", "labels")                  # (H, W) int32 maps; every other output is (H, W, C) float32


def _want_names(want, allowed):
    """a `want=` argument -> (names, single): a string names one output and asks for it bare, a sequence for tuples in its order"""
    single = isinstance(want, str)
    names = (want,) if single else tuple(want)
    for n in names:
        if n not in allowed:
            raise ValueError("unknown output %r (choose from %s)" % (n, ", ".join(allowed)))
    if not names:
        raise ValueError("want names no output")
    return names, single


def _want_outputs(names, shapes, C, device):
    """-> {name: [one output tensor per (H, W) of shapes]}"""
    return {n: [torch.empty((H, W) if n in _INT_OUTPUTS else (H, W, C), dtype=torch.int32 if n in _INT_OUTPUTS else torch.float32,
                            device=device) for H, W in shapes] for n in names}


def _ptrs(tensors):
    """host array of one device pointer per entry (null for a None entry); None: no array"""
    if tensors is None:
        return None
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _multiscale_args(scores, want, batched):
    """the shared front end of multiscale_unary and its batched forms: the `want` names, the checks of the score maps ((1, C, h, w)
    each, batched: one leading extent Gcap) and the launch's host arrays -> (names, single, scores, Gcap, C, (K, C, map pointers,
    map heights, map widths))"""
    names, single = _want_names(want, _MS_OUTPUTS)
    scores = [_f32c(s, "scores[%d]" % k) for k, s in enumerate(scores)]
    if not scores:
        raise ValueError("no score maps")
    if batched and scores[0].dim() != 4:
        raise ValueError("score maps must be (Gcap, C, h, w); got %s" % (tuple(scores[0].shape),))
    Gcap, C = scores[0].shape[0] if batched else 1, scores[0].shape[1]
    for s in scores:
        if s.dim() != 4 or s.shape[0] != Gcap or s.shape[1] != C:
            raise ValueError("score maps must be %s; got %s" % ("(Gcap, C, h, w) with one Gcap and one C" if batched
                                                                else "(1, C, h, w) with one C", tuple(s.shape)))
    K = len(scores)
    return names, single, scores, Gcap, C, (K, int(C), (ctypes.c_void_p * K)(*[s.data_ptr() for s in scores]),
                                            _i32s([s.shape[2] for s in scores]), _i32s([s.shape[3] for s in scores]))


def multiscale_unary(scores, H, W, eps=1e-5, want=("unary",), mirror=None):
    """test-ms.py:90-103 / test-ms-f.py:121-134 after the forwards, in one launch (dsrg_multiscale_unary): the K score maps
    zoomed to H x W, summed in scale order, softmax over labels clamped at eps.  scores: list of (1, C, h_k, w_k) float32 CUDA
    tensors (sizes may differ).  want: names among "unary" ((H, W, C) f32 log-probabilities, the layout CRF_device takes),
    "argmax" ((H, W) int32, the first maximum) and "sum" ((H, W, C) f32 summed scores, for parity checks).  A string returns
    that one tensor, a sequence a tuple in its order.  mirror: one flag per map (dsrg_multiscale_unary_mirror): a map whose flag
    is set is read with its columns reversed, the result being that of this call on torch.flip(map, [-1]) bit for bit (the
    scores of a mirrored network input, mirrored back); None: today's kernel.  Runs on torch's current stream."""
    names, single, scores, _, C, (K, C, ptrs, hs, ws) = _multiscale_args(scores, want, False)
    out = {n: ts[0] for n, ts in _want_outputs(names, [(H, W)], C, scores[0].device).items()}
    tail = (hs, ws, int(H), int(W), float(eps), _ptr(out.get("unary")), _ptr(out.get("argmax")), _ptr(out.get("sum")), _stream())
    if mirror is None:
        check(_lib.lib().dsrg_multiscale_unary(K, C, ptrs, *tail))
    else:
        mirror = [int(bool(m)) for m in mirror]
        if len(mirror) != K:
            raise ValueError("mirror must hold one flag per score map: %d flags for %d maps" % (len(mirror), K))
        check(_lib.lib().dsrg_multiscale_unary_mirror(K, C, ptrs, _i32s(mirror), *tail))
    res = tuple(out[n] for n in names)
    return res[0] if single else res


def multiscale_unary_batch(scores, shapes, eps=1e-5, want=("unary",)):
    """multiscale_unary for the G images of a group in one launch (dsrg_multiscale_unary_batch), for the fixed sizes of
    test-ms.py, where every image of a group has the same score map sizes.  scores: list of K (Gcap, C, h_k, w_k) float32 CUDA
    tensors, image g reads slice g; shapes: the G <= min(Gcap, 16) output sizes (H_g, W_g).  want: as multiscale_unary.  Returns a
    list of G entries, each what multiscale_unary(slices g, H_g, W_g, eps, want) returns, bit for bit.  Runs on torch's current
    stream."""
    return _multiscale_unary_batch(scores, shapes, eps, want, False)


def _multiscale_unary_batch(scores, shapes, eps, want, mirror):
    """multiscale_unary_batch (one slice per image) / multiscale_unary_mirror_batch (mirror: two)"""
    names, single, scores, Gcap, C, arrays = _multiscale_args(scores, want, True)
    shapes = [(int(H), int(W)) for H, W in shapes]
    G = len(shapes)
    if not 1 <= G * (2 if mirror else 1) <= Gcap:
        raise ValueError("%d output shapes for score maps of %d %s" % (G, Gcap, "slices, two per image" if mirror else "images"))
    out = _want_outputs(names, shapes, C, scores[0].device)
    entry = _lib.lib().dsrg_multiscale_unary_mirror_batch if mirror else _lib.lib().dsrg_multiscale_unary_batch
    check(entry(G, *arrays, _i32s([H for H, _ in shapes]), _i32s([W for _, W in shapes]), float(eps), _ptrs(out.get("unary")),
                _ptrs(out.get("argmax")), _ptrs(out.get("sum")), _stream()))
    if single:
        return out[names[0]]
    return [tuple(out[n][g] for n in names) for g in range(G)]


def multiscale_unary_mirror_batch(scores, shapes, eps=1e-5, want=("unary",)):
    """multiscale_unary_batch for mirrored test-time augmentation, in one launch (dsrg_multiscale_unary_mirror_batch).  scores: list
    of K <= 4 (Gcap, C, h_k, w_k) float32 CUDA tensors, the outputs of batched forwards on preprocess_rect_mirror_batch's inputs:
    image g reads slice 2g plain and slice 2g+1 mirrored back; shapes: the G <= min(Gcap // 2, 8) output sizes (H_g, W_g).  Per
    pixel the sum runs scale 0 plain, scale 0 mirror, scale 1 plain, ...  Returns a list of G entries, each what
    multiscale_unary([s_0[2g], s_0[2g+1], s_1[2g], ...], H_g, W_g, eps, want, mirror=[0, 1, 0, 1, ...]) returns, bit for bit.
    Runs on torch's current stream."""
    return _multiscale_unary_batch(scores, shapes, eps, want, True)


def train_gt_unary_batch(scores, shapes, eps=1e-5, want=("unary",), select=None, ignore_below=None):
    """generate_train_gt.py:85-104 after the forward, for the G images of a group (dsrg_train_gt_unary_batch): softmax over
    labels at map resolution, the probabilities zoomed to each image's H x W, clamped at eps.  scores: ONE (Gcap, C, h, w) float32
    CUDA tensor, image g reads slice g; shapes: the G <= min(Gcap, 16) output sizes (H_g, W_g).  want: names among "unary"
    ((H, W, C) f32 log-probabilities, the layout CRF_device takes), "probs" ((H, W, C) f32, for parity checks) and "labels"
    ((H, W) int32: per pixel the first maximum over the image's list select[g] — an ordered sequence of 1..128 labels, e.g.
    inference.train_gt_selection(labels) — or 255 where the largest probability over all labels is below ignore_below; None or
    <= 0: off).  A string returns the list of that one tensor per image, a sequence a list of tuples in its order.  Image g's
    results equal those of a G = 1 call on slice g bit for bit.  It is train_gt_ensemble_batch([scores], flip=False): the same
    kernels, one map per image, no sum and no division.  Runs on torch's current stream; the workspace (G * C * h * w floats) is a
    torch tensor."""
    names = _want_names(want, _TG_OUTPUTS)
    if not torch.is_tensor(scores):
        raise ValueError("scores must be one (Gcap, C, h, w) tensor")
    return _train_gt_batch([scores], shapes, False, eps, names, select, ignore_below)


def train_gt_ensemble_batch(scores, shapes, flip=False, eps=1e-5, want=("unary",), select=None, ignore_below=None):
    """train_gt_unary_batch as a probability ensemble over K sizes, with flip=True each also on the mirrored input
    (dsrg_train_gt_ensemble_batch; no counterpart in the reference).  scores: list of K (Gcap, C, h_k, w_k) float32 CUDA tensors;
    image g reads slice g, with flip slice 2g plain and slice 2g+1 mirrored (the outputs of batched forwards on
    preprocess_rect_mirror_batch's inputs); K * (1 + flip) <= 8.  shapes: the G output sizes (H_g, W_g), G <= min(Gcap, 16), with
    flip G <= min(Gcap // 2, 8).  Per map the softmax at map resolution and the zoom of the probabilities to the image (a mirror
    map read with its columns reversed), then in float32 and in the order scale 0 plain, scale 0 mirror, scale 1 plain, ...: the
    sum, / M (not at M = 1), the clamp at eps.  want / select / ignore_below and the return value: as train_gt_unary_batch, which
    is the case of one size without flip.  Image g's results do not depend on the group.  Runs on torch's current stream; the
    workspace (the probability planes of every used slice) is a torch tensor."""
    names = _want_names(want, _TG_OUTPUTS)
    if torch.is_tensor(scores):
        raise ValueError("scores must be a list of (Gcap, C, h, w) tensors, one per size")
    return _train_gt_batch(scores, shapes, flip, eps, names, select, ignore_below)


def _train_gt_batch(scores, shapes, flip, eps, want, select, ignore_below):
    """train_gt_unary_batch (one map, no flip) / train_gt_ensemble_batch after their `want` (parsed: _want_names) and type checks:
    the shape checks, the outputs, the workspace and the one launch"""
    names, single = want
    scores = [_f32c(s, "scores[%d]" % k) for k, s in enumerate(scores)]
    if not scores:
        raise ValueError("no score maps")
    if scores[0].dim() != 4:
        raise ValueError("score maps must be (Gcap, C, h, w); got %s" % (tuple(scores[0].shape),))
    Gcap, C = scores[0].shape[0], scores[0].shape[1]
    for s in scores:
        if s.dim() != 4 or s.shape[0] != Gcap or s.shape[1] != C:
            raise ValueError("score maps must be (Gcap, C, h, w) with one Gcap and one C; got %s" % (tuple(s.shape),))
    shapes = [(int(H), int(W)) for H, W in shapes]
    K, G, per, dev = len(scores), len(shapes), 2 if flip else 1, scores[0].device
    if not 1 <= G * per <= Gcap:
        raise ValueError("%d output shapes for score maps of %d %s" % (G, Gcap, "slices, two per image" if flip else "images"))
    sel = nsel = None
    stride = 0
    if "labels" in names:
        if select is None:
            raise ValueError('want="labels" needs one selection list per image (select=...)')
        sel, nsel, stride = select_arrays(select, G, C)
    out = _want_outputs(names, shapes, C, dev)
    workspace = torch.empty(sum(G * per * C * s.shape[2] * s.shape[3] for s in scores), dtype=torch.float32, device=dev)
    check(_lib.lib().dsrg_train_gt_ensemble_batch(G, K, int(bool(flip)), int(C), (ctypes.c_void_p * K)(*[s.data_ptr() for s in scores]),
                                                  _i32s([s.shape[2] for s in scores]), _i32s([s.shape[3] for s in scores]),
                                                  _i32s([H for H, _ in shapes]), _i32s([W for _, W in shapes]), float(eps), sel, nsel,
                                                  int(stride), float(ignore_below or 0.0), _ptr(workspace), _ptrs(out.get("unary")),
                                                  _ptrs(out.get("probs")), _ptrs(out.get("labels")), _stream()))
    if single:
        return out[names[0]]
    return [tuple(out[n][g] for n in names) for g in range(G)]


def _preprocess_group(images, out_shapes, capacity, mean, out, per_image=1):
    """the shared front end of preprocess_ms_batch / preprocess_rect_batch / preprocess_rect_mirror_batch (per_image = 2 slots per
    image): checks, output tensors and the launch's host arrays -> (G, capacity, K, image pointers, H, W, mean, output pointers,
    outputs)"""
    images = list(images)
    G, K = len(images), len(out_shapes)
    if G < 1 or K < 1:
        raise ValueError("no images / no sizes")
    if any(h < 1 or w < 1 for h, w in out_shapes):
        raise ValueError("every output size must be at least 1, got %s" % (out_shapes,))
    for g, im in enumerate(images):
        if not (torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and im.dim() == 3
                and im.shape[2] == 3):
            raise ValueError("images[%d] must be a contiguous (H, W, 3) uint8 CUDA tensor" % g)
    cap = per_image * G if capacity is None else int(capacity)
    if cap < per_image * G:
        raise ValueError("capacity %d is below the %d slots of %d images" % (cap, per_image * G, G))
    if len(mean) != 3:
        raise ValueError("mean must hold 3 values")
    dev = images[0].device
    if out is None:
        out = [torch.empty((cap, 3, h, w), dtype=torch.float32, device=dev) for h, w in out_shapes]
    else:
        out = list(out)
        if len(out) != K:
            raise ValueError("out must hold one tensor per size")
        for k, (o, (h, w)) in enumerate(zip(out, out_shapes)):
            _f32c(o, "out[%d]" % k)
            if tuple(o.shape) != (cap, 3, h, w):
                raise ValueError("out[%d] must be %s, got %s" % (k, (cap, 3, h, w), tuple(o.shape)))
    return (G, cap, K, (ctypes.c_void_p * G)(*[im.data_ptr() for im in images]), (ctypes.c_int32 * G)(*[im.shape[0] for im in images]),
            (ctypes.c_int32 * G)(*[im.shape[1] for im in images]), (ctypes.c_float * 3)(*[float(m) for m in mean]),
            (ctypes.c_void_p * K)(*[o.data_ptr() for o in out]), out)


def preprocess_ms_batch(images, sizes, capacity=None, mean=MEAN_PIXEL, out=None):
    """inference.preprocess (test-ms.py:68-81) for a group of images at every size, in one launch (dsrg_preprocess_ms_batch).
    images: G <= 16 contiguous (H_g, W_g, 3) RGB uint8 CUDA tensors (sizes may differ); sizes: the K <= 8 network input sizes S_k;
    capacity >= G (default G): the batch size of the outputs, slots G.. are written as zeros.  Returns a list of K
    (capacity, 3, S_k, S_k) float32 tensors, BGR, mean-subtracted: the inputs of K batched forwards.  out: K existing contiguous
    float32 CUDA tensors of those shapes to write into (the static inputs of captured graphs, for one) and return.  Runs on
    torch's current stream."""
    sizes = [int(s) for s in sizes]
    G, cap, K, ims, Hs, Ws, mean3, optrs, out = _preprocess_group(images, [(S, S) for S in sizes], capacity, mean, out)
    check(_lib.lib().dsrg_preprocess_ms_batch(G, cap, K, ims, Hs, Ws, (ctypes.c_int32 * K)(*sizes), mean3, optrs, _stream()))
    return out


def _rect_targets(out_shapes):
    """the out_shapes of the rectangular preprocess wrappers -> ([(h_k, w_k)] as ints, the launch's height and width arrays)"""
    try:
        out_shapes = [(int(h), int(w)) for h, w in out_shapes]
    except TypeError:
        raise ValueError("out_shapes must hold (h, w) pairs")
    return out_shapes, _i32s([h for h, _ in out_shapes]), _i32s([w for _, w in out_shapes])


def preprocess_rect_batch(images, out_shapes, capacity=None, mean=MEAN_PIXEL, out=None):
    """preprocess_ms_batch with a target (h_k, w_k) per scale, in one launch (dsrg_preprocess_rect_batch): what
    inference.preprocess_relative (test-ms-f.py:100-112) makes of a group of same-sized images at every relative scale.  images: G
    <= 16 contiguous (H_g, W_g, 3) RGB uint8 CUDA tensors; out_shapes: the K <= 8 targets (h_k, w_k); capacity, mean, out as
    there.  Returns a list of K (capacity, 3, h_k, w_k) float32 tensors, BGR, mean-subtracted; with h_k = w_k they are
    preprocess_ms_batch's bit for bit.  Runs on torch's current stream."""
    out_shapes, hs, ws = _rect_targets(out_shapes)
    G, cap, K, ims, Hs, Ws, mean3, optrs, out = _preprocess_group(images, out_shapes, capacity, mean, out)
    check(_lib.lib().dsrg_preprocess_rect_batch(G, cap, K, ims, Hs, Ws, hs, ws, mean3, optrs, _stream()))
    return out


def preprocess_rect_mirror_batch(images, out_shapes, capacity=None, mean=MEAN_PIXEL, out=None):
    """preprocess_rect_batch for mirrored test-time augmentation, in one launch (dsrg_preprocess_rect_mirror_batch): image g fills
    the slots 2g (what preprocess_rect_batch writes for it, bit for bit) and 2g+1 (the same tensor with its last axis reversed:
    the mirrored network input).  images: G <= 8 contiguous (H_g, W_g, 3) RGB uint8 CUDA tensors; out_shapes: the K <= 8 targets
    (h_k, w_k), (S, S) pairs for the fixed sizes of test-ms.py; capacity >= 2G (default 2G): the batch size of the outputs, slots
    2G.. are written as zeros; mean, out as there.  Returns a list of K (capacity, 3, h_k, w_k) float32 tensors.  Runs on torch's
    current stream."""
    out_shapes, hs, ws = _rect_targets(out_shapes)
    G, cap, K, ims, Hs, Ws, mean3, optrs, out = _preprocess_group(images, out_shapes, capacity, mean, out, per_image=2)
    check(_lib.lib().dsrg_preprocess_rect_mirror_batch(G, cap, K, ims, Hs, Ws, hs, ws, mean3, optrs, _stream()))
    return out


def _i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _train_input_args(stage, nbytes, desc, keys, mean, shapes, out):
    """What the training-input wrappers share -> (head, mean3, outputs).  head: the leading arguments of every dsrg_train_*_input_batch
    entry — B, the staging pointer, its byte count and one int32 array per key of `keys`, each checked to hold one entry per image;
    mean3: the mean as float[3]; outputs: one float32 tensor of (B,) + shape per shape of `shapes`, made here or, with `out`,
    checked to be that."""
    if not (torch.is_tensor(stage) and stage.is_cuda and stage.dtype == torch.uint8 and stage.is_contiguous() and stage.dim() == 1):
        raise ValueError("stage must be a contiguous 1-d uint8 CUDA tensor")
    nbytes = stage.numel() if nbytes is None else int(nbytes)
    if not 0 <= nbytes <= stage.numel():
        raise ValueError("the staging buffer holds %d bytes, the batch states %d" % (stage.numel(), nbytes))
    B = len(desc["H"])
    if len(mean) != 3:
        raise ValueError("mean must hold 3 values")
    if any(len(desc[k]) != B for k in keys):
        raise ValueError("every descriptor list must hold one entry per image")
    outputs = []
    for k, shape in enumerate(shapes):
        shape, t = (B,) + shape, None if out is None else out[k]
        if t is None:
            t = torch.empty(shape, dtype=torch.float32, device=stage.device)
        else:
            _f32c(t, "out[%d]" % k)
            if tuple(t.shape) != shape:
                raise ValueError("out[%d] must be %s, got %s" % (k, shape, tuple(t.shape)))
        outputs.append(t)
    return (B, _ptr(stage), nbytes) + tuple(_i32s(desc[k]) for k in keys), (ctypes.c_float * 3)(*[float(m) for m in mean]), outputs


def train_s_input_batch(stage, desc, size=321, num_classes=21, map_size=(41, 41), mean=MEAN_PIXEL, out=None, nbytes=None):
    """The stage-1 training batch in one launch (dsrg_train_s_input_batch): Caffe's ImageData layer (train-s.prototxt:3-22) followed
    by AnnotationLayer (pylayers.py:346-387).  stage: the batch's raw bytes as a 1-d uint8 CUDA tensor (input.pack_train_s makes
    them on the host; one upload); desc: the dict of per-image lists input.layout_train_s returns — image_off, H, W, cue_off, ncues,
    label_off, nlabels (byte offsets and counts) — and mirror (one flag per image).  Returns (images (B,3,S,S), labels (B,1,1,C),
    cues (B,C,Hm,Wm)), float32: the arguments of DSRGTrainer.step.  out: three existing tensors of those shapes to write into.
    Runs on torch's current stream."""
    S, C, (Hm, Wm) = int(size), int(num_classes), (int(map_size[0]), int(map_size[1]))
    head, mean3, (images, labels, cues) = _train_input_args(
        stage, nbytes, desc, ("image_off", "H", "W", "cue_off", "ncues", "label_off", "nlabels", "mirror"), mean,
        ((3, S, S), (1, 1, C), (C, Hm, Wm)), out)
    check(_lib.lib().dsrg_train_s_input_batch(*head, S, C, Hm, Wm, mean3, _ptr(images), _ptr(cues), _ptr(labels), _stream()))
    return images, labels, cues


def train_s_cuemap_input_batch(stage, desc, size, num_classes, map_size, mean, ignore_label=255, bgr=True, out=None, nbytes=None):
    """The stage-1 training batch of a run fed by cue maps, in one launch (dsrg_train_s_cuemap_input_batch): AnnotationLayerCOCO
    (pylayers.py:432-512).  stage: the batch's raw bytes as a 1-d uint8 CUDA tensor (input.pack_train_s_cuemap); desc: the dict of
    per-image lists input.layout_train_s_cuemap returns — image_off, H, W, cue_off, mirror.  size: the (h, w) the images are zoomed
    to (an int: square), as preprocess_rect_batch zooms; map_size: the (Hm, Wm) of every cue map; a cue byte counts unless it is
    ignore_label or >= num_classes; bgr: output channel c is source byte 2 - c (the order of this project's other pipelines) or,
    False, byte c (the layer's own).  Returns (images (B,3,h,w), labels (B,1,1,C), cues (B,C,Hm,Wm)), float32, every element
    written: the arguments of DSRGTrainer.step.  out: three existing tensors of those shapes to write into.  The launch takes no
    scratch.  Runs on torch's current stream."""
    Sh, Sw = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    C, (Hm, Wm) = int(num_classes), (int(map_size[0]), int(map_size[1]))
    head, mean3, (images, labels, cues) = _train_input_args(stage, nbytes, desc, ("image_off", "H", "W", "cue_off", "mirror"), mean,
                                                            ((3, Sh, Sw), (1, 1, C), (C, Hm, Wm)), out)
    check(_lib.lib().dsrg_train_s_cuemap_input_batch(*head, Sh, Sw, C, Hm, Wm, mean3, int(ignore_label), int(bool(bgr)), _ptr(images),
                                                     _ptr(cues), _ptr(labels), _stream()))
    return images, labels, cues


def train_f_input_batch(stage, desc, crop_size, mean, scale=1.0, ignore_label=255, out=None, nbytes=None):
    """The stage-2 training batch in one launch (dsrg_train_f_input_batch): data.SimpleTransformer.preprocess (layer.py:169-236) for
    every image of the batch.  stage: the batch's raw bytes as a 1-d uint8 CUDA tensor (input.pack_train_f); desc: the dict of
    per-image lists input.layout_train_f returns — image_off, label_off, H, W — and the host's draws top, left, mirror.  Returns
    (data (B,3,ch,cw), label (B,1,ch,cw)), float32: the arguments of RetrainTrainer.step.  out: two existing tensors of those shapes
    to write into.  A desc that carries Hs and Ws (layout_train_f's `scaled`) goes to dsrg_train_f_input_scaled_batch: every image
    is rescaled to (Hs, Ws) inside the same launch — 8-bit bilinear for the image, nearest neighbour for the label — and top /
    left are offsets on the rescaled image.  Runs on torch's current stream."""
    ch, cw = int(crop_size[0]), int(crop_size[1])
    scaled = "Hs" in desc or "Ws" in desc
    keys = ("image_off", "label_off", "H", "W") + (("Hs", "Ws") if scaled else ()) + ("top", "left", "mirror")
    head, mean3, (data, label) = _train_input_args(stage, nbytes, desc, keys, mean, ((3, ch, cw), (1, ch, cw)), out)
    entry = _lib.lib().dsrg_train_f_input_scaled_batch if scaled else _lib.lib().dsrg_train_f_input_batch
    check(entry(*head, ch, cw, mean3, float(scale), float(ignore_label), _ptr(data), _ptr(label), _stream()))
    return data, label


def supervision_step(logits, images, labels, cues, th1=0.99, th2=0.85, scale_factor=12.0, maxiter=10,
                     ctx=None, want_blobs=False, prepared=False, want_total=False):
    """The five Python layers of train-s.prototxt:746-810, forward and backward, in one
    stream-ordered launch sequence (CRF computed once).

    Returns (losses[2] = {loss-Seed, loss-Constrain}, d(sum)/d logits, blobs or None); want_total: a fourth result, the 0-d float32
    losses[0] + losses[1], stored by the kernel that finishes the two losses (the bits of losses.sum())."""
    _f32c(logits, "logits"), _f32c(images, "images"), _f32c(labels, "labels"), _f32c(cues, "cues")
    B, C, H, W = logits.shape
    if images.dim() != 4 or images.shape[0] != B or images.shape[1] != 3:
        raise ValueError("images must be (B,3,Hi,Wi) with the batch size of logits")
    if labels.numel() != B * C or tuple(cues.shape) != (B, C, H, W):
        raise ValueError("labels must hold B*C values and cues must have the shape of logits")
    if not lds_path_supports(H, W):
        # maps beyond the LDS path: the same five layers, layer by layer, in the prototxt's order and with its gradient wiring
        # (seed-loss gradient + constrain gradient wrt p + CRFLayer.backward(constrain gradient wrt log q), then
        # SoftmaxLayer.backward)
        probs = softmax_forward(logits)
        refined, logq = _crf_refine_large(probs, images, scale_factor, maxiter, True)
        seeds = srg_grow(labels.reshape(B, -1).contiguous(), cues, refined, th1, th2)
        l_seed, g_seed = seed_loss(probs, seeds)
        l_con, g_p, g_q = constrain_loss(probs, logq)
        grad = softmax_backward(logits, g_seed + g_p + crf_layer_backward(refined, g_q))
        losses = torch.stack([l_seed.reshape(()), l_con.reshape(())]).float()
        blobs = dict(probs=probs, seeds=seeds, logq=logq, refined=refined) if want_blobs else None
        return (losses, grad, blobs, losses.sum()) if want_total else (losses, grad, blobs)
    ctx = ctx or get_context(B, C, H, W)
    out3 = torch.empty(3, dtype=torch.float32, device=logits.device)      # the two losses and their sum
    losses = out3[:2]
    grad = torch.empty_like(logits)
    blobs = None
    if want_blobs:
        blobs = dict(probs=torch.empty_like(logits), seeds=torch.empty_like(logits), logq=torch.empty_like(logits))
    prm = CrfParams.from_crf_args(maxiter, scale_factor)
    check(_lib.lib().dsrg_supervision_step_total(
        ctx._h, B, _ptr(logits), None if prepared else _ptr(images), images.shape[2], images.shape[3],
        _ptr(labels), _ptr(cues),
        float(th1), float(th2), ctypes.byref(prm), _ptr(losses), _ptr(out3[2]) if want_total else None, _ptr(grad),
        _ptr(blobs["probs"]) if blobs else None, _ptr(blobs["seeds"]) if blobs else None,
        _ptr(blobs["logq"]) if blobs else None, _stream()))
    return (losses, grad, blobs, out3[2]) if want_total else (losses, grad, blobs)


def im2col3x3_nhwc(x_nhwc, dilation):
    """(B,H,W,C) contiguous bf16/fp16 (C % 8 == 0) or float32 (C % 4 == 0) -> (B*H*W, 9*C) im2col matrix of a 3x3 'same'
    dilated convolution.  The kernel moves 16-byte channel groups, so a float32 pixel is passed as 2*C two-byte elements."""
    es = x_nhwc.element_size()
    if not (x_nhwc.is_cuda and x_nhwc.is_contiguous() and es in (2, 4)):
        raise ValueError("x must be a contiguous 2- or 4-byte CUDA tensor in NHWC order")
    B, H, W, C = x_nhwc.shape
    out = torch.empty((B * H * W, 9 * C), dtype=x_nhwc.dtype, device=x_nhwc.device)
    check(_lib.lib().dsrg_im2col3x3_nhwc16(_ptr(x_nhwc), _ptr(out), B, H, W, C * (es // 2), int(dilation), _stream()))
    return out


def col2im3x3_nhwc(cols, B, H, W, C, dilation):
    """(B*H*W, 9*C) contiguous bf16 -> (B,C,H,W) channels_last bf16: the adjoint of im2col3x3_nhwc"""
    if not (cols.is_cuda and cols.is_contiguous() and cols.dtype == torch.bfloat16 and cols.shape == (B * H * W, 9 * C)):
        raise ValueError("cols must be a contiguous (B*H*W, 9*C) bf16 CUDA tensor")
    out = torch.empty((B, C, H, W), dtype=cols.dtype, device=cols.device, memory_format=torch.channels_last)
    check(_lib.lib().dsrg_col2im3x3_nhwc_bf16(_ptr(cols), _ptr(out), B, H, W, C, int(dilation), _stream()))
    return out


_PARTIAL_BLOCKS = 512                  # rows of per-block partial column sums (relu_bwd_bias, bias_grad, maxpool3x3_bwd_relu)


def relu_bwd_bias(g, y, scale=1.0, gb_out=None):
    """ReLU backward fused with the bias-gradient reduction of the convolution before it.
    g, y: (B,C,H,W) bf16 channels_last (y = the ReLU output, or the output of ReLU + Dropout with scale = 1/(1-p)).
    Returns (scale * g * (y > 0), its sum over B,H,W as f32 (C,))."""
    B, C, H, W = y.shape
    cl = torch.channels_last
    if not (g.is_cuda and g.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=cl)):
        raise ValueError("relu_bwd_bias needs bf16 channels_last CUDA tensors")
    g = g.contiguous(memory_format=cl)
    gm = torch.empty_like(y)
    gb = _bias_grad_dest(gb_out, (C,), y.device)
    part = _reduction_scratch(y.device, 4 * _PARTIAL_BLOCKS * C, "rows").view(torch.float32)
    check(_lib.lib().dsrg_relu_bwd_bias_bf16(_ptr(g), _ptr(y), _ptr(gm), _ptr(gb), _ptr(part), _PARTIAL_BLOCKS,
                                             B * H * W, C, float(scale), _stream()))
    return gm, gb


def bias_grad(g):
    """(B,C,H,W) bf16 channels_last -> per-channel sums over B,H,W as f32 (C,); C <= 256, or a multiple of 8 up to 2048"""
    B, C, H, W = g.shape
    if not (g.is_cuda and g.dtype == torch.bfloat16):
        raise ValueError("bias_grad needs a bf16 CUDA tensor")
    g = g.contiguous(memory_format=torch.channels_last)
    gb = _bias_grad_dest(None, (C,), g.device)
    part = _reduction_scratch(g.device, 4 * _PARTIAL_BLOCKS * C, "rows").view(torch.float32)
    if C % 8 == 0:                                   # 16-byte lanes, no mask, nothing stored
        check(_lib.lib().dsrg_relu_bwd_bias_bf16(_ptr(g), None, None, _ptr(gb), _ptr(part), _PARTIAL_BLOCKS,
                                                 B * H * W, C, 1.0, _stream()))
    else:
        check(_lib.lib().dsrg_bias_grad_bf16(_ptr(g), _ptr(gb), _ptr(part), _PARTIAL_BLOCKS, B * H * W, C, _stream()))
    return gb


def avgpool3x3_s1(x):
    """3x3 / stride 1 / pad 1 average over padded windows of a (B,C,H,W) bf16 channels_last tensor (also its own backward)"""
    B, C, H, W = x.shape
    x = x.contiguous(memory_format=torch.channels_last)
    out = torch.empty_like(x)
    check(_lib.lib().dsrg_avgpool3x3_s1_bf16(_ptr(x), _ptr(out), B, H, W, C, _stream()))
    return out


def add_relu(a, b):
    """relu(a + b) of two bf16 CUDA tensors of one shape and memory layout in one pass (fp32 sum, one rounding) — the tail of a
    ResNet bottleneck"""
    if not (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape and a.numel() % 8 == 0):
        raise ValueError("add_relu needs two bf16 CUDA tensors of one shape, 8 | elements")
    if a.stride() != b.stride() or not (a.is_contiguous() or a.is_contiguous(memory_format=torch.channels_last)):
        a, b = a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last)
    y = torch.empty_like(a)
    check(_lib.lib().dsrg_add_relu_bf16(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream()))
    return y


def relu_mask(g, y, g2=None):
    """(g (+ g2)) where y > 0, else 0: the backward of add_relu (y its output); bf16 CUDA tensors of y's layout"""
    if not (y.is_cuda and y.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and g.shape == y.shape and y.numel() % 8 == 0):
        raise ValueError("relu_mask needs bf16 CUDA tensors of one shape, 8 | elements")
    if not (y.is_contiguous() or y.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("relu_mask: y must be dense")
    mf = torch.contiguous_format if y.is_contiguous() else torch.channels_last

    def dense(t):
        return t if t.stride() == y.stride() else t.contiguous(memory_format=mf)
    g = dense(g)
    g2 = dense(g2) if g2 is not None else None
    gm = torch.empty_like(y)
    check(_lib.lib().dsrg_relu_mask_bf16(_ptr(g), _ptr(g2) if g2 is not None else None, _ptr(y), _ptr(gm), y.numel(), _stream()))
    return gm


DIRECT_CONV_CHANNELS = (64, 128)


def conv3x3_direct(x, weight, bias=None, relu=False):
    """3x3 / stride 1 / pad 1 convolution with 64 or 128 channels on either side, or 3 -> 64: x (B,cin,H,W) bf16 channels_last, weight
    (cout,cin,3,3) bf16 (made channels_last here), bias (cout) f32 or None -> (B,cout,H,W) bf16 channels_last; fp32
    accumulation, bias and ReLU fused"""
    B, C, H, W = x.shape
    cl = torch.channels_last
    cout = weight.shape[0]
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and tuple(weight.shape) == (cout, C, 3, 3)
            and ((C in DIRECT_CONV_CHANNELS and cout in DIRECT_CONV_CHANNELS) or (C, cout) == (3, 64))):
        raise ValueError("conv3x3_direct needs a bf16 CUDA input and a (cout,cin,3,3) bf16 kernel with cin, cout in (64, 128) or 3 -> 64")
    x = x.contiguous(memory_format=cl)
    w = weight.contiguous(memory_format=cl)
    if bias is not None:
        bias = bias.float().contiguous()
    y = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=cl)
    check(_lib.lib().dsrg_conv3x3_direct_bf16(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, H, W, C, cout, int(bool(relu)), _stream()))
    return y


def conv3x3_direct_dgrad(g, weight_t, mask):
    """conv3x3_direct(g, weight_t) — weight_t the flipped, channel-swapped kernel, 64 / 128 channels either side — with the ReLU
    backward of the layer below in the store: mask (B,cout,H,W) bf16 channels_last, that layer's output -> (gx bf16 masked by
    mask > 0, the layer's bias gradient (cout) f32)"""
    B, C, H, W = g.shape
    cl = torch.channels_last
    cout = weight_t.shape[0]
    if not (g.is_cuda and g.dtype == torch.bfloat16 and weight_t.dtype == torch.bfloat16 and tuple(weight_t.shape) == (cout, C, 3, 3)
            and C in DIRECT_CONV_CHANNELS and cout in DIRECT_CONV_CHANNELS and mask.dtype == torch.bfloat16
            and tuple(mask.shape) == (B, cout, H, W) and mask.is_contiguous(memory_format=cl)):
        raise ValueError("conv3x3_direct_dgrad needs bf16 CUDA tensors, 64 / 128 channels, a channels_last mask of the output's shape")
    g = g.contiguous(memory_format=cl)
    w = weight_t.contiguous(memory_format=cl)
    L = _lib.lib()
    gx = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=g.device, memory_format=cl)
    gb = _bias_grad_dest(None, (cout,), g.device)
    ws = _reduction_scratch(g.device, L.dsrg_conv3x3_direct_dgrad_workspace(cout))
    check(L.dsrg_conv3x3_direct_dgrad_bf16(_ptr(g), _ptr(w), _ptr(mask), _ptr(gx), _ptr(gb), _ptr(ws), ws.numel(), B, H, W, C, cout,
                                           _stream()))
    return gx, gb


WGRAD_CONV_SHAPES = ((3, 64), (64, 64), (64, 128), (128, 128))      # (cin, cout)


# ---- the packed bf16 kernels of the float32 master parameters, kept from step to step — only for parameters an optimizer that
# maintains them has claimed (keep_weight_packs: trainer.CaffeSGD).  A convolution node packs the kernel the first time it sees
# such a parameter and leaves the buffers on it; the optimizer's update (sgd_pack_step) rewrites them in the pass that updates the
# parameter, so from the second step on a forward finds its packs ready and reads no float32 weight.  A record is good for exactly
# one value of the parameter: it holds the tensor's version counter, which in-place writes bump (load_state_dict, a broadcast)
# — then the node packs again, into the same buffers.  NOT every writer bumps it: torch's private fused optimizer ops
# (torch._fused_sgd_, which torch.optim.SGD(fused=True) calls) leave the counter alone, which is why nothing is kept for a
# parameter unless its optimizer says it plays along; unclaimed parameters are packed inside every forward as before.  Writes
# through `param.data` (whose version counter is its own) or by foreign kernels are equally invisible: code that does that to a
# claimed parameter calls forget_weight_packs afterwards.
#
# All of it sits on the parameter, as its one attribute `_dsrg_packs`: the claim and the packs live and die with the tensor, and
# nothing is keyed by an address.  The record says where the parameter lay when the packs were written; a parameter whose storage
# has moved since (net.to(memory_format=...), `p.data = ...` — both keep attributes and version counter) no longer matches it.
class _KeptPacks(object):
    """owner: weakref to the claiming optimizer; kind: "igemm" (pack_conv_weight_pair), "direct" (pack_direct_weight_pair),
    "cast" (cast_weight_kept: `fwd` is the parameter cast to bf16 as it lies) or None = nothing kept yet; at: (address, shape,
    strides) of the parameter the packs were written from; version: the version counter they belong to; fwd / dg: the buffers"""
    __slots__ = ("owner", "kind", "at", "version", "fwd", "dg")

    def __init__(self, owner):
        self.owner = _weakref.ref(owner)
        self.forget()

    def forget(self):
        self.kind = self.at = self.version = self.fwd = self.dg = None


def _lies(weight):
    return weight.data_ptr(), tuple(weight.shape), tuple(weight.stride())


def keep_weight_packs(params, owner):
    """an optimizer's declaration that every write it makes to these parameters either goes through sgd_pack_step or bumps their
    version counter: the convolution nodes may then keep the packed kernels between steps.  The claim lasts as long as `owner`
    (the optimizer object) does — a parameter handed to another optimizer afterwards is packed inside every forward again;
    owner=None withdraws it"""
    for p in params:                              # a new record: whatever an earlier owner left may have missed writes made since
        p._dsrg_packs = _KeptPacks(owner) if owner is not None else None


def forget_weight_packs(params):
    """drop the kept packed kernels of these parameters (after a write that neither sgd_pack_step made nor a version counter saw)"""
    for p in params:
        if getattr(p, "_dsrg_packs", None) is not None:
            p._dsrg_packs.forget()


def _packs_claimed(weight):
    r = getattr(weight, "_dsrg_packs", None)
    return r is not None and r.owner() is not None


def kept_packs(weight, kind=None):
    """the record (kind, version, fwd, dg) of what is kept for this parameter — whatever value it was packed from — if it
    describes the parameter as it lies now (and is of `kind`, where one is given), else None.  A record that does not — the owner
    is dead, the storage moved, another shape, another kind — loses its buffers here"""
    r = getattr(weight, "_dsrg_packs", None)
    if r is None or r.kind is None:
        return None
    if r.owner() is None or r.at != _lies(weight) or (kind is not None and r.kind != kind):
        r.forget()
        return None
    return r


def _packs_keep(weight, kind, fwd, dg):
    """the one writer of a claimed parameter's record"""
    r = weight._dsrg_packs
    r.kind, r.at, r.version, r.fwd, r.dg = kind, _lies(weight), weight._version, fwd, dg


# DSRG_CHECK_PACKS=N (debugging aid): every N-th time a forward takes kept packs for good, the parameter is packed again into
# scratch buffers and compared — a writer the version counter cannot see (`p.data.copy_`, an EMA through `.data`, a foreign
# kernel, torch's private fused optimizer ops) then fails loudly instead of training on kernels one update behind.  0 = off.
_CHECK_PACKS = int(os.environ.get("DSRG_CHECK_PACKS", "0") or 0)
_check_packs_calls = [0]


def _check_kept_packs(weight, fwd, dg, pack):
    """pack(fwd_buffer_or_None, dg_buffer_or_None) packs `weight` into the buffers given"""
    if _CHECK_PACKS <= 0:
        return
    _check_packs_calls[0] += 1
    if _check_packs_calls[0] % _CHECK_PACKS:
        return
    f2 = torch.empty_like(fwd) if fwd is not None else None
    d2 = torch.empty_like(dg) if dg is not None else None
    pack(f2, d2)
    if (f2 is not None and not torch.equal(f2, fwd)) or (d2 is not None and not torch.equal(d2, dg)):
        raise RuntimeError("DSRG_CHECK_PACKS: the kept bf16 kernels of a %s parameter no longer match its float32 value — it was "
                           "written behind the version counter's back (param.data, a foreign kernel, torch._fused_sgd_); call "
                           "dsrg_amd.ops.forget_weight_packs([param]) after such a write" % (tuple(weight.shape),))


def _kept_or_packed(weight, kind, want_fwd, want_dgrad, fwd_shape, dg_shape, mf, pack):
    """-> (fwd, dg), None where not wanted: the kept packs of `weight` if they hold its present value, else packed now —
    into the kept buffers where there are any, every form already kept along with the wanted ones — and kept.
    pack(fwd_buffer_or_None, dg_buffer_or_None) packs `weight` into the buffers given; they have fwd_shape / dg_shape, layout mf"""
    # inside a hipGraph capture the packing launches belong in the graph (a replay must see the weights of its own time)
    keep = _packs_claimed(weight) and weight.is_cuda and not torch.cuda.is_current_stream_capturing()
    r = kept_packs(weight, kind) if keep else None
    fwd, dg = (r.fwd, r.dg) if r is not None else (None, None)
    if r is not None and r.version == weight._version and (fwd is not None or not want_fwd) and (dg is not None or not want_dgrad):
        _check_kept_packs(weight, fwd if want_fwd else None, dg if want_dgrad else None, pack)
    else:
        if fwd is None and want_fwd:
            fwd = torch.empty(fwd_shape, dtype=torch.bfloat16, device=weight.device, memory_format=mf)
        if dg is None and want_dgrad:
            dg = torch.empty(dg_shape, dtype=torch.bfloat16, device=weight.device, memory_format=mf)
        pack(fwd, dg)
        if keep:
            _packs_keep(weight, kind, fwd, dg)
    return (fwd if want_fwd else None), (dg if want_dgrad else None)


def sgd_pack_step(params, grads, bufs, lrs, wds, momentum):
    """Caffe's SGD update B <- momentum B + (g + wd W); W <- W - lr B of float32 CUDA parameters in one launch per sixteen
    tensors (dsrg_sgd_pack_cast_f32), rewriting the packed bf16 kernels the convolution nodes keep for them (and conv1_1's plain
    bf16 copy, cast_weight_kept) in the same pass.
    params / grads / bufs: dense tensors of one memory layout each; lrs / wds: per-tensor rates."""
    import numpy as np
    n = len(params)
    if n == 0:
        return
    ptr = lambda ts: np.array([0 if t is None else t.data_ptr() for t in ts], dtype=np.uint64)
    fwd, dg, cast, shape, entries = [None] * n, [None] * n, [None] * n, np.zeros((n, 4), dtype=np.int32), []
    for i, p in enumerate(params):
        e = kept_packs(p)
        if e is None:
            continue
        if e.kind == "cast":                                          # conv1_1: a bf16 copy in the parameter's own order
            cast[i] = e.fwd
        else:                                                         # the library's `plain` flag: 1 = the direct route's layout
            fwd[i], dg[i] = e.fwd, e.dg
            shape[i] = (p.shape[0], p.shape[1], p.shape[2] * p.shape[3], int(e.kind == "direct"))
        entries.append((e, p))
    pp, gp, bp, fp, dp, cp = ptr(params), ptr(grads), ptr(bufs), ptr(fwd), ptr(dg), ptr(cast)
    numel = np.array([p.numel() for p in params], dtype=np.int64)
    lr, wd = np.asarray(lrs, dtype=np.float32), np.asarray(wds, dtype=np.float32)
    a = lambda x: x.ctypes.data
    check(_lib.lib().dsrg_sgd_pack_cast_f32(n, a(pp), a(gp), a(bp), a(fp), a(dp), a(cp), a(shape), a(numel), a(lr), a(wd),
                                            float(momentum), _stream()))
    torch.autograd.graph.increment_version(list(params))              # an in-place write autograd has not seen
    for e, p in entries:
        e.version = p._version


def sgd_pack_eligible(p, g, b):
    """can dsrg_sgd_pack_f32 update this parameter: float32 CUDA tensors of one dense layout"""
    return p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and b.dtype == torch.float32 and g.is_cuda and \
        g.shape == p.shape and all(n == 1 or (sg == sp and sb == sp) for n, sp, sg, sb in zip(p.shape, p.stride(), g.stride(), b.stride())) and \
        (p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))) and \
        ((p.data_ptr() | b.data_ptr()) % 16 == 0 or kept_packs(p) is None)


def cast_weight_kept(weight):
    """weight.to(bfloat16) of a float32 parameter whose convolution reads its kernel unpacked (conv1_1: conv3x3_direct with three
    input channels), kept from step to step like the packed kernels: taken fresh the first time, after forget_weight_packs and
    whenever the version counter says the kept copy is stale; otherwise the copy sgd_pack_step wrote with the update"""
    w = weight.detach()
    dense = w.is_contiguous() or (w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last))
    if not (w.dtype == torch.float32 and dense):
        return w.to(torch.bfloat16)
    mf = torch.contiguous_format if w.is_contiguous() else torch.channels_last   # (the parameter's own order: sgd_pack_step writes it so)
    return _kept_or_packed(weight, "cast", True, False, w.shape, None, mf, lambda f, d: f.copy_(w))[0]


def pack_direct_weight_pair(weight, want_dgrad=True):
    """the bf16 kernels of conv3x3_direct from a float32 channels_last (cout, cin, 3, 3) parameter with 64 / 128 channels either
    side, one pass: (weight cast, weight flipped with its channel axes swapped — the data gradient's kernel — or None)"""
    cout, cin = weight.shape[0], weight.shape[1]
    cl = torch.channels_last
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous(memory_format=cl) and tuple(weight.shape[2:]) == (3, 3)
            and cin in DIRECT_CONV_CHANNELS and cout in DIRECT_CONV_CHANNELS):
        raise ValueError("pack_direct_weight_pair needs a float32 channels_last (cout,cin,3,3) CUDA parameter with 64 / 128 channels")
    pack = lambda f, d: check(_lib.lib().dsrg_pack_conv_weight_direct_f32(_ptr(weight.detach()), _ptr(f), _ptr(d), cout, cin, _stream()))
    return _kept_or_packed(weight, "direct", True, want_dgrad, (cout, cin, 3, 3), (cin, cout, 3, 3), cl, pack)


def conv3x3_wgrad(x, g, out_dtype=torch.bfloat16, out=None):
    """weight gradient of the 3x3 / stride 1 / pad 1 convolution y = conv(x, w): x (B,cin,H,W) and g = dL/dy (B,cout,H,W) bf16
    channels_last, (cin, cout) in WGRAD_CONV_SHAPES -> (cout,cin,3,3) bf16 (or float32: out_dtype) channels_last; fp32
    accumulation, deterministic"""
    B, cin, H, W = x.shape
    cout = g.shape[1]
    cl = torch.channels_last
    if not (x.is_cuda and x.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and tuple(g.shape) == (B, cout, H, W)
            and (cin, cout) in WGRAD_CONV_SHAPES):
        raise ValueError("conv3x3_wgrad needs bf16 CUDA tensors with (cin, cout) in %s" % (WGRAD_CONV_SHAPES,))
    x = x.contiguous(memory_format=cl)
    g = g.contiguous(memory_format=cl)
    ws = _stream_scratch("wgrad3x3", x.device, _lib.lib().dsrg_conv3x3_wgrad_workspace(B, H, W, cin, cout))
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("conv3x3_wgrad: bf16 or float32 output")
    gw = _dest(out, (cout, cin, 3, 3), out_dtype, x.device, True)
    fn = _lib.lib().dsrg_conv3x3_wgrad_f32 if out_dtype == torch.float32 else _lib.lib().dsrg_conv3x3_wgrad_bf16
    check(fn(_ptr(x), _ptr(g), _ptr(gw), _ptr(ws), ws.numel(), B, H, W, cin, cout, _stream()))
    return gw


def conv_igemm_supported(cin, cout, k):
    """the channel counts / kernel sizes the implicit-GEMM convolution serves (cin % 64 == 0, cout % 256 == 0, k in (1, 3))"""
    return bool(_lib.lib().dsrg_conv_igemm_supported(int(cin), int(cout), int(k)))


def set_igemm_variant(v):
    """tests / tools: the launch form of the implicit-GEMM kernels: 1 = two LDS stages of 64, 3 = 1 +
    staggered DMA issue + stream-K where it wins (the default), 4 = stream-K wherever legal, 2 / 5 = retired experiments (a ring of four
    stages of 32, an early barrier): they run the default, 6 = round 4's launches
    (every K-step multiplied, flat tile maps), 7 = 3 with the weight gradient skipping dead steps of the flat pixel order instead of
    summing over each tap's live pixels; -1 = the default.  Same results (6 / 7 / 3: forward bit-identical;
    weight gradient bit-identical between 6 and 7, equal up to fp32 reassociation for 3)"""
    _lib.lib().dsrg_debug_set_igemm_variant(int(v))


def pack_conv_weight(weight, for_dgrad=False, dtype=torch.bfloat16):
    """(cout, cin, k, k) kernel (any float dtype: the fp32 master weights are cast in the same copy) -> the layout
    dsrg_conv_igemm_bf16 reads: (cout, cin / 64, k*k, 64), w_packed[o][cc][tap][c] = w[o][cc*64 + c][tap].  for_dgrad: the kernel
    of the data gradient instead — flipped, channel axes swapped: (cin, cout / 64, k*k, 64)."""
    k = weight.shape[2]
    if for_dgrad:
        weight = weight.flip(2, 3).transpose(0, 1) if k > 1 else weight.transpose(0, 1)
    o, c = weight.shape[0], weight.shape[1]
    out = torch.empty((o, c // 64, k * k, 64), dtype=dtype, device=weight.device)
    if weight.is_contiguous(memory_format=torch.channels_last) and not weight.is_contiguous():
        # the net's parameters are channels_last: memory [o][tap][c] -> [o][c / 64][tap][64] is a strided view of it
        out.copy_(weight.permute(0, 2, 3, 1).reshape(o, k * k, c // 64, 64).permute(0, 2, 1, 3))
    else:
        out.copy_(weight.reshape(o, c // 64, 64, k * k).permute(0, 1, 3, 2))  # cast + permute in one pass
    return out


def pack_conv_weight_pair(weight, want_fwd=True, want_dgrad=True, scale=None):
    """both packed forms of a float32 channels_last (cout, cin, k, k) parameter in one pass (cast included) ->
    (pack_conv_weight(weight), pack_conv_weight(weight, for_dgrad=True)); an entry is None when not wanted.  Other dtypes /
    layouts take the torch copies of pack_conv_weight.  scale (cout) f32: weight[o] * scale[o] is what is packed (the same pass; fresh
    buffers every call — the kept packs of a parameter, which the fused optimizer step rewrites, are those of the bare weight)."""
    cout, cin, k, _ = weight.shape
    if scale is not None:
        if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous(memory_format=torch.channels_last)
                and cout % 64 == 0 and cin % 64 == 0 and k in (1, 3)):
            return pack_conv_weight_pair((weight.detach() * scale.view(-1, 1, 1, 1)).contiguous(memory_format=torch.channels_last), want_fwd, want_dgrad)
        fwd = torch.empty((cout, cin // 64, k * k, 64), dtype=torch.bfloat16, device=weight.device) if want_fwd else None
        dg = torch.empty((cin, cout // 64, k * k, 64), dtype=torch.bfloat16, device=weight.device) if want_dgrad else None
        check(_lib.lib().dsrg_pack_conv_weight_scaled_f32(_ptr(weight.detach()), _ptr(_f32c(scale, "scale")), _ptr(fwd), _ptr(dg), cout, cin, k,
                                                          _stream()))
        return fwd, dg
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous(memory_format=torch.channels_last)
            and cout % 64 == 0 and cin % 64 == 0 and k in (1, 3)):
        return (pack_conv_weight(weight) if want_fwd else None, pack_conv_weight(weight, for_dgrad=True) if want_dgrad else None)
    pack = lambda f, d: check(_lib.lib().dsrg_pack_conv_weight_f32(_ptr(weight.detach()), _ptr(f), _ptr(d), cout, cin, k, _stream()))
    return _kept_or_packed(weight, "igemm", want_fwd, want_dgrad, (cout, cin // 64, k * k, 64), (cin, cout // 64, k * k, 64),
                           torch.contiguous_format, pack)


def split3_bf16(t, dim):
    """a float32 tensor as three bf16 planes concatenated along `dim`: t = p0 + p1 + p2 up to 2^-24 relative (each plane the bf16
    rounding of what the planes before leave)"""
    p0 = t.to(torch.bfloat16)
    r1 = t - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    return torch.cat([p0, p1, p2], dim=dim)


def conv_igemm_split(x, weight, bias, dilation, relu):
    """layer-level prototype: a float32 'same' convolution (3x3 or 1x1, stride 1) on the bf16 MFMA with six bf16 products per
    multiply-add (dsrg_conv_igemm_split_f32): x (B,cin,H,W) float32, weight (cout,cin,k,k) float32, bias (cout) float32 or None ->
    (B,cout,H,W) float32 channels_last.  The operand splits are torch ops here (a production path would have the producing
    epilogue write the planes)."""
    B, cin, H, W = x.shape
    cout, k = weight.shape[0], weight.shape[2]
    x3 = split3_bf16(x.permute(0, 2, 3, 1).contiguous().float(), 3)                     # (B,H,W,3 cin)
    w0, w1, w2 = [pack_conv_weight(p) for p in split3_bf16(weight.float(), 0).split(cout, 0)]
    wv = torch.cat([w0, w1, w0, w2, w0, w1], dim=1).contiguous()                      # (cout, 6 cin / 64, k k, 64)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    b = bias.float().contiguous() if bias is not None else None
    check(_lib.lib().dsrg_conv_igemm_split_f32(_ptr(x3), _ptr(wv), _ptr(b), _ptr(y), int(dilation), B, H, W, cin, cout, k, int(bool(relu)),
                                               _stream()))
    return y


def _is_bf16(t, shape, channels_last=False):
    """a bf16 CUDA tensor of this shape (channels_last: and in that layout, not merely convertible to it)"""
    return (t.is_cuda and t.dtype == torch.bfloat16 and tuple(t.shape) == tuple(shape)
            and (not channels_last or t.is_contiguous(memory_format=torch.channels_last)))


def _is_packed(p, rows, chunk_channels, ksize):
    """a kernel as pack_conv_weight lays it out: (rows, chunk_channels / 64, ksize * ksize, 64) bf16, contiguous"""
    return p.dtype == torch.bfloat16 and tuple(p.shape) == (rows, chunk_channels // 64, ksize * ksize, 64) and p.is_contiguous()


def conv_igemm(xs, packed, biases, dilations, ksize, relu, dropout_p=0.0, seed=0, stream_k=True):
    """1 .. 4 convolutions of one geometry in one launch (the four ASPP branches): xs[g] (B,cin,H,W) bf16 channels_last,
    packed[g] = pack_conv_weight(w_g), biases[g] (cout) f32 or None -> list of (B,cout,H,W) bf16 channels_last; fp32
    accumulation, bias, ReLU and (dropout_p > 0, multiples of 1/256) the Dropout behind it fused — the mask is a function of
    (seed, branch, position) — no im2col matrix.  stream_k: lend the launch a per-stream scratch so that it may deal its K-steps
    out evenly over the CUs when whole tiles would leave part of the chip idle (same results up to fp32 summation order)"""
    n = len(xs)
    B, cin, H, W = xs[0].shape
    cout = packed[0].shape[0]
    cl = torch.channels_last
    if not (1 <= n <= 4 and len(packed) == n and len(dilations) == n):
        raise ValueError("conv_igemm: 1..4 groups")
    if not all(_is_bf16(x, (B, cin, H, W)) and _is_packed(p, cout, cin, ksize) for x, p in zip(xs, packed)):
        raise ValueError("conv_igemm needs bf16 CUDA inputs of one shape and kernels packed by pack_conv_weight")
    xs = [x.contiguous(memory_format=cl) for x in xs]
    bs = [None if b is None else _f32c(b, "bias") for b in (biases or [None] * n)]
    ys = [torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=xs[0].device, memory_format=cl) for _ in range(n)]
    ws = _igemm_sk_workspace(xs[0].device) if stream_k else None
    check(_lib.lib().dsrg_conv_igemm_bf16(_ptrs(xs), _ptrs(packed), _ptrs(bs), _ptrs(ys), _i32s(dilations), n, B, H, W, cin, cout, ksize,
                                          int(bool(relu)), float(dropout_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ws),
                                          ws.numel() if ws is not None else 0, _stream()))
    return ys


def conv_igemm_residual(x, packed, bias, res, mask, dilation, ksize, relu):
    """one convolution with a residual in its store (dsrg_conv_igemm_residual_bf16): x (B,cin,H,W) bf16 channels_last, packed =
    pack_conv_weight(w), bias (cout) f32 or None, res (B,cout,H,W) bf16 channels_last, mask the same or None ->
    post(bf16(conv + bias) + res), post = ReLU (relu) and / or zero where mask <= 0.  Forward of a residual block's last
    convolution (res = the shortcut); data gradient of its first (res = the shortcut's gradient, mask = the block input)."""
    B, cin, H, W = x.shape
    cout = packed.shape[0]
    cl = torch.channels_last
    if not (_is_bf16(x, x.shape) and _is_packed(packed, cout, cin, ksize) and _is_bf16(res, (B, cout, H, W), True)
            and (mask is None or _is_bf16(mask, (B, cout, H, W), True))):
        raise ValueError("conv_igemm_residual needs bf16 channels_last tensors of matching shapes and a kernel packed by pack_conv_weight")
    x = x.contiguous(memory_format=cl)
    b = None if bias is None else _f32c(bias, "bias")
    y = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=cl)
    check(_lib.lib().dsrg_conv_igemm_residual_bf16(_ptr(x), _ptr(packed), _ptr(b), _ptr(res), _ptr(mask), _ptr(y), int(dilation), B, H, W,
                                                   cin, cout, ksize, int(bool(relu)), _stream()))
    return y


def aspp_shift_sum(y, offsets, outputs, bias=None):
    """the gather half of an ASPP head run as one 1x1 convolution (dsrg_aspp_shift_sum_f32): y (B,CT,H,W) bf16 channels_last = the
    1x1 product of the feature map with all (branch, tap) kernels stacked (pair j's outputs at channels j * outputs ..), offsets a list
    of (dy, dx) per pair -> (B,outputs,H,W) float32 (channels_last strides): out[.,o,y,x] = bias[o] + sum_j y[., j outputs + o, y + dy_j,
    x + dx_j], zero outside the map"""
    B, CT, H, W = y.shape
    J = len(offsets)
    if not (y.is_cuda and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last) and 1 <= J <= 36 and J * outputs <= CT):
        raise ValueError("aspp_shift_sum needs a bf16 channels_last (B,CT,H,W) tensor with CT >= pairs * outputs, at most 36 pairs")
    out = torch.empty((B, H, W, outputs), dtype=torch.float32, device=y.device)
    off = (ctypes.c_int * (2 * J))(*[int(v) for pair in offsets for v in pair])
    b = None if bias is None else _f32c(bias, "bias")
    check(_lib.lib().dsrg_aspp_shift_sum_f32(_ptr(y), _ptr(b), _ptr(out), off, J, int(outputs), CT, B, H, W, _stream()))
    return out.permute(0, 3, 1, 2)


def aspp_shift_gather(g, offsets, channels):
    """the backward of aspp_shift_sum (dsrg_aspp_shift_gather_bf16): g (B,outputs,H,W) float32 -> the gradient of y, (B,channels,H,W) bf16
    channels_last: gp[., j outputs + o, y, x] = bf16(g[., o, y - dy_j, x - dx_j]), zero outside the map and in the channels past J outputs"""
    B, O, H, W = g.shape
    J = len(offsets)
    if not (g.is_cuda and 1 <= J <= 36 and J * O <= channels):
        raise ValueError("aspp_shift_gather: at most 36 pairs, channels >= pairs * outputs")
    gn = g.float().permute(0, 2, 3, 1).contiguous()                                    # (B,H,W,O): a view if g has channels_last strides
    gp = torch.empty((B, channels, H, W), dtype=torch.bfloat16, device=g.device, memory_format=torch.channels_last)
    off = (ctypes.c_int * (2 * J))(*[int(v) for pair in offsets for v in pair])
    check(_lib.lib().dsrg_aspp_shift_gather_bf16(_ptr(gn), _ptr(gp), off, J, O, int(channels), B, H, W, _stream()))
    return gp


def conv_igemm_dgrad(gs, packed_t, masks, dilations, ksize, mask_scale=1.0, bias_grad=True, gb_outs=None):
    """the data gradient of 1 .. 4 convolutions whose inputs were ReLU (+ Dropout) outputs, with that layer's backward folded
    in: gs[g] (B,cout_fwd,H,W) bf16 channels_last, packed_t[g] the flipped + transposed packing, masks[g] (B,cin_fwd,H,W) bf16
    the outputs of the layer below -> (list of (B,cin_fwd,H,W) bf16 = conv_T(g) * mask_scale where mask > 0, list of (cin_fwd)
    f32 bias gradients of the layer below or None)"""
    n = len(gs)
    B, cin, H, W = gs[0].shape
    cout = packed_t[0].shape[0]
    cl = torch.channels_last
    if not (1 <= n <= 4 and len(packed_t) == n and len(dilations) == n and len(masks) == n):
        raise ValueError("conv_igemm_dgrad: 1..4 groups")
    if not all(_is_bf16(g, (B, cin, H, W)) and _is_packed(p, cout, cin, ksize) and _is_bf16(m, (B, cout, H, W), True)
               for g, p, m in zip(gs, packed_t, masks)):
        raise ValueError("conv_igemm_dgrad needs bf16 channels_last gradients / masks of one shape and packed kernels")
    gs = [g.contiguous(memory_format=cl) for g in gs]
    outs = [torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=gs[0].device, memory_format=cl) for _ in range(n)]
    L = _lib.lib()
    gb = ws = None
    if bias_grad:
        gb = [_bias_grad_dest(gb_outs[i] if gb_outs is not None else None, (cout,), gs[0].device) for i in range(n)]
        ws = _reduction_scratch(gs[0].device, L.dsrg_conv_igemm_dgrad_workspace(n, B, H, W, cout))
    check(L.dsrg_conv_igemm_dgrad_bf16(_ptrs(gs), _ptrs(packed_t), _ptrs(masks), _ptrs(outs), _ptrs(gb), _i32s(dilations), n, B, H, W, cin,
                                       cout, ksize, float(mask_scale), _ptr(ws), ws.numel() if ws is not None else 0, _stream()))
    return outs, gb


def _conv_igemm_backward_args(name, g, packed_d, x, ksize, gw_out, **like_x):
    """what conv_igemm_backward and conv_igemm_backward_residual share: the checks (like_x: named tensors of x's shape and layout, or
    None), the weight gradient's scratch and the two results -> (library, g channels_last, scratch, gx, gw, (B, H, W, cin, cout, ksize))"""
    B, cout, H, W = g.shape
    cin = x.shape[1]
    cl = torch.channels_last
    if not (_is_bf16(g, g.shape) and _is_bf16(x, (B, cin, H, W), True) and _is_packed(packed_d, cin, cout, ksize)
            and all(t is None or _is_bf16(t, (B, cin, H, W), True) for t in like_x.values())):
        raise ValueError("%s needs bf16 channels_last g / x (/ %s) of one geometry and the data-gradient packing" % (name, " / ".join(like_x)))
    g = g.contiguous(memory_format=cl)
    L = _lib.lib()
    need = L.dsrg_conv_igemm_wgrad_workspace(1, B, H, W, cin, cout, ksize)
    if need == 0:
        raise ValueError("%s: 256 | cin (or cin = 128 with a 3x3 kernel), 256 | cout required (got %d, %d)" % (name, cin, cout))
    ws = _stream_scratch("igemm_wgrad", g.device, need)              # shared with conv_igemm_wgrad
    gx = torch.empty((B, cin, H, W), dtype=torch.bfloat16, device=g.device, memory_format=cl)
    gw = _dest(gw_out, (cout, cin, ksize, ksize), torch.float32, g.device, True)
    return L, g, ws, gx, gw, (B, H, W, cin, cout, ksize)


def conv_igemm_backward(g, packed_d, x, dilation, mask=None, mask_scale=1.0, ksize=3, gw_out=None, gb_out=None):
    """the whole backward of one 3x3 convolution (forward geometry cin -> cout) in one launch (dsrg_conv_igemm_backward_bf16): g
    (B,cout,H,W) and x (B,cin,H,W) bf16 channels_last, packed_d = pack_conv_weight(w, for_dgrad=True); mask: the layer's input when
    it is the sole-consumer ReLU output of the layer below (then that layer's ReLU / Dropout backward and bias gradient ride in
    the data gradient, as conv_igemm_dgrad) -> (gx (B,cin,H,W) bf16 channels_last, gw (cout,cin,k,k) float32 channels_last, bias
    gradient of the layer below (cin) f32 or None).  gx and the bias gradient equal conv_igemm(_dgrad)'s bit for bit, gw equals
    conv_igemm_wgrad's up to fp32 reassociation (another pixel split)."""
    L, g, ws, gx, gw, geom = _conv_igemm_backward_args("conv_igemm_backward", g, packed_d, x, ksize, gw_out, mask=mask)
    B, H, W, cin = geom[:4]
    gb = cws = None
    if mask is not None:
        gb = _bias_grad_dest(gb_out, (cin,), g.device)
        cws = _reduction_scratch(g.device, L.dsrg_conv_igemm_dgrad_workspace(1, B, H, W, cin))
    check(L.dsrg_conv_igemm_backward_bf16(_ptr(g), _ptr(packed_d), _ptr(x), _ptr(mask), _ptr(gx), _ptr(gw), int(dilation), _ptr(gb),
                                          float(mask_scale), _ptr(cws), cws.numel() if cws is not None else 0, _ptr(ws), ws.numel(),
                                          *geom, _stream()))
    return gx, gw, gb


def conv_igemm_backward_residual(g, packed_d, x, dilation, ksize, mask=None, res=None, gw_scale=None, gw_out=None):
    """conv_igemm_backward (3x3 or 1x1) for a convolution inside a residual block (dsrg_conv_igemm_backward_residual_bf16): res
    (B,cin,H,W) bf16 channels_last or None is added to the bf16-rounded data gradient before the mask (the gradient along the
    block's shortcut); gw_scale (cout) f32 or None multiplies the weight gradient per output channel (the constant scale the
    forward's kernel was packed with); no bias gradient -> (gx, gw)"""
    L, g, ws, gx, gw, geom = _conv_igemm_backward_args("conv_igemm_backward_residual", g, packed_d, x, ksize, gw_out, mask=mask, res=res)
    sc = None if gw_scale is None else _f32c(gw_scale, "gw_scale")
    check(L.dsrg_conv_igemm_backward_residual_bf16(_ptr(g), _ptr(packed_d), _ptr(x), _ptr(mask), _ptr(res), _ptr(gx), _ptr(gw), _ptr(sc),
                                                   int(dilation), _ptr(ws), ws.numel(), *geom, _stream()))
    return gx, gw


def conv_igemm_backward_groups(gs, packed_d, xs, dilations, ksize, masks=None, mask_scale=1.0, gw_outs=None, gb_outs=None, gx_outs=None,
                               force_ksplit=0, force_order=0):
    """conv_igemm_backward for 1 .. 4 convolutions of one geometry (the four ASPP branches; dsrg_conv_igemm_backward_groups_bf16):
    gs[i] (B,cout,H,W) and xs[i] (B,cin,H,W) bf16 channels_last, packed_d[i] = pack_conv_weight(w_i, for_dgrad=True), masks: None or
    the layers' inputs where they are sole-consumer ReLU outputs (then the ReLU / Dropout backward and bias gradients of the layers
    below ride in the data gradients) -> (list of gx, list of gw (cout,cin,k,k) float32 channels_last, list of bias gradients or
    None).  One grid for both gradients where the planner takes it (conv_igemm_backward_groups_plan), else two launches: the same
    bits.  gx and the bias gradients equal conv_igemm(_dgrad)'s bit for bit; gw equals conv_igemm_wgrad's bit for bit wherever the
    pixel split is that launch's (a dilated 3x3 launch: always; a uniform split is chosen for the merged grid, force_ksplit > 0
    sets it) and else up to fp32 reassociation.  force_order
    1 / 2 (tests): a merged grid takes the data / weight gradient's blocks first."""
    n = len(gs)
    B, cout, H, W = gs[0].shape
    cin = xs[0].shape[1]
    cl = torch.channels_last
    if not (1 <= n <= 4 and len(packed_d) == n and len(xs) == n and len(dilations) == n and (masks is None or len(masks) == n)):
        raise ValueError("conv_igemm_backward_groups: 1..4 groups")
    if not all(_is_bf16(gs[i], (B, cout, H, W)) and _is_bf16(xs[i], (B, cin, H, W), True) and _is_packed(packed_d[i], cin, cout, ksize)
               and (masks is None or _is_bf16(masks[i], (B, cin, H, W), True)) for i in range(n)):
        raise ValueError("conv_igemm_backward_groups needs bf16 channels_last g / x (/ mask) of one geometry and the data-gradient packing")
    gs = [g.contiguous(memory_format=cl) for g in gs]
    dev = gs[0].device
    L = _lib.lib()
    need = L.dsrg_conv_igemm_wgrad_workspace(n, B, H, W, cin, cout, ksize)
    if need == 0 or not conv_igemm_supported(cout, cin, ksize):
        raise ValueError("conv_igemm_backward_groups: 64 | cout, 128 | cin, k in (1, 3) required (got %d, %d, %d)" % (cout, cin, ksize))
    ws = _stream_scratch("igemm_wgrad", dev, need)                   # shared with conv_igemm_wgrad
    gxs = [_dest(gx_outs[i] if gx_outs is not None else None, (B, cin, H, W), torch.bfloat16, dev, True) for i in range(n)]
    gws = [_dest(gw_outs[i] if gw_outs is not None else None, (cout, cin, ksize, ksize), torch.float32, dev, True) for i in range(n)]
    gbs = cws = None
    if masks is not None:
        gbs = [_bias_grad_dest(gb_outs[i] if gb_outs is not None else None, (cin,), dev) for i in range(n)]
        cws = _reduction_scratch(dev, L.dsrg_conv_igemm_dgrad_workspace(n, B, H, W, cin))
    check(L.dsrg_conv_igemm_backward_groups_bf16(_ptrs(gs), _ptrs(packed_d), _ptrs(xs), _ptrs(masks), _ptrs(gxs), _ptrs(gws), _i32s(dilations), n,
                                                 _ptrs(gbs), float(mask_scale), _ptr(cws), cws.numel() if cws is not None else 0, _ptr(ws),
                                                 ws.numel(), B, H, W, cin, cout, ksize, int(force_ksplit), int(force_order), _stream()))
    return gxs, gws, gbs


def conv_igemm_backward_groups_plan(n, B, H, W, cin, cout, ksize, dilations, with_mask=False, force_ksplit=0, force_order=0):
    """what conv_igemm_backward_groups does for this geometry under the current variant: a dict with merged (one grid or two launches),
    w_first (the weight gradient's workgroups take the first block ids), ksplit (its uniform pixel split; 0: its work list), nd / nw
    (blocks of the two halves), merged_us / separate_us (the dispatch model's prices).  Host only: nothing is launched"""
    out = (ctypes.c_int * 5)()
    us = (ctypes.c_double * 2)()
    check(_lib.lib().dsrg_conv_igemm_backward_groups_plan(int(n), int(B), int(H), int(W), int(cin), int(cout), int(ksize),
                                                           (ctypes.c_int * n)(*[int(d) for d in dilations]), int(bool(with_mask)),
                                                           int(force_ksplit), int(force_order), out, us))
    return {"merged": bool(out[0]), "w_first": bool(out[1]), "ksplit": out[2], "nd": out[3], "nw": out[4],
            "merged_us": us[0], "separate_us": us[1]}


def _igemm_sk_workspace(device):
    """the stream-K scratch of (device, current stream): one accumulator tile per CU + flags — a fixed size, so never replaced"""
    return _stream_scratch("igemm_stream_k", device, _lib.lib().dsrg_conv_igemm_workspace())


def conv_igemm_stream_k_status(device=None):
    """tests: 0, or 1 if a workgroup of the last stream-K launch on the current stream gave up waiting for a partial tile"""
    device = device or torch.device("cuda", torch.cuda.current_device())
    ws = _igemm_sk_workspace(device)
    st = ctypes.c_int(0)
    check(_lib.lib().dsrg_conv_igemm_workspace_status(_ptr(ws), _stream(), ctypes.byref(st)))
    return st.value


def dropout_seed():
    """a 63-bit seed for a fused dropout from torch's CPU generator (deterministic under torch.manual_seed, no device sync)"""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def conv_igemm_wgrad_supported(cin, cout, k):
    """the shapes conv_igemm_wgrad is the recommended route for (full 256 x 256 tiles): 256 | cout, 256 | cin (or cin = 128 for a 3x3
    kernel), k in (1, 3)"""
    cin, cout, k = int(cin), int(cout), int(k)
    return k in (1, 3) and ((cin >= 256 and cin % 256 == 0) or (cin == 128 and k == 3)) and cout >= 256 and cout % 256 == 0


def conv_igemm_wgrad_launchable(cin, cout, k):
    """the shapes the launch takes: any multiples of 64 channels (narrow tensors leave part of a tile empty — fine where the layer is
    bandwidth-bound: ResNet res2 / res3, 64 / 128 channels over 42 - 166 thousand pixels)"""
    return _lib.lib().dsrg_conv_igemm_wgrad_workspace(1, 1, 8, 8, int(cin), int(cout), int(k)) > 0


def conv_igemm_wgrad(xs, gs, dilations, ksize, out_dtype=torch.float32, outs=None):
    """weight gradients of 1 .. 4 convolutions of one geometry in one launch: xs[g] (B,cin,H,W) the layer inputs and gs[g]
    (B,cout,H,W) the output gradients, bf16 channels_last -> list of (cout,cin,k,k) channels_last tensors in float32 (the
    master weights' gradient) or bf16; cin % 256 == 0, cout % 256 == 0; fp32 accumulation, deterministic, no im2col matrix"""
    n = len(xs)
    B, cin, H, W = xs[0].shape
    cout = gs[0].shape[1]
    cl = torch.channels_last
    if not (1 <= n <= 4 and len(gs) == n and len(dilations) == n) or out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("conv_igemm_wgrad: 1..4 groups, float32 or bfloat16 result")
    if not all(_is_bf16(x, (B, cin, H, W)) and _is_bf16(g, (B, cout, H, W)) for x, g in zip(xs, gs)):
        raise ValueError("conv_igemm_wgrad needs bf16 CUDA tensors of one geometry")
    xs = [x.contiguous(memory_format=cl) for x in xs]
    gs = [g.contiguous(memory_format=cl) for g in gs]
    L = _lib.lib()
    need = L.dsrg_conv_igemm_wgrad_workspace(n, B, H, W, cin, cout, ksize)
    if need == 0:
        raise ValueError("conv_igemm_wgrad: 64 | cin, 64 | cout, k in (1, 3) required (got %d, %d, %d)" % (cin, cout, ksize))
    ws = _stream_scratch("igemm_wgrad", xs[0].device, need)          # reused across layers and steps
    gws = [_dest(outs[i] if outs is not None else None, (cout, cin, ksize, ksize), out_dtype, xs[0].device, True) for i in range(n)]
    check(L.dsrg_conv_igemm_wgrad_bf16(_ptrs(xs), _ptrs(gs), _ptrs(gws), _i32s(dilations), n, _ptr(ws), ws.numel(), B, H, W, cin, cout, ksize,
                                       int(out_dtype == torch.bfloat16), _stream()))
    return gws


def conv_igemm_wgrad_splits(n, B, H, W, cin, cout, ksize, dilations):
    """the pixel splits conv_igemm_wgrad runs for this launch, per (group, tap): a list of n lists of ksize * ksize counts (0: the
    tap reaches no pixel).  Host only: nothing is launched"""
    taps = int(ksize) * int(ksize)
    out = (ctypes.c_int * (n * taps))()
    check(_lib.lib().dsrg_conv_igemm_wgrad_splits(int(n), int(B), int(H), int(W), int(cin), int(cout), int(ksize),
                                                   (ctypes.c_int * n)(*[int(d) for d in dilations]), out))
    return [list(out[g * taps:(g + 1) * taps]) for g in range(n)]


def heads_forward(xs, weight, bias):
    """fc8-SEC_k + Eltwise SUM in float32: xs = list of <= 4 (B,K,H,W) bf16 channels_last activations, weight (n,O,K) f32,
    bias (n,O) f32 or None -> (B,O,H,W) float32, NCHW-contiguous (what the supervision path reads)."""
    B, K, H, W = xs[0].shape
    n, O = weight.shape[0], weight.shape[1]
    cl = torch.channels_last
    xs = [x.contiguous(memory_format=cl) for x in xs]
    if not all(x.is_cuda and x.dtype == torch.bfloat16 and x.shape == xs[0].shape for x in xs) or len(xs) != n:
        raise ValueError("heads_forward needs n bf16 CUDA activations of one shape")
    _f32c(weight, "weight")
    if bias is not None:
        _f32c(bias, "bias")
    out = torch.empty((B, O, H, W), dtype=torch.float32, device=xs[0].device)
    ptrs = (ctypes.c_void_p * 4)(*([x.data_ptr() for x in xs] + [None] * (4 - n)))
    check(_lib.lib().dsrg_heads_forward_bf16(ptrs, n, _ptr(weight), _ptr(bias), _ptr(out), B, H * W, K, O, _stream()))
    return out


def heads_backward(xs, weight, g, need_gx=True, relu_scale=0.0):
    """backward of heads_forward from the float32 score gradient g (B,O,H,W): -> (list of gx_k (B,K,H,W) bf16 channels_last or
    None, gw (n,O,K) float32).  relu_scale > 0: the x_k are ReLU (+ Dropout, scale relu_scale) outputs nobody else reads — the
    gx_k come out masked by x_k > 0 and scaled, and a third result (n,K) float32 is the bias gradient of the layer below"""
    B, K, H, W = xs[0].shape
    n, O = weight.shape[0], weight.shape[1]
    cl = torch.channels_last
    xs = [x.contiguous(memory_format=cl) for x in xs]
    _f32c(weight, "weight")
    g = g.contiguous()
    _f32c(g, "g")
    L = _lib.lib()
    M = B * H * W
    gx = torch.empty((n, B, H, W, K), dtype=torch.bfloat16, device=g.device) if need_gx else None
    gw = torch.empty((n, O, K), dtype=torch.float32, device=g.device)
    part = torch.empty(L.dsrg_heads_backward_chunks(M) * n * O * K, dtype=torch.float32, device=g.device)
    ptrs = (ctypes.c_void_p * 4)(*([x.data_ptr() for x in xs] + [None] * (4 - n)))
    if relu_scale > 0.0 and need_gx:
        gb = _bias_grad_dest(None, (n, K), g.device)
        ws = _reduction_scratch(g.device, L.dsrg_heads_backward_relu_workspace(n, M, K))
        check(L.dsrg_heads_backward_relu_bf16(ptrs, n, _ptr(weight), _ptr(g), _ptr(gx), M * K * 2, _ptr(gw), _ptr(part),
                                              float(relu_scale), _ptr(gb), _ptr(ws), ws.numel(), B, H * W, K, O, _stream()))
        return [gx[k].permute(0, 3, 1, 2) for k in range(n)], gw, gb
    check(L.dsrg_heads_backward_bf16(ptrs, n, _ptr(weight), _ptr(g), _ptr(gx), M * K * 2, _ptr(gw), _ptr(part), B, H * W, K, O,
                                     _stream()))
    return ([gx[k].permute(0, 3, 1, 2) for k in range(n)] if need_gx else None), gw


def _vp4(ts):
    """host array of four device pointers (the library reads the first len(ts))"""
    return (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - len(ts))))


def heads_kernels_in_place(weights, biases=None):
    """can heads_forward_ptrs / heads_backward_ptrs read these classifier parameters where they lie: <= 4 float32 CUDA kernels
    (O,K,1,1) or (O,K) of one shape whose memory is (O,K) row-major (a channels_last 1x1 kernel is), biases (O) alike"""
    if not 1 <= len(weights) <= 4 or weights[0].dim() < 2:
        return False
    O, K = weights[0].shape[0], weights[0].shape[1]
    if not all(w.is_cuda and w.dtype == torch.float32 and w.shape == weights[0].shape and w.numel() == O * K and w.is_contiguous()
               for w in weights):
        return False
    return biases is None or (len(biases) == len(weights) and all(
        b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (O,) and b.is_contiguous() for b in biases))


def heads_forward_ptrs(xs, weights, biases):
    """heads_forward with the n kernels (heads_kernels_in_place) and biases (a list, or None) read where they lie — no stacked
    copy of either; the same bits"""
    B, K, H, W = xs[0].shape
    n, O = len(weights), weights[0].shape[0]
    cl = torch.channels_last
    xs = [x.contiguous(memory_format=cl) for x in xs]
    if not all(x.is_cuda and x.dtype == torch.bfloat16 and x.shape == xs[0].shape for x in xs) or len(xs) != n:
        raise ValueError("heads_forward_ptrs needs n bf16 CUDA activations of one shape")
    if not heads_kernels_in_place(weights, biases) or weights[0].shape[1] != K:
        raise ValueError("heads_forward_ptrs needs n float32 CUDA kernels whose memory is (O,K) row-major, and (O) biases")
    out = torch.empty((B, O, H, W), dtype=torch.float32, device=xs[0].device)
    check(_lib.lib().dsrg_heads_forward_ptrs_bf16(_vp4(xs), n, _vp4(weights), _vp4(biases) if biases is not None else None, _ptr(out),
                                                  B, H * W, K, O, _stream()))
    return out


def heads_backward_ptrs(xs, weights, g, need_gx=True, relu_scale=0.0, gw_outs=None):
    """heads_backward with the kernels read where they lie and every branch's weight gradient written to a tensor of its own, of
    its kernel's shape and strides: gw_outs[k] if that can take it (a reducer's slot), else a fresh one -> (gx list or None, list of
    gw_k[, (n,K) bias gradient of the layer below when relu_scale > 0]); the same bits as the stacked form"""
    B, K, H, W = xs[0].shape
    n, O = len(weights), weights[0].shape[0]
    cl = torch.channels_last
    xs = [x.contiguous(memory_format=cl) for x in xs]
    if not heads_kernels_in_place(weights) or weights[0].shape[1] != K:
        raise ValueError("heads_backward_ptrs needs n float32 CUDA kernels whose memory is (O,K) row-major")
    g = g.contiguous()
    _f32c(g, "g")
    L = _lib.lib()
    M = B * H * W
    gx = torch.empty((n, B, H, W, K), dtype=torch.bfloat16, device=g.device) if need_gx else None
    gws = []
    for k, w in enumerate(weights):
        out = gw_outs[k] if gw_outs is not None else None
        if out is not None and out.dtype == torch.float32 and out.shape == w.shape and out.device == w.device and out.is_contiguous():
            gws.append(out)
        else:
            gws.append(torch.empty_strided(tuple(w.shape), tuple(w.stride()), dtype=torch.float32, device=g.device))
    part = torch.empty(L.dsrg_heads_backward_chunks(M) * n * O * K, dtype=torch.float32, device=g.device)
    masked = relu_scale > 0.0 and need_gx
    gb = _bias_grad_dest(None, (n, K), g.device) if masked else None
    ws = _reduction_scratch(g.device, L.dsrg_heads_backward_relu_workspace(n, M, K)) if masked else None
    check(L.dsrg_heads_backward_ptrs_bf16(_vp4(xs), n, _vp4(weights), _ptr(g), _ptr(gx), M * K * 2, _vp4(gws), _ptr(part),
                                          float(relu_scale) if masked else 0.0, _ptr(gb), _ptr(ws), ws.numel() if masked else 0,
                                          B, H * W, K, O, _stream()))
    gxs = [gx[k].permute(0, 3, 1, 2) for k in range(n)] if need_gx else None
    return (gxs, gws, gb) if masked else (gxs, gws)


def image_to_bf16_nhwc(x):
    """the network's input in one pass (dsrg_image_nchw_to_nhwc_bf16): x (B,3,H,W) float32 NCHW-contiguous -> (B,3,H,W) bf16
    channels_last, the bits of x.contiguous(memory_format=channels_last).bfloat16()"""
    if not (x.dim() == 4 and x.shape[1] == 3):
        raise ValueError("image_to_bf16_nhwc needs a (B,3,H,W) image")
    _f32c(x, "x")
    B, _, H, W = x.shape
    y = torch.empty((B, 3, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    check(_lib.lib().dsrg_image_nchw_to_nhwc_bf16(_ptr(x), _ptr(y), B, H, W, _stream()))
    return y


def image_takes_fused_cast(x):
    """is x an image image_to_bf16_nhwc takes: float32, three channels, NCHW-contiguous, on the GPU"""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.is_contiguous() and x.numel() > 0


def sum_bf16(ts):
    """rne(rne(rne(t0 + t1) + t2) + t3) of 2..4 bf16 CUDA tensors of one shape and one dense memory order (dsrg_sum_bf16): float32
    adds, one bf16 rounding after each, in list order — what autograd's pairwise accumulation of these gradients gives, in one
    pass.  -> a tensor of t0's shape and strides"""
    t0 = ts[0]
    if not (2 <= len(ts) <= 4 and all(t.is_cuda and t.dtype == torch.bfloat16 and t.shape == t0.shape and t.stride() == t0.stride()
                                      for t in ts) and t0.numel() % 8 == 0 and t0.numel() > 0 and
            (t0.is_contiguous() or (t0.dim() == 4 and t0.is_contiguous(memory_format=torch.channels_last)))):
        raise ValueError("sum_bf16 needs 2..4 dense bf16 CUDA tensors of one shape and layout, 8 | elements")
    out = torch.empty_like(t0)
    check(_lib.lib().dsrg_sum_bf16(_vp4(ts), len(ts), _ptr(out), t0.numel(), _stream()))
    return out


def maxpool3x3_out_size(n, stride, ceil_mode):
    """output extent of a 3x3 / pad 1 pooling window walk over n pixels (Caffe's ceil rule, torch's with ceil_mode)"""
    num = n + 2 - 3
    o = (-(-num // stride) if ceil_mode else num // stride) + 1
    if (o - 1) * stride >= n + 1:                       # the last window must start inside the image or its left pad
        o -= 1
    return o


def resnet_stem_pack(weight, scale):
    """the stem kernel of ResNet101DeepLab with its frozen BatchNorm scale folded in, packed once for resnet_stem
    (dsrg_pack_resnet_stem_f32): weight (64,3,7,7) float32, scale (64) float32 -> (64,192) bf16,
    packed[o][(ky * 3 + c) * 8 + kx] = bf16(weight[o,c,ky,kx] * scale[o]) (one float32 product, one rounding), zero where kx = 7 or
    ky * 3 + c >= 21"""
    if not (weight.is_cuda and weight.dtype == torch.float32 and tuple(weight.shape) == (64, 3, 7, 7)):
        raise ValueError("resnet_stem_pack needs a (64,3,7,7) float32 CUDA kernel")
    if tuple(scale.shape) != (64,):
        raise ValueError("resnet_stem_pack needs 64 scales")
    w = weight.detach().contiguous()
    nbytes = _lib.lib().dsrg_resnet_stem_packed_bytes()
    packed = torch.empty((64, nbytes // 128), dtype=torch.bfloat16, device=weight.device)
    check(_lib.lib().dsrg_pack_resnet_stem_f32(_ptr(w), _ptr(_f32c(scale.detach(), "scale")), _ptr(packed), _stream()))
    return packed


def resnet_stem(x, packed, shift):
    """the whole ResNet stem in one launch (dsrg_resnet_stem_bf16): x (B,3,H,W) float32 contiguous NCHW (rounded to bf16 as it is
    read), packed = resnet_stem_pack(weight, scale), shift (64) float32 -> max_pool(3, 2, 1, ceil)(relu(conv7x7/2(x) + shift)),
    (B,64,PH,PW) bf16 channels_last, rounded once; pool windows see only the real convolution map"""
    if not (x.dim() == 4 and x.shape[1] == 3):
        raise ValueError("resnet_stem needs a (B,3,H,W) input")
    x = _f32c(x, "x")
    B, _, H, W = x.shape
    if not (packed.is_cuda and packed.dtype == torch.bfloat16 and packed.is_contiguous()
            and packed.numel() * 2 == _lib.lib().dsrg_resnet_stem_packed_bytes()):
        raise ValueError("resnet_stem needs a kernel packed by resnet_stem_pack")
    if tuple(shift.shape) != (64,):
        raise ValueError("resnet_stem needs 64 shifts")
    OHc, OWc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = maxpool3x3_out_size(OHc, 2, True), maxpool3x3_out_size(OWc, 2, True)
    y = torch.empty((B, 64, PH, PW), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    check(_lib.lib().dsrg_resnet_stem_bf16(_ptr(x), _ptr(packed), _ptr(_f32c(shift, "shift")), _ptr(y), B, H, W, _stream()))
    return y


def maxpool3x3_fwd(x, stride, ceil_mode, relu_input=False):
    """x (B,C,H,W) bf16 channels_last -> (pooled (B,C,OH,OW) channels_last, window codes (B,OH,OW,C) uint8).
    relu_input: x is a ReLU's output and maxpool3x3_bwd_relu will be given these codes WITHOUT x — windows whose maximum is
    not positive get a code that names no position (the ReLU mask rides in the codes; the pooled values are the same)"""
    B, C, H, W = x.shape
    OH, OW = maxpool3x3_out_size(H, stride, ceil_mode), maxpool3x3_out_size(W, stride, ceil_mode)
    out = torch.empty((B, C, OH, OW), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    code = torch.empty((B, OH, OW, C), dtype=torch.uint8, device=x.device)
    fn = _lib.lib().dsrg_maxpool3x3_relu_fwd_bf16 if relu_input else _lib.lib().dsrg_maxpool3x3_fwd_bf16
    check(fn(_ptr(x), _ptr(out), _ptr(code), B, H, W, OH, OW, C, stride, _stream()))
    return out, code


def maxpool3x3_bwd(gout, code, in_shape, stride):
    B, C, H, W = in_shape
    OH, OW = gout.shape[2], gout.shape[3]
    gout = gout.contiguous(memory_format=torch.channels_last)
    gin = torch.empty((B, C, H, W), dtype=gout.dtype, device=gout.device, memory_format=torch.channels_last)
    check(_lib.lib().dsrg_maxpool3x3_bwd_bf16(_ptr(gout), _ptr(code), _ptr(gin), B, H, W, OH, OW, C, stride, _stream()))
    return gin


def maxpool3x3_bwd_relu(gout, code, relu_out, stride=2, gb_out=None):
    """3x3 / stride 2 / pad 1 max-pool backward + the ReLU backward and bias gradient of the convolution in front of the pool:
    relu_out (B,C,H,W) bf16 channels_last = the pool's input -> (masked input gradient (B,C,H,W) bf16 channels_last,
    bias gradient (C) f32); the same values as maxpool3x3_bwd followed by relu_bwd_bias.
    relu_out may be the pool input's SHAPE (a torch.Size / tuple) when `code` was made by maxpool3x3_fwd(relu_input=True): the
    codes then carry the mask and the input is not read (same bits)"""
    have_y = torch.is_tensor(relu_out)
    B, C, H, W = relu_out.shape if have_y else relu_out
    OH, OW = gout.shape[2], gout.shape[3]
    cl = torch.channels_last
    if stride != 2 or not (gout.is_cuda and gout.dtype == torch.bfloat16 and C % 8 == 0 and 256 % (C // 8) == 0) or (
            have_y and not (relu_out.is_cuda and relu_out.dtype == torch.bfloat16 and relu_out.is_contiguous(memory_format=cl))):
        raise ValueError("maxpool3x3_bwd_relu: stride 2, bf16 channels_last, channels / 8 a divisor of 256")
    gout = gout.contiguous(memory_format=cl)
    gin = torch.empty((B, C, H, W), dtype=torch.bfloat16, device=gout.device, memory_format=cl)
    gb = _bias_grad_dest(gb_out, (C,), gout.device)
    part = _reduction_scratch(gout.device, 4 * _PARTIAL_BLOCKS * C, "rows").view(torch.float32)
    check(_lib.lib().dsrg_maxpool3x3_bwd_relu_bf16(_ptr(gout), _ptr(code), _ptr(relu_out) if have_y else None, _ptr(gin), _ptr(gb), _ptr(part),
                                                   _PARTIAL_BLOCKS, B, H, W, OH, OW, C, _stream()))
    return gin, gb


class DSRGSupervision(torch.autograd.Function):
    """loss-Seed + loss-Constrain as a differentiable function of the fc8 logits."""

    @staticmethod
    def forward(ctx, logits, images, labels, cues, th1, th2, scale_factor, maxiter, prepared=False):
        losses, grad, _, total = supervision_step(logits.contiguous(), images, labels, cues, th1, th2, scale_factor, maxiter,
                                                  prepared=prepared, want_total=True)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(losses)
        ctx.set_materialize_grads(False)         # no zero-filled gradient made for `losses` (a launch per step nobody reads)
        return total, losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        (grad,) = ctx.saved_tensors
        return (grad * g_total if g_total is not None else None), None, None, None, None, None, None, None, None


def dsrg_supervision_loss(logits, images, labels, cues, th1=0.99, th2=0.85, scale_factor=12.0, maxiter=10,
                          prepared=False):
    """-> (total loss (differentiable wrt logits), tensor [loss-Seed, loss-Constrain])."""
    return DSRGSupervision.apply(logits, images, labels, cues, th1, th2, scale_factor, maxiter, prepared)
