"""Test-time path of the reference on MI355X ("next" row 1): multi-scale inference,
full-resolution dense CRF on log-probabilities, pseudo-label generation, and the evaluation metrics.

  preprocess            <-> training/tools/test-ms.py:68-81
  predict_mask_ms       <-> training/tools/test-ms.py:84-111        (run.sh:6,10: pseudo labels / final test)
  preprocess_relative   <-> training/tools/test-ms-f.py:100-112
  predict_mask_ms_f     <-> training/tools/test-ms-f.py:115-142     (run.sh step 4: the final test at relative scales)
  predict_masks_ms_f_many <-> the loop of test-ms-f.py:153-160 over the test list (same-sized images batched: plan_size_groups)
  predict_train_gt      <-> training/tools/generate_train_gt.py:78-106
  predict_train_gt_many <-> the loop of generate_train_gt.py:117-123 over train_aug (batched forwards, fused HIP tail)
  predict_train_gt_ms / predict_train_gt_ms_many (no counterpart in the reference) the pseudo-label pass as a probability ensemble:
                        the zoomed softmax of several sizes, optionally with their mirrors, averaged before the clamp; one size
                        without flip is the reference's pass
  ConfusionMatrix       <-> training/tools/evaluate.py:17-68
  flip=True             (no counterpart in the reference) mirrored test-time augmentation of the ms / ms-f functions: every scale
                        runs on the image and on its mirror image, the mirror's scores are mirrored back, all 2K maps are summed

The network runs in PyTorch-ROCm; resampling uses align-corners bilinear interpolation, which is the
sampling scipy.ndimage.zoom(order=1) performs ((in-1)/(out-1) mapping); the CRF is
krahenbuhl2013.CRF (device-resident form crf.CRF_device) -> libdsrg_hip.so (global-memory lattice path for full-resolution maps).
"""
import collections
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from .crf import CRF_device

MEAN_PIXEL = (104.0, 117.0, 123.0)


def _zoom(x, h, w):
    """x: (B,C,h0,w0) -> (B,C,h,w), order-1 zoom with scipy's (in-1)/(out-1) coordinate mapping"""
    if x.shape[2] == h and x.shape[3] == w:
        return x
    # in float64: scipy evaluates the sampling coordinate o * (in - 1) / (out - 1) and the two-tap blend in double and rounds
    # once; with float32 weights the result is off by up to 4e-5 of the value range (measured against scipy.ndimage.zoom,
    # tests/test_inference.py), in float64 by the final rounding only
    return F.interpolate(x.double(), size=(h, w), mode="bilinear", align_corners=True).to(x.dtype)


def _zoom_steps(x, h, w):
    """_zoom's arithmetic (align-corners order-1 zoom: coordinate o * (in - 1) / (out - 1), the two-tap blend
    l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11) in float64, rounded once to x.dtype) issued as separate torch
    ops, so that every product and sum is rounded on its own.  _zoom's single GPU kernel (upsample_bilinear2d on float64) is
    compiled with products contracted into FMAs and differs from this in the last bit of about one value in a thousand; this form
    is what csrc/multiscale.hip computes (-ffp-contract=off), bit for bit, on the GPU and on the CPU"""
    def axis(n_in, n_out):
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        src = torch.arange(n_out, dtype=torch.float64, device=x.device) * scale
        i0 = src.to(torch.int64)
        return i0, i0 + (i0 < n_in - 1).to(torch.int64), src - i0.to(torch.float64)

    y0, y1, l1h = axis(x.shape[2], h)
    x0, x1, l1w = axis(x.shape[3], w)
    l0h, l1h = (1.0 - l1h).view(-1, 1), l1h.view(-1, 1)
    l0w = 1.0 - l1w
    v = x.double()
    r0, r1 = v.index_select(2, y0), v.index_select(2, y1)
    top = l0w * r0.index_select(3, x0) + l1w * r0.index_select(3, x1)
    bottom = l0w * r1.index_select(3, x0) + l1w * r1.index_select(3, x1)
    return (l0h * top + l1h * bottom).to(x.dtype)


@contextlib.contextmanager
def _eval_mode(net):
    """the reference runs these passes with caffe.TEST, where Dropout is the identity (test-ms.py:56-58): switch a net
    that comes straight from a trainer to eval mode for the call and restore its mode afterwards"""
    was_training = net.training
    net.eval()
    try:
        yield net
    finally:
        net.train(was_training)


def _preprocess_to(image, h, w, device):
    """image: (H,W,3) RGB uint8/float zoomed to h x w (order 1, float64 blend: _zoom) -> (1,3,h,w) float32 BGR, mean-subtracted"""
    # (uploaded in the image's own dtype and converted on the device: a float32 conversion on the host is a multi-threaded torch op,
    # and the idle spin of its ~100 worker threads after every call eats a container's CPU quota — 7 ms per image became 95)
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(image))).to(device).to(torch.float32).permute(2, 0, 1)[None]
    x = _zoom(x, h, w)
    x = x[:, [2, 1, 0]]
    return x - torch.tensor(MEAN_PIXEL, dtype=torch.float32, device=device).view(1, 3, 1, 1)


def preprocess(image, size, device="cuda"):
    """image: (H,W,3) RGB uint8/float -> (1,3,size,size) float32 BGR, mean-subtracted (test-ms.py:68-81)"""
    return _preprocess_to(image, size, size, device)


def _device_image(image, device):
    """image (H,W,3) -> the uint8 tensor on the device that the CRF reads"""
    return torch.as_tensor(np.asarray(image).astype('ubyte'), device=device)


def _host_mask(labels):
    """a label map on the device -> (H,W) int64 array, the only thing that crosses PCIe"""
    return labels.cpu().numpy().astype(np.int64)


def _device_mask(labels):
    """a label map on the device -> the (H,W) int32 CUDA tensor masks="device" yields: the tensor itself where it is one already
    (the CRF's map, the kernels' arg-max), torch's int64 argmax narrowed on the device.  Nothing crosses PCIe, nothing waits"""
    return labels if labels.dtype == torch.int32 and labels.is_contiguous() else labels.to(torch.int32).contiguous()


def _mask_out(masks):
    """the `masks` keyword of the *_many generators -> what turns a label map on the device into the yielded mask.  "host" (the
    default): _host_mask, an (H,W) int64 array.  "device": _device_mask, the (H,W) int32 CUDA tensor, same values in the same order
    with no copy to the host anywhere on the path.  A yielded tensor is final: it is ordered before anything the consumer enqueues
    afterwards on the stream that was current when the generator was first advanced (the generators hand control back with that
    stream current), and its memory cannot be reused by the stream that produced it while work the consumer queued there is
    pending.  ValueError for any other value, before any stream or worker exists"""
    if masks == "host":
        return _host_mask
    if masks == "device":
        return _device_mask
    raise ValueError('masks must be "host" or "device", got %r' % (masks,))


class GraphedForward(object):
    """`net(x)` of an eval-mode network for the FIXED input shapes of the test-time loop (test-ms.py resizes every image to 241 / 321 /
    401 before the forward, whatever its own size) as captured HIP graphs: one backbone.GraphedForward per input shape (and autocast
    state), made at the first call with that shape and replayed afterwards.  A batch-1 forward is ~40 launches of 10-30 us of GPU
    work each; issued one by one from Python it takes 1.4 ms whatever the map size (host-bound), replayed it takes what the GPU needs.
    The graph re-reads (and re-packs) the parameters at every replay, so in-place weight updates are seen; the returned tensor is the
    graph's static output: consume it before the next call with the same shape.

    The relative scales of test-ms-f.py give every image size its own three input shapes.  max_shapes: keep at most that many
    graphs, dropping (and freeing) the least recently used one before a new capture; capture_after = n: a shape runs eagerly
    until its n-th call, which captures it, so one-off shapes are never captured.  The defaults (no bound, capture at the first
    call) keep every shape's graph."""

    def __init__(self, net, max_shapes=None, capture_after=1):
        if max_shapes is not None and int(max_shapes) < 1:
            raise ValueError("max_shapes must be at least 1")
        self.net = net
        self.max_shapes = None if max_shapes is None else int(max_shapes)
        self.capture_after = max(1, int(capture_after))
        self._g = collections.OrderedDict()        # key -> graph, least recently used first
        self._calls = collections.Counter()        # key -> calls so far (while not captured)

    def __call__(self, x):
        amp = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None
        key = (tuple(x.shape), x.dtype, amp)
        g = self._g.get(key)
        if g is not None:
            self._g.move_to_end(key)
            return g(x)
        if self.net.training:
            raise RuntimeError("GraphedForward needs an eval-mode network (no dropout stream inside a graph)")
        self._calls[key] += 1
        if self._calls[key] < self.capture_after:
            # what the captured graph runs (backbone.GraphedForward._fwd), issued eagerly
            with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                return self.net(x).contiguous()
        if self.max_shapes is not None:
            while len(self._g) >= self.max_shapes:
                self._g.popitem(last=False)        # the graph and its private memory pool go with the last reference
        from .backbone import GraphedForward as _OneShape
        # a capture may now begin while the CRF workers of a *_many generator are busy on their own streams: only this thread's
        # calls are held to the capture rules
        g = self._g[key] = _OneShape(self.net, x, amp_dtype=amp, capture_error_mode="thread_local")
        return g(x)

    def static_input(self, shape, dtype=torch.float32):
        """the input buffer of the graph captured for `shape` under the current autocast state, or None while there is none.  A
        caller that writes its input there and passes that tensor to __call__ saves the copy into the buffer."""
        amp = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None
        g = self._g.get((tuple(shape), dtype, amp))
        return None if g is None else g.x


@torch.no_grad()
def multiscale_scores(net, image, sizes=(241, 321, 401), device="cuda", forward=None):
    """sum over scales of the fc8 scores zoomed to the image resolution (test-ms.py:89-97) -> (C,H,W).  forward: a callable used in
    place of `net` for the forward passes (a GraphedForward of the same net, already in eval mode)"""
    d1, d2 = image.shape[0], image.shape[1]
    total = None
    with _eval_mode(net):
        for size in sizes:
            scores = (forward or net)(preprocess(image, size, device)).float()
            scores = _zoom(scores, d1, d2)
            total = scores if total is None else total + scores
    return total[0]


def _probs_from_scores(scores, eps=0.00001):
    probs = torch.softmax(scores, dim=0)
    return torch.clamp(probs, min=eps)                       # probs[probs < eps] = eps (test-ms.py:102-103)


MAX_FLIP_SCALES = 4         # scales with flip=True: 2 K <= 8 maps in one dsrg_multiscale_unary_mirror launch
MAX_FLIP_BATCH = 8          # images per group with flip=True: two slots each in the batched forwards


def _check_flip(nscales, group=1):
    """the limits of flip=True, checked before any launch"""
    if nscales > MAX_FLIP_SCALES:
        raise ValueError("flip=True takes at most %d scales (each runs twice), got %d" % (MAX_FLIP_SCALES, nscales))
    if int(group) > MAX_FLIP_BATCH:
        raise ValueError("flip=True takes groups of at most %d images (two slots each), got %d" % (MAX_FLIP_BATCH, int(group)))


def _forwards(net, forward, xs):
    """the forwards of every test-time function: net (in eval mode for the call), or `forward` in its place (a GraphedForward of
    the same net), on each network input of xs -> list of contiguous float32 score maps.  A graph's output is its static buffer,
    which the replay for a later input of the same shape would overwrite: such a map is cloned; every other map is what the
    forward returned"""
    xs = list(xs)
    shapes = [tuple(x.shape) for x in xs]
    maps = []
    with _eval_mode(net):
        for k, x in enumerate(xs):
            sc = (forward or net)(x).float()
            if forward is not None and shapes[k] in shapes[k + 1:]:
                sc = sc.clone()
            maps.append(sc.contiguous())
    return maps


def _with_mirrors(slots):
    """per-image network inputs -> each followed by its mirror image (the slot pairs of the flip forwards)"""
    return [t for x in slots for t in (x, x.flip(-1))]


def _flip_pair_scores(net, inputs, forward):
    """flip=True, one image: every (1,3,h,w) network input runs with its mirror image as one batch-2 forward,
    cat([x, x.flip(-1)]) (a GraphedForward holds batch-2 graphs) -> the 2K (1,C,h',w') float32 score maps in the order of the
    sum: scale 0 plain, scale 0 mirror, scale 1 plain, ...  The mirror maps are NOT mirrored back here: ops.multiscale_unary
    (mirror=[0, 1, 0, 1, ...]) reads them reversed, the torch composition flips them"""
    return [half for sc in _forwards(net, forward, [torch.cat(_with_mirrors([x])) for x in inputs]) for half in (sc[0:1], sc[1:2])]


def _ms_flip_result(net, image, sizes, device, forward, want):
    """test-ms.py:89-103 with flip=True for one image: len(sizes) batch-2 forwards and one dsrg_multiscale_unary_mirror launch"""
    from . import ops
    maps = _flip_pair_scores(net, [preprocess(image, size, device) for size in sizes], forward)
    return ops.multiscale_unary(maps, image.shape[0], image.shape[1], eps=0.00001, want=want, mirror=[0, 1] * len(sizes))


def _ms_unary(net, image, sizes, device, forward, flip):
    """test-ms.py:89-103 for one image -> (H,W,C) float32 log-probabilities: the torch composition, or with flip the fused tail"""
    if flip:
        return _ms_flip_result(net, image, sizes, device, forward, "unary")
    probs = _probs_from_scores(multiscale_scores(net, image, sizes, device, forward))
    return torch.log(probs).permute(1, 2, 0).contiguous()


@torch.no_grad()
def predict_mask_ms(net, image, smooth=True, sizes=(241, 321, 401), device="cuda", forward=None, flip=False):
    """test-ms.py:84-111 -> (H,W) int64 label mask.  forward: see multiscale_scores.  flip=True (at most 4 sizes): every size
    runs on the image and its mirror image as one batch-2 forward, and the tail is the fused kernel (one
    dsrg_multiscale_unary_mirror launch on the 2K maps: zoom, the mirrors read reversed, sum, softmax, clamp, log) instead of the
    torch composition this function runs without flip"""
    return _host_mask(_ms_labels(net, image, smooth, tuple(sizes), device, forward, flip))


def _ms_labels(net, image, smooth, sizes, device, forward, flip):
    """predict_mask_ms up to the label map on the device: (H,W) int32, or int64 where it is torch's argmax (no CRF, no flip)"""
    if flip:
        _check_flip(len(sizes))
    if smooth:
        # scores, log-probabilities, CRF and arg-max all stay on the GPU; only the (H,W) mask crosses PCIe
        unary = _ms_unary(net, image, sizes, device, forward, flip)
        return CRF_device(_device_image(image, unary.device), unary, scale_factor=1.0, want="map")
    if flip:
        return _ms_flip_result(net, image, sizes, device, forward, "argmax")
    return _probs_from_scores(multiscale_scores(net, image, sizes, device, forward)).argmax(0)


MAX_FORWARD_BATCH = 16      # images per group of the batched path (the limit of the two batched kernels)


def _forward_groups(items, G):
    """items (any iterable) G at a time, in order -> lists of exactly G entries; the tail group is padded with None, the slots
    that the batched forwards run on zeros"""
    G = int(G)
    if not 1 <= G <= MAX_FORWARD_BATCH:
        raise ValueError("forward_batch must be 1..%d, got %d" % (MAX_FORWARD_BATCH, G))
    group = []
    for item in items:
        group.append(item)
        if len(group) == G:
            yield group
            group = []
    if group:
        yield group + [None] * (G - len(group))


# ---- one group of images: inputs, K batched forwards, one tail launch (the batched forms of ms, ms-f and gt) -----------------------
def _preprocess_square_batch(images, shapes, **kw):
    """ops.preprocess_ms_batch on (S, S) targets: the launch of the fixed sizes (preprocess_rect_batch's bits under its own name)"""
    from . import ops
    return ops.preprocess_ms_batch(images, [h for h, _ in shapes], **kw)


def _group_inputs(images, shapes, device, forward, flip, square=False):
    """one group -> (its images on the device, the K network inputs (B, 3, h_k, w_k) for the targets `shapes`).  images may end in
    None, the padding slots of _forward_groups, which run on zeros; B = len(images), with flip twice that: image g in slot 2g, its
    mirror image in slot 2g+1, the padding behind them.  uint8 images take ONE launch — dsrg_preprocess_rect_batch, with
    square=True (every target (S, S): the fixed sizes of test-ms.py) dsrg_preprocess_ms_batch, with flip
    dsrg_preprocess_rect_mirror_batch — written straight into the static inputs of `forward`'s graphs where those exist; in a
    group with other dtypes every slot is made on its own, those images by _preprocess_to"""
    from . import ops
    B = (2 if flip else 1) * len(images)                    # the batch of the forwards
    arrays = [np.ascontiguousarray(np.asarray(im)) for im in images if im is not None]
    plain = _preprocess_square_batch if square else ops.preprocess_rect_batch
    if all(a.dtype == np.uint8 for a in arrays):
        dev_images = [torch.from_numpy(a).to(device) for a in arrays]
        out = None
        if isinstance(forward, GraphedForward):
            out = [forward.static_input((B, 3, h, w)) for h, w in shapes]
            if len(set(shapes)) != len(shapes) or any(o is None for o in out):
                out = None                                  # (not captured yet: GraphedForward copies a fresh tensor in)
        return dev_images, (ops.preprocess_rect_mirror_batch if flip else plain)(dev_images, shapes, capacity=B, mean=MEAN_PIXEL,
                                                                                  out=out)
    dev_images = [_device_image(a, device) for a in arrays]
    xs = []
    for h, w in shapes:
        slots = [plain([d], [(h, w)], mean=MEAN_PIXEL)[0] if a.dtype == np.uint8 else _preprocess_to(a, h, w, device)
                 for a, d in zip(arrays, dev_images)]
        if flip:
            slots = _with_mirrors(slots)
        if len(slots) < B:
            slots.append(torch.zeros((B - len(slots), 3, h, w), dtype=torch.float32, device=device))
        xs.append(torch.cat(slots))
    return dev_images, xs


def _group_results(net, images, shapes, device, forward, want, flip, square=False):
    """test-ms.py:89-103 / test-ms-f.py:121-134 for one group: _group_inputs, len(shapes) batched forwards and one
    dsrg_multiscale_unary_batch launch (flip: dsrg_multiscale_unary_mirror_batch on the slot pairs) -> (the images on the device,
    the `want` output of ops.multiscale_unary per image); the padding slots' results are dropped"""
    from . import ops
    dev_images, xs = _group_inputs(images, shapes, device, forward, flip, square)
    scores = _forwards(net, forward, xs)
    tail = ops.multiscale_unary_mirror_batch if flip else ops.multiscale_unary_batch
    return dev_images, tail(scores, [(im.shape[0], im.shape[1]) for im in dev_images], eps=0.00001, want=want)


@torch.no_grad()
def predict_masks_ms_many(net, images, sizes=(241, 321, 401), device="cuda", forward=None, in_flight=3, batch=1, forward_batch=1,
                          flip=False, smooth=True, masks="host"):
    """predict_mask_ms over many images (the loop of test-ms.py over a split's 1 449 / 10 582 images), as a generator of (H,W) int64
    masks in order: the forwards of image i + 1 (on the caller's stream; `forward`: a GraphedForward) run while the CRFs of the images
    before it are in flight on `in_flight` worker streams (crf.CRF_device_many; batch > 1: consecutive same-sized images share one
    batched CRF call).  Same masks as predict_mask_ms image by image.  smooth=False: the arg-max, no CRF (and no stream or worker).

    forward_batch = G > 1: the images are taken G at a time.  test-ms.py resizes every image to the same `sizes`, so a group's
    forwards are len(sizes) batch-G forwards (a GraphedForward holds one batch-G graph per size; the tail group is padded with
    zero inputs) between one dsrg_preprocess_ms_batch launch and one dsrg_multiscale_unary_batch launch.  A batch-G forward need
    not round as a batch-1 forward does: the masks are predict_mask_ms's except where two labels all but tie.

    flip=True: predict_mask_ms(flip=True) image by image; with forward_batch = G (at most 8, and at most 4 sizes: ValueError
    before any stream or worker exists) a group is one dsrg_preprocess_rect_mirror_batch launch, len(sizes) batch-2G forwards
    (image g in slot 2g, its mirror image in slot 2g+1, the padding slots zero) and one dsrg_multiscale_unary_mirror_batch
    launch.

    masks="device": the (H,W) int32 CUDA tensors instead, nothing copied to the host (_mask_out has the contract)."""
    sizes = tuple(sizes)
    out = _mask_out(masks)
    if flip:
        _check_flip(len(sizes), forward_batch)
    if int(forward_batch) != 1:
        def results():
            for group in _forward_groups(images, forward_batch):
                yield from zip(*_group_results(net, group, [(S, S) for S in sizes], device, forward,
                                               "unary" if smooth else "argmax", flip, square=True))
    elif smooth:
        def results():
            for image in images:
                unary = _ms_unary(net, image, sizes, device, forward, flip)
                yield _device_image(image, unary.device), unary
    else:
        for image in images:
            yield out(_ms_labels(net, image, False, sizes, device, forward, flip))
        return
    if smooth:
        yield from _crf_in_flight(results(), device, in_flight, batch, masks=masks)
    else:
        for _, labels in results():
            yield out(labels)


@torch.no_grad()
def predict_masks_ms_batched(net, images, smooth=True, sizes=(241, 321, 401), device="cuda", forward=None, in_flight=3, batch=1,
                             capacity=None, flip=False):
    """predict_masks_ms_many(forward_batch=capacity) for ONE group of 1..16 images, as a list of (H,W) int64 masks.
    smooth=False: the arg-max of the summed scores (dsrg_multiscale_unary_batch's), no CRF.  capacity (default: the number of
    images): the batch size of the forwards, the slots beyond the images run on zeros (a tail group on the full groups' graphs).
    flip=True: as predict_masks_ms_many(flip=True); at most 8 images in the capacity, the forwards' batch is twice the capacity"""
    images = list(images)
    capacity = len(images) if capacity is None else int(capacity)
    sizes = tuple(sizes)
    if flip:
        _check_flip(len(sizes), capacity)
    if not 1 <= len(images) <= capacity <= MAX_FORWARD_BATCH:
        raise ValueError("one group holds 1..%d images within its capacity, got %d in %d" % (MAX_FORWARD_BATCH, len(images), capacity))
    dev_images, outs = _group_results(net, images + [None] * (capacity - len(images)), [(S, S) for S in sizes], device, forward,
                                      "unary" if smooth else "argmax", flip, square=True)
    if smooth:
        return list(_crf_in_flight(zip(dev_images, outs), device, in_flight, batch))
    return [_host_mask(labels) for labels in outs]


def _crf_in_flight(pairs, device, in_flight, batch, ignore_below=None, masks="host"):
    """the CRF half of the *_many generators: (image, unary) pairs -> (H,W) int64 masks in order, CRFs on worker streams while the
    pairs (the forwards) are produced on a forward stream of their own.  (image, unary, select) triples: the masks are restricted
    to each image's label list (crf.CRF_device_many), with ignore_below as DenseCRF.map takes it.

    masks="device": the workers' (H,W) int32 label maps themselves.  Between two yields this generator keeps the forward stream
    current, and a consumer's launches would land there, among the forwards; so a device mask is handed over with the CALLER's
    stream — the one current when the generator was first advanced — made current again for as long as the consumer holds
    control.  The map is final before that: the worker's library call returned with its stream drained (crf.CRF_device_many), so
    whatever the consumer enqueues, on any stream, comes after it.  Its memory belongs to the worker stream's pool and is marked
    as in use on the caller's stream (record_stream, as CRF_device_many marks it for the stream it was started on, here the
    forward stream): the worker cannot get the block back while launches the consumer queued on it are pending"""
    _mask_out(masks)
    from .crf import CRF_device_many
    from .streams import side_stream
    # the CRF workers come back from the library three times per image and need the interpreter lock for a few lines each time; the
    # caller's thread, busy issuing torch ops, would keep it for Python's default 5 ms switch interval — longer than a whole CRF
    import sys
    interval = sys.getswitchinterval()
    sys.setswitchinterval(min(interval, 1e-4))
    # ... and the forwards go to a stream of their own: on the caller's (usually the null) stream they share a hardware queue with one of
    # the CRF workers' streams or not, depending on how many streams the process made before — 178 or 240 images/s from run to run
    fstream = side_stream(device)
    caller = torch.cuda.current_stream(device)
    try:
        fstream.wait_stream(caller)
        with torch.cuda.stream(fstream):
            for lab in CRF_device_many(pairs, scale_factor=1.0, want="map", in_flight=in_flight, batch=batch,
                                       ignore_below=ignore_below):
                if masks == "host":
                    yield _host_mask(lab)
                    continue
                lab = _device_mask(lab)
                lab.record_stream(caller)
                with torch.cuda.stream(caller):
                    yield lab
    finally:
        sys.setswitchinterval(interval)
        # what the forward stream still holds (a forward issued ahead of a generator that was closed early, writes into a graph's
        # static buffers) is ordered before whatever the caller enqueues next; every yielded mask was already final
        caller.wait_stream(fstream)


# ---- the final test at relative scales (test-ms-f.py, run.sh step 4) ----------------------------------------------------------------
def relative_size(n, factor):
    """the length scipy.ndimage.zoom gives an axis of n samples zoomed by `factor`, as the reference ran it: scipy 0.18
    (python-dependencies.txt:15) computes int(round(n * factor)) and the reference ran under Python 2 (test-ms-f.py:154 is a print
    statement), whose round() takes halves away from zero: 334 * 0.75 = 250.5 -> 251, 338 * 1.25 = 422.5 -> 423 (Python 3's
    half-to-even round gives 250 / 422).  This follows from reading the two versions' code; no Python 2 run has confirmed it."""
    x = n * float(factor)
    f = math.floor(x)
    return int(f + 1 if x - f >= 0.5 else f)


def preprocess_relative(image, factor, device="cuda"):
    """test-ms-f.py:100-112: image (H,W,3) RGB uint8/float zoomed by `factor` (order 1, float64 blend as in _zoom) to
    (relative_size(H), relative_size(W)), BGR, mean-subtracted -> (1,3,h,w) float32"""
    return _preprocess_to(image, relative_size(image.shape[0], factor), relative_size(image.shape[1], factor), device)


def _relative_unary(net, image, scales, device, forward, fused, smooth, flip=False, want=None):
    """test-ms-f.py:121-134 -> (H,W,C) float32 log-probabilities (smooth) or (H,W) arg-max labels.  fused: one
    dsrg_multiscale_unary launch after the forwards; otherwise the torch composition (_zoom, sum, softmax, clamp, log).
    flip: batch-2 forwards (_flip_pair_scores); fused, one dsrg_multiscale_unary_mirror launch on the 2K maps, otherwise
    torch.flip of the mirrors' scores, the zoom and the sum in the same order — the zoom as _zoom_steps, _zoom's arithmetic
    without contracted products, so that the composition's sum is the fused kernel's bit for bit.  want="sum": the (H,W,C)
    summed scores of either route instead (parity checks)"""
    d1, d2 = image.shape[0], image.shape[1]
    want = want or ("unary" if smooth else "argmax")
    if flip:
        _check_flip(len(scales))
    xs = [preprocess_relative(image, s, device) for s in scales]
    scores = _flip_pair_scores(net, xs, forward) if flip else _forwards(net, forward, xs)
    if fused:
        from . import ops
        return ops.multiscale_unary(scores, d1, d2, eps=0.00001, want=want, mirror=[0, 1] * len(scales) if flip else None)
    total = None
    for k, sc in enumerate(scores):
        z = _zoom_steps(torch.flip(sc, [-1]) if k % 2 else sc, d1, d2) if flip else _zoom(sc, d1, d2)
        total = z if total is None else total + z
    if want == "sum":
        return total[0].permute(1, 2, 0).contiguous()
    probs = _probs_from_scores(total[0])
    if want == "unary":
        return torch.log(probs).permute(1, 2, 0).contiguous()
    return probs.argmax(0)


@torch.no_grad()
def predict_mask_ms_f(net, image, scales=(0.75, 1.0, 1.25), smooth=True, device="cuda", forward=None, fused=True, flip=False):
    """test-ms-f.py:115-142 -> (H,W) int64 label mask: forwards at `scales` relative to the image's own size, the fused
    multi-scale unary, then the full-resolution CRF (smooth) or the arg-max.  forward: see multiscale_scores (a GraphedForward,
    best bounded: GraphedForward(net, max_shapes=..., capture_after=2)); fused=False: the torch composition, for A/B runs.
    flip=True (at most 4 scales): every scale runs on the image and its mirror image as one batch-2 forward, the mirror's scores
    are mirrored back and all 2K maps summed (scale 0 plain, scale 0 mirror, scale 1 plain, ...) before the softmax: one
    dsrg_multiscale_unary_mirror launch, or with fused=False torch.flip of the mirrors' scores in the torch composition (zoomed
    by _zoom_steps: its summed scores are the kernel's bit for bit)"""
    return _host_mask(_ms_f_labels(net, image, tuple(scales), smooth, device, forward, fused, flip))


def _ms_f_labels(net, image, scales, smooth, device, forward, fused, flip):
    """predict_mask_ms_f up to the label map on the device: (H,W) int32, or int64 where it is torch's argmax (fused=False, no CRF)"""
    out = _relative_unary(net, image, scales, device, forward, fused, smooth, flip)
    if smooth:
        out = CRF_device(_device_image(image, out.device), out, scale_factor=1.0, want="map")
    return out


def plan_size_groups(keys, G, window):
    """the scheduler of the batched relative-scale test: collects same-keyed inputs (images keyed by their size) from a mixed
    stream into groups of up to G.  keys: any iterable of hashable keys, consumed lazily one key at a time; a generator of lists
    of input indices, ascending inside a list, every index in exactly one list.  For key i:
      (a) i joins its key's bucket;
      (b) a bucket that now holds G indices is emitted;
      (c) while anything is pending and i + 1 - (the oldest pending index) >= window, the whole bucket that holds the oldest
          pending index is emitted;
      (d) at the end of the input the remaining buckets are emitted in the order of their oldest members.
    So an input waits for at most window - 1 later inputs before its group is emitted, which bounds both the inputs held back
    (fewer than `window`) and the results a consumer holds to restore the input order; key i + 1 is not pulled before the
    groups due at key i were yielded.  window = 1 gives one input per group.  G outside 1..16 or window < 1: ValueError (at the
    call, not at the first group)."""
    G, window = int(G), int(window)
    if not 1 <= G <= MAX_FORWARD_BATCH:
        raise ValueError("groups hold 1..%d inputs, got %d" % (MAX_FORWARD_BATCH, G))
    if window < 1:
        raise ValueError("window must be at least 1, got %d" % window)

    def groups():
        buckets = {}                                        # key -> pending indices (fewer than `window` in all)
        for i, key in enumerate(keys):
            bucket = buckets.setdefault(key, [])
            bucket.append(i)
            if len(bucket) == G:
                yield buckets.pop(key)
            while buckets:
                oldest = min(buckets, key=lambda k: buckets[k][0])
                if i + 1 - buckets[oldest][0] < window:
                    break
                yield buckets.pop(oldest)
        for bucket in sorted(buckets.values(), key=lambda b: b[0]):
            yield bucket

    return groups()


def _relative_shapes(H, W, scales):
    """the network input sizes of an H x W image at the relative scales; one below one pixel: ValueError"""
    shapes = [(relative_size(H, s), relative_size(W, s)) for s in scales]
    if any(h < 1 or w < 1 for h, w in shapes):
        raise ValueError("a %d x %d image at the scales %s gives an input below one pixel: %s" % (H, W, tuple(scales), shapes))
    return shapes


@torch.no_grad()
def predict_masks_ms_f_many(net, images, scales=(0.75, 1.0, 1.25), device="cuda", forward=None, in_flight=3, batch=1, fused=True,
                            same_size_batch=1, window=64, smooth=True, flip=False, masks="host"):
    """predict_mask_ms_f over many images, as predict_masks_ms_many does it for test-ms.py: a generator of (H,W) int64 masks
    in order, the forwards of the next image running while the CRFs of the images before it are in flight (smooth=False: the
    arg-max, no CRF).  Same masks as predict_mask_ms_f image by image.

    same_size_batch = G > 1 (2..16): the relative scales give every image SIZE its own input shapes, and a dataset holds few
    sizes, so the images are keyed by (H, W) and collected by plan_size_groups(G, window) into groups of up to G same-sized
    images.  A group of n images (never padded to G) is one dsrg_preprocess_rect_batch launch, len(scales) batch-n forwards (a
    GraphedForward holds a graph per (n, size, scale) under its own capture_after / max_shapes policy) and one
    dsrg_multiscale_unary_batch launch; its (image, unary) pairs reach the CRFs consecutively, so batch > 1 gives them one batched
    CRF call.  Masks come back in input order through a reorder buffer: an image waits for at most window - 1 later images, so
    fewer than `window` images and masks are held (window = 64 is a judgement, not a measurement).  A batch-n forward need not
    round as a batch-1 forward does: the masks are predict_mask_ms_f's except where two labels all but tie, and there they
    depend on the grouping (G, window and the order of the images).  A relative size below one pixel: ValueError before any
    launch of that group.  These groups run the fused kernels only (fused=False: ValueError).

    flip=True: predict_mask_ms_f(flip=True) image by image; with same_size_batch = G (at most 8, and at most 4 scales:
    ValueError before any stream or worker exists) a group of n images is one dsrg_preprocess_rect_mirror_batch launch,
    len(scales) batch-2n forwards and one dsrg_multiscale_unary_mirror_batch launch.

    masks="device": the (H,W) int32 CUDA tensors instead, nothing copied to the host (_mask_out has the contract); the reorder
    buffer of same_size_batch > 1 then holds device tensors."""
    G = int(same_size_batch)
    scales = tuple(scales)
    to_mask = _mask_out(masks)
    if flip:
        _check_flip(len(scales), G)
    if G != 1:
        if not fused:
            raise ValueError("same_size_batch > 1 runs the fused kernels only")
        held_images, order = {}, collections.deque()       # images waiting for their group; input indices in emission order

        def keys():
            for i, image in enumerate(images):
                held_images[i] = image
                yield (image.shape[0], image.shape[1])

        groups = plan_size_groups(keys(), G, window)        # (G and window are checked here, before any stream or worker exists)

        def results():
            for idx in groups:
                group = [held_images.pop(i) for i in idx]
                shapes = _relative_shapes(group[0].shape[0], group[0].shape[1], scales)     # (checked ahead of any launch)
                dev_images, outs = _group_results(net, group, shapes, device, forward, "unary" if smooth else "argmax", flip)
                for i, im, out in zip(idx, dev_images, outs):
                    order.append(i)
                    yield im, out

        if smooth:
            produced = _crf_in_flight(results(), device, in_flight, batch, masks=masks)
        else:
            produced = (to_mask(lab) for _, lab in results())
        held_masks, nxt = {}, 0
        for mask in produced:
            held_masks[order.popleft()] = mask
            while nxt in held_masks:
                yield held_masks.pop(nxt)
                nxt += 1
        return
    if not smooth:
        for image in images:
            yield to_mask(_ms_f_labels(net, image, scales, False, device, forward, fused, flip))
        return

    def pairs():
        for image in images:
            unary = _relative_unary(net, image, scales, device, forward, fused, True, flip)
            yield _device_image(image, unary.device), unary

    yield from _crf_in_flight(pairs(), device, in_flight, batch, masks=masks)


@torch.no_grad()
def predict_train_gt(net, image, labels, smooth=True, device="cuda"):
    """generate_train_gt.py:78-106: single-scale (321) softmax, zoomed to the image, CRF on log-probs,
    argmax restricted to background + the image-level labels -> (H,W) int64 pseudo-label mask.  It is predict_train_gt_ms at the
    one size 321 without flip: the same torch operations in the same order (one map: no sum, no division)"""
    return predict_train_gt_ms(net, image, labels, sizes=(321,), flip=False, smooth=smooth, device=device)


def train_gt_selection(labels):
    """the label list of generate_train_gt.py:98-99 (`labels.insert(0, 0)`): background, then the image-level labels in the order
    (and with the duplicates) given"""
    return [0] + [int(l) for l in labels]


def predict_train_gt_many(net, items, smooth=True, size=321, device="cuda", forward=None, in_flight=3, batch=1, forward_batch=1,
                          ignore_below=None, masks="host"):
    """generate_train_gt.py:78-106 over many images (its loop over the 10 582 images of train_aug): items is an iterable of
    (image (H,W,3) RGB, image-level labels); a generator of (H,W) int64 masks in order, each restricted to background + the
    image's labels.  It is predict_train_gt_ms_many at the one size `size` without flip, which see for the groups, the CRFs and
    ignore_below: per group of forward_batch = G images one dsrg_preprocess_ms_batch launch at `size`, ONE batch-G forward and the
    pseudo-label tail on its one map per image (softmax at map resolution, zoom of the probabilities, clamp, log).
    forward_batch=1 is the per-image route on the same kernels; outside 1..16: ValueError before any launch.  A batch-G forward
    need not round as a batch-1 forward does: the masks are predict_train_gt's except where two labels all but tie.
    masks="device": the (H,W) int32 CUDA tensors instead (_mask_out has the contract)."""
    return predict_train_gt_ms_many(net, items, sizes=(size,), flip=False, smooth=smooth, device=device, forward=forward,
                                    in_flight=in_flight, batch=batch, forward_batch=forward_batch, ignore_below=ignore_below,
                                    masks=masks)


MAX_ENSEMBLE_MAPS = 8       # maps per image in one dsrg_train_gt_ensemble_batch: K sizes, with flip=True two maps each


def _check_ensemble(nsizes, flip, group=1):
    """the limits of the gt-ms functions (_check_flip's sibling), checked before any launch"""
    per = 2 if flip else 1
    if not 1 <= nsizes * per <= MAX_ENSEMBLE_MAPS:
        raise ValueError("gt-ms takes 1..%d sizes%s, got %d" % (MAX_ENSEMBLE_MAPS // per, " with flip=True (each runs twice)" if flip else "",
                                                             nsizes))
    if flip and int(group) > MAX_FLIP_BATCH:
        raise ValueError("flip=True takes groups of at most %d images (two slots each), got %d" % (MAX_FLIP_BATCH, int(group)))


def _train_gt_ms_probs(net, image, sizes, flip, device):
    """the ensemble of predict_train_gt_ms -> (C,H,W) float32 clamped probabilities: per size the softmax at map resolution zoomed
    to the image (_zoom), with flip also that of the mirrored input's scores mirrored back (flip(-1)); the float32 sum in the order
    size 0 plain, size 0 mirror, size 1 plain, ..., divided by the number of maps M (not at M = 1), clamped at 1e-5"""
    d1, d2 = image.shape[0], image.shape[1]
    acc = None
    with _eval_mode(net):
        for size in sizes:
            x = preprocess(image, size, device)
            maps = [net(x).float()] + ([net(x.flip(-1)).float().flip(-1)] if flip else [])
            for sc in maps:
                z = _zoom(torch.softmax(sc, dim=1), d1, d2)[0]
                acc = z if acc is None else acc + z
    M = len(sizes) * (2 if flip else 1)
    return torch.clamp(acc / float(M) if M > 1 else acc, min=0.00001)


@torch.no_grad()
def predict_train_gt_ms(net, image, labels, sizes=(241, 321, 401), flip=False, smooth=True, device="cuda"):
    """The pseudo-label mask of one image from a probability ensemble over `sizes`, with flip=True each size also on the mirror
    image (no counterpart in the reference; sizes=(321,) without flip is predict_train_gt, generate_train_gt.py:78-106): the mean
    of the zoomed softmax maps (_train_gt_ms_probs), CRF on its log, arg-max restricted to background + the image-level labels ->
    (H,W) int64 pseudo-label mask.  The per-image torch composition: the A/B route of predict_train_gt_ms_many"""
    sizes = tuple(sizes)
    _check_ensemble(len(sizes), flip)
    probs = _train_gt_ms_probs(net, image, sizes, flip, device)
    if smooth:
        unary = torch.log(probs).permute(1, 2, 0).contiguous()
        p = CRF_device(_device_image(image, unary.device), unary, scale_factor=1.0)
    else:
        p = probs.permute(1, 2, 0)
    sel = torch.as_tensor(train_gt_selection(labels), device=p.device)
    return sel[p[:, :, sel].argmax(2)].cpu().numpy()


@torch.no_grad()
def predict_train_gt_ms_many(net, items, sizes=(241, 321, 401), flip=False, smooth=True, device="cuda", forward=None, in_flight=3,
                             batch=1, forward_batch=1, ignore_below=None, masks="host"):
    """The pseudo-label pass over many images as a probability ensemble over `sizes`, with flip=True each size also on the mirror
    image (no counterpart in the reference; sizes=(S,) without flip is predict_train_gt_many(size=S)): items is an iterable of
    (image (H,W,3) RGB, image-level labels); a generator of (H,W) int64 masks in order, each restricted to background + the
    image's labels.  The images are taken forward_batch = G at a time (the tail group is padded with zero inputs): one
    preprocessing launch (dsrg_preprocess_ms_batch, into the static inputs of `forward`'s graphs where `forward` is a
    GraphedForward; flip: dsrg_preprocess_rect_mirror_batch, image g in slot 2g, its mirror image in slot 2g+1), len(sizes)
    batched forwards and one dsrg_train_gt_ensemble_batch (two launches: the softmax of every map at map resolution; the zoom of
    the probabilities, their mean in the order size 0 plain, size 0 mirror, size 1 plain, ..., clamp, log).  smooth: the
    full-resolution CRFs run on `in_flight` worker streams under the next group's forwards (batch > 1: consecutive same-sized
    images share one batched CRF call) and end in the restricted MAP of dsrg_crf_map_select; otherwise the labels are the kernel's
    own restricted arg-max of the clamped probabilities.  ignore_below: pixels whose largest probability / marginal over all
    labels is below it get 255 (the reference's commented-out line 104); None: off.  At most 8 sizes and forward_batch in 1..16;
    flip=True: at most 4 sizes and forward_batch <= 8 (ValueError before any stream or worker exists).  The masks are
    predict_train_gt_ms's except where two labels all but tie.  masks="device": the (H,W) int32 CUDA tensors instead, nothing
    copied to the host (_mask_out has the contract)."""
    from . import ops
    sizes = tuple(int(S) for S in sizes)
    to_mask = _mask_out(masks)
    _check_ensemble(len(sizes), flip, forward_batch)
    if not 1 <= int(forward_batch) <= MAX_FORWARD_BATCH:
        raise ValueError("forward_batch must be 1..%d, got %d" % (MAX_FORWARD_BATCH, int(forward_batch)))

    def group_results():
        for group in _forward_groups(items, forward_batch):
            real = [it for it in group if it is not None]
            dev_images, xs = _group_inputs([None if it is None else it[0] for it in group], [(S, S) for S in sizes], device, forward,
                                           flip=flip, square=True)
            scores = _forwards(net, forward, xs)
            shapes = [(im.shape[0], im.shape[1]) for im in dev_images]
            select = [train_gt_selection(labels) for _, labels in real]
            if smooth:
                unaries = ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=0.00001, want="unary")
                for triple in zip(dev_images, unaries, select):
                    yield triple
            else:
                for lab in ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=0.00001, want="labels", select=select,
                                                       ignore_below=ignore_below):
                    yield lab

    if smooth:
        yield from _crf_in_flight(group_results(), device, in_flight, batch, ignore_below, masks=masks)
        return
    for lab in group_results():
        yield to_mask(lab)


class ConfusionMatrix(object):
    """evaluate.py:17-68 (rows = ground truth, columns = prediction, 255 ignored)."""

    def __init__(self, nclass, classes=None):
        self.nclass = nclass
        self.classes = classes
        self.M = np.zeros((nclass, nclass))

    def add(self, gt, pred):
        gt, pred = np.asarray(gt).ravel(), np.asarray(pred).ravel()
        assert np.max(pred) <= self.nclass
        assert len(gt) == len(pred)
        keep = gt != 255
        self.M += np.bincount(gt[keep].astype(np.int64) * self.nclass + pred[keep].astype(np.int64),
                              minlength=self.nclass ** 2).reshape(self.nclass, self.nclass)

    def add_device(self, gt, pred):
        """`add` for uint8 CUDA tensors: the histogram runs on the GPU (dsrg_confusion_matrix), M is updated on the host"""
        from . import ops
        h = ops.confusion_matrix(gt.reshape(-1), pred.reshape(-1), self.nclass).cpu().numpy()
        assert h[-1] == 0, "labels or predictions outside [0, nclass)"
        self.M += h[:-1].reshape(self.nclass, self.nclass).astype(np.float64)

    def add_counts(self, hist):
        """add nclass*nclass + 1 counters as ops.confusion_matrix / ops.eval_confusion_batch return them (a tensor or an array):
        the first nclass*nclass go to M; a non-zero last counter — labels outside [0, nclass) that the rule kept — raises, as
        `add` would (the reference asserts there are none)"""
        h = hist.detach().cpu().numpy() if hasattr(hist, "detach") else np.asarray(hist)
        h = h.reshape(-1)
        if h.size != self.nclass ** 2 + 1:
            raise ValueError("expected %d counters, got %d" % (self.nclass ** 2 + 1, h.size))
        if h[-1] != 0:
            raise ValueError("%d kept pixels carry a label outside [0, %d)" % (int(h[-1]), self.nclass))
        self.M += h[:-1].reshape(self.nclass, self.nclass).astype(np.float64)

    def generateM(self, item):
        """evaluate.py:61-68: the matrix of one (gt, pred) pair, keeping ground truth < nclass"""
        gt, pred = np.asarray(item[0]).ravel(), np.asarray(item[1]).ravel()
        assert len(gt) == len(pred)
        keep = gt < self.nclass
        return np.bincount(gt[keep].astype(np.int64) * self.nclass + pred[keep].astype(np.int64),
                           minlength=self.nclass ** 2).reshape(self.nclass, self.nclass).astype(np.float64)

    def addM(self, matrix):
        assert matrix.shape == self.M.shape
        self.M += matrix

    def recall(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.sum(np.diag(self.M) / np.sum(self.M, axis=0)) / self.nclass)

    def accuracy(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.sum(np.diag(self.M) / np.sum(self.M, axis=1)) / self.nclass)

    def jaccard(self):
        d = np.diag(self.M)
        per = [d[i] / (np.sum(self.M[i, :]) + np.sum(self.M[:, i]) - d[i]) for i in range(self.nclass) if d[i] != 0]
        return np.sum(per) / len(per), per, self.M


MAX_SCORE_GROUP = 16        # label maps per MaskScorer.add (the limit of dsrg_score_labels_batch)


class MaskScorer(object):
    """The confusion counters of device label maps (what the *_many generators yield with masks="device") against ground truth
    read on the host, kept on the device: test-coco.py:62-81,138-173's running confusion matrix without the label maps ever
    leaving the GPU.  rule_lt=True keeps ground truth < nclass (generateM, the rule of `python -m dsrg_amd.evaluate`), False
    ground truth != ignore_label (ConfusionMatrix.add).

    add() packs the ground truth of a group of up to 16 images into one of two pinned staging slots and uploads it with ONE copy
    (the idea of input._StagedLoader: a slot is rewritten only after the upload of the group before last, which an event marks,
    has finished — normally long ago, so the host does not wait), then scores the group with one dsrg_score_labels_batch launch
    on torch's current stream.  With want_masks that launch also narrows the label maps to bytes into one device buffer, which
    comes down with ONE copy (this the host waits for) and is returned as uint8 arrays: the PNG payloads.  Nothing else waits;
    counts() synchronises once."""

    def __init__(self, nclass, device, rule_lt=True, ignore_label=255, want_masks=False):
        self.nclass, self.device = int(nclass), torch.device(device)
        if not 1 <= self.nclass <= 96:
            raise ValueError("1..96 classes, got %d" % self.nclass)
        self.rule_lt, self.ignore_label, self.want_masks = bool(rule_lt), int(ignore_label), bool(want_masks)
        self.hist = torch.zeros(self.nclass * self.nclass + 1, dtype=torch.int64, device=self.device)
        self._stage, self._uploaded, self._turn = [None, None], [None, None], 0
        self._mask_stage = None

    @staticmethod
    def _pinned(buf, nbytes):
        """buf if it holds nbytes, else a larger pinned uint8 buffer (half as much again, so that a run's slots settle)"""
        if buf is not None and buf.numel() >= nbytes:
            return buf
        return torch.empty(nbytes + nbytes // 2, dtype=torch.uint8, pin_memory=True)

    def add(self, labels, gts):
        """labels: 1..16 (H,W) int32 CUDA label maps; gts: as many (H,W) uint8 arrays of the same sizes (a mismatch: ValueError
        before any copy or launch).  Adds the group to the counters; with want_masks returns the group's (H,W) uint8 masks as host
        arrays (copies: they stay valid), otherwise None"""
        from . import ops
        labels, gts = list(labels), [np.asarray(g) for g in gts]
        if not 1 <= len(labels) <= MAX_SCORE_GROUP or len(gts) != len(labels):
            raise ValueError("a group holds 1..%d label maps and as many ground truths, got %d and %d"
                             % (MAX_SCORE_GROUP, len(labels), len(gts)))
        for g, (lab, gt) in enumerate(zip(labels, gts)):
            if gt.dtype != np.uint8 or gt.ndim != 2 or tuple(gt.shape) != tuple(lab.shape):
                raise ValueError("ground truth %d is %s %s, its label map %s" % (g, gt.dtype, tuple(gt.shape), tuple(lab.shape)))
        sizes = [gt.size for gt in gts]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(offs[-1])
        k = self._turn
        self._turn ^= 1
        if self._uploaded[k] is not None:
            self._uploaded[k].synchronize()                  # the upload that last read this slot
        stage = self._stage[k] = self._pinned(self._stage[k], total)
        flat = stage.numpy()
        for gt, o in zip(gts, offs):
            flat[o:o + gt.size] = gt.reshape(-1)
        with torch.cuda.device(self.device):
            packed = torch.empty(total, dtype=torch.uint8, device=self.device)
            packed.copy_(stage[:total], non_blocking=True)
            self._uploaded[k] = torch.cuda.Event()
            self._uploaded[k].record()

            def views(buf):
                return [buf[o:o + n].reshape(tuple(lab.shape)) for lab, o, n in zip(labels, offs.tolist(), sizes)]

            narrowed = torch.empty(total, dtype=torch.uint8, device=self.device) if self.want_masks else None
            ops.score_labels_batch(labels, views(packed), self.nclass, self.ignore_label, self.rule_lt, hist=self.hist,
                                   masks=None if narrowed is None else views(narrowed))
            if narrowed is None:
                return None
            host = self._mask_stage = self._pinned(self._mask_stage, total)
            host[:total].copy_(narrowed, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return [a.copy() for a in views(host.numpy())]

    def counts(self):
        """the nclass*nclass + 1 counters so far as an int64 array; synchronises once"""
        return self.hist.cpu().numpy()

    def result(self, images):
        """validate.result_from_counts of the counters so far: dict(miou, iou, pixel_accuracy, images, matrix, counts), miou as
        ConfusionMatrix.jaccard gives it (the mean over the classes with a non-zero diagonal)"""
        from .validate import result_from_counts
        return result_from_counts(self.counts(), self.nclass, images)
