"""The training input pipelines of both stages: files -> device tensors ready for DSRGTrainer.step / RetrainTrainer.step.

  TrainSInput  <-> Caffe's ImageData layer (train-s.prototxt:3-22) + AnnotationLayer (pylayers.py:346-387)
  TrainFInput  <-> ImageSegDataLayer (layer.py:17-251; train-f.prototxt:3-14)
  TrainSCueMapInput <-> AnnotationLayerCOCO (pylayers.py:432-512): stage 1 fed by 'image_path cue_path' lists, the cue a small
                   label map (255 = no cue) — any class count up to MAX_CLASSES; order and mirror draws as TrainSInput's
  (validate.ValInput, the one finite pass, is the fourth loader on the same core)

The host decodes files (PIL, on a thread pool), packs the raw bytes of a batch — uint8 pixels, uint8 labels or cue maps, int32
cue triplets and class ids — into ONE pinned staging buffer and uploads it with one copy; the batch itself (resize, BGR, mean,
cue planes, image-level labels, crop, mirror) is assembled on the device by one launch (ops.train_s_input_batch,
ops.train_s_cuemap_input_batch, ops.train_f_input_batch).  Everything that decides WHAT a batch holds is plain host code that
needs no device, and there is one of each: the two-field list file (`read_list`), the epoch order and its sharding over ranks
(`epoch_items`), the staging layout (`_layout`: per image its pixels, then the feeder's further pieces, each on a 16-byte
boundary) and the write of a piece (`_put`) — the public layout_* / pack_* functions state their pieces over these two — and the
loader mechanics (`_StagedLoader`: slots, streams, the pool, the end of a finite pass, `stage_batch`).  A loader is a plan, a
decode, a layout, its `pack` routine, its `out_shapes` and its launch; `_StageOneLoader` and `_PairLoader` hold what the two
stage-1 feeders and the two feeders of image / label pairs share of these.

Random numbers.  Each loader owns its generators, the global ones are never touched.  TrainSInput: the epoch shuffle comes from a
`random.Random(seed)` — NOT Caffe's RNG, so a run does not see the reference's image order — and the mirror draws from an
`np.random.RandomState(seed)`, one `choice(2)` per image in batch order, 0 = mirror: AnnotationLayer's draws under
`np.random.seed(seed)`.  TrainFInput: BatchLoader's and SimpleTransformer.preprocess's draws in their order — per image (only with `scale_factors`: the
factor's index, `randrange`, first,) the row offset, the column offset (`random.Random(seed).randint`), the mirror (`RandomState(seed).choice(2)`), and `shuffle` from the same
`random.Random` between the last image of an epoch and the first of the next — so a run seeded like `random.seed(seed);
np.random.seed(seed)` sees the reference's crops.  With world_size > 1 the shuffle moves to a second `random.Random(seed)` that
does nothing else (see TrainFInput.__init__), so that every rank shuffles alike.  All draws are made on the iterating thread, never
in a worker.
"""
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .data import SimpleTransformer, _Window, check_scale_factors, scaled_size

MAX_BATCH = 32                                   # images per launch (dsrg_train_s_input_batch / dsrg_train_f_input_batch)
MAX_CLASSES = 96                                 # kMaxLabels of the library: the layer and CRF kernels keep at most this many labels


def _align(n):
    return (n + 15) & ~15                        # every piece of a staging buffer starts on a 16-byte boundary


def epoch_items(entries, shuffle, rng, rank=0, world_size=1):
    """the endless item stream of one rank: the list in file order for the first epoch, reshuffled (rng.shuffle, identically on every
    rank) before each later one when `shuffle`; a rank takes items rank, rank + world_size, ... of each epoch.  Batches are cut from
    this stream, so the list wraps mid-batch (as Caffe's ImageData and layer.py's BatchLoader do)."""
    entries = list(entries)
    if not 0 <= rank < world_size:
        raise ValueError("rank %d outside world size %d" % (rank, world_size))
    if len(entries) <= rank:
        raise ValueError("%d list entries leave rank %d of %d without an image" % (len(entries), rank, world_size))
    while True:
        for i in range(rank, len(entries), world_size):
            yield entries[i]
        if shuffle:
            rng.shuffle(entries)


def read_list(path, line_format, what, second=str):
    """the list file every loader reads: two fields per line (further fields and empty lines are skipped) -> [(first,
    second(second field))].  A line with one field raises ValueError naming the file and `line_format`, what a line should look
    like; so does a file without a line, naming `what` it should have listed."""
    out = []
    with open(path) as f:
        for line in f:
            parts = line.split()
            if parts:
                if len(parts) < 2:
                    raise ValueError("%s: expected '%s', got %r" % (path, line_format, line.strip()))
                out.append((parts[0], second(parts[1])))
    if not out:
        raise ValueError("%s lists no %s" % (path, what))
    return out


def read_train_s_list(path):
    """'name.jpg <id>' lines (the reference's list/input_list.txt) -> [(name, id)]"""
    return read_list(path, "name.jpg <id>", "image", int)


def read_pair_list(path):
    """'image_path cue_path' lines (AnnotationLayerCOCO's `source`) -> [(image_path, cue_path)]"""
    return read_list(path, "image_path cue_path", "image / cue map pair")


def read_rgb(path):
    """(H, W, 3) RGB uint8, contiguous"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def read_gray(path):
    """(H, W) uint8, contiguous"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8))


def image_size(path):
    """(H, W) from the file's header (nothing is decoded)"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def cue_arrays(cue_dict, image_id, num_classes=21, map_size=(41, 41)):
    """-> ((3, K) int32 cue triplets, (L,) int32 class ids) of one image, checked: a triplet outside the (num_classes, *map_size)
    planes or a class id outside [0, num_classes) raises ValueError (numpy's fancy indexing in AnnotationLayer would raise
    IndexError or wrap a negative index; the kernel's own guard only keeps bad data from writing out of bounds)"""
    cues = np.asarray(cue_dict['%i_cues' % image_id])
    cues = np.ascontiguousarray(cues.reshape(3, -1), dtype=np.int32)
    labels = np.ascontiguousarray(np.asarray(cue_dict['%i_labels' % image_id]).reshape(-1), dtype=np.int32)
    for axis, bound in enumerate((num_classes, map_size[0], map_size[1])):
        if cues.shape[1] and (cues[axis].min() < 0 or cues[axis].max() >= bound):
            raise ValueError("image %d: a cue triplet lies outside the %d x %d x %d planes" % ((image_id, num_classes) + tuple(map_size)))
    if labels.size and (labels.min() < 0 or labels.max() >= num_classes):
        raise ValueError("image %d: a class id lies outside [0, %d)" % (image_id, num_classes))
    return cues, labels


def _layout(shapes, pieces, mirror, **carried):
    """The one layout of a staging buffer: per image its (H, W, 3) image and then, in order, one piece per entry of `pieces` — (the
    descriptor's offset key, bytes per image) — each on a 16-byte boundary.  shapes: (H, W) per image; mirror: one flag per image
    or None (none mirrored); carried: further per-image lists of ints the descriptor holds as they are (counts, top / left, Hs /
    Ws) -> (bytes, desc): desc is the dict of per-image lists the batch's ops wrapper takes."""
    n = len(shapes)
    if not 1 <= n <= MAX_BATCH:
        raise ValueError("a batch holds 1..%d images, got %d" % (MAX_BATCH, n))
    carried["mirror"] = [0] * n if mirror is None else [bool(m) for m in mirror]
    for key, values in list(carried.items()) + list(pieces):
        if len(values) != n:
            raise ValueError("one %s entry per image, got %d for %d images" % (key, len(values), n))
    desc = dict(image_off=[], H=[int(H) for H, _ in shapes], W=[int(W) for _, W in shapes])
    desc.update((key, [int(v) for v in values]) for key, values in carried.items())
    desc.update((key, []) for key, _ in pieces)
    off = 0
    for b, (H, W) in enumerate(zip(desc["H"], desc["W"])):
        if H < 1 or W < 1:
            raise ValueError("an image of %d x %d pixels" % (H, W))
        desc["image_off"].append(off)
        off = _align(off + H * W * 3)
        for key, nbytes in pieces:
            if nbytes[b] < 0:
                raise ValueError("image %d: %s names a piece of %d bytes" % (b, key, nbytes[b]))
            desc[key].append(off)
            off = _align(off + nbytes[b])
    if off >= 1 << 31:
        raise ValueError("the staging buffer of one batch would hold %d >= 2^31 bytes" % off)
    return off, desc


def _put(buf, desc, key, arrays, dtype, shape, what):
    """The one put of a piece: array b of `arrays`, which must have exactly `dtype` and `shape(b)`, goes as raw bytes to offset
    desc[key][b] of buf (a 1-d uint8 numpy array of at least the layout's size); nothing else of buf is written."""
    if len(arrays) != len(desc[key]):
        raise ValueError("%d %ss for %d images" % (len(arrays), what, len(desc[key])))
    for b, a in enumerate(arrays):
        if a.dtype != dtype or a.shape != shape(b):
            raise ValueError("%s %d must be %s %s" % (what, b, shape(b), np.dtype(dtype).name))
        o = desc[key][b]
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)


def _put_images(buf, desc, images):
    _put(buf, desc, "image_off", images, np.uint8, lambda b: (desc["H"][b], desc["W"][b], 3), "image")


def layout_train_s(shapes, ncues, nlabels, mirror=None):
    """where the pieces of a stage-1 batch lie in its staging buffer.  shapes: (H, W) per image; ncues / nlabels: triplets / class
    ids per image -> (bytes, desc): desc is the dict of per-image lists ops.train_s_input_batch takes."""
    return _layout(shapes, [("cue_off", [12 * int(K) for K in ncues]), ("label_off", [4 * int(L) for L in nlabels])], mirror,
                   ncues=ncues, nlabels=nlabels)


def pack_train_s(buf, desc, images, cues, labels):
    """write the batch's raw bytes into buf (1-d uint8 numpy array, at least the layout's size): images (H, W, 3) uint8 RGB, cues
    (3, K) int32, labels (L,) int32 (cues and labels: anything numpy converts to int32 with that many values)"""
    flat = lambda arrays: [np.asarray(a, dtype=np.int32).reshape(-1) for a in arrays]        # noqa: E731
    _put_images(buf, desc, images)
    _put(buf, desc, "cue_off", flat(cues), np.int32, lambda b: (3 * desc["ncues"][b],), "cue triplet array")
    _put(buf, desc, "label_off", flat(labels), np.int32, lambda b: (desc["nlabels"][b],), "class id array")


def check_cue_map(cue, num_classes, map_size, ignore_label=255, name="cue map"):
    """a decoded cue map is what dsrg_train_s_cuemap_input_batch takes: (Hm, Wm) uint8 of exactly map_size (cue maps are never
    resampled, as in AnnotationLayerCOCO) whose bytes are classes below num_classes or ignore_label (the layer's one-hot scatter
    would raise IndexError on any other; the kernel's own guard only keeps bad data in bounds).  ValueError names `name`."""
    if cue.dtype != np.uint8 or cue.ndim != 2:
        raise ValueError("%s: a cue map must be a 2-d uint8 array, got %s %s" % (name, cue.dtype, cue.shape))
    if tuple(cue.shape) != (int(map_size[0]), int(map_size[1])):
        raise ValueError("%s: the cue map is %d x %d, the net's map is %d x %d (cue maps are not resampled)"
                         % ((name,) + tuple(cue.shape) + (int(map_size[0]), int(map_size[1]))))
    bad = (cue >= num_classes) & (cue != ignore_label)
    if bad.any():
        raise ValueError("%s: cue value %d is neither one of %d classes nor the ignore label %d"
                         % (name, int(cue[bad].min()), num_classes, ignore_label))


def layout_train_s_cuemap(shapes, map_size, mirror=None):
    """where the pieces of a cue-map stage-1 batch lie in its staging buffer.  shapes: (H, W) per image; map_size: the (Hm, Wm)
    every cue map has -> (bytes, desc): desc is the dict of per-image lists ops.train_s_cuemap_input_batch takes (and Hm, Wm)."""
    Hm, Wm = int(map_size[0]), int(map_size[1])
    if Hm < 1 or Wm < 1:
        raise ValueError("a cue map of %d x %d pixels" % (Hm, Wm))
    nbytes, desc = _layout(shapes, [("cue_off", [Hm * Wm] * len(shapes))], mirror)
    desc.update(Hm=Hm, Wm=Wm)
    return nbytes, desc


def pack_train_s_cuemap(buf, desc, images, cue_maps):
    """write the batch's raw bytes into buf: images (H, W, 3) uint8 RGB, cue maps (Hm, Wm) uint8"""
    _put_images(buf, desc, images)
    _put(buf, desc, "cue_off", cue_maps, np.uint8, lambda b: (desc["Hm"], desc["Wm"]), "cue map")


def layout_train_f(shapes, top, left, mirror, scaled=None):
    """where the pieces of a stage-2 batch lie in its staging buffer.  shapes: (H, W) per image; top / left / mirror: the host's
    draws; scaled: (Hs, Ws) per image, the size each is rescaled to before the crop (top / left are then offsets on the rescaled
    image), or None -> (bytes, desc): desc is the dict of per-image lists ops.train_f_input_batch takes; with `scaled` it holds
    Hs and Ws too.  The bytes are the same either way: the source image is what is staged."""
    rescaled = {}
    if scaled is not None:
        if len(scaled) != len(shapes) or min([1] + [min(s) for s in scaled]) < 1:
            raise ValueError("one rescaled size >= 1 x 1 per image, got %r" % (list(scaled),))
        rescaled = dict(Hs=[s[0] for s in scaled], Ws=[s[1] for s in scaled])
    if min([0] + [int(v) for v in list(top) + list(left)]) < 0:
        raise ValueError("negative crop offset")
    return _layout(shapes, [("label_off", [H * W for H, W in shapes])], mirror, top=top, left=left, **rescaled)


def pack_train_f(buf, desc, images, labels):
    """write the batch's raw bytes into buf: images (H, W, 3) uint8 RGB, labels (H, W) uint8, each the size of its image"""
    _put_images(buf, desc, images)
    _put(buf, desc, "label_off", labels, np.uint8, lambda b: (desc["H"][b], desc["W"][b]), "label")


class _Slot(object):
    """one staging slot: a pinned host buffer and a device buffer of the same size (grown only when a batch needs more), the
    slot's own output tensors, and the events that order its reuse"""

    def __init__(self, torch, outputs):
        self.pinned = self.host = self.dev = None
        self.outputs = outputs
        self.copied = torch.cuda.Event()          # side stream: the upload has left the pinned buffer
        self.ready = torch.cuda.Event()           # side stream: the batch is assembled
        self.free = torch.cuda.Event()            # caller's stream: the caller's work on the slot's previous batch is enqueued before it
        self.in_flight = False
        self.desc, self.nbytes = None, 0
        self.count = 0                            # images of the batch staged here; 0: the plan was empty, nothing is staged


class _StagedLoader(object):
    """The mechanics every loader shares.  Two staging slots; per __next__ call n (0-based), on the calling thread:
      1. batch n — uploaded during call n-1 — is assembled by ONE launch on the loader's side stream, behind an event recorded
         on the caller's current stream (the caller's work on batch n-2, this slot's previous tenant, is in front of it), and the
         caller's stream is made to wait for the assembly;
      2. batch n+1 — decoding on the pool since call n-1 — is collected in list order, packed into the OTHER slot's pinned
         buffer and uploaded (non_blocking) on the side stream: it runs under the caller's step on batch n;
      3. the files of batch n+2 are handed to the pool.
    CONTRACT: the tensors of batch n are valid until the __next__ call after next (call n+2 hands their slot to batch n+2); a
    caller that keeps a batch longer clones it.  A call that raises (a file that does not decode, say) closes the loader: later
    calls raise RuntimeError.  No stream is left current across calls: every `with torch.cuda.stream` block
    closes inside the call that opens it.
    A FINITE pass: a loader whose plan_batch returns [] once its items are used up.  An empty plan stages nothing and marks its
    slot empty; the __next__ call that would return it raises StopIteration, which closes the loader like any other exception.
    The endless loaders never plan an empty batch."""

    def __init__(self, batch_size, workers, device):
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError("batch_size must be 1..%d, got %d" % (MAX_BATCH, self.batch_size))
        self.workers = int(workers)
        if self.workers < 1:
            raise ValueError("workers must be >= 1")
        self.device = device
        self._pool = self._side = self._slots = self._decoding = None
        self._count = 0
        self._closed = False

    # -- what a loader defines -------------------------------------------------------------------------------------------------
    pack = None                                   # staticmethod(pack_*): (buf, desc, *pieces) writes the batch's bytes

    def plan_batch(self):                         # iterating thread: the next batch's items with every random draw made
        raise NotImplementedError

    def _decode(self, item):                      # worker thread: files -> arrays
        raise NotImplementedError

    def _layout(self, plan, arrays):              # -> (bytes, desc, pieces to pack)
        raise NotImplementedError

    def out_shapes(self):                         # the shapes of a slot's float32 output tensors
        raise NotImplementedError

    def _assemble(self, slot):                    # one launch on the current (side) stream -> the tuple __next__ returns
        raise NotImplementedError

    # -- mechanics -------------------------------------------------------------------------------------------------------------
    def stage_batch(self):
        """-> (bytes, desc, pieces) of the next batch: planned, decoded and laid out on the calling thread, with no device touched —
        what an upload does before its first device call, every refusal of a bad file included.  Advances the loader's item
        stream and random draws like the batch it stands for; (0, None, ()) past the end of a finite pass."""
        plan = self.plan_batch()
        return self._layout(plan, [self._decode(item) for item in plan]) if plan else (0, None, ())

    def _submit(self):
        plan = self.plan_batch()
        return plan, [self._pool.submit(self._decode, item) for item in plan]

    def _upload(self, pending, slot):
        import torch
        plan, futures = pending
        slot.count = len(plan)
        if not plan:                                                    # the end of a finite pass
            return
        arrays = [f.result() for f in futures]                          # in list order, whatever order the workers finished in
        nbytes, desc, pieces = self._layout(plan, arrays)
        if slot.in_flight:
            slot.copied.synchronize()                                   # the slot's previous upload has left the pinned buffer
        if slot.pinned is None or slot.pinned.numel() < nbytes:
            cap = (nbytes + (1 << 20) - 1) & ~((1 << 20) - 1)
            slot.pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            slot.host = slot.pinned.numpy()
            with torch.cuda.stream(self._side):                         # (allocated and freed in the side stream's order)
                slot.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
        self.pack(slot.host, desc, *pieces)
        with torch.cuda.stream(self._side):
            slot.dev[:nbytes].copy_(slot.pinned[:nbytes], non_blocking=True)
            slot.copied.record(self._side)
        slot.in_flight = True
        slot.desc, slot.nbytes = desc, nbytes

    def _start(self):
        import torch
        from . import _lib
        _lib.require_gpu()
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(self.device)
        self._pool = ThreadPoolExecutor(self.workers)
        with torch.cuda.device(self.device):
            self._side = torch.cuda.Stream(device=self.device)
            self._slots = [_Slot(torch, tuple(torch.empty(shape, dtype=torch.float32, device=self.device) for shape in self.out_shapes()))
                           for _ in range(2)]
            self._upload(self._submit(), self._slots[0])
        self._decoding = self._submit()

    def __iter__(self):
        return self

    def __next__(self):
        if self._closed:
            raise RuntimeError("the loader is closed")
        try:
            return self._advance()
        except BaseException:
            # a file that does not decode, a bad cue, a failed launch: the batch this call was about to return may be assembled
            # and the one behind it half staged — no retry could be told apart from a fresh call, so the loader ends here
            self.close()
            raise

    def _advance(self):
        import torch
        if self._slots is None:
            self._start()
        n = self._count
        slot = self._slots[n % 2]
        if slot.count == 0:                                             # the plan of this batch was empty: the pass is over
            raise StopIteration
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            slot.free.record(cur)
            self._side.wait_event(slot.free)
            with torch.cuda.stream(self._side):
                out = self._assemble(slot)
                slot.ready.record(self._side)
            cur.wait_event(slot.ready)
            self._upload(self._decoding, self._slots[(n + 1) % 2])
        self._decoding = self._submit()
        self._count = n + 1
        return out

    def close(self):
        """join the pool, wait for the side stream; the tensors already returned stay valid (nothing overwrites them any more)"""
        if self._closed:
            return
        self._closed = True
        if self._pool is not None:
            if self._decoding is not None:
                for f in self._decoding[1]:
                    f.cancel()
            self._pool.shutdown(wait=True)
        if self._side is not None:
            self._side.synchronize()
        self._pool = self._decoding = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class _StageOneLoader(_StagedLoader):
    """What the two stage-1 feeders share: the item stream (`epoch_items` under a random.Random(seed)), the mirror draw (one
    RandomState(seed).choice(2) per image in batch order, 0 = mirror; none drawn when `mirror` is off) and the three outputs
    (images (B,3,Sh,Sw), labels (B,1,1,C), cues (B,C,Hm,Wm)).  A feeder sets num_classes, size (an int or (Sh, Sw)) and map_size,
    calls _open_stream with its list, and defines _item: a list entry -> the plan's dict for it (it may validate and raise)."""

    def _open_stream(self, entries, mirror, shuffle, seed, rank, world_size):
        self.entries, self.mirror = entries, bool(mirror)
        self._items = epoch_items(self.entries, shuffle, random.Random(seed), rank, world_size)
        self._mirror_rng = np.random.RandomState(seed)

    def _item(self, first, second):
        raise NotImplementedError

    def plan_batch(self):
        plan = []
        for _ in range(self.batch_size):
            item = self._item(*next(self._items))
            item["mirror"] = self.mirror and int(self._mirror_rng.choice(2)) == 0
            plan.append(item)
        return plan

    def out_shapes(self):
        B, C, (Hm, Wm) = self.batch_size, self.num_classes, self.map_size
        Sh, Sw = self.size if isinstance(self.size, tuple) else (self.size, self.size)
        return (B, 3, Sh, Sw), (B, 1, 1, C), (B, C, Hm, Wm)


class TrainSInput(_StageOneLoader):
    """Iterator of (images (B,3,size,size), labels (B,1,1,21), cues (B,21,41,41)) float32 device tensors for DSRGTrainer.step:
    Caffe's ImageData layer (train-s.prototxt:3-22: read, resize to size x size, mean 104/117/123, shuffle) followed by
    AnnotationLayer (pylayers.py:346-387), assembled on the device by ops.train_s_input_batch.

    list_file: 'name.jpg <id>' lines, the image is root/name; cues: the localisation-cue pickle (layers._open_cue_file) or its
    dictionary.  Epochs: file order first, reshuffled before each later epoch when `shuffle` (a random.Random(seed) of the loader's
    own: not Caffe's RNG); the list wraps mid-batch; with world_size > 1 every rank shuffles identically and takes items rank,
    rank + world_size, ... of the epoch.  Mirror: one RandomState(seed).choice(2) per image in batch order, 0 = mirror
    (AnnotationLayer's draw).  The tensors of batch n are valid until the __next__ call after next (_StagedLoader)."""

    num_classes, map_size, mean = 21, (41, 41), (104.0, 117.0, 123.0)
    pack = staticmethod(pack_train_s)

    def __init__(self, list_file, root, cues, batch_size=20, size=321, mirror=True, shuffle=True, seed=0, workers=8, rank=0,
                 world_size=1, device=None):
        _StagedLoader.__init__(self, batch_size, workers, device)
        self.size, self.root = int(size), root
        if isinstance(cues, dict):
            self.cues = cues
        else:
            from .layers import _open_cue_file
            self.cues = _open_cue_file(os.path.abspath(cues))
        self._open_stream(read_train_s_list(list_file), mirror, shuffle, seed, rank, world_size)
        self._checked = {}

    def _cues_of(self, image_id):
        if image_id not in self._checked:
            self._checked[image_id] = cue_arrays(self.cues, image_id, self.num_classes, self.map_size)
        return self._checked[image_id]

    def _item(self, name, image_id):
        self._cues_of(image_id)                                         # a bad triplet raises here, before any upload
        return dict(name=name, id=image_id)

    def _decode(self, item):
        return read_rgb(os.path.join(self.root, item["name"]))

    def _layout(self, plan, arrays):
        anno = [self._cues_of(item["id"]) for item in plan]
        cues, labels = [a[0] for a in anno], [a[1] for a in anno]
        nbytes, desc = layout_train_s([a.shape[:2] for a in arrays], [c.shape[1] for c in cues], [l.size for l in labels],
                                      [item["mirror"] for item in plan])
        return nbytes, desc, (arrays, cues, labels)

    def _assemble(self, slot):
        from . import ops
        return ops.train_s_input_batch(slot.dev, slot.desc, self.size, self.num_classes, self.map_size, self.mean,
                                       out=slot.outputs, nbytes=slot.nbytes)


class TrainSCueMapInput(_StageOneLoader):
    """Iterator of (images (B,3,Sh,Sw), labels (B,1,1,C), cues (B,C,Hm,Wm)) float32 device tensors for DSRGTrainer.step:
    AnnotationLayerCOCO (pylayers.py:432-512), the feeder of the 81-class runs, assembled on the device by
    ops.train_s_cuemap_input_batch.

    list_file: 'image_path cue_path' lines; `root` is prefixed to both as it stands (as TrainFInput and the layer do).  A cue file
    is a one-channel image of exactly map_size = (Sh // 8 + 1, Sw // 8 + 1) — the layer's top[1]; cue maps are never resampled —
    whose bytes are classes below num_classes or ignore_label (no cue); the image-level labels are the classes the map names
    (class 0 is not forced on; a map without a cue gives all zeros).  size: an int or (h, w): the images are zoomed to it
    (scipy.ndimage.zoom, order 1).  bgr: the channel order of the network input — True, B G R with `mean` in that order, is what
    every other pipeline of this project feeds the net; False is the layer's own R G B (`mean` is always in the OUTPUT order).
    Epochs: file order first, reshuffled after each pass when `shuffle` (the layer's order, from a random.Random(seed) of the
    loader's own); the list wraps mid-batch; with world_size > 1 every rank shuffles identically and takes items rank, rank +
    world_size, ... of the epoch.  Mirror: one RandomState(seed).choice(2) per image in batch order, 0 = mirror (the layer's
    choice(2) * 2 - 1).  A cue file of another size or with a byte that is neither a class nor ignore_label raises ValueError
    naming the file when its batch is laid out, before any upload.  The tensors of batch n are valid until the __next__ call
    after next (_StagedLoader)."""

    pack = staticmethod(pack_train_s_cuemap)

    def __init__(self, list_file, root, num_classes, batch_size=20, size=321, mean=(104.0, 117.0, 123.0), mirror=True,
                 ignore_label=255, bgr=True, shuffle=True, seed=0, workers=8, rank=0, world_size=1, device=None):
        _StagedLoader.__init__(self, batch_size, workers, device)
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError("num_classes must be 1..%d, got %d" % (MAX_CLASSES, self.num_classes))
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if min(self.size) < 1:
            raise ValueError("size %r" % (size,))
        self.map_size = (self.size[0] // 8 + 1, self.size[1] // 8 + 1)
        self.ignore_label = int(ignore_label)
        if not 0 <= self.ignore_label <= 255:
            raise ValueError("ignore_label must be a byte value, got %d" % self.ignore_label)
        if len(mean) != 3:
            raise ValueError("mean must hold 3 values")
        self.mean, self.bgr, self.root = tuple(float(m) for m in mean), bool(bgr), root
        self._open_stream(read_pair_list(list_file), mirror, shuffle, seed, rank, world_size)

    def _item(self, image_path, cue_path):
        return dict(image=self.root + image_path, cue=self.root + cue_path)

    def _decode(self, item):
        return read_rgb(item["image"]), read_gray(item["cue"])

    def _layout(self, plan, arrays):
        images, cue_maps = [a[0] for a in arrays], [a[1] for a in arrays]
        for item, cue in zip(plan, cue_maps):                           # a bad cue file raises here, before any upload
            check_cue_map(cue, self.num_classes, self.map_size, self.ignore_label, item["cue"])
        nbytes, desc = layout_train_s_cuemap([a.shape[:2] for a in images], self.map_size, [item["mirror"] for item in plan])
        return nbytes, desc, (images, cue_maps)

    def _assemble(self, slot):
        from . import ops
        return ops.train_s_cuemap_input_batch(slot.dev, slot.desc, self.size, self.num_classes, self.map_size, self.mean,
                                              self.ignore_label, self.bgr, out=slot.outputs, nbytes=slot.nbytes)


class _PairLoader(_StagedLoader):
    """What the feeders of 'image_path label_path' lists share (TrainFInput, validate.ValInput): the decode, the stage-2 layout
    and the two outputs (data (B,3,ch,cw), label (B,1,ch,cw)).  A feeder sets `crop` and plans items that hold image, label, top,
    left and mirror (and Hs, Ws where the image is rescaled first)."""

    pack = staticmethod(pack_train_f)

    def _decode(self, item):
        return read_rgb(item["image"]), read_gray(item["label"])

    def _layout(self, plan, arrays):
        images, labels = [a[0] for a in arrays], [a[1] for a in arrays]
        scaled = [(it["Hs"], it["Ws"]) for it in plan] if plan and "Hs" in plan[0] else None
        nbytes, desc = layout_train_f([a.shape[:2] for a in images], [it["top"] for it in plan], [it["left"] for it in plan],
                                      [it["mirror"] for it in plan], scaled)
        return nbytes, desc, (images, labels)

    def out_shapes(self):
        B, (ch, cw) = self.batch_size, self.crop
        return (B, 3, ch, cw), (B, 1, ch, cw)


class TrainFInput(_PairLoader):
    """Iterator of (data (B,3,ch,cw), label (B,1,ch,cw)) float32 device tensors for RetrainTrainer.step: ImageSegDataLayer
    (layer.py:17-251), assembled on the device by ops.train_f_input_batch.

    params: the layer's param dict — source ('image_path label_path' lines), root_folder (prefixed to both as it stands),
    batch_size, crop_size, mean, scale, mirror, phase, ignore_label; what is left out takes SimpleTransformer.check_params'
    defaults.  List order and reshuffling are BatchLoader's, the draws SimpleTransformer.preprocess's, in its order per image: row
    offset, column offset (phase 'Train' only), mirror choice (with `mirror` only) — from a random.Random(seed) and an
    np.random.RandomState(seed) of the loader's own.  `scale_factors` (default (): none; finite, > 0): in phase 'Train' each image
    is first rescaled by one of them — `randrange(len(scale_factors))` from the offsets' generator, drawn before the row offset —
    to data.scaled_size of its size, bilinearly (8 bit) for the image and by nearest neighbour for the label, and the window is
    the rescaled image's; the device does the rescaling inside the same launch, the staged bytes are the source image's.  An image's size is read from its label file's header when the batch is
    planned, so the draws never wait for a decode.  With world_size > 1 every rank shuffles identically — from a second
    random.Random(seed) that only shuffles, since the offsets' generator advances by amounts that depend on each rank's own images —
    and takes items rank, rank + world_size, ... of the epoch; the crops are then no longer the single-process run's.  The tensors of batch n are valid until the __next__ call after next (_StagedLoader)."""

    def __init__(self, params, seed=0, workers=8, rank=0, world_size=1, device=None):
        params = dict(params)
        SimpleTransformer.check_params(params)
        _StagedLoader.__init__(self, params['batch_size'], workers, device)
        self.params = params
        self.crop = (int(params['crop_size'][0]), int(params['crop_size'][1]))
        if min(self.crop) < 1:
            raise ValueError("crop_size %r" % (params['crop_size'],))
        self.mean, self.scale = tuple(float(np.float32(m)) for m in params['mean']), float(np.float32(params['scale']))
        self.is_mirror, self.phase, self.ignore_label = bool(params['mirror']), params['phase'], params['ignore_label']
        self.root_folder = params['root_folder']
        self.scale_factors = check_scale_factors(params['scale_factors'])
        self.entries = read_list(params['source'], "image_path label_path", "image / label pair")
        self._rng = random.Random(seed)
        self._np_rng = np.random.RandomState(seed)
        # One process: BatchLoader's shuffle, from the generator the crop offsets come from.  Several ranks: `randint` takes a
        # number of words from its generator that depends on the range, i.e. on the sizes of the images a rank draws for, so the
        # ranks' offset generators drift apart within an epoch — the shuffle then has a generator of its own, which every rank
        # advances alike: the shards stay disjoint and jointly the epoch.
        shuffle_rng = self._rng if world_size == 1 else random.Random(seed)
        self._items = epoch_items(self.entries, True, shuffle_rng, rank, world_size)

    def plan_batch(self):
        plan = []
        for _ in range(self.batch_size):
            image_path, label_path = next(self._items)                  # (reshuffles between two epochs, from the offsets' generator)
            image_path, label_path = self.root_folder + image_path, self.root_folder + label_path
            size, rescaled = image_size(label_path), {}
            if self.scale_factors and self.phase == 'Train':             # first draw of the image; the window is the rescaled image's
                k = self._rng.randrange(len(self.scale_factors))
                size = scaled_size(size[0], size[1], self.scale_factors[k])
                rescaled = dict(factor=k, Hs=size[0], Ws=size[1])
            win = _Window(size, self.crop)
            top, left = win.top, win.left                               # centred unless drawn
            if self.phase == 'Train':
                max_top, max_left = win.slack()
                top = self._rng.randint(0, max_top)
                left = self._rng.randint(0, max_left)
            mirror = self.is_mirror and int(self._np_rng.choice(2)) == 0
            plan.append(dict(image=image_path, label=label_path, top=top, left=left, mirror=mirror, **rescaled))
        return plan

    def _assemble(self, slot):
        from . import ops
        return ops.train_f_input_batch(slot.dev, slot.desc, self.crop, self.mean, self.scale, self.ignore_label, out=slot.outputs,
                                       nbytes=slot.nbytes)
