"""The GPU training input pipeline (dsrg_amd/csrc/train_input.hip, dsrg_amd/input.py) and `python -m dsrg_amd.train`.

CPU: the argument checks of dsrg_train_s_input_batch / dsrg_train_f_input_batch, the numpy restatement of the 8-bit bilinear resize
(written from the formula in DESIGN.md, not from the kernel), the loaders' order / sharding / draws / packing, the command's
arguments.
GPU: both kernels against the restatement, the host AnnotationLayer and SimpleTransformer.preprocess; both loaders end to end
against the host composition; the command in a child process.  Everything is integer arithmetic or a fixed sequence of float32
operations: bitwise equality throughout."""
import ctypes
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced
MEAN = (104.0, 117.0, 123.0)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- the numpy restatement of the resize ------------------------------------------------------------------------------------------
def _taps(n, S, zero_at_border):
    """source index, the two 11-bit weights and the clamp flags of every output coordinate on an axis of n source samples"""
    d = np.arange(S, dtype=np.float64)
    scale = 1.0 / (float(S) / float(n))
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= n - 1
    if zero_at_border:
        f = np.where(lo | hi, np.float32(0.0), f).astype(np.float32)
        s = np.clip(s, 0, n - 1)
    w1 = np.clip(np.rint(f * np.float32(2048.0)), -32768, 32767).astype(np.int32)
    w0 = np.clip(np.rint((np.float32(1.0) - f) * np.float32(2048.0)), -32768, 32767).astype(np.int32)
    return s, w0, w1, lo, hi


def resize_ref(src, S, stats=None):
    """(H, W, 3) uint8 -> (S, S, 3) int32: the 8-bit bilinear resize as DESIGN.md states it"""
    H, W = src.shape[:2]
    sx, a0, a1, xlo, xhi = _taps(W, S, True)
    sy, b0, b1, _, _ = _taps(H, S, False)
    x0, x1 = sx, np.minimum(sx + 1, W - 1)
    y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
    p = src.astype(np.int32)
    D = p[:, x0, :] * a0[None, :, None] + p[:, x1, :] * a1[None, :, None]            # (H, S, 3), int32
    D0, D1 = D[y0], D[y1]
    out = (((b0[:, None, None] * (D0 >> 4)) >> 16) + ((b1[:, None, None] * (D1 >> 4)) >> 16) + 2) >> 2
    if stats is not None:
        four = (a0 != 0)[None, :] & (a1 != 0)[None, :] & (b0 != 0)[:, None] & (b1 != 0)[:, None]
        stats["four"] = stats.get("four", 0) + int(four.sum())
        stats["pixels"] = stats.get("pixels", 0) + S * S
        for key, hit in (("left", xlo.any()), ("right", xhi.any()), ("top", (sy < 0).any()), ("bottom", (sy + 1 > H - 1).any())):
            stats[key] = stats.get(key, False) or bool(hit)
    return out.astype(np.int32)


def images_ref(sources, S, mean, mirror, stats=None):
    """-> (B, 3, S, S) float32: resize, BGR, float(pixel) - mean, mirror"""
    out = np.empty((len(sources), 3, S, S), np.float32)
    for b, src in enumerate(sources):
        r = resize_ref(src, S, stats)
        for c in range(3):
            out[b, c] = r[:, :, 2 - c].astype(np.float32) - np.float32(mean[c])
        if mirror[b]:
            out[b] = out[b][:, :, ::-1]
    return out


class _Blob(object):
    def __init__(self, a=None):
        self.data = a if a is not None else np.zeros((0,), np.float32)

    def reshape(self, *s):
        self.data = np.zeros(s, np.float32)


def annotation_ref(cue_path, ids, images, mirror, seed):
    """the host AnnotationLayer (pylayers.py:346-387) on the ids / images under np.random.seed(seed) -> labels, cues, images"""
    import pylayers
    lay = pylayers.AnnotationLayer()
    lay.param_str = "{'cues': %r, 'mirror': %s}" % (cue_path, bool(mirror))
    bottoms = [_Blob(np.asarray(ids, np.float32).reshape(-1, 1, 1, 1)), _Blob(images)]
    tops = [_Blob(), _Blob(), _Blob()]
    lay.setup(bottoms, tops)
    lay.reshape(bottoms, tops)
    state = np.random.get_state()
    try:
        if seed is not None:
            np.random.seed(seed)
        lay.forward(bottoms, tops)
    finally:
        if seed is not None:
            np.random.set_state(state)
    return tops[0].data, tops[1].data, tops[2].data


def _cue_dict(rng, ids, K=40):
    data = {}
    for i in ids:
        data['%i_labels' % i] = np.array(sorted(rng.choice(np.arange(1, 21), size=2, replace=False)))
        data['%i_cues' % i] = np.stack([rng.integers(0, 21, K), rng.integers(0, 41, K), rng.integers(0, 41, K)])
    return data


def _write_s_files(tmp_path, rng, n=5, sizes=((37, 53), (53, 37), (33, 33), (20, 45), (64, 31))):
    """n PNGs, a list file and a cue pickle -> (list path, image dir, pickle path, ids, names)"""
    from PIL import Image
    d = tmp_path / "JPEGImages"
    d.mkdir()
    ids = [11 + 3 * k for k in range(n)]
    names = ["im%d.png" % k for k in range(n)]
    for name, (H, W) in zip(names, sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(d / name))
    lst = tmp_path / "input_list.txt"
    lst.write_text("".join("%s %d\n" % (nm, i) for nm, i in zip(names, ids)))
    cues = tmp_path / "cues.pickle"
    with open(str(cues), "wb") as f:
        pickle.dump(_cue_dict(rng, ids), f, protocol=2)
    return str(lst), str(d), str(cues), ids, names


def _write_f_files(tmp_path, rng, sizes=((10, 9), (30, 40), (12, 30), (40, 8), (17, 13))):
    """PNG image / label pairs and a list file -> (list path, root folder)"""
    from PIL import Image
    lines = []
    for k, (H, W) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(tmp_path / ("im%d.png" % k)))
        Image.fromarray(rng.integers(0, 21, (H, W), dtype=np.uint8), mode="L").save(str(tmp_path / ("lab%d.png" % k)))
        lines.append("/im%d.png /lab%d.png\n" % (k, k))
    lst = tmp_path / "train.txt"
    lst.write_text("".join(lines))
    return str(lst), str(tmp_path)


# ---- CPU: argument checks -----------------------------------------------------------------------------------------------------------
def test_train_s_input_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(*MEAN)

    def call(B=3, stage=_FAKE, nbytes=4096, off="d", H="d", W="d", coff="d", nc="d", loff="d", nl="d", mir="d", S=5, C=21, Hm=41,
             Wm=41, mean=mean3, images=_FAKE, cues=_FAKE, labels=_FAKE):
        n = max(B, 1)
        d = lambda v, dflt: _i32(dflt) if isinstance(v, str) else v                    # noqa: E731
        return L.dsrg_train_s_input_batch(B, stage, nbytes, d(off, [256 * b for b in range(n)]), d(H, [4] * n), d(W, [5] * n),
                                          d(coff, [1024 + 64 * b for b in range(n)]), d(nc, [5] * n),
                                          d(loff, [3072 + 16 * b for b in range(n)]), d(nl, [2] * n), d(mir, [0] * n), S, C, Hm, Wm,
                                          mean, images, cues, labels, None)

    E = _lib.ERR_INVALID
    assert call(B=0) == E and b"images" in L.dsrg_last_error()
    assert call(B=33) == E and b"32" in L.dsrg_last_error()
    assert call(stage=None) == E and b"NULL" in L.dsrg_last_error()
    for name in ("off", "H", "W", "coff", "nc", "loff", "nl", "mir", "mean", "images", "cues", "labels"):
        assert call(**{name: None}) == E and b"NULL" in L.dsrg_last_error(), name
    for name in ("images", "cues", "labels"):
        assert call(**{name: 258}) == E and b"aligned" in L.dsrg_last_error(), name
    for name in ("S", "C", "Hm", "Wm"):
        assert call(**{name: 0}) == E, name
    assert call(H=_i32([4, 0, 4])) == E and call(W=_i32([5, 5, 0])) == E
    assert call(off=_i32([0, 256, 4096 - 59])) == E and b"outside" in L.dsrg_last_error()         # 60 bytes from 4037
    assert call(off=_i32([0, -4, 512])) == E and b"outside" in L.dsrg_last_error()
    assert call(coff=_i32([1024, 1088, 4096 - 56])) == E and b"outside" in L.dsrg_last_error()     # 60 bytes of triplets
    assert call(coff=_i32([1024, 1090, 1152])) == E and b"aligned" in L.dsrg_last_error()
    assert call(loff=_i32([3072, 3088, 4092])) == E and b"outside" in L.dsrg_last_error()
    assert call(loff=_i32([3072, 3089, 3104])) == E and b"aligned" in L.dsrg_last_error()
    assert call(nc=_i32([5, -1, 5])) == E and call(nl=_i32([2, 2, -1])) == E
    assert call(nbytes=100) == E and b"outside" in L.dsrg_last_error()
    U = _lib.ERR_UNSUPPORTED
    assert call(nbytes=1 << 31) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=32, S=4800) == U and b"2^31" in L.dsrg_last_error()                              # 32 * 3 * 4800^2
    assert call(B=32, C=1 << 12, Hm=128, Wm=128) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=1, H=_i32([32768]), W=_i32([32768])) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=32, nbytes=1 << 16, C=1 << 19, Hm=1, Wm=1) == U and b"2^24" in L.dsrg_last_error()               # 2^24 planes: a grid of 2^32 threads
    if not torch.cuda.is_available():                                                             # everything in order: only the device is missing
        assert call(B=32, nbytes=1 << 16, C=(1 << 19) - 1, Hm=1, Wm=1) == _lib.ERR_HIP                            # (2^24 - 32 planes + 4 pixel blocks)
        assert call() == _lib.ERR_HIP and L.dsrg_last_error()
        assert call(nc=_i32([0, 5, 5])) == _lib.ERR_HIP                                           # (an image without cues is fine)


def test_train_f_input_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(*MEAN)

    def call(B=3, stage=_FAKE, nbytes=4096, off="d", loff="d", H="d", W="d", top="d", left="d", mir="d", ch=17, cw=13, mean=mean3,
             data=_FAKE, label=_FAKE):
        n = max(B, 1)
        d = lambda v, dflt: _i32(dflt) if isinstance(v, str) else v                    # noqa: E731
        return L.dsrg_train_f_input_batch(B, stage, nbytes, d(off, [256 * b for b in range(n)]), d(loff, [2048 + 64 * b for b in range(n)]),
                                          d(H, [4] * n), d(W, [5] * n), d(top, [0] * n), d(left, [1] * n), d(mir, [0] * n), ch, cw, mean,
                                          1.0, 255.0, data, label, None)

    E = _lib.ERR_INVALID
    assert call(B=0) == E and b"images" in L.dsrg_last_error()
    assert call(B=33) == E and b"32" in L.dsrg_last_error()
    assert call(stage=None) == E and b"NULL" in L.dsrg_last_error()
    for name in ("off", "loff", "H", "W", "top", "left", "mir", "mean", "data", "label"):
        assert call(**{name: None}) == E and b"NULL" in L.dsrg_last_error(), name
    for name in ("data", "label"):
        assert call(**{name: 258}) == E and b"aligned" in L.dsrg_last_error(), name
    assert call(ch=0) == E and call(cw=0) == E
    assert call(H=_i32([4, 0, 4])) == E and call(W=_i32([5, 5, 0])) == E
    assert call(top=_i32([0, -1, 0])) == E and b"negative" in L.dsrg_last_error()
    assert call(left=_i32([0, 0, -1])) == E and b"negative" in L.dsrg_last_error()
    assert call(off=_i32([0, 256, 4096 - 59])) == E and b"outside" in L.dsrg_last_error()
    assert call(off=_i32([-1, 256, 512])) == E and b"outside" in L.dsrg_last_error()
    assert call(loff=_i32([2048, 2112, 4096 - 19])) == E and b"outside" in L.dsrg_last_error()     # 20 label bytes from 4077
    assert call(nbytes=100) == E and b"outside" in L.dsrg_last_error()
    U = _lib.ERR_UNSUPPORTED
    assert call(nbytes=1 << 31) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=32, ch=4800, cw=4800) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=1, H=_i32([32768]), W=_i32([32768])) == U and b"2^31" in L.dsrg_last_error()
    if not torch.cuda.is_available():
        assert call() == _lib.ERR_HIP and L.dsrg_last_error()
        assert call(top=_i32([0, 500, 0])) == _lib.ERR_HIP                                         # (a crop wholly off the image is fine)


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------
def test_resize_restatement_identity_constant_and_a_hand_computed_case():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (33, 33, 3), dtype=np.uint8)
    assert np.array_equal(resize_ref(src, 33), src.astype(np.int32))                   # H = W = S: every pixel comes through
    for H, W, S, v in ((5, 9, 33, 255), (37, 53, 33, 1), (53, 37, 9, 200), (1, 1, 7, 77), (120, 90, 321, 254)):
        assert np.array_equal(resize_ref(np.full((H, W, 3), v, np.uint8), S), np.full((S, S, 3), v, np.int32)), (H, W, S, v)
    # 2 x 2 -> 3 x 3 by hand.  x: dx = 0 has fx = -1/6 (clamped: weights 2048, 0), dx = 1 has fx = 1/2 (1024, 1024), dx = 2 has
    # sx = 1 = W - 1 (2048, 0 on column 1).  y: dy = 0 has sy = -1, fy = 5/6 -> (b0, b1) = (341, 1707) on rows (0, 0); dy = 1 has
    # (1024, 1024) on rows (0, 1); dy = 2 has sy = 1, fy = 1/6 -> (1707, 341) on rows (1, 1).
    # row sums >> 4 of [[10, 200], [90, 255]]: row 0 -> 1280, 13440, 25600; row 1 -> 11520, 22080, 32640
    #   dy = 0: (341*1280 >> 16) + (1707*1280 >> 16) + 2 = 6 + 33 + 2 = 41 >> 2 = 10;  69 + 350 + 2 = 421 >> 2 = 105;  133 + 666 + 2 >> 2 = 200
    #   dy = 1: 20 + 180 + 2 = 202 >> 2 = 50;  210 + 345 + 2 = 557 >> 2 = 139;  400 + 510 + 2 = 912 >> 2 = 228
    #   dy = 2: 300 + 59 + 2 = 361 >> 2 = 90;  575 + 114 + 2 = 691 >> 2 = 172;  850 + 169 + 2 = 1021 >> 2 = 255
    one = np.array([[10, 200], [90, 255]], np.uint8)
    src = np.stack([one, one.T, 255 - one], axis=2)
    want = np.array([[10, 105, 200], [50, 139, 228], [90, 172, 255]], np.int32)
    got = resize_ref(src, 3)
    assert np.array_equal(got[:, :, 0], want)
    sx, a0, a1, _, _ = _taps(2, 3, True)
    sy, b0, b1, _, _ = _taps(2, 3, False)
    assert sx.tolist() == [0, 0, 1] and a0.tolist() == [2048, 1024, 2048] and a1.tolist() == [0, 1024, 0]
    assert sy.tolist() == [-1, 0, 1] and b0.tolist() == [341, 1024, 1707] and b1.tolist() == [1707, 1024, 341]
    # the transposed channel [[10, 90], [200, 255]]: its corners come through and its centre is the same four-pixel blend
    assert got[1, 1, 1] == 139 and got[0, 0, 1] == 10 and got[0, 2, 1] == 90 and got[2, 0, 1] == 200 and got[2, 2, 1] == 255


# ---- CPU: loader logic -----------------------------------------------------------------------------------------------------------
def test_epoch_order_wraps_mid_batch_and_ranks_share_an_epoch(tmp_path):
    from dsrg_amd import input as I
    entries = list(range(5))
    it = I.epoch_items(entries, True, random.Random(7))
    got = [next(it) for _ in range(15)]
    r = random.Random(7)
    e1 = list(entries)
    r.shuffle(e1)
    e2 = list(e1)
    r.shuffle(e2)
    assert got == entries + e1 + e2                                                    # file order first, reshuffled before each later epoch
    it = I.epoch_items(entries, False, random.Random(7))
    assert [next(it) for _ in range(12)] == (entries * 3)[:12]
    # ranks: identical shuffles, items rank, rank + world, ...: disjoint and jointly the epoch
    entries = list(range(11))
    streams = [I.epoch_items(entries, True, random.Random(3), rank, 3) for rank in range(3)]
    per_epoch = [len(range(rank, 11, 3)) for rank in range(3)]
    r = random.Random(3)
    epoch = list(entries)
    for _ in range(3):
        shards = [[next(s) for _ in range(n)] for s, n in zip(streams, per_epoch)]
        assert [shard == epoch[rank::3] for rank, shard in enumerate(shards)] == [True] * 3
        assert sorted(sum(shards, [])) == entries and len(set(sum(shards, []))) == 11
        r.shuffle(epoch)
    with pytest.raises(ValueError):
        next(I.epoch_items([1, 2], True, random.Random(0), 2, 3))
    # the loader cuts batches from the stream: batch 2 of 5 images wraps in the third batch
    rng = np.random.default_rng(5)
    lst, root, cues, ids, names = _write_s_files(tmp_path, rng)
    ld = I.TrainSInput(lst, root, cues, batch_size=2, size=33, shuffle=False, seed=0)
    plans = [ld.plan_batch() for _ in range(5)]
    assert [[it["id"] for it in p] for p in plans] == [ids[0:2], ids[2:4], [ids[4], ids[0]], ids[1:3], ids[3:5]]
    assert [it["name"] for it in plans[2]] == [names[4], names[0]]
    ld.close()


def test_train_s_mirror_flags_are_annotation_layers_flips(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(6)
    lst, root, cues, ids, _ = _write_s_files(tmp_path, rng)
    seed = 4
    ld = I.TrainSInput(lst, root, cues, batch_size=5, size=33, shuffle=False, seed=seed)
    flags = [[it["mirror"] for it in ld.plan_batch()] for _ in range(3)]
    assert any(sum(flags, [])) and not all(sum(flags, []))
    # AnnotationLayer under np.random.seed(seed): an image whose columns differ shows each flip
    images = np.tile(np.arange(7, dtype=np.float32), (5, 3, 7, 1))
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        for k in range(3):
            out = annotation_ref(cues, ids, images, True, None)[2]
            assert [bool(out[b, 0, 0, 0] == 6.0) for b in range(5)] == flags[k]
    finally:
        np.random.set_state(state)
    plain = I.TrainSInput(lst, root, cues, batch_size=5, size=33, mirror=False, seed=seed)
    assert not any(it["mirror"] for it in plain.plan_batch())


def test_train_f_draws_are_simple_transformers(tmp_path, monkeypatch):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    rng = np.random.default_rng(8)
    lst, root = _write_f_files(tmp_path, rng)
    real_randint, real_choice = random.randint, np.random.choice
    for phase, mirror in (("Train", True), ("Train", False), ("Test", True)):
        params = dict(source=lst, root_folder=root, batch_size=3, crop_size=(17, 13), mean=MEAN, mirror=mirror, phase=phase)
        seed = 9
        ld = I.TrainFInput(params, seed=seed)
        plans = [it for _ in range(5) for it in ld.plan_batch()]                       # 15 images: 3 epochs
        got = [(it["image"], it["top"], it["left"], it["mirror"]) for it in plans]
        # the reference's draws: BatchLoader + SimpleTransformer.preprocess under the global generators, every draw recorded
        want, drawn = [], []
        monkeypatch.setattr(random, "randint", lambda lo, hi: drawn.append(real_randint(lo, hi)) or drawn[-1])
        monkeypatch.setattr(np.random, "choice", lambda n: drawn.append(real_choice(n)) or drawn[-1])
        states = random.getstate(), np.random.get_state()
        random.seed(seed)
        np.random.seed(seed)
        try:
            bl = D.BatchLoader(dict(params))
            for _ in range(15):
                image_path, label_path = next(bl._epochs)
                del drawn[:]
                out_img, out_lab = bl.transformer.preprocess(D._imread_bgr(image_path), D._imread_gray(label_path))
                want.append((image_path, list(drawn), out_img, out_lab))
        finally:
            random.setstate(states[0])
            np.random.set_state(states[1])
            monkeypatch.undo()
        assert [g[0] for g in got] == [w[0] for w in want]                               # list order and reshuffles
        for it, (_, draws, ref_img, ref_lab) in zip(plans, want):
            mine = ([it["top"], it["left"]] if phase == "Train" else []) + ([0 if it["mirror"] else 1] if mirror else [])
            assert mine == [int(v) for v in draws]                                      # the same draws in the same order
            img, lab = D._imread_bgr(it["image"]), D._imread_gray(it["label"])            # ... and they place the reference's crop
            win = D._Window(lab.shape, (17, 13), it["top"], it["left"])
            x = (np.asarray(img, np.float32) - np.asarray(MEAN, np.float32)) * np.float32(1.0)
            mine_img, mine_lab = win.cut(x, 0.0).transpose(2, 0, 1), win.cut(lab, 255)
            if it["mirror"]:
                mine_img, mine_lab = mine_img[:, :, ::-1], mine_lab[:, ::-1]
            assert np.array_equal(mine_img, ref_img) and np.array_equal(mine_lab, ref_lab)
        if phase == "Test":
            assert all(g[1:3] == ((max(H, 17) - 17) // 2, (max(W, 13) - 13) // 2)
                       for g, (H, W) in zip(got, ((10, 9), (30, 40), (12, 30))))
        if not mirror:
            assert not any(g[3] for g in got)
    assert ld.params["ignore_label"] == 255 and ld.scale == 1.0                        # check_params' defaults


def test_train_f_ranks_share_every_epoch(tmp_path):
    """phase 'Train' with images of many sizes: the ranks' offset generators advance by different amounts (randint's rejection loop
    depends on each image's slack), and the shards must stay disjoint and jointly the epoch all the same"""
    from dsrg_amd import input as I
    rng = np.random.default_rng(12)
    sizes = [(int(h), int(w)) for h, w in zip(rng.integers(5, 90, 12), rng.integers(5, 90, 12))]
    lst, root = _write_f_files(tmp_path, rng, sizes=sizes)
    everything = sorted(root + "/im%d.png" % k for k in range(12))
    for world in (2, 3):
        params = dict(source=lst, root_folder=root, batch_size=12 // world, crop_size=(17, 13), mean=MEAN, mirror=True, phase="Train")
        ranks = [I.TrainFInput(params, seed=1, rank=r, world_size=world) for r in range(world)]
        epochs = []
        for epoch in range(4):
            shards = [[it["image"] for it in ld.plan_batch()] for ld in ranks]            # one batch per rank = one epoch
            seen = sum(shards, [])
            assert len(set(seen)) == 12 and sorted(seen) == everything, (world, epoch)
            epochs.append(seen)
        assert epochs[0] == [root + "/im%d.png" % k for r in range(world) for k in range(r, 12, world)]   # file order first
        assert len(set(map(tuple, epochs))) == 4                                          # ... and reshuffled after it
        draws = [[(it["top"], it["left"]) for it in ld.plan_batch()] for ld in ranks]
        assert len(set(map(tuple, draws))) == world                                       # (the ranks do draw differently)


def test_packing_layouts_and_bad_cues(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(10)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in ((3, 5), (1, 1), (4, 2))]
    cues = [rng.integers(0, 21, (3, K)).astype(np.int32) for K in (7, 0, 2)]
    labels = [np.array(v, np.int32) for v in ([3, 1], [], [20])]
    nbytes, desc = I.layout_train_s([im.shape[:2] for im in images], [c.shape[1] for c in cues], [l.size for l in labels], [0, 1, 0])
    buf = np.full(nbytes + 8, 0xAB, np.uint8)
    I.pack_train_s(buf, desc, images, cues, labels)
    assert (buf[nbytes:] == 0xAB).all() and desc["mirror"] == [0, 1, 0]
    spans = []
    for b in range(3):
        o = desc["image_off"][b]
        assert np.array_equal(buf[o:o + images[b].size].reshape(images[b].shape), images[b])
        spans.append((o, images[b].size))
        o = desc["cue_off"][b]
        assert o % 4 == 0 and np.array_equal(buf[o:o + 12 * desc["ncues"][b]].view(np.int32).reshape(3, -1), cues[b])
        spans.append((o, 12 * desc["ncues"][b]))
        o = desc["label_off"][b]
        assert o % 4 == 0 and np.array_equal(buf[o:o + 4 * desc["nlabels"][b]].view(np.int32), labels[b])
        spans.append((o, 4 * desc["nlabels"][b]))
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= nbytes
    lab8 = [rng.integers(0, 21, im.shape[:2], dtype=np.uint8) for im in images]
    nbytes, desc = I.layout_train_f([im.shape[:2] for im in images], [0, 2, 1], [1, 0, 0], [True, False, True])
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_f(buf, desc, images, lab8)
    for b in range(3):
        o = desc["label_off"][b]
        assert np.array_equal(buf[o:o + lab8[b].size].reshape(lab8[b].shape), lab8[b])
    with pytest.raises(ValueError):
        I.pack_train_f(buf, desc, images, [lab8[0], lab8[1], lab8[2][:, :1]])              # a label of another size than its image
    with pytest.raises(ValueError):
        I.layout_train_f([(3, 5)], [-1], [0], [False])
    with pytest.raises(ValueError):
        I.layout_train_s([(3, 5)] * 33, [0] * 33, [0] * 33)
    # a cue triplet outside the planes raises before anything is uploaded
    good = {'7_labels': np.array([2, 5]), '7_cues': np.array([[2, 5], [0, 40], [40, 0]])}
    c, l = I.cue_arrays(good, 7)
    assert c.dtype == np.int32 and c.shape == (3, 2) and l.tolist() == [2, 5]
    for bad in ([[21], [0], [0]], [[1], [41], [0]], [[1], [0], [41]], [[1], [0], [-1]], [[-1], [0], [0]]):
        with pytest.raises(ValueError):
            I.cue_arrays({'7_labels': np.array([2]), '7_cues': np.array(bad)}, 7)
    with pytest.raises(ValueError):
        I.cue_arrays({'7_labels': np.array([21]), '7_cues': np.zeros((3, 0), int)}, 7)
    lst, root, cue_path, ids, _ = _write_s_files(tmp_path, rng)
    data = pickle.load(open(cue_path, "rb"))
    data['%i_cues' % ids[1]][2, 3] = 41
    ld = I.TrainSInput(lst, root, data, batch_size=2, size=33)
    with pytest.raises(ValueError):
        ld.plan_batch()


# ---- CPU: the command ------------------------------------------------------------------------------------------------------------
def _run_train(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


def test_train_command_help_and_solver_defaults():
    out = _run_train(["--help"], timeout=120)
    for word in ("--stage", "--list", "--root", "--weights", "--snapshot", "--prefix", "--iters", "--snapshot-every", "--batch", "--seed",
                 "--display", "--workers", "--cues", "--backbone", "--crop", "--mean", "--no-mirror"):
        assert word in out, word
    from dsrg_amd import train as T
    s = T.parse_args(["--stage", "s", "--list", "l", "--root", "r", "--cues", "c"])
    assert (s.iters, s.snapshot_every, s.display, s.prefix, s.batch, s.seed) == (8000, 8000, 10, "models/model-s", 20, 0)
    f = T.parse_args(["--stage", "f", "--list", "l", "--root", "r"])
    assert (f.iters, f.snapshot_every, f.display, f.prefix, f.batch, f.seed) == (20000, 10000, 20, "models/model-f", 10, 0)
    assert (f.backbone, f.crop, f.mean, f.no_mirror) == ("vgg16", 321, (104.0, 117.0, 123.0), False)
    f = T.parse_args(["--stage", "f", "--list", "l", "--root", "r", "--mean", "104.008,116.669,122.675", "--crop", "65", "--no-mirror",
                      "--backbone", "resnet101", "--iters", "7"])
    assert (f.backbone, f.crop, f.mean, f.no_mirror, f.iters) == ("resnet101", 65, (104.008, 116.669, 122.675), True, 7)
    for bad in (["--stage", "s", "--list", "l", "--root", "r"],                              # no cues
                ["--stage", "s", "--list", "l", "--root", "r", "--cues", "c", "--crop", "65"],
                ["--stage", "f", "--list", "l", "--root", "r", "--cues", "c"],
                ["--stage", "f", "--list", "l", "--root", "r", "--batch", "0"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
SOURCES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (37, 53), (53, 37), (33, 33))
ODD_MEAN = (104.008, 116.669, 122.675)


def _run_s_kernel(sources, cues, labels, mirror, S, C=21, map_size=(41, 41), mean=MEAN):
    from dsrg_amd import input as I
    from dsrg_amd import ops
    nbytes, desc = I.layout_train_s([s.shape[:2] for s in sources], [c.shape[1] for c in cues], [l.size for l in labels], mirror)
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_s(buf, desc, sources, cues, labels)
    stage = torch.from_numpy(buf).cuda()
    out = ops.train_s_input_batch(stage, desc, S, C, map_size, mean)
    again = ops.train_s_input_batch(stage, desc, S, C, map_size, mean, out=[torch.full_like(o, 7.0) for o in out])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, again))                           # every element is written, whatever was there
    return [o.cpu().numpy() for o in out]


@pytest.mark.gpu
def test_train_s_kernel_resize_mean_bgr_equals_the_restatement():
    rng = np.random.default_rng(20)
    srcs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SOURCES]
    none_c, none_l = np.zeros((3, 0), np.int32), np.zeros(0, np.int32)
    stats = {}
    images_ref(srcs[:-1], 33, ODD_MEAN, [False] * 7, stats)                             # the restatement's own data, non-identity sources
    print("S = 33: %d of %d pixels blend with four non-zero weights; clamps %s"
          % (stats["four"], stats["pixels"], {k: stats[k] for k in ("left", "right", "top", "bottom")}))
    assert 2 * stats["four"] > stats["pixels"]
    assert stats["left"] and stats["right"] and stats["top"] and stats["bottom"]
    cases = [(srcs, 33, [b % 2 == 1 for b in range(8)]), (srcs, 9, [b % 3 == 0 for b in range(8)]), ([srcs[5]], 33, [True]),
             ([srcs[4]], 9, [False]), ([srcs[b % 8] for b in range(20)], 33, [(b // 3) % 2 == 0 for b in range(20)]),
             ([rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)], 321, [True])]
    for sources, S, mirror in cases:
        B = len(sources)
        images, labels, cues = _run_s_kernel(sources, [none_c] * B, [none_l] * B, mirror, S, mean=ODD_MEAN)
        want = images_ref(sources, S, ODD_MEAN, mirror)
        bad = int((images != want).sum())
        print("B = %d, S = %d: %d of %d values differ from the restatement" % (B, S, bad, want.size))
        assert images.shape == want.shape and bad == 0
        assert not cues.any() and np.array_equal(labels.reshape(B, -1), np.eye(21, dtype=np.float32)[[0] * B])
    # integer mean: every value is an integer minus the mean, and the identity source comes through
    images, _, _ = _run_s_kernel([srcs[7]], [none_c], [none_l], [False], 33)
    assert np.array_equal(images[0], srcs[7][:, :, ::-1].transpose(2, 0, 1).astype(np.float32) - np.asarray(MEAN, np.float32)[:, None, None])


@pytest.mark.gpu
def test_train_s_kernel_cues_and_labels_equal_the_host_annotation_layer(tmp_path):
    rng = np.random.default_rng(21)
    ids = [5, 9, 12, 30, 31, 44]
    data = _cue_dict(rng, ids, K=300)
    data['9_cues'] = np.zeros((3, 0), dtype=np.int64)                                    # an image with no cues
    data['9_labels'] = np.zeros(0, dtype=np.int64)
    dup = np.array([[3, 3, 3, 7, 7], [4, 4, 4, 0, 0], [0, 0, 40, 40, 40]])               # duplicates, columns 0 and 40
    data['12_cues'], data['30_cues'] = np.concatenate([data['12_cues'], dup], 1), dup
    data['12_labels'], data['30_labels'] = np.array([17, 9, 3]), np.array([20, 7, 3, 1])  # descending order
    path = str(tmp_path / "cues.pickle")
    with open(path, "wb") as f:
        pickle.dump(data, f, protocol=2)
    from dsrg_amd import input as I
    srcs = [rng.integers(0, 256, (6, 8, 3), dtype=np.uint8) for _ in ids]
    anno = [I.cue_arrays(data, i) for i in ids]
    for seed in (0, 3):
        np_state = np.random.RandomState(seed)
        mirror = [int(np_state.choice(2)) == 0 for _ in ids]
        for flags in (mirror, [False] * len(ids), [True] * len(ids)):
            images, labels, cues = _run_s_kernel(srcs, [a[0] for a in anno], [a[1] for a in anno], flags, 9)
            host_images = images_ref(srcs, 9, MEAN, [False] * len(ids))
            if flags is mirror:
                want_l, want_c, want_i = annotation_ref(path, ids, host_images, True, seed)
            else:                                                                       # no draw: mirror none / mirror by hand
                want_l, want_c, want_i = annotation_ref(path, ids, host_images, False, None)
                if flags[0]:
                    want_c, want_i = want_c[..., ::-1], want_i[..., ::-1]
            assert np.array_equal(labels, want_l) and np.array_equal(cues, want_c) and np.array_equal(images, want_i)
            assert cues[1].sum() == 0 and labels[1].reshape(-1).tolist() == [1.0] + [0.0] * 20
    assert any(mirror) and not all(mirror)
    # a second geometry against plain numpy: C = 5, 7 x 3 planes
    K = 25
    cue = [np.stack([rng.integers(0, 5, K), rng.integers(0, 7, K), rng.integers(0, 3, K)]).astype(np.int32) for _ in range(3)]
    lab = [np.array(v, np.int32) for v in ([4, 2], [], [1])]
    flags = [True, False, True]
    _, labels, cues = _run_s_kernel(srcs[:3], cue, lab, flags, 9, C=5, map_size=(7, 3))
    want_c, want_l = np.zeros((3, 5, 7, 3), np.float32), np.zeros((3, 1, 1, 5), np.float32)
    for b in range(3):
        want_c[b, cue[b][0], cue[b][1], cue[b][2]] = 1.0
        want_l[b, 0, 0, 0] = 1.0
        want_l[b, 0, 0, lab[b]] = 1.0
        if flags[b]:
            want_c[b] = want_c[b][:, :, ::-1]
    assert np.array_equal(cues, want_c) and np.array_equal(labels, want_l)
    # the kernel's guard: a triplet outside the planes writes nothing (the loaders raise before they get here)
    wild = np.array([[1, 5, 2, -1, 2], [2, 0, 7, 0, 0], [1, 0, 0, 0, 3]], np.int32)
    _, _, cues = _run_s_kernel(srcs[:1], [wild], [lab[1]], [False], 9, C=5, map_size=(7, 3))
    want = np.zeros((1, 5, 7, 3), np.float32)
    want[0, 1, 2, 1] = 1.0
    assert np.array_equal(cues, want)


def _f_cases(rng):
    """(image RGB, label, top, left, mirror) at crop 17 x 13: smaller in both, larger in both, mixed; offsets 0 and the slack"""
    out = []
    for H, W in ((10, 9), (30, 40), (12, 30), (40, 8), (17, 13), (18, 14)):
        img, lab = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 21, (H, W), dtype=np.uint8)
        max_top, max_left = max(H, 17) - 17, max(W, 13) - 13
        for top, left, mirror in ((0, 0, False), (max_top, max_left, True), (max_top // 2, 0, True), (0, max_left, False)):
            out.append((img, lab, top, left, mirror))
    return out


@pytest.mark.gpu
def test_train_f_kernel_equals_simple_transformer_preprocess(monkeypatch):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    from dsrg_amd import ops
    rng = np.random.default_rng(22)
    cases = _f_cases(rng)
    assert len(cases) == 24
    crop = (17, 13)
    nbytes, desc = I.layout_train_f([c[0].shape[:2] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_f(buf, desc, [c[0] for c in cases], [c[1] for c in cases])
    stage = torch.from_numpy(buf).cuda()
    for scale, ignore in ((1.0, 255), (0.0039, 21)):
        data, label = ops.train_f_input_batch(stage, desc, crop, ODD_MEAN, scale, ignore)
        data, label = data.cpu().numpy(), label.cpu().numpy()
        tr = D.SimpleTransformer(dict(crop_size=crop, mean=ODD_MEAN, scale=scale, mirror=True, phase='Train', ignore_label=ignore))
        for b, (img, lab, top, left, mirror) in enumerate(cases):
            draws = iter([top, left])
            monkeypatch.setattr(D.random, "randint", lambda lo, hi: next(draws))       # the host's draws, fed to the reference
            monkeypatch.setattr(D.np.random, "choice", lambda n: 0 if mirror else 1)
            want_d, want_l = tr.preprocess(img[:, :, ::-1], lab)
            assert np.array_equal(data[b], want_d) and np.array_equal(label[b, 0], want_l), (b, scale)
        monkeypatch.undo()
    # phase 'Test': the centred window, no offset draws
    tr = D.SimpleTransformer(dict(crop_size=crop, mean=ODD_MEAN, scale=0.0039, mirror=False, phase='Test', ignore_label=21))
    imgs, labs = [c[0] for c in cases[::4]], [c[1] for c in cases[::4]]
    wins = [D._Window(l.shape, crop) for l in labs]
    nbytes, desc = I.layout_train_f([l.shape for l in labs], [w.top for w in wins], [w.left for w in wins], [False] * len(labs))
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_f(buf, desc, imgs, labs)
    data, label = ops.train_f_input_batch(torch.from_numpy(buf).cuda(), desc, crop, ODD_MEAN, 0.0039, 21)
    for b, (img, lab) in enumerate(zip(imgs, labs)):
        want_d, want_l = tr.preprocess(img[:, :, ::-1], lab)
        assert np.array_equal(data[b].cpu().numpy(), want_d) and np.array_equal(label[b, 0].cpu().numpy(), want_l)


@pytest.mark.gpu
def test_train_s_input_end_to_end_equals_the_host_composition(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(23)
    lst, root, cue_path, ids, names = _write_s_files(tmp_path, rng)
    seed = 2
    entries = list(zip(names, ids))
    order = I.epoch_items(entries, True, random.Random(seed))
    state = np.random.get_state()
    np.random.seed(seed)                                                                # AnnotationLayer's generator, across the batches
    kept = []
    try:
        with I.TrainSInput(lst, root, cue_path, batch_size=2, size=33, seed=seed, workers=3) as ld:
            for n in range(5):                                                          # two epochs and a wrap
                got = next(ld)
                batch = [next(order) for _ in range(2)]
                host = images_ref([I.read_rgb(os.path.join(root, nm)) for nm, _ in batch], 33, MEAN, [False, False])
                want_l, want_c, want_i = annotation_ref(cue_path, [i for _, i in batch], host, True, None)
                for g, w in zip(got, (want_i, want_l, want_c)):
                    assert g.is_cuda and g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), w), n
                if kept:                                                                # the slot contract: batch n-1 is still batch n-1
                    assert all(torch.equal(t, c) for t, c in zip(*kept)), n
                kept = (got, [t.clone() for t in got])
        assert all(torch.equal(t, c) for t, c in zip(*kept))                            # close() leaves the returned tensors alone
        assert torch.cuda.current_stream() == torch.cuda.default_stream()               # no stream state left behind
    finally:
        np.random.set_state(state)


@pytest.mark.gpu
def test_a_failed_decode_closes_the_loader(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(27)
    lst, root, cue_path, ids, names = _write_s_files(tmp_path, rng)
    os.remove(os.path.join(root, names[2]))
    ld = I.TrainSInput(lst, root, cue_path, batch_size=1, size=33, shuffle=False, workers=2)
    first = next(ld)                                                                    # batch 0; batch 1 uploaded, batch 2 decoding
    kept = [t.clone() for t in first]
    with pytest.raises(FileNotFoundError):
        next(ld)                                                                        # collecting batch 2 fails
    with pytest.raises(RuntimeError):
        next(ld)                                                                        # no retry: the loader is closed
    assert all(torch.equal(t, c) for t, c in zip(first, kept))
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


@pytest.mark.gpu
def test_train_f_input_end_to_end_equals_image_seg_data_layer(tmp_path):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    rng = np.random.default_rng(24)
    lst, root = _write_f_files(tmp_path, rng)
    params = dict(source=lst, root_folder=root, batch_size=2, crop_size=(17, 13), mean=ODD_MEAN, scale=0.0039, mirror=True, ignore_label=21)
    seed = 5
    layer = D.ImageSegDataLayer()
    layer.param_str = repr(params)
    tops = [_Blob(), _Blob()]
    states = random.getstate(), np.random.get_state()
    random.seed(seed)
    np.random.seed(seed)
    kept = []
    try:
        layer.setup([], tops)
        with I.TrainFInput(params, seed=seed, workers=3) as ld:
            for n in range(5):
                got = next(ld)
                layer.forward([], tops)
                for g, top in zip(got, tops):
                    assert g.is_cuda and g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), top.data), n
                if kept:
                    assert all(torch.equal(t, c) for t, c in zip(*kept)), n
                kept = (got, [t.clone() for t in got])
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
    finally:
        random.setstate(states[0])
        np.random.set_state(states[1])


def _losses(out):
    import re
    rows = [ln for ln in out.splitlines() if ln.startswith("Iteration ")]
    values = [float(v) for ln in rows for v in re.findall(r"loss[-\w]* = ([-+.\dnaife]+)", ln)]
    return rows, values


def _done(out):
    ln = [ln for ln in out.splitlines() if ln.startswith("done: ")][-1].split()
    return int(ln[2]), (int(ln[4]), int(ln[5]))


@pytest.mark.gpu
def test_train_command_stage_s_in_a_child_process(tmp_path):
    rng = np.random.default_rng(25)
    lst, root, cues, _, _ = _write_s_files(tmp_path, rng)
    common = ["--stage", "s", "--list", lst, "--root", root, "--cues", cues, "--iters", "2", "--batch", "2", "--display", "1",
              "--snapshot-every", "1", "--workers", "2", "--seed", "3"]
    first = _run_train(common + ["--prefix", str(tmp_path / "a" / "model-s")], timeout=600)
    rows, values = _losses(first)
    assert len(rows) == 2 and len(values) == 4 and np.isfinite(values).all(), first[-2000:]
    for it in (1, 2):
        assert (tmp_path / "a" / ("model-s_iter_%d.caffemodel" % it)).is_file()
        assert (tmp_path / "a" / ("model-s_iter_%d.solverstate.pt" % it)).is_file()
    again = _run_train(common + ["--prefix", str(tmp_path / "b" / "model-s")], timeout=600)
    assert _done(first)[0] == 2 and _done(again) == _done(first)                         # same seed, same weights, bit for bit
    resumed = _run_train(common + ["--prefix", str(tmp_path / "c" / "model-s"), "--snapshot",
                                   str(tmp_path / "a" / "model-s_iter_1.solverstate.pt")], timeout=600)
    assert "resumed" in resumed and _done(resumed)[0] == 2 and len(_losses(resumed)[0]) == 1
    assert (tmp_path / "c" / "model-s_iter_2.caffemodel").is_file() and not (tmp_path / "c" / "model-s_iter_1.caffemodel").exists()


@pytest.mark.gpu
def test_train_command_stage_f_in_a_child_process(tmp_path):
    rng = np.random.default_rng(26)
    lst, root = _write_f_files(tmp_path, rng, sizes=((70, 90), (50, 80), (66, 65), (100, 60), (65, 65)))
    common = ["--stage", "f", "--list", lst, "--root", root, "--iters", "2", "--batch", "2", "--display", "1", "--crop", "65",
              "--snapshot-every", "1", "--workers", "2", "--seed", "3"]
    first = _run_train(common + ["--prefix", str(tmp_path / "a" / "model-f")], timeout=600)
    rows, values = _losses(first)
    assert len(rows) == 2 and len(values) == 2 and np.isfinite(values).all(), first[-2000:]
    assert (tmp_path / "a" / "model-f_iter_2.caffemodel").is_file() and (tmp_path / "a" / "model-f_iter_2.solverstate.pt").is_file()
    assert _done(first)[0] == 2
