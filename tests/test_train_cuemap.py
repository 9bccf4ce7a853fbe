"""Stage-1 training fed by cue maps (AnnotationLayerCOCO's format) and `python -m dsrg_amd.train --class / --cue-maps`.

CPU: the argument checks of dsrg_train_s_cuemap_input_batch, the staging layout and packing, the loader's refusals, its order and
mirror draws, and the new options of the train command.
GPU: the launch against ops.preprocess_rect_batch and a float64 numpy restatement (bgr = 1), against
layers.AnnotationLayerCOCO.preprocess (bgr = 0; cue planes and image-level labels exactly), the loader end to end, and the train
command of both stages at 81 classes in child processes."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FAKE = 256                                                           # a "device pointer" that is never dereferenced
MEAN = (104.0, 117.0, 123.0)
ODD_MEAN = (104.008, 116.669, 122.675)
SOURCES = ((1, 1), (2, 3), (37, 53), (64, 48))
TARGETS = ((1, 1), (17, 25), (40, 24), (64, 48))
# (source, target) pairs on which this scipy's default zoom mode drops no last sample, i.e. agrees with mode="nearest" (see
# tests/test_multiscale_f.py); every other pair of SOURCES x TARGETS: test_scipy_precondition_of_the_layer_comparison
SCIPY_PAIRS = tuple((s, t) for s in SOURCES for t in TARGETS if (s, t) != ((64, 48), (40, 24)))


def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


_cache = {}


def _sources():
    """the source images of the value tests, made once, read-only"""
    if "src" not in _cache:
        rng = np.random.default_rng(41)
        ims = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SOURCES]
        for im in ims:
            im.setflags(write=False)
        _cache["src"] = ims
    return _cache["src"]


def _restated(i, h, w, mean, bgr=True):
    """source image i zoomed to h x w as preprocess.hip states it, in numpy float64 (every product and sum is one numpy operation,
    rounded on its own): coordinate y * (H-1)/(h-1), taps i0 = (int)src, i1 = i0 + (i0 < in-1), the blend l0h*(l0w*v00 + l1w*v01)
    + l1h*(l0w*v10 + l1w*v11), one rounding to f32, channel order, f32 mean subtraction -> (3, h, w) float32.  Once per case."""
    key = ("restated", i, h, w, tuple(mean), bool(bgr))
    if key not in _cache:
        _cache[key] = _zoom_restated(_sources()[i], h, w, mean, bgr)
        _cache[key].setflags(write=False)
    return _cache[key]


def _zoom_restated(im, h, w, mean, bgr=True):
    H, W = im.shape[0], im.shape[1]
    sy = (float(H - 1) / float(h - 1) if h > 1 else 0.0) * np.arange(h, dtype=np.float64)
    sx = (float(W - 1) / float(w - 1) if w > 1 else 0.0) * np.arange(w, dtype=np.float64)
    y0, x0 = sy.astype(np.int64), sx.astype(np.int64)
    y1, x1 = y0 + (y0 < H - 1), x0 + (x0 < W - 1)
    l1h, l1w = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
    l0h, l0w = 1.0 - l1h, 1.0 - l1w
    v = (im[:, :, ::-1] if bgr else im).astype(np.float64)
    v00, v01, v10, v11 = v[y0][:, x0], v[y0][:, x1], v[y1][:, x0], v[y1][:, x1]
    z = (l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)).astype(np.float32)
    out = np.ascontiguousarray((z - np.asarray(mean, dtype=np.float32)).transpose(2, 0, 1))
    assert out.dtype == np.float32
    return out


def _coco_layer(C, size, mean, ignore_label=255, mirror=False):
    """layers.AnnotationLayerCOCO set up by hand (its setup() reads a list file)"""
    from dsrg_amd import layers
    lay = layers.AnnotationLayerCOCO()
    lay.num_classes, lay.mean, (lay.new_h, lay.new_w) = C, mean, size
    lay.ignore_label, lay.is_mirror = ignore_label, mirror
    return lay


def _cues_ref(cue_maps, mirror, C, ignore_label):
    """(labels (B,1,1,C), cues (B,C,Hm,Wm)) float32 from AnnotationLayerCOCO.preprocess per image; the mirror is the layer's own,
    its draw driven through a seeded np.random replaced by the wanted flag"""
    lay = _coco_layer(C, (1, 1), (0.0, 0.0, 0.0), ignore_label, mirror=True)
    labels, cues = [], []
    state = np.random.get_state()
    try:
        for cue, m in zip(cue_maps, mirror):
            seed = 0
            while True:                                                 # a seed whose first choice(2) is the wanted draw
                np.random.seed(seed)
                if (np.random.choice(2) == 0) == bool(m):
                    break
                seed += 1
            np.random.seed(seed)
            _, planes, present = lay.preprocess(np.zeros((1, 1, 3), np.uint8), cue)
            cues.append(np.asarray(planes, dtype=np.float32))
            labels.append(np.asarray(present, dtype=np.float32))
    finally:
        np.random.set_state(state)
    return np.stack(labels), np.stack(cues)


def _write_cuemap_files(tmp_path, rng, sizes, map_size, C, sub=""):
    """PNG images and cue PNGs (classes below C, about a fifth 255) and a list file -> (list path, root, [(image, cue) names])"""
    from PIL import Image
    names = []
    for k, (H, W) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(tmp_path / ("%sim%d.png" % (sub, k))))
        cue = rng.integers(0, C, map_size).astype(np.uint8)
        cue[rng.random(map_size) < 0.2] = 255
        Image.fromarray(cue, mode="L").save(str(tmp_path / ("%scue%d.png" % (sub, k))))
        names.append(("/%sim%d.png" % (sub, k), "/%scue%d.png" % (sub, k)))
    lst = tmp_path / ("%strain_cuemap.txt" % sub)
    lst.write_text("".join("%s %s\n" % n for n in names))
    return str(lst), str(tmp_path), names


# ---- CPU: argument checks -----------------------------------------------------------------------------------------------------------
def test_cuemap_input_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(*MEAN)

    def call(B=3, stage=_FAKE, nbytes=4096, off="d", H="d", W="d", coff="d", mir="d", Sh=5, Sw=6, C=81, Hm=5, Wm=7, mean=mean3,
             ignore=255, bgr=1, images=_FAKE, cues=_FAKE, labels=_FAKE):
        n = max(B, 1)
        d = lambda v, dflt: _i32(dflt) if isinstance(v, str) else v                    # noqa: E731
        return L.dsrg_train_s_cuemap_input_batch(B, stage, nbytes, d(off, [256 * b for b in range(n)]), d(H, [4] * n), d(W, [5] * n),
                                                 d(coff, [1024 + 64 * b for b in range(n)]), d(mir, [0] * n), Sh, Sw, C, Hm, Wm,
                                                 mean, ignore, bgr, images, cues, labels, None)

    E, U = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert call(B=0) == E and b"images" in L.dsrg_last_error()
    assert call(B=33) == E and b"32" in L.dsrg_last_error()
    assert call(C=0) == E and b"classes" in L.dsrg_last_error()
    assert call(C=97) == U and b"96" in L.dsrg_last_error()
    for name in ("Sh", "Sw", "Hm", "Wm"):
        assert call(**{name: 0}) == E and b"size" in L.dsrg_last_error(), name
    assert call(H=_i32([4, 0, 4])) == E and call(W=_i32([5, 5, 0])) == E
    assert call(off=_i32([0, 256, 4096 - 59])) == E and b"image 2 lies outside" in L.dsrg_last_error()     # 60 bytes from 4037
    assert call(off=_i32([0, -4, 512])) == E and b"outside" in L.dsrg_last_error()
    assert call(coff=_i32([1024, 1088, 4096 - 34])) == E and b"cue map 2 lies outside" in L.dsrg_last_error()  # 35 bytes from 4062
    assert call(nbytes=100) == E and b"outside" in L.dsrg_last_error()
    assert call(stage=None) == E and b"NULL" in L.dsrg_last_error()
    for name in ("off", "H", "W", "coff", "mir", "mean"):
        assert call(**{name: None}) == E and b"NULL" in L.dsrg_last_error(), name
    for name in ("images", "cues", "labels"):
        assert call(**{name: None}) == E and b"NULL " + name.encode() in L.dsrg_last_error(), name
        assert call(**{name: 258}) == E and b"aligned" in L.dsrg_last_error(), name
    assert call(ignore=256) == E and call(ignore=-1) == E and b"ignore_label" in L.dsrg_last_error()
    assert call(bgr=2) == E and b"bgr" in L.dsrg_last_error()
    assert call(nbytes=1 << 31) == E and b"2^31" in L.dsrg_last_error()
    assert call(B=32, Sh=4800, Sw=4800) == E and b"2^31" in L.dsrg_last_error()                           # 32 * 3 * 4800^2
    assert call(B=32, C=96, Hm=1024, Wm=1024, nbytes=1 << 30) == E and b"2^31" in L.dsrg_last_error()     # 32 * 96 * 2^20
    assert call(B=1, H=_i32([32768]), W=_i32([32768])) == E and b"2^31" in L.dsrg_last_error()
    if not torch.cuda.is_available():                                  # everything in order: only the device is missing
        assert call() == _lib.ERR_HIP and L.dsrg_last_error()
        assert call(C=96, nbytes=1 << 16) == _lib.ERR_HIP               # the last class count the label flags hold
        # the pieces may end exactly at the buffer's end
        assert call(off=_i32([0, 256, 4096 - 60]), coff=_i32([1024, 1088, 2048])) == _lib.ERR_HIP
        assert call(coff=_i32([1024, 1088, 4096 - 35])) == _lib.ERR_HIP


# ---- CPU: layout, packing, refusals -------------------------------------------------------------------------------------------------
def test_cuemap_layout_and_packing():
    from dsrg_amd import input as I
    rng = np.random.default_rng(42)
    shapes, map_size = [(4, 5), (7, 3)], (5, 7)
    nbytes, desc = I.layout_train_s_cuemap(shapes, map_size, [True, False])
    # 60 image bytes -> 64; 35 cue bytes from 64 -> 99 -> 112; 63 image bytes from 112 -> 175 -> 176; 35 cue bytes -> 211 -> 224
    assert desc["image_off"] == [0, 112] and desc["cue_off"] == [64, 176] and nbytes == 224
    assert desc["H"] == [4, 7] and desc["W"] == [5, 3] and desc["mirror"] == [1, 0]
    assert all(o % 16 == 0 for o in desc["image_off"] + desc["cue_off"])
    assert I.layout_train_s_cuemap(shapes, map_size)[1]["mirror"] == [0, 0]
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    cues = [rng.integers(0, 256, map_size).astype(np.uint8) for _ in shapes]
    buf = np.full(nbytes, 0xEE, np.uint8)
    I.pack_train_s_cuemap(buf, desc, images, cues)
    for b in range(2):
        o = desc["image_off"][b]
        assert np.array_equal(buf[o:o + images[b].size].reshape(images[b].shape), images[b])
        o = desc["cue_off"][b]
        assert np.array_equal(buf[o:o + 35].reshape(map_size), cues[b])
    assert (buf[60:64] == 0xEE).all() and (buf[99:112] == 0xEE).all()                  # the padding is left alone
    with pytest.raises(ValueError):
        I.pack_train_s_cuemap(buf, desc, images, [cues[0], cues[1][:4]])
    with pytest.raises(ValueError):
        I.pack_train_s_cuemap(buf, desc, images, [cues[0], cues[1].astype(np.int32)])
    with pytest.raises(ValueError):
        I.pack_train_s_cuemap(buf, desc, [images[1], images[0]], cues)
    with pytest.raises(ValueError):
        I.pack_train_s_cuemap(buf, desc, [images[0], images[1].astype(np.float32)], cues)
    with pytest.raises(ValueError):
        I.layout_train_s_cuemap([(4, 5), (0, 3)], map_size)
    with pytest.raises(ValueError):
        I.layout_train_s_cuemap(shapes, (0, 7))
    with pytest.raises(ValueError) as e:
        I.layout_train_s_cuemap([(2, 2)] * 33, map_size)
    assert "33" in str(e.value)
    I.layout_train_s_cuemap([(2, 2)] * 32, map_size)
    with pytest.raises(ValueError):
        I.layout_train_s_cuemap([], map_size)


def test_cuemap_loader_refuses_bad_cue_files_before_any_upload(tmp_path):
    from PIL import Image
    from dsrg_amd import input as I
    rng = np.random.default_rng(43)
    lst, root, names = _write_cuemap_files(tmp_path, rng, [(9, 11), (12, 7), (8, 8)], (4, 6), 81)
    mk = lambda **kw: I.TrainSCueMapInput(lst, root, 81, batch_size=3, size=(24, 40), shuffle=False, **kw)    # noqa: E731

    def laid_out(ld):                                                   # what an upload does before it touches the device
        return ld.stage_batch()

    ld = mk()
    assert ld.map_size == (4, 6) and ld.size == (24, 40)
    nbytes, desc, pieces = laid_out(ld)
    assert len(desc["H"]) == 3 and nbytes % 16 == 0 and desc["H"] == [9, 12, 8]
    cue_file = str(tmp_path / "cue1.png")
    good = np.array(Image.open(cue_file))
    # a cue map of another size
    Image.fromarray(np.zeros((4, 5), np.uint8), mode="L").save(cue_file)
    with pytest.raises(ValueError) as e:
        laid_out(mk())
    assert "cue1.png" in str(e.value) and "4 x 5" in str(e.value)
    # a byte 81 at C = 81, while 255 passes
    bad = good.copy()
    bad[2, 3] = 81
    Image.fromarray(bad, mode="L").save(cue_file)
    with pytest.raises(ValueError) as e:
        laid_out(mk())
    assert "cue1.png" in str(e.value) and "81" in str(e.value)
    bad[2, 3] = 255
    Image.fromarray(bad, mode="L").save(cue_file)
    laid_out(mk())
    bad[:] = 255                                                        # a map with no kept pixel is allowed
    Image.fromarray(bad, mode="L").save(cue_file)
    laid_out(mk())
    bad[0, 0] = 80
    Image.fromarray(bad, mode="L").save(cue_file)
    laid_out(mk())
    with pytest.raises(ValueError) as e:                                # ... but is no class of an 80-class run
        plan_ld = I.TrainSCueMapInput(lst, root, 80, batch_size=3, size=(24, 40), shuffle=False)
        laid_out(plan_ld)
    assert "cue1.png" in str(e.value)
    for C in (0, 97, -1):
        with pytest.raises(ValueError) as e:
            I.TrainSCueMapInput(lst, root, C, batch_size=3, size=(24, 40))
        assert "num_classes" in str(e.value)
    I.TrainSCueMapInput(lst, root, 96, batch_size=3, size=(24, 40))
    I.TrainSCueMapInput(lst, root, 1, batch_size=3, size=(24, 40))
    with pytest.raises(ValueError):
        I.TrainSCueMapInput(lst, root, 81, batch_size=33, size=(24, 40))
    with pytest.raises(ValueError):
        I.TrainSCueMapInput(lst, root, 81, batch_size=3, size=(24, 40), ignore_label=256)
    assert I.TrainSCueMapInput(lst, root, 81, size=321).map_size == (41, 41)
    # check_cue_map on arrays
    with pytest.raises(ValueError) as e:
        I.check_cue_map(np.zeros((4, 6), np.int32), 81, (4, 6), 255, "x.png")
    assert "x.png" in str(e.value)
    I.check_cue_map(np.full((4, 6), 7, np.uint8), 8, (4, 6), 255, "x.png")
    with pytest.raises(ValueError):
        I.check_cue_map(np.full((4, 6), 7, np.uint8), 7, (4, 6), 255, "x.png")
    I.check_cue_map(np.full((4, 6), 7, np.uint8), 7, (4, 6), 7, "x.png")              # 7 is the ignore label there


# ---- CPU: planning ------------------------------------------------------------------------------------------------------------------
def test_cuemap_epoch_order_wraps_mid_batch_and_mirror_draws_are_the_layers(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(44)
    lst, root, names = _write_cuemap_files(tmp_path, rng, [(3, 3)] * 5, (1, 1), 81)
    seed = 6
    ld = I.TrainSCueMapInput(lst, root, 81, batch_size=3, size=(4, 4), seed=seed)
    plans = [ld.plan_batch() for _ in range(4)]                         # 12 items: two epochs and two of the third
    got = [(it["image"], it["cue"]) for plan in plans for it in plan]
    full = [(root + a, root + b) for a, b in names]
    second = list(full)
    shuffler = random.Random(seed)
    shuffler.shuffle(second)
    third = list(second)
    shuffler.shuffle(third)
    assert got[:5] == full                                              # file order first; batch 1 holds items 3, 4 and the new epoch's first
    assert got[5:10] == second and got[10:] == third[:2]
    assert second != full                                               # (the seed does shuffle)
    draws = np.random.RandomState(seed)
    want = [int(draws.choice(2)) == 0 for _ in range(12)]
    assert [it["mirror"] for plan in plans for it in plan] == want and True in want and False in want
    # no mirror: no flag, and the draws are not needed
    ld = I.TrainSCueMapInput(lst, root, 81, batch_size=3, size=(4, 4), seed=seed, mirror=False)
    assert not any(it["mirror"] for it in ld.plan_batch())
    # without shuffling every epoch is the file
    ld = I.TrainSCueMapInput(lst, root, 81, batch_size=5, size=(4, 4), seed=seed, shuffle=False)
    assert [[it["image"] for it in ld.plan_batch()] for _ in range(2)] == [[f[0] for f in full]] * 2
    # two ranks partition each epoch
    ranks = [I.TrainSCueMapInput(lst, root, 81, batch_size=1, size=(4, 4), seed=seed, rank=r, world_size=2) for r in range(2)]
    a = [ranks[0].plan_batch()[0]["image"] for _ in range(6)]           # 3 items of each epoch
    b = [ranks[1].plan_batch()[0]["image"] for _ in range(4)]           # 2 items of each epoch
    for n, epoch in enumerate((full, second)):
        assert a[3 * n:3 * n + 3] == [e[0] for e in epoch[0::2]] and b[2 * n:2 * n + 2] == [e[0] for e in epoch[1::2]]
        assert sorted(a[3 * n:3 * n + 3] + b[2 * n:2 * n + 2]) == sorted(e[0] for e in full)
    with pytest.raises(ValueError):                                     # (epoch_items speaks at the first item)
        I.TrainSCueMapInput(lst, root, 81, batch_size=1, size=(4, 4), rank=2, world_size=2).plan_batch()
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    with pytest.raises(ValueError):
        I.TrainSCueMapInput(str(empty), root, 81)
    short = tmp_path / "short.txt"
    short.write_text("/im0.png\n")
    with pytest.raises(ValueError):
        I.TrainSCueMapInput(str(short), root, 81)


# ---- CPU: the command and the trainers --------------------------------------------------------------------------------------------------
def test_train_command_class_and_cue_map_options():
    from dsrg_amd import train as T
    s = T.parse_args(["--stage", "s", "--list", "l", "--root", "r", "--cues", "c"])
    assert s.num_classes == 21 and s.cue_maps is False and s.channel_order == "bgr" and s.cues == "c"
    f = T.parse_args(["--stage", "f", "--list", "l", "--root", "r"])
    assert f.num_classes == 21 and f.cue_maps is False
    s = T.parse_args(["--stage", "s", "--list", "l", "--root", "r", "--cue-maps", "--class", "81"])
    assert s.num_classes == 81 and s.cue_maps is True and s.channel_order == "bgr" and s.cues is None
    s = T.parse_args(["--stage", "s", "--list", "l", "--root", "r", "--cue-maps", "--channel-order", "rgb"])
    assert s.num_classes == 21 and s.channel_order == "rgb"
    f = T.parse_args(["--stage", "f", "--list", "l", "--root", "r", "--class", "96"])
    assert f.num_classes == 96
    assert T.parse_args(["--stage", "f", "--list", "l", "--root", "r", "--class", "1"]).num_classes == 1
    base = ["--list", "l", "--root", "r"]
    for bad in (["--stage", "f", "--cue-maps"],
                ["--stage", "s", "--cue-maps", "--cues", "c"],
                ["--stage", "s"],
                ["--stage", "s", "--cues", "c", "--channel-order", "rgb"],
                ["--stage", "f", "--channel-order", "bgr"],
                ["--stage", "s", "--cue-maps", "--channel-order", "grb"],
                ["--stage", "s", "--cue-maps", "--class", "0"],
                ["--stage", "s", "--cue-maps", "--class", "97"],
                ["--stage", "f", "--class", "0"],
                ["--stage", "f", "--class", "97"],
                ["--stage", "s", "--cues", "c", "--class", "81"]):     # the pickle's planes are 21
        with pytest.raises(SystemExit) as e:
            T.parse_args(bad + base)
        assert e.value.code == 2, bad


def test_trainers_take_num_classes_and_keep_the_default_initial_weights():
    from dsrg_amd.backbone import VGG16ASPP
    from dsrg_amd.retrain import RetrainTrainer
    from dsrg_amd.trainer import DSRGTrainer
    cpu = torch.device("cpu")
    loss = lambda *a: None                                             # noqa: E731  (never called: no step is taken)
    t = DSRGTrainer(cpu, seed=4, loss_fn=loss, channels_last=False, num_classes=81)
    heads = [m for m in t.net.modules() if isinstance(m, torch.nn.Conv2d) and m.out_channels == 81]
    assert len(heads) == 4 and all(m.in_channels == 1024 for m in heads)
    r = RetrainTrainer(cpu, seed=4, num_classes=81)
    assert len([m for m in r.net.modules() if isinstance(m, torch.nn.Conv2d) and m.out_channels == 81]) == 4
    # the default run's initial weights: the net built behind the trainer's own manual_seed, bit for bit what a caller made before
    torch.manual_seed(4)
    want = VGG16ASPP()
    got = DSRGTrainer(cpu, seed=4, loss_fn=loss, channels_last=False).net
    assert all(torch.equal(a, b) for a, b in zip(want.parameters(), got.parameters()))
    for bad in (0, 97):
        with pytest.raises(ValueError):
            DSRGTrainer(cpu, loss_fn=loss, channels_last=False, num_classes=bad)
        with pytest.raises(ValueError):
            RetrainTrainer(cpu, num_classes=bad)


def test_scipy_precondition_of_the_layer_comparison():
    """the bgr = 0 GPU test compares with AnnotationLayerCOCO.preprocess, i.e. scipy's zoom in its DEFAULT mode; the kernel states
    the zoom that mode="nearest" gives (tests/test_multiscale_f.py).  On every pair of SCIPY_PAIRS the two modes agree exactly."""
    from scipy.ndimage import zoom
    assert len(SCIPY_PAIRS) == 15
    for (H, W), (h, w) in SCIPY_PAIRS:
        im = _sources()[SOURCES.index((H, W))].astype(np.float32)
        f = (h / float(H), w / float(W), 1.0)
        a, b = zoom(im, f, order=1), zoom(im, f, order=1, mode="nearest")
        assert a.shape == b.shape == (h, w, 3) and np.array_equal(a, b), ((H, W), (h, w))


def test_restatement_identity_and_a_hand_computed_case():
    im = _sources()[3]
    assert np.array_equal(_restated(3, 64, 48, (0.0, 0.0, 0.0)), im[:, :, ::-1].transpose(2, 0, 1).astype(np.float32))
    assert np.array_equal(_restated(3, 64, 48, (0.0, 0.0, 0.0), bgr=False), im.transpose(2, 0, 1).astype(np.float32))
    two = np.array([[[10, 20, 30], [50, 60, 70]]], np.uint8)                              # 1 x 2 -> 1 x 3: the middle is the mean
    assert np.array_equal(_zoom_restated(two, 1, 3, (1.0, 2.0, 3.0))[:, 0], [[29.0, 49.0, 69.0], [18.0, 38.0, 58.0], [7.0, 27.0, 47.0]])
    assert np.array_equal(_zoom_restated(two, 1, 3, (1.0, 2.0, 3.0), bgr=False)[:, 0], [[9.0, 29.0, 49.0], [18.0, 38.0, 58.0], [27.0, 47.0, 67.0]])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _run_kernel(images, cue_maps, mirror, size, C, map_size, mean=MEAN, ignore_label=255, bgr=True):
    """one launch, repeated into outputs prefilled with 7.0: every element is written and the bits repeat -> numpy (images, labels,
    cues)"""
    from dsrg_amd import input as I
    from dsrg_amd import ops
    nbytes, desc = I.layout_train_s_cuemap([s.shape[:2] for s in images], map_size, mirror)
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_s_cuemap(buf, desc, images, cue_maps)
    stage = torch.from_numpy(buf).cuda()
    filled = (torch.full((len(images), 3) + tuple(size), 7.0, device="cuda"), torch.full((len(images), 1, 1, C), 7.0, device="cuda"),
              torch.full((len(images), C) + tuple(map_size), 7.0, device="cuda"))
    out = ops.train_s_cuemap_input_batch(stage, desc, size, C, map_size, mean, ignore_label, bgr, out=filled)
    assert all(o is f for o, f in zip(out, filled))
    again = ops.train_s_cuemap_input_batch(stage, desc, size, C, map_size, mean, ignore_label, bgr)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert [tuple(o.shape) for o in out] == [tuple(f.shape) for f in filled] and all(o.dtype == torch.float32 for o in out)
    return [o.cpu().numpy() for o in out]


def _batches():
    """(source indices, mirror flags) of batches of 1, 3 and 32 images with mixed flags"""
    return [([2], [True]), ([0, 2, 3], [False, True, True]),
            ([k % 4 for k in range(32)], [bool((k * 5 // 3) % 2) for k in range(32)])]


@pytest.mark.gpu
@pytest.mark.parametrize("target", TARGETS)
def test_cuemap_kernel_images_bgr_equal_preprocess_rect_batch_and_the_restatement(target):
    from dsrg_amd import ops
    h, w = target
    srcs = _sources()
    rect = ops.preprocess_rect_batch([torch.from_numpy(s.copy()).cuda() for s in srcs], [target], mean=ODD_MEAN)[0]
    for i in range(4):
        assert np.array_equal(rect[i].cpu().numpy(), _restated(i, h, w, ODD_MEAN)), SOURCES[i]
    none = np.full((2, 3), 255, np.uint8)
    seen = set()
    for idx, mirror in _batches():
        got = _run_kernel([srcs[i] for i in idx], [none] * len(idx), mirror, target, 4, (2, 3), ODD_MEAN)[0]
        for b, (i, m) in enumerate(zip(idx, mirror)):
            want = torch.flip(rect[i], dims=[2]) if m else rect[i]
            assert np.array_equal(got[b], want.cpu().numpy()), (b, SOURCES[i], m)
            want = _restated(i, h, w, ODD_MEAN)
            assert np.array_equal(got[b], want[:, :, ::-1] if m else want), (b, SOURCES[i], m)
            seen.add((i, m))
    assert len(seen) == 8                                               # every source mirrored and not


@pytest.mark.gpu
@pytest.mark.parametrize("target", TARGETS)
def test_cuemap_kernel_images_rgb_equal_annotation_layer_coco(target):
    test_scipy_precondition_of_the_layer_comparison()
    srcs = _sources()
    lay = _coco_layer(4, target, list(ODD_MEAN))
    none = np.full((2, 3), 255, np.uint8)
    use = [SOURCES.index(s) for s, t in SCIPY_PAIRS if t == target]
    assert len(use) >= 3
    want = {i: np.asarray(lay.preprocess(srcs[i][:, :, ::-1], none)[0]) for i in use}    # (the layer is handed cv2's BGR)
    worst = 0.0
    for idx, mirror in _batches():
        idx = [use[i % len(use)] for i in idx]
        got = _run_kernel([srcs[i] for i in idx], [none] * len(idx), mirror, target, 4, (2, 3), ODD_MEAN, bgr=False)[0]
        for b, (i, m) in enumerate(zip(idx, mirror)):
            assert np.array_equal(got[b], _restated(i, target[0], target[1], ODD_MEAN, bgr=False)[:, :, ::(-1 if m else 1)])
            err = float(np.abs(got[b].astype(np.float64) - want[i][:, :, ::(-1 if m else 1)]).max())
            worst = max(worst, err)
            assert err <= 1e-5 * 255, (b, SOURCES[i], m, err)
    print("target %s: max |kernel - AnnotationLayerCOCO.preprocess| = %.3g" % (target, worst))


def _cue_batch(rng, B, C, map_size, ignore_label):
    """B cue maps; from B = 3 on the first three are: all ignore_label, one class other than 0 (where there is one), class C - 1"""
    maps = []
    for b in range(B):
        m = rng.integers(0, C, map_size).astype(np.uint8)
        m[rng.random(map_size) < 0.3] = ignore_label
        maps.append(m)
    if B >= 3:
        maps[0] = np.full(map_size, ignore_label, np.uint8)
        maps[1] = np.full(map_size, C // 2, np.uint8)
        maps[2][...] = rng.integers(0, C, map_size)
        maps[2].flat[0] = C - 1
    return maps


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_label", [255, 0])
@pytest.mark.parametrize("C", [1, 21, 81, 96])
def test_cuemap_kernel_cues_and_labels_equal_annotation_layer_coco(C, ignore_label):
    rng = np.random.default_rng(1000 * C + ignore_label)
    tiny = [rng.integers(0, 256, (2, 3, 3), dtype=np.uint8), rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)]
    for map_size in ((1, 1), (5, 7), (41, 41)):
        for B in (1, 3, 32):
            maps = _cue_batch(rng, B, C, map_size, ignore_label)
            mirror = [bool((b * 5 // 3 + 1) % 2) for b in range(B)]
            assert B == 1 or (True in mirror and False in mirror)
            want_l, want_c = _cues_ref(maps, mirror, C, ignore_label)
            plain_l, plain_c = _cues_ref(maps, [False] * B, C, ignore_label)
            for b in range(B):                                          # the layer's mirror is the flipped unmirrored result
                assert np.array_equal(want_c[b], plain_c[b][:, :, ::-1] if mirror[b] else plain_c[b])
            _, got_l, got_c = _run_kernel([tiny[b % 2] for b in range(B)], maps, mirror, (3, 2), C, map_size, MEAN, ignore_label)
            assert got_l.shape == want_l.shape and np.array_equal(got_l, want_l), (map_size, B)
            assert got_c.shape == want_c.shape and np.array_equal(got_c, want_c), (map_size, B)
            assert set(np.unique(got_c)) <= {0.0, 1.0} and set(np.unique(got_l)) <= {0.0, 1.0}
            if B >= 3:
                assert not got_l[0].any() and not got_c[0].any()        # all ignore_label: no cue, no label (class 0 is not forced on)
                if C // 2 != ignore_label:
                    assert got_l[1].sum() == 1 and got_l[1, 0, 0, C // 2] == 1 and got_c[1, C // 2].all()
                if C - 1 != ignore_label:
                    assert got_l[2, 0, 0, C - 1] == 1


def _host_batch(plan, size, C, map_size, mean, ignore_label=255, bgr=True):
    """the host composition of a plan: files -> the restated zoom and AnnotationLayerCOCO's planes and labels, with the plan's flags"""
    from dsrg_amd import input as I
    images, maps = [I.read_rgb(it["image"]) for it in plan], [I.read_gray(it["cue"]) for it in plan]
    mirror = [it["mirror"] for it in plan]
    want_i = np.stack([_zoom_restated(im, size[0], size[1], mean, bgr)[:, :, ::(-1 if m else 1)] for im, m in zip(images, mirror)])
    want_l, want_c = _cues_ref(maps, mirror, C, ignore_label)
    return want_i, want_l, want_c


@pytest.mark.gpu
def test_cuemap_loader_end_to_end_equals_the_host_composition(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(45)
    size, C = (24, 40), 81
    lst, root, _ = _write_cuemap_files(tmp_path, rng, [(37, 53), (24, 40), (9, 70), (64, 31), (5, 5)], (4, 6), C)
    seed = 2
    planner = I.TrainSCueMapInput(lst, root, C, batch_size=3, size=size, mean=ODD_MEAN, seed=seed)      # the same plans, no device
    kept = []
    with I.TrainSCueMapInput(lst, root, C, batch_size=3, size=size, mean=ODD_MEAN, seed=seed, workers=3) as ld:
        for n in range(4):                                              # two epochs and a wrap
            got = next(ld)
            plan = planner.plan_batch()
            assert [tuple(g.shape) for g in got] == [(3, 3, 24, 40), (3, 1, 1, C), (3, C, 4, 6)]
            for g, w in zip(got, _host_batch(plan, size, C, (4, 6), ODD_MEAN)):
                assert g.is_cuda and g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), w), n
            if kept:                                                    # the slot contract: batch n-1 is still batch n-1
                assert all(torch.equal(t, c) for t, c in zip(*kept)), n
            kept = (got, [t.clone() for t in got])
    assert all(torch.equal(t, c) for t, c in zip(*kept))                # close() leaves the returned tensors alone
    assert torch.cuda.current_stream() == torch.cuda.default_stream()   # no stream state left behind
    # the layer's own channel order, no mirror
    planner = I.TrainSCueMapInput(lst, root, C, batch_size=2, size=size, mean=ODD_MEAN, seed=seed, bgr=False, mirror=False, shuffle=False)
    with I.TrainSCueMapInput(lst, root, C, batch_size=2, size=size, mean=ODD_MEAN, seed=seed, bgr=False, mirror=False, shuffle=False,
                             workers=2) as ld:
        got = next(ld)
        for g, w in zip(got, _host_batch(planner.plan_batch(), size, C, (4, 6), ODD_MEAN, bgr=False)):
            assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.gpu
def test_an_undecodable_file_closes_the_cuemap_loader(tmp_path):
    from dsrg_amd import input as I
    rng = np.random.default_rng(46)
    lst, root, names = _write_cuemap_files(tmp_path, rng, [(9, 9), (8, 12), (7, 7), (6, 6)], (2, 2), 21)
    with open(root + names[2][1], "wb") as f:
        f.write(b"not a png")
    ld = I.TrainSCueMapInput(lst, root, 21, batch_size=1, size=(8, 8), shuffle=False, workers=2)
    first = next(ld)                                                    # batch 0; batch 1 uploaded, batch 2 decoding
    kept = [t.clone() for t in first]
    with pytest.raises(Exception) as e:
        next(ld)                                                        # collecting batch 2 fails
    assert not isinstance(e.value, RuntimeError) or "closed" not in str(e.value)
    with pytest.raises(RuntimeError):
        next(ld)                                                        # no retry: the loader is closed
    assert all(torch.equal(t, c) for t, c in zip(first, kept))
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


def _run_train(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


def _losses(out):
    import re
    rows = [ln for ln in out.splitlines() if ln.startswith("Iteration ")]
    values = [float(v) for ln in rows for v in re.findall(r"loss[-\w]* = ([-+.\dnaife]+)", ln)]
    return rows, values


def _classifier_outputs(caffemodel):
    """outputs of every fc8 classifier kernel in a snapshot"""
    from dsrg_amd.checkpoint import read_caffemodel
    layers = read_caffemodel(caffemodel)
    heads = sorted(n for n in layers if n.startswith("fc8"))
    return heads, [int(layers[n][0].shape[0]) for n in heads], [int(layers[n][1].size) for n in heads]


@pytest.mark.gpu
def test_train_command_stage_s_on_cue_maps_at_81_classes_in_a_child_process(tmp_path):
    rng = np.random.default_rng(47)
    lst, root, _ = _write_cuemap_files(tmp_path, rng, [(321, 321), (300, 340), (321, 200)], (41, 41), 81)
    out = _run_train(["--stage", "s", "--cue-maps", "--class", "81", "--list", lst, "--root", root, "--iters", "2", "--batch", "2",
                      "--display", "1", "--workers", "2", "--seed", "3", "--prefix", str(tmp_path / "a" / "model-s")], timeout=600)
    rows, values = _losses(out)
    assert len(rows) == 2 and len(values) == 4 and np.isfinite(values).all(), out[-2000:]
    assert [ln for ln in out.splitlines() if ln.startswith("done: iteration 2 weights_checksum ")], out[-2000:]
    heads, outs, biases = _classifier_outputs(str(tmp_path / "a" / "model-s_iter_2.caffemodel"))
    assert heads == ["fc8-SEC_%d" % k for k in (1, 2, 3, 4)] and outs == [81] * 4 and biases == [81] * 4


@pytest.mark.gpu
def test_train_command_stage_f_at_81_classes_in_a_child_process(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(48)
    lines = []
    for k, (H, W) in enumerate(((70, 90), (50, 80), (66, 65))):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(tmp_path / ("im%d.png" % k)))
        lab = rng.integers(0, 81, (H, W)).astype(np.uint8)
        lab[0, 0] = 80
        Image.fromarray(lab, mode="L").save(str(tmp_path / ("lab%d.png" % k)))
        lines.append("/im%d.png /lab%d.png\n" % (k, k))
    lst = tmp_path / "train.txt"
    lst.write_text("".join(lines))
    out = _run_train(["--stage", "f", "--class", "81", "--list", str(lst), "--root", str(tmp_path), "--iters", "2", "--batch", "2",
                      "--crop", "65", "--display", "1", "--workers", "2", "--seed", "3", "--prefix", str(tmp_path / "a" / "model-f")],
                     timeout=600)
    rows, values = _losses(out)
    assert len(rows) == 2 and len(values) == 2 and np.isfinite(values).all(), out[-2000:]
    assert [ln for ln in out.splitlines() if ln.startswith("done: iteration 2 weights_checksum ")], out[-2000:]
    heads, outs, biases = _classifier_outputs(str(tmp_path / "a" / "model-f_iter_2.caffemodel"))
    assert len(heads) == 4 and outs == [81] * 4 and biases == [81] * 4
