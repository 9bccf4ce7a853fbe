"""Random-scale augmentation of the stage-2 training input: `scale_factors` in data.SimpleTransformer, input.TrainFInput,
ops.train_f_input_batch -> dsrg_train_f_input_scaled_batch (dsrg_amd/csrc/train_input.hip) and `python -m dsrg_amd.train
--scale-factors`.

CPU: a scalar, loop-per-pixel restatement of the rescaling written from DESIGN.md ("The resize contract", the scaled path of
"Training input") against data.resize_bilinear_u8 / data.resize_nearest; fixed nearest-neighbour and scaled-size cases; which draws
are made, from which generator and in which order; the entry point's argument checks; the command's arguments.
GPU: the kernel against the host composition (resize -> window -> mean, scale, mirror), against its unscaled sibling at Hs = H,
Ws = W; the loader end to end against ImageSegDataLayer; the command in a child process.  Everything is integer arithmetic or a
fixed sequence of float32 operations: bitwise equality throughout."""
import ctypes
import functools
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced
MEAN = (104.0, 117.0, 123.0)
ODD_MEAN = (104.008, 116.669, 122.675)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- the scalar restatement -------------------------------------------------------------------------------------------------------
def _tap(d, n, S, zero_at_border):
    """one output coordinate of an axis of n source and S output samples -> (source index, w0, w1)"""
    scale = 1.0 / (float(S) / float(n))
    f = np.float32((d + 0.5) * scale - 0.5)
    s = int(math.floor(f))
    f = np.float32(f - np.float32(s))
    if zero_at_border:
        if s < 0:
            s, f = 0, np.float32(0.0)
        if s >= n - 1:
            s, f = n - 1, np.float32(0.0)
    w1 = int(np.rint(np.float32(f * np.float32(2048.0))))
    w0 = int(np.rint(np.float32((np.float32(1.0) - f) * np.float32(2048.0))))
    return s, min(max(w0, -32768), 32767), min(max(w1, -32768), 32767)


def bilinear_ref(src, Hs, Ws):
    """(H, W, C) uint8 -> (Hs, Ws, C) uint8, pixel by pixel"""
    H, W, C = src.shape
    out = np.zeros((Hs, Ws, C), np.uint8)
    for dy in range(Hs):
        sy, b0, b1 = _tap(dy, H, Hs, False)
        y0, y1 = min(max(sy, 0), H - 1), min(max(sy + 1, 0), H - 1)
        for dx in range(Ws):
            sx, a0, a1 = _tap(dx, W, Ws, True)
            x0, x1 = sx, min(sx + 1, W - 1)
            for c in range(C):
                D0 = int(src[y0, x0, c]) * a0 + int(src[y0, x1, c]) * a1
                D1 = int(src[y1, x0, c]) * a0 + int(src[y1, x1, c]) * a1
                v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
                assert 0 <= v <= 255
                out[dy, dx, c] = v
    return out


def _nearest_index(d, n, S):
    scale = 1.0 / (float(S) / float(n))
    return min(int(math.floor(float(d) * scale)), n - 1)


def nearest_ref(src, Hs, Ws):
    H, W = src.shape
    out = np.zeros((Hs, Ws), src.dtype)
    for dy in range(Hs):
        for dx in range(Ws):
            out[dy, dx] = src[_nearest_index(dy, H, Hs), _nearest_index(dx, W, Ws)]
    return out


class _Blob(object):
    def __init__(self, a=None):
        self.data = a if a is not None else np.zeros((0,), np.float32)

    def reshape(self, *s):
        self.data = np.zeros(s, np.float32)


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


# ---- CPU: the contract --------------------------------------------------------------------------------------------------------------
def test_numpy_resizes_equal_the_scalar_restatement():
    from dsrg_amd import data as D
    rng = np.random.default_rng(31)
    for (H, W), (Hs, Ws) in (((1, 1), (3, 2)), ((2, 3), (1, 1)), ((7, 5), (11, 8)), ((13, 9), (6, 4)), ((5, 4), (5, 4)), ((1, 9), (1, 4))):
        img, lab = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
        got = D.resize_bilinear_u8(img, Hs, Ws)
        assert got.dtype == np.uint8 and got.shape == (Hs, Ws, 3) and np.array_equal(got, bilinear_ref(img, Hs, Ws)), (H, W, Hs, Ws)
        assert np.array_equal(D.resize_bilinear_u8(img[:, :, 1], Hs, Ws), got[:, :, 1])       # (a plane alone is its channel)
        got = D.resize_nearest(lab, Hs, Ws)
        assert got.dtype == np.uint8 and got.shape == (Hs, Ws) and np.array_equal(got, nearest_ref(lab, Hs, Ws)), (H, W, Hs, Ws)
        if (H, W) == (Hs, Ws):                                                                # the identity: every byte comes through
            assert np.array_equal(D.resize_bilinear_u8(img, Hs, Ws), img) and np.array_equal(got, lab)
    with pytest.raises(TypeError):
        D.resize_bilinear_u8(np.zeros((3, 3, 3), np.float32), 2, 2)
    with pytest.raises(ValueError):
        D.resize_bilinear_u8(np.zeros((3, 3, 3), np.uint8), 0, 2)
    with pytest.raises(ValueError):
        D.resize_nearest(np.zeros((3, 3), np.uint8), 2, 0)


def test_nearest_neighbour_fixed_cases():
    from dsrg_amd import data as D
    for n, S, want in ((3, 5, [0, 0, 1, 1, 2]), (5, 3, [0, 1, 3]), (3, 6, [0, 0, 1, 1, 2, 2])):
        line = np.arange(n, dtype=np.uint8)
        assert D.resize_nearest(line[None, :], 1, S)[0].tolist() == want                      # along x
        assert D.resize_nearest(line[:, None], S, 1)[:, 0].tolist() == want                   # along y
        assert [_nearest_index(d, n, S) for d in range(S)] == want


def test_scaled_size_rounds_half_to_even_and_never_below_one():
    from dsrg_amd import data as D
    assert D.scaled_size(5, 7, 0.5) == (2, 4)                                                 # 2.5 -> 2, 3.5 -> 4
    assert D.scaled_size(3, 3, 0.1) == (1, 1)
    assert D.scaled_size(375, 500, 1.5) == (562, 750)
    assert D.scaled_size(375, 500, 1.0) == (375, 500)
    assert all(isinstance(v, int) for v in D.scaled_size(375, 500, 0.75))


# ---- CPU: the draws -----------------------------------------------------------------------------------------------------------------
FACTORS = (0.5, 1.0, 1.5)


def test_scale_factor_draws_come_first_and_the_loader_makes_the_same(tmp_path, monkeypatch):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    rng = np.random.default_rng(32)
    lst, root = _write_f_files(tmp_path, rng)
    crop, seed = (17, 13), 11
    params = dict(source=lst, root_folder=root, batch_size=3, crop_size=crop, mean=MEAN, mirror=True, phase="Train",
                  scale_factors=FACTORS)
    ld = I.TrainFInput(params, seed=seed)
    assert ld.scale_factors == FACTORS
    plans = [it for _ in range(4) for it in ld.plan_batch()]                                  # 12 images of five sizes: two epochs and a wrap
    # BatchLoader + SimpleTransformer.preprocess under the global generators, every draw recorded with its name
    real = random.randrange, random.randint, np.random.choice
    drawn, want = [], []
    monkeypatch.setattr(random, "randrange", lambda n: drawn.append(("randrange", real[0](n))) or drawn[-1][1])
    monkeypatch.setattr(random, "randint", lambda lo, hi: drawn.append(("randint", real[1](lo, hi))) or drawn[-1][1])
    monkeypatch.setattr(np.random, "choice", lambda n: drawn.append(("choice", int(real[2](n)))) or drawn[-1][1])
    states = random.getstate(), np.random.get_state()
    random.seed(seed)
    np.random.seed(seed)
    try:
        bl = D.BatchLoader(dict(params))
        assert bl.transformer.scale_factors == FACTORS
        for _ in range(12):
            image_path, label_path = next(bl._epochs)
            del drawn[:]
            out = bl.transformer.preprocess(D._imread_bgr(image_path), D._imread_gray(label_path))
            want.append((image_path, list(drawn), out))
        end_states = random.getstate(), np.random.get_state()
    finally:
        random.setstate(states[0])
        np.random.set_state(states[1])
        monkeypatch.undo()
    # replay: a fresh pair of generators, consumed as randrange(3), randint, randint, choice(2) per image (and BatchLoader's shuffle
    # between two epochs), arrives at the same values, the same crops and the same generator states
    r, nr = random.Random(seed), np.random.RandomState(seed)
    entries = [ln.split() for ln in open(lst)]
    sizes = set()
    for n, (it, (path, draws, (ref_img, ref_lab))) in enumerate(zip(plans, want)):
        if n and n % 5 == 0:
            r.shuffle(entries)
        assert path == root + entries[n % 5][0] == it["image"]
        img, lab = D._imread_bgr(it["image"]), D._imread_gray(it["label"])
        k = r.randrange(len(FACTORS))
        Hs, Ws = D.scaled_size(lab.shape[0], lab.shape[1], FACTORS[k])
        max_top, max_left = D._Window((Hs, Ws), crop).slack()
        top = r.randint(0, max_top)
        left = r.randint(0, max_left)
        c = int(nr.choice(2))
        assert draws == [("randrange", k), ("randint", top), ("randint", left), ("choice", c)], n
        assert (it["factor"], it["Hs"], it["Ws"], it["top"], it["left"], it["mirror"]) == (k, Hs, Ws, top, left, c == 0), n
        win = D._Window((Hs, Ws), crop, top, left)
        x = (D.resize_bilinear_u8(img, Hs, Ws).astype(np.float32) - np.asarray(MEAN, np.float32)) * np.float32(1.0)
        mine_img, mine_lab = win.cut(x, 0.0).transpose(2, 0, 1), win.cut(D.resize_nearest(lab, Hs, Ws), 255)
        if c == 0:
            mine_img, mine_lab = mine_img[:, :, ::-1], mine_lab[:, ::-1]
        assert np.array_equal(mine_img, ref_img) and np.array_equal(mine_lab, ref_lab), n
        sizes.add((k, lab.shape))
    assert r.getstate() == end_states[0] and all(np.array_equal(a, b) for a, b in zip(nr.get_state(), end_states[1]))
    assert len(set(k for k, _ in sizes)) == 3 and len(set(s for _, s in sizes)) == 5


def test_no_factors_draw_nothing_extra(tmp_path):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    rng = np.random.default_rng(33)
    lst, root = _write_f_files(tmp_path, rng)
    base = dict(source=lst, root_folder=root, batch_size=3, crop_size=(17, 13), mean=MEAN, mirror=True, phase="Train")
    absent, empty = I.TrainFInput(dict(base), seed=4), I.TrainFInput(dict(base, scale_factors=()), seed=4)
    with_factors = I.TrainFInput(dict(base, scale_factors=FACTORS), seed=4)
    a, b = [absent.plan_batch() for _ in range(4)], [empty.plan_batch() for _ in range(4)]
    assert a == b and not any("Hs" in it or "Ws" in it or "factor" in it for plan in a for it in plan)
    assert all("Hs" in it for it in with_factors.plan_batch())
    # phase 'Test': no factor is drawn, nothing is rescaled
    test = I.TrainFInput(dict(base, phase="Test", scale_factors=FACTORS), seed=4)
    plain = I.TrainFInput(dict(base, phase="Test"), seed=4)
    assert test.plan_batch() == plain.plan_batch()
    # the layouts: same bytes with and without sizes, Hs / Ws only when given
    nbytes, desc = I.layout_train_f([(3, 5), (4, 2)], [0, 1], [1, 0], [True, False])
    sbytes, sdesc = I.layout_train_f([(3, 5), (4, 2)], [0, 1], [1, 0], [True, False], [(2, 2), (6, 3)])
    assert sbytes == nbytes and "Hs" not in desc and "Ws" not in desc
    assert (sdesc["Hs"], sdesc["Ws"]) == ([2, 6], [2, 3]) and {k: v for k, v in sdesc.items() if k not in ("Hs", "Ws")} == desc
    with pytest.raises(ValueError):
        I.layout_train_f([(3, 5), (4, 2)], [0, 1], [1, 0], [True, False], [(2, 2), (0, 3)])
    with pytest.raises(ValueError):
        I.layout_train_f([(3, 5), (4, 2)], [0, 1], [1, 0], [True, False], [(2, 2)])
    for bad in ((0.5, 0.0), (-1.0,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError):
            I.TrainFInput(dict(base, scale_factors=bad))
        with pytest.raises(ValueError):
            D.SimpleTransformer(dict(base, scale_factors=bad))
    # the transformer: the default is no factor; with factors a float image is refused, the no-label path is untouched
    params = dict(crop_size=(17, 13), mean=MEAN)
    D.SimpleTransformer.check_params(params)
    assert params["scale_factors"] == ()
    tr = D.SimpleTransformer(dict(crop_size=(17, 13), mean=MEAN, scale_factors=FACTORS))
    img = rng.integers(0, 256, (10, 9, 3), dtype=np.uint8)
    with pytest.raises(TypeError):
        tr.preprocess(img.astype(np.float32), np.zeros((10, 9), np.uint8))
    plain = D.SimpleTransformer(dict(crop_size=(17, 13), mean=MEAN))
    assert np.array_equal(tr.preprocess(img.astype(np.float32)), plain.preprocess(img.astype(np.float32)))
    assert np.array_equal(tr.pre_test_image(img), plain.pre_test_image(img))


# ---- CPU: argument checks -----------------------------------------------------------------------------------------------------------
def test_train_f_input_scaled_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(*MEAN)

    def call(B=3, stage=_FAKE, nbytes=4096, off="d", loff="d", H="d", W="d", Hs="d", Ws="d", top="d", left="d", mir="d", ch=17, cw=13,
             mean=mean3, data=_FAKE, label=_FAKE):
        n = max(B, 1)
        d = lambda v, dflt: _i32(dflt) if isinstance(v, str) else v                    # noqa: E731
        return L.dsrg_train_f_input_scaled_batch(B, stage, nbytes, d(off, [256 * b for b in range(n)]),
                                                 d(loff, [2048 + 64 * b for b in range(n)]), d(H, [4] * n), d(W, [5] * n),
                                                 d(Hs, [6] * n), d(Ws, [3] * n), d(top, [0] * n), d(left, [1] * n), d(mir, [0] * n),
                                                 ch, cw, mean, 1.0, 255.0, data, label, None)

    E = _lib.ERR_INVALID
    # the new arguments
    assert call(Hs=None) == E and b"NULL" in L.dsrg_last_error()
    assert call(Ws=None) == E and b"NULL" in L.dsrg_last_error()
    assert call(Hs=_i32([6, 0, 6])) == E and b"rescaled" in L.dsrg_last_error()
    assert call(Ws=_i32([3, 3, -1])) == E and b"rescaled" in L.dsrg_last_error()
    U = _lib.ERR_UNSUPPORTED
    assert call(Hs=_i32([6, 65536, 6]), Ws=_i32([3, 32768, 3])) == U and b"2^31" in L.dsrg_last_error()
    # ... and the sibling's, check for check
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
    assert call(top=_i32([0, (1 << 31) - 17, 0])) == U and b"2^31" in L.dsrg_last_error()          # top + ch = 2^31
    assert call(left=_i32([0, 0, (1 << 31) - 13])) == U and b"2^31" in L.dsrg_last_error()
    assert call(off=_i32([0, 256, 4096 - 59])) == E and b"outside" in L.dsrg_last_error()
    assert call(loff=_i32([2048, 2112, 4096 - 19])) == E and b"outside" in L.dsrg_last_error()
    assert call(nbytes=100) == E and b"outside" in L.dsrg_last_error()
    assert call(nbytes=1 << 31) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=32, ch=4800, cw=4800) == U and b"2^31" in L.dsrg_last_error()
    assert call(B=1, H=_i32([32768]), W=_i32([32768])) == U and b"2^31" in L.dsrg_last_error()
    if not torch.cuda.is_available():                                                             # everything in order: only the device is missing
        assert call() == _lib.ERR_HIP and L.dsrg_last_error()
        assert call(Hs=_i32([6, 46340, 1]), Ws=_i32([3, 46340, 1])) == _lib.ERR_HIP               # (46340^2 < 2^31)
        assert call(top=_i32([0, 500, 0])) == _lib.ERR_HIP                                         # (a crop wholly off the image is fine)


# ---- CPU: the command ------------------------------------------------------------------------------------------------------------
def test_scale_factors_on_the_command_line():
    from dsrg_amd import train as T
    f = ["--stage", "f", "--list", "l", "--root", "r"]
    assert T.parse_args(f).scale_factors == ()
    a = T.parse_args(f + ["--scale-factors", "0.5,0.75,1,1.25,1.5"])
    assert a.scale_factors == (0.5, 0.75, 1.0, 1.25, 1.5) and all(isinstance(s, float) for s in a.scale_factors)
    assert T.parse_args(f + ["--scale-factors", "2"]).scale_factors == (2.0,)
    for bad in ("0", "-1", "nan", "0.5,,1", "", "0.5,inf", "half"):
        with pytest.raises(SystemExit):
            T.parse_args(f + ["--scale-factors=" + bad])
    with pytest.raises(SystemExit):
        T.parse_args(["--stage", "s", "--list", "l", "--root", "r", "--cues", "c", "--scale-factors", "0.5,1"])
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train", "--help"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"--scale-factors" in r.stdout


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
CROP = (16, 24)
SOURCES = ((10, 9), (30, 40), (12, 30), (40, 8), (17, 13), (1, 1), (2, 61))
SCALED = ((15, 5), (15, 20), (12, 30), (7, 19), (26, 20), (3, 2), (1, 30))          # up, down, identity, 1 x 1 source, a ratio per axis


@functools.lru_cache(maxsize=None)
def _cases():
    """(image RGB, label) per source — made once, shared by the tests below and never written to"""
    rng = np.random.default_rng(34)
    out = []
    for H, W in SOURCES:
        img, lab = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 21, (H, W), dtype=np.uint8)
        img.setflags(write=False), lab.setflags(write=False)
        out.append((img, lab))
    return tuple(out)


def _placements(sizes):
    """per image, four (top, left, mirror): offsets at 0 and at the slack's maximum, mirrors mixed -> list of (image index, Hs, Ws,
    top, left, mirror)"""
    from dsrg_amd import data as D
    out = []
    for k, (Hs, Ws) in enumerate(sizes):
        max_top, max_left = D._Window((Hs, Ws), CROP).slack()
        for top, left, mirror in ((0, 0, False), (max_top, max_left, True), (max_top, 0, True), (0, max_left, False)):
            out.append((k, Hs, Ws, top, left, mirror))
    return out


def _host(img, lab, Hs, Ws, top, left, mirror, crop, mean, scale, ignore):
    """resize -> window -> mean, scale -> mirror, on the host"""
    from dsrg_amd import data as D
    win = D._Window((Hs, Ws), crop, top, left)
    bgr = D.resize_bilinear_u8(np.ascontiguousarray(img[:, :, ::-1]), Hs, Ws)
    x = (bgr.astype(np.float32) - np.asarray(mean, np.float32)) * np.float32(scale)
    d, l = win.cut(x, 0.0).transpose(2, 0, 1), win.cut(D.resize_nearest(lab, Hs, Ws), ignore)
    return (d[:, :, ::-1], l[:, ::-1]) if mirror else (d, l)


def _stage(images, labels, placements, scaled=True):
    from dsrg_amd import input as I
    nbytes, desc = I.layout_train_f([images[p[0]].shape[:2] for p in placements], [p[3] for p in placements], [p[4] for p in placements],
                                    [p[5] for p in placements], [(p[1], p[2]) for p in placements] if scaled else None)
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_f(buf, desc, [images[p[0]] for p in placements], [labels[p[0]] for p in placements])
    return torch.from_numpy(buf).cuda(), desc


@pytest.mark.gpu
def test_scaled_kernel_equals_the_host_composition():
    from dsrg_amd import ops
    images, labels = [c[0] for c in _cases()], [c[1] for c in _cases()]
    placements = _placements(SCALED)
    assert len(placements) == 28
    # the crop is larger than some scaled images and smaller than others, on each axis separately
    assert any(p[1] < CROP[0] for p in placements) and any(p[1] > CROP[0] for p in placements)
    assert any(p[2] < CROP[1] for p in placements) and any(p[2] > CROP[1] for p in placements)
    stage, desc = _stage(images, labels, placements)
    for scale, ignore in ((1.0, 255), (0.0039, 21)):
        data, label = ops.train_f_input_batch(stage, desc, CROP, ODD_MEAN, scale, ignore)
        again = ops.train_f_input_batch(stage, desc, CROP, ODD_MEAN, scale, ignore,
                                        out=[torch.full_like(data, 7.0), torch.full_like(label, 7.0)])
        assert torch.equal(data, again[0]) and torch.equal(label, again[1])             # every element is written, whatever was there
        want = [_host(images[k], labels[k], Hs, Ws, top, left, mirror, CROP, ODD_MEAN, scale, ignore)
                for k, Hs, Ws, top, left, mirror in placements]
        want_d = torch.from_numpy(np.stack([np.ascontiguousarray(w[0]) for w in want]))
        want_l = torch.from_numpy(np.stack([np.ascontiguousarray(w[1]) for w in want])[:, None])
        bad = int((data.cpu() != want_d).sum()), int((label.cpu() != want_l).sum())
        print("scale %g: %d of %d data values and %d of %d labels differ from the host composition"
              % (scale, bad[0], want_d.numel(), bad[1], want_l.numel()))
        assert torch.equal(data.cpu(), want_d) and torch.equal(label.cpu(), want_l)
    # 32 images of 3 x 3, all mirrored: bit 31 of the mirror mask
    rng = np.random.default_rng(35)
    small = [rng.integers(0, 256, (3, 3, 3), dtype=np.uint8) for _ in range(32)]
    slabs = [rng.integers(0, 21, (3, 3), dtype=np.uint8) for _ in range(32)]
    crop = (4, 5)
    sizes = [((3, 3), (5, 4), (2, 6), (1, 1))[b % 4] for b in range(32)]
    placements = [(b, Hs, Ws, max(Hs, crop[0]) - crop[0], 0, True) for b, (Hs, Ws) in enumerate(sizes)]
    stage, desc = _stage(small, slabs, placements)
    assert desc["mirror"] == [1] * 32
    data, label = ops.train_f_input_batch(stage, desc, crop, MEAN, 1.0, 255)
    want = [_host(small[b], slabs[b], Hs, Ws, top, left, True, crop, MEAN, 1.0, 255) for b, Hs, Ws, top, left, _ in placements]
    for b in range(32):
        assert np.array_equal(data[b].cpu().numpy(), want[b][0]) and np.array_equal(label[b, 0].cpu().numpy(), want[b][1]), b
    assert not np.array_equal(want[31][0], want[31][0][:, :, ::-1])                     # (image 31 does look different unmirrored)


@pytest.mark.gpu
def test_scaled_kernel_at_the_source_size_equals_the_unscaled_kernel():
    from dsrg_amd import ops
    images, labels = [c[0] for c in _cases()], [c[1] for c in _cases()]
    placements = _placements(SOURCES)                                                   # Hs = H, Ws = W
    stage, desc = _stage(images, labels, placements)
    plain_stage, plain = _stage(images, labels, placements, scaled=False)
    assert "Hs" not in plain and desc["Hs"] == desc["H"] and desc["Ws"] == desc["W"] and torch.equal(stage, plain_stage)
    for scale, ignore in ((1.0, 255), (0.0039, 21)):
        got = ops.train_f_input_batch(stage, desc, CROP, ODD_MEAN, scale, ignore)
        want = ops.train_f_input_batch(stage, plain, CROP, ODD_MEAN, scale, ignore)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float(want[0].abs().max()) > 0 and len(torch.unique(want[1])) > 2


@pytest.mark.gpu
def test_train_f_input_with_scale_factors_end_to_end_equals_image_seg_data_layer(tmp_path):
    from dsrg_amd import data as D
    from dsrg_amd import input as I
    rng = np.random.default_rng(36)
    lst, root = _write_f_files(tmp_path, rng)
    params = dict(source=lst, root_folder=root, batch_size=3, crop_size=(17, 13), mean=ODD_MEAN, scale=0.0039, mirror=True,
                  ignore_label=21, scale_factors=FACTORS)
    seed = 6
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
            for n in range(4):                                                          # 12 images: two epochs of five and a wrap
                got = next(ld)
                layer.forward([], tops)
                for g, top in zip(got, tops):
                    assert g.is_cuda and g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(top.data)), n
                if kept:
                    assert all(torch.equal(t, c) for t, c in zip(*kept)), n
                kept = (got, [t.clone() for t in got])
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
    finally:
        random.setstate(states[0])
        np.random.set_state(states[1])


def _run_train(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


def _losses(out):
    rows = [ln for ln in out.splitlines() if ln.startswith("Iteration ")]
    values = [float(v) for ln in rows for v in re.findall(r"loss[-\w]* = ([-+.\dnaife]+)", ln)]
    return rows, values


def _done(out):
    ln = [ln for ln in out.splitlines() if ln.startswith("done: ")][-1].split()
    return int(ln[2]), (int(ln[4]), int(ln[5]))


@pytest.mark.gpu
def test_train_command_stage_f_with_scale_factors_in_a_child_process(tmp_path):
    rng = np.random.default_rng(37)
    lst, root = _write_f_files(tmp_path, rng, sizes=((70, 90), (50, 80), (66, 65), (100, 60), (65, 65)))
    common = ["--stage", "f", "--list", lst, "--root", root, "--scale-factors", "0.5,1,1.5", "--crop", "65", "--batch", "2", "--iters", "3",
              "--display", "1", "--workers", "2", "--seed", "3"]
    first = _run_train(common + ["--prefix", str(tmp_path / "a" / "model-f")], timeout=600)
    rows, values = _losses(first)
    assert len(rows) == 3 and len(values) == 3 and np.isfinite(values).all(), first[-2000:]
    again = _run_train(common + ["--prefix", str(tmp_path / "b" / "model-f")], timeout=600)
    assert _done(first)[0] == 3 and _done(again) == _done(first)                         # same seed, same weights, bit for bit
    assert _losses(again)[1] == values
