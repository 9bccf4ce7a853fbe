"""The relative-scale final test (training/tools/test-ms-f.py) with its forwards batched across same-sized images.

CPU: the scheduler inference.plan_size_groups, the argument checks of dsrg_preprocess_rect_batch, the --same-size-batch / --window
switches of `python -m dsrg_amd.predict`, and the numpy restatement of the kernel's arithmetic against
inference.preprocess_relative on the host.
GPU: the rectangular batched preprocessing against that restatement (bit for bit), against inference.preprocess_relative and
against its square sibling; predict_masks_ms_f_many(same_size_batch=G) against the staged composition (exact) and against the
per-image path (the project's agreement bar); one run on VGG16-ASPP through a bounded GraphedForward."""
import ctypes
import functools

import numpy as np
import pytest
import torch

_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced


def _vp(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- CPU: the scheduler -----------------------------------------------------------------------------------------------------------
def _trace(keys, G, window):
    """plan_size_groups over `keys` -> [(group, keys pulled when it was yielded, whether the input had ended)]"""
    from dsrg_amd import inference as I
    state = {"pulled": 0, "ended": False}

    def feed():
        for k in keys:
            state["pulled"] += 1
            yield k
        state["ended"] = True

    return [(g, state["pulled"], state["ended"]) for g in I.plan_size_groups(feed(), G, window)]


def _check_partition(groups, n, G):
    assert sorted(i for g in groups for i in g) == list(range(n)), "every index exactly once"
    for g in groups:
        assert 1 <= len(g) <= G and g == sorted(g), g


def test_plan_size_groups_worked_example_and_laziness():
    from dsrg_amd import inference as I
    keys = list("AABACAA")
    assert list(I.plan_size_groups(keys, 3, 4)) == [[0, 1, 3], [2], [4], [5, 6]]
    assert list(I.plan_size_groups(iter(keys), 3, 4)) == [[0, 1, 3], [2], [4], [5, 6]]       # (any iterable)
    # [0, 1, 3] is due at key 3 (four keys pulled), [2] at key 5 (5 + 1 - 2 = window); the rest at the end of the input
    assert _trace(keys, 3, 4) == [([0, 1, 3], 4, False), ([2], 6, False), ([4], 7, True), ([5, 6], 7, True)]
    # keys may be any hashable: the (H, W) pairs of the caller
    sizes = [(375, 500), (500, 375), (375, 500), (500, 375)]
    assert list(I.plan_size_groups(sizes, 2, 64)) == [[0, 2], [1, 3]]
    assert list(I.plan_size_groups([], 4, 4)) == []


def test_plan_size_groups_singletons_and_one_key():
    from dsrg_amd import inference as I
    keys = list("ABAABBBACA")
    singles = [[i] for i in range(len(keys))]
    assert list(I.plan_size_groups(keys, 1, 64)) == singles
    assert list(I.plan_size_groups(keys, 16, 1)) == singles
    assert [p for _, p, _ in _trace(keys, 16, 1)] == list(range(1, len(keys) + 1))            # each as soon as it is read
    assert list(I.plan_size_groups(["A"] * 11, 4, 64)) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert list(I.plan_size_groups(["A"] * 8, 4, 64)) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # one key under a window shorter than the group: the window cuts the groups
    assert list(I.plan_size_groups(["A"] * 7, 4, 3)) == [[0, 1, 2], [3, 4, 5], [6]]


@pytest.mark.parametrize("G,window", [(3, 6), (4, 2), (8, 5), (2, 64), (16, 16)])
def test_plan_size_groups_bounds_the_wait_of_a_rare_key(G, window):
    keys = ["A"] * 5 + ["B"] + ["A"] * 20 + ["C", "A", "C"] + ["A"] * 7
    tr = _trace(keys, G, window)
    _check_partition([g for g, _, _ in tr], len(keys), G)
    for g, pulled, ended in tr:
        assert max(g) <= pulled - 1, "a group cannot hold an input that was not read yet"
        # emitted while reading key i = pulled - 1: no later than window - 1 inputs after its oldest member
        assert (pulled - 1) - g[0] <= window - 1, (g, pulled)
        if not ended and len(g) < G:
            assert (pulled - 1) - g[0] == window - 1, "a partial group leaves exactly when its oldest member has waited out the window"
    rare = [(g, pulled) for g, pulled, _ in tr if 5 in g]
    assert rare == [([5], min(5 + window, len(keys)))]
    # the images held back never reach the window
    held = 0
    emitted = {}
    for g, pulled, _ in tr:
        emitted.setdefault(pulled, 0)
        emitted[pulled] += len(g)
    done = 0
    for i in range(len(keys)):
        done += emitted.get(i + 1, 0)
        held = max(held, i + 1 - done)
    assert held < window


def test_plan_size_groups_random_streams_partition_the_input():
    from dsrg_amd import inference as I
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(0, 60))
        keys = [int(k) for k in rng.choice(5, size=n, p=[0.55, 0.2, 0.1, 0.1, 0.05])]
        G, window = int(rng.integers(1, 17)), int(rng.integers(1, 20))
        groups = list(I.plan_size_groups(keys, G, window))
        _check_partition(groups, n, G)
        for g in groups:
            assert len(set(keys[i] for i in g)) == 1, "one key per group"


def test_plan_size_groups_rejects_bad_arguments_at_the_call():
    from dsrg_amd import inference as I
    for G, window in ((0, 4), (17, 4), (-1, 4), (4, 0), (4, -3)):
        with pytest.raises(ValueError):
            I.plan_size_groups(["A"], G, window)                       # (not only at the first group)


# ---- CPU: the C ABI and the command line --------------------------------------------------------------------------------------------
def test_preprocess_rect_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(104.0, 117.0, 123.0)

    def call(G=3, cap=None, K=2, images="fake", Hs="fake", Ws="fake", oh="fake", ow="fake", mean=mean3, out="fake"):
        g, k = max(G, 1), max(K, 1)
        P = _vp([_FAKE] * g) if images == "fake" else images
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        h = _i32([5] * k) if oh == "fake" else oh
        w = _i32([7] * k) if ow == "fake" else ow
        O = _vp([_FAKE] * k) if out == "fake" else out
        return L.dsrg_preprocess_rect_batch(G, G if cap is None else cap, K, P, H, W, h, w, mean, O, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error() and b"rect" in L.dsrg_last_error()
    assert call(G=17) == _lib.ERR_INVALID and b"16" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"sizes" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID
    assert call(cap=2) == _lib.ERR_INVALID and b"capacity" in L.dsrg_last_error()
    assert call(images=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(images=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=None) == _lib.ERR_INVALID and call(Ws=None) == _lib.ERR_INVALID
    assert call(oh=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(ow=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(mean=None) == _lib.ERR_INVALID
    assert call(out=None) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and call(Ws=_i32([0, 9, 9])) == _lib.ERR_INVALID
    assert call(oh=_i32([5, 0])) == _lib.ERR_INVALID and b"5x7" not in L.dsrg_last_error() and b"0x7" in L.dsrg_last_error()
    assert call(ow=_i32([-1, 7])) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, Hs=_i32([32768]), Ws=_i32([32768])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    # the bound is on capacity * 3 * h_k * w_k: a square target in a large group, and one long thin target on its own
    assert call(cap=16, oh=_i32([5, 8192]), ow=_i32([7, 8192])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(G=1, oh=_i32([5, 1 << 20]), ow=_i32([7, 1024])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_preprocess_rect_batch_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dsrg_amd import _lib
    L = _lib.lib()
    rc = L.dsrg_preprocess_rect_batch(2, 3, 1, _vp([_FAKE, 512]), _i32([8, 3]), _i32([8, 7]), _i32([5]), _i32([6]),
                                      (ctypes.c_float * 3)(104.0, 117.0, 123.0), _vp([_FAKE]), None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()


def test_predict_cli_same_size_batch_is_for_relative_scales(capsys):
    from dsrg_amd import predict
    common = ["--model", "m", "--images", "i", "--dir", "d", "--output", "o"]
    a = predict.parse_args(["--mode", "ms-f"] + common)
    assert a.same_size_batch == 1 and a.window == 64
    a = predict.parse_args(["--mode", "ms-f", "--same-size-batch", "8", "--window", "32", "--smooth"] + common)
    assert a.same_size_batch == 8 and a.window == 32 and a.smooth and a.forward_batch == 1
    assert predict.parse_args(["--mode", "ms-f", "--same-size-batch", "16"] + common).same_size_batch == 16
    for mode in (["--mode", "ms"], ["--mode", "gt", "--cues", "c"]):
        for flags in (["--same-size-batch", "2"], ["--window", "8"]):
            with pytest.raises(SystemExit) as e:
                predict.parse_args(mode + flags + common)
            assert e.value.code == 2
            assert "--same-size-batch and --window are for --mode ms-f only" in capsys.readouterr().err
        assert predict.parse_args(mode + common).same_size_batch == 1
    for flags in (["--same-size-batch", "0"], ["--same-size-batch", "17"], ["--window", "0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(["--mode", "ms-f"] + flags + common)
    capsys.readouterr()
    with pytest.raises(SystemExit):                                    # --forward-batch keeps its rejection beside the new switch
        predict.parse_args(["--mode", "ms-f", "--forward-batch", "2", "--same-size-batch", "2"] + common)
    assert "--forward-batch is for --mode ms only" in capsys.readouterr().err


# ---- the kernel's arithmetic, restated in numpy -----------------------------------------------------------------------------------
_PP_SHAPES = [(33, 47), (120, 90), (1, 1), (1, 57), (43, 1), (2, 3), (5, 4)]
_PP_FACTORS = (0.5, 0.75, 1.0, 1.25, 2.0)
_MEAN = (104.0, 117.0, 123.0)


@functools.lru_cache(maxsize=None)
def _pp_images():
    rng = np.random.default_rng(61)
    return tuple(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) for H, W in _PP_SHAPES)


def _targets(H, W):
    from dsrg_amd import inference as I
    return [(I.relative_size(H, f), I.relative_size(W, f)) for f in _PP_FACTORS]


@functools.lru_cache(maxsize=None)
def _restated(i, h, w):
    """image i of _pp_images zoomed to h x w as preprocess.hip states it, in numpy float64 (every product and sum is one numpy
    operation, rounded on its own): coordinate y * (H-1)/(h-1), two-tap blend l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11),
    one rounding to f32, BGR, f32 mean subtraction -> (3, h, w) float32.  Computed once per (image, target), shared, read-only."""
    im = _pp_images()[i]
    H, W = im.shape[0], im.shape[1]
    sy = (float(H - 1) / float(h - 1) if h > 1 else 0.0) * np.arange(h, dtype=np.float64)
    sx = (float(W - 1) / float(w - 1) if w > 1 else 0.0) * np.arange(w, dtype=np.float64)
    y0, x0 = sy.astype(np.int64), sx.astype(np.int64)
    y1, x1 = y0 + (y0 < H - 1), x0 + (x0 < W - 1)
    l1h, l1w = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
    l0h, l0w = 1.0 - l1h, 1.0 - l1w
    v = im[:, :, ::-1].astype(np.float64)                              # BGR
    v00, v01, v10, v11 = v[y0][:, x0], v[y0][:, x1], v[y1][:, x0], v[y1][:, x1]
    z = (l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)).astype(np.float32)
    out = np.ascontiguousarray((z - np.asarray(_MEAN, dtype=np.float32)).transpose(2, 0, 1))
    assert out.dtype == np.float32
    out.setflags(write=False)
    return out


def test_restatement_is_the_host_paths_arithmetic():
    """on exactly the inputs of the GPU tests the numpy restatement equals inference.preprocess_relative(device="cpu") bit for bit:
    the kernel is held to the host path's arithmetic, not to a second opinion"""
    from dsrg_amd import inference as I
    n = 0
    for i, im in enumerate(_pp_images()):
        for f, (h, w) in zip(_PP_FACTORS, _targets(*im.shape[:2])):
            want = I.preprocess_relative(im, f, device="cpu")[0].numpy()
            got = _restated(i, h, w)
            assert got.shape == want.shape == (3, h, w)
            assert np.array_equal(got, want), (im.shape, f)
            n += got.size
    assert n == 276546


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 16])
def test_preprocess_rect_batch_equals_the_float64_restatement_bit_for_bit(G):
    """every image at its own five relative targets (G = 1), and groups of mixed image sizes at one image's targets (the kernel
    does not need the group to share a size); capacity G + 2, the padding slots zero, `out=` buffers fully overwritten, two
    calls equal"""
    from dsrg_amd import ops
    images = _pp_images()
    dev_all = [torch.from_numpy(im).cuda() for im in images]
    n = 0
    for start in range(len(images) if G < 16 else 2):
        idx = [(start + g) % len(images) for g in range(G)]
        targets = _targets(*_PP_SHAPES[start])
        cap = G + 2
        dev = [dev_all[i] for i in idx]
        got = ops.preprocess_rect_batch(dev, targets, capacity=cap)
        again = ops.preprocess_rect_batch(dev, targets, capacity=cap, out=[torch.full_like(o, 7.0) for o in got])
        assert len(got) == len(targets)
        for (h, w), o, o2 in zip(targets, got, again):
            assert tuple(o.shape) == (cap, 3, h, w) and o.dtype == torch.float32 and o.is_contiguous()
            assert torch.equal(o, o2), "not reproducible / `out` buffers not fully written"
            assert (o[G:] == 0).all(), "padding slots must be zero"
            b = _bits(o)
            for g, i in enumerate(idx):
                want = _restated(i, h, w)
                assert np.array_equal(b[g], want.view(np.int32)), \
                    "image %s -> %dx%d in slot %d of %d: %d values differ from the restatement, largest difference %.3g" \
                    % (_PP_SHAPES[i], h, w, g, G, int((b[g] != want.view(np.int32)).sum()),
                       float(np.abs(o[g].cpu().numpy().astype(np.float64) - want).max()))
                n += want.size
    print("preprocess_rect_batch G=%d: %d values bit-equal to the float64 restatement" % (G, n))
    if G == 1:
        assert n == 276546


@pytest.mark.gpu
def test_preprocess_rect_batch_matches_preprocess_relative():
    """Every |difference| <= 2 float32 ulps at 255 (the bound and the reasoning of test_preprocess_ms_batch_matches_preprocess:
    torch's fp64 interpolate may contract to FMA, which moves the rounded blend by at most one ulp of a value <= 255, and the
    two float32 mean subtractions add at most half an ulp each); factor 1 is bit-equal"""
    from dsrg_amd import inference as I, ops
    bound = 2 * float(np.spacing(np.float32(255.0)))
    assert abs(bound - 3.05e-5) < 1e-7
    n = n_equal = 0
    worst = 0.0
    for im in _pp_images():
        H, W = im.shape[0], im.shape[1]
        got = ops.preprocess_rect_batch([torch.from_numpy(im).cuda()], _targets(H, W))
        for f, o in zip(_PP_FACTORS, got):
            want = I.preprocess_relative(im, f)
            assert o.shape == want.shape, (im.shape, f)
            d = (o.double() - want.double()).abs()
            worst = max(worst, float(d.max()))
            assert float(d.max()) <= bound, (im.shape, f, float(d.max()))
            if f == 1.0:
                assert torch.equal(o, want), "factor 1 must be bit-equal"
            n += d.numel()
            n_equal += int((o == want).sum())
    print("preprocess_rect_batch: %.6f of %d values bit-equal to inference.preprocess_relative, largest difference %.3g (bound %.3g)"
          % (n_equal / n, n, worst, bound))
    # `mean` is honoured, and the default capacity is the group
    im = torch.from_numpy(_pp_images()[1]).cuda()
    a = ops.preprocess_rect_batch([im], [(17, 23)], mean=(0.0, 0.0, 0.0))[0]
    assert tuple(a.shape) == (1, 3, 17, 23)
    assert torch.equal(a - torch.tensor(I.MEAN_PIXEL, device="cuda").view(1, 3, 1, 1), ops.preprocess_rect_batch([im], [(17, 23)])[0])


@pytest.mark.gpu
def test_preprocess_rect_batch_with_square_targets_equals_its_sibling():
    from dsrg_amd import ops
    images = _pp_images()
    sizes = [1, 2, 17, 33, 64]
    for G in (1, 3, 16):
        for start in range(0, len(images), 1 if G == 1 else len(images)):
            dev = [torch.from_numpy(images[(start + g) % len(images)]).cuda() for g in range(G)]
            a = ops.preprocess_rect_batch(dev, [(S, S) for S in sizes], capacity=G + 2)
            b = ops.preprocess_ms_batch(dev, sizes, capacity=G + 2)
            for S, x, y in zip(sizes, a, b):
                assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (G, start, S)


@pytest.mark.gpu
def test_preprocess_rect_batch_validates_like_its_sibling():
    from dsrg_amd import ops
    u8 = torch.zeros(4, 4, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([torch.zeros(4, 4, 3, device="cuda")], [(5, 6)])        # not uint8
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8.cpu()], [(5, 6)])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8] * 2, [(5, 6)], capacity=1)
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [(5, 6)], out=[torch.zeros(1, 3, 6, 5, device="cuda")])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [(5, 6)], out=[])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [(5, 0)])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [5])                                            # not (h, w) pairs
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([], [(5, 6)])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [])
    with pytest.raises(ValueError):
        ops.preprocess_rect_batch([u8], [(5, 6)], mean=(1.0, 2.0))


@pytest.mark.gpu
def test_side_streams_never_alias_the_capture_stream():
    """torch hands side streams out of a pool of 32 per device in turn; a CRF worker on the stream a forward thread captures a graph
    on would launch into the open capture.  Captures run on streams.capture_stream(), workers and forwards on side_stream()s"""
    from dsrg_amd import streams
    cap = streams.capture_stream("cuda")
    assert streams.capture_stream(torch.cuda.current_device()) is cap and streams.capture_stream() is cap
    seen = {streams.side_stream().cuda_stream for _ in range(70)}
    assert cap.cuda_stream not in seen and len(seen) > 1
    # the premise: torch's own pool does come round to it
    assert cap.cuda_stream in {torch.cuda.Stream().cuda_stream for _ in range(40)}


# ---- GPU: the batched relative-scale path -----------------------------------------------------------------------------------------
class TinyNet(torch.nn.Module):
    """a deterministic stand-in for the deploy net: stride-8 feature map with 21 outputs"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(21, 3, 9, 9, generator=g) * 0.02)

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.w, stride=8, padding=4)


def _image(rng, H, W, kind="smooth"):
    from dsrg_amd import synthetic as S
    im = (S.make_images(rng, 1, size=max(H, W), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
    return np.ascontiguousarray(im[:, :, ::-1]).clip(0, 255).astype(np.uint8)


# three sizes interleaved: with G = 3 the window decides the groups.  window 64: [0,1,3] [2,4,6] [5] [7,8]; window 4:
# [0,1,3] [2,4] [5] [6] [7,8] -- groups of 1, 2 and 3 images either way, emitted out of input order
_E2E_SHAPES = [(97, 131), (97, 131), (120, 90), (97, 131), (120, 90), (66, 70), (120, 90), (97, 131), (97, 131)]
_E2E_SCALES = (0.75, 1.0, 1.25)


def _e2e_images(seed):
    rng = np.random.default_rng(seed)
    return [_image(rng, H, W, kind=["smooth", "noise", "dark_corner"][k % 3]) for k, (H, W) in enumerate(_E2E_SHAPES)]


def _staged(fwd, ims, G, window, scales, smooth):
    """the batched path composed from its stages: the groups of plan_size_groups; per group ops.preprocess_rect_batch and the
    same batch-n forwards; then per image ops.multiscale_unary on the slices and CRF_device(want="map") -> list of (H,W) int64
    masks in input order"""
    from dsrg_amd import inference as I, ops
    from dsrg_amd.crf import CRF_device
    masks = [None] * len(ims)
    with torch.no_grad():
        for idx in I.plan_size_groups([im.shape[:2] for im in ims], G, window):
            dev = [torch.from_numpy(ims[i]).cuda() for i in idx]
            H, W = dev[0].shape[0], dev[0].shape[1]
            xs = ops.preprocess_rect_batch(dev, [(I.relative_size(H, s), I.relative_size(W, s)) for s in scales])
            assert len(set(tuple(x.shape) for x in xs)) == len(xs)      # distinct shapes: every graph's static output stays valid
            scores = [fwd(x).float().contiguous() for x in xs]
            for g, (i, im) in enumerate(zip(idx, dev)):
                sl = [s[g:g + 1] for s in scores]
                if smooth:
                    unary = ops.multiscale_unary(sl, H, W, eps=0.00001, want="unary")
                    masks[i] = CRF_device(im, unary, scale_factor=1.0, want="map").cpu().numpy().astype(np.int64)
                else:
                    masks[i] = ops.multiscale_unary(sl, H, W, eps=0.00001, want="argmax").cpu().numpy().astype(np.int64)
    return masks


def _assert_masks_equal(got, want, ims, tag):
    assert len(got) == len(want) == len(ims), tag
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], (tag, k, "masks must come back in input order")
        assert np.array_equal(a, b), "%s: mask %d differs from the staged composition on %d pixels" % (tag, k, int((a != b).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_predict_masks_ms_f_many_same_size_batch_equals_the_staged_composition(graphed):
    from dsrg_amd import inference as I
    ims = _e2e_images(71)
    net = TinyNet().cuda().eval()
    G = 3
    assert list(I.plan_size_groups([im.shape[:2] for im in ims], G, 64)) == [[0, 1, 3], [2, 4, 6], [5], [7, 8]]
    assert list(I.plan_size_groups([im.shape[:2] for im in ims], G, 4)) == [[0, 1, 3], [2, 4], [5], [6], [7, 8]]
    ref_fwd = I.GraphedForward(net) if graphed else None
    fwd = I.GraphedForward(net) if graphed else None                   # (kept over the runs: later runs write the static inputs)
    for window in (4, 64):
        want = _staged(ref_fwd or net, ims, G, window, _E2E_SCALES, True)
        want_plain = _staged(ref_fwd or net, ims, G, window, _E2E_SCALES, False)
        assert max(len(np.unique(m)) for m in want_plain) >= 2, "the stand-in net must give masks of several labels"
        for in_flight, batch in ((2, 1), (3, 2), (2, 3)):
            got = list(I.predict_masks_ms_f_many(net, iter(ims), scales=_E2E_SCALES, forward=fwd, in_flight=in_flight, batch=batch,
                                                 same_size_batch=G, window=window))
            _assert_masks_equal(got, want, ims, "window %d in_flight %d batch %d" % (window, in_flight, batch))
        got = list(I.predict_masks_ms_f_many(net, iter(ims), scales=_E2E_SCALES, forward=fwd, same_size_batch=G, window=window,
                                             smooth=False))
        _assert_masks_equal(got, want_plain, ims, "window %d smooth=False" % window)
    if graphed:                                                        # a graph per (n, size, scale) that occurred, none padded to G
        have = sorted(key[0] for key in fwd._g)
        want_keys = sorted((n, 3, I.relative_size(H, s), I.relative_size(W, s))
                           for n, (H, W) in ((3, (97, 131)), (2, (97, 131)), (3, (120, 90)), (2, (120, 90)), (1, (120, 90)),
                                             (1, (66, 70))) for s in _E2E_SCALES)
        assert have == want_keys
    # same_size_batch=1 is the per-image path, with and without the CRF
    for smooth in (True, False):
        one = list(I.predict_masks_ms_f_many(net, ims[1:4], scales=_E2E_SCALES, same_size_batch=1, smooth=smooth))
        assert len(one) == 3
        for a, im in zip(one, ims[1:4]):
            assert np.array_equal(a, I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth))


@pytest.mark.gpu
def test_predict_masks_ms_f_many_same_size_batch_argument_errors_and_float_images():
    from dsrg_amd import inference as I
    ims = _e2e_images(73)[:4]
    net = TinyNet().cuda().eval()
    for kw in (dict(same_size_batch=0), dict(same_size_batch=17), dict(same_size_batch=2, window=0),
               dict(same_size_batch=2, fused=False)):
        with pytest.raises(ValueError):
            list(I.predict_masks_ms_f_many(net, ims, **kw))
    # a relative size below one pixel is refused before any launch of its group
    with pytest.raises(ValueError):
        list(I.predict_masks_ms_f_many(net, [np.zeros((4, 1, 3), np.uint8)] * 2, scales=(0.25, 1.0), same_size_batch=2))
    # non-uint8 images take inference.preprocess_relative for their slot; with whole-number pixel values the masks are those of
    # the uint8 images up to the 2-ulp difference of the two preprocessing routes
    mixed = [ims[0], ims[1].astype(np.float32), ims[2], ims[3]]
    got = list(I.predict_masks_ms_f_many(net, mixed, same_size_batch=2))
    want = list(I.predict_masks_ms_f_many(net, ims, same_size_batch=2))
    assert len(got) == 4
    for a, b in zip(got, want):
        assert a.dtype == np.int64 and a.shape == b.shape and (a == b).mean() > 0.999


@pytest.mark.gpu
def test_predict_masks_ms_f_many_same_size_batch_agrees_with_the_per_image_path():
    """batch-n and batch-1 forwards need not agree bit for bit: the bar of test_ms_batched for the fixed-size path — agreement
    above 0.999 per image, every differing pixel with a top-2 margin below 1e-3 in the per-image path's CRF marginals (smooth) or
    probabilities (smooth=False)"""
    from dsrg_amd import inference as I
    from dsrg_amd.crf import CRF_device
    ims = _e2e_images(79)
    net = TinyNet().float().cuda().eval()
    got_smooth = list(I.predict_masks_ms_f_many(net, ims, scales=_E2E_SCALES, same_size_batch=3))
    got_plain = list(I.predict_masks_ms_f_many(net, ims, scales=_E2E_SCALES, same_size_batch=3, smooth=False))
    assert len(got_smooth) == len(got_plain) == len(ims)
    for k, im in enumerate(ims):
        with torch.no_grad():
            unary = I._relative_unary(net, im, _E2E_SCALES, "cuda", None, True, True)         # the per-image path's log-probabilities
            q = CRF_device(torch.as_tensor(im, device="cuda"), unary, scale_factor=1.0)
        for smooth, got, ref in ((True, got_smooth[k], q.cpu().numpy()), (False, got_plain[k], np.exp(unary.double().cpu().numpy()))):
            want = I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth)
            top2 = np.sort(ref, axis=2)[:, :, -2:]
            margin = top2[:, :, 1] - top2[:, :, 0]
            bad = got != want
            agree = 1.0 - bad.mean()
            print("image %d smooth=%s: agreement with predict_mask_ms_f %.6f; %d differing pixels, largest top-2 margin among them %.3g"
                  % (k, smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0))
            assert got.shape == want.shape and got.dtype == np.int64
            assert agree > 0.999
            assert not bad.any() or margin[bad].max() < 1e-3


def _vgg(num_classes=21, seed=0):
    """VGG16-ASPP in eval mode with He-initialised convolutions and zero biases, so that the scores of a random net vary over the
    image and the masks hold several labels"""
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(seed)
    net = VGG16ASPP(num_classes=num_classes)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                torch.nn.init.zeros_(m.bias)
    return net.cuda().to(memory_format=torch.channels_last).eval()


@pytest.mark.gpu
def test_same_size_batch_on_vgg16_aspp_through_a_bounded_graphed_forward():
    """VGG16-ASPP under bf16 autocast, 5 images of 2 sizes at same_size_batch 2 (two full groups and a partial one of one image,
    which is not padded) through GraphedForward(max_shapes=4, capture_after=2): the staged composition runs every shape once
    (eagerly), the path under test then captures them, dropping the least recently used graphs on the way; the masks are equal
    (a replayed forward equals the eager one bit for bit: test_bounded_graphed_forward)"""
    from dsrg_amd import inference as I
    rng = np.random.default_rng(83)
    shapes = ((97, 129), (120, 90), (97, 129), (97, 129), (120, 90))
    ims = [_image(rng, H, W, kind="noise") for H, W in shapes]
    net = _vgg()
    fwd = I.GraphedForward(net, max_shapes=4, capture_after=2)
    assert list(I.plan_size_groups(shapes, 2, 64)) == [[0, 2], [1, 4], [3]]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = _staged(fwd, ims, 2, 64, _E2E_SCALES, True)
        assert len(fwd._g) == 0
        got = list(I.predict_masks_ms_f_many(net, ims, scales=_E2E_SCALES, forward=fwd, in_flight=2, batch=2, same_size_batch=2))
        assert 0 < len(fwd._g) <= 4
        want_plain = _staged(fwd, ims, 2, 64, _E2E_SCALES, False)
        got_plain = list(I.predict_masks_ms_f_many(net, ims, scales=_E2E_SCALES, forward=fwd, same_size_batch=2, smooth=False))
    _assert_masks_equal(got, want, ims, "VGG16-ASPP same_size_batch=2")
    _assert_masks_equal(got_plain, want_plain, ims, "VGG16-ASPP same_size_batch=2, smooth=False")
    labels = np.unique(np.concatenate([m.ravel() for m in got + got_plain]))
    print("VGG16-ASPP same_size_batch=2: %d labels in the masks" % len(labels))
    assert len(labels) >= 2
