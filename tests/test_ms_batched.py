"""The fixed-size test-time loop (training/tools/test-ms.py) with its forwards batched across images.

CPU: the argument checks of dsrg_preprocess_ms_batch / dsrg_multiscale_unary_batch, the grouping helper of
predict_masks_ms_many, and the --forward-batch switch of `python -m dsrg_amd.predict`.
GPU: the batched unary against the single-image kernel (bit for bit), the batched preprocessing against inference.preprocess,
predict_masks_ms_many(forward_batch=G) / predict_masks_ms_batched against the staged composition (exact) and against the
per-image path (the project's agreement bar), and the batch-G graphs with a padded tail group on VGG16-ASPP."""
import ctypes

import numpy as np
import pytest
import torch

_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced


def _vp(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_multiscale_unary_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()

    def call(G=3, K=2, C=21, scores="fake", hs="fake", ws="fake", Hs="fake", Ws="fake", unary="fake", amax=None, sums=None):
        g, k = max(G, 1), max(K, 1)
        P = _vp([_FAKE] * k) if scores == "fake" else scores
        h = _i32([4] * k) if hs == "fake" else hs
        w = _i32([5] * k) if ws == "fake" else ws
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        u = _vp([_FAKE] * g) if unary == "fake" else unary
        return L.dsrg_multiscale_unary_batch(G, K, C, P, h, w, H, W, 1e-5, u, amax, sums, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=17) == _lib.ERR_INVALID and b"16" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"scales" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID
    assert call(C=97) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(C=0) == _lib.ERR_INVALID
    assert call(scores=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(scores=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(hs=None) == _lib.ERR_INVALID and call(ws=None) == _lib.ERR_INVALID
    assert call(Hs=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Ws=None) == _lib.ERR_INVALID
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and call(Ws=_i32([9, 9, 0])) == _lib.ERR_INVALID
    assert call(hs=_i32([4, 0])) == _lib.ERR_INVALID
    assert call(unary=None) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(unary=_vp([None] * 3)) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(amax=_vp([None, _FAKE, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(sums=_vp([_FAKE, _FAKE, None])) == _lib.ERR_INVALID
    assert call(unary=_vp([_FAKE, _FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(unary=None, sums=_vp([_FAKE, 264, _FAKE])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, C=96, Hs=_i32([16384]), Ws=_i32([16384])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_preprocess_ms_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(104.0, 117.0, 123.0)

    def call(G=3, cap=None, K=2, images="fake", Hs="fake", Ws="fake", sizes="fake", mean=mean3, out="fake"):
        g, k = max(G, 1), max(K, 1)
        P = _vp([_FAKE] * g) if images == "fake" else images
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        S = _i32([5] * k) if sizes == "fake" else sizes
        O = _vp([_FAKE] * k) if out == "fake" else out
        return L.dsrg_preprocess_ms_batch(G, G if cap is None else cap, K, P, H, W, S, mean, O, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=17) == _lib.ERR_INVALID and b"16" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"sizes" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID
    assert call(cap=2) == _lib.ERR_INVALID and b"capacity" in L.dsrg_last_error()
    assert call(images=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(images=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=None) == _lib.ERR_INVALID and call(Ws=None) == _lib.ERR_INVALID
    assert call(sizes=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(mean=None) == _lib.ERR_INVALID
    assert call(out=None) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and call(Ws=_i32([0, 9, 9])) == _lib.ERR_INVALID
    assert call(sizes=_i32([5, 0])) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, Hs=_i32([32768]), Ws=_i32([32768])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(cap=16, sizes=_i32([5, 8192])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_batched_entry_points_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dsrg_amd import _lib
    L = _lib.lib()
    rc = L.dsrg_multiscale_unary_batch(2, 1, 21, _vp([_FAKE]), _i32([4]), _i32([5]), _i32([8, 3]), _i32([8, 7]), 1e-5,
                                       _vp([_FAKE, 512]), None, None, None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()
    rc = L.dsrg_preprocess_ms_batch(2, 3, 1, _vp([_FAKE, 512]), _i32([8, 3]), _i32([8, 7]), _i32([5]),
                                    (ctypes.c_float * 3)(104.0, 117.0, 123.0), _vp([_FAKE]), None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()


def test_forward_groups_split_pad_and_keep_order():
    from dsrg_amd import inference as I
    from dsrg_amd import ops
    items = ["im%d" % k for k in range(9)]
    groups = list(I._forward_groups(iter(items), 4))                   # (any iterable: predict.py passes a generator)
    assert groups == [items[0:4], items[4:8], [items[8], None, None, None]]
    assert all(len(g) == 4 for g in groups)
    assert list(I._forward_groups(items[:8], 4)) == [items[0:4], items[4:8]]
    assert list(I._forward_groups(items[:3], 16)) == [items[:3] + [None] * 13]
    assert list(I._forward_groups([], 4)) == []
    for bad in (0, 17):
        with pytest.raises(ValueError):
            list(I._forward_groups(items, bad))
    assert tuple(ops.MEAN_PIXEL) == tuple(I.MEAN_PIXEL)


def test_predict_cli_rejects_forward_batch_at_relative_scales(capsys):
    from dsrg_amd import predict
    common = ["--model", "m", "--images", "i", "--dir", "d", "--output", "o"]
    with pytest.raises(SystemExit) as e:
        predict.parse_args(["--mode", "ms-f", "--forward-batch", "2"] + common)
    assert e.value.code == 2
    assert "--forward-batch is for --mode ms only" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse_args(["--mode", "ms", "--forward-batch", "17"] + common)
    assert predict.parse_args(["--mode", "ms-f", "--forward-batch", "1"] + common).forward_batch == 1
    assert predict.parse_args(["--mode", "ms-f"] + common).forward_batch == 1
    assert predict.parse_args(["--mode", "ms"] + common).forward_batch == 1
    assert predict.parse_args(["--mode", "ms", "--forward-batch", "8"] + common).forward_batch == 8


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
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


# output sizes mixed within a group: images under 64 pixels, pixel counts that are no multiple of 64 (37 x 53 = 30 blocks and
# 41 pixels: the blocks of the image after it follow a partial block), several blocks
_OUT = [(37, 53), (40, 31), (1, 1), (97, 131), (1, 57), (43, 1), (2, 3)]
_MAPS = [(1, 1), (2, 3), (5, 17), (17, 5), (3, 4), (12, 16), (6, 1), (13, 9)]


def _batched_scores(rng, Gcap, C, h, w, kind):
    """the three kinds of test_multiscale_f._scores, batched"""
    if kind == 0:
        a = rng.standard_normal((Gcap, C, h, w)) * 3.0
    elif kind == 1:
        a = rng.uniform(-300.0, 300.0, size=(Gcap, C, h, w))             # softmax far into the clamp
    else:
        a = rng.integers(-2, 3, size=(Gcap, C, h, w)) * 150.0            # +-300 with exact ties
    return torch.from_numpy(a.astype(np.float32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 8])
def test_multiscale_unary_batch_equals_the_single_image_kernel(K):
    from dsrg_amd import ops
    rng = np.random.default_rng(20 + K)
    names = ("unary", "argmax", "sum")
    case = 0
    for G in (1, 3, 8, 16):
        for C in (1, 2, 21, 96):
            case += 1
            Gcap = G + (case % 3)                                       # G, G + 1, G + 2 slices in the maps
            sizes = [_MAPS[(case + k) % len(_MAPS)] for k in range(K)]
            shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
            scores = [_batched_scores(rng, Gcap, C, h, w, (case + K) % 3) for h, w in sizes]
            got = ops.multiscale_unary_batch(scores, shapes, eps=1e-5, want=names)
            again = ops.multiscale_unary_batch(scores, shapes, eps=1e-5, want=names)
            assert len(got) == G
            for g, (H, W) in enumerate(shapes):
                want = ops.multiscale_unary([s[g:g + 1] for s in scores], H, W, eps=1e-5, want=names)
                for n, a, b, c in zip(names, got[g], want, again[g]):
                    assert a.shape == b.shape and a.dtype == b.dtype, (n, G, K, C, g)
                    assert torch.equal(a, b), "%s of image %d differs from the single-image kernel (G %d K %d C %d)" % (n, g, G, K, C)
                    assert torch.equal(a, c), "%s of image %d is not reproducible (G %d K %d C %d)" % (n, g, G, K, C)
            # one output class on its own, string and sequence forms of `want`
            only = ops.multiscale_unary_batch(scores, shapes, want="argmax")
            assert isinstance(only, list) and all(torch.equal(o, t[1]) for o, t in zip(only, got))
            default = ops.multiscale_unary_batch(scores, shapes)        # want=("unary",): 1-tuples
            assert all(len(o) == 1 and torch.equal(o[0], t[0]) for o, t in zip(default, got))


@pytest.mark.gpu
def test_multiscale_unary_batch_validates_like_the_single_image_front_end():
    from dsrg_amd import ops
    s = torch.zeros(3, 21, 4, 5, device="cuda")
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([s], [(8, 8)], want="probs")
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([s], [(8, 8)], want=())
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([], [(8, 8)])
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([s, torch.zeros(2, 21, 4, 5, device="cuda")], [(8, 8)])
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([s], [(8, 8)] * 4)                  # more images than slices
    with pytest.raises(ValueError):
        ops.multiscale_unary_batch([s.double()], [(8, 8)])
    with pytest.raises(ValueError):
        ops.preprocess_ms_batch([torch.zeros(4, 4, 3, device="cuda")], [5])          # not uint8
    with pytest.raises(ValueError):
        ops.preprocess_ms_batch([torch.zeros(4, 4, 3, dtype=torch.uint8, device="cuda")] * 2, [5], capacity=1)
    with pytest.raises(ValueError):
        ops.preprocess_ms_batch([torch.zeros(4, 4, 3, dtype=torch.uint8, device="cuda")], [5], out=[torch.zeros(1, 3, 6, 6, device="cuda")])


@pytest.mark.gpu
def test_preprocess_ms_batch_matches_preprocess():
    """Every |difference| <= 2 float32 ulps at 255: torch's fp64 interpolate may contract to FMA, which moves the rounded blend by at
    most one ulp of a value <= 255, and the two float32 mean subtractions add at most half an ulp each.  0.999 of all values bit-equal
    (the share test_multiscale_f demands of the unary kernel's sum); identity sizes bit-equal throughout"""
    from dsrg_amd import inference as I, ops
    rng = np.random.default_rng(31)
    shapes = [(33, 33), (120, 90), (1, 1), (1, 57), (43, 1), (2, 3)]
    images = [rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) for H, W in shapes]
    sizes = [1, 2, 17, 33]
    ref = {(i, S): I.preprocess(im, S) for i, im in enumerate(images) for S in sizes}          # computed once, shared
    bound = 2 * float(np.spacing(np.float32(255.0)))
    assert abs(bound - 3.05e-5) < 1e-7
    n = n_equal = 0
    worst = 0.0
    for G in (1, 3, 16):
        for start in range(0, len(images), 1 if G == 1 else len(images)):
            idx = [(start + g) % len(images) for g in range(G)]
            dev = [torch.from_numpy(images[i]).cuda() for i in idx]
            cap = G + 2
            got = ops.preprocess_ms_batch(dev, sizes, capacity=cap)
            again = ops.preprocess_ms_batch(dev, sizes, capacity=cap, out=[torch.full_like(o, 7.0) for o in got])
            assert len(got) == len(sizes)
            for S, o, o2 in zip(sizes, got, again):
                assert tuple(o.shape) == (cap, 3, S, S) and o.dtype == torch.float32 and o.is_contiguous()
                assert torch.equal(o, o2), "not reproducible / `out` buffers not fully written"
                assert (o[G:] == 0).all(), "padding slots must be zero"
                for g, i in enumerate(idx):
                    want = ref[(i, S)][0]
                    d = (o[g].double() - want.double()).abs()
                    worst = max(worst, float(d.max()))
                    assert float(d.max()) <= bound, (G, shapes[i], S, float(d.max()))
                    if shapes[i] == (S, S):
                        assert torch.equal(o[g], want), "identity size must be bit-equal"
                    n += d.numel()
                    n_equal += int((o[g] == want).sum())
    print("preprocess_ms_batch: %.6f of %d values bit-equal to inference.preprocess, largest difference %.3g (bound %.3g)"
          % (n_equal / n, n, worst, bound))
    assert n_equal >= 0.999 * n
    # the default capacity is the group, and `mean` is honoured
    a = ops.preprocess_ms_batch([torch.from_numpy(images[1]).cuda()], [17], mean=(0.0, 0.0, 0.0))[0]
    assert tuple(a.shape) == (1, 3, 17, 17)
    b = ops.preprocess_ms_batch([torch.from_numpy(images[1]).cuda()], [17])[0]
    assert torch.equal(a - torch.tensor(I.MEAN_PIXEL, device="cuda").view(1, 3, 1, 1), b)


_E2E_SHAPES = [(97, 131), (97, 131), (97, 131), (120, 90), (120, 90), (120, 90), (66, 70), (97, 131), (120, 90)]
_E2E_SIZES = (73, 97, 121)


def _e2e_images(seed):
    rng = np.random.default_rng(seed)
    return [_image(rng, H, W, kind=["smooth", "noise", "dark_corner"][k % 3]) for k, (H, W) in enumerate(_E2E_SHAPES)]


def _staged(fwd, ims, G, sizes, smooth):
    """the batched path composed from its stages: ops.preprocess_ms_batch, the same batch-G forwards (tail group padded), then per
    image ops.multiscale_unary on the slices and CRF_device(want="map") -> list of (H,W) int64 masks"""
    from dsrg_amd import ops
    from dsrg_amd.crf import CRF_device
    masks = []
    with torch.no_grad():
        for start in range(0, len(ims), G):
            part = ims[start:start + G]
            dev = [torch.from_numpy(im).cuda() for im in part]
            xs = ops.preprocess_ms_batch(dev, sizes, capacity=G)
            scores = [fwd(x).float().contiguous() for x in xs]          # (distinct sizes: every graph's static output stays valid)
            for g, im in enumerate(dev):
                sl = [s[g:g + 1] for s in scores]
                H, W = im.shape[0], im.shape[1]
                if smooth:
                    unary = ops.multiscale_unary(sl, H, W, eps=0.00001, want="unary")
                    masks.append(CRF_device(im, unary, scale_factor=1.0, want="map").cpu().numpy().astype(np.int64))
                else:
                    masks.append(ops.multiscale_unary(sl, H, W, eps=0.00001, want="argmax").cpu().numpy().astype(np.int64))
    return masks


def _assert_masks_equal(got, want, ims, tag):
    assert len(got) == len(want) == len(ims), tag
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], (tag, k)
        assert np.array_equal(a, b), "%s: mask %d differs from the staged composition on %d pixels" % (tag, k, int((a != b).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_predict_masks_ms_many_forward_batch_equals_the_staged_composition(graphed):
    from dsrg_amd import inference as I
    ims = _e2e_images(41)
    net = TinyNet().cuda().eval()
    G = 4

    def forward():
        return I.GraphedForward(net) if graphed else None

    ref_fwd = forward()
    want = _staged(ref_fwd or net, ims, G, _E2E_SIZES, True)
    want_plain = _staged(ref_fwd or net, ims, G, _E2E_SIZES, False)
    assert max(len(np.unique(m)) for m in want_plain) >= 2, "the stand-in net must give masks of several labels"
    for in_flight, batch in ((2, 1), (3, 2), (2, 2), (3, 1)):
        fwd = forward()
        got = list(I.predict_masks_ms_many(net, iter(ims), sizes=_E2E_SIZES, forward=fwd, in_flight=in_flight, batch=batch,
                                           forward_batch=G))
        _assert_masks_equal(got, want, ims, "in_flight %d batch %d" % (in_flight, batch))
        if graphed:
            assert len(fwd._g) == len(_E2E_SIZES)                      # one batch-G graph per size, the tail group included
            assert sorted(key[0] for key in fwd._g) == sorted((G, 3, S, S) for S in _E2E_SIZES)
    # the one-group form: smooth and not, a full group, a short group on its own and a short group padded to the capacity
    fwd = forward()
    for smooth, ref in ((True, want), (False, want_plain)):
        got = I.predict_masks_ms_batched(net, ims[0:4], smooth=smooth, sizes=_E2E_SIZES, forward=fwd) + \
            I.predict_masks_ms_batched(net, ims[4:8], smooth=smooth, sizes=_E2E_SIZES, forward=fwd, in_flight=2, batch=2) + \
            I.predict_masks_ms_batched(net, ims[8:9], smooth=smooth, sizes=_E2E_SIZES, forward=fwd, capacity=G)
        _assert_masks_equal(got, ref, ims, "predict_masks_ms_batched smooth=%s" % smooth)
    # forward_batch=1 is the per-image path
    one = list(I.predict_masks_ms_many(net, ims[:2], sizes=_E2E_SIZES, forward_batch=1))
    for a, im in zip(one, ims[:2]):
        assert np.array_equal(a, I.predict_mask_ms(net, im, sizes=_E2E_SIZES))


@pytest.mark.gpu
def test_predict_masks_ms_many_forward_batch_takes_float_images_through_preprocess():
    """non-uint8 images take inference.preprocess for their slot; with whole-number pixel values the masks are those of the uint8
    images up to the 2-ulp difference of the two preprocessing routes, which the exact staged comparison above does not cover"""
    from dsrg_amd import inference as I
    ims = _e2e_images(43)[:3]
    net = TinyNet().cuda().eval()
    mixed = [ims[0], ims[1].astype(np.float32), ims[2]]
    got = list(I.predict_masks_ms_many(net, mixed, sizes=_E2E_SIZES, forward_batch=2))
    want = list(I.predict_masks_ms_many(net, ims, sizes=_E2E_SIZES, forward_batch=2))
    assert len(got) == 3
    for a, b in zip(got, want):
        assert a.dtype == np.int64 and a.shape == b.shape and (a == b).mean() > 0.999


@pytest.mark.gpu
def test_predict_masks_ms_many_forward_batch_agrees_with_the_per_image_path():
    """batch-G and batch-1 forwards need not agree bit for bit: the bar of test_predict_mask_ms_f_vs_reference_restatement —
    agreement above 0.999 per image, every differing pixel with a top-2 margin below 1e-3 in the per-image path's CRF marginals
    (smooth) or probabilities (smooth=False)"""
    from dsrg_amd import inference as I
    from dsrg_amd.crf import CRF_device
    ims = _e2e_images(47)
    net = TinyNet().float().cuda().eval()
    got_smooth = list(I.predict_masks_ms_many(net, ims, sizes=_E2E_SIZES, forward_batch=4))
    got_plain = [m for s in range(0, len(ims), 4)
                 for m in I.predict_masks_ms_batched(net, ims[s:s + 4], smooth=False, sizes=_E2E_SIZES, capacity=4)]
    assert len(got_smooth) == len(got_plain) == len(ims)
    for k, im in enumerate(ims):
        with torch.no_grad():
            probs = I._probs_from_scores(I.multiscale_scores(net, im, _E2E_SIZES))
            unary = torch.log(probs).permute(1, 2, 0).contiguous()
            q = CRF_device(torch.as_tensor(im, device="cuda"), unary, scale_factor=1.0)
        for smooth, got, ref in ((True, got_smooth[k], q.cpu().numpy()), (False, got_plain[k], probs.permute(1, 2, 0).cpu().numpy())):
            want = I.predict_mask_ms(net, im, smooth=smooth, sizes=_E2E_SIZES)
            top2 = np.sort(ref, axis=2)[:, :, -2:]
            margin = top2[:, :, 1] - top2[:, :, 0]
            bad = got != want
            agree = 1.0 - bad.mean()
            print("image %d smooth=%s: agreement with predict_mask_ms %.6f; %d differing pixels, largest top-2 margin among them %.3g"
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
def test_forward_batch_on_vgg16_aspp_graphs_with_a_padded_tail_group():
    """the batch-2 graphs of VGG16-ASPP under bf16 autocast, 3 images (one full group and a padded tail group), against the
    staged composition on the same GraphedForward: exact"""
    from dsrg_amd import inference as I
    rng = np.random.default_rng(53)
    ims = [_image(rng, H, W, kind="noise") for H, W in ((97, 129), (120, 90), (97, 129))]
    sizes = (97, 129, 161)
    net = _vgg()
    fwd = I.GraphedForward(net)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = _staged(fwd, ims, 2, sizes, True)
        want_plain = _staged(fwd, ims, 2, sizes, False)
        got = list(I.predict_masks_ms_many(net, ims, sizes=sizes, forward=fwd, in_flight=2, forward_batch=2))
        got_plain = I.predict_masks_ms_batched(net, ims[:2], smooth=False, sizes=sizes, forward=fwd) + \
            I.predict_masks_ms_batched(net, ims[2:], smooth=False, sizes=sizes, forward=fwd, capacity=2)
    _assert_masks_equal(got, want, ims, "VGG16-ASPP forward_batch=2")
    _assert_masks_equal(got_plain, want_plain, ims, "VGG16-ASPP forward_batch=2, smooth=False")
    assert len(fwd._g) == len(sizes)
    labels = np.unique(np.concatenate([m.ravel() for m in got + got_plain]))
    print("VGG16-ASPP forward_batch=2: %d labels in the masks" % len(labels))
    assert len(labels) >= 2
