"""Multi-scale, mirrored pseudo-label generation (`--mode gt-ms`; no counterpart in the reference): the label-restricted pass of
generate_train_gt.py as a probability ensemble over K sizes, each optionally with its mirror.

CPU: the argument checks of dsrg_train_gt_ensemble_batch, the limits of the gt-ms functions and `--mode gt-ms` of
`python -m dsrg_amd.predict`.
GPU: one size without flip against ops.train_gt_unary_batch and both against its outputs recorded before the two shared their
kernels (bit for bit); the definition restated from the single-map case's exact zoomed probabilities (anchored by that record and
by test_train_gt.py's float64 restatement) and numpy float32 (bit for bit), the log against the kernel's own probabilities, the labels against the
selection rule in numpy (exact); a group against single-image calls with NaN in the unused slices; predict_train_gt_ms_many
against its staged composition (exact), against predict_train_gt_many at one size (exact) and against the torch composition
predict_train_gt_ms (the project's agreement bar)."""
import ctypes

import numpy as np
import pytest
import torch

_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced
_EPS = 1e-5


def _vp(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_train_gt_ensemble_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(_FAKE)

    def call(G=3, K=2, flip=0, C=21, scores="fake", hs="fake", ws="fake", Hs="fake", Ws="fake", sel=None, nsel=None, stride=0,
             work=one, unary="fake", probs=None, labels=None):
        g, k = max(G, 1), max(K, 1)
        s = _vp([_FAKE] * k) if scores == "fake" else scores
        h = _i32([4] * k) if hs == "fake" else hs
        w = _i32([5] * k) if ws == "fake" else ws
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        u = _vp([_FAKE] * g) if unary == "fake" else unary
        return L.dsrg_train_gt_ensemble_batch(G, K, flip, C, s, h, w, H, W, 1e-5, sel, nsel, stride, 0.0, work, u, probs, labels, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=17) == _lib.ERR_INVALID and b"1..16 images" in L.dsrg_last_error()
    assert call(G=9, flip=1) == _lib.ERR_INVALID and b"1..8 images" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"sizes" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID and b"1..8 sizes" in L.dsrg_last_error()
    assert call(K=5, flip=1) == _lib.ERR_INVALID and b"1..4 sizes" in L.dsrg_last_error()
    assert call(C=0) == _lib.ERR_INVALID and b"labels" in L.dsrg_last_error()
    assert call(C=97) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(scores=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(scores=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"score map 1 is NULL" in L.dsrg_last_error()
    assert call(hs=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(ws=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Ws=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(work=None) == _lib.ERR_INVALID and b"workspace" in L.dsrg_last_error()
    assert call(hs=_i32([4, 0])) == _lib.ERR_INVALID and b"score map 1 is 0x5" in L.dsrg_last_error()
    assert call(ws=_i32([0, 5])) == _lib.ERR_INVALID and b"score map 0" in L.dsrg_last_error()
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and b"output 1" in L.dsrg_last_error()
    assert call(Ws=_i32([9, 9, 0])) == _lib.ERR_INVALID and b"output 2" in L.dsrg_last_error()
    assert call(unary=None) == _lib.ERR_INVALID and b"no output" in L.dsrg_last_error()
    assert call(unary=_vp([None] * 3)) == _lib.ERR_INVALID and b"no output" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(probs=_vp([None, _FAKE, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(labels=_vp([_FAKE, _FAKE, None])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, _FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(unary=None, probs=_vp([_FAKE, 264, _FAKE])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, C=96, Hs=_i32([16384]), Ws=_i32([16384])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(G=1, C=96, hs=_i32([4, 8192]), ws=_i32([5, 8192])) == _lib.ERR_UNSUPPORTED
    assert b"score map 1 holds >= 2^31" in L.dsrg_last_error()
    # labels need the lists; a list holds 1..128 entries of [0, C) and fits the stride
    lab = _vp([_FAKE] * 3)
    good, n3 = _i32([0, 3, 7] * 3), _i32([3, 3, 3])
    assert call(labels=lab) == _lib.ERR_INVALID and b"selection" in L.dsrg_last_error()
    assert call(labels=lab, sel=good, nsel=None, stride=3) == _lib.ERR_INVALID and b"selection" in L.dsrg_last_error()
    assert call(labels=lab, sel=good, nsel=_i32([3, 0, 3]), stride=3) == _lib.ERR_INVALID and b"1..128" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0] * 3 * 129), nsel=_i32([3, 129, 3]), stride=129) == _lib.ERR_INVALID
    assert b"1..128" in L.dsrg_last_error() and b"image 1" in L.dsrg_last_error()
    assert call(labels=lab, sel=good, nsel=n3, stride=2) == _lib.ERR_INVALID and b"select_stride" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0, 3, 7, 0, 21, 7, 0, 3, 7]), nsel=n3, stride=3) == _lib.ERR_INVALID
    assert b"outside [0, 21)" in L.dsrg_last_error() and b"image 1" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0, 3, 7, 0, 3, 7, 0, 3, -1]), nsel=n3, stride=3) == _lib.ERR_INVALID
    assert b"outside" in L.dsrg_last_error()
    if not torch.cuda.is_available():                                 # valid calls reach the device: the limits themselves are legal
        assert call() == _lib.ERR_HIP
        assert call(G=16, K=8) == _lib.ERR_HIP
        assert call(G=8, K=4, flip=1) == _lib.ERR_HIP
        assert call(labels=lab, sel=good, nsel=n3, stride=3) == _lib.ERR_HIP


def test_predict_cli_gt_ms_mode(capsys):
    from dsrg_amd import predict
    common = ["--model", "m", "--images", "i", "--dir", "d", "--output", "o"]

    def rejected(args, text):
        with pytest.raises(SystemExit) as e:
            predict.parse_args(args + common)
        assert e.value.code == 2
        assert text in capsys.readouterr().err

    a = predict.parse_args(["--mode", "gt-ms", "--cues", "c"] + common)
    assert a.mode == "gt-ms" and a.cues == "c" and a.scales is None and not a.flip and a.forward_batch == 1 and not a.smooth
    a = predict.parse_args(["--mode", "gt-ms", "--cues", "c", "--flip", "--forward-batch", "8", "--scales", "97,129,161,193", "--smooth",
                            "--backbone", "resnet101", "--fp32"] + common)
    assert a.flip is True and a.forward_batch == 8 and a.scales == "97,129,161,193" and a.smooth and a.fp32
    assert predict.parse_args(["--mode", "gt-ms", "--cues", "c", "--scales", "1,2,3,4,5,6,7,8", "--forward-batch", "16"] + common)
    rejected(["--mode", "gt-ms", "--cues", "c", "--flip", "--scales", "97,129,161,193,225"], "at most 4 scales")
    rejected(["--mode", "gt-ms", "--cues", "c", "--scales", "1,2,3,4,5,6,7,8,9"], "at most 8 sizes")
    rejected(["--mode", "gt-ms", "--cues", "c", "--forward-batch", "9", "--flip"], "at most 8")
    rejected(["--mode", "gt-ms"], "--cues")
    rejected(["--mode", "gt-ms", "--cues", "c", "--same-size-batch", "2"], "ms-f only")


def test_gt_ms_limits_raise_before_any_launch():
    from dsrg_amd import inference as I
    im = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="1..8 sizes"):
        next(I.predict_train_gt_ms_many(None, [(im, [1])], sizes=range(1, 10)))
    with pytest.raises(ValueError, match="1..8 sizes"):
        next(I.predict_train_gt_ms_many(None, [(im, [1])], sizes=()))
    with pytest.raises(ValueError, match="1..4 sizes"):
        next(I.predict_train_gt_ms_many(None, [(im, [1])], sizes=range(1, 6), flip=True))
    with pytest.raises(ValueError, match="at most 8 images"):
        next(I.predict_train_gt_ms_many(None, [(im, [1])] * 9, forward_batch=9, flip=True))
    with pytest.raises(ValueError, match="forward_batch"):
        next(I.predict_train_gt_ms_many(None, [(im, [1])], forward_batch=17))
    with pytest.raises(ValueError, match="1..4 sizes"):
        I.predict_train_gt_ms(None, im, [1], sizes=range(1, 6), flip=True)


# ---- GPU: the ensemble kernel ------------------------------------------------------------------------------------------------------
import train_gt_golden_cases as golden                            # noqa: E402
from test_ms_batched import TinyNet, _batched_scores, _image    # noqa: E402  (shared fixtures)

# w odd, even and small; outputs below 64 pixels, no multiple of 64, several workgroups per image (391 = 6 * 64 + 7: the image
# after it starts behind a partial block)
_MAPS = [(4, 5), (6, 6), (9, 7), (1, 3)]
_OUT = [(9, 13), (1, 1), (33, 2), (17, 23)]
_CS = (5, 21, 96)
_NAMES = ("probs", "unary", "labels")


def _lists(rng, G, C):
    """one list per image: 1..4 labels of [0, C), any order, duplicates allowed; the first unsorted with a duplicate"""
    lists = [[int(c) for c in rng.integers(0, C, size=int(rng.integers(1, 5)))] for _ in range(G)]
    lists[0] = [C - 1, 0, 2, C - 1]
    return lists


def _select_host(v, sel, t=0.0):
    """the rule on the host: sel[first arg-max of v[..., sel]], 255 where the maximum over all labels is below t > 0"""
    sel = np.asarray(sel)
    out = sel[np.argmax(v[..., sel], axis=-1)]
    if t and t > 0:
        out = np.where(v.max(-1) < np.float32(t), 255, out)
    return out


def _maps(rng, K, Gcap, C, case, kind):
    return [_batched_scores(rng, Gcap, C, *_MAPS[(case + k) % len(_MAPS)], kind) for k in range(K)]


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 16])
def test_one_size_without_flip_is_train_gt_unary_batch_bit_for_bit(G):
    """the two ops against each other, and both against the outputs that train_gt_unary_batch's own kernels gave before it became
    the ensemble's K = 1 case (train_gt_golden_cases: sha256 of every output, the arrays at C = 5)"""
    from dsrg_amd import ops
    rng = np.random.default_rng(100 + G)
    case = 0
    for C in _CS:
        for h, w in _MAPS:
            case += 1
            scores = _batched_scores(rng, G + case % 2, C, h, w, case % 3)
            shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
            select = _lists(rng, G, C)
            t = (None, 0.5)[case % 2]
            got = ops.train_gt_ensemble_batch([scores], shapes, eps=_EPS, want=_NAMES, select=select, ignore_below=t)
            want = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want=_NAMES, select=select, ignore_below=t)
            assert len(got) == len(want) == G
            for g in range(G):
                for n, a, b in zip(_NAMES, got[g], want[g]):
                    assert a.shape == b.shape and a.dtype == b.dtype, (n, G, C, g)
                    assert torch.equal(a, b), "%s of image %d differs from train_gt_unary_batch (G %d C %d map %dx%d)" % (n, g, G, C, h, w)
            golden.assert_recorded("train_gt_ensemble_batch", G, case, scores, got)
            golden.assert_recorded("train_gt_unary_batch", G, case, scores, want)
    only = ops.train_gt_ensemble_batch([scores], shapes, eps=_EPS, want="unary")                # string form, no lists needed
    assert isinstance(only, list) and all(torch.equal(o, t3[1]) for o, t3 in zip(only, got))
    default = ops.train_gt_ensemble_batch([scores], shapes, eps=_EPS)                          # want=("unary",): 1-tuples
    assert all(len(o) == 1 and torch.equal(o[0], t3[1]) for o, t3 in zip(default, got))


def _restated(scores, shapes, flip, eps):
    """the definition from the single-map case (held to its recorded outputs and to the float64 / scipy restatement of
    test_train_gt.py): every z_m exactly, as ops.train_gt_unary_batch(eps=0.0, want="probs") on the slices of map k (the mirror
    slices through torch.flip), then in numpy float32 and in list order the sum, / M, the clamp -> one (H, W, C) float32 array per
    image"""
    from dsrg_amd import ops
    G, per = len(shapes), 2 if flip else 1
    zs = []                                                           # zs[m][g], m in list order
    for s in scores:
        zs.append(ops.train_gt_unary_batch(s[0:per * G:per].contiguous(), shapes, eps=0.0, want="probs"))
        if flip:
            zs.append(ops.train_gt_unary_batch(torch.flip(s[1:per * G:per], (-1,)).contiguous(), shapes, eps=0.0, want="probs"))
    M = len(zs)
    out = []
    for g in range(G):
        acc = zs[0][g].cpu().numpy().copy()
        assert acc.dtype == np.float32
        for m in range(1, M):
            acc += zs[m][g].cpu().numpy()
        if M > 1:
            acc = acc / np.float32(M)
        assert acc.dtype == np.float32
        out.append(np.maximum(acc, np.float32(eps)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_ensemble_equals_the_definition_bit_for_bit(G, flip):
    """probs: every value equals the restatement (_restated).  unary: within 2 float32 ulps of the float64 logarithm of the kernel's
    own probability (the bar of test_train_gt_probs_against_float64_restatement_and_unary_against_probs).  labels: the selection
    rule applied in numpy to the returned probs, exactly"""
    from dsrg_amd import ops
    rng = np.random.default_rng(200 + 10 * G + flip)
    per = 2 if flip else 1
    worst_log = 0.0
    case = 0
    for C in _CS:
        for kind in (0, 2):                                           # smooth scores; +-300 with exact ties, deep in the clamp
            case += 1
            scores = _maps(rng, 3, per * G + case % 2, C, case, kind)
            assert len({tuple(s.shape[2:]) for s in scores}) == 3
            shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
            select = _lists(rng, G, C)
            want = _restated(scores, shapes, flip, _EPS)
            for t in (None, 0.3, 1.5)[case % 2::2]:
                got = ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=_EPS, want=_NAMES, select=select, ignore_below=t)
                for g, (H, W) in enumerate(shapes):
                    probs, unary, lab = (x.cpu().numpy() for x in got[g])
                    assert probs.dtype == np.float32 and probs.shape == (H, W, C) and unary.shape == (H, W, C)
                    assert np.array_equal(probs, want[g]), "probs: G %d flip %s C %d kind %d image %d: %d of %d values differ" % (
                        G, flip, C, kind, g, int((probs != want[g]).sum()), probs.size)
                    assert probs.min() >= np.float32(_EPS)
                    lg = np.log(probs.astype(np.float64))
                    ulp = np.spacing(np.abs(lg).astype(np.float32)).astype(np.float64)
                    r = np.abs(unary.astype(np.float64) - lg) / ulp
                    worst_log = max(worst_log, float(r.max()))
                    assert r.max() <= 2.0, "unary: G %d flip %s C %d image %d: %.3g ulps" % (G, flip, C, g, r.max())
                    assert lab.dtype == np.int32 and lab.shape == (H, W)
                    assert np.array_equal(lab, _select_host(probs, select[g], t)), (G, flip, C, kind, g, t)
                    if t and t > 1:
                        assert (lab == 255).all()
                    if not t:
                        assert set(np.unique(lab)) <= set(select[g])
    print("train_gt_ensemble_batch G %d flip %s: probs bit-equal to the restatement; worst |unary - log(probs)| = %.3f ulps"
          % (G, flip, worst_log))


@pytest.mark.gpu
def test_mirror_slices_are_read_reversed_and_change_the_result():
    """a map whose mirror slice is torch.flip of its plain slice gives the plain result (z + z) / 2 = z; an unrelated mirror slice
    does not"""
    from dsrg_amd import ops
    rng = np.random.default_rng(5)
    s = _batched_scores(rng, 2, 21, 9, 7, 0)
    plain = ops.train_gt_ensemble_batch([s[0:1].contiguous()], [(17, 23)], eps=_EPS, want="probs")[0]
    pair = torch.cat([s[0:1], torch.flip(s[0:1], (-1,))]).contiguous()
    assert torch.equal(ops.train_gt_ensemble_batch([pair], [(17, 23)], flip=True, eps=_EPS, want="probs")[0], plain)
    assert not torch.equal(ops.train_gt_ensemble_batch([s], [(17, 23)], flip=True, eps=_EPS, want="probs")[0], plain)


@pytest.mark.gpu
def test_a_group_equals_single_image_calls_and_ignores_unused_slices():
    from dsrg_amd import ops
    rng = np.random.default_rng(7)
    for flip, G, Gcap in ((True, 8, 19), (False, 3, 5)):
        per = 2 if flip else 1
        for C in (5, 21):
            scores = _maps(rng, 3, Gcap, C, C, 0)
            for s in scores:
                s[per * G:] = float("nan")
            shapes = [_OUT[(C + g) % len(_OUT)] for g in range(G)]
            select = _lists(rng, G, C)
            got = ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=_EPS, want=_NAMES, select=select, ignore_below=0.3)
            again = ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=_EPS, want=_NAMES, select=select, ignore_below=0.3)
            for g in range(G):
                sl = [s[per * g:per * (g + 1)].contiguous() for s in scores]
                want = ops.train_gt_ensemble_batch(sl, [shapes[g]], flip=flip, eps=_EPS, want=_NAMES, select=[select[g]],
                                                   ignore_below=0.3)[0]
                for n, a, b, c in zip(_NAMES, got[g], want, again[g]):
                    assert torch.isfinite(a.float()).all(), "%s of image %d is not finite (flip %s)" % (n, g, flip)
                    assert torch.equal(a, b), "%s of image %d differs from the G = 1 call (flip %s C %d)" % (n, g, flip, C)
                    assert torch.equal(a, c), "%s of image %d is not reproducible (flip %s C %d)" % (n, g, flip, C)


@pytest.mark.gpu
def test_train_gt_ensemble_batch_validates_its_arguments():
    from dsrg_amd import ops
    s = torch.zeros(4, 21, 4, 5, device="cuda")
    for bad in (dict(scores=s), dict(scores=[]), dict(want="sum"), dict(want=()), dict(shapes=[(8, 8)] * 5),
                dict(shapes=[(8, 8)] * 3, flip=True), dict(scores=[s, s[:3]]), dict(scores=[s.double()]), dict(want="labels"),
                dict(want="labels", select=[[0, 21]]), dict(want="labels", select=[[0], [1]])):
        kw = dict(scores=[s], shapes=[(8, 8)])
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.train_gt_ensemble_batch(**kw)
    from dsrg_amd._lib import DsrgError
    with pytest.raises(DsrgError):
        ops.train_gt_ensemble_batch([s] * 9, [(8, 8)])
    with pytest.raises(DsrgError):
        ops.train_gt_ensemble_batch([s] * 5, [(8, 8)], flip=True)


# ---- GPU: end to end ---------------------------------------------------------------------------------------------------------------
_E2E_SHAPES = [(40, 56), (40, 56), (33, 47), (40, 56), (33, 47)]      # groups of 4: one full group, a tail group with padding
_E2E_SIZES = (33, 49)


def _e2e_items(seed, shapes=_E2E_SHAPES):
    rng = np.random.default_rng(seed)
    ims = [_image(rng, H, W, kind=["smooth", "noise", "dark_corner"][k % 3]) for k, (H, W) in enumerate(shapes)]
    return ims, [[int(c) for c in rng.choice(np.arange(1, 21), size=1 + k % 3, replace=False)] for k in range(len(ims))]


def _staged_gt_ms(fwd, ims, labels, G, sizes, flip, smooth):
    """predict_train_gt_ms_many composed from its stages: the launch of _group_inputs (ops.preprocess_ms_batch, with flip
    ops.preprocess_rect_mirror_batch), the same batched forwards (tail group padded), then per image
    ops.train_gt_ensemble_batch at G = 1 on its slices and CRF_device_many with the list, or the kernel's own labels"""
    from dsrg_amd import inference as I, ops
    from dsrg_amd.crf import CRF_device_many
    per = 2 if flip else 1
    masks = []
    with torch.no_grad():
        for start in range(0, len(ims), G):
            dev = [torch.from_numpy(im).cuda() for im in ims[start:start + G]]
            if flip:
                xs = ops.preprocess_rect_mirror_batch(dev, [(S, S) for S in sizes], capacity=2 * G)
            else:
                xs = ops.preprocess_ms_batch(dev, sizes, capacity=G)
            scores = [fwd(x).float().contiguous() for x in xs]        # (distinct sizes: every graph's static output stays valid)
            triples = []
            for g, im in enumerate(dev):
                sel = I.train_gt_selection(labels[start + g])
                sl = [s[per * g:per * (g + 1)].contiguous() for s in scores]
                shape = [(im.shape[0], im.shape[1])]
                if smooth:
                    triples.append((im, ops.train_gt_ensemble_batch(sl, shape, flip=flip, eps=0.00001, want="unary")[0], sel))
                else:
                    lab = ops.train_gt_ensemble_batch(sl, shape, flip=flip, eps=0.00001, want="labels", select=[sel])[0]
                    masks.append(lab.cpu().numpy().astype(np.int64))
            if triples:
                masks += [m.cpu().numpy().astype(np.int64) for m in CRF_device_many(triples, scale_factor=1.0, want="map", in_flight=2)]
    return masks


def _assert_masks_equal(got, want, ims, labels, tag):
    assert len(got) == len(want) == len(ims), tag
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], (tag, k)
        assert np.array_equal(a, b), "%s: mask %d differs on %d pixels" % (tag, k, int((a != b).sum()))
        assert set(np.unique(a)) <= set([0] + labels[k]), (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("graphed", [False, True])
def test_predict_train_gt_ms_many_equals_the_staged_composition(graphed, flip):
    from dsrg_amd import inference as I
    ims, labels = _e2e_items(141)
    net = TinyNet().cuda().eval()
    G = 4
    B = (2 if flip else 1) * G
    for smooth in (True, False):
        ref_fwd = I.GraphedForward(net) if graphed else None
        want = _staged_gt_ms(ref_fwd or net, ims, labels, G, _E2E_SIZES, flip, smooth)
        assert max(len(np.unique(m)) for m in want) >= 2
        fwd = I.GraphedForward(net) if graphed else None
        got = list(I.predict_train_gt_ms_many(net, iter(zip(ims, labels)), sizes=_E2E_SIZES, flip=flip, smooth=smooth, forward=fwd,
                                              in_flight=2, batch=2, forward_batch=G))
        _assert_masks_equal(got, want, ims, labels, "graphed %s flip %s smooth %s" % (graphed, flip, smooth))
        if graphed:                                                   # one graph per size, the padded tail group included
            assert sorted(key[0] for key in fwd._g) == [(B, 3, S, S) for S in _E2E_SIZES]
    # ignore_below reaches both routes: above 1 everything is 255
    for smooth in (True, False):
        m = list(I.predict_train_gt_ms_many(net, zip(ims[:2], labels[:2]), sizes=_E2E_SIZES, flip=flip, smooth=smooth, forward_batch=2,
                                            ignore_below=1.5))
        assert all((a == 255).all() for a in m)


@pytest.mark.gpu
def test_flip_changes_the_masks_of_a_net_that_is_not_mirror_symmetric():
    from dsrg_amd import inference as I
    ims, labels = _e2e_items(141)
    net = TinyNet().cuda().eval()
    a = list(I.predict_train_gt_ms_many(net, zip(ims, labels), sizes=_E2E_SIZES, flip=True, smooth=False, forward_batch=4))
    b = list(I.predict_train_gt_ms_many(net, zip(ims, labels), sizes=_E2E_SIZES, flip=False, smooth=False, forward_batch=4))
    assert any(not np.array_equal(x, y) for x, y in zip(a, b)), "a silently ignored flip flag"


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_one_size_without_flip_reduces_to_predict_train_gt_many(graphed):
    from dsrg_amd import inference as I
    ims, labels = _e2e_items(143)
    net = TinyNet().cuda().eval()
    for smooth in (True, False):
        for G in (1, 4):
            f1 = I.GraphedForward(net) if graphed else None
            f2 = I.GraphedForward(net) if graphed else None
            want = list(I.predict_train_gt_many(net, zip(ims, labels), smooth=smooth, size=49, forward=f1, forward_batch=G))
            got = list(I.predict_train_gt_ms_many(net, zip(ims, labels), sizes=(49,), flip=False, smooth=smooth, forward=f2,
                                                  forward_batch=G))
            _assert_masks_equal(got, want, ims, labels, "smooth %s G %d" % (smooth, G))


_AGREE_SHAPES = [(97, 131), (97, 131), (120, 90), (66, 70), (120, 90)]
_AGREE_SIZES = (73, 97, 121)


def _margin_among(q, sel):
    top2 = np.sort(q[..., sorted(set(sel))], axis=2)[:, :, -2:]
    return top2[:, :, 1] - top2[:, :, 0] if top2.shape[2] == 2 else np.full(q.shape[:2], np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_predict_train_gt_ms_many_agrees_with_predict_train_gt_ms(flip):
    """batched forwards and the fused tail against the per-image torch composition, at the bar of
    test_predict_train_gt_many_agrees_with_predict_train_gt: agreement above 0.999 per image, every differing pixel with a top-2
    margin below 1e-3 among the selected labels in predict_train_gt_ms's own CRF marginals (smooth) or probabilities
    (smooth=False).

    The image-level labels are the 1..3 foreground classes that the composition's own unrestricted arg-max uses most (as
    test_predict_train_gt_many_vs_reference_restatement picks them).  Random labels do not serve: the random-weight net saturates
    its softmax, so wherever it predicts a class outside the list the listed ones tie at marginals near 1e-15, and on the CPU the
    torch composition itself then misses this bar against a float64 restatement of it (oracle CRF; seed 147, flip: 51 of 4 620
    pixels of the 66 x 70 image differ, agreement 0.98896, 3 348 pixels with a margin below 1e-9).  With these labels that
    comparison gives agreement 1.0 on all five images."""
    from dsrg_amd import inference as I
    from dsrg_amd.crf import CRF_device
    ims, _ = _e2e_items(147, _AGREE_SHAPES)
    net = TinyNet().float().cuda().eval()
    with torch.no_grad():
        all_probs = [I._train_gt_ms_probs(net, im, _AGREE_SIZES, flip, "cuda") for im in ims]
    labels = []
    for k, p in enumerate(all_probs):
        counts = torch.bincount(p[1:].argmax(0).reshape(-1) + 1, minlength=21).cpu().numpy()
        labels.append(np.sort(np.argsort(-counts, kind="stable")[:1 + k % 3]).tolist())
    got_smooth = list(I.predict_train_gt_ms_many(net, zip(ims, labels), sizes=_AGREE_SIZES, flip=flip, forward_batch=4))
    got_plain = list(I.predict_train_gt_ms_many(net, zip(ims, labels), sizes=_AGREE_SIZES, flip=flip, smooth=False, forward_batch=4))
    for k, (im, lab) in enumerate(zip(ims, labels)):
        sel = I.train_gt_selection(lab)
        probs = all_probs[k]
        with torch.no_grad():
            q = CRF_device(torch.as_tensor(im, device="cuda"), torch.log(probs).permute(1, 2, 0).contiguous(), scale_factor=1.0)
        for smooth, got, ref in ((True, got_smooth[k], q.cpu().numpy()), (False, got_plain[k], probs.permute(1, 2, 0).cpu().numpy())):
            want = I.predict_train_gt_ms(net, im, lab, sizes=_AGREE_SIZES, flip=flip, smooth=smooth)
            margin = _margin_among(ref, sel)
            bad = got != want
            agree = 1.0 - bad.mean()
            print("flip=%s image %d smooth=%s: agreement with predict_train_gt_ms %.6f; %d differing pixels, largest top-2 margin among "
                  "them %.3g" % (flip, k, smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0))
            assert got.shape == want.shape and got.dtype == np.int64
            assert agree > 0.999
            assert not bad.any() or margin[bad].max() < 1e-3
