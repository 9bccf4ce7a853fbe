"""The final test at relative scales (training/tools/test-ms-f.py, run.sh step 4) and the evaluation front end.

CPU: inference.relative_size / preprocess_relative against scipy, the argument checks of dsrg_multiscale_unary, and
`python -m dsrg_amd.evaluate` against a restatement of training/tools/evaluate.py:132-162.
GPU: the fused multi-scale unary kernel against the torch composition, predict_mask_ms_f against a numpy/scipy restatement of
test-ms-f.py:100-142 with the oracle CRF, the bounded GraphedForward, the *_many generator and the two command-line front ends."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_relative_size_rounds_halves_away_from_zero():
    import scipy.ndimage as nd
    from dsrg_amd.inference import relative_size
    # Python 2's round (the reference's interpreter) on the exact .5 ties of real VOC sides
    assert relative_size(334, 0.75) == 251
    assert relative_size(338, 1.25) == 423
    assert relative_size(250, 1.25) == 313
    assert relative_size(366, 0.75) == 275 and relative_size(334, 1.25) == 418 and relative_size(250, 0.75) == 188
    assert [relative_size(375, f) for f in (0.75, 1, 1.25)] == [281, 375, 469]
    assert [relative_size(500, f) for f in (0.75, 1, 1.25)] == [375, 500, 625]
    # away from ties it is the shape scipy's zoom gives
    for n in (1, 2, 7, 97, 281, 333, 375, 500):
        for f in (0.75, 1.0, 1.25):
            if (n * f) % 1.0 == 0.5:
                continue
            assert relative_size(n, f) == nd.zoom(np.zeros((n, 1), np.float32), (f, 1.0), order=1).shape[0], (n, f)


@pytest.mark.parametrize("shape", [(334, 250), (97, 131), (366, 338)])
def test_preprocess_relative_is_the_reference_zoom(shape):
    """test-ms-f.py:100-112: nd.zoom(image, (s, s, 1), order=1), BGR, minus the mean.  The zoom factors are set from the expected
    shape, so the installed scipy reproduces the Python 2 shape at the .5 ties; mode='nearest' because this scipy's default
    constant mode drops a last sample whose coordinate rounds a hair past the edge"""
    import scipy.ndimage as nd
    from dsrg_amd import inference as I
    H, W = shape
    rng = np.random.default_rng(H * W)
    im = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    for f in (0.75, 1.0, 1.25):
        h, w = I.relative_size(H, f), I.relative_size(W, f)
        got = I.preprocess_relative(im, f, device="cpu")
        assert tuple(got.shape) == (1, 3, h, w) and got.dtype == torch.float32
        want = nd.zoom(im.astype('float32'), (h / float(H), w / float(W), 1.0), order=1, mode="nearest")[:, :, ::-1] - \
            np.array(I.MEAN_PIXEL)
        assert want.shape[:2] == (h, w)
        assert np.abs(got[0].numpy().transpose(1, 2, 0) - want).max() <= 1e-5 * 255


def test_multiscale_unary_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def call(K, C, H, W, ptrs=None, hs=None, ws=None, unary=fake):
        n = max(K, 1)
        P = (ctypes.c_void_p * n)(*([fake] * n)) if ptrs is None else ptrs
        Hs = (ctypes.c_int32 * n)(*([4] * n)) if hs is None else hs
        Ws = (ctypes.c_int32 * n)(*([5] * n)) if ws is None else ws
        return L.dsrg_multiscale_unary(K, C, P, Hs, Ws, H, W, 1e-5, unary, None, None, None)

    assert call(0, 21, 8, 8) == _lib.ERR_INVALID and b"scales" in L.dsrg_last_error()
    assert call(9, 21, 8, 8) == _lib.ERR_INVALID
    assert call(3, 97, 8, 8) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(3, 0, 8, 8) == _lib.ERR_INVALID
    assert call(3, 21, 0, 8) == _lib.ERR_INVALID and call(3, 21, 8, 0) == _lib.ERR_INVALID
    assert call(2, 21, 8, 8, ptrs=(ctypes.c_void_p * 2)(fake, None)) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert L.dsrg_multiscale_unary(1, 21, None, (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(4), 8, 8, 1e-5, fake, None, None,
                                   None) == _lib.ERR_INVALID
    assert call(2, 21, 8, 8, hs=(ctypes.c_int32 * 2)(4, 0)) == _lib.ERR_INVALID
    assert call(1, 21, 8, 8, unary=None) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(1, 96, 16384, 16384) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(1, 21, 8, 8, unary=ctypes.c_void_p(258)) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()


def test_multiscale_unary_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dsrg_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)
    rc = L.dsrg_multiscale_unary(1, 21, (ctypes.c_void_p * 1)(fake), (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(5), 8, 8, 1e-5,
                                 fake, None, None, None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()


def _reference_evaluate(pairs, n):
    """evaluate.py:17-68,132-162 as written: generateM's loops per image, addM, jaccard"""
    M = np.zeros((n, n))
    for gt, pred in pairs:
        m = np.zeros((n, n))
        assert len(gt) == len(pred)
        for i in range(len(gt)):
            if gt[i] < n:
                m[gt[i], pred[i]] += 1.0
        M += m
    jaccard_perclass = []
    for i in range(n):
        if not M[i, i] == 0:
            jaccard_perclass.append(M[i, i] / (np.sum(M[i, :]) + np.sum(M[:, i]) - M[i, i]))
    return np.sum(jaccard_perclass) / len(jaccard_perclass), jaccard_perclass, M


def _run_module(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


def _read_result(path):
    lines = open(path).read().split("\n", 2)
    assert lines[0].startswith("meanIOU: ")
    return float(lines[0][len("meanIOU: "):]), eval(lines[1]), lines[2]


def test_evaluate_cli_matches_the_reference_loops(tmp_path):
    from PIL import Image
    n = 6
    rng = np.random.default_rng(4)
    pred_dir, gt_dir = tmp_path / "pred", tmp_path / "gt"
    pred_dir.mkdir()
    gt_dir.mkdir()
    ids, pairs = ["img_%d" % k for k in range(4)], []
    for k, img_id in enumerate(ids):
        H, W = 17 + 3 * k, 23 - 2 * k
        gt = rng.integers(0, n, size=(H, W)).astype(np.uint8)
        gt[rng.random((H, W)) < 0.1] = 255
        gt[rng.random((H, W)) < 0.05] = 9                              # >= class_num: dropped by generateM's rule
        pred = np.where(rng.random((H, W)) < 0.6, np.minimum(gt, n - 1), rng.integers(0, n, size=(H, W))).astype(np.uint8)
        Image.fromarray(gt, mode="L").save(str(gt_dir / (img_id + ".png")))
        Image.fromarray(pred, mode="L").save(str(pred_dir / (img_id + ".png")))
        pairs.append((gt.flatten(), pred.flatten()))
    (tmp_path / "ids.txt").write_text("\n".join(ids) + "\n\n")
    save = tmp_path / "result.txt"
    _run_module(["dsrg_amd.evaluate", "--pred", str(pred_dir), "--gt", str(gt_dir), "--test_ids", str(tmp_path / "ids.txt"),
                 "--save_path", str(save), "--class_num", str(n)])
    miou, per, matrix = _read_result(str(save))
    want_miou, want_per, want_M = _reference_evaluate(pairs, n)
    assert abs(miou - want_miou) < 1e-12
    assert np.allclose(per, want_per, rtol=0, atol=1e-12) and len(per) == len(want_per)
    assert matrix.strip() == str(want_M).strip()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
class TinyNet(torch.nn.Module):
    """a deterministic stand-in for the deploy net: stride-8 feature map with 21 outputs"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.w = torch.nn.Parameter(torch.randn(21, 3, 9, 9, generator=g) * 0.02)

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.w, stride=8, padding=4)


def _image(rng, H, W, kind="smooth"):
    from dsrg_amd import synthetic as S
    im = (S.make_images(rng, 1, size=max(H, W), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
    return np.ascontiguousarray(im[:, :, ::-1]).clip(0, 255).astype(np.uint8)


# (output H x W, score map sizes taken cyclically up to K)
_CASES = [((375, 500), [(36, 47), (47, 63), (59, 79)]),               # the relative scales of a 375 x 500 VOC image
          ((37, 53), [(37, 53)]),                                     # identity
          ((40, 31), [(1, 1), (2, 3), (5, 17), (17, 5)]),
          ((1, 57), [(3, 4), (1, 1)]),
          ((43, 1), [(2, 3), (6, 1)]),
          ((1, 1), [(3, 3)]),
          ((2, 3), [(2, 3), (1, 1)])]


def _scores(rng, C, h, w, kind):
    if kind == 0:
        a = rng.standard_normal((1, C, h, w)) * 3.0
    elif kind == 1:
        a = rng.uniform(-300.0, 300.0, size=(1, C, h, w))                # softmax far into the clamp
    else:
        a = rng.integers(-2, 3, size=(1, C, h, w)) * 150.0               # +-300 with exact ties
    return torch.from_numpy(a.astype(np.float32)).cuda()


@pytest.mark.gpu
def test_multiscale_unary_kernel_matches_the_torch_composition():
    from dsrg_amd import inference as I, ops
    rng = np.random.default_rng(11)
    n_sum = n_sum_exact = n_pix = n_arg_same = 0
    worst_unary = 0.0
    case = 0
    for K in (1, 2, 3, 8):
        for C in (1, 2, 21, 81, 96):
            for (H, W), sizes in _CASES:
                case += 1
                kind = case % 3
                scores = [_scores(rng, C, *sizes[k % len(sizes)], kind) for k in range(K)]
                unary, amax, S = ops.multiscale_unary(scores, H, W, eps=1e-5, want=("unary", "argmax", "sum"))
                u2, a2, S2 = ops.multiscale_unary(scores, H, W, eps=1e-5, want=("unary", "argmax", "sum"))
                assert torch.equal(unary, u2) and torch.equal(amax, a2) and torch.equal(S, S2), "not reproducible"
                assert torch.equal(ops.multiscale_unary(scores, H, W, want="argmax"), amax)
                # the torch composition of predict_mask_ms (multiscale_scores -> _probs_from_scores -> log -> permute)
                zs = [I._zoom(s, H, W) for s in scores]
                total = zs[0]
                for z in zs[1:]:
                    total = total + z
                probs = I._probs_from_scores(total[0])
                want_unary = torch.log(probs).permute(1, 2, 0).cpu().numpy()
                want_S = total[0].permute(1, 2, 0).cpu().numpy()
                zmax = torch.stack([z[0].abs() for z in zs]).amax(0).permute(1, 2, 0).cpu().numpy()
                got_S, got_u, got_a = S.cpu().numpy(), unary.cpu().numpy(), amax.cpu().numpy()
                assert got_S.shape == (H, W, C) and got_u.shape == (H, W, C) and got_a.shape == (H, W)
                assert amax.dtype == torch.int32
                # the sum: one rounding per z_k at most (torch's fp64 kernel may contract to FMA, this one does not).  An ulp of the
                # largest |z_k| — or, where the blend cancels, of the largest score it blends: a contracted product changes the
                # double result by an ulp of its operands, which is many ulps of a result near zero
                d = np.abs(got_S.astype(np.float64) - want_S)
                smax = np.float32(max(float(s.abs().max()) for s in scores))
                tol = K * np.spacing(np.maximum(zmax, 1e-7 * smax).astype(np.float32)).astype(np.float64)
                assert (d <= tol).all(), (K, C, H, W, float(d.max()))
                n_sum += d.size
                n_sum_exact += int((d == 0).sum())
                du = float(np.abs(got_u - want_unary).max())
                worst_unary = max(worst_unary, du)
                assert du <= 8e-6, (K, C, H, W, du)
                # arg-max: the first maximum of the kernel's own sum
                assert np.array_equal(got_a, np.argmax(got_S, axis=2)), (K, C, H, W)
                ta = probs.argmax(0).cpu().numpy()
                diff = got_a != ta
                if diff.any():
                    ys, xs = np.nonzero(diff)
                    a_, b_ = want_S[ys, xs, got_a[diff]], want_S[ys, xs, ta[diff]]
                    assert (np.abs(a_ - b_) <= np.spacing(np.maximum(np.abs(a_), np.abs(b_)))).all(), (K, C, H, W)
                n_pix += got_a.size
                n_arg_same += int((~diff).sum())
    print("sum bit-exact on %.6f of %d values; arg-max as torch's on %.6f of %d pixels; largest |unary - torch| %.3g"
          % (n_sum_exact / n_sum, n_sum, n_arg_same / n_pix, n_pix, worst_unary))
    assert n_sum_exact >= 0.999 * n_sum
    assert n_arg_same >= 0.9999 * n_pix


@pytest.mark.gpu
def test_predict_mask_ms_f_vs_reference_restatement():
    """test-ms-f.py:100-142 in numpy/scipy (network: the same TinyNet on the CPU in float64, CRF: the oracle) on a 334 x 250 image,
    where Python 2's rounding makes the network inputs 251 rows at 0.75 and 313 columns at 1.25"""
    import scipy.ndimage as nd
    from dsrg_amd import inference as I
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    H, W = 334, 250
    im = _image(rng, H, W)
    net = TinyNet().cuda().eval()
    netc = TinyNet().double().eval()
    d1, d2 = float(H), float(W)
    shapes = [(251, 188), (334, 250), (418, 313)]                      # 0.75 / 1 / 1.25 as scipy 0.18 under Python 2 sized them
    assert [(I.relative_size(H, f), I.relative_size(W, f)) for f in (0.75, 1.0, 1.25)] == shapes
    scores_all = 0
    for (h, w) in shapes:
        # (zoom factors from the expected shapes; mode='nearest': see test_preprocess_relative_is_the_reference_zoom)
        x = nd.zoom(im.astype('float32'), (h / d1, w / d2, 1.0), order=1, mode="nearest")[:, :, [2, 1, 0]] - np.array(I.MEAN_PIXEL)
        with torch.no_grad():
            sc = netc(torch.tensor(x.transpose(2, 0, 1)[None], dtype=torch.float64))[0].numpy().transpose(1, 2, 0)
        scores_all = scores_all + nd.zoom(sc, (d1 / sc.shape[0], d2 / sc.shape[1], 1.0), order=1, mode="nearest")
    e = np.exp(scores_all - np.max(scores_all, axis=2, keepdims=True))
    probs = e / np.sum(e, axis=2, keepdims=True)
    probs[probs < 0.00001] = 0.00001
    q = O.CRF(im, np.log(probs), scale_factor=1.0)
    for smooth, ref in ((True, q), (False, probs)):
        got = I.predict_mask_ms_f(net, im, smooth=smooth)
        want = np.argmax(ref, axis=2)
        top2 = np.sort(ref, axis=2)[:, :, -2:]
        margin = top2[:, :, 1] - top2[:, :, 0]
        bad = got != want
        agree = 1.0 - bad.mean()
        print("smooth=%s: agreement with the test-ms-f.py restatement %.5f; %d differing pixels, largest reference top-2 margin "
              "among them %.3g" % (smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0))
        assert got.shape == (H, W) and got.dtype == np.int64
        assert agree > 0.999
        assert not bad.any() or margin[bad].max() < 1e-3


def _vgg(num_classes=21, seed=0, spread=False):
    """VGG16-ASPP in eval mode; spread: He-initialised convolutions with zero biases, so that the scores of a random net vary over
    the image and the masks hold several labels"""
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(seed)
    net = VGG16ASPP(num_classes=num_classes)
    if spread:
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                if m.bias is not None:
                    torch.nn.init.zeros_(m.bias)
    return net.cuda().to(memory_format=torch.channels_last).eval()


@pytest.mark.gpu
def test_predict_mask_ms_f_fused_equals_unfused_on_vgg16_aspp():
    """the fused unary against the torch composition on VGG16-ASPP under bf16 autocast at 375 x 500 (network inputs 281 x 375,
    375 x 500, 469 x 625)"""
    from dsrg_amd import inference as I
    net = _vgg(spread=True)
    im = _image(np.random.default_rng(7), 375, 500, kind="noise")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for smooth in (True, False):
            a = I.predict_mask_ms_f(net, im, smooth=smooth, fused=True)
            b = I.predict_mask_ms_f(net, im, smooth=smooth, fused=False)
            agree = (a == b).mean()
            print("smooth=%s: fused / unfused masks agree on %.6f of the pixels (%d labels used)" % (smooth, agree, len(np.unique(a))))
            assert a.shape == (375, 500) and agree >= 0.9999
            if not smooth:
                assert len(np.unique(b)) >= 2


@pytest.mark.gpu
def test_bounded_graphed_forward():
    """max_shapes bounds the captured graphs (least recently used dropped), capture_after runs a shape eagerly before capturing it,
    every call equals the eager forward bit for bit; the defaults keep one graph per shape"""
    from dsrg_amd import inference as I
    net = _vgg(seed=1)
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    shapes = [(65, 81), (81, 65), (97, 97), (65, 81), (97, 97), (81, 65), (65, 81), (65, 81)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        bounded = I.GraphedForward(net, max_shapes=2)
        late = I.GraphedForward(net, max_shapes=2, capture_after=2)
        plain = I.GraphedForward(net)
        seen = {}
        for k, (h, w) in enumerate(shapes):
            x = torch.randn(1, 3, h, w, device=dev, generator=g) * 40.0
            want = net(x).float().clone()
            for fwd in (bounded, late, plain):
                got = fwd(x).float()
                assert torch.equal(got, want), (k, h, w)
            seen[(h, w)] = seen.get((h, w), 0) + 1
            assert len(bounded._g) <= 2 and len(late._g) <= 2
            assert (bounded._g and list(bounded._g)[-1][0] == (1, 3, h, w))          # most recently used last
            assert ((1, 3, h, w) in [key[0] for key in late._g]) == (seen[(h, w)] >= 2)
        assert len(bounded._g) == 2
        assert len(plain._g) == 3


@pytest.mark.gpu
def test_predict_masks_ms_f_many_equals_the_one_image_calls():
    from dsrg_amd import inference as I
    rng = np.random.default_rng(9)
    shapes = [(97, 131), (97, 131), (120, 90), (66, 70), (97, 131), (120, 90), (120, 90), (66, 70), (97, 131)]
    ims = [_image(rng, H, W, kind=["smooth", "noise", "dark_corner"][k % 3]) for k, (H, W) in enumerate(shapes)]
    net = TinyNet().cuda().eval()
    want = [I.predict_mask_ms_f(net, im) for im in ims]
    bounded = I.GraphedForward(net, max_shapes=2, capture_after=2)
    for kw in (dict(in_flight=3), dict(in_flight=2, batch=2), dict(in_flight=2, forward=bounded),
               dict(in_flight=3, batch=2, forward=bounded)):
        got = list(I.predict_masks_ms_f_many(net, ims, **kw))
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dtype == np.int64 and np.array_equal(a, b), kw
    assert 0 < len(bounded._g) <= 2


@pytest.mark.gpu
def test_predict_and_evaluate_cli_end_to_end(tmp_path):
    """python -m dsrg_amd.predict --mode ms-f on two JPEGs with weights written by checkpoint.save_weights: the PNGs equal
    predict_mask_ms_f on the same decoded pixels; python -m dsrg_amd.evaluate of them against themselves gives mIoU 1"""
    from PIL import Image
    from dsrg_amd import checkpoint, inference as I
    from dsrg_amd.predict import read_image
    net = _vgg(seed=4, spread=True)
    model = str(tmp_path / "net.caffemodel")
    checkpoint.save_weights(net, model)
    voc = tmp_path / "VOC"
    (voc / "JPEGImages").mkdir(parents=True)
    rng = np.random.default_rng(12)
    ids = ["2007_000001", "2007_000002"]
    for img_id, (H, W) in zip(ids, [(97, 129), (120, 90)]):
        Image.fromarray(_image(rng, H, W, kind="noise"), mode="RGB").save(str(voc / "JPEGImages" / (img_id + ".jpg")), quality=95)
    (tmp_path / "val.txt").write_text("\n".join(ids) + "\n")
    out = tmp_path / "out"
    _run_module(["dsrg_amd.predict", "--mode", "ms-f", "--model", model, "--images", str(tmp_path / "val.txt"), "--dir", str(voc),
                 "--output", str(out), "--smooth"], timeout=900)
    net2 = _vgg(seed=99)
    checkpoint.load_weights(net2, model)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for img_id in ids:
            im = read_image(str(voc / "JPEGImages" / (img_id + ".jpg")))
            want = I.predict_mask_ms_f(net2, im, smooth=True)
            png = np.array(Image.open(str(out / (img_id + ".png"))))
            assert png.dtype == np.uint8 and png.shape == want.shape
            assert np.array_equal(png.astype(np.int64), want), img_id
    save = tmp_path / "result.txt"
    _run_module(["dsrg_amd.evaluate", "--pred", str(out), "--gt", str(out), "--test_ids", str(tmp_path / "val.txt"),
                 "--save_path", str(save), "--class_num", "21"])
    miou, per, _ = _read_result(str(save))
    assert miou == 1.0 and all(v == 1.0 for v in per)
