"""Label-restricted pseudo-label generation (training/tools/generate_train_gt.py:78-106), batched and on the GPU.

CPU: the argument checks of dsrg_train_gt_unary_batch / dsrg_crf_map_select, the selection helper and `--mode gt` of
`python -m dsrg_amd.predict`.
GPU: the softmax-then-zoom unary kernel (a group against single-image calls bit for bit; the wrapper and the C entry point against
the outputs recorded before the one-map form became the ensemble's K = 1 case, bit for bit; the probabilities against a float64
restatement with scipy's zoom; the log against the kernel's own probabilities), the selection rule of the unary kernel and of the
two CRF kernels against numpy on the returned probabilities / marginals (exact), predict_train_gt_many against its staged
composition (exact), against predict_train_gt and against the reference restated in numpy / scipy (the project's agreement bar)."""
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
def test_train_gt_unary_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(_FAKE)

    def call(G=3, C=21, scores=one, h=4, w=5, Hs="fake", Ws="fake", sel=None, nsel=None, stride=0, ws=one, unary="fake",
             probs=None, labels=None):
        g = max(G, 1)
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        u = _vp([_FAKE] * g) if unary == "fake" else unary
        return L.dsrg_train_gt_unary_batch(G, C, scores, h, w, H, W, 1e-5, sel, nsel, stride, 0.0, ws, u, probs, labels, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=17) == _lib.ERR_INVALID and b"16" in L.dsrg_last_error()
    assert call(C=0) == _lib.ERR_INVALID and b"labels" in L.dsrg_last_error()
    assert call(C=97) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(scores=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(ws=None) == _lib.ERR_INVALID and b"workspace" in L.dsrg_last_error()
    assert call(Hs=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Ws=None) == _lib.ERR_INVALID
    assert call(h=0) == _lib.ERR_INVALID and b"score map" in L.dsrg_last_error()
    assert call(w=0) == _lib.ERR_INVALID
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(Ws=_i32([9, 9, 0])) == _lib.ERR_INVALID
    assert call(unary=None) == _lib.ERR_INVALID and b"no output" in L.dsrg_last_error()
    assert call(unary=_vp([None] * 3)) == _lib.ERR_INVALID and b"no output" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(probs=_vp([None, _FAKE, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(labels=_vp([_FAKE, _FAKE, None])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, _FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(unary=None, probs=_vp([_FAKE, 264, _FAKE])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, C=96, Hs=_i32([16384]), Ws=_i32([16384])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(G=1, C=96, h=8192, w=8192) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    # labels need the lists; a list holds 1..128 entries of [0, C) and fits the stride
    lab = _vp([_FAKE] * 3)
    good, n3 = _i32([0, 3, 7] * 3), _i32([3, 3, 3])
    assert call(labels=lab) == _lib.ERR_INVALID and b"selection" in L.dsrg_last_error()
    assert call(labels=lab, sel=good, nsel=None, stride=3) == _lib.ERR_INVALID
    assert call(labels=lab, sel=good, nsel=_i32([3, 0, 3]), stride=3) == _lib.ERR_INVALID and b"1..128" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0] * 3 * 129), nsel=_i32([3, 129, 3]), stride=129) == _lib.ERR_INVALID
    assert b"1..128" in L.dsrg_last_error() and b"image 1" in L.dsrg_last_error()
    assert call(labels=lab, sel=good, nsel=n3, stride=2) == _lib.ERR_INVALID and b"select_stride" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0, 3, 7, 0, 21, 7, 0, 3, 7]), nsel=n3, stride=3) == _lib.ERR_INVALID
    assert b"outside [0, 21)" in L.dsrg_last_error() and b"image 1" in L.dsrg_last_error()
    assert call(labels=lab, sel=_i32([0, 3, 7, 0, 3, 7, 0, 3, -1]), nsel=n3, stride=3) == _lib.ERR_INVALID
    assert b"outside" in L.dsrg_last_error()
    # the lists are not looked at (may be NULL) when no labels are asked for
    if not torch.cuda.is_available():
        assert call() == _lib.ERR_HIP


def test_crf_map_select_checks_arguments_before_any_device_call():
    """without a GPU there is no object to pass: what does not depend on the object is checked first (pointers, the first list:
    every object has one image at least and 96 labels at most), then the handle"""
    from dsrg_amd import _lib
    L = _lib.lib()
    out = (_I32 * 4)()
    sel, n = _i32([0, 3, 7]), _i32([3])
    assert L.dsrg_crf_map_select(None, 10, None, n, 3, 0.0, out) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, sel, None, 3, 0.0, out) == _lib.ERR_INVALID
    assert L.dsrg_crf_map_select(None, 10, sel, n, 3, 0.0, None) == _lib.ERR_INVALID
    assert L.dsrg_crf_map_select(None, 10, sel, _i32([0]), 3, 0.0, out) == _lib.ERR_INVALID and b"1..128" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, _i32([0] * 129), _i32([129]), 129, 0.0, out) == _lib.ERR_INVALID
    assert b"1..128" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, sel, n, 2, 0.0, out) == _lib.ERR_INVALID and b"select_stride" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, _i32([0, 96, 7]), n, 3, 0.0, out) == _lib.ERR_INVALID
    assert b"outside [0, 96)" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, _i32([0, -1, 7]), n, 3, 0.0, out) == _lib.ERR_INVALID and b"outside" in L.dsrg_last_error()
    assert L.dsrg_crf_map_select(None, 10, sel, n, 3, 0.0, out) == _lib.ERR_INVALID and b"handle" in L.dsrg_last_error()


def test_train_gt_entry_points_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dsrg_amd import _lib
    from dsrg_amd.crf import DenseCRF
    L = _lib.lib()
    rc = L.dsrg_train_gt_unary_batch(2, 21, ctypes.c_void_p(_FAKE), 4, 5, _i32([8, 3]), _i32([8, 7]), 1e-5, _i32([0, 3, 0, 7]),
                                     _i32([2, 2]), 2, 0.0, ctypes.c_void_p(_FAKE), _vp([_FAKE, 512]), None, _vp([_FAKE, 512]), None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()
    with pytest.raises(_lib.DsrgError) as e:                          # the object dsrg_crf_map_select needs cannot be made
        DenseCRF(8, 8, 21)
    assert e.value.code == _lib.ERR_HIP


def test_train_gt_selection_keeps_order_and_duplicates():
    from dsrg_amd import inference as I
    from dsrg_amd.crf import select_arrays
    assert I.train_gt_selection([3, 7]) == [0, 3, 7]
    assert I.train_gt_selection(np.array([7, 3, 7])) == [0, 7, 3, 7]
    assert I.train_gt_selection([]) == [0]
    assert I.train_gt_selection([0]) == [0, 0]
    assert all(type(c) is int for c in I.train_gt_selection(np.array([15, 2], dtype=np.int64)))
    flat, counts, stride = select_arrays([[0, 5, 2], [0]], 2, 21)
    assert list(flat) == [0, 5, 2, 0, 0, 0] and list(counts) == [3, 1] and stride == 3
    for bad in ([[0, 21]], [[]], [[0] * 129], [[0], [1]]):
        with pytest.raises(ValueError):
            select_arrays(bad, 1, 21)


def test_predict_cli_gt_mode(capsys, tmp_path):
    from dsrg_amd import predict
    common = ["--model", "m", "--images", "i", "--dir", "d", "--output", "o"]
    with pytest.raises(SystemExit) as e:
        predict.parse_args(["--mode", "gt"] + common)
    assert e.value.code == 2
    assert "--cues" in capsys.readouterr().err
    a = predict.parse_args(["--mode", "gt", "--cues", "c.pickle"] + common)
    assert a.mode == "gt" and a.cues == "c.pickle" and a.forward_batch == 1 and a.scales is None and not a.smooth
    a = predict.parse_args(["--mode", "gt", "--cues", "c.pickle", "--forward-batch", "8", "--smooth", "--in-flight", "2",
                            "--scales", "241"] + common)
    assert a.forward_batch == 8 and a.smooth and a.in_flight == 2 and a.scales == "241"
    with pytest.raises(SystemExit):
        predict.parse_args(["--mode", "gt", "--cues", "c.pickle", "--scales", "241,321"] + common)
    with pytest.raises(SystemExit):
        predict.parse_args(["--mode", "gt", "--cues", "c.pickle", "--forward-batch", "17"] + common)
    with pytest.raises(SystemExit):
        predict.parse_args(["--mode", "ms", "--cues", "c.pickle"] + common)
    lst = tmp_path / "input_list.txt"
    lst.write_text("2007_000032.jpg 0\n\n2008_000008.jpg 17\n")
    assert predict.read_gt_list(str(lst)) == [("2007_000032", 0), ("2008_000008", 17)]


# ---- GPU: the unary kernel ----------------------------------------------------------------------------------------------------
from test_ms_batched import TinyNet, _E2E_SHAPES, _batched_scores, _e2e_images, _image    # noqa: E402  (shared fixtures)

_OUT = [(37, 53), (40, 31), (1, 1), (97, 131), (1, 57), (43, 1), (2, 3)]
_MAPS = [(1, 1), (2, 3), (5, 17), (17, 5), (12, 16), (13, 9)]
_CS = (1, 2, 21, 96)
_EPS = 1e-5


def _lists(rng, G, C):
    """one list per image: 1..4 labels of [0, C), any order, duplicates allowed"""
    return [[int(c) for c in rng.integers(0, C, size=int(rng.integers(1, 5)))] for _ in range(G)]


def _select_host(v, sel, t=0.0):
    """the rule on the host: sel[first arg-max of v[..., sel]], 255 where the maximum over all labels is below t > 0"""
    sel = np.asarray(sel)
    out = sel[np.argmax(v[..., sel], axis=-1)]
    if t > 0:
        out = np.where(v.max(-1) < np.float32(t), 255, out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 16])
def test_train_gt_unary_batch_equals_single_image_calls(G):
    from dsrg_amd import ops
    rng = np.random.default_rng(60 + G)
    names = ("probs", "unary", "labels")
    case = 0
    for C in _CS:
        for kind in range(3):
            case += 1
            h, w = _MAPS[(case + G) % len(_MAPS)]
            Gcap = G + 1 + case % 2
            shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
            scores = _batched_scores(rng, Gcap, C, h, w, kind)
            select = _lists(rng, G, C)
            t = (None, 0.85)[case % 2]
            got = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want=names, select=select, ignore_below=t)
            again = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want=names, select=select, ignore_below=t)
            assert len(got) == G
            for g, (H, W) in enumerate(shapes):
                want = ops.train_gt_unary_batch(scores[g:g + 1].contiguous(), [(H, W)], eps=_EPS, want=names, select=[select[g]],
                                                ignore_below=t)[0]
                for n, a, b, c in zip(names, got[g], want, again[g]):
                    assert a.shape == b.shape == ((H, W) if n == "labels" else (H, W, C)) and a.dtype == b.dtype, (n, G, C, g)
                    assert torch.equal(a, b), "%s of image %d differs from the G = 1 call (G %d C %d kind %d)" % (n, g, G, C, kind)
                    assert torch.equal(a, c), "%s of image %d is not reproducible (G %d C %d kind %d)" % (n, g, G, C, kind)
            only = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want="unary")          # string form, no lists needed
            assert isinstance(only, list) and all(torch.equal(o, t3[1]) for o, t3 in zip(only, got))
            default = ops.train_gt_unary_batch(scores, shapes, eps=_EPS)                     # want=("unary",): 1-tuples
            assert all(len(o) == 1 and torch.equal(o[0], t3[1]) for o, t3 in zip(default, got))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 16])
def test_train_gt_unary_batch_gives_the_recorded_outputs(G):
    """train_gt_unary_batch alone against the outputs its own kernels gave before it became the ensemble's K = 1 case
    (train_gt_golden_cases; the cases are the loop of test_train_gt_ms.py's
    test_one_size_without_flip_is_train_gt_unary_batch_bit_for_bit, with that file's shapes and lists)"""
    import test_train_gt_ms as MS
    import train_gt_golden_cases as golden
    from dsrg_amd import _lib, ops
    from dsrg_amd.crf import select_arrays
    rng = np.random.default_rng(100 + G)
    case = 0
    for C in MS._CS:
        for h, w in MS._MAPS:
            case += 1
            scores = _batched_scores(rng, G + case % 2, C, h, w, case % 3)
            shapes = [MS._OUT[(case + g) % len(MS._OUT)] for g in range(G)]
            select = MS._lists(rng, G, C)
            t = (None, 0.5)[case % 2]
            got = ops.train_gt_unary_batch(scores, shapes, eps=MS._EPS, want=golden.NAMES, select=select, ignore_below=t)
            golden.assert_recorded("train_gt_unary_batch", G, case, scores, got)
            # the C entry point of the one-map form, which the wrapper no longer goes through: G * C * h * w floats of workspace
            out = ops._want_outputs(golden.NAMES, shapes, C, scores.device)
            work = torch.empty(G * C * h * w, device="cuda")
            sel, nsel, stride = select_arrays(select, G, C)
            ops.check(_lib.lib().dsrg_train_gt_unary_batch(
                G, C, ops._ptr(scores), h, w, _i32([H for H, _ in shapes]), _i32([W for _, W in shapes]), MS._EPS, sel, nsel, stride,
                t or 0.0, ops._ptr(work), ops._ptrs(out["unary"]), ops._ptrs(out["probs"]), ops._ptrs(out["labels"]), ops._stream()))
            golden.assert_recorded("dsrg_train_gt_unary_batch", G, case, scores, list(zip(*(out[n] for n in golden.NAMES))))


@pytest.mark.gpu
def test_train_gt_unary_batch_validates_its_arguments():
    from dsrg_amd import ops
    s = torch.zeros(3, 21, 4, 5, device="cuda")
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)], want="sum")
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)], want=())
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch([s], [(8, 8)])
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)] * 4)                      # more images than slices
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s.double(), [(8, 8)])
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)], want="labels")           # no lists
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)], want="labels", select=[[0, 21]])
    with pytest.raises(ValueError):
        ops.train_gt_unary_batch(s, [(8, 8)], want="labels", select=[[0], [1]])


def _restated_probs(s, H, W):
    """generate_train_gt.py:85-93 for one (C, h, w) float32 score map: d = s - max in float32 as numpy computes it on the blob,
    then exp, normalisation and scipy's order-1 zoom in float64, clamp at eps -> (H, W, C) float64"""
    import scipy.ndimage as nd
    sc = np.transpose(s, (1, 2, 0))
    d = (sc - np.max(sc, axis=2, keepdims=True)).astype(np.float32)
    assert d.dtype == np.float32
    e = np.exp(d.astype(np.float64))
    p = e / np.sum(e, axis=2, keepdims=True)
    p = nd.zoom(p, (float(H) / p.shape[0], float(W) / p.shape[1], 1.0), order=1)
    assert p.shape == (H, W, s.shape[0])
    p[p < _EPS] = _EPS
    return p


@pytest.mark.gpu
def test_train_gt_probs_against_float64_restatement_and_unary_against_probs():
    """|probs - restatement| <= (C + 8) * 2^-24: at most 2 ulps for expf, (C - 1) / 2 ulps for the ordered float32 sum, half an ulp
    each for the division and the final rounding, all on values <= 1 (ulp <= 2^-24); the zoom is a convex combination and adds
    nothing.  unary: within 2 float32 ulps of the float64 logarithm of the kernel's own probability."""
    from dsrg_amd import ops
    rng = np.random.default_rng(71)
    worst = worst_log = 0.0
    case = 0
    for C in _CS:
        bound = (C + 8) * 2.0 ** -24
        for kind in range(3):
            for h, w in _MAPS:
                case += 1
                G = 3
                shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
                if case % 6 == 0:
                    shapes[0] = (97, 131)
                scores = _batched_scores(rng, G + 1, C, h, w, kind)
                got = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want=("probs", "unary"))
                s_host = scores.cpu().numpy()
                for g, (H, W) in enumerate(shapes):
                    probs = got[g][0].cpu().numpy()
                    unary = got[g][1].cpu().numpy()
                    assert probs.dtype == np.float32 and probs.shape == (H, W, C)
                    ref = _restated_probs(s_host[g], H, W)
                    err = float(np.abs(probs.astype(np.float64) - ref).max())
                    worst = max(worst, err / bound)
                    assert err <= bound, "probs: C %d kind %d map %s out %s: %.3g > %.3g" % (C, kind, (h, w), (H, W), err, bound)
                    assert probs.min() >= np.float32(_EPS)
                    lg = np.log(probs.astype(np.float64))
                    ulp = np.spacing(np.abs(lg).astype(np.float32)).astype(np.float64)
                    r = np.abs(unary.astype(np.float64) - lg) / ulp
                    worst_log = max(worst_log, float(r.max()))
                    assert r.max() <= 2.0, "unary: C %d kind %d map %s out %s: %.3g ulps" % (C, kind, (h, w), (H, W), r.max())
    print("train_gt_unary_batch: worst |probs - restatement| / bound = %.3f; worst |unary - log(probs)| = %.3f ulps"
          % (worst, worst_log))


@pytest.mark.gpu
def test_train_gt_labels_follow_the_selection_rule_exactly():
    from dsrg_amd import ops
    rng = np.random.default_rng(73)
    case = 0
    for C in _CS:
        for kind in range(3):
            case += 1
            h, w = _MAPS[case % len(_MAPS)]
            G = 3
            shapes = [_OUT[(case + g) % len(_OUT)] for g in range(G)]
            scores = _batched_scores(rng, G + 1, C, h, w, kind)
            if C > 5:
                scores[:, 5] = scores[:, 2]                          # label 5 is a bit-copy of label 2: exact ties
            lists = _lists(rng, G, C)
            if C > 5:
                lists[0], lists[1] = [0, 5, 2], [0, 2, 5]
            lists[2] = lists[2] + [lists[2][0]]                      # a duplicate
            for t in (0.0, 0.85, 1.5):
                got = ops.train_gt_unary_batch(scores, shapes, eps=_EPS, want=("probs", "labels"), select=lists, ignore_below=t)
                for g in range(G):
                    p, lab = got[g][0].cpu().numpy(), got[g][1].cpu().numpy()
                    assert lab.dtype == np.int32
                    assert np.array_equal(lab, _select_host(p, lists[g], t)), (C, kind, g, t)
                    if t > 1:
                        assert (lab == 255).all()
                    if t == 0:
                        assert set(np.unique(lab)) <= set(lists[g])
            if C > 5:
                # the tie goes to whichever of the two comes first in the list
                shapes2 = [(37, 53), (37, 53)]
                a = ops.train_gt_unary_batch(scores, shapes2, want=("probs", "labels"), select=[[0, 5, 2], [0, 2, 5]])
                for g, first in ((0, 5), (1, 2)):
                    p, lab = a[g][0].cpu().numpy(), a[g][1].cpu().numpy()
                    tie = p[..., 2] > p[..., 0]
                    assert np.array_equal(p[..., 2], p[..., 5])
                    if kind == 0:
                        assert tie.any()
                    assert (lab[tie] == first).all() and (lab[~tie] == 0).all()


# ---- GPU: the restricted MAP of the CRF objects ----------------------------------------------------------------------------------
def _crf_case(rng, H, W, C=21):
    """an image and log-probability unaries in which label 5 is a bit-copy of label 2 and the two lead in the left half"""
    im = torch.from_numpy(_image(rng, H, W, kind="smooth")).cuda()
    s = rng.standard_normal((H, W, C)).astype(np.float32)
    s[:, :W // 2 + 1, 2] += 3.0
    s[:, W // 2:, 7] += 2.0
    s[:, :, 5] = s[:, :, 2]
    u = torch.log_softmax(torch.from_numpy(s), dim=2).contiguous()
    u[:, :, 5] = u[:, :, 2]
    return im, u.cuda()


_SELECT_LISTS = ([0, 5, 2], [0, 2, 5], [0, 7, 7, 3], [7], [20, 0, 2, 7, 5, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(37, 53), (97, 131)])      # the LDS-resident path / the global-memory path
def test_crf_map_select_one_image_object(H, W):
    from dsrg_amd import ops
    from dsrg_amd.crf import CRF_device
    assert ops.lds_path_supports(H, W) == ((H, W) == (37, 53))
    rng = np.random.default_rng(80 + H)
    im, u = _crf_case(rng, H, W)
    q = CRF_device(im, u, scale_factor=1.0).cpu().numpy()                      # computed once, shared
    assert np.array_equal(q[..., 5], q[..., 2]), "a bit-copied label must get bit-equal marginals"
    plain = CRF_device(im, u, scale_factor=1.0, want="map").cpu().numpy()
    assert np.array_equal(plain, np.argmax(q, axis=2))                         # no select: what map returns today
    tie = (q[..., 2] > q[..., 0])
    assert tie.any() and (~tie).any()
    for sel in _SELECT_LISTS:
        for t in (0.0, 0.85, 1.5):
            got = CRF_device(im, u, scale_factor=1.0, want="map", select=sel, ignore_below=t).cpu().numpy()
            assert got.dtype == np.int32 and got.shape == (H, W)
            assert np.array_equal(got, _select_host(q, sel, t)), (sel, t)
            if t > 1:
                assert (got == 255).all()
    a = CRF_device(im, u, scale_factor=1.0, want="map", select=[0, 5, 2]).cpu().numpy()
    b = CRF_device(im, u, scale_factor=1.0, want="map", select=[0, 2, 5]).cpu().numpy()
    assert (a[tie] == 5).all() and (b[tie] == 2).all() and np.array_equal(a[~tie], b[~tie])
    t85 = CRF_device(im, u, scale_factor=1.0, want="map", select=[0, 5, 2], ignore_below=0.85).cpu().numpy()
    assert (t85 == 255).any(), "with two tied leaders no marginal reaches 0.85 in the left half"
    # the plain map after a restricted one on a recycled object is the plain map again
    assert np.array_equal(CRF_device(im, u, scale_factor=1.0, want="map").cpu().numpy(), plain)
    with pytest.raises(ValueError):
        CRF_device(im, u, scale_factor=1.0, want="map", select=[0, 21])
    with pytest.raises(ValueError):
        CRF_device(im, u, scale_factor=1.0, select=[0, 2])                     # marginals take no list


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (3, 40, 31)])
def test_crf_map_select_batched_object(B, H, W):
    from dsrg_amd.crf import CRF_device_batch, CRF_device_many
    rng = np.random.default_rng(90 + B)
    cases = [_crf_case(rng, H, W) for _ in range(B)]
    ims, us = torch.stack([c[0] for c in cases]), torch.stack([c[1] for c in cases])
    q = CRF_device_batch(ims, us, scale_factor=1.0).cpu().numpy()
    plain = CRF_device_batch(ims, us, scale_factor=1.0, want="map").cpu().numpy()
    assert np.array_equal(plain, np.argmax(q, axis=3))
    lists = [list(_SELECT_LISTS[(b + B) % len(_SELECT_LISTS)]) for b in range(B)]
    assert len(set(map(tuple, lists))) == B                                    # a different list per image
    for t in (0.0, 0.85, 1.5):
        got = CRF_device_batch(ims, us, scale_factor=1.0, want="map", select=lists, ignore_below=t).cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], _select_host(q[b], lists[b], t)), (b, t)
    a = CRF_device_batch(ims, us, scale_factor=1.0, want="map", select=[[0, 5, 2]] * B).cpu().numpy()
    c = CRF_device_batch(ims, us, scale_factor=1.0, want="map", select=[[0, 2, 5]] * B).cpu().numpy()
    tie = q[..., 2] > q[..., 0]
    assert tie.any() and (a[tie] == 5).all() and (c[tie] == 2).all()
    # the many-image form: triples share a batched call, each with its own list; pairs stay what they were
    many = [m.cpu().numpy() for m in CRF_device_many([(i, u, s) for (i, u), s in zip(cases, lists)], scale_factor=1.0, in_flight=2,
                                                     batch=B)]
    one = [m.cpu().numpy() for m in CRF_device_many([(i, u, s) for (i, u), s in zip(cases, lists)], scale_factor=1.0, in_flight=2)]
    pairs = [m.cpu().numpy() for m in CRF_device_many(cases, scale_factor=1.0, in_flight=2, batch=B)]
    for b in range(B):
        want = _select_host(q[b], lists[b])
        assert np.array_equal(many[b], want) and np.array_equal(one[b], want) and np.array_equal(pairs[b], plain[b])
    with pytest.raises(ValueError):
        CRF_device_batch(ims, us, scale_factor=1.0, want="map", select=lists[:1])


# ---- GPU: end to end ---------------------------------------------------------------------------------------------------------------
_SIZE = 97


def _e2e_items(seed):
    rng = np.random.default_rng(seed)
    ims = _e2e_images(seed)
    return ims, [[int(c) for c in rng.choice(np.arange(1, 21), size=1 + k % 3, replace=False)] for k in range(len(ims))]


def _staged_gt(fwd, ims, labels, G, size, smooth):
    """predict_train_gt_many composed from its stages: ops.preprocess_ms_batch, the same batch-G forward (tail group padded), then
    per image ops.train_gt_unary_batch at G = 1 on the slice and CRF_device(want="map", select=...) or the kernel's own labels"""
    from dsrg_amd import inference as I, ops
    from dsrg_amd.crf import CRF_device
    masks = []
    with torch.no_grad():
        for start in range(0, len(ims), G):
            dev = [torch.from_numpy(im).cuda() for im in ims[start:start + G]]
            scores = fwd(ops.preprocess_ms_batch(dev, [size], capacity=G)[0]).float().contiguous()
            for g, im in enumerate(dev):
                sel = I.train_gt_selection(labels[start + g])
                shape = [(im.shape[0], im.shape[1])]
                sl = scores[g:g + 1].contiguous()
                if smooth:
                    unary = ops.train_gt_unary_batch(sl, shape, eps=0.00001, want="unary")[0]
                    m = CRF_device(im, unary, scale_factor=1.0, want="map", select=sel)
                else:
                    m = ops.train_gt_unary_batch(sl, shape, eps=0.00001, want="labels", select=[sel])[0]
                masks.append(m.cpu().numpy().astype(np.int64))
    return masks


def _assert_masks_equal(got, want, ims, labels, tag):
    assert len(got) == len(want) == len(ims), tag
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], (tag, k)
        assert np.array_equal(a, b), "%s: mask %d differs from the staged composition on %d pixels" % (tag, k, int((a != b).sum()))
        assert set(np.unique(a)) <= set([0] + labels[k]), (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_predict_train_gt_many_equals_the_staged_composition(graphed):
    from dsrg_amd import inference as I
    ims, labels = _e2e_items(41)
    assert [im.shape[:2] for im in ims] == _E2E_SHAPES
    net = TinyNet().cuda().eval()
    G = 4

    def forward():
        return I.GraphedForward(net) if graphed else None

    ref_fwd = forward()
    want = _staged_gt(ref_fwd or net, ims, labels, G, _SIZE, True)
    want_plain = _staged_gt(ref_fwd or net, ims, labels, G, _SIZE, False)
    assert max(len(np.unique(m)) for m in want) >= 2 and max(len(np.unique(m)) for m in want_plain) >= 2
    for in_flight, batch in ((2, 1), (3, 2), (2, 2)):
        fwd = forward()
        got = list(I.predict_train_gt_many(net, iter(zip(ims, labels)), size=_SIZE, forward=fwd, in_flight=in_flight, batch=batch,
                                           forward_batch=G))
        _assert_masks_equal(got, want, ims, labels, "in_flight %d batch %d" % (in_flight, batch))
        if graphed:
            assert [key[0] for key in fwd._g] == [(G, 3, _SIZE, _SIZE)]          # ONE batch-G graph, the padded tail group included
    fwd = forward()
    got = list(I.predict_train_gt_many(net, zip(ims, labels), smooth=False, size=_SIZE, forward=fwd, forward_batch=G))
    _assert_masks_equal(got, want_plain, ims, labels, "smooth=False")
    if graphed:
        assert [key[0] for key in fwd._g] == [(G, 3, _SIZE, _SIZE)]
    # forward_batch=1: the per-image route on the same kernels
    for smooth in (True, False):
        fwd = forward()
        one = list(I.predict_train_gt_many(net, zip(ims[:3], labels[:3]), smooth=smooth, size=_SIZE, forward=fwd))
        _assert_masks_equal(one, _staged_gt(fwd or net, ims[:3], labels[:3], 1, _SIZE, smooth), ims[:3], labels[:3], "forward_batch=1")
    # ignore_below reaches both routes: above 1 everything is 255
    for smooth in (True, False):
        m = list(I.predict_train_gt_many(net, zip(ims[:2], labels[:2]), smooth=smooth, size=_SIZE, forward_batch=2, ignore_below=1.5))
        assert all((a == 255).all() for a in m)


def _margin_among(q, sel):
    top2 = np.sort(q[..., sorted(set(sel))], axis=2)[:, :, -2:]
    return top2[:, :, 1] - top2[:, :, 0] if top2.shape[2] == 2 else np.full(q.shape[:2], np.inf)


@pytest.mark.gpu
def test_predict_train_gt_many_agrees_with_predict_train_gt():
    """batch-G forwards and the fused tail against the per-image torch composition: agreement above 0.999 per image, every differing
    pixel with a top-2 margin below 1e-3 among the selected labels in predict_train_gt's own CRF marginals (smooth) or
    probabilities (smooth=False)"""
    from dsrg_amd import inference as I
    from dsrg_amd.crf import CRF_device
    ims, labels = _e2e_items(47)
    ims, labels = ims[:5], labels[:5]
    net = TinyNet().float().cuda().eval()
    got_smooth = list(I.predict_train_gt_many(net, zip(ims, labels), forward_batch=4))              # size 321, as predict_train_gt
    got_plain = list(I.predict_train_gt_many(net, zip(ims, labels), smooth=False, forward_batch=4))
    for k, (im, lab) in enumerate(zip(ims, labels)):
        sel = I.train_gt_selection(lab)
        with torch.no_grad():
            scores = net(I.preprocess(im, 321)).float()
            probs = torch.clamp(I._zoom(torch.softmax(scores, dim=1), im.shape[0], im.shape[1])[0], min=0.00001)
            q = CRF_device(torch.as_tensor(im, device="cuda"), torch.log(probs).permute(1, 2, 0).contiguous(), scale_factor=1.0)
        for smooth, got, ref in ((True, got_smooth[k], q.cpu().numpy()), (False, got_plain[k], probs.permute(1, 2, 0).cpu().numpy())):
            want = I.predict_train_gt(net, im, lab, smooth=smooth)
            margin = _margin_among(ref, sel)
            bad = got != want
            agree = 1.0 - bad.mean()
            print("image %d smooth=%s: agreement with predict_train_gt %.6f; %d differing pixels, largest top-2 margin among them %.3g"
                  % (k, smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0))
            assert got.shape == want.shape and got.dtype == np.int64
            assert agree > 0.999
            assert not bad.any() or margin[bad].max() < 1e-3


@pytest.mark.gpu
def test_predict_train_gt_many_vs_reference_restatement():
    """generate_train_gt.py:78-106 in numpy / scipy for one 97 x 131 image, the network evaluated by the same TinyNet on the CPU in
    float64 and the CRF by the oracle: agreement above 0.999, every differing pixel with a top-2 margin below 1e-3 among the
    selected labels in the restatement's marginals"""
    import scipy.ndimage as nd
    from dsrg_amd import inference as I, synthetic as S
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    H, W = 97, 131
    im = (S.make_images(rng, 1, size=max(H, W))[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
    im = np.ascontiguousarray(im[:, :, ::-1]).astype(np.uint8)            # an "RGB" uint8 image
    net = TinyNet().cuda().eval()
    netc = TinyNet().double().eval()
    d1, d2 = float(H), float(W)
    x = nd.zoom(im.astype('float32'), (321 / d1, 321 / d2, 1.0), order=1)[:, :, [2, 1, 0]] - np.array(I.MEAN_PIXEL)
    with torch.no_grad():
        scores = netc(torch.tensor(x.transpose(2, 0, 1)[None], dtype=torch.float64))[0].numpy().transpose(1, 2, 0)
    e = np.exp(scores - np.max(scores, axis=2, keepdims=True))
    probs = e / np.sum(e, axis=2, keepdims=True)
    probs = nd.zoom(probs, (d1 / probs.shape[0], d2 / probs.shape[1], 1.0), order=1)
    probs[probs < 0.00001] = 0.00001
    # the image-level labels: the three foreground classes the restatement's own unrestricted arg-max uses most
    counts = np.bincount(np.argmax(probs[:, :, 1:], axis=2).ravel() + 1, minlength=21)
    labels = np.sort(np.argsort(-counts)[:3])
    q = O.CRF(im, np.log(probs), scale_factor=1.0)
    for smooth, ref in ((True, q), (False, probs)):
        sel = labels.tolist()
        sel.insert(0, 0)
        want = np.vectorize(lambda j: sel[j])(np.argmax(ref[:, :, sel], axis=2))
        got = list(I.predict_train_gt_many(net, [(im, labels)], smooth=smooth))[0]
        margin = _margin_among(ref, sel)
        bad = got != want
        agree = 1.0 - bad.mean()
        print("smooth=%s: agreement with the reference restatement %.6f; %d differing pixels, largest top-2 margin among them %.3g; "
              "labels in the mask %s" % (smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0,
                                         np.unique(got).tolist()))
        assert got.shape == (H, W) and got.dtype == np.int64
        assert agree > 0.999
        assert not bad.any() or margin[bad].max() < 1e-3
        assert set(np.unique(got)) <= set(sel) and len(np.unique(got)) >= 2
