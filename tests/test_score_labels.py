"""dsrg_score_labels_batch (csrc/eval.hip; ops.score_labels_batch): the confusion counters of a group of differently sized int32
label maps against their uint8 ground truth, and the maps narrowed to bytes.

CPU: the options of `python -m dsrg_amd.predict` that go with --gt; a numpy restatement of the kernel's rule against
ConfusionMatrix.add / generateM; the argument checks of the entry point, which come before the first device call.
GPU: the kernel against the restatement, exactly (integer counters, bytes), both keep rules.
"""
import ctypes

import numpy as np
import pytest
import torch


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
def restate(labels, gts, C, ignore_label=255, rule_lt=False):
    """-> (C*C + 1 int64 counters, the uint8 masks) of a group of (H, W) integer label maps and uint8 ground truths"""
    hist = np.zeros(C * C + 1, np.int64)
    masks = []
    for lab, gt in zip(labels, gts):
        assert lab.shape == gt.shape
        l, t = lab.astype(np.int64).ravel(), gt.astype(np.int64).ravel()
        keep = (t < C) if rule_lt else (t != ignore_label)
        inside = keep & (t < C) & (l >= 0) & (l < C)
        hist[:C * C] += np.bincount(t[inside] * C + l[inside], minlength=C * C)
        hist[C * C] += int((keep & ~inside).sum())
        masks.append(np.where((lab >= 0) & (lab <= 255), lab, 255).astype(np.uint8))
    return hist, masks


def make_group(rng, shapes, C, odd_predictions=False):
    """random label maps in 0..C-1 and ground truth with about a tenth of the pixels at 255, a few in C..254 and the rest below C;
    odd_predictions: some labels are 255 (ignore_below's value) and some negative"""
    labels, gts = [], []
    for H, W in shapes:
        lab = rng.integers(0, C, size=(H, W)).astype(np.int32)
        gt = rng.integers(0, C, size=(H, W)).astype(np.uint8)
        u = rng.random((H, W))
        gt[u < 0.10] = 255
        if C < 254:
            between = (u >= 0.10) & (u < 0.13)
            gt[between] = rng.integers(C, 255, size=(H, W)).astype(np.uint8)[between]
        if odd_predictions:
            v = rng.random((H, W))
            lab[v < 0.05] = 255
            lab[(v >= 0.05) & (v < 0.08)] = -3
        labels.append(lab)
        gts.append(gt)
    return labels, gts


FIVE = [(1, 1), (7, 300), (33, 17), (1, 257), (256, 1)]      # 2 100 + 561 + 1 + 257 + 256 = 3 175 pixels: runs straddle the seams


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def _parse(extra):
    from dsrg_amd.predict import parse_args
    return parse_args(["--mode", "ms-f", "--model", "m", "--images", "i", "--dir", "d"] + extra)


def test_predict_options_that_go_with_gt(capsys):
    a = _parse(["--gt", "GT"])
    assert a.output is None and a.gt == "GT" and a.score_every == 100 and a.save_path is None and a.image_subdir == "JPEGImages"
    a = _parse(["--gt", "GT", "--output", "OUT", "--save_path", "r.txt", "--score-every", "7", "--image-subdir", "images/val2014"])
    assert (a.output, a.save_path, a.score_every, a.image_subdir) == ("OUT", "r.txt", 7, "images/val2014")
    a = _parse(["--output", "OUT"])                                    # an unscored run, as before
    assert a.gt is None and a.output == "OUT"
    for bad in ([], ["--output", "OUT", "--save_path", "r.txt"], ["--output", "OUT", "--score-every", "5"],
                ["--gt", "GT", "--score-every", "0"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    capsys.readouterr()


@pytest.mark.parametrize("C", [1, 21, 96])
def test_restatement_agrees_with_the_confusion_matrix_class(C):
    from dsrg_amd.inference import ConfusionMatrix
    rng = np.random.default_rng(100 + C)
    labels, gts = make_group(rng, [(40, 50), (13, 7), (1, 300)], C)
    assert any((g == 255).any() for g in gts) and any((g < C).any() for g in gts)
    assert any(((g >= C) & (g < 255)).any() for g in gts)
    # generateM keeps ground truth < C: every kept pixel is inside the matrix
    hist, masks = restate(labels, gts, C, rule_lt=True)
    cm = ConfusionMatrix(C)
    want = sum(cm.generateM((g, l)) for g, l in zip(gts, labels))
    assert hist[-1] == 0 and np.array_equal(hist[:-1].reshape(C, C), want.astype(np.int64))
    # add keeps ground truth != 255 and has no place for a ground truth in C..254 (its bincount outgrows the matrix): those pixels
    # are the restatement's last counter, the others are add's matrix
    hist, _ = restate(labels, gts, C, rule_lt=False)
    cm = ConfusionMatrix(C)
    stray = 0
    for g, l in zip(gts, labels):
        fits = (g < C) | (g == 255)
        stray += int((~fits).sum())
        cm.add(g[fits], l[fits])
    assert hist[-1] == stray and stray > 0
    assert np.array_equal(hist[:-1].reshape(C, C), cm.M.astype(np.int64))
    # the byte: astype(uint8) of everything the project writes (0..C-1 and the 255 of ignore_below)
    for lab, m in zip(labels, masks):
        assert m.dtype == np.uint8 and np.array_equal(m, lab.astype(np.uint8))


def test_restatement_counts_odd_predictions_and_narrows_them():
    C = 21
    labels, gts = make_group(np.random.default_rng(5), [(30, 40)], C, odd_predictions=True)
    lab, gt = labels[0], gts[0]
    for rule_lt in (False, True):
        hist, masks = restate(labels, gts, C, rule_lt=rule_lt)
        keep = (gt < C) if rule_lt else (gt != 255)
        assert hist.sum() == keep.sum()
        assert hist[-1] == (keep & ((gt >= C) | (lab < 0) | (lab >= C))).sum() > 0
        assert np.array_equal(masks[0][lab == 255], np.full((lab == 255).sum(), 255, np.uint8))
        assert (masks[0][lab < 0] == 255).all() and np.array_equal(masks[0][lab >= 0], lab[lab >= 0].astype(np.uint8))


def test_score_labels_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def ptrs(n, hole=None):
        return (ctypes.c_void_p * max(n, 1))(*[None if k == hole else fake for k in range(max(n, 1))])

    def sizes(n, v):
        return (ctypes.c_int32 * max(n, 1))(*([v] * max(n, 1)))

    def call(G, C, labels=0, gt=0, H=0, W=0, hist=fake, mask=None):
        return L.dsrg_score_labels_batch(G, C, ptrs(G) if labels == 0 else labels, ptrs(G) if gt == 0 else gt,
                                         sizes(G, 4) if H == 0 else H, sizes(G, 5) if W == 0 else W, 255, 1, hist, mask, None)

    def refused(rc, code, word):
        return rc == code and word in L.dsrg_last_error()

    assert refused(call(0, 21), _lib.ERR_INVALID, b"images")
    assert refused(call(17, 21), _lib.ERR_INVALID, b"images")
    assert refused(call(2, 0), _lib.ERR_INVALID, b"labels")
    assert refused(call(2, 97), _lib.ERR_UNSUPPORTED, b"96")
    for kw in (dict(labels=None), dict(gt=None), dict(H=None), dict(W=None), dict(hist=None)):
        assert refused(call(2, 21, **kw), _lib.ERR_INVALID, b"NULL"), kw
    assert refused(call(3, 21, labels=ptrs(3, hole=1)), _lib.ERR_INVALID, b"NULL")
    assert refused(call(3, 21, gt=ptrs(3, hole=2)), _lib.ERR_INVALID, b"NULL")
    assert refused(call(3, 21, mask=ptrs(3, hole=0)), _lib.ERR_INVALID, b"NULL")
    assert refused(call(2, 21, H=(ctypes.c_int32 * 2)(4, 0)), _lib.ERR_INVALID, b"0x5")
    assert refused(call(2, 21, W=(ctypes.c_int32 * 2)(0, 5)), _lib.ERR_INVALID, b"4x0")
    assert refused(call(16, 21, H=sizes(16, 16384), W=sizes(16, 8192)), _lib.ERR_INVALID, b"2^31")
    assert refused(call(2, 21, H=sizes(2, 2147483647), W=sizes(2, 2147483647)), _lib.ERR_INVALID, b"2^31")
    # (no well-formed call here: with a GPU present it would launch on the fake pointers.  Every refusal above left the process
    # usable: each was followed by further calls into the library)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _score(labels, gts, C, rule_lt, hist=None, want_masks=True, ignore_label=255):
    from dsrg_amd import ops
    dl = [torch.from_numpy(l).cuda() for l in labels]
    dg = [torch.from_numpy(g).cuda() for g in gts]
    dm = [torch.full(l.shape, 77, dtype=torch.uint8, device="cuda") for l in labels] if want_masks else None
    out = ops.score_labels_batch(dl, dg, C, ignore_label=ignore_label, rule_lt=rule_lt, hist=hist, masks=dm)
    assert out.dtype == torch.int64 and out.numel() == C * C + 1 and (hist is None or out is hist)
    return out, dm


def _check(labels, gts, C, rule_lt, want_masks=True):
    got, masks = _score(labels, gts, C, rule_lt, want_masks=want_masks)
    want, bytes_ = restate(labels, gts, C, rule_lt=rule_lt)
    assert np.array_equal(got.cpu().numpy(), want)
    if want_masks:
        for g, (m, b) in enumerate(zip(masks, bytes_)):
            assert np.array_equal(m.cpu().numpy(), b), "mask %d" % g
    return want


SHAPES = {
    "one_pixel": [(1, 1)],
    "five": FIVE,
    "under_256": [(5, 7), (2, 3), (10, 10)],                           # 141 pixels: one workgroup, most lanes idle
    "sixteen": [(1 + 3 * g, 40 - 2 * g) for g in range(16)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("rule_lt", [False, True])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_equals_the_restatement(name, rule_lt):
    labels, gts = make_group(np.random.default_rng(sorted(SHAPES).index(name)), SHAPES[name], 21)
    want = _check(labels, gts, 21, rule_lt)
    assert want.sum() > 0 or name == "one_pixel"
    _check(labels, gts, 21, rule_lt, want_masks=False)                 # (the path that reads no label of a dropped pixel)


@pytest.mark.gpu
@pytest.mark.parametrize("rule_lt", [False, True])
@pytest.mark.parametrize("C", [1, 21, 96])
def test_label_counts(C, rule_lt):
    """C = 96 is the largest LDS histogram, 36 868 bytes"""
    labels, gts = make_group(np.random.default_rng(C), FIVE, C)
    want = _check(labels, gts, C, rule_lt)
    assert (want[-1] > 0) == (not rule_lt)


@pytest.mark.gpu
@pytest.mark.parametrize("rule_lt", [False, True])
def test_an_image_that_is_all_ignored(rule_lt):
    labels, gts = make_group(np.random.default_rng(8), [(19, 23), (40, 30), (3, 3)], 21)
    gts[1][:] = 255
    _check(labels, gts, 21, rule_lt)
    _check(labels, gts, 21, rule_lt, want_masks=False)
    want = _check(labels[1:2], gts[1:2], 21, rule_lt)
    assert want.sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rule_lt", [False, True])
def test_predictions_outside_the_labels(rule_lt):
    """the 255 of ignore_below and a negative value go to the last counter and come out as the byte 255"""
    labels, gts = make_group(np.random.default_rng(9), [(31, 33), (8, 200)], 21, odd_predictions=True)
    labels[0][0, :4] = [256, 1000, -1, -2147483648]
    want = _check(labels, gts, 21, rule_lt)
    assert want[-1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("rule_lt", [False, True])
def test_voc_sized_images_run_the_strided_loop(rule_lt):
    """2 x 375 x 500 = 375 000 pixels > kEvalMaxBlocks * 256 = 262 144"""
    labels, gts = make_group(np.random.default_rng(10), [(375, 500), (375, 500)], 21)
    _check(labels, gts, 21, rule_lt)


@pytest.mark.gpu
def test_two_calls_accumulate_and_a_side_stream_gives_the_same():
    C = 21
    a = make_group(np.random.default_rng(11), FIVE, C)
    b = make_group(np.random.default_rng(12), SHAPES["sixteen"], C, odd_predictions=True)
    for rule_lt in (False, True):
        hist, _ = _score(a[0], a[1], C, rule_lt)
        hist, _ = _score(b[0], b[1], C, rule_lt, hist=hist)
        want = restate(a[0], a[1], C, rule_lt=rule_lt)[0] + restate(b[0], b[1], C, rule_lt=rule_lt)[0]
        assert np.array_equal(hist.cpu().numpy(), want)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            on_side, masks = _score(b[0], b[1], C, rule_lt)
        side.synchronize()
        on_default, masks0 = _score(b[0], b[1], C, rule_lt)
        assert torch.equal(on_side, on_default)
        assert all(torch.equal(m, m0) for m, m0 in zip(masks, masks0))


@pytest.mark.gpu
def test_another_ignore_label_under_the_not_equal_rule():
    labels, gts = make_group(np.random.default_rng(13), [(20, 20)], 21)
    got, _ = _score(labels, gts, 21, False, ignore_label=254)
    assert np.array_equal(got.cpu().numpy(), restate(labels, gts, 21, ignore_label=254)[0])


@pytest.mark.gpu
def test_wrapper_refuses_mismatched_inputs():
    from dsrg_amd import ops
    lab = torch.zeros((4, 5), dtype=torch.int32, device="cuda")
    gt = torch.zeros((4, 5), dtype=torch.uint8, device="cuda")
    for labels, gts, masks in (([lab], [gt[:, :4].contiguous()], None), ([lab.long()], [gt], None), ([lab], [gt, gt], None),
                               ([lab], [gt], [gt[:3].contiguous()]), ([], [], None)):
        with pytest.raises(ValueError):
            ops.score_labels_batch(labels, gts, 21, masks=masks)
