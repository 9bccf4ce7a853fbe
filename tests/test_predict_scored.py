"""Scoring the multi-scale test against ground truth as it runs (GPU): masks="device" of the four *_many generators,
inference.MaskScorer, and `python -m dsrg_amd.predict --gt` against `predict --output` followed by `python -m dsrg_amd.evaluate`.
Every comparison is exact: label maps value for value, integer counters, result files and PNGs byte for byte."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 21
SIZES = [(97, 129), (120, 90), (97, 129), (81, 113), (120, 90)]       # three distinct sizes; 0/2 and 1/4 share one
IDS = ["2007_00000%d" % (k + 1) for k in range(len(SIZES))]
CUE_LABELS = [[3, 7], [12], [1, 20, 5], [7], [2, 9]]


def _vgg(seed):
    """VGG16-ASPP in eval mode, He-initialised with zero biases: the masks of a random net then hold several labels"""
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(seed)
    net = VGG16ASPP(num_classes=C)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                torch.nn.init.zeros_(m.bias)
    return net.cuda().to(memory_format=torch.channels_last).eval()


def _ground_truth(rng, H, W):
    """about a tenth of the pixels at 255, a few in C..254, the rest a coarse pattern of labels"""
    gt = np.repeat(np.repeat(rng.integers(0, C, size=((H + 7) // 8, (W + 7) // 8)), 8, 0), 8, 1)[:H, :W].astype(np.uint8)
    u = rng.random((H, W))
    gt[u < 0.10] = 255
    gt[(u >= 0.10) & (u < 0.12)] = rng.integers(C, 255, size=(H, W)).astype(np.uint8)[(u >= 0.10) & (u < 0.12)]
    return gt


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the files of a run: weights, JPEGs, ground-truth PNGs, the two list formats and the cue pickle; the decoded images"""
    from PIL import Image
    from dsrg_amd import checkpoint, synthetic as S
    from dsrg_amd.predict import read_image
    root = tmp_path_factory.mktemp("scored")
    net = _vgg(seed=4)
    model = str(root / "net.caffemodel")
    checkpoint.save_weights(net, model)
    voc, gt_dir = root / "VOC", root / "GT"
    (voc / "JPEGImages").mkdir(parents=True)
    gt_dir.mkdir()
    rng = np.random.default_rng(12)
    gts = []
    for img_id, (H, W) in zip(IDS, SIZES):
        im = (S.make_images(rng, 1, size=max(H, W), kind="noise")[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
        im = np.ascontiguousarray(im[:, :, ::-1]).clip(0, 255).astype(np.uint8)
        Image.fromarray(im, mode="RGB").save(str(voc / "JPEGImages" / (img_id + ".jpg")), quality=95)
        gts.append(_ground_truth(rng, H, W))
        Image.fromarray(gts[-1], mode="L").save(str(gt_dir / (img_id + ".png")))
    (root / "val.txt").write_text("\n".join(IDS) + "\n")
    (root / "input_list.txt").write_text("".join("%s.jpg %d\n" % (i, k) for k, i in enumerate(IDS)))
    with open(str(root / "cues.pickle"), "wb") as f:
        pickle.dump({"%d_labels" % k: np.array(l) for k, l in enumerate(CUE_LABELS)}, f, protocol=2)
    images = [read_image(str(voc / "JPEGImages" / (i + ".jpg"))) for i in IDS]
    return dict(root=root, net=net, model=model, voc=str(voc), gt_dir=str(gt_dir), gts=gts, images=images,
                val=str(root / "val.txt"), gt_list=str(root / "input_list.txt"), cues=str(root / "cues.pickle"))


def _generator(world, which, batched, smooth, masks):
    from dsrg_amd import inference as I
    net, images = world["net"], world["images"]
    if which == "ms":
        return I.predict_masks_ms_many(net, images, sizes=(97, 129), forward_batch=2 if batched else 1, batch=2, smooth=smooth,
                                       masks=masks)
    if which == "ms-f":
        return I.predict_masks_ms_f_many(net, images, same_size_batch=2 if batched else 1, batch=2, smooth=smooth, masks=masks)
    items = list(zip(images, CUE_LABELS))
    if which == "gt":
        return I.predict_train_gt_many(net, items, size=97, forward_batch=2 if batched else 1, batch=2, smooth=smooth, masks=masks)
    return I.predict_train_gt_ms_many(net, items, sizes=(97, 129), flip=True, forward_batch=2 if batched else 1, batch=2,
                                      smooth=smooth, masks=masks)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("which", ["ms", "ms-f", "gt", "gt-ms"])
def test_device_masks_equal_host_masks(world, which, batched, smooth):
    host = list(_generator(world, which, batched, smooth, "host"))
    caller = torch.cuda.current_stream()
    device = []
    for lab in _generator(world, which, batched, smooth, "device"):
        # handed over with the caller's stream current, whatever stream the generator works on in between
        assert torch.cuda.current_stream() == caller
        assert lab.is_cuda and lab.dtype == torch.int32 and lab.is_contiguous()
        device.append(lab)
    assert torch.cuda.current_stream() == caller
    assert len(host) == len(device) == len(SIZES)
    for k, (h, d) in enumerate(zip(host, device)):
        assert tuple(d.shape) == SIZES[k] == h.shape
        assert np.array_equal(d.cpu().numpy().astype(np.int64), h), (which, k)
    assert len(set(np.concatenate([h.ravel() for h in host]).tolist())) > 1


def test_masks_keyword_is_checked(world):
    with pytest.raises(ValueError, match="masks"):
        next(_generator(world, "ms", False, False, "numpy"))
    with pytest.raises(ValueError, match="masks"):
        next(_generator(world, "gt-ms", True, True, None))


@pytest.mark.parametrize("want_masks", [False, True])
@pytest.mark.parametrize("rule_lt", [True, False])
def test_mask_scorer_equals_generate_m(world, want_masks, rule_lt):
    """21 label maps: a full group of 16 and a last group of 5"""
    from dsrg_amd import inference as I
    host = list(_generator(world, "ms-f", True, True, "host"))
    device = list(_generator(world, "ms-f", True, True, "device"))
    n = 21
    labs, gts, hosts = ([seq[k % 5] for k in range(n)] for seq in (device, world["gts"], host))
    scorer = I.MaskScorer(C, "cuda", rule_lt=rule_lt, want_masks=want_masks)
    out = []
    for k0 in (0, 16):
        got = scorer.add(labs[k0:k0 + 16], gts[k0:k0 + 16])
        assert (got is not None) == want_masks
        out += got or []
    cm = I.ConfusionMatrix(C)
    stray = 0
    for gt, h in zip(gts, hosts):
        if rule_lt:
            cm.addM(cm.generateM((gt, h)))
        else:                                                # add has no place for a ground truth in C..254: the last counter's
            fits = (gt < C) | (gt == 255)
            stray += int((~fits).sum())
            cm.add(gt[fits], h[fits])
    counts = scorer.counts()
    assert counts.dtype == np.int64 and counts.shape == (C * C + 1,)
    assert counts[-1] == stray and (stray > 0) == (not rule_lt)
    assert np.array_equal(counts[:-1].reshape(C, C), cm.M.astype(np.int64))
    if want_masks:
        for m, h in zip(out, hosts):
            assert m.dtype == np.uint8 and np.array_equal(m, h.astype(np.uint8))
    if rule_lt:
        r = scorer.result(n)
        miou, per, M = cm.jaccard()
        assert r["miou"] == float(miou) and r["iou"] == [float(j) for j in per] and r["images"] == n
        assert np.array_equal(r["matrix"], M)
    # a shape mismatch: refused before any copy or launch
    before = scorer.counts().copy()
    with pytest.raises(ValueError):
        scorer.add(labs[:2], [gts[0], gts[1][:, :-1]])
    with pytest.raises(ValueError):
        scorer.add(labs[:17], gts[:17])
    with pytest.raises(ValueError):
        scorer.add(labs[:2], gts[:1])
    assert np.array_equal(scorer.counts(), before)


def _predict(args, capsys):
    from dsrg_amd import predict
    capsys.readouterr()
    assert predict.main(args) == 0
    return capsys.readouterr().out


def _evaluate(world, pred, save, ids_file, capsys):
    from dsrg_amd import evaluate
    assert evaluate.main(["--pred", pred, "--gt", world["gt_dir"], "--test_ids", ids_file, "--save_path", save, "--class_num",
                          str(C)]) == 0
    capsys.readouterr()
    return open(save, "rb").read()


def _pngs(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_predict_gt_is_predict_then_evaluate(world, capsys, tmp_path):
    common = ["--mode", "ms-f", "--smooth", "--model", world["model"], "--images", world["val"], "--dir", world["voc"]]
    scored, plain = str(tmp_path / "scored"), str(tmp_path / "plain")
    r, e, r2 = (str(tmp_path / n) for n in ("r.txt", "e.txt", "r2.txt"))
    out = _predict(common + ["--gt", world["gt_dir"], "--output", scored, "--save_path", r], capsys)
    assert "meanIOU: " in out
    want = _evaluate(world, scored, e, world["val"], capsys)
    assert open(r, "rb").read() == want
    assert out.strip().split("\n")[-1] == want.decode().split("\n")[0]
    # the same command without --gt writes the same PNGs
    _predict(common + ["--output", plain], capsys)
    assert sorted(_pngs(plain)) == [i + ".png" for i in IDS] and _pngs(plain) == _pngs(scored)
    # ... and without --output the same result and no PNG, with a progress line every two images
    before = set(os.listdir(str(tmp_path)))
    out = _predict(common + ["--gt", world["gt_dir"], "--save_path", r2, "--score-every", "2"], capsys)
    assert open(r2, "rb").read() == want
    assert set(os.listdir(str(tmp_path))) - before == {"r2.txt"}
    progress = [l for l in out.split("\n") if " images, meanIOU = " in l]
    assert [l.split(" ")[0] for l in progress] == ["2", "4"]


def test_predict_gt_in_pseudo_label_mode(world, capsys, tmp_path):
    out_dir, r, e = (str(tmp_path / n) for n in ("out", "r.txt", "e.txt"))
    _predict(["--mode", "gt", "--cues", world["cues"], "--model", world["model"], "--images", world["gt_list"], "--dir", world["voc"],
              "--scales", "97", "--forward-batch", "2", "--gt", world["gt_dir"], "--output", out_dir, "--save_path", r], capsys)
    assert open(r, "rb").read() == _evaluate(world, out_dir, e, world["val"], capsys)


def test_predict_gt_of_the_wrong_size_names_the_image(world, capsys, tmp_path):
    from PIL import Image
    from dsrg_amd import predict
    bad = tmp_path / "GT"
    bad.mkdir()
    Image.fromarray(world["gts"][1][:, :-1].copy(), mode="L").save(str(bad / (IDS[1] + ".png")))
    (tmp_path / "one.txt").write_text(IDS[1] + "\n")
    with pytest.raises(ValueError, match=IDS[1]):
        predict.main(["--mode", "ms", "--scales", "97", "--model", world["model"], "--images", str(tmp_path / "one.txt"), "--dir",
                      world["voc"], "--gt", str(bad)])
    capsys.readouterr()
