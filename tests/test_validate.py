"""dsrg_amd.validate on the GPU: Validator.run against a host computation on the same forward's scores, sharding over ranks, a
training run left untouched by a validation pass, and the two commands (`python -m dsrg_amd.train --val-list`, `python -m
dsrg_amd.validate`) in child processes.  All inputs are tiny synthetic files; the crop is 65 and batches hold 2 images.  Counters are
compared as integers, checksums as integers, the mean IoU as the float that ConfusionMatrix.jaccard returns for those counters."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_confusion_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((40, 50), (65, 65), (50, 41), (64, 47), (45, 60))
CROP, BATCH, C = 65, 2, 21

pytestmark = pytest.mark.gpu


def _net(seed=11):
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(seed)
    net = VGG16ASPP(num_classes=C)
    with torch.no_grad():                                              # torch's default initialisation lets the signal die out on the way up, and
        for p in net.parameters():                                     # the classifier's bias would decide every pixel alike: keep it alive
            if p.dim() == 4:                                           # (ReLU's gain: sqrt(6) on a uniform(+-1/sqrt(fan_in)) kernel)
                p.mul_(2.45)
    return net.cuda().to(memory_format=torch.channels_last)


def _run_hooked(validator):
    """-> (result, [the scores of each forward as float32 arrays])"""
    seen = []
    hook = validator.net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().cpu().numpy()))
    try:
        return validator.run(), seen
    finally:
        hook.remove()


def _host_counts(seen, labels):
    """the NumPy restatement on the scores the forwards gave and the labels of the PNGs, 255 outside the image, batch by batch"""
    hist = np.zeros(C * C + 1, dtype=np.int64)
    assert [s.shape[0] for s in seen] == [min(BATCH, len(labels) - k) for k in range(0, len(labels), BATCH)]
    for k, scores in zip(range(0, len(labels), BATCH), seen):
        assert scores.shape[1] == C
        hist += K.counters(scores, K.padded_labels(labels[k:k + BATCH], CROP), C, rule_lt=True)
    return hist


def test_validator_equals_the_host_computation_and_shards_over_ranks(tmp_path):
    from dsrg_amd.inference import ConfusionMatrix
    from dsrg_amd.validate import Validator
    rng = np.random.default_rng(51)
    lst, root, labels = K.write_val_files(tmp_path, rng, SIZES)
    net = _net()
    assert net.training
    res, seen = _run_hooked(Validator(net, lst, root, crop=CROP, batch=BATCH, num_classes=C))
    assert net.training                                                # the mode it was found in
    want = _host_counts(seen, labels)
    assert np.array_equal(res["counts"], want)
    assert res["images"] == 5 and want[-1] == 0
    assert want[:-1].sum() == sum(int((lab != 255).sum()) for lab in labels)          # every labelled pixel once, nothing off the images
    cm = ConfusionMatrix(C)
    cm.M += want[:-1].reshape(C, C)
    miou, per, M = cm.jaccard()
    assert res["miou"] == float(miou) and res["iou"] == [float(j) for j in per] and np.array_equal(res["matrix"], M)
    assert res["pixel_accuracy"] == float(np.trace(M) / M.sum())
    assert len(np.unique(np.argmax(seen[0][0], axis=0))) > 2           # (the net tells regions apart: several labels are predicted)
    assert np.count_nonzero(want[:-1].reshape(C, C).sum(0)) > 2

    # an eval-mode net stays in eval mode, and the pass repeats itself
    net.eval()
    again = Validator(net, lst, root, crop=CROP, batch=BATCH, num_classes=C).run()
    assert not net.training and np.array_equal(again["counts"], want)

    # ranks 0 and 1 of world 2, one after the other, without a process group: their counters sum to the single rank's
    parts = []
    for rank in (0, 1):
        r, s = _run_hooked(Validator(net, lst, root, crop=CROP, batch=BATCH, num_classes=C, rank=rank, world_size=2))
        assert np.array_equal(r["counts"], _host_counts(s, labels[rank::2]))
        parts.append(r)
    assert [p["images"] for p in parts] == [3, 2]
    assert np.array_equal(parts[0]["counts"] + parts[1]["counts"], want)
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_val_input_is_one_finite_pass_over_the_ranks(tmp_path, n):
    """ValInput on n images of 8 x 8 at crop 16 and batch 2, world sizes 1 and 2: every listed image comes exactly once over the
    ranks and in list order within a rank (told apart by its label plane), a rank beyond the end of a one-image list yields nothing,
    the pass ends in StopIteration and the loader is closed after it"""
    from dsrg_amd.validate import ValInput
    lst, root, labels = K.write_val_files(tmp_path, np.random.default_rng(60 + n), ((8, 8),) * n)
    want = K.padded_labels(labels, 16)
    assert len({w.tobytes() for w in want}) == n                       # (the label planes tell the images apart)
    for world in (1, 2):
        seen = []
        for rank in range(world):
            share = list(range(rank, n, world))
            loader = ValInput(lst, root, crop=16, batch_size=2, workers=2, rank=rank, world_size=world)
            got = []
            for k in range(0, len(share), 2):
                data, label = next(loader)
                m = min(2, len(share) - k)
                assert tuple(data.shape) == (m, 3, 16, 16) and tuple(label.shape) == (m, 1, 16, 16)
                assert not data[:, :, 8:].any() and not data[:, :, :, 8:].any()         # nothing off the 8 x 8 images
                for plane in label.cpu().numpy():
                    got += [i for i in range(n) if np.array_equal(plane, want[i])]
            assert got == share, (world, rank)
            with pytest.raises(StopIteration):
                next(loader)
            with pytest.raises(RuntimeError, match="loader is closed"):
                next(loader)
            seen += got
        assert sorted(seen) == list(range(n)), world
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


def test_validation_between_two_steps_leaves_the_run_bit_identical(tmp_path):
    from dsrg_amd.retrain import RetrainTrainer
    from dsrg_amd.trainer import params_checksum
    from dsrg_amd.validate import Validator
    rng = np.random.default_rng(52)
    lst, root, _ = K.write_val_files(tmp_path, rng, SIZES[:3])
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(2, 3, CROP, CROP, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (2, 1, CROP, CROP), generator=g).float().cuda()

    def two_steps(validate):
        tr = RetrainTrainer(torch.device("cuda", torch.cuda.current_device()), backbone="vgg16", max_iter=10, seed=3)
        losses = [tr.step(images, label).item()]
        if validate:
            res = Validator(tr.net, lst, root, crop=CROP, batch=BATCH, num_classes=C, amp_dtype=tr.amp_dtype).run()
            assert res["images"] == 3 and tr.net.training
        losses.append(tr.step(images, label).item())
        words = params_checksum(list(tr.net.parameters()) + [b for grp in tr.opt.groups for b in grp["bufs"]])
        return losses, [int(v) for v in words.cpu()]

    assert two_steps(True) == two_steps(False)


def _run(module, args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


_VAL_LINE = re.compile(r"^Iteration (\d+), validation: meanIOU = ([-+.\dnaife]+), pixel accuracy = ([-+.\dnaife]+) \((\d+) images\)$")


def _val_lines(out):
    return [m.groups() for m in (_VAL_LINE.match(ln) for ln in out.splitlines()) if m]


def _done(out):
    ln = [ln for ln in out.splitlines() if ln.startswith("done: ")][-1].split()
    return int(ln[2]), (int(ln[4]), int(ln[5]))


def test_train_command_stage_f_with_validation_in_a_child_process(tmp_path):
    rng = np.random.default_rng(53)
    (tmp_path / "train").mkdir()
    (tmp_path / "val").mkdir()
    lst, root, _ = K.write_val_files(tmp_path / "train", rng, ((70, 90), (50, 80), (66, 65), (100, 60), (65, 65)))
    vlst, vroot, _ = K.write_val_files(tmp_path / "val", rng, SIZES)
    common = ["--stage", "f", "--list", lst, "--root", root, "--crop", "65", "--batch", "2", "--iters", "4", "--display", "1", "--workers", "2",
              "--seed", "3"]
    result = tmp_path / "val_result.txt"
    plain = _run("dsrg_amd.train", common + ["--prefix", str(tmp_path / "a" / "model-f")], timeout=600)
    assert not _val_lines(plain)
    out = _run("dsrg_amd.train", common + ["--prefix", str(tmp_path / "b" / "model-f"), "--val-list", vlst, "--val-root", vroot, "--val-every", "2",
                                           "--val-crop", "65", "--val-result", str(result)], timeout=600)
    lines = _val_lines(out)
    assert [(int(it), int(n)) for it, _, _, n in lines] == [(2, 5), (4, 5)], out[-2000:]
    assert all(0.0 <= float(v) <= 1.0 for _, miou, acc, _ in lines for v in (miou, acc))
    assert _done(out)[0] == 4 and _done(out) == _done(plain)            # the weights of the run without validation, bit for bit
    written = result.read_text().splitlines()
    assert written[0].startswith("meanIOU: ") and written[1].startswith("[") and len(written) >= 3
    assert "%.6f" % float(written[0].split()[1]) == lines[-1][1]

    # the snapshot of iteration 4, scored by the stand-alone command: the number the run reported last
    check = tmp_path / "check.txt"
    said = _run("dsrg_amd.validate", ["--model", str(tmp_path / "b" / "model-f_iter_4.caffemodel"), "--list", vlst, "--root", vroot, "--crop", "65",
                                      "--batch", "2", "--save_path", str(check)], timeout=600)
    assert check.read_text() == result.read_text()
    assert [ln for ln in said.splitlines() if ln.startswith("meanIOU: ")] == [written[0]]


def test_train_command_stage_s_with_validation_in_a_child_process(tmp_path):
    import pickle
    from PIL import Image
    rng = np.random.default_rng(54)
    d = tmp_path / "JPEGImages"
    d.mkdir()
    ids = [11, 14, 17]
    cues = {}
    for k, i in enumerate(ids):
        Image.fromarray(rng.integers(0, 256, (37 + 5 * k, 53 - 4 * k, 3), dtype=np.uint8)).save(str(d / ("im%d.png" % k)))
        cues['%i_labels' % i] = np.array(sorted(rng.choice(np.arange(1, 21), size=2, replace=False)))
        cues['%i_cues' % i] = np.stack([rng.integers(0, 21, 40), rng.integers(0, 41, 40), rng.integers(0, 41, 40)])
    (tmp_path / "input_list.txt").write_text("".join("im%d.png %d\n" % (k, i) for k, i in enumerate(ids)))
    with open(str(tmp_path / "cues.pickle"), "wb") as f:
        pickle.dump(cues, f, protocol=2)
    (tmp_path / "val").mkdir()
    vlst, vroot, _ = K.write_val_files(tmp_path / "val", rng, SIZES[:3])
    out = _run("dsrg_amd.train", ["--stage", "s", "--list", str(tmp_path / "input_list.txt"), "--root", str(d), "--cues", str(tmp_path / "cues.pickle"),
                                  "--iters", "2", "--batch", "2", "--display", "1", "--workers", "2", "--seed", "3", "--prefix",
                                  str(tmp_path / "m" / "model-s"), "--val-list", vlst, "--val-root", vroot, "--val-every", "1", "--val-crop", "65"],
               timeout=600)
    assert [(int(it), int(n)) for it, _, _, n in _val_lines(out)] == [(1, 3), (2, 3)], out[-2000:]
    assert _done(out)[0] == 2
