"""Stage 2 with the loss at label resolution: RetrainTrainer(loss_at="label") and `python -m dsrg_amd.train --stage f --loss-at label`
on the GPU.  Crop 65, batches of 2 images, the VGG backbone, tiny synthetic files.  Losses and gradients are compared as bit
patterns, weights as the integer checksums of trainer.params_checksum."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_confusion_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP, C = 65, 21

pytestmark = pytest.mark.gpu


def _batch():
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(2, 3, CROP, CROP, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (2, 1, CROP, CROP), generator=g).float()
    label[0, 0, 10:30, 5:40] = 255.0
    return images, label.cuda()


def _trainer(**kw):
    from dsrg_amd.retrain import RetrainTrainer
    return RetrainTrainer(torch.device("cuda", torch.cuda.current_device()), backbone="vgg16", max_iter=10, seed=3, **kw)


def _checksum(tr):
    from dsrg_amd.trainer import params_checksum
    words = params_checksum(list(tr.net.parameters()) + [b for grp in tr.opt.groups for b in grp["bufs"]])
    return [int(v) for v in words.cpu()]


def test_step_returns_the_op_on_the_logits_the_forward_produced():
    from dsrg_amd import ops
    images, label = _batch()
    tr = _trainer(loss_at="label")
    assert tr.loss_counters.tolist() == [0, 0, 0]
    seen = []
    hook = tr.net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().contiguous().clone()))
    try:
        loss = tr.step(images, label)
    finally:
        hook.remove()
    assert len(seen) == 1 and tuple(seen[0].shape) == (2, C, 9, 9)
    want, _, cnt = ops.seg_loss_zoom(seen[0], label)
    assert torch.equal(loss.view(torch.int32), want.view(torch.int32))
    assert tr.loss_counters.tolist() == cnt.tolist() and cnt[0].item() == int((label != 255).sum()) and cnt[2].item() == 0
    tr.step(images, label)
    assert tr.loss_counters[0].item() == 2 * cnt[0].item()                      # the counters run on over the steps
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


def test_checksums_after_two_steps():
    images, label = _batch()

    def two_steps(**kw):
        tr = _trainer(**kw)
        losses = [tr.step(images, label).item(), tr.step(images, label).item()]
        assert all(np.isfinite(losses))
        return _checksum(tr)

    at_label = two_steps(loss_at="label")
    assert two_steps(loss_at="label") == at_label                               # same seed, same weights: no atomics on the way
    at_map = two_steps(loss_at="map")
    assert two_steps() == at_map                                                # the default is the map
    assert at_label != at_map
    assert _trainer().loss_counters is None


def _run(args, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout.decode(errors="replace")


_LINE = re.compile(r"^Iteration (\d+), lr = \S+, loss = ([-+.\dnaife]+)(?:, accuracy = ([-+.\dnaife]+))?$")


def test_the_command_in_a_child_process(tmp_path):
    rng = np.random.default_rng(61)
    lst, root, _ = K.write_val_files(tmp_path, rng, ((70, 90), (50, 80), (66, 65), (100, 60)))
    common = ["--stage", "f", "--list", lst, "--root", root, "--crop", "65", "--batch", "2", "--iters", "2", "--display", "1", "--workers", "2",
              "--seed", "3"]
    out = _run(common + ["--prefix", str(tmp_path / "a" / "model-f"), "--loss-at", "label"], timeout=600)
    lines = [m.groups() for m in (_LINE.match(ln) for ln in out.splitlines()) if m]
    assert [int(it) for it, _, _ in lines] == [1, 2], out[-2000:]
    assert all(acc is not None and 0.0 <= float(acc) <= 1.0 and np.isfinite(float(loss)) for _, loss, acc in lines), out[-2000:]
    assert any(ln.startswith("done: iteration 2 ") for ln in out.splitlines())
    assert "warning" not in out                                                 # the files hold classes and 255 only
    plain = _run(common + ["--prefix", str(tmp_path / "b" / "model-f")], timeout=600)
    assert "accuracy" not in plain and any(ln.startswith("done: iteration 2 ") for ln in plain.splitlines())
    assert [int(m.group(1)) for m in (_LINE.match(ln) for ln in plain.splitlines()) if m] == [1, 2]
