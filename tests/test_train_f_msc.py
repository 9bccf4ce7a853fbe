"""Stage 2 with multi-scale inputs and max fusion: RetrainTrainer(msc_scales=(0.75, 0.5)) and `python -m dsrg_amd.train --stage f
--msc-scales 0.75,0.5` on the GPU.  Crop 65 (inputs of 65, 49 and 33 pixels: score maps of 9, 7 and 5 cells), batches of 2 images,
tiny synthetic files.  Losses are compared as bit patterns, weights as the integer checksums of trainer.params_checksum."""
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
SCALES = (0.75, 0.5)

pytestmark = pytest.mark.gpu


def _batch():
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(2, 3, CROP, CROP, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (2, 1, CROP, CROP), generator=g).float()
    label[0, 0, 10:30, 5:40] = 255.0
    return images, label.cuda()


def _trainer(**kw):
    from dsrg_amd.retrain import RetrainTrainer
    kw.setdefault("backbone", "vgg16")
    return RetrainTrainer(torch.device("cuda", torch.cuda.current_device()), max_iter=10, seed=3, **kw)


def _checksum(tr):
    from dsrg_amd.trainer import params_checksum
    words = params_checksum(list(tr.net.parameters()) + [b for grp in tr.opt.groups for b in grp["bufs"]])
    return [int(v) for v in words.cpu()]


def test_step_returns_the_op_on_the_maps_the_three_forwards_produced():
    from dsrg_amd import ops
    images, label = _batch()
    tr = _trainer(msc_scales=SCALES)
    assert tr.loss_counters.tolist() == [0, 0, 0]
    seen = []
    hook = tr.net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().contiguous().clone()))
    try:
        got = tr.step(images, label)
    finally:
        hook.remove()
    assert [tuple(m.shape) for m in seen] == [(2, C, 9, 9), (2, C, 7, 7), (2, C, 5, 5)]
    want, _, cnt = ops.msc_loss(seen, label)
    assert tuple(got.shape) == (5,) and torch.equal(got[1:].view(torch.int32), want.view(torch.int32))      # fused, res1, res0.75, res0.5
    assert torch.equal(got[0].view(torch.int32), want.sum().view(torch.int32))                               # the total
    assert tr.loss_counters.tolist() == cnt.tolist() and cnt[0].item() == int((label[:, :, ::8, ::8] != 255).sum()) and cnt[2].item() == 0
    tr.step(images, label)
    assert tr.loss_counters[0].item() == 2 * cnt[0].item()                      # the counters run on over the steps
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


def test_checksums_after_two_steps():
    images, label = _batch()

    def two_steps(**kw):
        tr = _trainer(**kw)
        losses = [tr.step(images, label), tr.step(images, label)]
        assert all(torch.isfinite(l).all() for l in losses)
        return _checksum(tr), tr

    msc, _ = two_steps(msc_scales=SCALES)
    assert two_steps(msc_scales=SCALES)[0] == msc                               # same seed, same weights: no atomics on the way
    plain, tr = two_steps()
    assert tr.loss_counters is None and tr.msc_scales == ()
    assert two_steps(msc_scales=())[0] == plain                                 # the default is the single-scale step
    assert msc != plain
    # behind the bucketed reducer (world size 1): the same weights; no slot is handed out, every large gradient is copied after backward
    ddp, tr = two_steps(msc_scales=SCALES, ddp=True)
    assert ddp == msc
    assert tr.reducer.copies > 0 and all(getattr(p, "_dsrg_grad_out", None) is None for p in tr.net.parameters())
    plain_ddp, tr = two_steps(ddp=True)
    assert plain_ddp == plain and any(getattr(p, "_dsrg_grad_out", None) is not None for p in tr.net.parameters())


def test_one_backward_accumulates_the_three_contributions():
    """Per parameter, the gradient of the ONE multi-scale backward against the float64 host sum of three separate backwards, each fed
    only the op's grad_s.  A small ResNet without Dropout (blocks 1, 1, 1, 1) in float32.  Bound, element-wise: max(4 D, 4 * 2^-24 *
    sum_s |g_s|), D = the largest run-to-run distance of one single-scale backward on the same input over the parameter's elements
    (three contributions, each repeatable only to within D; two float32 additions, each within 2^-24 of a partial sum that is at
    most sum_s |g_s|; the factor 4 leaves a margin of 4/3 and 2).  Measured on an MI355X: the run-to-run distance of the single-scale
    backward is 0 for every parameter (D = 0.000e+00: the backward is repeatable to the bit, so the float32 term alone bounds), and
    the largest error is 0.488 of its bound."""
    from dsrg_amd import ops
    from dsrg_amd.retrain import ResNet101DeepLab, msc_sizes
    torch.manual_seed(11)
    net = ResNet101DeepLab(num_classes=C, blocks=(1, 1, 1, 1))
    tr = _trainer(backbone="resnet101", net=net, amp_dtype=None, msc_scales=SCALES)
    tr.opt.step = lambda: None                                                  # the gradients are what is looked at: no update
    images, label = _batch()
    params = [p for p in tr.net.parameters() if p.requires_grad]
    sides = msc_sizes(CROP, SCALES)
    xs = [images.contiguous(memory_format=torch.channels_last)] + ops.msc_pyramid(images, [(s, s) for s in sides])

    def backward_of(s, grad):
        for p in params:
            p.grad = None
        tr.net(xs[s]).backward(grad)
        return [p.grad.detach().double().cpu() if p.grad is not None else None for p in params]

    with torch.no_grad():
        maps = [tr.net(x).float().contiguous() for x in xs]
    _, grads, _ = ops.msc_loss(maps, label)
    parts = [backward_of(s, grads[s]) for s in range(3)]
    again = backward_of(0, grads[0])
    tr.step(images, label)
    worst_d = worst = 0.0
    for k, p in enumerate(params):
        if parts[0][k] is None:
            assert p.grad is None
            continue
        want = sum(part[k] for part in parts)
        mass = sum(part[k].abs() for part in parts)
        d = float((again[k] - parts[0][k]).abs().max())
        bound = torch.clamp(4.0 * 2.0 ** -24 * mass, min=4.0 * d)
        err = (p.grad.detach().double().cpu() - want).abs()
        worst_d, worst = max(worst_d, d), max(worst, float((err / bound.clamp(min=1e-300)).max()) if float(err.max()) > 0 else 0.0)
        assert bool((err <= bound).all()), (k, tuple(p.shape), float(err.max()), d)
    print("msc accumulation: largest run-to-run distance of a single-scale backward %.3e, largest error / bound %.3f" % (worst_d, worst))


def _run(args, ok=True, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "dsrg_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert (r.returncode == 0) == ok, r.stdout.decode(errors="replace")[-3000:]
    return r.returncode, r.stdout.decode(errors="replace")


_NUM = r"([-+.\dnaife]+)"
_MSC = re.compile(r"^Iteration (\d+), lr = \S+, loss = %s, loss-fusion = %s, loss-res1 = %s, loss-res0\.75 = %s, loss-res0\.5 = %s, accuracy = %s$"
                  % ((_NUM,) * 6))
_PLAIN = re.compile(r"^Iteration (\d+), lr = \S+, loss = %s$" % _NUM)


def test_the_command_in_a_child_process(tmp_path):
    rng = np.random.default_rng(61)
    lst, root, _ = K.write_val_files(tmp_path, rng, ((70, 90), (50, 80), (66, 65), (100, 60)))
    common = ["--stage", "f", "--list", lst, "--root", root, "--crop", "65", "--batch", "2", "--iters", "2", "--display", "1", "--workers", "2",
              "--seed", "3"]
    _, out = _run(common + ["--prefix", str(tmp_path / "a" / "model-f"), "--msc-scales", "0.75,0.5"], timeout=600)
    lines = [tuple(float(v) for v in m.groups()) for m in (_MSC.match(ln) for ln in out.splitlines()) if m]
    assert [int(ln[0]) for ln in lines] == [1, 2], out[-2000:]
    for _, total, fused, r1, r075, r05, acc in lines:
        assert all(np.isfinite(v) and v > 0 for v in (fused, r1, r075, r05)) and 0.0 <= acc <= 1.0, out[-2000:]
        assert abs(total - (fused + r1 + r075 + r05)) < 1e-4
    assert any(ln.startswith("done: iteration 2 ") for ln in out.splitlines()) and "warning" not in out
    _, plain = _run(common + ["--prefix", str(tmp_path / "b" / "model-f")], timeout=600)
    assert "accuracy" not in plain and "fusion" not in plain and any(ln.startswith("done: iteration 2 ") for ln in plain.splitlines())
    assert [int(m.group(1)) for m in (_PLAIN.match(ln) for ln in plain.splitlines()) if m] == [1, 2]        # the old line, unchanged
    rc, refused = _run(common + ["--prefix", str(tmp_path / "c" / "model-f"), "--msc-scales", "0.75,0.5", "--loss-at", "label"], ok=False,
                       timeout=600)
    assert rc == 2 and "usage:" in refused and "do not combine" in refused
