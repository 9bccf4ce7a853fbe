#!/usr/bin/env python
"""Validation scoring (dsrg_amd/validate.py, csrc/eval.hip) measured in one process, at the workload's shape: 10 images, 21 labels,
65 x 65 score maps, crop 513, images of 375 x 500 and 500 x 375 at the top left of the crop (labels 255 off them).

  (a) the fused launch alone: ops.eval_confusion_batch (dsrg_eval_confusion_batch).
  (b) the composition it replaces, on the same tensors: ops.multiscale_unary_batch with the argmax output only (ten 513 x 513 int32
      maps), the casts of labels and argmax to uint8, ops.confusion_matrix.
      (a) and (b) alternate; device-event medians over rounds of back-to-back calls (each call builds its arguments on the host, so
      these bound the kernels' time from above); their counters are compared first.
  (c) a whole Validator.run() over a generated list of JPEG / PNG files (VGG16-ASPP, bf16, batch 10, 8 decoding threads), host clock
      around the call (it ends in a device synchronise), in images/s; next to it the time of one train-f step (RetrainTrainer.step,
      VGG16-ASPP, bf16) at batch 10 on resident tensors at train-f's crop 321 and at crop 513.

  (k) the fused launch and the composition alone, 200 times each, for `rocprofv3 --kernel-trace --stats` in a run of its own
      (tools/rocpd_stats.py summarises its database): the kernels' own time.

usage: python tools/validate_probe.py [a c k ...]      (default: a c; (a) includes (b); one JSON line at the end)
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

B, C, HS, CROP = 10, 21, 65, 513
SIZES = ((375, 500), (500, 375))
N_FILES = 40


def _tensors():
    rng = np.random.default_rng(91)
    scores = rng.standard_normal((B, C, HS, HS)).astype(np.float32) * 4
    labels = np.full((B, 1, CROP, CROP), 255.0, dtype=np.float32)
    for b in range(B):
        H, W = SIZES[b % 2]
        lab = rng.integers(0, C, ((H + 24) // 25, (W + 24) // 25)).repeat(25, 0).repeat(25, 1)[:H, :W].astype(np.float32)
        lab[rng.random((H, W)) < 0.05] = 255.0                          # VOC's object borders
        labels[b, 0, :H, :W] = lab
    return torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()


def _rounds(fns, reps=20, rounds=9, warmup=5):
    """-> per function the list of per-call microseconds of each round; the functions alternate round by round"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1000.0 / reps)
    return out


def _sides():
    """-> (fused, composed, hist): the two ways from scores and labels to counters, adding into hist"""
    from dsrg_amd import ops
    scores, labels = _tensors()
    hist = torch.zeros(C * C + 1, dtype=torch.int64, device="cuda")
    shapes = [(CROP, CROP)] * B

    def fused():
        return ops.eval_confusion_batch(scores, labels, C, hist=hist)

    def composed():
        amax = ops.multiscale_unary_batch([scores], shapes, want="argmax")
        pred = torch.stack(amax).to(torch.uint8)
        return ops.confusion_matrix(labels.to(torch.uint8).reshape(-1), pred.reshape(-1), C, hist=hist)

    return fused, composed, hist


def probe_k(n=200):
    fused, composed, _ = _sides()
    for fn in (fused, composed):
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    print("(k) %d fused launches, %d compositions" % (n, n), flush=True)
    return dict(launches=n)


def probe_a():
    fused, composed, hist = _sides()
    hist.zero_()
    ha = fused().clone()
    hist.zero_()
    hb = composed().clone()
    same = bool(torch.equal(ha, hb))
    kept = int(ha.sum())
    ta, tb = _rounds([fused, composed])
    ma, mb = float(np.median(ta)), float(np.median(tb))
    print("(a) fused launch:  median %.1f us per batch of %d (rounds: %s)" % (ma, B, " ".join("%.1f" % t for t in ta)), flush=True)
    print("(b) composition:   median %.1f us per batch of %d (rounds: %s)" % (mb, B, " ".join("%.1f" % t for t in tb)), flush=True)
    print("    counters equal: %s; %d of %d pixels kept; (b) / (a) = %.2f" % (same, kept, B * CROP * CROP, mb / ma), flush=True)
    return dict(fused_us=round(ma, 1), composed_us=round(mb, 1), ratio=round(mb / ma, 2), counters_equal=same, kept_pixels=kept,
                fused_rounds_us=[round(t, 1) for t in ta], composed_rounds_us=[round(t, 1) for t in tb])


def _files(d):
    from PIL import Image
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(92)
    lines = []
    for k in range(N_FILES):
        H, W = SIZES[k % 2]
        img = S.make_images(rng, 1, size=500, kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8)).save(
            os.path.join(d, "im%d.jpg" % k), quality=92)
        Image.fromarray(rng.integers(0, C, (H // 25, W // 25), dtype=np.uint8).repeat(25, 0).repeat(25, 1), mode="L").save(
            os.path.join(d, "lab%d.png" % k))
        lines.append("/im%d.jpg /lab%d.png\n" % (k, k))
    with open(os.path.join(d, "val.txt"), "w") as f:
        f.write("".join(lines))
    return os.path.join(d, "val.txt"), d


def _step_ms(trainer, crop, steps=10, warmup=3):
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(B, 3, crop, crop, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (B, 1, crop, crop), generator=g).float().cuda()
    for _ in range(warmup):
        trainer.step(images, label)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(images, label)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / steps


def probe_c():
    from dsrg_amd.retrain import RetrainTrainer
    from dsrg_amd.validate import Validator
    trainer = RetrainTrainer(torch.device("cuda", torch.cuda.current_device()), backbone="vgg16", seed=0)
    with tempfile.TemporaryDirectory() as d:
        lst, root = _files(d)
        val = Validator(trainer.net, lst, root, crop=CROP, batch=B, num_classes=C, amp_dtype=trainer.amp_dtype)
        val.run()                                                       # warm-up: the forward's shapes, the decoders
        rates = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = val.run()
            rates.append(res["images"] / (time.perf_counter() - t0))
    step321, step513 = _step_ms(trainer, 321), _step_ms(trainer, 513)
    print("(c) Validator.run over %d files at batch %d, crop %d: %s images/s" % (N_FILES, B, CROP, " ".join("%.1f" % r for r in rates)),
          flush=True)
    print("    one train-f step at batch %d: %.1f ms at crop 321, %.1f ms at crop 513" % (B, step321, step513), flush=True)
    return dict(validator_images_per_s=[round(r, 1) for r in rates], files=N_FILES, train_f_step_ms_crop321=round(step321, 1),
                train_f_step_ms_crop513=round(step513, 1))


def main(argv):
    from dsrg_amd import _lib
    _lib.require_gpu()
    modes = argv or ["a", "c"]
    out = {}
    if "a" in modes:
        out["a"] = probe_a()
    if "c" in modes:
        out["c"] = probe_c()
    if "k" in modes:
        out["k"] = probe_k()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
