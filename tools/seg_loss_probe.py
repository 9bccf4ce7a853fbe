#!/usr/bin/env python
"""The softmax loss at label resolution (dsrg_amd/csrc/seg_loss.hip, ops.seg_loss_zoom) measured in one process.

  (a) the fused call (loss, gradient and counters: two launches) against the float32 torch composition it stands for, forward and
      backward: F.interpolate(bilinear, align_corners=True) -> F.cross_entropy(ignore_index=255) -> backward to the logits.
      Shapes (B, C, h -> H): (10, 21, 41 -> 321), (10, 21, 65 -> 513), (10, 81, 41 -> 321).  Labels: blocks of classes with 5 %
      of the pixels 255.  The two alternate round by round; device-event medians over rounds of back-to-back calls, and the spread
      (min .. max over the rounds).  Their losses and gradients are compared first.
  (b) one train-f step (RetrainTrainer.step, VGG16-ASPP, bf16, batch 10, crop 321, resident tensors) with loss_at="map", with
      loss_at="label", and with "label" computed by that torch composition; the three trainers alternate round by round, device
      events around rounds of steps.  Reported: what "label" costs over "map" as a share of the step.

usage: python tools/seg_loss_probe.py [a b ...]      (default: a b; one JSON line at the end)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = ((10, 21, 41, 321), (10, 21, 65, 513), (10, 81, 41, 321))


def _tensors(B, C, h, H, seed=91):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C, h, h)) * 3).astype(np.float32)
    lab = rng.integers(0, C, (B, 1, (H + 24) // 25, (H + 24) // 25)).repeat(25, 2).repeat(25, 3)[:, :, :H, :H].astype(np.float32)
    lab[rng.random(lab.shape) < 0.05] = 255.0
    return torch.from_numpy(logits).cuda(), torch.from_numpy(lab).cuda()


def torch_composition(logits, label):
    """the float32 torch composition as a differentiable scalar"""
    z = F.interpolate(logits.float(), size=label.shape[-2:], mode="bilinear", align_corners=True)
    return F.cross_entropy(z, label.reshape(label.shape[0], *label.shape[-2:]).long(), ignore_index=255, reduction="mean")


def _rounds(fns, reps, rounds=9, warmup=3):
    """-> per function the per-call microseconds of each round; the functions alternate round by round"""
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


def _say(tag, ts, unit="us"):
    print("%s median %.1f %s (min %.1f, max %.1f over %d rounds)" % (tag, float(np.median(ts)), unit, min(ts), max(ts), len(ts)), flush=True)


def probe_a():
    from dsrg_amd import ops
    res = []
    for B, C, h, H in SHAPES:
        logits, label = _tensors(B, C, h, H)
        counters = torch.zeros(3, dtype=torch.int64, device="cuda")

        def fused():
            return ops.seg_loss_zoom(logits, label, counters=counters)

        def composed():
            x = logits.detach().requires_grad_(True)
            loss = torch_composition(x, label)
            loss.backward()
            return loss.detach(), x.grad

        (lf, gf, _), (lc, gc) = fused(), composed()
        dl = abs(lf.item() - lc.item())
        dg = (gf - gc).abs().max().item() / gc.abs().max().item()
        tf, tc = _rounds([fused, composed], reps=20)
        print("(a) B %d, C %d, %d -> %d: loss %.6f (fused) %.6f (torch), |difference| %.2e; max|grad difference| / max|grad| %.2e"
              % (B, C, h, H, lf.item(), lc.item(), dl, dg), flush=True)
        _say("    fused call:        ", tf)
        _say("    torch composition: ", tc)
        print("    torch / fused = %.2f" % (float(np.median(tc)) / float(np.median(tf))), flush=True)
        res.append(dict(shape=[B, C, h, H], fused_us=round(float(np.median(tf)), 1), torch_us=round(float(np.median(tc)), 1),
                        fused_rounds_us=[round(t, 1) for t in tf], torch_rounds_us=[round(t, 1) for t in tc],
                        loss_difference=dl, grad_relative_difference=dg))
    return res


def probe_b(B=10, C=21, crop=321):
    from dsrg_amd import retrain
    from dsrg_amd.retrain import RetrainTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(B, 3, crop, crop, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (B, 1, crop, crop), generator=g).float().cuda()
    t_map = RetrainTrainer(dev, backbone="vgg16", seed=0, loss_at="map")
    t_label = RetrainTrainer(dev, backbone="vgg16", seed=0, loss_at="label")
    t_torch = RetrainTrainer(dev, backbone="vgg16", seed=0, loss_at="label")
    fused_loss = retrain.seg_softmax_loss_zoom

    def step_torch():
        retrain.seg_softmax_loss_zoom = lambda logits, lab, counters=None: torch_composition(logits, lab)
        try:
            return t_torch.step(images, label)
        finally:
            retrain.seg_softmax_loss_zoom = fused_loss

    fns = [lambda: t_map.step(images, label), lambda: t_label.step(images, label), step_torch]
    tm, tl, tt = ([t / 1000.0 for t in ts] for ts in _rounds(fns, reps=5, rounds=9, warmup=4))
    print("(b) one train-f step, VGG16-ASPP, bf16, batch %d, crop %d" % (B, crop), flush=True)
    _say("    loss_at=map:                    ", tm, "ms")
    _say("    loss_at=label (fused):          ", tl, "ms")
    _say("    loss_at=label (torch composed): ", tt, "ms")
    mm, ml, mt = (float(np.median(t)) for t in (tm, tl, tt))
    print("    label over map: %+.3f ms = %+.2f %% of the step (fused); %+.3f ms = %+.2f %% (torch composed)"
          % (ml - mm, 100.0 * (ml - mm) / mm, mt - mm, 100.0 * (mt - mm) / mm), flush=True)
    return dict(map_ms=round(mm, 3), label_ms=round(ml, 3), label_torch_ms=round(mt, 3), map_rounds_ms=[round(t, 3) for t in tm],
                label_rounds_ms=[round(t, 3) for t in tl], label_torch_rounds_ms=[round(t, 3) for t in tt],
                label_over_map_percent=round(100.0 * (ml - mm) / mm, 2))


def main(argv):
    from dsrg_amd import _lib
    _lib.require_gpu()
    modes = argv or ["a", "b"]
    out = {}
    if "a" in modes:
        out["a"] = probe_a()
    if "b" in modes:
        out["b"] = probe_b()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
