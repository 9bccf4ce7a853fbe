#!/usr/bin/env python
"""The multi-scale-input step with max fusion (dsrg_amd/csrc/msc.hip, ops.msc_loss / ops.msc_pyramid) measured in one process.

  (a) the fused loss call (S + 1 losses, S gradients and counters: three launches) against the float32 torch composition it stands
      for, forward and backward: F.interpolate(bilinear, align_corners=True) -> stack().max(0) -> four F.cross_entropy(ignore_index=
      255), summed -> backward to the three maps.  Shapes (B, C, maps, H): (10, 21, 41 / 31 / 21, 321), (10, 21, 65 / 49 / 33, 513).
      Labels: blocks of classes with 5 % of the pixels 255; the composition's four integer target maps (label.long() and the
      nearest-sample gathers) are computed once OUTSIDE the timed call, the fused call samples the labels inside.  The two alternate round by round; device-event medians over rounds of
      back-to-back calls, and the spread (min .. max over the rounds).  Their losses and gradients are compared first.
  (b) the pyramid launch against F.interpolate per scale + the copy into channels-last, (10, 3, 321) -> 241, 161 and 513 -> 385, 257.
  (c) one train-f step (RetrainTrainer.step, bf16, resident tensors) with msc_scales=(0.75, 0.5) against the single-scale step,
      VGG16-ASPP at batch 10, crop 321 and ResNet-101 at batch 10, crop 321; the trainers alternate round by round, device events
      around rounds of steps.  Reported: the ratio (the forwards' arithmetic alone is 1 + 0.5625 + 0.25 = 1.81).

usage: python tools/msc_probe.py [a b c-vgg16 c-resnet101 ...]      (default: all; one JSON line at the end)
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

SHAPES = ((10, 21, (41, 31, 21), 321), (10, 21, (65, 49, 33), 513))
SCALES = (0.75, 0.5)


def _tensors(B, C, sides, H, seed=91):
    rng = np.random.default_rng(seed)
    maps = [torch.from_numpy((rng.standard_normal((B, C, h, h)) * 3).astype(np.float32)).cuda() for h in sides]
    lab = rng.integers(0, C, (B, 1, (H + 24) // 25, (H + 24) // 25)).repeat(25, 2).repeat(25, 3)[:, :, :H, :H].astype(np.float32)
    lab[rng.random(lab.shape) < 0.05] = 255.0
    return maps, torch.from_numpy(lab).cuda()


def _nearest_index(n, N, device):
    i = torch.arange(n, device=device)
    return (2 * i * (N - 1) + (n - 1)) // (2 * (n - 1)) if n > 1 else torch.zeros(1, dtype=torch.long, device=device)


def torch_targets(maps, label):
    """the S + 1 integer target maps of the torch composition (fused first): the label sampling, which a careful torch user
    computes once per batch — it is NOT part of what probe (a) times, although the fused call does it inside"""
    H, W = label.shape[-2:]
    lab = label.reshape(label.shape[0], H, W).long()
    sizes = [maps[0].shape[-2:]] + [m.shape[-2:] for m in maps]
    return [lab[:, _nearest_index(h, H, lab.device)][:, :, _nearest_index(w, W, lab.device)].contiguous() for h, w in sizes]


def torch_composition(maps, targets):
    """the float32 torch composition -> the S + 1 losses (fused first), differentiable"""
    h0, w0 = maps[0].shape[-2:]
    fused = torch.stack([maps[0]] + [F.interpolate(m, size=(h0, w0), mode="bilinear", align_corners=True) for m in maps[1:]]).max(0).values
    return torch.stack([F.cross_entropy(z, t, ignore_index=255, reduction="mean") for z, t in zip([fused] + list(maps), targets)])


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
    for B, C, sides, H in SHAPES:
        maps, label = _tensors(B, C, sides, H)
        counters = torch.zeros(3, dtype=torch.int64, device="cuda")
        targets = torch_targets(maps, label)

        def fused():
            return ops.msc_loss(maps, label, counters=counters)

        def composed():
            xs = [m.detach().requires_grad_(True) for m in maps]
            losses = torch_composition(xs, targets)
            losses.sum().backward()
            return losses.detach(), [x.grad for x in xs]

        (lf, gf, _), (lc, gc) = fused(), composed()
        dl = (lf - lc).abs().max().item()
        dg = max((a - b).abs().max().item() / b.abs().max().item() for a, b in zip(gf, gc))
        tf, tc = _rounds([fused, composed], reps=20)
        print("(a) B %d, C %d, maps %s, labels %d: losses %s (fused) %s (torch), max|difference| %.2e; max|grad difference| / max|grad| %.2e"
              % (B, C, "/".join(str(s) for s in sides), H, " ".join("%.6f" % v for v in lf.tolist()),
                 " ".join("%.6f" % v for v in lc.tolist()), dl, dg), flush=True)
        _say("    fused call:        ", tf)
        _say("    torch composition: ", tc)
        print("    torch / fused = %.2f" % (float(np.median(tc)) / float(np.median(tf))), flush=True)
        res.append(dict(shape=[B, C, list(sides), H], fused_us=round(float(np.median(tf)), 1), torch_us=round(float(np.median(tc)), 1),
                        fused_rounds_us=[round(t, 1) for t in tf], torch_rounds_us=[round(t, 1) for t in tc],
                        loss_difference=dl, grad_relative_difference=dg))
    return res


def probe_b(B=10):
    from dsrg_amd import ops
    from dsrg_amd.retrain import msc_sizes
    res = []
    g = torch.Generator().manual_seed(5)
    for crop in (321, 513):
        images = (torch.rand(B, 3, crop, crop, generator=g) * 255 - 115).cuda()
        sides = msc_sizes(crop, SCALES)

        def fused():
            return ops.msc_pyramid(images, sides)

        def composed():
            return [F.interpolate(images, size=(s, s), mode="bilinear", align_corners=True).contiguous(memory_format=torch.channels_last)
                    for s in sides]

        diff = max((a - b).abs().max().item() for a, b in zip(fused(), composed()))
        tf, tc = _rounds([fused, composed], reps=20)
        print("(b) B %d, %d -> %s: max|difference| %.2e" % (B, crop, ", ".join(str(s) for s in sides), diff), flush=True)
        _say("    pyramid launch:                 ", tf)
        _say("    F.interpolate + layout copies:  ", tc)
        res.append(dict(crop=crop, fused_us=round(float(np.median(tf)), 1), torch_us=round(float(np.median(tc)), 1),
                        fused_rounds_us=[round(t, 1) for t in tf], torch_rounds_us=[round(t, 1) for t in tc], difference=diff))
    return res


def probe_c(backbone, B=10, C=21, crop=321):
    from dsrg_amd.retrain import RetrainTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(B, 3, crop, crop, generator=g) * 255 - 115).cuda()
    label = torch.randint(0, C, (B, 1, crop, crop), generator=g).float().cuda()
    t_one = RetrainTrainer(dev, backbone=backbone, seed=0)
    t_msc = RetrainTrainer(dev, backbone=backbone, seed=0, msc_scales=SCALES)
    fns = [lambda: t_one.step(images, label), lambda: t_msc.step(images, label)]
    to, tm = ([t / 1000.0 for t in ts] for ts in _rounds(fns, reps=3, rounds=7, warmup=3))
    print("(c) one train-f step, %s, bf16, batch %d, crop %d" % (backbone, B, crop), flush=True)
    _say("    single scale:            ", to, "ms")
    _say("    msc_scales=(0.75, 0.5):  ", tm, "ms")
    mo, mm = float(np.median(to)), float(np.median(tm))
    print("    msc / single = %.2f" % (mm / mo), flush=True)
    return dict(backbone=backbone, batch=B, crop=crop, single_ms=round(mo, 3), msc_ms=round(mm, 3), ratio=round(mm / mo, 3),
                single_rounds_ms=[round(t, 3) for t in to], msc_rounds_ms=[round(t, 3) for t in tm])


def main(argv):
    from dsrg_amd import _lib
    _lib.require_gpu()
    modes = argv or ["a", "b", "c-vgg16", "c-resnet101"]
    out = {}
    if "a" in modes:
        out["a"] = probe_a()
    if "b" in modes:
        out["b"] = probe_b()
    for m in modes:
        if m.startswith("c-"):
            out[m] = probe_c(m[2:])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
