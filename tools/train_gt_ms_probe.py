#!/usr/bin/env python
"""The multi-scale, mirrored pseudo-label pass (--mode gt-ms), measured in one process.

  (a) the fused tail (ops.train_gt_ensemble_batch, want="unary") against the composition it replaces, at the workload's shapes (21
      labels, 375 x 500 images, the fc8 maps of the sizes 241 / 321 / 401), with and without flip, for 1 and 8 images: the
      composition is M calls of the one-map case (ops.train_gt_unary_batch, eps = 0, want="probs": the same kernels at K = 1; the
      mirror slices through torch.flip) plus the torch sum, divide, clamp and log per image.  Device-event medians, every shape warmed first, the two
      sides alternating; the spread is (max - min) / median over the rounds.  The two sides' outputs are compared first.
  (b) images/s of the pass with --smooth on seeded synthetic 375 x 500 images, VGG16-ASPP under bf16 autocast, graphed forwards,
      forward_batch 8, CRFs in flight: gt at 321 (predict_train_gt_many: predict_train_gt_ms_many at that one size), gt-ms at
      241,321,401 and the same with flip (predict_train_gt_ms_many); the three alternate, three windows each, host clock around a window that ends in a device
      synchronise.

usage: python tools/train_gt_ms_probe.py [a|b ...] [--out FILE]     (default: both; FILE: profiles/train_gt_ms_probe.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# as tools/flip_tta_probe.py: no online GEMM tuning, MIOpen's heuristic pick; every side of a comparison runs in this one process
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0")
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

H, W, C = 375, 500, 21
SIZES = (241, 321, 401)
MAPS = [(31, 31), (41, 41), (51, 51)]                                 # fc8 maps of 241 / 321 / 401
GROUP = 8
N_IMAGES = 64
IN_FLIGHT = 3
EPS = 1e-5
_LINES = []


def say(text):
    print(text, flush=True)
    _LINES.append(text)


def _timed(fn, reps=20, rounds=9, warmup=5):
    """-> (median, spread) in us over `rounds` of (device time of `reps` back-to-back calls) / reps; spread = (max - min) / median"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / reps)
    med = float(np.median(t))
    return med, (max(t) - min(t)) / med


def _images(n):
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(4242)
    out = []
    for k in range(n):
        img = S.make_images(rng, 1, size=max(H, W), kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        out.append(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8))
    return out


def probe_tail():
    from dsrg_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    res = []
    say("(a) maps %s -> %d x %d, %d labels, want=unary" % (MAPS, H, W, C))
    for flip in (False, True):
        per = 2 if flip else 1
        M = per * len(MAPS)
        for G in (1, GROUP):
            scores = [torch.randn(per * G, C, h, w, device="cuda", generator=g) * 3.0 for h, w in MAPS]
            shapes = [(H, W)] * G

            def fused():
                return ops.train_gt_ensemble_batch(scores, shapes, flip=flip, eps=EPS, want="unary")

            def composed():
                zs = []
                for s in scores:
                    zs.append(ops.train_gt_unary_batch(s[0::per].contiguous() if flip else s, shapes, eps=0.0, want="probs"))
                    if flip:
                        zs.append(ops.train_gt_unary_batch(torch.flip(s[1::per], [-1]), shapes, eps=0.0, want="probs"))
                out = []
                for i in range(G):
                    acc = zs[0][i]
                    for m in range(1, M):
                        acc = acc + zs[m][i]
                    out.append(torch.log(torch.clamp(acc / float(M), min=EPS)))
                return out

            diff = max(float((a - b).abs().max()) for a, b in zip(fused(), composed()))
            rows = {"fused": [], "composed": []}
            for _ in range(2):
                rows["fused"].append(_timed(fused))
                rows["composed"].append(_timed(composed))
            n, o = min(m for m, _ in rows["fused"]), min(m for m, _ in rows["composed"])
            spread = max(s for v in rows.values() for _, s in v)
            tag = "flip %-5s %d image(s), %d maps" % (flip, G, M)
            say("%-32s fused %s us | %d kernel calls + torch %s us | ratio of the lower medians %.2f (largest spread within a side "
                "%.1f %%); largest |unary difference| %.3g" % (tag, ["%.1f" % m for m, _ in rows["fused"]], M,
                                                                ["%.1f" % m for m, _ in rows["composed"]], o / n, 100.0 * spread, diff))
            res.append(dict(flip=flip, images=G, maps=M, fused_us=[round(m, 1) for m, _ in rows["fused"]],
                            composed_us=[round(m, 1) for m, _ in rows["composed"]], composed_over_fused=round(o / n, 2),
                            spread=round(spread, 3), max_abs_unary_diff=diff))
    return res


def probe_throughput():
    from dsrg_amd import inference as I
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(0)
    net = VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()
    ims = _images(4)
    rng = np.random.default_rng(7)
    labels = [[int(c) for c in rng.choice(np.arange(1, C), size=1 + k % 3, replace=False)] for k in range(len(ims))]
    fwd = I.GraphedForward(net)

    def run(mode, n):
        items = [(ims[i % len(ims)], labels[i % len(ims)]) for i in range(n)]
        if mode == "gt":
            gen = I.predict_train_gt_many(net, items, size=321, forward=fwd, in_flight=IN_FLIGHT, forward_batch=GROUP)
        else:
            gen = I.predict_train_gt_ms_many(net, items, sizes=SIZES, flip=mode == "gt-ms flip", forward=fwd, in_flight=IN_FLIGHT,
                                             forward_batch=GROUP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in gen)
        torch.cuda.synchronize()
        assert k == n
        return n / (time.perf_counter() - t0)

    modes = ("gt", "gt-ms", "gt-ms flip")
    say("(b) images/s, VGG16-ASPP bf16, %d x %d, --smooth, forward_batch %d, in_flight %d, %d images per window"
        % (H, W, GROUP, IN_FLIGHT, N_IMAGES))
    rates = {m: [] for m in modes}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for m in modes:                                               # every graph, CRF object and kernel of this setting
            run(m, 3 * GROUP)
        for _ in range(3):
            for m in modes:
                rates[m].append(round(run(m, N_IMAGES), 1))
    base = float(np.median(rates["gt"]))
    for m in modes:
        say("%-11s %s images/s (median %.1f, x%.2f the time per image of gt)" % (m, rates[m], np.median(rates[m]),
                                                                                base / float(np.median(rates[m]))))
    return dict(images_per_s=rates)


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "train_gt_ms_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    which = argv or ["a", "b"]
    from dsrg_amd import _lib
    _lib.require_gpu()
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    say("tools/train_gt_ms_probe.py %s on %s" % (" ".join(which), torch.cuda.get_device_name(0)))
    out = {"device": torch.cuda.get_device_name(0)}
    if "a" in which:
        out["tail"] = probe_tail()
    if "b" in which:
        out["throughput"] = probe_throughput()
    say(json.dumps(out))
    with open(out_path, "w") as f:
        f.write("\n".join(_LINES) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
