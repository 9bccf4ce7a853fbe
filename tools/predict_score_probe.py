#!/usr/bin/env python
"""The scored multi-scale test (`python -m dsrg_amd.predict --gt`) against the route it replaces, measured in one process on synthetic
images of VOC size (375 x 500, 500 x 375, 333 x 500) with a randomly initialised VGG16-ASPP and random ground truth.

  (a) the parent's route: `predict ... --output OUT` (every label map down as int32, a PNG per image) followed by
      `evaluate --pred OUT --gt GT` (every PNG read back, counted on the CPU);
  (b) `predict ... --gt GT --output OUT`: scored on the GPU, the PNGs written from the scorer's uint8 masks;
  (c) `predict ... --gt GT`: scored on the GPU, nothing but the ground truth goes up and the counters come down.

The three are the commands' own main() functions called in this process on one network (the checkpoint is not re-read; everything
else a command does is inside the clock: reading and decoding the JPEGs and the ground truth, capturing the forward graphs, the
forwards, the CRFs, the PNGs, the result file).  They alternate round by round after one unclocked round; host clock around each
command, images/s.  The three result files are compared first.

usage: python tools/predict_score_probe.py [N images, default 192] [rounds, default 4] [further predict options, e.g.
       --same-size-batch 8]      (one JSON line at the end)
"""
import contextlib
import io
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

C = 21
SIZES = ((375, 500), (500, 375), (375, 500), (333, 500))


def _files(d, n):
    from PIL import Image
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(93)
    os.makedirs(os.path.join(d, "VOC", "JPEGImages"))
    os.makedirs(os.path.join(d, "GT"))
    ids = ["im%04d" % k for k in range(n)]
    for k, i in enumerate(ids):
        H, W = SIZES[k % len(SIZES)]
        img = S.make_images(rng, 1, size=500, kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8)).save(
            os.path.join(d, "VOC", "JPEGImages", i + ".jpg"), quality=92)
        gt = rng.integers(0, C, ((H + 24) // 25, (W + 24) // 25), dtype=np.uint8).repeat(25, 0).repeat(25, 1)[:H, :W].copy()
        gt[rng.random((H, W)) < 0.05] = 255                              # VOC's object borders
        Image.fromarray(gt, mode="L").save(os.path.join(d, "GT", i + ".png"))
    with open(os.path.join(d, "val.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")


def _net():
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(3)
    net = VGG16ASPP(num_classes=C)
    for m in net.modules():                                              # (He-initialised: the masks hold several labels)
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                torch.nn.init.zeros_(m.bias)
    return net.cuda().to(memory_format=torch.channels_last).eval()


def main(argv):
    from dsrg_amd import _lib, evaluate, predict
    _lib.require_gpu()
    argv = list(argv)
    n = int(argv.pop(0)) if argv and argv[0].isdigit() else 192
    rounds = int(argv.pop(0)) if argv and argv[0].isdigit() else 4
    extra = argv                                                         # what is left goes to predict
    net = _net()
    with tempfile.TemporaryDirectory() as d:
        _files(d, n)
        common = ["--mode", "ms-f", "--smooth", "--model", "unused", "--images", os.path.join(d, "val.txt"), "--dir",
                  os.path.join(d, "VOC")] + extra
        gt, val = os.path.join(d, "GT"), os.path.join(d, "val.txt")

        def route_a(tag):
            out = os.path.join(d, "a" + tag)
            predict.main(common + ["--output", out], net=net)
            evaluate.main(["--pred", out, "--gt", gt, "--test_ids", val, "--save_path", os.path.join(d, "a.txt")])

        def route_b(tag):
            predict.main(common + ["--gt", gt, "--output", os.path.join(d, "b" + tag), "--save_path", os.path.join(d, "b.txt")], net=net)

        def route_c(tag):
            predict.main(common + ["--gt", gt, "--save_path", os.path.join(d, "c.txt")], net=net)

        routes = (("a", route_a), ("b", route_b), ("c", route_c))
        rates = {name: [] for name, _ in routes}
        for r in range(rounds + 1):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    fn(str(r))
                torch.cuda.synchronize()
                if r:                                                    # (round 0: MIOpen's picks, the allocator's pools)
                    rates[name].append(n / (time.perf_counter() - t0))
        results = [open(os.path.join(d, name + ".txt"), "rb").read() for name, _ in routes]
        same = results[0] == results[1] == results[2]
        miou = results[2].decode().split("\n")[0]
    med = {name: float(np.median(v)) for name, v in rates.items()}
    print("%d images (%s), VGG16-ASPP bf16, predict --mode ms-f --smooth %s; %d clocked rounds, images/s" %
          (n, ", ".join("%dx%d" % s for s in sorted(set(SIZES))), " ".join(extra), rounds))
    for name, what in (("a", "predict --output, then evaluate   "), ("b", "predict --gt --output             "),
                       ("c", "predict --gt                      ")):
        print("(%s) %s median %.1f (rounds: %s)" % (name, what, med[name], " ".join("%.1f" % v for v in rates[name])))
    print("    result files identical: %s (%s); (b) / (a) = %.3f, (c) / (a) = %.3f" % (same, miou, med["b"] / med["a"], med["c"] / med["a"]))
    print(json.dumps(dict(images=n, rounds=rounds, options=extra, images_per_s={k: [round(x, 1) for x in v] for k, v in rates.items()},
                          median_images_per_s={k: round(v, 1) for k, v in med.items()}, results_identical=same)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
