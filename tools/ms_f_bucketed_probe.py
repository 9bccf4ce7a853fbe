#!/usr/bin/env python
"""The relative-scale final test (test-ms-f.py) with the forwards batched across same-sized images, against the per-image path, in
one process.

  (a) inference.predict_masks_ms_f_many images/s on VGG16-ASPP under bf16 autocast over a generated list of 128 images:
      same_size_batch = 1 (the per-image path, CRF batch 1: what `python -m dsrg_amd.predict --mode ms-f --smooth` runs) alternating
      with same_size_batch = 2 / 4 / 8 (CRF batch min(G, 8), window 64: what --same-size-batch G runs).  Each side has its own
      GraphedForward(max_shapes=12, capture_after=2), as each would have in a run of its own.  Host clock around a window that
      ends in a device synchronise, one full pass per setting as warm-up, three repeats each.
      THE SIZE MIX IS ASSUMED, NOT TAKEN FROM THE DATASET: about 60 % 375 x 500, 20 % 500 x 375, the rest spread over eight
      other sizes.  Also printed: the histogram of the group sizes inference.plan_size_groups emits on that list.
  (b) device-event medians of one dsrg_preprocess_rect_batch launch (8 images of 375 x 500 at 0.75 / 1 / 1.25, and 1 image) against
      the per-image torch composition it replaces (inference.preprocess_relative after its upload, per image and scale).

usage: python tools/ms_f_bucketed_probe.py [a|b ...]     (default: both; one JSON line at the end)
"""
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# no online GEMM tuning and MIOpen's heuristic pick (as tools/test_ms_batched_probe.py): batch sizes x sizes x scales are many shapes,
# and both sides of every comparison run in this one process under the same setting
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0")
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

SCALES = (0.75, 1.0, 1.25)
N_IMAGES = 128
IN_FLIGHT = 3
WINDOW = 64
MAX_GRAPHS = 12
OTHER = [(334, 500), (500, 334), (366, 500), (500, 366), (333, 500), (281, 500), (375, 400), (442, 500)]


def _shapes(n=N_IMAGES, seed=2):
    """the ASSUMED size mix (not the dataset's): ~60 % 375 x 500, ~20 % 500 x 375, the rest over eight other sizes in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        r = rng.random()
        out.append((375, 500) if r < 0.6 else (500, 375) if r < 0.8 else OTHER[k % len(OTHER)])
    return out


def _images(shapes, seed=4242):
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(seed)
    out = []
    for k, (H, W) in enumerate(shapes):
        img = S.make_images(rng, 1, size=max(H, W), kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        out.append(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8))
    return out


def _net():
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(0)
    return VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()


def group_histogram(shapes, G, window=WINDOW):
    from dsrg_amd import inference as I
    h = collections.Counter(len(g) for g in I.plan_size_groups(shapes, G, window))
    return {str(n): h[n] for n in sorted(h)}


def probe_a():
    from dsrg_amd import inference as I
    from dsrg_amd.crf import MAX_BATCH
    shapes = _shapes()
    ims = _images(shapes)
    mix = collections.Counter(shapes)
    print("(a) ASSUMED size mix (not taken from the dataset), %d images: %s"
          % (len(shapes), ", ".join("%dx%d: %d" % (H, W, n) for (H, W), n in mix.most_common())), flush=True)
    net = _net()
    fwds = {G: I.GraphedForward(net, max_shapes=MAX_GRAPHS, capture_after=2) for G in (1, 2, 4, 8)}

    def window(G):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in I.predict_masks_ms_f_many(net, ims, scales=SCALES, forward=fwds[G], in_flight=IN_FLIGHT,
                                                     batch=min(G, MAX_BATCH), same_size_batch=G, window=WINDOW))
        torch.cuda.synchronize()
        assert k == len(ims)
        return len(ims) / (time.perf_counter() - t0)

    res = []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for G in (1, 2, 4, 8):                                         # kernels, CRF objects, the common shapes' graphs
            window(G)
        for G in (2, 4, 8):
            hist = group_histogram(shapes, G)
            base, batched = [], []
            for _ in range(3):
                base.append(round(window(1), 1))
                batched.append(round(window(G), 1))
            r = dict(same_size_batch=G, window=WINDOW, crf_batch=min(G, MAX_BATCH), group_sizes=hist,
                     images_per_s_same_size_batch_1=base, images_per_s=batched,
                     ratio_of_medians=round(float(np.median(batched) / np.median(base)), 3), graphs_kept=len(fwds[G]._g))
            print("(a) same_size_batch %d (window %d, CRF batch %d; groups by size %s): %s images/s against %s at same_size_batch 1 "
                  "-> x%.3f; %d graphs kept" % (G, WINDOW, r["crf_batch"], hist, batched, base, r["ratio_of_medians"],
                                                r["graphs_kept"]), flush=True)
            res.append(r)
    return dict(size_mix="assumed, not taken from the dataset", images=len(ims),
                sizes={"%dx%d" % k: v for k, v in mix.items()}, runs=res)


def _median_us(fn, reps=20, rounds=9, warmup=5):
    """median over `rounds` of (device time of `reps` back-to-back calls) / reps"""
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
    return float(np.median(t))


def probe_b(H=375, W=500):
    from dsrg_amd import inference as I, ops
    targets = [(I.relative_size(H, s), I.relative_size(W, s)) for s in SCALES]
    mean = torch.tensor(I.MEAN_PIXEL, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    res = []
    for G in (8, 1):
        dev = [torch.from_numpy(im).cuda() for im in _images([(H, W)] * G)]
        out = [torch.empty((G, 3, h, w), dtype=torch.float32, device="cuda") for h, w in targets]

        def kernel():
            return ops.preprocess_rect_batch(dev, targets, out=out)

        def composition():                                             # inference.preprocess_relative after its upload
            return [I._zoom(d.to(torch.float32).permute(2, 0, 1)[None], h, w)[:, [2, 1, 0]] - mean for d in dev for h, w in targets]

        r = dict(group=G, image="%dx%d" % (H, W), targets=["%dx%d" % t for t in targets],
                 preprocess_rect_batch_us=round(_median_us(kernel), 2), torch_composition_us=round(_median_us(composition, reps=5), 1))
        r["speedup"] = round(r["torch_composition_us"] / r["preprocess_rect_batch_us"], 1)
        print("(b) %d image(s) of %dx%d at %s: dsrg_preprocess_rect_batch %.2f us, per-image torch composition %.1f us (%.1fx)"
              % (G, H, W, SCALES, r["preprocess_rect_batch_us"], r["torch_composition_us"], r["speedup"]), flush=True)
        res.append(r)
    return res


def main(which):
    from dsrg_amd import _lib
    _lib.require_gpu()
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    out = {"device": torch.cuda.get_device_name(0), "scales": list(SCALES), "in_flight": IN_FLIGHT}
    if "b" in which:
        out["b"] = probe_b()
    if "a" in which:
        out["a"] = probe_a()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or ["a", "b"])
