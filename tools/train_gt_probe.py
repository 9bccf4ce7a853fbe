#!/usr/bin/env python
"""Label-restricted pseudo-label generation (generate_train_gt.py): the batched path against the per-image one, in one process.

  (a) images/s on 64 seeded synthetic 375 x 500 images with 1-3 image-level labels each, VGG16-ASPP under bf16 autocast: a loop
      of inference.predict_train_gt (eager batch-1 forward, torch tail, CRF on the null stream, marginals read back through torch
      indexing) alternating with inference.predict_train_gt_many(forward_batch=8, in_flight=3) at CRF batch = 1 and 8 (forwards
      replayed from one batch-8 graph).  Host clock around a window that ends in a device synchronise, every shape warmed first,
      three repeats each.
  (b) device-event medians of one group's tail, ops.train_gt_unary_batch (8 images of 375 x 500, 41 x 41 maps: the pseudo-label
      kernels of train_gt.hip at one map per image, train_gt_ms_softmax_kernel and train_gt_ms_zoom_kernel<1, false>) against the
      torch composition it replaces (softmax, fp64 zoom, clamp, log, permute per image), and of the restricted MAP
      (CRF_device(want="map", select=...)) against marginals + torch indexing on one 375 x 500 image.
  (k) a short run of the tail's two kernels and the selection kernels and nothing else, for `rocprofv3 --kernel-trace --stats --
      python tools/train_gt_probe.py k`.

usage: python tools/train_gt_probe.py [a|b|k ...]     (default: a b; one JSON line at the end)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0")        # as tools/test_ms_batched_probe.py
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

N_IMAGES = 64
IN_FLIGHT = 3
FORWARD_BATCH = 8
H, W = 375, 500


def _items(n):
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(4242)
    out = []
    for k in range(n):
        img = S.make_images(rng, 1, size=max(H, W), kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        im = np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8)
        out.append((im, sorted(int(c) for c in rng.choice(np.arange(1, 21), size=1 + k % 3, replace=False))))
    return out


def _net():
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(0)
    return VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()


def probe_a():
    from dsrg_amd import inference as I
    net = _net()
    fwd = I.GraphedForward(net)
    items = _items(4)

    def feed(n):
        return [items[i % len(items)] for i in range(n)]

    def per_image(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for im, labels in feed(n):
            I.predict_train_gt(net, im, labels)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    def many(n, cb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in I.predict_train_gt_many(net, feed(n), forward=fwd, in_flight=IN_FLIGHT, batch=cb,
                                                   forward_batch=FORWARD_BATCH))
        torch.cuda.synchronize()
        assert k == n
        return n / (time.perf_counter() - t0)

    res = []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        per_image(8)
        for cb in (1, 8):
            many(32, cb)
        for cb in (1, 8):
            base, batched = [], []
            for _ in range(3):
                base.append(round(per_image(N_IMAGES), 1))
                batched.append(round(many(N_IMAGES, cb), 1))
            r = dict(crf_batch=cb, forward_batch=FORWARD_BATCH, images_per_s_predict_train_gt=base, images_per_s_many=batched,
                     ratio_of_medians=round(float(np.median(batched) / np.median(base)), 3))
            print("(a) CRF batch %d: predict_train_gt_many %s images/s against %s for the predict_train_gt loop -> x%.3f"
                  % (cb, batched, base, r["ratio_of_medians"]), flush=True)
            res.append(r)
    return res


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


def _kernel_inputs(G=8, C=21, m=41):
    g = torch.Generator(device="cuda").manual_seed(0)
    scores = torch.randn(G, C, m, m, device="cuda", generator=g) * 3.0
    im = torch.from_numpy(_items(1)[0][0]).cuda()
    unary = torch.log_softmax(torch.randn(H, W, C, device="cuda", generator=g) * 3.0, dim=2).contiguous()
    return scores, im, unary


def probe_b(G=8, C=21):
    from dsrg_amd import inference as I, ops
    from dsrg_amd.crf import CRF_device
    scores, im, unary = _kernel_inputs(G, C)
    shapes = [(H, W)] * G
    sel = [0, 3, 7]
    sel_t = torch.as_tensor(sel, device="cuda")

    def unary_kernel():
        return ops.train_gt_unary_batch(scores, shapes, want="unary")

    def unary_torch():
        outs = []
        for i in range(G):
            p = torch.clamp(I._zoom(torch.softmax(scores[i:i + 1], dim=1), H, W)[0], min=0.00001)
            outs.append(torch.log(p).permute(1, 2, 0).contiguous())
        return outs

    def map_select():
        return CRF_device(im, unary, scale_factor=1.0, want="map", select=sel)

    def map_plain():
        return CRF_device(im, unary, scale_factor=1.0, want="map")

    def map_torch():
        p = CRF_device(im, unary, scale_factor=1.0)
        return sel_t[p[:, :, sel_t].argmax(2)]

    r = dict(group=G, image="%dx%d" % (H, W), labels=C,
             unary_batch_us=round(_median_us(unary_kernel), 2), unary_torch_us=round(_median_us(unary_torch, reps=3), 1),
             crf_map_select_us=round(_median_us(map_select, reps=3), 1), crf_map_us=round(_median_us(map_plain, reps=3), 1),
             crf_marginals_torch_select_us=round(_median_us(map_torch, reps=3), 1))
    r["unary_speedup_over_torch"] = round(r["unary_torch_us"] / r["unary_batch_us"], 1)
    print("(b) group of %d %dx%d images: unary %.2f us (torch %.1f us, %.1fx); one CRF ending in the restricted MAP %.1f us, in the "
          "plain MAP %.1f us, in marginals + torch indexing %.1f us"
          % (G, H, W, r["unary_batch_us"], r["unary_torch_us"], r["unary_speedup_over_torch"], r["crf_map_select_us"],
             r["crf_map_us"], r["crf_marginals_torch_select_us"]), flush=True)
    return r


def probe_k(G=8, C=21):
    """only the tail's kernels at one map per image (and the CRF the selection kernel follows): for a kernel trace"""
    from dsrg_amd import ops
    from dsrg_amd.crf import CRF_device
    scores, im, unary = _kernel_inputs(G, C)
    for _ in range(20):
        ops.train_gt_unary_batch(scores, [(H, W)] * G, want="unary")
        ops.train_gt_unary_batch(scores, [(H, W)] * G, want="labels", select=[[0, 3, 7]] * G)
    for _ in range(5):
        CRF_device(im, unary, scale_factor=1.0, want="map", select=[0, 3, 7])                  # global-memory path
        CRF_device(im[:37, :53].contiguous(), unary[:37, :53].contiguous(), scale_factor=1.0, want="map", select=[0, 3, 7])   # LDS path
    torch.cuda.synchronize()
    return dict(unary_launches=40, select_launches=10)


def main(which):
    from dsrg_amd import _lib
    _lib.require_gpu()
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    out = {"device": torch.cuda.get_device_name(0), "images_per_window": N_IMAGES, "in_flight": IN_FLIGHT}
    if "k" in which:
        out["k"] = probe_k()
    if "b" in which:
        out["b"] = probe_b()
    if "a" in which:
        out["a"] = probe_a()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or ["a", "b"])
