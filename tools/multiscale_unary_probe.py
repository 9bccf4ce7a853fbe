#!/usr/bin/env python
"""Timings of the final test at relative scales (test-ms-f.py): device-event medians after warm-up.

  (a) ops.multiscale_unary (one dsrg_multiscale_unary launch) against the torch composition it replaces (_zoom of every scale in
      float64, sum, softmax, clamp, log, permute to label-fastest): 375 x 500, C = 21, maps 36x47 / 47x63 / 59x79 (the relative
      scales of a VOC image), and 480 x 640, C = 81, K = 1 (COCO's single scale of 481)
  (b) inference.predict_mask_ms_f per image at 375 x 500 on VGG16-ASPP (bf16 autocast): eager forwards against a bounded
      GraphedForward
  (c) inference.predict_masks_ms_f_many images/s over 64 synthetic images of a VOC-like mix of shapes

usage: python tools/multiscale_unary_probe.py [a|b|c ...]     (default: all three; one JSON line at the end)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def _median_us(fn, reps=50, rounds=11, warmup=10):
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


def probe_a():
    from dsrg_amd import inference as I, ops
    res = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (H, W), C, sizes in [("voc_375x500_c21_k3", (375, 500), 21, [(36, 47), (47, 63), (59, 79)]),
                                   ("coco_480x640_c81_k1", (480, 640), 81, [(61, 61)])]:
        scores = [torch.randn(1, C, h, w, device="cuda", generator=g) * 3.0 for h, w in sizes]

        def fused():
            return ops.multiscale_unary(scores, H, W, want="unary")

        def composed():
            total = None
            for s in scores:
                z = I._zoom(s, H, W)
                total = z if total is None else total + z
            return torch.log(I._probs_from_scores(total[0])).permute(1, 2, 0).contiguous()

        tf, tt = _median_us(fused), _median_us(composed, reps=10)
        out_mb = H * W * C * 4 / 1e6
        in_mb = sum(C * h * w * 4 for h, w in sizes) / 1e6
        r = dict(case=name, fused_us=round(tf, 2), torch_us=round(tt, 1), speedup=round(tt / tf, 1),
                 unary_mb=round(out_mb, 2), maps_mb=round(in_mb, 3), fused_tb_s=round((out_mb + in_mb) / tf, 2))
        print("(a) %-22s fused %7.2f us   torch %8.1f us   %5.1fx   %.2f MB written -> %.2f TB/s" %
              (name, tf, tt, tt / tf, out_mb, (out_mb + in_mb) / tf))
        res.append(r)
    return res


def _voc_image(rng, H, W):
    from dsrg_amd import synthetic as S
    im = (S.make_images(rng, 1, size=max(H, W), kind="noise")[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
    return np.ascontiguousarray(im[:, :, ::-1]).clip(0, 255).astype(np.uint8)


def _net():
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(0)
    return VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()


def probe_b(net):
    from dsrg_amd import inference as I
    im = _voc_image(np.random.default_rng(1), 375, 500)
    res = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for name, fwd in (("eager", None), ("graphed", I.GraphedForward(net, max_shapes=12, capture_after=2))):
            for _ in range(4):
                I.predict_mask_ms_f(net, im, forward=fwd)
            t = []
            for _ in range(15):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                I.predict_mask_ms_f(net, im, forward=fwd)
                t.append((time.perf_counter() - t0) * 1e3)
            res[name + "_ms"] = round(float(np.median(t)), 2)
            print("(b) predict_mask_ms_f 375x500 %-8s %.2f ms per image (median of 15)" % (name, res[name + "_ms"]))
    return res


def probe_c(net):
    from dsrg_amd import inference as I
    rng = np.random.default_rng(2)
    other = [(334, 500), (500, 334), (366, 500), (500, 366), (333, 500), (281, 500), (375, 400), (442, 500)]
    shapes = []
    for k in range(64):
        r = rng.random()
        shapes.append((375, 500) if r < 0.45 else (500, 375) if r < 0.7 else other[k % len(other)])
    ims = [_voc_image(rng, H, W) for H, W in shapes]
    fwd = I.GraphedForward(net, max_shapes=12, capture_after=2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in I.predict_masks_ms_f_many(net, ims[:8], forward=fwd):            # warm-up: kernels, CRF objects, common graphs
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in I.predict_masks_ms_f_many(net, ims, forward=fwd))
        dt = time.perf_counter() - t0
    res = dict(images=n, distinct_shapes=len(set(shapes)), images_per_s=round(n / dt, 1), graphs_kept=len(fwd._g))
    print("(c) predict_masks_ms_f_many: %d images (%d shapes) in %.2f s -> %.1f images/s, %d graphs kept" %
          (n, res["distinct_shapes"], dt, res["images_per_s"], res["graphs_kept"]))
    return res


def main(which):
    from dsrg_amd import _lib
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0)}
    if "a" in which:
        out["a"] = probe_a()
    if "b" in which or "c" in which:
        net = _net()
        if "b" in which:
            out["b"] = probe_b(net)
        if "c" in which:
            out["c"] = probe_c(net)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or ["a", "b", "c"])
