#!/usr/bin/env python
"""The fixed-size test-time loop (test-ms.py) with the forwards batched across images, against the per-image path, in one process.

  (a) inference.predict_masks_ms_many images/s on the workload of `bench.py --mode test-ms` (VGG16-ASPP under bf16 autocast, seeded
      synthetic images, forwards replayed from HIP graphs, in_flight = 3): forward_batch = 1 (the per-image path) alternating with
      forward_batch = 2 / 4 / 8, for CRF batch = 1 and 8, on 64 images of 375 x 500 and on 64 images alternating 375 x 500 /
      500 x 375.  Host clock around a window that ends in a device synchronise, every shape warmed first, three repeats each.
  (b) device-event medians of one group's dsrg_preprocess_ms_batch launch and dsrg_multiscale_unary_batch launch (8 images of
      375 x 500) against the torch compositions they replace (inference.preprocess per image and size on device-resident pixels;
      _zoom, sum, softmax, clamp, log, permute per image) and against 8 single-image dsrg_multiscale_unary launches.

usage: python tools/test_ms_batched_probe.py [a|b ...]     (default: both; one JSON line at the end)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# as bench.py --mode test-ms: no online GEMM tuning (three sizes x several batch sizes are hundreds of GEMM shapes)
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0")
# the heuristic pick of MIOpen for whatever convolution torch sends there, not an exhaustive search per new shape: both sides of
# every comparison run in this one process under the same setting
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

SIZES = (241, 321, 401)
N_IMAGES = 64
IN_FLIGHT = 3


def _images(shapes):
    """bench.py's test-ms images (seed 4242, four kinds), cut to the given shapes in turn"""
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(4242)
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


def probe_a():
    from dsrg_amd import inference as I
    net = _net()
    fwd = I.GraphedForward(net)
    sets = {"375x500": _images([(375, 500)] * 4), "375x500_500x375_alternating": _images([(375, 500), (500, 375)] * 2)}

    def window(ims, n, fb, cb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in I.predict_masks_ms_many(net, [ims[i % len(ims)] for i in range(n)], forward=fwd, in_flight=IN_FLIGHT,
                                                   batch=cb, forward_batch=fb))
        torch.cuda.synchronize()
        assert k == n
        return n / (time.perf_counter() - t0)

    res = []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for name, ims in sets.items():
            for cb in (1, 8):
                for fb in (1, 2, 4, 8):                                # every graph, CRF object and kernel of this setting
                    window(ims, 32, fb, cb)
                for fb in (2, 4, 8):
                    base, batched = [], []
                    for _ in range(3):
                        base.append(round(window(ims, N_IMAGES, 1, cb), 1))
                        batched.append(round(window(ims, N_IMAGES, fb, cb), 1))
                    r = dict(images=name, crf_batch=cb, forward_batch=fb, images_per_s_forward_batch_1=base, images_per_s=batched,
                             ratio_of_medians=round(float(np.median(batched) / np.median(base)), 3))
                    print("(a) %-28s CRF batch %d  forward_batch %d: %s images/s against %s at forward_batch 1 -> x%.3f"
                          % (name, cb, fb, batched, base, r["ratio_of_medians"]), flush=True)
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


def probe_b(G=8, H=375, W=500, C=21):
    from dsrg_amd import inference as I, ops
    dev = [torch.from_numpy(im).cuda() for im in _images([(H, W)] * G)]
    mean = torch.tensor(I.MEAN_PIXEL, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    out = [torch.empty((G, 3, S, S), dtype=torch.float32, device="cuda") for S in SIZES]

    def pre_kernel():
        return ops.preprocess_ms_batch(dev, SIZES, out=out)

    def pre_torch():                                                   # inference.preprocess after its upload, per image and size
        xs = []
        for S in SIZES:
            xs.append(torch.cat([I._zoom(d.to(torch.float32).permute(2, 0, 1)[None], S, S)[:, [2, 1, 0]] - mean for d in dev]))
        return xs

    g = torch.Generator(device="cuda").manual_seed(0)
    scores = [torch.randn(G, C, m, m, device="cuda", generator=g) * 3.0 for m in (31, 41, 51)]      # fc8 maps of 241 / 321 / 401
    shapes = [(H, W)] * G

    def unary_kernel():
        return ops.multiscale_unary_batch(scores, shapes, want="unary")

    def unary_single():
        return [ops.multiscale_unary([s[i:i + 1] for s in scores], H, W, want="unary") for i in range(G)]

    def unary_torch():
        outs = []
        for i in range(G):
            total = None
            for s in scores:
                z = I._zoom(s[i:i + 1], H, W)
                total = z if total is None else total + z
            outs.append(torch.log(I._probs_from_scores(total[0])).permute(1, 2, 0).contiguous())
        return outs

    r = dict(group=G, image="%dx%d" % (H, W), labels=C,
             preprocess_batch_us=round(_median_us(pre_kernel), 2), preprocess_torch_us=round(_median_us(pre_torch, reps=5), 1),
             unary_batch_us=round(_median_us(unary_kernel), 2), unary_single_launches_us=round(_median_us(unary_single), 2),
             unary_torch_us=round(_median_us(unary_torch, reps=3), 1))
    r["preprocess_speedup"] = round(r["preprocess_torch_us"] / r["preprocess_batch_us"], 1)
    r["unary_speedup_over_torch"] = round(r["unary_torch_us"] / r["unary_batch_us"], 1)
    print("(b) group of %d %dx%d images: preprocess %.2f us (torch %.1f us, %.1fx); unary %.2f us (%d single launches %.2f us, "
          "torch %.1f us, %.1fx)" % (G, H, W, r["preprocess_batch_us"], r["preprocess_torch_us"], r["preprocess_speedup"],
                                     r["unary_batch_us"], G, r["unary_single_launches_us"], r["unary_torch_us"],
                                     r["unary_speedup_over_torch"]), flush=True)
    return r


def main(which):
    from dsrg_amd import _lib
    _lib.require_gpu()
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    out = {"device": torch.cuda.get_device_name(0), "sizes": list(SIZES), "images_per_window": N_IMAGES, "in_flight": IN_FLIGHT}
    if "b" in which:
        out["b"] = probe_b()
    if "a" in which:
        out["a"] = probe_a()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or ["a", "b"])
