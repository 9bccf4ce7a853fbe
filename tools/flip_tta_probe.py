#!/usr/bin/env python
"""Mirrored test-time augmentation (flip=True of the ms / ms-f tests), measured in one process.

  (1) the mirror kernels against the work they replace, at the workload's shapes (21 labels, a 375 x 500 image, the fc8 maps of
      the scales 0.75 / 1 / 1.25 and of the sizes 241 / 321 / 401): each mirror kernel against the existing kernel fed by
      torch.flip + cat copies of the maps / inputs.  Device-event medians, every shape warmed first; the spread is (max - min) /
      median over the rounds.
  (2) the mirror instantiations against the existing kernels on the same 2K maps with no flag set: what the reversed
      addressing itself costs.
  (3) images/s of predict_masks_ms_many / predict_masks_ms_f_many with and without flip on seeded synthetic 375 x 500 images,
      VGG16-ASPP under bf16 autocast, graphed forwards, CRFs in flight (--smooth), per image and in groups of 8; plain and flip
      windows alternate, three repeats each, host clock around a window that ends in a device synchronise.

usage: python tools/flip_tta_probe.py [1|2|3 ...] [--out FILE]     (default: all three; FILE: profiles/flip_tta_probe.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# as tools/test_ms_batched_probe.py: no online GEMM tuning, MIOpen's heuristic pick; both sides of every comparison run in this one
# process under the same setting
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "0")
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

H, W, C = 375, 500, 21
SIZES = (241, 321, 401)
SCALES = (0.75, 1.0, 1.25)
MAPS = {"ms": [(31, 31), (41, 41), (51, 51)],                         # fc8 maps of 241 / 321 / 401
        "ms-f": [(36, 47), (47, 63), (59, 79)]}                       # ... of 281 x 375, 375 x 500, 469 x 625
GROUP = 8
N_IMAGES = 64
IN_FLIGHT = 3
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


def _compare(tag, new, old, new_name, old_name):
    """alternate the two sides twice, report both medians of each"""
    rows = {new_name: [], old_name: []}
    for _ in range(2):
        rows[new_name].append(_timed(new))
        rows[old_name].append(_timed(old))
    n = min(m for m, _ in rows[new_name])
    o = min(m for m, _ in rows[old_name])
    spread = max(s for v in rows.values() for _, s in v)
    say("%-46s %s %s us | %s %s us | ratio of the lower medians %.3f (largest spread within a side %.1f %%)"
        % (tag, new_name, ["%.2f" % m for m, _ in rows[new_name]], old_name, ["%.2f" % m for m, _ in rows[old_name]], o / n,
           100.0 * spread))
    return dict(case=tag, new_us=[round(m, 2) for m, _ in rows[new_name]], old_us=[round(m, 2) for m, _ in rows[old_name]],
                old_over_new=round(o / n, 3), spread=round(spread, 3))


def _images(n):
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(4242)
    out = []
    for k in range(n):
        img = S.make_images(rng, 1, size=max(H, W), kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        out.append(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8))
    return out


def probe_kernels(which):
    from dsrg_amd import inference as I, ops
    g = torch.Generator(device="cuda").manual_seed(0)
    res = []
    dev = [torch.from_numpy(im).cuda() for im in _images(GROUP)]
    for mode, maps in MAPS.items():
        K = len(maps)
        pair = [torch.randn(2, C, h, w, device="cuda", generator=g) * 3.0 for h, w in maps]            # one image: batch-2 outputs
        group = [torch.randn(2 * GROUP, C, h, w, device="cuda", generator=g) * 3.0 for h, w in maps]   # a group: batch-16 outputs
        slices = [s[j:j + 1] for s in pair for j in (0, 1)]
        shapes = [(H, W)] * GROUP
        if "1" in which:
            say("(1) %s maps %s -> %d x %d, %d labels" % (mode, maps, H, W, C))

            def one_new():
                return ops.multiscale_unary(slices, H, W, want="unary", mirror=[0, 1] * K)

            def one_old():
                flipped = [t for s in pair for t in (s[0:1], torch.flip(s[1:2], [-1]))]
                return ops.multiscale_unary(flipped, H, W, want="unary")

            res.append(_compare("%s unary, 1 image, %d maps" % (mode, 2 * K), one_new, one_old, "mirror kernel", "flip + kernel"))

            def group_new():
                return ops.multiscale_unary_mirror_batch(group, shapes, want="unary")

            def group_old():
                flipped = [t for s in group for t in (s[0::2].contiguous(), torch.flip(s[1::2], [-1]))]
                return ops.multiscale_unary_batch(flipped, shapes, want="unary")

            res.append(_compare("%s unary, %d images, %d maps" % (mode, GROUP, 2 * K), group_new, group_old, "mirror kernel",
                                "flip + cat + kernel"))
            targets = [(S, S) for S in SIZES] if mode == "ms" else [(I.relative_size(H, s), I.relative_size(W, s)) for s in SCALES]
            out2 = [torch.empty((2 * GROUP, 3, h, w), dtype=torch.float32, device="cuda") for h, w in targets]
            out1 = [torch.empty((GROUP, 3, h, w), dtype=torch.float32, device="cuda") for h, w in targets]

            def pre_new():
                return ops.preprocess_rect_mirror_batch(dev, targets, out=out2)

            def pre_old():
                xs = ops.preprocess_rect_batch(dev, targets, out=out1)
                return [torch.stack([x, torch.flip(x, [-1])], 1).reshape((2 * GROUP,) + tuple(x.shape[1:])) for x in xs]

            res.append(_compare("%s preprocess, %d images, %d sizes" % (mode, GROUP, K), pre_new, pre_old, "mirror kernel",
                                "kernel + flip + cat"))
        if "2" in which:
            say("(2) %s: the mirror instantiation with no flag set against the existing kernel, same %d maps" % (mode, 2 * K))
            res.append(_compare("%s unary, 1 image, %d maps, flags 0" % (mode, 2 * K),
                                lambda: ops.multiscale_unary(slices, H, W, want="unary", mirror=[0] * (2 * K)),
                                lambda: ops.multiscale_unary(slices, H, W, want="unary"), "mirror<2K>", "plain<2K>"))
    return res


def probe_throughput():
    from dsrg_amd import inference as I
    from dsrg_amd.backbone import VGG16ASPP
    from dsrg_amd.crf import MAX_BATCH
    torch.manual_seed(0)
    net = VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()
    ims = _images(4)
    fwd_ms = I.GraphedForward(net)
    fwd_f = I.GraphedForward(net, max_shapes=12, capture_after=2)

    def run(mode, group, flip, n):
        seq = [ims[i % len(ims)] for i in range(n)]
        if mode == "ms":
            gen = I.predict_masks_ms_many(net, seq, sizes=SIZES, forward=fwd_ms, in_flight=IN_FLIGHT, forward_batch=group, flip=flip)
        else:
            gen = I.predict_masks_ms_f_many(net, seq, scales=SCALES, forward=fwd_f, in_flight=IN_FLIGHT,
                                            batch=min(group, MAX_BATCH), same_size_batch=group, flip=flip)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = sum(1 for _ in gen)
        torch.cuda.synchronize()
        assert k == n
        return n / (time.perf_counter() - t0)

    res = []
    say("(3) images/s, VGG16-ASPP bf16, %d x %d, --smooth, in_flight %d, %d images per window" % (H, W, IN_FLIGHT, N_IMAGES))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for mode in ("ms", "ms-f"):
            for group in (1, GROUP):
                for flip in (False, True):                              # every graph, CRF object and kernel of this setting
                    run(mode, group, flip, 3 * max(group, 4))
                plain, flipped = [], []
                for _ in range(3):
                    plain.append(round(run(mode, group, False, N_IMAGES), 1))
                    flipped.append(round(run(mode, group, True, N_IMAGES), 1))
                ratio = float(np.median(plain) / np.median(flipped))
                say("%-5s group %d: plain %s images/s, flip %s images/s -> the flip run costs x%.3f the plain run (medians)"
                    % (mode, group, plain, flipped, ratio))
                res.append(dict(mode=mode, group=group, images_per_s_plain=plain, images_per_s_flip=flipped,
                                flip_cost_ratio=round(ratio, 3)))
    return res


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "flip_tta_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    which = argv or ["1", "2", "3"]
    from dsrg_amd import _lib
    _lib.require_gpu()
    try:
        torch.cuda.tunable.enable(False)
        torch.cuda.tunable.tuning_enable(False)
    except Exception:
        pass
    say("tools/flip_tta_probe.py %s on %s" % (" ".join(which), torch.cuda.get_device_name(0)))
    out = {"device": torch.cuda.get_device_name(0)}
    if "1" in which or "2" in which:
        out["kernels"] = probe_kernels(which)
    if "3" in which:
        out["throughput"] = probe_throughput()
    say(json.dumps(out))
    with open(out_path, "w") as f:
        f.write("\n".join(_LINES) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
