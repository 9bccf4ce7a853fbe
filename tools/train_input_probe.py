#!/usr/bin/env python
"""The GPU training input pipeline (dsrg_amd/input.py, csrc/train_input.hip) measured in one process, the sides of every comparison
alternating.

  (a) images/s of each loader alone (TrainSInput at batch 20 / 321, TrainFInput at batch 10 / crop 321) on generated JPEG files of
      VOC-like sizes (375 x 500 and 500 x 375), 8 decoding threads: host clock around a window that ends in a device synchronise.
  (b) device-event medians of 200 back-to-back ops.train_s_input_batch calls (20 images) and ops.train_f_input_batch calls (10
      images): an upper bound on the kernels' time, since every call builds its argument arrays on the host.  The kernels' own time
      comes from a trace of mode k.
  (c) images/s of DSRGTrainer.step fed by TrainSInput against the same steps on resident tensors, windows of 50 steps.
  (d) the host composition the stage-1 kernel replaces: numpy restatement of the resize -> AnnotationLayer -> float32 upload, per
      batch of 20 (host clock, ends in a device synchronise).

  (e) as (b) for the stage-2 launch at batch 10 / crop 513 without and with rescaling (train_f_input_scaled_kernel, factors 0.5 ...
      1.5 over the 10 images), the sides alternating.
  (f) images/s of TrainFInput at batch 10 / crop 513 without and with scale_factors = 0.5 ... 1.5, alternating windows.

  (k) the two launches alone, 200 times each, for `rocprofv3 --kernel-trace --stats` in a run of its own (tools/rocpd_stats.py
      summarises its database).
  (j) the same for the two stage-2 launches of (e).

  (m) the cue-map feeder of the 81-class runs (TrainSCueMapInput, train_s_cuemap_input_kernel) at B = 20, C = 81, 321 / 41 x 41:
      the launch alone as in (b); the host composition it replaces (layers.AnnotationLayerCOCO.load_next_image x 20 — decode, scipy
      zoom, one-hot scatter — plus the three uploads; also with the files already decoded); DSRGTrainer.step at C = 81 fed by the
      loader against the same step on resident tensors; the C = 81 step next to the C = 21 step, both on resident tensors.  The
      sides of every comparison alternate within the one process.

usage: python tools/train_input_probe.py [a|b|c|d|e|f|j|k|m ...]     (default: a b c d; one JSON line at the end)
"""
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "2")

import numpy as np
import torch

N_FILES = 60
MEAN = (104.0, 117.0, 123.0)


def _files(d):
    """N_FILES JPEG images / PNG labels of 375 x 500 and 500 x 375, the two list files and a cue pickle"""
    from PIL import Image
    from dsrg_amd import synthetic as S
    rng = np.random.default_rng(77)
    cues, s_lines, f_lines = {}, [], []
    for k in range(N_FILES):
        H, W = ((375, 500), (500, 375))[k % 2]
        img = S.make_images(rng, 1, size=500, kind=["smooth", "noise", "dark_corner", "smooth"][k % 4])[0, :, :H, :W] + \
            S.MEAN_PIXEL[:, None, None]
        Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0))[:, :, ::-1]).clip(0, 255).astype(np.uint8)).save(
            os.path.join(d, "im%d.jpg" % k), quality=92)
        Image.fromarray(rng.integers(0, 21, (H // 25, W // 25), dtype=np.uint8).repeat(25, 0).repeat(25, 1), mode="L").save(
            os.path.join(d, "lab%d.png" % k))
        s_lines.append("im%d.jpg %d\n" % (k, k))
        f_lines.append("/im%d.jpg /lab%d.png\n" % (k, k))
        cues['%i_labels' % k] = np.array(sorted(rng.choice(np.arange(1, 21), size=2, replace=False)))
        cues['%i_cues' % k] = np.stack([rng.integers(0, 21, 400), rng.integers(0, 41, 400), rng.integers(0, 41, 400)])
    paths = dict(s=os.path.join(d, "s.txt"), f=os.path.join(d, "f.txt"), cues=os.path.join(d, "cues.pickle"), root=d)
    open(paths["s"], "w").write("".join(s_lines))
    open(paths["f"], "w").write("".join(f_lines))
    with open(paths["cues"], "wb") as f:
        pickle.dump(cues, f, protocol=2)
    return paths


def _loaders(p, workers=8):
    from dsrg_amd.input import TrainFInput, TrainSInput
    s = lambda: TrainSInput(p["s"], p["root"] + "/", p["cues"], batch_size=20, workers=workers)                    # noqa: E731
    f = lambda: TrainFInput(dict(source=p["f"], root_folder=p["root"], batch_size=10, crop_size=(321, 321), mean=MEAN,      # noqa: E731
                                 mirror=True), workers=workers)
    return s, f


def _window(loader, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        next(loader)
    torch.cuda.synchronize()
    return batches * loader.batch_size / (time.perf_counter() - t0)


def probe_a(p):
    mk_s, mk_f = _loaders(p)
    out = {}
    with mk_s() as s, mk_f() as f:
        _window(s, 3), _window(f, 3)
        rs, rf = [], []
        for _ in range(3):
            rs.append(round(_window(s, 60), 1))
            rf.append(round(_window(f, 120), 1))
        out = dict(train_s_images_per_s=rs, train_f_images_per_s=rf, workers=8)
    print("(a) loaders alone: TrainSInput %s images/s, TrainFInput %s images/s" % (rs, rf), flush=True)
    return out


def _median_us(fn, reps=20, rounds=9, warmup=5):
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


def _s_batch(p, n=20):
    from dsrg_amd import input as I
    cues = pickle.load(open(p["cues"], "rb"))
    images = [I.read_rgb(os.path.join(p["root"], "im%d.jpg" % k)) for k in range(n)]
    anno = [I.cue_arrays(cues, k) for k in range(n)]
    return images, [a[0] for a in anno], [a[1] for a in anno]


def _kernel_calls(p):
    """-> (launch stage 1, launch stage 2, byte counts): one batch of 20 / of 10 staged on the device, outputs preallocated"""
    from dsrg_amd import input as I, ops
    images, cues, labels = _s_batch(p)
    nbytes, desc = I.layout_train_s([im.shape[:2] for im in images], [c.shape[1] for c in cues], [l.size for l in labels],
                                    [k % 2 for k in range(20)])
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_s(buf, desc, images, cues, labels)
    stage = torch.from_numpy(buf).cuda()
    out = ops.train_s_input_batch(stage, desc)
    labs = [I.read_gray(os.path.join(p["root"], "lab%d.png" % k)) for k in range(10)]
    fbytes, fdesc = I.layout_train_f([l.shape for l in labs], [k * 5 for k in range(10)], [k * 3 for k in range(10)],
                                     [k % 2 for k in range(10)])
    fbuf = np.zeros(fbytes, np.uint8)
    I.pack_train_f(fbuf, fdesc, images[:10], labs)
    fstage = torch.from_numpy(fbuf).cuda()
    fout = ops.train_f_input_batch(fstage, fdesc, (321, 321), MEAN)
    sizes = dict(train_s_staging_bytes=nbytes, train_s_output_bytes=sum(o.numel() * 4 for o in out),
                 train_f_staging_bytes=fbytes, train_f_output_bytes=sum(o.numel() * 4 for o in fout))
    return (lambda: ops.train_s_input_batch(stage, desc, out=out),
            lambda: ops.train_f_input_batch(fstage, fdesc, (321, 321), MEAN, out=fout), sizes)


def probe_b(p):
    run_s, run_f, sizes = _kernel_calls(p)
    s_us, f_us = _median_us(run_s, reps=200), _median_us(run_f, reps=200)
    r = dict(train_s_call_us=round(s_us, 2), train_f_call_us=round(f_us, 2), **sizes)
    print("(b) back-to-back calls, device events (an UPPER BOUND on kernel time: the host builds the argument arrays per call): "
          "train-s %.2f us for 20 images (%d staging bytes -> %d output bytes); train-f %.2f us for 10 images"
          % (s_us, sizes["train_s_staging_bytes"], sizes["train_s_output_bytes"], f_us), flush=True)
    return r


def probe_k(p, launches=200):
    """kernels only, for a trace: rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/train_input_probe.py k, then
    tools/rocpd_stats.py DIR/NAME_results.db"""
    run_s, run_f, sizes = _kernel_calls(p)
    for _ in range(launches):
        run_s()
        run_f()
    torch.cuda.synchronize()
    return dict(launches_each=launches, **sizes)


SCALE_FACTORS = (0.5, 0.75, 1.0, 1.25, 1.5)


def _scaled_calls(p, crop=513, n=10):
    """-> (launch train_f_input_kernel, launch train_f_input_scaled_kernel, sizes): the same 10 staged images at crop 513, the scaled
    launch with the factors 0.5 ... 1.5 twice over, offsets in the middle of each window's slack"""
    from dsrg_amd import data as D, input as I, ops
    images = [I.read_rgb(os.path.join(p["root"], "im%d.jpg" % k)) for k in range(n)]
    labs = [I.read_gray(os.path.join(p["root"], "lab%d.png" % k)) for k in range(n)]
    shapes = [l.shape for l in labs]
    scaled = [D.scaled_size(H, W, SCALE_FACTORS[k % 5]) for k, (H, W) in enumerate(shapes)]
    mid = lambda sizes: [[v // 2 for v in D._Window(s, (crop, crop)).slack()] for s in sizes]                  # noqa: E731
    mirror = [k % 2 for k in range(n)]
    nbytes, plain = I.layout_train_f(shapes, [m[0] for m in mid(shapes)], [m[1] for m in mid(shapes)], mirror)
    sbytes, desc = I.layout_train_f(shapes, [m[0] for m in mid(scaled)], [m[1] for m in mid(scaled)], mirror, scaled)
    assert sbytes == nbytes
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_f(buf, plain, images, labs)
    stage = torch.from_numpy(buf).cuda()
    out = ops.train_f_input_batch(stage, plain, (crop, crop), MEAN)
    sout = ops.train_f_input_batch(stage, desc, (crop, crop), MEAN)
    sizes = dict(crop=crop, images=n, staging_bytes=nbytes, output_bytes=sum(o.numel() * 4 for o in out), scaled_sizes=scaled)
    return (lambda: ops.train_f_input_batch(stage, plain, (crop, crop), MEAN, out=out),
            lambda: ops.train_f_input_batch(stage, desc, (crop, crop), MEAN, out=sout), sizes)


def probe_e(p):
    run_f, run_scaled, sizes = _scaled_calls(p)
    us = [[], []]
    for _ in range(3):                                                    # the sides alternating
        us[0].append(round(_median_us(run_f, reps=200), 2))
        us[1].append(round(_median_us(run_scaled, reps=200), 2))
    print("(e) back-to-back calls at crop 513, 10 images, device events (an UPPER BOUND on kernel time): unscaled %s us, scaled "
          "(factors %s) %s us; %d staging bytes -> %d output bytes either way"
          % (us[0], list(SCALE_FACTORS), us[1], sizes["staging_bytes"], sizes["output_bytes"]), flush=True)
    return dict(train_f_call_us=us[0], train_f_scaled_call_us=us[1], **sizes)


def probe_j(p, launches=200):
    """the unscaled and the scaled stage-2 launch at crop 513 alone, 200 times each, for a trace as in mode k"""
    run_f, run_scaled, sizes = _scaled_calls(p)
    for _ in range(launches):
        run_f()
        run_scaled()
    torch.cuda.synchronize()
    return dict(launches_each=launches, **sizes)


def probe_f(p, workers=8, crop=513):
    """TrainFInput at batch 10 / crop 513 without and with scale factors, alternating windows of 60 batches in one process"""
    from dsrg_amd.input import TrainFInput
    mk = lambda factors: TrainFInput(dict(source=p["f"], root_folder=p["root"], batch_size=10, crop_size=(crop, crop), mean=MEAN,      # noqa: E731
                                          mirror=True, scale_factors=factors), workers=workers)
    with mk(()) as plain, mk(SCALE_FACTORS) as scaled:
        _window(plain, 3), _window(scaled, 3)
        rp, rs = [], []
        for _ in range(3):
            rp.append(round(_window(plain, 60), 1))
            rs.append(round(_window(scaled, 60), 1))
    print("(f) TrainFInput at crop %d, batch 10, %d threads: %s images/s without factors, %s images/s with %s"
          % (crop, workers, rp, rs, list(SCALE_FACTORS)), flush=True)
    return dict(train_f_images_per_s=rp, train_f_scaled_images_per_s=rs, workers=workers, crop=crop)


def probe_c(p, steps=50):
    from dsrg_amd.trainer import DSRGTrainer
    mk_s, _ = _loaders(p)
    dev = torch.device("cuda", torch.cuda.current_device())
    tr = DSRGTrainer(dev)
    with mk_s() as ld:
        resident = [t.clone() for t in next(ld)]
        for _ in range(3):
            tr.step(*resident)
            tr.step(*next(ld))

        def window(fed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(*(next(ld) if fed else resident))
            torch.cuda.synchronize()
            return steps * 20 / (time.perf_counter() - t0)
        res, fed = [], []
        for _ in range(3):
            res.append(round(window(False), 1))
            fed.append(round(window(True), 1))
    r = dict(step_images_per_s_resident=res, step_images_per_s_fed_by_loader=fed,
             ratio_of_medians=round(float(np.median(fed) / np.median(res)), 3))
    print("(c) DSRGTrainer.step, windows of %d steps: %s images/s fed by TrainSInput against %s on resident tensors -> x%.3f"
          % (steps, fed, res, r["ratio_of_medians"]), flush=True)
    return r


def _resize_numpy(src, S):
    """the 8-bit bilinear resize of DESIGN.md in numpy (the restatement tests/test_train_input.py checks the kernel against)"""
    def taps(n, zero):
        f = ((np.arange(S, dtype=np.float64) + 0.5) * (1.0 / (float(S) / float(n))) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(np.float32)).astype(np.float32)
        if zero:
            f = np.where((s < 0) | (s >= n - 1), np.float32(0.0), f).astype(np.float32)
            s = np.clip(s, 0, n - 1)
        return s, np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int32), np.rint(f * np.float32(2048.0)).astype(np.int32)
    H, W = src.shape[:2]
    sx, a0, a1 = taps(W, True)
    sy, b0, b1 = taps(H, False)
    p = src.astype(np.int32)
    D = p[:, sx, :] * a0[None, :, None] + p[:, np.minimum(sx + 1, W - 1), :] * a1[None, :, None]
    D0, D1 = D[np.clip(sy, 0, H - 1)], D[np.clip(sy + 1, 0, H - 1)]
    return (((b0[:, None, None] * (D0 >> 4)) >> 16) + ((b1[:, None, None] * (D1 >> 4)) >> 16) + 2) >> 2


def probe_d(p):
    import pylayers

    class Blob(object):
        def __init__(self, a=None):
            self.data = a if a is not None else np.zeros((0,), np.float32)

        def reshape(self, *s):
            self.data = np.zeros(s, np.float32)
    images, _, _ = _s_batch(p)
    lay = pylayers.AnnotationLayer()
    lay.param_str = "{'cues': %r, 'mirror': True}" % p["cues"]
    ids = Blob(np.arange(20, dtype=np.float32).reshape(20, 1, 1, 1))
    mean = np.asarray(MEAN, np.float32)[:, None, None]

    def host():
        x = np.stack([_resize_numpy(im, 321)[:, :, ::-1].transpose(2, 0, 1).astype(np.float32) - mean for im in images])
        bottoms, tops = [ids, Blob(x)], [Blob(), Blob(), Blob()]
        lay.setup(bottoms, tops)
        lay.reshape(bottoms, tops)
        lay.forward(bottoms, tops)
        out = [torch.from_numpy(t.data).cuda() for t in tops]
        torch.cuda.synchronize()
        return out
    host()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        host()
        t.append((time.perf_counter() - t0) * 1e3)
    r = dict(host_composition_ms_per_batch_of_20=[round(v, 1) for v in t], images_per_s=round(20e3 / float(np.median(t)), 1))
    print("(d) host composition (numpy resize -> AnnotationLayer -> float32 upload, files already decoded): %s ms per batch of 20 -> "
          "%.1f images/s" % (r["host_composition_ms_per_batch_of_20"], r["images_per_s"]), flush=True)
    return r


def _cuemap_files(p, C=81):
    """a 41 x 41 cue PNG (classes below C, a third 255) per image of _files and the 'image_path cue_path' list"""
    from PIL import Image
    rng = np.random.default_rng(78)
    lines = []
    for k in range(N_FILES):
        cue = rng.integers(0, C, (41, 41)).astype(np.uint8)
        cue[rng.random((41, 41)) < 0.33] = 255
        Image.fromarray(cue, mode="L").save(os.path.join(p["root"], "cue%d.png" % k))
        lines.append("/im%d.jpg /cue%d.png\n" % (k, k))
    path = os.path.join(p["root"], "cuemap.txt")
    open(path, "w").write("".join(lines))
    return path


def probe_m(p, B=20, C=81, steps=30):
    from dsrg_amd import input as I, layers, ops
    from dsrg_amd.trainer import DSRGTrainer
    lst = _cuemap_files(p, C)
    out = {}
    # the launch alone
    images = [I.read_rgb(os.path.join(p["root"], "im%d.jpg" % k)) for k in range(B)]
    maps = [I.read_gray(os.path.join(p["root"], "cue%d.png" % k)) for k in range(B)]
    nbytes, desc = I.layout_train_s_cuemap([im.shape[:2] for im in images], (41, 41), [k % 2 for k in range(B)])
    buf = np.zeros(nbytes, np.uint8)
    I.pack_train_s_cuemap(buf, desc, images, maps)
    stage = torch.from_numpy(buf).cuda()
    res = ops.train_s_cuemap_input_batch(stage, desc, 321, C, (41, 41), MEAN)
    call = lambda: ops.train_s_cuemap_input_batch(stage, desc, 321, C, (41, 41), MEAN, out=res)      # noqa: E731
    us = [round(_median_us(call, reps=200), 2) for _ in range(3)]
    out.update(cuemap_call_us=us, staging_bytes=nbytes, output_bytes=sum(o.numel() * 4 for o in res))
    print("(m) back-to-back train_s_cuemap_input_batch calls, %d images, C = %d, device events (an UPPER BOUND on kernel time): %s us "
          "(%d staging bytes -> %d output bytes)" % (B, C, us, nbytes, out["output_bytes"]), flush=True)

    # the host composition the launch replaces
    class Blob(object):
        def reshape(self, *s):
            self.data = np.zeros(s, np.float32)
    lay = layers.AnnotationLayerCOCO()
    lay.param_str = repr({'source': lst, 'root': p["root"], 'batch_size': B, 'mean': MEAN, 'new_size': (321, 321), 'mirror': True})
    tops = [Blob(), Blob(), Blob()]
    lay.setup([], tops)

    def host_files():
        lay.forward([], tops)                                            # load_next_image x B: decode, zoom, scatter
        dev = [torch.from_numpy(t.data).cuda() for t in tops]
        torch.cuda.synchronize()
        return dev

    def host_decoded():
        parts = [lay.preprocess(im[:, :, ::-1], cue) for im, cue in zip(images, maps)]
        dev = [torch.from_numpy(np.stack([np.asarray(q[i], dtype=np.float32) for q in parts])).cuda() for i in range(3)]
        torch.cuda.synchronize()
        return dev
    for name, fn in (("host_composition_ms", host_files), ("host_composition_decoded_ms", host_decoded)):
        fn()
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            t.append(round((time.perf_counter() - t0) * 1e3, 1))
        out[name] = t
    print("(m) host composition per batch of %d (AnnotationLayerCOCO.load_next_image x %d + 3 uploads): %s ms; files already decoded "
          "(preprocess x %d + uploads): %s ms" % (B, B, out["host_composition_ms"], B, out["host_composition_decoded_ms"]), flush=True)

    # the step at C = 81 fed by the loader against resident tensors; the C = 81 step next to the C = 21 step
    dev = torch.device("cuda", torch.cuda.current_device())
    tr81, tr21 = DSRGTrainer(dev, num_classes=C), DSRGTrainer(dev)
    mk_s, _ = _loaders(p)
    with I.TrainSCueMapInput(lst, p["root"], C, batch_size=B, workers=8) as ld, mk_s() as ld21:
        resident = [t.clone() for t in next(ld)]
        resident21 = [t.clone() for t in next(ld21)]
        for _ in range(3):
            tr81.step(*resident)
            tr81.step(*next(ld))
            tr21.step(*resident21)

        def window(tr, feed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(*feed())
            torch.cuda.synchronize()
            return round(steps * B / (time.perf_counter() - t0), 1)
        r81, fed, r21 = [], [], []
        for _ in range(3):
            r81.append(window(tr81, lambda: resident))
            fed.append(window(tr81, lambda: next(ld)))
            r21.append(window(tr21, lambda: resident21))
    out.update(step81_images_per_s_resident=r81, step81_images_per_s_fed_by_loader=fed, step21_images_per_s_resident=r21,
               fed_over_resident=round(float(np.median(fed) / np.median(r81)), 3),
               c81_over_c21=round(float(np.median(r81) / np.median(r21)), 3))
    print("(m) DSRGTrainer.step, batch %d, windows of %d steps, alternating: C = %d fed by TrainSCueMapInput %s images/s, C = %d on "
          "resident tensors %s images/s -> x%.3f; C = 21 on resident tensors %s images/s -> C = %d runs at x%.3f of C = 21"
          % (B, steps, C, fed, C, r81, out["fed_over_resident"], r21, C, out["c81_over_c21"]), flush=True)
    return out


def main(which):
    from dsrg_amd import _lib
    _lib.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "files": N_FILES}
    with tempfile.TemporaryDirectory() as d:
        p = _files(d)
        for key, fn in (("k", probe_k), ("j", probe_j), ("b", probe_b), ("e", probe_e), ("d", probe_d), ("a", probe_a), ("f", probe_f),
                        ("c", probe_c), ("m", probe_m)):
            if key in which:
                out[key] = fn(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or ["a", "b", "c", "d"])
