#!/usr/bin/env python
"""The ResNet-101 test-time path (dsrg_amd/resnet_test.py, csrc/resnet_stem.hip) against the module's own bf16 forward, on one MI355X.

  python tools/resnet_test_probe.py [--out profiles/resnet_test_probe.txt] [--workdir DIR]

runs two child processes one after the other, each under its own `timeout`, and stops at the first that fails:
  (t) --step time: ONE process, device events, the two sides alternating ROUNDS times (the spread is reported, not just a median):
        the fused stem kernel against the module's `stem` under autocast + no_grad at (1,3,401,401), (8,3,321,321), (1,3,513,513);
        the whole forward of ResNetTestNet against the module at batch 1 (401) and 8 (321), eager and through inference.GraphedForward;
        images/s of inference.predict_masks_ms_many (sizes 241, 321, 401, CRF on) at forward_batch 1 and 8, both sides.
  (l) --step launches under `rocprofv3 --kernel-trace` (a run of its own, the program after `--`): the kernel dispatches per eager
        forward of both sides at batch 8 (321), split by a marker launch (the stem's pack kernel, which no forward runs), and how
        many of them are `pack_conv_weight_kernel`; every kernel whose count differs between the sides is listed by name (the
        head's cat / pad copies among them).
Weights are seeded random numbers: times do not depend on them."""
import argparse
import glob
import os
import sqlite3
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ROUNDS = 5


def _setup():
    import torch
    from dsrg_amd import retrain as R
    from dsrg_amd.resnet_test import ResNetTestNet
    torch.manual_seed(0)
    net = R.ResNet101DeepLab()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, R._FrozenBN):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    net = net.cuda().to(memory_format=torch.channels_last).eval()
    return net, ResNetTestNet(net)


def _timed(fn, reps):
    """mean ms per call over `reps` calls between two device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _ab(name, sides, reps, warm=3):
    """sides: [(label, fn)]; warmed, then ROUNDS rounds alternating the sides -> one line with median [min .. max] per side"""
    for _, fn in sides:
        for _ in range(warm):
            fn()
    ms = {label: [] for label, _ in sides}
    for _ in range(ROUNDS):
        for label, fn in sides:
            ms[label].append(_timed(fn, reps))
    parts = ["%s %.3f ms [%.3f .. %.3f]" % (label, statistics.median(v), min(v), max(v)) for label, v in ms.items()]
    print("%-44s %s   (%d rounds x %d calls, alternating)" % (name, "   ".join(parts), ROUNDS, reps), flush=True)


def step_time():
    import numpy as np
    import torch
    from dsrg_amd import inference as I, ops
    net, w = _setup()
    amp = lambda: torch.autocast("cuda", dtype=torch.bfloat16)          # noqa: E731
    print("# stem: ops.resnet_stem against net.stem (library convolution, BatchNorm map, ReLU, max pool) under autocast + no_grad")
    scale, shift = net.stem[1].frozen_affine()
    packed = ops.resnet_stem_pack(net.stem[0].weight.detach(), scale)
    for shape in ((1, 3, 401, 401), (8, 3, 321, 321), (1, 3, 513, 513)):
        x = torch.randn(shape, device="cuda")

        def module_stem():
            with torch.no_grad(), amp():
                return net.stem(x)
        _ab("stem %s" % (shape,), [("module", module_stem), ("fused", lambda: ops.resnet_stem(x, packed, shift))], 50)
    print("# whole forward: ResNetTestNet against the module, eager and through inference.GraphedForward")
    for shape in ((1, 3, 401, 401), (8, 3, 321, 321)):
        x = torch.randn(shape, device="cuda")

        def eager(m):
            def run():
                with torch.no_grad(), amp():
                    return m(x)
            return run
        _ab("forward %s eager" % (shape,), [("module", eager(net)), ("wrapper", eager(w))], 10)
        with amp():
            g_net, g_w = I.GraphedForward(net), I.GraphedForward(w)

            def graphed(g):
                def run():
                    with amp():
                        return g(x)
                return run
            _ab("forward %s graphed" % (shape,), [("module", graphed(g_net)), ("wrapper", graphed(g_w))], 10)
    print("# inference.predict_masks_ms_many, sizes 241 / 321 / 401, CRF on, 48 images of 366 x 500 per pass")
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (366, 500, 3), dtype=np.uint8) for _ in range(8)] * 6
    for fb in (1, 8):
        sides = []
        with amp():
            for label, m in (("module", net), ("wrapper", w)):
                fwd = I.GraphedForward(m)
                for _ in I.predict_masks_ms_many(m, images[:16], device="cuda", forward=fwd, forward_batch=fb):   # captures
                    pass
                sides.append((label, m, fwd))
            rates = {label: [] for label, _, _ in sides}
            for _ in range(3):
                for label, m, fwd in sides:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = sum(1 for _ in I.predict_masks_ms_many(m, images, device="cuda", forward=fwd, forward_batch=fb))
                    torch.cuda.synchronize()
                    rates[label].append(n / (time.perf_counter() - t0))
        print("predict_masks_ms_many forward_batch %d:  %s   (3 passes, alternating)" % (
            fb, "   ".join("%s %.1f images/s [%.1f .. %.1f]" % (k, statistics.median(v), min(v), max(v)) for k, v in rates.items())), flush=True)


FORWARDS = 5


def step_launches():
    """under rocprofv3: warm-up | marker | FORWARDS module forwards | marker | FORWARDS wrapper forwards | marker"""
    import torch
    from dsrg_amd import ops
    net, w = _setup()
    x = torch.randn(8, 3, 321, 321, device="cuda")
    scale = torch.ones(64, device="cuda")
    marker = lambda: (torch.cuda.synchronize(), ops.resnet_stem_pack(net.stem[0].weight.detach(), scale), torch.cuda.synchronize())   # noqa: E731
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for m in (net, w):
            for _ in range(3):
                m(x)
        for m in (net, w):
            marker()
            for _ in range(FORWARDS):
                m(x)
        marker()


def count_launches(db):
    c = sqlite3.connect(db)
    tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    scol = [r[1] for r in c.execute("pragma table_info(%s)" % ks)]
    name_col = "kernel_name" if "kernel_name" in scol else "display_name"
    rows = sorted((st, name) for name, st in c.execute("select s.%s, d.start from %s d join %s s on d.kernel_id = s.id" % (name_col, kd, ks)))
    marks = [i for i, (_, name) in enumerate(rows) if "resnet_stem_pack_kernel" in name]
    if len(marks) < 3:
        raise SystemExit("expected at least 3 marker dispatches in %s, found %d" % (db, len(marks)))
    marks = marks[-3:]
    import collections
    sides = {}
    for label, lo, hi in (("module", marks[0], marks[1]), ("wrapper", marks[1], marks[2])):
        names = [name for _, name in rows[lo + 1:hi]]
        sides[label] = collections.Counter(names)
        print("launches per forward (8,3,321,321) eager, %-7s: %.1f kernel dispatches, of which pack_conv_weight_kernel %.1f, "
              "resnet_stem_kernel %.1f" % (label, len(names) / FORWARDS, sum(v for n, v in sides[label].items() if "pack_conv_weight_kernel" in n) / FORWARDS,
                                           sum(v for n, v in sides[label].items() if "resnet_stem_kernel" in n) / FORWARDS), flush=True)
    # no guess at what the library calls its cat / pad kernels: every kernel whose count differs between the sides, by name
    print("kernels whose dispatches per forward differ (module -> wrapper):")
    for n in sorted(set(sides["module"]) | set(sides["wrapper"]), key=lambda n: sides["wrapper"][n] - sides["module"][n]):
        if sides["module"][n] != sides["wrapper"][n]:
            print("  %6.1f -> %6.1f  %s" % (sides["module"][n] / FORWARDS, sides["wrapper"][n] / FORWARDS, n[:110]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--step", choices=("all", "time", "launches"), default="all")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_test_probe.txt"))
    p.add_argument("--workdir", default=None, help="where rocprofv3 writes its database (default: a new temporary directory)")
    a = p.parse_args()
    if a.workdir is None and a.step == "all":
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix="resnet_test_probe_")
    if a.step == "time":
        return step_time()
    if a.step == "launches":
        return step_launches()
    os.makedirs(a.workdir, exist_ok=True)
    me = os.path.abspath(__file__)
    steps = [["timeout", "-k", "10", "600", sys.executable, me, "--step", "time"],
             ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "-d", a.workdir, "-o", "launches", "--", sys.executable, me,
              "--step", "launches"]]
    text = ["# tools/resnet_test_probe.py on one MI355X; times by device events, median [min .. max] over alternating rounds\n"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for k, cmd in enumerate(steps):                                      # a failed step ends the probe: nothing more runs on the GPU
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.stderr.write(r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace")[-4000:])
            raise SystemExit("step %d (%s) ended with status %d" % (k, " ".join(cmd[4:8]), r.returncode))
        if k == 0:
            text.append(r.stdout.decode())
            with open(a.out, "w") as f:                                  # the times are kept whatever becomes of the trace
                f.write("".join(text))
    dbs = sorted(glob.glob(os.path.join(a.workdir, "**", "*_results.db"), recursive=True))     # rocprofv3 -o NAME writes NAME_results.db
    if not dbs:
        raise SystemExit("rocprofv3 left no *_results.db under %s: %s" % (a.workdir, sorted(os.listdir(a.workdir))))
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        print("# kernel dispatches per forward, from one rocprofv3 --kernel-trace run of its own")
        count_launches(dbs[-1])
    text.append(buf.getvalue())
    out = "".join(text)
    with open(a.out, "w") as f:
        f.write(out)
    sys.stdout.write(out)


if __name__ == "__main__":
    main()
