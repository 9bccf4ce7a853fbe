"""Do the test-time entry points of dsrg_amd/inference.py give the same outputs, through the same launches, in two trees?

    python tools/inference_paths_diff.py dump DIR                      # in each tree, a fresh process per dump
    python tools/inference_paths_diff.py compare DIR_A DIR_B [--rerun DIR_A2] [--out FILE]

dump: a seeded ColumnNet (tests/test_flip_tta.py) on the six _E2E_SHAPES images through every public entry point over a matrix of
options (eager and through a GraphedForward where the entry point takes one); each configuration goes to DIR/<configuration>.pt:
  out.<i>   the i-th output (a mask, or the summed scores of _relative_unary)
  calls     per ops wrapper of the multiscale, preprocess and train-gt kernels: [calls, calls that were given out= buffers]
  keys      the sorted keys of the GraphedForward afterwards
compare: every entry of DIR_B against DIR_A, tensors with torch.equal, the rest with ==.  --rerun names a second dump of tree A,
the run-to-run control: an entry that differs between A's own two runs is no valid witness and is marked so; B is still held to
A's first run.  Exit status 1 if anything differs between A and B."""
import argparse
import itertools
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "2")        # as tests/conftest.py: MIOpen's heuristic pick, no ~50 s search per new shape

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

WRAPPERS = ("multiscale_unary", "multiscale_unary_batch", "multiscale_unary_mirror_batch", "preprocess_ms_batch",
            "preprocess_rect_batch", "preprocess_rect_mirror_batch", "train_gt_unary_batch", "train_gt_ensemble_batch")


def _count_calls(ops, counts):
    """wrap the ops wrappers (inference looks them up at every call) so that they count into `counts`"""
    def counted(name, fn):
        def wrapper(*args, **kw):
            c = counts.setdefault(name, [0, 0])
            c[0] += 1
            c[1] += kw.get("out") is not None
            return fn(*args, **kw)
        return wrapper

    for name in WRAPPERS:
        setattr(ops, name, counted(name, getattr(ops, name)))


def _configurations(net):
    """yields (name, callable(forward) -> list of arrays / tensors, takes a GraphedForward?)"""
    from dsrg_amd import inference as I
    from test_flip_tta import _E2E_SCALES as SCALES, _E2E_SIZES as SIZES, _e2e_images
    ims = _e2e_images(97)
    labelled = [(im, [1 + k % 5, 7 + k]) for k, im in enumerate(ims)]
    tf = (False, True)
    for smooth, flip in itertools.product(tf, tf):
        tag = "smooth%d.flip%d" % (smooth, flip)
        yield "mask_ms." + tag, lambda f, s=smooth, fl=flip: [I.predict_mask_ms(net, im, smooth=s, sizes=SIZES, forward=f, flip=fl)
                                                              for im in ims], True
        for fused in tf:
            yield "mask_ms_f.%s.fused%d" % (tag, fused), lambda f, s=smooth, fl=flip, fu=fused: [
                I.predict_mask_ms_f(net, im, scales=SCALES, smooth=s, forward=f, fused=fu, flip=fl) for im in ims], True
        yield "ms_batched." + tag, lambda f, s=smooth, fl=flip: (
            I.predict_masks_ms_batched(net, ims[:4], smooth=s, sizes=SIZES, forward=f, flip=fl) +
            I.predict_masks_ms_batched(net, ims[4:], smooth=s, sizes=SIZES, forward=f, capacity=4, flip=fl)), True
        for G in (1, 3):
            yield "ms_f_many.G%d.%s" % (G, tag), lambda f, s=smooth, fl=flip, G=G: list(
                I.predict_masks_ms_f_many(net, iter(ims), scales=SCALES, forward=f, in_flight=2, batch=2, same_size_batch=G,
                                          smooth=s, flip=fl)), True
    for G, flip in itertools.product((1, 4), tf):
        yield "ms_many.G%d.flip%d" % (G, flip), lambda f, G=G, fl=flip: list(
            I.predict_masks_ms_many(net, iter(ims), sizes=SIZES, forward=f, in_flight=2, batch=2, forward_batch=G, flip=fl)), True
    for G, smooth in itertools.product((1, 4), tf):
        yield "train_gt_many.G%d.smooth%d" % (G, smooth), lambda f, G=G, s=smooth: list(
            I.predict_train_gt_many(net, iter(labelled), smooth=s, size=SIZES[1], forward=f, in_flight=2, forward_batch=G)), True
    for fused, flip in itertools.product(tf, tf):
        yield "relative_unary_sum.fused%d.flip%d" % (fused, flip), lambda f, fu=fused, fl=flip: [
            I._relative_unary(net, im, SCALES, "cuda", f, fu, True, flip=fl, want="sum") for im in ims], False


def dump(directory):
    from dsrg_amd import inference as I, ops
    os.makedirs(directory, exist_ok=True)
    from test_flip_tta import ColumnNet
    counts = {}
    _count_calls(ops, counts)
    net = ColumnNet(seed=3).cuda().eval()
    for name, run, takes_forward in _configurations(net):
        for graphed in (False, True) if takes_forward else (False,):
            counts.clear()
            fwd = I.GraphedForward(net) if graphed else None
            with torch.no_grad():
                outs = run(fwd)
            torch.cuda.synchronize()
            entry = {"out.%d" % i: torch.as_tensor(np.asarray(o.cpu() if torch.is_tensor(o) else o)).clone() for i, o in enumerate(outs)}
            entry["calls"] = {k: list(v) for k, v in sorted(counts.items())}
            entry["keys"] = sorted(repr(k) for k in fwd._g) if graphed else []
            full = "%s.%s" % (name, "graphed" if graphed else "eager")
            torch.save(entry, os.path.join(directory, full + ".pt"))
            print("dumped %-48s %2d outputs, calls %s, %d graphs" % (full, len(outs), entry["calls"], len(entry["keys"])), flush=True)


def _same(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return (not torch.is_tensor(a)) and (not torch.is_tensor(b)) and a == b


def _describe(v):
    return "%s %s" % (str(v.dtype).replace("torch.", ""), tuple(v.shape)) if torch.is_tensor(v) else repr(v)


def compare(dir_a, dir_b, rerun, out):
    lines, bad, noisy, total = [], 0, 0, 0
    for f in sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b))):
        if not (os.path.exists(os.path.join(dir_a, f)) and os.path.exists(os.path.join(dir_b, f))):
            lines.append("MISSING   %s in one of the two dumps" % f)
            bad += 1
            continue
        a, b = torch.load(os.path.join(dir_a, f)), torch.load(os.path.join(dir_b, f))
        a2 = torch.load(os.path.join(rerun, f)) if rerun else None
        for key in sorted(set(a) | set(b)):
            what = "%s:%s" % (f[:-3], key)
            total += 1
            if key not in a or key not in b:
                lines.append("MISSING   %s in one of the two dumps" % what)
                bad += 1
                continue
            same = _same(a[key], b[key])
            own = a2 is None or (key in a2 and _same(a[key], a2[key]))
            note = "" if own else "  [A's own two runs differ here: no valid witness]"
            noisy += 0 if own else 1
            bad += 0 if same else 1
            lines.append("%s %-64s %s%s" % ("identical" if same else "DIFFERENT", what, _describe(a[key]), note))
    lines.append("# %d entries, %d differ between A and B, %d differ between A's own two runs" % (total, bad, noisy))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    sub.add_parser("dump").add_argument("dir")
    c = sub.add_parser("compare")
    c.add_argument("dir_a")
    c.add_argument("dir_b")
    c.add_argument("--rerun", default=None)
    c.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.exit(dump(args.dir) if args.mode == "dump" else compare(args.dir_a, args.dir_b, args.rerun, args.out))
