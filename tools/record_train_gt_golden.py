#!/usr/bin/env python
"""Record the outputs of ops.train_gt_unary_batch into tests/golden/train_gt_parent_outputs.npz.

Run on the MI355X in a checkout of commit 7a9e6b3, the last one whose train_gt_unary_batch ran kernels of its own
(train_gt_softmax_kernel / train_gt_zoom_kernel).  Since then train_gt_unary_batch is the ensemble's K = 1, no-flip case, and a test
of one against the other compares a kernel with itself: tests/test_train_gt.py and tests/test_train_gt_ms.py hold both to this file.

The cases are the loop of test_one_size_without_flip_is_train_gt_unary_batch_bit_for_bit, restated here with its seeds (one numpy
generator per G, seed 100 + G, drawn from in the test's order): maps (4,5) (6,6) (9,7) (1,3), outputs (9,13) (1,1) (33,2) (17,23),
C in (5, 21, 96), G in (1, 3, 16), both ignore_below settings, the lists of that file's _lists.  Inputs are not stored: the file
holds the case parameters, the sha256 of every input, the sha256 of the raw bytes of every output, and for C = 5 the outputs
themselves, so that a mismatch can be located.  The recorder also asserts that train_gt_ensemble_batch([scores], ...) gives the same
digests.

usage: python tools/record_train_gt_golden.py [--out FILE]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

MAPS = [(4, 5), (6, 6), (9, 7), (1, 3)]
OUT = [(9, 13), (1, 1), (33, 2), (17, 23)]
CS = (5, 21, 96)
GS = (1, 3, 16)
NAMES = ("probs", "unary", "labels")
EPS = 1e-5
STORED_C = 5


def batched_scores(rng, Gcap, C, h, w, kind):
    """_batched_scores of tests/test_ms_batched.py, on the host"""
    if kind == 0:
        a = rng.standard_normal((Gcap, C, h, w)) * 3.0
    elif kind == 1:
        a = rng.uniform(-300.0, 300.0, size=(Gcap, C, h, w))
    else:
        a = rng.integers(-2, 3, size=(Gcap, C, h, w)) * 150.0
    return a.astype(np.float32)


def lists(rng, G, C):
    """_lists of tests/test_train_gt_ms.py"""
    out = [[int(c) for c in rng.integers(0, C, size=int(rng.integers(1, 5)))] for _ in range(G)]
    out[0] = [C - 1, 0, 2, C - 1]
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(argv):
    out_path = os.path.join(ROOT, "tests", "golden", "train_gt_parent_outputs.npz")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    from dsrg_amd import _lib, ops
    _lib.require_gpu()
    cases, arrays = {}, {}
    for G in GS:
        rng = np.random.default_rng(100 + G)
        case = 0
        for C in CS:
            for h, w in MAPS:
                case += 1
                host = batched_scores(rng, G + case % 2, C, h, w, case % 3)
                scores = torch.from_numpy(host).cuda()
                shapes = [OUT[(case + g) % len(OUT)] for g in range(G)]
                select = lists(rng, G, C)
                t = (None, 0.5)[case % 2]
                got = ops.train_gt_unary_batch(scores, shapes, eps=EPS, want=NAMES, select=select, ignore_below=t)
                twin = ops.train_gt_ensemble_batch([scores], shapes, eps=EPS, want=NAMES, select=select, ignore_below=t)
                key = "G%d/case%d" % (G, case)
                sha = {}
                for g in range(G):
                    for n, a, b in zip(NAMES, got[g], twin[g]):
                        a = a.cpu().numpy()
                        sha["%d/%s" % (g, n)] = digest(a)
                        assert digest(b.cpu().numpy()) == sha["%d/%s" % (g, n)], "train_gt_ensemble_batch differs: %s image %d %s" % (
                            key, g, n)
                        if C == STORED_C:
                            arrays["%s/%d/%s" % (key, g, n)] = a
                cases[key] = dict(seed=100 + G, G=G, Gcap=G + case % 2, C=C, map=[h, w], kind=case % 3, shapes=shapes, select=select,
                                  ignore_below=t, eps=EPS, scores_sha256=digest(host), sha256=sha)
    meta = dict(commit="7a9e6b3", hip=torch.version.hip, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                stored_arrays="C == %d" % STORED_C, cases=cases)
    np.savez_compressed(out_path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print("%d cases, %d stored arrays, %d bytes -> %s (HIP %s, %s)" % (len(cases), len(arrays), os.path.getsize(out_path), out_path,
                                                                      meta["hip"], meta["device"]))


if __name__ == "__main__":
    main(sys.argv[1:])
