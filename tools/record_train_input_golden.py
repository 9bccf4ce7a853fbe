#!/usr/bin/env python
"""Record what the six staging functions of dsrg_amd/input.py (layout_train_s / pack_train_s, layout_train_s_cuemap /
pack_train_s_cuemap, layout_train_f / pack_train_f) make of a fixed set of batches into tests/golden/train_input_staging.json.
CPU only.

Run in a checkout of commit 4da5128, the last one in which each of the three pairs was a loop of its own; since then they are
statements over one layout and one put routine, and tests/test_train_input_staging.py holds them to this file field for field and
hash for hash.

Per case the file holds the case's parameters, `nbytes`, the descriptor, and the sha256 of a staging buffer of nbytes + 16 bytes
prefilled with 0xA5 and then packed: the prefill makes a write into the alignment gaps or past the end show.  Contents are not
stored: `contents` below draws them from np.random.default_rng(seed) in a fixed order, and the test restates it.  The cases are the
smallest that take every branch: one 1 x 1 image without triplets or class ids; three images whose byte counts are no multiples of
16, mixed mirrors, 0 / 5 / 1 triplets; 32 images of 2 x 2; cue maps of (1, 1) and (4, 6); stage 2 without and with `scaled`, with
non-zero top / left.

usage: python tools/record_train_input_golden.py [--out FILE]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ODD = [[4, 5], [5, 4], [1, 7]]                   # 60, 60 and 21 image bytes: none a multiple of 16
B32 = [[2, 2]] * 32
CASES = {
    "s/one_pixel": dict(kind="s", seed=1, shapes=[[1, 1]], ncues=[0], nlabels=[0], mirror=None),
    "s/odd_sizes": dict(kind="s", seed=2, shapes=ODD, ncues=[0, 5, 1], nlabels=[2, 0, 3], mirror=[1, 0, 1]),
    "s/batch_32": dict(kind="s", seed=3, shapes=B32, ncues=[k % 3 for k in range(32)], nlabels=[k % 2 for k in range(32)],
                       mirror=[k % 2 for k in range(32)]),
    "c/one_pixel": dict(kind="c", seed=4, shapes=[[1, 1]], map_size=[1, 1], mirror=None),
    "c/odd_sizes": dict(kind="c", seed=5, shapes=ODD, map_size=[4, 6], mirror=[0, 1, 1]),
    "c/batch_32": dict(kind="c", seed=6, shapes=B32, map_size=[4, 6], mirror=[(k // 2) % 2 for k in range(32)]),
    "f/one_pixel": dict(kind="f", seed=7, shapes=[[1, 1]], top=[0], left=[0], mirror=[0], scaled=None),
    "f/odd_sizes": dict(kind="f", seed=8, shapes=ODD, top=[3, 0, 7], left=[0, 2, 5], mirror=[1, 0, 1], scaled=None),
    "f/odd_sizes_scaled": dict(kind="f", seed=8, shapes=ODD, top=[3, 0, 7], left=[0, 2, 5], mirror=[1, 0, 1],
                               scaled=[[2, 3], [10, 8], [1, 1]]),
    "f/batch_32": dict(kind="f", seed=9, shapes=B32, top=[k % 5 for k in range(32)], left=[k % 3 for k in range(32)],
                       mirror=[k % 2 for k in range(32)], scaled=None),
}


def contents(case):
    """the pieces of a case, one list per piece: per image, in order, the image and then its further pieces"""
    rng = np.random.default_rng(case["seed"])
    pieces = ([], [], []) if case["kind"] == "s" else ([], [])
    for b, (H, W) in enumerate(case["shapes"]):
        pieces[0].append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        if case["kind"] == "s":
            pieces[1].append(rng.integers(0, 41, (3, case["ncues"][b])).astype(np.int32))
            pieces[2].append(rng.integers(0, 21, (case["nlabels"][b],)).astype(np.int32))
        elif case["kind"] == "c":
            pieces[1].append(rng.integers(0, 256, tuple(case["map_size"])).astype(np.uint8))
        else:
            pieces[1].append(rng.integers(0, 256, (H, W)).astype(np.uint8))
    return pieces


def stage(I, case):
    """-> (nbytes, desc, the packed buffer of nbytes + 16 bytes) of a case through the public functions of module I"""
    shapes = [tuple(s) for s in case["shapes"]]
    if case["kind"] == "s":
        (nbytes, desc), pack = I.layout_train_s(shapes, case["ncues"], case["nlabels"], case["mirror"]), I.pack_train_s
    elif case["kind"] == "c":
        (nbytes, desc), pack = I.layout_train_s_cuemap(shapes, tuple(case["map_size"]), case["mirror"]), I.pack_train_s_cuemap
    else:
        scaled = None if case["scaled"] is None else [tuple(s) for s in case["scaled"]]
        (nbytes, desc), pack = I.layout_train_f(shapes, case["top"], case["left"], case["mirror"], scaled), I.pack_train_f
    buf = np.full(nbytes + 16, 0xA5, np.uint8)
    pack(buf, desc, *contents(case))
    return nbytes, desc, buf


def main(argv):
    out_path = os.path.join(ROOT, "tests", "golden", "train_input_staging.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    from dsrg_amd import input as I
    cases = {}
    for name, case in CASES.items():
        nbytes, desc, buf = stage(I, case)
        cases[name] = dict(case, nbytes=nbytes, desc=desc, sha256=hashlib.sha256(buf.tobytes()).hexdigest())
    with open(out_path, "w") as f:
        json.dump(dict(commit="4da5128", prefill=0xA5, tail=16, cases=cases), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d bytes -> %s" % (len(cases), os.path.getsize(out_path), out_path))


if __name__ == "__main__":
    main(sys.argv[1:])
