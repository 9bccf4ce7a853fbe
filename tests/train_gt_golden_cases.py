"""tests/golden/train_gt_parent_outputs.npz: the outputs of ops.train_gt_unary_batch at commit 7a9e6b3, the last one whose kernels
for one map per image were their own (tools/record_train_gt_golden.py, which see for the cases: the loop of
test_one_size_without_flip_is_train_gt_unary_batch_bit_for_bit).  Since then train_gt_unary_batch and train_gt_ensemble_batch at one
size run the same kernels, so a test of one against the other proves nothing alone: both are held to this record."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

NAMES = ("probs", "unary", "labels")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_gt_parent_outputs.npz")


@functools.lru_cache(maxsize=None)
def _load():
    z = np.load(_PATH)
    return json.loads(str(z["meta"])), z


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def assert_recorded(who, G, case, scores, outputs):
    """outputs: per image the (probs, unary, labels) tensors that `who` returned for case `case` of the loop at group size G.
    Every output must have the recorded sha256 of its raw bytes, and equal the recorded array where one is stored (C = 5)"""
    meta, z = _load()
    key = "G%d/case%d" % (G, case)
    rec = meta["cases"][key]
    assert _sha(scores.cpu().numpy()) == rec["scores_sha256"], "%s: the test no longer builds the recorded inputs" % key
    assert len(outputs) == rec["G"]
    env = "recorded at %s with HIP %s on %s; running HIP %s on %s" % (meta["commit"], meta["hip"], meta["device"], torch.version.hip,
                                                                      torch.cuda.get_device_name(0))
    for g, out in enumerate(outputs):
        for n, a in zip(NAMES, out):
            a = a.cpu().numpy()
            stored = "%s/%d/%s" % (key, g, n)
            if stored in z.files:
                want = z[stored]
                assert a.shape == want.shape and a.dtype == want.dtype, (who, stored)
                assert np.array_equal(a, want), "%s: %s differs from the recorded array in %d of %d values, first at %s (%s)" % (
                    who, stored, int((a != want).sum()), a.size, tuple(np.argwhere(a != want)[0]), env)
            assert _sha(a) == rec["sha256"]["%d/%s" % (g, n)], "%s: %s of image %d of %s (C %d, map %s, output %s) differs from the " \
                "recorded digest (%s)" % (who, n, g, key, rec["C"], rec["map"], rec["shapes"][g], env)
