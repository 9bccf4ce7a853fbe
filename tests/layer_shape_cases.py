"""Generated inputs for tests/test_gpu_layer_shapes.py: the stand-alone layer kernels of csrc/layers.hip away from the
21-label 41x41 blob — one label, fewer labels than the four lanes of a pixel, both sides of the 21 / 96-label template
switch, C * HW on either side of the seed-loss walk's 4 x 1024 stride, B * HW far from a multiple of 64 or 256."""
import functools

import numpy as np

SHAPES = [(1, 1, 1, 1), (3, 2, 1, 5), (2, 3, 7, 9), (1, 4, 8, 8), (2, 5, 3, 21), (1, 20, 9, 7), (2, 22, 9, 7), (1, 23, 16, 16),
          (2, 64, 5, 13), (1, 95, 4, 16), (3, 96, 6, 11),
          (1, 21, 13, 15), (1, 16, 16, 16), (1, 17, 241, 1),          # C * HW = 4095, 4096, 4097
          (257, 2, 1, 1)]
SPREADS = (1.0, 10.0, 40.0)
# the noise added to the logits before the second softmax that gives log q: 8 as in test_losses_forward_backward, wider where
# that clips under 1 % of the constrain-loss terms (clipped shares: the docstring of test_constrain_loss_clips_enough)
NOISE = {(1, 95, 4, 16): 16.0, (3, 96, 6, 11): 16.0}


def ids(shapes=SHAPES):
    return ["%dx%dx%dx%d" % s for s in shapes]


def spread_of(shape):
    return SPREADS[SHAPES.index(shape) % 3]


@functools.lru_cache(maxsize=None)
def inputs(shape, spread=None):
    """-> dict: logits (normal, times the spread), g (a top gradient), cues (random at 20 %; image 1 without a background cue,
    image 2 without a foreground cue: the max(count, 1e-4) guards), noise (normal, for log q)"""
    B, C, H, W = shape
    spread = spread_of(shape) if spread is None else spread
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + int(spread))
    d = {"logits": (rng.standard_normal(shape) * spread).astype(np.float32),
         "g": rng.standard_normal(shape).astype(np.float32),
         "cues": (rng.random(shape) < 0.2).astype(np.float32),
         "noise": rng.standard_normal(shape) * NOISE.get(shape, 8.0)}
    if B > 1:
        d["cues"][1, 0] = 0.0
    if B > 2:
        d["cues"][2, 1:] = 0.0
    for a in d.values():
        a.setflags(write=False)
    return d


def logq_of(O, d, p):
    """the logarithm of the oracle's softmax of logits + noise, float32; p is not used beyond its shape"""
    return np.log(O.softmax_forward((d["logits"] + d["noise"]).astype(np.float32))).astype(np.float32)


def clip_census(p, lq):
    """-> (r = q / p in float64, near: within rounding of an (inclusive) clip bound, clipped: outside [0.05, 20])"""
    r = np.exp(lq.astype(np.float64)) / p
    near = (np.abs(r - 0.05) <= 1e-5) | (np.abs(r - 20) <= 1e-3)
    return r, near, (r < 0.05) | (r > 20)
