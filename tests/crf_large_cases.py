"""Inputs shared by tests/test_oracle_splat_segments.py (CPU) and tests/test_gpu_crf_large.py (GPU): images on which the
global-memory dense CRF (dsrg_amd/csrc/lattice_large.hip) cuts vertex rows into segments, and natural ones on which it does not.

A case is (image (H,W,3) uint8, the nine pairwise parameters).  What each generator promises about row lengths is asserted
from the ORACLE's lattice in test_oracle_splat_segments.py, never from the kernel under test."""
import numpy as np

from dsrg_amd import synthetic as S

SEG = 4096                      # lattice_large.hip: kSplatSeg


def params(scale=1.0, theta_gamma=None):
    """krahenbuhl2013.CRF's parameters (CRF.py:27-35) at `scale`; theta_gamma overrides the spatial kernel's width"""
    tg = 3 / scale if theta_gamma is None else theta_gamma
    return (10, 80 / scale, 80 / scale, 13, 13, 13, 3, tg, tg)


def _synthetic(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    img = S.make_images(rng, 1, size=max(H, W, 8), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
    return np.ascontiguousarray(np.transpose(img, (1, 2, 0))).astype(np.uint8)


def constant(H, W, value=128):
    return np.full((H, W, 3), value, np.uint8)


def sky():
    """a 120x120 smooth image whose top 75 rows are saturated"""
    im = _synthetic("smooth", 120, 120, 7001)
    im[:75] = 255
    return im


# name -> (image, parameters, lattice that holds the long rows: 1 bilateral, 0 Gaussian)
def long_row_cases():
    return {
        "const66": (constant(66, 66), params(), 1),                  # fits the LDS path: through a forced-large object
        "const71": (constant(71, 71), params(), 1),
        "const100_255": (constant(100, 100, 255), params(), 1),
        "sky": (sky(), params(), 1),
        "gauss_wide": (_synthetic("noise", 90, 77, 7002), params(theta_gamma=60.0), 0),
    }


# name -> (image, parameters); no row above SEG
def natural_cases():
    return {
        "smooth24x31": (_synthetic("smooth", 24, 31, 7003), params()),          # the two below fit the LDS path: forced large
        "noise17x40": (_synthetic("noise", 17, 40, 7004), params(3.0)),
        "noise71x71": (_synthetic("noise", 71, 71, 7005), params(12.0)),
        "smooth101x123": (_synthetic("smooth", 101, 123, 7006), params()),      # N % 4 = 3: SSE padding pixel, phantom vertices
    }


def batch_case():
    """three 73x75 images (N % 4 = 3) for one batched object: flat, smooth, noise"""
    return np.stack([constant(73, 75, 200), _synthetic("smooth", 73, 75, 7007), _synthetic("noise", 73, 75, 7008)]), params()


def field(H, W, C, seed=0, gain=8.0):
    """a valid marginal field (N, C) float32, label-fastest"""
    from oracle import oracle as O
    rng = np.random.default_rng(100000 + 1000 * C + H * W + seed)
    q = O.softmax_forward(S.make_logits(rng, 1, C, H, W, gain=gain))[0]
    return np.ascontiguousarray(q.reshape(C, H * W).T)


def oracle_crf(O, im, prm, C):
    H, W = im.shape[:2]
    oc = O.DenseCRF(W, H, C)
    oc.add_pairwise_energy(*prm, im.ravel())
    return oc


def row_lengths(oc, k):
    """entries per vertex row of the oracle's lattice k"""
    return np.bincount(oc.lattice_dump(k)[1].ravel(), minlength=oc.lattice_size(k))


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())
