"""Inputs shared by the tests of tests/test_gpu_crf_params.py: the dense CRF off its default kernel parameters.

A parameter set is the nine arguments of DenseCRF.add_pairwise_energy (w1, theta_alpha x / y, theta_beta r / g / b, w2, theta_gamma
x / y).  Every other CRF test of the suite draws them from one family (w = (10, 3), theta_alpha = 80 / s and theta_gamma = 3 / s with
x = y, theta_beta = 13 three times, s in {1, 3, 12}), in which a swap of x and y, a permutation of the colour widths and the pixel-
local Gaussian lattice near its boundary are invisible.  What the generator promises — that the two members of a mirrored pair give
different marginals, how many vertices the Gaussian lattices have and which of them are pixel-local — is asserted from the ORACLE in the file's CPU tests, never
from the kernels under test."""
import numpy as np

from dsrg_amd import synthetic as S

_A, _G = 80 / 12.0, 0.25

# tag -> (w1, alpha_x, alpha_y, beta_r, beta_g, beta_b, w2, gamma_x, gamma_y)
PARAMS = {
    "default12": (10, _A, _A, 13, 13, 13, 3, _G, _G),
    "alpha_xy": (10, 4, 9, 13, 13, 13, 3, _G, _G),
    "alpha_yx": (10, 9, 4, 13, 13, 13, 3, _G, _G),
    "beta_rgb": (10, 6.7, 6.7, 5, 13, 40, 3, _G, _G),
    "beta_bgr": (10, 6.7, 6.7, 40, 13, 5, 3, _G, _G),
    "gamma_xy": (10, 6.7, 6.7, 13, 13, 13, 3, _G, 3.0),
    "gamma_yx": (10, 6.7, 6.7, 13, 13, 13, 3, 3.0, _G),
    "gamma_0.4": (10, _A, _A, 13, 13, 13, 3, 0.4, 0.4),
    "gamma_0.5": (10, _A, _A, 13, 13, 13, 3, 0.5, 0.5),
    "gamma_0.7": (10, _A, _A, 13, 13, 13, 3, 0.7, 0.7),
    "weights": (4, 6.7, 6.7, 13, 13, 13, 7, 1.0, 2.0),
    "w1_zero": (0, _A, _A, 13, 13, 13, 3, _G, _G),
    "w2_zero": (10, _A, _A, 13, 13, 13, 0, _G, _G),
}
TAGS = list(PARAMS)
MIRRORS = [("alpha_xy", "alpha_yx"), ("beta_rgb", "beta_bgr"), ("gamma_xy", "gamma_yx")]
GAMMA_EDGE = ["gamma_0.4", "gamma_0.5", "gamma_0.7"]
# the sets whose mean field is also run for 0, 1 and 2 iterations: the default and one member of every mirrored pair
ITER_SWEEP = ["default12", "alpha_xy", "beta_rgb", "gamma_xy"]

SMALL = (23, 37)                # (H, W): odd, not square, N % 4 = 3
TRAIN = (41, 41)                # the training map
BEYOND = (71, 73)               # a plain one-image object just beyond the LDS-resident path


def images(HW, seed=0):
    """(2, H, W, 3) uint8: image 0 "smooth", image 1 "noise" """
    H, W = HW
    rng = np.random.default_rng(9100 + 100 * H + W + seed)
    out = []
    for kind in ("smooth", "noise"):
        img = S.make_images(rng, 1, size=max(H, W, 8), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
        out.append(np.transpose(img, (1, 2, 0)).astype(np.uint8))
    return np.ascontiguousarray(np.stack(out))


def unaries(HW, C, log=False, seed=0):
    """(2, H, W, C) float32 `unary` arguments of krahenbuhl2013.CRF (minus the energy), as test_crf_function_vs_oracle makes
    them: softmax of smooth logits floored at 1e-4, or its logarithm (the test-time call)"""
    from oracle import oracle as O
    H, W = HW
    rng = np.random.default_rng(9200 + 1000 * C + 100 * H + W + seed)
    un = np.maximum(O.softmax_forward(S.make_logits(rng, 2, C, H, W)), 1e-4)
    un = np.ascontiguousarray(np.transpose(un, (0, 2, 3, 1)))
    return np.log(un) if log else un


def log_unary(tag):
    """which sets run on log-probabilities: the ones with a wide spatial kernel, as the test-time call that uses such kernels"""
    return tag in ("weights", "gamma_xy", "gamma_yx", "gamma_0.7")


def field(HW, C, seed=0):
    """(2, C, H, W) float32: a valid marginal field per image"""
    from oracle import oracle as O
    H, W = HW
    rng = np.random.default_rng(9300 + 1000 * C + 100 * H + W + seed)
    return O.softmax_forward(S.make_logits(rng, 2, C, H, W, gain=8.0))


def oracle_crf(O, im, prm, C, unary=None):
    """the oracle's object for one image (H, W, 3); unary (H, W, C) as krahenbuhl2013.CRF takes it, None = no unary set"""
    H, W = im.shape[:2]
    oc = O.DenseCRF(W, H, C)
    if unary is not None:
        oc.set_unary_energy(-unary.ravel())
    oc.add_pairwise_energy(*prm, im.ravel())
    return oc


def pixel_local(oc):
    """whether the oracle's Gaussian lattice has the pixel-local form (lattice.hip: lattice_local_kernel): every vertex belongs to
    one pixel, every blur neighbour of a vertex belongs to the same pixel, and along each of the three axes exactly one of a
    pixel's vertices has a forward neighbour"""
    N = oc.W * oc.H
    off = oc.lattice_dump(0)[1][:N]
    n1, n2 = oc.lattice_neighbours(0)
    M = n1.shape[1]
    if M != 3 * N or np.unique(off).size != 3 * N:
        return False
    owner = np.empty(M, np.int64)
    owner[off.ravel()] = np.repeat(np.arange(N), 3)
    for nb in (n1, n2):
        has = nb >= 0
        if (owner[np.where(has, nb, 0)] != owner[None, :])[has].any():
            return False
    return all((np.bincount(owner[n2[j] >= 0], minlength=N) == 1).all() for j in range(3))


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())
