"""The dense CRF off its default kernel parameters and across rebuilds, HIP against the oracle (tests/crf_param_cases.py has the
parameter sets and says what the rest of the suite cannot see with its one family of parameters).

CPU (unmarked): what the generator promises, asserted from the oracle alone — the members of every mirrored pair give marginals
that differ by 100 times the contract, and the Gaussian lattices have the vertex counts that put them on, at and beyond the edge
of the pixel-local form.
GPU: 2. lattice structure id for id, 3. norm and one filter application to 2 ulp and the filter options bit for bit, 4. marginals
(the 1e-4 contract) and MAP labels after 0, 1, 2 and 10 iterations, 5. rebuilds on live contexts and objects, each on the
LDS-resident path (ops.Context, DenseCRF(W, H, C)) and on the global-memory path (DenseCRF(..., nimages=1 or 2), a 71x73 map).
The fused step off its defaults is in test_gpu_parity.py (test_fused_step_off_the_default_crf_arguments)."""
import ctypes

import numpy as np
import pytest
import torch

import crf_param_cases as K
from crf_param_cases import PARAMS, TAGS, ulps

gpu = pytest.mark.gpu

CRF_TOL = 1e-4           # north_star: "CRF marginals within 1e-4"
MIRROR_GAP = 1e-2        # 100 x the contract: a swapped width in a kernel cannot pass


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def planes(x):
    """(B, H, W, C) -> contiguous (B, C, H, W)"""
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


@pytest.fixture(scope="module")
def crf_mod():
    from dsrg_amd import crf, _lib
    _lib.require_gpu()
    return crf


class _Oracles(object):
    """the oracle's objects and results, computed once, shared by the tests and left unchanged"""

    def __init__(self, O):
        self.O, self._im, self._un, self._obj, self._run = O, {}, {}, {}, {}

    def images(self, HW):
        if HW not in self._im:
            self._im[HW] = K.images(HW)
        return self._im[HW]

    def unaries(self, tag, HW, C):
        key = (HW, C, K.log_unary(tag))
        if key not in self._un:
            self._un[key] = K.unaries(HW, C, K.log_unary(tag))
        return self._un[key]

    def crf(self, tag, HW, i):
        """lattices, norms and filters of image i (they do not depend on the label count)"""
        key = (tag, HW, i)
        if key not in self._obj:
            self._obj[key] = K.oracle_crf(self.O, self.images(HW)[i], PARAMS[tag], 1)
        return self._obj[key]

    def run(self, tag, HW, C, i, n, unary=True):
        """-> (marginals (H, W, C), MAP labels (H * W,)) after n iterations; unary False: none set (zero energies)"""
        key = (tag, HW, C, i, n, unary)
        if key not in self._run:
            oc = K.oracle_crf(self.O, self.images(HW)[i], PARAMS[tag], C, self.unaries(tag, HW, C)[i] if unary else None)
            self._run[key] = (oc.inference(n).reshape(HW + (C,)), oc.map(n))
        return self._run[key]


@pytest.fixture(scope="module")
def oracles(O):
    return _Oracles(O)


@pytest.fixture(scope="module")
def seen():
    """largest marginal deviation from the oracle per (path, parameter set), printed when the module is done"""
    worst = {}

    def note(path, tag, d):
        worst[(path, tag)] = max(worst.get((path, tag), 0.0), float(d))
    yield note
    for path in sorted({p for p, _ in worst}):
        print("\nmax|dQ| from the oracle, %s:" % path, ", ".join("%s %.2e" % (t, worst[(path, t)]) for t in TAGS if (path, t) in worst))


def prm(tag, n_iters):
    from dsrg_amd._lib import CrfParams
    return CrfParams(*PARAMS[tag], int(n_iters))


def gauss_dropped(ctx, B, C):
    """whether the launcher leaves the Gaussian workgroups out of the filter grid (the host found the lattice pixel-local), from
    filter_plan's workgroup count: bilateral workgroups alone, or those plus ceil(C / planes) Gaussian ones per image"""
    pb, pg, wgs, _ = ctx.filter_plan(B)
    groups_b, groups_g = -(-C // pb), -(-C // pg)
    stride = 8 if B < 8 else B & ~7
    nblk_b = groups_b * stride + (groups_b * (B - stride) if B > stride else 0)
    assert wgs in (nblk_b, nblk_b + groups_g * B), (pb, pg, wgs)
    return wgs == nblk_b


def cache_hits():
    """objects handed out from the library's cache of destroyed ones so far (a tests-only counter of the library)"""
    from dsrg_amd import _lib
    return _lib.lib().dsrg_debug_crf_cache_hits()


def flush_object_cache(crf_mod):
    """destroyed DenseCRF objects are parked, device buffers and all, in a cache of four slots and handed out again for the same
    shape; a destroy takes the first free slot and drops the oldest entry only when all four are taken.  Eight tiny objects of
    shapes no test uses, alive together and then destroyed: whatever the slots held before, the last four destroys have pushed it
    out, and the cache holds tiny objects alone."""
    tiny = [crf_mod.DenseCRF(2 + i, 2, 2) for i in range(8)]
    del tiny


def new_object(crf_mod, HW, C, nimages=None):
    """a DenseCRF that is newly made, not a parked one handed out again — asserted from the library's own count"""
    flush_object_cache(crf_mod)
    before = cache_hits()
    obj = crf_mod.DenseCRF(HW[1], HW[0], C, nimages=nimages)
    assert cache_hits() == before, "the object came from the cache"
    return obj


def run_object(crf_mod, HW, C, tag, im, un, n, nimages=None, newly_made=False):
    """inference and map of a new DenseCRF call sequence -> (marginals (..., H, W, C), labels (..., H, W), the object)"""
    H, W = HW
    obj = new_object(crf_mod, HW, C, nimages) if newly_made else crf_mod.DenseCRF(W, H, C, nimages=nimages)
    if un is not None:
        obj.set_unary_energy(-un.ravel())
    obj.add_pairwise_energy(*PARAMS[tag], im.ravel())
    lead = (nimages,) if nimages and nimages > 1 else ()
    return obj.inference(n).reshape(lead + (H, W, C)), obj.map(n).reshape(lead + (H, W)), obj


def check_marginals(q, lab, want_q, want_lab, what):
    """the 1e-4 contract, rows that sum to one, and MAP labels equal to the oracle's — a label may differ only where the oracle's
    own top two marginals are a near tie (test_crf_function_vs_oracle's rule).  Returns max|dQ|."""
    C = want_q.shape[-1]
    d = float(np.abs(q - want_q).max())
    print("%s: max|dQ| %.2e" % (what, d))
    assert q.dtype == np.float32 and np.isfinite(q).all() and np.abs(q.sum(-1) - 1).max() < 1e-5, what
    assert d < CRF_TOL, (what, d)
    lab, wq = np.asarray(lab).ravel(), want_q.reshape(-1, C)
    flip = np.flatnonzero(lab != np.asarray(want_lab).ravel())
    assert all(wq[i].max() - wq[i, int(lab[i])] < 1e-5 for i in flip), (what, len(flip))
    return d


# ---------------------------------------------------------------- 1. what the generator promises (CPU)
@pytest.mark.parametrize("a,b", K.MIRRORS)
def test_mirrored_parameter_sets_give_different_marginals(oracles, a, b):
    """swapping theta_alpha x / y, reversing theta_beta r / g / b, swapping theta_gamma x / y: the oracle's marginals move by at
    least 1e-2 on every image, label count and iteration count (>= 1) the GPU tests use (measured: 0.02 .. 0.96 after one
    iteration, 0.95 .. 1.0 after ten)"""
    for HW in (K.SMALL, K.TRAIN):
        for C in (5, 21):
            for i in (0, 1):
                for n in (1, 2, 10):
                    gap = np.abs(oracles.run(a, HW, C, i, n)[0] - oracles.run(b, HW, C, i, n)[0]).max()
                    assert gap >= MIRROR_GAP, (a, b, HW, C, i, n, gap)


def test_gaussian_lattices_sit_on_both_sides_of_the_pixel_local_form(oracles):
    """theta_gamma 0.25, 0.4 and 0.5 give exactly 3 N vertices (every vertex has one contributor: the pixel-local form is
    possible, the blur-neighbour condition decides), 0.7 a mixed lattice, the anisotropic sets a lattice shared along one axis;
    every lattice coordinate stays far inside the batched objects' +-2048"""
    for HW, counts in ((K.SMALL, {}), (K.TRAIN, {"gamma_0.7": 3823, "gamma_xy": 1215, "gamma_yx": 1066})):
        N = HW[0] * HW[1]
        for tag in TAGS:
            oc = oracles.crf(tag, HW, 0)
            mg = oc.lattice_size(0)
            if tag in ("gamma_0.7", "gamma_xy", "gamma_yx", "weights"):
                assert mg < 3 * N, (tag, HW, mg)
            else:
                assert mg == 3 * N, (tag, HW, mg)
            assert mg == counts.get(tag, mg), (tag, HW, mg)
            assert oracles.crf(tag, HW, 1).lattice_size(0) == mg                       # the Gaussian lattice knows no image
            # pixel-local: theta_gamma 0.25 alone — at 0.4 and 0.5 every vertex still has one contributor, but blur neighbours
            # reach into other pixels
            assert K.pixel_local(oc) == (PARAMS[tag][7:] == (0.25, 0.25)), (tag, HW)
            for k in (0, 1):
                assert np.abs(oc.lattice_dump(k)[0].astype(np.int32)).max() < 1024, (tag, HW, k)


# ---------------------------------------------------------------- 2. lattice structure
def same_lattice(got, oc, k, tag):
    """M, keys, per-pixel vertex ids and (bit for bit) weights, both neighbour tables: id for id, whole arrays"""
    keys, off, bary = oc.lattice_dump(k)
    n1, n2 = oc.lattice_neighbours(k)
    assert got["M"] == keys.shape[0], (tag, got["M"], keys.shape[0])
    assert np.array_equal(got["keys"], keys), tag
    assert np.array_equal(got["vid"], off), tag
    assert np.array_equal(got["bary"].view(np.uint32), bary.view(np.uint32)), tag
    assert np.array_equal(got["n1"], n1) and np.array_equal(got["n2"], n2), tag


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_lattice_structure_off_the_default_parameters(ops, crf_mod, oracles, tag):
    """Permutohedral::init of both lattices at 23x37 (x != y, N % 4 = 3) on a two-image context, on one-image objects forced to
    the global-memory path and on a two-image batched object, against the oracle: an x / y swap in the spatial widths or a
    permutation of the colour widths changes the keys"""
    HW, C = K.SMALL, 3
    H, W = HW
    ims = oracles.images(HW)
    ctx = ops.Context(2, C, H, W)
    ops.crf_meanfield(dev(planes(oracles.unaries(tag, HW, C))), dev(ims, torch.uint8), ctx=ctx, params=prm(tag, 0))
    same_lattice(ctx.lattice_dump(0, 0), oracles.crf(tag, HW, 0), 0, "%s context Gaussian" % tag)
    both = crf_mod.DenseCRF(W, H, C, nimages=2)
    both.add_pairwise_energy(*PARAMS[tag], ims.ravel())
    for i in (0, 1):
        oc = oracles.crf(tag, HW, i)
        same_lattice(ctx.lattice_dump(1, i), oc, 1, "%s context bilateral image %d" % (tag, i))
        one = crf_mod.DenseCRF(W, H, C, nimages=1)
        one.add_pairwise_energy(*PARAMS[tag], ims[i].ravel())
        for k in (0, 1):
            same_lattice(one.lattice_dump(k), oc, k, "%s forced-large image %d lattice %d" % (tag, i, k))
            same_lattice(both.lattice_dump(k, i), oc, k, "%s batched image %d lattice %d" % (tag, i, k))
            assert one.lattice_size(k) == oc.lattice_size(k)
    assert ctx.lattice_sizes(2) == (oracles.crf(tag, HW, 0).lattice_size(0), [oracles.crf(tag, HW, i).lattice_size(1) for i in (0, 1)])


# ---------------------------------------------------------------- 3. norm, one filter application, filter options
@gpu
@pytest.mark.parametrize("tag,C", [(t, c) for t in TAGS for c in (5, 21)] + [("default12", 2), ("gamma_xy", 2)])
def test_norm_and_single_filter_application_off_the_default_parameters(ops, crf_mod, oracles, seen, tag, C):
    """the normalisation vectors and ONE application of each normalised kernel within 2 ulp of the oracle (the bar of
    test_single_filter_application_and_norm_vs_oracle) on both paths; two labels take the reference's seqCompute arithmetic.
    Then ten iterations with the plain filter launch (options 0: the general form of the Gaussian message) and with the default
    options (the per-pixel form wherever the lattice is found pixel-local): bit-identical, whatever kLatticeLocal decided — and what
    it decided is what the oracle's tables say."""
    from dsrg_amd import _lib
    HW = K.SMALL
    H, W = HW
    N = H * W
    ims, q = oracles.images(HW), K.field(HW, C)
    ctx = ops.Context(2, C, H, W)
    ops.crf_meanfield(dev(q), dev(ims, torch.uint8), ctx=ctx, params=prm(tag, 1))       # builds the lattices of these images
    got = {k: ctx.filter_once(k, dev(q)).cpu().numpy() for k in (0, 1)}
    dropped = gauss_dropped(ctx, 2, C)
    print("%s C=%d: Gaussian lattice %s" % (tag, C, "pixel-local (its workgroups are left out of the filter grid)" if dropped
                                             else "general form"))
    # the form follows from the lattice alone: lattice_local_kernel's condition evaluated on the oracle's tables (two label planes
    # or fewer take seqCompute's arithmetic, which has no per-pixel form)
    assert dropped == (C > 2 and K.pixel_local(oracles.crf(tag, HW, 0))), (tag, C, dropped)
    for i in (0, 1):
        oc = oracles.crf(tag, HW, i)
        qlf = np.ascontiguousarray(q[i].reshape(C, N).T)                               # (N, C) label-fastest
        one = crf_mod.DenseCRF(W, H, C, nimages=1)
        one.add_pairwise_energy(*PARAMS[tag], ims[i].ravel())
        for k in (0, 1):
            what = "%s C=%d image %d kernel %d" % (tag, C, i, k)
            norm_o, want = oc.lattice_norm(k), oc.kernel_filter(k, qlf)
            assert (want > 0).all(), what
            assert ulps(ctx.lattice_norm(k, i if k == 1 else 0), norm_o) <= 2, what
            have = got[k][i].reshape(C, N).T
            assert ulps(have, want) <= 2, "%s context: %d ulp" % (what, ulps(have, want))
            assert ulps(one.lattice_norm(k), norm_o) <= 2, what
            have = one.filter_once(k, qlf)
            assert ulps(have, want) <= 2, "%s global path: %d ulp" % (what, ulps(have, want))
    un = dev(planes(oracles.unaries(tag, HW, C)))
    outs = {}
    L = _lib.lib()
    try:
        for opts in (0, -1):
            L.dsrg_debug_set_filter_opts(opts)
            outs[opts] = ops.crf_meanfield(un, dev(ims, torch.uint8), ctx=ops.Context(2, C, H, W), params=prm(tag, 10))
    finally:
        L.dsrg_debug_set_filter_opts(-1)
    assert torch.equal(outs[0], outs[-1]), "%s C=%d: the default filter options differ from the plain launch loop" % (tag, C)
    for i in (0, 1):
        have = np.transpose(outs[-1][i].cpu().numpy(), (1, 2, 0))
        d = float(np.abs(have - oracles.run(tag, HW, C, i, 10)[0]).max())
        seen("context of two images (LDS-resident)", tag, d)
        assert d < CRF_TOL, (tag, C, i, d)


# ---------------------------------------------------------------- 4. marginals and MAP
def _marginal_cases():
    cases = []
    for tag in TAGS:
        for n in ((0, 1, 2, 10) if tag in K.ITER_SWEEP else (10,)):
            cases.append((tag, n, K.SMALL, 21 if tag in K.ITER_SWEEP else 5))
    for tag in K.ITER_SWEEP:
        cases.append((tag, 10, K.SMALL, 5))
    for tag in K.ITER_SWEEP + K.GAMMA_EDGE + ["weights"]:
        cases.append((tag, 10, K.TRAIN, 21))
    cases += [("gamma_xy", 1, K.TRAIN, 21), ("default12", 0, K.TRAIN, 21), ("gamma_xy", 10, K.SMALL, 2), ("alpha_xy", 1, K.SMALL, 2)]
    return cases


@gpu
@pytest.mark.parametrize("tag,n,HW,C", _marginal_cases())
def test_marginals_and_map_off_the_default_parameters(crf_mod, oracles, seen, tag, n, HW, C):
    """DenseCRF.inference and .map after n iterations on the LDS-resident path (DenseCRF(W, H, C)), on one-image objects forced
    to the global-memory path and on a two-image batched object: marginals within the 1e-4 contract, labels equal.  n = 0: the
    first update launch writes the result; n = 1: the first iteration is also the last.  The batched object equals the one-image
    objects bit for bit."""
    ims, uns = oracles.images(HW), oracles.unaries(tag, HW, C)
    qb, lb, _ = run_object(crf_mod, HW, C, tag, ims, uns, n, nimages=2)
    for i in (0, 1):
        want_q, want_lab = oracles.run(tag, HW, C, i, n)
        what = "%s %dx%d C=%d n=%d image %d" % ((tag,) + HW + (C, n, i))
        q, lab, _ = run_object(crf_mod, HW, C, tag, ims[i], uns[i], n)
        seen("one-image object (LDS-resident)", tag, check_marginals(q, lab, want_q, want_lab, what + " LDS-resident"))
        q, lab, _ = run_object(crf_mod, HW, C, tag, ims[i], uns[i], n, nimages=1)
        seen("forced one-image object (global memory)", tag, check_marginals(q, lab, want_q, want_lab, what + " global memory"))
        seen("batched object (global memory)", tag, check_marginals(qb[i], lb[i], want_q, want_lab, what + " batched"))
        assert np.array_equal(qb[i], q) and np.array_equal(lb[i], lab), what


@gpu
@pytest.mark.parametrize("tag,n", [("gamma_xy", 10), ("beta_rgb", 10), ("weights", 10), ("gamma_0.5", 1), ("alpha_yx", 0)])
def test_marginals_and_map_just_beyond_the_lds_path(crf_mod, O, seen, tag, n):
    """a plain DenseCRF(73, 71, 5) — the global-memory path without being forced — on a noise image"""
    HW, C = K.BEYOND, 5
    im, un = K.images(HW)[1], K.unaries(HW, C, K.log_unary(tag))[1]
    oc = K.oracle_crf(O, im, PARAMS[tag], C, un)
    q, lab, obj = run_object(crf_mod, HW, C, tag, im, un, n)
    assert obj.lattice_norm(0).shape == (HW[0] * HW[1],)       # (only an object on the global-memory path answers this)
    seen("plain 71x73 object (global memory)", tag,
         check_marginals(q, lab, oc.inference(n).reshape(HW + (C,)), oc.map(n), "%s 71x73 n=%d" % (tag, n)))
    assert (obj.lattice_size(0), obj.lattice_size(1)) == (oc.lattice_size(0), oc.lattice_size(1))


@gpu
@pytest.mark.parametrize("HW,nimages", [(K.SMALL, 1), (K.BEYOND, None), (K.SMALL, 2)])
def test_map_without_iterations_on_the_global_path(crf_mod, O, HW, nimages):
    """map(0) on the global-memory path is the arg-max of the softmax of the unaries (no slice launch has written labels:
    lg_argmax_rows_kernel does) — asked first, after ten iterations, and after a restricted map has overwritten the labels"""
    C, tag = 21, "gamma_xy"
    H, W = HW
    nimg = nimages or 1
    ims, uns = K.images(HW)[:nimg], K.unaries(HW, C, True)[:nimg]
    want0 = uns.argmax(-1).reshape(nimg, H * W)                 # softmax is monotone: the arg-max of the scores themselves
    obj = crf_mod.DenseCRF(W, H, C, nimages=nimages)
    obj.set_unary_energy(-uns.ravel())
    obj.add_pairwise_energy(*PARAMS[tag], ims.ravel())
    assert np.array_equal(obj.map(0).reshape(nimg, -1), want0)
    oracle = [K.oracle_crf(O, ims[i], PARAMS[tag], C, uns[i]) for i in range(nimg)]
    q0 = obj.inference(0).reshape(nimg, H * W, C)
    for i in range(nimg):
        assert np.array_equal(oracle[i].map(0), want0[i])
        assert np.abs(q0[i] - oracle[i].inference(0).reshape(-1, C)).max() < 1e-6
    lab10 = obj.map(10).reshape(nimg, -1)
    assert all((oracle[i].map(10) != want0[i]).any() for i in range(nimg))      # ten iterations move labels: stale ones would show below
    assert np.array_equal(obj.map(0).reshape(nimg, -1), want0)
    sel = [[0, 3, 7]] * nimg
    restricted = obj.map(10, select=sel if nimages and nimages > 1 else sel[0]).reshape(nimg, -1)
    assert set(np.unique(restricted)) <= {0, 3, 7}
    assert np.array_equal(obj.map(0).reshape(nimg, -1), want0)
    assert np.array_equal(obj.map(10).reshape(nimg, -1), lab10)


# ---------------------------------------------------------------- 5. rebuilds on live state
@gpu
def test_context_follows_a_change_of_parameters(ops, oracles, seen):
    """one context through default12 -> gamma_xy -> default12 -> gamma 0.5 -> gamma 0.7 -> default12 -> alpha_xy: the cached
    Gaussian lattice (keyed on theta_gamma), the host's copy of its pixel-local flag (1 -> 0 -> 1, which decides whether the
    Gaussian workgroups are in the filter grid) and the bilateral lattices follow — after every step the marginals, one
    application of the Gaussian kernel and the filter plan equal those of a new context that has only seen that set, bit for
    bit, and the marginals are within the contract of the oracle"""
    HW, C = K.SMALL, 5
    H, W = HW
    ims = dev(oracles.images(HW), torch.uint8)
    f = dev(K.field(HW, C))
    live = ops.Context(2, C, H, W)
    local = []
    for step, tag in enumerate(["default12", "gamma_xy", "default12", "gamma_0.5", "gamma_0.7", "default12", "alpha_xy"]):
        un = dev(planes(oracles.unaries(tag, HW, C)))
        what = "step %d (%s)" % (step, tag)
        q = ops.crf_meanfield(un, ims, ctx=live, params=prm(tag, 10))
        fresh = ops.Context(2, C, H, W)
        assert torch.equal(q, ops.crf_meanfield(un, ims, ctx=fresh, params=prm(tag, 10))), what
        assert live.lattice_sizes(2) == fresh.lattice_sizes(2) == \
            (oracles.crf(tag, HW, 0).lattice_size(0), [oracles.crf(tag, HW, i).lattice_size(1) for i in (0, 1)]), what
        assert live.filter_plan(2) == fresh.filter_plan(2), what
        for k in (0, 1):
            assert torch.equal(live.filter_once(k, f), fresh.filter_once(k, f)), what
        for i in (0, 1):
            d = float(np.abs(np.transpose(q[i].cpu().numpy(), (1, 2, 0)) - oracles.run(tag, HW, C, i, 10)[0]).max())
            seen("context of two images (LDS-resident)", tag, d)
            assert d < CRF_TOL, (what, i, d)
        local.append(gauss_dropped(live, 2, C))
    print("Gaussian workgroups left out of the filter grid, step by step:", local)
    assert local[0] and local[2] and local[5] and not local[1] and not local[4]


@gpu
@pytest.mark.parametrize("HW,nimages", [(K.SMALL, 1), (K.BEYOND, None)])
def test_global_path_object_follows_a_change_of_parameters(crf_mod, O, seen, HW, nimages):
    """one object through weights (few vertices) -> beta_rgb (more vertices and segments: the value and partial-sum buffers grow)
    -> weights, add_pairwise_energy with the same image every time: bit-equal to newly made objects, within the contract of the
    oracle.  Then the same parameters with another image (the lattices must be rebuilt), and inference twice on unchanged state."""
    C = 5
    H, W = HW
    ims, uns = K.images(HW), K.unaries(HW, C, True)
    live = new_object(crf_mod, HW, C, nimages)
    live.set_unary_energy(-uns[0].ravel())
    sizes = []
    for step, (tag, i) in enumerate([("weights", 0), ("beta_rgb", 0), ("weights", 0), ("weights", 1)]):
        what = "step %d (%s, image %d)" % (step, tag, i)
        live.add_pairwise_energy(*PARAMS[tag], ims[i].ravel())
        q, lab = live.inference(10).reshape(H, W, C), live.map(10)
        oc = K.oracle_crf(O, ims[i], PARAMS[tag], C, uns[0])
        seen("rebuilt object (global memory)", tag, check_marginals(q, lab, oc.inference(10).reshape(H, W, C), oc.map(10), what))
        sizes.append((live.lattice_size(0), live.lattice_size(1)))
        assert sizes[-1] == (oc.lattice_size(0), oc.lattice_size(1)), what
        fq, flab, _ = run_object(crf_mod, HW, C, tag, ims[i], uns[0], 10, nimages=nimages, newly_made=True)
        assert np.array_equal(q, fq) and np.array_equal(lab, flab.ravel()), what
        assert np.array_equal(live.inference(10).reshape(H, W, C), q), what          # unchanged state: no rebuild, same bits
        assert np.array_equal(live.inference(2).reshape(H, W, C), run_object(crf_mod, HW, C, tag, ims[i], uns[0], 2, nimages=nimages,
                                                                                newly_made=True)[0]), what
        assert np.array_equal(live.inference(10).reshape(H, W, C), q), what
    assert sum(sizes[1]) > sum(sizes[0]) and sizes[2] == sizes[0] and sizes[3] != sizes[2]


@gpu
def test_lds_path_object_follows_a_change_of_parameters_and_image(crf_mod, O, seen):
    """the same on a DenseCRF(W, H, C) of the LDS-resident path, whose context caches the Gaussian lattice"""
    HW, C = K.SMALL, 5
    H, W = HW
    ims, uns = K.images(HW), K.unaries(HW, C, False)
    live = new_object(crf_mod, HW, C)
    live.set_unary_energy(-uns[0].ravel())
    for step, (tag, i) in enumerate([("default12", 0), ("gamma_yx", 0), ("default12", 0), ("default12", 1), ("gamma_0.7", 1)]):
        what = "step %d (%s, image %d)" % (step, tag, i)
        live.add_pairwise_energy(*PARAMS[tag], ims[i].ravel())
        q, lab = live.inference(10).reshape(H, W, C), live.map(10)
        oc = K.oracle_crf(O, ims[i], PARAMS[tag], C, uns[0])
        seen("rebuilt object (LDS-resident)", tag, check_marginals(q, lab, oc.inference(10).reshape(H, W, C), oc.map(10), what))
        assert (live.lattice_size(0), live.lattice_size(1)) == (oc.lattice_size(0), oc.lattice_size(1)), what
        fq, flab, _ = run_object(crf_mod, HW, C, tag, ims[i], uns[0], 10, newly_made=True)
        assert np.array_equal(q, fq) and np.array_equal(lab, flab.ravel()), what
        assert np.array_equal(live.inference(10).reshape(H, W, C), q), what


@gpu
@pytest.mark.parametrize("nimages", [None, 1])
def test_recycled_object_keeps_nothing_of_its_last_use(crf_mod, oracles, seen, nimages):
    """a destroyed object is parked with its device buffers (and, on the LDS-resident path, its context and that context's cached
    Gaussian lattice) and handed out again for the same shape: run with other parameters and no unary, it gives the oracle's
    zero-unary inference and the bits of an object that was newly made"""
    HW, C = K.SMALL, 7
    H, W = HW
    im, un = oracles.images(HW)[0], oracles.unaries("default12", HW, C)[0]
    q, _, first = run_object(crf_mod, HW, C, "default12", im, un, 10, nimages=nimages, newly_made=True)
    assert np.abs(q - oracles.run("default12", HW, C, 0, 10)[0]).max() < CRF_TOL
    handle, hits = first._h.value, cache_hits()
    del first
    again = crf_mod.DenseCRF(W, H, C, nimages=nimages)
    assert again._h.value == handle and cache_hits() == hits + 1        # the parked object
    new = crf_mod.DenseCRF(W, H, C, nimages=nimages)                     # the cache holds no second one of this shape:
    assert new._h.value != handle and cache_hits() == hits + 1          # newly made
    want_q, want_lab = oracles.run("gamma_xy", HW, C, 0, 10, unary=False)
    got = []
    for obj in (again, new):
        obj.add_pairwise_energy(*PARAMS["gamma_xy"], im.ravel())
        got.append((obj.inference(10).reshape(H, W, C), obj.map(10)))
    seen("recycled object (%s)" % ("global memory" if nimages else "LDS-resident"), "gamma_xy",
         check_marginals(got[0][0], got[0][1], want_q, want_lab, "recycled object, zero unary"))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    # (zero energies and Potts weights keep the marginals uniform whatever the kernels: that run shows that the old unary is gone.
    # With a unary the kernels count, the cached Gaussian lattice of the last use among them.)
    want_q, want_lab = oracles.run("gamma_xy", HW, C, 0, 10)
    un = oracles.unaries("gamma_xy", HW, C)[0]
    got = []
    for obj in (again, new):
        obj.set_unary_energy(-un.ravel())
        got.append((obj.inference(10).reshape(H, W, C), obj.map(10)))
    check_marginals(got[0][0], got[0][1], want_q, want_lab, "recycled object, with a unary")
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@gpu
def test_prepared_lattices_are_refused_for_other_kernel_widths(ops, O):
    """crf_prepare with the training parameters, then dsrg_crf_refine_batch(images = NULL) with a theta_gamma_y that differs:
    refused before anything is launched; the context then still runs — prepared, and from the images — with the same bits"""
    from dsrg_amd import synthetic as S, _lib
    from dsrg_amd._lib import CrfParams
    L = _lib.lib()
    B, C, H, W = 2, 21, 41, 41
    b = S.make_batch(29, B)
    probs, images = O.softmax_forward(b["logits"]), dev(b["images"])
    ctx = ops.Context(B, C, H, W)
    ops.crf_prepare(images, C, H, W, ctx=ctx)
    good, bad = CrfParams.from_crf_args(10, 12.0), CrfParams.from_crf_args(10, 12.0)
    bad.theta_gamma_y = 3.0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refine(p, params, with_images):
        refined = torch.empty((B, C, H, W), dtype=torch.float64, device="cuda")
        logq = torch.empty((B, C, H, W), dtype=torch.float32, device="cuda")
        _lib.check(L.dsrg_crf_refine_batch(ctx._h, B, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(images.data_ptr()) if with_images
                                           else None, images.shape[2], images.shape[3], ctypes.byref(params),
                                           ctypes.c_void_p(refined.data_ptr()), ctypes.c_void_p(logq.data_ptr()), stream))
        return refined, logq
    p = dev(probs)
    with pytest.raises(_lib.DsrgError, match="kernel parameters"):
        refine(p, bad, False)
    assert np.array_equal(p.cpu().numpy(), probs)               # not even the in-place clip ran
    r1, q1 = refine(p, good, False)                              # the prepared lattices are still there, and taken now
    with pytest.raises(_lib.DsrgError):
        refine(p, good, False)                                   # ... once
    r2, q2 = refine(dev(probs), good, True)
    assert torch.equal(r1, r2) and torch.equal(q1, q2)
    want, _ = O.crf_refine_batch(probs.copy(), b["images"], 12.0, 10)
    assert np.abs(r1.cpu().numpy() - want).max() < CRF_TOL
    r3, _ = refine(dev(probs), bad, True)                        # from the images, the other widths are simply built
    assert not torch.equal(r3, r1)
