"""GPU (-m gpu): the global-memory dense CRF (dsrg_amd/csrc/lattice_large.hip) against the oracle piece by piece — lattice
structure, the normalisation vector and ONE application of each normalised kernel — instead of only through marginals after ten
softmax-contracted iterations.  Small maps reach this path through DenseCRF(W, H, C, nimages=1).

What the pieces cover that the end-to-end tests cannot see (CPU figures: tests/test_oracle_splat_segments.py):
  * vertex rows of more than kSplatSeg = 4096 entries (flat regions): lg_splat_unit's per-segment partial sums and
    lg_combine_kernel, on the bilateral lattice and (a 60-pixel spatial kernel) on the Gaussian one.  The bar is 2 ulp against
    the oracle summing in the SAME segment order (oracle.splat_segments) — one wrong entry at a segment boundary moves a
    filtered value by far more than that, and the ten-iteration marginals by less than the 1e-4 contract;
  * 61 to 96 labels: lg_update_kernel's 256 x (CP + 1) floats of LDS pass 64 KiB at CP = 64, and a lane group of the splat and
    the combine is at most a wave, so channels 64 and above need a second walk.

Observed on an MI355X (profiles/crf_large_filter_ulps.txt): the filters 0 ulp from their yardstick in all 184 comparisons
of B and C (the norms within their 2 ulp); where rows are cut, 5 to 41 ulp from the reference order; end to end at most
3.2e-6 from the plain oracle (constant 100x100) and 3.0e-7 from the segment-order one on images with cut rows, 1.6e-6 on noise
71x71 at 81 labels.  Before the second channel walk the marginals
at 65, 81 and 96 labels were off by 1.0 (profiles/crf_large_parent_60_to_96_labels.txt); 61 and 64 labels ran before too."""
import numpy as np
import pytest
import torch

import crf_large_cases as K
from crf_large_cases import SEG, ulps

pytestmark = pytest.mark.gpu

CRF_TOL = 1e-4           # north_star: "CRF marginals within 1e-4"
SEG_TOL = 3e-5           # the bar of this path's pinned end-to-end cases (test_crf_sweep_worst_cases_vs_oracle)
LABELS = [1, 2, 3, 21, 33, 60, 61, 64, 65, 81, 96]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def crf_mod():
    from dsrg_amd import crf, _lib
    _lib.require_gpu()
    return crf


@pytest.fixture(scope="module")
def oracles(O):
    """one oracle object per image, built once and left unchanged: its lattices and filters do not depend on the label count
    (kernel_filter takes the channel count from its argument)"""
    cache = {}

    def get(name, im, prm):
        if name not in cache:
            cache[name] = K.oracle_crf(O, im, prm, 1)
        return cache[name]
    return get


def _object(crf_mod, im, prm, C, unary=None):
    """a one-image object on the global-memory path, whatever the map size"""
    H, W = im.shape[:2]
    obj = crf_mod.DenseCRF(W, H, C, nimages=1)
    if unary is not None:
        obj.set_unary_energy(unary)
    obj.add_pairwise_energy(*prm, im.ravel())
    return obj


def _assert_same_lattice(got, keys, off, bary, n1, n2, tag):
    """test_lattice_structure_vs_oracle's comparison: the id-invariant form, then id for id"""
    N = off.shape[0]
    assert got["M"] == keys.shape[0], tag
    gk, ok = [tuple(r) for r in got["keys"]], [tuple(r) for r in keys]
    assert sorted(gk) == sorted(ok) and len(set(gk)) == len(gk), tag
    per_px_g = [sorted((gk[v], float(w)) for v, w in zip(got["vid"][i], got["bary"][i])) for i in range(N)]
    per_px_o = [sorted((ok[v], float(w)) for v, w in zip(off[i], bary[i])) for i in range(N)]
    assert per_px_g == per_px_o, tag
    nb_g = {gk[v]: [(gk[a] if a >= 0 else None, gk[z] if z >= 0 else None) for a, z in zip(got["n1"][:, v], got["n2"][:, v])]
            for v in range(got["M"])}
    nb_o = {ok[v]: [(ok[a] if a >= 0 else None, ok[z] if z >= 0 else None) for a, z in zip(n1[:, v], n2[:, v])]
            for v in range(keys.shape[0])}
    assert nb_g == nb_o, tag
    assert np.array_equal(got["keys"], keys) and np.array_equal(got["vid"], off), tag
    assert np.array_equal(got["bary"].view(np.uint32), bary.view(np.uint32)), tag      # bit-exact weights
    assert np.array_equal(got["n1"], n1) and np.array_equal(got["n2"], n2), tag


# ---------------------------------------------------------------- A. structure
@pytest.mark.parametrize("name", ["noise71x71", "smooth101x123", "const71", "sky"])
def test_large_lattice_structure_vs_oracle(crf_mod, O, oracles, name):
    """Permutohedral::init (permutohedral.cpp:140-321) of the global-memory build — hash insertion with wave-level leaders,
    first-occurrence ids from a scan, CSR by a radix sort — against the oracle: M, keys, per-pixel vertices and weights, blur
    neighbours of BOTH lattices, in the id-invariant form and id for id.  smooth101x123: N % 4 = 3, the SSE padding pixel's
    phantom vertices; const71 / sky: thousands of pixels in one simplex."""
    case = {**K.natural_cases(), **K.long_row_cases()}[name]
    im, prm = case[0], case[1]
    obj = _object(crf_mod, im, prm, 3)
    oc = oracles(name, im, prm)
    for k in (0, 1):
        keys, off, bary = oc.lattice_dump(k)
        n1, n2 = oc.lattice_neighbours(k)
        _assert_same_lattice(obj.lattice_dump(k), keys, off, bary, n1, n2, "%s lattice %d" % (name, k))
        assert obj.lattice_size(k) == keys.shape[0]
    print("lattices", name, "M_gauss", oc.lattice_size(0), "M_bil", oc.lattice_size(1))


def test_large_lattice_structure_of_a_batched_object_vs_oracle(crf_mod, O, oracles):
    """three 73x75 images (flat, smooth, noise; N % 4 = 3) in one batched object: every image's lattices, image number stripped
    from the keys and ids made local, against that image's own one-image oracle lattice"""
    ims, prm = K.batch_case()
    B, H, W = ims.shape[:3]
    obj = crf_mod.DenseCRF(W, H, 3, nimages=B)
    obj.add_pairwise_energy(*prm, ims.ravel())
    total = [0, 0]
    for b in range(B):
        oc = oracles("batch%d" % b, ims[b], prm)
        for k in (0, 1):
            keys, off, bary = oc.lattice_dump(k)
            n1, n2 = oc.lattice_neighbours(k)
            _assert_same_lattice(obj.lattice_dump(k, b), keys, off, bary, n1, n2, "batch image %d lattice %d" % (b, k))
            total[k] += keys.shape[0]
    assert [obj.lattice_size(0), obj.lattice_size(1)] == total


# ---------------------------------------------------------------- B. norm and one filter application, plain oracle
def _check_filters(obj, oc, x, tag, b=0, segments=False, O=None):
    """norm and norm . K (norm . x) of both kernels: at most 2 ulp from the oracle (the arithmetic and its order are the
    oracle's; where a row is cut, the order of oracle.splat_segments).  Returns the observed ulp distances."""
    seen = []
    for k in (0, 1):
        assert ulps(obj.lattice_norm(k, b), oc.lattice_norm(k)) <= 2, tag
        have = obj.filter_once(k, x, b)
        if segments:
            with O.splat_segments(SEG):
                want = oc.kernel_filter(k, x)
            plain = ulps(have, oc.kernel_filter(k, x))
        else:
            want = oc.kernel_filter(k, x)
        assert have.shape == want.shape and (want > 0).all(), tag
        u = ulps(have, want)
        print("%s kernel %d: %d ulp" % (tag, k, u) + (" (%d ulp from the plain order)" % plain if segments else ""))
        assert u <= 2, "%s kernel %d: %d ulp" % (tag, k, u)
        seen.append(u)
    return seen


@pytest.mark.parametrize("C", LABELS)
@pytest.mark.parametrize("name", ["smooth24x31", "noise17x40", "noise71x71", "smooth101x123"])
def test_large_norm_and_single_filter_application_vs_oracle(crf_mod, O, oracles, name, C):
    """the production lg_splat2 / lg_combine / lg_blur2 launches of one mean-field iteration and lg_slice_elem, on natural images
    (no row above 4096 entries: the reference's accumulation order exactly).  1 and 2 labels take seqCompute's arithmetic; 61 and
    64 are the first label counts whose padded rows pass 64 KiB in lg_update_kernel; 65, 81 and 96 need channels beyond a wave's
    64 lanes; 24x31 and 17x40 are maps the LDS path would take, forced here."""
    im, prm = K.natural_cases()[name]
    H, W = im.shape[:2]
    _check_filters(_object(crf_mod, im, prm, C), oracles(name, im, prm), K.field(H, W, C), "%s C=%d" % (name, C))


@pytest.mark.parametrize("C", LABELS)
def test_large_norm_and_single_filter_application_of_a_batched_object(crf_mod, O, oracles, C):
    """the same image by image on the batched object (the other images filter zeros); its flat image has rows above 4096"""
    ims, prm = K.batch_case()
    B, H, W = ims.shape[:3]
    obj = crf_mod.DenseCRF(W, H, C, nimages=B)
    obj.add_pairwise_energy(*prm, ims.ravel())
    for b in range(B):
        _check_filters(obj, oracles("batch%d" % b, ims[b], prm), K.field(H, W, C, seed=b), "batch image %d C=%d" % (b, C), b=b,
                       segments=(b == 0), O=O)


# ---------------------------------------------------------------- C. rows cut into segments, segment-order oracle
@pytest.mark.parametrize("C", [3, 21, 65])
@pytest.mark.parametrize("name", ["const66", "const71", "const100_255", "sky", "gauss_wide"])
def test_large_filter_with_segmented_rows_vs_segment_order_oracle(crf_mod, O, oracles, name, C):
    """rows of 4248 to 9481 entries (two and three segments; the longest rows end in segments of 152, 837, 1289, 742 and 1904
    entries, 837 and 1289 no multiples of 8): the per-segment partial sums of lg_splat_unit and their combination in segment order,
    for the bilateral lattice and — gauss_wide — for the Gaussian half of lg_combine_kernel; at 65 labels with the second channel
    walk.  The distance to the plain oracle is printed and carries no bar.  Observed on an MI355X: 0 ulp from the segment-order
    oracle in all 15 cases; 6 to 41 ulp from the plain one on the lattice whose rows are cut, 0 on the other."""
    im, prm, _ = K.long_row_cases()[name]
    H, W = im.shape[:2]
    _check_filters(_object(crf_mod, im, prm, C), oracles(name, im, prm), K.field(H, W, C), "%s C=%d" % (name, C), segments=True, O=O)


# ---------------------------------------------------------------- D. end to end
def _end_to_end(O, name, im, C, scale):
    import krahenbuhl2013
    from dsrg_amd.crf import CRF_device_batch
    H, W = im.shape[:2]
    uns = [np.log(np.maximum(K.field(H, W, C, seed=s).reshape(H, W, C), 1e-5)) for s in (0, 1)]
    imf = im.astype(np.float32)
    batch = CRF_device_batch(torch.from_numpy(np.stack([im, im])).cuda(), torch.from_numpy(np.stack(uns)).cuda(), scale_factor=scale)
    bmap = CRF_device_batch(torch.from_numpy(np.stack([im, im])).cuda(), torch.from_numpy(np.stack(uns)).cuda(), scale_factor=scale,
                            want="map").cpu().numpy()
    for s, un in enumerate(uns):
        plain = O.CRF(imf, un, scale_factor=scale)
        with O.splat_segments(SEG):
            seg = O.CRF(imf, un, scale_factor=scale)
        gots = [("batch", batch[s].cpu().numpy(), bmap[s])]
        if s == 0:
            one = krahenbuhl2013.CRF(imf, un, scale_factor=scale)
            gots.append(("CRF()", one, one.argmax(2)))
        for who, got, lab in gots:
            d_seg, d_plain = float(np.abs(got - seg).max()), float(np.abs(got - plain).max())
            print("%s C=%d %s unary %d: max|dQ| %.2e from the segment-order oracle, %.2e from the plain one" % (name, C, who, s, d_seg, d_plain))
            assert np.isfinite(got).all() and np.abs(got.sum(-1) - 1).max() < 1e-5
            assert d_seg < SEG_TOL and d_plain < CRF_TOL, (name, C, who)
            # a label may differ only where the oracle's own top two marginals are a near tie (test_crf_function_vs_oracle)
            wq, lab = plain.reshape(-1, C), np.asarray(lab).ravel()
            flip = np.flatnonzero(lab != wq.argmax(1))
            assert all(wq[i].max() - wq[i, int(lab[i])] < 1e-5 for i in flip), (name, C, who, len(flip))


@pytest.mark.parametrize("name,C", [("const71", 21), ("const100_255", 21), ("sky", 21), ("const71", 81), ("const71", 96)])
def test_large_crf_end_to_end_on_flat_images_and_many_labels(O, crf_mod, name, C):
    """marginals and MAP of krahenbuhl2013.CRF and CRF_device_batch, ten iterations: below 3e-5 from the oracle in segment order,
    below the 1e-4 contract from the plain oracle"""
    _end_to_end(O, name, K.long_row_cases()[name][0], C, 1.0)


@pytest.mark.parametrize("C", [81, 96])
def test_large_crf_end_to_end_on_a_natural_71x71_map_with_many_labels(O, crf_mod, C):
    """the smallest map of the path at the training scale, no row cut: the COCO blobs' 81 labels and the limit"""
    _end_to_end(O, "noise71x71", K.natural_cases()["noise71x71"][0], C, 12.0)


def test_large_crf_batch_equals_single_image_calls_at_65_labels(crf_mod, O):
    """the batched object against one-image objects of the same path at 65 labels (two channel walks), bit for bit"""
    from dsrg_amd.crf import CRF_device_batch
    ims, prm = K.batch_case()
    B, H, W = ims.shape[:3]
    C = 65
    uns = torch.from_numpy(np.stack([np.log(np.maximum(K.field(H, W, C, seed=b).reshape(H, W, C), 1e-5)) for b in range(B)])).cuda()
    imt = torch.from_numpy(ims).cuda()
    got_q, got_l = CRF_device_batch(imt, uns), CRF_device_batch(imt, uns, want="map")
    for b in range(B):
        one = _object(crf_mod, ims[b], prm, C, unary=(-uns[b]).contiguous())
        assert torch.equal(got_q[b], one.inference(10, out=torch.empty((H, W, C), dtype=torch.float32, device="cuda"))), b
        assert torch.equal(got_l[b], one.map(10, out=torch.empty((H, W), dtype=torch.int32, device="cuda"))), b
    want = O.CRF(ims[1].astype(np.float32), uns[1].cpu().numpy())
    assert np.abs(got_q[1].cpu().numpy() - want).max() < CRF_TOL


# ---------------------------------------------------------------- E. limits
def test_large_crf_limits_fail_loudly(crf_mod):
    """up to 96 labels run (above); what stays unsupported fails at creation, and the introspection says what it needs"""
    from dsrg_amd._lib import DsrgError
    with pytest.raises(DsrgError, match="at most 96 labels"):
        crf_mod.DenseCRF(71, 71, 97)
    with pytest.raises(DsrgError, match="at most 96 labels"):
        crf_mod.DenseCRF(71, 71, 97, nimages=2)
    with pytest.raises(DsrgError, match="images per batched"):
        crf_mod.DenseCRF(71, 71, 21, nimages=9)
    im = K.constant(20, 20)
    small = crf_mod.DenseCRF(20, 20, 3)                      # the LDS-resident path
    small.add_pairwise_energy(*K.params(), im.ravel())
    for call in (lambda o: o.lattice_dump(1), lambda o: o.lattice_norm(0), lambda o: o.filter_once(1, K.field(20, 20, 3))):
        with pytest.raises(DsrgError, match="LDS-resident path"):
            call(small)
    fresh = crf_mod.DenseCRF(20, 20, 3, nimages=1)
    with pytest.raises(DsrgError, match="add_pairwise_energy must be called first"):
        fresh.lattice_norm(1)
    fresh.add_pairwise_energy(*K.params(), im.ravel())
    with pytest.raises(DsrgError, match="image 1 outside"):
        fresh.lattice_norm(1, b=1)
    assert fresh.lattice_norm(1).shape == (400,)
