"""CPU: the oracle's segment-order splat (oracle.splat_segments), the reference order's stand-in for what the HIP global-memory
CRF does with vertex rows of more than 4096 entries, and what the generators of tests/crf_large_cases.py promise.

Recorded (raw output: profiles/crf_large_oracle_orders.txt):
  longest row per case    const66 4248 | const71 4933 | const100_255 9481 | sky 8934 | gauss_wide 6000 (Gaussian lattice;
                          its bilateral rows stay at 11 or fewer) | natural cases: 3 .. 196 (bilateral), 1 .. 28 (Gaussian)
  max |dQ| between the two orders after ten iterations, 21 labels
                          const66 1.19e-07 | const71 1.19e-07 | const100_255 3.16e-06 | sky 4.77e-07   (contract: 1e-4)"""
import numpy as np
import pytest

import crf_large_cases as K
from crf_large_cases import SEG


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def rows(O):
    """longest rows of both lattices of every case, from the oracle's own dump: name -> (row lengths Gaussian, bilateral)"""
    out = {}
    for name, case in list(K.long_row_cases().items()) + list(K.natural_cases().items()):
        oc = K.oracle_crf(O, case[0], case[1], 3)
        out[name] = (K.row_lengths(oc, 0), K.row_lengths(oc, 1))
        print("rows %-14s Gaussian: longest %5d, %d above %d | bilateral: longest %5d, %d above %d"
              % (name, out[name][0].max(), (out[name][0] > SEG).sum(), SEG, out[name][1].max(), (out[name][1] > SEG).sum(), SEG))
    im, prm = K.batch_case()
    for b in range(im.shape[0]):
        oc = K.oracle_crf(O, im[b], prm, 3)
        out["batch%d" % b] = (K.row_lengths(oc, 0), K.row_lengths(oc, 1))
    return out


def test_generators_keep_their_promises(rows):
    """every long-row case has a row above 4096 in the intended lattice, one has a row above 8192 (three segments), one a last
    segment whose length is no multiple of 8 (the 8-wide rounds of lg_splat_segment end in a masked tail), the flat image of the
    batched case has long rows too, and the natural cases have none."""
    last_segments = []
    for name, case in K.long_row_cases().items():
        n = rows[name][case[2]]
        assert n.max() > SEG, name
        last_segments += [int(v) % SEG for v in n[n > SEG]]
    assert rows["gauss_wide"][1].max() <= SEG              # only the Gaussian half of the combine sees this case
    assert max(rows[name][1].max() for name in K.long_row_cases()) > 2 * SEG
    assert any(t % 8 != 0 for t in last_segments), last_segments
    assert rows["batch0"][1].max() > SEG and max(r.max() for r in rows["batch1"] + rows["batch2"]) <= SEG
    for name in K.natural_cases():
        assert max(rows[name][0].max(), rows[name][1].max()) <= SEG, name


@pytest.mark.parametrize("C", [2, 3])
def test_segment_mode_is_the_plain_oracle_where_no_row_is_cut(O, rows, C):
    """n at or above the longest row, and n = 4096 on a natural image: bit-identical filters and marginals (2 labels: seqCompute)"""
    im, prm, k_long = K.long_row_cases()["const71"]
    nat, nprm = K.natural_cases()["smooth101x123"]
    for image, p, n in ((im, prm, int(max(rows["const71"][0].max(), rows["const71"][1].max()))), (im, prm, 1 << 20), (nat, nprm, SEG)):
        H, W = image.shape[:2]
        oc = K.oracle_crf(O, image, p, C)
        x = K.field(H, W, C)
        oc.set_unary_energy(-np.log(x))
        plain = [oc.kernel_filter(k, x) for k in (0, 1)] + [oc.lattice_filter(k, x) for k in (0, 1)] + [oc.inference(3)]
        with O.splat_segments(n):
            seg = [oc.kernel_filter(k, x) for k in (0, 1)] + [oc.lattice_filter(k, x) for k in (0, 1)] + [oc.inference(3)]
        for a, b in zip(plain, seg):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (H, W, n)
    # and the mode is off again outside the block
    oc = K.oracle_crf(O, im, prm, C)
    x = K.field(71, 71, C)
    a = oc.kernel_filter(k_long, x)
    with O.splat_segments(SEG):
        b = oc.kernel_filter(k_long, x)
    assert not np.array_equal(a, b) and np.array_equal(a, oc.kernel_filter(k_long, x))


def _numpy_lattice_filter(oc, k, x, seg):
    """Permutohedral::sseCompute (permutohedral.cpp:529-589) with the splat in segment order, in float32 numpy, from the
    oracle's dump alone.  np.cumsum over float32 is a sequential sum."""
    f32 = np.float32
    keys, off, bary = oc.lattice_dump(k)
    n1, n2 = oc.lattice_neighbours(k)
    M, d1 = keys.shape[0], off.shape[1]
    order = np.argsort(off.ravel(), kind="stable")              # a vertex's entries in visiting order (pixel-major)
    t = bary.ravel()[order][:, None] * x[order // d1]           # float32 products w * in
    start = np.concatenate([[0], np.cumsum(np.bincount(off.ravel(), minlength=M))])
    vals = np.zeros((M + 1, x.shape[1]), f32)                   # row 0 = "no neighbour"
    for v in range(M):
        parts = [np.cumsum(t[p:min(p + seg, start[v + 1])], axis=0, dtype=f32)[-1] for p in range(start[v], start[v + 1], seg)]
        acc = parts[0] if parts else np.zeros(x.shape[1], f32)
        for p in parts[1:]:
            acc = acc + p
        vals[v + 1] = acc
    for j in range(d1):
        new = vals.copy()
        s = vals[n1[j] + 1] + vals[n2[j] + 1]
        new[1:] = vals[1:] + f32(0.5) * s
        vals = new
    alpha = f32(1.0) / (f32(1.0) + f32(2.0 ** -(d1 - 1)))
    out = np.zeros_like(x)
    for j in range(d1):
        out = out + (bary[:, j] * alpha)[:, None] * vals[off[:, j] + 1]
    assert t.dtype == f32 and vals.dtype == f32 and out.dtype == f32
    return out


@pytest.mark.parametrize("name", ["const71", "gauss_wide"])
def test_segment_mode_equals_a_numpy_restatement_bit_for_bit(O, name):
    im, prm, k = K.long_row_cases()[name]
    H, W = im.shape[:2]
    oc = K.oracle_crf(O, im, prm, 3)
    x = K.field(H, W, 3)
    with O.splat_segments(SEG):
        got = oc.lattice_filter(k, x)
    want = _numpy_lattice_filter(oc, k, x, SEG)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    whole = _numpy_lattice_filter(oc, k, x, 1 << 30)
    assert np.array_equal(oc.lattice_filter(k, x).view(np.uint32), whole.view(np.uint32))
    assert not np.array_equal(want, whole)


def test_the_two_orders_agree_within_the_contract_after_ten_iterations(O):
    """the reference against itself: what cutting rows at 4096 costs, ten iterations, 21 labels, log-probability unaries.
    Bar: the 1e-4 contract of the marginals.  Measured: see the module docstring."""
    for name in ("const66", "const71", "const100_255", "sky"):
        im, prm, _ = K.long_row_cases()[name]
        H, W = im.shape[:2]
        oc = K.oracle_crf(O, im, prm, 21)
        oc.set_unary_energy(-np.log(K.field(H, W, 21)))
        plain = oc.inference(10)
        with O.splat_segments(SEG):
            seg = oc.inference(10)
        d = float(np.abs(plain - seg).max())
        print("orders %-13s max|dQ| after 10 iterations: %.2e" % (name, d))
        assert d < 1e-4, name
