"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracle and the golden
fixtures.  Integer work (SRG) must be bit-exact; floating point within the stated tolerance
(CRF marginals 1e-4 per BASELINE.json's north_star; observed ~1e-6)."""
import numpy as np
import pytest
import torch

from conftest import srg_case, glue_inputs, seeds_match_or_borderline
from dsrg_amd import synthetic as S

pytestmark = pytest.mark.gpu

CRF_TOL = 1e-4          # north_star: "CRF marginals within 1e-4"


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


# ---------------------------------------------------------------- SRG: bit-exact
def test_srg_golden_vectors_bit_exact(ops, golden_srg):
    for name in golden_srg["names"]:
        labels, seed, refined, want = srg_case(golden_srg, str(name))
        got = ops.srg_grow(dev(labels[None]), dev(seed[None]), dev(refined[None], torch.float64), 0.99, 0.85)
        assert np.array_equal(got.cpu().numpy()[0].astype(np.uint8), want), name


def test_srg_random_batches_vs_oracle(ops, O):
    """sides 3..69, so mostly the 64-bit one-row form: the other growth forms and their seams are in tests/test_srg_paths.py"""
    rng = np.random.default_rng(5)
    for trial in range(8):
        B, C = 5, (21 if trial < 6 else 81 + 15 * (trial - 6))              # 81 = COCO (pylayers.py:389-512), 96 = the cap
        H, W = (41, 41) if trial < 3 or trial >= 6 else (int(rng.integers(3, 70)), int(rng.integers(3, 70)))
        labels, cues = S.make_labels_cues(rng, B, C, max(H, 7), max(W, 7))
        cues = np.ascontiguousarray(cues[:, :, :H, :W])
        refined = np.empty((B, C, H, W))
        for b in range(B):
            pres = np.where(labels[b, 0, 0] == 1)[0]
            z = S.make_logits(rng, 1, C, H, W, gain=60.0)[0].astype(np.float64)
            e = np.exp(z[pres] - z[pres].max(0, keepdims=True))
            p = np.full((C, H, W), 1e-4)
            p[pres] = np.maximum(e / e.sum(0, keepdims=True), 1e-4)
            refined[b] = p / p.sum(0, keepdims=True)
        want = O.srg_grow_batch(labels, cues, refined)
        got = ops.srg_grow(dev(labels), dev(cues), dev(refined, torch.float64)).cpu().numpy()
        assert want.sum() > cues.sum()
        assert np.array_equal(got, want)
        # invariants: monotone, absent classes untouched, idempotent
        assert (got >= cues).all()
        absent = labels[:, 0, 0] != 1
        assert np.array_equal(got[absent], cues[absent])
        again = ops.srg_grow(dev(labels), dev(got), dev(refined, torch.float64)).cpu().numpy()
        assert np.array_equal(again, got)


# ---------------------------------------------------------------- pointwise layers
def test_softmax_forward_backward(ops, O):
    b = S.make_batch(1, 4)
    x = b["logits"]
    p = ops.softmax_forward(dev(x)).cpu().numpy()
    assert np.abs(p - O.softmax_forward(x)).max() < 1e-6
    g = np.random.default_rng(0).standard_normal(x.shape).astype(np.float32)
    dx = ops.softmax_backward(dev(x), dev(g)).cpu().numpy()
    want = O.softmax_backward(x, g)
    assert np.abs(dx - want).max() < 1e-5 * max(1.0, np.abs(want).max())


def test_losses_forward_backward(ops, O):
    b = S.make_batch(2, 4)
    p = O.softmax_forward(b["logits"])
    seeds = b["cues"]
    seeds[1] = 0
    loss, grad = ops.seed_loss(dev(p), dev(seeds))
    wl, wg = O.seed_loss(p, seeds)
    assert abs(loss.item() - wl) < 1e-5 * max(1, abs(wl))
    assert np.abs(grad.cpu().numpy() - wg).max() < 1e-5 * max(1.0, np.abs(wg).max())
    rng = np.random.default_rng(4)
    lq = np.log(O.softmax_forward((b["logits"] + rng.standard_normal(p.shape) * 8).astype(np.float32)))
    loss, gp, gq = ops.constrain_loss(dev(p), dev(lq))
    wl, wgp, wgq = O.constrain_loss(p, lq)
    assert abs(loss.item() - wl) < 1e-5 * max(1, abs(wl))
    # elements whose ratio sits within float rounding of the (inclusive) clip bounds may take the other branch — but then they
    # must equal exactly what that other branch gives: in range dp = -(q/p)/BHW, dlq = (q log r + q)/BHW; clipped dp = 0,
    # dlq = q log(bound)/BHW
    qd = np.exp(lq.astype(np.float64))
    r = qd / p
    safe = (np.abs(r - 0.05) > 1e-5) & (np.abs(r - 20) > 1e-3)
    gpn, gqn = gp.cpu().numpy(), gq.cpu().numpy()
    assert np.abs(gpn - wgp)[safe].max() < 1e-6
    assert np.abs(gqn - wgq)[safe].max() < 1e-6
    n = p.shape[0] * p.shape[2] * p.shape[3]
    near = ~safe
    if near.any():
        bound = np.where(np.abs(r - 0.05) <= 1e-5, 0.05, 20.0)
        in_p, in_q = -(qd / p) / n, (qd * np.log(np.clip(r, 0.05, 20.0)) + qd) / n
        out_p, out_q = np.zeros_like(in_p), qd * np.log(bound) / n
        ok_p = np.minimum(np.abs(gpn - in_p), np.abs(gpn - out_p)) < 1e-6
        ok_q = np.minimum(np.abs(gqn - in_q), np.abs(gqn - out_q)) < 1e-6
        assert ok_p[near].all() and ok_q[near].all()
    print("constrain-loss gradient: %d of %d elements within rounding of a clip bound" % (int(near.sum()), near.size))


# ---------------------------------------------------------------- dense CRF
@pytest.mark.parametrize("kind,scale,HW,C", [("smooth", 12.0, (41, 41), 21), ("noise", 12.0, (41, 41), 21),
                                             ("dark_corner", 12.0, (41, 41), 21), ("smooth", 12.0, (65, 65), 21),
                                             ("smooth", 1.0, (24, 31), 7), ("noise", 3.0, (17, 40), 3),
                                             ("smooth", 12.0, (1, 9), 2), ("noise", 12.0, (1, 1), 2),
                                             ("noise", 1.0, (2, 3), 4), ("smooth", 3.0, (5, 1), 21),
                                             ("noise", 12.0, (70, 70), 3),      # largest LDS-resident map
                                             ("noise", 12.0, (71, 71), 3),      # smallest map on the global-memory path
                                             # maps beyond the LDS-resident kernels: global-memory path (test-time CRF)
                                             ("smooth", 1.0, (121, 161), 21), ("noise", 3.0, (100, 150), 5),
                                             ("smooth", 1.0, (321, 321), 21),
                                             ("smooth", 1.0, (375, 500), 21),   # the largest VOC image shape (test-ms.py)
                                             ("noise", 1.0, (101, 123), 4),     # odd width, N % 4 = 3: phantom vertices on the large path
                                             # entry counts whose arrays end exactly on an allocation boundary (6 N x 4 bytes a
                                             # multiple of 256): one element past the end corrupts the neighbouring array there and
                                             # nowhere else (a round-3 bug: seg_start / seg_cnt hold 6 N + 1 entries)
                                             ("smooth", 1.0, (64, 94), 33), ("smooth", 1.0, (147, 160), 21),
                                             ("dark_corner", 12.0, (123, 186), 21)])
def test_crf_function_vs_oracle(O, kind, scale, HW, C):
    """krahenbuhl2013.CRF (host API of the reference) — marginals within 1e-4 of the oracle,
    identical lattice sizes."""
    import krahenbuhl2013
    from dsrg_amd.crf import DenseCRF
    H, W = HW
    rng = np.random.default_rng(hash((kind, H, W, C)) % 2 ** 31)
    img = S.make_images(rng, 1, size=max(H, W), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
    im = np.ascontiguousarray(np.transpose(img, (1, 2, 0)))
    logits = S.make_logits(rng, 1, C, H, W)
    un = np.ascontiguousarray(np.transpose(np.maximum(O.softmax_forward(logits)[0], 1e-4), (1, 2, 0)))
    if scale == 1.0:
        un = np.log(un)                                     # test-time call passes log-probs (test-ms.py:106)
    want = O.CRF(im, un, scale_factor=scale)
    got = krahenbuhl2013.CRF(im, un, scale_factor=scale)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got.sum(-1) - 1).max() < 1e-5
    assert np.abs(got - want).max() < CRF_TOL
    oc = O.DenseCRF(W, H, C)
    oc.add_pairwise_energy(10, 80 / scale, 80 / scale, 13, 13, 13, 3, 3 / scale, 3 / scale, im.astype(np.uint8).ravel())
    hc = DenseCRF(W, H, C)
    hc.set_unary_energy(-un.ravel())
    hc.add_pairwise_energy(10, 80 / scale, 80 / scale, 13, 13, 13, 3, 3 / scale, 3 / scale, im.astype(np.uint8).ravel())
    lab = hc.map(10)
    assert hc.lattice_size(0) == oc.lattice_size(0) and hc.lattice_size(1) == oc.lattice_size(1)
    oc.set_unary_energy(-un.ravel())
    wl = oc.map(10)
    # the labels may differ only where the oracle's own top two marginals are a near tie: at such a pixel the label we chose must
    # be within 1e-5 of the oracle's maximum (no budget of "a few flipped pixels")
    flip = np.flatnonzero(np.asarray(lab).ravel() != np.asarray(wl).ravel())
    wq = want.reshape(-1, C)
    assert all(wq[i].max() - wq[i, int(np.asarray(lab).ravel()[i])] < 1e-5 for i in flip), (len(flip), H, W)


@pytest.mark.parametrize("seed", [20083, 20173])
def test_crf_sweep_worst_cases_vs_oracle(O, seed):
    """the two worst cases the randomised sweep (tools/parity_sweep_crf.py, 240 calls, profiles/r05_parity_sweeps_long.txt) ever
    found, pinned as tests with the sweep's own generator: seed 20173 = 138 x 163, 21 labels, scale 3, dark_corner — the
    global-memory path, where a vertex that gathers thousands of equal-coloured pixels sums its row in segments and the oracle
    sums it pixel by pixel (fp32 reassociation, amplified by ten softmax iterations at weight 10); seed 20083 = 89 x 96, 7 labels,
    scale 1.  Round 5 (rows cut into 64-entry segments): 7.44e-5 and 2.21e-5 of the contract's 1e-4; since round 6 a row is summed
    whole, in the reference's order, up to 4 096 entries (lattice_large.hip, kSplatSeg): 4.4e-6 and 7e-9.  Bar here: 3e-5."""
    import krahenbuhl2013
    it = seed - 20000
    rng = np.random.default_rng(seed)
    H, W = (int(rng.integers(1, 71)), int(rng.integers(1, 71))) if it % 2 == 0 else (int(rng.integers(60, 180)), int(rng.integers(60, 220)))
    C = int(rng.choice([2, 3, 7, 21, 21, 21, 33]))
    scale = float(rng.choice([1.0, 3.0, 12.0]))
    kind = ["smooth", "noise", "dark_corner"][it % 3]
    assert (H, W, C, scale, kind) in ((89, 96, 7, 1.0, "dark_corner"), (138, 163, 21, 3.0, "dark_corner"))
    img = S.make_images(rng, 1, size=max(H, W, 8), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
    im = np.ascontiguousarray(np.transpose(img, (1, 2, 0)))
    logits = S.make_logits(rng, 1, C, H, W, gain=float(rng.uniform(2, 40)), sigma=float(rng.uniform(1, 10)))
    un = np.ascontiguousarray(np.transpose(np.maximum(O.softmax_forward(logits)[0], 1e-5), (1, 2, 0)))
    if rng.random() < 0.5:
        un = np.log(un)
    want = O.CRF(im, un, scale_factor=scale)
    got = krahenbuhl2013.CRF(im, un, scale_factor=scale)
    d = float(np.abs(got - want).max())
    print("sweep worst case seed %d (%dx%d C=%d scale %g): max|dQ| %.2e" % (seed, H, W, C, scale, d))
    assert np.isfinite(got).all() and d < 3e-5
    assert (got.argmax(2) == want.argmax(2)).all()


@pytest.mark.parametrize("kind,scale,HW", [("smooth", 12.0, (41, 41)), ("noise", 12.0, (41, 41)), ("dark_corner", 12.0, (41, 41)),
                                           ("smooth", 12.0, (65, 65)), ("noise", 1.0, (24, 31)), ("smooth", 3.0, (17, 40))])
def test_lattice_structure_vs_oracle(ops, O, kind, scale, HW):
    """SURVEY 8c, last row: Permutohedral::init (permutohedral.cpp:140-321) -> M, the keys, the per-pixel (vertex,
    weight) lists and the blur-neighbour table of BOTH lattices, HIP against the oracle.  Compared id for id (the HIP
    build hands out the reference's first-occurrence ids) and, so that a future renumbering only has to relax the
    former, in the id-invariant form too (key multiset, per-pixel sorted (key, weight), neighbour KEYS per vertex key)."""
    H, W = HW
    B, C = 2, 3
    rng = np.random.default_rng(hash((kind, H, W)) % 2 ** 31)
    img = S.make_images(rng, B, size=max(H, W), kind=kind)[:, :, :H, :W] + S.MEAN_PIXEL[None, :, None, None]
    im_u8 = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1))).astype(np.uint8)
    unary = np.log(np.maximum(O.softmax_forward(S.make_logits(rng, B, C, H, W)), 1e-4))
    ctx = ops.Context(B, C, H, W)
    ops.crf_meanfield(dev(unary), dev(im_u8, torch.uint8), 10, scale, ctx=ctx)
    for b in range(B):
        oc = O.DenseCRF(W, H, C)
        oc.add_pairwise_energy(10, 80 / scale, 80 / scale, 13, 13, 13, 3, 3 / scale, 3 / scale, im_u8[b].ravel())
        for k in (0, 1):
            if k == 0 and b > 0:
                continue                                    # one Gaussian lattice shared by the batch
            keys, off, bary = oc.lattice_dump(k)
            n1, n2 = oc.lattice_neighbours(k)
            got = ctx.lattice_dump(k, b if k == 1 else 0)
            tag = "%s %dx%d scale %g image %d lattice %d" % (kind, H, W, scale, b, k)
            assert got["M"] == keys.shape[0], tag
            # id-invariant form
            gk, ok = [tuple(r) for r in got["keys"]], [tuple(r) for r in keys]
            assert sorted(gk) == sorted(ok) and len(set(gk)) == len(gk), tag
            per_px_g = [sorted((gk[v], float(w)) for v, w in zip(got["vid"][i], got["bary"][i])) for i in range(H * W)]
            per_px_o = [sorted((ok[v], float(w)) for v, w in zip(off[i], bary[i])) for i in range(H * W)]
            assert per_px_g == per_px_o, tag
            nb_g = {gk[v]: [(gk[a] if a >= 0 else None, gk[z] if z >= 0 else None) for a, z in zip(got["n1"][:, v], got["n2"][:, v])]
                    for v in range(got["M"])}
            nb_o = {ok[v]: [(ok[a] if a >= 0 else None, ok[z] if z >= 0 else None) for a, z in zip(n1[:, v], n2[:, v])]
                    for v in range(keys.shape[0])}
            assert nb_g == nb_o, tag
            # id for id
            assert np.array_equal(got["keys"], keys) and np.array_equal(got["vid"], off), tag
            assert np.array_equal(got["bary"].view(np.uint32), bary.view(np.uint32)), tag      # bit-exact weights
            assert np.array_equal(got["n1"], n1) and np.array_equal(got["n2"], n2), tag
        print("lattices", kind, HW, "image", b, "M_gauss", oc.lattice_size(0), "M_bil", oc.lattice_size(1))


def test_crf_refine_batch_vs_oracle(ops, O):
    for seed, B, kind in [(3, 4, "smooth"), (4, 2, "noise")]:
        b = S.make_batch(seed, B, image_kind=kind)
        probs = O.softmax_forward(b["logits"])
        assert (probs < 1e-4).any()
        p_ref = probs.copy()
        want_ref, want_log = O.crf_refine_batch(p_ref, b["images"], 12.0, 10)
        p_dev = dev(probs)
        ctx = ops.get_context(B, 21, 41, 41)
        refined, logq = ops.crf_refine(p_dev, dev(b["images"]), 12.0, 10, ctx=ctx)
        assert np.array_equal(p_dev.cpu().numpy(), p_ref)                       # in-place clip
        assert np.abs(refined.cpu().numpy() - want_ref).max() < CRF_TOL
        assert np.abs(np.exp(logq.cpu().numpy()) - want_ref).max() < CRF_TOL
        assert np.abs(refined.cpu().numpy().sum(1) - 1).max() < 1e-12
        mg, mb = ctx.lattice_sizes(B)
        print("lattice sizes: gaussian %d bilateral %s (N=1681)" % (mg, mb))
        assert mg >= 3 * 1681 and all(1681 < m <= 6 * 1684 for m in mb)
        bd = ops.crf_layer_backward(refined, dev(b["cues"])).cpu().numpy()
        assert np.abs(bd - O.crf_layer_backward(refined.cpu().numpy(), b["cues"])).max() < 1e-6


@pytest.mark.parametrize("B,C,HW,scale", [(16, 21, (41, 41), 12.0), (1, 21, (41, 41), 12.0), (20, 21, (41, 41), 12.0),
                                          (3, 30, (33, 29), 12.0), (2, 21, (65, 65), 12.0), (2, 5, (24, 31), 1.0),
                                          (30, 7, (20, 20), 3.0), (2, 40, (9, 9), 12.0), (1, 2, (1, 9), 12.0), (2, 81, (41, 41), 12.0)])
def test_filter_variants_are_bit_identical(ops, O, B, C, HW, scale):
    """Every option of the mean-field launch (meanfield.hip kOpt*) keeps the arithmetic and its order: the marginals must be
    BIT-IDENTICAL to the plain launch loop (options 0 = the round-2 kernels: Gaussian workgroups in the filter launch, all
    vertex slots).  Option 1 moves the pixel-local Gaussian lattice of the training scale into the
    update kernel (per-pixel evaluation in registers); shapes with scale 1 / 3 have a non-local Gaussian lattice and take the
    general path under every option; 65x65 takes the chunked-index variant; 81 labels = the COCO blobs."""
    from dsrg_amd import _lib
    L = _lib.lib()
    H, W = HW
    rng = np.random.default_rng(B * 131 + C)
    img = S.make_images(rng, B, size=max(H, W, 8), kind="noise" if B == 2 else "smooth")[:, :, :H, :W] + S.MEAN_PIXEL[None, :, None, None]
    im_u8 = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1))).astype(np.uint8)
    unary = np.maximum(O.softmax_forward(S.make_logits(rng, B, C, H, W)), 1e-4)
    outs = {}
    try:
        for opts in (0, 3, 1, 2):
            L.dsrg_debug_set_filter_opts(opts)
            ctx = ops.Context(B, C, H, W)
            q = ops.crf_meanfield(dev(unary), dev(im_u8, torch.uint8), 10, scale, ctx=ctx)
            q1 = ops.crf_meanfield(dev(unary), dev(im_u8, torch.uint8), 3, scale, ctx=ctx)       # same context, cached Gaussian lattice
            outs[opts] = (q.cpu().numpy(), q1.cpu().numpy())
    finally:
        L.dsrg_debug_set_filter_opts(-1)
    for opts, o in outs.items():
        for k in (0, 1):
            assert np.array_equal(outs[0][k], o[k]), "options %d differ from the plain launch loop" % opts
    want = np.stack([np.transpose(O.CRF(im_u8[b], np.ascontiguousarray(np.transpose(unary[b], (1, 2, 0))), scale_factor=scale), (2, 0, 1))
                     for b in range(min(B, 2))])
    assert np.abs(outs[3][0][:min(B, 2)] - want).max() < CRF_TOL


@pytest.mark.parametrize("kind,scale,HW,C", [("smooth", 12.0, (41, 41), 21), ("noise", 12.0, (41, 41), 21), ("smooth", 12.0, (65, 65), 21),
                                             ("dark_corner", 12.0, (41, 41), 5), ("noise", 1.0, (24, 31), 7), ("smooth", 3.0, (17, 40), 4),
                                             ("noise", 12.0, (28, 5), 1), ("smooth", 12.0, (41, 41), 2), ("noise", 1.0, (33, 20), 2)])
def test_single_filter_application_and_norm_vs_oracle(ops, O, kind, scale, HW, C):
    """a7 / a9 without the softmax contraction of ten iterations: the normalisation vector of DenseKernel::initLattice
    (pairwise.cpp:40-62) and ONE application of DenseKernel::filter (pairwise.cpp:63-80: x norm, Permutohedral::compute
    permutohedral.cpp:529-604, x norm) on both lattices, HIP against the oracle.  The arithmetic and its order are the
    oracle's, so the results are compared to 2 ulp (observed: bit-equal).  One and two label planes take the reference's
    seqCompute arithmetic (permutohedral.cpp:476-527 via :600-601): blur summed in double, slice as (w * value) * alpha."""
    H, W = HW
    B, N = 2, H * W
    rng = np.random.default_rng(hash((kind, H, W, C)) % 2 ** 31)
    img = S.make_images(rng, B, size=max(H, W), kind=kind)[:, :, :H, :W] + S.MEAN_PIXEL[None, :, None, None]
    im_u8 = np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1))).astype(np.uint8)
    q = O.softmax_forward(S.make_logits(rng, B, C, H, W, gain=8.0))          # a valid marginal field
    ctx = ops.Context(B, C, H, W)
    ops.crf_meanfield(dev(q), dev(im_u8, torch.uint8), 1, scale, ctx=ctx)     # builds the lattices of these images
    got = {k: ctx.filter_once(k, dev(q)).cpu().numpy() for k in (0, 1)}

    def ulps(a, b):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
        return int(np.abs(ia - ib).max())
    for b in range(B):
        oc = O.DenseCRF(W, H, C)
        oc.add_pairwise_energy(10, 80 / scale, 80 / scale, 13, 13, 13, 3, 3 / scale, 3 / scale, im_u8[b].ravel())
        qlf = np.ascontiguousarray(np.transpose(q[b].reshape(C, N), (1, 0)))                   # (N, C) label-fastest
        for k in (0, 1):
            tag = "%s %dx%d scale %g image %d kernel %d" % (kind, H, W, scale, b, k)
            norm_o = oc.lattice_norm(k)
            norm_g = ctx.lattice_norm(k, b if k == 1 else 0)
            assert ulps(norm_g, norm_o) <= 2, tag
            want = oc.kernel_filter(k, qlf)                                                     # (N, C)
            have = np.transpose(got[k][b].reshape(C, N), (1, 0))
            assert (want > 0).all() and ulps(have, want) <= 2, "%s: %d ulp" % (tag, ulps(have, want))
            # and the raw lattice filter of a 1-channel field of ones is what the norm was made from (pairwise.cpp:44)
            k1 = oc.lattice_filter(k, np.ones((N, 1), np.float32))[:, 0]
            assert np.allclose(1.0 / np.sqrt(k1.astype(np.float64) + 1e-20), norm_o, rtol=1e-6, atol=0)


def test_crf_is_deterministic(ops, O):
    b = S.make_batch(9, 3)
    probs = O.softmax_forward(b["logits"])
    outs = []
    for _ in range(3):
        refined, _ = ops.crf_refine(dev(probs), dev(b["images"]), 12.0, 10)
        outs.append(refined.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---------------------------------------------------------------- Caffe-protocol layers vs golden glue
class Blob(object):
    def __init__(self, data):
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.diff = np.zeros_like(self.data)

    def reshape(self, *shape):
        if self.data.shape != tuple(shape):
            self.data = np.zeros(shape, np.float32)
            self.diff = np.zeros(shape, np.float32)


@pytest.mark.parametrize("tag", ["voc", "tiny", "grow"])
def test_pylayers_protocol_vs_reference_glue(golden_glue, tag):
    """Drive the drop-in `pylayers` classes exactly as Caffe would and compare with what the
    reference's Python layers produced on the same blobs (tests/golden/layer_glue.npz)."""
    import pylayers
    g = golden_glue
    probs, images = glue_inputs(g, tag)
    crf = pylayers.CRFLayer()
    b_probs, b_im, top = Blob(probs), Blob(images), Blob(np.zeros_like(probs))
    crf.setup([b_probs, b_im], [top])
    crf.reshape([b_probs, b_im], [top])
    crf.forward([b_probs, b_im], [top])
    assert np.array_equal(b_probs.data, g[tag + "_probs_clipped"])
    assert crf.result.dtype == np.float64
    assert np.abs(crf.result - g[tag + "_refined"]).max() < CRF_TOL
    assert np.abs(np.exp(top.data) - g[tag + "_refined"]).max() < CRF_TOL
    top.diff[...] = g[tag + "_top_diff"]
    crf.backward([top], [True, False], [b_probs, b_im])
    # backward = (1 - result) * top.diff (pylayers.py:90-92): held to 1e-6 on the layer's own marginals (as
    # test_crf_refine_batch_vs_oracle holds dsrg_crf_layer_backward), and against the reference's output as far as the two sets
    # of marginals agree — the only other source of a difference
    dmax = np.abs(g[tag + "_top_diff"]).max()
    gap = np.abs(crf.result - g[tag + "_refined"]).max()
    assert np.abs(b_probs.diff - (1.0 - crf.result) * g[tag + "_top_diff"]).max() <= 1e-6 * dmax
    assert np.abs(b_probs.diff - g[tag + "_crf_bottom_diff"]).max() <= (gap + 1e-6) * dmax

    dsrg = pylayers.DSRGLayer()
    dsrg.param_str = "{'th1': 0.99, 'th2': 0.85}"
    from dsrg_amd import layers as _layers
    # as in the net, DSRGLayer reads the very blobs CRFLayer read (train-s.prototxt:760-800): it takes that layer's marginals
    d_probs = b_probs
    bottoms = [Blob(g[tag + "_labels"]), d_probs, Blob(g[tag + "_cues"]), b_im]
    dtop = Blob(np.zeros_like(probs))
    dsrg.setup(bottoms, [dtop])
    dsrg.reshape(bottoms, [dtop])
    reused = _layers.crf_reuse_count
    dsrg.forward(bottoms, [dtop])
    assert _layers.crf_reuse_count == reused + (1 if _layers._digest is not None else 0)
    assert np.array_equal(d_probs.data, g[tag + "_probs_clipped"])
    # other bytes in either blob: the CRF runs again, same seeds on the original blobs' copies
    dsrg2 = pylayers.DSRGLayer()
    dsrg2.param_str = dsrg.param_str
    im2 = Blob(images.copy())
    im2.data[0, 0, 0, 0] += 1.0
    bottoms2 = [Blob(g[tag + "_labels"]), Blob(b_probs.data.copy()), Blob(g[tag + "_cues"]), im2]
    dtop2 = Blob(np.zeros_like(probs))
    dsrg2.setup(bottoms2, [dtop2])
    dsrg2.reshape(bottoms2, [dtop2])
    reused = _layers.crf_reuse_count
    dsrg2.forward(bottoms2, [dtop2])
    assert _layers.crf_reuse_count == reused
    # grown masks bit-exact against the reference glue's seeds; a differing pixel must trace to a threshold decision
    # within 1e-5 of th on the reference side (conftest.seeds_match_or_borderline), anything else fails
    from dsrg_amd import ops as _ops
    from oracle import oracle as _O
    hip_refined, _ = _ops.crf_refine(dev(probs), dev(images), 12.0, 10, want_log=False)    # what the layer thresholded
    labels_g, cues_g = g[tag + "_labels"].astype(np.float32), g[tag + "_cues"].astype(np.float32)
    ref_refined = g[tag + "_refined"]
    assert np.array_equal(_O.srg_grow_batch(labels_g, cues_g, ref_refined).astype(np.uint8), g[tag + "_seeds"].astype(np.uint8))
    seeds_match_or_borderline(_O, dtop.data, labels_g, cues_g, ref_refined, hip_refined.cpu().numpy(), tag="glue/" + tag)


# ---------------------------------------------------------------- fused step vs layer-by-layer oracle
def _check_fused_step(ops, O, logits, images, labels, cues, tag, scale_factor=12.0, maxiter=10):
    """dsrg_supervision_step against the oracle layer by layer in the order of train-s.prototxt:746-810 / SURVEY A.3:
    softmax blob, CRF marginals (1e-4), seeds bit-exact (borderline-proof otherwise), both losses, the fc8 gradient"""
    B, C, H, W = logits.shape
    if ops.lds_path_supports(H, W):
        ctx = ops.get_context(B, C, H, W)
        losses, grad, blobs = ops.supervision_step(dev(logits), dev(images), dev(labels), dev(cues), want_blobs=True, ctx=ctx,
                                                   scale_factor=scale_factor, maxiter=maxiter)
        hip_refined = ctx.read_refined(B).cpu().numpy()
    else:                                                                   # the global-memory composition hands its marginals out
        losses, grad, blobs = ops.supervision_step(dev(logits), dev(images), dev(labels), dev(cues), want_blobs=True,
                                                   scale_factor=scale_factor, maxiter=maxiter)
        hip_refined = blobs["refined"].cpu().numpy()
    probs = O.softmax_forward(logits)
    refined, logq = O.crf_refine_batch(probs, images, scale_factor, maxiter)           # clips probs in place
    gp = blobs["probs"].cpu().numpy()
    assert np.abs(gp - probs).max() < 1e-6 and gp.min() >= np.float32(1e-4)
    assert np.abs(hip_refined - refined).max() < CRF_TOL
    assert np.abs(np.exp(blobs["logq"].cpu().numpy()) - refined).max() < CRF_TOL
    nflip, _, seeds = seeds_match_or_borderline(O, blobs["seeds"].cpu().numpy(), labels, cues, refined, hip_refined, tag=tag)
    l_seed, g_seed = O.seed_loss(probs, seeds)
    l_con, g_p, g_lq = O.constrain_loss(probs, logq)
    want_grad = O.softmax_backward(logits, g_seed + g_p + O.crf_layer_backward(refined, g_lq))
    # float32 sums in the reference's order on both sides: 1e-7 / 5e-7 of the maximum observed over the randomised sweeps
    # (profiles/r03_parity_sweeps.txt); the bars leave one order of magnitude
    assert abs(losses[0].item() - l_seed) < 1e-6 * max(1, abs(l_seed))
    assert abs(losses[1].item() - l_con) < 1e-6 * max(1, abs(l_con))
    assert np.abs(grad.cpu().numpy() - want_grad).max() < 1e-5 * np.abs(want_grad).max()
    return nflip


def test_supervision_step_vs_oracle_composition(ops, O):
    b = S.make_batch(21, 4)
    _check_fused_step(ops, O, b["logits"], b["images"], b["labels"], b["cues"], "fused B=4")
    assert (O.softmax_forward(b["logits"]) < 1e-4).any()               # the clip floor is exercised


def test_prepared_lattices_on_side_stream(ops):
    """dsrg_crf_prepare_batch on a side stream + supervision_step(prepared) == the one-call path."""
    b = S.make_batch(23, 3)
    args = [dev(b[k]) for k in ("logits", "images", "labels", "cues")]
    ctx = ops.get_context(3, 21, 41, 41)
    l0, g0, _ = ops.supervision_step(*args, ctx=ctx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.crf_prepare(args[1], 21, 41, 41, ctx=ctx)
    torch.cuda.current_stream().wait_stream(side)
    l1, g1, _ = ops.supervision_step(*args, ctx=ctx, prepared=True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    from dsrg_amd import _lib
    with pytest.raises(_lib.DsrgError):                      # prepared lattices are single-use
        ops.supervision_step(*args, ctx=ctx, prepared=True)
    # the same for the CRF layer alone (bench.py --mode infer)
    from oracle import oracle as O
    probs = O.softmax_forward(b["logits"])
    r0, q0 = ops.crf_refine(dev(probs), args[1], ctx=ctx)
    side.wait_stream(torch.cuda.current_stream())            # the call above still reads the context's lattices
    with torch.cuda.stream(side):
        ops.crf_prepare(args[1], 21, 41, 41, ctx=ctx)
    torch.cuda.current_stream().wait_stream(side)
    r1, q1 = ops.crf_refine(dev(probs), args[1], ctx=ctx, prepared=True)
    assert torch.equal(r0, r1) and torch.equal(q0, q1)


def test_autograd_function(ops):
    from dsrg_amd.ops import dsrg_supervision_loss
    b = S.make_batch(22, 2)
    x = dev(b["logits"]).requires_grad_(True)
    total, losses = dsrg_supervision_loss(x, dev(b["images"]), dev(b["labels"]), dev(b["cues"]))
    (2.0 * total).backward()
    _, grad, _ = ops.supervision_step(dev(b["logits"]), dev(b["images"]), dev(b["labels"]), dev(b["cues"]))
    assert torch.allclose(x.grad, 2.0 * grad)
    assert abs(total.item() - losses.sum().item()) < 1e-6


# ---------------------------------------------------------------- size-independent properties
def test_crf_label_permutation_equivariance_on_gpu(ops, O):
    b = S.make_batch(31, 2)
    probs = O.softmax_forward(b["logits"])
    perm = np.random.default_rng(0).permutation(21)
    r1, _ = ops.crf_refine(dev(probs), dev(b["images"]), 12.0, 10)
    r2, _ = ops.crf_refine(dev(probs[:, perm]), dev(b["images"]), 12.0, 10)
    # the label sum inside expAndNormalize runs in label order, so a permutation reorders float
    # additions; ten mean-field iterations amplify that to ~2e-5 at undecided pixels (the CPU
    # oracle shows the same 1.9e-5 on this input)
    assert np.abs(r1.cpu().numpy()[:, perm] - r2.cpu().numpy()).max() < 1e-4


def test_unsupported_sizes_fail_loudly(ops):
    """a context's size limit is a function of the map size alone (include/dsrg_hip.h: DSRG_CTX_MAX_PIXELS) and is met at
    creation, with a message — never by an unlucky batch in the middle of a run"""
    from dsrg_amd import _lib
    with pytest.raises(_lib.DsrgError):
        ops.Context(1, 21, 321, 321)          # full-resolution lattice: not on the LDS-resident path
    assert ops.LDS_PATH_MAX_PIXELS == 4488
    ops.Context(1, 21, 66, 68)                # 4488 pixels: the largest map of the path
    with pytest.raises(_lib.DsrgError, match="4489 pixels"):
        ops.Context(1, 21, 67, 67)
    # ... whatever the image: a noise image (largest lattice a map can have) at the limit runs
    b = S.make_batch(3, 1, H=66, W=68, size=66 * 8 - 7, image_kind="noise")
    refined, _ = ops.crf_refine(ops.softmax_forward(dev(b["logits"])), dev(b["images"]))
    assert torch.isfinite(refined).all()


def test_supervision_step_beyond_the_lds_path_vs_oracle(ops, O):
    """maps beyond DSRG_CTX_MAX_PIXELS (round-4 review, weak 11): supervision_step / crf_refine no longer fail there — the same
    five layers run on the global-memory path (batched full-resolution CRF + the stand-alone layer kernels, dsrg_amd/ops.py) —
    against the oracle layer by layer, as the fused step is checked: 70x70 maps of 553x553 images, and a 75x69 map"""
    for seed, B, H, W in [(11, 2, 70, 70), (12, 1, 75, 69)]:
        b = S.make_batch(seed, B, H=H, W=W, size=max(H, W) * 8 - 7)
        b["images"] = np.ascontiguousarray(b["images"][:, :, :H * 8 - 7, :W * 8 - 7])
        _check_fused_step(ops, O, b["logits"], b["images"], b["labels"], b["cues"], "large %dx%d" % (H, W))


def test_gemm_conv_matches_miopen_conv():
    """backbone plumbing: the im2col+GEMM forward equals nn.Conv2d (bf16 rounding), backward identical path"""
    from dsrg_amd.backbone import GemmConv2d
    torch.manual_seed(0)
    for cin, cout, k, d, relu, gemm in [(32, 48, 3, 1, False, True), (32, 48, 3, 6, True, True), (64, 21, 1, 1, False, True),
                                        (64, 64, 1, 1, True, True), (3, 64, 3, 1, True, False), (16, 24, 3, 2, True, True),
                                        (64, 1024, 3, 12, True, True)]:      # wide output: GEMM data AND weight gradients
        a = GemmConv2d(cin, cout, k, padding=d * (k // 2), dilation=d, fuse_relu=relu, gemm=gemm).cuda().to(memory_format=torch.channels_last)
        b = torch.nn.Conv2d(cin, cout, k, padding=d * (k // 2), dilation=d).cuda().to(memory_format=torch.channels_last)
        b.load_state_dict(a.state_dict())
        x = torch.randn(2, cin, 41, 41, device="cuda").contiguous(memory_format=torch.channels_last)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ya, yb = a(xa), b(xb)
            if relu:
                yb = torch.relu(yb)
        assert (ya.float() - yb.float()).abs().max() < 0.05 * yb.float().abs().max()
        g = torch.randn_like(yb)
        ya.backward(g.to(ya.dtype)); yb.backward(g)
        # with a ReLU the two paths can disagree on the sign of outputs that round to +-0: compare in the L2 sense
        def close(u, v, tol):
            return (u.float() - v.float()).norm() <= tol * v.float().norm() if relu else \
                (u.float() - v.float()).abs().max() < 0.05 * v.float().abs().max()
        if cin > 3:
            assert close(xa.grad, xb.grad, 0.03)
        assert close(a.weight.grad, b.weight.grad, 0.03)
        assert (a.bias.grad - b.bias.grad).norm() <= 0.03 * b.bias.grad.norm()


def test_relu_bwd_bias_and_maxpool_match_torch(ops):
    """backbone plumbing: the fused ReLU-backward/bias-gradient pass and the 3x3 max pooling pair against torch"""
    import torch.nn.functional as F
    torch.manual_seed(1)
    cl = torch.channels_last
    for B, C, H, W in [(2, 64, 33, 29), (1, 1024, 7, 5), (3, 24, 17, 17), (2, 512, 41, 41)]:
        y = torch.relu(torch.randn(B, C, H, W, device="cuda")).bfloat16().contiguous(memory_format=cl)
        g = torch.randn(B, C, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        gm, gb = ops.relu_bwd_bias(g, y)
        want = g * (y > 0)
        assert torch.equal(gm, want)
        ref = want.float().sum((0, 2, 3))
        assert (gb - ref).abs().max() <= 1e-4 * want.float().abs().sum((0, 2, 3)).max()
    for B, C, H, W in [(2, 21, 41, 41), (1, 5, 3, 7), (3, 256, 9, 9), (16, 21, 41, 41)]:
        g = torch.randn(B, C, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        gb = ops.bias_grad(g)
        ref = g.float().sum((0, 2, 3))
        assert (gb - ref).abs().max() <= 1e-4 * g.float().abs().sum((0, 2, 3)).max()
        assert torch.equal(gb, ops.bias_grad(g))                           # fixed summation order
    for B, C, H, W in [(2, 512, 41, 41), (1, 8, 1, 1), (2, 16, 2, 5), (1, 64, 7, 3)]:
        # reference in fp32 NCHW: PyTorch-ROCm 2.10's avg_pool2d BACKWARD is wrong for channels_last tensors (O(1) errors
        # against the CPU, f32 and bf16 alike), which is one more reason pool5a has its own kernel
        x = torch.randn(B, C, H, W, device="cuda").bfloat16()
        xr = x.float().requires_grad_(True)
        ref = F.avg_pool2d(xr, 3, 1, 1)
        out = ops.avgpool3x3_s1(x.contiguous(memory_format=cl))
        assert (out.float() - ref).abs().max() <= 0.01 * ref.abs().max() + 1e-6
        go = torch.randn_like(ref).bfloat16()
        ref.backward(go.float())
        gin = ops.avgpool3x3_s1(go.contiguous(memory_format=cl))
        assert (gin.float() - xr.grad).abs().max() <= 0.01 * xr.grad.abs().max() + 1e-6
    for B, C, H, W, stride, ceil in [(2, 64, 33, 29, 2, True), (2, 64, 321, 321, 2, True), (1, 8, 6, 6, 2, False),
                                     (2, 512, 41, 41, 1, False), (1, 16, 1, 1, 1, False), (1, 16, 2, 3, 2, True)]:
        x = torch.randn(B, C, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        out, code = ops.maxpool3x3_fwd(x, stride, ceil)
        xr = x.clone().requires_grad_(True)
        ref = F.max_pool2d(xr, 3, stride, 1, ceil_mode=ceil)
        assert out.shape == ref.shape, (out.shape, ref.shape)
        assert torch.equal(out, ref)
        go = torch.randn_like(ref)
        ref.backward(go)
        gin = ops.maxpool3x3_bwd(go, code, x.shape, stride)
        assert (gin.float() - xr.grad.float()).abs().max() <= 0.02 * xr.grad.float().abs().max()
        assert torch.equal(gin != 0, xr.grad != 0)


@pytest.mark.parametrize("B,C,HW", [(16, 21, (41, 41)), (20, 21, (41, 41)), (2, 30, (33, 29)), (2, 21, (65, 65)),
                                    (1, 21, (41, 41)), (3, 81, (41, 41))])
def test_fused_step_other_shapes_vs_oracle(ops, O, B, C, HW):
    """BASELINE configs[2]'s batch of 16, the reference's batch size 20, more than 21 labels (generic-width kernels),
    the 65x65 map of a 513x513 input, a lone image (BASELINE configs[1]; one label plane per workgroup), and the 81-label
    blobs of AnnotationLayerCOCO (pylayers.py:389-512) through the fused step, against the oracle layer by layer"""
    H, W = HW
    rng = np.random.default_rng(B * 1000 + C)
    size = 8 * (H - 1) + 1
    images = S.make_images(rng, B, size=size)
    logits = S.make_logits(rng, B, C, H, W)
    labels, cues = S.make_labels_cues(rng, B, C, H, W)
    _check_fused_step(ops, O, logits, images, labels, cues, "fused B=%d C=%d %dx%d" % (B, C, H, W))


@pytest.mark.parametrize("HW,scale,maxiter", [((41, 41), 12.0, 0), ((41, 41), 12.0, 1), ((41, 41), 3.0, 10), ((41, 41), 1.0, 2),
                                              ((70, 70), 3.0, 1)])
def test_fused_step_off_the_default_crf_arguments(ops, O, HW, scale, maxiter):
    """the fused step with other CRF arguments than (12, 10), B = 2, 21 labels: no iteration at all (the first update launch
    writes the marginals and their logarithm, the softmax pass leaves Q0 out), a first iteration that is also the last, and
    scales 3 and 1, whose Gaussian lattice is not pixel-local (its workgroups are in the filter grid); 70x70: the global-memory
    composition.  Against the oracle layer by layer, every bar as at the defaults."""
    H, W = HW
    rng = np.random.default_rng(7000 + 100 * int(scale) + maxiter + H)
    images = S.make_images(rng, 2, size=8 * (H - 1) + 1, kind="smooth" if maxiter else "noise")
    logits = S.make_logits(rng, 2, 21, H, W)
    labels, cues = S.make_labels_cues(rng, 2, 21, H, W)
    _check_fused_step(ops, O, logits, images, labels, cues, "fused %dx%d scale %g, %d iterations" % (H, W, scale, maxiter),
                      scale_factor=scale, maxiter=maxiter)


@pytest.mark.parametrize("seed", [50_002, 50_005, 50_011, 50_024, 50_027, 50_049, 50_054])
def test_fused_step_random_shapes_vs_oracle(ops, O, seed):
    """a slice of tools/parity_sweep_shapes.py in the suite: random batch, label count (2..96) and map size (2..65 a side),
    images without background, cues of absent classes — the fused step against the oracle layer by layer.  (The sweep over
    shapes, not data, is what found this round's allocation bug of the global-memory path.)"""
    rng = np.random.default_rng(seed)
    B, C = int(rng.integers(1, 7)), int(rng.choice([2, 3, 5, 21, 21, 21, 30, 64, 81, 96]))
    H, W = int(rng.integers(2, 66)), int(rng.integers(2, 66))
    size = 8 * (max(H, W) - 1) + 1
    kind = ["smooth", "noise", "dark_corner"][seed % 3]
    images = np.ascontiguousarray(S.make_images(rng, B, size=size, kind=kind)[:, :, :8 * (H - 1) + 1, :8 * (W - 1) + 1])
    logits = S.make_logits(rng, B, C, H, W, gain=float(rng.uniform(2, 60)), sigma=float(rng.uniform(1, 8)))
    labels = np.zeros((B, 1, 1, C), np.float32)
    cues = np.zeros((B, C, H, W), np.float32)
    for b in range(B):
        pres = rng.choice(C, size=int(rng.integers(1, min(C, 7) + 1)), replace=False)
        if rng.random() < 0.7:
            pres[0] = 0
        labels[b, 0, 0, np.unique(pres)] = 1.0
        for c in rng.choice(C, size=min(C, len(pres) + 2), replace=False):
            for _ in range(int(rng.integers(0, 4))):
                h, w = int(rng.integers(1, max(2, H // 3 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
                y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                cues[b, c, y:y + h, x:x + w] = 1.0
    _check_fused_step(ops, O, logits, images, labels, cues, "fused random shape seed %d: B=%d C=%d %dx%d" % (seed, B, C, H, W))


def test_unused_pylayers_vs_oracle(ops, O):
    """SeedLossLayer, ExpandLossLayer (sort-weighted pooling) and the evaluation histogram on the GPU"""
    rng = np.random.default_rng(11)
    for B, C, H, W in [(3, 21, 41, 41), (2, 21, 65, 65), (2, 5, 9, 11)]:
        logits = S.make_logits(rng, B, C, H, W, gain=6.0, sigma=2.0)
        _, cues = S.make_labels_cues(rng, B, C, H, W)
        p = O.softmax_forward(logits)
        want_l, want_g = O.seed_loss_plain(p, cues)
        loss, grad = ops.seed_loss_plain(dev(p), dev(cues))
        assert abs(loss.item() - want_l) < 1e-5 * max(1, abs(want_l))
        assert np.abs(grad.cpu().numpy() - want_g).max() < 1e-5 * max(1.0, np.abs(want_g).max())
        stat = (rng.random((B, 1, 1, C)) < 0.3).astype(np.float32)
        stat[:, 0, 0, 1] = 1.0                                           # at least one present and one absent class
        stat[:, 0, 0, 2] = 0.0
        want_l, want_g = O.expand_loss(p, stat)
        loss, grad = ops.expand_loss(dev(p), dev(stat))
        assert abs(loss.item() - want_l) < 1e-5 * max(1, abs(want_l)), (loss.item(), want_l)
        assert np.abs(grad.cpu().numpy() - want_g).max() < 1e-5 * max(1.0, np.abs(want_g).max())
        l2, g2 = ops.expand_loss(dev(p), dev(stat))                       # deterministic
        assert l2.item() == loss.item() and torch.equal(g2, grad)
    # ties: a constant plane keeps the stable pixel order of the oracle's sort
    p = np.full((1, 3, 4, 4), 1.0 / 3, np.float32)
    stat = np.array([1, 1, 0], np.float32).reshape(1, 1, 1, 3)
    want_l, want_g = O.expand_loss(p, stat)
    loss, grad = ops.expand_loss(dev(p), dev(stat))
    assert abs(loss.item() - want_l) < 1e-6 and np.abs(grad.cpu().numpy() - want_g).max() < 1e-7
    n = 21
    gt = rng.integers(0, n, size=200000).astype(np.uint8)
    gt[rng.random(gt.size) < 0.1] = 255
    pred = rng.integers(0, n, size=gt.size).astype(np.uint8)
    h = ops.confusion_matrix(dev(gt, torch.uint8), dev(pred, torch.uint8), n).cpu().numpy()
    assert h[-1] == 0 and np.array_equal(h[:-1].reshape(n, n).astype(np.float64), O.confusion_matrix(gt, pred, n))
    from dsrg_amd.inference import ConfusionMatrix
    cm = ConfusionMatrix(n)
    cm.add_device(dev(gt[:1000], torch.uint8), dev(pred[:1000], torch.uint8))
    cm.add_device(dev(gt[1000:], torch.uint8), dev(pred[1000:], torch.uint8))
    assert np.array_equal(cm.M, O.confusion_matrix(gt, pred, n))
    gt2 = gt.copy(); gt2[:50] = 60
    h = ops.confusion_matrix(dev(gt2, torch.uint8), dev(pred, torch.uint8), n, rule_lt=True).cpu().numpy()
    assert np.array_equal(h[:-1].reshape(n, n).astype(np.float64), O.confusion_matrix(gt2, pred, n, rule_lt=True))


def test_object_api_accepts_device_pointers(O):
    """the DenseCRF object with CUDA tensors in and out equals the numpy form bit for bit (small and large path)"""
    import krahenbuhl2013
    for (H, W, C, scale) in [(41, 41, 21, 12.0), (90, 110, 6, 1.0)]:
        rng = np.random.default_rng(H)
        img = S.make_images(rng, 1, size=max(H, W))[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
        im = np.ascontiguousarray(np.transpose(img, (1, 2, 0))).astype(np.uint8)
        un = np.log(np.ascontiguousarray(np.transpose(np.maximum(O.softmax_forward(S.make_logits(rng, 1, C, H, W))[0], 1e-4), (1, 2, 0))))
        q = krahenbuhl2013.CRF(im, un, scale_factor=scale)
        qd = krahenbuhl2013.CRF_device(torch.from_numpy(im).cuda(), torch.from_numpy(un).cuda(), scale_factor=scale)
        assert qd.is_cuda and np.array_equal(qd.cpu().numpy(), q)
        lab = krahenbuhl2013.CRF_device(torch.from_numpy(im).cuda(), torch.from_numpy(un).cuda(), scale_factor=scale, want="map")
        assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), q.argmax(2))


def test_error_paths_return_codes(ops):
    """wrong shapes / NULL pointers / unsupported sizes come back as DsrgError with a message, never as a crash"""
    import ctypes
    from dsrg_amd import _lib
    L = _lib.lib()
    x = torch.zeros(2, 21, 41, 41, device="cuda")
    assert L.dsrg_softmax_forward(2, 21, 1681, None, ctypes.c_void_p(x.data_ptr()), None) != 0
    assert b"" != L.dsrg_last_error()
    h = ctypes.c_void_p()
    assert L.dsrg_crf_create(0, 5, 3, ctypes.byref(h)) != 0
    assert L.dsrg_crf_create(5, 5, 100, ctypes.byref(h)) != 0                 # more than 96 labels
    with pytest.raises(ValueError):
        ops.supervision_step(x, torch.zeros(1, 3, 321, 321, device="cuda"), torch.zeros(2, 1, 1, 21, device="cuda"),
                             torch.zeros(2, 21, 41, 41, device="cuda"))            # batch mismatch images vs logits
    with pytest.raises(ValueError):
        ops.srg_grow(torch.zeros(2, 1, 1, 21, device="cuda"), x, torch.zeros(2, 21, 41, 41, device="cuda"))  # refined must be f64
    with pytest.raises(_lib.DsrgError):
        ops.expand_loss(torch.rand(1, 3, 100, 100, device="cuda"), torch.ones(1, 1, 1, 3, device="cuda"))   # plane > 8192 px
    from dsrg_amd.crf import DenseCRF
    c = DenseCRF(4, 4, 3)
    with pytest.raises(_lib.DsrgError):
        c.inference(5)                                                             # no pairwise energy yet
    with pytest.raises(ValueError):
        c.set_unary_energy(np.zeros(7, np.float32))


def test_backbone_runs_with_and_without_autocast():
    """the VGG16-ASPP net (GEMM convs, fused ReLU, HIP pooling) gives the same scores in plain fp32 (every fast path
    falls back to its torch form) and under bf16 autocast, and matches an nn.Conv2d/nn.ReLU/nn.MaxPool2d twin"""
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(0)
    net = VGG16ASPP().cuda().to(memory_format=torch.channels_last).eval()
    ref = VGG16ASPP(gemm_convs=False).cuda().eval()
    ref.load_state_dict(net.state_dict())
    x = torch.randn(2, 3, 97, 97, device="cuda")
    with torch.no_grad():
        y32 = net(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = net(x.contiguous(memory_format=torch.channels_last)).float()
        yr = ref(x)
    assert y32.shape == (2, 21, 13, 13)
    scale = yr.abs().max()
    assert (y32 - yr).abs().max() < 1e-3 * scale
    assert (y16 - yr).abs().max() < 0.05 * scale
    # training mode: gradients reach the first convolution through the fused backward kernels
    from dsrg_amd.backbone import GemmConv2d
    net.train()
    ref.train()
    for m in list(net.modules()) + list(ref.modules()):
        if isinstance(m, GemmConv2d):
            m.fuse_dropout = 0.0                         # dropout off: the two nets must see the same function
    g = torch.randn(2, 21, 13, 13, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        la = (net(x.contiguous(memory_format=torch.channels_last)).float() * g).sum()
        lb = (ref(x).float() * g).sum()
    la.backward(); lb.backward()
    # near the output the two bf16 routes agree closely; sixteen layers down the rounding differences have compounded
    for name, tol in [("branches.0.6.weight", 0.03), ("branches.2.3.weight", 0.05), ("branches.1.0.weight", 0.08),
                      ("features.28.weight", 0.15), ("features.17.weight", 0.4)]:
        ga, gb = dict(net.named_parameters())[name].grad, dict(ref.named_parameters())[name].grad
        assert torch.isfinite(ga).all() and (ga - gb).norm() < tol * gb.norm(), (name, float((ga - gb).norm() / gb.norm()))


def test_supervision_entry_points_capture_into_a_hip_graph(ops):
    """the batched entry points are stream-ordered and never synchronise, so a fixed-shape sequence can be
    captured into a hipGraph — here the lattice build on a side stream, Softmax, the ten mean-field iterations and region
    growing; the replay reproduces the launched path's seeds and marginals bit for bit, also on new inputs written in place"""
    from dsrg_amd import synthetic as S
    B = 2
    b = S.make_batch(77, B)
    d = lambda a: torch.from_numpy(a).cuda()
    logits, images, labels, cues = d(b["logits"]), d(b["images"]), d(b["labels"]), d(b["cues"])
    ctx = ops.get_context(B, 21, 41, 41)
    side = torch.cuda.Stream()

    def run():
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            ops.crf_prepare(images, 21, 41, 41, ctx=ctx)
        probs = ops.softmax_forward(logits)
        main.wait_stream(side)
        refined, _ = ops.crf_refine(probs, images, ctx=ctx, want_log=False, prepared=True)
        return ops.srg_grow(labels, cues, refined), refined
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        seeds_s, refined_s = run()
    for seed in (78, 79):
        nb = S.make_batch(seed, B)
        logits.copy_(d(nb["logits"])); images.copy_(d(nb["images"])); labels.copy_(d(nb["labels"])); cues.copy_(d(nb["cues"]))
        g.replay()
        seeds, refined = run()
        assert torch.equal(seeds_s, seeds) and torch.equal(refined_s, refined)


def test_fp32_heads_kernel_matches_fp32_convolutions(ops):
    """fc8-SEC_k + Eltwise SUM in one HIP pass (bf16 activations, fp32 weights/accumulation/result, NCHW) against the fp32
    1x1 convolutions of the same bf16-valued activations; the backward of the autograd wrapper against torch's"""
    import torch.nn.functional as F
    from dsrg_amd.backbone import _HeadsFn
    torch.manual_seed(7)
    for B, K, H, W, O, n in [(2, 1024, 41, 41, 21, 4), (1, 256, 5, 7, 32, 2), (3, 512, 9, 9, 3, 1), (16, 1024, 41, 41, 21, 4),
                             (1, 2048, 3, 3, 21, 3)]:
        xs = [torch.randn(B, K, H, W, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(n)]
        w = (torch.randn(n, O, K, device="cuda") * 0.05).requires_grad_(True)
        b = torch.randn(n, O, device="cuda").requires_grad_(True)
        want = sum(F.conv2d(x.float(), w[k].reshape(O, K, 1, 1), b[k]) for k, x in enumerate(xs))
        got = ops.heads_forward(xs, w.detach(), b.detach())
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (B, O, H, W)
        assert (got - want).abs().max() <= 2e-5 * want.abs().max()
        assert torch.equal(got, ops.heads_forward(xs, w.detach(), b.detach()))              # deterministic
        xa = [x.clone().requires_grad_(True) for x in xs]
        wa, ba = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        ya = _HeadsFn.apply(None, wa, ba, *xa)
        g = torch.randn_like(ya)
        ya.backward(g)
        xr = [x.float().requires_grad_(True) for x in xs]
        want2 = sum(F.conv2d(x, w[k].reshape(O, K, 1, 1), b[k]) for k, x in enumerate(xr))
        want2.backward(g)
        assert (wa.grad - w.grad).abs().max() <= 1e-4 * w.grad.abs().max()             # fp32 fma chains both sides
        assert (ba.grad - b.grad).norm() <= 1e-4 * b.grad.norm()
        for u, v in zip(xa, xr):
            assert u.grad.dtype == torch.bfloat16 and (u.grad.float() - v.grad).norm() <= 0.005 * v.grad.norm()   # one bf16 rounding


@pytest.mark.parametrize("cf,cb", [(64, 64), (128, 128), (128, 64), (64, 128)])
def test_direct_conv_data_gradient_absorbs_the_relu_backward(ops, cf, cb):
    """dsrg_conv3x3_direct_dgrad_bf16 == the plain direct convolution masked by (output of the layer below > 0) afterwards, and the
    bias gradient == the column sums of what was stored; ragged tiles, more tiles than workgroups"""
    torch.manual_seed(21)
    cl = torch.channels_last
    for B, H, W in [(2, 33, 29), (1, 8, 16), (3, 161, 161)]:
        g = torch.randn(B, cf, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        wt = (torch.randn(cb, cf, 3, 3, device="cuda") * 0.05).bfloat16()
        y = torch.relu(torch.randn(B, cb, H, W, device="cuda")).bfloat16().contiguous(memory_format=cl)
        y.permute(0, 2, 3, 1).view(-1)[::41] = -0.0
        plain = ops.conv3x3_direct(g, wt, None, False)
        got, gb = ops.conv3x3_direct_dgrad(g, wt, y)
        want = torch.where(y > 0, plain, torch.zeros_like(plain))
        assert torch.equal(got, want) and got.is_contiguous(memory_format=cl)
        ref_b = want.float().sum((0, 2, 3))
        assert gb.dtype == torch.float32 and float((gb - ref_b).abs().max()) <= 2e-3 * float(ref_b.abs().max()) + 1e-4
        got2, gb2 = ops.conv3x3_direct_dgrad(g, wt, y)
        assert torch.equal(got, got2) and torch.equal(gb, gb2)                        # deterministic


def test_heads_backward_absorbs_the_relu_backward_of_its_inputs(ops):
    """dsrg_heads_backward_relu_bf16: data gradients masked by x_k > 0 and scaled == the plain ones pushed through
    ops.relu_bwd_bias' arithmetic (same bits for a power-of-two scale); the bias gradient of the layer below == column sums of
    what was stored; the weight gradient is untouched"""
    torch.manual_seed(9)
    for B, K, H, W, O, n, scale in [(2, 1024, 41, 41, 21, 4, 2.0), (1, 256, 5, 7, 32, 2, 1.0), (3, 512, 9, 15, 3, 1, 2.0)]:
        xs = [torch.relu(torch.randn(B, K, H, W, device="cuda")).bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(n)]
        for x in xs:
            x.permute(0, 2, 3, 1).view(-1)[::53] = -0.0
        w = torch.randn(n, O, K, device="cuda") * 0.05
        g = torch.randn(B, O, H, W, device="cuda")
        plain, gw0 = ops.heads_backward(xs, w, g)
        got, gw1, gb = ops.heads_backward(xs, w, g, True, scale)
        assert torch.equal(gw0, gw1) and gb.shape == (n, K) and gb.dtype == torch.float32
        for k in range(n):
            want = torch.where(xs[k] > 0, (plain[k].float() * scale).bfloat16(), torch.zeros_like(plain[k]))
            assert torch.equal(got[k], want)
            ref_b = want.float().sum((0, 2, 3))
            assert float((gb[k] - ref_b).abs().max()) <= 2e-3 * float(ref_b.abs().max()) + 1e-4


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (128, 64), (3, 64)])
def test_direct_conv_matches_torch(ops, cin, cout):
    """the direct 3x3 convolutions (one MFMA kernel, weights in registers) against F.conv2d in fp32 on the same bf16-valued
    operands: odd sizes, partial tiles, bias / ReLU, and the data-gradient form (flipped, transposed kernel)"""
    import torch.nn.functional as F
    torch.manual_seed(11)
    cl = torch.channels_last
    big = (1, 321, 321, True, True) if cout == 64 and cin in (3, 64) else (2, 161, 161, True, True)
    for B, H, W, relu, bias in [(2, 33, 29, True, True), (1, 8, 16, False, False), (3, 1, 1, True, True), big, (2, 17, 40, False, True)]:
        x = torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        w = (torch.randn(cout, cin, 3, 3, device="cuda") * 0.05).bfloat16()
        b = torch.randn(cout, device="cuda") if bias else None
        want = F.conv2d(x.float(), w.float(), b, padding=1)
        if relu:
            want = torch.relu(want)
        got = ops.conv3x3_direct(x, w, b, relu)
        assert got.shape == want.shape and got.dtype == torch.bfloat16 and got.is_contiguous(memory_format=cl)
        err = (got.float() - want).abs().max()
        assert err <= 0.01 * want.abs().max() + 1e-3, (B, H, W, float(err), float(want.abs().max()))
        assert torch.equal(got, ops.conv3x3_direct(x, w, b, relu))                    # deterministic
        if cin == 3:
            continue                                                                  # the image needs no gradient
        # data gradient of y = conv(x, w): conv(g, flip(w)^T)
        g = torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        xr = x.float().requires_grad_(True)
        F.conv2d(xr, w.float(), None, padding=1).backward(g.float())
        gx = ops.conv3x3_direct(g, w.flip(2, 3).transpose(0, 1).contiguous(), None, False)
        assert gx.shape == x.shape
        assert (gx.float() - xr.grad).abs().max() <= 0.01 * xr.grad.abs().max() + 1e-3


def test_lds_transposing_read_lane_map(ops):
    """the lane map the weight-gradient kernel assumes of ds_read_b64_tr_b16, checked through the smallest case that
    exercises it: one pixel row, delta inputs — gw[o][tap][c] must pick exactly x[px + tap][c] * g[px][o]"""
    cl = torch.channels_last
    for px, o, c in [(0, 0, 0), (5, 17, 33), (15, 63, 62), (9, 31, 16), (3, 48, 5)]:
        x = torch.zeros(1, 64, 1, 16, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=cl)
        g = torch.zeros_like(x)
        x[0, c, 0, px] = 2.0
        g[0, o, 0, px] = 3.0
        gw = ops.conv3x3_wgrad(x, g).float()
        want = torch.zeros(64, 64, 3, 3, device="cuda")
        want[o, c, 1, 1] = 6.0                                       # only the centre tap sees the same pixel
        assert torch.equal(gw, want), (px, o, c, gw.nonzero().tolist()[:8])


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (3, 64)])
def test_direct_conv_weight_gradient_matches_torch(ops, cin, cout):
    """the direct weight-gradient kernel (transposing LDS reads + MFMA, per-workgroup partials summed in a fixed order)
    against autograd through F.conv2d in fp32 on the same bf16-valued operands: partial tiles, one pixel, many tiles per
    workgroup, both slices of a 128-channel input"""
    import torch.nn.functional as F
    torch.manual_seed(5)
    cl = torch.channels_last
    big = (2, 321, 321) if cout == 64 else (4, 161, 161)
    for B, H, W in [(2, 33, 29), (1, 8, 16), (3, 1, 1), (2, 17, 40), big]:
        x = torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        g = (torch.randn(B, cout, H, W, device="cuda") * (torch.rand(B, cout, H, W, device="cuda") < 0.5)).bfloat16().contiguous(memory_format=cl)
        w = torch.zeros(cout, cin, 3, 3, device="cuda", requires_grad=True)
        F.conv2d(x.float(), w, None, padding=1).backward(g.float())
        got = ops.conv3x3_wgrad(x, g)
        assert got.shape == w.shape and got.dtype == torch.bfloat16
        err = (got.float() - w.grad).abs().max()
        assert err <= 0.006 * w.grad.abs().max() + 1e-3, (B, H, W, float(err), float(w.grad.abs().max()))   # one bf16 rounding of the sum
        assert torch.equal(got, ops.conv3x3_wgrad(x, g))                                                    # deterministic


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (3, 64)])
def test_narrow_conv_layers_differentiate_like_torch(ops, cin, cout):
    """conv1_2 / conv2_1 / conv2_2 as the backbone runs them (GemmConv2d + fused ReLU under autocast: direct forward, data and
    weight gradient kernels, fused ReLU-mask + bias gradient) against nn.Conv2d + relu differentiated by torch"""
    import torch.nn.functional as F
    from dsrg_amd.backbone import GemmConv2d
    torch.manual_seed(9)
    cl = torch.channels_last
    a = GemmConv2d(cin, cout, 3, padding=1, fuse_relu=True).cuda().to(memory_format=cl)
    b = torch.nn.Conv2d(cin, cout, 3, padding=1).cuda().to(memory_format=cl)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, cin, 37, 45, device="cuda").contiguous(memory_format=cl)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = a(xa)
        yb = torch.relu(b(xb))
    assert ya.dtype == torch.bfloat16 and (ya.float() - yb.float()).norm() <= 0.01 * yb.float().norm()
    g = torch.randn_like(yb)
    ya.backward(g.to(ya.dtype)); yb.backward(g)
    for u, v in [(xa.grad, xb.grad), (a.weight.grad, b.weight.grad), (a.bias.grad, b.bias.grad)]:
        assert u.shape == v.shape and (u.float() - v.float()).norm() <= 0.02 * v.float().norm()


def test_pool_backward_with_fused_relu_mask_and_bias_gradient(ops):
    """conv + ReLU + stride-2 max pool as one node: the fused backward pass (pool backward, ReLU mask, bias gradient) writes the
    same masked gradient, bit for bit, as maxpool3x3_bwd followed by relu_bwd_bias; then the module against torch's sequence"""
    import torch.nn.functional as F
    from dsrg_amd.backbone import GemmConv2d
    torch.manual_seed(13)
    cl = torch.channels_last
    for B, C, H, W, ceil in [(2, 64, 33, 29, True), (1, 128, 6, 6, False), (2, 256, 41, 40, True), (16, 64, 321, 321, True), (1, 8, 2, 3, True)]:
        y = torch.relu(torch.randn(B, C, H, W, device="cuda")).bfloat16().contiguous(memory_format=cl)
        pooled, code = ops.maxpool3x3_fwd(y, 2, ceil)
        go = torch.randn_like(pooled)
        g_ref, gb_ref = ops.relu_bwd_bias(ops.maxpool3x3_bwd(go, code, y.shape, 2), y, 1.0)
        g, gb = ops.maxpool3x3_bwd_relu(go, code, y, 2)
        assert torch.equal(g, g_ref), (B, C, H, W)
        assert (gb - gb_ref).abs().max() <= 1e-4 * gb_ref.abs().max() + 1e-4                    # fp32 sums, other grouping
        # the mask inside the window codes (round 5): windows without a positive value get a code that names no position, and
        # the backward runs without the pool's input — same pooled values, same gradient and bias gradient, bit for bit.  A third
        # of the planes are zeroed so that whole windows are dead
        y[:, ::3] = 0
        pooled, code = ops.maxpool3x3_fwd(y, 2, ceil)
        pooled_m, code_m = ops.maxpool3x3_fwd(y, 2, ceil, relu_input=True)
        assert torch.equal(pooled, pooled_m)
        dead = code_m.permute(0, 3, 1, 2) == 0xfe
        assert torch.equal(dead, pooled <= 0) and bool(dead.any()) and torch.equal(code_m.permute(0, 3, 1, 2)[~dead], code.permute(0, 3, 1, 2)[~dead])
        g_y, gb_y = ops.maxpool3x3_bwd_relu(go, code, y, 2)
        g_m, gb_m = ops.maxpool3x3_bwd_relu(go, code_m, tuple(y.shape), 2)
        assert torch.equal(g_m, g_y) and torch.equal(gb_m, gb_y), (B, C, H, W)
    from dsrg_amd.backbone import _pool3x3
    for cin, cout in [(64, 64), (128, 128), (256, 256)]:
        a = GemmConv2d(cin, cout, 3, padding=1, fuse_relu=True, fuse_pool=(2, True)).cuda().to(memory_format=cl)
        b = GemmConv2d(cin, cout, 3, padding=1, fuse_relu=True).cuda().to(memory_format=cl)      # the same convolution, pool as a node of its own
        c = torch.nn.Conv2d(cin, cout, 3, padding=1).cuda().to(memory_format=cl)
        b.load_state_dict(a.state_dict()); c.load_state_dict(a.state_dict())
        x = torch.randn(2, cin, 37, 45, device="cuda").contiguous(memory_format=cl)
        xa, xb, xc = (x.clone().requires_grad_(True) for _ in range(3))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ya = a(xa)
            yb = _pool3x3(b(xb), 2, True)
            yc = F.max_pool2d(torch.relu(c(xc)), 3, 2, 1, ceil_mode=True)
        assert torch.equal(ya, yb)
        assert ya.shape == yc.shape and (ya.float() - yc.float()).norm() <= 0.01 * yc.float().norm()
        g = torch.randn_like(yc)
        ya.backward(g.to(ya.dtype)); yb.backward(g.to(yb.dtype)); yc.backward(g)
        assert torch.equal(xa.grad, xb.grad) and torch.equal(a.weight.grad, b.weight.grad)       # the same masked gradient into the same kernels
        assert (a.bias.grad - b.bias.grad).abs().max() <= 1e-4 * b.bias.grad.abs().max() + 1e-4
        # against torch's conv -> relu -> max_pool2d only loosely: two convolution kernels round a few outputs differently, and a
        # window whose two largest values swap order routes its gradient to another pixel
        for u, v in [(xa.grad, xc.grad), (a.weight.grad, c.weight.grad), (a.bias.grad, c.bias.grad)]:
            assert u.shape == v.shape and (u.float() - v.float()).norm() <= 0.15 * v.float().norm()
        with torch.no_grad():                                                                    # float32 / no autocast: the pool runs behind the node
            assert a(x).shape == ya.shape


def test_fused_relu_dropout_backward_matches_unfused_sequence():
    """conv + ReLU + Dropout in one autograd function: same dropout mask as F.dropout under the same seed, and the fused
    backward (one pass reading the sign of the dropped output) equals conv -> relu -> dropout differentiated by torch"""
    import torch.nn.functional as F
    from dsrg_amd.backbone import GemmConv2d
    for k, d in [(3, 6), (1, 1)]:
        torch.manual_seed(3)
        a = GemmConv2d(64, 128, k, padding=d * (k // 2), dilation=d, fuse_relu=True, fuse_dropout=0.5).cuda().to(
            memory_format=torch.channels_last).train()
        b = torch.nn.Conv2d(64, 128, k, padding=d * (k // 2), dilation=d).cuda().to(memory_format=torch.channels_last)
        b.load_state_dict(a.state_dict())
        x = torch.randn(2, 64, 41, 41, device="cuda").contiguous(memory_format=torch.channels_last)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            torch.manual_seed(11)
            ya = a(xa)
            torch.manual_seed(11)
            yb = F.dropout(torch.relu(b(xb)), 0.5, True)
        zero_a, zero_b = ya == 0, yb == 0
        assert (zero_a != zero_b).float().mean() < 0.01            # same mask (the two convs may disagree on a few signs)
        g = torch.randn_like(yb)
        ya.backward(g.to(ya.dtype)); yb.backward(g)
        for u, v in [(xa.grad, xb.grad), (a.weight.grad, b.weight.grad), (a.bias.grad, b.bias.grad)]:
            assert (u.float() - v.float()).norm() <= 0.03 * v.float().norm()
    a.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y1, y2 = a(x), a(x)
    assert torch.equal(y1, y2)                                      # no dropout in eval mode


@pytest.mark.parametrize("train_affine,size", [(True, 65), (False, 257)])
def test_resnet_folded_bn_path_matches_unfused_reference(train_affine, size):
    """train-f's ResNet-101: conv + frozen BN (+ ReLU) folded into one GEMM on the GPU against the plain
    conv -> affine -> relu sequence in fp32 on the CPU, forward and the gradients.  train_affine: gamma and beta train (im2col +
    library GEMM, the affine folded into the weights by autograd); otherwise (the default) the BatchNorm layers are constant maps
    and the bottlenecks whose channel counts the kernels take run on the implicit-GEMM kernels — scale in the packed kernel,
    shift as the epilogue's bias, relu(y + identity) in one pass: at 257 x 257 the res3 .. res5 maps have 2 178 pixels, enough
    for that route to be taken (checked: the nodes are in the graph)"""
    from dsrg_amd import retrain as R
    torch.manual_seed(0)
    ref = R.ResNet101DeepLab(blocks=(1, 1, 1, 1), train_bn_affine=train_affine)
    with torch.no_grad():
        for m in ref.modules():                      # non-trivial statistics and affine parameters
            if isinstance(m, R._FrozenBN):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    net = R.ResNet101DeepLab(blocks=(1, 1, 1, 1), train_bn_affine=train_affine)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, size, size)
    h = (size - 1) // 8 + 1
    g = torch.randn(2, 21, h, h)
    yr = ref(x)
    (yr * g).sum().backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(x.cuda().contiguous(memory_format=torch.channels_last))
        yg = out.float()
    if not train_affine:                             # the implicit-GEMM nodes and the fused block tails are what ran
        seen, todo = set(), [out.grad_fn]
        while todo:
            f = todo.pop()
            if f is None or f in seen:
                continue
            seen.add(f)
            todo.extend(nf for nf, _ in f.next_functions)
        names = [type(f).__name__ for f in seen]
        # (every block has the shortcut in its last convolution's store — res2's 64-channel 1x1 layers run the kernels' half-empty tiles)
        assert sum(n.startswith("_FoldedIgemmFn") for n in names) >= 12 and sum(n.startswith("_AddReLUFn") for n in names) == 0, names
    (yg * g.cuda()).sum().backward()
    assert yg.shape == yr.shape
    assert (yg.cpu() - yr).norm() < 0.05 * yr.norm()
    pr, pg = dict(ref.named_parameters()), dict(net.named_parameters())
    affine = ["layers.3.b3.weight", "layers.3.b3.bias", "layers.2.b2.weight", "layers.1.b1.bias", "layers.0.b2.weight"]
    for name in ["layers.3.c3.weight", "layers.3.c1.weight", "layers.3.down.0.weight", "layers.2.c2.weight", "layers.2.c3.weight",
                 "layers.1.c1.weight", "layers.1.c2.weight", "layers.0.down.0.weight", "aspp.2.weight"] + (affine if train_affine else []):
        a, b = pg[name].grad.float().cpu(), pr[name].grad
        assert torch.isfinite(a).all() and (a - b).norm() < 0.15 * b.norm(), (name, float((a - b).norm() / b.norm()))
    if not train_affine:
        assert all(pg[n].grad is None and not pg[n].requires_grad for n in affine)


def test_igemm_residual_store_equals_the_separate_passes(ops):
    """ops.conv_igemm_residual (the shortcut of a residual block in the convolution's store) against the passes it replaces, bit for
    bit: forward = conv_igemm + add_relu; data gradient = conv_igemm + bf16 add + relu_mask.  1x1 and dilated 3x3 (class-ordered
    tiles), pixel counts that are no multiple of the 256-pixel tile, a 128-channel output (half-idle channel tile)"""
    torch.manual_seed(11)
    cl = torch.channels_last
    for B, cin, cout, H, W, k, d in [(2, 128, 512, 33, 33, 1, 1), (3, 256, 256, 29, 31, 3, 12), (2, 512, 128, 33, 35, 1, 1), (1, 64, 256, 41, 41, 3, 1),
                                     (2, 256, 64, 37, 35, 1, 1), (1, 64, 64, 50, 41, 1, 1)]:      # (64 outputs: half-empty channel tiles)
        x = torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        w = (torch.randn(cout, cin, k, k, device="cuda") * (1.0 / (cin * k * k) ** 0.5)).contiguous(memory_format=cl)
        bias = torch.randn(cout, device="cuda")
        res = torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        below = torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        pk = ops.pack_conv_weight(w)
        (plain,) = ops.conv_igemm([x], [pk], [bias], [d], k, False)
        ref = torch.nn.functional.conv2d(x.float(), w.bfloat16().float(), bias, padding=d * (k // 2), dilation=d)
        assert (plain.float() - ref).abs().max() <= 0.02 * ref.abs().max()
        assert torch.equal(ops.conv_igemm_residual(x, pk, bias, res, None, d, k, True), ops.add_relu(plain, res))
        assert torch.equal(ops.conv_igemm_residual(x, pk, bias, res, None, d, k, False), (plain.float() + res.float()).bfloat16())
        (nob,) = ops.conv_igemm([x], [pk], None, [d], k, False)
        want = ops.relu_mask((nob.float() + res.float()).bfloat16(), below)
        assert torch.equal(ops.conv_igemm_residual(x, pk, None, res, below, d, k, False), want)
        (gxm,), (gb,) = ops.conv_igemm_dgrad([x], [pk], [below], [d], k, 1.0, bias_grad=True)      # mask + column sums at this width
        assert torch.equal(gxm, ops.relu_mask(nob, below)) and (gb - gxm.float().sum((0, 2, 3))).abs().max() <= 2e-3 * gxm.float().abs().sum((0, 2, 3)).max()
    with pytest.raises(ValueError):
        ops.conv_igemm_residual(x, pk, None, res[:, :, 1:], None, d, k, False)


def test_igemm_backward_residual_and_scaled_pack(ops):
    """dsrg_conv_igemm_backward_residual_bf16 (a bottleneck convolution's whole backward: merged grid for 1x1 and 3x3 dilation < 3, two
    launches for dilation 4) against its pieces — data gradient bit-equal to conv_igemm_residual / conv_igemm_dgrad / conv_igemm, weight
    gradient = conv_igemm_wgrad times the per-output scale up to fp32 reassociation (another pixel split); and the scaled pack against
    multiply-then-pack, bit for bit"""
    torch.manual_seed(13)
    cl = torch.channels_last
    for B, cin, cout, H, W, k, d in [(2, 256, 1024, 33, 33, 1, 1), (2, 256, 256, 33, 35, 3, 2), (2, 512, 512, 33, 33, 3, 4), (3, 1024, 256, 29, 31, 1, 1)]:
        x = torch.relu(torch.randn(B, cin, H, W, device="cuda")).bfloat16().contiguous(memory_format=cl)
        g = torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        res = torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
        w = (torch.randn(cout, cin, k, k, device="cuda") * (1.0 / (cin * k * k) ** 0.5)).contiguous(memory_format=cl)
        scale = torch.rand(cout, device="cuda") + 0.5
        pf, pd = ops.pack_conv_weight_pair(w, True, True, scale)
        ws = (w * scale.view(-1, 1, 1, 1)).contiguous(memory_format=cl)
        assert torch.equal(pf, ops.pack_conv_weight(ws)) and torch.equal(pd, ops.pack_conv_weight(ws, for_dgrad=True))
        (gw_ref,) = ops.conv_igemm_wgrad([x], [g], [d], k)
        gw_ref = gw_ref * scale.view(-1, 1, 1, 1)
        for mask, r in [(x, res), (None, res), (x, None), (None, None)]:
            gx, gw = ops.conv_igemm_backward_residual(g, pd, x, d, k, mask, r, scale)
            if r is not None:
                want = ops.conv_igemm_residual(g, pd, None, r, mask, d, k, False)
            elif mask is not None:
                want = ops.conv_igemm_dgrad([g], [pd], [mask], [d], k, 1.0, bias_grad=False)[0][0]
            else:
                want = ops.conv_igemm([g], [pd], None, [d], k, False)[0]
            assert torch.equal(gx, want)
            assert gw.is_contiguous(memory_format=cl) and (gw - gw_ref).abs().max() <= 2e-5 * gw_ref.abs().max() + 1e-6
        slot = torch.zeros_like(w)
        _, gw2 = ops.conv_igemm_backward_residual(g, pd, x, d, k, x, res, scale, gw_out=slot)
        assert gw2 is slot and torch.equal(slot, gw)


def test_resnet_shortcut_in_the_store_is_bit_identical_to_the_separate_passes(monkeypatch):
    """three bottlenecks (projection shortcut, then two identity shortcuts) with the shortcut's add + ReLU in the last convolution's
    store and its backward in the first convolution's data gradient (retrain._FUSE_RES) against the same blocks with add_relu /
    relu_mask passes and autograd's accumulation: outputs, input gradient and every weight gradient bit-equal; the fused graph has
    no _AddReLUFn node"""
    from dsrg_amd import retrain as R
    torch.manual_seed(5)
    blocks = torch.nn.Sequential(R._Bottleneck(256, 128, 1, 2, True, False), R._Bottleneck(512, 128, 1, 2, False, False),
                                 R._Bottleneck(512, 128, 1, 4, False, False)).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in blocks.modules():
            if isinstance(m, R._FrozenBN):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    x0 = torch.randn(2, 256, 33, 35, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, 512, 33, 35, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(R, "_FUSE_RES", fused)
        for p in blocks.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        y = blocks(x)
        seen, todo = set(), [y.grad_fn]
        while todo:
            f = todo.pop()
            if f is not None and f not in seen:
                seen.add(f)
                todo.extend(nf for nf, _ in f.next_functions)
        n_add = sum(type(f).__name__.startswith("_AddReLUFn") for f in seen)
        assert n_add == (0 if fused else 3)
        y.backward(g)
        runs.append((y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in blocks.named_parameters() if p.grad is not None}))
    (ya, xa, ga), (yb, xb, gb) = runs
    assert torch.equal(ya, yb) and torch.equal(xa, xb)
    assert set(ga) == set(gb) and len(ga) == 10
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    with torch.no_grad():                                # inference takes the fused store too
        monkeypatch.setattr(R, "_FUSE_RES", True)
        assert torch.equal(blocks(x0), ya)


def test_aspp_head_as_one_1x1_product_plus_shifted_gather(ops):
    """the ResNet ASPP head (four dilated 3x3 classifiers of one map, summed) as ONE 1x1 convolution + ops.aspp_shift_sum, backward by
    ops.aspp_shift_gather + the 1x1 layer's merged backward (retrain._AsppFn): the two shift kernels against torch index arithmetic
    (exact), and the whole head — output, feature gradient, every kernel's and bias's gradient — against F.conv2d in float32 on the
    same bf16-valued operands"""
    import torch.nn.functional as F
    from dsrg_amd import retrain as R
    torch.manual_seed(21)
    cl = torch.channels_last
    B, H, W, O, CT = 2, 19, 23, 5, 128
    offsets = [(-3, 0), (0, 2), (4, -5), (0, 0), (30, 0)]                               # (the last: every source outside the map)
    y = torch.randn(B, CT, H, W, device="cuda").bfloat16().contiguous(memory_format=cl)
    bias = torch.randn(O, device="cuda")
    got = ops.aspp_shift_sum(y, offsets, O, bias)
    want = bias.view(1, O, 1, 1).expand(B, O, H, W).clone()
    yf = y.float()
    for j, (dy, dx) in enumerate(offsets):
        src = torch.zeros(B, O, H, W, device="cuda")
        ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if ye > ys and xe > xs:
            src[:, :, ys:ye, xs:xe] = yf[:, j * O:(j + 1) * O, ys + dy:ye + dy, xs + dx:xe + dx]
        want = want + src
    assert torch.equal(got, want) and tuple(got.shape) == (B, O, H, W)
    g = torch.randn(B, O, H, W, device="cuda")
    gp = ops.aspp_shift_gather(g, offsets, CT)
    wantp = torch.zeros(B, CT, H, W, device="cuda")
    for j, (dy, dx) in enumerate(offsets):
        ys, ye, xs, xe = max(0, dy), min(H, H + dy), max(0, dx), min(W, W + dx)
        if ye > ys and xe > xs:
            wantp[:, j * O:(j + 1) * O, ys:ye, xs:xe] = g[:, :, ys - dy:ye - dy, xs - dx:xe - dx]
    assert torch.equal(gp, wantp.bfloat16()) and gp.is_contiguous(memory_format=cl)
    # the whole head
    B, cin, H, W, O, dils = 2, 256, 33, 35, 21, (6, 12, 18, 24)
    f = torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=cl).requires_grad_(True)
    ws = [(torch.randn(O, cin, 3, 3, device="cuda") * 0.02).bfloat16().float().contiguous(memory_format=cl).requires_grad_(True) for _ in dils]
    bs = [torch.randn(O, device="cuda").requires_grad_(True) for _ in dils]
    out = R._AsppFn.apply(dils, f, *ws, *bs)
    gout = torch.randn(B, O, H, W, device="cuda")
    out.backward(gout)
    f32 = f.detach().float().requires_grad_(True)
    ws32 = [w.detach().clone().requires_grad_(True) for w in ws]
    bs32 = [b.detach().clone().requires_grad_(True) for b in bs]
    ref = sum(F.conv2d(f32, w, b, padding=d, dilation=d) for w, b, d in zip(ws32, bs32, dils))
    ref.backward(gout)
    assert (out - ref).abs().max() <= 0.02 * ref.abs().max()                           # 36 bf16-rounded partial products per output
    assert (f.grad.float() - f32.grad).abs().max() <= 0.02 * f32.grad.abs().max()
    for w, w32, b, b32 in zip(ws, ws32, bs, bs32):
        assert (w.grad - w32.grad).abs().max() <= 0.02 * w32.grad.abs().max()
        assert (b.grad - b32.grad).abs().max() <= 1e-4 * b32.grad.abs().max() + 1e-4


def test_add_relu_and_its_backward(ops):
    """ops.add_relu / ops.relu_mask (the fused tail of a ResNet bottleneck): relu(a + b) with one rounding, and (g (+ g2)) where y > 0"""
    torch.manual_seed(3)
    for shape, cl in [((2, 64, 9, 7), True), ((3, 8, 5, 5), False), ((1, 256, 33, 33), True)]:
        mk = lambda: (torch.randn(*shape, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last) if cl  # noqa: E731
                      else torch.randn(*shape, device="cuda").bfloat16())
        a, b, g, g2 = mk(), mk(), mk(), mk()
        y = ops.add_relu(a, b)
        assert torch.equal(y, torch.relu(a.float() + b.float()).bfloat16()) and y.stride() == a.stride()
        assert torch.equal(ops.relu_mask(g, y), torch.where(y > 0, g, torch.zeros_like(g)))
        want = torch.where(y > 0, (g.float() + g2.float()).bfloat16(), torch.zeros_like(g))
        assert torch.equal(ops.relu_mask(g, y, g2), want)


def test_col2im_is_the_adjoint_of_im2col(ops):
    """<col2im(c), x> == <c, im2col(x)> for random bf16 tensors (f32 dot products), several dilations"""
    torch.manual_seed(5)
    for B, C, H, W, d in [(2, 16, 9, 7, 1), (1, 64, 41, 41, 12), (2, 8, 5, 5, 6), (1, 24, 13, 11, 2)]:
        x = torch.randn(B, H, W, C, device="cuda").bfloat16()
        c = torch.randn(B * H * W, 9 * C, device="cuda").bfloat16()
        lhs = (ops.col2im3x3_nhwc(c, B, H, W, C, d).permute(0, 2, 3, 1).float() * x.float()).sum()
        rhs = (c.float() * ops.im2col3x3_nhwc(x, d).float()).sum()
        assert abs(lhs.item() - rhs.item()) <= 0.01 * max(1.0, abs(rhs.item())) + 0.02 * (c.float().abs().sum() * 2 ** -8).item() ** 0.5


def test_four_host_threads_four_contexts(ops):
    """include/dsrg_hip.h, "threads": different handles may be driven from different host threads at once.  Four threads,
    each with its own context, stream, batch and map size (so that the kernels' shared dynamic-LDS tables are raced for
    different sizes), run the fused step, a CRF and an SRG call six times; every result must equal the single-threaded run
    of the same inputs bit for bit."""
    import threading
    shapes = [(3, 21, 41, 41), (2, 21, 65, 65), (1, 30, 33, 47), (4, 21, 41, 41)]
    cases = []
    for k, (B, C, H, W) in enumerate(shapes):
        b = S.make_batch(700 + k, B, C=C, H=H, W=W, size=8 * (max(H, W) - 1) + 1)
        cases.append({k_: dev(v) for k_, v in b.items()})

    def work(k, out, reps):
        torch.cuda.set_device(0)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            c = cases[k]
            B, C, H, W = c["logits"].shape
            ctx = ops.Context(B, C, H, W)
            res = None
            for _ in range(reps):
                losses, grad, blobs = ops.supervision_step(c["logits"], c["images"], c["labels"], c["cues"], ctx=ctx, want_blobs=True)
                refined, logq = ops.crf_refine(blobs["probs"].clone(), c["images"], ctx=ctx)
                seeds = ops.srg_grow(c["labels"], c["cues"], refined)
                res = [losses.clone(), grad.clone(), blobs["seeds"].clone(), refined.clone(), logq.clone(), seeds.clone()]
            st.synchronize()
            out[k] = [t.cpu() for t in res]

    alone = {}
    for k in range(4):
        work(k, alone, 1)
    together = {}
    threads = [threading.Thread(target=work, args=(k, together, 6)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert sorted(together) == [0, 1, 2, 3]
    for k in range(4):
        for a, b in zip(alone[k], together[k]):
            assert torch.equal(a, b), k


def test_crf_objects_on_their_own_streams(ops, O):
    """dsrg_crf_set_stream: several images in flight (one DenseCRF object and stream each, asynchronous calls) give exactly the
    one-at-a-time results, in order — mixed sizes, both paths (LDS-resident and global-memory), maps and marginals"""
    from dsrg_amd.crf import CRF_device, CRF_device_many
    pairs = []
    for k, (H, W, C) in enumerate([(97, 131, 21), (41, 41, 21), (97, 131, 21), (120, 90, 5), (97, 131, 21), (120, 90, 5), (97, 131, 21)]):
        rng = np.random.default_rng(500 + k)
        img = S.make_images(rng, 1, size=max(H, W))[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
        im = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (1, 2, 0))).astype(np.uint8)).cuda()
        logits = S.make_logits(rng, 1, C, H, W, gain=12.0, sigma=6.0)[0]
        e = np.exp(logits - logits.max(0, keepdims=True))
        un = torch.from_numpy(np.log(np.maximum(e / e.sum(0, keepdims=True), 1e-5)).transpose(1, 2, 0).astype(np.float32).copy()).cuda()
        pairs.append((im, un))
    for want in ("map", "marginals"):
        one = [CRF_device(im, un, scale_factor=1.0, want=want) for im, un in pairs]
        many = list(CRF_device_many(pairs, scale_factor=1.0, want=want, in_flight=3))
        assert len(many) == len(one)
        for a, b in zip(one, many):
            assert torch.equal(a, b)
    q = many[0].cpu().numpy()
    want_q = O.CRF(pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy(), scale_factor=1.0)
    assert np.abs(q - want_q).max() < CRF_TOL


def _fullres_case(seed, H, W, C, kind="smooth"):
    rng = np.random.default_rng(seed)
    img = S.make_images(rng, 1, size=max(H, W), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]
    im = torch.from_numpy(np.ascontiguousarray(np.transpose(img, (1, 2, 0))).astype(np.uint8)).cuda()
    logits = S.make_logits(rng, 1, C, H, W, gain=12.0, sigma=6.0)[0]
    e = np.exp(logits - logits.max(0, keepdims=True))
    un = torch.from_numpy(np.log(np.maximum(e / e.sum(0, keepdims=True), 1e-5)).transpose(1, 2, 0).astype(np.float32).copy()).cuda()
    return im, un


@pytest.mark.parametrize("H,W,C,B", [(97, 123, 21, 4),      # N % 4 = 3: every image brings its own SSE padding pixel and phantom vertices
                                     (100, 120, 21, 3),     # N % 4 = 0
                                     (61, 47, 5, 8),        # the largest batch an object takes; N % 4 = 3
                                     (123, 186, 21, 2)])    # one of the shapes of the round-3 allocation bug
def test_crf_batch_equals_single_image_calls_bit_for_bit(ops, O, H, W, C, B):
    """dsrg_crf_create_batch (round-4 review item 4): B same-sized images through ONE set of launches — lattices built together
    (every key carries its image's number), every splat / blur / slice launch carrying all of them — against B calls of the
    one-image object on the same (global-memory) path: marginals and labels equal bit for bit, image by image; and the batch
    against the oracle.  Cases: a dark-corner image (many pixels in the origin simplex, where the SSE padding's phantom vertices
    sit) next to smooth and noise images."""
    from dsrg_amd.crf import CRF_device_batch, DenseCRF
    kinds = ["smooth", "dark_corner", "noise", "smooth"]
    cases = [_fullres_case(900 + 7 * k + H, H, W, C, kinds[k % 4]) for k in range(B)]
    ims, uns = torch.stack([c[0] for c in cases]), torch.stack([c[1] for c in cases])
    for want in ("marginals", "map"):
        got = CRF_device_batch(ims, uns, scale_factor=1.0, want=want)
        for k in range(B):
            # the one-image object of the same path (a batched object of one image: no image number in any key)
            crf = DenseCRF(W, H, C, nimages=1)
            crf.set_unary_energy((-uns[k]).contiguous())
            crf.add_pairwise_energy(10, 80.0, 80.0, 13, 13, 13, 3, 3.0, 3.0, ims[k].contiguous())
            one = crf.map(10, out=torch.empty((H, W), dtype=torch.int32, device="cuda")) if want == "map" else \
                crf.inference(10, out=torch.empty((H, W, C), dtype=torch.float32, device="cuda"))
            assert torch.equal(got[k], one), (want, k)
    q = got if want == "marginals" else CRF_device_batch(ims, uns, scale_factor=1.0)
    for k in (0, B - 1):
        want_q = O.CRF(ims[k].cpu().numpy(), uns[k].cpu().numpy(), scale_factor=1.0)
        assert np.abs(q[k].cpu().numpy() - want_q).max() < CRF_TOL
    # on a caller's side stream the cached objects are bound to THAT stream for the call (no detour over the null stream), inputs
    # produced on the stream just before are seen, and the objects go back to the cache unbound
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        uns2 = uns * 1.0
        q2 = CRF_device_batch(ims, uns2, scale_factor=1.0)
    side.synchronize()
    assert torch.equal(q2, q)
    assert torch.equal(CRF_device_batch(ims, uns, scale_factor=1.0), q)


def test_crf_batch_through_the_many_images_loop_and_its_limits(ops, O):
    """CRF_device_many(batch=k): consecutive same-sized images share batched calls, results in order and bit-equal to the
    one-at-a-time results (mixed sizes break the runs); a batched object refuses more than eight images, and refuses — at
    inference, loudly — a spatial kernel so narrow that the image number does not fit beside its lattice coordinates"""
    from dsrg_amd.crf import CRF_device, CRF_device_many, CRF_device_batch, DenseCRF
    from dsrg_amd._lib import DsrgError
    shapes = [(97, 131, 21)] * 5 + [(120, 90, 5)] * 2 + [(97, 131, 21)] * 3 + [(41, 41, 21)]
    pairs = [_fullres_case(700 + k, H, W, C) for k, (H, W, C) in enumerate(shapes)]
    one = [CRF_device(im, un, scale_factor=1.0, want="map") for im, un in pairs]
    for batch, in_flight in ((4, 2), (3, 1), (8, 3)):
        many = list(CRF_device_many(pairs, scale_factor=1.0, want="map", in_flight=in_flight, batch=batch))
        assert len(many) == len(one)
        for k, (a, b) in enumerate(zip(one, many)):
            assert torch.equal(a, b), (batch, k)
    with pytest.raises(DsrgError):
        DenseCRF(50, 50, 21, nimages=9)
    # scale_factor 12 at 400 pixels a side: sigma_gamma = 0.25 px, lattice coordinates reach ~2800 > 2040
    im, un = _fullres_case(5, 400, 400, 3)
    with pytest.raises(DsrgError):
        CRF_device_batch(torch.stack([im, im]), torch.stack([un, un]), scale_factor=12.0)
    # ... while the same two images at the test-time scale pass, and the one-image call never has the limit
    assert CRF_device_batch(torch.stack([im, im]), torch.stack([un, un]), scale_factor=1.0).shape == (2, 400, 400, 3)
    assert CRF_device(im, un, scale_factor=12.0).shape == (400, 400, 3)


def test_pylayers_resident_blobs_follow_host_writes():
    """dsrg_amd.layers keeps blobs resident in HBM between the layers of an iteration (cost table): a host blob
    whose bytes are unchanged is not uploaded again; any write between iterations is seen (full digest at the first sight of an
    epoch), a write at a sampled position also inside an iteration; the registries stay bounded; a non-contiguous input is
    never cached under its temporary's address"""
    from dsrg_amd import layers as L
    if L._digest is None or L._TRUST:
        pytest.skip("xxhash absent or DSRG_PYLAYERS_TRUST set")
    rng = np.random.default_rng(0)
    a = rng.random((16, 21, 41, 41), dtype=np.float32)
    with L._call("t", new_epoch="softmax"):
        t0 = L._dev(a)
        assert L._dev(a) is t0                                   # same bytes, same epoch: the resident copy (every byte compared)
    with L._call("t", new_epoch="softmax"):
        assert L._dev(a) is t0                                   # next iteration, unchanged: full digest, still resident
        a[7, 3, 20, 20] += 1.0                                   # a sparse write to a HOST-PROVIDED blob inside the iteration, at
        t1 = L._dev(a)                                           # a position the sampled digest does not cover: seen at once
        assert t1 is not t0 and torch.equal(t1.cpu(), torch.from_numpy(a))
    with L._call("t", new_epoch="softmax"):
        assert L._dev(a) is t1
        a[0, 0, 0, 0] += 1.0
        t2 = L._dev(a)
        assert t2 is not t1 and float(t2[0, 0, 0, 0]) == float(a[0, 0, 0, 0])
    # a blob we wrote mirrors the tensor it was written from: inside the iteration the sampled digest vouches for it ...
    host = np.zeros_like(a)
    with L._call("t", new_epoch="softmax"):
        L._publish(host, t2)
    assert np.array_equal(host, a)
    with L._call("t"):
        assert L._dev(host).data_ptr() == t2.data_ptr()          # (no upload: the tensor the blob was written from)
    # ... and a layer whose forward runs a second time without the head of the path in between (a stand-alone driver: numeric
    # gradient checks on a loss layer) begins a new iteration: every byte of a blob we wrote is compared again
    e0 = L._epoch[0]
    with L._call("X.forward"):
        assert L._dev(host).data_ptr() == t2.data_ptr() and L._epoch[0] == e0
    host[7, 3, 20, 21] += 1.0                                    # not a sampled position
    with L._call("X.forward"):
        assert L._epoch[0] == e0 + 1
        t3 = L._dev(host)
        assert t3.data_ptr() != t2.data_ptr() and torch.equal(t3.cpu(), torch.from_numpy(host))
    # non-contiguous input: uploaded from a temporary, never cached
    n0 = len(L._resident)
    with L._call("t"):
        v = L._dev(a[:, ::2])
    assert v.shape == (16, 11, 41, 41) and len(L._resident) == n0
    # bounded registries
    with L._call("t", new_epoch="softmax"):
        keep = [rng.random((1, 21, 41, 41), dtype=np.float32) for _ in range(L._MAX_RESIDENT + 8)]
        for x in keep:
            L._dev(x); L._dev(x)
    assert len(L._resident) <= L._MAX_RESIDENT and len(L._pinned) <= L._MAX_RESIDENT
