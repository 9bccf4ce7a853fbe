"""dsrg_msc_loss_batch / dsrg_msc_pyramid_batch (dsrg_amd/csrc/msc.hip), ops.msc_loss / ops.msc_pyramid / ops.MscLossFn and
retrain.seg_softmax_loss_msc: the multi-scale-input step's pyramid and its S + 1 softmax losses with max fusion.

CPU: the entry points' argument checks (refused calls only: every call returns before any device call), the workspace size over
the case list, the --msc-scales option of `python -m dsrg_amd.train`, msc_sizes, the label sampling, and the NumPy restatement of
the contract (tests/msc_cases.py) against the float64 torch reference.
GPU: counters and valid counts as integers; losses and gradients against the float64 reference (gradient of map s: max|grad_s - g64_s|
<= max(4 e32_s, 16 * 2^-24) max|g64_s| with e32_s the float32 torch composition's own relative error on the same input, loss: 2
float32 ulps); exact data bit for bit; one class; nothing valid; determinism, overwriting, accumulation of the counters, the stream;
autograd; the pyramid bit for bit.

Measured on an MI355X (the figures the tests print before they assert): see the docstrings of the two tolerance tests."""
import ctypes

import numpy as np
import pytest
import torch

import msc_cases as M

_FAKE = 256                                                           # a "device pointer" that is never dereferenced: refused calls only
IDS = [M.case_id(c) for c in M.CASES]
WORKLOADS = [(10, 21, ((41, 41), (31, 31), (21, 21)), 321, 321), (10, 21, ((65, 65), (49, 49), (33, 33)), 513, 513)]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _fakes(n, value=_FAKE):
    return (ctypes.c_void_p * n)(*([value] * n))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_msc_loss_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    ok = dict(S=3, B=2, C=21, h=(9, 7, 5), w=(9, 7, 5), H=65, W=65)
    ptrs = ("maps", "labels", "losses", "grads", "counters", "workspace")
    big = 1 << 40                                                     # (a workspace size no shape below needs)

    def call(nbytes, **kw):
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        p = {name: kw.get(name, _FAKE) for name in ptrs}
        for name in ("maps", "grads"):
            if p[name] == _FAKE:
                p[name] = _fakes(4)
        h = _ints(a["h"]) if a["h"] is not None else None
        w = _ints(a["w"]) if a["w"] is not None else None
        return L.dsrg_msc_loss_batch(a["S"], a["B"], a["C"], p["maps"], h, w, p["labels"], a["H"], a["W"], 255.0, p["losses"],
                                     p["grads"], p["counters"], p["workspace"], nbytes, None)

    E, U = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    for name in ptrs:
        assert call(big, **{name: None}) == E and b"NULL" in L.dsrg_last_error(), name
    assert call(big, h=None) == E and call(big, w=None) == E
    assert call(big, maps=_fakes(4, None)) == E and b"NULL" in L.dsrg_last_error()
    assert call(big, grads=(ctypes.c_void_p * 4)(_FAKE, _FAKE, None, _FAKE)) == E and b"NULL" in L.dsrg_last_error()
    assert call(big, S=1) == E and b"score maps" in L.dsrg_last_error()
    assert call(big, S=5, h=(9,) * 5, w=(9,) * 5) == E and b"score maps" in L.dsrg_last_error()
    assert call(big, B=0) == E and b"images" in L.dsrg_last_error()
    assert call(big, B=33) == E and b"32" in L.dsrg_last_error()
    assert call(big, C=0) == E and b"labels" in L.dsrg_last_error()
    assert call(big, C=97) == U and b"96" in L.dsrg_last_error()
    for name in ("H", "W"):
        assert call(big, **{name: 0}) == E and call(big, **{name: -3}) == E, name
    for name in ("h", "w"):
        assert call(big, **{name: (9, 0, 5)}) == E and call(big, **{name: (9, 7, -1)}) == E, name
    assert call(big, B=32, C=64, h=(9, 1024, 5), w=(9, 1024, 5)) == E and b"2^31" in L.dsrg_last_error()     # B*C*h*w = 2^31
    assert call(big, B=32, C=96, h=((1 << 31) - 1,) * 3, w=((1 << 31) - 1,) * 3) == E                        # (no wrap-around in the check)
    assert call(big, B=32, C=32, h=(1024,) * 3, w=(1023,) * 3) == E and b"2^31" in L.dsrg_last_error()       # only the sum reaches 2^31
    assert call(big, B=32, H=8192, W=8192) == E and b"2^31" in L.dsrg_last_error()                           # B*H*W = 2^31
    assert call(big, B=1, H=(1 << 31) - 1, W=(1 << 31) - 1) == E
    need = L.dsrg_msc_loss_workspace(3, 2, 21, _ints(ok["h"]), _ints(ok["w"]), 65, 65)
    assert need > 0
    assert call(need - 1) == E and b"workspace" in L.dsrg_last_error()                                       # one byte short
    assert call(0) == E
    assert call(big, workspace=_FAKE + 4) == E and b"aligned" in L.dsrg_last_error()
    # the size function answers 0 for what the launch refuses
    for bad in (dict(S=1), dict(S=5, h=(9,) * 5, w=(9,) * 5), dict(B=0), dict(B=33), dict(C=0), dict(C=97), dict(h=(9, 0, 5)), dict(W=0),
                dict(B=32, C=64, h=(9, 1024, 5), w=(9, 1024, 5)), dict(B=32, C=32, h=(1024,) * 3, w=(1023,) * 3)):
        a = dict(ok, **bad)
        assert L.dsrg_msc_loss_workspace(a["S"], a["B"], a["C"], _ints(a["h"]), _ints(a["w"]), a["H"], a["W"]) == 0, bad
    assert L.dsrg_msc_loss_workspace(3, 2, 21, None, _ints(ok["w"]), 65, 65) == 0


def test_msc_pyramid_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    E = _lib.ERR_INVALID

    def call(B=2, images=_FAKE, H=65, W=65, n=2, h=(49, 33), w=(49, 33), out="fake"):
        out = _fakes(3) if out == "fake" else out
        return L.dsrg_msc_pyramid_batch(B, images, H, W, n, _ints(h) if h is not None else None, _ints(w) if w is not None else None, out,
                                        None)

    assert call(images=None) == E and b"NULL" in L.dsrg_last_error()
    assert call(h=None) == E and call(w=None) == E and call(out=None) == E
    assert call(out=(ctypes.c_void_p * 3)(_FAKE, None, _FAKE)) == E and b"NULL" in L.dsrg_last_error()
    assert call(n=0) == E and call(n=4, h=(9,) * 4, w=(9,) * 4) == E and b"copies" in L.dsrg_last_error()
    assert call(B=0) == E and call(B=33) == E and b"32" in L.dsrg_last_error()
    assert call(H=0) == E and call(W=-1) == E
    assert call(h=(49, 0)) == E and call(w=(-2, 33)) == E
    assert call(B=32, H=8192, W=8192) == E and b"2^31" in L.dsrg_last_error()
    assert call(B=32, H=1 << 30, W=1 << 30) == E and call(B=32, H=(1 << 31) - 1, W=(1 << 31) - 1) == E     # (no wrap-around in the check)
    assert call(B=32, h=(8192, 33), w=(8192, 33)) == E and b"2^31" in L.dsrg_last_error()
    assert call(h=((1 << 31) - 1, 33), w=((1 << 31) - 1, 33)) == E                                           # (no wrap-around in the check)


def test_workspace_size_is_positive_for_every_case():
    from dsrg_amd import _lib
    L = _lib.lib()
    for B, C, maps, H, W in M.CASES + M.EXACT_CASES + WORKLOADS + [(32, 96, ((65, 65), (49, 49), (33, 33), (17, 17)), 513, 513)]:
        n = L.dsrg_msc_loss_workspace(len(maps), B, C, _ints([h for h, _ in maps]), _ints([w for _, w in maps]), H, W)
        n0 = B * C * maps[0][0] * maps[0][1]
        assert 5 * n0 < n < 5 * n0 + (1 << 20), (B, C, maps)             # O(B C h_0 w_0) floats plus the slots


def test_ops_check_their_tensors_before_the_library_is_called():
    from dsrg_amd import ops
    with pytest.raises(ValueError, match="CUDA"):
        ops.msc_loss([torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2, 2)], torch.zeros(2, 1, 9, 9))
    with pytest.raises(ValueError, match="score maps"):
        ops.msc_loss([torch.zeros(2, 3, 4, 4)], torch.zeros(2, 1, 9, 9))
    with pytest.raises(ValueError, match="CUDA"):
        ops.msc_pyramid(torch.zeros(2, 3, 9, 9), [5])


def test_msc_scales_option():
    from dsrg_amd.train import parse_args
    f = ["--stage", "f", "--list", "l", "--root", "r"]
    assert parse_args(f).msc_scales == ()
    assert parse_args(f + ["--msc-scales", "0.75,0.5"]).msc_scales == (0.75, 0.5)
    assert parse_args(f + ["--msc-scales", "0.75,0.5", "--loss-at", "map"]).msc_scales == (0.75, 0.5)
    assert parse_args(f + ["--msc-scales", "2", "--backbone", "resnet101", "--crop", "65"]).msc_scales == (2.0,)
    s = ["--stage", "s", "--list", "l", "--root", "r", "--cues", "c"]
    assert parse_args(s).msc_scales is None
    for bad in (s + ["--msc-scales", "0.75,0.5"],                             # stage s
                f + ["--msc-scales", "0.75,0.5", "--loss-at", "label"],       # out of scope together
                f + ["--msc-scales", "0.75,x"], f + ["--msc-scales", ""], f + ["--msc-scales", "0"], f + ["--msc-scales", "-0.5"],
                f + ["--msc-scales", "2.5"], f + ["--msc-scales", "nan"], f + ["--msc-scales", "0.75,1"], f + ["--msc-scales", "0.5,0.5"], f + ["--msc-scales", "0.9,0.8,0.7,0.6"],
                f + ["--msc-scales", "0.04"],                                 # 321 -> 14 < 17
                f + ["--msc-scales", "0.2", "--crop", "65"]):                 # 65 -> 14
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_trainer_refuses_bad_msc_scales():
    from dsrg_amd.retrain import RetrainTrainer
    cpu = torch.device("cpu")
    for bad in ((0.0,), (-1.0,), (2.5,), (float("nan"),), (0.9, 0.8, 0.7, 0.6), ("x",), 0.5, (1.0,), (0.75, 0.5, 0.75)):
        with pytest.raises(ValueError, match="msc_scales"):
            RetrainTrainer(cpu, msc_scales=bad)
    with pytest.raises(ValueError, match="msc_scales"):
        RetrainTrainer(cpu, msc_scales=(0.75,), loss_at="label")


def test_msc_sizes_and_label_sampling():
    from dsrg_amd.retrain import msc_sizes
    assert msc_sizes(321, (0.75, 0.5)) == (241, 161)
    assert msc_sizes(513, (0.75, 0.5)) == (385, 257)
    assert msc_sizes(65, (0.75, 0.5)) == (49, 33) and msc_sizes(321, ()) == ()
    for H, h in ((321, 41), (513, 65), (65, 9)):
        assert np.array_equal(M.label_index(h, H), np.arange(H)[::8])
    assert np.array_equal(M.label_index(1, 9), [0]) and np.array_equal(M.label_index(3, 3), [0, 1, 2])
    assert np.array_equal(M.label_index(2, 10), [0, 9]) and np.array_equal(M.label_index(3, 4), [0, 2, 3])   # 1.5 rounds up
    lab = np.arange(2 * 321 * 321, dtype=np.float32).reshape(2, 1, 321, 321)
    assert np.array_equal(M.sample_labels(lab, 41, 41), lab[:, 0, ::8, ::8])


def test_restatement_by_hand():
    # map 0: 1 x 2, map 1: 1 x 1, two classes, one label pixel per cell.  u_1 is the constant z_1.
    z0 = np.array([[[[2.0, 0.0]], [[0.0, 0.0]]]], dtype=np.float32)             # (1, 2, 1, 2)
    z1 = np.array([[[[1.0]], [[0.0]]]], dtype=np.float32)                       # class 0: scale 1 wins at x = 1 only; class 1: ties -> 0
    lab = np.array([[[[0.0, 1.0]]]], dtype=np.float32)
    losses, grads, cnt, N = M.msc_loss([z0, z1], lab)
    assert N == [2, 1] and cnt[0] == 2 and cnt[2] == 0
    f = np.array([[2.0, 1.0], [0.0, 0.0]])                                      # fused (class, x)
    p = np.exp(f) / np.exp(f).sum(0)
    assert abs(float(losses[0]) - float(-(np.log(p[0, 0]) + np.log(p[1, 1])) / 2)) < 1e-6
    # map 1's gradient: its own head (label: the nearest sample of a one-cell axis is x = 0, class 0) + the fused head's share,
    # which is class 0 at x = 1 only (the gather's weights of a one-cell axis are l0 + l1 = 1)
    p1 = np.exp([1.0, 0.0]) / np.exp([1.0, 0.0]).sum()
    want = np.array([p1[0] - 1.0 + p[0, 1] / 2, p1[1]])
    assert np.abs(grads[1].reshape(2) - want).max() < 1e-6
    # nothing valid: no NaN
    l0, g0, c0, n0 = M.msc_loss([z0, z1], np.full_like(lab, 255))
    assert not l0.any() and not any(g.any() for g in g0) and c0 == [0, 0, 0] and n0 == [0, 0]


@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_restatement_against_the_float64_reference(case):
    maps, labels, _ = M.make_case(case)
    assert M.fused_gap(maps) >= M.MIN_GAP and max(float(np.abs(m).max()) for m in maps) < 16.0
    losses, grads, cnt, N = M.msc_loss(maps, labels)
    l64, g64, e32 = M.reference(case)
    C = case[1]
    for s, m in enumerate(maps):
        valid, invalid = M.SL.classify(M.sample_labels(labels, *m.shape[-2:]), C)
        assert N[s] == int(valid.sum())
        if s == 0:
            assert cnt[0] == N[0] and cnt[2] == int(invalid.sum()) and 0 <= cnt[1] <= cnt[0]
    for g, r, bound in zip(grads, g64, M.grad_bounds(case)):
        assert np.abs(g.astype(np.float64) - r).max() <= bound
    for a, b in zip(losses, l64):
        assert abs(float(a) - b) <= 2 * float(np.spacing(np.float32(b)))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _d(a):
    return torch.from_numpy(np.array(a)).cuda()


def _run(maps, labels, **kw):
    from dsrg_amd import ops
    losses, grads, cnt = ops.msc_loss([_d(m) for m in maps], _d(labels), **kw)
    return losses.cpu().numpy(), [g.cpu().numpy() for g in grads], cnt.cpu().numpy().tolist()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw(maps, labels, counters=(0, 0, 0), fill=float("nan")):
    """the C entry point on buffers of the test's own (full of `fill`) -> (losses, grads, counters, the workspace's valid counts)"""
    from dsrg_amd import _lib, ops
    L = _lib.lib()
    dm, dl = [_d(m) for m in maps], _d(labels)
    B, C = maps[0].shape[:2]
    H, W = labels.shape[-2:]
    hs, ws = _ints([m.shape[2] for m in maps]), _ints([m.shape[3] for m in maps])
    grads = [torch.full(m.shape, fill, device="cuda") for m in maps]
    losses = torch.full((len(maps) + 1,), fill, device="cuda")
    cnt = torch.tensor(list(counters), dtype=torch.int64, device="cuda")
    buf = torch.full((L.dsrg_msc_loss_workspace(len(maps), B, C, hs, ws, H, W),), 0xA5, dtype=torch.uint8, device="cuda")
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    _lib.check(L.dsrg_msc_loss_batch(len(maps), B, C, ptrs(dm), hs, ws, dl.data_ptr(), H, W, 255.0, losses.data_ptr(), ptrs(grads),
                                     cnt.data_ptr(), buf.data_ptr(), buf.numel(), ops._stream()))
    return losses, grads, cnt, buf[:8 * len(maps)].view(torch.int64).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_counters_and_valid_counts_are_exact(case):
    maps, labels, _ = M.make_case(case)
    _, _, want_cnt, want_n = M.msc_loss(maps, labels)
    _, _, cnt, n = _raw(maps, labels)
    assert cnt.tolist() == want_cnt and n == want_n
    assert _run(maps, labels)[2] == want_cnt


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_gradients_against_the_float64_reference(case):
    """per map: max|grad_s - g64_s| <= max(4 e32_s, 16 * 2^-24) max|g64_s|.  On an MI355X the kernel's error relative to max|g64_s| is
    at most 2.6e-7 over the cases (2x81-9x9_7x7_5x5_3x3-65x65, map 0; 2.5e-7, 1.6e-7 and 1.9e-7 for the three maps of
    2x21-41x41_31x31_21x21-321x321; 2.0e-7 at the identity zoom 2x21-5x7_5x7_5x7-33x49, map 2); the float32 torch composition's on
    the CPU: 4.7e-8 to 3.3e-7; the floor of the bound: 9.5e-7."""
    maps, labels, _ = M.make_case(case)
    _, grads, _ = _run(maps, labels)
    _, g64, e32 = M.reference(case)
    bounds = M.grad_bounds(case)
    errs = []
    for s, (g, r) in enumerate(zip(grads, g64)):
        err, top = float(np.abs(g.astype(np.float64) - r).max()), float(np.abs(r).max())
        errs.append(err)
        print("msc grad %s map %d: max|grad - g64| = %.3e, max|g64| = %.3e, relative %.3e, e32 %.3e, bound %.3e"
              % (M.case_id(case), s, err, top, err / top if top else 0.0, e32[s], bounds[s]))
    assert all(np.isfinite(g).all() for g in grads)
    assert all(e <= b for e, b in zip(errs, bounds))


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_losses_against_the_float64_reference(case):
    """every head: |loss - l64| <= 2 float32 ulps of l64.  On an MI355X: at most 0.593 ulp over the cases and heads (map 0 of
    2x3-3x4_2x3_1x2-17x25; 0.525 at 2x21-19x18_14x13_9x9-145x137, map 2; 0.363 at 2x21-41x41_31x31_21x21-321x321)."""
    maps, labels, _ = M.make_case(case)
    losses, _, _ = _run(maps, labels)
    l64 = M.reference(case)[0]
    ulps = [float(np.spacing(np.float32(b))) for b in l64]
    print("msc loss %s: %s ulp" % (M.case_id(case), ", ".join("%.3f" % (abs(float(a) - b) / u) for a, b, u in zip(losses, l64, ulps))))
    assert all(abs(float(a) - b) <= 2 * u for a, b, u in zip(losses, l64, ulps))


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.EXACT_CASES, ids=[M.case_id(c) for c in M.EXACT_CASES])
def test_exact_data_bit_for_bit(case):
    maps, labels = M.make_exact_case(case)
    want_losses, want, want_cnt, want_n = M.msc_loss(maps, labels)
    assert want_cnt[0] == maps[0][:, 0].size and want_cnt[2] == 0 and all(g.any() for g in want)    # all labels are valid
    import eval_confusion_cases as K
    u = np.stack([maps[0][0]] + [K.zoom(m[0], *maps[0].shape[-2:]) for m in maps[1:]])
    assert ((u == u.max(0)).sum(0) > 1).sum() >= 4                              # scales tie (6 - 8 % of the cells): the lowest-s rule decides there
    losses, grads, cnt = _run(maps, labels)
    assert cnt == want_cnt
    for g, w in zip(grads, want):
        assert np.array_equal(_bits(g), _bits(w))
    ln2 = np.float32(np.log(2.0))
    assert all(abs(float(l) - float(ln2)) <= 2 * float(np.spacing(ln2)) for l in losses)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [((3, 4), (2, 3), (1, 2)), ((5, 6), (7, 9))], ids=("shrinking", "a-larger-map"))
def test_one_label_gives_zero_exactly(sizes):
    rng = np.random.default_rng(4)
    maps = [rng.standard_normal((2, 1, h, w)).astype(np.float32) for h, w in sizes]
    labels = np.zeros((2, 1, 17, 25), dtype=np.float32)
    losses, grads, cnt = _run(maps, labels)
    assert cnt == [2 * sizes[0][0] * sizes[0][1]] * 2 + [0]
    assert not _bits(losses).any() and not any(_bits(g).any() for g in grads)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [M.CASES[2], M.CASES[4]], ids=[IDS[2], IDS[4]])
def test_nothing_valid(case):
    maps, labels, _ = M.make_case(case)
    n0 = maps[0].shape[0] * maps[0].shape[2] * maps[0].shape[3]
    for value, want in ((255.0, [0, 0, 0]), (200.0, [0, 0, n0])):
        losses, grads, cnt = _run(maps, np.full_like(labels, value))
        assert cnt == want
        assert not _bits(losses).any() and not any(_bits(g).any() for g in grads)
    # image 1 of make_labels is ignored as a whole: its gradient slices are zero, the others' are not
    _, grads, _ = _run(maps, labels)
    assert (labels[1] == 255).all() and all(not _bits(g[1]).any() and g[0].any() for g in grads)


@pytest.mark.gpu
def test_determinism_overwriting_and_accumulation():
    from dsrg_amd import ops
    for case in (M.CASES[4], M.CASES[5], M.CASES[7]):                           # empty footprints; several workgroups; S = 4
        maps, labels, _ = M.make_case(case)
        dm, dl = [_d(m) for m in maps], _d(labels)
        first = ops.msc_loss(dm, dl)
        for _ in range(2):
            again = ops.msc_loss(dm, dl)
            assert torch.equal(again[0].view(torch.int32), first[0].view(torch.int32)) and torch.equal(again[2], first[2])
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again[1], first[1]))
        # results are written, not added to: through the C entry point, into buffers full of NaN; the counters are added to
        losses, grads, cnt, _ = _raw(maps, labels, counters=(5, 6, 7))
        assert torch.equal(losses.view(torch.int32), first[0].view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, first[1]))
        assert cnt.tolist() == [a + b for a, b in zip([5, 6, 7], first[2].tolist())]
        both = ops.msc_loss(dm, dl, counters=first[2].clone())[2]
        assert both.tolist() == [2 * v for v in first[2].tolist()]
        for m, d in zip(maps, dm):
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(m))              # the inputs are left as they were
    assert torch.cuda.current_stream() == torch.cuda.default_stream()


@pytest.mark.gpu
def test_autograd():
    from dsrg_amd import ops
    from dsrg_amd.retrain import seg_softmax_loss_msc
    maps, labels, _ = M.make_case(M.CASES[2])
    want_losses, want, want_cnt = ops.msc_loss([_d(m) for m in maps], _d(labels))
    xs = [_d(m).requires_grad_(True) for m in maps]
    total, losses = seg_softmax_loss_msc(xs, _d(labels))
    assert total.dim() == 0 and not losses.requires_grad and torch.equal(losses.view(torch.int32), want_losses.view(torch.int32))
    assert torch.equal(total.detach().view(torch.int32), want_losses.sum().view(torch.int32))
    total.backward()
    for x, w in zip(xs, want):
        assert x.grad.is_contiguous() and x.grad.dtype == torch.float32 and torch.equal(x.grad.view(torch.int32), w.view(torch.int32))
    for g in (2.0, 0.37):                                                       # leaf gradients are the op's grad_s * g, bit for bit
        xs2 = [_d(m).requires_grad_(True) for m in maps]
        (g * seg_softmax_loss_msc(xs2, _d(labels))[0]).backward()
        for x, w in zip(xs2, want):
            assert torch.equal(x.grad.view(torch.int32), (w * torch.tensor(g, device="cuda")).view(torch.int32))
    # a (B, H, W) label map, and the counters handed through
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    xs3 = [_d(m).requires_grad_(True) for m in maps]
    seg_softmax_loss_msc(xs3, _d(labels)[:, 0], counters=cnt)[0].backward()
    assert all(torch.equal(x.grad.view(torch.int32), w.view(torch.int32)) for x, w in zip(xs3, want)) and cnt.tolist() == want_cnt.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,sizes", [((2, 3, 65, 65), ((49, 49), (33, 33))), ((2, 3, 321, 321), ((241, 241), (161, 161))),
                                         ((1, 3, 17, 23), ((9, 31), (17, 23), (1, 1)))], ids=("65", "321", "odd"))
def test_pyramid_bit_for_bit(shape, sizes):
    from dsrg_amd import ops
    rng = np.random.default_rng(sum(shape))
    images = (rng.random(shape) * 255 - 115).astype(np.float32)
    dx = _d(images)
    outs = ops.msc_pyramid(dx, sizes)
    assert len(outs) == len(sizes)
    for out, want, (h, w) in zip(outs, M.pyramid(images, sizes), sizes):
        assert tuple(out.shape) == (shape[0], 3, h, w) and out.dtype == torch.float32
        assert out.is_contiguous(memory_format=torch.channels_last) and out.stride() == (3 * h * w, 1, 3 * w, 3)
        assert out.contiguous(memory_format=torch.channels_last).data_ptr() == out.data_ptr()            # the step's call is a no-op
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(dx.cpu().numpy()), _bits(images))
    assert [tuple(o.shape[-2:]) for o in ops.msc_pyramid(dx, [5])] == [(5, 5)]                            # a single side
