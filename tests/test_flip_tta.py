"""Mirrored (horizontal-flip) test-time augmentation of the multi-scale tests: every scale runs on the image and on its mirror
image, the mirror's scores are mirrored back, all 2K maps are summed before the softmax.

CPU: the argument checks of dsrg_multiscale_unary_mirror / dsrg_multiscale_unary_mirror_batch / dsrg_preprocess_rect_mirror_batch,
the limits of flip=True in inference.py, the --flip switch of `python -m dsrg_amd.predict`, and a numpy float64 restatement of the
mirrored zoom-and-sum pinned to inference._zoom of torch.flip-ped maps.
GPU: the mirror kernels against the existing kernels on explicitly flipped maps and against the restatement (bit for bit), the
batch forms against the single-image form, flip=True end to end against the staged composition (exact) and against the per-image
path (the project's agreement bar), and the batch-2 graph of VGG16-ASPP."""
import ctypes

import numpy as np
import pytest
import torch

_I32 = ctypes.c_int32
_FAKE = 256                                                           # a "device pointer" that is never dereferenced


def _vp(values):
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def _i32(values):
    return (_I32 * max(len(values), 1))(*values)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _axis(n_in, n_out):
    """multiscale.hip's header, one axis: scale = (in - 1) / (out - 1) (0 when out == 1), src = scale * dst, i0 = (int)src,
    i1 = i0 + (i0 < in - 1), l1 = src - i0 -> (i0, i1, l1), all in float64"""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0             # one correctly rounded IEEE division, as on the device
    src = scale * np.arange(n_out, dtype=np.float64)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0


def mirror_sum_reference(maps, flags, H, W):
    """The `sum` output of dsrg_multiscale_unary_mirror in numpy: per map v = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 +
    l1w * v11) in float64 (numpy contracts nothing), rounded once to float32, the maps added in list order in float32.  x0, x1 and
    the weights come from the output pixel; a map whose flag is set is loaded from the columns w - 1 - x0 and w - 1 - x1.
    maps: (C, h_k, w_k) float32 arrays -> (H, W, C) float32"""
    S = None
    for m, flag in zip(maps, flags):
        C, h, w = m.shape
        y0, y1, l1h = _axis(h, H)
        x0, x1, l1w = _axis(w, W)
        xa, xb = (w - 1 - x0, w - 1 - x1) if flag else (x0, x1)
        v = m.astype(np.float64)
        v00, v01 = v[:, y0][:, :, xa], v[:, y0][:, :, xb]
        v10, v11 = v[:, y1][:, :, xa], v[:, y1][:, :, xb]
        l0h, l0w = 1.0 - l1h, 1.0 - l1w
        z = (l0h[:, None] * (l0w * v00 + l1w * v01) + l1h[:, None] * (l0w * v10 + l1w * v11)).astype(np.float32)
        S = z if S is None else S + z
        assert S.dtype == np.float32
    return np.ascontiguousarray(S.transpose(1, 2, 0))


# the shape list of the kernel tests: map sizes (a single row, a single column, one pixel among them), output sizes ((1, 70) and
# (70, 1) cross a 64-pixel block, (3, 5) is less than one block)
_MAPS = [(5, 7), (9, 4), (1, 1), (1, 6), (6, 1)]
_OUTS = [(13, 11), (1, 70), (70, 1), (3, 5), (1, 1)]
_LABELS = [1, 21, 96]


def _flags(K, case):
    """K flags: mixed where K allows it, all set / the two alternations among the cases"""
    if K == 1:
        return [case % 2]
    pats = [[(k + case) % 2 for k in range(K)], [1] * (K - 1) + [0], [0] + [1] * (K - 1), [((case >> k) & 1) for k in range(K)], [1] * K]
    return pats[case % len(pats)]


def _kernel_cases(C):
    """(K, flags, map sizes, (H, W), seed) for every K in 1..8 and every output size"""
    case = 0
    for K in range(1, 9):
        for H, W in _OUTS:
            case += 1
            yield K, _flags(K, case), [_MAPS[(case + k) % len(_MAPS)] for k in range(K)], (H, W), 1000 * C + case


def _host_maps(seed, C, sizes):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((C, h, w)) * 3.0).astype(np.float32) for h, w in sizes]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_multiscale_unary_mirror_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()

    def call(K=3, C=21, scores="fake", mirror="fake", hs="fake", ws="fake", H=8, W=9, unary=_FAKE, amax=None, sums=None):
        k = max(K, 1)
        P = _vp([_FAKE] * k) if scores == "fake" else scores
        m = _i32([0, 1, 0, 1, 0, 1, 0, 1][:k]) if mirror == "fake" else mirror
        h = _i32([4] * k) if hs == "fake" else hs
        w = _i32([5] * k) if ws == "fake" else ws
        return L.dsrg_multiscale_unary_mirror(K, C, P, m, h, w, H, W, 1e-5, unary, amax, sums, None)

    assert call(K=0) == _lib.ERR_INVALID and b"scales" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID and b"8" in L.dsrg_last_error()
    assert call(C=0) == _lib.ERR_INVALID
    assert call(C=97) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(H=0) == _lib.ERR_INVALID and call(W=0) == _lib.ERR_INVALID
    assert call(scores=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(scores=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(hs=None) == _lib.ERR_INVALID and call(ws=None) == _lib.ERR_INVALID
    assert call(mirror=None) == _lib.ERR_INVALID and b"mirror" in L.dsrg_last_error()
    assert call(hs=_i32([4, 0, 4])) == _lib.ERR_INVALID and call(ws=_i32([5, 5, 0])) == _lib.ERR_INVALID
    assert call(unary=None) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(unary=258) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(unary=None, sums=264) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(C=96, H=16384, W=16384) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_multiscale_unary_mirror_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()

    def call(G=3, K=2, C=21, scores="fake", hs="fake", ws="fake", Hs="fake", Ws="fake", unary="fake", amax=None, sums=None):
        g, k = max(G, 1), max(K, 1)
        P = _vp([_FAKE] * k) if scores == "fake" else scores
        h = _i32([4] * k) if hs == "fake" else hs
        w = _i32([5] * k) if ws == "fake" else ws
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        u = _vp([_FAKE] * g) if unary == "fake" else unary
        return L.dsrg_multiscale_unary_mirror_batch(G, K, C, P, h, w, H, W, 1e-5, u, amax, sums, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=9) == _lib.ERR_INVALID and b"8" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"scales" in L.dsrg_last_error()
    assert call(K=5) == _lib.ERR_INVALID and b"4" in L.dsrg_last_error()
    assert call(C=97) == _lib.ERR_INVALID and b"96" in L.dsrg_last_error()
    assert call(C=0) == _lib.ERR_INVALID
    assert call(scores=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(scores=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(hs=None) == _lib.ERR_INVALID and call(ws=None) == _lib.ERR_INVALID
    assert call(Hs=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Ws=None) == _lib.ERR_INVALID
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and call(Ws=_i32([9, 9, 0])) == _lib.ERR_INVALID
    assert call(hs=_i32([4, 0])) == _lib.ERR_INVALID
    assert call(unary=None) == _lib.ERR_INVALID and b"output" in L.dsrg_last_error()
    assert call(unary=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(amax=_vp([None, _FAKE, _FAKE])) == _lib.ERR_INVALID and b"every image" in L.dsrg_last_error()
    assert call(sums=_vp([_FAKE, _FAKE, None])) == _lib.ERR_INVALID
    assert call(unary=_vp([_FAKE, _FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(unary=None, sums=_vp([_FAKE, 264, _FAKE])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, C=96, Hs=_i32([16384]), Ws=_i32([16384])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_preprocess_rect_mirror_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()
    mean3 = (ctypes.c_float * 3)(104.0, 117.0, 123.0)

    def call(G=3, cap=None, K=2, images="fake", Hs="fake", Ws="fake", oh="fake", ow="fake", mean=mean3, out="fake"):
        g, k = max(G, 1), max(K, 1)
        P = _vp([_FAKE] * g) if images == "fake" else images
        H = _i32([8] * g) if Hs == "fake" else Hs
        W = _i32([9] * g) if Ws == "fake" else Ws
        h = _i32([5] * k) if oh == "fake" else oh
        w = _i32([7] * k) if ow == "fake" else ow
        O = _vp([_FAKE] * k) if out == "fake" else out
        return L.dsrg_preprocess_rect_mirror_batch(G, 2 * G if cap is None else cap, K, P, H, W, h, w, mean, O, None)

    assert call(G=0) == _lib.ERR_INVALID and b"images" in L.dsrg_last_error()
    assert call(G=9) == _lib.ERR_INVALID and b"8" in L.dsrg_last_error()
    assert call(K=0) == _lib.ERR_INVALID and b"sizes" in L.dsrg_last_error()
    assert call(K=9) == _lib.ERR_INVALID
    assert call(cap=5) == _lib.ERR_INVALID and b"capacity" in L.dsrg_last_error()          # 2 G = 6 slots
    assert call(cap=3) == _lib.ERR_INVALID and b"capacity" in L.dsrg_last_error()          # (enough for the plain form)
    assert call(images=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(images=_vp([_FAKE, None, _FAKE])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=None) == _lib.ERR_INVALID and call(Ws=None) == _lib.ERR_INVALID
    assert call(oh=None) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(ow=None) == _lib.ERR_INVALID
    assert call(mean=None) == _lib.ERR_INVALID
    assert call(out=None) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, None])) == _lib.ERR_INVALID and b"NULL" in L.dsrg_last_error()
    assert call(Hs=_i32([8, 0, 8])) == _lib.ERR_INVALID and call(Ws=_i32([0, 9, 9])) == _lib.ERR_INVALID
    assert call(oh=_i32([5, 0])) == _lib.ERR_INVALID and call(ow=_i32([0, 7])) == _lib.ERR_INVALID
    assert call(out=_vp([_FAKE, 258])) == _lib.ERR_INVALID and b"aligned" in L.dsrg_last_error()
    assert call(G=1, Hs=_i32([32768]), Ws=_i32([32768])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()
    assert call(cap=16, oh=_i32([5, 8192]), ow=_i32([5, 8192])) == _lib.ERR_UNSUPPORTED and b"2^31" in L.dsrg_last_error()


def test_mirror_entry_points_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from dsrg_amd import _lib
    L = _lib.lib()
    rc = L.dsrg_multiscale_unary_mirror(2, 21, _vp([_FAKE, 512]), _i32([0, 1]), _i32([4, 4]), _i32([5, 5]), 8, 7, 1e-5, _FAKE, None,
                                        None, None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()
    rc = L.dsrg_multiscale_unary_mirror_batch(2, 1, 21, _vp([_FAKE]), _i32([4]), _i32([5]), _i32([8, 3]), _i32([8, 7]), 1e-5,
                                              _vp([_FAKE, 512]), None, None, None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()
    rc = L.dsrg_preprocess_rect_mirror_batch(2, 5, 1, _vp([_FAKE, 512]), _i32([8, 3]), _i32([8, 7]), _i32([5]), _i32([6]),
                                             (ctypes.c_float * 3)(104.0, 117.0, 123.0), _vp([_FAKE]), None)
    assert rc == _lib.ERR_HIP and L.dsrg_last_error()


def test_predict_cli_flip_switch(capsys):
    from dsrg_amd import predict
    common = ["--model", "m", "--images", "i", "--dir", "d", "--output", "o"]

    def rejected(args, message):
        with pytest.raises(SystemExit) as e:
            predict.parse_args(args + common)
        assert e.value.code == 2
        assert message in capsys.readouterr().err

    rejected(["--mode", "gt", "--cues", "c", "--flip"], "--flip is for --mode ms and --mode ms-f only")
    rejected(["--mode", "ms", "--flip", "--forward-batch", "9"], "at most 8")
    rejected(["--mode", "ms-f", "--flip", "--same-size-batch", "9"], "at most 8")
    rejected(["--mode", "ms", "--flip", "--scales", "97,129,161,193,225"], "at most 4 scales")
    rejected(["--mode", "ms-f", "--flip", "--scales", "0.5,0.75,1,1.25,1.5"], "at most 4 scales")
    assert predict.parse_args(["--mode", "ms"] + common).flip is False
    assert predict.parse_args(["--mode", "ms-f"] + common).flip is False
    a = predict.parse_args(["--mode", "ms", "--flip", "--forward-batch", "8", "--scales", "97,129,161,193"] + common)
    assert a.flip is True and a.forward_batch == 8
    a = predict.parse_args(["--mode", "ms-f", "--flip", "--same-size-batch", "8", "--backbone", "resnet101"] + common)
    assert a.flip is True and a.same_size_batch == 8
    assert predict.parse_args(["--mode", "ms", "--forward-batch", "16"] + common).forward_batch == 16      # (without flip: as before)


def test_flip_limits_raise_before_any_launch():
    """five scales or a group of nine: ValueError from the call's own checks.  Neither a network nor a GPU is needed to get
    there (net=None: anything later would fail differently)"""
    from dsrg_amd import inference as I
    im = np.zeros((12, 14, 3), np.uint8)
    five, rel5 = (33, 41, 49, 57, 65), (0.5, 0.75, 1.0, 1.25, 1.5)
    with pytest.raises(ValueError, match="at most 4 scales"):
        I.predict_mask_ms(None, im, sizes=five, flip=True)
    with pytest.raises(ValueError, match="at most 4 scales"):
        I.predict_mask_ms_f(None, im, scales=rel5, flip=True)
    with pytest.raises(ValueError, match="at most 4 scales"):
        next(I.predict_masks_ms_many(None, [im], sizes=five, flip=True))
    with pytest.raises(ValueError, match="at most 4 scales"):
        next(I.predict_masks_ms_f_many(None, [im], scales=rel5, flip=True))
    with pytest.raises(ValueError, match="at most 4 scales"):
        I.predict_masks_ms_batched(None, [im], sizes=five, flip=True)
    with pytest.raises(ValueError, match="at most 8 images"):
        next(I.predict_masks_ms_many(None, [im] * 9, forward_batch=9, flip=True))
    with pytest.raises(ValueError, match="at most 8 images"):
        next(I.predict_masks_ms_f_many(None, [im] * 9, same_size_batch=9, flip=True))
    with pytest.raises(ValueError, match="at most 8 images"):
        I.predict_masks_ms_batched(None, [im] * 9, flip=True)
    with pytest.raises(ValueError, match="at most 8 images"):
        I.predict_masks_ms_batched(None, [im], capacity=9, flip=True)
    assert I.MAX_FLIP_SCALES == 4 and I.MAX_FLIP_BATCH == 8


def test_restatement_agrees_with_zoom_of_flipped_maps_on_the_cpu():
    """the restatement against the torch composition it restates, both on the CPU: inference._zoom (float64 upsample_bilinear2d,
    align_corners) of torch.flip-ped maps, summed in float32 in list order.  Both blend in float64 and round once, so a z_k
    can differ only where torch's compiled blend contracts a product into an FMA: by one float32 ulp u of the largest |z_k| (or,
    where the blend cancels, of 1e-7 of the largest score: the floor test_multiscale_unary_kernel_matches_the_torch_composition
    uses).  The K - 1 float32 additions carry those K u on and may each round the other way, by an ulp of a partial sum that is
    at most K times the largest |z_k|: |difference| <= K u + (K - 1) ulp(K max|z_k|).  And 0.999 of all values are bit-equal
    (the share that test demands of the kernel's sum)"""
    from dsrg_amd import inference as I
    n = n_equal = 0
    for C in _LABELS:
        for K, flags, sizes, (H, W), seed in _kernel_cases(C):
            maps = _host_maps(seed, C, sizes)
            got = mirror_sum_reference(maps, flags, H, W)
            zs = [I._zoom(torch.flip(torch.from_numpy(m)[None], [-1]) if f else torch.from_numpy(m)[None], H, W)
                  for m, f in zip(maps, flags)]
            total = zs[0]
            for z in zs[1:]:
                total = total + z
            want = total[0].permute(1, 2, 0).numpy()
            assert got.shape == want.shape == (H, W, C) and got.dtype == want.dtype == np.float32
            zmax = torch.stack([z[0].abs() for z in zs]).amax(0).permute(1, 2, 0).numpy()
            smax = np.float32(max(float(np.abs(m).max()) for m in maps))
            zfloor = np.maximum(zmax, 1e-7 * smax).astype(np.float32)
            tol = K * np.spacing(zfloor).astype(np.float64) + (K - 1) * np.spacing(np.float32(K) * zfloor).astype(np.float64)
            d = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert (d <= tol).all(), (C, K, flags, sizes, H, W, float(d.max()))
            n += d.size
            n_equal += int((d == 0).sum())
    print("restatement bit-equal to _zoom of flipped maps on %.6f of %d values" % (n_equal / n, n))
    assert n_equal >= 0.999 * n
    # a mirrored map is not the plain map: the flags matter
    m = _host_maps(1, 2, [(5, 7)])
    assert not np.array_equal(mirror_sum_reference(m, [0], 13, 11), mirror_sum_reference(m, [1], 13, 11))
    assert np.array_equal(mirror_sum_reference(m, [1], 13, 11), mirror_sum_reference([m[0][:, :, ::-1]], [0], 13, 11))


def _zoom_steps_sum(maps, flags, H, W, device):
    """the torch composition of predict_mask_ms_f(flip=True, fused=False) on given maps -> (H, W, C) float32 numpy"""
    from dsrg_amd import inference as I
    total = None
    for m, f in zip(maps, flags):
        t = torch.from_numpy(m)[None].to(device)
        z = I._zoom_steps(torch.flip(t, [-1]) if f else t, H, W)
        total = z if total is None else total + z
    return total[0].permute(1, 2, 0).cpu().numpy()


def test_zoom_steps_is_the_restatement_bit_for_bit_and_zoom_to_the_last_bit():
    """inference._zoom_steps (the zoom of the fused=False composition with flip) on the CPU: the restatement's arithmetic op by
    op, so equal bit for bit; and _zoom itself within one float32 ulp of the value, which is all a contracted product can move"""
    from dsrg_amd import inference as I
    for C in (1, 21):
        for K, flags, sizes, (H, W), seed in _kernel_cases(C):
            maps = _host_maps(seed, C, sizes)
            assert np.array_equal(_zoom_steps_sum(maps, flags, H, W, "cpu"), mirror_sum_reference(maps, flags, H, W)), (C, K, sizes, H, W)
            t = torch.from_numpy(maps[0])[None]
            a, b = I._zoom_steps(t, H, W), I._zoom(t, H, W)
            assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
            floor = 1e-7 * float(t.abs().max())
            ulp = np.spacing(np.maximum(np.abs(b.numpy()), floor).astype(np.float32))
            assert (np.abs(a.double().numpy() - b.double().numpy()) <= ulp).all(), (C, sizes[0], H, W)


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zoom_steps_on_the_gpu_is_the_restatement_bit_for_bit():
    for K, flags, sizes, (H, W), seed in _kernel_cases(21):
        maps = _host_maps(seed, 21, sizes)
        assert np.array_equal(_zoom_steps_sum(maps, flags, H, W, "cuda"), mirror_sum_reference(maps, flags, H, W)), (K, sizes, H, W)


_NAMES = ("unary", "argmax", "sum")


def _assert_same(got, want, tag):
    for n, a, b in zip(_NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (n,) + tag
        assert torch.equal(a, b), "%s differs: %s" % (n, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("C", _LABELS)
def test_multiscale_unary_mirror_with_no_flag_set_is_the_plain_kernel(C):
    from dsrg_amd import ops
    for K, _, sizes, (H, W), seed in _kernel_cases(C):
        scores = [torch.from_numpy(m)[None].cuda() for m in _host_maps(seed, C, sizes)]
        want = ops.multiscale_unary(scores, H, W, eps=1e-5, want=_NAMES)
        got = ops.multiscale_unary(scores, H, W, eps=1e-5, want=_NAMES, mirror=[0] * K)
        _assert_same(got, want, (C, K, sizes, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("C", _LABELS)
def test_multiscale_unary_mirror_equals_the_plain_kernel_on_flipped_maps_and_the_restatement(C):
    from dsrg_amd import ops
    flagged = 0
    for K, flags, sizes, (H, W), seed in _kernel_cases(C):
        maps = _host_maps(seed, C, sizes)
        scores = [torch.from_numpy(m)[None].cuda() for m in maps]
        flipped = [torch.flip(s, [-1]).contiguous() if f else s for s, f in zip(scores, flags)]
        want = ops.multiscale_unary(flipped, H, W, eps=1e-5, want=_NAMES)
        got = ops.multiscale_unary(scores, H, W, eps=1e-5, want=_NAMES, mirror=flags)
        _assert_same(got, want, (C, K, flags, sizes, H, W))
        assert torch.equal(ops.multiscale_unary(scores, H, W, want="argmax", mirror=flags), got[1])
        ref = mirror_sum_reference(maps, flags, H, W)
        assert np.array_equal(got[2].cpu().numpy(), ref), "sum differs from the restatement: %s" % ((C, K, flags, sizes, H, W),)
        flagged += sum(flags)
    assert flagged > 0
    with pytest.raises(ValueError):
        ops.multiscale_unary(scores, H, W, mirror=[1])                 # one flag per map


def _batch_case(rng, G, K, C, Gcap):
    sizes = [_MAPS[(G + k) % len(_MAPS)] for k in range(K)]
    shapes = [_OUTS[(G + g) % len(_OUTS)] for g in range(G)]           # differing (H_g, W_g) within the group
    scores = [torch.from_numpy((rng.standard_normal((Gcap, C, h, w)) * 3.0).astype(np.float32)).cuda() for h, w in sizes]
    return sizes, shapes, scores


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4])
def test_multiscale_unary_mirror_batch_equals_the_single_image_form(K):
    from dsrg_amd import ops
    rng = np.random.default_rng(60 + K)
    for G in (1, 3, 8):
        for C in _LABELS:
            Gcap = 2 * G + 1 + (C % 2)                                  # more slices than the pairs
            sizes, shapes, scores = _batch_case(rng, G, K, C, Gcap)
            got = ops.multiscale_unary_mirror_batch(scores, shapes, eps=1e-5, want=_NAMES)
            assert len(got) == G
            for g, (H, W) in enumerate(shapes):
                pairs = [s[j:j + 1] for s in scores for j in (2 * g, 2 * g + 1)]          # scale-major: plain, mirror
                want = ops.multiscale_unary(pairs, H, W, eps=1e-5, want=_NAMES, mirror=[0, 1] * K)
                _assert_same(got[g], want, (G, K, C, g))
            only = ops.multiscale_unary_mirror_batch(scores, shapes, want="sum")
            assert isinstance(only, list) and all(torch.equal(o, t[2]) for o, t in zip(only, got))
    s = torch.zeros(6, 21, 4, 5, device="cuda")
    with pytest.raises(ValueError):
        ops.multiscale_unary_mirror_batch([s], [(8, 8)] * 4)           # 4 images need 8 slices
    from dsrg_amd import _lib
    with pytest.raises(_lib.DsrgError):
        ops.multiscale_unary_mirror_batch([torch.zeros(18, 2, 4, 5, device="cuda")], [(8, 8)] * 9)
    with pytest.raises(_lib.DsrgError):
        ops.multiscale_unary_mirror_batch([torch.zeros(2, 2, 4, 5, device="cuda")] * 5, [(8, 8)])


@pytest.mark.gpu
def test_preprocess_rect_mirror_batch_fills_slot_pairs():
    """even slots: preprocess_rect_batch's outputs; odd slots: torch.flip of them; the tail slots: zeros; all bit for bit"""
    from dsrg_amd import ops
    rng = np.random.default_rng(71)
    im_shapes = [(33, 33), (12, 9), (1, 1), (1, 57), (43, 1), (2, 3), (20, 31), (7, 8)]
    images = [torch.from_numpy(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda() for H, W in im_shapes]
    out_shapes = [(5, 1), (3, 2), (9, 7), (4, 8), (1, 1), (17, 33)]      # widths 1, 2, 7, 8 and a row longer than a wave half
    for G in (1, 3, 8):
        dev = images[:G]
        cap = 2 * G + 3
        plain = ops.preprocess_rect_batch(dev, out_shapes)
        got = ops.preprocess_rect_mirror_batch(dev, out_shapes, capacity=cap)
        again = ops.preprocess_rect_mirror_batch(dev, out_shapes, capacity=cap, out=[torch.full_like(o, 7.0) for o in got])
        exact = ops.preprocess_rect_mirror_batch(dev, out_shapes)         # the default capacity: 2 G
        assert len(got) == len(out_shapes)
        for (h, w), p, o, o2, e in zip(out_shapes, plain, got, again, exact):
            assert tuple(o.shape) == (cap, 3, h, w) and o.dtype == torch.float32 and o.is_contiguous()
            assert tuple(e.shape) == (2 * G, 3, h, w)
            assert torch.equal(o[0:2 * G:2], p), "even slots differ from preprocess_rect_batch (G %d, %dx%d)" % (G, h, w)
            assert torch.equal(o[1:2 * G:2], torch.flip(p, [-1])), "odd slots are not the mirrored inputs (G %d, %dx%d)" % (G, h, w)
            assert (o[2 * G:] == 0).all(), "the tail slots must be zero"
            assert torch.equal(o, o2), "the out= route differs / leaves values unwritten"
            assert torch.equal(e, o[:2 * G])
    # the fixed sizes of test-ms.py are the square case
    sq = ops.preprocess_rect_mirror_batch(images[:2], [(17, 17)])[0]
    assert torch.equal(sq[0::2], ops.preprocess_ms_batch(images[:2], [17])[0])
    with pytest.raises(ValueError):
        ops.preprocess_rect_mirror_batch(images[:2], [(5, 5)], capacity=3)
    with pytest.raises(ValueError):
        ops.preprocess_rect_mirror_batch(images[:1], [(5, 5)], out=[torch.zeros(1, 3, 5, 5, device="cuda")])


# ---- GPU: end to end --------------------------------------------------------------------------------------------------------------
class ColumnNet(torch.nn.Module):
    """a deterministic stand-in for the deploy net whose scores depend on the column: a stride-8 convolution plus a per-label
    ramp over the columns of the map, so the scores of a mirrored input are not the mirrored scores and flip=True must change
    the result"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(21, 3, 9, 9, generator=g) * 0.02)
        self.slope = torch.nn.Parameter(torch.randn(21, generator=g) * 4.0)

    def forward(self, x):
        y = torch.nn.functional.conv2d(x, self.w, stride=8, padding=4)
        ramp = torch.linspace(-1.0, 1.0, y.shape[3], device=y.device, dtype=y.dtype)
        return y + self.slope.to(y.dtype).view(1, -1, 1, 1) * ramp.view(1, 1, 1, -1)


def _image(rng, H, W, kind="smooth"):
    from dsrg_amd import synthetic as S
    im = (S.make_images(rng, 1, size=max(H, W), kind=kind)[0, :, :H, :W] + S.MEAN_PIXEL[:, None, None]).transpose(1, 2, 0)
    return np.ascontiguousarray(im[:, :, ::-1]).clip(0, 255).astype(np.uint8)


_E2E_SHAPES = [(97, 131), (97, 131), (97, 131), (120, 90), (66, 70), (97, 131)]
_E2E_SIZES = (73, 97, 121)
_E2E_SCALES = (0.75, 1.0, 1.25)


def _e2e_images(seed):
    rng = np.random.default_rng(seed)
    return [_image(rng, H, W, kind=["smooth", "noise", "dark_corner"][k % 3]) for k, (H, W) in enumerate(_E2E_SHAPES)]


def _pair_batch(x, n, B):
    """the slots of the batched flip forwards from the existing kernels' outputs: x (>= n, 3, h, w) -> (B, 3, h, w) with image g
    in slot 2g, torch.flip of it in slot 2g+1 and zeros behind"""
    X = torch.zeros((B,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    X[0:2 * n:2] = x[:n]
    X[1:2 * n:2] = torch.flip(x[:n], [-1])
    return X


def _staged_tail(scores, g, im, smooth):
    """image g of a batched flip forward through the existing single-image kernel and torch.flip -> (H,W) int64 mask"""
    from dsrg_amd import ops
    from dsrg_amd.crf import CRF_device
    maps = [t for s in scores for t in (s[2 * g:2 * g + 1], torch.flip(s[2 * g + 1:2 * g + 2], [-1]).contiguous())]
    H, W = im.shape[0], im.shape[1]
    if smooth:
        unary = ops.multiscale_unary(maps, H, W, eps=0.00001, want="unary")
        return CRF_device(im, unary, scale_factor=1.0, want="map").cpu().numpy().astype(np.int64)
    return ops.multiscale_unary(maps, H, W, eps=0.00001, want="argmax").cpu().numpy().astype(np.int64)


def _staged_ms(fwd, ims, G, sizes, smooth):
    """the batched ms path with flip, composed from the existing functions plus torch.flip: ops.preprocess_ms_batch, the same
    batch-2G forwards (tail group padded with zeros), ops.multiscale_unary on flipped copies, CRF_device"""
    from dsrg_amd import ops
    masks = []
    with torch.no_grad():
        for start in range(0, len(ims), G):
            dev = [torch.from_numpy(im).cuda() for im in ims[start:start + G]]
            xs = ops.preprocess_ms_batch(dev, sizes, capacity=G)
            scores = [fwd(_pair_batch(x, len(dev), 2 * G)).float().contiguous() for x in xs]
            masks += [_staged_tail(scores, g, im, smooth) for g, im in enumerate(dev)]
    return masks


def _staged_ms_f(fwd, group, scales, smooth):
    """one same-sized group of the batched ms-f path with flip, composed likewise (ops.preprocess_rect_batch)"""
    from dsrg_amd import inference as I, ops
    H, W = group[0].shape[:2]
    shapes = [(I.relative_size(H, s), I.relative_size(W, s)) for s in scales]
    with torch.no_grad():
        dev = [torch.from_numpy(im).cuda() for im in group]
        xs = ops.preprocess_rect_batch(dev, shapes)
        scores = [fwd(_pair_batch(x, len(dev), 2 * len(dev))).float().contiguous() for x in xs]
        return [_staged_tail(scores, g, im, smooth) for g, im in enumerate(dev)]


def _assert_masks_equal(got, want, ims, tag):
    assert len(got) == len(want) == len(ims), tag
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], (tag, k)
        assert np.array_equal(a, b), "%s: mask %d differs from the staged composition on %d pixels" % (tag, k, int((a != b).sum()))


_SUM_SHAPES = ((97, 131), (66, 70), (41, 57))
_SUMS = {}


def _flip_sums(H, W):
    """the summed scores of one image through predict_mask_ms_f's three routes -> (fused flip, fused=False flip, fused plain, the
    per-pixel largest |z_k| of the flip composition); computed once per shape and shared"""
    from dsrg_amd import inference as I
    if (H, W) not in _SUMS:
        net = ColumnNet().cuda().eval()
        im = _image(np.random.default_rng(81 + H), H, W, kind="noise")
        with torch.no_grad():
            fused = I._relative_unary(net, im, _E2E_SCALES, "cuda", None, True, True, flip=True, want="sum")
            comp = I._relative_unary(net, im, _E2E_SCALES, "cuda", None, False, True, flip=True, want="sum")
            plain = I._relative_unary(net, im, _E2E_SCALES, "cuda", None, True, True, flip=False, want="sum")
            maps = I._flip_pair_scores(net, [I.preprocess_relative(im, s, "cuda") for s in _E2E_SCALES], None)
            zmax = torch.stack([I._zoom(torch.flip(m, [-1]) if k % 2 else m, H, W)[0].abs() for k, m in enumerate(maps)]).amax(0)
            smax = max(float(m.abs().max()) for m in maps)
        _SUMS[(H, W)] = (im, fused, comp, plain, zmax.permute(1, 2, 0), smax)
    return _SUMS[(H, W)]


@pytest.mark.gpu
def test_predict_mask_ms_f_flip_fused_equals_the_torch_composition_on_the_sum():
    """the summed scores of predict_mask_ms_f(flip=True) through the fused kernel and through fused=False (torch.flip of the
    mirrors' scores, the zoom, the sum in the same order): bit for bit.

    The composition zooms with inference._zoom_steps (_zoom's arithmetic, every product and sum rounded on its own, as the
    kernel rounds them): through _zoom itself, torch's float64 upsample_bilinear2d, whose compiled blend contracts products into
    FMAs, 0.999389 - 0.999969 of these values were bit-equal on an MI355X and the others one float32 ulp off"""
    rows = []
    for H, W in _SUM_SHAPES:
        _, fused, comp, _, _, _ = _flip_sums(H, W)
        assert fused.shape == comp.shape == (H, W, 21)
        rows.append((H, W, float((fused == comp).float().mean()), float((fused - comp).abs().max())))
        print("%dx%d: fused sum bit-equal to the torch composition on %.6f of the values, largest difference %.3g" % rows[-1])
    assert all(torch.equal(_flip_sums(H, W)[1], _flip_sums(H, W)[2]) for H, W in _SUM_SHAPES), rows


@pytest.mark.gpu
def test_predict_mask_ms_f_flip_fused_agrees_with_the_torch_composition():
    """the two routes of the test above within the bound of test_restatement_agrees_with_zoom_of_flipped_maps_on_the_cpu (one
    contracted rounding per map, carried through the float32 sum: K u + (K - 1) ulp(K max|z_k|) for the K = 6 maps) and bit-equal
    on 0.999 of the values; and flip=True is not flip=False: the sums and the masks differ"""
    from dsrg_amd import inference as I
    net = ColumnNet().cuda().eval()
    K = 2 * len(_E2E_SCALES)
    differ = 0
    for H, W in _SUM_SHAPES:
        im, fused, comp, plain, zmax, smax = _flip_sums(H, W)
        zfloor = np.maximum(zmax.cpu().numpy(), 1e-7 * np.float32(smax)).astype(np.float32)
        tol = K * np.spacing(zfloor).astype(np.float64) + (K - 1) * np.spacing(np.float32(K) * zfloor).astype(np.float64)
        d = (fused.double() - comp.double()).abs().cpu().numpy()
        assert (d <= tol).all(), (H, W, float(d.max()))
        assert (d == 0).mean() >= 0.999
        assert not torch.equal(fused, plain)
        for smooth in (True, False):
            a = I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth, flip=True)
            b = I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth, flip=False)
            c = I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth, flip=True, fused=False)
            assert a.shape == b.shape == (H, W) and a.dtype == np.int64
            assert (a == c).mean() >= 0.999
            differ += int((a != b).sum())
    assert differ > 0, "a silently ignored flip flag: the flipped and the plain predictions are equal"


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
def test_batched_flip_paths_equal_the_staged_composition(graphed):
    from dsrg_amd import inference as I
    ims = _e2e_images(83)
    net = ColumnNet().cuda().eval()
    G = 4                                                               # 6 images: a full group and a tail group of 2, padded

    def forward():
        return I.GraphedForward(net) if graphed else None

    ref_fwd = forward()
    want = _staged_ms(ref_fwd or net, ims, G, _E2E_SIZES, True)
    want_plain = _staged_ms(ref_fwd or net, ims, G, _E2E_SIZES, False)
    assert max(len(np.unique(m)) for m in want_plain) >= 2, "the stand-in net must give masks of several labels"
    for in_flight, batch in ((2, 1), (3, 2)):
        fwd = forward()
        got = list(I.predict_masks_ms_many(net, iter(ims), sizes=_E2E_SIZES, forward=fwd, in_flight=in_flight, batch=batch,
                                           forward_batch=G, flip=True))
        _assert_masks_equal(got, want, ims, "ms in_flight %d batch %d" % (in_flight, batch))
        if graphed:
            assert sorted(key[0] for key in fwd._g) == sorted((2 * G, 3, S, S) for S in _E2E_SIZES)    # batch-2G graphs only
    fwd = forward()
    for smooth, ref in ((True, want), (False, want_plain)):
        got = I.predict_masks_ms_batched(net, ims[0:4], smooth=smooth, sizes=_E2E_SIZES, forward=fwd, flip=True) + \
            I.predict_masks_ms_batched(net, ims[4:6], smooth=smooth, sizes=_E2E_SIZES, forward=fwd, capacity=G, flip=True)
        _assert_masks_equal(got, ref, ims, "predict_masks_ms_batched smooth=%s" % smooth)
    no_flip = list(I.predict_masks_ms_many(net, ims, sizes=_E2E_SIZES, forward_batch=G))
    assert any(not np.array_equal(a, b) for a, b in zip(no_flip, want)), "flip=True must change the masks of this net"

    # ms-f: the three 97 x 131 images that open the list form one group of 3; (120, 90) and (66, 70) groups of one
    idx3 = [k for k, s in enumerate(_E2E_SHAPES) if s == (97, 131)][:3]
    part = ims[:5]
    ref_fwd = forward()
    for smooth in (True, False):
        want_f = [None] * len(part)
        for group_idx in (idx3, [3], [4]):
            for k, m in zip(group_idx, _staged_ms_f(ref_fwd or net, [part[k] for k in group_idx], _E2E_SCALES, smooth)):
                want_f[k] = m
        fwd = forward()
        got = list(I.predict_masks_ms_f_many(net, iter(part), scales=_E2E_SCALES, forward=fwd, in_flight=2, batch=2,
                                             same_size_batch=3, smooth=smooth, flip=True))
        _assert_masks_equal(got, want_f, part, "ms-f same_size_batch=3 smooth=%s" % smooth)
        if graphed:
            assert all(key[0][0] in (6, 2) for key in fwd._g)           # batch-2n graphs: 6 for the group of 3, 2 for the singles


@pytest.mark.gpu
def test_batched_flip_paths_agree_with_the_per_image_path():
    """batch-2G and batch-2 forwards need not agree bit for bit: the bar of
    test_predict_masks_ms_many_forward_batch_agrees_with_the_per_image_path — agreement above 0.999 per image, every differing
    pixel with a top-2 margin below 1e-3 in the per-image path's CRF marginals (smooth) or probabilities (smooth=False)"""
    from dsrg_amd import inference as I
    from dsrg_amd.crf import CRF_device
    ims = _e2e_images(87)
    net = ColumnNet().float().cuda().eval()
    got_ms = {True: list(I.predict_masks_ms_many(net, ims, sizes=_E2E_SIZES, forward_batch=4, flip=True)),
              False: [m for s in range(0, len(ims), 4)
                      for m in I.predict_masks_ms_batched(net, ims[s:s + 4], smooth=False, sizes=_E2E_SIZES, capacity=4, flip=True)]}
    got_f = {smooth: list(I.predict_masks_ms_f_many(net, ims, scales=_E2E_SCALES, same_size_batch=3, smooth=smooth, flip=True))
             for smooth in (True, False)}
    for k, im in enumerate(ims):
        dev = torch.as_tensor(im, device="cuda")
        with torch.no_grad():
            unary_ms = I._ms_flip_result(net, im, _E2E_SIZES, "cuda", None, "unary")
            unary_f = I._relative_unary(net, im, _E2E_SCALES, "cuda", None, True, True, flip=True)
        for tag, got, unary, one in (
                ("ms", got_ms, unary_ms, lambda smooth: I.predict_mask_ms(net, im, smooth=smooth, sizes=_E2E_SIZES, flip=True)),
                ("ms-f", got_f, unary_f, lambda smooth: I.predict_mask_ms_f(net, im, scales=_E2E_SCALES, smooth=smooth, flip=True))):
            with torch.no_grad():
                q = CRF_device(dev, unary, scale_factor=1.0)
            for smooth, ref in ((True, q.cpu().numpy()), (False, torch.exp(unary).cpu().numpy())):
                want = one(smooth)
                top2 = np.sort(ref, axis=2)[:, :, -2:]
                margin = top2[:, :, 1] - top2[:, :, 0]
                bad = got[smooth][k] != want
                agree = 1.0 - bad.mean()
                print("%s image %d smooth=%s: agreement with the per-image flip path %.6f; %d differing pixels, largest top-2 margin "
                      "among them %.3g" % (tag, k, smooth, agree, int(bad.sum()), float(margin[bad].max()) if bad.any() else 0.0))
                assert got[smooth][k].shape == want.shape and got[smooth][k].dtype == np.int64
                assert agree > 0.999
                assert not bad.any() or margin[bad].max() < 1e-3


def _vgg(num_classes=21, seed=0):
    """VGG16-ASPP in eval mode with He-initialised convolutions and zero biases, so that the scores of a random net vary over the
    image and the masks hold several labels"""
    from dsrg_amd.backbone import VGG16ASPP
    torch.manual_seed(seed)
    net = VGG16ASPP(num_classes=num_classes)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                torch.nn.init.zeros_(m.bias)
    return net.cuda().to(memory_format=torch.channels_last).eval()


@pytest.mark.gpu
def test_flip_on_vgg16_aspp_with_a_graphed_batch_2_forward():
    """VGG16-ASPP under bf16 autocast at 97 x 129 with flip=True: the batch-2 graphs capture (first call) and replay (second
    call), and both give the masks of the eager run"""
    from dsrg_amd import inference as I
    im = _image(np.random.default_rng(91), 97, 129, kind="noise")
    scales = (0.75, 1.0)
    net = _vgg()
    fwd = I.GraphedForward(net)
    labels = set()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for smooth in (True, False):
            eager = I.predict_mask_ms_f(net, im, scales=scales, smooth=smooth, flip=True)
            captured = I.predict_mask_ms_f(net, im, scales=scales, smooth=smooth, forward=fwd, flip=True)
            replayed = I.predict_mask_ms_f(net, im, scales=scales, smooth=smooth, forward=fwd, flip=True)
            assert eager.shape == (97, 129) and eager.dtype == np.int64
            assert np.array_equal(captured, eager), "smooth=%s: %d pixels differ at the capture" % (smooth, int((captured != eager).sum()))
            assert np.array_equal(replayed, eager), "smooth=%s: %d pixels differ at the replay" % (smooth, int((replayed != eager).sum()))
            labels |= set(np.unique(eager).tolist())
    assert sorted(key[0] for key in fwd._g) == sorted((2, 3, I.relative_size(97, s), I.relative_size(129, s)) for s in scales)
    print("VGG16-ASPP flip=True, batch-2 graphs: %d labels in the masks" % len(labels))
    assert len(labels) >= 2
