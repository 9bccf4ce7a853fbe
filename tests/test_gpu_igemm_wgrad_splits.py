"""The weight gradient of dilated 3x3 kernels with its pixel splits chosen per (group, tap) (csrc/conv_igemm.hip: the work list
of a launch, build_wgrad_plan), bit for bit on exact data.

As in test_gpu_exact_conv.py: operands are integers small enough that every product and every partial sum, in whatever order a
kernel adds them and however it cuts them into partial tiles, is an integer below 2^24: every fp32 accumulation is exact, the
float64 CPU gradient of the same operands IS the value, a float32 result must equal it and a bf16 result must be its
round-to-nearest-even.  Each case asserts that bound on its own data and that the values it rounds really need rounding (at least
10 % are not bf16-representable, at least one is an exact tie).  Operand ranges by the same rule as there: x, g in [-8, 8], or
[-32, 32] for a gradient over fewer than 400 pixels.  The result tensors are handed in filled with NaN: an element no workgroup
and no reduction thread writes shows."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
CL = torch.channels_last
LIMIT = float(2 ** 24)
F64 = torch.float64

GROUPED = (2, 26, 29, 256, 256, (6, 12, 18, 24))          # a corner tap of dilation 24 reaches 2 x 5 pixels per image, the centre tap 1 508
EMPTY = (1, 13, 17, 256, 256, (12, 24))                   # dilation 24 exceeds both sides: eight of its nine taps reach nothing
TILE_GRID = (1, 9, 11, 512, 1024, (4, 6))                 # four output tiles x two channel blocks per tap, as fc6 has
# launches that keep ONE split count for all their tiles (B, H, W, cin, cout, k, dilation): 874 and 99 pixels, a ragged last K-step
UNIFORM = [(2, 19, 23, 256, 256, 3, 2), (1, 9, 11, 1024, 1024, 1, 1)]


def _ints(shape, r, gen):
    return torch.randint(-r, r + 1, tuple(shape), generator=gen).to(F64).contiguous(memory_format=CL)


def _wgrad64(x, g, dil, k=3):
    w = torch.zeros(g.shape[1], x.shape[1], k, k, dtype=F64, requires_grad=True)
    F.conv2d(x, w, None, padding=dil * (k // 2), dilation=dil).backward(g)
    return w.grad


def _f32(ref):
    r = ref.float()
    assert torch.equal(r.to(F64), ref), "reference not exact in float32 (the bound should have caught it)"
    return r


def _nonvacuous(rounded, what):
    low = _f32(rounded).contiguous().view(torch.int32).bitwise_and(0xFFFF)
    share, ties = float((low != 0).float().mean()), int((low == 0x8000).sum())
    assert share >= 0.10 and ties >= 1, "%s: %.3f of the values need rounding, %d ties: the rounding is not under test" % (what, share, ties)


_cases = {}


def _case(shape):
    """-> xs, gs, refs (float64, one per group), computed once per shape and never written to; asserts the exactness bound per
    group and non-vacuity over all the values the comparison rounds"""
    if shape not in _cases:
        B, H, W, cin, cout, dils = shape
        gen = torch.Generator().manual_seed(17)
        r = 8 if B * H * W >= 400 else 32
        xs = [_ints((B, cin, H, W), r, gen) for _ in dils]
        gs = [_ints((B, cout, H, W), r, gen) for _ in dils]
        refs = [_wgrad64(x, g, d) for x, g, d in zip(xs, gs, dils)]
        for x, g, d in zip(xs, gs, dils):
            absmax = float(_wgrad64(x.abs(), g.abs(), d).max())
            assert absmax < LIMIT, "inputs too large for exact fp32 sums: %g" % absmax
        _nonvacuous(torch.cat([v.reshape(-1) for v in refs]), "weight gradients of %s" % (shape,))
        _cases[shape] = (xs, gs, refs)
    return _cases[shape]


def _uniform_case(shape):
    """-> x, g, ref of one layer outside the per-tap splits, as _case"""
    if shape not in _cases:
        B, H, W, cin, cout, k, dil = shape
        gen = torch.Generator().manual_seed(19)
        r = 8 if B * H * W >= 400 else 32
        x, g = _ints((B, cin, H, W), r, gen), _ints((B, cout, H, W), r, gen)
        absmax = float(_wgrad64(x.abs(), g.abs(), dil, k).max())
        assert absmax < LIMIT, "inputs too large for exact fp32 sums: %g" % absmax
        ref = _wgrad64(x, g, dil, k)
        _nonvacuous(ref.reshape(-1), "weight gradient of %s" % (shape,))
        _cases[shape] = (x, g, ref)
    return _cases[shape]


def _dev(t):
    d = t.to(torch.bfloat16)
    assert torch.equal(d.to(F64), t), "operand not representable in bf16"
    return d.cuda().contiguous(memory_format=CL)


def _same(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i.tolist())]), float(want[tuple(i.tolist())])) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ; first (index, got, want): %s" % (what, bad.shape[0], want.numel(), first))


def _nan_outs(n, cout, cin, dtype, k=3):
    return [torch.full((cout, cin, k, k), float("nan"), dtype=dtype, device="cuda").contiguous(memory_format=CL) for _ in range(n)]


def _run_exact(ops, shape):
    B, H, W, cin, cout, dils = shape
    xs, gs, refs = _case(shape)
    xd, gd = [_dev(x) for x in xs], [_dev(g) for g in gs]
    n = len(dils)
    got32 = ops.conv_igemm_wgrad(xd, gd, dils, 3, outs=_nan_outs(n, cout, cin, torch.float32))
    got16 = ops.conv_igemm_wgrad(xd, gd, dils, 3, out_dtype=torch.bfloat16, outs=_nan_outs(n, cout, cin, torch.bfloat16))
    for i, d in enumerate(dils):
        _same(got32[i], _f32(refs[i]), "dilation %d, float32" % d)
        _same(got16[i], _f32(refs[i]).bfloat16(), "dilation %d, bf16" % d)
    return got32, got16


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


@pytest.mark.parametrize("shape", [GROUPED, EMPTY, TILE_GRID])
def test_generated_data_is_exact_and_exercises_the_rounding(shape):
    """the CPU half of the cases below: the bound, non-vacuity, and that float32 torch agrees with float64 on this data"""
    B, H, W, cin, cout, dils = shape
    xs, gs, refs = _case(shape)
    w32 = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    F.conv2d(xs[-1].float(), w32, None, padding=dils[-1], dilation=dils[-1]).backward(gs[-1].float())
    assert torch.equal(w32.grad.to(F64), refs[-1])


@gpu
def test_grouped_dilated_launch_with_unequal_splits_is_the_float64_gradient(ops):
    B, H, W, cin, cout, dils = GROUPED
    splits = ops.conv_igemm_wgrad_splits(len(dils), B, H, W, cin, cout, 3, dils)
    flat = [c for grp in splits for c in grp]
    # not vacuous: this launch really runs taps with different split counts, and one with a single split
    assert len(set(flat)) >= 2 and min(flat) == 1 and max(flat) >= 2, splits
    assert splits[3][4] > splits[3][0], splits                                   # dilation 24: centre (1 508 pixels) against corner (20)
    _run_exact(ops, GROUPED)


@gpu
def test_taps_that_reach_no_pixel_are_exact_zeros(ops):
    B, H, W, cin, cout, dils = EMPTY
    splits = ops.conv_igemm_wgrad_splits(len(dils), B, H, W, cin, cout, 3, dils)
    assert [c > 0 for c in splits[1]] == [False] * 4 + [True] + [False] * 4, splits      # no workgroup for an empty rectangle
    assert all(c > 0 for c in splits[0]), splits
    got32, got16 = _run_exact(ops, EMPTY)
    for got in (got32[1], got16[1]):
        dead = got.cpu().float().flatten(2)[:, :, [0, 1, 2, 3, 5, 6, 7, 8]]
        assert torch.equal(dead, torch.zeros_like(dead)) and not torch.signbit(dead).any()


@gpu
def test_the_fc6_tile_grid_at_a_tiny_map(ops):
    _run_exact(ops, TILE_GRID)


@pytest.mark.parametrize("shape", UNIFORM)
def test_generated_data_of_the_uniform_launches_is_exact(shape):
    _uniform_case(shape)


@gpu
@pytest.mark.parametrize("shape", UNIFORM)
def test_launches_outside_the_per_tap_splits_are_the_float64_gradient(ops, shape):
    """dilation 2 and 1x1 keep the uniform split (stand-alone launch) and the merged backward launch: a multi-step reduction with
    a ragged last step through both"""
    B, H, W, cin, cout, k, dil = shape
    x, g, ref = _uniform_case(shape)
    xd, gd = _dev(x), _dev(g)
    assert len(set(ops.conv_igemm_wgrad_splits(1, B, H, W, cin, cout, k, [dil])[0])) == 1       # one count for every tap
    (got32,) = ops.conv_igemm_wgrad([xd], [gd], [dil], k, outs=_nan_outs(1, cout, cin, torch.float32, k))
    (got16,) = ops.conv_igemm_wgrad([xd], [gd], [dil], k, out_dtype=torch.bfloat16, outs=_nan_outs(1, cout, cin, torch.bfloat16, k))
    _same(got32, _f32(ref), "conv_igemm_wgrad, float32")
    _same(got16, _f32(ref).bfloat16(), "conv_igemm_wgrad, bf16")
    if k == 3:
        gen = torch.Generator().manual_seed(29)
        w = torch.randint(-2, 3, (cout, cin, k, k), generator=gen).float().cuda()
        gx, gw, gb = ops.conv_igemm_backward(gd, ops.pack_conv_weight(w, for_dgrad=True), xd, dil,
                                             gw_out=_nan_outs(1, cout, cin, torch.float32, k)[0])
        _same(gw, _f32(ref), "conv_igemm_backward, float32")


@gpu
def test_random_data_is_deterministic_and_close_to_each_branch_alone_and_to_torch(ops):
    B, H, W, cin, cout, dils = GROUPED
    torch.manual_seed(23)
    xs = [torch.randn(B, cin, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in dils]
    gs = [torch.randn(B, cout, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in dils]
    n = len(dils)
    together = ops.conv_igemm_wgrad(xs, gs, dils, 3, outs=_nan_outs(n, cout, cin, torch.float32))
    again = ops.conv_igemm_wgrad(xs, gs, dils, 3, outs=_nan_outs(n, cout, cin, torch.float32))
    for i, d in enumerate(dils):
        assert torch.equal(together[i], again[i]), d                             # two identical calls: identical bits
        (alone,) = ops.conv_igemm_wgrad([xs[i]], [gs[i]], [d], 3)
        assert torch.equal(alone, ops.conv_igemm_wgrad([xs[i]], [gs[i]], [d], 3)[0]), d
        assert (together[i] - alone).abs().max() <= 1e-4 * alone.abs().max(), d  # another pixel split: another summation order
        wr = torch.zeros(cout, cin, 3, 3, device="cuda", requires_grad=True)
        F.conv2d(xs[i].float(), wr, None, padding=d, dilation=d).backward(gs[i].float())
        assert (together[i] - wr.grad).abs().max() <= 2e-3 * wr.grad.abs().max() + 1e-4, d
