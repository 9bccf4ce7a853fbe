"""The direct 3x3 convolutions (csrc/conv_direct.hip) with MANY tiles per persistent workgroup, bit for bit.

The kernels finish an M-tile under the MFMAs of the next one and carry it — accumulators, store offsets, mask vectors — across
tile boundaries; a drain behind the tile loop finishes the last one.  tests/test_gpu_exact_conv.py runs maps of at most 20
tiles, where every workgroup has exactly one tile: the one path that carried state does not exercise.  Here the tests-only
knob dsrg_debug_set_direct_grid caps the launch at 1, 2, 3 and 7 workgroups — odd and even tile counts per workgroup, up to
all 20 tiles on one — on the same exact-integer data and float64 references as that file (no tolerance).  With one workgroup
the tiles are processed in raster order, so a store that runs past x = W lands on a pixel of the next row that is already
written and stays wrong: edge overruns show deterministically.  The masked form's bias gradient is compared exactly too
(integer sums do not depend on the association).  A last test asserts on random bf16 data that the outputs do not depend on
the grid at all."""
import pytest
import torch

from test_gpu_exact_conv import (_bounded, _dev, _dgrad64, _fwd_case, _gen, _ints, _masked, _nonvacuous, _post, _relu_out, _rounded,
                                 _same, ops)  # noqa: F401  (ops: the module's fixture)

gpu = pytest.mark.gpu
CL = torch.channels_last
MAPS = [(2, 33, 29), (2, 17, 40), (1, 1, 1)]              # 20 and 18 tiles, ragged on both axes; the drain with nothing before it
CAPS = [1, 2, 3, 7]
SHAPES = [(64, 64), (64, 128), (128, 128), (128, 64)]


class _grid(object):
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from dsrg_amd import _lib
        _lib.lib().dsrg_debug_set_direct_grid(int(self.n))

    def __exit__(self, *exc):
        from dsrg_amd import _lib
        _lib.lib().dsrg_debug_set_direct_grid(0)


_CASES = {}


def _forward_case(cin, cout, B, H, W):
    """data and the four expected tensors (bias x relu), computed once per shape and map and left unchanged"""
    key = ("f", cin, cout, B, H, W)
    if key not in _CASES:
        full = (H, W) != (1, 1)
        x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, 3, 1, 11, full_window=full)
        want = {}
        for bias in (False, True):
            for relu in (False, True):
                what = "%d -> %d, %dx%dx%d bias %d relu %d" % (cin, cout, B, H, W, bias, relu)
                want[bias, relu] = _rounded(_post(ref, b if bias else None, relu), full, what, relu)
        _CASES[key] = (x.to(torch.bfloat16), w.to(torch.bfloat16), b.float(), want, (x, w, b))
    return _CASES[key]


def _gradient_case(cf, cb, B, H, W):
    key = ("g", cf, cb, B, H, W)
    if key not in _CASES:
        gen = _gen(21)
        g, w, y = _ints((B, cf, H, W), -8, 8, gen), _ints((cf, cb, 3, 3), -4, 4, gen), _relu_out((B, cb, H, W), 8, gen)
        ref = _dgrad64(g, w, 1, (H, W))
        _bounded(_dgrad64(g.abs(), w.abs(), 1, (H, W)).max())
        full = (H, W) != (1, 1)
        if full:
            _nonvacuous(ref[y > 0], "masked data gradient")
        plain = _rounded(ref, full, "data gradient")
        stored, sums = _masked(ref, y, 1.0)
        _CASES[key] = (g, w.flip(2, 3).transpose(0, 1).contiguous(), y, plain, stored, sums)
    return _CASES[key]


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_direct_forward_is_exact_with_many_tiles_per_workgroup(ops, cin, cout, cap):
    for B, H, W in MAPS:
        _, _, _, want, (x, w, b) = _forward_case(cin, cout, B, H, W)
        xd, wd, bd = _dev(x), _dev(w), _dev(b, torch.float32)
        with _grid(cap):
            for (bias, relu), expected in want.items():
                got = ops.conv3x3_direct(xd, wd, bd if bias else None, relu)
                _same(got, expected, "%d -> %d, %dx%dx%d bias %d relu %d, %d workgroups" % (cin, cout, B, H, W, bias, relu, cap))


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cf,cb", SHAPES)
def test_direct_data_gradient_is_exact_with_many_tiles_per_workgroup(ops, cf, cb, cap):
    """cf: channels of the incoming gradient, cb: of the layer below, whose ReLU backward and bias gradient ride along"""
    for B, H, W in MAPS:
        g, wt, y, plain, stored, sums = _gradient_case(cf, cb, B, H, W)
        gd, wd, yd = _dev(g), _dev(wt), _dev(y)
        what = "%d -> %d, %dx%dx%d, %d workgroups" % (cf, cb, B, H, W, cap)
        with _grid(cap):
            _same(ops.conv3x3_direct(gd, wd, None, False), plain, what + ": plain")
            gx, gb = ops.conv3x3_direct_dgrad(gd, wd, yd)
        _same(gx, stored, what + ": gx")
        _same(gb, sums, what + ": bias gradient")


@gpu
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_direct_outputs_do_not_depend_on_the_grid(ops, cin, cout):
    """random, non-integer bf16 data on a (3, 61, 70) map (120 tiles): y and gx under 1, 7, 64 workgroups and the default grid
    are the same bits.  (The bias gradient is left out: its summation order follows the grid by design.)"""
    gen = _gen(5)
    x = torch.randn(3, cin, 61, 70, generator=gen).bfloat16().cuda().contiguous(memory_format=CL)
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.05).bfloat16().cuda().contiguous(memory_format=CL)
    b = torch.randn(cout, generator=gen).cuda()
    mask = torch.relu(torch.randn(3, cout, 61, 70, generator=gen)).bfloat16().cuda().contiguous(memory_format=CL)
    outs = []
    for cap in (0, 1, 7, 64):
        with _grid(cap):
            outs.append((ops.conv3x3_direct(x, w, b, True), ops.conv3x3_direct(x, w, None, False), ops.conv3x3_direct_dgrad(x, w, mask)[0]))
    assert float(outs[0][0].float().abs().sum()) > 0 and float(outs[0][2].float().abs().sum()) > 0
    for cap, got in zip((1, 7, 64), outs[1:]):
        for name, r, o in zip(("y with bias and relu", "y", "gx"), outs[0], got):
            assert torch.equal(r, o), "%d -> %d, %s: %d workgroups differ from the default grid" % (cin, cout, name, cap)
