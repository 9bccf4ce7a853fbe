"""GPU (-m gpu): the routes of backbone._IgemmConvFn.backward that the VGG16-ASPP step never takes — an input that needs no
gradient, channel counts the data-gradient or the weight-gradient launch does not tile, an input that is not channels_last, and
the separate 1x1 launches — against torch.ops.aten.convolution_backward on float32 copies of the same bf16-valued operands.
Tolerances: test_gpu_igemm.py's for the same kernels (test_igemm_conv_matches_torch for data gradients,
test_igemm_weight_gradient_matches_torch for weight and bias gradients); a weight gradient the library returns in bf16 gets that
format's rounding on top (_close_w)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
B, H, W = 4, 64, 64                     # 64 output tiles of 256 x 256 at 256 output channels: the fewest _igemm_route takes


@pytest.fixture(scope="module")
def backbone():
    from dsrg_amd import backbone, _lib
    _lib.require_gpu()
    return backbone


def _reference(x, w, b, y, g, k, dil, need_x=True):
    """float32 gradients of relu(conv(x, bf16(w)) + b) for the output gradient g, masked where the node's own output y is positive"""
    gm = g.float() * (y > 0)
    p = dil * (k // 2)
    return torch.ops.aten.convolution_backward(gm, x.detach().float(), w.detach().bfloat16().float(), [b.shape[0]], [1, 1], [p, p],
                                               [dil, dil], False, [0, 0], 1, [need_x, True, True])


def _close_x(got, want):
    err = (got.float() - want).abs().max()
    assert err <= 0.01 * want.abs().max() + 1e-3, (float(err), float(want.abs().max()))


def _close_w(got, want, library=False):
    """library: the weight gradient came from the library in bf16 and was cast up (shapes conv_igemm_wgrad does not tile) — every
    element then carries one more rounding to 8 significant bits, at most 2^-8 of its value, which the float32 launch's bound
    cannot hold (measured: 1.90 at an element of 689, bound 1.38)"""
    assert got.dtype == torch.float32 and got.shape == want.shape
    bound = 2e-3 * want.abs().max() + 1e-4 + (2.0 ** -8 * want.abs() if library else 0.0)
    err = (got - want).abs()
    assert bool((err <= bound).all()), (float(err.max()), float(want.abs().max()))


def _layer(backbone, cin, cout, k=3, dil=1, **kw):
    torch.manual_seed(cin + cout)
    m = backbone.GemmConv2d(cin, cout, k, padding=dil * (k // 2), dilation=dil, fuse_relu=True, **kw).cuda().to(memory_format=CL)
    with torch.no_grad():
        m.bias.normal_(0.0, 0.5)
    return m


def _input(cin, seed, layout=CL):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, cin, H, W, device="cuda", generator=g).bfloat16().contiguous(memory_format=layout)


@pytest.mark.parametrize("cin,cout,need_x,layout,dgrad_tiled,wgrad_tiled", [
    (256, 256, False, CL, True, True),                     # no data gradient asked for: the weight gradients' own launch alone
    (192, 256, True, CL, False, False),                    # input channels no multiple of 128: both gradients by the library
    (384, 256, True, CL, True, False),                     # the forward kernel for the data gradient, the library for the weights'
    (256, 256, True, torch.contiguous_format, True, True),  # an NCHW input: two launches instead of the merged grid
])
def test_single_layer_routes_match_torch(backbone, cin, cout, need_x, layout, dgrad_tiled, wgrad_tiled):
    ops = backbone.ops
    assert ops.conv_igemm_supported(cin, cout, 3)
    assert ops.conv_igemm_supported(cout, cin, 3) == dgrad_tiled and ops.conv_igemm_wgrad_supported(cin, cout, 3) == wgrad_tiled
    m = _layer(backbone, cin, cout, dil=2)
    x = _input(cin, 3, layout).requires_grad_(need_x)
    assert backbone._igemm_route(m, x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    assert type(y.grad_fn).__name__ == "_IgemmConvFnBackward"
    g = _input(cout, 4)
    y.backward(g)
    gx, gw, gb = _reference(x, m.weight, m.bias, y, g, 3, 2, need_x)
    if need_x:
        _close_x(x.grad, gx)
    else:
        assert x.grad is None
    _close_w(m.weight.grad, gw, library=not wgrad_tiled)
    _close_w(m.bias.grad, gb)


@pytest.mark.parametrize("upper", ["3x3 to 384 channels", "1x1 node"])
def test_absorbing_data_gradient_in_a_launch_of_its_own(backbone, upper):
    """a 256 -> 256 layer whose ReLU backward rides in the data gradient of its one consumer, where that consumer's two gradients do
    not share a grid: a 3x3 layer with 384 output channels (weight gradient by the library) and a single 1x1 node (weight gradient
    by its own launch).  The masked gradient the consumer leaves is what retain_grad() shows on the activation between them"""
    ops = backbone.ops
    lower = _layer(backbone, 256, 256)
    x = _input(256, 5)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1 = lower(x)
        link = y1._dsrg_grad_link
        y1.retain_grad()
        if upper == "1x1 node":
            top, k = _layer(backbone, 256, 256, k=1), 1
            (y2,) = backbone._IgemmConvFn.apply(1, [1], True, 0.0, None, 1, [link], None, y1, top.weight, top.bias)
        else:
            top, k = _layer(backbone, 256, 384, chain_input=True), 3
            assert not ops.conv_igemm_wgrad_supported(256, 384, 3) and backbone._igemm_route(top, y1)
            y2 = top(y1)
    g = _input(top.out_channels, 6)
    y2.backward(g)
    gx, gw, gb = _reference(y1, top.weight, top.bias, y2, g, k, 1)
    masked = gx * (y1 > 0)
    _close_x(y1.grad, masked)
    assert bool(((y1.grad != 0) <= (y1 > 0)).all())                      # masked in the store
    _close_w(top.weight.grad, gw, library=k == 3)
    _close_w(top.bias.grad, gb)
    # the lower layer's bias gradient: the column sums of what that store wrote (as test_igemm_dgrad_absorbs_relu_backward_and_bias_
    # gradient defines it; against the float32 `masked` the bf16 roundings of 16 384 stored values add up: 0.25 at 113, bound 0.23)
    _close_w(lower.bias.grad, y1.grad.float().sum((0, 2, 3)))


def test_separate_1x1_launches_match_torch(backbone):
    """two 1x1 layers in one node of which only one input needs a gradient: plain GEMMs for that data gradient, both weight
    gradients in one launch"""
    tops = [_layer(backbone, 256, 256, k=1), _layer(backbone, 256, 256, k=1)]
    with torch.no_grad():
        tops[1].weight.mul_(-1.0)
    xs = [_input(256, 7).requires_grad_(True), _input(256, 8)]
    ys = backbone._IgemmConvFn.apply(1, [1, 1], True, 0.0, None, 2, None, None, *xs, *[m.weight for m in tops], *[m.bias for m in tops])
    gs = [_input(256, 9), _input(256, 10)]
    torch.autograd.backward(ys, gs)
    assert xs[1].grad is None
    for m, x, y, g, need in zip(tops, xs, ys, gs, (True, False)):
        gx, gw, gb = _reference(x, m.weight, m.bias, y, g, 1, 1, need)
        if need:
            _close_x(x.grad, gx)
        _close_w(m.weight.grad, gw)
        _close_w(m.bias.grad, gb)
