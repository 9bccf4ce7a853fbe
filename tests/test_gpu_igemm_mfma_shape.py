"""The 16x16x32 fragment mapping of csrc/conv_igemm.hip's forward / data-gradient body on the launch forms that
test_gpu_exact_conv.py leaves out: the unstaggered issue path (debug variant 1) and the retired variant numbers.

Exact integer data, as there (its generators, references and comparisons are imported): every fp32 sum is exact whatever the
order, so a float64 convolution of the same operands, rounded once to bf16, is the expected output bit for bit, and a wrong
lane -> element mapping names the element instead of drifting inside a tolerance."""
import pytest
import torch

from test_gpu_exact_conv import (_bounded, _dev, _dgrad64, _fwd_case, _gen, _ints, _masked, _nonvacuous, _post, _relu_out, _rounded,
                                 _same, _variant, ops)  # noqa: F401  (ops: the module fixture)

gpu = pytest.mark.gpu

SHAPES = [                                                # (B, H, W, cin, cout, k, dil)
    (1, 16, 16, 64, 256, 1, 1),                           # exactly one full tile and one K-step: both 32-deep slices, all 8 x 4 blocks of every wave
    (2, 19, 23, 128, 256, 3, 2),                          # ragged last tile, two chunks
    (2, 27, 31, 256, 128, 3, 1),                          # half an n-tile: the upper waves idle
    (1, 4, 4, 64, 64, 3, 1),                              # a 64-output launch
]


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil", SHAPES)
def test_unstaggered_forward_is_the_rounded_float64_convolution(ops, B, H, W, cin, cout, k, dil):
    x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, k, dil, 11)
    xd, pk, bd = _dev(x), ops.pack_conv_weight(_dev(w)), _dev(b, torch.float32)
    with _variant(ops, 1):
        for bias in (False, True):
            for relu in (False, True):
                (got,) = ops.conv_igemm([xd], [pk], [bd if bias else None], [dil], k, relu, stream_k=False)
                what = "variant 1 bias %d relu %d" % (bias, relu)
                _same(got, _rounded(_post(ref, b if bias else None, relu), True, what, relu), what)


@gpu
def test_unstaggered_masked_data_gradient_with_column_sums(ops):
    B, H, W, cf, cb, k, dils, scale = 1, 20, 23, 512, 256, 3, [1, 3], 2.0
    n = len(dils)
    gen = _gen(78)
    gs = [_ints((B, cf, H, W), -8, 8, gen) for _ in range(n)]
    ws = [_ints((cf, cb, k, k), -4, 4, gen) for _ in range(n)]
    ys = [_relu_out((B, cb, H, W), 8, gen) for _ in range(n)]
    refs = [_dgrad64(gs[i], ws[i], dils[i], (H, W)) for i in range(n)]
    for i in range(n):
        _bounded(scale * _dgrad64(gs[i].abs(), ws[i].abs(), dils[i], (H, W)).max())
        _nonvacuous((scale * refs[i])[ys[i] > 0], "masked data gradient")
    packs = [ops.pack_conv_weight(_dev(w), for_dgrad=True) for w in ws]
    with _variant(ops, 1):
        got, gb = ops.conv_igemm_dgrad([_dev(g) for g in gs], packs, [_dev(y) for y in ys], dils, k, scale)
    for i in range(n):
        stored, sums = _masked(refs[i], ys[i], scale)
        _same(got[i], stored, "gx, branch %d" % i)
        _same(gb[i], sums, "bias gradient, branch %d" % i)


@gpu
@pytest.mark.parametrize("variant", [2, 5])
def test_retired_variants_run_the_default(ops, variant):
    B, H, W, cin, cout, k, dil = SHAPES[0]
    x, w, b, _, _ = _fwd_case(B, H, W, cin, cout, k, dil, 12)
    xd, pk, bd = _dev(x), ops.pack_conv_weight(_dev(w)), _dev(b, torch.float32)
    (want,) = ops.conv_igemm([xd], [pk], [bd], [dil], k, True, stream_k=False)
    with _variant(ops, variant):
        (got,) = ops.conv_igemm([xd], [pk], [bd], [dil], k, True, stream_k=False)
    assert torch.equal(got, want), "variant %d: %d elements differ from the default's" % (variant, int((got != want).sum()))
