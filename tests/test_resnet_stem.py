"""The fused ResNet stem (csrc/resnet_stem.hip: dsrg_pack_resnet_stem_f32, dsrg_resnet_stem_bf16; ops.resnet_stem_pack,
ops.resnet_stem): conv 7x7 / 2 / pad 3 with the frozen BatchNorm folded in -> ReLU -> max pool 3x3 / 2 / pad 1, ceil mode.

Without a GPU: the entry points' argument checks, and `_stem64`, a float64 numpy restatement of the contract in
include/dsrg_hip.h, against torch's CPU float64 conv2d -> + shift -> relu -> max_pool2d(ceil_mode=True).

On the GPU, bit for bit: operands are integers (kernel x scale: multiples of 1/2) so small that every partial sum, in any order,
is a multiple of 1/2 below 2^23 — every float32 accumulation is exact, the float64 restatement IS the accumulator value and the
bf16 output must be its round-to-nearest-even.  No tolerance; a failure names the element.  Three channels of every case have a
zero kernel and shift -40 (whole windows are 0), three more ("phantom" channels) have all-negative pre-activations on the real map
and a POSITIVE shift: a pool window position off the map computed as a convolution over zero padding would give relu(shift) > 0
there, and the expected output is 0."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 7), (1, 8, 9), (2, 15, 16), (1, 17, 33), (3, 23, 38), (1, 65, 63), (1, 97, 131), (2, 129, 129)]
DEAD = (5, 21, 37)            # zero kernel, shift -40
PHANTOM = (9, 30, 58)         # centre tap on input channel 2 (all positive), negative; shift > 0
K_PACKED = 192


# ---- bf16, nearest even, in numpy ------------------------------------------------------------------------------------------
def _bf16_bits(a):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_round(a):
    """float32-representable array -> the float64 values of its bf16 rounding"""
    bits = _bf16_bits(a).astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64)


def _bits_of(t):
    """a bf16 torch tensor (any strides) -> uint16 bit patterns in its logical (B,C,H,W) order"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- the contract, float64 -------------------------------------------------------------------------------------------------
def _pool_size(n):
    from dsrg_amd import ops
    return ops.maxpool3x3_out_size(n, 2, True)


def _stem64(x, wq, shift):
    """x (B,3,H,W), wq (64,3,7,7) = the kernel the launch multiplies with (w * scale, rounded by the caller where the case rounds),
    shift (64), all float64 -> (pre-activation (B,64,OHc,OWc), output (B,64,PH,PW)), before the final rounding"""
    B, _, H, W = x.shape
    OHc, OWc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.pad(x, ((0, 0), (0, 0), (3, 3), (3, 3)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7), axis=(2, 3))[:, :, ::2, ::2][:, :, :OHc, :OWc]     # (B,3,OHc,OWc,7,7)
    pre = np.einsum("bcijyx,ocyx->boij", win, wq, optimize=True) + shift[None, :, None, None]
    act = np.maximum(pre, 0.0) + 0.0
    PH, PW = _pool_size(OHc), _pool_size(OWc)
    # window positions off the OHc x OWc map do not exist: -inf never wins
    pad = np.full((B, 64, 2 * PH + 1, 2 * PW + 1), -np.inf)
    pad[:, :, 1:1 + OHc, 1:1 + OWc] = act[:, :, :2 * PH, :2 * PW]
    out = np.full((B, 64, PH, PW), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, pad[:, :, dy:dy + 2 * PH:2, dx:dx + 2 * PW:2])
    return pre, out


def _exact_case(B, H, W, seed):
    """-> x, w, scale, shift (float64; every value and every w * scale a bf16 number)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (B, 3, H, W)).astype(np.float64)
    x[:, 2] = rng.integers(1, 9, (B, H, W))                               # channel 2 is positive: the phantom channels lean on it
    w = rng.integers(-3, 4, (64, 3, 7, 7)).astype(np.float64)
    scale = rng.choice([0.5, 1.0, 2.0], 64)
    shift = rng.integers(-40, 41, 64).astype(np.float64)
    for o in DEAD:
        w[o], shift[o] = 0.0, -40.0
    for n, o in enumerate(PHANTOM):
        w[o] = 0.0
        w[o, 2, 3, 3], scale[o], shift[o] = -3.0, 2.0, float(1 + 2 * n)   # pre-activation = shift - 6 x <= -1 on the map
    return x, w, scale, shift


def _expected_exact(x, w, scale, shift):
    wq = w * scale[:, None, None, None]
    assert np.array_equal(_bf16_round(wq.astype(np.float32)), wq) and np.array_equal(_bf16_round(x.astype(np.float32)), x)
    # the exactness bound, a condition on the inputs: every partial sum is a multiple of 1/2 below 2^23
    assert (np.abs(wq).sum((1, 2, 3)).max() * np.abs(x).max() + np.abs(shift).max()) * 2 < 2 ** 24
    pre, out = _stem64(x, wq, shift)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    for o in PHANTOM:
        # the phantom-position case occurs: every real pre-activation is negative, the shift is positive, so a position off the
        # map taken as a convolution over zeros (pre-activation = shift) would win its window
        assert pre[:, o].max() < 0 and shift[o] > 0 and out[:, o].max() == 0
    for o in DEAD:
        assert out[:, o].max() == 0
    return pre, out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    from dsrg_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(64)                                              # never dereferenced: the checks come first
    assert L.dsrg_resnet_stem_packed_bytes() == 64 * K_PACKED * 2
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert L.dsrg_pack_resnet_stem_f32(*args, None) == _lib.ERR_INVALID
        assert b"resnet stem pack" in L.dsrg_last_error()
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert L.dsrg_resnet_stem_bf16(*args, 1, 8, 8, None) == _lib.ERR_INVALID
        assert b"NULL" in L.dsrg_last_error()
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8)):
        assert L.dsrg_resnet_stem_bf16(one, one, one, one, B, H, W, None) == _lib.ERR_INVALID
        assert b"resnet stem" in L.dsrg_last_error()
    assert L.dsrg_resnet_stem_bf16(one, one, one, ctypes.c_void_p(72), 1, 8, 8, None) == _lib.ERR_INVALID      # output not 16-byte aligned
    assert b"aligned" in L.dsrg_last_error()


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_restatement_matches_torch_float64(B, H, W):
    x, w, scale, shift = _exact_case(B, H, W, 100 + H * W)
    _, out = _expected_exact(x, w, scale, shift)
    wq = torch.from_numpy(w * scale[:, None, None, None])
    conv = F.conv2d(torch.from_numpy(x), wq, stride=2, padding=3) + torch.from_numpy(shift).view(1, -1, 1, 1)
    ref = F.max_pool2d(F.relu(conv), 3, 2, 1, ceil_mode=True)
    OHc, OWc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(conv.shape[2:]) == (OHc, OWc)
    assert tuple(ref.shape) == (B, 64, _pool_size(OHc), _pool_size(OWc)) == out.shape       # PH / PW are torch's
    assert np.array_equal(ref.numpy(), out)                                                    # integer data: exact in any order


def test_restatement_on_random_data_matches_torch_float64():
    rng = np.random.default_rng(3)
    x, w, shift = rng.standard_normal((2, 3, 21, 18)), rng.standard_normal((64, 3, 7, 7)), rng.standard_normal(64)
    _, out = _stem64(x, w, shift)
    ref = F.max_pool2d(F.relu(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(shift), stride=2, padding=3)), 3, 2, 1,
                       ceil_mode=True).numpy()
    assert out.shape == ref.shape and np.abs(out - ref).max() < 1e-12


def test_exact_cases_round_and_tie():
    """non-vacuity of "rounds once to nearest even": over the cases, a good share of the expected values is not a bf16 number and
    some are exact ties; and some case has pool windows overhanging the map at the bottom / right (ceil mode)"""
    inexact = ties = total = 0
    overhang = False
    for B, H, W in SHAPES[3:6]:
        _, out = _expected_exact(*_exact_case(B, H, W, 100 + H * W))
        live = out[out > 0]
        r = _bf16_round(live.astype(np.float32))
        inexact += int((r != live).sum())
        total += live.size
        ulp = 2.0 ** (np.floor(np.log2(live)) - 7)
        ties += int((np.abs(r - live) == ulp / 2).sum())
        OHc = (H - 1) // 2 + 1
        overhang = overhang or 2 * (_pool_size(OHc) - 1) + 1 > OHc - 1
    assert inexact > 0.1 * total and ties > 0 and overhang, (inexact, ties, total, overhang)


# ---- GPU, exact ------------------------------------------------------------------------------------------------------------
def _name_mismatch(got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        f = lambda b: float((np.uint32(b) << 16).view(np.float32))        # noqa: E731
        pytest.fail("%s: %d of %d elements differ; first at (b, channel, row, column) = %s: got %r (0x%04x), want %r (0x%04x)"
                    % (what, len(bad), got.size, i, f(got[i]), got[i], f(want[i]), want[i]))


def _run(x, w, scale, shift):
    from dsrg_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
    packed = ops.resnet_stem_pack(d(w), d(scale))
    y = ops.resnet_stem(d(x), packed, d(shift))
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    return y


@gpu
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_stem_exact(B, H, W):
    x, w, scale, shift = _exact_case(B, H, W, 100 + H * W)
    _, out = _expected_exact(x, w, scale, shift)
    y = _run(x, w, scale, shift)
    assert tuple(y.shape) == out.shape
    _name_mismatch(_bits_of(y), _bf16_bits(out.astype(np.float32)), "stem %s" % ((B, H, W),))


@gpu
def test_stem_rounds_its_input_to_nearest_even():
    """delta kernels (centre tap 1 on input channel o % 3, scale 1, shift 0): the output is the window maximum of bf16_rne(x) at the
    sampled positions — ties to even, not truncation"""
    rng = np.random.default_rng(11)
    palette = np.array([1 + 2.0 ** -8 + 2.0 ** -12, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -7 - 2.0 ** -20,
                        0.75 + 2.0 ** -9, 3.0 + 2.0 ** -7, -2.5, 0.0], dtype=np.float32)
    x = rng.choice(palette, (2, 3, 29, 35)).astype(np.float32)
    w = np.zeros((64, 3, 7, 7))
    for o in range(64):
        w[o, o % 3, 3, 3] = 1.0
    xr = _bf16_round(x)
    _, out = _stem64(xr, w, np.zeros(64))
    trunc = ((x.view(np.uint32) >> 16) << 16).view(np.float32).astype(np.float64)
    assert (_stem64(trunc, w, np.zeros(64))[1] != out).any()                # truncation would be told apart
    assert np.array_equal(_bf16_round(out.astype(np.float32)), out)         # a maximum of bf16 numbers: nothing left to round
    y = _run(x, w, np.ones(64), np.zeros(64))
    _name_mismatch(_bits_of(y), _bf16_bits(out.astype(np.float32)), "delta kernel")


@gpu
def test_pack_is_one_product_one_rounding():
    from dsrg_amd import ops
    rng = np.random.default_rng(5)
    w = rng.standard_normal((64, 3, 7, 7)).astype(np.float32)
    scale = (rng.standard_normal(64) * 3).astype(np.float32)
    packed = ops.resnet_stem_pack(torch.from_numpy(w).cuda(), torch.from_numpy(scale).cuda())
    assert packed.dtype == torch.bfloat16 and tuple(packed.shape) == (64, K_PACKED)
    bits = packed.cpu().view(torch.int16).numpy().view(np.uint16).reshape(64, 24, 8)       # [o][ky * 3 + c][kx]
    assert not bits[:, 21:].any() and not bits[:, :, 7].any()               # padding groups and the eighth tap are zeros
    got = bits[:, :21, :7].reshape(64, 7, 3, 7).transpose(0, 2, 1, 3)       # -> [o][c][ky][kx]
    want = _bf16_bits(w * scale[:, None, None, None])                       # the float32 product, rounded once
    _name_mismatch(got, want, "packed kernel")
    # a channels_last parameter (what the network holds) packs the same
    wcl = torch.from_numpy(w).cuda().contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.resnet_stem_pack(wcl, torch.from_numpy(scale).cuda()), packed)


# ---- GPU, random data --------------------------------------------------------------------------------------------------------
@gpu
def test_stem_error_no_larger_than_the_module_stem():
    """random normal data at (2, 3, 161, 161): against the float64 restatement on UNROUNDED operands, the RMS error of the fused
    kernel is no larger than that of the module's stem under bf16 autocast — its rounding steps are a strict subset of the module's
    (which also rounds the convolution, the BatchNorm's scale, shift, product and sum), so no margin.
    Measured on an MI355X: see CHANGELOG.md."""
    from dsrg_amd import ops
    from dsrg_amd.retrain import ResNet101DeepLab
    torch.manual_seed(7)
    stem = ResNet101DeepLab(num_classes=21, blocks=(1, 1, 1, 1)).stem
    bn = stem[1]
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0.0, 0.3)
        bn.running_mean.normal_(0.0, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 3, 161, 161)
    scale64 = bn.weight.double() * torch.rsqrt(bn.running_var.double() + 1e-5)
    shift64 = bn.bias.double() - bn.running_mean.double() * scale64
    _, ref = _stem64(x.double().numpy(), (stem[0].weight.double() * scale64.view(-1, 1, 1, 1)).detach().numpy(), shift64.detach().numpy())
    stem = stem.cuda().eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        old = stem(x.cuda())
    scale, shift = bn.frozen_affine()
    new = ops.resnet_stem(x.cuda(), ops.resnet_stem_pack(stem[0].weight.detach(), scale), shift)
    assert tuple(new.shape) == tuple(old.shape) == ref.shape
    rms = lambda t: float(np.sqrt(np.mean((t.double().cpu().numpy() - ref) ** 2)))          # noqa: E731
    e_new, e_old = rms(new), rms(old)
    print("stem RMS error against float64: fused kernel %.6g, module stem under autocast %.6g (RMS of the reference %.6g)"
          % (e_new, e_old, float(np.sqrt(np.mean(ref ** 2)))))
    assert e_new <= e_old, "fused stem RMS error %.6g > module stem %.6g" % (e_new, e_old)
