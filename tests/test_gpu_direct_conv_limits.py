"""The size limit of the direct 3x3 convolutions with 64 / 128 channels (csrc/conv_direct.hip): a map whose
B * H * W * max(cin, cout) * 2 bytes reach 2^31 is refused with DSRG_ERR_UNSUPPORTED before anything is launched — forward
and masked alike, for all four channel pairs — and the 3 -> 64 kernel, which addresses with 64 bits, is not subject to it.

No kernel runs on the refused shapes, so the pointers are those of tiny dummy tensors.  The shape is exactly 2^31 bytes on
the wider side: B = 1, H = 4096, W = 2^31 / (4096 * max(cin, cout) * 2).  3 -> 64 cannot be asked for that shape (it would
launch on the dummies); it is asked for one with more than 2^31 tiles, which it refuses as a bad shape while 64 -> 64 at
the same shape meets the size limit first."""
import pytest
import torch

gpu = pytest.mark.gpu
PAIRS = [(64, 64), (64, 128), (128, 128), (128, 64)]
LIMIT = "2^31"                                            # what the message names


@pytest.fixture(scope="module")
def L():
    from dsrg_amd import _lib
    _lib.require_gpu()
    return _lib.lib()


@pytest.fixture(scope="module")
def dummy():
    return torch.zeros(64, dtype=torch.float32, device="cuda")


def _at_limit(cin, cout):
    W = 2 ** 31 // (4096 * max(cin, cout) * 2)
    assert 4096 * W * max(cin, cout) * 2 == 2 ** 31
    return 1, 4096, W


def _forward(L, p, B, H, W, cin, cout):
    return L.dsrg_conv3x3_direct_bf16(p, p, None, p, B, H, W, cin, cout, 1, None)


def _masked(L, p, B, H, W, cin, cout):
    return L.dsrg_conv3x3_direct_dgrad_bf16(p, p, p, p, p, p, 256, B, H, W, cin, cout, None)


def _small_launch_works(cin, cout):
    from dsrg_amd import ops
    x = torch.ones(1, cin, 1, 1, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    w = torch.ones(cout, cin, 3, 3, device="cuda").bfloat16()
    y = ops.conv3x3_direct(x, w)
    torch.cuda.synchronize()
    assert torch.equal(y.float().flatten(), torch.full((cout,), float(cin), device="cuda"))   # the centre tap alone meets the map


@gpu
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("form", [_forward, _masked], ids=["forward", "masked"])
def test_map_of_2_gib_is_refused(L, dummy, form, cin, cout):
    from dsrg_amd import _lib
    B, H, W = _at_limit(cin, cout)
    assert form(L, dummy.data_ptr(), B, H, W, cin, cout) == _lib.ERR_UNSUPPORTED
    msg = L.dsrg_last_error().decode()
    assert LIMIT in msg and "conv3x3_direct" in msg, msg
    _small_launch_works(cin, cout)


@gpu
def test_one_pixel_column_less_is_not_refused_for_its_size(L, dummy):
    """just below the limit the size check passes: the masked form gets as far as its scratch check (256 bytes: too small), which
    comes behind it and launches nothing either"""
    from dsrg_amd import _lib
    B, H, W = _at_limit(128, 128)
    assert _masked(L, dummy.data_ptr(), B, H, W - 1, 128, 128) == _lib.ERR_INVALID
    assert LIMIT not in L.dsrg_last_error().decode()


@gpu
def test_first_layer_is_not_subject_to_the_limit(L, dummy):
    from dsrg_amd import _lib
    B = H = W = 65536                                      # 2^41 tiles: no launch can take it
    assert _forward(L, dummy.data_ptr(), B, H, W, 64, 64) == _lib.ERR_UNSUPPORTED
    assert LIMIT in L.dsrg_last_error().decode()
    assert _forward(L, dummy.data_ptr(), B, H, W, 3, 64) == _lib.ERR_INVALID
    msg = L.dsrg_last_error().decode()
    assert LIMIT not in msg and "bad shape" in msg, msg
    _small_launch_works(3, 64)
