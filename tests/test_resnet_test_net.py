"""resnet_test.ResNetTestNet: the test-time forward of retrain.ResNet101DeepLab (fused stem, kernels packed once, the strided 1x1
layers on the subsampled map, the stacked ASPP kernel kept) against the module's own forward — bit for bit where the launches are
the same, within the project's bf16 bar (tests/test_gpu_parity.py: |a - b| < 0.05 |b| against the float32 CPU forward) elsewhere.
BatchNorm statistics and affine parameters are randomised as in test_resnet_folded_bn_path_matches_unfused_reference."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _randomised(blocks, seed=0):
    from dsrg_amd import retrain as R
    torch.manual_seed(seed)
    ref = R.ResNet101DeepLab(blocks=blocks)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, R._FrozenBN):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    return ref.eval()


def _nets(blocks=(1, 1, 1, 1)):
    """(float32 CPU reference, its copy on the GPU, the wrapper of that copy) — made once, shared by the tests, never modified"""
    return _nets_once(tuple(blocks))


@functools.lru_cache(maxsize=None)
def _nets_once(blocks):
    from dsrg_amd.resnet_test import ResNetTestNet
    ref = _randomised(blocks)
    net = copy.deepcopy(ref).cuda().to(memory_format=CL).eval()
    return ref, net, ResNetTestNet(net)


def _amp():
    return torch.autocast("cuda", dtype=torch.bfloat16)


def _act(shape, seed):
    """a ReLU output: bf16 channels_last, about half zeros"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).clamp_(min=0).to(torch.bfloat16).cuda().contiguous(memory_format=CL)


@pytest.mark.parametrize("B", [8, 1])
def test_stride1_block_is_the_modules_bit_for_bit(B):
    """(8, 64, 33, 33): 8 712 pixels, the implicit-GEMM route — same launches, same packing function, same bits; (1, 64, 33, 33):
    the library route"""
    from dsrg_amd import retrain as R
    _, net, w = _nets()
    x = _act((B, 64, 33, 33), 1)
    with torch.no_grad(), _amp():
        assert bool(R._igemm_bn_route(x, net.layers[0].c1, net.layers[0].b1)) == (B == 8)
        want = net.layers[0](x)
        got = w.block(0, x)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def test_stride2_block_is_the_stride1_block_on_the_subsampled_map():
    ref, net, w = _nets()
    x = _act((8, 256, 33, 33), 2)                                  # -> 17 x 17 x 8 = 2 312 pixels
    blk = copy.deepcopy(net.layers[1])
    assert blk.c1.stride == (2, 2) and blk.down[0].stride == (2, 2)
    blk.c1.stride = blk.down[0].stride = (1, 1)
    with torch.no_grad(), _amp():
        got = w.block(1, x)
        want = blk(x[:, :, ::2, ::2].contiguous(memory_format=CL))
    assert tuple(got.shape) == (8, 512, 17, 17) and torch.equal(got, want)
    with torch.no_grad():
        strided = ref.layers[1](x.float().cpu())                   # the strided block itself, float32
    err, nrm = float((got.float().cpu() - strided).norm()), float(strided.norm())
    assert err < 0.05 * nrm, (err, nrm)


@pytest.mark.parametrize("B", [8, 1])
def test_head_is_the_modules_bit_for_bit(B):
    """(8, 2048, 17, 17): the one-launch head on the stored stacked kernel; (1, 2048, 17, 17): the plain sum of four convolutions"""
    from dsrg_amd import retrain as R
    _, net, w = _nets()
    head = R.ResNet101DeepLab(blocks=(0, 0, 0, 0))                 # forward = stem -> (no layers) -> the head
    head.stem, head.aspp = nn.Identity(), net.aspp
    head = head.eval()
    f = _act((B, 2048, 17, 17), 3)
    with torch.no_grad(), _amp():
        want = head(f)
        got = w.head(f)
    assert got.dtype == want.dtype and tuple(got.shape) == (B, 21, 17, 17) and torch.equal(got, want)


@pytest.mark.parametrize("blocks,shape", [((1, 1, 1, 1), (8, 3, 129, 129)), ((1, 1, 1, 1), (1, 3, 97, 97)), ((3, 4, 23, 3), (2, 3, 129, 129))])
def test_whole_net_against_float32(blocks, shape):
    """|y - y_ref| < 0.05 |y_ref| (the bar of tests/test_gpu_parity.py), and max |y - y_ref| at most 1.5 x the module's bf16 forward's
    against the same reference: the rounding points are the same except at the stem and two layers, so the two errors are samples
    of one distribution and 1.5 covers the noise of a maximum.  Measured on an MI355X: see CHANGELOG.md."""
    ref, net, w = _nets(blocks)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        yr = ref(x)
        with _amp():
            y_old = net(x.cuda()).float().cpu()
            y_new = w(x.cuda()).float().cpu()
    assert y_new.shape == yr.shape
    rel_new, rel_old = float((y_new - yr).norm() / yr.norm()), float((y_old - yr).norm() / yr.norm())
    max_new, max_old = float((y_new - yr).abs().max()), float((y_old - yr).abs().max())
    msg = "%s %s: relative error wrapper %.5f, module %.5f; max error wrapper %.6g, module %.6g" % (blocks, shape, rel_new, rel_old, max_new, max_old)
    print(msg)
    assert rel_new < 0.05, msg
    assert max_new <= 1.5 * max_old, msg


@pytest.mark.parametrize("shape", [(1, 3, 97, 97), (8, 3, 129, 129)])
def test_graphed_forward_replays_the_eager_bits(shape):
    from dsrg_amd.inference import GraphedForward
    _, _, w = _nets()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    fwd = GraphedForward(w)
    with _amp():
        eager = w(x).contiguous().clone()
        first = fwd(x).clone()                                     # captures
        again = fwd(x).clone()                                     # replays
    assert torch.equal(first, eager) and torch.equal(again, eager)


def test_weights_are_packed_once_until_refresh():
    """one weight changed in place — the stem's, which is packed at every shape (at one image the bottlenecks and the head take the
    library routes, which read the float32 parameters themselves)"""
    from dsrg_amd.inference import GraphedForward
    from dsrg_amd.resnet_test import ResNetTestNet
    net = copy.deepcopy(_nets()[1])
    w = ResNetTestNet(net)
    x = torch.randn((1, 3, 97, 97), generator=torch.Generator().manual_seed(6)).cuda()
    fwd = GraphedForward(w)
    with _amp():
        before = fwd(x).clone()
        with torch.no_grad():
            net.stem[0].weight.mul_(1.25)
        assert torch.equal(fwd(x), before) and torch.equal(w(x).contiguous(), before)       # packed once: not seen
        w.refresh()
        after_eager = w(x).contiguous().clone()
        after = GraphedForward(w)(x).clone()                       # a new capture
    assert not torch.equal(after, before) and torch.equal(after, after_eager)


def test_training_mode_and_trained_affine_raise():
    from dsrg_amd import retrain as R
    from dsrg_amd.resnet_test import ResNetTestNet
    with pytest.raises(ValueError, match="train_bn_affine"):
        ResNetTestNet(R.ResNet101DeepLab(blocks=(1, 1, 1, 1), train_bn_affine=True).cuda().eval())
    with pytest.raises(ValueError, match="eval"):
        ResNetTestNet(R.ResNet101DeepLab(blocks=(1, 1, 1, 1)).cuda().train())
    w = ResNetTestNet(copy.deepcopy(_nets()[1]))
    assert not w.training
    x = torch.zeros(1, 3, 33, 33, device="cuda")
    w.train()
    with _amp(), pytest.raises(RuntimeError, match="eval"):
        w(x)
    w.eval()
    with pytest.raises(RuntimeError, match="autocast"):              # bf16 by contract
        w(x)
    with _amp():
        assert tuple(w(x).shape) == (1, 21, 5, 5)


@pytest.mark.parametrize("smooth", [False, True])
def test_predict_mask_ms_takes_the_wrapper(smooth):
    from dsrg_amd import inference as I
    _, _, w = _nets()
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:60, 0:45]
    img = np.stack([(yy * 4) % 256, (xx * 5) % 256, ((yy + xx) * 3) % 256], -1).astype(np.uint8)
    img = np.clip(img.astype(np.int32) + rng.integers(-10, 11, img.shape), 0, 255).astype(np.uint8)
    with _amp():
        a = I.predict_mask_ms(w, img, smooth=smooth, sizes=(65, 97), device="cuda")
        b = I.predict_mask_ms(w, img, smooth=smooth, sizes=(65, 97), device="cuda")
    assert a.shape == (60, 45) and a.min() >= 0 and a.max() < 21 and np.array_equal(a, b)
