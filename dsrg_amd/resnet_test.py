"""The test-time forward of the DeepLab-v2 ResNet-101 (retrain.ResNet101DeepLab; no counterpart in the reference, whose test
scripts run VGG16 only: training/tools/test-ms.py, test-ms-f.py): the same network with everything that is constant at test time
done once instead of at every forward.

  stem                     one launch (ops.resnet_stem: conv 7x7 / 2 with the frozen BatchNorm folded in, ReLU, ceil-mode max pool)
                           instead of the library convolution and four passes over a 2x larger map
  bottleneck convolutions  the routes of retrain._Bottleneck.forward / _conv_bn, decided per layer by retrain._igemm_bn_route; on the
                           implicit-GEMM route the kernel packed ONCE from w * scale (ops.pack_conv_weight_pair) and the stored shift
  stride-2 1x1 layers      (c1 / down of the first res3 block) a 1x1 / 2 convolution is the 1x1 / 1 convolution of x[:, :, ::2, ::2]:
                           the subsampled map is copied once (torch, plumbing) and both layers run as stride-1 layers on it
  ASPP head                the stacked 36-tap kernel packed once, the biases summed once
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import retrain as _R
from .backbone import _bf16_run
from .retrain import ResNet101DeepLab, _aspp_bias_sum, _aspp_stacked_kernel, _conv_bn, _igemm_bn_route


class _Layer(object):
    """one convolution + frozen BatchNorm of a bottleneck at test time: `conv` is the module itself, or for a strided 1x1 layer a
    shallow copy with stride 1 (it shares the weight) that sees the subsampled map; pack / shift: the implicit-GEMM route's operands"""
    __slots__ = ("conv", "bn", "pack", "shift")

    def __init__(self, conv, bn):
        self.bn = bn
        if conv.stride != (1, 1):
            if conv.kernel_size != (1, 1) or conv.padding != (0, 0):
                raise ValueError("ResNetTestNet: only 1x1 convolutions may be strided")
            # A shallow copy of the module with stride 1, so that _igemm_bn_route and _conv_bn — which read .stride, .weight,
            # .dilation, ... and call the module — treat the layer as they treat every stride-1 layer.  copy.copy shares the
            # module's `_parameters` dict (not just the tensor), so `.to()`, `load_state_dict` and in-place updates of the
            # original are seen here; the copy is not registered anywhere and owns nothing.
            strided, conv = conv, copy.copy(conv)
            conv.stride = (1, 1)
            if conv._parameters is not strided._parameters or strided.stride == (1, 1):
                raise RuntimeError("ResNetTestNet: the stride-1 view of a strided layer must alias its parameters")
        self.conv = conv
        self.pack = self.shift = None

    def refresh(self):
        from .ops import pack_conv_weight_pair
        scale, shift = self.bn.frozen_affine()
        self.shift = shift
        self.pack = pack_conv_weight_pair(self.conv.weight.detach(), True, False, scale)[0]     # what _FoldedIgemmFn.forward packs

    def __call__(self, x, relu, res=None):
        from .ops import conv_igemm, conv_igemm_residual
        conv = self.conv
        if x.is_cuda and _bf16_run(x) and _igemm_bn_route(x, conv, self.bn):
            x = x if x.dtype == torch.bfloat16 else x.bfloat16()
            k, dil = conv.kernel_size[0], conv.dilation[0]
            if res is not None:
                return conv_igemm_residual(x, self.pack, self.shift, res, None, dil, k, relu)
            return conv_igemm([x], [self.pack], [self.shift], [dil], k, relu)[0]
        if res is not None:
            raise RuntimeError("ResNetTestNet: a shortcut in the store needs the implicit-GEMM route")
        return _conv_bn(x, conv, self.bn, relu)          # the library routes as they are (small maps, one image)


class ResNetTestNet(nn.Module):
    """An eval-mode retrain.ResNet101DeepLab (train_bn_affine=False) called like it — (B,3,S,S') float32 -> (B,C,h,w) float32 scores
    under bf16 autocast — for inference._eval_mode, inference.GraphedForward and every predict_* function, as `net` or `forward`.

    Unlike the module's own forward (and unlike what the docstring of inference.GraphedForward says of a captured graph), this
    class does NOT re-read the float32 parameters at every call: the stem kernel, every bottleneck kernel (w * BatchNorm scale) and
    the stacked ASPP kernel are packed ONCE, at construction.  After changing the weights or BatchNorm statistics in place (or
    loading a checkpoint into `net`), call refresh() — and capture new graphs: a GraphedForward made before holds the old buffers.
    (Layers that take the library routes at a given input size — small maps, one image — still read the float32 parameters
    themselves, so without refresh() a changed network would run partly on old and partly on new weights.)

    The forward runs under no_grad and builds no autograd node.  Its arithmetic is the module's bf16 forward's except at the stem
    (inputs and folded kernel rounded once each to bf16, float32 sums, ONE rounding at the pooled store — the module rounds the
    convolution, the BatchNorm's scale, shift and result as well) and at the two strided 1x1 layers (implicit-GEMM or im2col route on
    the subsampled map instead of the library's strided convolution).  It needs bf16 activations: call it under
    torch.autocast("cuda", dtype=torch.bfloat16); for a float32 forward use the module itself."""

    def __init__(self, net):
        super().__init__()
        if not isinstance(net, ResNet101DeepLab):
            raise TypeError("ResNetTestNet wraps a retrain.ResNet101DeepLab")
        if any(p.requires_grad for m in net.modules() if isinstance(m, _R._FrozenBN) for p in (m.weight, m.bias)):
            raise ValueError("ResNetTestNet needs constant BatchNorm maps (ResNet101DeepLab(train_bn_affine=False))")
        if net.training:
            raise ValueError("ResNetTestNet wraps an eval-mode network (net.eval())")
        self.net = net
        self.training = False                             # born in the mode of the network it wraps
        self._blocks = []
        for blk in net.layers:
            self._blocks.append((blk, _Layer(blk.c1, blk.b1), _Layer(blk.c2, blk.b2), _Layer(blk.c3, blk.b3),
                                 _Layer(blk.down[0], blk.down[1]) if blk.down is not None else None))
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        """pack everything again from the current parameters and BatchNorm statistics of `net`"""
        from .ops import pack_conv_weight_pair, resnet_stem_pack
        net = self.net
        conv, bn = net.stem[0], net.stem[1]
        if not conv.weight.is_cuda:
            raise ValueError("ResNetTestNet needs the network on the GPU")
        scale, shift = bn.frozen_affine()
        self._stem_pack, self._stem_shift = resnet_stem_pack(conv.weight.detach().float(), scale), shift
        for _, *layers in self._blocks:
            for layer in layers:
                if layer is not None:
                    layer.refresh()
        self._head_dils = tuple(m.dilation[0] for m in net.aspp)
        self._head_offsets = self._head_pack = self._head_bias = None
        if self._head_stackable():
            self._head_offsets, wcat, _ = _aspp_stacked_kernel(self._head_dils, [m.weight for m in net.aspp])
            self._head_pack = pack_conv_weight_pair(wcat, True, False)[0]                 # what _AsppFn.forward packs
            self._head_bias = _aspp_bias_sum([m.bias for m in net.aspp])
        return self

    def _head_stackable(self):
        """the part of ResNet101DeepLab.forward's condition for the one-launch head that depends on the modules alone"""
        from .ops import conv_igemm_supported
        aspp = self.net.aspp
        cin = aspp[0].in_channels
        return (len(aspp) <= 4 and 9 * len(aspp) * aspp[0].out_channels <= 2048 and conv_igemm_supported(cin, 128, 1) and cin % 256 == 0 and
                all(m.kernel_size == (3, 3) and m.padding == m.dilation and m.stride == (1, 1) for m in aspp))

    def stem(self, x):
        from .ops import resnet_stem
        x = x if x.dtype == torch.float32 else x.float()
        return resnet_stem(x.contiguous(), self._stem_pack, self._stem_shift)

    def block(self, i, x):
        """bottleneck i: the decisions of retrain._Bottleneck.forward without its autograd side channels"""
        from .ops import add_relu
        blk, c1, c2, c3, down = self._blocks[i]
        cl = torch.channels_last
        bf16 = x.is_cuda and _bf16_run(x)
        xs = x
        if blk.c1.stride != (1, 1):                       # both strided layers read the same subsampled map
            if down is None or blk.down[0].stride != blk.c1.stride:
                raise RuntimeError("ResNetTestNet: a strided block needs a projection shortcut of the same stride")
            sy, sx = blk.c1.stride
            xs = x[:, :, ::sy, ::sx].contiguous(memory_format=cl)
        y2 = c2(c1(xs, True), True)
        idn = down(xs, False) if down is not None else x
        if _R._FUSE_RES and bf16 and blk.c3.stride == (1, 1) and y2.is_cuda and _igemm_bn_route(y2, c3.conv, c3.bn) and \
                y2.dtype == torch.bfloat16 and idn.dtype == torch.bfloat16 and idn.is_contiguous(memory_format=cl) and \
                tuple(idn.shape) == (y2.shape[0], blk.c3.out_channels, y2.shape[2], y2.shape[3]):
            return c3(y2, True, idn)                      # the shortcut and the ReLU in the last launch's store
        y = c3(y2, False)
        if y.is_cuda and y.dtype == torch.bfloat16 and idn.dtype == torch.bfloat16 and y.numel() % 8 == 0:
            return add_relu(y, idn)                       # _AddReLUFn's pass
        return F.relu(y + idn)

    def head(self, f):
        """the ASPP head: ResNet101DeepLab.forward's, the one-launch form on the stored stacked kernel"""
        from .ops import aspp_shift_sum, conv_igemm
        aspp = self.net.aspp
        if self._head_pack is not None and f.is_cuda and _bf16_run(f) and f.shape[0] * f.shape[2] * f.shape[3] >= 2048:
            f = f if f.dtype == torch.bfloat16 else f.bfloat16()
            f = f if f.is_contiguous(memory_format=torch.channels_last) else f.contiguous(memory_format=torch.channels_last)
            (yp,) = conv_igemm([f], [self._head_pack], None, [1], 1, False)
            return aspp_shift_sum(yp, self._head_offsets, aspp[0].out_channels, self._head_bias)
        out = aspp[0](f)
        for m in aspp[1:]:
            out = out + m(f)
        return out

    @torch.no_grad()
    def forward(self, x):
        if self.training or self.net.training:
            raise RuntimeError("ResNetTestNet is a test-time forward: call eval() first")
        if not (x.is_cuda and _bf16_run(x)):
            raise RuntimeError("ResNetTestNet runs in bf16 on the GPU: call it under torch.autocast('cuda', dtype=torch.bfloat16) "
                               "(float32: the module's own forward)")
        f = self.stem(x)
        for i in range(len(self._blocks)):
            f = self.block(i, f)
        return self.head(f)
