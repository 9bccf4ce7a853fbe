"""VGG16 DeepLab-v2 ASPP backbone of training/experiment/seed_mc/train-s.prototxt:41-744.

Layer shapes follow the prototxt exactly: 3x3/2 ceil-mode max pools with pad 1
(321 -> 161 -> 81 -> 41), pool4/pool5 stride 1, conv5_x dilation 2, AVE pool5a,
four branches fc6_k (3x3, dilation 6/12/18/24) -> fc7_k (1x1) -> fc8-SEC_k (1x1, 21
outputs, N(0, 0.01) init), summed (Eltwise SUM, train-s.prototxt:737-744).

On the default step (bf16 autocast, float32 channels_last master parameters, a training batch) every layer runs on this
package's HIP kernels, one autograd node per layer or group of layers:
  conv1_1 .. conv2_2             _DirectConvFn   direct MFMA kernels (csrc/conv_direct.hip), pool1 / pool2 inside the node
  conv3_1 .. conv5_3             _IgemmConvFn    implicit-GEMM kernels (csrc/conv_igemm.hip), n = 1, pool3 inside conv3_3's node
  fc6_1..4, then fc7_1..4        _IgemmConvFn    n = 4: the four branches of a level share every launch
  fc8-SEC_1..4 + Eltwise SUM     _HeadsPtrFn     (_HeadsFn where the parameters are not float32 channels_last)
  pool4, pool5, pool5a           _MaxPool3x3Fn, _AvgPool3x3Fn
Everything else — float32, small launches, other parameter layouts, the reference of the route comparisons — is _ConvFn's
(see its docstring): im2col + hipBLASLt GEMM or MIOpen.  Adjacent conv nodes hand the ReLU backward and the bias gradient of
the lower one to the upper one's data gradient through a _GradLink.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import os as _os

from . import ops
from .streams import capture_stream

# Which kernels a convolution runs is decided from what the call observes (device, dtype, layout, shape), by measured thresholds.
# _ConvFn: fewest output channels for the GEMM weight gradient g^T @ im2col(x) (round 2 A/B: 939.9 images/s with 512, 932.8 with 1024)
_WGRAD_MIN_COUT = 512
# _ConvFn: largest map (pixels) whose 3x3 data gradient is im2col(g) + GEMM, the 41x41 stages (round 2: at 81x81 1 221 against 1 233)
_GEMM_DGRAD_MAX_MAP = 2048
# _ConvFn: largest map (pixels) whose 3x3 weight gradient is a GEMM over the kept im2col(x) (round 1: 883 -> 902 images/s)
_GEMM_WGRAD_MAX_MAP = 2048
# fewest 256 x 256 output tiles for which a layer takes the implicit-GEMM kernels: one image at 41x41 is 14 tiles of 72 K-steps for
# 256 CUs, where the library GEMM's small-M kernels win (batch-1 inference 740 against 970 images/s; see _igemm_route)
_IGEMM_MIN_TILES = 64
# The two switches left are the references of comparisons (tests/test_gpu_igemm.py, tools/igemm_route_diag.py assign them between
# two runs): module globals read at call time, never captured at import or construction.
# 3x3 layers with >= 256 output channels (conv3_x .. fc6_k) through the implicit-GEMM kernels; "0": the im2col + hipBLASLt route of
# rounds 1-3 (_ConvFn)
_IGEMM = _os.environ.get("DSRG_IGEMM", "1") == "1"
# adjacent conv nodes fold the lower one's ReLU (+ Dropout) backward and bias gradient into the upper one's data gradient
# (_GradLink); "0": one ordinary autograd node per layer
_FUSE_CHAIN = _os.environ.get("DSRG_FUSE_CHAIN", "1") != "0"
# (measured and dropped in round 5, CHANGELOG.md: the wide layers' packs on a second stream under conv1_x / conv2_x, 1 822 -> 1 798
# images/s; an implicit-GEMM layer's weight gradient on a second stream beside its data gradient, 1 761 -> 1 715)


def _bf16_run(x):
    """do the convolution kernels see x in bf16: it is bf16 already, or autocast to bf16 will cast it"""
    return x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def _im2col_gemm(x, weight, bias, dilation, relu, want_cols=False):
    """(B,C,H,W) bf16 -> conv(+ReLU) output as a channels_last tensor: NHWC im2col (HIP) + one hipBLASLt GEMM whose
    epilogue adds the bias (and applies the ReLU)."""
    B, C, H, W = x.shape
    cout, k = weight.shape[0], weight.shape[2]
    xn = x.permute(0, 2, 3, 1)                                       # free for channels_last tensors
    if not xn.is_contiguous():
        xn = xn.contiguous()
    if k == 1:
        a = xn.reshape(-1, C)
    elif (C * x.element_size()) % 16 == 0 and x.element_size() in (2, 4):
        a = ops.im2col3x3_nhwc(xn, dilation)                          # one bandwidth-bound HIP kernel (16-byte channel groups)
    else:
        p = dilation
        xp = F.pad(xn, (0, 0, p, p, p, p))
        a = torch.cat([xp[:, dy * p:dy * p + H, dx * p:dx * p + W, :] for dy in range(3) for dx in range(3)],
                      dim=-1).reshape(-1, 9 * C)
    wmat = weight.permute(2, 3, 1, 0).reshape(k * k * C, cout)
    # write straight into a channels_last (B,cout,H,W) tensor: its NHWC memory is the GEMM's C matrix
    out = torch.empty((B, cout, H, W), dtype=a.dtype, device=a.device, memory_format=torch.channels_last)
    o2 = out.permute(0, 2, 3, 1).view(-1, cout)
    if bias is None:
        torch.mm(a, wmat, out=o2)
    elif relu:
        torch._addmm_activation(bias, a, wmat, out=o2)
    else:
        torch.addmm(bias, a, wmat, out=o2)
    return (out, a) if want_cols else out


class _GradLink:
    """side channel between two adjacent nodes of a conv chain: when the upper node's data gradient was taken with the lower
    node's ReLU (+ Dropout) backward folded into its store (ops.conv_igemm_dgrad), it leaves that here — with the lower node's
    bias gradient where the store summed one — and the lower node's backward takes the incoming gradient as already masked.
    Only wired where the model declares the lower node's output to have this one consumer (GemmConv2d(chain_input=True);
    VGG16ASPP's fc6 -> fc7; retrain.py's bottlenecks)."""
    __slots__ = ("scale", "gb", "ptr", "version")

    def __init__(self):
        self.arm(1.0)

    def arm(self, scale):
        """lower node's forward: its Dropout scale (1.0 without Dropout), which the upper node's store applies with the mask;
        whatever an earlier step left is discarded"""
        self.scale, self.gb, self.ptr, self.version = scale, None, None, -1

    def leave(self, gx, gb=None):
        """upper node: gx is the masked (and scaled) data gradient it returns for the lower node's output, gb that node's bias
        gradient (None: the lower node has none, retrain.py's folded convolutions)"""
        self.gb, self.ptr, self.version = gb, gx.data_ptr(), gx._version

    def take(self, g):
        """lower node -> (accepted, bias gradient): accepted iff g is exactly the tensor the upper node left (autograd hands a lone
        gradient through untouched; had the output a second consumer after all, the sum would be another tensor or a later
        version of this one).  Declined: the caller runs its own ReLU backward, which is still right on a masked gradient unless
        a Dropout scale was applied with it.  Either way nothing stays left"""
        gb, ptr, self.gb, self.ptr = self.gb, self.ptr, None, None
        if ptr is None:
            return False, None
        if g.data_ptr() == ptr and g._version == self.version:
            return True, gb
        if self.scale != 1.0:
            raise RuntimeError("chain_input: the output of a conv + ReLU + Dropout node declared to have one consumer has several")
        return False, None


def _forward_tail(ctx, outs, relu, pool, links_out, scale):
    """the end of a conv node's forward, outs its n convolution outputs (+ bias (+ ReLU (+ Dropout))) -> (what the node returns, the
    outputs it saves for backward, the pool's window codes or None).  pool = (stride, ceil_mode): conv + ReLU + 3x3 max pool as
    one node (n = 1: conv1_2, conv2_2, conv3_3) — the pool's backward then masks with this ReLU and sums the bias gradient in the
    same pass (ops.maxpool3x3_bwd_relu); the window codes carry the ReLU's mask (relu_input), so the backward never reads the
    full-resolution output and the node does not keep it.  links_out: this node's _GradLinks (or None), armed where a consumer
    can mask for it — behind a ReLU without a pool.  Leaves out_shape, relu, pool, scale and links_out on ctx for _backward_head"""
    code, kept = None, outs if (relu and pool is None) else ()
    if pool is not None:
        pooled, code = ops.maxpool3x3_fwd(outs[0], pool[0], pool[1], relu_input=True)
    ctx.out_shape, ctx.relu, ctx.pool, ctx.scale = tuple(outs[0].shape), relu, pool, scale
    ctx.links_out = links_out if (relu and pool is None) else None
    for lk in ctx.links_out or ():
        lk.arm(scale)
    return (tuple(outs) if pool is None else (pooled,)), kept, code


def _backward_head(ctx, g, y, code, i=0, fallback=True):
    """the start of a conv node's backward for its i-th output, g the incoming bf16 gradient -> (gradient of the pre-activation,
    channels_last; bias gradient): g itself when the consumer left it masked in the link, the bias gradient beside it; else one
    fused HIP pass of this node's own — or None where the caller says those passes do not take g (fallback=False)"""
    if ctx.links_out is not None:
        accepted, gb = ctx.links_out[i].take(g)
        if accepted:
            return g, gb
    if not fallback:
        return None
    if ctx.pool is not None:     # the pool's backward masks with the ReLU the window codes carry
        return ops.maxpool3x3_bwd_relu(g, code, ctx.out_shape, ctx.pool[0])
    if ctx.relu:                 # mask by the sign of the output y, times the Dropout scale
        return ops.relu_bwd_bias(g, y, ctx.scale)
    g = g.contiguous(memory_format=torch.channels_last)      # (e.g. the 21-channel fc8 outputs): the column sums alone
    return g, ops.bias_grad(g)


def _landed(g, slot):
    """the gradient a backward returns for a parameter: when the kernel wrote it into the reducer's slot, a FRESH alias of the slot
    (autograd adopts a gradient as `.grad` without a copy only if nobody else holds the tensor object)"""
    return g.detach() if (slot is not None and g is slot) else g


class _ConvFn(torch.autograd.Function):
    """3x3 / 1x1 stride-1 'same' convolution (+ ReLU (+ Dropout) (+ the stride-2 max pool)) on bf16 or float32 COPIES of the
    parameters (autocast's casts).  What is left to this node since _DirectConvFn and _IgemmConvFn took the default bf16 step:
      * the float32 leg (no autocast) of every layer;
      * launches below _IGEMM_MIN_TILES output tiles (batch-1 test-time forwards, small crops);
      * 1x1 layers outside VGG16ASPP's grouped route (fc7_k then, the fc8 classifiers outside the heads kernels);
      * parameters that are not float32 channels_last masters (a model never converted, or cast to bf16);
      * retrain.py's convolutions with trained BatchNorm affine maps or shapes the folded implicit-GEMM node does not take;
      * the DSRG_IGEMM=0 reference of the route comparisons (tests/test_gpu_igemm.py, tools/igemm_route_diag.py).
    Forward: the direct MFMA kernel for bf16 64 / 128-channel 3x3 layers, else NHWC im2col + one hipBLASLt GEMM when `gemm`
    (tools/conv_probe.py: 300-1200 TFLOP/s at the 41x41 stages against MIOpen's ~180), MIOpen otherwise.  Backward: ReLU mask,
    Dropout mask and scale and the bias gradient in one fused HIP pass (ops.relu_bwd_bias: the output of ReLU + Dropout is
    positive exactly where both masks pass); data and weight gradients by hipBLASLt GEMMs where that beats MIOpen/CK (the 41x41
    stages, see the comments in backward) and by MIOpen/CK otherwise."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x, weight, bias, dilation, relu, gemm, drop_p, pool=None, link_in=None, link_out=None):
        k = weight.shape[2]
        cols = None
        # 64 / 128 channels on both sides (conv1_2 at full resolution, conv2_1 / conv2_2 at half): the direct MFMA kernel
        # (weights in registers, bias + ReLU in the epilogue; csrc/conv_direct.hip) — MIOpen's implicit GEMM runs conv1_2 at
        # ~255 TFLOP/s, the im2col route would move 1.9 GB there and 0.96 GB for conv2_2; conv1_1 (3 -> 64) with bias + ReLU in one pass
        shape = tuple(weight.shape[:2])
        direct = k == 3 and dilation == 1 and x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and (
            (shape[0] in (64, 128) and shape[1] in (64, 128)) or shape == (64, 3))
        if direct:
            out = ops.conv3x3_direct(x, weight, bias, relu)
        elif gemm:
            # the im2col matrix is kept for the layers whose weight gradient is a GEMM too (see backward)
            keep = k == 3 and weight.shape[0] >= _WGRAD_MIN_COUT and x.shape[1] % 8 == 0 and x.shape[2] * x.shape[3] <= _GEMM_WGRAD_MAX_MAP
            out = _im2col_gemm(x, weight, bias, dilation, relu, want_cols=keep)
            if keep:
                out, cols = out
        else:
            out = F.conv2d(x.contiguous(memory_format=torch.channels_last), weight, bias, 1, dilation * (k // 2), dilation)
            if relu:
                out.relu_()
        if drop_p > 0.0:
            out = torch.ops.aten.native_dropout(out, drop_p, True)[0]    # out = relu * mask / (1 - p)
        # link_in — x is the ReLU output of the node in front and feeds nothing else; link_out — ours, without Dropout only (the
        # Dropout mask of this node is torch's: a consumer's store could not apply it)
        (ret,), kept, code = _forward_tail(ctx, [out], relu, pool, [link_out] if (link_out is not None and drop_p == 0.0) else None,
                                           1.0 / (1.0 - drop_p))
        ctx.save_for_backward(x, weight, cols, code, *kept)
        ctx.dilation, ctx.k, ctx.gemm, ctx.direct = dilation, k, gemm, direct
        ctx.link_in = link_in if (direct and link_in is not None and link_in.scale == 1.0 and x.shape[1] in (64, 128) and
                                  x.is_contiguous(memory_format=torch.channels_last)) else None
        return ret

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, weight, cols, code, *y = ctx.saved_tensors
        y = y[0] if y else None                        # the output: kept for a ReLU without a pool only
        pad = ctx.dilation * (ctx.k // 2)
        cout = weight.shape[0]
        # the fused passes take g: always behind a pool (forward guaranteed bf16, ReLU, no dropout, cout | 2048); a link's masked g
        # needs none
        head = _backward_head(ctx, g, y, code, 0, ctx.pool is not None or (
            g.dtype == torch.bfloat16 and ((cout % 8 == 0 and cout <= 2048) or (not ctx.relu and cout <= 256))))
        fused = head is not None
        if fused:
            g, gb = head
        else:
            if ctx.relu:
                g = g * (y > 0) * ctx.scale
            g = g.contiguous(memory_format=torch.channels_last)
        # data gradient of a 3x3 'same' convolution = the forward convolution of g with the flipped, transposed kernel:
        # the im2col + hipBLASLt route again (~1.2 PFLOP/s at the 41x41 stages against 550-630 TFLOP/s for CK's dgrad)
        gemm_dgrad = ctx.gemm and ctx.k == 3 and ctx.needs_input_grad[0] and g.dtype in (torch.bfloat16, torch.float32) \
            and cout % 8 == 0 and x.shape[2] * x.shape[3] <= _GEMM_DGRAD_MAX_MAP
        gx = None
        gemm_1x1 = ctx.gemm and ctx.k == 1 and g.dtype in (torch.bfloat16, torch.float32) and cout % 8 == 0 \
            and x.shape[1] % 8 == 0 and g.dtype == x.dtype
        if gemm_1x1:
            # fc7 (1024 -> 1024, 1x1): both gradients are plain GEMMs over the NHWC matrices (MIOpen's wrw 120 us and CK's dgrad
            # 98 us per branch at 56 GFLOP each)
            cin = x.shape[1]
            g2d = g.permute(0, 2, 3, 1).reshape(-1, cout)
            if ctx.needs_input_grad[0]:
                gx = torch.mm(g2d, weight.reshape(cout, cin)).view(x.shape[0], x.shape[2], x.shape[3], cin).permute(0, 3, 1, 2)
            gemm_dgrad = True
        elif ctx.direct and ctx.needs_input_grad[0] and g.dtype == torch.bfloat16 and x.shape[1] in (64, 128):
            # the data gradient is the same convolution with the kernel flipped and its channel axes swapped
            if _FUSE_CHAIN and ctx.link_in is not None:
                gx, gb_below = ops.conv3x3_direct_dgrad(g, weight.flip(2, 3).transpose(0, 1), x)
                ctx.link_in.leave(gx, gb_below)
            else:
                gx = ops.conv3x3_direct(g, weight.flip(2, 3).transpose(0, 1), None, False)
            gemm_dgrad = True
        elif gemm_dgrad and cout > x.shape[1] and x.shape[1] % 8 == 0 and g.dtype == torch.bfloat16:
            # more output than input channels (fc6: 1024 vs 512): g @ W^T first, then gather the nine taps (col2im) —
            # half the traffic of an im2col of the wide g
            B_, cin, H_, W_ = x.shape
            wmat = weight.permute(2, 3, 1, 0).reshape(9 * cin, cout)
            gx = ops.col2im3x3_nhwc(torch.mm(g.permute(0, 2, 3, 1).reshape(-1, cout), wmat.t()), B_, H_, W_, cin, ctx.dilation)
        elif gemm_dgrad:
            gx = _im2col_gemm(g, weight.flip(2, 3).transpose(0, 1), None, ctx.dilation, False)
        # weight gradient = im2col(x)^T @ g, taken as its transpose g^T @ im2col(x) (+0.6 %), again one hipBLASLt GEMM (K = B*H*W), for
        # the 41x41 layers from _WGRAD_MIN_COUT output channels (MIOpen's wrw runs fc6 at 650 TFLOP/s there)
        gemm_wgrad = gemm_dgrad and x.shape[2] * x.shape[3] <= _GEMM_WGRAD_MAX_MAP and x.shape[1] % 8 == 0 and cout >= _WGRAD_MIN_COUT
        gw = None
        if gemm_1x1:
            x2d = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])       # NHWC memory of a channels_last activation
            gw = torch.mm(g2d.t(), x2d).view(cout, x.shape[1], 1, 1)
            gemm_wgrad = True
        elif ctx.direct and g.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and \
                (x.shape[1], cout) in ((3, 64), (64, 64), (64, 128), (128, 128)):
            # the narrow full-resolution layers again: MIOpen's wrw kernels run them at ~250 TFLOP/s (conv1_2: 0.48 ms)
            gw = ops.conv3x3_wgrad(x, g)
            gemm_wgrad = True
        elif gemm_wgrad:
            cin = x.shape[1]
            if cols is None or cols.dtype != g.dtype:
                cols = ops.im2col3x3_nhwc(x.permute(0, 2, 3, 1).contiguous(), ctx.dilation)  # (M, 9*Cin)
            g2d = g.permute(0, 2, 3, 1).reshape(-1, cout)                                # (M, Cout), NHWC memory
            gw = torch.mm(g2d.t(), cols).view(cout, 3, 3, cin).permute(0, 3, 1, 2)
        mask = [ctx.needs_input_grad[0] and not gemm_dgrad, not gemm_wgrad, not fused]
        gx2 = gw2 = gb2 = None
        if any(mask):
            gx2, gw2, gb2 = torch.ops.aten.convolution_backward(
                g, x, weight, None if fused else [weight.shape[0]], [1, 1], [pad, pad],
                [ctx.dilation, ctx.dilation], False, [0, 0], 1, mask)
        return (gx if gemm_dgrad else gx2), (gw if gemm_wgrad else gw2), (gb if fused else gb2), None, None, None, None, None, None, None


class _IgemmConvFn(torch.autograd.Function):
    """n convolutions of one geometry (n = 1, or the four ASPP branches) + bias (+ ReLU (+ Dropout) (+ the stride-2 max pool)):
    apply(k, dils, relu, drop_p, pool, n, links_in, links_out, x_1..x_n, w_1..w_n, b_1..b_n) (links: lists of _GradLink or None —
    links_in[i] says x_i is the sole-consumer output of a ReLU node whose backward this node's data gradient absorbs).
    k = 3 (conv3_x .. fc6_k): forward, data and weight gradient by the implicit-GEMM kernels; k = 1 (fc7_k): the same with Dropout
    behind it, else forward and data gradient are plain hipBLASLt GEMMs over the NHWC matrices (nothing to gather) and the weight
    gradients of all branches one implicit-GEMM launch.
    x: bf16 channels_last; w, b: the float32 master parameters — the kernel is cast to bf16 by the same copy that packs it
    for the kernel, and the weight gradient comes back in float32, so autocast's per-layer casts both ways disappear.
    Backward: _backward_head, then data and weight gradients in ONE grid where all inputs need gradients and the kernels tile the
    shape, else the data gradients of all branches in one launch and the weight gradients in one."""
    LEAD = 8                                           # arguments of apply in front of the 3 n tensors

    @staticmethod
    def forward(ctx, k, dils, relu, drop_p, pool, n, links_in, links_out, *t):
        xs, ws, bs = t[:n], t[n:2 * n], t[2 * n:3 * n]
        # one tensor fed n times (the four fc6_k read pool5a's output): backward returns the sum of its n data gradients, formed in
        # one pass the way autograd's accumulation forms it, instead of leaving n - 1 pairwise adds to the engine
        # (bf16 inputs only: a float32 input's gradients are cast up before the engine adds them)
        ctx.same_x = n > 1 and xs[0].dtype == torch.bfloat16 and all(
            x.data_ptr() == xs[0].data_ptr() and x.shape == xs[0].shape and x.stride() == xs[0].stride() and x.dtype == xs[0].dtype
            and x._version == xs[0]._version for x in xs[1:])
        xs = [x if x.dtype == torch.bfloat16 else x.bfloat16() for x in xs]
        packs_d = [None] * n
        fb = [b.detach().float().contiguous() for b in bs]
        # Dropout rides in the implicit-GEMM epilogue (mask = f(seed, branch, position), p in steps of 1/256), always behind a ReLU:
        # GemmConv2d refuses fuse_dropout without fuse_relu and VGG16ASPP's grouped calls pass relu=True, so no caller needs a
        # Dropout pass of its own behind this node
        if drop_p > 0.0 and not relu:
            raise ValueError("_IgemmConvFn: Dropout needs the ReLU in front of it")
        fused_drop = drop_p > 0.0
        scale = 256.0 / (256 - min(255, int(drop_p * 256.0 + 0.5))) if fused_drop else 1.0
        seed = ops.dropout_seed() if fused_drop else 0
        if links_in is not None and not all(lk is not None for lk in links_in):
            links_in = None
        if k == 3 or fused_drop:
            # (fc7_k with Dropout behind it: one 1x1 implicit-GEMM launch for all branches with the mask in its epilogue beats four
            # hipBLASLt GEMMs + four dropout passes.)  Both packed forms of every kernel from the float32 master in one pass each,
            # the data-gradient form, which waits for backward, only where backward is sure to launch with it
            lead = _IgemmConvFn.LEAD
            need_d = (any(ctx.needs_input_grad[lead:lead + n]) and ops.conv_igemm_supported(ws[0].shape[0], ws[0].shape[1], 3)) \
                if k == 3 else (links_in is not None and _FUSE_CHAIN)
            packs = [ops.pack_conv_weight_pair(w, True, need_d) for w in ws]
            packs_d = [p[1] for p in packs]
            outs = ops.conv_igemm(xs, [p[0] for p in packs], fb, dils, k, relu, drop_p, seed)
        else:
            outs = [_im2col_gemm(x, w.to(torch.bfloat16), b.to(torch.bfloat16), 1, relu) for x, w, b in zip(xs, ws, bs)]
        ret, kept, code = _forward_tail(ctx, outs, relu, pool, links_out, scale)          # (a pool: n == 1, conv3_3)
        ctx.save_for_backward(code, *xs, *ws, *kept)
        # where a data-parallel reducer wants the weight gradients written (dsrg_amd/reducer.py: the parameters' bucket slots)
        ctx.gw_out = [getattr(w, "_dsrg_grad_out", None) for w in ws]
        ctx.packs_d = packs_d                  # not an input or output of the node: kept outside save_for_backward
        ctx.dils, ctx.n, ctx.k, ctx.links_in = dils, n, k, links_in
        return ret

    @staticmethod
    def backward(ctx, *gs):
        n, k, lead = ctx.n, ctx.k, _IgemmConvFn.LEAD
        code, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        xs, ws, ys = saved[:n], saved[n:2 * n], saved[2 * n:] or (None,) * n      # outputs: kept for a ReLU without a pool only
        cout, cin = ws[0].shape[0], ws[0].shape[1]
        gms, gbs = map(list, zip(*[_backward_head(ctx, g, ys[i], code, i) for i, g in enumerate(gs)]))
        need_x = list(ctx.needs_input_grad[lead:lead + n])
        # do the data-gradient launches that share a grid or a store with other work take this node
        takes = all(need_x) and ops.conv_igemm_supported(cout, cin, k) and all(x.is_contiguous(memory_format=torch.channels_last) for x in xs)
        # inputs that are another node's ReLU outputs with no other consumer: that node's backward rides in this data gradient
        absorb = takes and _FUSE_CHAIN and ctx.links_in is not None and cin >= 256
        masks, mask_scale = (list(xs), ctx.links_in[0].scale) if absorb else (None, 1.0)
        # both gradients in one grid: a single 3x3 layer, or the branches of one level
        merged = takes and ops.conv_igemm_wgrad_supported(cin, cout, k) and (n > 1 or k == 3)

        def packs_d():           # the forward's data-gradient packings, made now where it had no reason to (one route at most asks)
            return [p if p is not None else ops.pack_conv_weight(w, for_dgrad=True) for p, w in zip(ctx.packs_d, ws)]

        def library(i, which):   # shapes the kernels do not tile (input channels not a multiple of 128, ...): MIOpen / CK
            d = ctx.dils[i]
            return torch.ops.aten.convolution_backward(gms[i], xs[i], ws[i].to(torch.bfloat16), None, [1, 1], [d, d], [d, d], False,
                                                       [0, 0], 1, [which == 0, which == 1, False])[which]

        def wgrads():            # the weight gradients of all branches in a launch of their own: float32, the parameters' own layout
            if k == 1 or ops.conv_igemm_wgrad_supported(cin, cout, 3):
                return ops.conv_igemm_wgrad(list(xs), gms, ctx.dils, k, outs=ctx.gw_out)
            return [library(i, 1).float() for i in range(n)]

        gb_below = None
        if merged and n == 1:
            # ops.conv_igemm_backward: the data gradient's tiles and the weight gradient's workgroups share a grid, so the CUs a
            # 212-tile data gradient leaves idle do weight-gradient work
            gx, gw, gb = ops.conv_igemm_backward(gms[0], packs_d()[0], xs[0], ctx.dils[0], xs[0] if absorb else None, mask_scale,
                                                 gw_out=ctx.gw_out[0])
            gxs, gws, gb_below = [gx], [gw], [gb]
        elif merged:
            # the four ASPP branches (fc7_k: 1x1 with the mask and bias gradients of fc6_k in the store; fc6_k: 3x3, dilations 6 - 24):
            # the same one grid in the grouped forms of both halves.  With or without the masks: the weight gradient's pixel split
            # belongs to the grid, so fc7_k's weight gradients are the same bits whether or not fc6_k's ReLU backward rides along
            gxs, gws, gb_below = ops.conv_igemm_backward_groups(gms, packs_d(), list(xs), ctx.dils, k, masks, mask_scale,
                                                                gw_outs=ctx.gw_out)
        elif absorb:
            gxs, gb_below = ops.conv_igemm_dgrad(gms, packs_d(), masks, ctx.dils, k, mask_scale)
            gws = wgrads()
        elif k == 1:             # plain hipBLASLt GEMMs over the NHWC matrices
            gxs = [torch.mm(gm.permute(0, 2, 3, 1).reshape(-1, cout), w.to(torch.bfloat16).reshape(cout, cin)).view(
                x.shape[0], x.shape[2], x.shape[3], cin).permute(0, 3, 1, 2) if nx else None for gm, w, x, nx in zip(gms, ws, xs, need_x)]
            gws = wgrads()
        else:                    # the forward kernel on the flipped, transposed kernels
            gxs = [None] * n
            if any(need_x):
                gxs = ops.conv_igemm(gms, packs_d(), None, ctx.dils, 3, False) if ops.conv_igemm_supported(cout, cin, 3) else \
                    [library(i, 0) for i in range(n)]
            gws = wgrads()
        if absorb:
            for lk, gx, gb in zip(ctx.links_in, gxs, gb_below):
                lk.leave(gx, gb)
        # one tensor fed n times: rne(rne(rne(g_1 + g_2) + g_3) + g_4), the bits the engine's accumulation of its n gradients has
        # (the separate 1x1 launches never formed this sum, and no model feeds one tensor to several 1x1 layers: left to the engine)
        if ctx.same_x and all(need_x) and (merged or k == 3) and _sum_takes(gxs):
            gxs = [ops.sum_bf16(list(gxs))] + [None] * (n - 1)
        return (None,) * lead + tuple(gx if nx else None for gx, nx in zip(gxs, need_x)) + \
            tuple(_landed(gw, o) for gw, o in zip(gws, ctx.gw_out)) + tuple(gbs)


def _sum_takes(gs):
    """does ops.sum_bf16 take these gradients: 2..4 bf16 CUDA tensors of one shape and one dense layout, 8 | elements"""
    g0 = gs[0]
    return 2 <= len(gs) <= 4 and all(g is not None and g.is_cuda and g.dtype == torch.bfloat16 and g.shape == g0.shape and
                                     g.stride() == g0.stride() for g in gs) and g0.numel() > 0 and g0.numel() % 8 == 0 and \
        (g0.is_contiguous() or (g0.dim() == 4 and g0.is_contiguous(memory_format=torch.channels_last)))


class _DirectConvFn(torch.autograd.Function):
    """conv1_1 … conv2_2 (3 / 64 / 128 channels at 321x321 and 161x161) + bias + ReLU (+ the stride-2 max pool) on the direct
    kernels with the float32 MASTER parameters as inputs, as _IgemmConvFn takes them: one pass makes both bf16 kernels (forward;
    flipped + transposed for the data gradient), the bias is read as it is, weight and bias gradients come back in float32 —
    autocast's casts (kernel and bias down, both gradients up), the flip and its copy are gone: five small launches per layer.
    apply(x, weight, bias, relu, pool, link_in, link_out); links as in _IgemmConvFn."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, pool, link_in, link_out):
        cl = torch.channels_last
        if ops.image_takes_fused_cast(x):
            x = ops.image_to_bf16_nhwc(x)              # the float32 NCHW image: layout and cast in one pass, the same bits
        x = x if x.dtype == torch.bfloat16 else x.bfloat16()
        x = x if x.is_contiguous(memory_format=cl) else x.contiguous(memory_format=cl)
        if weight.shape[1] == 3:
            w16, wd = ops.cast_weight_kept(weight), None                                  # the image needs no gradient
        else:
            w16, wd = ops.pack_direct_weight_pair(weight, ctx.needs_input_grad[0])
        out = ops.conv3x3_direct(x, w16, bias.detach(), relu)
        (ret,), kept, code = _forward_tail(ctx, [out], relu, pool, [link_out] if link_out is not None else None, 1.0)
        ctx.save_for_backward(x, code, *kept)
        ctx.wd = wd                                    # not an input or output of the node: kept outside save_for_backward
        ctx.gw_out = getattr(weight, "_dsrg_grad_out", None)      # a reducer's slot for the weight gradient (dsrg_amd/reducer.py)
        ctx.link_in = link_in if (link_in is not None and link_in.scale == 1.0 and wd is not None) else None
        return ret

    @staticmethod
    def backward(ctx, g):
        x, code, *y = ctx.saved_tensors
        g, gb = _backward_head(ctx, g, y[0] if y else None, code)
        gx = None
        if ctx.needs_input_grad[0]:
            if _FUSE_CHAIN and ctx.link_in is not None:
                gx, gb_below = ops.conv3x3_direct_dgrad(g, ctx.wd, x)
                ctx.link_in.leave(gx, gb_below)
            else:
                gx = ops.conv3x3_direct(g, ctx.wd, None, False)
        gw = ops.conv3x3_wgrad(x, g, torch.float32, out=ctx.gw_out)
        return gx, _landed(gw, ctx.gw_out), gb, None, None, None, None


def _pool_in_node(cout):
    """can pool1-3 ride inside the conv node (pool backward + ReLU mask + bias gradient in one pass): the pool kernels' tiling,
    8 | channels and (channels / 8) | 256"""
    return cout % 8 == 0 and 256 % (cout // 8) == 0


def _direct_route(conv, x, p, pool):
    """does this GemmConv2d call take _DirectConvFn: one of the four narrow full-resolution layers with float32 channels_last
    master parameters under bf16 autocast, no Dropout, a pool only if it rides in the node (the node does not pool outside itself)"""
    cin, cout = conv.in_channels, conv.out_channels
    if not (conv.kernel_size == (3, 3) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is not None
            and (cin, cout) in ops.WGRAD_CONV_SHAPES and p == 0.0):
        return False
    if not _bf16_run(x):
        return False
    w = conv.weight
    if not (w.dtype == torch.float32 and conv.bias.dtype == torch.float32 and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    if cin == 3 and x.requires_grad and torch.is_grad_enabled():      # no direct data gradient into three channels (the image needs none)
        return False
    return pool is None or _pool_in_node(cout)


def _igemm_route(conv, x, groups=1):
    """does this GemmConv2d call take the implicit-GEMM kernels: a 3x3 'same' convolution with bias on bf16 activations
    (autocast), 64 | input channels, 256 | output channels — and enough 256 x 256 output tiles to occupy the chip
    (_IGEMM_MIN_TILES); `groups` problems share the launch (the four fc6_k)"""
    if not (_IGEMM and x.is_cuda and conv.gemm and conv.kernel_size == (3, 3) and conv.bias is not None and conv.groups == 1):
        return False
    if not _bf16_run(x):
        return False
    if conv.out_channels < 256:                 # conv1_x / conv2_x: the direct kernels (weights in registers) serve the narrow layers
        return False
    pixels = x.shape[0] * x.shape[2] * x.shape[3]
    if groups * ((pixels + 255) // 256) * ((conv.out_channels + 255) // 256) < _IGEMM_MIN_TILES:
        return False
    return ops.conv_igemm_supported(conv.in_channels, conv.out_channels, 3)


class GemmConv2d(nn.Conv2d):
    """nn.Conv2d (same parameters, same init, same state_dict) with the following ReLU (`fuse_relu`), Dropout (`fuse_dropout` = p,
    needs fuse_relu) and stride-2 max pool (`fuse_pool`) in the same autograd node.  A stride-1 'same' 3x3 / 1x1 call on the GPU
    picks its node from what it observes: _IgemmConvFn (_igemm_route: bf16 run, >= 256 output channels, >= _IGEMM_MIN_TILES
    tiles), else _DirectConvFn (_direct_route: the four narrow layers with float32 channels_last masters under bf16 autocast),
    else _ConvFn (its docstring lists what that leaves; `gemm` there chooses im2col + GEMM over MIOpen).  Any other call, and the
    CPU, is the plain convolution (+ ReLU (+ Dropout) (+ pool)).

    Contract of the fused forms (what a user of these modules may and may not rely on):
      * `fuse_dropout` = p is realised in steps of 1/256 on the implicit-GEMM route (keep a value iff its random byte >= round(256 p);
        scale 256 / (256 - round(256 p))): p = 0.5 is exact, p = 0.3 becomes 77/256 = 0.3008.  The mask is a pure function of (seed,
        branch, position) drawn per forward from torch's generator (ops.dropout_seed), so torch.manual_seed reproduces it;
      * `chain_input=True` is the caller's PROMISE that this layer's input is the fused-ReLU output of the GemmConv2d in front of it
        and feeds nothing else.  Then the data gradient this layer returns for that activation is ALREADY masked by the lower layer's
        ReLU (and scaled by its Dropout): it is the gradient with respect to the lower layer's pre-activation, not dL/dy.  Such
        chained activations are therefore not autograd inspection points — `retain_grad()`, `torch.autograd.grad` or a tensor hook
        on them sees the masked value; a hook that RETURNS a new tensor makes the lower node fall back to its own ReLU backward
        (right on a masked gradient too) or, when a Dropout scale rides in the mask, raise (`_GradLink.take`).  Without the
        promise (the default) every activation is an ordinary autograd tensor;
      * `fuse_pool`: the node returns the pooled tensor only; the un-pooled ReLU output is not kept (the window codes carry its
        mask) and cannot be asked for."""

    def __init__(self, *args, fuse_relu=False, gemm=True, fuse_dropout=0.0, fuse_pool=None, chain_input=False, **kw):
        super().__init__(*args, **kw)
        # chain_input: the caller's promise that this layer's input is the fused-ReLU output of the GemmConv2d in front of it and
        # feeds nothing else — the data gradient may then carry that layer's ReLU backward and bias gradient (_GradLink)
        self.chain_input = bool(chain_input)
        if fuse_dropout and not fuse_relu:
            raise ValueError("fuse_dropout needs fuse_relu (the fused backward reads both masks from the output sign)")
        if fuse_pool is not None and (not fuse_relu or fuse_dropout or fuse_pool[0] != 2):
            raise ValueError("fuse_pool = (2, ceil_mode) follows a fused ReLU without dropout")
        self.fuse_relu, self.gemm, self.fuse_dropout = fuse_relu, gemm, float(fuse_dropout)
        self.fuse_pool = fuse_pool                                      # the 3x3 / stride 2 / pad 1 max pool behind the ReLU, (2, ceil_mode)

    def forward(self, x):
        p = self.fuse_dropout if self.training else 0.0
        pool = self.fuse_pool
        if x.is_cuda and self.stride == (1, 1) and self.kernel_size[0] in (1, 3) and \
                self.padding[0] == self.dilation[0] * (self.kernel_size[0] // 2):
            igemm = _igemm_route(self, x)
            direct = not igemm and _direct_route(self, x, p, pool)     # (refuses a pool it could not take into the node)
            # the pool rides inside the node when its kernels apply: their tiling of the channels and, which the two routes above have
            # checked for themselves, a bias and bf16 activations (autocast)
            in_node = pool is not None and _pool_in_node(self.out_channels) and (
                igemm or direct or (self.bias is not None and _bf16_run(x)))
            lin = getattr(x, "_dsrg_grad_link", None) if self.chain_input else None
            # a consumer may fold this node's ReLU backward into its data gradient (_GradLink); behind Dropout only the implicit-GEMM
            # node leaves the scale in the link (_ConvFn accepts a link without Dropout only, _direct_route takes no Dropout)
            lout = _GradLink() if (self.fuse_relu and pool is None and (igemm or p == 0.0) and torch.is_grad_enabled()) else None
            node_pool = pool if in_node else None
            if igemm:
                (out,) = _IgemmConvFn.apply(3, [self.dilation[0]], self.fuse_relu, p, node_pool, 1, [lin] if lin is not None else None,
                                            [lout] if lout is not None else None, x, self.weight, self.bias)
            elif direct:
                out = _DirectConvFn.apply(x, self.weight, self.bias, self.fuse_relu, node_pool, lin, lout)
            else:
                out = _ConvFn.apply(x, self.weight, self.bias, self.dilation[0], self.fuse_relu, self.gemm, p, node_pool, lin, lout)
            if lout is not None:
                out._dsrg_grad_link = lout
            return out if pool is None or in_node else _pool3x3(out, pool[0], pool[1])
        out = super().forward(x)
        out = F.relu(out) if self.fuse_relu else out
        out = F.dropout(out, p, True) if p > 0.0 else out
        return out if pool is None else _pool3x3(out, pool[0], pool[1])


class FusedReLU(nn.Identity):
    """placeholder that keeps the Sequential indices (and state_dict keys) of the conv/ReLU pairs: the ReLU itself
    runs inside the GemmConv2d in front of it"""


class FusedPool(nn.Identity):
    """placeholder for the max-pool layer that runs inside the GemmConv2d two slots in front of it (`fuse_pool`)"""


class FusedDropout(nn.Identity):
    """placeholder for the Dropout layer that runs inside the GemmConv2d two slots in front of it (`fuse_dropout`)"""


def _hip_pool_takes(x):
    """does the HIP pooling pass take x: bf16 channels_last on the GPU, 8 | channels (16-byte channel groups)"""
    return x.is_cuda and x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0 and x.is_contiguous(memory_format=torch.channels_last)


class _MaxPool3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride, ceil_mode):
        out, code = ops.maxpool3x3_fwd(x, stride, ceil_mode)
        ctx.save_for_backward(code)
        ctx.in_shape, ctx.stride = x.shape, stride
        return out

    @staticmethod
    def backward(ctx, g):
        (code,) = ctx.saved_tensors
        return ops.maxpool3x3_bwd(g, code, ctx.in_shape, ctx.stride), None, None


class _AvgPool3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.avgpool3x3_s1(x)

    @staticmethod
    def backward(ctx, g):
        return ops.avgpool3x3_s1(g)                                          # symmetric stencil: its own adjoint


class AvgPool3x3(nn.AvgPool2d):
    """pool5a: 3x3 / stride 1 / pad 1 average over padded windows (Caffe AVE); one HIP pass each way for bf16
    channels_last activations, nn.AvgPool2d otherwise.  Not only a speed matter: PyTorch-ROCm 2.10's avg_pool2d
    backward returns wrong gradients for channels_last inputs (tests/test_gpu_parity.py checks ours against the fp32
    NCHW adjoint), so any other channels_last input is made contiguous first."""

    def __init__(self):
        super().__init__(3, 1, 1)

    def forward(self, x):
        if _hip_pool_takes(x):
            return _AvgPool3x3Fn.apply(x)
        if x.is_cuda and x.dim() == 4 and not x.is_contiguous():
            x = x.contiguous()                                            # keep torch's kernel on its correct (NCHW) path
        return super().forward(x)


class MaxPool3x3(nn.MaxPool2d):
    """3x3 / pad 1 max pooling (stride 1 or 2): one HIP pass each way over bf16 channels_last activations with
    1-byte window codes instead of torch's int64 indices; anything else takes nn.MaxPool2d's path."""

    def __init__(self, stride, ceil_mode=False):
        super().__init__(3, stride, 1, ceil_mode=ceil_mode)

    def forward(self, x):
        return _pool3x3(x, self.stride, self.ceil_mode)


def _pool3x3(x, stride, ceil_mode):
    """3x3 / pad 1 max pool outside a conv node: the HIP pass for bf16 channels_last activations, torch's otherwise"""
    if _hip_pool_takes(x):
        return _MaxPool3x3Fn.apply(x, stride, ceil_mode)
    return F.max_pool2d(x, 3, stride, 1, ceil_mode=ceil_mode)


def _conv_relu(cin, cout, dilation=1, gemm=False, pool=None, chain=False):
    """conv + ReLU (+ the stride-2 max pool behind them, `pool` = (2, ceil_mode)): Sequential slots as in the prototxt;
    chain: the input is the conv + ReLU in front and nothing else reads it (GemmConv2d.chain_input)"""
    conv = GemmConv2d(cin, cout, 3, padding=dilation, dilation=dilation, fuse_relu=True, gemm=gemm, fuse_pool=pool, chain_input=chain)
    return [conv, FusedReLU()] + ([FusedPool()] if pool is not None else [])


class _HeadsFn(torch.autograd.Function):
    """The four fc8-SEC_k classifiers + Eltwise SUM on bf16 activations with fp32 weights, fp32 accumulation and an fp32
    NCHW result (one HIP pass on the f32-input MFMA, ops.heads_forward).  Backward (ops.heads_backward): the gradient that
    continues into the bf16 trunk is accumulated in fp32 and rounded once; weight and bias gradients are fp32."""

    @staticmethod
    def forward(ctx, links, weight, bias, *xs):
        cl = torch.channels_last
        # links: the x_k are ReLU (+ Dropout) outputs of nodes that feed these classifiers only (their backward rides along)
        ctx.links = links if (links is not None and all(lk is not None for lk in links) and
                              all(x.is_contiguous(memory_format=cl) for x in xs)) else None
        xs = [x.contiguous(memory_format=cl) for x in xs]
        weight = weight.contiguous()
        ctx.save_for_backward(weight, *xs)
        return ops.heads_forward(xs, weight, bias.contiguous())

    @staticmethod
    def backward(ctx, g):
        weight, *xs = ctx.saved_tensors
        n, O, K = weight.shape
        if _FUSE_CHAIN and ctx.links is not None and all(ctx.needs_input_grad[3:]):
            gxs, gw, gb_below = ops.heads_backward(xs, weight, g, True, ctx.links[0].scale)
            for i, lk in enumerate(ctx.links):
                lk.leave(gxs[i], gb_below[i])
        else:
            gxs, gw = ops.heads_backward(xs, weight, g, need_gx=any(ctx.needs_input_grad[3:]))
        gb1 = g.sum((0, 2, 3))                                            # fp32, the same for every branch
        return (None, gw, gb1.unsqueeze(0).expand(n, O).contiguous()) + (tuple(gxs) if gxs is not None else (None,) * n)


class _HeadsPtrFn(torch.autograd.Function):
    """_HeadsFn with the n classifier kernels and biases read where the parameters lie (ops.heads_forward_ptrs: no stacked copy
    of either per step) and every kernel's gradient written to a tensor of its own with the parameter's strides — a reducer's slot
    (`_dsrg_grad_out`) where the parameter names one.  apply(links, n, w_1..w_n, b_1..b_n, x_1..x_n); the same bits as _HeadsFn."""
    LEAD = 2                                           # arguments of apply in front of the 3 n tensors

    @staticmethod
    def forward(ctx, links, n, *t):
        ws, bs, xs = t[:n], t[n:2 * n], t[2 * n:]
        cl = torch.channels_last
        ctx.links = links if (links is not None and all(lk is not None for lk in links) and
                              all(x.is_contiguous(memory_format=cl) for x in xs)) else None
        xs = [x.contiguous(memory_format=cl) for x in xs]
        ctx.n = n
        ctx.gw_out = [getattr(w, "_dsrg_grad_out", None) for w in ws]
        ctx.save_for_backward(*ws, *xs)
        return ops.heads_forward_ptrs(xs, [w.detach() for w in ws], [b.detach() for b in bs])

    @staticmethod
    def backward(ctx, g):
        n = ctx.n
        ws, xs = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        O = ws[0].shape[0]
        need_x = ctx.needs_input_grad[_HeadsPtrFn.LEAD + 2 * n:]
        if _FUSE_CHAIN and ctx.links is not None and all(need_x):
            gxs, gws, gb_below = ops.heads_backward_ptrs(xs, ws, g, True, ctx.links[0].scale, gw_outs=ctx.gw_out)
            for i, lk in enumerate(ctx.links):
                lk.leave(gxs[i], gb_below[i])
        else:
            gxs, gws = ops.heads_backward_ptrs(xs, ws, g, need_gx=any(need_x), gw_outs=ctx.gw_out)
        gb = g.sum((0, 2, 3)).unsqueeze(0).expand(n, O).contiguous()      # fp32, the same for every branch (torch's sum, as _HeadsFn)
        gws = [_landed(gw, o) for gw, o in zip(gws, ctx.gw_out)]
        return (None,) * _HeadsPtrFn.LEAD + tuple(gws) + tuple(gb[i] for i in range(n)) + (tuple(gxs) if gxs is not None else (None,) * n)


class _StackKernels(torch.autograd.Function):
    """the (cout, cin, 1, 1) classifier kernels as one (n, cout, cin) tensor; backward hands every kernel its slice of the gradient
    in the PARAMETER's strides (a channels_last 1x1 kernel has strides (cin, 1, cin, cin); the plain reshape's gradient has
    (cin, 1, 1, 1) — the same memory, but DistributedDataParallel compares strides, warns and copies the gradient into its bucket)"""

    @staticmethod
    def forward(ctx, *ws):
        ctx.layouts = [(tuple(w.shape), tuple(w.stride())) for w in ws]
        return torch.stack([w.reshape(w.shape[0], w.shape[1]) for w in ws])

    @staticmethod
    def backward(ctx, g):
        return tuple(g[i].as_strided(shape, stride) if g[i].is_contiguous() else g[i].reshape(shape)
                     for i, (shape, stride) in enumerate(ctx.layouts))


class VGG16ASPP(nn.Module):
    """features (conv1_1 .. conv5_3, pools, pool5a) + four ASPP branches fc6_k -> fc7_k -> fc8-SEC_k, summed.  On a GPU under
    bf16 autocast conv1_2, conv2_2, conv3_2 .. conv5_3, fc7_k and the classifiers are built with `chain_input` (see GemmConv2d):
    the activations between them are not autograd inspection points, and Dropout's p is rounded to a multiple of 1/256 (the
    prototxt's 0.5 is exact).  `DSRG_FUSE_CHAIN=0` restores one ordinary autograd node per layer."""

    def __init__(self, num_classes=21, dropout=0.5, gemm_convs=True):
        super().__init__()
        L = []
        p2 = (2, True)                                                  # pool1-3: 3x3 / stride 2 / pad 1, ceil mode (Caffe), inside the conv node
        L += _conv_relu(3, 64) + _conv_relu(64, 64, pool=p2, chain=True)
        L += _conv_relu(64, 128, 1, gemm_convs) + _conv_relu(128, 128, 1, gemm_convs, pool=p2, chain=True)
        L += _conv_relu(128, 256, 1, gemm_convs) + _conv_relu(256, 256, 1, gemm_convs, chain=True) + \
            _conv_relu(256, 256, 1, gemm_convs, pool=p2, chain=True)
        g = gemm_convs                                                  # the 41x41 stages
        L += _conv_relu(256, 512, 1, g) + _conv_relu(512, 512, 1, g, chain=True) + _conv_relu(512, 512, 1, g, chain=True) + [MaxPool3x3(1)]
        L += _conv_relu(512, 512, 2, g) + _conv_relu(512, 512, 2, g, chain=True) + _conv_relu(512, 512, 2, g, chain=True) + [MaxPool3x3(1)]
        L += [AvgPool3x3()]                                   # pool5a AVE (count_include_pad, as Caffe)
        self.features = nn.Sequential(*L)
        self.branches = nn.ModuleList()
        for d in (6, 12, 18, 24):
            g = gemm_convs
            fc8 = GemmConv2d(1024, num_classes, 1, gemm=g)
            nn.init.normal_(fc8.weight, std=0.01)
            nn.init.zeros_(fc8.bias)
            self.branches.append(nn.Sequential(
                GemmConv2d(512, 1024, 3, padding=d, dilation=d, fuse_relu=True, gemm=g, fuse_dropout=dropout), FusedReLU(),
                FusedDropout(),
                GemmConv2d(1024, 1024, 1, fuse_relu=True, gemm=g, fuse_dropout=dropout), FusedReLU(), FusedDropout(), fc8))

    def forward(self, x):
        """-> fc8-SEC scores (B,21,h,w) in float32.  Under autocast the trunk and fc6/fc7 run in the autocast dtype, but
        the four fc8-SEC_k classifiers and their Eltwise SUM (train-s.prototxt:737-744) always run in float32 (fp32
        weights, fp32 accumulation, fp32 sum): these scores feed hard decisions the reference takes on fp32/fp64 values
        (Softmax + 1e-4, the CRF, the 0.85 / 0.99 SRG thresholds, the 0.05 / 20 clip of the constrain loss), and a bf16
        score of magnitude 8-16 has a step of 0.06-0.125."""
        f = self.features(x)
        hs = self._grouped_branches(f)
        if hs is None:
            hs = [f] * len(self.branches)
            for i, br in enumerate(self.branches):
                for m in list(br)[:-1]:
                    hs[i] = m(hs[i])
        heads = [br[-1] for br in self.branches]
        out = self._fused_heads(heads, hs)
        if out is None:
            with torch.autocast(device_type=hs[0].device.type, enabled=False):
                for m, h in zip(heads, hs):
                    s = m(h.float())
                    out = s if out is None else out + s
        return out

    def _grouped_branches(self, f):
        """pool5a's output -> the fc7_k outputs with the four fc6_k (same input, own dilation) in one launch each way: 1696 tiles fill
        the chip where 424 leave a sixth idle; None where the launch does not take them (_igemm_route)"""
        fc6 = [br[0] for br in self.branches]
        n = len(fc6)
        if not (n <= 4 and all(_igemm_route(m, f, n) and m.stride == (1, 1) and m.padding == m.dilation for m in fc6)):
            return None
        p = fc6[0].fuse_dropout if self.training else 0.0
        links = [_GradLink() for _ in range(n)] if torch.is_grad_enabled() else None
        hs = list(_IgemmConvFn.apply(3, [m.dilation[0] for m in fc6], True, p, None, n, None, links, *([f] * n),
                                     *[m.weight for m in fc6], *[m.bias for m in fc6]))
        fc7 = [br[3] for br in self.branches]
        if not all(isinstance(m, GemmConv2d) and m.kernel_size == (1, 1) and m.fuse_relu and m.bias is not None and m.gemm
                   and m.in_channels % 256 == 0 and m.out_channels % 256 == 0 for m in fc7):
            for i, br in enumerate(self.branches):
                for m in list(br)[1:-1]:
                    hs[i] = m(hs[i])
            return hs
        # fc7_k: own input each, one launch for the four weight gradients; fc6_k's output feeds fc7_k only, so its ReLU / Dropout
        # backward and bias gradient ride in fc7_k's data gradient (links), as fc7_k's ride in the classifiers' (links7)
        p7 = fc7[0].fuse_dropout if self.training else 0.0
        links7 = [_GradLink() for _ in range(n)] if torch.is_grad_enabled() else None
        hs = list(_IgemmConvFn.apply(1, [1] * n, True, p7, None, n, links, links7, *hs, *[m.weight for m in fc7], *[m.bias for m in fc7]))
        for h, lk in zip(hs, links7 or []):
            h._dsrg_grad_link = lk
        return hs

    def _fused_heads(self, heads, hs):
        """the four classifiers and their sum in one HIP pass each way over bf16 fc7_k outputs; None where the kernels do not take them"""
        if not (hs[0].is_cuda and hs[0].dtype == torch.bfloat16 and len(hs) <= 4 and heads[0].out_channels <= 32
                and heads[0].in_channels % 256 == 0):
            return None
        # (on the grouped route the fc7_k outputs feed these classifiers and nothing else)
        links = [getattr(h, "_dsrg_grad_link", None) for h in hs]
        if all(m.bias is not None for m in heads) and ops.heads_kernels_in_place([m.weight for m in heads], [m.bias for m in heads]):
            # the kernels and biases read where they lie, every weight gradient written to its own tensor
            return _HeadsPtrFn.apply(links, len(heads), *[m.weight for m in heads], *[m.bias for m in heads], *hs)
        w = _StackKernels.apply(*[m.weight for m in heads])       # the fallback (another dtype / layout): stacked copies
        b = torch.stack([m.bias for m in heads])
        return _HeadsFn.apply(links, w.float(), b.float(), *hs)

    def caffe_param_groups(self):
        """lr_mult / decay_mult of the prototxt: weights (1,1), biases (2,0); fc8-SEC (10,1)/(20,0)."""
        groups = {}
        for name, p in self.named_parameters():
            is_fc8 = name.startswith("branches") and name.split(".")[2] == "6"
            is_bias = name.endswith("bias")
            key = ((10.0 if is_fc8 else 1.0) * (2.0 if is_bias else 1.0), 0.0 if is_bias else 1.0)
            groups.setdefault(key, []).append(p)
        return [dict(params=ps, lr_mult=k[0], decay_mult=k[1]) for k, ps in groups.items()]


def count_flops_per_image(size=321):
    """forward multiply-accumulates x2 of the conv stack at size x size (160.2 GFLOP)."""
    def pool(n): return -(-(n + 2 - 3) // 2) + 1
    h1 = size; h2 = pool(h1); h3 = pool(h2); h4 = pool(h3)
    macs = 0
    for (cin, cout, h, n) in [(3, 64, h1, 1), (64, 64, h1, 1), (64, 128, h2, 1), (128, 128, h2, 1),
                              (128, 256, h3, 1), (256, 256, h3, 2), (256, 512, h4, 1), (512, 512, h4, 5)]:
        macs += n * cin * cout * 9 * h * h
    macs += 4 * (512 * 1024 * 9 + 1024 * 1024 + 1024 * 21) * h4 * h4
    return 2 * macs


class GraphedForward(object):
    """An eval-mode forward of `net` captured once into a hipGraph (torch.cuda.CUDAGraph) and replayed per call.  At batch 1
    the VGG16-ASPP forward is ~150 launches of 3-30 us and launch-bound (1.6 ms eager, 0.7 ms replayed); its shapes, weights
    and buffers are static at test time, and every HIP kernel of this package launches on torch's current stream, which is
    the capture stream.  The eager warm-up runs first so that TunableOp has picked its GEMM solutions and the kernels have
    reserved their LDS outside the capture.  __call__(x) copies x into the captured input buffer and returns the captured
    output buffer (overwritten by the next call).  capture_error_mode: torch.cuda.graph's; "thread_local" lets other host threads
    (the CRF workers of the test-time loop) allocate and synchronise while this thread captures."""

    def __init__(self, net, example, amp_dtype=torch.bfloat16, warmup=3, capture_error_mode="global"):
        if net.training:
            raise ValueError("GraphedForward captures an eval-mode forward (dropout would replay one mask)")
        self.net, self.amp = net, amp_dtype
        self.x = example.detach().clone(memory_format=torch.preserve_format)
        warm = torch.cuda.Stream(device=example.device)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            for _ in range(warmup):
                self._fwd()
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # (on a stream no CRF worker of the test-time loops can hold: streams.py)
        with torch.cuda.graph(self.graph, stream=capture_stream(example.device), capture_error_mode=capture_error_mode):
            self.out = self._fwd()

    def _fwd(self):
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp, enabled=self.amp is not None):
            return self.net(self.x).contiguous()

    def __call__(self, x=None):
        if x is not None and x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x)
        self.graph.replay()
        return self.out
