"""GPU: the classifier heads read their parameters in place, and the small passes at the ends of the train step run as HIP kernels
(image layout + cast, conv1_1's bf16 kernel from the update, the total loss, the one-pass sum of the fc6 data gradients).  Every
comparison is on bit patterns: none of these changes may move a result."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


def bits(t):
    """the bit patterns of a tensor in its logical order (NaNs compare by payload)"""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _vp4(ts):
    return (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - len(ts))))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- heads: pointer form against the stacked form
@pytest.mark.parametrize("relu_scale", [0.0, 2.0])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 3, 5)])        # M = 70: a ragged 64-row workgroup and a ragged 32-row tile; M = 15 < 32
@pytest.mark.parametrize("n", [4, 1])
@pytest.mark.parametrize("K", [256, 1024])
def test_heads_pointer_form_equals_the_stacked_form(ops, K, n, B, H, W, relu_scale):
    from dsrg_amd import _lib
    L = _lib.lib()
    O, M = 21, B * H * W
    gen = torch.Generator(device="cuda").manual_seed(1000 + K + 10 * n + M)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)       # noqa: E731
    xs = [torch.relu(rnd(B, K, H, W)).bfloat16().contiguous(memory_format=CL) for _ in range(n)]
    for x in xs:
        x.permute(0, 2, 3, 1).reshape(-1)[::37] = -0.0
    w = rnd(n, O, K) * 0.05
    b = rnd(n, O)
    g = rnd(B, O, H, W)
    # the parameters as the net holds them: channels_last (O, K, 1, 1) kernels and (O) biases, each a tensor of its own
    ws = [w[k].clone().reshape(O, K, 1, 1).contiguous(memory_format=CL) for k in range(n)]
    bs = [b[k].clone() for k in range(n)]
    assert ops.heads_kernels_in_place(ws, bs)

    # forward, straight through the C ABI into a NaN-filled result
    want = ops.heads_forward(xs, w, b)
    out = torch.full((B, O, H, W), NAN, device="cuda")
    assert L.dsrg_heads_forward_ptrs_bf16(_vp4(xs), n, _vp4(ws), _vp4(bs), _p(out), B, H * W, K, O, _stream()) == 0
    assert same_bits(out, want)
    assert same_bits(ops.heads_forward_ptrs(xs, ws, bs), want)
    assert same_bits(ops.heads_forward_ptrs(xs, ws, None), ops.heads_forward(xs, w, None))

    # backward: gx, every gw (into destinations the caller gives) and, with the ReLU / Dropout link, the layer-below bias gradient
    if relu_scale > 0.0:
        gx_w, gw_w, gb_w = ops.heads_backward(xs, w, g, True, relu_scale)
    else:
        (gx_w, gw_w), gb_w = ops.heads_backward(xs, w, g), None
    dests = [torch.full((O, K, 1, 1), NAN, device="cuda").contiguous(memory_format=CL) for _ in range(n)]
    gx = torch.full((n, B, H, W, K), NAN, device="cuda", dtype=torch.bfloat16)
    gb = torch.full((n, K), NAN, device="cuda") if relu_scale > 0.0 else None
    part = torch.full((L.dsrg_heads_backward_chunks(M) * n * O * K,), NAN, device="cuda")
    nws = L.dsrg_heads_backward_relu_workspace(n, M, K)
    wsb = torch.empty(nws, dtype=torch.uint8, device="cuda")
    assert L.dsrg_heads_backward_ptrs_bf16(_vp4(xs), n, _vp4(ws), _p(g), _p(gx), M * K * 2, _vp4(dests), _p(part), float(relu_scale),
                                           _p(gb), _p(wsb), nws, B, H * W, K, O, _stream()) == 0
    for k in range(n):
        assert same_bits(gx[k].permute(0, 3, 1, 2), gx_w[k]), k
        assert same_bits(dests[k].reshape(O, K), gw_w[k]), k
    if relu_scale > 0.0:
        assert same_bits(gb, gb_w)
    # the Python wrapper: the destinations it is given are the tensors it returns
    dests2 = [torch.full((O, K, 1, 1), NAN, device="cuda").contiguous(memory_format=CL) for _ in range(n)]
    res = ops.heads_backward_ptrs(xs, ws, g, True, relu_scale, gw_outs=dests2)
    assert all(a is d for a, d in zip(res[1], dests2))
    for k in range(n):
        assert same_bits(res[0][k], gx_w[k]) and same_bits(res[1][k].reshape(O, K), gw_w[k])
    if relu_scale > 0.0:
        assert same_bits(res[2], gb_w)
    # weight gradient alone (no data gradient asked for), fresh destinations with the kernels' strides
    _, gws = ops.heads_backward_ptrs(xs, ws, g, need_gx=False)
    for k in range(n):
        assert gws[k].stride() == ws[k].stride() and same_bits(gws[k].reshape(O, K), gw_w[k])


def test_heads_node_equals_the_stacked_node(ops):
    """backbone._HeadsPtrFn against _StackKernels + torch.stack + _HeadsFn: scores and every parameter / input gradient"""
    from dsrg_amd import backbone
    torch.manual_seed(3)
    n, O, K, B, H, W = 4, 21, 256, 2, 5, 7
    xs = [torch.randn(B, K, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in range(n)]
    w0 = [(torch.randn(O, K, 1, 1, device="cuda") * 0.05).contiguous(memory_format=CL) for _ in range(n)]
    b0 = [torch.randn(O, device="cuda") for _ in range(n)]
    g = torch.randn(B, O, H, W, device="cuda")
    res = []
    for ptr in (True, False):
        ws = [t.clone(memory_format=torch.preserve_format).requires_grad_(True) for t in w0]
        bs = [t.clone().requires_grad_(True) for t in b0]
        xa = [x.clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs]
        if ptr:
            y = backbone._HeadsPtrFn.apply(None, n, *ws, *bs, *xa)
        else:
            y = backbone._HeadsFn.apply(None, backbone._StackKernels.apply(*ws), torch.stack(bs), *xa)
        y.backward(g)
        res.append([y] + [t.grad for t in ws + bs + xa])
    for a, b in zip(*res):
        assert same_bits(a, b)
    for gw, w in zip(res[0][1:1 + n], w0):
        assert gw.stride() == w.stride()


# ---------------------------------------------------------------- the weight gradient's fixed-order reduction
def _first_m_with_chunks(L, ok):
    for M in range(1, 1 << 16):
        if ok(L.dsrg_heads_backward_chunks(M)):
            return M
    raise AssertionError("no such M")


@pytest.mark.parametrize("case", ["batches_and_tail", "one_chunk"])
def test_heads_weight_gradient_is_the_chunk_order_sum(ops, case):
    """gw == the float32 sum of the partial planes in chunk order 0 .. nchunks - 1, formed on the host: more than two load batches
    of 16 with a ragged last one, and a single chunk"""
    from dsrg_amd import _lib
    L = _lib.lib()
    batch = 16
    if case == "one_chunk":
        M = 70
    else:
        M = _first_m_with_chunks(L, lambda c: c >= 2 * batch and c % batch != 0)
    nch = L.dsrg_heads_backward_chunks(M)
    assert nch == 1 if case == "one_chunk" else (nch >= 2 * batch and nch % batch)
    n, O, K, B = 2, 21, 256, 1
    gen = torch.Generator(device="cuda").manual_seed(77)
    xs = [torch.randn(B, K, M, 1, device="cuda", generator=gen).bfloat16().contiguous(memory_format=CL) for _ in range(n)]
    w = torch.randn(n, O, K, device="cuda", generator=gen) * 0.05
    g = torch.randn(B, O, M, 1, device="cuda", generator=gen)
    part = torch.full((nch * n * O * K,), NAN, device="cuda")
    gw = torch.full((n, O, K), NAN, device="cuda")
    assert L.dsrg_heads_backward_bf16(_vp4(xs), n, _p(w), _p(g), None, 0, _p(gw), _p(part), B, M, K, O, _stream()) == 0
    planes = part.view(nch, n, O, K).cpu().numpy()
    assert np.isfinite(planes).all()
    s = np.zeros((n, O, K), dtype=np.float32)
    for c in range(nch):
        s = s + planes[c]                                                   # float32, chunk order
    assert np.array_equal(gw.cpu().numpy().view(np.int32), s.view(np.int32))


# ---------------------------------------------------------------- image: float32 NCHW -> bf16 NHWC
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 33, 31)])
def test_image_cast_equals_torchs_two_passes(ops, shape):
    gen = torch.Generator(device="cuda").manual_seed(shape[2])
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, device="cuda", generator=gen, dtype=torch.int64).to(torch.int32)
    special = [0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7f800000, 0xff800000,      # +-0, NaNs, +-inf
               0x00000001, 0x807fffff, 0x00008000, 0x00018000,                                                       # denormals (one a tie)
               0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7f8000, 0x7f7fffff]      # ties, neighbours, overflow
    sp = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in special], dtype=torch.int32, device="cuda")
    flat = x.view(-1)
    flat[:sp.numel()] = sp
    flat[-sp.numel():] = sp.flip(0)
    x = x.view(torch.float32)
    assert ops.image_takes_fused_cast(x)
    want = x.contiguous(memory_format=CL).bfloat16()
    got = ops.image_to_bf16_nhwc(x)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape and got.is_contiguous(memory_format=CL)
    assert same_bits(got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1))


# ---------------------------------------------------------------- conv1_1's bf16 kernel from the update
def test_conv1_1_keeps_its_bf16_kernel_through_the_update(ops):
    from dsrg_amd.trainer import CaffeSGD
    torch.manual_seed(11)
    p = torch.nn.Parameter((torch.randn(64, 3, 3, 3, device="cuda") * 0.1).contiguous(memory_format=CL))
    wide = torch.nn.Parameter((torch.randn(64, 64, 3, 3, device="cuda") * 0.1).contiguous(memory_format=CL))
    bias = torch.nn.Parameter(torch.randn(64, device="cuda"))
    fc8 = torch.nn.Parameter((torch.randn(21, 256, 1, 1, device="cuda") * 0.01).contiguous(memory_format=CL))
    opt = CaffeSGD([dict(params=[bias, p, fc8], lr_mult=1.0, decay_mult=1.0), dict(params=[wide], lr_mult=2.0, decay_mult=0.0)],
                   base_lr=0.1)
    first = ops.cast_weight_kept(p)                         # what conv1_1's forward does: the first time a fresh cast
    assert same_bits(first, p.detach().to(torch.bfloat16)) and first.stride() == p.stride()
    ops.pack_direct_weight_pair(wide)                       # another kept kernel in the same launch
    kept_ptr = first.data_ptr()
    for step in (1, 2):
        before = p.detach().clone(memory_format=torch.preserve_format)
        for t in (p, wide, bias, fc8):
            t.grad = torch.randn_like(t, memory_format=torch.preserve_format)
        opt.step()
        assert not torch.equal(before, p.detach())
        kept = ops.cast_weight_kept(p)
        assert kept.data_ptr() == kept_ptr, "the update did not maintain the kept copy (step %d)" % step
        assert same_bits(kept, p.detach().to(torch.bfloat16)), step
    # a write the version counter sees: the copy is taken fresh
    with torch.no_grad():
        p.mul_(1.5)
    assert same_bits(ops.cast_weight_kept(p), p.detach().to(torch.bfloat16))
    # a write it cannot see (what loading a checkpoint through .data is), followed by forget_weight_packs
    p.data.add_(0.25)
    ops.forget_weight_packs([p])
    fresh = ops.cast_weight_kept(p)
    assert same_bits(fresh, p.detach().to(torch.bfloat16))
    for t in (p, wide, bias, fc8):
        t.grad = torch.randn_like(t, memory_format=torch.preserve_format)
    opt.step()
    again = ops.cast_weight_kept(p)
    assert again.data_ptr() == fresh.data_ptr() and same_bits(again, p.detach().to(torch.bfloat16))
    # a parameter no optimizer has claimed is cast inside every forward
    q = torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))
    c1, c2 = ops.cast_weight_kept(q), ops.cast_weight_kept(q)
    assert c1.data_ptr() != c2.data_ptr() and same_bits(c1, c2)


# ---------------------------------------------------------------- the total loss
@pytest.mark.parametrize("B", [1, 2])
def test_total_loss_equals_the_sum_of_the_two(ops, B):
    from dsrg_amd import synthetic as S
    b = S.make_batch(4321 + B, B)
    d = lambda a: torch.from_numpy(a).cuda()                                # noqa: E731
    assert b["logits"].shape[2:] == (41, 41)
    losses, grad, _, total = ops.supervision_step(d(b["logits"]), d(b["images"]), d(b["labels"]), d(b["cues"]), want_total=True)
    assert total.shape == () and total.dtype == torch.float32
    assert same_bits(total, losses.sum())
    assert len(ops.supervision_step(d(b["logits"]), d(b["images"]), d(b["labels"]), d(b["cues"]))) == 3
    t2, l2 = ops.dsrg_supervision_loss(d(b["logits"]).requires_grad_(True), d(b["images"]), d(b["labels"]), d(b["cues"]))
    assert l2.shape == (2,) and same_bits(t2, l2.sum()) and t2.requires_grad and not l2.requires_grad


# ---------------------------------------------------------------- the one-pass gradient sum
class _FedNTimes(torch.autograd.Function):
    """one tensor fed n times; backward returns n different gradients for it: autograd accumulates them"""

    @staticmethod
    def forward(ctx, gs, *xs):
        ctx.gs = gs
        return xs[0].new_zeros(())

    @staticmethod
    def backward(ctx, g):
        return (None,) + tuple(ctx.gs)


def _tie_rich(shape, gen):
    """bf16 values whose float32 sums hit rounding ties (small integers around 256, where bf16 steps by 2) and cancel"""
    v = torch.randint(-300, 301, shape, device="cuda", generator=gen).float()
    v = v * torch.tensor([1.0, 0.5, 2.0 ** -9, 2.0 ** 100], device="cuda")[torch.randint(0, 4, shape, device="cuda", generator=gen)]
    return v.bfloat16().contiguous(memory_format=CL)


@pytest.mark.parametrize("n", [4, 3, 2])
@pytest.mark.parametrize("shape", [(2, 8, 3, 5), (1, 512, 5, 7)])
def test_gradient_sum_equals_autograds_accumulation(ops, shape, n):
    gen = torch.Generator(device="cuda").manual_seed(shape[1] + n)
    gs = [_tie_rich(shape, gen) for _ in range(n)]
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1)                     # noqa: E731  (a view of the channels_last memory)
    flat(gs[1])[::7] = -flat(gs[0])[::7]                                   # exact cancellations
    flat(gs[-1])[:4] = torch.tensor([float("inf"), -float("inf"), NAN, 0.0], device="cuda").bfloat16()
    flat(gs[0])[:4] = torch.tensor([-float("inf"), -float("inf"), 1.0, -0.0], device="cuda").bfloat16()
    leaf = torch.zeros(shape, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    _FedNTimes.apply(gs, *([leaf] * n)).backward()
    got = ops.sum_bf16(gs)
    assert got.stride() == gs[0].stride() and same_bits(got, leaf.grad)
    chain = gs[0]
    for g in gs[1:]:
        chain = chain + g                                                    # bf16 adds: float32 sum, one rounding each
    assert same_bits(got, chain)


def test_fc6_gradient_sum_through_the_net(ops):
    """VGG16ASPP, B = 1 on 65 x 65, train mode, fixed dropout seed: the gradient of pool5a's output with the four fc6_k fed one
    tensor (the node sums their data gradients in one pass) against the node fed four separate clones, whose four gradients are
    added in order in bf16 — plain autograd accumulation.  (The 9 x 9 map is below the tile count at which the net groups the
    fc6_k into one node, so the threshold is lowered for the test.)"""
    from dsrg_amd import backbone
    torch.manual_seed(0)
    net = backbone.VGG16ASPP(dropout=0.5).cuda().to(memory_format=CL).train()
    x = torch.randn(1, 3, 65, 65, device="cuda")
    old = backbone._IGEMM_MIN_TILES
    try:
        backbone._IGEMM_MIN_TILES = 0
        got = {}
        hook = net.features.register_forward_hook(lambda m, i, o: (o.retain_grad(), got.__setitem__("f", o))[0])
        torch.manual_seed(123)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net(x.contiguous(memory_format=CL))
        hook.remove()
        gy = torch.randn(y.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        y.backward(gy)
        f = got["f"]
        assert f.dtype == torch.bfloat16 and f.grad is not None
        # the same tail of the net on four clones of f: the grouped fc6_k node, the fc7_k node, the classifiers
        fs = [f.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for _ in range(4)]
        fc6, fc7 = [br[0] for br in net.branches], [br[3] for br in net.branches]
        heads = [br[-1] for br in net.branches]
        torch.manual_seed(123)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            links = [backbone._GradLink() for _ in range(4)]
            hs = list(backbone._IgemmConvFn.apply(3, [m.dilation[0] for m in fc6], True, 0.5, None, 4, None, links, *fs,
                                                  *[m.weight for m in fc6], *[m.bias for m in fc6]))
            links7 = [backbone._GradLink() for _ in range(4)]
            hs = list(backbone._IgemmConvFn.apply(1, [1] * 4, True, 0.5, None, 4, links, links7, *hs, *[m.weight for m in fc7],
                                                  *[m.bias for m in fc7]))
            y2 = backbone._HeadsPtrFn.apply(links7, 4, *[m.weight for m in heads], *[m.bias for m in heads], *hs)
        assert same_bits(y2, y)
        y2.backward(gy)
    finally:
        backbone._IGEMM_MIN_TILES = old
    want = fs[0].grad
    for t in fs[1:]:
        want = want + t.grad
    assert want.dtype == torch.bfloat16 and same_bits(f.grad, want)
