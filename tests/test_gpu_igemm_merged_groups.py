"""The backward of the four ASPP branches as ONE grid (ops.conv_igemm_backward_groups; csrc/conv_igemm.hip: the grouped data
gradient's tiles and the grouped weight gradient's workgroups in conv_igemm_bwd_kernel, planned by merged_groups_plan), on the
smallest shapes where the grid logic can go wrong:

  fc7 form: 4 groups, 1x1, 256 -> 256, masks (the layers' inputs), mask scale 2.0 and bias gradients in the data gradient's store;
            B = 2 at 9 x 11 (a single ragged tile per group) and at 26 x 29 (six tiles, the last one ragged)
  fc6 form: 4 groups, 3x3, 256 -> 256, dilations 6 / 12 / 18 / 24 (XCD-interleaved class-ordered tiles; the weight gradient's
            per-tap work list); B = 2 at 26 x 29 (unequal split counts) and at 13 x 17 (eight taps of dilation 24 reach nothing)

Operands are exact integers as in test_gpu_exact_conv.py / test_gpu_igemm_wgrad_splits.py: every product and partial sum is an
integer below 2^24, so every fp32 accumulation is exact whatever its order, the float64 CPU gradient IS the value, a float32
result equals it and a bf16 result is its round-to-nearest-even.  Every output is handed in filled with NaN.  Every case asserts
through the plan query that it really runs the merged grid."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
CL = torch.channels_last
LIMIT = float(2 ** 24)
F64 = torch.float64
DILS6 = (6, 12, 18, 24)
NO_MERGE = 4              # a debug variant without the merged backward; the halves of a backward never take its stream-K

#        form   B  H   W   k  dilations
SHAPES = [("fc7", 2, 9, 11, 1, (1, 1, 1, 1)), ("fc7", 2, 26, 29, 1, (1, 1, 1, 1)),
          ("fc6", 2, 26, 29, 3, DILS6), ("fc6", 2, 13, 17, 3, DILS6)]
C = 256
SCALE = 2.0


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


def _ints(shape, r, gen, cl=True):
    t = torch.randint(-r, r + 1, tuple(shape), generator=gen).to(F64)
    return t.contiguous(memory_format=CL) if cl else t


def _grads64(x, w, g, d, k):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    F.conv2d(x, w, None, padding=d * (k // 2), dilation=d).backward(g)
    return x.grad, w.grad


def _bf16(t):
    """round-to-nearest-even to bf16, as float64"""
    r = t.float()
    assert torch.equal(r.to(F64), t), "not exact in float32"
    return r.bfloat16().to(F64)


_cases = {}


def _case(shape):
    """-> dict of float64 operands and expected results per group, computed once per shape and never written to"""
    if shape not in _cases:
        form, B, H, W, k, dils = shape
        gen = torch.Generator().manual_seed(31)
        r = 8 if B * H * W >= 400 else 32
        xs = [_ints((B, C, H, W), r, gen) for _ in dils]
        gs = [_ints((B, C, H, W), r, gen) for _ in dils]
        ws = [_ints((C, C, k, k), 2, gen, cl=False) for _ in dils]
        gxs, gws, gbs = [], [], []
        for x, g, w, d in zip(xs, gs, ws, dils):
            ax, aw = _grads64(x.abs(), w.abs(), g.abs(), d, k)
            assert float(ax.max()) * SCALE < LIMIT and float(aw.max()) < LIMIT, "inputs too large for exact fp32 sums"
            gx, gw = _grads64(x, w, g, d, k)
            if form == "fc7":       # the layer's input is a ReLU (+ Dropout) output: kept where it is positive, times the Dropout scale
                gx = torch.where(x > 0, _bf16(gx * SCALE), torch.zeros_like(gx))
                gb = gx.sum((0, 2, 3))
                assert float(gx.abs().sum((0, 2, 3)).max()) < LIMIT
                gbs.append(gb)
            else:
                gx = _bf16(gx)
            gxs.append(gx); gws.append(gw)
        low = torch.cat([v.reshape(-1) for v in gws]).float().contiguous().view(torch.int32).bitwise_and(0xFFFF)
        assert float((low != 0).float().mean()) >= 0.10, "the weight gradients' low bits are not under test"
        _cases[shape] = dict(xs=xs, gs=gs, ws=ws, gxs=gxs, gws=gws, gbs=gbs)
    return _cases[shape]


def _dev(t, cl=True):
    d = t.to(torch.bfloat16)
    assert torch.equal(d.to(F64), t), "operand not representable in bf16"
    return d.cuda().contiguous(memory_format=CL) if cl else d.cuda()


def _same(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    assert not torch.isnan(got.float()).any(), "%s: an element nobody wrote" % what
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i.tolist())]), float(want[tuple(i.tolist())])) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ; first (index, got, want): %s" % (what, bad.shape[0], want.numel(), first))


def _nan(shape, dtype, cl=True):
    t = torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")
    return t.contiguous(memory_format=CL) if cl else t


def _operands(ops, shape):
    form, B, H, W, k, dils = shape
    c = _case(shape)
    xd, gd = [_dev(x) for x in c["xs"]], [_dev(g) for g in c["gs"]]
    pd = [ops.pack_conv_weight(_dev(w, cl=False).float(), for_dgrad=True) for w in c["ws"]]
    return c, xd, gd, pd


def _backward(ops, shape, xd, gd, pd, **kw):
    form, B, H, W, k, dils = shape
    n = len(dils)
    outs = dict(gx_outs=[_nan((B, C, H, W), torch.bfloat16) for _ in range(n)], gw_outs=[_nan((C, C, k, k), torch.float32) for _ in range(n)])
    if form == "fc7":
        outs["gb_outs"] = [_nan((C,), torch.float32, cl=False) for _ in range(n)]
    gxs, gws, gbs = ops.conv_igemm_backward_groups(gd, pd, xd, dils, k, xd if form == "fc7" else None, SCALE if form == "fc7" else 1.0,
                                                   **outs, **kw)
    for got, out in zip(list(gxs) + list(gws) + list(gbs or []), outs["gx_outs"] + outs["gw_outs"] + outs.get("gb_outs", [])):
        assert got.data_ptr() == out.data_ptr(), "a result did not land in the tensor that was handed in"
    return gxs, gws, gbs


def _alone_split(ops, shape):
    """the uniform split of the weight gradient launched alone (fc7 form), or 0 (fc6 form: a work list either way)"""
    form, B, H, W, k, dils = shape
    if form == "fc6":
        return 0
    counts = {c for grp in ops.conv_igemm_wgrad_splits(len(dils), B, H, W, C, C, k, dils) for c in grp}
    assert len(counts) == 1
    return counts.pop()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_takes_the_merged_grid(ops, shape):
    form, B, H, W, k, dils = shape
    plan = ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, with_mask=form == "fc7")
    assert plan["merged"] and plan["nd"] >= 4 and plan["nw"] >= 4, plan
    assert plan["merged_us"] <= plan["separate_us"], plan
    assert (plan["ksplit"] == 0) == (form == "fc6"), plan                                # fc6: the weight gradient keeps its work list
    forced = ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, form == "fc7", _alone_split(ops, shape), 2)
    assert forced["merged"] and forced["w_first"] and forced["ksplit"] == _alone_split(ops, shape), forced
    if form == "fc6":
        assert plan["nd"] % 8 == 0 and plan["nw"] % 8 == 0, plan                         # both XCD-interleaved maps: whole rows of 8 blocks
        splits = ops.conv_igemm_wgrad_splits(4, B, H, W, C, C, 3, dils)
        assert len({c for grp in splits for c in grp}) >= 2, splits                      # ... of unequal length
    ops.set_igemm_variant(NO_MERGE)
    try:
        assert not ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, with_mask=form == "fc7")["merged"]
    finally:
        ops.set_igemm_variant(-1)


@gpu
@pytest.mark.parametrize("order", [1, 2], ids=["d_first", "w_first"])
@pytest.mark.parametrize("shape", SHAPES)
def test_merged_grid_is_the_float64_gradient_and_the_separate_launches_bit_for_bit(ops, shape, order):
    form, B, H, W, k, dils = shape
    c, xd, gd, pd = _operands(ops, shape)
    ks = _alone_split(ops, shape)
    plan = ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, form == "fc7", ks, order)
    assert plan["merged"] and plan["w_first"] == (order == 2) and plan["ksplit"] == ks, plan
    gxs, gws, gbs = _backward(ops, shape, xd, gd, pd, force_ksplit=ks, force_order=order)
    # the separate launches
    if form == "fc7":
        dx, db = ops.conv_igemm_dgrad(gd, pd, xd, dils, k, SCALE)
    else:
        dx, db = ops.conv_igemm(gd, pd, None, dils, k, False, stream_k=False), None
    dw = ops.conv_igemm_wgrad(xd, gd, dils, k)
    for i, d in enumerate(dils):
        _same(gxs[i], c["gxs"][i].to(torch.bfloat16).contiguous(memory_format=CL), "data gradient %d against float64" % i)
        _same(gws[i], c["gws"][i].float().contiguous(memory_format=CL), "weight gradient %d against float64" % i)
        _same(gxs[i], dx[i], "data gradient %d against the launch alone" % i)
        _same(gws[i], dw[i], "weight gradient %d against the launch alone" % i)
        if form == "fc7":
            _same(gbs[i], c["gbs"][i].float(), "bias gradient %d against float64" % i)
            _same(gbs[i], db[i], "bias gradient %d against the launch alone" % i)
    if form == "fc7":            # another uniform split than the launch alone runs (forced): exact data does not see the order
        other = 1 if ks > 1 else 2
        assert ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, True, other, order)["ksplit"] == other
        _, gws1, _ = _backward(ops, shape, xd, gd, pd, force_ksplit=other, force_order=order)
        for i in range(len(dils)):
            _same(gws1[i], c["gws"][i].float().contiguous(memory_format=CL), "weight gradient %d on %d split(s) against float64" % (i, other))
    if form == "fc6" and (H, W) == (13, 17):
        dead = gws[3].cpu().flatten(2)[:, :, [0, 1, 2, 3, 5, 6, 7, 8]]
        assert torch.equal(dead, torch.zeros_like(dead)) and not torch.signbit(dead).any()       # taps that reach nothing: exact zeros


def _random_operands(ops, shape, seed):
    form, B, H, W, k, dils = shape
    torch.manual_seed(seed)
    xd = [torch.randn(B, C, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in dils]
    gd = [torch.randn(B, C, H, W, device="cuda").bfloat16().contiguous(memory_format=CL) for _ in dils]
    pd = [ops.pack_conv_weight(torch.randn(C, C, k, k, device="cuda") * 0.05, for_dgrad=True) for _ in dils]
    return xd, gd, pd


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_random_data_planner_choice_repeats_and_matches_the_two_launch_variant(ops, shape):
    """the planner's own split and order on data whose sums DO depend on their order: two calls give the same bits, the variant
    without the merged grid (the same prepared halves as two launches — with the split forced to the merged grid's where the
    planner cut the pixels differently for it) gives the same bits, data and bias gradients are those of the launches alone"""
    form, B, H, W, k, dils = shape
    xd, gd, pd = _random_operands(ops, shape, 37)
    plan = ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, with_mask=form == "fc7")
    assert plan["merged"], plan
    first = _backward(ops, shape, xd, gd, pd)
    again = _backward(ops, shape, xd, gd, pd)
    ops.set_igemm_variant(NO_MERGE)
    try:
        assert not ops.conv_igemm_backward_groups_plan(len(dils), B, H, W, C, C, k, dils, form == "fc7", plan["ksplit"])["merged"]
        two = _backward(ops, shape, xd, gd, pd, force_ksplit=plan["ksplit"])
    finally:
        ops.set_igemm_variant(-1)
    if form == "fc7":
        dx, db = ops.conv_igemm_dgrad(gd, pd, xd, dils, k, SCALE)
    else:
        dx, db = ops.conv_igemm(gd, pd, None, dils, k, False, stream_k=False), None
    dw = ops.conv_igemm_wgrad(xd, gd, dils, k)
    for i in range(len(dils)):
        for a, b in zip(first, again):
            if a is not None:
                _same(a[i], b[i], "two identical calls, group %d" % i)
        for a, b in zip(first, two):
            if a is not None:
                _same(a[i], b[i], "merged grid against two launches, group %d" % i)
        _same(first[0][i], dx[i], "data gradient %d against the launch alone" % i)
        if form == "fc7":
            _same(first[2][i], db[i], "bias gradient %d against the launch alone" % i)
        if plan["ksplit"] == _alone_split(ops, shape):
            _same(first[1][i], dw[i], "weight gradient %d against the launch alone" % i)
        else:                                                                            # another pixel split: another fp32 summation order
            assert (first[1][i] - dw[i]).abs().max() <= 1e-4 * dw[i].abs().max(), i


@gpu
def test_the_aspp_nodes_of_vgg16aspp_give_the_same_gradients_with_and_without_the_merged_grid(ops):
    """VGG16ASPP's own fc6_k / fc7_k nodes (train mode: Dropout masks in both) on a 21 x 21 map, the trunk replaced by the identity:
    .grad of the eight kernels and the gradient of the map, backward under the default variant against backward under the variant
    without the merged grid.  The forward runs under the default variant both times"""
    from dsrg_amd.backbone import VGG16ASPP
    B, H, W = 2, 21, 21
    for cin, cout, k, dils, mask in ((512, 1024, 3, DILS6, False), (1024, 1024, 1, (1, 1, 1, 1), True)):
        assert ops.conv_igemm_backward_groups_plan(4, B, H, W, cin, cout, k, dils, with_mask=mask)["merged"]
    torch.manual_seed(41)
    net = VGG16ASPP().cuda().train()
    net.features = torch.nn.Identity()
    f0 = torch.randn(B, 512, H, W, device="cuda").relu().bfloat16().contiguous(memory_format=CL)
    r = torch.randn(B, 21, H, W, device="cuda")
    kernels = [br[i].weight for br in net.branches for i in (0, 3)]

    def run(variant):
        for p in net.parameters():
            p.grad = None
        f = f0.clone().requires_grad_(True)
        torch.manual_seed(43)                                  # the Dropout seeds come from torch's CPU generator
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(f)
        ops.set_igemm_variant(variant)
        try:
            (out.float() * r).sum().backward()
        finally:
            ops.set_igemm_variant(-1)
        torch.cuda.synchronize()
        return [w.grad.clone() for w in kernels] + [f.grad.clone()]

    merged, two = run(-1), run(NO_MERGE)
    assert len(merged) == 9
    # fc7_k's weight gradient runs a uniform pixel split, which the planner may cut differently for the merged grid: then the two
    # forms add the same products in another order (everything else is bit for bit either way)
    same_split = ops.conv_igemm_backward_groups_plan(4, B, H, W, 1024, 1024, 1, (1, 1, 1, 1), with_mask=True)["ksplit"] == \
        ops.conv_igemm_wgrad_splits(4, B, H, W, 1024, 1024, 1, (1, 1, 1, 1))[0][0]
    for i, (a, b) in enumerate(zip(merged, two)):
        assert float(a.float().abs().max()) > 0.0, i
        if i < 8 and i % 2 == 1 and not same_split:
            assert (a - b).abs().max() <= 1e-4 * b.abs().max(), i
        else:
            _same(a, b, "gradient %d (kernels of fc6_k / fc7_k per branch, then the map)" % i)
