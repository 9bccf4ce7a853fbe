"""ops.py's two launch contracts: per-stream scratch (_stream_scratch) and deferred bias-gradient reductions (deferred_reductions:
every recording op takes its scratch from _reduction_scratch and its destination from _bias_grad_dest, which keep both alive until
the flush) — and the `want=` parsing the multiscale / train-gt front ends share."""
import pytest
import torch

gpu = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


def _bf16(gen, *shape, relu=False):
    t = torch.randn(*shape, device="cuda", generator=gen)
    return (torch.relu(t) if relu else t).bfloat16().contiguous(memory_format=CL)


def _igemm_dgrad_case(ops, gen, cf, cb, dils):
    """the igemm data gradient at (B,H,W) = (1,20,23): gradients of cf channels, masks / results of cb channels"""
    n = len(dils)
    gs = [_bf16(gen, 1, cf, 20, 23) for _ in range(n)]
    packs = [ops.pack_conv_weight(torch.randn(cf, cb, 3, 3, device="cuda", generator=gen) * 0.02, for_dgrad=True) for _ in range(n)]
    ys = [_bf16(gen, 1, cb, 20, 23, relu=True) for _ in range(n)]

    def call():
        outs, gbs = ops.conv_igemm_dgrad(gs, packs, ys, dils, 3, 2.0)
        return outs, gbs
    return call


@pytest.fixture(scope="module")
def recording_ops(ops):
    """the seven ops that record a reduction inside deferred_reductions(): name -> (call, reference), call() -> (other outputs,
    bias gradients) as two lists of tensors; reference = one call outside a block, computed once and left alone"""
    gen = torch.Generator(device="cuda").manual_seed(31)
    g, y = _bf16(gen, 2, 64, 9, 11), _bf16(gen, 2, 64, 9, 11, relu=True)
    pooled, code = ops.maxpool3x3_fwd(y, 2, True)
    go = _bf16(gen, *pooled.shape)
    gd, wt, yd = _bf16(gen, 1, 64, 8, 16), (torch.randn(64, 64, 3, 3, device="cuda", generator=gen) * 0.05).bfloat16(), \
        _bf16(gen, 1, 64, 8, 16, relu=True)
    xb, gb_ = _bf16(gen, 1, 512, 13, 17, relu=True), _bf16(gen, 1, 256, 13, 17)
    pd = ops.pack_conv_weight(torch.randn(256, 512, 3, 3, device="cuda", generator=gen) * 0.03, for_dgrad=True)
    xs = [_bf16(gen, 1, 256, 5, 7, relu=True) for _ in range(2)]
    wh, gh = torch.randn(2, 32, 256, device="cuda", generator=gen) * 0.05, torch.randn(1, 32, 5, 7, device="cuda", generator=gen)

    def one(fn):                                       # (output, bias gradient) -> ([output], [bias gradient])
        return lambda: (lambda r: ([r[0]], [r[1]]))(fn())

    def backward():
        gx, gw, gb = ops.conv_igemm_backward(gb_, pd, xb, 2, xb, 2.0)
        return [gx, gw], [gb]

    def heads():
        gx, gw, gb = ops.heads_backward(xs, wh, gh, True, 2.0)
        return list(gx) + [gw], [gb]

    calls = {
        "relu_bwd_bias": one(lambda: ops.relu_bwd_bias(g, y)),
        "bias_grad": lambda: ([], [ops.bias_grad(g)]),
        "maxpool3x3_bwd_relu": one(lambda: ops.maxpool3x3_bwd_relu(go, code, y, 2)),
        "conv3x3_direct_dgrad": one(lambda: ops.conv3x3_direct_dgrad(gd, wt, yd)),
        "conv_igemm_dgrad": _igemm_dgrad_case(ops, gen, 512, 256, [1, 3]),
        "conv_igemm_backward": backward,
        "heads_backward": heads,
    }
    return {name: (call, call()) for name, call in calls.items()}


_RECORDING = ("relu_bwd_bias", "bias_grad", "maxpool3x3_bwd_relu", "conv3x3_direct_dgrad", "conv_igemm_dgrad", "conv_igemm_backward",
              "heads_backward")


@gpu
@pytest.mark.parametrize("name", _RECORDING)
def test_recording_op_gives_the_same_bits_inside_a_deferral_block(ops, recording_ops, name):
    """a call inside deferred_reductions(), read after the block == the same call outside: every output, bit for bit"""
    call, (want_outs, want_gbs) = recording_ops[name]
    with ops.deferred_reductions():
        outs, gbs = call()
    assert len(outs) == len(want_outs) and len(gbs) == len(want_gbs) >= 1
    for a, b in zip(list(outs) + list(gbs), list(want_outs) + list(want_gbs)):
        assert a.shape == b.shape and torch.equal(a, b), name


@gpu
def test_deferred_destinations_outlive_their_tensors(ops, recording_ops):
    """bias gradients dropped inside a block (a frozen bias, a declined _GradLink, a hook's clone): the flush still writes them, so
    their memory must not go back to the allocator before it — tensors of the same sizes allocated behind them keep their values —
    and after the block the module holds nothing"""
    sentinel = 12345.0
    with ops.deferred_reductions():
        sizes = []
        for name in _RECORDING:
            outs, gbs = recording_ops[name][0]()
            sizes += [tuple(gb.shape) for gb in gbs]
            del gbs
        assert ops._defer[0] and len(ops._defer_keep) >= 2 * len(_RECORDING)
        guards = [torch.full(s, sentinel, dtype=torch.float32, device="cuda") for s in sizes]
    torch.cuda.synchronize()
    assert len(guards) == 8
    for t in guards:
        assert bool((t == sentinel).all()), tuple(t.shape)
    assert not ops._defer[0] and not ops._defer_keep


@gpu
def test_a_launch_records_its_groups_all_or_none(ops):
    """46 recorded sums leave two of the library's 48 entries: a four-group data gradient behind them records none of its column sums
    and runs them at once — no error, the same bits as outside a block, and the 46 are right too"""
    gen = torch.Generator(device="cuda").manual_seed(37)
    g = _bf16(gen, 2, 64, 9, 11)
    dgrad = _igemm_dgrad_case(ops, gen, 256, 256, [1, 3, 1, 3])
    want_sum = ops.bias_grad(g).clone()
    want_outs, want_gbs = dgrad()
    with ops.deferred_reductions():
        sums = [ops.bias_grad(g) for _ in range(46)]
        outs, gbs = dgrad()
    assert len(outs) == len(gbs) == 4
    for a, b in zip(list(outs) + list(gbs), list(want_outs) + list(want_gbs)):
        assert torch.equal(a, b)
    assert all(torch.equal(s, want_sum) for s in sums)
    ref = g.float().sum((0, 2, 3))
    assert (want_sum - ref).abs().max() <= 1e-4 * g.float().abs().sum((0, 2, 3)).max()


@gpu
def test_stream_scratch_identity(ops):
    """one buffer per (kind, device, stream), replaced only when too small; the stream-K buffer of a stream survives its launches"""
    dev = torch.device("cuda", torch.cuda.current_device())
    kind = "test_stream_scratch_identity"
    try:
        a = ops._stream_scratch(kind, dev, 1024)
        assert a.dtype == torch.uint8 and a.numel() >= 1024 and ops._stream_scratch(kind, dev, 512) is a
        big = ops._stream_scratch(kind, dev, 4096)
        assert big.numel() >= 4096 and ops._stream_scratch(kind, dev, 1024) is big
        assert ops._stream_scratch(kind + "2", dev, 1024) is not big
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = ops._stream_scratch(kind, dev, 1024)
            assert ops._stream_scratch(kind, dev, 1024) is other
        assert other is not big and other.data_ptr() != big.data_ptr()
        assert ops._stream_scratch(kind, dev, 1024) is big
    finally:
        for key in [k for k in ops._scratch if k[0].startswith(kind)]:
            del ops._scratch[key]
    # partial rows: the per-stream buffer outside a block, a held tensor of the launch's own inside
    rows = ops._reduction_scratch(dev, 4 * 512 * 64, "rows")
    assert ops._reduction_scratch(dev, 4 * 512 * 64, "rows") is rows and rows.view(torch.float32).numel() >= 512 * 64
    with ops.deferred_reductions():
        own = ops._reduction_scratch(dev, 4 * 512 * 64, "rows")
        assert own is not rows and own.data_ptr() != rows.data_ptr() and any(t is own for t in ops._defer_keep)
    assert not ops._defer_keep
    # stream-K: the same object before and after a launch that uses it, which conv_igemm_stream_k_status then reads
    gen = torch.Generator(device="cuda").manual_seed(41)
    x = _bf16(gen, 1, 64, 5, 7)
    packed = ops.pack_conv_weight(torch.randn(256, 64, 3, 3, device="cuda", generator=gen) * 0.05)
    before = ops._igemm_sk_workspace(dev)
    ops.set_igemm_variant(4)                         # stream-K wherever legal
    try:
        ops.conv_igemm([x], [packed], [None], [1], 3, True, stream_k=True)
        assert ops.conv_igemm_stream_k_status() == 0
    finally:
        ops.set_igemm_variant(-1)
    assert ops._igemm_sk_workspace(dev) is before


@pytest.mark.parametrize("fn,allowed,accepted", [
    ("multiscale_unary", "unary, argmax, sum", "no score maps"),
    ("multiscale_unary_batch", "unary, argmax, sum", "no score maps"),
    ("train_gt_unary_batch", "unary, probs, labels", "scores must be one (Gcap, C, h, w) tensor"),
])
def test_want_argument_validation_messages(fn, allowed, accepted):
    """the shared `want=` parsing: unknown names and an empty selection are refused with the functions' own words, before anything
    touches a device; a string or a sequence of allowed names passes on to the next argument check (no score maps given here)"""
    from dsrg_amd import ops
    names = allowed.split(", ")
    other = {"unary, argmax, sum": "probs", "unary, probs, labels": "sum"}[allowed]

    def call(want):
        if fn == "multiscale_unary":
            return ops.multiscale_unary([], 8, 8, want=want)
        if fn == "multiscale_unary_batch":
            return ops.multiscale_unary_batch([], [(8, 8)], want=want)
        return ops.train_gt_unary_batch(None, [(8, 8)], want=want)

    def message(want):
        with pytest.raises(ValueError) as e:
            call(want)
        return str(e.value)

    for bad in (other, "Unary", ""):
        assert message(bad) == "unknown output %r (choose from %s)" % (bad, allowed)
        assert message((names[0], bad)) == "unknown output %r (choose from %s)" % (bad, allowed)
    assert message(()) == "want names no output" and message([]) == "want names no output"
    for good in names + [tuple(names), list(reversed(names)), (names[1], names[1])]:
        assert message(good) == accepted
    assert ops._want_names(names[2], tuple(names)) == ((names[2],), True)
    assert ops._want_names(list(names), tuple(names)) == (tuple(names), False)
