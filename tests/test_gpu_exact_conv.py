"""The convolution kernels of the backbone (csrc/conv_igemm.hip, csrc/conv_direct.hip, the fc8 heads and the ASPP shifts of
csrc/backbone_ops.hip) bit for bit, on exact data.

Operands are integers (or multiples of one power of two, the "quantum") small enough that every product and every partial sum
of a kernel, in whatever order it adds them, is a multiple of the quantum below 2^24 quanta: every fp32 accumulation is exact,
the float64 CPU convolution of the same operands IS the fp32 accumulator value, a float32 output must equal it and a bf16
output must be its round-to-nearest-even.  No tolerance anywhere; a failure names the element.

Every case asserts, on its own data,
  * the exactness bound (`_bounded`): the same operation on |x|, |w|, |bias|, in quanta, stays below 2^24 — a condition on the
    inputs, not a measurement of the kernel;
  * where a bf16 result comes from full windows, non-vacuity (`_nonvacuous`, through `_rounded` on every expected tensor): at
    least 10 % of the values that get rounded in that comparison are not bf16-representable and at least one is an exact tie —
    otherwise "rounds to nearest even" is not being tested.
Default ranges: x, g in [-8, 8], w in [-4, 4], bias in [-64, 64].  Where a sum has too few terms to leave bf16's 8 bits the
default ranges miss the 10 % (share of unrepresentable values on the CPU: 0.0002 for a 3-channel 3x3 input, 0.007 for a
64-channel 1x1, 0.02 for a weight gradient over 35 pixels), so there the ranges are widened — fewer than 500 terms per output:
x to [-64, 64], w to [-16, 16]; a weight gradient over fewer than 400 pixels: x, g to [-32, 32] — still far inside the bound.
The rule looks at the number of terms of the sum only, not at what a kernel returns."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
CL = torch.channels_last
LIMIT = float(2 ** 24)
F64 = torch.float64


# ---- data ------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, gen):
    """integer-valued float64 tensor, uniform in [lo, hi]; 4-d tensors are channels_last"""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(F64)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t


def _relu_out(shape, hi, gen):
    """what a ReLU leaves: integers in [1, hi] with about half the elements zero, every 97th element (memory order) -0.0 —
    a -0.0 counts as "off", like +0.0"""
    t = (_ints(shape, 1, hi, gen) * (torch.rand(tuple(shape), generator=gen) < 0.5).to(F64)).contiguous(memory_format=CL)
    t.permute(0, 2, 3, 1).view(-1)[::97] = -0.0
    return t


def _wide(shape, bits, quantum, gen, ties=False):
    """+-m * quantum, m odd and uniform in [2^(bits-1), 2^bits): exactly `bits` significant bits.  ties: every third value is made
    an exact bf16 tie instead (nine significant bits: the ninth set, nothing below it)"""
    m = torch.randint(2 ** (bits - 1), 2 ** bits, tuple(shape), generator=gen) | 1
    if ties:
        low = 2 ** (bits - 8)
        m.view(-1)[::3] = m.view(-1)[::3] // low * low + low // 2
    s = torch.randint(0, 2, tuple(shape), generator=gen) * 2 - 1
    return (m * s).to(F64) * quantum


def _dev(t, dtype=torch.bfloat16):
    """to the GPU; the cast must be exact (the data generators' promise)"""
    d = t.to(dtype)
    assert torch.equal(d.to(F64), t), "operand not representable in %s" % dtype
    d = d.cuda()
    return d.contiguous(memory_format=CL) if d.dim() == 4 and dtype == torch.bfloat16 else d.contiguous()


# ---- references (float64, CPU) ---------------------------------------------------------------------------------------------
def _conv64(x, w, b, dil):
    k = w.shape[2]
    return F.conv2d(x, w, b, padding=dil * (k // 2), dilation=dil)


def _dgrad64(g, w, dil, hw):
    """autograd through the float64 convolution: d/dx of <conv(x, w), g>"""
    x = torch.zeros(g.shape[0], w.shape[1], hw[0], hw[1], dtype=F64, requires_grad=True)
    _conv64(x, w, None, dil).backward(g)
    return x.grad


def _wgrad64(x, g, k, dil):
    w = torch.zeros(g.shape[1], x.shape[1], k, k, dtype=F64, requires_grad=True)
    _conv64(x, w, None, dil).backward(g)
    return w.grad


def _bounded(absmax, quantum=1.0):
    """the exactness bound: `absmax` = max of the operation on the operands' absolute values"""
    assert float(absmax) / quantum < LIMIT, "inputs too large for exact fp32 sums: %g quanta" % (float(absmax) / quantum)


def _f32(ref):
    r = ref.float()
    assert torch.equal(r.to(F64), ref), "reference not exact in float32 (the bound should have caught it)"
    return r


def _bf16(ref):
    return _f32(ref).bfloat16()


def _nonvacuous(rounded, what=""):
    """`rounded`: the float64 values a kernel rounds to bf16 (those of live elements)"""
    low = _f32(rounded).contiguous().view(torch.int32).bitwise_and(0xFFFF)
    share, ties = float((low != 0).float().mean()), int((low == 0x8000).sum())
    assert share >= 0.10 and ties >= 1, "%s: %.3f of the values need rounding, %d ties: the rounding is not under test" % (what, share, ties)
    return share, ties


def _split_live(t, terms, what):
    """the float32 operand a heads kernel splits into three bf16 terms (t0 = bf16(t), t1 = bf16(t - t0), t2 = bf16(t - t0 - t1)):
    each of the first `terms` terms is non-zero in at least a quarter of the non-zero values of t"""
    r = _f32(t)[t != 0]
    for i in range(terms):
        term = r.bfloat16().float()
        share = float((term != 0).float().mean())
        assert share >= 0.25, "%s: split term %d is non-zero in only %.3f of the values: it is not under test" % (what, i, share)
        r = r - term


def _same(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i.tolist())]), float(want[tuple(i.tolist())])) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ; first (index, got, want): %s" % (what, bad.shape[0], want.numel(), first))


def _ends(n):
    """the first and the last 64 channels"""
    return list(range(n)) if n <= 128 else list(range(64)) + list(range(n - 64, n))


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


class _variant(object):
    def __init__(self, ops, v):
        self.ops, self.v = ops, v

    def __enter__(self):
        self.ops.set_igemm_variant(self.v)

    def __exit__(self, *exc):
        self.ops.set_igemm_variant(-1)


# ---- case builders: data, reference and the two input conditions, all on the CPU --------------------------------------------
def _fwd_case(B, H, W, cin, cout, k, dil, seed, img=None, full_window=True):
    """-> x, w, bias (float64) and ref = conv(x, w) WITHOUT bias on the compared slice (image `img` only, channels _ends(cout),
    when img is given), the slice, and whether the windows are full (non-vacuity is then asserted by _rounded on every
    expected bf16 tensor made from ref)"""
    gen = _gen(seed)
    xr, wr = (64, 16) if cin * k * k < 500 else (8, 4)     # few terms per sum: wider operands, so that sums leave bf16's 8 bits
    x, w, b = _ints((B, cin, H, W), -xr, xr, gen), _ints((cout, cin, k, k), -wr, wr, gen), _ints((cout,), -64, 64, gen)
    ch = _ends(cout) if img is not None else list(range(cout))
    xs = x[img:img + 1] if img is not None else x
    ref = _conv64(xs, w[ch], None, dil)
    _bounded(_conv64(xs.abs(), w[ch].abs(), b[ch].abs(), dil).max())
    if img is not None:                                   # the elements outside the slice are computed too (stream-K: compared with
        _bounded(x.abs().max() * w.abs().sum((1, 2, 3)).max() + b.abs().max())      # the whole-tile launch): a bound for all
    return x, w, b, ref, (slice(img, img + 1) if img is not None else slice(None), ch)


def _post(ref, bias, relu):
    v = ref + bias.view(1, -1, 1, 1) if bias is not None else ref
    return torch.relu(v) if relu else v


def _rounded(v, full, what, relu=False):
    """the expected bf16 tensor of the float64 values `v`; full windows: non-vacuity asserted on exactly the values that are
    rounded here (behind a ReLU the live ones: a zero needs no rounding)"""
    if full:
        _nonvacuous(v[v > 0] if relu else v, what)
    return _bf16(v)


def _wgrad_case(B, H, W, cin, cout, k, dil, seed, relu_x=False):
    gen = _gen(seed)
    r = 8 if B * H * W >= 400 else 32                     # few pixels: few terms per sum; wider operands so that sums leave 8 bits
    x = _relu_out((B, cin, H, W), r, gen) if relu_x else _ints((B, cin, H, W), -r, r, gen)
    g = _ints((B, cout, H, W), -r, r, gen)
    ref, absmax = _wgrad64(x, g, k, dil), _wgrad64(x.abs(), g.abs(), k, dil).max()
    _bounded(absmax)
    return x, g, ref, absmax


FWD_SHAPES = [                                            # (B, H, W, cin, cout, k, dil, full windows)
    (1, 5, 7, 64, 256, 3, 1, True),                       # one partial tile, every border case
    (1, 5, 7, 64, 256, 3, 9, False),                      # degenerate: only the centre tap is inside the map
    (3, 1, 1, 64, 256, 3, 1, False),                      # degenerate
    (2, 19, 23, 128, 256, 3, 2, True),                    # several tiles, a ragged last one, two channel chunks
    (1, 20, 20, 128, 384, 3, 2, True),                    # one and a half n-tiles
    (2, 27, 31, 256, 128, 3, 1, True),                    # half an n-tile
    (1, 9, 11, 1024, 1024, 1, 1, True),                   # 1x1, sixteen K-steps
    (2, 13, 17, 512, 256, 3, 6, True),                    # dilated: class-ordered tiles
    (1, 4, 4, 64, 64, 3, 1, True),                        # a 64-output launch
]
WGRAD_SHAPES = [                                          # (B, H, W, cin, cout, k, dil)
    (1, 5, 7, 256, 256, 3, 1), (2, 19, 23, 256, 256, 3, 2), (1, 3, 100, 256, 512, 3, 24), (2, 27, 31, 128, 256, 3, 1),
    (2, 37, 35, 256, 64, 1, 1), (2, 37, 35, 64, 256, 1, 1), (2, 33, 35, 128, 128, 3, 1), (1, 29, 31, 64, 128, 3, 2),
    (1, 21, 23, 320, 192, 1, 1),
]
DIRECT_MAPS = [(2, 33, 29), (1, 8, 16), (3, 1, 1), (2, 17, 40)]


# ---- CPU: the generators keep their promises ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FWD_SHAPES[0], FWD_SHAPES[3], FWD_SHAPES[7]])
def test_generated_forward_data_is_exact_and_exercises_the_rounding(shape):
    B, H, W, cin, cout, k, dil, full = shape
    x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, k, dil, 5)             # asserts the bound
    for bias in (None, b):
        for relu in (False, True):                                         # non-vacuity of every expected tensor of the forward tests
            _rounded(_post(ref, bias, relu), full, "bias %d relu %d" % (bias is not None, relu), relu)
    ref = ref + b.view(1, -1, 1, 1)
    assert torch.equal(_conv64(x.float(), w.float(), b.float(), dil).to(F64), ref)      # float32 == float64: every sum exact
    share, ties = _nonvacuous(ref)
    assert share >= 0.10 and ties >= 1
    y = _relu_out((B, cin, H, W), 8, _gen(1))
    flat = y.permute(0, 2, 3, 1).reshape(-1)
    assert torch.signbit(flat[::97]).all() and not (flat[::97] > 0).any() and 0.4 < float((y > 0).float().mean()) < 0.6


@pytest.mark.parametrize("shape", [WGRAD_SHAPES[0], WGRAD_SHAPES[1]])
def test_generated_gradient_data_is_exact_and_exercises_the_rounding(shape):
    B, H, W, cin, cout, k, dil = shape
    x, g, ref, _ = _wgrad_case(B, H, W, cin, cout, k, dil, 9)                 # asserts the bound
    w32 = torch.zeros(cout, cin, k, k, requires_grad=True)
    _conv64(x.float(), w32, None, dil).backward(g.float())
    assert torch.equal(w32.grad.to(F64), ref)
    _nonvacuous(ref, "weight gradient")
    w = _ints((cout, cin, k, k), -4, 4, _gen(3))
    gx = _dgrad64(g, w, dil, (H, W))
    _bounded(_dgrad64(g.abs(), w.abs(), dil, (H, W)).max())
    x32 = torch.zeros(B, cin, H, W, requires_grad=True)
    _conv64(x32, w.float(), None, dil).backward(g.float())
    assert torch.equal(x32.grad.to(F64), gx)
    _nonvacuous(gx, "data gradient")


# ---- 1. conv_igemm forward ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil,full", FWD_SHAPES)
def test_igemm_forward_is_the_rounded_float64_convolution(ops, B, H, W, cin, cout, k, dil, full):
    x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, k, dil, 5, full_window=full)
    xd, pk, bd = _dev(x), ops.pack_conv_weight(_dev(w)), _dev(b, torch.float32)
    for variant in (1, 2, 5, -1):
        with _variant(ops, variant):
            for bias in (False, True):
                for relu in (False, True):
                    (got,) = ops.conv_igemm([xd], [pk], [bd if bias else None], [dil], k, relu, stream_k=False)
                    what = "variant %d bias %d relu %d" % (variant, bias, relu)
                    _same(got, _rounded(_post(ref, b if bias else None, relu), full, what, relu), what)


@gpu
def test_igemm_forward_four_branches_in_one_launch(ops):
    B, H, W, cin, cout, dils = 1, 13, 17, 512, 256, [6, 12, 18, 24]
    cases = [_fwd_case(B, H, W, cin, cout, 3, d, 20 + i) for i, d in enumerate(dils)]
    xs, ws = [_dev(c[0]) for c in cases], [ops.pack_conv_weight(_dev(c[1])) for c in cases]
    bs = [_dev(c[2], torch.float32) for c in cases]
    for variant in (1, 2, 5, -1):
        with _variant(ops, variant):
            got = ops.conv_igemm(xs, ws, bs, dils, 3, True, stream_k=False)
            for i, c in enumerate(cases):
                _same(got[i], _rounded(_post(c[3], c[2], True), True, "branch %d" % i, True), "variant %d branch %d" % (variant, i))
    shared = ops.conv_igemm([xs[0]] * 4, ws, None, dils, 3, False, stream_k=False)          # one input for every branch
    for i, c in enumerate(cases):
        ref = _conv64(cases[0][0], c[1], None, dils[i])
        _bounded(_conv64(cases[0][0].abs(), c[1].abs(), None, dils[i]).max())
        _same(shared[i], _rounded(ref, True, "shared input, branch %d" % i), "shared input, branch %d" % i)


# ---- 2. stream-K -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dils", [
    (16, 41, 41, 512, 512, 3, [2]),
    (16, 41, 41, 512, 256, 3, [1]),
    (4, 41, 41, 512, 1024, 3, [6, 12, 18, 24]),
    (4, 81, 81, 256, 128, 3, [1]),
    (16, 41, 41, 1024, 1024, 1, [1]),
])
def test_igemm_stream_k_is_bit_equal_to_whole_tiles_and_to_float64(ops, B, H, W, cin, cout, k, dils):
    """On exact data the summation order cannot matter: the cut launch == the whole-tile launch, bit for bit, and both == the
    float64 reference (compared on the last image, first and last 64 output channels)"""
    n = len(dils)
    cases = [_fwd_case(B, H, W, cin, cout, k, d, 60 + i, img=B - 1) for i, d in enumerate(dils)]
    xs, ws = [_dev(c[0]) for c in cases], [ops.pack_conv_weight(_dev(c[1])) for c in cases]
    bs = [_dev(c[2], torch.float32) for c in cases]
    for p in (0.0, 0.5):
        whole = ops.conv_igemm(xs, ws, bs, dils, k, True, p, 77, stream_k=False)
        with _variant(ops, 4):                            # stream-K wherever legal
            cut = ops.conv_igemm(xs, ws, bs, dils, k, True, p, 77, stream_k=True)
            assert ops.conv_igemm_stream_k_status() == 0
        for i in range(n):
            assert torch.equal(whole[i], cut[i]), "p %g branch %d: %d elements differ between the cut and the whole-tile launch" % (
                p, i, int((whole[i] != cut[i]).sum()))
            x, w, b, ref, (im, ch) = cases[i]
            want = _post(ref, b[ch], True)
            for tag, t in (("whole", whole[i]), ("cut", cut[i])):
                part = t[im][:, ch]
                if p == 0.0:
                    _same(part, _rounded(want, True, "branch %d" % i, True), "%s, branch %d" % (tag, i))
                else:
                    _dropped(part, want, "%s with dropout, branch %d" % (tag, i))


# ---- 3. fused dropout --------------------------------------------------------------------------------------------------------
def _dropped(got, ref_relu, what):
    """fused Dropout with p = 0.5 (scale 2, exact): every element is 0 or bf16(2 relu(ref)); nothing is kept where the ReLU is
    off; the kept set is the kernel's own, but both kinds must occur"""
    got = got.detach().cpu()
    want = _bf16(2.0 * ref_relu)
    kept = got != 0
    bad = (kept & (got != want)).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i.tolist())]), float(want[tuple(i.tolist())])) for i in bad[:6]]
    assert bad.shape[0] == 0, "%s: %d kept elements are not bf16(2 relu(ref)); first (index, got, want): %s" % (what, bad.shape[0], first)
    on = ref_relu > 0
    assert (kept & on).any() and (~kept & on).any(), what


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil", [(2, 19, 23, 128, 256, 3, 2), (1, 9, 11, 1024, 1024, 1, 1)])
def test_igemm_fused_dropout_keeps_exactly_twice_the_relu(ops, B, H, W, cin, cout, k, dil):
    x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, k, dil, 41)
    xd, pk, bd = _dev(x), ops.pack_conv_weight(_dev(w)), _dev(b, torch.float32)
    _nonvacuous((2.0 * _post(ref, b, True))[ref + b.view(1, -1, 1, 1) > 0], "2 relu(conv + bias)")
    for variant in (1, 2, 5, -1):
        with _variant(ops, variant):
            (got,) = ops.conv_igemm([xd], [pk], [bd], [dil], k, True, 0.5, 1234, stream_k=False)
        _dropped(got, _post(ref, b, True), "variant %d" % variant)


# ---- 4. data gradients -------------------------------------------------------------------------------------------------------
@gpu
def test_igemm_data_gradient_packing_is_the_rounded_float64_gradient(ops):
    B, H, W, cin, cout, dil = 2, 13, 17, 256, 512, 2
    gen = _gen(7)
    g, w = _ints((B, cout, H, W), -8, 8, gen), _ints((cout, cin, 3, 3), -4, 4, gen)
    ref = _dgrad64(g, w, dil, (H, W))
    _bounded(_dgrad64(g.abs(), w.abs(), dil, (H, W)).max())
    _nonvacuous(ref, "data gradient")
    pd = ops.pack_conv_weight(_dev(w), for_dgrad=True)
    for variant in (1, 2, 5, -1):
        with _variant(ops, variant):
            (gx,) = ops.conv_igemm([_dev(g)], [pd], [None], [dil], 3, False, stream_k=False)
        _same(gx, _bf16(ref), "variant %d" % variant)


def _masked(ref, mask, scale):
    """the masked, scaled, once-rounded data gradient and its column sums (the bias gradient of the layer below: the sums of
    what was stored)"""
    want = torch.where(mask > 0, scale * ref, torch.zeros_like(ref))
    stored = _bf16(want)
    _bounded(stored.to(F64).abs().sum((0, 2, 3)).max())
    return stored, _f32(stored.to(F64).sum((0, 2, 3)))


@gpu
@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("B,H,W,cf,cb,k,dils", [
    (1, 33, 29, 256, 256, 3, [2]),                        # ragged pixel tail, dilation
    (1, 20, 23, 512, 256, 3, [1, 3]),
    (1, 9, 11, 1024, 1024, 1, [1, 1, 1, 1]),              # fc7_k -> fc6_k, four branches
])
def test_igemm_dgrad_with_mask_is_the_masked_scaled_rounded_gradient(ops, B, H, W, cf, cb, k, dils, scale):
    n = len(dils)
    gen = _gen(77)
    gs = [_ints((B, cf, H, W), -8, 8, gen) for _ in range(n)]
    ws = [_ints((cf, cb, k, k), -4, 4, gen) for _ in range(n)]
    ys = [_relu_out((B, cb, H, W), 8, gen) for _ in range(n)]
    refs = [_dgrad64(gs[i], ws[i], dils[i], (H, W)) for i in range(n)]
    for i in range(n):
        _bounded(scale * _dgrad64(gs[i].abs(), ws[i].abs(), dils[i], (H, W)).max())
        _nonvacuous((scale * refs[i])[ys[i] > 0], "masked data gradient")
    packs = [ops.pack_conv_weight(_dev(w), for_dgrad=True) for w in ws]
    got, gb = ops.conv_igemm_dgrad([_dev(g) for g in gs], packs, [_dev(y) for y in ys], dils, k, scale)
    for i in range(n):
        stored, sums = _masked(refs[i], ys[i], scale)
        _same(got[i], stored, "gx, branch %d" % i)
        _same(gb[i], sums, "bias gradient, branch %d" % i)


# ---- 5. weight gradients, merged backward, residual forms ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil", WGRAD_SHAPES)
def test_igemm_weight_gradient_is_the_float64_gradient(ops, B, H, W, cin, cout, k, dil):
    x, g, ref, _ = _wgrad_case(B, H, W, cin, cout, k, dil, 9)
    _nonvacuous(ref, "weight gradient")
    xd, gd = _dev(x), _dev(g)
    for variant in (3, 6, 7):
        with _variant(ops, variant):
            (gw,) = ops.conv_igemm_wgrad([xd], [gd], [dil], k)
            (gwb,) = ops.conv_igemm_wgrad([xd], [gd], [dil], k, out_dtype=torch.bfloat16)
        _same(gw, _f32(ref), "variant %d, float32" % variant)
        _same(gwb, _bf16(ref), "variant %d, bf16" % variant)


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,dil,absorb", [
    (1, 20, 23, 256, 512, 1, True),                       # a ragged last tile on both sides
    (2, 19, 23, 128, 256, 1, False),                      # a 128-channel x: two taps per weight-gradient tile
    (1, 13, 17, 512, 256, 2, True),
    (1, 13, 17, 256, 256, 12, False),                     # a dilated layer: two launches behind the entry point
])
def test_igemm_merged_backward_is_exact(ops, B, H, W, cin, cout, dil, absorb):
    x, g, ref_w, _ = _wgrad_case(B, H, W, cin, cout, 3, dil, 13, relu_x=True)
    w = _ints((cout, cin, 3, 3), -4, 4, _gen(14))
    ref_x = _dgrad64(g, w, dil, (H, W))
    scale = 2.0 if absorb else 1.0
    _bounded(scale * _dgrad64(g.abs(), w.abs(), dil, (H, W)).max())
    _nonvacuous((scale * ref_x)[x > 0] if absorb else ref_x, "data gradient")
    xd = _dev(x)
    gx, gw, gb = ops.conv_igemm_backward(_dev(g), ops.pack_conv_weight(_dev(w), for_dgrad=True), xd, dil, xd if absorb else None, scale)
    _same(gw, _f32(ref_w), "gw")
    if absorb:
        stored, sums = _masked(ref_x, x, scale)
        _same(gx, stored, "gx")
        _same(gb, sums, "bias gradient")
    else:
        assert gb is None
        _same(gx, _bf16(ref_x), "gx")


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil", [(1, 13, 17, 256, 512, 1, 1), (1, 13, 17, 256, 256, 3, 2), (1, 9, 11, 512, 256, 3, 4)])
def test_igemm_backward_residual_is_exact(ops, B, H, W, cin, cout, k, dil):
    """gx = mask(bf16(bf16(data gradient) + res)): two roundings; gw = the float64 gradient times a power of two per output"""
    x, g, ref_w, abs_w = _wgrad_case(B, H, W, cin, cout, k, dil, 15, relu_x=True)
    gen = _gen(16)
    w, res = _ints((cout, cin, k, k), -4, 4, gen), _ints((B, cin, H, W), -8, 8, gen)
    sc = 2.0 ** _ints((cout,), -2, 2, gen)
    ref_x = _dgrad64(g, w, dil, (H, W))
    _bounded(_dgrad64(g.abs(), w.abs(), dil, (H, W)).max() + res.abs().max())
    _bounded(4.0 * abs_w, 0.25)                           # the scaled weight gradient: multiples of 1/4, up to 4 |gw|
    first = _rounded(ref_x, True, "data gradient").to(F64)
    _nonvacuous(first + res, "bf16(data gradient) + res")
    _nonvacuous((first + res)[x > 0], "masked bf16(data gradient) + res")
    _nonvacuous(ref_x[x > 0], "masked data gradient")
    xd, gd, pd = _dev(x), _dev(g), ops.pack_conv_weight(_dev(w), for_dgrad=True)
    for mask, r, s in [(True, True, True), (False, True, False), (True, False, True), (False, False, False)]:
        gx, gw = ops.conv_igemm_backward_residual(gd, pd, xd, dil, k, xd if mask else None, _dev(res) if r else None,
                                                  _dev(sc, torch.float32) if s else None)
        want = _bf16(first + res) if r else _bf16(ref_x)
        if mask:
            want = torch.where(x > 0, want, torch.zeros_like(want))
        _same(gx, want, "gx (mask %d, res %d)" % (mask, r))
        _same(gw, _f32(ref_w * sc.view(-1, 1, 1, 1) if s else ref_w), "gw (scale %d)" % s)


@gpu
@pytest.mark.parametrize("B,H,W,cin,cout,k,dil", [(1, 13, 17, 128, 512, 1, 1), (1, 19, 23, 256, 256, 3, 12), (2, 9, 11, 256, 64, 1, 1),
                                                  (1, 10, 9, 64, 64, 1, 1)])
def test_igemm_residual_forward_has_its_two_roundings(ops, B, H, W, cin, cout, k, dil):
    """post(bf16(conv + bias) + res): the sum is rounded, the residual added in fp32, the result rounded again"""
    x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, k, dil, 17)
    gen = _gen(18)
    res, below = _ints((B, cout, H, W), -8, 8, gen), _relu_out((B, cout, H, W), 8, gen)
    _bounded(_conv64(x.abs(), w.abs(), b.abs(), dil).max() + res.abs().max())
    xd, pk, bd, rd = _dev(x), ops.pack_conv_weight(_dev(w)), _dev(b, torch.float32), _dev(res)
    with_b = _rounded(ref + b.view(1, -1, 1, 1), True, "conv + bias").to(F64) + res         # the first rounding, then the second sum
    no_b = _rounded(ref, True, "conv").to(F64) + res
    _same(ops.conv_igemm_residual(xd, pk, bd, rd, None, dil, k, True), _rounded(torch.relu(with_b), True, "relu(.. + res)", True),
          "relu(bf16(conv + bias) + res)")
    _same(ops.conv_igemm_residual(xd, pk, bd, rd, None, dil, k, False), _rounded(with_b, True, ".. + res"), "bf16(conv + bias) + res")
    _nonvacuous(no_b[below > 0], "masked .. + res")
    want = torch.where(below > 0, no_b, torch.zeros_like(no_b))
    _same(ops.conv_igemm_residual(xd, pk, None, rd, _dev(below), dil, k, False), _bf16(want), "masked bf16(conv) + res")


# ---- 6. the direct kernels ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 64), (64, 128), (128, 128), (128, 64)])
def test_direct_conv_is_the_rounded_float64_convolution(ops, cin, cout):
    for B, H, W in DIRECT_MAPS:
        full = (H, W) != (1, 1)
        x, w, b, ref, _ = _fwd_case(B, H, W, cin, cout, 3, 1, 11, full_window=full)
        xd, wd, bd = _dev(x), _dev(w), _dev(b, torch.float32)
        for bias in (False, True):
            for relu in (False, True):
                got = ops.conv3x3_direct(xd, wd, bd if bias else None, relu)
                what = "%dx%dx%d bias %d relu %d" % (B, H, W, bias, relu)
                _same(got, _rounded(_post(ref, b if bias else None, relu), full, what, relu), what)


@gpu
@pytest.mark.parametrize("cf,cb", [(64, 64), (128, 128), (128, 64), (64, 128)])
def test_direct_conv_data_gradient_is_exact(ops, cf, cb):
    """cf: channels of the incoming gradient, cb: channels of the layer below, whose ReLU backward and bias gradient ride along"""
    for B, H, W in DIRECT_MAPS:
        gen = _gen(21)
        g, w, y = _ints((B, cf, H, W), -8, 8, gen), _ints((cf, cb, 3, 3), -4, 4, gen), _relu_out((B, cb, H, W), 8, gen)
        ref = _dgrad64(g, w, 1, (H, W))
        _bounded(_dgrad64(g.abs(), w.abs(), 1, (H, W)).max())
        if (H, W) != (1, 1):
            _nonvacuous(ref[y > 0], "masked data gradient")
        wt = _dev(w.flip(2, 3).transpose(0, 1).contiguous())
        _same(ops.conv3x3_direct(_dev(g), wt, None, False), _rounded(ref, (H, W) != (1, 1), "data gradient"), "%dx%dx%d plain" % (B, H, W))
        gx, gb = ops.conv3x3_direct_dgrad(_dev(g), wt, _dev(y))
        stored, sums = _masked(ref, y, 1.0)
        _same(gx, stored, "%dx%dx%d gx" % (B, H, W))
        _same(gb, sums, "%dx%dx%d bias gradient" % (B, H, W))


@gpu
def test_direct_conv_weight_gradient_is_exact(ops):
    for cin, cout in ops.WGRAD_CONV_SHAPES:
        for B, H, W in DIRECT_MAPS:
            x, g, ref, _ = _wgrad_case(B, H, W, cin, cout, 3, 1, 5)
            if (H, W) != (1, 1):
                _nonvacuous(ref, "weight gradient")
            xd, gd = _dev(x), _dev(g)
            _same(ops.conv3x3_wgrad(xd, gd, out_dtype=torch.float32), _f32(ref), "%d -> %d, %dx%dx%d float32" % (cin, cout, B, H, W))
            _same(ops.conv3x3_wgrad(xd, gd), _bf16(ref), "%d -> %d, %dx%dx%d bf16" % (cin, cout, B, H, W))


# ---- 7. the fc8 heads ----------------------------------------------------------------------------------------------------------
# The float32 operand of the MFMA GEMMs (w in the forward, g in the weight gradient) is split into three bf16 terms inside the
# kernels; integer weights would leave the second and third zero.  Dense-narrow: every element +-m / 16, m odd with `bits`
# (9 - 11) significant bits — the second term is live.  Sparse-wide: at most four non-zero values per output sum, each +-m 2^-16 with
# 20 significant bits — all three terms are live.  _split_live asserts both on the operand itself.
HEAD_SHAPES = [                                           # (B, K, H, W, O, n)
    (1, 256, 5, 7, 32, 2),
    (2, 512, 13, 17, 3, 1),                               # M = 442: two weight-gradient chunks
    (1, 1024, 6, 7, 21, 4),                               # the row-strip data gradient
    (1, 2048, 3, 3, 21, 3),                               # the f32-input MFMA weight gradient
]
FWD_BITS = {256: 11, 512: 11, 1024: 10, 2048: 9}          # by K: bits of the dense w (sums of n K terms), so that the bound holds
BWD_BITS = {35: 11, 442: 9, 42: 11, 9: 11}                # by M = B H W: bits of the dense g (sums of M terms)
WIDE = 2.0 ** -16


def _heads64(xs, w, b):
    n, O, K = w.shape
    return sum(F.conv2d(xs[k], w[k].reshape(O, K, 1, 1), None if b is None else b[k]) for k in range(n))


def _sparse_rows(rows, cols, per_col, gen, ties):
    """(rows, cols) with per_col (or all, if fewer) non-zero 20-bit values in every column"""
    t = torch.zeros(rows, cols, dtype=F64)
    for c in range(cols):
        at = torch.randperm(rows, generator=gen)[:per_col]
        t[at, c] = _wide((at.numel(),), 20, WIDE, gen, ties)
    return t


@gpu
@pytest.mark.parametrize("pattern", ["dense-narrow", "sparse-wide"])
@pytest.mark.parametrize("B,K,H,W,O,n", HEAD_SHAPES)
def test_heads_forward_is_the_float64_product(ops, B, K, H, W, O, n, pattern):
    gen, bits = _gen(7), FWD_BITS[K]
    if pattern == "dense-narrow":
        xs = [_ints((B, K, H, W), -3, 3, gen) for _ in range(n)]
        w, b, q = _wide((n, O, K), bits, 1.0 / 16, gen), _ints((n, O), -64, 64, gen) / 16, 1.0 / 16
    else:
        xs = [_ints((B, K, H, W), -2, 2, gen) for _ in range(n)]
        w = _sparse_rows(n * K, O, 4, gen, False).reshape(n, K, O).permute(0, 2, 1).contiguous()      # four per output over all branches
        b, q = _ints((n, O), -64, 64, gen) / 16, WIDE
    _split_live(w, 2 if pattern == "dense-narrow" else 3, "w")
    ref = _heads64(xs, w, b)
    _bounded(1.01 * _heads64([x.abs() for x in xs], w.abs(), b.abs()).max(), q)      # (1.01: a first split term may exceed its operand by 2^-8)
    got = ops.heads_forward([_dev(x) for x in xs], _dev(w, torch.float32), _dev(b, torch.float32))
    _same(got, _f32(ref), pattern)


@gpu
@pytest.mark.parametrize("relu_scale", [0.0, 2.0])
@pytest.mark.parametrize("pattern", ["dense-narrow", "sparse-wide"])
@pytest.mark.parametrize("B,K,H,W,O,n", HEAD_SHAPES)
def test_heads_backward_is_exact(ops, B, K, H, W, O, n, pattern, relu_scale):
    """gw (float32, exact), gx (one bf16 rounding; with relu_scale masked by x > 0 and scaled before it) and the absorbed bias
    gradient (the column sums of the stored gx)"""
    gen = _gen(9)
    M, scale = B * H * W, relu_scale if relu_scale > 0 else 1.0
    bits = BWD_BITS[M]
    if pattern == "dense-narrow":
        g, w, q, xr = _wide((B, O, H, W), bits, 1.0 / 16, gen), _ints((n, O, K), -2, 2, gen), 1.0 / 16, 3
    else:
        g = _sparse_rows(M, O, 4, gen, True).reshape(B, H, W, O).permute(0, 3, 1, 2).contiguous()      # (ties: gx is one such value, rounded)
        w, q, xr = torch.zeros(n, O, K, dtype=F64), WIDE, 2
        for k in range(n):                                # one +-1 per channel: gx is a single 20-bit value, rounded
            w[k, torch.randint(0, O, (K,), generator=gen), torch.arange(K)] = (torch.randint(0, 2, (K,), generator=gen) * 2 - 1).to(F64)
    xs = [_relu_out((B, K, H, W), xr, gen) if relu_scale > 0 else _ints((B, K, H, W), -xr, xr, gen) for _ in range(n)]
    _split_live(g, 2 if pattern == "dense-narrow" else 3, "g")
    gm = g.permute(0, 2, 3, 1).reshape(M, O)
    ref_w = torch.stack([gm.t() @ x.permute(0, 2, 3, 1).reshape(M, K) for x in xs])
    ref_x = [(gm @ w[k]).reshape(B, H, W, K).permute(0, 3, 1, 2) for k in range(n)]
    _bounded(1.01 * max((gm.abs().t() @ x.abs().permute(0, 2, 3, 1).reshape(M, K)).max() for x in xs), q)
    _bounded(scale * max((gm.abs() @ w[k].abs()).max() for k in range(n)), q)
    live = torch.stack(ref_x)[(torch.stack(xs) > 0) if relu_scale > 0 else torch.ones_like(torch.stack(xs), dtype=torch.bool)]
    _nonvacuous(live[live != 0] if pattern == "sparse-wide" else live, "gx")      # (sparse: most sums have no term at all)
    out = ops.heads_backward([_dev(x) for x in xs], _dev(w, torch.float32), _dev(g, torch.float32), True, relu_scale)
    _same(out[1], _f32(ref_w), "gw")
    for k in range(n):
        if relu_scale > 0:
            stored = _bf16(torch.where(xs[k] > 0, scale * ref_x[k], torch.zeros_like(ref_x[k])))
            sums = stored.to(F64).sum((0, 2, 3))
            _bounded(stored.to(F64).abs().sum((0, 2, 3)).max(), q)
            _same(out[0][k], stored, "gx, branch %d" % k)
            _same(out[2][k], _f32(sums), "bias gradient, branch %d" % k)
        else:
            _same(out[0][k], _bf16(ref_x[k]), "gx, branch %d" % k)


# ---- 8. the ASPP shifts (the geometry of test_aspp_head_as_one_1x1_product_plus_shifted_gather) ----------------------------------
@gpu
def test_aspp_shift_sum_and_gather_are_exact(ops):
    B, H, W, O, CT, P = 2, 19, 23, 5, 128, 30
    offsets = [(-3, 0), (0, 2), (4, -5), (0, 0), (30, 0)]                               # (the last: every source outside the map)
    gen = _gen(21)
    y, bias, g = _ints((B, CT, H, W), -256, 256, gen), _ints((O,), -64, 64, gen), _ints((B, O, H, W), -4095, 4095, gen).contiguous() / 16
    shift = lambda t, dy, dx: F.pad(t, (P, P, P, P))[:, :, P + dy:P + dy + H, P + dx:P + dx + W]      # noqa: E731  out[y, x] = t[y + dy, x + dx]
    want = bias.view(1, O, 1, 1) + sum(shift(y[:, j * O:(j + 1) * O], dy, dx) for j, (dy, dx) in enumerate(offsets))
    _bounded(bias.abs().max() + len(offsets) * y.abs().max())
    _same(ops.aspp_shift_sum(_dev(y), offsets, O, _dev(bias, torch.float32)), _f32(want), "shift sum")
    wantp = torch.zeros(B, CT, H, W, dtype=F64)
    for j, (dy, dx) in enumerate(offsets):
        wantp[:, j * O:(j + 1) * O] = shift(g, -dy, -dx)
    _nonvacuous(g, "bf16(g)")
    _same(ops.aspp_shift_gather(_dev(g, torch.float32), offsets, CT), _bf16(wantp).contiguous(memory_format=CL), "shift gather")
