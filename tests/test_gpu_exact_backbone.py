"""The pooling and elementwise passes of the backbone (csrc/backbone_ops.hip: max pool forward and its three backwards, average
pool, relu_bwd_bias / bias_grad and their finishing pass, add_relu / relu_mask; csrc/layers.hip: im2col / col2im) bit for bit.

Same rules as test_gpu_exact_conv.py: every reference is float64 on the CPU, written from the kernel's stated contract; where a
kernel stores bf16 the reference rounds once (float64 -> float32 -> bf16, `_bf16`); operands are integers (or multiples of one
power of two) small enough that every fp32 partial sum of a kernel is exact in whatever order it adds (`_bounded`), so there is no
tolerance anywhere and a failure names the element.  The references themselves are verified against torch's CPU float64
operators by the tests that need no GPU, and so are the promises of the data generators (ties in the pooling windows, every
window code, gradients that need rounding).

The max pool's contract (backbone_ops.hip, "3x3 max pooling"): the window is clipped to the image and walked dy, then dx; a tap
replaces the best so far when it is greater, or a NaN, or the first taken; code = 3 dy + dx; under relu_input a window whose
maximum is not positive (`<= 0`, false for a NaN) carries 0xfe; the backward adds each window's gradient onto the pixel its code
names and codes >= 9 name nothing.

Notes on the cases.  Window codes: a 1 x W map can only produce the codes of its middle row (and the single floor-mode
stride-2 window row of a 2 x 3 map none of the top row), so "every code occurs" is asserted for the codes the geometry allows,
computed from the shape alone; those are all nine on every map of at least 3 x 3.
col2im: the rounding condition (`_nonvacuous`) is asserted for every case but (2, 8, 5, 5, 6), whose dilation is at least the map's
extent: only the centre tap lies inside, every output is a copy of one bf16 value and nothing is rounded (asserted instead).
add_relu / relu_mask on eight elements: one 16-byte group cannot hold a rounding share or every special value in both halves of a
word, so those two conditions are asserted on the two larger sizes only.
The fused stride-2 backward gives a block more than one round of 256 items only above 512 * 256 items:
B ceil(H/2) ceil(W/2) C/8 = 135168 for (4, 256, 66, 63); (4, 64, 66, 63) has 33792 and stays at one round per block."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_exact_conv import _gen, _ints, _relu_out, _dev, _bounded, _f32, _bf16, _nonvacuous, _same

gpu = pytest.mark.gpu
CL = torch.channels_last
F64 = torch.float64
SUB = 2.0 ** -133                                         # the smallest positive bf16 subnormal (bits 0x0001)
INF = float("inf")
NAN = float("nan")
DEAD = 0xfe


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


def _same_bits(got, want, what):
    """NaN at the same positions, equal bit patterns everywhere else (so -0.0 != +0.0, unlike torch.equal)"""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    bits = torch.int16 if got.element_size() == 2 else torch.int32
    gn, wn = torch.isnan(got), torch.isnan(want)
    gb, wb = got.contiguous().view(bits), want.contiguous().view(bits)
    bad = ((gn != wn) | (~wn & (gb != wb))).nonzero()
    if bad.shape[0] == 0:
        return
    mask = 0xffff if got.element_size() == 2 else 0xffffffff
    first = [(tuple(i.tolist()), "%#x" % (int(gb[tuple(i.tolist())]) & mask), "%#x" % (int(wb[tuple(i.tolist())]) & mask)) for i in bad[:6]]
    raise AssertionError("%s: %d of %d elements differ; first (index, got bits, want bits): %s" % (what, bad.shape[0], want.numel(), first))


def _bits(t):
    return int(t.view(torch.int16))


def _same_codes(got, want, what):
    """got: the kernel's (B, OH, OW, C) uint8 codes; want: (B, C, OH, OW)"""
    got = got.detach().cpu().permute(0, 3, 1, 2)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape), tuple(want.shape))
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), int(got[tuple(i.tolist())]), int(want[tuple(i.tolist())])) for i in bad[:6]]
    assert bad.shape[0] == 0, "%s: %d of %d window codes differ; first (index, got, want): %s" % (what, bad.shape[0], want.numel(), first)


# ---- references (float64, CPU) ---------------------------------------------------------------------------------------------
def _out_size(n, stride, ceil):
    """windows of a 3-wide, pad-1 walk over n pixels (the rule of ops.maxpool3x3_out_size, restated): floor or ceil of
    (n + 2 - 3) / stride, plus one; a last window that would start beyond the image's last pixel's right pad is dropped"""
    num = n - 1
    o = (num + stride - 1) // stride + 1 if ceil else num // stride + 1
    return o - 1 if (o - 1) * stride >= n + 1 else o


def _taps(H, W, OH, OW, stride):
    """for each of the nine taps: (dy, dx, source rows clamped, source cols clamped, the (OH, OW) mask of windows that have it)"""
    oy, ox = torch.arange(OH) * stride - 1, torch.arange(OW) * stride - 1
    for dy in range(3):
        for dx in range(3):
            yy, xx = oy + dy, ox + dx
            inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
            yield dy, dx, yy.clamp(0, H - 1), xx.clamp(0, W - 1), inside


def _pool_ref(x, stride, ceil):
    """-> (values float64, codes uint8), both (B, C, OH, OW)"""
    B, C, H, W = x.shape
    OH, OW = _out_size(H, stride, ceil), _out_size(W, stride, ceil)
    best = torch.zeros(B, C, OH, OW, dtype=F64)
    code = torch.full((B, C, OH, OW), 0xff, dtype=torch.uint8)
    taken = torch.zeros(B, C, OH, OW, dtype=torch.bool)
    for dy, dx, yy, xx, inside in _taps(H, W, OH, OW, stride):
        v = x[:, :, yy][:, :, :, xx]
        take = inside & ((v > best) | torch.isnan(v) | ~taken)
        best = torch.where(take, v, best)                 # (a copy: the selected element's sign of zero is kept)
        code = torch.where(take, torch.full_like(code, 3 * dy + dx), code)
        taken |= take
    assert taken.all()
    return best, code


def _pool_dead(values):
    return values <= 0


def _pool_bwd_ref(go, codes, H, W, stride):
    B, C, OH, OW = go.shape
    gin = torch.zeros(B, C, H, W, dtype=F64)
    for dy, dx, yy, xx, inside in _taps(H, W, OH, OW, stride):
        hit = codes == 3 * dy + dx
        assert not (hit & ~inside).any(), "a code names a tap outside the image"
        add = torch.where(hit, go, torch.zeros_like(go)).permute(2, 3, 0, 1)                  # (clamped taps repeat a pixel: accumulate)
        gin.permute(2, 3, 0, 1).index_put_((yy[:, None].expand(OH, OW), xx[None, :].expand(OH, OW)), add, accumulate=True)
    return gin


def _avg64(x):
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 1, 1))
    return sum(p[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / 9.0


def _avg_ref(x):
    """one correctly rounded fp32 division (float64 quotient -> float32 is that: 53 >= 2 * 24 + 2), then bf16"""
    return _avg64(x).float().bfloat16()


def _unfold_ref(x, dil):
    """x (B, C, H, W) -> (B H W, 9 C) in the kernel's [pixel][tap][channel] order"""
    B, C, H, W = x.shape
    u = F.unfold(x, 3, dilation=dil, padding=dil)                                            # (B, C * 9, H W), channel-major
    return u.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)


def _fold_ref(cols, B, C, H, W, dil):
    u = cols.reshape(B, H * W, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, H * W)
    return F.fold(u, (H, W), 3, dilation=dil, padding=dil)


def _share_ties(v):
    """of the float64 values v: the share that bf16 cannot hold, and the number of exact ties"""
    low = _f32(v).contiguous().view(torch.int32).bitwise_and(0xFFFF)
    return float((low != 0).float().mean()), int((low == 0x8000).sum())


# ---- cases -------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 16, 7, 9), (1, 8, 6, 6), (2, 8, 5, 8), (1, 16, 2, 3), (1, 8, 1, 1), (3, 8, 1, 5),
               (2, 24, 33, 29),                           # C8 = 3 does not divide 256
               (1, 136, 4, 5)]                            # C8 = 17: the thread count is no multiple of the channel groups
MODES = [(1, False), (2, False), (2, True)]              # (stride, ceil)
# the fused stride-2 backward needs 256 % (C / 8) == 0: C from {8, 16, 64, 256}, and one case with more than 512 * 256 items
FUSED_SHAPES = [s for s in POOL_SHAPES if 256 % (s[1] // 8) == 0 and s[1] % 8 == 0] + [(1, 64, 5, 8), (2, 256, 4, 5), (4, 256, 66, 63)]
AVG_SHAPES = [(B, 24 if i % 2 else 8, H, W) for i, (B, C, H, W) in enumerate(POOL_SHAPES)]


def _pool_in(shape, kind, seed):
    """kind "relu": integers 0..3, about 40 % zeros; "signed": integers in -2..2.  Both are full of ties."""
    gen = _gen(seed)
    if kind == "signed":
        return _ints(shape, -2, 2, gen)
    return (_ints(shape, 1, 3, gen) * (torch.rand(tuple(shape), generator=gen) < 0.6).to(F64)).contiguous(memory_format=CL)


def _reachable(H, W, stride, ceil):
    """the window codes the geometry allows: taps that lie inside the image for at least one window"""
    OH, OW = _out_size(H, stride, ceil), _out_size(W, stride, ceil)
    return {3 * dy + dx for dy, dx, _, _, inside in _taps(H, W, OH, OW, stride) if inside.any()}


def _fwd_case(shape, stride, ceil, kind):
    x = _pool_in(shape, kind, 31 + shape[2] * shape[3])
    val, code = _pool_ref(x, stride, ceil)
    return x, val, code


def _bwd_case(shape, stride, ceil, relu_out=False):
    """-> x, the reference codes, go (integers in +-255) and the float64 input gradient"""
    B, C, H, W = shape
    gen = _gen(77 + H * W)
    x = _relu_out(shape, 3, gen) if relu_out else _pool_in(shape, "relu", 5 + H * W)
    val, code = _pool_ref(x, stride, ceil)
    go = _ints(val.shape, -255, 255, gen)
    ref = _pool_bwd_ref(go, code, H, W, stride)
    _bounded(_pool_bwd_ref(go.abs(), code, H, W, stride).max())
    return x, val, code, go, ref


def _codes_dev(code):
    return code.permute(0, 2, 3, 1).contiguous().cuda()


def _blocks(rows, lanes, part_blocks=512):
    """partial blocks of a bias-gradient launch (launch_relu_bwd_bias: lanes = 256 // (C / 8); launch_bias_grad: 256 // C): rows
    per block = ceil(rows / 512) rounded up to whole sweeps of `lanes` rows -> (blocks, rows per block)"""
    rpb = -(-rows // part_blocks)
    rpb = -(-rpb // lanes) * lanes
    return -(-rows // rpb), rpb


# (C, rows): blocks, rows per block, rows of the last block.  C % 8 == 0: relu_bwd_bias_kernel (bias_grad: its y == nullptr path)
BIAS8_CASES = [
    (8, 200),                                             # 1 block of 256 rows (200 used)
    (8, 2051),                                            # 9 blocks of 256, the last with 3
    (24, 300),                                            # 4 blocks of 85, the last with 45
    (24, 2628),                                           # 31 blocks of 85, the last with 78
    (1024, 64),                                           # 32 blocks of 2
    (1024, 65),                                           # 33 blocks of 2, the last with 1
    (1024, 601),                                          # 301 blocks of 2, the last with 1
    (2048, 5),                                            # 5 blocks of 1
    (2048, 300),                                          # 300 blocks of 1
]
BIAS8_BLOCKS = [1, 9, 4, 31, 32, 33, 301, 5, 300]
# any C <= 256: bias_grad_kernel
BIAS1_CASES = [
    (1, 100),                                             # 1 block of 256 rows
    (1, 2100),                                            # 9 blocks of 256, the last with 52
    (5, 1550),                                            # 31 blocks of 51, the last with 20
    (21, 70),                                             # 6 blocks of 12, the last with 10
    (21, 385),                                            # 33 blocks of 12, the last with 1
    (129, 32),                                            # 32 blocks of 1
    (129, 300),                                           # 300 blocks of 1
    (255, 31),                                            # 31 blocks of 1
    (255, 700),                                           # 350 blocks of 2
]
BIAS1_BLOCKS = [1, 9, 31, 6, 33, 32, 300, 31, 350]


def _bias_g(C, rows, seed):
    r = 8 if rows >= 400 else 64
    g = _ints((1, C, rows, 1), -r, r, _gen(seed))
    _bounded(g.abs().sum((0, 2, 3)).max())
    return g


def _flat(t):
    """the memory of a channels_last tensor as one row (a view)"""
    flat = t.permute(0, 2, 3, 1).reshape(-1)
    assert flat.data_ptr() == t.data_ptr()
    return flat


def _mask_y(shape, seed):
    """a ReLU output with -0.0 (off), +inf and the positive subnormal (both on) sprinkled in"""
    y = _relu_out(shape, 8, _gen(seed))
    flat = _flat(y)
    flat[5::53], flat[7::59], flat[11::61] = -0.0, INF, SUB
    return y


IM2COL_CASES = [(2, 16, 9, 7, 1), (1, 24, 13, 11, 2), (2, 8, 5, 5, 6), (1, 8, 7, 30, 12)]      # (B, C, H, W, dil)
ELEMS = [8, 8 * 255, 8 * 257]
EW_SHAPES = {8: (1, 8, 1, 1), 8 * 255: (1, 8, 15, 17), 8 * 257: (1, 8, 1, 257)}      # "flat": the same memory as one row


def _col2im_case(B, C, H, W, dil):
    """integer columns in +-255 and their float64 fold; asserts the exactness bound and, unless only the centre tap lies inside
    the map (dil >= max(H, W): every output is a copy of one bf16 value, which never rounds), that the rounding is under test"""
    cols = _ints((B * H * W, 9 * C), -255, 255, _gen(20))
    ref = _fold_ref(cols, B, C, H, W, dil)
    _bounded(_fold_ref(cols.abs(), B, C, H, W, dil).max())
    if dil >= max(H, W):
        assert torch.equal(ref, cols[:, 4 * C:5 * C].reshape(B, H, W, C).permute(0, 3, 1, 2))
    else:
        _nonvacuous(ref, "col2im, dilation %d" % dil)
    return cols, ref


def _sum_operands(shape, seed):
    """a: integers in +-255, b: multiples of 1/4 below 64 — both bf16, their sum mostly not"""
    gen = _gen(seed)
    return _ints(shape, -255, 255, gen), _ints(shape, -255, 255, gen) / 4.0


def _special_y(shape, seed):
    """a ReLU output whose first elements (memory order) cycle through +0.0, -0.0, the subnormal, +inf and a negative value:
    the period is odd, so each lands on an even and on an odd position (both halves of a 32-bit word)"""
    y = _relu_out(shape, 8, _gen(seed))
    flat = _flat(y)
    cyc = [0.0, -0.0, SUB, INF, -3.0]
    n = min(flat.numel(), 40)
    flat[:n] = torch.tensor([cyc[i % 5] for i in range(n)], dtype=F64)
    return y, flat


# special values at known positions: a (1, 8, 9, 15) map of -1 with six 3 x 3 blocks whose centres (2 | 6, 4 | 8 | 12) are window
# centres at both strides, and an all -inf top-left corner whose window starts in the padding
SPECIAL_BLOCKS = [                                        # (centre, the nine values, value, code, live under relu_input)
    ((2, 4), [0.0, -0.0, -1, -1, -1, -1, -1, -1, -1], 0.0, 0, False),
    ((2, 8), [-0.0, 0.0, -1, -1, -1, -1, -1, -1, -1], -0.0, 0, False),
    ((2, 12), [1, INF, 2, INF, 3, -1, -1, -1, -1], INF, 1, True),
    ((6, 4), [1, NAN, 3, NAN, 5, -1, -1, -1, -1], NAN, 3, True),
    ((6, 8), [0.0, SUB, -1, -1, -1, -1, -1, -1, -1], SUB, 1, True),
    ((6, 12), [SUB, 0.0, -1, -1, -1, -1, SUB, -1, -1], SUB, 0, True),
]


def _special_map():
    x = torch.full((1, 8, 9, 15), -1.0, dtype=F64)
    for (cy, cx), vals, _, _, _ in SPECIAL_BLOCKS:
        x[0, :, cy - 1:cy + 2, cx - 1:cx + 2] = torch.tensor(vals, dtype=F64).view(3, 3)
    x[0, :, 0:2, 0:2] = -INF
    return x.contiguous(memory_format=CL)


# ---- CPU: the references equal torch's float64 operators -------------------------------------------------------------------------
@pytest.mark.parametrize("stride,ceil", MODES)
def test_pool_references_equal_torch_cpu_float64(stride, ceil):
    for shape in POOL_SHAPES + [(1, 2, 2, 2), (1, 3, 41, 41)]:
        B, C, H, W = shape
        for kind in ("relu", "signed"):
            x = _pool_in(shape, kind, 3).contiguous().requires_grad_(True)
            val, code = _pool_ref(x.detach(), stride, ceil)
            assert (_out_size(H, stride, ceil), _out_size(W, stride, ceil)) == tuple(val.shape[2:])
            tv, ti = F.max_pool2d(x, 3, stride, 1, ceil_mode=ceil, return_indices=True)
            assert tuple(tv.shape) == tuple(val.shape), (shape, tuple(tv.shape), tuple(val.shape))
            assert torch.equal(tv.detach(), val)
            oy = (torch.arange(val.shape[2]) * stride - 1).view(1, 1, -1, 1)
            ox = (torch.arange(val.shape[3]) * stride - 1).view(1, 1, 1, -1)
            idx = (oy + code.long() // 3) * W + ox + code.long() % 3
            assert torch.equal(idx, ti), "%s %s: first-maximum indices differ from torch's" % (shape, kind)
            go = _ints(val.shape, -255, 255, _gen(4)).contiguous()
            tv.backward(go)
            assert torch.equal(x.grad, _pool_bwd_ref(go, code, H, W, stride))
            dead = torch.where(_pool_dead(val), torch.full_like(code, DEAD), code)      # dead windows' gradient goes nowhere:
            assert torch.equal(_pool_bwd_ref(go, dead, H, W, stride),                    # the same as masking with x > 0
                               torch.where(x.detach() > 0, x.grad, torch.zeros_like(x.grad)))


def test_avg_reference_equals_torch_cpu_float64():
    for shape in AVG_SHAPES:
        x = _ints(shape, -255, 255, _gen(6)).contiguous().requires_grad_(True)
        t = F.avg_pool2d(x, 3, 1, 1, count_include_pad=True)
        assert torch.equal(t.detach(), _avg64(x.detach()))
        g = 9.0 * _ints(shape, -255, 255, _gen(7)).contiguous()          # multiples of 9: torch divides every term, we divide the sum
        t.backward(g)
        assert torch.equal(x.grad, _avg64(g))                             # the stencil is its own adjoint
        assert torch.equal(_avg_ref(x.detach()).view(torch.int16), t.detach().float().bfloat16().view(torch.int16))
    q = torch.arange(-2295, 2296, dtype=F64)                               # every sum nine taps in +-255 can give
    assert torch.equal((q / 9.0).float(), q.float() / 9.0)                 # float64 quotient -> float32 == the float32 division


@pytest.mark.parametrize("B,C,H,W,dil", IM2COL_CASES)
def test_unfold_and_fold_references_equal_shifted_copies(B, C, H, W, dil):
    x = _ints((B, C, H, W), -255, 255, _gen(8)).contiguous().requires_grad_(True)
    cols = _unfold_ref(x, dil)
    p = F.pad(x.detach(), (dil, dil, dil, dil))
    for tap in range(9):                                  # out[(b, y, x)][tap][c] = in[b][c][y + (ty - 1) dil][x + (tx - 1) dil]
        ty, tx = tap // 3, tap % 3
        want = p[:, :, ty * dil:ty * dil + H, tx * dil:tx * dil + W].permute(0, 2, 3, 1).reshape(B * H * W, C)
        assert torch.equal(cols.detach()[:, tap * C:(tap + 1) * C], want), tap
    g = _ints((B * H * W, 9 * C), -255, 255, _gen(9))
    cols.backward(g)                                      # fold is the adjoint of unfold
    assert torch.equal(x.grad, _fold_ref(g, B, C, H, W, dil))


# ---- CPU: the generators keep their promises ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,ceil", MODES)
def test_pool_inputs_are_full_of_ties_and_reach_every_code(stride, ceil):
    dead = live = 0
    for kind in ("relu", "signed"):
        tied = total = 0
        for shape in POOL_SHAPES:
            B, C, H, W = shape
            x, val, code = _fwd_case(shape, stride, ceil, kind)
            reach = _reachable(H, W, stride, ceil)
            if H >= 3 and W >= 3:
                assert reach == set(range(9)), (shape, reach)
            assert set(code.unique().tolist()) == reach, "%s %s: codes %s of %s occur" % (shape, kind, sorted(code.unique().tolist()), sorted(reach))
            count = torch.zeros_like(val)
            for dy, dx, yy, xx, inside in _taps(H, W, val.shape[2], val.shape[3], stride):
                count += (inside & (x[:, :, yy][:, :, :, xx] == val)).to(F64)
            assert (count >= 1).all()
            tied, total = tied + int((count >= 2).sum()), total + count.numel()
            if kind == "relu":
                assert 0.3 < float((x == 0).double().mean()) < 0.5 or x.numel() < 200
                dead, live = dead + int(_pool_dead(val).sum()), live + int((~_pool_dead(val)).sum())
        assert tied > 0.5 * total, (kind, tied, total)     # over all maps: more than half the windows hold their maximum twice
    assert dead >= 8 and live >= 8, (dead, live)           # relu_input has windows of both kinds
    for shape in FUSED_SHAPES if stride == 2 else []:     # the fused backward's inputs: _relu_out with its -0.0
        B, C, H, W = shape
        x, val, code, go, ref = _bwd_case(shape, stride, ceil, relu_out=True)
        assert set(code.unique().tolist()) == _reachable(H, W, stride, ceil), shape
        assert torch.signbit(x.permute(0, 2, 3, 1).reshape(-1)[::97]).all()


@pytest.mark.parametrize("stride", [1, 2])
def test_pool_gradients_need_rounding(stride):
    """over all shapes of one stride: stride 1 at least 10 % of the non-zero input gradients are not bf16 values and one is
    an exact tie; stride 2 (at most four windows per pixel) at least 3 %"""
    for cases, relu_out in ((POOL_SHAPES, False), (FUSED_SHAPES, True)):
        if relu_out and stride == 1:
            continue
        vals = []
        for shape in cases:
            for s, ceil in MODES:
                if s == stride:
                    x, val, code, go, ref = _bwd_case(shape, s, ceil, relu_out)           # asserts the exactness bound
                    assert set(code.unique().tolist()) == _reachable(shape[2], shape[3], s, ceil), (shape, s, ceil)
                    if relu_out:
                        ref = torch.where(x > 0, ref, torch.zeros_like(ref))
                        _bounded(_bf16(ref).to(F64).abs().sum((0, 2, 3)).max())
                    vals.append(ref[ref != 0])
        share, ties = _share_ties(torch.cat(vals))
        assert share >= (0.10 if stride == 1 else 0.03) and ties >= 1, (stride, relu_out, share, ties)


def test_bias_cases_cover_the_finishing_pass():
    """block counts (a property of rows and C): 1, one of 2-7, 9, 31, 32, 33 and one above 256 — the x32 loop of
    bias_finalize_block, its x8 tail and both left empty; a ragged last block; on both kernels"""
    for cases, blocks, lanes in ((BIAS8_CASES, BIAS8_BLOCKS, lambda C: 256 // (C // 8)), (BIAS1_CASES, BIAS1_BLOCKS, lambda C: 256 // C)):
        got = [_blocks(rows, lanes(C)) for C, rows in cases]
        assert [n for n, _ in got] == blocks
        n = set(blocks)
        assert {1, 9, 31, 32, 33} <= n and n & set(range(2, 8)) and max(n) > 256
        assert any(rows % rpb for (C, rows), (_, rpb) in zip(cases, got))
        assert all(nb <= 512 for nb in n)
    assert {C for C, _ in BIAS8_CASES} == {8, 24, 1024, 2048} and {C for C, _ in BIAS1_CASES} == {1, 5, 21, 129, 255}
    B, C, H, W = FUSED_SHAPES[-1]                          # the fused pool backward: several blocks, each more than one round
    items = B * ((H + 1) // 2) * ((W + 1) // 2) * (C // 8)
    ipb = -(-(-(-items // 512)) // 256) * 256           # ceil(items / 512), rounded up to whole rounds of 256
    assert items > 512 * 256 and ipb >= 512 and -(-items // ipb) > 1
    assert {s[1] for s in FUSED_SHAPES} == {8, 16, 64, 256}


def test_elementwise_operands_exercise_the_rounding():
    for n, shape in EW_SHAPES.items():
        a, b = _sum_operands(shape, 12)
        assert torch.equal(a.bfloat16().to(F64), a) and torch.equal(b.bfloat16().to(F64), b)
        y, flat = _special_y(shape, 13)
        for v in (SUB, INF, 0.0, -3.0):                   # "on" (the first two) and "off" (+0.0 and -0.0, a negative) show only where
            assert (a[y == v] != 0).any() and ((a + b)[y == v] != 0).any(), (n, v)      # the gradient is not zero
        if n > 8:                                         # eight elements: one 16-byte group, every special value once or twice; too
            _nonvacuous((a + b)[a + b > 0], "relu(a + b), %d" % n)      # few for a rounding share or for both halves of a word
            _nonvacuous((a + b)[y > 0], "masked g + g2, %d" % n)
            for v, neg in ((0.0, False), (0.0, True), (SUB, False), (INF, False), (-3.0, True)):
                at = ((flat[:40] == v) & (torch.signbit(flat[:40]) == neg)).nonzero().view(-1)
                assert (at % 2 == 0).any() and (at % 2 == 1).any(), v
    assert torch.tensor(SUB, dtype=F64).bfloat16().view(torch.int16).item() == 1      # the subnormal survives the host's casts


@pytest.mark.parametrize("B,C,H,W,dil", IM2COL_CASES)
def test_col2im_columns_exercise_the_rounding(B, C, H, W, dil):
    _col2im_case(B, C, H, W, dil)


def test_special_value_map_means_what_it_says():
    x = _special_map()
    for stride, ceil in MODES:
        val, code = _pool_ref(x, stride, ceil)
        for (cy, cx), _, v, c, live in SPECIAL_BLOCKS:
            got, gc = val[0, 0, cy // stride, cx // stride], int(code[0, 0, cy // stride, cx // stride])
            assert gc == c and (torch.isnan(got) if v != v else (got == v and torch.signbit(got) == torch.signbit(torch.tensor(v)))), ((cy, cx), float(got), gc)
            assert bool(_pool_dead(val)[0, 0, cy // stride, cx // stride]) == (not live)
        assert val[0, 0, 0, 0] == -INF and int(code[0, 0, 0, 0]) == 4                  # the first tap inside the image


def test_chain_gradients_stay_exact():
    _chain_case()


# ---- A. max pool forward ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("stride,ceil", MODES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_values_and_codes(ops, shape, stride, ceil):
    for kind in ("relu", "signed"):
        x, val, code = _fwd_case(shape, stride, ceil, kind)
        xd = _dev(x)
        out, cd = ops.maxpool3x3_fwd(xd, stride, ceil)
        _same_bits(out, _bf16(val), "%s values" % kind)
        _same_codes(cd, code, "%s codes" % kind)
        out, cd = ops.maxpool3x3_fwd(xd, stride, ceil, relu_input=True)
        _same_bits(out, _bf16(val), "%s values, relu_input" % kind)
        _same_codes(cd, torch.where(_pool_dead(val), torch.full_like(code, DEAD), code), "%s codes, relu_input" % kind)


@gpu
@pytest.mark.parametrize("stride,ceil", MODES)
def test_maxpool_forward_special_values(ops, stride, ceil):
    """signed zeros (the first of two equal taps is stored, sign and all), infinities, NaN (the value is NaN, the code the last
    NaN's: torch's rule) and a bf16 subnormal, which beats +0.0 and keeps its window alive — IEEE comparisons, no flushing"""
    x = _special_map()
    val, code = _pool_ref(x, stride, ceil)
    want = val.float().bfloat16()                          # (exact: every value is a bf16 value; _bf16 cannot compare a NaN)
    assert torch.equal(torch.nan_to_num(want.to(F64), nan=7.0), torch.nan_to_num(val, nan=7.0))
    xd = x.bfloat16().cuda().contiguous(memory_format=CL)
    for relu_in in (False, True):
        out, cd = ops.maxpool3x3_fwd(xd, stride, ceil, relu_input=relu_in)
        _same_bits(out, want, "values, relu_input %d" % relu_in)
        wc = torch.where(_pool_dead(val), torch.full_like(code, DEAD), code) if relu_in else code
        _same_codes(cd, wc, "codes, relu_input %d" % relu_in)
        out, cd = out.cpu(), cd.cpu()
        for (cy, cx), _, v, c, live in SPECIAL_BLOCKS:     # the named windows, spelled out
            oy, ox = cy // stride, cx // stride
            assert int(cd[0, oy, ox, 0]) == (c if live or not relu_in else DEAD), ((cy, cx), int(cd[0, oy, ox, 0]))
            assert _bits(out[0, 0, oy, ox]) == _bits(torch.tensor(v).bfloat16()) or v != v, ((cy, cx), float(out[0, 0, oy, ox]))


# ---- B. max pool backward ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("stride,ceil", MODES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_backward_is_the_rounded_scatter(ops, shape, stride, ceil):
    """stride 1: the gather kernel; stride 2: the 2 x 2-block kernel.  The codes are the reference's, not the forward kernel's"""
    x, val, code, go, ref = _bwd_case(shape, stride, ceil)
    gd = _dev(go)
    _same(ops.maxpool3x3_bwd(gd, _codes_dev(code), tuple(shape), stride), _bf16(ref), "plain codes")
    dead = torch.where(_pool_dead(val), torch.full_like(code, DEAD), code)
    _same(ops.maxpool3x3_bwd(gd, _codes_dev(dead), tuple(shape), stride), _bf16(_pool_bwd_ref(go, dead, shape[2], shape[3], stride)), "codes >= 9 name nothing")


@gpu
@pytest.mark.parametrize("ceil", [False, True])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_maxpool_backward_fused_with_relu_and_bias_gradient(ops, shape, ceil):
    """both forms — plain codes and the pool's input, or relu_input codes and the input's shape — store bf16(x > 0 ? scatter : 0)
    and return the exact column sums of what they stored"""
    x, val, code, go, ref = _bwd_case(shape, 2, ceil, relu_out=True)
    stored = _bf16(torch.where(x > 0, ref, torch.zeros_like(ref)))
    _bounded(stored.to(F64).abs().sum((0, 2, 3)).max())
    sums = _f32(stored.to(F64).sum((0, 2, 3)))
    dead = torch.where(_pool_dead(val), torch.full_like(code, DEAD), code)
    gd = _dev(go)
    for tag, cd, y in (("codes + input", code, _dev(x)), ("relu_input codes + shape", dead, tuple(shape))):
        gin, gb = ops.maxpool3x3_bwd_relu(gd, _codes_dev(cd), y)
        _same(gin, stored, "%s: input gradient" % tag)
        _same(gb, sums, "%s: bias gradient" % tag)


# ---- C. average pool ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", AVG_SHAPES)
def test_avgpool_is_the_rounded_float64_average(ops, shape):
    for seed, what in ((14, "forward"), (15, "on a gradient")):      # the backward is the same pass on the gradient
        x = _ints(shape, -255, 255, _gen(seed))
        _same_bits(ops.avgpool3x3_s1(_dev(x)), _avg_ref(x), what)


# ---- D. relu_bwd_bias, bias_grad and the finishing pass ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("scale", [1.0, 2.0, 1.25])
@pytest.mark.parametrize("C,rows", BIAS8_CASES)
def test_relu_bwd_bias_is_exact(ops, C, rows, scale):
    g, y = _bias_g(C, rows, 16), _mask_y((1, C, rows, 1), 17)
    stored = _bf16(torch.where(y > 0, scale * g, torch.zeros_like(g)))
    _bounded(stored.to(F64).abs().sum((0, 2, 3)).max(), 0.25)
    assert (stored[y == INF] != 0).any() and (stored[y == SUB] != 0).any()
    gm, gb = ops.relu_bwd_bias(_dev(g), _dev(y), scale)
    _same(gm, stored, "gm")
    _same(gb, _f32(stored.to(F64).sum((0, 2, 3))), "bias gradient")


@gpu
@pytest.mark.parametrize("C,rows", BIAS8_CASES + BIAS1_CASES)
def test_bias_grad_is_the_exact_column_sum(ops, C, rows):
    g = _bias_g(C, rows, 18)
    _same(ops.bias_grad(_dev(g)), _f32(g.sum((0, 2, 3))), "bias gradient")


# ---- E. add_relu, relu_mask --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", ELEMS)
@pytest.mark.parametrize("layout", ["flat", "cl"])
def test_add_relu_and_relu_mask_are_exact(ops, layout, n):
    shape = EW_SHAPES[n]
    a, b = _sum_operands(shape, 12)
    y, _ = _special_y(shape, 13)
    if layout == "flat":
        a, b, y = _flat(a), _flat(b), _flat(y)
    ad, bd = _dev(a), _dev(b)
    _same(ops.add_relu(ad, bd), _bf16(torch.relu(a + b)), "relu(a + b)")       # (_same: the sign of a zero result is not specified)
    yd = _dev(y)
    zero = torch.zeros_like(a)
    _same(ops.relu_mask(ad, yd), _bf16(torch.where(y > 0, a, zero)), "g where y > 0")
    _same(ops.relu_mask(ad, yd, bd), torch.where(y > 0, _bf16(a + b).to(F64), zero).bfloat16(), "bf16(g + g2) where y > 0")


# ---- F. im2col, col2im -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,C,H,W,dil", IM2COL_CASES)
def test_im2col_is_a_copy_and_col2im_its_rounded_adjoint(ops, B, C, H, W, dil):
    gen = _gen(19)
    bits = torch.randint(-32768, 32768, (B, C, H, W), generator=gen)           # arbitrary bf16 patterns, NaNs among them
    bits.view(-1)[::7] = -32768                                                # -0.0
    want = _unfold_ref(bits.to(F64), dil).to(torch.int16).view(torch.bfloat16)                # (a copy: exact through float64)
    x = bits.to(torch.int16).view(torch.bfloat16).permute(0, 2, 3, 1).contiguous().cuda()
    _same_bits(ops.im2col3x3_nhwc(x, dil), want, "bf16")
    for C4 in (4, 12):                                                         # the float32 entry: 16-byte groups of four
        bits = torch.randint(-2 ** 31, 2 ** 31, (B, C4, H, W), generator=gen)
        want = _unfold_ref(bits.to(F64), dil).to(torch.int32).view(torch.float32)
        x = bits.to(torch.int32).view(torch.float32).permute(0, 2, 3, 1).contiguous().cuda()
        _same_bits(ops.im2col3x3_nhwc(x, dil), want, "float32, C = %d" % C4)
    cols, ref = _col2im_case(B, C, H, W, dil)
    _same(ops.col2im3x3_nhwc(_dev(cols), B, H, W, C, dil), _bf16(ref), "col2im")


# ---- G. pool4 -> pool5 -> pool5a through the autograd nodes ------------------------------------------------------------------------
def _chain_case():
    """stride-1 max, stride-1 max, average; bf16 after every node, both ways.  The gradient behind the average node is
    bf16(k / 9), a multiple of 2^-11 (|k / 9| >= 2^-4); the two max-pool backwards add up to nine such values each"""
    shape, q = (2, 16, 9, 11), 2.0 ** -11
    B, C, H, W = shape
    x = _pool_in(shape, "relu", 23)
    g = _ints(shape, -255, 255, _gen(24))
    v4, c4 = _pool_ref(x, 1, False)
    v5, c5 = _pool_ref(_bf16(v4).to(F64), 1, False)
    out = _avg_ref(_bf16(v5).to(F64))
    ga = _avg_ref(g).to(F64)
    assert torch.equal(ga / q, torch.round(ga / q)) and float(ga[ga != 0].abs().min()) >= 2.0 ** -4
    _bounded(_pool_bwd_ref(ga.abs(), c5, H, W, 1).max(), q)
    g5 = _bf16(_pool_bwd_ref(ga, c5, H, W, 1)).to(F64)
    _bounded(_pool_bwd_ref(g5.abs(), c4, H, W, 1).max(), q)
    g4 = _bf16(_pool_bwd_ref(g5, c4, H, W, 1))
    _nonvacuous(_pool_bwd_ref(g5, c4, H, W, 1)[g4 != 0], "the chain's input gradient")
    return x, g, out, g4


@gpu
def test_pool4_pool5_pool5a_chain_forward_and_backward(ops):
    """what a fused or tiled pool5 chain must also pass, unchanged"""
    from dsrg_amd import backbone
    x, g, out, g4 = _chain_case()
    xd = _dev(x).requires_grad_(True)
    y = backbone.AvgPool3x3()(backbone.MaxPool3x3(1)(backbone._pool3x3(xd, 1, False)))
    nodes, todo = [], [y.grad_fn]                         # every node between y and x is an autograd Function of the backbone's own:
    while todo:                                           # nothing went to torch's pooling, which is exact on this data too
        node = todo.pop()
        if node is not None and type(node).__name__ != "AccumulateGrad":
            nodes.append(node)
            todo += [f for f, _ in node.next_functions]
    assert nodes and all(getattr(n, "_forward_cls", None) is not None and n._forward_cls.__module__ == backbone.__name__ for n in nodes), \
        [type(n).__name__ for n in nodes]
    _same_bits(y, out, "forward")
    y.backward(_dev(g))
    _same(xd.grad, g4, "input gradient")
