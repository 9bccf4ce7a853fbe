"""What the implicit-GEMM entry points refuse, and that a refusal leaves nothing behind (ops.conv_igemm ... ops.conv_igemm_wgrad; the
launchers of csrc/conv_igemm.hip behind the C ABI).  Every case is refused by host validation before anything is launched: the seven
ctypes wrappers raise ValueError, the library returns DSRG_ERR_INVALID / DSRG_ERR_UNSUPPORTED with its dsrg_last_error() text.  After
every refusal a valid launch of the same entry point gives the bits it gave before.  One geometry throughout: 1 x 256 x 8 x 8, 256 ->
256 channels, 1x1 kernels (so a kernel's two packings have one shape), two groups where an entry takes groups.

Not covered: a residual together with a dropout probability (prepare_igemm's "a residual goes with one group, no column sums, no
dropout").  No exported entry point takes both — dsrg_conv_igemm_residual_bf16 has no dropout argument, dsrg_conv_igemm_bf16 no
residual — so nothing outside the library can ask for it; the dropout probability's own range check stands in on dsrg_conv_igemm_bf16."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu
CL = torch.channels_last
B, C, H, W, K = 1, 256, 8, 8, 1
N = 2
DILS = (1, 1)


class Data:
    def __init__(self):
        from dsrg_amd import ops, _lib
        _lib.require_gpu()
        self.ops, self.lib, self.L = ops, _lib, _lib.lib()
        gen = torch.Generator().manual_seed(7)
        act = lambda: torch.randn(B, C, H, W, generator=gen).bfloat16().cuda().contiguous(memory_format=CL)      # noqa: E731
        self.xs, self.gs, self.masks = [act() for _ in range(N)], [act() for _ in range(N)], [act() for _ in range(N)]
        self.res = act()
        self.packed = [(torch.randn(C, C // 64, K * K, 64, generator=gen) / 16).bfloat16().cuda() for _ in range(N)]
        self.bias = [torch.randn(C, generator=gen).cuda() for _ in range(N)]
        self.scale = torch.rand(C, generator=gen).cuda() + 0.5
        self.valid = {
            "conv_igemm": lambda: ops.conv_igemm(self.xs, self.packed, self.bias, DILS, K, True),
            "conv_igemm_residual": lambda: ops.conv_igemm_residual(self.xs[0], self.packed[0], self.bias[0], self.res, self.masks[0], 1, K, True),
            "conv_igemm_dgrad": lambda: ops.conv_igemm_dgrad(self.gs, self.packed, self.masks, DILS, K, 2.0),
            "conv_igemm_backward": lambda: ops.conv_igemm_backward(self.gs[0], self.packed[0], self.xs[0], 1, self.masks[0], 2.0, K),
            "conv_igemm_backward_residual": lambda: ops.conv_igemm_backward_residual(self.gs[0], self.packed[0], self.xs[0], 1, K, self.masks[0],
                                                                                     self.res, self.scale),
            "conv_igemm_backward_groups": lambda: ops.conv_igemm_backward_groups(self.gs, self.packed, self.xs, DILS, K, self.masks, 2.0),
            "conv_igemm_wgrad": lambda: ops.conv_igemm_wgrad(self.xs, self.gs, DILS, K),
        }
        self.before = {name: self.run(name) for name in self.valid}

    def run(self, name):
        """the valid launch of an entry point -> its results as CPU tensors"""
        out = self.valid[name]()
        torch.cuda.synchronize()
        flat = []
        for o in (out if isinstance(out, (tuple, list)) else [out]):
            flat += [t for t in (o if isinstance(o, (tuple, list)) else [o]) if t is not None]
        return [t.detach().cpu().clone() for t in flat]

    def unchanged(self, name):
        now = self.run(name)
        assert len(now) == len(self.before[name]) and all(torch.equal(a, b) for a, b in zip(now, self.before[name])), \
            "%s: a valid launch after the refused call differs from the one before it" % name


@pytest.fixture(scope="module")
def D():
    return Data()


def _f32(t):
    return t.float()


def _nchw(t):
    return t.contiguous()                                     # (1, 256, 8, 8) NCHW-contiguous: not channels_last


def _other_shape(t):
    return t[:, :, :, :4].contiguous(memory_format=CL)


def _not_bf16(p):
    return p.half()


def _wrong_pack(p):
    return p.reshape(C, C // 128, K * K, 128)


def _first(f):
    return lambda ts: [f(ts[0])] + list(ts[1:])


# name -> callable(D, replacements) running the wrapper on D's tensors with some of them replaced
def _call(D, name, **r):
    o = D.ops
    xs, gs, masks, packed = r.get("xs", D.xs), r.get("gs", D.gs), r.get("masks", D.masks), r.get("packed", D.packed)
    res, dils = r.get("res", D.res), r.get("dils", DILS)
    if name == "conv_igemm":
        return o.conv_igemm(xs, packed, D.bias, dils, K, True)
    if name == "conv_igemm_residual":
        return o.conv_igemm_residual(xs[0], packed[0], D.bias[0], res, masks[0], 1, K, True)
    if name == "conv_igemm_dgrad":
        return o.conv_igemm_dgrad(gs, packed, masks, dils, K, 2.0)
    if name == "conv_igemm_backward":
        return o.conv_igemm_backward(gs[0], packed[0], xs[0], 1, masks[0], 2.0, K)
    if name == "conv_igemm_backward_residual":
        return o.conv_igemm_backward_residual(gs[0], packed[0], xs[0], 1, K, masks[0], res, D.scale)
    if name == "conv_igemm_backward_groups":
        return o.conv_igemm_backward_groups(gs, packed, xs, dils, K, masks, 2.0)
    return o.conv_igemm_wgrad(xs, gs, dils, K)


FIRST_ACTIVATION = {"conv_igemm": "xs", "conv_igemm_residual": "xs", "conv_igemm_dgrad": "gs", "conv_igemm_backward": "gs",
                    "conv_igemm_backward_residual": "gs", "conv_igemm_backward_groups": "gs", "conv_igemm_wgrad": "xs"}
# the tensors a wrapper wants channels_last as they come (it makes the others so itself)
NEEDS_CL = {"conv_igemm_residual": ("masks", "res"), "conv_igemm_dgrad": ("masks",), "conv_igemm_backward": ("xs", "masks"),
            "conv_igemm_backward_residual": ("xs", "masks", "res"), "conv_igemm_backward_groups": ("xs", "masks")}
HAS_KERNEL = [n for n in FIRST_ACTIVATION if n != "conv_igemm_wgrad"]
HAS_GROUPS = ["conv_igemm", "conv_igemm_dgrad", "conv_igemm_backward_groups", "conv_igemm_wgrad"]
HAS_MASK = ["conv_igemm_residual", "conv_igemm_dgrad", "conv_igemm_backward", "conv_igemm_backward_residual", "conv_igemm_backward_groups"]

WRAPPER_CASES = [(n, "float32 activation", {FIRST_ACTIVATION[n]: _first(_f32)}) for n in FIRST_ACTIVATION]
WRAPPER_CASES += [(n, "NCHW " + which, {which: _nchw if which == "res" else _first(_nchw)}) for n, ws in NEEDS_CL.items() for which in ws]
WRAPPER_CASES += [(n, "kernel not bf16", {"packed": _first(_not_bf16)}) for n in HAS_KERNEL]
WRAPPER_CASES += [(n, "kernel of another packed shape", {"packed": _first(_wrong_pack)}) for n in HAS_KERNEL]
WRAPPER_CASES += [(n, "three dilations for two groups", {"dils": lambda d: (1, 1, 1)}) for n in HAS_GROUPS]
WRAPPER_CASES += [(n, "five groups", {k: (lambda ts: [ts[0]] * 5) for k in ("xs", "gs", "masks", "packed")} | {"dils": lambda d: (1,) * 5})
                  for n in HAS_GROUPS]
WRAPPER_CASES += [(n, "mask of another shape", {"masks": _first(_other_shape)}) for n in HAS_MASK]


@gpu
@pytest.mark.parametrize("name,what,changes", WRAPPER_CASES, ids=["%s-%s" % (n, w.replace(" ", "_")) for n, w, _ in WRAPPER_CASES])
def test_wrapper_refuses(D, name, what, changes):
    base = {"xs": D.xs, "gs": D.gs, "masks": D.masks, "packed": D.packed, "res": D.res, "dils": DILS}
    with pytest.raises(ValueError):
        _call(D, name, **{k: f(base[k]) for k, f in changes.items()})
    D.unchanged(name)


# ---- the library itself: (entry point's wrapper, what is wrong, error code, dsrg_last_error() text)
def _vp(ts, n=None):
    """host array of device pointers; entries may be None or integers"""
    vals = [t.data_ptr() if torch.is_tensor(t) else t for t in ts]
    return (ctypes.c_void_p * max(len(vals), n or 0))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Lib:
    """the seven entry points on D's tensors with the arguments a case overrides"""

    def __init__(self, D):
        self.D, self.L = D, D.L
        dev = D.xs[0].device
        self.out = [torch.empty((B, C, H, W), dtype=torch.bfloat16, device=dev, memory_format=CL) for _ in range(5)]
        self.gw = [torch.empty((C, C, K, K), dtype=torch.float32, device=dev, memory_format=CL) for _ in range(5)]
        self.gb = [torch.empty(C, dtype=torch.float32, device=dev) for _ in range(5)]
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scratch(self, nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.D.xs[0].device)

    def five(self, ts):
        return [ts[i % len(ts)] for i in range(5)]

    def conv_igemm(self, n=N, x=None, cin=C, drop_p=0.0):
        D = self.D
        return self.L.dsrg_conv_igemm_bf16(_vp(x or self.five(D.xs)), _vp(self.five(D.packed)), _vp(self.five(D.bias)), _vp(self.out),
                                           _ints([1] * 5), n, B, H, W, cin, C, K, 1, drop_p, 0, None, 0, self.stream)

    def conv_igemm_dgrad(self, n=N, mask=None, short=0):
        D = self.D
        need = self.L.dsrg_conv_igemm_dgrad_workspace(N, B, H, W, C)
        ws = self.scratch(need)
        return self.L.dsrg_conv_igemm_dgrad_bf16(_vp(self.five(D.gs)), _vp(self.five(D.packed)), _vp(mask or self.five(D.masks)), _vp(self.out),
                                                 _vp(self.gb), _ints([1] * 5), n, B, H, W, C, C, K, 2.0, _p(ws), need - short, self.stream)

    def conv_igemm_wgrad(self, n=N, g=None, cin=C, short=0):
        D = self.D
        need = self.L.dsrg_conv_igemm_wgrad_workspace(N, B, H, W, C, C, K)
        ws = self.scratch(need)
        return self.L.dsrg_conv_igemm_wgrad_bf16(_vp(self.five(D.xs)), _vp(g or self.five(D.gs)), _vp(self.gw), _ints([1] * 5), n, _p(ws),
                                                 need - short, B, H, W, cin, C, K, 0, self.stream)

    def conv_igemm_backward(self, mask=True, cin=C, wshort=0, cshort=0):
        D = self.D
        need = self.L.dsrg_conv_igemm_wgrad_workspace(1, B, H, W, C, C, K)
        cneed = self.L.dsrg_conv_igemm_dgrad_workspace(1, B, H, W, C)
        ws, cws = self.scratch(need), self.scratch(cneed)
        return self.L.dsrg_conv_igemm_backward_bf16(_p(D.gs[0]), _p(D.packed[0]), _p(D.xs[0]), _p(D.masks[0]) if mask else None, _p(self.out[0]),
                                                    _p(self.gw[0]), 1, _p(self.gb[0]), 2.0, _p(cws), cneed - cshort, _p(ws), need - wshort,
                                                    B, H, W, cin, C, K, self.stream)

    def conv_igemm_backward_residual(self, wshort=0):
        D = self.D
        need = self.L.dsrg_conv_igemm_wgrad_workspace(1, B, H, W, C, C, K)
        ws = self.scratch(need)
        return self.L.dsrg_conv_igemm_backward_residual_bf16(_p(D.gs[0]), _p(D.packed[0]), _p(D.xs[0]), _p(D.masks[0]), _p(D.res), _p(self.out[0]),
                                                             _p(self.gw[0]), _p(D.scale), 1, _p(ws), need - wshort, B, H, W, C, C, K, self.stream)

    def conv_igemm_backward_groups(self, n=N, mask=True, masks=None, gw=None, wshort=0, cshort=0):
        D = self.D
        need = self.L.dsrg_conv_igemm_wgrad_workspace(N, B, H, W, C, C, K)
        cneed = self.L.dsrg_conv_igemm_dgrad_workspace(N, B, H, W, C)
        ws, cws = self.scratch(need), self.scratch(cneed)
        return self.L.dsrg_conv_igemm_backward_groups_bf16(_vp(self.five(D.gs)), _vp(self.five(D.packed)), _vp(self.five(D.xs)),
                                                           _vp(masks or self.five(D.masks)) if mask else None, _vp(self.out), _vp(gw or self.gw),
                                                           _ints([1] * 5), n, _vp(self.gb), 2.0, _p(cws), cneed - cshort, _p(ws), need - wshort,
                                                           B, H, W, C, C, K, 0, 0, self.stream)


INVALID, UNSUPPORTED = -1, -3
GROUPS = "conv_igemm: 1..4 groups"
WGROUPS = "conv_igemm_wgrad: 1..4 groups"
NULL = "conv_igemm: null pointer"
WNULL = "conv_igemm_wgrad: null pointer"
COLSUM = "conv_igemm: column-sum scratch missing or too small"
WSPACE = "conv_igemm_wgrad: workspace of %d bytes needed"
SHAPE = "conv_igemm: cin %% 64 == 0, cout %% 128 == 0 (or cout = 64), k in (1, 3) required (got %d, %d, %d)"
WSHAPE = "conv_igemm_wgrad: cin %% 64 == 0, cout %% 64 == 0, k in (1, 3) required (got %d, %d, %d)"


def _null_second(name):
    return lambda lib: [getattr(lib.D, name)[0], None] + [getattr(lib.D, name)[0]] * 3


LIB_CASES = [
    ("conv_igemm", "no groups", dict(n=0), INVALID, GROUPS),
    ("conv_igemm", "five groups", dict(n=5), INVALID, GROUPS),
    ("conv_igemm_dgrad", "no groups", dict(n=0), INVALID, GROUPS),
    ("conv_igemm_dgrad", "five groups", dict(n=5), INVALID, GROUPS),
    ("conv_igemm_wgrad", "no groups", dict(n=0), INVALID, WGROUPS),
    ("conv_igemm_wgrad", "five groups", dict(n=5), INVALID, WGROUPS),
    ("conv_igemm_backward_groups", "no groups", dict(n=0), INVALID, GROUPS),
    ("conv_igemm_backward_groups", "five groups", dict(n=5), INVALID, GROUPS),
    ("conv_igemm", "null input of the second group", dict(x=_null_second("xs")), INVALID, NULL),
    ("conv_igemm_dgrad", "null mask of the second group", dict(mask=_null_second("masks")), INVALID, NULL),
    ("conv_igemm_wgrad", "null gradient of the second group", dict(g=_null_second("gs")), INVALID, WNULL),
    ("conv_igemm_backward_groups", "null mask of the second group", dict(masks=_null_second("masks")), INVALID, NULL),
    ("conv_igemm_backward_groups", "null weight gradient of the second group", dict(gw=lambda lib: [lib.gw[0], None] + lib.gw[2:]), INVALID, WNULL),
    ("conv_igemm_wgrad", "workspace one byte short", dict(short=1), INVALID, (WSPACE, N)),
    ("conv_igemm_backward", "weight-gradient workspace one byte short", dict(wshort=1), INVALID, (WSPACE, 1)),
    ("conv_igemm_backward_residual", "weight-gradient workspace one byte short", dict(wshort=1), INVALID, (WSPACE, 1)),
    ("conv_igemm_backward_groups", "weight-gradient workspace one byte short", dict(wshort=1), INVALID, (WSPACE, N)),
    ("conv_igemm_dgrad", "column-sum scratch one byte short", dict(short=1), INVALID, COLSUM),
    ("conv_igemm_backward", "column-sum scratch one byte short", dict(cshort=1), INVALID, COLSUM),
    ("conv_igemm_backward_groups", "column-sum scratch one byte short", dict(cshort=1), INVALID, COLSUM),
    ("conv_igemm_backward_groups", "bias gradients without masks", dict(mask=False), INVALID, "conv_igemm_backward_groups: bad arguments"),
    ("conv_igemm_backward", "bias gradient without a mask", dict(mask=False), INVALID, "conv_igemm_backward: bad arguments"),
    ("conv_igemm", "dropout probability 1", dict(drop_p=1.0), INVALID, "conv_igemm: 0 <= dropout probability < 1"),
    ("conv_igemm", "96 input channels", dict(cin=96), UNSUPPORTED, SHAPE % (96, C, K)),
    ("conv_igemm_wgrad", "96 input channels", dict(cin=96), UNSUPPORTED, WSHAPE % (96, C, K)),
    ("conv_igemm_backward", "96 input channels", dict(cin=96), UNSUPPORTED, SHAPE % (C, 96, K)),      # (its data gradient runs cout -> cin)
]


@gpu
@pytest.mark.parametrize("name,what,args,code,text", LIB_CASES, ids=["%s-%s" % (c[0], c[1].replace(" ", "_")) for c in LIB_CASES])
def test_library_refuses(D, name, what, args, code, text):
    lib = Lib(D)
    if isinstance(text, tuple):                               # the byte count the library asks for
        text = text[0] % D.L.dsrg_conv_igemm_wgrad_workspace(text[1], B, H, W, C, C, K)
    rc = getattr(lib, name)(**{k: v(lib) if callable(v) else v for k, v in args.items()})
    assert (rc, D.L.dsrg_last_error().decode()) == (code, text)
    torch.cuda.synchronize()
    D.unchanged(name)
