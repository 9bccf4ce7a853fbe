"""The numpy restatement of csrc/sgd_pack.hip and the cases tests/test_gpu_sgd_pack.py runs it on (no GPU, no torch here).

The library is built with -ffp-contract=off and the kernel's update is three separately rounded float32 expressions in a fixed
order, so `step32` reproduces it bit for bit; the packed bf16 forms are index arithmetic (`layouts`) plus round-to-nearest-even
(`bf16_bits`).  tests/test_sgd_pack_reference.py holds these three against float64, literal loops and torch on the CPU.

A `Case` lays a list of tensors out in one allocation (`Arena`) whose every other word is a sentinel: parameter, momentum buffer,
one gradient per step, the packed forms and the bf16 copy each sit at a chosen misalignment between guard words.  The expected
state after a step is a whole image of that allocation, so one comparison covers the values written, the gradient that must not
be, and every guard word on both sides of every tensor."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------- the reference


def step32(w, g, b, m, lr, wd):
    """-> (w', b'): d = g + wd w; b' = m b + d; w' = w - lr b', every operation rounded to float32 (sgd4 / scalar of sgd_pack.hip);
    the rates first rounded to float32 as ops.sgd_pack_step's arrays and the C `float momentum` do"""
    m, lr, wd = np.float32(m), np.float32(lr), np.float32(wd)
    w, g, b = (np.asarray(x, dtype=np.float32) for x in (w, g, b))
    d = g + wd * w
    b2 = m * b + d
    w2 = w - lr * b2
    assert d.dtype == b2.dtype == w2.dtype == np.float32
    return w2, b2


def bf16_bits(x):
    """float32 -> the uint16 patterns of its bfloat16 rounding (nearest, ties to even, on the bit pattern); a NaN stays a NaN (quiet,
    payload's top bits kept) — compare NaNs with `is_nan16`, not by payload"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    nan = (u & 0x7fffffff) > 0x7f800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def is_nan16(h):
    return (np.asarray(h, dtype=np.uint16) & 0x7fff) > 0x7f80


def memory_to_logical(mem, cout, cin, k):
    """a channels_last (cout, cin, k, k) parameter's memory [o][ky][kx][c] -> the logical array"""
    return np.asarray(mem).reshape(cout, k, k, cin).transpose(0, 3, 1, 2)


def layouts(w):
    """logical (cout, cin, k, k) float32 -> the four packed bf16 forms as uint16 patterns: igemm_fwd [o][c/64][tap][64 c],
    igemm_dg [c][o/64][T-1-tap][64 o], direct_fwd [o][tap][c], direct_dg [c][T-1-tap][o]"""
    cout, cin, k, _ = w.shape
    T = k * k
    p = bf16_bits(np.ascontiguousarray(w.transpose(0, 2, 3, 1))).reshape(cout, T, cin)       # the parameter's channels_last memory
    f = p[:, ::-1, :].transpose(2, 1, 0)                                                    # [c][T-1-tap][o]
    return {"igemm_fwd": np.ascontiguousarray(p.reshape(cout, T, cin // 64, 64).transpose(0, 2, 1, 3)),
            "igemm_dg": np.ascontiguousarray(f.reshape(cin, T, cout // 64, 64).transpose(0, 2, 1, 3)),
            "direct_fwd": np.ascontiguousarray(p),
            "direct_dg": np.ascontiguousarray(f)}


# the values of tests/test_gpu_heads_glue.py::test_image_cast_equals_torchs_two_passes
SPECIAL = np.array([0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7f800000, 0xff800000,      # +-0, NaNs, +-inf
                    0x00000001, 0x807fffff, 0x00008000, 0x00018000,                                                       # denormals (one a tie)
                    0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7f8000, 0x7f7fffff],     # ties, neighbours, overflow
                   dtype=np.uint32)


def special_values(n):
    """SPECIAL tiled to n values, as float32"""
    return np.resize(SPECIAL, n).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- guarded memory
SENTINEL = 0x5A3CA5C3          # as bf16 halves 0xa5c3, 0x5a3c: no value the update or a rounding produces from the data used here
GUARD = 64                     # bytes of sentinel at least on either side of every tensor


class Arena(object):
    """one allocation, byte addressed: alloc() reserves a region at a chosen misalignment (bytes past a 16-byte boundary) with at
    least GUARD bytes of sentinel words before and after it"""

    def __init__(self):
        self.size = 0
        self.regions = []                                          # (name, first byte, bytes, "f32" | "bf16")

    def alloc(self, name, nbytes, misalign, kind):
        assert 0 <= misalign < 16 and kind in ("f32", "bf16")
        at = (self.size + GUARD + 15) // 16 * 16 + misalign
        self.regions.append((name, at, nbytes, kind))
        self.size = at + nbytes
        return at

    def image(self):
        """the allocation full of sentinel words, as bytes (a multiple of 16, GUARD past the last region)"""
        return np.full(((self.size + GUARD + 15) // 16 * 16) // 4, SENTINEL, dtype=np.uint32).view(np.uint8)


def put(img, at, arr):
    arr = np.ascontiguousarray(arr)
    img[at:at + arr.nbytes] = arr.reshape(-1).view(np.uint8)


def get(img, at, n, dtype):
    return img[at:at + n * np.dtype(dtype).itemsize].copy().view(dtype)


class Spec(object):
    """one tensor of a list.  n: elements; packed: None or (cout, cin, taps, plain); fwd / dg: which packed forms exist; cast: None
    or the bf16 copy's misalignment in bf16 elements; update: has a gradient; buf: has a momentum buffer; offs: misalignment of
    (parameter, momentum, gradient) in floats; lr, wd: its rates; values: the parameter's initial values or None (random).
    The rest only shapes the arguments of a call that is to be refused: null_p, numel_arg, skew = {field: bytes added to the
    pointer passed}"""

    def __init__(self, name, n, packed=None, fwd=False, dg=False, cast=None, update=True, buf=True, offs=(0, 0, 0), lr=0.01, wd=5e-4,
                 values=None, null_p=False, numel_arg=None, skew=None):
        self.name, self.n, self.packed, self.fwd, self.dg, self.cast, self.update, self.buf = name, n, packed, fwd, dg, cast, update, buf
        self.offs, self.lr, self.wd, self.values = offs, lr, wd, values
        self.null_p, self.numel_arg, self.skew = null_p, numel_arg, skew or {}
        if packed is not None:
            assert packed[0] * packed[1] * packed[2] == n


_POOL = np.random.default_rng(2024).standard_normal(1 << 22, dtype=np.float32)


class Case(object):
    """a list of tensors in one guarded allocation, `steps` gradients each, and what the allocation must hold after every step"""

    def __init__(self, name, specs, steps=2, momentum=0.9, seed=0):
        self.name, self.specs, self.steps, self.momentum = name, specs, steps, momentum
        self._cursor = (seed * 7919) % _POOL.size
        A = self.arena = Arena()
        for i, s in enumerate(specs):
            tag = "%s[%d]" % (s.name, i)
            s.p_at = A.alloc(tag + " parameter", 4 * s.n, 4 * s.offs[0], "f32")
            s.b_at = A.alloc(tag + " momentum", 4 * s.n, 4 * s.offs[1], "f32") if s.buf else None
            s.g_at = [A.alloc(tag + " gradient of step %d" % k, 4 * s.n, 4 * s.offs[2], "f32") for k in range(steps)] if s.update else None
            kind = None if s.packed is None else ("direct" if s.packed[3] else "igemm")
            s.fwd_at = A.alloc(tag + " %s forward pack" % kind, 2 * s.n, 0, "bf16") if s.fwd else None
            s.dg_at = A.alloc(tag + " %s data-gradient pack" % kind, 2 * s.n, 0, "bf16") if s.dg else None
            s.cast_at = A.alloc(tag + " bf16 copy", 2 * s.n, 2 * s.cast, "bf16") if s.cast is not None else None
        img = self.image0 = A.image()
        for s in specs:
            put(img, s.p_at, s.values if s.values is not None else self._normal(s.n))
            if s.buf:
                put(img, s.b_at, self._normal(s.n) * np.float32(0.25))
            for at in s.g_at or ():
                put(img, at, self._normal(s.n))

    def _normal(self, n):
        """n standard normal values: the next stretch of one pool drawn once (a case starts where its seed says)"""
        if self._cursor + n > _POOL.size:
            self._cursor = 0
        self._cursor += n
        return _POOL[self._cursor - n:self._cursor]

    def args(self, base, step):
        """the arrays of one dsrg_sgd_pack_cast_f32 call on the allocation at address `base` (keep them alive over the call)"""
        n = len(self.specs)
        a = {k: np.zeros(n, dtype=np.uint64) for k in ("p", "g", "b", "fwd", "dg", "cast")}
        a["shape"] = np.zeros((n, 4), dtype=np.int32)
        a["numel"] = np.zeros(n, dtype=np.int64)
        a["lr"], a["wd"] = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        for i, s in enumerate(self.specs):
            at = {"p": None if s.null_p else s.p_at, "g": s.g_at[step] if s.update else None, "b": s.b_at, "fwd": s.fwd_at, "dg": s.dg_at,
                  "cast": s.cast_at}
            for k, v in at.items():
                a[k][i] = 0 if v is None else base + v + s.skew.get(k, 0)
            if s.packed is not None:
                a["shape"][i] = s.packed
            a["numel"][i] = s.n if s.numel_arg is None else s.numel_arg
            a["lr"][i], a["wd"][i] = s.lr, s.wd
        return a

    def after(self, img, step, ran=None, inplace=False):
        """the image after step `step` from the image before it (inplace: written into it; a tensor's inputs are read before its
        outputs are written and no two tensors share a byte); ran: the tensors the call reaches (default: all)"""
        out = img if inplace else img.copy()
        for i, s in enumerate(self.specs):
            if ran is not None and i not in ran:
                continue
            w = get(img, s.p_at, s.n, np.float32)
            if s.update:
                w, b = step32(w, get(img, s.g_at[step], s.n, np.float32), get(img, s.b_at, s.n, np.float32), self.momentum, s.lr, s.wd)
                put(out, s.p_at, w)
                put(out, s.b_at, b)
            if s.fwd or s.dg:
                cout, cin, taps, plain = s.packed
                L = layouts(memory_to_logical(w, cout, cin, {1: 1, 9: 3}[taps]))
                kind = "direct" if plain else "igemm"
                if s.fwd:
                    put(out, s.fwd_at, L[kind + "_fwd"])
                if s.dg:
                    put(out, s.dg_at, L[kind + "_dg"])
            if s.cast is not None:
                put(out, s.cast_at, bf16_bits(w))
        return out

    def diff(self, got, want):
        """None if the two images agree (bf16 NaNs as NaNs), else a sentence naming the case, the tensor, the form and the first
        differing element — or the guard word next to it"""
        assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
        if np.array_equal(got, want):
            return None
        got, want = got.copy(), want.copy()
        for _, at, nb, kind in self.arena.regions:
            if kind == "bf16":
                for im in (got, want):
                    h = im[at:at + nb].view(np.uint16)             # a view: written in place
                    h[is_nan16(h)] = 0x7fc0
        bad = np.flatnonzero(got != want)
        if bad.size == 0:
            return None
        x = int(bad[0])
        for name, at, nb, kind in self.arena.regions:
            if at <= x < at + nb:
                size = 4 if kind == "f32" else 2
                e = (x - at) // size
                fmt = "0x%08x" if size == 4 else "0x%04x"
                g, w = (int(get(im, at + e * size, 1, np.uint32 if size == 4 else np.uint16)[0]) for im in (got, want))
                return "%s: %s: element %d of %d is %s, expected %s (%d bytes differ in all)" % (self.name, name, e, nb // size, fmt % g, fmt % w,
                                                                                               bad.size)
        near = min(self.arena.regions, key=lambda r: min(abs(x - r[1]), abs(x - (r[1] + r[2] - 1))))
        side = "before" if x < near[1] else "after"
        dist = near[1] - x if x < near[1] else x - (near[1] + near[2] - 1)
        return "%s: guard byte %d %s %s was written (%d bytes differ in all)" % (self.name, dist, side, near[0], bad.size)


# ---------------------------------------------------------------------------------------------------------------- 3a: plain tensors
PLAIN_SIZES = (1, 2, 3, 4, 5, 7, 8, 255, 256, 1023, 1025, 4092, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 12289)
PLAIN_OFFSETS = ((0, 0, 0), (0, 0, 1), (0, 0, 3), (1, 0, 0), (0, 2, 0), (1, 1, 1), (3, 2, 1))      # (parameter, momentum, gradient), floats
PLAIN_RATES = tuple((m, wd) for m in (0.9, 0.0) for wd in (5e-4, 0.0))


def plain_cases(offs):
    for n in PLAIN_SIZES:
        for m, wd in PLAIN_RATES:
            yield Case("plain n=%d offsets=%s momentum=%g wd=%g" % (n, offs, m, wd),
                       [Spec("plain", n, offs=offs, lr=0.05, wd=wd)], steps=2, momentum=m, seed=n)


# ---------------------------------------------------------------------------------------------------------------- 3b: the bf16 copy
CAST_OFFSETS = (0, 1, 2, 3, 4)                                    # bf16 elements: 8-, 2-, 4-, 2-, 8-byte aligned
CAST_SIZES = (1, 3, 4, 5, 4096, 4097)


def cast_cases(cast_off):
    for n in CAST_SIZES:
        for poff in (0, 1):
            yield Case("cast n=%d at +%d bf16, parameter +%d floats, updating" % (n, cast_off, poff),
                       [Spec("plain", n, cast=cast_off, offs=(poff, 0, 0), lr=0.05)], steps=2, seed=100 + n)
            yield Case("cast n=%d at +%d bf16, parameter +%d floats, cast only" % (n, cast_off, poff),
                       [Spec("plain", n, cast=cast_off, offs=(poff, 0, 0), update=False, buf=False, values=special_values(n))], steps=1)


# ---------------------------------------------------------------------------------------------------------------- 3c: packed kernels
PACKED_SHAPES = ((64, 64, 1, 0), (64, 64, 9, 0), (128, 64, 9, 0), (64, 192, 9, 0), (192, 128, 1, 0), (256, 128, 9, 0),
                 (64, 64, 9, 1), (128, 64, 9, 1), (64, 128, 9, 1), (128, 128, 9, 1))
PACKED_FORMS = ((True, True), (True, False), (False, True))       # (fwd, dg)


def packed_cases(shape):
    cout, cin, taps, plain = shape
    for fwd, dg in PACKED_FORMS:
        for update in (True, False):
            for goff in (0, 1):
                yield Case("packed %s fwd=%d dg=%d %s gradient +%d floats" % (shape, fwd, dg, "update" if update else "pack only", goff),
                           [Spec("kernel", cout * cin * taps, packed=shape, fwd=fwd, dg=dg, update=update, offs=(0, 0, goff), lr=0.05)],
                           steps=2 if update else 1, seed=cout + cin + taps)


# ---------------------------------------------------------------------------------------------------------------- 3d: lists
LIST_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 40)
LIST_KINDS = ("igemm", "bias", "plain4097", "one", "direct", "cast", "slice21", "packonly", "nothing")
# the rotations of the cycle that put a packed kernel (kind 0), the one-element tensor (3) and the do-nothing entry (8) at
# positions 15, 16 and 17 in turn: tensor i is kind (i + r) % 9
LIST_ROTATIONS = tuple(sorted({(k - pos) % 9 for k in (0, 3, 8) for pos in (15, 16, 17)}))


def list_rates(i):
    """tensor i's own (lr, wd): distinct non-zero values and some zeros"""
    return (0.0 if i % 7 == 3 else 0.01 * (1 + 0.37 * i)), (0.0 if i % 5 == 2 else 1e-4 * (1 + i))


def list_spec(kind, i):
    lr, wd = list_rates(i)
    if kind == "igemm":                                           # 2 x 1 x 9 = 18 blocks
        return Spec(kind, 128 * 64 * 9, packed=(128, 64, 9, 0), fwd=True, dg=True, lr=lr, wd=wd)
    if kind == "bias":
        return Spec(kind, 64, lr=lr, wd=wd)
    if kind == "plain4097":                                       # two blocks
        return Spec(kind, 4097, lr=lr, wd=wd)
    if kind == "one":
        return Spec(kind, 1, lr=lr, wd=wd)
    if kind == "direct":
        return Spec(kind, 64 * 64 * 9, packed=(64, 64, 9, 1), fwd=True, dg=True, lr=lr, wd=wd)
    if kind == "cast":                                            # conv1_1
        return Spec(kind, 64 * 3 * 9, cast=0, lr=lr, wd=wd)
    if kind == "slice21":
        return Spec(kind, 21, offs=(1, 1, 1), lr=lr, wd=wd)
    if kind == "packonly":
        return Spec(kind, 64 * 64, packed=(64, 64, 1, 0), fwd=True, dg=True, update=False, lr=lr, wd=wd)
    assert kind == "nothing"
    return Spec(kind, 100, update=False, lr=lr, wd=wd)


def list_case(length, rotation):
    kinds = [LIST_KINDS[(i + rotation) % 9] for i in range(length)]
    return Case("list of %d, rotation %d" % (length, rotation), [list_spec(k, i) for i, k in enumerate(kinds)], steps=3, seed=1000 + 9 * length + rotation)


# ---------------------------------------------------------------------------------------------------------------- 3e: refusals
MSG_BASIC = "sgd_pack: tensor %d: null parameter, bad size or a gradient without a momentum buffer"
MSG_ALIGN = "sgd_pack: tensor %d is not aligned (4 bytes; parameter and momentum of a packed kernel: 16)"
MSG_SHAPE = "sgd_pack: tensor %d: a packed kernel needs 64 | cout, 64 | cin, 1 or 9 taps (got %u, %u, %u)"
MSG_CAST = "sgd_pack: tensor %d: a bf16 copy goes with a tensor without packed forms, 2-byte aligned"

_K = dict(packed=(64, 64, 9, 0), fwd=True, dg=True)
REFUSALS = {   # name -> (Spec keywords (n first), message, its arguments after the index)
    "null parameter": (dict(n=64, null_p=True), MSG_BASIC, ()),
    "numel 0": (dict(n=64, numel_arg=0), MSG_BASIC, ()),
    "numel 2^31": (dict(n=64, numel_arg=2 ** 31), MSG_BASIC, ()),
    "gradient without momentum": (dict(n=64, buf=False), MSG_BASIC, ()),
    "float pointer off by 2 bytes": (dict(n=64, skew={"g": 2}), MSG_ALIGN, ()),
    "cin 96": (dict(n=64 * 96 * 9, fwd=True, dg=True, packed=(64, 96, 9, 0)), MSG_SHAPE, (64, 96, 9)),
    "4 taps": (dict(n=64 * 64 * 4, fwd=True, dg=True, packed=(64, 64, 4, 0)), MSG_SHAPE, (64, 64, 4)),
    "cout cin taps != numel": (dict(n=64 * 64 * 9, numel_arg=64 * 64 * 9 - 64, **_K), MSG_SHAPE, (64, 64, 9)),
    "packed kernel, parameter 4-byte aligned": (dict(n=64 * 64 * 9, offs=(1, 0, 0), **_K), MSG_ALIGN, ()),
    "cast with fwd": (dict(n=64 * 64 * 9, cast=0, **_K), MSG_CAST, ()),
    "odd cast address": (dict(n=64, cast=0, skew={"cast": 1}), MSG_CAST, ()),
}


def refusal_case(which, length):
    """-> (Case, index of the refused tensor, the message expected): the refused tensor is tensor 0 of a list of 3 (length 3) or
    the last of a longer list (tensor 17 of 18), the others good plain tensors"""
    kw, msg, extra = REFUSALS[which]
    bad = 0 if length == 3 else length - 1
    specs = []
    for i in range(length):
        lr, wd = list_rates(i)
        specs.append(Spec("refused: " + which, lr=lr, wd=wd, **kw) if i == bad else Spec("good", 300 + i, lr=lr, wd=wd))
    return Case("refusal of %s as tensor %d of %d" % (which, bad, length), specs, steps=1, seed=bad), bad, msg % ((bad,) + extra)
