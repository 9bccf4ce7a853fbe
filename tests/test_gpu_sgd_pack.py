"""GPU: sgd_pack_kernel (csrc/sgd_pack.hip) bit for bit against the numpy restatement of tests/sgd_pack_cases.py, on every path
(float4, split gradient loads, scalar; the bf16 copy's stores; both packed layouts, each form alone; pack only; nothing to do), at
the sizes around its 4096-element blocks, across the sixteen-tensor launch seam with per-tensor rates, and with every tensor between
guard words that must come back untouched.  Refused lists leave memory alone.  Last, trainer.CaffeSGD on CUDA parameters against
the literal Caffe rule — the GPU twin of tests/test_optimizer.py.

Neither torch._fused_sgd_ nor pack_conv_weight_kernel is a reference here; tests/test_sgd_pack_reference.py holds the restatement
itself against float64, literal loops and torch's CPU casts."""
import numpy as np
import pytest
import torch

import sgd_pack_cases as K

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


@pytest.fixture(scope="module")
def lib(ops):
    from dsrg_amd import _lib
    return _lib.lib()


def _call(lib, case, base, step):
    a = case.args(base, step)                                     # alive until the call returns
    ad = lambda x: x.ctypes.data                                  # noqa: E731
    return lib.dsrg_sgd_pack_cast_f32(len(case.specs), ad(a["p"]), ad(a["g"]), ad(a["b"]), ad(a["fwd"]), ad(a["dg"]), ad(a["cast"]),
                                      ad(a["shape"]), ad(a["numel"]), ad(a["lr"]), ad(a["wd"]), float(case.momentum),
                                      torch.cuda.current_stream().cuda_stream or None)


def _run(lib, case):
    """every step of a case: the whole allocation after it equals the expected image"""
    dev = torch.from_numpy(case.image0).cuda()
    base = dev.data_ptr()
    assert base % 16 == 0
    want = case.image0.copy()
    for k in range(case.steps):
        rc = _call(lib, case, base, k)
        assert rc == 0, "%s, step %d: refused: %s" % (case.name, k, lib.dsrg_last_error().decode())
        case.after(want, k, inplace=True)
        msg = case.diff(dev.cpu().numpy(), want)
        assert msg is None, "step %d: %s" % (k, msg)
    return want


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("offs", K.PLAIN_OFFSETS, ids=lambda o: "p%d_b%d_g%d" % o)
def test_plain_tensors_at_every_size_and_alignment(lib, offs):
    """20 sizes around the float4 tail and the 4096-element block seams x momentum {0.9, 0} x wd {5e-4, 0}, two steps, parameter /
    momentum / gradient at these float offsets from a 16-byte boundary: parameter and momentum equal step32, the gradient and every
    guard word are untouched.  No combination is refused"""
    ran = 0
    for case in K.plain_cases(offs):
        last = _run(lib, case)
        s = case.specs[0]
        assert not np.array_equal(K.get(last, s.p_at, s.n, np.uint32), K.get(case.image0, s.p_at, s.n, np.uint32)), case.name
        ran += 1
    assert ran == len(K.PLAIN_SIZES) * len(K.PLAIN_RATES)


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("cast_off", K.CAST_OFFSETS)
def test_bf16_copy_at_every_destination_alignment(lib, cast_off):
    """the `cast` copy at 0..4 bf16 elements past an 8-byte boundary (the uint2 store and the four scalar stores), n around one
    float4 and one block, parameter aligned and one float off (the scalar path): updating, copy = bf16_bits(w'); cast only
    (g = buf = null) on the special values (ties, denormals, overflow to inf, NaNs as NaNs), parameter bits unchanged"""
    ran = 0
    for case in K.cast_cases(cast_off):
        last = _run(lib, case)
        s = case.specs[0]
        if not s.update:
            assert np.array_equal(K.get(last, s.p_at, s.n, np.uint32), np.resize(K.SPECIAL, s.n)), case.name
        ran += 1
    assert ran == 2 * 2 * len(K.CAST_SIZES)


# ---------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("shape", K.PACKED_SHAPES, ids=lambda s: "%dx%dx%d_%s" % (s[0], s[1], s[2], "direct" if s[3] else "igemm"))
def test_packed_kernels_each_form_alone_and_pack_only(lib, shape):
    """{fwd + dg, fwd only, dg only} x {update, pack only} x {gradient aligned, one float off}: parameter and momentum equal step32
    (unchanged when only packing), each present form equals layouts(w') in its guarded buffer, an absent form's pointer is null and
    nothing else is written"""
    ran = 0
    for case in K.packed_cases(shape):
        last = _run(lib, case)
        s = case.specs[0]
        same = np.array_equal(K.get(last, s.p_at, s.n, np.uint32), K.get(case.image0, s.p_at, s.n, np.uint32)) and \
            np.array_equal(K.get(last, s.b_at, s.n, np.uint32), K.get(case.image0, s.b_at, s.n, np.uint32))
        assert same == (not s.update), case.name
        ran += 1
    assert ran == 12


# ---------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("length", K.LIST_LENGTHS)
def test_lists_across_the_launch_seam_with_per_tensor_rates(lib, length):
    """lists of nine kinds of tensor in rotation (a packed kernel of 18 blocks, a one-element tensor and an entry with nothing to
    do each take positions 15, 16 and 17 in turn), every tensor with its own lr and wd (some zero), three steps: every tensor's
    bits as in a., b. and c.; the pack-only and do-nothing entries' parameter and momentum as before"""
    for r in K.LIST_ROTATIONS:
        case = K.list_case(length, r)
        last = _run(lib, case)
        for s in case.specs:
            if not s.update:
                for at in (s.p_at, s.b_at):
                    assert np.array_equal(K.get(last, at, s.n, np.uint32), K.get(case.image0, at, s.n, np.uint32)), (case.name, s.name)


# ---------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("which", sorted(K.REFUSALS))
def test_refused_lists_leave_memory_alone(lib, which):
    """a malformed tensor is refused with DSRG_ERR_INVALID and the source's message.  As tensor 0 of 3 nothing at all is written.
    As tensor 17 of 18 the first launch of sixteen HAS run when the second list is found malformed: tensors 0-15 are updated once,
    16 and 17 untouched — today's behaviour, pinned so that a change to it is a decision"""
    from dsrg_amd import _lib
    for length in (3, 18):
        case, bad, msg = K.refusal_case(which, length)
        dev = torch.from_numpy(case.image0).cuda()
        rc = _call(lib, case, dev.data_ptr(), 0)
        assert rc == _lib.ERR_INVALID, (case.name, rc)
        assert lib.dsrg_last_error().decode() == msg, case.name
        want = case.after(case.image0, 0, ran=set(range(16 * (bad // 16))))
        assert (length == 3) == np.array_equal(want, case.image0)
        diff = case.diff(dev.cpu().numpy(), want)
        assert diff is None, diff


# ---------------------------------------------------------------------------------------------------------------- f
_F_SHAPES = [   # name, shape, group, what is kept for it
    ("igemm", (128, 64, 3, 3), 0, "igemm"), ("direct", (64, 64, 3, 3), 0, "direct"), ("conv1_1", (64, 3, 3, 3), 0, "cast"),
    ("sometimes", (256,), 0, None), ("nchw_grad", (16, 16, 3, 3), 0, None), ("bias_slice", (64,), 0, None),      # the scalar path, with decay
    ("bias", (128,), 1, None), ("bf16", (512,), 1, None),
    ("fc8", (21, 256, 1, 1), 2, None)]
_F_MULTS = [(1.0, 1.0), (2.0, 0.0), (10.0, 1.0)]
_F_NOT_ELIGIBLE = ("bf16", "nchw_grad")
_F_BASE_LR, _F_M, _F_WD, _F_GAMMA, _F_STEPSIZE, _F_STEPS = 0.1, 0.9, 5e-4, 0.33, 3, 11


def _f_host():
    rng = np.random.default_rng(41)
    init = {n: (rng.standard_normal(sh) * 0.1).astype(np.float32) for n, sh, _, _ in _F_SHAPES}
    grads = [{n: (rng.standard_normal(sh) * 0.1).astype(np.float32) for n, sh, _, _ in _F_SHAPES} for _ in range(_F_STEPS)]
    for d in (init,) + tuple(grads):
        d["bf16"] = torch.from_numpy(d["bf16"]).bfloat16().float().numpy()
    for it in (2, 5):
        grads[it]["sometimes"] = None
    return init, grads


def _f_params(values):
    ps = {}
    for n, sh, _, _ in _F_SHAPES:
        v = torch.from_numpy(values[n]).cuda()
        if n == "bias_slice":
            big = torch.zeros(sh[0] + 8, device="cuda")
            t = big[1:1 + sh[0]]
            t.copy_(v)
            assert t.data_ptr() % 16 == 4
        elif n == "bf16":
            t = v.bfloat16()
        else:
            t = v.contiguous(memory_format=CL) if len(sh) == 4 else v
        ps[n] = torch.nn.Parameter(t)
    return ps


def _f_groups(ps):
    return [dict(params=[ps[n] for n, _, g, _ in _F_SHAPES if g == k], lr_mult=lm, decay_mult=dm) for k, (lm, dm) in enumerate(_F_MULTS)]


def _f_take_packs(ops, ps):
    """what the convolution nodes' forward does"""
    return {"igemm": ops.pack_conv_weight_pair(ps["igemm"], True, True), "direct": ops.pack_direct_weight_pair(ps["direct"], True),
            "conv1_1": (ops.cast_weight_kept(ps["conv1_1"]), None)}


def _f_set_grads(ps, g):
    for n, p in ps.items():
        if g[n] is None:
            p.grad = None
            continue
        t = torch.from_numpy(g[n]).cuda()
        if n == "bf16":
            t = t.bfloat16()
        elif n != "nchw_grad" and t.dim() == 4:
            t = t.contiguous(memory_format=CL)
        p.grad = t


def _h16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f_check_packs(ops, ps, ptrs):
    """every kept form equals layouts / bf16_bits of the parameter as it now lies, belongs to its version and has not moved"""
    for n in ("igemm", "direct", "conv1_1"):
        p = ps[n]
        e = ops.kept_packs(p)
        assert e is not None and e.version == p._version, n
        assert (e.fwd.data_ptr(), None if e.dg is None else e.dg.data_ptr()) == ptrs[n], n
        w = p.detach().cpu().numpy()
        if n == "conv1_1":
            assert e.kind == "cast" and np.array_equal(_h16(e.fwd), K.bf16_bits(w)), n
            continue
        L = K.layouts(w)
        if n == "igemm":
            got = (_h16(e.fwd), _h16(e.dg))
        else:                                                     # channels_last (cout, cin, 3, 3) / (cin, cout, 3, 3): memory [.][tap][.]
            got = tuple(_h16(t.permute(0, 2, 3, 1)).reshape(t.shape[0], 9, t.shape[1]) for t in (e.fwd, e.dg))
        for form, g in zip(("fwd", "dg"), got):
            want = L["%s_%s" % (e.kind, form)]
            assert g.shape == want.shape, (n, form)
            bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
            assert bad.size == 0, "%s %s pack: element %d of %d differs (%d in all)" % (n, form, bad[0], want.size, bad.size)


def test_caffe_sgd_on_the_gpu_equals_the_literal_caffe_rule(ops, monkeypatch):
    """CaffeSGD.step on CUDA parameters of the net's kinds in three groups, 11 steps across three rate changes (stepsize 3).
    Every step: the tensors handed to the kernel are exactly the eligible ones; their parameter and momentum bits equal step32 of
    what lay on the device when the kernel was called (after torch's rescale of the history); every kept form equals layouts /
    bf16_bits of the parameter, with its version, in the same buffer.  At the end every parameter is within twice the float32
    restatement's own distance of the float64 literal rule V <- m V + lr (g + wd W); W <- W - V.  A run resumed from
    state_dict() after step 4 ends on the same bits and packs.

    Measured on an MI355X (max |W_gpu - W_literal|, the restatement's distance the same to the digits shown — the kernel's tensors
    are bit-identical to it, and torch's own path agreed here too): igemm 1.353e-07, direct 1.398e-07, conv1_1 1.023e-07,
    sometimes 4.409e-08, nchw_grad 9.433e-08, bias_slice 8.747e-08, bias 1.120e-07, fc8 (lr x 10, |W| up to 4.05) 1.019e-06,
    bf16 (parameter, gradient and history in bfloat16) 5.577e-03."""
    from dsrg_amd.trainer import CaffeSGD
    init, grads = _f_host()
    ps = _f_params(init)
    opt = CaffeSGD(_f_groups(ps), base_lr=_F_BASE_LR, momentum=_F_M, weight_decay=_F_WD, gamma=_F_GAMMA, stepsize=_F_STEPSIZE)
    packs = _f_take_packs(ops, ps)
    ptrs = {n: (f.data_ptr(), None if d is None else d.data_ptr()) for n, (f, d) in packs.items()}
    _f_check_packs(ops, ps, ptrs)
    seen = []
    real = ops.sgd_pack_step

    def spy(params, gs, bufs, lrs, wds, momentum):
        seen.append(([p.detach().cpu().numpy() for p in params], [g.detach().cpu().numpy() for g in gs],
                     [b.detach().cpu().numpy() for b in bufs], list(lrs), list(wds), momentum, list(params), list(bufs)))
        return real(params, gs, bufs, lrs, wds, momentum)
    monkeypatch.setattr(ops, "sgd_pack_step", spy)

    # the float64 literal rule and the float32 restatement on the CPU, on the same gradients
    group_of = {n: g for n, _, g, _ in _F_SHAPES}
    W = {n: init[n].astype(np.float64) for n in init}
    V = {n: np.zeros_like(W[n]) for n in init}
    rw = {n: init[n].copy() for n in init}
    rb = {n: np.zeros_like(init[n]) for n in init}
    r_buf_lr = [None] * len(_F_MULTS)
    to16 = lambda a: torch.from_numpy(a).bfloat16().float().numpy()          # noqa: E731
    saved = None
    for it in range(_F_STEPS):
        lr = _F_BASE_LR * _F_GAMMA ** (it // _F_STEPSIZE)
        for k, (lm, dm) in enumerate(_F_MULTS):
            local_lr, local_wd = lr * lm, _F_WD * dm
            names = [n for n in init if group_of[n] == k]
            if r_buf_lr[k] is not None and r_buf_lr[k] != local_lr:
                for n in names:
                    rb[n] = (torch.from_numpy(rb[n]) * (r_buf_lr[k] / local_lr)).numpy()
                    if n == "bf16":
                        rb[n] = to16(rb[n])
            r_buf_lr[k] = local_lr
            for n in names:
                g = grads[it][n]
                if g is None:
                    continue
                V[n] = _F_M * V[n] + lr * lm * (g.astype(np.float64) + _F_WD * dm * W[n])
                W[n] = W[n] - V[n]
                rw[n], rb[n] = K.step32(rw[n], g, rb[n], _F_M, local_lr, local_wd)
                if n == "bf16":
                    rw[n], rb[n] = to16(rw[n]), to16(rb[n])
        _f_set_grads(ps, grads[it])
        assert opt.lr() == lr
        opt.step()
        assert len(seen) == it + 1
        w0, g0, b0, lrs, wds, m, params, bufs = seen[-1]
        want_names = [n for n, _, k, _ in sorted(_F_SHAPES, key=lambda s: s[2]) if n not in _F_NOT_ELIGIBLE and grads[it][n] is not None]
        got_names = [next(n for n in ps if ps[n] is p) for p in params]
        assert got_names == want_names, (it, got_names)
        for n, w, g, b, l, d, p, bf in zip(got_names, w0, g0, b0, lrs, wds, params, bufs):
            assert l == lr * _F_MULTS[group_of[n]][0] and d == _F_WD * _F_MULTS[group_of[n]][1], (it, n)
            w2, b2 = K.step32(w, g, b, m, l, d)
            for what, got, want in (("parameter", p, w2), ("momentum", bf, b2)):
                bad = np.flatnonzero(got.detach().cpu().numpy().view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
                assert bad.size == 0, "step %d, %s %s: element %d differs (%d of %d)" % (it, n, what, bad[0], bad.size, want.size)
        _f_check_packs(ops, ps, ptrs)
        if it == 3:                                               # four steps done: one past the first rate change
            saved = (opt.state_dict(), {n: p.detach().clone(memory_format=torch.preserve_format) for n, p in ps.items()})
    for n in init:
        gpu = np.abs(ps[n].detach().float().cpu().numpy().astype(np.float64) - W[n]).max()
        rest = np.abs(rw[n].astype(np.float64) - W[n]).max()
        print("%-10s distance from the literal rule: GPU %.3e, float32 restatement %.3e, |W| up to %.3g" % (n, gpu, rest, np.abs(W[n]).max()))
        assert rest > 0 and gpu <= 2 * rest, n
        if n not in _F_NOT_ELIGIBLE:
            assert np.array_equal(ps[n].detach().cpu().numpy().view(np.uint32), rw[n].view(np.uint32)), n
    final = {n: p.detach().clone(memory_format=torch.preserve_format) for n, p in ps.items()}
    final_packs = _f_take_packs(ops, ps)
    assert all(final_packs[n][0] is packs[n][0] for n in packs)    # the forward after the last step takes what the kernel left

    # resumed: fresh parameters and a fresh solver, the values copied in behind the version counter's back
    monkeypatch.setattr(ops, "sgd_pack_step", real)
    ps2 = _f_params({n: np.zeros_like(v) for n, v in init.items()})
    opt2 = CaffeSGD(_f_groups(ps2), base_lr=_F_BASE_LR, momentum=_F_M, weight_decay=_F_WD, gamma=_F_GAMMA, stepsize=_F_STEPSIZE)
    _f_take_packs(ops, ps2)
    for n, p in ps2.items():
        p.data.copy_(saved[1][n])
    ops.forget_weight_packs(list(ps2.values()))
    opt2.load_state_dict(saved[0])
    assert opt2.iter == 4
    for it in range(4, _F_STEPS):
        _f_set_grads(ps2, grads[it])
        _f_take_packs(ops, ps2)                                   # the forward of this step
        opt2.step()
    packs2 = _f_take_packs(ops, ps2)
    for n in init:
        a, b = ps2[n].detach(), final[n]
        assert a.stride() == b.stride() and torch.equal(a.view(torch.int16 if n == "bf16" else torch.int32), b.view(torch.int16 if n == "bf16" else torch.int32)), n
    for n in packs2:
        for x, y in zip(packs2[n], final_packs[n]):
            assert (x is None and y is None) or (x.stride() == y.stride() and torch.equal(x.view(torch.int16), y.view(torch.int16))), n
