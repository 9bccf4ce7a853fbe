"""CPU: the numpy restatement of csrc/sgd_pack.hip that tests/test_gpu_sgd_pack.py compares the kernel with bit for bit
(tests/sgd_pack_cases.py) is itself held against float64, against literal loops over the kernel's destination formulas, against
torch's bfloat16 cast and the project's torch packing, and — driven like trainer.CaffeSGD — against the literal Caffe rule."""
import numpy as np
import pytest
import torch

import sgd_pack_cases as K

EPS = 2.0 ** -23


@pytest.mark.parametrize("m,lr,wd", [(0.9, 0.05, 5e-4), (0.0, 0.05, 5e-4), (0.9, 0.0033, 0.0), (0.9, 1.0, 5e-3)])
def test_step32_is_within_one_rounding_per_operation_of_float64(m, lr, wd):
    """the same formula in float64 with the float32-rounded rates: |db'| <= 2^-23 (|wd w| + |d| + |m b| + |b'|) and
    |dw'| <= lr |db'| + 2^-23 (|lr b'| + |w'|) per element — one rounding (relative 2^-24) per operation, the bound twice that"""
    rng = np.random.default_rng(3)
    n = 20000
    w = (rng.standard_normal(n) * 3).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    b = (rng.standard_normal(n) * 5).astype(np.float32)
    w[:100] *= np.float32(1e-6)
    g[50:150] *= np.float32(1e4)
    w2, b2 = K.step32(w, g, b, m, lr, wd)
    assert w2.dtype == np.float32 and b2.dtype == np.float32
    M, LR, WD = (np.float64(np.float32(x)) for x in (m, lr, wd))
    W, G, B = w.astype(np.float64), g.astype(np.float64), b.astype(np.float64)
    D = G + WD * W
    B2 = M * B + D
    W2 = W - LR * B2
    db = np.abs(b2.astype(np.float64) - B2)
    bound_b = EPS * (np.abs(WD * W) + np.abs(D) + np.abs(M * B) + np.abs(B2))
    assert (db <= bound_b).all(), "momentum: %g over the bound" % (db - bound_b).max()
    dw = np.abs(w2.astype(np.float64) - W2)
    bound_w = LR * db + EPS * (np.abs(LR * B2) + np.abs(W2))
    assert (dw <= bound_w).all(), "parameter: %g over the bound" % (dw - bound_w).max()
    # and it is torch's float32 arithmetic on the CPU, bit for bit
    tw, tg, tb = torch.from_numpy(w), torch.from_numpy(g), torch.from_numpy(b)
    f = lambda x: torch.tensor(x, dtype=torch.float32)          # noqa: E731
    td = tg + f(wd) * tw
    tb2 = f(m) * tb + td
    tw2 = tw - f(lr) * tb2
    assert np.array_equal(tb2.numpy().view(np.uint32), b2.view(np.uint32)) and np.array_equal(tw2.numpy().view(np.uint32), w2.view(np.uint32))


def _literal_layouts(w):
    """four nested loops over (o, c, ky, kx) with the destination formulas of sgd_pack.hip written out"""
    cout, cin, k, _ = w.shape
    T, cbs, obs = k * k, cin // 64, cout // 64
    h = K.bf16_bits(w)
    out = {name: np.full(cout * cin * T, 0xffff, dtype=np.uint16) for name in ("igemm_fwd", "igemm_dg", "direct_fwd", "direct_dg")}
    for o in range(cout):
        ob, oq = o // 64, o % 64
        for c in range(cin):
            cb, cq = c // 64, c % 64
            for ky in range(k):
                for kx in range(k):
                    tap = ky * k + kx
                    v = h[o, c, ky, kx]
                    out["igemm_fwd"][(((ob * 64 + oq) * cbs + cb) * T + tap) * 64 + cq] = v
                    out["igemm_dg"][(((cb * 64 + cq) * obs + ob) * T + (T - 1 - tap)) * 64 + oq] = v
                    out["direct_fwd"][((ob * 64 + oq) * T + tap) * cin + cb * 64 + cq] = v
                    out["direct_dg"][((cb * 64 + cq) * T + (T - 1 - tap)) * cout + ob * 64 + oq] = v
    return out


@pytest.mark.parametrize("cout,cin,k", [(64, 64, 1), (128, 64, 3), (64, 192, 3)])
def test_layouts_equal_a_literal_loop_and_the_torch_packing(cout, cin, k):
    rng = np.random.default_rng(cout + cin + k)
    w = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
    got = K.layouts(w)
    want = _literal_layouts(w)
    for name in want:
        assert got[name].dtype == np.uint16 and got[name].size == w.size
        assert np.array_equal(got[name].reshape(-1), want[name]), name
    assert got["igemm_fwd"].shape == (cout, cin // 64, k * k, 64) and got["igemm_dg"].shape == (cin, cout // 64, k * k, 64)
    # the parameter's channels_last memory round trip the GPU cases rely on
    mem = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(-1)
    assert np.array_equal(K.memory_to_logical(mem, cout, cin, k), w)
    # the project's own torch definition, on the logical tensor in both memory layouts
    from dsrg_amd import ops
    for t in (torch.from_numpy(w), torch.from_numpy(w).contiguous(memory_format=torch.channels_last)):
        assert np.array_equal(ops.pack_conv_weight(t).view(torch.int16).numpy().view(np.uint16), got["igemm_fwd"])
        assert np.array_equal(ops.pack_conv_weight(t, for_dgrad=True).view(torch.int16).numpy().view(np.uint16), got["igemm_dg"])


def test_bf16_bits_equal_torchs_cast():
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    bits[:K.SPECIAL.size] = K.SPECIAL
    bits[K.SPECIAL.size:2 * K.SPECIAL.size] = K.SPECIAL ^ np.uint32(0x80000000)
    x = bits.view(np.float32)
    got = K.bf16_bits(x)
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert nan.sum() > 100 and (K.is_nan16(got) == nan).all() and (K.is_nan16(want) == nan).all()
    assert np.array_equal(got[~nan], want[~nan])
    sp = K.bf16_bits(K.SPECIAL.view(np.float32))
    assert sp[18] == 0x7f80 and sp[19] == 0x7f80 and sp[12] == 0x3f80 and sp[13] == 0x3f82 and sp[10] == 0 and sp[11] == 2   # overflow, ties


def test_guarded_images_name_what_differs():
    """the helper the GPU file reports with: a changed value, a changed guard word and a bf16 NaN of another payload"""
    c = K.Case("demo", [K.Spec("plain", 5, cast=1, offs=(1, 2, 3))], steps=1)
    img = c.image0
    assert img.size % 16 == 0 and c.diff(img, img.copy()) is None
    s = c.specs[0]
    assert (s.p_at % 16, s.b_at % 16, s.g_at[0] % 16, s.cast_at % 16) == (4, 8, 12, 2)
    words = img.view(np.uint32)
    inside = np.zeros(img.size, dtype=bool)
    for _, at, nb, _k in c.arena.regions:
        inside[at:at + nb] = True
        assert not inside[at - K.GUARD:at].any() and at + nb + K.GUARD <= img.size
    assert (words[~inside.reshape(-1, 4).any(1)] == K.SENTINEL).all()
    want = c.after(img, 0)
    assert np.array_equal(K.get(want, s.g_at[0], 5, np.float32), K.get(img, s.g_at[0], 5, np.float32))
    bad = want.copy()
    bad[s.b_at + 4 * 3] ^= 1
    assert "momentum: element 3 of 5" in c.diff(bad, want)
    bad = want.copy()
    bad[s.p_at + 4 * 5] ^= 1
    assert "guard byte 1 after plain[0] parameter" in c.diff(bad, want)
    bad = want.copy()
    bad[s.cast_at - 1] ^= 1
    assert "guard byte 1 before plain[0] bf16 copy" in c.diff(bad, want)
    a, b = want.copy(), want.copy()
    K.put(a, s.cast_at, np.array([0x7fc1], dtype=np.uint16))
    K.put(b, s.cast_at, np.array([0xffff], dtype=np.uint16))
    assert c.diff(a, b) is None
    K.put(b, s.cast_at, np.array([0x7f80], dtype=np.uint16))
    assert "bf16 copy: element 0 of 5" in c.diff(a, b)


def test_case_lists_are_the_ones_promised():
    assert len(K.PLAIN_SIZES) == 20 and len(K.PLAIN_OFFSETS) == 7 and sum(1 for o in K.PLAIN_OFFSETS for _ in K.plain_cases(o)) == 560
    assert sum(1 for o in K.CAST_OFFSETS for _ in K.cast_cases(o)) == 120
    assert sum(1 for s in K.PACKED_SHAPES for _ in K.packed_cases(s)) == 120 and max(s[0] * s[1] * s[2] for s in K.PACKED_SHAPES) == 256 * 128 * 9
    for pos in (15, 16, 17):
        for kind in ("igemm", "one", "nothing"):
            assert any(K.LIST_KINDS[(pos + r) % 9] == kind for r in K.LIST_ROTATIONS)
    rates = [K.list_rates(i) for i in range(40)]
    for col in (0, 1):
        nz = [r[col] for r in rates if r[col] != 0.0]
        assert len(set(np.float32(nz).tolist())) == len(nz) and 0 < len(nz) < 40
    c, bad, msg = K.refusal_case("4 taps", 18)
    assert bad == 17 and msg.endswith("(got 64, 64, 4)") and "tensor 17" in msg
    assert len(K.REFUSALS) == 11


def test_float32_restatement_driven_like_caffe_sgd_stays_near_the_literal_rule():
    """step32 under CaffeSGD's buf_lr / local_lr rescale, 11 steps with stepsize 3, against the float64 literal rule
    V <- m V + lr (g + wd W); W <- W - V: within 2 x the 5e-6 that test_caffe_sgd_matches_literal_update_across_lr_steps allows
    (measured 1.0e-6 on 5000 normal values at base_lr 0.1) — and CaffeSGD itself on CPU tensors within that of the restatement"""
    from dsrg_amd.trainer import CaffeSGD
    rng = np.random.default_rng(0)
    n, base_lr, m, wd0, gamma = 5000, 0.1, 0.9, 5e-4, 0.33
    mults = [(1.0, 1.0), (2.0, 0.0)]                       # the groups of tests/test_optimizer.py: the absolute bar belongs to their |W|
    w = [rng.standard_normal(n).astype(np.float32) for _ in mults]
    ps = [torch.from_numpy(x.copy()).requires_grad_(True) for x in w]
    opt = CaffeSGD([dict(params=[p], lr_mult=lm, decay_mult=dm) for p, (lm, dm) in zip(ps, mults)], base_lr=base_lr, momentum=m,
                   weight_decay=wd0, gamma=gamma, stepsize=3)
    b = [np.zeros(n, dtype=np.float32) for _ in mults]
    buf_lr = [None] * len(mults)
    W = [x.astype(np.float64) for x in w]
    V = [np.zeros(n) for _ in mults]
    for it in range(11):
        lr = base_lr * gamma ** (it // 3)
        for k, (lm, dm) in enumerate(mults):
            g = rng.standard_normal(n).astype(np.float32)
            ps[k].grad = torch.from_numpy(g.copy())
            local_lr, local_wd = lr * lm, wd0 * dm
            if buf_lr[k] is not None and buf_lr[k] != local_lr:
                b[k] = (torch.from_numpy(b[k]) * (buf_lr[k] / local_lr)).numpy()          # torch._foreach_mul_ with a Python scalar
            buf_lr[k] = local_lr
            w[k], b[k] = K.step32(w[k], g, b[k], m, local_lr, local_wd)
            V[k] = m * V[k] + lr * lm * (g.astype(np.float64) + wd0 * dm * W[k])
            W[k] = W[k] - V[k]
        opt.step()
    for k in range(len(mults)):
        dist = np.abs(w[k].astype(np.float64) - W[k]).max()
        print("group %d: restatement %.3g from the literal rule, |W| up to %.3g" % (k, dist, np.abs(W[k]).max()))
        assert dist < 1e-5
        assert np.abs(ps[k].detach().numpy().astype(np.float64) - w[k]).max() < 1e-5
