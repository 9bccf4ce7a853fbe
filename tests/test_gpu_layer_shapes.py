"""The stand-alone layer kernels of csrc/layers.hip — softmax forward / backward, balanced seed loss, constrain loss, CRF layer
backward: what ops.supervision_step runs layer by layer for maps beyond the LDS path — over label counts 1..96 and blob sizes
away from the default 21 x 41 x 41 (shapes and inputs: tests/layer_shape_cases.py), each at logits of spread 1, 10 and 40.

On the GPU, against the oracle with the bars of test_gpu_parity.py's test_softmax_forward_backward and
test_losses_forward_backward (both sides follow the reference's float32 order, which is why the kernels are held to the
oracle and not to float64); then the layer-by-layer step itself with 22 and 96 labels at 67 x 67, the first map beyond the
LDS path.  Without a GPU: the oracle on the same inputs against float64 autograd, as tests/test_oracle_layers.py does at
its one shape."""
import numpy as np
import pytest
import torch

import layer_shape_cases as K
from test_gpu_parity import _check_fused_step

gpu = pytest.mark.gpu
CASES = [(s, v) for s in K.SHAPES for v in K.SPREADS]
CASE_IDS = ["%s-spread%d" % (i, v) for i in K.ids() for v in K.SPREADS]

# max |oracle softmax - float64 softmax| measured per label count over the shapes and the three spreads (the oracle sums
# float32 terms in label order, so the distance grows with the label count); the companion's bar is twice this
F64_SOFTMAX = {1: 0.0, 2: 8.8e-8, 3: 9.1e-8, 4: 1.1e-7, 5: 1.4e-7, 16: 3.2e-7, 17: 3.3e-7, 20: 3.2e-7, 21: 3.8e-7, 22: 3.9e-7,
               23: 3.8e-7, 64: 1.1e-6, 95: 1.6e-6, 96: 1.6e-6}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ops():
    from dsrg_amd import ops, _lib
    _lib.require_gpu()
    return ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a)).to("cuda", dtype)              # a copy: the cached inputs are read-only


def _softmax_t(x):
    s = torch.softmax(x, dim=1) + 1e-4
    return s / s.sum(1, keepdim=True)


# ---- without a GPU: the oracle against float64 autograd --------------------------------------------------------------------
@pytest.mark.parametrize("shape,spread", CASES, ids=CASE_IDS)
def test_oracle_softmax_vs_float64(O, shape, spread):
    """measured: forward at most 1.6e-6 from float64 at 95 / 96 labels, 1.1e-6 at 64, at most 3.9e-7 at 23 or fewer (the table
    F64_SOFTMAX; the bar is twice the entry); backward (the oracle forms it in float64) at most 5.1e-8, under the 1e-6 of
    tests/test_oracle_layers.py"""
    d = K.inputs(shape, spread)
    x = d["logits"]
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pt = _softmax_t(xt)
    err = np.abs(O.softmax_forward(x) - pt.detach().numpy()).max()
    print("softmax forward, %d labels: %.2e from float64" % (shape[1], err))
    assert err <= 2 * F64_SOFTMAX[shape[1]]
    (pt * torch.tensor(d["g"], dtype=torch.float64)).sum().backward()
    assert np.abs(O.softmax_backward(x, d["g"]) - xt.grad.numpy()).max() < 1e-6
    if spread == 40.0 and shape[1] >= 2:
        assert (torch.softmax(xt, 1) < 1e-4).any(), "the 1e-4 floor is not reached"


@pytest.mark.parametrize("shape,spread", CASES, ids=CASE_IDS)
def test_oracle_losses_vs_float64(O, shape, spread):
    """bars of tests/test_oracle_layers.py; the constrain-loss gradients relative to their largest value where that exceeds 1
    (blobs of a few pixels: the gradient is (q / p) / (B HW), up to 20 / (B HW), and the oracle returns float32)"""
    d = K.inputs(shape, spread)
    B, C = shape[:2]
    p = O.softmax_forward(d["logits"])
    cues = d["cues"]
    loss, grad = O.seed_loss(p, cues)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    St = torch.tensor(cues, dtype=torch.float64)
    cb = St[:, 0].sum((1, 2), keepdim=True)
    lt = -((St[:, 0] * torch.log(pt[:, 0])).sum((1, 2), keepdim=True) / torch.clamp(cb, min=1e-4)).mean()
    if C > 1:
        cf = St[:, 1:].sum((1, 2, 3), keepdim=True)
        lt = lt - ((St[:, 1:] * torch.log(pt[:, 1:])).sum((1, 2, 3), keepdim=True) / torch.clamp(cf, min=1e-4)).mean()
    lt.backward()
    assert abs(loss - lt.item()) < 1e-9 * max(1, abs(lt.item()))
    assert np.abs(grad - pt.grad.numpy()).max() < 1e-5 * max(1.0, np.abs(pt.grad.numpy()).max())

    lq = K.logq_of(O, d, p)
    loss, gp, gq = O.constrain_loss(p, lq)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    qt = torch.tensor(lq, dtype=torch.float64, requires_grad=True)
    L = (torch.exp(qt) * torch.log(torch.clamp(torch.exp(qt) / pt, 0.05, 20.0))).sum(1).mean()
    L.backward()
    assert abs(loss - L.item()) < 1e-9 * max(1, abs(L.item()))
    r, near, clipped = K.clip_census(p, lq)
    safe = ~near
    assert np.abs(gp - pt.grad.numpy())[safe].max() < 1e-7 * max(1.0, np.abs(pt.grad.numpy()).max())
    assert np.abs(gq - qt.grad.numpy())[safe].max() < 1e-7 * max(1.0, np.abs(qt.grad.numpy()).max())


@pytest.mark.parametrize("shape,spread", CASES, ids=CASE_IDS)
def test_constrain_loss_clips_enough(O, shape, spread):
    """at most 0.1 % of the constrain-loss terms within rounding of a clip bound (measured: 1 element at 1x21x13x15 and at
    3x96x6x11, spread 1; else none) and, with three labels or more, at least 1 % clipped.  Measured clipped shares with noise
    8: 83-88 % at spread 1 and 16 labels or more, 39-64 % below; 5-29 % at spread 10; 1.03-10 % at spread 40 — except
    1x95x4x16 and 3x96x6x11, which clip 0.74 % and 1.06 % at spread 40 with noise 8: their noise is 16
    (layer_shape_cases.NOISE), which gives 1.25 % and 1.55 % there (5.4 % and 5.5 % at spread 10, 87 % at spread 1)."""
    d = K.inputs(shape, spread)
    p = O.softmax_forward(d["logits"])
    r, near, clipped = K.clip_census(p, K.logq_of(O, d, p))
    print("%s spread %g: %d of %d near a bound, %.2f %% clipped" % (shape, spread, near.sum(), near.size, 100 * clipped.mean()))
    assert near.mean() <= 1e-3
    if shape[1] >= 3:
        assert clipped.mean() >= 0.01


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,spread", CASES, ids=CASE_IDS)
def test_softmax_kernels_vs_oracle(ops, O, shape, spread):
    """softmax_fwd_kernel<21> / <kMaxLabels> and softmax_bwd_kernel<21> / <kMaxLabels> (the latter at 22, 23, 64, 95 and 96
    labels: no other test launches it)"""
    d = K.inputs(shape, spread)
    x, g = d["logits"], d["g"]
    dx_, dg_ = dev(x), dev(g)
    p = ops.softmax_forward(dx_)
    want = O.softmax_forward(x)
    assert np.abs(p.cpu().numpy() - want).max() < 1e-6
    if spread == 40.0 and shape[1] >= 2:
        s = torch.softmax(torch.tensor(x, dtype=torch.float64), 1)
        assert (s < 1e-4).any(), "the 1e-4 floor is not reached"
    dx = ops.softmax_backward(dx_, dg_)
    want = O.softmax_backward(x, g)
    assert np.abs(dx.cpu().numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    assert torch.equal(ops.softmax_forward(dx_), p) and torch.equal(ops.softmax_backward(dx_, dg_), dx)


@gpu
@pytest.mark.parametrize("shape,spread", CASES, ids=CASE_IDS)
def test_loss_kernels_vs_oracle(ops, O, shape, spread):
    """seed_loss (the C * HW walk in strides of 4 x 1024, its clamped tail, the split at index HW, images without background /
    foreground cues), constrain_loss (reduction and gradients, the near-a-clip-bound rule of test_losses_forward_backward)
    and crf_layer_backward, which must equal float32((1 - refined) * g) formed in float64: the kernel's own formula"""
    d = K.inputs(shape, spread)
    B, C, H, W = shape
    p = O.softmax_forward(d["logits"])
    seeds = d["cues"]
    dp_, ds_ = dev(p), dev(seeds)
    loss, grad = ops.seed_loss(dp_, ds_)
    wl, wg = O.seed_loss(p, seeds)
    assert abs(loss.item() - wl) < 1e-5 * max(1, abs(wl))
    assert np.abs(grad.cpu().numpy() - wg).max() < 1e-5 * max(1.0, np.abs(wg).max())
    again = ops.seed_loss(dp_, ds_)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grad)

    lq = K.logq_of(O, d, p)
    dq_ = dev(lq)
    loss, gp, gq = ops.constrain_loss(dp_, dq_)
    wl, wgp, wgq = O.constrain_loss(p, lq)
    assert abs(loss.item() - wl) < 1e-5 * max(1, abs(wl))
    r, near, clipped = K.clip_census(p, lq)
    qd = np.exp(lq.astype(np.float64))
    safe = ~near
    gpn, gqn = gp.cpu().numpy(), gq.cpu().numpy()
    assert np.abs(gpn - wgp)[safe].max() < 1e-6
    assert np.abs(gqn - wgq)[safe].max() < 1e-6
    if near.any():                       # either branch, but exactly one of them (test_losses_forward_backward)
        n = B * H * W
        bound = np.where(np.abs(r - 0.05) <= 1e-5, 0.05, 20.0)
        in_p, in_q = -(qd / p) / n, (qd * np.log(np.clip(r, 0.05, 20.0)) + qd) / n
        out_p, out_q = np.zeros_like(in_p), qd * np.log(bound) / n
        ok_p = np.minimum(np.abs(gpn - in_p), np.abs(gpn - out_p)) < 1e-6
        ok_q = np.minimum(np.abs(gqn - in_q), np.abs(gqn - out_q)) < 1e-6
        assert ok_p[near].all() and ok_q[near].all()
    again = ops.constrain_loss(dp_, dq_)
    assert all(torch.equal(a, b) for a, b in zip(again, (loss, gp, gq)))

    refined = qd                                                    # float64 marginals whose float32 logarithm is lq
    back = ops.crf_layer_backward(dev(refined, torch.float64), gq)
    want = ((1.0 - refined) * gqn.astype(np.float64)).astype(np.float32)
    assert np.array_equal(back.cpu().numpy(), want)
    assert np.array_equal(back.cpu().numpy(), O.crf_layer_backward(refined, gqn))
    assert torch.equal(ops.crf_layer_backward(dev(refined, torch.float64), gq), back)


@gpu
@pytest.mark.parametrize("B,C", [(3, 22), (2, 96)])
def test_layer_by_layer_step_with_more_than_21_labels(ops, O, B, C):
    """ops.supervision_step on the global-memory path (67 x 67 = 4489 pixels, one beyond the LDS path) with more than 21
    labels: softmax forward, full-resolution CRF, SRG, both losses, CRF backward and softmax_bwd_kernel<kMaxLabels> in
    sequence, against the oracle layer by layer; inputs as in test_fused_step_other_shapes_vs_oracle"""
    from dsrg_amd import synthetic as S
    H = W = 67
    assert not ops.lds_path_supports(H, W) and ops.lds_path_supports(66, 68)
    rng = np.random.default_rng(B * 1000 + C)
    images = S.make_images(rng, B, size=8 * (H - 1) + 1)
    logits = S.make_logits(rng, B, C, H, W)
    labels, cues = S.make_labels_cues(rng, B, C, H, W)
    _check_fused_step(ops, O, logits, images, labels, cues, "layer by layer B=%d C=%d %dx%d" % (B, C, H, W))
