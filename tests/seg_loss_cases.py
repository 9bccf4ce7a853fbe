"""The contract of dsrg_seg_loss_zoom_batch (include/dsrg_hip.h) restated in NumPy, the float64 reference it is judged against,
and the inputs tests/test_seg_loss.py and tests/test_train_f_loss_at.py share.  Nothing here needs a GPU.

The restatement follows the contract operation for operation — the zoom of eval_confusion_cases, m, e_c = exp(z_c - m), s summed
in float32 with c ascending, r = 1 / s, p_c = e_c * r, the float32 weights and the product (wy * wx) * (p_c - [c == label]) — except
for the ORDER of the gradient's sum, which the contract leaves to the kernel: the products are summed in float64 here and rounded
once.  On data whose sums are exact in any order (test_seg_loss.py, "exact data") that is the kernel's result bit for bit;
elsewhere both are compared with the float64 reference.

The reference: torch on the CPU in float64, F.interpolate(bilinear, align_corners=True) -> cross_entropy(reduction="sum",
ignore_index=255) / max(N, 1) with autograd, labels that are neither a class nor 255 mapped to 255 first."""
import functools

import numpy as np

import eval_confusion_cases as K

IGNORE = 255.0

# (B, C, h, w, H, W): one pixel; one source sample (scale 0); identity; out == 1 on one axis; shrinking (cells with an empty footprint);
# factor 8; a non-integral factor; factor 8 over several tiles each way (19 rows: 4 + 4 + 4 + 4 + 3, 18 columns: 6 + 6 + 6); the
# label limit; 81 labels; and, beyond the issue's list, a factor so large that a tile's pixels take several chunks each way (150
# columns: more than a chunk's 128; 70 x 128 pixels: more than a chunk parks)
CASES = [(1, 1, 1, 1, 1, 1), (2, 2, 1, 1, 5, 7), (2, 3, 3, 4, 3, 4), (2, 5, 4, 3, 1, 9), (2, 21, 9, 9, 5, 4), (3, 21, 5, 6, 33, 41),
         (2, 21, 7, 5, 30, 23), (2, 21, 19, 18, 145, 137), (1, 96, 6, 5, 41, 33), (2, 81, 5, 5, 33, 33), (1, 3, 2, 3, 70, 150)]
# (B, 2, h, w, H, W) with H - 1 = 8 (h - 1) or 4 (h - 1): every blend weight is a multiple of 1/8
EXACT_CASES = [(2, 2, 3, 2, 9, 5), (1, 2, 19, 18, 145, 137)]


def _seed(case):
    return 1000 + sum(int(v) * k for v, k in zip(case, (1, 3, 7, 11, 13, 17)))


def case_id(case):
    return "%dx%dx%dx%d-%dx%d" % case


@functools.lru_cache(maxsize=None)
def make_case(case, ties=False):
    """-> (logits (B, C, h, w) float32: 3 * standard normal (ties: eval_confusion_cases.make_scores' tied integer planes), labels
    (B, 1, H, W) float32 of eval_confusion_cases.make_labels: a 255 rectangle, values C and 200, image 1 wholly ignored).  Shared:
    callers do not write to them"""
    B, C, h, w, H, W = case
    rng = np.random.default_rng(_seed(case) + (7 if ties else 0))
    logits = K.make_scores(rng, B, C, h, w, ties)
    if not ties:
        logits = (np.float32(3.0) * logits).astype(np.float32)
    labels = K.make_labels(rng, B, C, H, W)
    logits.setflags(write=False)
    labels.setflags(write=False)
    return logits, labels


@functools.lru_cache(maxsize=None)
def make_exact_case(case):
    """two equal planes of small integers and labels that are all valid: p = 0.5 everywhere"""
    B, C, h, w, H, W = case
    rng = np.random.default_rng(_seed(case) + 3)
    logits = rng.integers(-3, 4, (B, 1, h, w)).astype(np.float32).repeat(2, axis=1)
    labels = rng.integers(0, 2, (B, 1, H, W)).astype(np.float32)
    logits.setflags(write=False)
    labels.setflags(write=False)
    return logits, labels


def classify(labels, C, ignore_label=IGNORE):
    """labels (...) float32 -> (valid, invalid) boolean masks; ignore_label is neither"""
    lab = np.asarray(labels, dtype=np.float32)
    ignored = lab == np.float32(ignore_label)
    with np.errstate(invalid="ignore"):
        exact = (lab >= 0) & (lab < np.float32(C)) & (np.floor(lab) == lab)
    return exact & ~ignored, ~exact & ~ignored


def _axis_weights(n_in, n_out):
    """-> [(cell index (n_out), float32 weight (n_out), mask (n_out))]: the cells an output coordinate adds to.  Where both taps
    are one cell (the last source sample, or a one-sample axis) the weight is float32(l0) + float32(l1), a float32 sum"""
    i0, i1, l0, l1 = K.axis_taps(n_in, n_out)
    l0, l1 = l0.astype(np.float32), l1.astype(np.float32)
    same = i1 == i0
    first = np.where(same, (l0 + l1).astype(np.float32), l0)
    return [(i0, first, np.ones(n_out, dtype=bool)), (i1, l1, ~same)]


def seg_loss(logits, labels, ignore_label=IGNORE, B=None):
    """logits (>= B, C, h, w) f32, labels (B, 1, H, W) f32 -> (loss float32, grad (B, C, h, w) float32, [valid, correct, invalid])"""
    logits = np.asarray(logits, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.float32)
    B = labels.shape[0] if B is None else B
    C, h, w = logits.shape[1:]
    H, W = labels.shape[-2:]
    f32, one = np.float32, np.float32(1.0)
    S = np.zeros((B, C, h, w), dtype=np.float64)
    total, n_valid, n_correct, n_invalid = 0.0, 0, 0, 0
    ty, tx = _axis_weights(h, H), _axis_weights(w, W)
    for b in range(B):
        lab = labels[b].reshape(H, W)
        valid, invalid = classify(lab, C, ignore_label)
        n_invalid += int(invalid.sum())
        z = K.zoom(logits[b], H, W)                                               # (C, H, W) float32
        m = z.max(axis=0)
        e = np.exp((z - m[None]).astype(f32)).astype(f32)
        s = np.zeros((H, W), dtype=f32)
        for c in range(C):                                                        # float32, c ascending
            s = (s + e[c]).astype(f32)
        r = (one / s).astype(f32)
        g = np.where(valid, lab, 0).astype(np.int64)
        zl = np.take_along_axis(z, g[None], axis=0)[0]
        ell = (np.log(s).astype(f32) - (zl - m).astype(f32)).astype(f32)
        total += float(ell[valid].astype(np.float64).sum())
        n_valid += int(valid.sum())
        n_correct += int((np.argmax(z, axis=0)[valid] == g[valid]).sum())
        d = (e * r[None]).astype(f32)
        d = (d - (np.arange(C)[:, None, None] == g[None]).astype(f32)).astype(f32)
        d[:, ~valid] = 0.0
        for iy, wy, my in ty:
            for ix, wx, mx in tx:
                wgt = (wy[:, None] * wx[None, :]).astype(f32)                     # (wy * wx) in float32
                con = (wgt[None] * d).astype(f32).astype(np.float64)             # ... * (p - [c == label]) in float32
                con[:, ~(my[:, None] & mx[None, :])] = 0.0
                np.add.at(S[b], (slice(None), iy[:, None], ix[None, :]), con)
    den = max(n_valid, 1)
    grad = (S.astype(f32) / f32(den)).astype(f32)
    return f32(total / den), grad, [n_valid, n_correct, n_invalid]


def torch_reference(logits, labels, dtype, ignore_label=IGNORE, B=None):
    """the torch composition on the CPU in `dtype` -> (loss, grad (B, C, h, w)) as float64 arrays"""
    import torch
    import torch.nn.functional as F
    labels = np.asarray(labels, dtype=np.float32)
    B = labels.shape[0] if B is None else B
    H, W = labels.shape[-2:]
    C = logits.shape[1]
    valid, _ = classify(labels.reshape(-1, H, W)[:B], C, ignore_label)
    lab = torch.from_numpy(np.where(valid, labels.reshape(-1, H, W)[:B], 255).astype(np.int64))
    x = torch.from_numpy(np.array(logits[:B])).to(dtype).requires_grad_(True)
    z = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
    loss = F.cross_entropy(z, lab, reduction="sum", ignore_index=255) / max(int(valid.sum()), 1)
    loss.backward()
    return float(loss.detach().double()), x.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (l64, g64, e32) of make_case(case): the float64 reference and the relative error max|g32 - g64| / max|g64| of the float32
    torch composition on the same input (0 where the gradient is zero)"""
    import torch
    logits, labels = make_case(case)
    l64, g64 = torch_reference(logits, labels, torch.float64)
    _, g32 = torch_reference(logits, labels, torch.float32)
    top = float(np.abs(g64).max())
    return l64, g64, (float(np.abs(g32 - g64).max()) / top if top > 0 else 0.0)


def grad_bound(case):
    """the issue's bound on max|grad - g64|: max(4 * e32, 16 * 2^-24) * max|g64|"""
    _, g64, e32 = reference(case)
    return max(4.0 * e32, 16.0 * 2.0 ** -24) * float(np.abs(g64).max())
