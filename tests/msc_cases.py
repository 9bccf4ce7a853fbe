"""The contract of dsrg_msc_loss_batch and dsrg_msc_pyramid_batch (include/dsrg_hip.h) restated in NumPy, the float64 reference the
loss is judged against, and the inputs tests/test_msc_loss.py and tests/test_train_f_msc.py share.  Nothing here needs a GPU.

The restatement follows the contract operation for operation — the label sampling in integers, the zoom of eval_confusion_cases,
the maximum with its lowest-index winner, every head's m, e_c = exp(z_c - m), s summed in float32 with c ascending, r = 1 / s,
d_c = e_c * r - [c == label], the float32 weights and the product (wy * wx) * d_f — except for the ORDER of the gather's sum, which
the contract leaves to the kernel: the products are summed in float64 here and rounded once.  On data whose sums are exact in any
order (test_msc_loss.py, "exact data") that is the kernel's result bit for bit; elsewhere both are compared with the float64
reference.

The reference: torch on the CPU in float64, F.interpolate(bilinear, align_corners=True) -> stack().max(0) -> S + 1 times
cross_entropy(reduction="sum", ignore_index=255) / max(N, 1), summed, with autograd; labels that are neither a class nor 255 mapped
to 255 first.

The maximum is discontinuous: a float32 rounding of a blend may hand a cell's gradient to another scale.  make_case therefore walks
seeds until the float64 reference's smallest gap between the two largest u_s,c is at least 2^-15 (32 float32 ulps below 16) and every
|score| is below 16, and asserts both."""
import functools

import numpy as np

import eval_confusion_cases as K
import seg_loss_cases as SL

IGNORE = 255.0
MIN_GAP = 2.0 ** -15
MAX_SEEDS = 64

# (B, C, maps, H, W): one pixel; tiny odd maps; crop 65 through VGG; identity zoom; a map larger than map 0 (cells with empty
# footprints); several workgroups each way; the label limit; S = 4 at 81 labels; the workload's own shape
CASES = [(1, 1, ((1, 1), (1, 1)), 1, 1),
         (2, 3, ((3, 4), (2, 3), (1, 2)), 17, 25),
         (2, 21, ((9, 9), (7, 7), (5, 5)), 65, 65),
         (2, 21, ((5, 7), (5, 7), (5, 7)), 33, 49),
         (2, 21, ((5, 6), (7, 9)), 33, 41),
         (2, 21, ((19, 18), (14, 13), (9, 9)), 145, 137),
         (1, 96, ((6, 5), (5, 4)), 41, 33),
         (2, 81, ((9, 9), (7, 7), (5, 5), (3, 3)), 65, 65),
         (2, 21, ((41, 41), (31, 31), (21, 21)), 321, 321)]
# (B, 2, maps, H, W) whose blend weights are all dyadic: (9 - 1) = 2 (5 - 1) = 4 (3 - 1)
EXACT_CASES = [(2, 2, ((9, 9), (5, 5), (3, 3)), 65, 65), (1, 2, ((5, 5), (3, 3)), 65, 65)]


def case_id(case):
    B, C, maps, H, W = case
    return "%dx%d-%s-%dx%d" % (B, C, "_".join("%dx%d" % m for m in maps), H, W)


def _seed(case):
    B, C, maps, H, W = case
    return 5000 + B + 3 * C + 17 * H + 13 * W + sum((7 + 4 * k) * h + (11 + 2 * k) * w for k, (h, w) in enumerate(maps))


def label_index(n, N):
    """the label coordinates of an axis of n cells under N labels: (2 i (N - 1) + (n - 1)) // (2 (n - 1)), 0 when n == 1"""
    i = np.arange(n, dtype=np.int64)
    return (2 * i * (N - 1) + (n - 1)) // (2 * (n - 1)) if n > 1 else np.zeros(1, dtype=np.int64)


def sample_labels(labels, h, w):
    """(B, 1, H, W) -> (B, h, w): the nearest sample at the align-corners position"""
    lab = np.asarray(labels, dtype=np.float32)
    H, W = lab.shape[-2:]
    return lab.reshape(-1, H, W)[:, label_index(h, H)][:, :, label_index(w, W)]


def fused_gap(maps):
    """the smallest gap between the two largest u_s,c of the float64 reference's zoomed maps"""
    import torch
    import torch.nn.functional as F
    h0, w0 = maps[0].shape[-2:]
    u = [torch.from_numpy(np.array(maps[0])).double()]
    for m in maps[1:]:
        u.append(F.interpolate(torch.from_numpy(np.array(m)).double(), size=(h0, w0), mode="bilinear", align_corners=True))
    top = torch.stack(u).topk(2, dim=0).values
    return float((top[0] - top[1]).min())


def _draw(case, seed):
    B, C, sizes, H, W = case
    rng = np.random.default_rng(seed)
    maps = [(np.float32(3.0) * K.make_scores(rng, B, C, h, w, False)).astype(np.float32) for h, w in sizes]
    return maps, K.make_labels(rng, B, C, H, W)


@functools.lru_cache(maxsize=None)
def make_case(case):
    """-> (maps: tuple of (B, C, h_s, w_s) float32, 3 * standard normal; labels (B, 1, H, W) float32 of
    eval_confusion_cases.make_labels: a 255 rectangle, values C and 200, image 1 wholly ignored; the seed's offset).  The first
    seed without a near-tie is taken.  Shared: callers do not write to them"""
    for k in range(MAX_SEEDS):
        maps, labels = _draw(case, _seed(case) + 1009 * k)
        if max(float(np.abs(m).max()) for m in maps) < 16.0 and fused_gap(maps) >= MIN_GAP:
            break
    else:
        raise AssertionError("no seed without a near-tie among %d for %s" % (MAX_SEEDS, case_id(case)))
    assert fused_gap(maps) >= MIN_GAP and all(float(np.abs(m).max()) < 16.0 for m in maps)
    for a in maps + [labels]:
        a.setflags(write=False)
    return tuple(maps), labels, k


@functools.lru_cache(maxsize=None)
def make_exact_case(case):
    """two equal planes of integers in -3..3 per map and labels that are all valid: every head's p is 0.5 everywhere, the scales
    tie often, and every weight is dyadic"""
    B, C, sizes, H, W = case
    rng = np.random.default_rng(_seed(case) + 3)
    maps = [rng.integers(-3, 4, (B, 1, h, w)).astype(np.float32).repeat(2, axis=1) for h, w in sizes]
    labels = rng.integers(0, 2, (B, 1, H, W)).astype(np.float32)
    for a in maps + [labels]:
        a.setflags(write=False)
    return tuple(maps), labels


def _head(z, lab, C, ignore_label):
    """one head on one image: z (C, h, w) f32, lab (h, w) f32 -> (sum of the loss terms (float64), d (C, h, w) f32, valid, invalid,
    correct)"""
    f32, one = np.float32, np.float32(1.0)
    valid, invalid = SL.classify(lab, C, ignore_label)
    m = z.max(axis=0)
    e = np.exp((z - m[None]).astype(f32)).astype(f32)
    s = np.zeros(z.shape[1:], dtype=f32)
    for c in range(C):                                                            # float32, c ascending
        s = (s + e[c]).astype(f32)
    r = (one / s).astype(f32)
    g = np.where(valid, lab, 0).astype(np.int64)
    zl = np.take_along_axis(z, g[None], axis=0)[0]
    ell = (np.log(s).astype(f32) - (zl - m).astype(f32)).astype(f32)
    d = (e * r[None]).astype(f32)
    d = (d - (np.arange(C)[:, None, None] == g[None]).astype(f32)).astype(f32)
    d[:, ~valid] = 0.0
    correct = int((np.argmax(z, axis=0)[valid] == g[valid]).sum())
    return float(ell[valid].astype(np.float64).sum()), d, int(valid.sum()), int(invalid.sum()), correct


def msc_loss(maps, labels, ignore_label=IGNORE):
    """maps [(B, C, h_s, w_s) f32], labels (B, 1, H, W) f32 -> (losses (S + 1) float32: fused, map 0, ...; grads [(B, C, h_s, w_s)
    float32]; [valid, correct, invalid] of the fused head; [N_0, ..., N_{S-1}])"""
    maps = [np.asarray(m, dtype=np.float32) for m in maps]
    S, (B, C, h0, w0) = len(maps), maps[0].shape
    f32 = np.float32
    labs = [sample_labels(labels, *m.shape[-2:]) for m in maps]
    total = np.zeros(S + 1, dtype=np.float64)
    N = np.zeros(S, dtype=np.int64)
    n_correct = n_invalid = 0
    d = [np.zeros(m.shape, dtype=f32) for m in maps]
    G = [np.zeros(m.shape, dtype=np.float64) for m in maps]
    d0f = np.zeros(maps[0].shape, dtype=f32)                                      # [k == 0] * d_f
    for b in range(B):
        for s in range(S):
            t, d[s][b], nv, ni, _ = _head(maps[s][b], labs[s][b], C, ignore_label)
            total[1 + s] += t
            N[s] += nv
        u = np.stack([maps[0][b]] + [K.zoom(maps[s][b], h0, w0) for s in range(1, S)])
        k = np.argmax(u, axis=0)                                                  # the first maximum: the lowest s
        t, df, _, ni, nc = _head(u.max(axis=0), labs[0][b], C, ignore_label)
        total[0] += t
        n_invalid += ni
        n_correct += nc
        d0f[b] = np.where(k == 0, df, f32(0.0))
        for s in range(1, S):
            hs, ws = maps[s].shape[-2:]
            dfs = np.where(k == s, df, f32(0.0)).astype(f32)
            for iy, wy, my in SL._axis_weights(hs, h0):
                for ix, wx, mx in SL._axis_weights(ws, w0):
                    wgt = (wy[:, None] * wx[None, :]).astype(f32)                 # (wy * wx) in float32
                    con = (wgt[None] * dfs).astype(f32).astype(np.float64)        # ... * [k == s] d_f in float32
                    con[:, ~(my[:, None] & mx[None, :])] = 0.0
                    np.add.at(G[s][b], (slice(None), iy[:, None], ix[None, :]), con)
    den = [f32(max(int(n), 1)) for n in N]
    grads = [((d[0] + d0f).astype(f32) / den[0]).astype(f32)]
    for s in range(1, S):
        grads.append(((d[s] / den[s]).astype(f32) + (G[s].astype(f32) / den[0]).astype(f32)).astype(f32))
    losses = np.array([total[0] / max(int(N[0]), 1)] + [total[1 + s] / max(int(N[s]), 1) for s in range(S)]).astype(f32)
    return losses, grads, [int(N[0]), n_correct, n_invalid], [int(n) for n in N]


def torch_reference(maps, labels, dtype, ignore_label=IGNORE):
    """the torch composition on the CPU in `dtype` -> (losses (S + 1), [grad_s]) as float64 arrays"""
    import torch
    import torch.nn.functional as F
    C = maps[0].shape[1]
    h0, w0 = maps[0].shape[-2:]
    xs = [torch.from_numpy(np.array(m)).to(dtype).requires_grad_(True) for m in maps]
    fused = torch.stack([xs[0]] + [F.interpolate(x, size=(h0, w0), mode="bilinear", align_corners=True) for x in xs[1:]]).max(0).values
    losses = []
    for z in [fused] + xs:
        lab = sample_labels(labels, *z.shape[-2:])
        valid, _ = SL.classify(lab, C, ignore_label)
        target = torch.from_numpy(np.where(valid, lab, 255).astype(np.int64))
        losses.append(F.cross_entropy(z, target, reduction="sum", ignore_index=255) / max(int(valid.sum()), 1))
    torch.stack(losses).sum().backward()
    return np.array([float(l.detach().double()) for l in losses]), [x.grad.double().numpy() for x in xs]


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (l64 (S + 1), [g64_s], [e32_s]) of make_case(case): the float64 reference and, per map, the relative error
    max|g32 - g64| / max|g64| of the float32 torch composition on the same input (0 where the gradient is zero)"""
    import torch
    maps, labels, _ = make_case(case)
    l64, g64 = torch_reference(maps, labels, torch.float64)
    _, g32 = torch_reference(maps, labels, torch.float32)
    e32 = []
    for a, b in zip(g32, g64):
        top = float(np.abs(b).max())
        e32.append(float(np.abs(a - b).max()) / top if top > 0 else 0.0)
    return l64, g64, e32


def grad_bounds(case):
    """the issue's bound on max|grad_s - g64_s| per map: max(4 * e32_s, 16 * 2^-24) * max|g64_s| (seg_loss_cases.grad_bound's rule)"""
    _, g64, e32 = reference(case)
    return [max(4.0 * e, 16.0 * 2.0 ** -24) * float(np.abs(g).max()) for g, e in zip(g64, e32)]


def pyramid(images, sizes):
    """(B, 3, H, W) f32 -> [(B, 3, h, w) f32]: the zoom restatement of eval_confusion_cases per image"""
    images = np.asarray(images, dtype=np.float32)
    return [np.stack([K.zoom(im, h, w) for im in images]) for h, w in sizes]
