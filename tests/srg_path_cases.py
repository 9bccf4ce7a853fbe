"""Generated cases for tests/test_srg_paths.py: seeded region growing on every growth form of srg_grow_kernel
(dsrg_amd/csrc/srg.hip), with components laid over the seams of the row-mask forms.

The form follows from the map shape and the label count alone (launch_srg):

    lds        = 2 * roundup16((H + 2) * (W + 2)) + roundup16(H * W) + 16
    mask_bytes = 2 * (C + 1) * H * 16
    row masks  iff W <= 128 and H <= 128 and lds + mask_bytes <= 150 * 1024, else the per-pixel flood fill in LDS
    row masks: 64-bit words iff W <= 64, one row per lane iff H <= 64

`form_of` restates that for the case table's own bookkeeping; the library offers no query for the form a launch took, so
nothing here or in the test asserts it.

A case is a label map L (H x W, -1 = no label, else 0..C-1), a seed mask, the set of present classes, explicit extra
cues and explicit marginals of single pixels.  refined[L[p], p] = 0.995 (above th1 = 0.99 for the background and above
th2 = 0.85 for a foreground class), the other labels share 0.005; pixels without a label carry 1 / C everywhere;
cues[L[p], p] = 1 on the seed mask."""
import functools

import numpy as np
from scipy import ndimage

TH1, TH2 = 0.99, 0.85

SHAPES = [(64, 64, 21), (65, 64, 21), (128, 33, 21), (64, 65, 21), (40, 128, 21), (128, 128, 21), (100, 97, 5),
          (129, 40, 21), (40, 129, 21), (129, 130, 3), (65, 65, 96),
          (44, 50, 96),       # lds 7 024 + masks 136 576 <= 153 600: row masks
          (48, 50, 96)]       # lds 7 632 + masks 148 992 >  153 600: flood fill, by the mask-fit branch alone


def _r16(n):
    return (n + 15) & ~15


def form_of(H, W, C):
    lds = 2 * _r16((H + 2) * (W + 2)) + _r16(H * W) + 16
    if W > 128 or H > 128 or lds + 2 * (C + 1) * H * 16 > 150 * 1024:
        return "flood fill"
    return "%d-bit masks, %d per lane" % (64 if W <= 64 else 128, 1 if H <= 64 else 2)


class Case(object):
    def __init__(self, pattern, L, seed, present, extra=(), values=(), seams=""):
        self.pattern = pattern
        self.L = L                      # (H, W) int, -1 or 0..C-1
        self.seed = seed                # (H, W) bool: cues[L[p], p] = 1
        self.present = sorted(present)
        self.extra = list(extra)        # (class, y, x): further cues
        self.values = list(values)      # (y, x, v): refined[L[y, x], y, x] = v, the others share 1 - v
        self.seams = seams              # which of the column ("c") and row ("r") seams 63|64 the growth has to cross


def materialise(case, C):
    """-> labels (C) f32, cues (C,H,W) f32, refined (C,H,W) f64"""
    L = case.L
    H, W = L.shape
    labels = np.zeros(C, np.float32)
    labels[case.present] = 1.0
    refined = np.full((C, H, W), 1.0 / C)
    cues = np.zeros((C, H, W), np.float32)
    ys, xs = np.nonzero(L >= 0)
    refined[:, ys, xs] = 0.005 / (C - 1)
    refined[L[ys, xs], ys, xs] = 0.995
    for y, x, v in case.values:
        refined[:, y, x] = (1.0 - v) / (C - 1)
        refined[L[y, x], y, x] = v
    ys, xs = np.nonzero(case.seed)
    assert (L[ys, xs] >= 0).all()
    cues[L[ys, xs], ys, xs] = 1.0
    for c, y, x in case.extra:
        cues[c, y, x] = 1.0
    return labels, cues, refined


# ---- the literal restatement of generate_seed_step (pylayers.py:237-275) ------------------------------------------------
def _label8(mat, blind):
    """scipy's 8-connected components of a boolean map; blind: label the parts left / right of columns 63|64 ("c") and
    above / below rows 63|64 ("r") separately, as a kernel that lost the link over that seam would"""
    H, W = mat.shape
    ycuts = [0, 64, H] if "r" in blind and H > 64 else [0, H]
    xcuts = [0, 64, W] if "c" in blind and W > 64 else [0, W]
    lab = np.zeros((H, W), np.int64)
    n = 0
    for y0, y1 in zip(ycuts[:-1], ycuts[1:]):
        for x0, x1 in zip(xcuts[:-1], xcuts[1:]):
            part, k = ndimage.label(mat[y0:y1, x0:x1], structure=np.ones((3, 3), int))
            lab[y0:y1, x0:x1] = np.where(part > 0, part + n, 0)
            n += k
    return lab


def label_map(labels, cues, refined, th1=TH1, th2=TH2):
    """class + 1 per pixel, 0 = none: the highest cued class, overridden by the thresholded arg-max over the present classes"""
    C, H, W = cues.shape
    lm = np.zeros((H, W), np.int64)
    for c in range(C):
        lm[cues[c] > 0] = c + 1
    pres = np.nonzero(labels == 1)[0]
    if pres.size:
        sub = refined[pres]
        k, v = sub.argmax(0), sub.max(0)                       # first maximum wins
        cls = pres[k]
        take = (v > th2) & ((cls != 0) | (v > th1))             # strict float64 compares
        lm[take] = cls[take] + 1
    return lm


def restate(labels, cues, refined, th1=TH1, th2=TH2, blind=""):
    out = cues.copy()
    lm = label_map(labels, cues, refined, th1, th2)
    cue_sum = cues.sum(0)
    for c in np.nonzero(labels == 1)[0]:
        mat = lm == c + 1
        lab = _label8(mat, blind)
        own = cues[c] == 1
        keep = np.unique(lab[mat & own])                        # components holding a pixel cued by their own class
        member = mat & np.isin(lab, keep)
        out[c][member & ~(~own & (cue_sum == 1))] = 1.0         # not where the own cue is 0 and the cue sum is 1
    return out


def jacobi_rounds(labels, cues, refined, cls):
    """neighbour-propagation rounds a plain Jacobi flood fill needs for class `cls`: every round a pixel of the class's
    mask joins when one of its 8 neighbours was a member after the round before"""
    mat = label_map(labels, cues, refined) == cls + 1
    g = mat & (cues[cls] == 1)
    rounds = 0
    while True:
        p = np.pad(g, 1)
        d = np.zeros_like(g)
        for dy in range(3):
            for dx in range(3):
                d |= p[dy:dy + g.shape[0], dx:dx + g.shape[1]]
        g1 = d & mat
        if np.array_equal(g1, g):
            return rounds
        g, rounds = g1, rounds + 1


# ---- patterns ----------------------------------------------------------------------------------------------------------
def _seam(n):
    """the last index before the seam of an axis of length n: 63 where the axis has the 63|64 seam, else its middle"""
    return 63 if n > 64 else n // 2 - 1


def _first(mask):
    ys, xs = np.nonzero(mask)
    m = np.zeros_like(mask)
    m[ys[0], xs[0]] = True
    return m


def _diagonals(H, W, C):
    """main diagonal (label a) through (cy, cx) -> (cy+1, cx+1), anti diagonal (label b) through (cy, cx+1) -> (cy+1, cx);
    one pixel wide, linked by corners only; the rest is background, grown from one cue"""
    a, b = C - 1, max(1, C - 5)
    cy, cx = _seam(H), _seam(W)
    L = np.zeros((H, W), np.int64)
    main, anti = [], []
    for t in range(-max(H, W), max(H, W)):
        if 0 <= cy + t < H and 0 <= cx + t < W:
            main.append((cy + t, cx + t))
        if 0 <= cy + t < H and 0 <= cx + 1 - t < W:
            anti.append((cy + t, cx + 1 - t))
    for y, x in main:
        L[y, x] = a
    for y, x in anti:
        L[y, x] = b
    seams = ("c" if W > 64 else "") + ("r" if H > 64 else "")
    cases = []
    for end in (0, -1):
        seed = _first(L == 0)
        seed[main[end]] = True
        seed[anti[end]] = True
        cases.append(Case("diagonals seeded at the %s end" % ("top" if end == 0 else "bottom"), L, seed, [0, a, b], seams=seams))
    return cases


def _runs(H, W, C, transpose):
    """full-width runs in rows 0, 63, 64 and the last (adjacent rows in different labels), seeded at one column only;
    then with one pixel of another label at the seam, where the growth has to stop.  transpose: the same for columns."""
    if transpose:
        H, W = W, H
    rows = sorted(set(r for r in (0, 63, 64, H - 1) if r < H))
    nfg = min(C - 1, 4)
    sx = _seam(W)
    out = []

    def build(seed_x, stop_x):
        L = np.full((H, W), -1, np.int64)
        seed = np.zeros((H, W), bool)
        for k, r in enumerate(rows):
            lab = 1 + k % nfg
            L[r] = lab
            if stop_x is not None:
                L[r, stop_x] = 0                            # background: present, never cued
            seed[r, seed_x] = True
        return L, seed

    seam = ("r" if transpose else "c") if W > 64 else ""
    for s in sorted(set((0, W - 1, sx, sx + 1))):
        L, seed = build(s, None)
        out.append(Case("%s seeded at %d" % ("columns" if transpose else "rows", s), L, seed, range(0, nfg + 1), seams=seam))
    for s, stop in ((0, sx), (W - 1, sx), (0, sx + 1), (W - 1, sx + 1)):
        if abs(s - stop) < 2:                               # W = 65: nothing lies between column 64 and the foreign pixel
            continue
        L, seed = build(s, stop)
        out.append(Case("%s seeded at %d, another label at %d" % ("columns" if transpose else "rows", s, stop), L, seed,
                        range(0, nfg + 1)))
    if transpose:
        for c in out:
            c.L, c.seed = np.ascontiguousarray(c.L.T), np.ascontiguousarray(c.seed.T)
    return out


def spiral_path(H, W):
    """a one-pixel-wide rectangular spiral from (0, 0) inwards, one pixel between its turns"""
    A = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    A[0, 0] = True
    path = [(0, 0)]
    turns = 0
    while turns < 2:
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < H and 0 <= nx < W and not A[ny, nx] and not (0 <= my < H and 0 <= mx < W and A[my, mx]):
            y, x = ny, nx
            A[y, x] = True
            path.append((y, x))
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return path


def _spirals(H, W, C):
    a = min(17, C - 1)
    path = spiral_path(H, W)
    L = np.zeros((H, W), np.int64)
    for y, x in path:
        L[y, x] = a
    seams = ("c" if W > 64 else "") + ("r" if H > 64 else "")
    cases = []
    for end, name in ((0, "outer end"), (-1, "centre")):
        seed = np.zeros((H, W), bool)
        seed[path[end]] = True
        if end == 0:
            seed |= _first(L == 0)                          # the background between the turns is a spiral too
        c = Case("spiral seeded at the " + name, L, seed, [0, a], seams=seams)
        c.spiral = (a, len(path))
        cases.append(c)
    return cases


def _combs(H, W, C):
    """comb a: spine in row 0, teeth down at columns 0, 4, ...; comb b: spine in the last row, teeth up at columns 2, 6, ...;
    a further piece of label a that touches a's spine by a corner only (joins) and one behind a one-pixel gap (does not)"""
    a, b = 1, C - 1
    Wc = (W - 4) // 4 * 4
    L = np.zeros((H, W), np.int64)
    L[:, Wc:] = -1
    L[0, :Wc] = a
    L[H - 1, :Wc] = b
    for x in range(0, Wc, 4):
        L[0:H - 2, x] = a
    for x in range(2, Wc, 4):
        L[2:H, x] = b
    L[1:H // 2, Wc] = a                                       # (1, Wc) meets (0, Wc - 1) by the corner
    L[:, Wc + 2] = a                                          # column Wc + 1 stays empty
    s_a = np.zeros((H, W), bool)
    s_a[H - 3, 0] = True                                      # the tip of a's first tooth
    s_b = np.zeros((H, W), bool)
    s_b[2, 2] = True                                          # the tip of b's first tooth
    col = "c" if Wc > 65 else ""                              # the spines reach over columns 63|64
    return [Case("combs, a seeded", L, s_a, [0, a, b], seams=col + ("r" if H - 3 >= 64 else "")),     # a's teeth end in row H - 3
            Case("combs, b and the background seeded", L, s_b | _first(L == 0), [0, a, b], seams=col + ("r" if H > 64 else ""))]


def _excluded(H, W, C):
    """a corridor of label a whose pixels about the seam carry exactly one cue of another class x: members (the growth
    passes) that are not written; one pixel carries two foreign cues and is written.  x present, then absent."""
    a, x_cls, y_cls = 1, 2, 0
    cases = []
    for transpose in (False, True):
        h, w = (W, H) if transpose else (H, W)
        r, sx = _seam(h), _seam(w)
        L = np.full((h, w), -1, np.int64)
        L[r] = a
        seed = np.zeros((h, w), bool)
        seed[r, 0] = True
        extra = [(x_cls, r, x) for x in range(sx - 1, min(sx + 2, w - 1))] + [(x_cls, r, sx - 3), (y_cls, r, sx - 3)]
        if transpose:
            L, seed = np.ascontiguousarray(L.T), np.ascontiguousarray(seed.T)
            extra = [(c, x, y) for c, y, x in extra]
        seam = ("r" if transpose else "c") if w > 64 else ""
        for present in ([0, a, x_cls], [a]):
            cases.append(Case("%s corridor through excluded pixels, the other class %s" %
                              ("vertical" if transpose else "horizontal", "present" if len(present) > 1 else "absent"),
                              L, seed, present, extra=extra, seams=seam))
    return cases


def _all_classes(H, W, C):
    """every class present and growing: one three-pixel diagonal per class, seeded at its top, the classes spread over a
    grid of 4 x 4 cells that starts at (2, 2), so that a cell lies over 62..64"""
    ny, nx = (H - 2) // 4, (W - 2) // 4
    assert ny * nx >= C
    L = np.full((H, W), -1, np.int64)
    seed = np.zeros((H, W), bool)
    for c in range(C):
        cell = c * (ny * nx) // C
        y0, x0 = 2 + 4 * (cell // nx), 2 + 4 * (cell % nx)
        for t in range(3):
            L[y0 + t, x0 + t] = c
        seed[y0, x0] = True
    return [Case("all %d classes at once" % C, L, seed, range(C))]


def _thresholds(H, W, C):
    """eight corridors over the seam, seeded at their start, whose pixel behind the seam has v exactly at or one ulp above
    a threshold: foreground passes above 0.85 only, background above 0.99 only (strict compares)"""
    a = C - 1
    vs = [0.85, np.nextafter(0.85, 1.0), 0.99, np.nextafter(0.99, 1.0)]
    cases = []
    for transpose in (False, True):
        h, w = (W, H) if transpose else (H, W)
        sx = _seam(w)
        L = np.full((h, w), -1, np.int64)
        seed = np.zeros((h, w), bool)
        values = []
        for k in range(8):
            r = 1 + 2 * k + (h - 17) // 2
            L[r] = a if k < 4 else 0
            seed[r, 0] = True
            values.append((r, sx + 1, vs[k % 4]))
        if transpose:
            L, seed = np.ascontiguousarray(L.T), np.ascontiguousarray(seed.T)
            values = [(x, y, v) for y, x, v in values]
        seam = ("r" if transpose else "c") if w > 64 else ""
        cases.append(Case("%s corridors with a threshold pixel" % ("vertical" if transpose else "horizontal"), L, seed, [0, a],
                          values=values, seams=seam))
    return cases


@functools.lru_cache(maxsize=2)
def cases_of(H, W, C):
    """-> (cases, labels (B,1,1,C), cues (B,C,H,W), refined (B,C,H,W) f64): every pattern of a shape as one batch"""
    cases = (_diagonals(H, W, C) + _runs(H, W, C, False) + _runs(H, W, C, True) + _spirals(H, W, C) + _combs(H, W, C) +
             _excluded(H, W, C) + _all_classes(H, W, C) + _thresholds(H, W, C))
    parts = [materialise(c, C) for c in cases]
    labels = np.stack([p[0] for p in parts]).reshape(len(cases), 1, 1, C)
    cues = np.stack([p[1] for p in parts])
    refined = np.stack([p[2] for p in parts])
    for a in (labels, cues, refined):
        a.setflags(write=False)
    return cases, labels, cues, refined
