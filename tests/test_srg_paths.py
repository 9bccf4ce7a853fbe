"""Seeded region growing (csrc/srg.hip, ops.srg_grow) on every growth form of srg_grow_kernel: 64- and 128-bit row masks
with one and two rows per lane, and the per-pixel flood fill, reached by the map size and by the mask-fit limit (shapes and
the limit's formula: tests/srg_path_cases.py).  The patterns lie over the seams of the row-mask forms — columns 63|64 (the
two words of a 128-bit mask), rows 63|64 (the two rows of a lane), W = 64 / 128 (the carry leaves the word) — and use labels
beyond the sixteenth (a wave's second trip) and beyond the 64th.

Without a GPU: the oracle against a literal numpy / scipy restatement of generate_seed_step, bit for bit, and that no case
is vacuous — something grows, a restatement blind to a seam gives another answer wherever a case claims to cross it, and
the spiral needs as many propagation rounds as half its length.

On the GPU: ops.srg_grow equals the oracle bit for bit; a failure names case, pattern, class and the first pixel."""
import numpy as np
import pytest
import torch

import srg_path_cases as K

gpu = pytest.mark.gpu
IDS = ["%dx%dx%d" % s for s in K.SHAPES]


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


def _same(got, want, cases, what):
    """bit equality of two (B,C,H,W) seed blobs; the message names case, pattern, class and the first differing pixel"""
    if np.array_equal(got, want):
        return
    b, c, y, x = (int(v[0]) for v in np.nonzero(got != want))
    raise AssertionError("%s: case %d (%s), class %d, pixel (%d, %d): %r, expected %r; %d values differ in this case" %
                         (what, b, cases[b].pattern, c, y, x, got[b, c, y, x], want[b, c, y, x], int((got[b] != want[b]).sum())))


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_the_shapes_reach_every_form_with_a_seam_case():
    """by the restated launch formula (not a statement about a launch): the table holds all five forms, 44x50x96 and
    48x50x96 lie on either side of the mask-fit limit, and every form whose maps can hold a seam has a shape with a
    seam-crossing case on it (the 64-bit one-row form serves maps up to 64x64, which have no seam: there the cases are
    checked for growth and for the rounds the spiral needs)"""
    forms = {}
    for H, W, C in K.SHAPES:
        forms.setdefault(K.form_of(H, W, C), []).append((H, W, C))
    assert sorted(forms) == ["128-bit masks, 1 per lane", "128-bit masks, 2 per lane", "64-bit masks, 1 per lane",
                             "64-bit masks, 2 per lane", "flood fill"]
    assert K.form_of(44, 50, 96) == "64-bit masks, 1 per lane" and K.form_of(48, 50, 96) == "flood fill"
    assert 7024 + 136576 <= 150 * 1024 < 7632 + 148992
    for form, shapes in forms.items():
        if form == "64-bit masks, 1 per lane":
            continue
        seams = set()
        for s in shapes:
            for c in K.cases_of(*s)[0]:
                seams |= set(c.seams)
        want = {"64-bit masks, 2 per lane": {"r"}, "128-bit masks, 1 per lane": {"c"}}.get(form, {"c", "r"})
        assert seams >= want, (form, seams)


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_oracle_equals_the_literal_restatement(O, shape):
    cases, labels, cues, refined = K.cases_of(*shape)
    want = O.srg_grow_batch(labels, cues, refined)
    got = np.stack([K.restate(labels[b, 0, 0], cues[b], refined[b]) for b in range(len(cases))])
    _same(want, got, cases, "oracle against the restatement")
    # the oracle itself keeps the invariants the kernel is held to
    assert (want >= cues).all()
    absent = labels[:, 0, 0] != 1
    assert np.array_equal(want[absent], cues[absent])
    _same(O.srg_grow_batch(labels, want, refined), want, cases, "oracle applied twice")


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_no_case_is_vacuous(shape):
    H, W, C = shape
    cases, labels, cues, refined = K.cases_of(*shape)
    crossed = set()
    for b, case in enumerate(cases):
        args = labels[b, 0, 0], cues[b], refined[b]
        want = K.restate(*args)
        assert want.sum() > cues[b].sum(), "nothing grows in case %d (%s)" % (b, case.pattern)
        for s in case.seams:
            assert (H if s == "r" else W) > 64
            assert not np.array_equal(K.restate(*args, blind=s), want), \
                "case %d (%s) does not need the %s seam" % (b, case.pattern, {"r": "row", "c": "column"}[s])
            crossed.add(s)
        if hasattr(case, "spiral"):
            cls, length = case.spiral
            assert length > (H * W) // 2 - H - W
            assert K.jacobi_rounds(*args, cls) >= length // 2, case.pattern
    assert crossed == set(("c" if W > 64 else "") + ("r" if H > 64 else ""))


def test_patterns_do_what_their_names_say():
    """spot checks of the generated cases on one shape, so that a slip in a generator cannot turn a pattern into an easy one"""
    H, W, C = 128, 128, 21
    cases, labels, cues, refined = K.cases_of(H, W, C)
    by = dict((c.pattern, (b, c)) for b, c in enumerate(cases))
    out = lambda b: K.restate(labels[b, 0, 0], cues[b], refined[b])
    # a stopped run: grown up to the foreign pixel, not behind it
    b, c = by["rows seeded at 0, another label at 63"]
    g = out(b)[c.L[63, 0], 63]
    assert g[:63].all() and not g[63:].any()
    b, c = by["rows seeded at 127, another label at 64"]
    g = out(b)[c.L[64, 127], 64]
    assert g[65:].all() and not g[:65].any()
    # the unseeded comb stays empty, the corner piece joins, the piece behind the gap does not
    b, c = by["combs, a seeded"]
    g = out(b)
    assert g[C - 1].sum() == 0 and g[1][c.L == 1][:].sum() > 0
    Wc = (W - 4) // 4 * 4
    assert g[1, 1:H // 2, Wc].all() and not g[1, :, Wc + 2].any() and g[1, 0, :Wc].all()
    # excluded pixels: members that are not written, with growth behind them; the pixel with two foreign cues is written
    b, c = by["horizontal corridor through excluded pixels, the other class absent"]
    g = out(b)[1, 63]
    assert not g[62:65].any() and g[:62].all() and g[65:].all() and g[60] == 1 and cues[b][:, 63, 60].sum() == 2
    assert np.array_equal(out(b)[2], cues[b][2])
    # thresholds: foreground passes above 0.85 only, background above 0.99 only
    b, c = by["horizontal corridors with a threshold pixel"]
    g = out(b)
    rows = [r for r, _, _ in sorted(c.values)]
    passed = [bool(g[c.L[r, 0], r, W - 1]) for r in rows]
    assert passed == [False, True, True, True, False, False, False, True]
    # all classes: every plane grows
    b, c = by["all 21 classes at once"]
    assert ((out(b) - cues[b]).sum((1, 2)) == 2).all()


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_srg_grow_equals_the_oracle_on_every_pattern(ops, O, shape):
    cases, labels, cues, refined = K.cases_of(*shape)
    want = O.srg_grow_batch(labels, cues, refined)
    d_labels, d_refined = dev(labels), dev(refined, torch.float64)
    first = ops.srg_grow(d_labels, dev(cues), d_refined)
    got = first.cpu().numpy()
    _same(got, want, cases, "ops.srg_grow against the oracle")
    # invariants: monotone over the cues, absent classes untouched, idempotent
    assert (got >= cues).all()
    absent = labels[:, 0, 0] != 1
    assert np.array_equal(got[absent], cues[absent])
    _same(ops.srg_grow(d_labels, first, d_refined).cpu().numpy(), got, cases, "ops.srg_grow applied to its own output")
    assert torch.equal(ops.srg_grow(d_labels, dev(cues), d_refined), first), "two calls differ"
    # an image alone gives the bits it gives inside the batch: the spirals (the longest growth), the first and the last case
    alone = [b for b, c in enumerate(cases) if hasattr(c, "spiral")] + [0, len(cases) - 1]
    for b in alone:
        one = ops.srg_grow(dev(labels[b:b + 1]), dev(cues[b:b + 1]), dev(refined[b:b + 1], torch.float64)).cpu().numpy()
        _same(one, got[b:b + 1], cases[b:b + 1], "case %d alone against the same image in the batch" % b)
