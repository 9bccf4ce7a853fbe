"""The six staging functions of dsrg_amd/input.py — layout_train_s / pack_train_s, layout_train_s_cuemap / pack_train_s_cuemap,
layout_train_f / pack_train_f — held to what they gave while each pair was a loop of its own: tests/golden/train_input_staging.json,
recorded by tools/record_train_input_golden.py at commit 4da5128.  Per case the byte count and every field of the descriptor are
compared, and the sha256 of a staging buffer of nbytes + 16 bytes prefilled with 0xA5 and then packed, so a byte written into an
alignment gap or past the end shows.  Then what the six refuse.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from dsrg_amd import input as I

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_input_staging.json")
with open(GOLDEN) as _f:
    RECORD = json.load(_f)


def _contents(case):
    """`contents` of tools/record_train_input_golden.py: the pieces of a case from np.random.default_rng(seed), per image the
    image and then its further pieces"""
    rng = np.random.default_rng(case["seed"])
    pieces = ([], [], []) if case["kind"] == "s" else ([], [])
    for b, (H, W) in enumerate(case["shapes"]):
        pieces[0].append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        if case["kind"] == "s":
            pieces[1].append(rng.integers(0, 41, (3, case["ncues"][b])).astype(np.int32))
            pieces[2].append(rng.integers(0, 21, (case["nlabels"][b],)).astype(np.int32))
        elif case["kind"] == "c":
            pieces[1].append(rng.integers(0, 256, tuple(case["map_size"])).astype(np.uint8))
        else:
            pieces[1].append(rng.integers(0, 256, (H, W)).astype(np.uint8))
    return pieces


def _layout(case):
    shapes = [tuple(s) for s in case["shapes"]]
    if case["kind"] == "s":
        return I.layout_train_s(shapes, case["ncues"], case["nlabels"], case["mirror"]), I.pack_train_s
    if case["kind"] == "c":
        return I.layout_train_s_cuemap(shapes, tuple(case["map_size"]), case["mirror"]), I.pack_train_s_cuemap
    scaled = None if case["scaled"] is None else [tuple(s) for s in case["scaled"]]
    return I.layout_train_f(shapes, case["top"], case["left"], case["mirror"], scaled), I.pack_train_f


def test_the_record_holds_the_cases_the_recorder_states():
    assert RECORD["prefill"] == 0xA5 and RECORD["tail"] == 16
    kinds = [c["kind"] for c in RECORD["cases"].values()]
    assert len(kinds) == 10 and {k: kinds.count(k) for k in "scf"} == dict(s=3, c=3, f=4)
    assert sorted(len(c["shapes"]) for c in RECORD["cases"].values()) == [1, 1, 1, 3, 3, 3, 3, 32, 32, 32]
    assert any(c["kind"] == "f" and c["scaled"] for c in RECORD["cases"].values())


@pytest.mark.parametrize("name", sorted(RECORD["cases"]))
def test_layout_and_packed_bytes_are_the_recorded_ones(name):
    case = RECORD["cases"][name]
    (nbytes, desc), pack = _layout(case)
    assert nbytes == case["nbytes"] and nbytes % 16 == 0
    assert sorted(desc) == sorted(case["desc"])
    for key, want in case["desc"].items():                              # field for field: the same ints, and ints they are
        assert desc[key] == want, key
        assert all(type(v) is int for v in (desc[key] if isinstance(desc[key], list) else [desc[key]])), key
    buf = np.full(nbytes + RECORD["tail"], RECORD["prefill"], np.uint8)
    pack(buf, desc, *_contents(case))
    assert hashlib.sha256(buf.tobytes()).hexdigest() == case["sha256"]
    assert (buf[nbytes:] == RECORD["prefill"]).all()


# ---- what the six refuse: ValueError, every time ------------------------------------------------------------------------------------
LAYOUTS = {
    "s": lambda shapes, mirror="zeros": I.layout_train_s(shapes, [1] * len(shapes), [2] * len(shapes),
                                                         [0] * len(shapes) if mirror == "zeros" else mirror),
    "c": lambda shapes, mirror="zeros": I.layout_train_s_cuemap(shapes, (4, 6), [0] * len(shapes) if mirror == "zeros" else mirror),
    "f": lambda shapes, mirror="zeros": I.layout_train_f(shapes, [0] * len(shapes), [1] * len(shapes),
                                                         [0] * len(shapes) if mirror == "zeros" else mirror),
}


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_layouts_refuse_bad_batches(kind):
    layout = LAYOUTS[kind]
    layout([(2, 2)] * 32)
    for shapes in ([], [(2, 2)] * 33, [(4, 5), (0, 3)], [(4, 5), (3, 0)], [(-1, 5)]):
        with pytest.raises(ValueError):
            layout(shapes)
    for mirror in ([0], [0, 1, 0]):                                     # one flag per image
        with pytest.raises(ValueError):
            layout([(4, 5), (5, 4)], mirror)
    assert layout([(4, 5), (5, 4)], [0, 7])[1]["mirror"] == [0, 1]


def test_stage_2_layout_refuses_negative_offsets_and_bad_rescaled_sizes():
    shapes = [(4, 5), (5, 4)]
    I.layout_train_f(shapes, [0, 3], [2, 0], [0, 1], [(1, 1), (9, 2)])
    for top, left in (([0, -1], [0, 0]), ([0, 0], [-1, 0])):
        with pytest.raises(ValueError):
            I.layout_train_f(shapes, top, left, [0, 0])
    for scaled in ([(4, 5)], [(4, 5), (0, 4)], [(4, 5), (5, -4)]):
        with pytest.raises(ValueError):
            I.layout_train_f(shapes, [0, 0], [0, 0], [0, 0], scaled)
    for top, left in (([0], [0, 0]), ([0, 0], [0, 0, 0])):             # one offset per image
        with pytest.raises(ValueError):
            I.layout_train_f(shapes, top, left, [0, 0])


def test_stage_1_layouts_refuse_their_own_bad_arguments():
    shapes = [(4, 5), (5, 4)]
    for ncues, nlabels in (([1], [2, 2]), ([1, 1], [2, 2, 2]), ([1, -1], [2, 2]), ([1, 1], [-2, 2])):
        with pytest.raises(ValueError):
            I.layout_train_s(shapes, ncues, nlabels)
    for map_size in ((0, 6), (4, 0), (-4, 6)):
        with pytest.raises(ValueError):
            I.layout_train_s_cuemap(shapes, map_size)


def _case_of(kind):
    case = RECORD["cases"]["%s/odd_sizes" % kind]
    (nbytes, desc), pack = _layout(case)
    return np.zeros(nbytes, np.uint8), desc, pack, [list(p) for p in _contents(case)]


@pytest.mark.parametrize("kind", ["s", "c", "f"])
def test_packs_refuse_a_piece_of_the_wrong_dtype_or_shape(kind):
    """every piece in turn: another shape, another dtype (the int32 pieces of stage 1 are converted, as they always were: for them
    another number of values), a piece too few; the images also exchanged among themselves"""
    buf, desc, pack, pieces = _case_of(kind)
    pack(buf, desc, *pieces)

    def refused(p, b, bad):
        changed = [list(q) for q in pieces]
        changed[p][b] = bad
        with pytest.raises(ValueError):
            pack(buf, desc, *changed)

    for p in range(len(pieces)):
        for b in (0, 1, 2):
            a = pieces[p][b]
            refused(p, b, np.zeros((a.size + 1,), a.dtype))
            if a.dtype == np.uint8:
                refused(p, b, a.reshape(a.shape + (1,)))                # one axis more, as many values
                refused(p, b, a.astype(np.int32))
                refused(p, b, a.astype(np.float32))
                refused(p, b, a[:-1])
                refused(p, b, a.T)                                      # (4, 5, 3) -> (3, 5, 4); (4, 6) -> (6, 4); (1, 7) -> (7, 1)
        with pytest.raises(ValueError):
            pack(buf, desc, *[q[:2] if k == p else q for k, q in enumerate(pieces)])
    with pytest.raises(ValueError):
        pack(buf, desc, [pieces[0][1], pieces[0][0], pieces[0][2]], *pieces[1:])
    if kind == "s":                                                     # what numpy converts to int32 with the right count passes
        before = buf.copy()
        pack(buf, desc, pieces[0], [c.astype(np.int64).reshape(-1) for c in pieces[1]], [l.tolist() for l in pieces[2]])
        assert np.array_equal(buf, before)
