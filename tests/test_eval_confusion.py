"""dsrg_eval_confusion_batch (dsrg_amd/csrc/eval.hip) / ops.eval_confusion_batch: a batch of score maps and label maps -> confusion
counters in one launch, and the host code around it (validate.reduce_counts, validate.ValInput's planning, the --val-* options of
`python -m dsrg_amd.train`).

CPU: the NumPy restatement of the contract (tests/eval_confusion_cases.py) on hand-made cases; the entry point's argument checks,
which return before any device call; reduce_counts over a 2-rank gloo group; which images a rank plans, in which order; the
command's arguments.
GPU: the kernel against the restatement and against the composition of the existing ops it replaces (ops.multiscale_unary's
argmax per image -> uint8 -> ops.confusion_matrix), both keep rules, Gaussian scores and integer scores with duplicated planes
(exact ties at and between source pixels); accumulation, counters above 2^32, a batch prefix, repeated calls.
Every comparison is an equality of integers."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_confusion_cases as K

_FAKE = 256                                                           # a "device pointer" that is never dereferenced

# (B, C, h, w, Hz, Wz): the exact x8 geometry; a non-multiple one; one label; a one-pixel source; the label limit; four images of
# 4225 pixels (neither it nor 33*49 nor 19*10 is a multiple of a workgroup's run of 256 pixels, and 4225 takes several: workgroups
# whose lanes lie in two images); 32 images
SHAPES = [(3, 21, 5, 7, 33, 49), (2, 21, 4, 3, 19, 10), (1, 1, 2, 2, 5, 5), (2, 2, 1, 1, 7, 3), (1, 96, 3, 3, 17, 17),
          (4, 21, 9, 9, 65, 65), (32, 3, 2, 2, 9, 9)]


# ---- CPU: the restatement on hand-made cases ----------------------------------------------------------------------------------------
def test_restatement_constant_map_predicts_label_zero():
    s = np.full((5, 3, 4), 1.25, dtype=np.float32)
    assert np.array_equal(K.zoom(s, 11, 9), np.full((5, 11, 9), 1.25, dtype=np.float32))
    assert not K.predict(s, 11, 9).any()
    lab = np.full((1, 1, 11, 9), 3.0, dtype=np.float32)
    h = K.counters(s[None], lab, 5)
    assert h[3 * 5 + 0] == 99 and h.sum() == 99


def test_restatement_2x2_to_3x3_by_hand():
    # scale = 1/2 on both axes: output 1 lies halfway between the two sources
    s = np.array([[[0, 2], [4, 6]], [[3, 3], [3, 3]]], dtype=np.float32)
    z = K.zoom(s, 3, 3)
    assert np.array_equal(z[0], np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]], dtype=np.float32))
    assert np.array_equal(z[1], np.full((3, 3), 3, dtype=np.float32))
    # label 1 wins below 3, label 0 above, and the tie at the centre goes to the first maximum
    assert np.array_equal(K.predict(s, 3, 3), np.array([[1, 1, 1], [1, 0, 0], [0, 0, 0]]))
    lab = np.array([[0, 1, 255], [1, 1, 0], [2, 0.5, -1]], dtype=np.float32)[None, None]
    h = K.counters(s[None], lab, 2)                                   # rule `add`: all but the 255 kept
    assert h.tolist() == [1, 1, 1, 2, 3]                              # (0,0) (0,1) (1,0) (1,1) and 2, 0.5, -1 in the overflow
    h = K.counters(s[None], lab, 2, rule_lt=True)                     # rule `generateM`: 255 and 2 dropped; 0.5 and -1 kept
    assert h.tolist() == [1, 1, 1, 2, 2]


def test_restatement_one_row_or_one_column():
    s = np.array([[[1, 5], [9, 0]], [[2, 4], [0, 9]]], dtype=np.float32)
    assert K.axis_taps(2, 1)[0].tolist() == [0] and K.axis_taps(2, 1)[3].tolist() == [0.0]
    assert np.array_equal(K.zoom(s, 1, 1)[:, 0, 0], s[:, 0, 0])                      # both scales 0: the top left source pixel
    assert K.predict(s, 1, 1).tolist() == [[1]]
    assert np.array_equal(K.zoom(s, 1, 3), np.array([[[1, 3, 5]], [[2, 3, 4]]], dtype=np.float32))      # row 0 only
    assert K.predict(s, 1, 3).tolist() == [[1, 0, 0]]
    assert np.array_equal(K.zoom(s, 3, 1), np.array([[[1], [5], [9]], [[2], [1], [0]]], dtype=np.float32))   # column 0 only
    assert K.predict(s, 3, 1).tolist() == [[1], [0], [0]]
    assert K.axis_taps(1, 4)[1].tolist() == [0, 0, 0, 0]                              # a one-sample axis has no second tap


# ---- CPU: argument checks -----------------------------------------------------------------------------------------------------------
def test_eval_confusion_batch_checks_arguments_before_any_device_call():
    from dsrg_amd import _lib
    L = _lib.lib()

    def call(B=3, C=21, scores=_FAKE, h=5, w=7, labels=_FAKE, Hz=33, Wz=49, hist=_FAKE, rule_lt=0):
        return L.dsrg_eval_confusion_batch(B, C, scores, h, w, labels, Hz, Wz, 255.0, rule_lt, hist, None)

    E, U = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    for name in ("scores", "labels", "hist"):
        assert call(**{name: None}) == E and b"NULL" in L.dsrg_last_error(), name
    assert call(B=0) == E and b"images" in L.dsrg_last_error()
    assert call(B=33) == E and b"32" in L.dsrg_last_error()
    assert call(B=-1) == E
    assert call(C=0) == E and b"labels" in L.dsrg_last_error()
    assert call(C=97) == U and b"96" in L.dsrg_last_error()
    for name in ("h", "w", "Hz", "Wz"):
        assert call(**{name: 0}) == E and call(**{name: -3}) == E, name
    assert call(B=32, C=64, h=1024, w=1024) == E and b"2^31" in L.dsrg_last_error()                 # B*C*h*w = 2^31
    assert call(B=32, C=96, h=837, w=836) == E and b"2^31" in L.dsrg_last_error()
    assert call(B=32, C=96, h=(1 << 31) - 1, w=(1 << 31) - 1) == E                                   # (no wrap-around in the check)
    assert call(B=32, Hz=8192, Wz=8192) == E and b"2^31" in L.dsrg_last_error()                      # B*Hz*Wz = 2^31
    assert call(B=1, Hz=(1 << 31) - 1, Wz=(1 << 31) - 1) == E
    if not torch.cuda.is_available():                                                                # everything in order: only the device is missing
        assert call() == _lib.ERR_HIP and L.dsrg_last_error()
        assert call(B=32, C=96, rule_lt=1) == _lib.ERR_HIP
        assert call(B=32, C=64, h=1024, w=1023) == _lib.ERR_HIP                                      # (just below 2^31)


def test_op_checks_its_tensors_before_the_library_is_called():
    from dsrg_amd import ops
    s, lab = torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 9, 9)
    with pytest.raises(ValueError, match="CUDA"):
        ops.eval_confusion_batch(s, lab, 3)


def test_confusion_matrix_add_counts():
    from dsrg_amd.inference import ConfusionMatrix
    cm = ConfusionMatrix(2)
    cm.add_counts(np.array([5, 1, 2, 7, 0], dtype=np.int64))
    cm.add_counts(torch.tensor([1, 0, 0, 1, 0], dtype=torch.int64))
    assert cm.M.tolist() == [[6.0, 1.0], [2.0, 8.0]]
    with pytest.raises(ValueError, match="outside"):
        cm.add_counts(np.array([1, 0, 0, 1, 3], dtype=np.int64))
    with pytest.raises(ValueError, match="counters"):
        cm.add_counts(np.zeros(4, dtype=np.int64))
    assert cm.M.tolist() == [[6.0, 1.0], [2.0, 8.0]]


# ---- CPU: reduce_counts over gloo ---------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_counts(rank):
    return torch.arange(10, dtype=torch.int64) * (rank + 1) + (rank << 33)                            # (above 2^32: no 32-bit path)


def _reduce_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dsrg_amd.validate import reduce_counts
    mine = _rank_counts(rank)
    got = reduce_counts(mine)
    assert torch.equal(mine, _rank_counts(rank))                                                      # the argument is left as it was
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), got.numpy())
    dist.destroy_process_group()


def test_reduce_counts_two_rank_gloo_equals_the_sum(tmp_path):
    from dsrg_amd.validate import reduce_counts
    mp.spawn(_reduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    want = (_rank_counts(0) + _rank_counts(1)).numpy()
    for rank in (0, 1):
        got = np.load(str(tmp_path / ("rank%d.npy" % rank)))
        assert got.dtype == np.int64 and np.array_equal(got, want), rank
    alone = _rank_counts(1)
    assert reduce_counts(alone) is alone                                                               # no group: the tensor itself


# ---- CPU: which images a rank plans -------------------------------------------------------------------------------------------------
def _plan_all(loader):
    plans = []
    while True:
        plan = loader.plan_batch()
        if not plan:
            assert loader.plan_batch() == []                                                           # the end stays the end
            return plans
        plans.append(plan)


def test_val_input_plans_every_image_once(tmp_path):
    from dsrg_amd.validate import ValInput
    rng = np.random.default_rng(41)
    lst, root, _ = K.write_val_files(tmp_path, rng, ((6, 9), (12, 5), (7, 7), (12, 12), (3, 4)))
    listed = [(root + "/val_im%d.png" % k, root + "/val_lab%d.png" % k) for k in range(5)]
    one = _plan_all(ValInput(lst, root, crop=12, batch_size=2))
    assert [len(p) for p in one] == [2, 2, 1]
    assert [(it["image"], it["label"]) for p in one for it in p] == listed
    per_rank = []
    for rank in (0, 1):
        plans = _plan_all(ValInput(lst, root, crop=12, batch_size=2, rank=rank, world_size=2))
        per_rank.append([(it["image"], it["label"]) for p in plans for it in p])
        assert all(len(p) <= 2 for p in plans)
    assert per_rank[0] == listed[0::2] and per_rank[1] == listed[1::2]                                 # in list order within a rank
    assert sorted(per_rank[0] + per_rank[1]) == sorted(listed)                                         # jointly the list, each image once
    for world in (3, 5, 7):                                                                            # (a rank past a short list's end has nothing)
        got = [it["label"] for r in range(world) for p in _plan_all(ValInput(lst, root, crop=12, batch_size=4, rank=r, world_size=world))
               for it in p]
        assert sorted(got) == sorted(l for _, l in listed), world
    with pytest.raises(ValueError):
        ValInput(lst, root, crop=12, batch_size=2, rank=2, world_size=2)


def test_val_input_refuses_an_image_larger_than_the_crop(tmp_path):
    from dsrg_amd.validate import ValInput
    rng = np.random.default_rng(42)
    lst, root, _ = K.write_val_files(tmp_path, rng, ((6, 9), (12, 5), (7, 13), (12, 12)))
    loader = ValInput(lst, root, crop=12, batch_size=2)
    assert len(loader.plan_batch()) == 2
    with pytest.raises(ValueError, match="val_lab2.png"):
        loader.plan_batch()
    with pytest.raises(ValueError, match="val_lab0.png"):
        ValInput(lst, root, crop=8, batch_size=2).plan_batch()                                         # (6 x 9: too wide)


# ---- CPU: the command's arguments ---------------------------------------------------------------------------------------------------
def test_train_command_validation_arguments(capsys):
    from dsrg_amd.train import parse_args, val_batch
    base = ["--stage", "f", "--list", "l.txt", "--root", "r/"]
    a = parse_args(base)
    assert a.val_list is None and a.val_every is None and a.val_result is None
    for extra in (["--val-root", "x/"], ["--val-every", "5"], ["--val-crop", "65"], ["--val-batch", "2"], ["--val-result", "f.txt"]):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert "--val-list" in capsys.readouterr().err
    a = parse_args(base + ["--val-list", "v.txt"])
    assert (a.val_list, a.val_root, a.val_every, a.val_crop, a.val_batch, a.val_result) == ("v.txt", "r/", 10000, 513, None, None)
    assert val_batch(a, 1) == 10 and val_batch(a, 2) == 5                                              # the per-rank batch
    a = parse_args(base + ["--val-list", "v.txt", "--snapshot-every", "500", "--batch", "8"])
    assert a.val_every == 500 and val_batch(a, 4) == 2                                                 # whenever a snapshot is written
    a = parse_args(["--stage", "s", "--list", "l.txt", "--root", "r/", "--cues", "c.pickle", "--val-list", "v.txt", "--val-root", "g/",
                    "--val-every", "7", "--val-crop", "65", "--val-batch", "3", "--val-result", "res.txt"])
    assert (a.val_root, a.val_every, a.val_crop, a.val_batch, a.val_result) == ("g/", 7, 65, 3, "res.txt") and val_batch(a, 2) == 3
    assert a.val_every != a.snapshot_every == 8000
    for bad in (["--val-every", "0"], ["--val-crop", "0"], ["--val-batch", "0"], ["--val-batch", "33"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--val-list", "v.txt"] + bad)


def test_validate_command_arguments():
    from dsrg_amd.validate import parse_args
    a = parse_args(["--model", "m", "--list", "l", "--root", "r", "--save_path", "s"])
    assert (a.backbone, a.num_classes, a.crop, a.batch, a.fp32) == ("vgg16", 21, 513, 10, False)
    a = parse_args(["--model", "m", "--list", "l", "--root", "r", "--save_path", "s", "--backbone", "resnet101", "--class", "81", "--crop", "65",
                    "--batch", "2", "--fp32"])
    assert (a.backbone, a.num_classes, a.crop, a.batch, a.fp32) == ("resnet101", 81, 65, 2, True)
    with pytest.raises(SystemExit):
        parse_args(["--model", "m", "--list", "l", "--root", "r"])


# ---- GPU: the kernel ----------------------------------------------------------------------------------------------------------------
def _case(shape, ties):
    B, C, h, w, Hz, Wz = shape
    rng = np.random.default_rng(1000 + sum(shape) + int(ties))
    return K.make_scores(rng, B, C, h, w, ties), K.make_labels(rng, B, C, Hz, Wz)


def _composition(scores, labels, C, rule_lt):
    """what the kernel replaces: per image ops.multiscale_unary's argmax -> uint8 -> ops.confusion_matrix (integral labels in 0..255)"""
    from dsrg_amd import ops
    hist = torch.zeros(C * C + 1, dtype=torch.int64, device=scores.device)
    Hz, Wz = labels.shape[2:]
    for b in range(labels.shape[0]):
        amax = ops.multiscale_unary([scores[b:b + 1]], Hz, Wz, want="argmax")
        assert int(amax.min()) >= 0 and int(amax.max()) < C
        ops.confusion_matrix(labels[b, 0].to(torch.uint8).reshape(-1), amax.to(torch.uint8).reshape(-1), C, rule_lt=rule_lt, hist=hist)
    return hist


@pytest.mark.gpu
@pytest.mark.parametrize("ties", (False, True), ids=("gaussian", "ties"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_kernel_equals_restatement_and_composition(shape, ties):
    from dsrg_amd import ops
    B, C, h, w, Hz, Wz = shape
    scores, labels = _case(shape, ties)
    if ties and C > 1:                                                 # the case does hold ties between different labels
        z = K.zoom(scores[0], Hz, Wz)
        assert (np.sort(z, axis=0)[-1] == np.sort(z, axis=0)[-2]).any()
    ds, dl = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    for rule_lt in (False, True):
        got = ops.eval_confusion_batch(ds, dl, C, rule_lt=rule_lt)
        assert got.dtype == torch.int64 and got.shape == (C * C + 1,)
        want = K.counters(scores, labels, C, rule_lt=rule_lt)
        assert np.array_equal(got.cpu().numpy(), want), rule_lt
        assert torch.equal(got, _composition(ds, dl, C, rule_lt)), rule_lt
        # what the case is meant to exercise is there: kept pixels, and an overflow under `add` alone
        assert want[:-1].sum() > 0
        assert want[-1] == (0 if rule_lt else np.count_nonzero((labels != 255) & (labels >= C)))


@pytest.mark.gpu
def test_kernel_with_more_pixels_than_one_pass_of_the_grid():
    """the grid is capped (1024 workgroups of 256 lanes): 2 x 513 x 513 pixels make every workgroup take two or three runs, the last
    pass is a partial one, and the runs of one workgroup lie in different images"""
    from dsrg_amd import ops
    shape = (2, 3, 4, 5, 513, 513)
    B, C, h, w, Hz, Wz = shape
    assert B * Hz * Wz > 2 * 1024 * 256 and (B * Hz * Wz) % (1024 * 256)
    rng = np.random.default_rng(77)
    scores = K.make_scores(rng, B, C, h, w, False)
    labels = rng.integers(0, C, (B, 1, Hz, Wz)).astype(np.float32)
    labels[0, 0, 300:, :] = 255.0                                      # whole passes of dropped pixels between kept ones
    labels[1, 0, :, 400:] = 255.0
    labels[1, 0, 512, :7] = [float(C), 0.5, -1.0, 200.0, 0.0, 1.0, 2.0]
    ds, dl = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    for rule_lt in (False, True):
        want = K.counters(scores, labels, C, rule_lt=rule_lt)
        assert np.array_equal(ops.eval_confusion_batch(ds, dl, C, rule_lt=rule_lt).cpu().numpy(), want), rule_lt
        assert want[-1] == (2 if rule_lt else 4)


@pytest.mark.gpu
def test_kernel_other_ignore_label_and_labels_that_are_no_class_id():
    from dsrg_amd import ops
    B, C, h, w, Hz, Wz = 2, 5, 3, 4, 21, 13
    rng = np.random.default_rng(7)
    scores = K.make_scores(rng, B, C, h, w, False)
    labels = rng.integers(0, C, (B, 1, Hz, Wz)).astype(np.float32)
    labels[0, 0, 2:9, 1:6] = 7.0                                       # the ignore label of this call
    labels[1, 0, 0, :] = [-1.0, 0.5, 3.999, 4.0, 5.0, 255.0, -0.0, 1e9, -1e9, 2.0, 1.5, 7.0, 4.25]
    ds, dl = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    for rule_lt in (False, True):
        got = ops.eval_confusion_batch(ds, dl, C, ignore_label=7, rule_lt=rule_lt).cpu().numpy()
        assert np.array_equal(got, K.counters(scores, labels, C, ignore_label=7.0, rule_lt=rule_lt)), rule_lt
    # rule `add` drops the 7s alone: -1, 0.5, 3.999, 5, 255, 1e9, -1e9, 1.5, 4.25 overflow; rule `generateM` keeps what is < 5
    assert ops.eval_confusion_batch(ds, dl, C, ignore_label=7)[-1].item() == 9
    assert ops.eval_confusion_batch(ds, dl, C, ignore_label=7, rule_lt=True)[-1].item() == 6


@pytest.mark.gpu
def test_kernel_accumulates_keeps_large_counters_scores_a_prefix_and_repeats():
    from dsrg_amd import ops
    shape = (3, 21, 5, 7, 33, 49)
    C = shape[1]
    (s1, l1), (s2, l2) = _case(shape, False), _case(shape, True)
    d = lambda a: torch.from_numpy(a).cuda()                            # noqa: E731
    h1, h2 = ops.eval_confusion_batch(d(s1), d(l1), C), ops.eval_confusion_batch(d(s2), d(l2), C)
    both = ops.eval_confusion_batch(d(s1), d(l1), C)
    assert ops.eval_confusion_batch(d(s2), d(l2), C, hist=both) is both
    assert torch.equal(both, h1 + h2)
    big = (torch.arange(C * C + 1, dtype=torch.int64, device="cuda") + 1) * ((1 << 32) + 12345)
    got = ops.eval_confusion_batch(d(s1), d(l1), C, hist=big.clone())
    assert torch.equal(got, big + h1) and int(got.min()) > 1 << 32
    # a batch prefix: two label maps for three score maps score slices 0 and 1 only
    pre = ops.eval_confusion_batch(d(s1), d(l1[:2]), C)
    assert np.array_equal(pre.cpu().numpy(), K.counters(s1, l1[:2], C))
    other = s1.copy()
    other[2] = -other[2]                                               # (slice 2 is never read)
    assert torch.equal(ops.eval_confusion_batch(d(other), d(l1[:2]), C), pre)
    with pytest.raises(ValueError):
        ops.eval_confusion_batch(d(s1[:2]), d(l1), C)                  # more label maps than score maps
    for _ in range(3):
        assert torch.equal(ops.eval_confusion_batch(d(s1), d(l1), C), h1)
