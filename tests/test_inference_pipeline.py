"""The one group pipeline of dsrg_amd/inference.py (inputs, forwards, one tail launch) behind ms, ms-f and gt.

CPU: the clone rule of inference._forwards, the only forwards loop.
GPU: predict_masks_ms_many(smooth=False) against the per-group / per-image functions it stands for, and the non-uint8 fallback
of inference._group_inputs with flip=True against the all-uint8 group.
"""
import numpy as np
import pytest
import torch

from test_flip_tta import ColumnNet, _E2E_SCALES, _E2E_SIZES, _e2e_images    # noqa: E402  (shared fixtures)


class _StaticOutputs(torch.nn.Module):
    """what a captured graph does with its output: one static tensor per input shape, refilled at every call (here with the
    number of the call); as a module it is the `net`, as a plain callable the `forward`"""

    def __init__(self):
        super().__init__()
        self.static, self.calls, self.modes = {}, 0, []

    def forward(self, x):
        self.calls += 1
        out = self.static.setdefault(tuple(x.shape), torch.empty((x.shape[0], 2) + tuple(x.shape[2:]), dtype=torch.float32))
        return out.fill_(float(self.calls))


def test_forwards_clones_a_static_output_only_where_its_shape_comes_again():
    from dsrg_amd import inference as I
    A, B = (1, 3, 5, 7), (1, 3, 4, 6)
    xs = [torch.zeros(s) for s in (A, B, A, A)]
    net = torch.nn.Dropout(0.5).train()
    graph = _StaticOutputs()

    def forward(x):
        graph.modes.append(net.training)
        return graph(x)

    maps = I._forwards(net, forward, xs)
    assert graph.calls == 4 and graph.modes == [False] * 4             # eval mode for the call ...
    assert net.training                                                 # ... and the trainer's mode afterwards
    for k, (m, x) in enumerate(zip(maps, xs)):
        assert m.dtype == torch.float32 and m.is_contiguous() and m.shape == (1, 2) + tuple(x.shape[2:])
        assert bool((m == float(k + 1)).all()), "map %d does not hold the values of its own call" % k
    ptrs = [m.untyped_storage().data_ptr() for m in maps]
    assert len({ptrs[0], ptrs[2], ptrs[3]}) == 3                        # the three A maps do not share storage
    assert maps[1] is graph.static[B]                                   # no later B: the static tensor itself, not a copy
    assert maps[3] is graph.static[A]                                   # the last A likewise

    # without `forward` the maps are whatever the module returned: nothing is cloned, whatever the shapes
    plain = _StaticOutputs().train()
    maps = I._forwards(plain, None, xs)
    assert plain.calls == 4 and plain.training
    assert maps[0] is maps[2] is maps[3] is plain.static[A] and maps[1] is plain.static[B]


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("forward_batch", [1, 4])
def test_predict_masks_ms_many_without_crf_is_the_per_group_and_per_image_functions(forward_batch, flip, graphed):
    """smooth=False: the masks of predict_masks_ms_batched(smooth=False, capacity=G) group by group (forward_batch = G > 1) and of
    predict_mask_ms(smooth=False) image by image (forward_batch = 1), bit for bit"""
    from dsrg_amd import inference as I
    ims = _e2e_images(89)                                               # 6 images: a full group of 4 and a tail group of 2, padded
    net = ColumnNet().cuda().eval()
    fwd, ref_fwd = (I.GraphedForward(net), I.GraphedForward(net)) if graphed else (None, None)
    got = list(I.predict_masks_ms_many(net, iter(ims), sizes=_E2E_SIZES, forward=fwd, forward_batch=forward_batch, flip=flip,
                                       smooth=False))
    if forward_batch == 1:
        want = [I.predict_mask_ms(net, im, smooth=False, sizes=_E2E_SIZES, forward=ref_fwd, flip=flip) for im in ims]
    else:
        want = [m for s in range(0, len(ims), forward_batch)
                for m in I.predict_masks_ms_batched(net, ims[s:s + forward_batch], smooth=False, sizes=_E2E_SIZES, forward=ref_fwd,
                                                    capacity=forward_batch, flip=flip)]
    assert len(got) == len(want) == len(ims)
    assert max(len(np.unique(m)) for m in want) >= 2, "the stand-in net must give masks of several labels"
    for k, (a, b, im) in enumerate(zip(got, want, ims)):
        assert a.dtype == np.int64 and a.shape == im.shape[:2], k
        assert np.array_equal(a, b), "mask %d differs on %d pixels" % (k, int((a != b).sum()))
    if graphed:
        assert sorted(fwd._g) == sorted(ref_fwd._g)


@pytest.mark.gpu
def test_flip_groups_take_float_images_through_the_per_slot_fallback():
    """a group whose middle image is float32 (whole-number pixel values) takes the per-slot route of inference._group_inputs —
    mirrors by torch.flip, zero padding, cat — and gives the masks of the all-uint8 group, which takes the one mirror launch"""
    from dsrg_amd import inference as I
    ims = _e2e_images(91)[:3]                                           # three 97 x 131 images
    assert len({im.shape for im in ims}) == 1
    mixed = [ims[0], ims[1].astype(np.float32), ims[2]]
    net = ColumnNet().cuda().eval()
    runs = (("ms", lambda group: I.predict_masks_ms_batched(net, group, sizes=_E2E_SIZES, capacity=4, flip=True)),
            ("ms-f", lambda group: list(I.predict_masks_ms_f_many(net, group, scales=_E2E_SCALES, same_size_batch=3, flip=True,
                                                                  smooth=False))))
    for tag, run in runs:
        got, want = run(mixed), run(ims)
        assert len(got) == len(want) == 3
        for k, (a, b) in enumerate(zip(got, want)):
            print("%s image %d: %d of %d pixels differ from the all-uint8 group" % (tag, k, int((a != b).sum()), a.size))
        for a, b in zip(got, want):
            assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)
