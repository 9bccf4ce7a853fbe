"""backbone._GradLink on plain CPU tensors: the protocol between two adjacent conv nodes — the lower node's forward arms the link,
the upper node's backward leaves its masked data gradient (and the lower node's bias gradient, where there is one), the lower node's
backward takes the incoming gradient as masked only if it is that very tensor in that very version."""
import pytest
import torch

from dsrg_amd.backbone import _GradLink


def _left(scale=1.0, gb="bias"):
    lk, gx = _GradLink(), torch.randn(2, 3)
    lk.arm(scale)
    lk.leave(gx, torch.ones(3) if gb == "bias" else gb)
    return lk, gx


def test_accepted_on_the_very_tensor_left():
    lk, gx = _left()
    accepted, gb = lk.take(gx)
    assert accepted is True and torch.equal(gb, torch.ones(3))


def test_declined_on_another_tensor():
    lk, gx = _left()
    assert lk.take(gx.clone()) == (False, None)


def test_declined_after_an_in_place_write():
    lk, gx = _left()
    gx.add_(1.0)                                                         # same memory, a later version
    assert lk.take(gx) == (False, None)


def test_declined_after_a_second_take():
    lk, gx = _left()
    assert lk.take(gx)[0] is True
    assert lk.take(gx) == (False, None)                                  # the first take cleared what was left
    assert lk.gb is None


def test_a_declined_take_clears_what_was_left_too():
    lk, gx = _left()
    assert lk.take(gx.clone()) == (False, None)
    assert lk.take(gx) == (False, None) and lk.gb is None


def test_raises_when_declined_behind_a_dropout_scale():
    lk, gx = _left(scale=2.0)
    with pytest.raises(RuntimeError, match="one consumer"):
        lk.take(gx.clone())
    lk, gx = _left(scale=2.0)
    assert lk.take(gx)[0] is True                                        # accepted: the scale rode in the store
    assert lk.take(gx) == (False, None)                                  # nothing left: no consumer masked, nothing to raise about


def test_masked_without_a_bias_gradient_is_accepted_and_distinct_from_declined():
    lk, gx = _left(gb=None)
    assert lk.take(gx) == (True, None)
    lk, gx = _GradLink(), torch.randn(2, 3)
    lk.leave(gx)                                                         # gb defaults to None
    assert lk.take(gx) == (True, None)
    assert lk.take(gx) == (False, None)


def test_arm_discards_what_an_earlier_step_left():
    lk, gx = _left()
    lk.arm(1.0)
    assert lk.take(gx) == (False, None) and lk.gb is None
    lk, gx = _left(scale=2.0)
    lk.arm(1.0)
    assert lk.scale == 1.0 and lk.take(gx.clone()) == (False, None)      # the new step's scale decides whether declining raises


def test_a_fresh_link_is_armed_without_dropout_and_holds_nothing():
    lk = _GradLink()
    assert lk.scale == 1.0 and lk.take(torch.randn(2)) == (False, None)
