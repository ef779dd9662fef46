"""The guard harness of tests/guarded.py against planted misbehaviour, on the CPU: a plain Python stand-in for a kernel goes wrong
in each of five ways, and the harness must report each with its offset; a well-behaved stand-in passes."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import FRONT, MIN_BACK, PASS_SLOTS, frozen, guarded, sentinel_bits  # noqa: E402

B, K = 3, 5
DTYPES = [torch.float32, torch.float64, torch.int32, torch.int64]


def _good_kernel(g, inp=None):
    """Writes every slot of the view, -1 / 0.0 padding included, and nothing else."""
    flat = g.view.view(-1)
    flat[:] = torch.arange(g.numel).to(g.dtype)
    flat[g.numel - 2:] = 0 if g.dtype.is_floating_point else -1


def _raw(g):
    """The whole allocation in the output's own type, for the planted writes."""
    return g._raw.view(g.dtype) if g.dtype.is_floating_point else g._raw


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_well_behaved_kernel_passes(dtype):
    g, inp = guarded((B, K), dtype, "cpu"), frozen(torch.arange(7, dtype=torch.float32))
    _good_kernel(g)
    g.check("good")
    inp.check("good input")
    with pytest.raises(AssertionError, match=r"refused call wrote the buffer at offset 0"):
        g.untouched("good")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_layout_is_as_documented(dtype):
    g = guarded((B, K), dtype, "cpu")
    assert FRONT == 17 and g.view.shape == (B, K) and g.view.dtype == dtype and g.view.is_contiguous()
    assert g._raw.numel() == FRONT + B * K + PASS_SLOTS * K
    assert g.data_ptr() == g._raw.data_ptr() + FRONT * g.view.element_size()
    assert g.data_ptr() % g.view.element_size() == 0
    assert guarded((B,), dtype, "cpu").back == PASS_SLOTS and guarded((B, 2, 3), dtype, "cpu").back == PASS_SLOTS * 6
    assert guarded((B, K), dtype, "cpu", per_query=0).back == MIN_BACK
    bits = g._raw
    assert bool((bits == sentinel_bits(dtype)).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.view).all())          # no finite input gives a NaN
    g.untouched("fresh")
    with pytest.raises(AssertionError, match=r"slot at offset 0 of 15 was left unwritten \(15 in all\)"):
        g.check("fresh")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_past_the_end_is_reported(dtype):
    g = guarded((B, K), dtype, "cpu")
    _good_kernel(g)
    _raw(g)[FRONT + B * K] = 1
    with pytest.raises(AssertionError, match=r"past: write behind the buffer at offset 15, 0 past its 15 elements"):
        g.check("past")
    with pytest.raises(AssertionError, match=r"write behind the buffer at offset 15"):
        g.untouched("past")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_in_front_is_reported(dtype):
    g = guarded((B, K), dtype, "cpu")
    _good_kernel(g)
    _raw(g)[FRONT - 1] = 1
    with pytest.raises(AssertionError, match=r"front: write in front of the buffer at offset -1 "):
        g.check("front")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_whole_pad_row_behind_is_reported(dtype):
    """Slot 255 of a 256-query pass that served B = 3 queries writes its row: [255][0..K) relative to the view."""
    g = guarded((B, K), dtype, "cpu")
    _good_kernel(g)
    row = FRONT + (PASS_SLOTS - 1) * K
    _raw(g)[row:row + K] = -1
    assert row + K <= g._raw.numel()                   # BACK holds it: the write stays inside the allocation
    with pytest.raises(AssertionError, match=rf"pad: write behind the buffer at offset {(PASS_SLOTS - 1) * K}, {(PASS_SLOTS - 1 - B) * K} past"):
        g.check("pad")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_slot_left_unwritten_is_reported(dtype):
    g = guarded((B, K), dtype, "cpu")
    _good_kernel(g)
    g._raw[FRONT + 7] = sentinel_bits(dtype)                            # the kernel skipped slot 7: it still holds the sentinel
    with pytest.raises(AssertionError, match=r"gap: slot at offset 7 of 15 was left unwritten \(1 in all\)"):
        g.check("gap")


@pytest.mark.parametrize("dtype", DTYPES + [torch.uint8])
def test_one_input_element_changed_is_reported(dtype):
    t = torch.arange(12).to(dtype).view(3, 4).contiguous()
    inp = frozen(t)
    inp.check("input")
    t[2, 1] += 1
    with pytest.raises(AssertionError, match=r"input: input element at offset 9 of 12 was changed by the call"):
        inp.check("input")


def test_a_negative_zero_for_a_zero_is_a_change():
    """By bit pattern, not by value."""
    t = torch.zeros(4, dtype=torch.float32)
    inp = frozen(t)
    t[3] = -0.0
    with pytest.raises(AssertionError, match=r"offset 3 of 4"):
        inp.check("sign")
