"""Guard words round a caller's buffers: what a call does to memory outside what it returns.

`guarded(shape, dtype, device)` hands out a view into one larger allocation that is full of a sentinel no route returns on finite
inputs; after the call `check()` asserts, by bit pattern, that the elements in front of and behind the view still hold it and that
every element of the view no longer does (include/rq.h defines a value for every slot, padding included).  `untouched()` is the
opposite assertion for a call the library refuses.  `frozen(tensor)` remembers the bits of an input.

The view starts FRONT = 17 elements into the allocation, so it is only naturally aligned for its element type: the alignment
include/rq.h ("Caller buffers") asks of a caller.  BACK holds the stray row of every pad slot of a 256-query pass, so an overrun is a
failed assertion and never a write into memory the test does not own.

Works on torch tensors of any device (tests/test_guarded.py tries it on the CPU).
"""
from __future__ import annotations

import math

import torch

FRONT = 17
PASS_SLOTS = 256                 # query slots of the widest pass: BACK holds one row per slot
MIN_BACK = 64

# dtype -> (the integer type of the same width, the sentinel's bits as a signed value of that type)
_BITS = {
    torch.float32: (torch.int32, 0x7FC0DEAD),                                # a quiet NaN with a payload
    torch.float64: (torch.int64, 0x7FF8DEADBEEF5A5A),                        # likewise
    torch.int32: (torch.int32, 0x5A5A5A5A),
    torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
    torch.uint64: (torch.int64, 0x5A5A5A5A5A5A5A5A),
}


def sentinel_bits(dtype) -> int:
    return _BITS[dtype][1]


def _as_bits(t: torch.Tensor) -> torch.Tensor:
    """The elements of a contiguous tensor as integers of the same width (a view)."""
    if t.dtype in _BITS:
        return t.view(_BITS[t.dtype][0])
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    def __init__(self, shape, dtype, device, per_query=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.shape, self.dtype = shape, dtype
        self.numel = math.prod(shape)
        if per_query is None:                                                # [B][k], [B][k][s], [B][cap] -> k, k*s, cap; [B] -> 1
            per_query = math.prod(shape[1:])
        self.back = max(PASS_SLOTS * int(per_query), MIN_BACK)
        ity, self.bits = _BITS[dtype]
        self._raw = torch.full((FRONT + self.numel + self.back,), self.bits, dtype=ity, device=device)      # the bits of every element
        self.view = self._raw[FRONT:FRONT + self.numel].view(dtype).view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() == self._raw.data_ptr() + FRONT * self._raw.element_size()

    # what the calls take: _native._ptr uses data_ptr()
    def data_ptr(self) -> int:
        return self.view.data_ptr()

    def _host(self):
        return self._raw.detach().cpu()

    @staticmethod
    def _first(bad: torch.Tensor) -> int:
        return int(torch.nonzero(bad)[0, 0])

    def _check_guards(self, host, what):
        front, back = host[:FRONT], host[FRONT + self.numel:]
        bad = front != self.bits
        if bool(bad.any()):
            i = self._first(bad)
            raise AssertionError(f"{what}: write in front of the buffer at offset {i - FRONT} (bits {int(front[i]) & (2 ** (8 * host.element_size()) - 1):#x})")
        bad = back != self.bits
        if bool(bad.any()):
            i = self._first(bad)
            raise AssertionError(f"{what}: write behind the buffer at offset {self.numel + i}, {i} past its {self.numel} elements "
                                 f"(bits {int(back[i]) & (2 ** (8 * host.element_size()) - 1):#x})")

    def check(self, what: str) -> None:
        """Guards intact, every slot of the view written."""
        host = self._host()
        self._check_guards(host, what)
        bad = host[FRONT:FRONT + self.numel] == self.bits
        if bool(bad.any()):
            raise AssertionError(f"{what}: slot at offset {self._first(bad)} of {self.numel} was left unwritten ({int(bad.sum())} in all)")

    def untouched(self, what: str) -> None:
        """A refused call: guards and view alike still hold the sentinel."""
        host = self._host()
        self._check_guards(host, what)
        bad = host[FRONT:FRONT + self.numel] != self.bits
        if bool(bad.any()):
            raise AssertionError(f"{what}: a refused call wrote the buffer at offset {self._first(bad)}")

    def cpu(self) -> torch.Tensor:
        return self.view.detach().cpu()

    def numpy(self):
        v = self.cpu()
        if v.dtype == torch.uint64:
            return v.view(torch.int64).numpy().view("uint64")
        return v.numpy()


def guarded(shape, dtype, device, per_query=None) -> Guarded:
    return Guarded(shape, dtype, device, per_query)


class Frozen:
    def __init__(self, tensor: torch.Tensor):
        assert tensor.is_contiguous()
        self.tensor = tensor
        self._before = _as_bits(tensor.detach().reshape(-1)).cpu().clone()

    def data_ptr(self) -> int:
        return self.tensor.data_ptr()

    def check(self, what: str) -> None:
        now = _as_bits(self.tensor.detach().reshape(-1)).cpu()
        bad = now != self._before
        if bool(bad.any()):
            raise AssertionError(f"{what}: input element at offset {int(torch.nonzero(bad)[0, 0])} of {now.numel()} was changed by the call")


def frozen(tensor: torch.Tensor) -> Frozen:
    return Frozen(tensor)
