"""A deterministic embedder with a host route and a device route that see the SAME numbers -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

DenseIndex and HybridRetriever take a different path through streaming_index.py when the embedder offers `embed_device` (the query
matrix stays in HBM: `_search_device_rows`, `_score_device_rows`, `_fuse_batch_device` with the embedder's tensor).  An encoder cannot
pin that path bit for bit: its forward need not repeat.  DeviceTwinEmbedder can: text -> vector is a table (or a function) of the
test's, `embed(texts)` returns the float32 matrix and `embed_device(texts)` the same values as a tensor on `device`, so the answers of
the two routes are compared in their bits.

    table: {"q": Q, "p": X}     "q17" -> Q[17], "p123" -> X[123]  (one letter, then the row)
    function: fn(text) -> [dim] (e.g. `seeded_gaussian(dim)`: one Gaussian vector per distinct text)

Modes: dtype="float16" (the tensor is fp16, `embed` returns the fp32 image of the fp16-rounded values: `.to(torch.float32)` is
exercised and both routes still see identical numbers); strided=True (the tensor is every second column of a [B][2 dim] buffer: not
contiguous, `.contiguous()` is exercised); fail_after=n (`embed_device` raises from its n-th call on: the fall-back).  Counters:
`host_calls`, `device_calls` (calls that returned a matrix), `device_failures` (calls that raised).  `host_twin()` is the same mapping
WITHOUT `embed_device`: the embedder of the index the device route is compared with."""
import hashlib
from typing import Callable, Dict, Optional, Sequence, Union

import numpy as np


def seeded_gaussian(dim: int) -> Callable[[str], np.ndarray]:
    """text -> a standard Gaussian float32 vector seeded by SHA-256 of the text; the vector of a text is computed once."""
    cache: Dict[str, np.ndarray] = {}

    def fn(text: str) -> np.ndarray:
        v = cache.get(text)
        if v is None:
            seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
            v = cache[text] = np.random.default_rng(seed).standard_normal(dim).astype(np.float32)
        return v

    return fn


class _Mapping:
    """text -> float32 row, shared by the device twin and its host twin."""

    def __init__(self, table_or_fn: Union[Dict[str, np.ndarray], Callable[[str], np.ndarray]], dim: int, dtype: str):
        if dtype not in ("float32", "float16"):
            raise ValueError(f"dtype must be 'float32' or 'float16', not {dtype!r}")
        self.dim, self.dtype = int(dim), dtype
        if callable(table_or_fn):
            self.fn, self.table = table_or_fn, None
        else:
            self.fn, self.table = None, {key: np.asarray(m) for key, m in table_or_fn.items()}
            for key, m in self.table.items():
                if len(key) != 1 or m.ndim != 2 or m.shape[1] != self.dim:
                    raise ValueError(f"table entry {key!r}: one letter -> [n][{self.dim}] matrix expected, got {m.shape}")

    def row(self, text: str) -> np.ndarray:
        if self.fn is not None:
            v = np.asarray(self.fn(text), dtype=np.float32)
        else:
            if not text or text[0] not in self.table:
                raise KeyError(f"no table for {text!r}")
            v = self.table[text[0]][int(text[1:])].astype(np.float32)
        if v.shape != (self.dim,):
            raise ValueError(f"{text!r} maps to shape {v.shape}, expected ({self.dim},)")
        return v

    def matrix(self, texts: Sequence[str]) -> np.ndarray:
        """float32 [len(texts)][dim]; under dtype "float16" every value is fp16-representable (rounded once, here)."""
        out = np.zeros((len(texts), self.dim), dtype=np.float32)
        for i, t in enumerate(texts):
            out[i] = self.row(t)
        if self.dtype == "float16":
            with np.errstate(over="ignore"):
                out = out.astype(np.float16).astype(np.float32)
        return out


class HostTwinEmbedder:
    """The mapping of a DeviceTwinEmbedder with a host route only (no `embed_device`)."""

    def __init__(self, mapping: _Mapping):
        self._mapping, self.dim = mapping, mapping.dim
        self.host_calls = 0

    def embed(self, texts: Sequence[str]) -> np.ndarray:
        self.host_calls += 1
        return self._mapping.matrix(list(texts))


class DeviceTwinEmbedder:
    def __init__(self, table_or_fn, dim: int, device="cpu", *, dtype: str = "float32", strided: bool = False, fail_after: Optional[int] = None):
        self._mapping = _Mapping(table_or_fn, dim, dtype)
        self.dim, self.device, self.dtype, self.strided = int(dim), device, dtype, bool(strided)
        self.fail_after = None if fail_after is None else int(fail_after)
        self.host_calls = self.device_calls = self.device_failures = 0

    def host_twin(self) -> HostTwinEmbedder:
        return HostTwinEmbedder(self._mapping)

    def embed(self, texts: Sequence[str]) -> np.ndarray:
        self.host_calls += 1
        return self._mapping.matrix(list(texts))

    def embed_device(self, texts: Sequence[str]):
        import torch
        if self.fail_after is not None and self.device_calls + self.device_failures + 1 >= self.fail_after:
            self.device_failures += 1
            raise RuntimeError(f"DeviceTwinEmbedder: embed_device fails from call {self.fail_after} on")
        v = self._mapping.matrix(list(texts))
        tdtype = torch.float16 if self.dtype == "float16" else torch.float32
        t = torch.from_numpy(v).to(tdtype)                       # (fp16: exact, the values were rounded in `matrix`)
        if self.strided:
            wide = torch.full((v.shape[0], 2 * self.dim), 7.0, dtype=tdtype)      # the odd columns hold a value no answer may show
            wide[:, ::2] = t
            out = wide.to(self.device)[:, ::2]
        else:
            out = t.to(self.device)
        self.device_calls += 1
        return out
