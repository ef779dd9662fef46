"""The router gate: the forward pass of the reference's RetrievalRouter (rag_uq/router.py:74-177) and the rerank the evaluation loop
applies with it (experiments/run_evaluation.py:165-184), in the float64 definition of include/rq.h "router gate".

`RouterGate` holds the weights of a router with one or two layers.  `gate` and `rerank` are the numpy float64 host implementation of
that definition -- product code, what `HybridRetriever.route_batch` runs when the device route is not taken; `native(device)` is the
same gate on a device (`_native.RouterGate`, csrc/rq_router.hip), which reports the same bits except for the last ulps of exp.

Normalisation is "query" (each question's columns by their own mean and unbiased standard deviation: what the evaluation loop gets
from a restored checkpoint, one question at a time) or "stats" (the four running statistics).  The reference's batch-wise form over a
whole [B][P] tensor is not offered: a question's answer would depend on its neighbours in the batch.
"""
from __future__ import annotations

import re
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import _native

_EPS = 1e-6
_STAT_KEYS = ("bm25_mean", "bm25_std", "dense_mean", "dense_std")


def _array(x, dtype=np.float32) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _tree_sum(x: np.ndarray) -> np.ndarray:
    """S of the definition over the last axis of x [B][P]: pad with +0.0 to the next power of two n, then a[i] = a[i] + a[i + n/2]
    for i < n/2, n halved each time."""
    B, P = x.shape
    n = 1
    while n < P:
        n <<= 1
    a = np.zeros((B, n), np.float64)
    a[:, :P] = x
    while n > 1:
        n >>= 1
        a = a[:, :n] + a[:, n: 2 * n]
    return a[:, 0]


class RouterGate:
    """Weights of a RetrievalRouter with `num_layers` 1 (w1 [3], b1) or 2 (w0 [H][3], b0 [H], w1 [H], b1), fp32 as in a state dict,
    widened exactly; read-only after creation."""

    def __init__(self, w0, b0, w1, b1, *, num_layers: int = 2, use_batch_norm: bool = False, stats=None, normalize: str = "query"):
        if use_batch_norm:
            raise ValueError("use_batch_norm: a router with batch norm is not supported")
        if num_layers not in (1, 2):
            raise ValueError(f"num_layers {num_layers}: only routers with 1 or 2 layers are supported")
        self.num_layers = int(num_layers)
        self.w1 = _array(w1).reshape(-1)
        self.b1 = np.float32(_array(b1).reshape(-1)[0])
        if self.num_layers == 2:
            self.w0, self.b0 = _array(w0), _array(b0).reshape(-1)
            H = self.w0.shape[0] if self.w0.ndim == 2 else -1
            if self.w0.ndim != 2 or self.w0.shape[1] != 3 or self.b0.shape != (H,) or self.w1.shape != (H,):
                raise ValueError(f"w0 [H][3], b0 [H] and w1 [H] expected, got {self.w0.shape}, {self.b0.shape} and {self.w1.shape}")
            if not 1 <= H <= _native.ROUTER_MAX_HIDDEN:
                raise ValueError(f"hidden {H} outside 1..{_native.ROUTER_MAX_HIDDEN}")
            self.hidden = H
        else:
            if self.w1.shape != (3,):
                raise ValueError(f"one layer takes w1 [3], got {self.w1.shape}")
            self.w0 = self.b0 = None
            self.hidden = 0
        self.stats = np.array([0.0, 1.0, 0.0, 1.0]) if stats is None else self._four(stats)
        self.normalize = normalize
        self._native: Dict[int, Any] = {}

    # ---- construction ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, hidden: Optional[int] = None, *, normalize: str = "query") -> "RouterGate":
        """From `RetrievalRouter.state_dict()` (tensors, arrays or lists): `scorer.0.*`, `scorer.3.*` and the four statistics buffers.
        A state dict does not say whether the statistics were ever set (`stats_initialized` is a plain attribute), so the gate
        normalises per query unless told otherwise -- as a router restored from a checkpoint does."""
        if any("running_mean" in k or "running_var" in k for k in sd):
            raise ValueError("use_batch_norm: a router with batch norm is not supported")
        layers = sorted({int(m.group(1)) for m in (re.fullmatch(r"scorer\.(\d+)\.weight", k) for k in sd) if m})
        if layers == [0, 3]:
            gate = cls(sd["scorer.0.weight"], sd["scorer.0.bias"], sd["scorer.3.weight"], sd["scorer.3.bias"], num_layers=2, normalize=normalize)
        elif layers == [0]:
            gate = cls(None, None, sd["scorer.0.weight"], sd["scorer.0.bias"], num_layers=1, normalize=normalize)
        else:
            raise ValueError(f"linear layers at scorer.{layers}: only routers with 1 or 2 layers (and no batch norm) are supported")
        if hidden is not None and int(hidden) != gate.hidden:
            raise ValueError(f"hidden {hidden} given, the state dict holds {gate.hidden}")
        if all(k in sd for k in _STAT_KEYS):
            gate.stats = cls._four([float(_array(sd[k], np.float64).reshape(-1)[0]) for k in _STAT_KEYS])
        return gate

    @classmethod
    def from_module(cls, module) -> "RouterGate":
        """From a live RetrievalRouter: its state dict, and "stats" normalisation when its running statistics are initialised."""
        config = getattr(module, "config", None)
        if config is not None and getattr(config, "use_batch_norm", False):
            raise ValueError("use_batch_norm: a router with batch norm is not supported")
        return cls.from_state_dict(module.state_dict(), normalize="stats" if getattr(module, "stats_initialized", False) else "query")

    @staticmethod
    def _four(stats) -> np.ndarray:
        stats = np.asarray(stats, np.float64).reshape(-1)
        if stats.shape != (4,):
            raise ValueError("router statistics are (bm25_mean, bm25_std, dense_mean, dense_std)")
        return stats.copy()

    def set_stats(self, bm25_mean: float, bm25_std: float, dense_mean: float, dense_std: float) -> None:
        """The running statistics; like the reference's `update_stats`, setting them switches the gate to normalize="stats"."""
        self.stats = self._four([bm25_mean, bm25_std, dense_mean, dense_std])
        self.normalize = "stats"

    @property
    def normalize(self) -> str:
        return self._normalize

    @normalize.setter
    def normalize(self, value: str) -> None:
        if value not in ("query", "stats"):
            raise ValueError(f"normalize must be 'query' or 'stats', not {value!r}")
        self._normalize = value

    @property
    def mode(self) -> int:
        return _native.ROUTER_NORM_QUERY if self._normalize == "query" else _native.ROUTER_NORM_STATS

    # ---- the device ------------------------------------------------------------------------------------------------------------------
    def native(self, device: int = 0) -> "_native.RouterGate":
        """The same weights on `device` (`_native.RouterGate`), made on first use; RqError without a gfx950 device."""
        if device not in self._native:
            self._native[device] = _native.RouterGate(self.w0, self.b0, self.w1, float(self.b1), num_layers=self.num_layers, device=device)
        return self._native[device]

    def close(self) -> None:
        for handle in self._native.values():
            handle.close()
        self._native = {}

    # ---- the definition on the host -----------------------------------------------------------------------------------------------
    def _normalized(self, b: np.ndarray, d: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        if self._normalize == "stats":
            mean_b, std_b, mean_d, std_d = self.stats
            return (b - mean_b) / (std_b + _EPS), (d - mean_d) / (std_d + _EPS)
        out = []
        P = np.float64(b.shape[1])
        for x in (b, d):
            mean = _tree_sum(x) / P
            e = x - mean[:, None]
            var = _tree_sum(e * e) / (P - 1.0)
            out.append(e / (np.sqrt(var) + _EPS)[:, None])
        return out[0], out[1]

    def gate(self, b, d) -> np.ndarray:
        """w [B][P] in input order (RetrievalRouter.forward) of the columns b, d [B][P] -- a single column [P] is one question."""
        b, d = np.asarray(b, np.float64), np.asarray(d, np.float64)
        single = b.ndim == 1
        b, d = np.atleast_2d(b), np.atleast_2d(d)
        if b.ndim != 2 or b.shape != d.shape or b.shape[1] < 1:
            raise ValueError(f"router columns are [B][P] twice, got {b.shape} and {d.shape}")
        with np.errstate(all="ignore"):
            nb, nd = self._normalized(b, d)
            df = nd - nb
            if self.num_layers == 1:
                w1 = self.w1.astype(np.float64)
                z = ((w1[0] * nb + w1[1] * nd) + w1[2] * df) + np.float64(self.b1)
            else:
                w0, b0, w1 = self.w0.astype(np.float64), self.b0.astype(np.float64), self.w1.astype(np.float64)
                z = np.zeros(b.shape, np.float64)
                for j in range(self.hidden):
                    a = ((w0[j, 0] * nb + w0[j, 1] * nd) + w0[j, 2] * df) + b0[j]
                    z = z + w1[j] * np.where(a > 0, a, 0.0)
                z = z + np.float64(self.b1)
            w = 1.0 / (1.0 + np.exp(-z))
        return w[0] if single else w

    def rerank(self, keys, b, d, count, top_k: int):
        """The best min(candidates, top_k) positions of every question by h = w*d + (1 - w)*b: (keys int32, b, d, w, h float64,
        positions int32 -- all [B][top_k] -- and count int32 [B]).  Candidates are the positions below count[q] with a key >= 0; h
        descending, -0.0 as +0.0, a NaN as -inf, equal h by ascending position; entries beyond the count are (-1, 0, 0, 0, 0, -1)."""
        b, d = np.atleast_2d(np.asarray(b, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        keys = np.atleast_2d(np.asarray(keys)).astype(np.int32)
        count = np.asarray(count).reshape(-1).astype(np.int64)
        B, P = b.shape
        top_k = int(top_k)
        if keys.shape != b.shape or d.shape != b.shape or count.shape != (B,) or not 1 <= top_k <= P:
            raise ValueError(f"router rerank: keys {keys.shape}, b {b.shape}, d {d.shape}, count {count.shape}, top_k {top_k}")
        w = self.gate(b, d)
        return rerank_given_w(keys, b, d, w, count, top_k)


def rerank_given_w(keys: np.ndarray, b: np.ndarray, d: np.ndarray, w: np.ndarray, count: np.ndarray, top_k: int):
    """The rerank of the definition for given gate weights (everything after exp)."""
    B, P = b.shape
    with np.errstate(all="ignore"):
        h = w * d + (1.0 - w) * b
    cand = (np.arange(P)[None, :] < np.clip(count, 0, P)[:, None]) & (keys >= 0)
    rank = np.where(np.isnan(h), -np.inf, h)
    rank = np.where(rank == 0, 0.0, rank)
    order = np.lexsort((-rank, ~cand), axis=1)[:, :top_k]              # stable: equal h by ascending position, candidates first
    out_count = np.minimum(cand.sum(axis=1), top_k).astype(np.int32)
    live = np.arange(top_k)[None, :] < out_count[:, None]
    take = lambda x, fill: np.where(live, np.take_along_axis(x, order, 1), fill)
    return (take(keys, -1).astype(np.int32), take(b, 0.0), take(d, 0.0), take(w, 0.0), take(h, 0.0), take(np.broadcast_to(np.arange(P), (B, P)), -1).astype(np.int32),
            out_count)
