"""Drop-in mirror of reference `rag_uq/streaming_index.py` with the dense path on MI355X.

Same module-level names, constructor signatures, defaults and return conventions as the reference
(Document :54-77, RetrievalResult :80-89, BM25Index :92-225, DenseIndex :228-373, HybridRetriever
:376-560, StreamingIndex :563-686), so `experiments/run_evaluation.py:165-167`,
`experiments/run_router_training.py:80-82` and `data/preprocessing/build_chroma_index.py:55-125`
run unchanged against it.  What differs underneath:

  * DenseIndex keeps the passage vectors as an fp16 matrix in HBM and answers `search` with an exact
    cosine top-k computed by hand-written HIP kernels (librq_hip.so, include/rq.h) instead of
    ChromaDB/HNSW; embeddings come from an in-process embedder instead of one Ollama HTTP request
    per text.  There is no CPU fallback for this class.
  * BM25Index restates rank-bm25's BM25Okapi (not installed here) over an inverted index, so adding
    documents no longer rebuilds the whole model.  It stays on the CPU (BASELINE.json configs[4]).
  * Batched entry points are added next to the single-query ones (`search_batch`,
    `hybrid_search_batch`, `get_scores_for_router_batch`); the originals are thin wrappers.
"""
from __future__ import annotations

import gc
import io
import json
import logging
import math
import os
import pickle
from collections import Counter
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .embedders import default_embedder

logger = logging.getLogger(__name__)


def _gpu_backend_available() -> bool:
    """True when librq_hip.so loads and sees a device.  A missing library raises (loud), a missing
    GPU only disables dense retrieval, like the reference's HAS_CHROMA switch (:31-37, :412-420)."""
    return _native.device_count() > 0


# =============================================================================================
# records (reference :54-89)
# =============================================================================================
@dataclass
class Document:
    """A document for indexing."""
    id: str
    text: str
    title: Optional[str] = None
    metadata: Optional[Dict[str, Any]] = None

    def to_dict(self) -> Dict[str, Any]:
        return {"id": self.id, "text": self.text, "title": self.title or "", "metadata": self.metadata or {}}

    @classmethod
    def from_dict(cls, data: Dict[str, Any]) -> "Document":
        return cls(id=data["id"], text=data["text"], title=data.get("title"), metadata=data.get("metadata"))


@dataclass
class RetrievalResult:
    """Result from hybrid retrieval."""
    doc_id: str
    text: str
    bm25_score: float
    dense_score: float
    hybrid_score: Optional[float] = None
    title: Optional[str] = None
    metadata: Optional[Dict[str, Any]] = None


class _PlainUnpickler(pickle.Unpickler):
    """The BM25 snapshot holds dicts, lists, strings and floats only (reference :189-201), so loading it needs no global
    at all: refusing every class lookup keeps the file format and removes pickle's code-execution surface."""

    def find_class(self, module, name):
        raise pickle.UnpicklingError(f"BM25 snapshot must not reference {module}.{name}")


def _load_plain_pickle(path) -> Any:
    with open(path, "rb") as f:
        return _PlainUnpickler(io.BytesIO(f.read())).load()


def _atomic_write(path: Path, data: bytes) -> None:
    tmp = Path(str(path) + ".tmp")
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


# ---- grouping (`distinct_by=`): the value a passage is grouped by, on both sides ------------------------------------------
def _meta_group_value(meta: Optional[Dict[str, Any]], key: str):
    """The value a passage is grouped by (`distinct_by=`): its metadata's `key`; None -- a group of its own -- when the key is
    missing or holds "" / None.  Unhashable values are grouped by their repr."""
    value = (meta or {}).get(key)
    if value is None or value == "":
        return None
    try:
        hash(value)
    except TypeError:
        return repr(value)
    return value


def _per_group_size(distinct_by: Optional[str], per_group: Optional[int]) -> int:
    """`per_group=` (how many passages of each group a `distinct_by=` search returns) as a checked int; absent = 1."""
    if per_group is None:
        return 1
    if distinct_by is None:
        raise ValueError("per_group needs distinct_by")
    if isinstance(per_group, bool) or not isinstance(per_group, (int, np.integer)) or int(per_group) < 1:
        raise ValueError(f"per_group must be an integer >= 1, got {per_group!r}")
    return int(per_group)


def _refuse_per_group(per_group: Optional[int], what: str) -> None:
    """The calls that return one passage per group only (the sparse side, the fused lists, the row forms)."""
    if per_group is not None and (isinstance(per_group, bool) or not isinstance(per_group, (int, np.integer)) or int(per_group) != 1):
        raise ValueError(f"{what} returns one passage per group: per_group={per_group!r} is not supported (use DenseIndex.search)")


def _given(**keywords) -> Dict[str, Any]:
    """Only the keywords that were given (not None): an index of someone else's, whose `search(query, top_k)` knows none of the
    extensions, is never handed one its caller did not use."""
    return {name: value for name, value in keywords.items() if value is not None}


def _with_made_filters(entries, passes, make, call):
    """`call(filters)`, one filter per entry: an entry that `passes` stays as it is; any other becomes `make(entry)` -- made once per distinct
    OBJECT, in the order of the entries -- and is closed once the call has returned or raised (the `_with_filters` of both classes)."""
    made = {}
    try:
        filters = []
        for e in entries:
            if not passes(e):
                if id(e) not in made:
                    made[id(e)] = make(e)
                e = made[id(e)]
            filters.append(e)
        return call(filters)
    finally:
        for flt in made.values():
            flt.close()


def _group_value(doc: "Document", key: str):
    """... of a Document: the metadata DenseIndex.add_documents stores for it, {"title": title, **metadata}."""
    return _meta_group_value({"title": doc.title or "", **(doc.metadata or {})}, key)


class SparseMask:
    """The BM25 rows of one set of ids as mask words (`BM25Index.make_mask`; include/rq_bm25.h rq_bm25_topk_masked: bit r % 32 of
    word r / 32 = row r is allowed).  It describes the corpus as it is now: adding documents makes it stale."""

    __slots__ = ("words", "n_docs", "count")

    def __init__(self, words: np.ndarray, n_docs: int, count: int):
        self.words, self.n_docs, self.count = words, int(n_docs), int(count)

    def __len__(self) -> int:
        return self.count


# =============================================================================================
# sparse side (reference :92-225).  CPU, host logic.
# =============================================================================================
class BM25Index:
    """BM25Okapi over an inverted index; same API, pickle layout and scores as the reference class.

    Scoring restates rank-bm25 0.2.2 `BM25Okapi` (requirements.txt:8; not vendored, not installed):
      idf(t)  = ln(N - n_t + 0.5) - ln(n_t + 0.5); negative idfs are replaced by 0.25 * mean(idf)
      score   = sum over query tokens t (with repetition) of
                idf(t) * f * (k1 + 1) / (f + k1 * (1 - b + b * dl / avgdl))
    `search` keeps the reference's selection verbatim (:172-177): argsort, reversed, first top_k,
    score > 0 only.

    Persistence.  The reference rebuilds BM25Okapi and re-pickles the WHOLE index on every add_documents (:141-146,
    :185-201): O(N^2) bytes over an indexing run (10 000 full dumps for 1M passages in batches of 100).  Here an add
    appends its documents to `<persist_path>.log.jsonl`; the snapshot at `persist_path` keeps the reference's pickle
    layout and is rewritten (atomically) when the log has grown as large as the snapshot (so total snapshot bytes stay
    linear), on `save()` and on `close()`.  Loading = snapshot + replay of the log.  `snapshot_every=1` restores the
    reference's "pickle on every add".
    """

    EPSILON = 0.25
    SNAPSHOT_MIN_DOCS = 10_000

    def __init__(self, persist_path: Optional[str] = None, k1: float = 1.5, b: float = 0.75, *, snapshot_every: Optional[int] = None):
        self.persist_path = Path(persist_path) if persist_path else None
        self.snapshot_every = snapshot_every
        self._snapshot_docs = 0        # documents covered by the snapshot file
        self._log_file = None
        self.k1 = k1
        self.b = b
        self.documents: Dict[str, Document] = {}
        self.doc_ids: List[str] = []
        self.tokenized_corpus: List[List[str]] = []
        # inverted index: token -> (doc rows, term frequencies), appended in row order
        self._post_rows: Dict[str, List[int]] = {}
        self._post_tf: Dict[str, List[int]] = {}
        self._doc_len: List[int] = []
        self._total_len = 0
        self._idf: Optional[Dict[str, float]] = None   # None = stale
        if self.persist_path and (self.persist_path.exists() or self._log_path().exists()):
            self._load()

    @property
    def bm25(self):
        """The reference exposes the BM25Okapi object; callers only test it for None (:165)."""
        return self if self.doc_ids else None

    def _tokenize(self, text: str) -> List[str]:
        return text.lower().split()

    def _index_tokens(self, row: int, tokens: List[str]) -> None:
        for tok, tf in Counter(tokens).items():
            self._post_rows.setdefault(tok, []).append(row)
            self._post_tf.setdefault(tok, []).append(tf)
        self._doc_len.append(len(tokens))
        self._total_len += len(tokens)
        self._idf = None

    def add_documents(self, documents: List[Document]) -> int:
        new_count = 0
        for doc in documents:
            if doc.id in self.documents:
                continue
            self.documents[doc.id] = doc
            self.doc_ids.append(doc.id)
            toks = self._tokenize(doc.text)
            self.tokenized_corpus.append(toks)
            self._index_tokens(len(self.doc_ids) - 1, toks)
            new_count += 1
        if new_count:
            logger.info(f"Added {new_count} documents to BM25 index. Total: {len(self.doc_ids)}")
        if self.persist_path and new_count:
            self._persist_new(len(self.doc_ids) - new_count)
        return new_count

    def _ensure_idf(self) -> Dict[str, float]:
        if self._idf is not None:
            return self._idf
        n_docs = len(self.doc_ids)
        idf: Dict[str, float] = {}
        idf_sum = 0.0
        negative: List[str] = []
        for tok, rows in self._post_rows.items():   # insertion order = first-seen order, as BM25Okapi's nd dict
            n_t = len(rows)
            v = math.log(n_docs - n_t + 0.5) - math.log(n_t + 0.5)
            idf[tok] = v
            idf_sum += v
            if v < 0:
                negative.append(tok)
        if idf:
            eps = self.EPSILON * (idf_sum / len(idf))
            for tok in negative:
                idf[tok] = eps
        self._idf = idf
        return idf

    def _np_doc_len(self) -> np.ndarray:
        cache = getattr(self, "_doc_len_np", None)
        if cache is None or len(cache) != len(self._doc_len):
            cache = self._doc_len_np = np.asarray(self._doc_len, dtype=np.float64)
        return cache

    def _np_postings(self, tok: str, rows: List[int]) -> Tuple[np.ndarray, np.ndarray]:
        """numpy views of a token's posting list, rebuilt when the list has grown (the lists are append-only).  Converting the
        Python lists on every query was 70 % of a search over 50 k passages (cProfile: 4.9 of 7.0 ms per query)."""
        cache = self.__dict__.setdefault("_post_np", {})
        hit = cache.get(tok)
        if hit is None or len(hit[0]) != len(rows):
            hit = cache[tok] = (np.asarray(rows, dtype=np.int64), np.asarray(self._post_tf[tok], dtype=np.float64))
        return hit

    def _token_contribution(self, tok: str, rows: List[int], idf: Dict[str, float], avgdl: float) -> Tuple[np.ndarray, np.ndarray]:
        """(rows, idf * tf-saturation per row) of one token for the CURRENT corpus: the same expression the per-query loop used
        to evaluate, kept until the next add (idf and avgdl change with every added document)."""
        n_docs = len(self.doc_ids)
        cache = self.__dict__.setdefault("_contrib", {})
        if cache.get("#docs") != n_docs:
            cache.clear()
            cache["#docs"] = n_docs
        hit = cache.get(tok)
        if hit is None:
            r, f = self._np_postings(tok, rows)
            w = idf.get(tok) or 0
            hit = cache[tok] = (r, w * (f * (self.k1 + 1) / (f + self.k1 * (1 - self.b + self.b * self._np_doc_len()[r] / avgdl))))
        return hit

    def get_scores(self, tokenized_query: List[str]) -> np.ndarray:
        n_docs = len(self.doc_ids)
        scores = np.zeros(n_docs)
        if n_docs == 0:
            return scores
        idf = self._ensure_idf()
        avgdl = self._total_len / n_docs
        for tok in tokenized_query:
            rows = self._post_rows.get(tok)
            if not rows:
                continue
            r, c = self._token_contribution(tok, rows, idf, avgdl)
            scores[r] += c
        return scores

    def _score_rows_tokens(self, tokens: List[str], rows: np.ndarray) -> np.ndarray:
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        out = np.zeros(rows.size)
        n_docs = len(self.doc_ids)
        if n_docs == 0 or rows.size == 0:
            return out
        inside = (rows >= 0) & (rows < n_docs)
        if not inside.any():
            return out
        idf = self._ensure_idf()
        avgdl = self._total_len / n_docs
        for tok in tokens:
            post = self._post_rows.get(tok)
            if not post:
                continue
            r, c = self._token_contribution(tok, post, idf, avgdl)
            at = np.minimum(np.searchsorted(r, rows), len(r) - 1)      # (posting rows ascend: they are appended in row order)
            hit = inside & (r[at] == rows)
            out[hit] += c[at[hit]]
        return out

    def score_rows(self, query: str, rows) -> np.ndarray:
        """`get_scores(tokens)[rows]` (float64 [m]) without one float per PASSAGE (extension): per query token, in order, the token's
        posting rows are searched for the given rows and its cached contribution is added where a row is present -- the same
        additions per row in the same order, hence the same bits.  Rows < 0 (and rows the index does not hold) score 0.0; rows may
        repeat."""
        return self._score_rows_tokens(self._tokenize(query), rows)

    def score_rows_batch(self, queries: Sequence[str], rows, *, backend: str = "host") -> np.ndarray:
        """`score_rows` for one list of rows per query: rows [B][m] -> float64 [B][m].
        `backend` as in `search_batch_rows`: "host" (default) is the loop below; "gpu" scores every pair on the device (include/rq.h
        rq_sparse_score_rows over the `_native.SparseIndex` of the current corpus: the same bits; m <= 65 536, at most 65 535 queries;
        RqError without a device); "auto" takes the device when one is visible."""
        if backend not in ("host", "gpu", "auto"):
            raise ValueError(f"backend must be 'host', 'gpu' or 'auto', not {backend!r}")
        rows = np.asarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[0] != len(queries):
            raise ValueError(f"expected [{len(queries)}][m] rows, one list per query, got {rows.shape}")
        if (backend == "gpu" or (backend == "auto" and _native.sparse_available())) and self.doc_ids and rows.size:
            c = self._csr()
            q_ptr, q_tok = self._query_csr(c, queries)
            inside = (rows >= 0) & (rows < len(self.doc_ids))
            return self._sparse_index(c).score_rows(q_ptr, q_tok, len(queries), np.where(inside, rows, -1).astype(np.int32))
        out = np.zeros(rows.shape)
        for b, q in enumerate(queries):
            if (rows[b] >= 0).any():
                out[b] = self._score_rows_tokens(self._tokenize(q), rows[b])
        return out

    def _row_of_id(self) -> Dict[str, int]:
        """id -> row (first occurrence), rebuilt when documents were added"""
        c = self.__dict__.get("_row_of_cache")
        if c is None or c[0] != len(self.doc_ids):
            table: Dict[str, int] = {}
            for i, d in enumerate(self.doc_ids):
                table.setdefault(d, i)
            c = self.__dict__["_row_of_cache"] = (len(self.doc_ids), table)
        return c[1]

    @staticmethod
    def _select_topk(scores: np.ndarray, top_k: int) -> np.ndarray:
        """Rows of the reference's selection (:172-177: argsort, reversed, first top_k, score > 0 only) without sorting the whole
        score vector (80 % of a search over 50 k passages).  Exact ties -- which numpy's default argsort orders in an unspecified,
        build-dependent way -- are ordered as `np.argsort(scores, kind="stable")[::-1]` would: by DESCENDING row.  The same rule as
        librq_bm25.so (include/rq_bm25.h), so `search` and `search_batch` agree to the last bit."""
        pos = np.flatnonzero(scores > 0)
        if top_k <= 0 or pos.size == 0:
            return pos[:0]
        if pos.size > top_k:
            vals = scores[pos]
            kth = np.partition(vals, pos.size - top_k)[pos.size - top_k]
            pos = pos[vals >= kth]                     # every row tied with the k-th score takes part in the tie-break
        order = np.lexsort((-pos, -scores[pos]))
        return pos[order[:top_k]]

    SINGLE_NATIVE_AFTER: Optional[int] = 4   # one-query searches in a row over an unchanged corpus before they pay for the batch scorer's arrays (None: never)

    def _search_distinct(self, query: str, top_k: int, distinct_by: str, allowed_ids=None) -> List[Tuple[str, float]]:
        """`search` with one passage per value of the documents' `distinct_by` field (extension, the sparse side of a grouped search):
        collapsed on the host over `get_scores`, in the order of `_select_topk` -- score descending, exact ties by DESCENDING row --
        keeping the first passage of every value.  A document without the field, or with "", is a group of its own."""
        keep = None
        if allowed_ids is not None:
            keep = np.zeros(len(self.doc_ids), dtype=bool)
            keep[[r for r in (self._row_of_id().get(d) for d in allowed_ids) if r is not None]] = True
        rows, scores = self._distinct_rows(query, top_k, distinct_by, keep)
        return [(self.doc_ids[i], float(scores[i])) for i in rows]

    def _distinct_rows(self, query: str, top_k: int, distinct_by: str, keep: Optional[np.ndarray] = None) -> Tuple[List[int], np.ndarray]:
        """The walk of `_search_distinct` in row space: (the kept rows in order, the score vector); `keep`: the allowed rows as booleans."""
        scores = self.get_scores(self._tokenize(query))
        if keep is not None:
            scores = np.where(keep, scores, 0.0)
        pos = np.flatnonzero(scores > 0)
        out: List[int] = []
        seen = set()
        for i in pos[np.lexsort((-pos, -scores[pos]))].tolist():
            if len(out) >= top_k:
                break
            value = _group_value(self.documents[self.doc_ids[i]], distinct_by)
            if value is not None:
                if value in seen:
                    continue
                seen.add(value)
            out.append(i)
        return out, scores

    def search(self, query: str, top_k: int = 10, *, allowed_ids=None, distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[Tuple[str, float]]:
        if self.bm25 is None or not self.doc_ids:
            return []
        _refuse_per_group(per_group, "BM25Index.search")
        if distinct_by is not None:
            return self._search_distinct(query, top_k, distinct_by, allowed_ids)
        if allowed_ids is not None:
            # restricted to a set of ids (extension, the `where` of a Chroma query on the sparse side): the scores of every other
            # passage are masked to 0 before the reference's selection, which keeps positive scores only.  Unknown ids are ignored.
            scores = self.get_scores(self._tokenize(query))
            keep = np.zeros(len(scores), dtype=bool)
            rows = [r for r in (self._row_of_id().get(d) for d in allowed_ids) if r is not None]
            keep[rows] = True
            scores = np.where(keep, scores, 0.0)
            return [(self.doc_ids[i], float(scores[i])) for i in self._select_topk(scores, top_k).tolist()]
        # One query per call is the reference's evaluation loop (experiments/run_evaluation.py:157-206).  The path below allocates and
        # selects over one float64 per PASSAGE per query (20 ms at 1M passages); the batch scorer (librq_bm25.so) walks the same posting
        # lists in 3.4 ms -- same additions, same bits -- but needs the CSR form of the index, which every add invalidates (2.3 s to
        # rebuild at 1M passages).  So: through the batch scorer when its arrays are current, or once a few searches in a row have
        # seen the same corpus (an evaluation loop); a build loop that alternates adds and searches stays on this path.
        n = len(self.doc_ids)
        if top_k > 0 and self.SINGLE_NATIVE_AFTER is not None and _native.bm25_available():
            c = self.__dict__.get("_csr_cache")
            current = c is not None and c["n_docs"] == n
            if not current:
                streak = self.__dict__.get("_single_streak", (0, -1))
                streak = (streak[0] + 1, n) if streak[1] == n else (1, n)
                self.__dict__["_single_streak"] = streak
            if current or streak[0] > self.SINGLE_NATIVE_AFTER:
                return self.search_batch([query], top_k, n_threads=1)[0]
        scores = self.get_scores(self._tokenize(query))
        return [(self.doc_ids[i], float(scores[i])) for i in self._select_topk(scores, top_k).tolist()]

    # ---- a whole batch of queries at once (extension; configs[4]: 500 questions per call) ---------------------------------
    def _csr(self) -> Dict[str, Any]:
        """The inverted index as CSR arrays for the CURRENT corpus (rebuilt after an add: idf and avgdl change with every document):
        token ids in first-seen order, postings concatenated, and every posting's contribution idf * tf-saturation evaluated with
        the SAME float64 expression as _token_contribution -- the batch path then only adds them, in query-token order."""
        n_docs = len(self.doc_ids)
        c = self.__dict__.get("_csr_cache")
        if c is not None and c["n_docs"] == n_docs:
            return c
        if c is not None and c.get("handle") is not None:
            _native.bm25_destroy(c["handle"])
        if c is not None and c.get("sparse") is not None:
            c.pop("sparse").close()
        from itertools import chain
        idf = self._ensure_idf()
        avgdl = self._total_len / n_docs
        toks = list(self._post_rows)
        lens = np.fromiter((len(self._post_rows[t]) for t in toks), np.int64, len(toks))
        indptr = np.zeros(len(toks) + 1, np.int64)
        np.cumsum(lens, out=indptr[1:])
        nnz = int(indptr[-1])
        rows = np.fromiter(chain.from_iterable(self._post_rows.values()), np.int32, nnz)
        f = np.fromiter(chain.from_iterable(self._post_tf.values()), np.float64, nnz)
        w = np.repeat(np.fromiter(((idf.get(t) or 0) for t in toks), np.float64, len(toks)), lens)
        contrib = w * (f * (self.k1 + 1) / (f + self.k1 * (1 - self.b + self.b * self._np_doc_len()[rows] / avgdl)))
        c = {"n_docs": n_docs, "tid": {t: i for i, t in enumerate(toks)}, "indptr": indptr, "rows": rows, "contrib": contrib, "handle": None}
        if _native.bm25_available():
            c["handle"] = _native.bm25_create(indptr, rows, contrib, len(toks), n_docs)
        self.__dict__["_csr_cache"] = c
        return c

    def _sparse_index(self, c: Dict[str, Any]):
        """The device copy of the CSR arrays (`backend="gpu"`): built by the first search that wants it, dropped with the arrays it was
        built from (`_drop_csr`, an add).  Raises RqError without the library or a gfx950 device: there is no silent fallback."""
        if c.get("sparse") is None:
            c["sparse"] = _native.SparseIndex(c["indptr"], c["rows"], c["contrib"], len(c["tid"]), c["n_docs"], device=self.__dict__.get("sparse_device", 0))
        return c["sparse"]

    def _group_table(self, c: Dict[str, Any], key: str) -> np.ndarray:
        """One int32 per document for `distinct_by=key` (include/rq.h rq_sparse_set_groups): `_group_value` -> an id in first-seen order,
        -1 for a document that is a group of its own.  Cached per key with the CSR arrays, dropped with them on every add."""
        tables = c.setdefault("groups", {})
        if key not in tables:
            ids: Dict[Any, int] = {}
            docs = self.documents
            values = (_group_value(docs[d], key) for d in self.doc_ids)
            tables[key] = np.fromiter((_native.GROUP_NONE if v is None else ids.setdefault(v, len(ids)) for v in values), np.int32, len(self.doc_ids))
        return tables[key]

    def _sparse_index_grouped(self, c: Dict[str, Any], key: str):
        """`_sparse_index` with the group table of `key` on the device (it is sent when the key changes)."""
        sp = self._sparse_index(c)
        if c.get("sparse_group_key") != key:
            sp.set_groups(self._group_table(c, key))
            c["sparse_group_key"] = key
        return sp

    def _query_csr(self, c: Dict[str, Any], queries: Sequence[str]) -> Tuple[List[int], List[int]]:
        """The queries as token ids of `c` in query order, with repetition, tokens the corpus does not hold left out: (offsets [B + 1], ids)."""
        tid = c["tid"]
        q_tok: List[int] = []
        q_ptr = [0]
        for q in queries:
            for t in self._tokenize(q):
                j = tid.get(t)
                if j is not None:
                    q_tok.append(j)
            q_ptr.append(len(q_tok))
        return q_ptr, q_tok

    # ---- one allowed set per query (extension: the batch form of `search(..., allowed_ids=)`; include/rq.h rq_sparse_topk_masked) ----
    def make_mask(self, ids) -> SparseMask:
        """A reusable mask that restricts batch searches to the passages with these ids (`allowed_ids=` / `allowed_ids_each=` accept
        it as well as the ids themselves).  Ids map to rows through `_row_of_id()`, exactly as in `search`; unknown ids are ignored."""
        n = len(self.doc_ids)
        row_of = self._row_of_id()
        rows = sorted({r for r in (row_of.get(d) for d in ids) if r is not None})
        return SparseMask(_native.pack_row_mask(np.asarray(rows, np.int64), n), n, len(rows))

    def _mask_entries(self, n_queries: int, allowed_ids=None, allowed_ids_each=None) -> Optional[list]:
        """The two filter keywords of a batch call as one entry per query (ids, a `make_mask` result, or None), or None without either."""
        if allowed_ids_each is not None:
            return DenseIndex._each_entries(allowed_ids_each, n_queries, allowed_ids)
        return None if allowed_ids is None else [allowed_ids] * int(n_queries)

    def _mask_table(self, entries: list) -> Tuple[Optional[np.ndarray], np.ndarray]:
        """(masks uint32 [n_masks][words] or None, mask_of int32 [B]) of one batch: one mask per distinct entry OBJECT, -1 for None."""
        n = len(self.doc_ids)
        slot: Dict[int, int] = {}
        words: List[np.ndarray] = []
        mask_of = np.full(len(entries), -1, np.int32)
        for q, e in enumerate(entries):
            if e is None:
                continue
            if id(e) not in slot:
                m = e if isinstance(e, SparseMask) else self.make_mask(e)
                if m.n_docs != n:
                    raise _native.RqError(f"the sparse mask is stale: made over {m.n_docs} passages, the index holds {n}")
                slot[id(e)] = len(words)
                words.append(m.words)
            mask_of[q] = slot[id(e)]
        return (np.stack(words) if words else None), mask_of

    def search_batch_rows(self, queries: Sequence[str], top_k: int = 10, *, n_threads: int = 0, use_native: Optional[bool] = None,
                          backend: str = "host", allowed_ids=None, allowed_ids_each=None, distinct_by: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The selection of `search` for a whole batch, in ROW space: (rows int32 [B][top_k], -1 padded; scores float64 [B][top_k]).
        librq_bm25.so (include/rq_bm25.h) walks the posting lists of every query on the host cores -- term at a time, one float64
        accumulator per thread, the contributions added in query order (the same additions as get_scores: identical bits), top-k by a
        heap with the tie rule of _select_topk.  Without the library (`use_native=False`, or it is not built) the same arrays are
        scored with numpy, one query at a time.
        `backend`: "host" (default) is the path above; "gpu" scores and selects on the device (include/rq.h rq_sparse_topk, a
        `_native.SparseIndex` over the same arrays: the same rows and the same score bits; top_k <= 1024, at most 65 535 queries;
        RqError without a device); "auto" takes the device when one is visible and the host otherwise.
        `allowed_ids` (ids or a `make_mask` result: one set for the whole batch) and `allowed_ids_each` (one such entry, or None for
        an unrestricted query, per query; entries that are the same object become one mask): query q is answered as
        `search(q, top_k, allowed_ids=entry)` answers it -- scored as ever, every passage outside its set then scores 0.0 before the
        selection -- under every backend and on the numpy branch (rq_bm25_topk_masked, rq_sparse_topk_masked).  The two do not combine.
        `distinct_by` (a metadata key such as "title"): one passage per value of that field, query q answered as
        `search(q, top_k, distinct_by=key, allowed_ids=entry)` answers it (`_search_distinct`); it combines with either filter keyword.
        "gpu" collapses on the device (rq_sparse_topk_grouped over a group table built from `_group_value`, cached per key); "host" is the
        loop of `_search_distinct` itself -- no host-core grouped scorer exists, `n_threads` and `use_native` do not apply to it."""
        if backend not in ("host", "gpu", "auto"):
            raise ValueError(f"backend must be 'host', 'gpu' or 'auto', not {backend!r}")
        B, k = len(queries), max(int(top_k), 1)
        entries = self._mask_entries(B, allowed_ids, allowed_ids_each)
        if self.bm25 is None or not self.doc_ids or top_k <= 0 or B == 0:
            return np.full((B, k), -1, np.int32), np.zeros((B, k))
        masked = {}
        if entries is not None:
            masks, mask_of = self._mask_table(entries)
            masked = {"masks": masks, "mask_of": mask_of}
        on_device = backend == "gpu" or (backend == "auto" and _native.sparse_available())
        if distinct_by is not None and not on_device:
            n = len(self.doc_ids)
            keep = [] if not masked or masks is None else [np.unpackbits(m.view(np.uint8), bitorder="little")[:n].astype(bool) for m in masks]
            out_rows, out_scores = np.full((B, k), -1, np.int32), np.zeros((B, k))
            for b, q in enumerate(queries):
                sel, scores = self._distinct_rows(q, k, distinct_by, keep[mask_of[b]] if masked and mask_of[b] >= 0 else None)
                out_rows[b, :len(sel)] = sel
                out_scores[b, :len(sel)] = scores[sel]
            return out_rows, out_scores
        c = self._csr()
        q_ptr, q_tok = self._query_csr(c, queries)
        if on_device and distinct_by is not None:
            return self._sparse_index_grouped(c, distinct_by).topk_grouped(np.asarray(q_ptr, np.int64), np.asarray(q_tok, np.int32), B, k, **masked)[:2]
        if on_device:
            return self._sparse_index(c).topk(np.asarray(q_ptr, np.int64), np.asarray(q_tok, np.int32), B, k, **masked)
        if use_native and c["handle"] is None:
            raise _native.RqError("librq_bm25.so is not built: `make -C csrc` (or use_native=False for the numpy path)")
        native = c["handle"] is not None if use_native is None else (use_native and c["handle"] is not None)
        if native:
            return _native.bm25_topk(c["handle"], np.asarray(q_ptr, np.int64), np.asarray(q_tok, np.int32), B, k, n_threads, **masked)
        indptr, rows, contrib = c["indptr"], c["rows"], c["contrib"]
        out_rows, out_scores = np.full((B, k), -1, np.int32), np.zeros((B, k))
        n = len(self.doc_ids)
        keep = [] if not masked or masks is None else [np.unpackbits(m.view(np.uint8), bitorder="little")[:n].astype(bool) for m in masks]
        for b in range(B):
            scores = np.zeros(len(self.doc_ids))
            for j in q_tok[q_ptr[b]: q_ptr[b + 1]]:
                lo, hi = indptr[j], indptr[j + 1]
                scores[rows[lo:hi]] += contrib[lo:hi]
            if masked and mask_of[b] >= 0:
                scores = np.where(keep[mask_of[b]], scores, 0.0)
            sel = self._select_topk(scores, k)
            out_rows[b, :len(sel)] = sel
            out_scores[b, :len(sel)] = scores[sel]
        return out_rows, out_scores

    def _ids_array(self) -> np.ndarray:
        cache = self.__dict__.get("_ids_np")
        if cache is None or len(cache) != len(self.doc_ids):
            cache = np.empty(len(self.doc_ids), dtype=object)
            cache[:] = self.doc_ids
            self.__dict__["_ids_np"] = cache
        return cache

    def search_batch(self, queries: Sequence[str], top_k: int = 10, *, n_threads: int = 0, use_native: Optional[bool] = None,
                     backend: str = "host", allowed_ids=None, allowed_ids_each=None, distinct_by: Optional[str] = None) -> List[List[Tuple[str, float]]]:
        """`[self.search(q, top_k) for q in queries]`, scored as one job (search_batch_rows; `backend` as there).  With `allowed_ids`
        (one set for the batch) or `allowed_ids_each` (one entry per query, None = unrestricted), as there:
        `[self.search(q, top_k, allowed_ids=entry_q) for q in queries]`; with `distinct_by`, as there: one passage per value of that
        field, `[self.search(q, top_k, distinct_by=key, allowed_ids=entry_q) for q in queries]`."""
        given = _given(allowed_ids=allowed_ids, allowed_ids_each=allowed_ids_each, distinct_by=distinct_by)
        if self.bm25 is None or not self.doc_ids or top_k <= 0:
            self._mask_entries(len(queries), allowed_ids, allowed_ids_each)      # (the keywords are still checked)
            return [[] for _ in queries]
        out_rows, out_scores = self.search_batch_rows(queries, top_k, n_threads=n_threads, use_native=use_native, backend=backend, **given)
        idl = self._ids_array()[np.where(out_rows >= 0, out_rows, 0)].tolist()
        scl = out_scores.tolist()
        have = (out_rows >= 0).sum(axis=1).tolist()
        return [list(zip(idl[b][:have[b]], scl[b][:have[b]])) for b in range(len(have))]

    def _drop_csr(self) -> None:
        c = self.__dict__.pop("_csr_cache", None)
        if c is not None and c.get("handle") is not None:
            _native.bm25_destroy(c["handle"])
        if c is not None and c.get("sparse") is not None:
            c.pop("sparse").close()

    def __del__(self):
        try:
            self._drop_csr()
        except Exception:
            pass

    def get_document(self, doc_id: str) -> Optional[Document]:
        return self.documents.get(doc_id)

    # ---- persistence: append-only log + occasional snapshot in the reference's pickle layout ----------------
    def _log_path(self) -> Path:
        return Path(str(self.persist_path) + ".log.jsonl")

    def _persist_new(self, first_new: int) -> None:
        n = len(self.doc_ids)
        logged = n - self._snapshot_docs
        every = self.snapshot_every
        if (every is not None and logged >= every) or (every is None and logged >= max(self.SNAPSHOT_MIN_DOCS, self._snapshot_docs)):
            self._save()
            return
        if self._log_file is None:
            self.persist_path.parent.mkdir(parents=True, exist_ok=True)
            self._log_file = open(self._log_path(), "a")
        for i in range(first_new, n):
            self._log_file.write(json.dumps(self.documents[self.doc_ids[i]].to_dict()) + "\n")
        self._log_file.flush()

    def _save(self):
        """Snapshot in the reference's layout (:189-201), written atomically; the log restarts empty."""
        if self.persist_path is None:
            return
        self.persist_path.parent.mkdir(parents=True, exist_ok=True)
        data = {
            "documents": {k: v.to_dict() for k, v in self.documents.items()},
            "doc_ids": self.doc_ids,
            "tokenized_corpus": self.tokenized_corpus,
            "k1": self.k1,
            "b": self.b,
        }
        _atomic_write(self.persist_path, pickle.dumps(data))
        self._snapshot_docs = len(self.doc_ids)
        if self._log_file is not None:
            self._log_file.close()
            self._log_file = None
        if self._log_path().exists():
            self._log_path().unlink()

    def save(self) -> None:
        self._save()

    def close(self) -> None:
        if self.persist_path is not None and len(self.doc_ids) != self._snapshot_docs:
            self._save()
        if self._log_file is not None:
            self._log_file.close()
            self._log_file = None

    def _load(self):
        if self.persist_path is None:
            return
        if self.persist_path.exists():
            data = _load_plain_pickle(self.persist_path)   # plain containers only: no class is ever resolved
            self.documents = {k: Document.from_dict(v) for k, v in data["documents"].items()}
            self.doc_ids = data["doc_ids"]
            self.tokenized_corpus = data["tokenized_corpus"]
            self.k1 = data["k1"]
            self.b = data["b"]
        self._post_rows, self._post_tf, self._doc_len, self._total_len = {}, {}, [], 0
        self.__dict__.pop("_post_np", None)              # numpy views of the posting lists (get_scores): rebuilt on demand
        self.__dict__.pop("_doc_len_np", None)
        self.__dict__.pop("_contrib", None)
        self._drop_csr()
        for row, toks in enumerate(self.tokenized_corpus):
            self._index_tokens(row, toks)
        self._snapshot_docs = len(self.doc_ids)
        if self._log_path().exists():                      # documents added since the snapshot
            # Replay stops at the first line that is not a complete record (a torn tail: the process died inside a write).  The
            # torn bytes must not stay in the file: the next add reopens the log in append mode, its first record would be glued
            # onto them, and every document acknowledged from then on would be unreadable at the following load.  So the log
            # is cut back to the end of the last good record (and a record that lost only its newline gets it back).
            good_end, needs_newline = 0, False
            with open(self._log_path(), "rb") as f:
                for raw in f:
                    try:
                        doc = Document.from_dict(json.loads(raw.decode("utf-8")))
                    except (json.JSONDecodeError, UnicodeDecodeError, KeyError, TypeError, AttributeError):
                        break
                    good_end += len(raw)
                    needs_newline = not raw.endswith(b"\n")
                    if doc.id in self.documents:
                        continue
                    self.documents[doc.id] = doc
                    self.doc_ids.append(doc.id)
                    toks = self._tokenize(doc.text)
                    self.tokenized_corpus.append(toks)
                    self._index_tokens(len(self.doc_ids) - 1, toks)
            if good_end != self._log_path().stat().st_size or needs_newline:
                logger.warning(f"BM25 log {self._log_path()}: dropping a torn tail after {good_end} bytes")
                with open(self._log_path(), "r+b") as f:
                    f.truncate(good_end)
                    if needs_newline:
                        f.seek(0, os.SEEK_END)
                        f.write(b"\n")
        logger.info(f"Loaded BM25 index with {len(self.doc_ids)} documents")

    def __len__(self) -> int:
        return len(self.doc_ids)


# =============================================================================================
# dense side (reference :228-373) -- the hot path
# =============================================================================================
def _read_meta(meta_path: Path) -> Optional[Dict[str, int]]:
    """<collection>.meta: 'rq-index 1 / dim D / rows N / dtype f16' (what rq_load parses) + an optional 'docs_bytes B' line."""
    if not meta_path.exists():
        return None
    kv = dict(line.split(None, 1) for line in meta_path.read_text().splitlines() if " " in line)
    if kv.get("rq-index", "").strip() != "1" or kv.get("dtype", "").strip() != "f16":
        raise RuntimeError(f"{meta_path} is not an rq-index v1 meta file")
    out = {"dim": int(kv["dim"]), "rows": int(kv["rows"])}
    if "docs_bytes" in kv:
        out["docs_bytes"] = int(kv["docs_bytes"])
    return out


def repair_persisted_collection(base: Path, docs_path: Path, truncate: bool = True) -> Optional[Dict[str, int]]:
    """Bring the three files of a persisted collection back to the last COMMITTED state.

    An add appends rows to <base>.f16, records to <docs_path>, and only then replaces <base>.meta (the commit point,
    written atomically).  A process killed in between leaves data files LONGER than the meta says; they are cut back
    here, so that the collection reopens with exactly the committed rows (Chroma's PersistentClient, which the reference
    uses at :257, is transactional on add).  Data files SHORTER than the commit are real corruption and raise.
    `truncate=False` only READS the commit (what a process that merely opens the collection does: bytes beyond the commit may
    belong to a writer that sits between appending its data and replacing the meta -- cutting them off would leave that
    writer's next meta describing more bytes than exist); the writer path truncates before it appends.
    Returns {'dim', 'rows', 'docs_bytes'} or None when nothing was ever committed."""
    meta = _read_meta(Path(str(base) + ".meta"))
    if meta is None:
        return None
    f16_path = Path(str(base) + ".f16")
    want = meta["rows"] * meta["dim"] * 2
    have = f16_path.stat().st_size if f16_path.exists() else 0
    if have < want:
        raise RuntimeError(f"persisted index is inconsistent: {f16_path} holds {have} bytes, the commit record needs {want}")
    if have > want and truncate:
        with open(f16_path, "r+b") as f:
            f.truncate(want)
    docs_have = docs_path.stat().st_size if docs_path.exists() else 0
    if "docs_bytes" in meta:
        docs_want = meta["docs_bytes"]
    else:                                   # a meta written by rq_save alone: the commit is the first `rows` lines
        docs_want, seen = 0, 0
        if docs_path.exists():
            with open(docs_path, "rb") as f:
                for line in f:
                    if seen == meta["rows"] or not line.endswith(b"\n"):
                        break
                    docs_want += len(line)
                    seen += 1
        if seen < meta["rows"]:
            raise RuntimeError(f"persisted index is inconsistent: {seen} ids vs {meta['rows']} rows")
    if docs_have < docs_want:
        raise RuntimeError(f"persisted index is inconsistent: {docs_path} holds {docs_have} bytes, the commit record needs {docs_want}")
    if docs_have > docs_want and truncate:
        with open(docs_path, "r+b") as f:
            f.truncate(docs_want)
    meta["docs_bytes"] = docs_want
    return meta

class DenseIndex:
    """Exact cosine top-k over fp16 passage vectors resident in MI355X HBM.

    Signature and defaults follow reference :236-243.  `chroma_host` / `chroma_port` are accepted for
    call compatibility and ignored (there is no service).  Keyword-only extras: `embedder`, `device`,
    `metric`, `backend_options`.  Construction raises when the GPU backend is unavailable, as the reference raises
    ImportError without chromadb (:248-249).
    """

    def __init__(self, collection_name: str = "rag_documents", persist_directory: str = "./data/chroma_db",
                 embedding_model: str = "nomic-embed-text", chroma_host: Optional[str] = None, chroma_port: int = 8000,
                 *, embedder=None, device: int = 0, devices: Optional[Sequence[int]] = None, metric: str = "cosine",
                 load_persisted: bool = True, auto_persist: bool = True, backend_options: Optional[Dict[str, float]] = None):
        self.collection_name = collection_name
        # options of the C library (include/rq.h rq_set_option), applied when the index is created or loaded -- e.g.
        # {"scan8": 0} keeps the fp16 rows as the only copy of the corpus in HBM (no int8 image for the scan)
        self.backend_options = dict(backend_options or {})
        self.persist_directory = persist_directory
        self.embedding_model = embedding_model
        if chroma_host:
            logger.info("chroma_host=%s ignored: the dense index is in-process on GPU %d", chroma_host, device)
        if not _gpu_backend_available():
            raise ImportError("a gfx950 GPU (librq_hip.so backend) is required for DenseIndex")
        self.embedder = embedder if embedder is not None else default_embedder(embedding_model)
        self.device = int(device)
        self.devices = [int(d) for d in devices] if devices else None     # several GPUs in this process: rows are sharded
        self.metric = _native.METRIC_IP if metric in ("ip", "inner_product") else _native.METRIC_COSINE
        self.auto_persist = bool(auto_persist) and bool(persist_directory)   # Chroma's PersistentClient is durable on add (:257)
        self.dim: Optional[int] = None
        self._index: Optional[_native.NativeIndex] = None
        self._ids: List[str] = []
        self._row_of: Dict[str, int] = {}
        self._texts: List[str] = []
        self._metas: List[Dict[str, Any]] = []
        if load_persisted and persist_directory and self._files()[0].exists():
            self._load()
        logger.info(f"Initialized DenseIndex with collection '{collection_name}'")

    # ---- embedding (reference :267-288) -----------------------------------------------------------
    def _zero(self) -> List[float]:
        return [0.0] * (self.dim or getattr(self.embedder, "dim", 768) or 768)

    def _get_embedding(self, text: str) -> List[float]:
        try:
            return [float(v) for v in self.embedder.embed([text])[0]]
        except Exception as e:   # reference :281-284: log, zero vector
            logger.error(f"Embedding failed: {e}")
            return self._zero()

    def _get_embeddings_batch(self, texts: List[str]) -> List[List[float]]:
        return self._embed_matrix(texts).tolist()

    def _embed_matrix(self, texts: Sequence[str]) -> np.ndarray:
        """One embedder call for the whole batch; on failure fall back to per-text calls so a bad text
        degrades to a zero row instead of failing its neighbours."""
        if not texts:
            return np.zeros((0, self.dim or getattr(self.embedder, "dim", 768)), np.float32)
        try:
            v = np.asarray(self.embedder.embed(list(texts)), dtype=np.float32)
            if v.ndim == 2 and v.shape[0] == len(texts):
                return v
            raise ValueError(f"embedder returned shape {v.shape}")
        except Exception as e:
            logger.error(f"Batch embedding failed ({e}); retrying one text at a time")
            return np.asarray([self._get_embedding(t) for t in texts], dtype=np.float32)

    # ---- build (reference :290-336) -----------------------------------------------------------------
    def _ensure_index(self, dim: int) -> None:
        if self._index is None:
            self.dim = int(dim)
            if self.devices and len(self.devices) > 1:
                from .distributed import MultiDeviceIndex
                self._index = MultiDeviceIndex(self.dim, self.devices)
            else:
                self._index = _native.NativeIndex(self.dim, self.devices[0] if self.devices else self.device)
            self._apply_backend_options()
        elif dim != self.dim:
            raise ValueError(f"embedding dimension {dim} does not match the index ({self.dim})")

    def _apply_backend_options(self) -> None:
        for name, value in self.backend_options.items():
            # the stripe layout of a multi-device index and the stored row length are fixed by the first rows (a persisted collection
            # comes back with the row length of the library's rule, include/rq.h "row_pad")
            if name in ("stripe_rows", "row_pad") and len(self._index):
                continue
            self._index.set_option(name, float(value))

    def add_documents(self, documents: List[Document], batch_size: int = 100) -> int:
        # the reference fetches every stored id per call (:306); a hash table does the same filter
        seen = set()
        new_docs = []
        for d in documents:
            if d.id in self._row_of or d.id in seen:
                continue
            seen.add(d.id)
            new_docs.append(d)
        if not new_docs:
            logger.info("No new documents to add")
            return 0
        total_added = 0
        for i in range(0, len(new_docs), batch_size):
            batch = new_docs[i:i + batch_size]
            vecs = self._embed_matrix([d.text for d in batch])
            self.add_vectors([d.id for d in batch], vecs, [d.text for d in batch],
                             [{"title": d.title or "", **(d.metadata or {})} for d in batch])
            total_added += len(batch)
            logger.info(f"Indexed batch {i // batch_size + 1}, total: {total_added}/{len(new_docs)}")
        return total_added

    def add_vectors(self, ids: Sequence[str], vectors: np.ndarray, texts: Optional[Sequence[str]] = None,
                    metadatas: Optional[Sequence[Dict[str, Any]]] = None) -> int:
        """Append pre-computed embeddings (the `collection.add(embeddings=...)` of reference :326-331)."""
        vectors = np.asarray(vectors, dtype=np.float32)
        if vectors.ndim != 2 or vectors.shape[0] != len(ids):
            raise ValueError("vectors must be [len(ids), dim]")
        self._ensure_index(vectors.shape[1])
        # cosine index: rows are unit-normalised before fp16 rounding (cosine is invariant, fp16 range is safe)
        self._index.add_f32(vectors, normalize=self.metric == _native.METRIC_COSINE)
        first_new = len(self._ids)
        for j, doc_id in enumerate(ids):
            self._row_of[doc_id] = len(self._ids)
            self._ids.append(doc_id)
            self._texts.append(texts[j] if texts is not None else "")
            self._metas.append(dict(metadatas[j]) if metadatas is not None else {})
        if self.auto_persist and hasattr(self._index, "get_rows_f16"):
            self._persist_append(first_new)
        return len(ids)

    def _persist_append(self, first_new: int) -> None:
        """Append the rows [first_new, len) to the rq_save layout (<collection>.f16 / .meta) and their records to
        <collection>.docs.jsonl, so that a later process finds the index (reference: Chroma persists on add).
        Order: data files first, then the meta file replaces the old one atomically -- the commit point.  Whatever an
        interrupted earlier add left behind the commit is cut off before appending (repair_persisted_collection)."""
        docs_path, base = self._files()
        docs_path.parent.mkdir(parents=True, exist_ok=True)
        n = len(self._ids)
        f16_path, meta_path = Path(str(base) + ".f16"), Path(str(base) + ".meta")
        committed = repair_persisted_collection(base, docs_path) if first_new else None
        if committed is None or committed["rows"] != first_new or committed["dim"] != self.dim:
            first_new = 0                         # nothing usable on disk: (re)write from scratch
            docs_bytes = 0
            if meta_path.exists():                # ... and say so first: an old commit over half-rewritten files could never be reopened
                meta_path.unlink()
        else:
            docs_bytes = committed["docs_bytes"]
        rows = self._index.get_rows_f16(first_new, n - first_new)
        with open(f16_path, "ab" if first_new else "wb") as f:
            f.write(np.ascontiguousarray(rows).view(np.uint16).tobytes())
        with open(docs_path, "ab" if first_new else "wb") as f:
            for i in range(first_new, n):
                line = (json.dumps({"id": self._ids[i], "text": self._texts[i], "metadata": self._metas[i]}) + "\n").encode()
                f.write(line)
                docs_bytes += len(line)
        _atomic_write(meta_path, f"rq-index 1\ndim {self.dim}\nrows {n}\ndtype f16\ndocs_bytes {docs_bytes}\n".encode())

    # ---- query (reference :338-370) -------------------------------------------------------------------
    @classmethod
    def from_native(cls, index: "_native.NativeIndex", ids: Sequence[str], texts: Optional[Sequence[str]] = None, *,
                    embedder=None, metric: str = "cosine") -> "DenseIndex":
        """Wrap a shard that already sits in HBM (built through the C ABI / `add_f16_device`) as a DenseIndex: row i of `index`
        answers as `ids[i]`.  Nothing is persisted (extension; the reference has no counterpart)."""
        if len(ids) != len(index):
            raise ValueError(f"{len(ids)} ids for {len(index)} rows")
        self = cls.__new__(cls)
        self.collection_name, self.persist_directory, self.embedding_model = "rag_documents", "", "nomic-embed-text"
        self.backend_options = {}
        self.embedder = embedder if embedder is not None else default_embedder(self.embedding_model)
        self.device, self.devices = index.device, None
        self.metric = _native.METRIC_IP if metric in ("ip", "inner_product") else _native.METRIC_COSINE
        self.auto_persist = False
        self.dim = index.dim
        self._index = index
        self._ids = list(ids)
        self._row_of = {d: i for i, d in enumerate(self._ids)}
        self._texts = list(texts) if texts is not None else [""] * len(self._ids)
        self._metas = [{} for _ in self._ids] if len(self._ids) < 100_000 else [{}] * len(self._ids)
        return self

    def _id_text_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        """object arrays of the ids / texts (one fancy-index gather per search instead of a Python loop over B * k results)"""
        cache = self.__dict__.get("_idtext_np")
        if cache is None or len(cache[0]) != len(self._ids):
            ids = np.empty(len(self._ids), dtype=object)
            ids[:] = self._ids
            texts = None                       # a collection that stores no passage text (add_vectors without texts): nothing to gather
            if any(self._texts):
                texts = np.empty(len(self._texts), dtype=object)
                texts[:] = self._texts
            cache = self.__dict__["_idtext_np"] = (ids, texts)
        return cache

    def _assemble(self, scores: np.ndarray, rows: np.ndarray) -> List[List[Tuple[str, float, str]]]:
        """(scores [B][k], rows [B][k], -1 padded) -> the reference's result lists (:361-368): (doc_id, float(score), text), best first"""
        ids, texts = self._id_text_arrays()
        ok = rows >= 0
        all_ok = bool(ok.all())
        safe = rows if all_ok else np.where(ok, rows, 0)
        # B * k tuples + B lists of (str, float, str): nothing here can form a cycle, but every 700th container allocation starts a
        # young-generation collection -- 40 % of this function at 256 x 10 (370 -> 220 us on the build container) -- so the collector
        # is paused for these few lines
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            idl, scl = ids[safe].tolist(), scores.astype(np.float64).tolist()
            txl = texts[safe].tolist() if texts is not None else [[""] * rows.shape[1]] * rows.shape[0]
            if all_ok:
                return [list(zip(i, s, t)) for i, s, t in zip(idl, scl, txl)]
            okl = ok.tolist()
            return [[(i, s, t) for i, s, t, v in zip(ib, sb, tb, vb) if v] for ib, sb, tb, vb in zip(idl, scl, txl, okl)]
        finally:
            if gc_was_on:
                gc.enable()

    # ---- the parts every request below is put together from ----------------------------------------------------------------
    # What a call needs of the index: (the method, whether an index over several devices is refused here too, the refusal).  Two
    # idioms, kept apart on purpose.  The first four probe the method alone, and an index that does not exist yet is refused as well:
    # an index over several devices has every method, and it is the library that refuses it.  Range and scoring also refuse
    # several devices, and let a missing index pass (they answer "nothing" for it).  "device" refuses nobody: the host route answers.
    _NEEDS = {
        "filter": ("make_filter", False, "filtered searches need a single-device index that holds rows"),
        "groups": ("set_groups", False, "grouped searches need a single-device index"),
        "members": ("search_group_members", False, "grouped searches need a single-device index"),
        "mmr": ("search_mmr", False, "MMR searches need a single-device index"),
        "range": ("search_range", True, "search_threshold / count_above need a single-device index"),
        "scoring": ("score_rows", True, "score_vectors / score_rows_batch / score_ids need a single-device index"),
        "device": ("search_device", True, None),
    }

    def _can(self, what: str) -> bool:
        method, one_device, _ = self._NEEDS[what]
        return hasattr(self._index, method) and not (one_device and len(getattr(self._index, "devices", [0])) > 1)

    def _require(self, what: str):
        """The index, after refusing the call if the index cannot serve it (`_NEEDS`)."""
        if not self._can(what) and not (self._index is None and self._NEEDS[what][1]):
            raise _native.RqError(self._NEEDS[what][2])
        return self._index

    def _k(self, top_k, limit: int = _native.MAX_K) -> int:
        """top_k as the k of a native call: no more than the index holds, nor than the library takes"""
        return min(int(top_k), len(self._ids), limit)

    def _nothing_to_search(self, top_k=1, n_queries: int = 1) -> bool:
        return self._index is None or len(self._ids) == 0 or top_k <= 0 or n_queries == 0

    @staticmethod
    def _no_passages(n_queries: int) -> List[List[Tuple[str, float, str]]]:
        return [[] for _ in range(n_queries)]

    @staticmethod
    def _no_rows(n_queries: int) -> Tuple[np.ndarray, np.ndarray]:
        return np.zeros((n_queries, 0), np.float32), np.zeros((n_queries, 0), np.int64)

    @staticmethod
    def _query_matrix(vectors) -> np.ndarray:
        """Query vectors as a float32 matrix [B][dim] (one query may come as a vector); a float32 matrix is passed through as it is."""
        v = np.asarray(vectors, dtype=np.float32)
        return v if v.ndim == 2 else np.atleast_2d(v)

    def _check_dim(self, dim: int) -> None:
        if dim != self.dim:
            raise ValueError(f"query dimension {dim} does not match the index ({self.dim})")

    def _embed_device(self, queries: Sequence[str]):
        """The queries as a tensor in HBM -- from an embedder that can leave them there, for an index that holds rows -- or None:
        the host path (`_embed_matrix`) then embeds them, after the reason was logged if the embedder failed."""
        if not hasattr(self.embedder, "embed_device") or self._index is None or not len(self._ids):
            return None
        try:
            return self.embedder.embed_device(list(queries))
        except Exception as e:     # reference :281-284 semantics live in _embed_matrix (per-text retry, zero vector)
            logger.error(f"Device embedding failed ({e}); falling back to the host path")
            return None

    # ---- filtered searches (extension: the `where` of reference :355-359's collection.query) -------------------------
    def make_filter(self, ids) -> "_native.RowFilter":
        """A reusable filter that restricts searches to the passages with these ids (`allowed_ids=` accepts it as well as the ids
        themselves).  Unknown ids are ignored.  It describes the collection as it is now: adding documents makes it stale."""
        index = self._require("filter")
        rows = [r for r in (self._row_of.get(d) for d in ids) if r is not None]
        return index.make_filter(np.asarray(rows, dtype=np.int64))

    def _with_filters(self, entries, call):
        """`call(filters)` with every entry as the native calls take it: None (unrestricted) and a caller's own filter pass through untouched;
        ids become a filter made now and closed behind the call (`_with_made_filters`) -- a filter's whole set-up and tear-down per call (O(rows)
        on the host, two device allocations, the masked scale, a device synchronisation): reuse a `make_filter` result for repeated questions."""
        return _with_made_filters(entries, lambda e: e is None or isinstance(e, _native.RowFilter), self.make_filter, call)

    def _with_filter(self, allowed_ids, call):
        """`call(row_filter)` for one `allowed_ids`; free when there is no filter to make."""
        if allowed_ids is None or isinstance(allowed_ids, _native.RowFilter):
            return call(allowed_ids)
        return self._with_filters([allowed_ids], lambda filters: call(filters[0]))

    @staticmethod
    def _each_entries(allowed_ids_each, n_queries: int, allowed_ids=None, distinct_by=None, per_group=None) -> list:
        """`allowed_ids_each=` as a checked list: one entry per query (a `make_filter` result, an iterable of ids, or None for an
        unrestricted query); it does not combine with `allowed_ids`, `distinct_by` or `per_group`."""
        if allowed_ids is not None or distinct_by is not None or per_group is not None:
            raise ValueError("allowed_ids_each does not combine with allowed_ids, distinct_by or per_group")
        entries = list(allowed_ids_each)
        if len(entries) != int(n_queries):
            raise ValueError(f"allowed_ids_each needs one entry per query: {n_queries} queries, {len(entries)} entries")
        return entries

    # ---- grouped searches (extension: `distinct_by=` -- one passage per value of a metadata field, e.g. "title": the best passage
    # of each of the top_k articles of a chunked corpus; include/rq.h "grouped searches") --------------------------------------
    def _push_groups(self, key: str) -> None:
        """Group ids of the rows the index has not been told about yet: metadata value -> id, assigned lazily in row order; a row
        whose metadata lacks `key`, or holds "", is a group of its own.  Another key than the last call's re-pushes every row."""
        index = self._require("groups")
        st = self.__dict__.get("_group_state")
        if st is None or st["key"] != key or st["pushed"] > len(self._ids):
            st = self.__dict__["_group_state"] = {"key": key, "ids": {}, "pushed": 0}
        first, n = st["pushed"], len(self._ids)
        if first == n:
            return
        table = st["ids"]
        groups = np.full(n - first, _native.GROUP_NONE, dtype=np.int32)
        for j in range(first, n):
            value = _meta_group_value(self._metas[j], key)
            if value is not None:
                groups[j - first] = table.setdefault(value, len(table))
        index.set_groups(groups, first)
        st["pushed"] = n

    def _group_member_rows(self, vectors: np.ndarray, top_k: int, distinct_by: str, per_group: int, allowed_ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """(scores, rows), each [B][k x per_group]: the best per_group passages of each of the top_k groups, group by group, members
        best first; entries a group does not fill, and groups beyond those in play, are (0.0, -1) (include/rq.h "group members").
        top_k is clamped so that k x per_group <= MAX_K."""
        if per_group > _native.MAX_K:
            raise ValueError(f"per_group {per_group} beyond {_native.MAX_K}")
        index = self._require("members")
        self._push_groups(distinct_by)
        k = self._k(top_k, _native.MAX_K // per_group)
        scores, rows = self._with_filter(allowed_ids, lambda flt: index.search_group_members(vectors, k, per_group, self.metric, row_filter=flt)[:2])
        B = rows.shape[0]
        return scores.reshape(B, k * per_group), rows.reshape(B, k * per_group)

    # ---- the one choice of route: every search that ranks passages ends here -------------------------------------------------
    def _search_rows(self, vectors, top_k: int, allowed_ids=None, distinct_by: Optional[str] = None, per: int = 1, each: Optional[list] = None, *,
                     on_device: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(scores float32, rows int64, (0.0, -1) padded) of one batch of query vectors by the first route that applies:
          each         query q over the passages of each[q] only, all in ONE native call (include/rq.h "per-query filters")
          per > 1      the best `per` passages of each of the top_k groups: [B][k x per] (`_group_member_rows`)
          distinct_by  the best passage of each of the top_k groups, best group first
          allowed_ids  the top_k of the allowed passages only
          on_device    `vectors` is a tensor in HBM and is searched there (`_search_device_rows`); no restricted route takes one
          otherwise    the plain search: host matrix in, k = min(top_k, rows of the index, MAX_K).
        The caller has answered "nothing to search" and validated its keywords (`_per_group_size`, `_each_entries`)."""
        index, metric = self._index, self.metric
        if each is not None:
            return self._with_filters(each, lambda filters: index.search_filtered_each(vectors, self._k(top_k), filters, metric))
        if per > 1:
            return self._group_member_rows(vectors, top_k, distinct_by, per, allowed_ids)
        if distinct_by is not None:
            self._push_groups(distinct_by)
            return self._with_filter(allowed_ids, lambda flt: index.search_grouped(vectors, self._k(top_k), metric, row_filter=flt)[:2])
        if allowed_ids is not None:
            return self._with_filter(allowed_ids, lambda flt: index.search(vectors, self._k(top_k), metric, row_filter=flt))
        if on_device:
            return self._search_device_rows(vectors, top_k)
        return index.search(vectors, self._k(top_k), metric)

    def search_vectors(self, vectors: np.ndarray, top_k: int = 10, *, allowed_ids=None, distinct_by: Optional[str] = None,
                       per_group: Optional[int] = None, allowed_ids_each=None) -> List[List[Tuple[str, float, str]]]:
        """`allowed_ids_each` (keyword-only): one entry per query -- a `make_filter` result, an iterable of ids, or None -- each
        query ranked over its own passages, the whole batch in one native call."""
        per = _per_group_size(distinct_by, per_group)
        vectors = self._query_matrix(vectors)
        each = None if allowed_ids_each is None else self._each_entries(allowed_ids_each, vectors.shape[0], allowed_ids, distinct_by, per_group)
        if self._nothing_to_search(top_k):
            return self._no_passages(vectors.shape[0])
        self._check_dim(vectors.shape[1])
        return self._assemble(*self._search_rows(vectors, top_k, allowed_ids, distinct_by, per, each))

    # ---- diversified searches (extension: what LangChain's max_marginal_relevance_search does on the host with the fetch_k
    # embeddings of reference :355-359's collection.query) -----------------------------------------------------------------
    def search_mmr_vectors(self, vectors: np.ndarray, top_k: int = 10, fetch_k: int = 50, lambda_mult: float = 0.5, *,
                           allowed_ids=None) -> List[List[Tuple[str, float, str]]]:
        """`search_vectors` with the top_k chosen among the exact top fetch_k by greedy maximal marginal relevance (include/rq.h
        rq_search_mmr): (doc_id, score, text) in SELECTION order, the score still the cosine.  lambda_mult = 1 is the plain search,
        0 looks at diversity alone.  fetch_k is clamped to [top_k, min(len(self), MAX_K)].  The queries take the host path."""
        vectors = self._query_matrix(vectors)
        if not 0.0 <= float(lambda_mult) <= 1.0:
            raise ValueError(f"lambda_mult must lie within [0, 1], got {lambda_mult!r}")
        if self._nothing_to_search(top_k):
            return self._no_passages(vectors.shape[0])
        self._check_dim(vectors.shape[1])
        index = self._require("mmr")
        k = self._k(top_k)
        fetch = self._k(max(int(fetch_k), k))
        return self._assemble(*self._with_filter(allowed_ids, lambda flt: index.search_mmr(vectors, k, fetch, float(lambda_mult), self.metric, row_filter=flt)))

    def search_mmr_batch(self, queries: Sequence[str], top_k: int = 10, fetch_k: int = 50, lambda_mult: float = 0.5, *,
                         allowed_ids=None) -> List[List[Tuple[str, float, str]]]:
        if not queries:
            return []
        return self.search_mmr_vectors(self._embed_matrix(list(queries)), top_k, fetch_k, lambda_mult, allowed_ids=allowed_ids)

    def search_mmr(self, query: str, top_k: int = 10, fetch_k: int = 50, lambda_mult: float = 0.5, *, allowed_ids=None) -> List[Tuple[str, float, str]]:
        """top_k passages that are relevant and not copies of each other: see `search_mmr_vectors`."""
        return self.search_mmr_batch([query], top_k, fetch_k, lambda_mult, allowed_ids=allowed_ids)[0]

    def search_device_vectors(self, d_vectors, top_k: int = 10) -> List[List[Tuple[str, float, str]]]:
        """Queries that are already in HBM (a CUDA tensor [B][dim] fp32, e.g. `NomicBertEmbedder.embed_device`): searched where they
        are (rq_search_device on torch's current stream), repaired if a certificate failed, ONE device-to-host copy of rows + scores."""
        B = int(d_vectors.shape[0])
        if self._nothing_to_search(top_k, B):
            return self._no_passages(B)
        return self._assemble(*self._search_rows(d_vectors, top_k, on_device=True))

    def _search_device_rows(self, d_vectors, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(scores float32 [B][k], rows int64 [B][k], -1 padded), k = min(top_k, rows of the index)"""
        import torch
        B = int(d_vectors.shape[0])
        self._check_dim(int(d_vectors.shape[1]))
        k = self._k(top_k)
        if not self._can("device"):
            return self._index.search(d_vectors.float().cpu().numpy(), k, self.metric)       # multi-device parent: host-buffer calls only
        dev = d_vectors.device
        q = d_vectors.to(torch.float32).contiguous()
        buf = self.__dict__.get("_dev_out")
        if buf is None or buf[0] < B or buf[1] < k or buf[2].device != dev:
            nb, nk = max(B, buf[0] if buf else 0), max(k, buf[1] if buf else 0)
            block = torch.empty((nb * nk * 3 + nb,), device=dev, dtype=torch.int32)          # [rows int64 | scores fp32 | status int32]
            buf = self.__dict__["_dev_out"] = (nb, nk, block, torch.empty((nb * nk * 3 + nb,), dtype=torch.int32).pin_memory())
        block, pinned = buf[2], buf[3]
        rows_t = block[: 2 * B * k].view(torch.int64).view(B, k)
        scores_t = block[2 * B * k: 3 * B * k].view(torch.float32).view(B, k)
        status_t = block[3 * B * k: 3 * B * k + B]
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            self._index.search_device(q, B, k, self.metric, scores_t, rows_t, None, status_t, stream.cuda_stream)
            self._index.search_flush_device(stream.cuda_stream)
            n = 3 * B * k + B
            pinned[:n].copy_(block[:n], non_blocking=True)
            stream.synchronize()
            if bool(pinned[3 * B * k: n].any()):        # rare: a certificate failed -> exact repair on the device, fetch again
                self._index.search_fixup_device(q, B, k, self.metric, scores_t, rows_t, None, status_t, stream.cuda_stream)
                pinned[:n].copy_(block[:n], non_blocking=True)
                stream.synchronize()
        host = pinned.numpy()
        # copies: the pinned block is written again by the next call, and `search_rows_batch` hands these arrays to its caller
        rows = host[: 2 * B * k].view(np.int64).reshape(B, k).copy()
        scores = host[2 * B * k: 3 * B * k].view(np.float32).reshape(B, k).copy()
        return scores, rows

    # ---- range searches (extension: every passage at least this similar, and how many there are -- what a caller of reference
    # :355-359's collection.query gets by fetching n_results and cutting the list; include/rq.h rq_search_range) -----------------
    def _range_rows(self, vectors: np.ndarray, threshold, cap: int, allowed_ids=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(scores [B][cap], rows [B][cap] -1 padded, counts [B]) of the passages scoring at least `threshold` (a scalar or one value
        per query) under this index's metric.  counts is exact also beyond cap."""
        vectors = self._query_matrix(vectors)
        B = vectors.shape[0]
        cap = max(1, min(int(cap), _native.MAX_K))
        index = self._require("range")
        if self._nothing_to_search(n_queries=B):
            return np.zeros((B, cap), np.float32), np.full((B, cap), -1, np.int64), np.zeros(B, np.int64)
        self._check_dim(vectors.shape[1])
        return self._with_filter(allowed_ids, lambda flt: index.search_range(vectors, threshold, cap, self.metric, row_filter=flt))

    def search_threshold_vectors(self, vectors: np.ndarray, threshold, max_results: int = 100, *, allowed_ids=None) -> List[List[Tuple[str, float, str]]]:
        """Per query vector the passages scoring at least `threshold`, best first, at most max_results (<= 1024) of them:
        [(doc_id, score, text)].  An empty list is the answer "nothing is similar enough"."""
        if max_results <= 0 or self._require("range") is None or len(self._ids) == 0:
            return self._no_passages(np.atleast_2d(np.asarray(vectors)).shape[0])
        scores, rows, _ = self._range_rows(vectors, threshold, max_results, allowed_ids)
        return self._assemble(scores, rows)

    def search_threshold_batch(self, queries: Sequence[str], threshold, max_results: int = 100, *, allowed_ids=None) -> List[List[Tuple[str, float, str]]]:
        if not queries:
            return []
        return self.search_threshold_vectors(self._embed_matrix(list(queries)), threshold, max_results, allowed_ids=allowed_ids)

    def search_threshold(self, query: str, threshold: float, max_results: int = 100, *, allowed_ids=None) -> List[Tuple[str, float, str]]:
        """List of (doc_id, score, text) of the passages whose score is at least `threshold`, best first.  `allowed_ids` as in `search`."""
        return self.search_threshold_batch([query], threshold, max_results, allowed_ids=allowed_ids)[0]

    def count_above(self, query: str, threshold: float, *, allowed_ids=None) -> int:
        """How many passages (of `allowed_ids`, when given) score at least `threshold` for `query`: exact, whatever the number."""
        return int(self._range_rows(self._embed_matrix([query]), threshold, 1, allowed_ids)[2][0])

    # ---- scoring given passages (extension: the dense score of a passage the dense search did not return; Chroma scores only what
    # its query returns, reference :355-359, so the reference's fusion writes 0.0 there, :498-499) -----------------------------------
    def _nothing_to_score(self, n_rows: int) -> bool:
        """... asked once an index that cannot score is refused (`_NEEDS`); the answer is then 0.0 for every row"""
        return self._require("scoring") is None or len(self._ids) == 0 or n_rows == 0

    @staticmethod
    def _row_lists(rows, n_queries: int) -> np.ndarray:
        rows = np.atleast_2d(np.asarray(rows, dtype=np.int64))
        if rows.ndim != 2 or rows.shape[0] != n_queries:
            raise ValueError(f"expected [{n_queries}][m] rows, one list per query, got {rows.shape}")
        return rows

    def score_vectors(self, vectors: np.ndarray, rows) -> np.ndarray:
        """The exact score (this index's metric) of every given query vector against its own list of rows: vectors [B][dim], rows
        [B][m] (row r is `self._ids[r]`; -1 or any row the index does not hold scores 0.0) -> float32 [B][m], the values a search
        returns for those pairs (include/rq.h rq_score_rows)."""
        vectors = self._query_matrix(vectors)
        rows = self._row_lists(rows, vectors.shape[0])
        if self._nothing_to_score(rows.size):
            return np.zeros(rows.shape, np.float32)
        self._check_dim(vectors.shape[1])
        return self._index.score_rows(vectors, rows, self.metric)

    def _score_device_rows(self, d_vectors, rows: np.ndarray) -> np.ndarray:
        """`score_vectors` for queries that are already in HBM (rq_score_rows_device on torch's current stream)."""
        import torch
        B, m = rows.shape
        dev = d_vectors.device
        q = d_vectors.to(torch.float32).contiguous()
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(dev, non_blocking=False)
            d_scores = torch.empty((B, m), device=dev, dtype=torch.float32)
            self._index.score_rows_device(q, B, d_rows, m, self.metric, d_scores, stream.cuda_stream)
            return d_scores.cpu().numpy()

    def _embed_queries(self, queries: Sequence[str], *, host_only: bool = False):
        """The query vectors of one call, embedded ONCE: ("device", tensor in HBM) from an embedder that can leave them there and an
        index that searches them there, else ("host", float32 matrix).  What searched is what scores."""
        d_q = None if host_only or not self._can("device") else self._embed_device(queries)
        return ("host", self._embed_matrix(list(queries))) if d_q is None else ("device", d_q)

    def _search_embedded(self, qv, top_k: int, allowed_ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search_rows_batch` over vectors from `_embed_queries`."""
        kind, vecs = qv
        B = int(vecs.shape[0])
        if self._nothing_to_search(top_k, B):
            return self._no_rows(B)
        return self._search_rows(vecs, top_k, allowed_ids, on_device=kind == "device")

    def _score_embedded(self, qv, rows: np.ndarray) -> np.ndarray:
        kind, vecs = qv
        rows = np.asarray(rows, dtype=np.int64)
        if self._nothing_to_score(rows.size) or not (rows >= 0).any():
            return np.zeros(rows.shape, np.float32)
        if kind == "device":
            return self._score_device_rows(vecs, rows)
        return self.score_vectors(vecs, rows)

    def score_rows_batch(self, queries: Sequence[str], rows) -> np.ndarray:
        """Embeds the query strings (once, where a search would embed them) and scores each against its own list of rows: float32
        [B][m], see `score_vectors`."""
        rows = self._row_lists(rows, len(queries))
        if self._nothing_to_score(rows.size):
            return np.zeros(rows.shape, np.float32)
        return self._score_embedded(self._embed_queries(list(queries)), rows)

    def score_ids(self, query: str, ids: Sequence[str]) -> List[float]:
        """The dense score of `query` for each of the passages `ids`, in their order: what `search` would report for that passage if
        it ranked it.  An id the index does not hold scores 0.0 (the reference's value for "not scored"); an empty index returns
        zeros."""
        ids = list(ids)
        if self._nothing_to_score(len(ids)):
            return [0.0] * len(ids)
        rows = np.fromiter((self._row_of.get(d, -1) for d in ids), np.int64, len(ids))[None, :]
        return self.score_rows_batch([query], rows)[0].astype(np.float64).tolist()

    def search_rows_batch(self, queries: Sequence[str], top_k: int = 10, *, allowed_ids=None, distinct_by: Optional[str] = None,
                          per_group: Optional[int] = None, allowed_ids_each=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search_batch` without the (doc_id, score, text) tuples: (scores float32 [B][k], rows int64 [B][k], -1 padded; row r is
        `self._ids[r]`), k = min(top_k, len(self)).  What HybridRetriever's batched fusion consumes (extension).
        `allowed_ids` (ids or a `make_filter` result): only those passages are ranked; the queries then take the host path.
        `allowed_ids_each`: one such entry (or None) per query, as in `search_vectors`."""
        _refuse_per_group(per_group, "search_rows_batch")
        B = len(queries)
        each = None if allowed_ids_each is None else self._each_entries(allowed_ids_each, B, allowed_ids, distinct_by, per_group)
        if self._nothing_to_search(top_k, B):
            return self._no_rows(B)
        restricted = each is not None or distinct_by is not None or allowed_ids is not None      # (these queries take the host path)
        d_q = None if restricted else self._embed_device(queries)
        if d_q is not None:
            return self._search_rows(d_q, top_k, on_device=True)
        return self._search_rows(self._embed_matrix(list(queries)), top_k, allowed_ids, distinct_by, 1, each)

    def search_batch(self, queries: Sequence[str], top_k: int = 10, *, allowed_ids=None, distinct_by: Optional[str] = None,
                     per_group: Optional[int] = None, allowed_ids_each=None) -> List[List[Tuple[str, float, str]]]:
        """`allowed_ids_each` (keyword-only): one allowed set per query -- a batch of questions from different tenants, sources or
        users in one native call; see `search_vectors`."""
        per = _per_group_size(distinct_by, per_group)
        if not queries and allowed_ids_each is None:
            return []
        # an embedder that can leave its output in HBM (embedders.NomicBertEmbedder.embed_device) feeds the unrestricted search
        # directly: no device -> host -> numpy -> pinned -> device round trip of the query matrix.  Every restricted search
        # takes the host path.
        restricted = allowed_ids_each is not None or per > 1 or distinct_by is not None or allowed_ids is not None
        d_q = None if restricted else self._embed_device(queries)
        if d_q is not None:
            return self.search_device_vectors(d_q, top_k)
        vectors = self._embed_matrix(list(queries)) if queries else np.zeros((0, self.dim), np.float32)      # (none: `allowed_ids_each` is still checked)
        return self.search_vectors(vectors, top_k, allowed_ids=allowed_ids, distinct_by=distinct_by, per_group=per_group, allowed_ids_each=allowed_ids_each)

    def search(self, query: str, top_k: int = 10, *, allowed_ids=None, distinct_by: Optional[str] = None,
               per_group: Optional[int] = None) -> List[Tuple[str, float, str]]:
        """List of (doc_id, score, text), best first; score = cosine similarity (= 1 - Chroma distance).  `allowed_ids` (keyword-only
        extension: ids, or a `make_filter` result for reuse) restricts the ranking to those passages, like a Chroma `where`.
        `distinct_by` (keyword-only extension: a metadata key, e.g. "title") returns one passage per value of that field -- the best
        passage of each of the top_k groups; a passage without the field is a group of its own.  It combines with `allowed_ids`.
        `per_group` (with `distinct_by`; default 1): the best per_group passages of each of the top_k groups, group by group, members
        best first -- up to top_k x per_group entries."""
        per = _per_group_size(distinct_by, per_group)
        return self.search_batch([query], top_k, **_given(allowed_ids=allowed_ids, distinct_by=distinct_by, per_group=per_group if per > 1 else None))[0]

    def __len__(self) -> int:
        return len(self._ids)

    # ---- persistence (the Chroma persist directory of the reference) ------------------------------------
    def _files(self) -> Tuple[Path, Path]:
        base = Path(self.persist_directory) / self.collection_name
        return Path(str(base) + ".docs.jsonl"), base

    def save(self) -> None:
        """rows -> <dir>/<collection>.f16/.meta (rq_save), ids/texts/metadata -> <collection>.docs.jsonl.  Everything is written
        under temporary names first; the data files are then moved into place and the meta replaces the old one LAST (the commit
        point): a process killed anywhere in between leaves either the old commit over files that still contain it as a prefix, or
        the new one."""
        docs_path, base = self._files()
        docs_path.parent.mkdir(parents=True, exist_ok=True)
        if self._index is None:
            return
        docs_tmp, base_tmp = Path(str(docs_path) + ".tmp"), Path(str(base) + ".saving")
        docs_bytes = 0
        with open(docs_tmp, "wb") as f:
            for i, doc_id in enumerate(self._ids):
                line = (json.dumps({"id": doc_id, "text": self._texts[i], "metadata": self._metas[i]}) + "\n").encode()
                f.write(line)
                docs_bytes += len(line)
            f.flush()
            os.fsync(f.fileno())
        self._index.save(str(base_tmp))              # rows (+ a meta of its own, discarded) through rq_save
        os.replace(str(base_tmp) + ".f16", str(base) + ".f16")
        os.replace(docs_tmp, docs_path)
        Path(str(base_tmp) + ".meta").unlink(missing_ok=True)
        _atomic_write(Path(str(base) + ".meta"), f"rq-index 1\ndim {self.dim}\nrows {len(self._ids)}\ndtype f16\ndocs_bytes {docs_bytes}\n".encode())

    def _load(self) -> None:
        docs_path, base = self._files()
        # read-only: bytes beyond the commit are ignored, not cut off (another process may be in the middle of an add; this
        # process truncates only when it appends itself, _persist_append)
        committed = repair_persisted_collection(base, docs_path, truncate=False)
        if committed is None:
            return
        self._index = _native.NativeIndex.load(str(base), self.device, devices=self.devices)     # (rq_load reads `rows` rows, no more)
        self._apply_backend_options()
        self.dim = self._index.dim
        with open(docs_path, "rb") as f:
            for line in f.read(committed["docs_bytes"]).splitlines():
                rec = json.loads(line)
                self._row_of[rec["id"]] = len(self._ids)
                self._ids.append(rec["id"])
                self._texts.append(rec.get("text", ""))
                self._metas.append(rec.get("metadata", {}))
        if len(self._ids) != len(self._index):
            raise RuntimeError(f"persisted index is inconsistent: {len(self._ids)} ids vs {len(self._index)} rows")
        logger.info(f"Loaded DenseIndex with {len(self._ids)} documents")


# =============================================================================================
# hybrid fusion (reference :376-560) -- pure host logic, kept semantically identical
# =============================================================================================
class HybridFilter:
    """One allowed set on both sides of a HybridRetriever (`HybridRetriever.make_filter`): the ids, the sparse mask words over the
    BM25 rows (`BM25Index.make_mask`) and a dense `RowFilter` (`DenseIndex.make_filter`); a side whose index held nothing has None.
    The batch calls accept it wherever they take ids.  It is stale once either index has grown."""

    def __init__(self, ids, sparse: Optional[SparseMask], dense, stamp: Tuple[int, int]):
        self.ids, self.sparse, self.dense, self.stamp = frozenset(ids), sparse, dense, stamp

    def close(self) -> None:
        if self.dense is not None:
            self.dense.close()
            self.dense = None

    def __len__(self) -> int:
        return len(self.ids)


@dataclass(frozen=True)
class _BatchRequest:
    """One hybrid batch call after its keywords were checked (`HybridRetriever._batch_call`): what the private functions pass on."""
    queries: Sequence[str]
    n: int                                  # top_k of hybrid_search_batch, num_passages of the router calls
    pool: int                               # retrieval_pool_size
    complete_scores: bool = False
    each: Optional[list] = None             # one checked HybridFilter or None per query (`_with_filters`); None: no filter keyword was given
    distinct_by: Optional[str] = None


class HybridRetriever:
    """Unified hybrid retrieval combining BM25 and dense retrieval (reference :376-560).

    Extra keyword-only arguments: `dense_index` (inject a ready index), `embedder`, `device`, `sparse_backend` ("host" = default:
    BM25 on the host cores; "gpu": the batch calls -- hybrid_search_batch, get_scores_for_router_batch -- score BM25 on the device,
    same rows and score bits, RqError without one; "auto": the device when one is visible), `fusion_backend` ("host" = default: the
    batch calls fuse both pools with numpy on the host; "gpu": both pools stay in HBM and are fused there -- include/rq.h "hybrid
    fusion", the same values bit for bit -- and only [B][top_k] results come back; it needs `sparse_backend` "gpu" or "auto" and a
    single-device DenseIndex, and raises RqError with the reason otherwise; "auto": the device when all of that holds, else the host).
    The batch calls take `allowed_ids=` / `allowed_ids_each=` (one allowed set per query; `make_filter` for reuse) under every backend.
    `router_backend` ("host" = default: `route_batch` gates and reranks the fused columns with numpy, `router.RouterGate`; "gpu": the
    fused pool stays in HBM, rq_router_rerank_device reranks it there -- include/rq.h "router gate" -- and only [B][top_k] results
    come back; it needs what `fusion_backend`'s device route needs, and raises RqError with the reason otherwise; "auto": the device
    when all of that holds, else the host).
    """

    def __init__(self, bm25_persist_path: str = "./data/bm25_index.pkl", chroma_persist_path: str = "./data/chroma_db",
                 chroma_host: Optional[str] = None, embedding_model: str = "nomic-embed-text",
                 *, dense_index=None, embedder=None, device: int = 0, sparse_backend: str = "host", fusion_backend: str = "host",
                 router_backend: str = "host"):
        for name, backend in (("sparse_backend", sparse_backend), ("fusion_backend", fusion_backend), ("router_backend", router_backend)):
            if backend not in ("host", "gpu", "auto"):
                raise ValueError(f"{name} must be 'host', 'gpu' or 'auto', not {backend!r}")
        self.router_backend = router_backend   # where `route_batch` gates and reranks the fused pool
        self.sparse_backend = sparse_backend   # where the BATCH calls score BM25 (BM25Index.search_batch_rows `backend`); per-query calls stay on the host
        self.fusion_backend = fusion_backend   # where the BATCH calls fuse the two pools (`_fused_rows`)
        self.bm25_index = BM25Index(persist_path=bm25_persist_path)
        if dense_index is not None:
            self.dense_index = dense_index
        elif _gpu_backend_available():
            self.dense_index = DenseIndex(persist_directory=chroma_persist_path,
                                          chroma_host=chroma_host or os.environ.get("CHROMA_HOST"),
                                          embedding_model=embedding_model, embedder=embedder, device=device)
        else:
            self.dense_index = None
            logger.warning("Dense retrieval disabled")   # reference :418-420
        # The reference starts with an empty document store (:422-423) although both indexes persist, so a fresh
        # process over a persisted index answers [].  The BM25 pickle holds every Document:
        # restore the store from it (same signatures, DESIGN.md "deviations").
        self.documents: Dict[str, Document] = dict(self.bm25_index.documents)

    def _sparse_kw(self) -> Dict[str, str]:
        """The `backend` keyword of the BM25 batch calls; nothing for "host", so an injected sparse index needs no such keyword."""
        backend = getattr(self, "sparse_backend", "host")
        return {} if backend == "host" else {"backend": backend}

    def add_documents(self, documents: List[Document], batch_size: int = 100) -> Dict[str, int]:
        for doc in documents:
            self.documents[doc.id] = doc
        stats: Dict[str, int] = {}
        # The reference tests `if self.bm25_index:` / `if self.dense_index:` (:442, :445); both classes
        # define __len__, so an EMPTY index is falsy and never receives its first documents.  That is a
        # defect, not a contract: here the test is `is not None` (DESIGN.md "deviations").
        if self.bm25_index is not None:
            stats["bm25_added"] = self.bm25_index.add_documents(documents)
        if self.dense_index is not None:
            stats["dense_added"] = self.dense_index.add_documents(documents, batch_size)
        stats["total_documents"] = len(self.documents)
        return stats

    # `allowed_ids` (keyword-only extension on the per-query calls): only passages with these ids are ranked, on both sides -- the
    # `where` of a Chroma query.  The sparse side needs the ids themselves; the dense side also takes a DenseIndex.make_filter result.
    # `distinct_by` (keyword-only extension on the per-query calls, a metadata key such as "title"): one passage per value of that
    # field on each side, and the fused list is collapsed once more by best hybrid score.  The `*_batch` calls and `route_batch` take
    # it too: query q's answer is that of the per-query call, value for value; with `allowed_ids`, not with
    # `allowed_ids_each` or `complete_scores`.
    # The `*_batch` calls take `allowed_ids` (one set for the batch) or `allowed_ids_each` (one entry per query: ids, a `make_filter`
    # result, or None for an unrestricted query); query q's answer is that of the per-query call with that entry, value for value.
    # `per_group` (with `distinct_by`): `dense_search` alone passes it on (DenseIndex.search); the sparse side and the fused list
    # return one passage per group, and refuse any other value.
    def bm25_search(self, query: str, top_k: int = 20, *, allowed_ids=None, distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[Tuple[str, float]]:
        _refuse_per_group(per_group, "bm25_search")
        if self.bm25_index is None:
            return []
        return self.bm25_index.search(query, top_k, **_given(allowed_ids=allowed_ids, distinct_by=distinct_by))

    def dense_search(self, query: str, top_k: int = 20, *, allowed_ids=None, distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[Tuple[str, float]]:
        per = _per_group_size(distinct_by, per_group)
        if self.dense_index is None:
            return []
        given = _given(allowed_ids=allowed_ids, distinct_by=distinct_by, per_group=per if per > 1 else None)   # (per > 1: the best `per` passages of each group)
        return [(doc_id, score) for doc_id, score, _ in self.dense_index.search(query, top_k, **given)]

    def dense_search_mmr(self, query: str, top_k: int = 20, fetch_k: int = 50, lambda_mult: float = 0.5, *, allowed_ids=None) -> List[Tuple[str, float]]:
        """`dense_search` diversified: top_k of the exact top fetch_k by maximal marginal relevance, in selection order (DenseIndex.search_mmr)."""
        if self.dense_index is None:
            return []
        return [(doc_id, score) for doc_id, score, _ in self.dense_index.search_mmr(query, top_k, fetch_k, lambda_mult, allowed_ids=allowed_ids)]

    def dense_search_threshold(self, query: str, threshold: float, max_results: int = 100, *, allowed_ids=None) -> List[Tuple[str, float]]:
        """Every passage whose dense score is at least `threshold`, best first, at most max_results (DenseIndex.search_threshold)."""
        if self.dense_index is None:
            return []
        return [(doc_id, score) for doc_id, score, _ in self.dense_index.search_threshold(query, threshold, max_results, allowed_ids=allowed_ids)]

    def dense_search_batch(self, queries: Sequence[str], top_k: int = 20, *, allowed_ids=None, allowed_ids_each=None,
                           distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[List[Tuple[str, float]]]:
        """`allowed_ids` / `allowed_ids_each`: ids, a `make_filter` result or -- this call has no sparse side -- a dense `RowFilter`.
        `distinct_by`: one passage per value of that field, `[dense_search(q, top_k, distinct_by=key, allowed_ids=...) for q in queries]`
        from one grouped search; it takes one filter for the batch (`allowed_ids`), not `allowed_ids_each`."""
        self._check_distinct(distinct_by, per_group, False, allowed_ids_each, "dense_search_batch")
        entries = self._filter_entries(len(queries), allowed_ids, allowed_ids_each, dense_only=True)
        if self.dense_index is None:
            return [[] for _ in queries]
        if distinct_by is not None:
            res = self._dense_batch(queries, top_k, distinct_by=distinct_by, **_given(allowed_ids=None if entries is None else self._dense_half(entries[0])))
        else:
            res = self._dense_batch(queries, top_k, None if entries is None else [self._dense_half(e) for e in entries])
        return [[(d, s) for d, s, _ in r] for r in res]

    def _dense_half(self, entry):
        """What the dense side takes for one filter entry: of a `make_filter` result -- refused when stale -- its RowFilter, or its ids
        where the dense index gave it none; anything else as it came (DenseIndex makes one filter per distinct object of ids)."""
        if not isinstance(entry, HybridFilter):
            return entry
        return list(entry.ids) if self._checked(entry).dense is None else entry.dense

    def _dense_batch(self, queries: Sequence[str], top_k: int, each: Optional[list] = None, **shared):
        """The dense index's `search_batch`, or its `search` query by query where it has none; `each`: one allowed set per query."""
        if hasattr(self.dense_index, "search_batch"):
            return self.dense_index.search_batch(list(queries), top_k, **shared, **_given(allowed_ids_each=each))
        return [self.dense_index.search(q, top_k, **shared, **_given(allowed_ids=e)) for q, e in zip(queries, each or [None] * len(queries))]

    @staticmethod
    def _check_distinct(distinct_by: Optional[str], per_group: Optional[int], complete_scores: bool, allowed_ids_each, what: str) -> None:
        """What the batch calls refuse around `distinct_by=`: the refusals of the per-query calls, and one allowed set
        per query -- the grouped dense search takes one filter for the batch."""
        _refuse_per_group(per_group, what)
        if distinct_by is None:
            return
        if complete_scores:
            raise ValueError("distinct_by does not combine with complete_scores")
        if allowed_ids_each is not None:
            raise ValueError(f"{what}: distinct_by does not combine with allowed_ids_each (the grouped dense search takes one filter for the batch: allowed_ids)")

    # ---- one allowed set per query in the batch calls (extension) --------------------------------------------------
    def _filter_stamp(self) -> Tuple[int, int]:
        bm, dn = self.bm25_index, self.dense_index
        return (len(bm.doc_ids) if isinstance(bm, BM25Index) else -1, len(dn._ids) if isinstance(dn, DenseIndex) else -1)

    def make_filter(self, ids) -> HybridFilter:
        """A reusable filter for the batch calls (`allowed_ids=` / `allowed_ids_each=` accept it wherever they take ids): the id set,
        its mask over the BM25 rows and a dense `RowFilter`.  Unknown ids are ignored.  It describes both indexes as they are now:
        once either has grown the calls refuse it as stale.  `close()` frees the dense filter."""
        ids = list(ids)
        bm, dn = self.bm25_index, self.dense_index
        sparse = bm.make_mask(ids) if isinstance(bm, BM25Index) and bm.doc_ids else None
        dense = dn.make_filter(ids) if isinstance(dn, DenseIndex) and dn._index is not None and len(dn._ids) else None
        return HybridFilter(ids, sparse, dense, self._filter_stamp())

    def _checked(self, flt: HybridFilter) -> HybridFilter:
        if flt.stamp != self._filter_stamp():
            raise _native.RqError(f"the hybrid filter is stale: made over {flt.stamp} (BM25, dense) passages, the indexes hold {self._filter_stamp()}")
        return flt

    def _filter_entries(self, n_queries: int, allowed_ids=None, allowed_ids_each=None, dense_only: bool = False) -> Optional[list]:
        """The two filter keywords of a batch call as one entry per query (ids, a `make_filter` result, or None), or None without
        either.  A bare dense RowFilter is refused by the hybrid calls: it says nothing about BM25 rows."""
        if allowed_ids_each is not None:
            entries = DenseIndex._each_entries(allowed_ids_each, n_queries, allowed_ids)
        elif allowed_ids is not None:
            entries = [allowed_ids] * int(n_queries)
        else:
            return None
        if any(isinstance(e, SparseMask) or (isinstance(e, _native.RowFilter) and not dense_only) for e in entries):
            raise ValueError("the hybrid batch calls take ids or a HybridRetriever.make_filter result: a dense RowFilter or a sparse mask covers one side only")
        return entries

    def _with_filters(self, entries: list, call):
        """`call(filters)` with every entry a checked HybridFilter or None: a caller's own filter passes through; ids become a filter made now
        and closed behind the call (`_with_made_filters`; a filter's whole set-up and tear-down: reuse a `make_filter` result for repeated questions)."""
        return _with_made_filters(entries, lambda e: e is None or (isinstance(e, HybridFilter) and self._checked(e) is e), self.make_filter, call)

    def _batch_call(self, what: str, body, queries: Sequence[str], n: int, pool: int, *, complete_scores: bool, allowed_ids, allowed_ids_each,
                    distinct_by: Optional[str], per_group: Optional[int], early=None):
        """The one way into the hybrid batch calls: the refusals around `distinct_by=` (`what` names the call in them), the call's own checks
        (`early()`; an answer it gives is the call's), the filter keywords as one entry per query, then `body(request)` inside `_with_filters`."""
        self._check_distinct(distinct_by, per_group, complete_scores, allowed_ids_each, what)
        answer = None if early is None else early()
        if answer is not None:
            return answer
        entries = self._filter_entries(len(queries), allowed_ids, allowed_ids_each)
        if entries is None:
            return body(_BatchRequest(queries, n, pool, complete_scores, None, distinct_by))
        return self._with_filters(entries, lambda each: body(_BatchRequest(queries, n, pool, complete_scores, each, distinct_by)))

    def _fuse_columns(self, bm25_list: List[Tuple[str, float]], dense_list: List[Tuple[str, float]], top_k: int, extra=None):
        """Reference :485-523 on parallel lists: union of both pools, ids unknown to `self.documents` dropped, missing score 0.0,
        hybrid = (bm25/max_bm25 + dense/max_dense)/2 with `max(...) or 1` over ALL candidates, stable sort desc, first top_k.
        The reference walks a Python set (arbitrary order); here the union is walked in first-seen order (BM25 pool, then dense
        pool), one admissible instance of that order.  Returns (ids, bm25 scores, dense scores, hybrid scores) of the top_k --
        the RetrievalResult objects (2 us each, 200 candidates per question) are only built for what is returned.
        `extra` (`complete_scores`, from `_completions`): (bm25 scores, dense scores) by id for candidates the other pool does not
        hold; they replace the 0.0, nothing else changes -- not the candidates, not their order."""
        bm25_results = dict(bm25_list)
        dense_results = dict(dense_list)
        documents = self.documents
        ids = [d for d in dict.fromkeys(list(bm25_results) + list(dense_results)) if d in documents]
        if not ids:
            return [], [], [], []
        b = [bm25_results.get(d, 0.0) for d in ids]
        de = [dense_results.get(d, 0.0) for d in ids]
        if extra is not None:
            b = [x if d in bm25_results else extra[0].get(d, 0.0) for d, x in zip(ids, b)]
            de = [y if d in dense_results else extra[1].get(d, 0.0) for d, y in zip(ids, de)]
        max_bm25 = max(b) or 1
        max_dense = max(de) or 1
        h = [(x / max_bm25 + y / max_dense) / 2 for x, y in zip(b, de)]
        order = sorted(range(len(ids)), key=lambda i: h[i] or 0, reverse=True)[:top_k]      # stable, like list.sort(reverse=True)
        return [ids[i] for i in order], [b[i] for i in order], [de[i] for i in order], [h[i] for i in order]

    def _fuse(self, bm25_list: List[Tuple[str, float]], dense_list: List[Tuple[str, float]], top_k: int, extra=None,
              distinct_by: Optional[str] = None) -> List[RetrievalResult]:
        if distinct_by is None:
            ids, b, de, h = self._fuse_columns(bm25_list, dense_list, top_k, extra)
        else:   # every candidate in hybrid order, then the first -- the best hybrid score -- of every value of the field
            ids, b, de, h = self._fuse_columns(bm25_list, dense_list, len(bm25_list) + len(dense_list), extra)
            keep, seen = [], set()
            for i, doc_id in enumerate(ids):
                value = _group_value(self.documents[doc_id], distinct_by)
                if value is not None:
                    if value in seen:
                        continue
                    seen.add(value)
                keep.append(i)
            keep = keep[:max(int(top_k), 0)]
            ids, b, de, h = [ids[i] for i in keep], [b[i] for i in keep], [de[i] for i in keep], [h[i] for i in keep]
        return self._results([ids], [b], [de], [h], [len(ids)])[0]

    def _results(self, ids, b, d, h, count) -> List[List[RetrievalResult]]:
        """The RetrievalResult lists of fused columns: [B][n] ids, bm25, dense and hybrid scores (arrays or lists), the first count[q]
        of row q; text, title and metadata are read from `self.documents` now."""
        documents = self.documents

        def result(doc_id, bs, ds, hs):
            doc = documents[doc_id]
            return RetrievalResult(doc_id=doc_id, text=doc.text, bm25_score=bs, dense_score=ds, hybrid_score=hs, title=doc.title, metadata=doc.metadata)
        rows = [x.tolist() if isinstance(x, np.ndarray) else x for x in (ids, b, d, h)]
        return [[result(*c) for c in zip(row_ids[:int(n)], row_b, row_d, row_h)] for n, row_ids, row_b, row_d, row_h in zip(count, *rows)]

    # `complete_scores` (keyword-only extension on the four fusion calls): the reference's fusion writes 0.0 for the score a passage
    # did not get from the other retriever (:498-499) -- an artefact of the pool size that goes straight into the router's features.
    # With True every candidate gets the score it is missing before the maxima are taken: its exact dense score if the dense index
    # holds its id (rq_score_rows), its BM25 score if BM25 holds it.  False (default) changes nothing.
    def _pools_completed(self, query: str, retrieval_pool_size: int, allowed_ids=None):
        """Both pools of one query and the missing scores of their candidates: (bm25 list, dense list, (bm25 extra, dense extra)).
        The query is embedded once: the vector that searched is the vector that scores."""
        if allowed_ids is not None:
            allowed_ids = list(allowed_ids)
        bm25_list = self.bm25_search(query, retrieval_pool_size, **_given(allowed_ids=allowed_ids))
        dn, bm = self.dense_index, self.bm25_index
        dense_list: List[Tuple[str, float]] = []
        qv = None
        if dn is not None:
            if not isinstance(dn, DenseIndex):
                raise _native.RqError("complete_scores needs this module's DenseIndex on the dense side")
            qv = dn._embed_queries([query], host_only=allowed_ids is not None)
            dense_list = [(d, sc) for d, sc, _ in dn._assemble(*dn._search_embedded(qv, retrieval_pool_size, allowed_ids))[0]] if len(dn) else []
        in_b, in_d, docs = dict(bm25_list), dict(dense_list), self.documents
        dense_extra: Dict[str, float] = {}
        if dn is not None and len(dn):
            miss = [d for d in in_b if d not in in_d and d in docs and d in dn._row_of]
            if miss:
                rows = np.fromiter((dn._row_of[d] for d in miss), np.int64, len(miss))[None, :]
                dense_extra = dict(zip(miss, dn._score_embedded(qv, rows)[0].astype(np.float64).tolist()))
        bm25_extra: Dict[str, float] = {}
        if isinstance(bm, BM25Index) and len(bm):
            row_of = bm._row_of_id()
            miss = [d for d in in_d if d not in in_b and d in docs and d in row_of]
            if miss:
                bm25_extra = dict(zip(miss, bm.score_rows(query, [row_of[d] for d in miss]).tolist()))
        return bm25_list, dense_list, (bm25_extra, dense_extra)

    def hybrid_search(self, query: str, top_k: int = 10, retrieval_pool_size: int = 50, *, allowed_ids=None, complete_scores: bool = False,
                      distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[RetrievalResult]:
        _refuse_per_group(per_group, "hybrid_search")
        if distinct_by is not None:
            if complete_scores:
                raise ValueError("distinct_by does not combine with complete_scores")
            if allowed_ids is not None and not isinstance(allowed_ids, _native.RowFilter):
                allowed_ids = list(allowed_ids)      # (walked twice)
            return self._fuse(self.bm25_search(query, retrieval_pool_size, allowed_ids=allowed_ids, distinct_by=distinct_by),
                              self.dense_search(query, retrieval_pool_size, allowed_ids=allowed_ids, distinct_by=distinct_by), top_k, None, distinct_by)
        if complete_scores:
            bm25_list, dense_list, extra = self._pools_completed(query, retrieval_pool_size, allowed_ids)
            return self._fuse(bm25_list, dense_list, top_k, extra)
        given = _given(allowed_ids=None if allowed_ids is None else list(allowed_ids))      # (walked twice)
        return self._fuse(self.bm25_search(query, retrieval_pool_size, **given), self.dense_search(query, retrieval_pool_size, **given), top_k)

    def hybrid_search_batch(self, queries: Sequence[str], top_k: int = 10, retrieval_pool_size: int = 50, *, complete_scores: bool = False,
                            allowed_ids=None, allowed_ids_each=None, distinct_by: Optional[str] = None, per_group: Optional[int] = None) -> List[List[RetrievalResult]]:
        """All dense pools from one GPU batch, all BM25 pools from one pass over the posting lists on the host cores (librq_bm25.so);
        fusion per query.  `allowed_ids` (one set for the batch) / `allowed_ids_each` (one entry per query: ids, a `make_filter`
        result, or None) restrict both pools of each query: the answer is `hybrid_search(q, ..., allowed_ids=entry_q)`, value for value,
        from one masked BM25 call and one per-query-filtered dense call.  `distinct_by` (a metadata key): one passage per value of that
        field in both pools and in the fused list, `hybrid_search(q, ..., distinct_by=key, allowed_ids=...)` value for value -- on the
        device route one grouped BM25 call, one grouped dense search and the grouped fusion (include/rq.h rq_sparse_topk_grouped_device,
        rq_search_grouped_device, rq_hybrid_fuse_grouped_device)."""
        return self._batch_call("hybrid_search_batch", self._hybrid_search_batch, queries, top_k, retrieval_pool_size, complete_scores=complete_scores,
                                allowed_ids=allowed_ids, allowed_ids_each=allowed_ids_each, distinct_by=distinct_by, per_group=per_group)

    def _hybrid_search_batch(self, req: _BatchRequest) -> List[List[RetrievalResult]]:
        fused = self._fused_rows(req)
        if fused is not None:
            return self._results(*fused)
        return self._per_query_fallback(req, lambda q, **kw: self.hybrid_search(q, req.n, req.pool, **kw), lambda sparse, dense: self._fuse(sparse, dense, req.n))

    def _per_query_fallback(self, req: _BatchRequest, per_query, fuse_pools) -> list:
        """A batch call when one side is not this module's own index class (`_fused_rows` gave None): with filters, `distinct_by` or `complete_scores`
        the per-query call, `per_query(query, **the keywords that were given)`; else `fuse_pools(sparse pool, dense pool)` over `_pools_batch`'s."""
        if req.each is not None or req.distinct_by is not None or req.complete_scores:
            shared = _given(complete_scores=True if req.complete_scores else None, distinct_by=req.distinct_by)
            return [per_query(q, **shared, **_given(allowed_ids=None if e is None else e.ids)) for q, e in zip(req.queries, req.each or [None] * len(req.queries))]
        dense, sparse = self._pools_batch(req.queries, req.pool)
        return [fuse_pools(sparse[i], dense[i]) for i in range(len(req.queries))]

    def _pools_batch(self, queries: Sequence[str], retrieval_pool_size: int):
        dense = self.dense_search_batch(queries, retrieval_pool_size)
        if self.bm25_index is None:
            sparse = [[] for _ in queries]
        elif hasattr(self.bm25_index, "search_batch"):
            sparse = self.bm25_index.search_batch(list(queries), retrieval_pool_size, **self._sparse_kw())
        else:
            sparse = [self.bm25_search(q, retrieval_pool_size) for q in queries]
        return dense, sparse

    @staticmethod
    def _router_arrays(results: List[RetrievalResult], num_passages: int):
        bm25_scores = [r.bm25_score for r in results]
        dense_scores = [r.dense_score for r in results]
        doc_ids = [r.doc_id for r in results]
        texts = [r.text for r in results]
        pad = num_passages - len(results)
        if pad > 0:
            bm25_scores += [0.0] * pad
            dense_scores += [0.0] * pad
            doc_ids += [""] * pad
            texts += [""] * pad
        return bm25_scores, dense_scores, doc_ids, texts

    def get_scores_for_router(self, query: str, num_passages: int = 20, *, retrieval_pool_size: int = 50, allowed_ids=None,
                              complete_scores: bool = False, distinct_by: Optional[str] = None,
                              per_group: Optional[int] = None) -> Tuple[List[float], List[float], List[str], List[str]]:
        """Reference :525-557 (its pools are always 50, :537); `retrieval_pool_size` is a keyword-only extension for
        BASELINE.json configs[4] (top-100 pools), `allowed_ids` restricts both pools to those passages, `complete_scores` fills in the
        score a passage did not get from the other retriever (see `_pools_completed`), `distinct_by` is `hybrid_search`'s: one passage
        per value of that field."""
        given = _given(allowed_ids=allowed_ids, complete_scores=True if complete_scores else None, distinct_by=distinct_by, per_group=per_group)
        return self._router_arrays(self.hybrid_search(query, top_k=num_passages, retrieval_pool_size=retrieval_pool_size, **given), num_passages)

    def get_scores_for_router_batch(self, queries: Sequence[str], num_passages: int = 20, *, retrieval_pool_size: int = 50, complete_scores: bool = False,
                                    allowed_ids=None, allowed_ids_each=None, distinct_by: Optional[str] = None, per_group: Optional[int] = None):
        """`[get_scores_for_router(q, ...) for q in queries]` with the pools of the whole batch computed at once.  When both sides are
        this module's own indexes the fusion itself runs on the whole batch in row space (`_fuse_batch_rows`); otherwise per query on the
        fused columns (no RetrievalResult objects in between).  `allowed_ids` / `allowed_ids_each` as in `hybrid_search_batch`: query
        q's answer is `get_scores_for_router(q, ..., allowed_ids=entry_q)`.  `distinct_by` as in `hybrid_search_batch`: query q's answer
        is `get_scores_for_router(q, ..., distinct_by=key)`."""
        return self._batch_call("get_scores_for_router_batch", self._scores_for_router_batch, queries, num_passages, retrieval_pool_size,
                                complete_scores=complete_scores, allowed_ids=allowed_ids, allowed_ids_each=allowed_ids_each, distinct_by=distinct_by, per_group=per_group)

    def _scores_for_router_batch(self, req: _BatchRequest) -> List[tuple]:
        """`_router_columns` as `get_scores_for_router` returns them: per query (b, d, ids, texts), Python lists."""
        ids, b, de = self._router_columns(req)
        idl, documents = ids.tolist(), self.documents      # (texts are read from the store at call time, as the per-query path does)
        texts = [[documents[d].text if d else "" for d in row] for row in idl]
        return list(zip(b.tolist(), de.tolist(), idl, texts))

    def _router_columns(self, req: _BatchRequest):
        """The columns `get_scores_for_router_batch` hands the router, as arrays: ids [B][P] ("" = padding), b, d float64 [B][P] -- of
        the fused rows of the whole batch, or, where `_fused_rows` gives none, of the per-query path."""
        P = req.n
        fused = self._fused_rows(req)
        if fused is not None:
            ids, b, de, _, count = fused
            ids[np.arange(P)[None, :] >= count[:, None]] = ""
            return ids, b, de

        def padded(sparse, dense):
            ids, b, de, _ = self._fuse_columns(sparse, dense, P)
            pad = max(P - len(ids), 0)
            return b + [0.0] * pad, de + [0.0] * pad, ids + [""] * pad
        cols = self._per_query_fallback(req, lambda q, **kw: self.get_scores_for_router(q, P, retrieval_pool_size=req.pool, **kw), padded)
        ids = np.empty((len(cols), P), dtype=object)
        for q, c in enumerate(cols):
            ids[q, :] = c[2]
        return ids, np.array([c[0] for c in cols], np.float64).reshape(len(cols), P), np.array([c[1] for c in cols], np.float64).reshape(len(cols), P)

    # ---- the learned router over the fused pool (extension; include/rq.h "router gate") ------------------------------
    def _route_batch(self, req: _BatchRequest, router, top_k: int, return_weights: bool):
        P, r = req.n, min(int(top_k), req.n)

        def refusal():
            if not (isinstance(self.bm25_index, BM25Index) and isinstance(self.dense_index, DenseIndex)):
                return "one of the two indexes is not this module's own index class"
            reason = self._device_fusion_refusal(P, req.pool)
            if reason is None:
                try:
                    router.native(self._fusion_device())
                except _native.RqError as e:
                    reason = f"the gate cannot be placed on the device: {e}"
            return reason
        if self._on_device("router_backend", refusal):
            ids, b, de, w, h, count = self._fuse_batch_device(req, route=(router, r))
        else:
            ids, cb, cd = self._router_columns(req)
            keys = np.where(ids != "", np.arange(P, dtype=np.int32)[None, :], -1)
            _, b, de, w, h, pos, count = router.rerank(keys, cb, cd, np.full(len(req.queries), P), r)
            ids = np.take_along_axis(ids, np.where(pos >= 0, pos, 0).astype(np.int64), 1)
        out = self._results(ids, b, de, h, count)
        return (out, w) if return_weights else out

    def route_batch(self, queries: Sequence[str], router, top_k: int = 10, *, num_passages: int = 20, retrieval_pool_size: int = 50, complete_scores: bool = False,
                    allowed_ids=None, allowed_ids_each=None, return_weights: bool = False, distinct_by: Optional[str] = None, per_group: Optional[int] = None):
        """Retrieve, gate and rerank a batch: the loop of reference experiments/run_evaluation.py:165-184 as one call.  For every
        question the `num_passages` fused passages of `get_scores_for_router` are weighted by `router` (a `router.RouterGate`) and
        reordered by h = w*dense + (1 - w)*bm25; the first `top_k` real passages come back, best first, `hybrid_score` = h.  Question
        q's answer is the host gate's rerank of `get_scores_for_router(q, num_passages, ...)`'s columns, with the same filters and
        `complete_scores`.  `return_weights=True` adds the gate weights, float64 [B][top_k] (0.0 beyond a question's results).
        `distinct_by`: the fused passages are `get_scores_for_router(q, ..., distinct_by=key)`'s, one per value of that field; the
        rerank is unchanged.  Where it runs is `router_backend`'s choice."""
        queries = list(queries)

        def early():      # this call's own two checks, where they stand in the order of refusals: behind `distinct_by`'s, before the filters'
            if int(num_passages) < 1 or int(top_k) < 1:
                raise ValueError(f"num_passages {num_passages} and top_k {top_k} must be at least 1")
            if not queries:
                return ([], np.zeros((0, min(int(top_k), int(num_passages))))) if return_weights else []
        return self._batch_call("route_batch", lambda req: self._route_batch(req, router, top_k, return_weights), queries, int(num_passages), retrieval_pool_size,
                                complete_scores=complete_scores, allowed_ids=allowed_ids, allowed_ids_each=allowed_ids_each, distinct_by=distinct_by,
                                per_group=per_group, early=early)

    def route(self, query: str, router, top_k: int = 10, **keywords):
        """`route_batch([query], ...)[0]` (with `return_weights=True`: the list and the weights of that one question)."""
        out = self.route_batch([query], router, top_k, **keywords)
        return (out[0][0], out[1][0]) if keywords.get("return_weights") else out[0]

    # ---- batched fusion in row space (extension; configs[4]: 500 questions x two pools of 100) ------------------------------------
    def _key_space(self):
        """One integer key per document either index can return: BM25 row r -> r, dense row j -> the BM25 row of the same id if BM25
        holds it, else n_bm25 + j.  Per key: the id and whether `self.documents` knows it at all (reference :491-493 skips ids it does
        not), and the dense row that holds its id (-1: none; `complete_scores`).  Rebuilt when any of the three stores has grown."""
        bm, dn = self.bm25_index, self.dense_index
        stamp = (len(bm.doc_ids), len(dn._ids), len(self.documents))
        c = self.__dict__.get("_keys_cache")
        if c is not None and c["stamp"] == stamp:
            return c
        if c is not None and c.get("map") is not None:      # the device copy follows the key space it was built from
            c.pop("map").close()
        nb = len(bm.doc_ids)
        row_of = {d: i for i, d in enumerate(bm.doc_ids)}
        dense_key = np.fromiter((row_of.get(d, nb + j) for j, d in enumerate(dn._ids)), np.int64, len(dn._ids))
        all_ids = list(bm.doc_ids) + list(dn._ids)
        ids = np.empty(len(all_ids), dtype=object)
        ids[:] = all_ids
        docs = self.documents
        known = np.fromiter((d in docs for d in all_ids), np.bool_, len(all_ids))
        dense_row = np.full(len(all_ids), -1, np.int64)
        dense_row[dense_key] = np.arange(len(dn._ids), dtype=np.int64)
        # DenseIndex.add_documents skips ids it holds, but add_vectors, from_native and a loaded collection take ids as they come: whether
        # dense_key is injective (the device fusion needs it, include/rq.h rq_hybrid_create) is checked once per rebuild
        injective = len(np.unique(dense_key)) == len(dense_key)
        c = self.__dict__["_keys_cache"] = {"stamp": stamp, "nb": nb, "dense_key": dense_key, "ids": ids, "known": known, "dense_row": dense_row,
                                            "injective": injective, "map": None}
        return c

    # ---- the same fusion on the device (extension; include/rq.h "hybrid fusion") -----------------------------------
    def _device_fusion_refusal(self, top_k: int, retrieval_pool_size: int) -> Optional[str]:
        """Why this call cannot be fused on the device, or None.  (DenseIndex never sets a row offset: its rows are positions in `_ids`.)"""
        bm, dn = self.bm25_index, self.dense_index
        sparse = getattr(self, "sparse_backend", "host")
        if not _native.sparse_available():
            return "no HIP device is visible"
        if sparse == "host":
            return "sparse_backend is 'host': the sparse pool must be drawn on the device (sparse_backend='gpu' or 'auto')"
        if dn._index is not None and not (isinstance(dn._index, _native.NativeIndex) and dn._can("device")):
            return "the dense index is not a single-device NativeIndex"
        if dn._index is not None and bm.__dict__.get("sparse_device", 0) != dn._index.device:
            return "the sparse and the dense index are on different devices"
        if not 1 <= int(top_k) <= _native.MAX_K or max(int(retrieval_pool_size), 1) > _native.SPARSE_MAX_K:
            return f"top_k {top_k} or pool {retrieval_pool_size} beyond {_native.MAX_K}"
        if not self._key_space()["injective"]:
            return "the dense index holds an id twice: dense rows do not map to distinct keys"
        return None

    def _on_device(self, which: str, refusal) -> bool:
        """The placement rule of `fusion_backend` and `router_backend` (`which` names the attribute): "host" stays on the host; "auto"
        takes the device unless `refusal()` gives a reason; "gpu" raises that reason."""
        backend = getattr(self, which, "host")
        if backend == "host":
            return False
        reason = refusal()
        if reason is not None and backend == "gpu":
            raise _native.RqError(f"{which}='gpu': {reason}")
        return reason is None

    def _fusion_device(self) -> int:
        """The device both pools are drawn on: the dense index's, the sparse index's while the dense index holds nothing."""
        dn = self.dense_index
        return dn._index.device if dn._index is not None else self.bm25_index.__dict__.get("sparse_device", 0)

    def _hybrid_map(self, ks, device: int):
        """The device copy of the key space (`_native.HybridMap`): built by the first fusion that wants it, dropped with the key space."""
        if ks.get("map") is None:
            ks["map"] = _native.HybridMap(ks["nb"], ks["dense_key"], ks["known"], device=device)
        return ks["map"]

    def _key_groups(self, ks, key: str) -> np.ndarray:
        """One int32 per key of the key space for `distinct_by=key`: the group of the document `self.documents` holds under the key's id
        (what `_fuse` reads), -1 for a group of its own and for ids the store does not know.  Cached per key with the key space."""
        tables = ks.setdefault("groups", {})
        if key not in tables:
            ids: Dict[Any, int] = {}
            docs = self.documents
            values = (_group_value(docs[d], key) if d in docs else None for d in ks["ids"].tolist())
            tables[key] = np.fromiter((_native.GROUP_NONE if v is None else ids.setdefault(v, len(ids)) for v in values), np.int32, len(ks["ids"]))
        return tables[key]

    def _fuse_batch_device(self, req: _BatchRequest, route: Optional[tuple] = None):
        """`_fused_rows` with both pools left where they are drawn, in steps on torch's current stream of the fusion device: token ids
        and query vectors go down and fill the two pools in HBM (`_device_sparse_pool`, `_device_dense_pool`), `complete_scores` adds
        the scores they miss (`_device_completions`), `_device_fuse` ranks, and one copy brings [B][top_k] keys, scores and the counts
        back (`_device_block`).  Same return value.  Pools that are already filtered (`each`) or grouped (`distinct_by`, DESIGN.md 4.23:
        never with `complete_scores`, `each` then holds one filter for the whole batch) fuse as they are.
        `route` = (router.RouterGate, top_r): the fused block stays on the device, rq_router_rerank_device runs on the same stream
        over its keys, b, d and counts, and the one copy brings [B][top_r] up instead: (ids, b, d, w, h -- [B][top_r] -- and count [B])."""
        import torch
        queries = list(req.queries)
        B, k, K1 = len(queries), int(req.n), max(int(req.pool), 1)
        ks = self._key_space()
        device = self._fusion_device()
        hm = self._hybrid_map(ks, device)
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            sparse = self._device_sparse_pool(req, queries, K1, dev, s)
            dense = self._device_dense_pool(req, queries, dev, s)
            extra = self._device_completions(hm, sparse, dense, B, K1, dev, s) if req.complete_scores else {}
            (b, de, h), (keys,), count, read = self._device_block(dev, B, k, 3, 1)
            self._device_fuse(req, ks, hm, (sparse[0], sparse[1], dense[2], dense[3], B, K1, dense[0], k), (keys, b, de, h, None, count, s), extra)
            if route is not None:
                gate, r = route
                (ob, od, ow, oh), (okeys, opos), ocount, read = self._device_block(dev, B, r, 4, 2)
                gate.native(device).rerank_device(keys, b, de, count, B, k, r, okeys, ob, od, ow, oh, opos, ocount, mode=gate.mode, stats=gate.stats, stream=s)
            scores, (keys, *_), count = read()
        return (ks["ids"][np.where(keys >= 0, keys, 0)], *scores, count)

    def _device_sparse_pool(self, req: _BatchRequest, queries: List[str], K1: int, dev, s):
        """The sparse pool in HBM: (rows int32 [B][K1], scores float64 [B][K1], what rescoring needs -- the index, the queries' token
        pointers, tokens and their count -- or None where BM25 has nothing to search: a pool of padding)."""
        import torch
        bm, B = self.bm25_index, len(queries)
        d_rows = torch.empty((B, K1), device=dev, dtype=torch.int32)
        d_scores = torch.empty((B, K1), device=dev, dtype=torch.float64)
        if not (bm.bm25 is not None and bm.doc_ids and req.pool > 0):
            d_rows.fill_(-1)
            d_scores.zero_()
            return d_rows, d_scores, None
        c = bm._csr()
        sp = bm._sparse_index(c)
        q_ptr, q_tok = bm._query_csr(c, queries)
        d_ptr = torch.tensor(q_ptr, dtype=torch.int64).to(dev)
        d_tok = torch.tensor(q_tok or [0], dtype=torch.int32).to(dev)
        masked = {}
        if req.each is not None:
            masks, mask_of = bm._mask_table([None if e is None else e.sparse for e in req.each])
            # (torch has no arithmetic on uint32 and needs none: the words travel as int32)
            masked = {"d_masks": None if masks is None else torch.from_numpy(masks.view(np.int32)).to(dev),
                      "n_masks": 0 if masks is None else len(masks), "d_mask_of": torch.from_numpy(mask_of).to(dev)}
        if req.distinct_by is not None:
            sp = bm._sparse_index_grouped(c, req.distinct_by)
            sp.topk_grouped_device(d_ptr, d_tok, B, len(q_tok), K1, d_rows, d_scores, torch.empty((B,), device=dev, dtype=torch.int32), stream=s, **masked)
        else:
            sp.topk_device(d_ptr, d_tok, B, len(q_tok), K1, d_rows, d_scores, stream=s, **masked)
        return d_rows, d_scores, (sp, d_ptr, d_tok, len(q_tok))

    def _device_dense_pool(self, req: _BatchRequest, queries: List[str], dev, s):
        """The dense pool in HBM: (K2, query vectors fp32 [B][dim], rows int64 [B][K2], scores float32 [B][K2]), or (0, None, None, None)
        where the dense index has nothing to search.  One of three routes -- grouped under the batch's one filter, one filter per
        query, plain -- as (search, fixup, their arguments); the status is read once, and the fixup runs where it says so."""
        import torch
        dn, B = self.dense_index, len(queries)
        if dn._nothing_to_search(req.pool, B):
            return 0, None, None, None
        d_q = dn._embed_device(queries)
        if d_q is None:
            d_q = torch.from_numpy(np.ascontiguousarray(dn._embed_matrix(list(queries)), dtype=np.float32)).to(dev)
        d_q = d_q.to(torch.float32).contiguous()
        dn._check_dim(int(d_q.shape[1]))
        K2, index = dn._k(req.pool), dn._index
        d_rows = torch.empty((B, K2), device=dev, dtype=torch.int64)
        d_scores = torch.empty((B, K2), device=dev, dtype=torch.float32)
        d_status = torch.empty((B,), device=dev, dtype=torch.int32)
        keywords = {}
        if req.distinct_by is not None:      # (its fixup: fewer than K2 groups in the first rung, or no certificate)
            dn._push_groups(req.distinct_by)
            keywords = {"row_filter": None if req.each is None or req.each[0] is None else req.each[0].dense}
            d_groups = torch.empty((B, K2), device=dev, dtype=torch.int32)
            search, fixup, args = index.search_grouped_device, index.search_grouped_fixup_device, (d_scores, d_rows, d_groups, None, d_status, s)
        elif req.each is not None:
            filters = [None if e is None else e.dense for e in req.each]
            search, fixup, args = index.search_filtered_each_device, index.search_filtered_each_fixup_device, (d_scores, d_rows, None, d_status, filters, s)
        else:                                # (its fixup is rare: a certificate failed -> exact repair on the device)
            search, fixup, args = index.search_device, index.search_fixup_device, (d_scores, d_rows, None, d_status, s)
        search(d_q, B, K2, dn.metric, *args, **keywords)
        if req.distinct_by is None and req.each is None:
            index.search_flush_device(s)
        if bool(d_status.any()):
            fixup(d_q, B, K2, dn.metric, *args, **keywords)
        return K2, d_q, d_rows, d_scores

    def _device_completions(self, hm, sparse, dense, B: int, K1: int, dev, s) -> dict:
        """`complete_scores` in HBM: which candidates miss a score (rq_hybrid_missing_device), then the dense scores of the sparse pool
        and the BM25 scores of the dense pool; returns the miss / extra keywords of `fuse_device`."""
        import torch
        d_sp_rows, _, rescore = sparse
        K2, d_q, d_de_rows, _ = dense
        dn, extra = self.dense_index, {}
        d_miss_dense = torch.empty((B, K1), device=dev, dtype=torch.int64)
        d_miss_sparse = torch.empty((B, max(K2, 1)), device=dev, dtype=torch.int32)
        hm.missing_device(d_sp_rows, d_de_rows, B, K1, K2, d_miss_dense, d_miss_sparse, s)
        if K2:
            d_extra_dense = torch.empty((B, K1), device=dev, dtype=torch.float32)
            dn._index.score_rows_device(d_q, B, d_miss_dense, K1, dn.metric, d_extra_dense, s)
            extra.update(d_miss_dense=d_miss_dense, d_extra_dense=d_extra_dense)
            if rescore is not None:
                sp, d_ptr, d_tok, n_tok = rescore
                d_extra_sparse = torch.empty((B, K2), device=dev, dtype=torch.float64)
                sp.score_rows_device(d_ptr, d_tok, B, n_tok, d_miss_sparse, K2, d_extra_sparse, s)
                extra.update(d_miss_sparse=d_miss_sparse, d_extra_sparse=d_extra_sparse)
        return extra

    def _device_fuse(self, req: _BatchRequest, ks, hm, pools: tuple, out: tuple, extra: dict) -> None:
        """Rank `pools` (rows and scores of both, B, K1, K2, top_k) into `out` (keys, b, d, h, positions, count, stream):
        rq_hybrid_fuse_device, or under `distinct_by` the grouped form over the key groups of that field (pushed when it changes)."""
        if req.distinct_by is None:
            return hm.fuse_device(*pools, *out, **extra)
        if ks.get("map_group_key") != req.distinct_by:
            hm.set_groups(self._key_groups(ks, req.distinct_by))
            ks["map_group_key"] = req.distinct_by
        hm.fuse_grouped_device(*pools, *out)

    @staticmethod
    def _device_block(dev, B: int, width: int, n_scores: int, n_keys: int):
        """One int32 block in HBM: n_scores float64 planes [B][width] | n_keys int32 planes [B][width] | count int32 [B].  Returns the planes and
        the count as flat device views, and `read()`: the one copy up, as (float64 [n_scores][B][width], int32 [n_keys][B][width], count int64 [B])."""
        import torch
        m, a, z = B * width, 2 * n_scores * B * width, (2 * n_scores + n_keys) * B * width
        block = torch.empty((z + B,), device=dev, dtype=torch.int32)
        scores = block[:a].view(torch.float64)

        def read():
            host = block.cpu().numpy()
            return host[:a].view(np.float64).reshape(n_scores, B, width), host[a:z].reshape(n_keys, B, width), host[z:].astype(np.int64)
        return [scores[i * m: (i + 1) * m] for i in range(n_scores)], [block[a + i * m: a + (i + 1) * m] for i in range(n_keys)], block[z:], read

    def _fuse_batch_rows(self, queries: Sequence[str], top_k: int, retrieval_pool_size: int, complete_scores: bool = False, each: Optional[list] = None,
                         distinct_by: Optional[str] = None):
        """`_fused_rows` of these arguments (the name tools, tests and include/rq.h know the batched fusion by)."""
        return self._fused_rows(_BatchRequest(queries, top_k, retrieval_pool_size, complete_scores, each, distinct_by))

    def _fused_rows(self, req: _BatchRequest):
        """`_fuse_columns` for every query of the batch at once, on integer keys: same candidates (union of both pools in first-seen
        order -- BM25 pool, then dense pool -- ids unknown to `self.documents` dropped), same float64 arithmetic (`max(...) or 1` over all
        candidates, hybrid = (b/max_b + d/max_d)/2), same stable descending sort, first top_k.  Returns (ids [B][top_k] object,
        bm25 scores, dense scores, hybrid scores, count [B]) -- entries beyond count[b] are padding -- or None when one of the two sides
        is not this module's own index class (then the per-query path runs).
        `complete_scores`: after both pools are drawn and before the maxima are taken, ONE dense scoring call for the batch ([B][K1]
        dense rows of the BM25 pool, -1 where nothing is missing or no dense row exists) and one BM25 batch call for the dense-only
        entries fill in the scores the reference leaves at 0.0; the queries are embedded once for the search and the scoring.
        `each` (one HybridFilter or None per query, from `_with_filters`): the sparse pool comes from the masked `search_batch_rows`,
        the dense pool from ONE per-query-filtered call (`DenseIndex._search_rows(each=...)`) over vectors embedded on the host, as the
        per-query filtered calls embed them; the rest is untouched -- a candidate comes from a filtered pool, its missing score is
        the plain score of that pair.
        `distinct_by` (never with `complete_scores`; `each` then holds one filter for the whole batch): on the host route the sparse
        pools come from `search_batch(distinct_by=)`, the dense pools from the grouped `search_batch(distinct_by=)`, and `_fuse(...,
        distinct_by=)` runs per query -- the per-query call's own steps; the device route is `_fuse_batch_device`'s."""
        bm, dn = self.bm25_index, self.dense_index
        queries, top_k, retrieval_pool_size, complete_scores, each, distinct_by = req.queries, req.n, req.pool, req.complete_scores, req.each, req.distinct_by
        if not (isinstance(bm, BM25Index) and isinstance(dn, DenseIndex)) or len(queries) == 0 or top_k <= 0:
            return None
        if self._on_device("fusion_backend", lambda: self._device_fusion_refusal(top_k, retrieval_pool_size)):
            return self._fuse_batch_device(req)
        B = len(queries)
        if distinct_by is not None:
            e = None if each is None else each[0]
            sparse = bm.search_batch(list(queries), retrieval_pool_size, **self._sparse_kw(), distinct_by=distinct_by, **_given(allowed_ids=None if e is None else e.sparse))
            dense = [[(d, sc) for d, sc, _ in r] for r in dn.search_batch(list(queries), retrieval_pool_size, distinct_by=distinct_by, **_given(allowed_ids=self._dense_half(e)))]
            ids = np.full((B, top_k), "", dtype=object)
            b, de, hy, count = np.zeros((B, top_k)), np.zeros((B, top_k)), np.zeros((B, top_k)), np.zeros(B, np.int64)
            for q in range(B):
                res = self._fuse(sparse[q], dense[q], top_k, None, distinct_by)
                count[q] = len(res)
                ids[q, :len(res)] = [r.doc_id for r in res]
                b[q, :len(res)], de[q, :len(res)], hy[q, :len(res)] = [r.bm25_score for r in res], [r.dense_score for r in res], [r.hybrid_score for r in res]
            return ids, b, de, hy, count
        ks = self._key_space()
        sparse_each = {} if each is None else {"allowed_ids_each": [None if e is None else e.sparse for e in each]}
        sp_rows, sp_scores = bm.search_batch_rows(list(queries), retrieval_pool_size, **self._sparse_kw(), **sparse_each)
        if each is not None:
            qv = dn._embed_queries(list(queries), host_only=True)
            if dn._nothing_to_search(retrieval_pool_size, B):
                de_scores, de_rows = dn._no_rows(B)
            else:
                de_scores, de_rows = dn._search_rows(qv[1], retrieval_pool_size, each=[None if e is None else e.dense for e in each])
        elif complete_scores:
            qv = dn._embed_queries(list(queries))
            de_scores, de_rows = dn._search_embedded(qv, retrieval_pool_size)
        else:
            de_scores, de_rows = dn.search_rows_batch(list(queries), retrieval_pool_size)
        K1, K2 = sp_rows.shape[1], de_rows.shape[1]
        sp_keys = sp_rows.astype(np.int64)
        de_keys = np.where(de_rows >= 0, ks["dense_key"][np.where(de_rows >= 0, de_rows, 0)], -1) if K2 else np.zeros((B, 0), np.int64)
        keys = np.concatenate([sp_keys, de_keys], axis=1)
        bsc = np.concatenate([sp_scores, np.zeros((B, K2))], axis=1)
        dsc = np.concatenate([np.zeros((B, K1)), de_scores.astype(np.float64)], axis=1)
        valid = keys >= 0
        valid &= ks["known"][np.where(valid, keys, 0)]
        # a document in both pools: its dense score moves to the BM25 entry (first seen), the dense entry goes
        order = np.argsort(keys, axis=1, kind="stable")
        sk = np.take_along_axis(keys, order, 1)
        r, j = np.nonzero((sk[:, 1:] == sk[:, :-1]) & (sk[:, 1:] >= 0))
        first, second = order[r, j], order[r, j + 1]
        dsc[r, first] = dsc[r, second]
        valid[r, second] = False
        if complete_scores:
            have_dense = np.zeros(keys.shape, dtype=bool)
            have_dense[:, K1:] = True
            have_dense[r, first] = True
            need = valid[:, :K1] & ~have_dense[:, :K1]
            d_rows = np.where(need, ks["dense_row"][np.where(need, keys[:, :K1], 0)], -1)
            if K1 and (d_rows >= 0).any():
                got = dn._score_embedded(qv, d_rows).astype(np.float64)
                dsc[:, :K1] = np.where(d_rows >= 0, got, dsc[:, :K1])
            b_rows = np.where(valid[:, K1:] & (keys[:, K1:] < ks["nb"]), keys[:, K1:], -1)      # dense-only entries that are still candidates
            if K2 and (b_rows >= 0).any():
                bsc[:, K1:] = np.where(b_rows >= 0, bm.score_rows_batch(list(queries), b_rows), bsc[:, K1:])
        neg_inf = -np.inf
        max_b = np.where(valid, bsc, neg_inf).max(axis=1, initial=neg_inf)
        max_d = np.where(valid, dsc, neg_inf).max(axis=1, initial=neg_inf)
        max_b = np.where((max_b == 0) | ~np.isfinite(max_b), 1.0, max_b)          # `max(...) or 1` (a row without candidates: anything)
        max_d = np.where((max_d == 0) | ~np.isfinite(max_d), 1.0, max_d)
        h = (bsc / max_b[:, None] + dsc / max_d[:, None]) / 2
        sort_key = np.where(valid, -np.where(h == 0, 0.0, h), np.inf)            # `key = hybrid or 0`, descending, stable; dropped entries last
        sel = np.argsort(sort_key, axis=1, kind="stable")[:, :top_k]
        if sel.shape[1] < top_k:                                                  # pools smaller than top_k: pad the columns
            sel = np.concatenate([sel, np.zeros((B, top_k - sel.shape[1]), np.int64)], axis=1)
        count = np.minimum(valid.sum(axis=1), top_k)
        live = np.arange(top_k)[None, :] < count[:, None]
        out_keys = np.where(live, np.take_along_axis(keys, sel, 1), 0)
        b = np.where(live, np.take_along_axis(bsc, sel, 1), 0.0)
        de = np.where(live, np.take_along_axis(dsc, sel, 1), 0.0)
        hy = np.where(live, np.take_along_axis(h, sel, 1), 0.0)
        return ks["ids"][out_keys], b, de, hy, count

    def close(self) -> None:
        """Write the BM25 snapshot if documents were added since the last one (extension; the reference has no close)."""
        if self.bm25_index is not None and hasattr(self.bm25_index, "close"):
            self.bm25_index.close()
        c = self.__dict__.pop("_keys_cache", None)
        if c is not None and c.get("map") is not None:
            c.pop("map").close()

    def __len__(self) -> int:
        return len(self.documents)


# =============================================================================================
# streaming indexer + checkpoint (reference :563-686)
# =============================================================================================
class StreamingIndex:
    """Resumable JSONL -> retriever feeder with the reference's checkpoint schema
    {'last_offset', 'total_indexed', 'files_completed'} (:593-604)."""

    def __init__(self, retriever: HybridRetriever, checkpoint_path: str = "./data/index_checkpoint.json", batch_size: int = 100):
        self.retriever = retriever
        self.checkpoint_path = Path(checkpoint_path)
        self.batch_size = batch_size
        self.progress = self._load_checkpoint()

    def _load_checkpoint(self) -> Dict[str, Any]:
        if self.checkpoint_path.exists():
            with open(self.checkpoint_path) as f:
                return json.load(f)
        return {"last_offset": 0, "total_indexed": 0, "files_completed": []}

    def _save_checkpoint(self):
        self.checkpoint_path.parent.mkdir(parents=True, exist_ok=True)
        with open(self.checkpoint_path, "w") as f:
            json.dump(self.progress, f)

    def _commit(self, batch: List[Document], offset: int) -> int:
        self.retriever.add_documents(batch)
        self.progress["last_offset"] = offset
        self.progress["total_indexed"] += len(batch)
        self._save_checkpoint()
        return len(batch)

    def stream_from_jsonl(self, jsonl_path: str, resume: bool = True) -> Iterator[int]:
        path = Path(jsonl_path)
        if not path.exists():
            raise FileNotFoundError(f"Corpus file not found: {jsonl_path}")
        start_offset = self.progress["last_offset"] if resume else 0
        with open(path) as f:
            for _ in range(start_offset):
                f.readline()
            batch: List[Document] = []
            offset = start_offset
            for line in f:
                try:
                    data = json.loads(line.strip())
                    batch.append(Document(id=data["id"], text=data["text"], title=data.get("title"), metadata=data.get("metadata")))
                except (json.JSONDecodeError, KeyError) as e:
                    logger.warning(f"Skipping invalid line at offset {offset}: {e}")
                offset += 1
                if len(batch) >= self.batch_size:
                    n = self._commit(batch, offset)
                    logger.info(f"Indexed batch: {n} docs, total: {self.progress['total_indexed']}")
                    yield n
                    batch = []
            if batch:
                yield self._commit(batch, offset)
        if jsonl_path not in self.progress["files_completed"]:
            self.progress["files_completed"].append(jsonl_path)
            self._save_checkpoint()
        logger.info(f"Completed indexing {jsonl_path}")

    def get_progress(self) -> Dict[str, Any]:
        return {**self.progress, "retriever_size": len(self.retriever)}
