"""One corpus for the route_batch checks -- TEST INFRASTRUCTURE shared by tests/test_router.py (host route over a host stand-in for the
dense index, where the separation of the hybrid scores is established) and tests/test_gpu_router.py (both routes over the real
indexes): 3 000 passages of 12 to 30 words from a skewed vocabulary of 300 (the generator of tests/test_gpu_hybrid.py), 70 questions,
per-question tenant sets, and a seeded router of 64 hidden units."""
import os

import numpy as np

from rag_uq_amd import router as rt
from rag_uq_amd import streaming_index as si

import router_gate_oracle as rgo

SEED, N_PASSAGES, N_QUESTIONS = 4, 3000, 70


def _words(rng, lo, hi):
    p = 1.0 / np.arange(1, 301) ** 0.9
    p /= p.sum()
    return " ".join(f"w{w}" for w in rng.choice(300, rng.integers(lo, hi), p=p))


def corpus():
    rng = np.random.default_rng(SEED)
    docs = [si.Document(id=f"p{i}", text=_words(rng, 12, 31), title=f"T{i % 40}") for i in range(N_PASSAGES)]
    questions = [_words(rng, 1, 10) for _ in range(N_QUESTIONS - 2)] + ["", "zzz unknown words"]
    tenants = [{f"p{i}" for i in range(t, N_PASSAGES, 4)} | {f"nobody{t}"} for t in range(4)]
    each = [None if q % 5 == 2 else (set() if q == 11 else tenants[q % 4]) for q in range(N_QUESTIONS)]
    return docs, questions, each


def gate(normalize="query"):
    w = rgo.make_weights(64, 2024)
    g = rt.RouterGate(w["w0"], w["b0"], w["w1"], w["b1"], normalize=normalize)
    if normalize == "stats":
        g.set_stats(6.0, 4.0, 0.3, 0.25)
    return g


def retriever(path, dense_index=None, embedder=None, **keywords):
    """`embedder`: HashEmbedder() unless given (tests/test_gpu_device_queries.py passes the twins of tests/device_twin.py)."""
    from rag_uq_amd.embedders import HashEmbedder
    os.makedirs(path, exist_ok=True)
    return si.HybridRetriever(bm25_persist_path=str(path / "bm25.pkl"), chroma_persist_path=str(path / "dense"),
                              embedder=HashEmbedder() if embedder is None else embedder, dense_index=dense_index, **keywords)


def answers(out):
    return [[(x.doc_id, x.text, x.bm25_score, x.dense_score, x.hybrid_score) for x in res] for res in out]


def separated(out, rel=1e-9):
    """Adjacent distinct hybrid scores of every question differ by more than `rel` relative: a tolerance on w cannot reorder them."""
    for res in out:
        h = np.array([x.hybrid_score for x in res])
        for x, y in zip(h[:-1], h[1:]):
            if x != y and not abs(x - y) > rel * max(abs(x), abs(y)):
                return False
    return True
