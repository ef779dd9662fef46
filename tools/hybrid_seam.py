"""The Python seam of HybridRetriever's batch calls on the host route, timed without a device: a 5 000-passage synthetic corpus (12 to 30
words from a skewed vocabulary of 300, 40 titles), RandomProjectionEmbedder(64), the host stand-in for the dense index the CPU tests use
(tests/test_hybrid_filtered.py `_StubNative`), 64 questions, pools of 50, 20 passages to the router, top_k 10.  One JSON line: per call
the median and the best of `--reps` timed calls after one warm-up call, in milliseconds:
  hybrid_search_batch, get_scores_for_router_batch, route_batch (host gate, 64 hidden units), and
  hybrid_search_batch(allowed_ids_each=...) over four made filters (`make_filter`) and unrestricted questions.
What it is for: an A/B of two checkouts of rag_uq_amd/streaming_index.py -- run it alternately on both, compare the medians of the
runs with the spread of one side's runs (profiles/hybrid_seam_ab.txt).

    python tools/hybrid_seam.py [--reps 5] [--label NAME]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rag_uq_amd import streaming_index as si  # noqa: E402
from rag_uq_amd.embedders import RandomProjectionEmbedder  # noqa: E402
import router_scenario as rs  # noqa: E402
import test_hybrid_filtered as th  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
N, NQ, POOL, P, TOP = 5000, 64, 50, 20, 10

rng = np.random.default_rng(11)
docs = [si.Document(id=f"p{i}", text=rs._words(rng, 12, 31), title=f"T{i % 40}") for i in range(N)]
questions = [rs._words(rng, 2, 10) for _ in range(NQ)]
emb = RandomProjectionEmbedder(64)
stub = th._StubNative(emb.embed([d.text for d in docs]), normalize=True)
with tempfile.TemporaryDirectory() as tmp:
    r = rs.retriever(Path(tmp), dense_index=si.DenseIndex.from_native(stub, [d.id for d in docs], embedder=emb, metric="cosine"))
    r.bm25_index.add_documents(docs)
    for d in docs:
        r.documents[d.id] = d
    gate = rs.gate()
    tenants = [r.make_filter([f"p{i}" for i in range(t, N, 4)]) for t in range(4)]
    each = [None if q % 5 == 2 else tenants[q % 4] for q in range(NQ)]
    calls = {
        "hybrid_search_batch": lambda: r.hybrid_search_batch(questions, TOP, POOL),
        "get_scores_for_router_batch": lambda: r.get_scores_for_router_batch(questions, P, retrieval_pool_size=POOL),
        "route_batch": lambda: r.route_batch(questions, gate, TOP, num_passages=P, retrieval_pool_size=POOL),
        "hybrid_search_batch_each": lambda: r.hybrid_search_batch(questions, TOP, POOL, allowed_ids_each=each),
    }
    out = {"label": args.label, "passages": N, "questions": NQ, "pool": POOL, "reps": args.reps, "ms": {}}
    for name, call in calls.items():
        assert sum(len(x) for x in call()) > NQ
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t) * 1e3)
        out["ms"][name] = {"median": round(statistics.median(ms), 3), "best": round(min(ms), 3)}
print(json.dumps(out))
