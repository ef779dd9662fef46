"""Drop-in check against the reference's own consumers, as captured in tests/golden/g7_dropin.json.  The consumers of the hot
path -- `RetrievalRouter.hybrid_rerank` (rag_uq/router.py:179-202, used by experiments/run_evaluation.py:170-184),
`RAGEvaluator` (rag_uq/eval_protocol.py) and the reference's own `HybridRetriever.hybrid_search` (streaming_index.py:464-521) --
were run UNCHANGED by tests/golden/make_golden.py on what this package returns for the scenarios below.  The tests pin that this
package still returns exactly those inputs, and that the recorded consumer outputs follow from them (router restatement pinned by
g2_router.json, recall restatements pinned by g3_retrieval_metrics.json)."""
import json
import os

import numpy as np
import pytest


class FakeDense:
    """Stands in for DenseIndex on a GPU-less machine: same duck type (search/add_documents/__len__)."""
    def __init__(self):
        self.docs = {}

    def add_documents(self, documents, batch_size=100):
        new = [d for d in documents if d.id not in self.docs]
        self.docs.update({d.id: d for d in new})
        return len(new)

    def search(self, query, top_k=10):
        toks = set(query.lower().split())
        scored = sorted(((len(toks & set(d.text.lower().split())) / (1 + len(toks)), i) for i, d in self.docs.items()), reverse=True)
        return [(i, s, self.docs[i].text) for s, i in scored[:top_k]]

    def __len__(self):
        return len(self.docs) or 1


CORPUS = [(f"d{i}", t) for i, t in enumerate([
    "the sky is blue on a clear day", "grass is green in the spring", "the sun is a bright star", "blue whales swim in the sea",
    "stars shine in the night sky", "rain makes the green grass grow", "a star is born in a nebula", "the sea is deep and blue",
    "night follows day", "clear water in a mountain lake", "mountains rise above the clouds", "clouds bring rain to the valley"])]
QUESTIONS = [("what color is the sky", "d0"), ("where do blue whales swim", "d3"), ("what makes grass grow", "d5")]
QUERIES = ["blue sea", "green grass rain", "night sky stars"]


def positive(results):
    """entries tied at hybrid 0.0 are cut at top_k in set-iteration order (reference :489,:521): compare the rest"""
    key = lambda r: (-(r.hybrid_score or 0), r.doc_id)
    return [[x.doc_id, x.bm25_score, x.dense_score, x.hybrid_score] for x in sorted(results, key=key) if x.hybrid_score > 0]


@pytest.fixture(scope="module")
def g7(golden_dir):
    with open(os.path.join(golden_dir, "g7_dropin.json")) as f:
        return json.load(f)


def test_unchanged_router_and_evaluator_consume_our_retriever(g7, golden_dir, tmp_path):
    from oracle import dense_oracle as orc
    from oracle import router_oracle as ro
    from rag_uq_amd import streaming_index as si
    g = g7["router"]
    assert [(c["question"], c["answer_doc"]) for c in g["questions"]] == QUESTIONS
    r = si.HybridRetriever(bm25_persist_path=str(tmp_path / "b.pkl"), chroma_persist_path=str(tmp_path / "c"), dense_index=FakeDense())
    r.add_documents([si.Document(id=i, text=t) for i, t in CORPUS])
    with open(os.path.join(golden_dir, "g2_router.json")) as f:
        model = ro.RouterOracle(json.load(f)["state_dict"])       # the reference's RetrievalRouter(RouterConfig()) after torch.manual_seed(0)
    retrieved, gold = [], []
    for c in g["questions"]:
        bm25, dense, ids, texts = r.get_scores_for_router(c["question"], num_passages=g["num_passages"])     # run_evaluation.py:165-167
        assert len(bm25) == len(dense) == len(ids) == len(texts) == g["num_passages"]
        # exactly what the reference's router and evaluator consumed when the fixture was captured
        assert [list(bm25), list(dense), list(ids), list(texts)] == [c["bm25"], c["dense"], c["ids"], c["texts"]]
        scores, order = model.hybrid_rerank([bm25], [dense], top_k=g["top_k"])                                 # run_evaluation.py:170-173
        hyb = model.hybrid_scores([bm25], [dense])[0]
        # the reference's torch.topk order, up to the order inside a group of exactly tied hybrid scores (the zero padding)
        assert all(m == t or hyb[m] == hyb[t] for m, t in zip(order[0].tolist(), c["rerank_indices"]))
        np.testing.assert_allclose(scores[0], np.asarray(c["rerank_scores"], np.float32), rtol=2e-6, atol=2e-6)
        retrieved.append([ids[i] for i in c["rerank_indices"] if ids[i]])
        gold.append([c["answer_doc"]])
        assert retrieved[-1] == c["retrieved"]
        assert ro.recall_at_k(retrieved[-1], gold[-1], g["top_k"]) == pytest.approx(c["recall_at_5"])      # RAGEvaluator._recall_at_k
    rec = float(np.mean([c["recall_at_5"] for c in g["questions"]]))
    assert 0.0 <= rec <= 1.0 and rec == pytest.approx(g["recall_at_5"])
    # identical to the oracle-side restatement of the metric
    ids_all = {d: i for i, (d, _) in enumerate(CORPUS)}
    found = np.full((len(retrieved), g["top_k"]), -1, dtype=np.int64)
    for b, lst in enumerate(retrieved):
        for j, d in enumerate(lst[:g["top_k"]]):
            found[b, j] = ids_all[d]
    assert orc.recall_at_k(found, np.array([[ids_all[x[0]]] for x in gold])) == pytest.approx(rec)


def test_reference_hybrid_retriever_accepts_our_indexes(g7, tmp_path):
    """INTEGRATION.md option B: the reference's HybridRetriever with this package's BM25Index + a dense index object.  It calls
    `bm25_index.search(query, pool)` (streaming_index.py:451-455) and fuses; this package's BM25Index must still answer those calls
    with what the reference consumed, and this package's own HybridRetriever must fuse to the reference's output."""
    from rag_uq_amd import streaming_index as si
    g = g7["hybrid"]
    assert [c["query"] for c in g["queries"]] == QUERIES
    bm = si.BM25Index()
    bm.add_documents([si.Document(id=i, text=t) for i, t in CORPUS])
    ours = si.HybridRetriever(bm25_persist_path=str(tmp_path / "y.pkl"), chroma_persist_path=str(tmp_path / "c2"), dense_index=FakeDense())
    ours.add_documents([si.Document(id=i, text=t) for i, t in CORPUS])
    for c in g["queries"]:
        assert [[d, s] for d, s in bm.search(c["query"], g["pool"])] == c["bm25_search"]
        pos = positive(ours.hybrid_search(c["query"], top_k=g["top_k"], retrieval_pool_size=g["pool"]))
        assert pos == c["positive"] and len(pos) >= 2
