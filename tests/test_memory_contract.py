"""Every device-form method of rag_uq_amd._native that takes an output pointer has a case in tests/test_gpu_memory_contract.py: the
methods are listed by introspection, so a route added later cannot skip the memory contract (include/rq.h "Caller buffers")."""
import inspect
import os
import re
import sys

from rag_uq_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_memory_contract as contract  # noqa: E402

CLASSES = (nat.NativeIndex, nat.SparseIndex, nat.HybridMap, nat.RouterGate)
NO_OUTPUTS = re.compile(r"^(add_\w+|search_hint_next|search_train|search_flush)_device$")        # the append, hint, train and flush calls


def device_forms():
    return sorted(f"{cls.__name__}.{name}" for cls in CLASSES for name, fn in vars(cls).items()
                  if name.endswith("_device") and inspect.isfunction(fn) and not NO_OUTPUTS.match(name))


def test_the_introspection_finds_the_routes_the_issue_names():
    forms = device_forms()
    for known in ("NativeIndex.search_device", "NativeIndex.search_filtered_each_fixup_device", "NativeIndex.group_fill_device", "SparseIndex.score_rows_device",
                  "HybridMap.fuse_grouped_device", "RouterGate.rerank_device"):
        assert known in forms
    assert not [f for f in forms if "add_" in f or "hint" in f or "train" in f or "flush" in f]


def test_the_header_states_the_contract():
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rq.h")).read()
    doc = h[h.index("Caller buffers"):h.index("Score definition")]
    for word in ("natural alignment of the element type", "4 bytes for float", "8 bytes for double", "view into a larger array", "one element wide",
                 "exactly the extents", "no row of a pad slot", "Every slot of every output array is written", "-1, 0.0, key 0", "d_status included",
                 "NULL is skipped", "flagged queries only", "are never written", "RQ_EINVAL has written none of its outputs",
                 '"pipeline" 1 and 2', "bundles", "belong to the library", "the call that completes them", "flush", "release", "each call's own [B][k]",
                 "tests/test_gpu_memory_contract.py"):
        assert word in doc, f"include/rq.h \"Caller buffers\" no longer says: {word}"


def test_every_device_form_has_a_case_in_the_memory_contract():
    source = inspect.getsource(contract)
    for form in device_forms():
        tests = contract.COVERED.get(form, [])
        assert tests, f"{form} has no case in tests/test_gpu_memory_contract.py"
        method = form.split(".")[1]
        for t in tests:
            assert f".{method}(" in inspect.getsource(getattr(contract, t)), f"{t} claims to cover {form} and never calls it"
        assert f".{method}(" in source
    assert not set(contract.COVERED) - set(device_forms()), "a covered name is not a device form of _native"
    guarded_tests = {t for ts in contract.COVERED.values() for t in ts}
    for t in guarded_tests:                                  # every such test goes through the harness
        src = inspect.getsource(getattr(contract, t))
        assert ".check(" in src or "refused(" in src, t
