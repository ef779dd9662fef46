"""tests/device_twin.py on the CPU (device="cpu"): both routes of the twin return the same bits in every mode, the strided tensor is not
contiguous, the fp16 mode returns fp16 of values that survive the rounding, the counters count, `fail_after` fails from that call on.
tests/test_gpu_device_queries.py relies on each of these."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_twin as dt  # noqa: E402

DIM = 24
RNG = np.random.default_rng(12)
Q = RNG.standard_normal((9, DIM)).astype(np.float32)
Q[4, 3] = 1e-9                                                   # rounds to 0 in fp16
Q[5, 7] = -0.0
X = RNG.standard_normal((31, DIM)).astype(np.float16)
TEXTS = ["q0", "p30", "q8", "q4", "q5", "p0", "q8"]               # a repeat, both tables, first and last rows
WANT = np.stack([Q[0], X[30].astype(np.float32), Q[8], Q[4], Q[5], X[0].astype(np.float32), Q[8]])
MODES = [dict(), dict(dtype="float16"), dict(strided=True), dict(dtype="float16", strided=True)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("source", ["table", "function"])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()) or "plain")
def test_both_routes_return_the_same_bits(mode, source):
    fn = dt.seeded_gaussian(DIM)
    twin = dt.DeviceTwinEmbedder({"q": Q, "p": X} if source == "table" else fn, DIM, "cpu", **mode)
    texts = TEXTS if source == "table" else ["a question", "", "a question", "w1 w2"]
    host = twin.embed(texts)
    dev = twin.embed_device(texts)
    assert host.dtype == np.float32 and host.shape == (len(texts), DIM) == tuple(dev.shape)
    assert dev.dtype == (torch.float16 if mode.get("dtype") == "float16" else torch.float32)
    assert dev.is_contiguous() != bool(mode.get("strided"))
    assert np.array_equal(_bits(host), _bits(dev.float().numpy()))
    assert np.array_equal(_bits(host), _bits(dev.to(torch.float32).contiguous().numpy()))          # what streaming_index.py does with it
    assert np.array_equal(_bits(host), _bits(twin.host_twin().embed(texts)))
    want = WANT if source == "table" else np.stack([fn(t) for t in texts])
    if mode.get("dtype") == "float16":
        assert np.array_equal(_bits(host), _bits(want.astype(np.float16).astype(np.float32))) and not np.array_equal(_bits(host), _bits(want))
        assert np.array_equal(_bits(host), _bits(host.astype(np.float16)))                           # every value is an fp16 value
    else:
        assert np.array_equal(_bits(host), _bits(want))
    if source == "function":
        assert np.array_equal(host[0], host[2]) and not np.array_equal(host[0], host[1])            # per distinct text, seeded
        assert np.array_equal(_bits(host), _bits(dt.DeviceTwinEmbedder(dt.seeded_gaussian(DIM), DIM, **mode).embed(texts)))


def test_counters_and_the_host_twin():
    twin = dt.DeviceTwinEmbedder({"q": Q, "p": X}, DIM, "cpu")
    assert (twin.host_calls, twin.device_calls, twin.device_failures) == (0, 0, 0)
    twin.embed(TEXTS)
    twin.embed(TEXTS[:1])
    assert (twin.host_calls, twin.device_calls) == (2, 0)
    twin.embed_device(TEXTS)
    assert (twin.host_calls, twin.device_calls, twin.device_failures) == (2, 1, 0)
    host = twin.host_twin()
    assert not hasattr(host, "embed_device") and host.dim == DIM
    host.embed(TEXTS)
    assert host.host_calls == 1 and twin.host_calls == 2
    assert tuple(twin.embed_device([]).shape) == (0, DIM) and twin.embed([]).shape == (0, DIM)


@pytest.mark.parametrize("n", [1, 3])
def test_fail_after_raises_from_that_call_on(n):
    twin = dt.DeviceTwinEmbedder({"q": Q}, DIM, "cpu", fail_after=n)
    for _ in range(n - 1):
        twin.embed_device(["q1"])
    for i in range(2):
        with pytest.raises(RuntimeError, match="embed_device fails"):
            twin.embed_device(["q1"])
        assert (twin.device_calls, twin.device_failures) == (n - 1, i + 1)
    assert np.array_equal(twin.embed(["q1"]), Q[1:2]) and twin.host_calls == 1           # the host route still answers


def test_bad_inputs_are_refused():
    with pytest.raises(ValueError):
        dt.DeviceTwinEmbedder({"q": Q}, DIM + 1)
    with pytest.raises(ValueError):
        dt.DeviceTwinEmbedder({"q": Q}, DIM, dtype="bfloat16")
    twin = dt.DeviceTwinEmbedder({"q": Q}, DIM)
    with pytest.raises(KeyError):
        twin.embed(["x3"])
    with pytest.raises(IndexError):
        twin.embed_device(["q9"])
