"""The blocking host-buffer forms on the MI355X (include/rq.h rq_search_filtered, rq_search_mmr; csrc/rq_stage.h): each stages its
buffers, runs the device forms and copies the results back, so what it returns equals, BIT FOR BIT, what a caller gets who
runs the device forms on buffers of their own -- search, repair ladder, (selection) -- as
tests/test_gpu_score_rows.py::test_device_form_equals_the_host_form_bit_for_bit has it for rq_score_rows.  The oracle
comparisons of both forms are tests/test_gpu_filter.py's and tests/test_gpu_mmr.py's."""
import numpy as np
import pytest

from oracle import dense_oracle as orc
from rag_uq_amd import _native as nat

pytestmark = pytest.mark.gpu
COS, IP = nat.METRIC_COSINE, nat.METRIC_IP
B, K, FETCH_K, LAM = 3, 5, 20, 0.5


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _device_search(idx, q, k, metric, flt):
    """rq_search(_filtered)_device, then the repair ladder, on the null stream: device (scores, rows) and the status on the host."""
    import torch
    d_q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    d_s = torch.full((len(q), k), 7.0, dtype=torch.float32, device="cuda")
    d_r = torch.full((len(q), k), 7, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(q),), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.search_device(d_q, len(q), k, metric, d_s, d_r, None, d_st, 0, row_filter=flt)
    idx.search_fixup_device(d_q, len(q), k, metric, d_s, d_r, None, d_st, 0, row_filter=flt)
    torch.cuda.synchronize()
    return d_s, d_r, d_st.cpu().numpy()


@pytest.mark.parametrize("metric", [COS, IP])
@pytest.mark.parametrize("dim", [768, 384])
@pytest.mark.parametrize("n", [70, 4101])                                # two bins / 65 bins, a ragged last bin in both
def test_blocking_forms_equal_their_device_forms_bit_for_bit(n, dim, metric):
    import torch
    x16 = orc.synthetic_corpus(n, dim, seed=n + dim)
    q = orc.synthetic_queries(B, dim, seed=n + dim + 1)
    idx = nat.NativeIndex(dim, 0)
    idx.add_f16(x16)
    flt = idx.make_filter(np.arange(0, n, 3))                            # every third row
    try:
        # ---- rq_search_filtered
        host = idx.search(q, K, metric, row_filter=flt)
        d_s, d_r, st = _device_search(idx, q, K, metric, flt)
        assert not st.any()
        assert np.array_equal(_bits(d_s.cpu().numpy()), _bits(host[0])) and np.array_equal(d_r.cpu().numpy(), host[1]), "filtered"
        assert (host[1] % 3 == 0).all() and (host[1] >= 0).all()
        # ---- rq_search_mmr, without and with the filter: the exact top m, then the selection over it
        for f, in_play in ((None, n), (flt, flt.count)):
            m = max(K, min(FETCH_K, in_play))
            host = idx.search_mmr(q, K, FETCH_K, LAM, metric, row_filter=f, return_mmr=True)
            c_s, c_r, st = _device_search(idx, q, m, metric, f)
            assert not st.any()
            o_s = torch.full((B, K), 7.0, dtype=torch.float32, device="cuda")
            o_r = torch.full((B, K), 7, dtype=torch.int64, device="cuda")
            o_v = torch.full((B, K), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            idx.mmr_select_device(c_r, c_s, B, m, K, LAM, metric, o_s, o_r, o_v, 0)
            torch.cuda.synchronize()
            for name, dev, h in (("scores", o_s, host[0]), ("rows", o_r, host[1]), ("mmr", o_v, host[2])):
                assert np.array_equal(_bits(dev.cpu().numpy()), _bits(h)), f"MMR {'filtered' if f else 'unfiltered'}: {name}"
            assert (host[1] >= 0).all() and (f is None or (host[1] % 3 == 0).all())
    finally:
        flt.close()
        idx.close()
