"""Global rows with bit 31 set, on the host: keys carry the global row in 32 bits (csrc/rq_device.h rq_make_key, distributed.py
pack_keys), and rq_index_set_row_offset accepts any offset with row_offset + rows < 2^32 - 1, so a row may be anything up to
2^32 - 2.  The host codec must pack, unpack, order and merge such rows exactly as it does small ones: a signed 32-bit slip would turn
row 2^31 into a negative number or order it before row 2^31 - 1.  The device side is tests/test_gpu_high_rows.py."""
import numpy as np
import pytest

from rag_uq_amd import distributed as dist

HALF = 2 ** 31
TOP = 2 ** 32 - 2                          # the largest row a key can carry: 2^32 - 1 is reserved
HIGH_ROWS = [HALF - 1, HALF, TOP]


def test_pack_and_unpack_round_trip_rows_around_bit_31():
    rows = np.array([0, 1, HALF - 2, HALF - 1, HALF, HALF + 1, TOP - 1, TOP, -1], np.int64)
    scores = np.array([0.5, -0.5, np.inf, -np.inf, 0.0, -0.0, 1e36, -1e-40, 3.0], np.float32)
    keys = dist.pack_keys(scores, rows)
    assert keys.dtype == np.uint64 and keys[-1] == 0                      # an empty entry is key 0, whatever its score
    assert len(set(keys[:-1].tolist())) == 8
    s, r = dist.unpack_keys(keys)
    assert r.dtype == np.int64 and r.tolist() == rows.tolist()
    want = scores.copy()
    want[5] = 0.0                                                         # -0.0 leaves as +0.0
    want[8] = 0.0                                                         # the empty entry
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32))
    assert (keys[:-1] & np.uint64(0xFFFFFFFF)).tolist() == [0xFFFFFFFF - x for x in rows[:-1].tolist()]      # the row field, spelled out


def test_equal_scores_order_by_row_ascending_across_bit_31():
    rows = np.array([TOP, HALF, 7, HALF - 1, HALF + 1, 0], np.int64)
    for score in (0.25, 0.0, -3.0, np.inf, -np.inf):
        keys = dist.pack_keys(np.full(rows.size, score, np.float32), rows)
        order = np.argsort(keys)[::-1]                                    # a larger key is a better entry
        assert rows[order].tolist() == sorted(rows.tolist()), score
    # ... and the score still decides first: a better score at a high row beats a worse one at a low row, and the reverse
    keys = dist.pack_keys(np.array([0.5, 0.75, 0.75, 0.25], np.float32), np.array([3, TOP, HALF, 0], np.int64))
    assert np.argsort(keys)[::-1].tolist() == [2, 1, 0, 3]


def test_merge_keys_host_with_high_rows():
    rng = np.random.default_rng(31)
    B, n, k = 5, 24, 10
    rows = np.stack([rng.permutation(np.concatenate([HIGH_ROWS, [HALF - 2, HALF + 1, TOP - 1], np.arange(n - 6) * 1000 + 5])) for _ in range(B)]).astype(np.int64)
    scores = rng.standard_normal((B, n)).astype(np.float32)
    scores[:, :12] = np.float32(0.5)                                      # a tie run of 12 entries per query, high and low rows among them
    scores[0, 12:15] = np.inf
    scores[1, 12:15] = -np.inf
    rows[2, 20:] = -1                                                     # empty entries
    keys = dist.pack_keys(scores, rows)
    got_s, got_r = dist.merge_keys_host(keys, k)
    for b in range(B):
        ok = np.flatnonzero(rows[b] >= 0)
        order = ok[np.lexsort((rows[b, ok], -scores[b, ok].astype(np.float64)))][:k]
        assert got_r[b].tolist() == rows[b, order].tolist(), b
        assert np.array_equal(got_s[b].view(np.uint32), scores[b, order].view(np.uint32)), b
    assert (got_r >= HALF).any() and (got_r[got_r >= 0] < HALF).any()
    # merging the merged halves gives the merge of the whole (what a two-level reduction over shards relies on)
    left, right = dist.merge_keys_host(keys[:, :n // 2], k), dist.merge_keys_host(keys[:, n // 2:], k)
    again = dist.merge_keys_host(np.concatenate([dist.pack_keys(*left), dist.pack_keys(*right)], axis=1), k)
    assert np.array_equal(again[1], got_r) and np.array_equal(again[0].view(np.uint32), got_s.view(np.uint32))
    # more asked for than there is: padding (0.0, -1)
    s, r = dist.merge_keys_host(dist.pack_keys(np.ones((1, 3), np.float32), np.array([HIGH_ROWS], np.int64)), 5)
    assert r.tolist() == [HIGH_ROWS + [-1, -1]] and s.tolist() == [[1.0, 1.0, 1.0, 0.0, 0.0]]


def test_the_reserved_row_is_refused():
    for rows in ([2 ** 32 - 1], [0, 2 ** 32 - 1, 5], [2 ** 32], [2 ** 40]):
        with pytest.raises(ValueError):
            dist.pack_keys(np.zeros(len(rows), np.float32), np.array(rows, np.int64))
    assert dist.pack_keys(np.zeros(1, np.float32), np.array([TOP], np.int64))[0] == (np.uint64(0x80000000) << np.uint64(32)) | np.uint64(1)
