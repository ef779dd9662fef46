"""ctypes binding of librq_hip.so (C ABI declared in include/rq.h).

This is the only place Python touches the native library.  There is no CPU fallback: if the shared
object is missing or no gfx950 device is visible, construction of an index raises.

Replaces the chromadb client calls of reference rag_uq/streaming_index.py:252-263,326-331,355-359,373.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["RQ_LIB_PATH"]) if os.environ.get("RQ_LIB_PATH") else _PKG_DIR / "librq_hip.so"   # override: A/B of builds

METRIC_COSINE = 0
METRIC_IP = 1
MAX_DIM = 768
MAX_K = 1024
MAX_SCORE_ROWS = 65536
GROUP_NONE = -1


class RqError(RuntimeError):
    """A call into librq_hip.so failed; the message is rq_last_error()."""


class rq_timing(C.Structure):
    _fields_ = [
        ("scan_ms", C.c_double),
        ("scan_launches", C.c_int64),
        ("scan_bytes", C.c_int64),
        ("searches", C.c_int64),
        ("queries", C.c_int64),
        ("widened", C.c_int64),
        ("exact_scans", C.c_int64),
    ]


# name -> (restype, argtypes); must list every symbol include/rq.h declares (tests check this)
_SIGNATURES = {
    "rq_device_count": (C.c_int, []),
    "rq_index_create": (C.c_void_p, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rq_index_destroy": (None, [C.c_void_p]),
    "rq_index_dim": (C.c_int, [C.c_void_p]),
    "rq_index_size": (C.c_int64, [C.c_void_p]),
    "rq_index_set_row_offset": (C.c_int, [C.c_void_p, C.c_int64]),
    "rq_index_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "rq_index_add_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_index_add_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "rq_index_add_f16_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_index_add_f32_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "rq_index_get_rows_f16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rq_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_fixup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_flush_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rq_filter_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_filter_create_device": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rq_filter_count": (C.c_int64, [C.c_void_p]),
    "rq_filter_destroy": (None, [C.c_void_p]),
    "rq_search_filtered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_search_filtered_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_fixup_filtered_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_filtered_each": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_search_filtered_each_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_fixup_filtered_each_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_mmr_select_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "rq_search_mmr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_score_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_score_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "rq_search_range_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_range_fixup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_index_set_groups": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rq_index_get_groups": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "rq_group_collapse_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_grouped_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "rq_search_grouped_fixup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_group_fill_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_group_members_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_group_members_fixup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_search_group_members": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rq_sparse_create": (C.c_void_p, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "rq_sparse_destroy": (None, [C.c_void_p]),
    "rq_sparse_postings": (C.c_int64, [C.c_void_p]),
    "rq_sparse_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_sparse_topk_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_sparse_topk_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_sparse_topk_masked_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_sparse_set_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_sparse_topk_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "rq_sparse_topk_grouped_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_hybrid_set_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_hybrid_fuse_grouped_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 7),
    "rq_hybrid_fuse_grouped": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 6),
    "rq_sparse_score_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_sparse_score_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rq_hybrid_create": (C.c_void_p, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_hybrid_destroy": (None, [C.c_void_p]),
    "rq_hybrid_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "rq_hybrid_missing_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_hybrid_missing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_hybrid_fuse_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 7),
    "rq_hybrid_fuse": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6),
    "rq_router_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    "rq_router_destroy": (None, [C.c_void_p]),
    "rq_router_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "rq_router_gate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rq_router_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rq_router_rerank_device": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "rq_router_rerank": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 7),
    "rq_sparse_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "rq_sparse_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "rq_search_train_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int]),
    "rq_nb_rope_table_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "rq_nb_attention_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rq_nb_add_layernorm_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "rq_nb_swiglu_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "rq_nb_mean_pool_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rq_nb_attention_packed_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rq_nb_mean_pool_packed_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rq_search_hint_next_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rq_stream_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rq_merge_keys_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "rq_debug_pooled": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "rq_debug_bin_records": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "rq_debug_bin_err": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
    "rq_debug_read_bandwidth": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rq_debug_stamps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rq_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "rq_get_option": (C.c_double, [C.c_void_p, C.c_char_p]),
    "rq_get_timing": (C.c_int, [C.c_void_p, C.POINTER(rq_timing)]),
    "rq_reset_timing": (C.c_int, [C.c_void_p]),
    "rq_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rq_load": (C.c_void_p, [C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "rq_last_error": (C.c_char_p, []),
    "rq_version": (C.c_char_p, []),
}

_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen librq_hip.so and declare every entry point.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).
    # Whichever is loaded first serves both, a second copy cannot open the GPU -- so load torch's first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise RqError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {(_PKG_DIR / 'csrc')}`; this backend has no CPU fallback"
        )
    lib = C.CDLL(str(LIB_PATH), mode=getattr(os, "RTLD_NOW", 2) | getattr(os, "RTLD_LOCAL", 0))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load_library().rq_last_error().decode("utf-8", "replace")


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise RqError(f"{what}: {last_error()} (code {rc})")
    return rc


def device_count() -> int:
    return int(load_library().rq_device_count())


def _ptr(a) -> C.c_void_p:
    """Pointer of a numpy array, a torch tensor (host or device) or a raw integer address."""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError(f"cannot take the address of {type(a)!r}")


def pack_row_mask(mask_or_rows, n_rows: int) -> np.ndarray:
    """The bitmap rq_filter_create reads (include/rq.h): bit r % 32 of uint32 word r / 32 set = local row r is allowed.  A boolean
    array of n_rows entries is a mask; anything else is a list of row numbers (out-of-range rows raise, duplicates are harmless)."""
    a = np.asarray(mask_or_rows)
    if a.dtype == np.bool_:
        if a.shape != (int(n_rows),):
            raise ValueError(f"expected a boolean mask of {n_rows} rows, got shape {a.shape}")
        mask = a
    else:
        rows = a.astype(np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
            raise ValueError(f"row numbers outside 0..{int(n_rows) - 1}")
        mask = np.zeros(int(n_rows), dtype=np.bool_)
        mask[rows] = True
    packed = np.packbits(mask, bitorder="little")
    packed = np.concatenate([packed, np.zeros((-packed.size) % 4, np.uint8)])        # whole uint32 words
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32)


def mask_words(n_rows: int) -> int:
    """uint32 words of one row mask over n_rows rows"""
    return (int(n_rows) + 31) // 32


def pack_row_masks(masks_or_rows, n_rows: int) -> np.ndarray:
    """A mask table [n_masks][mask_words(n_rows)] uint32 for the masked sparse calls (include/rq.h rq_sparse_topk_masked,
    include/rq_bm25.h rq_bm25_topk_masked): one `pack_row_mask` per entry -- the layout is the same bitmap."""
    entries = list(masks_or_rows)
    table = np.zeros((len(entries), mask_words(n_rows)), np.uint32)
    for i, e in enumerate(entries):
        table[i] = pack_row_mask(e, n_rows)
    return table


def _mask_args(what: str, masks, mask_of, B: int, n_docs: int) -> Tuple[Optional[np.ndarray], int, np.ndarray]:
    """(masks or None, n_masks, mask_of) of a masked sparse call on host arrays, shapes checked here: the library cannot see them."""
    mask_of = np.ascontiguousarray(mask_of, np.int32)
    if mask_of.shape != (int(B),):
        raise RqError(f"{what}: mask_of needs one entry per query: {B} queries, shape {mask_of.shape}")
    if masks is None:
        return None, 0, mask_of
    masks = np.ascontiguousarray(masks, np.uint32)
    if masks.ndim != 2 or masks.shape[1] != mask_words(n_docs):
        raise RqError(f"{what}: masks must be [n_masks][{mask_words(n_docs)}] uint32 for {n_docs} documents, got shape {masks.shape}")
    return (masks if masks.size else None), masks.shape[0], mask_of


class RowFilter:
    """Owner of one rq_filter: the rows a filtered search may return.  Holds its index (the C object belongs to it: an index that
    was closed first has already freed it, and close() then only forgets the handle)."""

    def __init__(self, index: "NativeIndex", handle: int):
        self._index = index
        self._h = C.c_void_p(handle)
        self.count = int(index._lib.rq_filter_count(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self._index, "_h", None):
                self._index._lib.rq_filter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return self.count


class NativeIndex:
    """Thin owner of one rq_index handle: one row shard on one GPU, or -- `devices=[...]` with more than one entry -- rows
    sharded across several GPUs inside the library (host-buffer calls only, see include/rq.h rq_index_create)."""

    def __init__(self, dim: int, device: int = 0, _handle: Optional[int] = None, devices: Optional[Sequence[int]] = None):
        self._lib = load_library()
        devs = [int(d) for d in devices] if devices else [int(device)]
        if _handle is None:
            ids = (C.c_int * len(devs))(*devs)
            _handle = self._lib.rq_index_create(int(dim), len(devs), ids)
            if not _handle:
                raise RqError(f"rq_index_create(dim={dim}, devices={devs}): {last_error()}")
        self._h = C.c_void_p(_handle)
        self.dim = int(self._lib.rq_index_dim(self._h))
        self.device = devs[0]
        self.devices = devs

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rq_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.rq_index_size(self._h))

    @property
    def row_pad(self) -> int:
        """Elements per stored row: 384 (dim <= 384) or 768 (include/rq.h option "row_pad"; settable with set_option while empty)."""
        return int(self.get_option("row_pad"))

    # -- build ------------------------------------------------------------------------------
    def reserve(self, n_rows: int) -> None:
        _check(self._lib.rq_index_reserve(self._h, int(n_rows)), "rq_index_reserve")

    def set_row_offset(self, off: int) -> None:
        _check(self._lib.rq_index_set_row_offset(self._h, int(off)), "rq_index_set_row_offset")

    def add_f16(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows)
        if rows.dtype == np.float16:
            rows = rows.view(np.uint16)
        if rows.dtype != np.uint16 or rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"expected [n][{self.dim}] float16/uint16 rows, got {rows.dtype} {rows.shape}")
        _check(self._lib.rq_index_add_f16(self._h, _ptr(rows), rows.shape[0]), "rq_index_add_f16")

    def add_f32(self, rows: np.ndarray, normalize: bool = True) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"expected [n][{self.dim}] float32 rows, got {rows.shape}")
        _check(self._lib.rq_index_add_f32(self._h, _ptr(rows), rows.shape[0], int(bool(normalize))), "rq_index_add_f32")

    def add_f16_device(self, d_rows, n_rows: int) -> None:
        _check(self._lib.rq_index_add_f16_device(self._h, _ptr(d_rows), int(n_rows)), "rq_index_add_f16_device")

    def add_f32_device(self, d_rows, n_rows: int, normalize: bool = True) -> None:
        _check(self._lib.rq_index_add_f32_device(self._h, _ptr(d_rows), int(n_rows), int(bool(normalize))),
               "rq_index_add_f32_device")

    def get_rows_f16(self, row_begin: int, n_rows: int) -> np.ndarray:
        out = np.empty((int(n_rows), self.dim), dtype=np.uint16)
        _check(self._lib.rq_index_get_rows_f16(self._h, int(row_begin), int(n_rows), _ptr(out)), "rq_index_get_rows_f16")
        return out.view(np.float16)

    # -- filters ----------------------------------------------------------------------------
    def make_filter(self, mask_or_rows) -> RowFilter:
        """A filter over this index's current rows from a boolean mask [len(self)] or a list of LOCAL row numbers
        (include/rq.h rq_filter_create).  An append makes it stale."""
        bits = pack_row_mask(mask_or_rows, len(self))
        h = self._lib.rq_filter_create(self._h, _ptr(bits) if bits.size else None, len(self))
        if not h:
            raise RqError(f"rq_filter_create: {last_error()}")
        return RowFilter(self, h)

    def _filter_handle(self, row_filter: RowFilter) -> C.c_void_p:
        if not isinstance(row_filter, RowFilter) or not row_filter._h:
            raise ValueError("row_filter must be an open RowFilter (NativeIndex.make_filter)")
        return row_filter._h

    def _opt_filter(self, row_filter: Optional[RowFilter]) -> Optional[C.c_void_p]:
        """The rq_filter argument of a call that takes one or NULL (no restriction)."""
        return None if row_filter is None else self._filter_handle(row_filter)

    # -- checks and outputs the calls below share --------------------------------------------------
    @staticmethod
    def _check_call(B: int, metric: int, *own: Tuple[bool, str]) -> None:
        """B and metric as every call below takes them; `own`: (holds, what to say if not) for the call's own arguments, checked
        between the two."""
        for holds, message in ((1 <= int(B) <= 65535, f"B {B} outside 1..65535"), *own,
                               (int(metric) in (METRIC_COSINE, METRIC_IP), f"unknown metric {metric!r}")):
            if not holds:
                raise ValueError(message)

    @staticmethod
    def _out(*shape: int) -> Tuple[np.ndarray, np.ndarray]:
        """(scores float32, rows int64) of a blocking call, for the library to fill"""
        return np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.int64)

    # -- search -----------------------------------------------------------------------------
    def _as_queries(self, queries: np.ndarray) -> np.ndarray:
        """The queries of a host-buffer call as contiguous float32 [B][dim]; one query may come as a vector."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [B][{self.dim}] float32 queries, got {q.shape}")
        return q

    def search(self, queries: np.ndarray, k: int, metric: int = METRIC_COSINE, *, row_filter: Optional[RowFilter] = None) -> Tuple[np.ndarray, np.ndarray]:
        q = self._as_queries(queries)
        B = q.shape[0]
        scores, rows = self._out(B, int(k))
        if row_filter is not None:
            _check(self._lib.rq_search_filtered(self._h, self._filter_handle(row_filter), _ptr(q), B, int(k), int(metric), _ptr(scores), _ptr(rows)),
                   "rq_search_filtered")
            return scores, rows
        _check(self._lib.rq_search(self._h, _ptr(q), B, int(k), int(metric), _ptr(scores), _ptr(rows)), "rq_search")
        return scores, rows

    def search_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_keys, d_status, stream: int = 0, *,
                      row_filter: Optional[RowFilter] = None) -> None:
        if row_filter is not None:
            _check(self._lib.rq_search_filtered_device(self._h, self._filter_handle(row_filter), _ptr(d_queries), int(B), int(k), int(metric),
                                                       _ptr(d_scores), _ptr(d_rows), _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)),
                   "rq_search_filtered_device")
            return
        _check(self._lib.rq_search_device(self._h, _ptr(d_queries), int(B), int(k), int(metric), _ptr(d_scores), _ptr(d_rows),
                                          _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)), "rq_search_device")

    def search_fixup_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_keys, d_status, stream: int = 0, *,
                            row_filter: Optional[RowFilter] = None) -> int:
        if row_filter is not None:
            return _check(self._lib.rq_search_fixup_filtered_device(self._h, self._filter_handle(row_filter), _ptr(d_queries), int(B), int(k),
                                                                    int(metric), _ptr(d_scores), _ptr(d_rows), _ptr(d_keys), _ptr(d_status),
                                                                    C.c_void_p(stream)), "rq_search_fixup_filtered_device")
        return _check(self._lib.rq_search_fixup_device(self._h, _ptr(d_queries), int(B), int(k), int(metric), _ptr(d_scores),
                                                       _ptr(d_rows), _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)),
                      "rq_search_fixup_device")

    # -- per-query filters (include/rq.h "per-query filters") ------------------------------------------
    def _filter_array(self, filters, B: int):
        """The host array of B rq_filter pointers of an each-call: one open RowFilter or None (unrestricted) per query."""
        filters = list(filters)
        if len(filters) != int(B):
            raise ValueError(f"expected one filter (or None) per query: {B} queries, {len(filters)} filters")
        return (C.c_void_p * int(B))(*[None if f is None else self._filter_handle(f).value for f in filters])

    def search_filtered_each(self, queries: np.ndarray, k: int, filters, metric: int = METRIC_COSINE) -> Tuple[np.ndarray, np.ndarray]:
        """Query q over the rows of filters[q] only (a RowFilter, or None for every row), all in one call
        (include/rq.h rq_search_filtered_each): blocking, host buffers, repair included."""
        q = self._as_queries(queries)
        B = q.shape[0]
        arr = self._filter_array(filters, B)
        scores, rows = self._out(B, int(k))
        _check(self._lib.rq_search_filtered_each(self._h, arr, _ptr(q), B, int(k), int(metric), _ptr(scores), _ptr(rows)), "rq_search_filtered_each")
        return scores, rows

    def search_filtered_each_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_keys, d_status, filters, stream: int = 0) -> None:
        _check(self._lib.rq_search_filtered_each_device(self._h, self._filter_array(filters, B), _ptr(d_queries), int(B), int(k), int(metric),
                                                        _ptr(d_scores), _ptr(d_rows), _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)),
               "rq_search_filtered_each_device")

    def search_filtered_each_fixup_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_keys, d_status, filters, stream: int = 0) -> int:
        return _check(self._lib.rq_search_fixup_filtered_each_device(self._h, self._filter_array(filters, B), _ptr(d_queries), int(B), int(k),
                                                                     int(metric), _ptr(d_scores), _ptr(d_rows), _ptr(d_keys), _ptr(d_status),
                                                                     C.c_void_p(stream)), "rq_search_fixup_filtered_each_device")

    # -- diversified search (include/rq.h "diversified search") --------------------------------------
    @staticmethod
    def _check_mmr(k: int, m: int, lambda_mult: float, what: str) -> None:
        if not (isinstance(lambda_mult, (int, float, np.floating, np.integer)) and 0.0 <= float(lambda_mult) <= 1.0):   # (NaN fails)
            raise ValueError(f"lambda_mult must lie within [0, 1], got {lambda_mult!r}")
        if not 1 <= int(m) <= MAX_K:
            raise ValueError(f"{what} {m} outside 1..{MAX_K}")
        if not 1 <= int(k) <= int(m):
            raise ValueError(f"k {k} outside 1..{what} = {m}")

    def search_mmr(self, queries: np.ndarray, k: int, fetch_k: int, lambda_mult: float = 0.5, metric: int = METRIC_COSINE, *,
                   row_filter: Optional[RowFilter] = None, return_mmr: bool = False):
        """k of the exact top fetch_k rows per query by greedy maximal marginal relevance (include/rq.h rq_search_mmr): (scores, rows)
        in selection order, the scores being the rows' own search scores; return_mmr adds the value v of every pick."""
        self._check_mmr(k, fetch_k, lambda_mult, "fetch_k")
        q = self._as_queries(queries)
        B = q.shape[0]
        scores, rows = self._out(B, int(k))
        mmr = np.empty((B, int(k)), dtype=np.float32) if return_mmr else None
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_search_mmr(self._h, flt, _ptr(q), B, int(k), int(fetch_k), float(lambda_mult), int(metric), _ptr(scores), _ptr(rows),
                                       _ptr(mmr)), "rq_search_mmr")
        return (scores, rows, mmr) if return_mmr else (scores, rows)

    def mmr_select_device(self, d_cand_rows, d_cand_rel, B: int, m: int, k: int, lambda_mult: float, metric: int, d_scores, d_rows, d_mmr=None,
                          stream: int = 0) -> None:
        """Asynchronous selection over a caller's candidates [B][m] in device memory (include/rq.h rq_mmr_select_device)."""
        self._check_mmr(k, m, lambda_mult, "m")
        if int(B) < 1:
            raise ValueError(f"B {B} must be at least 1")
        _check(self._lib.rq_mmr_select_device(self._h, _ptr(d_cand_rows), _ptr(d_cand_rel), int(B), int(m), int(k), float(lambda_mult), int(metric),
                                              _ptr(d_scores), _ptr(d_rows), _ptr(d_mmr), C.c_void_p(stream)), "rq_mmr_select_device")

    # -- scoring given rows (include/rq.h "scoring given rows") ------------------------------------------
    @classmethod
    def _check_score(cls, B: int, m: int, metric: int) -> None:
        cls._check_call(B, metric, (1 <= int(m) <= MAX_SCORE_ROWS, f"m {m} outside 1..{MAX_SCORE_ROWS}"))

    def score_rows(self, queries: np.ndarray, rows: np.ndarray, metric: int = METRIC_COSINE) -> np.ndarray:
        """The exact score of every (query, row) pair of one list of GLOBAL rows per query (include/rq.h rq_score_rows): float32
        [B][m], position for position; an entry outside the index (-1 included) scores 0.0."""
        q = self._as_queries(queries)
        r = np.asarray(rows)
        if r.dtype.kind not in "iu":
            raise ValueError(f"rows must be integers, got {r.dtype}")
        if r.ndim == 1:
            r = r[None, :]
        if r.ndim != 2 or r.shape[0] != q.shape[0]:
            raise ValueError(f"expected [{q.shape[0]}][m] rows, one list per query, got {r.shape}")
        r = np.ascontiguousarray(r, dtype=np.int64)
        B, m = r.shape
        self._check_score(B, m, metric)
        scores = np.empty((B, m), dtype=np.float32)
        _check(self._lib.rq_score_rows(self._h, _ptr(q), B, _ptr(r), m, int(metric), _ptr(scores)), "rq_score_rows")
        return scores

    def score_rows_device(self, d_queries, B: int, d_rows, m: int, metric: int, d_scores, stream: int = 0) -> None:
        """Asynchronous form over device memory: d_queries [B][dim] fp32, d_rows [B][m] int64, d_scores [B][m] fp32 (include/rq.h
        rq_score_rows_device); complete in stream order."""
        self._check_score(B, m, metric)
        _check(self._lib.rq_score_rows_device(self._h, _ptr(d_queries), int(B), _ptr(d_rows), int(m), int(metric), _ptr(d_scores), C.c_void_p(stream)),
               "rq_score_rows_device")

    # -- range searches (include/rq.h "range searches") ---------------------------------------------------
    @classmethod
    def _check_range(cls, B: int, cap: int, metric: int) -> None:
        cls._check_call(B, metric, (1 <= int(cap) <= MAX_K, f"cap {cap} outside 1..{MAX_K}"))

    def search_range(self, queries: np.ndarray, threshold, cap: int, metric: int = METRIC_COSINE, *,
                     row_filter: Optional[RowFilter] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Every row scoring at least `threshold` (a scalar, or one value per query): (scores [B][cap], rows [B][cap], counts [B]).
        counts is exact also beyond cap; the rows are the best min(count, cap) in the canonical order, (0.0, -1) padded
        (include/rq.h rq_search_range)."""
        q = self._as_queries(queries)
        B = q.shape[0]
        self._check_range(B, cap, metric)
        thr = np.asarray(threshold, dtype=np.float32)
        if thr.ndim == 0:
            thr = np.full(B, thr, dtype=np.float32)
        if thr.shape != (B,):
            raise ValueError(f"threshold must be a scalar or [{B}] values, one per query, got {thr.shape}")
        if not np.isfinite(thr).all():
            raise ValueError("every threshold must be finite")
        thr = np.ascontiguousarray(thr)
        scores, rows = self._out(B, int(cap))
        counts = np.empty(B, dtype=np.int64)
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_search_range(self._h, flt, _ptr(q), B, _ptr(thr), int(cap), int(metric), _ptr(scores), _ptr(rows), _ptr(counts)),
               "rq_search_range")
        return scores, rows, counts

    def search_range_device(self, d_queries, B: int, d_thr, cap: int, metric: int, d_scores, d_rows, d_keys, d_count, d_status, stream: int = 0, *,
                            row_filter: Optional[RowFilter] = None) -> None:
        """Asynchronous form over device memory (include/rq.h rq_search_range_device): d_thr [B] fp32, d_count [B] int64, d_status [B]
        int32 (1 = repair that query with search_range_fixup_device); complete in stream order."""
        self._check_range(B, cap, metric)
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_search_range_device(self._h, flt, _ptr(d_queries), int(B), _ptr(d_thr), int(cap), int(metric), _ptr(d_scores), _ptr(d_rows),
                                                _ptr(d_keys), _ptr(d_count), _ptr(d_status), C.c_void_p(stream)), "rq_search_range_device")

    def search_range_fixup_device(self, d_queries, B: int, d_thr, cap: int, metric: int, d_scores, d_rows, d_keys, d_count, d_status, stream: int = 0, *,
                                  row_filter: Optional[RowFilter] = None) -> int:
        self._check_range(B, cap, metric)
        flt = self._opt_filter(row_filter)
        return _check(self._lib.rq_search_range_fixup_device(self._h, flt, _ptr(d_queries), int(B), _ptr(d_thr), int(cap), int(metric), _ptr(d_scores),
                                                             _ptr(d_rows), _ptr(d_keys), _ptr(d_count), _ptr(d_status), C.c_void_p(stream)),
                      "rq_search_range_fixup_device")

    # -- grouped searches (include/rq.h "grouped searches") -----------------------------------------------
    @classmethod
    def _check_grouped(cls, B: int, k: int, m: int, metric: int, what: str = "m") -> None:
        cls._check_call(B, metric, (1 <= int(m) <= MAX_K, f"{what} {m} outside 1..{MAX_K}"), (1 <= int(k) <= int(m), f"k {k} outside 1..{what} = {m}"))

    def set_groups(self, groups, row_begin: int = 0) -> None:
        """Group ids (int32; GROUP_NONE = -1: a group of its own) of the LOCAL rows [row_begin, row_begin + len(groups))
        (include/rq.h rq_index_set_groups).  Blocking; rows appended later are GROUP_NONE."""
        g = np.asarray(groups)
        if g.dtype.kind not in "iu" or g.ndim != 1:
            raise ValueError(f"groups must be a vector of integers, got {g.dtype} {g.shape}")
        if g.size and (int(g.min()) < GROUP_NONE or int(g.max()) > 2 ** 31 - 1):
            raise ValueError(f"group ids must lie within {GROUP_NONE}..2^31 - 1")
        if int(row_begin) < 0:
            raise ValueError(f"row_begin {row_begin} is negative")
        g = np.ascontiguousarray(g, dtype=np.int32)
        _check(self._lib.rq_index_set_groups(self._h, int(row_begin), int(g.size), _ptr(g) if g.size else None), "rq_index_set_groups")

    def get_groups(self, row_begin: int = 0, n_rows: Optional[int] = None) -> np.ndarray:
        if int(row_begin) < 0 or (n_rows is not None and int(n_rows) < 0):
            raise ValueError("row_begin and n_rows must not be negative")
        n = len(self) - int(row_begin) if n_rows is None else int(n_rows)
        out = np.empty(max(n, 0), dtype=np.int32)
        _check(self._lib.rq_index_get_groups(self._h, int(row_begin), n, _ptr(out) if out.size else None), "rq_index_get_groups")
        return out

    def search_grouped(self, queries: np.ndarray, k: int, metric: int = METRIC_COSINE, *, row_filter: Optional[RowFilter] = None
                       ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The best row of each of the k best groups per query (include/rq.h rq_search_grouped): (scores [B][k], rows [B][k],
        groups [B][k]), best group first, (0.0, -1, GROUP_NONE) padded beyond the distinct groups among the rows in play."""
        q = self._as_queries(queries)
        B = q.shape[0]
        self._check_grouped(B, k, MAX_K, metric, "MAX_K")
        flt = self._opt_filter(row_filter)
        scores, rows = self._out(B, int(k))
        groups = np.empty((B, int(k)), dtype=np.int32)
        _check(self._lib.rq_search_grouped(self._h, flt, _ptr(q), B, int(k), int(metric), _ptr(scores), _ptr(rows), _ptr(groups)), "rq_search_grouped")
        return scores, rows, groups

    def search_grouped_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_groups, d_keys, d_status, stream: int = 0, *,
                              row_filter: Optional[RowFilter] = None) -> None:
        """Asynchronous form over device memory (include/rq.h rq_search_grouped_device): d_groups [B][k] int32, d_status [B] int32
        (1 = repair that query with search_grouped_fixup_device); complete in stream order."""
        self._check_grouped(B, k, MAX_K, metric, "MAX_K")
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_search_grouped_device(self._h, flt, _ptr(d_queries), int(B), int(k), int(metric), _ptr(d_scores), _ptr(d_rows), _ptr(d_groups),
                                                  _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)), "rq_search_grouped_device")

    def search_grouped_fixup_device(self, d_queries, B: int, k: int, metric: int, d_scores, d_rows, d_groups, d_keys, d_status, stream: int = 0, *,
                                    row_filter: Optional[RowFilter] = None) -> int:
        self._check_grouped(B, k, MAX_K, metric, "MAX_K")
        flt = self._opt_filter(row_filter)
        return _check(self._lib.rq_search_grouped_fixup_device(self._h, flt, _ptr(d_queries), int(B), int(k), int(metric), _ptr(d_scores), _ptr(d_rows),
                                                               _ptr(d_groups), _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)),
                      "rq_search_grouped_fixup_device")

    def group_collapse_device(self, d_cand_rows, d_cand_scores, d_cand_groups, B: int, m: int, k: int, d_scores, d_rows, d_groups, d_keys, d_status,
                              stream: int = 0) -> None:
        """Asynchronous collapse of a caller's candidates [B][m] in device memory (include/rq.h rq_group_collapse_device);
        d_cand_groups None = the groups are looked up by row in the index."""
        self._check_grouped(B, k, m, METRIC_COSINE)
        _check(self._lib.rq_group_collapse_device(self._h, _ptr(d_cand_rows), _ptr(d_cand_scores), _ptr(d_cand_groups), int(B), int(m), int(k), _ptr(d_scores),
                                                  _ptr(d_rows), _ptr(d_groups), _ptr(d_keys), _ptr(d_status), C.c_void_p(stream)), "rq_group_collapse_device")

    # -- group members (include/rq.h "group members") -----------------------------------------------------
    @classmethod
    def _check_group_members(cls, B: int, k: int, group_size: int, metric: int) -> None:
        fits = int(k) >= 1 and int(group_size) >= 1 and int(k) * int(group_size) <= MAX_K
        cls._check_call(B, metric, (fits, f"k {k} x group_size {group_size} outside 1..{MAX_K}"))

    def search_group_members(self, queries: np.ndarray, k: int, group_size: int, metric: int = METRIC_COSINE, *, row_filter: Optional[RowFilter] = None
                             ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The best `group_size` rows of each of the k best groups per query (include/rq.h rq_search_group_members): (scores [B][k][s],
        rows [B][k][s], groups [B][k], counts [B][k]); members best first, (0.0, -1) padded beyond a slot's count, slots beyond the
        distinct groups among the rows in play are (0.0, -1, GROUP_NONE, 0)."""
        q = self._as_queries(queries)
        B = q.shape[0]
        self._check_group_members(B, k, group_size, metric)
        flt = self._opt_filter(row_filter)
        k, s = int(k), int(group_size)
        scores, rows = self._out(B, k, s)
        groups = np.empty((B, k), dtype=np.int32)
        counts = np.empty((B, k), dtype=np.int32)
        _check(self._lib.rq_search_group_members(self._h, flt, _ptr(q), B, k, s, int(metric), _ptr(scores), _ptr(rows), _ptr(groups), _ptr(counts)),
               "rq_search_group_members")
        return scores, rows, groups, counts

    def search_group_members_device(self, d_queries, B: int, k: int, group_size: int, metric: int, d_scores, d_rows, d_groups, d_count, d_status,
                                    stream: int = 0, *, row_filter: Optional[RowFilter] = None) -> None:
        """Asynchronous form over device memory (include/rq.h rq_search_group_members_device): d_scores / d_rows [B][k][s], d_groups /
        d_count [B][k] int32, d_status [B] int32 (1 = repair that query with search_group_members_fixup_device)."""
        self._check_group_members(B, k, group_size, metric)
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_search_group_members_device(self._h, flt, _ptr(d_queries), int(B), int(k), int(group_size), int(metric), _ptr(d_scores),
                                                        _ptr(d_rows), _ptr(d_groups), _ptr(d_count), _ptr(d_status), C.c_void_p(stream)),
               "rq_search_group_members_device")

    def search_group_members_fixup_device(self, d_queries, B: int, k: int, group_size: int, metric: int, d_scores, d_rows, d_groups, d_count, d_status,
                                          stream: int = 0, *, row_filter: Optional[RowFilter] = None) -> int:
        self._check_group_members(B, k, group_size, metric)
        flt = self._opt_filter(row_filter)
        return _check(self._lib.rq_search_group_members_fixup_device(self._h, flt, _ptr(d_queries), int(B), int(k), int(group_size), int(metric),
                                                                     _ptr(d_scores), _ptr(d_rows), _ptr(d_groups), _ptr(d_count), _ptr(d_status),
                                                                     C.c_void_p(stream)), "rq_search_group_members_fixup_device")

    def group_fill_device(self, d_queries, B: int, k: int, group_size: int, metric: int, d_win_rows, d_win_groups, d_scores, d_rows, d_count, d_status,
                          stream: int = 0, *, row_filter: Optional[RowFilter] = None) -> None:
        """Asynchronous fill over a caller's group slots (include/rq.h rq_group_fill_device): d_win_rows [B][k] int64 global rows,
        d_win_groups [B][k] int32 ids; the best `group_size` members of every slot's group."""
        self._check_group_members(B, k, group_size, metric)
        flt = self._opt_filter(row_filter)
        _check(self._lib.rq_group_fill_device(self._h, flt, _ptr(d_queries), int(B), int(k), int(group_size), int(metric), _ptr(d_win_rows),
                                              _ptr(d_win_groups), _ptr(d_scores), _ptr(d_rows), _ptr(d_count), _ptr(d_status), C.c_void_p(stream)),
               "rq_group_fill_device")

    def search_hint_next_device(self, d_next_queries, B: int, stream: int = 0) -> None:
        """Announce the queries of the NEXT search_device call on `stream` (include/rq.h: rq_search_hint_next_device)."""
        _check(self._lib.rq_search_hint_next_device(self._h, _ptr(d_next_queries), int(B), C.c_void_p(stream)), "rq_search_hint_next_device")

    @staticmethod
    def make_train(d_queries: Sequence, d_scores: Sequence, d_rows: Sequence, d_keys: Optional[Sequence], d_status: Sequence,
                   streams: Sequence[int], d_announce: Optional[Sequence] = None) -> dict:
        """Pointer tables of a train of searches (include/rq.h rq_search_train_device), built once and re-used: batch i = d_queries[i]
        -> d_scores[i] / d_rows[i] / d_keys[i] / d_status[i] on streams[i % len(streams)]; d_announce = the first len(streams)
        batches of the train that follows (announced to the last launches of this one), or None."""
        n, ns = len(d_queries), len(streams)
        ann = list(d_announce) if d_announce is not None else []
        ann = (ann + [None] * ns)[:ns]
        addr = lambda a: 0 if a is None else (_ptr(a).value or 0)
        tab = lambda seq: (C.c_void_p * len(seq))(*[addr(a) for a in seq])
        return {"n": n, "ns": ns, "q": tab(list(d_queries) + ann), "scores": tab(d_scores), "rows": tab(d_rows),
                "keys": tab(d_keys) if d_keys is not None else None, "status": tab(d_status), "streams": (C.c_void_p * ns)(*[int(s) for s in streams]),
                "keep": (d_queries, d_scores, d_rows, d_keys, d_status, ann)}

    def search_train_device(self, train: dict, B: int, k: int, metric: int = METRIC_COSINE) -> None:
        _check(self._lib.rq_search_train_device(self._h, train["n"], train["q"], int(B), int(k), int(metric), train["scores"], train["rows"],
                                                train["keys"], train["status"], train["streams"], train["ns"]), "rq_search_train_device")

    def search_flush_device(self, stream: int = 0) -> None:
        _check(self._lib.rq_search_flush_device(self._h, C.c_void_p(stream)), "rq_search_flush_device")

    def stream_release(self, stream: int = 0) -> None:
        """Drop the search workspace kept for `stream` (call before destroying a stream that was used for searches)."""
        _check(self._lib.rq_stream_release(self._h, C.c_void_p(stream)), "rq_stream_release")

    def debug_pooled(self, query: int, max_bins: int, stream: int = 0) -> np.ndarray:
        out = np.empty((int(max_bins),), dtype=np.float32)
        n = _check(self._lib.rq_debug_pooled(self._h, C.c_void_p(stream), int(query), _ptr(out), int(max_bins)), "rq_debug_pooled")
        return out[:n]

    def debug_bin_records(self, q0: int, nq: int, stream: int = 0) -> np.ndarray:
        """Raw bin records (x, y) of query slots q0 .. q0 + nq of the last search on `stream`: uint32 [nq][bins][2] (include/rq.h)."""
        nbins = (len(self) + 63) // 64
        out = np.empty((int(nq), nbins, 2), dtype=np.uint32)
        n = _check(self._lib.rq_debug_bin_records(self._h, C.c_void_p(stream), int(q0), int(nq), _ptr(out), nbins), "rq_debug_bin_records")
        return out.reshape(-1)[: int(nq) * n * 2].reshape(int(nq), n, 2)   # (rows per slot packed: n bins each)

    def debug_bin_err(self, max_bins: int) -> np.ndarray:
        out = np.empty((int(max_bins),), dtype=np.float32)
        n = _check(self._lib.rq_debug_bin_err(self._h, _ptr(out), int(max_bins)), "rq_debug_bin_err")
        return out[:n]

    def read_bandwidth(self, iters: int = 20, nt: int = -1, wg_per_cu: int = 8) -> float:
        """GB/s of a plain streaming read of the stored shard (measurement yardstick, see include/rq.h)."""
        v = float(self._lib.rq_debug_read_bandwidth(self._h, int(iters), int(nt), int(wg_per_cu)))
        if v < 0:
            raise RqError(f"rq_debug_read_bandwidth: {last_error()}")
        return v

    # -- knobs / timing -----------------------------------------------------------------------
    def set_option(self, name: str, value: float) -> None:
        _check(self._lib.rq_set_option(self._h, name.encode(), float(value)), f"rq_set_option({name})")

    def get_option(self, name: str) -> float:
        return float(self._lib.rq_get_option(self._h, name.encode()))

    def timing(self) -> dict:
        t = rq_timing()
        _check(self._lib.rq_get_timing(self._h, C.byref(t)), "rq_get_timing")
        return {f: getattr(t, f) for f, _ in rq_timing._fields_}

    def reset_timing(self) -> None:
        _check(self._lib.rq_reset_timing(self._h), "rq_reset_timing")

    # -- persistence ------------------------------------------------------------------------
    def save(self, path: str) -> None:
        _check(self._lib.rq_save(self._h, str(path).encode()), "rq_save")

    @classmethod
    def load(cls, path: str, device: int = 0, devices: Optional[Sequence[int]] = None) -> "NativeIndex":
        lib = load_library()
        devs = [int(d) for d in devices] if devices else [int(device)]
        ids = (C.c_int * len(devs))(*devs)
        h = lib.rq_load(str(path).encode(), len(devs), ids)
        if not h:
            raise RqError(f"rq_load({path}): {last_error()}")
        return cls(0, devs[0], _handle=h, devices=devs)


# -- sparse search on the device (include/rq.h "sparse search", csrc/rq_sparse.hip) ----------------------------------------------------
SPARSE_MAX_K = 1024


class SparseIndex:
    """Owner of one rq_sparse handle: a posting index (CSR arrays, COPIED to the device: 12 B per posting + 8 B per token) and the exact
    BM25 top-k over it -- the rows and score bits of `bm25_topk`.  No host fallback: without the library or a gfx950 device the
    constructor raises."""

    def __init__(self, indptr: np.ndarray, rows: np.ndarray, contrib: np.ndarray, n_tokens: int, n_docs: int, device: int = 0):
        self._lib = load_library()
        indptr = np.ascontiguousarray(indptr, np.int64)
        rows = np.ascontiguousarray(rows, np.int32)
        contrib = np.ascontiguousarray(contrib, np.float64)
        if len(indptr) != int(n_tokens) + 1:
            raise RqError(f"rq_sparse_create: indptr holds {len(indptr)} entries for {n_tokens} tokens")
        if len(indptr) and (len(rows) < int(indptr[-1]) or len(contrib) < int(indptr[-1])):
            raise RqError(f"rq_sparse_create: indptr names {int(indptr[-1])} postings, rows / contrib hold {len(rows)} / {len(contrib)}")
        h = self._lib.rq_sparse_create(int(device), _ptr(indptr), _ptr(rows), _ptr(contrib), int(n_tokens), int(n_docs))
        if not h:
            raise RqError(f"rq_sparse_create: {last_error()}")
        self._h = C.c_void_p(h)
        self.n_tokens, self.n_docs, self.device = int(n_tokens), int(n_docs), int(device)
        self.postings = int(self._lib.rq_sparse_postings(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rq_sparse_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def topk(self, q_indptr, q_tokens, B: int, k: int, *, masks=None, mask_of=None) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking, host arrays: (rows int32 [B][k], -1 padded; scores float64 [B][k], 0.0 padded).  With `mask_of` (int32 [B]: the
        mask of each query, -1 = unrestricted) and `masks` ([n_masks][mask_words(n_docs)] uint32, `pack_row_masks`; None when every
        entry is -1) query q is answered over its allowed documents only (rq_sparse_topk_masked)."""
        q_indptr = np.ascontiguousarray(q_indptr, np.int64)
        q_tokens = np.ascontiguousarray(q_tokens, np.int32)
        if len(q_indptr) != int(B) + 1 or (int(B) >= 1 and len(q_tokens) < int(q_indptr[-1])):
            raise RqError(f"rq_sparse_topk: q_indptr holds {len(q_indptr)} entries for {B} queries, or names more tokens than q_tokens holds")
        out_rows = np.empty((max(int(B), 0), max(int(k), 0)), np.int32)
        out_scores = np.empty((max(int(B), 0), max(int(k), 0)), np.float64)
        if masks is not None and mask_of is None:
            raise RqError("rq_sparse_topk_masked: masks without mask_of")
        if mask_of is not None:
            masks, n_masks, mask_of = _mask_args("rq_sparse_topk_masked", masks, mask_of, B, self.n_docs)
            _check(self._lib.rq_sparse_topk_masked(self._h, _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(B), int(k), _ptr(masks), n_masks,
                                                   _ptr(mask_of), _ptr(out_rows), _ptr(out_scores)), "rq_sparse_topk_masked")
            return out_rows, out_scores
        _check(self._lib.rq_sparse_topk(self._h, _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(B), int(k),
                                        _ptr(out_rows), _ptr(out_scores)), "rq_sparse_topk")
        return out_rows, out_scores

    def topk_device(self, d_q_indptr, d_q_tokens, B: int, n_q_tokens: int, k: int, d_rows, d_scores, stream: int = 0, *,
                    d_masks=None, n_masks: int = 0, d_mask_of=None) -> None:
        """Asynchronous, device pointers (torch tensors or raw addresses): int64 [B + 1], int32 [n_q_tokens] -> int32 [B][k], float64 [B][k].
        With `d_mask_of` (int32 [B]) the masked call: `d_masks` uint32 [n_masks][mask_words(n_docs)] (rq_sparse_topk_masked_device)."""
        if d_masks is not None and d_mask_of is None:
            raise RqError("rq_sparse_topk_masked_device: d_masks without d_mask_of")
        if d_mask_of is not None:
            _check(self._lib.rq_sparse_topk_masked_device(self._h, _ptr(d_q_indptr), _ptr(d_q_tokens), int(B), int(n_q_tokens), int(k), _ptr(d_masks),
                                                          int(n_masks), _ptr(d_mask_of), _ptr(d_rows), _ptr(d_scores), C.c_void_p(stream)),
                   "rq_sparse_topk_masked_device")
            return
        _check(self._lib.rq_sparse_topk_device(self._h, _ptr(d_q_indptr), _ptr(d_q_tokens), int(B), int(n_q_tokens), int(k), _ptr(d_rows),
                                               _ptr(d_scores), C.c_void_p(stream)), "rq_sparse_topk_device")

    def set_groups(self, groups) -> None:
        """The group of every document, int32 [n_docs]: -1 (`GROUP_NONE`) = a group of its own, any other value >= 0; COPIED to the
        device, a second call replaces the table (rq_sparse_set_groups)."""
        groups = np.ascontiguousarray(groups, np.int32)
        if groups.shape != (self.n_docs,):
            raise RqError(f"rq_sparse_set_groups: one group id per document: {self.n_docs} documents, shape {groups.shape}")
        _check(self._lib.rq_sparse_set_groups(self._h, _ptr(groups) if self.n_docs else None, self.n_docs), "rq_sparse_set_groups")

    def topk_grouped(self, q_indptr, q_tokens, B: int, k: int, *, masks=None, mask_of=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Blocking, host arrays: `topk` with one document per group of the `set_groups` table -- (rows int32 [B][k], -1 padded; scores
        float64 [B][k], 0.0 padded; count int32 [B]); `masks` / `mask_of` as in `topk` (rq_sparse_topk_grouped)."""
        q_indptr = np.ascontiguousarray(q_indptr, np.int64)
        q_tokens = np.ascontiguousarray(q_tokens, np.int32)
        if len(q_indptr) != int(B) + 1 or (int(B) >= 1 and len(q_tokens) < int(q_indptr[-1])):
            raise RqError(f"rq_sparse_topk_grouped: q_indptr holds {len(q_indptr)} entries for {B} queries, or names more tokens than q_tokens holds")
        out_rows = np.empty((max(int(B), 0), max(int(k), 0)), np.int32)
        out_scores = np.empty((max(int(B), 0), max(int(k), 0)), np.float64)
        out_count = np.empty(max(int(B), 0), np.int32)
        if masks is not None and mask_of is None:
            raise RqError("rq_sparse_topk_grouped: masks without mask_of")
        n_masks = 0
        if mask_of is not None:
            masks, n_masks, mask_of = _mask_args("rq_sparse_topk_grouped", masks, mask_of, B, self.n_docs)
        _check(self._lib.rq_sparse_topk_grouped(self._h, _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(B), int(k), _ptr(masks), n_masks,
                                                _ptr(mask_of), _ptr(out_rows), _ptr(out_scores), _ptr(out_count)), "rq_sparse_topk_grouped")
        return out_rows, out_scores, out_count

    def topk_grouped_device(self, d_q_indptr, d_q_tokens, B: int, n_q_tokens: int, k: int, d_rows, d_scores, d_count, stream: int = 0, *,
                            d_masks=None, n_masks: int = 0, d_mask_of=None) -> None:
        """Asynchronous, device pointers: `topk_device` with one document per group and int32 [B] counts (rq_sparse_topk_grouped_device)."""
        if d_masks is not None and d_mask_of is None:
            raise RqError("rq_sparse_topk_grouped_device: d_masks without d_mask_of")
        _check(self._lib.rq_sparse_topk_grouped_device(self._h, _ptr(d_q_indptr), _ptr(d_q_tokens), int(B), int(n_q_tokens), int(k), _ptr(d_masks), int(n_masks),
                                                       _ptr(d_mask_of), _ptr(d_rows), _ptr(d_scores), _ptr(d_count), C.c_void_p(stream)),
               "rq_sparse_topk_grouped_device")

    def score_rows(self, q_indptr, q_tokens, B: int, rows) -> np.ndarray:
        """Blocking, host arrays: the BM25 score of every (query, row) pair of one list of rows per query, rows int32 [B][m] -> float64
        [B][m] with the bits of a full score vector's entry; a row outside the index (-1 included) scores 0.0 (rq_sparse_score_rows)."""
        q_indptr = np.ascontiguousarray(q_indptr, np.int64)
        q_tokens = np.ascontiguousarray(q_tokens, np.int32)
        rows = np.ascontiguousarray(rows, np.int32)
        if len(q_indptr) != int(B) + 1 or (int(B) >= 1 and len(q_tokens) < int(q_indptr[-1])) or rows.ndim != 2 or rows.shape[0] != int(B):
            raise RqError(f"rq_sparse_score_rows: q_indptr holds {len(q_indptr)} entries and rows has shape {rows.shape} for {B} queries, or q_tokens is short")
        out = np.empty(rows.shape, np.float64)
        _check(self._lib.rq_sparse_score_rows(self._h, _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(B), _ptr(rows), int(rows.shape[1]),
                                              _ptr(out)), "rq_sparse_score_rows")
        return out

    def score_rows_device(self, d_q_indptr, d_q_tokens, B: int, n_q_tokens: int, d_rows, m: int, d_scores, stream: int = 0) -> None:
        """Asynchronous, device pointers: int64 [B + 1], int32 [n_q_tokens], int32 [B][m] -> float64 [B][m]; complete in stream order."""
        _check(self._lib.rq_sparse_score_rows_device(self._h, _ptr(d_q_indptr), _ptr(d_q_tokens), int(B), int(n_q_tokens), _ptr(d_rows), int(m),
                                                     _ptr(d_scores), C.c_void_p(stream)), "rq_sparse_score_rows_device")

    def set_option(self, name: str, value: float) -> None:
        _check(self._lib.rq_sparse_set_option(self._h, name.encode(), float(value)), f"rq_sparse_set_option({name})")

    def get_option(self, name: str) -> float:
        return float(self._lib.rq_sparse_get_option(self._h, name.encode()))


def sparse_available() -> bool:
    """librq_hip.so is built and a device is visible (SparseIndex may still refuse a device that is not a gfx950)."""
    try:
        return device_count() > 0
    except (RqError, OSError):
        return False


# -- hybrid fusion on the device (include/rq.h "hybrid fusion", csrc/rq_hybrid.hip) ------------------------------------------------------
HYBRID_MAX_CAND = 2048


class HybridMap:
    """Owner of one rq_hybrid handle: the key space that joins a sparse and a dense index (dense_key [n_dense] int64, injective; known
    [n_keys] one byte per key; COPIED to the device with the inverse map) and the two calls over a batch of pools: `missing` (the rows
    whose score the other retriever did not give) and `fuse` (the hybrid ranking, bit for bit the host path's).  No host fallback."""

    def __init__(self, nb: int, dense_key: np.ndarray, known: np.ndarray, device: int = 0):
        self._lib = load_library()
        dense_key = np.ascontiguousarray(dense_key, np.int64)
        known = np.ascontiguousarray(np.asarray(known) != 0, np.uint8)
        if dense_key.ndim != 1 or known.ndim != 1:
            raise RqError("rq_hybrid_create: dense_key and known are one-dimensional")
        h = self._lib.rq_hybrid_create(int(device), int(nb), len(dense_key), _ptr(dense_key) if len(dense_key) else None,
                                       _ptr(known) if len(known) else None, len(known))
        if not h:
            raise RqError(f"rq_hybrid_create: {last_error()}")
        self._h = C.c_void_p(h)
        self.nb, self.n_dense, self.n_keys, self.device = int(nb), len(dense_key), len(known), int(device)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rq_hybrid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_option(self, name: str) -> float:
        return float(self._lib.rq_hybrid_get_option(self._h, name.encode()))

    @staticmethod
    def _pools(sp_rows, de_rows) -> Tuple[np.ndarray, np.ndarray]:
        sp_rows = np.ascontiguousarray(sp_rows, np.int32)
        de_rows = np.ascontiguousarray(de_rows, np.int64)
        if sp_rows.ndim != 2 or de_rows.ndim != 2 or sp_rows.shape[0] != de_rows.shape[0]:
            raise RqError(f"hybrid pools are [B][K1] and [B][K2], got {sp_rows.shape} and {de_rows.shape}")
        return sp_rows, de_rows

    def missing(self, sp_rows, de_rows) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking, host arrays: (miss_dense int64 [B][K1], miss_sparse int32 [B][K2]), -1 where nothing is missing."""
        sp_rows, de_rows = self._pools(sp_rows, de_rows)
        B, K1, K2 = sp_rows.shape[0], sp_rows.shape[1], de_rows.shape[1]
        miss_dense, miss_sparse = np.empty((B, K1), np.int64), np.empty((B, K2), np.int32)
        _check(self._lib.rq_hybrid_missing(self._h, _ptr(sp_rows) if K1 else None, _ptr(de_rows) if K2 else None, B, K1, K2,
                                           _ptr(miss_dense) if K1 else None, _ptr(miss_sparse) if K2 else None), "rq_hybrid_missing")
        return miss_dense, miss_sparse

    def missing_device(self, d_sp_rows, d_de_rows, B: int, K1: int, K2: int, d_miss_dense, d_miss_sparse, stream: int = 0) -> None:
        """Asynchronous, device pointers: int32 [B][K1], int64 [B][K2] -> int64 [B][K1], int32 [B][K2]; complete in stream order."""
        _check(self._lib.rq_hybrid_missing_device(self._h, _ptr(d_sp_rows), _ptr(d_de_rows), int(B), int(K1), int(K2), _ptr(d_miss_dense),
                                                  _ptr(d_miss_sparse), C.c_void_p(stream)), "rq_hybrid_missing_device")

    def fuse(self, sp_rows, sp_scores, de_rows, de_scores, top_k: int, *, miss_dense=None, extra_dense=None, miss_sparse=None, extra_sparse=None):
        """Blocking, host arrays: (keys int32, b, d, h float64, positions int32 -- all [B][top_k] -- and count int32 [B])."""
        sp_rows, de_rows = self._pools(sp_rows, de_rows)
        B, K1, K2, k = sp_rows.shape[0], sp_rows.shape[1], de_rows.shape[1], int(top_k)
        sp_scores = np.ascontiguousarray(sp_scores, np.float64)
        de_scores = np.ascontiguousarray(de_scores, np.float32)
        if sp_scores.shape != sp_rows.shape or de_scores.shape != de_rows.shape:
            raise RqError("hybrid pools: scores and rows differ in shape")
        opt = [None if x is None else np.ascontiguousarray(x, t)
               for x, t in ((miss_dense, np.int64), (extra_dense, np.float32), (miss_sparse, np.int32), (extra_sparse, np.float64))]
        for x, shape in zip(opt, (sp_rows.shape, sp_rows.shape, de_rows.shape, de_rows.shape)):
            if x is not None and x.shape != shape:
                raise RqError(f"hybrid fuse: a miss / extra array of shape {x.shape} for a pool of shape {shape}")
        kk = max(k, 0)
        keys, pos, count = np.empty((B, kk), np.int32), np.empty((B, kk), np.int32), np.empty(B, np.int32)
        b, d, h = np.empty((B, kk)), np.empty((B, kk)), np.empty((B, kk))
        _check(self._lib.rq_hybrid_fuse(self._h, _ptr(sp_rows) if K1 else None, _ptr(sp_scores) if K1 else None, _ptr(de_rows) if K2 else None,
                                        _ptr(de_scores) if K2 else None, B, K1, K2, *[_ptr(x) if x is not None and x.size else None for x in opt], k,
                                        _ptr(keys), _ptr(b), _ptr(d), _ptr(h), _ptr(pos), _ptr(count)), "rq_hybrid_fuse")
        return keys, b, d, h, pos, count

    def fuse_device(self, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, B: int, K1: int, K2: int, top_k: int, d_keys, d_b, d_d, d_h, d_pos, d_count,
                    stream: int = 0, *, d_miss_dense=None, d_extra_dense=None, d_miss_sparse=None, d_extra_sparse=None) -> None:
        """Asynchronous, device pointers (include/rq.h rq_hybrid_fuse_device); d_pos and the four miss / extra arrays may be None."""
        _check(self._lib.rq_hybrid_fuse_device(self._h, _ptr(d_sp_rows), _ptr(d_sp_scores), _ptr(d_de_rows), _ptr(d_de_scores), int(B), int(K1), int(K2),
                                               _ptr(d_miss_dense), _ptr(d_extra_dense), _ptr(d_miss_sparse), _ptr(d_extra_sparse), int(top_k), _ptr(d_keys),
                                               _ptr(d_b), _ptr(d_d), _ptr(d_h), _ptr(d_pos), _ptr(d_count), C.c_void_p(stream)), "rq_hybrid_fuse_device")

    def set_groups(self, key_group) -> None:
        """The group of every key, int32 [n_keys]: -1 = a group of its own, any other value >= 0; COPIED to the device, a second call
        replaces the table (rq_hybrid_set_groups)."""
        key_group = np.ascontiguousarray(key_group, np.int32)
        if key_group.shape != (self.n_keys,):
            raise RqError(f"rq_hybrid_set_groups: one group id per key: {self.n_keys} keys, shape {key_group.shape}")
        _check(self._lib.rq_hybrid_set_groups(self._h, _ptr(key_group) if self.n_keys else None, self.n_keys), "rq_hybrid_set_groups")

    def fuse_grouped(self, sp_rows, sp_scores, de_rows, de_scores, top_k: int):
        """Blocking, host arrays: `fuse` with the first candidate of every group of the `set_groups` table only -- the same six arrays."""
        sp_rows, de_rows = self._pools(sp_rows, de_rows)
        B, K1, K2, k = sp_rows.shape[0], sp_rows.shape[1], de_rows.shape[1], int(top_k)
        sp_scores = np.ascontiguousarray(sp_scores, np.float64)
        de_scores = np.ascontiguousarray(de_scores, np.float32)
        if sp_scores.shape != sp_rows.shape or de_scores.shape != de_rows.shape:
            raise RqError("hybrid pools: scores and rows differ in shape")
        kk = max(k, 0)
        keys, pos, count = np.empty((B, kk), np.int32), np.empty((B, kk), np.int32), np.empty(B, np.int32)
        b, d, h = np.empty((B, kk)), np.empty((B, kk)), np.empty((B, kk))
        _check(self._lib.rq_hybrid_fuse_grouped(self._h, _ptr(sp_rows) if K1 else None, _ptr(sp_scores) if K1 else None, _ptr(de_rows) if K2 else None,
                                                _ptr(de_scores) if K2 else None, B, K1, K2, k, _ptr(keys), _ptr(b), _ptr(d), _ptr(h), _ptr(pos), _ptr(count)),
               "rq_hybrid_fuse_grouped")
        return keys, b, d, h, pos, count

    def fuse_grouped_device(self, d_sp_rows, d_sp_scores, d_de_rows, d_de_scores, B: int, K1: int, K2: int, top_k: int, d_keys, d_b, d_d, d_h, d_pos, d_count,
                            stream: int = 0) -> None:
        """Asynchronous, device pointers (include/rq.h rq_hybrid_fuse_grouped_device); d_pos may be None."""
        _check(self._lib.rq_hybrid_fuse_grouped_device(self._h, _ptr(d_sp_rows), _ptr(d_sp_scores), _ptr(d_de_rows), _ptr(d_de_scores), int(B), int(K1), int(K2),
                                                       int(top_k), _ptr(d_keys), _ptr(d_b), _ptr(d_d), _ptr(d_h), _ptr(d_pos), _ptr(d_count), C.c_void_p(stream)),
               "rq_hybrid_fuse_grouped_device")


# -- router gate on the device (include/rq.h "router gate", csrc/rq_router.hip) -----------------------------------------------------------
ROUTER_MAX_HIDDEN = 256
ROUTER_NORM_STATS = 0
ROUTER_NORM_QUERY = 1


class RouterGate:
    """Owner of one rq_router handle: the weights of a RetrievalRouter with one or two layers (w0 [H][3], b0 [H], w1 [H] or [3], b1;
    fp32, COPIED to the device) and the two calls over a batch of fused columns: `gate` (the weight of every slot, in input order) and
    `rerank` (the best top_r candidates by w*d + (1 - w)*b).  `mode` is ROUTER_NORM_QUERY or ROUTER_NORM_STATS, `stats` the four
    doubles (bm25_mean, bm25_std, dense_mean, dense_std) of the latter.  No host fallback."""

    def __init__(self, w0, b0, w1, b1: float, *, num_layers: int = 2, use_batch_norm: bool = False, device: int = 0):
        self._lib = load_library()
        w1 = np.ascontiguousarray(w1, np.float32).reshape(-1)
        hidden = 0
        if int(num_layers) == 2:
            w0 = np.ascontiguousarray(w0, np.float32)
            b0 = np.ascontiguousarray(b0, np.float32).reshape(-1)
            if w0.ndim != 2 or w0.shape[1] != 3 or b0.shape != (w0.shape[0],) or w1.shape != (w0.shape[0],):
                raise RqError(f"rq_router_create: w0 [H][3], b0 [H] and w1 [H], got {w0.shape}, {b0.shape} and {w1.shape}")
            hidden = w0.shape[0]
        elif int(num_layers) == 1:
            if w1.shape != (3,):
                raise RqError(f"rq_router_create: one layer takes w1 [3], got {w1.shape}")
            w0 = b0 = None
        h = self._lib.rq_router_create(int(device), int(num_layers), hidden, int(bool(use_batch_norm)), _ptr(w0) if hidden else None,
                                       _ptr(b0) if hidden else None, _ptr(w1), float(b1))
        if not h:
            raise RqError(f"rq_router_create: {last_error()}")
        self._h = C.c_void_p(h)
        self.hidden, self.layers, self.device = hidden, int(num_layers), int(device)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rq_router_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_option(self, name: str) -> float:
        return float(self._lib.rq_router_get_option(self._h, name.encode()))

    @staticmethod
    def _stats(mode: int, stats) -> Optional[np.ndarray]:
        """The four statistics as the host array the library reads at call time (None: the per-query mode needs none)."""
        if stats is None:
            return None
        stats = np.ascontiguousarray(stats, np.float64)
        if stats.shape != (4,):
            raise RqError(f"router statistics are (bm25_mean, bm25_std, dense_mean, dense_std), got shape {stats.shape}")
        return stats

    @staticmethod
    def _columns(b, d) -> Tuple[np.ndarray, np.ndarray]:
        b, d = np.ascontiguousarray(b, np.float64), np.ascontiguousarray(d, np.float64)
        if b.ndim != 2 or b.shape != d.shape:
            raise RqError(f"router columns are [B][P] twice, got {b.shape} and {d.shape}")
        return b, d

    def gate(self, b, d, mode: int = ROUTER_NORM_QUERY, stats=None) -> np.ndarray:
        """Blocking, host arrays: w float64 [B][P] in input order."""
        b, d = self._columns(b, d)
        stats = self._stats(mode, stats)
        w = np.empty(b.shape, np.float64)
        _check(self._lib.rq_router_gate(self._h, _ptr(b), _ptr(d), b.shape[0], b.shape[1], int(mode), _ptr(stats), _ptr(w)), "rq_router_gate")
        return w

    def gate_device(self, d_b, d_d, B: int, P: int, d_w, mode: int = ROUTER_NORM_QUERY, stats=None, stream: int = 0) -> None:
        """Asynchronous, device pointers: float64 [B][P] twice -> float64 [B][P]; complete in stream order."""
        stats = self._stats(mode, stats)
        _check(self._lib.rq_router_gate_device(self._h, _ptr(d_b), _ptr(d_d), int(B), int(P), int(mode), _ptr(stats), _ptr(d_w), C.c_void_p(stream)),
               "rq_router_gate_device")

    def rerank(self, keys, b, d, count, top_r: int, mode: int = ROUTER_NORM_QUERY, stats=None):
        """Blocking, host arrays: (keys int32, b, d, w, h float64, positions int32 -- all [B][top_r] -- and count int32 [B])."""
        b, d = self._columns(b, d)
        keys, count = np.ascontiguousarray(keys, np.int32), np.ascontiguousarray(count, np.int32)
        if keys.shape != b.shape or count.shape != (b.shape[0],):
            raise RqError(f"router rerank: keys {keys.shape} and count {count.shape} for columns {b.shape}")
        stats = self._stats(mode, stats)
        B, k = b.shape[0], max(int(top_r), 0)
        ok, op, oc = np.empty((B, k), np.int32), np.empty((B, k), np.int32), np.empty(B, np.int32)
        ob, od, ow, oh = np.empty((B, k)), np.empty((B, k)), np.empty((B, k)), np.empty((B, k))
        _check(self._lib.rq_router_rerank(self._h, _ptr(keys), _ptr(b), _ptr(d), _ptr(count), B, b.shape[1], int(mode), _ptr(stats), int(top_r), _ptr(ok),
                                          _ptr(ob), _ptr(od), _ptr(ow), _ptr(oh), _ptr(op), _ptr(oc)), "rq_router_rerank")
        return ok, ob, od, ow, oh, op, oc

    def rerank_device(self, d_keys, d_b, d_d, d_count, B: int, P: int, top_r: int, d_out_keys, d_out_b, d_out_d, d_out_w, d_out_h, d_out_pos, d_out_count,
                      mode: int = ROUTER_NORM_QUERY, stats=None, stream: int = 0) -> None:
        """Asynchronous, device pointers (include/rq.h rq_router_rerank_device); complete in stream order."""
        stats = self._stats(mode, stats)
        _check(self._lib.rq_router_rerank_device(self._h, _ptr(d_keys), _ptr(d_b), _ptr(d_d), _ptr(d_count), int(B), int(P), int(mode), _ptr(stats), int(top_r),
                                                 _ptr(d_out_keys), _ptr(d_out_b), _ptr(d_out_d), _ptr(d_out_w), _ptr(d_out_h), _ptr(d_out_pos), _ptr(d_out_count),
                                                 C.c_void_p(stream)), "rq_router_rerank_device")


# -- encoder pieces (include/rq.h "encoder pieces", csrc/rq_encoder.hip): torch tensors or raw device addresses -------------
def nb_rope_table(rope, seq: int, rope_theta: float, stream: int = 0) -> None:
    _check(load_library().rq_nb_rope_table_f32(_ptr(rope), int(seq), float(rope_theta), C.c_void_p(stream)), "rq_nb_rope_table_f32")


def nb_attention(qkv, lengths, rope, ctx, batch: int, seq: int, heads: int, stream: int = 0) -> None:
    _check(load_library().rq_nb_attention_f16(_ptr(qkv), _ptr(lengths), _ptr(rope), _ptr(ctx), int(batch), int(seq), int(heads),
                                              C.c_void_p(stream)), "rq_nb_attention_f16")


def nb_attention_packed(qkv, offsets, rope, ctx, batch: int, max_seq: int, heads: int, stream: int = 0) -> None:
    _check(load_library().rq_nb_attention_packed_f16(_ptr(qkv), _ptr(offsets), _ptr(rope), _ptr(ctx), int(batch), int(max_seq), int(heads),
                                                     C.c_void_p(stream)), "rq_nb_attention_packed_f16")


def nb_add_layernorm(x, res, gamma, beta, out, rows: int, width: int, eps: float, stream: int = 0) -> None:
    _check(load_library().rq_nb_add_layernorm_f16(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), int(rows), int(width), float(eps),
                                                  C.c_void_p(stream)), "rq_nb_add_layernorm_f16")


def nb_swiglu(gate_up, out, rows: int, inter: int, stream: int = 0) -> None:
    _check(load_library().rq_nb_swiglu_f16(_ptr(gate_up), _ptr(out), int(rows), int(inter), C.c_void_p(stream)), "rq_nb_swiglu_f16")


def nb_mean_pool(h, lengths, out, batch: int, seq: int, width: int, stream: int = 0) -> None:
    _check(load_library().rq_nb_mean_pool_f16(_ptr(h), _ptr(lengths), _ptr(out), int(batch), int(seq), int(width), C.c_void_p(stream)),
           "rq_nb_mean_pool_f16")


def nb_mean_pool_packed(h, offsets, out, batch: int, max_seq: int, width: int, stream: int = 0) -> None:
    _check(load_library().rq_nb_mean_pool_packed_f16(_ptr(h), _ptr(offsets), _ptr(out), int(batch), int(max_seq), int(width), C.c_void_p(stream)),
           "rq_nb_mean_pool_packed_f16")


def merge_keys_device(d_keys_in, n_per_query: int, B: int, k: int, d_scores, d_rows, d_keys_out=None, stream: int = 0) -> None:
    lib = load_library()
    _check(lib.rq_merge_keys_device(_ptr(d_keys_in), int(n_per_query), int(B), int(k), _ptr(d_scores), _ptr(d_rows),
                                    _ptr(d_keys_out), C.c_void_p(stream)), "rq_merge_keys_device")


# -- librq_bm25.so (include/rq_bm25.h, csrc/rq_bm25.cpp): batched CPU BM25 for BM25Index.search_batch -- host cores, no GPU code ----------
BM25_LIB_PATH = _PKG_DIR / "librq_bm25.so"
_BM25_SIGNATURES = {
    "rq_bm25_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "rq_bm25_destroy": (None, [C.c_void_p]),
    "rq_bm25_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "rq_bm25_topk_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int]),
    "rq_bm25_version": (C.c_char_p, []),
}
_bm25_lib: Optional[C.CDLL] = None
_bm25_docs: dict = {}      # handle -> n_docs: the width of a mask table is checked against it (the library cannot see an array's length)


def load_bm25_library() -> C.CDLL:
    global _bm25_lib
    if _bm25_lib is None:
        if not BM25_LIB_PATH.exists():
            raise RqError(f"{BM25_LIB_PATH} is missing: build it with `make -C {(_PKG_DIR / 'csrc')}`")
        lib = C.CDLL(str(BM25_LIB_PATH))
        for name, (res, args) in _BM25_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bm25_lib = lib
    return _bm25_lib


def bm25_available() -> bool:
    try:
        load_bm25_library()
        return True
    except (RqError, OSError):
        return False


def bm25_create(indptr: np.ndarray, rows: np.ndarray, contrib: np.ndarray, n_tokens: int, n_docs: int) -> int:
    """Handle over BORROWED arrays (the caller keeps them alive until bm25_destroy)."""
    assert indptr.dtype == np.int64 and rows.dtype == np.int32 and contrib.dtype == np.float64
    assert indptr.flags.c_contiguous and rows.flags.c_contiguous and contrib.flags.c_contiguous and len(indptr) == n_tokens + 1
    h = load_bm25_library().rq_bm25_create(_ptr(indptr), _ptr(rows), _ptr(contrib), int(n_tokens), int(n_docs))
    if not h:
        raise RqError("rq_bm25_create: malformed posting arrays")
    _bm25_docs[h] = int(n_docs)
    return h


def bm25_destroy(handle: int) -> None:
    _bm25_docs.pop(handle, None)
    if handle and _bm25_lib is not None:
        _bm25_lib.rq_bm25_destroy(C.c_void_p(handle))


def bm25_topk(handle: int, q_indptr: np.ndarray, q_tokens: np.ndarray, n_queries: int, k: int, n_threads: int = 0, *, masks=None,
              mask_of=None) -> Tuple[np.ndarray, np.ndarray]:
    """`mask_of` (int32 [n_queries], -1 = unrestricted) with `masks` ([n_masks][mask_words(n_docs)] uint32; None when every entry is -1)
    answers each query over its allowed documents only (rq_bm25_topk_masked)."""
    out_rows = np.empty((n_queries, k), np.int32)
    out_scores = np.empty((n_queries, k), np.float64)
    q_indptr = np.ascontiguousarray(q_indptr, np.int64)
    q_tokens = np.ascontiguousarray(q_tokens, np.int32)
    if masks is not None and mask_of is None:
        raise RqError("rq_bm25_topk_masked: masks without mask_of")
    if mask_of is not None:
        masks, n_masks, mask_of = _mask_args("rq_bm25_topk_masked", masks, mask_of, n_queries, _bm25_docs[handle])
        rc = load_bm25_library().rq_bm25_topk_masked(C.c_void_p(handle), _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(n_queries), int(k),
                                                     _ptr(masks), n_masks, _ptr(mask_of), _ptr(out_rows), _ptr(out_scores), int(n_threads))
        if rc != 0:
            raise RqError(f"rq_bm25_topk_masked failed (code {rc})")
        return out_rows, out_scores
    rc = load_bm25_library().rq_bm25_topk(C.c_void_p(handle), _ptr(q_indptr), _ptr(q_tokens) if len(q_tokens) else None, int(n_queries), int(k),
                                          _ptr(out_rows), _ptr(out_scores), int(n_threads))
    if rc != 0:
        raise RqError(f"rq_bm25_topk failed (code {rc})")
    return out_rows, out_scores
