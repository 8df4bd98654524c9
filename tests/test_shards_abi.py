"""Shard-set C-ABI surface (CPU-side): the symbols exist and are bound,
sptag_amd_shards_create refuses what include/sptag_amd.h says it refuses,
and without a HIP device the set's search, its truth and the merge utility
fail with SPTAG_AMD_ERR_NOGPU as the single-index search does. Handles come
from tiny arrays, as in test_abi.py; none of this needs a GPU."""
import ctypes

import numpy as np
import pytest

import sptag_amd
from sptag_amd import AnnIndex, ShardedIndex, SptagAmdError

SYMBOLS = ["sptag_amd_merge_topk", "sptag_amd_merge_topk_device",
           "sptag_amd_shards_create", "sptag_amd_shards_free",
           "sptag_amd_shards_search_batch",
           "sptag_amd_shards_search_batch_device", "sptag_amd_shards_truth",
           "sptag_amd_shards_count", "sptag_amd_shards_num_vectors"]
ERR_PARAM, ERR_NOGPU = -2, -3
INT32_MAX = 2 ** 31 - 1


def _tiny(n=4, dim=4, dtype=np.float32, dm="L2", algo="bkt"):
    """An index handle that loads anywhere: zero vectors, empty graph rows."""
    vectors = np.zeros((n, dim), dtype=dtype)
    tree_start = np.zeros(1, dtype=np.int32)
    graph = np.full((n, 2), -1, dtype=np.int32)
    if algo == "kdt":
        return AnnIndex.FromArraysKDT(vectors, tree_start,
                                      np.zeros((2, 4), dtype=np.int32), graph, dm)
    return AnnIndex.FromArrays(vectors, tree_start,
                               np.zeros((2, 3), dtype=np.int32), graph, dm)


def _create(indexes, vid_base=None, nshards=None):
    """Raw sptag_amd_shards_create; `indexes` may hold None for a NULL entry."""
    lib = sptag_amd.load_library()
    arr = (ctypes.c_void_p * max(len(indexes), 1))(
        *[ix._h if ix is not None else None for ix in indexes])
    basep = None
    if vid_base is not None:
        vid_base = np.asarray(vid_base, dtype=np.int32)
        basep = vid_base.ctypes.data_as(ctypes.c_void_p)
    return lib.sptag_amd_shards_create(
        arr, len(indexes) if nshards is None else nshards, basep)


def test_symbols_exported_and_bound():
    lib = sptag_amd.load_library()
    for s in SYMBOLS:
        fn = getattr(lib, s, None)
        assert fn is not None, f"missing export {s}"
        if s != "sptag_amd_shards_free":
            assert fn.argtypes, f"{s} has no argtypes bound"
    assert lib.sptag_amd_shards_create.restype is ctypes.c_void_p
    assert lib.sptag_amd_shards_num_vectors.restype is ctypes.c_int64
    assert lib.sptag_amd_shards_free.argtypes == [ctypes.c_void_p]
    for name in ("ShardedIndex", "merge_topk"):
        assert name in sptag_amd.__all__ and hasattr(sptag_amd, name)


def test_create_counts_and_default_bases():
    a, b, c = _tiny(n=4), _tiny(n=7, algo="kdt"), _tiny(n=2)
    sh = ShardedIndex.FromIndexes([a, b, c])
    assert sh.NumShards() == 3
    assert sh.NumVectors() == 13
    assert sh.shards == [a, b, c]      # references kept: shards outlive the set
    one = ShardedIndex.FromIndexes([a])
    assert one.NumShards() == 1 and one.NumVectors() == 4
    lib = sptag_amd.load_library()
    assert lib.sptag_amd_shards_count(None) == -1
    assert lib.sptag_amd_shards_num_vectors(None) == -1
    lib.sptag_amd_shards_free(None)    # a no-op, like free_index(NULL)


def test_create_rejects_bad_shard_counts():
    ix = _tiny()
    assert _create([ix], nshards=0) is None
    assert _create([ix] * 65) is None
    h = _create([ix] * 64)             # 64 is the most a set holds
    assert h is not None
    sptag_amd.load_library().sptag_amd_shards_free(h)
    assert sptag_amd.load_library().sptag_amd_shards_create(None, 1, None) is None


def test_create_rejects_null_entry():
    ix = _tiny()
    assert _create([ix, None, ix]) is None
    assert _create([None]) is None


def test_create_rejects_mismatched_shards():
    base = _tiny(dim=4)
    assert _create([base, _tiny(dim=8)]) is None
    assert _create([base, _tiny(dtype=np.int8)]) is None
    assert _create([base, _tiny(dm="Cosine")]) is None
    with pytest.raises(SptagAmdError):
        ShardedIndex.FromIndexes([base, _tiny(dim=8)])


def test_create_rejects_int32_overflow():
    a, b = _tiny(n=4), _tiny(n=4)
    # base + n == 2^31 - 1 is the last sum that fits
    h = _create([a, b], [0, INT32_MAX - 4])
    assert h is not None
    sptag_amd.load_library().sptag_amd_shards_free(h)
    assert _create([a, b], [0, INT32_MAX - 3]) is None
    assert _create([a, b], [INT32_MAX - 3, 0]) is None
    assert _create([a, b], [0, -1]) is None


def test_search_arguments_checked():
    lib = sptag_amd.load_library()
    sh = ShardedIndex.FromIndexes([_tiny(), _tiny()])
    q = np.zeros((2, 4), dtype=np.float32)
    v = np.zeros((2, 10), dtype=np.int32)
    d = np.zeros((2, 10), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for fn in (lib.sptag_amd_shards_search_batch,
               lib.sptag_amd_shards_search_batch_device):
        assert fn(None, p(q), 2, 10, 0, p(v), p(d)) == ERR_PARAM
        assert fn(sh._h, None, 2, 10, 0, p(v), p(d)) == ERR_PARAM
        assert fn(sh._h, p(q), 0, 10, 0, p(v), p(d)) == ERR_PARAM
        assert fn(sh._h, p(q), 2, 0, 0, p(v), p(d)) == ERR_PARAM
        assert fn(sh._h, p(q), 2, 1025, 0, p(v), p(d)) == ERR_PARAM
    assert lib.sptag_amd_shards_truth(None, p(q), 2, 10, p(v), p(d)) == ERR_PARAM
    # merge: S, k_in and k_out ranges, null pointers, negative base
    lv = np.zeros((2, 2, 10), dtype=np.int32)
    ld = np.zeros((2, 2, 10), dtype=np.float32)
    base = np.zeros(2, dtype=np.int32)
    neg = np.array([0, -5], dtype=np.int32)
    m = lib.sptag_amd_merge_topk
    assert m(0, 0, 2, 10, 10, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 65, 2, 10, 10, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 0, 10, 10, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 0, 10, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 1025, 10, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 10, 0, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 10, 1025, p(lv), p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 10, 10, None, p(ld), p(base), p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 10, 10, p(lv), p(ld), None, p(v), p(d)) == ERR_PARAM
    assert m(0, 2, 2, 10, 10, p(lv), p(ld), p(neg), p(v), p(d)) == ERR_PARAM


def test_search_fails_loudly_without_gpu():
    if sptag_amd.gpu_available():
        pytest.skip("GPU present; loud-failure path not reachable")
    sh = ShardedIndex.FromIndexes([_tiny(), _tiny()])
    q = np.zeros((2, 4), dtype=np.float32)
    keep_v = np.full((2, 3), 77, dtype=np.int32)
    keep_d = np.full((2, 3), 5.0, dtype=np.float32)
    v, d = keep_v.copy(), keep_d.copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = sptag_amd.load_library().sptag_amd_shards_search_batch(
        sh._h, p(q), 2, 3, 0, p(v), p(d))
    assert rc == ERR_NOGPU
    np.testing.assert_array_equal(v, keep_v)    # outputs left untouched
    np.testing.assert_array_equal(d, keep_d)
    for call in (lambda: sh.BatchSearch(q, 3), lambda: sh.Truth(q, 3),
                 lambda: sptag_amd.merge_topk(np.zeros((2, 2, 3), np.int32),
                                              np.zeros((2, 2, 3), np.float32),
                                              [0, 10], 3)):
        with pytest.raises(SptagAmdError) as e:
            call()
        assert e.value.code == ERR_NOGPU
