"""sptag_amd — MI355X-native SPTAG search backend (Python host mirror).

This module mirrors the reference Python wrapper's ``AnnIndex`` facade
(reference Wrappers/inc/CoreInterface.h:14: Load:72, Search:45,
BatchSearch:49) over the C-ABI in include/sptag_amd.h. Host logic lives in
the C++ library (sptag_amd/libsptag_amd.so); this wrapper only marshals
numpy arrays across the C boundary.

THE GPU IS THE PRODUCT PATH: importing works anywhere (so CPU-side tests can
check symbol exports), but every search raises loudly when the HIP device or
the extension is missing. There is no CPU fallback in this package.
"""
import ctypes
import os

import numpy as np

__all__ = ["AnnIndex", "ShardedIndex", "merge_topk", "group_knn_device",
           "group_knn_sort_max", "rng_prune_device", "pool_join_device", "kmeans_assign_device",
           "tpt_partition_device",
           "MetadataSet", "load_library", "gpu_available", "SptagAmdError"]

_LIB = None
_LIBPATH = os.environ.get(
    "SPTAG_AMD_LIB",
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsptag_amd.so"))

VT_FLOAT, VT_INT8 = 0, 1
DM_L2, DM_COSINE = 0, 1

_ERRNAMES = {
    0: "OK", -1: "IO", -2: "PARAM", -3: "NOGPU", -4: "UNSUPPORTED",
    -5: "OOM", -6: "INTERNAL",
}


class SptagAmdError(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__(f"sptag_amd error {_ERRNAMES.get(code, code)} {what}")
        self.code = code


def load_library():
    """Load libsptag_amd.so; raises if the extension was not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIBPATH):
        raise SptagAmdError(
            -6, f"HIP extension missing: {_LIBPATH} — build it with "
                "`make -C sptag_amd/csrc` (or __graft_entry__.build()); "
                "this package has no CPU fallback")
    lib = ctypes.CDLL(_LIBPATH)
    lib.sptag_amd_load_index.restype = ctypes.c_void_p
    lib.sptag_amd_load_index.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.sptag_amd_create_index.restype = ctypes.c_void_p
    lib.sptag_amd_create_index.argtypes = [
        ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int]
    lib.sptag_amd_create_index_kdt.restype = ctypes.c_void_p
    lib.sptag_amd_create_index_kdt.argtypes = lib.sptag_amd_create_index.argtypes
    lib.sptag_amd_free_index.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_search_batch.restype = ctypes.c_int
    lib.sptag_amd_search_batch.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.sptag_amd_search_batch_device.restype = ctypes.c_int
    lib.sptag_amd_search_batch_device.argtypes = lib.sptag_amd_search_batch.argtypes
    lib.sptag_amd_last_stats.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    lib.sptag_amd_truth.restype = ctypes.c_int
    lib.sptag_amd_truth.argtypes = lib.sptag_amd_search_batch.argtypes[:4] + [
        ctypes.c_void_p, ctypes.c_void_p]
    lib.sptag_amd_exact_search.restype = ctypes.c_int
    lib.sptag_amd_exact_search.argtypes = lib.sptag_amd_truth.argtypes
    lib.sptag_amd_exact_search_device.restype = ctypes.c_int
    lib.sptag_amd_exact_search_device.argtypes = lib.sptag_amd_truth.argtypes
    lib.sptag_amd_group_knn.restype = ctypes.c_int
    lib.sptag_amd_group_knn.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p]
    lib.sptag_amd_group_knn_device.restype = ctypes.c_int
    lib.sptag_amd_group_knn_device.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p]
    # the _sel forms take `selection` before k
    lib.sptag_amd_group_knn_sel.restype = ctypes.c_int
    lib.sptag_amd_group_knn_sel.argtypes = (
        lib.sptag_amd_group_knn.argtypes[:6] + [ctypes.c_int32] +
        lib.sptag_amd_group_knn.argtypes[6:])
    lib.sptag_amd_group_knn_sel_device.restype = ctypes.c_int
    lib.sptag_amd_group_knn_sel_device.argtypes = (
        lib.sptag_amd_group_knn_device.argtypes[:11] + [ctypes.c_int32] +
        lib.sptag_amd_group_knn_device.argtypes[11:])
    lib.sptag_amd_group_knn_sort_max.restype = ctypes.c_int32
    lib.sptag_amd_group_knn_sort_max.argtypes = [ctypes.c_int, ctypes.c_int32]
    lib.sptag_amd_rng_prune.restype = ctypes.c_int
    lib.sptag_amd_rng_prune.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
        ctypes.c_int32, ctypes.c_void_p]
    lib.sptag_amd_rng_prune_device.restype = ctypes.c_int
    lib.sptag_amd_rng_prune_device.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
        ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    lib.sptag_amd_pool_join.restype = ctypes.c_int
    lib.sptag_amd_pool_join.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.sptag_amd_pool_join_device.restype = ctypes.c_int
    lib.sptag_amd_pool_join_device.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p]
    lib.sptag_amd_kmeans_assign.restype = ctypes.c_int
    lib.sptag_amd_kmeans_assign.argtypes = (
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] +
        [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_void_p,
                                 ctypes.c_int32, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_int32] +
        [ctypes.c_void_p] * 6)
    lib.sptag_amd_kmeans_assign_device.restype = ctypes.c_int
    lib.sptag_amd_kmeans_assign_device.argtypes = (
        [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
         ctypes.c_int32, ctypes.c_int32] +
        lib.sptag_amd_kmeans_assign.argtypes[1:])
    lib.sptag_amd_tpt_partition.restype = ctypes.c_int
    lib.sptag_amd_tpt_partition.argtypes = (
        [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 5 +
        [ctypes.c_uint64] + [ctypes.c_void_p] * 3 +
        [ctypes.c_int32, ctypes.c_void_p])
    lib.sptag_amd_tpt_partition_device.restype = ctypes.c_int
    lib.sptag_amd_tpt_partition_device.argtypes = (
        [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
         ctypes.c_int32] + lib.sptag_amd_tpt_partition.argtypes[1:])
    lib.sptag_amd_save_index.restype = ctypes.c_int
    lib.sptag_amd_save_index.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    for f in ["num_vectors", "dim", "valuetype", "distmethod", "degree",
              "default_maxcheck", "algo"]:
        fn = getattr(lib, "sptag_amd_" + f)
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_add.restype = ctypes.c_int
    lib.sptag_amd_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_int32, ctypes.c_int]
    lib.sptag_amd_delete.restype = ctypes.c_int
    lib.sptag_amd_delete.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int32]
    lib.sptag_amd_delete_by_vector.restype = ctypes.c_int
    lib.sptag_amd_delete_by_vector.argtypes = lib.sptag_amd_delete.argtypes
    lib.sptag_amd_deleted_count.restype = ctypes.c_int64
    lib.sptag_amd_deleted_count.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_iter_create.restype = ctypes.c_void_p
    lib.sptag_amd_iter_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int32, ctypes.c_int32]
    lib.sptag_amd_iter_next.restype = ctypes.c_int
    lib.sptag_amd_iter_next.argtypes = [ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]
    lib.sptag_amd_iter_free.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_set_search_params.restype = None
    lib.sptag_amd_set_search_params.argtypes = [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
        ctypes.c_int32]
    lib.sptag_amd_merge_topk.restype = ctypes.c_int
    lib.sptag_amd_merge_topk.argtypes = [
        ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p]
    lib.sptag_amd_merge_topk_device.restype = ctypes.c_int
    lib.sptag_amd_merge_topk_device.argtypes = lib.sptag_amd_merge_topk.argtypes
    lib.sptag_amd_shards_create.restype = ctypes.c_void_p
    lib.sptag_amd_shards_create.argtypes = [ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.c_void_p]
    lib.sptag_amd_shards_free.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_shards_search_batch.restype = ctypes.c_int
    lib.sptag_amd_shards_search_batch.argtypes = lib.sptag_amd_search_batch.argtypes
    lib.sptag_amd_shards_search_batch_device.restype = ctypes.c_int
    lib.sptag_amd_shards_search_batch_device.argtypes = \
        lib.sptag_amd_search_batch.argtypes
    lib.sptag_amd_shards_truth.restype = ctypes.c_int
    lib.sptag_amd_shards_truth.argtypes = lib.sptag_amd_truth.argtypes
    lib.sptag_amd_shards_exact_search.restype = ctypes.c_int
    lib.sptag_amd_shards_exact_search.argtypes = lib.sptag_amd_truth.argtypes
    lib.sptag_amd_shards_count.restype = ctypes.c_int32
    lib.sptag_amd_shards_count.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_shards_num_vectors.restype = ctypes.c_int64
    lib.sptag_amd_shards_num_vectors.argtypes = [ctypes.c_void_p]
    lib.sptag_amd_gpu_available.restype = ctypes.c_int
    lib.sptag_amd_build_info.restype = ctypes.c_char_p
    _LIB = lib
    return lib


def gpu_available():
    return bool(load_library().sptag_amd_gpu_available())


def _np_dtype(vt):
    return np.float32 if vt == VT_FLOAT else np.int8


class AnnIndex:
    """Mirror of the reference Python AnnIndex facade over the GPU backend.

    Reference method -> here:
      AnnIndex.Load(folder)            -> AnnIndex.Load(folder)
      AnnIndex.Search(query, k)        -> .Search(query, k)
      AnnIndex.BatchSearch(q, n, k, _) -> .BatchSearch(queries, k)
      (SaveIndex)                      -> .Save(folder)
    """

    def __init__(self, handle, owns=True):
        self._lib = load_library()
        self._h = handle
        self._owns = owns
        if not handle:
            raise SptagAmdError(-1, "index load/create failed (see stderr)")

    # -- construction -------------------------------------------------
    @classmethod
    def Load(cls, folder, device=0):
        lib = load_library()
        h = lib.sptag_amd_load_index(str(folder).encode(), device)
        ix = cls(h)
        ix.metadata = MetadataSet.from_index_folder(str(folder))
        return ix

    @classmethod
    def _from_arrays(cls, symbol, words, vectors, tree_start, nodes, graph,
                     distmethod, deleted, device):
        """Shared body of FromArrays / FromArraysKDT: `symbol` names the C
        constructor, `words` is the int32 count of one tree node."""
        vectors = np.ascontiguousarray(vectors)
        if vectors.dtype not in (np.float32, np.int8):
            raise ValueError("dtype must be float32 or int8")
        lib = load_library()
        vt = VT_FLOAT if vectors.dtype == np.float32 else VT_INT8
        n, dim = vectors.shape
        tree_start = np.ascontiguousarray(tree_start, dtype=np.int32)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        graph = np.ascontiguousarray(graph, dtype=np.int32)
        dm = {"L2": DM_L2, "Cosine": DM_COSINE}.get(distmethod, distmethod)
        delp = None
        if deleted is not None:
            deleted = np.ascontiguousarray(deleted, dtype=np.uint8)
            delp = deleted.ctypes.data_as(ctypes.c_void_p)
        h = getattr(lib, symbol)(
            n, dim, vt, dm, vectors.ctypes.data_as(ctypes.c_void_p),
            len(tree_start), tree_start.ctypes.data_as(ctypes.c_void_p),
            nodes.size // words, nodes.ctypes.data_as(ctypes.c_void_p),
            graph.shape[1], graph.ctypes.data_as(ctypes.c_void_p),
            delp, device)
        return cls(h)

    @classmethod
    def FromArrays(cls, vectors, tree_start, tree_nodes, graph, distmethod,
                   deleted=None, device=0):
        """Assemble from raw numpy blobs (file layouts without headers)."""
        return cls._from_arrays("sptag_amd_create_index", 3, vectors,
                                tree_start, tree_nodes, graph, distmethod,
                                deleted, device)

    @classmethod
    def FromArraysKDT(cls, vectors, tree_start, kdt_nodes, graph, distmethod,
                      deleted=None, device=0):
        """KDT variant: kdt_nodes is an int32 [N,4] array whose 4th column
        holds the float split_value bit pattern (KDTree.h:22)."""
        return cls._from_arrays("sptag_amd_create_index_kdt", 4, vectors,
                                tree_start, kdt_nodes, graph, distmethod,
                                deleted, device)

    def __del__(self):
        if getattr(self, "_owns", False) and getattr(self, "_h", None):
            self._lib.sptag_amd_free_index(self._h)
            self._h = None

    # -- metadata -----------------------------------------------------
    @property
    def n(self):
        return self._lib.sptag_amd_num_vectors(self._h)

    @property
    def dim(self):
        return self._lib.sptag_amd_dim(self._h)

    @property
    def valuetype(self):
        return self._lib.sptag_amd_valuetype(self._h)

    @property
    def distmethod(self):
        return self._lib.sptag_amd_distmethod(self._h)

    @property
    def algo(self):
        """0 = BKT, 1 = KDT (from the loaded indexloader.ini)."""
        return self._lib.sptag_amd_algo(self._h)

    @property
    def degree(self):
        return self._lib.sptag_amd_degree(self._h)

    @property
    def default_maxcheck(self):
        return self._lib.sptag_amd_default_maxcheck(self._h)

    # -- search -------------------------------------------------------
    def _rows(self, a):
        """`a` as the C side reads row vectors: contiguous, the index's
        dtype, [rows, dim] (a single vector becomes one row)."""
        a = np.ascontiguousarray(a, dtype=_np_dtype(self.valuetype))
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError(f"expected rows of {self.dim} values, got shape {a.shape}")
        return a

    def BatchSearch(self, queries, k, max_check=0):
        """GPU batched search. Returns (vids int32 [nq,k], dists f32 [nq,k]),
        ascending by (dist, vid), vid=-1 padding — the contract of the
        reference batch overload VectorIndex.h:103."""
        queries = self._rows(queries)
        nq = queries.shape[0]
        vids = np.empty((nq, k), dtype=np.int32)
        dists = np.empty((nq, k), dtype=np.float32)
        rc = self._lib.sptag_amd_search_batch(
            self._h, queries.ctypes.data_as(ctypes.c_void_p), nq, k, max_check,
            vids.ctypes.data_as(ctypes.c_void_p),
            dists.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, "search_batch")
        return vids, dists

    def BatchSearchDevice(self, d_queries_ptr, nq, k, d_vids_ptr, d_dists_ptr,
                          max_check=0):
        """Device-resident search: all pointers are HIP device addresses
        (e.g. torch cuda tensors' .data_ptr()); no PCIe copies inside."""
        rc = self._lib.sptag_amd_search_batch_device(
            self._h, ctypes.c_void_p(d_queries_ptr), nq, k, max_check,
            ctypes.c_void_p(d_vids_ptr), ctypes.c_void_p(d_dists_ptr))
        if rc != 0:
            raise SptagAmdError(rc, "search_batch_device")

    def LastStats(self):
        """(kernel_ms, checked, popped) of the last search call."""
        ms = ctypes.c_double()
        ch = ctypes.c_longlong()
        po = ctypes.c_longlong()
        self._lib.sptag_amd_last_stats(self._h, ctypes.byref(ms),
                                       ctypes.byref(ch), ctypes.byref(po))
        return ms.value, ch.value, po.value

    def Search(self, query, k, max_check=0):
        vids, dists = self.BatchSearch(query, k, max_check)
        return vids[0], dists[0]

    def BatchSearchWithMeta(self, queries, k, max_check=0):
        """reference AnnIndex.BatchSearchWithMetaData: results plus the
        per-result metadata blobs (empty when the index has none)."""
        vids, dists = self.BatchSearch(queries, k, max_check)
        meta = getattr(self, "metadata", None)
        blobs = [[meta.get(int(v)) if meta else b"" for v in row]
                 for row in vids]
        return vids, dists, blobs

    def Truth(self, queries, k):
        """Exact brute-force top-k on the GPU."""
        queries = self._rows(queries)
        nq = queries.shape[0]
        vids = np.empty((nq, k), dtype=np.int32)
        dists = np.empty((nq, k), dtype=np.float32)
        rc = self._lib.sptag_amd_truth(
            self._h, queries.ctypes.data_as(ctypes.c_void_p), nq, k,
            vids.ctypes.data_as(ctypes.c_void_p),
            dists.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, "truth")
        return vids, dists

    def ExactSearch(self, queries, k):
        """Exact top-k by the tiled brute-force kernels: Truth's answer, bit
        for bit, at workload scale."""
        queries = self._rows(queries)
        nq = queries.shape[0]
        vids = np.empty((nq, k), dtype=np.int32)
        dists = np.empty((nq, k), dtype=np.float32)
        rc = self._lib.sptag_amd_exact_search(
            self._h, queries.ctypes.data_as(ctypes.c_void_p), nq, k,
            vids.ctypes.data_as(ctypes.c_void_p),
            dists.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, "exact_search")
        return vids, dists

    def ExactSearchDevice(self, d_queries_ptr, nq, k, d_vids_ptr, d_dists_ptr):
        """ExactSearch on HIP device addresses, as BatchSearchDevice."""
        rc = self._lib.sptag_amd_exact_search_device(
            self._h, ctypes.c_void_p(d_queries_ptr), nq, k,
            ctypes.c_void_p(d_vids_ptr), ctypes.c_void_p(d_dists_ptr))
        if rc != 0:
            raise SptagAmdError(rc, "exact_search_device")

    def GroupKnn(self, members, starts, counts, k, selection="stream"):
        """Exact kNN inside row groups: group g is members[starts[g] :
        starts[g] + counts[g]] (vector ids, any order, none twice). Returns
        (vids int32 [n,k], dists f32 [n,k]) indexed by vector id: the k
        nearest OTHER members of the id's group, ascending (dist, vid),
        vid=-1 padding; all padding for an id in no group. selection picks the
        kernel, never the result: "stream" (a threshold and merges), "sort"
        (all distances of a query in LDS, one select and one sort; groups up
        to group_knn_sort_max members, larger ones are an error) or "auto"
        (per group, the one measured faster)."""
        selection = _gk_selection(selection)
        members = np.ascontiguousarray(members, dtype=np.int32)
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if starts.shape != counts.shape or starts.ndim != 1:
            raise ValueError("starts and counts must be 1-d and of one length")
        n = self.n
        vids = np.empty((n, k), dtype=np.int32)
        dists = np.empty((n, k), dtype=np.float32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.sptag_amd_group_knn_sel(
            self._h, p(members), members.size, p(starts), p(counts),
            starts.size, selection, k, p(vids), p(dists))
        if rc != 0:
            raise SptagAmdError(rc, "group_knn")
        return vids, dists

    def RngPrune(self, nodes, cand_ids, cand_dists, degree, rng_factor=1.0,
                 fill_pruned=False):
        """The reference's RebuildNeighbors over candidate lists: row r walks
        cand_ids[r] (ascending cand_dists[r], never recomputed) and accepts a
        valid candidate (id >= 0, not nodes[r], finite distance) unless an
        accepted a has rng_factor * dist(a, c) < cand_dists[r][c], up to
        `degree`; dist is the handle's search distance. Returns int32
        [nrows, degree]: the accepted ids in list order, -1 padded; with
        fill_pruned a short row keeps its nearest rejected candidates too."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.int32)
        cand_dists = np.ascontiguousarray(cand_dists, dtype=np.float32)
        if (nodes.ndim != 1 or cand_ids.ndim != 2 or
                cand_ids.shape != cand_dists.shape or
                cand_ids.shape[0] != nodes.size):
            raise ValueError("nodes [nrows], cand_ids and cand_dists "
                             "[nrows, ncand] expected")
        out = np.empty((nodes.size, max(int(degree), 0)), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.sptag_amd_rng_prune(
            self._h, p(nodes), nodes.size, p(cand_ids), p(cand_dists),
            cand_ids.shape[1], degree, rng_factor, 1 if fill_pruned else 0,
            p(out))
        if rc != 0:
            raise SptagAmdError(rc, "rng_prune")
        return out

    def PoolJoin(self, nodes, pool_ids, pool_dists, new_ids, kout,
                 new_dists=None):
        """Grow candidate pools: row r merges its old pool (pool_ids[r] with
        pool_dists[r], used as given; both may be None) with new_ids[r], whose
        distances are new_dists[r] or, when that is None, the handle's search
        distance to vector nodes[r]. Ids < 0, nodes[r] itself and non-finite
        given distances are dropped, a new id already valid in the pool keeps
        the pool's entry, repeats keep their smallest distance. Returns
        (ids int32, dists float32), both [nrows, kout]: the kout smallest in
        ascending (dist, id), padded with -1 at +inf."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        new_ids = np.ascontiguousarray(new_ids, dtype=np.int32)
        if pool_ids is None:
            pool_ids = np.empty((nodes.size, 0), dtype=np.int32)
            pool_dists = np.empty((nodes.size, 0), dtype=np.float32)
        pool_ids = np.ascontiguousarray(pool_ids, dtype=np.int32)
        pool_dists = np.ascontiguousarray(pool_dists, dtype=np.float32)
        if new_dists is not None:
            new_dists = np.ascontiguousarray(new_dists, dtype=np.float32)
        if (nodes.ndim != 1 or pool_ids.ndim != 2 or new_ids.ndim != 2 or
                pool_ids.shape != pool_dists.shape or
                pool_ids.shape[0] != nodes.size or
                new_ids.shape[0] != nodes.size or
                (new_dists is not None and new_dists.shape != new_ids.shape)):
            raise ValueError("nodes [nrows], pool_ids and pool_dists "
                             "[nrows, npool], new_ids (and new_dists) "
                             "[nrows, nnew] expected")
        kout = int(kout)
        ids = np.empty((nodes.size, max(kout, 0)), dtype=np.int32)
        dists = np.empty(ids.shape, dtype=np.float32)
        # an empty list goes in as a null pointer
        p = lambda a: (a.ctypes.data_as(ctypes.c_void_p)
                       if a is not None and a.size else None)
        rc = self._lib.sptag_amd_pool_join(
            self._h, p(nodes), nodes.size, p(pool_ids), p(pool_dists),
            pool_ids.shape[1], p(new_ids), p(new_dists), new_ids.shape[1],
            kout, ids.ctypes.data_as(ctypes.c_void_p),
            dists.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, "pool_join")
        return ids, dists

    def KmeansAssign(self, members, seg_starts, seg_sizes, centers, ncenters,
                     update, prev_counts=None, lambdas=None):
        """One k-means assign pass over segments of a member list: segment s
        is members[seg_starts[s] : seg_starts[s] + seg_sizes[s]] (vector ids)
        with centers centers[s, :ncenters[s]] of centers [nseg, kmax, dim] in
        the vectors' value type. A member goes to the center of smallest
        handle search distance plus lambdas[s] * prev_counts[s, k] (both or
        neither given), ties to the lowest k. Returns (labels int32
        [nmembers], dists f32 [nmembers], counts int32 [nseg, kmax],
        cluster_idx int32 [nseg, kmax], cluster_dist f32 [nseg, kmax], sums):
        per center one extreme member as a vector id, the farthest with
        update, the nearest without, -1 for an empty center; sums f32
        [nseg, kmax, dim] of the members' vectors with update, else None.
        Entries of centers at or past ncenters[s], and labels of places in no
        segment, come back as 0."""
        members = np.ascontiguousarray(members, dtype=np.int32)
        seg_starts = np.ascontiguousarray(seg_starts, dtype=np.int32)
        seg_sizes = np.ascontiguousarray(seg_sizes, dtype=np.int32)
        ncenters = np.ascontiguousarray(ncenters, dtype=np.int32)
        centers = np.ascontiguousarray(
            centers, dtype=np.float32 if self.valuetype == VT_FLOAT else np.int8)
        if (members.ndim != 1 or seg_starts.ndim != 1 or centers.ndim != 3 or
                not (seg_starts.shape == seg_sizes.shape == ncenters.shape
                     == centers.shape[:1]) or centers.shape[2] != self.dim):
            raise ValueError("members [nmembers], seg_starts, seg_sizes and "
                             "ncenters [nseg], centers [nseg, kmax, dim] "
                             "expected")
        nseg, kmax = centers.shape[:2]
        if (prev_counts is None) != (lambdas is None):
            raise ValueError("prev_counts and lambdas go together")
        if lambdas is not None:
            prev_counts = np.ascontiguousarray(prev_counts, dtype=np.int32)
            lambdas = np.ascontiguousarray(lambdas, dtype=np.float32)
            if prev_counts.shape != (nseg, kmax) or lambdas.shape != (nseg,):
                raise ValueError("prev_counts [nseg, kmax] and lambdas [nseg] "
                                 "expected")
        labels = np.zeros(members.size, dtype=np.int32)
        dists = np.zeros(members.size, dtype=np.float32)
        counts = np.zeros((nseg, kmax), dtype=np.int32)
        cidx = np.zeros((nseg, kmax), dtype=np.int32)
        cdist = np.zeros((nseg, kmax), dtype=np.float32)
        sums = (np.zeros((nseg, kmax, self.dim), dtype=np.float32)
                if update else None)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.sptag_amd_kmeans_assign(
            self._h, p(members), members.size, p(seg_starts), p(seg_sizes),
            p(ncenters), nseg, p(centers), kmax, p(prev_counts), p(lambdas),
            1 if update else 0, p(labels), p(dists), p(counts), p(cidx),
            p(cdist), p(sums))
        if rc != 0:
            raise SptagAmdError(rc, "kmeans_assign")
        return labels, dists, counts, cidx, cdist, sums

    def TptPartition(self, members, leaf_size, samples=1000, topdims=5,
                     trials=100, seed=0):
        """TP-tree partition of a member list (vector ids) by the reference's
        hyperplane rule (include/sptag_amd.h): a segment longer than leaf_size
        splits at the mean of the projection of largest variance among
        `trials` random weightings of the `topdims` widest dimensions of its
        first `samples` members, stably. Returns (members int32 [nmembers]
        permuted, starts int32 [nleaves], counts int32 [nleaves]): leaf i is
        members[starts[i] : starts[i] + counts[i]], in ascending start order."""
        members = np.ascontiguousarray(members, dtype=np.int32)
        if members.ndim != 1:
            raise ValueError("members [nmembers] expected")
        out = np.empty_like(members)

        def call(starts, counts, nleaves):
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            return self._lib.sptag_amd_tpt_partition(
                self._h, p(members), members.size, leaf_size, samples,
                topdims, trials, seed, p(out), p(starts), p(counts),
                starts.size, ctypes.byref(nleaves))
        starts, counts = _tpt_leaf_table(call, members.size, leaf_size,
                                         "tpt_partition")
        return out, starts, counts

    def Add(self, vectors, normalized=False):
        """Online add (reference AddIndex semantics below the tree-rebuild
        threshold); runs GPU refine searches per added vector."""
        vectors = self._rows(vectors)
        rc = self._lib.sptag_amd_add(
            self._h, vectors.ctypes.data_as(ctypes.c_void_p),
            vectors.shape[0], 1 if normalized else 0)
        if rc != 0:
            raise SptagAmdError(rc, "add")

    def Delete(self, vids):
        """Flag vector ids as deleted (reference DeleteIndex semantics);
        searches exclude them from then on."""
        vids = np.ascontiguousarray(vids, dtype=np.int32)
        rc = self._lib.sptag_amd_delete(
            self._h, vids.ctypes.data_as(ctypes.c_void_p), vids.size)
        if rc != 0:
            raise SptagAmdError(rc, "delete")

    def DeleteByVector(self, vectors):
        """Delete exact duplicates of the given vectors (reference
        DeleteIndex(const void*, n) semantics: CEF search + dist < 1e-6)."""
        vectors = self._rows(vectors)
        rc = self._lib.sptag_amd_delete_by_vector(
            self._h, vectors.ctypes.data_as(ctypes.c_void_p), vectors.shape[0])
        if rc != 0:
            raise SptagAmdError(rc, "delete_by_vector")

    @property
    def deleted_count(self):
        return self._lib.sptag_amd_deleted_count(self._h)

    def SetSearchParams(self, init_pivots=0, other_pivots=0,
                        nobetter_threshold=0, max_check=0):
        """Reference SetParameter equivalents (NumberOfInitialDynamicPivots
        etc., BKTIndex.cpp:980); pass 0 to keep a value."""
        self._lib.sptag_amd_set_search_params(
            self._h, init_pivots, other_pivots, nobetter_threshold, max_check)

    def Iterate(self, queries, max_check=0):
        """Streaming search: mirrors the reference GetIterator/Next protocol
        (ResultIterator) for a batch of queries with device-persistent
        traversal state."""
        return IterBatch(self, queries, max_check)

    def Save(self, folder):
        os.makedirs(folder, exist_ok=True)
        rc = self._lib.sptag_amd_save_index(self._h, str(folder).encode())
        if rc != 0:
            raise SptagAmdError(rc, "save_index")


GK_SELECTIONS = {"stream": 0, "sort": 1, "auto": 2}


def _gk_selection(selection):
    if selection not in GK_SELECTIONS:
        raise ValueError('selection must be "stream", "sort" or "auto"')
    return GK_SELECTIONS[selection]


def group_knn_sort_max(valuetype, dim):
    """The largest group that selection="sort" takes for a value type
    (VT_FLOAT / VT_INT8) and dim; 0 where grouped kNN rejects them."""
    return int(load_library().sptag_amd_group_knn_sort_max(valuetype, dim))


def group_knn_device(d_vectors_ptr, valuetype, distmethod, n, dim,
                     d_members_ptr, nmembers, starts, counts, k, d_vids_ptr,
                     d_dists_ptr, device=0, selection="stream"):
    """AnnIndex.GroupKnn without a handle, on HIP device addresses (e.g. torch
    tensors' .data_ptr()): vectors [n, dim] of `valuetype`, int32 members
    [nmembers], outputs int32 / float32 [n, k]. starts and counts are host
    arrays. The caller guarantees that every member is inside [0, n) and
    occurs once. selection as in AnnIndex.GroupKnn."""
    selection = _gk_selection(selection)
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if starts.shape != counts.shape or starts.ndim != 1:
        raise ValueError("starts and counts must be 1-d and of one length")
    dm = {"L2": DM_L2, "Cosine": DM_COSINE}.get(distmethod, distmethod)
    rc = load_library().sptag_amd_group_knn_sel_device(
        device, ctypes.c_void_p(d_vectors_ptr), valuetype, dm, n, dim,
        ctypes.c_void_p(d_members_ptr), nmembers,
        starts.ctypes.data_as(ctypes.c_void_p),
        counts.ctypes.data_as(ctypes.c_void_p), starts.size, selection, k,
        ctypes.c_void_p(d_vids_ptr), ctypes.c_void_p(d_dists_ptr))
    if rc != 0:
        raise SptagAmdError(rc, "group_knn_device")


def rng_prune_device(d_vectors_ptr, valuetype, distmethod, n, dim,
                     d_nodes_ptr, nrows, d_cand_ids_ptr, d_cand_dists_ptr,
                     ncand, degree, rng_factor, fill_pruned, d_out_ptr,
                     device=0):
    """AnnIndex.RngPrune without a handle, on HIP device addresses (e.g. torch
    tensors' .data_ptr()): vectors [n, dim] of `valuetype`, int32 nodes
    [nrows], int32 / float32 lists [nrows, ncand], output int32
    [nrows, degree]. The caller guarantees that every node and every
    candidate id >= 0 is inside [0, n)."""
    dm = {"L2": DM_L2, "Cosine": DM_COSINE}.get(distmethod, distmethod)
    rc = load_library().sptag_amd_rng_prune_device(
        device, ctypes.c_void_p(d_vectors_ptr), valuetype, dm, n, dim,
        ctypes.c_void_p(d_nodes_ptr), nrows, ctypes.c_void_p(d_cand_ids_ptr),
        ctypes.c_void_p(d_cand_dists_ptr), ncand, degree, rng_factor,
        1 if fill_pruned else 0, ctypes.c_void_p(d_out_ptr))
    if rc != 0:
        raise SptagAmdError(rc, "rng_prune_device")


def pool_join_device(d_vectors_ptr, valuetype, distmethod, n, dim,
                     d_nodes_ptr, nrows, d_pool_ids_ptr, d_pool_dists_ptr,
                     npool, d_new_ids_ptr, d_new_dists_ptr, nnew, kout,
                     d_out_ids_ptr, d_out_dists_ptr, device=0):
    """AnnIndex.PoolJoin without a handle, on HIP device addresses (e.g. torch
    tensors' .data_ptr()): vectors [n, dim] of `valuetype`, int32 nodes
    [nrows], int32 / float32 pools [nrows, npool] and new lists
    [nrows, nnew], outputs int32 / float32 [nrows, kout], which may be the
    pool's own buffers when kout == npool. The pool pointers may be None at
    npool == 0; d_new_dists_ptr None has the distances computed. The caller
    guarantees that every node and every id >= 0 is inside [0, n)."""
    dm = {"L2": DM_L2, "Cosine": DM_COSINE}.get(distmethod, distmethod)
    vp = lambda a: ctypes.c_void_p(a) if a else None
    rc = load_library().sptag_amd_pool_join_device(
        device, vp(d_vectors_ptr), valuetype, dm, n, dim, vp(d_nodes_ptr),
        nrows, vp(d_pool_ids_ptr), vp(d_pool_dists_ptr), npool,
        vp(d_new_ids_ptr), vp(d_new_dists_ptr), nnew, kout,
        vp(d_out_ids_ptr), vp(d_out_dists_ptr))
    if rc != 0:
        raise SptagAmdError(rc, "pool_join_device")


def kmeans_assign_device(d_vectors_ptr, valuetype, distmethod, n, dim,
                         d_members_ptr, nmembers, seg_starts, seg_sizes,
                         ncenters, d_centers_ptr, kmax, d_prev_counts_ptr,
                         d_lambdas_ptr, update, d_labels_ptr, d_dists_ptr,
                         d_counts_ptr, d_cluster_idx_ptr, d_cluster_dist_ptr,
                         d_sums_ptr, device=0):
    """AnnIndex.KmeansAssign without a handle, on HIP device addresses (e.g.
    torch tensors' .data_ptr()): vectors [n, dim] and centers [nseg, kmax,
    dim] of `valuetype`, int32 members [nmembers], outputs int32 / float32
    [nmembers] and [nseg, kmax], float32 sums [nseg, kmax, dim]. seg_starts,
    seg_sizes and ncenters are host arrays. d_prev_counts_ptr and
    d_lambdas_ptr are both None or both given; d_dists_ptr may be None, and
    d_sums_ptr without update. The caller guarantees that every member is
    inside [0, n)."""
    seg_starts = np.ascontiguousarray(seg_starts, dtype=np.int32)
    seg_sizes = np.ascontiguousarray(seg_sizes, dtype=np.int32)
    ncenters = np.ascontiguousarray(ncenters, dtype=np.int32)
    if not (seg_starts.shape == seg_sizes.shape == ncenters.shape) or \
            seg_starts.ndim != 1:
        raise ValueError("seg_starts, seg_sizes and ncenters must be 1-d and "
                         "of one length")
    dm = {"L2": DM_L2, "Cosine": DM_COSINE}.get(distmethod, distmethod)
    vp = lambda a: ctypes.c_void_p(a) if a else None
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = load_library().sptag_amd_kmeans_assign_device(
        device, vp(d_vectors_ptr), valuetype, dm, n, dim, vp(d_members_ptr),
        nmembers, hp(seg_starts), hp(seg_sizes), hp(ncenters),
        seg_starts.size, vp(d_centers_ptr), kmax, vp(d_prev_counts_ptr),
        vp(d_lambdas_ptr), 1 if update else 0, vp(d_labels_ptr),
        vp(d_dists_ptr), vp(d_counts_ptr), vp(d_cluster_idx_ptr),
        vp(d_cluster_dist_ptr), vp(d_sums_ptr))
    if rc != 0:
        raise SptagAmdError(rc, "kmeans_assign_device")


def _tpt_leaf_table(call, nmembers, leaf_size, what):
    """Runs call(starts, counts, nleaves) with a modest leaf table and once
    more with the size the library asked for; returns (starts, counts)."""
    nleaves = ctypes.c_int32(-1)
    cap = min(max(nmembers, 1), 64 + 4 * (nmembers // max(leaf_size, 1)))
    for _ in range(2):
        starts = np.empty(cap, dtype=np.int32)
        counts = np.empty(cap, dtype=np.int32)
        rc = call(starts, counts, nleaves)
        if rc == 0:
            return starts[:nleaves.value].copy(), counts[:nleaves.value].copy()
        if nleaves.value <= cap:
            break
        cap = nleaves.value
    raise SptagAmdError(rc, what)


def tpt_partition_device(d_vectors_ptr, valuetype, n, dim, d_members_ptr,
                         nmembers, leaf_size, d_out_members_ptr, samples=1000,
                         topdims=5, trials=100, seed=0, device=0):
    """AnnIndex.TptPartition without a handle, on HIP device addresses (e.g.
    torch tensors' .data_ptr()): vectors [n, dim] of `valuetype`, int32
    members and out_members [nmembers]; the output may be the input. Returns
    the leaf table (starts, counts) as int32 numpy arrays. The caller
    guarantees that every member is inside [0, n)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None
    lib = load_library()

    def call(starts, counts, nleaves):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        return lib.sptag_amd_tpt_partition_device(
            device, vp(d_vectors_ptr), valuetype, n, dim, vp(d_members_ptr),
            nmembers, leaf_size, samples, topdims, trials, seed,
            vp(d_out_members_ptr), p(starts), p(counts), starts.size,
            ctypes.byref(nleaves))
    return _tpt_leaf_table(call, nmembers, leaf_size, "tpt_partition_device")


def merge_topk(vids, dists, vid_base, k, device=0):
    """Merge per-shard top-k lists on the GPU (reference AggregatorService::
    AggregateResults, AggregatorService.cpp:363). vids int32 / dists float32
    of shape [S, nq, k_in], every list ascending (dist, vid) with its padding
    a suffix of vid < 0; vid_base [S] is added to the ids of shard s. Returns
    (vids [nq,k], dists [nq,k]) ascending (dist, global vid), vid=-1 padding."""
    vids = np.ascontiguousarray(vids, dtype=np.int32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    vid_base = np.ascontiguousarray(vid_base, dtype=np.int32)
    if vids.ndim != 3 or dists.shape != vids.shape:
        raise ValueError("vids and dists must both be [S, nq, k_in]")
    nshards, nq, k_in = vids.shape
    if vid_base.shape != (nshards,):
        raise ValueError(f"vid_base must hold {nshards} values")
    out_v = np.empty((nq, k), dtype=np.int32)
    out_d = np.empty((nq, k), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = load_library().sptag_amd_merge_topk(
        device, nshards, nq, k_in, k, p(vids), p(dists), p(vid_base),
        p(out_v), p(out_d))
    if rc != 0:
        raise SptagAmdError(rc, "merge_topk")
    return out_v, out_d


class ShardedIndex:
    """Several AnnIndex shards searched as one: every shard answers the whole
    batch and the lists are merged on the GPU of shard 0, ascending (dist,
    global vid) with global vid = shard vid + vid_base[shard]. Add and Delete
    stay on the shards' own AnnIndex objects (`.shards`); the set sees them
    on its next call."""

    def __init__(self, handle, shards):
        self._lib = load_library()
        self._h = handle
        self.shards = list(shards)   # the C set borrows their handles
        if not handle:
            raise SptagAmdError(-2, "shards_create refused (see stderr)")

    @classmethod
    def FromIndexes(cls, indexes, vid_base=None):
        """vid_base None = running sum of the shards' sizes now; give
        explicit bases with room if shards other than the last will grow."""
        indexes = list(indexes)
        lib = load_library()
        handles = (ctypes.c_void_p * len(indexes))(*[ix._h for ix in indexes])
        basep = None
        if vid_base is not None:
            vid_base = np.ascontiguousarray(vid_base, dtype=np.int32)
            if vid_base.shape != (len(indexes),):
                raise ValueError(f"vid_base must hold {len(indexes)} values")
            basep = vid_base.ctypes.data_as(ctypes.c_void_p)
        return cls(lib.sptag_amd_shards_create(handles, len(indexes), basep),
                   indexes)

    @classmethod
    def Load(cls, folders, devices=None):
        """One index folder per shard; devices[i] is shard i's GPU
        (default: all on device 0)."""
        folders = list(folders)
        if devices is None:
            devices = [0] * len(folders)
        if len(devices) != len(folders):
            raise ValueError("one device per folder")
        return cls.FromIndexes([AnnIndex.Load(f, d)
                                for f, d in zip(folders, devices)])

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.sptag_amd_shards_free(self._h)
            self._h = None

    def NumShards(self):
        return self._lib.sptag_amd_shards_count(self._h)

    def NumVectors(self):
        return self._lib.sptag_amd_shards_num_vectors(self._h)

    def _call(self, fn, what, queries, k, *mid):
        queries = self.shards[0]._rows(queries)
        nq = queries.shape[0]
        vids = np.empty((nq, k), dtype=np.int32)
        dists = np.empty((nq, k), dtype=np.float32)
        rc = fn(self._h, queries.ctypes.data_as(ctypes.c_void_p), nq, k, *mid,
                vids.ctypes.data_as(ctypes.c_void_p),
                dists.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, what)
        return vids, dists

    def BatchSearch(self, queries, k, max_check=0):
        """(vids int32 [nq,k], dists f32 [nq,k]) over all shards, global ids."""
        return self._call(self._lib.sptag_amd_shards_search_batch,
                          "shards_search_batch", queries, k, max_check)

    def BatchSearchDevice(self, d_queries_ptr, nq, k, d_vids_ptr, d_dists_ptr,
                          max_check=0):
        """All pointers are HIP device addresses on the device of shard 0."""
        rc = self._lib.sptag_amd_shards_search_batch_device(
            self._h, ctypes.c_void_p(d_queries_ptr), nq, k, max_check,
            ctypes.c_void_p(d_vids_ptr), ctypes.c_void_p(d_dists_ptr))
        if rc != 0:
            raise SptagAmdError(rc, "shards_search_batch_device")

    def Truth(self, queries, k):
        """Exact brute-force top-k over all shards, global ids."""
        return self._call(self._lib.sptag_amd_shards_truth, "shards_truth",
                          queries, k)

    def ExactSearch(self, queries, k):
        """Truth's answer by AnnIndex.ExactSearch per shard."""
        return self._call(self._lib.sptag_amd_shards_exact_search,
                          "shards_exact_search", queries, k)


class MetadataSet:
    """Reference MemMetadataSet file pair (src/Core/MetadataSet.cpp:269-283:
    metadataIndex = [int32 count][uint64 offsets x (count+1)]; metadata =
    concatenated byte blobs). Post-search VID -> bytes lookup — host-side
    only, exactly as the reference's SearchIndex metadata copy
    (BKTIndex.cpp:611-618)."""

    def __init__(self, meta_file, metaindex_file):
        with open(metaindex_file, "rb") as f:
            self.count = int(np.frombuffer(f.read(4), dtype=np.int32)[0])
            self.offsets = np.frombuffer(f.read(8 * (self.count + 1)),
                                         dtype=np.uint64)
        self.blob = open(meta_file, "rb").read()

    def get(self, vid):
        if vid < 0 or vid >= self.count:
            return b""
        return self.blob[int(self.offsets[vid]):int(self.offsets[vid + 1])]

    @classmethod
    def from_index_folder(cls, folder):
        """Load the pair named by indexloader.ini's [MetaData] section
        (VectorIndex.cpp:618 LoadIndex), or None when the index has none."""
        ini = os.path.join(folder, "indexloader.ini")
        if not os.path.exists(ini):
            return None
        meta = metaidx = None
        section = None
        for line in open(ini):
            line = line.strip()
            if line.startswith("["):
                section = line
            elif section == "[MetaData]" and "=" in line:
                key, val = line.split("=", 1)
                if key == "MetaDataFilePath":
                    meta = val
                elif key == "MetaDataIndexPath":
                    metaidx = val
        if not meta or not metaidx:
            return None
        return cls(os.path.join(folder, meta), os.path.join(folder, metaidx))


class IterBatch:
    """Batch of per-query result iterators (reference ResultIterator
    semantics; state persists on the GPU between Next calls)."""

    def __init__(self, index, queries, max_check=0):
        self._lib = index._lib
        self._index = index   # keep the index alive
        queries = index._rows(queries)
        self.nq = queries.shape[0]
        self._h = self._lib.sptag_amd_iter_create(
            index._h, queries.ctypes.data_as(ctypes.c_void_p), self.nq,
            max_check)
        if not self._h:
            raise SptagAmdError(-6, "iter_create failed (see stderr)")

    def Next(self, batch):
        """Returns (vids [nq,batch], dists, counts [nq], relaxed [nq]):
        the next `counts[i]` nearest results of query i, sorted; vid=-1
        padding; relaxed = the sticky relaxed-monotonicity flag."""
        vids = np.empty((self.nq, batch), dtype=np.int32)
        dists = np.empty((self.nq, batch), dtype=np.float32)
        counts = np.empty(self.nq, dtype=np.int32)
        relaxed = np.empty(self.nq, dtype=np.int32)
        rc = self._lib.sptag_amd_iter_next(
            self._h, batch, vids.ctypes.data_as(ctypes.c_void_p),
            dists.ctypes.data_as(ctypes.c_void_p),
            counts.ctypes.data_as(ctypes.c_void_p),
            relaxed.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise SptagAmdError(rc, "iter_next")
        return vids, dists, counts, relaxed

    def Close(self):
        if getattr(self, "_h", None):
            self._lib.sptag_amd_iter_free(self._h)
            self._h = None

    def __del__(self):
        self.Close()
