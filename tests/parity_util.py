"""Shared helpers of the mutation / deep-iterator / small-index parity tests:
raw index arrays of a golden fixture, the oracle's add entry points, seeded
CPU-built indexes (cached, never modified) and iterator drivers."""
import ctypes
import os

import numpy as np

from oracle.pyoracle import OrcIndex, OrcIter, load_library

MAXDIST = np.float32(np.finfo(np.float32).max / np.float32(10.0))  # Common.h:122


def read_index_arrays(folder, dtype):
    """(vectors, tree_start, tree_nodes, graph) of a saved BKT/KDT folder;
    tree_nodes is the flat int32 array as stored (3 or 4 words per node)."""
    with open(os.path.join(folder, "vectors.bin"), "rb") as f:
        n, dim = np.frombuffer(f.read(8), dtype=np.int32)
        vec = np.frombuffer(f.read(), dtype=dtype).reshape(n, dim)
    with open(os.path.join(folder, "graph.bin"), "rb") as f:
        gn, deg = np.frombuffer(f.read(8), dtype=np.int32)
        graph = np.frombuffer(f.read(), dtype=np.int32).reshape(gn, deg)
    with open(os.path.join(folder, "tree.bin"), "rb") as f:
        ntrees = np.frombuffer(f.read(4), dtype=np.int32)[0]
        tstart = np.frombuffer(f.read(4 * ntrees), dtype=np.int32)
        nnodes = np.frombuffer(f.read(4), dtype=np.int32)[0]
        tnodes = np.frombuffer(f.read(), dtype=np.int32)
    assert tnodes.size % nnodes == 0
    return vec, tstart, tnodes, graph


def golden_dtype(g):
    return np.float32 if g["meta"]["valuetype"] == "Float" else np.int8


def read_graph(path):
    with open(path, "rb") as f:
        gn, deg = np.frombuffer(f.read(8), dtype=np.int32)
        return np.frombuffer(f.read(), dtype=np.int32).reshape(gn, deg)


def read_vectors(path, dtype):
    with open(path, "rb") as f:
        n, dim = np.frombuffer(f.read(8), dtype=np.int32)
        return np.frombuffer(f.read(), dtype=dtype).reshape(n, dim)


_orc = None


def _lib():
    """The oracle library with the add entry points' signatures declared."""
    global _orc
    if _orc is not None:
        return _orc
    lib = load_library()
    lib.orc_add.restype = ctypes.c_int
    lib.orc_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                            ctypes.c_int32, ctypes.c_int]
    lib.orc_graph_ptr.restype = ctypes.POINTER(ctypes.c_int32)
    lib.orc_graph_ptr.argtypes = [ctypes.c_void_p]
    lib.orc_vectors_ptr.restype = ctypes.c_void_p
    lib.orc_vectors_ptr.argtypes = [ctypes.c_void_p]
    _orc = lib
    return lib


def orc_add(oix, vectors, normalized=False):
    """AddIndex restatement with the AddCEF default of 500."""
    dtype = np.float32 if oix.valuetype == 0 else np.int8
    vectors = np.ascontiguousarray(vectors, dtype=dtype)
    rc = _lib().orc_add(oix._h, vectors.ctypes.data_as(ctypes.c_void_p),
                        vectors.shape[0], 500, 1 if normalized else 0)
    assert rc == 0


def orc_graph(oix):
    """Copy of the oracle's current graph, [n, degree]."""
    lib = _lib()
    deg = lib.orc_degree(oix._h)
    return np.ctypeslib.as_array(lib.orc_graph_ptr(oix._h),
                                 shape=(oix.n, deg)).copy()


def orc_vectors(oix):
    """Copy of the oracle's current vectors (normalised as stored), [n, dim]."""
    dtype = np.float32 if oix.valuetype == 0 else np.int8
    nbytes = oix.n * oix.dim * np.dtype(dtype).itemsize
    buf = (ctypes.c_char * nbytes).from_address(_lib().orc_vectors_ptr(oix._h))
    return np.frombuffer(buf, dtype=dtype).reshape(oix.n, oix.dim).copy()


# ---------------------------------------------------------------------------
# distance pairs recorded from the reference's own ComputeDistance
# ---------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_dist_pairs = {}


def load_dist_pairs(tag):
    """The committed pairs of `tag` ("f32" or "i8") and what the reference
    computed on them (oracle/gen_golden.py dist): (dims, pairs, ref), where
    pairs[i] is [ppd, 2, dims[i]] (x then y) and ref is float32
    [ndims, ppd, 2] (L2, Cosine). Read once, read-only."""
    if tag not in _dist_pairs:
        dtype = np.float32 if tag == "f32" else np.int8
        raw = open(os.path.join(GOLDEN, f"dist_pairs_{tag}.bin"), "rb").read()
        vt, ndims, ppd = np.frombuffer(raw, dtype=np.int32, count=3)
        assert vt == (0 if tag == "f32" else 1)
        dims = np.frombuffer(raw, dtype=np.int32, count=ndims, offset=12).tolist()
        esz = np.dtype(dtype).itemsize
        off, pairs = 12 + 4 * ndims, []
        for d in dims:
            a = np.frombuffer(raw, dtype=dtype, count=ppd * 2 * d, offset=off)
            pairs.append(a.reshape(ppd, 2, d))
            off += ppd * 2 * d * esz
        assert off == len(raw)
        ref = np.fromfile(os.path.join(GOLDEN, f"dist_ref_{tag}.bin"),
                          dtype=np.float32).reshape(ndims, ppd, 2)
        ref.setflags(write=False)
        _dist_pairs[tag] = (dims, pairs, ref)
    return _dist_pairs[tag]


# ---------------------------------------------------------------------------
# seeded CPU-built indexes
# ---------------------------------------------------------------------------

_built = {}


def built_case(n, dim, vt, dm, algo="BKT", nq=8, seed=0, latent=0):
    """Seeded random index built on the CPU, with queries. Cached per
    argument tuple; callers must not modify what they get.

    With latent = 0 every element is independent. At dims of 60 and more
    such points are all nearly equally far apart, and no graph search
    finds the nearest one within a small MaxCheck. latent = m draws rows
    and queries as m standard-normal factors times a random [m, dim]
    matrix, plus 5% independent noise: full-rank data that a search can
    find its way through."""
    key = (n, dim, vt, dm, algo, nq, seed, latent)
    if key not in _built:
        from sptag_amd.build import build_index_arrays
        rng = np.random.default_rng(7000 + 31 * n + dim + (0 if vt == "f32" else 1)
                                    + 100003 * seed)
        if latent:
            mix = rng.standard_normal((latent, dim)) / np.sqrt(latent)
            draw = lambda m: (rng.standard_normal((m, latent)) @ mix
                              + 0.05 * rng.standard_normal((m, dim)))
        else:
            draw = lambda m: rng.standard_normal((m, dim))
        if vt == "f32":
            x = draw(n).astype(np.float32)
            q = draw(nq).astype(np.float32)
            if dm == "Cosine":
                q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        elif latent:
            x = np.clip(np.rint(draw(n) * 40), -100, 100).astype(np.int8)
            q = np.clip(np.rint(draw(nq) * 40), -100, 100).astype(np.int8)
        else:
            x = rng.integers(-100, 101, (n, dim)).astype(np.int8)
            q = rng.integers(-100, 101, (nq, dim)).astype(np.int8)
        a = build_index_arrays(x, dm, algo=algo, device="cpu", ntrees=2,
                               tpt_leaf=100, cand=64)
        args = (np.ascontiguousarray(a["vectors"]), a["tree_start"],
                a["tree_nodes"], a["graph"], dm)
        for arr in args[:4]:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        q.setflags(write=False)
        _built[key] = {"args": args, "q": q, "n": n, "algo": algo}
    return _built[key]


def orc_from_case(c, deleted=None):
    mk = OrcIndex.from_arrays_kdt if c["algo"] == "KDT" else OrcIndex.from_arrays
    return mk(*c["args"], deleted=deleted)


def gpu_from_case(c, deleted=None):
    from sptag_amd import AnnIndex
    mk = AnnIndex.FromArraysKDT if c["algo"] == "KDT" else AnnIndex.FromArrays
    return mk(*c["args"], deleted=deleted)


# ---------------------------------------------------------------------------
# brute force, independent of the oracle
# ---------------------------------------------------------------------------

def brute_force_topk(vectors, queries, k, dm, deleted=None):
    """Exact top-k by (distance, id) in float64 (exact integers for int8),
    padded with -1. Returns ids only plus the float64 distances: the float
    kernels' rounding is the oracle's business, the order is checked here."""
    x = np.asarray(vectors, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    if dm == "L2":
        d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    else:
        base = 16129.0 if np.asarray(vectors).dtype == np.int8 else 1.0
        d = base - q @ x.T
    ids = np.arange(x.shape[0])
    if deleted is not None:
        keep = np.asarray(deleted) == 0
        d, ids = d[:, keep], ids[keep]
    out = np.full((q.shape[0], k), -1, dtype=np.int64)
    outd = np.full((q.shape[0], k), np.inf)
    for i in range(q.shape[0]):
        order = np.lexsort((ids, d[i]))[:k]
        out[i, :len(order)] = ids[order]
        outd[i, :len(order)] = d[i, order]
    return out, outd


# ---------------------------------------------------------------------------
# iterator drivers
# ---------------------------------------------------------------------------

def orc_iter_open(oix, queries, max_check):
    """One OrcIter per query."""
    return [OrcIter(oix, q, max_check) for q in queries]


def orc_iter_next(its, b):
    """One Next(b) on every iterator: (vids [nq,b], dists [nq,b],
    counts [nq], relaxed [nq]); only the first `count` of a row are results."""
    v = np.empty((len(its), b), dtype=np.int32)
    d = np.empty((len(its), b), dtype=np.float32)
    cnt = np.empty(len(its), dtype=np.int32)
    rel = np.empty(len(its), dtype=np.int32)
    for i, it in enumerate(its):
        cnt[i], v[i], d[i], rel[i] = it.next(b)
    return v, d, cnt, rel


def orc_iter_run(oix, queries, max_check, batches):
    """Drive one OrcIter per query through the Next(batch) sequence; the
    list of orc_iter_next results, one per call."""
    its = orc_iter_open(oix, queries, max_check)
    return [orc_iter_next(its, b) for b in batches]


def assert_iter_calls_equal(gpu_iter, ref_calls, batches, tag=""):
    """Next(batch) on the GPU iterator for every batch in turn; counts,
    flags, and the first `count` ids and distances of every query must equal
    the reference's."""
    for c, (b, (rv, rd, rcnt, rrel)) in enumerate(zip(batches, ref_calls)):
        gv, gd, gcnt, grel = gpu_iter.Next(b)
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=f"{tag} call {c} counts")
        np.testing.assert_array_equal(grel, rrel, err_msg=f"{tag} call {c} relaxed")
        for i in range(len(rcnt)):
            n = rcnt[i]
            np.testing.assert_array_equal(gv[i, :n], rv[i, :n],
                                          err_msg=f"{tag} call {c} query {i} ids")
            np.testing.assert_array_equal(gd[i, :n], rd[i, :n],
                                          err_msg=f"{tag} call {c} query {i} dists")
