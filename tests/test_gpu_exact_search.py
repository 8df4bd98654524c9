"""AnnIndex.ExactSearch / ShardedIndex.ExactSearch: the tiled exact top-k
against the oracle's truth, the scan kernel (`Truth`) on the same handle and,
for int8, float64 brute force. Ids as int32, distances as float32 bit
patterns. For f32 the returned distances are also recomputed in float64: a
chain of at most dim fused steps, each with one rounded subtract (L2) or one
rounded product term (cosine), stays within dim * 2^-23 of the sum of the
terms' magnitudes."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd import AnnIndex, ShardedIndex, load_library
from parity_util import brute_force_topk

pytestmark = pytest.mark.gpu

MAX_K = 1024
N, NQ = 5003, 65            # ragged last row tile and last query tile
TYPES = [("f32", "L2"), ("f32", "Cosine"), ("i8", "L2"), ("i8", "Cosine")]
DIM = {"f32": 40, "i8": 100}


@functools.lru_cache(maxsize=None)
def data(vt, n, d, nq, ties=False):
    """Seeded rows and queries, read-only. ties: 50 distinct vectors of small
    exact integers repeated to n rows, so the order is decided by id alone."""
    rng = np.random.default_rng(9000 + 7 * n + d + (vt == "i8"))
    dtype = np.float32 if vt == "f32" else np.int8
    if ties:
        x = rng.integers(-4, 5, (50, d)).astype(dtype)[np.arange(n) % 50]
        q = rng.integers(-4, 5, (nq, d)).astype(dtype)
    elif vt == "f32":
        x = rng.standard_normal((n, d)).astype(dtype)
        q = rng.standard_normal((nq, d)).astype(dtype)
    else:
        x = rng.integers(-127, 128, (n, d)).astype(dtype)
        q = rng.integers(-127, 128, (nq, d)).astype(dtype)
    for a in (x, q):
        a.setflags(write=False)
    return x, q


def flat_args(x, dm):
    """Arrays of an index whose tree and graph exact search never reads."""
    return (x, np.zeros(1, dtype=np.int32), np.zeros((2, 3), dtype=np.int32),
            np.full((x.shape[0], 2), -1, dtype=np.int32), dm)


def assert_bits_equal(gv, gd, ev, ed, tag):
    assert gv.dtype == np.int32 and gd.dtype == np.float32
    np.testing.assert_array_equal(gv, ev, err_msg=f"{tag} ids")
    np.testing.assert_array_equal(gd.view(np.uint32), ed.view(np.uint32),
                                  err_msg=f"{tag} distance bits")


def check(x, q, dm, ks, deleted=None):
    """ExactSearch at every k of ks against all the expected values."""
    args = flat_args(x, dm)
    gpu = AnnIndex.FromArrays(*args, deleted=deleted)
    orc = OrcIndex.from_arrays(*args, deleted=deleted)
    d = x.shape[1]
    for k in ks:
        gv, gd = gpu.ExactSearch(q, k)
        assert_bits_equal(gv, gd, *orc.truth(q, k), f"k={k} oracle")
        assert_bits_equal(gv, gd, *gpu.Truth(q, k), f"k={k} Truth")
        real = gv >= 0
        if x.dtype == np.int8:
            for lo in range(0, q.shape[0], 8):      # bounds the float64 temporaries
                bv, bd = brute_force_topk(x, q[lo:lo + 8], k, dm, deleted)
                np.testing.assert_array_equal(gv[lo:lo + 8], bv)
                r = real[lo:lo + 8]
                np.testing.assert_array_equal(gd[lo:lo + 8][r], bd[r].astype(np.float32))
            continue
        xs = x[np.where(real, gv, 0)].astype(np.float64)        # [nq, k, d]
        qs = q.astype(np.float64)[:, None, :]
        if dm == "L2":
            d64 = ((qs - xs) ** 2).sum(-1)
            mag = d64
        else:
            d64 = 1.0 - (qs * xs).sum(-1)
            mag = np.abs(qs * xs).sum(-1)
        err = np.abs(gd.astype(np.float64) - d64)[real]
        assert (err <= d * 2.0 ** -23 * mag[real]).all()
    return gpu


@pytest.mark.parametrize("vt,dm,d", [(vt, dm, d) for vt, dm in TYPES for d in
                                     ((16, 40, 100, 131, 128, 768) if vt == "f32"
                                      else (64, 100, 37, 260))])
def test_exact_every_dimension_form(vt, dm, d, monkeypatch):
    """f32: one chunk, 8-tail, 4-tail, scalar tail, fixed form, several
    K-slabs with a streamed query tile; int8: whole K, K padding, odd, guard,
    in one slice, so that every row path carries its data over 40 tiles."""
    if vt == "i8":
        monkeypatch.setenv("SPTAG_AMD_EXACT_SLICES", "1")
    x, q = data(vt, N, d, NQ)
    check(x, q, dm, [10])


@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("n,nq,ks", [(1, 1, [1, 10]), (1, 65, [1]), (65, 1, [10]),
                                     (65, 65, [1, 100]), (5003, 1, [10]),
                                     (5003, 65, [1, MAX_K])])
def test_exact_shapes_and_k(vt, dm, n, nq, ks, monkeypatch):
    """k = 100 at n = 65 pads its tail; k = MAX_K in one slice fills the
    longest lists, so merges move entries in every chunk of them."""
    if MAX_K in ks:
        monkeypatch.setenv("SPTAG_AMD_EXACT_SLICES", "1")
    x, q = data(vt, n, DIM[vt], nq)
    check(x, q, dm, ks)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("slices", [1, 3, 7])
@pytest.mark.parametrize("vt,dm", TYPES)
def test_exact_forced_slices(vt, dm, slices, ties, monkeypatch):
    """Lists cross slice boundaries; with ties each distance occurs about 100
    times across tiles and slices."""
    monkeypatch.setenv("SPTAG_AMD_EXACT_SLICES", str(slices))
    x, q = data(vt, N, DIM[vt], NQ, ties)
    check(x, q, dm, [10, 150])


@pytest.mark.parametrize("mask", ["every_third", "all_but_two", "nearest"])
@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "Cosine")])
def test_exact_delete_masks(vt, dm, mask, monkeypatch):
    monkeypatch.setenv("SPTAG_AMD_EXACT_SLICES", "3")
    x, q = data(vt, N, DIM[vt], NQ)
    deleted = np.zeros(N, dtype=np.uint8)
    if mask == "every_third":
        deleted[::3] = 1
    elif mask == "all_but_two":
        deleted[:] = 1
        deleted[[700, 4999]] = 0
    else:
        deleted[brute_force_topk(x, q, 1, dm)[0][:, 0]] = 1
    gpu = check(x, q, dm, [10], deleted)
    gv = gpu.ExactSearch(q, 3)[0]
    assert not deleted[gv[gv >= 0]].any()


@pytest.mark.parametrize("vt,dm", [("f32", "Cosine"), ("i8", "L2")])
def test_exact_device_pointers_and_kdt_handle(vt, dm):
    import torch
    x, q = data(vt, N, DIM[vt], NQ)
    gpu = AnnIndex.FromArraysKDT(x, np.zeros(1, dtype=np.int32),
                                 np.zeros((2, 4), dtype=np.int32),
                                 np.full((N, 2), -1, dtype=np.int32), dm)
    hv, hd = gpu.ExactSearch(q, 10)
    assert_bits_equal(hv, hd, *AnnIndex.FromArrays(*flat_args(x, dm)).ExactSearch(q, 10),
                      "KDT handle")
    d_q = torch.from_numpy(np.array(q)).to("cuda:0")
    d_v = torch.full((NQ, 10), -7, dtype=torch.int32, device="cuda:0")
    d_d = torch.full((NQ, 10), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.ExactSearchDevice(d_q.data_ptr(), NQ, 10, d_v.data_ptr(), d_d.data_ptr())
    assert_bits_equal(d_v.cpu().numpy(), d_d.cpu().numpy(), hv, hd, "device form")


@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "Cosine")])
def test_exact_shard_set_equals_unsplit(vt, dm):
    x, q = data(vt, N, DIM[vt], NQ)
    whole = AnnIndex.FromArrays(*flat_args(x, dm))
    sh = ShardedIndex.FromIndexes([AnnIndex.FromArrays(*flat_args(x[lo:hi], dm))
                                   for lo, hi in [(0, 4000), (4000, 4998), (4998, N)]])
    for k in (1, 10, 200):
        assert_bits_equal(*sh.ExactSearch(q, k), *whole.ExactSearch(q, k), f"k={k}")


def test_exact_argument_errors():
    lib = load_library()
    x, q = data("f32", 65, 40, 1)
    gpu = AnnIndex.FromArrays(*flat_args(x, "L2"))
    v = np.empty(MAX_K + 1, dtype=np.int32)
    d = np.empty(MAX_K + 1, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for fn in (lib.sptag_amd_exact_search, lib.sptag_amd_exact_search_device):
        for args in [(gpu._h, p(q), 1, 0, p(v), p(d)),
                     (gpu._h, p(q), 1, MAX_K + 1, p(v), p(d)),
                     (gpu._h, p(q), 0, 10, p(v), p(d)),
                     (None, p(q), 1, 10, p(v), p(d)),
                     (gpu._h, None, 1, 10, p(v), p(d)),
                     (gpu._h, p(q), 1, 10, None, p(d)),
                     (gpu._h, p(q), 1, 10, p(v), None)]:
            assert fn(*args) == -2, args[2:4]       # SPTAG_AMD_ERR_PARAM
    assert lib.sptag_amd_shards_exact_search(None, p(q), 1, 10, p(v), p(d)) == -2
