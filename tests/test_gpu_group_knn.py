"""AnnIndex.GroupKnn / group_knn_device: exact kNN inside row groups against
the oracle's truth over each group alone. A group's members are sorted, so
the oracle's local-id tie order is the vid order; the row's own vid is dropped
from its k + 1 nearest if it is there (with un-normalised f32 cosine a row
need not be its own nearest). Ids as int32, distances as float32 bit patterns;
int8 also against float64 brute force."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd import AnnIndex, group_knn_device, load_library
from parity_util import brute_force_topk
from test_gpu_exact_search import MAX_K, TYPES, DIM, assert_bits_equal, data, flat_args

pytestmark = pytest.mark.gpu

N = 2003
# alone, a pair, around the 32-query tile, past one 128-row int8 tile, several
# tiles with a ragged last one; members[1228:] are in no group
COUNTS = (1, 2, 31, 32, 33, 129, 300, 700)
MAXDIST = np.float32(np.finfo(np.float32).max) / np.float32(10)


@functools.lru_cache(maxsize=None)
def case(vt, d, counts=COUNTS, ties=False):
    """(x [N, d], members, starts, counts): members a seeded shuffle of all
    vids, so no group is in vid order; group g is the next counts[g] of them."""
    x = data(vt, N, d, 1, ties)[0]
    members = np.random.default_rng(77).permutation(N).astype(np.int32)
    counts = np.array(counts, dtype=np.int32)
    starts = (np.cumsum(counts) - counts).astype(np.int32)
    return x, members, starts, counts


def reference(x, dm, members, starts, counts, k):
    """Expected (vids, dists) by the oracle and, for int8, the expected ids by
    float64 brute force (else None)."""
    n = x.shape[0]
    ev = np.full((n, k), -1, dtype=np.int32)
    ed = np.full((n, k), MAXDIST, dtype=np.float32)
    bv = ev.copy() if x.dtype == np.int8 else None
    for s, c in zip(starts, counts):
        sm = np.sort(members[s:s + c])
        xs = x[sm]
        tv, td = OrcIndex.from_arrays(*flat_args(xs, dm)).truth(xs, k + 1)
        lists = [(tv, ev)]
        if bv is not None:
            lists.append((np.concatenate([brute_force_topk(xs, xs[lo:lo + 64], k + 1, dm)[0]
                                          for lo in range(0, c, 64)]), bv))
        for loc, out in lists:
            for i, v in enumerate(sm):
                keep = (loc[i] >= 0) & (sm[loc[i]] != v)
                m = min(k, int(keep.sum()))
                out[v, :m] = sm[loc[i][keep]][:m]
                if out is ev:
                    ed[v, :m] = td[i][keep][:m]
    return ev, ed, bv


def check(x, dm, members, starts, counts, ks):
    gpu = AnnIndex.FromArrays(*flat_args(x, dm))
    for k in ks:
        gv, gd = gpu.GroupKnn(members, starts, counts, k)
        ev, ed, bv = reference(x, dm, members, starts, counts, k)
        assert_bits_equal(gv, gd, ev, ed, f"k={k} oracle")
        if bv is not None:
            np.testing.assert_array_equal(gv, bv, err_msg=f"k={k} float64 ids")
    return gpu


@pytest.mark.parametrize("vt,dm,d", [(vt, dm, d) for vt, dm in TYPES for d in
                                     ((16, 40, 131, 128, 768) if vt == "f32"
                                      else (64, 100, 37, 260))])
def test_group_knn_mixed_groups_every_dimension_form(vt, dm, d):
    """One call over groups of every size class. f32: one chunk, 8-tail,
    scalar tail (dword loads), 16-byte loads, streamed query slabs; int8:
    16-byte rows, dword rows, byte rows, the dim guard."""
    x, members, starts, counts = case(vt, d)
    check(x, dm, members, starts, counts, [10])


@pytest.mark.parametrize("vt,dm", TYPES)
def test_group_knn_k_extremes(vt, dm):
    """k = 64 pads the tails of the groups below 65 members; k = MAX_K over
    one group of 1500 moves entries in every 64-chunk of the lists."""
    x, members, starts, counts = case(vt, DIM[vt])
    check(x, dm, members, starts, counts, [1, 64])
    check(x, dm, *case(vt, DIM[vt], (1500,))[1:], [MAX_K])


@pytest.mark.parametrize("vt,dm", TYPES)
def test_group_knn_ties_are_decided_by_vid(vt, dm):
    """50 distinct vectors over all rows: each distance occurs many times in a
    group, and rows arrive in member order, not vid order."""
    x, members, starts, counts = case(vt, DIM[vt], ties=True)
    check(x, dm, members, starts, counts, [10, 150])


@pytest.mark.parametrize("vt,dm", TYPES)
def test_group_knn_device_form_and_kdt_handle(vt, dm):
    """The handle-free form over torch tensors writes every row of outputs
    pre-filled with a sentinel and equals the host form bit for bit."""
    import torch
    x, members, starts, counts = case(vt, DIM[vt])
    hv, hd = AnnIndex.FromArrays(*flat_args(x, dm)).GroupKnn(members, starts, counts, 10)
    kdt = AnnIndex.FromArraysKDT(x, np.zeros(1, dtype=np.int32),
                                 np.zeros((2, 4), dtype=np.int32),
                                 np.full((N, 2), -1, dtype=np.int32), dm)
    assert_bits_equal(*kdt.GroupKnn(members, starts, counts, 10), hv, hd, "KDT handle")
    d_x = torch.from_numpy(np.array(x)).to("cuda:0")
    d_m = torch.from_numpy(members).to("cuda:0")
    d_v = torch.full((N, 10), -7, dtype=torch.int32, device="cuda:0")
    d_d = torch.full((N, 10), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    group_knn_device(d_x.data_ptr(), 0 if vt == "f32" else 1, dm, N, x.shape[1],
                     d_m.data_ptr(), N, starts, counts, 10, d_v.data_ptr(), d_d.data_ptr())
    assert_bits_equal(d_v.cpu().numpy(), d_d.cpu().numpy(), hv, hd, "device form")
    assert (hv[members[counts.sum():]] == -1).all() and (hv[members[0]] == -1).all()


def test_group_knn_argument_errors():
    lib = load_library()
    x, members, starts, counts = case("f32", 40)
    gpu = AnnIndex.FromArrays(*flat_args(x, "L2"))
    ng, nm = len(counts), len(members)
    v = np.full((N, 2), -7, dtype=np.int32)
    d = np.full((N, 2), -7.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def changed(a, i, val):
        b = a.copy()
        b[i] = val
        return b
    good = (gpu._h, p(members), nm, p(starts), p(counts), ng, 2, p(v), p(d))
    bad = [{i: None} for i in (0, 1, 3, 4, 7, 8)]
    bad += [{6: 0}, {6: MAX_K + 1}, {5: 0}, {2: 1227},       # the last group ends at 1228
            {4: p(changed(counts, 3, -1))}, {3: p(changed(starts, 7, N - 699))},
            {3: p(changed(starts, 1, 0))},                   # groups 0 and 1 overlap
            {1: p(changed(members, 5, -1))}, {1: p(changed(members, 5, N))},
            {1: p(changed(members, 1500, members[3]))}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_group_knn(*args) == -2, b         # SPTAG_AMD_ERR_PARAM
    assert (v == -7).all() and (d == -7.0).all()

    # the device form returns before it touches the device: any non-null
    # address stands for the buffers
    good = (0, p(x), 0, 0, N, 40, p(members), nm, p(starts), p(counts), ng, 2, p(v), p(d))
    bad = [{i: None} for i in (1, 6, 8, 9, 12, 13)]
    bad += [{11: 0}, {11: MAX_K + 1}, {10: 0}, {7: 1227}, {9: p(changed(counts, 3, -1))},
            {2: 2}, {3: 2}, {4: 0}, {5: 0}, {2: 1, 5: 261}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_group_knn_device(*args) == -2, b


def test_group_knn_builder_plumbing():
    import torch
    from sptag_amd import build
    x = np.array(data("f32", N, 40, 1)[0])      # writable, for torch
    xf = torch.from_numpy(x).to("cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(3)
    perm, starts, counts = build._tpt_leaves(xf, 100, gen)
    ids, dst = build._leaf_knn_hip(xf, perm, starts, counts, 64)
    gv, gd = AnnIndex.FromArrays(*flat_args(x, "L2")).GroupKnn(
        perm.cpu().numpy(), starts.cpu().numpy(), counts.cpu().numpy(), 64)
    gd[gv < 0] = np.inf
    assert_bits_equal(ids.cpu().numpy(), dst.cpu().numpy(), gv, gd, "hip leaf step")
    with pytest.raises(RuntimeError, match="GPU"):
        build._leaf_knn_hip(xf.cpu(), perm.cpu(), starts.cpu(), counts.cpu(), 64)

    kw = dict(tpt_leaf=100, ntrees=2, device="cuda:0")
    graph = build.build_index_arrays(x, "L2", leaf_knn="hip", **kw)["graph"]
    assert graph.shape == (N, 32) and graph.dtype == np.int32
    assert graph.min() >= -1 and graph.max() < N
    assert not (graph == np.arange(N)[:, None]).any()
    np.testing.assert_array_equal(
        build.build_index_arrays(x, "L2", leaf_knn="torch", **kw)["graph"],
        build.build_index_arrays(x, "L2", **kw)["graph"])
