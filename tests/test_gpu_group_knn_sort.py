"""The sorted selection of grouped kNN (selection="sort" / "auto") against a
numpy reference: all pairwise distances of a group in exact integer
arithmetic, then a lexicographic sort by (dist, vid) with self removed. The
data makes the reference exact: int8 as it is, f32 with integer coordinates
in [-8, 8], whose every partial sum is exact in f32 in any order. Such data is
full of ties, cosine distances go negative, and ids and distance bits are
compared for equality; "stream" must give the same bytes."""
import functools

import numpy as np
import pytest

from sptag_amd import (AnnIndex, SptagAmdError, group_knn_device, group_knn_sort_max,
                       VT_FLOAT, VT_INT8)
from test_gpu_exact_search import TYPES, assert_bits_equal, flat_args

pytestmark = pytest.mark.gpu

T = 32      # the kernels' query tile
MAXDIST = np.float32(np.finfo(np.float32).max) / np.float32(10)
# alone, a pair, around the query tile, around one 64-lane chunk
SMALL = (1, 2, T - 1, T, T + 1, 63, 64, 65)
FORMS = [("f32", 1), ("f32", 7), ("f32", 128), ("f32", 768), ("i8", 3), ("i8", 100), ("i8", 128)]


@functools.lru_cache(maxsize=None)
def case(vt, dm, d, counts, k):
    """(x, members, starts, counts, expected vids, expected dists): members a
    seeded shuffle, 20 vids in no group, the 64-member group (if there is
    one) of identical vectors, so that vid alone orders it."""
    counts = np.array(counts, dtype=np.int32)
    starts = (np.cumsum(counts) - counts).astype(np.int32)
    n = int(counts.sum()) + 20
    rng = np.random.default_rng(1000 * d + len(counts))
    x = (rng.integers(-8, 9, (n, d)).astype(np.float32) if vt == "f32"
         else rng.integers(-127, 128, (n, d)).astype(np.int8))
    members = rng.permutation(n).astype(np.int32)
    ev = np.full((n, k), -1, dtype=np.int32)
    ed = np.full((n, k), MAXDIST, dtype=np.float32)
    for s, c in zip(starts, counts):
        m = members[s:s + c]
        if c == 64:
            x[m] = x[m[0]]
        g = x[m].astype(np.float64)         # integers: every product and sum is exact
        sq = (g * g).sum(1)
        D = (sq[:, None] + sq[None, :] - 2 * g @ g.T if dm == "L2"
             else (1.0 if vt == "f32" else 16129.0) - g @ g.T)
        for i, v in enumerate(m):
            o = np.lexsort((m, D[i]))
            o = o[o != i][:k]
            ev[v, :len(o)] = m[o]
            ed[v, :len(o)] = D[i][o]
    assert dm == "L2" or (ed < 0).any()
    return x, members, starts, counts, ev, ed


@pytest.mark.parametrize("k", [1, T, 64, 70])
@pytest.mark.parametrize("dm", ["L2", "Cosine"])
@pytest.mark.parametrize("vt,d", FORMS)
def test_sort_small_groups_every_form(vt, d, dm, k):
    """k = 1; k = group - 1, group, group + 5 for the groups around 32 and 64;
    every dimension form, the streamed-query f32 form and byte-wise int8."""
    x, members, starts, counts, ev, ed = case(vt, dm, d, SMALL, k)
    gpu = AnnIndex.FromArrays(*flat_args(x, dm))
    for sel in ("sort", "auto", "stream"):
        assert_bits_equal(*gpu.GroupKnn(members, starts, counts, k, selection=sel), ev, ed, sel)


@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("k", [64, 1024])
def test_sort_at_the_cap_and_mixed_launch(vt, dm, k):
    """Groups of C - 1 and C sorted (k = 1024 takes all of them and pads);
    with C + 1 in the call "auto" streams that group and "sort" refuses the
    call, leaving prefilled outputs as they were. The device form agrees."""
    import torch
    d = 128 if vt == "f32" else 100
    C = group_knn_sort_max(VT_FLOAT if vt == "f32" else VT_INT8, d)
    assert C >= 1024
    x, members, starts, counts, ev, ed = case(vt, dm, d, (C - 1, C, C + 1, 2), k)
    gpu = AnnIndex.FromArrays(*flat_args(x, dm))
    assert_bits_equal(*gpu.GroupKnn(members, starts, counts, k, selection="auto"), ev, ed, "auto")
    assert_bits_equal(*gpu.GroupKnn(members, starts, counts, k), ev, ed, "stream")
    fit = [0, 1, 3]
    sv, sd = gpu.GroupKnn(members, starts[fit], counts[fit], k, selection="sort")
    rows = np.concatenate([members[s:s + c] for s, c in zip(starts[fit], counts[fit])])
    assert_bits_equal(sv[rows], sd[rows], ev[rows], ed[rows], "sort")
    assert (sv[members[starts[2]:starts[2] + C + 1]] == -1).all()

    n = x.shape[0]
    d_x = torch.from_numpy(x).to("cuda:0")
    d_m = torch.from_numpy(members).to("cuda:0")
    d_v = torch.full((n, k), -7, dtype=torch.int32, device="cuda:0")
    d_d = torch.full((n, k), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dev = lambda st, ct: group_knn_device(
        d_x.data_ptr(), VT_FLOAT if vt == "f32" else VT_INT8, dm, n, d, d_m.data_ptr(), n,
        st, ct, k, d_v.data_ptr(), d_d.data_ptr(), selection="sort")
    with pytest.raises(SptagAmdError) as err:
        dev(starts, counts)
    assert err.value.code == -2                         # SPTAG_AMD_ERR_PARAM
    assert (d_v == -7).all() and (d_d == -7.0).all()
    dev(starts[fit], counts[fit])
    assert_bits_equal(d_v.cpu().numpy(), d_d.cpu().numpy(), sv, sd, "device form")


def test_build_with_hip_sort_equals_hip():
    from sptag_amd.build import build_rng_graph
    x = np.random.default_rng(5).standard_normal((3001, 40)).astype(np.float32)
    kw = dict(tpt_leaf=200, ntrees=2, device="cuda:0")
    for a, b in zip(build_rng_graph(x, leaf_knn="hip_sort", **kw),
                    build_rng_graph(x, leaf_knn="hip", **kw)):
        assert a.dtype == b.dtype and (a.view(a.dtype).cpu().numpy().view(np.uint8) ==
                                       b.cpu().numpy().view(np.uint8)).all()
    with pytest.raises(ValueError, match="leaf_knn"):
        build_rng_graph(x, leaf_knn="sort", **kw)
