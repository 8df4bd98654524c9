"""AnnIndex.PoolJoin / pool_join_device against a plain restatement of the
contract, one row at a time. On small exact integers every distance is exact
in f32 and float64 alike, so ids and distances are compared exactly; for
generic f32 the expected distances are the oracle's (the reference-order
contract). Every data-driven case checks on the EXPECTED output that it holds
a row cut at kout with valid entries left over, a row that ends in padding, a
dropped pool/new duplicate and a dropped repeat."""
import ctypes

import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd import AnnIndex, load_library, pool_join_device
from test_gpu_exact_search import data, flat_args, TYPES, DIM  # noqa: F401 (data: via vectors)
from test_gpu_rng_prune import vectors, pair_matrix, pools, handle, N, ROWS, BIG_N, BIG_ROWS

pytestmark = pytest.mark.gpu


def lists(vt, dm, n, d, kind, rows, npool, nnew):
    """Old pools: the npool nearest others, some entries at inf, every third
    row half empty. New lists: random ids, three ids of the row's pool (one of
    them an inf entry's), a repeated id, the node and -1; every third row
    mostly -1."""
    nodes, pid, pdd = pools(vt, dm, n, d, kind, rows, npool)
    pid, pdd = pid.copy(), pdd.copy()
    rng = np.random.default_rng(5 + npool + nnew)
    new = rng.integers(0, n, (rows, nnew)).astype(np.int32)
    if npool > 3:
        pdd[::4, 3] = np.inf
        pid[::3, npool // 2:], pdd[::3, npool // 2:] = -1, np.inf
    if nnew >= 8:
        if npool > 3:
            new[:, :3] = pid[:, [0, 3, npool // 2 - 1]]
        new[:, 4] = new[:, 5]
        new[:, 6] = nodes
        new[:, 7] = -1
    if nnew > 1:
        new[::3, max(nnew // 4, 1):] = -1
    return nodes, pid, pdd, new


def ref_join(dist, nodes, pid, pdd, new, ndd, kout):
    """The contract. dist(node, id): the f32 distance, asked once per
    surviving new id. Returns ids, dists and (rows cut at kout, rows that end
    in padding, dropped pool/new duplicates, dropped repeats)."""
    out_i = np.full((len(nodes), kout), -1, dtype=np.int32)
    out_d = np.full((len(nodes), kout), np.inf, dtype=np.float32)
    cut = padded = dups = reps = 0
    for r, node in enumerate(nodes):
        ok = lambda i, v: i >= 0 and i != node and np.isfinite(v)
        old, fresh = {}, {}
        for i, v in zip(pid[r], pdd[r]):
            if ok(i, v):
                old[i] = min(old.get(i, np.inf), v)
        for j, i in enumerate(new[r]):
            v = 0.0 if ndd is None else ndd[r][j]
            if not ok(i, v):
                continue
            if i in old:
                dups += 1
                continue
            reps += i in fresh
            if ndd is None:
                v = fresh[i] if i in fresh else dist(node, i)
            fresh[i] = min(fresh.get(i, np.inf), v)
        # + 0: a given -0.0 counts as 0.0
        ent = sorted((np.float32(v) + np.float32(0), i) for i, v in {**old, **fresh}.items())
        cut += len(ent) > kout
        padded += len(ent) < kout
        ent = ent[:kout]
        out_i[r, :len(ent)] = [i for _, i in ent]
        out_d[r, :len(ent)] = [v for v, _ in ent]
    return out_i, out_d, (cut, padded, dups, reps)


def matrix_dist(vt, dm, n, d, kind):
    P = pair_matrix(vt, dm, n, d, kind)
    return lambda node, i: np.float32(P[node, i])


def check(vt, dm, n, d, kind, nodes, pid, pdd, new, kout, ndd=None, dist=None, nonvacuous=True):
    exp_i, exp_d, stats = ref_join(dist or matrix_dist(vt, dm, n, d, kind), nodes, pid, pdd, new,
                                   ndd, kout)
    print("cut %d padded %d duplicates %d repeats %d" % stats)
    if nonvacuous:
        assert all(s > 0 for s in stats), stats
    pool = (pid, pdd) if pid.shape[1] else (None, None)
    ids, dists = handle(vt, dm, n, d, kind).PoolJoin(nodes, *pool, new, kout, ndd)
    assert ids.dtype == np.int32 and dists.dtype == np.float32
    np.testing.assert_array_equal(ids, exp_i)
    np.testing.assert_array_equal(dists, exp_d)
    return exp_i, exp_d


@pytest.mark.parametrize("vt,dm,d,kind", [("f32", dm, d, "ints") for dm in ("L2", "Cosine")
                                          for d in (16, 40, 131, 128, 768)] +
                         [("i8", dm, d, "ints") for dm in ("L2", "Cosine") for d in (64, 100, 37)] +
                         [("f32", dm, d, "real") for dm in ("L2", "Cosine") for d in (40, 131)])
def test_pool_join_every_dimension_form(vt, dm, d, kind):
    dist = None
    if kind == "real":
        x = vectors(vt, N, d, kind)
        orc = OrcIndex.from_arrays(*flat_args(x, dm))
        dist = lambda node, i: np.float32(orc.distance(x[node], x[i]))
    check(vt, dm, N, d, kind, *lists(vt, dm, N, d, kind, ROWS, 64, 72), 64, dist=dist)


# (3, 16, 8) and (3, 33, 64): new lists one short of and one past whole tiles of 16
@pytest.mark.parametrize("npool,nnew,kout", [
    (0, 1, 1), (0, 40, 64), (64, 0, 16), (256, 272, 256), (15, 17, 40), (3, 16, 8), (3, 33, 64),
    (1024, 1024, 1024)])
@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "L2")])
def test_pool_join_list_and_tile_boundaries(vt, dm, npool, nnew, kout):
    n, rows = (BIG_N, BIG_ROWS) if npool > 256 else (N, ROWS)
    check(vt, dm, n, DIM[vt], "ints", *lists(vt, dm, n, DIM[vt], "ints", rows, npool, nnew), kout,
          nonvacuous=npool >= 256)


@pytest.mark.parametrize("vt,dm", TYPES)
def test_pool_join_ties(vt, dm):
    exp_i, exp_d = check(vt, dm, N, DIM[vt], "ties",
                         *lists(vt, dm, N, DIM[vt], "ties", ROWS, 64, 72), 64)
    same = (exp_d[:, 1:] == exp_d[:, :-1]) & (exp_i[:, 1:] >= 0)
    assert same.sum() > ROWS and (exp_i[:, 1:][same] > exp_i[:, :-1][same]).all()


# 256 + 64 is the one-wave kernel, 300 + 300 the four-wave one
@pytest.mark.parametrize("npool,nnew", [(256, 64), (300, 300)])
def test_pool_join_given_distances(npool, nnew):
    vt, dm, d = "f32", "L2", DIM["f32"]
    nodes, pid, pdd, new = lists(vt, dm, N, d, "ints", ROWS, npool, nnew)
    P = pair_matrix(vt, dm, N, d, "ints")
    ndd = (np.take_along_axis(P[:ROWS], new.clip(0), 1) + 3.0).astype(np.float32)
    ndd[:, 4] += 1.0                                # the repeat: its later copy is nearer
    ndd[1::5, 10], ndd[2::5, 11] = np.inf, np.nan
    new[:, 8:10] = -np.sort(-new[:, 8:10], axis=1)  # id of -0.0 above the id of 0.0
    ndd[:, 8], ndd[:, 9] = -0.0, 0.0
    exp_i, exp_d = check(vt, dm, N, d, "ints", nodes, pid, pdd, new, npool, ndd=ndd)
    # a pool/new duplicate kept the pool's distance, not the given new one
    at = exp_i[1] == pid[1, 0]
    assert at.sum() == 1 and exp_d[1][at] == pdd[1, 0] != ndd[1, 0]


@pytest.mark.parametrize("vt,dm", [("f32", "Cosine"), ("i8", "L2")])
def test_pool_join_in_place_and_kdt_handle(vt, dm):
    import torch
    d = DIM[vt]
    nodes, pid, pdd, new = lists(vt, dm, N, d, "ints", ROWS, 64, 72)
    exp_i, exp_d = check(vt, dm, N, d, "ints", nodes, pid, pdd, new, 64)
    ids, dists = handle(vt, dm, N, d, "ints", kdt=True).PoolJoin(nodes, pid, pdd, new, 64)
    np.testing.assert_array_equal(ids, exp_i)
    np.testing.assert_array_equal(dists, exp_d)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    tx, tn, ti, td, tw = dev(vectors(vt, N, d, "ints")), dev(nodes), dev(pid), dev(pdd), dev(new)
    torch.cuda.synchronize()
    pool_join_device(tx.data_ptr(), 0 if vt == "f32" else 1, dm, N, d, tn.data_ptr(), ROWS,
                     ti.data_ptr(), td.data_ptr(), 64, tw.data_ptr(), None, 72, 64,
                     ti.data_ptr(), td.data_ptr())
    np.testing.assert_array_equal(ti.cpu().numpy(), exp_i)
    np.testing.assert_array_equal(td.cpu().numpy(), exp_d)


def test_pool_join_argument_errors():
    lib = load_library()
    nodes, pid, pdd, new = lists("f32", "L2", N, 40, "ints", ROWS, 64, 72)
    gpu = handle("f32", "L2", N, 40, "ints")
    oi = np.full((ROWS, 64), -7, dtype=np.int32)
    od = np.full((ROWS, 64), -7, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def changed(a, i, val):
        b = a.copy()
        b[i] = val
        return b
    good = (gpu._h, p(nodes), ROWS, p(pid), p(pdd), 64, p(new), None, 72, 64, p(oi), p(od))
    bad = [{i: None} for i in (0, 1, 3, 4, 6, 10, 11)]
    bad += [{2: 0}, {5: -1}, {5: 1025}, {8: -1}, {8: 1025}, {9: 0}, {9: 1025}, {5: 0, 8: 0},
            {1: p(changed(nodes, 3, -1))}, {1: p(changed(nodes, 3, N))},
            {3: p(changed(pid, (5, 5), N))}, {6: p(changed(new, (5, 5), N))}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_pool_join(*args) == -2, b         # SPTAG_AMD_ERR_PARAM
    assert (oi == -7).all() and (od == -7).all()

    # the device form returns before it touches the device: any non-null
    # address stands for the buffers
    x = vectors("f32", N, 40, "ints")
    good = (0, p(x), 0, 0, N, 40, p(nodes), ROWS, p(pid), p(pdd), 64, p(new), None, 72, 64,
            p(oi), p(od))
    bad = [{i: None} for i in (1, 6, 8, 9, 11, 15, 16)]
    bad += [{7: 0}, {10: -1}, {10: 1025}, {13: -1}, {13: 1025}, {14: 0}, {14: 1025},
            {10: 0, 13: 0}, {2: 2}, {3: 2}, {4: 0}, {5: 0}, {5: 4097}, {2: 1, 5: 261}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_pool_join_device(*args) == -2, b
    assert (oi == -7).all() and (od == -7).all()


def test_pool_join_builder_plumbing():
    import torch
    from sptag_amd import build
    x = np.array(vectors("f32", N, 40, "ints"))     # writable, for torch
    xf = torch.from_numpy(x).to("cuda:0")
    nodes, pid, pdd, new = lists("f32", "L2", N, 40, "ints", ROWS, 64, 72)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    ids, dists = build._pool_join_hip(xf, dev(pid), dev(pdd), dev(new), None, 64, dev(nodes))
    want = handle("f32", "L2", N, 40, "ints").PoolJoin(nodes, pid, pdd, new, 64)
    np.testing.assert_array_equal(ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(dists.cpu().numpy(), want[1])
    cpu = [torch.from_numpy(a) for a in (pid, pdd, new)]
    with pytest.raises(RuntimeError, match="GPU"):
        build._pool_join_hip(xf.cpu(), *cpu, None, 64, torch.from_numpy(nodes))
    with pytest.raises(RuntimeError, match="GPU"):
        build.build_rng_graph(x, device="cpu", join="hip")
    with pytest.raises(ValueError, match="join"):
        build.build_index_arrays(x, "L2", join="cuda")

    kw = dict(tpt_leaf=100, ntrees=2, device="cuda:0", refine_rounds=1)
    graph = build.build_index_arrays(x, "L2", join="hip", prune="hip", leaf_knn="hip",
                                     **kw)["graph"]
    assert graph.shape == (N, 32) and graph.dtype == np.int32
    assert graph.min() >= -1 and graph.max() < N
    assert not (graph == np.arange(N)[:, None]).any()
    np.testing.assert_array_equal(
        build.build_index_arrays(x, "L2", join="torch", **kw)["graph"],
        build.build_index_arrays(x, "L2", **kw)["graph"])
