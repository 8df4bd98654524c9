"""AnnIndex.KmeansAssign / kmeans_assign_device against a plain restatement of
the contract, one member at a time. On small exact integers every distance
and every sum is exact in f32 and float64 alike, so all outputs are compared
exactly; for generic f32 the expected distances are the oracle's (the
reference-order contract) and the sums are held to the bound of an f32 sum in
any order. Every data-driven case checks on the EXPECTED output that it holds
an empty center and a member whose two best centers tie."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd import load_library, kmeans_assign_device
from test_gpu_exact_search import data, flat_args, TYPES, DIM  # noqa: F401 (data: via vectors)
from test_gpu_rng_prune import vectors, pair_matrix, handle, N, BIG_N

pytestmark = pytest.mark.gpu

MAXDIST = np.float32(np.finfo(np.float32).max) / np.float32(10)
KMAX = 64
# sizes 0 and 1, one below, at and above the member tile of f32 (16) and of
# int8 (64), and more than two tiles of either; three list places in no segment
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 200]
NCENT = [1, 1, 2, 31, 32, 33, 64, 2, 64]


def layout(n, sizes, ncent, seed=3):
    """A shuffled member list cut into segments, a gap of 3 places before the
    last; centers are vectors of the segment's members, the last a repeat of
    the first. Returns members, starts, sizes, ncenters, center ids."""
    rng = np.random.default_rng(seed)
    members = rng.permutation(n).astype(np.int32)
    sizes = np.array(sizes, dtype=np.int32)
    starts = (np.cumsum(sizes) - sizes).astype(np.int32)
    starts[-1] += 3
    ncent = np.array(ncent, dtype=np.int32)
    cid = np.zeros((len(sizes), KMAX), dtype=np.int32)
    for s, (st, sz, nc) in enumerate(zip(starts, sizes, ncent)):
        if sz:
            cid[s, :nc] = members[st + (np.arange(nc) * 7) % sz]
            cid[s, nc - 1] = cid[s, 0]
    return members, starts, sizes, ncent, cid


def center_rows(x, cid, ncent):
    """[nseg, KMAX, d] in x's type; rows past ncenters hold NaN (f32) or 127"""
    c = x[cid].copy()
    for s, nc in enumerate(ncent):
        c[s, nc:] = np.nan if x.dtype == np.float32 else 127
    return c


def ref_assign(dist, x, members, starts, sizes, ncent, update, pc=None, lam=None):
    """The contract. dist(s, vid): f32 D(x[vid], center_k) for k < ncenters[s].
    Untouched entries hold -7. Returns the six outputs and (empty centers,
    members whose best two centers tie, centers whose extreme two places
    share)."""
    nseg, d = len(starts), x.shape[1]
    labels = np.full(len(members), -7, dtype=np.int32)
    dists = np.full(len(members), -7, dtype=np.float32)
    counts = np.full((nseg, KMAX), -7, dtype=np.int32)
    cidx = np.full((nseg, KMAX), -7, dtype=np.int32)
    cdist = np.full((nseg, KMAX), -7, dtype=np.float32)
    sums = np.full((nseg, KMAX, d), -7, dtype=np.float64)
    ties = shared = 0
    for s in range(nseg):
        nc = ncent[s]
        counts[s, :nc], cidx[s, :nc], sums[s, :nc] = 0, -1, 0
        cdist[s, :nc] = -MAXDIST if update else MAXDIST
        for i in range(sizes[s]):
            vid = members[starts[s] + i]
            dk = dist(s, vid)
            if lam is not None:
                with np.errstate(over="ignore"):
                    dk = dk + np.float32(lam[s]) * pc[s, :nc].astype(np.float32)
            lab, small = 0, MAXDIST
            for k in range(nc):
                if dk[k] > -MAXDIST and dk[k] < small:
                    lab, small = k, dk[k]
            ties += small < MAXDIST and (dk == small).sum() > 1
            labels[starts[s] + i], dists[starts[s] + i] = lab, small
            counts[s, lab] += 1
            sums[s, lab] += x[vid].astype(np.float64)
            if small > cdist[s, lab] if update else small <= cdist[s, lab]:
                cidx[s, lab], cdist[s, lab] = vid, small
        seg = slice(starts[s], starts[s] + sizes[s])
        shared += sum(((labels[seg] == k) & (dists[seg] == cdist[s, k])).sum() > 1
                      for k in range(nc))
    empty = sum((counts[s, :ncent[s]] == 0).sum() for s in range(nseg))
    return (labels, dists, counts, cidx, cdist, sums), (empty, ties, shared)


def matrix_dist(vt, dm, n, d, kind, cid, ncent):
    P = pair_matrix(vt, dm, n, d, kind)
    return lambda s, vid: P[vid, cid[s, :ncent[s]]].astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_dist(dm, n, d):
    """real f32: the oracle's distance, each (vid, center id) pair asked once"""
    x = vectors("f32", n, d, "real")
    orc = OrcIndex.from_arrays(*flat_args(x, dm))
    return functools.lru_cache(maxsize=None)(
        lambda vid, c: np.float32(orc.distance(x[vid], x[c])))


def run(gpu, x, members, starts, sizes, ncent, cid, update, pc=None, lam=None):
    """KmeansAssign with the untouched entries set to the reference's -7"""
    got = list(gpu.KmeansAssign(members, starts, sizes, center_rows(x, cid, ncent), ncent, update,
                                pc, lam))
    inseg = np.zeros(len(members), dtype=bool)
    for st, sz in zip(starts, sizes):
        inseg[st:st + sz] = True
    assert (got[0][~inseg] == 0).all() and (got[1][~inseg] == 0).all()
    got[0][~inseg], got[1][~inseg] = -7, -7
    past = np.arange(KMAX)[None, :] >= ncent[:, None]
    for a in got[2:5] + ([got[5]] if update else []):
        assert (a[past] == 0).all()
        a[past] = -7
    return got


def check(vt, dm, n, d, kind, lay, update, pc=None, lam=None, dist=None, nonvacuous=True):
    members, starts, sizes, ncent, cid = lay
    x = vectors(vt, n, d, kind)
    exp, stats = ref_assign(dist or matrix_dist(vt, dm, n, d, kind, cid, ncent), x, members,
                            starts, sizes, ncent, update, pc, lam)
    print("empty centers %d, tied members %d, shared extremes %d" % stats)
    if nonvacuous:
        assert stats[0] > 0 and stats[1] > 0, stats
    got = run(handle(vt, dm, n, d, kind), x, members, starts, sizes, ncent, cid, update, pc, lam)
    for g, e in zip(got[:5], exp[:5]):
        assert g.dtype == e.dtype
        np.testing.assert_array_equal(g, e)
    if not update:
        assert got[5] is None
    elif kind != "real":
        np.testing.assert_array_equal(got[5], exp[5].astype(np.float32))
    else:
        # an f32 sum of m terms in any order: (m - 1) * 2^-24 * sum |x_j| per coordinate
        mag = np.zeros_like(exp[5])
        for s, (st, sz) in enumerate(zip(starts, sizes)):
            np.add.at(mag[s], exp[0][st:st + sz], np.abs(x[members[st:st + sz]]).astype(np.float64))
        m = np.maximum(exp[2], 1)[..., None]
        past = np.arange(KMAX)[None, :] >= ncent[:, None]
        err = np.abs(got[5].astype(np.float64) - exp[5])
        assert (err[~past] <= ((m - 1) * 2.0 ** -24 * mag)[~past]).all()
    return exp, stats


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("vt,dm,d,kind", [("f32", dm, d, "ints") for dm in ("L2", "Cosine")
                                          for d in (16, 40, 131, 128, 768)] +
                         [("i8", dm, d, "ints") for dm in ("L2", "Cosine") for d in (64, 100, 37)] +
                         [("f32", dm, d, "real") for dm in ("L2", "Cosine") for d in (40, 131)])
def test_kmeans_assign_every_dimension_form(vt, dm, d, kind, update):
    lay = layout(N, SIZES, NCENT)
    dist = None
    if kind == "real":
        od, cid, ncent = oracle_dist(dm, N, d), lay[4], lay[3]
        dist = lambda s, vid: np.array([od(vid, c) for c in cid[s, :ncent[s]]], dtype=np.float32)
    check(vt, dm, N, d, kind, lay, update, dist=dist)


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("vt,dm", TYPES)
def test_kmeans_assign_balance_term(vt, dm, update):
    """lambda 2 with small counts (every dist_k exact), lambda 0, and a lambda
    whose every penalty overflows: those members end at label 0 and MaxDist"""
    lay = layout(N, [150, 150, 150], [32, 32, 32], seed=4)
    pc = np.random.default_rng(8).integers(0, 6, (3, KMAX)).astype(np.int32)
    pc[2] = 1000
    lam = np.array([2.0, 0.0, 1e38], dtype=np.float32)
    exp, _ = check(vt, dm, N, DIM[vt], "ints", lay, update, pc, lam)
    plain, _ = ref_assign(matrix_dist(vt, dm, N, DIM[vt], "ints", lay[4], lay[3]),
                          vectors(vt, N, DIM[vt], "ints"), *lay[:4], update)
    seg = [slice(st, st + 150) for st in lay[1]]
    assert (exp[0][seg[0]] != plain[0][seg[0]]).any()
    np.testing.assert_array_equal(exp[0][seg[1]], plain[0][seg[1]])
    assert (exp[0][seg[2]] == 0).all() and (exp[1][seg[2]] == MAXDIST).all()


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("vt,dm", TYPES)
def test_kmeans_assign_ties(vt, dm, update):
    _, stats = check(vt, dm, N, DIM[vt], "ties", layout(N, [200, 397], [32, 64], seed=5), update)
    assert stats[2] > 0, stats


@pytest.mark.parametrize("update", [1, 0])
def test_kmeans_assign_large_segment(update):
    check("f32", "L2", BIG_N, 128, "ints", layout(BIG_N, [BIG_N - 3], [32], seed=6), update)


@pytest.mark.parametrize("update", [1, 0])
def test_kmeans_assign_items_of_several_tiles(update):
    """more than 2048 tiles in one call: an item holds two tiles, and ids occur
    many times"""
    members, starts, sizes, ncent, cid = layout(N, [500, 90], [4, 3], seed=7)
    members = np.tile(members, 56)
    lay = (members, np.array([0, 20003], np.int32), np.array([20000, 12990], np.int32), ncent, cid)
    check("f32", "L2", N, 40, "ints", lay, update)


def test_kmeans_assign_same_bytes_twice():
    lay = layout(N, SIZES, NCENT)
    x = vectors("f32", N, 131, "real")
    gpu = handle("f32", "L2", N, 131, "real")
    a = run(gpu, x, *lay, 1)
    b = run(gpu, x, *lay, 1)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("vt,dm,update", [("f32", "Cosine", 1), ("i8", "L2", 0)])
def test_kmeans_assign_device_form_and_kdt_handle(vt, dm, update):
    import torch
    d = DIM[vt]
    members, starts, sizes, ncent, cid = lay = layout(N, SIZES, NCENT)
    x = vectors(vt, N, d, "ints")
    want = run(handle(vt, dm, N, d, "ints", kdt=True), x, *lay, update)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    tx, tm, tc = dev(x), dev(members), dev(center_rows(x, cid, ncent))
    outs = [dev(np.full(a.shape, -7, dtype=a.dtype)) for a in want[:5]]
    sums = dev(np.full((len(sizes), KMAX, d), -7, dtype=np.float32)) if update else None
    torch.cuda.synchronize()
    kmeans_assign_device(tx.data_ptr(), 0 if vt == "f32" else 1, dm, N, d, tm.data_ptr(),
                         members.size, starts, sizes, ncent, tc.data_ptr(), KMAX, None, None,
                         update, *[t.data_ptr() for t in outs], sums.data_ptr() if update else None)
    for t, w in zip(outs + ([sums] if update else []), want):
        np.testing.assert_array_equal(t.cpu().numpy(), w)


def test_kmeans_assign_argument_errors():
    lib = load_library()
    members, starts, sizes, ncent, cid = layout(N, SIZES, NCENT)
    x = vectors("f32", N, 40, "ints")
    gpu = handle("f32", "L2", N, 40, "ints")
    cen = center_rows(x, cid, ncent)
    nseg = len(sizes)
    pc, lam = np.zeros((nseg, KMAX), np.int32), np.zeros(nseg, np.float32)
    outs = [np.full(members.size, -7, np.int32), np.full(members.size, -7, np.float32),
            np.full((nseg, KMAX), -7, np.int32), np.full((nseg, KMAX), -7, np.int32),
            np.full((nseg, KMAX), -7, np.float32), np.full((nseg, KMAX, 40), -7, np.float32)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def changed(a, i, val):
        b = a.copy()
        b[i] = val
        return b
    good = (gpu._h, p(members), members.size, p(starts), p(sizes), p(ncent), nseg, p(cen), KMAX,
            None, None, 1, *[p(a) for a in outs])
    assert lib.sptag_amd_kmeans_assign(*[None if i == 13 else a for i, a in enumerate(good)]) == 0
    for a in outs:
        a[...] = -7
    bad = [{i: None} for i in (0, 1, 3, 4, 5, 7, 12, 14, 15, 16, 17)]
    bad += [{6: 0}, {8: 0}, {8: 65}, {8: 32}, {11: 2}, {9: p(pc)}, {10: p(lam)},
            {5: p(changed(ncent, 2, 0))}, {3: p(changed(starts, 2, -1))},
            {4: p(changed(sizes, 2, -1))}, {4: p(changed(sizes, 8, 400))},
            {3: p(changed(starts, 4, 20))}, {1: p(changed(members, 5, -1))},
            {1: p(changed(members, 5, N))}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_kmeans_assign(*args) == -2, b          # SPTAG_AMD_ERR_PARAM
    assert all((a == -7).all() for a in outs)

    # the device form returns before it touches the device: any non-null
    # address stands for the buffers
    good = (0, p(x), 0, 0, N, 40) + good[1:]
    bad = [{i: None} for i in (1, 6, 8, 9, 10, 12, 17, 19, 20, 21, 22)]
    bad += [{11: 0}, {13: 0}, {13: 65}, {13: 32}, {16: 2}, {14: p(pc)}, {15: p(lam)},
            {10: p(changed(ncent, 2, 0))}, {9: p(changed(sizes, 8, 400))},
            {8: p(changed(starts, 4, 20))}, {2: 2}, {3: 2}, {4: 0}, {5: 0}, {5: 4097},
            {2: 1, 5: 261}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_kmeans_assign_device(*args) == -2, b
    assert all((a == -7).all() for a in outs)
