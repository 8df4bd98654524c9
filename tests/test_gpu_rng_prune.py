"""AnnIndex.RngPrune / rng_prune_device against a plain restatement of
RebuildNeighbors. On small exact integers every pair distance is exact in f32
and float64 alike, so the expected ids are unambiguous; for generic f32 the
pair distances are the oracle's (the reference-order contract). Every
data-driven case checks on the EXPECTED output that it holds a row stopped by
the degree cap with valid candidates left, a row that ends short, and a
rejection."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd import AnnIndex, load_library, rng_prune_device
from test_gpu_exact_search import data, flat_args, TYPES, DIM

pytestmark = pytest.mark.gpu

N, ROWS = 600, 300
BIG_N, BIG_ROWS = 1500, 70      # pools of up to 1024 candidates
F32, F64 = 1.5, 2.0             # factors at which these pools fill degree 32 and 64


@functools.lru_cache(maxsize=None)
def vectors(vt, n, d, kind):
    """ints: small exact integers; ties: 50 distinct ones repeated; real
    (f32): a 6-d manifold in d dims plus noise, so that the rule rejects."""
    if kind == "ties":
        return data(vt, n, d, 1, ties=True)[0]
    rng = np.random.default_rng(77 + n + d)
    if kind == "real":
        x = rng.standard_normal((n, 6)) @ rng.standard_normal((6, d))
        x = (x + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    else:
        lat = rng.integers(-2, 3, (n, 6)) @ rng.integers(-1, 2, (6, d))
        x = np.clip(lat + rng.integers(-1, 2, (n, d)), -4, 4)
        x = x.astype(np.float32 if vt == "f32" else np.int8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pair_matrix(vt, dm, n, d, kind):
    """float64 [n, n] distances of the metric: exact for the integer kinds"""
    x = vectors(vt, n, d, kind).astype(np.float64)
    dot = x @ x.T
    if dm == "L2":
        sq = np.diag(dot)
        return sq[:, None] + sq[None, :] - 2.0 * dot
    return (1.0 if vt == "f32" else 16129.0) - dot


def pools(vt, dm, n, d, kind, rows, C):
    """nodes 0..rows-1 and their C nearest others, ascending (dist, id)"""
    P = pair_matrix(vt, dm, n, d, kind)[:rows].copy()
    P[np.arange(rows), np.arange(rows)] = np.inf
    ids = np.argsort(P, axis=1, kind="stable")[:, :C].astype(np.int32)
    return (np.arange(rows, dtype=np.int32), ids,
            np.take_along_axis(P, ids, 1).astype(np.float32))


def ref_prune(pair, nodes, ids, cd, degree, factor, fill):
    """The rule, one candidate at a time. pair(acc, c): f32 distances of the
    accepted ids to c. Returns the graph and (capped rows with valid
    candidates left, short rows, rejections)."""
    out = np.full((len(nodes), degree), -1, dtype=np.int32)
    capped = short = nrej = 0
    for r, node in enumerate(nodes):
        acc, rej, left = [], [], False
        for j, (c, dc) in enumerate(zip(ids[r], cd[r])):
            if c < 0 or c == node or not np.isfinite(dc):
                continue
            if len(acc) == degree:
                left = True
                break
            if acc and (np.float32(factor) * pair(ids[r][acc], c) < dc).any():
                rej.append(j)
            else:
                acc.append(j)
        keep = sorted(acc + (rej[:degree - len(acc)] if fill else []))
        out[r, :len(keep)] = ids[r][keep]
        capped += left
        short += len(acc) < degree
        nrej += len(rej)
    return out, (capped, short, nrej)


def matrix_pair(vt, dm, n, d, kind):
    P = pair_matrix(vt, dm, n, d, kind)
    return lambda acc, c: P[acc, c].astype(np.float32)


def handle(vt, dm, n, d, kind, kdt=False):
    x = vectors(vt, n, d, kind)
    if kdt:
        return AnnIndex.FromArraysKDT(x, np.zeros(1, dtype=np.int32),
                                      np.zeros((2, 4), dtype=np.int32),
                                      np.full((n, 2), -1, dtype=np.int32), dm)
    return AnnIndex.FromArrays(*flat_args(x, dm))


def check(vt, dm, n, d, kind, nodes, ids, cd, degree, factor=1.0, fill=False, pair=None,
          nonvacuous=True):
    exp, (capped, short, nrej) = ref_prune(pair or matrix_pair(vt, dm, n, d, kind), nodes, ids,
                                           cd, degree, factor, fill)
    print(f"capped {capped} short {short} rejections {nrej}")
    if nonvacuous:
        assert capped > 0 and short > 0 and nrej > 0, (capped, short, nrej)
    got = handle(vt, dm, n, d, kind).RngPrune(nodes, ids, cd, degree, factor, fill)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, exp)
    return exp


@pytest.mark.parametrize("vt,dm,d", [("f32", dm, d) for dm in ("L2", "Cosine")
                                     for d in (16, 40, 131, 128, 768)] +
                         [("i8", dm, d) for dm in ("L2", "Cosine") for d in (64, 100, 37)])
def test_rng_prune_every_dimension_form(vt, dm, d):
    if vt == "i8":
        check(vt, dm, N, d, "ints", *pools(vt, dm, N, d, "ints", ROWS, 40), 8)
        return
    x = vectors(vt, N, d, "real")
    orc = OrcIndex.from_arrays(*flat_args(x, dm))
    pair = lambda acc, c: np.array([orc.distance(x[a], x[c]) for a in acc], dtype=np.float32)
    check(vt, dm, N, d, "real", *pools(vt, dm, N, d, "real", ROWS, 40), 8, pair=pair)


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("C,degree,factor", [
    (1, 1, 1.0), (15, 4, 1.0), (16, 16, 1.0), (17, 17, F32), (33, 32, F32), (264, 32, F32),
    (384, 33, F32), (1024, 64, F64)])
@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "L2")])
def test_rng_prune_tile_and_cap_boundaries(vt, dm, C, degree, factor, fill):
    check(vt, dm, BIG_N, DIM[vt], "ints", *pools(vt, dm, BIG_N, DIM[vt], "ints", BIG_ROWS, C),
          degree, factor, fill, nonvacuous=C - degree > 1)


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("vt,dm", TYPES)
def test_rng_prune_junk_and_ties(vt, dm, fill):
    d = DIM[vt]
    nodes, ids, cd = pools(vt, dm, N, d, "ties", ROWS, 200)
    check(vt, dm, N, d, "ties", nodes, ids, cd, 20, fill=fill)
    ids, cd = ids.copy(), cd.copy()
    ids[::3, 5], cd[::3, 5] = -1, np.inf            # holes in the middle
    ids[::4, 30:], cd[::4, 30:] = -1, np.inf        # and in the tail
    ids[1::5, 2] = nodes[1::5]                      # the node itself
    ids[2::5, 7] = ids[2::5, 1]                     # a repeated id (at a larger distance)
    cd[3::7, 4] = np.nan
    ids[9], cd[9] = -1, np.inf                      # nothing valid
    cd[10] = np.inf                                 # nor here, with ids
    exp = check(vt, dm, N, d, "ties", nodes, ids, cd, 20, fill=fill)
    assert (exp[9] == -1).all() and (exp[10] == -1).all()


@pytest.mark.parametrize("vt,dm", [("f32", "Cosine"), ("i8", "L2")])
def test_rng_prune_device_form_and_kdt_handle(vt, dm):
    import torch
    d = DIM[vt]
    nodes, ids, cd = pools(vt, dm, N, d, "ints", ROWS, 40)
    exp = check(vt, dm, N, d, "ints", nodes, ids, cd, 8, fill=True)
    np.testing.assert_array_equal(
        handle(vt, dm, N, d, "ints", kdt=True).RngPrune(nodes, ids, cd, 8, fill_pruned=True), exp)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    tx, tn, ti, tc = dev(vectors(vt, N, d, "ints")), dev(nodes), dev(ids), dev(cd)
    out = torch.full((ROWS, 8), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rng_prune_device(tx.data_ptr(), 0 if vt == "f32" else 1, dm, N, d, tn.data_ptr(), ROWS,
                     ti.data_ptr(), tc.data_ptr(), 40, 8, 1.0, True, out.data_ptr())
    np.testing.assert_array_equal(out.cpu().numpy(), exp)


def test_rng_prune_argument_errors():
    lib = load_library()
    nodes, ids, cd = pools("f32", "L2", N, 40, "ints", ROWS, 40)
    gpu = handle("f32", "L2", N, 40, "ints")
    out = np.full((ROWS, 8), -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    F = ctypes.c_float

    def changed(a, i, val):
        b = a.copy()
        b[i] = val
        return b
    good = (gpu._h, p(nodes), ROWS, p(ids), p(cd), 40, 8, F(1.0), 0, p(out))
    bad = [{i: None} for i in (0, 1, 3, 4, 9)]
    bad += [{2: 0}, {5: 0}, {5: 1025}, {6: 0}, {6: 65}, {7: F(0.0)}, {7: F(-1.0)},
            {7: F(np.inf)}, {7: F(np.nan)}, {1: p(changed(nodes, 3, -1))},
            {1: p(changed(nodes, 3, N))}, {3: p(changed(ids, (5, 5), N))}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_rng_prune(*args) == -2, b         # SPTAG_AMD_ERR_PARAM
    assert (out == -7).all()

    # the device form returns before it touches the device: any non-null
    # address stands for the buffers
    x = vectors("f32", N, 40, "ints")
    good = (0, p(x), 0, 0, N, 40, p(nodes), ROWS, p(ids), p(cd), 40, 8, F(1.0), 0, p(out))
    bad = [{i: None} for i in (1, 6, 8, 9, 14)]
    bad += [{7: 0}, {10: 0}, {10: 1025}, {11: 0}, {11: 65}, {12: F(0.0)}, {12: F(np.nan)},
            {2: 2}, {3: 2}, {4: 0}, {5: 0}, {5: 4097}, {2: 1, 5: 261}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_rng_prune_device(*args) == -2, b
    assert (out == -7).all()


def test_rng_prune_builder_plumbing():
    import torch
    from sptag_amd import build
    x = np.array(vectors("f32", N, 40, "ints"))     # writable, for torch
    xf = torch.from_numpy(x).to("cuda:0")
    nodes, ids, cd = pools("f32", "L2", N, 40, "ints", ROWS, 40)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    for fill in (False, True):
        got = build._rng_prune_hip(xf, dev(ids), dev(cd), 8, 1.0, fill, nodes=dev(nodes))
        np.testing.assert_array_equal(
            got.cpu().numpy(), handle("f32", "L2", N, 40, "ints").RngPrune(nodes, ids, cd, 8, 1.0, fill))
    with pytest.raises(RuntimeError, match="GPU"):
        build._rng_prune_hip(xf.cpu(), torch.from_numpy(ids), torch.from_numpy(cd), 8, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        build.build_rng_graph(x, device="cpu", prune="hip")
    with pytest.raises(ValueError, match="prune"):
        build.build_index_arrays(x, "L2", prune="cuda")

    kw = dict(tpt_leaf=100, ntrees=2, device="cuda:0", refine_rounds=1)
    graph = build.build_index_arrays(x, "L2", prune="hip", **kw)["graph"]
    assert graph.shape == (N, 32) and graph.dtype == np.int32
    assert graph.min() >= -1 and graph.max() < N
    assert not (graph == np.arange(N)[:, None]).any()
    np.testing.assert_array_equal(
        build.build_index_arrays(x, "L2", prune="torch", **kw)["graph"],
        build.build_index_arrays(x, "L2", **kw)["graph"])
