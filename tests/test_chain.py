"""The duplicate-chain walk on indexes that the reference's own builder made.

A set of identical vectors larger than the leaf size becomes one collapsed
tree node (negative childStart) with the copies as its children; the
representative's graph row carries -2 - treeNode in its last slot and no
graph row names a copy (BKTree.h:598-608, NeighborhoodGraph.h:395-400).
A copy reaches a result list only through the chain walk of the search loops
(BKTIndex.cpp:290-310 batched, :387-405 iterative). The fixtures
f32_l2_chain and i8_cos_chain (oracle/gen_golden.py, gen_chain_goldens) hold
three such nodes each, with chains of 68, 38 and 18 (17) copies.

One member of every set is an ordinary vector: k-means made it the centre of
the cluster that then held nothing but its copies, so it stays in the graph
and is found without the chain (`stray` below).

Queries 0..2 lie next to the three chained vectors (longest chain first),
queries 3..5 equal them, the other 26 are random. Everything is compared bit
for bit, ids and distances as uint32. The CPU tests show that the answers
depend on the chain; the oracle is held to the reference's recordings and
the GPU to both.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle.gen_golden import chain_layout
from oracle.pyoracle import OrcIndex
from parity_util import (assert_iter_calls_equal, brute_force_topk, golden_dtype,
                         orc_add, orc_graph, orc_iter_next, orc_iter_open,
                         orc_iter_run, read_graph, read_index_arrays, read_vectors)
from test_gpu_insert_batch import (_child_search, assert_bits_equal,
                                   orc_search_counted)

CHAIN = ["f32_l2_chain", "i8_cos_chain"]
NQ = 32
NADD = 16
ITER_GOLDENS = [(8, 5), (64, 3)]
# (k, MaxCheck) of the reference's recordings; 3 ends the walk inside a chain,
# 100 holds a whole chain of 68
RECORDED = [(10, 512), (10, 2048), (3, 512), (100, 512), (3, 2048), (100, 2048)]
# (k, MaxCheck) compared with the oracle alone
SMALL_MC = [(10, 8), (10, 64)]
_fx, _ref = {}, {}


def fx(name):
    """Golden, raw arrays, chains (longest first) and oracle of a fixture;
    read once, never modified."""
    if name not in _fx:
        g = load_golden(name)
        dtype = golden_dtype(g)
        arrs = read_index_arrays(g["index"], dtype)
        _fx[name] = {"g": g, "dtype": dtype, "arrs": arrs,
                     "dm": g["meta"]["distmethod"],
                     "chains": chain_layout(g["index"], dtype),
                     "oix": OrcIndex.load(g["index"]), "q": g["queries"]}
    return _fx[name]


def recorded(name, k, mc):
    """The reference searcher's (ids, dists) at (k, MaxCheck)."""
    f = f"results_mc{mc}.bin" if k == 10 else f"results_k{k}_mc{mc}.bin"
    raw = open(os.path.join(GOLDEN, name, f), "rb").read()
    nq, kk = np.frombuffer(raw[:8], dtype=np.int32)
    assert (nq, kk) == (NQ, k)
    rec = np.frombuffer(raw[8:], dtype=np.dtype([("vid", np.int32),
                                                 ("dist", np.float32)])).reshape(nq, k)
    return np.ascontiguousarray(rec["vid"]), np.ascontiguousarray(rec["dist"])


def recorded_iter(name, batch, ncalls):
    """An iterprobe file as the calls of parity_util: per call (vids [nq, b],
    dists [nq, b], counts [nq], relaxed [nq])."""
    raw = open(os.path.join(GOLDEN, name, f"iter_b{batch}_c{ncalls}.bin"), "rb").read()
    assert tuple(np.frombuffer(raw[:12], dtype=np.int32)) == (NQ, batch, ncalls)
    rec = np.frombuffer(raw[12:], dtype=np.int32).reshape(NQ, ncalls, 2 + 2 * batch)
    calls = []
    for c in range(ncalls):
        pairs = rec[:, c, 2:].reshape(NQ, batch, 2)
        calls.append((np.ascontiguousarray(pairs[:, :, 0]),
                      np.ascontiguousarray(pairs[:, :, 1]).view(np.float32),
                      rec[:, c, 0].copy(), rec[:, c, 1].copy()))
    return calls


def oracle_ref(name, k, mc, deleted=None, tag=None):
    """(ids, dists, checked [nq]) of the oracle, on the fixture as it is or
    under a delete mask; computed once."""
    key = (name, k, mc, tag)
    if key not in _ref:
        f = fx(name)
        oix = f["oix"] if deleted is None else OrcIndex.from_arrays(
            *f["arrs"], f["dm"], deleted=deleted)
        _ref[key] = orc_search_counted(oix, f["q"], k, mc)
    return _ref[key]


def assert_calls_bits_equal(got, want, tag):
    assert len(got) == len(want)
    for c, ((gv, gd, gc, gr), (wv, wd, wc, wr)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(gc, wc, err_msg=f"{tag} call {c} counts")
        np.testing.assert_array_equal(gr, wr, err_msg=f"{tag} call {c} relaxed")
        for i in range(len(wc)):
            assert_bits_equal(gv[i, :wc[i]], gd[i, :wc[i]], wv[i, :wc[i]],
                              wd[i, :wc[i]], f"{tag} call {c} query {i}")


# ---------------------------------------------------------------------------
# the committed fixtures are what the generator asserted
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CHAIN)
def test_fixture_holds_chains(name):
    f = fx(name)
    vec, _, tnodes, graph = f["arrs"]
    tnodes = tnodes.reshape(-1, 3)
    chains = f["chains"]             # chain_layout asserts while it reads
    assert vec.shape[0] >= 1000 and f["q"].shape[0] == NQ
    markers = np.where(graph[:, -1] < -1)[0]
    assert len(markers) >= 3 and sorted(c["rep"] for c in chains) == markers.tolist()
    counts = [len(c["copies"]) for c in chains]
    assert counts[0] > 64 and 11 <= counts[1] <= 64 and counts[2] > 3
    for c in chains:
        assert tnodes[c["node"], 1] < -1
        assert not np.isin(graph, c["copies"]).any()
        assert (vec[c["copies"]] == vec[c["rep"]]).all()
        # the walk reads the node after the last child; the tree's closing
        # node keeps that inside the array
        assert tnodes[c["node"], 2] < len(tnodes)
        # a stray keeps an incoming edge, a copy has none
        assert all((graph == s).any() for s in c["stray"])
    # query i and query 3 + i belong to chain i
    tv, td = f["oix"].truth(f["q"][:6], 1)
    for i in range(3):
        assert tv[i, 0] in chains[i]["group"] and tv[3 + i, 0] in chains[i]["group"]
    if name == "f32_l2_chain":
        np.testing.assert_array_equal(f["q"][3:6], vec[[c["rep"] for c in chains]])
        assert (td[3:6, 0] == 0).all() and (td[:3, 0] > 0).all()


# ---------------------------------------------------------------------------
# CPU: the answers depend on the chain, and the oracle equals the recordings
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CHAIN)
def test_oracle_answers_depend_on_the_chain(name):
    """Next to a chained vector the ten results are ten members of its set,
    at one distance. With the markers overwritten by -1 the same search
    finds the representative and no copy."""
    f = fx(name)
    vec, tstart, tnodes, graph = f["arrs"]
    ov, od, _ = oracle_ref(name, 10, 512)
    cut = graph.copy()
    cut[cut[:, -1] < -1, -1] = -1
    cv, _ = OrcIndex.from_arrays(vec, tstart, tnodes, cut, f["dm"]).search_batch(
        f["q"][:6], 10, 512)
    for i in range(6):
        c = f["chains"][i % 3]
        chain_ids = np.append(c["copies"], c["rep"])
        assert np.isin(ov[i], c["group"]).all(), f"query {i}: {ov[i]}"
        assert np.isin(ov[i], c["copies"]).sum() >= 8
        assert len(set(od[i].view(np.uint32).tolist())) == 1
        assert np.isin(cv[i], chain_ids).sum() == 1 and c["rep"] in cv[i]
        assert np.isin(cv[i], c["group"]).sum() == 1 + len(c["stray"])


@pytest.mark.parametrize("k,mc", RECORDED[2:])
@pytest.mark.parametrize("name", CHAIN)
def test_oracle_equals_recorded_search(name, k, mc):
    """k = 10 is test_oracle_bit_exact's; here 3 and 100."""
    f = fx(name)
    ov, od, _ = oracle_ref(name, k, mc)
    rv, rd = recorded(name, k, mc)
    assert_bits_equal(ov, od, rv, rd, f"{name} k={k}")
    for i in range(3):
        c = f["chains"][i]
        if k == 3:      # AddPoint rejects inside the chain
            assert np.isin(rv[i], c["group"]).all()
        else:           # the whole set is there: the walk ends at childEnd
            assert np.isin(c["group"], rv[i]).all()
            assert np.isin(c["group"], rv[3 + i]).all()


@pytest.mark.parametrize("batch,ncalls", ITER_GOLDENS)
@pytest.mark.parametrize("name", CHAIN)
def test_oracle_equals_recorded_iterator(name, batch, ncalls):
    f = fx(name)
    want = recorded_iter(name, batch, ncalls)
    got = orc_iter_run(f["oix"], f["q"], 8192, [batch] * ncalls)
    assert_calls_bits_equal(got, want, f"{name} b={batch}")
    # copies come out of the stream: the first Next of a near-chain query
    # returns nothing but members of the set
    for i in range(3):
        c = f["chains"][i]
        first = want[0][0][i, :want[0][2][i]]
        n = min(batch, len(c["group"]))
        assert np.isin(first[:n], c["group"]).all()
        assert np.isin(first[:n], c["copies"]).sum() == n - 1 - len(c["stray"])


def _postadd():
    """The oracle after the 16 recorded adds, with its answers; once."""
    if "add" not in _ref:
        f = fx("f32_l2_chain")
        add = read_vectors(os.path.join(GOLDEN, "f32_l2_chain", "add16_vectors.bin"),
                           np.float32)
        assert add.shape[0] == NADD
        oix = OrcIndex.load(f["g"]["index"])
        orc_add(oix, add)
        q = np.concatenate([f["q"], add])
        _ref["add"] = {"add": add, "oix": oix, "graph": orc_graph(oix), "q": q,
                       "search": {kmc: orc_search_counted(oix, q, *kmc)
                                  for kmc in [(10, 512), (100, 512), (10, 64)]},
                       "truth": oix.truth(q, 10),
                       "iter": orc_iter_run(oix, q[:8], 8192, [64, 8])}
    return _ref["add"]


def test_oracle_add_equals_recorded_graph():
    """AddIndex of 4 copies of chained vectors, 4 vectors within 1e-3 of a
    representative and 8 random ones: the refine search takes the NeverDup
    walk (the representative alone, then break) and InsertNeighbors spares a
    marker's slot."""
    f = fx("f32_l2_chain")
    r = _postadd()
    want = read_graph(os.path.join(GOLDEN, "f32_l2_chain", "postadd16_graph.bin"))
    before = f["arrs"][3]
    reps = [c["rep"] for c in f["chains"]]
    assert (want[reps] != before[reps]).any()
    np.testing.assert_array_equal(want[reps, -1], before[reps, -1])
    np.testing.assert_array_equal(r["graph"], want)


# ---------------------------------------------------------------------------
# deletes: cases and oracle answers
# ---------------------------------------------------------------------------

DELETES = ["rep", "half", "group"]


def delete_mask(name, case):
    """The mask of a case over all three sets: the representative alone (the
    walk skips it and goes on), every second copy, or the whole set."""
    f = fx(name)
    m = np.zeros(f["arrs"][0].shape[0], dtype=np.uint8)
    for c in f["chains"]:
        if case == "rep":
            m[c["rep"]] = 1
        elif case == "half":
            m[c["copies"][::2]] = 1
        else:
            m[c["group"]] = 1
    return m


def deleted_iter_ref(name, case):
    key = (name, case, "iter")
    if key not in _ref:
        f = fx(name)
        oix = OrcIndex.from_arrays(*f["arrs"], f["dm"], deleted=delete_mask(name, case))
        _ref[key] = orc_iter_run(oix, f["q"][:8], 8192, [64, 8, 8])
    return _ref[key]


@pytest.mark.parametrize("case", DELETES)
@pytest.mark.parametrize("name", CHAIN)
def test_oracle_deletes_reach_the_walk(name, case):
    f = fx(name)
    m = delete_mask(name, case)
    dead = np.where(m)[0]
    ov, od, _ = oracle_ref(name, 100, 512, m, case)
    stream = deleted_iter_ref(name, case)[0]
    assert not np.isin(ov, dead).any()
    for i in range(3):
        c = f["chains"][i]
        live = c["group"][m[c["group"]] == 0]
        got = ov[i][np.isin(ov[i], c["group"])]
        assert sorted(got.tolist()) == live.tolist(), f"{case} query {i}"
        if case != "group":     # copies behind a deleted entry still come out
            assert np.isin(got, c["copies"]).sum() >= len(c["copies"]) // 2
        first = stream[0][i, :stream[2][i]]
        assert not np.isin(first, dead).any()
        n = min(64, len(live))
        assert np.isin(first[:n], live).all(), f"{case} iterator query {i}"


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_gpu = {}


def gpu_ix(name):
    from sptag_amd import AnnIndex
    if name not in _gpu:
        _gpu[name] = AnnIndex.Load(fx(name)["g"]["index"])
    return _gpu[name]


def search_counted(ix, q, k, mc, ref, tag):
    v, d = ix.BatchSearch(q, k, mc)
    _, checked, popped = ix.LastStats()
    print(f"{tag}: checked {checked} (oracle {ref[2].sum()}) popped {popped}")
    assert_bits_equal(v, d, ref[0], ref[1], tag)
    assert checked == ref[2].sum(), tag
    return popped


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_search_equals_recordings_and_oracle(name):
    ix = gpu_ix(name)
    f = fx(name)
    for k, mc in RECORDED + SMALL_MC:
        ref = oracle_ref(name, k, mc)
        if (k, mc) in RECORDED:
            rv, rd = recorded(name, k, mc)
            assert_bits_equal(ref[0], ref[1], rv, rd, f"{name} oracle k={k} mc={mc}")
        search_counted(ix, f["q"], k, mc, ref, f"{name} k={k} mc={mc}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 10, 100])
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_search_global_heap_rerun(tmp_path, name, k, mc=2048):
    """A frontier held to 256 entries overflows, and the queries run again
    with both heaps in global memory at the reference's capacities; answers
    and counts must not notice. 256 is the smallest capacity the planner
    takes (plan.h), and on these indexes only MaxCheck 2048 outgrows it:
    counted on the oracle, the frontier of a query peaks at 240..304 entries
    there (17 of 32 queries of f32_l2_chain above 256, all 32 of
    i8_cos_chain), but at 118..154 at MaxCheck 512 with k = 3 or 10, at
    200..261 with k = 100, and below 113 at MaxCheck 8 and 64. So the rerun
    is compared at MaxCheck 2048, with the reference's recordings."""
    f = fx(name)
    ref = oracle_ref(name, k, mc)
    rv, rd = recorded(name, k, mc)
    assert_bits_equal(ref[0], ref[1], rv, rd, f"{name} oracle k={k} mc={mc}")
    v, d, stats, n_over, n_global = _child_search(
        tmp_path, name, NQ, k, mc, {"SPTAG_AMD_NG_CAP": "256"})
    print(f"{name} k={k} mc={mc} NG_CAP 256: {n_over}/{NQ} overflowed, {n_global} "
          f"rerun, checked {stats[0]} (oracle {ref[2].sum()}) popped {stats[1]}")
    assert n_global > 0, "no query reached the global-heap pass"
    assert_bits_equal(v, d, ref[0], ref[1], f"{name} k={k} mc={mc} rerun")
    assert stats[0] == ref[2].sum()
    # the traversal is the same wherever the frontier is stored
    ix = gpu_ix(name)
    ix.BatchSearch(f["q"], k, mc)
    assert ix.LastStats()[2] == stats[1]


def _exhaust(its, batch, limit=200):
    calls = []
    while not calls or (calls[-1][2] > 0).any():
        calls.append(orc_iter_next(its, batch))
        assert len(calls) < limit
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_iterator_equals_recordings_then_exhausts(name):
    f = fx(name)
    ix = gpu_ix(name)
    n = f["arrs"][0].shape[0]
    for batch, ncalls in ITER_GOLDENS:
        it = ix.Iterate(f["q"], max_check=8192)
        assert_iter_calls_equal(it, recorded_iter(name, batch, ncalls),
                                [batch] * ncalls, f"{name} b={batch}")
        it.Close()
    # to exhaustion against the oracle: every id once, the copies included
    q = f["q"][:4]
    calls = _exhaust(orc_iter_open(f["oix"], q, 8192), 256)
    it = ix.Iterate(q, max_check=8192)
    got = [[] for _ in q]
    for c, (rv, rd, rcnt, rrel) in enumerate(calls):
        gv, gd, gcnt, grel = it.Next(256)
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=f"call {c} counts")
        np.testing.assert_array_equal(grel, rrel, err_msg=f"call {c} relaxed")
        for i in range(len(q)):
            assert_bits_equal(gv[i, :rcnt[i]], gd[i, :rcnt[i]], rv[i, :rcnt[i]],
                              rd[i, :rcnt[i]], f"{name} call {c} query {i}")
            got[i].extend(gv[i, :gcnt[i]].tolist())
    it.Close()
    for ids in got:
        assert sorted(ids) == list(range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("case", DELETES)
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_deletes(name, case):
    from sptag_amd import AnnIndex
    f = fx(name)
    m = delete_mask(name, case)
    ix = AnnIndex.FromArrays(*f["arrs"], f["dm"], deleted=m)
    assert ix.deleted_count == int(m.sum())
    for k, mc in [(100, 512), (10, 512), (3, 64)]:
        search_counted(ix, f["q"], k, mc, oracle_ref(name, k, mc, m, case),
                       f"{name} {case} k={k} mc={mc}")
    batches = [64, 8, 8]
    it = ix.Iterate(f["q"][:8], max_check=8192)
    assert_iter_calls_equal(it, deleted_iter_ref(name, case), batches,
                            f"{name} {case}")
    it.Close()
    # the same mask set by Delete on a loaded index
    ix2 = AnnIndex.Load(f["g"]["index"])
    ix2.Delete(np.where(m)[0])
    search_counted(ix2, f["q"], 100, 512, oracle_ref(name, 100, 512, m, case),
                   f"{name} {case} Delete()")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_delete_by_vector_flags_every_copy(name):
    """DeleteIndex(vector): a search of 1000 results, every id nearer than
    1e-6 is flagged. The count is numpy's, in float64 on the stored vectors
    (for int8 cosine a vector's distance to itself is 16129 - |v|^2, which
    is above 1e-6 unless the truncated norm is exactly 127)."""
    from sptag_amd import AnnIndex
    f = fx(name)
    vec = f["arrs"][0]
    x = vec.astype(np.float64)
    ix = AnnIndex.Load(f["g"]["index"])
    total = 0
    for c in f["chains"]:
        v = x[c["rep"]]
        if f["dm"] == "L2":
            dist = ((x - v) ** 2).sum(1)
        else:
            dist = (16129.0 if vec.dtype == np.int8 else 1.0) - x @ v
        want = int((dist < 1e-6).sum())
        if name == "f32_l2_chain":
            assert want == len(c["group"])
        ix.DeleteByVector(vec[c["rep"]][None, :])
        total += want
        assert ix.deleted_count == total, f"{name} rep {c['rep']}"
    if name == "f32_l2_chain":
        m = np.zeros(len(vec), dtype=np.uint8)
        for c in f["chains"]:
            m[c["group"]] = 1
        search_counted(ix, f["q"], 10, 512, oracle_ref(name, 10, 512, m, "group"),
                       f"{name} after DeleteByVector")


@pytest.mark.gpu
def test_gpu_add_equals_recorded_graph(tmp_path):
    from sptag_amd import AnnIndex
    name = "f32_l2_chain"
    f = fx(name)
    r = _postadd()
    ix = AnnIndex.Load(f["g"]["index"])
    ix.Add(r["add"])
    assert ix.n == f["arrs"][0].shape[0] + NADD
    for (k, mc), ref in r["search"].items():
        search_counted(ix, r["q"], k, mc, ref, f"post-add k={k} mc={mc}")
    gv, gd = ix.Truth(r["q"], 10)
    assert_bits_equal(gv, gd, r["truth"][0], r["truth"][1], "post-add truth")
    it = ix.Iterate(r["q"][:8], max_check=8192)
    assert_iter_calls_equal(it, r["iter"], [64, 8], "post-add")
    it.Close()
    out = str(tmp_path / "postadd")
    ix.Save(out)
    saved = read_graph(os.path.join(out, "graph.bin"))
    np.testing.assert_array_equal(
        saved, read_graph(os.path.join(GOLDEN, name, "postadd16_graph.bin")))
    np.testing.assert_array_equal(saved, r["graph"])


def assert_truth_is_brute_force(f, k, v, d, tag):
    """Exact top-k by (distance, id) in float64. int8 distances are exact
    integers, so ids and distances are equal. float32 rounding may swap two
    distances that differ in the last bit, so there the order must hold by
    (own distance, id), which decides every tie inside a set of equal
    vectors by id alone, and the sets must agree."""
    bv, bd = brute_force_topk(f["arrs"][0], f["q"], k, f["dm"])
    if f["dtype"] == np.int8:
        np.testing.assert_array_equal(v, bv, err_msg=tag)
        np.testing.assert_array_equal(d, bd.astype(np.float32), err_msg=tag)
        return
    dd = d.astype(np.float64)
    step_d, step_id = np.diff(dd, axis=1), np.diff(v, axis=1)
    assert ((step_d > 0) | ((step_d == 0) & (step_id > 0))).all(), tag
    for a, b in zip(v, bv):
        assert set(a.tolist()) == set(b.tolist()), tag
    np.testing.assert_allclose(dd, bd, rtol=1e-5, atol=1e-5, err_msg=tag)


@pytest.mark.parametrize("name", CHAIN)
def test_oracle_truth_is_brute_force(name):
    f = fx(name)
    for k in (10, 100):
        tv, td = f["oix"].truth(f["q"], k)
        assert_truth_is_brute_force(f, k, tv, td, f"{name} k={k}")
        # whole sets of equal vectors, in id order
        for i in range(3):
            grp = f["chains"][i]["group"][:k]
            np.testing.assert_array_equal(tv[3 + i, :len(grp)], grp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAIN)
def test_gpu_truth_equals_brute_force(name):
    f = fx(name)
    for k in (10, 100):
        gv, gd = gpu_ix(name).Truth(f["q"], k)
        ov, od = f["oix"].truth(f["q"], k)
        assert_bits_equal(gv, gd, ov, od, f"{name} truth k={k}")
        assert_truth_is_brute_force(f, k, gv, gd, f"{name} gpu k={k}")
