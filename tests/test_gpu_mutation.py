"""Search, truth and iteration on an index that the library has changed
after creation. test_add.py compares only the saved graph, which Save writes
from the host arrays; here the device state after Add / Delete (re-uploaded
vectors, graph rows patched one add at a time, re-uploaded delete mask,
larger n) is what answers the queries.

The same steps are applied to an OrcIndex (orc_add with AddCEF 500). L2
fixtures add the first 16 rows of their add_vectors.bin; cosine fixtures add
the 16 seeded un-normalised vectors of their add16_vectors.bin with
normalized=False, so the host normalisation is checked through the saved
vectors. For the cosine fixtures the reference's own AddIndex recorded what
it stored for those 16 vectors and every graph row it changed
(oracle/gen_golden.py, gen_cosine_add_goldens); the oracle and the GPU are
both held to that record."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle.pyoracle import OrcIndex
from parity_util import (golden_dtype, orc_add, orc_graph, orc_iter_run,
                         orc_vectors, read_graph, read_index_arrays,
                         read_vectors, assert_iter_calls_equal)

FIXTURES = ["f32_l2_n10k_d32", "i8_l2_n10k_d100", "f32_cos_n10k_d48",
            "i8_cos_deg48"]
COSINE = ["f32_cos_n10k_d48", "i8_cos_deg48"]
NADD = 16
_ref = {}


def add_vectors(name):
    """The 16 vectors a fixture adds, as given to Add (not normalised)."""
    g = load_golden(name)
    dtype = golden_dtype(g)
    if g["meta"]["distmethod"] == "L2":
        return read_vectors(os.path.join(GOLDEN, name, "add_vectors.bin"),
                            dtype)[:NADD]
    return read_vectors(os.path.join(GOLDEN, name, "add16_vectors.bin"), dtype)


def reference_postadd(name):
    """What the reference's AddIndex left behind for a cosine fixture: the
    whole post-add graph (index/graph.bin with the recorded rows replaced
    and the 16 new rows appended) and the 16 vectors as it stored them."""
    g = load_golden(name)
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "postadd16_rows.bin"), "rb") as f:
        n_after, deg, nrows = np.frombuffer(f.read(12), dtype=np.int32)
        rec = np.frombuffer(f.read(), dtype=np.int32).reshape(nrows, 1 + deg)
    base = read_graph(os.path.join(g["index"], "graph.bin"))
    assert base.shape == (n_after - NADD, deg)
    graph = np.concatenate([base, np.full((NADD, deg), -1, dtype=np.int32)])
    ids = rec[:, 0]
    assert (np.diff(ids) > 0).all() and ids[-NADD] == n_after - NADD
    graph[ids] = rec[:, 1:]
    tail = read_vectors(os.path.join(d, "postadd16_vectors.bin"),
                        golden_dtype(g))
    assert tail.shape[0] == NADD
    return graph, tail


def _postadd(name):
    """Oracle after the add and its answers; computed once, never modified."""
    if name not in _ref:
        g = load_golden(name)
        oix = OrcIndex.load(g["index"])
        n0 = oix.n
        orc_add(oix, add_vectors(name))
        vec = orc_vectors(oix)
        q = np.concatenate([g["queries"][:32], vec[n0:]])
        _ref[name] = {
            "g": g, "oix": oix, "n0": n0, "q": q, "vec": vec,
            "graph": orc_graph(oix),
            "search": {mc: oix.search_batch(q, 10, mc, nthreads=4)
                       for mc in (512, 2048)},
            "truth": oix.truth(q, 10, nthreads=4),
            "iter": orc_iter_run(oix, q[28:36], 8192, [8, 8])}
    return _ref[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_postadd_state(name):
    """The oracle after the add: added vectors are normalised to the stored
    norm (1 for float, at most 127 with C-cast truncation for int8), each is
    its own nearest neighbour in the exact top-k, and the searches reach
    added ids, so a GPU that missed the new rows could not match."""
    r = _postadd(name)
    g, n0, vec = r["g"], r["n0"], r["vec"]
    assert vec.shape[0] == n0 + NADD and r["graph"].shape[0] == n0 + NADD
    raw = add_vectors(name)
    tail = vec[n0:]
    if g["meta"]["distmethod"] == "L2":
        np.testing.assert_array_equal(tail, raw)
    elif tail.dtype == np.float32:
        x = raw.astype(np.float64)
        want = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)
        np.testing.assert_array_equal(tail, want)
    else:
        x = raw.astype(np.float64)
        want = np.trunc(x * 127.0 / np.sqrt((x * x).sum(1, keepdims=True)))
        np.testing.assert_array_equal(tail, want.astype(np.int8))
        assert (tail != raw).any()
    tv, td = r["truth"]
    new_ids = np.arange(n0, n0 + NADD)
    if tail.dtype == np.int8 and g["meta"]["distmethod"] == "Cosine":
        # truncated norms differ, so a longer base vector may beat the
        # query itself on 16129 - dot; it is still in the exact top 10
        assert all(new_ids[i] in tv[32 + i] for i in range(NADD))
    else:
        np.testing.assert_array_equal(tv[32:, 0], new_ids)
    assert (r["graph"][n0:, 0] >= 0).all()
    for mc, (sv, _) in r["search"].items():
        assert (sv >= n0).any(), f"mc={mc}: no added id in any result row"


@pytest.mark.parametrize("name", COSINE)
def test_oracle_cosine_add_matches_reference(name):
    """orc_add against the reference's own AddIndex on un-normalised cosine
    input: every graph row and the stored form of the 16 vectors."""
    r = _postadd(name)
    graph, tail = reference_postadd(name)
    assert (graph[:r["n0"]] != read_graph(
        os.path.join(r["g"]["index"], "graph.bin"))).any(), "no back-link recorded"
    np.testing.assert_array_equal(r["vec"][r["n0"]:], tail)
    np.testing.assert_array_equal(r["graph"], graph)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_search_after_add(name, tmp_path):
    from sptag_amd import AnnIndex
    r = _postadd(name)
    g, n0 = r["g"], r["n0"]
    dtype = golden_dtype(g)
    ix = AnnIndex.Load(g["index"])
    ix.Add(add_vectors(name), normalized=False)
    assert ix.n == n0 + NADD
    for mc, (ov, od) in r["search"].items():
        gv, gd = ix.BatchSearch(r["q"], 10, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"{name} mc={mc}")
        np.testing.assert_array_equal(gd, od, err_msg=f"{name} mc={mc}")
    gv, gd = ix.Truth(r["q"], 10)
    np.testing.assert_array_equal(gv, r["truth"][0])
    np.testing.assert_array_equal(gd, r["truth"][1])
    it = ix.Iterate(r["q"][28:36], max_check=8192)
    assert_iter_calls_equal(it, r["iter"], [8, 8], name)
    it.Close()

    # Save -> the host arrays; Load -> a fresh upload of the same state
    out = str(tmp_path / "postadd")
    ix.Save(out)
    np.testing.assert_array_equal(read_graph(os.path.join(out, "graph.bin")),
                                  r["graph"])
    saved = read_vectors(os.path.join(out, "vectors.bin"), dtype)
    np.testing.assert_array_equal(saved[n0:], r["vec"][n0:])
    if name in COSINE:
        ref_graph, ref_tail = reference_postadd(name)
        np.testing.assert_array_equal(
            read_graph(os.path.join(out, "graph.bin")), ref_graph)
        np.testing.assert_array_equal(saved[n0:], ref_tail)
    np.testing.assert_array_equal(saved[:n0], r["vec"][:n0])
    before = ix.BatchSearch(r["q"], 10, 2048)
    ix2 = AnnIndex.Load(out)
    after = ix2.BatchSearch(r["q"], 10, 2048)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    lv, ld = OrcIndex.load(out).search_batch(r["q"], 10, 2048, nthreads=4)
    np.testing.assert_array_equal(after[0], lv)
    np.testing.assert_array_equal(after[1], ld)


# ---- Delete -> Add -> Delete --------------------------------------------

DAD = "f32_l2_n10k_d32"


def _dad():
    """Oracle construction: the oracle has no delete call. A first oracle is
    built from_arrays with the first mask and takes orc_add (its refine
    searches run with searchDeleted on, as the GPU's do, and its mask grows
    by 16 zeros). A second oracle is then built from_arrays from the first
    one's vectors and graph, the unchanged tree, and the final mask (first
    mask + 16 zeros, then the 8 later deletes set). That second oracle holds
    exactly the GPU's final state: same vectors, graph, tree and mask."""
    if "dad" not in _ref:
        g = load_golden(DAD)
        vec, tstart, tnodes, graph = read_index_arrays(g["index"], np.float32)
        n0 = vec.shape[0]
        rng = np.random.default_rng(23)
        mask0 = (rng.random(n0) < 0.05).astype(np.uint8)
        first = OrcIndex.from_arrays(vec, tstart, tnodes, graph, "L2",
                                     deleted=mask0)
        add = add_vectors(DAD)
        orc_add(first, add)
        new_del = np.array([n0 + 1, n0 + 5, n0 + 6, n0 + 15], dtype=np.int32)
        old_live = np.where(mask0 == 0)[0]
        old_del = rng.choice(old_live, 4, replace=False).astype(np.int32)
        final = np.concatenate([mask0, np.zeros(NADD, dtype=np.uint8)])
        final[new_del] = 1
        final[old_del] = 1
        second = OrcIndex.from_arrays(orc_vectors(first), tstart, tnodes,
                                      orc_graph(first), "L2", deleted=final)
        q = np.concatenate([g["queries"][:32], add])
        _ref["dad"] = {
            "arrs": (vec, tstart, tnodes, graph), "mask0": mask0, "add": add,
            "dels": np.concatenate([new_del, old_del]), "final": final, "q": q,
            "n0": n0, "graph": orc_graph(first),
            "search": {mc: second.search_batch(q, 10, mc, nthreads=4)
                       for mc in (512, 2048)},
            "truth": second.truth(q, 10, nthreads=4)}
    return _ref["dad"]


def test_oracle_delete_add_delete_state():
    r = _dad()
    dead = np.where(r["final"])[0]
    assert r["final"].sum() == r["mask0"].sum() + 8
    tv, _ = r["truth"]
    assert not np.isin(tv, dead).any()
    # a live added vector finds itself, a deleted one does not
    for i in range(NADD):
        vid = r["n0"] + i
        assert (tv[32 + i, 0] == vid) == (r["final"][vid] == 0)
    for sv, _ in r["search"].values():
        assert not np.isin(sv, dead).any()
        assert (sv >= r["n0"]).any()


@pytest.mark.gpu
def test_gpu_delete_add_delete(tmp_path):
    from sptag_amd import AnnIndex
    r = _dad()
    ix = AnnIndex.FromArrays(*r["arrs"], "L2", deleted=r["mask0"])
    assert ix.deleted_count == int(r["mask0"].sum())
    ix.Add(r["add"])
    assert ix.n == r["n0"] + NADD
    assert ix.deleted_count == int(r["mask0"].sum())
    ix.Delete(r["dels"])
    assert ix.deleted_count == int(r["final"].sum())
    for mc, (ov, od) in r["search"].items():
        gv, gd = ix.BatchSearch(r["q"], 10, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"mc={mc}")
        np.testing.assert_array_equal(gd, od, err_msg=f"mc={mc}")
    gv, gd = ix.Truth(r["q"], 10)
    np.testing.assert_array_equal(gv, r["truth"][0])
    np.testing.assert_array_equal(gd, r["truth"][1])
    out = str(tmp_path / "dad")
    ix.Save(out)
    np.testing.assert_array_equal(read_graph(os.path.join(out, "graph.bin")),
                                  r["graph"])
    with open(os.path.join(out, "deletes.bin"), "rb") as f:
        cnt, rows, _ = np.frombuffer(f.read(12), dtype=np.int32)
        saved = np.frombuffer(f.read(), dtype=np.uint8)
    assert cnt == int(r["final"].sum()) and rows == len(r["final"])
    np.testing.assert_array_equal(saved, r["final"])
