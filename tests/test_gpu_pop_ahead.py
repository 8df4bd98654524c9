"""The batched and iterative BKT kernels read the top of a heap before they
pop it and issue the loads that follow from that node alone ahead of the pop
(kernels.hip, peek_frontier / SPTAG_POP_AHEAD): the adjacency row in the graph
loop and the tree node's triple in the tree descent. The traversal must not
change, so every case compares ids and float bits with the oracle:

- 5 and 65 vectors: the top is also the last entry at many pops, and at n = 5
  the row is mostly -1;
- 300 vectors under a hand-made tree whose two inner nodes have 150 children
  each (the builder never gives a node more than 32), so one early triple
  is followed by three chunks of children;
- deleted vectors, and the f32_l2_dups fixture (every vector four times;
  built_case draws its own data, so the committed fixture, 8000 vectors of
  16 dims, stands in). Neither that fixture nor this project's builder
  writes a chain marker into a row's last slot, so the chain walk itself is
  reached by no test, here as before; the row's last slot is read as it was;
- a frontier capacity that sends queries through the LDS pass and then the
  global-heap pass, where the peek is a global read;
- one Next sequence of the iterator, whose tree heap is all in global memory.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle.pyoracle import OrcIndex
from parity_util import (assert_iter_calls_equal, built_case, gpu_from_case,
                         orc_from_case, orc_iter_run)

pytestmark = pytest.mark.gpu

TYPES = [("f32", "L2"), ("i8", "Cosine")]
MAXCHECKS = [1, 64, 8192]
_ref = {}


def _wide_case(vt, dm):
    """built_case(300) under a tree of our own: root -> two inner nodes of
    150 leaves each (three chunks of 64, 64 and 22 children)."""
    key = ("wide", vt, dm)
    if key not in _ref:
        c = built_case(300, 16, vt, dm, "BKT")
        vec, _, _, graph, _ = c["args"]
        n = 300
        nodes = np.empty((3 + n, 3), dtype=np.int32)
        nodes[0] = (n, 1, 3)               # root: center id n, unused
        nodes[1] = (0, 3, 3 + 150)
        nodes[2] = (150, 3 + 150, 3 + n)
        nodes[3:, 0] = np.arange(n)
        nodes[3:, 1:] = -1
        nodes.setflags(write=False)
        tstart = np.zeros(1, dtype=np.int32)
        tstart.setflags(write=False)
        _ref[key] = dict(c, args=(vec, tstart, nodes, graph, dm))
    return _ref[key]


def _case(kind, n, vt, dm):
    return _wide_case(vt, dm) if kind == "wide" else built_case(n, 16, vt, dm, "BKT")


def _search_ref(kind, n, vt, dm, deleted=None):
    """Oracle answers over the k x MaxCheck grid of one index; computed once."""
    key = ("search", kind, n, vt, dm, None if deleted is None else deleted.tobytes())
    if key not in _ref:
        c = _case(kind, n, vt, dm)
        oix = orc_from_case(c, deleted)
        _ref[key] = {(k, mc): oix.search_batch(c["q"], k, mc)
                     for k in (1, n + 3) for mc in MAXCHECKS}
    return _ref[key]


def _compare_grid(ix, c, ref, tag):
    for (k, mc), (ov, od) in ref.items():
        gv, gd = ix.BatchSearch(c["q"], k, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"{tag} k={k} mc={mc} ids")
        np.testing.assert_array_equal(gd, od, err_msg=f"{tag} k={k} mc={mc} dists")


@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("kind,n", [("built", 5), ("built", 65), ("wide", 300)])
def test_search_grid(kind, n, vt, dm):
    c = _case(kind, n, vt, dm)
    if kind == "wide":
        nodes = c["args"][2]
        assert (nodes[:, 2] - nodes[:, 1]).max() > 128
    _compare_grid(gpu_from_case(c), c, _search_ref(kind, n, vt, dm),
                  f"{kind} n={n} {vt} {dm}")


def _mask(n):
    """every third vector deleted, the first and the last among them"""
    m = np.zeros(n, dtype=np.uint8)
    m[::3] = 1
    m[n - 1] = 1
    return m


@pytest.mark.parametrize("kind,n", [("built", 65), ("wide", 300)])
def test_deleted(kind, n):
    c = _case(kind, n, "f32", "L2")
    ix = gpu_from_case(c, _mask(n))
    assert ix.deleted_count == int(_mask(n).sum())
    _compare_grid(ix, c, _search_ref(kind, n, "f32", "L2", _mask(n)),
                  f"deleted {kind} n={n}")


def test_duplicate_vectors():
    from sptag_amd import AnnIndex
    g = load_golden("f32_l2_dups")
    q = g["queries"][:16]
    oix = OrcIndex.load(g["index"])
    ix = AnnIndex.Load(g["index"])
    for mc in (1, 64, 512):
        ov, od = oix.search_batch(q, 10, mc)
        gv, gd = ix.BatchSearch(q, 10, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"mc={mc} ids")
        np.testing.assert_array_equal(gd, od, err_msg=f"mc={mc} dists")


def test_lds_pass_then_global_heap_pass(monkeypatch, capfd):
    import re
    from sptag_amd import AnnIndex
    g = load_golden("f32_l2_n10k_d32")
    q = g["queries"][:64]
    ov, od = OrcIndex.load(g["index"]).search_batch(q, 10, 2048)
    ix = AnnIndex.Load(g["index"])
    monkeypatch.setenv("SPTAG_AMD_NG_CAP", "256")
    monkeypatch.setenv("SPTAG_AMD_DEBUG", "1")
    capfd.readouterr()
    gv, gd = ix.BatchSearch(q, 10, 2048)
    m = re.search(r"(\d+)/64 queries overflowed", capfd.readouterr().err)
    assert m and int(m.group(1)) > 0
    np.testing.assert_array_equal(gv, ov)
    np.testing.assert_array_equal(gd, od)


@pytest.mark.parametrize("kind", ["built", "wide"])
def test_iterator_next_sequence(kind):
    c = _case(kind, 300, "f32", "L2")
    batches = [1, 8, 8, 3, 8]
    calls = orc_iter_run(orc_from_case(c), c["q"], 8192, batches)
    it = gpu_from_case(c).Iterate(c["q"], max_check=8192)
    assert_iter_calls_equal(it, calls, batches, f"iter {kind}")
    it.Close()
