"""The batched search decides a whole adjacency row's results-queue accepts
at once (kernels.hip, dpq_accept_row) and then runs the row's frontier
inserts back to back. Everything here is compared bit for bit, ids and
float distances, with the oracle; `checked` is compared with the oracle's own
count of distance evaluations, and `checked` and `popped` must not depend on
where the frontier heap is stored.

The results queue holds cap = max(MaxCheck/16, k) distances in 64-slot
chunks, so the sizes are chosen around the chunk: below one chunk (10, and
k above MaxCheck/16), exactly one (64), one past (65), a partial second
(100), two (128), one past two (129), and more than two (200 from k, 256).

Frontier placement is read from the environment by every search; those
cases run in a fresh child process per setting (this file is its own child
program) with the capacities that tests/test_gpu_ng_tier.py measured: at
SPTAG_AMD_NG_CAP 448 every query of f32_l2_n10k_d32 fills more than 320
frontier entries, of which 255, 127 or 63 are in LDS, so the inserts of one
row land in the global tail and the parent warm's slots are real ones; 384
makes some queries overflow into the global-heap rerun, 256 all of them.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

if __name__ == "__main__":      # child: one search under the caller's environment
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sptag_amd import AnnIndex
    folder, qfile, k, mc, out = sys.argv[1:6]
    ix = AnnIndex.Load(folder)
    v, d = ix.BatchSearch(np.load(qfile), int(k), int(mc))
    _, checked, popped = ix.LastStats()
    np.savez(out, v=v, d=d, stats=np.array([checked, popped], dtype=np.int64))
    sys.exit(0)

import pytest

from conftest import load_golden
from oracle.pyoracle import OrcIndex
from parity_util import built_case, gpu_from_case, orc_from_case
from sptag_amd import AnnIndex

pytestmark = pytest.mark.gpu

NQ = 32
_gold, _oracle_ix, _gpu_ix, _ref = {}, {}, {}, {}


def _golden(name):
    if name not in _gold:
        _gold[name] = load_golden(name)
    return _gold[name]


def orc_search_counted(oix, queries, k, mc):
    """(vids, dists, checked [nq]) of the oracle, one orc_search per query:
    its return value is the query's number of distance evaluations."""
    queries = oix._qarr(queries)
    v = np.empty((len(queries), k), dtype=np.int32)
    d = np.empty((len(queries), k), dtype=np.float32)
    checked = np.zeros(len(queries), dtype=np.int64)
    for i, q in enumerate(queries):
        q = np.ascontiguousarray(q)
        checked[i] = oix._lib.orc_search(
            oix._h, q.ctypes.data_as(ctypes.c_void_p), k, mc,
            v[i].ctypes.data_as(ctypes.c_void_p), d[i].ctypes.data_as(ctypes.c_void_p))
    return v, d, checked


def _fixture_ref(name, k, mc, nq=NQ):
    """Oracle answer of the first nq golden queries; computed once."""
    key = (name, k, mc, nq)
    if key not in _ref:
        if name not in _oracle_ix:
            _oracle_ix[name] = OrcIndex.load(_golden(name)["index"])
        _ref[key] = orc_search_counted(_oracle_ix[name], _golden(name)["queries"][:nq],
                                       k, mc)
    return _ref[key]


def _fixture_gpu(name):
    if name not in _gpu_ix:
        _gpu_ix[name] = AnnIndex.Load(_golden(name)["index"])
    return _gpu_ix[name]


def assert_bits_equal(v, d, rv, rd, tag):
    np.testing.assert_array_equal(v, rv, err_msg=f"{tag} ids")
    np.testing.assert_array_equal(np.ascontiguousarray(d).view(np.uint32),
                                  np.ascontiguousarray(rd).view(np.uint32),
                                  err_msg=f"{tag} dists")


def _search_and_compare(ix, q, k, mc, ref, tag):
    rv, rd, rchecked = ref
    v, d = ix.BatchSearch(q, k, mc)
    _, checked, popped = ix.LastStats()
    print(f"{tag}: checked {checked} (oracle {rchecked.sum()}) popped {popped}")
    assert_bits_equal(v, d, rv, rd, tag)
    assert checked == rchecked.sum(), tag


# ---------------------------------------------------------------------------
# equal distances inside one row and equal to the queue's maximum
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mc", [512, 2048])
@pytest.mark.parametrize("name", ["f32_l2_grid_ties", "f32_l2_dups"])
def test_tie_fixtures_at_golden_k(name, mc):
    g = _golden(name)
    k = g["meta"]["k"]
    assert k == (3 if name == "f32_l2_grid_ties" else 10)
    nq = 64
    ref = _fixture_ref(name, k, mc, nq)
    gold = g["results"][mc][:nq]
    assert_bits_equal(ref[0], ref[1], gold["vid"], gold["dist"], f"{name} oracle")
    _search_and_compare(_fixture_gpu(name), g["queries"][:nq], k, mc, ref,
                        f"{name} mc={mc}")


# ---------------------------------------------------------------------------
# queue sizes around the 64-slot chunk, on every element type
# ---------------------------------------------------------------------------

# (MaxCheck, k, cap)
QUEUE_SIZES = [(64, 10, 10), (1024, 10, 64), (1040, 10, 65), (1600, 10, 100),
               (2048, 10, 128), (2064, 10, 129), (4096, 10, 256), (512, 200, 200)]
# f32 L2, f32 cosine, int8 (many exact ties)
TYPE_FIXTURES = ["f32_l2_n10k_d32", "f32_cos_n10k_d48", "i8_cos_n20k_d100"]


@pytest.mark.parametrize("mc,k,cap", QUEUE_SIZES)
@pytest.mark.parametrize("name", TYPE_FIXTURES)
def test_queue_sizes(name, mc, k, cap):
    assert max(mc // 16, k) == cap      # host.cpp base_cfg, WorkSpace.h:268
    _search_and_compare(_fixture_gpu(name), _golden(name)["queries"][:NQ], k, mc,
                        _fixture_ref(name, k, mc), f"{name} mc={mc} k={k}")


# ---------------------------------------------------------------------------
# queues that never fill, and one that fills inside a row
# ---------------------------------------------------------------------------

def _built_ref(n, vt, dm, k, mc):
    key = ("built", n, vt, dm, k, mc)
    if key not in _ref:
        c = built_case(n, 16, vt, dm, "BKT")
        _ref[key] = (c, orc_search_counted(orc_from_case(c), c["q"], k, mc))
    return _ref[key]


@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("f32", "Cosine"), ("i8", "Cosine")])
@pytest.mark.parametrize("n", [5, 65, 300])
def test_queue_never_full(n, vt, dm):
    """MaxCheck 8192 gives 512 slots, more than the index has vectors, and a
    vector enters the queue at most once."""
    c, ref = _built_ref(n, vt, dm, 10, 8192)
    assert n < 8192 // 16
    _search_and_compare(gpu_from_case(c), c["q"], 10, 8192, ref, f"n={n} {vt} {dm}")


@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "Cosine")])
def test_queue_fills_inside_a_row(vt, dm):
    """300 vectors, rows of up to 32 neighbours, and queues of 20, 33 and 47
    slots. While the queue is not full it takes every candidate, and every
    query evaluates more than twice as many as it holds (checked below), so
    it fills; with three sizes and eight queries it cannot fill at the last
    candidate of a row every time."""
    c = built_case(300, 16, vt, dm, "BKT")
    ix = gpu_from_case(c)
    for cap in (20, 33, 47):
        _, ref = _built_ref(300, vt, dm, 10, 16 * cap)
        assert (ref[2] > 2 * cap).all()
        _search_and_compare(ix, c["q"], 10, 16 * cap, ref, f"{vt} {dm} cap={cap}")


# ---------------------------------------------------------------------------
# frontier placement: a fresh process per setting
# ---------------------------------------------------------------------------

def _child_search(tmp_path, name, nq, k, mc, env):
    g = _golden(name)
    qfile, out = tmp_path / "q.npy", tmp_path / "out.npz"
    np.save(qfile, g["queries"][:nq])
    p = subprocess.run(
        [sys.executable, os.path.abspath(__file__), g["index"], str(qfile), str(k),
         str(mc), str(out)],
        env=dict(os.environ, SPTAG_AMD_DEBUG="1", **env),
        capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    r = np.load(out)
    m = re.search(r"(\d+)/%d queries overflowed" % nq, p.stderr)
    n_over = int(m.group(1)) if m else 0
    m = re.search(r"global-heap pass for (\d+)/%d" % nq, p.stderr)
    n_global = int(m.group(1)) if m else 0
    return r["v"], r["d"], tuple(r["stats"].tolist()), n_over, n_global


# (fixture, SPTAG_AMD_NG_CAP, SPTAG_AMD_NG_GLEVELS, queries expected in the
# global-heap rerun: none, some, all)
PLACEMENTS = [
    ("f32_l2_n10k_d32", 448, 0, "none"), ("f32_l2_n10k_d32", 448, 1, "none"),
    ("f32_l2_n10k_d32", 448, 2, "none"), ("f32_l2_n10k_d32", 448, 3, "none"),
    ("f32_l2_n10k_d32", 384, 2, "some"), ("f32_l2_n10k_d32", 256, 3, "all"),
    ("i8_cos_deg48", 512, 3, "none"),
]
_stats_seen = {}


@pytest.mark.parametrize("name,cap,g,rerun", PLACEMENTS)
def test_frontier_placement(tmp_path, name, cap, g, rerun):
    nq, k, mc = 64, 10, 2048
    ref = _fixture_ref(name, k, mc, nq)
    v, d, stats, n_over, n_global = _child_search(
        tmp_path, name, nq, k, mc,
        {"SPTAG_AMD_NG_CAP": str(cap), "SPTAG_AMD_NG_GLEVELS": str(g)})
    print(f"{name} NG_CAP {cap} G={g}: {n_over}/{nq} overflowed, {n_global} rerun, "
          f"checked {stats[0]} (oracle {ref[2].sum()}) popped {stats[1]}")
    if rerun == "none":
        assert n_over == 0 and n_global == 0
    elif rerun == "some":
        assert 0 < n_over <= nq // 2 and n_global == n_over
    else:
        assert n_over == nq and n_global == nq
    assert_bits_equal(v, d, ref[0], ref[1], f"{name} cap={cap} G={g}")
    assert stats[0] == ref[2].sum()
    # the traversal is the same wherever the frontier is stored
    assert _stats_seen.setdefault(name, stats) == stats
