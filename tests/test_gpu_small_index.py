"""Indexes smaller than a wave, than k, or than the graph degree: n = 5 gives
a 32-wide graph row that is mostly -1, n = 65 is one past a wave, n = 300 is
below every default capacity. Built on the CPU with a fixed seed; the GPU is
compared bit-exactly with the oracle, and the oracle with numpy brute force
in float64 (exact integers for int8). n = 1 and n = 2 are CPU-only."""
import numpy as np
import pytest

from parity_util import (MAXDIST, brute_force_topk, built_case, gpu_from_case,
                         orc_from_case, orc_iter_run)

SIZES = [5, 65, 300]
TYPES = [("f32", "L2"), ("i8", "Cosine")]
ALGOS = ["BKT", "KDT"]
MAXCHECKS = [1, 64, 8192]
_ref = {}


def _case_ref(n, vt, dm, algo):
    """Oracle search/truth answers of one built index; computed once."""
    key = (n, vt, dm, algo)
    if key not in _ref:
        c = built_case(n, 16, vt, dm, algo)
        oix = orc_from_case(c)
        r = {"search": {}, "truth": {}}
        for k in sorted({1, n, n + 3}):
            for mc in MAXCHECKS:
                r["search"][(k, mc)] = oix.search_batch(c["q"], k, mc)
        for k in (1, n + 3):
            r["truth"][k] = oix.truth(c["q"], k)
        _ref[key] = (c, r)
    return _ref[key]


def _check_padding(v, d, nvalid):
    assert ((v >= 0).sum(1) == nvalid).all()
    assert (v[:, nvalid:] == -1).all()
    assert (d[:, nvalid:] == MAXDIST).all()
    for row in v[:, :nvalid]:
        assert len(set(row.tolist())) == nvalid


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("n", [1, 2] + SIZES)
def test_oracle_small_index_vs_brute_force(n, vt, dm, algo):
    """Truth equals float64 brute force by (distance, id); a search at
    MaxCheck 8192 with k = n+3 finds all n and pads with -1 / MaxDist."""
    c, r = _case_ref(n, vt, dm, algo)
    vec, q = c["args"][0], c["q"]
    tv, td = r["truth"][n + 3]
    bv, bd = brute_force_topk(vec, q, n + 3, dm)
    _check_padding(tv, td, n)
    if vt == "i8":
        np.testing.assert_array_equal(tv, bv)
        np.testing.assert_array_equal(td[:, :n], bd[:, :n].astype(np.float32))
    else:
        # float32 rounding may swap near-ties; order by the oracle's own
        # distances must hold and the sets must agree
        assert (np.diff(td[:, :n].astype(np.float64), axis=1) >= 0).all()
        for a, b in zip(tv, bv):
            assert set(a.tolist()) == set(b.tolist())
        np.testing.assert_allclose(td[:, :n], bd[:, :n], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(r["truth"][1][0][:, 0], tv[:, 0])
    # k < n, where the ids are a real choice among the n
    kk = (n + 1) // 2
    hv, hd = orc_from_case(c).truth(q, kk)
    if vt == "i8":
        np.testing.assert_array_equal(hv, bv[:, :kk])
    else:
        for a, b in zip(hv, bv[:, :kk]):
            assert set(a.tolist()) == set(b.tolist())
        np.testing.assert_array_equal(hv[:, 0], bv[:, 0])
    np.testing.assert_array_equal(hv, tv[:, :kk])
    np.testing.assert_array_equal(hd, td[:, :kk])
    sv, sd = r["search"][(n + 3, 8192)]
    _check_padding(sv, sd, n)
    np.testing.assert_array_equal(sv, tv)
    np.testing.assert_array_equal(sd, td)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_gpu_small_index_search_and_truth(n, vt, dm, algo):
    c, r = _case_ref(n, vt, dm, algo)
    ix = gpu_from_case(c)
    for (k, mc), (ov, od) in r["search"].items():
        gv, gd = ix.BatchSearch(c["q"], k, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"k={k} mc={mc}")
        np.testing.assert_array_equal(gd, od, err_msg=f"k={k} mc={mc}")
    for k, (ov, od) in r["truth"].items():
        gv, gd = ix.Truth(c["q"], k)
        np.testing.assert_array_equal(gv, ov, err_msg=f"truth k={k}")
        np.testing.assert_array_equal(gd, od, err_msg=f"truth k={k}")
    gv, gd = ix.BatchSearch(c["q"], n + 3, 8192)
    _check_padding(gv, gd, n)


def _iter_ref(n, vt, dm, deleted=None):
    key = ("iter", n, vt, dm, None if deleted is None else deleted.tobytes())
    if key not in _ref:
        c = built_case(n, 16, vt, dm, "BKT")
        live = n if deleted is None else int((deleted == 0).sum())
        batches = [8] * (live // 8 + 3)
        _ref[key] = (c, batches, orc_iter_run(orc_from_case(c, deleted), c["q"],
                                              8192, batches))
    return _ref[key]


@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_small_iter_exhausts(n, vt, dm):
    c, batches, calls = _iter_ref(n, vt, dm)
    for i in range(len(c["q"])):
        ids = np.concatenate([v[i, :cnt[i]] for v, _, cnt, _ in calls])
        assert sorted(ids.tolist()) == list(range(n))
        for v, d, cnt, _ in calls:
            assert (np.diff(d[i, :cnt[i]]) >= 0).all()
    assert (calls[-1][2] == 0).all() and (calls[-2][2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("vt,dm", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_gpu_small_iter_to_exhaustion(n, vt, dm):
    from parity_util import assert_iter_calls_equal
    c, batches, calls = _iter_ref(n, vt, dm)
    it = gpu_from_case(c).Iterate(c["q"], max_check=8192)
    assert_iter_calls_equal(it, calls, batches, f"n={n}")
    it.Close()


# ---- all but two deleted ------------------------------------------------

KEEP = (17, 64)     # one id inside the first wave, the one past it


def _mask65():
    m = np.ones(65, dtype=np.uint8)
    m[list(KEEP)] = 0
    return m


@pytest.mark.parametrize("algo", ALGOS)
def test_oracle_all_but_two_deleted(algo):
    c = built_case(65, 16, "f32", "L2", algo)
    oix = orc_from_case(c, _mask65())
    tv, td = oix.truth(c["q"], 5)
    bv, _ = brute_force_topk(c["args"][0], c["q"], 5, "L2", deleted=_mask65())
    np.testing.assert_array_equal(tv, bv)
    _check_padding(tv, td, 2)
    sv, sd = oix.search_batch(c["q"], 5, 8192)
    np.testing.assert_array_equal(sv, tv)
    np.testing.assert_array_equal(sd, td)
    if algo == "BKT":
        _, _, calls = _iter_ref(65, "f32", "L2", _mask65())
        assert (calls[0][2] == 2).all() and (calls[1][2] == 0).all()
        np.testing.assert_array_equal(calls[0][0][:, :2], tv[:, :2])


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ALGOS)
def test_gpu_all_but_two_deleted(algo):
    from parity_util import assert_iter_calls_equal
    c = built_case(65, 16, "f32", "L2", algo)
    oix = orc_from_case(c, _mask65())
    ix = gpu_from_case(c, _mask65())
    assert ix.deleted_count == 63
    for k, mc in [(1, 64), (5, 64), (5, 8192), (68, 8192)]:
        ov, od = oix.search_batch(c["q"], k, mc)
        gv, gd = ix.BatchSearch(c["q"], k, mc)
        np.testing.assert_array_equal(gv, ov, err_msg=f"k={k} mc={mc}")
        np.testing.assert_array_equal(gd, od, err_msg=f"k={k} mc={mc}")
    ov, od = oix.truth(c["q"], 5)
    gv, gd = ix.Truth(c["q"], 5)
    np.testing.assert_array_equal(gv, ov)
    np.testing.assert_array_equal(gd, od)
    if algo == "BKT":
        _, batches, calls = _iter_ref(65, "f32", "L2", _mask65())
        it = ix.Iterate(c["q"], max_check=8192)
        assert_iter_calls_equal(it, calls, batches, "masked")
        it.Close()


def test_kdt_builder_single_point_tree_terminates():
    """A one-point KDT never reaches a split. Its root's children must be
    leaves: a root that named itself as a child would make every descent
    (oracle and kernel alike) loop for ever."""
    from sptag_amd.build import build_kdt_tree
    start, nodes = build_kdt_tree(np.ones((1, 16), dtype=np.float32),
                                  device="cpu")
    assert start.tolist() == [0] and nodes.shape == (1, 4)
    assert nodes[0, 0] == -1          # leaf of vector 0
    assert nodes[0, 1] == -2          # empty side: id n, ignored by search
