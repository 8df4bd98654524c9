"""The two dimension classes of the float kernels (kernels.hip, DC_SMALL /
DC_LARGE): every kernel that computes a float distance exists once for dims
up to 128 (fixed forms 32..128 and the generic rolled form) and once for
larger dims (fixed forms 256/512/768 and the generic form), and the launchers
pick by the index's dim. The dims here sit on both sides of that choice:

  112  generic form in the small class
  128  last fixed form of the small class
  132  generic form in the large class (first dims past the boundary)
  256  first fixed form of the large class

On seeded random indexes of 2000 vectors built on the CPU, Truth, the batched
BKT search, the KDT search and two Next calls of an iterator must equal the
oracle's answers bit for bit, for both metrics. The oracle's answers are
computed once per (dim, metric) and shared.
"""
import numpy as np
import pytest

from parity_util import (assert_iter_calls_equal, built_case, gpu_from_case,
                         orc_from_case, orc_iter_run)

pytestmark = pytest.mark.gpu

N, NQ, K, MC = 2000, 16, 10, 512
DIMS = [112, 128, 132, 256]
ITER_BATCHES = [8, 8]

_ref = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(dim, dm):
    key = (dim, dm)
    if key not in _ref:
        bkt = built_case(N, dim, "f32", dm, "BKT", nq=NQ)
        kdt = built_case(N, dim, "f32", dm, "KDT", nq=NQ)
        obkt, okdt = orc_from_case(bkt), orc_from_case(kdt)
        _ref[key] = {
            "bkt": bkt, "kdt": kdt,
            "truth": obkt.truth(bkt["q"], K, nthreads=4),
            "search": obkt.search_batch(bkt["q"], K, MC, nthreads=4),
            "kdt_search": okdt.search_batch(kdt["q"], K, MC, nthreads=4),
            "iter": orc_iter_run(obkt, bkt["q"], MC, ITER_BATCHES)}
    return _ref[key]


def _assert_same(got, want, what):
    gv, gd = got
    wv, wd = want
    assert wv.shape == (NQ, K) and (wv >= 0).all() and (wv < N).all(), what
    np.testing.assert_array_equal(gv, wv, err_msg=what)
    np.testing.assert_array_equal(_bits(gd), _bits(wd), err_msg=what)


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
@pytest.mark.parametrize("dim", DIMS)
def test_truth_at_class_boundary(dim, dm):
    c = _case(dim, dm)
    _assert_same(gpu_from_case(c["bkt"]).Truth(c["bkt"]["q"], K), c["truth"],
                 f"Truth d={dim} {dm}")


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
@pytest.mark.parametrize("dim", DIMS)
def test_bkt_search_at_class_boundary(dim, dm):
    c = _case(dim, dm)
    _assert_same(gpu_from_case(c["bkt"]).BatchSearch(c["bkt"]["q"], K, MC),
                 c["search"], f"BKT d={dim} {dm}")


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
@pytest.mark.parametrize("dim", DIMS)
def test_kdt_search_at_class_boundary(dim, dm):
    c = _case(dim, dm)
    _assert_same(gpu_from_case(c["kdt"]).BatchSearch(c["kdt"]["q"], K, MC),
                 c["kdt_search"], f"KDT d={dim} {dm}")


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
@pytest.mark.parametrize("dim", DIMS)
def test_iterator_at_class_boundary(dim, dm):
    c = _case(dim, dm)
    for v, d, cnt, _ in c["iter"]:
        assert (cnt == 8).all() and (v >= 0).all()
    it = gpu_from_case(c["bkt"]).Iterate(c["bkt"]["q"], max_check=MC)
    assert_iter_calls_equal(it, c["iter"], ITER_BATCHES, f"iter d={dim} {dm}")
    it.Close()
