"""The batched search evaluates its frontier and tree heaps with the whole
wave (kernels.hip, ndheap_insert_wave and ndheap_pop_wave). The heap itself
is checked in tests/test_gpu_heap_ops.py; here the search is compared end to
end with the oracle, ids and float bits, and `checked` with the oracle's own
count of distance evaluations:

- fixtures full of equal distances, down to MaxCheck 8, where the planner
  gives both heaps the reference's capacities (plan.h: MaxCheck below 18 and
  410) and a full heap replaces its largest last-level entry;
- every placement of the frontier heap: all in LDS, three levels in the
  global tail, and a capacity that sends every query to the global-heap
  rerun, each in a fresh child process (the settings are read from the
  environment);
- indexes of 1, 2, 33 and 300 vectors.
"""
import numpy as np
import pytest

from parity_util import built_case, gpu_from_case, orc_from_case
from test_gpu_insert_batch import (_child_search, _fixture_gpu, _fixture_ref,
                                   _search_and_compare, _golden, assert_bits_equal,
                                   orc_search_counted)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mc", [8, 64, 512])
@pytest.mark.parametrize("name,k", [("f32_l2_grid_ties", 3), ("f32_l2_dups", 10)])
def test_tie_fixtures_small_maxcheck(name, k, mc):
    nq = 64
    _search_and_compare(_fixture_gpu(name), _golden(name)["queries"][:nq], k, mc,
                        _fixture_ref(name, k, mc, nq), f"{name} k={k} mc={mc}")


@pytest.mark.parametrize("cap", [448, 256])
@pytest.mark.parametrize("glevels", [0, 3])
@pytest.mark.parametrize("name", ["f32_l2_n10k_d32", "i8_cos_deg48"])
def test_frontier_placements(tmp_path, name, glevels, cap):
    nq, k, mc = 64, 10, 2048
    ref = _fixture_ref(name, k, mc, nq)
    v, d, stats, n_over, n_global = _child_search(
        tmp_path, name, nq, k, mc,
        {"SPTAG_AMD_NG_CAP": str(cap), "SPTAG_AMD_NG_GLEVELS": str(glevels)})
    print(f"{name} NG_CAP {cap} G={glevels}: {n_over}/{nq} overflowed, {n_global} "
          f"rerun, checked {stats[0]} (oracle {ref[2].sum()}) popped {stats[1]}")
    if name == "f32_l2_n10k_d32":
        # measured in tests/test_gpu_ng_tier.py: no query needs more than 448
        # frontier entries, every query more than 256
        assert n_global == (nq if cap == 256 else 0)
    assert_bits_equal(v, d, ref[0], ref[1], f"{name} cap={cap} G={glevels}")
    assert stats[0] == ref[2].sum()


@pytest.mark.parametrize("n", [1, 2, 33, 300])
def test_tiny_indexes(n):
    c = built_case(n, 16, "f32", "L2", "BKT")
    k, mc = 10, 512
    ref = orc_search_counted(orc_from_case(c), c["q"], k, mc)
    _search_and_compare(gpu_from_case(c), c["q"], k, mc, ref, f"n={n}")
