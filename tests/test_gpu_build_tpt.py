"""build_rng_graph / build_index_arrays with tpt="hip": repeatable graphs over
ragged leaves, and the recall of the recipe that test_build pins for the torch
partition."""
import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd.build import build_rng_graph, build_index_arrays
from test_build import make_clustered, check_tree

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("leaf_knn", ["torch", "hip"])
def test_rng_graph_hip_tpt_repeatability(leaf_knn):
    x, _ = make_clustered(5000, 16, 50)
    a = build_rng_graph(x, tpt="hip", tpt_leaf=200, leaf_knn=leaf_knn)
    b = build_rng_graph(x, tpt="hip", tpt_leaf=200, leaf_knn=leaf_knn)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.cpu().numpy(), v.cpu().numpy())
    assert (a[0][:, 0] >= 0).all()


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
def test_build_and_search_recall_hip_tpt(dm):
    n = 20000
    x, q = make_clustered(n, 32, 200, nq=200)
    arrays = build_index_arrays(x, dm, tpt="hip", ntrees=4, tpt_leaf=500, refine_rounds=1)
    check_tree(arrays["tree_nodes"], n)
    ix = OrcIndex.from_arrays(arrays["vectors"], arrays["tree_start"], arrays["tree_nodes"],
                              arrays["graph"], dm)
    if dm == "Cosine":
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    tv, _ = ix.truth(q, 10, nthreads=4)
    vids, _ = ix.search_batch(q, 10, 2048, nthreads=4)
    recall = sum(len(set(tv[i]).intersection(vids[i])) for i in range(len(q))) / (len(q) * 10)
    print(f"tpt=hip {dm}: recall@10 = {recall:.4f}")
    assert recall > 0.95, recall
