"""build_bkt_tree / build_index_arrays with kmeans="hip": the tree's structure
and the recall of the recipe that test_build pins for the torch splits."""
import numpy as np
import pytest

from oracle.pyoracle import OrcIndex
from sptag_amd.build import build_bkt_tree, build_index_arrays
from test_build import make_clustered, check_tree

pytestmark = pytest.mark.gpu


def test_bkt_tree_hip_structure_and_repeatability():
    x, _ = make_clustered(5000, 16, 50)
    ts, tn = build_bkt_tree(x, kmeans="hip", big_cluster=512)
    check_tree(tn, 5000)
    ts2, tn2 = build_bkt_tree(x, kmeans="hip", big_cluster=512)
    np.testing.assert_array_equal(ts, ts2)
    np.testing.assert_array_equal(tn, tn2)


@pytest.mark.parametrize("dm", ["L2", "Cosine"])
def test_build_and_search_recall_hip_kmeans(dm):
    n = 20000
    x, q = make_clustered(n, 32, 200, nq=200)
    arrays = build_index_arrays(x, dm, kmeans="hip", ntrees=4, tpt_leaf=500, refine_rounds=1)
    check_tree(arrays["tree_nodes"], n)
    ix = OrcIndex.from_arrays(arrays["vectors"], arrays["tree_start"], arrays["tree_nodes"],
                              arrays["graph"], dm)
    if dm == "Cosine":
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    tv, _ = ix.truth(q, 10, nthreads=4)
    vids, _ = ix.search_batch(q, 10, 2048, nthreads=4)
    recall = sum(len(set(tv[i]).intersection(vids[i])) for i in range(len(q))) / (len(q) * 10)
    print(f"kmeans=hip {dm}: recall@10 = {recall:.4f}")
    assert recall > 0.95, recall
