"""The builder's kmeans switch: its values, and that "hip" refuses vectors
on the CPU."""
import numpy as np
import pytest

from sptag_amd import build

X = np.random.default_rng(1).standard_normal((300, 8)).astype(np.float32)


@pytest.mark.parametrize("fn", [lambda **kw: build.build_bkt_tree(X, **kw),
                                lambda **kw: build.build_index_arrays(X, "L2", **kw)])
def test_kmeans_switch(fn):
    with pytest.raises(ValueError, match="kmeans"):
        fn(kmeans="bogus", device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        fn(kmeans="hip", device="cpu")
