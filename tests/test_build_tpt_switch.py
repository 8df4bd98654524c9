"""The builder's tpt switch: its values, and that "hip" refuses vectors on
the CPU."""
import numpy as np
import pytest

from sptag_amd import build

X = np.random.default_rng(1).standard_normal((300, 8)).astype(np.float32)


@pytest.mark.parametrize("fn", [lambda **kw: build.build_rng_graph(X, **kw),
                                lambda **kw: build.build_index_arrays(X, "L2", **kw)])
def test_tpt_switch(fn):
    with pytest.raises(ValueError, match="tpt"):
        fn(tpt="bogus", device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        fn(tpt="hip", device="cpu")
