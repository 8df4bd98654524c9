"""bench.py's built-index cache and --dump-outputs writer (host-side logic).

The cache must hand back exactly the arrays the builder produced, never a
half-written folder, and its key must change with the data, the build
parameters and the shard. The dump holds float arrays with aligned rows.
"""
import os

import numpy as np

import bench


def _arrays(rng, n=64, degree=8):
    return {"tree_start": np.array([0], dtype=np.int32),
            "tree_nodes": rng.integers(-1, n, (n + 5, 3)).astype(np.int32),
            "graph": rng.integers(-1, n, (n, degree)).astype(np.int32),
            "vectors": rng.random((n, 4)).astype(np.float32)}


def test_index_cache_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    arrays = _arrays(rng)
    path = str(tmp_path / "cache" / "key")
    assert bench.index_cache_load(path) is None
    assert bench.index_cache_store(path, arrays)
    got = bench.index_cache_load(path)
    assert sorted(got) == ["graph", "tree_nodes", "tree_start"]
    for name, a in got.items():
        assert a.dtype == arrays[name].dtype
        np.testing.assert_array_equal(a, arrays[name])
    # a second writer of the same key keeps the first copy, leaves no litter
    assert bench.index_cache_store(path, _arrays(rng))
    np.testing.assert_array_equal(bench.index_cache_load(path)["graph"],
                                  arrays["graph"])
    assert os.listdir(str(tmp_path / "cache")) == ["key"]


def test_index_cache_refuses_oversized(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "INDEX_CACHE_MAX_BYTES", 16)
    path = str(tmp_path / "key")
    assert not bench.index_cache_store(path, _arrays(np.random.default_rng(4)))
    assert not os.path.exists(path)


def test_index_cache_key_tracks_data_params_and_shard():
    rng = np.random.default_rng(5)
    x = rng.random((10_000, 8)).astype(np.float32)
    kw = dict(algo="BKT", degree=32, cand=256)
    key = bench.index_cache_key("w", x, kw, 0, 1)
    assert key == bench.index_cache_key("w", x.copy(), dict(kw), 0, 1)
    y = x.copy()
    y[0, 0] += 1.0
    assert key != bench.index_cache_key("w", y, kw, 0, 1)
    assert key != bench.index_cache_key("w", x, dict(kw, degree=48), 0, 1)
    assert key != bench.index_cache_key("w", x, kw, 1, 2)
    assert key != bench.index_cache_key("v", x, kw, 0, 1)


def test_index_cache_root_follows_environment(tmp_path, monkeypatch):
    monkeypatch.setenv("SPTAG_AMD_CACHE", str(tmp_path / "a"))
    assert bench.index_cache_root() == str(tmp_path / "a" / "bench_index")
    monkeypatch.delenv("SPTAG_AMD_CACHE")
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "b"))
    assert bench.index_cache_root() == str(
        tmp_path / "b" / "sptag_amd" / "bench_index")


def test_dump_outputs_writes_float_arrays(tmp_path):
    vids = np.array([[7, 3, -1], [2_000_000_011, 5, 6]], dtype=np.int32)
    dists = np.array([[0.5, 1.5, 3.4e38], [0.0, 2.0, 4.0]], dtype=np.float32)
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, vids, dists)
    assert sorted(os.listdir(out)) == ["dists.npy", "vids.npy"]
    v = np.load(os.path.join(out, "vids.npy"))
    d = np.load(os.path.join(out, "dists.npy"))
    assert v.dtype == np.float64 and d.dtype == np.float32
    np.testing.assert_array_equal(v.astype(np.int64), vids)
    np.testing.assert_array_equal(d, dists)


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 44 * 10)   # 10 rows of k=3
    rng = np.random.default_rng(6)
    vids = rng.integers(0, 1000, (100, 3)).astype(np.int32)
    dists = rng.random((100, 3)).astype(np.float32)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, vids, dists)
    bench.dump_outputs(b, vids, dists)
    rows = np.load(os.path.join(a, "rows.npy"))
    assert rows.shape == (10,) and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, np.load(os.path.join(b, "rows.npy")))
    sel = rows.astype(np.int64)
    np.testing.assert_array_equal(
        np.load(os.path.join(a, "vids.npy")).astype(np.int64), vids[sel])
    np.testing.assert_array_equal(np.load(os.path.join(a, "dists.npy")),
                                  dists[sel])
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= 44 * 10 + 3 * 128   # payload + the three .npy headers
