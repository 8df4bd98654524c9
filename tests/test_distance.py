"""Distance unit tests — the reference DistanceTest.cpp:36-50 analog:
the backend's distance must match a plain scalar reference within 1e-5
relative for float, and exactly for int8 (integer distances are exact in
the reference — SURVEY.md §8a row a4)."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle
from parity_util import GOLDEN, load_dist_pairs


def scalar_l2(x, y):
    d = x.astype(np.float64) - y.astype(np.float64)
    return float((d * d).sum())


def scalar_cos(x, y, base):
    return base * base - float((x.astype(np.float64) * y.astype(np.float64)).sum())


@pytest.mark.parametrize("dim", [2, 3, 8, 10, 12, 16, 24, 31, 32, 48, 100, 128, 200,
                                 256, 768])
@pytest.mark.parametrize("dm", [0, 1])
def test_f32_distance_close(dim, dm):
    rng = np.random.default_rng(dim * 10 + dm)
    lib = pyoracle.load_library()
    for _ in range(20):
        x = rng.random(dim, dtype=np.float32)
        y = rng.random(dim, dtype=np.float32)
        got = lib.orc_distance(0, dm, x.ctypes.data_as(ctypes.c_void_p),
                               y.ctypes.data_as(ctypes.c_void_p), dim)
        want = scalar_l2(x, y) if dm == 0 else 1.0 - float(
            (x.astype(np.float64) * y.astype(np.float64)).sum())
        assert got == pytest.approx(want, rel=1e-5, abs=1e-6)


@pytest.mark.parametrize("dim", [2, 4, 8, 10, 12, 24, 100, 128, 256, 260])
@pytest.mark.parametrize("dm", [0, 1])
def test_i8_distance_exact(dim, dm):
    rng = np.random.default_rng(dim * 10 + dm)
    lib = pyoracle.load_library()
    for _ in range(20):
        x = rng.integers(-128, 128, dim).astype(np.int8)
        y = rng.integers(-128, 128, dim).astype(np.int8)
        got = lib.orc_distance(1, dm, x.ctypes.data_as(ctypes.c_void_p),
                               y.ctypes.data_as(ctypes.c_void_p), dim)
        want = scalar_l2(x, y) if dm == 0 else scalar_cos(x, y, 127)
        assert got == want  # exact integers


# --- pinned to the reference's own ComputeDistance ------------------------
#
# tests/golden/dist_pairs_*.bin hold seeded pairs at every dim form and
# dist_ref_*.bin what the reference computed on them on its AVX512 path
# (oracle/distprobe.cpp, `gen_golden.py dist`).

F32_DIMS = list(range(1, 145)) + [160, 192, 255, 256, 257, 384, 512, 513, 768,
                                  1024, 4096]
I8_DIMS = list(range(1, 145)) + [160, 192, 255, 256, 257, 258, 259, 260]


def test_dist_fixture_covers_every_dim_form():
    import json
    import os
    meta = json.load(open(os.path.join(GOLDEN, "dist_pairs.json")))
    assert meta["instruction_set"] == "AVX512"   # the order the oracle restates
    for tag, want in [("f32", F32_DIMS), ("i8", I8_DIMS)]:
        dims, pairs, ref = load_dist_pairs(tag)
        assert dims == want == meta[tag]["dims"]
        assert ref.shape == (len(dims), meta["pairs_per_dim"], 2)
        assert meta["pairs_per_dim"] >= 3
        assert np.isfinite(ref).all()


@pytest.mark.parametrize("tag", ["f32", "i8"])
def test_oracle_distance_equals_reference_bitwise(tag):
    """orc_distance gives the recorded value, bit for bit, for every pair and
    both metrics."""
    lib = pyoracle.load_library()
    dims, pairs, ref = load_dist_pairs(tag)
    bad = []
    for di, (d, pr) in enumerate(zip(dims, pairs)):
        for p in range(pr.shape[0]):
            x = np.ascontiguousarray(pr[p, 0])
            y = np.ascontiguousarray(pr[p, 1])
            for dm in (0, 1):
                got = np.float32(lib.orc_distance(
                    0 if tag == "f32" else 1, dm,
                    x.ctypes.data_as(ctypes.c_void_p),
                    y.ctypes.data_as(ctypes.c_void_p), d))
                if got.view(np.uint32) != ref[di, p, dm].view(np.uint32):
                    bad.append((d, p, dm, float(got), float(ref[di, p, dm])))
    assert not bad, f"{len(bad)} differ, first (dim, pair, metric, got, ref): {bad[:5]}"


def test_recorded_f32_within_derived_bound_of_float64():
    """A float32 fma chain and fold of d terms, in any order, is within
    (d + 3) * 2^-23 * S of the exact sum: S = sum (x-y)^2 for L2; for cosine
    S = sum |x*y|, plus 2^-24 for the final 1 - s. Exact and S in float64."""
    dims, pairs, ref = load_dist_pairs("f32")
    bad = []
    for di, (d, pr) in enumerate(zip(dims, pairs)):
        x = pr[:, 0].astype(np.float64)
        y = pr[:, 1].astype(np.float64)
        l2 = ((x - y) ** 2).sum(1)
        dot = (x * y).sum(1)
        sabs = np.abs(x * y).sum(1)
        k = (d + 3) * 2.0 ** -23
        for p in range(pr.shape[0]):
            if abs(float(ref[di, p, 0]) - l2[p]) > k * l2[p]:
                bad.append((d, p, "L2", float(ref[di, p, 0]), l2[p]))
            if abs(float(ref[di, p, 1]) - (1.0 - dot[p])) > k * sabs[p] + 2.0 ** -24:
                bad.append((d, p, "Cosine", float(ref[di, p, 1]), 1.0 - dot[p]))
    assert not bad, f"{len(bad)} outside the bound: {bad[:5]}"


def test_recorded_i8_is_exact_integer_rounded_once():
    dims, pairs, ref = load_dist_pairs("i8")
    bad = []
    for di, (d, pr) in enumerate(zip(dims, pairs)):
        for p in range(pr.shape[0]):
            x = [int(v) for v in pr[p, 0]]
            y = [int(v) for v in pr[p, 1]]
            l2 = sum((a - b) ** 2 for a, b in zip(x, y))
            cos = 127 * 127 - sum(a * b for a, b in zip(x, y))
            for dm, exact in ((0, l2), (1, cos)):
                assert abs(exact) < 2 ** 53       # float64 holds it exactly
                if np.float32(np.float64(exact)) != ref[di, p, dm]:
                    bad.append((d, p, dm, exact, float(ref[di, p, dm])))
    assert not bad, f"{len(bad)} differ: {bad[:5]}"
    # the largest pair really is past 2^24, where float32 stops holding
    # every integer: rounding once is a claim, not a tautology
    assert 260 * 255 * 255 > 2 ** 24
