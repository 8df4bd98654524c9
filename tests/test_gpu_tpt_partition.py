"""AnnIndex.TptPartition / tpt_partition_device against a plain numpy float32
restatement of the contract in include/sptag_amd.h: vectorised over columns
and over trials, sequential along the members, so every sum has the contract's
order and every operation is rounded once. All outputs are arg-max or
threshold decisions, so they are compared exactly."""
import ctypes
import functools

import numpy as np
import pytest

from sptag_amd import load_library, tpt_partition_device
from test_gpu_exact_search import DIM, N as MANY
from test_gpu_rng_prune import vectors, handle, N, BIG_N

pytestmark = pytest.mark.gpu

F = np.float32


def ordered_sum(rows):
    """rows[0] + rows[1] + .. from 0, in order, f32"""
    acc = np.zeros(rows.shape[1:], dtype=F)
    for r in rows:
        acc = acc + r
    return acc


def project(cols, w):
    """cols [m, T], w [.., T] -> [m, ..]: w_0*x_0 + w_1*x_1 + .. from 0 in order"""
    acc = np.zeros((cols.shape[0],) + w.shape[:-1], dtype=F)
    for j in range(cols.shape[1]):
        acc = acc + w[..., j] * cols[:, j].reshape((-1,) + (1,) * (w.ndim - 1))
    return acc


def draws(seed, level, first, trials, T):
    u = lambda v: np.array(v, dtype=np.uint64)
    t, j = np.arange(trials, dtype=np.uint64)[:, None], np.arange(T, dtype=np.uint64)[None, :]
    key = (((((u(level) << u(31)) | u(first)) << u(8)) | t) << u(3)) | j
    z = u(seed) + u(0x9E3779B97F4A7C15) * (u(1) + key)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z ^= z >> u(31)
    return (z >> u(32)) % u(10000)


def ref_rule(v, level, first, samples, topdims, trials, seed):
    """v [c, dim] f32, the segment's vectors in list order. Returns (idx, w,
    mean, whether a trial won)."""
    s = min(samples, len(v))
    smp, fs = v[:s], F(s)
    mean = ordered_sum(smp) / fs
    var = ordered_sum((smp - mean) ** 2)
    T = min(topdims, v.shape[1])
    idx = np.argsort(-np.where(np.isnan(var), F(-1), var), kind="stable")[:T]
    bw, bvar, bmean, won = np.eye(1, T, dtype=F)[0], var[idx[0]], mean[idx[0]], False
    if trials:
        w = draws(seed, level, first, trials, T).astype(F) / F(5000) - F(1)
        nn = np.zeros(trials, dtype=F)
        for j in range(T):
            nn = nn + w[:, j] * w[:, j]
        norm = np.sqrt(nn)
        w = w / np.where(norm == 0, F(1), norm)[:, None]
        val = project(smp[:, idx], w)                   # [s, trials]
        tmean = ordered_sum(val) / fs
        tvar = ordered_sum((val - tmean) ** 2)
        for t in range(trials):
            if norm[t] != 0 and tvar[t] > bvar:
                bw, bvar, bmean, won = w[t], tvar[t], tmean[t], True
    return idx, bw, bmean, won


@functools.lru_cache(maxsize=None)
def ref_partition(vt, n, d, kind, leaf, samples, topdims, trials, seed):
    """The contract. Returns (members, starts, counts) and (splits a trial
    won, splits that kept the axis rule, splits cut by rank)."""
    x = vectors(vt, n, d, kind).astype(F)
    out = member_list(n)
    leaves, won, kept, cut = [], 0, 0, 0
    segs, level = [(0, len(out))], 0
    with np.errstate(all="ignore"):
        while segs:
            nxt = []
            for first, c in segs:
                if c <= leaf:
                    leaves.append((first, c))
                    continue
                seg = out[first:first + c].copy()
                idx, w, mean, w_won = ref_rule(x[seg], level, first, samples, topdims, trials,
                                               seed)
                won, kept = won + w_won, kept + (not w_won)
                left = project(x[seg][:, idx], w) < mean
                nl = int(left.sum())
                if nl in (0, c):
                    nl, cut = c // 2, cut + 1
                else:
                    out[first:first + c] = np.concatenate([seg[left], seg[~left]])
                nxt += [(first, nl), (first + nl, c - nl)]
            segs, level = nxt, level + 1
    leaves = np.array(sorted(leaves), dtype=np.int32)
    return (out, leaves[:, 0], leaves[:, 1]), (won, kept, cut)


def member_list(n):
    return np.random.default_rng(5).permutation(n).astype(np.int32)


def check(vt, n, d, kind, leaf, samples=1000, topdims=5, trials=100, seed=1):
    want, stats = ref_partition(vt, n, d, kind, leaf, samples, topdims, trials, seed)
    gpu = handle(vt, "L2", n, d, kind)
    got = gpu.TptPartition(member_list(n), leaf, samples, topdims, trials, seed)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    return stats


@pytest.mark.parametrize("samples", [1, 50, 1000])
@pytest.mark.parametrize("vt,kind,d", [("f32", k, d) for k in ("ints", "real")
                                       for d in (3, 40, 131, 768)] +
                         [("i8", "ints", d) for d in (37, 64, 100)])
def test_tpt_partition_every_dimension_form(vt, kind, d, samples):
    check(vt, N, d, kind, 32, samples)      # d = 3: topdims 5 is clipped to 3


@pytest.mark.parametrize("trials", [0, 1, 100, 256])
def test_tpt_partition_axis_rule_kept(trials):
    won, kept, _ = check("f32", N, 40, "ints", 32, trials=trials)
    if trials == 0:
        assert won == 0 and kept > 0
    if trials == 1:
        assert won > 0 and kept > 0


@pytest.mark.parametrize("vt", ["f32", "i8"])
def test_tpt_partition_rank_cut(vt):
    assert check(vt, N, DIM[vt], "ties", 8)[2] > 0


def test_tpt_partition_several_items_and_many_levels():
    """the top segments hold many items and waves; a prime leaf size leaves
    segments of 1 and 2 at the deepest levels"""
    want, _ = ref_partition("f32", MANY, 40, "ints", 5, 1000, 5, 100, 1)
    assert want[2].min() == 1 and want[2].max() == 5
    check("f32", MANY, 40, "ints", 5)


def test_tpt_partition_kd_form_and_same_bytes_twice():
    check("f32", BIG_N, 131, "real", 16, topdims=1, trials=0)
    gpu = handle("f32", "L2", BIG_N, 131, "real")
    a = gpu.TptPartition(member_list(BIG_N), 16, seed=9)
    b = gpu.TptPartition(member_list(BIG_N), 16, seed=9)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("vt", ["f32", "i8"])
def test_tpt_partition_device_form_and_kdt_handle(vt):
    import torch
    d = DIM[vt]
    want, _ = ref_partition(vt, N, d, "ints", 32, 50, 5, 100, 3)
    got = handle(vt, "L2", N, d, "ints", kdt=True).TptPartition(member_list(N), 32, 50, seed=3)
    tx = torch.from_numpy(np.array(vectors(vt, N, d, "ints"))).to("cuda:0")
    tm = torch.from_numpy(member_list(N)).to("cuda:0")
    torch.cuda.synchronize()
    starts, counts = tpt_partition_device(tx.data_ptr(), 0 if vt == "f32" else 1, N, d,
                                          tm.data_ptr(), N, 32, tm.data_ptr(), samples=50, seed=3)
    for g, h, w in zip(got, (tm.cpu().numpy(), starts, counts), want):
        np.testing.assert_array_equal(g, w)
        np.testing.assert_array_equal(h, w)


def test_tpt_partition_max_leaves_and_argument_errors():
    lib = load_library()
    x = vectors("f32", N, 40, "ints")
    gpu = handle("f32", "L2", N, 40, "ints")
    want, _ = ref_partition("f32", N, 40, "ints", 32, 1000, 5, 100, 1)
    nl = len(want[1])
    members = member_list(N)
    outs = [np.full(N, -7, np.int32), np.full(N, -7, np.int32), np.full(N, -7, np.int32)]
    nleaves = np.full(1, -7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def changed(a, i, val):
        b = a.copy()
        b[i] = val
        return b
    good = (gpu._h, p(members), N, 32, 1000, 5, 100, 1, *[p(a) for a in outs], N, p(nleaves))
    # a leaf table too small: the needed number, nothing else
    assert lib.sptag_amd_tpt_partition(*[nl - 1 if i == 11 else a
                                         for i, a in enumerate(good)]) == -2
    assert nleaves[0] == nl and all((a == -7).all() for a in outs)
    assert lib.sptag_amd_tpt_partition(*[nl if i == 11 else a for i, a in enumerate(good)]) == 0
    for g, w in zip(outs, want):
        np.testing.assert_array_equal(g[:len(w)], w)
    for a in outs + [nleaves]:
        a[...] = -7
    bad = [{i: None} for i in (0, 1, 8, 9, 10, 12)]
    bad += [{2: 0}, {3: 0}, {4: 0}, {4: 2049}, {5: 0}, {5: 9}, {6: -1}, {6: 257}, {11: -1},
            {1: p(changed(members, 5, -1))}, {1: p(changed(members, 5, N))}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_tpt_partition(*args) == -2, b          # SPTAG_AMD_ERR_PARAM
    # the device form returns before it touches the device: any non-null
    # address stands for the buffers
    good = (0, p(x), 0, N, 40) + good[1:]
    bad = [{i: None} for i in (1, 5, 12, 13, 14, 16)]
    bad += [{6: 0}, {7: 0}, {8: 0}, {8: 2049}, {9: 0}, {9: 9}, {10: -1}, {10: 257}, {15: -1},
            {2: 2}, {3: 0}, {4: 0}, {4: 4097}, {2: 1, 4: 261}]
    for b in bad:
        args = [b.get(i, a) for i, a in enumerate(good)]
        assert lib.sptag_amd_tpt_partition_device(*args) == -2, b
    assert all((a == -7).all() for a in outs + [nleaves])
