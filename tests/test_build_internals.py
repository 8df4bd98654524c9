"""Unit tests of the builder's internal pieces (build.py): the TP-tree
partition, candidate merge, and RNG prune — each checked against a
straightforward numpy restatement of the same rule."""
import numpy as np
import pytest
import torch

from sptag_amd.build import (_tpt_leaves, _merge_candidates, _rng_prune,
                             _ragged_arange, _segmented_order,
                             _pos_in_segment, _pairwise_sq_l2, build_kdt_tree,
                             build_index_arrays)


def test_ragged_arange():
    np.testing.assert_array_equal(_ragged_arange([3, 1, 2]),
                                  [0, 1, 2, 0, 0, 1])
    assert _ragged_arange([]).size == 0
    assert _ragged_arange([5]).tolist() == [0, 1, 2, 3, 4]
    assert _ragged_arange([0, 2, 0, 0, 1]).tolist() == [0, 1, 0]


def test_tpt_leaves_partition():
    g = torch.Generator()
    g.manual_seed(1)
    x = torch.rand((5000, 8), generator=g)
    perm, starts, counts = _tpt_leaves(x, 200, g)
    bounds = list(zip(starts.tolist(), counts.tolist()))
    # bounds tile perm exactly; every point appears once
    total = sum(c for _, c in bounds)
    assert total == 5000
    assert sorted(perm.tolist()) == list(range(5000))
    assert all(c <= 200 for _, c in bounds)
    starts = sorted(s for s, _ in bounds)
    ends = sorted(s + c for s, c in bounds)
    assert starts[0] == 0 and ends[-1] == 5000


def test_merge_candidates_dedupe_and_order():
    ids_a = torch.tensor([[3, 1, -1, 7]], dtype=torch.int32)
    dst_a = torch.tensor([[1.0, 2.0, float("inf"), 9.0]])
    ids_b = torch.tensor([[1, 5, 0, 3]], dtype=torch.int32)
    dst_b = torch.tensor([[2.0, 0.5, 4.0, 1.0]])
    self_ids = torch.tensor([0], dtype=torch.int32)
    ci, cd = _merge_candidates(ids_a, dst_a, ids_b, dst_b, 6, self_ids)
    # nearest first, ids deduped (1 and 3 appear once), self (0) dropped,
    # padded to width 6 with -1/inf
    assert ci.shape == (1, 6)
    got = [(int(i), float(d)) for i, d in zip(ci[0], cd[0]) if i >= 0]
    assert got == [(5, 0.5), (3, 1.0), (1, 2.0), (7, 9.0)]
    assert ci[0, 4] == -1 and not torch.isfinite(cd[0, 4])


def naive_rng_prune(x, cand_ids, cand_dst, degree, factor=1.0):
    """direct restatement of RebuildNeighbors (ascending candidates,
    accept c iff factor*dist(b,c) >= dist(q,c) for all accepted b)."""
    out = np.full(degree, -1, dtype=np.int32)
    cnt = 0
    for j in range(len(cand_ids)):
        if cnt >= degree or not np.isfinite(cand_dst[j]):
            break
        good = True
        for b in out[:cnt]:
            d = ((x[b] - x[cand_ids[j]]) ** 2).sum()
            if factor * d < cand_dst[j]:
                good = False
                break
        if good:
            out[cnt] = cand_ids[j]
            cnt += 1
    return out


def test_rng_prune_matches_naive():
    g = torch.Generator()
    g.manual_seed(3)
    x = torch.rand((500, 8), generator=g)
    q_rows = torch.arange(20)
    # candidates: 24 random others per row, sorted by true distance
    cid = torch.randint(20, 500, (20, 24), generator=g, dtype=torch.int32)
    d = ((x[cid.long()] - x[q_rows][:, None, :]) ** 2).sum(-1)
    order = d.argsort(1)
    cid = torch.gather(cid, 1, order)
    cdd = torch.gather(d, 1, order)
    pruned = _rng_prune(x, cid, cdd, 8, 1.0).numpy()
    xn = x.numpy()
    for i in range(20):
        want = naive_rng_prune(xn, cid[i].numpy(), cdd[i].numpy(), 8)
        np.testing.assert_array_equal(pruned[i], want, err_msg=f"row {i}")


def test_kdt_tree_routes_every_point():
    """descending the built kd-tree by its own split rules reaches every
    vector exactly once (leaf ids -(v+1) partition the dataset)."""
    g = torch.Generator()
    g.manual_seed(5)
    x = torch.rand((2000, 12), generator=g).numpy().astype(np.float32)
    ts, nodes = build_kdt_tree(x, ntrees=2, device="cpu")
    n = x.shape[0]
    for t in range(2):
        seen = set()
        stack = [int(ts[t])]
        while stack:
            nd = stack.pop()
            if nd < 0:
                v = -nd - 1
                if v < n:
                    assert v not in seen
                    seen.add(v)
                continue
            stack.append(int(nodes[nd, 0]))
            stack.append(int(nodes[nd, 1]))
        assert len(seen) == n, (t, len(seen))


def test_rng_prune_fill_pruned():
    """fill_pruned pads leftover degree slots with the nearest REJECTED
    candidates (billion-scale build knob); the RNG-accepted prefix must be
    identical to the strict prune, and the filled row stays ascending."""
    torch.manual_seed(5)
    n, c, d, deg = 40, 24, 8, 12
    x = torch.randn(n, d)
    cdd0 = torch.rand(n, c).sort(dim=1).values * 10
    cid = torch.stack([torch.randperm(n)[:c] for _ in range(n)]).int()
    strict = _rng_prune(x, cid, cdd0, deg, 1.0).numpy()
    filled = _rng_prune(x, cid, cdd0, deg, 1.0,
                        fill_pruned=True).numpy()
    for i in range(n):
        s = strict[i][strict[i] >= 0]
        f = filled[i][filled[i] >= 0]
        assert len(f) >= len(s)
        assert len(f) == min(deg, c)  # all slots used (valid pool is full)
        # accepted set preserved (as a subsequence of the filled row)
        it = iter(f.tolist())
        assert all(v in it for v in s.tolist()) or set(s) <= set(f)
        # filled row ascending by the pool's distance order
        pos = {int(v): j for j, v in enumerate(cid[i].tolist())}
        order = [pos[int(v)] for v in f.tolist()]
        assert order == sorted(order)


# ---- the shared steps -------------------------------------------------------

def _seg_cases():
    """(key, seg) pairs: empty, one segment, segments of size 1, many equal
    keys, and unsorted segment ids with gaps in the sizes."""
    g = torch.Generator()
    g.manual_seed(11)
    return {
        "empty": (torch.zeros(0), torch.zeros(0, dtype=torch.int64)),
        "one segment": (torch.rand(9, generator=g),
                        torch.zeros(9, dtype=torch.int64)),
        "size-1 segments": (torch.rand(6, generator=g), torch.arange(6)),
        "equal keys": (torch.randint(0, 2, (40,), generator=g).float(),
                       torch.randint(0, 3, (40,), generator=g)),
        "mixed": (torch.rand(50, generator=g),
                  torch.randint(0, 7, (50,), generator=g)),
    }


def test_segmented_order_matches_lexsort():
    """Grouped by segment, sorted by key inside; with the stable flag equal
    keys keep their order, which np.lexsort (stable) restates. Without it
    only the order of distinct keys is promised."""
    for name, (key, seg) in _seg_cases().items():
        want = np.lexsort((key.numpy(), seg.numpy()))
        got = _segmented_order(key, seg, stable=True).numpy()
        np.testing.assert_array_equal(got, want, err_msg=name)
        got = _segmented_order(key, seg).numpy()
        assert sorted(got.tolist()) == list(range(key.numel())), name
        np.testing.assert_array_equal(seg.numpy()[got], seg.numpy()[want], name)
        np.testing.assert_array_equal(key.numpy()[got], key.numpy()[want], name)


def test_pos_in_segment_matches_loop():
    for counts in ([], [7], [1, 1, 1, 1], [3, 0, 2, 5, 0, 1]):
        want = [p for c in counts for p in range(c)]
        seg = [i for i, c in enumerate(counts) for _ in range(c)]
        got = _pos_in_segment(torch.tensor(seg, dtype=torch.int64),
                              torch.tensor(counts, dtype=torch.int64))
        assert got.tolist() == want, counts


def test_pairwise_sq_l2_within_float32_bound():
    """|a|^2 + |b|^2 - 2ab in float32 against the difference form in
    float64. Each of the three sums has d terms of magnitude at most
    S = max |row|^2, so its error is at most d*u*S (u = 2^-24, any summation
    order); the dot enters doubled; the two remaining additions round
    results of at most 2S and 4S. Total (4d + 6)*u*S, taken as 4d + 8."""
    g = torch.Generator()
    g.manual_seed(12)
    for B, m, d, scale in [(3, 17, 13, 50.0), (1, 1, 5, 1.0), (2, 33, 100, 127.0)]:
        a = (torch.rand((B, m, d), generator=g) - 0.5) * 2 * scale
        got = _pairwise_sq_l2(a).numpy().astype(np.float64)
        a64 = a.numpy().astype(np.float64)
        want = ((a64[:, :, None, :] - a64[:, None, :, :]) ** 2).sum(-1)
        S = (a64 ** 2).sum(-1).max()
        bound = (4 * d + 8) * 2.0 ** -24 * S
        err = np.abs(got - want).max()
        print(f"B={B} m={m} d={d}: max error {err:.3g}, bound {bound:.3g}")
        assert got.shape == (B, m, m) and err <= bound


def test_kdt_tree_with_duplicate_rows():
    """Identical rows cannot be split at a mean: those segments are split by
    rank, also below the first level, where fewer than n members are open."""
    g = torch.Generator()
    g.manual_seed(13)
    x = torch.rand((150, 6), generator=g).numpy().repeat(3, axis=0)
    ts, nodes = build_kdt_tree(x, device="cpu")
    seen, stack = [], [0]
    while stack:
        nd = stack.pop()
        if nd >= 0:
            stack += [int(nodes[nd, 0]), int(nodes[nd, 1])]
        elif -nd - 1 < len(x):
            seen.append(-nd - 1)
    assert sorted(seen) == list(range(len(x)))


@pytest.mark.parametrize("algo,kw", [("BKT", {"refine_rounds": 1}),
                                     ("KDT", {"kdt_trees": 2})])
def test_same_seed_same_index(algo, kw):
    """The benchmark caches a built index under a key of the builder's
    arguments and source, so the same arguments must give the same arrays.
    One thread: with more, the reverse-edge scatter of refine_graph lets
    colliding writes race, and float sums change with the thread count."""
    x = np.random.default_rng(14).standard_normal((3000, 24)).astype(np.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        a, b = (build_index_arrays(x, "L2", algo=algo, device="cpu", ntrees=2,
                                   tpt_leaf=100, cand=64, **kw)
                for _ in range(2))
    finally:
        torch.set_num_threads(threads)
    for k in ("vectors", "tree_start", "tree_nodes", "graph"):
        assert a[k].dtype == b[k].dtype
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_kdt_constructors_check_the_dtype_as_bkt_ones_do():
    """The KDT array constructors share the BKT ones' bodies: the GPU
    binding refuses anything but float32 and int8 vectors for both; the
    oracle has no such check and labels float64 as int8 for both."""
    from oracle.pyoracle import OrcIndex
    from sptag_amd import AnnIndex
    x = np.random.default_rng(15).standard_normal((40, 8)).astype(np.float32)
    ts, kn = build_kdt_tree(x, device="cpu")
    graph = np.full((40, 4), -1, dtype=np.int32)
    bkt = (np.zeros(1, dtype=np.int32), np.full((2, 3), -1, dtype=np.int32))
    for mk, tree in ((AnnIndex.FromArraysKDT, (ts, kn)),
                     (AnnIndex.FromArrays, bkt)):
        with pytest.raises(ValueError):
            mk(x.astype(np.float64), *tree, graph, "L2")
    for mk, tree in ((OrcIndex.from_arrays_kdt, (ts, kn)),
                     (OrcIndex.from_arrays, bkt)):
        ix = mk(x.astype(np.float64), *tree, graph, "L2")
        assert (ix.n, ix.dim, ix.valuetype) == (40, 8, 1)
        assert mk(x, *tree, graph, "L2").valuetype == 0
