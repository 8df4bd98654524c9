"""Shard sets on the GPU: the merge kernel alone on synthetic lists, and
ShardedIndex search / truth against the oracle. The answer of a shard set is
defined as the (dist, global vid) merge of the per-shard answers, so the
expected result is always built the same way in numpy: map vid to global
id, drop padding, np.lexsort((gvid, dist)), cut to k, pad with -1 / MaxDist.
Every comparison is bit for bit: ids, and distances viewed as uint32."""
import numpy as np
import pytest

from sptag_amd import AnnIndex, ShardedIndex, merge_topk
from parity_util import MAXDIST, built_case, gpu_from_case, orc_from_case

pytestmark = pytest.mark.gpu


def ref_merge(vids, dists, base, k_out, paddist=MAXDIST):
    """vids/dists [S, nq, k_in] -> (vids [nq, k_out], dists [nq, k_out])."""
    base = np.asarray(base, dtype=np.int64)
    nq = vids.shape[1]
    out_v = np.full((nq, k_out), -1, dtype=np.int32)
    out_d = np.full((nq, k_out), paddist, dtype=np.float32)
    for q in range(nq):
        real = vids[:, q, :] >= 0
        g = (vids[:, q, :] + base[:, None])[real]
        d = dists[:, q, :][real]
        order = np.lexsort((g, d))[:k_out]
        out_v[q, :len(order)] = g[order]
        out_d[q, :len(order)] = d[order]
    return out_v, out_d


def assert_bits_equal(gv, gd, ev, ed, tag=""):
    assert gv.dtype == np.int32 and gd.dtype == np.float32
    np.testing.assert_array_equal(gv, ev, err_msg=f"{tag} ids")
    np.testing.assert_array_equal(gd.view(np.uint32), ed.view(np.uint32),
                                  err_msg=f"{tag} distance bits")


# ---------------------------------------------------------------------------
# the merge alone
# ---------------------------------------------------------------------------

# eight distinct values, so ties inside and across shards are the rule;
# 0.0 and -0.0 compare equal and must keep their own bits
DVALS = np.array([-0.0, 0.0, -3.0, 0.25, 1.0,
                  np.nextafter(np.float32(1), np.float32(2)), 7.5, 1e20],
                 dtype=np.float32)
assert len(set(DVALS.view(np.uint32).tolist())) == 8
NLOCAL = 5000      # local ids are drawn below this; bases are multiples of it

SHAPES = [        # (S, k_in, k_out, nq)
    (1, 10, 10, 3),        # identity plus base offset
    (2, 1, 1, 1),          # smallest non-trivial merge
    (3, 10, 10, 5),        # small plain case
    (8, 10, 10, 65),       # more queries than one wave of anything
    (2, 64, 64, 4),        # either side of the wave width
    (2, 65, 65, 4),
    (3, 200, 200, 2),      # larger k
    (4, 1024, 1024, 2),    # last shape staged in LDS: 4096 entries
    (5, 1024, 1024, 2),    # first shape served from global memory
    (64, 4, 16, 2),        # widest fan-in
    (2, 10, 30, 2),        # k_out > S*k_in: the tail is padding
    (4, 10, 3, 2),         # k_out < k_in
]


def synth_lists(S, k_in, nq, fill, seed, paddist=MAXDIST):
    """Seeded per-shard lists, each ascending (dist, vid) with a padding
    suffix. `fill(s, q, rng)` gives the number of real entries of list s of
    query q. The bases are a permutation of multiples of NLOCAL, so the
    global-id order of tied entries is not the shard order."""
    rng = np.random.default_rng(seed)
    vids = np.full((S, nq, k_in), -1, dtype=np.int32)
    dists = np.full((S, nq, k_in), paddist, dtype=np.float32)
    for s in range(S):
        for q in range(nq):
            n = fill(s, q, rng)
            v = rng.choice(NLOCAL, n, replace=False).astype(np.int32)
            d = DVALS[rng.integers(0, len(DVALS), n)]
            order = np.lexsort((v, d))
            vids[s, q, :n] = v[order]
            dists[s, q, :n] = d[order]
    base = (rng.permutation(S) * NLOCAL).astype(np.int32)
    return vids, dists, base


def check_merge(S, k_in, k_out, nq, fill, seed, paddist=MAXDIST, out_pad=None):
    vids, dists, base = synth_lists(S, k_in, nq, fill, seed, paddist)
    ev, ed = ref_merge(vids, dists, base, k_out,
                       paddist if out_pad is None else out_pad)
    gv, gd = merge_topk(vids, dists, base, k_out)
    assert_bits_equal(gv, gd, ev, ed, f"S={S} k_in={k_in} k_out={k_out} nq={nq}")
    return gv


@pytest.mark.parametrize("S,k_in,k_out,nq", SHAPES)
def test_merge_full_lists(S, k_in, k_out, nq):
    gv = check_merge(S, k_in, k_out, nq, lambda s, q, rng: k_in, seed=S * 7919 + k_in)
    assert ((gv >= 0).sum(1) == min(k_out, S * k_in)).all()


@pytest.mark.parametrize("S,k_in,k_out,nq", SHAPES)
def test_merge_ragged_lists(S, k_in, k_out, nq):
    """Every list has its own number of real entries, 0 and k_in included."""
    check_merge(S, k_in, k_out, nq,
                lambda s, q, rng: int(rng.integers(0, k_in + 1)),
                seed=S * 104729 + k_in)


PADDING_CASES = {
    # one list entirely padding
    "one_list_empty": lambda k: (lambda s, q, rng: 0 if s == 1 else k),
    # one list padded from position 0 in some queries and full in others
    "one_list_empty_or_full": lambda k: (lambda s, q, rng: k if s or q % 2 else 0),
    # all lists padding
    "all_empty": lambda k: (lambda s, q, rng: 0),
}


@pytest.mark.parametrize("case", sorted(PADDING_CASES))
@pytest.mark.parametrize("S,k_in,k_out,nq",
                         [(3, 10, 10, 5), (2, 65, 65, 4), (5, 1024, 1024, 2)])
def test_merge_padding_cases(S, k_in, k_out, nq, case):
    gv = check_merge(S, k_in, k_out, nq, PADDING_CASES[case](k_in), seed=4242 + S)
    if case == "all_empty":
        assert (gv == -1).all()


def test_merge_padding_distance():
    """Padding carries the inputs' own padding distance where they have one,
    and MaxDist (what the single-index search writes) where they have none."""
    pad = np.float32(9e30)
    check_merge(3, 10, 40, 4, lambda s, q, rng: 3 * s, seed=5, paddist=pad)
    check_merge(5, 1024, 1024, 2, lambda s, q, rng: 100 * s, seed=6, paddist=pad)
    # full lists, k_out > S*k_in: no input padding to copy from
    check_merge(2, 10, 30, 2, lambda s, q, rng: 10, seed=7, paddist=pad,
                out_pad=MAXDIST)


# ---------------------------------------------------------------------------
# set search, expected from the oracle
# ---------------------------------------------------------------------------

DIM, NQ, MC = 16, 8, 512
SIZES = [300, 65, 5]        # the 5-vector shard pads at k = 10
TYPES = [("f32", "L2"), ("f32", "Cosine"), ("i8", "Cosine")]
KS = [1, 10, 64]


def oracle_merged(cases, masks, q, k, base=None, max_check=MC):
    """Per-shard OrcIndex.search_batch, merged in numpy."""
    if base is None:
        base = np.concatenate([[0], np.cumsum([c["n"] for c in cases])[:-1]])
    lists = [orc_from_case(c, m).search_batch(q, k, max_check)
             for c, m in zip(cases, masks)]
    return ref_merge(np.stack([v for v, _ in lists]),
                     np.stack([d for _, d in lists]), base, k)


@pytest.mark.parametrize("vt,dm", TYPES)
def test_set_search_three_shards(vt, dm):
    cases = [built_case(n, DIM, vt, dm) for n in SIZES]
    q = cases[0]["q"]
    sh = ShardedIndex.FromIndexes([gpu_from_case(c) for c in cases])
    assert sh.NumShards() == 3 and sh.NumVectors() == sum(SIZES)
    for k in KS:
        ev, ed = oracle_merged(cases, [None] * 3, q, k)
        gv, gd = sh.BatchSearch(q, k, MC)
        assert_bits_equal(gv, gd, ev, ed, f"{vt} {dm} k={k}")
    # explicit bases with room between the shards
    base = np.array([1000, 0, 2 ** 31 - 1 - 5], dtype=np.int32)
    sh2 = ShardedIndex.FromIndexes(sh.shards, vid_base=base)
    ev, ed = oracle_merged(cases, [None] * 3, q, 10, base=base)
    gv, gd = sh2.BatchSearch(q, 10, MC)
    assert_bits_equal(gv, gd, ev, ed, f"{vt} {dm} explicit bases")


@pytest.mark.parametrize("vt,dm", [("f32", "L2"), ("i8", "Cosine")])
def test_set_search_same_case_twice(vt, dm):
    """Two shards built from the same case: every distance ties across the
    shards, and the order is decided by global vid alone."""
    c = built_case(300, DIM, vt, dm)
    sh = ShardedIndex.FromIndexes([gpu_from_case(c), gpu_from_case(c)])
    for k in (10, 64):
        ev, ed = oracle_merged([c, c], [None, None], c["q"], k)
        gv, gd = sh.BatchSearch(c["q"], k, MC)
        assert_bits_equal(gv, gd, ev, ed, f"k={k}")


def test_set_search_bkt_and_kdt_mixed():
    cases = [built_case(300, DIM, "f32", "L2", "BKT"),
             built_case(65, DIM, "f32", "L2", "KDT")]
    q = cases[0]["q"]
    sh = ShardedIndex.FromIndexes([gpu_from_case(c) for c in cases])
    assert [ix.algo for ix in sh.shards] == [0, 1]
    for k in KS:
        ev, ed = oracle_merged(cases, [None, None], q, k)
        gv, gd = sh.BatchSearch(q, k, MC)
        assert_bits_equal(gv, gd, ev, ed, f"k={k}")


def test_set_search_with_delete_mask_and_later_delete():
    cases = [built_case(n, DIM, "f32", "L2") for n in SIZES]
    q = cases[0]["q"]
    mask65 = np.zeros(65, dtype=np.uint8)
    mask65[::3] = 1
    masks = [None, mask65, None]
    shards = [gpu_from_case(c, m) for c, m in zip(cases, masks)]
    sh = ShardedIndex.FromIndexes(shards)
    ev, ed = oracle_merged(cases, masks, q, 10)
    gv, gd = sh.BatchSearch(q, 10, MC)
    assert_bits_equal(gv, gd, ev, ed, "mask at create")
    assert not np.isin(gv, 300 + np.flatnonzero(mask65)).any()

    # Delete on a shard handle: the set's next search sees it. The ids
    # deleted are shard 0's part of the answers just given.
    gone = np.unique(gv[(gv >= 0) & (gv < 300)])
    assert gone.size > 0
    shards[0].Delete(gone)
    mask300 = np.zeros(300, dtype=np.uint8)
    mask300[gone] = 1
    ev2, ed2 = oracle_merged(cases, [mask300, mask65, None], q, 10)
    gv2, gd2 = sh.BatchSearch(q, 10, MC)
    assert_bits_equal(gv2, gd2, ev2, ed2, "after Delete")
    assert not np.isin(gv2, gone).any()
    assert (ev2 != ev).any()


# ---------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------

def _trivial_orc(x, dm):
    """Whole-array oracle index for truth, which reads no tree or graph."""
    from oracle.pyoracle import OrcIndex
    return OrcIndex.from_arrays(x, np.zeros(1, dtype=np.int32),
                                np.zeros((2, 3), dtype=np.int32),
                                np.full((x.shape[0], 2), -1, dtype=np.int32), dm)


@pytest.mark.parametrize("vt", ["f32", "i8"])
def test_set_truth_equals_whole_array_truth(vt):
    from sptag_amd.build import build_index_arrays
    rng = np.random.default_rng(370)
    if vt == "f32":
        x = rng.standard_normal((370, DIM)).astype(np.float32)
        q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    else:
        x = rng.integers(-100, 101, (370, DIM)).astype(np.int8)
        q = rng.integers(-100, 101, (NQ, DIM)).astype(np.int8)
    shards = []
    for lo, hi in [(0, 300), (300, 365), (365, 370)]:
        a = build_index_arrays(x[lo:hi], "L2", algo="BKT", device="cpu",
                               ntrees=2, tpt_leaf=100, cand=64)
        shards.append(AnnIndex.FromArrays(np.ascontiguousarray(a["vectors"]),
                                          a["tree_start"], a["tree_nodes"],
                                          a["graph"], "L2"))
    sh = ShardedIndex.FromIndexes(shards)
    whole = _trivial_orc(x, "L2")
    for k in (1, 10, 373):          # 373 > 370: three entries of padding
        ev, ed = whole.truth(q, k)
        gv, gd = sh.Truth(q, k)
        assert_bits_equal(gv, gd, ev, ed, f"truth k={k}")


# ---------------------------------------------------------------------------
# device pointers, two devices
# ---------------------------------------------------------------------------

def test_set_search_device_pointers():
    import torch
    cases = [built_case(n, DIM, "f32", "L2") for n in SIZES]
    q = cases[0]["q"]
    sh = ShardedIndex.FromIndexes([gpu_from_case(c) for c in cases])
    d_q = torch.from_numpy(np.array(q)).to("cuda:0")
    for k in (10, 64):
        hv, hd = sh.BatchSearch(q, k, MC)
        d_v = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda:0")
        d_d = torch.full((NQ, k), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        sh.BatchSearchDevice(d_q.data_ptr(), NQ, k, d_v.data_ptr(),
                             d_d.data_ptr(), MC)
        assert_bits_equal(d_v.cpu().numpy(), d_d.cpu().numpy(), hv, hd, f"k={k}")


def test_set_search_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    cases = [built_case(n, DIM, "f32", "L2") for n in SIZES]
    q = cases[0]["q"]
    one = ShardedIndex.FromIndexes([gpu_from_case(c) for c in cases])
    two = ShardedIndex.FromIndexes([AnnIndex.FromArrays(*c["args"], device=d)
                                    for c, d in zip(cases, (0, 1, 0))])
    for k in KS:
        ev, ed = one.BatchSearch(q, k, MC)
        gv, gd = two.BatchSearch(q, k, MC)
        assert_bits_equal(gv, gd, ev, ed, f"k={k}")
    ev, ed = one.Truth(q, 10)
    gv, gd = two.Truth(q, 10)
    assert_bits_equal(gv, gd, ev, ed, "truth")
