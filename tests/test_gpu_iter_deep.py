"""Iterator parity beyond the first five Next(8) calls of the two iterator
goldens: fixtures without an iterator golden, deletes, a batch size that
changes between calls, a non-default MaxCheck, exhaustion and visited-table
saturation. The reference is one OrcIter per query; the CPU siblings check
that the oracle really reaches the branch a case is named for."""
import numpy as np
import pytest

from conftest import load_golden
from oracle.pyoracle import OrcIndex
from parity_util import (assert_iter_calls_equal, built_case, golden_dtype,
                         gpu_from_case, orc_from_case, orc_iter_next,
                         orc_iter_open, orc_iter_run, read_index_arrays)

NQ = 16
NO_ITER_GOLDEN = ["f32_l2_dups", "f32_cos_n10k_d48", "i8_cos_deg48",
                  "f32_l2_bkt2trees"]
_ref = {}


def _golden_ref(name, max_check, batches, nq=NQ):
    """Oracle answers for the first nq golden queries; computed once."""
    key = (name, max_check, tuple(batches), nq)
    if key not in _ref:
        g = load_golden(name)
        oix = OrcIndex.load(g["index"])
        _ref[key] = orc_iter_run(oix, g["queries"][:nq], max_check, batches)
    return _ref[key]


def _stream(calls, i):
    return np.concatenate([v[i, :cnt[i]] for v, _, cnt, _ in calls])


# ---- fixtures without an iterator golden --------------------------------

def test_oracle_dups_stream_returns_duplicates():
    """The duplicate chain (checkNode < -1) is only entered if duplicates
    come out of the stream as separate results: every query must return an
    id whose vector equals that of an id returned earlier."""
    g = load_golden("f32_l2_dups")
    vec = read_index_arrays(g["index"], np.float32)[0]
    calls = _golden_ref("f32_l2_dups", 8192, [8] * 5)
    for i in range(NQ):
        ids = _stream(calls, i)
        assert len(ids) == 40 and len(set(ids.tolist())) == 40
        rows = vec[ids]
        dup = [(rows[j] == rows[:j]).all(1).any() for j in range(1, len(ids))]
        assert any(dup), f"query {i}: no duplicate vector in the stream"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NO_ITER_GOLDEN)
def test_gpu_iter_fixtures_without_golden(name):
    from sptag_amd import AnnIndex
    g = load_golden(name)
    ref = _golden_ref(name, 8192, [8] * 5)
    it = AnnIndex.Load(g["index"]).Iterate(g["queries"][:NQ], max_check=8192)
    assert_iter_calls_equal(it, ref, [8] * 5, name)
    it.Close()


# ---- deletes ------------------------------------------------------------

def _deleted_case():
    if "del" not in _ref:
        g = load_golden("f32_l2_n10k_d32")
        arrs = read_index_arrays(g["index"], np.float32)
        deleted = (np.random.default_rng(11).random(arrs[0].shape[0]) < 0.05
                   ).astype(np.uint8)
        oix = OrcIndex.from_arrays(*arrs, "L2", deleted=deleted)
        q = g["queries"][:NQ]
        _ref["del"] = (arrs, deleted, q, orc_iter_run(oix, q, 8192, [8] * 5))
    return _ref["del"]


def test_oracle_iter_skips_deleted():
    arrs, deleted, q, calls = _deleted_case()
    dels = np.where(deleted)[0]
    assert 300 < len(dels) < 700
    plain = _golden_ref("f32_l2_n10k_d32", 8192, [8] * 5)
    changed = 0
    for i in range(NQ):
        ids = _stream(calls, i)
        assert not np.isin(ids, dels).any()
        changed += int(np.isin(_stream(plain, i), dels).any())
    # the mask must matter: some query's undeleted stream holds a deleted id
    assert changed > 0


@pytest.mark.gpu
def test_gpu_iter_with_deletes():
    from sptag_amd import AnnIndex
    arrs, deleted, q, calls = _deleted_case()
    it = AnnIndex.FromArrays(*arrs, "L2", deleted=deleted).Iterate(
        q, max_check=8192)
    dels = np.where(deleted)[0]
    for c, (rv, rd, rcnt, rrel) in enumerate(calls):
        gv, gd, gcnt, grel = it.Next(8)
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=f"call {c}")
        np.testing.assert_array_equal(grel, rrel, err_msg=f"call {c}")
        assert not np.isin(gv[gv >= 0], dels).any()
        for i in range(NQ):
            np.testing.assert_array_equal(gv[i, :rcnt[i]], rv[i, :rcnt[i]])
            np.testing.assert_array_equal(gd[i, :rcnt[i]], rd[i, :rcnt[i]])
    it.Close()


# ---- changing batch -----------------------------------------------------

CHANGING = [1, 8, 3, 64, 2, 256]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32_l2_n10k_d32", "i8_l2_n10k_d100"])
def test_gpu_iter_changing_batch(name):
    """The output buffers grow at 8, 64 and 256, and every call has its own
    LDS layout; the stream must not notice."""
    from sptag_amd import AnnIndex
    g = load_golden(name)
    ref = _golden_ref(name, 8192, CHANGING)
    it = AnnIndex.Load(g["index"]).Iterate(g["queries"][:NQ], max_check=8192)
    assert_iter_calls_equal(it, ref, CHANGING, name)
    it.Close()


# ---- non-default MaxCheck -----------------------------------------------

MC512_PLAIN = [16] * 10
# Next(16) alone cannot raise the flag at MaxCheck 512: measured on the
# oracle, one such call checks 186..452 vectors per query, never more than
# 512, and the flag stays 0 for all 16 queries through 80 calls (by call 20
# more than 4096 ids are visited, which the GPU's table at this MaxCheck
# cannot hold). A Next(64) call checks 760..1419 > 512, so the sequence
# below shows the flag at 0 after the first call and at 1 after the second.
MC512_FLIP = [16, 64, 64]


def test_oracle_relaxed_flag_flips_at_mc512():
    calls = _golden_ref("f32_l2_n10k_d32", 512, MC512_FLIP)
    rel = np.stack([c[3] for c in calls])            # [call, query]
    flips = ((rel[:-1] == 0) & (rel[1:] == 1)).any(axis=0)
    assert flips.any(), "relaxed flag never went 0 -> 1"
    assert (np.diff(rel, axis=0) >= 0).all(), "the flag is sticky"
    # and the plain sequence is the quiet case described above
    plain = _golden_ref("f32_l2_n10k_d32", 512, MC512_PLAIN)
    assert all((c[3] == 0).all() for c in plain)
    assert all((c[2] == 16).all() for c in plain)


@pytest.mark.gpu
@pytest.mark.parametrize("batches", [MC512_PLAIN, MC512_FLIP],
                         ids=["ten_next16", "flag_flips"])
def test_gpu_iter_maxcheck_512(batches):
    from sptag_amd import AnnIndex
    g = load_golden("f32_l2_n10k_d32")
    ref = _golden_ref("f32_l2_n10k_d32", 512, batches)
    it = AnnIndex.Load(g["index"]).Iterate(g["queries"][:NQ], max_check=512)
    assert_iter_calls_equal(it, ref, batches, "mc512")
    it.Close()


# ---- exhaustion ---------------------------------------------------------

def _exhaust(oix, q, max_check, batch, extra=2, limit=5000):
    """Next(batch) until some call is short for every query, then `extra`
    more calls. Returns the list of calls."""
    its = orc_iter_open(oix, q, max_check)
    calls, after = [], None
    while after is None or after < extra:
        calls.append(orc_iter_next(its, batch))
        if after is not None:
            after += 1
        elif (calls[-1][2] < batch).all():
            after = 0
        assert len(calls) < limit
    return calls


def _exhaust_case():
    if "exh" not in _ref:
        c = built_case(300, 16, "f32", "L2")
        _ref["exh"] = (c, _exhaust(orc_from_case(c), c["q"], 8192, 8))
    return _ref["exh"]


def test_oracle_iter_exhausts_to_a_permutation():
    c, calls = _exhaust_case()
    assert len(calls) == 40       # 37 full calls, 4 ids, then nothing twice
    for i in range(len(c["q"])):
        ids = _stream(calls, i)
        assert sorted(ids.tolist()) == list(range(300))
        for v, d, cnt, _ in calls:
            assert (np.diff(d[i, :cnt[i]]) >= 0).all()
    for _, _, cnt, _ in calls[-2:]:
        assert (cnt == 0).all()


@pytest.mark.gpu
def test_gpu_iter_exhaustion():
    c, calls = _exhaust_case()
    it = gpu_from_case(c).Iterate(c["q"], max_check=8192)
    got = [[] for _ in c["q"]]
    for n, (rv, rd, rcnt, rrel) in enumerate(calls):
        gv, gd, gcnt, grel = it.Next(8)
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=f"call {n}")
        np.testing.assert_array_equal(grel, rrel, err_msg=f"call {n}")
        for i in range(len(got)):
            np.testing.assert_array_equal(gv[i, :rcnt[i]], rv[i, :rcnt[i]])
            np.testing.assert_array_equal(gd[i, :rcnt[i]], rd[i, :rcnt[i]])
            got[i].extend(gv[i, :gcnt[i]].tolist())
    assert (gcnt == 0).all()
    for ids in got:
        assert sorted(ids) == list(range(300))
    it.Close()


# ---- visited-table saturation -------------------------------------------

SAT_N, SAT_MC, SAT_VCAP = 6000, 256, 4096


def _saturation_case():
    if "sat" not in _ref:
        c = built_case(SAT_N, 16, "f32", "L2", nq=2)
        _ref["sat"] = (c, _exhaust(orc_from_case(c), c["q"], SAT_MC, 8, extra=0))
    return _ref["sat"]


def test_oracle_iter_runs_past_maxcheck_to_exhaustion():
    """The reference iterator has no stop at MaxCheck: at MaxCheck 256 it
    still returns every one of the 6000 ids once."""
    c, calls = _saturation_case()
    for i in range(2):
        assert sorted(_stream(calls, i).tolist()) == list(range(SAT_N))


@pytest.mark.gpu
def test_gpu_iter_saturation_is_an_error(capfd):
    """The iterator's visited table holds next_pow2(max(4096, 4*256)) = 4096
    ids and the index 6000, so the stream cannot reach exhaustion. Required
    behaviour: every call matches the oracle until the call in which the
    table saturates, and that call raises (ERR_INTERNAL) with a stderr line
    naming the saturation. A short count while the oracle still has results
    must never be returned."""
    import time
    from sptag_amd import SptagAmdError
    c, calls = _saturation_case()
    it = gpu_from_case(c).Iterate(c["q"], max_check=SAT_MC)
    capfd.readouterr()
    t0 = time.time()
    raised_at = None
    for n, (rv, rd, rcnt, rrel) in enumerate(calls):
        try:
            gv, gd, gcnt, grel = it.Next(8)
        except SptagAmdError as e:
            assert e.code == -6
            raised_at = n
            break
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=f"call {n} counts")
        np.testing.assert_array_equal(grel, rrel, err_msg=f"call {n} relaxed")
        for i in range(2):
            np.testing.assert_array_equal(gv[i, :rcnt[i]], rv[i, :rcnt[i]])
            np.testing.assert_array_equal(gd[i, :rcnt[i]], rd[i, :rcnt[i]])
    print(f"saturation: raised at call {raised_at} of {len(calls)}, "
          f"{time.time() - t0:.2f} s")
    # every returned id sits in the table: 4096 slots end the stream by
    # call 512 at the latest, long before the oracle's last full call
    assert raised_at is not None and raised_at <= SAT_VCAP // 8
    assert (calls[raised_at][2] == 8).all()
    assert "visited-table saturation" in capfd.readouterr().err
    with pytest.raises(SptagAmdError):      # sticky
        it.Next(8)
    it.Close()
