#!/usr/bin/env python3
"""Generate golden parity fixtures under tests/golden/ using the REFERENCE
binaries in oracle/_ref (compiled from /root/reference by oracle/Makefile).

Run in the dev container (where /root/reference exists):
    python3 oracle/gen_golden.py

For each fixture we commit:
  index/            the reference-built index folder (vectors/tree/graph/
                    deletes + indexloader.ini) — build is NOT deterministic
                    (SURVEY.md §8c), so golden answers are pinned to this
                    saved index, never to a rebuild.
  queries.bin       queries in DEFAULT format [int32 n][int32 dim][data]
  results_mc{M}.bin reference indexsearcher output, binary format
                    [int32 nq][int32 K] + nq*K*{int32 vid, float dist}
                    (reference src/IndexSearcher/main.cpp:314-331)
  meta.json         shapes/types/maxchecks

Fixture search results verified byte-stable across runs and thread counts
(SURVEY.md §8c), so they are exact golden answers for any backend that
claims bit-parity.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(HERE, "_ref")
GOLDEN = os.path.join(REPO, "tests", "golden")

K = 10
MAXCHECKS = [512, 2048, 8192]


def write_default(path, arr):
    """DEFAULT file format: [int32 rows][int32 cols][row-major data]
    (reference Dataset.h:146 / Helper VectorSetReaders/DefaultReader)."""
    with open(path, "wb") as f:
        f.write(np.int32(arr.shape[0]).tobytes())
        f.write(np.int32(arr.shape[1]).tobytes())
        f.write(arr.tobytes())


def run(cmd):
    print("+", " ".join(cmd))
    subprocess.run(cmd, check=True, cwd=REPO)


def gen_fixture(name, data, queries, vtype, dist, maxchecks=MAXCHECKS, k=K,
                algo="BKT"):
    d = os.path.join(GOLDEN, name)
    idx = os.path.join(d, "index")
    os.makedirs(d, exist_ok=True)
    write_default(os.path.join(d, "data.bin"), data)
    write_default(os.path.join(d, "queries.bin"), queries)

    run([os.path.join(REF, "indexbuilder"),
         "-d", str(data.shape[1]), "-v", vtype, "-f", "DEFAULT",
         "-i", os.path.join(d, "data.bin"), "-o", idx, "-a", algo,
         "-t", "4",
         "Index.DistCalcMethod=" + dist])

    for mc in maxchecks:
        run([os.path.join(REF, "indexsearcher"),
             "-d", str(data.shape[1]), "-v", vtype, "-f", "DEFAULT",
             "-i", os.path.join(d, "queries.bin"), "-x", idx,
             "-k", str(k), "-m", str(mc), "-t", "2", "-of", "1",
             "-o", os.path.join(d, f"results_mc{mc}.bin")])

    # data.bin duplicates index/vectors.bin content (normalized for cosine);
    # keep queries only + the index folder to stay small.
    os.remove(os.path.join(d, "data.bin"))
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"n": int(data.shape[0]), "dim": int(data.shape[1]),
                   "valuetype": vtype, "distmethod": dist, "k": k, "algo": algo,
                   "maxchecks": maxchecks, "nq": int(queries.shape[0])}, f)
    print(f"fixture {name} done")


def gen_fixture_ex(name, data, queries, vtype, dist, maxchecks, algo="BKT",
                   k=K, extra=()):
    """gen_fixture with extra builder parameters (Section.Name=Value argv,
    reference IndexSearcher/IndexBuilder main.cpp:362-389)."""
    d = os.path.join(GOLDEN, name)
    idx = os.path.join(d, "index")
    os.makedirs(d, exist_ok=True)
    write_default(os.path.join(d, "data.bin"), data)
    write_default(os.path.join(d, "queries.bin"), queries)
    run([os.path.join(REF, "indexbuilder"), "-d", str(data.shape[1]),
         "-v", vtype, "-f", "DEFAULT", "-i", os.path.join(d, "data.bin"),
         "-o", idx, "-a", algo, "-t", "4",
         "Index.DistCalcMethod=" + dist, *extra])
    for mc in maxchecks:
        run([os.path.join(REF, "indexsearcher"), "-d", str(data.shape[1]),
             "-v", vtype, "-f", "DEFAULT", "-i", os.path.join(d, "queries.bin"),
             "-x", idx, "-k", str(k), "-m", str(mc), "-t", "2", "-of", "1",
             "-o", os.path.join(d, f"results_mc{mc}.bin")])
    os.remove(os.path.join(d, "data.bin"))
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"n": int(data.shape[0]), "dim": int(data.shape[1]),
                   "valuetype": vtype, "distmethod": dist, "k": k, "algo": algo,
                   "maxchecks": maxchecks, "nq": int(queries.shape[0])}, f)
    print(f"fixture {name} done")


def gen_iter_and_add_goldens():
    """Iterative-search and online-add golden answers, produced by driving
    the reference's OWN ResultIterator / AddIndex (iterprobe / addprobe
    harnesses linked against the oracle/_ref objects)."""
    rng = np.random.default_rng(555)
    for name in ["f32_l2_n10k_d32", "i8_l2_n10k_d100"]:
        d = os.path.join(GOLDEN, name)
        meta = json.load(open(os.path.join(d, "meta.json")))
        run([os.path.join(REF, "iterprobe"), os.path.join(d, "index"),
             os.path.join(d, "queries.bin"), "8", "5",
             os.path.join(d, "iter_b8_c5.bin")])
        dim = meta["dim"]
        if meta["valuetype"] == "Float":
            add = (rng.random((64, dim), dtype=np.float32) * 100).astype(np.float32)
        else:
            add = rng.integers(-100, 101, (64, dim)).astype(np.int8)
        write_default(os.path.join(d, "add_vectors.bin"), add)
        out = os.path.join("/tmp", "postadd_" + name)
        run([os.path.join(REF, "addprobe"), os.path.join(d, "index"),
             os.path.join(d, "add_vectors.bin"), out])
        import shutil
        shutil.copy(os.path.join(out, "graph.bin"),
                    os.path.join(d, "postadd_graph.bin"))
    gen_cosine_add_goldens()


COSINE_ADD = ["f32_cos_n10k_d48", "i8_cos_deg48"]
NADD_COSINE = 16


def read_default(path, dtype):
    with open(path, "rb") as f:
        n, dim = np.frombuffer(f.read(8), dtype=np.int32)
        return np.frombuffer(f.read(), dtype=dtype).reshape(n, dim)


def gen_cosine_add_goldens():
    """Post-add state of the reference's own AddIndex on the cosine fixtures:
    16 un-normalised vectors go in, the reference normalises them itself.
    A whole post-add graph is larger than a committed file may be, so only
    what the add changed is kept:
      add16_vectors.bin      the 16 vectors as given to AddIndex
      postadd16_vectors.bin  the last 16 rows of the saved vectors.bin,
                             i.e. the reference's normalised form
      postadd16_rows.bin     [int32 n_after][int32 degree][int32 nrows], then
                             nrows * {int32 row id, int32 row[degree]}: every
                             row of the saved graph.bin that is new or differs
                             from index/graph.bin, in id order
    The fixture's index folder is only read. Also reachable on its own as
    `gen_golden.py cosine-add`, since main() would rebuild every index."""
    import tempfile
    for name in COSINE_ADD:
        d = os.path.join(GOLDEN, name)
        meta = json.load(open(os.path.join(d, "meta.json")))
        dim = meta["dim"]
        rng = np.random.default_rng(9000 + dim)
        if meta["valuetype"] == "Float":
            dtype = np.float32
            add = (rng.standard_normal((NADD_COSINE, dim)) * 3).astype(np.float32)
        else:
            dtype = np.int8
            add = rng.integers(-100, 101, (NADD_COSINE, dim)).astype(np.int8)
        write_default(os.path.join(d, "add16_vectors.bin"), add)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "postadd")
            run([os.path.join(REF, "addprobe"), os.path.join(d, "index"),
                 os.path.join(d, "add16_vectors.bin"), out])
            before = read_default(os.path.join(d, "index", "graph.bin"), np.int32)
            after = read_default(os.path.join(out, "graph.bin"), np.int32)
            vec = read_default(os.path.join(out, "vectors.bin"), dtype)
        n0, deg = before.shape
        assert after.shape == (n0 + NADD_COSINE, deg) and vec.shape[0] == after.shape[0]
        changed = np.where((after[:n0] != before).any(axis=1))[0]
        rows = np.concatenate([changed, np.arange(n0, n0 + NADD_COSINE)]).astype(np.int32)
        write_default(os.path.join(d, "postadd16_vectors.bin"), vec[n0:])
        with open(os.path.join(d, "postadd16_rows.bin"), "wb") as f:
            f.write(np.array([after.shape[0], deg, len(rows)], dtype=np.int32).tobytes())
            f.write(np.column_stack([rows, after[rows]]).astype(np.int32).tobytes())
        print(f"cosine add golden {name}: {len(changed)} old rows changed")


# Distance pairs: every generic-form tail below 144, then the fixed-dim forms,
# their neighbours and MAX_DIM; int8 up to 260, the largest admitted dim.
DIST_DIMS_F32 = list(range(1, 145)) + [160, 192, 255, 256, 257, 384, 512, 513,
                                       768, 1024, 4096]
DIST_DIMS_I8 = list(range(1, 145)) + [160, 192, 255, 256, 257, 258, 259, 260]
DIST_PPD = 3
DIST_SEED_F32 = 20240
DIST_SEED_I8 = 20241


def dist_pairs_f32(dims=DIST_DIMS_F32, seed=DIST_SEED_F32):
    """Per dim three (x, y) pairs: standard normal; magnitudes spread over
    six decades, so that the fold order changes the rounded sum; both unit
    length, the cosine case."""
    rng = np.random.default_rng(seed)
    out = []
    for d in dims:
        p = rng.standard_normal((2, d))
        s = rng.standard_normal((2, d)) * 10.0 ** rng.uniform(-3, 3, (2, d))
        u = rng.standard_normal((2, d))
        u = u.astype(np.float32)
        u = u / np.linalg.norm(u.astype(np.float64), axis=1, keepdims=True)
        out.append(np.stack([p, s, u]).astype(np.float32))   # [3, 2, d]
    return out


def dist_pairs_i8(dims=DIST_DIMS_I8, seed=DIST_SEED_I8):
    """Per dim three pairs: uniform over the whole range; all -128 against
    all 127, the largest distance there is; the same with the last 126."""
    rng = np.random.default_rng(seed)
    out = []
    for d in dims:
        p = rng.integers(-128, 128, (2, d))
        e = np.stack([np.full(d, -128), np.full(d, 127)])
        f = e.copy()
        f[1, -1] = 126
        out.append(np.stack([p, e, f]).astype(np.int8))
    return out


def write_dist_pairs(path, vt, dims, pairs):
    with open(path, "wb") as f:
        f.write(np.array([vt, len(dims), DIST_PPD] + list(dims),
                         dtype=np.int32).tobytes())
        for a in pairs:
            f.write(np.ascontiguousarray(a).tobytes())


def gen_dist_goldens():
    """The reference's own ComputeDistance on seeded pairs at every dim
    form (distprobe). Plain files directly under tests/golden/:
      dist_pairs_{f32,i8}.bin  the pairs, in distprobe's input format
      dist_ref_{f32,i8}.bin    float32 [ndims * ppd][2]: L2, Cosine
      dist_pairs.json          dims, pairs per dim, seeds, instruction set
    Reachable on its own as `gen_golden.py dist`; no index is rebuilt."""
    meta = {"pairs_per_dim": DIST_PPD, "metrics": ["L2", "Cosine"]}
    isets = set()
    for tag, vt, dims, seed, mk in [
            ("f32", 0, DIST_DIMS_F32, DIST_SEED_F32, dist_pairs_f32),
            ("i8", 1, DIST_DIMS_I8, DIST_SEED_I8, dist_pairs_i8)]:
        src = os.path.join(GOLDEN, f"dist_pairs_{tag}.bin")
        dst = os.path.join(GOLDEN, f"dist_ref_{tag}.bin")
        write_dist_pairs(src, vt, dims, mk())
        cmd = [os.path.join(REF, "distprobe"), src, dst]
        print("+", " ".join(cmd))
        out = subprocess.run(cmd, check=True, cwd=REPO, capture_output=True,
                             text=True).stdout
        iset = out.split("instruction_set", 1)[1].split()[0]
        print(out.strip())
        isets.add(iset)
        assert os.path.getsize(dst) == len(dims) * DIST_PPD * 8
        meta[tag] = {"dims": list(dims), "seed": seed}
    # the oracle restates the AVX512 order; values of another path would pin
    # the wrong thing
    if isets != {"AVX512"}:
        for tag in ("f32", "i8"):
            os.remove(os.path.join(GOLDEN, f"dist_ref_{tag}.bin"))
            os.remove(os.path.join(GOLDEN, f"dist_pairs_{tag}.bin"))
        sys.exit(f"reference took {sorted(isets)}, not AVX512: no fixture written")
    meta["instruction_set"] = "AVX512"
    with open(os.path.join(GOLDEN, "dist_pairs.json"), "w") as f:
        json.dump(meta, f)
    print("distance pairs done")


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    rng = np.random.default_rng(2016)

    # 1. f32 L2, uniform — the basic float case (BASELINE config #1 shape, small)
    data = rng.random((10000, 32), dtype=np.float32)
    queries = rng.random((100, 32), dtype=np.float32)
    gen_fixture("f32_l2_n10k_d32", data, queries, "Float", "L2")

    # 2. int8 cosine, SPACEV-shaped (config #3, small). Builder normalizes
    #    base vectors to norm 127 in place (BKTIndex.cpp:749-756).
    data = rng.integers(-100, 101, (20000, 100)).astype(np.int8)
    queries = rng.integers(-100, 101, (200, 100)).astype(np.int8)
    gen_fixture("i8_cos_n20k_d100", data, queries, "Int8", "Cosine")

    # 3. int8 L2 (config #5 dtype/metric, small): integer distances — the
    #    identical-top-k-IDs parity case.
    data = rng.integers(-100, 101, (10000, 100)).astype(np.int8)
    queries = rng.integers(-100, 101, (100, 100)).astype(np.int8)
    gen_fixture("i8_l2_n10k_d100", data, queries, "Int8", "L2")

    # 4. AlgoTest-style deterministic grid (reference Test/src/AlgoTest.cpp:161:
    #    vector i = (i,i,...,i), query j = (2j,...)): heavy distance ties and
    #    duplicate-free but collapse-prone clusters; known answers.
    n, dim = 2000, 10
    data = np.tile(np.arange(n, dtype=np.float32)[:, None], (1, dim))
    queries = np.tile((np.arange(100, dtype=np.float32) * 2)[:, None], (1, dim))
    gen_fixture("f32_l2_grid_ties", data, queries, "Float", "L2",
                maxchecks=[512, 2048], k=3)

    # 5. duplicate vectors — exercises the collapsed-center duplicate chain
    #    (BKTIndex.cpp:292-312, BKTree.h:598-608): 2000 base vectors, each
    #    repeated 4x.
    base = rng.random((2000, 16), dtype=np.float32)
    data = np.repeat(base, 4, axis=0)
    perm = rng.permutation(len(data))
    data = data[perm]
    queries = rng.random((100, 16), dtype=np.float32)
    gen_fixture("f32_l2_dups", data, queries, "Float", "L2",
                maxchecks=[512, 2048], k=10)

    # 7. KDT fixtures (config #4 algo): same traversal machinery, kd-tree
    #    seeds + no-better-propagation termination (KDTIndex.cpp:184-241)
    data = rng.standard_normal((10000, 64)).astype(np.float32)
    queries = rng.standard_normal((100, 64)).astype(np.float32)
    gen_fixture("kdt_f32_cos_n10k_d64", data, queries, "Float", "Cosine",
                maxchecks=[512, 2048, 8192], algo="KDT")
    data = rng.random((10000, 32), dtype=np.float32)
    queries = rng.random((100, 32), dtype=np.float32)
    gen_fixture("kdt_f32_l2_n10k_d32", data, queries, "Float", "L2",
                maxchecks=[512, 2048, 8192], algo="KDT")
    data = rng.integers(-100, 101, (10000, 100)).astype(np.int8)
    queries = rng.integers(-100, 101, (100, 100)).astype(np.int8)
    gen_fixture("kdt_i8_l2_n10k_d100", data, queries, "Int8", "L2",
                maxchecks=[2048, 8192], algo="KDT")

    # 6. f32 cosine (config #4 metric; KDT later — BKT for now), normalized
    #    gaussian rows, d=48 not a multiple of 16 to cover distance tails.
    data = rng.standard_normal((10000, 48)).astype(np.float32)
    queries = rng.standard_normal((100, 48)).astype(np.float32)
    gen_fixture("f32_cos_n10k_d48", data, queries, "Float", "Cosine",
                maxchecks=[512, 2048, 8192])

    # 8. builder-parameter coverage: multi-tree BKT, non-default degree,
    #    2-tree KDT, odd int8 dim (byte-wise distance path)
    rng2 = np.random.default_rng(777)
    data = rng2.random((8000, 32), dtype=np.float32) * 100
    queries = rng2.random((100, 32), dtype=np.float32) * 100
    gen_fixture_ex("f32_l2_bkt2trees", data, queries, "Float", "L2",
                   [512, 2048], extra=("Index.BKTNumber=2",))
    data = rng2.random((8000, 48), dtype=np.float32)
    queries = rng2.random((100, 48), dtype=np.float32)
    gen_fixture_ex("f32_l2_deg16", data, queries, "Float", "L2", [512, 2048],
                   extra=("Index.NeighborhoodSize=16",))
    data = rng2.integers(-100, 101, (8000, 100)).astype(np.int8)
    queries = rng2.integers(-100, 101, (100, 100)).astype(np.int8)
    gen_fixture_ex("kdt_i8_cos_2trees", data, queries, "Int8", "Cosine",
                   [2048, 8192], algo="KDT", extra=("Index.KDTNumber=2",))
    rng3 = np.random.default_rng(4242)
    data = rng3.integers(-100, 101, (8000, 37)).astype(np.int8)
    queries = rng3.integers(-100, 101, (100, 37)).astype(np.int8)
    gen_fixture_ex("i8_l2_odd_d37", data, queries, "Int8", "L2", [512, 2048])

    # 9. iterative + online-add golden answers
    gen_iter_and_add_goldens()


if __name__ == "__main__":
    if sys.argv[1:] == ["cosine-add"]:
        sys.exit(gen_cosine_add_goldens())
    if sys.argv[1:] == ["dist"]:
        sys.exit(gen_dist_goldens())
    sys.exit(main())
