#!/usr/bin/env python3
"""Benchmark of the MI355X-native SPTAG search backend.

Measures BASELINE.json's metric — QPS at recall@10 >= 0.95 on a 10k-query
batch — on the named config. Default (no flags): config #2, SPTAG-BKT
10M x 128 float32 L2 on 1 GPU ("bkt_10m_d128_f32_l2").

A "step" is one batched search of the full query set through the hot path
(sptag_amd_search_batch_device: queries and outputs resident in HBM; the
host->device query upload happens once, before the timed region).

Multi-GPU (--gpus N, launched via torch.distributed.run): the SAME dataset
is range-sharded by contiguous VID ranges across ranks;
each rank builds/searches its own shard, one all-gather of per-shard top-k
per step, host merge on rank 0. Total work fixed => "scaling": "strong".

Synthetic data: overlapping Gaussian mixture (SIFT-like clusterability —
BASELINE.md synthetic-data note; i.i.d. uniform makes recall 0.95
unreachable for ANY backend). Fixed seed 2016.

A plain run does only what the headline figure needs: data, index, exact
truth, the MaxCheck sweep for the recall gate, warmup, the timed steps and
the result line. The built index (tree + graph; the vectors are regenerated
from the seed) is kept in a per-user cache keyed by the data, the build
parameters and the builder source, so only the first run of a workload
pays the on-GPU index build (`--prepare-index` fills the cache and exits;
`--no-index-cache` ignores it). The build runs under torch's deterministic
mode, so a rebuilt index is byte-identical to a cached one.

--dump-outputs DIR writes what the last timed step returned (vids.npy,
dists.npy) so two builds of the project can be compared output for output.

--full adds everything else the benchmark measures. cpu_baseline: the
REFERENCE CPU implementation (the oracle/_ref indexsearcher binary) timed
on the host cores on the same index files, full query batch; falls back to
the oracle C port if the binary is absent.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak (spec), MI355X_MICROARCH.md

CONFIGS = {
    # BASELINE.json configs[0] — plumbing scale (CPU-runnable reference case)
    "bkt_100k_d128_f32_l2": dict(n=100_000, d=128, dtype="f32", metric="L2",
                                 nq=1000, k=10, ncenters=1024, sigma=32.0),
    # BASELINE.json configs[1] — the headline single-GPU config (DEFAULT)
    "bkt_10m_d128_f32_l2": dict(n=10_000_000, d=128, dtype="f32", metric="L2",
                                nq=10_000, k=10, ncenters=8192, sigma=32.0),
    # quick smoke-scale variant for plumbing runs (not a bench line)
    "bkt_1m_d128_f32_l2": dict(n=1_000_000, d=128, dtype="f32", metric="L2",
                               nq=10_000, k=10, ncenters=4096, sigma=32.0),
    # BASELINE.json configs[2] — int8 cosine SPACEV shape. The search
    # kernel is bit-identical to the reference at every scale
    # (scripts/diag_scale.py); graph quality at 30M+ comes from the
    # round-2 recipe: NN-descent rounds + wide-prune search-refine
    # (reference RefineGraph semantics) + fill-pruned slots. See DESIGN.md
    # §5 for the measured progression.
    "bkt_100m_d100_i8_cos": dict(n=100_000_000, d=100, dtype="i8",
                                 metric="Cosine", nq=10_000, k=10,
                                 ncenters=16384, sigma=30.0, cand=160,
                                 degree=48, ntrees=4, refine=2, srefine=1,
                                 srefine_k=512, srefine_mc=2048,
                                 fill_pruned=True),
    # 30M validation scale for the config-#3 build recipe
    "bkt_30m_d100_i8_cos": dict(n=30_000_000, d=100, dtype="i8",
                                metric="Cosine", nq=10_000, k=10,
                                ncenters=16384, sigma=30.0, cand=160,
                                degree=48, ntrees=4, refine=2, srefine=1,
                                srefine_k=512, srefine_mc=2048,
                                fill_pruned=True),
    # BASELINE.json configs[4] — 1B int8 L2, meant for --gpus 8 (125M rows
    # per shard; per-shard recipe = the config-#3 recipe)
    "bkt_1b_d100_i8_l2": dict(n=1_000_000_000, d=100, dtype="i8",
                              metric="L2", nq=10_000, k=10,
                              ncenters=65536, sigma=30.0, cand=160,
                              degree=48, ntrees=4, refine=2, srefine=1,
                              srefine_k=512, srefine_mc=2048,
                              fill_pruned=True),
    # BASELINE.json configs[3] — KDT, embedding shape. Note: the KDT
    # algorithm's no-better-propagation termination caps recall on this
    # data family at ~0.93-0.94 for the REFERENCE implementation as well
    # (measured at 100k: reference 0.935, this builder 0.932) — the 0.95
    # gate is reported as unmet honestly; QPS comparisons stay
    # apples-to-apples at the plateau.
    "kdt_10m_d768_f32_cos": dict(n=10_000_000, d=768, dtype="f32",
                                 metric="Cosine", nq=10_000, k=10,
                                 ncenters=8192, style="emb", sigma=5.0,
                                 algo="KDT", cand=128),
    # KDT validation scale
    "kdt_1m_d768_f32_cos": dict(n=1_000_000, d=768, dtype="f32",
                                metric="Cosine", nq=10_000, k=10,
                                ncenters=4096, style="emb", sigma=5.0,
                                algo="KDT", cand=128),
    # int8 validation scale (same dtype/metric path as config #3)
    "bkt_10m_d100_i8_cos": dict(n=10_000_000, d=100, dtype="i8",
                                metric="Cosine", nq=10_000, k=10,
                                ncenters=8192, sigma=30.0),
    "bkt_10m_d100_i8_l2": dict(n=10_000_000, d=100, dtype="i8",
                               metric="L2", nq=10_000, k=10,
                               ncenters=8192, sigma=30.0),
}
DEFAULT_WORKLOAD = "bkt_10m_d128_f32_l2"
MC_SWEEP = [512, 1024, 2048, 4096, 8192, 16384]


def log(rank, *a):
    if rank == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


GEN_CHUNK = 1_000_000


def gen_data(cfg, shard, world, device, torch):
    """Deterministic mixture. The dataset is defined GLOBALLY in fixed 1M-row
    chunks with per-chunk seeds, so rank r's rows [lo, hi) are identical for
    every world size — N=1 and N=8 runs search the same data (strong-scaling
    comparability)."""
    n, d = cfg["n"], cfg["d"]
    gen = torch.Generator(device=device)
    gen.manual_seed(2016)
    if cfg.get("style") == "emb":
        # embedding-shaped: gaussian centers scaled vs unit noise (config #4)
        centers = torch.randn((cfg["ncenters"], d), generator=gen,
                              device=device) * cfg["sigma"]
    elif cfg["dtype"] == "i8":
        # SPACEV-shaped (int8 values ~U[-100,100]): the
        # hierarchical mixture centered at 0 so the int8 clamp at +-127
        # only cuts a rare tail (7% of coords). Round 1 reused the SIFT
        # [0,255] box here; the clamp then saturated 50% of ALL
        # coordinates at exactly +127 — half the dimensions binarized, a
        # data-generator bug that degrades metric structure at scale.
        # Round-1 int8 lines were measured on that flawed data.
        supers = torch.rand((256, d), generator=gen, device=device) * 160.0 - 80.0
        slab = torch.randint(0, 256, (cfg["ncenters"],), generator=gen,
                             device=device)
        centers = supers[slab] + torch.randn((cfg["ncenters"], d), generator=gen,
                                             device=device) * (cfg["sigma"] * 1.5)
    else:
        # SIFT-shaped: hierarchical mixture over the [0,255] box (super-
        # centers -> centers -> points; BASELINE.md clusterability note)
        supers = torch.rand((256, d), generator=gen, device=device) * 255.0
        slab = torch.randint(0, 256, (cfg["ncenters"],), generator=gen,
                             device=device)
        centers = supers[slab] + torch.randn((cfg["ncenters"], d), generator=gen,
                                             device=device) * (cfg["sigma"] * 1.5)
    lo = n * shard // world
    hi = n * (shard + 1) // world
    noise = 1.0 if cfg.get("style") == "emb" else cfg["sigma"]
    parts = []
    for c0 in range(lo // GEN_CHUNK, (hi + GEN_CHUNK - 1) // GEN_CHUNK):
        cs_, ce_ = c0 * GEN_CHUNK, min((c0 + 1) * GEN_CHUNK, n)
        gen.manual_seed(2016 + 100 + c0)
        lab = torch.randint(0, cfg["ncenters"], (ce_ - cs_,), generator=gen,
                            device=device)
        xc = centers[lab] + torch.randn((ce_ - cs_, d), generator=gen,
                                        device=device) * noise
        a = max(lo, cs_) - cs_
        b = min(hi, ce_) - cs_
        parts.append(xc[a:b])
        del lab, xc
    x = torch.cat(parts) if len(parts) > 1 else parts[0]
    del parts
    gen.manual_seed(2016 + 9999)
    qlab = torch.randint(0, cfg["ncenters"], (cfg["nq"],), generator=gen, device=device)
    q = centers[qlab] + torch.randn((cfg["nq"], d), generator=gen, device=device) * noise
    if cfg["dtype"] == "i8":
        x = x.clamp(-127, 127).round()
        q = q.clamp(-127, 127).round()
        return x.to(torch.int8), q.to(torch.int8), lo
    return x.float(), q.float(), lo


def shard_truth(x, q, k, metric, torch, lo, chunk=None):
    """Exact top-k of q against shard x (ids offset by lo). GEMM shortlist
    (f32) + float64 rescore of a 64-deep shortlist."""
    short = min(64, x.shape[0])
    if chunk is None:   # keep the [nq, chunk] distance tile ~2GB
        chunk = max(65_536, int(2e9 // (max(q.shape[0], 1) * 4)))
    xq = q.float()
    best_d = None
    best_i = None
    for s in range(0, x.shape[0], chunk):
        xc = x[s:s + chunk].float()
        dots = xq @ xc.T
        if metric == "L2":
            d2 = (xq * xq).sum(1, keepdim=True) + (xc * xc).sum(1)[None, :] - 2.0 * dots
        else:
            base = 1.0 if x.dtype == torch.float32 else 127.0
            d2 = base * base - dots
        vals, idx = torch.topk(d2, min(short, xc.shape[0]), dim=1, largest=False)
        idx = idx + s
        if best_d is None:
            best_d, best_i = vals, idx
        else:
            cd = torch.cat([best_d, vals], 1)
            ci = torch.cat([best_i, idx], 1)
            vals2, pos = torch.topk(cd, short, dim=1, largest=False)
            best_d = vals2
            best_i = torch.gather(ci, 1, pos)
    # exact float64 rescore of the shortlist
    xv = x[best_i.reshape(-1)].reshape(*best_i.shape, x.shape[1]).double()
    qv = q.double()[:, None, :]
    if metric == "L2":
        dd = ((xv - qv) ** 2).sum(-1)
    else:
        base = 1.0 if x.dtype == torch.float32 else 127.0
        dd = base * base - (xv * qv).sum(-1)
    vals, pos = torch.topk(dd, k, dim=1, largest=False)
    ids = torch.gather(best_i, 1, pos) + lo
    return ids.int(), vals.float()


def merge_topk(vids, dists, k):
    """host merge of concatenated per-shard top-k lists (AggregatorService
    AggregateResults semantics: concatenate + select)."""
    idx = np.argsort(dists, axis=1, kind="stable")[:, :k]
    return (np.take_along_axis(vids, idx, 1)[:, :k],
            np.take_along_axis(dists, idx, 1)[:, :k])


def recall_at_k(got_vids, truth_vids, k):
    nq = got_vids.shape[0]
    hits = 0
    for i in range(nq):
        hits += len(set(truth_vids[i, :k].tolist()) & set(got_vids[i, :k].tolist()))
    return hits / (nq * k)


def cpu_baseline_leg(index_dir, q_np, mc, k, seconds_budget=25):
    """Time the reference CPU searcher (oracle/_ref) on this box's host
    cores on the FULL metric batch (10k queries — it costs seconds at 256
    cores; VERDICT r01 asked for the full batch over a 1k sample).
    Returns the cpu_baseline JSON object or None."""
    import multiprocessing
    cores = multiprocessing.cpu_count()
    ref = os.path.join(REPO, "oracle", "_ref", "indexsearcher")
    nq = q_np.shape[0]
    qfile = os.path.join(index_dir, "bench_queries.bin")
    with open(qfile, "wb") as f:
        f.write(np.int32(nq).tobytes())
        f.write(np.int32(q_np.shape[1]).tobytes())
        f.write(q_np[:nq].tobytes())
    vt = "Float" if q_np.dtype == np.float32 else "Int8"
    if os.path.exists(ref):
        try:
            out = subprocess.run(
                [ref, "-d", str(q_np.shape[1]), "-v", vt, "-f", "DEFAULT",
                 "-i", qfile, "-x", index_dir, "-k", str(k), "-m", str(mc),
                 "-t", str(cores)],
                capture_output=True, text=True, timeout=1200, cwd=index_dir)
            qps = None
            for line in (out.stdout + out.stderr).splitlines():
                # "[1] 0-NQ  mc  avg  p99  p95  recall  QPS  peakGB"
                parts = line.split()
                for i, tok in enumerate(parts):
                    if tok == f"0-{nq}" and len(parts) >= i + 7:
                        qps = float(parts[i + 6])
                        break
            if qps:
                return {"value": qps, "unit": "queries/s", "cores": cores,
                        "kind": "reference",
                        "sample": f"{nq} queries @ MaxCheck {mc}, "
                                  f"reference indexsearcher -t {cores}"}
        except Exception as e:  # noqa: BLE001
            print("[bench] reference baseline failed:", e, file=sys.stderr)
    # fallback: the oracle C port, in process
    try:
        from oracle.pyoracle import OrcIndex
        oix = OrcIndex.load(index_dir)
        t0 = time.time()
        done = 0
        step = 128
        while time.time() - t0 < seconds_budget and done < q_np.shape[0]:
            oix.search_batch(q_np[done:done + step], k, mc, nthreads=cores)
            done += step
        dt = time.time() - t0
        return {"value": done / dt, "unit": "queries/s", "cores": cores,
                "kind": "port",
                "sample": f"{done} queries @ MaxCheck {mc}, oracle port, "
                          f"{cores} OpenMP threads"}
    except Exception as e:  # noqa: BLE001
        print("[bench] oracle baseline failed:", e, file=sys.stderr)
        return None


# ------------------------------------------------------------------ #
# built-index cache (tree + graph; vectors are regenerated from the seed)
# ------------------------------------------------------------------ #

INDEX_CACHE_MAX_BYTES = 4 << 30   # larger indexes are rebuilt, not stored


def index_cache_root():
    root = os.environ.get("SPTAG_AMD_CACHE")
    if not root:
        base = os.environ.get("XDG_CACHE_HOME") or os.path.join(
            os.path.expanduser("~"), ".cache")
        root = os.path.join(base, "sptag_amd")
    return os.path.join(root, "bench_index")


def index_cache_key(workload, x_np, build_kw, shard, world):
    """Identity of a built index: the data actually generated (strided row
    fingerprint), every build parameter, the shard, and the builder source
    (a changed builder never reuses an old index)."""
    h = hashlib.sha256()
    with open(os.path.join(REPO, "sptag_amd", "build.py"), "rb") as f:
        h.update(f.read())
    h.update(json.dumps([workload, list(x_np.shape), str(x_np.dtype), shard,
                         world, sorted(build_kw.items())]).encode())
    stride = max(1, x_np.shape[0] // 4096)
    h.update(np.ascontiguousarray(x_np[::stride]).tobytes())
    return f"{workload}-s{shard}of{world}-{h.hexdigest()[:20]}"


def index_cache_load(path):
    try:
        return {name: np.load(os.path.join(path, name + ".npy"))
                for name in ("tree_start", "tree_nodes", "graph")}
    except (OSError, ValueError):
        return None


def index_cache_store(path, arrays):
    """Write to a private temp folder, then rename: a reader never sees a
    half-written index. Returns False (with the reason logged by the
    caller) when the index is too large or the cache is not writable."""
    nbytes = sum(arrays[name].nbytes
                 for name in ("tree_start", "tree_nodes", "graph"))
    if nbytes > INDEX_CACHE_MAX_BYTES:
        return False
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        os.makedirs(tmp, exist_ok=True)
        for name in ("tree_start", "tree_nodes", "graph"):
            np.save(os.path.join(tmp, name + ".npy"),
                    np.ascontiguousarray(arrays[name]))
        os.rename(tmp, path)
        return True
    except OSError:
        shutil.rmtree(tmp, ignore_errors=True)
        return os.path.isdir(path)


DUMP_MAX_BYTES = 60_000_000


def dump_outputs(out_dir, vids, dists):
    """vids.npy (float64: exact for any int32 id) and dists.npy (float32) of
    one step, rows aligned. Above the size cap a fixed seeded row sample is
    written instead (rows.npy holds the sampled row numbers)."""
    os.makedirs(out_dir, exist_ok=True)
    vids = np.asarray(vids)
    dists = np.asarray(dists)
    row_bytes = vids.shape[1] * (8 + 4) + 8
    if vids.shape[0] * row_bytes > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // row_bytes
        rows = np.sort(np.random.default_rng(2016).choice(
            vids.shape[0], size=keep, replace=False))
        vids, dists = vids[rows], dists[rows]
        np.save(os.path.join(out_dir, "rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "vids.npy"), vids.astype(np.float64))
    np.save(os.path.join(out_dir, "dists.npy"), dists.astype(np.float32))


def main():
    # reduce allocator fragmentation at 100M+ build scale
    os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default=DEFAULT_WORKLOAD)
    ap.add_argument("--mc", type=int, default=0, help="force MaxCheck (skip sweep)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need "
                         "(the CPU baseline leg on the saved index)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline leg")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's results to "
                         "DIR/vids.npy and DIR/dists.npy")
    ap.add_argument("--no-index-cache", action="store_true",
                    help="always build the index; neither read nor write "
                         "the built-index cache")
    ap.add_argument("--prepare-index", action="store_true",
                    help="build the workload's index into the cache and "
                         "exit (nothing to do without a HIP device)")
    ap.add_argument("--ntrees", type=int, default=4)
    ap.add_argument("--degree", type=int, default=0,
                    help="graph NeighborhoodSize (reference default 32)")
    ap.add_argument("--cand", type=int, default=0)
    ap.add_argument("--ncenters", type=int, default=0)
    ap.add_argument("--refine", type=int, default=-1,
                    help="NN-descent refine rounds (override config)")
    ap.add_argument("--srefine", type=int, default=-1,
                    help="search-refine rounds (override config)")
    ap.add_argument("--srefine-k", type=int, default=0)
    ap.add_argument("--srefine-mc", type=int, default=0)
    ap.add_argument("--fill-pruned", type=int, default=-1)
    ap.add_argument("--init-pivots", type=int, default=0,
                    help="NumberOfInitialDynamicPivots override (seed leaves)")
    ap.add_argument("--force-shard", default="",
                    help="R/W: build+search shard R of W on ONE process "
                         "(no collectives; shard-local recall) — verifies "
                         "the config-#5 per-shard path on a single GPU")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    if args.prepare_index and not torch.cuda.is_available():
        print("[bench] no HIP device: no index to prepare", file=sys.stderr)
        return 0
    cfg = dict(CONFIGS[args.workload])
    if args.ncenters:
        cfg["ncenters"] = args.ncenters
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    forced_shard = False
    if args.force_shard:
        r, w = args.force_shard.split("/")
        rank, world, local_rank = int(r), int(w), 0
        forced_shard = True
    dist = None
    if world > 1 and not forced_shard:
        import torch.distributed as tdist
        dist = tdist
        dist.init_process_group("nccl")
        torch.cuda.set_device(local_rank)
    assert torch.cuda.is_available(), "bench requires a HIP device"
    device = f"cuda:{local_rank}"
    torch.cuda.set_device(device)

    import sptag_amd
    from sptag_amd.build import build_index_arrays

    t_setup0 = time.time()
    x, q, lo = gen_data(cfg, rank, world, device, torch)
    log(rank, f"data: shard {rank}/{world} rows {x.shape} ({time.time()-t_setup0:.1f}s)")

    t0 = time.time()
    x_np = x.cpu().numpy()
    build_kw = dict(
        algo=cfg.get("algo", "BKT"),
        degree=args.degree or cfg.get("degree", 32),
        cand=args.cand or cfg.get("cand", 256),
        kdt_trees=cfg.get("kdt_trees", 2),
        ntrees=cfg.get("ntrees", args.ntrees),
        refine_rounds=args.refine if args.refine >= 0 else cfg.get("refine", 0),
        search_refine_rounds=(args.srefine if args.srefine >= 0
                              else cfg.get("srefine", 0)),
        srefine_k=args.srefine_k or cfg.get("srefine_k", 512),
        srefine_mc=args.srefine_mc or cfg.get("srefine_mc", 8192),
        fill_pruned=bool(args.fill_pruned if args.fill_pruned >= 0
                         else cfg.get("fill_pruned", False)))
    arrays = None
    cache_state = "off"
    if not args.no_index_cache:
        cache_path = os.path.join(
            index_cache_root(),
            index_cache_key(args.workload, x_np, build_kw, rank, world))
        arrays = index_cache_load(cache_path)
        cache_state = "hit" if arrays is not None else "miss"
    if arrays is not None:
        from sptag_amd.build import normalize_base
        arrays["vectors"] = normalize_base(x_np, cfg["metric"])
        log(rank, f"index loaded from {cache_path} ({time.time()-t0:.1f}s)")
    else:
        # The index is an INPUT of the timed path: the same arguments must
        # give the same index in every run, cache or no cache. The builder's
        # float index_add_ sums (k-means centroids) and rocBLAS kernels that
        # may use atomics are order-dependent by default, so the build runs
        # under torch's deterministic mode (warn-only: integer bincount /
        # cumsum are flagged by torch but are exact).
        import warnings
        det_prev = (torch.are_deterministic_algorithms_enabled(),
                    torch.is_deterministic_algorithms_warn_only_enabled())
        fill_prev = torch.utils.deterministic.fill_uninitialized_memory
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.utils.deterministic.fill_uninitialized_memory = False
        try:
            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message=".*deterministic.*")
                arrays = build_index_arrays(
                    x_np, cfg["metric"], device=device, normalized=False,
                    verbose=(rank == 0), **build_kw)
        finally:
            torch.use_deterministic_algorithms(det_prev[0],
                                               warn_only=det_prev[1])
            torch.utils.deterministic.fill_uninitialized_memory = fill_prev
        log(rank, f"index built ({time.time()-t0:.1f}s)")
        if not args.no_index_cache:
            t0 = time.time()
            kept = index_cache_store(cache_path, arrays)
            log(rank, f"index {'stored in' if kept else 'NOT stored in'} "
                      f"{cache_path} ({time.time()-t0:.1f}s)")
    if args.prepare_index:
        return 0
    torch.cuda.empty_cache()   # release build-phase cache so the extension's
    t0 = time.time()           # hipMalloc can place the index blobs
    if cfg.get("algo") == "KDT":
        ix = sptag_amd.AnnIndex.FromArraysKDT(
            arrays["vectors"], arrays["tree_start"], arrays["tree_nodes"],
            arrays["graph"], cfg["metric"], device=local_rank)
    else:
        ix = sptag_amd.AnnIndex.FromArrays(
            arrays["vectors"], arrays["tree_start"], arrays["tree_nodes"],
            arrays["graph"], cfg["metric"], device=local_rank)
    ipv = args.init_pivots or cfg.get("init_pivots", 0)
    if ipv:
        ix.SetSearchParams(init_pivots=ipv)
    log(rank, f"index uploaded ({time.time()-t0:.1f}s)")

    # truth runs in the STORED vector space (cosine bases are normalized on
    # disk; queries stay RAW — SURVEY.md §8a cosine notes).
    if cfg["metric"] == "Cosine":
        xs = torch.as_tensor(arrays["vectors"], device=device)
    else:
        xs = x
    del arrays
    torch.cuda.empty_cache()
    t0 = time.time()
    tv, td = shard_truth(xs, q, cfg["k"], cfg["metric"], torch, lo)
    if dist:
        gv = [torch.zeros_like(tv) for _ in range(world)]
        gd = [torch.zeros_like(td) for _ in range(world)]
        dist.all_gather(gv, tv.contiguous())
        dist.all_gather(gd, td.contiguous())
        tv_np, _ = merge_topk(torch.cat(gv, 1).cpu().numpy(),
                              torch.cat(gd, 1).cpu().numpy(), cfg["k"])
    else:
        tv_np = tv.cpu().numpy()
    log(rank, f"truth ready ({time.time()-t0:.1f}s)")

    k = cfg["k"]
    nq = cfg["nq"]
    d_q = q.contiguous()
    d_vids = torch.empty((nq, k), dtype=torch.int32, device=device)
    d_dists = torch.empty((nq, k), dtype=torch.float32, device=device)

    def one_step(mc):
        ix.BatchSearchDevice(d_q.data_ptr(), nq, k, d_vids.data_ptr(),
                             d_dists.data_ptr(), mc)

    def step_merged(mc):
        """one full job step: per-shard search + top-k exchange + merge.
        The RCCL all-gather of (k x 8B) x nq per shard and the device-side
        top-k merge (AggregatorService::AggregateResults semantics,
        reference AggregatorService.cpp:363) are part of the timed work at
        world > 1."""
        one_step(mc)
        v = (d_vids + lo).masked_fill(d_vids < 0, -1)
        if not dist:
            return v, d_dists
        gv = [torch.empty_like(v) for _ in range(world)]
        gd = [torch.empty_like(d_dists) for _ in range(world)]
        dist.all_gather(gv, v.contiguous())
        dist.all_gather(gd, d_dists.contiguous())
        av = torch.cat(gv, 1)
        ad = torch.cat(gd, 1)
        vals, pos = torch.topk(ad, k, dim=1, largest=False)
        return torch.gather(av, 1, pos), vals

    def merged_results(mc):
        mv, md = step_merged(mc)
        return mv.cpu().numpy(), md.cpu().numpy()

    # MaxCheck sweep -> cheapest mc with recall >= 0.95
    chosen_mc, chosen_recall = None, 0.0
    sweep = [args.mc] if args.mc else MC_SWEEP
    for mc in sweep:
        gv, _ = merged_results(mc)
        r = recall_at_k(gv, tv_np, k)
        log(rank, f"sweep mc={mc}: recall@{k}={r:.4f}")
        chosen_mc, chosen_recall = mc, r
        if r >= 0.95:
            break

    # timed region — a step is the WHOLE job: search + (at N>1) top-k
    # all-gather + device merge
    for _ in range(args.warmup):
        step_merged(chosen_mc)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        last_out = step_merged(chosen_mc)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.time() - t0
    if dist:
        te = torch.tensor([elapsed], device=device)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())

    kernel_ms, checked, popped = ix.LastStats()
    esz = 4 if cfg["dtype"] == "f32" else 1
    alg_bytes = checked * cfg["d"] * esz + popped * ix.degree * 4
    achieved = (alg_bytes / 1e9) / (kernel_ms / 1e3) if kernel_ms > 0 else 0.0

    # measured HBM traffic per launch: PMC counters are collected in their
    # own rocprofv3 passes (they cannot run inside this bench process), so
    # bench reports the committed calibration for THIS workload+MaxCheck
    # (profiles/pmc_calib.json: FETCH_SIZE/WRITE_SIZE with the gfx950
    # correction measured on a known-byte pattern; see profiles/README note
    # inside the file). Null when no matching calibration exists.
    traffic = None
    traffic_src = None
    try:
        calib = json.load(open(os.path.join(REPO, "profiles",
                                            "pmc_calib.json")))
        ent = calib.get(args.workload)
        if ent and int(ent.get("mc", -1)) == int(chosen_mc):
            traffic = int(ent["hbm_bytes_per_launch"])
            traffic_src = ent.get("source")
    except (OSError, ValueError, KeyError):
        pass

    value = nq * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    result = None
    if rank == 0 or forced_shard:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last_out[0].cpu().numpy(),
                         last_out[1].cpu().numpy())
        cpu = None
        if (args.full and not args.no_cpu_baseline and not dist
                and not forced_shard):
            t0 = time.time()
            idx_dir = os.environ.get("BENCH_INDEX_DIR", "/tmp/bench_index")
            os.makedirs(idx_dir, exist_ok=True)
            ix.Save(idx_dir)
            q_np = q.cpu().numpy()
            cpu = cpu_baseline_leg(idx_dir, q_np, chosen_mc, k)
            log(rank, f"cpu baseline done ({time.time()-t0:.1f}s): {cpu}")
        result = {
            "metric": "QPS @ recall@10>=0.95, batch=10k queries",
            "value": round(value, 1),
            "unit": "queries/s",
            "n_gpus": 1 if forced_shard else world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": cfg["dtype"],
            "data": "synthetic",
            "full": bool(args.full),
            "index_cache": cache_state,
            "config": {
                "workload": args.workload,
                "n": cfg["n"], "dim": cfg["d"], "metric": cfg["metric"],
                "nq": nq, "k": k, "max_check": chosen_mc,
                "recall_at_10": round(chosen_recall, 4),
                "recall_gate_met": bool(chosen_recall >= 0.95),
                "sharding": (f"forced shard {rank}/{world} (1 process, "
                             "shard-local)" if forced_shard else
                             "contiguous VID ranges" if world > 1 else
                             "none"),
            },
            "roofline": {
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "traffic_source": traffic_src,
                "kernel_ms_per_step": round(kernel_ms, 3),
                "alg_bytes_per_step": alg_bytes,
            },
            "cpu_baseline": cpu,
        }
        print(json.dumps(result))
    if dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
