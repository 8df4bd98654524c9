#!/usr/bin/env python3
"""Measurements behind profiles/shard_merge.txt (one process, one GPU).

  merge   the library's shard merge against the form bench.py uses on the
          same lists (torch.cat + torch.topk + gather), at nq=10000, S=8,
          k_in=k=10. Both timed with HIP events on the default stream, median
          of --reps after --warmup. sptag_amd_merge_topk_device returns after
          a device synchronise, so its event span is the whole call (launch,
          kernel, the host's wake-up); the torch form is three asynchronous
          launches. The kernels' own times come from a separate
          `rocprofv3 --kernel-trace --stats` run of `--part merge`.
  set     ShardedIndex over 8 co-located shards of a bench.py workload's
          vectors (default the 1M f32 one, 125k vectors a shard): wall time
          of BatchSearchDevice against the sum of the eight shards' kernel
          times from sptag_amd_last_stats, and against one merge call.

Prints plain lines; --out also writes them to a file as they come."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

OUT = None    # open file of --out; every line goes there as it is printed


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def event_median_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def part_merge(args, torch, sptag_amd):
    S, nq, k = args.shards, args.nq, args.k
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(2016)
    dists = torch.rand((S, nq, k), generator=g, device=dev).sort(-1).values.contiguous()
    # distinct ids inside a list; shard s owns [s*nloc, (s+1)*nloc)
    nloc = 1_250_000
    i = torch.arange(k, device=dev, dtype=torch.int64)[None, None, :]
    qi = torch.arange(nq, device=dev, dtype=torch.int64)[None, :, None]
    si = torch.arange(S, device=dev, dtype=torch.int64)[:, None, None]
    vids = ((i * 7919 + qi * 31 + si * 17) % nloc).to(torch.int32).contiguous()
    base = (np.arange(S) * nloc).astype(np.int32)
    d_base = torch.as_tensor(base, device=dev)
    out_v = torch.empty((nq, k), dtype=torch.int32, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    lib = sptag_amd.load_library()
    basep = base.ctypes.data_as(ctypes.c_void_p)

    def ours():
        rc = lib.sptag_amd_merge_topk_device(
            0, S, nq, k, k, ctypes.c_void_p(vids.data_ptr()),
            ctypes.c_void_p(dists.data_ptr()), basep,
            ctypes.c_void_p(out_v.data_ptr()), ctypes.c_void_p(out_d.data_ptr()))
        assert rc == 0, rc

    gv = vids + d_base[:, None, None]      # bench.py adds its `lo` before the gather
    lists_v = [gv[s] for s in range(S)]
    lists_d = [dists[s] for s in range(S)]
    res = {}

    def torch_form():
        av = torch.cat(lists_v, 1)
        ad = torch.cat(lists_d, 1)
        vals, pos = torch.topk(ad, k, dim=1, largest=False)
        res["v"], res["d"] = torch.gather(av, 1, pos), vals

    ours()
    torch_form()
    torch.cuda.synchronize()
    same_d = bool((out_d == res["d"]).all())
    same_v = float((out_v == res["v"]).float().mean())
    say(f"merge: S={S} nq={nq} k_in=k_out={k}; distances equal to the torch form: "
        f"{same_d}; ids equal: {same_v:.6f} of entries (ties may differ)")
    # alternate the two forms, as the measuring guide asks for comparisons
    r = {"ours": [], "torch": []}
    for rnd in range(3):
        r["ours"].append(event_median_ms(torch, ours, args.warmup, args.reps))
        r["torch"].append(event_median_ms(torch, torch_form, args.warmup, args.reps))
    for name, label in (("ours", "sptag_amd_merge_topk_device (whole call)"),
                        ("torch", "torch.cat + topk + gather (3 async launches)")):
        for rnd, (med, lo, hi) in enumerate(r[name]):
            say(f"merge: {label}: round {rnd}: median {med * 1e3:.1f} us "
                f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f}) over {args.reps} "
                f"after {args.warmup} warm-ups")


def part_set(args, torch, sptag_amd):
    import warnings
    import bench
    from sptag_amd.build import build_index_arrays
    cfg = dict(bench.CONFIGS[args.workload])
    S, k, nq, mc = args.shards, cfg["k"], cfg["nq"], args.mc
    dev = "cuda:0"
    shards, q = [], None
    t0 = time.time()
    torch.use_deterministic_algorithms(True, warn_only=True)
    for s in range(S):
        x, q, lo = bench.gen_data(cfg, s, S, dev, torch)
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=".*deterministic.*")
            a = build_index_arrays(x.cpu().numpy(), cfg["metric"], device=dev,
                                   normalized=False, degree=32, cand=256, ntrees=4)
        del x
        torch.cuda.empty_cache()
        shards.append(sptag_amd.AnnIndex.FromArrays(
            a["vectors"], a["tree_start"], a["tree_nodes"], a["graph"],
            cfg["metric"], device=0))
        say(f"set: shard {s}: {shards[-1].n} vectors from row {lo}, built "
            f"({time.time() - t0:.0f}s so far)")
    torch.use_deterministic_algorithms(False)
    sh = sptag_amd.ShardedIndex.FromIndexes(shards)
    d_q = q.contiguous()
    d_v = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_d = torch.empty((nq, k), dtype=torch.float32, device=dev)

    def step():
        sh.BatchSearchDevice(d_q.data_ptr(), nq, k, d_v.data_ptr(), d_d.data_ptr(), mc)

    for _ in range(args.warmup):
        step()
    walls, sums = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        step()                      # returns after its own device synchronise
        walls.append((time.perf_counter() - t) * 1e3)
        sums.append(sum(ix.LastStats()[0] for ix in shards))
    wall, ksum = statistics.median(walls), statistics.median(sums)
    say(f"set: workload {args.workload}, {S} shards on one device, "
        f"{sh.NumVectors()} vectors, nq={nq} k={k} MaxCheck={mc}")
    say(f"set: end-to-end BatchSearchDevice: median {wall:.2f} ms "
        f"(min {min(walls):.2f}, max {max(walls):.2f}) over {args.reps} "
        f"after {args.warmup} warm-ups = {nq / wall * 1e3:.0f} QPS")
    say(f"set: sum of the {S} per-shard search kernel times "
        f"(sptag_amd_last_stats): median {ksum:.2f} ms; "
        f"end-to-end minus that: {wall - ksum:.2f} ms "
        f"({(wall - ksum) / wall * 100:.1f}% of the call)")
    # recall against the set's own exact answer, on the first 1000 queries
    nt = min(nq, 1000)
    tv, _ = sh.Truth(q[:nt].cpu().numpy(), k)
    got = d_v[:nt].cpu().numpy()
    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(got, tv))
    say(f"set: recall@{k} against ShardedIndex.Truth ({nt} queries): "
        f"{hits / (nt * k):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["merge", "set", "both"], default="both")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--mc", type=int, default=2048)
    ap.add_argument("--workload", default="bkt_1m_d128_f32_l2")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP device: nothing here is measured on a CPU"
    global OUT
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        OUT = open(args.out, "w")
    torch.zeros(1, device="cuda:0")     # torch's context first, as bench.py does
    import sptag_amd
    say("device:", torch.cuda.get_device_name(0), "| devices visible:",
        torch.cuda.device_count())
    if args.part in ("merge", "both"):
        part_merge(args, torch, sptag_amd)
    if args.part in ("set", "both"):
        part_set(args, torch, sptag_amd)
    return 0


if __name__ == "__main__":
    sys.exit(main())
