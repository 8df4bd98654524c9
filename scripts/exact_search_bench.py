#!/usr/bin/env python3
"""Measurements behind profiles/exact_search.txt (one process, one GPU).

For each workload (f32 d=128 L2, int8 d=100 cosine; n rows, nq queries, k)
an index over seeded random rows with a trivial tree and graph, which neither
path reads. Timed with HIP events on the default stream, both calls ending in
a device synchronise inside the library:

  exact   AnnIndex.ExactSearchDevice (queries and outputs in HBM)
  scan    AnnIndex.Truth, the one-wave-per-query scan kernel (host pointers:
          its span includes a copy of the queries in and of nq*k results out)

The two alternate for --rounds rounds of --reps calls (the scan gets
--scan-reps) after one warm-up call each; the outputs are compared bit for
bit first. --big-n adds the exact path alone at a larger row count.

Prints plain lines; --out also writes them to a file as they come."""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

OUT = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def event_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def make_index(sptag_amd, vt, dm, n, d, seed):
    rng = np.random.default_rng(seed)
    if vt == "f32":
        x = rng.standard_normal((n, d), dtype=np.float32)
    else:
        x = rng.integers(-127, 128, (n, d), dtype=np.int8)
    return sptag_amd.AnnIndex.FromArrays(
        x, np.zeros(1, dtype=np.int32), np.zeros((2, 3), dtype=np.int32),
        np.full((n, 2), -1, dtype=np.int32), dm)


def make_queries(vt, nq, d, seed):
    rng = np.random.default_rng(seed)
    if vt == "f32":
        return rng.standard_normal((nq, d), dtype=np.float32)
    return rng.integers(-127, 128, (nq, d), dtype=np.int8)


def exact_fn(torch, ix, q, k):
    d_q = torch.from_numpy(q).to("cuda:0")
    d_v = torch.empty((q.shape[0], k), dtype=torch.int32, device="cuda:0")
    d_d = torch.empty((q.shape[0], k), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fn = lambda: ix.ExactSearchDevice(d_q.data_ptr(), q.shape[0], k, d_v.data_ptr(),
                                      d_d.data_ptr())
    return fn, d_v, d_d


def workload(args, torch, sptag_amd, vt, dm, d):
    tag = f"{vt} d={d} {dm} n={args.n} nq={args.nq} k={args.k}"
    ix = make_index(sptag_amd, vt, dm, args.n, d, 11)
    q = make_queries(vt, args.nq, d, 12)
    exact, d_v, d_d = exact_fn(torch, ix, q, args.k)
    res = {}

    def scan():
        res["v"], res["d"] = ix.Truth(q, args.k)

    exact()         # warm-up, and the outputs to compare
    scan()
    same = (np.array_equal(d_v.cpu().numpy(), res["v"]) and
            np.array_equal(d_d.cpu().numpy().view(np.uint32), res["d"].view(np.uint32)))
    say(f"{tag}: exact equals scan bit for bit: {same}")
    te, ts = [], []
    for rnd in range(args.rounds):
        e = event_ms(torch, exact, args.reps)
        s = event_ms(torch, scan, args.scan_reps)
        te += e
        ts += s
        say(f"{tag}: round {rnd}: exact median {statistics.median(e):.2f} ms "
            f"(min {min(e):.2f}, max {max(e):.2f}, {len(e)} calls); scan median "
            f"{statistics.median(s):.1f} ms (min {min(s):.1f}, max {max(s):.1f}, "
            f"{len(s)} calls)")
    me, ms = statistics.median(te), statistics.median(ts)
    say(f"{tag}: exact {me:.2f} ms, spread {(max(te) - min(te)) / me * 100:.1f}% of "
        f"median; scan {ms:.1f} ms, spread {(max(ts) - min(ts)) / ms * 100:.1f}%; "
        f"scan / exact = {ms / me:.1f}; slowest exact call against fastest scan "
        f"call = {min(ts) / max(te):.1f}")


def big(args, torch, sptag_amd):
    tag = f"f32 d=128 L2 n={args.big_n} nq={args.big_nq} k={args.k}"
    ix = make_index(sptag_amd, "f32", "L2", args.big_n, 128, 21)
    q = make_queries("f32", args.big_nq, 128, 22)
    exact, _, _ = exact_fn(torch, ix, q, args.k)
    exact()
    t = event_ms(torch, exact, args.reps)
    say(f"{tag}: exact alone: median {statistics.median(t):.1f} ms (min {min(t):.1f}, "
        f"max {max(t):.1f}, {len(t)} calls)")


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scan-reps", type=int, default=2)
    ap.add_argument("--big-n", type=int, default=0)
    ap.add_argument("--big-nq", type=int, default=10_000)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        OUT = open(args.out, "w")
    import torch
    import sptag_amd
    if not sptag_amd.gpu_available():
        sys.exit("exact_search_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    workload(args, torch, sptag_amd, "f32", "L2", 128)
    workload(args, torch, sptag_amd, "i8", "Cosine", 100)
    if args.big_n:
        big(args, torch, sptag_amd)


if __name__ == "__main__":
    main()
