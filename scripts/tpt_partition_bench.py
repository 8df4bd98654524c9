#!/usr/bin/env python3
"""Measurements behind profiles/tpt_partition.txt (one process, one GPU).

n x 128 seeded random f32 rows. One TP-tree partition at --leaf is timed as one
whole call, wall clock around a device synchronise (both paths read counts back
on the host every level, so device events alone would miss their waits),
alternating for --rounds rounds of --reps calls after one warm-up each:

  torch   build._tpt_leaves: a dense random direction a level, two sorts, a
          split at the median (the parent's step)
  hip     build._tpt_leaves_hip: tpt_partition_device with the reference's
          parameters (samples 1000, 5 dimensions, 100 trials)

with the peak extra device memory and the leaf sizes of each. Then the
candidate phase of build_rng_graph (--trees partitions, the leaf kNN and the
pool join on their HIP kernels, up to the candidate pools) with each partition,
--build-reps times each after one warm-up.

Prints plain lines; --out also writes them to a file as they come."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_search_bench                                # noqa: E402
from group_knn_bench import say, summary, peak_extra     # noqa: E402


def wall_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - a) * 1e3)
    return times


def workload(args, torch, build):
    n, d = args.n, 128
    tag = f"f32 d=128 n={n} leaf={args.leaf}"
    dev = torch.device("cuda:0")
    xf = torch.from_numpy(np.random.default_rng(11).standard_normal(
        (n, d), dtype=np.float32)).to(dev)

    def gen():
        g = torch.Generator(device=dev)
        g.manual_seed(2016 + 77)
        return g
    fns = {"torch": lambda: build._tpt_leaves(xf, args.leaf, gen()),
           "hip": lambda: build._tpt_leaves_hip(xf, args.leaf, gen())}
    for name, fn in fns.items():
        perm, starts, counts = fn()      # warm-up, and the leaves to describe
        assert int(counts.sum()) == n and perm.sort().values.equal(torch.arange(n, device=dev))
        say(f"{tag}: partition {name}: {counts.numel()} leaves, sizes min {int(counts.min())}, "
            f"median {int(counts.median())}, max {int(counts.max())}; peak extra device memory "
            f"{peak_extra(torch, fn) / 2**20:.0f} MiB")
    say(f"{tag}: partition hip: the library's own buffers (three lists and the side codes, 16 "
        f"bytes a member, freed at return) are outside torch's counter: {16 * n / 2**20:.0f} MiB "
        "by their sizes")
    th, tt = [], []
    for rnd in range(args.rounds):
        h = wall_ms(torch, fns["hip"], args.reps)
        t = wall_ms(torch, fns["torch"], args.reps)
        th += h
        tt += t
        say(f"{tag}: partition: round {rnd}: hip median {statistics.median(h):.2f} ms, torch "
            f"median {statistics.median(t):.2f} ms")
    mh, sh = summary(tag, "partition hip", th)
    mt, st = summary(tag, "partition torch", tt)
    say(f"{tag}: partition: torch / hip = {mt / mh:.2f}; torch - hip = {mt - mh:.2f} ms against "
        f"the two spreads combined {sh + st:.2f} ms")

    cand, kper = 256, 64
    self_ids = torch.arange(n, device=dev, dtype=torch.int32)
    join = build._join_fn("hip")

    def candidates(tpt):
        g, ids, dst = gen(), None, None
        for _ in range(args.trees):
            perm, starts, counts = build._tpt_fn(tpt)(xf, args.leaf, g)
            tids, tdst = build._leaf_knn_hip(xf, perm, starts, counts, kper)
            if ids is None:
                ids, dst = join(xf, tids, tdst, tids[:, :0], tdst[:, :0], cand, self_ids)
            else:
                ids, dst = join(xf, ids, dst, tids, tdst, cand, self_ids, out=(ids, dst))
        return ids, dst
    for tpt in ("hip", "torch"):
        fn = lambda: candidates(tpt)
        ids, _ = fn()       # warm-up
        say(f"{tag}: candidate phase tpt={tpt}, {args.trees} trees: "
            f"{float((ids >= 0).sum(1).float().mean()):.1f} candidates a row")
        del ids
        summary(tag, f"candidate phase tpt={tpt} wall", wall_ms(torch, fn, args.build_reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--leaf", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--build-reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        exact_search_bench.OUT = open(args.out, "w")
    import torch
    import sptag_amd
    from sptag_amd import build
    if not sptag_amd.gpu_available():
        sys.exit("tpt_partition_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    workload(args, torch, build)


if __name__ == "__main__":
    main()
