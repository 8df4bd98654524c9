#!/usr/bin/env python3
"""Measurements behind profiles/kmeans_assign.txt (one process, one GPU).

n x 128 seeded random f32 rows, L2. A level of --clusters equal clusters of
the rows (a random partition: the timings do not depend on what the clusters
hold) with K = --k centers each, drawn from their members. Two steps are timed
as one whole call of the HIP path against the torch step of _kmeans_split run
cluster by cluster, with HIP events on the default stream, alternating for
--rounds rounds of --reps calls after one warm-up each:

  lloyd   one Lloyd iteration over --sample sampled members of every cluster
            hip    kmeans_assign_device(update=1), one call
            torch  cdist + argmin + index_add_ + bincount per cluster
  final   the final assignment of all n members
            hip    kmeans_assign_device(update=0), one call
            torch  cdist + argmin, the masked argmin for the representatives
                   and bincount per cluster (no .item() calls)

Then build_bkt_tree end to end with kmeans="hip" and kmeans="torch", wall
clock, --build-reps times each after one warm-up, with the peak extra device
memory of one build.

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

from exact_search_bench import event_ms                  # noqa: E402
import exact_search_bench                                # noqa: E402
from group_knn_bench import say, summary, peak_extra     # noqa: E402


def versus(args, torch, tag, name, hip, tor):
    hip(), tor()        # warm-up
    say(f"{tag}: {name}: peak extra device memory: hip {peak_extra(torch, hip) / 2**20:.0f} MiB, "
        f"torch {peak_extra(torch, tor) / 2**20:.0f} MiB")
    th, tt = [], []
    for rnd in range(args.rounds):
        h = event_ms(torch, hip, args.reps)
        t = event_ms(torch, tor, args.reps)
        th += h
        tt += t
        say(f"{tag}: {name}: round {rnd}: hip median {statistics.median(h):.2f} ms, torch "
            f"median {statistics.median(t):.2f} ms")
    mh, sh = summary(tag, f"{name} hip", th)
    mt, st = summary(tag, f"{name} torch", tt)
    say(f"{tag}: {name}: torch / hip = {mt / mh:.2f}; torch - hip = {mt - mh:.2f} ms against "
        f"the two spreads combined {sh + st:.2f} ms")


def workload(args, torch, build):
    import sptag_amd
    n, S, K, d = args.n, args.clusters, args.k, 128
    tag = f"f32 d=128 L2 n={n} clusters={S} K={K}"
    dev = torch.device("cuda:0")
    xf = torch.from_numpy(np.random.default_rng(11).standard_normal(
        (n, d), dtype=np.float32)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    perm = torch.randperm(n, generator=gen, device=dev).to(torch.int32)
    sizes = np.full(S, n // S, dtype=np.int32)
    sizes[: n % S] += 1
    starts = (np.cumsum(sizes) - sizes).astype(np.int32)
    ssz = np.minimum(sizes, args.sample).astype(np.int32)
    ncent = np.full(S, K, dtype=np.int32)
    # a cluster's sample is the head of its slice, its centers the first K of it
    centers = torch.stack([xf[perm[s:s + K].long()] for s in starts]).contiguous()
    counts = torch.zeros((S, K), dtype=torch.int32, device=dev)
    cidx = torch.zeros_like(counts)
    cdist = torch.zeros((S, K), device=dev)
    sums = torch.zeros((S, K, d), device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)

    def hip(szs, update):
        torch.cuda.synchronize()
        sptag_amd.kmeans_assign_device(
            xf.data_ptr(), 0, "L2", n, d, perm.data_ptr(), n, starts, szs, ncent,
            centers.data_ptr(), K, None, None, update, lab.data_ptr(), None, counts.data_ptr(),
            cidx.data_ptr(), cdist.data_ptr(), sums.data_ptr() if update else None)
        return lab

    def lloyd_torch():
        out = []
        for s in range(S):
            pts = xf[perm[starts[s]:starts[s] + ssz[s]].long()]
            lb = torch.cdist(pts, centers[s]).argmin(1)
            sm = torch.zeros_like(centers[s])
            sm.index_add_(0, lb, pts)
            out.append((sm, torch.bincount(lb, minlength=K)))
        return out

    def final_torch():
        out = []
        for s in range(S):
            d2 = torch.cdist(xf[perm[starts[s]:starts[s] + sizes[s]].long()], centers[s])
            lb = d2.argmin(1)
            dmask = d2.clone()
            dmask[~torch.nn.functional.one_hot(lb, K).bool()] = torch.finfo(d2.dtype).max
            out.append((lb, dmask.argmin(0), torch.bincount(lb, minlength=K)))
        return out

    hl = hip(ssz, 1)
    c0 = counts[0].cpu().numpy()
    t0 = lloyd_torch()[0][1].cpu().numpy()
    say(f"{tag}: cluster 0 of the Lloyd step: centers whose counts differ between hip and torch: "
        f"{int((c0 != t0).sum())} of {K}")
    del hl
    versus(args, torch, tag, f"lloyd iteration, {int(ssz.sum())} sampled members",
           lambda: hip(ssz, 1), lloyd_torch)
    versus(args, torch, tag, f"final assign, {n} members", lambda: hip(sizes, 0), final_torch)
    del centers, counts, cidx, cdist, sums, lab, perm

    for km in ("hip", "torch"):
        fn = lambda: build.build_bkt_tree(xf, device="cuda:0", kmeans=km)
        ts, tn = fn()       # warm-up
        say(f"{tag}: build_bkt_tree kmeans={km}: {len(tn)} nodes; peak extra device memory "
            f"{peak_extra(torch, fn) / 2**20:.0f} MiB")
        t = []
        for _ in range(args.build_reps):
            torch.cuda.synchronize()
            a = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - a) * 1e3)
        summary(tag, f"build_bkt_tree kmeans={km} wall", t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--k", type=int, default=32)
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
        sys.exit("kmeans_assign_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    workload(args, torch, build)


if __name__ == "__main__":
    main()
