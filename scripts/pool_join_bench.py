#!/usr/bin/env python3
"""Measurements behind profiles/pool_join.txt (one process, one GPU).

n x 128 seeded random f32 rows, L2. build_rng_graph (leaf kNN, join and prune
all "hip") gives the graph and the pools of --cand candidates that a
refine_graph round starts from. Two steps are then timed for all n rows, each
as one whole call of the HIP path against the torch step on the same inputs,
with HIP events on the default stream, alternating for --rounds rounds of
--reps calls after one warm-up each:

  descent  the NN-descent join of one refine_graph round: the pools plus
           hop-2 and sampled reverse neighbours (hop_sample 8 x degree + 16
           new ids a row), distances computed.
             hip    build._pool_join_hip, one launch
             torch  build._exact_l2 + build._merge_candidates in chunks of
                    build._prune_chunk rows, as refine_graph runs them
  tree     one TP-tree merge: the pools plus the 64 leaf neighbours of a fresh
           partition, distances given.
             hip    build._pool_join_hip, one launch
             torch  build._merge_candidates with its own row chunking

Both write to fresh outputs, so every call sees the same pools. The peak extra
device memory of one call of each is recorded, and the answers are compared
first: rows whose id lists differ are counted; the descent ones are not
expected to be equal everywhere (the torch step's distances are (b - a)^2
sums in another order, and its duplicate rule keeps the nearer of pool and new).

Prints plain lines; --out also writes them to a file as they come."""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exact_search_bench import event_ms                  # noqa: E402
import exact_search_bench                                # noqa: E402
from group_knn_bench import say, summary, peak_extra     # noqa: E402


def descent_ids(torch, build, g, hop_sample, r=0):
    """refine_graph's new candidates of round r for every row: hop-2
    neighbours and the sampled reverse edges"""
    n, deg = g.shape
    self_ids = torch.arange(n, device=g.device, dtype=torch.int32)
    rev = torch.full((n, 16), -1, dtype=torch.int32, device=g.device)
    for es, ee in build._chunks(n, max(1, 64_000_000 // deg)):
        srcc = self_ids[es:ee].repeat_interleave(deg)
        dstc = g[es:ee].reshape(-1).long()
        keep = dstc >= 0
        srcc, dstc = srcc[keep], dstc[keep]
        rev[dstc, ((srcc.long() * 2654435761) + r * 97) % 16] = srcc
    out = torch.empty((n, hop_sample * deg + 16), dtype=torch.int32, device=g.device)
    for s, e in build._chunks(n, 65_536):
        nbr = g[s:e, :hop_sample]
        hop2 = g[nbr.clamp(min=0).long()].reshape(e - s, -1)
        hop2 = torch.where((nbr < 0).repeat_interleave(deg, dim=1),
                           torch.full_like(hop2, -1), hop2)
        out[s:e] = torch.cat([hop2, rev[s:e]], dim=1)
    return out


def compare(args, torch, tag, name, hip, tor, inplace_note=""):
    (hi, hd), (ti, td) = hip(), tor()       # warm-up, and the outputs to compare
    both = (hi >= 0) & (ti >= 0)
    say(f"{tag}: {name}: rows whose id lists differ: {int((hi != ti).any(1).sum())} of "
        f"{hi.shape[0]}; valid per row: hip {float((hi >= 0).sum(1).float().mean()):.1f}, torch "
        f"{float((ti >= 0).sum(1).float().mean()):.1f}; largest distance difference where both "
        f"are valid {float((hd - td)[both].abs().max()):.3g}")
    del hi, hd, ti, td, both
    say(f"{tag}: {name}: peak extra device memory: hip {peak_extra(torch, hip) / 2**20:.0f} MiB "
        f"(the outputs{inplace_note}), torch {peak_extra(torch, tor) / 2**20:.0f} MiB")
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
    n, cand = args.n, args.cand
    tag = f"f32 d=128 L2 n={n} cand={cand}"
    xf = torch.from_numpy(np.random.default_rng(11).standard_normal(
        (n, 128), dtype=np.float32)).to("cuda:0")
    g, ids, dst = build.build_rng_graph(xf, degree=args.degree, ntrees=args.trees,
                                        tpt_leaf=args.leaf, cand=cand, device="cuda:0",
                                        leaf_knn="hip", prune="hip", join="hip")
    self_ids = torch.arange(n, device=xf.device, dtype=torch.int32)
    newc = descent_ids(torch, build, g, 8)
    say(f"{tag}: pools with {float((ids >= 0).sum(1).float().mean()):.1f} valid entries a row; "
        f"descent lists of {newc.shape[1]} ids, {float((newc >= 0).sum(1).float().mean()):.1f} "
        f"valid a row")

    def descent_torch():
        oi, od = torch.empty_like(ids), torch.empty_like(dst)
        for s, e in build._chunks(n, build._prune_chunk(cand, 128)):
            newd = build._exact_l2(xf, torch.arange(s, e, device=xf.device), newc[s:e])
            oi[s:e], od[s:e] = build._merge_candidates(ids[s:e], dst[s:e], newc[s:e], newd,
                                                       cand, self_ids[s:e])
        return oi, od
    compare(args, torch, tag, "descent join",
            lambda: build._pool_join_hip(xf, ids, dst, newc, None, cand, self_ids),
            descent_torch, "; none in place, as refine_graph calls it")
    del newc

    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(99)
    perm, starts, counts = build._tpt_leaves(xf, args.leaf, gen)
    tids, tdst = build._leaf_knn_hip(xf, perm, starts, counts, 64)
    compare(args, torch, tag, f"tree merge {cand} + 64",
            lambda: build._pool_join_hip(xf, ids, dst, tids, tdst, cand, self_ids),
            lambda: build._merge_candidates(ids, dst, tids, tdst, cand, self_ids),
            "; none in place, as build_rng_graph calls it")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--leaf", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--cand", type=int, default=256)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        exact_search_bench.OUT = open(args.out, "w")
    import torch
    import sptag_amd
    from sptag_amd import build
    if not sptag_amd.gpu_available():
        sys.exit("pool_join_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    workload(args, torch, build)


if __name__ == "__main__":
    main()
