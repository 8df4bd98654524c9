#!/usr/bin/env python3
"""Measurements behind profiles/rng_prune.txt (one process, one GPU).

f32: n x 128 seeded random rows, L2. The candidate pools are the ones
build_rng_graph prunes: --trees TP-tree partitions at --leaf, leaf kNN by the
grouped-kNN kernels, merged to --cand candidates, plus the bridges of the last
partition (the pool is widened by them, not truncated). Two whole calls over
the same pools for all n rows, degree 32, timed with HIP events on the default
stream, alternating for --rounds rounds of --reps calls after one warm-up
each:

  hip     build._rng_prune_hip: sptag_amd.rng_prune_device on the vectors'
          own device buffer, one launch for all rows
  torch   build._rng_prune, the [B, C, C] pairwise tensor and the column loop,
          in chunks of build._prune_chunk rows (the parent's path)

and the peak extra device memory of one call of each. The answers are
compared first: rows whose id lists differ are counted; they are not expected
to be equal everywhere (the torch step compares approximate distances).

int8: n x 100 rows, cosine, pools of 264 nearest of a random 4096-row window
by brute force in torch, through the handle form AnnIndex.RngPrune (host
pointers: its span includes the copies of the lists in and of the graph out).

Prints plain lines; --out also writes them to a file as they come."""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exact_search_bench import event_ms, make_index      # noqa: E402
import exact_search_bench                                # noqa: E402
from group_knn_bench import say, summary, peak_extra     # noqa: E402


def f32_pools(args, torch, build, xf):
    """build_rng_graph's pools for all rows: (ids int32 [n, C], dists f32)"""
    n = xf.shape[0]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(2016 + 77)
    self_ids = torch.arange(n, device=xf.device, dtype=torch.int32)
    kper = min(max(33, args.cand // max(args.trees, 1)), 64)
    ids = dst = None
    for _ in range(args.trees):
        perm, starts, counts = build._tpt_leaves(xf, args.leaf, gen)
        tids, tdst = build._leaf_knn_hip(xf, perm, starts, counts, kper)
        if ids is None:
            ids, dst = build._merge_candidates(tids, tdst, tids[:, :0], tdst[:, :0],
                                               args.cand, self_ids)
        else:
            ids, dst = build._merge_candidates(ids, dst, tids, tdst, args.cand, self_ids,
                                               out=(ids, dst))
    bridge = build._bridge_ids(xf, perm, counts)
    wide = args.cand + bridge.shape[1]
    wi = torch.empty((n, wide), dtype=torch.int32, device=xf.device)
    wd = torch.empty((n, wide), dtype=torch.float32, device=xf.device)
    for s, e in build._chunks(n, 65_536):
        bd = build._exact_l2(xf, torch.arange(s, e, device=xf.device), bridge[s:e].long())
        wi[s:e], wd[s:e] = build._merge_candidates(ids[s:e], dst[s:e], bridge[s:e], bd, wide,
                                                   self_ids[s:e])
    return wi, wd


def f32_workload(args, torch, build):
    tag = f"f32 d=128 L2 n={args.n} degree={args.degree}"
    xf = torch.from_numpy(np.random.default_rng(11).standard_normal(
        (args.n, 128), dtype=np.float32)).to("cuda:0")
    cid, cdd = f32_pools(args, torch, build, xf)
    nodes = torch.arange(args.n, device=xf.device, dtype=torch.int32)
    say(f"{tag}: pools of {cid.shape[1]} candidates ({args.cand} + bridges), "
        f"{float((cid >= 0).sum(1).float().mean()):.1f} valid per row")
    hip = lambda: build._rng_prune_hip(xf, cid, cdd, args.degree, 1.0, nodes=nodes)
    tor = lambda: build._rng_prune(xf, cid, cdd, args.degree, 1.0)
    hg, tg = hip(), tor()       # warm-up, and the outputs to compare
    say(f"{tag}: rows whose id lists differ: {int((hg != tg).any(1).sum())} of {args.n}; "
        f"mean accepted per row: hip {float((hg >= 0).sum(1).float().mean()):.2f}, torch "
        f"{float((tg >= 0).sum(1).float().mean()):.2f}; rows at the cap "
        f"{int((hg[:, -1] >= 0).sum())}")
    del hg, tg
    say(f"{tag}: peak extra device memory: hip {peak_extra(torch, hip) / 2**20:.0f} MiB "
        f"(the [n, degree] output), torch {peak_extra(torch, tor) / 2**20:.0f} MiB")
    th, tt = [], []
    for rnd in range(args.rounds):
        h = event_ms(torch, hip, args.reps)
        t = event_ms(torch, tor, args.reps)
        th += h
        tt += t
        say(f"{tag}: round {rnd}: hip median {statistics.median(h):.2f} ms, torch median "
            f"{statistics.median(t):.2f} ms")
    mh, sh = summary(tag, "hip", th)
    mt, st = summary(tag, "torch", tt)
    say(f"{tag}: torch / hip = {mt / mh:.2f}; torch - hip = {mt - mh:.2f} ms against the "
        f"two spreads combined {sh + st:.2f} ms")


def i8_workload(args, torch, sptag_amd):
    n, C = args.n, 264
    tag = f"i8 d=100 Cosine n={n} C={C} degree={args.degree}"
    ix = make_index(sptag_amd, "i8", "Cosine", n, 100, 11)
    x = torch.from_numpy(np.random.default_rng(11).integers(
        -127, 128, (n, 100), dtype=np.int8)).to("cuda:0").float()
    ids = torch.empty((n, C), dtype=torch.int32, device="cuda:0")
    dst = torch.empty((n, C), dtype=torch.float32, device="cuda:0")
    for s in range(0, n, 4096):         # candidates from the row's own window
        w = x[s:s + 4096]
        dd = 16129.0 - w @ w.T
        dd.fill_diagonal_(float("inf"))
        v, i = torch.topk(dd, min(C, w.shape[0] - 1), dim=1, largest=False)
        ids[s:s + 4096, :i.shape[1]] = (i + s).int()
        dst[s:s + 4096, :i.shape[1]] = v
        ids[s:s + 4096, i.shape[1]:] = -1
        dst[s:s + 4096, i.shape[1]:] = float("inf")
    nodes = np.arange(n, dtype=np.int32)
    ids, dst = ids.cpu().numpy(), dst.cpu().numpy()
    fn = lambda: ix.RngPrune(nodes, ids, dst, args.degree)
    g = fn()
    say(f"{tag}: mean accepted per row {float((g >= 0).sum(1).mean()):.2f}")
    summary(tag, "hip, handle form with its copies", event_ms(torch, fn, args.rounds * args.reps))


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
        sys.exit("rng_prune_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    f32_workload(args, torch, build)
    i8_workload(args, torch, sptag_amd)


if __name__ == "__main__":
    main()
