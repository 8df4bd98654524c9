#!/usr/bin/env python3
"""Measurements behind profiles/group_knn.txt (one process, one GPU).

f32: n x 128 seeded random rows, one TP-tree partition of the index builder
(build._tpt_leaves at --leaf), k = 64 (the builder's kper ceiling). Two
whole calls over the same partition, timed with HIP events on the default
stream, alternating for --rounds rounds of --reps calls after one warm-up
each:

  hip     build._leaf_knn_hip: sptag_amd.group_knn_device on the vectors'
          own device buffer, plus the builder's padding conventions, once
          for every --selection given ("stream", "sort", "auto"), all in the
          same rounds; their outputs are compared for equal bytes first
  torch   build._leaf_knn, the padded [B, m, m] GEMM-identity + topk step

and the peak extra device memory of one call of each
(torch.cuda.max_memory_allocated above the level before the call; the tile
table of the hip call, 12 bytes per 32 members, is allocated by the library
and is not in torch's count). The two answers are compared first: ids that
differ are counted, they are not expected to be equal (the torch step ranks
by an approximate distance and breaks ties by position).

int8: n x 100 rows, cosine, the same kind of partition, through the handle
form AnnIndex.GroupKnn (host pointers: its span includes the copy of the
members in and of n*k results out).

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


def say(*a):
    exact_search_bench.say(*a)


def summary(tag, name, t):
    m = statistics.median(t)
    say(f"{tag}: {name} median {m:.2f} ms (min {min(t):.2f}, max {max(t):.2f}, "
        f"{len(t)} calls), spread {(max(t) - min(t)) / m * 100:.1f}% of median")
    return m, max(t) - min(t)


def peak_extra(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def f32_workload(args, torch, build):
    tag = f"f32 d=128 L2 n={args.n} leaf={args.leaf} k={args.k}"
    xf = torch.from_numpy(np.random.default_rng(11).standard_normal(
        (args.n, 128), dtype=np.float32)).to("cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(2016)
    perm, starts, counts = build._tpt_leaves(xf, args.leaf, gen)
    say(f"{tag}: {counts.numel()} leaves of {int(counts.min())}..{int(counts.max())} rows")
    hips = {s: (lambda s=s: build._leaf_knn_hip(xf, perm, starts, counts, args.k, s))
            for s in args.selection}
    hip = hips[args.selection[0]]
    tor = lambda: build._leaf_knn(xf, perm, starts, counts, args.k)
    hv, hd = hip()          # warm-up, and the outputs to compare
    for s in args.selection[1:]:
        sv, sd = hips[s]()
        say(f"{tag}: {s} equals {args.selection[0]} in every byte: "
            f"{bool((sv == hv).all() and (sd.view(torch.int32) == hd.view(torch.int32)).all())}")
        del sv, sd
    tv, td = tor()
    say(f"{tag}: rows whose id lists differ: {int((hv != tv).any(1).sum())} of {args.n}; "
        f"largest relative distance difference "
        f"{float(((hd - td).abs() / hd.clamp(min=1e-30)).max()):.2e}")
    del hv, hd, tv, td
    say(f"{tag}: peak extra device memory: hip {peak_extra(torch, hip) / 2**20:.0f} MiB "
        f"(the [n, k] outputs and the int32 members), torch "
        f"{peak_extra(torch, tor) / 2**20:.0f} MiB")
    th, tt = {s: [] for s in hips}, []
    for rnd in range(args.rounds):
        line = []
        for s, fn in hips.items():
            h = event_ms(torch, fn, args.reps)
            th[s] += h
            line.append(f"hip {s} median {statistics.median(h):.2f} ms")
        t = event_ms(torch, tor, args.reps)
        tt += t
        say(f"{tag}: round {rnd}: {', '.join(line)}, torch median "
            f"{statistics.median(t):.2f} ms")
    mt, st = summary(tag, "torch", tt)
    for s in hips:
        mh, sh = summary(tag, f"hip {s}", th[s])
        say(f"{tag}: torch / hip {s} = {mt / mh:.2f}; torch - hip {s} = {mt - mh:.2f} ms "
            f"against the two spreads combined {sh + st:.2f} ms")


def i8_workload(args, torch, sptag_amd, build):
    tag = f"i8 d=100 Cosine n={args.n} leaf={args.leaf} k={args.k}"
    ix = make_index(sptag_amd, "i8", "Cosine", args.n, 100, 11)
    x = np.random.default_rng(11).integers(-127, 128, (args.n, 100), dtype=np.int8)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(2016)
    perm, starts, counts = build._tpt_leaves(torch.from_numpy(x).to("cuda:0").float(),
                                             args.leaf, gen)
    perm, starts, counts = (a.cpu().numpy().astype(np.int32) for a in (perm, starts, counts))
    for s in args.selection:
        fn = lambda: ix.GroupKnn(perm, starts, counts, args.k, selection=s)
        fn()
        summary(tag, f"hip {s}, handle form with its copies",
                event_ms(torch, fn, args.rounds * args.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--leaf", type=int, default=1000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--selection", nargs="+", default=["stream"],
                    choices=["stream", "sort", "auto"])
    ap.add_argument("--skip-i8", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        exact_search_bench.OUT = open(args.out, "w")
    import torch
    import sptag_amd
    from sptag_amd import build
    if not sptag_amd.gpu_available():
        sys.exit("group_knn_bench.py needs a HIP device")
    say(f"device: {torch.cuda.get_device_name(0)}")
    f32_workload(args, torch, build)
    if not args.skip_i8:
        i8_workload(args, torch, sptag_amd, build)


if __name__ == "__main__":
    main()
