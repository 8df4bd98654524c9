"""The search planner (sptag_amd/csrc/plan.h) on the CPU: plan_probe.cpp is
compiled with the host compiler and every line it prints is compared with
values worked by hand from the sizing rules as they stood in
search_device_core and sptag_amd_iter_create before the planner existed:

  dpq    = max(mc/16, k)                               WorkSpace.h:268
  vcap   = next_pow2(max(4096, 4*mc + 64*k))           iterator: no 64*k
  ng     = BKT mc/2 + 512, KDT mc + 2048; + 4*k when k > 64;
           SPTAG_AMD_NG_CAP replaces it, at least 256; then min(ng, 30*mc)
  spt    = min(4096, 10*mc)
  lsplit = last index of the levels kept in LDS when the deepest G levels of
           a heap filled to ng go to global memory (G = 0: ng)
  global = 30*mc / 10*mc                               WorkSpace.h:265
  lds    = align16(dim*esz) + 64*4 + 64*4 + k*8 + (dpq+1)*4 + 64 + 256*8
           + (lsplit+1)*8
  lds_ok = lds <= min(device limit, 65536); ng_tail = lds_ok and lsplit < ng
  a heap slab is (cap+1)*8 bytes, the visited table vcap*4
"""
import os
import shutil
import subprocess

from conftest import REPO

# name: (k, mc, dup, del, dpq, vcap, ng, spt, lsplit, gng, gspt, lds, lds_ok,
#        ng_tail, prof, sstride)
BKT_2048 = (10, 2048, 1, 0, 128, 16384, 1536, 4096, 255, 61440, 20480,
            512 + 256 + 256 + 80 + 516 + 64 + 2048 + 2048, 1, 1, 0, 2)
assert BKT_2048[11] == 5780
KDT_512 = (10, 512, 1, 0, 32, 4096, 2560, 4096, 511, 15360, 5120,
           512 + 256 + 256 + 80 + 132 + 64 + 2048 + 4096, 1, 1, 0, 2)
D4096 = 16384 + 256 + 256 + 8192 + 4100 + 64 + 2048     # without the NG heap


def _with(row, **kw):
    names = ("k", "mc", "dup", "del_", "dpq", "vcap", "ng", "spt", "lsplit", "gng",
             "gspt", "lds", "lds_ok", "ng_tail", "prof", "sstride")
    d = dict(zip(names, row))
    d.update(kw)
    return tuple(d[n] for n in names)


PLANS = {
    "bkt_mc2048": BKT_2048,
    # the add path's refine search: k = 501 at MaxCheck 8192
    "bkt_refine": (501, 8192, 0, 1, 512, 65536, 4608 + 2004, 4096, 1023, 245760,
                   81920, 512 + 512 + 4008 + 2052 + 64 + 2048 + 8192, 1, 1, 0, 2),
    # below MaxCheck 18 / 410 the reference's own capacities are the smaller
    "bkt_mc16": (10, 16, 1, 0, 10, 4096, 480, 160, 63, 480, 160,
                 512 + 512 + 80 + 44 + 64 + 2048 + 512, 1, 1, 0, 2),
    "kdt_mc512": KDT_512,
    "cap384_g2": _with(BKT_2048, ng=384, lsplit=127, lds=3732 + 1024),
    "cap100": _with(BKT_2048, ng=256, lsplit=63, lds=3732 + 512),
    "i8_d100": _with(BKT_2048, lds=5780 - 512 + 112),
    "g9": BKT_2048,
    "g_neg": _with(BKT_2048, lsplit=1536, lds=3732 + 1537 * 8, ng_tail=0),
    "d4096_g0": (1024, 8192, 1, 0, 1024, 131072, 4096 + 512 + 4096, 4096, 8704,
                 245760, 81920, D4096 + 8705 * 8, 0, 0, 0, 2),
    "d4096_g3": (1024, 8192, 1, 0, 1024, 131072, 8704, 4096, 2047, 245760, 81920,
                 D4096 + 2048 * 8, 1, 1, 0, 2),
    "small_device": _with(BKT_2048, lds_ok=0, ng_tail=0),
    "bkt_prof": _with(BKT_2048, prof=1, sstride=16),
    "kdt_prof": KDT_512,     # the KDT kernel has no phase clock
}

# name: per-query scratch bytes (visited, gspt0, gng0, gng, gspt)
DETAIL = {
    "bkt_mc2048": (65536, 32776, 12296, 491528, 163848),
    "bkt_refine": (262144, 32776, 6613 * 8, 245761 * 8, 81921 * 8),
    "d4096_g0": (524288, 32776, 0, 245761 * 8, 81921 * 8),
    "bkt_prof": (65536, 32776, 12296, 491528, 163848),
}


def expected_lines():
    out = []
    for name, p in PLANS.items():
        out.append("%s: nq=0 k=%d mc=%d piv=50/4/3 dup=%d del=%d dpq=%d vcap=%d "
                   "ng=%d spt=%d lsplit=%d global=%d/%d lds=%d lds_ok=%d "
                   "ng_tail=%d prof=%d sstride=%d" % ((name,) + p))
        if name in DETAIL:
            out.append("%s scratch: visited=%d gspt0=%d gng0=%d gng=%d gspt=%d"
                       % ((name,) + DETAIL[name]))
    out.append("iter_mc512: ng=15360 spt=5120 dpq_alloc=1024 vcap=4096")
    out.append("iter_mc8192: ng=245760 spt=81920 dpq_alloc=1024 vcap=32768")
    out.append("ref caps mc1: 30 10")
    return out


def test_planner_matches_hand_worked_values(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan_probe")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "sptag_amd", "csrc"),
                    os.path.join(REPO, "tests", "plan_probe.cpp"), "-o", exe],
                   check=True)
    got = subprocess.run([exe], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    want = expected_lines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)

