"""The frontier and tree heaps of the search kernels are the reference's
binary min-heap (inc/Core/Common/Heap.h) in two forms: lane 0 alone
(ndheap_insert, ndheap_pop) and the whole wave (ndheap_insert_wave,
ndheap_pop_wave). The probe entry point runs one script of inserts and pops
through both; this file restates Heap.h in Python and compares each form with
it bit for bit: every popped (node, distance), the final count, the overflow
flag and the array [1..count].

Sizes are the smallest at which a rule can go wrong: 1, 2, 3 entries; 7 and 8
(a level fills, the next starts); 63, 64, 65 (the edge of the pop's first
6-level block); 100 and 300; 2047 and 2048 (a second block that ends inside a
level); 4097 (13 levels, a third block). The LDS tier holds entries
[0..lsplit]: none (the iterator's all-global heaps) and 1, 3, 63, 255, so that
ancestor paths and blocks straddle it. Keys come from four distinct distances
(most comparisons are ties) and from random floats; node ids are distinct.
With cap == ref_cap the heap is driven full and inserts take the replace
path; with cap < ref_cap the insert that does not fit raises the flag.
"""
import ctypes

import numpy as np
import pytest

import sptag_amd

pytestmark = pytest.mark.gpu

MAXDIST = np.float32(np.finfo(np.float32).max) / np.float32(10)

CAPS = [1, 2, 3, 7, 8, 63, 64, 65, 100, 300, 2047, 2048, 4097]
LSPLITS = [0, 1, 3, 63, 255]


class PyHeap:
    """Heap.h:14-105 on (node, distance) pairs ordered by distance, plus the
    kernels' overflow rule for a buffer smaller than the reference's."""

    def __init__(self, cap, ref_cap):
        self.cap, self.ref_cap = cap, ref_cap
        self.a = [(-1, MAXDIST)] + [None] * cap
        self.count = 0
        self.oflow = 0
        self.replaced = 0
        self.lastlevel = 1 << (cap.bit_length() - 1)

    def insert(self, node, d):
        a = self.a
        if self.count == self.cap:
            if self.cap < self.ref_cap:
                self.oflow = 1
                return
            maxi = self.lastlevel
            for i in range(self.lastlevel + 1, self.cap + 1):
                if a[maxi][1] < a[i][1]:
                    maxi = i
            if d > a[maxi][1]:
                return
            loc = maxi
            self.replaced += 1
        else:
            self.count += 1
            loc = self.count
        par = loc >> 1
        while par > 0 and d < a[par][1]:
            a[loc] = a[par]
            loc = par
            par >>= 1
        a[loc] = (node, d)

    def pop(self):
        a = self.a
        if self.count == 0:
            return a[0]
        a[1], a[self.count] = a[self.count], a[1]
        self.count -= 1
        parent, nxt = 1, 2
        while nxt < self.count:
            if a[nxt][1] > a[nxt + 1][1]:
                nxt += 1
            if a[nxt][1] < a[parent][1]:
                a[parent], a[nxt] = a[nxt], a[parent]
                parent = nxt
                nxt <<= 1
            else:
                break
        else:
            if nxt == self.count and a[nxt][1] < a[parent][1]:
                a[parent], a[nxt] = a[nxt], a[parent]
        return a[self.count + 1]


def make_script(cap, full, ties, seed):
    """(ops, nodes, dists): fill the heap (a pop now and then), a few hundred
    mixed operations around the capacity, then pops down to empty and two
    past it. `full` keeps inserting at the capacity."""
    rng = np.random.default_rng(seed)
    ops = []
    # fill to the capacity, one pop in ten
    n = 0
    while n < cap:
        if n > 0 and rng.random() < 0.1:
            ops.append(0)
            n -= 1
        else:
            ops.append(1)
            n += 1
    ops.append(1)       # the heap is full: this one replaces or overflows
    # at the capacity: more inserts than pops when the heap is to stay full
    for _ in range(300):
        ops.append(1 if rng.random() < (0.7 if full else 0.5) else 0)
    if full:
        ops += [1] * 40
    ops += [0] * (min(cap, 400) + 2)
    # finish with inserts, so that the array compared at the end is not empty
    ops += [1] * min(cap, 200)
    ops = np.array(ops, dtype=np.int32)
    nodes = rng.permutation(len(ops)).astype(np.int32) + 7
    if ties:
        dists = rng.choice(np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32), len(ops))
    else:
        dists = rng.random(len(ops), dtype=np.float32)
    return ops, nodes, dists.astype(np.float32)


_models = {}


def model(cap, full, ties):
    """Script and the Python heap's answer; computed once per script."""
    key = (cap, full, ties)
    if key not in _models:
        ops, nodes, dists = make_script(cap, full, ties, seed=cap * 4 + full * 2 + ties)
        h = PyHeap(cap, cap if full else cap + 5)
        pops = []
        for op, node, d in zip(ops, nodes, dists):
            if op:
                h.insert(int(node), d)
            else:
                pops.append(h.pop())
        _models[key] = (ops, nodes, dists, h, pops)
    return _models[key]


def run_probe(cap, ref_cap, lsplit, ops, nodes, dists):
    lib = sptag_amd.load_library()
    fn = lib.sptagamd_dbg_heap_probe
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 6
    nops = len(ops)
    heaps = np.zeros((2, cap + 1, 2), dtype=np.int32)
    pops = np.zeros((2, nops, 2), dtype=np.int32)
    final = np.zeros((2, 2), dtype=np.int32)
    rc = fn(0, cap, ref_cap, lsplit, nops, ops.ctypes.data, nodes.ctypes.data,
            dists.ctypes.data, heaps.ctypes.data, pops.ctypes.data, final.ctypes.data)
    assert rc == 0, f"heap probe failed: {rc}"
    return heaps, pops, final


def bits(d):
    return int(np.float32(d).view(np.uint32))


@pytest.mark.parametrize("lsplit", LSPLITS)
@pytest.mark.parametrize("cap", CAPS)
def test_heap_forms_match_heap_h(cap, lsplit):
    for full in (True, False):
        for ties in (True, False):
            ops, nodes, dists, h, ref_pops = model(cap, full, ties)
            tag = f"cap={cap} lsplit={lsplit} full={full} ties={ties}"
            if full:
                assert h.replaced >= 1, f"{tag}: the script never took the replace branch"
                assert h.oflow == 0
            else:
                assert h.oflow == 1, f"{tag}: the script never overflowed"
            heaps, pops, final = run_probe(cap, h.cap if full else h.ref_cap, lsplit,
                                           ops, nodes, dists)
            want_pops = np.array([[n, bits(d)] for n, d in ref_pops], dtype=np.int64)
            want_heap = np.array([[n, bits(d)] for n, d in h.a[1:h.count + 1]],
                                 dtype=np.int64).reshape(-1, 2)
            for form, name in enumerate(("serial", "wave-wide")):
                got = pops[form][ops == 0].view(np.uint32).astype(np.int64)
                got[:, 0] = pops[form][ops == 0][:, 0]
                np.testing.assert_array_equal(got, want_pops, err_msg=f"{tag} {name} pops")
                assert final[form, 0] == h.count, f"{tag} {name} count"
                assert final[form, 1] == h.oflow, f"{tag} {name} overflow flag"
                arr = heaps[form][1:h.count + 1]
                got = arr.view(np.uint32).astype(np.int64)
                got[:, 0] = arr[:, 0]
                np.testing.assert_array_equal(got, want_heap, err_msg=f"{tag} {name} array")
