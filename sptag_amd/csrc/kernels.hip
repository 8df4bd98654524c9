/* sptag_amd GPU kernels — gfx950 (MI355X, CDNA4) native.
 *
 * Batched BKT best-first graph search: one query per 64-thread workgroup
 * (one wave64). The traversal replicates the reference CPU algorithm
 * decision-for-decision (citations to /root/reference/AnnService):
 *   - seed phase: BKTree::InitSearchTrees / SearchTrees (BKTree.h:697,772)
 *   - traversal:  BKT::Index<T>::Search<> loop (BKTIndex.cpp:272-352)
 *   - frontier:   Heap<NodeDistPair> semantics (Heap.h:14-110)
 *   - pruning:    DistPriorityQueue (WorkSpace.h:167-225)
 *   - top-k:      QueryResultSet AddPoint/SortResult (QueryResultSet.h:31)
 * Distances reproduce the reference binary's float summation order
 * (AVX512 16-lane chunking with fused mul+add; exact integer math for int8),
 * so int8 results are bit-exact and float results are bit-exact against
 * the oracle/_ref build (see oracle/sptag_oracle.c).
 *
 * Division of labor inside the wave:
 *   - frontier/tree heaps: the reference's binary heap, comparison for
 *     comparison (pop order on equal keys is part of the parity contract),
 *     evaluated by the whole wave in the batched search (ndheap_*_wave) and
 *     by lane 0 where inserts interleave with other serial work; result-set
 *     mutation -> lane 0, state in LDS;
 *   - adjacency row load: lanes 0..deg-1, one coalesced 128B line;
 *   - visited-set: per-query open-addressing table in GLOBAL memory
 *     (512KB-class tables do not fit LDS at MaxCheck 8192 — SURVEY.md §7),
 *     probed in parallel with atomicCAS (set semantics only, order-free);
 *   - distances: 16-lane groups, 4 candidates in flight per wave.
 *
 * HEAPS_IN_LDS=true keeps the top levels of the NG/SPT frontier heaps in LDS
 * (tails in per-query global slabs) with reduced
 * capacities; if a heap would exceed its reduced capacity while the
 * reference's (30*maxCheck / 10*maxCheck, WorkSpace.h:265) would not, the
 * query sets an overflow flag and the host reruns it with the global-memory
 * variant at full reference capacities — never a silent semantic change.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"

namespace sptag_amd {

#define DEV __device__ __forceinline__

#ifndef SPTAG_LB_WAVES
#define SPTAG_LB_WAVES 1   /* min waves/SIMD hint; raise to cap VGPRs */
#endif
#ifndef SPTAG_WAVE_POP
#define SPTAG_WAVE_POP 1   /* 0: serial frontier/tree pops (measurement builds) */
#endif
/* Loads that depend on nothing but the node a pop is about to return, issued
 * ahead of that pop (peek_frontier). Bit mask, so that measurement builds can
 * take the parts apart: 1 graph row, 2 tree triple. (4, the first chunk of a
 * tree node's children's center ids, issued once the triple is in, was built
 * and lost to the build without it: profiles/pop_ahead_bench.txt.) Serial
 * pops go without. */
#ifndef SPTAG_POP_AHEAD
#define SPTAG_POP_AHEAD 3
#endif
#if !SPTAG_WAVE_POP
#undef SPTAG_POP_AHEAD
#define SPTAG_POP_AHEAD 0
#endif

static constexpr float MAXDIST = __FLT_MAX__ / 10.0f; /* Common.h:122 */

struct NodeDist { int32_t node; float distance; };
struct QRes { int32_t vid; float dist; };

/* ------------------------------------------------------------------ *
 * serial structures (lane 0 only), exact reference semantics
 * ------------------------------------------------------------------ */

/* 2^floor(log2(size)) — start of the heap's last level (Heap.h:25) */
DEV int heap_lastlevel(int size) { return 1 << (31 - __clz(size)); }

/* Binary min-heap, EXACT Heap.h semantics (pop order on equal keys is part
 * of the parity contract), with TIERED storage: entries with index <=
 * lsplit live in an LDS cache, the tail in `a` (global scratch or LDS).
 * Storage placement never changes semantics — only access latency. The
 * round-1 all-global SPT heap made the seed phase 41.5% of kernel cycles
 * (profiles/r2 phase breakdown): every percolate level was an ~HBM-latency
 * round trip. The hot top levels now stay in LDS. */
enum { SPT_LDS_TIER = SPT_LDS_TIER_H };  /* 8 levels (1..255) + sentinel [0] */

struct HeapRef {
    NodeDist* a;    /* 1-based backing array; [0] = sentinel {-1, MAXDIST} */
    NodeDist* lds;  /* optional LDS cache of [0..lsplit]; null = none */
    int lsplit;
    int cap;        /* this buffer's capacity */
    int ref_cap;    /* the reference's capacity for this heap */
};

DEV NodeDist hget(const HeapRef& h, int i)
{
    /* unsigned index: the global access is base + 32-bit offset */
    return (h.lds && i <= h.lsplit) ? h.lds[(uint32_t)i] : h.a[(uint32_t)i];
}

DEV void hset(const HeapRef& h, int i, NodeDist v)
{
    if (h.lds && i <= h.lsplit) h.lds[(uint32_t)i] = v;
    else h.a[(uint32_t)i] = v;
}

/* Heap.h:38-62 insert (incl. the full-heap last-level replace path). */
DEV void ndheap_insert(HeapRef h, int* count, NodeDist v, int* oflow)
{
    int loc;
    if (*count == h.cap) {
        if (h.cap < h.ref_cap) { *oflow = 1; return; }
        int lastlevel = heap_lastlevel(h.cap);
        int maxi = lastlevel;
        float maxd = hget(h, maxi).distance;
        for (int i = lastlevel + 1; i <= h.cap; i++) {
            float di = hget(h, i).distance;
            if (maxd < di) { maxi = i; maxd = di; }
        }
        if (v.distance > maxd) return;
        loc = maxi;
    } else {
        loc = ++(*count);
    }
    int par = loc >> 1;
    while (par > 0) {
        NodeDist p = hget(h, par);
        if (!(v.distance < p.distance)) break;
        hset(h, loc, p);
        loc = par;
        par >>= 1;
    }
    hset(h, loc, v);
}

/* Heap.h:90-105 heapify + :74-82 pop. The sinking element is the original
 * root value throughout (the reference swaps it level by level), so it is
 * carried in a register instead of re-read. */
DEV void ndheap_heapify(HeapRef h, int count)
{
    int parent = 1, next = 2;
    if (next > count) return;
    NodeDist pv = hget(h, parent);
    while (next < count) {
        NodeDist nv = hget(h, next);
        NodeDist nv2 = hget(h, next + 1);
        if (nv.distance > nv2.distance) { next++; nv = nv2; }
        if (nv.distance < pv.distance) {
            hset(h, parent, nv);
            hset(h, next, pv);
            parent = next;
            next <<= 1;
        } else {
            return;
        }
    }
    if (next == count) {
        NodeDist nv = hget(h, next);
        if (nv.distance < pv.distance) {
            hset(h, parent, nv);
            hset(h, next, pv);
        }
    }
}

DEV NodeDist ndheap_pop(HeapRef h, int* count)
{
    if (*count == 0) return hget(h, 0);
    NodeDist top = hget(h, 1);
    hset(h, 1, hget(h, *count));
    /* the vacated slot beyond count is dead until the next insert writes
     * it (Heap.h swaps the old top there; nothing ever reads it) */
    (*count)--;
    ndheap_heapify(h, *count);
    return top;
}

DEV NodeDist ndheap_top(HeapRef h, int count) { return count == 0 ? hget(h, 0) : hget(h, 1); }

/* ------------------------------------------------------------------ *
 * the same heap, evaluated by the whole wave: same comparisons on the
 * same array, so the array after every operation is the serial one's
 * ------------------------------------------------------------------ */

/* v broadcast from lane l (wave-uniform l) */
DEV float lane_bcast(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

DEV NodeDist lane_bcast(NodeDist v, int l)
{
    return NodeDist{__builtin_amdgcn_readlane(v.node, l), lane_bcast(v.distance, l)};
}

/* Orders one wave-wide heap operation against the next, which reads what
 * this one wrote through other lanes, in LDS or in the global tail. A block
 * is exactly one wave, and a wave's LDS operations, and its vector memory
 * operations, are each carried out in the order they were issued (AMDGPU
 * memory model: a wavefront-scope release/acquire needs no wait and no
 * cache action on gfx9xx; an index lives in one of the two storages for
 * good). What the fence has to stop is the compiler moving or forwarding
 * accesses across it, so the stores of an insert are not waited for. */
DEV void heap_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

/* ndheap_insert by all 64 lanes; v and count are wave-uniform. The ancestors
 * of the slot are loc>>1, loc>>2, .., 1, known before the first comparison;
 * the serial loop passes those v is strictly below, moving each down one
 * step, and stops at the first it is not. No ancestor is written before it
 * is read, so lane j reads ancestor j+1, a ballot finds the stop level, and
 * lane j writes level j: its ancestor below the stop, v at it. */
DEV void ndheap_insert_wave(HeapRef h, int& count, NodeDist v, int* oflow)
{
    const int lane = threadIdx.x;
    int loc;
    if (count == h.cap) {
        if (h.cap < h.ref_cap) {
            if (lane == 0) *oflow = 1;
            return;
        }
        /* only where a heap sits at the reference's capacity: lane 0 scans */
        int maxi = 0;
        float maxd = 0.0f;
        if (lane == 0) {
            int lastlevel = heap_lastlevel(h.cap);
            maxi = lastlevel;
            maxd = hget(h, maxi).distance;
            for (int i = lastlevel + 1; i <= h.cap; i++) {
                float di = hget(h, i).distance;
                if (maxd < di) { maxi = i; maxd = di; }
            }
        }
        maxi = __builtin_amdgcn_readfirstlane(maxi);
        maxd = lane_bcast(maxd, 0);
        if (v.distance > maxd) return;
        loc = maxi;
    } else {
        loc = ++count;
    }
    const int nanc = 31 - __clz(loc);       /* ancestors of loc; < 32 */
    NodeDist p = v;
    bool below = false;
    if (lane < nanc) {
        p = hget(h, loc >> (lane + 1));
        below = v.distance < p.distance;
    }
    const int stop = __builtin_ctzll(__ballot(!below));   /* <= nanc */
    if (lane <= stop) hset(h, loc >> lane, lane == stop ? v : p);
    heap_fence();
}

/* ndheap_pop by all 64 lanes; count is wave-uniform, the old top comes back
 * on every lane. The sinking value (the old last entry) follows the
 * smaller-child path, left on ties, and stops at the first child that is not
 * strictly below it; children are read before anything under them is
 * written. The wave loads the path's surroundings a block at a time: lane l
 * >= 2 holds the descendant of the block's root r whose index relative to r
 * is l (five levels, 62 entries; lanes past the count hold nothing), the
 * walk inside the block runs on wave-uniform indexes with readlane, every
 * entry on the path is then written to its parent's index by the lane that
 * holds it, and lane 0 writes the sunk value where the walk stopped. The
 * first block also brings the old top (lane 1) and the old last entry
 * (lane 0) in the same read. */
DEV NodeDist ndheap_pop_wave(HeapRef h, int& count)
{
    const int lane = threadIdx.x;
    if (count == 0) return hget(h, 0);
    const uint32_t n = (uint32_t)count - 1;      /* entries left */
    /* lane l >= 1 is `off` entries into level `d` under the block's root */
    const int d = lane ? 31 - __clz(lane) : 0;
    const int off = lane - (1 << d);
    uint32_t r = 1;
    uint32_t gi = lane == 0 ? (uint32_t)count : (r << d) + off;
    NodeDist val{0, 0.0f};
    if (lane <= 1 || gi <= n) val = hget(h, (int)gi);
    const NodeDist pv = lane_bcast(val, 0);
    const NodeDist top = lane_bcast(val, 1);
    /* the vacated slot beyond count is dead until the next insert writes it */
    count = (int)n;
    if (n == 0) return top;
    for (;;) {
        int p = 1;                  /* relative index the sinking value is at */
        uint64_t path = 0;          /* relative indexes that move up one level */
        bool stopped = false;
#pragma unroll
        for (int lvl = 1; lvl <= 5; lvl++) {
            int cr = p << 1;
            uint32_t gc = (r << lvl) + (uint32_t)(cr - (1 << lvl));
            if (gc > n) { stopped = true; break; }
            NodeDist nv = lane_bcast(val, cr);
            if (gc < n) {
                NodeDist nv2 = lane_bcast(val, cr + 1);
                if (nv.distance > nv2.distance) { cr++; nv = nv2; }
            }
            if (!(nv.distance < pv.distance)) { stopped = true; break; }
            path |= 1ull << cr;
            p = cr;
        }
        const int dp = 31 - __clz(p);
        const uint32_t gp = (r << dp) + (uint32_t)(p - (1 << dp));
        const bool onpath = (path >> lane) & 1;
        if (onpath || (stopped && lane == 0))
            hset(h, (int)(onpath ? gi >> 1 : gp), onpath ? val : pv);
        if (stopped) break;
        /* the next block is strictly below everything written so far */
        r = gp;
        gi = (r << d) + off;
        if (lane >= 2 && gi <= n) val = hget(h, (int)gi);
    }
    heap_fence();
    return top;
}

/* DistPriorityQueue (WorkSpace.h:167-225): 1-based bounded float max-heap
 * seeded with MaxDist; len starts at 1. */
DEV int dpq_insert(float* a, int* len, int cap, float dist)
{
    if (dist > a[1]) return 0;
    if (*len == cap) {
        a[1] = dist;
        int parent = 1, next = 2;
        while (next < *len) {
            if (a[next] < a[next + 1]) next++;
            if (a[next] > a[parent]) {
                float t = a[parent]; a[parent] = a[next]; a[next] = t;
                parent = next;
                next <<= 1;
            } else break;
        }
        if (next == *len && a[next] > a[parent]) {
            float t = a[parent]; a[parent] = a[next]; a[next] = t;
        }
    } else {
        int next = ++(*len), parent = next >> 1;
        while (parent > 0 && dist > a[parent]) {
            a[next] = a[parent];
            next = parent;
            parent >>= 1;
        }
        a[next] = dist;
    }
    return 1;
}

/* DistPriorityQueue (WorkSpace.h:167-225) for one whole adjacency row, wave-
 * wide. Only the queue's kept multiset and its maximum are observable, so
 * the batched search keeps it as `cap` floats in LDS, SORTED ascending, with
 * dmax == dpq[cap-1] replicated in a register. Unfilled slots hold MaxDist:
 * a queue of len < cap with its MaxDist seed behaves exactly like a full one
 * padded with MaxDist (an append is a replace of one MaxDist, and the
 * maximum is MaxDist either way), so there is no length.
 *
 * The reference visits candidates r = 0..ncand-1 in row order: if
 * !(d_r > max(S_r)) it replaces one maximum of S_r by d_r and NG-inserts r.
 * By induction S_r is the cap smallest of U_r = S0 + {accepted j < r}, so
 * max(S_r) is U_r's cap-th smallest and
 *     accept_r  <=>  #{x in U_r : x < d_r} < cap.
 * A rejected j < r has d_j > max(S_j) >= max(S_r): it is never strictly
 * below an accepted d_r, and counting it for an r that is rejected anyway
 * only raises a count already >= cap. So the count may run over S0 and ALL
 * earlier candidates, which makes it a function of S0 and the row alone:
 *     accept_r  <=>  #{x in S0 : x < d_r} + #{j < r : d_j < d_r} < cap.
 * The strict `<` is `dist > a[1] -> reject` on ties. d_r > dmax0 implies
 * cap elements of S0 below d_r; that gate only skips work.
 *
 * Lane r holds d_r (`dv`, lanes >= ncand unused). Returns the accept mask
 * and leaves the cap smallest of S0 + accepted in dpq, merged by rank: ties
 * put accepted before S0 and lower lane / lower slot first, so S0 slot i
 * moves to i + #{a : d_a <= x_i} and accepted a to #{x in S0 : x < d_a} +
 * #{a' before a}; ranks >= cap fall out. Slots only move up, by at most
 * popc(acc) <= 64, so 64-slot chunks are rewritten in place top down, and
 * the accepted, whose ranks may lie in a chunk not read yet, go in last. */
DEV uint64_t dpq_accept_row(float* dpq, int cap, int ncand, float dv, float& dmax)
{
    const int lane = threadIdx.x;
    const uint64_t gate = __ballot(lane < ncand && !(dv > dmax));
    if (!gate) return 0;

    int below_row = 0;      /* #{j < lane : d_j < dv} */
    for (uint64_t m = gate; m; m &= m - 1) {
        int j = __builtin_ctzll(m);
        below_row += (j < lane && lane_bcast(dv, j) < dv);
    }
    int below_set = 0;      /* #{x in S0 : x < dv} */
    for (int base = 0; base < cap; base += 64) {
        float x = base + lane < cap ? dpq[base + lane] : MAXDIST;
        for (uint64_t m = gate; m; m &= m - 1) {
            int r = __builtin_ctzll(m);
            int n = __popcll(__ballot(x < lane_bcast(dv, r)));
            if (lane == r) below_set += n;
        }
    }
    const uint64_t acc = __ballot(((gate >> lane) & 1) && below_set + below_row < cap);
    if (!acc) return 0;

    int ra = below_set;     /* rank of this lane's accepted candidate */
    for (uint64_t m = acc; m; m &= m - 1) {
        int a = __builtin_ctzll(m);
        float da = lane_bcast(dv, a);
        ra += (da < dv || (da == dv && a < lane));
    }
    for (int base = (cap - 1) & ~63; base >= 0; base -= 64) {
        const int i = base + lane;
        float x = i < cap ? dpq[i] : MAXDIST;
        int rx = i;
        for (uint64_t m = acc; m; m &= m - 1)
            rx += (lane_bcast(dv, __builtin_ctzll(m)) <= x);
        /* sorted: a chunk that stays put is below every accepted value,
         * and so is everything under it */
        if (!__ballot(i < cap && rx != i)) break;
        __syncthreads();
        if (i < cap && rx < cap) dpq[rx] = x;
    }
    __syncthreads();
    if (((acc >> lane) & 1) && ra < cap) dpq[ra] = dv;
    __syncthreads();
    dmax = dpq[cap - 1];
    return acc;
}

/* QueryResultSet (QueryResultSet.h:17-120): 0-based k-entry max-heap on
 * (dist, vid). */
DEV int qres_lt(QRes x, QRes y)
{
    return (x.dist < y.dist) || (x.dist == y.dist && x.vid < y.vid);
}

DEV void qrs_heapify(QRes* r, int count)
{
    int parent = 0, next = 1, maxidx = count - 1;
    while (next < maxidx) {
        if (qres_lt(r[next], r[next + 1])) next++;
        if (qres_lt(r[parent], r[next])) {
            QRes t = r[next]; r[next] = r[parent]; r[parent] = t;
            parent = next;
            next = (parent << 1) + 1;
        } else break;
    }
    if (next == maxidx && qres_lt(r[parent], r[next])) {
        QRes t = r[next]; r[next] = r[parent]; r[parent] = t;
    }
}

DEV int qrs_add(QRes* r, int k, int32_t vid, float dist)
{
    if (dist < r[0].dist || (dist == r[0].dist && vid < r[0].vid)) {
        r[0].vid = vid; r[0].dist = dist;
        qrs_heapify(r, k);
        return 1;
    }
    return 0;
}

DEV void qrs_sort(QRes* r, int k)
{
    for (int i = k - 1; i >= 0; i--) {
        QRes t = r[0]; r[0] = r[i]; r[i] = t;
        qrs_heapify(r, i);
    }
}

/* ------------------------------------------------------------------ *
 * visited set — per-query global open-addressing table, atomicCAS
 * claim (set membership only; probe order is not part of the parity
 * contract — OptHashPosVector is a pure set, WorkSpace.h:113).
 * ------------------------------------------------------------------ */

/* returns 1 if idx was already present; inserts otherwise */
DEV int visited_test_insert(int32_t* tab, uint32_t mask, int32_t idx, int* oflow)
{
    uint32_t key = (uint32_t)(idx + 1);
    uint32_t h = (key * 2654435761u) & mask;
    for (int probe = 0; probe < 4096; probe++) {
        int32_t cur = atomicCAS(&tab[h], 0, (int32_t)key);
        if (cur == 0) return 0;
        if (cur == (int32_t)key) return 1;
        h = (h + 1) & mask;
    }
    *oflow = 1;
    return 1;
}

/* ------------------------------------------------------------------ *
 * distances — one candidate per 16-lane group, reference order
 * ------------------------------------------------------------------ */

/* the fused per-element step of both metrics */
template <int DM>
DEV float acc(float x, float y, float a)
{
    return (DM == DM_L2) ? fmaf(x - y, x - y, a) : fmaf(x, y, a);
}

/* float: the AVX512 chunk/fold order of DistanceUtils.cpp:650 (L2) /
 * the cosine analog, with fused lane accumulate (fmaf) as compiled in
 * the reference build (see oracle/sptag_oracle.c header). Result valid
 * on every lane of the group.
 *
 * The fixed-dim form fully unrolls the 16-element chunk loop so the
 * per-candidate global loads all issue before the fma chain waits on
 * them (the rolled loop costs one memory latency PER CHUNK — 8x the
 * stalls at d=128). Dims must be multiples of 16.
 *
 * It is split into load and reduce for software-pipelining candidate
 * rounds (loads of round r+1 issue while round r reduces). Only the
 * candidate's elements are register-resident: the query side is re-read
 * from LDS in the reduce (cheap ds_reads), keeping the pipeline's
 * register cost at C floats per fragment. */
template <int DM, int DFIX>
struct FragF32 {
    static constexpr int C = DFIX / 16;
    float y[C];
    DEV void load(const float* __restrict__ v)
    {
        const int g = threadIdx.x & 15;
#pragma unroll
        for (int c = 0; c < C; c++) y[c] = v[c * 16 + g];
    }
    /* xat(c) yields this lane's query element of chunk c */
    template <typename XAt>
    DEV float reduce_with(XAt xat) const
    {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) a = acc<DM>(xat(c), y[c], a);
        a = a + __shfl_down(a, 8, 16);
        a = a + __shfl_down(a, 4, 16);
        float sv = ((__shfl(a, 0, 16) + __shfl(a, 1, 16)) + __shfl(a, 2, 16)) +
                   __shfl(a, 3, 16);
        return (DM == DM_L2) ? sv : 1.0f - sv;
    }
    DEV float reduce(const float* __restrict__ q) const
    {
        const int g = threadIdx.x & 15;
        return reduce_with([&](int c) { return q[c * 16 + g]; });
    }
};

template <int DM, int DFIX>
DEV float dist_f32_fix(const float* __restrict__ q, const float* __restrict__ v)
{
    FragF32<DM, DFIX> x, y;
    x.load(q);
    y.load(v);
    return y.reduce_with([&](int c) { return x.y[c]; });
}

/* Dimension class of a float kernel instantiation. A kernel's register
 * allocation is the maximum over all its code paths, and the fully unrolled
 * 768-wide form holds 2 x 48 floats live: compiled into the same kernel it
 * costs a d=128 launch 77 VGPRs (146 against 69) for a form that launch
 * never runs. So each float kernel exists once per class, holding only that
 * class's fixed forms plus the generic rolled one, and the launchers pick
 * the class from the index's dim. The int8 kernels have no fixed forms and
 * exist once, as DC_SMALL. */
enum { DC_SMALL = 0, DC_LARGE = 1 };
enum { DC_SMALL_MAX_DIM = 128 };   /* float dims above this launch DC_LARGE */

template <int DM, int DC>
DEV float ref_dist_grp_f32(const float* __restrict__ q,
                           const float* __restrict__ v, int d)
{
    if constexpr (DC == DC_SMALL) {
        switch (d) {
        case 32:  return dist_f32_fix<DM, 32>(q, v);
        case 48:  return dist_f32_fix<DM, 48>(q, v);
        case 64:  return dist_f32_fix<DM, 64>(q, v);
        case 96:  return dist_f32_fix<DM, 96>(q, v);
        case 128: return dist_f32_fix<DM, 128>(q, v);
        default: break;
        }
    } else {
        switch (d) {
        case 256: return dist_f32_fix<DM, 256>(q, v);
        case 512: return dist_f32_fix<DM, 512>(q, v);
        case 768: return dist_f32_fix<DM, 768>(q, v);
        default: break;
        }
    }
    const int g = threadIdx.x & 15;
    float a = 0.0f;
    const int nd16 = (d >> 4) << 4;
    for (int i = 0; i < nd16; i += 16) {
        a = acc<DM>(q[i + g], v[i + g], a);
    }
    a = a + __shfl_down(a, 8, 16);           /* a8[g] on lanes g<8 */
    const int nd8 = (d >> 3) << 3;
    for (int i = nd16; i < nd8; i += 8) {
        if (g < 8) a = acc<DM>(q[i + g], v[i + g], a);
    }
    a = a + __shfl_down(a, 4, 16);           /* a4[g] on lanes g<4 */
    const int nd4 = (d >> 2) << 2;
    for (int i = nd8; i < nd4; i += 4) {
        if (g < 4) a = acc<DM>(q[i + g], v[i + g], a);
    }
    float s = ((__shfl(a, 0, 16) + __shfl(a, 1, 16)) + __shfl(a, 2, 16)) + __shfl(a, 3, 16);
    for (int i = nd4; i < d; i++) s = acc<DM>(q[i], v[i], s);
    return (DM == DM_L2) ? s : 1.0f - s;
}

/* int8: exact integer accumulation (order-free; partials exact in the
 * reference's float lanes for dim*254^2 < 2^24 — guarded host-side:
 * create_index() in host.cpp, which every create and load entry point goes
 * through, refuses int8 dims of 261 and more;
 * tests/test_abi.py::test_create_validation exercises it).
 * The dword path runs on the CDNA4 int8 dot units (v_dot4c_i32_i8 via
 * __builtin_amdgcn_sdot4) — the gfx950 analog of the reference's own GPU
 * __dp4a int8 path (cuda/Distance.hxx:84-101). Integer dots are exact and
 * order-free, so results stay bit-identical to the byte-wise form:
 * L2 uses sum (xa-xb)^2 = dot(a,a) - 2 dot(a,b) + dot(b,b), every term
 * < 2^25 at the guarded dims. */
template <int DM>
DEV float ref_dist_grp_i8(const int8_t* __restrict__ q,
                          const int8_t* __restrict__ v, int d)
{
    const int g = threadIdx.x & 15;
    int s = 0;
    if ((d & 3) == 0) {
        const int W = d >> 2;
        const int32_t* qw = (const int32_t*)q;
        const int32_t* vw = (const int32_t*)v;
        if (DM == DM_COSINE) {
            for (int w = g; w < W; w += 16)
                s = __builtin_amdgcn_sdot4(qw[w], vw[w], s, false);
        } else {
            int aa = 0, ab = 0, bb = 0;
            for (int w = g; w < W; w += 16) {
                int32_t a = qw[w], b = vw[w];
                aa = __builtin_amdgcn_sdot4(a, a, aa, false);
                ab = __builtin_amdgcn_sdot4(a, b, ab, false);
                bb = __builtin_amdgcn_sdot4(b, b, bb, false);
            }
            s = aa - 2 * ab + bb;
        }
    } else {
        for (int i = g; i < d; i += 16) {
            int xa = q[i], xb = v[i];
            s += (DM == DM_L2) ? (xa - xb) * (xa - xb) : xa * xb;
        }
    }
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    return (DM == DM_L2) ? (float)s : (float)(16129 - s);
}

template <typename T, int DM, int DC>
DEV float ref_dist_grp(const T* q, const T* v, int d)
{
    if constexpr (sizeof(T) == 4)
        return ref_dist_grp_f32<DM, DC>((const float*)q, (const float*)v, d);
    else
        return ref_dist_grp_i8<DM>((const int8_t*)q, (const int8_t*)v, d);
}

/* Per-phase cycle marks, diagnostic builds only; every member is empty
 * without PROF. One wave per workgroup, so lane-0 clock64 spans are
 * wave-accurate. With SPTAG_POP_AHEAD the `pop` span takes in the row's
 * latency and the SPT-pop span the tree triple's, so `pop + row` and the
 * seed / tree totals are what compare with a build without it, not the
 * single lines. */
template <bool PROF>
struct PhaseClock {
    uint64_t pc[9] = {};
    uint64_t t = 0, ng = 0, t_ng = 0;
    uint64_t aux[3] = {}, t_aux = 0;
    DEV void mark() { if (PROF && threadIdx.x == 0) t = clock64(); }
    DEV void acc(int i)
    {
        if (PROF && threadIdx.x == 0) {
            uint64_t now = clock64();
            pc[i] += now - t;
            t = now;
        }
    }
    /* lane 0 only: NG-insert share of the `insert` phase */
    DEV void ng_begin() { if (PROF) t_ng = clock64(); }
    DEV void ng_end() { if (PROF) ng += clock64() - t_ng; }
    /* lane 0 only, inside a phase: 0 SPT inserts, 1 SPT pops, 2 leaf branch
     * of search_trees_dev (visited CAS + NG insert) */
    DEV void aux_begin() { if (PROF) t_aux = clock64(); }
    DEV void aux_end(int i) { if (PROF) aux[i] += clock64() - t_aux; }
    DEV void store(int32_t* s) const   /* stats slots 2..15 */
    {
#pragma unroll
        for (int i = 0; i < 9; i++) s[2 + i] = (int32_t)pc[i];
        s[11] = (int32_t)ng;
#pragma unroll
        for (int i = 0; i < 3; i++) s[12 + i] = (int32_t)aux[i];
        s[15] = 0;
    }
};

/* ------------------------------------------------------------------ *
 * per-query context
 * ------------------------------------------------------------------ */

struct SerialState {          /* in LDS; lane 0 writes, wave reads after sync */
    int ng_count, spt_count;
    int dpq_len;                   /* iterative: results-queue length */
    int checked;
    int oflow, terminate, break_flag, want_tree;
    int tree_checked, no_better;   /* KDT counters */
    float fbcast;                  /* KDT upper-bound broadcast */
    NodeDist popped;
    int relaxed;                   /* iterative: sticky relaxedMono flag */
};
static_assert(sizeof(SerialState) <= SERIAL_STATE_BYTES,
              "SerialState outgrew its LDS slot");

template <typename T>
struct QCtx {
    const DevIndex* di;
    const SearchCfg* cfg;
    const T* qlds;            /* query vector staged in LDS */
    float* dstage;            /* MAX_DEG staged distances */
    int32_t* istage;          /* MAX_DEG staged ids / compacted lanes */
    QRes* qrs;                /* k results */
    float* dpq;               /* dpq_cap+1 */
    HeapRef ng, spt;
    int32_t* vtab;            /* this query's visited table */
    uint32_t vmask;
    SerialState* ss;
    int lane;
};

/* Query prologue shared by every one-wave-per-query kernel: carve the LDS
 * regions of `L`, stage query `q`, and let lane 0 start the serial state
 * from `ss0`, empty the `nres`-entry result set and (on a fresh traversal)
 * seed both heaps' empty-top sentinels. Ends in the barrier that publishes
 * all of it. `dpq` overrides the LDS results queue (null = use L.dpq). */
template <typename T>
DEV QCtx<T> begin_query(const DevIndex* di, const SearchCfg* cfg, const LdsLayout& L,
                        const void* queries, int q, int nres, float* dpq,
                        HeapRef ng, HeapRef spt, int32_t* visited, int32_t vcap,
                        const SerialState& ss0, bool fresh)
{
    extern __shared__ char smem[];
    const int lane = threadIdx.x;
    T* qlds = (T*)(smem + L.q);
    QCtx<T> c{di, cfg, qlds, (float*)(smem + L.dstage), (int32_t*)(smem + L.istage),
              (QRes*)(smem + L.qrs), dpq ? dpq : (float*)(smem + L.dpq), ng, spt,
              visited + (size_t)q * vcap, (uint32_t)(vcap - 1),
              (SerialState*)(smem + L.ss), lane};

    const T* gq = (const T*)queries + (size_t)q * di->dim;
    for (int i = lane; i < di->dim; i += 64) qlds[i] = gq[i];

    if (lane == 0) {
        *c.ss = ss0;
        if (fresh) {
            hset(ng, 0, NodeDist{-1, MAXDIST});   /* Heap empty-top sentinel */
            hset(spt, 0, NodeDist{-1, MAXDIST});
        }
        for (int i = 0; i < nres; i++) c.qrs[i] = QRes{-1, MAXDIST};
    }
    __syncthreads();
    return c;
}

/* Result epilogue: lane 0 sorts the result set (SortResult), then the wave
 * writes query q's k rows. */
DEV void write_topk(QRes* qrs, int k, int q, int32_t* out_vids, float* out_dists)
{
    if (threadIdx.x == 0) qrs_sort(qrs, k);
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += 64) {
        out_vids[(size_t)q * k + i] = qrs[i].vid;
        out_dists[(size_t)q * k + i] = qrs[i].dist;
    }
}

/* Frontier heaps of the batched search kernels. NG: at its reduced capacity
 * (LDSHEAP) entries [0..ng_lsplit] sit in LDS and the tail, if the host
 * chose a split below the capacity, in this query's global slab; the
 * global-heap variant keeps the whole heap in the slab. The capacity is the
 * total either way, so overflow means what it meant with the heap all in
 * LDS. SPT (tree) heap: hot top levels
 * in an LDS tier, tail in global scratch — full reference capacity without
 * the LDS cost of the whole heap (its all-global round-1 form made the seed
 * phase 41.5% of kernel cycles). */
template <bool LDSHEAP>
DEV void search_heaps(const SearchCfg& cfg, const SearchBufs& bufs, const LdsLayout& L,
                      int q, HeapRef& ng, HeapRef& spt)
{
    extern __shared__ char smem[];
    ng.cap = cfg.ng_cap;  ng.ref_cap = ref_ng_cap(cfg.max_check);
    ng.lds = LDSHEAP ? (NodeDist*)(smem + L.ng) : nullptr;
    ng.lsplit = LDSHEAP ? cfg.ng_lsplit : 0;
    /* with ng_lsplit == ng_cap no index reaches `a` and the host passes no slab */
    ng.a = bufs.gheap_ng ? (NodeDist*)bufs.gheap_ng + (size_t)q * (cfg.ng_cap + 1)
                         : nullptr;
    spt.cap = cfg.spt_cap; spt.ref_cap = ref_spt_cap(cfg.max_check);
    spt.a = (NodeDist*)bufs.gheap_spt + (size_t)q * (cfg.spt_cap + 1);
    spt.lds = (NodeDist*)(smem + L.spt_tier);
    spt.lsplit = SPT_LDS_TIER;
}

template <typename T>
DEV const T* vec_at(const DevIndex& di, int32_t v)
{
    return (const T*)di.vectors + (size_t)v * di.dim;
}

DEV int not_deleted(const DevIndex& di, int32_t v)
{
    /* StaticDispatch::CheckIfNotDeleted vs AlwaysTrue (BKTIndex.cpp:437,
     * dispatch :471-507): deletes ignored when the index has none. */
    if (!di.has_deleted) return 1;
    return di.deleted[v] == 0;
}

/* Read one byte of every 128B line of vector `vid` (a prefetch the compiler
 * cannot drop). Returns the sum; the caller sinks it where the loads may
 * land. */
template <typename T>
DEV uint32_t touch_lines(const DevIndex& di, int32_t vid)
{
    const char* vp = (const char*)vec_at<T>(di, vid);
    const int nline = ((int)((unsigned)di.dim * sizeof(T)) + 127) >> 7;
    uint32_t s = 0;
    for (int l = 0; l < nline; l++) s += (uint32_t)(uint8_t)vp[(size_t)l << 7];
    return s;
}

/* pipelined fixed-dim staging: group g handles candidates g, g+4, ...,
 * double-buffering fragments so the next round's global loads are in
 * flight while the current round reduces. */
template <int DM, int DFIX>
DEV void stage_dists_pipe_f32(QCtx<float>& c, int cnt)
{
    const DevIndex& di = *c.di;
    const int grp = c.lane >> 4;
    FragF32<DM, DFIX> A, B;
    int j = grp;
    if (j < cnt) A.load(vec_at<float>(di, c.istage[j]));
    while (j < cnt) {
        int jn = j + 4;
        if (jn < cnt) B.load(vec_at<float>(di, c.istage[jn]));
        float dv = A.reduce(c.qlds);
        if ((c.lane & 15) == 0) c.dstage[j] = dv;
        A = B;
        j = jn;
    }
    __syncthreads();
}

/* stage distances of `cnt` (<=64) data vectors whose ids are in istage[0..cnt)
 * into dstage[0..cnt); whole-wave cooperative, 4 candidates in flight. */
template <typename T, int DM, int DC>
DEV void stage_dists(QCtx<T>& c, int cnt)
{
    if constexpr (sizeof(T) == 4 && DC == DC_SMALL) {
        QCtx<float>& cf = reinterpret_cast<QCtx<float>&>(c);
        switch (c.di->dim) {
        /* pipelining holds 2 fragments (2*C VGPRs) live; C <= 8 only */
        case 32:  stage_dists_pipe_f32<DM, 32>(cf, cnt); return;
        case 48:  stage_dists_pipe_f32<DM, 48>(cf, cnt); return;
        case 64:  stage_dists_pipe_f32<DM, 64>(cf, cnt); return;
        case 96:  stage_dists_pipe_f32<DM, 96>(cf, cnt); return;
        case 128: stage_dists_pipe_f32<DM, 128>(cf, cnt); return;
        default: break;
        }
    }
    for (int r = 0; r < cnt; r += 4) {
        int j = r + (c.lane >> 4);
        if (j < cnt) {
            float dv = ref_dist_grp<T, DM, DC>(c.qlds, vec_at<T>(*c.di, c.istage[j]), c.di->dim);
            if ((c.lane & 15) == 0) c.dstage[j] = dv;
        }
    }
    __syncthreads();
}

/* Warm the GLOBAL parent-chain levels of the next `cnt` (<= 64) insertion
 * slots of heap `h` holding `count` entries (slot for the i-th insert is
 * count+1+i while the heap is not full, and the warm is advisory: a wrong
 * slot guess only wastes a touch; slots past the capacity are not guessed).
 * Lane-0's serial percolate-up then reads L1/L2-warm lines instead of
 * paying an HBM round trip per level — the seed phase was 31% of kernel
 * cycles with cold SPT parent reads. Levels in the LDS tier are skipped. */
DEV void heap_warm_parents(const HeapRef& h, int count, int cnt)
{
    const int lane = threadIdx.x;
    int loc = count + 1 + lane;
    uint32_t wsink = 0;
    if (lane < cnt && loc <= h.cap && h.a) {
        int par = loc >> 1;
        while (par > h.lsplit) {
            wsink += ((const uint8_t*)&h.a[par])[0];
            par >>= 1;
        }
    }
    asm volatile("" :: "v"(wsink));
}

/* Load the center ids of tree nodes [base, base+cnt) (cnt <= 64) into
 * istage and stage their distances into dstage. With TOUCH, issue ALL
 * children's vector lines before the staged distance rounds start: every
 * one of them is needed (no speculation waste), so the 16 round-pipeline
 * latencies collapse into one. Seed-phase tree-center gathers were 31% of
 * kernel cycles. */
template <typename T, int DM, int DC, bool TOUCH>
DEV void stage_child_dists(QCtx<T>& c, int base, int cnt)
{
    if (c.lane < cnt) c.istage[c.lane] = c.di->tree_nodes[(size_t)(base + c.lane) * 3];
    __syncthreads();
    uint32_t ts = 0;
    if (TOUCH && c.lane < cnt) ts = touch_lines<T>(*c.di, c.istage[c.lane]);
    stage_dists<T, DM, DC>(c, cnt);
    /* sink after the staging so the touches and the first rounds overlap */
    if constexpr (TOUCH) asm volatile("" :: "v"(ts));
}

/* wave-uniform read of a counter that lane 0 keeps in LDS */
DEV int uniform_count(const int* p) { return __builtin_amdgcn_readfirstlane(*p); }

/* Pop heap `h`, whose count lane 0 keeps at *pcount; the old top comes back
 * on every lane. The serial form (SPTAG_WAVE_POP=0, measurement builds) goes
 * through ss->popped and a barrier. */
DEV NodeDist pop_frontier(HeapRef h, int* pcount, SerialState* ss)
{
#if SPTAG_WAVE_POP
    int n = uniform_count(pcount);
    NodeDist top = ndheap_pop_wave(h, n);
    if (threadIdx.x == 0) *pcount = n;
    return top;
#else
    if (threadIdx.x == 0) ss->popped = ndheap_pop(h, pcount);
    __syncthreads();
    return ss->popped;
#endif
}

/* The node the next pop_frontier of `h` returns, wave-uniform; the heap is
 * not empty. Index 1 is final once the last heap operation has been issued
 * (heap_fence), so the loads whose address follows from this node alone can
 * be issued ahead of the pop and come back under its own waits: vector
 * memory loads return in the order they were issued, so the pop's wait for
 * its next block covers them. The entry sits in the LDS tier where there is
 * one, else in the line that the pop's first block reads. */
DEV int32_t peek_frontier(const HeapRef& h)
{
    return __builtin_amdgcn_readfirstlane(hget(h, 1).node);
}

/* One chunk of a BKT node's children into the SPT heap: cnt wave-wide
 * inserts back to back, child i's distance taken from lane i. */
template <typename T, int DM, int DC, bool PROF>
DEV void stage_children(QCtx<T>& c, int base, int cnt, PhaseClock<PROF>& clk)
{
    stage_child_dists<T, DM, DC, true>(c, base, cnt);
    int n = uniform_count(&c.ss->spt_count);
    heap_warm_parents(c.spt, n, cnt);
    const float dv = c.lane < cnt ? c.dstage[c.lane] : MAXDIST;
    clk.aux_begin();
    for (int i = 0; i < cnt; i++)
        ndheap_insert_wave(c.spt, n, NodeDist{base + i, lane_bcast(dv, i)}, &c.ss->oflow);
    clk.aux_end(0);
    if (c.lane == 0) c.ss->spt_count = n;
    __syncthreads();
}

/* A tree node's center joins the NG frontier unless it was visited: lane 0
 * claims it in the visited table, the wave inserts. Returns 1 if it went in. */
template <typename T>
DEV int frontier_add_center(QCtx<T>& c, int32_t center, float dist)
{
    int seen = 1;
    if (c.lane == 0) seen = visited_test_insert(c.vtab, c.vmask, center, &c.ss->oflow);
    if (__builtin_amdgcn_readfirstlane(seen)) return 0;
    int n = uniform_count(&c.ss->ng_count);
    ndheap_insert_wave(c.ng, n, NodeDist{center, dist}, &c.ss->oflow);
    if (c.lane == 0) c.ss->ng_count = n;
    return 1;
}

/* BKTree.h:772 SearchTrees — the whole wave pops, inserts and expands; lane 0
 * keeps the counters. Every counter read here follows a barrier that follows
 * its last write. */
template <typename T, int DM, int DC, bool PROF>
DEV void search_trees_dev(QCtx<T>& c, int limit, PhaseClock<PROF>& clk)
{
    const DevIndex& di = *c.di;
    for (;;) {
        __syncthreads();
        if (c.ss->spt_count <= 0 || c.ss->oflow) break;
        clk.aux_begin();
#if SPTAG_POP_AHEAD & 2
        /* the node about to be popped: its triple on lanes 0..2, issued
         * ahead of the pop */
        const int32_t* tn = di.tree_nodes + (size_t)peek_frontier(c.spt) * 3;
        int32_t tri = 0;
        if (c.lane < 3) tri = tn[c.lane];
        NodeDist bcell = pop_frontier(c.spt, &c.ss->spt_count, c.ss);
        clk.aux_end(1);
        int32_t center = __builtin_amdgcn_readlane(tri, 0);
        int32_t cs = __builtin_amdgcn_readlane(tri, 1);
        int32_t ce = __builtin_amdgcn_readlane(tri, 2);
#else
        NodeDist bcell = pop_frontier(c.spt, &c.ss->spt_count, c.ss);
        clk.aux_end(1);
        int32_t center = di.tree_nodes[(size_t)bcell.node * 3 + 0];
        int32_t cs = di.tree_nodes[(size_t)bcell.node * 3 + 1];
        int32_t ce = di.tree_nodes[(size_t)bcell.node * 3 + 2];
#endif
        if (cs < 0) {
            clk.aux_begin();
            const int checked = uniform_count(&c.ss->checked) +
                                frontier_add_center(c, center, bcell.distance);
            if (c.lane == 0) c.ss->checked = checked;
            clk.aux_end(2);
            if (checked >= limit) break;
        } else {
            frontier_add_center(c, center, bcell.distance);
            for (int base = cs; base < ce; base += 64)
                stage_children<T, DM, DC>(c, base, min(64, ce - base), clk);
        }
    }
    __syncthreads();
}

/* BKTree.h:697 InitSearchTrees (m_bfs = 0). */
template <typename T, int DM, int DC, bool PROF>
DEV void init_search_trees_dev(QCtx<T>& c, PhaseClock<PROF>& clk)
{
    const DevIndex& di = *c.di;
    for (int t = 0; t < di.ntrees; t++) {
        int32_t root = di.tree_start[t];
        int32_t center = di.tree_nodes[(size_t)root * 3 + 0];
        int32_t cs = di.tree_nodes[(size_t)root * 3 + 1];
        int32_t ce = di.tree_nodes[(size_t)root * 3 + 2];
        if (cs < 0) {
            float dv = 0.0f;
            if (c.lane < 16)
                dv = ref_dist_grp<T, DM, DC>(c.qlds, vec_at<T>(di, center), di.dim);
            int n = uniform_count(&c.ss->spt_count);
            ndheap_insert_wave(c.spt, n, NodeDist{root, lane_bcast(dv, 0)}, &c.ss->oflow);
            if (c.lane == 0) c.ss->spt_count = n;
            __syncthreads();
        } else {
            for (int base = cs; base < ce; base += 64)
                stage_children<T, DM, DC>(c, base, min(64, ce - base), clk);
        }
    }
}

/* ------------------------------------------------------------------ *
 * graph traversal steps shared by the BKT, iterative and KDT kernels
 * ------------------------------------------------------------------ */

/* adjacency row of one node: lane i < deg holds neighbor i */
struct Row {
    int32_t nn;         /* this lane's neighbor id (-1 past deg) */
    int firstneg;       /* first lane with no neighbor: the row ends there */
    int32_t checkNode;  /* last slot: < -1 marks a duplicate chain */
};

/* the load alone: this lane's slot of `node`'s row */
template <typename T>
DEV int32_t load_row_lanes(QCtx<T>& c, int32_t node)
{
    const int deg = c.di->deg;
    const int32_t* row = c.di->graph + (size_t)node * deg;
    return c.lane < deg ? row[c.lane] : -1;
}

/* the row whose slots the lanes hold (first use of the loaded values) */
template <typename T>
DEV Row make_row(QCtx<T>& c, int32_t nn)
{
    const int deg = c.di->deg;
    Row r;
    r.nn = nn;
    uint64_t negm = __ballot(c.lane >= deg || r.nn < 0);
    r.firstneg = negm ? (int)__builtin_ctzll(negm) : 64;
    r.checkNode = __shfl(r.nn, deg - 1);
    return r;
}

template <typename T>
DEV Row load_row(QCtx<T>& c, int32_t node)
{
    return make_row(c, load_row_lanes(c, node));
}

/* neighbor expansion (BKTIndex.cpp:333-345): compact the unvisited
 * neighbors of `r` (row order preserved) into istage[0..ncand) and return
 * ncand; ends in a barrier. */
template <typename T>
DEV int expand_neighbors(QCtx<T>& c, const Row& r)
{
    int already = 1;
    if (c.lane < r.firstneg)
        already = visited_test_insert(c.vtab, c.vmask, r.nn, &c.ss->oflow);
    uint64_t candm = __ballot(c.lane < r.firstneg && !already);
    if ((candm >> c.lane) & 1) {
        int pos = __popcll(candm & ((1ull << c.lane) - 1));
        c.istage[pos] = r.nn;
    }
    __syncthreads();
    return __popcll(candm);
}

/* ------------------------------------------------------------------ *
 * main search kernel
 * ------------------------------------------------------------------ */


/* The small class is held to the 7 waves/SIMD step (72 VGPRs) by hint; it
 * allocates 70 without scratch (profiles/wave_heaps_kernel_resources.txt). */
template <typename T, int DM, int DC, bool LDSHEAP, bool PROF = false>
__global__ __launch_bounds__(64, (DC == DC_SMALL && !PROF && SPTAG_LB_WAVES < 7) ? 7 : SPTAG_LB_WAVES)
void bkt_search_kernel(DevIndex di, SearchCfg cfg, SearchBufs bufs)
{
    const int q = blockIdx.x;
    if (q >= cfg.nq) return;
    const int lane = threadIdx.x;
    PhaseClock<PROF> clk;

    const LdsLayout L = lds_layout(di.dim, sizeof(T), cfg.k, MAX_DEG, cfg.dpq_cap,
                                   true, LDSHEAP ? cfg.ng_lsplit : 0);
    HeapRef ng, spt;
    search_heaps<LDSHEAP>(cfg, bufs, L, q, ng, spt);
    QCtx<T> c = begin_query<T>(&di, &cfg, L, bufs.queries, q, cfg.k, nullptr, ng, spt,
                               bufs.visited, cfg.vcap, SerialState{}, true);
    SerialState* ss = c.ss;
    QRes* qrs = c.qrs;
    float* dpq = c.dpq;

    /* m_Results: the sorted LDS set of dpq_accept_row, the queue's MaxDist
     * seed and its unfilled slots alike as MaxDist; published by the
     * barriers of the seed phase. */
    for (int i = lane; i < cfg.dpq_cap; i += 64) dpq[i] = MAXDIST;
    float dmax = MAXDIST;

    clk.mark();
    init_search_trees_dev<T, DM, DC>(c, clk);
    __syncthreads();
    search_trees_dev<T, DM, DC>(c, cfg.init_pivots, clk);
    clk.acc(0);

    int popped = 0;

    for (;;) {
        __syncthreads();
        if (ss->ng_count <= 0 || ss->terminate || ss->oflow) break;
        clk.mark();
#if SPTAG_POP_AHEAD & 1
        /* the row of the node about to be popped, issued ahead of the pop */
        const int32_t nn = load_row_lanes(c, peek_frontier(c.ng));
        const NodeDist gnode = pop_frontier(c.ng, &ss->ng_count, ss);
        clk.acc(1);
        popped++;
        const Row row = make_row(c, nn);
#else
        const NodeDist gnode = pop_frontier(c.ng, &ss->ng_count, ss);
        clk.acc(1);
        popped++;
        const Row row = load_row(c, gnode.node);
#endif
        clk.acc(2);

        if (lane == 0) {
            /* BKTIndex.cpp:290-331: result/termination block. The dispatch
             * flags (BKTIndex.cpp:471-507): searchDeleted makes the delete
             * filter AlwaysTrue; searchDuplicated selects CheckDup (walk
             * the duplicate chain until AddPoint rejects) vs NeverDup (add
             * the center only). */
            if (gnode.distance <= qrs[0].dist) {
                if (row.checkNode < -1) {
                    const int32_t* tn = &di.tree_nodes[(size_t)(-2 - row.checkNode) * 3];
                    int32_t i = -tn[1];
                    int32_t tmpNode = gnode.node;
                    do {
                        if (cfg.search_deleted || not_deleted(di, tmpNode)) {
                            if (cfg.search_dup) {
                                if (!qrs_add(qrs, cfg.k, tmpNode, gnode.distance)) break;
                            } else {
                                qrs_add(qrs, cfg.k, tmpNode, gnode.distance);
                                break;
                            }
                        }
                        if (i <= 0) break;
                        tmpNode = di.tree_nodes[(size_t)i * 3];
                    } while (i++ < tn[2]);
                } else {
                    if (cfg.search_deleted || not_deleted(di, gnode.node))
                        qrs_add(qrs, cfg.k, gnode.node, gnode.distance);
                }
            } else {
                if (cfg.search_deleted || not_deleted(di, gnode.node)) {
                    if (gnode.distance > dmax || ss->checked > cfg.max_check)
                        ss->terminate = 1;
                }
            }
        }
        __syncthreads();
        clk.acc(3);
        if (ss->terminate) break;

        int ncand = expand_neighbors(c, row);
        clk.acc(4);
        stage_dists<T, DM, DC>(c, ncand);
        clk.acc(5);
        /* insert phase (BKTIndex.cpp:337-344). Which of the row's
         * candidates m_Results accepts is decided once, wave-wide, from the
         * set at the start of the pop (dpq_accept_row); nothing between two
         * NG inserts depends on the set any more. The NG frontier heap stays
         * an exact Heap.h emulation (its pop order on equal keys is part of
         * the parity contract), evaluated by the whole wave: the accepted
         * candidates go in row order, back to back, each taken from the lane
         * that holds it. Nothing reads `checked` inside a row. */
        const NodeDist cand{lane < ncand ? c.istage[lane] : -1,
                            lane < ncand ? c.dstage[lane] : MAXDIST};
        const uint64_t acc = dpq_accept_row(dpq, cfg.dpq_cap, ncand, cand.distance, dmax);
        int ngc = uniform_count(&ss->ng_count);
        clk.ng_begin();
        for (uint64_t m = acc; m; m &= m - 1)
            ndheap_insert_wave(c.ng, ngc, lane_bcast(cand, __builtin_ctzll(m)), &ss->oflow);
        clk.ng_end();
        if (lane == 0) {
            ss->checked += ncand;
            ss->ng_count = ngc;
            /* dynamic pivots (BKTIndex.cpp:346-349) */
            ss->want_tree = (ndheap_top(c.ng, ss->ng_count).distance >
                             ndheap_top(c.spt, ss->spt_count).distance);
        }
        __syncthreads();
        clk.acc(6);
        if (ss->want_tree)
            search_trees_dev<T, DM, DC>(c, cfg.other_pivots + ss->checked, clk);
        clk.acc(7);
    }
    __syncthreads();

    if (lane == 0) bufs.oflow[q] = ss->oflow;
    clk.mark();
    write_topk(qrs, cfg.k, q, bufs.out_vids, bufs.out_dists);
    clk.acc(8);
    if (lane == 0 && bufs.stats) {
        int32_t* s = bufs.stats + (size_t)q * (PROF ? (int)PROF_STATS : 2);
        s[0] = ss->checked;
        s[1] = popped;
        if constexpr (PROF) clk.store(s);
    }
}

/* ------------------------------------------------------------------ *
 * Iterative (streaming) BKT search — reference SearchIterative
 * (src/Core/BKT/BKTIndex.cpp:354-427) driven per ResultIterator::Next
 * (src/Core/ResultIterator.cpp) with per-call ResetResult
 * (BKTIndex.cpp:663). One wave per iterator; ALL traversal state
 * (frontier/tree heaps at the reference's own capacities, visited table,
 * results queue, counters) persists in global scratch between calls.
 * ------------------------------------------------------------------ */

/* The small-class cosine form allocates 81 VGPRs unhinted, one above the
 * 6 waves/SIMD step; the hint brings it to 80 without scratch (checked in
 * profiles/occupancy_kernel_resources.txt). */
template <typename T, int DM, int DC>
__global__ __launch_bounds__(64, (DC == DC_SMALL && SPTAG_LB_WAVES < 6) ? 6 : SPTAG_LB_WAVES)
void bkt_iter_kernel(DevIndex di, SearchCfg cfg, IterBufs ib, int batch)
{
    const int q = blockIdx.x;
    if (q >= cfg.nq) return;
    const int lane = threadIdx.x;

    float* dpq = ib.dpq + (size_t)q * (cfg.dpq_cap + 1);
    HeapRef ng, spt;
    ng.cap = cfg.ng_cap;  ng.ref_cap = cfg.ng_cap;   /* reference capacities */
    spt.cap = cfg.spt_cap; spt.ref_cap = cfg.spt_cap;
    /* untiered: heap state persists in global scratch across Next() calls */
    ng.lds = nullptr; ng.lsplit = 0;
    spt.lds = nullptr; spt.lsplit = 0;
    ng.a = (NodeDist*)ib.gheap_ng + (size_t)q * (cfg.ng_cap + 1);
    spt.a = (NodeDist*)ib.gheap_spt + (size_t)q * (cfg.spt_cap + 1);

    IterState st = ib.state[q];
    /* ResetResult (WorkSpace.h:276): fresh m_Results + zeroed counters;
     * queues, visited set and the sticky relaxed flag persist. */
    SerialState ss0{};
    ss0.ng_count = st.ng_count;
    ss0.spt_count = st.spt_count;
    ss0.oflow = st.oflow;
    ss0.relaxed = st.relaxed;
    ss0.dpq_len = 1;
    if (lane == 0) dpq[1] = MAXDIST;

    QCtx<T> c = begin_query<T>(&di, &cfg, iter_lds_layout(di.dim, sizeof(T), batch),
                               ib.queries, q, batch, dpq, ng, spt, ib.visited,
                               cfg.vcap, ss0, st.first);
    SerialState* ss = c.ss;
    QRes* qrs = c.qrs;

    PhaseClock<false> clk;
    if (st.first) {
        init_search_trees_dev<T, DM, DC>(c, clk);
        __syncthreads();
        search_trees_dev<T, DM, DC>(c, cfg.init_pivots, clk);
    }

    int count = 0;

    for (;;) {
        __syncthreads();
        if (ss->ng_count <= 0 || ss->oflow || count >= batch) break;
        if (lane == 0) ss->popped = ndheap_pop(c.ng, &ss->ng_count);
        __syncthreads();
        NodeDist gnode = ss->popped;
        const Row row = load_row(c, gnode.node);

        if (lane == 0) {
            int cnt_new = count;
            if (not_deleted(di, gnode.node)) {
                qrs_add(qrs, batch, gnode.node, gnode.distance);
                cnt_new = count + 1;
                if (gnode.distance > dpq[1] || ss->checked > cfg.max_check)
                    ss->relaxed = 1;                     /* relaxedMono */
            }
            ss->fbcast = __int_as_float(cnt_new);
        }
        __syncthreads();
        count = __float_as_int(ss->fbcast);

        if (row.checkNode < -1) {
            /* iterative duplicate chain (BKTIndex.cpp:387-405): duplicates
             * enter the frontier; stage chunk distances, lane 0 inserts */
            const int32_t* tn = &di.tree_nodes[(size_t)(-2 - row.checkNode) * 3];
            int32_t cs0 = -tn[1], ce0 = tn[2];
            for (int base = cs0; base < ce0; base += 64) {
                int cnt = min(64, ce0 - base);
                stage_child_dists<T, DM, DC, false>(c, base, cnt);
                if (lane == 0) {
                    for (int i = 0; i < cnt; i++) {
                        int32_t tmpNode = c.istage[i];
                        if (!not_deleted(di, tmpNode)) continue;
                        if (!visited_test_insert(c.vtab, c.vmask, tmpNode, &ss->oflow))
                            ndheap_insert(c.ng, &ss->ng_count,
                                          NodeDist{tmpNode, c.dstage[i]}, &ss->oflow);
                    }
                }
                __syncthreads();
            }
        }

        int ncand = expand_neighbors(c, row);
        stage_dists<T, DM, DC>(c, ncand);
        if (lane == 0) {
            for (int r = 0; r < ncand; r++) {
                float dv = c.dstage[r];
                ss->checked++;
                ndheap_insert(c.ng, &ss->ng_count, NodeDist{c.istage[r], dv}, &ss->oflow);
                dpq_insert(dpq, &ss->dpq_len, cfg.dpq_cap, dv);
            }
            ss->want_tree = (ndheap_top(c.ng, ss->ng_count).distance >
                             ndheap_top(c.spt, ss->spt_count).distance);
        }
        __syncthreads();
        if (ss->want_tree)
            search_trees_dev<T, DM, DC>(c, cfg.other_pivots + ss->checked, clk);
    }
    __syncthreads();

    if (lane == 0) {
        st.ng_count = ss->ng_count;
        st.spt_count = ss->spt_count;
        st.checked = ss->checked;
        st.tree_checked = ss->tree_checked;
        st.relaxed = ss->relaxed;
        st.first = 0;
        st.oflow = ss->oflow;
        ib.state[q] = st;
        ib.out_counts[q] = count;
        ib.out_relaxed[q] = st.relaxed;
    }
    write_topk(qrs, batch, q, ib.out_vids, ib.out_dists);
}

/* ------------------------------------------------------------------ *
 * KDT search (reference src/Core/KDT/KDTIndex.cpp:184-241 +
 * inc/Core/Common/KDTree.h:213-273). Shares the heaps/visited/top-k/
 * distance machinery; differs in the seed descent (kd-tree with
 * squared-split-plane lower bounds in the SPT queue), in the frontier
 * update (every computed neighbor enters the queue — no results-queue
 * gate) and in termination (continuous-no-better-propagation counter).
 * ------------------------------------------------------------------ */

struct KdtNode { int32_t left, right, split_dim; float split_value; };

/* KDTree.h:234-271 KDTSearch, iterative; lane 0 descends (serial pointer
 * chase), the wave's first 16-lane group computes the leaf distance. */
template <typename T, int DM, int DC>
DEV void kdt_search_node_dev(QCtx<T>& c, int32_t node, float dist_bound)
{
    const DevIndex& di = *c.di;
    const KdtNode* kn = (const KdtNode*)di.tree_nodes;
    SerialState* ss = c.ss;
    /* descent: lane 0 walks, broadcasting the final leaf via ss->popped */
    if (c.lane == 0) {
        while (node >= 0) {
            KdtNode tn = kn[node];
            float qv = (float)c.qlds[tn.split_dim];
            float diff = qv - tn.split_value;
            float other_bound = dist_bound + diff * diff;
            int32_t best = diff < 0.0f ? tn.left : tn.right;
            int32_t other = diff < 0.0f ? tn.right : tn.left;
            ndheap_insert(c.spt, &ss->spt_count, NodeDist{other, other_bound},
                          &ss->oflow);
            node = best;
        }
        int32_t index = -node - 1;
        if (index >= di.n) index = -1;
        else if (visited_test_insert(c.vtab, c.vmask, index, &ss->oflow)) index = -1;
        ss->popped.node = index;
    }
    __syncthreads();
    int32_t index = ss->popped.node;
    if (index >= 0) {
        float dv = 0.0f;
        if (c.lane < 16)
            dv = ref_dist_grp<T, DM, DC>(c.qlds, vec_at<T>(di, index), di.dim);
        if (c.lane == 0) {
            ss->tree_checked++;
            ss->checked++;
            ndheap_insert(c.ng, &ss->ng_count, NodeDist{index, dv}, &ss->oflow);
        }
    }
    __syncthreads();
}

/* KDTree.h:219-231 SearchTrees: pop bounds until the leaf budget. */
template <typename T, int DM, int DC>
DEV void kdt_search_trees_dev(QCtx<T>& c, int limits)
{
    SerialState* ss = c.ss;
    for (;;) {
        __syncthreads();
        if (ss->spt_count <= 0 || ss->checked >= limits || ss->oflow) break;
        if (c.lane == 0) ss->popped = ndheap_pop(c.spt, &ss->spt_count);
        __syncthreads();
        NodeDist tcell = ss->popped;
        kdt_search_node_dev<T, DM, DC>(c, tcell.node, tcell.distance);
    }
    __syncthreads();
}

template <typename T, int DM, int DC, bool LDSHEAP>
__global__ __launch_bounds__(64, SPTAG_LB_WAVES)
void kdt_search_kernel(DevIndex di, SearchCfg cfg, SearchBufs bufs)
{
    const int q = blockIdx.x;
    if (q >= cfg.nq) return;
    const int lane = threadIdx.x;

    /* same layout as the BKT kernel; the results-queue region is reserved
     * but unused here (KDT has no results-queue gate) */
    const LdsLayout L = lds_layout(di.dim, sizeof(T), cfg.k, MAX_DEG, cfg.dpq_cap,
                                   true, LDSHEAP ? cfg.ng_lsplit : 0);
    HeapRef ng, spt;
    search_heaps<LDSHEAP>(cfg, bufs, L, q, ng, spt);
    QCtx<T> c = begin_query<T>(&di, &cfg, L, bufs.queries, q, cfg.k, nullptr, ng, spt,
                               bufs.visited, cfg.vcap, SerialState{}, true);
    SerialState* ss = c.ss;
    QRes* qrs = c.qrs;

    /* InitSearchTrees (KDTree.h:213): every tree root at bound 0 */
    for (int t = 0; t < di.ntrees; t++)
        kdt_search_node_dev<T, DM, DC>(c, di.tree_start[t], 0.0f);
    kdt_search_trees_dev<T, DM, DC>(c, cfg.init_pivots);

    int popped = 0;

    for (;;) {
        __syncthreads();
        if (ss->ng_count <= 0 || ss->terminate || ss->oflow) break;
        if (lane == 0) ss->popped = ndheap_pop(c.ng, &ss->ng_count);
        __syncthreads();
        popped++;
        NodeDist gnode = ss->popped;
        const Row row = load_row(c, gnode.node);

        if (lane == 0) {
            /* KDTIndex.cpp:201-209: result + budget termination */
            if (not_deleted(di, gnode.node)) {
                if (!qrs_add(qrs, cfg.k, gnode.node, gnode.distance) &&
                    ss->checked > cfg.max_check)
                    ss->terminate = 1;
            }
            float worst = qrs[0].dist;
            ss->fbcast = worst > gnode.distance ? worst : gnode.distance;
        }
        __syncthreads();
        if (ss->terminate) break;
        float upper_bound = ss->fbcast;

        int ncand = expand_neighbors(c, row);
        stage_dists<T, DM, DC>(c, ncand);
        if (lane == 0) {
            /* KDTIndex.cpp:211-233: every computed neighbor joins the
             * frontier; track whether any beat the upper bound */
            int local_opt = 1;
            for (int r = 0; r < ncand; r++) {
                float dv = c.dstage[r];
                if (dv <= upper_bound) local_opt = 0;
                ss->checked++;
                ndheap_insert(c.ng, &ss->ng_count, NodeDist{c.istage[r], dv}, &ss->oflow);
            }
            if (local_opt) ss->no_better++;
            else ss->no_better = 0;
            ss->want_tree = 0;
            ss->break_flag = 0;
            if (ss->no_better > cfg.nobetter_threshold) {
                if (ss->tree_checked <= ss->checked / 10)
                    ss->want_tree = 1;
                else if (gnode.distance > qrs[0].dist)
                    ss->break_flag = 1;
            }
        }
        __syncthreads();
        if (ss->break_flag) break;
        if (ss->want_tree)
            kdt_search_trees_dev<T, DM, DC>(c, cfg.other_pivots + ss->checked);
    }
    __syncthreads();

    if (lane == 0) {
        bufs.oflow[q] = ss->oflow;
        if (bufs.stats) {
            bufs.stats[(size_t)q * 2 + 0] = ss->checked;
            bufs.stats[(size_t)q * 2 + 1] = popped;
        }
    }
    write_topk(qrs, cfg.k, q, bufs.out_vids, bufs.out_dists);
}

/* ------------------------------------------------------------------ *
 * brute-force truth kernel (TruthSet::GenerateTruth semantics,
 * TruthSet.h:163): exact top-k by (dist, vid) over all non-deleted rows.
 * One query per wave; test-scale only.
 * ------------------------------------------------------------------ */

template <typename T, int DM, int DC>
__global__ __launch_bounds__(64)
void truth_kernel(DevIndex di, const void* queries, int32_t nq, int32_t k,
                  int32_t* out_vids, float* out_dists)
{
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int lane = threadIdx.x;

    QCtx<T> c = begin_query<T>(&di, nullptr, truth_lds_layout(di.dim, sizeof(T), k),
                               queries, q, k, nullptr, HeapRef{}, HeapRef{}, nullptr, 0,
                               SerialState{}, false);
    /* no traversal state here: the scalar slot stages the 4 distances */
    float* dstage = (float*)c.ss;

    for (int32_t base = 0; base < di.n; base += 4) {
        int cnt = min(4, di.n - base);
        int j = lane >> 4;
        if (j < cnt) {
            float dv = ref_dist_grp<T, DM, DC>(c.qlds, vec_at<T>(di, base + j), di.dim);
            if ((lane & 15) == 0) dstage[j] = dv;
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < cnt; i++) {
                if (di.has_deleted && di.deleted[base + i]) continue;
                qrs_add(c.qrs, k, base + i, dstage[i]);
            }
        }
        __syncthreads();
    }
    write_topk(c.qrs, k, q, out_vids, out_dists);
}

/* ------------------------------------------------------------------ *
 * row gather/scatter (flagged-query reruns): copy nrows rows, with idx
 * naming the source rows (SRC_INDEXED, gather) or the destination rows
 * ------------------------------------------------------------------ */

template <bool SRC_INDEXED>
__global__ void copy_rows_kernel(char* dst, const char* src, int row_bytes,
                                 const int32_t* idx, int nrows)
{
    int r = blockIdx.x;
    if (r >= nrows) return;
    const char* s = src + (size_t)(SRC_INDEXED ? idx[r] : r) * row_bytes;
    char* d = dst + (size_t)(SRC_INDEXED ? r : idx[r]) * row_bytes;
    if ((row_bytes & 3) == 0) {
        for (int i = threadIdx.x; i < row_bytes / 4; i += blockDim.x)
            ((uint32_t*)d)[i] = ((const uint32_t*)s)[i];
    } else {
        for (int i = threadIdx.x; i < row_bytes; i += blockDim.x)
            d[i] = s[i];
    }
}

int launch_copy_rows(bool gather, void* dst, const void* src, int row_bytes,
                     const int32_t* d_idx, int nrows)
{
    hipLaunchKernelGGL(gather ? copy_rows_kernel<true> : copy_rows_kernel<false>,
                       dim3(nrows), dim3(64), 0, nullptr, (char*)dst, (const char*)src,
                       row_bytes, d_idx, nrows);
    return (int)hipGetLastError();
}

/* ------------------------------------------------------------------ *
 * shard merge (AggregatorService::AggregateResults semantics,
 * src/Aggregator/AggregatorService.cpp:363: concatenate the per-shard
 * lists, then select): S lists of k_in entries per query, each ascending
 * by (dist, vid) with a vid < 0 padding suffix, become one list of k_out
 * entries ascending by (dist, vid + base[s]), padded with vid = -1.
 *
 * One wave per query and no sort. Every list is sorted already, so a real
 * candidate's output rank is its position in its own list plus, for each
 * other list, the number of entries whose key is smaller, and that number
 * is a binary search. Keys order by distance (float `<`), then global id,
 * then shard number; padding is greater than everything. Global ids of a
 * well-formed shard set are distinct, so the shard number never decides
 * there; it only keeps the ranks distinct, and every output slot written
 * exactly once, when a caller's bases overlap. A candidate writes itself
 * iff its rank is below k_out. Lanes stride over the S*k_in candidates.
 *
 * STAGED keeps the query's lists in LDS as (dist, global id) pairs;
 * otherwise the searches read global memory. Same result either way.
 * ------------------------------------------------------------------ */

struct MergeKey { float dist; int32_t gvid; };   /* gvid < 0: padding */

/* is list entry `e` of shard `es` ordered before the real candidate `c` of
 * shard `cs`? */
DEV bool merge_before(MergeKey e, int es, MergeKey c, int cs)
{
    if (e.gvid < 0) return false;
    if (e.dist < c.dist) return true;
    if (c.dist < e.dist) return false;
    if (e.gvid != c.gvid) return e.gvid < c.gvid;
    return es < cs;
}

template <bool STAGED>
__global__ __launch_bounds__(64)
void merge_topk_kernel(const int32_t* __restrict__ vids,
                       const float* __restrict__ dists, MergeBases bases,
                       int S, int nq, int k_in, int k_out,
                       int32_t* __restrict__ out_vids, float* __restrict__ out_dists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int lane = threadIdx.x;
    const int ncand = S * k_in;              /* <= 64 * MAX_K */
    const size_t list_stride = (size_t)nq * k_in;
    const int32_t* qv = vids + (size_t)q * k_in;    /* + s * list_stride */
    const float* qd = dists + (size_t)q * k_in;
    MergeKey* keys = (MergeKey*)merge_lds;   /* STAGED: [S][k_in] */

    /* entry i of list s as a key */
    auto entry = [&](int s, int i) -> MergeKey {
        if constexpr (STAGED) return keys[s * k_in + i];
        int32_t v = qv[s * list_stride + i];
        return MergeKey{qd[s * list_stride + i], v < 0 ? -1 : v + bases.b[s]};
    };

    if constexpr (STAGED) {
        for (int c = lane; c < ncand; c += 64) {
            int s = c / k_in, i = c - s * k_in;
            int32_t v = qv[s * list_stride + i];
            keys[c] = MergeKey{qd[s * list_stride + i], v < 0 ? -1 : v + bases.b[s]};
        }
        __syncthreads();
    }

    int nreal = 0;                 /* wave-uniform: real candidates seen */
    float paddist = MAXDIST;       /* wave-uniform: the inputs' own padding */
    bool have_pad = false;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < ncand;
        int s = 0, i = 0;
        MergeKey me{MAXDIST, -1};
        if (in) {
            s = c / k_in;
            i = c - s * k_in;
            me = entry(s, i);
        }
        const bool real = in && me.gvid >= 0;
        const unsigned long long padmask = __ballot(in && !real);
        nreal += __popcll(__ballot(real));
        if (!have_pad && padmask) {
            paddist = __shfl(me.dist, __ffsll((long long)padmask) - 1);
            have_pad = true;
        }
        if (!real) continue;
        int rank = i;
        for (int t = 0; t < S && rank < k_out; t++) {
            if (t == s) continue;
            int lo = 0, hi = k_in;          /* first entry not before `me` */
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (merge_before(entry(t, mid), t, me, s)) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < k_out) {
            out_vids[(size_t)q * k_out + rank] = me.gvid;
            out_dists[(size_t)q * k_out + rank] = me.dist;
        }
    }
    for (int r = nreal + lane; r < k_out; r += 64) {
        out_vids[(size_t)q * k_out + r] = -1;
        out_dists[(size_t)q * k_out + r] = paddist;
    }
}

int launch_merge_topk(const int32_t* vids, const float* dists,
                      const MergeBases& bases, int nshards, int32_t nq,
                      int32_t k_in, int32_t k_out, int32_t* out_vids,
                      float* out_dists)
{
    /* the kernel indexes nothing outside these bounds */
    if (nshards < 1 || nshards > MAX_SHARDS || nq < 1 || k_in < 1 || k_in > MAX_K ||
        k_out < 1 || k_out > MAX_K)
        return (int)hipErrorInvalidValue;
    const int ncand = nshards * k_in;
    const bool staged = ncand <= MERGE_LDS_ENTRIES;
    hipLaunchKernelGGL(staged ? merge_topk_kernel<true> : merge_topk_kernel<false>,
                       dim3(nq), dim3(64), staged ? (size_t)ncand * sizeof(MergeKey) : 0,
                       nullptr, vids, dists, bases, nshards, nq, k_in, k_out, out_vids,
                       out_dists);
    return (int)hipGetLastError();
}

/* ------------------------------------------------------------------ *
 * heap probe (tests): one script of inserts and pops on a HeapRef built
 * from the arguments, run by block 0 with the serial functions and by
 * block 1 with the wave-wide ones, each on its own array.
 * ------------------------------------------------------------------ */

__global__ __launch_bounds__(64)
void heap_probe_kernel(HeapProbeArgs p)
{
    extern __shared__ char smem[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    HeapRef h;
    h.a = (NodeDist*)p.heaps + (size_t)b * (p.cap + 1);
    h.lds = p.lsplit > 0 ? (NodeDist*)smem : nullptr;
    h.lsplit = p.lsplit;
    h.cap = p.cap;
    h.ref_cap = p.ref_cap;
    NodeDist* pops = (NodeDist*)p.pops + (size_t)b * p.nops;
    int* oflow = p.final + b * 2 + 1;
    int count = 0;
    if (lane == 0) hset(h, 0, NodeDist{-1, MAXDIST});
    __syncthreads();
    if (b == 1) {
        for (int i = 0; i < p.nops; i++) {
            if (p.ops[i]) {
                ndheap_insert_wave(h, count, NodeDist{p.nodes[i], p.dists[i]}, oflow);
            } else {
                NodeDist t = ndheap_pop_wave(h, count);
                if (lane == 0) pops[i] = t;
            }
        }
    } else if (lane == 0) {
        for (int i = 0; i < p.nops; i++) {
            if (p.ops[i]) ndheap_insert(h, &count, NodeDist{p.nodes[i], p.dists[i]}, oflow);
            else pops[i] = ndheap_pop(h, &count);
        }
    }
    __syncthreads();
    if (lane == 0) p.final[b * 2] = count;
    /* the caller reads the whole array from global memory */
    if (h.lds)
        for (int i = lane; i <= min(p.lsplit, p.cap); i += 64) h.a[i] = h.lds[i];
}

int launch_heap_probe(const HeapProbeArgs& p)
{
    /* the kernel indexes nothing outside these bounds */
    if (p.cap < 1 || p.cap > HEAP_PROBE_MAX_CAP || p.ref_cap < p.cap || p.lsplit < 0 ||
        p.lsplit > HEAP_PROBE_MAX_LSPLIT || p.nops < 1)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(heap_probe_kernel, dim3(2), dim3(64),
                       p.lsplit > 0 ? ((size_t)p.lsplit + 1) * sizeof(NodeDist) : 0,
                       nullptr, p);
    return (int)hipGetLastError();
}

/* ------------------------------------------------------------------ *
 * launchers
 * ------------------------------------------------------------------ */

template <typename T> struct TypeTag { using type = T; };

/* call f(TypeTag<T>, integral_constant<DM>, integral_constant<DC>) for the
 * runtime (vt, dm, dim); only float has two dimension classes */
template <typename F>
static int dispatch_kernel(int vt, int dm, int dim, F&& f)
{
    using L2 = std::integral_constant<int, DM_L2>;
    using Cos = std::integral_constant<int, DM_COSINE>;
    using Small = std::integral_constant<int, DC_SMALL>;
    using Large = std::integral_constant<int, DC_LARGE>;
    const bool large = dim > DC_SMALL_MAX_DIM;
    if (vt == VT_FLOAT && dm == DM_L2)
        return large ? f(TypeTag<float>{}, L2{}, Large{})
                     : f(TypeTag<float>{}, L2{}, Small{});
    if (vt == VT_FLOAT && dm == DM_COSINE)
        return large ? f(TypeTag<float>{}, Cos{}, Large{})
                     : f(TypeTag<float>{}, Cos{}, Small{});
    if (vt == VT_INT8 && dm == DM_L2) return f(TypeTag<int8_t>{}, L2{}, Small{});
    if (vt == VT_INT8 && dm == DM_COSINE) return f(TypeTag<int8_t>{}, Cos{}, Small{});
    return (int)hipErrorInvalidValue;
}

template <typename T, int DM, int DC, bool LDSHEAP>
static int launch_one(const DevIndex& di, const SearchCfg& cfg,
                      const SearchBufs& bufs)
{
    size_t lds = lds_bytes(di.dim, sizeof(T), cfg, LDSHEAP);
    auto kernel = di.algo == ALGO_KDT ? kdt_search_kernel<T, DM, DC, LDSHEAP>
                  : cfg.prof          ? bkt_search_kernel<T, DM, DC, LDSHEAP, true>
                                      : bkt_search_kernel<T, DM, DC, LDSHEAP, false>;
    hipLaunchKernelGGL(kernel, dim3(cfg.nq), dim3(64), lds, nullptr, di, cfg, bufs);
    return (int)hipGetLastError();
}

int launch_bkt_search(int vt, int dm, bool heaps_in_lds, const DevIndex& di,
                      const SearchCfg& cfg, const SearchBufs& bufs)
{
    return dispatch_kernel(vt, dm, di.dim, [&](auto t, auto d, auto c) {
        using T = typename decltype(t)::type;
        constexpr int DM = decltype(d)::value, DC = decltype(c)::value;
        return heaps_in_lds ? launch_one<T, DM, DC, true>(di, cfg, bufs)
                            : launch_one<T, DM, DC, false>(di, cfg, bufs);
    });
}

int launch_bkt_iter(int vt, int dm, const DevIndex& di, const SearchCfg& cfg,
                    const IterBufs& ib, int batch)
{
    return dispatch_kernel(vt, dm, di.dim, [&](auto t, auto d, auto c) {
        using T = typename decltype(t)::type;
        constexpr int DM = decltype(d)::value, DC = decltype(c)::value;
        size_t lds = iter_lds_layout(di.dim, sizeof(T), batch).total;
        hipLaunchKernelGGL((bkt_iter_kernel<T, DM, DC>), dim3(cfg.nq),
                           dim3(64), lds, nullptr, di, cfg, ib, batch);
        return (int)hipGetLastError();
    });
}

int launch_truth(int vt, int dm, const DevIndex& di, const void* queries,
                 int32_t nq, int32_t k, int32_t* ov, float* od)
{
    return dispatch_kernel(vt, dm, di.dim, [&](auto t, auto d, auto c) {
        using T = typename decltype(t)::type;
        constexpr int DM = decltype(d)::value, DC = decltype(c)::value;
        size_t lds = truth_lds_layout(di.dim, sizeof(T), k).total;
        hipLaunchKernelGGL((truth_kernel<T, DM, DC>), dim3(nq), dim3(64),
                           lds, nullptr, di, queries, nq, k, ov, od);
        return (int)hipGetLastError();
    });
}

}  /* namespace sptag_amd */
