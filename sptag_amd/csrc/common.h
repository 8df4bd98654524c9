/* Internal host<->device shared definitions for the sptag_amd backend.
 * Not part of the public ABI (that is include/sptag_amd.h). */
#pragma once
#include <stdint.h>

namespace sptag_amd {

/* mirror of the public constants */
enum { VT_FLOAT = 0, VT_INT8 = 1 };
enum { DM_L2 = 0, DM_COSINE = 1 };

/* default search parameters (reference BKT/ParameterDefinitionList.h:47-49) */
enum { DEFAULT_MAXCHECK = 8192, INIT_PIVOTS = 50, OTHER_PIVOTS = 4 };

/* hard caps of the v1 kernel (host validates before launch) */
enum { MAX_DEG = 64, MAX_K = 1024, MAX_DIM = 4096 };

enum { ALGO_BKT = 0, ALGO_KDT = 1 };

/* device-resident index description (POD, passed by value to kernels) */
struct DevIndex {
    const void* vectors;       /* n*dim row-major, element size by vt */
    const int32_t* graph;      /* n*deg row-major adjacency */
    const int32_t* tree_nodes; /* BKT: {centerid,childStart,childEnd} int32x3;
                                  KDT: {left,right,split_dim,split_value} 16B */
    const int32_t* tree_start; /* ntrees roots */
    const uint8_t* deleted;    /* may be null */
    int32_t n, dim, deg, ntrees, n_tree_nodes;
    int32_t has_deleted;
    int32_t algo;
};

/* per-launch search configuration */
struct SearchCfg {
    int32_t nq, k, max_check;
    int32_t init_pivots, other_pivots;
    int32_t nobetter_threshold;  /* KDT: ThresholdOfNumberOfContinuousNoBetterPropagation */
    int32_t search_dup;          /* searchDuplicated (BKT dispatch bit 1) */
    int32_t search_deleted;      /* searchDeleted (dispatch bit 2) */
    int32_t ng_cap, spt_cap, dpq_cap;  /* heap capacities (entries) */
    int32_t ng_lsplit;   /* LDS pass: NG heap entries [0..ng_lsplit] live in
                            LDS, the rest in the query's gheap_ng slab;
                            == ng_cap keeps the whole heap in LDS */
    int32_t vcap;                      /* visited table slots (pow2) */
    int32_t prof;        /* 1 = per-phase cycle breakdown into stats
                            (stride PROF_STATS int32 per query; lane-0
                            clock64 marks — one wave per WG makes lane-0
                            spans wave-accurate). Diagnostic only. */
};

enum { PROF_STATS = 16 };  /* stats stride (int32) in prof mode; slots:
    0 checked, 1 popped, 2 seed, 3 pop, 4 row, 5 serial, 6 cas, 7 dist,
    8 insert, 9 tree, 10 epilogue (cycles), 11 NG-insert share of 8; inside
    2 + 9: 12 tree-heap inserts, 13 tree-heap pops, 14 SearchTrees leaf
    branch (visited CAS + NG insert) */

/* per-launch buffers */
struct SearchBufs {
    const void* queries;   /* nq*dim */
    int32_t* out_vids;     /* nq*k */
    float* out_dists;      /* nq*k */
    int32_t* visited;      /* nq*vcap, zeroed before launch */
    int32_t* oflow;        /* nq flags: nonzero => rerun with bigger caps */
    int32_t* stats;        /* nq*2: {checked, popped} per query (may be null) */
    /* per-query strided scratch: the whole heap in the global-heap variant,
     * the tail below the LDS tier in the LDS pass (gheap_ng may be null
     * there when ng_lsplit == ng_cap) */
    void* gheap_ng;        /* nq * (ng_cap+1) * 8B */
    void* gheap_spt;       /* nq * (spt_cap+1) * 8B */
};

enum { SPT_LDS_TIER_H = 255 };  /* SPT heap LDS tier entries (see kernels) */
enum { NG_GLEVELS = 3 };  /* NG heap: deepest levels kept in global memory in
                             the LDS pass (see ng_lds_split); chosen by
                             measurement, profiles/occupancy_ng_tier.txt */
enum { SERIAL_STATE_BYTES = 64 };  /* LDS slot of the kernels' SerialState */

#ifdef __HIPCC__
#define SPTAG_HD __host__ __device__
#else
#define SPTAG_HD
#endif

/* the reference's heap capacities (WorkSpace.h:265): frontier and tree heap */
SPTAG_HD inline int32_t ref_ng_cap(int32_t max_check) { return max_check * 30; }
SPTAG_HD inline int32_t ref_spt_cap(int32_t max_check) { return max_check * 10; }

/* Dynamic-LDS carve-up of the one-wave-per-query kernels: byte offsets of
 * each region and the total. The kernels take their pointers and the
 * launchers their LDS size from this one function. */
struct LdsLayout {
    uint32_t q, dstage, istage, qrs, dpq, ss, spt_tier, ng, total;
};

/* nstage: staged candidates (dstage + istage entries each); dpq_cap < 0: no
 * results queue in LDS; ng_lds: NG heap entries [0..ng_lds] in LDS, 0: none. */
SPTAG_HD inline LdsLayout lds_layout(int dim, size_t esz, int k, int nstage,
                                     int dpq_cap, bool spt_tier, int ng_lds)
{
    LdsLayout l;
    uint32_t b = 0;
    l.q = b;        b += (uint32_t)(((size_t)dim * esz + 15) & ~15ul);  /* query vector */
    l.dstage = b;   b += (uint32_t)nstage * 4;             /* staged dists */
    l.istage = b;   b += (uint32_t)nstage * 4;             /* staged ids */
    l.qrs = b;      b += (uint32_t)k * 8;                  /* result set */
    l.dpq = b;      if (dpq_cap >= 0) b += ((uint32_t)dpq_cap + 1) * 4;  /* DistPriorityQueue */
    l.ss = b;       b += SERIAL_STATE_BYTES;               /* scalar slots, padding */
    l.spt_tier = b; if (spt_tier) b += ((uint32_t)SPT_LDS_TIER_H + 1) * 8;
    l.ng = b;       if (ng_lds > 0) b += ((uint32_t)ng_lds + 1) * 8;  /* heap tails are global */
    l.total = b;
    return l;
}

/* batched BKT/KDT search; the KDT kernel reserves the results queue too */
inline size_t lds_bytes(int dim, size_t esz, const SearchCfg& c, bool heaps_in_lds)
{
    return lds_layout(dim, esz, c.k, MAX_DEG, c.dpq_cap, true,
                      heaps_in_lds ? c.ng_lsplit : 0).total;
}

/* NG heap entries kept in LDS when the deepest `glevels` levels of a heap
 * filled to `ng_cap` go to global memory: every shallower level stays, so
 * the split is the last index of a level. glevels 0 keeps the whole heap. */
inline int32_t ng_lds_split(int32_t ng_cap, int glevels)
{
    if (glevels <= 0 || ng_cap <= 0) return ng_cap;
    int32_t lastlevel = 1;             /* first index of the deepest level */
    while (lastlevel * 2 <= ng_cap) lastlevel *= 2;
    int32_t first_global = lastlevel >> (glevels - 1);
    return first_global > 1 ? first_global - 1 : 1;   /* the root stays in LDS */
}

/* iterative search: results queue and both heaps persist in global memory */
SPTAG_HD inline LdsLayout iter_lds_layout(int dim, size_t esz, int batch)
{
    return lds_layout(dim, esz, batch, MAX_DEG, -1, false, 0);
}

/* brute-force truth: query and result set only; its four staged distances
 * sit in the scalar slot */
SPTAG_HD inline LdsLayout truth_lds_layout(int dim, size_t esz, int k)
{
    return lds_layout(dim, esz, k, 0, -1, false, 0);
}

/* persistent per-iterator device state (iterative search) */
struct IterState {
    int32_t ng_count, spt_count, checked, tree_checked;
    int32_t relaxed, first, oflow, pad;
};

/* iterative-search launch buffers: persistent state + per-call outputs */
struct IterBufs {
    const void* queries;   /* nq*dim (device, owned by the iterator batch) */
    void* gheap_ng;        /* nq * (ng_cap+1) * 8 */
    void* gheap_spt;       /* nq * (spt_cap+1) * 8 */
    float* dpq;            /* nq * (dpq_cap+1) */
    int32_t* visited;      /* nq * vcap (zeroed at create) */
    IterState* state;      /* nq */
    int32_t* out_vids;     /* nq * batch */
    float* out_dists;      /* nq * batch */
    int32_t* out_counts;   /* nq */
    int32_t* out_relaxed;  /* nq */
};

int launch_bkt_iter(int valuetype, int distmethod, const DevIndex& di,
                    const SearchCfg& cfg, const IterBufs& bufs, int batch);

/* launchers implemented in kernels.hip; return hipError_t as int */
int launch_bkt_search(int valuetype, int distmethod, bool heaps_in_lds,
                      const DevIndex& di, const SearchCfg& cfg,
                      const SearchBufs& bufs);
/* gather: dst row r = src row d_idx[r]; scatter: dst row d_idx[r] = src row r */
int launch_copy_rows(bool gather, void* dst, const void* src, int row_bytes,
                     const int32_t* d_idx, int nrows);
int launch_truth(int valuetype, int distmethod, const DevIndex& di,
                 const void* queries, int32_t nq, int32_t k,
                 int32_t* out_vids, float* out_dists);

/* shard merge: at most MAX_SHARDS lists per query; the lists of one query
 * are staged in LDS up to MERGE_LDS_ENTRIES entries of 8 bytes (32 KiB) */
enum { MAX_SHARDS = 64, MERGE_LDS_ENTRIES = 4096 };

/* global id of a shard's vector 0, per shard; passed to the kernel by value */
struct MergeBases { int32_t b[MAX_SHARDS]; };

/* vids/dists: [nshards][nq][k_in] on the current device, each list ascending
 * (dist, vid) with a vid < 0 padding suffix; out: [nq][k_out], which must
 * not overlap the inputs */
int launch_merge_topk(const int32_t* vids, const float* dists,
                      const MergeBases& bases, int nshards, int32_t nq,
                      int32_t k_in, int32_t k_out, int32_t* out_vids,
                      float* out_dists);

/* heap probe (tests/test_gpu_heap_ops.py): a script of nops heap operations
 * (ops[i] != 0: insert {nodes[i], dists[i]}; 0: pop) on a heap of capacity
 * `cap` whose entries [0..lsplit] sit in LDS (lsplit 0: none), run once with
 * the serial heap functions (block 0) and once with the wave-wide ones
 * (block 1). All pointers are device memory: heaps [2][cap+1] entries of
 * {int32 node, float distance}, pops [2][nops] entries (written at pop ops
 * only), final [2] x {count, overflow flag}, zeroed by the caller. */
enum { HEAP_PROBE_MAX_CAP = 1 << 20, HEAP_PROBE_MAX_LSPLIT = 4095 };
struct HeapProbeArgs {
    int32_t cap, ref_cap, lsplit, nops;
    const int32_t* ops;
    const int32_t* nodes;
    const float* dists;
    void* heaps;
    void* pops;
    int32_t* final;
};
int launch_heap_probe(const HeapProbeArgs& args);

/* host entry of the probe, all pointers host memory; exported for the tests
 * and deliberately not part of include/sptag_amd.h */
extern "C" int sptagamd_dbg_heap_probe(int device, int32_t cap, int32_t ref_cap,
                                       int32_t lsplit, int32_t nops, const int32_t* ops,
                                       const int32_t* nodes, const float* dists,
                                       void* out_heaps, void* out_pops,
                                       int32_t* out_final);

}  /* namespace sptag_amd */
