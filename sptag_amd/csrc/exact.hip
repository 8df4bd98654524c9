/* sptag_amd exact search — tiled brute-force top-k for gfx950 (MI355X).
 *
 * Same answer as truth_kernel (kernels.hip), bit for bit: over the
 * non-deleted rows, ascending (dist, vid), distances in the reference's
 * summation order, vid = -1 at MaxDist as padding. Where truth_kernel gives a
 * query one wave that reads the whole index, a workgroup here owns a tile of
 * XQT queries and a slice of the rows, so a row read from HBM serves XQT
 * queries, and a grid of (query tiles) x (slices) fills the device at any nq.
 * Every (slice, query) leaves one sorted k-list in a [S][nq][k] buffer that
 * merge_topk_kernel merges with all bases 0 (the vids are global already).
 *
 * Distances
 *   f32: vector ALUs, in the reference order. A 16-lane group owns an 8 x 4
 *        (queries x rows) micro-tile; lane g holds, for each of the 32 pairs,
 *        accumulator g of the reference's 16 (column c*16+g of every chunk
 *        c), so a chunk costs 12 LDS reads for 64 sub/fma pairs. The
 *        dimension streams through LDS in slabs of FKS columns with the
 *        accumulators kept, then each pair is folded 16->8, 8-tail, 8->4,
 *        4-tail, ((a0+a1)+a2)+a3, scalar tail, with DPP row shifts.
 *   int8: v_mfma_i32_32x32x32_i8, queries as A, rows as B; a wave owns 32
 *        rows of the tile. Integer dots are exact and order-free, so
 *        (float)(16129 - dot) and (float)(aa - 2ab + bb) are ref_dist_grp_i8's
 *        values; A and B use the same lane/byte -> k assignment, which is
 *        all a dot product needs of it. K is zero-filled up to 32.
 *
 * Selection
 *   Rows reach a query in ascending vid inside a slice. thr[q] is the k-th
 *   distance of the query's list (MaxDist until it holds k rows). A row
 *   enters only with dist < thr: with dist == thr every list entry has a
 *   key (dist', vid') below (dist, vid), because dist' <= thr and vid' < vid,
 *   so the row is not among the k smallest; a stale (larger) thr only lets
 *   more through. Survivors are appended to a per-query buffer of XCB
 *   candidates in LDS; the wave that owns the query merges a buffer at
 *   XFLUSH and at the slice end into the sorted list by rank. The lists live
 *   in the [S][nq][k] buffer itself, in global memory: they are touched only
 *   by merges, which are rare after the first tiles, and so one path serves
 *   every k <= MAX_K.
 *
 * Grouped kNN (all pairs inside row groups, the index builder's leaf step)
 * runs on the same tiles and the same selection, with gathered loads and
 * the lists in the output rows: see its section below.
 */
#include <hip/hip_runtime.h>

#include "common.h"

namespace sptag_amd {

#define DEV __device__ __forceinline__

static constexpr float MAXDIST = __FLT_MAX__ / 10.0f; /* Common.h:122 */

enum {
    XQT = EXACT_QT,      /* queries of a workgroup */
    XTHREADS = 256,      /* four waves */
    XWAVES = XTHREADS / 64,
    XCB = 64,            /* candidates buffered per query: one per lane of a merge */
    XFLUSH = 32,         /* merge a buffer that holds this many */
};

/* ------------------------------------------------------------------ *
 * selection
 * ------------------------------------------------------------------ */

struct XCand { float dist; int32_t vid; };

struct XSel {
    float* thr;      /* LDS [XQT] */
    int* cnt;        /* LDS [XQT]; may run past XCB, entries past it were not stored */
    XCand* cand;     /* LDS [XQT][XCB] */
    int32_t* lv;     /* the lists; query ql's is row qrow[ql] of k entries */
    float* ld;
    int k;
    int nql;         /* queries of the tile that exist */
    const int32_t* qrow;   /* LDS [XQT]; null: row ql (exact search, whose lv/ld
                              start at its (slice, query tile)) */
};

DEV size_t sel_list_at(const XSel& s, int ql)
{
    return (size_t)(s.qrow ? s.qrow[ql] : ql) * s.k;
}

/* (da, va) ordered before (db, vb); vids are distinct, so this is total */
DEV bool key_before(float da, int32_t va, float db, int32_t vb)
{
    return da < db || (da == db && va < vb);
}

DEV float wave_bcast(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

/* An f32 as an unsigned key of the same order (negative distances included),
 * -0 folded to +0; the pool join's keys and the sorted grouped selection's. */
DEV uint32_t dist_key(float dist)
{
    const uint32_t b = dist == 0.0f ? 0u : (uint32_t)__float_as_int(dist);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEV float dist_unkey(uint32_t b)
{
    return __int_as_float((int)((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b));
}

/* One wave merges n <= 64 candidates (any order, keys distinct from the
 * list's) into the sorted list lv/ld of k entries, in place. The new place of
 * a list entry is its index plus the candidates before it, of a candidate
 * the list entries before it (a binary search) plus the candidates before
 * it; places >= k fall out. Padding (vid < 0) is after everything. Entries
 * only move up, by at most n <= 64, so 64-entry chunks are rewritten top
 * down: what a chunk's stores overwrite was read in this step or an earlier
 * one. A chunk in which nothing moves is below every candidate, and so is
 * everything under it. The candidates, whose places may lie in chunks not
 * read yet, go in last. */
DEV void merge_cands(int32_t* lv, float* ld, int k, const XCand* cb, int n)
{
    const int lane = threadIdx.x & 63;
    XCand c = lane < n ? cb[lane] : XCand{MAXDIST, -1};
    int rank = 0;
    for (int j = 0; j < n; j++)
        rank += key_before(wave_bcast(c.dist, j), __builtin_amdgcn_readlane(c.vid, j),
                           c.dist, c.vid);
    int lo = 0, hi = k;             /* first list entry not before c */
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        int32_t ev = lv[mid];
        float ed = ld[mid];
        if (ev >= 0 && key_before(ed, ev, c.dist, c.vid)) lo = mid + 1;
        else hi = mid;
    }
    rank += lo;
    for (int base = (k - 1) & ~63; base >= 0; base -= 64) {
        const int i = base + lane;
        const bool in = i < k;
        int32_t ev = in ? lv[i] : -1;
        float ed = in ? ld[i] : MAXDIST;
        int up = 0;
        for (int j = 0; j < n; j++)
            up += key_before(wave_bcast(c.dist, j), __builtin_amdgcn_readlane(c.vid, j),
                             ed, ev);
        if (ev < 0) up = n;
        if (!__ballot(in && up != 0)) break;
        if (in && i + up < k) { lv[i + up] = ev; ld[i + up] = ed; }
    }
    if (lane < n && rank < k) { lv[rank] = c.vid; ld[rank] = c.dist; }
    /* the next merge of this list reads it through other lanes */
    __threadfence();
}

/* Every wave merges the buffers of its queries (ql = wave, wave + XWAVES, ..)
 * that hold at least `level` candidates and refreshes their thresholds. */
DEV void flush_cands(const XSel& s, int level)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int ql = wave; ql < s.nql; ql += XWAVES) {
        const int n = min(__builtin_amdgcn_readfirstlane(s.cnt[ql]), (int)XCB);
        if (n < level || n == 0) continue;
        int32_t* lv = s.lv + sel_list_at(s, ql);
        float* ld = s.ld + sel_list_at(s, ql);
        merge_cands(lv, ld, s.k, s.cand + ql * XCB, n);
        const float kth = ld[s.k - 1];
        if (lane == 0) { s.cnt[ql] = 0; s.thr[ql] = kth; }
    }
}

/* Empty lists, empty buffers, thresholds at MaxDist. Ends with a barrier. */
DEV void sel_init(const XSel& s)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < XQT) { s.thr[threadIdx.x] = MAXDIST; s.cnt[threadIdx.x] = 0; }
    for (int ql = wave; ql < s.nql; ql += XWAVES) {
        const size_t at = sel_list_at(s, ql);
        for (int i = lane; i < s.k; i += 64) {
            s.lv[at + i] = -1;
            s.ld[at + i] = MAXDIST;
        }
    }
    __threadfence();
    __syncthreads();
}

/* Called by every thread after a tile: bit m of `pend` says that this lane's
 * pair m (query ql[m] of the tile, row vid[m], distance dist[m]) passed its
 * threshold. A pair that finds its query's buffer full stays pending while
 * the owner merges the buffer, and goes in on the next round without a
 * second threshold test: the threshold may by then stem from a later row of
 * the same tile. Ends with a barrier. */
template <int NP>
DEV void sel_append(const XSel& s, uint32_t pend, const float (&dist)[NP],
                    const int (&ql)[NP], const int32_t (&vid)[NP])
{
    for (;;) {
#pragma unroll
        for (int m = 0; m < NP; m++) {
            if (!((pend >> m) & 1)) continue;
            const int slot = atomicAdd(&s.cnt[ql[m]], 1);
            if (slot < XCB) {
                s.cand[ql[m] * XCB + slot] = XCand{dist[m], vid[m]};
                pend &= ~(1u << m);
            }
        }
        const int again = __syncthreads_or(pend != 0);
        flush_cands(s, XFLUSH);
        __syncthreads();
        if (!again) break;
    }
}

/* rows [r0, r1) of slice blockIdx.y */
DEV void slice_rows(int32_t n, int32_t rows_per_slice, int32_t& r0, int32_t& r1)
{
    const int64_t b = (int64_t)blockIdx.y * rows_per_slice;
    r0 = (int32_t)min(b, (int64_t)n);
    r1 = (int32_t)min(b + rows_per_slice, (int64_t)n);
}

DEV XSel make_sel(unsigned char* lds, uint32_t thr, uint32_t cnt, uint32_t cand,
                  int32_t* lists_v, float* lists_d, int32_t nq, int32_t k, int q0)
{
    XSel s;
    s.thr = (float*)(lds + thr);
    s.cnt = (int*)(lds + cnt);
    s.cand = (XCand*)(lds + cand);
    const size_t at = ((size_t)blockIdx.y * nq + q0) * k;
    s.lv = lists_v + at;
    s.ld = lists_d + at;
    s.k = k;
    s.nql = min((int)XQT, nq - q0);
    s.qrow = nullptr;
    return s;
}

/* ------------------------------------------------------------------ *
 * f32
 * ------------------------------------------------------------------ */

enum {
    FMQ = 8, FMR = 4,   /* a group's micro-tile: queries gq + 4*i, rows 4*wave + j */
    FRT = 16,     /* rows of a tile: 4 waves x FMR */
    FKS = 64,     /* columns of a slab: four chunks of 16 */
    FQSS = 80,    /* row stride of a streamed query slab */
    FQRES_MAX = 256,   /* largest resident query row stride (32 KiB of LDS) */
};

/* Row stride of the resident query tile: the dim rounded up to whole chunks,
 * and an odd number of them, so that the four groups of a wave, which read
 * queries one row apart, sit 16 banks apart. */
static inline __host__ __device__ int f32_qstride(int d)
{
    const int p = (d + 15) & ~15;
    return ((p >> 4) & 1) ? p : p + 16;
}

struct F32Lds { uint32_t q, rows, thr, cnt, cand, total; };

static inline __host__ __device__ F32Lds f32_lds(int d)
{
    F32Lds l;
    const int qs = f32_qstride(d);
    uint32_t b = 0;
    l.q = b;    b += (qs <= FQRES_MAX ? XQT * qs : 2 * XQT * FQSS) * 4;
    l.rows = b; b += 2 * FRT * FKS * 4;
    l.thr = b;  b += XQT * 4;
    l.cnt = b;  b += XQT * 4;
    l.cand = b; b += XQT * XCB * 8;
    l.total = b;
    return l;
}

/* the fused per-element step of both metrics (acc<DM> of kernels.hip) */
template <int DM>
DEV float xstep(float x, float y, float a)
{
    return (DM == DM_L2) ? fmaf(x - y, x - y, a) : fmaf(x, y, a);
}

template <int CTRL>
DEV float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf,
                                                      true));
}
enum { DPP_ROW_SHL8 = 0x108, DPP_ROW_SHL4 = 0x104,     /* lane g reads lane g + n */
       DPP_QUAD0 = 0x00, DPP_QUAD1 = 0x55, DPP_QUAD2 = 0xaa, DPP_QUAD3 = 0xff };

/* The gathered form of f32_slab_load below (grouped kNN): columns
 * k0 + 4*(tid%16) .. +3 of the row of d floats at `row`, zero past d and for
 * a null row. vec: the row and the columns are 16-byte aligned. */
DEV float4 f32_cols_load(const float* __restrict__ row, int d, int k0, bool vec)
{
    const int c = k0 + (threadIdx.x & 15) * 4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row && c < d) {
        const float* p = row + c;
        if (vec) {
            v = *(const float4*)p;
        } else {
            v.x = p[0];
            if (c + 1 < d) v.y = p[1];
            if (c + 2 < d) v.z = p[2];
            if (c + 3 < d) v.w = p[3];
        }
    }
    return v;
}

/* The block's threads cover 16 rows x FKS columns with four columns each:
 * this thread's are row r = r16 + tid/16, columns k0 + 4*(tid%16) .. +3 of
 * `base`'s rows (row pitch d), zero outside nrows x d. vec: rows and columns
 * are 16-byte aligned. */
DEV float4 f32_slab_load(const float* __restrict__ base, int nrows, int d, int k0, bool vec,
                         int r16 = 0)
{
    const int r = r16 + (threadIdx.x >> 4), c = k0 + (threadIdx.x & 15) * 4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < nrows && c < d) {
        const float* p = base + (size_t)r * d + c;
        if (vec) {
            v = *(const float4*)p;
        } else {
            v.x = p[0];
            if (c + 1 < d) v.y = p[1];
            if (c + 2 < d) v.z = p[2];
            if (c + 3 < d) v.w = p[3];
        }
    }
    return v;
}

DEV void f32_slab_store(float* buf, int stride, float4 v, int r16 = 0)
{
    *(float4*)(buf + (r16 + (threadIdx.x >> 4)) * stride + (threadIdx.x & 15) * 4) = v;
}

/* f32_slab_math and f32_fold are the grouped-kNN kernel's statement of the
 * slab loop and the fold that exact_f32_kernel spells out in its body. With
 * both kernels calling them, and f32_slab_load going through f32_cols_load,
 * the compiler scheduled exact_f32_kernel differently and exact search came
 * out 6% slower (profiles/group_knn.txt), so that kernel keeps its text; the
 * tests pin both to the same reference bits.
 *
 * One slab of a group's micro-tile: the whole 16-column chunks of slab `slab`
 * (columns slab*FKS ..) go into lane g's accumulators, cleared at slab 0.
 * qb: this group's query gq of the slab (query gq + 4*i at + 4*i*qstride);
 * rb: this wave's first row of the slab (row j at + j*FKS). */
template <int DM>
DEV void f32_slab_math(float (&acc)[FMQ][FMR], const float* qb, const float* rb, int qstride,
                       int slab, int d, int g)
{
    if (slab == 0) {
#pragma unroll
        for (int i = 0; i < FMQ; i++)
#pragma unroll
            for (int j = 0; j < FMR; j++) acc[i][j] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < FKS / 16; c++) {
        if (slab * FKS + c * 16 + 16 > d) break;
        float x[FMQ], y[FMR];
#pragma unroll
        for (int i = 0; i < FMQ; i++) x[i] = qb[4 * i * qstride + c * 16 + g];
#pragma unroll
        for (int j = 0; j < FMR; j++) y[j] = rb[j * FKS + c * 16 + g];
#pragma unroll
        for (int i = 0; i < FMQ; i++)
#pragma unroll
            for (int j = 0; j < FMR; j++) acc[i][j] = xstep<DM>(x[i], y[j], acc[i][j]);
    }
}

/* After the last slab: the reference's folds and tails. dist[i] on lane
 * g < FMR is the distance of query gq + 4*i to row g of the wave's four. */
template <int DM>
DEV void f32_fold(const float (&acc)[FMQ][FMR], const float* qb, const float* rb, int qstride,
                  int slab, int d, int g, float (&dist)[FMQ])
{
    const int nd16 = d & ~15, nd8 = d & ~7, nd4 = d & ~3;
    /* the tails' columns sit in this slab, from tc on */
    const int tc = nd16 - slab * FKS;
    float x8[FMQ], x4[FMQ], y8[FMR], y4[FMR];
#pragma unroll
    for (int i = 0; i < FMQ; i++) {
        x8[i] = (nd8 > nd16 && g < 8) ? qb[4 * i * qstride + tc + g] : 0.0f;
        x4[i] = (nd4 > nd8 && g < 4) ? qb[4 * i * qstride + tc + (nd8 - nd16) + g] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < FMR; j++) {
        y8[j] = (nd8 > nd16 && g < 8) ? rb[j * FKS + tc + g] : 0.0f;
        y4[j] = (nd4 > nd8 && g < 4) ? rb[j * FKS + tc + (nd8 - nd16) + g] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < FMQ; i++) {
        float mine = 0.0f;
#pragma unroll
        for (int j = 0; j < FMR; j++) {
            float a = acc[i][j];
            a = a + dpp<DPP_ROW_SHL8>(a);               /* a8[g] on g < 8 */
            if (nd8 > nd16) a = xstep<DM>(x8[i], y8[j], a);
            a = a + dpp<DPP_ROW_SHL4>(a);               /* a4[g] on g < 4 */
            if (nd4 > nd8) a = xstep<DM>(x4[i], y4[j], a);
            const float s = ((dpp<DPP_QUAD0>(a) + dpp<DPP_QUAD1>(a)) +
                             dpp<DPP_QUAD2>(a)) + dpp<DPP_QUAD3>(a);
            mine = (j == 0 || g == j) ? s : mine;
        }
        for (int c = nd4; c < d; c++)
            mine = xstep<DM>(qb[4 * i * qstride + (c - slab * FKS)],
                             rb[(g & 3) * FKS + (c - slab * FKS)], mine);
        dist[i] = (DM == DM_L2) ? mine : 1.0f - mine;
    }
}

/* QRES: the whole query tile stays in LDS; otherwise (large dims) its slab
 * streams with the rows' slab. */
template <int DM, bool QRES>
__global__ __launch_bounds__(XTHREADS, 2)
void exact_f32_kernel(DevIndex di, const float* __restrict__ queries, int32_t nq, int32_t k,
                      int32_t rows_per_slice, int32_t* lists_v, float* lists_d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int d = di.dim;
    const F32Lds L = f32_lds(d);
    float* qlds = (float*)(xlds + L.q);
    float* rlds = (float*)(xlds + L.rows);
    const int tid = threadIdx.x;
    const int g = tid & 15, gq = (tid >> 4) & 3, gr = tid >> 6;
    const int q0 = blockIdx.x * XQT;
    const XSel sel = make_sel(xlds, L.thr, L.cnt, L.cand, lists_v, lists_d, nq, k, q0);
    int32_t r0, r1;
    slice_rows(di.n, rows_per_slice, r0, r1);
    const float* vectors = (const float*)di.vectors;
    const bool vecv = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;
    const bool vecq = (d & 3) == 0 && ((uintptr_t)queries & 15) == 0;
    const int qstride = QRES ? f32_qstride(d) : FQSS;

    if constexpr (QRES) {
        for (int i = tid; i < XQT * qstride; i += XTHREADS) {
            const int r = i / qstride, c = i - r * qstride;
            qlds[i] = (r < sel.nql && c < d) ? queries[(size_t)(q0 + r) * d + c] : 0.0f;
        }
    }
    sel_init(sel);

    const int nslab = (d + FKS - 1) / FKS;
    const int ntile = (r1 - r0 + FRT - 1) / FRT;
    const int nstep = ntile * nslab;
    const int nd16 = d & ~15, nd8 = d & ~7, nd4 = d & ~3;
    const float* qbase = queries + (size_t)q0 * d;

    float acc[FMQ][FMR];
    float4 pr = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pq0 = pr, pq1 = pr;
    if (nstep > 0) {
        pr = f32_slab_load(vectors + (size_t)r0 * d, min((int)FRT, r1 - r0), d, 0, vecv);
        f32_slab_store(rlds, FKS, pr);
        if constexpr (!QRES) {
            pq0 = f32_slab_load(qbase, sel.nql, d, 0, vecq, 0);
            pq1 = f32_slab_load(qbase, sel.nql, d, 0, vecq, 16);
            f32_slab_store(qlds, FQSS, pq0, 0);
            f32_slab_store(qlds, FQSS, pq1, 16);
        }
    }
    __syncthreads();

    int tile = 0, slab = 0;
    for (int st = 0; st < nstep; st++) {
        int ntl = tile, nsl = slab + 1;
        if (nsl == nslab) { nsl = 0; ntl++; }
        const bool more = st + 1 < nstep;
        if (more) {     /* in flight while this slab computes */
            const int tr0 = r0 + ntl * FRT;
            pr = f32_slab_load(vectors + (size_t)tr0 * d, min((int)FRT, r1 - tr0), d,
                               nsl * FKS, vecv);
            if constexpr (!QRES) {
                pq0 = f32_slab_load(qbase, sel.nql, d, nsl * FKS, vecq, 0);
                pq1 = f32_slab_load(qbase, sel.nql, d, nsl * FKS, vecq, 16);
            }
        }
        const float* rb = rlds + (st & 1) * (FRT * FKS) + (gr * FMR) * FKS;
        const float* qb = (QRES ? qlds + slab * FKS : qlds + (st & 1) * (XQT * FQSS)) +
                          gq * qstride;          /* query gq + 4*i at + 4*i*qstride */
        if (slab == 0) {
#pragma unroll
            for (int i = 0; i < FMQ; i++)
#pragma unroll
                for (int j = 0; j < FMR; j++) acc[i][j] = 0.0f;
        }
#pragma unroll
        for (int c = 0; c < FKS / 16; c++) {
            if (slab * FKS + c * 16 + 16 > d) break;
            float x[FMQ], y[FMR];
#pragma unroll
            for (int i = 0; i < FMQ; i++) x[i] = qb[4 * i * qstride + c * 16 + g];
#pragma unroll
            for (int j = 0; j < FMR; j++) y[j] = rb[j * FKS + c * 16 + g];
#pragma unroll
            for (int i = 0; i < FMQ; i++)
#pragma unroll
                for (int j = 0; j < FMR; j++) acc[i][j] = xstep<DM>(x[i], y[j], acc[i][j]);
        }

        if (slab == nslab - 1) {
            /* the tails' columns sit in this slab, from tc on */
            const int tc = nd16 - slab * FKS;
            float x8[FMQ], x4[FMQ], y8[FMR], y4[FMR];
#pragma unroll
            for (int i = 0; i < FMQ; i++) {
                x8[i] = (nd8 > nd16 && g < 8) ? qb[4 * i * qstride + tc + g] : 0.0f;
                x4[i] = (nd4 > nd8 && g < 4) ? qb[4 * i * qstride + tc + (nd8 - nd16) + g] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < FMR; j++) {
                y8[j] = (nd8 > nd16 && g < 8) ? rb[j * FKS + tc + g] : 0.0f;
                y4[j] = (nd4 > nd8 && g < 4) ? rb[j * FKS + tc + (nd8 - nd16) + g] : 0.0f;
            }
            /* lane g < FMR of the group keeps the pairs of row g: pair i is
             * query gq + 4*i against row 4*wave + g of the tile */
            float dist[FMQ];
            int ql[FMQ];
            int32_t vid[FMQ];
            uint32_t pend = 0;
            const int32_t myrow = r0 + tile * FRT + gr * FMR + (g & 3);
#pragma unroll
            for (int i = 0; i < FMQ; i++) {
                float mine = 0.0f;
#pragma unroll
                for (int j = 0; j < FMR; j++) {
                    float a = acc[i][j];
                    a = a + dpp<DPP_ROW_SHL8>(a);               /* a8[g] on g < 8 */
                    if (nd8 > nd16) a = xstep<DM>(x8[i], y8[j], a);
                    a = a + dpp<DPP_ROW_SHL4>(a);               /* a4[g] on g < 4 */
                    if (nd4 > nd8) a = xstep<DM>(x4[i], y4[j], a);
                    const float s = ((dpp<DPP_QUAD0>(a) + dpp<DPP_QUAD1>(a)) +
                                     dpp<DPP_QUAD2>(a)) + dpp<DPP_QUAD3>(a);
                    mine = (j == 0 || g == j) ? s : mine;
                }
                for (int c = nd4; c < d; c++)
                    mine = xstep<DM>(qb[4 * i * qstride + (c - slab * FKS)],
                                     rb[(g & 3) * FKS + (c - slab * FKS)], mine);
                dist[i] = (DM == DM_L2) ? mine : 1.0f - mine;
                ql[i] = gq + 4 * i;
                vid[i] = myrow;
                if (g < FMR && myrow < r1 && ql[i] < sel.nql && dist[i] < sel.thr[ql[i]] &&
                    !(di.has_deleted && di.deleted[myrow]))
                    pend |= 1u << i;
            }
            sel_append(sel, pend, dist, ql, vid);
        }

        if (more) {
            f32_slab_store(rlds + ((st + 1) & 1) * (FRT * FKS), FKS, pr);
            if constexpr (!QRES) {
                f32_slab_store(qlds + ((st + 1) & 1) * (XQT * FQSS), FQSS, pq0, 0);
                f32_slab_store(qlds + ((st + 1) & 1) * (XQT * FQSS), FQSS, pq1, 16);
            }
        }
        __syncthreads();
        tile = ntl;
        slab = nsl;
    }
    flush_cands(sel, 1);
}

/* ------------------------------------------------------------------ *
 * int8
 * ------------------------------------------------------------------ */

enum {
    IRT = 128,               /* rows of a tile: 4 waves x one 32-row MFMA block */
    I_MAX_W = 65,            /* dwords of a row at the int8 dim guard (260) */
    I_NCH = (IRT * I_MAX_W * 4 + XTHREADS * 16 - 1) / (XTHREADS * 16),   /* 16-byte chunks per thread */
};
static_assert(IRT == EXACT_ROW_ALIGN, "slices start on int8 tile boundaries");
static_assert(IRT % FRT == 0, "and on f32 ones");

struct I8Lds { uint32_t q, rows, aa, thr, cnt, cand, total; };

/* rows and queries are stored as dwords, W = ceil(d/4) to a row, at an odd
 * row stride so that the 32 rows an MFMA operand reads fall in 32 banks */
static inline __host__ __device__ I8Lds i8_lds(int d)
{
    I8Lds l;
    const uint32_t wl = (uint32_t)((d + 3) >> 2) | 1;
    uint32_t b = 0;
    l.q = b;    b += XQT * wl * 4;
    l.rows = b; b += IRT * wl * 4;
    l.aa = b;   b += XQT * 4;
    l.thr = b;  b += XQT * 4;
    l.cnt = b;  b += XQT * 4;
    l.cand = b; b += XQT * XCB * 8;
    l.total = b;
    return l;
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

/* dword w of row r of an int8 array of pitch d bytes, bytes past d zero;
 * byte loads, for pitches that are not a multiple of 4 */
DEV uint32_t i8_pack_dword(const int8_t* __restrict__ base, int r, int w, int d)
{
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
        const int c = 4 * w + b;
        if (c < d) v |= (uint32_t)(uint8_t)base[(size_t)r * d + c] << (8 * b);
    }
    return v;
}

/* four dwords at dword offset kb of a row of W dwords, zero past the row */
DEV v4i i8_operand(const uint32_t* row, int kb, int W)
{
    v4i v;
    v.x = kb < W ? (int)row[kb] : 0;
    v.y = kb + 1 < W ? (int)row[kb + 1] : 0;
    v.z = kb + 2 < W ? (int)row[kb + 2] : 0;
    v.w = kb + 3 < W ? (int)row[kb + 3] : 0;
    return v;
}

/* A wave's 32 queries x 32 rows of dots: arow/brow are this lane's query and
 * row (lane % 32) in LDS, h = lane / 32 the half of each 32-byte K step it
 * feeds. bb (L2): the row's self-dot. */
template <int DM>
DEV void i8_tile_dots(const uint32_t* arow, const uint32_t* brow, int W, int h, v16i& acc,
                      int& bb)
{
    acc = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bb = 0;
    const int nks = (W + 7) >> 3;
    for (int ks = 0; ks < nks; ks++) {
        const int kb = ks * 8 + h * 4;
        const v4i a = i8_operand(arow, kb, W);
        const v4i b = i8_operand(brow, kb, W);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
        if (DM == DM_L2) {
            bb = __builtin_amdgcn_sdot4(b.x, b.x, bb, false);
            bb = __builtin_amdgcn_sdot4(b.y, b.y, bb, false);
            bb = __builtin_amdgcn_sdot4(b.z, b.z, bb, false);
            bb = __builtin_amdgcn_sdot4(b.w, b.w, bb, false);
        }
    }
    if (DM == DM_L2) bb += __shfl_xor(bb, 32);      /* both halves of the row's bytes */
}

template <int DM>
__global__ __launch_bounds__(XTHREADS, 2)
void exact_i8_kernel(DevIndex di, const int8_t* __restrict__ queries, int32_t nq, int32_t k,
                     int32_t rows_per_slice, int32_t* lists_v, float* lists_d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int d = di.dim;
    const I8Lds L = i8_lds(d);
    uint32_t* qlds = (uint32_t*)(xlds + L.q);
    uint32_t* rlds = (uint32_t*)(xlds + L.rows);
    int* aa = (int*)(xlds + L.aa);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * XQT;
    const XSel sel = make_sel(xlds, L.thr, L.cnt, L.cand, lists_v, lists_d, nq, k, q0);
    int32_t r0, r1;
    slice_rows(di.n, rows_per_slice, r0, r1);
    const int8_t* vectors = (const int8_t*)di.vectors;
    const int W = (d + 3) >> 2, WL = W | 1;
    /* A tile's rows are one contiguous byte range that starts on a multiple
     * of IRT * d bytes, so with whole dwords to a row it is copied flat, 16
     * bytes at a time, and scattered to the padded rows in LDS. */
    const bool flat = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;

    for (int i = tid; i < XQT * W; i += XTHREADS) {
        const int r = i / W, w = i - r * W;
        qlds[r * WL + w] = r < sel.nql ? i8_pack_dword(queries + (size_t)q0 * d, r, w, d) : 0u;
    }
    sel_init(sel);
    if (tid < XQT) {        /* query self-dots, for L2 */
        int s = 0;
        for (int w = 0; w < W; w++) {
            const int v = (int)qlds[tid * WL + w];
            s = __builtin_amdgcn_sdot4(v, v, s, false);
        }
        aa[tid] = s;
    }

    /* flat copy: chunk c of this thread is dwords 4*(tid + c*XTHREADS) .. +3
     * of the tile; (fr, fw) is the row and dword of the first */
    const int fr0 = (4 * tid) / W, fw0 = (4 * tid) - fr0 * W;
    const int fdr = (4 * XTHREADS) / W, fdw = (4 * XTHREADS) - fdr * W;
    uint4 pre[I_NCH];
    auto stage_load = [&](int tr0) {
        if (!flat) return;
        const uint32_t valid = (uint32_t)min((int)IRT, r1 - tr0) * (uint32_t)d;   /* bytes */
        const unsigned char* src = (const unsigned char*)vectors + (size_t)tr0 * d;
#pragma unroll
        for (int c = 0; c < I_NCH; c++) {
            const uint32_t off = (uint32_t)(tid + c * XTHREADS) * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (off + 16 <= valid) {
                v = *(const uint4*)(src + off);
            } else if (off < valid) {       /* valid is a multiple of 4 */
                v.x = *(const uint32_t*)(src + off);
                if (off + 4 < valid) v.y = *(const uint32_t*)(src + off + 4);
                if (off + 8 < valid) v.z = *(const uint32_t*)(src + off + 8);
            }
            pre[c] = v;
        }
    };
    auto stage_store = [&](int tr0) {
        const int nrows = min((int)IRT, r1 - tr0);
        if (!flat) {
            for (int i = tid; i < nrows * W; i += XTHREADS) {
                const int r = i / W, w = i - r * W;
                rlds[r * WL + w] = i8_pack_dword(vectors + (size_t)tr0 * d, r, w, d);
            }
            return;
        }
        int fr = fr0, fw = fw0;
#pragma unroll
        for (int c = 0; c < I_NCH; c++) {
            const uint32_t v[4] = {pre[c].x, pre[c].y, pre[c].z, pre[c].w};
            int r = fr, w = fw;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                while (w >= W) { w -= W; r++; }
                if (r < nrows) rlds[r * WL + w] = v[j];
                w++;
            }
            fr += fdr;
            fw += fdw;
            if (fw >= W) { fw -= W; fr++; }
        }
    };

    const int ntile = (r1 - r0 + IRT - 1) / IRT;
    if (ntile > 0) {
        stage_load(r0);
        stage_store(r0);
    }
    __syncthreads();

    const int h = lane >> 5, col = lane & 31;
    const uint32_t* arow = qlds + col * WL;
    const uint32_t* brow = rlds + (wave * 32 + col) * WL;
    for (int t = 0; t < ntile; t++) {
        const int tr0 = r0 + t * IRT;
        if (t + 1 < ntile) stage_load(tr0 + IRT);   /* in flight while this tile computes */

        v16i acc;
        int bb;
        i8_tile_dots<DM>(arow, brow, W, h, acc, bb);

        /* acc[r] is query 8*(r/4) + 4*h + r%4 against row `col` of the wave's 32 */
        uint32_t pend = 0;
        float dist[16];
        int ql[16];
        int32_t vid[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            ql[r] = 8 * (r >> 2) + 4 * h + (r & 3);
            vid[r] = tr0 + wave * 32 + col;
            dist[r] = (DM == DM_L2) ? (float)(aa[ql[r]] - 2 * acc[r] + bb)
                                    : (float)(16129 - acc[r]);
            if (vid[r] < r1 && ql[r] < sel.nql && dist[r] < sel.thr[ql[r]] &&
                !(di.has_deleted && di.deleted[vid[r]]))
                pend |= 1u << r;
        }
        sel_append(sel, pend, dist, ql, vid);   /* ends with a barrier: the tile is free */

        if (t + 1 < ntile) stage_store(tr0 + IRT);
        __syncthreads();
    }
    flush_cands(sel, 1);
}

/* ------------------------------------------------------------------ *
 * grouped kNN: all pairs inside row groups
 * ------------------------------------------------------------------ *
 * Group g is members[start : start + count], vids in any order; the answer
 * of a member is its k nearest other members, in row `vid` of out[n][k]. A
 * workgroup owns one GroupTile: XQT consecutive members of one group as its
 * queries, against which it streams all members of the group as rows, with
 * the tiles and the math of the exact kernels above. What differs:
 *
 *   gather  Queries and rows are vectors[members[..]]: every row of a tile
 *           has a base of its own. The ids of a row tile are read one tile
 *           ahead of its vectors (a register for f32, whose loader thread
 *           needs one id; a double-buffered LDS array for int8, whose
 *           thread touches several rows), so the vector loads of the next
 *           tile leave before the current tile's math, as in exact search,
 *           and never wait for an id. Loads are 16 bytes where the row pitch
 *           and the base allow it, else dwords, else (int8 pitches that are
 *           no multiple of 4) bytes packed at the LDS store.
 *   lists   A query's list is its own output row (XSel::qrow = the query
 *           vids): no slices, no merge kernel. group_fill_kernel pads the
 *           whole output first, for the vids that are in no group.
 *   admit   Rows arrive in member order, not vid order, so a row enters with
 *           dist <= thr: keys are distinct, a row whose key is above the
 *           k-th falls out in the merge, which ranks by (dist, vid).
 *   self    The pair (v, v) is skipped by vid; another vid with the same
 *           vector is a neighbour at its distance.
 *
 * That is the streaming selection (SORTED = false). A leaf of the index
 * builder is the opposite of exact search's shape: about 1000 rows, k a
 * sizeable part of them, a threshold that never gets tight, so most rows cost
 * a merge. The sorted selection (SORTED = true, groups of at most
 * group_knn_sort_max members) runs the same distance phase and no admission
 * at all:
 *
 *   matrix  Every distance of the tile goes, as f32 bits, to mat[query][row
 *           position] in LDS; the self pair, and a distance the streaming
 *           form would never admit (above MaxDist, NaN), is stored as
 *           GK_WORST. The member ids of the whole group sit in LDS beside it,
 *           so a position gives its vid.
 *   select  After the last tile a wave takes the queries wave, wave + 4, ..
 *           one at a time. The query's row goes to registers as dist_key's
 *           (position lane + 64 j in register j), a bitwise radix descent
 *           with ballots finds the k-th smallest distance key, and if more
 *           rows tie there than are wanted a second descent over the vids of
 *           the ties finds the last vid to take: members come in any order.
 *           The at most k survivors are compacted by ballot, keys into the
 *           query's own row, whose values are all in registers by then, vids
 *           into the wave's scratch, which lies over the row and query tiles
 *           that the distance phase is done with.
 *   sort    Up to 64 survivors are ranked in registers (readlane, as
 *           merge_cands does); more by a bitonic network over the two LDS
 *           arrays in its always-ascending form, in which a pair whose upper
 *           index is past the survivors is a no-op, so nothing is padded to a
 *           power of two. Then the row is written; group_fill_kernel has
 *           padded it already.
 *
 * The same (dist, vid) order decides both selections, so they write the same
 * bytes. */

struct GrpLds { uint32_t qvid, mids, total; };

/* behind the exact kernel's regions: the query vids and 2 x rt row-tile ids */
static inline __host__ __device__ GrpLds grp_lds(uint32_t base, int rt)
{
    GrpLds l;
    l.qvid = base;
    l.mids = l.qvid + XQT * 4;
    l.total = l.mids + 2 * rt * 4;
    return l;
}

__global__ __launch_bounds__(256)
void group_fill_kernel(int32_t* out_v, float* out_d, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (size_t)gridDim.x * 256) {
        out_v[i] = -1;
        out_d[i] = MAXDIST;
    }
}

/* the tile's query vids into LDS (-1 past the group's end); returns how many
 * exist. Ends with a barrier. */
DEV int group_queries(const GroupTile& T, const int32_t* __restrict__ members, int32_t* qvid)
{
    const int nql = min((int)XQT, T.count - T.q0);
    if (threadIdx.x < XQT)
        qvid[threadIdx.x] = (int)threadIdx.x < nql ? members[T.start + T.q0 + threadIdx.x] : -1;
    __syncthreads();
    return nql;
}

/* The sorted selection's LDS: gfx950 gives a workgroup up to 160 KiB, and the
 * matrix takes what the launch's largest group needs of it. */
enum { GK_SORT_CAP = 1024, GK_LDS_MAX = 160 * 1024, GK_WORST = 0x7fffffff };
static constexpr uint32_t GK_KEY_WORST = 0xffffffffu;      /* dist_key of GK_WORST */
static_assert(GK_SORT_CAP <= MAX_K && GK_SORT_CAP % 64 == 0, "a row is whole 64-lane chunks");

struct SrtLds { uint32_t scratch, qvid, mids, gids, mat, total; };

/* tile_bytes: the distance phase's regions (query tile, row tiles, self-dots:
 * everything below `thr` of the exact kernels' layout), which the selection
 * reuses as XWAVES x stride words of scratch; rt: rows of a tile; stride: the
 * matrix's row stride in words, a multiple of 64 that covers every group of
 * the launch. */
static inline __host__ __device__ SrtLds srt_lds(uint32_t tile_bytes, int rt, int stride)
{
    SrtLds l;
    const uint32_t scratch = (uint32_t)XWAVES * stride * 4;
    uint32_t b = tile_bytes > scratch ? tile_bytes : scratch;
    l.scratch = 0;
    l.qvid = b; b += XQT * 4;
    l.mids = b; b += 2 * rt * 4;
    l.gids = b; b += (uint32_t)stride * 4;
    l.mat = b;  b += (uint32_t)XQT * stride * 4;
    l.total = b;
    return l;
}

/* what goes into the matrix for a pair: `other` is false for the self pair */
DEV uint32_t srt_bits(float dist, bool other)
{
    return (other && dist <= MAXDIST) ? (uint32_t)__float_as_int(dist) : (uint32_t)GK_WORST;
}

/* Orders a wave's LDS accesses against those of its other lanes: a wave's
 * LDS operations are carried out in issue order, so this only has to stop
 * the compiler moving or forwarding accesses across it. */
DEV void srt_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

/* One wave selects and writes one query's row. row: the query's `count`
 * distances as f32 bits (destroyed); gids: the group's member ids by
 * position; sv: the wave's scratch, as long as a row; ov/od: the output row,
 * all padding. NCH: 64-lane chunks that cover count. */
template <int NCH>
DEV void srt_select(uint32_t* row, const int32_t* gids, uint32_t* sv, int count, int k,
                    int32_t* ov, float* od)
{
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t key[NCH];
    int m = 0;          /* rows that may be taken at all */
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        const int pos = j * 64 + lane;
        key[j] = pos < count ? dist_key(__int_as_float((int)row[pos])) : GK_KEY_WORST;
        m += __popcll(__ballot(key[j] != GK_KEY_WORST));
    }
    const int kk = min(k, m);
    if (kk == 0) return;

    /* taken: key < P, or key == P with vid <= Q. With kk == m that is every
     * valid key: they are all below dist_key(MaxDist). */
    uint32_t P = GK_KEY_WORST - 1, Q = 0x7fffffffu;
    if (kk < m) {
        P = 0;      /* the largest P with fewer than kk keys below it: the kk-th smallest */
        for (int b = 31; b >= 0; b--) {
            const uint32_t trial = P | (1u << b);
            int c = 0;
#pragma unroll
            for (int j = 0; j < NCH; j++) c += __popcll(__ballot(key[j] < trial));
            if (c < kk) P = trial;
        }
        int less = 0, eq = 0;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            less += __popcll(__ballot(key[j] < P));
            eq += __popcll(__ballot(key[j] == P));
        }
        const int need = kk - less;     /* >= 1 of the eq ties */
        if (eq > need) {                /* the need-th smallest vid among them */
            uint32_t tv[NCH];
#pragma unroll
            for (int j = 0; j < NCH; j++)
                tv[j] = key[j] == P ? (uint32_t)gids[j * 64 + lane] : 0xffffffffu;
            Q = 0;
            for (int b = 30; b >= 0; b--) {
                const uint32_t trial = Q | (1u << b);
                int c = 0;
#pragma unroll
                for (int j = 0; j < NCH; j++) c += __popcll(__ballot(tv[j] < trial));
                if (c < need) Q = trial;
            }
        }
    }

    srt_fence();        /* the previous query's reads of sv are behind us */
    int base = 0;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        const int pos = j * 64 + lane;
        const uint32_t v = key[j] != GK_KEY_WORST ? (uint32_t)gids[pos] : 0u;
        const bool take = key[j] < P || (key[j] == P && v <= Q);
        const uint64_t mask = __ballot(take);
        if (take) {
            const int p = base + __popcll(mask & below);
            row[p] = key[j];
            sv[p] = v;
        }
        base += __popcll(mask);
    }
    srt_fence();

    if (kk <= 64) {     /* one survivor to a lane: its rank is its place */
        const uint32_t dk = lane < kk ? row[lane] : GK_KEY_WORST;
        const uint32_t dv = lane < kk ? sv[lane] : 0xffffffffu;
        int rank = 0;
        for (int j = 0; j < kk; j++) {
            const uint32_t jk = (uint32_t)__builtin_amdgcn_readlane((int)dk, j);
            const uint32_t jv = (uint32_t)__builtin_amdgcn_readlane((int)dv, j);
            rank += jk < dk || (jk == dk && jv < dv);
        }
        if (lane < kk) {
            ov[rank] = (int32_t)dv;
            od[rank] = dist_unkey(dk);
        }
        return;
    }

    int P2 = 128;
    while (P2 < kk) P2 <<= 1;
    for (int size = 2; size <= P2; size <<= 1) {
        const int half = size >> 1;
        for (int s = half; s > 0; s >>= 1) {
            for (int i = lane; i < (P2 >> 1); i += 64) {
                int lo, hi;
                if (s == half) {    /* the stage's first step mirrors the upper half */
                    const int r = i & (half - 1);
                    lo = 2 * (i - r) + r;
                    hi = 2 * (i - r) + size - 1 - r;
                } else {
                    lo = 2 * i - (i & (s - 1));
                    hi = lo + s;
                }
                if (hi >= kk) continue;
                const uint32_t ak = row[lo], bk = row[hi], av = sv[lo], bv = sv[hi];
                if (bk < ak || (bk == ak && bv < av)) {
                    row[lo] = bk; row[hi] = ak;
                    sv[lo] = bv;  sv[hi] = av;
                }
            }
            srt_fence();
        }
    }
    for (int i = lane; i < kk; i += 64) {
        ov[i] = (int32_t)sv[i];
        od[i] = dist_unkey(row[i]);
    }
}

/* After the distance phase's last barrier: every wave selects its queries. */
DEV void srt_select_tile(unsigned char* lds, const SrtLds& S, int stride, const int32_t* qvid,
                         int nql, int count, int k, int32_t* out_v, float* out_d)
{
    const int wave = threadIdx.x >> 6;
    uint32_t* mat = (uint32_t*)(lds + S.mat);
    const int32_t* gids = (const int32_t*)(lds + S.gids);
    uint32_t* sv = (uint32_t*)(lds + S.scratch) + wave * stride;
    for (int ql = wave; ql < nql; ql += XWAVES) {
        uint32_t* row = mat + ql * stride;
        int32_t* ov = out_v + (size_t)qvid[ql] * k;
        float* od = out_d + (size_t)qvid[ql] * k;
        if (count <= 64) srt_select<1>(row, gids, sv, count, k, ov, od);
        else if (count <= 256) srt_select<4>(row, gids, sv, count, k, ov, od);
        else srt_select<GK_SORT_CAP / 64>(row, gids, sv, count, k, ov, od);
    }
}

/* sstride: the sorted selection's matrix stride (SORTED only) */
template <int DM, bool QRES, bool SORTED>
__global__ __launch_bounds__(XTHREADS, 2)
void group_f32_kernel(const float* __restrict__ vectors, int d,
                      const int32_t* __restrict__ members,
                      const GroupTile* __restrict__ tiles, int32_t k, int sstride,
                      int32_t* out_v, float* out_d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const F32Lds L = f32_lds(d);
    const GrpLds G = grp_lds(L.total, FRT);
    const SrtLds S = srt_lds(L.thr, FRT, sstride);
    float* qlds = (float*)(xlds + L.q);
    float* rlds = (float*)(xlds + L.rows);
    int32_t* qvid = (int32_t*)(xlds + (SORTED ? S.qvid : G.qvid));
    int32_t* mids = (int32_t*)(xlds + (SORTED ? S.mids : G.mids));     /* [2][FRT], by tile parity */
    const int tid = threadIdx.x;
    const int g = tid & 15, gq = (tid >> 4) & 3, gr = tid >> 6, lr = tid >> 4;
    const GroupTile T = tiles[blockIdx.x];
    const int32_t* mem = members + T.start;
    const int nql = group_queries(T, members, qvid);
    const XSel sel = {(float*)(xlds + L.thr), (int*)(xlds + L.cnt), (XCand*)(xlds + L.cand),
                      out_v, out_d, k, nql, qvid};
    const bool vec = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;
    const int qstride = QRES ? f32_qstride(d) : FQSS;

    /* this thread's slab columns of the vector `id` */
    auto cols = [&](int32_t id, int k0) {
        return f32_cols_load(id >= 0 ? vectors + (size_t)id * d : nullptr, d, k0, vec);
    };
    /* the member this thread loads for row tile t: row lr of it */
    auto row_id = [&](int t) {
        const int ri = t * FRT + lr;
        return ri < T.count ? mem[ri] : -1;
    };

    int32_t qid0 = -1, qid1 = -1;       /* streamed query rows lr and 16 + lr */
    if constexpr (QRES) {
        for (int i = tid; i < XQT * qstride; i += XTHREADS) {
            const int r = i / qstride, c = i - r * qstride;
            qlds[i] = (r < nql && c < d) ? vectors[(size_t)qvid[r] * d + c] : 0.0f;
        }
    } else {
        qid0 = qvid[lr];
        qid1 = qvid[16 + lr];
    }
    if constexpr (SORTED) {
        int32_t* gids = (int32_t*)(xlds + S.gids);
        for (int i = tid; i < T.count; i += XTHREADS) gids[i] = mem[i];
    } else {
        sel_init(sel);
    }

    const int nslab = (d + FKS - 1) / FKS;
    const int ntile = (T.count + FRT - 1) / FRT;
    const int nstep = ntile * nslab;            /* >= 1: a group is not empty */

    float acc[FMQ][FMR];
    int32_t idc = row_id(0), idn = row_id(1);   /* of the tile being loaded, and the next */
    float4 pr = cols(idc, 0), pq0 = pr, pq1 = pr;
    f32_slab_store(rlds, FKS, pr);
    if (g == 0) mids[lr] = idc;
    if constexpr (!QRES) {
        pq0 = cols(qid0, 0);
        pq1 = cols(qid1, 0);
        f32_slab_store(qlds, FQSS, pq0, 0);
        f32_slab_store(qlds, FQSS, pq1, 16);
    }
    __syncthreads();

    int tile = 0, slab = 0;
    for (int st = 0; st < nstep; st++) {
        int ntl = tile, nsl = slab + 1;
        if (nsl == nslab) { nsl = 0; ntl++; }
        const bool more = st + 1 < nstep;
        if (more) {     /* in flight while this slab computes */
            if (ntl != tile) {
                idc = idn;
                idn = row_id(ntl + 1);
            }
            pr = cols(idc, nsl * FKS);
            if constexpr (!QRES) {
                pq0 = cols(qid0, nsl * FKS);
                pq1 = cols(qid1, nsl * FKS);
            }
        }
        const float* rb = rlds + (st & 1) * (FRT * FKS) + (gr * FMR) * FKS;
        const float* qb = (QRES ? qlds + slab * FKS : qlds + (st & 1) * (XQT * FQSS)) +
                          gq * qstride;
        f32_slab_math<DM>(acc, qb, rb, qstride, slab, d, g);

        if (slab == nslab - 1) {
            float dist[FMQ];
            int ql[FMQ];
            int32_t vid[FMQ];
            uint32_t pend = 0;
            const int32_t myvid = mids[(tile & 1) * FRT + gr * FMR + (g & 3)];
            f32_fold<DM>(acc, qb, rb, qstride, slab, d, g, dist);
            if constexpr (SORTED) {
                uint32_t* col = (uint32_t*)(xlds + S.mat) + tile * FRT + gr * FMR + (g & 3);
#pragma unroll
                for (int i = 0; i < FMQ; i++) {
                    const int q = gq + 4 * i;
                    if (g < FMR && myvid >= 0 && q < nql)
                        col[q * sstride] = srt_bits(dist[i], myvid != qvid[q]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < FMQ; i++) {
                    ql[i] = gq + 4 * i;
                    vid[i] = myvid;
                    if (g < FMR && myvid >= 0 && ql[i] < nql && myvid != qvid[ql[i]] &&
                        dist[i] <= sel.thr[ql[i]])
                        pend |= 1u << i;
                }
                sel_append(sel, pend, dist, ql, vid);
            }
        }

        if (more) {
            f32_slab_store(rlds + ((st + 1) & 1) * (FRT * FKS), FKS, pr);
            if (g == 0) mids[(ntl & 1) * FRT + lr] = idc;   /* read at ntl's last slab */
            if constexpr (!QRES) {
                f32_slab_store(qlds + ((st + 1) & 1) * (XQT * FQSS), FQSS, pq0, 0);
                f32_slab_store(qlds + ((st + 1) & 1) * (XQT * FQSS), FQSS, pq1, 16);
            }
        }
        __syncthreads();
        tile = ntl;
        slab = nsl;
    }
    if constexpr (SORTED)
        srt_select_tile(xlds, S, sstride, qvid, nql, T.count, k, out_v, out_d);
    else
        flush_cands(sel, 1);
}

enum { GI_CPR_MAX = (I_MAX_W + 3) / 4,      /* 16-byte chunks of a row at the dim guard */
       GI_NCH = (IRT * GI_CPR_MAX + XTHREADS - 1) / XTHREADS };  /* chunks per thread */

template <int DM, bool SORTED>
__global__ __launch_bounds__(XTHREADS, 2)
void group_i8_kernel(const int8_t* __restrict__ vectors, int d,
                     const int32_t* __restrict__ members,
                     const GroupTile* __restrict__ tiles, int32_t k, int sstride,
                     int32_t* out_v, float* out_d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const I8Lds L = i8_lds(d);
    const GrpLds G = grp_lds(L.total, IRT);
    const SrtLds S = srt_lds(L.thr, IRT, sstride);
    uint32_t* qlds = (uint32_t*)(xlds + L.q);
    uint32_t* rlds = (uint32_t*)(xlds + L.rows);
    int* aa = (int*)(xlds + L.aa);
    int32_t* qvid = (int32_t*)(xlds + (SORTED ? S.qvid : G.qvid));
    int32_t* mids = (int32_t*)(xlds + (SORTED ? S.mids : G.mids));     /* [2][IRT], by tile parity */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GroupTile T = tiles[blockIdx.x];
    const int32_t* mem = members + T.start;
    const int nql = group_queries(T, members, qvid);
    const XSel sel = {(float*)(xlds + L.thr), (int*)(xlds + L.cnt), (XCand*)(xlds + L.cand),
                      out_v, out_d, k, nql, qvid};
    const int W = (d + 3) >> 2, WL = W | 1, CPR = (W + 3) >> 2;
    /* how a row may be read: 2 = 16 bytes, 1 = dwords, 0 = bytes */
    const int wide = ((d & 15) == 0 && ((uintptr_t)vectors & 15) == 0) ? 2
                   : ((d & 3) == 0 && ((uintptr_t)vectors & 3) == 0) ? 1 : 0;

    for (int i = tid; i < XQT * W; i += XTHREADS) {
        const int r = i / W, w = i - r * W;
        uint32_t v = 0;
        if (r < nql)
            v = wide ? *(const uint32_t*)(vectors + (size_t)qvid[r] * d + 4 * w)
                     : i8_pack_dword(vectors, qvid[r], w, d);
        qlds[r * WL + w] = v;
    }
    /* the member of row tid of row tile t, -1 past the group's end */
    auto tile_id = [&](int t) {
        const int ri = t * IRT + tid;
        return (tid < IRT && ri < T.count) ? mem[ri] : -1;
    };
    if (tid < IRT) {
        mids[tid] = tile_id(0);
        mids[IRT + tid] = tile_id(1);
    }
    int32_t idn = tile_id(2);           /* ids are read two tiles ahead of their use */
    if constexpr (SORTED) {
        int32_t* gids = (int32_t*)(xlds + S.gids);
        for (int i = tid; i < T.count; i += XTHREADS) gids[i] = mem[i];
        __syncthreads();
    } else {
        sel_init(sel);
    }
    if (tid < XQT) {        /* query self-dots, for L2 */
        int s = 0;
        for (int w = 0; w < W; w++) {
            const int v = (int)qlds[tid * WL + w];
            s = __builtin_amdgcn_sdot4(v, v, s, false);
        }
        aa[tid] = s;
    }

    /* chunk c of this thread is 16-byte chunk j of row r of the tile, with
     * r * CPR + j = tid + c * XTHREADS; (r0, j0) is the first */
    const int cr0 = tid / CPR, cj0 = tid - cr0 * CPR;
    const int cdr = XTHREADS / CPR, cdj = XTHREADS - cdr * CPR;
    uint4 pre[GI_NCH];
    auto stage_load = [&](int t) {
        if (!wide) return;
        const int32_t* ids = mids + (t & 1) * IRT;
        int r = cr0, j = cj0;
#pragma unroll
        for (int c = 0; c < GI_NCH; c++) {
            uint4 v = make_uint4(0, 0, 0, 0);
            const int32_t id = r < IRT ? ids[r] : -1;
            if (id >= 0) {
                const unsigned char* p = (const unsigned char*)vectors + (size_t)id * d + 16 * j;
                if (wide == 2) {
                    v = *(const uint4*)p;
                } else {
                    v.x = *(const uint32_t*)p;
                    if (4 * j + 1 < W) v.y = *(const uint32_t*)(p + 4);
                    if (4 * j + 2 < W) v.z = *(const uint32_t*)(p + 8);
                    if (4 * j + 3 < W) v.w = *(const uint32_t*)(p + 12);
                }
            }
            pre[c] = v;
            r += cdr;
            j += cdj;
            if (j >= CPR) { j -= CPR; r++; }
        }
    };
    auto stage_store = [&](int t) {
        if (!wide) {
            const int32_t* ids = mids + (t & 1) * IRT;
            for (int i = tid; i < IRT * W; i += XTHREADS) {
                const int r = i / W, w = i - r * W;
                rlds[r * WL + w] = ids[r] >= 0 ? i8_pack_dword(vectors, ids[r], w, d) : 0u;
            }
            return;
        }
        int r = cr0, j = cj0;
#pragma unroll
        for (int c = 0; c < GI_NCH; c++) {
            const uint32_t v[4] = {pre[c].x, pre[c].y, pre[c].z, pre[c].w};
            if (r < IRT) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (4 * j + e < W) rlds[r * WL + 4 * j + e] = v[e];
            }
            r += cdr;
            j += cdj;
            if (j >= CPR) { j -= CPR; r++; }
        }
    };

    const int ntile = (T.count + IRT - 1) / IRT;    /* >= 1 */
    stage_load(0);          /* the barrier above is behind the ids of tiles 0 and 1 */
    stage_store(0);
    __syncthreads();

    const int h = lane >> 5, col = lane & 31;
    const uint32_t* arow = qlds + col * WL;
    const uint32_t* brow = rlds + (wave * 32 + col) * WL;
    for (int t = 0; t < ntile; t++) {
        if (t + 1 < ntile) stage_load(t + 1);   /* in flight while this tile computes */

        v16i acc;
        int bb;
        i8_tile_dots<DM>(arow, brow, W, h, acc, bb);

        uint32_t pend = 0;
        float dist[16];
        int ql[16];
        int32_t vid[16];
        const int32_t myvid = mids[(t & 1) * IRT + wave * 32 + col];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            ql[r] = 8 * (r >> 2) + 4 * h + (r & 3);
            vid[r] = myvid;
            dist[r] = (DM == DM_L2) ? (float)(aa[ql[r]] - 2 * acc[r] + bb)
                                    : (float)(16129 - acc[r]);
            if constexpr (SORTED) {
                if (myvid >= 0 && ql[r] < nql)
                    ((uint32_t*)(xlds + S.mat))[ql[r] * sstride + t * IRT + wave * 32 + col] =
                        srt_bits(dist[r], myvid != qvid[ql[r]]);
            } else if (myvid >= 0 && ql[r] < nql && myvid != qvid[ql[r]] &&
                       dist[r] <= sel.thr[ql[r]]) {
                pend |= 1u << r;
            }
        }
        /* ends with a barrier: the tile is free */
        if constexpr (SORTED) __syncthreads();
        else sel_append(sel, pend, dist, ql, vid);

        if (t + 1 < ntile) stage_store(t + 1);
        /* tile t's ids are done with: tile t + 2's take their place */
        if (tid < IRT) mids[(t & 1) * IRT + tid] = idn;
        idn = tile_id(t + 3);
        __syncthreads();
    }
    if constexpr (SORTED)
        srt_select_tile(xlds, S, sstride, qvid, nql, T.count, k, out_v, out_d);
    else
        flush_cands(sel, 1);
}

/* ------------------------------------------------------------------ *
 * RNG prune: RebuildNeighbors over candidate lists
 * ------------------------------------------------------------------ *
 * Row r has a node id and a list of C candidates in ascending distance. The
 * list is walked in order while fewer than `degree` are accepted; a valid
 * candidate c (id >= 0, not the node, finite distance) is rejected when some
 * accepted a has factor * dist(a, c) < cand_dists[c], and accepted otherwise.
 * The rule needs dist(accepted, candidate) only, so nothing like the C x C
 * matrix is formed: a workgroup owns one row, keeps the accepted vectors in
 * LDS as the "query tile" of the kernels above (32 slots, or 64 for
 * degree > 32) and streams the list as row tiles, each candidate vector
 * gathered from global memory once.
 *
 *   tile    A tile is speculative: which of its candidates are accepted is
 *           not known when its distances are computed. So a tile computes
 *           dist(accepted before the tile, tile) and dist(tile, tile), as
 *           bits: rej[c] (some earlier accepted vector rejects c) and
 *           viol[c] (bit q: candidate q of the tile would reject c). One wave
 *           then walks the tile in list order: c is accepted iff it is valid,
 *           rej[c] is clear and viol[c] has no bit of a candidate accepted
 *           earlier in this walk. That is the serial rule exactly: every
 *           pair the rule would look at has been compared with the same
 *           operands, and pairs it would not look at are masked out.
 *   append  The vectors of the newly accepted candidates are copied to their
 *           slots of the query tile from the tile's copy in LDS.
 *   stop    A row ends at `degree` accepted; later tiles are never loaded.
 *   lists   The ids and distances of the whole list (C <= 1024) are read
 *           into LDS first, so no vector load ever waits for its id.
 *   fill    With fill_pruned, a row that ends short keeps its first
 *           degree - count valid rejected candidates too; the kept ids go
 *           out in list order (a status byte per candidate, ballots).
 *
 * f32: 256 threads, tiles of 16 candidates, the micro-tiles and the
 *   reference-order fold of the kernels above. RES: vectors whole in LDS, the next
 *   tile's loads in flight in registers during the math. Otherwise (large
 *   dims) the accepted vectors and the tile stream through LDS in slabs of
 *   FKS columns with the accumulators kept; the accepted vectors are then
 *   read again (by id) for every tile, the candidates still once.
 * int8: one wave, tiles of 32 candidates, three 32x32 MFMA blocks a tile
 *   (accepted 0..31, accepted 32..63, tile x tile), everything resident. */

enum { RP_INVALID = 0, RP_VALID = 1, RP_ACC = 2, RP_REJ = 3 };
enum { RP_MAX_C = 1024, RP_LDS_MAX = 65536, RI_T = 32, RI_NP = (I_MAX_W + 1) / 2 };

struct RpCtl {
    int count;              /* accepted so far */
    uint32_t newmask;       /* accepted candidates of the last tile */
    uint32_t rej;           /* f32: bit c, an earlier accepted vector rejects c */
    uint32_t viol[32];      /* f32: bit q of [c], tile candidate q rejects c */
    int32_t accid[MAX_DEG]; /* accepted ids, in list order */
    int asd[MAX_DEG];       /* int8: self-dots of the accepted vectors */
    int tsd[RI_T];          /* int8: and of the tile's */
};

struct RpLds { uint32_t ctl, acc, tile, cids, cdd, status, total; };

/* acc_words / tile_words: dwords of the accepted vectors and of a tile */
static inline __host__ __device__ RpLds rp_lds(uint32_t acc_words, uint32_t tile_words, int C)
{
    RpLds l;
    uint32_t b = 0;
    l.ctl = b;    b += (uint32_t)(sizeof(RpCtl) + 15) & ~15u;
    l.acc = b;    b += acc_words * 4;
    l.tile = b;   b += tile_words * 4;
    l.cids = b;   b += (uint32_t)C * 4;
    l.cdd = b;    b += (uint32_t)C * 4;
    l.status = b; b += ((uint32_t)C + 3) & ~3u;
    l.total = b;
    return l;
}

/* whether the f32 kernel keeps nqt * 32 accepted vectors and a tile whole */
static inline __host__ __device__ bool rp_f32_resident(int d, int nqt, int C)
{
    const int qs = f32_qstride(d);
    return qs <= FQRES_MAX &&
           rp_lds((uint32_t)(nqt * XQT * qs), (uint32_t)(FRT * qs), C).total <= RP_LDS_MAX;
}

/* the row's list into LDS, every candidate's status, an empty accepted set.
 * Ends with a barrier. */
DEV void rp_lists(RpCtl* ctl, int32_t* cids, float* cdd, uint8_t* status,
                  const int32_t* __restrict__ gi, const float* __restrict__ gd, int C,
                  int32_t node)
{
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const int32_t id = gi[c];
        const float dd = gd[c];
        cids[c] = id;
        cdd[c] = dd;
        status[c] = (id >= 0 && id != node && __builtin_isfinite(dd)) ? RP_VALID : RP_INVALID;
    }
    if (threadIdx.x == 0) { ctl->count = 0; ctl->newmask = 0; ctl->rej = 0; }
    if (threadIdx.x < 32) ctl->viol[threadIdx.x] = 0;
    __syncthreads();
}

/* One wave walks a tile of nt candidates in list order. Lane c holds viol[c];
 * bit c of okmask: c is valid and no earlier accepted vector rejects it. cnt
 * (wave-uniform) goes from the accepted count before the tile to the one
 * after it; returns the accepted candidates. */
DEV uint32_t rp_resolve(uint32_t viol, uint32_t okmask, int nt, int& cnt, int degree)
{
    uint32_t accm = 0;
    for (int c = 0; c < nt && cnt < degree; c++) {
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)viol, c);
        if (((okmask >> c) & 1) && !(v & accm)) {
            accm |= 1u << c;
            cnt++;
        }
    }
    return accm;
}

/* the walk's outcome into LDS: lane < nt is candidate c of the list */
DEV void rp_commit(RpCtl* ctl, uint8_t* status, const int32_t* cids, int c, bool valid,
                   int lane, uint32_t accm, int count0, int cnt)
{
    if (valid) {
        const bool a = (accm >> lane) & 1;
        status[c] = a ? RP_ACC : RP_REJ;
        if (a) ctl->accid[count0 + __popc(accm & ((1u << lane) - 1))] = cids[c];
    }
    if (lane == 0) { ctl->count = cnt; ctl->newmask = accm; }
}

/* One wave writes the row: the accepted ids, with `fill` and a short row the
 * first degree - count rejected ones among them, in list order; then -1. */
DEV void rp_write_out(const RpCtl* ctl, const uint8_t* status, const int32_t* cids, int C,
                      int degree, int fill, int32_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int cnt = ctl->count;
    if (!fill || cnt >= degree) {
        for (int i = lane; i < degree; i += 64) out[i] = i < cnt ? ctl->accid[i] : -1;
        return;
    }
    const uint64_t below = (1ull << lane) - 1;
    const int spare = degree - cnt;
    int pos = 0, rejseen = 0;
    for (int base = 0; base < C; base += 64) {
        const int c = base + lane;
        const int st = c < C ? status[c] : RP_INVALID;
        const bool isrej = st == RP_REJ || st == RP_VALID;
        const uint64_t rb = __ballot(isrej);
        const bool keep = st == RP_ACC || (isrej && rejseen + __popcll(rb & below) < spare);
        const uint64_t kb = __ballot(keep);
        if (keep) out[pos + __popcll(kb & below)] = cids[c];
        pos += __popcll(kb);
        rejseen += __popcll(rb);
    }
    for (int i = pos + lane; i < degree; i += 64) out[i] = -1;
}

/* columns c .. c+3 of the row of d floats at `row`, zero past d and for a
 * null row (f32_cols_load with the column given) */
DEV float4 rp_cols4(const float* __restrict__ row, int d, int c, bool vec)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row && c < d) {
        const float* p = row + c;
        if (vec) {
            v = *(const float4*)p;
        } else {
            v.x = p[0];
            if (c + 1 < d) v.y = p[1];
            if (c + 2 < d) v.z = p[2];
            if (c + 3 < d) v.w = p[3];
        }
    }
    return v;
}

/* f32_slab_math / f32_fold over the first NI query rows of the micro-tile
 * (queries gq + 4*i, i < NI), with a row stride of its own for the rows */
template <int DM, int NI>
DEV void rp_math(float (&acc)[FMQ][FMR], const float* qb, const float* rb, int qstride,
                 int rstride, int slab, int d, int g)
{
    if (slab == 0) {
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int j = 0; j < FMR; j++) acc[i][j] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < FKS / 16; c++) {
        if (slab * FKS + c * 16 + 16 > d) break;
        float x[NI], y[FMR];
#pragma unroll
        for (int i = 0; i < NI; i++) x[i] = qb[4 * i * qstride + c * 16 + g];
#pragma unroll
        for (int j = 0; j < FMR; j++) y[j] = rb[j * rstride + c * 16 + g];
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int j = 0; j < FMR; j++) acc[i][j] = xstep<DM>(x[i], y[j], acc[i][j]);
    }
}

template <int DM, int NI>
DEV void rp_fold(const float (&acc)[FMQ][FMR], const float* qb, const float* rb, int qstride,
                 int rstride, int slab, int d, int g, float (&dist)[FMQ])
{
    const int nd16 = d & ~15, nd8 = d & ~7, nd4 = d & ~3;
    const int tc = nd16 - slab * FKS;
    float x8[NI], x4[NI], y8[FMR], y4[FMR];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        x8[i] = (nd8 > nd16 && g < 8) ? qb[4 * i * qstride + tc + g] : 0.0f;
        x4[i] = (nd4 > nd8 && g < 4) ? qb[4 * i * qstride + tc + (nd8 - nd16) + g] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < FMR; j++) {
        y8[j] = (nd8 > nd16 && g < 8) ? rb[j * rstride + tc + g] : 0.0f;
        y4[j] = (nd4 > nd8 && g < 4) ? rb[j * rstride + tc + (nd8 - nd16) + g] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < NI; i++) {
        float mine = 0.0f;
#pragma unroll
        for (int j = 0; j < FMR; j++) {
            float a = acc[i][j];
            a = a + dpp<DPP_ROW_SHL8>(a);
            if (nd8 > nd16) a = xstep<DM>(x8[i], y8[j], a);
            a = a + dpp<DPP_ROW_SHL4>(a);
            if (nd4 > nd8) a = xstep<DM>(x4[i], y4[j], a);
            const float s = ((dpp<DPP_QUAD0>(a) + dpp<DPP_QUAD1>(a)) +
                             dpp<DPP_QUAD2>(a)) + dpp<DPP_QUAD3>(a);
            mine = (j == 0 || g == j) ? s : mine;
        }
        for (int c = nd4; c < d; c++)
            mine = xstep<DM>(qb[4 * i * qstride + (c - slab * FKS)],
                             rb[(g & 3) * rstride + (c - slab * FKS)], mine);
        dist[i] = (DM == DM_L2) ? mine : 1.0f - mine;
    }
}

/* NQT: query tiles of 32 accepted slots (2 for degree > 32) */
template <int DM, bool RES, int NQT>
__global__ __launch_bounds__(XTHREADS, NQT == 1 ? 2 : 1)
void rng_prune_f32_kernel(const float* __restrict__ vectors, int d,
                          const int32_t* __restrict__ nodes,
                          const int32_t* __restrict__ cand_ids,
                          const float* __restrict__ cand_dists, int C, int degree,
                          float factor, int fill, int32_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int qs = RES ? f32_qstride(d) : FQSS;    /* row stride of both buffers */
    const RpLds L = rp_lds((uint32_t)(NQT * XQT * qs), (uint32_t)(FRT * qs), C);
    RpCtl* ctl = (RpCtl*)(xlds + L.ctl);
    float* abuf = (float*)(xlds + L.acc);       /* accepted vectors (or their slab) */
    float* tbuf = (float*)(xlds + L.tile);      /* the tile's (or their slab) */
    int32_t* cids = (int32_t*)(xlds + L.cids);
    float* cdd = (float*)(xlds + L.cdd);
    uint8_t* status = xlds + L.status;
    const int tid = threadIdx.x;
    const int g = tid & 15, gq = (tid >> 4) & 3, gr = tid >> 6, lr = tid >> 4;
    const size_t row = blockIdx.x;
    rp_lists(ctl, cids, cdd, status, cand_ids + row * C, cand_dists + row * C, C, nodes[row]);

    const bool vec = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;
    const int nslab = (d + FKS - 1) / FKS;
    const int ntile = (C + FRT - 1) / FRT;
    /* the vector of candidate lr of tile t, null for a hole or past the list */
    auto cand_row = [&](int t) -> const float* {
        const int c = t * FRT + lr;
        const int32_t id = c < C ? cids[c] : -1;
        return id >= 0 ? vectors + (size_t)id * d : nullptr;
    };
    /* RES: this thread's columns 4*(g + 16*k) of row lr of a tile */
    float4 pre[FQRES_MAX / 64];
    auto tile_load = [&](int t) {
        const float* p = cand_row(t);
#pragma unroll
        for (int k = 0; k < FQRES_MAX / 64; k++) {
            const int col = 4 * (g + 16 * k);
            if (col < qs) pre[k] = rp_cols4(p, d, col, vec);
        }
    };
    auto tile_store = [&]() {
#pragma unroll
        for (int k = 0; k < FQRES_MAX / 64; k++) {
            const int col = 4 * (g + 16 * k);
            if (col < qs) *(float4*)(tbuf + lr * qs + col) = pre[k];
        }
    };
    if constexpr (RES) {
        tile_load(0);
        tile_store();
        __syncthreads();
    }

    float a0[FMQ][FMR], a1[FMQ][FMR], aT[FMQ][FMR];
    for (int t = 0;; t++) {
        const int count0 = __builtin_amdgcn_readfirstlane(ctl->count);
        const bool use0 = count0 > 0, use1 = NQT == 2 && count0 > XQT;   /* tiles in use */
        if constexpr (RES) {
            if (t + 1 < ntile) tile_load(t + 1);    /* in flight while this tile computes */
        }
        for (int slab = 0; slab < nslab; slab++) {
            const int off = RES ? slab * FKS : 0;
            if constexpr (!RES) {
                for (int r16 = 0; r16 < NQT * XQT && r16 < count0; r16 += 16) {
                    const int slot = r16 + lr;
                    const int32_t id = slot < count0 ? ctl->accid[slot] : -1;
                    f32_slab_store(abuf, FQSS,
                                   f32_cols_load(id >= 0 ? vectors + (size_t)id * d : nullptr,
                                                 d, slab * FKS, vec), r16);
                }
                f32_slab_store(tbuf, FQSS, f32_cols_load(cand_row(t), d, slab * FKS, vec));
                __syncthreads();
            }
            const float* qa = abuf + gq * qs + off;         /* accepted gq + 4*i */
            const float* qt = tbuf + gq * qs + off;         /* tile candidate gq + 4*i */
            const float* rb = tbuf + gr * FMR * qs + off;   /* this wave's four candidates */
            if (use0) rp_math<DM, FMQ>(a0, qa, rb, qs, qs, slab, d, g);
            if (use1) rp_math<DM, FMQ>(a1, qa + XQT * qs, rb, qs, qs, slab, d, g);
            rp_math<DM, 4>(aT, qt, rb, qs, qs, slab, d, g);

            if (slab == nslab - 1) {
                float d0[FMQ] = {}, d1[FMQ] = {}, dT[FMQ] = {};
                if (use0) rp_fold<DM, FMQ>(a0, qa, rb, qs, qs, slab, d, g, d0);
                if (use1) rp_fold<DM, FMQ>(a1, qa + XQT * qs, rb, qs, qs, slab, d, g, d1);
                rp_fold<DM, 4>(aT, qt, rb, qs, qs, slab, d, g, dT);
                /* lane g < FMR of a group: candidate r of the tile against
                 * accepted gq + 4*i (+ 32) and tile candidates gq + 4*i */
                const int r = gr * FMR + (g & 3), c = t * FRT + r;
                if (g < FMR && c < C) {
                    const float cdr = cdd[c];
                    bool rej = false;
                    uint32_t m = 0;
#pragma unroll
                    for (int i = 0; i < FMQ; i++) {
                        if (gq + 4 * i < count0 && factor * d0[i] < cdr) rej = true;
                        if (NQT == 2 && XQT + gq + 4 * i < count0 && factor * d1[i] < cdr)
                            rej = true;
                        if (i < 4 && factor * dT[i] < cdr) m |= 1u << (gq + 4 * i);
                    }
                    if (rej) atomicOr(&ctl->rej, 1u << r);
                    if (m) atomicOr(&ctl->viol[r], m);
                }
            }
            if constexpr (!RES) __syncthreads();    /* the slab is free */
        }
        __syncthreads();
        if (gr == 0) {
            const int c = t * FRT + tid;
            const bool valid = tid < FRT && c < C && status[c] == RP_VALID;
            const uint32_t viol = tid < FRT ? ctl->viol[tid] : 0u;
            const uint32_t ok = (uint32_t)__ballot(valid) &
                                ~(uint32_t)__builtin_amdgcn_readfirstlane((int)ctl->rej);
            int cnt = count0;
            const uint32_t accm = rp_resolve(viol, ok, FRT, cnt, degree);
            rp_commit(ctl, status, cids, c, valid, tid, accm, count0, cnt);
            if (tid == 0) ctl->rej = 0;
            if (tid < FRT) ctl->viol[tid] = 0;
        }
        __syncthreads();
        const uint32_t newmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctl->newmask);
        if constexpr (RES) {        /* the accepted vectors to their slots */
            if ((newmask >> lr) & 1) {
                const int slot = count0 + __popc(newmask & ((1u << lr) - 1));
#pragma unroll
                for (int k = 0; k < FQRES_MAX / 64; k++) {
                    const int col = 4 * (g + 16 * k);
                    if (col < qs)
                        *(float4*)(abuf + slot * qs + col) = *(const float4*)(tbuf + lr * qs + col);
                }
            }
        }
        if (__builtin_amdgcn_readfirstlane(ctl->count) >= degree || t + 1 == ntile) break;
        __syncthreads();
        if constexpr (RES) {
            tile_store();
            __syncthreads();
        }
    }
    __syncthreads();
    if (gr == 0) rp_write_out(ctl, status, cids, C, degree, fill, out + row * degree);
}

template <int DM>
__global__ __launch_bounds__(64)
void rng_prune_i8_kernel(const int8_t* __restrict__ vectors, int d,
                         const int32_t* __restrict__ nodes,
                         const int32_t* __restrict__ cand_ids,
                         const float* __restrict__ cand_dists, int C, int degree,
                         float factor, int fill, int32_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int W = (d + 3) >> 2, WL = W | 1;
    const RpLds L = rp_lds((uint32_t)(MAX_DEG * WL), (uint32_t)(RI_T * WL), C);
    RpCtl* ctl = (RpCtl*)(xlds + L.ctl);
    uint32_t* abuf = (uint32_t*)(xlds + L.acc);     /* [MAX_DEG][WL] accepted vectors */
    uint32_t* tbuf = (uint32_t*)(xlds + L.tile);    /* [RI_T][WL] the tile's */
    int32_t* cids = (int32_t*)(xlds + L.cids);
    float* cdd = (float*)(xlds + L.cdd);
    uint8_t* status = xlds + L.status;
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const size_t row = blockIdx.x;
    rp_lists(ctl, cids, cdd, status, cand_ids + row * C, cand_dists + row * C, C, nodes[row]);

    /* whole dwords to a row, dword aligned: lanes 2r and 2r + 1 load the even
     * and the odd dwords of candidate r into registers a tile ahead; other
     * pitches are packed from bytes at the store */
    const bool wide = (d & 3) == 0 && ((uintptr_t)vectors & 3) == 0;
    const int ntile = (C + RI_T - 1) / RI_T;
    uint32_t pre[RI_NP];
    auto tile_load = [&](int t) {
        if (!wide) return;
        const int c = t * RI_T + (lane >> 1);
        const int32_t id = c < C ? cids[c] : -1;
        const uint32_t* p = (const uint32_t*)(vectors + (size_t)(id >= 0 ? id : 0) * d);
#pragma unroll
        for (int j = 0; j < RI_NP; j++) {
            const int w = (lane & 1) + 2 * j;
            pre[j] = (id >= 0 && w < W) ? p[w] : 0u;
        }
    };
    /* ends with a barrier behind the tile and its self-dots */
    auto tile_store = [&](int t) {
        if (wide) {
#pragma unroll
            for (int j = 0; j < RI_NP; j++) {
                const int w = (lane & 1) + 2 * j;
                if (w < W) tbuf[(lane >> 1) * WL + w] = pre[j];
            }
        } else {
            for (int i = lane; i < RI_T * W; i += 64) {
                const int r = i / W, w = i - r * W, c = t * RI_T + r;
                const int32_t id = c < C ? cids[c] : -1;
                tbuf[r * WL + w] = id >= 0 ? i8_pack_dword(vectors, id, w, d) : 0u;
            }
        }
        __syncthreads();
        if (lane < RI_T) {
            int s = 0;
            for (int w = 0; w < W; w++) {
                const int v = (int)tbuf[lane * WL + w];
                s = __builtin_amdgcn_sdot4(v, v, s, false);
            }
            ctl->tsd[lane] = s;
        }
        __syncthreads();
    };
    tile_load(0);
    tile_store(0);

    const uint32_t* trow = tbuf + col * WL;
    for (int t = 0;; t++) {
        const int count0 = __builtin_amdgcn_readfirstlane(ctl->count);
        if (t + 1 < ntile) tile_load(t + 1);    /* in flight while this tile computes */

        /* acc[r] is query 8*(r/4) + 4*h + r%4 against candidate `col` */
        v16i vT, v0 = {}, v1 = {};
        int bb, bbx;
        i8_tile_dots<DM>(trow, trow, W, h, vT, bb);
        if (count0 > 0) i8_tile_dots<DM>(abuf + col * WL, trow, W, h, v0, bbx);
        if (count0 > 32) i8_tile_dots<DM>(abuf + (32 + col) * WL, trow, W, h, v1, bbx);

        const int c = t * RI_T + col;
        const float cdc = c < C ? cdd[c] : 0.0f;
        uint32_t viol = 0;
        int rej = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int q = 8 * (r >> 2) + 4 * h + (r & 3);
            const float dT = (DM == DM_L2) ? (float)(ctl->tsd[q] - 2 * vT[r] + bb)
                                           : (float)(16129 - vT[r]);
            if (factor * dT < cdc) viol |= 1u << q;
            if (q < count0) {
                const float d0 = (DM == DM_L2) ? (float)(ctl->asd[q] - 2 * v0[r] + bb)
                                               : (float)(16129 - v0[r]);
                if (factor * d0 < cdc) rej = 1;
            }
            if (32 + q < count0) {
                const float d1 = (DM == DM_L2) ? (float)(ctl->asd[32 + q] - 2 * v1[r] + bb)
                                               : (float)(16129 - v1[r]);
                if (factor * d1 < cdc) rej = 1;
            }
        }
        viol |= (uint32_t)__shfl_xor((int)viol, 32);    /* both halves of the queries */
        rej |= __shfl_xor(rej, 32);
        const bool valid = lane < RI_T && c < C && status[c] == RP_VALID;
        const uint32_t ok = (uint32_t)__ballot(valid && !rej);
        int cnt = count0;
        const uint32_t accm = rp_resolve(viol, ok, RI_T, cnt, degree);
        rp_commit(ctl, status, cids, c, valid, lane, accm, count0, cnt);
        __syncthreads();
        int slot = count0;          /* the accepted vectors to their slots */
        for (uint32_t m = accm; m; m &= m - 1, slot++) {
            const int b = __builtin_ctz(m);
            for (int w = lane; w < W; w += 64) abuf[slot * WL + w] = tbuf[b * WL + w];
            if (lane == 0) ctl->asd[slot] = ctl->tsd[b];
        }
        if (cnt >= degree || t + 1 == ntile) break;
        __syncthreads();
        tile_store(t + 1);
    }
    __syncthreads();
    rp_write_out(ctl, status, cids, C, degree, fill, out + row * degree);
}

/* ------------------------------------------------------------------ *
 * Pool join: merge candidate lists into sorted pools
 * ------------------------------------------------------------------ *
 * Row r has a node id, an old pool (ids with distances that stand as given)
 * and a list of new candidates whose distances are given too or are computed
 * here, against the node's vector, in the search paths' arithmetic. The row's
 * output is the kout smallest distinct valid ids in ascending (dist, id),
 * then id -1 at +inf. A workgroup owns one row.
 *
 *   lists    Both id lists become 64-bit keys (id << 32 | entry) in LDS, the
 *            pool's entries before the new ones, an invalid entry (id < 0,
 *            the node itself, a non-finite given distance) all ones; the
 *            given distances go to LDS beside them. Nothing of the row is
 *            read from global memory after this step but vectors, so the
 *            output may be the pool's own buffers.
 *   dedupe   A bitonic sort of the keys puts the entries of one id next to
 *            each other, the pool's first, in list order. The thread that
 *            holds the first entry of a run walks it: a run that starts in
 *            the pool keeps the pool's smallest (dist, position) and drops
 *            every new entry of that id; a run of new entries keeps its
 *            smallest given (dist, position), or its first entry when the
 *            distance is still to be computed. Survivors are appended to the
 *            final keys: the pool's from slot 0, the new ones from slot
 *            npool, so the new ones are a dense work list. All of this is
 *            decided before any vector is touched.
 *   compute  Tiles of 16 surviving new candidates, one per 16-lane group.
 *            f32: the tile passes through LDS in slabs of PJ_KS columns
 *            (float4 loads, the next slab's in flight in registers during
 *            the math); lane g owns accumulator g of the reference's 16, the
 *            slabs keep it, and pj_fold_f32 is f32_fold for one pair. The
 *            node's vector sits in LDS; with a single slab (d <= PJ_KS)
 *            lane g keeps its columns in registers for the whole row.
 *            int8: no LDS at all; a lane holds up to five dwords of its
 *            candidate and of the node's vector (16-byte loads when rows
 *            are 16-byte multiples), the next tile's in flight, v_dot4c for
 *            ab and bb in one pass, a DPP fold over the group.
 *   select   A final key is (order-preserving f32 bits << 32 | id), -0
 *            folded to +0. A second bitonic sort, over the slots in use
 *            only, and the first kout keys are the answer.
 *
 * Given distances need no compute step: pool_join_given_kernel is lists,
 * dedupe and select alone, launched with one wave for short lists. */

enum { PJ_MAX_L = POOL_JOIN_MAX_LIST, PJ_T = 16, PJ_KS = 128, PJ_QS = PJ_KS + 16, PJ_I8_NW = 5,
       PJ_ONE_WAVE_MAX = 512 };
static_assert((PJ_QS / 16) % 2 == 1, "groups one row apart sit 16 banks apart");
static_assert(PJ_I8_NW * 16 >= I_MAX_W, "a group's lanes hold a whole int8 row");

static constexpr uint64_t PJ_NONE = ~0ull;

struct PjCtl { int npool; int nnew; };   /* survivors of each list */

struct PjLds { uint32_t ctl, a, b, dd, q, tile, total; };

static constexpr __host__ __device__ int pj_pow2(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

/* given: the new list brings its distances; qwords / twords: dwords of the
 * node's vector and of a tile slab */
static constexpr __host__ __device__ PjLds pj_lds(int npool, int nnew, bool given,
                                                  uint32_t qwords, uint32_t twords)
{
    PjLds l = {};
    const uint32_t P = (uint32_t)pj_pow2(npool + nnew);
    uint32_t b = 0;
    l.ctl = b;  b += 16;
    l.a = b;    b += P * 8;
    l.b = b;    b += P * 8;
    l.dd = b;   b += (((uint32_t)npool + (given ? (uint32_t)nnew : 0u)) * 4 + 15) & ~15u;
    l.q = b;    b += (qwords * 4 + 15) & ~15u;
    l.tile = b; b += twords * 4;
    l.total = b;
    return l;
}
static_assert(pj_lds(PJ_MAX_L, PJ_MAX_L, false, MAX_DIM, PJ_T * PJ_QS).total <= RP_LDS_MAX &&
              pj_lds(PJ_MAX_L, PJ_MAX_L, true, 0, 0).total <= RP_LDS_MAX,
              "the largest lists at the largest dim fit the prune's LDS budget");

DEV uint64_t pj_pack(float dist, int32_t id)
{
    return ((uint64_t)dist_key(dist) << 32) | (uint32_t)id;
}

DEV float pj_unpack_dist(uint64_t key)
{
    return dist_unkey((uint32_t)(key >> 32));
}

/* ascending bitonic sort of P (a power of two) keys in LDS by the whole
 * block; starts and ends with a barrier */
DEV void pj_sort(uint64_t* keys, int P)
{
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (P >> 1); i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const uint64_t x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & size) == 0)) { keys[lo] = y; keys[hi] = x; }
            }
            __syncthreads();
        }
    }
}

/* lists and dedupe. Leaves the final keys of the surviving pool entries in
 * kb[0 .. ctl->npool) and the surviving new entries in kb[npool .. npool +
 * ctl->nnew), as final keys (GIVEN) or as (all ones << 32 | id); every other
 * slot of kb[0 .. P) is PJ_NONE. Ends with a barrier. */
template <bool GIVEN>
DEV void pj_dedupe(PjCtl* ctl, uint64_t* ka, uint64_t* kb, float* dd, int P, int32_t node,
                   const int32_t* __restrict__ pool_ids, const float* __restrict__ pool_dists,
                   int npool, const int32_t* __restrict__ new_ids,
                   const float* __restrict__ new_dists, int nnew)
{
    for (int e = threadIdx.x; e < P; e += blockDim.x) {
        uint64_t key = PJ_NONE;
        if (e < npool + nnew) {
            const bool pool = e < npool;
            const int32_t id = pool ? pool_ids[e] : new_ids[e - npool];
            bool valid = id >= 0 && id != node;
            if (pool || GIVEN) {
                const float v = pool ? pool_dists[e] : new_dists[e - npool];
                dd[e] = v;
                valid = valid && __builtin_isfinite(v);
            }
            if (valid) key = ((uint64_t)(uint32_t)id << 32) | (uint32_t)e;
        }
        ka[e] = key;
        kb[e] = PJ_NONE;
    }
    if (threadIdx.x == 0) { ctl->npool = 0; ctl->nnew = 0; }
    pj_sort(ka, P);
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const uint64_t key = ka[i];
        if (key == PJ_NONE) continue;
        const uint32_t id = (uint32_t)(key >> 32);
        if (i > 0 && (uint32_t)(ka[i - 1] >> 32) == id) continue;   /* not a run's first */
        const int e = (int)(uint32_t)key;
        const bool pool = e < npool;
        float best = 0.0f;
        if (pool || GIVEN) {
            best = dd[e];
            for (int j = i + 1; j < P; j++) {
                const uint64_t kj = ka[j];
                const int ej = (int)(uint32_t)kj;
                if ((uint32_t)(kj >> 32) != id || (pool && ej >= npool)) break;
                const float v = dd[ej];
                if (v < best) best = v;      /* entries come in list order */
            }
        }
        if (pool)
            kb[atomicAdd(&ctl->npool, 1)] = pj_pack(best, (int32_t)id);
        else
            kb[npool + atomicAdd(&ctl->nnew, 1)] =
                GIVEN ? pj_pack(best, (int32_t)id) : (0xffffffffull << 32) | id;
    }
    __syncthreads();
}

/* select: sort the slots in use and write the row. Every new survivor has
 * its final key. */
DEV void pj_select(const PjCtl* ctl, uint64_t* kb, int npool, int kout,
                   int32_t* __restrict__ out_ids, float* __restrict__ out_dists)
{
    const int nn = ctl->nnew, total = ctl->npool + nn;
    const int P = pj_pow2(npool + nn);
    pj_sort(kb, P);
    for (int i = threadIdx.x; i < kout; i += blockDim.x) {
        const bool in = i < total;
        const uint64_t key = in ? kb[i] : PJ_NONE;
        out_ids[i] = in ? (int32_t)(uint32_t)key : -1;
        out_dists[i] = in ? pj_unpack_dist(key) : __builtin_inff();
    }
}

template <int CTRL>
DEV int dpp_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

/* f32_fold for one pair: lane g's accumulator `a` of the reference's 16,
 * q and r at the first column of the last slab, which starts at column k0.
 * The distance, on lane g == 0 of the group. */
template <int DM>
DEV float pj_fold_f32(float a, const float* q, const float* r, int k0, int d, int g)
{
    const int nd16 = d & ~15, nd8 = d & ~7, nd4 = d & ~3;
    const int tc = nd16 - k0;
    a = a + dpp<DPP_ROW_SHL8>(a);
    if (nd8 > nd16) a = g < 8 ? xstep<DM>(q[tc + g], r[tc + g], a) : a;
    a = a + dpp<DPP_ROW_SHL4>(a);
    if (nd4 > nd8)
        a = g < 4 ? xstep<DM>(q[tc + (nd8 - nd16) + g], r[tc + (nd8 - nd16) + g], a) : a;
    float s = ((dpp<DPP_QUAD0>(a) + dpp<DPP_QUAD1>(a)) + dpp<DPP_QUAD2>(a)) + dpp<DPP_QUAD3>(a);
    for (int c = nd4; c < d; c++) s = xstep<DM>(q[c - k0], r[c - k0], s);
    return (DM == DM_L2) ? s : 1.0f - s;
}

__global__ __launch_bounds__(XTHREADS)
void pool_join_given_kernel(const int32_t* __restrict__ nodes,
                            const int32_t* pool_ids, const float* pool_dists, int npool,
                            const int32_t* __restrict__ new_ids,
                            const float* __restrict__ new_dists, int nnew, int kout,
                            int32_t* out_ids, float* out_dists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const PjLds L = pj_lds(npool, nnew, true, 0, 0);
    PjCtl* ctl = (PjCtl*)(xlds + L.ctl);
    uint64_t* kb = (uint64_t*)(xlds + L.b);
    const size_t row = blockIdx.x;
    pj_dedupe<true>(ctl, (uint64_t*)(xlds + L.a), kb, (float*)(xlds + L.dd),
                    pj_pow2(npool + nnew), nodes[row], pool_ids + row * npool,
                    pool_dists + row * npool, npool, new_ids + row * nnew,
                    new_dists + row * nnew, nnew);
    pj_select(ctl, kb, npool, kout, out_ids + row * kout, out_dists + row * kout);
}

/* ONE: d <= PJ_KS, a single slab, the node's columns in registers */
template <int DM, bool ONE>
__global__ __launch_bounds__(XTHREADS)
void pool_join_f32_kernel(const float* __restrict__ vectors, int d,
                          const int32_t* __restrict__ nodes,
                          const int32_t* pool_ids, const float* pool_dists, int npool,
                          const int32_t* __restrict__ new_ids, int nnew, int kout,
                          int32_t* out_ids, float* out_dists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const PjLds L = pj_lds(npool, nnew, false, (uint32_t)((d + 3) & ~3), PJ_T * PJ_QS);
    PjCtl* ctl = (PjCtl*)(xlds + L.ctl);
    uint64_t* kb = (uint64_t*)(xlds + L.b);
    float* qv = (float*)(xlds + L.q);
    float* tbuf = (float*)(xlds + L.tile);
    const int tid = threadIdx.x, g = tid & 15, lr = tid >> 4;
    const size_t row = blockIdx.x;
    const int32_t node = nodes[row];
    const bool vec = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;

    /* the node's vector; the barriers of the dedupe stand behind it */
    for (int c = 4 * tid; c < d; c += 4 * XTHREADS)
        *(float4*)(qv + c) = rp_cols4(vectors + (size_t)node * d, d, c, vec);
    pj_dedupe<false>(ctl, (uint64_t*)(xlds + L.a), kb, (float*)(xlds + L.dd),
                     pj_pow2(npool + nnew), node, pool_ids + row * npool,
                     pool_dists + row * npool, npool, new_ids + row * nnew, nullptr, nnew);

    const int nn = ctl->nnew;
    const int nslab = (d + PJ_KS - 1) / PJ_KS, nstep = ((nn + PJ_T - 1) / PJ_T) * nslab;
    float xq[PJ_KS / 16];
    if constexpr (ONE) {
#pragma unroll
        for (int c = 0; c < PJ_KS / 16; c++) xq[c] = c * 16 + 16 <= d ? qv[c * 16 + g] : 0.0f;
    }
    /* this thread's columns 4*(g + 16*k) of candidate lr of a tile, one slab */
    float4 pre[PJ_KS / 64];
    auto slab_load = [&](int step) {
        const int t = step / nslab, slab = step - t * nslab, w = t * PJ_T + lr;
        const float* p = w < nn ? vectors + (size_t)(uint32_t)kb[npool + w] * d : nullptr;
#pragma unroll
        for (int k = 0; k < PJ_KS / 64; k++)
            pre[k] = rp_cols4(p, d, slab * PJ_KS + 4 * (g + 16 * k), vec);
    };
    if (nstep > 0) slab_load(0);
    float acc = 0.0f;
    for (int step = 0; step < nstep; step++) {
        const int t = step / nslab, slab = step - t * nslab;
#pragma unroll
        for (int k = 0; k < PJ_KS / 64; k++)
            *(float4*)(tbuf + lr * PJ_QS + 4 * (g + 16 * k)) = pre[k];
        __syncthreads();
        if (step + 1 < nstep) slab_load(step + 1);   /* in flight during the math */
        const float* qb = qv + slab * PJ_KS;
        const float* rb = tbuf + lr * PJ_QS;
        if (slab == 0) acc = 0.0f;
#pragma unroll
        for (int c = 0; c < PJ_KS / 16; c++) {
            if (slab * PJ_KS + c * 16 + 16 > d) break;
            acc = xstep<DM>(ONE ? xq[c] : qb[c * 16 + g], rb[c * 16 + g], acc);
        }
        if (slab == nslab - 1) {
            const float dist = pj_fold_f32<DM>(acc, qb, rb, slab * PJ_KS, d, g);
            const int w = t * PJ_T + lr;
            if (g == 0 && w < nn) kb[npool + w] = pj_pack(dist, (int32_t)(uint32_t)kb[npool + w]);
        }
        __syncthreads();    /* the slab is free */
    }
    pj_select(ctl, kb, npool, kout, out_ids + row * kout, out_dists + row * kout);
}

template <int DM>
__global__ __launch_bounds__(XTHREADS)
void pool_join_i8_kernel(const int8_t* __restrict__ vectors, int d,
                         const int32_t* __restrict__ nodes,
                         const int32_t* pool_ids, const float* pool_dists, int npool,
                         const int32_t* __restrict__ new_ids, int nnew, int kout,
                         int32_t* out_ids, float* out_dists)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const PjLds L = pj_lds(npool, nnew, false, 0, 0);
    PjCtl* ctl = (PjCtl*)(xlds + L.ctl);
    uint64_t* kb = (uint64_t*)(xlds + L.b);
    const int tid = threadIdx.x, g = tid & 15, lr = tid >> 4;
    const size_t row = blockIdx.x;
    const int32_t node = nodes[row];
    const int W = (d + 3) >> 2;
    /* a lane's dwords of a row: 4g .. 4g+3 by one 16-byte load when rows are
     * 16-byte multiples, else g + 16*j, loaded whole or packed from bytes.
     * Both operands of a dot use the same assignment, which is all it needs. */
    const bool v16 = (d & 15) == 0 && ((uintptr_t)vectors & 15) == 0;
    const bool v4 = (d & 3) == 0 && ((uintptr_t)vectors & 3) == 0;
    auto row_load = [&](int32_t id, uint32_t (&v)[PJ_I8_NW]) {
#pragma unroll
        for (int j = 0; j < PJ_I8_NW; j++) v[j] = 0u;
        if (id < 0) return;
        if (v16) {
            if (4 * g < W) {
                const uint4 x = *(const uint4*)(vectors + (size_t)id * d + 16 * g);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < PJ_I8_NW; j++) {
            const int w = g + 16 * j;
            if (w < W)
                v[j] = v4 ? ((const uint32_t*)(vectors + (size_t)id * d))[w]
                          : i8_pack_dword(vectors, id, w, d);
        }
    };
    uint32_t qd[PJ_I8_NW], cur[PJ_I8_NW], nxt[PJ_I8_NW];
    row_load(node, qd);
    int aa = 0;
#pragma unroll
    for (int j = 0; j < PJ_I8_NW; j++)
        aa = __builtin_amdgcn_sdot4((int)qd[j], (int)qd[j], aa, false);
    pj_dedupe<false>(ctl, (uint64_t*)(xlds + L.a), kb, (float*)(xlds + L.dd),
                     pj_pow2(npool + nnew), node, pool_ids + row * npool,
                     pool_dists + row * npool, npool, new_ids + row * nnew, nullptr, nnew);

    const int nn = ctl->nnew, ntile = (nn + PJ_T - 1) / PJ_T;
    auto cand_load = [&](int t, uint32_t (&v)[PJ_I8_NW]) {
        const int w = t * PJ_T + lr;
        row_load(w < nn ? (int32_t)(uint32_t)kb[npool + w] : -1, v);
    };
    if (ntile > 0) cand_load(0, nxt);
    for (int t = 0; t < ntile; t++) {
#pragma unroll
        for (int j = 0; j < PJ_I8_NW; j++) cur[j] = nxt[j];
        if (t + 1 < ntile) cand_load(t + 1, nxt);    /* in flight during the dots */
        int ab = 0, bb = 0;
#pragma unroll
        for (int j = 0; j < PJ_I8_NW; j++) {
            ab = __builtin_amdgcn_sdot4((int)qd[j], (int)cur[j], ab, false);
            if (DM == DM_L2) bb = __builtin_amdgcn_sdot4((int)cur[j], (int)cur[j], bb, false);
        }
        int s = (DM == DM_L2) ? aa - 2 * ab + bb : ab;    /* this lane's share */
        s += dpp_i<DPP_ROW_SHL8>(s);
        s += dpp_i<DPP_ROW_SHL4>(s);
        s = dpp_i<DPP_QUAD0>(s) + dpp_i<DPP_QUAD1>(s) + dpp_i<DPP_QUAD2>(s) + dpp_i<DPP_QUAD3>(s);
        const float dist = (DM == DM_L2) ? (float)s : (float)(16129 - s);
        const int w = t * PJ_T + lr;
        if (g == 0 && w < nn) kb[npool + w] = pj_pack(dist, (int32_t)(uint32_t)kb[npool + w]);
    }
    pj_select(ctl, kb, npool, kout, out_ids + row * kout, out_dists + row * kout);
}

/* ------------------------------------------------------------------ *
 * K-means assign: segmented nearest-center step
 * ------------------------------------------------------------------ *
 * Segment s has a slice of the member list and at most 64 centers of its own.
 * A workgroup owns one KmItem, a run of consecutive members of one segment,
 * and walks it in tiles. The centers are the LDS-resident side, the "query
 * tile" of the kernels above (32 slots, or 64 for kmax > 32); a member's
 * vector is gathered from global memory once, into LDS, and serves the
 * distances and then the sums.
 *
 *   dists   f32: tiles of 16 members, the micro-tiles and the reference-order
 *           fold of the kernels above. RES: centers and tile whole in LDS,
 *           the next tile's loads in flight in registers during the math.
 *           Otherwise (large dims) centers and tile stream through LDS in
 *           slabs of FKS columns with the accumulators kept, the next slab's
 *           loads in flight.
 *           int8: tiles of 64 members, one 32x32 MFMA block per wave (two
 *           member blocks x one or two center blocks), everything resident.
 *   choose  The tile's distances go through LDS as [member][center]; a wave
 *           takes a member at a time, lane k adds center k's penalty (an f32
 *           product and an f32 sum, each rounded once) and a butterfly over
 *           (dist, k) keeps the smallest qualifying distance, the lowest k
 *           among equals: the serial rule's answer.
 *   counts  Per item in LDS, then one integer atomic per center.
 *   extreme A 64-bit key (order-preserving f32 bits, -0 folded to +0, above
 *           the complemented position) goes through an LDS atomic max
 *           (update) or min, then one global atomic per center and item: the
 *           largest distance at the smallest position, or the smallest
 *           distance at the largest position, whatever the arrival order.
 *   sums    The item's sums live in LDS as [center][column], a thread owning
 *           its columns and adding the members in order: no atomics. Where
 *           every column fits beside the resident tile they are added tile
 *           by tile from LDS, the one read serving both. Where they do not
 *           (the streaming f32 form; int8 with kmax > 32 and d > 48) the
 *           item's labels stay in LDS and its vectors are read a second
 *           time after the last tile, a slab of columns at a time. Each
 *           item writes its partial; kmeans_finish_kernel adds the partials
 *           of a segment in list order (int8: as 64-bit integers, rounded
 *           once), so equal calls give equal bytes. */

enum { KM_MAX_K = KMEANS_MAX_K, KM_ITEM_MAX = KMEANS_ITEM_MAX, KM_IT = 64, KM_DS = KM_MAX_K + 1,
       KM_PF = 8, KM_ITEMS_TARGET = 2048, KM_LDS_MAX = RP_LDS_MAX };
static_assert(KM_MAX_K == 2 * XQT && KM_IT == 2 * RI_T, "two query tiles, two MFMA blocks");

struct KmLds { uint32_t ext, cnt, aux, lab, dmat, cen, tile, sums, total; int ss; };

/* cen_words / tile_words: dwords of the centers and of a tile (or of their
 * slabs), trows: members of a tile. ss: columns of the sums that fit (a
 * multiple of 4, at most the padded dim; 0 without update). */
static inline __host__ __device__ KmLds km_lds(uint32_t cen_words, uint32_t tile_words,
                                               int trows, int kmax, int d, int update)
{
    KmLds l;
    uint32_t b = 0;
    l.ext = b;  b += KM_MAX_K * 8;
    l.cnt = b;  b += KM_MAX_K * 4;
    l.aux = b;  b += (KM_MAX_K + 2 * KM_IT) * 4;   /* int8: center self-dots, tile ids */
    l.lab = b;  b += KM_ITEM_MAX;
    l.dmat = b; b += (uint32_t)trows * KM_DS * 4;
    b = (b + 15) & ~15u;
    l.cen = b;  b += cen_words * 4;
    b = (b + 15) & ~15u;
    l.tile = b; b += tile_words * 4;
    b = (b + 15) & ~15u;
    l.sums = b;
    l.ss = 0;
    if (update && b < KM_LDS_MAX) {
        const int room = (int)((KM_LDS_MAX - b) / ((uint32_t)kmax * 4)) & ~3;
        const int dp = (d + 3) & ~3;
        l.ss = room < dp ? room : dp;
    }
    b += (uint32_t)l.ss * kmax * 4;
    l.total = b;
    return l;
}

static inline __host__ __device__ KmLds km_f32_lds(int d, int nqt, int kmax, int update, bool res)
{
    const int qs = res ? f32_qstride(d) : FQSS;
    return km_lds((uint32_t)(nqt * XQT * qs), (uint32_t)(FRT * qs), FRT, kmax, d, update);
}

/* whether the f32 kernel keeps the centers and a tile whole, and with update
 * every column of the sums beside them */
static inline __host__ __device__ bool km_f32_resident(int d, int nqt, int kmax, int update)
{
    if (f32_qstride(d) > FQRES_MAX) return false;
    const KmLds l = km_f32_lds(d, nqt, kmax, update, true);
    return l.total <= KM_LDS_MAX && (!update || l.ss >= d);
}

static inline __host__ __device__ KmLds km_i8_lds(int d, int ncb, int kmax, int update)
{
    const uint32_t wl = (uint32_t)((d + 3) >> 2) | 1;
    return km_lds(ncb * XQT * wl, KM_IT * wl, KM_IT, kmax, d, update);
}

struct KmCtx {
    unsigned long long* ext;    /* LDS [KM_MAX_K] */
    int* cnt;                   /* LDS [KM_MAX_K] */
    uint8_t* lab;               /* LDS [KM_ITEM_MAX]: the labels of the item's members */
    float* dmat;                /* LDS [tile rows][KM_DS] */
    int nc;
    bool haspen;
    float pen;                  /* lane k: lambda * prev_counts[k] */
};

/* Empty counts and extremes, this lane's penalty. Ends with a barrier. */
DEV KmCtx km_begin(unsigned char* lds, const KmLds& L, const KmArgs& A, const KmItem& it, int nc)
{
    KmCtx c;
    c.ext = (unsigned long long*)(lds + L.ext);
    c.cnt = (int*)(lds + L.cnt);
    c.lab = lds + L.lab;
    c.dmat = (float*)(lds + L.dmat);
    c.nc = nc;
    c.haspen = A.lambdas != nullptr;
    c.pen = 0.0f;
    const int lane = threadIdx.x & 63;
    if (c.haspen && lane < nc)
        c.pen = __fmul_rn(A.lambdas[it.seg], (float)A.prev_counts[(size_t)it.seg * A.kmax + lane]);
    if (threadIdx.x < KM_MAX_K) {
        c.cnt[threadIdx.x] = 0;
        c.ext[threadIdx.x] = A.update ? 0ull : ~0ull;
    }
    uint32_t* sums = (uint32_t*)(lds + L.sums);
    for (int i = threadIdx.x; i < L.ss * A.kmax; i += blockDim.x) sums[i] = 0u;
    __syncthreads();
    return c;
}

/* One wave settles rows [row0, row0 + nrows) of dmat; row r is member m0 + r
 * of the item. Lane k speaks for center k. */
DEV void km_choose(const KmCtx& c, const KmArgs& A, const KmItem& it, int row0, int nrows, int m0)
{
    const int lane = threadIdx.x & 63;
    for (int r = row0; r < row0 + nrows && m0 + r < it.count; r++) {
        float v = c.dmat[r * KM_DS + lane];
        if (c.haspen) v = __fadd_rn(v, c.pen);
        const bool ok = lane < c.nc && v > -MAXDIST && v < MAXDIST;
        float bv = ok ? v : MAXDIST;
        int bk = ok ? lane : (int)KM_MAX_K;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int ok2 = __shfl_xor(bk, o);
            if (ov < bv || (ov == bv && ok2 < bk)) { bv = ov; bk = ok2; }
        }
        if (bk == KM_MAX_K) bk = 0;     /* no center qualifies: label 0 at MaxDist */
        if (lane == 0) {
            const int mi = m0 + r;
            A.out_labels[(size_t)it.start + mi] = bk;
            if (A.out_dists) A.out_dists[(size_t)it.start + mi] = bv;
            c.lab[mi] = (uint8_t)bk;
            atomicAdd(&c.cnt[bk], 1);
            const unsigned long long key = pj_pack(bv, (int32_t)~(uint32_t)(it.pos0 + mi));
            if (A.update) atomicMax(&c.ext[bk], key);
            else atomicMin(&c.ext[bk], key);
        }
    }
}

/* the item's counts and extremes to the segment's. Starts with a barrier. */
DEV void km_end(const KmCtx& c, const KmArgs& A, const KmItem& it)
{
    __syncthreads();
    const int k = threadIdx.x;
    if (k < c.nc && c.cnt[k] > 0) {
        const size_t at = (size_t)it.seg * A.kmax + k;
        atomicAdd(&A.out_counts[at], c.cnt[k]);
        if (A.update) atomicMax(&A.keys[at], c.ext[k]);
        else atomicMin(&A.keys[at], c.ext[k]);
    }
}

/* columns [0, ncol) of the sums += members m0 .. m0 + nm - 1 of the item, in
 * that order; src(mi, c): column c of member mi. A thread owns its columns. */
template <class ACC, class SRC>
DEV void km_accumulate(ACC* sums, int ss, const uint8_t* lab, int m0, int nm, int ncol, SRC src)
{
    for (int c = threadIdx.x; c < ncol; c += blockDim.x)
        for (int m = 0; m < nm; m += KM_PF) {
            ACC v[KM_PF];
#pragma unroll
            for (int j = 0; j < KM_PF; j++) v[j] = m + j < nm ? src(m0 + m + j, c) : (ACC)0;
#pragma unroll
            for (int j = 0; j < KM_PF; j++)
                if (m + j < nm) sums[lab[m0 + m + j] * ss + c] += v[j];
        }
}

/* columns [0, ncol) of the sums to `part` (the item's partial at the slab's
 * first column), and cleared. Barriers before and after. */
template <class ACC>
DEV void km_flush_sums(ACC* sums, int ss, int nc, int ncol, ACC* __restrict__ part, int d)
{
    __syncthreads();
    for (int i = threadIdx.x; i < nc * ncol; i += blockDim.x) {
        const int k = i / ncol, c = i - k * ncol;
        part[(size_t)k * d + c] = sums[k * ss + c];
        sums[k * ss + c] = (ACC)0;
    }
    __syncthreads();
}

/* the sums of a resident tile (members m0 .. m0 + nm - 1, `last`: the item's
 * last); every column fits (ss >= d). Ends with a barrier. */
template <class ACC, class SRC>
DEV void km_tile_sums(ACC* sums, int ss, const KmCtx& c, int m0, int nm, bool last, int d,
                      ACC* __restrict__ part, SRC src)
{
    km_accumulate(sums, ss, c.lab, m0, nm, d, src);
    if (last) km_flush_sums(sums, ss, c.nc, d, part, d);
    else __syncthreads();
}

/* the sums of the whole item after its last tile, a slab of ss columns at a
 * time, from the labels in LDS; src(mi, c) reads the vectors again */
template <class ACC, class SRC>
DEV void km_item_sums(ACC* sums, int ss, const KmCtx& c, int count, int d,
                      ACC* __restrict__ part, SRC src)
{
    for (int c0 = 0; c0 < d; c0 += ss) {
        const int ncol = min(ss, d - c0);
        km_accumulate(sums, ss, c.lab, 0, count, ncol,
                      [&](int mi, int col) { return src(mi, c0 + col); });
        km_flush_sums(sums, ss, c.nc, ncol, part + c0, d);
    }
}

__global__ __launch_bounds__(256)
void kmeans_init_kernel(KmArgs A)
{
    const size_t total = (size_t)A.nseg * A.kmax;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (size_t)gridDim.x * 256) {
        if ((int)(i % A.kmax) >= A.segs[i / A.kmax].ncenters) continue;
        A.out_counts[i] = 0;
        A.keys[i] = A.update ? 0ull : ~0ull;
    }
}

/* block (s, y): the extremes of segment s (y == 0) and columns of its sums */
template <bool I8>
__global__ __launch_bounds__(256)
void kmeans_finish_kernel(KmArgs A, int d)
{
    const int s = blockIdx.x;
    const KmSeg sg = A.segs[s];
    const size_t at = (size_t)s * A.kmax;
    if (blockIdx.y == 0 && (int)threadIdx.x < sg.ncenters) {
        const int k = threadIdx.x;
        const bool any = A.out_counts[at + k] > 0;
        const unsigned long long key = A.keys[at + k];
        /* the key's low word is the complemented position in the segment */
        const size_t first = sg.nitems > 0 ? (size_t)A.items[sg.item0].start : 0;
        A.out_cluster_idx[at + k] = any ? A.members[first + (uint32_t)~(uint32_t)key] : -1;
        A.out_cluster_dist[at + k] = any ? pj_unpack_dist(key) : (A.update ? -MAXDIST : MAXDIST);
    }
    if (!A.update) return;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= sg.ncenters * d) return;
    const size_t stride = (size_t)A.kmax * d;
    if (I8) {
        const int32_t* p = (const int32_t*)A.partials + (size_t)sg.item0 * stride + i;
        long long acc = 0;
        for (int j = 0; j < sg.nitems; j++) acc += p[j * stride];
        A.out_sums[at * d + i] = (float)acc;
    } else {
        const float* p = (const float*)A.partials + (size_t)sg.item0 * stride + i;
        float acc = 0.0f;
        for (int j = 0; j < sg.nitems; j++) acc += p[j * stride];
        A.out_sums[at * d + i] = acc;
    }
}

/* NQT: query tiles of 32 center slots (2 for kmax > 32) */
template <int DM, bool RES, int NQT>
__global__ __launch_bounds__(XTHREADS)
void kmeans_f32_kernel(const float* __restrict__ vectors, int d, KmArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int qs = RES ? f32_qstride(d) : FQSS;     /* row stride of both buffers */
    const KmLds L = km_f32_lds(d, NQT, A.kmax, A.update, RES);
    float* cbuf = (float*)(xlds + L.cen);       /* the centers (or their slab) */
    float* tbuf = (float*)(xlds + L.tile);      /* the tile's vectors (or their slab) */
    float* sums = (float*)(xlds + L.sums);
    const int tid = threadIdx.x;
    const int g = tid & 15, gq = (tid >> 4) & 3, gr = tid >> 6, lr = tid >> 4;
    const KmItem it = A.items[blockIdx.x];
    const int nc = A.segs[it.seg].ncenters;
    const float* cen = (const float*)A.centers + (size_t)it.seg * A.kmax * d;
    const int32_t* mem = A.members + it.start;
    float* part = A.update ? (float*)A.partials + (size_t)blockIdx.x * A.kmax * d : nullptr;
    const bool vec = (d & 3) == 0 && ((uintptr_t)vectors & 15) == 0;
    const bool vecc = (d & 3) == 0 && ((uintptr_t)A.centers & 15) == 0;
    const bool two = NQT == 2 && nc > XQT;      /* the second center tile is in use */
    const KmCtx ctx = km_begin(xlds, L, A, it, nc);

    const int nslab = (d + FKS - 1) / FKS;
    const int ntile = (it.count + FRT - 1) / FRT;   /* >= 1: an item is not empty */
    /* the vector of member lr of tile t, null past the item's end */
    auto row_of = [&](int32_t id) { return id >= 0 ? vectors + (size_t)id * d : nullptr; };
    auto tile_id = [&](int t) { return t * FRT + lr < it.count ? mem[t * FRT + lr] : -1; };
    float a0[FMQ][FMR], a1[FMQ][FMR];
    /* after a tile's last slab: the distances to LDS, the members settled */
    auto settle = [&](int t, const float* qa, const float* rb, int slab) {
        float d0[FMQ], d1[FMQ] = {};
        rp_fold<DM, FMQ>(a0, qa, rb, qs, qs, slab, d, g, d0);
        if (two) rp_fold<DM, FMQ>(a1, qa + XQT * qs, rb, qs, qs, slab, d, g, d1);
        if (g < FMR) {      /* member gr*4 + g of the tile against centers gq + 4*i (+ 32) */
            float* row = ctx.dmat + (gr * FMR + g) * KM_DS;
#pragma unroll
            for (int i = 0; i < FMQ; i++) {
                row[gq + 4 * i] = d0[i];
                if (NQT == 2) row[XQT + gq + 4 * i] = d1[i];
            }
        }
        __syncthreads();
        km_choose(ctx, A, it, gr * FMR, FMR, t * FRT);
        __syncthreads();
    };

    if constexpr (RES) {
        for (int i = tid; i < NQT * XQT * qs; i += XTHREADS) {
            const int r = i / qs, c = i - r * qs;
            cbuf[i] = (r < nc && c < d) ? cen[(size_t)r * d + c] : 0.0f;
        }
        /* this thread's columns 4*(g + 16*k) of row lr of a tile */
        float4 pre[FQRES_MAX / 64];
        auto tile_load = [&](int32_t id) {
            const float* p = row_of(id);
#pragma unroll
            for (int k = 0; k < FQRES_MAX / 64; k++) {
                const int col = 4 * (g + 16 * k);
                if (col < qs) pre[k] = rp_cols4(p, d, col, vec);
            }
        };
        auto tile_store = [&]() {
#pragma unroll
            for (int k = 0; k < FQRES_MAX / 64; k++) {
                const int col = 4 * (g + 16 * k);
                if (col < qs) *(float4*)(tbuf + lr * qs + col) = pre[k];
            }
        };
        int32_t idn = tile_id(1);       /* ids are read a tile ahead of their vectors */
        tile_load(tile_id(0));
        tile_store();
        __syncthreads();
        for (int t = 0; t < ntile; t++) {
            if (t + 1 < ntile) {        /* in flight while this tile computes */
                tile_load(idn);
                idn = tile_id(t + 2);
            }
            for (int slab = 0; slab < nslab; slab++) {
                const float* qa = cbuf + gq * qs + slab * FKS;
                const float* rb = tbuf + gr * FMR * qs + slab * FKS;
                rp_math<DM, FMQ>(a0, qa, rb, qs, qs, slab, d, g);
                if (two) rp_math<DM, FMQ>(a1, qa + XQT * qs, rb, qs, qs, slab, d, g);
                if (slab == nslab - 1) settle(t, qa, rb, slab);
            }
            if (A.update)
                km_tile_sums(sums, L.ss, ctx, t * FRT, min((int)FRT, it.count - t * FRT),
                             t + 1 == ntile, d, part,
                             [&](int mi, int c) { return tbuf[(mi - t * FRT) * qs + c]; });
            if (t + 1 < ntile) {
                tile_store();
                __syncthreads();
            }
        }
    } else {
        /* step st is slab st % nslab of tile st / nslab; this thread's columns
         * of member lr and of centers lr + 16*q */
        float4 pr, pc[NQT * 2];
        auto slab_load = [&](int st) {
            const int t = st / nslab, k0 = (st - t * nslab) * FKS;
            pr = f32_cols_load(row_of(tile_id(t)), d, k0, vec);
#pragma unroll
            for (int q = 0; q < NQT * 2; q++) {
                const int k = q * 16 + lr;
                pc[q] = f32_cols_load(k < nc ? cen + (size_t)k * d : nullptr, d, k0, vecc);
            }
        };
        const int nstep = ntile * nslab;
        slab_load(0);
        for (int st = 0; st < nstep; st++) {
            const int t = st / nslab, slab = st - t * nslab;
            f32_slab_store(tbuf, FQSS, pr);
#pragma unroll
            for (int q = 0; q < NQT * 2; q++) f32_slab_store(cbuf, FQSS, pc[q], q * 16);
            __syncthreads();
            if (st + 1 < nstep) slab_load(st + 1);      /* in flight during the math */
            const float* qa = cbuf + gq * qs;
            const float* rb = tbuf + gr * FMR * qs;
            rp_math<DM, FMQ>(a0, qa, rb, qs, qs, slab, d, g);
            if (two) rp_math<DM, FMQ>(a1, qa + XQT * qs, rb, qs, qs, slab, d, g);
            if (slab == nslab - 1) settle(t, qa, rb, slab);
            __syncthreads();    /* the slab is free */
        }
        if (A.update) {
            __syncthreads();
            km_item_sums(sums, L.ss, ctx, it.count, d, part,
                         [&](int mi, int c) { return vectors[(size_t)mem[mi] * d + c]; });
        }
    }
    km_end(ctx, A, it);
}

/* NCB: 32-center MFMA blocks (2 for kmax > 32); 64 * 2 * NCB threads */
template <int DM, int NCB>
__global__ __launch_bounds__(128 * NCB)
void kmeans_i8_kernel(const int8_t* __restrict__ vectors, int d, KmArgs A)
{
    enum { NT = 128 * NCB, NP = (KM_IT * I_MAX_W + NT - 1) / NT, RPW = KM_IT / (2 * NCB) };
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int W = (d + 3) >> 2, WL = W | 1;
    const KmLds L = km_i8_lds(d, NCB, A.kmax, A.update);
    uint32_t* cl = (uint32_t*)(xlds + L.cen);       /* [NCB * 32][WL] the centers */
    uint32_t* tl = (uint32_t*)(xlds + L.tile);      /* [KM_IT][WL] the tile's vectors */
    int* caa = (int*)(xlds + L.aux);                /* the centers' self-dots */
    int32_t* mids = caa + KM_MAX_K;                 /* [2][KM_IT], by tile parity */
    int* sums = (int*)(xlds + L.sums);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mb = wave & 1, cb = wave >> 1, h = lane >> 5, col = lane & 31;
    const KmItem it = A.items[blockIdx.x];
    const int nc = A.segs[it.seg].ncenters;
    const int8_t* cen = (const int8_t*)A.centers + (size_t)it.seg * A.kmax * d;
    const int32_t* mem = A.members + it.start;
    int* part = A.update ? (int*)A.partials + (size_t)blockIdx.x * A.kmax * d : nullptr;
    /* whole dwords to a row, dword aligned: loaded into registers a tile
     * ahead; other pitches are packed from bytes at the store */
    const bool wide = (d & 3) == 0 && ((uintptr_t)vectors & 3) == 0;
    const bool widec = (d & 3) == 0 && ((uintptr_t)A.centers & 3) == 0;

    for (int i = tid; i < NCB * XQT * W; i += NT) {
        const int r = i / W, w = i - r * W;
        uint32_t v = 0;
        if (r < nc)
            v = widec ? *(const uint32_t*)(cen + (size_t)r * d + 4 * w) : i8_pack_dword(cen, r, w, d);
        cl[r * WL + w] = v;
    }
    /* the member of row tid of tile t, -1 past the item's end */
    auto tile_id = [&](int t) {
        const int ri = t * KM_IT + tid;
        return (tid < KM_IT && ri < it.count) ? mem[ri] : -1;
    };
    if (tid < KM_IT) {
        mids[tid] = tile_id(0);
        mids[KM_IT + tid] = tile_id(1);
    }
    int32_t idn = tile_id(2);           /* ids are read two tiles ahead of their use */
    const KmCtx ctx = km_begin(xlds, L, A, it, nc);
    if (tid < KM_MAX_K) {
        int s = 0;
        if (tid < NCB * XQT)
            for (int w = 0; w < W; w++) {
                const int v = (int)cl[tid * WL + w];
                s = __builtin_amdgcn_sdot4(v, v, s, false);
            }
        caa[tid] = s;
    }

    /* dword j of this thread is dword w of row r of the tile, with
     * r * W + w = tid + j * NT; (r0, w0) is the first */
    const int r0 = tid / W, w0 = tid - r0 * W, dr = NT / W, dw = NT - dr * W;
    uint32_t pre[NP];
    auto stage_load = [&](int t) {
        if (!wide) return;
        const int32_t* ids = mids + (t & 1) * KM_IT;
        int r = r0, w = w0;
#pragma unroll
        for (int j = 0; j < NP; j++) {
            const int32_t id = r < KM_IT ? ids[r] : -1;
            pre[j] = id >= 0 ? ((const uint32_t*)(vectors + (size_t)id * d))[w] : 0u;
            r += dr;
            w += dw;
            if (w >= W) { w -= W; r++; }
        }
    };
    auto stage_store = [&](int t) {
        if (!wide) {
            const int32_t* ids = mids + (t & 1) * KM_IT;
            for (int i = tid; i < KM_IT * W; i += NT) {
                const int r = i / W, w = i - r * W;
                tl[r * WL + w] = ids[r] >= 0 ? i8_pack_dword(vectors, ids[r], w, d) : 0u;
            }
            return;
        }
        int r = r0, w = w0;
#pragma unroll
        for (int j = 0; j < NP; j++) {
            if (r < KM_IT) tl[r * WL + w] = pre[j];
            r += dr;
            w += dw;
            if (w >= W) { w -= W; r++; }
        }
    };

    const int ntile = (it.count + KM_IT - 1) / KM_IT;   /* >= 1 */
    stage_load(0);          /* km_begin's barrier is behind the ids of tiles 0 and 1 */
    stage_store(0);
    __syncthreads();
    const uint32_t* arow = cl + (cb * XQT + col) * WL;
    const uint32_t* brow = tl + (mb * RI_T + col) * WL;
    for (int t = 0; t < ntile; t++) {
        if (t + 1 < ntile) stage_load(t + 1);   /* in flight while this tile computes */
        v16i acc;
        int bb;
        i8_tile_dots<DM>(arow, brow, W, h, acc, bb);
        /* acc[r] is center cb*32 + 8*(r/4) + 4*h + r%4 against member mb*32 + col */
        float* row = ctx.dmat + (mb * RI_T + col) * KM_DS;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int k = cb * XQT + 8 * (r >> 2) + 4 * h + (r & 3);
            row[k] = (DM == DM_L2) ? (float)(caa[k] - 2 * acc[r] + bb) : (float)(16129 - acc[r]);
        }
        __syncthreads();
        km_choose(ctx, A, it, wave * RPW, RPW, t * KM_IT);
        __syncthreads();
        if (A.update && L.ss >= d)
            km_tile_sums(sums, L.ss, ctx, t * KM_IT, min((int)KM_IT, it.count - t * KM_IT),
                         t + 1 == ntile, d, part, [&](int mi, int c) {
                             const uint32_t v = tl[(mi - t * KM_IT) * WL + (c >> 2)];
                             return (int)(int8_t)(v >> (8 * (c & 3)));
                         });
        if (t + 1 < ntile) stage_store(t + 1);
        /* tile t's ids are done with: tile t + 2's take their place */
        if (tid < KM_IT) mids[(t & 1) * KM_IT + tid] = idn;
        idn = tile_id(t + 3);
        __syncthreads();
    }
    if (A.update && L.ss < d)       /* the sums do not fit beside the tile */
        km_item_sums(sums, L.ss, ctx, it.count, d, part,
                     [&](int mi, int c) { return (int)vectors[(size_t)mem[mi] * d + c]; });
    km_end(ctx, A, it);
}

/* ------------------------------------------------------------------ *
 * TP-tree partition: one level of the reference's hyperplane splits
 * (PartitionByTptreeCore, NeighborhoodGraph.h:152-299) over the open segments
 * of a member list, by the rule of include/sptag_amd.h. Four kernels a level:
 *   rule     one workgroup a segment. A thread owns columns (stride
 *            TP_THREADS) and walks the sample rows in order, TP_AHEAD rows'
 *            loads in flight ahead of the dependent adds: every step reads
 *            one row coalesced and the sums have the contract's order. The
 *            variance pass reads the rows again (L2). Var and Mean go to LDS;
 *            T rounds of a workgroup arg-max (wave butterfly, then one entry
 *            a wave in LDS) pick the dimensions. The sample's T columns are
 *            staged as [s][T] f32 over the same LDS; thread t owns trial t
 *            and walks the staged sample twice, every lane at one address (a
 *            broadcast). The winner, or thread 0 for the axis rule, writes
 *            the segment's TptRule.
 *   sides    one workgroup an item, one member a thread: T column loads, the
 *            projection, the side as a bit; ballot and popcount give the
 *            lefts before a member in its wave, LDS the waves before it.
 *   scan     one wave a segment: exclusive scan of the items' left counts.
 *   scatter  one workgroup an item: the stable place of every member, in
 *            `fin` when its child is a leaf already, else in `next`.
 * No loop's end depends on data that a kernel computed.
 * ------------------------------------------------------------------ */

enum {
    TP_THREADS = 256,
    TP_WAVES = TP_THREADS / 64,
    TP_AHEAD = 8,                   /* sample rows in flight in the column walks */
    TP_SCRATCH = 2 * TP_WAVES * 4,  /* the arg-max's entries, in front of Var and Mean */
    TP_LDS_MAX = 65536,
};
static_assert(TPT_MAX_TRIALS <= TP_THREADS && TPT_ITEM == TP_THREADS &&
                  TPT_MAX_SAMPLES * TPT_MAX_DIMS * 4 <= TP_LDS_MAX &&
                  TP_SCRATCH + 8 * MAX_DIM <= TP_LDS_MAX,
              "a trial a thread, a member a thread, the sample in LDS");

/* The contract's arithmetic: f32, rounded once, never fused. The pragma keeps
 * the contract flag off the instruction, so no later pass joins it with a
 * neighbour into an fma; division and square root are the correctly rounded
 * ones (__fsqrt_rn of this toolchain is the native, approximate one). */
DEV float tp_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
DEV float tp_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
DEV float tp_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
DEV float tp_div(float a, float b)
{
#pragma clang fp contract(off)
    return a / b;
}
DEV float tp_sqrt(float a) { return __builtin_sqrtf(a); }

template <class VT>
DEV float tp_load(const VT* __restrict__ vectors, int32_t m, int32_t dim, int k)
{
    return (float)vectors[(size_t)m * dim + k];
}

/* w_0*x_0 + .. + w_{T-1}*x_{T-1}, summed from 0 in order */
DEV float tp_dot(const float* x, const float* w, int T)
{
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < TPT_MAX_DIMS; j++)
        if (j < T) acc = tp_add(acc, tp_mul(w[j], x[j]));
    return acc;
}

/* entry (va, da) ranks before (vb, db): the larger value, a NaN below every
 * number, then the lower index; an index < 0 is no entry */
DEV bool tp_rank_before(float va, int da, float vb, int db)
{
    if (da < 0) return false;
    if (db < 0) return true;
    const bool above = va > vb || (vb != vb && va == va);
    const bool below = vb > va || (va != va && vb == vb);
    return above || (!below && da < db);
}

/* the workgroup's first-ranked entry, in every thread; sv/sd: LDS [TP_WAVES] */
DEV void tp_block_best(float& v, int& d, float* sv, int* sd)
{
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int od = __shfl_xor(d, o);
        if (tp_rank_before(ov, od, v, d)) { v = ov; d = od; }
    }
    __syncthreads();        /* the entries of the round before are read */
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sd[threadIdx.x >> 6] = d; }
    __syncthreads();
    v = sv[0];
    d = sd[0];
    for (int w = 1; w < TP_WAVES; w++)
        if (tp_rank_before(sv[w], sd[w], v, d)) { v = sv[w]; d = sd[w]; }
}

/* draw(t, j) of the segment at (level, first): a pure function of its key */
DEV uint32_t tp_draw(uint64_t seed, uint32_t level, uint32_t first, uint32_t t, uint32_t j)
{
    const uint64_t key = ((((((uint64_t)level << 31) | first) << 8) | t) << 3) | j;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (1 + key);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32) % 10000u;
}

/* one column's walk over the sample rows: f(acc, x) in row order */
template <class VT, class F>
DEV float tp_column_walk(const VT* __restrict__ vectors, int32_t dim, const int32_t* mem, int s,
                         int k, F f)
{
    float acc = 0.f;
    int i = 0;
    for (; i + TP_AHEAD <= s; i += TP_AHEAD) {
        float x[TP_AHEAD];
#pragma unroll
        for (int u = 0; u < TP_AHEAD; u++) x[u] = tp_load(vectors, mem[i + u], dim, k);
#pragma unroll
        for (int u = 0; u < TP_AHEAD; u++) acc = f(acc, x[u]);
    }
    for (; i < s; i++) acc = f(acc, tp_load(vectors, mem[i], dim, k));
    return acc;
}

template <class VT>
__global__ __launch_bounds__(TP_THREADS)
void tpt_rule_kernel(const VT* __restrict__ vectors, int32_t dim, TptArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const TptSeg sg = A.segs[blockIdx.x];
    const int tid = threadIdx.x;
    const int s = min(A.samples, sg.count), T = min(A.topdims, dim);
    const int32_t* mem = A.cur + sg.first;
    const float fs = (float)s;
    float* sv = (float*)xlds;                   /* [TP_WAVES] */
    int* sd = (int*)(sv + TP_WAVES);            /* [TP_WAVES] */
    float* var = (float*)(xlds + TP_SCRATCH);   /* [dim] */
    float* mean = var + dim;                    /* [dim] */
    float* stage = (float*)xlds;                /* [s][T], once var and mean are read */

    for (int k = tid; k < dim; k += TP_THREADS) {
        const float sum = tp_column_walk(vectors, dim, mem, s, k,
                                         [](float a, float x) { return tp_add(a, x); });
        const float mu = tp_div(sum, fs);
        var[k] = tp_column_walk(vectors, dim, mem, s, k, [mu](float a, float x) {
            const float df = tp_sub(x, mu);
            return tp_add(a, tp_mul(df, df));
        });
        mean[k] = mu;
    }
    __syncthreads();

    int idx[TPT_MAX_DIMS];
#pragma unroll
    for (int r = 0; r < TPT_MAX_DIMS; r++) {
        idx[r] = 0;
        if (r < T) {        /* uniform: the barriers inside are met by all */
            float bv = 0.f;
            int bd = -1;
            for (int k = tid; k < dim; k += TP_THREADS) {
                bool taken = false;
#pragma unroll
                for (int q = 0; q < TPT_MAX_DIMS; q++) taken |= q < r && idx[q] == k;
                const float vk = var[k];
                if (!taken && tp_rank_before(vk, k, bv, bd)) { bv = vk; bd = k; }
            }
            tp_block_best(bv, bd, sv, sd);
            idx[r] = bd;
        }
    }
    const float axis_var = var[idx[0]], axis_mean = mean[idx[0]];
    __syncthreads();

    for (int i = tid; i < s; i += TP_THREADS) {
        const int32_t m = mem[i];
#pragma unroll
        for (int j = 0; j < TPT_MAX_DIMS; j++)
            if (j < T) stage[i * T + j] = tp_load(vectors, m, dim, idx[j]);
    }
    __syncthreads();

    float w[TPT_MAX_DIMS], tvar = 0.f, tmean = 0.f;
    int tt = -1;
#pragma unroll
    for (int j = 0; j < TPT_MAX_DIMS; j++) w[j] = 0.f;
    if (tid < A.trials) {
        float nn = 0.f;
#pragma unroll
        for (int j = 0; j < TPT_MAX_DIMS; j++)
            if (j < T) {
                const uint32_t dr = tp_draw(A.seed, (uint32_t)sg.level, (uint32_t)sg.first,
                                            (uint32_t)tid, (uint32_t)j);
                w[j] = tp_sub(tp_div((float)dr, 5000.0f), 1.0f);
                nn = tp_add(nn, tp_mul(w[j], w[j]));
            }
        const float norm = tp_sqrt(nn);
        if (!(norm == 0.f)) {
#pragma unroll
            for (int j = 0; j < TPT_MAX_DIMS; j++)
                if (j < T) w[j] = tp_div(w[j], norm);
            float sum = 0.f;
            for (int i = 0; i < s; i++) sum = tp_add(sum, tp_dot(stage + i * T, w, T));
            const float mu = tp_div(sum, fs);
            float acc = 0.f;
            for (int i = 0; i < s; i++) {
                const float df = tp_sub(tp_dot(stage + i * T, w, T), mu);
                acc = tp_add(acc, tp_mul(df, df));
            }
            if (acc > axis_var) { tvar = acc; tmean = mu; tt = tid; }
        }
    }
    /* the largest variance, the earliest trial among equals: what keeping a
     * trial iff it is strictly above the best so far ends at */
    float bv = tvar;
    int bt = tt;
    tp_block_best(bv, bt, sv, sd);      /* its first barrier is behind the last read of stage */

    if (bt >= 0 ? tid == bt : tid == 0) {
        TptRule* R = A.rules + blockIdx.x;
#pragma unroll
        for (int j = 0; j < TPT_MAX_DIMS; j++) {
            R->idx[j] = idx[j];
            R->w[j] = bt >= 0 ? w[j] : (j == 0 ? 1.f : 0.f);
        }
        R->mean = bt >= 0 ? tmean : axis_mean;
    }
}

template <class VT>
__global__ __launch_bounds__(TP_THREADS)
void tpt_side_kernel(const VT* __restrict__ vectors, int32_t dim, TptArgs A)
{
    __shared__ int wl[TP_WAVES];
    const TptItem it = A.items[blockIdx.x];
    const TptRule* R = A.rules + it.seg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = min(A.topdims, dim);
    bool left = false;
    if (tid < it.count) {
        const int32_t m = A.cur[it.start + tid];
        float x[TPT_MAX_DIMS], w[TPT_MAX_DIMS];
#pragma unroll
        for (int j = 0; j < TPT_MAX_DIMS; j++) {
            x[j] = j < T ? tp_load(vectors, m, dim, R->idx[j]) : 0.f;
            w[j] = R->w[j];
        }
        left = tp_dot(x, w, T) < R->mean;
    }
    const uint64_t b = __ballot(left);
    int before = __popcll(b & ((1ull << lane) - 1));
    if (lane == 0) wl[wave] = __popcll(b);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int v = 0; v < TP_WAVES; v++) {
        if (v < wave) before += wl[v];
        total += wl[v];
    }
    if (tid < it.count) A.codes[it.start + tid] = (before << 1) | (left ? 1 : 0);
    if (tid == 0) A.item_left[blockIdx.x] = total;
}

__global__ __launch_bounds__(64)
void tpt_scan_kernel(TptArgs A)
{
    const TptSeg sg = A.segs[blockIdx.x];
    const int lane = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < sg.nitems; base += 64) {
        const int i = base + lane;
        const int x = i < sg.nitems ? A.item_left[sg.item0 + i] : 0;
        int inc = x;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        if (i < sg.nitems) A.item_base[sg.item0 + i] = carry + inc - x;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) A.seg_left[blockIdx.x] = carry;
}

__global__ __launch_bounds__(TP_THREADS)
void tpt_scatter_kernel(TptArgs A)
{
    const TptItem it = A.items[blockIdx.x];
    const TptSeg sg = A.segs[it.seg];
    const int tid = threadIdx.x;
    if (tid >= it.count) return;
    const int total = A.seg_left[it.seg], c = sg.count, p = it.pos0 + tid;
    const int code = A.codes[it.start + tid];
    const int lb = A.item_base[blockIdx.x] + (code >> 1);      /* lefts before p */
    const bool cut = total == 0 || total == c;                  /* by rank: order kept */
    const int nl = cut ? c / 2 : total;
    const bool left = cut ? p < nl : (code & 1) != 0;
    const int dest = cut ? p : left ? lb : nl + (p - lb);
    int32_t* out = (left ? nl : c - nl) <= A.leaf_size ? A.fin : A.next;
    out[sg.first + dest] = A.cur[it.start + tid];
}

/* ------------------------------------------------------------------ *
 * launchers
 * ------------------------------------------------------------------ */

int launch_exact(int vt, int dm, const DevIndex& di, const void* queries, int32_t nq,
                 int32_t k, int32_t nslices, int32_t rows_per_slice, int32_t* lists_v,
                 float* lists_d)
{
    /* the kernels index nothing outside these bounds */
    if (nq < 1 || k < 1 || k > MAX_K || nslices < 1 || nslices > MAX_SHARDS ||
        rows_per_slice < EXACT_ROW_ALIGN || rows_per_slice % EXACT_ROW_ALIGN != 0 ||
        (int64_t)nslices * rows_per_slice < di.n || di.dim < 1 ||
        (vt == VT_INT8 && di.dim > 4 * I_MAX_W))
        return (int)hipErrorInvalidValue;
    const dim3 grid((nq + XQT - 1) / XQT, nslices), block(XTHREADS);
    if (vt == VT_FLOAT) {
        const bool qres = f32_qstride(di.dim) <= FQRES_MAX;
        auto kernel = dm == DM_L2 ? (qres ? exact_f32_kernel<DM_L2, true>
                                          : exact_f32_kernel<DM_L2, false>)
                                  : (qres ? exact_f32_kernel<DM_COSINE, true>
                                          : exact_f32_kernel<DM_COSINE, false>);
        hipLaunchKernelGGL(kernel, grid, block, f32_lds(di.dim).total, nullptr, di,
                           (const float*)queries, nq, k, rows_per_slice, lists_v, lists_d);
    } else if (vt == VT_INT8) {
        auto kernel = dm == DM_L2 ? exact_i8_kernel<DM_L2> : exact_i8_kernel<DM_COSINE>;
        hipLaunchKernelGGL(kernel, grid, block, i8_lds(di.dim).total, nullptr, di,
                           (const int8_t*)queries, nq, k, rows_per_slice, lists_v, lists_d);
    } else {
        return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

/* the sorted selection's LDS at row stride `stride` */
static SrtLds group_sort_lds(int vt, int32_t dim, int stride)
{
    return vt == VT_FLOAT ? srt_lds(f32_lds(dim).thr, FRT, stride)
                          : srt_lds(i8_lds(dim).thr, IRT, stride);
}

int group_knn_sort_max(int vt, int32_t dim)
{
    if (dim < 1 || dim > MAX_DIM || (vt != VT_FLOAT && vt != VT_INT8) ||
        (vt == VT_INT8 && dim > 4 * I_MAX_W))
        return 0;
    for (int s = GK_SORT_CAP; s >= 64; s -= 64)
        if (group_sort_lds(vt, dim, s).total <= GK_LDS_MAX) return s;
    return 0;
}

/* one of the two grouped kernels over its part of the tile table */
template <bool SORTED>
static int launch_group_tiles(int vt, int dm, const void* vectors, int32_t dim,
                              const int32_t* members, const GroupTile* tiles, int32_t ntiles,
                              int32_t k, int stride, int32_t* out_v, float* out_d)
{
    const dim3 grid(ntiles), block(XTHREADS);
    const void* fn;
    uint32_t lds;
    if (vt == VT_FLOAT) {
        const bool qres = f32_qstride(dim) <= FQRES_MAX;
        auto kernel = dm == DM_L2 ? (qres ? group_f32_kernel<DM_L2, true, SORTED>
                                          : group_f32_kernel<DM_L2, false, SORTED>)
                                  : (qres ? group_f32_kernel<DM_COSINE, true, SORTED>
                                          : group_f32_kernel<DM_COSINE, false, SORTED>);
        fn = (const void*)kernel;
        lds = SORTED ? group_sort_lds(vt, dim, stride).total
                     : grp_lds(f32_lds(dim).total, FRT).total;
        if (SORTED && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds) != hipSuccess)
            return (int)hipGetLastError();
        hipLaunchKernelGGL(kernel, grid, block, lds, nullptr, (const float*)vectors, dim,
                           members, tiles, k, stride, out_v, out_d);
    } else {
        auto kernel = dm == DM_L2 ? group_i8_kernel<DM_L2, SORTED>
                                  : group_i8_kernel<DM_COSINE, SORTED>;
        fn = (const void*)kernel;
        lds = SORTED ? group_sort_lds(vt, dim, stride).total
                     : grp_lds(i8_lds(dim).total, IRT).total;
        if (SORTED && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds) != hipSuccess)
            return (int)hipGetLastError();
        hipLaunchKernelGGL(kernel, grid, block, lds, nullptr, (const int8_t*)vectors, dim,
                           members, tiles, k, stride, out_v, out_d);
    }
    return (int)hipGetLastError();
}

int launch_group_knn(int vt, int dm, const void* vectors, int32_t n, int32_t dim,
                     const int32_t* members, const GroupTile* tiles, int32_t nsorted,
                     int32_t sort_stride, int32_t nstream, int32_t k, int32_t* out_v,
                     float* out_d)
{
    /* the kernels index nothing outside these bounds */
    if (n < 1 || dim < 1 || k < 1 || k > MAX_K || nsorted < 0 || nstream < 0 ||
        (vt != VT_FLOAT && vt != VT_INT8) || (vt == VT_INT8 && dim > 4 * I_MAX_W) ||
        (nsorted > 0 && (sort_stride < 64 || sort_stride % 64 != 0 ||
                         sort_stride > group_knn_sort_max(vt, dim))))
        return (int)hipErrorInvalidValue;
    const size_t total = (size_t)n * k;
    const size_t fblocks = (total + 255) / 256;
    const unsigned fill = fblocks < 65536 ? (unsigned)fblocks : 65536u;   /* grid-stride */
    hipLaunchKernelGGL(group_fill_kernel, dim3(fill), dim3(256), 0, nullptr, out_v, out_d,
                       total);
    int err = (int)hipGetLastError();
    if (err == 0 && nsorted > 0)
        err = launch_group_tiles<true>(vt, dm, vectors, dim, members, tiles, nsorted, k,
                                       sort_stride, out_v, out_d);
    if (err == 0 && nstream > 0)
        err = launch_group_tiles<false>(vt, dm, vectors, dim, members, tiles + nsorted,
                                        nstream, k, 0, out_v, out_d);
    return err;
}

int launch_rng_prune(int vt, int dm, const void* vectors, int32_t dim, const int32_t* nodes,
                     int32_t nrows, const int32_t* cand_ids, const float* cand_dists,
                     int32_t ncand, int32_t degree, float rng_factor, int32_t fill_pruned,
                     int32_t* out)
{
    /* the kernels index nothing outside these bounds */
    if (nrows < 1 || dim < 1 || ncand < 1 || ncand > RP_MAX_C || degree < 1 ||
        degree > MAX_DEG || (vt != VT_FLOAT && vt != VT_INT8) ||
        (vt == VT_INT8 && dim > 4 * I_MAX_W))
        return (int)hipErrorInvalidValue;
    const dim3 grid(nrows);
    if (vt == VT_FLOAT) {
        const int nqt = degree > XQT ? 2 : 1;
        const bool res = rp_f32_resident(dim, nqt, ncand);
        const int qs = res ? f32_qstride(dim) : FQSS;
        const uint32_t lds =
            rp_lds((uint32_t)(nqt * XQT * qs), (uint32_t)(FRT * qs), ncand).total;
        auto pick = [&](auto k11, auto k12, auto k01, auto k02) {
            return res ? (nqt == 1 ? k11 : k12) : (nqt == 1 ? k01 : k02);
        };
        auto kernel = dm == DM_L2
            ? pick(rng_prune_f32_kernel<DM_L2, true, 1>, rng_prune_f32_kernel<DM_L2, true, 2>,
                   rng_prune_f32_kernel<DM_L2, false, 1>, rng_prune_f32_kernel<DM_L2, false, 2>)
            : pick(rng_prune_f32_kernel<DM_COSINE, true, 1>,
                   rng_prune_f32_kernel<DM_COSINE, true, 2>,
                   rng_prune_f32_kernel<DM_COSINE, false, 1>,
                   rng_prune_f32_kernel<DM_COSINE, false, 2>);
        hipLaunchKernelGGL(kernel, grid, dim3(XTHREADS), lds, nullptr, (const float*)vectors,
                           dim, nodes, cand_ids, cand_dists, ncand, degree, rng_factor,
                           fill_pruned, out);
    } else {
        const uint32_t wl = (uint32_t)((dim + 3) >> 2) | 1;
        auto kernel = dm == DM_L2 ? rng_prune_i8_kernel<DM_L2> : rng_prune_i8_kernel<DM_COSINE>;
        hipLaunchKernelGGL(kernel, grid, dim3(64), rp_lds(MAX_DEG * wl, RI_T * wl, ncand).total,
                           nullptr, (const int8_t*)vectors, dim, nodes, cand_ids, cand_dists,
                           ncand, degree, rng_factor, fill_pruned, out);
    }
    return (int)hipGetLastError();
}

int launch_pool_join(int vt, int dm, const void* vectors, int32_t dim, const int32_t* nodes,
                     int32_t nrows, const int32_t* pool_ids, const float* pool_dists,
                     int32_t npool, const int32_t* new_ids, const float* new_dists,
                     int32_t nnew, int32_t kout, int32_t* out_ids, float* out_dists)
{
    /* the kernels index nothing outside these bounds */
    if (nrows < 1 || npool < 0 || npool > PJ_MAX_L || nnew < 0 || nnew > PJ_MAX_L ||
        npool + nnew < 1 || kout < 1 || kout > PJ_MAX_L)
        return (int)hipErrorInvalidValue;
    const dim3 grid(nrows);
    if (new_dists) {
        /* lists and sorts only: one wave does a short row */
        const dim3 block(npool + nnew <= PJ_ONE_WAVE_MAX ? 64 : XTHREADS);
        hipLaunchKernelGGL(pool_join_given_kernel, grid, block,
                           pj_lds(npool, nnew, true, 0, 0).total, nullptr, nodes, pool_ids,
                           pool_dists, npool, new_ids, new_dists, nnew, kout, out_ids,
                           out_dists);
        return (int)hipGetLastError();
    }
    if (dim < 1 || dim > MAX_DIM || (vt != VT_FLOAT && vt != VT_INT8) ||
        (vt == VT_INT8 && dim > 4 * I_MAX_W))
        return (int)hipErrorInvalidValue;
    if (vt == VT_FLOAT) {
        const bool one = dim <= PJ_KS;
        auto kernel = dm == DM_L2 ? (one ? pool_join_f32_kernel<DM_L2, true>
                                         : pool_join_f32_kernel<DM_L2, false>)
                                  : (one ? pool_join_f32_kernel<DM_COSINE, true>
                                         : pool_join_f32_kernel<DM_COSINE, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(XTHREADS),
                           pj_lds(npool, nnew, false, (uint32_t)((dim + 3) & ~3),
                                  PJ_T * PJ_QS).total,
                           nullptr, (const float*)vectors, dim, nodes, pool_ids, pool_dists,
                           npool, new_ids, nnew, kout, out_ids, out_dists);
    } else {
        auto kernel = dm == DM_L2 ? pool_join_i8_kernel<DM_L2> : pool_join_i8_kernel<DM_COSINE>;
        hipLaunchKernelGGL(kernel, grid, dim3(XTHREADS), pj_lds(npool, nnew, false, 0, 0).total,
                           nullptr, (const int8_t*)vectors, dim, nodes, pool_ids, pool_dists,
                           npool, new_ids, nnew, kout, out_ids, out_dists);
    }
    return (int)hipGetLastError();
}

int kmeans_assign_tile(int vt) { return vt == VT_FLOAT ? (int)FRT : (int)KM_IT; }

int kmeans_assign_item_tiles(int vt, int64_t ntiles)
{
    const int64_t cap = KM_ITEM_MAX / kmeans_assign_tile(vt);
    const int64_t want = (ntiles + KM_ITEMS_TARGET - 1) / KM_ITEMS_TARGET;
    return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

int launch_kmeans_assign(int vt, int dm, const void* vectors, int32_t dim, const KmArgs& A)
{
    /* the kernels index nothing outside these bounds */
    if (A.nseg < 1 || A.nitems < 0 || A.kmax < 1 || A.kmax > KM_MAX_K || dim < 1 ||
        dim > MAX_DIM || (vt != VT_FLOAT && vt != VT_INT8) ||
        (vt == VT_INT8 && dim > 4 * I_MAX_W) || (A.update && !(A.out_sums && A.partials)) ||
        (A.lambdas != nullptr) != (A.prev_counts != nullptr))
        return (int)hipErrorInvalidValue;
    const size_t cells = (size_t)A.nseg * A.kmax;
    const size_t iblocks = (cells + 255) / 256;
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(iblocks < 65536 ? (unsigned)iblocks : 65536u),
                       dim3(256), 0, nullptr, A);
    const int nqt = A.kmax > XQT ? 2 : 1;
    if (A.nitems > 0 && vt == VT_FLOAT) {
        const bool res = km_f32_resident(dim, nqt, A.kmax, A.update);
        const KmLds L = km_f32_lds(dim, nqt, A.kmax, A.update, res);
        if (L.total > KM_LDS_MAX || (A.update && L.ss < 4)) return (int)hipErrorInvalidValue;
        auto pick = [&](auto k11, auto k12, auto k01, auto k02) {
            return res ? (nqt == 1 ? k11 : k12) : (nqt == 1 ? k01 : k02);
        };
        auto kernel = dm == DM_L2
            ? pick(kmeans_f32_kernel<DM_L2, true, 1>, kmeans_f32_kernel<DM_L2, true, 2>,
                   kmeans_f32_kernel<DM_L2, false, 1>, kmeans_f32_kernel<DM_L2, false, 2>)
            : pick(kmeans_f32_kernel<DM_COSINE, true, 1>, kmeans_f32_kernel<DM_COSINE, true, 2>,
                   kmeans_f32_kernel<DM_COSINE, false, 1>,
                   kmeans_f32_kernel<DM_COSINE, false, 2>);
        hipLaunchKernelGGL(kernel, dim3(A.nitems), dim3(XTHREADS), L.total, nullptr,
                           (const float*)vectors, dim, A);
    } else if (A.nitems > 0) {
        const KmLds L = km_i8_lds(dim, nqt, A.kmax, A.update);
        if (L.total > KM_LDS_MAX || (A.update && L.ss < 4)) return (int)hipErrorInvalidValue;
        auto kernel = dm == DM_L2
            ? (nqt == 1 ? kmeans_i8_kernel<DM_L2, 1> : kmeans_i8_kernel<DM_L2, 2>)
            : (nqt == 1 ? kmeans_i8_kernel<DM_COSINE, 1> : kmeans_i8_kernel<DM_COSINE, 2>);
        hipLaunchKernelGGL(kernel, dim3(A.nitems), dim3(128 * nqt), L.total, nullptr,
                           (const int8_t*)vectors, dim, A);
    }
    const dim3 fgrid(A.nseg, A.update ? ((unsigned)A.kmax * dim + 255) / 256 : 1);
    if (vt == VT_INT8)
        hipLaunchKernelGGL(kmeans_finish_kernel<true>, fgrid, dim3(256), 0, nullptr, A, dim);
    else
        hipLaunchKernelGGL(kmeans_finish_kernel<false>, fgrid, dim3(256), 0, nullptr, A, dim);
    return (int)hipGetLastError();
}

int launch_tpt_level(int vt, const void* vectors, int32_t dim, const TptArgs& A)
{
    /* the kernels index nothing outside these bounds */
    if (A.nseg < 1 || A.nitems < 1 || A.leaf_size < 1 || A.samples < 1 ||
        A.samples > TPT_MAX_SAMPLES || A.topdims < 1 || A.topdims > TPT_MAX_DIMS ||
        A.trials < 0 || A.trials > TPT_MAX_TRIALS || dim < 1 || dim > MAX_DIM ||
        (vt != VT_FLOAT && vt != VT_INT8) || A.cur == A.next || A.cur == A.fin ||
        A.next == A.fin)
        return (int)hipErrorInvalidValue;
    const size_t T = (size_t)std::min(A.topdims, dim);
    const size_t lds = std::max<size_t>(TP_SCRATCH + 8 * (size_t)dim, 4 * A.samples * T);
    if (lds > TP_LDS_MAX) return (int)hipErrorInvalidValue;
    if (vt == VT_FLOAT) {
        hipLaunchKernelGGL(tpt_rule_kernel<float>, dim3(A.nseg), dim3(TP_THREADS), lds, nullptr,
                           (const float*)vectors, dim, A);
        hipLaunchKernelGGL(tpt_side_kernel<float>, dim3(A.nitems), dim3(TP_THREADS), 0, nullptr,
                           (const float*)vectors, dim, A);
    } else {
        hipLaunchKernelGGL(tpt_rule_kernel<int8_t>, dim3(A.nseg), dim3(TP_THREADS), lds, nullptr,
                           (const int8_t*)vectors, dim, A);
        hipLaunchKernelGGL(tpt_side_kernel<int8_t>, dim3(A.nitems), dim3(TP_THREADS), 0, nullptr,
                           (const int8_t*)vectors, dim, A);
    }
    hipLaunchKernelGGL(tpt_scan_kernel, dim3(A.nseg), dim3(64), 0, nullptr, A);
    hipLaunchKernelGGL(tpt_scatter_kernel, dim3(A.nitems), dim3(TP_THREADS), 0, nullptr, A);
    return (int)hipGetLastError();
}

}  /* namespace sptag_amd */
