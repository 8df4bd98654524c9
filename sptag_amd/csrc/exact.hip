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
    int32_t* lv;     /* this (slice, query tile)'s lists, query ql at ql*k */
    float* ld;
    int k;
    int nql;         /* queries of the tile that exist */
};

/* (da, va) ordered before (db, vb); vids are distinct, so this is total */
DEV bool key_before(float da, int32_t va, float db, int32_t vb)
{
    return da < db || (da == db && va < vb);
}

DEV float wave_bcast(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
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
        int32_t* lv = s.lv + (size_t)ql * s.k;
        float* ld = s.ld + (size_t)ql * s.k;
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
    for (int ql = wave; ql < s.nql; ql += XWAVES)
        for (int i = lane; i < s.k; i += 64) {
            s.lv[(size_t)ql * s.k + i] = -1;
            s.ld[(size_t)ql * s.k + i] = MAXDIST;
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
    const int nks = (d + 31) >> 5;
    for (int t = 0; t < ntile; t++) {
        const int tr0 = r0 + t * IRT;
        if (t + 1 < ntile) stage_load(tr0 + IRT);   /* in flight while this tile computes */

        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int bb = 0;
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
 * launcher
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

}  /* namespace sptag_amd */
