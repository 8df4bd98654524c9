/* sptag_amd — C-ABI boundary of the MI355X-native SPTAG search backend.
 *
 * This is the drop-in seam: a host (C++, Python, or any FFI) that today
 * drives the reference SPTAG through VectorIndex can route the in-memory
 * BKT hot path through these entry points instead. Each entry point cites
 * the reference interface it replaces (paths relative to
 * /root/reference/AnnService):
 *
 *   sptag_amd_load_index    <- VectorIndex::LoadIndex(folder)
 *                              (inc/Core/VectorIndex.h:157, src/Core/
 *                              VectorIndex.cpp:618): same folder layout,
 *                              indexloader.ini + vectors/tree/graph/deletes.
 *   sptag_amd_create_index  <- BKT::Index<T>::LoadIndexDataFromMemory /
 *                              the blob form of LoadIndexData
 *                              (src/Core/BKT/BKTIndex.cpp:86).
 *   sptag_amd_search_batch  <- the batch overload
 *                              VectorIndex::SearchIndex(const void* p_vectors,
 *                              int p_vectorNum, int p_neighborCount, bool
 *                              p_withMeta, BasicResult* p_results)
 *                              (inc/Core/VectorIndex.h:103, src/Core/
 *                              VectorIndex.cpp:455): contiguous queries in,
 *                              per-query top-k (vid,dist) out, ascending by
 *                              (dist, vid), vid=-1 padding — identical result
 *                              contract, with (vid,dist) in two flat arrays
 *                              instead of BasicResult structs so no C++ types
 *                              cross the ABI.
 *   sptag_amd_save_index    <- VectorIndex::SaveIndex(folder)
 *                              (inc/Core/VectorIndex.h:87): writes the same
 *                              byte format the reference loads.
 *   sptag_amd_shards_*      <- AggregatorService::AggregateResults
 *                              (src/Aggregator/AggregatorService.cpp:363):
 *                              per-shard lists concatenated, top k selected;
 *                              here inside one process, merged on the GPU.
 *
 * All device state lives behind the opaque handle. Errors are negative int
 * codes; no exceptions cross this boundary. Thread-safety: search is
 * internally batched; concurrent callers on one handle are serialized by an
 * internal lock (the reference allows concurrent SearchIndex callers —
 * SURVEY.md §8b).
 *
 * THE GPU IS THE PRODUCT PATH: every search entry fails loudly (returns
 * SPTAG_AMD_ERR_NOGPU) when no HIP device is present. There is no CPU
 * fallback anywhere behind this ABI.
 */
#ifndef SPTAG_AMD_H
#define SPTAG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* value types — subset of reference VectorValueType the hot path covers */
#define SPTAG_AMD_VT_FLOAT 0
#define SPTAG_AMD_VT_INT8  1
/* distance methods — reference DistCalcMethod */
#define SPTAG_AMD_DM_L2     0
#define SPTAG_AMD_DM_COSINE 1

#define SPTAG_AMD_OK            0
#define SPTAG_AMD_ERR_IO       -1   /* missing/corrupt index files */
#define SPTAG_AMD_ERR_PARAM    -2   /* bad argument */
#define SPTAG_AMD_ERR_NOGPU    -3   /* no HIP device / HIP runtime failure */
#define SPTAG_AMD_ERR_UNSUPP   -4   /* index feature outside the hot path */
#define SPTAG_AMD_ERR_OOM      -5
#define SPTAG_AMD_ERR_INTERNAL -6

typedef struct SptagAmdIndex SptagAmdIndex;

/* Load a reference-format index folder onto GPU `device`. */
SptagAmdIndex* sptag_amd_load_index(const char* folder, int device);

/* Assemble an index from raw blobs (layouts as in the files, no headers);
 * copies to device. tree_nodes: int32 triples {centerid,childStart,childEnd}. */
SptagAmdIndex* sptag_amd_create_index(int32_t n, int32_t dim, int valuetype,
                                      int distmethod, const void* vectors,
                                      int32_t ntrees, const int32_t* tree_start,
                                      int32_t n_tree_nodes, const int32_t* tree_nodes,
                                      int32_t degree, const int32_t* graph,
                                      const uint8_t* deleted /* NULL = none */,
                                      int device);

/* KDT variant of create (reference inc/Core/Common/KDTree.h:22 KDTNode
 * {left,right,split_dim,split_value}; kdt_nodes = 16-byte records). */
SptagAmdIndex* sptag_amd_create_index_kdt(int32_t n, int32_t dim, int valuetype,
                                          int distmethod, const void* vectors,
                                          int32_t ntrees, const int32_t* tree_start,
                                          int32_t n_tree_nodes, const void* kdt_nodes,
                                          int32_t degree, const int32_t* graph,
                                          const uint8_t* deleted, int device);

void sptag_amd_free_index(SptagAmdIndex* idx);

/* Batched search. queries: nq contiguous vectors of the index's dtype/dim.
 * out_vids/out_dists: nq*k, ascending (dist, vid), vid=-1 padding.
 * max_check <= 0 uses the index's MaxCheck (ini value or 8192 default).
 * Returns SPTAG_AMD_OK or a negative error. */
int sptag_amd_search_batch(SptagAmdIndex* idx, const void* queries, int32_t nq,
                           int32_t k, int32_t max_check,
                           int32_t* out_vids, float* out_dists);

/* Device-pointer variant: queries/outputs are HIP device buffers already
 * resident in HBM (e.g. torch tensors' data_ptr); no host<->device copies
 * inside the timed path. Same contract otherwise. */
int sptag_amd_search_batch_device(SptagAmdIndex* idx, const void* d_queries,
                                  int32_t nq, int32_t k, int32_t max_check,
                                  int32_t* d_out_vids, float* d_out_dists);

/* Instrumentation of the LAST search call on this handle: accumulated HIP
 * kernel time (events around each search launch, on the launch stream) and
 * the traversal totals across all queries (checked = distance evaluations,
 * popped = frontier pops) — the inputs to the roofline's algorithmic-bytes
 * numerator. */
void sptag_amd_last_stats(SptagAmdIndex* idx, double* kernel_ms,
                          long long* checked, long long* popped);

/* Exact brute-force top-k on the GPU (truth generation / recall gates;
 * reference TruthSet::GenerateTruth semantics, inc/Core/Common/TruthSet.h:163). */
int sptag_amd_truth(SptagAmdIndex* idx, const void* queries, int32_t nq,
                    int32_t k, int32_t* out_vids, float* out_dists);

/* Exact search: sptag_amd_truth's answer, bit for bit (non-deleted rows,
 * ascending (dist, vid), vid = -1 at MaxDist as padding, any k <= 1024),
 * computed by the tiled kernels of exact.hip: a row read from HBM serves a
 * tile of queries, int8 dots run on the matrix units, and the rows are cut
 * into slices so that a small batch still fills the device. The tree and
 * graph are not used. The _device form takes HIP device buffers, as
 * sptag_amd_search_batch_device does. SPTAG_AMD_EXACT_SLICES=<1..64> in the
 * environment overrides the number of slices (never the result). */
int sptag_amd_exact_search(SptagAmdIndex* idx, const void* queries, int32_t nq,
                           int32_t k, int32_t* out_vids, float* out_dists);
int sptag_amd_exact_search_device(SptagAmdIndex* idx, const void* d_queries,
                                  int32_t nq, int32_t k, int32_t* d_out_vids,
                                  float* d_out_dists);

/* Grouped exact kNN: all-pairs top-k inside row groups (the index builder's
 * leaf step). Group g is members[starts[g] : starts[g] + counts[g]], vector
 * ids in any order; no id occurs twice and an id may be in no group. Row v
 * of out_vids/out_dists ([n][k], n the handle's row count) receives the k
 * smallest (dist, vid) over the OTHER members of v's group: ascending (dist,
 * vid), distances exactly those of the search paths for the handle's value
 * type and metric, vid = -1 at MaxDist as padding behind the real entries.
 * Only v itself is left out, by id: another id with an identical vector is a
 * neighbour at its distance. The row of an id that is in no group, or alone
 * in its group, is all padding; every row is written. The delete set, the
 * tree and the graph are not consulted (BKT and KDT handles alike): the
 * caller decides what is a member. Any 1 <= k <= 1024 and any group size,
 * up to one group of all n rows. Computed by the grouped tiles of exact.hip:
 * a workgroup owns 32 members of a group as queries and streams the group.
 * Returns SPTAG_AMD_ERR_PARAM, with the outputs untouched, for a null
 * pointer, k outside [1, 1024], ngroups < 1, a negative start or count, a
 * group that ends past nmembers, two groups that overlap, a member outside
 * [0, n) and an id that occurs twice in members. */
int sptag_amd_group_knn(SptagAmdIndex* idx, const int32_t* members, int32_t nmembers,
                        const int32_t* starts, const int32_t* counts, int32_t ngroups,
                        int32_t k, int32_t* out_vids, float* out_dists);
/* The same without a handle: d_vectors ([n][dim] of valuetype), d_members
 * and the outputs are HIP device buffers on `device`; starts and counts stay
 * host arrays (one entry per group). It checks what the host can see (the
 * pointers, k, the ranges of starts/counts, value type, metric, 1 <= dim <=
 * 4096, the int8 dim guard of the create calls) and returns
 * SPTAG_AMD_ERR_PARAM for those. That every member is inside [0, n) and
 * occurs once is the CALLER'S to guarantee: a member outside [0, n) makes
 * the kernels read outside d_vectors. Runs on the default stream and returns
 * after a device synchronise, as sptag_amd_exact_search_device does. */
int sptag_amd_group_knn_device(int device, const void* d_vectors, int valuetype,
                               int distmethod, int32_t n, int32_t dim,
                               const int32_t* d_members, int32_t nmembers,
                               const int32_t* starts, const int32_t* counts,
                               int32_t ngroups, int32_t k, int32_t* d_out_vids,
                               float* d_out_dists);

/* Grouped exact kNN with a choice of selection. The result is that of
 * sptag_amd_group_knn[_device] in every byte, whatever the selection; the
 * arguments are theirs, with `selection` before k, and so are the checks.
 *   SPTAG_AMD_GK_STREAM  the two calls above: rows stream past a threshold
 *                        and survivors are merged into the list 32 at a
 *                        time. Made for few survivors (exact search's shape).
 *   SPTAG_AMD_GK_SORT    every distance of a query to its group goes into a
 *                        row of an LDS matrix; one wave then radix-selects
 *                        the k-th (dist, vid), compacts the survivors and
 *                        sorts them once. Made for leaf-sized groups, where k
 *                        is a sizeable part of the group. Groups of at most
 *                        sptag_amd_group_knn_sort_max(valuetype, dim)
 *                        members; SPTAG_AMD_ERR_PARAM, outputs untouched, if
 *                        any group is larger.
 *   SPTAG_AMD_GK_AUTO    per group, the selection that was measured faster
 *                        for its size and k; larger groups
 *                        stream, in the same call. Never fails for size.
 * Any other selection is SPTAG_AMD_ERR_PARAM. */
#define SPTAG_AMD_GK_STREAM 0
#define SPTAG_AMD_GK_SORT 1
#define SPTAG_AMD_GK_AUTO 2
int sptag_amd_group_knn_sel(SptagAmdIndex* idx, const int32_t* members, int32_t nmembers,
                            const int32_t* starts, const int32_t* counts, int32_t ngroups,
                            int32_t selection, int32_t k, int32_t* out_vids,
                            float* out_dists);
int sptag_amd_group_knn_sel_device(int device, const void* d_vectors, int valuetype,
                                   int distmethod, int32_t n, int32_t dim,
                                   const int32_t* d_members, int32_t nmembers,
                                   const int32_t* starts, const int32_t* counts,
                                   int32_t ngroups, int32_t selection, int32_t k,
                                   int32_t* d_out_vids, float* d_out_dists);
/* The largest group SPTAG_AMD_GK_SORT takes for a value type and dim: what
 * 160 KiB of LDS leave for a 32-query distance matrix beside the distance
 * tiles, a multiple of 64, at most 1024 (1024 at f32 dim 128 and int8 dim
 * 100). 0 for a value type or dim that the grouped calls reject. */
int32_t sptag_amd_group_knn_sort_max(int valuetype, int32_t dim);

/* RNG prune: the reference's RebuildNeighbors rule
 * (RelativeNeighborhoodGraph.h:18-35) over caller-supplied candidate lists,
 * the step that ends every graph stage of the index builder. Row r has a node
 * id nodes[r] and the list cand_ids[r][0..ncand) with cand_dists[r][0..ncand),
 * given in ascending distance and never recomputed. The list is walked in
 * order while fewer than `degree` candidates are accepted:
 *   - a candidate whose id is < 0 or equals nodes[r], or whose distance is
 *     not finite, is skipped;
 *   - candidate c is rejected if some already accepted a has
 *     rng_factor * dist(a, c) < cand_dists[c] (an f32 product, strict <);
 *   - otherwise it is accepted.
 * dist is the search paths' distance for the value type and metric, bit for
 * bit: f32 in the reference's 16/8/4-accumulator order (1 - dot for cosine),
 * int8 exact integers (16129 - dot for cosine). Ids are not deduplicated: the
 * rule decides a repeated id. out_graph[r][0..degree) receives the accepted
 * ids in list order, then -1. With fill_pruned != 0 a row that ends short of
 * `degree` also keeps its degree - count nearest valid rejected candidates,
 * and every kept id, accepted or filled, is written in list order.
 * 1 <= ncand <= 1024, 1 <= degree <= 64, any nrows >= 1. The handle form
 * takes host arrays and uses the handle's vectors, value type and metric; the
 * delete set, the tree and the graph are not consulted (BKT and KDT handles
 * alike). Computed by the prune kernels of exact.hip: a workgroup owns a row,
 * keeps the accepted vectors in LDS and streams the list in tiles, each
 * candidate vector read once. Returns SPTAG_AMD_ERR_PARAM, with the output
 * untouched, for a null pointer, nrows < 1, ncand or degree out of range, an
 * rng_factor that is not finite and positive, a node outside [0, n) and a
 * candidate id >= n. */
int sptag_amd_rng_prune(SptagAmdIndex* idx, const int32_t* nodes, int32_t nrows,
                        const int32_t* cand_ids, const float* cand_dists, int32_t ncand,
                        int32_t degree, float rng_factor, int32_t fill_pruned,
                        int32_t* out_graph);
/* The same without a handle: d_vectors ([n][dim] of valuetype), d_nodes, the
 * lists and the output are HIP device buffers on `device`. It checks what the
 * host can see (the pointers, nrows, ncand, degree, rng_factor, value type,
 * metric, 1 <= dim <= 4096, the int8 dim guard of the create calls) and
 * returns SPTAG_AMD_ERR_PARAM for those. That every node and every candidate
 * id >= 0 is inside [0, n) is the CALLER'S to guarantee: an id outside makes
 * the kernels read outside d_vectors. Runs on the default stream and returns
 * after a device synchronise. */
int sptag_amd_rng_prune_device(int device, const void* d_vectors, int valuetype,
                               int distmethod, int32_t n, int32_t dim,
                               const int32_t* d_nodes, int32_t nrows,
                               const int32_t* d_cand_ids, const float* d_cand_dists,
                               int32_t ncand, int32_t degree, float rng_factor,
                               int32_t fill_pruned, int32_t* d_out_graph);

/* Pool join: grow candidate pools, the index builder's step between the leaf
 * kNN and the RNG prune. Row r has a node id nodes[r] (its query is that
 * vector), an old pool pool_ids[r][0..npool) with pool_dists[r][0..npool),
 * used as given and never recomputed, and new candidates new_ids[r][0..nnew).
 * With new_dists null the distance of every new candidate to the node's
 * vector is computed: the search paths' distance for the value type and
 * metric, bit for bit (f32 in the reference's 16/8/4-accumulator order, 1 -
 * dot for cosine; int8 exact integers, 16129 - dot for cosine). With
 * new_dists given those values are used and no vector is read.
 *   - An entry is invalid if its id is < 0 or equals nodes[r], or its given
 *     distance is not finite. A given -0.0 counts as 0.0.
 *   - A new candidate whose id is a valid entry of the old pool is dropped:
 *     the pool's entry and distance stand, and no vector is read for it.
 *   - Of several valid entries of one id inside the old pool, or inside the
 *     new list, the smallest (dist, position) stays.
 * out_ids[r][0..kout) / out_dists[r][0..kout) receive the kout smallest
 * remaining entries in ascending (dist, id), distances compared as f32
 * numbers (cosine ones may be negative), ids as int32; all ids are distinct.
 * Behind them comes padding of id -1 at +inf, so an output is a valid old pool
 * of a later call. A row is read completely before it is written: the device
 * form's outputs may be the old pool's own buffers when kout == npool.
 * 0 <= npool <= 1024, 0 <= nnew <= 1024, npool + nnew >= 1, 1 <= kout <= 1024,
 * any nrows >= 1; pool_ids and pool_dists may be null at npool == 0. The
 * handle form takes host arrays and uses the handle's vectors, value type and
 * metric; the delete set, the tree and the graph are not consulted (BKT and
 * KDT handles alike). Computed by the pool-join kernels of exact.hip: a
 * workgroup owns a row, settles validity and duplicates in LDS before any
 * distance, reads each surviving new vector once and sorts packed (dist, id)
 * keys. Returns SPTAG_AMD_ERR_PARAM, with the outputs untouched, for a null
 * required pointer, nrows < 1, a size out of range or both sizes zero, a null
 * pool pointer with npool > 0, a node outside [0, n) and an id >= n. */
int sptag_amd_pool_join(SptagAmdIndex* idx, const int32_t* nodes, int32_t nrows,
                        const int32_t* pool_ids, const float* pool_dists, int32_t npool,
                        const int32_t* new_ids, const float* new_dists, int32_t nnew,
                        int32_t kout, int32_t* out_ids, float* out_dists);
/* The same without a handle: d_vectors ([n][dim] of valuetype), d_nodes, the
 * lists and the outputs are HIP device buffers on `device`. It checks what the
 * host can see (the pointers, nrows, the sizes, value type, metric, 1 <= dim
 * <= 4096, the int8 dim guard of the create calls) and returns
 * SPTAG_AMD_ERR_PARAM for those. That every node and every id >= 0 is inside
 * [0, n) is the CALLER'S to guarantee: with d_new_dists null an id outside
 * makes the kernels read outside d_vectors. Runs on the default stream and
 * returns after a device synchronise. */
int sptag_amd_pool_join_device(int device, const void* d_vectors, int valuetype,
                               int distmethod, int32_t n, int32_t dim,
                               const int32_t* d_nodes, int32_t nrows,
                               const int32_t* d_pool_ids, const float* d_pool_dists,
                               int32_t npool, const int32_t* d_new_ids,
                               const float* d_new_dists, int32_t nnew, int32_t kout,
                               int32_t* d_out_ids, float* d_out_dists);

/* K-means assign: one KmeansAssign pass (the reference's BKTree.h:220-311)
 * over many independent segments, the index builder's tree step. Segment s is
 * members[seg_starts[s] .. + seg_sizes[s]) (vector ids; an id may occur twice,
 * in one segment or in several; a size of 0 is allowed; segments do not
 * overlap) with centers centers[s][0..ncenters[s]) of centers[nseg][kmax][dim],
 * which have the value type of the vectors; rows at or past ncenters[s] are
 * never read. 1 <= ncenters[s] <= kmax, 1 <= kmax <= 64. prev_counts
 * [nseg][kmax] and lambdas [nseg] are both given or both null (no penalty).
 * The member at position i of segment s, with vector x:
 *   - For k = 0 .. ncenters[s] - 1 in order, dist_k = D(x, center_k) +
 *     lambdas[s] * (float)prev_counts[s][k]. D is the search paths' distance
 *     for the value type and metric, bit for bit (f32 in the reference's
 *     16/8/4-accumulator order, 1 - dot for cosine; int8 exact integers, 16129
 *     - dot for cosine); the penalty is an f32 product rounded once, then an
 *     f32 sum rounded once, never fused; with lambdas null nothing is added.
 *   - Center k replaces the choice iff dist_k > -MaxDist && dist_k < smallest,
 *     from (label 0, smallest = MaxDist), MaxDist = FLT_MAX / 10: ties go to
 *     the lowest k, a NaN or a value at or above MaxDist is never chosen, and a
 *     member no center qualifies for ends at label 0 with distance MaxDist.
 * out_labels[nmembers] / out_dists[nmembers] (may be null) receive the choice
 * and its `smallest` at the member's place in the list; places in no segment
 * are untouched. Per segment and center below ncenters[s] (entries at or past
 * it are untouched): out_counts[nseg][kmax], the members of the center;
 * out_cluster_idx / out_cluster_dist, one extreme member as a vector id with
 * its `smallest`: with update == 1 the member of largest `smallest`, ties to
 * the smallest position, with update == 0 the member of smallest `smallest`,
 * ties to the largest position (the reference's > and <= over ascending
 * positions); an empty center gets -1 with -MaxDist (update 1) or MaxDist.
 * out_sums[nseg][kmax][dim] (f32) is written with update == 1 only and may be
 * null otherwise: the sum of the center's members' vectors, int8 as integers
 * rounded to f32 once, f32 in an order that is the kernel's but fixed, so
 * equal calls give equal bytes; all zeros for an empty center. Dividing and
 * casting the sums into the next centers stays with the caller.
 * The handle form takes host arrays and uses the handle's vectors, value type
 * and metric; the delete set, the tree and the graph are not consulted (BKT
 * and KDT handles alike). Computed by the k-means-assign kernels of
 * exact.hip: a workgroup owns a run of one segment's members, keeps the
 * centers in LDS, reads each vector once for distance and sum where LDS
 * allows, and leaves counts and extremes by integer atomics and sums as
 * partials that a second kernel adds in list order. Returns
 * SPTAG_AMD_ERR_PARAM, with the outputs untouched, for a null required
 * pointer, kmax or an ncenters[s] out of range, nseg < 1, a negative start or
 * size, a segment past nmembers, overlapping segments, one of prev_counts /
 * lambdas without the other, update not 0 or 1, update == 1 with null sums,
 * and a member outside [0, n). */
int sptag_amd_kmeans_assign(SptagAmdIndex* idx, const int32_t* members, int32_t nmembers,
                            const int32_t* seg_starts, const int32_t* seg_sizes,
                            const int32_t* ncenters, int32_t nseg, const void* centers,
                            int32_t kmax, const int32_t* prev_counts, const float* lambdas,
                            int32_t update, int32_t* out_labels, float* out_dists,
                            int32_t* out_counts, int32_t* out_cluster_idx,
                            float* out_cluster_dist, float* out_sums);
/* The same without a handle: d_vectors ([n][dim] of valuetype), d_members,
 * d_centers, d_prev_counts, d_lambdas and the outputs are HIP device buffers
 * on `device`; seg_starts, seg_sizes and ncenters are host arrays. It checks
 * what the host can see (the pointers, the segments, kmax and ncenters, value
 * type, metric, 1 <= dim <= 4096, the int8 dim guard of the create calls) and
 * returns SPTAG_AMD_ERR_PARAM for those. That every member is inside [0, n)
 * is the CALLER'S to guarantee: an id outside makes the kernels read outside
 * d_vectors. Runs on the default stream and returns after a device
 * synchronise. */
int sptag_amd_kmeans_assign_device(int device, const void* d_vectors, int valuetype,
                                   int distmethod, int32_t n, int32_t dim,
                                   const int32_t* d_members, int32_t nmembers,
                                   const int32_t* seg_starts, const int32_t* seg_sizes,
                                   const int32_t* ncenters, int32_t nseg,
                                   const void* d_centers, int32_t kmax,
                                   const int32_t* d_prev_counts, const float* d_lambdas,
                                   int32_t update, int32_t* d_out_labels, float* d_out_dists,
                                   int32_t* d_out_counts, int32_t* d_out_cluster_idx,
                                   float* d_out_cluster_dist, float* d_out_sums);

/* TP-tree partition: the reference's hyperplane splits (PartitionByTptreeCore,
 * NeighborhoodGraph.h:152-299) of a member list (vector ids) into leaves, the
 * step of the index builder that makes the leaves of the kNN candidates. The
 * list is split level by level, the root being level 0; a segment is
 * members[first .. first + c). A segment with c <= leaf_size is a leaf (the
 * reference tests last - first <= leaf, one member more; this is the
 * builder's own test). A longer one splits as follows, where a coordinate
 * enters as (float)v[k], every operation is f32 and rounded once, none is
 * fused, and sums run from 0 in the stated order:
 *   1. s = min(samples, c); the sample is the first s members in list order,
 *      v_0 .. v_{s-1}.
 *   2. Mean[k] = (v_0[k] + v_1[k] + ..) / (float)s; Var[k] = the sum over i in
 *      order of (v_i[k] - Mean[k])^2.
 *   3. T = min(topdims, dim); idx_0 .. idx_{T-1} are the dimensions of largest
 *      Var, ties to the lower dimension, a NaN below every number.
 *   4. The best rule starts as weights (1, 0, .., 0), bestvar = Var[idx_0],
 *      bestmean = Mean[idx_0].
 *   5. For trial t = 0 .. trials - 1 in order: w_j = (float)draw(t, j) /
 *      5000.0f - 1.0f; norm = sqrt(w_0*w_0 + w_1*w_1 + ..) in order; the trial
 *      is skipped if norm == 0, else w_j = w_j / norm. Val_i = w_0*v_i[idx_0]
 *      + w_1*v_i[idx_1] + .., in order of j; mean = (Val_0 + Val_1 + ..) /
 *      (float)s; var = the sum over i of (Val_i - mean)^2. The trial replaces
 *      the best rule iff var > bestvar: the earliest of equals wins, and the
 *      axis rule stays unless strictly beaten.
 *      draw(t, j), in uint64 wrapping arithmetic: key = (((((uint64)level <<
 *      31) | first) << 8 | t) << 3) | j; z = seed + 0x9E3779B97F4A7C15 * (1 +
 *      key); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *      0x94D049BB133111EB; z ^= z >> 31; draw = (z >> 32) % 10000. (The
 *      reference draws from rand() after srand(clock()).)
 *   6. Each of the c members goes left iff bw_0*v[idx_0] + .. < bestmean, the
 *      sum as in 5. The split is a STABLE partition: lefts in list order, then
 *      rights in list order (the reference swaps from both ends, and is not).
 *      If one side is empty the segment is cut at c / 2 (floor) with the list
 *      order kept, the reference's rule for equal points.
 * out_members is a permutation of members; out_leaf_starts / out_leaf_counts
 * are in ascending start order and tile [0, nmembers) with no gap and no empty
 * leaf; *out_nleaves is their number. If max_leaves is too small the call
 * returns SPTAG_AMD_ERR_PARAM with the needed number in *out_nleaves and every
 * other output untouched. Equal calls give equal bytes. nmembers >= 1,
 * leaf_size >= 1, 1 <= samples <= 2048, 1 <= topdims <= 8, 0 <= trials <= 256
 * (trials 0 with topdims 1: a kd-style split of the widest axis at its mean).
 * The handle form takes host arrays and uses the handle's vectors and value
 * type; the metric, the delete set, the tree and the graph are not consulted
 * (BKT and KDT handles alike). Computed by the TP-tree kernels of exact.hip: a
 * workgroup settles a segment's rule from the sample, the sides are ranked by
 * ballots and a scan of per-item counts, and the host reads only a left count
 * per segment and level. Returns SPTAG_AMD_ERR_PARAM, with the outputs
 * untouched, for a null pointer, a value outside the limits, max_leaves < 0
 * and a member outside [0, n). */
int sptag_amd_tpt_partition(SptagAmdIndex* idx, const int32_t* members, int32_t nmembers,
                            int32_t leaf_size, int32_t samples, int32_t topdims, int32_t trials,
                            uint64_t seed, int32_t* out_members, int32_t* out_leaf_starts,
                            int32_t* out_leaf_counts, int32_t max_leaves, int32_t* out_nleaves);
/* The same without a handle: d_vectors ([n][dim] of valuetype, f32 or int8),
 * d_members and d_out_members (which may be d_members) are HIP device buffers
 * on `device`; the leaf table and out_nleaves are host memory. There is no
 * metric: the rule reads coordinates only. It checks what the host can see
 * (the pointers, the limits, value type, 1 <= dim <= 4096, the int8 dim guard
 * of the create calls) and returns SPTAG_AMD_ERR_PARAM for those. That every
 * member is inside [0, n) is the CALLER'S to guarantee: an id outside makes
 * the kernels read outside d_vectors. Runs on the default stream and returns
 * after a device synchronise. */
int sptag_amd_tpt_partition_device(int device, const void* d_vectors, int valuetype, int32_t n,
                                   int32_t dim, const int32_t* d_members, int32_t nmembers,
                                   int32_t leaf_size, int32_t samples, int32_t topdims,
                                   int32_t trials, uint64_t seed, int32_t* d_out_members,
                                   int32_t* out_leaf_starts, int32_t* out_leaf_counts,
                                   int32_t max_leaves, int32_t* out_nleaves);

/* Iterative (streaming) search — mirrors the reference's ResultIterator /
 * SearchIndexIterativeNext protocol (inc/Core/VectorIndex.h:43-49,
 * src/Core/ResultIterator.cpp) over a BATCH of nq per-query iterators whose
 * traversal state persists on the device between calls. Each next() call
 * returns up to `batch` further results per query, sorted, with the
 * per-query result count and the sticky relaxed-monotonicity flag. */
typedef struct SptagAmdIterBatch SptagAmdIterBatch;
SptagAmdIterBatch* sptag_amd_iter_create(SptagAmdIndex* idx, const void* queries,
                                         int32_t nq, int32_t max_check);
/* A count below `batch` means that query's iterator is exhausted, and only
 * that. The per-query visited table is fixed at create time
 * (next_pow2(max(4096, 4*max_check)) slots) while the reference's grows on
 * demand and its iterator runs on past MaxCheck. On the call in which any
 * query's table saturates, and on every later call of that batch, next()
 * prints a line naming visited-table saturation to stderr and returns
 * SPTAG_AMD_ERR_INTERNAL with the outputs untouched; every earlier call is
 * exact. The table is not grown or re-sized. */
int sptag_amd_iter_next(SptagAmdIterBatch* it, int32_t batch,
                        int32_t* out_vids, float* out_dists,
                        int32_t* out_counts, int32_t* out_relaxed);
void sptag_amd_iter_free(SptagAmdIterBatch* it);

/* Online add — mirrors BKT AddIndex below the tree-rebuild threshold
 * (src/Core/BKT/BKTIndex.cpp:902-970): appends the vectors, then per new
 * node a GPU refine search (AddCEF=500, MaxCheckForRefineGraph) followed by
 * the reference's RNG rebuild + two-way neighbor inserts. Requires a HIP
 * device (the refine searches run on it). */
int sptag_amd_add(SptagAmdIndex* idx, const void* vectors, int32_t nadd,
                  int normalized);

/* Incremental delete — mirrors VectorIndex::DeleteIndex(SizeType)
 * (inc/Core/VectorIndex.h, BKT DeleteIndex -> Labelset::Insert,
 * src/Core/BKT/BKTIndex.cpp:896): flags the ids; subsequent searches
 * filter them with the reference's CheckIfNotDeleted dispatch (already
 * covered by the parity suite). Persisted by save_index in deletes.bin. */
int sptag_amd_delete(SptagAmdIndex* idx, const int32_t* vids, int32_t n);
/* the by-vector overload (BKTIndex.cpp:876: search CEF results, delete the
 * exact duplicates at distance < 1e-6) */
int sptag_amd_delete_by_vector(SptagAmdIndex* idx, const void* vectors,
                               int32_t n);
int64_t sptag_amd_deleted_count(const SptagAmdIndex* idx);

/* Write the index back out in the reference's byte format
 * (vectors/tree/graph/deletes + indexloader.ini). */
int sptag_amd_save_index(SptagAmdIndex* idx, const char* folder);

/* Search-parameter setter — the C-ABI form of the reference's
 * SetParameter("NumberOfInitialDynamicPivots"/"NumberOfOtherDynamicPivots"/
 * "ThresholdOfNumberOfContinuousNoBetterPropagation"/"MaxCheck", ...)
 * (BKTIndex.cpp:980, ParameterDefinitionList.h). Pass <=0 to keep a
 * value unchanged. */
void sptag_amd_set_search_params(SptagAmdIndex* idx, int32_t init_pivots,
                                 int32_t other_pivots,
                                 int32_t nobetter_threshold,
                                 int32_t default_maxcheck);

/* Shard sets — several indexes searched as one, the per-shard top-k lists
 * merged on the GPU. This is the in-process form of the reference's
 * aggregator, AggregatorService::AggregateResults
 * (src/Aggregator/AggregatorService.cpp:363): every shard answers the whole
 * query batch, the lists are concatenated and the best k selected. The
 * result contract is the single index's, over global ids: ascending
 * (dist, global vid) with global vid = shard-local vid + vid_base[shard],
 * then vid = -1 padding that carries the padding distance of the
 * single-index search. Ties between shards are therefore decided by global
 * id, exactly as ties inside one index are decided by id.
 *
 * Merge utility, usable without a shard set (e.g. on lists gathered from
 * other processes). vids/dists are [nshards][nq][k_in]; every list is
 * ascending (dist, vid) and its padding is a suffix of vid < 0 entries. The
 * outputs are [nq][k_out] and must not overlap the inputs; k_out may exceed
 * nshards*k_in, the surplus is padding. 1 <= nshards <= 64,
 * 1 <= k_in, k_out <= 1024, every vid_base[s] >= 0; vid_base is always a
 * host array. The _device form takes buffers on GPU `device`, runs on that
 * device's default stream and returns when the output is complete. */
int sptag_amd_merge_topk_device(int device, int32_t nshards, int32_t nq,
                                int32_t k_in, int32_t k_out,
                                const int32_t* d_vids, const float* d_dists,
                                const int32_t* vid_base,
                                int32_t* d_out_vids, float* d_out_dists);
int sptag_amd_merge_topk(int device, int32_t nshards, int32_t nq,
                         int32_t k_in, int32_t k_out,
                         const int32_t* vids, const float* dists,
                         const int32_t* vid_base,
                         int32_t* out_vids, float* out_dists);

/* A set of 1..64 shards that agree in dim, value type and distance method;
 * BKT and KDT shards may be mixed, and the shards may sit on one device or
 * on several. vid_base[s] is the global id of shard s's vector 0; NULL
 * means the running sum of the shards' vector counts at create time.
 * Returns NULL, with a line on stderr, when nshards is out of range, a
 * shard is NULL, the shards disagree, or some vid_base[s] + num_vectors(s)
 * does not fit int32.
 *
 * The set borrows the handles: it never frees them, and they must outlive
 * it. Add and delete stay on the shard handles and a set sees them on its
 * next call. vid_base is fixed at create time, so vectors added to any
 * shard but the last run into the next shard's ids under the default bases:
 * a set whose shards will grow needs explicit bases that leave room.
 * Iterators over a set are not provided. */
typedef struct SptagAmdShards SptagAmdShards;
SptagAmdShards* sptag_amd_shards_create(SptagAmdIndex* const* shards,
                                        int32_t nshards,
                                        const int32_t* vid_base);
void sptag_amd_shards_free(SptagAmdShards* set);

/* Batched search of the whole set; arguments and result layout as in the
 * single-index search, ids global. Shards on one device run one after
 * another in the calling thread; with more than one device there is one
 * host thread per device, and queries and lists travel between devices by
 * hipMemcpyPeer (peer access is not required). The merge runs on the device
 * of shard 0. A failing shard's error code is returned and the outputs are
 * left untouched. Concurrent callers on one set are serialized. */
int sptag_amd_shards_search_batch(SptagAmdShards* set, const void* queries,
                                  int32_t nq, int32_t k, int32_t max_check,
                                  int32_t* out_vids, float* out_dists);
/* Device-pointer variant: all three buffers on the device of shard 0. */
int sptag_amd_shards_search_batch_device(SptagAmdShards* set,
                                         const void* d_queries, int32_t nq,
                                         int32_t k, int32_t max_check,
                                         int32_t* d_out_vids,
                                         float* d_out_dists);
/* Exact brute-force top-k over all shards: the same fan-out over the
 * per-shard truth, the same merge. Host pointers. */
int sptag_amd_shards_truth(SptagAmdShards* set, const void* queries,
                           int32_t nq, int32_t k, int32_t* out_vids,
                           float* out_dists);
/* The same over sptag_amd_exact_search per shard. */
int sptag_amd_shards_exact_search(SptagAmdShards* set, const void* queries,
                                  int32_t nq, int32_t k, int32_t* out_vids,
                                  float* out_dists);
int32_t sptag_amd_shards_count(const SptagAmdShards* set);
/* sum of the shards' current vector counts */
int64_t sptag_amd_shards_num_vectors(const SptagAmdShards* set);

/* metadata */
int32_t sptag_amd_num_vectors(const SptagAmdIndex* idx);
int32_t sptag_amd_dim(const SptagAmdIndex* idx);
int     sptag_amd_valuetype(const SptagAmdIndex* idx);
int     sptag_amd_distmethod(const SptagAmdIndex* idx);
int32_t sptag_amd_degree(const SptagAmdIndex* idx);
int32_t sptag_amd_default_maxcheck(const SptagAmdIndex* idx);
/* 0 = BKT, 1 = KDT (the loaded indexloader.ini IndexAlgoType). */
int     sptag_amd_algo(const SptagAmdIndex* idx);

/* Runtime probe: 1 if a usable HIP device exists (search will run), else 0. */
int sptag_amd_gpu_available(void);

/* Version/build tag of the loaded library (for the loud-failure message). */
const char* sptag_amd_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
