/*
 * pcr.h — C ABI of libpcr_hip.so: the MI355X-native (gfx950) k-NN correspondence + ICP + plane-inlier
 * hot path of yf26/Hands-On-Point-Cloud-Processing.
 *
 * This is the drop-in boundary: plain pointers and sizes, caller-owned memory, `int`
 * status (0 = ok, negative = error; never exit()), one context per GPU / per process.  The source-level
 * replacement headers in include/pcr/ (kdtree.hpp, resultSet.hpp, KDTreeVectorOfVectorsAdaptor.h,
 * registration.hpp) forward to these entry points; INTEGRATION.md shows the reference-side bindings.
 * All file:line citations are relative to the reference repository root.
 *
 * Arithmetic contracts (bit-exact parity with the reference's CPU path):
 *   A1  f32 squared distance ((dx*dx + dy*dy) + dz*dz), d = q - t, every op rounded, no FMA
 *       — nanoflann::L2_Adaptor::evalMetric, Homework9/hw9/include/nanoflann.hpp:383-408
 *   A2  f64 d = sqrt(((dx*dx) + dy*dy) + dz*dz), d = t - q
 *       — KDTreeKNNSearch leaf loop, Homework2/hw2/include/kdtree.hpp:339-348
 *   ties: minimum distance, then lowest index (canonical rule)
 */
#ifndef PCR_H
#define PCR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_OK 0
#define PCR_ERR_ARG (-1)     /* bad argument */
#define PCR_ERR_HIP (-2)     /* a HIP runtime call failed; see pcr_ctx_last_error */
#define PCR_ERR_NOMEM (-3)
#define PCR_ERR_STATE (-4)   /* e.g. collective requested before pcr_comm_init */
#define PCR_ERR_COMM (-5)    /* RCCL failure */
#define PCR_ERR_EMPTY (-6)   /* ICP iteration kept no pair (the reference would divide by zero) */

typedef struct pcr_ctx pcr_ctx;
typedef struct pcr_cloud pcr_cloud;   /* an N-point f32 cloud resident in HBM as SoA x[N] | y[N] | z[N] */

/* host layouts accepted / produced at the boundary */
enum pcr_layout {
    PCR_SOA = 0,   /* x[n], y[n], z[n] contiguous — Eigen column-major N x 3 MatrixXf (registration.cpp:903) */
    PCR_AOS3 = 1,  /* xyzxyz...        — KITTI rows without intensity */
    PCR_AOS4 = 2,  /* xyz?xyz?...      — pcl::PointXYZ (16 B) and KITTI .bin rows (test.hpp:26-28) */
    PCR_AOS6 = 6   /* xyz???xyz???...  — hw9 registration .bin rows: xyz + normal (registration.cpp:25-26) */
};

/* ---- context ------------------------------------------------------------------------------------ */
int pcr_device_count(int* count);                     /* GPUs visible to this process (hipGetDeviceCount) */
int pcr_ctx_create(int device, pcr_ctx** out);
int pcr_ctx_destroy(pcr_ctx* ctx);
int pcr_ctx_sync(pcr_ctx* ctx);                       /* wait for the context's HIP stream */
const char* pcr_ctx_last_error(const pcr_ctx* ctx);   /* text of the last failure on this context */
const char* pcr_version(void);
/* device facts for the bench / roofline: name (e.g. "gfx950"), CU count, HBM bytes */
int pcr_ctx_device_info(const pcr_ctx* ctx, char* arch, size_t arch_cap, int* n_cu, uint64_t* hbm_bytes);

/* ---- clouds --------------------------------------------------------------------------------------- */
int pcr_cloud_create(pcr_ctx* ctx, const float* host_xyz, size_t n, int layout, pcr_cloud** out);
/* clone and assign copy a spatial shard's global indices with its points (pcr_cloud_global_index answers the same for the copy); assign
 * drops dst's own when src has none, and dst loses the mapping of an earlier pcr_cloud_sort_for_target (it is now in src's order) */
int pcr_cloud_clone(pcr_ctx* ctx, const pcr_cloud* src, pcr_cloud** out);
int pcr_cloud_assign(pcr_ctx* ctx, pcr_cloud* dst, const pcr_cloud* src);   /* dst <- src, same size, on device */
int pcr_cloud_read(pcr_ctx* ctx, const pcr_cloud* c, float* host_xyz, int layout);
size_t pcr_cloud_size(const pcr_cloud* c);
/* synchronises the context's stream, then frees the cloud's HBM (hipFree) — whatever context it is destroyed through */
int pcr_cloud_destroy(pcr_ctx* ctx, pcr_cloud* c);
/* The ICP loops clone the source into a working copy; that copy's buffer is parked on the context (at most two, each <= 2 GB, replaced
 * as soon as a call needs another size) so that the next call's clone costs no hipMalloc / hipFree.  pcr_ctx_trim frees what is parked. */
int pcr_ctx_trim(pcr_ctx* ctx);
int pcr_ctx_parked_bytes(const pcr_ctx* ctx, uint64_t* bytes);   /* HBM held by those parked buffers right now */
/* DIAGNOSTIC, no stability promise (it may change or go with the route it describes; nothing but tests should call it).
 * The one-wave-per-query k-NN route (at most 16 host queries on a handle): the ticket its waves draw from, read behind a
 * stream synchronisation, the batch size m of the last call, the calls so far and those whose completion word did not show up in time (they
 * fell back to a stream synchronisation).  The wave that draws ticket m - 1 modulo m publishes the completion word, so between calls the
 * ticket is a multiple of the last m: a call with another m starts it from zero.  Any pointer may be NULL. */
int pcr_ctx_knn_coop_state(pcr_ctx* ctx, uint32_t* ticket, uint64_t* m, uint64_t* calls, uint64_t* unseen);

/* ---- A6 (search): 1-NN correspondence, brute force over LDS-tiled targets ----------------------------
 * replaces the loop `for i: tar_mat_index.index->findNeighbors(result_set, query, ...)`,
 * Homework9/hw9/src/registration.cpp:925-934, and KDTreeVectorOfVectorsAdaptor::query(q, 1, ...),
 * Homework3/nano_vs_my/include/KDTreeVectorOfVectorsAdaptor.h:80-85.
 * idx[i] = argmin_j d2(src_i, tgt_j) (A1, canonical ties), d2[i] the squared distance.
 * A query with no acceptable candidate (n_tgt == 0, NaN input, d2 >= FLT_MAX — nanoflann.hpp:163,1360)
 * gets idx = UINT32_MAX, d2 = +inf. */
int pcr_nn1_f32(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, uint32_t* idx, float* d2);
/* same, results stay in HBM (context workspace) for the Kabsch step; asynchronous on the ctx stream */
int pcr_nn1_f32_async(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src);
/* ---- a caller's OWN loop over the same pair (what the searches inside pcr_icp_p2p_f32 do, one call at a time) --------------------
 * pcr_cloud_sort_for_target: re-orders `cloud` IN PLACE into the order of the target's index (built if needed), once, before the loop:
 *   the queries of a wave are then neighbours in space (coalesced loads, shared candidates; at >= 4 M target points the tile search
 *   needs it).  orig_index (host, n entries, may be NULL) receives, per position of the re-ordered cloud, the index the point had
 *   before; pcr_kabsch_sums reports `last_kept` in the ORIGINAL numbering for such a cloud (registration.cpp:939's "last pair").
 *   Moving the cloud with pcr_transform_f32 keeps the order valid; results of pcr_nn1_fetch are in the re-ordered numbering.
 * pcr_nn1_f32_loop: one search of such a loop — seeded by the previous call's correspondences, and bounded by the gate of
 *   registration.cpp:936: a pair is only ever kept if d2 < max_corr, so a query with no target inside the gate comes back as
 *   "none" (idx UINT32_MAX, d2 +inf) instead of with a neighbour the caller would discard.  Same kept pairs, same sums, bit for bit. */
int pcr_cloud_sort_for_target(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud* cloud, uint32_t* orig_index);
int pcr_nn1_f32_loop(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr);
/* fetch the results of the caller's last pcr_nn1_f32_async / pcr_nn1_f32_loop for n queries.
 * WHICH SEARCH: the context has ONE result workspace, and every stage that searches writes it — the two calls above, and inside the library
 * the searches of pcr_icp_p2p_f32 and pcr_icp_p2plane_f32.  pcr_nn1_fetch answers only while the LAST search on the context was one of
 * the caller's two: after an ICP call it returns PCR_ERR_STATE (n != the size of the last search: PCR_ERR_ARG), never the loop's
 * correspondences.  Every other stage (pcr_cloud_sort_for_target and pcr_cloud_shard_spatial, which order queries but pair nothing; k-NN,
 * radius, normals, voxel grids, descriptors, clustering, PointNet rows, ...) leaves the workspace alone, and so does anything done to the
 * clouds afterwards: the rows are a record of the search as it ran, indices in the target's numbering at that time. */
int pcr_nn1_fetch(pcr_ctx* ctx, size_t n, uint32_t* idx, float* d2);

/* ---- A8: transformCloudInplace, Homework9/hw9/src/registration.cpp:165-178 ---------------------------
 * p <- R p + t per point, f32, unfused, row-wise ((R_i0 x + R_i1 y) + R_i2 z) + t_i.  T row-major 4x4. */
int pcr_transform_f32(pcr_ctx* ctx, pcr_cloud* cloud, const float T[16]);

/* ---- A7 (accumulate): cross-covariance sums over the kept pairs of the last pcr_nn1_f32_async ---------
 * sums[0..2] = sum p, [3..5] = sum q, [6..14] = sum q_r p_c (row-major, rows = target), [15] = count,
 * f64, over pairs with d2 < max_corr (squared distance vs un-squared parameter, registration.cpp:936).
 * last_kept: index of the last kept source or -1; last_d2: its squared distance (loss, :939).
 * WHICH SEARCH: as for pcr_nn1_fetch the last search on the context must be the caller's own, and here it must be the search of exactly
 * (tgt, src) — the same two handles — with neither modified since (pcr_transform_f32, pcr_cloud_assign, an in-place
 * pcr_cloud_sort_for_target, destroy + create: a new handle is a new cloud even at the old address).  The sums pair src's points as they are
 * now with the target points the search named, so a cloud that moved or changed order in between would give sums of pairs that never
 * were: PCR_ERR_STATE instead.  (A loop therefore runs search -> sums -> transform, as pcr_icp_p2p_f32 does.) */
int pcr_kabsch_sums(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr,
                    double sums[16], int64_t* last_kept, float* last_d2);
/* ---- A7 (solve): registration.cpp:979-998 incl. the det<0 branch (:990-996). Host, f64. -------------- */
int pcr_kabsch_solve(const double sums[16], float R[9], float t[3]);
/* The same solve in the form the device-resident ICP loop runs, its operations spread over a group of lanes (bit for bit the
 * result of pcr_kabsch_solve): by the host's lane group, and by one wavefront per problem on the GPU — n problems, host arrays
 * sums[16 n] in, R[9 n], t[3 n], rc[n] out; rc[i] is what pcr_kabsch_solve returns for problem i, R and t of a problem that
 * kept no pair are zero. */
int pcr_kabsch_solve_lanes(const double sums[16], float R[9], float t[3]);
int pcr_kabsch_solve_batch_device(pcr_ctx* ctx, const double* sums, size_t n, float* R, float* t, int* rc);

/* ---- A9: Registration::ICPpoint2point, Homework9/hw9/src/registration.cpp:862-1011 -------------------
 * (after its normal-space sampling: the clouds passed here are the sampled clouds). */
typedef struct {
    float max_corr;       /* setICPparams max_corres_dist (registration.hpp:126-137); vs SQUARED distance */
    uint64_t max_iter;    /* setICPparams max_iter */
    float eps;            /* setICPparams loss_epsilon */
} pcr_icp_params;

typedef struct {
    uint64_t iters_run;   /* iterations whose update was applied */
    int32_t converged;    /* the `unchanged_count > 15` break fired (:954) */
    int32_t empty_pairs;  /* an iteration kept no pair */
    uint64_t last_pairs;  /* kept pairs (whole job, after the all-reduce) in the last NN pass */
    float last_loss;
    float reserved;
    double ms_total;      /* wall time of the loop */
    double ms_nn;         /* HIP-event time of the 1-NN kernel, summed over iterations; 0 unless pcr_tune_set(ctx, "prof", >= 1) */
    uint64_t nn_launches;
} pcr_icp_stats;

/* src is not modified (a working copy is transformed in place, :872-874). init_T / out_T row-major 4x4.
 * With a communicator attached (pcr_comm_*), src is this rank's shard: the 16 f64 sums are all-reduced
 * once per iteration and every rank computes the identical pose. */
int pcr_icp_p2p_f32(pcr_ctx* ctx, const pcr_cloud* src, const pcr_cloud* tgt, const float init_T[16],
                    const pcr_icp_params* prm, float out_T[16], pcr_icp_stats* stats);

/* Which tail the iterations of the last pcr_icp_p2p_f32 call on this context took (diagnostics; every chain gives the same bits):
 * 0 = the synchronous loop, no call yet, or a call that failed; 1 = sums, solve and move as launches of their own; 2 = sums -> solve + move;
 * 3 = sums + solve + move in one launch; 4 = sums + solve in one launch, the NEXT search moves the cloud (tune "icp_move_in_search"); 5 = the sums
 * alone in one launch, the NEXT search reduces them, solves and moves the cloud (tune "icp_solve_in_search"). */
int pcr_icp_last_chain(const pcr_ctx* ctx);
/* How the last pcr_icp_p2p_f32 call on this context learnt its loop's state (diagnostics; same bits either way): 0 = copies and events on the stream
 * (also: no call yet, a call that failed, the synchronous loop, a call of no iteration); 1 = written into pinned host memory by the sums + solve launch
 * itself (chain 4), or by the next chunk's first search and the call's finishing launch (chain 5); tune "icp_host_snapshots": 2 = off. */
int pcr_icp_last_snapshots(const pcr_ctx* ctx);
/* Host logic, no GPU: with an arrival counter per accumulator replica (tune "icp_ticket_levels": 1 = one counter, 2 = per replica), how many of the
 * `blocks` workgroups of a sums + solve launch arrive at replica `replica` (0 .. 7); 0 = the launch does not reach it and nobody waits for it. */
uint32_t pcr_icp_replica_members(uint32_t blocks, uint32_t replica);
/* Host logic, no GPU: would a single-rank exhaustive loop of n_src points over a target of n_tgt points, whose searches take the three-level
 * sphere kernel, run chain 4?  The tunes are passed as RAW values, 0 = default: icp_move_in_search (1 on / 2 off), icp_fused_sums (2 off),
 * icp_fused_sums_min, nn1_s3_transposed (2 = the form without the move), nn1_sphere_qg, nn1_sphere_l0_per_slice, nn1_sphere_blocks (the search
 * must be ONE slice: it moves its queries in place).  Returns 1 or 0. */
int pcr_icp_move_route(uint64_t n_src, uint64_t n_tgt, int nranks, int64_t move_in_search, int64_t fused_sums, int64_t fused_sums_min,
                       int64_t s3_transposed, int64_t sphere_qg, int64_t sphere_l0_per_slice, int64_t sphere_blocks);
/* Host logic, no GPU: would that loop run chain 5 — chain 4's conditions (pcr_icp_move_route) and the tune icp_solve_in_search: 1 = on, 2 = off,
 * 0 = auto, which holds only while icp_move_in_search is 0 as well (a caller that sets that tune to 1 keeps chain 4) and is then the library's default:
 * on for up to pcr_icp_solve_in_search_auto() source points (0 = auto is off).  Raw tune values as above.  Returns 1 or 0. */
int pcr_icp_solve_route(uint64_t n_src, uint64_t n_tgt, int nranks, int64_t solve_in_search, int64_t move_in_search, int64_t fused_sums,
                        int64_t fused_sums_min, int64_t s3_transposed, int64_t sphere_qg, int64_t sphere_l0_per_slice, int64_t sphere_blocks);
uint64_t pcr_icp_solve_in_search_auto(void);
/* Host logic, no GPU: what the default three-level sphere kernel visits in ONE level-0 super-tile S0 (131 072 records) given its flag masks, in its
 * order.  rows[t] bit j: level 0 flagged level-1 tile T1 = (S0 * 8 + t) * 32 + j (512 records); tiles[T1 - S0 * 256] bit k: level 1 flagged level-2
 * tile T1 * 16 + k (32 records).  Tiles at or behind n_rec records (the padded size of the index) are not visited.  The visits are written as pairs
 * (kind, value): 0 = a run starts, value = the level-1 super-tile (eight level-1 tiles); 1 = a level-1 tile of the run; 2 = a batch of value (1 ... 4)
 * level-2 tiles starts; 3 = a level-2 tile of the batch.  *n_out = the number of pairs; PCR_ERR_ARG (with *n_out set) when out holds fewer than
 * 2 * *n_out words (cap counts words). */
int pcr_s3_walk_visits(uint32_t S0, const uint32_t rows[8], const uint16_t tiles[256], uint32_t n_rec, uint32_t* out, size_t cap, size_t* n_out);

/* ---- A10: plane-inlier count, Homework4/ground_detection_ransac.py:138-139,152-153 -------------------
 * dist_i = |((x a + y b) + z c) + d| in f64; counts[h] = #{i : dist_i < thr} for n_planes hypotheses in
 * ONE pass over the points. planes4: n_planes x 4 f64. */
int pcr_plane_count_f64(pcr_ctx* ctx, const pcr_cloud* pts, const double* planes4, size_t n_planes,
                        double thr, int64_t* counts);
/* final mask of one plane (:152-153): mask[i] = dist_i < thr (uint8), n_inliers optional */
int pcr_plane_mask_f64(pcr_ctx* ctx, const pcr_cloud* pts, const double plane4[4], double thr,
                       uint8_t* mask, int64_t* n_inliers);

/* ---- A2/A4: batched k-NN with the hw2 arithmetic (f64, sqrt), canonical order ------------------------
 * replaces `KNNResultSet rs(k); KDTreeKNNSearch(root, db, rs, query)` per query
 * (Homework2/hw2/include/kdtree.hpp:329-364, benchmark.hpp:59-66).
 * db: n x 3 f64 AoS (vector<vector<double>> flattened), q: m x 3. idx/dist: m x k; empty slots (n < k)
 * hold (1e10, 0) like the pre-filled result set (resultSet.hpp:35-42). k <= 32.
 * The 1e10 rule: that result set starts with worstDist = 1e10 and rejects dist > worstDist (resultSet.hpp:32,69), so
 * a point at d > 1e10 is never a neighbour — its slot stays empty — and one at d == 1e10 exactly is, with its index.
 * Every route of the search answers that way (the exhaustive scan, the grid batches, the one-wave calls). */
int pcr_knn_f64(pcr_ctx* ctx, const double* db, size_t n, const double* q, size_t m, int k,
                int32_t* idx, double* dist);
/* ---- A11: radius search (kdtree.hpp:367-402, resultSet.hpp:130-140): all j with d <= r, CSR, ascending
 * index. Pass idx = dist = NULL to get row_ptr (m+1) only, then call again with arrays of row_ptr[m]. */
int pcr_radius_f64(pcr_ctx* ctx, const double* db, size_t n, const double* q, size_t m, double r,
                   int64_t* row_ptr, int32_t* idx, double* dist);

/* ---- the same searches on a database kept resident in HBM: the counterpart of the tree object the
 * reference builds once (KDTreeConstruction, kdtree.hpp:419; nanoflann buildIndex, nanoflann.hpp:1191) and
 * queries many times.  squared = 0: hw2 contract (d = sqrt(s)); squared = 1: nanoflann contract for
 * T = double (squared L2, nanoflann.hpp:403-406; empty slots hold (DBL_MAX, -1)). */
typedef struct pcr_db64 pcr_db64;
int pcr_db64_create(pcr_ctx* ctx, const double* db, size_t n, pcr_db64** out);
int pcr_db64_destroy(pcr_ctx* ctx, pcr_db64* db);
size_t pcr_db64_size(const pcr_db64* db);
int pcr_db64_knn(pcr_ctx* ctx, const pcr_db64* db, const double* q, size_t m, int k, int squared,
                 int32_t* idx, double* dist);
int pcr_db64_radius(pcr_ctx* ctx, const pcr_db64* db, const double* q, size_t m, double r,
                    int64_t* row_ptr, int32_t* idx, double* dist);

/* ---- device-resident radius rows: the CSR of a radius search kept in HBM (12 B per neighbour never cross PCIe unless asked for) --------
 * What the batched consumers of the reference do with radius rows is reduce them — neighbour counts and 1 / count weights
 * (Homework7/hw7/src/iss_detector.cpp:48-76), neighbourhood moments for normals (Homework1 pca_normal.py:89-103) — or walk them in query
 * order (the self-query loop of Homework2/hw2/include/benchmark.hpp:66-70).  q == NULL: every point of db queries db (m is ignored).
 * Same rows as pcr_db64_radius, bit for bit (ascending index inside a row, d <= r inclusive).  The database must outlive the handle. */
typedef struct pcr_rows pcr_rows;
int pcr_db64_radius_rows(pcr_ctx* ctx, const pcr_db64* db, const double* q, size_t m, double r, pcr_rows** out);
int pcr_rows_destroy(pcr_ctx* ctx, pcr_rows* rows);
int pcr_rows_info(const pcr_rows* rows, size_t* m, uint64_t* total);            /* queries, reported neighbours */
int pcr_rows_row_ptr(const pcr_rows* rows, int64_t* row_ptr);                   /* the m + 1 offsets (host copy, no GPU work) */
/* rows [row_begin, row_end) -> idx / dist (either may be NULL), (row_ptr[row_end] - row_ptr[row_begin]) entries: iterate in bounded blocks */
int pcr_rows_fetch(pcr_ctx* ctx, const pcr_rows* rows, size_t row_begin, size_t row_end, int32_t* idx, double* dist);
enum pcr_rows_op { PCR_ROWS_COUNT = 0, PCR_ROWS_SUM_DIST = 1, PCR_ROWS_MAX_DIST = 2 };
int pcr_rows_reduce(pcr_ctx* ctx, const pcr_rows* rows, int op, double* out);    /* out[m]; an empty row gives 0 */
/* per row: mean (m x 3) and scatter matrix sum (p - mean)(p - mean)^T / count as xx xy xz yy yz zz (m x 6) of its neighbours' coordinates */
int pcr_rows_moments(pcr_ctx* ctx, const pcr_rows* rows, double* mean, double* cov);

/* Registration::ICPpoint2plane (registration.hpp:195-202, registration.cpp:710-860): the point-to-plane variant on the same
 * 1-NN loop.  tgt_normals: one normal per target point (a cloud whose x/y/z are normal_x/y/z; e.g. floats 3..5 of hw9's .bin
 * rows).  Rows A = [n x p, n], b = n.q - n.p in f32 as written (:807-814); normal equations in f64; update R_delta = I + [x]_x,
 * NOT re-orthonormalised (:843).  Same parameters, stop rules and stats as pcr_icp_p2p_f32; `empty_pairs` is also set when
 * the 6x6 system is singular.  Sources shard like the point-to-point loop: one all-reduce of 29 f64 per iteration. */
int pcr_icp_p2plane_f32(pcr_ctx* ctx, const pcr_cloud* src, const pcr_cloud* tgt, const pcr_cloud* tgt_normals, const float init_T[16],
                        const pcr_icp_params* prm, float out_T[16], pcr_icp_stats* stats);

/* ---- next row N3: voxel-grid down-sampling, Homework1 voxel_filter.py:17-52 (centroid mode) -----------------
 * One centroid per occupied voxel of edge leaf_size, in ascending voxel-index order; f32 arithmetic and summation
 * order of the reference (bit-exact), including its quirk that the last voxel of the sorted order is never emitted
 * (:41-50).  The result is a new device cloud (feed it to pcr_icp_p2p_f32 without leaving HBM). */
int pcr_voxel_filter_f32(pcr_ctx* ctx, const pcr_cloud* in, double leaf_size, pcr_cloud** out);

/* ---- next row N1: ISS keypoints, ISSKeypoint::compute (Homework7/hw7/src/iss_detector.cpp:38-152) ----------------
 * Batched radius neighbourhoods over a uniform grid instead of one kd-tree search per point.  Membership uses hw7's
 * float arithmetic (src/kdtree.cpp:310-316) bit for bit; the neighbourhood covariance is accumulated in f64 (the
 * reference: f32 in tree-visit order through Eigen) and its eigenvalues come from an f64 Jacobi solver, rounded to
 * f32 before the gamma tests (:79).  Setters mirrored: setLocalRadius / setNonMaxRadius / setThreshold(g21, g32) /
 * setMinNeighbors / useWeightedCovMat (iss_detector.cpp:8-31).
 * is_key[i] = 1 iff input point i is a keypoint (the reference emits them in ascending i, :103); lambda3 (optional, n
 * floats) is lambda3_vec_forall (:67); neighbor_counts (optional, n) is rnn_idx[i].size() (:47-57); n_keypoints
 * (optional) the number of ones. */
typedef struct {
    float local_radius;
    float non_max_radius;
    float gamma21, gamma32;
    int min_neighbors;
    int weighted_covariance;
} pcr_iss_params;
int pcr_iss_keypoints_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_iss_params* prm, uint8_t* is_key, float* lambda3,
                          uint32_t* neighbor_counts, uint64_t* n_keypoints);

/* ---- next row N1 (second consumer): batched exact k-NN on resident clouds + per-point PCA normals ------------------
 * k-NN of every point of `queries` (may be `db` itself) in `db`, k <= 32, over a uniform grid; f64 leaf arithmetic of
 * hw2 / FLANN / nanoflann at dim 3 on the f32 coordinates widened to f64: s = ((dx*dx) + dy*dy) + dz*dz.
 * squared != 0: order and report s (FLANN / open3d / nanoflann contract), empty slots (DBL_MAX, -1); radius >= 0 adds the
 * hybrid-search cap s < radius^2 (strict, FLANN's KNNRadiusResultSet); radius < 0: none.
 * squared == 0: order and report d = sqrt(s) (hw2, kdtree.hpp:341-346), empty slots (1e10, 0) (resultSet.hpp:35-42);
 * the 1e10 rule of pcr_knn_f64 holds: d > 1e10 is never a neighbour (not counted in `found`), d == 1e10 is one.  The
 * squared mode has no such rule: every finite s below the cap is a neighbour.
 * A non-finite database point is never a neighbour and a non-finite query finds nothing, in both modes.
 * Canonical order: value ascending, then index ascending.  idx, dist: m x k row-major; found (optional): m. */
int pcr_cloud_knn_f64(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* queries, int k, double radius, int squared,
                      int32_t* idx, double* dist, uint32_t* found);
/* pca_normal.py:89-103: normals[i] = eigenvector of the smallest eigenvalue of the scatter matrix of the <= k nearest
 * points within `radius` of point i (itself included; the reference: search_hybrid_vector_3d(radius = 5, max_nn = 10) +
 * PCA, :17-36), zeros when fewer than 3.  Sign and eigen-solver follow FastEigen3x3 (the reference's PCA_faster, :39-45;
 * np.linalg.eig leaves the sign unspecified) with ONE exception: a scatter matrix that is exactly diag(a, a, b) with a < b
 * (a row of points along z) gets (1, 0, 0), where FastEigen3x3 answers (0, 0, 1) — the row's own direction, the
 * eigenvector of the LARGEST eigenvalue.  pcr_fast_eigen3x3 below keeps the reference's answer.  Zeros also when the
 * scatter matrix is zero (coincident neighbours).  normals: n x 3 f64. */
int pcr_normals_knn_f64(pcr_ctx* ctx, const pcr_cloud* cloud, int k, double radius, double* normals);

/* pca_normal.py:17-36 PCA(data, correlation = False, sort = True) of the whole cloud: eigenvalues descending, eigenvectors in
 * the columns of the row-major 3x3 (signs unspecified, as with np.linalg.eig); centre (optional) = sum / n.  Non-finite
 * points are skipped; PCR_ERR_EMPTY without a finite point. */
int pcr_cloud_pca_f64(pcr_ctx* ctx, const pcr_cloud* cloud, double eigenvalues[3], double eigenvectors[9], double centre[3]);

/* ---- next row N2: PCA ground fit around the inlier count, Homework4/ground_detection_SVD.py:46-101 --------------
 * f64 arithmetic on the f32 points of the cloud (the reference's points are f64 after pcd_preprocessing, :35).
 * pcr_fast_eigen3x3 (host logic, no GPU) = mylib.FastEigen3x3 (Homework1/.../my_pybind11/src/mylib.cpp:105-189): unit
 * eigenvector of the smallest eigenvalue of the symmetric row-major A; (0,0,0) when the signed maximum of A is 0. */
int pcr_fast_eigen3x3(const double A[9], double normal[3]);
/* extract_initial_seeds (:46-71): seed_mask[i] = z_i < -1.73 + 0.5 && z_i < LPR_z + threshold_seeds, LPR_z = mean z of
 * the lpr_size lowest candidates (all of them when fewer).  upper_bound / n_seeds optional. */
int pcr_ground_seeds_f64(pcr_ctx* ctx, const pcr_cloud* cloud, size_t lpr_size, double threshold_seeds, uint8_t* seed_mask,
                         double* upper_bound, uint64_t* n_seeds);
/* ground_detection (:88-101): seeds, then max_iter (>= 1) x { estimate_plane (:74-85); inliers = |[p 1].params| <
 * threshold_dist }.  params = the last plane (normal, d); ground_mask = the last inliers_filter; PCR_ERR_EMPTY when a
 * fit has no point (the reference would propagate NaN). */
int pcr_ground_detection_f64(pcr_ctx* ctx, const pcr_cloud* cloud, int max_iter, size_t lpr_size, double threshold_dist,
                             double params[4], uint8_t* ground_mask, uint64_t* n_ground);

/* ---- Homework4 foreground stage: DBSCAN and statistical outlier removal, ground_detection_SVD.py:22-37 and :173 ---------
 * Distances as pcr_cloud_knn_f64: the f32 coordinates widened to f64, s = ((dx*dx) + dy*dy) + dz*dz, unfused.
 * pcr_dbscan_f32 (foreground_pcd.cluster_dbscan(0.8, 20), :173; foreground_clustering_DBSCAN.py):
 *   N(p) = { j : s(p, j) <= eps*eps } (p included, eps*eps the f64 product); core(p) = |N(p)| >= min_points (min_points <= 1:
 *   every finite point is core).  Clusters = connected components of the core points under "within eps"; a cluster's key is
 *   its smallest core index (input numbering) and ids 0, 1, ... follow ascending keys.  A non-core point with a core neighbour
 *   (border point) takes the SMALLEST id among its core neighbours' clusters; every other point is noise, label -1.
 *   Non-finite points are noise and nobody's neighbour.  This is what sklearn.cluster.DBSCAN returns (points visited in
 *   index order, a border point goes to the first cluster that reaches it); equivalence with Open3D's ClusterDBSCAN (BFS in
 *   the same order, an inclusive or strict radius test depending on its version) is UNPINNED.
 *   labels: n int32 (required); is_core: n bytes, neighbor_counts: n u32 (|N(p)|), n_clusters: optional.  PCR_ERR_ARG for
 *   eps < 0, NaN or inf, or n > 2^31 - 16; eps = 0 links exact duplicates only.  PCR_ERR_STATE if the union-find's bound
 *   is exceeded (never in a correct run).
 * pcr_statistical_outlier_f32 (pcd.remove_statistical_outlier(nb_neighbors = 20, std_ratio = 2.7), :33; Open3D's
 * PointCloud::RemoveStatisticalOutliers):
 *   avg[i] = (sum of sqrt(s) over the nb_neighbors nearest points, itself included — pcr_cloud_knn_f64 with squared = 1,
 *   fewer when n < k — added in slot order) / found, -1 for a non-finite point; valid = points with found > 0;
 *   mean = sum_{avg > 0} avg / valid; std = sqrt(sum_{avg > 0} (avg - mean)^2 / (valid - 1)); thr = mean + std_ratio std;
 *   keep[i] = avg[i] > 0 && avg[i] < thr (Open3D's quirk: a point with k or more exact duplicates has avg 0 and is dropped).
 *   The two global sums are deterministic (fixed reduction order) but not Open3D's sequential std::accumulate bit for bit.
 *   stats3 = (mean, std, thr); kept_cloud = a new device cloud of the kept points in ascending input order (input to the
 *   ground fit or to DBSCAN without a host round trip).  Every output is optional.  PCR_ERR_ARG for nb_neighbors < 1 or
 *   > 32 (the limit of the k-NN service) and for std_ratio <= 0 or non-finite (Open3D rejects the same). */
int pcr_dbscan_f32(pcr_ctx* ctx, const pcr_cloud* cloud, double eps, int min_points, int32_t* labels, uint8_t* is_core,
                   uint32_t* neighbor_counts, uint64_t* n_clusters);
int pcr_statistical_outlier_f32(pcr_ctx* ctx, const pcr_cloud* cloud, int nb_neighbors, double std_ratio, uint8_t* keep, double* avg_dist,
                                double stats3[3], uint64_t* n_kept, pcr_cloud** kept_cloud);

/* ---- Homework4 foreground stage, second path: range-image clustering, Homework4/foreground_clustering_range.py ---------------
 * A pcr_range_image is an opaque, device-resident handle: the cropped f64 range image (-1 = empty pixel), its labels once
 * labelled and, for an image projected from a cloud, the pixel of every point.
 * pcr_range_image_create_f32 (pcd_to_range_image, :13-48), f64 on the cloud's f32 coordinates widened (what pcd_preprocessing
 * hands over), every operation rounded, unfused:
 *   res_rad = pi / 180 * resolution; width = floor(360 / resolution) + 1, height = floor(60 / resolution) + 1, offsets
 *   ceil(size / 2); d = sqrt((x*x + y*y) + z*z) (np.linalg.norm); alpha = atan2(y, x);
 *   beta = atan2(z, sqrt(x*x + y*y))   DIFFERS: :34 is math.asin(z, sqrt(...)), which raises TypeError (two arguments) — the
 *   reference's function cannot run; the two-argument form with the horizontal range second is atan2's;
 *   x = width - 1 - (floor(alpha / res_rad) + offset_width), y likewise from beta; an index in [-size, 0) wraps as numpy's
 *   negative indexing does.  A point with an index outside [-size, size) (the reference: IndexError) or a non-finite coordinate
 *   is DROPPED: pixel -1, label -1, counted in n_dropped.  The pixel's range is d of its HIGHEST point index (:38 in index
 *   order).  Rows without a point are removed, then columns without a point (:41-47); a point at the origin has range 0, which
 *   is neither empty nor ever labelled.  PCR_ERR_ARG for a resolution that is non-finite or <= 0 or gives more than 2^31 - 16
 *   pixels; PCR_ERR_EMPTY when no point lands in the image (an empty cloud included).
 * pcr_range_image_from_host_f64: the caller's rows x cols image as it is (no crop, no points; assign is then a no-op).
 * pcr_range_image_shape: rows / cols of the cropped image, the number of points and of dropped points (each optional).
 * pcr_range_image_read: the image (rows x cols f64) and the pixel of every point (r * cols + c, -1 = dropped), each optional.
 * pcr_range_image_close_f64 (depth_completion, :136-149), in place: dila[r, c] = max of the (2 pad + 1)^2 window for
 *   pad <= r < rows - pad, pad <= c < cols - pad, else -1; result = the same with min over dila.  NaN propagates as in
 *   np.amax / np.amin.  pad in 0 ... 16 (PCR_ERR_ARG).  Labels of an earlier call are dropped.
 * pcr_range_image_label_f64 (range_image_labeling, :51-95; phi, theta in degrees): phi_rad = phi * pi / 180, thr = theta * pi /
 *   180, sin(phi_rad) and cos(phi_rad) from the host's libm.  Two pixels are LINKED when both ranges are > 0, the second lies in
 *   the first's window (rows r - nn_mode .. r + nn_mode clipped to the image, columns c - nn_mode .. c + nn_mode wrapped ONCE
 *   around the image), and with d1 = max, d2 = min of the two ranges: fabs(d1 - d2) < 1 and
 *   atan2(d2 * sin(phi), d1 - d2 * cos(phi)) > thr.  The relation is symmetric.
 *   DIFFERS: image_label = the CONNECTED COMPONENTS of that relation, numbered 0, 1, ... by each component's first pixel in
 *   raster order; pixels with range <= 0 get -1.  The reference's flood fill assigns `[r, c] = queue[0]` (:66) and thereby
 *   overwrites the row variable of its own seed scan: for the rest of that row it scans a wrong row, so that some components
 *   are never seeded (all their pixels stay -1) and the numbers follow no raster order.  Relation to its output: on the
 *   pixels the reference labels, its labels and the components correspond one to one; every occupied pixel it leaves at -1
 *   lies in a component it labels nowhere (measured: 182 labels of 236 components on the 000099 foreground at (0.7, 30, 7)).
 *   Which components it drops depends on its FIFO order.
 *   PCR_ERR_ARG for theta outside [0, 90), nn_mode outside 1 ... 8, a non-finite phi, or an image narrower than nn_mode columns
 *   (single wrapping equals the reference only from that width on).  image_label (rows x cols int32) and n_labels are optional;
 *   the labels stay in the handle.  PCR_ERR_STATE if the union-find's bound is exceeded (never in a correct run).
 * pcr_range_image_assign (cluster_assignment, :124-133): cluster_idx[i] = image_label[pixel(i)], every point of a pixel, -1 for
 *   a dropped point.  PCR_ERR_STATE before a labelling.
 * pcr_range_cluster_f32: `__main__` :164-167 in one call — create(resolution), label(phi = resolution, theta, nn_mode), assign.
 *   stats4 (optional) = rows, cols of the cropped image, dropped points, pixels of the full image.
 * ROUNDING BAND.  Everything above is IEEE arithmetic both sides agree on bit for bit, except atan2: glibc documents an error
 *   of at most 1 ulp for its double atan2, the device library (OCML) is held to OpenCL's bound for double atan2, 6 ulp.  Hence
 *   two results for the same arguments lie within 7 ulp(a) <= 7 * 2^-52 |a| of each other.
 *   (1) pixel: q = fl(a / res_rad) adds half an ulp on either side: |q_dev - q_host| <= (7 + 1) * 2^-52 |q| = 2^-49 |q|.  A point
 *       with |q - round(q)| <= 2^-49 max(|q|, 1) for alpha or beta may land in the neighbouring pixel; all others are pinned.
 *   (2) edge: a pair with |angle - thr| <= 2^-49 max(angle, thr) may or may not be linked (the arguments of that atan2 are
 *       equal bit for bit); all others are pinned.  The library's partition then lies between the components of the certain
 *       links and those of the certain plus the in-band links.
 *   On the KITTI scans the points in band (1) are those with y = 0 or z = 0 exactly (atan2(+-0, x > 0) = +-0 on both sides, C Annex F). */
typedef struct pcr_range_image pcr_range_image;
int pcr_range_image_create_f32(pcr_ctx* ctx, const pcr_cloud* cloud, double resolution_deg, pcr_range_image** img);
int pcr_range_image_from_host_f64(pcr_ctx* ctx, const double* image, size_t rows, size_t cols, pcr_range_image** img);
int pcr_range_image_shape(const pcr_range_image* img, size_t* rows, size_t* cols, size_t* n_points, uint64_t* n_dropped);
int pcr_range_image_read(pcr_ctx* ctx, const pcr_range_image* img, double* image, int32_t* pixel);
int pcr_range_image_close_f64(pcr_ctx* ctx, pcr_range_image* img, int pad);
int pcr_range_image_label_f64(pcr_ctx* ctx, pcr_range_image* img, double phi_deg, double theta_deg, int nn_mode, int32_t* image_label,
                              uint64_t* n_labels);
int pcr_range_image_assign(pcr_ctx* ctx, const pcr_range_image* img, int32_t* cluster_idx);
int pcr_range_image_destroy(pcr_ctx* ctx, pcr_range_image* img);
int pcr_range_cluster_f32(pcr_ctx* ctx, const pcr_cloud* cloud, double resolution_deg, double theta_deg, int nn_mode, int32_t* cluster_idx,
                          uint64_t* n_clusters, uint64_t stats4[4]);

/* ---- Homework9 descriptors: FPFH33, getFPFH33Descriptors (Homework9/hw9/src/registration.cpp:254-269, PCL FPFHEstimationOMP) --
 * PCL is not pinned here: this is the library's own operation sequence, a restatement of PCL's FPFHEstimation.
 * Inputs: surface (n points), normals (one per surface point, a cloud whose x/y/z are normal_x/y/z, used as given, not
 * re-normalised), keypoints (m query points; NULL = the surface itself, m = n), radius.  All arithmetic below is unfused.
 * Neighbourhood (FLANN's radius search at dim 3): N(q) = { j in surface : s(q, j) < r2 }, STRICT, with
 *   s = ((dx*dx) + dy*dy) + dz*dz in f32 and r2 = (float)((double)radius * (double)radius).  A non-finite surface point is
 *   nobody's neighbour; a surface point is its own neighbour.
 * Pair features computePairFeatures(p1 = centre, n1, p2 = neighbour, n2), f32, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x):
 *   a pair with a non-finite normal at either end is skipped (the library's rule; PCL's behaviour there is undefined);
 *   dp = p2 - p1, f4 = sqrtf(dot(dp, dp)), skipped if f4 == 0; a1 = dot(n1, dp) / f4, a2 = dot(n2, dp) / f4;
 *   swap iff |a1| <= 1 && |a2| <= 1 && |a1| < |a2| (PCL: acos(|a1|) > acos(|a2|), NaN above 1): then exchange n1 and n2,
 *   negate dp and f3 = -a2, else f3 = a1;  v = cross(dp, n1), vn = sqrtf(dot(v, v)), skipped if vn == 0, v = v / vn (three
 *   divides);  w = cross(n1, v);  f2 = dot(v, n2);  f1 = (float)atan2((double)dot(w, n2), (double)dot(n1, n2)) (f64 atan2).
 * Bins (PCL's double arithmetic on the f32 features), each floor()ed and clamped to [0, 10] (NaN -> 0):
 *   b1 = 11 * (((double)f1 + M_PI) * (double)(1.0f / (2.0f * (float)M_PI))), b2 = 11 * (((double)f2 + 1.0) * 0.5), b3 the same on f3;
 *   the 33 slots are [f1 bins | f2 bins | f3 bins] (FPFHSignature33).
 * SPFH of surface point p: incr = 100.0f / (float)(|N(p)| - 1); every pair (p, j), j in N(p), j != p BY INDEX, that is not
 *   skipped adds incr to its three bins; a bin's value is incr added to 0.0f cnt times in f32 (equal addends: independent of
 *   order, equal to PCL's repeated +=).  A point with |N(p)| == 0 (non-finite) has an all-zero SPFH.
 * FPFH of keypoint q: for j in N(q) with s(q, j) != 0, w = 1.0f / s(q, j) (the SQUARED distance, as PCL's
 *   weightPointSPFHSignature), val_b = spfh_j[b] * w in f32; per sub-histogram acc_b and sum are accumulated in f64 and
 *   out_b = (float)(acc_b * (100.0 / sum)), or acc_b unchanged when sum == 0.  The keypoint's own SPFH is NOT added (PCL's
 *   behaviour, not the paper's nor Open3D's).  A non-finite keypoint or one with empty N(q) gets a row of NaN (PCL computeFeature).
 * Order: PCL accumulates the histogram in f32 in FLANN's distance order; here the f64 accumulation order is free (lanes of a
 *   group, then a fixed shuffle tree).  Promise: every run gives the same bits; results agree with the exact-order
 *   restatement (f64 in ascending-s order) to <= 1 f32 ulp per slot.  UNPINNED: PCL's f32 accumulation order and FLANN's strict
 *   `<`, which are restated here and not checked against PCL.
 * fpfh: m x 33 row-major (required); neighbor_counts (optional, m) = |N(q)|; spfh (optional, n x 33) = every surface point's SPFH.
 * PCR_ERR_ARG for a radius that is non-finite or <= 0, or a normal cloud whose size differs from the surface's; an empty
 * surface or no keypoints: PCR_OK with nothing written.  Tune key fpfh_lanes (lanes per query: 1, 2, 4, 8, 16, 32); profile
 * names fpfh_grid_build, fpfh_spfh, fpfh_weight. */
int pcr_fpfh33_f32(pcr_ctx* ctx, const pcr_cloud* surface, const pcr_cloud* normals, const pcr_cloud* keypoints, float radius, float* fpfh,
                   uint32_t* neighbor_counts, float* spfh);

/* ---- Homework9 keypoints: Harris3D, getHarris3DKeypoints (Homework9/hw9/src/registration.cpp:221-250, PCL HarrisKeypoint3D) -----
 * PCL is not pinned here: this is the library's own operation sequence, a restatement of PCL's
 * HarrisKeypoint3D<PointXYZ, PointXYZI> as hw9 configures it: normals supplied by the caller (setNormals), setRadius,
 * setThreshold, setNonMaxSupression, setRefine(false), default method HARRIS.  All f32 arithmetic below is unfused.
 * Inputs: cloud (n points), normals (one per point, a cloud whose x/y/z are normal_x/y/z, used as given).
 * Neighbourhood (the same as pcr_fpfh33_f32): N(i) = { j : s(i, j) < r2 }, STRICT, s = ((dx*dx) + dy*dy) + dz*dz in f32,
 *   r2 = (float)((double)radius * (double)radius).  A non-finite point is nobody's neighbour; a finite point is its own.
 * Normal moments (calculateNormalCovar): neighbour j contributes iff all three components of its normal are finite and of
 *   magnitude <= 2 (the library's rule; PCL tests normal_x only); count = the number of contributors.  For each of the six
 *   products xx, xy, xz, yy, yz, zz of a contributor's normal: p = fl32(a * b), q = rint(ldexp((double)p, 32)) (ties to
 *   even; an integer of magnitude <= 2^34), S = the sum of q over the contributors AS AN EXACT INTEGER, and the coefficient is
 *   c = (float)(((double)S * 0x1p-32) / (double)count); all six are 0 when count == 0.  This departs from PCL on purpose: PCL
 *   adds the f32 products in FLANN's distance order or in SSE lanes, depending on how it was built, so there is no single PCL
 *   answer to match; the integer sum does not depend on neighbour order, lanes per point, grid layout or input permutation.
 *   The quantisation is <= 2^-33 per coefficient.
 * Response (responseHarris): trace = (cxx + cyy) + czz; when trace != 0,
 *   det = cxx*cyy*czz + 2.0f*cxy*cxz*cyz - cxz*cxz*cyy - cxy*cxy*czz - cyz*cyz*cxx (left to right, as C parses it) and
 *   method 0 (HARRIS): response = (0.04f + det) - (0.04f * trace) * trace;  1 (NOBLE): det / trace;  2 (LOWE): det / (trace * trace);
 *   response = 0 when trace == 0 and for a non-finite point.  TOMASI, CURVATURE and setRefine(true) are not provided: any other
 *   method is PCR_ERR_ARG.
 * Keypoints (detectKeypoints): non_max_suppression != 0: is_key[i] = 1 iff point i is finite, response[i] is finite,
 *   !(response[i] < threshold), and no j in N(i) has response[i] < response[j] (strict: equal responses suppress nobody, so
 *   the result does not depend on the visiting order).  non_max_suppression == 0: is_key[i] = 1 for every finite point (PCL
 *   copies the whole response cloud and ignores the threshold).  PCL emits keypoints in OpenMP completion order; here the
 *   order is ascending input index.
 * UNPINNED (restated, not compared with PCL): FLANN's strict `<`; PCL's f32 accumulation order (replaced by the integer sum
 *   above); the response formula 0.04f + det - 0.04f * trace * trace of PCL 1.8-1.12's harris_3d.hpp.
 * is_key: n bytes (required); response (optional, n floats), neighbor_counts (optional, n) = |N(i)|, n_keypoints (optional) the
 * number of ones.  PCR_ERR_ARG for a NULL context / cloud / normals / params / is_key, a radius that is non-finite or <= 0, a NaN
 * threshold, a normal cloud of another size; an empty cloud: PCR_OK with nothing written.  Tune key harris_lanes (lanes per
 * point: 1, 2, 4, 8, 16, 32); profile names harris_grid_build, harris_response, harris_nms. */
typedef struct {
    float radius;
    float threshold;
    int method;                  /* 0 HARRIS, 1 NOBLE, 2 LOWE */
    int non_max_suppression;
} pcr_harris3d_params;
int pcr_harris3d_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_cloud* normals, const pcr_harris3d_params* prm, uint8_t* is_key,
                     float* response, uint32_t* neighbor_counts, uint64_t* n_keypoints);

/* ---- Homework9, the front of the flow: readBinaryAndVoxelDown (Homework9/hw9/src/registration.cpp:8-68) and VoxelGridSampling
 * (:665-707) — pcl::VoxelGrid<pcl::PointNormal> over points AND normals -----------------------------------------------------------
 * PCL is not pinned here: this is the library's own operation sequence, a restatement of PCL 1.8-1.12 voxel_grid.hpp::applyFilter
 * with one leaf size for the three axes, setDownsampleAllData(true), no field filter, min_points_per_voxel 0.  (pcr_voxel_filter_f32
 * above is Homework1's script: another lattice — anchored at the cloud's minimum — xyz only, last voxel dropped.)  All f32
 * arithmetic below is unfused.
 * Inputs: cloud (n points), normals (NULL, or one per point: a cloud whose x/y/z are normal_x/y/z), leaf, normal_mode.
 * Lattice: inv = 1.0f / leaf (f32); per axis c = (int)floorf(fl32(x * inv)); a point with a non-finite coordinate is SKIPPED (hw9
 *   sets is_dense = true, so PCL does not look).  min_b / max_b = min / max of c over the other points, div = max_b - min_b + 1,
 *   voxel id = (cx - min_bx) + (cy - min_by) * div_x + (cz - min_bz) * div_x * div_y  (int64).
 * Output: one row per occupied voxel in ASCENDING VOXEL ID (PCL's order), the last one included; m rows.
 * Centroid: E = the smallest integer >= -149 such that every coordinate of a point that is not skipped has |coordinate| < 2^E.  Each
 *   f32 coordinate v becomes the integer q = rint(ldexp((double)v, 32 - E)) (ties to even, |q| <= 2^32), S = the sum of q over the
 *   voxel's points AS AN EXACT INTEGER (int64: n <= 2^31 - 16), and the output is (float)(((double)S * 2^(E - 32)) / (double)count).
 *   The quantisation is <= 2^(E - 33) per component of the mean, before the one rounding to f32.
 * Normal: the same form with E = 2 fixed: a normal contributes iff its three components are finite and of magnitude <= 2 (the rule
 *   of pcr_harris3d_f32), q = rint(ldexp((double)v, 30)), mean = (float)(((double)S * 2^-30) / (double)count_n) with count_n the
 *   number of contributing normals of the voxel; (0, 0, 0) when count_n == 0.  A point whose normal does not contribute still counts
 *   for the centroid.  Quantisation <= 2^-31 per component.
 *   normal_mode 0: the mean.  normal_mode 1: the mean scaled to unit length in f32, len = sqrtf((nx*nx + ny*ny) + nz*nz), each
 *   component divided by len; left as it is when len == 0.  hw9's stage is mode 1.
 * This departs from PCL on purpose: PCL adds the f32 values of a voxel in the order std::sort (unstable) leaves them in, so there
 *   is no single PCL answer to match; the integer sums do not depend on the order of the points, on how the work is split over
 *   lanes or on the launch geometry.  Promise: the outputs are a function of the SET of (point, normal) pairs — the same bits for
 *   any permutation of the input (rows are keyed by voxel id) and on every run.
 * UNPINNED (restated, not compared with PCL): the lattice arithmetic above as PCL 1.8-1.12 write it; that PCL's CentroidPoint
 *   normalises an accumulated normal (accumulators.hpp, from memory — which is why normal_mode is a parameter); PCL's f32
 *   accumulation order (replaced by the integer sums).
 * out_cloud (required) / out_normals (required iff normals != NULL): new device clouds of m points, the caller's to destroy.
 * voxel_of_point (optional, n int32, host): the output row of every input point, -1 for a skipped point.  counts (optional, host,
 * room for n entries, the first m written): points per voxel.  n_voxels (optional): m.
 * PCR_ERR_ARG: NULL ctx / cloud / out_cloud; a leaf that is non-finite or <= 0 or whose f32 reciprocal is infinite; a normal_mode
 * other than 0 / 1; a normal cloud of another size or without out_normals; n > 2^31 - 16; a voxel coordinate outside int32 or
 * div_x * div_y * div_z > INT32_MAX (PCL prints a warning and returns its input).  Empty input, or no finite point: PCR_OK, m = 0.
 * Profile names vgn_bounds, vgn_keys, vgn_sort, vgn_segments, vgn_accum, vgn_finalize. */
int pcr_voxel_grid_normals_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_cloud* normals, float leaf, int normal_mode,
                               pcr_cloud** out_cloud, pcr_cloud** out_normals, int32_t* voxel_of_point, uint32_t* counts, uint64_t* n_voxels);

/* ---- Homework9, in front of ICP: normalSpaceSampling (Homework9/hw9/src/registration.cpp:630-662, called at :728-729 / :880-881) ---
 * PCL is not pinned here: this is the library's own operation sequence, a restatement of PCL's NormalSpaceSampling (normal_space.hpp).
 * Inputs: normals (n, a cloud whose x/y/z are normal_x/y/z), bins[3], sample, seed.  hw9: bins 10 x 10 x 10, sample 4 000, seed 0.
 * Bin of point i (f32, unfused): ix = roundf((0.5f * (bins_x - 1.f)) * (nx + 1.f)) (half away from zero), clamped to [0, bins_x - 1]
 *   as a float before the conversion to unsigned; the same for y and z; bin = ix * (bins_y * bins_z) + iy * bins_z + iz.  A point
 *   whose normal has a non-finite component is never sampled; n_valid = the number of the others.
 * sample >= n_valid: every samplable point, in ascending index (PCL returns its index list unchanged).
 * Otherwise PCL goes round the bins in ascending bin order and draws from each bin that is not exhausted one member not yet drawn,
 *   uniformly at random, until `sample` points are out.  The order-free form of that, which is the contract: point i has the key
 *     z = seed ^ (0x9E3779B97F4A7C15 * (i + 1));  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     k(i) = z ^ (z >> 31)                       (uint64 arithmetic modulo 2^64: SplitMix64's output function on seed ^ golden * (i + 1))
 *   inside a bin the members are ranked by (k, i) ascending -> rank r = 0, 1, ...; the output is the first `sample` points in
 *   ascending (r, bin), in that order.  Within a bin this is a uniform draw without replacement, across bins it is PCL's round-robin.
 * The result depends on (normals, bins, sample, seed) only, not on lanes or launch geometry.
 * UNPINNED: the random STREAM is not PCL's (boost::mt19937 through `% size` with rejection of members already drawn), so the points
 *   drawn differ from PCL's for the same seed; PCL's bin formula and its clamping of out-of-range normals are restated, not compared.
 * indices (host, room for min(sample, n) entries; may be NULL when that is 0): the first *n_out = min(sample, n_valid) written.
 * gather_cloud + out_cloud (optional, together; gather_cloud has n points): a new device cloud of gather_cloud's points at the
 * indices, in their order; out_normals (optional): the same of the normals — so that ICP takes both without a host round trip.
 * PCR_ERR_ARG: NULL ctx / normals / bins / n_out; a bin count < 1 or a product of the three > 2^20; gather_cloud without out_cloud
 * or the reverse, or of another size; n > 2^31 - 16.  Profile names nss_keys, nss_sort, nss_rank, nss_gather. */
int pcr_normal_space_sample_f32(pcr_ctx* ctx, const pcr_cloud* normals, const uint32_t bins[3], size_t sample, uint64_t seed, uint32_t* indices,
                                size_t* n_out, const pcr_cloud* gather_cloud, pcr_cloud** out_cloud, pcr_cloud** out_normals);

/* ---- HomeworkFinal: the sampling and grouping front of PointNet++ (HomeworkFinal/models/pointnet_util.py:66-156) and the object
 * extraction loop of HomeworkFinal/foreground_obj_cls.py:143-180 ------------------------------------------------------------------------
 * The three operators work on SEGMENTS of one cloud: seg_ptr[n_seg + 1] (host) holds ascending offsets into the cloud, segment s is
 * the points [seg_ptr[s], seg_ptr[s + 1]).  A PointNet batch [B, N, 3] is seg_ptr[b] = b * N; the objects of a scan are the ragged case.
 * Every index returned is SEGMENT-LOCAL (the reference's are batch-local).  All arithmetic below is unfused.
 *
 * pcr_fps_f32 — farthest point sampling, two arithmetic modes over the same f32 coordinates:
 *   PCR_FPS_F32  pointnet_util.farthest_point_sample (:66-87, torch f32): s = ((dx*dx) + dy*dy) + dz*dz in f32, d = p - centre,
 *                running distance starts at 1e10f;
 *   PCR_FPS_F64  DataLoader.farthest_point_sample (HomeworkFinal/data_utils/DataLoader.py:17-38, numpy f64 on widened f32 points):
 *                the same expression in f64 on the coordinates widened to f64, running distance starts at 1e10.
 *   The two modes are two contracts: on real neighbourhoods they pick different sequences now and then.
 *   Rule (both): pick[0] = start[s] (an input: the reference draws it unseeded); for k >= 1: every point's running distance becomes s
 *   when s < distance (strict), then pick[k] = the point with the LARGEST running distance, ties to the LOWEST index (np.argmax /
 *   torch.max return the first maximum).  npoint larger than the segment is legal and follows from the rule: once every distance is 0
 *   the argmax is index 0.  A point with a non-finite coordinate is never picked by the rule: its running distance counts as -inf and is
 *   never updated (so a NaN cannot be chosen forever); start[s] itself is returned as given.  When every running distance is -inf — a
 *   segment with no finite point — every pick after the first is index 0.  A non-finite CENTRE updates nobody (s is NaN or +inf).
 *   indices: n_seg x npoint (host); regime (optional, n_seg bytes): which kernel served the segment — 1 one wave (<= 256 points, no barrier
 *   in the loop), 2 / 3 / 4 one workgroup holding 4 x 256 / 4 x 1024 / 16 x 1024 points in registers, 5 one launch per pick (any size).
 *   Tune key fps_regime [0] r = no segment is served by a regime below r (results never depend on it).  Profile names fps_small, fps_large.
 *   PCR_ERR_ARG: NULL ctx / cloud / seg_ptr, or start / indices with something to do; another mode; a seg_ptr that descends or ends
 *   beyond the cloud; start[s] outside its segment (so: an EMPTY segment with npoint > 0); n_seg x npoint > 2^31 - 16.  n_seg == 0 or
 *   npoint == 0: PCR_OK, nothing written.  PCR_ERR_STATE if a pick lies outside its segment (never in a correct run).
 *
 * pcr_ball_query_f32 — pointnet_util.query_ball_point (:90-116).  centres is a second segmented cloud (centre_seg_ptr, the same n_seg);
 *   its points need not be members of the first.  For every centre q of segment s: the hits are the points j of segment s with
 *   s(q, j) <= r2, s = ((dx*dx) + dy*dy) + dz*dz in f32 computed DIRECTLY from d = q - p (the reference expands -2 q.p + |q|^2 + |p|^2
 *   through a matmul: the two forms can differ for a pair whose distance is within rounding of the radius), r2 = (float)(radius * radius)
 *   with the product in f64 (what comparing an f32 tensor with the Python float radius ** 2 does).  A comparison with NaN is false: a
 *   non-finite point is never a hit and a non-finite centre has none.  Row q = the first nsample hits in ascending index, the rest of
 *   the row filled with the first hit; an EMPTY row is filled with the segment's size N, as the reference leaves it.  counts (optional)
 *   = min(hits seen, nsample) per row — the walk stops at the chunk of 64 points that fills the row — 0 for an empty row.
 *   idx: (number of centres) x nsample, rows in centre order starting at centre_seg_ptr[0].  PCR_ERR_ARG: NULL ctx / clouds / seg_ptrs / idx;
 *   nsample == 0; a radius that is negative or non-finite; a seg_ptr that descends or ends beyond its cloud.  Profile name ball_query.
 *
 * pcr_group_points_f32 — the gather of pointnet_util.sample_and_group (:145-150) in one pass: new_xyz[q] = centre q (rows x 3) and
 *   new_points[q][k] = (xyz[idx[q][k]] - centre q | features[idx[q][k]]), rows x nsample x (3 + D), one f32 subtraction per coordinate
 *   (bit-exact against torch).  features: host, one row of D floats per point of the CLOUD (addressed by cloud position; only the rows of
 *   the segments are read), NULL with D == 0.  idx: host, segment-local, rows x nsample.  PCR_ERR_ARG as above, and for an index outside
 *   its segment — which is what an empty ball-query row holds: the reference's indexing raises there too.  Profile name group_points.
 *
 * pcr_objects_from_labels_f32 — the loop of foreground_obj_cls.py:143-180 in one call.  labels: n int32 (host), -1 = noise, else a cluster
 *   id < n_clusters (pcr_dbscan_f32's output).  Members of a cluster are taken in ascending input index (cluster_indices_dict's order: a
 *   STABLE sort by label).  Per cluster c: size, z_min, z_max (f32, exact) and the class code
 *     3   when the cluster is empty, or (double)z_min - ground_z > z_min_above_ground (:162), or e = (double)z_max - (double)z_min has
 *         e < z_extent[0] or e > z_extent[1] (:167) — the reference writes 3 there and goes on;
 *     -1  "to be classified": the cluster gives one object row.
 *   Object rows come in ascending cluster id (the reference walks its dict in order of first appearance and keys its result by cluster).
 *   A row has npoints members (member = position inside the cluster):
 *     size > npoints: PCR_FPS_F64 picks with pick[0] = starts[c] when starts != NULL and starts[c] != UINT32_MAX, else
 *         K(seed, (c + 1) << 32) mod size;
 *     size <= npoints: members 0 .. size - 1, then for t = 0 .. npoints - size - 1 member K(seed, (c + 1) << 32 | (t + 1)) mod size (a draw with
 *         replacement, :177);
 *     K(seed, a): z = seed ^ (0x9E3779B97F4A7C15 * (a + 1)); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *         K = z ^ (z >> 31) (uint64 arithmetic modulo 2^64: the keying of pcr_normal_space_sample_f32).  A draw depends on (seed, c, t) only,
 *         never on lanes or launch geometry.
 *   Centroid (pc_normalize, :24-29): per coordinate the f64 sum of the npoints rows IN ROW ORDER starting from 0.0, divided by npoints;
 *   objects[row][t] = (float)((double)p - centroid): rounded to f32 once, as `input[0, ...] = torch.from_numpy(obj_pts)` does (:183).
 *   UNPINNED: the reference's draws (np.random.randint / np.random.choice, unseeded) — the stream here is the library's own; with
 *   explicit starts the FPS rows are the reference's.
 *   objects: room for n_clusters x npoints x 3 floats, object_cluster: n_clusters (the cluster of each row), source_index (optional): n_clusters x
 *   npoints (the cloud index of every row member); the first *n_objects rows are written.  codes: n_clusters; z_min_max (optional): n_clusters x 2
 *   ((+inf, -inf) for an empty cluster); sizes (optional): n_clusters.  PCR_ERR_ARG: NULL ctx / cloud / labels / z_extent / n_objects / objects /
 *   object_cluster / codes; a label outside [-1, n_clusters); npoints outside [1, 4096]; a NaN gate; a start outside its cluster.
 *   Profile names obj_sort, obj_zstats, obj_build (+ fps_*). */
enum pcr_fps_mode { PCR_FPS_F32 = 0, PCR_FPS_F64 = 1 };
int pcr_fps_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg, size_t npoint, int mode, const uint32_t* start,
                uint32_t* indices, uint8_t* regime);
int pcr_ball_query_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                       size_t n_seg, double radius, size_t nsample, uint32_t* idx, uint32_t* counts);
int pcr_group_points_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                         size_t n_seg, const float* features, size_t D, const uint32_t* idx, size_t nsample, float* new_xyz, float* new_points);
int pcr_objects_from_labels_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels, size_t n_clusters, size_t npoints, double ground_z,
                                double z_min_above_ground, const double z_extent[2], uint64_t seed, const uint32_t* starts, float* objects,
                                uint32_t* object_cluster, uint32_t* source_index, int32_t* codes, float* z_min_max, uint32_t* sizes, size_t* n_objects);

/* ---- HomeworkFinal: the two box operators — the points inside ORIENTED boxes (dataset_building/dataset_build.py:97-125, Open3D's
 * OrientedBoundingBox::GetPointIndicesWithinBoundingBox) and the AXIS-ALIGNED box of every cluster (foreground_obj_cls.py:190-199) -------
 * pcr_obox: centre, R row-major whose COLUMN a is box axis a, extent = the full edge lengths along the three axes.
 *
 * pcr_points_in_boxes_f64 — many points against a few boxes, on SEGMENTS as pcr_ball_query_f32: segment s of the cloud, the points
 *   [seg_ptr[s], seg_ptr[s + 1]), is tested against the boxes [box_seg_ptr[s], box_seg_ptr[s + 1]) only (a batch of frames is one call; boxes
 *   holds box_seg_ptr[n_seg] entries, n_boxes below).  Every index returned is SEGMENT-LOCAL.
 *   Membership: point p (the f32 coordinates widened to f64) is inside box b iff |t_a| <= extent[a] * 0.5 for a = 0, 1, 2, with d = p - centre
 *   and t_a = (d0*R[0][a] + d1*R[1][a]) + d2*R[2][a], every operation rounded, unfused, left to right: the CLOSED box of Open3D.  A comparison
 *   with NaN is false: a non-finite point is in no box, and a box with a non-finite field (centre, R or extent) holds nothing.  R is used as
 *   given (orthonormality is not checked).  extent[a] == 0 is legal: a rectangle, which holds the points exactly on it.
 *   row_ptr: n_boxes + 1 (host), ALWAYS written: row b of idx is [row_ptr[b], row_ptr[b + 1]) = the members of box b in ASCENDING index (the
 *   order of Open3D's loop, so points[idx] is the instance dataset_build.py writes).  hits (optional): one entry per point OF THE CLOUD, the
 *   number of boxes of its segment that hold it (0 for a point in no segment): hits == 0 is the mask of other_obj_idx.  total (optional) =
 *   row_ptr[n_boxes].  When idx_cap < total, idx is left alone and the call returns PCR_ERR_ARG with row_ptr, hits and total valid (the
 *   convention of pcr_s3_walk_visits): idx == NULL with idx_cap == 0 is the counting call.
 *   The rows are the same bits in the same order under any launch geometry: a position is a prefix sum of ballot popcounts, never the
 *   outcome of an atomic.  Tune key pib_tile [512]: the points per workgroup, clamped to 64 ... 2048 and rounded down to a multiple of 64
 *   (results never depend on it).  Profile names pib_count, pib_scan, pib_fill.
 *   PCR_ERR_ARG: NULL ctx / cloud / seg_ptr / box_seg_ptr / row_ptr, or boxes with n_boxes > 0, or idx with total > 0 and room for it; a seg_ptr
 *   that descends or ends beyond the cloud, a box_seg_ptr that descends; a negative extent; more than 2^31 - 16 points or boxes, or
 *   sum over segments of (boxes x ceil(points / pib_tile)) beyond that.  n_seg == 0 or no boxes: PCR_OK, row_ptr all zero, hits all zero.
 *   PCR_ERR_STATE for a row_ptr that descends (never in a correct run).
 *
 * pcr_label_aabb_f32 — per cluster id c < n_clusters the exact f32 minimum and maximum of x, y, z over the points with labels[i] == c, and
 *   the member count; labels: n int32 (host) as pcr_dbscan_f32 writes them, -1 (noise) is skipped.  aabb: n_clusters x 6 =
 *   (min x, min y, min z, max x, max y, max z), which is AxisAlignedBoundingBox.create_from_points's (min_bound, max_bound); counts
 *   (optional): n_clusters.  The library's own rules where the reference has none: an EMPTY cluster gives (+inf, -inf) in every coordinate;
 *   a NaN coordinate is skipped IN THAT COORDINATE (fminf / fmaxf; the point still counts as a member), so a coordinate that is NaN in every
 *   member also gives (+inf, -inf); -0 orders below +0.  Min and max do not depend on order: the same bits for any permutation of the input
 *   and any launch geometry.  PCR_ERR_ARG: NULL ctx / cloud / labels / aabb with something to do; a label outside [-1, n_clusters);
 *   n > 2^31 - 16.  n_clusters == 0: PCR_OK, nothing written.  Profile name label_aabb. */
typedef struct pcr_obox {
    double centre[3];
    double R[9];
    double extent[3];
} pcr_obox;
int pcr_points_in_boxes_f64(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg, const pcr_obox* boxes,
                            const uint32_t* box_seg_ptr, uint64_t* row_ptr, uint32_t* idx, size_t idx_cap, uint32_t* hits, uint64_t* total);
int pcr_label_aabb_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels, size_t n_clusters, float* aabb, uint32_t* counts);

/* ---- Homework6: the KITTI object evaluator, Homework6/devkit_object/cpp/evaluate_object.cpp — box overlaps, computeStatistics, AP curves ----
 * All arithmetic is f64, every operation rounded, unfused.  Boxes travel as flat rows of 15 doubles with per-frame row_ptr arrays of
 * n_frames + 1 uint64 entries (row_ptr[0] == 0, ascending; at most 2^22 rows of a kind in one call).
 *   ground-truth row: class code, truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry       (loadGroundtruth's fscanf order)
 *   detection row:    class code, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score, one pad              (loadDetections' order)
 *   class codes: 0 Car, 1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else (names are matched in Python, hw6.py).
 * metric: PCR_KITTI_IMAGE / GROUND / BOX3D.  criterion: -1 union, 0 over the detection, 1 over the ground truth.  difficulty 0 / 1 / 2.
 *
 * The overlap of (detection d, ground truth g):
 *   IMAGE   imageBoxOverlap(d, g, criterion) with the reference's operations in its order (:230-264).
 *   GROUND  Both quads are formed as toPolygon forms them (:272-294): with c = cos(ry), s = sin(ry), corner i = (c X_i + s Z_i + t1,
 *           -s X_i + c Z_i + t3) for (X, Z) = (l/2, w/2), (l/2, -w/2), (-l/2, -w/2), (-l/2, w/2).  c and s are computed ON THE HOST (std::cos,
 *           std::sin, in csrc/kitti_eval.hip's prepare step) — nowhere else, so the device does plain arithmetic and a matrix does not depend on
 *           launch geometry.  The INTERSECTION follows a rule of our own (boost::geometry is not reproduced):
 *             sgn = -1 if the ground-truth quad's fan sum sum_{k=1,2} cross(g_k - g_0, g_{k+1} - g_0) is negative, else +1;
 *             the detection quad V (4 vertices, corner order) is clipped by ground-truth edge e = 0 ... 3 (g_e -> g_{e+1 mod 4}) in turn:
 *               d_k = sgn * (ex * (V_k.z - g_e.z) - ez * (V_k.x - g_e.x)), (ex, ez) = g_{e+1} - g_e; a vertex is inside iff d_k >= 0;
 *               for k = 0 ... n-1 with P = V_k, Q = V_{k+1 mod n}: P is kept if inside, then, if exactly one of P, Q is inside, the point
 *               I + (O - I) * (d_I / (d_I - d_O)) follows, I the inside one of the two and O the other (a vertex ON the edge is thus
 *               returned exactly, and boxes that only touch intersect in 0).  At most 8 vertices result (they are kept in registers).
 *             area = | 0.5 * sum_{k=1}^{n-2} ( (V_k.x - V_0.x)(V_{k+1}.z - V_0.z) - (V_{k+1}.x - V_0.x)(V_k.z - V_0.z) ) |: the shoelace sum in
 *             vertex order, taken about vertex 0 so that its rounding does not grow with the distance from the origin; 0 for n < 3.
 *           overlap = inter / (area_d + area_g - inter), inter / area_d or inter / area_g with area = |l * w|.  DEPARTURE from the reference:
 *           it divides by the area of boost's union_ polygon; the two agree up to rounding for proper boxes.
 *   BOX3D   box3DOverlap as written (:320-347): ymax = min(d.t2, g.t2), ymin = max(d.t2 - d.h, g.t2 - g.h), inter_vol = inter *
 *           max(0, ymax - ymin), volumes h * l * w (signed, as there), inter_vol / (det_vol + gt_vol - inter_vol) for the union.
 *   A 0 / 0 (a zero-area detection under criterion 0) is NaN and matches nothing: every comparison is written as the reference writes it.
 *
 * pcr_box_overlap_f64 — one launch, one (ground truth, detection) pair per lane over all frames: frame f's matrix is out[mat_ptr[f] + i * nd_f
 *   + j] for ground truth i and detection j of the frame.  mat_ptr (n_frames + 1, host) is always written; out_cap < mat_ptr[n_frames]:
 *   PCR_ERR_ARG with mat_ptr valid (out == NULL, out_cap == 0 is the sizing call).  Profile name kitti_overlap.
 * pcr_kitti_clean_data_f64 — cleanData's codes (:384-457) for one frame, host only (no context): ignored_gt / ignored_det in {0, 1, -1} and
 *   the count of valid ground truth.  int32_t height = fabs(y1 - y2) truncates for detections, height <= MIN_HEIGHT in double for ground
 *   truth; Van for Car and Person_sitting for Pedestrian are neighbour classes.  DontCare areas are the rows of class code 5.
 * pcr_kitti_frame_stats_f64 — computeStatistics (:459-617) for every frame under one (class, metric, difficulty).  compute_fp != 0: for each
 *   of n_thresholds <= 41 thresholds, tp / fp / fn / similarity [n_frames][n_thresholds]; similarity is the frame's sum of (1 + cos(delta)) / 2
 *   in ground-truth order, -1 for a frame without tp and fp, 0 when compute_aos == 0.  compute_fp == 0 (the collecting mode): tp / fp / fn
 *   [n_frames] and tp_scores (as many doubles as ground-truth rows): frame f's true-positive scores, in the reference's push order, are
 *   tp_scores[gt_ptr[f] ... gt_ptr[f] + tp[f]); the rest is NaN.  One wave works one frame, lane t carries threshold t; assigned_detection is
 *   a register bitmask up to 64 detections and spills to lane-interleaved words in device memory beyond: any number of detections in a frame.
 *   Profile names kitti_collect / kitti_match.
 * pcr_kitti_thresholds_f64 — getThresholds (:349-382) on the device: thresholds[count <= 41].  Which sorted positions the recall walk keeps
 *   depends on (n, n_gt) alone; each kept position receives the score of that descending rank (ties: equal values, so the reference's picks).
 *   A NaN score is PCR_ERR_ARG.  Profile name kitti_thresholds.
 * pcr_kitti_eval_f64 — eval_class (:623-707) for all 3 metrics x 3 difficulties of one class in ONE call with ONE host wait: out[metric * 3 +
 *   difficulty].  Overlaps (three launches), the collecting pass, the thresholds and the matching pass of all nine run back to back on the
 *   stream.  tp / fp / fn are summed over frames with integer atomics; the similarity of every frame is rounded to the grid 2^-40 and summed
 *   as an integer too (no floating-point atomic: the same bits for any frame order, chunking or launch geometry; the rounding is at most
 *   2^-41 per frame, so aos moves by less than 4.6e-13).  precision[t] = tp / (tp + fp), aos[t] = similarity / (tp + fp) (IMAGE only, and
 *   only if compute_aos), both replaced by their running maximum from the right over all 41 entries; entries beyond n_thresholds stay 0.
 *   Tune key kitti_blocks [2048]: the cap on the workgroups of each launch (results never depend on it).
 * Empty frames and empty inputs are valid everywhere.  PCR_ERR_ARG: a NULL that is needed, a class outside 0 ... 2, a metric, criterion or
 *   difficulty out of range, a row_ptr that does not start at 0, descends or ends beyond 2^22, more than 41 thresholds. */
#define PCR_KITTI_IMAGE 0
#define PCR_KITTI_GROUND 1
#define PCR_KITTI_BOX3D 2
#define PCR_KITTI_SAMPLE_PTS 41
typedef struct pcr_kitti_curve {
    uint64_t n_gt;
    int32_t n_thresholds;
    int32_t has_aos;
    double thresholds[PCR_KITTI_SAMPLE_PTS];
    int64_t tp[PCR_KITTI_SAMPLE_PTS], fp[PCR_KITTI_SAMPLE_PTS], fn[PCR_KITTI_SAMPLE_PTS];
    double similarity[PCR_KITTI_SAMPLE_PTS];
    double precision[PCR_KITTI_SAMPLE_PTS], aos[PCR_KITTI_SAMPLE_PTS];
} pcr_kitti_curve;
int pcr_box_overlap_f64(pcr_ctx* ctx, int metric, int criterion, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows,
                        const uint64_t* det_ptr, size_t n_frames, uint64_t* mat_ptr, double* out, size_t out_cap);
int pcr_kitti_clean_data_f64(int cls, int difficulty, const double* gt_rows, size_t n_gt_rows, const double* det_rows, size_t n_det_rows,
                             int32_t* ignored_gt, int32_t* ignored_det, uint64_t* n_gt);
int pcr_kitti_frame_stats_f64(pcr_ctx* ctx, int cls, int metric, int difficulty, int compute_fp, int compute_aos, const double* thresholds,
                              size_t n_thresholds, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows, const uint64_t* det_ptr,
                              size_t n_frames, int32_t* tp, int32_t* fp, int32_t* fn, double* similarity, double* tp_scores);
int pcr_kitti_thresholds_f64(pcr_ctx* ctx, const double* scores, size_t n, uint64_t n_gt, double* thresholds, int32_t* count);
int pcr_kitti_eval_f64(pcr_ctx* ctx, int cls, int compute_aos, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows,
                       const uint64_t* det_ptr, size_t n_frames, pcr_kitti_curve* out);

/* ---- HomeworkFinal: the PointNet++ (SSG) classifier, HomeworkFinal/models/pointnet2_cls_ssg.py + pointnet_util.py:159-215, eval mode -----------
 * A model is a chain of up to 4 set-abstraction (SA) layers and up to 4 fully connected (FC) layers, described by pcr_pn2_desc:
 *   D0         feature channels of the input besides xyz (0: xyz only, 3: normal_channel)
 *   sa[l]      npoint, radius, nsample (sampling layers), group_all (0 / 1), n_mlp in 1 ... 4 shared-MLP widths.  The input of an SA layer has
 *              3 + D channels, xyz FIRST (torch.cat([grouped_xyz_norm, grouped_points]), pointnet_util.py:150), D = D0 or the width the layer
 *              before ends in; a group_all layer takes xyz un-centred (:173) and makes ONE group of all points of a segment.  Only the LAST
 *              SA layer may be group_all, and pcr_pn2_forward_f32 needs it to be (the head reads one row per object).
 *   fc_widths  n_fc in 1 ... 4 output widths; the input of the head is the last SA layer's last width; every FC layer but the last carries
 *              BatchNorm + ReLU (dropout is the identity in eval mode); the last width is the number of classes.
 *   bn_eps     BatchNorm's eps (torch: 1e-5)
 * weights: ONE flat f32 array, layer after layer in the order SA 0 (its convolutions in order) ... SA n_sa - 1, FC 0 ... FC n_fc - 1; per
 *   convolution / linear layer: W [out][in] row-major, bias [out], then — where the layer has BN (every convolution, every FC but the last) —
 *   gamma [out], beta [out], running_mean [out], running_var [out].  pcr_pn2_model_info reports the length this adds up to.
 * BN is folded on the host in f64 and rounded to f32 ONCE, at pcr_pn2_model_create: s = gamma / sqrt(var + eps), W' = s W,
 *   b' = (b - mean) s + beta.  The device copy holds W' with K zero-padded to 16 (four K steps of the MFMA), in the operand order of the kernel.
 * Arithmetic of every layer: out[n] = relu(c_K), c_0 = b'[n], c_(k+1) = fmaf(x[k], W'[n][k], c_k) for k = 0 ... K - 1 ASCENDING input channel —
 *   ONE f32 fma chain per output that STARTS FROM THE BIAS IN THE ACCUMULATOR (not: the bias added after the chain).  It runs on
 *   v_mfma_f32_16x16x4_f32, which is bit for bit that chain; the zero padding adds fmaf(0, 0, c) = c.  relu(v) = v > 0 ? v : +0.  The last FC
 *   layer has no ReLU.  So a row's result does not depend on the tile geometry, on the other rows of the call, or on the workgroup that served it.
 * Limits (PCR_ERR_ARG otherwise): n_sa in 1 ... 4, n_mlp in 1 ... 4, n_fc in 1 ... 4, every width and 3 + D0 in 1 ... 1024; a sampling layer
 *   has npoint >= 1, nsample in 1 ... 65536 and a finite radius >= 0; group_all only on the last SA layer; bn_eps finite; n_weights equal to the
 *   model's count; every weight finite; var + eps > 0.
 *
 * pcr_sa_mlp_max_f32 — ONE fused launch for SA layer `layer` of the model: per group gather the nsample members (idx, segment-local, as
 *   pcr_ball_query_f32 returns them), subtract the centre (one f32 subtraction, as pcr_group_points_f32), run the layer's MLP chain, take the
 *   max over the group's samples.  The activations of a row tile stay in LDS; nothing of size rows x nsample x C goes to memory.  Arguments as
 *   in pcr_group_points_f32 (features: host, one row of D floats per point of the cloud, D = the layer's input channels - 3; NULL with D == 0);
 *   for a group_all layer centres, centre_seg_ptr and idx are NULL and every segment is one group (an empty segment gives a row of zeros).
 *   out: rows x C_out f32 (host), rows = number of centres, or n_seg for group_all.  Tune key pn2_rows [0 = the largest that fits in LDS]
 *   16 / 32 / 64 rows per workgroup tile (results never depend on it; a value that does not fit falls back to the largest that does).
 *   PCR_ERR_ARG as pcr_group_points_f32, and for a layer outside the model or centres / idx that do not go with its group_all flag.
 *   Profile name pn2_sa.
 *
 * pcr_pn2_forward_f32 — the whole forward pass for n_obj objects of npts points each.  objects: host, n_obj x npts x (3 + D0), uploaded once.
 *   Per sampling layer l (cloud = the input points, then the centres of the layer before): pcr_fps_f32's rule in PCR_FPS_F32 mode ->
 *   centres = the picked points -> pcr_ball_query_f32's rule -> the fused kernel; the group_all layer; then the head through the same chain
 *   kernel and log_softmax in f32, x - m - log(sum exp(x - m)), m = max, the sum in ascending class order.
 *   starts (optional): n_sampling_layers x n_obj first picks, each below the layer's cloud size (npts, then npoint of the layer before).  NULL:
 *   K(seed, (layer + 1) << 32 | obj) mod that size with the SplitMix keying above.  UNPINNED: the reference's unseeded torch.randint.
 *   logp: n_obj x n_class; pred (optional): the FIRST maximum of a row, as max(1)[1]; global_feat (optional): n_obj x C_last, the reference's
 *   l3_points; fps_idx (optional): the picks of the sampling layers one block after the other, block l = n_obj x npoint_l (object-local).
 *   The stages hand device buffers to each other; the number of launches depends on the model and on npts, not on n_obj; the host waits once,
 *   at the end.  n_obj == 0: PCR_OK, nothing written.  PCR_ERR_ARG: NULL ctx / model / objects / logp; a model whose last SA layer is not
 *   group_all; npts < 1; a non-finite coordinate or feature (checked on the host copy); a start outside its object; more than 2^31 - 16 rows in
 *   a stage.  Profile names pn2_sa, pn2_head, pn2_centres, pn2_logsoftmax (+ fps_small / fps_large, ball_query). */
#define PCR_PN2_MAX_SA 4
#define PCR_PN2_MAX_MLP 4
#define PCR_PN2_MAX_FC 4
typedef struct pcr_pn2_sa_desc {
    uint32_t npoint;     /* ignored for group_all */
    uint32_t nsample;    /* ignored for group_all */
    double radius;       /* ignored for group_all */
    uint32_t group_all;
    uint32_t n_mlp;
    uint32_t widths[PCR_PN2_MAX_MLP];
} pcr_pn2_sa_desc;
typedef struct pcr_pn2_desc {
    uint32_t D0;
    uint32_t n_sa;
    pcr_pn2_sa_desc sa[PCR_PN2_MAX_SA];
    uint32_t n_fc;
    uint32_t fc_widths[PCR_PN2_MAX_FC];
    double bn_eps;
} pcr_pn2_desc;
typedef struct pcr_pn2_info {
    uint64_t n_weights;          /* length of the flat weight array */
    uint64_t macs_per_object;    /* multiply-adds of one object of npts_hint points (unpadded) */
    uint32_t n_sampling;         /* SA layers that are not group_all */
    uint32_t n_class;
    uint32_t c_last;             /* width of the global feature */
    uint32_t reserved;
} pcr_pn2_info;
typedef struct pcr_pn2_model pcr_pn2_model;
int pcr_pn2_model_create(pcr_ctx* ctx, const pcr_pn2_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out);
int pcr_pn2_model_destroy(pcr_ctx* ctx, pcr_pn2_model* model);
/* desc (optional): the descriptor the model was made from; npts_hint: the object size macs_per_object is counted for */
int pcr_pn2_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn2_desc* desc);
int pcr_sa_mlp_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int layer, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres,
                       const uint32_t* centre_seg_ptr, size_t n_seg, const float* features, const uint32_t* idx, float* out);
int pcr_pn2_forward_f32(pcr_ctx* ctx, const pcr_pn2_model* model, const float* objects, size_t n_obj, size_t npts, const uint32_t* starts, uint64_t seed,
                        float* logp, int32_t* pred, float* global_feat, uint32_t* fps_idx);

/* ---- HomeworkFinal: the multi-scale (MSG) classifier, models/pointnet2_cls_msg.py + pointnet_util.py:223-281, eval mode -----------
 * pcr_pn2_msg_desc is a superset of pcr_pn2_desc.  An SA layer has npoint, group_all, xyz_last and n_branch in 1 ... 4 BRANCHES over ONE set of
 * centres; a branch has its own radius, nsample and n_mlp in 1 ... 4 widths.  The branches' outputs are concatenated in branch order
 * (torch.cat(new_points_list, dim=1), :279): the width of the layer is the sum of its branches' last widths, at most 1024, and it is the D of
 * the next layer.
 *   xyz_last   0: the input channels of the layer are (xyz - centre | features), as PointNetSetAbstraction has them (:150);
 *              1: (features | xyz - centre), as PointNetSetAbstractionMsg has them (:266).  With D == 0 the two are the same.
 *   group_all  only on the last layer, with ONE branch whose radius and nsample are ignored (the reference's sa3 is a PointNetSetAbstraction:
 *              xyz first; xyz_last is honoured there too).
 * weights: layer by layer, branch by branch, convolution by convolution, then the FC layers; every convolution laid out as for
 *   pcr_pn2_model_create (W, bias, gamma, beta, running_mean, running_var).  The fold and the arithmetic are the ones written there: one f32 fma
 *   chain per output over ascending input channel IN THE LAYER'S OWN CHANNEL ORDER, starting from the folded bias.
 * pcr_pn2_msg_model_create returns the same handle type.  On it pcr_pn2_model_destroy, pcr_pn2_forward_f32 (the same arguments: starts stays
 *   n_sampling x n_obj, one set of centres per layer) and pcr_pn2_model_info work as on any model; pcr_pn2_model_info returns PCR_ERR_ARG when it
 *   is asked for a pcr_pn2_desc and the model has a layer with several branches or with xyz_last; pcr_pn2_msg_model_info returns the descriptor
 *   of EVERY model; with model == NULL it READS *desc and fills info with what a model made from it would report (no device is needed;
 *   PCR_ERR_ARG for a descriptor outside the limits).  pcr_sa_mlp_max_f32 returns PCR_ERR_ARG on a layer with more than one branch.
 *   Per layer with several branches the forward pass is: FPS, centres, ONE multi-radius ball query, one scan of all branches' counts, one clear
 *   of the concatenated rows, one chain launch per branch (each writes its own columns).  Profile names ball_query_multi, pn2_scan.
 *
 * Tune key pn2_compact [-1 = the model's default] 0: a chain runs every row of the padded groups, npoint x nsample; 1: it runs the real hits
 *   only — the copies of the first hit that fill a ball-query row are skipped: tile row g maps to (group, member) through the exclusive scan of
 *   the counts.  The max over a group does not change when copies are dropped, so results NEVER depend on the key.  The launch is sized for the
 *   padded rows and tiles past the total return at once: the host does not wait to learn the total.  Default: 1 for models of
 *   pcr_pn2_msg_model_create, 0 for models of pcr_pn2_model_create.
 *
 * pcr_ball_query_multi_f32 — n_radii in 1 ... 4 radii per centre in ONE walk of the segment (one wave per centre, one distance per point,
 *   one ballot per radius; the walk stops when every row is full).  Every radius follows the rule of pcr_ball_query_f32 exactly, with its own
 *   nsample: idx and counts are equal on every element to pcr_ball_query_f32 called once per radius.  idx: the row blocks one after the other,
 *   block b = (number of centres) x nsamples[b]; counts (optional): n_radii x (number of centres).  PCR_ERR_ARG as pcr_ball_query_f32, and for
 *   n_radii outside 1 ... 4 or NULL radii / nsamples.  Profile name ball_query_multi.
 *
 * pcr_sa_msg_mlp_max_f32 — ONE SA layer of a model on the caller's indices: the arguments of pcr_sa_mlp_max_f32, with idx holding the branches'
 *   row blocks one after the other (block b = centres x nsample_b) and out = centres x (the layer's concatenated width).  A row that holds the
 *   segment's size in EVERY entry (pcr_ball_query_f32's empty row) is a group without a hit: its columns of that branch stay zero; any other
 *   index outside its segment is PCR_ERR_ARG.  Under pn2_compact 1 the trailing entries of a row that repeat its first entry are not run. */
#define PCR_PN2_MAX_BRANCH 4
typedef struct pcr_pn2_branch_desc {
    double radius;       /* ignored for group_all */
    uint32_t nsample;    /* ignored for group_all */
    uint32_t n_mlp;
    uint32_t widths[PCR_PN2_MAX_MLP];
} pcr_pn2_branch_desc;
typedef struct pcr_pn2_msg_sa_desc {
    uint32_t npoint;     /* ignored for group_all */
    uint32_t group_all;
    uint32_t xyz_last;
    uint32_t n_branch;
    pcr_pn2_branch_desc branch[PCR_PN2_MAX_BRANCH];
} pcr_pn2_msg_sa_desc;
typedef struct pcr_pn2_msg_desc {
    uint32_t D0;
    uint32_t n_sa;
    pcr_pn2_msg_sa_desc sa[PCR_PN2_MAX_SA];
    uint32_t n_fc;
    uint32_t fc_widths[PCR_PN2_MAX_FC];
    double bn_eps;
} pcr_pn2_msg_desc;
int pcr_pn2_msg_model_create(pcr_ctx* ctx, const pcr_pn2_msg_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out);
int pcr_pn2_msg_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn2_msg_desc* desc);
int pcr_ball_query_multi_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                             size_t n_seg, size_t n_radii, const double* radii, const size_t* nsamples, uint32_t* idx, uint32_t* counts);
int pcr_sa_msg_mlp_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int layer, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres,
                           const uint32_t* centre_seg_ptr, size_t n_seg, const float* features, const uint32_t* idx, float* out);

/* ---- HomeworkFinal: the vanilla PointNet classifier, models/pointnet_cls.py + models/pointnet.py (STN3d, STNkd, PointNetEncoder), eval mode -----
 * No sampling and no grouping: every point goes through shared convolutions, the object's feature is the max over its points, and two small
 * networks (T-Nets) predict PER OBJECT a 3 x 3 matrix for xyz and a K x K matrix for the features after the first convolution.  pcr_pn1_desc:
 *   D0         feature channels besides xyz (0, or 3: normal_channel); the input of a point is (xyz | features), C0 = 3 + D0 channels
 *   stn3       1: a T-Net on the C0 input channels predicts trans (3 x 3); xyz <- xyz . trans, the features pass unchanged (pointnet.py:105-111)
 *   fstn       1: a T-Net on the first convolution's output predicts trans_feat (K x K, K = widths[0]); x <- x . trans_feat (:114-118)
 *   widths     n_mlp in 2 ... 4 encoder convolutions (the reference: 64, 128, 1024); BN + ReLU on every one but the LAST, which has BN only
 *              (:125): the max over the points of an object is a SIGNED max
 *   tnet_conv  the 3 convolution widths of BOTH T-Nets (64, 128, 1024; BN + ReLU, then the max over points), tnet_fc their 2 FC widths
 *              (512, 256; BN + ReLU); a last linear layer without BN gives the k x k entries, row-major (k = 3 / K)
 *   fc_widths  n_fc in 1 ... 4 head widths as in pcr_pn2_desc (512, 256, classes); bn_eps as there
 * weights: ONE flat f32 array in the reference's module order — [stn3: the T-Net on the input: conv1 conv2 conv3 fc1 fc2 fc3] [the encoder's
 *   convolutions in order] [fstn: the T-Net on the features, the same six layers] [the head's FC layers]; every layer laid out as for
 *   pcr_pn2_model_create: W [out][in], bias [out], and gamma, beta, running_mean, running_var where it has BN (all but a T-Net's fc3 and the
 *   head's last layer).  A T-Net that the flags leave out has no weights.
 * pcr_pn1_model_create returns the handle type of pcr_pn2_model_create; pcr_pn2_model_destroy frees it.  BN is folded in f64 and rounded ONCE,
 *   as there.  The "+ identity" that follows a T-Net's fc3 (:41-46, :79-84) is NOT folded into that layer's bias: a chain that starts at
 *   1 + b rounds every one of its steps in the binade of 1 (measured on the reference model: 8 to 14 times the reference's own f32 deviation
 *   on trans).  It is ONE f32 addition to the finished chain of every diagonal entry, as the reference adds it.
 * Arithmetic: the library's — every output is one f32 fma chain over ascending input channel that starts from the folded bias, on
 *   v_mfma_f32_16x16x4_f32.  A TRANSFORM is the same chain starting from +0 with the object's own matrix as weights:
 *   y[j] = c_K, c_0 = +0, c_(k+1) = fmaf(x[k], T[k][j], c_k), k ascending (the 3 x 3 one in plain fmaf, the K x K one on the matrix pipe with T
 *   staged in LDS).  The max over an object's points is taken on the integer key of pcr_label_aabb_f32, which orders ALL floats:
 *   -inf < ... < -0 < +0 < ... < +inf (so -0 is BELOW +0); the output row starts at the key of -inf, not at +0.  A workgroup tile holds rows of
 *   ONE object (tiles per object = ceil(npts / R), R = the tune key pn2_rows), so a B operand never mixes two objects' matrices, and a row's
 *   bits do not depend on R, on the batch, on the object's place in it or on the workgroup that served it.
 * Limits (PCR_ERR_ARG otherwise): D0 0 ... 1021; stn3, fstn 0 / 1; n_mlp 2 ... 4; n_fc 1 ... 4; every width 1 ... 1024; with fstn widths[0] <= 128
 *   (the matrix is staged in LDS); bn_eps finite; n_weights the model's count; every weight finite; var + eps > 0.
 *
 * pcr_pn1_model_info — info (n_sampling = 0; macs_per_object: every layer and transform ONCE per point of npts_hint points plus the three
 *   heads, unpadded — the recomputation below is not counted) and the descriptor.  With model == NULL it READS *desc (no device needed).
 * On a model of pcr_pn1_model_create, pcr_pn2_forward_f32, pcr_pn2_model_info, pcr_pn2_msg_model_info, pcr_sa_mlp_max_f32 and
 *   pcr_sa_msg_mlp_max_f32 return PCR_ERR_ARG; on any other model pcr_pn1_model_info with a model, pcr_pointwise_chain_max_f32 and
 *   pcr_pointnet_forward_f32 do.
 *
 * pcr_pointwise_chain_max_f32 — ONE fused launch for one stage of the model on the caller's inputs (cloud, seg_ptr, n_seg as
 *   pcr_sa_mlp_max_f32 takes them: a segment is an object; features: host, D0 floats per point of the cloud, NULL with D0 == 0):
 *     stage 0   (stn3)  the input T-Net's convolutions -> max                                   out: n_seg x tnet_conv[2]
 *     stage 1   (fstn)  xyz . trans3 -> conv 0 -> the feature T-Net's convolutions -> max       out: n_seg x tnet_conv[2]
 *     stage 2           xyz . trans3 -> conv 0 -> . trans_feat -> conv 1 ... (last: no ReLU) -> signed max      out: n_seg x widths[n_mlp - 1]
 *   trans3: host, n_seg x 9 row-major (NULL: no transform; it must be NULL for stage 0), trans_feat: host, n_seg x K x K: stage 2 of a model
 *   with fstn needs it, every other call takes NULL.  Convolution 0 is recomputed in stages 1 and 2, not stored: the activations of a tile
 *   stay in LDS and nothing of size rows x C goes to memory.  An EMPTY segment gives a row of -inf.  PCR_ERR_ARG as pcr_sa_mlp_max_f32, and for a stage the model does not have.
 *   Profile name pn1_chain.
 *
 * pcr_pointnet_forward_f32 — the forward pass for n_obj objects of npts points: objects host, n_obj x npts x (3 + D0), uploaded once ->
 *   stage 0 -> the T-Net's FC layers (trans) -> stage 1 -> the T-Net's FC layers (trans_feat) -> stage 2 (global_feat) -> the head ->
 *   log_softmax, as pcr_pn2_forward_f32 has the last two; the identity joins a T-Net's matrix in a launch of its own (pn1_identity).  The stages hand device buffers to each other, the number of launches does not
 *   depend on n_obj, the host waits once.  logp: n_obj x n_class; optional: pred (the first maximum), global_feat n_obj x widths[n_mlp - 1],
 *   trans n_obj x 9, trans_feat n_obj x K x K (each must be NULL when the model has no such T-Net).  n_obj == 0: PCR_OK, nothing written.
 *   PCR_ERR_ARG: NULL ctx / model / objects / logp; npts < 1; a non-finite coordinate or feature (checked on the host copy, nothing is
 *   launched); more than 2^31 - 16 rows in a stage.  Profile names pn1_chain, pn1_identity, pn2_head, pn2_logsoftmax. */
typedef struct pcr_pn1_desc {
    uint32_t D0;
    uint32_t stn3;
    uint32_t fstn;
    uint32_t n_mlp;
    uint32_t widths[PCR_PN2_MAX_MLP];
    uint32_t tnet_conv[3];
    uint32_t tnet_fc[2];
    uint32_t n_fc;
    uint32_t fc_widths[PCR_PN2_MAX_FC];
    double bn_eps;
} pcr_pn1_desc;
int pcr_pn1_model_create(pcr_ctx* ctx, const pcr_pn1_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out);
int pcr_pn1_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn1_desc* desc);
int pcr_pointwise_chain_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int stage, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg,
                                const float* features, const float* trans3, const float* trans_feat, float* out);
int pcr_pointnet_forward_f32(pcr_ctx* ctx, const pcr_pn2_model* model, const float* objects, size_t n_obj, size_t npts, float* logp, int32_t* pred,
                             float* global_feat, float* trans, float* trans_feat);

/* ---- HomeworkFinal: the PointNet++ (SSG) TRAINING pass, train_cls.py's step without its optimiser: training-mode forward, get_loss
 * (pointnet2_cls_ssg.py:50-52) and the gradient of every parameter.  The optimiser is either the caller's (torch.optim.Adam on host tensors, through
 * the gradient this call downloads) or the library's own on the device (pcr_pn2_trainer_optim_set and pcr_pn2_train_step_f32, below).
 * A trainer is made from a pcr_pn2_desc (any model it can describe whose last SA layer is group_all) and the flat weight array of
 * pcr_pn2_model_create, UNFOLDED: the trainer keeps W, bias, gamma, beta, running_mean, running_var as they are given.
 * pcr_pn2_train_grad_f32 runs, for n_obj >= 2 objects of npts points (objects as pcr_pn2_forward_f32 takes them) and int32 target[n_obj]:
 *   Sampling   FPS and ball query exactly as in pcr_pn2_forward_f32, the same starts / seed rule.  No gradient flows through either.
 *   Rows       an SA layer's rows are the PADDED rows, centres x nsample, the copies that pad a ball included (torch's statistics count them);
 *              the group_all layer has one row per point.  A row's input is (xyz - centre in one f32 subtraction | the features), xyz as it
 *              is for group_all.
 *   Product    z[n] = the k-ascending fma chain from the bias of pcr_pn2_model_create's contract, on the raw W, b.
 *   BatchNorm  training mode, over the M rows of the layer (the head: M = n_obj): mu = sum z / M, var = sum (z - mu)^2 / M (biased), both
 *              accumulated in f64 (below); rstd = 1 / sqrt(var + eps) in f64; y = (z - mu) rstd gamma + beta evaluated in f64 from the f32 z
 *              and rounded ONCE.  running_mean <- (1 - m) running_mean + m mu, running_var <- (1 - m) running_var + m var M / (M - 1), in
 *              f64, rounded once to f32; m = bn_momentum (torch: 0.1).  M == 1 is PCR_ERR_ARG, as torch refuses it.
 *   ReLU, max  relu(v) = v > 0 ? v : +0; the max over a group is taken after it; its gradient goes to the LOWEST member position among the
 *              maxima (copies tie exactly and carry the same input row, so no parameter gradient depends on the choice); a max of 0 passes nothing.
 *   Head       FC -> BN -> ReLU -> dropout for every FC layer but the last.  dropout: a = y s where keep != 0, +0 elsewhere, s = f32(1 / (1 - p)),
 *              one f32 product.  keep (optional): bytes, one per object and unit, layer after layer ([n_obj][fc_widths[0]], [n_obj][fc_widths[1]] ...).
 *              NULL: keep[layer i][cell e] = (K(seed, (0x100 + i) << 32 | e) >> 11) 2^-53 >= p with the SplitMix keying above.  UNPINNED: torch's stream.
 *   Loss       log_softmax of the last FC layer as in pcr_pn2_forward_f32; loss = -(1 / n_obj) sum_b logp[b][target[b]], ascending b, in f64.
 *   Backward   dlogits = (exp(logp) - onehot) / n_obj (f64, rounded once).  Dropout: the same mask and s.  ReLU passes where y > 0.  BN, with
 *              gy the gradient at y: dbeta = sum gy, dgamma = sum gy xhat, xhat = (z - mu) rstd,
 *              dz = rstd gamma (gy - dbeta / M - xhat dgamma / M), in f64, rounded once.  dW = dz^T x, dx = dz W (one f32 fma chain from +0
 *              over ascending output channel).  The gradient of a layer's input features goes back to the point each row read, summed in
 *              f64 over the rows that read that point, rows ascending, rounded once; the xyz columns are dropped.  The bias of a layer that BN
 *              follows has a gradient that is analytically zero: the library writes +0 there and does not compute it.  The last FC layer's
 *              bias gradient is the column sum of dlogits.
 *   Order      No floating-point atomic anywhere.  Every sum over the rows of a layer (mu, var, dbeta, dgamma, the last bias, dW) runs over
 *              consecutive chunks of chunk_rows rows: rows ascending inside a chunk, then the chunk partials added in ascending order; in f64
 *              for the statistics, dbeta, dgamma and the bias, in f32 for dW (one fma chain from +0 per chunk on v_mfma_f32_16x16x4_f32, the
 *              partials added in f32).  chunk_rows is a creation parameter (0 = 256), reported by pcr_pn2_trainer_info, and the ONLY thing
 *              besides the inputs the bits may depend on: pn2_rows, every other tune key, the launch geometry and a repeat of the call give
 *              the same bits.  With chunk_rows >= the rows of every layer each sum is one chunk.
 *   Outputs    loss (f64), logp n_obj x n_class, grad: n_weights floats in the weight layout, +0 in the running_mean / running_var slots and
 *              in the pre-BN biases.  The trainer's own running statistics advance once per call, on the device.
 * pcr_pn2_trainer_set_weights replaces the weights (keep_running_stats != 0: all but the running statistics, which stay the device's);
 * pcr_pn2_trainer_get_weights reads them back, the updated running statistics included.  pcr_pn2_trainer_info: device_bytes is what a call
 * with n_obj objects of npts points takes (0 when either is 0); keep_per_object the length of an object's part of `keep`, summed over layers.
 * PCR_ERR_ARG: NULL arguments; everything pcr_pn2_model_create / pcr_pn2_forward_f32 refuse; n_obj == 1; a layer with one row; a target outside
 *   [0, n_class); dropout_p outside [0, 1); bn_momentum outside [0, 1]; a last SA layer that is not group_all; a non-finite input or weight;
 *   more than 65535 chunks or 2^21 rows in a layer.  n_obj == 0: PCR_OK, nothing written, the running statistics untouched.
 * Profile names pn2t_gather, pn2t_centres, pn2t_gemm_fwd, pn2t_stat, pn2t_bn_relu, pn2t_max, pn2t_loss, pn2t_max_back, pn2t_bn_back,
 *   pn2t_gemm_dw, pn2t_dw_reduce, pn2t_gemm_dx, pn2t_gather_back (+ fps_small / fps_large, ball_query). */
typedef struct pcr_pn2_trainer pcr_pn2_trainer;
typedef struct pcr_pn2_train_info {
    uint64_t n_weights;
    uint64_t device_bytes;
    uint64_t keep_per_object;
    uint32_t chunk_rows;
    uint32_t n_class;
    uint32_t n_sampling;
    uint32_t reserved;
    double dropout_p;
    double bn_momentum;
} pcr_pn2_train_info;
int pcr_pn2_trainer_create(pcr_ctx* ctx, const pcr_pn2_desc* desc, const float* weights, size_t n_weights, double dropout_p, double bn_momentum,
                           uint32_t chunk_rows, pcr_pn2_trainer** out);
int pcr_pn2_trainer_destroy(pcr_ctx* ctx, pcr_pn2_trainer* trainer);
int pcr_pn2_trainer_info(const pcr_pn2_trainer* trainer, size_t n_obj, size_t npts, pcr_pn2_train_info* info);
int pcr_pn2_trainer_set_weights(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const float* weights, size_t n, int keep_running_stats);
int pcr_pn2_trainer_get_weights(pcr_ctx* ctx, const pcr_pn2_trainer* trainer, float* weights, size_t n);
int pcr_pn2_train_grad_f32(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const float* objects, size_t n_obj, size_t npts, const int32_t* target,
                           const uint32_t* starts, uint64_t seed, const uint8_t* keep, double* loss, float* logp, float* grad);

/* ---- HomeworkFinal: the vanilla PointNet (pointnet_cls) TRAINING pass: training-mode forward, pointnet_cls.get_loss (:32-42, with
 * pointnet.py:135-141's feature-transform regulariser) and the gradient of every parameter.  The optimiser: as for the SSG trainer (pcr_pointnet_train_step_f32).
 * A trainer is made from a pcr_pn1_desc (the limits of pcr_pn1_model_create) and the flat weight array of pcr_pn1_model_create, UNFOLDED: W,
 * bias, gamma, beta, running_mean, running_var are kept as given.  The handle is the SSG trainer's type: pcr_pn2_trainer_destroy, _info
 * (n_sampling = 0), _set_weights and _get_weights work on it; pcr_pn2_train_grad_f32 on it is PCR_ERR_ARG, and so is
 * pcr_pointnet_train_grad_f32 on a trainer of pcr_pn2_trainer_create.
 * pcr_pointnet_train_grad_f32 runs, for n_obj >= 2 objects of npts points (objects as pcr_pointnet_forward_f32 takes them) and int32 target[n_obj]:
 *   Rows       a convolution stage has n_obj x npts rows: no sampling, no padding.  An FC stage (the T-Nets' and the head's) has n_obj rows.
 *   Product    on the raw W, b, BLOCKED over k (v_mfma_f32_16x16x4_f32): inside every block of 64 consecutive k an output is ONE f32 fma chain from +0
 *              over ascending k; the block results join an f64 sum that starts at the bias, blocks ascending; z[n] is that sum rounded ONCE.  dx is taken
 *              the same way over the output channels, from +0.  (Not the SSG trainer's single chain: this model has three 1024-term products in front of
 *              its first FC layers and three 1024-wide convolutions, and one f32 chain over 1024 terms put the gradients of the small exact fixture up
 *              to 40 of the reference's own f32 errors away from its f64 pass; blocked, 7.)  dW is the SSG trainer's: chains over chunks of rows.
 *   BatchNorm  the SSG trainer's, word for word: mu, biased var in f64 by chunks, rstd in f64, y evaluated in f64 from the f32 z and rounded
 *              ONCE; the running statistics of all the model's BatchNorms (15 with both T-Nets) advance once per call, in f64, rounded once.
 *   T-Net      three times conv -> BN -> ReLU on the stage's rows; the max over the object's points (after the ReLU; its gradient goes to the
 *              LOWEST position among the maxima, a max of 0 passes nothing); two times FC -> BN -> ReLU; a linear layer WITHOUT BN with k k
 *              outputs (k = 3, or K = widths[0] <= 128: up to 16 384, the 1 024 limit on a width does not apply to it) whose bias has a real
 *              gradient, the column sum of its dz; then "+ identity": ONE f32 addition of 1 to every diagonal entry of the finished chain.
 *   Transform  forward: y[j] = c_K, c_0 = +0, c_(k+1) = fmaf(x[k], T[k][j], c_k) with the object's own matrix, k ascending (3 x 3: plain fmaf
 *              on xyz, the D0 features pass through; K x K: on the matrix pipe, T staged in LDS, a workgroup serving rows of ONE object).
 *              The transformed rows are kept in memory.  Backward: dx[k] = the chain from +0 over ascending j of dy[j] T[k][j] (dx = dy T^T;
 *              not taken for the 3 x 3 transform: the input takes no gradient), and dT[b][k][j] = sum over the rows n of object b ALONE of
 *              x[b,n][k] dy[b,n][j]: ONE f32 fma chain from +0 over ascending n (the dW product with one chunk per object: chunk_rows does
 *              not enter it).  dT is the gradient of the T-Net's last layer's output (the identity has none).
 *   Encoder    conv 0 -> BN -> ReLU; the feature transform; the middle convolutions with BN + ReLU; the last convolution has BN only, so the
 *              max over an object's points is SIGNED: taken in the order -inf < ... < -0 < +0 < ... < +inf (the integer key of
 *              pcr_pointnet_forward_f32), the gradient goes to the LOWEST position that holds the maximum, always to exactly one.
 *   Two paths  conv 0's activation feeds the feature T-Net and the transform: its gradient is g_transform + g_tnet, ONE f32 addition, the
 *              T-Net's path added to the transform's.
 *   Head       FC -> BN -> ReLU for every layer but the last; the dropout sits on the PRODUCT of the last hidden FC layer (n_fc - 2), before
 *              its BN (pointnet_cls.py:25-27: fc2 -> dropout -> bn2 -> relu); none with n_fc == 1.  z <- z s where keep != 0, +0 elsewhere,
 *              s = f32(1 / (1 - p)), one f32 product; the statistics are those of the dropped z.  keep (optional): one byte per object and
 *              unit of that layer, [n_obj][keep_per_object].  NULL: keep[e] = (K(seed, (0x100 + n_fc - 2) << 32 | e) >> 11) 2^-53 >= p with the
 *              SplitMix keying of the SSG trainer.  UNPINNED: torch's stream.  p == 0: s = 1 and a drawn mask is all ones, so z is unchanged
 *              bit for bit; a caller's mask still applies.  The dropped layer's bias is NOT analytically zero (dropout lies between it and the
 *              BN): its gradient is computed, the column sum of the masked, scaled dz.
 *   Loss       loss[1] = the NLL as in the SSG trainer.  With fstn, per object A = trans_feat (f32), in f64 with products and sums rounded
 *              separately: M = A (A^T - I) = A A^T - A as pointnet.py:140 has it (NOT A A^T - I), M[i][j] = (sum over ascending k of
 *              A[i][k] A[j][k]) - A[i][j]; norm = sqrt(sum over ascending i of (sum over ascending j of M[i][j]^2)); loss[2] = reg = (sum over
 *              ascending b of norm_b) / n_obj; loss[0] = nll + reg_scale reg.  dA[p][q] = reg_scale / (n_obj norm) ((sum over ascending j of
 *              (M[p][j] + M[j][p]) A[j][q]) - M[p][q]) in f64, rounded ONCE, then dT + dA in ONE f32 addition (dA added to the gradient that
 *              came back through the transform).  Without fstn reg = 0 (the reference would raise).  UNPINNED: a zero norm gives dA = +0,
 *              where torch gives NaN.
 *   Backward   everything else as the SSG trainer has it: dlogits, ReLU, BN, dW, +0 in the bias of a layer that BN follows directly; dx as under Product.
 *   Order      No floating-point atomic anywhere.  Every sum over the rows of a layer follows the SSG trainer's chunk scheme, so the bits
 *              depend on the inputs and on chunk_rows only: not on pn2_rows or any other tune key, not on a repeat of the call.
 *   Outputs    loss[3] (f64: total, NLL, the unscaled regulariser), logp n_obj x n_class, grad: n_weights floats in the weight layout, +0 in
 *              the running-statistic slots and in the biases BN follows directly; optional trans n_obj x 9 and trans_feat n_obj x K x K,
 *              identity included (each must be NULL when the model has no such T-Net).
 * PCR_ERR_ARG: NULL arguments; a descriptor pcr_pn1_model_create refuses; a trainer of the other kind; n_obj == 1; npts < 1; a target outside
 *   [0, n_class); dropout_p outside [0, 1); bn_momentum outside [0, 1]; a non-finite reg_scale, input or weight; trans / trans_feat without
 *   its T-Net; more than 65535 objects, 65535 chunks or 2^21 rows in a stage.  n_obj == 0: PCR_OK, nothing written, the running statistics
 *   untouched.
 * Profile names pn1t_gemm_fwd, pn1t_gemm_dx, pn1t_transform3, pn1t_transform, pn1t_identity, pn1t_smax, pn1t_dropout, pn1t_reg, pn1t_loss_fin, pn1t_add,
 *   pn1t_gemm_dt; the shared kernels keep pn2t_stat, pn2t_bn_relu, pn2t_max, pn2t_loss, pn2t_max_back, pn2t_bn_back, pn2t_gemm_dw, pn2t_dw_reduce. */
int pcr_pn1_trainer_create(pcr_ctx* ctx, const pcr_pn1_desc* desc, const float* weights, size_t n_weights, double dropout_p, double bn_momentum,
                           double reg_scale, uint32_t chunk_rows, pcr_pn2_trainer** out);
int pcr_pointnet_train_grad_f32(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const float* objects, size_t n_obj, size_t npts, const int32_t* target,
                                uint64_t seed, const uint8_t* keep, double loss[3], float* logp, float* trans, float* trans_feat, float* grad);

/* ---- HomeworkFinal: the PointNet++ multi-scale (MSG) TRAINING pass: training-mode forward, pointnet2_cls_msg.get_loss and the gradient of
 * every parameter.  A trainer is made from a pcr_pn2_msg_desc (any descriptor pcr_pn2_msg_model_create accepts whose last SA layer is
 * group_all) and that function's flat weight array, UNFOLDED.  The handle is the SSG trainer's type: pcr_pn2_trainer_destroy, _info,
 * _set_weights and _get_weights work on it, and pcr_pn2_train_grad_f32 RUNS THE STEP on it with the same arguments (starts stays
 * n_sampling x n_obj, one set of centres per layer; the same seed rule); pcr_pointnet_train_grad_f32 on it is PCR_ERR_ARG.  It is the SAME
 * pass: a trainer of pcr_pn2_trainer_create is the case of one xyz-first branch per layer and one p, bit for bit.
 * dropout_p: n_dropout = n_fc - 1 probabilities in [0, 1), one per hidden FC layer (the reference: drop1 0.4, drop2 0.5,
 *   pointnet2_cls_msg.py:18,21); with n_fc == 1 n_dropout is 0 and dropout_p may be NULL.  pcr_pn2_trainer_info reports the FIRST hidden
 *   layer's p in dropout_p (0 with n_fc == 1); pcr_pn2_msg_trainer_info reports all of them.
 * Everything the SSG trainer's contract says holds word for word per (branch, convolution).  Added:
 *   Sampling   FPS once per layer; a layer with several branches takes ONE multi-radius walk (pcr_ball_query_multi_f32's kernel): idx is, on
 *              every element, what pcr_ball_query_f32 gives per radius.  No gradient flows through either.  npoint may exceed the points of
 *              an object, as in the eval pass (picks repeat index 0 once every distance is 0).
 *   Rows       branch b of a layer has the PADDED rows, centres x nsample_b, copies included; every (branch, convolution) has its own BatchNorm
 *              over its own M_b rows with its own chunks.  A row's input is (xyz - centre | features) with xyz_last == 0 and
 *              (features | xyz - centre) with xyz_last == 1, xyz - centre in one f32 subtraction; the product's chain runs over ascending
 *              channel IN THAT ORDER.  The limits of 2^21 rows and 65535 chunks apply per (branch, layer).
 *   Max        per branch, after the ReLU, at the lowest member position; it writes columns [off_b, off_b + w_b) of the layer's concatenated
 *              row, off_b = the sum of the earlier branches' last widths.  Backward, each branch reads its own columns of that row's gradient.
 *   Features   the gradient of a layer's input features is, per point and channel, ONE f64 sum over the rows of ALL branches that read the
 *              point: branches ascending, rows ascending inside a branch (one launch per branch, the sum handed on in f64), rounded once to
 *              f32.  The xyz columns (0 ... 2, or the last three with xyz_last) are dropped; a point no row read gets +0.  The first SA layer's
 *              convolutions take no dx.
 *   Head       as the SSG trainer's with layer i's OWN p: s_i = f32(1 / (1 - p_i)), the drawn mask is keep[i][e] =
 *              (K(seed, (0x100 + i) << 32 | e) >> 11) 2^-53 >= p_i; the keep bytes are laid out as there.
 *   Order      No floating-point atomic.  The bits depend on the inputs and chunk_rows only: not on pn2_rows, pn2_compact or any other tune
 *              key, nor on a repeat.
 * pcr_pn2_msg_trainer_info — pcr_pn2_trainer_info's fields, plus (optional) the descriptor in the superset form (a trainer of
 *   pcr_pn2_trainer_create reports one xyz-first branch per layer) and (optional) PCR_PN2_MAX_FC - 1 doubles: the hidden layers' p, 0 behind
 *   the last.  PCR_ERR_ARG: NULL trainer / info, a trainer of pcr_pn1_trainer_create, a call too large (as pcr_pn2_trainer_info).
 * PCR_ERR_ARG (create): NULL ctx / desc / weights / out; a descriptor pcr_pn2_msg_model_create refuses; a last SA layer that is not
 *   group_all; n_dropout != n_fc - 1; NULL dropout_p with n_dropout > 0; a p outside [0, 1); bn_momentum outside [0, 1]; n_weights not the
 *   model's count; a non-finite weight; var + eps <= 0.  The step: as pcr_pn2_train_grad_f32, a (branch, layer) with one row included.
 * Profile names: the SSG trainer's (+ ball_query_multi). */
int pcr_pn2_msg_trainer_create(pcr_ctx* ctx, const pcr_pn2_msg_desc* desc, const float* weights, size_t n_weights, const double* dropout_p,
                               size_t n_dropout, double bn_momentum, uint32_t chunk_rows, pcr_pn2_trainer** out);
int pcr_pn2_msg_trainer_info(const pcr_pn2_trainer* trainer, size_t n_obj, size_t npts, pcr_pn2_train_info* info, pcr_pn2_msg_desc* desc,
                             double* dropout_p);

/* ---- HomeworkFinal: the OPTIMISER of the three trainers on the device: torch.optim.Adam (amsgrad off, coupled weight decay) and
 * torch.optim.SGD (momentum, dampening, weight decay, no nesterov), the two train_cls.py:147-155 builds.  It lives on the pcr_pn2_trainer handle,
 * whichever create made it; its state is f32 in the weight layout, on the device, beside the weights and the gradient a pass leaves there.
 * pcr_pn2_trainer_optim_set attaches or replaces it (state +0, step count 0); a NULL desc detaches it and frees the state, and so does
 * pcr_pn2_trainer_destroy.  pcr_pn2_trainer_set_weights keeps it, as torch's load_state_dict of a model keeps its optimiser.
 *   Parameters an element of the flat array is a PARAMETER unless it is a running_mean / running_var slot.  Only parameters move: the update neither
 *              reads nor writes a running-statistic slot of the weights, the gradient or the state (the state stays +0 there, whatever the
 *              gradient holds).  Pre-BN biases ARE parameters: their gradient is +0 by the pass's contract and weight decay still moves them.
 *   Adam       with t = the step count after its increment, per parameter element, every operation in f64 from the f32 w, g, m, v, each operation
 *              rounded on its own (no fused multiply-add), sqrt and / correctly rounded:
 *                g' = g + wd w;   m' = m + (1 - beta1) (g' - m);   v' = beta2 v + (1 - beta2) (g' g');
 *                w <- f32(w - step (m' / (sqrt(v') / sqrt(bc2) + eps))),  m <- f32(m'),  v <- f32(v'): each stored value rounded ONCE, and w
 *              takes the f64 m' and v' BEFORE their rounding.  On the host in f64: 1 - beta1 and 1 - beta2; bc1 = 1 - p1_t, bc2 = 1 - p2_t with
 *              p_t = p_(t-1) beta, p_0 = 1 (the product chain, not pow: torch's beta ** t may differ in the last place); step = lr / bc1;
 *              sqrt(bc2).  torch rounds to f32 after every operation and evaluates step_size m / denom as addcdiv does.
 *   SGD        g' = g + wd w;  the FIRST update (step count 0 before it) and every update with momentum == 0: b' = g'; later:
 *              b' = momentum b + (1 - dampening) g';  b <- f32(b'),  w <- f32(w - lr b'), in f64 as above, b' before its rounding.
 *   Bits       depend on the inputs and the step count only: not on the launch geometry, a tune key or a repeat.  f32 subnormals are kept
 *              (a subnormal v, an underflowing g' g'), g = 0 gives what IEEE gives.
 * pcr_pn2_trainer_optim_step applies one update from the gradient the last pass left on the device (one launch on the context's stream, then a
 *   wait).  pcr_pn2_train_step_f32 / pcr_pointnet_train_step_f32 take the arguments of pcr_pn2_train_grad_f32 / pcr_pointnet_train_grad_f32 with lr
 *   in front of the outputs and grad OPTIONAL: the same pass, then the update in the same stream (only where the pass raised no error), then the
 *   downloads of loss, logp, the optional outputs and, where grad is not NULL, the gradient; one wait.  The pass reads the weights BEFORE the
 *   update, so a pass followed by pcr_pn2_trainer_optim_step gives the same bits.  n_obj == 0: PCR_OK, nothing touched, the count stays.
 * pcr_pn2_trainer_optim_info: attached (0: everything else is 0), the descriptor, the step count, state_bytes (the state arrays and the range
 *   table on the device), n_ranges (the merged parameter ranges of the flat array).  pcr_pn2_trainer_info reports what it reported before.
 * pcr_pn2_trainer_optim_get_state / _set_state: the step count and the state in the weight layout, n = n_weights floats each (Adam: state0 =
 *   exp_avg, state1 = exp_avg_sq; SGD: state0 = momentum_buffer, state1 unused and may be NULL), for checkpoints.
 * pcr_pn2_trainer_get_grad reads the gradient the last pass left on the device (n = n_weights floats, the layout of the grad output of
 *   pcr_pn2_train_grad_f32): what a step call with grad == NULL did not download.  PCR_ERR_ARG before any pass has run.
 * PCR_ERR_ARG: NULL ctx / trainer (desc may be NULL: detach); a trainer on another device; an unknown kind; a beta outside [0, 1); a negative or
 *   non-finite eps, weight_decay or momentum; a non-finite dampening.  A step: no optimiser attached; a non-finite lr; pcr_pn2_trainer_optim_step
 *   before any pass has run on the trainer; the step functions: everything their *_train_grad_f32 refuses but a NULL grad, the other kind of trainer
 *   included.  The state calls: no optimiser attached; n not the model's count; a NULL array the kind needs; a non-finite value or a negative exp_avg_sq.
 * Profile names pnopt_adam, pnopt_sgd. */
enum pcr_optim_kind { PCR_OPTIM_ADAM = 1, PCR_OPTIM_SGD = 2 };
typedef struct pcr_optim_desc {
    int32_t kind;            /* PCR_OPTIM_ADAM or PCR_OPTIM_SGD */
    uint32_t reserved0;
    double beta1, beta2, eps;        /* Adam */
    double weight_decay;             /* both */
    double momentum, dampening;      /* SGD */
    double reserved[4];
} pcr_optim_desc;
typedef struct pcr_optim_info {
    pcr_optim_desc desc;
    uint64_t step;
    uint64_t state_bytes;
    uint32_t attached;
    uint32_t n_ranges;
} pcr_optim_info;
int pcr_pn2_trainer_optim_set(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const pcr_optim_desc* desc);
int pcr_pn2_trainer_optim_step(pcr_ctx* ctx, pcr_pn2_trainer* trainer, double lr);
int pcr_pn2_trainer_optim_info(const pcr_pn2_trainer* trainer, pcr_optim_info* info);
int pcr_pn2_trainer_optim_get_state(pcr_ctx* ctx, const pcr_pn2_trainer* trainer, uint64_t* step, float* state0, float* state1, size_t n);
int pcr_pn2_trainer_optim_set_state(pcr_ctx* ctx, pcr_pn2_trainer* trainer, uint64_t step, const float* state0, const float* state1, size_t n);
int pcr_pn2_trainer_get_grad(pcr_ctx* ctx, const pcr_pn2_trainer* trainer, float* grad, size_t n);
int pcr_pn2_train_step_f32(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const float* objects, size_t n_obj, size_t npts, const int32_t* target,
                           const uint32_t* starts, uint64_t seed, const uint8_t* keep, double lr, double* loss, float* logp, float* grad);
int pcr_pointnet_train_step_f32(pcr_ctx* ctx, pcr_pn2_trainer* trainer, const float* objects, size_t n_obj, size_t npts, const int32_t* target,
                                uint64_t seed, const uint8_t* keep, double lr, double loss[3], float* logp, float* trans, float* trans_feat,
                                float* grad);

/* ---- next row N4: global-registration front half, Homework9/hw9/src/registration.cpp:288-434, :535-615 -----------
 * N4a: exhaustive 1-NN between two descriptor sets (row-major n x dim / m x dim f32, host memory; dim 33 = FPFH),
 * nanoflann's evalMetric arithmetic for any dim (nanoflann.hpp:382-405: groups of four + tail, f32, unfused), canonical
 * tie rule (min d2, lowest index), acceptance d2 < FLT_MAX; idx = UINT32_MAX / d2 = +inf when nothing is accepted. */
int pcr_nn1_desc_f32(pcr_ctx* ctx, const float* db, size_t n, const float* q, size_t m, int dim, uint32_t* idx, float* d2);
/* N4b: findRANSACCorrespondencesUnion (:535-615).  pairs: room for 2 * (n_src + n_tgt) u32, (src, tgt) interleaved;
 * dist: n_src + n_tgt floats (squared descriptor distance of each kept pair); *n_pairs = floor((1 - rate) * total) as
 * the reference computes it (f32).  Sorted by distance; ties in input order (the reference: std::sort, unspecified). */
int pcr_match_union_f32(pcr_ctx* ctx, const float* desc_src, size_t n_src, const float* desc_tgt, size_t n_tgt, int dim,
                        float rejection_rate, uint32_t* pairs, float* dist, size_t* n_pairs);
/* findRANSACCorrespondencesInter (:437-533): the mutual-nearest-neighbour variant — (s, nn_tgt(s)) kept iff nn_src(nn_tgt(s)) == s,
 * ascending s, then sorted by the source->target distance and cut to floor((1 - rate) * count).  pairs: room for 2 * n_src. */
int pcr_match_inter_f32(pcr_ctx* ctx, const float* desc_src, size_t n_src, const float* desc_tgt, size_t n_tgt, int dim,
                        float rejection_rate, uint32_t* pairs, float* dist, size_t* n_pairs);
/* N4c: Registration::RANSAC (:288-434).  Sampling (host logic, no GPU): n_hyp quads of correspondence indices drawn as
 * :318-352 draws them (std::mt19937 + uniform_int_distribution, non-coplanar SOURCE keypoints), seeded explicitly
 * instead of std::random_device.  PCR_ERR_STATE when no admissible quad exists (the reference would loop forever). */
int pcr_ransac_sample_quads(const float* src_xyz, size_t n_src, const uint32_t* pairs, size_t n_pairs, size_t n_hyp,
                            uint64_t seed, uint32_t* quads);
/* consensus-set size (:395-421) of n_hyp given poses Rt[h] = {R row-major 9, t 3} over all correspondences:
 * counts[h] = #{i : || tgt_i - (R src_i + t) || <= thr}, f32, unfused.  xyz arrays are AoS (n x 3), host memory. */
int pcr_consensus_count_f32(pcr_ctx* ctx, const float* src_xyz, size_t n_src, const float* tgt_xyz, size_t n_tgt,
                            const uint32_t* pairs, size_t n_pairs, const float* Rt, size_t n_hyp, float thr, uint32_t* counts);
/* the whole loop over given quads: 4-point Kabsch per hypothesis (:354-392, f64 moments + the solve of
 * pcr_kabsch_solve) -> consensus counts -> first hypothesis with the largest count (:423-428).  *winner = -1 (R, t
 * untouched) when every consensus set is empty; counts (optional): n_hyp. */
int pcr_ransac_global_f32(pcr_ctx* ctx, const float* src_xyz, size_t n_src, const float* tgt_xyz, size_t n_tgt,
                          const uint32_t* pairs, size_t n_pairs, const uint32_t* quads, size_t n_hyp, float thr,
                          float R[9], float t[3], uint32_t* best_count, int64_t* winner, uint32_t* counts);

/* ---- multi-GPU: one process per GPU, sources sharded, targets replicated ------------------------------
 * Exactly one collective per ICP iteration: all-reduce(sum) of 56 + 2 * nranks f64 (wire format below; 104 at PCR_MAX_RANKS —
 * a pcr_allreduce_fn must accept n up to 128). */
#define PCR_COMM_ID_BYTES 128
#define PCR_MAX_RANKS 24      /* one node has 8 GPUs; the per-iteration reduce buffer holds 56 + 2 * nranks <= 128 f64 */
int pcr_comm_unique_id(char id[PCR_COMM_ID_BYTES]);                     /* rank 0; broadcast it out of band */
int pcr_comm_init_rccl(pcr_ctx* ctx, int nranks, int rank, const char id[PCR_COMM_ID_BYTES]);
/* alternative transport: a host callback that sums buf[0..n) over ranks in place and returns 0
 * (lets the caller use its own process group, e.g. torch.distributed gloo on CPU boxes) */
typedef int (*pcr_allreduce_fn)(void* user, double* buf, int n);
int pcr_comm_init_callback(pcr_ctx* ctx, int nranks, int rank, pcr_allreduce_fn fn, void* user);
int pcr_comm_destroy(pcr_ctx* ctx);
/* one real ncclAllReduce on the attached RCCL communicator (any nranks, also 1), result checked */
int pcr_comm_selftest(pcr_ctx* ctx);
/* Wire format of the per-iteration collective (what a pcr_allreduce_fn sums): 56 + 2 * nranks doubles —
 *   [0..54]  the 16 Kabsch moments as exact 40-bit integer limbs on a fixed-point grid shared by all ranks (unit 2^(e-80) for the
 *            six coordinate sums: 3 doubles each = limb 0, limb 1, carry; unit 2^(2e-120) for the nine products q_r p_c: 4 doubles
 *            each; [54] the pair count), [55] overflow flag, [56 + 2r] / [57 + 2r] (ORDER KEY, d2 of the last kept pair) of rank r: the key
 *            is 0 when the rank kept no pair, else the pair's index in the whole source cloud + 1 for a shard made by
 *            pcr_cloud_shard_spatial, rank + 1 for any other cloud (contiguous blocks in rank order).  The iteration's `loss`
 *            (registration.cpp:939: d2 of the last pair pushed) is taken from the slot with the LARGEST key.
 * Every entry is an integer (or one rank's value) below 2^53, so the sum is exact in any order: the pose does not depend on the
 * number of ranks.  pcr_kabsch_limbs_to_sums (host logic, no GPU) propagates the carries of a summed row in place and returns
 * the 16 moments pcr_kabsch_solve takes; e = pcr_kabsch_grid_exponent(largest finite |target coordinate|, max_corr). */
int pcr_kabsch_grid_exponent(float target_absmax, float max_corr);
int pcr_kabsch_limbs_to_sums(double row[55], int e, double sums[16]);
/* contiguous shard [begin, end) of n items for `rank` of `nranks` (sizes differ by at most one) */
void pcr_shard_range(size_t n, int nranks, int rank, size_t* begin, size_t* end);
/* SPATIALLY COHERENT shards (the reference shards nothing — registration.cpp:925-941 is one serial loop — so the partition is ours to
 * choose, and the exact integer sums make the pose independent of it, bit for bit).  `full` = the WHOLE source cloud, uploaded on
 * every rank (10 M points: 120 MB); out = this rank's share: the cloud in the order of the target's index (cell, then Morton code
 * inside the cell) is cut into nranks x chunks_per_rank runs of equal length (0 = 64 per rank) that are dealt round-robin.  Every rank
 * holds compact pieces of the scene at the scene's own density — the tile search of large targets needs that; a uniformly drawn 1 / N
 * sample (contiguous blocks of a shuffled cloud) spreads its queries N times thinner — and the deal balances expensive regions
 * against cheap ones.  Deterministic: all ranks compute the same order from the same two clouds (shards disjoint, complete).  The
 * shard keeps ascending original order and remembers each point's index in `full` (pcr_cloud_global_index), which is what makes
 * "the last kept pair" well defined across ranks (the wire format above).  `full` may be destroyed afterwards. */
int pcr_cloud_shard_spatial(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* full, int nranks, int rank, int chunks_per_rank, pcr_cloud** out);
int pcr_cloud_global_index(pcr_ctx* ctx, const pcr_cloud* shard, uint32_t* index);   /* host, pcr_cloud_size(shard) entries, ascending */

/* ---- Homework3: K-Means, its k-means++-style seeding and Gaussian-mixture EM (csrc/mixture.hip) ------------------------
 * Data is row-major f64, n x dim, as the reference's arrays are; limits 1 <= dim <= 8, 1 <= k <= 64, k <= n < 2^31, every datum finite
 * and the largest |x| within 2^-400 .. 2^400 (or 0).  Anything else is PCR_ERR_ARG.  pcr_mat64_create uploads the data ONCE; no call
 * below moves an n-sized array across the bus inside its loop (labels, p_last and post are copied out once, at the end, when asked for).
 *
 * ORDER-FREE SUMS.  Every sum over points (cluster coordinate sums, the seeding's mean distance, N_k, sum gamma x, sum gamma (x - mu)(x - mu)^T)
 * is taken on a fixed-point grid: with 2^e the smallest power of two above every |x| of the handle, a term is cut towards zero to a
 * multiple of the unit — 2^(e - 96) for coordinates and gamma x, 2^-95 for gamma, 2^(e + 3 - 96) for distances, 2^(2e + 2 - 96) for the
 * second moments —, the multiples are added as integers (three signed 32-bit limbs in 64-bit words) and the total is rounded to f64 once.
 * The results are the same bits under any launch geometry: pcr_tune_set(ctx, "mixture_geometry", 1) selects another one (128-lane
 * workgroups, at most 24 of them, one shared set of limb rows) for tests to show this; "mixture_batch" [8] = iterations per read-back.
 *
 * pcr_kmeans_step_f64: one iteration of KMeans.py:61-65.  Assignment: s = sum_d (x_d - c_d)^2 in f64, unfused, ascending d starting from
 *   (x_0 - c_0)^2; argmin s, lowest centre index on ties (scipy's KDTree returns sqrt(s); which of two centres within a rounding of each
 *   other it reports is UNPINNED).  centres_out[j] = (order-free sum of the members, rounded once) / count, so
 *   |c - exact mean| <= 2^-52 max|x|.  An empty cluster has count 0 and a NaN centre (np.mean of an empty slice), and the call returns the
 *   positive status PCR_EMPTY_CLUSTER.  labels (int32, n), counts (k), centres_out (k dim) may each be NULL.
 * pcr_kmeans_fit_f64: the whole loop on the device; the host reads one 32-byte status record per batch of iterations.
 *   PCR_KMEANS_PY  (KMeans.py:55-70): `while not converged and count <= max_iter`, i.e. up to max_iter + 1 passes; the SIGNED test
 *                  all((new - old) < tol) as written.  PCR_KMEANS_CPP (spectralClustering.cpp:337-407, 413-427): the fabs test; converged
 *                  when it holds and count < max_iter, else the loop ends unconverged once count > max_iter.
 *   centres = the centres of the last pass (the reference's center_ on convergence), *iters = passes made, labels (may be NULL) = the
 *   assignment under those centres (KMeans.predict).  Stops at, and returns, PCR_EMPTY_CLUSTER (the reference goes on with NaN centres).
 * pcr_kmeans_predict_f64: the assignment alone (KMeans.py:73-83); any k <= 64.
 * pcr_kmeanspp_init_f64: init_choice of hw3/sript/KMeans.py:16-41 (factor 1.0) and hw3/sript/GMM.py (factor 1.25).  idx[0] = floor(u_0 n);
 *   for each further pick j: d_i = distance to the nearest chosen point (sqrt(s), a running minimum), mean_d = (order-free sum of d) / n,
 *   w_i = 0 where d_i < factor mean_d, else exp(d_i); idx[j] = the first i with cumsum(w)_i / cumsum(w)_{n-1} > u_j, which is what
 *   Generator.choice(n, 1, p = w / sum w) computes from one uniform (searchsorted(cdf, u, side = 'right')).  The reference draws unseeded:
 *   the uniforms are the caller's (u, k entries in [0, 1)), or with u == NULL u_j = (K(seed, j) >> 11) 2^-53 under the SplitMix64 keying
 *   of pcr_normal_space_sample_f32.  UNPINNED: numpy's stream, the order of the inclusive scan (a rocPRIM device scan) and so a pick
 *   whose u lies within rounding of a cdf edge.  exp overflow (d > 709.78) and weights that sum to 0 are PCR_ERR_STATE (the reference
 *   gets NaN probabilities and raises).  p_last (n, may be NULL, needs k >= 2): the distribution w / sum w of the last pick.
 * pcr_gmm_em_step_f64: GMM.posterior + GMM.EM of nano_vs_my/sript/GMM.py:43-78.  gamma_nk proportional to pi_k N(x_n; mu_k, Sigma_k), evaluated
 *   in the LOG domain: Sigma_k = L L^T (Cholesky), log p = log pi_k - (dim log 2 pi + log det Sigma_k) / 2 - |L^-1 (x - mu_k)|^2 / 2, and
 *   a log-sum-exp over k.  N_k = sum gamma, pi = N_k / n, mu_new = sum gamma x / N_k, Sigma_new = sum (gamma (x - mu_new)) (x - mu_new)^T / N_k
 *   around the NEW mean, from the stored gamma in a second pass.  A covariance that is not positive definite is PCR_ERR_STATE (scipy raises).
 *   DIFFERS from the reference where its plain pdf underflows: a row whose every pi_k pdf is 0 is 0 / 0 = NaN there, and a well-defined
 *   posterior here.  post (n x k, may be NULL) receives gamma.
 * pcr_gmm_fit_f64: GMM.fit.  Initial Sigma = amplitude I, pi = 1 / k, mu = init_mean (hw3/sript/GMM.py: amplitude 0.3, eps 1e-4;
 *   nano_vs_my/sript/GMM.py: 1 and 1e-3).  After each EM pass: a component with ||Sigma_k||_F < 0.01 gets Sigma_k = amplitude I and
 *   mu_k = data[K(seed, count << 32 | k) mod n] (the reference draws unseeded; *resets counts how often this fired); the loop ends when
 *   the max-abs differences of mean, covariance and pi are all < eps (*converged = 1) or when count == max_iter.  *iters = count.
 * pcr_gmm_predict_f64: argmax_k of the log posterior, the first maximum wins (GMM.predict). */
#define PCR_EMPTY_CLUSTER 1  /* positive: the call completed, a cluster has no member */
#define PCR_KMEANS_PY 0
#define PCR_KMEANS_CPP 1
typedef struct pcr_mat64 pcr_mat64;
int pcr_mat64_create(pcr_ctx* ctx, const double* rows, size_t n, int dim, pcr_mat64** out);
int pcr_mat64_destroy(pcr_ctx* ctx, pcr_mat64* m);
int pcr_mat64_info(const pcr_mat64* m, size_t* n, int* dim, int* grid_exponent);   /* grid_exponent = e above */
int pcr_kmeans_step_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* centres_in, int32_t* labels, int64_t* counts, double* centres_out);
int pcr_kmeans_fit_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* init_centres, double tol, int max_iter, int mode, double* centres,
                       int32_t* labels, int* iters, int* converged);
int pcr_kmeans_predict_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* centres, int32_t* labels);
int pcr_kmeanspp_init_f64(pcr_ctx* ctx, pcr_mat64* data, int k, double factor, const double* u, uint64_t seed, int32_t* idx_out, double* p_last);
int pcr_gmm_em_step_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* mean_in, const double* cov_in, const double* pi_in, double* mean_out,
                        double* cov_out, double* pi_out, double* post);
int pcr_gmm_fit_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* init_mean, double amplitude, double eps, int max_iter, uint64_t seed,
                    double* mean, double* cov, double* pi, int* iters, int* converged, int* resets);
int pcr_gmm_predict_f64(pcr_ctx* ctx, pcr_mat64* data, int k, const double* mean, const double* cov, const double* pi, int32_t* labels);

/* ---- Homework3: spectral clustering (csrc/spectral.hip, csrc/numerics.cpp) -----------------------------------------------
 * Spec_Cluster::fit of Homework3/hw3/spectralClustering.cpp: kNN graph -> random-walk Laplacian L = I - D^-1 W -> the eigenpairs of L with
 * the smallest real part -> K by the eigengap rule -> K-Means (PCR_KMEANS_CPP above) on the first K eigenvector columns.  All f64 over a
 * pcr_mat64.  Every sum runs in a fixed order (no floating-point atomics): a call repeats bit for bit.
 *
 * pcr_mat64_knn_f64: the k nearest rows of every row among ALL rows, the row itself included (nanoflann's findNeighbors returns it).
 *   d2 = sum_dim (a - b) (a - b), accumulated from 0 in dimension order, unfused; results ascending by (d2, index); 1 <= k <= 32, k <= n.
 *   idx (int32) and d2: n x k, host.  Exhaustive and tiled (targets through LDS, the result set of a row in registers); d2 must not overflow.
 * pcr_spectral_graph_f64: buildKNNGraph (:53-119).  Row i holds 1 on the diagonal and -(w_ij / s_i) for every neighbour j != i of its
 *   k_neighbors nearest rows (only the row's own index is skipped, :90), w_ij = 1 / sqrt(d2_ij), s_i = the w of the row added in ascending
 *   column order starting from 0.  Columns ascending within a row; every row has k_neighbors entries.  2 <= k_neighbors <= 32.
 *   A neighbour at distance 0 (a duplicate point: inf / NaN in the reference) gives the positive status PCR_SPECTRAL_DUPLICATE and no graph.
 *   pcr_spgraph_read copies the CSR arrays to the host (row_ptr: n + 1, col / val: nnz; each may be NULL); pcr_spgraph_info reports n and nnz.
 *   buildRNNGraph (:122-161) is never called by the reference and is not provided.
 * pcr_eig_small_f64 (host, no GPU): every eigenpair of a real n x n matrix (row-major, 1 <= n <= 16): Householder -> Hessenberg, shifted QR
 *   with accumulated transformations, back-substitution.  Eigenvalues (wr, wi) ascending by real part, a conjugate pair adjacent with the
 *   positive imaginary part first.  vectors (n x n row-major, may be NULL): column j is the unit eigenvector of a real eigenvalue; for a pair
 *   at (j, j + 1) the columns are the real and the imaginary part of the unit vector of wr[j] + i wi[j].  PCR_ERR_STATE: no convergence.
 * pcr_spectral_embed_f64: the n_eig eigenpairs of L with the smallest real part, by block iteration with n_basis orthonormal columns on the
 *   damped walk A = I - L / 2 (re-orthonormalised every 8 steps, Cholesky-QR on the device), a Rayleigh-Ritz step on T = Q^T L Q
 *   (pcr_eig_small_f64) every 256 steps, and the stop rule max_j |L v_j - theta_j v_j| <= tol over the n_eig unit Ritz vectors.
 *   1 <= n_eig <= n_basis <= 16, n_basis <= n; 0 selects the defaults 8 and n_eig + 5 (clamped); tol <= 0: 1e-10; max_iter <= 0: 400 000 steps.
 *   n <= 4 096: one persistent workgroup runs all steps between two Ritz checks in one launch; larger n: one launch per step over all CUs.
 *   eigenvalues: n_eig real parts, ascending.  vectors: n x n_eig row-major, unit 2-norm, the component of largest magnitude (the first
 *   such) positive.  A complex Ritz pair among the n_eig is flagged in info->complex_mask (bit j: column j belongs to a pair; its two
 *   columns hold the real and the imaginary part of the unit complex vector, the real part's largest component positive) and its imaginary
 *   part stands in info->eigenvalues_im.  Positive status PCR_SPECTRAL_NOT_CONVERGED when max_iter ends first (outputs = the last Ritz pairs).
 *   A pair that n_eig cuts is completed inside while n_eig < n_basis (bit n_eig - 1 is set, column n_eig - 1 is the real part of the unit
 *   complex vector); with n_basis == n_eig there is no room, its first member is then treated as real and the call ends NOT_CONVERGED.
 *   n <= 32 with n_basis == 0: no iteration.  L is read back as a dense matrix and the host solves it whole (the algorithm of
 *   pcr_eig_small_f64 after a permutation that isolates eigenvalues): same outputs, solver_steps = 0, n_basis = 0 and one_workgroup = 0 in
 *   info, residual <= tol decides between PCR_OK and NOT_CONVERGED as above.  Block iteration cannot serve every such graph: L of a 2-row
 *   cloud has the eigenvalue 2, which A maps to 0, and with k_neighbors = 2 (every row has one neighbour, mutual pairs give the eigenvalues
 *   0 and 2, the rows hanging off them Jordan blocks at 1) L is defective.  A given n_basis always asks for the iteration: it returns
 *   PCR_ERR_STATE when Cholesky-QR meets a pivot <= 0 (rank((I - L/2)^8) < n_basis: n_basis near n, or such a graph), and on a defective L of
 *   any size it either stalls near a residual of 1e-8 or stops at tol with an eigenvalue off by up to 1e-3 (a Jordan block of size m turns a
 *   residual r into an eigenvalue error near r^(1/m)).  k_neighbors = 2 above 32 rows is therefore accepted but not served accurately.
 * pcr_spectral_select_k (host): the eigengap rule of :188-197 as written — diff = e[1] - e[0]; the first i >= 1 with e[i + 1] - e[i] >
 *   50 diff gives K = i + 1 — reading e[i + 1] only while i + 1 < n_eig (the reference reads one past its vector); 1 if no gap fires.
 * pcr_spectral_cluster_f64: graph, embedding (n_eig, its default basis, tol 1e-10), K = n_clusters if > 0 else the rule (K <= min(8, n_eig)),
 *   initial_choice (:249-289: row 0, then every row whose squared distance to each chosen row is >= 1e-4, until K are chosen; on the host
 *   over the n x K features) — PCR_SPECTRAL_FEW_SEEDS if fewer than K exist —, then pcr_kmeans_fit_f64(PCR_KMEANS_CPP, tol 1e-4, 200).
 *   PCR_SPECTRAL_COMPLEX if a complex pair falls inside the K columns (the reference takes .real() of an arbitrary phase there).
 *   labels: n int32.  features (may be NULL): n x K.  info (may be NULL) carries K, the eigenvalues, steps, residual and K-Means passes; it is
 *   written once the graph exists, and holds zeros in every byte when the embedding then refuses its arguments (n_eig > n).  A call that
 *   fails before that (arguments, PCR_SPECTRAL_DUPLICATE) leaves it untouched. */
#define PCR_SPECTRAL_DUPLICATE 2
#define PCR_SPECTRAL_COMPLEX 3
#define PCR_SPECTRAL_NOT_CONVERGED 4
#define PCR_SPECTRAL_FEW_SEEDS 5
typedef struct pcr_spgraph pcr_spgraph;
typedef struct {
    int32_t k_clusters;          /* K used by pcr_spectral_cluster_f64 (0 from pcr_spectral_embed_f64) */
    int32_t n_eig, n_basis;
    int32_t solver_steps;        /* applications of A */
    int32_t one_workgroup;       /* 1: the persistent single-workgroup path served the iteration */
    int32_t kmeans_iters, kmeans_converged;
    uint32_t complex_mask;
    double residual;             /* the largest |L v - theta v| over the n_eig Ritz pairs at the last check */
    double eigenvalues[16], eigenvalues_im[16];
} pcr_spectral_info;
int pcr_mat64_knn_f64(pcr_ctx* ctx, pcr_mat64* data, int k, int32_t* idx, double* d2);
int pcr_spectral_graph_f64(pcr_ctx* ctx, pcr_mat64* data, int k_neighbors, pcr_spgraph** out);
int pcr_spgraph_info(const pcr_spgraph* g, size_t* n, size_t* nnz);
int pcr_spgraph_read(pcr_ctx* ctx, const pcr_spgraph* g, int64_t* row_ptr, int32_t* col, double* val);
int pcr_spgraph_destroy(pcr_ctx* ctx, pcr_spgraph* g);
int pcr_eig_small_f64(int n, const double* a, double* wr, double* wi, double* vectors);
int pcr_spectral_embed_f64(pcr_ctx* ctx, pcr_spgraph* graph, int n_eig, int n_basis, double tol, int max_iter, double* eigenvalues, double* vectors,
                           pcr_spectral_info* info);
int pcr_spectral_select_k(const double* eigenvalues, int n_eig);
int pcr_spectral_cluster_f64(pcr_ctx* ctx, pcr_mat64* data, int k_neighbors, int n_eig, int n_clusters, int32_t* labels, double* features,
                             pcr_spectral_info* info);

/* ---- profiling hooks for bench.py: HIP-event timing of the dominant kernel on the ctx stream ----------
 * Off by default (an event pair costs ~6 us of stream time on each side of the kernel it brackets):
 * pcr_tune_set(ctx, "prof", 1) times the correspondence kernels, 2 every kernel, 0 switches it off again. */
int pcr_prof_reset(pcr_ctx* ctx);
int pcr_prof_get(pcr_ctx* ctx, const char* kernel, uint64_t* launches, double* total_ms);
/* the individual durations (ms, launch order, at most 4096 since the last reset): *n = how many exist, ms[0 .. min(*n, cap)) filled */
int pcr_prof_get_each(pcr_ctx* ctx, const char* kernel, double* ms, size_t cap, size_t* n);
/* diagnostics of the last grid search launched with tune "grid_stats" = 1:
 * out = { candidates evaluated, fine x-rows opened, coarse rows tested, far stages run } summed over the queries */
int pcr_grid_stats(pcr_ctx* ctx, uint64_t out[4]);
/* the sixteen diagnostics words of the last 1-NN launch made with tune "grid_stats" = 1.  Cell walk: [0..3] as pcr_grid_stats.
 * Matrix-core exhaustive search (HTRACK / BTRACK): [2] = (wave, query group) pairs that were filtered a second time, [4] = shader
 * cycles (s_memtime) and [5] = 100 MHz real-time ticks (s_memrealtime) summed over the workgroups: [4] / [5] x 100 MHz is the shader
 * clock the chip held under that launch (bench.py: the clock-corrected roofline).  STRACK (the sign form of the f16 filter): [2] =
 * joint evaluations of a wave's list of flagged chunks, [6] = (query, 16-record chunk) pairs evaluated exactly, [4] / [5] as above.
 * STRACK3 (csrc/nn1_sphere.hpp) in addition: [7] level-0 MFMAs, [3] level-1 tiles flagged by level 0, [8] level-1 MFMAs, [9] level-2 tiles flagged
 * by level 1, [10] level-2 MFMAs.  Sign tile search (csrc/grid_stile.hpp) + the walk of its deferred
 * queries: [0] pairs through the sign filter, [1] coarse cells read, [2] tile spheres tested, [3] operand setups, [4] / [5] box / ball (um,
 * summed), [6] queries deferred, [7] passes, [8] exact evaluations, [9] joint evaluations, [10] records under listed tiles, [11] MFMAs,
 * [12] most tiles in a pass, [13] / [14] / [15] deferred because: beyond the ball limit / more clusters than passes / list overflow. */
int pcr_nn1_stats(pcr_ctx* ctx, uint64_t out[16]);
/* Checks on THIS device the arithmetic the matrix-core forms of the exhaustive 1-NN filter rely on (csrc/nn1_brute.hip: BTRACK = two
 * v_mfma_f32_32x32x16_bf16 per tile, three-piece operands; HTRACK = one v_mfma_f32_32x32x16_f16, two-piece scaled operands — the default).
 * `trials` random tiles per mode plus 4 structured (cancellation across K-slots, alternating signs, subnormal pieces, maximal exponent
 * spread) and 8 underflow-regime tiles, through the kernel's own MFMA(s) and operand code; u = 2^-24:
 *   worst[0] = max |D - exact| / (u sum |a_k b_k|), random operands                                   (the bounds assume <= 16)
 *   worst[1] = max (|G - (w - 2 r.t)| - 2 u) / (u (|r|^2 + |t|^2)), the kernel's operand layout       (assume <= 34.2 bf16 / <= 82 f16)
 *   worst[2] = max |G - (w - 2 r.t)| / u over pairs with |r|^2 + |t|^2 <= 2^-6 (f16 underflow regime)  (HTRACK subtracts 4 u)
 *   worst[3] = as worst[0] on the structured tiles                                                    (<= 16) */
int pcr_selftest_mfma_bf16_v2(pcr_ctx* ctx, int trials, double worst[4]);
int pcr_selftest_mfma_f16_v2(pcr_ctx* ctx, int trials, double worst[4]);
/* the round-2 forms of the same self-tests: worst[0] and worst[1] only (a caller built against the older header passes two doubles) */
int pcr_selftest_mfma_bf16(pcr_ctx* ctx, int trials, double worst[2]);
int pcr_selftest_mfma_f16(pcr_ctx* ctx, int trials, double worst[2]);
/* The DECISION of the sign form of the f16 filter (STRACK, csrc/nn1_brute.hip — the default exhaustive search on targets that fit f16:
 * the query's threshold rides in two K-slots, an accumulator is bound - threshold, its sign bit says whether the record can matter),
 * checked on THIS device: `trials` random super-tile tiles + 8 in the f16 underflow regimes, a power-of-two scale per tile, thresholds
 * ON the exact distance of one pair, one ulp below / above it and a factor away, through the kernel's own operand code and MFMA.
 * out = { pairs whose exact f32 distance lies at or below their query's threshold, of those WITHOUT the sign — must be 0 —,
 * pairs with the sign set, pairs in all }.  A short form is part of the once-per-context check below. */
int pcr_selftest_sign_f16(pcr_ctx* ctx, int trials, uint64_t out[4]);
/* The SPHERE statement of the hierarchical form of that filter (STRACK3, csrc/nn1_sphere.hpp: one MFMA row per set of records — its bounding
 * sphere — before any per-record row): `trials` random level-1 tiles of 32 chunks (tight and wide clusters, chunks spread beyond the scaled
 * range, empty chunks, non-finite records) against 32 queries each (near, inside, far, beyond the clamp) with thresholds on / one ulp off / a
 * factor off exact distances and zero, through the index build's operand code, the kernel's query code and the MFMA.
 * out = { (query, chunk) pairs with a record at or below the threshold, of those WITHOUT the sign (must be 0), pairs flagged, pairs }. */
int pcr_selftest_sphere_f16(pcr_ctx* ctx, int trials, uint64_t out[4]);
/* The library runs a short form of the two self-tests ITSELF, once per context, before it first picks a matrix-core kernel, and only
 * uses a form whose four figures stay within HALF of what its bound assumes (f16 -> bf16 -> the f32 filters, whose bounds need IEEE
 * arithmetic only).  This reports the verdicts (-1 = not run yet; run_now != 0 runs them), the figures, the host time the checks
 * took, and which 1-NN kernel family served the last search ("strack3", "strack", "htrack", "btrack", "etrack", "ftrack",
 * "track", "grid", "grid-stile"). */
typedef struct {
    int32_t f16_ok, bf16_ok;
    double f16_worst[4], bf16_worst[4];
    double check_ms;
    char last_nn1_kernel[16];
} pcr_mfma_check;
int pcr_ctx_mfma_check(pcr_ctx* ctx, int run_now, pcr_mfma_check* out);
/* Tuning / diagnostic knobs by name.  A value of 0 means "library default" for every key except "prof"; results never depend on a knob
 * (the parity tests run the switches against each other), only speed and which kernel serves a call.  Defaults in brackets.
 *  dispatch    nn_method [0 auto: api.cpp nn1_auto_grid] 1 exhaustive / 2 exact grid · nn1_variant [0: table above launch_nn1_brute,
 *              csrc/nn1_brute.hip] 1 FTRACK, 2 TRACK (exact arithmetic only), 4 ETRACK, 6 BTRACK, 7 HTRACK, 8 STRACK for every search
 *              that has or can make itself a seed (HTRACK otherwise), 10 STRACK3 (the sphere form on targets of any size; 9 = its old number) ·
 *              nn1_bf16, nn1_f16 [on] 1 force / 2 forbid the matrix-core forms ·
 *              nn1_sign [on: the sign forms for every search on a target that fits f16 — a cold one seeds itself] 2 = never (HTRACK) ·
 *              nn1_sphere [0: STRACK3 from 32 768 target points] 1 always / 2 never (STRACK) ·
 *              mfma_force_fail 1 f16 / 2 bf16 / 3 both (tests: a failing device check) ·
 *              knn_method, radius_method [auto] 1 exhaustive / 2 grid · nn1_async_in_loop [off] 1 = pcr_nn1_f32_async calls of one
 *              caller-side loop seed each other as the searches inside pcr_icp_p2p_f32 do
 *  exhaustive  nn1_btrack_qg [2 up to 49 152 queries, else 4] · nn1_supers_per_slice [from nn1_btrack_blocks = 14 336] ·
 *              nn1_sign_flush [64: entries of a wave's list of flagged chunks from which the end of a super-tile evaluates them] ·
 *              nn1_sign_dense [12: flagged half-lanes of one (group, tile) from which they evaluate their chunk in place] ·
 *              nn1_sphere_qg [1: groups of 32 queries per STRACK3 wave] 2 / 4 · nn1_sphere_flush_end [1: entries from which the end of
 *              a level-1 super-tile evaluates them] · nn1_sphere_l0_per_slice [from nn1_sphere_blocks = 1 024] ·
 *              nn1_s3_transposed [1: STRACK3 reads its sphere-row masks from one ballot of the transposed product] 2 = one ballot per accumulator ·
 *              nn1_xcd [4] 1 / 2 / 4, -1 plain launch · nn1_cold_seed [on] 2 = off, 3 = round 3's rule (sliced launches only) ·
 *              nn1_seed_mode [0: centre of the nearest super-tile + Morton neighbour for a cold search, the centre alone beside stale correspondences]
 *              1 centre / 2 Morton neighbour / 3 both · nn1_seed_levels [2: the centre scan goes through the level-1 super-tiles' centres first] 1 = all centres · nn1_sphere_reseed [on] 2 = a warm search of the sphere forms keeps stale seeds as they are ·
 *              bt_sort_begin_bit [0: low bits of the Morton key the working-cloud sort ignores] ·
 *              nn1_warm_start [on] 2 = off · nn1_chunks_per_slice [from
 *              nn1_etrack_blocks = 32 768] · nn1_tiles_per_slice [from nn1_target_blocks = 16 384] · bt_sort_work [on] 2 = off
 *  exact grid  grid_order [0: Morton + bounding spheres from 256 points] 1 x-sorted / 2 Morton · grid_mode [by index] 1 plain / 2 x-window / 3 spheres ·
 *              grid_lanes [16] · grid_cell_um, grid_cell_scale_x100 [150 for Morton], grid_occupancy_x10 [20], grid_max_cells ·
 *              grid_sort_queries, grid_sort_work, grid_warm_start, grid_wpos, grid_seed_run, grid_far_brute [on] 2 = off ·
 *              grid_sort_fine [auto] 1 / 2 · grid_query_bins_log2 [22], grid_query_bin_min [2] · grid_xcd_run [32 from 4 096 blocks]
 *              -1 = identity · grid_tile [0: the tile search for targets from 4 000 000 points whose working cloud is about as dense as the target] 1 on / 2 off,
 *              grid_tile_reach_pct [200], grid_tile_min_members [8], grid_tile_list_segs [1] (csrc/grid.hip launch_nn1_grid) · knn_cell_scale_x100, knn_slices ·
 *              the sign tile search (csrc/grid_stile.hpp, what grid_tile selects): grid_stile [on] 2 = off, the cell walk ·
 *              grid_stile_cbits [9: bits per axis of the coarse Morton cells] · bt_fine_bits [6 from 2^20 points] · grid_stile_bmax_cm [100],
 *              grid_stile_lim_pct [400], grid_stile_lim_floor_mm [150], grid_stile_split_mm [40] (ball limits of a pass) · grid_stile_keep [768],
 *              grid_stile_keep_small [192], grid_stile_cells [2 048] (tiles / cells a pass may hold) · grid_stile_flush [64], grid_stile_dense [32] ·
 *              grid_stile_passes [3] · grid_stile_queue [on] 2 = static list walk, grid_stile_list_wgs [8 per CU] ·
 *              grid_stile_l1 [on: per-record operands in the scale of the level-1 super-tiles] 2 = the 256-record super-tiles' ·
 *              grid_stile_cold [on] 2 = off, grid_stile_cold_own [32], grid_stile_cold_per [4] (cold seeds from the coarse cells)
 *  ICP loop    icp_pipeline [0 = 1 device-resident] -1 synchronous · icp_chunk [4] · icp_bounded_search [on] 2 = off ·
 *              icp_fused_move [on] 2 = off, icp_fused_max [262 144] · icp_seed_in_move [on] 2 = off · icp_force_slots (tests) ·
 *              icp_fused_sums [on] 2 = off (exhaustive loops: the sums in the solve + move launch, one grid barrier), icp_fused_sums_min [60 000 points],
 *              icp_fused_sums_max_blocks [CUs of the device], icp_fused_sums_threads [512] 256, icp_fused_sums_grid [off] 1 = grid loops too ·
 *              icp_host_snapshots [on where the chain is 4: the sums + solve launch writes the state snapshots into pinned host memory] 2 = copies and
 *              events on the stream · icp_ticket_levels [1: one arrival counter for that launch] 2 = one per accumulator replica ·
 *              kabsch_bfly [on], kabsch_records [on], kabsch_one_pair_blocks [128], kabsch_max_blocks [1 024]
 *  other       plane_group [20: hypotheses per workgroup row of the plane count] · iss_lanes [32] · fpfh_lanes [16] · harris_lanes [16] · radius_fused [on] 2 = off · grid_stats 1 = the next 1-NN launch fills pcr_nn1_stats · prof 0 / 1 / 2 / 3 (3 = 2 plus one
 *              radius_emit_class scope per length-class launch inside radius_emit) */
int pcr_tune_set(pcr_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* PCR_H */
