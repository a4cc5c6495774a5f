// cluster.hip — Homework4's foreground stage on the GPU: DBSCAN (foreground_pcd.cluster_dbscan(0.8, 20),
// Homework4/ground_detection_SVD.py:173) and the statistical outlier removal of pcd_preprocessing (:22-37,
// remove_statistical_outlier(nb_neighbors = 20, std_ratio = 2.7)).
//
// Arithmetic of both = pcr_cloud_knn_f64: s = ((dx*dx) + dy*dy) + dz*dz on the f32 coordinates widened to f64, unfused.
//
// DBSCAN — five passes over the uniform grid with cell edge >= eps, so that N(p) lies in the 27-cell block of p's cell (the
// walk: grid_walk.hpp).  The cloud is searched against itself: query p IS grid record p, G lanes share one query and
// stride over each x-row, long rows are clipped to the x window of the query.  No neighbour list is ever stored: O(n) memory.
//   count   cnt[p] = |N(p)| (p included), core[p] = finite && cnt >= min_points
//   union   every core record p unions itself with each core neighbour j < p (record numbering: lock-free union-find, below)
//   final   full pointer jumping (root[p]), key[root] = min original index of the component's core points
//   border  a non-core record with a neighbour takes the smallest key over its core neighbours' components
//   label   flag[i] = core(i) && key[root(i)] == i (input numbering); exclusive scan = cluster ids in ascending key order
// Union-find (union_find.hpp): parent[] in record numbering, parent[x] <= x always (a root is hooked under a SMALLER root by
// atomicCAS(&parent[hi], hi, lo)), so every path strictly decreases and a find takes at most n steps; more means a corrupt
// structure: a device error word is set and the call returns PCR_ERR_STATE.  A failed CAS means another lane hooked `hi`
// first; the union continues from the value the CAS returned.  Hooks succeed at most n - 1 times overall, so the retry loop
// is bounded by n as well.  Finds halve their path with plain atomic stores: a node that is not a root is never hooked
// again, and the grandparent it is pointed at is one of its ancestors for good, so a stale or overwritten shortcut is still a
// shortcut within the same set.  parent[] is read with agent-scope atomic loads (eight XCDs, eight L2s): only the
// per-location order of parent[] itself matters, no other data is published through it, so relaxed order suffices.
//
// SOR — the existing grid k-NN (knn_grid.hip, squared, self included), then per point avg = sum of sqrt over the found slots
// in slot order / found (-1 without a neighbour); the two global sums in a fixed order (a fixed number of workgroups for a
// given n, each a fixed strided sequence + a shuffle tree), mask, exclusive scan, gather into a new device cloud.
#include "grid_walk.hpp"
#include "union_find.hpp"

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int CL_BLOCK = 256;
constexpr uint32_t CL_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ double cl_s(const float4& t, double qx, double qy, double qz)
{
    const double dx = (double)t.x - qx, dy = (double)t.y - qy, dz = (double)t.z - qz;   // t - q, as knn_grid.hip
    return (dx * dx + dy * dy) + dz * dz;
}

// ---------------------------------------------------------------------------------------- DBSCAN
template <int G>
__global__ __launch_bounds__(CL_BLOCK) void db_count_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                            uint32_t n, double eps2, int min_points, uint32_t* __restrict__ cnt_sorted,
                                                            uint8_t* __restrict__ core_sorted, uint32_t* __restrict__ cnt_out, uint8_t* __restrict__ core_out)
{
    const uint64_t pg = ((uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x) / G;     // (n * G may exceed 2^32)
    const int sub = threadIdx.x % G;
    if (pg >= n) return;                                    // whole groups leave together (CL_BLOCK % G == 0)
    const uint32_t p = (uint32_t)pg;
    const float4 q = records[p];
    const bool fin = finite3(q.x, q.y, q.z);
    unsigned c = 0;
    if (fin) {
        const double qx = q.x, qy = q.y, qz = q.z;
        const RadiusWalk walk(g, cell_start, records, query_cell(g, q), x_window_f64(q.x, eps2));
        for (int k = 0; k < 9; k++) {
            uint32_t b, e;
            walk.row<384>(k, b, e);
            for (uint32_t j = b + sub; j < e; j += G) c += cl_s(records[j], qx, qy, qz) <= eps2;
        }
    }
    c = group_sum<G>(c);
    if (sub == 0) {
        const uint8_t core = (fin && (long long)c >= (long long)min_points) ? 1 : 0;
        const uint32_t orig = __float_as_uint(q.w);
        cnt_sorted[p] = c;
        core_sorted[p] = core;
        cnt_out[orig] = c;
        core_out[orig] = core;
    }
}

__global__ __launch_bounds__(CL_BLOCK) void db_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ key, uint32_t n)
{
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    key[i] = CL_NONE;
}

template <int G>
__global__ __launch_bounds__(CL_BLOCK) void db_union_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                            uint32_t n, double eps2, const uint8_t* __restrict__ core_sorted, uint32_t* parent,
                                                            uint32_t* err)
{
    const uint64_t pg = ((uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x) / G;     // (n * G may exceed 2^32)
    const int sub = threadIdx.x % G;
    if (pg >= n) return;                                    // whole groups leave together (CL_BLOCK % G == 0)
    const uint32_t p = (uint32_t)pg;
    if (!core_sorted[p]) return;                            // uniform over the group; core implies finite
    const float4 q = records[p];
    const double qx = q.x, qy = q.y, qz = q.z;
    const RadiusWalk walk(g, cell_start, records, query_cell(g, q), x_window_f64(q.x, eps2));
    uint32_t rp = p;                                        // an ancestor of p (refreshed by every find)
    for (int k = 0; k < 9; k++) {
        uint32_t b, e;
        walk.range(k, b, e);
        e = min(e, p);                                      // each pair once: the larger record links
        if (b >= e) continue;
        walk.clip<384>(b, e);
        for (uint32_t j = b + sub; j < e; j += G) {
            if (!core_sorted[j] || !(cl_s(records[j], qx, qy, qz) <= eps2)) continue;
            rp = uf_find(parent, rp, n, err);
            const uint32_t rj = uf_find(parent, j, n, err);
            if (rp != rj) uf_union(parent, rp, rj, n, err);
        }
    }
}

// full pointer jumping into root[] (no hook can happen any more: roots are final) and the key of every component.  parent[] is
// only read here: a halving store of a lane that read an older grandparent could otherwise overwrite a root written in place
__global__ __launch_bounds__(CL_BLOCK) void db_final_kernel(const float4* __restrict__ records, uint32_t n, const uint8_t* __restrict__ core_sorted,
                                                            uint32_t* parent, uint32_t* __restrict__ root, uint32_t* __restrict__ key, uint32_t* err)
{
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = uf_find<false>(parent, i, n, err);
    root[i] = r;
    if (core_sorted[i]) atomicMin(key + r, __float_as_uint(records[i].w));
}

// bkey[p] = smallest key over the core neighbours of a non-core record p (CL_NONE: none, or p is core)
template <int G>
__global__ __launch_bounds__(CL_BLOCK) void db_border_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                             uint32_t n, double eps2, const uint32_t* __restrict__ cnt_sorted,
                                                             const uint8_t* __restrict__ core_sorted, const uint32_t* __restrict__ root,
                                                             const uint32_t* __restrict__ key, uint32_t* __restrict__ bkey)
{
    const uint64_t pg = ((uint64_t)blockIdx.x * CL_BLOCK + threadIdx.x) / G;     // (n * G may exceed 2^32)
    const int sub = threadIdx.x % G;
    if (pg >= n) return;                                    // whole groups leave together (CL_BLOCK % G == 0)
    const uint32_t p = (uint32_t)pg;
    unsigned m = CL_NONE;
    if (!core_sorted[p] && cnt_sorted[p] >= 2) {            // uniform over the group; a count implies finite
        const float4 q = records[p];
        const double qx = q.x, qy = q.y, qz = q.z;
        const RadiusWalk walk(g, cell_start, records, query_cell(g, q), x_window_f64(q.x, eps2));
        for (int k = 0; k < 9; k++) {
            uint32_t b, e;
            walk.row<384>(k, b, e);
            for (uint32_t j = b + sub; j < e; j += G)
                if (core_sorted[j] && cl_s(records[j], qx, qy, qz) <= eps2) m = min(m, key[root[j]]);
        }
    }
    m = group_min<G>(m);
    if (sub == 0) bkey[p] = m;
}

// flag[i] = 1 iff input point i is the key (smallest core index) of its component
__global__ __launch_bounds__(CL_BLOCK) void db_flag_kernel(const float4* __restrict__ records, uint32_t n, const uint8_t* __restrict__ core_sorted,
                                                           const uint32_t* __restrict__ root, const uint32_t* __restrict__ key, uint32_t* __restrict__ flag)
{
    const uint32_t p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t orig = __float_as_uint(records[p].w);
    flag[orig] = (core_sorted[p] && key[root[p]] == orig) ? 1u : 0u;
}

__global__ __launch_bounds__(CL_BLOCK) void db_label_kernel(const float4* __restrict__ records, uint32_t n, const uint8_t* __restrict__ core_sorted,
                                                            const uint32_t* __restrict__ root, const uint32_t* __restrict__ key,
                                                            const uint32_t* __restrict__ bkey, const uint32_t* __restrict__ ids, int32_t* __restrict__ labels)
{
    const uint32_t p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = core_sorted[p] ? key[root[p]] : bkey[p];
    labels[__float_as_uint(records[p].w)] = k == CL_NONE ? -1 : (int32_t)ids[k];
}

// ---------------------------------------------------------------------------------------- statistical outlier removal
constexpr uint32_t SOR_MAX_BLOCKS = 1024;

// sum over the CL_BLOCK threads of a workgroup in a fixed order (shuffle tree inside each wave, then the waves in order)
__device__ __forceinline__ double sor_block_sum(double v, double* lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < CL_BLOCK / 64; w++) t += lds[w];
    __syncthreads();
    return t;                                               // valid in thread 0
}

// avg[i]; per workgroup: sum of the positive avg, number of points with a neighbour
__global__ __launch_bounds__(CL_BLOCK) void sor_avg_kernel(const double* __restrict__ val, const uint32_t* __restrict__ found, uint32_t n, int k,
                                                           double* __restrict__ avg, double* __restrict__ part_sum, double* __restrict__ part_cnt)
{
    __shared__ double lds[CL_BLOCK / 64];
    double s = 0.0, c = 0.0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += gridDim.x * CL_BLOCK) {
        const uint32_t f = found[i];
        double a = -1.0;
        if (f) {
            double acc = 0.0;
            for (uint32_t t = 0; t < f; t++) acc += sqrt(val[(size_t)i * k + t]);
            a = acc / (double)f;
            c += 1.0;
        }
        avg[i] = a;
        if (a > 0) s += a;
    }
    s = sor_block_sum(s, lds);
    c = sor_block_sum(c, lds);
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = s; part_cnt[blockIdx.x] = c; }
}

// per workgroup: sum of (avg - mean)^2 over the positive avg
__global__ __launch_bounds__(CL_BLOCK) void sor_dev_kernel(const double* __restrict__ avg, uint32_t n, const double* __restrict__ stats,
                                                           double* __restrict__ part_sq)
{
    __shared__ double lds[CL_BLOCK / 64];
    const double mean = stats[0];
    double s = 0.0;
    for (uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += gridDim.x * CL_BLOCK) {
        const double a = avg[i];
        if (a > 0) s += (a - mean) * (a - mean);
    }
    s = sor_block_sum(s, lds);
    if (threadIdx.x == 0) part_sq[blockIdx.x] = s;
}

// one workgroup: stage 0 -> stats = {mean, -, -, valid}; stage 1 -> stats[1] = std, stats[2] = mean + std_ratio std
__global__ __launch_bounds__(CL_BLOCK) void sor_stats_kernel(const double* __restrict__ part_a, const double* __restrict__ part_b, uint32_t nb, int stage,
                                                             double std_ratio, double* __restrict__ stats)
{
    __shared__ double lds[CL_BLOCK / 64];
    double a = 0.0, b = 0.0;
    for (uint32_t i = threadIdx.x; i < nb; i += CL_BLOCK) {
        a += part_a[i];
        if (stage == 0) b += part_b[i];
    }
    a = sor_block_sum(a, lds);
    b = sor_block_sum(b, lds);
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        stats[0] = a / b;                                   // mean over the valid points (Open3D: / valid_distances)
        stats[3] = b;
    } else {
        const double sd = sqrt(a / (stats[3] - 1.0));
        stats[1] = sd;
        stats[2] = stats[0] + std_ratio * sd;
    }
}

__global__ __launch_bounds__(CL_BLOCK) void sor_mask_kernel(const double* __restrict__ avg, uint32_t n, const double* __restrict__ stats,
                                                            uint8_t* __restrict__ keep, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double a = avg[i];
    const bool k = a > 0 && a < stats[2];
    keep[i] = k ? 1 : 0;
    flag[i] = k ? 1u : 0u;
}

// kept points in ascending input order, then the padding of the new cloud (x = +inf)
__global__ __launch_bounds__(CL_BLOCK) void sor_gather_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              uint32_t n, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                              uint32_t n_kept, uint32_t cap, float* __restrict__ ox, float* __restrict__ oy,
                                                              float* __restrict__ oz)
{
    const uint32_t i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i < n && flag[i]) {
        const uint32_t o = pos[i];
        ox[o] = x[i]; oy[o] = y[i]; oz[o] = z[i];
    }
    const uint32_t t = n_kept + i;
    if (t < cap) { ox[t] = __builtin_inff(); oy[t] = 0.0f; oz[t] = 0.0f; }
}

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_dbscan_f32(pcr_ctx* ctx, const pcr_cloud* cloud, double eps, int min_points, int32_t* labels, uint8_t* is_core,
                              uint32_t* neighbor_counts, uint64_t* n_clusters)
{
    if (!ctx || !cloud) return fail(ctx, PCR_ERR_ARG, "pcr_dbscan_f32");
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(ctx, PCR_ERR_ARG, "pcr_dbscan_f32: eps must be finite and >= 0");
    const size_t n = cloud->n;
    if (n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_dbscan_f32: cloud too large");
    if (n && !labels) return fail(ctx, PCR_ERR_ARG, "pcr_dbscan_f32: labels is required");
    if (n_clusters) *n_clusters = 0;
    if (n == 0) return PCR_OK;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const double eps2 = eps * eps;
    Grid* g = nullptr;
    {
        ProfScope ps(ctx, "dbscan_grid", 1);
        int rc = grid_build(ctx, cloud, &g, radius_cell_edge(eps));
        if (rc) return rc;
    }
    const GridPtr g_owner(g);
    if ((double)g->p.h < eps * 1.005) return fail(ctx, PCR_ERR_STATE, "pcr_dbscan_f32: grid cell smaller than eps");
    uint32_t *cnt_sorted, *cnt_out, *parent, *root, *key, *bkey, *flag, *ids, *totals, *n_ids, *err;
    int32_t* lab_out;
    uint8_t *core_sorted, *core_out;
    Layout L;
    L.add(&cnt_sorted, n);
    L.add(&cnt_out, n);
    L.add(&parent, n);
    L.add(&root, n);
    L.add(&key, n);          // indexed by root record, value = original index
    L.add(&bkey, n);
    L.add(&flag, n);         // input numbering
    L.add(&ids, n);          // input numbering
    L.add(&lab_out, n);
    L.add(&core_sorted, n);
    L.add(&core_out, n);
    L.add(&totals, scan_blocks(n));
    L.add(&n_ids, 1);        // the scan's grand total: the number of clusters
    L.add(&err, 1);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    const dim3 grid1((unsigned)((n + CL_BLOCK - 1) / CL_BLOCK));
    hipError_t e = hipMemsetAsync(err, 0, 4, ctx->stream);
    const int G = (int)tune_get(ctx, "dbscan_lanes", 32);    // lanes per query
#define PCR_DB(GG)                                                                                                                     \
    {                                                                                                                                  \
        const dim3 gridg((unsigned)((n * GG + CL_BLOCK - 1) / CL_BLOCK));                                                              \
        { ProfScope ps(ctx, "dbscan_count", 1);                                                                                        \
          hipLaunchKernelGGL((db_count_kernel<GG>), gridg, dim3(CL_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, (uint32_t)n, eps2, \
                             min_points, cnt_sorted, core_sorted, cnt_out, core_out); }                                                \
        { ProfScope ps(ctx, "dbscan_union", 1);                                                                                        \
          hipLaunchKernelGGL(db_init_kernel, grid1, dim3(CL_BLOCK), 0, ctx->stream, parent, key, (uint32_t)n);                         \
          hipLaunchKernelGGL((db_union_kernel<GG>), gridg, dim3(CL_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, (uint32_t)n, eps2, \
                             core_sorted, parent, err);                                                                                \
          hipLaunchKernelGGL(db_final_kernel, grid1, dim3(CL_BLOCK), 0, ctx->stream, g->records, (uint32_t)n, core_sorted, parent, root, key, err); } \
        { ProfScope ps(ctx, "dbscan_border", 1);                                                                                       \
          hipLaunchKernelGGL((db_border_kernel<GG>), gridg, dim3(CL_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, (uint32_t)n, eps2, \
                             cnt_sorted, core_sorted, root, key, bkey); }                                                            \
    }
    switch (G) {
    case 1: PCR_DB(1) break;
    case 2: PCR_DB(2) break;
    case 4: PCR_DB(4) break;
    case 8: PCR_DB(8) break;
    case 16: PCR_DB(16) break;
    default: PCR_DB(32) break;
    }
#undef PCR_DB
    if (e == hipSuccess) e = hipGetLastError();
    {
        ProfScope ps(ctx, "dbscan_label", 1);
        hipLaunchKernelGGL(db_flag_kernel, grid1, dim3(CL_BLOCK), 0, ctx->stream, g->records, (uint32_t)n, core_sorted, root, key, flag);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && exclusive_scan_u32(ctx, flag, ids, n, totals, n_ids)) e = hipErrorUnknown;
        hipLaunchKernelGGL(db_label_kernel, grid1, dim3(CL_BLOCK), 0, ctx->stream, g->records, (uint32_t)n, core_sorted, root, key, bkey, ids, lab_out);
    }
    uint32_t words[2] = { 0, 0 };                           // error word, clusters
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(labels, lab_out, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && is_core) e = hipMemcpyAsync(is_core, core_out, n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && neighbor_counts) e = hipMemcpyAsync(neighbor_counts, cnt_out, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&words[0], err, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&words[1], n_ids, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_dbscan_f32", e);
    prof_flush(ctx);
    if (words[0]) return fail(ctx, PCR_ERR_STATE, "pcr_dbscan_f32: union-find bound exceeded (corrupt structure)");
    if (n_clusters) *n_clusters = words[1];
    return PCR_OK;
}

extern "C" int pcr_statistical_outlier_f32(pcr_ctx* ctx, const pcr_cloud* cloud, int nb_neighbors, double std_ratio, uint8_t* keep, double* avg_dist,
                                           double stats3[3], uint64_t* n_kept, pcr_cloud** kept_cloud)
{
    if (kept_cloud) *kept_cloud = nullptr;
    if (!ctx || !cloud) return fail(ctx, PCR_ERR_ARG, "pcr_statistical_outlier_f32");
    if (nb_neighbors < 1 || nb_neighbors > 32) return fail(ctx, PCR_ERR_ARG, "pcr_statistical_outlier_f32: nb_neighbors must be in [1, 32]");
    if (!(std_ratio > 0.0) || std::isinf(std_ratio)) return fail(ctx, PCR_ERR_ARG, "pcr_statistical_outlier_f32: std_ratio must be finite and > 0");
    const size_t n = cloud->n;
    if (n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_statistical_outlier_f32: cloud too large");
    if (n_kept) *n_kept = 0;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        if (stats3) stats3[0] = stats3[1] = stats3[2] = NAN;    // Open3D: 0 / 0
        if (!kept_cloud) return PCR_OK;
        float dummy = 0.f;
        return pcr_cloud_create(ctx, &dummy, 0, PCR_SOA, kept_cloud);
    }
    const int k = nb_neighbors;
    void* res = nullptr;
    int32_t* idx_dev = nullptr;
    double* val_dev = nullptr;
    uint32_t* found_dev = nullptr;
    int rc;
    {
        ProfScope ps(ctx, "sor_knn", 1);
        rc = knn_grid_device(ctx, cloud, cloud, k, INFINITY, true, 1.7976931348623157e308, -1, &res, &idx_dev, &val_dev, &found_dev);
    }
    if (rc) return rc;
    const uint32_t nblk = (uint32_t)std::min<size_t>(SOR_MAX_BLOCKS, (n + CL_BLOCK - 1) / CL_BLOCK);    // a function of n only: fixed sum order
    double *avg, *part_a, *part_b, *part_sq, *stats;
    uint32_t *flag, *pos, *totals, *n_kept_dev;
    uint8_t* keep_dev;
    Layout L;
    L.add(&avg, n);
    L.add(&flag, n);
    L.add(&pos, n);
    L.add(&keep_dev, n);
    L.add(&part_a, SOR_MAX_BLOCKS);
    L.add(&part_b, SOR_MAX_BLOCKS);
    L.add(&part_sq, SOR_MAX_BLOCKS);
    L.add(&stats, 4);        // mean, std, threshold, valid count (sor_stats_kernel)
    L.add(&totals, scan_blocks(n));
    L.add(&n_kept_dev, 1);
    rc = bind_scratch(ctx, L);
    if (rc) { hipFree(res); return rc; }
    const dim3 grid1((unsigned)((n + CL_BLOCK - 1) / CL_BLOCK));
    {
        ProfScope ps(ctx, "sor_stats", 1);
        hipLaunchKernelGGL(sor_avg_kernel, dim3(nblk), dim3(CL_BLOCK), 0, ctx->stream, val_dev, found_dev, (uint32_t)n, k, avg, part_a, part_b);
        hipLaunchKernelGGL(sor_stats_kernel, dim3(1), dim3(CL_BLOCK), 0, ctx->stream, part_a, part_b, nblk, 0, std_ratio, stats);
        hipLaunchKernelGGL(sor_dev_kernel, dim3(nblk), dim3(CL_BLOCK), 0, ctx->stream, avg, (uint32_t)n, stats, part_sq);
        hipLaunchKernelGGL(sor_stats_kernel, dim3(1), dim3(CL_BLOCK), 0, ctx->stream, part_sq, part_sq, nblk, 1, std_ratio, stats);
        hipLaunchKernelGGL(sor_mask_kernel, grid1, dim3(CL_BLOCK), 0, ctx->stream, avg, (uint32_t)n, stats, keep_dev, flag);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && exclusive_scan_u32(ctx, flag, pos, n, totals, n_kept_dev)) e = hipErrorUnknown;
    double st[4] = { 0, 0, 0, 0 };
    uint32_t kept = 0;
    if (e == hipSuccess && keep) e = hipMemcpyAsync(keep, keep_dev, n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && avg_dist) e = hipMemcpyAsync(avg_dist, avg, n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(st, stats, sizeof(st), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&kept, n_kept_dev, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipFree(res);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_statistical_outlier_f32", e);
    if (stats3) { stats3[0] = st[0]; stats3[1] = st[1]; stats3[2] = st[2]; }
    if (n_kept) *n_kept = kept;
    if (kept_cloud) {
        pcr_cloud* out = nullptr;
        rc = cloud_alloc(ctx, kept, &out);
        if (rc) return rc;
        {
            ProfScope ps(ctx, "sor_gather", 1);
            const size_t span = std::max(n, out->cap);        // every input point and every padding slot of the output
            hipLaunchKernelGGL(sor_gather_kernel, dim3((unsigned)((span + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(),
                               cloud->z(), (uint32_t)n, flag, pos, kept, (uint32_t)out->cap, out->x(), out->y(), out->z());
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { pcr_cloud_destroy(ctx, out); return fail(ctx, PCR_ERR_HIP, "pcr_statistical_outlier_f32: gather", e); }
        *kept_cloud = out;
    }
    prof_flush(ctx);
    return PCR_OK;
}
