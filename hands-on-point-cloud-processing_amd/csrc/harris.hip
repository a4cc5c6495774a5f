// harris.hip — Harris3D keypoints (Homework9/hw9/src/registration.cpp:221-250, PCL's HarrisKeypoint3D with the caller's normals) as
// two radius passes over the uniform grid (the walk: grid_walk.hpp).  The contract (neighbourhood, normal moments as exact integer sums,
// response, suppression) is written out above pcr_harris3d_f32 in include/pcr.h; this file follows it operation by operation.
//
//   pass 0  harris_normals   one lane per grid record: its point's normal in RECORD order, scaled by 2^16, as one float4 whose w is 1
//                            for a contributor (three finite components of magnitude <= 2) and 0 otherwise (x = y = z = 0 then)
//   pass 1  harris_response  G lanes per SURFACE point (the queries are the grid records): one walk of the
//                            27-cell block counts |N(i)| and the contributors and adds the six products as integers; a fixed
//                            xor-shuffle tree sums the group and lane 0 turns the sums into the coefficients and the response
//   pass 2  harris_nms       G lanes per surface point: a group whose own response fails the finite / threshold test never walks; the
//                            others walk and leave at the first neighbour with a larger response
//
// The integer q = rint(fl32(a * b) * 2^32) of a product.  With a' = a * 2^16 and b' = b * 2^16 (exact: |a| <= 2), fl32(a' * b') equals
// fl32(a * b) * 2^32 whenever fl32(a * b) is a normal number, and both are below 2^-94 in magnitude (q = 0 either way) when it is not:
// so q = v_rndne_f32(a' * b'), an integer-valued float of magnitude <= 2^34, at the price of ONE vector instruction beyond the
// product.  It is added in f64 (v_cvt_f64_f32 + v_add_f64: exact while a lane's pending terms keep |sum| < 2^53) and a lane moves
// its f64 sums into int64 accumulators before more than 2^18 terms are pending, so that the sums are exact integers for any count.
// Per pair and product: v_mul_f32, v_rndne_f32, v_cvt_f64_f32, v_add_f64.
#include "grid_walk.hpp"

#include <cmath>

namespace pcr {

namespace {

constexpr int HARRIS_BLOCK = 256;
constexpr uint32_t HARRIS_PENDING_MAX = 1u << 18;          // terms a lane adds in f64 before it moves them to int64: 2^18 * 2^34 < 2^53

__device__ __forceinline__ float hr_s(float dx, float dy, float dz) { return ((dx * dx) + dy * dy) + dz * dz; }

__global__ __launch_bounds__(HARRIS_BLOCK) void harris_normals_kernel(const float4* __restrict__ records, uint32_t n, const float* __restrict__ nx,
                                                                      const float* __restrict__ ny, const float* __restrict__ nz,
                                                                      float4* __restrict__ nrec)
{
    const uint32_t p = blockIdx.x * HARRIS_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = __float_as_uint(records[p].w);
    const float x = nx[i], y = ny[i], z = nz[i];
    const bool ok = fabsf(x) <= 2.0f && fabsf(y) <= 2.0f && fabsf(z) <= 2.0f;      // false for NaN / inf
    nrec[p] = ok ? make_float4(x * 65536.0f, y * 65536.0f, z * 65536.0f, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float hr_response(float cxx, float cxy, float cxz, float cyy, float cyz, float czz, int method)
{
    const float trace = (cxx + cyy) + czz;
    if (!(trace != 0.0f)) return 0.0f;
    const float det = cxx * cyy * czz + 2.0f * cxy * cxz * cyz - cxz * cxz * cyy - cxy * cxy * czz - cyz * cyz * cxx;
    if (method == 1) return det / trace;
    if (method == 2) return det / (trace * trace);
    return (0.04f + det) - (0.04f * trace) * trace;
}

template <int G>
__global__ __launch_bounds__(HARRIS_BLOCK) void harris_response_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start,
                                                                       GridParams g, uint32_t n, float r2, float s_win, int method,
                                                                       const float4* __restrict__ nrec, float* __restrict__ resp_sorted,
                                                                       float* __restrict__ resp_out, uint32_t* __restrict__ cnt_out)
{
    const uint32_t p = (blockIdx.x * HARRIS_BLOCK + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    if (p >= n) return;                                     // whole groups leave together (HARRIS_BLOCK % G == 0)
    const float4 q = records[p];
    double f[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };         // pending terms (integer-valued)
    long long S[6] = { 0, 0, 0, 0, 0, 0 };
    unsigned c = 0, m = 0, pending = 0;
    if (finite3(q.x, q.y, q.z)) {
        const RadiusWalk walk(g, cell_start, records, query_cell(g, q), radius_window(q.x, s_win));
        for (int k = 0; k < 9; k++) {
            uint32_t b, e;
            walk.row<384>(k, b, e);
            while (b < e) {                                 // pieces of at most HARRIS_PENDING_MAX records per lane
                const uint32_t piece = (e - b + G - 1) / G <= HARRIS_PENDING_MAX ? e : b + HARRIS_PENDING_MAX * G;
                const uint32_t len = (piece - b + G - 1) / G;
                if (pending + len > HARRIS_PENDING_MAX) {
#pragma unroll
                    for (int t = 0; t < 6; t++) { S[t] += (long long)f[t]; f[t] = 0.0; }
                    pending = 0;
                }
                pending += len;
                for (uint32_t j = b + sub; j < piece; j += G) {
                    const float4 t = records[j];
                    if (!(hr_s(t.x - q.x, t.y - q.y, t.z - q.z) < r2)) continue;
                    c++;
                    const float4 v = nrec[j];
                    m += (unsigned)v.w;
                    f[0] += (double)__builtin_rintf(v.x * v.x);
                    f[1] += (double)__builtin_rintf(v.x * v.y);
                    f[2] += (double)__builtin_rintf(v.x * v.z);
                    f[3] += (double)__builtin_rintf(v.y * v.y);
                    f[4] += (double)__builtin_rintf(v.y * v.z);
                    f[5] += (double)__builtin_rintf(v.z * v.z);
                }
                b = piece;
            }
        }
    }
    c = group_sum<G>(c);
    m = group_sum<G>(m);
#pragma unroll
    for (int t = 0; t < 6; t++) S[t] = group_sum<G>(S[t] + (long long)f[t]);
    if (sub != 0) return;
    float co[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (m != 0) {
#pragma unroll
        for (int t = 0; t < 6; t++) co[t] = (float)(((double)S[t] * 0x1p-32) / (double)m);
    }
    const float r = hr_response(co[0], co[1], co[2], co[3], co[4], co[5], method);
    const uint32_t pi = __float_as_uint(q.w);
    resp_sorted[p] = r;
    resp_out[pi] = r;
    cnt_out[pi] = c;
}

// nms == 0: every finite point is a keypoint (PCL copies the whole response cloud).  A non-finite point has response 0 and lies in
// the grid's extra cell: it is nobody's neighbour and never a keypoint.
template <int G>
__global__ __launch_bounds__(HARRIS_BLOCK) void harris_nms_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start,
                                                                  GridParams g, uint32_t n, float r2, float s_win, float threshold, int nms,
                                                                  const float* __restrict__ resp_sorted, uint8_t* __restrict__ is_key)
{
    const uint32_t p = (blockIdx.x * HARRIS_BLOCK + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    if (p >= n) return;
    const float4 q = records[p];
    const float mine = resp_sorted[p];
    const bool fin = finite3(q.x, q.y, q.z);
    bool key = fin;
    if (nms) {
        key = fin && fabsf(mine) <= FLT_MAX && !(mine < threshold);
        if (key) {                                          // uniform over the group
            bool beaten = false;
            const RadiusWalk walk(g, cell_start, records, query_cell(g, q), radius_window(q.x, s_win));
            for (int k = 0; k < 9 && !beaten; k++) {
                uint32_t b, e;
                walk.row<384>(k, b, e);
                for (uint32_t j0 = b; j0 < e; j0 += G) {    // uniform over the group: it leaves together at the first larger neighbour
                    const uint32_t j = j0 + sub;
                    bool lost = false;
                    if (j < e) {
                        const float4 t = records[j];
                        lost = hr_s(t.x - q.x, t.y - q.y, t.z - q.z) < r2 && mine < resp_sorted[j];
                    }
                    if (group_any<G>(lost)) { beaten = true; break; }
                }
            }
            key = !beaten;
        }
    }
    if (sub == 0) is_key[__float_as_uint(q.w)] = key ? 1 : 0;
}

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_harris3d_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_cloud* normals, const pcr_harris3d_params* prm, uint8_t* is_key,
                                float* response, uint32_t* neighbor_counts, uint64_t* n_keypoints)
{
    if (!ctx || !cloud || !normals || !prm || !is_key) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32");
    if (!(prm->radius > 0.0f) || std::isinf(prm->radius)) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32: radius must be finite and > 0");
    if (prm->threshold != prm->threshold) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32: threshold is NaN");
    if (prm->method < 0 || prm->method > 2) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32: method must be 0 (HARRIS), 1 (NOBLE) or 2 (LOWE)");
    if (normals->n != cloud->n) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32: one normal per point");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = cloud->n;
    if (n_keypoints) *n_keypoints = 0;
    if (n == 0) return PCR_OK;
    if (n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_harris3d_f32: cloud too large");
    const float radius = prm->radius;
    const float r2 = (float)((double)radius * (double)radius);
    const float s_win = std::nextafterf(r2, 0.0f);         // largest float below r2 (fpfh.hip)
    Grid* g = nullptr;
    {
        ProfScope ps(ctx, "harris_grid_build");
        int rc = grid_build(ctx, cloud, &g, radius_cell_edge(radius));
        if (rc) return rc;
    }
    const GridPtr g_owner(g);
    if ((double)g->p.h < (double)radius * 1.005) return fail(ctx, PCR_ERR_STATE, "pcr_harris3d_f32: grid cell smaller than the radius");
    float4* nrec;
    float *resp_sorted, *resp_dev;
    uint32_t* cnt_dev;
    uint8_t* key_dev;
    Layout L;
    L.add(&nrec, n);
    L.add(&resp_sorted, n);
    L.add(&resp_dev, n);
    L.add(&cnt_dev, n);
    L.add(&key_dev, n);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    const int nms = prm->non_max_suppression ? 1 : 0;
    const int G = (int)tune_get(ctx, "harris_lanes", 16);   // measured: profiles/harris.txt (best at hw9's size)
#define PCR_HARRIS(GG)                                                                                                                \
    {                                                                                                                                 \
        const dim3 grid((unsigned)((n * GG + HARRIS_BLOCK - 1) / HARRIS_BLOCK));                                                      \
        { ProfScope ps(ctx, "harris_response", 1);                                                                                    \
          hipLaunchKernelGGL(harris_normals_kernel, dim3((unsigned)((n + HARRIS_BLOCK - 1) / HARRIS_BLOCK)), dim3(HARRIS_BLOCK), 0, ctx->stream, \
                             g->records, (uint32_t)n, normals->x(), normals->y(), normals->z(), nrec);                                \
          hipLaunchKernelGGL((harris_response_kernel<GG>), grid, dim3(HARRIS_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, \
                             (uint32_t)n, r2, s_win, prm->method, nrec, resp_sorted, resp_dev, cnt_dev); }                            \
        { ProfScope ps(ctx, "harris_nms", 1);                                                                                         \
          hipLaunchKernelGGL((harris_nms_kernel<GG>), grid, dim3(HARRIS_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p,      \
                             (uint32_t)n, r2, s_win, prm->threshold, nms, resp_sorted, key_dev); }                                    \
    }
    switch (G) {
    case 1: PCR_HARRIS(1) break;
    case 2: PCR_HARRIS(2) break;
    case 4: PCR_HARRIS(4) break;
    case 8: PCR_HARRIS(8) break;
    case 32: PCR_HARRIS(32) break;
    default: PCR_HARRIS(16) break;
    }
#undef PCR_HARRIS
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(is_key, key_dev, n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && response) e = hipMemcpyAsync(response, resp_dev, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && neighbor_counts) e = hipMemcpyAsync(neighbor_counts, cnt_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_harris3d_f32", e);
    prof_flush(ctx);
    if (n_keypoints) {
        uint64_t c = 0;
        for (size_t i = 0; i < n; i++) c += is_key[i];
        *n_keypoints = c;
    }
    return PCR_OK;
}
