// fpfh.hip — FPFH33 descriptors (Homework9/hw9/src/registration.cpp:254-269, PCL's FPFHEstimationOMP) as two radius passes over the
// uniform grid (the walk: grid_walk.hpp).  The contract (neighbourhood, pair features, bins, weighting) is written out above
// pcr_fpfh33_f32 in include/pcr.h; this file follows it operation by operation.
//
//   pass 1  fpfh_spfh    G lanes per SURFACE point (the queries are the grid records): one walk of the 27-cell block
//                        counts |N(p)| and bins every pair (p, j), j != p, into 33 u32 counts in LDS (atomics inside the point's
//                        group: counts do not depend on order); then the lanes of the group turn the counts into f32 values
//                        (incr added cnt times) and write the SPFH row in record order (and in input order when asked for)
//   pass 2  fpfh_weight  G lanes per KEYPOINT (grid records when keypoints = surface, else the keypoint cloud in input order): one walk
//                        accumulates spfh_j * (1 / s) into 33 f64 per lane, a fixed-order xor-shuffle reduction sums the group, and
//                        the sums are normalised to 100 per sub-histogram
//
// Distances are the f32 sum s = ((dx*dx) + dy*dy) + dz*dz, member iff s < r2 (FLANN's strict radius test).  The window of a row
// (radius_window) takes the largest float BELOW r2: its bound |dx|^2 <= s_max (1 + 3 * 2^-24) holds for the f32 sum as well, since
// every partial sum of non-negative terms rounds to at least its first term.
#include "grid_walk.hpp"

#include <cmath>

namespace pcr {

namespace {

constexpr int FPFH_BLOCK = 256;
constexpr int FPFH_BINS = 11;
constexpr int FPFH_DIM = 33;

__device__ __forceinline__ float fp_s(float dx, float dy, float dz) { return ((dx * dx) + dy * dy) + dz * dz; }
__device__ __forceinline__ float fp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// clamped bin of a value v in bin units (floor, then [0, 10]; NaN -> 0)
__device__ __forceinline__ int fp_bin(double v)
{
    const double f = floor(v);
    return f >= 10.0 ? 10 : (f >= 0.0 ? (int)f : 0);
}

// computePairFeatures (p1 = centre with normal n1, p2 = neighbour with normal n2) -> the three bins, or false for a skipped pair
__device__ __forceinline__ bool fp_pair_bins(float dpx, float dpy, float dpz, float n1x, float n1y, float n1z, float n2x, float n2y, float n2z,
                                             int& b1, int& b2, int& b3)
{
    if (!finite3(n1x, n1y, n1z) || !finite3(n2x, n2y, n2z)) return false;
    const float f4 = sqrtf(fp_dot(dpx, dpy, dpz, dpx, dpy, dpz));
    if (f4 == 0.0f) return false;
    const float a1 = fp_dot(n1x, n1y, n1z, dpx, dpy, dpz) / f4;
    const float a2 = fp_dot(n2x, n2y, n2z, dpx, dpy, dpz) / f4;
    float f3 = a1;
    if (fabsf(a1) <= 1.0f && fabsf(a2) <= 1.0f && fabsf(a1) < fabsf(a2)) {      // acos(|a1|) > acos(|a2|)
        float t;
        t = n1x; n1x = n2x; n2x = t;
        t = n1y; n1y = n2y; n2y = t;
        t = n1z; n1z = n2z; n2z = t;
        dpx = -dpx; dpy = -dpy; dpz = -dpz;
        f3 = -a2;
    }
    float vx = dpy * n1z - dpz * n1y, vy = dpz * n1x - dpx * n1z, vz = dpx * n1y - dpy * n1x;      // v = dp x n1
    const float vn = sqrtf(fp_dot(vx, vy, vz, vx, vy, vz));
    if (vn == 0.0f) return false;
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const float wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;      // w = n1 x v
    const float f2 = fp_dot(vx, vy, vz, n2x, n2y, n2z);
    const float f1 = (float)atan2((double)fp_dot(wx, wy, wz, n2x, n2y, n2z), (double)fp_dot(n1x, n1y, n1z, n2x, n2y, n2z));
    const float d_pi = 1.0f / (2.0f * (float)M_PI);
    b1 = fp_bin(11.0 * (((double)f1 + M_PI) * (double)d_pi));
    b2 = fp_bin(11.0 * (((double)f2 + 1.0) * 0.5));
    b3 = fp_bin(11.0 * (((double)f3 + 1.0) * 0.5));
    return true;
}

// pass 1.  LDS: 33 counts per point of the block (G = 1: 256 x 132 B = 33 KiB)
template <int G>
__global__ __launch_bounds__(FPFH_BLOCK) void fpfh_spfh_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                               uint32_t n, float r2, float s_win, const float* __restrict__ nx,
                                                               const float* __restrict__ ny, const float* __restrict__ nz,
                                                               float* __restrict__ spfh_sorted, float* __restrict__ spfh_out)
{
    __shared__ uint32_t hist[FPFH_BLOCK / G][FPFH_DIM];
    const uint32_t slot = threadIdx.x / G;
    const uint32_t p = blockIdx.x * (FPFH_BLOCK / G) + slot;
    const int sub = threadIdx.x % G;
    for (int b = sub; b < FPFH_DIM; b += G) hist[slot][b] = 0u;
    __syncthreads();
    unsigned c = 0;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < n) {                                            // uniform over the group (FPFH_BLOCK % G == 0)
        q = records[p];
        if (finite3(q.x, q.y, q.z)) {
            const uint32_t pi = __float_as_uint(q.w);
            const float n1x = nx[pi], n1y = ny[pi], n1z = nz[pi];
            const RadiusWalk walk(g, cell_start, records, query_cell(g, q), radius_window(q.x, s_win));
            for (int k = 0; k < 9; k++) {
                uint32_t b, e;
                walk.row<384>(k, b, e);
                for (uint32_t j = b + sub; j < e; j += G) {
                    const float4 t = records[j];
                    const float dx = t.x - q.x, dy = t.y - q.y, dz = t.z - q.z;
                    if (!(fp_s(dx, dy, dz) < r2)) continue;
                    c++;
                    const uint32_t ji = __float_as_uint(t.w);
                    if (ji == pi) continue;
                    int b1, b2, b3;
                    if (!fp_pair_bins(dx, dy, dz, n1x, n1y, n1z, nx[ji], ny[ji], nz[ji], b1, b2, b3)) continue;
                    atomicAdd(&hist[slot][b1], 1u);
                    atomicAdd(&hist[slot][FPFH_BINS + b2], 1u);
                    atomicAdd(&hist[slot][2 * FPFH_BINS + b3], 1u);
                }
            }
        }
    }
    c = group_sum<G>(c);
    __syncthreads();
    if (p >= n) return;
    // value of a bin = incr added cnt times in f32: all addends are equal, so this is PCL's repeated += in any order
    const float incr = 100.0f / (float)((int)c - 1);
    const uint32_t pi = __float_as_uint(q.w);
    for (int b = sub; b < FPFH_DIM; b += G) {
        const uint32_t cnt = hist[slot][b];
        float v = 0.0f;
        for (uint32_t i = 0; i < cnt; i++) v += incr;
        spfh_sorted[(size_t)p * FPFH_DIM + b] = v;
        if (spfh_out) spfh_out[(size_t)pi * FPFH_DIM + b] = v;
    }
}

// pass 2.  Queries: qrec (grid records, output row = the record's original index) or the SoA keypoint cloud (output row = i)
template <int G>
__global__ __launch_bounds__(FPFH_BLOCK) void fpfh_weight_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                                 float r2, float s_win, const float4* __restrict__ qrec, const float* __restrict__ qx,
                                                                 const float* __restrict__ qy, const float* __restrict__ qz, uint32_t m,
                                                                 const float* __restrict__ spfh_sorted, float* __restrict__ fpfh, uint32_t* __restrict__ cnt_out)
{
    const uint32_t i = (blockIdx.x * FPFH_BLOCK + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    if (i >= m) return;                                     // whole groups leave together
    const float4 q = qrec ? qrec[i] : make_float4(qx[i], qy[i], qz[i], __uint_as_float(i));
    const uint32_t row = __float_as_uint(q.w);
    double acc[FPFH_DIM];
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) acc[b] = 0.0;
    unsigned c = 0;
    const bool fin = finite3(q.x, q.y, q.z);
    if (fin) {
        const RadiusWalk walk(g, cell_start, records, query_cell(g, q), radius_window(q.x, s_win));
        for (int k = 0; k < 9; k++) {
            uint32_t b, e;
            walk.row<384>(k, b, e);
            for (uint32_t j = b + sub; j < e; j += G) {
                const float4 t = records[j];
                const float s = fp_s(t.x - q.x, t.y - q.y, t.z - q.z);
                if (!(s < r2)) continue;
                c++;
                if (s == 0.0f) continue;
                const float w = 1.0f / s;                   // the SQUARED distance, as weightPointSPFHSignature
                const float* h = spfh_sorted + (size_t)j * FPFH_DIM;
#pragma unroll
                for (int bb = 0; bb < FPFH_DIM; bb++) acc[bb] += (double)(h[bb] * w);
            }
        }
    }
    c = group_sum<G>(c);
#pragma unroll
    for (int b = 0; b < FPFH_DIM; b++) acc[b] = group_sum<G>(acc[b]);
    if (sub == 0 && cnt_out) cnt_out[row] = c;
    float* out = fpfh + (size_t)row * FPFH_DIM;
    if (!fin || c == 0) {                                   // computeFeature: a row of NaN
#pragma unroll
        for (int b = 0; b < FPFH_DIM; b++)
            if (b % G == sub) out[b] = __builtin_nanf("");
        return;
    }
#pragma unroll
    for (int h = 0; h < 3; h++) {
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; b++) sum += acc[h * FPFH_BINS + b];
        const double sc = sum != 0.0 ? 100.0 / sum : 1.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; b++)
            if ((h * FPFH_BINS + b) % G == sub) out[h * FPFH_BINS + b] = (float)(sum != 0.0 ? acc[h * FPFH_BINS + b] * sc : acc[h * FPFH_BINS + b]);
    }
}

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_fpfh33_f32(pcr_ctx* ctx, const pcr_cloud* surface, const pcr_cloud* normals, const pcr_cloud* keypoints, float radius, float* fpfh,
                              uint32_t* neighbor_counts, float* spfh)
{
    if (!ctx || !surface || !normals || !fpfh) return fail(ctx, PCR_ERR_ARG, "pcr_fpfh33_f32");
    if (!(radius > 0.0f) || std::isinf(radius)) return fail(ctx, PCR_ERR_ARG, "pcr_fpfh33_f32: radius must be finite and > 0");
    if (normals->n != surface->n) return fail(ctx, PCR_ERR_ARG, "pcr_fpfh33_f32: one normal per surface point");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = surface->n;
    const size_t m = keypoints ? keypoints->n : n;
    if (n == 0 || m == 0) return PCR_OK;
    if (n > 0x7FFFFFF0ull || m > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_fpfh33_f32: cloud too large");
    const float r2 = (float)((double)radius * (double)radius);
    const float s_win = std::nextafterf(r2, 0.0f);         // largest float below r2 (r2 > 0 here or the set is empty anyway)
    Grid* g = nullptr;
    {
        ProfScope ps(ctx, "fpfh_grid_build");
        int rc = grid_build(ctx, surface, &g, radius_cell_edge(radius));
        if (rc) return rc;
    }
    const GridPtr g_owner(g);
    if ((double)g->p.h < (double)radius * 1.005) return fail(ctx, PCR_ERR_STATE, "pcr_fpfh33_f32: grid cell smaller than the radius");
    float *spfh_sorted, *fpfh_dev, *spfh_dev = nullptr;
    uint32_t* cnt_dev;
    Layout L;
    L.add(&spfh_sorted, n * FPFH_DIM);
    L.add(&fpfh_dev, m * FPFH_DIM);
    L.add(&cnt_dev, m);
    if (spfh) L.add(&spfh_dev, n * FPFH_DIM);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    const float4* qrec = keypoints ? nullptr : g->records;
    const float* kx = keypoints ? keypoints->x() : nullptr;
    const float* ky = keypoints ? keypoints->y() : nullptr;
    const float* kz = keypoints ? keypoints->z() : nullptr;
    const int G = (int)tune_get(ctx, "fpfh_lanes", 16);    // measured: profiles/fpfh.txt (best at hw9's size; 32 wins on |N| in the thousands)
#define PCR_FPFH(GG)                                                                                                                  \
    {                                                                                                                                 \
        { ProfScope ps(ctx, "fpfh_spfh", 1);                                                                                          \
          hipLaunchKernelGGL((fpfh_spfh_kernel<GG>), dim3((unsigned)((n + FPFH_BLOCK / GG - 1) / (FPFH_BLOCK / GG))), dim3(FPFH_BLOCK), 0, ctx->stream, \
                             g->records, g->cell_start, g->p, (uint32_t)n, r2, s_win, normals->x(), normals->y(), normals->z(), spfh_sorted, spfh_dev); } \
        { ProfScope ps(ctx, "fpfh_weight", 1);                                                                                        \
          hipLaunchKernelGGL((fpfh_weight_kernel<GG>), dim3((unsigned)((m * GG + FPFH_BLOCK - 1) / FPFH_BLOCK)), dim3(FPFH_BLOCK), 0, ctx->stream, \
                             g->records, g->cell_start, g->p, r2, s_win, qrec, kx, ky, kz, (uint32_t)m, spfh_sorted, fpfh_dev, cnt_dev); } \
    }
    switch (G) {
    case 1: PCR_FPFH(1) break;
    case 2: PCR_FPFH(2) break;
    case 4: PCR_FPFH(4) break;
    case 8: PCR_FPFH(8) break;
    case 32: PCR_FPFH(32) break;
    default: PCR_FPFH(16) break;
    }
#undef PCR_FPFH
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(fpfh, fpfh_dev, m * FPFH_DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && neighbor_counts) e = hipMemcpyAsync(neighbor_counts, cnt_dev, m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && spfh) e = hipMemcpyAsync(spfh, spfh_dev, n * FPFH_DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_fpfh33_f32", e);
    prof_flush(ctx);
    return PCR_OK;
}
