// sample.hip — the two sampling stages at either end of Homework9's shipped flow, both as order-free restatements of the PCL filters hw9
// calls (the contracts are written out above pcr_voxel_grid_normals_f32 / pcr_normal_space_sample_f32 in include/pcr.h; this file follows
// them operation by operation):
//
//   pcr_voxel_grid_normals_f32   readBinaryAndVoxelDown (registration.cpp:8-68) / VoxelGridSampling (:665-707): pcl::VoxelGrid over
//                                points AND normals, one output row per occupied voxel in ascending voxel id.
//     vg_bounds    one read of the scan: min / max of floorf(x * inv) per axis and the largest |coordinate| (the ONE box read-back)
//     vg_keys      voxel id per point (the id space's size for a skipped point: it sorts behind every voxel)
//     sort         stable radix sort of (id, index) over the bits the id space needs (sort.hip)
//     vg_heads + scan + vg_accum   every sorted position turns its point (and normal) into integers on the fixed-point grid of the
//                  contract; a segmented shuffle scan adds the runs of one voxel inside a wave and the last lane of each run adds the
//                  run's seven words (six int64 sums, two packed counts) to the voxel's row with vector atomics — integers, so exact
//                  and independent of how the runs fall
//     vg_finalize  one lane per voxel: sums -> centroid, mean normal (unit length in mode 1), count
//
//   pcr_normal_space_sample_f32  normalSpaceSampling (:630-662): bin + SplitMix64 key per point, stable sort by key, stable sort by bin
//                                (=> (bin, key, index) order), rank inside the bin, sort by (rank, bin), first `sample` of it; gather.
#include "pcr_internal.hpp"

#include "sort.hpp"

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int SM_BLOCK = 256;
constexpr int VG_WORDS = 7;             // per voxel row: Sx, Sy, Sz, Snx, Sny, Snz (int64), count | normal count << 32

__device__ __forceinline__ bool sm_finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

// out[block][7] = { min fx, min fy, min fz, max fx, max fy, max fz, max |coordinate| } over the finite points, f* = floorf(fl32(* x inv));
// a block without a finite point leaves { FLT_MAX x 3, -FLT_MAX x 3, -1 }
__global__ __launch_bounds__(SM_BLOCK) void vg_bounds_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                             uint32_t n, float inv, float* __restrict__ out)
{
    float v[7] = { FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, -1.0f };
    for (uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x; i < n; i += gridDim.x * SM_BLOCK) {
        const float px = x[i], py = y[i], pz = z[i];
        if (!sm_finite3(px, py, pz)) continue;
        const float fx = floorf(px * inv), fy = floorf(py * inv), fz = floorf(pz * inv);
        v[0] = fminf(v[0], fx); v[1] = fminf(v[1], fy); v[2] = fminf(v[2], fz);
        v[3] = fmaxf(v[3], fx); v[4] = fmaxf(v[4], fy); v[5] = fmaxf(v[5], fz);
        v[6] = fmaxf(v[6], fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz))));
    }
    __shared__ float red[SM_BLOCK / 64][7];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        float a = v[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a = c < 3 ? fminf(a, __shfl_down(a, o, 64)) : fmaxf(a, __shfl_down(a, o, 64));
        if (lane == 0) red[wave][c] = a;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int c = threadIdx.x;
        float a = red[0][c];
        for (int w = 1; w < SM_BLOCK / 64; w++) a = c < 3 ? fminf(a, red[w][c]) : fmaxf(a, red[w][c]);
        out[blockIdx.x * 7 + c] = a;
    }
}

struct VgParams {
    float inv;
    int min_b[3];
    long long div_x, div_xy, total;      // total = div_x * div_y * div_z <= INT32_MAX: the key of a skipped point
    double to_q, from_q;                 // 2^(32 - E), 2^(E - 32)
};

__global__ __launch_bounds__(SM_BLOCK) void vg_keys_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                           uint32_t n, VgParams p, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float px = x[i], py = y[i], pz = z[i];
    long long id = p.total;
    if (sm_finite3(px, py, pz)) {        // inside [min_b, max_b] by construction of the bounds: the casts are exact
        const long long cx = (long long)(int)floorf(px * p.inv) - p.min_b[0];
        const long long cy = (long long)(int)floorf(py * p.inv) - p.min_b[1];
        const long long cz = (long long)(int)floorf(pz * p.inv) - p.min_b[2];
        id = cx + cy * p.div_x + cz * p.div_xy;
    }
    keys[i] = (unsigned long long)id;
    vals[i] = i;
}

__global__ __launch_bounds__(SM_BLOCK) void vg_heads_kernel(const unsigned long long* __restrict__ keys, uint32_t n, unsigned long long skipped,
                                                            uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= n) return;
    flags[i] = (keys[i] != skipped && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}

// one lane per SORTED position.  gid_excl + flags give the position's output row; a skipped point has key == skipped (row -1).
template <bool HAS_N>
__global__ __launch_bounds__(SM_BLOCK) void vg_accum_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                            const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz,
                                                            const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ flags, const uint32_t* __restrict__ gid_excl, uint32_t n,
                                                            uint32_t m, VgParams p, unsigned long long* __restrict__ table, int32_t* __restrict__ vop)
{
    const uint32_t pos = blockIdx.x * SM_BLOCK + threadIdx.x;      // no early exit: every lane takes part in the shuffles
    const int lane = threadIdx.x & 63;
    int g = -1;
    long long v[VG_WORDS] = { 0, 0, 0, 0, 0, 0, 0 };
    if (pos < n) {
        const uint32_t i = order[pos];
        if (keys[pos] != (unsigned long long)p.total) {
            g = (int)(gid_excl[pos] + flags[pos]) - 1;
            v[0] = (long long)__builtin_rint((double)x[i] * p.to_q);
            v[1] = (long long)__builtin_rint((double)y[i] * p.to_q);
            v[2] = (long long)__builtin_rint((double)z[i] * p.to_q);
            v[6] = 1;
            if (HAS_N) {
                const float a = nx[i], b = ny[i], c = nz[i];
                if (fabsf(a) <= 2.0f && fabsf(b) <= 2.0f && fabsf(c) <= 2.0f) {      // false for NaN / inf
                    v[3] = (long long)__builtin_rint((double)a * 0x1p30);
                    v[4] = (long long)__builtin_rint((double)b * 0x1p30);
                    v[5] = (long long)__builtin_rint((double)c * 0x1p30);
                    v[6] += 1ll << 32;
                }
            }
        }
        vop[i] = g;
    }
    // segmented inclusive scan over the wave: runs of equal g are contiguous (sorted order)
    const int gprev = __shfl_up(g, 1, 64);
    const bool head = lane == 0 || gprev != g;
    const unsigned long long heads = __ballot(head);
    const int s = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));      // first lane of this lane's run (bit `lane`'s run head; bit 0 is set)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int w = 0; w < VG_WORDS; w++) {
            if (!HAS_N && w >= 3 && w < 6) continue;
            const long long t = __shfl_up(v[w], d, 64);
            if (lane - d >= s) v[w] += t;
        }
    }
    const int gnext = __shfl_down(g, 1, 64);
    const bool tail = lane == 63 || gnext != g;
    if (tail && g >= 0 && (uint32_t)g < m) {
        unsigned long long* row = table + (size_t)g * VG_WORDS;
#pragma unroll
        for (int w = 0; w < VG_WORDS; w++) {
            if (!HAS_N && w >= 3 && w < 6) continue;
            atomicAdd(row + w, (unsigned long long)v[w]);          // two's complement: the sum of the words is the int64 sum
        }
    }
}

template <bool HAS_N>
__global__ __launch_bounds__(SM_BLOCK) void vg_finalize_kernel(const unsigned long long* __restrict__ table, uint32_t m, uint32_t cap, VgParams p,
                                                               int normal_mode, float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                               float* __restrict__ onx, float* __restrict__ ony, float* __restrict__ onz, uint32_t ncap,
                                                               uint32_t* __restrict__ counts)
{
    const uint32_t g = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (g >= m) {                                                   // the padding of the new clouds (x = +inf: never anybody's neighbour)
        if (g < cap) { ox[g] = __builtin_inff(); oy[g] = 0.0f; oz[g] = 0.0f; }
        if (HAS_N && g < ncap) { onx[g] = __builtin_inff(); ony[g] = 0.0f; onz[g] = 0.0f; }
        return;
    }
    const unsigned long long* row = table + (size_t)g * VG_WORDS;
    const uint32_t cnt = (uint32_t)(row[6] & 0xFFFFFFFFull), cntn = (uint32_t)(row[6] >> 32);
    ox[g] = (float)(((double)(long long)row[0] * p.from_q) / (double)cnt);
    oy[g] = (float)(((double)(long long)row[1] * p.from_q) / (double)cnt);
    oz[g] = (float)(((double)(long long)row[2] * p.from_q) / (double)cnt);
    counts[g] = cnt;
    if (HAS_N) {
        float a = 0.0f, b = 0.0f, c = 0.0f;
        if (cntn != 0) {
            a = (float)(((double)(long long)row[3] * 0x1p-30) / (double)cntn);
            b = (float)(((double)(long long)row[4] * 0x1p-30) / (double)cntn);
            c = (float)(((double)(long long)row[5] * 0x1p-30) / (double)cntn);
            if (normal_mode == 1) {
                const float len = sqrtf((a * a + b * b) + c * c);
                if (len != 0.0f) { a = a / len; b = b / len; c = c / len; }
            }
        }
        onx[g] = a; ony[g] = b; onz[g] = c;
    }
}

// ---- normal-space sampling --------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ns_key(unsigned long long seed, uint32_t i)
{
    unsigned long long zz = seed ^ (0x9E3779B97F4A7C15ull * ((unsigned long long)i + 1ull));
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    return zz ^ (zz >> 31);
}

__device__ __forceinline__ uint32_t ns_axis(float v, uint32_t bins)
{
    const float r = roundf((0.5f * ((float)bins - 1.0f)) * (v + 1.0f));
    const float hi = (float)(bins - 1u);                            // exact: bins <= 2^20
    return !(r > 0.0f) ? 0u : (r > hi ? bins - 1u : (uint32_t)r);
}

struct NsParams {
    uint32_t bx, by, bz, nbins;
    unsigned long long seed, sample, sentinel;
};

__global__ __launch_bounds__(SM_BLOCK) void ns_keys_kernel(const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz,
                                                           uint32_t n, NsParams p, uint32_t* __restrict__ bin_of, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals, uint32_t* __restrict__ n_valid)
{
    const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const float a = nx[i], b = ny[i], c = nz[i];
        ok = sm_finite3(a, b, c);
        bin_of[i] = ok ? (ns_axis(a, p.bx) * (p.by * p.bz) + ns_axis(b, p.by) * p.bz) + ns_axis(c, p.bz) : p.nbins;
        keys[i] = ns_key(p.seed, i);
        vals[i] = i;
    }
    const unsigned long long mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && mask != 0ull) atomicAdd(n_valid, (uint32_t)__popcll(mask));
}

__global__ __launch_bounds__(SM_BLOCK) void ns_bin_keys_kernel(const uint32_t* __restrict__ bin_of, const uint32_t* __restrict__ order, uint32_t n,
                                                               unsigned long long* __restrict__ keys)
{
    const uint32_t pos = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (pos < n) keys[pos] = bin_of[order[pos]];
}

// start[b] = first position of bin b in the (bin, key, index) order; written for the bins that occur (nbins itself included)
__global__ __launch_bounds__(SM_BLOCK) void ns_starts_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t nbins, uint32_t* __restrict__ start)
{
    const uint32_t pos = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (pos >= n) return;
    const unsigned long long b = keys[pos];
    if (b <= (unsigned long long)nbins && (pos == 0 || keys[pos - 1] != b)) start[b] = pos;
}

__global__ __launch_bounds__(SM_BLOCK) void ns_rank_keys_kernel(const unsigned long long* __restrict__ bins_sorted, const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ start, const uint32_t* __restrict__ n_valid, uint32_t n,
                                                                NsParams p, unsigned long long* __restrict__ keys)
{
    const uint32_t pos = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (pos >= n) return;
    const unsigned long long b = bins_sorted[pos];
    unsigned long long k = p.sentinel;
    if (b < (unsigned long long)p.nbins) {
        if (p.sample >= (unsigned long long)*n_valid) k = order[pos];                  // everything: ascending index
        else k = ((unsigned long long)(pos - start[b]) << 20) | b;                     // (rank, bin)
    }
    keys[pos] = k;
}

__global__ __launch_bounds__(SM_BLOCK) void ns_gather_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, uint32_t n,
                                                             const uint32_t* __restrict__ order, uint32_t m, uint32_t cap, float* __restrict__ ox,
                                                             float* __restrict__ oy, float* __restrict__ oz)
{
    const uint32_t t = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (t >= cap) return;
    float a = __builtin_inff(), b = 0.0f, c = 0.0f;
    if (t < m) {
        const uint32_t i = order[t];
        if (i < n) { a = x[i]; b = y[i]; c = z[i]; }
    }
    ox[t] = a; oy[t] = b; oz[t] = c;
}

inline unsigned bit_length(unsigned long long v) { unsigned b = 0; while (v) { b++; v >>= 1; } return b; }
inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + SM_BLOCK - 1) / SM_BLOCK)); }

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_voxel_grid_normals_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_cloud* normals, float leaf, int normal_mode,
                                          pcr_cloud** out_cloud, pcr_cloud** out_normals, int32_t* voxel_of_point, uint32_t* counts, uint64_t* n_voxels)
{
    if (out_cloud) *out_cloud = nullptr;
    if (out_normals) *out_normals = nullptr;
    if (n_voxels) *n_voxels = 0;
    if (!ctx || !cloud || !out_cloud) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32");
    if (!(leaf > 0.0f) || std::isinf(leaf)) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: leaf must be finite and > 0");
    if (normal_mode != 0 && normal_mode != 1) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: normal_mode must be 0 (mean) or 1 (unit length)");
    if (normals && normals->n != cloud->n) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: one normal per point");
    if (normals && !out_normals) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: normals given without out_normals");
    const float inv = 1.0f / leaf;
    if (std::isinf(inv)) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: 1 / leaf is not finite");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = cloud->n;
    if (n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: cloud too large");
    const bool has_n = normals != nullptr;
    float dummy = 0.f;
    if (n == 0) {
        int rc = pcr_cloud_create(ctx, &dummy, 0, PCR_SOA, out_cloud);
        if (rc == PCR_OK && has_n) rc = pcr_cloud_create(ctx, &dummy, 0, PCR_SOA, out_normals);
        return rc;
    }
    // ---- scratch: everything whose size depends on n only (the per-voxel rows go to the second scratch once their number is known)
    size_t temp_bytes = 0;
    sort_pairs_u64_u32(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, n, 0, 32, ctx->stream);
    const uint32_t bb = (uint32_t)std::max<size_t>(1, std::min<size_t>(256, (n + SM_BLOCK - 1) / SM_BLOCK));
    float* bounds_dev;
    unsigned long long *k_in, *k_out;
    uint32_t *v_in, *v_out, *flags, *gid, *totals, *m_dev;
    int32_t* vop_dev;
    void* sort_temp;
    Layout L;
    L.add(&bounds_dev, (size_t)bb * 7);
    L.add(&k_in, n);
    L.add(&k_out, n);
    L.add(&v_in, n);
    L.add(&v_out, n);
    L.add(&flags, n);
    L.add(&gid, n);
    L.add(&vop_dev, n);
    L.add(&totals, scan_blocks(n));
    L.add(&m_dev, 1);            // the scan's grand total: the number of voxels
    L.add(&sort_temp, temp_bytes);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    const dim3 gridn = blocks_for(n);
    // ---- 1. the box (the one read-back of it)
    {
        ProfScope ps(ctx, "vgn_bounds");
        hipLaunchKernelGGL(vg_bounds_kernel, dim3(bb), dim3(SM_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), (uint32_t)n, inv, bounds_dev);
    }
    std::vector<float> hb((size_t)bb * 7);
    PCR_HIP(ctx, hipMemcpyAsync(hb.data(), bounds_dev, hb.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float b7[7] = { FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, -1.0f };
    for (uint32_t k = 0; k < bb; k++)
        for (int c = 0; c < 7; c++) b7[c] = c < 3 ? std::min(b7[c], hb[k * 7 + c]) : std::max(b7[c], hb[k * 7 + c]);
    const bool any_finite = b7[6] >= 0.0f;
    VgParams p{};
    p.inv = inv;
    p.div_x = p.div_xy = 1; p.total = 1;
    p.to_q = p.from_q = 1.0;
    if (any_finite) {
        for (int c = 0; c < 6; c++)
            if (!(b7[c] >= -2147483648.0f && b7[c] < 2147483648.0f))
                return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: leaf too small for the cloud: a voxel coordinate does not fit int32");
        long long div[3];
        for (int c = 0; c < 3; c++) {
            p.min_b[c] = (int)b7[c];
            div[c] = (long long)b7[3 + c] - (long long)b7[c] + 1;
        }
        // (each div <= 2^32: the partial product is tested before the next factor so that nothing overflows int64)
        if (div[0] > INT32_MAX || div[0] * div[1] > INT32_MAX || div[0] * div[1] * div[2] > INT32_MAX)
            return fail(ctx, PCR_ERR_ARG, "pcr_voxel_grid_normals_f32: leaf too small for the cloud: the voxel ids overflow int32");
        p.div_x = div[0]; p.div_xy = div[0] * div[1]; p.total = div[0] * div[1] * div[2];
        int E = -149;
        if (b7[6] > 0.0f) { (void)std::frexp(b7[6], &E); E = std::max(E, -149); }      // absmax = f 2^E, 0.5 <= f < 1: every |coordinate| < 2^E
        p.to_q = std::ldexp(1.0, 32 - E);
        p.from_q = std::ldexp(1.0, E - 32);
    }
    // ---- 2. keys, stable sort by voxel id, segment heads, row of every sorted position
    uint32_t m = 0;
    if (any_finite) {
        {
            ProfScope ps(ctx, "vgn_keys");
            hipLaunchKernelGGL(vg_keys_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), (uint32_t)n, p, k_in, v_in);
        }
        {
            ProfScope ps(ctx, "vgn_sort");
            PCR_HIP(ctx, sort_pairs_u64_u32(sort_temp, temp_bytes, k_in, k_out, v_in, v_out, n, 0, std::max(1u, bit_length((unsigned long long)p.total)), ctx->stream));
        }
        {
            ProfScope ps(ctx, "vgn_segments");
            hipLaunchKernelGGL(vg_heads_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, k_out, (uint32_t)n, (unsigned long long)p.total, flags);
            rc = exclusive_scan_u32(ctx, flags, gid, n, totals, m_dev);
            if (rc) return rc;
        }
        PCR_HIP(ctx, hipMemcpyAsync(&m, m_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (m > n) return fail(ctx, PCR_ERR_STATE, "pcr_voxel_grid_normals_f32: more voxels than points");
    }
    // ---- 3. output clouds, per-voxel rows, sums, means
    pcr_cloud *oc = nullptr, *on = nullptr;
    rc = cloud_alloc(ctx, m, &oc);
    if (rc == PCR_OK && has_n) rc = cloud_alloc(ctx, m, &on);
    unsigned long long* table;
    uint32_t* counts_dev;
    Layout La;
    La.add(&table, (size_t)m * VG_WORDS);
    La.add(&counts_dev, m);
    if (rc == PCR_OK) rc = bind_aux(ctx, La);
    if (rc) { pcr_cloud_destroy(ctx, oc); pcr_cloud_destroy(ctx, on); return rc; }
    hipError_t e = hipSuccess;
    if (any_finite) {
        e = hipMemsetAsync(table, 0, (size_t)m * VG_WORDS * 8, ctx->stream);
        ProfScope ps(ctx, "vgn_accum");
        if (has_n)
            hipLaunchKernelGGL((vg_accum_kernel<true>), gridn, dim3(SM_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), normals->x(), normals->y(),
                               normals->z(), k_out, v_out, flags, gid, (uint32_t)n, m, p, table, vop_dev);
        else
            hipLaunchKernelGGL((vg_accum_kernel<false>), gridn, dim3(SM_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), (const float*)nullptr,
                               (const float*)nullptr, (const float*)nullptr, k_out, v_out, flags, gid, (uint32_t)n, m, p, table, vop_dev);
    } else if (voxel_of_point) {
        e = hipMemsetAsync(vop_dev, 0xFF, n * 4, ctx->stream);
    }
    {
        ProfScope ps(ctx, "vgn_finalize");
        const size_t span = std::max(oc->cap, has_n ? on->cap : (size_t)0);
        if (has_n)
            hipLaunchKernelGGL((vg_finalize_kernel<true>), blocks_for(span), dim3(SM_BLOCK), 0, ctx->stream, table, m, (uint32_t)oc->cap, p, normal_mode, oc->x(),
                               oc->y(), oc->z(), on->x(), on->y(), on->z(), (uint32_t)on->cap, counts_dev);
        else
            hipLaunchKernelGGL((vg_finalize_kernel<false>), blocks_for(span), dim3(SM_BLOCK), 0, ctx->stream, table, m, (uint32_t)oc->cap, p, normal_mode, oc->x(),
                               oc->y(), oc->z(), (float*)nullptr, (float*)nullptr, (float*)nullptr, 0u, counts_dev);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && voxel_of_point) e = hipMemcpyAsync(voxel_of_point, vop_dev, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && counts && m) e = hipMemcpyAsync(counts, counts_dev, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { pcr_cloud_destroy(ctx, oc); pcr_cloud_destroy(ctx, on); return fail(ctx, PCR_ERR_HIP, "pcr_voxel_grid_normals_f32", e); }
    prof_flush(ctx);
    *out_cloud = oc;
    if (has_n) *out_normals = on;
    if (n_voxels) *n_voxels = m;
    return PCR_OK;
}

extern "C" int pcr_normal_space_sample_f32(pcr_ctx* ctx, const pcr_cloud* normals, const uint32_t bins[3], size_t sample, uint64_t seed, uint32_t* indices,
                                           size_t* n_out, const pcr_cloud* gather_cloud, pcr_cloud** out_cloud, pcr_cloud** out_normals)
{
    if (out_cloud) *out_cloud = nullptr;
    if (out_normals) *out_normals = nullptr;
    if (n_out) *n_out = 0;
    if (!ctx || !normals || !bins || !n_out) return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32");
    if (bins[0] < 1 || bins[1] < 1 || bins[2] < 1 || (unsigned long long)bins[0] * bins[1] > (1ull << 20) ||
        (unsigned long long)bins[0] * bins[1] * bins[2] > (1ull << 20))
        return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32: every bin count must be >= 1 and their product <= 2^20");
    if ((gather_cloud != nullptr) != (out_cloud != nullptr)) return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32: gather_cloud and out_cloud go together");
    if (gather_cloud && gather_cloud->n != normals->n) return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32: one normal per point of gather_cloud");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = normals->n;
    if (n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32: cloud too large");
    const size_t want = std::min(sample, n);
    if (want > 0 && !indices) return fail(ctx, PCR_ERR_ARG, "pcr_normal_space_sample_f32: indices is NULL");
    NsParams p{};
    p.bx = bins[0]; p.by = bins[1]; p.bz = bins[2]; p.nbins = bins[0] * bins[1] * bins[2];
    p.seed = seed; p.sample = sample;
    const unsigned rank_bits = 20 + bit_length(n);                 // (rank << 20 | bin) and a plain index both stay below 2^rank_bits
    p.sentinel = 1ull << rank_bits;
    uint32_t n_valid = 0;
    const uint32_t* order = nullptr;
    if (n > 0) {
        size_t temp_bytes = 0;
        sort_pairs_u64_u32(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, n, 0, 64, ctx->stream);
        unsigned long long *k_a, *k_b;
        uint32_t *v_a, *v_b, *bin_of, *start, *cnt_dev;
        void* sort_temp;
        Layout L;
        L.add(&k_a, n);
        L.add(&k_b, n);
        L.add(&v_a, n);
        L.add(&v_b, n);
        L.add(&bin_of, n);
        L.add(&start, (size_t)p.nbins + 1);
        L.add(&cnt_dev, 1);
        L.add(&sort_temp, temp_bytes);
        int rc = bind_scratch(ctx, L);
        if (rc) return rc;
        const dim3 gridn = blocks_for(n);
        PCR_HIP(ctx, hipMemsetAsync(cnt_dev, 0, 4, ctx->stream));
        {
            ProfScope ps(ctx, "nss_keys");
            hipLaunchKernelGGL(ns_keys_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, normals->x(), normals->y(), normals->z(), (uint32_t)n, p, bin_of, k_a, v_a, cnt_dev);
        }
        {
            ProfScope ps(ctx, "nss_sort");
            // by key (ties: ascending index, the sort is stable), then by bin: (bin, key, index) order, keys in k_b, indices in v_a
            PCR_HIP(ctx, sort_pairs_u64_u32(sort_temp, temp_bytes, k_a, k_b, v_a, v_b, n, 0, 64, ctx->stream));
            hipLaunchKernelGGL(ns_bin_keys_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, bin_of, v_b, (uint32_t)n, k_a);
            PCR_HIP(ctx, sort_pairs_u64_u32(sort_temp, temp_bytes, k_a, k_b, v_b, v_a, n, 0, std::max(1u, bit_length(p.nbins)), ctx->stream));
        }
        {
            ProfScope ps(ctx, "nss_rank");
            hipLaunchKernelGGL(ns_starts_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, k_b, (uint32_t)n, p.nbins, start);
            hipLaunchKernelGGL(ns_rank_keys_kernel, gridn, dim3(SM_BLOCK), 0, ctx->stream, k_b, v_a, start, cnt_dev, (uint32_t)n, p, k_a);
            PCR_HIP(ctx, sort_pairs_u64_u32(sort_temp, temp_bytes, k_a, k_b, v_a, v_b, n, 0, rank_bits + 1, ctx->stream));
        }
        order = v_b;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&n_valid, cnt_dev, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && want) e = hipMemcpyAsync(indices, v_b, want * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_normal_space_sample_f32", e);
        if (n_valid > n) return fail(ctx, PCR_ERR_STATE, "pcr_normal_space_sample_f32: more samplable points than points");
    }
    const size_t m = std::min(sample, (size_t)n_valid);
    // ---- the gathered clouds (the scratch still holds the order)
    pcr_cloud *oc = nullptr, *on = nullptr;
    int rc = PCR_OK;
    if (out_cloud) rc = cloud_alloc(ctx, m, &oc);
    if (rc == PCR_OK && out_normals) rc = cloud_alloc(ctx, m, &on);
    if (rc) { pcr_cloud_destroy(ctx, oc); pcr_cloud_destroy(ctx, on); return rc; }
    if (oc || on) {
        ProfScope ps(ctx, "nss_gather");
        if (oc)
            hipLaunchKernelGGL(ns_gather_kernel, blocks_for(oc->cap), dim3(SM_BLOCK), 0, ctx->stream, gather_cloud->x(), gather_cloud->y(), gather_cloud->z(),
                               (uint32_t)n, order, (uint32_t)m, (uint32_t)oc->cap, oc->x(), oc->y(), oc->z());
        if (on)
            hipLaunchKernelGGL(ns_gather_kernel, blocks_for(on->cap), dim3(SM_BLOCK), 0, ctx->stream, normals->x(), normals->y(), normals->z(), (uint32_t)n, order,
                               (uint32_t)m, (uint32_t)on->cap, on->x(), on->y(), on->z());
    }
    if (oc || on) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { pcr_cloud_destroy(ctx, oc); pcr_cloud_destroy(ctx, on); return fail(ctx, PCR_ERR_HIP, "pcr_normal_space_sample_f32: gather", e); }
    }
    prof_flush(ctx);
    if (out_cloud) *out_cloud = oc;
    if (out_normals) *out_normals = on;
    *n_out = m;
    return PCR_OK;
}
