// boxes.hip — the two box operators of HomeworkFinal: the points inside a set of ORIENTED boxes (dataset_building/dataset_build.py:97-125,
// Open3D's OrientedBoundingBox::GetPointIndicesWithinBoundingBox) and the AXIS-ALIGNED box of every cluster (foreground_obj_cls.py:190-199).
// The contracts are written out above pcr_points_in_boxes_f64 / pcr_label_aabb_f32 in include/pcr.h; this file follows them.
//
//   points in boxes   The cloud is cut into TILES of pib_tile points that never cross a segment, so the boxes a workgroup tests are the same
//     pib_kernel<false>   for all its points (wave-uniform reads).  A workgroup stages its tile in LDS once (every point is read from HBM once
//     (pib_count)         per pass), then walks its segment's boxes PIB_BOXC at a time: one ballot per (64-point chunk, box) goes to LDS, one
//                         lane per box adds the chunk popcounts up to the (tile, box) count.  The counts lie box-major, tile-minor, which is
//     scan                the order of the output: ONE exclusive scan over that array (u64, three launches, any length: the top level loops
//                         with a carry) gives every (tile, box) its first position in idx, every box its row_ptr and the total.
//     pib_kernel<true>    The second pass forms the same ballots, one lane per box turns them into per-chunk offsets, and every member is
//     (pib_fill)          written at base + offset of its chunk + popcount(mask below its lane): ascending index, no atomic anywhere.
//   label boxes       min / max are order-free: one integer-ordered atomic per (point, coordinate, bound), or one per wave where the 64 labels
//     (label_aabb)        of a wave agree (DBSCAN's labels come in runs).
#include "pcr_internal.hpp"
#include "f32_key.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int PIB_BLOCK = 256;
constexpr uint32_t PIB_TILE_MIN = 64, PIB_TILE_MAX = 2048, PIB_TILE_DEFAULT = 512;      // points per workgroup (tune key pib_tile), a multiple of 64
constexpr uint32_t PIB_BOXC = 32;                                                        // boxes per LDS round of ballots
constexpr uint32_t PIB_CHUNKS_MAX = PIB_TILE_MAX / 64;
constexpr uint32_t PIB_SCAN_PER_THREAD = 8, PIB_SCAN_TILE = PIB_BLOCK * PIB_SCAN_PER_THREAD;

// a box as the kernel reads it: the half extents are formed on the host (extent * 0.5, the same f64 product); a box with a non-finite field
// arrives as all NaN, so every comparison against it is false
struct BoxDev {
    double c[3], R[9], half[3];
};

// one workgroup's share: points [p0, p0 + np) of the cloud, all of segment-local index local0 ..., against boxes [b0, b0 + nb);
// its (tile, box k) count lies at cnt[cnt0 + k * stride]
struct PibTile {
    uint32_t p0, np, local0, b0, nb, stride;
    unsigned long long cnt0;
};

__device__ __forceinline__ bool pib_inside(double px, double py, double pz, const BoxDev& b)
{
    const double d0 = px - b.c[0], d1 = py - b.c[1], d2 = pz - b.c[2];
    const double t0 = (d0 * b.R[0] + d1 * b.R[3]) + d2 * b.R[6];
    const double t1 = (d0 * b.R[1] + d1 * b.R[4]) + d2 * b.R[7];
    const double t2 = (d0 * b.R[2] + d1 * b.R[5]) + d2 * b.R[8];
    return fabs(t0) <= b.half[0] && fabs(t1) <= b.half[1] && fabs(t2) <= b.half[2];      // a comparison with NaN is false
}

template <bool FILL>
__global__ __launch_bounds__(PIB_BLOCK) void pib_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                        const PibTile* __restrict__ tiles, const BoxDev* __restrict__ boxes, uint32_t* __restrict__ cnt,
                                                        const unsigned long long* __restrict__ offs, uint32_t* __restrict__ idx, uint32_t* __restrict__ hits)
{
    __shared__ float sx[PIB_TILE_MAX], sy[PIB_TILE_MAX], sz[PIB_TILE_MAX];
    __shared__ uint32_t sh[PIB_TILE_MAX];                                   // hits of every point of the tile (count pass)
    __shared__ unsigned long long smask[PIB_CHUNKS_MAX][PIB_BOXC];          // the ballot of (chunk, box of this round)
    __shared__ uint32_t spre[PIB_CHUNKS_MAX][PIB_BOXC];                     // fill pass: members of the box in the chunks before
    const PibTile t = tiles[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t nchunk = (t.np + 63u) >> 6;                              // <= PIB_CHUNKS_MAX: the host cuts tiles of at most PIB_TILE_MAX points
    for (uint32_t i = tid; i < t.np; i += PIB_BLOCK) {
        sx[i] = x[t.p0 + i];
        sy[i] = y[t.p0 + i];
        sz[i] = z[t.p0 + i];
        sh[i] = 0u;
    }
    __syncthreads();
    for (uint32_t bc = 0; bc < t.nb; bc += PIB_BOXC) {
        const uint32_t nbc = min(PIB_BOXC, t.nb - bc);
        const BoxDev* bx = boxes + t.b0 + bc;
        for (uint32_t i = tid; i < nchunk * 64u; i += PIB_BLOCK) {         // whole waves: i - lane is the same for the 64 lanes
            const bool valid = i < t.np;
            const double px = valid ? (double)sx[i] : 0.0, py = valid ? (double)sy[i] : 0.0, pz = valid ? (double)sz[i] : 0.0;
            uint32_t h = 0;
            for (uint32_t k = 0; k < nbc; k++) {
                const bool in = valid && pib_inside(px, py, pz, bx[k]);
                const unsigned long long m = __ballot(in);
                if (lane == 0) smask[i >> 6][k] = m;
                h += in ? 1u : 0u;
            }
            if (!FILL && valid) sh[i] += h;
        }
        __syncthreads();
        if (!FILL) {
            if (tid < nbc) {
                uint32_t c = 0;
                for (uint32_t j = 0; j < nchunk; j++) c += (uint32_t)__popcll(smask[j][tid]);
                cnt[t.cnt0 + (unsigned long long)(bc + tid) * t.stride] = c;
            }
        } else {
            if (tid < nbc) {
                uint32_t c = 0;
                for (uint32_t j = 0; j < nchunk; j++) {
                    spre[j][tid] = c;
                    c += (uint32_t)__popcll(smask[j][tid]);
                }
            }
            __syncthreads();
            for (uint32_t i = tid; i < t.np; i += PIB_BLOCK) {
                const uint32_t j = i >> 6;
                for (uint32_t k = 0; k < nbc; k++) {
                    const unsigned long long m = smask[j][k];
                    if ((m >> lane) & 1ull) {
                        const unsigned long long base = offs[t.cnt0 + (unsigned long long)(bc + k) * t.stride];
                        idx[base + spre[j][k] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t.local0 + i;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!FILL && hits)
        for (uint32_t i = tid; i < t.np; i += PIB_BLOCK) hits[t.p0 + i] = sh[i];
}

// ---- exclusive scan u32 -> u64 over n entries: block sums, one workgroup over the block sums (a loop with a carry: any number of them), apply
__device__ __forceinline__ unsigned long long pib_block_exscan(unsigned long long v, unsigned long long* s, unsigned long long* total)
{
    const uint32_t tid = threadIdx.x;                  // Hillis-Steele over PIB_BLOCK values in LDS; integer sums: any order gives the same bits
    s[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < PIB_BLOCK; d <<= 1) {
        const unsigned long long a = tid >= d ? s[tid - d] : 0ull;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    const unsigned long long incl = s[tid];
    *total = s[PIB_BLOCK - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(PIB_BLOCK) void pib_scan_sums_kernel(const uint32_t* __restrict__ in, unsigned long long n, unsigned long long* __restrict__ bsum)
{
    __shared__ unsigned long long s[PIB_BLOCK];
    const unsigned long long e0 = (unsigned long long)blockIdx.x * PIB_SCAN_TILE + (unsigned long long)threadIdx.x * PIB_SCAN_PER_THREAD;
    unsigned long long v = 0;
    for (uint32_t k = 0; k < PIB_SCAN_PER_THREAD; k++)
        if (e0 + k < n) v += in[e0 + k];
    unsigned long long total;
    pib_block_exscan(v, s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// bsum[nblk] -> its exclusive scan in place, out[n] = the sum of everything (the entry behind the last: a trailing box without a tile reads it)
__global__ __launch_bounds__(PIB_BLOCK) void pib_scan_top_kernel(unsigned long long* __restrict__ bsum, unsigned long long nblk, unsigned long long* __restrict__ out,
                                                                 unsigned long long n)
{
    __shared__ unsigned long long s[PIB_BLOCK];
    unsigned long long carry = 0;
    for (unsigned long long b0 = 0; b0 < nblk; b0 += PIB_BLOCK) {
        const unsigned long long i = b0 + threadIdx.x;
        const unsigned long long v = i < nblk ? bsum[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = pib_block_exscan(v, s, &total);
        if (i < nblk) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(PIB_BLOCK) void pib_scan_apply_kernel(const uint32_t* __restrict__ in, unsigned long long n, const unsigned long long* __restrict__ bbase,
                                                                   unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long s[PIB_BLOCK];
    const unsigned long long e0 = (unsigned long long)blockIdx.x * PIB_SCAN_TILE + (unsigned long long)threadIdx.x * PIB_SCAN_PER_THREAD;
    uint32_t a[PIB_SCAN_PER_THREAD];
    unsigned long long v = 0;
    for (uint32_t k = 0; k < PIB_SCAN_PER_THREAD; k++) {
        a[k] = e0 + k < n ? in[e0 + k] : 0u;
        v += a[k];
    }
    unsigned long long total;
    unsigned long long run = bbase[blockIdx.x] + pib_block_exscan(v, s, &total);
    for (uint32_t k = 0; k < PIB_SCAN_PER_THREAD; k++) {
        if (e0 + k < n) out[e0 + k] = run;
        run += a[k];
    }
}

// row_ptr[b] = the first position of box b's first (tile, box) entry; row_ptr[n_boxes] = the total
__global__ void pib_row_ptr_kernel(const unsigned long long* __restrict__ offs, const unsigned long long* __restrict__ box_off, uint32_t n_boxes, unsigned long long n,
                                   unsigned long long* __restrict__ row_ptr)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_boxes) row_ptr[b] = offs[box_off[b]];
    if (b == n_boxes) row_ptr[b] = offs[n];
}

// ---- label boxes ---------------------------------------------------------------------------------------------------------------------
// the order of the floats as unsigned integers (f32_key.hpp): -inf < ... < -0 < +0 < ... < +inf
constexpr uint32_t KEY_NONE_MIN = 0xFFFFFFFFu, KEY_NONE_MAX = 0u;      // "no value" of a lane under min / max (a NaN coordinate)

__global__ void aabb_init_kernel(uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ count, uint32_t n_clusters)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    for (int a = 0; a < 3; a++) {
        lo[3 * c + a] = KEY_PINF;
        hi[3 * c + a] = KEY_NINF;
    }
    count[c] = 0u;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

__global__ __launch_bounds__(PIB_BLOCK) void label_aabb_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                               const int32_t* __restrict__ labels, uint32_t n, uint32_t n_clusters, uint32_t* __restrict__ lo,
                                                               uint32_t* __restrict__ hi, uint32_t* __restrict__ count)
{
    const uint32_t i = blockIdx.x * PIB_BLOCK + threadIdx.x;                  // whole waves reach the shuffles: no early return
    const int32_t l = i < n ? labels[i] : -1;
    const bool member = l >= 0 && (uint32_t)l < n_clusters;                   // the host has checked the range; a lane never writes outside the tables
    const float p[3] = { i < n ? x[i] : 0.f, i < n ? y[i] : 0.f, i < n ? z[i] : 0.f };
    uint32_t kmin[3], kmax[3];
    for (int a = 0; a < 3; a++) {
        const bool use = member && p[a] == p[a];                              // a NaN coordinate is skipped in that coordinate
        kmin[a] = use ? f32_key(p[a]) : KEY_NONE_MIN;
        kmax[a] = use ? f32_key(p[a]) : KEY_NONE_MAX;
    }
    const int32_t l0 = __shfl(l, 0, 64);
    if (__all(l == l0)) {                                                     // one label in the wave (or none): one atomic per bound
        if (l0 < 0 || (uint32_t)l0 >= n_clusters) return;
        for (int a = 0; a < 3; a++) {
            kmin[a] = wave_min_u32(kmin[a]);
            kmax[a] = wave_max_u32(kmax[a]);
        }
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(&count[l0], 64u);
            for (int a = 0; a < 3; a++) {
                if (kmin[a] != KEY_NONE_MIN) atomicMin(&lo[3 * l0 + a], kmin[a]);
                if (kmax[a] != KEY_NONE_MAX) atomicMax(&hi[3 * l0 + a], kmax[a]);
            }
        }
        return;
    }
    if (!member) return;
    atomicAdd(&count[l], 1u);
    for (int a = 0; a < 3; a++) {
        if (kmin[a] != KEY_NONE_MIN) atomicMin(&lo[3 * l + a], kmin[a]);
        if (kmax[a] != KEY_NONE_MAX) atomicMax(&hi[3 * l + a], kmax[a]);
    }
}

bool pib_seg_ok(const uint32_t* p, size_t n_seg, size_t limit)
{
    for (size_t s = 0; s < n_seg; s++)
        if (p[s] > p[s + 1]) return false;
    return p[n_seg] <= limit;
}

uint32_t pib_tile_points(const pcr_ctx* ctx)
{
    int64_t t = tune_get(ctx, "pib_tile", PIB_TILE_DEFAULT);
    t = std::max<int64_t>(PIB_TILE_MIN, std::min<int64_t>(PIB_TILE_MAX, t));
    return (uint32_t)(t & ~(int64_t)63);
}

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_points_in_boxes_f64(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg, const pcr_obox* boxes,
                                       const uint32_t* box_seg_ptr, uint64_t* row_ptr, uint32_t* idx, size_t idx_cap, uint32_t* hits, uint64_t* total)
{
    if (total) *total = 0;
    if (!ctx || !cloud || !seg_ptr || !box_seg_ptr || !row_ptr) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64");
    if (n_seg > 0x7FFFFFF0ull || cloud->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: too large");
    if (!pib_seg_ok(seg_ptr, n_seg, cloud->n)) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: seg_ptr must ascend and end inside the cloud");
    if (!pib_seg_ok(box_seg_ptr, n_seg, 0x7FFFFFF0ull)) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: box_seg_ptr must ascend (at most 2^31 - 16 boxes)");
    const size_t n_boxes = box_seg_ptr[n_seg];            // the boxes array holds box_seg_ptr[n_seg] entries; those below box_seg_ptr[0] belong to no segment
    for (size_t b = 0; b <= n_boxes; b++) row_ptr[b] = 0;
    if (n_boxes && !boxes) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: boxes is NULL");
    std::vector<BoxDev> bdev(n_boxes);
    for (size_t b = 0; b < n_boxes; b++) {
        const pcr_obox& o = boxes[b];
        bool finite = true;
        for (int a = 0; a < 3; a++) {
            if (o.extent[a] < 0.0) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: a negative extent");
            finite = finite && std::isfinite(o.centre[a]) && std::isfinite(o.extent[a]);
        }
        for (int a = 0; a < 9; a++) finite = finite && std::isfinite(o.R[a]);
        BoxDev& d = bdev[b];
        for (int a = 0; a < 3; a++) {
            d.c[a] = finite ? o.centre[a] : NAN;
            d.half[a] = finite ? o.extent[a] * 0.5 : NAN;
        }
        for (int a = 0; a < 9; a++) d.R[a] = finite ? o.R[a] : NAN;
    }
    const size_t n = cloud->n;
    if (hits) memset(hits, 0, n * sizeof(uint32_t));      // a point outside every segment, or of a segment without a box, is in no box
    if (n_seg == 0 || n_boxes == 0) return PCR_OK;
    // ---- tiles: one per pib_tile points of a segment that has boxes; counts box-major, tile-minor: the order of idx
    const uint32_t tile = pib_tile_points(ctx);
    std::vector<PibTile> tiles;
    std::vector<unsigned long long> box_off(n_boxes, 0ull);
    unsigned long long E = 0;
    for (size_t b = 0; b < box_seg_ptr[0]; b++) box_off[b] = 0;
    for (size_t s = 0; s < n_seg; s++) {
        const uint32_t p0 = seg_ptr[s], np = seg_ptr[s + 1] - p0, b0 = box_seg_ptr[s], nb = box_seg_ptr[s + 1] - b0;
        const uint32_t nt = (np + tile - 1) / tile;
        for (uint32_t k = 0; k < nb; k++) box_off[b0 + k] = E + (unsigned long long)k * nt;
        if (nb == 0) continue;
        for (uint32_t t = 0; t < nt; t++) tiles.push_back({ p0 + t * tile, std::min(tile, np - t * tile), t * tile, b0, nb, nt, E + t });
        E += (unsigned long long)nb * nt;
        if (E > 0x7FFFFFF0ull || tiles.size() > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: boxes x tiles too large");
    }
    uint64_t tot = 0;
    if (E == 0) {                                          // boxes, but not one point to test
        if (idx_cap < tot) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: idx_cap");
        return PCR_OK;
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nblk = (size_t)((E + PIB_SCAN_TILE - 1) / PIB_SCAN_TILE);
    PibTile* tiles_dev;
    BoxDev* boxes_dev;
    uint32_t *cnt_dev, *hits_dev;
    unsigned long long *offs_dev, *bsum_dev, *box_off_dev, *row_ptr_dev;
    Layout L;
    L.add(&tiles_dev, tiles.size());
    L.add(&boxes_dev, n_boxes);
    L.add(&cnt_dev, (size_t)E);
    L.add(&offs_dev, (size_t)E + 1);
    L.add(&bsum_dev, nblk);
    L.add(&box_off_dev, n_boxes);
    L.add(&row_ptr_dev, n_boxes + 1);
    L.add(&hits_dev, hits ? n : 0);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    if (!hits) hits_dev = nullptr;
    PCR_HIP(ctx, hipMemcpyAsync(tiles_dev, tiles.data(), tiles.size() * sizeof(PibTile), hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(boxes_dev, bdev.data(), n_boxes * sizeof(BoxDev), hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(box_off_dev, box_off.data(), n_boxes * 8, hipMemcpyHostToDevice, ctx->stream));
    if (hits) PCR_HIP(ctx, hipMemsetAsync(hits_dev, 0, n * 4, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    {
        ProfScope ps(ctx, "pib_count");
        hipLaunchKernelGGL((pib_kernel<false>), dim3((unsigned)tiles.size()), dim3(PIB_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), tiles_dev, boxes_dev,
                           cnt_dev, (const unsigned long long*)nullptr, (uint32_t*)nullptr, hits_dev);
    }
    {
        ProfScope ps(ctx, "pib_scan");
        hipLaunchKernelGGL(pib_scan_sums_kernel, dim3((unsigned)nblk), dim3(PIB_BLOCK), 0, ctx->stream, cnt_dev, E, bsum_dev);
        hipLaunchKernelGGL(pib_scan_top_kernel, dim3(1), dim3(PIB_BLOCK), 0, ctx->stream, bsum_dev, (unsigned long long)nblk, offs_dev, E);
        hipLaunchKernelGGL(pib_scan_apply_kernel, dim3((unsigned)nblk), dim3(PIB_BLOCK), 0, ctx->stream, cnt_dev, E, bsum_dev, offs_dev);
        hipLaunchKernelGGL(pib_row_ptr_kernel, dim3((unsigned)((n_boxes + 1 + PIB_BLOCK - 1) / PIB_BLOCK)), dim3(PIB_BLOCK), 0, ctx->stream, offs_dev, box_off_dev,
                           (uint32_t)n_boxes, E, row_ptr_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(row_ptr, row_ptr_dev, (n_boxes + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (hits) PCR_HIP(ctx, hipMemcpyAsync(hits, hits_dev, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tot = row_ptr[n_boxes];
    if (total) *total = tot;
    for (size_t b = 0; b < n_boxes; b++)                   // rows ascend and no row is longer than its segment: a violation is a corrupt run, not an answer
        if (row_ptr[b] > row_ptr[b + 1] || row_ptr[b + 1] - row_ptr[b] > n) return fail(ctx, PCR_ERR_STATE, "pcr_points_in_boxes_f64: corrupt row_ptr");
    if (idx_cap < tot) {
        prof_flush(ctx);
        return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: idx_cap is smaller than the total (row_ptr and total are valid)");
    }
    if (tot == 0) { prof_flush(ctx); return PCR_OK; }
    if (!idx) return fail(ctx, PCR_ERR_ARG, "pcr_points_in_boxes_f64: idx is NULL");
    uint32_t* idx_dev;
    Layout LA;
    LA.add(&idx_dev, (size_t)tot);
    rc = bind_aux(ctx, LA);
    if (rc) return rc;
    {
        ProfScope ps(ctx, "pib_fill");
        hipLaunchKernelGGL((pib_kernel<true>), dim3((unsigned)tiles.size()), dim3(PIB_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), tiles_dev, boxes_dev,
                           (uint32_t*)nullptr, offs_dev, idx_dev, (uint32_t*)nullptr);
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(idx, idx_dev, (size_t)tot * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_label_aabb_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels, size_t n_clusters, float* aabb, uint32_t* counts)
{
    if (!ctx || !cloud) return fail(ctx, PCR_ERR_ARG, "pcr_label_aabb_f32");
    const size_t n = cloud->n;
    if (n > 0x7FFFFFF0ull || n_clusters > 0x7FFFFFF0ull / 3) return fail(ctx, PCR_ERR_ARG, "pcr_label_aabb_f32: too large");
    if (n && !labels) return fail(ctx, PCR_ERR_ARG, "pcr_label_aabb_f32: labels is NULL");
    for (size_t i = 0; i < n; i++)
        if (labels[i] < -1 || (labels[i] >= 0 && (size_t)labels[i] >= n_clusters)) return fail(ctx, PCR_ERR_ARG, "pcr_label_aabb_f32: a label outside [-1, n_clusters)");
    if (n_clusters == 0) return PCR_OK;
    if (!aabb) return fail(ctx, PCR_ERR_ARG, "pcr_label_aabb_f32: aabb is NULL");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* labels_dev;
    uint32_t *lo_dev, *hi_dev, *count_dev;
    Layout L;
    L.add(&labels_dev, n);
    L.add(&lo_dev, 3 * n_clusters);
    L.add(&hi_dev, 3 * n_clusters);
    L.add(&count_dev, n_clusters);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    if (n) PCR_HIP(ctx, hipMemcpyAsync(labels_dev, labels, n * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    {
        ProfScope ps(ctx, "label_aabb");
        hipLaunchKernelGGL(aabb_init_kernel, dim3((unsigned)((n_clusters + PIB_BLOCK - 1) / PIB_BLOCK)), dim3(PIB_BLOCK), 0, ctx->stream, lo_dev, hi_dev, count_dev,
                           (uint32_t)n_clusters);
        if (n)
            hipLaunchKernelGGL(label_aabb_kernel, dim3((unsigned)((n + PIB_BLOCK - 1) / PIB_BLOCK)), dim3(PIB_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(),
                               labels_dev, (uint32_t)n, (uint32_t)n_clusters, lo_dev, hi_dev, count_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> lo(3 * n_clusters), hi(3 * n_clusters);
    PCR_HIP(ctx, hipMemcpyAsync(lo.data(), lo_dev, lo.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(hi.data(), hi_dev, hi.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) PCR_HIP(ctx, hipMemcpyAsync(counts, count_dev, n_clusters * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    for (size_t c = 0; c < n_clusters; c++)
        for (int a = 0; a < 3; a++) {
            aabb[6 * c + a] = f32_from_key(lo[3 * c + a]);
            aabb[6 * c + 3 + a] = f32_from_key(hi[3 * c + a]);
        }
    return PCR_OK;
}
