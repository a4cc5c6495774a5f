// pointnet.hip — the sampling and grouping front of HomeworkFinal's PointNet++ (models/pointnet_util.py:66-156) and the object extraction
// loop of HomeworkFinal/foreground_obj_cls.py:143-180.  The contracts are written out above pcr_fps_f32 / pcr_ball_query_f32 /
// pcr_group_points_f32 / pcr_objects_from_labels_f32 in include/pcr.h; this file follows them operation by operation.
//
//   farthest point sampling   a chain of npoint dependent argmax steps.  A segment of up to FPS_SMALL_MAX points lives in the registers of
//     fps_small_kernel          ONE workgroup for the whole chain: 4 or 16 points per lane (coordinates + running distance), the centre of a
//                               step is carried through the argmax together with its key (no dependent load), the argmax is four DPP steps
//                               inside a row + four v_readlane across rows, and — from two waves on — one LDS exchange and one barrier.  A
//                               segment of up to 256 points is one wave: no barrier in the loop at all.
//     fps_large_kernel          larger segments: one launch per pick.  A launch first takes the maximum of the per-workgroup candidates the
//                               launch before left behind (every workgroup of the segment does that for itself: the kernel boundary is the
//                               only hand-off between workgroups — no ticket, no fence, no wait), then updates its share of the running
//                               distances and leaves its own candidate.  Several large segments share the launches.
//   ball query                one wave per centre walks its segment in index order 64 points at a time; the hits of a chunk are placed by the
//                               prefix popcount of their ballot and the walk stops at the chunk that fills the row.
//   group                     one lane per output element: (xyz[idx] - centre | features[idx]).
//   objects                   stable sort by label (sort.hip) -> segments; min / max z per cluster; FPS (f64 mode) or pad; centroid.
#include "pcr_internal.hpp"

#include "sort.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int PN_BLOCK = 256;
constexpr uint32_t FPS_SMALL_MAX = 16384;       // 1024 lanes x 16 points: 64 (f32) / 80 (f64) of the 128 VGPRs a lane of a 16-wave workgroup has
constexpr uint32_t FPS_LARGE_WG_MAX = 512;      // workgroups per large segment (each strides over the segment)
constexpr uint32_t FPS_LARGE_PER_WG = 2048;     // points per workgroup below that cap

__device__ __forceinline__ bool pn_finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

template <int CTRL>
__device__ __forceinline__ uint32_t pn_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float pn_dppf(float v) { return __uint_as_float(pn_dpp<CTRL>(__float_as_uint(v))); }
__device__ __forceinline__ uint32_t pn_rl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float pn_rlf(float v, int l) { return __uint_as_float(pn_rl(__float_as_uint(v), l)); }

// f32 mode: the 64-bit key dist_bits << 32 | ~idx under max (legal because a running distance is >= +0); 0 = "no candidate" (a point with
// a non-finite coordinate carries the distance -inf, a slot beyond the segment too), which index() turns into point 0
struct KeyF32 {
    unsigned long long k;
    __device__ __forceinline__ static KeyF32 none() { return { 0ull }; }
    __device__ __forceinline__ static KeyF32 make(float d, uint32_t i) { return { d < 0.0f ? 0ull : ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)~i }; }
    __device__ __forceinline__ bool beats(const KeyF32& o) const { return k > o.k; }
    template <int CTRL>
    __device__ __forceinline__ KeyF32 dpp() const { return { ((unsigned long long)pn_dpp<CTRL>((uint32_t)(k >> 32)) << 32) | pn_dpp<CTRL>((uint32_t)k) }; }
    __device__ __forceinline__ KeyF32 lane(int l) const { return { ((unsigned long long)pn_rl((uint32_t)(k >> 32), l) << 32) | pn_rl((uint32_t)k, l) }; }
    __device__ __forceinline__ uint32_t index() const { return k == 0ull ? 0u : ~(uint32_t)k; }
};

// f64 mode (and the candidates large segments exchange, in both modes): the pair (distance, index), larger distance first, then lower index
struct KeyF64 {
    double d;
    uint32_t i;
    __device__ __forceinline__ static KeyF64 none() { return { -__builtin_inf(), 0xFFFFFFFFu }; }
    __device__ __forceinline__ static KeyF64 make(double d, uint32_t i) { return { d, i }; }
    __device__ __forceinline__ bool beats(const KeyF64& o) const { return d > o.d || (d == o.d && i < o.i); }
    template <int CTRL>
    __device__ __forceinline__ KeyF64 dpp() const
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(d);
        const unsigned long long w = ((unsigned long long)pn_dpp<CTRL>((uint32_t)(b >> 32)) << 32) | pn_dpp<CTRL>((uint32_t)b);
        return { __longlong_as_double((long long)w), pn_dpp<CTRL>(i) };
    }
    __device__ __forceinline__ KeyF64 lane(int l) const
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(d);
        const unsigned long long w = ((unsigned long long)pn_rl((uint32_t)(b >> 32), l) << 32) | pn_rl((uint32_t)b, l);
        return { __longlong_as_double((long long)w), pn_rl(i, l) };
    }
    __device__ __forceinline__ uint32_t index() const { return i == 0xFFFFFFFFu ? 0u : i; }
};

template <class K>
__device__ __forceinline__ void pn_take(K& b, float& x, float& y, float& z, const K& ob, float ox, float oy, float oz)
{
    if (ob.beats(b)) { b = ob; x = ox; y = oy; z = oz; }
}

template <class K, int CTRL>
__device__ __forceinline__ void pn_step(K& b, float& x, float& y, float& z)
{
    const K ob = b.template dpp<CTRL>();
    const float ox = pn_dppf<CTRL>(x), oy = pn_dppf<CTRL>(y), oz = pn_dppf<CTRL>(z);
    pn_take(b, x, y, z, ob, ox, oy, oz);
}

// best candidate of the 16 lanes of a DPP row, in every lane of the row's key (the coordinates that travel with it are read from one lane afterwards)
template <class K>
__device__ __forceinline__ void pn_row_argmax(K& b, float& x, float& y, float& z)
{
    pn_step<K, 0xB1>(b, x, y, z);       // quad_perm [1, 0, 3, 2]
    pn_step<K, 0x4E>(b, x, y, z);       // quad_perm [2, 3, 0, 1]
    pn_step<K, 0x141>(b, x, y, z);      // row_half_mirror
    pn_step<K, 0x140>(b, x, y, z);      // row_mirror
}

// best candidate of the wave, wave-uniform, with the coordinates of the point that holds it
template <class K>
__device__ __forceinline__ void pn_wave_argmax(K& b, float& x, float& y, float& z)
{
    pn_row_argmax(b, x, y, z);
    K kb = b.lane(0);
    int s = 0;
    const K k1 = b.lane(16), k2 = b.lane(32), k3 = b.lane(48);
    if (k1.beats(kb)) { kb = k1; s = 16; }
    if (k2.beats(kb)) { kb = k2; s = 32; }
    if (k3.beats(kb)) { kb = k3; s = 48; }
    b = kb;
    x = pn_rlf(x, s); y = pn_rlf(y, s); z = pn_rlf(z, s);
}

template <class K>
struct FpsEntry {
    K k;
    float x, y, z;
};

// best candidate of a workgroup of W waves (W a power of two <= 16): one LDS exchange, ONE barrier; `slot` = the W entries of this exchange
template <class K, int W>
__device__ __forceinline__ void pn_block_argmax(K& b, float& x, float& y, float& z, FpsEntry<K>* slot, int wave, int lane)
{
    pn_wave_argmax(b, x, y, z);
    if (W > 1) {
        if (lane == 0) slot[wave] = { b, x, y, z };
        __syncthreads();
        const FpsEntry<K> e = slot[lane & (W - 1)];      // the W entries lie in the first DPP row of every wave
        b = e.k; x = e.x; y = e.y; z = e.z;
        pn_row_argmax(b, x, y, z);
        b = b.lane(0);
        x = pn_rlf(x, 0); y = pn_rlf(y, 0); z = pn_rlf(z, 0);
    }
}

template <bool F64>
struct FpsArith;
template <>
struct FpsArith<false> {
    typedef float D;
    typedef KeyF32 K;
    __device__ __forceinline__ static float d2(float px, float py, float pz, float cx, float cy, float cz)
    {
        const float dx = px - cx, dy = py - cy, dz = pz - cz;
        return (dx * dx + dy * dy) + dz * dz;
    }
    __device__ __forceinline__ static float init(bool ok) { return ok ? 1e10f : -__builtin_inff(); }
};
template <>
struct FpsArith<true> {
    typedef double D;
    typedef KeyF64 K;
    __device__ __forceinline__ static double d2(float px, float py, float pz, float cx, float cy, float cz)
    {
        const double dx = (double)px - (double)cx, dy = (double)py - (double)cy, dz = (double)pz - (double)cz;
        return (dx * dx + dy * dy) + dz * dz;
    }
    __device__ __forceinline__ static double init(bool ok) { return ok ? 1e10 : -__builtin_inf(); }
};

// ---- small segments: the whole chain in one workgroup, points and running distances in registers -----------------------------------------
template <bool F64, int T, int P>
__global__ __launch_bounds__(T) void fps_small_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                      const FpsJob* __restrict__ jobs, uint32_t npoint, uint32_t* __restrict__ out)
{
    typedef FpsArith<F64> A;
    typedef typename A::K K;
    typedef typename A::D D;
    constexpr int W = T / 64;
    __shared__ FpsEntry<K> ex[2][W];
    const FpsJob job = jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float px[P], py[P], pz[P];
    D d[P];
#pragma unroll
    for (int j = 0; j < P; j++) {
        const uint32_t i = (uint32_t)(j * T + tid);
        const float nan = __builtin_nanf("");
        float a = nan, b = nan, c = nan;
        if (i < job.n) { a = x[job.base + i]; b = y[job.base + i]; c = z[job.base + i]; }
        const bool ok = pn_finite3(a, b, c);           // false for the slots beyond the segment
        px[j] = ok ? a : nan; py[j] = b; pz[j] = c;    // a NaN coordinate: s is NaN, `s < d` never holds, the distance stays -inf
        d[j] = A::init(ok);
    }
    uint32_t c = job.start;                            // < job.n (checked by the host)
    float cx = x[job.base + c], cy = y[job.base + c], cz = z[job.base + c];
    uint32_t* o = out + (size_t)job.out_row * npoint;
    for (uint32_t step = 0; step < npoint; step++) {   // bounded by npoint; every pick is < job.n by construction
        if (tid == 0) o[step] = c;
        if (step + 1 == npoint) break;
        K best = K::none();
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
        for (int j = 0; j < P; j++) {
            const D s = A::d2(px[j], py[j], pz[j], cx, cy, cz);
            if (s < d[j]) d[j] = s;
            pn_take(best, bx, by, bz, K::make(d[j], (uint32_t)(j * T + tid)), px[j], py[j], pz[j]);      // ascending index inside a lane: strict `beats` keeps the lowest
        }
        pn_block_argmax<K, W>(best, bx, by, bz, ex[step & 1], wave, lane);
        c = best.index();
        cx = bx; cy = by; cz = bz;
    }
}

// ---- large segments: one launch per pick --------------------------------------------------------------------------------------------------
struct FpsLargeSeg {
    uint32_t base, n, start, out_row, wg0, nwg;
    unsigned long long dist_off;
};
typedef FpsEntry<KeyF64> FpsPart;       // what a workgroup leaves for the next launch (both modes: an f32 distance widens exactly)

template <bool F64>
__global__ __launch_bounds__(PN_BLOCK) void fps_large_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                             const FpsLargeSeg* __restrict__ tab, const uint32_t* __restrict__ wg_tab,
                                                             typename FpsArith<F64>::D* __restrict__ dist, const FpsPart* __restrict__ prev,
                                                             FpsPart* __restrict__ cur, uint32_t step, uint32_t npoint, uint32_t* __restrict__ out)
{
    typedef FpsArith<F64> A;
    typedef typename A::D D;
    constexpr int W = PN_BLOCK / 64;
    __shared__ FpsPart ex[2][W];
    const FpsLargeSeg t = tab[wg_tab[blockIdx.x]];
    const uint32_t w = blockIdx.x - t.wg0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t c;
    float cx, cy, cz;
    if (step == 0) {
        c = t.start;
        cx = x[t.base + c]; cy = y[t.base + c]; cz = z[t.base + c];
    } else {
        KeyF64 best = KeyF64::none();
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        for (uint32_t k = (uint32_t)tid; k < t.nwg; k += PN_BLOCK) {
            const FpsPart e = prev[t.wg0 + k];
            pn_take(best, bx, by, bz, e.k, e.x, e.y, e.z);
        }
        pn_block_argmax<KeyF64, W>(best, bx, by, bz, ex[0], wave, lane);
        c = best.index();
        cx = bx; cy = by; cz = bz;
    }
    if (w == 0 && tid == 0) out[(size_t)t.out_row * npoint + step] = c;
    if (step + 1 >= npoint) return;
    KeyF64 best = KeyF64::none();
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
    D* dseg = dist + t.dist_off;
    for (uint32_t i = w * PN_BLOCK + (uint32_t)tid; i < t.n; i += t.nwg * PN_BLOCK) {      // ascending index inside a lane
        const float a = x[t.base + i], b = y[t.base + i], q = z[t.base + i];
        D dd = step == 0 ? A::init(pn_finite3(a, b, q)) : dseg[i];
        const D s = A::d2(a, b, q, cx, cy, cz);
        if (s < dd) dd = s;                                                               // never for a non-finite point: s is NaN or +inf, dd is -inf
        dseg[i] = dd;
        pn_take(best, bx, by, bz, KeyF64::make((double)dd, i), a, b, q);
    }
    pn_block_argmax<KeyF64, W>(best, bx, by, bz, ex[1], wave, lane);
    if (tid == 0) cur[blockIdx.x] = { best, bx, by, bz };
}

// ---- ball query: one wave per centre ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PN_BLOCK) void ball_query_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                              const uint32_t* __restrict__ seg_ptr, const uint32_t* __restrict__ centre_seg, uint32_t n_centres,
                                                              float r2, uint32_t nsample, uint32_t* __restrict__ idx, uint32_t* __restrict__ counts)
{
    const uint32_t q = blockIdx.x * (PN_BLOCK / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (q >= n_centres) return;
    const int lane = threadIdx.x & 63;
    const uint32_t s = centre_seg[q], base = seg_ptr[s], n = seg_ptr[s + 1] - base;
    const float ax = qx[q], ay = qy[q], az = qz[q];
    uint32_t* row = idx + (size_t)q * nsample;
    uint32_t cnt = 0, first = n;
    for (uint32_t i0 = 0; i0 < n && cnt < nsample; i0 += 64) {                // bounded by the segment
        const uint32_t i = i0 + (uint32_t)lane;
        bool hit = false;
        if (i < n) {
            const float dx = ax - x[base + i], dy = ay - y[base + i], dz = az - z[base + i];
            hit = ((dx * dx + dy * dy) + dz * dz) <= r2;                       // false for NaN: a non-finite point is never a hit
        }
        const unsigned long long mask = __ballot(hit);
        if (mask != 0ull) {
            const uint32_t pos = cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (hit && pos < nsample) row[pos] = i;
            if (cnt == 0) first = i0 + (uint32_t)__builtin_ctzll(mask);
            cnt += (uint32_t)__popcll(mask);
        }
    }
    if (cnt > nsample) cnt = nsample;
    for (uint32_t p = cnt + (uint32_t)lane; p < nsample; p += 64) row[p] = first;      // the first hit, or the segment's size for an empty row
    if (lane == 0) counts[q] = cnt;
}

// ---- ball query at up to four radii: one wave per centre, ONE walk of the segment, one distance per point and chunk, one ballot per radius.
// Every radius keeps the state of ball_query_kernel (cnt, first) and stops taking hits at the chunk that fills its row, so its row and its
// count are what that kernel gives; the walk ends when every row is full.
struct BallMultiArgs {
    float r2[4];
    uint32_t nsample[4];
    uint32_t* idx[4];
    uint32_t* counts[4];
    uint32_t n_radii;
};

__global__ __launch_bounds__(PN_BLOCK) void ball_query_multi_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                                    const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                                    const uint32_t* __restrict__ seg_ptr, const uint32_t* __restrict__ centre_seg, uint32_t n_centres,
                                                                    const BallMultiArgs a)
{
    const uint32_t q = blockIdx.x * (PN_BLOCK / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (q >= n_centres) return;
    const int lane = threadIdx.x & 63;
    const uint32_t s = centre_seg[q], base = seg_ptr[s], n = seg_ptr[s + 1] - base;
    const float ax = qx[q], ay = qy[q], az = qz[q];
    uint32_t cnt[4] = { 0, 0, 0, 0 }, first[4] = { n, n, n, n };
    uint32_t open = 0;                                                         // radii whose row is not full yet
#pragma unroll
    for (int b = 0; b < 4; b++)
        if ((uint32_t)b < a.n_radii) open |= 1u << b;
    for (uint32_t i0 = 0; i0 < n && open != 0u; i0 += 64) {                    // bounded by the segment
        const uint32_t i = i0 + (uint32_t)lane;
        float d = __builtin_nanf("");                                          // no point: no hit at any radius
        if (i < n) {
            const float dx = ax - x[base + i], dy = ay - y[base + i], dz = az - z[base + i];
            d = (dx * dx + dy * dy) + dz * dz;
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (!(open & (1u << b))) continue;                                 // wave-uniform
            const bool hit = d <= a.r2[b];                                     // false for NaN: a non-finite point is never a hit
            const unsigned long long mask = __ballot(hit);
            if (mask != 0ull) {
                const uint32_t pos = cnt[b] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (hit && pos < a.nsample[b]) a.idx[b][(size_t)q * a.nsample[b] + pos] = i;
                if (cnt[b] == 0) first[b] = i0 + (uint32_t)__builtin_ctzll(mask);
                cnt[b] += (uint32_t)__popcll(mask);
                if (cnt[b] >= a.nsample[b]) open &= ~(1u << b);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if ((uint32_t)b >= a.n_radii) continue;
        const uint32_t ns = a.nsample[b], c = cnt[b] > ns ? ns : cnt[b];
        uint32_t* row = a.idx[b] + (size_t)q * ns;
        for (uint32_t p = c + (uint32_t)lane; p < ns; p += 64) row[p] = first[b];      // the first hit, or the segment's size for an empty row
        if (lane == 0) a.counts[b][q] = c;
    }
}

// ---- group: new_points[q][k] = (xyz[idx] - centre | features[idx]) ------------------------------------------------------------------------------
__global__ __launch_bounds__(PN_BLOCK) void group_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                         const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                         const uint32_t* __restrict__ seg_ptr, const uint32_t* __restrict__ centre_seg,
                                                         const uint32_t* __restrict__ idx, const float* __restrict__ feat, uint32_t D, uint32_t nsample,
                                                         unsigned long long total, float* __restrict__ new_xyz, float* __restrict__ new_points)
{
    const unsigned long long e = (unsigned long long)blockIdx.x * PN_BLOCK + threadIdx.x;
    if (e >= total) return;
    const uint32_t C = 3u + D;
    const uint32_t ch = (uint32_t)(e % C);
    const unsigned long long qk = e / C;
    const uint32_t q = (uint32_t)(qk / nsample), k = (uint32_t)(qk % nsample);
    const uint32_t s = centre_seg[q], base = seg_ptr[s];
    const uint32_t p = base + idx[qk];                                        // < seg_ptr[s + 1]: checked by the host
    float v;
    if (ch < 3) {
        const float* pc = ch == 0 ? x : (ch == 1 ? y : z);
        const float* cc = ch == 0 ? qx : (ch == 1 ? qy : qz);
        v = pc[p] - cc[q];
        if (k == 0) new_xyz[(size_t)q * 3 + ch] = cc[q];
    } else {
        v = feat[(size_t)p * D + (ch - 3u)];
    }
    new_points[e] = v;
}

// ---- objects ----------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long pn_splitmix(unsigned long long seed, unsigned long long a)
{
    unsigned long long zz = seed ^ (0x9E3779B97F4A7C15ull * (a + 1ull));
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    return zz ^ (zz >> 31);
}
inline unsigned long long pn_splitmix_host(unsigned long long seed, unsigned long long a)
{
    unsigned long long zz = seed ^ (0x9E3779B97F4A7C15ull * (a + 1ull));
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    return zz ^ (zz >> 31);
}

__global__ __launch_bounds__(PN_BLOCK) void obj_keys_kernel(const int32_t* __restrict__ labels, uint32_t n, uint32_t n_clusters,
                                                            unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t i = blockIdx.x * PN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    keys[i] = l < 0 ? (unsigned long long)n_clusters : (unsigned long long)l;      // noise sorts behind every cluster
    vals[i] = i;
}

__global__ __launch_bounds__(PN_BLOCK) void obj_gather_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              const uint32_t* __restrict__ order, uint32_t n, float* __restrict__ sx,
                                                              float* __restrict__ sy, float* __restrict__ sz)
{
    const uint32_t t = blockIdx.x * PN_BLOCK + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = order[t];
    if (i < n) { sx[t] = x[i]; sy[t] = y[i]; sz[t] = z[i]; }
}

// one workgroup per cluster: zmm[c] = (min z, max z) over its members (fminf / fmaxf: (+inf, -inf) for an empty cluster)
__global__ __launch_bounds__(PN_BLOCK) void obj_zstats_kernel(const float* __restrict__ sz, const uint32_t* __restrict__ seg_ptr, float* __restrict__ zmm)
{
    const uint32_t c = blockIdx.x, b = seg_ptr[c], e = seg_ptr[c + 1];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (uint32_t i = b + threadIdx.x; i < e; i += PN_BLOCK) { lo = fminf(lo, sz[i]); hi = fmaxf(hi, sz[i]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_down(lo, o, 64)); hi = fmaxf(hi, __shfl_down(hi, o, 64)); }
    __shared__ float red[2][PN_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w2 = 1; w2 < PN_BLOCK / 64; w2++) { lo = fminf(lo, red[0][w2]); hi = fmaxf(hi, red[1][w2]); }
        zmm[2 * c] = lo; zmm[2 * c + 1] = hi;
    }
}

struct ObjDesc {
    uint32_t base, n, cluster;
    int32_t fps_row;                    // row of the FPS picks, -1: all members, then padding draws
};

// one workgroup per object: member of every row, its coordinates into LDS, the f64 sum of the rows IN ROW ORDER (one lane per coordinate),
// mean = sum / npoints, out = (float)((double)p - mean)
__global__ __launch_bounds__(PN_BLOCK) void obj_build_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                                                             const uint32_t* __restrict__ order, const ObjDesc* __restrict__ objs,
                                                             const uint32_t* __restrict__ fps_idx, uint32_t npoints, unsigned long long seed,
                                                             float* __restrict__ objects, uint32_t* __restrict__ src_index)
{
    extern __shared__ float pts[];      // [3][npoints]
    __shared__ double mean[3];
    const ObjDesc o = objs[blockIdx.x];
    for (uint32_t t = threadIdx.x; t < npoints; t += PN_BLOCK) {
        uint32_t m;
        if (o.fps_row >= 0) m = fps_idx[(size_t)o.fps_row * npoints + t];
        else if (t < o.n) m = t;
        else m = (uint32_t)(pn_splitmix(seed, ((unsigned long long)(o.cluster + 1u) << 32) | (unsigned long long)(t - o.n + 1u)) % (unsigned long long)o.n);
        if (m >= o.n) m = 0;            // (never: the picks are members)
        pts[t] = sx[o.base + m]; pts[npoints + t] = sy[o.base + m]; pts[2 * npoints + t] = sz[o.base + m];
        src_index[(size_t)blockIdx.x * npoints + t] = order[o.base + m];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (uint32_t t = 0; t < npoints; t++) acc = acc + (double)pts[threadIdx.x * npoints + t];
        mean[threadIdx.x] = acc / (double)npoints;
    }
    __syncthreads();
    float* out = objects + (size_t)blockIdx.x * npoints * 3;
    for (uint32_t e = threadIdx.x; e < npoints * 3; e += PN_BLOCK) {
        const uint32_t t = e / 3, ch = e % 3;
        out[e] = (float)((double)pts[ch * npoints + t] - mean[ch]);
    }
}

inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + PN_BLOCK - 1) / PN_BLOCK)); }
inline unsigned bit_length(unsigned long long v) { unsigned b = 0; while (v) { b++; v >>= 1; } return b; }

// regime of a segment: 1 one wave (<= 256 points), 2 / 3 / 4 one workgroup of 256 x 4 / 1024 x 4 / 1024 x 16 points, 5 one launch per pick
inline int fps_regime(uint32_t n, int at_least)
{
    const int r = n <= 256 ? 1 : n <= 1024 ? 2 : n <= 4096 ? 3 : n <= FPS_SMALL_MAX ? 4 : 5;
    return std::max(r, std::min(at_least, 5));
}

template <bool F64, int T, int P>
void fps_launch_small(pcr_ctx* ctx, const float* x, const float* y, const float* z, const FpsJob* jobs_dev, size_t count, uint32_t npoint, uint32_t* out_dev)
{
    if (count == 0) return;
    ProfScope ps(ctx, "fps_small");
    hipLaunchKernelGGL((fps_small_kernel<F64, T, P>), dim3((unsigned)count), dim3(T), 0, ctx->stream, x, y, z, jobs_dev, npoint, out_dev);
}

// the picks of every job, out_dev[job.out_row][npoint] (device).  Uses ctx->aux; asynchronous on the stream.  regimes (host, optional): per job.
// keep != nullptr: the job tables move into *keep and the call does not synchronise (fps_device)
int fps_run(pcr_ctx* ctx, const float* x, const float* y, const float* z, std::vector<FpsJob> jobs, uint32_t npoint, int mode, uint32_t* out_dev, uint8_t* regimes,
            HostKeep* keep = nullptr)
{
    if (jobs.empty() || npoint == 0) return PCR_OK;
    const int at_least = (int)tune_get(ctx, "fps_regime", 0);
    std::vector<int> reg(jobs.size());
    for (size_t j = 0; j < jobs.size(); j++) {
        reg[j] = fps_regime(jobs[j].n, at_least);
        if (regimes) regimes[j] = (uint8_t)reg[j];
    }
    std::vector<size_t> perm(jobs.size());
    for (size_t j = 0; j < perm.size(); j++) perm[j] = j;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return reg[a] < reg[b]; });
    auto sorted_h = std::make_shared<std::vector<FpsJob>>(jobs.size());
    auto tab_h = std::make_shared<std::vector<FpsLargeSeg>>();
    auto wg_tab_h = std::make_shared<std::vector<uint32_t>>();
    std::vector<FpsJob>& sorted = *sorted_h;
    std::vector<FpsLargeSeg>& tab = *tab_h;
    std::vector<uint32_t>& wg_tab = *wg_tab_h;
    size_t first[7] = { 0, 0, 0, 0, 0, 0, 0 };          // first[r] = first job of regime r in `sorted`
    for (size_t k = 0; k < perm.size(); k++) { sorted[k] = jobs[perm[k]]; first[reg[perm[k]] + 1]++; }
    for (int r = 1; r < 7; r++) first[r] += first[r - 1];
    // the large segments' table
    unsigned long long dist_total = 0;
    for (size_t k = first[5]; k < first[6]; k++) {
        const FpsJob& j = sorted[k];
        FpsLargeSeg t;
        t.base = j.base; t.n = j.n; t.start = j.start; t.out_row = j.out_row;
        t.wg0 = (uint32_t)wg_tab.size();
        t.nwg = std::max<uint32_t>(1u, std::min<uint32_t>(FPS_LARGE_WG_MAX, (j.n + FPS_LARGE_PER_WG - 1) / FPS_LARGE_PER_WG));
        t.dist_off = dist_total;
        dist_total += ((unsigned long long)j.n + 63ull) & ~63ull;
        for (uint32_t w = 0; w < t.nwg; w++) wg_tab.push_back((uint32_t)tab.size());
        tab.push_back(t);
    }
    const size_t dsz = mode == 1 ? 8 : 4;
    FpsJob* jobs_dev;
    FpsLargeSeg* tab_dev;
    uint32_t* wg_dev;
    FpsPart* part[2];
    void* dist_dev;
    Layout L;
    L.add(&jobs_dev, sorted.size());
    L.add(&tab_dev, tab.size());
    L.add(&wg_dev, wg_tab.size());
    L.add(&part[0], wg_tab.size());
    L.add(&part[1], wg_tab.size());
    L.add(&dist_dev, (size_t)dist_total * dsz);
    int rc = bind_aux(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(jobs_dev, sorted.data(), sorted.size() * sizeof(FpsJob), hipMemcpyHostToDevice, ctx->stream));
    if (!tab.empty()) {
        PCR_HIP(ctx, hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(FpsLargeSeg), hipMemcpyHostToDevice, ctx->stream));
        PCR_HIP(ctx, hipMemcpyAsync(wg_dev, wg_tab.data(), wg_tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (keep) {
        keep->held.push_back(sorted_h);
        keep->held.push_back(tab_h);
        keep->held.push_back(wg_tab_h);
    } else {
        PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the host vectors go out of scope with this call
    }
    if (mode == 1) {
        fps_launch_small<true, 64, 4>(ctx, x, y, z, jobs_dev + first[1], first[2] - first[1], npoint, out_dev);
        fps_launch_small<true, 256, 4>(ctx, x, y, z, jobs_dev + first[2], first[3] - first[2], npoint, out_dev);
        fps_launch_small<true, 1024, 4>(ctx, x, y, z, jobs_dev + first[3], first[4] - first[3], npoint, out_dev);
        fps_launch_small<true, 1024, 16>(ctx, x, y, z, jobs_dev + first[4], first[5] - first[4], npoint, out_dev);
    } else {
        fps_launch_small<false, 64, 4>(ctx, x, y, z, jobs_dev + first[1], first[2] - first[1], npoint, out_dev);
        fps_launch_small<false, 256, 4>(ctx, x, y, z, jobs_dev + first[2], first[3] - first[2], npoint, out_dev);
        fps_launch_small<false, 1024, 4>(ctx, x, y, z, jobs_dev + first[3], first[4] - first[3], npoint, out_dev);
        fps_launch_small<false, 1024, 16>(ctx, x, y, z, jobs_dev + first[4], first[5] - first[4], npoint, out_dev);
    }
    if (!tab.empty()) {
        ProfScope ps(ctx, "fps_large");
        for (uint32_t step = 0; step < npoint; step++) {      // launch `step` resolves pick `step` from what launch `step - 1` left in part[(step - 1) & 1]
            if (mode == 1)
                hipLaunchKernelGGL((fps_large_kernel<true>), dim3((unsigned)wg_tab.size()), dim3(PN_BLOCK), 0, ctx->stream, x, y, z, tab_dev, wg_dev,
                                   (double*)dist_dev, part[(step + 1) & 1], part[step & 1], step, npoint, out_dev);
            else
                hipLaunchKernelGGL((fps_large_kernel<false>), dim3((unsigned)wg_tab.size()), dim3(PN_BLOCK), 0, ctx->stream, x, y, z, tab_dev, wg_dev,
                                   (float*)dist_dev, part[(step + 1) & 1], part[step & 1], step, npoint, out_dev);
        }
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// seg_ptr: n_seg + 1 ascending offsets, the last one <= limit
bool seg_ptr_ok(const uint32_t* seg_ptr, size_t n_seg, size_t limit)
{
    for (size_t s = 0; s < n_seg; s++)
        if (seg_ptr[s] > seg_ptr[s + 1]) return false;
    return seg_ptr[n_seg] <= limit;
}

}  // namespace

int fps_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, std::vector<FpsJob> jobs, uint32_t npoint, int mode, uint32_t* out_dev, HostKeep* keep)
{
    if (!keep) return fail(ctx, PCR_ERR_ARG, "fps_device: keep is NULL");
    return fps_run(ctx, x, y, z, std::move(jobs), npoint, mode, out_dev, nullptr, keep);
}

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_fps_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg, size_t npoint, int mode, const uint32_t* start,
                           uint32_t* indices, uint8_t* regime)
{
    if (!ctx || !cloud || !seg_ptr) return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32");
    if (mode != PCR_FPS_F32 && mode != PCR_FPS_F64) return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32: mode must be PCR_FPS_F32 or PCR_FPS_F64");
    if (n_seg > 0x7FFFFFF0ull || npoint > 0x7FFFFFF0ull || cloud->n > 0x7FFFFFF0ull || (n_seg && npoint > 0x7FFFFFF0ull / n_seg))
        return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32: too large");
    if (!seg_ptr_ok(seg_ptr, n_seg, cloud->n)) return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32: seg_ptr must ascend and end inside the cloud");
    if (n_seg == 0 || npoint == 0) return PCR_OK;
    if (!start || !indices) return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32: start / indices is NULL");
    std::vector<FpsJob> jobs(n_seg);
    for (size_t s = 0; s < n_seg; s++) {
        const uint32_t n = seg_ptr[s + 1] - seg_ptr[s];
        if (start[s] >= n) return fail(ctx, PCR_ERR_ARG, "pcr_fps_f32: start outside its segment (an empty segment has no first pick)");
        jobs[s] = { seg_ptr[s], n, start[s], (uint32_t)s };
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t out_bytes = n_seg * npoint * 4;
    int rc = ensure_scratch(ctx, out_bytes);
    if (rc) return rc;
    uint32_t* out_dev = (uint32_t*)ctx->scratch;
    rc = fps_run(ctx, cloud->x(), cloud->y(), cloud->z(), std::move(jobs), (uint32_t)npoint, mode, out_dev, regime);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(indices, out_dev, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    for (size_t s = 0; s < n_seg; s++) {                   // the bound of every pick, checked: a violation is a corrupt run, not an answer
        const uint32_t n = seg_ptr[s + 1] - seg_ptr[s];
        for (size_t k = 0; k < npoint; k++)
            if (indices[s * npoint + k] >= n) return fail(ctx, PCR_ERR_STATE, "pcr_fps_f32: a pick lies outside its segment");
    }
    return PCR_OK;
}

namespace {

// per-centre segment ids from the centres' seg_ptr
std::vector<uint32_t> centre_segments(const uint32_t* centre_seg_ptr, size_t n_seg)
{
    std::vector<uint32_t> cs(centre_seg_ptr[n_seg]);
    for (size_t s = 0; s < n_seg; s++)
        for (uint32_t q = centre_seg_ptr[s]; q < centre_seg_ptr[s + 1]; q++) cs[q] = (uint32_t)s;
    return cs;
}

}  // namespace

int pcr::ball_query_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, const float* qx, const float* qy, const float* qz, const uint32_t* seg_dev,
                           const uint32_t* centre_seg_dev, size_t nq, double radius, size_t nsample, uint32_t* idx_dev, uint32_t* cnt_dev)
{
    if (nq == 0) return PCR_OK;
    const float r2 = (float)(radius * radius);
    {
        ProfScope ps(ctx, "ball_query");
        hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)((nq + PN_BLOCK / 64 - 1) / (PN_BLOCK / 64))), dim3(PN_BLOCK), 0, ctx->stream, x, y, z, qx, qy, qz, seg_dev,
                           centre_seg_dev, (uint32_t)nq, r2, (uint32_t)nsample, idx_dev, cnt_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

extern "C" int pcr_ball_query_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                                  size_t n_seg, double radius, size_t nsample, uint32_t* idx, uint32_t* counts)
{
    if (!ctx || !cloud || !seg_ptr || !centres || !centre_seg_ptr) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32");
    if (!(radius >= 0.0) || std::isinf(radius)) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: radius must be finite and >= 0");
    if (nsample == 0 || nsample > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: nsample must be >= 1");
    if (n_seg > 0x7FFFFFF0ull || cloud->n > 0x7FFFFFF0ull || centres->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: too large");
    if (!seg_ptr_ok(seg_ptr, n_seg, cloud->n) || !seg_ptr_ok(centre_seg_ptr, n_seg, centres->n))
        return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: seg_ptr must ascend and end inside its cloud");
    if (n_seg == 0) return PCR_OK;
    const size_t q0 = centre_seg_ptr[0], nq = centre_seg_ptr[n_seg] - q0;
    if (nq == 0) return PCR_OK;
    if (!idx) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: idx is NULL");
    if (nq > 0x7FFFFFF0ull / nsample) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_f32: too large");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> cs = centre_segments(centre_seg_ptr, n_seg);      // indexed by centre (rows below q0 unused)
    uint32_t *seg_dev, *cs_dev, *idx_dev, *cnt_dev;
    Layout L;
    L.add(&seg_dev, n_seg + 1);
    L.add(&cs_dev, cs.size());
    L.add(&idx_dev, nq * nsample);
    L.add(&cnt_dev, nq);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg_ptr, (n_seg + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(cs_dev, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rc = ball_query_device(ctx, cloud->x(), cloud->y(), cloud->z(), centres->x() + q0, centres->y() + q0, centres->z() + q0, seg_dev, cs_dev + q0, nq, radius, nsample,
                           idx_dev, cnt_dev);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(idx, idx_dev, nq * nsample * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) PCR_HIP(ctx, hipMemcpyAsync(counts, cnt_dev, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

int pcr::ball_query_multi_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, const float* qx, const float* qy, const float* qz,
                                 const uint32_t* seg_dev, const uint32_t* centre_seg_dev, size_t nq, size_t n_radii, const double* radii, const uint32_t* nsamples,
                                 uint32_t* const* idx_dev, uint32_t* const* cnt_dev)
{
    if (nq == 0) return PCR_OK;
    if (n_radii < 1 || n_radii > 4) return fail(ctx, PCR_ERR_ARG, "ball_query_multi_device: 1 ... 4 radii");
    BallMultiArgs a;
    memset(&a, 0, sizeof(a));
    a.n_radii = (uint32_t)n_radii;
    for (size_t b = 0; b < n_radii; b++) {
        a.r2[b] = (float)(radii[b] * radii[b]);
        a.nsample[b] = nsamples[b];
        a.idx[b] = idx_dev[b];
        a.counts[b] = cnt_dev[b];
    }
    {
        ProfScope ps(ctx, "ball_query_multi");
        hipLaunchKernelGGL(ball_query_multi_kernel, dim3((unsigned)((nq + PN_BLOCK / 64 - 1) / (PN_BLOCK / 64))), dim3(PN_BLOCK), 0, ctx->stream, x, y, z, qx, qy, qz,
                           seg_dev, centre_seg_dev, (uint32_t)nq, a);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

extern "C" int pcr_ball_query_multi_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                                        size_t n_seg, size_t n_radii, const double* radii, const size_t* nsamples, uint32_t* idx, uint32_t* counts)
{
    if (!ctx || !cloud || !seg_ptr || !centres || !centre_seg_ptr || !radii || !nsamples) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32");
    if (n_radii < 1 || n_radii > 4) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: n_radii must be 1 ... 4");
    size_t row_total = 0;
    for (size_t b = 0; b < n_radii; b++) {
        if (!(radii[b] >= 0.0) || std::isinf(radii[b])) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: a radius must be finite and >= 0");
        if (nsamples[b] == 0 || nsamples[b] > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: nsample must be >= 1");
        row_total += nsamples[b];
    }
    if (n_seg > 0x7FFFFFF0ull || cloud->n > 0x7FFFFFF0ull || centres->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: too large");
    if (!seg_ptr_ok(seg_ptr, n_seg, cloud->n) || !seg_ptr_ok(centre_seg_ptr, n_seg, centres->n))
        return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: seg_ptr must ascend and end inside its cloud");
    if (n_seg == 0) return PCR_OK;
    const size_t q0 = centre_seg_ptr[0], nq = centre_seg_ptr[n_seg] - q0;
    if (nq == 0) return PCR_OK;
    if (!idx) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: idx is NULL");
    if (nq > 0x7FFFFFF0ull / row_total) return fail(ctx, PCR_ERR_ARG, "pcr_ball_query_multi_f32: too large");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> cs = centre_segments(centre_seg_ptr, n_seg);      // indexed by centre (rows below q0 unused)
    uint32_t *seg_dev, *cs_dev, *idx_dev, *cnt_dev;
    Layout L;
    L.add(&seg_dev, n_seg + 1);
    L.add(&cs_dev, cs.size());
    L.add(&idx_dev, nq * row_total);
    L.add(&cnt_dev, nq * n_radii);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg_ptr, (n_seg + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(cs_dev, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t *ib[4] = { nullptr, nullptr, nullptr, nullptr }, *cb[4] = { nullptr, nullptr, nullptr, nullptr }, ns[4] = { 0, 0, 0, 0 };
    size_t off = 0;
    for (size_t b = 0; b < n_radii; b++) {
        ib[b] = idx_dev + off;
        cb[b] = cnt_dev + b * nq;
        ns[b] = (uint32_t)nsamples[b];
        off += nq * nsamples[b];
    }
    rc = ball_query_multi_device(ctx, cloud->x(), cloud->y(), cloud->z(), centres->x() + q0, centres->y() + q0, centres->z() + q0, seg_dev, cs_dev + q0, nq, n_radii,
                                 radii, ns, ib, cb);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(idx, idx_dev, nq * row_total * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) PCR_HIP(ctx, hipMemcpyAsync(counts, cnt_dev, nq * n_radii * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_group_points_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres, const uint32_t* centre_seg_ptr,
                                    size_t n_seg, const float* features, size_t D, const uint32_t* idx, size_t nsample, float* new_xyz, float* new_points)
{
    if (!ctx || !cloud || !seg_ptr || !centres || !centre_seg_ptr) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32");
    if (nsample == 0 || nsample > 0x7FFFFFF0ull || D > 65536 || (D > 0 && !features)) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: nsample >= 1, D <= 65536, features with D > 0");
    if (n_seg > 0x7FFFFFF0ull || cloud->n > 0x7FFFFFF0ull || centres->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: too large");
    if (!seg_ptr_ok(seg_ptr, n_seg, cloud->n) || !seg_ptr_ok(centre_seg_ptr, n_seg, centres->n))
        return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: seg_ptr must ascend and end inside its cloud");
    if (n_seg == 0) return PCR_OK;
    const size_t q0 = centre_seg_ptr[0], nq = centre_seg_ptr[n_seg] - q0;
    if (nq == 0) return PCR_OK;
    if (!idx || !new_xyz || !new_points) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: idx / new_xyz / new_points is NULL");
    const size_t C = 3 + D;
    if (nq > (1ull << 40) / nsample / C) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: too large");
    std::vector<uint32_t> cs = centre_segments(centre_seg_ptr, n_seg);
    for (size_t q = 0; q < nq; q++) {                       // an empty ball-query row holds the segment's size: the reference's indexing raises there
        const uint32_t sg = cs[q0 + q], n = seg_ptr[sg + 1] - seg_ptr[sg];
        for (size_t k = 0; k < nsample; k++)
            if (idx[q * nsample + k] >= n) return fail(ctx, PCR_ERR_ARG, "pcr_group_points_f32: an index lies outside its segment (an empty ball-query row?)");
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t p0 = seg_ptr[0], np = seg_ptr[n_seg] - p0;
    const size_t total_e = nq * nsample * C;
    uint32_t *seg_dev, *cs_dev, *idx_dev;
    float *feat_dev, *xyz_dev, *out_dev;
    Layout L;
    L.add(&seg_dev, n_seg + 1);
    L.add(&cs_dev, cs.size());
    L.add(&idx_dev, nq * nsample);
    L.add(&feat_dev, np * D);
    L.add(&xyz_dev, nq * 3);
    L.add(&out_dev, total_e);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg_ptr, (n_seg + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(cs_dev, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(idx_dev, idx, nq * nsample * 4, hipMemcpyHostToDevice, ctx->stream));
    if (D && np) PCR_HIP(ctx, hipMemcpyAsync(feat_dev, features + p0 * D, np * D * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    {
        ProfScope ps(ctx, "group_points");
        // features are addressed by cloud position: the pointer is moved back by the p0 rows that were not uploaded (never dereferenced there)
        hipLaunchKernelGGL(group_kernel, blocks_for(total_e), dim3(PN_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), centres->x() + q0,
                           centres->y() + q0, centres->z() + q0, seg_dev, cs_dev + q0, idx_dev, feat_dev - p0 * D, (uint32_t)D, (uint32_t)nsample,
                           (unsigned long long)total_e, xyz_dev, out_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(new_xyz, xyz_dev, nq * 12, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(new_points, out_dev, total_e * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_objects_from_labels_f32(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels, size_t n_clusters, size_t npoints, double ground_z,
                                           double z_min_above_ground, const double z_extent[2], uint64_t seed, const uint32_t* starts, float* objects,
                                           uint32_t* object_cluster, uint32_t* source_index, int32_t* codes, float* z_min_max, uint32_t* sizes,
                                           size_t* n_objects)
{
    if (n_objects) *n_objects = 0;
    if (!ctx || !cloud || !z_extent || !n_objects) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32");
    const size_t n = cloud->n;
    if (n > 0x7FFFFFF0ull || n_clusters > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: too large");
    if (npoints < 1 || npoints > 4096) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: npoints must be in [1, 4096]");
    if (n > 0 && !labels) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: labels is NULL");
    if (std::isnan(ground_z) || std::isnan(z_min_above_ground) || std::isnan(z_extent[0]) || std::isnan(z_extent[1]))
        return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: NaN gate");
    if (n_clusters == 0) return PCR_OK;
    if (!objects || !object_cluster || !codes) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: objects / object_cluster / codes is NULL");
    // ---- segments from the labels (host: one pass), the order from a stable device sort
    std::vector<uint32_t> seg(n_clusters + 2, 0u);      // [c] = first sorted position of cluster c, [n_clusters] = of the noise, [n_clusters + 1] = n
    for (size_t i = 0; i < n; i++) {
        const int32_t l = labels[i];
        if (l < -1 || (l >= 0 && (size_t)l >= n_clusters)) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: a label outside [-1, n_clusters)");
        seg[(l < 0 ? n_clusters : (size_t)l) + 1]++;
    }
    for (size_t c = 0; c + 1 < seg.size(); c++) seg[c + 1] += seg[c];
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    size_t temp_bytes = 0;
    sort_pairs_u64_u32(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, std::max<size_t>(n, 1), 0, 32, ctx->stream);
    int32_t* lab_dev;
    unsigned long long *k_in, *k_out;
    uint32_t *v_in, *order, *seg_dev;
    float *sx, *sy, *sz, *zmm_dev;
    void* sort_temp;
    Layout L;
    L.add(&lab_dev, n);
    L.add(&k_in, n);
    L.add(&k_out, n);
    L.add(&v_in, n);
    L.add(&order, n);
    L.add(&sx, n);
    L.add(&sy, n);
    L.add(&sz, n);
    L.add(&seg_dev, seg.size());
    L.add(&zmm_dev, n_clusters * 2);
    L.add(&sort_temp, temp_bytes);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    std::vector<float> zmm(n_clusters * 2);
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n) {
        PCR_HIP(ctx, hipMemcpyAsync(lab_dev, labels, n * 4, hipMemcpyHostToDevice, ctx->stream));
        ProfScope ps(ctx, "obj_sort");
        hipLaunchKernelGGL(obj_keys_kernel, blocks_for(n), dim3(PN_BLOCK), 0, ctx->stream, lab_dev, (uint32_t)n, (uint32_t)n_clusters, k_in, v_in);
        PCR_HIP(ctx, sort_pairs_u64_u32(sort_temp, temp_bytes, k_in, k_out, v_in, order, n, 0, std::max(1u, bit_length(n_clusters)), ctx->stream));
        hipLaunchKernelGGL(obj_gather_kernel, blocks_for(n), dim3(PN_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), order, (uint32_t)n, sx, sy, sz);
    }
    {
        ProfScope ps(ctx, "obj_zstats");
        hipLaunchKernelGGL(obj_zstats_kernel, dim3((unsigned)n_clusters), dim3(PN_BLOCK), 0, ctx->stream, sz, seg_dev, zmm_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(zmm.data(), zmm_dev, n_clusters * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // ---- gates (f64 on the widened f32 statistics, foreground_obj_cls.py:160-169), the objects in ascending cluster id
    std::vector<ObjDesc> objs;
    std::vector<FpsJob> jobs;
    for (size_t c = 0; c < n_clusters; c++) {
        const uint32_t size = seg[c + 1] - seg[c];
        const double lo = (double)zmm[2 * c], hi = (double)zmm[2 * c + 1];
        int32_t code = -1;
        if (size == 0) code = 3;
        else if (lo - ground_z > z_min_above_ground) code = 3;
        else if ((hi - lo) < z_extent[0] || (hi - lo) > z_extent[1]) code = 3;
        codes[c] = code;
        if (z_min_max) { z_min_max[2 * c] = zmm[2 * c]; z_min_max[2 * c + 1] = zmm[2 * c + 1]; }
        if (sizes) sizes[c] = size;
        if (code != -1) continue;
        ObjDesc o = { seg[c], size, (uint32_t)c, -1 };
        if (size > npoints) {
            uint32_t st;
            if (starts && starts[c] != UINT32_MAX) {
                if (starts[c] >= size) return fail(ctx, PCR_ERR_ARG, "pcr_objects_from_labels_f32: a start outside its cluster");
                st = starts[c];
            } else {
                st = (uint32_t)(pn_splitmix_host(seed, (unsigned long long)(c + 1) << 32) % (unsigned long long)size);
            }
            o.fps_row = (int32_t)jobs.size();
            jobs.push_back({ seg[c], size, st, (uint32_t)jobs.size() });
        }
        object_cluster[objs.size()] = (uint32_t)c;
        objs.push_back(o);
    }
    const size_t n_obj = objs.size();
    if (n_obj == 0) { prof_flush(ctx); return PCR_OK; }
    // ---- FPS (f64 mode) of the large clusters, then one workgroup per object
    ObjDesc* desc_dev;
    uint32_t *fps_dev, *src_dev;
    float* obj_dev;
    Layout L2;
    L2.add(&desc_dev, n_obj);
    L2.add(&fps_dev, jobs.size() * npoints);
    L2.add(&obj_dev, n_obj * npoints * 3);
    L2.add(&src_dev, n_obj * npoints);
    void* b2 = nullptr;
    PCR_HIP(ctx, hipMalloc(&b2, L2.bytes()));
    L2.bind(b2);
    hipError_t e = hipMemcpyAsync(desc_dev, objs.data(), n_obj * sizeof(ObjDesc), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    rc = PCR_OK;
    if (e == hipSuccess && !jobs.empty()) rc = fps_run(ctx, sx, sy, sz, jobs, (uint32_t)npoints, PCR_FPS_F64, fps_dev, nullptr);
    if (e == hipSuccess && rc == PCR_OK) {
        ProfScope ps(ctx, "obj_build");
        hipLaunchKernelGGL(obj_build_kernel, dim3((unsigned)n_obj), dim3(PN_BLOCK), npoints * 12, ctx->stream, sx, sy, sz, order, desc_dev, fps_dev,
                           (uint32_t)npoints, (unsigned long long)seed, obj_dev, src_dev);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(objects, obj_dev, n_obj * npoints * 12, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && source_index) e = hipMemcpyAsync(source_index, src_dev, n_obj * npoints * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    (void)hipFree(b2);
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_objects_from_labels_f32", e != hipSuccess ? e : e2);
    prof_flush(ctx);
    if (source_index)
        for (size_t k = 0; k < n_obj * npoints; k++)
            if (source_index[k] >= n) return fail(ctx, PCR_ERR_STATE, "pcr_objects_from_labels_f32: a source index lies outside the cloud");
    *n_objects = n_obj;
    return PCR_OK;
}
