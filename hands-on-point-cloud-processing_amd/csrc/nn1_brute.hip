// nn1_brute.hip — brute-force 1-NN correspondence for gfx950 (MI355X), LDS-tiled.
//
// Replaces the per-query kd-tree descent of the reference's ICP inner loop
// (Homework9/hw9/src/registration.cpp:925-934 -> nanoflann.hpp:1222,1347) by an exhaustive scan that
// returns the same argmin: A1 arithmetic (nanoflann.hpp:403-406: ((dx*dx + dy*dy) + dz*dz), every op
// rounded to f32, NO fma) and the canonical tie rule "min d2, then lowest index".
//
// Mapping to CDNA4:
//  * one query per lane, QPL queries per lane held in VGPRs for the whole kernel;
//  * targets stream HBM -> registers (coalesced float4 of the SoA arrays) -> LDS tile of TILE points;
//    the next tile's global loads are issued before the current tile is consumed (software pipeline);
//  * every lane reads the same LDS address (ds_read_b128 broadcast: 4 targets per coordinate per read),
//    so LDS traffic is 12 B per 64*QPL pair evaluations and never bank-conflicts;
//    (default transport: the uniform target reads are s_load_dwordx4 through the scalar cache instead of LDS -
//    measured 3-4 % faster; the LDS path stays selectable);
//  * inner loop per CH targets and query: distance arithmetic + a v_min3_u32 tree on the raw bit patterns
//    (d2 >= 0, so IEEE bits are order preserving; NaN bits sort above +inf and never win);
//    TRACK: branch-free - the lane remembers only the running minimum and the FIRST chunk that
//    attained it (v_cmp + v_min + v_cndmask per chunk); the index inside that chunk is resolved once per
//    query after the scan by re-evaluating its CH targets.  Profiling showed why: with scan-ordered
//    targets a divergent "resolve now" branch (the first version of this kernel) is taken by some lane of the
//    wave for a large share of the chunks: +24 % VALU instructions (profiles/r01_tune_nn1_resolve_variants.txt);
//    FTRACK (default, see its kernel): the same tracking on a fused 6-op filter value, winner decided exactly;
//  * the target set is cut into slices (gridDim.y) so that >> 256 workgroups exist even for one scan;
//    slices merge through one 64-bit atomicMin per query on key = d2_bits << 32 | idx, which implements
//    "min d2, then lowest index" exactly and independently of arrival order.
// The kernel is VALU-bound: 9 algorithmic lane-ops per (query, target) pair.
#include "grid_common.hpp"
#include "icp_finish.hpp"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace pcr {

constexpr int NN_BLOCK = 256;
constexpr int NN_TILE = 1024;   // targets per LDS tile: 3 * 4 KiB
constexpr bool NN_F16_DEFAULT = true;      // measured: 0.72 against 0.88 ms per warm 120k x 120k search (profiles/r02_mfma_filter_experiments.txt)
// (the f16 form stages its operands through LDS per workgroup — 0.706 against 0.737 ms per 120k x 120k search — and tracks first / second
// minimum per pair of tiles = chunks of 32 records: both were switches in round 2, both are what the kernel is since round 3)
constexpr int NN_XCD_DEFAULT = 4;          // XCD-aware launch of the matrix-core kernels (tune nn1_xcd; nn1_btrack_kernel): 24.6 against 68.5 MiB fetched per 120k x 120k launch, same time
constexpr bool NN_BF16_DEFAULT = true;     // measured: 0.90 against 1.30 ms per warm 120k x 120k search (profiles/r02_mfma_filter_experiments.txt)

__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c)
{
    return min(min(a, b), c);   // -> v_min3_u32
}

// slice merge: one 64-bit atomicMin implements "min d2, then lowest index" independently of arrival order.  The key only ever
// decreases, so a slice whose result cannot lower what is already published skips the read-modify-write (device-scope atomics
// go to the fabric: at ~60-280 slices per query they were 57-267 MB of write traffic per launch; now only improving slices write).
__device__ __forceinline__ void merge_key(unsigned long long* slot, unsigned long long key)
{
    if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
}

// exact A1 distance as raw bits
__device__ __forceinline__ uint32_t d2_exact_bits(float qx, float qy, float qz, float x, float y, float z)
{
    const float dx = qx - x, dy = qy - y, dz = qz - z;
    return __float_as_uint((dx * dx + dy * dy) + dz * dz);
}

// fused filter value as raw bits (never decides, only gates)
__device__ __forceinline__ uint32_t d2_fused_bits(float qx, float qy, float qz, float x, float y, float z)
{
    const float dx = qx - x, dy = qy - y, dz = qz - z;
    return __float_as_uint(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
}

__device__ __forceinline__ uint32_t gate_bits(uint32_t best_bits)
{
    // best*(1 + 2^-20) + 1e-30, saturating at +inf; with best == FLT_MAX-init this is +inf: accept anything
    const float t = __uint_as_float(best_bits) * 1.00000095367431640625f + 1e-30f;
    return __float_as_uint(t);
}

// branch-free variant: running minimum + first chunk attaining it
template <int QPL, int CH>
struct TrackLane {
    float qx[QPL], qy[QPL], qz[QPL];
    uint32_t best[QPL], bchunk[QPL];

    __device__ __forceinline__ void chunk(const float (&X)[CH], const float (&Y)[CH], const float (&Z)[CH], uint32_t j0)
    {
#pragma unroll
        for (int k = 0; k < QPL; k++) {
            uint32_t d[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) d[j] = d2_exact_bits(qx[k], qy[k], qz[k], X[j], Y[j], Z[j]);
            uint32_t m = umin3(d[0], d[1], d[2]);
#pragma unroll
            for (int j = 3; j + 1 < CH; j += 2) m = umin3(m, d[j], d[j + 1]);
            m = min(m, d[CH - 1]);
            const bool better = m < best[k];          // strict: the FIRST chunk attaining the minimum is kept
            best[k] = min(best[k], m);
            bchunk[k] = better ? j0 : bchunk[k];
        }
    }
};

template <int QPL, int CH>
__global__ __launch_bounds__(NN_BLOCK) void nn1_track_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
    const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
    uint32_t ns, uint32_t n_tiles, uint32_t tiles_per_slice,
    unsigned long long* __restrict__ keys, int merge_atomic, const int* __restrict__ stop)
{
    if (stop && (stop[0] | stop[1])) return;      // pipelined ICP: the loop has ended, the enqueued tail is a no-op
    const uint32_t tid = threadIdx.x;
    const uint32_t qbase = blockIdx.x * (NN_BLOCK * QPL);
    TrackLane<QPL, CH> L;
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        uint32_t i = min(qbase + k * NN_BLOCK + tid, ns - 1);
        L.qx[k] = sx[i]; L.qy[k] = sy[i]; L.qz[k] = sz[i];
        L.best[k] = 0x7F7FFFFFu;        // FLT_MAX: nanoflann.hpp:163; accept only d2 < worst (:1360)
        L.bchunk[k] = 0xFFFFFFFFu;
    }
    const uint32_t tile0 = blockIdx.y * tiles_per_slice;
    const uint32_t tile1 = min(tile0 + tiles_per_slice, n_tiles);
    // the targets are wave-uniform data: s_load_dwordx4 of the SoA arrays through the scalar cache — operands arrive in SGPRs, no LDS,
    // no barriers (round 1 also carried an LDS-tiled transport of the same loop: 3-4 % slower, retired in round 3; since round 2 the
    // LDS-staged kernel of this file is the matrix-core one, nn1_btrack_kernel)
    const uint32_t j_begin = tile0 * NN_TILE, j_end = tile1 * NN_TILE;
#pragma unroll 2
    for (uint32_t j0 = j_begin; j0 < j_end; j0 += CH) {
        float X[CH], Y[CH], Z[CH];
#pragma unroll
        for (int g = 0; g < CH / 4; g++) {
            const float4 a = *reinterpret_cast<const float4*>(tx + j0 + 4 * g);
            const float4 b = *reinterpret_cast<const float4*>(ty + j0 + 4 * g);
            const float4 c = *reinterpret_cast<const float4*>(tz + j0 + 4 * g);
            X[4 * g] = a.x; X[4 * g + 1] = a.y; X[4 * g + 2] = a.z; X[4 * g + 3] = a.w;
            Y[4 * g] = b.x; Y[4 * g + 1] = b.y; Y[4 * g + 2] = b.z; Y[4 * g + 3] = b.w;
            Z[4 * g] = c.x; Z[4 * g + 1] = c.y; Z[4 * g + 2] = c.z; Z[4 * g + 3] = c.w;
        }
        L.chunk(X, Y, Z, j0);
    }
    // once per query: which target of the remembered chunk attained the minimum (lowest index first)
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        const uint32_t i = qbase + k * NN_BLOCK + tid;
        uint32_t bidx = 0xFFFFFFFFu;
        if (L.bchunk[k] != 0xFFFFFFFFu) {
            const uint32_t j0 = L.bchunk[k];
#pragma unroll
            for (int j = CH - 1; j >= 0; j--) {
                const uint32_t e = d2_exact_bits(L.qx[k], L.qy[k], L.qz[k], tx[j0 + j], ty[j0 + j], tz[j0 + j]);
                if (e == L.best[k]) bidx = j0 + j;
            }
        }
        if (i < ns) {
            const uint32_t bits = (bidx == 0xFFFFFFFFu) ? 0x7F800000u : L.best[k];
            const unsigned long long key = ((unsigned long long)bits << 32) | bidx;
            if (merge_atomic) merge_key(&keys[i], key);
            else keys[i] = key;
        }
    }
}

// ---- FTRACK: branch-free tracking on the FUSED filter value (6 instead of 8 distance ops per pair).
// Per query the hot loop keeps a1 = smallest chunk-minimum of a = fma(dz,dz,fma(dy,dy,dx*dx)), c1 = the first chunk
// attaining it, and a2 = the smallest chunk-minimum over all OTHER chunks.  Since |a - d2| <= 7u*d2 (u = 2^-24, all
// terms non-negative), a2 > a1*(1 + 2^-20) + 1e-30 proves that every target outside c1 has an exact d2 strictly
// above the exact minimum of c1: the answer is then decided by evaluating c1's CH targets with the exact unfused
// arithmetic.  If the proof fails for some lane (near-ties between chunks, duplicates, overflow), the wave rescans
// the slice with the exact TRACK loop.  Either way the result is bit-identical to brute force.
template <int QPL, int CH>
__global__ __launch_bounds__(NN_BLOCK) void nn1_ftrack_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
    const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
    uint32_t ns, uint32_t n_tiles, uint32_t tiles_per_slice,
    unsigned long long* __restrict__ keys, int merge_atomic, const int* __restrict__ stop,
    const uint32_t* __restrict__ qlist, const uint32_t* __restrict__ qcount, uint32_t qcap)
{
    if (stop && (stop[0] | stop[1])) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t qbase = blockIdx.x * (NN_BLOCK * QPL);
    // qlist: only the listed queries (the far queries the grid walk handed over, grid.hip); their keys[] already hold a real
    // candidate or "none", and the results are merged into them
    uint32_t nq = ns;
    if (qlist) {
        nq = min(*qcount, qcap);
        if (qbase >= nq) return;
    }
    float qx[QPL], qy[QPL], qz[QPL];
    uint32_t a1[QPL], a2[QPL], c1[QPL], iq[QPL];
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        const uint32_t slot = min(qbase + k * NN_BLOCK + tid, nq - 1);
        const uint32_t i = qlist ? qlist[slot] : slot;
        iq[k] = i;
        qx[k] = sx[i]; qy[k] = sy[i]; qz[k] = sz[i];
        a1[k] = 0x7F800000u; a2[k] = 0x7F800000u; c1[k] = 0xFFFFFFFFu;
    }
    const uint32_t tile0 = blockIdx.y * tiles_per_slice;
    const uint32_t tile1 = min(tile0 + tiles_per_slice, n_tiles);
    const uint32_t j_begin = tile0 * NN_TILE, j_end = tile1 * NN_TILE;
#pragma unroll 2
    for (uint32_t j0 = j_begin; j0 < j_end; j0 += CH) {
        float X[CH], Y[CH], Z[CH];
#pragma unroll
        for (int g = 0; g < CH / 4; g++) {      // wave-uniform addresses: s_load_dwordx4
            const float4 a = *reinterpret_cast<const float4*>(tx + j0 + 4 * g);
            const float4 b = *reinterpret_cast<const float4*>(ty + j0 + 4 * g);
            const float4 c = *reinterpret_cast<const float4*>(tz + j0 + 4 * g);
            X[4 * g] = a.x; X[4 * g + 1] = a.y; X[4 * g + 2] = a.z; X[4 * g + 3] = a.w;
            Y[4 * g] = b.x; Y[4 * g + 1] = b.y; Y[4 * g + 2] = b.z; Y[4 * g + 3] = b.w;
            Z[4 * g] = c.x; Z[4 * g + 1] = c.y; Z[4 * g + 2] = c.z; Z[4 * g + 3] = c.w;
        }
#pragma unroll
        for (int k = 0; k < QPL; k++) {
            uint32_t d[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) d[j] = d2_fused_bits(qx[k], qy[k], qz[k], X[j], Y[j], Z[j]);
            uint32_t m = umin3(d[0], d[1], d[2]);
#pragma unroll
            for (int j = 3; j + 1 < CH; j += 2) m = umin3(m, d[j], d[j + 1]);
            m = min(m, d[CH - 1]);
            a2[k] = min(a2[k], max(a1[k], m));       // smallest chunk-minimum among the chunks that are not c1
            const bool better = m < a1[k];
            a1[k] = min(a1[k], m);
            c1[k] = better ? j0 : c1[k];
        }
    }
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        uint32_t best = 0x7F7FFFFFu, bidx = 0xFFFFFFFFu;      // FLT_MAX gate, nanoflann.hpp:163,1360
        const bool proven = (c1[k] != 0xFFFFFFFFu) && (a2[k] > gate_bits(a1[k]));
        if (__all(proven || j_begin >= j_end)) {
            if (c1[k] != 0xFFFFFFFFu) {
                const uint32_t j0 = c1[k];
#pragma unroll
                for (int j = 0; j < CH; j++) {
                    const uint32_t e = d2_exact_bits(qx[k], qy[k], qz[k], tx[j0 + j], ty[j0 + j], tz[j0 + j]);
                    if (e < best) { best = e; bidx = j0 + j; }
                }
            }
        } else {
            // exact rescan of the slice for this query (the whole wave: lanes that were proven get the same answer)
            uint32_t bchunk = 0xFFFFFFFFu;
            for (uint32_t j0 = j_begin; j0 < j_end; j0 += CH) {
                uint32_t m = 0xFFFFFFFFu;
#pragma unroll
                for (int j = 0; j < CH; j++) m = min(m, d2_exact_bits(qx[k], qy[k], qz[k], tx[j0 + j], ty[j0 + j], tz[j0 + j]));
                const bool better = m < best;
                best = min(best, m);
                bchunk = better ? j0 : bchunk;
            }
            if (bchunk != 0xFFFFFFFFu) {
#pragma unroll
                for (int j = CH - 1; j >= 0; j--) {
                    const uint32_t e = d2_exact_bits(qx[k], qy[k], qz[k], tx[bchunk + j], ty[bchunk + j], tz[bchunk + j]);
                    if (e == best) bidx = bchunk + j;
                }
            }
        }
        if (qbase + k * NN_BLOCK + tid < nq) {
            const uint32_t i = iq[k];
            const uint32_t bits = (bidx == 0xFFFFFFFFu) ? 0x7F800000u : best;
            const unsigned long long key = ((unsigned long long)bits << 32) | bidx;
            if (merge_atomic) merge_key(&keys[i], key);
            else keys[i] = key;
        }
    }
}

// ---- ETRACK: the filter in EXPANDED form on chunk-centred targets: 3 FMAs per pair instead of 3 subtractions + 3 (mul / fma).
// The target is taken in the cell-sorted order of its grid index (grid.hip), 16 consecutive = spatially neighbouring points
// per chunk, stored relative to the chunk centre C:  t'' = fl(t - C) (kept as -2 t'', exact),  w = fl(|t''|^2) (1 - 2^-18)   (Grid::chunks).
// Per (query, chunk):  r = fl(q - C),  R = fl(|r|^2);  per pair  g = fma(rx, -2t''x, fma(ry, -2t''y, fma(rz, -2t''z, w))).
// In real arithmetic |q - t|^2 = |r|^2 + |t''|^2 - 2 r.t''.  With u = 2^-24, Q = |r|^2, W = |t''|^2 (of the float vectors):
//   rounding of g                      <= 3.1 u (2 W + Q)        (three nested FMAs, partial results <= W + 2 |r||t''| <= 2 W + Q)
//   w vs W                             <= 3 u W
//   r, t'' vs the true q - C, t - C    |D - |r - t''|^2| <= 4 u (Q + W)         (D = true squared distance)
//   exact A1 value d2 vs D             d2 >= D (1 - 5 u),  D <= 2 (Q + W)
//   R vs Q, the final fma              <= 3 u Q,  <= 2 u (Q + W)
// Sum: d2 >= Q (1 - 22.1 u) + g_real - 25.2 u W.  The stored w carries (1 - 2^-18) = 1 - 64 u and R is scaled by
// KAPPA = 1 - 2^-19 = 1 - 32 u, so   L = fma(R, KAPPA, g)  <=  d2   for EVERY target (absolute slack 1e-30 for underflow).
// Per query the loop tracks, branch-free, m1 = smallest chunk value min_j L, c1 = the first chunk attaining it, m2 = the smallest
// over all other chunks.  After the scan the 16 targets of c1 are evaluated with the exact A1 arithmetic (original coordinates
// from the grid records) -> (e, index);  m2 - 1e-30 > e  proves that every target outside c1 is strictly farther: the answer is
// exact and canonical.  Otherwise the wave rescans its slice exactly.  Chunk radius ~ 0.2 m keeps the absolute error of L
// around 1e-7 m^2, far below the gap between the nearest and the next candidates of a LiDAR scan.
// Cost per (query, chunk of 16): 3 sub + 3 (mul / fma) for R + 24 v_pk_fma_f32 + 8 v_min3 + fma + med3 + cmp + min + cndmask;
// priced with tools/ubench/valu_rate.hip (min / max / med3 issue at ~0.6 of the add / fma rate): 80.6 ns per wave.
template <int QPL>
__global__ __launch_bounds__(NN_BLOCK) void nn1_etrack_kernel(
    const float* __restrict__ chunks, const float4* __restrict__ records, uint32_t nt, uint32_t n_chunks, uint32_t chunks_per_slice,
    const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
    unsigned long long* __restrict__ keys, int merge_atomic, const int* __restrict__ stop, unsigned long long* __restrict__ stats)
{
    if (stop && (stop[0] | stop[1])) return;
    constexpr int CH = 16;
    constexpr float KAPPA = 0.99999809265136718750f;          // 1 - 2^-19
    const uint32_t tid = threadIdx.x;
    const uint32_t qbase = blockIdx.x * (NN_BLOCK * QPL);
    float qx[QPL], qy[QPL], qz[QPL], m1[QPL], m2[QPL], cur0[QPL];
    uint32_t c1[QPL];
    bool okq[QPL];
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        const uint32_t i = min(qbase + k * NN_BLOCK + tid, ns - 1);
        qx[k] = sx[i]; qy[k] = sy[i]; qz[k] = sz[i];
        okq[k] = fabsf(qx[k]) < 1e18f && fabsf(qy[k]) < 1e18f && fabsf(qz[k]) < 1e18f;      // false for NaN / inf
        m1[k] = INFINITY; m2[k] = INFINITY; c1[k] = 0xFFFFFFFFu;
        // what is published for this query right now (the seed of a warm ICP iteration, or results of slices that already
        // finished): an upper bound of the final answer.  Requested here so that its latency hides behind the scan.
        cur0[k] = merge_atomic ? __uint_as_float((uint32_t)(__atomic_load_n(&keys[i], __ATOMIC_RELAXED) >> 32)) : INFINITY;   // 0xFFFFFFFF = NaN: no claim
    }
    const uint32_t cb = blockIdx.y * chunks_per_slice, ce = min(cb + chunks_per_slice, n_chunks);
    typedef float f2 __attribute__((ext_vector_type(2)));
    for (uint32_t c = cb; c < ce; c++) {
        const float4* __restrict__ p = reinterpret_cast<const float4*>(chunks + (size_t)c * (4 + 4 * CH));   // wave-uniform: scalar loads
        const float4 C = p[0];
        float TX[CH], TY[CH], TZ[CH], WW[CH];
#pragma unroll
        for (int j = 0; j < CH / 4; j++) {
            const float4 a = p[1 + j], b = p[1 + CH / 4 + j], d = p[1 + 2 * (CH / 4) + j], e = p[1 + 3 * (CH / 4) + j];
            TX[4 * j] = a.x; TX[4 * j + 1] = a.y; TX[4 * j + 2] = a.z; TX[4 * j + 3] = a.w;
            TY[4 * j] = b.x; TY[4 * j + 1] = b.y; TY[4 * j + 2] = b.z; TY[4 * j + 3] = b.w;
            TZ[4 * j] = d.x; TZ[4 * j + 1] = d.y; TZ[4 * j + 2] = d.z; TZ[4 * j + 3] = d.w;
            WW[4 * j] = e.x; WW[4 * j + 1] = e.y; WW[4 * j + 2] = e.z; WW[4 * j + 3] = e.w;
        }
#pragma unroll
        for (int k = 0; k < QPL; k++) {
            const float rx = qx[k] - C.x, ry = qy[k] - C.y, rz = qz[k] - C.z;
            const float ax = rx, ay = ry, az = rz;             // the -2 of the cross term is stored with the targets (exact)
            const float R = __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx));
            // two neighbouring targets per instruction: v_pk_fma_f32 with the SGPR pair costs 2.15 ns per wave-instruction against
            // 2 x 1.18 ns for two scalar FMAs (profiles/r01_ubench_valu_rate.txt); the query operand is broadcast by op_sel_hi
            const f2 ax2 = { ax, ax }, ay2 = { ay, ay }, az2 = { az, az };
            float g[CH];
#pragma unroll
            for (int j = 0; j < CH; j += 2) {
                f2 acc = { WW[j], WW[j + 1] };
                acc = __builtin_elementwise_fma(az2, (f2){ TZ[j], TZ[j + 1] }, acc);
                acc = __builtin_elementwise_fma(ay2, (f2){ TY[j], TY[j + 1] }, acc);
                acc = __builtin_elementwise_fma(ax2, (f2){ TX[j], TX[j + 1] }, acc);
                g[j] = acc.x; g[j + 1] = acc.y;
            }
            float m = fminf(fminf(g[0], g[1]), g[2]);
#pragma unroll
            for (int j = 3; j + 1 < CH; j += 2) m = fminf(fminf(m, g[j]), g[j + 1]);
            m = fminf(m, g[CH - 1]);
            const float L = __builtin_fmaf(R, KAPPA, m);
            m2[k] = __builtin_amdgcn_fmed3f(m1[k], m2[k], L);  // second smallest of (m1 <= m2, L): the smallest chunk value outside c1
            const bool better = L < m1[k];
            m1[k] = fminf(m1[k], L);
            c1[k] = better ? c : c1[k];
        }
    }
#pragma unroll
    for (int k = 0; k < QPL; k++) {
        uint32_t best = 0x7F7FFFFFu, bidx = 0xFFFFFFFFu;      // FLT_MAX gate, nanoflann.hpp:163,1360
        bool proven = false;
        // The other slices of this query publish their results through keys[] as they finish.  Whatever is there now is an upper
        // bound of the final answer (the key only ever decreases; a stale read is merely less helpful): a slice whose every
        // target is provably farther than that bound (m1 = min L <= every d2 of the slice) cannot win or tie and is done;
        // likewise "every chunk but c1 is farther than the bound" (m2) settles the slice with c1's exact result alone.
        const float cur = cur0[k];
        const bool slice_out = okq[k] && (m1[k] - 1e-30f) > cur;
        if (!slice_out && okq[k] && c1[k] != 0xFFFFFFFFu) {
            const uint32_t j0 = c1[k] * CH;
#pragma unroll
            for (int j = 0; j < CH; j++) {
                if (j0 + j < nt) {
                    const float4 rec = records[j0 + j];                                  // original coordinates + original index
                    const uint32_t e = d2_exact_bits(qx[k], qy[k], qz[k], rec.x, rec.y, rec.z);
                    const uint32_t oi = __float_as_uint(rec.w);
                    if (e < best || (e == best && e < 0x7F7FFFFFu && oi < bidx)) { best = e; bidx = oi; }
                }
            }
            proven = (bidx != 0xFFFFFFFFu && (m2[k] - 1e-30f) > __uint_as_float(best)) || (m2[k] - 1e-30f) > cur;
        }
        if (!__all(proven || slice_out || cb >= ce)) {
            if (stats && (tid & 63) == 0) atomicAdd(&stats[2], 1ull);          // diagnostics: (wave, query slot) pairs that had to rescan
            // exact rescan of the slice (the whole wave: lanes that were proven get the same answer); the records are not in index
            // order, so the canonical rule needs the lexicographic (d2, index) minimum
            unsigned long long kbest = ~0ull;
            for (uint32_t j = cb * CH; j < min(ce * CH, nt); j++) {
                const float4 rec = records[j];
                const uint32_t e = d2_exact_bits(qx[k], qy[k], qz[k], rec.x, rec.y, rec.z);
                const unsigned long long key = ((unsigned long long)e << 32) | __float_as_uint(rec.w);
                if (e < 0x7F7FFFFFu && key < kbest) kbest = key;
            }
            best = (uint32_t)(kbest >> 32);
            bidx = kbest == ~0ull ? 0xFFFFFFFFu : (uint32_t)(kbest & 0xFFFFFFFFull);
        }
        const uint32_t i = qbase + k * NN_BLOCK + tid;
        if (i < ns) {
            const uint32_t bits = (bidx == 0xFFFFFFFFu) ? 0x7F800000u : best;
            const unsigned long long key = ((unsigned long long)bits << 32) | bidx;
            if (merge_atomic) merge_key(&keys[i], key);
            else keys[i] = key;
        }
    }
}


// ---- BTRACK: the filter on the bf16 matrix pipe (the f32 MFMA was tried twice — it runs at the vector ALU's own FMA rate and the two
// never overlap: DESIGN.md 5, profiles/r02_mfma_filter_experiments.txt).  f32 values are cut into three bf16 pieces each
// (v = v1 + v2 + v3 exactly: 3 x 8 significant bits), so that  r . t'' = sum_{i,j} r_i t''_j  with every product exact in f32;
// v_mfma_f32_32x32x16_bf16 sums 16 such products per instruction.  Per coordinate the 8 K-slots of one lane-half hold the pairs
// (1,1) (1,2) (2,1) (1,3) (2,2) (3,1) (2,3) (3,2); only r3 t''3 (<= 2^-28 |r_c t''_c|) is dropped.  Two instructions = 32 slots:
//   instruction 0: lanes < 32 the x-terms, lanes >= 32 the y-terms;   instruction 1: lanes < 32 the z-terms, lanes >= 32 the three
//   pieces of w against the "coordinate" 1.0 (pieces 1, 0, 0).
// The vector ALU no longer multiplies: per (query, tile) it takes the minimum of 16 accumulators and tracks m1 / m2 / c1; what it does
// per query — r = q - C, R = |r|^2, the split and the packing — is done once per SUPER-TILE of 8 tiles, which share one centre.  That
// needs spatially compact runs of 256 targets: the target is taken in Morton order of its cells (Grid::bt_records).
// Bound.  With Q = |r|^2, W = |t''|^2, u = 2^-24 and G the MFMA result:
//   dropped r3 t''3 terms                                   <= 2 * 2^-28 |r||t''|            <= 0.13 u (Q + W)
//   accumulation of the 32 slots (measured <= 4.1 u sum|a b|, tools/ubench/mfma_filter.hip; taken as 16 u):
//       sum |a b| <= w + 2.1 |r||t''| <= 2.1 (Q + W)                                          <= 34 u (Q + W)
//   r, t'' vs q - C, t - C; exact A1 value vs D; R vs Q; w vs W; the final fma  (as for ETRACK)  <= 4 u + 10 u + 3 u + 3 u + 2 u
//   => d2 >= Q (1 - 56 u) + W (1 - 56 u) - 2 r.t''  >= KAPPA R + G  when  KAPPA = 1 - 2^-17 (128 u) and w = fl(W)(1 - 2^-17):
// L = fma(R, KAPPA, min_j G_j) is a lower bound of every exact distance of the chunk; the decision is ETRACK's (exact evaluation of
// c1, proof by m2, exact rescan otherwise).  A bound that is too LOW only costs time (a rescan); one that were too HIGH could hide the
// true neighbour, so the one assumption no document backs — how the matrix pipe accumulates — is measured on the device under test
// (pcr_selftest_mfma_bf16: 4.1 u of the 16 u assumed, 3.7 u (Q + W) of the 34.2 u assumed for the whole filter value; asserted with
// a factor two of head-room by tests/test_gpu_parity.py), next to the sweeps with adversarial magnitudes and tools/soak_nn1.py.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void bt_pack(float c, uint4& b)
{
    // pieces c1 + c2 + c3 = c (bf16 each, kept in the top halves), K slots [c1, c1, c2, c1, c2, c3, c2, c3]
    const uint32_t a1 = __float_as_uint(c) & 0xFFFF0000u;
    const float d = c - __uint_as_float(a1);
    const uint32_t a2 = __float_as_uint(d) & 0xFFFF0000u;
    const uint32_t a3 = __float_as_uint(d - __uint_as_float(a2));
    const uint32_t s2 = a2 >> 16;
    b.x = (a1 >> 16) | a1;
    b.y = s2 | a1;
    b.z = s2 | (a3 & 0xFFFF0000u);
    b.w = b.z;
}

// F16 (HTRACK): the same filter from ONE v_mfma_f32_32x32x16_f16 per tile.  An f16 carries 11 significant bits, so two pieces hold
// 22 of an f32's 24 (remainder <= 2^-21 |v|), the four piece products per coordinate + two pieces of w fill 14 of the 16 K-slots,
// and every product is exact in f32.  f16 has a narrow exponent range: the super-tile's coordinates are scaled by a power of two
// (centres[].w: |t''| scale <= 2^7, so w <= 3 * 2^14 fits) and the query offset is CLAMPED to +-32000 per coordinate after scaling —
// moving r towards the box that holds every t'' can only shorten |r - t''|, so the bound stays a lower bound (far tiles get a weaker
// one, still far above anything near).  Error budget (u = 2^-24, scaled units): a two-piece f16 value misses < 2^-20 of itself, so the
// cross term 2 r.t'' is off by <= 2 (2^-20 + 2^-20) |r||t''| <= 32 u (Q + W) and w by 16 u W; accumulation taken as 16 u sum|a b| <=
// 34 u (Q + W); the ETRACK terms 22 u (Q + W): 104 u of the 128 u that KAPPA and w carry.  Measured on the device
// (pcr_selftest_mfma_f16): accumulation 4.4 u, the whole filter value 10.4 u (Q + W) of the 82 u budgeted for it.
// f16 UNDERFLOW (round 3): "misses < 2^-20 of itself" only holds while the second piece is a normal f16.  For a scaled value below
// 2^-4 the remainder falls into f16's subnormal range (spacing 2^-24) or below it, so in general
//     |v - v1 - v2| <= 2^-20 |v| + u [|v| < 2^-4],
// and the cross term of coordinate c (a = -2 t''_c, |a| <= 2^8; b = r_c) picks up an ABSOLUTE error u (|a| [|b| < 2^-4] + |b| [|a| < 2^-4])
// that does not shrink with (Q + W) the way the 128 u (Q + W) of slack does.  Of it, u |a| is covered by the 24 u (Q + W) the budget
// leaves unused as soon as |a| >= 1/6 (W >= a^2 / 4), u |b| as soon as |b| >= 1/24; what is not covered is below u / 6 per
// coordinate, u / 2 in all (w's pieces are rounded toward zero: they can only lower the bound).  ht_setup therefore takes 2^-22 = 4 u
// (scaled units) off R: eight times what is needed, one fma per (query, super-tile), nothing in the tile loop; where it matters
// (Q + W < 1/48) R is small enough for the subtraction to be exact to 2^-29.  The self-test measures this regime on the device too
// (worst[2]: |r|, |t''| both in 2^-20 .. 2^-3, subnormal pieces; <= 2 u asserted): an MFMA that FLUSHED f16 subnormals would show
// up there as ~2^-14-sized errors and fail the verdict (mfma_verdict below).

// (ht_pair, ht_setup: grid_common.hpp — the tile search of grid.hip builds the same operands)

// waves per SIMD the headline instance (four query groups, f16, LDS-staged) is built for: 5 = at most 96 VGPRs (two spilled outside the
// tile loop) — measured 0.574 (130 VGPRs, unbounded) / 0.559 (4 waves, 128) / 0.551 ms (5 waves) per 120 k x 120 k search
#ifndef PCR_BT_WAVES
#define PCR_BT_WAVES 5
#endif
template <int QG, bool F16>
__global__ __launch_bounds__(NN_BLOCK, (F16 && QG == 4) ? PCR_BT_WAVES : 1) void nn1_btrack_kernel(
    const float4* __restrict__ centres, const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_super,
    uint32_t supers_per_slice, const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
    unsigned long long* __restrict__ keys, int merge_atomic, const int* __restrict__ stop, unsigned long long* __restrict__ stats,
    uint32_t xq, uint32_t qblocks, uint32_t slices)
{
    const int stopv = stop ? (stop[0] | stop[1]) : 0;         // requested here, tested after the query loads are on their way
    constexpr int CH = 16, TPS = BT_SUPER / 32;
    constexpr float KAPPA = 0.99999237060546875f;             // 1 - 2^-17
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = lane & 31;
    const bool h = lane >= 32;
    // (query block, slice) of this workgroup.  xq = 0: the plain 2-D launch — workgroups go to the 8 XCDs round-robin, so every XCD's
    // L2 pulls in ALL operands and ALL queries.  xq = 1 / 2 / 4: a 1-D launch in which XCD k = id % 8 owns the query blocks = k % xq
    // (mod xq) and the slices = k / xq (mod 8 / xq): its L2 holds 1 / xq of the queries and xq / 8 of the operands.
    // The f16 form stages its operands through LDS: the four waves of a workgroup scan the SAME tiles for different queries; instead of
    // four per-wave streams of 16-byte loads from L1 / L2, the workgroup holds the operands of one super-tile (8 KB) in LDS, the next
    // one prefetched into registers a whole super-tile ahead, one barrier per super-tile (a wave beyond the queries then stays for the
    // barriers: it repeats the last query and stores nothing).  The bf16 form (two MFMAs per tile, 16 KB per super-tile) measured the
    // same either way and keeps the per-wave loads.  (Round 2 carried both transports for both forms as template / tune switches.)
    constexpr bool lds = F16;
    constexpr bool PAIR = F16;                                // chunks of 32 records (two tiles), see the f16 loop
    uint32_t qb = blockIdx.x, sl = blockIdx.y;
    if (xq) {
        const uint32_t k = blockIdx.x & 7u, j = blockIdx.x >> 3, xs = 8u / xq, qb_per = (qblocks + xq - 1) / xq;
        qb = (j % qb_per) * xq + k % xq;
        sl = (j / qb_per) * xs + k / xq;
        if (qb >= qblocks || sl >= slices) return;             // (the padding of an uneven split: block-uniform)
    }
    const uint32_t qbase = (qb * (NN_BLOCK / 64) + wave) * (32 * QG);
    if (qbase >= ns && !lds) return;                          // a whole wave beyond the queries (wave-uniform)
    float qx[QG], qy[QG], qz[QG], m1[QG], m2[QG], cur0[QG];
    uint32_t c1[QG];
    bool okq[QG];
#pragma unroll
    for (int g = 0; g < QG; g++) {
        const uint32_t i = min(qbase + g * 32 + n, ns - 1);
        qx[g] = sx[i]; qy[g] = sy[i]; qz[g] = sz[i];
        okq[g] = fabsf(qx[g]) < 1e18f && fabsf(qy[g]) < 1e18f && fabsf(qz[g]) < 1e18f;      // false for NaN / inf
        m1[g] = INFINITY; m2[g] = INFINITY; c1[g] = 0xFFFFFFFFu;
        cur0[g] = merge_atomic ? __uint_as_float((uint32_t)(__atomic_load_n(&keys[i], __ATOMIC_RELAXED) >> 32)) : INFINITY;
    }
    if (stopv) return;
    // diagnostics launch (tune grid_stats): shader-clock and real-time stamps around the workgroup's work — the clock the chip holds
    // under THIS kernel's load = sum of shader cycles / sum of 100 MHz ticks (bench.py: the clock-corrected roofline)
    unsigned long long clk0 = 0, rt0 = 0;
    if (stats) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    const uint32_t sb = sl * supers_per_slice, se = min(sb + supers_per_slice, n_super);
    float big;
    asm volatile("v_mov_b32 %0, 0x7f800000" : "=v"(big));      // +inf the optimiser cannot see through
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    if (F16) {
        __shared__ uint4 sA[2][TPS * 64];                     // the operands of two super-tiles: 16 KB
        uint4 pre0 = make_uint4(0, 0, 0, 0), pre1 = pre0;
        if (sb < se) {
            sA[0][threadIdx.x] = ops[(size_t)sb * TPS * 64 + threadIdx.x];
            sA[0][NN_BLOCK + threadIdx.x] = ops[(size_t)sb * TPS * 64 + NN_BLOCK + threadIdx.x];
        }
        __syncthreads();
        for (uint32_t S = sb; S < se; S++) {
            const uint32_t buf = (S - sb) & 1u;
            if (S + 1 < se) {                                 // the next super-tile: in flight during this one's eight tiles
                pre0 = ops[(size_t)(S + 1) * TPS * 64 + threadIdx.x];
                pre1 = ops[(size_t)(S + 1) * TPS * 64 + NN_BLOCK + threadIdx.x];
            }
            const float4 C = centres[S];                      // wave-uniform: scalar load; .w = the super-tile's scale (a power of two)
            float inv2 = 0.0f;
            uint4 bq[QG];
            float R[QG];
#pragma unroll
            for (int g = 0; g < QG; g++) ht_setup(qx[g], qy[g], qz[g], C, h, bq[g], R[g], inv2);
            // chunks of 32: the minimum chain of a lane runs on through the two tiles of a pair (the second tile's chain starts from the
            // first tile's minimum), and first / second minimum and the winning chunk are tracked once per PAIR — 3 of the 22 vector
            // issue slots of a tile less.  Chunk 2 P + h = the records of half-lane h in tiles 2 P and 2 P + 1 (two runs of 16).
            static_assert(TPS % 2 == 0, "pairs of tiles must not straddle super-tiles");
#pragma unroll 1
            for (int tp = 0; tp < TPS / 2; tp++) {
                const uint32_t Pr = (S * TPS) / 2 + tp;
                const uint4 A0 = sA[buf][(2 * tp) * 64 + lane], A1 = sA[buf][(2 * tp + 1) * 64 + lane];
                const uint32_t c = 2 * Pr + (h ? 1u : 0u);
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    // minimum of the accumulators: v_min3 chains starting from an opaque +inf (a plain two-operand fminf of two MFMA
                    // results is first canonicalised: three half-rate instructions instead of one).  (No inline-asm v_min3 on the
                    // accumulators themselves: the compiler would not know to wait for the MFMA before it — measured: wrong minima.)
                    const f32x16 acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A0), __builtin_bit_cast(f16x8, bq[g]), zero, 0, 0, 0);
                    float m = big;
#pragma unroll
                    for (int j = 0; j + 1 < CH; j += 2) m = fminf(fminf(m, acc0[j]), acc0[j + 1]);
                    const f32x16 acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A1), __builtin_bit_cast(f16x8, bq[g]), zero, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j + 1 < CH; j += 2) m = fminf(fminf(m, acc1[j]), acc1[j + 1]);
                    const float L = __builtin_fmaf(m, inv2, R[g]);
                    m2[g] = __builtin_amdgcn_fmed3f(m1[g], m2[g], L);
                    const bool better = L < m1[g];            // (false for a NaN L: a non-finite query is rescanned exactly anyway)
                    m1[g] = better ? L : m1[g];
                    c1[g] = better ? c : c1[g];
                }
            }
            if (S + 1 < se) { sA[buf ^ 1u][threadIdx.x] = pre0; sA[buf ^ 1u][NN_BLOCK + threadIdx.x] = pre1; }
            __syncthreads();
        }
    } else {
        uint4 a0n = make_uint4(0, 0, 0, 0), a1n = a0n;
        if (sb < se) { a0n = ops[(size_t)sb * TPS * 128 + lane]; a1n = ops[(size_t)sb * TPS * 128 + 64 + lane]; }
        for (uint32_t S = sb; S < se; S++) {
            const float4 C = centres[S];                      // wave-uniform: scalar load
            uint4 b0[QG], b1[QG];
            float R[QG];
#pragma unroll
            for (int g = 0; g < QG; g++) {
                const float rx = qx[g] - C.x, ry = qy[g] - C.y, rz = qz[g] - C.z;
                R[g] = __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx));
                bt_pack(h ? ry : rx, b0[g]);
                bt_pack(h ? 1.0f : rz, b1[g]);
            }
#pragma unroll 1
            for (int tt = 0; tt < TPS; tt++) {                // (not unrolled: the scheduler would keep all 16 accumulator tiles alive)
                const uint32_t T = S * TPS + tt;
                const uint4 A0 = a0n, A1 = a1n;
                if (tt + 1 < TPS || S + 1 < se) { a0n = ops[(size_t)(T + 1) * 128 + lane]; a1n = ops[(size_t)(T + 1) * 128 + 64 + lane]; }   // next tile in flight
                const uint32_t c = 2 * T + (h ? 1u : 0u);
                // (Tried: reducing the PREVIOUS group's accumulators between the two MFMAs of the current one, in program order enforced with
                // sched_group_barrier — 0.892 against 0.900 ms.  On this chip the bf16 MFMA and the vector instructions of one SIMD's waves
                // take turns rather than overlap in this loop: tools/ubench/mfma_filter.hip part C, profiles/r02_mfma_filter_experiments.txt.)
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A0), __builtin_bit_cast(bf16x8, b0[g]), zero, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1), __builtin_bit_cast(bf16x8, b1[g]), acc, 0, 0, 0);
                    float m = big;
#pragma unroll
                    for (int j = 0; j + 1 < CH; j += 2) m = fminf(fminf(m, acc[j]), acc[j + 1]);
                    const float L = __builtin_fmaf(R[g], KAPPA, m);
                    m2[g] = __builtin_amdgcn_fmed3f(m1[g], m2[g], L);
                    const bool better = L < m1[g];
                    m1[g] = better ? L : m1[g];
                    c1[g] = better ? c : c1[g];
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < QG; g++) {
        // the two half-lanes of a query: smallest chunk value, a chunk attaining it, smallest value over all OTHER chunks
        const float m1o = __shfl_xor(m1[g], 32, 64), m2o = __shfl_xor(m2[g], 32, 64);
        const uint32_t c1o = (uint32_t)__shfl_xor((int)c1[g], 32, 64);
        const bool take = m1o < m1[g] || (m1o == m1[g] && c1o < c1[g]);
        const float M1 = take ? m1o : m1[g];
        const float M2 = fminf(fminf(m2[g], m2o), take ? m1[g] : m1o);
        const uint32_t C1 = take ? c1o : c1[g];
        uint32_t best = 0x7F7FFFFFu, bidx = 0xFFFFFFFFu;      // FLT_MAX gate, nanoflann.hpp:163,1360
        bool proven = false;
        const float cur = cur0[g];                            // see nn1_etrack_kernel: what the other slices have published
        const bool slice_out = okq[g] && (M1 - 1e-30f) > cur;
        if (!slice_out && okq[g] && C1 != 0xFFFFFFFFu) {
            // exact A1 evaluation of the records of chunk C1, split over the two half-lanes, merged lexicographically (d2, index):
            // 16 records = 8 each; a pair chunk (PAIR) = the winner's half-lane run of 16 in each of its two tiles, one run each
            const uint32_t j0 = PAIR ? (4u * (C1 >> 1) + (C1 & 1u) + (h ? 2u : 0u)) * CH : C1 * CH + (h ? 8u : 0u);
#pragma unroll
            for (int j = 0; j < (PAIR ? CH : CH / 2); j++) {
                const float4 rec = records[j0 + j];                                     // (padding records: x = +inf, never accepted)
                const uint32_t e = d2_exact_bits(qx[g], qy[g], qz[g], rec.x, rec.y, rec.z);
                const uint32_t oi = __float_as_uint(rec.w);
                if (e < best || (e == best && e < 0x7F7FFFFFu && oi < bidx)) { best = e; bidx = oi; }
            }
            const uint32_t bo = (uint32_t)__shfl_xor((int)best, 32, 64), io = (uint32_t)__shfl_xor((int)bidx, 32, 64);
            if (bo < best || (bo == best && io < bidx)) { best = bo; bidx = io; }
            proven = (bidx != 0xFFFFFFFFu && (M2 - 1e-30f) > __uint_as_float(best)) || (M2 - 1e-30f) > cur;
        }
        const bool unsettled = !__all(proven || slice_out || sb >= se);
        if (F16 && unsettled && __all(okq[g])) {
            // Some query of this group could not be settled by its best chunk alone: another chunk's bound lies at or below the exact
            // distance found (or nothing was found).  The slice is FILTERED again for this group — one MFMA per tile as in the main
            // pass, operands straight from memory — and every chunk whose bound does not exceed the query's threshold (the exact best so
            // far, or what the other slices have published) is evaluated exactly by its half-lane; a record at or below the threshold
            // can only sit in such a chunk, and the threshold only falls.  A tenth of the whole-slice exact rescan this replaces (which
            // cost 9 % of a warm 120 k x 120 k launch and tied the slice length to three super-tiles).
            if (stats && lane == 0) atomicAdd(&stats[2], 1ull);
            const bool active = !(proven || slice_out);
            float thr = active ? fminf(bidx != 0xFFFFFFFFu ? __uint_as_float(best) : INFINITY, cur) : -INFINITY;
            for (uint32_t S = sb; S < se; S++) {
                const float4 C = centres[S];
                // A super-tile none of whose records can lie within the threshold of any unsettled query of the group is not filtered again
                // (its pairs WERE evaluated by the main pass): every record lies within 128 / scale of the centre in each coordinate
                // (bt_centres_kernel), so |q - t| >= |q - C| - sqrt(3) 128 / scale.
                {
                    const float dx = qx[g] - C.x, dy = qy[g] - C.y, dz = qz[g] - C.z;
                    const float gap = sqrtf((dx * dx + dy * dy) + dz * dz) * 0.99999f - (221.7026f / C.w) * 1.00001f;
                    const bool cannot = !active || (gap > 0.0f && gap * gap * 0.99999f > thr);        // (false for NaN: scanned)
                    if (__all(cannot)) continue;
                }
                uint4 bqg;
                float Rg, inv2;
                ht_setup(qx[g], qy[g], qz[g], C, h, bqg, Rg, inv2);
#pragma unroll 1
                for (int tt = 0; tt < TPS; tt++) {
                    const uint32_t T = S * TPS + tt;
                    const uint4 A = ops[(size_t)T * 64 + lane];
                    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, bqg), zero, 0, 0, 0);
                    float m = big;
#pragma unroll
                    for (int j = 0; j + 1 < CH; j += 2) m = fminf(fminf(m, acc[j]), acc[j + 1]);
                    const float L = __builtin_fmaf(m, inv2, Rg);
                    if (!((L - 1e-30f) > thr)) {                     // (also taken for a NaN bound: evaluating a chunk is always safe)
                        const uint32_t j0 = (2 * T + (h ? 1u : 0u)) * CH;
#pragma unroll
                        for (int j = 0; j < CH; j++) {
                            const float4 rec = records[j0 + j];
                            const uint32_t e = d2_exact_bits(qx[g], qy[g], qz[g], rec.x, rec.y, rec.z);
                            const uint32_t oi = __float_as_uint(rec.w);
                            if (e < best || (e == best && e < 0x7F7FFFFFu && oi < bidx)) { best = e; bidx = oi; }
                        }
                        if (bidx != 0xFFFFFFFFu) thr = fminf(thr, __uint_as_float(best));
                    }
                }
            }
            const uint32_t bo = (uint32_t)__shfl_xor((int)best, 32, 64), io = (uint32_t)__shfl_xor((int)bidx, 32, 64);
            if (bo < best || (bo == best && io < bidx)) { best = bo; bidx = io; }
        } else if (!F16 && unsettled && __all(okq[g])) {
            // the same for the bf16 form: two MFMAs per tile, operands of three pieces, bound = fma(|r|^2, KAPPA, min)
            if (stats && lane == 0) atomicAdd(&stats[2], 1ull);
            const bool active = !(proven || slice_out);
            float thr = active ? fminf(bidx != 0xFFFFFFFFu ? __uint_as_float(best) : INFINITY, cur) : -INFINITY;
            for (uint32_t S = sb; S < se; S++) {
                const float4 C = centres[S];
                const float rx = qx[g] - C.x, ry = qy[g] - C.y, rz = qz[g] - C.z;
                const float Rg = __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx));
                uint4 b0g, b1g;
                bt_pack(h ? ry : rx, b0g);
                bt_pack(h ? 1.0f : rz, b1g);
#pragma unroll 1
                for (int tt = 0; tt < TPS; tt++) {
                    const uint32_t T = S * TPS + tt;
                    const uint4 A0 = ops[(size_t)T * 128 + lane], A1 = ops[(size_t)T * 128 + 64 + lane];
                    f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A0), __builtin_bit_cast(bf16x8, b0g), zero, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1), __builtin_bit_cast(bf16x8, b1g), acc, 0, 0, 0);
                    float m = big;
#pragma unroll
                    for (int j = 0; j + 1 < CH; j += 2) m = fminf(fminf(m, acc[j]), acc[j + 1]);
                    const float L = __builtin_fmaf(Rg, KAPPA, m);
                    if (!((L - 1e-30f) > thr)) {
                        const uint32_t j0 = (2 * T + (h ? 1u : 0u)) * CH;
#pragma unroll 4
                        for (int j = 0; j < CH; j++) {
                            const float4 rec = records[j0 + j];
                            const uint32_t e = d2_exact_bits(qx[g], qy[g], qz[g], rec.x, rec.y, rec.z);
                            const uint32_t oi = __float_as_uint(rec.w);
                            if (e < best || (e == best && e < 0x7F7FFFFFu && oi < bidx)) { best = e; bidx = oi; }
                        }
                        if (bidx != 0xFFFFFFFFu) thr = fminf(thr, __uint_as_float(best));
                    }
                }
            }
            const uint32_t bo = (uint32_t)__shfl_xor((int)best, 32, 64), io = (uint32_t)__shfl_xor((int)bidx, 32, 64);
            if (bo < best || (bo == best && io < bidx)) { best = bo; bidx = io; }
        } else if (unsettled) {
            if (stats && lane == 0) atomicAdd(&stats[2], 1ull);          // diagnostics: (wave, query group) pairs that had to rescan
            // exact rescan of the slice by the whole wave, each half-lane one half of it (non-finite queries)
            const uint32_t r0 = sb * BT_SUPER, r1 = min(se * BT_SUPER, n_rec), mid = r0 + (r1 - r0) / 2;
            unsigned long long kbest = ~0ull;
            for (uint32_t j = h ? mid : r0; j < (h ? r1 : mid); j++) {
                const float4 rec = records[j];
                const uint32_t e = d2_exact_bits(qx[g], qy[g], qz[g], rec.x, rec.y, rec.z);
                const unsigned long long key = ((unsigned long long)e << 32) | __float_as_uint(rec.w);
                if (e < 0x7F7FFFFFu && key < kbest) kbest = key;
            }
            const unsigned long long ko = key_xor32(kbest);
            kbest = ko < kbest ? ko : kbest;
            best = (uint32_t)(kbest >> 32);
            bidx = kbest == ~0ull ? 0xFFFFFFFFu : (uint32_t)(kbest & 0xFFFFFFFFull);
        }
        const uint32_t i = qbase + g * 32 + n;
        if (!h && i < ns) {
            const uint32_t bits = (bidx == 0xFFFFFFFFu) ? 0x7F800000u : best;
            const unsigned long long key = ((unsigned long long)bits << 32) | bidx;
            if (merge_atomic) merge_key(&keys[i], key);
            else keys[i] = key;
        }
    }
    if (stats && threadIdx.x == 0) {
        atomicAdd(&stats[4], (unsigned long long)__builtin_amdgcn_s_memtime() - clk0);
        atomicAdd(&stats[5], (unsigned long long)__builtin_amdgcn_s_memrealtime() - rt0);
    }
}

// ---- STRACK: the SIGN form of the f16 filter (round 3, second session).  HTRACK's launch is vector time plus matrix time: per 32 x 32
// pairs one MFMA (32 cycles) and ~22 vector instructions, eight of them half-rate v_min3 — the vector side is the larger share and the
// two pipes take turns.  Every search this kernel serves starts from a genuine candidate per query (keys[]: the previous correspondence
// re-evaluated by the move / nn1_seed_kernel, or bt_seed_kernel's for a cold search), so the question per pair is not "what is the
// minimum" but "can this record matter": with the query's threshold folded into the two free K-slots the accumulator is
// bound - threshold and its sign bit answers (st_setup / st_theta, grid_common.hpp: error analysis there).  Per (query group, tile)
// the vector ALU ORs 16 accumulators (8 v_or3_b32 — half-rate like v_min3, it turned out: what is saved is the tracking) and the wave
// tests ONE word per tile; no minimum, no chunk tracking, no second pass.  A set sign = "the 16 records of this half-lane's chunk may
// hold one at or below the query's threshold": the lane notes (chunk, query) in a wave-private LDS list and the scan goes on; when the
// list holds nn1_sign_flush entries at the end of a super-tile, when it is full, and at the end of the slice the wave evaluates the
// listed chunks TOGETHER — 16 lanes per chunk, one record each, one coalesced 256-byte load, A1 arithmetic, canonical (d2, index)
// minimum by DPP and a 64-bit LDS minimum per query — and the queries' thresholds fall to what was found before the next super-tile's
// operands are built.  Where nn1_sign_dense or more columns of a group flag the SAME tile (sorted queries behind coarse seeds) the
// flagged half-lanes evaluate their chunk in place instead (uniform addresses per half: broadcast loads).  (First form: every flagged
// lane evaluated its 16 records itself at once, one dependent load after the other, the other 63 lanes waiting — one such visit per
// query and slice-with-a-candidate: 0.59 ms against HTRACK's 0.50.)
// Same keys bit for bit: a record at or below a query's final answer always raises its flag, the exact evaluation decides
// (pcr_selftest_sign_f16 checks the first half of that sentence on the device, the parity suite the whole).
#ifndef PCR_ST_WAVES
#define PCR_ST_WAVES 4
#endif
#ifndef PCR_ST_UNROLL
#define PCR_ST_UNROLL 2
#endif
constexpr int ST_CAP = 128;                                   // entries of a wave's list
template <int QG>
struct StWaveLds {
    float4 q[QG * 32];                                        // the wave's queries (the evaluating lanes are not the owning ones)
    unsigned long long best[QG * 32];                         // (d2 bits << 32 | index) found so far, ~0 = nothing
    uint32_t list[ST_CAP];                                    // (chunk relative to the slice << 7) | query slot
};

// the listed chunks against their queries: 16 lanes per chunk, four chunks per wave-instruction
template <int QG>
__device__ __forceinline__ void st_flush(StWaveLds<QG>& L, uint32_t cnt, uint32_t chunk0, const float4* __restrict__ records, uint32_t lane)
{
#ifdef PCR_ST_TIMING_NOFLUSH                                  // (timing builds only: what the joint evaluations cost — wrong answers)
    return;
#endif
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (uint32_t e0 = 0; e0 < cnt; e0 += 8) {                 // eight chunks per round: both record loads of a lane are in flight together
        bool valid[2];
        uint32_t slot[2];
        float4 q[2], rec[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t e = e0 + 4u * u + (lane >> 4);
            valid[u] = e < cnt;
            const uint32_t ent = L.list[valid[u] ? e : 0];
            slot[u] = ent & 127u;
            q[u] = L.q[slot[u]];
            rec[u] = records[(size_t)(chunk0 + (ent >> 7)) * 16 + (lane & 15)];          // (padding records: x = +inf, never accepted)
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t d = d2_exact_bits(q[u].x, q[u].y, q[u].z, rec[u].x, rec[u].y, rec[u].z);
            unsigned long long key = (valid[u] && d < 0x7F7FFFFFu) ? (((unsigned long long)d << 32) | __float_as_uint(rec[u].w)) : ~0ull;   // FLT_MAX gate
            key = key_min_dpp<0xB1>(key); key = key_min_dpp<0x4E>(key);                       // quad xor 1, xor 2,
            key = key_min_dpp<0x141>(key); key = key_min_dpp<0x140>(key);                     // half-row mirror, row mirror
            if ((lane & 15) == 0 && key != ~0ull) atomicMin(&L.best[slot[u]], key);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <int QG>
__global__ __launch_bounds__(NN_BLOCK, PCR_ST_WAVES) void nn1_strack_kernel(
    const float4* __restrict__ centres, const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_super,
    uint32_t supers_per_slice, const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
    unsigned long long* __restrict__ keys, const int* __restrict__ stop, unsigned long long* __restrict__ stats,
    uint32_t xq, uint32_t qblocks, uint32_t slices, uint32_t flush_at, uint32_t dense_at)
{
    const int stopv = stop ? (stop[0] | stop[1]) : 0;
    constexpr int TPS = BT_SUPER / 32;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = lane & 31;
    const bool h = lane >= 32;
    uint32_t qb = blockIdx.x, sl = blockIdx.y;                // (query block, slice): as nn1_btrack_kernel
    if (xq) {
        const uint32_t k = blockIdx.x & 7u, j = blockIdx.x >> 3, xs = 8u / xq, qb_per = (qblocks + xq - 1) / xq;
        qb = (j % qb_per) * xq + k % xq;
        sl = (j / qb_per) * xs + k / xq;
        if (qb >= qblocks || sl >= slices) return;
    }
    __shared__ uint4 sA[2][TPS * 64];                         // the operands of two super-tiles: 16 KB
    __shared__ StWaveLds<QG> lds_all[NN_BLOCK / 64];
    StWaveLds<QG>& L = lds_all[wave];
    const uint32_t qbase = (qb * (NN_BLOCK / 64) + wave) * (32 * QG);
    // lane (n, h) owns query n of the groups 2 p + h: it builds their operands (st_setup) and carries their thresholds; the other
    // half-lane of the column gets its half of the operand by v_permlane32_swap.  The flush reads the queries from LDS.
    static_assert(QG % 2 == 0, "groups come in pairs");
    float qx[QG / 2], qy[QG / 2], qz[QG / 2], thr[QG / 2];
    bool ok[QG / 2];
    bool okg[QG];                                             // per group: every query of it served by the filter (wave-uniform)
#pragma unroll
    for (int p = 0; p < QG / 2; p++) {
        const uint32_t slot = (2 * p + (h ? 1 : 0)) * 32 + n, i = min(qbase + slot, ns - 1);
        qx[p] = sx[i]; qy[p] = sy[i]; qz[p] = sz[i];
        const uint32_t cb = (uint32_t)(__atomic_load_n(&keys[i], __ATOMIC_RELAXED) >> 32);      // the candidate's d2 (or what other slices published)
        // a query the filter can serve: finite coordinates and a finite candidate (else: exact scan of the slice below)
        ok[p] = fabsf(qx[p]) < 1e18f && fabsf(qy[p]) < 1e18f && fabsf(qz[p]) < 1e18f && cb < 0x7F7FFFFFu;
        thr[p] = ok[p] ? __uint_as_float(cb) : -INFINITY;
        L.q[slot] = make_float4(qx[p], qy[p], qz[p], 0.0f);
        L.best[slot] = ~0ull;
        if (!ok[p]) { qx[p] = 0.0f; qy[p] = 0.0f; qz[p] = 0.0f; }                                // (finite operands; thr = -inf: no flag, ever)
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok[p]);
        okg[2 * p] = (uint32_t)okm == 0xFFFFFFFFu; okg[2 * p + 1] = (uint32_t)(okm >> 32) == 0xFFFFFFFFu;
    }
    if (stopv) return;
    unsigned long long clk0 = 0, rt0 = 0;
    if (stats) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    uint32_t st_flushes = 0, st_eval = 0;
    const uint32_t sb = sl * supers_per_slice, se = min(sb + supers_per_slice, n_super);
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    uint4 pre0 = make_uint4(0, 0, 0, 0), pre1 = pre0;
    if (sb < se) {
        sA[0][threadIdx.x] = ops[(size_t)sb * TPS * 64 + threadIdx.x];
        sA[0][NN_BLOCK + threadIdx.x] = ops[(size_t)sb * TPS * 64 + NN_BLOCK + threadIdx.x];
    }
    __syncthreads();
    uint32_t cnt = 0;                                         // entries in the wave's list (wave-uniform)
    bool refresh = false;                                     // LDS holds better candidates than the thresholds in registers (wave-uniform)
    uint32_t st_dense = 0;
    uint4 bq[QG];
    for (uint32_t S = sb; S < se; S++) {
        const uint32_t buf = (S - sb) & 1u;
        if (S + 1 < se) {                                     // the next super-tile: in flight during this one's eight tiles
            pre0 = ops[(size_t)(S + 1) * TPS * 64 + threadIdx.x];
            pre1 = ops[(size_t)(S + 1) * TPS * 64 + NN_BLOCK + threadIdx.x];
        }
        const float4 C = centres[S];                          // wave-uniform: scalar load; .w = the super-tile's scale (a power of two)
        const float sc2 = C.w * C.w;                          // exact: |exponent| <= 120
        uint4 A = sA[buf][lane];                              // the first tile's operand: on its way while the query side is built
#ifdef PCR_ST_TIMING_NOSETUP                                  // (timing builds only: what the operand setup costs — wrong answers)
        if (S == sb)
#endif
#pragma unroll
        for (int p = 0; p < QG / 2; p++) {
            uint32_t P[4], Q[4];
            st_setup(qx[p], qy[p], qz[p], C, thr[p], sc2, P, Q);
            // P: what the lower half-lane of my column feeds the MFMA, Q: the upper half-lane's.  Swapping P's upper 32 lanes with Q's
            // lower 32 leaves group 2 p complete in P and group 2 p + 1 complete in Q.
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const auto r = __builtin_amdgcn_permlane32_swap(P[j], Q[j], false, false);
                P[j] = r[0]; Q[j] = r[1];
            }
            bq[2 * p] = make_uint4(P[0], P[1], P[2], P[3]);
            bq[2 * p + 1] = make_uint4(Q[0], Q[1], Q[2], Q[3]);
        }
#pragma unroll PCR_ST_UNROLL
        for (int tt = 0; tt < TPS; tt++) {
            const uint4 An = sA[buf][min(tt + 1, TPS - 1) * 64 + lane];       // the next tile's operand, one tile ahead
            // ONE chain of ORs over the 64 accumulators of the tile's four groups (8 v_or3_b32 per group and nothing to combine afterwards:
            // 32 vector instructions per tile instead of 36); which group raised a sign is found out in the rare branch, by running the
            // tile's MFMAs again
            uint32_t any;
            {
                const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, bq[0]), zero, 0, 0, 0);
                any = __float_as_uint(acc[0]) | __float_as_uint(acc[1]) | __float_as_uint(acc[2]);
#pragma unroll
                for (int j = 3; j + 1 < 16; j += 2) any = any | __float_as_uint(acc[j]) | __float_as_uint(acc[j + 1]);
                any |= __float_as_uint(acc[15]);
            }
#pragma unroll
            for (int g = 1; g < QG; g++) {
                const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, bq[g]), zero, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 16; j += 2) any = any | __float_as_uint(acc[j]) | __float_as_uint(acc[j + 1]);
            }
            if (__builtin_amdgcn_ballot_w64((int)any < 0)) {
                // rare: some half-lane's chunk (records 32 T + 16 h ...) may hold a record at or below its query's threshold
                const uint32_t crel = (((S - sb) * TPS + (uint32_t)tt) * 2 + (h ? 1u : 0u)) << 7;
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    uint32_t og;
                    {
                        const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, bq[g]), zero, 0, 0, 0);
                        og = __float_as_uint(acc[0]) | __float_as_uint(acc[1]) | __float_as_uint(acc[2]);
#pragma unroll
                        for (int j = 3; j + 1 < 16; j += 2) og = og | __float_as_uint(acc[j]) | __float_as_uint(acc[j + 1]);
                        og |= __float_as_uint(acc[15]);
                    }
                    const unsigned long long m = __builtin_amdgcn_ballot_w64((int)og < 0);
                    if (!m) continue;
                    const uint32_t k = (uint32_t)__popcll(m);
                    if (k >= dense_at) {
                        // Many columns of this group flag the SAME tile (a sorted working cloud behind coarse seeds: the first search of a
                        // loop): the flagged half-lanes evaluate their chunk in place — the 32 lanes of a half read the same 16 records
                        // (uniform addresses, four loads in flight), every lane for its own query — instead of filling the list with up to
                        // 64 entries per group and tile (lists that overflowed several times per tile: 1.17 ms for such a search, 0.5x now)
                        if ((int)og < 0) {
                            const float4 q = L.q[g * 32 + n];
                            const float4* rp = records + (size_t)(sb * TPS * 2 + (crel >> 7)) * 16;
                            unsigned long long kb = ~0ull;
#pragma unroll 4
                            for (int j = 0; j < 16; j++) {
                                const float4 rec = rp[j];                                   // (padding records: x = +inf, never accepted)
                                const uint32_t d = d2_exact_bits(q.x, q.y, q.z, rec.x, rec.y, rec.z);
                                const unsigned long long key = ((unsigned long long)d << 32) | __float_as_uint(rec.w);
                                if (d < 0x7F7FFFFFu && key < kb) kb = key;                   // FLT_MAX gate
                            }
                            if (kb != ~0ull) atomicMin(&L.best[g * 32 + n], kb);
                        }
                        st_eval += k; st_dense++;
                        refresh = true;
                        continue;
                    }
                    if (cnt + k > (uint32_t)ST_CAP) { st_flush<QG>(L, cnt, sb * TPS * 2, records, lane); st_flushes++; st_eval += cnt; cnt = 0; refresh = true; }
                    if ((int)og < 0) L.list[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = crel | (uint32_t)(g * 32) | n;
                    cnt += k;
                }
            }
            A = An;
        }
        if (cnt >= flush_at || (cnt && S + 1 == se)) {
            // the chunks flagged so far, evaluated together.  (Not after every super-tile: a flush is a dependent global round trip,
            // longer than a super-tile's 32 MFMAs, and the other three waves of the workgroup wait for it at the barrier below.)
            st_flush<QG>(L, cnt, sb * TPS * 2, records, lane); st_flushes++; st_eval += cnt; cnt = 0; refresh = true;
        }
        if (refresh) {
            // the thresholds fall to what was found before the next operands are built
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int p = 0; p < QG / 2; p++) {
                const uint32_t fb = (uint32_t)(L.best[(2 * p + (h ? 1 : 0)) * 32 + n] >> 32);   // (~0 >> 32 is a NaN pattern: fminf keeps thr)
                thr[p] = ok[p] ? fminf(thr[p], __uint_as_float(fb)) : thr[p];
            }
            refresh = false;
        }
        if (S + 1 < se) { sA[buf ^ 1u][threadIdx.x] = pre0; sA[buf ^ 1u][NN_BLOCK + threadIdx.x] = pre1; }
        __syncthreads();
    }
#pragma unroll
    for (int g = 0; g < QG; g++) {
        unsigned long long kbest = L.best[g * 32 + n];
        if (!okg[g] && sb < se) {
            // a query without finite coordinates or without a candidate: the wave scans the slice exactly for this group, each half-lane
            // one half of it (rare: NaN / inf queries, a seed kernel that found nothing acceptable)
            const float4 q = L.q[g * 32 + n];
            const uint32_t r0 = sb * BT_SUPER, r1 = min(se * BT_SUPER, n_rec), mid = r0 + (r1 - r0) / 2;
            for (uint32_t j = h ? mid : r0; j < (h ? r1 : mid); j++) {
                const float4 rec = records[j];
                const uint32_t e = d2_exact_bits(q.x, q.y, q.z, rec.x, rec.y, rec.z);
                const unsigned long long key = ((unsigned long long)e << 32) | __float_as_uint(rec.w);
                if (e < 0x7F7FFFFFu && key < kbest) kbest = key;
            }
            const unsigned long long ko = key_xor32(kbest);
            kbest = ko < kbest ? ko : kbest;
            // "no neighbour" is the key (+inf, no index), as every other kernel writes it (a seed kernel that found nothing left ~0 behind)
            if (kbest == ~0ull) kbest = 0x7F800000FFFFFFFFull;
        }
        const uint32_t i = qbase + g * 32 + n;
        if (!h && i < ns && kbest != ~0ull) merge_key(&keys[i], kbest);
    }
    if (stats) {
        if (lane == 0) {
            if (st_flushes) atomicAdd(&stats[2], (unsigned long long)st_flushes);                 // joint evaluations (wave level)
            if (st_dense) atomicAdd(&stats[7], (unsigned long long)st_dense);                     // (group, tile) pairs evaluated in place
            if (st_eval) atomicAdd(&stats[6], (unsigned long long)st_eval);                       // (query, chunk) pairs evaluated exactly
        }
        if (threadIdx.x == 0) {
            atomicAdd(&stats[4], (unsigned long long)__builtin_amdgcn_s_memtime() - clk0);
            atomicAdd(&stats[5], (unsigned long long)__builtin_amdgcn_s_memrealtime() - rt0);
        }
    }
}

#include "nn1_sphere.hpp"

// ICP iterations after the first: the previous correspondence, re-evaluated exactly against the moved query, is a genuine
// candidate and therefore an upper bound of the new answer from the first instruction on (ETRACK settles every far slice with it).
__global__ __launch_bounds__(NN_BLOCK) void nn1_seed_kernel(const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, uint32_t nt,
                                                            const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
                                                            unsigned long long* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const uint32_t j = (uint32_t)(keys[i] & 0xFFFFFFFFull);
    unsigned long long key = ~0ull;
    if (j < nt) {
        const uint32_t e = d2_exact_bits(sx[i], sy[i], sz[i], tx[j], ty[j], tz[j]);
        if (e < 0x7F7FFFFFu) key = ((unsigned long long)e << 32) | j;                   // FLT_MAX gate, nanoflann.hpp:163,1360
    }
    keys[i] = key;
}

// Seeds for a COLD search over BTRACK's index: the super-tile whose centre is nearest to the query (a scan of the few hundred
// centres, wave-uniform loads), then 32 of its 256 records evaluated exactly — a genuine candidate a few centimetres to decimetres
// from the true neighbour.  With it published in keys[] the main pass settles nearly every slice in its prologue, as in a warm ICP
// iteration (0.95 -> ? ms per unseeded 120 k x 120 k search); without it every slice evaluates a chunk exactly and proves it.
__global__ __launch_bounds__(NN_BLOCK) void bt_seed_kernel(const float4* __restrict__ centres, const float4* __restrict__ records, uint32_t n_super, uint32_t centre_step,
                                                           const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
                                                           unsigned long long* __restrict__ keys, int merge, const float4* __restrict__ l1_centres, uint32_t n_l1)
{
    const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const float qx = sx[i], qy = sy[i], qz = sz[i];
    float bc = INFINITY;
    uint32_t sc = 0;
    if (l1_centres) {
        // two levels (round 4, where the level-1 super-tiles exist): the two nearest level-1 centres (means of 4 096 records) of all of them, then the 16
        // super-tile centres under each — 30 + 32 centres at 120 000 points instead of 469
        float b1 = INFINITY, b2 = INFINITY;
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t c = 0; c < n_l1; c++) {
            const float4 C = l1_centres[c];
            const float dx = qx - C.x, dy = qy - C.y, dz = qz - C.z;
            const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            if (d < b1) { b2 = b1; s2 = s1; b1 = d; s1 = c; } else if (d < b2) { b2 = d; s2 = c; }
        }
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const uint32_t c0 = (pass ? s2 : s1) * (BT_L1_SUPER / BT_SUPER);
            if (pass && !(b2 < INFINITY)) break;
            for (uint32_t u = 0; u < (uint32_t)(BT_L1_SUPER / BT_SUPER) && c0 + u < n_super; u++) {
                const float4 C = centres[c0 + u];
                const float dx = qx - C.x, dy = qy - C.y, dz = qz - C.z;
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                if (d < bc) { bc = d; sc = c0 + u; }
            }
        }
    } else {
    // (eight wave-uniform centre loads in flight: one scalar-cache round trip per centre made this scan 64 us at 120 k queries)
    const uint32_t n_c = (n_super + centre_step - 1) / centre_step;
    uint32_t c0 = 0;
    if (centre_step == 1) {                                   // (up to 1 024 super-tiles: consecutive centres, wide scalar loads)
        for (; c0 + 8 <= n_c; c0 += 8) {
            float4 C[8];
#pragma unroll
            for (int u = 0; u < 8; u++) C[u] = centres[c0 + u];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const float dx = qx - C[u].x, dy = qy - C[u].y, dz = qz - C[u].z;
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                if (d < bc) { bc = d; sc = c0 + u; }
            }
        }
    }
    for (; c0 < n_c; c0++) {
        const float4 C = centres[(size_t)c0 * centre_step];
        const float dx = qx - C.x, dy = qy - C.y, dz = qz - C.z;
        const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        if (d < bc) { bc = d; sc = c0 * centre_step; }
    }
    }
    unsigned long long key = ~0ull;
    // (64 / 128 / 256 samples: 6.1 / 5.5 / 5.1 instead of 6.9 flagged chunks per query, no faster.)  Eight gathers in flight per lane: the
    // 32 loads of a lane are scattered 16-byte reads (every lane its own super-tile unless the queries are sorted)
    const float4* rp = records + (size_t)sc * BT_SUPER + (i & (BT_SUPER / 32 - 1));
#pragma unroll 1
    for (int j0 = 0; j0 < 32; j0 += 8) {
        float4 rec[8];
#pragma unroll
        for (int u = 0; u < 8; u++) rec[u] = rp[(uint32_t)(j0 + u) * (BT_SUPER / 32)];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t e = d2_exact_bits(qx, qy, qz, rec[u].x, rec[u].y, rec[u].z);
            const unsigned long long k = ((unsigned long long)e << 32) | __float_as_uint(rec[u].w);
            if (e < 0x7F7FFFFFu && k < key) key = k;                               // FLT_MAX gate; padding records have x = +inf
        }
    }
    // merge: keys[] already holds a candidate (a stale correspondence re-evaluated by nn1_seed_kernel) — the better of the two stays
    if (merge) { const unsigned long long old = keys[i]; key = old < key ? old : key; }
    keys[i] = key;
}

// Seeds for a cold search, second form (round 4): the records are in Morton order on a known lattice (BtIndex::key_lo / key_inv), so the record whose
// key is nearest to the QUERY's key is found by a binary search over the records themselves (their 30-bit key recomputed from their coordinates — a
// prefix of the key they were sorted by, so it is monotone along them) — 17 dependent 16-byte loads instead of a scan of every super-tile's centre —
// and the 32 records around it are evaluated exactly.  A Morton neighbour is a spatial neighbour except across the curve's jumps; those queries get a
// poorer seed, never a wrong answer (the search that follows is exhaustive).
__global__ __launch_bounds__(NN_BLOCK) void bt_seed_morton_kernel(const float4* __restrict__ records, uint32_t n_rec, float lox, float loy, float loz, float inv,
                                                                  const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,
                                                                  unsigned long long* __restrict__ keys, int merge)
{
    const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const float qx = sx[i], qy = sy[i], qz = sz[i];
    unsigned long long key = ~0ull;
    if (fabsf(qx) < 1e30f && fabsf(qy) < 1e30f && fabsf(qz) < 1e30f) {
        const uint32_t kq = bt_morton(bt_fine_cell(qx, lox, inv), bt_fine_cell(qy, loy, inv), bt_fine_cell(qz, loz, inv));
        uint32_t lo = 0, hi = n_rec;                          // the first record whose key is >= kq
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const float4 r = records[mid];
            const bool fin = fabsf(r.x) < 1e30f && fabsf(r.y) < 1e30f && fabsf(r.z) < 1e30f;
            const uint32_t kr = fin ? bt_morton(bt_fine_cell(r.x, lox, inv), bt_fine_cell(r.y, loy, inv), bt_fine_cell(r.z, loz, inv)) : (1u << 30);
            if (kr < kq) lo = mid + 1; else hi = mid;
        }
        const uint32_t p0 = (uint32_t)max((int)min(lo, n_rec - 1u) - 16, 0), p1 = min(p0 + 32u, n_rec);
#pragma unroll 1
        for (uint32_t j0 = p0; j0 < p1; j0 += 8) {
            float4 rec[8];
#pragma unroll
            for (int u = 0; u < 8; u++) rec[u] = records[min(j0 + (uint32_t)u, n_rec - 1u)];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t e = d2_exact_bits(qx, qy, qz, rec[u].x, rec[u].y, rec[u].z);
                const unsigned long long k = ((unsigned long long)e << 32) | __float_as_uint(rec[u].w);
                if (e < 0x7F7FFFFFu && k < key) key = k;                               // FLT_MAX gate; padding records have x = +inf
            }
        }
    }
    if (merge) { const unsigned long long old = keys[i]; key = old < key ? old : key; }
    keys[i] = key;
}

// a caller's loop search is bounded by its gate (pcr.h pcr_nn1_f32_loop): a key at or beyond it becomes "none", as the grid search returns it
// (test_context_state.py §A / §E: the exhaustive path returned the neighbour outside the gate)
__global__ __launch_bounds__(NN_BLOCK) void nn1_gate_kernel(unsigned long long* __restrict__ keys, uint32_t ns, float gate)
{
    const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const unsigned long long k = keys[i];
    if ((uint32_t)k != 0xFFFFFFFFu && !(__uint_as_float((uint32_t)(k >> 32)) < gate)) keys[i] = (0x7F800000ull << 32) | 0xFFFFFFFFull;   // none: (+inf, UINT32_MAX)
}

int launch_nn1_gate(pcr_ctx* ctx, size_t ns, float gate)
{
    if (ns == 0 || !(gate < __builtin_inff())) return PCR_OK;
    hipLaunchKernelGGL(nn1_gate_kernel, dim3((unsigned)((ns + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, ctx->stream, ctx->keys, (uint32_t)ns, gate);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// keys -> (idx, d2) split for the host-facing API
__global__ void nn1_unpack_kernel(const unsigned long long* __restrict__ keys, uint32_t n,
                                  uint32_t* __restrict__ idx, float* __restrict__ d2)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        unsigned long long k = keys[i];
        idx[i] = (uint32_t)(k & 0xFFFFFFFFull);
        d2[i] = __uint_as_float((uint32_t)(k >> 32));
    }
}

// ---------------------------------------------------------------------------------------------------------------- dispatcher
// Which kernel serves an exhaustive search (tune nn1_variant forces one; 0 = this table):
//
//   target                          search                                   kernel
//   ------------------------------  ---------------------------------------  -----------------------------------------------------------
//   >= 32 768 points, fits f16      any (a cold search seeds itself first)   STRACK3 nn1_strack3_kernel<1 | 2 | 4>  (nn1_sphere.hpp; variant 10: any size.  The sign
//                                                                            filter at three levels — rows per 512-record tile, per 16-record chunk, per record)
//   >= 8 192 points, fits f16       any (a cold search seeds itself first)   STRACK  nn1_strack_kernel<4 | 2>       (variant 8: small targets too)
//   —                               only on request (nn1_sign = 2)           HTRACK  nn1_btrack_kernel<4 | 2, true>   (variant 7: the minimum-tracking form of
//                                                                            the f16 filter — round 4: no default path reaches it any more; measured cold,
//                                                                            8 192 ... 60 000 points: STRACK 0.020 / 0.044 / 0.090 / 0.235 ms against 0.029 /
//                                                                            0.052 / 0.105 / 0.253; it stays as the parity sweeps' second f16 kernel)
//   >= 8 192 points, beyond f16     any                                      BTRACK  nn1_btrack_kernel<4 | 2, false>  (variant 6)
//   either form failing the device check (mfma_verdict), or nn1_bf16 = 2     the two rows below
//   >= 2 048 points                 inside a loop / index exists / 2nd search ETRACK  nn1_etrack_kernel<4>             (variant 4)
//   anything else                   (first one-shot search, small targets)   FTRACK  nn1_ftrack_kernel<2, 16>         (variant 1)
//   —                               only on request                          TRACK   nn1_track_kernel<2, 16>          (variant 2: exact arithmetic
//                                                                            for every pair — the on-device reference of the others)
// (Targets below 2 048 points inside loops, and one-shot searches with queries x targets > 2e9, never get here: api.cpp nn1_auto_grid
// sends them to the exact grid.)  Tune keys read here — every one 0 = default:
//   nn1_variant (above) · nn1_bf16 (1 force / 2 forbid the matrix-core forms) · nn1_f16 (1 / 2 the same for the f16 form) ·
//   nn1_sign (the sign forms: 2 = never) · nn1_sphere (0 auto / 1 always / 2 never), nn1_sphere_qg (groups of 32 queries per wave), nn1_sphere_flush_end,
//   nn1_sphere_l0_per_slice / nn1_sphere_blocks, nn1_sphere_reseed, nn1_seed_mode ·
//   nn1_sign_flush (list entries from which the end
//   of a super-tile evaluates them, default 64) · nn1_sign_dense (flagged half-lanes of one (group, tile) from which they evaluate in place, 12) ·
//   nn1_btrack_qg (query groups of 32 per wave: 2 or 4; default 2 up to 49 152 queries) · nn1_supers_per_slice / nn1_btrack_blocks
//   (slice length of the matrix-core launch directly / via the workgroup count, default 14 336) · nn1_xcd (XCD-aware launch: 1 / 2 / 4
//   query-block groups per 8 XCDs, -1 plain 2-D launch; default 4) · nn1_cold_seed (2 = off) · nn1_warm_start (2 = off) ·
//   nn1_chunks_per_slice / nn1_etrack_blocks (ETRACK, default 32 768 workgroups) · nn1_tiles_per_slice / nn1_target_blocks (FTRACK / TRACK,
//   default 16 384) · mfma_force_fail (tests) · grid_stats (diagnostics launch).  Retired in round 3 with the kernels they selected:
//   nn1_qpl, nn1_chunk, nn1_etrack_qpl, nn1_lds_ops, variant 3 (LDS-tiled TRACK).

// slices of `n_units` units such that about `want_blocks` workgroups exist; returns units per slice, *slices = how many (<= 65 535)
static uint32_t slice_plan(uint32_t n_units, uint32_t qblocks, int64_t per_slice_tune, int64_t want_blocks, uint32_t* slices)
{
    int64_t per = per_slice_tune;
    if (per <= 0) {
        const int64_t s = std::max<int64_t>(1, (want_blocks + qblocks - 1) / std::max<uint32_t>(qblocks, 1u));
        per = std::max<int64_t>(1, ((int64_t)n_units + s - 1) / s);
    }
    uint32_t ns = n_units ? (uint32_t)((n_units + per - 1) / per) : 1u;
    if (ns > 65535u) { ns = 65535u; per = (n_units + ns - 1) / ns; ns = (uint32_t)((n_units + per - 1) / per); }
    *slices = ns;
    return (uint32_t)per;
}

static int stats_buffer(pcr_ctx* ctx, unsigned long long** out)
{
    *out = nullptr;
    if (tune_get(ctx, "grid_stats", 0) <= 0) return PCR_OK;
    if (!ctx->grid_stats_dev) PCR_HIP(ctx, hipMalloc((void**)&ctx->grid_stats_dev, PCR_NSTATS * sizeof(unsigned long long)));
    PCR_HIP(ctx, hipMemsetAsync(ctx->grid_stats_dev, 0, PCR_NSTATS * sizeof(unsigned long long), ctx->stream));
    *out = ctx->grid_stats_dev;
    return PCR_OK;
}

// the seeds of a warm search: keys[] <- the previous correspondences re-evaluated exactly (unless the last move wrote them already)
static void seed_warm(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool pre_seeded)
{
    if (pre_seeded) return;
    hipLaunchKernelGGL(nn1_seed_kernel, dim3((unsigned)((src->n + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(),
                       (uint32_t)tgt->n, src->x(), src->y(), src->z(), (uint32_t)src->n, ctx->keys);
}

// STRACK3's launch: one wave per 32 x qg queries and slice of level-0 super-tiles (131 072 records each).  From plain numbers: the loop asks before it
// has a launch to look at (s3_move_route)
struct S3Geometry { uint32_t qg, qblocks, l0_per_slice, slices; };
static S3Geometry s3_geometry(uint64_t n_l0, uint64_t ns, int64_t qg_tune, int64_t l0_per_slice_tune, int64_t blocks_tune)
{
    S3Geometry G;
    G.qg = qg_tune == 4 ? 4u : qg_tune == 2 ? 2u : 1u;        // (one group of 32 queries per wave: 120 000 queries are 3 750 waves for 1 024 SIMDs — the search is a chain of
                                                              // dependent trips to memory per wave, and waves are what hides them)
    const uint64_t qpb = (uint64_t)(NN_BLOCK / 64) * 32 * G.qg;
    G.qblocks = (uint32_t)((ns + qpb - 1) / qpb);
    G.slices = 1;
    G.l0_per_slice = slice_plan((uint32_t)n_l0, G.qblocks, l0_per_slice_tune, blocks_tune ? blocks_tune : 1024, &G.slices);
    return G;
}

uint64_t s3_l0_super_tiles(uint64_t n_tgt)
{
    const uint64_t n_pad = (n_tgt + BT_SUPER - 1) / BT_SUPER * BT_SUPER;       // (bt_ensure pads to whole super-tiles of records, bt_ensure_l1 counts from there)
    return (n_pad + BT_L0_SUPER - 1) / BT_L0_SUPER;
}

// Can a seeded STRACK3 search of ns queries over n_l0 level-0 super-tiles move its queries in place (nn1_strack3_move_kernel)?  Only the transposed
// default form is built with the move, and only ONE slice is safe: with more, several workgroups read a query block that one of them overwrites.
// Raw tune values (0 = default), no context: pure host logic (pcr_icp_move_route)
bool s3_move_route(uint64_t n_l0, uint64_t ns, int64_t transposed_tune, int64_t qg_tune, int64_t l0_per_slice_tune, int64_t blocks_tune)
{
    if (ns == 0 || n_l0 == 0 || transposed_tune == 2) return false;
    return s3_geometry(n_l0, ns, qg_tune, l0_per_slice_tune, blocks_tune).slices == 1;
}

// HTRACK / BTRACK over the target's Morton-ordered operands (bt_ensure)
static int launch_matrix(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool f16, bool warm, bool pre_seeded, bool force_sign)
{
    const BtIndex* g = tgt->bt;
    const size_t ns = src->n;
    // the loop's chain search -> sums + solve (icp.cpp): this search moves its queries by the pending Rd, td of that state and seeds itself from the
    // previous correspondences on the way — nothing to seed in front of it.  It is STRACK3's move-carrying form or an error, never another kernel
    const IcpState* const move_state = ctx->nn1_move_state;
    if (move_state) pre_seeded = true;
    // ... and on the chain sums -> search it finishes the previous iteration first: the same form with the solve in its prologue
    const IcpSolveArgs* const solve = ctx->nn1_solve;
    if (solve && !move_state) return fail(ctx, PCR_ERR_STATE, "nn1: a search that finishes an iteration must carry its move");
    // query groups (of 32) per wave: four amortise the per-tile operand loads best on a full batch; a source shard of a strong-scaling run
    // (15-30 k queries against the whole target) fills the chip better with two — measured, per ICP iteration: 15 k queries 0.158 -> 0.137
    // ms, 30 k 0.241 -> 0.218, 60 k 0.378 / 0.375, 120 k 0.664 -> 0.723
    int qg = tune_get(ctx, "nn1_btrack_qg", ns <= 49152 ? 2 : 4) == 2 ? 2 : 4;
    if (tune_get(ctx, "nn1_variant", 0) == 9 || tune_get(ctx, "nn1_variant", 0) == 10 || tune_get(ctx, "nn1_sphere", 0) == 1 || (tune_get(ctx, "nn1_sphere", 0) == 0 && tune_get(ctx, "nn1_variant", 0) == 0 && f16 &&
        tgt->n >= 32768 && tune_get(ctx, "nn1_btrack_qg", 0) == 0)) qg = 4;                     // (the launch geometry below is STRACK's; the sphere form has its own)
    const size_t qpb = (size_t)(NN_BLOCK / 64) * 32 * qg;                          // queries per workgroup
    const uint32_t qblocks = (uint32_t)((ns + qpb - 1) / qpb);
    const uint32_t n_super = (uint32_t)(g->n_tiles / (BT_SUPER / 32));
    // (120 k: 8 super-tiles per slice, the measured optimum of both forms since their unsettled queries are filtered again)
    uint32_t slices = 1;
    const uint32_t sps = slice_plan(n_super, qblocks, tune_get(ctx, "nn1_supers_per_slice", 0), tune_get(ctx, "nn1_btrack_blocks", 14336), &slices);
    // a cold search seeds itself from the nearest super-tile (tune nn1_cold_seed: 2 = off, 3 = only sliced launches — round 3's rule, under which
    // the one-slice launches of small targets were HTRACK's last default use)
    const int64_t cs_tune = tune_get(ctx, "nn1_cold_seed", 1);
    const bool cold_seed = !warm && (cs_tune == 1 || (cs_tune == 3 && (slices > 1 || force_sign)));
    const int merge_atomic = (slices > 1 || warm || cold_seed) ? 1 : 0;
    // STRACK, the sign form of the f16 filter, serves every search that starts from a candidate per query in keys[]: the searches seeded by
    // the move of the previous iteration (kabsch.hip seed_next_search), the cold ones that seed themselves (bt_seed_kernel: 0.55 ms against
    // HTRACK's 0.60), and the warm ones whose seeds are old correspondences re-evaluated by nn1_seed_kernel.  Those may stem from another
    // loop's final pose — decimetres to metres off, 0.88 ms — so they are merged with the cold seed: every seed is then at least as good
    // as a cold search's.  Tune nn1_sign: 2 = never (HTRACK's minimum tracking), nn1_variant 8 = also the one-slice launches of small
    // targets (the parity tests' way to put the kernel in front of every input).
    const int64_t sign_tune = tune_get(ctx, "nn1_sign", 0);
    const bool sign = force_sign ? (warm || cold_seed) : f16 && sign_tune != 2 && (warm || cold_seed);
    bool reseed = sign && warm && !pre_seeded && tune_get(ctx, "nn1_cold_seed", 1) == 1;
    // STRACK3 (nn1_sphere.hpp): the sign filter over three levels of bounding spheres.  Tune nn1_sphere: 0 auto (targets from 32 768 points on, where a
    // level-1 super-tile of 4 096 records is a small part of the cloud), 1 = always, 2 = never; nn1_variant 10 (9: its old number) forces it.
    const int64_t sph_tune = tune_get(ctx, "nn1_sphere", 0), variant_now = tune_get(ctx, "nn1_variant", 0);
    bool sphere = sign && f16 && qg == 4 && sph_tune != 2 && (variant_now == 9 || variant_now == 10 || sph_tune == 1 || (variant_now == 0 && tgt->n >= 32768));
    if (sphere) {
        int rc1 = bt_ensure_l1(ctx, tgt);
        if (rc1) return rc1;
        BtIndex* bt = tgt->bt;
        if (bt->l1_bad_host < 0) {
            int flag = 1;
            PCR_HIP(ctx, hipMemcpyAsync(&flag, bt->l1_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
            bt->l1_bad_host = flag;
        }
        sphere = bt->l1_bad_host == 0;
    }
    // (the sphere forms pay far less for a poor seed than STRACK does — tune nn1_sphere_reseed: 2 = a warm search keeps its stale seeds as they are)
    if (sphere && tune_get(ctx, "nn1_sphere_reseed", 0) == 2) reseed = false;
    const int64_t s3_tr = tune_get(ctx, "nn1_s3_transposed", 0), s3_qg = tune_get(ctx, "nn1_sphere_qg", 0), s3_l0ps = tune_get(ctx, "nn1_sphere_l0_per_slice", 0),
                  s3_blocks = tune_get(ctx, "nn1_sphere_blocks", 0);
    ctx->nn1_move_l0 = sphere ? g->n_l0_super : 0;      // (what the loop asks after its first search: icp_move_route)
    if (move_state && !(sphere && warm && s3_move_route(g->n_l0_super, ns, s3_tr, s3_qg, s3_l0ps, s3_blocks))) return fail(ctx, PCR_ERR_STATE, "nn1: this search cannot carry the loop's pending move (STRACK3, transposed, one slice)");
    ctx->last_nn1_kernel = sphere ? "strack3" : sign ? "strack" : f16 ? "htrack" : "btrack";
    if (warm) seed_warm(ctx, tgt, src, pre_seeded);
    else if (merge_atomic && !cold_seed) PCR_HIP(ctx, hipMemsetAsync(ctx->keys, 0xFF, ns * sizeof(unsigned long long), ctx->stream));
    unsigned long long* stats_dev = nullptr;
    int rc = stats_buffer(ctx, &stats_dev);
    if (rc) return rc;
    {
        ProfScope p(ctx, "nn1_brute", 1);
        // (tune nn1_seed_mode: 1 = the nearest super-tile's centre, 2 = the Morton neighbour by binary search, 3 = both, merged; 0 = both for a cold search —
        // first search of a fresh pair, 120 k, three pairs: 0.147 / 0.295 / 0.290 -> 0.095 / 0.159 / 0.212 ms; a one-shot search of unsorted queries 0.366 ->
        // 0.304 ms, 6.5 -> 2.4 chunks evaluated per query — and the centre alone where stale correspondences are merged in: 0.185 against 0.194 ms)
        const int64_t seed_tune = tune_get(ctx, "nn1_seed_mode", 0), seed_mode = seed_tune ? seed_tune : (cold_seed ? 3 : 1);
        // the centre seed merges only with what this search wrote: without the Morton seed (a target of zero extent, or one below the Morton lattice:
        // key_inv = 0) a cold search's keys[] still holds an earlier search's keys (test_context_state.py §A)
        const bool morton = (cold_seed || reseed) && seed_mode >= 2 && g->key_inv > 0.f;
        if (morton)
            hipLaunchKernelGGL(bt_seed_morton_kernel, dim3((unsigned)((ns + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, ctx->stream, g->records, n_super * BT_SUPER,
                               g->key_lo[0], g->key_lo[1], g->key_lo[2], g->key_inv, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, reseed ? 1 : 0);
        if ((cold_seed || reseed) && (seed_mode < 2 || seed_mode == 3 || !(g->key_inv > 0.f)))          // (inside the timed scope: it is part of the search)
            hipLaunchKernelGGL(bt_seed_kernel, dim3((unsigned)((ns + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, ctx->stream, g->centres, g->records, n_super,
                               std::max<uint32_t>(1u, n_super / 1024u), src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, (reseed || (morton && seed_mode == 3)) ? 1 : 0,
                               (sphere && tune_get(ctx, "nn1_seed_levels", 0) != 1) ? g->l1_centres : (const float4*)nullptr, (uint32_t)g->n_l1_super);
        // XCD-aware launch (tune nn1_xcd: 1 / 2 / 4 = query-block groups per 8 XCDs, -1 = the plain 2-D launch): see the kernel
        // STRACK: entries in a wave's list from which the end of a super-tile evaluates them (tune nn1_sign_flush; the end of the slice always does)
        const uint32_t st_flush_at = (uint32_t)std::min<int64_t>(std::max<int64_t>(tune_get(ctx, "nn1_sign_flush", 64), 1), 1 << 20);
        // ... and flagged half-lanes of one (group, tile) from which they evaluate their chunk in place instead of listing it (tune nn1_sign_dense)
        const uint32_t st_dense_at = (uint32_t)std::min<int64_t>(std::max<int64_t>(tune_get(ctx, "nn1_sign_dense", 12), 1), 65);
        int64_t xq = tune_get(ctx, "nn1_xcd", NN_XCD_DEFAULT);
        if ((xq != 1 && xq != 2 && xq != 4) || slices < 8 || (uint64_t)qblocks * slices >= (1ull << 27)) xq = 0;
        const dim3 grid = xq ? dim3(8u * ((qblocks + (uint32_t)xq - 1) / (uint32_t)xq) * ((slices + 8u / (uint32_t)xq - 1) / (8u / (uint32_t)xq)), 1) : dim3(qblocks, slices);
#define PCR_BTRACK(Q, H, OPS)                                                                                                              \
    hipLaunchKernelGGL((nn1_btrack_kernel<Q, H>), grid, dim3(NN_BLOCK), 0, ctx->stream, g->centres, OPS, g->records, n_super * BT_SUPER, n_super, sps,  \
                       src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, merge_atomic, ctx->stop_flag_dev, stats_dev, (uint32_t)xq, qblocks, slices)
#define PCR_STRACK(Q)                                                                                                                      \
    hipLaunchKernelGGL((nn1_strack_kernel<Q>), grid, dim3(NN_BLOCK), 0, ctx->stream, g->centres, g->ops16, g->records, n_super * BT_SUPER, n_super, sps,  \
                       src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, ctx->stop_flag_dev, stats_dev, (uint32_t)xq, qblocks, slices, st_flush_at, st_dense_at)
        if (sphere) {
            // one wave per 128 (64: tune nn1_sphere_qg = 2) queries and slice of level-0 super-tiles (131 072 records each: one slice up to there)
            const uint32_t n_l0 = (uint32_t)g->n_l0_super;
            const S3Geometry G3 = s3_geometry(n_l0, ns, s3_qg, s3_l0ps, s3_blocks);
            const uint32_t qg3 = G3.qg, l0ps = G3.l0_per_slice;
            const dim3 grid3(G3.qblocks, G3.slices);
            const uint32_t s3_flush_end = (uint32_t)std::min<int64_t>(std::max<int64_t>(tune_get(ctx, "nn1_sphere_flush_end", 1), 1), S2_CAP);   // entries from which the end of a level-1 super-tile evaluates them
#define PCR_STRACK3(Q)                                                                                                                     \
    hipLaunchKernelGGL((nn1_strack3_kernel<Q>), grid3, dim3(NN_BLOCK), 0, ctx->stream, g->l0_centres, g->l0_ops, g->l1_centres, g->l1_ops, g->l1_rec_ops, g->records,  \
                       n_super * BT_SUPER, n_l0, l0ps, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, ctx->stop_flag_dev, stats_dev, std::min<uint32_t>(st_flush_at, (uint32_t)S2_CAP), s3_flush_end)
            // how levels 0 / 1 read the sphere-row masks (tune nn1_s3_transposed: 1 = one ballot of the transposed product, default; 2 = one ballot per accumulator)
#define PCR_STRACK3_ROWS(Q)                                                                                                                \
    hipLaunchKernelGGL((nn1_strack3_rows_kernel<Q>), grid3, dim3(NN_BLOCK), 0, ctx->stream, g->l0_centres, g->l0_ops, g->l1_centres, g->l1_ops, g->l1_rec_ops, g->records,  \
                       n_super * BT_SUPER, n_l0, l0ps, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, ctx->stop_flag_dev, stats_dev, std::min<uint32_t>(st_flush_at, (uint32_t)S2_CAP), s3_flush_end)
#define PCR_STRACK3_MOVE(Q)                                                                                                                \
    hipLaunchKernelGGL((nn1_strack3_move_kernel<Q>), grid3, dim3(NN_BLOCK), 0, ctx->stream, g->l0_centres, g->l0_ops, g->l1_centres, g->l1_ops, g->l1_rec_ops, g->records,  \
                       n_super * BT_SUPER, n_l0, l0ps, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, stats_dev, std::min<uint32_t>(st_flush_at, (uint32_t)S2_CAP), s3_flush_end, \
                       S3Move{ move_state, tgt->x(), tgt->y(), tgt->z(), (uint32_t)tgt->n })
#define PCR_STRACK3_SOLVE_MOVE(Q)                                                                                                          \
    hipLaunchKernelGGL((nn1_strack3_solve_move_kernel<Q>), grid3, dim3(NN_BLOCK), 0, ctx->stream, g->l0_centres, g->l0_ops, g->l1_centres, g->l1_ops, g->l1_rec_ops, g->records,  \
                       n_super * BT_SUPER, n_l0, l0ps, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, stats_dev, std::min<uint32_t>(st_flush_at, (uint32_t)S2_CAP), s3_flush_end, \
                       S3Move{ move_state, tgt->x(), tgt->y(), tgt->z(), (uint32_t)tgt->n }, *solve)
            if (move_state && solve) { if (qg3 == 1) PCR_STRACK3_SOLVE_MOVE(1); else if (qg3 == 2) PCR_STRACK3_SOLVE_MOVE(2); else PCR_STRACK3_SOLVE_MOVE(4); ctx->nn1_moved = true; }
            else if (move_state) { if (qg3 == 1) PCR_STRACK3_MOVE(1); else if (qg3 == 2) PCR_STRACK3_MOVE(2); else PCR_STRACK3_MOVE(4); ctx->nn1_moved = true; }
            else if (s3_tr == 2) { if (qg3 == 1) PCR_STRACK3_ROWS(1); else if (qg3 == 2) PCR_STRACK3_ROWS(2); else PCR_STRACK3_ROWS(4); }
            else if (qg3 == 1) PCR_STRACK3(1); else if (qg3 == 2) PCR_STRACK3(2); else PCR_STRACK3(4);
#undef PCR_STRACK3_SOLVE_MOVE
#undef PCR_STRACK3_MOVE
#undef PCR_STRACK3_ROWS
#undef PCR_STRACK3
        }
        else if (sign) { if (qg == 2) PCR_STRACK(2); else PCR_STRACK(4); }
        else if (f16) { if (qg == 2) PCR_BTRACK(2, true, g->ops16); else PCR_BTRACK(4, true, g->ops16); }
        else { if (qg == 2) PCR_BTRACK(2, false, g->ops); else PCR_BTRACK(4, false, g->ops); }
#undef PCR_STRACK
#undef PCR_BTRACK
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// ETRACK over the chunked, centred copy of the target's grid index (build_target_grid)
static int launch_etrack(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool warm, bool pre_seeded)
{
    const Grid* g = tgt->grid;
    const size_t ns = src->n;
    ctx->last_nn1_kernel = "etrack";
    constexpr int EQ = 4;                          // queries per lane: the filter is bound by the scalar operand path (272 B per chunk per wave)
    const uint32_t qblocks = (uint32_t)((ns + (size_t)NN_BLOCK * EQ - 1) / ((size_t)NN_BLOCK * EQ));
    uint32_t slices = 1;
    const uint32_t cps = slice_plan((uint32_t)g->n_chunks, qblocks, tune_get(ctx, "nn1_chunks_per_slice", 0), tune_get(ctx, "nn1_etrack_blocks", 32768), &slices);
    const int merge_atomic = (slices > 1 || warm) ? 1 : 0;
    if (warm) seed_warm(ctx, tgt, src, pre_seeded);
    else if (merge_atomic) PCR_HIP(ctx, hipMemsetAsync(ctx->keys, 0xFF, ns * sizeof(unsigned long long), ctx->stream));
    unsigned long long* stats_dev = nullptr;               // diagnostics: slot 2 counts the exact rescans of this launch
    int rc = stats_buffer(ctx, &stats_dev);
    if (rc) return rc;
    {
        ProfScope p(ctx, "nn1_brute", 1);
        hipLaunchKernelGGL((nn1_etrack_kernel<EQ>), dim3(qblocks, slices), dim3(NN_BLOCK), 0, ctx->stream, g->chunks, g->records, (uint32_t)tgt->n, (uint32_t)g->n_chunks,
                           cps, src->x(), src->y(), src->z(), (uint32_t)ns, ctx->keys, merge_atomic, ctx->stop_flag_dev, stats_dev);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// FTRACK (exact = false) / TRACK (exact = true) straight over the SoA target: no index at all
static int launch_plain(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool exact)
{
    const size_t ns = src->n;
    ctx->last_nn1_kernel = exact ? "track" : "ftrack";
    constexpr int QPL = 2;
    const uint32_t n_tiles = (uint32_t)((tgt->n + NN_TILE - 1) / NN_TILE);
    const uint32_t qblocks = (uint32_t)((ns + (size_t)NN_BLOCK * QPL - 1) / ((size_t)NN_BLOCK * QPL));
    // enough workgroups to balance 256 CUs x 8 resident blocks over several rounds
    uint32_t slices = 1;
    const uint32_t tps = slice_plan(n_tiles, qblocks, tune_get(ctx, "nn1_tiles_per_slice", 0), tune_get(ctx, "nn1_target_blocks", 16384), &slices);
    const int merge_atomic = slices > 1;
    if (merge_atomic) PCR_HIP(ctx, hipMemsetAsync(ctx->keys, 0xFF, ns * sizeof(unsigned long long), ctx->stream));
    {
        ProfScope p(ctx, "nn1_brute", 1);
        if (exact)
            hipLaunchKernelGGL((nn1_track_kernel<QPL, 16>), dim3(qblocks, slices), dim3(NN_BLOCK), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(), src->x(), src->y(),
                               src->z(), (uint32_t)ns, n_tiles, tps, ctx->keys, merge_atomic, ctx->stop_flag_dev);
        else
            hipLaunchKernelGGL((nn1_ftrack_kernel<QPL, 16>), dim3(qblocks, slices), dim3(NN_BLOCK), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(), src->x(), src->y(),
                               src->z(), (uint32_t)ns, n_tiles, tps, ctx->keys, merge_atomic, ctx->stop_flag_dev, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

int launch_nn1_brute(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool in_loop)
{
    const size_t ns = src->n;
    if (ns == 0) { ctx->keys_n = 0; return PCR_OK; }
    if (ns > 0xFFFFFFF0ull || tgt->n > 0xFFFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "cloud too large for u32 indices");
    // keys[] still holds this source's correspondences of the previous ICP iteration?
    const bool warm = in_loop && ctx->keys_warm && (ctx->keys_src == src->id || ctx->keys_tgt == tgt->id) && ctx->keys_warm_n == ns &&
                      tune_get(ctx, "nn1_warm_start", 1) == 1;
    // ... and the move of the previous iteration already turned them into this search's seeds (kabsch.hip seed_next_search)?
    const bool pre_seeded = warm && ctx->keys_seeded && ctx->keys_seed_src == src->id && ctx->keys_seed_tgt == tgt->id && ctx->keys_n == ns;
    ctx->keys_seeded = false;
    ctx->nn1_move_l0 = 0; ctx->nn1_moved = false;      // (set by launch_matrix alone: every other family leaves "no")
    int rc = ensure_keys(ctx, ns);
    if (rc) return rc;
    ctx->keys_n = ns;
    ctx->wpos_valid = false;              // keys[] is about to be rewritten without record positions
    ctx->keys_warm = in_loop;
    ctx->keys_warm_n = ns;
    keys_record(ctx, tgt, src);

    const int64_t variant = tune_get(ctx, "nn1_variant", 0), bf16_tune = tune_get(ctx, "nn1_bf16", 0), f16_tune = tune_get(ctx, "nn1_f16", 0);
    // The matrix-core forms, from a target's FIRST search on: the index (operands in Morton order, bt_ensure) costs one bounding-box
    // round trip and ~0.2 ms at 120 k points, less than the kernel saves (small targets stay on the f32 filters: 44 against 53 us per
    // ICP iteration at 4 000 points, 114 against 72 at 20 000 — profiles/r02_mfma_filter_experiments.txt)
    if (variant == 6 || variant == 7 || variant == 8 || variant == 9 || variant == 10 || (variant == 0 && bf16_tune != 2 && (bf16_tune == 1 || (NN_BF16_DEFAULT && tgt->n >= 8192)))) {
        rc = bt_ensure(ctx, tgt);
        if (rc) return rc;
        if (tgt->bt->safe && tgt->bt->n_tiles) {
            // HTRACK: one f16 MFMA per tile instead of two bf16 ones, when the cloud fits f16's range (the flag of the operand build, read once)
            bool f16 = variant == 7 || variant == 8 || variant == 9 || variant == 10 || (variant == 0 && f16_tune != 2 && (f16_tune == 1 || NN_F16_DEFAULT));
            if (f16 && tgt->bt->bad16_host < 0) {
                int flag = 1;
                PCR_HIP(ctx, hipMemcpyAsync(&flag, tgt->bt->bad16, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
                PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
                tgt->bt->bad16_host = flag;
            }
            if (f16 && tgt->bt->bad16_host != 0) f16 = false;
            // The bounds of both forms assume how the matrix pipe accumulates (header of nn1_btrack_kernel) — measured ON THIS DEVICE before
            // either is first chosen (mfma_verdict: once per context, cached): a form whose measured error exceeds half of what its bound
            // budgets is not used here; the f32 filters below (bounds from IEEE arithmetic alone) answer instead.
            if (f16 && !mfma_verdict(ctx, true)) f16 = false;
            if (f16 || mfma_verdict(ctx, false)) return launch_matrix(ctx, tgt, src, f16, warm, pre_seeded, f16 && (variant == 8 || variant == 9 || variant == 10));
        }
    }
    // ETRACK needs the cell index (chunked, centred copy of the target): cold searches take it when that index exists or will be needed
    // anyway (inside an ICP loop), or on a target's second search; its FIRST one-shot search stays on FTRACK, which needs no index at all
    const bool reused = tgt->grid == nullptr && tgt->brute_searches++ >= 1;
    if (variant == 4 || (variant == 0 && tgt->n >= 2048 && (warm || in_loop || tgt->grid || reused))) {
        rc = build_target_grid(ctx, tgt);
        if (rc) return rc;
        if (tgt->grid->chunk_safe && tgt->grid->n_chunks) return launch_etrack(ctx, tgt, src, warm, pre_seeded);
        // (non-finite or astronomically large coordinates: the kernels below handle them)
    }
    return launch_plain(ctx, tgt, src, variant == 2);
}


// exhaustive search of the listed queries only (count on the device, at most qcap), merged into keys[] (grid.hip hands its far
// queries over: one tiled pass over the target per ~512 of them instead of a cube walk to a neighbour tens of metres away)
int launch_nn1_brute_list(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, const uint32_t* qlist, const uint32_t* qcount, uint32_t qcap)
{
    if (qcap == 0 || tgt->n == 0) return PCR_OK;
    constexpr int Q = 2;
    const uint32_t n_tiles = (uint32_t)((tgt->n + NN_TILE - 1) / NN_TILE);
    const uint32_t qblocks = (qcap + NN_BLOCK * Q - 1) / (NN_BLOCK * Q);
    // few query blocks: slice the target so that the listed queries still fill the chip
    uint32_t slices = std::max<uint32_t>(1u, std::min<uint32_t>(n_tiles, 2048u / std::max<uint32_t>(1u, std::min<uint32_t>(qblocks, 2048u))));
    uint32_t tps = (n_tiles + slices - 1) / slices;
    slices = (n_tiles + tps - 1) / tps;
    hipLaunchKernelGGL((nn1_ftrack_kernel<Q, 16>), dim3(qblocks, slices), dim3(NN_BLOCK), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(),
                       src->x(), src->y(), src->z(), (uint32_t)src->n, n_tiles, tps, ctx->keys, 1, ctx->stop_flag_dev, qlist, qcount, qcap);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// ---- self-tests of the matrix-pipe arithmetic the bounds of BTRACK / HTRACK rest on (pcr_selftest_mfma_bf16 / _f16, and — a short form of
// the same, once per context — mfma_verdict below, which the dispatcher consults before it first picks either kernel).  One wave per tile
// runs the kernel's own MFMA(s); the host compares every accumulator with the exact value in f64.  Tiles, in this order:
//   [0, trials)         RAW random operands, exponents spread over the type's usable range in every K-slot            -> worst[0]
//   4 RAW structured    cancellation across K-slots (x y - x y', y' the neighbour of y), alternating signs on geometrically falling
//                       magnitudes, subnormal / smallest pieces against large ones, maximal exponent spread inside one instruction -> worst[3]
//   trials KERNEL       the kernel's own operand construction for random r, t'' of the magnitudes a search produces    -> worst[1]
//   8 KERNEL            the same where f16 underflows: |r|, |t''| both in 2^-20 .. 2^-3 (also r == t'': a query ON a target), and the
//                       two mixed cases (one side small, the other large)                                              -> worst[1], worst[2]
// worst[0], worst[3] = max |D - exact| / (u sum |a b|);  worst[1] = max (|G - want| - 2 u) / (u (Q + W)) over every KERNEL tile (2 u: the half
// of the absolute slack the verdict grants);  worst[2] = max |G - want| / u over the pairs with Q + W <= 2^-6;  u = 2^-24, want = w - 2 r.t''.
namespace {
struct SelfRng {                                              // splitmix64: the same stream on every host
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }                    // [0, 1)
    float sym(float a) { return (float)((uni() * 2.0 - 1.0) * a); }
    int range(int lo, int hi) { return lo + (int)(next() % (uint64_t)(hi - lo + 1)); }               // inclusive
};
// number formats of the two pipes: P significant bits, normal exponents [emin, emax], subnormal spacing 2^(emin - P + 1)
struct Fmt { int P, emin, emax; bool f16; };
constexpr Fmt FMT_F16 = { 11, -14, 15, true }, FMT_BF16 = { 8, -126, 127, false };
inline double fmt_decode(const Fmt& f, uint32_t b)
{
    if (!f.f16) { const uint32_t u = b << 16; float v; std::memcpy(&v, &u, 4); return (double)v; }
    const int e = (int)((b >> 10) & 31); const double m = (double)(b & 1023);
    const double v = e == 0 ? std::ldexp(m, -24) : std::ldexp(1024.0 + m, e - 25);
    return (b & 0x8000u) ? -v : v;
}
inline uint32_t fmt_encode(const Fmt& f, double v)            // v exactly representable (the generators below make no other values)
{
    if (!f.f16) { const float x = (float)v; uint32_t u; std::memcpy(&u, &x, 4); return u >> 16; }
    const uint32_t sg = std::signbit(v) ? 0x8000u : 0u;
    const double a = std::fabs(v);
    if (a == 0.0) return sg;
    int e; const double m = std::frexp(a, &e);                 // a = m 2^e, m in [0.5, 1)
    if (e - 1 < -14) return sg | (uint32_t)std::ldexp(a, 24);  // subnormal: multiples of 2^-24
    return sg | ((uint32_t)(e - 1 + 15) << 10) | ((uint32_t)std::ldexp(m, 11) & 1023u);
}
// a random value with P significant bits and exponent e (normal), or a subnormal / smallest-binade one (sub)
inline double fmt_rand(const Fmt& f, SelfRng& r, int e, bool sub = false)
{
    const double sg = (r.next() & 1) ? -1.0 : 1.0;
    if (sub) return sg * std::ldexp((double)r.range(1, (1 << (f.P - 1)) - 1), f.emin - f.P + 1);
    return sg * std::ldexp((double)((1 << (f.P - 1)) + r.range(0, (1 << (f.P - 1)) - 1)), e - f.P + 1);
}
// RAW tile: A[32 rows][K], B[K][32 columns] as doubles (exactly representable); K = 16 (one f16 MFMA) or 32 (two bf16 MFMAs)
inline void raw_tile(const Fmt& f, SelfRng& r, int kind, int K, std::vector<double>& A, std::vector<double>& B, int spread)
{
    A.assign(32 * K, 0.0); B.assign(K * 32, 0.0);
    const int hi = f.f16 ? 15 : 58, lo = f.f16 ? -14 : -58;   // bf16: products stay far inside f32's range
    for (int i = 0; i < 32; i++)
        for (int k = 0; k < K; k++) {
            double a = 0.0, b = 0.0;
            switch (kind) {
            case 0: a = fmt_rand(f, r, r.range(-spread, spread)); b = fmt_rand(f, r, r.range(-spread, spread)); break;      // random
            case 1:                                                                                                          // cancellation
                if (k & 1) { a = A[i * K + k - 1]; const double y = B[(k - 1) * 32 + i]; b = -(y + std::copysign(std::ldexp(1.0, (int)std::floor(std::log2(std::fabs(y))) - f.P + 1), y)); }
                else { a = fmt_rand(f, r, r.range(-2, 2)); b = fmt_rand(f, r, r.range(-2, 2)); }
                break;
            case 2: a = std::fabs(fmt_rand(f, r, 6 - (k % 16))); b = ((k & 1) ? -1.0 : 1.0) * std::fabs(fmt_rand(f, r, k % 3)); break;   // alternating signs
            case 3:                                                                                                          // subnormal / smallest pieces
                a = (k & 1) ? fmt_rand(f, r, r.range(lo, lo + 4)) : (f.f16 ? fmt_rand(f, r, 0, true) : fmt_rand(f, r, -100));
                b = fmt_rand(f, r, r.range(0, 10));
                break;
            default:                                                                                                         // exponent spread
                if (k == 0) { a = fmt_rand(f, r, hi); b = fmt_rand(f, r, hi); }
                else if (k == 1) { a = f.f16 ? std::ldexp(1.0, -24) : fmt_rand(f, r, lo); b = f.f16 ? -std::ldexp(1.0, -24) : fmt_rand(f, r, lo); }
                else { a = fmt_rand(f, r, r.range(lo, hi)); b = fmt_rand(f, r, r.range(lo, hi)); }
                break;
            }
            A[i * K + k] = a; B[k * 32 + i] = b;
        }
}
// (r, t'') of one KERNEL tile: regime 0 = search magnitudes, 1 = both small, 2 = both small and r == t'', 3 = r small / t'' large, 4 = r large / t'' small
inline void kernel_tile(SelfRng& r, int regime, bool f16, float* q /* 32 x 3 */, float* t /* 32 x 3 */)
{
    const float big_r = std::ldexp(1.0f, f16 ? r.range(0, 14) : r.range(-2, 6)), big_t = std::ldexp(1.0f, f16 ? r.range(0, 7) : r.range(-3, 2));
    const float cap_r = f16 ? 32000.0f : 3e38f, cap_t = f16 ? 0.57f : 1.0f;                     // f16: |t''| <= 2^7 in norm terms too (w < 65000)
    auto small = [&]() { return r.sym(1.0f) * std::ldexp(1.0f, -r.range(3, 20)); };
    for (int i = 0; i < 32; i++)
        for (int c = 0; c < 3; c++) {
            const float rl = std::min(std::max(r.sym(1.95f) * big_r, -cap_r), cap_r), tl = r.sym(1.0f) * big_t * cap_t;
            float rv = rl, tv = tl;
            if (regime == 1 || regime == 2) { rv = small(); tv = small(); }
            else if (regime == 3) rv = small();
            else if (regime == 4) tv = small();
            q[i * 3 + c] = rv; t[i * 3 + c] = regime == 2 ? rv : tv;
        }
}
constexpr int SELF_STRUCT = 4, SELF_EDGE = 8;
inline void score(double got, double want, double Q, double W, double worst[4])
{
    const double err = std::fabs(got - want) * 16777216.0;    // in u
    if (Q + W > 0.0) worst[1] = std::max(worst[1], (err - 2.0) / (Q + W));
    if (Q + W <= 0.015625) worst[2] = std::max(worst[2], err);
}
}  // namespace

__global__ __launch_bounds__(64) void bt_selftest_kernel(const uint4* __restrict__ ops, float* __restrict__ out)
{
    const uint32_t lane = threadIdx.x, T = blockIdx.x;
    const uint4 A0 = ops[(size_t)T * 256 + lane], B0 = ops[(size_t)T * 256 + 64 + lane], A1 = ops[(size_t)T * 256 + 128 + lane], B1 = ops[(size_t)T * 256 + 192 + lane];
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A0), __builtin_bit_cast(bf16x8, B0), zero, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1), __builtin_bit_cast(bf16x8, B1), acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) out[((size_t)T * 64 + lane) * 16 + j] = acc[j];
}

// tiles < n_raw run the MFMA on operands the host built (f16 bit patterns); the others get f32 query offsets and target offsets (already
// scaled) and build their operands with the kernel's own device code
__global__ __launch_bounds__(64) void ht_selftest_kernel(const uint4* __restrict__ ab, const float* __restrict__ rt, uint32_t n_raw, float* __restrict__ out)
{
    const uint32_t lane = threadIdx.x, T = blockIdx.x, n = lane & 31;
    const bool h = lane >= 32;
    uint4 A, B;
    if (T < n_raw) { A = ab[(size_t)T * 128 + lane]; B = ab[(size_t)T * 128 + 64 + lane]; }
    else {
        const float* q = rt + ((size_t)T * 64 + n) * 3;                    // query n
        const float* t = rt + ((size_t)T * 64 + 32 + n) * 3;               // target row n (= lane & 31)
        uint32_t f1, f2, s1, s2;
        ht_pair(h ? q[2] : q[0], f1, f2);
        ht_pair(q[1], s1, s2);
        B = make_uint4(f1, f2, h ? 0x3C003C00u : s1, h ? 0u : s2);
        A = ht_target_operand(t[0], t[1], t[2], true, h);
    }
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), zero, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) out[((size_t)T * 64 + lane) * 16 + j] = acc[j];
}

// device buffers of a self-test: the context's scratch and pinned stage (no allocation in the common case — the verdict runs inside a search)
static int selftest_run(pcr_ctx* ctx, const void* h_in, size_t in_bytes, size_t out_bytes, float** h_out, void** d_in, float** d_out)
{
    void* h_stage;
    Layout Ld, Lh;                                             // the same two slots on the device and in the pinned stage
    Ld.add(d_in, in_bytes);
    Ld.add((void**)d_out, out_bytes);
    Lh.add(&h_stage, in_bytes);
    Lh.add((void**)h_out, out_bytes);
    int rc = bind_scratch(ctx, Ld);
    if (rc) return rc;
    rc = ensure_stage(ctx, Lh.bytes());
    if (rc) return rc;
    Lh.bind(ctx->host_stage);
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));           // the staging buffer may still be in flight
    std::memcpy(h_stage, h_in, in_bytes);
    PCR_HIP(ctx, hipMemcpyAsync(*d_in, h_stage, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    return PCR_OK;
}

int bt_mfma_selftest(pcr_ctx* ctx, int trials, double worst[4])
{
    worst[0] = worst[1] = worst[2] = worst[3] = 0.0;
    if (trials <= 0) return PCR_OK;
    const Fmt& F = FMT_BF16;
    const size_t n_raw = (size_t)trials + SELF_STRUCT, n_tiles = n_raw + (size_t)trials + SELF_EDGE;
    std::vector<uint32_t> h(n_tiles * 256 * 4, 0u);
    std::vector<double> dec(n_tiles * 4 * 64 * 8);             // every operand element decoded once: [tile][A0, B0, A1, B1][lane][j]
    std::vector<float> rv(n_tiles * 32 * 3), tv(n_tiles * 32 * 3);
    SelfRng rng{ 0x5EEDF00Dull };
    auto put = [&](size_t T, int which, int lane, int j, uint32_t bf) {          // element j (0..7) of operand `which` (A0, B0, A1, B1) of a lane
        uint32_t& w = h[((T * 4 + which) * 64 + lane) * 4 + j / 2];
        w = (j & 1) ? ((w & 0x0000FFFFu) | (bf << 16)) : ((w & 0xFFFF0000u) | bf);
        dec[((T * 4 + which) * 64 + lane) * 8 + j] = fmt_decode(F, bf);
    };
    std::vector<double> A, B;
    for (size_t T = 0; T < n_raw; T++) {                                         // RAW: K index = 16 ins + 8 hh + j
        raw_tile(F, rng, T < (size_t)trials ? 0 : 1 + (int)(T - trials), 32, A, B, 20);
        for (int i = 0; i < 32; i++)
            for (int k = 0; k < 32; k++) {
                put(T, 2 * (k >> 4), i + 32 * ((k >> 3) & 1), k & 7, fmt_encode(F, A[i * 32 + k]));
                put(T, 2 * (k >> 4) + 1, i + 32 * ((k >> 3) & 1), k & 7, fmt_encode(F, B[k * 32 + i]));
            }
    }
    auto split3 = [](float v, uint32_t (&p)[3]) {
        uint32_t u; std::memcpy(&u, &v, 4);
        const uint32_t a = u & 0xFFFF0000u; float fa; std::memcpy(&fa, &a, 4);
        const float d = v - fa; uint32_t ud; std::memcpy(&ud, &d, 4);
        const uint32_t b = ud & 0xFFFF0000u; float fb; std::memcpy(&fb, &b, 4);
        const float e = d - fb; uint32_t ue; std::memcpy(&ue, &e, 4);
        p[0] = a >> 16; p[1] = b >> 16; p[2] = ue >> 16;
    };
    for (size_t T = n_raw; T < n_tiles; T++) {                                   // KERNEL: rows = targets, columns = queries
        const int regime = T < n_raw + (size_t)trials ? 0 : 1 + (int)((T - n_raw - trials) % 4);
        kernel_tile(rng, regime, false, &rv[T * 96], &tv[T * 96]);
        for (int m = 0; m < 32; m++) {
            uint32_t t[3][3], w[3];
            const float* tt = &tv[(T * 32 + m) * 3];
            for (int c = 0; c < 3; c++) split3(-2.0f * tt[c], t[c]);
            split3((tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2], w);
            const int sel[8] = { 0, 1, 0, 2, 1, 0, 2, 1 };                                            // [t1, t2, t1, t3, t2, t1, t3, t2]
            for (int j = 0; j < 8; j++) { put(T, 0, m, j, t[0][sel[j]]); put(T, 0, 32 + m, j, t[1][sel[j]]); put(T, 2, m, j, t[2][sel[j]]); }
            const uint32_t wl[8] = { w[0], w[1], 0, w[2], 0, 0, 0, 0 };
            for (int j = 0; j < 8; j++) put(T, 2, 32 + m, j, wl[j]);
        }
        for (int n = 0; n < 32; n++) {
            uint32_t r[3][3], one[3];
            for (int c = 0; c < 3; c++) split3(rv[(T * 32 + n) * 3 + c], r[c]);
            split3(1.0f, one);
            const int sel[8] = { 0, 0, 1, 0, 1, 2, 1, 2 };                                            // [r1, r1, r2, r1, r2, r3, r2, r3]
            for (int j = 0; j < 8; j++) { put(T, 1, n, j, r[0][sel[j]]); put(T, 1, 32 + n, j, r[1][sel[j]]); put(T, 3, n, j, r[2][sel[j]]); put(T, 3, 32 + n, j, one[sel[j]]); }
        }
    }
    float* out = nullptr; void* d_in = nullptr; float* d_out = nullptr;
    const size_t out_bytes = n_tiles * 64 * 16 * sizeof(float);
    int rc = selftest_run(ctx, h.data(), h.size() * 4, out_bytes, &out, &d_in, &d_out);
    if (rc) return rc;
    hipLaunchKernelGGL(bt_selftest_kernel, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, (const uint4*)d_in, d_out);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t T = 0; T < n_tiles; T++)
        for (int lane = 0; lane < 64; lane++)
            for (int reg = 0; reg < 16; reg++) {
                const int n = lane & 31, m = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                const double got = (double)out[(T * 64 + lane) * 16 + reg];
                if (T < n_raw) {
                    double ex = 0.0, mag = 0.0;
                    for (int ins = 0; ins < 2; ins++)
                        for (int hh = 0; hh < 2; hh++) {
                            const double* a = &dec[((T * 4 + 2 * ins) * 64 + m + 32 * hh) * 8];
                            const double* b = &dec[((T * 4 + 2 * ins + 1) * 64 + n + 32 * hh) * 8];
                            for (int j = 0; j < 8; j++) { const double p = a[j] * b[j]; ex += p; mag += std::fabs(p); }
                        }
                    double& w = worst[T < (size_t)trials ? 0 : 3];
                    if (mag > 0.0) w = std::max(w, std::fabs(got - ex) / mag * 16777216.0);
                } else {
                    const float* r = &rv[(T * 32 + n) * 3]; const float* t = &tv[(T * 32 + m) * 3];
                    const double Q = (double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2], W = (double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2];
                    const float wf = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
                    score(got, (double)wf - 2.0 * ((double)r[0] * t[0] + (double)r[1] * t[1] + (double)r[2] * t[2]), Q, W, worst);
                }
            }
    return PCR_OK;
}

int ht_mfma_selftest(pcr_ctx* ctx, int trials, double worst[4])
{
    worst[0] = worst[1] = worst[2] = worst[3] = 0.0;
    if (trials <= 0) return PCR_OK;
    const Fmt& F = FMT_F16;
    const size_t n_raw = (size_t)trials + SELF_STRUCT, n_tiles = n_raw + (size_t)trials + SELF_EDGE;
    // one upload: [n_raw][A, B][64 lanes] x 16 bytes of f16 patterns, then [n_tiles][64 rows (32 queries, 32 targets)] x 3 floats
    const size_t ab_words = n_raw * 128 * 4, rt_off = al256(ab_words * 4), rt_floats = n_tiles * 64 * 3;
    std::vector<unsigned char> blob(rt_off + rt_floats * 4, 0);
    uint32_t* hab = reinterpret_cast<uint32_t*>(blob.data());
    float* rt = reinterpret_cast<float*>(blob.data() + rt_off);
    std::vector<double> dec(n_raw * 2 * 64 * 8);
    SelfRng rng{ 0xF16F16F1ull };
    auto put = [&](size_t T, int which, int lane, int j, uint32_t b) {
        uint32_t& w = hab[((T * 2 + which) * 64 + lane) * 4 + j / 2];
        w = (j & 1) ? ((w & 0x0000FFFFu) | (b << 16)) : ((w & 0xFFFF0000u) | b);
        dec[((T * 2 + which) * 64 + lane) * 8 + j] = fmt_decode(F, b);
    };
    std::vector<double> A, B;
    for (size_t T = 0; T < n_raw; T++) {                                         // RAW: K index = 8 hh + j
        raw_tile(F, rng, T < (size_t)trials ? 0 : 1 + (int)(T - trials), 16, A, B, 8);
        for (int i = 0; i < 32; i++)
            for (int k = 0; k < 16; k++) { put(T, 0, i + 32 * (k >> 3), k & 7, fmt_encode(F, A[i * 16 + k])); put(T, 1, i + 32 * (k >> 3), k & 7, fmt_encode(F, B[k * 32 + i])); }
    }
    for (size_t T = n_raw; T < n_tiles; T++) {
        const int regime = T < n_raw + (size_t)trials ? 0 : 1 + (int)((T - n_raw - trials) % 4);
        kernel_tile(rng, regime, true, &rt[T * 192], &rt[T * 192 + 96]);
    }
    float* out = nullptr; void* d_in = nullptr; float* d_out = nullptr;
    const size_t out_bytes = n_tiles * 64 * 16 * sizeof(float);
    int rc = selftest_run(ctx, blob.data(), blob.size(), out_bytes, &out, &d_in, &d_out);
    if (rc) return rc;
    hipLaunchKernelGGL(ht_selftest_kernel, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, (const uint4*)d_in, (const float*)((const char*)d_in + rt_off),
                       (uint32_t)n_raw, d_out);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t T = 0; T < n_tiles; T++)
        for (int lane = 0; lane < 64; lane++)
            for (int reg = 0; reg < 16; reg++) {
                const int n = lane & 31, m = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                const double got = (double)out[(T * 64 + lane) * 16 + reg];
                if (T < n_raw) {
                    double ex = 0.0, mag = 0.0;
                    for (int hh = 0; hh < 2; hh++) {
                        const double* a = &dec[((T * 2) * 64 + m + 32 * hh) * 8];
                        const double* b = &dec[((T * 2 + 1) * 64 + n + 32 * hh) * 8];
                        for (int j = 0; j < 8; j++) { const double p = a[j] * b[j]; ex += p; mag += std::fabs(p); }
                    }
                    double& w = worst[T < (size_t)trials ? 0 : 3];
                    if (mag > 0.0) w = std::max(w, std::fabs(got - ex) / mag * 16777216.0);
                } else {
                    const float* r = &rt[(T * 64 + n) * 3]; const float* t = &rt[(T * 64 + 32 + m) * 3];
                    const double Q = (double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2], W = (double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2];
                    const float wf = ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) * 0.99999237060546875f;
                    score(got, (double)wf - 2.0 * ((double)r[0] * t[0] + (double)r[1] * t[1] + (double)r[2] * t[2]), Q, W, worst);
                }
            }
    return PCR_OK;
}

// ---- self-test of STRACK's DECISION (pcr_selftest_sign_f16; a short form is part of the f16 verdict below).  The sign form adds to the
// f16 filter's assumptions nothing but st_theta's rounding — this checks the property the search relies on directly, on the device: for
// random queries / targets of a super-tile (the regimes of kernel_tile, a power-of-two scale per tile) and thresholds placed ON the exact
// distance of one pair, one ulp below and above it, and a factor away, EVERY pair whose A1 distance (f32, unfused, as the exact
// evaluation computes it) lies at or below its query's threshold must come out of the kernel's own operand code + MFMA with its sign set.
// out = { pairs at or below their threshold, of those WITHOUT the sign (must be 0), pairs with the sign set, pairs in all }.
__global__ __launch_bounds__(64) void st_selftest_kernel(const float* __restrict__ rt, const float* __restrict__ thr, const float* __restrict__ scale, float* __restrict__ out)
{
    const uint32_t lane = threadIdx.x, T = blockIdx.x, n = lane & 31;
    const bool h = lane >= 32;
    const float sc = scale[T];
    const float* q = rt + ((size_t)T * 64 + n) * 3;                        // query n (cloud units)
    const float* t = rt + ((size_t)T * 64 + 32 + n) * 3;                   // target row n (cloud units)
    uint32_t P[4], Q[4];
    st_setup(q[0], q[1], q[2], make_float4(0.0f, 0.0f, 0.0f, sc), thr[(size_t)T * 32 + n], sc * sc, P, Q);
    const uint4 B = h ? make_uint4(Q[0], Q[1], Q[2], Q[3]) : make_uint4(P[0], P[1], P[2], P[3]);
    const uint4 A = ht_target_operand(t[0] * sc, t[1] * sc, t[2] * sc, true, h);          // (exact scaling)
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), zero, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) out[((size_t)T * 64 + lane) * 16 + j] = acc[j];
}

int st_sign_selftest(pcr_ctx* ctx, int trials, unsigned long long res[4])
{
    res[0] = res[1] = res[2] = res[3] = 0;
    if (trials <= 0) return PCR_OK;
    const size_t n_tiles = (size_t)trials + SELF_EDGE;
    // one upload: [n_tiles][64 rows (32 queries, 32 targets)] x 3 floats, [n_tiles][32] thresholds, [n_tiles] scales
    const size_t rt_floats = n_tiles * 192, thr_off = rt_floats, sc_off = thr_off + n_tiles * 32, in_floats = sc_off + n_tiles;
    std::vector<float> in(in_floats, 0.0f);
    SelfRng rng{ 0x5160F16Full };
    auto a1 = [](const float* a, const float* b) { const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2]; return (dx * dx + dy * dy) + dz * dz; };
    for (size_t T = 0; T < n_tiles; T++) {
        const int regime = T < (size_t)trials ? 0 : 1 + (int)((T - trials) % 4);
        float* q = &in[T * 192]; float* t = &in[T * 192 + 96];
        kernel_tile(rng, regime, true, q, t);                              // scaled units ...
        const float sc = std::ldexp(1.0f, rng.range(-8, 8)), inv = 1.0f / sc;
        for (int i = 0; i < 192; i++) in[T * 192 + i] *= inv;              // ... -> cloud units (exact)
        in[sc_off + T] = sc;
        for (int n = 0; n < 32; n++) {
            const float d = a1(&q[n * 3], &t[((n * 7 + (int)T) % 32) * 3]);
            float th = d;
            switch (n % 4) {
            case 1: th = std::nextafter(d, 0.0f); break;
            case 2: th = std::nextafter(d, 3.0e38f); break;
            case 3: th = d * std::ldexp(1.0f, rng.range(-2, 2)) * (1.0f + (float)rng.uni()); break;
            default: break;
            }
            in[thr_off + T * 32 + n] = th;
        }
    }
    float* out = nullptr; void* d_in = nullptr; float* d_out = nullptr;
    const size_t out_bytes = n_tiles * 64 * 16 * sizeof(float);
    int rc = selftest_run(ctx, in.data(), in.size() * sizeof(float), out_bytes, &out, &d_in, &d_out);
    if (rc) return rc;
    const float* df = (const float*)d_in;
    hipLaunchKernelGGL(st_selftest_kernel, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, df, df + thr_off, df + sc_off, d_out);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t T = 0; T < n_tiles; T++)
        for (int lane = 0; lane < 64; lane++)
            for (int reg = 0; reg < 16; reg++) {
                const int n = lane & 31, m = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                uint32_t bits; std::memcpy(&bits, &out[(T * 64 + lane) * 16 + reg], 4);
                const bool flagged = (bits >> 31) != 0;
                const float d = a1(&in[(T * 64 + n) * 3], &in[(T * 64 + 32 + m) * 3]);
                const bool must = d <= in[thr_off + T * 32 + n];
                res[0] += must; res[1] += must && !flagged; res[2] += flagged; res[3] += 1;
            }
    return PCR_OK;
}

// ---- self-test of the SPHERE statement of STRACK3 (pcr_selftest_sphere_f16; a short form is part of the f16 verdict below): random level-1
// tiles — 32 chunks of 16 records in the scaled range of a level-1 super-tile: tight clusters, wide ones, chunks spread beyond 2^7 (the
// whole-super-tile sphere), chunks without a finite record, records on the edge of the range — through the index build's own operand code
// (l1_chunk_operand), the kernel's query code (st_setup_l1) and the MFMA, a power-of-two scale per tile; queries near a chunk, inside one, far
// away, at the clamp; thresholds ON the exact A1 distance to some record, one ulp below / above it, a factor away, zero.  EVERY (query,
// chunk) pair with a record whose A1 distance is at or below the query's threshold must come out with its sign set.
// out = { such pairs, of those WITHOUT the sign (must be 0), pairs with the sign set, pairs in all }.
__global__ __launch_bounds__(64) void sp_selftest_kernel(const float* __restrict__ rec, const float* __restrict__ qs, const float* __restrict__ thr, const float* __restrict__ scale,
                                                         float* __restrict__ out)
{
    const uint32_t lane = threadIdx.x, T = blockIdx.x, n = lane & 31;
    const bool h = lane >= 32;
    const float sc = scale[T];
    // the product in the role STRACK3 uses (nn1_strack3_body, TR): queries as A, sphere rows as B.  Lane n builds chunk n's row and query n's operand.
    const uint32_t chunk = n;
    float tx[16], ty[16], tz[16];
    bool fin[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const float* r = rec + (((size_t)T * 32 + chunk) * 16 + j) * 3;    // cloud units; the level-1 centre is the origin
        tx[j] = r[0] * sc; ty[j] = r[1] * sc; tz[j] = r[2] * sc;
        fin[j] = fabsf(r[0]) <= 3.0e38f && fabsf(r[1]) <= 3.0e38f && fabsf(r[2]) <= 3.0e38f && fabsf(tx[j]) <= 128.0f && fabsf(ty[j]) <= 128.0f && fabsf(tz[j]) <= 128.0f;
    }
    uint4 lo, hi;
    l1_chunk_operand(tx, ty, tz, fin, lo, hi);
    const uint4 B = h ? hi : lo;
    const float* q = qs + ((size_t)T * 32 + n) * 3;
    uint32_t P[4], Q[4];
    st_setup_l1(q[0], q[1], q[2], make_float4(0.0f, 0.0f, 0.0f, sc), thr[(size_t)T * 32 + n], sc * sc, P, Q);
    const uint4 A = h ? make_uint4(Q[0], Q[1], Q[2], Q[3]) : make_uint4(P[0], P[1], P[2], P[3]);
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), zero, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) out[((size_t)T * 64 + lane) * 16 + j] = acc[j];
}

int st_sphere_selftest(pcr_ctx* ctx, int trials, unsigned long long res[4])
{
    res[0] = res[1] = res[2] = res[3] = 0;
    if (trials <= 0) return PCR_OK;
    const size_t n_tiles = (size_t)trials;
    // one upload: [n_tiles][32 chunks][16 records] x 3 floats | [n_tiles][32 queries] x 3 | [n_tiles][32] thresholds | [n_tiles] scales
    const size_t rec_floats = n_tiles * 32 * 16 * 3, q_off = rec_floats, thr_off = q_off + n_tiles * 96, sc_off = thr_off + n_tiles * 32, in_floats = sc_off + n_tiles;
    std::vector<float> in(in_floats, 0.0f);
    SelfRng rng{ 0x5B4E2E16Full };
    auto a1 = [](const float* a, const float* b) { const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2]; return (dx * dx + dy * dy) + dz * dz; };
    for (size_t T = 0; T < n_tiles; T++) {
        const float sc = std::ldexp(1.0f, rng.range(-8, 8)), inv = 1.0f / sc;
        in[sc_off + T] = sc;
        float* rec = &in[T * 32 * 16 * 3];
        for (int c = 0; c < 32; c++) {
            // scaled units, |.| <= 128: a cluster of radius 2^-12 .. 2^6 around a centre in the box (clipped to it), now and then spread over
            // the whole box, on its faces, or empty
            const int kind = (int)(rng.uni() * 16.0);
            const float rad = kind == 0 ? 250.0f : std::ldexp(1.0f, rng.range(-12, 6));
            float cen[3];
            for (int k = 0; k < 3; k++) cen[k] = rng.sym(120.0f);
            for (int j = 0; j < 16; j++)
                for (int k = 0; k < 3; k++) {
                    float v = cen[k] + rng.sym(1.0f) * rad;
                    v = std::min(std::max(v, -128.0f), 128.0f);
                    if (kind == 1 && j < 4) v = (rng.uni() < 0.5 ? -128.0f : 128.0f);
                    if (kind == 2) v = std::numeric_limits<float>::quiet_NaN();                     // an empty chunk
                    if (kind == 3 && j == 5) v = std::numeric_limits<float>::infinity();            // one non-finite record among finite ones
                    rec[(c * 16 + j) * 3 + k] = v * inv;                                              // -> cloud units (exact)
                }
        }
        float* q = &in[q_off + T * 96];
        for (int n = 0; n < 32; n++) {
            const int kind = (int)(rng.uni() * 8.0);
            const int c = (int)(rng.uni() * 32.0) % 32, j = (int)(rng.uni() * 16.0) % 16;
            const float* near = &rec[(c * 16 + j) * 3];
            for (int k = 0; k < 3; k++) {
                float v;
                if (kind <= 3) v = (std::isfinite(near[k]) ? near[k] * sc : 0.0f) + rng.sym(1.0f) * std::ldexp(1.0f, rng.range(-10, 5));     // near a record
                else if (kind == 4) v = rng.sym(128.0f);                                                                             // somewhere in the box
                else if (kind == 5) v = rng.sym(1.0f) * std::ldexp(1.0f, rng.range(7, 14));                                           // outside, up to the clamp
                else if (kind == 6) v = rng.sym(40000.0f);                                                                            // beyond the clamp
                else v = std::isfinite(near[k]) ? near[k] * sc : 0.0f;                                                                  // ON a record
                q[n * 3 + k] = v * inv;
            }
            // threshold: the exact A1 distance to a record of some chunk (finite ones only), displaced
            const int c2 = (n * 5 + (int)T) % 32, j2 = (n * 3) % 16;
            const float* tr = &rec[(c2 * 16 + j2) * 3];
            float d = (std::isfinite(tr[0]) && std::isfinite(tr[1]) && std::isfinite(tr[2])) ? a1(&q[n * 3], tr) : 1.0f * inv * inv;
            if (!(d < 3.0e38f)) d = 3.0e38f;
            float th = d;
            switch (n % 6) {
            case 1: th = std::nextafter(d, 0.0f); break;
            case 2: th = std::nextafter(d, 3.0e38f); break;
            case 3: th = d * std::ldexp(1.0f, rng.range(-3, 3)) * (1.0f + (float)rng.uni()); break;
            case 4: th = 0.0f; break;
            default: break;
            }
            in[thr_off + T * 32 + n] = th;
        }
    }
    float* out = nullptr; void* d_in = nullptr; float* d_out = nullptr;
    const size_t out_bytes = n_tiles * 64 * 16 * sizeof(float);
    int rc = selftest_run(ctx, in.data(), in.size() * sizeof(float), out_bytes, &out, &d_in, &d_out);
    if (rc) return rc;
    const float* df = (const float*)d_in;
    hipLaunchKernelGGL(sp_selftest_kernel, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, df, df + q_off, df + thr_off, df + sc_off, d_out);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t T = 0; T < n_tiles; T++)
        for (int lane = 0; lane < 64; lane++)
            for (int reg = 0; reg < 16; reg++) {
                const int chunk = lane & 31, n = 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3);       // lane (c, h): chunk c; its accumulator `reg` <-> query 8 (reg >> 2) + 4 h + (reg & 3)
                uint32_t bits; std::memcpy(&bits, &out[(T * 64 + lane) * 16 + reg], 4);
                const bool flagged = (bits >> 31) != 0;
                const float* q = &in[q_off + (T * 32 + n) * 3];
                const float th = in[thr_off + T * 32 + n];
                bool must = false;
                for (int j = 0; j < 16 && !must; j++) {
                    const float* t = &in[((T * 32 + chunk) * 16 + j) * 3];
                    if (!(std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]))) continue;
                    must = a1(q, t) <= th;
                }
                res[0] += must; res[1] += must && !flagged; res[2] += flagged; res[3] += 1;
            }
    return PCR_OK;
}

// The verdict the dispatcher acts on (launch_nn1_brute): the short form of the self-test above, once per context and form, with HALF of
// every assumed bound as the pass mark — accumulation (random and structured) <= 8 u sum|a b| of the 16 assumed; the whole filter value
// <= 41 u (Q + W) of 82 (f16) / <= 17.1 of 34.2 (bf16); the underflow regime <= 2 u of the 4 u ht_setup subtracts.  A form that fails is
// never chosen on this context: the f16 form falls back to the bf16 one, that to the f32 filters (ETRACK / FTRACK), whose bounds need
// nothing beyond IEEE arithmetic.  tune "mfma_force_fail" (1 = f16, 2 = bf16, 3 = both) forces a failing verdict (tests).
bool mfma_verdict(pcr_ctx* ctx, bool f16)
{
    int& v = f16 ? ctx->mfma_ok16 : ctx->mfma_okbf;
    const int64_t force = tune_get(ctx, "mfma_force_fail", 0);
    if (force > 0 && (force & (f16 ? 1 : 2))) return false;
    if (v >= 0) return v == 1;
    const auto t0 = std::chrono::steady_clock::now();
    double* w = f16 ? ctx->mfma_worst16 : ctx->mfma_worstbf;
    const int rc = f16 ? ht_mfma_selftest(ctx, 2, w) : bt_mfma_selftest(ctx, 2, w);
    bool ok = rc == PCR_OK && w[0] > 0.0 && w[0] <= 8.0 && w[3] <= 8.0 && w[1] <= (f16 ? 41.0 : 17.1) && w[2] <= 2.0;
    if (ok && f16) {
        // ... and the decision of the sign form (STRACK, the default search on this form): no pair at or below its threshold without the sign
        unsigned long long sg[4];
        ok = st_sign_selftest(ctx, 2, sg) == PCR_OK && sg[0] > 0 && sg[1] == 0;
        // ... and the sphere statement of the hierarchical form (STRACK3): no (query, chunk) pair with a record at or below the threshold without it
        if (ok) ok = st_sphere_selftest(ctx, 4, sg) == PCR_OK && sg[0] > 0 && sg[1] == 0;
    }
    v = ok ? 1 : 0;
    ctx->mfma_check_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ok;
}


int nn1_unpack(pcr_ctx* ctx, size_t n, uint32_t* idx_dev, float* d2_dev)
{
    if (n == 0) return PCR_OK;
    hipLaunchKernelGGL(nn1_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->keys, (uint32_t)n, idx_dev, d2_dev);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

}  // namespace pcr

// The visits of STRACK3's scalar walk (nn1_sphere.hpp, S3 SCALAR WALK) over ONE level-0 super-tile, enumerated on the host with the kernel's own index
// functions and loop order: pure host logic for the test that sets it against the list form (tests/test_strack3_scalar_walk.py).  Contract: include/pcr.h
extern "C" int pcr_s3_walk_visits(uint32_t S0, const uint32_t rows[8], const uint16_t tiles[256], uint32_t n_rec, uint32_t* out, size_t cap, size_t* n_out)
{
    using namespace pcr;
    if (!rows || !tiles || !n_out || (!out && cap)) return PCR_ERR_ARG;
    size_t k = 0;
    bool fits = true;
    auto emit = [&](uint32_t kind, uint32_t v) { if (2 * k + 2 <= cap) { out[2 * k] = kind; out[2 * k + 1] = v; } else fits = false; k++; };
    const uint32_t n_l1_tiles = (n_rec + 511u) / 512u, n_l2 = (n_rec + 31u) / 32u;
    uint32_t w0[8];
    for (uint32_t t = 0; t < 8; t++) w0[t] = rows[t] & s3w_valid32((S0 * 8u + t) * 32u, n_l1_tiles);
    unsigned long long m0 = w0[0] | ((unsigned long long)w0[1] << 32), m1 = w0[2] | ((unsigned long long)w0[3] << 32),
                       m2 = w0[4] | ((unsigned long long)w0[5] << 32), m3 = w0[6] | ((unsigned long long)w0[7] << 32);
    for (uint32_t s1b = S0 * 32u; m0 | m1 | m2 | m3; s1b += 8u) {
        unsigned long long cur = m0;
        m0 = m1; m1 = m2; m2 = m3; m3 = 0ull;
        while (cur) {
            uint32_t rm;
            const uint32_t S1 = s1b + s3w_take_run(cur, rm);
            emit(0u, S1);
            unsigned long long tl = 0ull, th = 0ull;
            for (uint32_t u = 0; u < 8; u++) {
                if (!((rm >> u) & 1u)) continue;
                const uint32_t T1 = S1 * 8u + u;
                emit(1u, T1);
                const unsigned long long tm = tiles[T1 - S0 * 256u];
                if (u < 4) tl |= tm << (16 * (u & 3)); else th |= tm << (16 * (u & 3));
            }
            const uint32_t t2b = S1 * 128u;
            tl &= s3w_valid64(t2b, n_l2); th &= s3w_valid64(t2b + 64u, n_l2);
            uint32_t left = (uint32_t)__builtin_popcountll(tl) + (uint32_t)__builtin_popcountll(th), tb = 0u;
            while (left) {
                const uint32_t nb = left < 4u ? left : 4u;
                emit(2u, nb);
                for (uint32_t u = 0; u < nb; u++) emit(3u, t2b + s3w_next(tl, th, tb));
                left -= nb;
            }
        }
    }
    *n_out = k;
    return fits ? PCR_OK : PCR_ERR_ARG;
}
