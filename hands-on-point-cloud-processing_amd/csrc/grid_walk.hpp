// grid_walk.hpp — how a fixed-radius neighbourhood is walked over the cell grid of grid_common.hpp.  The one place that knows it: ISS,
// FPFH, Harris3D, DBSCAN and the radius search walk through RadiusWalk; the k-NN scan and the 1-NN search share its row clip and windows.
//
// The contract.  The host builds the grid with cell edge radius_cell_edge(r), so every neighbour within r of a query lies in the 27-cell
// block around the query's cell.  The block is nine x-rows of three cells; the records of a row are one range sorted by x (grid_build).
// A long row is cut to the x-window [lo, hi] that can still hold a neighbour (clip_row_x); G lanes of a group then stride over what is
// left — the loops stay in the kernels, they differ — and reduce with the shuffles at the end of this file.  Two facts carry every
// radius stage: a neighbour is never clipped out of its row (the windows below), and it always lies inside the block (the cell edge).
#pragma once

#include "grid_common.hpp"

#include <algorithm>

namespace pcr {

// Cell edge of the grid of a radius stage: >= 1.01 r — the margin covers the rounding of the cell coordinate, so that every neighbour
// lies in the 27-cell block — and >= 2e-15: below that, squared f32 distances underflow and a point outside the block could still
// compute s == 0 <= s_max (with h >= 2e-15 every outside point has s >= ~4e-30, in the normal range); it also bounds the cell count for
// r -> 0.  grid_build may only enlarge the cell (cell budget, <= 4001 cells per axis).
inline double radius_cell_edge(double r) { return std::max(r * 1.01, 2e-15); }

// A cell of the grid.  CLAMPED is part of the type: query_cell() gives a cell inside the grid box, cell_of() the cell a point is binned to,
// wherever it lies — and row_range() tests only for the second kind whether the three x cells miss the grid.
template <bool CLAMPED>
struct CellT { int x, y, z; };
struct XWindow { float lo, hi; };

// the cell of a point as the grid bins it, NOT clamped to the grid box (a foreign query may lie outside: RadiusWalk then finds no row)
__device__ __forceinline__ CellT<false> cell_of(const GridParams& g, float x, float y, float z)
{
    return { cell_coord(x, g.lo[0], g.inv_h), cell_coord(y, g.lo[1], g.inv_h), cell_coord(z, g.lo[2], g.inv_h) };
}

// ... clamped: every point of the cloud lies inside the grid box, non-finite ones were binned into cell 0 and never pass a distance
// test (inf - inf = NaN)
__device__ __forceinline__ CellT<true> query_cell(const GridParams& g, const float4& q)
{
    return { min(max(cell_coord(q.x, g.lo[0], g.inv_h), 0), g.n[0] - 1), min(max(cell_coord(q.y, g.lo[1], g.inv_h), 0), g.n[1] - 1),
             min(max(cell_coord(q.z, g.lo[2], g.inv_h), 0), g.n[2] - 1) };
}

// the 9 x-rows of the 27-cell block around cell c: row k -> [begin, end) in records; false (and an empty range) when the row lies outside
// the grid.  x0 > x1 (none of the three x cells lies in the grid) can hold for an unclamped cell only (a clamped one has 0 <= c.x <= n[0] - 1, so
// x0 <= c.x <= x1), and only that kind is tested: the kernels that walk from query_cell() compile to the code they had without the test.
template <bool CLAMPED>
__device__ __forceinline__ bool row_range(const GridParams& g, const uint32_t* __restrict__ cell_start, const CellT<CLAMPED>& c, int k, uint32_t& b,
                                          uint32_t& e)
{
    const int yy = c.y + (k % 3) - 1, zz = c.z + (k / 3) - 1;
    if (yy < 0 || yy >= g.n[1] || zz < 0 || zz >= g.n[2]) { b = e = 0; return false; }
    const int x0 = max(c.x - 1, 0), x1 = min(c.x + 1, g.n[0] - 1);
    if (!CLAMPED && x0 > x1) { b = e = 0; return false; }
    const uint32_t row = (uint32_t)((zz * g.n[1] + yy) * g.n[0]);
    b = cell_start[row + x0];
    e = cell_start[row + x1 + 1];
    return true;
}

// THE row clip.  The records of a row are sorted by x: cut [b, e) to the records with lo <= x <= hi, the only ones that can lie within
// the bound the window was made from.  Two bounded binary searches (32 halvings), skipped on rows of at most MIN_LEN records, where they
// would cost more than they save.  The predicates are false for NaN, which cannot occur inside a row (non-finite points live in the
// extra cell).  [lo, hi] must contain every x the caller can still accept: the windows below.
template <unsigned MIN_LEN>
__device__ __forceinline__ void clip_row_x(const float4* __restrict__ records, uint32_t& b, uint32_t& e, float lo, float hi)
{
    if (e - b <= MIN_LEN) return;
    uint32_t l = b, h = e;                                      // first p with x >= lo
    for (int it = 0; it < 32 && l < h; it++) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (records[mid].x < lo) l = mid + 1; else h = mid;
    }
    const uint32_t nb = l;
    h = e;                                                      // first p >= nb with x > hi
    for (int it = 0; it < 32 && l < h; it++) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (records[mid].x <= hi) l = mid + 1; else h = mid;
    }
    b = nb;
    e = l;
}

// ---- the windows: [lo, hi] around qx that holds every x with |x - qx| <= d, one definition per arithmetic
// f32: d widened by the rounding of qx -+ d (relative to |qx|, not to d).  The radius search calls it with the host's (float)(r 1.00001) + 1e-30.
__device__ __forceinline__ XWindow padded_window(float qx, float d)
{
    const float pad = (fabsf(qx) + d) * 2.4e-7f;
    return { qx - d - pad, qx + d + pad };
}
// from a squared bound (the 1-NN search: the best distance so far)
__device__ __forceinline__ XWindow x_window(float qx, float bound2) { return padded_window(qx, sqrtf(bound2) * 1.00001f); }
// every x whose f32 sum (hw7's, or ((dx dx) + dy dy) + dz dz) can still be <= s_max: |dx|^2 <= s_max (1 + 3 * 2^-24); the floor 1e-18
// covers differences whose squares vanish in f32 (|e| < 3.7e-23 gives s == 0)
__device__ __forceinline__ XWindow radius_window(float qx, float s_max) { return padded_window(qx, sqrtf(fmaxf(s_max, 0.0f)) * 1.00001f + 1e-18f); }
// every x whose f64 sum can still be <= s_max: |dx| > sqrt(s_max) (1 + 1e-5) gives dx * dx > s_max; the pad covers the rounding of
// qx -+ d to f32 (DBSCAN, the k-NN scan)
__device__ __forceinline__ XWindow x_window_f64(double qx, double s_max)
{
    const double d = sqrt(s_max) * 1.00001 + 1e-30;
    return { (float)((qx - d) - (fabs(qx) + d) * 2.4e-7), (float)((qx + d) + (fabs(qx) + d) * 2.4e-7) };
}

// The walk of one query: for (k < 9) { walk.row<MIN_LEN>(k, b, e); ... the kernel's own loop over records[b .. e) ... }.  Everything is
// uniform over the lanes that share the query.
template <bool CLAMPED>
struct RadiusWalk {
    const GridParams& g;
    const uint32_t* cell_start;
    const float4* records;
    const CellT<CLAMPED> c;
    const XWindow w;
    __device__ __forceinline__ RadiusWalk(const GridParams& g_, const uint32_t* cell_start_, const float4* records_, const CellT<CLAMPED>& c_, const XWindow& w_)
        : g(g_), cell_start(cell_start_), records(records_), c(c_), w(w_) {}
    // row k, whole; false: outside the grid
    __device__ __forceinline__ bool range(int k, uint32_t& b, uint32_t& e) const { return row_range(g, cell_start, c, k, b, e); }
    // ... cut to the window (apart for a kernel that shortens the range first: db_union)
    template <unsigned MIN_LEN>
    __device__ __forceinline__ void clip(uint32_t& b, uint32_t& e) const { clip_row_x<MIN_LEN>(records, b, e, w.lo, w.hi); }
    // row k, cut.  A foreign query often has whole rows outside the grid and leaves before the clip's length test (the radius search's
    // shape, which keeps its count kernel a loop over the rows); a clamped cell's rows go straight on, as those kernels always did.
    template <unsigned MIN_LEN>
    __device__ __forceinline__ void row(int k, uint32_t& b, uint32_t& e) const { if (range(k, b, e) || CLAMPED) clip<MIN_LEN>(b, e); }
};

// ---- reductions over the G lanes of a group (G a power of two <= 64): a fixed xor-shuffle tree, every lane gets the result
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v)                    // unsigned, double, long long
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
template <int G, typename T>
__device__ __forceinline__ T group_min(T v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = min(v, (T)__shfl_xor(v, o, G));
    return v;
}
// true when any lane of this lane's group of G raised `flag` (lanes of the group that have left count as not raised)
template <int G>
__device__ __forceinline__ bool group_any(bool flag)
{
    if (G == 1) return flag;
    const unsigned long long b = __ballot(flag);
    const unsigned lane = threadIdx.x & 63u;               // workgroups are one-dimensional
    const unsigned long long m = (G >= 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << (lane & ~(unsigned)(G - 1));
    return (b & m) != 0ull;
}

}  // namespace pcr
