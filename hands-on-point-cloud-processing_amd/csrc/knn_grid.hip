// knn_grid.hip — exact batched k-NN over the uniform grid (next row N1: "k-NN as a service"), and its first consumer,
// per-point PCA normals (Homework1/YuF_KIT-第1章作业/pca_normal.py:89-103).
//
// Arithmetic = the hw2 / FLANN / nanoflann leaf arithmetic at dim 3 in f64:  s = ((dx*dx) + dy*dy) + dz*dz on the f32
// coordinates of the cloud widened to f64 (exactly what the reference does with KITTI / PLY floats, test.hpp:28).
//   SQ = true : order and report s   (FLANN / open3d / nanoflann contract; optional strict cap s < cap_s = hybrid search)
//   SQ = false: order and report d = sqrt(s)   (hw2 contract, kdtree.hpp:341-346)
// Canonical order everywhere: value ascending, then index ascending — the top-k lives in registers with a
// branch-free lexicographic insertion, so the result does not depend on the order in which cells are visited.
//
// One lane per query.  Queries are taken in cell order (the grid records themselves for a self-query, a cell-sorted
// permutation otherwise), so the lanes of a wave walk the same x-rows and their loads coalesce into broadcasts.
// Search = growing cubes of cells around the query; cube r proves the current k-th value v when every point outside it
// is farther: v < ((r - slack) h)^2.  The next radius is the smallest one that can prove the current k-th value
// (or 2 r while fewer than k points have been seen); only the new shell is scanned, rows beyond the k-th ball are
// skipped.  Every loop has an unconditional bound.
#include "grid_walk.hpp"
#include "eig3.hpp"

#include <atomic>
#include <chrono>
#include <cmath>
#include <vector>

namespace pcr {

namespace {

constexpr int KG_BLOCK = 256;
constexpr unsigned KG_CLIP_MIN = 32;    // rows up to this length are scanned whole (one lane per query: the searches pay off early)

template <int K>
struct TopK {
    double v[K];
    int32_t i[K];
};

__device__ __forceinline__ bool lex_less(double va, int32_t ia, double vb, int32_t ib) { return va < vb || (va == vb && ia < ib); }

// The value of an unused list slot (its index is 0x7FFFFFFF).  SQ = false follows hw2's result set (resultSet.hpp:32,69: worstDist starts at
// 1e10 and a candidate is rejected when dist > worstDist): a neighbour at d > 1e10 never enters, one at d == 1e10 does — (1e10, j) is
// lexicographically below the unused slot (1e10, 0x7FFFFFFF), (1e10 + ulp, j) is not.  The same rule as knn_f64_kernel<K, false>.
template <bool SQ>
__device__ __forceinline__ constexpr double unused_value() { return SQ ? INFINITY : 1e10; }

// s-domain bound of a k-th value w: nothing with s above it can enter.  While slots are unused w is unused_value(): no bound yet (the walk keeps
// doubling its cube, rows are not clipped) — in the SQ = false mode that also holds for a full list whose k-th entry sits at exactly 1e10.
template <bool SQ>
__device__ __forceinline__ double kth_bound(double w) { return SQ ? w : (w < 1e10 ? w * w * (1.0 + 1e-12) : INFINITY); }   // sqrt(s) <= w  =>  s <= w*w*(1 + 2^-52 ...)

// precondition: (val, idx) < (t.v[K-1], t.i[K-1]).  Slots are rewritten from the back: slot s keeps its entry when the
// candidate is not better than it, takes its left neighbour when the candidate beats that one too, else the candidate.
template <int K>
__device__ __forceinline__ void topk_insert(TopK<K>& t, double val, int32_t idx)
{
#pragma unroll
    for (int s = K - 1; s >= 0; s--) {
        const bool beats_s = lex_less(val, idx, t.v[s], t.i[s]);
        const bool beats_l = s > 0 ? lex_less(val, idx, t.v[s > 0 ? s - 1 : 0], t.i[s > 0 ? s - 1 : 0]) : false;
        const double nv = !beats_s ? t.v[s] : (beats_l ? t.v[s > 0 ? s - 1 : 0] : val);
        const int32_t ni = !beats_s ? t.i[s] : (beats_l ? t.i[s > 0 ? s - 1 : 0] : idx);
        t.v[s] = nv;
        t.i[s] = ni;
    }
}

template <int K, bool SQ>
__device__ __forceinline__ void scan_cells(const float4* __restrict__ records, uint32_t b, uint32_t e, double qx, double qy, double qz, double cap_s,
                                           TopK<K>& t, double& kth_s)
{
#pragma clang fp contract(off)
    // rows of the index are sorted by x: once a bound is known, a long row shrinks to |x - qx| <= sqrt(bound) (clip_row_x,
    // grid_walk.hpp; a candidate outside cannot pass `s < cap_s && s <= kth_s`: s >= dx*dx up to rounding, margin 1e-5)
    const double lim = fmin(kth_s, cap_s);
    if (e - b > KG_CLIP_MIN && lim < 1e300) {               // (the length once more: no f64 sqrt for a short row)
        const XWindow w = x_window_f64(qx, lim);
        clip_row_x<KG_CLIP_MIN>(records, b, e, w.lo, w.hi);
    }
    for (uint32_t p = b; p < e; p++) {
        const float4 rec = records[p];
        const double dx = (double)rec.x - qx, dy = (double)rec.y - qy, dz = (double)rec.z - qz;   // t - q, kdtree.hpp:343
        const double s = (dx * dx + dy * dy) + dz * dz;
        if (!(s < cap_s) || !(s <= kth_s)) continue;             // kth_s: conservative s-domain bound of the k-th entry
        const int32_t j = (int32_t)__float_as_uint(rec.w);
        const double val = SQ ? s : sqrt(s);
        if (lex_less(val, j, t.v[K - 1], t.i[K - 1])) {
            topk_insert<K>(t, val, j);
            kth_s = kth_bound<SQ>(t.v[K - 1]);
        }
    }
}

// perm == nullptr, direct == 0: query p is grid record p (self-query), row = its original index; perm: query = perm[t] of
// (qx, qy, qz); direct: query t of (qx, qy, qz)
template <int K, bool SQ>
__global__ __launch_bounds__(KG_BLOCK) void knn_grid_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                            const float* __restrict__ qxs, const float* __restrict__ qys, const float* __restrict__ qzs,
                                                            const uint32_t* __restrict__ perm, uint32_t m, int k_out, double cap_s, double empty_val,
                                                            int32_t empty_idx, int32_t* __restrict__ idx_out, double* __restrict__ val_out,
                                                            uint32_t* __restrict__ found_out, int direct)
{
    const uint32_t tq = blockIdx.x * KG_BLOCK + threadIdx.x;
    if (tq >= m) return;
    uint32_t row;
    float fx, fy, fz;
    if (perm) {
        row = perm[tq];
        fx = qxs[row]; fy = qys[row]; fz = qzs[row];
    } else if (direct) {                 // a small batch, searched in the order given (cloud_knn_small)
        row = tq;
        fx = qxs[tq]; fy = qys[tq]; fz = qzs[tq];
    } else {
        const float4 rec = records[tq];
        row = __float_as_uint(rec.w);
        fx = rec.x; fy = rec.y; fz = rec.z;
    }
    TopK<K> t;
#pragma unroll
    for (int s = 0; s < K; s++) { t.v[s] = unused_value<SQ>(); t.i[s] = 0x7FFFFFFF; }
    double kth_s = INFINITY;
    if (finite3(fx, fy, fz)) {
        const double qx = fx, qy = fy, qz = fz;
        const int ux = cell_coord(fx, g.lo[0], g.inv_h), uy = cell_coord(fy, g.lo[1], g.inv_h), uz = cell_coord(fz, g.lo[2], g.inv_h);
        const int r0 = max(max(max(-ux, ux - (g.n[0] - 1)), max(-uy, uy - (g.n[1] - 1))), max(max(-uz, uz - (g.n[2] - 1)), 0));
        int r = max(r0, 1), rp = -1;
        const double h = g.h, slack = g.slack;
        for (int step = 0; step < 40; step++) {
            const int xlo = max(ux - r, 0), xhi = min(ux + r, g.n[0] - 1);
            const int ylo = max(uy - r, 0), yhi = min(uy + r, g.n[1] - 1);
            const int zlo = max(uz - r, 0), zhi = min(uz + r, g.n[2] - 1);
            if (xlo <= xhi && ylo <= yhi && zlo <= zhi) {
                for (int cz = zlo; cz <= zhi; cz++) {
                    const int adz = abs(cz - uz);
                    const double fz2 = fmax((double)adz - 1.0 - slack, 0.0) * h;
                    for (int cy = ylo; cy <= yhi; cy++) {
                        const int ady = abs(cy - uy);
                        const double fy2 = fmax((double)ady - 1.0 - slack, 0.0) * h;
                        const double lim = fmin(kth_s, cap_s);
                        if (fy2 * fy2 + fz2 * fz2 > lim * 1.0001) continue;          // the whole row is outside the k-th ball
                        const uint32_t rowbase = (uint32_t)((cz * g.n[1] + cy) * g.n[0]);
                        if (ady <= rp && adz <= rp) {                                  // crosses the old cube: two end pieces
                            const int lb = min(xhi, ux - rp - 1), ra = max(xlo, ux + rp + 1);
                            if (xlo <= lb) scan_cells<K, SQ>(records, cell_start[rowbase + xlo], cell_start[rowbase + lb + 1], qx, qy, qz, cap_s, t, kth_s);
                            if (ra <= xhi) scan_cells<K, SQ>(records, cell_start[rowbase + ra], cell_start[rowbase + xhi + 1], qx, qy, qz, cap_s, t, kth_s);
                        } else {
                            scan_cells<K, SQ>(records, cell_start[rowbase + xlo], cell_start[rowbase + xhi + 1], qx, qy, qz, cap_s, t, kth_s);
                        }
                    }
                }
            }
            const bool covers = (ux - r <= 0) && (ux + r >= g.n[0] - 1) && (uy - r <= 0) && (uy + r >= g.n[1] - 1) && (uz - r <= 0) && (uz + r >= g.n[2] - 1);
            const double reach = ((double)r - slack) * h;
            const double lim = fmin(kth_s, cap_s);                                     // nothing at or beyond `lim` can enter
            if (covers || lim < reach * reach * 0.99999) break;
            rp = r;
            if (lim < INFINITY) {
                const double need = fmin(sqrt(lim * 1.00002) * (double)g.inv_h + slack + 1.0, 16777216.0);
                r = max((int)need, rp + 1);
            } else {
                r = min(r * 2, 1 << 24);
            }
        }
    }
    uint32_t found = 0;
#pragma unroll
    for (int s = 0; s < K; s++) {
        if (s < k_out) {
            const bool have = t.i[s] != 0x7FFFFFFF;
            found += have;
            idx_out[(size_t)row * k_out + s] = have ? t.i[s] : empty_idx;
            val_out[(size_t)row * k_out + s] = have ? t.v[s] : empty_val;
        }
    }
    if (found_out) found_out[row] = found;
}

// ---- ONE WAVE PER QUERY (round 3): the same search for a handful of queries — the one-question-at-a-time calls of the reference API
// (KDTreeKNNSearch, kdtree.hpp:329; nanoflann findNeighbors, nanoflann.hpp:1222).  With one LANE per query a single call is one lane's
// serial walk (~30 us of a 71 us call); here the 64 lanes stride the records of every opened row (coalesced loads), each keeping its own
// top-k of what it saw; after every cube the lists are merged — k rounds of "smallest head over the wave" — into the exact global
// top-k, which decides termination as in the serial walk (and bounds the next shell).  Every record is seen by exactly one lane and
// every comparison is on (value, index): the result is the canonical one, bit for bit that of knn_grid_kernel.
// Completion is signalled through host memory: results (zero-copy) -> system-scope fence -> the last wave stores `done`; the host polls
// that word instead of paying the interrupt + wake-up of a stream synchronisation.
struct CoopQueries { float x[16], y[16], z[16]; };       // the queries travel as kernel arguments: no read over PCIe in front of the walk

template <int K, bool SQ>
__global__ __launch_bounds__(64) void knn_grid_coop_kernel(const float4* __restrict__ records, const uint32_t* __restrict__ cell_start, GridParams g,
                                                            CoopQueries qs, uint32_t m, int k_out, double cap_s, double empty_val, int32_t empty_idx,
                                                            int32_t* __restrict__ idx_out, double* __restrict__ val_out, uint32_t* __restrict__ done,
                                                            uint32_t done_value, uint32_t* __restrict__ ticket)
{
#pragma clang fp contract(off)
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    if (row >= m) return;
    const float fx = qs.x[row], fy = qs.y[row], fz = qs.z[row];
    TopK<K> t;                          // this lane's candidates
    double mv[K];                       // the merged global top-k (the same in every lane)
    int32_t mi[K];
#pragma unroll
    for (int s = 0; s < K; s++) { t.v[s] = unused_value<SQ>(); t.i[s] = 0x7FFFFFFF; mv[s] = unused_value<SQ>(); mi[s] = 0x7FFFFFFF; }
    double kth_s = INFINITY;            // s-domain bound of the global k-th entry (from the last merge)
    if (finite3(fx, fy, fz)) {
        const double qx = fx, qy = fy, qz = fz;
        const int ux = cell_coord(fx, g.lo[0], g.inv_h), uy = cell_coord(fy, g.lo[1], g.inv_h), uz = cell_coord(fz, g.lo[2], g.inv_h);
        const int r0 = max(max(max(-ux, ux - (g.n[0] - 1)), max(-uy, uy - (g.n[1] - 1))), max(max(-uz, uz - (g.n[2] - 1)), 0));
        int r = max(r0, 1), rp = -1;
        const double h = g.h, slack = g.slack;
        for (int step = 0; step < 40; step++) {
            const int xlo = max(ux - r, 0), xhi = min(ux + r, g.n[0] - 1);
            const int ylo = max(uy - r, 0), yhi = min(uy + r, g.n[1] - 1);
            const int zlo = max(uz - r, 0), zhi = min(uz + r, g.n[2] - 1);
            const double lim0 = fmin(kth_s, cap_s);                                        // (uniform: the bound of the last merge)
            double my_kth = kth_s;                                                         // tightened by this lane's own list
            auto consider = [&](const float4 rec) {
                const double dx = (double)rec.x - qx, dy = (double)rec.y - qy, dz = (double)rec.z - qz;   // t - q, kdtree.hpp:343
                const double s = (dx * dx + dy * dy) + dz * dz;
                if (!(s < cap_s) || !(s <= my_kth)) return;
                const int32_t j = (int32_t)__float_as_uint(rec.w);
                const double val = SQ ? s : sqrt(s);
                if (lex_less(val, j, t.v[K - 1], t.i[K - 1])) {
                    topk_insert<K>(t, val, j);
                    my_kth = fmin(my_kth, kth_bound<SQ>(t.v[K - 1]));                       // (a lane's own k-th bounds the global k-th from above)
                }
            };
            if (xlo <= xhi && ylo <= yhi && zlo <= zhi) {
                // The rows of the shell, 64 at a time, ONE ROW PER LANE: every lane resolves its row (pruning against the k-th ball, the
                // cell_start bounds of its one or two pieces — all 64 x 2..4 loads in flight together instead of one dependent pair per
                // row), an inclusive scan lays the pieces out as one index space, and the wave strides that space: candidate f belongs to
                // the lane whose offset is the last one <= f (six shuffle steps).
                const int ny_rows = yhi - ylo + 1, n_rows = ny_rows * (zhi - zlo + 1);
                for (int k0 = 0; k0 < n_rows; k0 += 64) {
                    const int kk = k0 + (int)lane;
                    uint32_t b1 = 0, c1 = 0, b2 = 0, c2 = 0;
                    if (kk < n_rows) {
                        const int cy = ylo + kk % ny_rows, cz = zlo + kk / ny_rows;
                        const int ady = abs(cy - uy), adz = abs(cz - uz);
                        const double fy2 = fmax((double)ady - 1.0 - slack, 0.0) * h, fz2 = fmax((double)adz - 1.0 - slack, 0.0) * h;
                        if (!(fy2 * fy2 + fz2 * fz2 > lim0 * 1.0001)) {                    // (else: the whole row is outside the k-th ball)
                            const uint32_t rowbase = (uint32_t)((cz * g.n[1] + cy) * g.n[0]);
                            if (ady <= rp && adz <= rp) {                                  // crosses the old cube: two end pieces
                                const int lb = min(xhi, ux - rp - 1), ra = max(xlo, ux + rp + 1);
                                if (xlo <= lb) { b1 = cell_start[rowbase + xlo]; c1 = cell_start[rowbase + lb + 1] - b1; }
                                if (ra <= xhi) { b2 = cell_start[rowbase + ra]; c2 = cell_start[rowbase + xhi + 1] - b2; }
                            } else {
                                b1 = cell_start[rowbase + xlo]; c1 = cell_start[rowbase + xhi + 1] - b1;
                            }
                        }
                    }
                    uint32_t inc = c1 + c2;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64); if ((int)lane >= o) inc += up; }
                    const uint32_t off = inc - (c1 + c2), total = (uint32_t)__shfl((int)inc, 63, 64);
                    for (uint32_t f = lane; f < total + 63u - (total + 63u) % 64u; f += 64) {     // (whole trips: the shuffles need every lane)
                        int owner = 0;
#pragma unroll
                        for (int step = 32; step > 0; step >>= 1)
                            if ((uint32_t)__shfl((int)off, owner + step, 64) <= f) owner += step;
                        const uint32_t rel = f - (uint32_t)__shfl((int)off, owner, 64);
                        const uint32_t ob1 = (uint32_t)__shfl((int)b1, owner, 64), oc1 = (uint32_t)__shfl((int)c1, owner, 64), ob2 = (uint32_t)__shfl((int)b2, owner, 64);
                        if (f < total) consider(records[rel < oc1 ? ob1 + rel : ob2 + (rel - oc1)]);
                    }
                }
            }
            // merge: K rounds, each takes the smallest head over the wave (the lane that owns it pops it); the previous merged list
            // takes part through lane 0, which holds it as its own list from the second stage on
#pragma unroll
            for (int s = 0; s < K; s++) {
                double hv = t.v[0];
                int32_t hi = t.i[0];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ov = __shfl_xor(hv, o, 64);
                    const int32_t oi = __shfl_xor(hi, o, 64);
                    if (lex_less(ov, oi, hv, hi)) { hv = ov; hi = oi; }
                }
                mv[s] = hv; mi[s] = hi;
                if (t.i[0] == hi && t.v[0] == hv && hi != 0x7FFFFFFF) {                    // mine: pop
#pragma unroll
                    for (int u = 0; u + 1 < K; u++) { t.v[u] = t.v[u + 1]; t.i[u] = t.i[u + 1]; }
                    t.v[K - 1] = unused_value<SQ>(); t.i[K - 1] = 0x7FFFFFFF;
                }
            }
#pragma unroll
            for (int s = 0; s < K; s++) { t.v[s] = lane == 0 ? mv[s] : unused_value<SQ>(); t.i[s] = lane == 0 ? mi[s] : 0x7FFFFFFF; }
            kth_s = kth_bound<SQ>(mv[K - 1]);                                              // INFINITY while fewer than K were seen
            const bool covers = (ux - r <= 0) && (ux + r >= g.n[0] - 1) && (uy - r <= 0) && (uy + r >= g.n[1] - 1) && (uz - r <= 0) && (uz + r >= g.n[2] - 1);
            const double reach = ((double)r - slack) * h;
            const double lim = fmin(kth_s, cap_s);                                         // nothing at or beyond `lim` can enter
            if (covers || lim < reach * reach * 0.99999) break;
            rp = r;
            if (lim < INFINITY) {
                const double need = fmin(sqrt(lim * 1.00002) * (double)g.inv_h + slack + 1.0, 16777216.0);
                r = max((int)need, rp + 1);
            } else {
                r = min(r * 2, 1 << 24);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < K; s++) {
        if (s < k_out && (int)lane == s) {
            const bool have = mi[s] != 0x7FFFFFFF;
            idx_out[(size_t)row * k_out + s] = have ? mi[s] : empty_idx;
            val_out[(size_t)row * k_out + s] = have ? mv[s] : empty_val;
        }
    }
    // results -> system-scope fence -> a ticket in device memory; the wave that draws the last ticket (every other wave's results are
    // fenced by then) publishes the completion word in host memory: ONE transaction over PCIe per call, not one per query
    __threadfence_system();
    if (lane == 0) {
        const uint32_t old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old % m == m - 1) __hip_atomic_store(done, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// normals[i] = eigenvector of the smallest eigenvalue of the scatter matrix of point i's neighbours (pca_normal.py:17-36,
// :96-103): centre = sum / n, XTX = sum (p - c)(p - c)^T in neighbour order (ascending distance); zeros when fewer than 3
__global__ __launch_bounds__(KG_BLOCK) void normals_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, uint32_t n,
                                                           const int32_t* __restrict__ nbr, const uint32_t* __restrict__ found, int k,
                                                           double* __restrict__ normals)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * KG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = found[i];
    double out[3] = { 0.0, 0.0, 0.0 };
    if (cnt >= 3) {                                                                    // pca_normal.py:97
        double sx = 0, sy = 0, sz = 0;
        for (uint32_t s = 0; s < cnt; s++) {
            const int32_t j = nbr[(size_t)i * k + s];
            sx += (double)x[j]; sy += (double)y[j]; sz += (double)z[j];
        }
        const double cx = sx / (double)cnt, cy = sy / (double)cnt, cz = sz / (double)cnt;   // :20
        double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
        for (uint32_t s = 0; s < cnt; s++) {
            const int32_t j = nbr[(size_t)i * k + s];
            const double dx = (double)x[j] - cx, dy = (double)y[j] - cy, dz = (double)z[j] - cz;
            xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;   // :22
        }
        const double A[9] = { xx, xy, xz, xy, yy, yz, xz, yz, zz };
        eig3::smallest_eigenvector<false>(A, out);         // (false: diag(a, a, b), a < b answers x — eig3.hpp)
    }
    normals[3 * (size_t)i] = out[0]; normals[3 * (size_t)i + 1] = out[1]; normals[3 * (size_t)i + 2] = out[2];
}

// a grid for k-NN: the cached 1-NN grid's cell (occupancy ~2) widened by sqrt(k / 4) so that the first cube usually
// holds the k neighbours (points per cell grow with h^2 on surfaces)
int knn_grid_for(pcr_ctx* ctx, const pcr_cloud* db, int k, Grid** out, bool* owned)
{
    *owned = false;
    {
        int rcb = build_target_grid(ctx, db);
        if (rcb) return rcb;
    }
    const double scale = (double)tune_get(ctx, "knn_cell_scale_x100", 0) / 100.0;
    const double f = scale > 0 ? scale : std::min(2.0, std::sqrt(std::max(1.0, (double)k / 4.0)));   // measured: profiles/r01_knn_grid.txt
    if (f <= 1.05 && db->grid->x_sorted) { *out = db->grid; return PCR_OK; }     // (a Morton-ordered 1-NN grid cannot serve the x-window walk)
    // the widened grid is kept on the cloud as well (one slot: the factor of the last batch), so that repeated batches with
    // the same k — normals, ISS, the hw2 benchmark protocol — do not rebuild it
    pcr_cloud* mdb = const_cast<pcr_cloud*>(db);
    if (mdb->knn_grid && mdb->knn_grid_factor == f) { *out = mdb->knn_grid; return PCR_OK; }
    if (mdb->knn_grid) {
        PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // a kernel of an earlier batch may still read it
        grid_free(mdb->knn_grid); mdb->knn_grid = nullptr; mdb->knn_grid_factor = 0.0;
    }
    ProfScope p(ctx, "grid_build");
    int rc = grid_build(ctx, db, out, (double)db->grid->p.h * f);
    if (rc) return rc;
    mdb->knn_grid = *out;
    mdb->knn_grid_factor = f;
    return PCR_OK;
}

}  // namespace

// device results: idx [m x k], val [m x k], found [m] at the head of a fresh allocation (caller frees)
int knn_grid_device(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* q, int k, double cap_s, bool squared, double empty_val, int32_t empty_idx,
                    void** result, int32_t** idx_dev, double** val_dev, uint32_t** found_dev)
{
    const size_t m = q->n;
    Grid* g = nullptr;
    bool owned = false;
    int rc = knn_grid_for(ctx, db, k, &g, &owned);
    if (rc) return rc;
    const GridPtr g_owner(owned ? g : nullptr);
    const uint32_t* perm = nullptr;
    if (q != db) {
        // cell-sorted permutation of the queries (coarse cells of db's cached grid; any spatial grouping will do)
        ProfScope p(ctx, "grid_sort_queries");
        rc = grid_prepare_queries(ctx, db, q);
        if (rc) return rc;
        perm = ctx->qperm;
    }
    Layout L;
    L.add(val_dev, m * (size_t)k);
    L.add(idx_dev, m * (size_t)k);
    L.add(found_dev, m);
    void* res = nullptr;
    hipError_t e = hipMalloc(&res, L.bytes());
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "hipMalloc(knn)", e);
    L.bind(res);
    *result = res;
    {
        ProfScope p(ctx, "knn_grid", 1);
        const dim3 grid((unsigned)((m + KG_BLOCK - 1) / KG_BLOCK));
#define PCR_KG(KK)                                                                                                                          \
    do {                                                                                                                                    \
        if (squared)                                                                                                                        \
            hipLaunchKernelGGL((knn_grid_kernel<KK, true>), grid, dim3(KG_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, q->x(), q->y(), q->z(), \
                               perm, (uint32_t)m, k, cap_s, empty_val, empty_idx, *idx_dev, *val_dev, *found_dev, 0);                          \
        else                                                                                                                                \
            hipLaunchKernelGGL((knn_grid_kernel<KK, false>), grid, dim3(KG_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, q->x(), q->y(), q->z(), \
                               perm, (uint32_t)m, k, cap_s, empty_val, empty_idx, *idx_dev, *val_dev, *found_dev, 0);                          \
    } while (0)
        if (k <= 1) PCR_KG(1);
        else if (k <= 4) PCR_KG(4);
        else if (k <= 8) PCR_KG(8);
        else if (k <= 16) PCR_KG(16);
        else PCR_KG(32);
#undef PCR_KG
    }
    e = hipGetLastError();
    if (e == hipSuccess && owned) e = hipStreamSynchronize(ctx->stream);      // the private grid must outlive the kernel
    if (e != hipSuccess) { hipFree(res); *result = nullptr; return fail(ctx, PCR_ERR_HIP, "knn_grid", e); }
    return PCR_OK;
}

// Small batches (m <= KNN_SMALL_MAX queries given on the host as f32 rows): ONE launch and one stream synchronisation — no
// query cloud, no result allocation, no copy command.  The kernel reads the queries from pinned host memory and writes the
// rows there (zero-copy over PCIe: a few hundred bytes per query); the widened grid of db is cached on the cloud.
// A driver that asks one question at a time (KDTreeKNNSearch per query, nanoflann findNeighbors) pays a launch + a wake-up
// per call instead of the 13 ms single-lane scan of the exhaustive kernel.
// a handful of queries (<= KNN_COOP_MAX): one wave per query, completion polled in host memory (tune knn_coop: 2 = off)
constexpr size_t KNN_COOP_MAX = 16;

static int cloud_knn_coop(pcr_ctx* ctx, const Grid* g, const float* q_rows, size_t m, int k, double cap_s, bool squared, double empty_val, int32_t empty_idx,
                          int32_t* idx, double* val)
{
    // a small coherent (fine-grained) host buffer of its own: [done word | values | indices], and a ticket word in device memory
    constexpr size_t OFF_V = 256, OFF_I = OFF_V + KNN_COOP_MAX * 32 * 8, TOTAL = OFF_I + KNN_COOP_MAX * 32 * 4;
    if (!ctx->coop_host || !ctx->coop_ticket) {
        // (both or neither: a failure between the two allocations must not leave a host buffer behind that makes the next call skip the
        // ticket's allocation and launch with a null pointer — ADVICE r3)
        if (ctx->coop_host) { hipHostFree(ctx->coop_host); ctx->coop_host = nullptr; }
        if (ctx->coop_ticket) { hipFree(ctx->coop_ticket); ctx->coop_ticket = nullptr; }
        void* host = nullptr; uint32_t* ticket = nullptr;
        hipError_t e = hipHostMalloc(&host, TOTAL, hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipMalloc((void**)&ticket, 256);
        if (e == hipSuccess) e = hipMemset(ticket, 0, 256);
        if (e != hipSuccess) { if (host) hipHostFree(host); if (ticket) hipFree(ticket); return fail(ctx, PCR_ERR_HIP, "knn coop buffers", e); }
        memset(host, 0, TOTAL);
        ctx->coop_host = host; ctx->coop_ticket = ticket;
    }
    char* st = (char*)ctx->coop_host;
    volatile uint32_t* done = (volatile uint32_t*)st;
    CoopQueries qs;
    for (size_t i = 0; i < KNN_COOP_MAX; i++) { const size_t j = i < m ? i : 0; qs.x[i] = q_rows[3 * j]; qs.y[i] = q_rows[3 * j + 1]; qs.z[i] = q_rows[3 * j + 2]; }
    double* val_p = (double*)(st + OFF_V);
    int32_t* idx_p = (int32_t*)(st + OFF_I);
    // the ticket counts waves modulo m: a call must find it at a multiple of m (the previous call used another m: reset it, in stream order)
    if (ctx->coop_m != m) { PCR_HIP(ctx, hipMemsetAsync(ctx->coop_ticket, 0, 4, ctx->stream)); ctx->coop_m = m; }
    const uint32_t target = ++ctx->coop_seq;
    ctx->coop_calls++;
#define PCR_KC(KK)                                                                                                                          \
    do {                                                                                                                                    \
        if (squared)                                                                                                                        \
            hipLaunchKernelGGL((knn_grid_coop_kernel<KK, true>), dim3((unsigned)m), dim3(64), 0, ctx->stream, g->records, g->cell_start, g->p, qs, \
                               (uint32_t)m, k, cap_s, empty_val, empty_idx, idx_p, val_p, (uint32_t*)st, target, ctx->coop_ticket);          \
        else                                                                                                                                \
            hipLaunchKernelGGL((knn_grid_coop_kernel<KK, false>), dim3((unsigned)m), dim3(64), 0, ctx->stream, g->records, g->cell_start, g->p, qs, \
                               (uint32_t)m, k, cap_s, empty_val, empty_idx, idx_p, val_p, (uint32_t*)st, target, ctx->coop_ticket);          \
    } while (0)
    if (k <= 1) PCR_KC(1);
    else if (k <= 4) PCR_KC(4);
    else if (k <= 8) PCR_KC(8);
    else if (k <= 16) PCR_KC(16);
    else PCR_KC(32);
#undef PCR_KC
    PCR_HIP(ctx, hipGetLastError());
    // poll the completion word (a few microseconds after the last wave's store); a stream synchronisation settles it if it does not
    // show up in time — correctness never depends on the poll
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (uint32_t spin = 0; ; spin++) {
        if (*done == target) { seen = true; break; }
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!seen) {
        // (a wave count the ticket did not expect, a failed launch ...: the stream settles it; the ticket restarts from zero)
        ctx->coop_unseen++;
        PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PCR_HIP(ctx, hipMemsetAsync(ctx->coop_ticket, 0, 4, ctx->stream));
    }
    memcpy(idx, idx_p, m * (size_t)k * 4);
    memcpy(val, val_p, m * (size_t)k * 8);
    return PCR_OK;
}

int cloud_knn_small(pcr_ctx* ctx, const pcr_cloud* db, const float* q_rows, size_t m, int k, double cap_s, bool squared, double empty_val,
                    int32_t empty_idx, int32_t* idx, double* val)
{
    if (m == 0) return PCR_OK;
    Grid* g = nullptr;
    bool owned = false;
    int rc = knn_grid_for(ctx, db, k, &g, &owned);
    if (rc) return rc;
    const GridPtr g_owner(owned ? g : nullptr);
    if (m <= KNN_COOP_MAX && !owned && tune_get(ctx, "knn_coop", 1) == 1) return cloud_knn_coop(ctx, g, q_rows, m, k, cap_s, squared, empty_val, empty_idx, idx, val);
    float *qx, *qy, *qz;
    double* val_p;
    int32_t* idx_p;
    uint32_t* found_p;
    Layout L;
    L.add(&qx, m);
    L.add(&qy, m);
    L.add(&qz, m);
    L.add(&val_p, m * (size_t)k);
    L.add(&idx_p, m * (size_t)k);
    L.add(&found_p, m);
    rc = ensure_stage(ctx, L.bytes());
    if (rc == PCR_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, PCR_ERR_HIP, "knn small: sync");
    if (rc) return rc;
    L.bind(ctx->host_stage);
    for (size_t i = 0; i < m; i++) { qx[i] = q_rows[3 * i]; qy[i] = q_rows[3 * i + 1]; qz[i] = q_rows[3 * i + 2]; }
    {
        ProfScope p(ctx, "knn_grid", 1);
        const dim3 grid((unsigned)((m + KG_BLOCK - 1) / KG_BLOCK));
#define PCR_KG(KK)                                                                                                                          \
    do {                                                                                                                                    \
        if (squared)                                                                                                                        \
            hipLaunchKernelGGL((knn_grid_kernel<KK, true>), grid, dim3(KG_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, qx, qy, qz, \
                               (const uint32_t*)nullptr, (uint32_t)m, k, cap_s, empty_val, empty_idx, idx_p, val_p, found_p, 1);             \
        else                                                                                                                                \
            hipLaunchKernelGGL((knn_grid_kernel<KK, false>), grid, dim3(KG_BLOCK), 0, ctx->stream, g->records, g->cell_start, g->p, qx, qy, qz, \
                               (const uint32_t*)nullptr, (uint32_t)m, k, cap_s, empty_val, empty_idx, idx_p, val_p, found_p, 1);             \
    } while (0)
        if (k <= 1) PCR_KG(1);
        else if (k <= 4) PCR_KG(4);
        else if (k <= 8) PCR_KG(8);
        else if (k <= 16) PCR_KG(16);
        else PCR_KG(32);
#undef PCR_KG
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "knn small", e);
    memcpy(idx, idx_p, m * (size_t)k * 4);
    memcpy(val, val_p, m * (size_t)k * 8);
    return PCR_OK;
}

int cloud_knn_host(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* q, int k, double cap_s, bool squared, double empty_val, int32_t empty_idx,
                   int32_t* idx, double* val, uint32_t* found)
{
    const size_t m = q->n;
    if (m == 0) return PCR_OK;
    void* res = nullptr;
    int32_t* idx_dev = nullptr;
    double* val_dev = nullptr;
    uint32_t* found_dev = nullptr;
    int rc = knn_grid_device(ctx, db, q, k, cap_s, squared, empty_val, empty_idx, &res, &idx_dev, &val_dev, &found_dev);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(idx, idx_dev, m * (size_t)k * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(val, val_dev, m * (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && found) e = hipMemcpyAsync(found, found_dev, m * 4, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    hipFree(res);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, "knn_grid read-back", e != hipSuccess ? e : e2);
    return PCR_OK;
}

}  // namespace pcr

using namespace pcr;

extern "C" {

int pcr_cloud_knn_f64(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* queries, int k, double radius, int squared, int32_t* idx, double* dist,
                      uint32_t* found)
{
    if (!ctx || !db || !queries || k < 1 || k > 32 || (queries->n && (!idx || !dist))) return fail(ctx, PCR_ERR_ARG, "pcr_cloud_knn_f64");
    if (db->n > 0x7FFFFFF0ull || queries->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_cloud_knn_f64: cloud too large");
    if (std::isnan(radius)) return fail(ctx, PCR_ERR_ARG, "pcr_cloud_knn_f64: radius is NaN");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    // hybrid search: strict cap on the squared distance (FLANN KNNRadiusResultSet semantics); radius < 0 = no cap
    const double cap_s = radius < 0 ? INFINITY : radius * radius;
    const int rc = cloud_knn_host(ctx, db, queries, k, cap_s, squared != 0, squared ? 1.7976931348623157e308 : 1e10, squared ? -1 : 0, idx, dist, found);
    prof_flush(ctx);
    return rc;
}

int pcr_normals_knn_f64(pcr_ctx* ctx, const pcr_cloud* cloud, int k, double radius, double* normals)
{
    if (!ctx || !cloud || k < 1 || k > 32 || (cloud->n && !normals) || std::isnan(radius)) return fail(ctx, PCR_ERR_ARG, "pcr_normals_knn_f64");
    if (cloud->n > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_normals_knn_f64: cloud too large");
    const size_t n = cloud->n;
    if (n == 0) return PCR_OK;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    void* res = nullptr;
    int32_t* idx_dev = nullptr;
    double* val_dev = nullptr;
    uint32_t* found_dev = nullptr;
    int rc = knn_grid_device(ctx, cloud, cloud, k, radius < 0 ? INFINITY : radius * radius, true, 1.7976931348623157e308, -1, &res, &idx_dev, &val_dev, &found_dev);
    if (rc) return rc;
    double* nrm_dev = nullptr;
    hipError_t e = hipMalloc((void**)&nrm_dev, n * 3 * sizeof(double));
    if (e == hipSuccess) {
        ProfScope p(ctx, "normals_pca", 1);
        hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((n + KG_BLOCK - 1) / KG_BLOCK)), dim3(KG_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(),
                           (uint32_t)n, idx_dev, found_dev, k, nrm_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(normals, nrm_dev, n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    hipFree(res);
    if (nrm_dev) hipFree(nrm_dev);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_normals_knn_f64", e != hipSuccess ? e : e2);
    prof_flush(ctx);
    return PCR_OK;
}

}  // extern "C"
