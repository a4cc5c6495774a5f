// kitti_eval.hip — Homework6: the KITTI object evaluator (Homework6/devkit_object/cpp/evaluate_object.cpp) on the GPU.
// The contracts are written out above pcr_box_overlap_f64 in include/pcr.h; this file follows them.
//
//   prepare (host)      rows -> KBox: the fields plus cos(ry), sin(ry) — the ONE place the heading's sine and cosine are formed (std::cos / std::sin
//                       of the host), so a matrix is plain unfused f64 arithmetic on the device.  cleanData's codes for the three difficulties.
//   ke_overlap_kernel   one (ground truth, detection) pair per lane over ALL frames: a binary search of mat_ptr finds the lane's frame.  IMAGE is
//                       imageBoxOverlap; GROUND / BOX3D form the corners as toPolygon does and clip the detection quad by the four edges of the
//                       ground-truth quad (ke_quad_inter): at most 8 vertices, appended through unrolled selects so they stay in registers.
//   ke_match_kernel     computeStatistics: one WAVE per (frame, metric, difficulty), lane t = threshold t (at most 41).  The overlap row, the codes
//                       and the scores are wave-uniform reads; assigned_detection is a 64-bit register per lane up to 64 detections and
//                       ceil(nd / 64) lane-interleaved words of a per-wave spill block beyond.  <false>: the collecting mode, lane 0 alone.
//   ke_walk_kernel      getThresholds without the sort: which ranks the recall walk picks depends on (count, n_gt) alone — one workgroup per
//   ke_rank_kernel      (metric, difficulty) finds them (a block-wide find-first per pick); then every pooled score counts the scores above it
//                       (ties by position; the pool is read through LDS tiles) and the picked ranks write their value: the element std::sort
//                       would leave at that index.  The collecting pass appends a frame's scores to its pool at an atomically drawn offset: the
//                       order of a pool is not fixed, the value at every rank is.
//   totals              tp / fp / fn: integer atomics.  Similarity: every frame's f64 sum rounded to the grid 2^-40 and added as an integer.
#include "pcr_internal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int KE_BLOCK = 256, KE_WAVES = KE_BLOCK / 64, KE_NT = PCR_KITTI_SAMPLE_PTS, KE_NCOMBO = 9;
constexpr double KE_NO_DETECTION = -10000000.0;
constexpr double KE_SIM_GRID = 1099511627776.0;            // 2^40: the fixed-point grid of the similarity totals
constexpr int KE_MIN_HEIGHT[3] = { 40, 25, 25 };
constexpr int KE_MAX_OCCLUSION[3] = { 0, 1, 2 };
constexpr double KE_MAX_TRUNCATION[3] = { 0.15, 0.3, 0.5 };
constexpr int64_t KE_BLOCKS_DEFAULT = 2048;                // tune key kitti_blocks: the grid of every launch here is capped, the kernels stride
constexpr size_t KE_MAX_ROWS = 1ull << 22;                 // boxes of one kind in a call: the similarity total stays below 2^62 on its grid

enum { CLS_CAR = 0, CLS_PEDESTRIAN = 1, CLS_CYCLIST = 2, CLS_VAN = 3, CLS_PERSON_SITTING = 4, CLS_DONTCARE = 5 };

// a box as the kernels read it (ground truth and detections alike)
struct KBox {
    double x1, y1, x2, y2, h, w, l, t1, t2, t3, c, s, alpha, score, cls, pad;
};

// std::min / std::max as the reference calls them (the second argument wins only on a strict comparison)
__host__ __device__ __forceinline__ double ke_min(double a, double b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ double ke_max(double a, double b) { return a < b ? b : a; }

__device__ __forceinline__ void ke_corners(const KBox& b, double* px, double* pz)
{
    const double hl = b.l / 2, hw = b.w / 2, ns = -b.s;
    const double X[4] = { hl, hl, -hl, -hl }, Z[4] = { hw, -hw, -hw, hw };
#pragma unroll
    for (int i = 0; i < 4; i++) {
        px[i] = (b.c * X[i] + b.s * Z[i]) + b.t1;
        pz[i] = (ns * X[i] + b.c * Z[i]) + b.t3;
    }
}

// o[m] = v for a run-time m with compile-time indices only: the arrays stay in registers; m >= 8 writes nothing
__device__ __forceinline__ void ke_put(double* ox, double* oz, int m, double x, double z)
{
#pragma unroll
    for (int q = 0; q < 8; q++) {
        ox[q] = q == m ? x : ox[q];
        oz[q] = q == m ? z : oz[q];
    }
}

// the area of (detection quad) ∩ (ground-truth quad): the rule of include/pcr.h
__device__ __forceinline__ double ke_quad_inter(const double* gx, const double* gz, const double* dx, const double* dz)
{
    double a2 = 0.0;
#pragma unroll
    for (int k = 1; k < 3; k++) a2 = a2 + ((gx[k] - gx[0]) * (gz[k + 1] - gz[0]) - (gx[k + 1] - gx[0]) * (gz[k] - gz[0]));
    const double sgn = a2 < 0.0 ? -1.0 : 1.0;
    double vx[8], vz[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        vx[k] = k < 4 ? dx[k] : 0.0;
        vz[k] = k < 4 ? dz[k] : 0.0;
    }
    int n = 4;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const double ax = gx[e], az = gz[e], ex = gx[(e + 1) & 3] - ax, ez = gz[(e + 1) & 3] - az;
        double d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = sgn * (ex * (vz[k] - az) - ez * (vx[k] - ax));
        double ox[8], oz[8];
#pragma unroll
        for (int k = 0; k < 8; k++) ox[k] = oz[k] = 0.0;
        int m = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (k < n) {
                const bool wrap = k + 1 >= 8 || k + 1 >= n;
                const double qx = wrap ? vx[0] : vx[(k + 1) & 7], qz = wrap ? vz[0] : vz[(k + 1) & 7], dq = wrap ? d[0] : d[(k + 1) & 7];
                const double px = vx[k], pz = vz[k], dp = d[k];
                const bool in_p = dp >= 0.0, in_q = dq >= 0.0;
                if (in_p) {
                    ke_put(ox, oz, m, px, pz);
                    m++;
                }
                if (in_p != in_q) {                                         // from the INSIDE end: a vertex on the edge (d == 0) is returned exactly
                    const double ix = in_p ? px : qx, iz = in_p ? pz : qz, jx = in_p ? qx : px, jz = in_p ? qz : pz;
                    const double di = in_p ? dp : dq, dj = in_p ? dq : dp;
                    const double t = di / (di - dj);
                    ke_put(ox, oz, m, ix + (jx - ix) * t, iz + (jz - iz) * t);
                    m++;
                }
            }
        }
        n = m < 8 ? m : 8;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            vx[k] = ox[k];
            vz[k] = oz[k];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 1; k < 7; k++)
        if (k + 1 < n) s = s + ((vx[k] - vx[0]) * (vz[k + 1] - vz[0]) - (vx[k + 1] - vx[0]) * (vz[k] - vz[0]));
    return fabs(s * 0.5);
}

// boxoverlap(det, gt, criterion) of the reference for the three metrics
__device__ __forceinline__ double ke_overlap(int metric, int criterion, const KBox& g, const KBox& d)
{
    if (metric == PCR_KITTI_IMAGE) {                                        // imageBoxOverlap(a = detection, b = ground truth)
        const double x1 = ke_max(d.x1, g.x1), y1 = ke_max(d.y1, g.y1), x2 = ke_min(d.x2, g.x2), y2 = ke_min(d.y2, g.y2);
        const double w = x2 - x1, h = y2 - y1;
        if (w <= 0 || h <= 0) return 0.0;
        const double inter = w * h, a_area = (d.x2 - d.x1) * (d.y2 - d.y1), b_area = (g.x2 - g.x1) * (g.y2 - g.y1);
        if (criterion == -1) return inter / (a_area + b_area - inter);
        return criterion == 0 ? inter / a_area : inter / b_area;
    }
    double gx[4], gz[4], dx[4], dz[4];
    ke_corners(g, gx, gz);
    ke_corners(d, dx, dz);
    const double inter = ke_quad_inter(gx, gz, dx, dz);
    if (metric == PCR_KITTI_GROUND) {
        const double ad = fabs(d.l * d.w), ag = fabs(g.l * g.w);
        if (criterion == -1) return inter / (ad + ag - inter);
        return criterion == 0 ? inter / ad : inter / ag;
    }
    const double ymax = ke_min(d.t2, g.t2), ymin = ke_max(d.t2 - d.h, g.t2 - g.h);
    const double inter_vol = inter * ke_max(0.0, ymax - ymin);
    const double det_vol = d.h * d.l * d.w, gt_vol = g.h * g.l * g.w;
    if (criterion == -1) return inter_vol / (det_vol + gt_vol - inter_vol);
    return criterion == 0 ? inter_vol / det_vol : inter_vol / gt_vol;
}

__global__ __launch_bounds__(KE_BLOCK) void ke_overlap_kernel(const KBox* __restrict__ gt, const KBox* __restrict__ det, const uint64_t* __restrict__ gt_ptr,
                                                              const uint64_t* __restrict__ det_ptr, const uint64_t* __restrict__ mat_ptr, uint32_t n_frames,
                                                              int metric, int criterion, double* __restrict__ out)
{
    const uint64_t total = mat_ptr[n_frames];
    for (uint64_t p = (uint64_t)blockIdx.x * KE_BLOCK + threadIdx.x; p < total; p += (uint64_t)gridDim.x * KE_BLOCK) {
        uint32_t lo = 0, hi = n_frames;                                     // the last frame f with mat_ptr[f] <= p (empty frames share an offset)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (mat_ptr[mid] <= p) lo = mid; else hi = mid;
        }
        const uint64_t local = p - mat_ptr[lo], nd = det_ptr[lo + 1] - det_ptr[lo];
        const uint64_t i = local / nd, j = local - i * nd;
        out[p] = ke_overlap(metric, criterion, gt[gt_ptr[lo] + i], det[det_ptr[lo] + j]);
    }
}

// ---- matching ------------------------------------------------------------------------------------------------------------------------------
struct KeArgs {
    const KBox *gt, *det;
    const uint64_t *gt_ptr, *det_ptr, *mat_ptr;
    const double* ov[3];                 // per metric: the union-criterion matrices (null where no combo uses the metric)
    const int8_t *ign_gt, *ign_det;      // [3 difficulties][rows]
    uint64_t n_gt_rows, n_det_rows;
    uint32_t n_frames, n_combo;
    int metric[KE_NCOMBO], diff[KE_NCOMBO], aos[KE_NCOMBO];
    double min_overlap;
    const double* thr;                   // [n_combo][41]
    const int32_t* n_thr;                // [n_combo]
    int32_t *frame_tp, *frame_fp, *frame_fn;      // per frame and threshold (frame_stats, n_combo == 1), or null
    double* frame_sim;
    uint32_t frame_width;
    unsigned long long* tot;             // [n_combo][41][4] = tp, fp, fn, similarity on the grid, or null
    double* scores;                      // collecting mode: [n_combo][n_gt_rows], frame f's at gt_ptr[f] ...
    double* pool;                        // ... and, where the thresholds follow on the device, appended to [n_combo][n_gt_rows] without holes
    uint32_t* n_scores;                  // [n_combo]: the fill of every pool (with pool), or null
    unsigned long long* spill;           // [waves of the grid][spill_words][64 lanes]
    uint32_t spill_words;
};

struct RegMask {
    unsigned long long m;
    __device__ __forceinline__ bool get(uint32_t j) const { return (m >> j) & 1ull; }
    __device__ __forceinline__ void set(uint32_t j) { m |= 1ull << j; }
};
struct MemMask {
    unsigned long long* p;               // this lane's column: word k at p[64 k]
    __device__ __forceinline__ bool get(uint32_t j) const { return (p[(size_t)(j >> 6) * 64] >> (j & 63u)) & 1ull; }
    __device__ __forceinline__ void set(uint32_t j) { p[(size_t)(j >> 6) * 64] |= 1ull << (j & 63u); }
};

template <bool FP, class Mask>
__device__ __forceinline__ void ke_match(const KeArgs& A, uint32_t f, uint32_t cb, uint32_t lane, Mask assigned)
{
    const int metric = A.metric[cb], diff = A.diff[cb];
    const bool aos = A.aos[cb] != 0;
    const uint64_t g0 = A.gt_ptr[f], d0 = A.det_ptr[f];
    const uint32_t ng = (uint32_t)(A.gt_ptr[f + 1] - g0), nd = (uint32_t)(A.det_ptr[f + 1] - d0);
    const KBox* G = A.gt + g0;
    const KBox* D = A.det + d0;
    const int8_t* ig = A.ign_gt + (size_t)diff * A.n_gt_rows + g0;
    const int8_t* id = A.ign_det + (size_t)diff * A.n_det_rows + d0;
    const double* ov = A.ov[metric] + A.mat_ptr[f];
    const double mo = A.min_overlap;
    const uint32_t nthr = FP ? (uint32_t)A.n_thr[cb] : 1u;
    const bool live = lane < nthr;
    const double thr = (FP && live) ? A.thr[cb * KE_NT + lane] : 0.0;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if (live) {
        for (uint32_t i = 0; i < ng; i++) {
            const int igi = ig[i];
            if (igi == -1) continue;
            int det_idx = -1;
            double valid_detection = KE_NO_DETECTION, max_overlap = 0.0;
            bool assigned_ignored_det = false;
            for (uint32_t j = 0; j < nd; j++) {
                const int idj = id[j];
                if (idj == -1) continue;
                if (assigned.get(j)) continue;
                const double sc = D[j].score;
                if (FP && sc < thr) continue;                               // ignored_threshold[j]
                const double overlap = ov[(size_t)i * nd + j];
                if (!FP && overlap > mo && sc > valid_detection) {
                    det_idx = (int)j;
                    valid_detection = sc;
                } else if (FP && overlap > mo && (overlap > max_overlap || assigned_ignored_det) && idj == 0) {
                    max_overlap = overlap;
                    det_idx = (int)j;
                    valid_detection = 1;
                    assigned_ignored_det = false;
                } else if (FP && overlap > mo && valid_detection == KE_NO_DETECTION && idj == 1) {
                    det_idx = (int)j;
                    valid_detection = 1;
                    assigned_ignored_det = true;
                }
            }
            if (valid_detection == KE_NO_DETECTION && igi == 0) {
                fn++;
            } else if (valid_detection != KE_NO_DETECTION && (igi == 1 || id[det_idx] == 1)) {
                assigned.set((uint32_t)det_idx);
            } else if (valid_detection != KE_NO_DETECTION) {
                if (!FP) A.scores[(size_t)cb * A.n_gt_rows + g0 + (uint32_t)tp] = D[det_idx].score;
                tp++;
                if (FP && aos) sim = sim + (1.0 + cos(G[i].alpha - D[det_idx].alpha)) / 2.0;
                assigned.set((uint32_t)det_idx);
            }
        }
        if (FP) {
            for (uint32_t j = 0; j < nd; j++) {
                const int idj = id[j];
                if (!(assigned.get(j) || idj == -1 || idj == 1 || D[j].score < thr)) fp++;
            }
            int nstuff = 0;
            for (uint32_t i = 0; i < ng; i++) {
                if (G[i].cls != (double)CLS_DONTCARE) continue;
                for (uint32_t j = 0; j < nd; j++) {
                    const int idj = id[j];
                    if (idj == -1 || idj == 1) continue;
                    if (assigned.get(j)) continue;
                    if (D[j].score < thr) continue;
                    if (ke_overlap(metric, 0, G[i], D[j]) > mo) {
                        assigned.set(j);
                        nstuff++;
                    }
                }
            }
            fp -= nstuff;
        }
        const bool any = tp > 0 || fp > 0;
        if (A.frame_tp) {
            const size_t o = (size_t)f * A.frame_width + lane;
            A.frame_tp[o] = tp;
            A.frame_fp[o] = fp;
            A.frame_fn[o] = fn;
            if (A.frame_sim) A.frame_sim[o] = (FP && aos) ? (any ? sim : -1.0) : 0.0;
        }
        if (FP && A.tot) {
            unsigned long long* t = A.tot + ((size_t)cb * KE_NT + lane) * 4;
            if (tp) atomicAdd(t + 0, (unsigned long long)tp);
            if (fp) atomicAdd(t + 1, (unsigned long long)fp);
            if (fn) atomicAdd(t + 2, (unsigned long long)fn);
            if (aos && any) {
                const unsigned long long q = (unsigned long long)llrint(sim * KE_SIM_GRID);
                if (q) atomicAdd(t + 3, q);
            }
        }
        if (!FP && A.pool && tp) {
            const uint32_t base = atomicAdd(A.n_scores + cb, (uint32_t)tp);     // < n_gt_rows: a ground truth gives at most one score
            for (int k = 0; k < tp; k++) A.pool[(size_t)cb * A.n_gt_rows + base + (uint32_t)k] = A.scores[(size_t)cb * A.n_gt_rows + g0 + (uint32_t)k];
        }
    }
}

template <bool FP>
__global__ __launch_bounds__(KE_BLOCK) void ke_match_kernel(KeArgs A)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint64_t n_work = (uint64_t)A.n_frames * A.n_combo, w0 = (uint64_t)blockIdx.x * KE_WAVES + wave;
    for (uint64_t w = w0; w < n_work; w += (uint64_t)gridDim.x * KE_WAVES) {
        const uint32_t f = (uint32_t)(w / A.n_combo), cb = (uint32_t)(w - (uint64_t)f * A.n_combo);
        const uint64_t nd = A.det_ptr[f + 1] - A.det_ptr[f];
        if (nd <= 64) {
            ke_match<FP, RegMask>(A, f, cb, lane, RegMask{ 0ull });
        } else {
            const uint32_t words = (uint32_t)((nd + 63) >> 6);              // <= spill_words: the host sized the block by the largest frame
            unsigned long long* p = A.spill + (size_t)w0 * A.spill_words * 64 + lane;
            for (uint32_t k = 0; k < words; k++) p[(size_t)k * 64] = 0ull;
            ke_match<FP, MemMask>(A, f, cb, lane, MemMask{ p });
        }
    }
}

// ---- getThresholds ---------------------------------------------------------------------------------------------------------------------------
struct KeWalkArgs {
    const uint32_t* n_scores;            // [n_combo]
    double n_gt[KE_NCOMBO];
    int32_t* picks;                      // [n_combo][41]: the indices the recall walk keeps
    int32_t* n_pick;                     // [n_combo]
};

__global__ __launch_bounds__(KE_BLOCK) void ke_walk_kernel(KeWalkArgs A)
{
    __shared__ uint32_t s_min;
    const uint32_t cb = blockIdx.x, tid = threadIdx.x, n = A.n_scores[cb];
    const double n_gt = A.n_gt[cb];
    uint32_t start = 0;
    double current_recall = 0.0;
    int np = 0;
    while (start < n && np < KE_NT) {
        uint32_t found = 0xFFFFFFFFu;
        for (uint32_t base = start; base < n; base += KE_BLOCK) {          // the first i >= start the walk does not skip
            const uint32_t i = base + tid;
            bool pick = false;
            if (i < n) {
                const double l_recall = (double)(i + 1) / n_gt;
                const double r_recall = i < n - 1 ? (double)(i + 2) / n_gt : l_recall;
                pick = !((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1);
            }
            if (tid == 0) s_min = 0xFFFFFFFFu;
            __syncthreads();
            if (pick) atomicMin(&s_min, i);
            __syncthreads();
            found = s_min;
            __syncthreads();
            if (found != 0xFFFFFFFFu) break;
        }
        if (found == 0xFFFFFFFFu) break;                                    // (the last index is always kept)
        if (tid == 0) A.picks[cb * KE_NT + np] = (int32_t)found;
        np++;
        current_recall += 1.0 / (41.0 - 1.0);
        start = found + 1;
    }
    if (tid == 0) A.n_pick[cb] = np;
}

// pool: [n_combo][stride], n_scores[cb] scores each; the score of descending rank picks[t] goes to thr[t]
constexpr uint32_t KE_RANK_TILE = 1024;
__global__ __launch_bounds__(KE_BLOCK) void ke_rank_kernel(const double* __restrict__ pool, uint64_t stride, const uint32_t* __restrict__ n_scores,
                                                           const int32_t* __restrict__ picks, const int32_t* __restrict__ n_pick, double* __restrict__ thr)
{
    __shared__ double tile[KE_RANK_TILE];
    const uint32_t cb = blockIdx.y, tid = threadIdx.x, n = n_scores[cb];
    const double* s = pool + (size_t)cb * stride;
    const int np = n_pick[cb];
    for (uint32_t e0 = blockIdx.x * KE_BLOCK; e0 < n; e0 += gridDim.x * KE_BLOCK) {     // the same trips for the whole workgroup
        const uint32_t e = e0 + tid;
        const bool live = e < n;
        const double v = live ? s[e] : 0.0;
        uint32_t rank = 0;
        for (uint32_t base = 0; base < n; base += KE_RANK_TILE) {
            const uint32_t cnt = min(KE_RANK_TILE, n - base);
            __syncthreads();
            for (uint32_t k = tid; k < cnt; k += KE_BLOCK) tile[k] = s[base + k];
            __syncthreads();
            for (uint32_t k = 0; k < cnt; k++) {
                const double x = tile[k];
                rank += (x > v || (x == v && base + k < e)) ? 1u : 0u;
            }
        }
        if (live)
            for (int t = 0; t < np; t++)
                if ((uint32_t)picks[cb * KE_NT + t] == rank) thr[cb * KE_NT + t] = v;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
int32_t ke_trunc_i32(double a)             // int32_t height = fabs(...): the conversion of x86-64 (out of range and NaN give INT32_MIN)
{
    return (a == a && a > -2147483649.0 && a < 2147483648.0) ? (int32_t)a : INT32_MIN;
}

void ke_clean(int cls, int diff, const double* gt_rows, size_t ng, const double* det_rows, size_t nd, int8_t* ign_gt, int8_t* ign_det, uint64_t* n_gt)
{
    for (size_t i = 0; i < ng; i++) {
        const double* g = gt_rows + 15 * i;
        const int code = ke_trunc_i32(g[0]);
        const double height = g[7] - g[5];
        int valid_class;
        if (code == cls) valid_class = 1;
        else if (cls == CLS_PEDESTRIAN && code == CLS_PERSON_SITTING) valid_class = 0;
        else if (cls == CLS_CAR && code == CLS_VAN) valid_class = 0;
        else valid_class = -1;
        const bool ignore = ke_trunc_i32(g[2]) > KE_MAX_OCCLUSION[diff] || g[1] > KE_MAX_TRUNCATION[diff] || height <= KE_MIN_HEIGHT[diff];
        if (valid_class == 1 && !ignore) {
            ign_gt[i] = 0;
            (*n_gt)++;
        } else if (valid_class == 0 || (ignore && valid_class == 1)) {
            ign_gt[i] = 1;
        } else {
            ign_gt[i] = -1;
        }
    }
    for (size_t j = 0; j < nd; j++) {
        const double* d = det_rows + 15 * j;
        const int32_t height = ke_trunc_i32(fabs(d[3] - d[5]));
        if (height < KE_MIN_HEIGHT[diff]) ign_det[j] = 1;
        else if (ke_trunc_i32(d[0]) == cls) ign_det[j] = 0;
        else ign_det[j] = -1;
    }
}

bool ke_ptr_ok(const uint64_t* p, size_t n_frames)
{
    if (p[0] != 0) return false;
    for (size_t f = 0; f < n_frames; f++)
        if (p[f] > p[f + 1]) return false;
    return p[n_frames] <= KE_MAX_ROWS;
}

void ke_box_gt(const double* r, KBox* b)
{
    *b = { r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], std::cos(r[14]), std::sin(r[14]), r[3], 0.0, r[0], 0.0 };
}
void ke_box_det(const double* r, KBox* b)
{
    *b = { r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], std::cos(r[12]), std::sin(r[12]), r[1], r[13], r[0], 0.0 };
}

unsigned ke_blocks(const pcr_ctx* ctx, uint64_t items_per_block_total)
{
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(65535, tune_get(ctx, "kitti_blocks", KE_BLOCKS_DEFAULT)));
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)cap, items_per_block_total));
}

// one evaluation's device block: everything the host fills is a prefix of the layout, mirrored in the pinned stage and uploaded by ONE copy
struct KePlan {
    const char* who;
    size_t n_frames = 0, ng = 0, nd = 0;
    uint64_t total_pairs = 0, max_nd = 0;
    unsigned match_blocks = 1;
    uint32_t spill_words = 0;
    // uploaded
    KBox *gt = nullptr, *det = nullptr;
    uint64_t *gt_ptr = nullptr, *det_ptr = nullptr, *mat_ptr = nullptr;
    int8_t *ign_gt = nullptr, *ign_det = nullptr;
    double* thr_in = nullptr;            // [9][41] (frame_stats: the caller's thresholds)
    int32_t* n_thr_in = nullptr;
    size_t upload_bytes = 0;
    // device only
    double* ov[3] = { nullptr, nullptr, nullptr };
    double *scores = nullptr, *pool = nullptr;
    unsigned long long* spill = nullptr;
    // downloaded (one contiguous run)
    unsigned long long* tot = nullptr;
    double* thr = nullptr;
    int32_t *picks = nullptr, *n_pick = nullptr;
    uint32_t* n_scores = nullptr;
    size_t down_off = 0, down_bytes = 0;
    uint64_t n_gt[3] = { 0, 0, 0 };
    Layout L;
};

// validates, lays the block out and fills the stage; metrics: which overlap matrices get room; n_score_sets / n_pool_sets: per-frame score
// arrays and hole-free pools of n_gt_rows doubles each
int ke_prepare(pcr_ctx* ctx, KePlan& P, int cls, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows, const uint64_t* det_ptr, size_t n_frames,
               const bool metrics[3], size_t n_score_sets, size_t n_pool_sets)
{
    if (!ctx || !gt_ptr || !det_ptr) return fail(ctx, PCR_ERR_ARG, P.who);
    if (cls < 0 || cls > 2) return fail(ctx, PCR_ERR_ARG, "kitti: class must be 0 (Car), 1 (Pedestrian) or 2 (Cyclist)");
    if (n_frames > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "kitti: too many frames");
    if (!ke_ptr_ok(gt_ptr, n_frames) || !ke_ptr_ok(det_ptr, n_frames))
        return fail(ctx, PCR_ERR_ARG, "kitti: a row_ptr must start at 0, ascend and end at no more than 2^22 rows");
    P.n_frames = n_frames;
    P.ng = (size_t)gt_ptr[n_frames];
    P.nd = (size_t)det_ptr[n_frames];
    if ((P.ng && !gt_rows) || (P.nd && !det_rows)) return fail(ctx, PCR_ERR_ARG, "kitti: rows is NULL");
    std::vector<uint64_t> mat(n_frames + 1, 0);
    for (size_t f = 0; f < n_frames; f++) {
        const uint64_t a = gt_ptr[f + 1] - gt_ptr[f], b = det_ptr[f + 1] - det_ptr[f];
        mat[f + 1] = mat[f] + a * b;
        P.max_nd = std::max(P.max_nd, b);
    }
    P.total_pairs = mat[n_frames];
    if (P.total_pairs > (1ull << 40)) return fail(ctx, PCR_ERR_ARG, "kitti: more than 2^40 (ground truth, detection) pairs");
    P.match_blocks = ke_blocks(ctx, (n_frames * KE_NCOMBO + KE_WAVES - 1) / KE_WAVES);
    P.spill_words = P.max_nd > 64 ? (uint32_t)((P.max_nd + 63) >> 6) : 0u;
    Layout& L = P.L;
    L.add(&P.gt, P.ng);
    L.add(&P.det, P.nd);
    L.add(&P.gt_ptr, n_frames + 1);
    L.add(&P.det_ptr, n_frames + 1);
    L.add(&P.mat_ptr, n_frames + 1);
    L.add(&P.ign_gt, 3 * P.ng);
    L.add(&P.ign_det, 3 * P.nd);
    L.add(&P.thr_in, (size_t)KE_NCOMBO * KE_NT);
    L.add(&P.n_thr_in, (size_t)KE_NCOMBO);
    P.upload_bytes = L.bytes();
    for (int m = 0; m < 3; m++) L.add(&P.ov[m], metrics[m] ? (size_t)P.total_pairs : 0);
    L.add(&P.spill, (size_t)P.match_blocks * KE_WAVES * P.spill_words * 64);
    L.add(&P.scores, n_score_sets * P.ng);
    L.add(&P.pool, n_pool_sets * P.ng);
    P.down_off = L.bytes();
    L.add(&P.tot, (size_t)KE_NCOMBO * KE_NT * 4);
    L.add(&P.thr, (size_t)KE_NCOMBO * KE_NT);
    L.add(&P.picks, (size_t)KE_NCOMBO * KE_NT);
    L.add(&P.n_pick, (size_t)KE_NCOMBO);
    L.add(&P.n_scores, (size_t)KE_NCOMBO);
    P.down_bytes = L.bytes() - P.down_off;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_stage(ctx, P.upload_bytes + P.down_bytes);
    if (rc) return rc;
    rc = ensure_scratch(ctx, L.bytes());
    if (rc) return rc;
    L.bind(ctx->host_stage);                                                // the pointers name the stage while the host fills it ...
    for (size_t i = 0; i < P.ng; i++) ke_box_gt(gt_rows + 15 * i, P.gt + i);
    for (size_t j = 0; j < P.nd; j++) ke_box_det(det_rows + 15 * j, P.det + j);
    memcpy(P.gt_ptr, gt_ptr, (n_frames + 1) * 8);
    memcpy(P.det_ptr, det_ptr, (n_frames + 1) * 8);
    memcpy(P.mat_ptr, mat.data(), (n_frames + 1) * 8);
    for (int d = 0; d < 3; d++) ke_clean(cls, d, gt_rows, P.ng, det_rows, P.nd, P.ign_gt + d * P.ng, P.ign_det + d * P.nd, &P.n_gt[d]);
    memset(P.thr_in, 0, (size_t)KE_NCOMBO * KE_NT * 8);
    memset(P.n_thr_in, 0, (size_t)KE_NCOMBO * 4);
    return PCR_OK;
}

// ... and the device block from here on
int ke_upload(pcr_ctx* ctx, KePlan& P)
{
    P.L.bind(ctx->scratch);
    PCR_HIP(ctx, hipMemcpyAsync(ctx->scratch, ctx->host_stage, P.upload_bytes, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemsetAsync((char*)ctx->scratch + P.down_off, 0, P.down_bytes, ctx->stream));
    return PCR_OK;
}

int ke_download(pcr_ctx* ctx, KePlan& P, char** down)
{
    *down = (char*)ctx->host_stage + P.upload_bytes;
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(*down, (char*)ctx->scratch + P.down_off, P.down_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}
template <class T> T* ke_down(const KePlan& P, const pcr_ctx* ctx, char* down, T* dev) { return (T*)(down + ((char*)dev - ((char*)ctx->scratch + P.down_off))); }

void ke_launch_overlap(pcr_ctx* ctx, const KePlan& P, int metric, int criterion, double* out)
{
    if (P.total_pairs == 0) return;
    ProfScope ps(ctx, "kitti_overlap");
    hipLaunchKernelGGL(ke_overlap_kernel, dim3(ke_blocks(ctx, (P.total_pairs + KE_BLOCK - 1) / KE_BLOCK)), dim3(KE_BLOCK), 0, ctx->stream, P.gt, P.det, P.gt_ptr,
                       P.det_ptr, P.mat_ptr, (uint32_t)P.n_frames, metric, criterion, out);
}

KeArgs ke_args(const KePlan& P, int cls)
{
    KeArgs A = {};
    A.gt = P.gt; A.det = P.det; A.gt_ptr = P.gt_ptr; A.det_ptr = P.det_ptr; A.mat_ptr = P.mat_ptr;
    for (int m = 0; m < 3; m++) A.ov[m] = P.ov[m];
    A.ign_gt = P.ign_gt; A.ign_det = P.ign_det;
    A.n_gt_rows = P.ng; A.n_det_rows = P.nd;
    A.n_frames = (uint32_t)P.n_frames;
    A.min_overlap = cls == CLS_CAR ? 0.7 : 0.5;                             // MIN_OVERLAP[metric][class]: the three rows are the same
    A.spill = P.spill; A.spill_words = P.spill_words;
    A.scores = P.scores;
    return A;
}

template <bool FP> void ke_launch_match(pcr_ctx* ctx, const KePlan& P, const KeArgs& A)
{
    if (P.n_frames == 0) return;
    ProfScope ps(ctx, FP ? "kitti_match" : "kitti_collect");
    hipLaunchKernelGGL((ke_match_kernel<FP>), dim3(P.match_blocks), dim3(KE_BLOCK), 0, ctx->stream, A);
}

void ke_launch_thresholds(pcr_ctx* ctx, const KePlan& P, uint32_t n_combo, const double* n_gt, uint64_t n_slots)      // n_slots: the room of a pool
{
    ProfScope ps(ctx, "kitti_thresholds");
    KeWalkArgs W = {};
    W.n_scores = P.n_scores; W.picks = P.picks; W.n_pick = P.n_pick;
    for (uint32_t c = 0; c < n_combo; c++) W.n_gt[c] = n_gt[c];
    hipLaunchKernelGGL(ke_walk_kernel, dim3(n_combo), dim3(KE_BLOCK), 0, ctx->stream, W);
    if (n_slots)
        hipLaunchKernelGGL(ke_rank_kernel, dim3(ke_blocks(ctx, (n_slots + KE_BLOCK - 1) / KE_BLOCK), n_combo), dim3(KE_BLOCK), 0, ctx->stream, P.pool, n_slots,
                           P.n_scores, P.picks, P.n_pick, P.thr);
}

}  // namespace

}  // namespace pcr

using namespace pcr;

extern "C" int pcr_kitti_clean_data_f64(int cls, int difficulty, const double* gt_rows, size_t n_gt_rows, const double* det_rows, size_t n_det_rows,
                                        int32_t* ignored_gt, int32_t* ignored_det, uint64_t* n_gt)
{
    if (cls < 0 || cls > 2 || difficulty < 0 || difficulty > 2 || (n_gt_rows && (!gt_rows || !ignored_gt)) || (n_det_rows && (!det_rows || !ignored_det)))
        return PCR_ERR_ARG;
    std::vector<int8_t> ig(n_gt_rows), id(n_det_rows);
    uint64_t n = 0;
    ke_clean(cls, difficulty, gt_rows, n_gt_rows, det_rows, n_det_rows, ig.data(), id.data(), &n);
    for (size_t i = 0; i < n_gt_rows; i++) ignored_gt[i] = ig[i];
    for (size_t j = 0; j < n_det_rows; j++) ignored_det[j] = id[j];
    if (n_gt) *n_gt = n;
    return PCR_OK;
}

extern "C" int pcr_box_overlap_f64(pcr_ctx* ctx, int metric, int criterion, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows,
                                   const uint64_t* det_ptr, size_t n_frames, uint64_t* mat_ptr, double* out, size_t out_cap)
{
    if (!ctx || !mat_ptr) return fail(ctx, PCR_ERR_ARG, "pcr_box_overlap_f64");
    if (metric < 0 || metric > 2 || criterion < -1 || criterion > 1) return fail(ctx, PCR_ERR_ARG, "pcr_box_overlap_f64: metric 0 ... 2, criterion -1 ... 1");
    KePlan P;
    P.who = "pcr_box_overlap_f64";
    const bool metrics[3] = { metric == 0, metric == 1, metric == 2 };
    int rc = ke_prepare(ctx, P, 0, gt_rows, gt_ptr, det_rows, det_ptr, n_frames, metrics, 0, 0);
    if (rc) return rc;
    memcpy(mat_ptr, P.mat_ptr, (n_frames + 1) * 8);
    if (out_cap < P.total_pairs) return fail(ctx, PCR_ERR_ARG, "pcr_box_overlap_f64: out_cap is smaller than the total (mat_ptr is valid)");
    if (P.total_pairs == 0) return PCR_OK;
    if (!out) return fail(ctx, PCR_ERR_ARG, "pcr_box_overlap_f64: out is NULL");
    rc = ke_upload(ctx, P);
    if (rc) return rc;
    ke_launch_overlap(ctx, P, metric, criterion, P.ov[metric]);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, P.ov[metric], (size_t)P.total_pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_kitti_frame_stats_f64(pcr_ctx* ctx, int cls, int metric, int difficulty, int compute_fp, int compute_aos, const double* thresholds,
                                         size_t n_thresholds, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows, const uint64_t* det_ptr,
                                         size_t n_frames, int32_t* tp, int32_t* fp, int32_t* fn, double* similarity, double* tp_scores)
{
    if (!ctx) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_frame_stats_f64");
    if (metric < 0 || metric > 2 || difficulty < 0 || difficulty > 2) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_frame_stats_f64: metric / difficulty 0 ... 2");
    if (compute_fp && (n_thresholds > (size_t)KE_NT || (n_thresholds && !thresholds))) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_frame_stats_f64: at most 41 thresholds");
    const size_t width = compute_fp ? n_thresholds : 1;
    KePlan P;
    P.who = "pcr_kitti_frame_stats_f64";
    const bool metrics[3] = { metric == 0, metric == 1, metric == 2 };
    int rc = ke_prepare(ctx, P, cls, gt_rows, gt_ptr, det_rows, det_ptr, n_frames, metrics, compute_fp ? 0 : 1, 0);
    if (rc) return rc;
    if (n_frames == 0 || width == 0) return PCR_OK;
    if (!tp || !fp || !fn || (compute_fp && !similarity) || (!compute_fp && P.ng && !tp_scores)) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_frame_stats_f64: an output is NULL");
    if (n_frames * width > 0x7FFFFFF0ull) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_frame_stats_f64: frames x thresholds too large");
    for (size_t t = 0; compute_fp && t < n_thresholds; t++) P.thr_in[t] = thresholds[t];
    P.n_thr_in[0] = (int32_t)width;
    rc = ke_upload(ctx, P);
    if (rc) return rc;
    int32_t *ftp, *ffp, *ffn;                                               // the per-frame outputs: the second device block
    double* fsim;
    Layout LA;
    LA.add(&ftp, n_frames * width);
    LA.add(&ffp, n_frames * width);
    LA.add(&ffn, n_frames * width);
    LA.add(&fsim, n_frames * width);
    rc = bind_aux(ctx, LA);
    if (rc) return rc;
    if (!compute_fp && P.ng) PCR_HIP(ctx, hipMemsetAsync(P.scores, 0xFF, P.ng * 8, ctx->stream));      // all ones: a NaN = "no score here"
    ke_launch_overlap(ctx, P, metric, -1, P.ov[metric]);
    KeArgs A = ke_args(P, cls);
    A.n_combo = 1;
    A.metric[0] = metric; A.diff[0] = difficulty; A.aos[0] = compute_aos != 0;
    A.thr = P.thr_in; A.n_thr = P.n_thr_in;
    A.frame_tp = ftp; A.frame_fp = ffp; A.frame_fn = ffn; A.frame_sim = fsim; A.frame_width = (uint32_t)width;
    if (compute_fp) ke_launch_match<true>(ctx, P, A); else ke_launch_match<false>(ctx, P, A);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(tp, ftp, n_frames * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(fp, ffp, n_frames * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(fn, ffn, n_frames * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (similarity) PCR_HIP(ctx, hipMemcpyAsync(similarity, fsim, n_frames * width * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!compute_fp && P.ng) PCR_HIP(ctx, hipMemcpyAsync(tp_scores, P.scores, P.ng * 8, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_kitti_thresholds_f64(pcr_ctx* ctx, const double* scores, size_t n, uint64_t n_gt, double* thresholds, int32_t* count)
{
    if (count) *count = 0;
    if (!ctx || !thresholds || !count || (n && !scores)) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_thresholds_f64");
    if (n > KE_MAX_ROWS) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_thresholds_f64: more than 2^22 scores");
    for (size_t i = 0; i < n; i++)
        if (scores[i] != scores[i]) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_thresholds_f64: a NaN score");
    if (n == 0) return PCR_OK;
    KePlan P;
    P.who = "pcr_kitti_thresholds_f64";
    const uint64_t ptr[2] = { 0, n };                                       // the scores ride in the slots of one frame's ground truth
    const uint64_t none[2] = { 0, 0 };
    const bool metrics[3] = { false, false, false };
    std::vector<double> rows(15 * n, 0.0);
    int rc = ke_prepare(ctx, P, 0, rows.data(), ptr, nullptr, none, 1, metrics, 0, 1);
    if (rc) return rc;
    rc = ke_upload(ctx, P);
    if (rc) return rc;
    const uint32_t n32 = (uint32_t)n;
    PCR_HIP(ctx, hipMemcpyAsync(P.pool, scores, n * 8, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(P.n_scores, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));                        // (pageable sources: the copies have read them)
    const double ngt[1] = { (double)n_gt };
    ke_launch_thresholds(ctx, P, 1, ngt, n);
    char* down;
    rc = ke_download(ctx, P, &down);
    if (rc) return rc;
    const int32_t np = *ke_down(P, ctx, down, P.n_pick);
    if (np < 0 || np > KE_NT) return fail(ctx, PCR_ERR_STATE, "pcr_kitti_thresholds_f64: corrupt count");
    memcpy(thresholds, ke_down(P, ctx, down, P.thr), (size_t)np * 8);
    *count = np;
    return PCR_OK;
}

extern "C" int pcr_kitti_eval_f64(pcr_ctx* ctx, int cls, int compute_aos, const double* gt_rows, const uint64_t* gt_ptr, const double* det_rows,
                                  const uint64_t* det_ptr, size_t n_frames, pcr_kitti_curve* out)
{
    if (!ctx || !out) return fail(ctx, PCR_ERR_ARG, "pcr_kitti_eval_f64");
    KePlan P;
    P.who = "pcr_kitti_eval_f64";
    const bool metrics[3] = { true, true, true };
    int rc = ke_prepare(ctx, P, cls, gt_rows, gt_ptr, det_rows, det_ptr, n_frames, metrics, KE_NCOMBO, KE_NCOMBO);
    if (rc) return rc;
    rc = ke_upload(ctx, P);
    if (rc) return rc;
    for (int m = 0; m < 3; m++) ke_launch_overlap(ctx, P, m, -1, P.ov[m]);
    KeArgs A = ke_args(P, cls);
    A.n_combo = KE_NCOMBO;
    double n_gt[KE_NCOMBO];
    for (int cb = 0; cb < KE_NCOMBO; cb++) {
        A.metric[cb] = cb / 3;
        A.diff[cb] = cb % 3;
        A.aos[cb] = compute_aos && cb / 3 == PCR_KITTI_IMAGE;
        n_gt[cb] = (double)P.n_gt[cb % 3];
    }
    A.n_scores = P.n_scores;
    A.pool = P.pool;
    ke_launch_match<false>(ctx, P, A);
    ke_launch_thresholds(ctx, P, KE_NCOMBO, n_gt, P.ng);
    A.thr = P.thr; A.n_thr = P.n_pick; A.tot = P.tot;
    ke_launch_match<true>(ctx, P, A);
    char* down;
    rc = ke_download(ctx, P, &down);                                        // the one wait of the call
    if (rc) return rc;
    const unsigned long long* tot = ke_down(P, ctx, down, P.tot);
    const double* thr = ke_down(P, ctx, down, P.thr);
    const int32_t* n_pick = ke_down(P, ctx, down, P.n_pick);
    for (int cb = 0; cb < KE_NCOMBO; cb++) {
        pcr_kitti_curve& c = out[cb];
        memset(&c, 0, sizeof(c));
        c.n_gt = P.n_gt[cb % 3];
        const int nt = n_pick[cb];
        if (nt < 0 || nt > KE_NT) return fail(ctx, PCR_ERR_STATE, "pcr_kitti_eval_f64: corrupt threshold count");
        c.n_thresholds = nt;
        c.has_aos = A.aos[cb];
        for (int t = 0; t < nt; t++) {
            const unsigned long long* q = tot + ((size_t)cb * KE_NT + t) * 4;
            c.thresholds[t] = thr[cb * KE_NT + t];
            c.tp[t] = (int64_t)q[0];
            c.fp[t] = (int64_t)q[1];
            c.fn[t] = (int64_t)q[2];
            c.similarity[t] = (double)(int64_t)q[3] / KE_SIM_GRID;
            c.precision[t] = (double)c.tp[t] / (double)(c.tp[t] + c.fp[t]);
            if (c.has_aos) c.aos[t] = c.similarity[t] / (double)(c.tp[t] + c.fp[t]);
        }
        for (int t = 0; t < nt; t++) {                                      // max_{i..end}: over all 41 entries, zeros beyond the last threshold included
            c.precision[t] = *std::max_element(c.precision + t, c.precision + KE_NT);
            if (c.has_aos) c.aos[t] = *std::max_element(c.aos + t, c.aos + KE_NT);
        }
    }
    return PCR_OK;
}
