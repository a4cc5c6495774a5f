// kabsch.hip — the streaming (HBM-bound) passes of one ICP iteration on gfx950:
//   * kabsch_partial_kernel / kabsch_final_kernel: A7 accumulation — the sums of p, q and q p^T over the kept pairs
//     (Homework9/hw9/src/registration.cpp:936-940,964-985).  The sums are EXACT and therefore independent of the order of the
//     additions: every term is cut into 40-bit integer limbs on one fixed-point grid (numerics.hpp), integer partial sums are
//     reduced per wavefront with DPP shuffles, per workgroup through LDS, across workgroups by one final workgroup and across
//     ranks by the one all-reduce of the iteration, with carry propagation between the levels.  The same bits come out for
//     any launch geometry, any visiting order of the queries (original order, cell order) and any number of GPUs.
//     Algorithmic traffic: 28 B per kept pair (12 B source + 8 B key + 12 B gathered target - the key carries idx and d2).
//   * transform_kernel: A8 transformCloudInplace (registration.cpp:165-178), f32, unfused, in place,
//     24 B per point, float4-vectorised over the SoA arrays.
#include "grid_common.hpp"
#include "icp_finish.hpp"
#include "numerics.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>

#pragma clang fp contract(off)

namespace pcr {

constexpr int KB_BLOCK = 256;
constexpr int KB_NV = 16;             // 3 + 3 + 9 sums + count
// (KB_NL, KB_ROW, KB_NLC — the limbs and slots of a partial row — and the steps from a reduced row to the new loop state: icp_finish.hpp)
constexpr int KB_MAX_BLOCKS = 8192;   // == the capacity of ctx->partials (api.cpp)
static_assert(KB_ROW * KB_MAX_BLOCKS == 8192 * 58, "api.cpp sizes ctx->partials as 8192 x 58 doubles");

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// one coordinate term into its two limbs (y = v * 2^(80 - e), |y| < 2^80)
__device__ __forceinline__ void acc2(double v, double sc, double& a0, double& a1)
{
    const double y = v * sc;                                  // exact: power of two
    const double l1 = trunc(y * num::KB_2mW);
    const double r = fma(-l1, num::KB_2W, y);                 // exact remainder, |r| < 2^40
    a1 += l1;
    a0 += trunc(r);
}

// one product term into its three limbs (y = v * 2^(120 - 2e), |y| < 2^120)
__device__ __forceinline__ void acc3(double v, double sp, double& a0, double& a1, double& a2)
{
    const double y = v * sp;
    const double l2 = trunc(y * (num::KB_2mW * num::KB_2mW));
    const double r = fma(-l2, num::KB_2W * num::KB_2W, y);    // |r| < 2^80
    const double l1 = trunc(r * num::KB_2mW);
    const double r2 = fma(-l1, num::KB_2W, r);                // |r2| < 2^40
    a2 += l2;
    a1 += l1;
    a0 += trunc(r2);
}

// the workgroup's reduction of the per-thread limbs: tn[KB_NL] (normalised per thread) -> row[] in LDS, normalised again
__host__ __device__ constexpr bool is_carry_slot(int k) { return k < 18 ? (k % 3 == 2) : (k < 54 && (k - 18) % 4 == 3); }

// Wave totals of N values per lane by a butterfly that HALVES what a lane holds at every step: with partner distance D the lanes
// whose bit D is clear keep the lower half of their values and send the upper half, the others the reverse; both add what they
// receive.  After the six steps lane l holds the wave's total of ONE value, number slot(l) (or nothing: slot < 0) — N - 1 + (a few
// for odd halves) exchanged values per lane in all, where one shuffle tree per value costs 6 N: 41 against 240 for the 40 limbs of
// the usual case.  The totals are integers below 2^53, so the order of the additions does not matter (numerics.hpp).
template <int N, int D>
__device__ __forceinline__ void bfly_halve(double (&v)[KB_NL], bool up)
{
    constexpr int H = (N + 1) / 2;
#pragma unroll
    for (int i = 0; i < H; i++) {
        const double a = v[i], b = (H + i < N) ? v[H + i] : 0.0;
        const double send = up ? a : b, keep = up ? b : a;
        v[i] = keep + __shfl_xor(send, D, 64);
    }
}

template <int N>
__device__ __forceinline__ int wave_totals(double (&v)[KB_NL], int lane)
{
    static_assert(N >= 1 && N <= 64, "six halvings must leave one value");
    constexpr int N1 = (N + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, N4 = (N3 + 1) / 2, N5 = (N4 + 1) / 2;
    bfly_halve<N, 32>(v, (lane & 32) != 0);
    bfly_halve<N1, 16>(v, (lane & 16) != 0);
    bfly_halve<N2, 8>(v, (lane & 8) != 0);
    bfly_halve<N3, 4>(v, (lane & 4) != 0);
    bfly_halve<N4, 2>(v, (lane & 2) != 0);
    bfly_halve<N5, 1>(v, (lane & 1) != 0);
    // which value this lane ended up with: its position in the arrays of the six steps, innermost first
    int p = 0;
    bool ok = true;
    p += (lane & 1) ? (N5 + 1) / 2 : 0;  ok = ok && p < N5;
    p += (lane & 2) ? (N4 + 1) / 2 : 0;  ok = ok && p < N4;
    p += (lane & 4) ? (N3 + 1) / 2 : 0;  ok = ok && p < N3;
    p += (lane & 8) ? (N2 + 1) / 2 : 0;  ok = ok && p < N2;
    p += (lane & 16) ? (N1 + 1) / 2 : 0; ok = ok && p < N1;
    p += (lane & 32) ? (N + 1) / 2 : 0;  ok = ok && p < N;
    return ok ? p : -1;
}

// carries: false when the carry slots of tn[] are known to be zero (no per-thread normalisation): they are not exchanged at all
// BFLY: the halving butterfly over the 40 live limbs (needs carries == false); it keeps all of them in registers at once (~160
// VGPRs), so only the instance for few terms per thread — where the reduction IS the pass — is built with it
// WAVES: the wavefronts of the workgroup (the sums are exact integers: any grouping gives the same row)
// NORM: false leaves row[] as the workgroup's plain totals (carry slots zero) for a caller that hands them on as integers (icp_sums_solve_kernel)
template <bool BFLY, int WAVES = KB_BLOCK / 64, bool NORM = true>
__device__ __forceinline__ void block_reduce_limbs(double (&tn)[KB_NL], unsigned long long lastkey, int overflow,
                                                   double (&red)[WAVES][KB_NL], double (&row)[KB_ROW], bool carries)
{
    __shared__ unsigned long long red_key[WAVES];
    __shared__ int red_ovf[WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (!BFLY) {
#pragma unroll
        for (int k = 0; k < KB_NL; k++) {
            double sum = 0.0;
            if (carries || !is_carry_slot(k)) sum = wave_sum(tn[k]);      // 64 integers below 2^46 (+ small carries): exact
            if (lane == 0) red[wave][k] = sum;
        }
    } else {
        int j = 0;
#pragma unroll
        for (int k = 0; k < KB_NL; k++)
            if (!is_carry_slot(k)) tn[j++] = tn[k];                       // compact: the 40 live limbs (static indices)
        const int p = wave_totals<KB_NLC>(tn, lane);
        if (p >= 0) {
            // live limb p -> its slot of the row: coordinates 2 of every 3 slots, products 3 of every 4, the count last
            const int slot = p < 12 ? 3 * (p / 2) + p % 2 : (p < 39 ? 18 + 4 * ((p - 12) / 3) + (p - 12) % 3 : 54);
            red[wave][slot] = tn[0];
        }
        if (lane < 15) red[wave][lane < 6 ? 3 * lane + 2 : 18 + 4 * (lane - 6) + 3] = 0.0;      // the 15 carry slots
    }
    const unsigned long long km = wave_max_u64(lastkey);
    const int ov = __any(overflow) ? 1 : 0;
    if (lane == 0) { red_key[wave] = km; red_ovf[wave] = ov; }
    __syncthreads();
    if (threadIdx.x < KB_NL) {
        const int k = threadIdx.x;
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < WAVES; w++) t += red[w][k];
        row[k] = t;
    } else if (threadIdx.x == KB_NL) {
        unsigned long long m = red_key[0];
        int ov = red_ovf[0];
        for (int w = 1; w < WAVES; w++) { m = red_key[w] > m ? red_key[w] : m; ov |= red_ovf[w]; }
        row[55] = __longlong_as_double((long long)m);
        row[56] = ov ? 1.0 : 0.0;
        row[57] = 0.0;
    }
    __syncthreads();
    if (!NORM) return;
    if (threadIdx.x < 6) num::limbs_normalize(row + 3 * threadIdx.x, 2);
    else if (threadIdx.x < 15) num::limbs_normalize(row + 18 + 4 * (threadIdx.x - 6), 3);
    __syncthreads();
}

// partials layout: [block][KB_ROW].  RECORDS: the target of pair i is grid record wpos[i] (one 16-byte gather from the cell-
// sorted records, which neighbouring queries share) instead of the three 4-byte gathers at its original index.
// orig: original index of query i (the working cloud of the grid ICP is cell-sorted) or nullptr = i.
// SMALL: at most 4 pairs per thread (clouds up to ~1 M points): no per-thread carries, butterfly reduction.
template <bool RECORDS, bool SMALL>
__global__ __launch_bounds__(KB_BLOCK) void kabsch_partial_kernel(
    const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
    const float4* __restrict__ records, const uint32_t* __restrict__ wpos, const uint32_t* __restrict__ orig,
    const unsigned long long* __restrict__ keys, uint32_t ns, uint32_t nt, float max_corr, KabschPlan plan,
    double* __restrict__ partials)
{
    double c0[6], c1[6], p0[9], p1[9], p2[9], cnt = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) { c0[k] = 0.0; c1[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 9; k++) { p0[k] = 0.0; p1[k] = 0.0; p2[k] = 0.0; }
    unsigned long long lastkey = 0;
    int overflow = 0;
    // contiguous chunk per block, strided by lane inside it (coalesced); the order does not matter for the result
    const uint32_t per_block = (ns + gridDim.x - 1) / gridDim.x;
    const uint32_t lo = min(blockIdx.x * per_block, ns);
    const uint32_t hi = min(lo + per_block, ns);
    // Software pipeline: the coalesced loads of the NEXT pair are requested before the current one is consumed, and the target gather
    // of the current pair is issued first thing, unconditionally (clamped position): one exposed round trip per iteration instead of
    // two, twice the bytes in flight per wave (the pass is bound by latency x bytes in flight, not by bandwidth: DESIGN.md 6b).
    uint32_t i = lo + threadIdx.x;
    unsigned long long key_n = 0;
    float p_n0 = 0.f, p_n1 = 0.f, p_n2 = 0.f;
    uint32_t wp_n = 0, og_n = i;
    if (i < hi) {
        key_n = keys[i]; p_n0 = sx[i]; p_n1 = sy[i]; p_n2 = sz[i];
        if (RECORDS) wp_n = wpos[i];
        if (orig) og_n = orig[i];
    }
    const uint32_t last_rec = nt ? nt - 1 : 0u;
    for (; i < hi; i += KB_BLOCK) {
        const unsigned long long key = key_n;
        const float pf0 = p_n0, pf1 = p_n1, pf2 = p_n2;
        const uint32_t og = og_n;
        float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RECORDS) rec = records[min(wp_n, last_rec)];
        const uint32_t in = i + KB_BLOCK;
        if (in < hi) {
            key_n = keys[in]; p_n0 = sx[in]; p_n1 = sy[in]; p_n2 = sz[in];
            if (RECORDS) wp_n = wpos[in];
            og_n = orig ? orig[in] : in;
        }
        const uint32_t d2b = (uint32_t)(key >> 32);
        const float d2 = __uint_as_float(d2b);
        const uint32_t j = (uint32_t)(key & 0xFFFFFFFFull);
        if (d2 < max_corr && j < nt) {                       // registration.cpp:936
            float qf0, qf1, qf2;
            if (RECORDS) {
                qf0 = rec.x; qf1 = rec.y; qf2 = rec.z;
            } else {
                qf0 = tx[j]; qf1 = ty[j]; qf2 = tz[j];
            }
            // 2^e bounds every coordinate of a kept pair (kabsch_plan); a source beyond it would overflow its limbs
            if (!(fabsf(pf0) < plan.lim && fabsf(pf1) < plan.lim && fabsf(pf2) < plan.lim)) { overflow = 1; continue; }
            const double P[3] = { pf0, pf1, pf2 }, Q[3] = { qf0, qf1, qf2 };
#pragma unroll
            for (int c = 0; c < 3; c++) { acc2(P[c], plan.sc, c0[c], c1[c]); acc2(Q[c], plan.sc, c0[3 + c], c1[3 + c]); }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) acc3(Q[r] * P[c], plan.sp, p0[3 * r + c], p1[3 * r + c], p2[3 * r + c]);
            cnt += 1.0;
            // the LAST kept pair of the reference's loop (registration.cpp:939) = the kept pair with the highest original index
            const unsigned long long lk = ((unsigned long long)og << 32) | d2b;
            lastkey = lk > lastkey ? lk : lastkey;
        }
    }
    // per-thread carry propagation only when a thread may hold many terms (limbs below 2^40 x terms must stay below 2^53 through
    // the 256-thread sum): at most 16 terms per thread need none
    const bool many = !SMALL && per_block > 16u * KB_BLOCK;
    double tn[KB_NL];
#pragma unroll
    for (int c = 0; c < 6; c++) { tn[3 * c] = c0[c]; tn[3 * c + 1] = c1[c]; tn[3 * c + 2] = 0.0; if (many) num::limbs_normalize(tn + 3 * c, 2); }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        tn[18 + 4 * k] = p0[k]; tn[19 + 4 * k] = p1[k]; tn[20 + 4 * k] = p2[k]; tn[21 + 4 * k] = 0.0;
        if (many) num::limbs_normalize(tn + 18 + 4 * k, 3);
    }
    tn[54] = cnt;
    __shared__ double red[KB_BLOCK / 64][KB_NL];
    __shared__ double row[KB_ROW];
    block_reduce_limbs<SMALL>(tn, lastkey, overflow, red, row, many);
    if (threadIdx.x < KB_ROW) partials[(size_t)blockIdx.x * KB_ROW + threadIdx.x] = row[threadIdx.x];
}

// one workgroup of KF_BLOCK threads = 16 groups of 64 lanes: the block rows -> ONE normalised row in LDS (limbs, last-kept key,
// overflow flag).  Lane k of a group owns column k (coalesced 464-byte row reads), group g takes rows g, g + 16, ...; column sums
// of <= 1024 integers below 2^40 are exact.  Thread k < 16 then converts moment k: out[0..15] = the moments,
// [16] original index of the last kept pair or -1, [17] its d2, [18] overflow flag.
constexpr int KF_BLOCK = 1024;
constexpr int KF_GROUPS = KF_BLOCK / 64;

// (GROUPS: the wavefronts of the calling workgroup, 16 for the KF_BLOCK kernels)
template <int GROUPS = KF_GROUPS>
__device__ __forceinline__ void reduce_rows(const double* __restrict__ partials, uint32_t n_blocks, double (&red)[GROUPS][64], double (&row)[KB_ROW])
{
    const int k = threadIdx.x & 63, grp = threadIdx.x >> 6;
    double acc = 0.0;
    unsigned long long key = 0;
    if (k < 57) {
        // more rows than groups: eight rows of a group in flight at once (a row that does not exist reads as 0.0, neutral for the sum,
        // the key maximum and the flag alike) — one memory round trip per eight rows instead of one per row; the additions are exact,
        // any order.  Few rows (small clouds, where this kernel is pure latency): the one-row loop, a fraction of the code to fetch.
        if (n_blocks <= (uint32_t)GROUPS) {
            if ((uint32_t)grp < n_blocks) {
                const double v = partials[(size_t)grp * KB_ROW + k];
                if (k == 55) key = (unsigned long long)__double_as_longlong(v);
                else if (k == 56) acc = v != 0.0 ? 1.0 : 0.0;
                else acc = v;
            }
        } else {
            constexpr int INF = 8;
            for (uint32_t b = grp; b < n_blocks; b += GROUPS * INF) {
                double v[INF];
#pragma unroll
                for (int j = 0; j < INF; j++) {
                    const uint32_t bb = b + (uint32_t)j * GROUPS;
                    v[j] = bb < n_blocks ? partials[(size_t)bb * KB_ROW + k] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < INF; j++) {
                    if (k == 55) { const unsigned long long lk = (unsigned long long)__double_as_longlong(v[j]); key = lk > key ? lk : key; }
                    else if (k == 56) acc = (acc != 0.0 || v[j] != 0.0) ? 1.0 : 0.0;
                    else acc += v[j];
                }
            }
        }
    }
    red[grp][k] = k == 55 ? __longlong_as_double((long long)key) : acc;
    __syncthreads();
    if (threadIdx.x < 57) {
        const int c = threadIdx.x;
        if (c == 55) {
            unsigned long long m = 0;
            for (int g = 0; g < GROUPS; g++) { const unsigned long long lk = (unsigned long long)__double_as_longlong(red[g][c]); m = lk > m ? lk : m; }
            row[c] = __longlong_as_double((long long)m);
        } else {
            double t = 0.0;
            for (int g = 0; g < GROUPS; g++) t += red[g][c];
            row[c] = c == 56 ? (t != 0.0 ? 1.0 : 0.0) : t;
        }
    }
    if (threadIdx.x == 57) row[57] = 0.0;
    __syncthreads();
    if (threadIdx.x < 6) num::limbs_normalize(row + 3 * threadIdx.x, 2);
    else if (threadIdx.x < 15) num::limbs_normalize(row + 18 + 4 * (threadIdx.x - 6), 3);
    __syncthreads();
}

__global__ __launch_bounds__(KF_BLOCK) void kabsch_final_kernel(const double* __restrict__ partials, uint32_t n_blocks, int e, double* __restrict__ out)
{
    __shared__ double red[KF_GROUPS][64];
    __shared__ double row[KB_ROW];
    reduce_rows(partials, n_blocks, red, row);
    row_to_out18(row, e, out);
}

// the order of the additions does not matter any more; the geometry only has to keep the pass busy: one pair per thread while
// that needs few workgroups (the pass is latency-bound at 120 k), then a capped number of fatter workgroups — every workgroup
// ends in a 464-byte row that ONE workgroup has to reduce afterwards (8 192 rows cost 0.22 ms at 10 M, 1 024 rows 0.05 ms, and the pass itself runs 0.27 -> 0.14 ms)
static uint32_t kabsch_blocks(pcr_ctx* ctx, size_t ns)
{
    // one pair per thread up to 128 workgroups, then four pairs per thread, then the cap: at 120 k the 469 rows of the one-pair rule
    // cost the reduce 24 us against 15 us for 128 rows, the pass itself the same 18 us (profiles/r02_kabsch_probes.txt)
    uint32_t blocks = (uint32_t)((ns + KB_BLOCK - 1) / KB_BLOCK);
    const uint32_t one_pair = (uint32_t)std::min<int64_t>(KB_MAX_BLOCKS, std::max<int64_t>(1, tune_get(ctx, "kabsch_one_pair_blocks", 128)));
    if (blocks > one_pair) blocks = std::max<uint32_t>(one_pair, (uint32_t)((ns + 4 * KB_BLOCK - 1) / (4 * KB_BLOCK)));
    if (blocks < 1) blocks = 1;
    // (round 4: at most one workgroup per 2 048 pairs as well — a 1 / 8 shard of the 10 M pair ran 1 024 workgroups of 1 220 pairs and its solve reduced
    // 1 024 rows: 0.370 -> 0.352 ms per iteration with 610; the 10 M pair itself stays at the cap)
    const int64_t cap_t = tune_get(ctx, "kabsch_max_blocks", 0);
    const uint32_t cap = (uint32_t)std::min<int64_t>(KB_MAX_BLOCKS, std::max<int64_t>(1, cap_t > 0 ? cap_t : std::min<int64_t>(1024, std::max<int64_t>(128, (int64_t)(ns / 2048)))));
    if (blocks > cap) blocks = cap;
    // exactness before tuning: a thread's limb accumulators are normalised only after its whole chunk, every term adds < 2^40 to
    // each, so a thread may hold < 2^13 terms: never fewer workgroups than 4 096 pairs per thread need (10 M points: 10)
    const uint32_t need = (uint32_t)((ns + (size_t)4096 * KB_BLOCK - 1) / ((size_t)4096 * KB_BLOCK));
    if (blocks < need) blocks = need;
    return blocks;
}

// The fixed-point grid of one accumulation.  Every coordinate of a KEPT pair is bounded by what is known up front and is the
// same on every rank: the target's largest finite |coordinate| (cached on the cloud) plus the gate — a pair is kept only if
// d2 < max_corr (registration.cpp:936), so |p - q| < sqrt(max_corr).  An unbounded gate is capped at 2^20 target extents;
// a kept source beyond 2^e then raises the overflow flag (PCR_ERR_STATE) instead of a wrong sum.
int kabsch_grid_exponent(float amax, float max_corr)
{
    const double a = std::max((double)amax, 1e-30);
    double gate = max_corr > 0.f ? 2.0 * std::sqrt((double)max_corr) : 0.0;     // NaN / <= 0: no pair is kept anyway
    if (!(gate <= a * 1048576.0)) gate = a * 1048576.0;
    const double M = a + gate;
    int e = std::ilogb(M) + 2;                                                      // 2^e > 2 M
    if (e > 140) e = 140;
    return e;
}

int kabsch_plan(pcr_ctx* ctx, const pcr_cloud* tgt, float max_corr, KabschPlan* plan)
{
    float amax = 0.f;
    int rc = cloud_absmax(ctx, tgt, &amax);
    if (rc) return rc;
    const int e = kabsch_grid_exponent(amax, max_corr);
    plan->e = e;
    plan->lim = e >= 128 ? __builtin_inff() : std::ldexp(1.0f, e);
    plan->sc = std::ldexp(1.0, 2 * num::KB_W - e);
    plan->sp = std::ldexp(1.0, 3 * num::KB_W - 2 * e);
    return PCR_OK;
}

int launch_kabsch_partial(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr, const KabschPlan& plan, uint32_t* n_blocks)
{
    const size_t ns = src->n;
    if (ctx->keys_n != ns) return fail(ctx, PCR_ERR_STATE, "kabsch: no matching correspondence pass");
    const uint32_t blocks = kabsch_blocks(ctx, ns);
    // the grid search of an ICP loop leaves the record position of every winner behind (ctx->wpos): gather from the records
    // — of THIS target's grid as it is now (wpos_is_of): after a rebuild the same positions name other points
    const bool rec = wpos_is_of(ctx, tgt, ns) && tgt->grid->records && tune_get(ctx, "kabsch_records", 1) == 1;
    const uint32_t* orig = src->orig;     // (the cloud's own mapping: no other call on the context resets it — test_context_state.py §B)
    {
        ProfScope p(ctx, "kabsch_partial");
        const uint32_t per_block = (uint32_t)((ns + blocks - 1) / blocks);      // as the kernel computes it
        const bool small = per_block <= 4u * KB_BLOCK && tune_get(ctx, "kabsch_bfly", 1) == 1;
#define PCR_KABSCH(R, S, RECS, WPOS)                                                                                                      \
        hipLaunchKernelGGL((kabsch_partial_kernel<R, S>), dim3(blocks), dim3(KB_BLOCK), 0, ctx->stream, src->x(), src->y(), src->z(), tgt->x(),  \
                           tgt->y(), tgt->z(), RECS, WPOS, orig, ctx->keys, (uint32_t)ns, (uint32_t)tgt->n, max_corr, plan, ctx->partials)
        if (rec) { if (small) PCR_KABSCH(true, true, tgt->grid->records, ctx->wpos); else PCR_KABSCH(true, false, tgt->grid->records, ctx->wpos); }
        else { if (small) PCR_KABSCH(false, true, (const float4*)nullptr, (const uint32_t*)nullptr); else PCR_KABSCH(false, false, (const float4*)nullptr, (const uint32_t*)nullptr); }
#undef PCR_KABSCH
    }
    PCR_HIP(ctx, hipGetLastError());
    *n_blocks = blocks;
    return PCR_OK;
}

// dev_out[0..18] = moments, last kept (original index, d2), overflow flag
int launch_kabsch_sums(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr, const KabschPlan& plan)
{
    uint32_t blocks = 0;
    int rc = launch_kabsch_partial(ctx, tgt, src, max_corr, plan, &blocks);
    if (rc) return rc;
    {
        ProfScope p(ctx, "kabsch_final");
        hipLaunchKernelGGL(kabsch_final_kernel, dim3(1), dim3(KF_BLOCK), 0, ctx->stream, ctx->partials, blocks, plan.e, ctx->dev_out);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// ---------------------------------------------------------------------------------------------- device-resident ICP state
// (icp_state_step_wave — state machine + Kabsch solve + pose composition, by the first wave of the kernels below, DESIGN.md 6l — and ST_WORDS: icp_finish.hpp)

// the whole state in ONE coalesced read: thread w copies 32-bit word w into the workgroup's LDS copy (ends in a barrier)
__device__ __forceinline__ void icp_state_stage(const IcpState* st, IcpState* lds)
{
    if (threadIdx.x < ST_WORDS)
        __builtin_memcpy(reinterpret_cast<char*>(lds) + 4 * threadIdx.x, reinterpret_cast<const char*>(st) + 4 * threadIdx.x, 4);
    __syncthreads();
}

// single rank: reduce the block rows and advance the state in one launch
__global__ __launch_bounds__(KF_BLOCK) void icp_update_kernel(const double* __restrict__ partials, uint32_t n_blocks, int e, IcpState* st,
                                                              double* __restrict__ out)
{
    __shared__ double red[KF_GROUPS][64];
    __shared__ double row[KB_ROW];
    __shared__ double o18[19];
    __shared__ IcpState s_st;
    icp_state_stage(st, &s_st);
    if (s_st.stop) return;
    if (s_st.stop_after_transform) { if (threadIdx.x == 0) st->stop = 1; return; }
    reduce_rows(partials, n_blocks, red, row);
    row_to_out18(row, e, o18);
    __syncthreads();
    if (threadIdx.x < 19) out[threadIdx.x] = o18[threadIdx.x];
    if (threadIdx.x < 64) {                    // the first wave, whole (icp_finish.hpp icp_state_step_wave)
        icp_state_step_wave((int)threadIdx.x, &s_st, o18, o18[16] >= 0.0, (float)o18[17], o18[18] != 0.0);
        if (threadIdx.x == 0) *st = s_st;
    }
}

// The seed of the NEXT exhaustive search, computed where the point moves (round 3: one launch less per iteration than nn1_seed_kernel
// in front of every warm search, nn1_brute.hip): keys[] holds this iteration's correspondence of point i; that target, evaluated with
// the exact A1 arithmetic against the point's NEW position, is a genuine candidate of the next search and therefore an upper bound of
// its answer from the first instruction on.  Same values as nn1_seed_kernel writes (a correspondence that is not acceptable any more,
// or none at all, leaves "no claim").
struct SeedArgs {
    const float* tx; const float* ty; const float* tz;     // the target cloud (nullptr: no seeding)
    unsigned long long* keys;
    uint32_t nt;
};

__device__ __forceinline__ void seed_next_search(const SeedArgs& sd, uint32_t i, uint32_t n, float x, float y, float z)
{
    if (i >= n) return;
    const uint32_t j = (uint32_t)(sd.keys[i] & 0xFFFFFFFFull);
    unsigned long long key = ~0ull;
    if (j < sd.nt) {
        const float dx = x - sd.tx[j], dy = y - sd.ty[j], dz = z - sd.tz[j];
        const uint32_t e = __float_as_uint((dx * dx + dy * dy) + dz * dz);       // A1, unfused (nanoflann.hpp:403-406)
        if (e < 0x7F7FFFFFu) key = ((unsigned long long)e << 32) | j;              // FLT_MAX gate, nanoflann.hpp:163,1360
    }
    sd.keys[i] = key;
}

// Small clouds, single rank: the solve AND the move in one launch — one link less in the latency chain of an iteration
// (search -> sums -> solve -> move), which is all an iteration is at hw9's own size.  Every workgroup repeats the reduce and the 3 x 3
// solve on its own LDS copy of the state it read from st_in (deterministic arithmetic on the same rows: all of them arrive at the
// same new state), workgroup 0 publishes it to st_out — the OTHER buffer of a pair, so nobody reads what is being written; the
// next search tests the stop flags there — and each workgroup moves its own 4 096 points, whose loads were issued before the solve.
// The exits are those of icp_update_kernel + transform_state_kernel: a stopped loop stays as it is, stop_after_transform turns
// into stop without a move, a step that stops (converged, no pair, overflow) does not move, any other step moves.
__global__ __launch_bounds__(KF_BLOCK) void icp_update_move_kernel(const double* __restrict__ partials, uint32_t n_blocks, int e, const IcpState* __restrict__ st_in,
                                                                   IcpState* __restrict__ st_out, double* __restrict__ out, float* __restrict__ x,
                                                                   float* __restrict__ y, float* __restrict__ z, uint32_t n, uint32_t n4, SeedArgs sd)
{
    __shared__ double red[KF_GROUPS][64];
    __shared__ double row[KB_ROW];
    __shared__ double o18[19];
    __shared__ IcpState s_st;
    const uint32_t i = blockIdx.x * KF_BLOCK + threadIdx.x;
    const bool mine = i < n4;
    float4 px = make_float4(0.f, 0.f, 0.f, 0.f), py = px, pz = px;
    if (mine) { px = reinterpret_cast<float4*>(x)[i]; py = reinterpret_cast<float4*>(y)[i]; pz = reinterpret_cast<float4*>(z)[i]; }
    // the seeds of the next search (seed_next_search): the previous correspondences and their target points do not depend on the new pose — requested
    // here, in front of the reduce and the solve, so that the two dependent trips to memory (key -> target point) are over when the move is done
    unsigned long long sk[4] = { ~0ull, ~0ull, ~0ull, ~0ull };
    float sq[4][3] = { { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f } };
    if (sd.tx && mine) {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (4 * i + u < n) sk[u] = sd.keys[4 * i + u];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t j = (uint32_t)(sk[u] & 0xFFFFFFFFull);
            if (j < sd.nt) { sq[u][0] = sd.tx[j]; sq[u][1] = sd.ty[j]; sq[u][2] = sd.tz[j]; }
        }
    }
    icp_state_stage(st_in, &s_st);
    const int phase = s_st.stop ? 0 : (s_st.stop_after_transform ? 1 : 2);       // (uniform over the workgroup)
    if (phase == 2) {
        reduce_rows(partials, n_blocks, red, row);
        row_to_out18(row, e, o18);
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x < 19) out[threadIdx.x] = o18[threadIdx.x];
        if (threadIdx.x < 64) icp_state_step_wave((int)threadIdx.x, &s_st, o18, o18[16] >= 0.0, (float)o18[17], o18[18] != 0.0);
    } else if (phase == 1) {
        if (threadIdx.x == 0) s_st.stop = 1;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = s_st;
    if (s_st.stop || !mine) return;
    const float r0 = s_st.Rd[0], r1 = s_st.Rd[1], r2 = s_st.Rd[2], r3 = s_st.Rd[3], r4 = s_st.Rd[4], r5 = s_st.Rd[5],
                r6 = s_st.Rd[6], r7 = s_st.Rd[7], r8 = s_st.Rd[8], t0 = s_st.td[0], t1 = s_st.td[1], t2 = s_st.td[2];
    float4 ox, oy, oz;
#define PCR_ROW(o, a, b, c, tt)                      \
    o.x = ((a * px.x + b * py.x) + c * pz.x) + tt;   \
    o.y = ((a * px.y + b * py.y) + c * pz.y) + tt;   \
    o.z = ((a * px.z + b * py.z) + c * pz.z) + tt;   \
    o.w = ((a * px.w + b * py.w) + c * pz.w) + tt;
    PCR_ROW(ox, r0, r1, r2, t0)
    PCR_ROW(oy, r3, r4, r5, t1)
    PCR_ROW(oz, r6, r7, r8, t2)
#undef PCR_ROW
    const uint32_t base = 4 * i;                     // (the padding invariant of the tail group: transform_state_kernel)
    if (base + 3 >= n) {
        const float inf = __builtin_inff();
        if (base + 0 >= n) { ox.x = inf; oy.x = 0.f; oz.x = 0.f; }
        if (base + 1 >= n) { ox.y = inf; oy.y = 0.f; oz.y = 0.f; }
        if (base + 2 >= n) { ox.z = inf; oy.z = 0.f; oz.z = 0.f; }
        if (base + 3 >= n) { ox.w = inf; oy.w = 0.f; oz.w = 0.f; }
    }
    reinterpret_cast<float4*>(x)[i] = ox;
    reinterpret_cast<float4*>(y)[i] = oy;
    reinterpret_cast<float4*>(z)[i] = oz;
    if (sd.tx) {
        const float mx[4] = { ox.x, ox.y, ox.z, ox.w }, my[4] = { oy.x, oy.y, oy.z, oy.w }, mz[4] = { oz.x, oz.y, oz.z, oz.w };
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (base + u >= n) continue;
            const uint32_t j = (uint32_t)(sk[u] & 0xFFFFFFFFull);
            unsigned long long key = ~0ull;
            if (j < sd.nt) {
                const float dx = mx[u] - sq[u][0], dy = my[u] - sq[u][1], dz = mz[u] - sq[u][2];
                const uint32_t e2 = __float_as_uint((dx * dx + dy * dy) + dz * dz);       // A1, unfused (nanoflann.hpp:403-406): seed_next_search's arithmetic
                if (e2 < 0x7F7FFFFFu) key = ((unsigned long long)e2 << 32) | j;            // FLT_MAX gate, nanoflann.hpp:163,1360
            }
            sd.keys[base + u] = key;
        }
    }
}

// Exhaustive and grid loops on one rank whose cloud fits one workgroup per CU: the SUMS as well — kabsch_partial_kernel<., true> + icp_update_move_kernel as
// ONE launch.  Both passes read the same three things per pair (key, source point, gathered target point); here a thread reads its four
// consecutive pairs once, adds their limbs exactly as the sums pass does, the workgroup writes its row, and all workgroups meet ONCE at a grid barrier —
// one monotonic counter, never reset: the host passes the value it has when everybody has arrived (the release / acquire hand-off: rows, the storing
// wave's vmcnt(0), an agent-scope release by the arriving lane, the add; waiters poll relaxed with s_sleep; one agent-scope acquire before the rows are
// read).  Behind it every workgroup reduces the gridDim.x rows, solves and moves its points from registers, as icp_update_move_kernel does.  The sums are
// exact integers, so the new grouping of the pairs changes no bit (6b).
// All workgroups are resident from the grid size alone: the host launches at most one per CU (icp_fused_sums_blocks).  EVERY workgroup arrives exactly once
// per launch, in every phase (a stopped loop's launches too: that keeps the counter in step with the host's count); only phase 2 waits.
// The spin is bounded: FS_SPIN_TICKS of s_memrealtime (100 MHz) = 50 ms.  A legitimate wait is the skew between the workgroups of one launch — all of them
// are dispatched within a microsecond and do a few microseconds of identical work — so three to four orders of magnitude lie between it and the bound, which
// also covers a chip that other processes keep busy for whole milliseconds; 50 ms per launch still ends a loop that can never meet within seconds.  On
// expiry the workgroup raises barrier_timeout in the state it hands on (the host turns it into PCR_ERR_STATE), stops the loop and does not move.
constexpr int FS_TMO_WORD = (int)(offsetof(IcpState, barrier_timeout) / 4);
constexpr unsigned long long FS_SPIN_TICKS = 5000000ull;
static_assert(KB_ROW <= 64, "one wave stores the workgroup's row and arrives for it");

template <int T>
__global__ __launch_bounds__(T) void icp_sums_update_move_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, const uint32_t* __restrict__ orig,
    unsigned long long* __restrict__ keys, uint32_t nt, float max_corr, KabschPlan plan, double* partials, unsigned long long* counter,
    unsigned long long target, const IcpState* __restrict__ st_in, IcpState* __restrict__ st_out, double* __restrict__ out, float* __restrict__ x,
    float* __restrict__ y, float* __restrict__ z, uint32_t n, uint32_t n4, int seed
#ifdef PCR_FS_PROF
    , unsigned long long* prof
#endif
    )
{
    constexpr int WAVES = T / 64;
    __shared__ double red_l[WAVES][KB_NL];
    __shared__ double red[WAVES][64];
    __shared__ double row[KB_ROW];
    __shared__ double o18[19];
    __shared__ IcpState s_st;
    __shared__ int s_tmo;
#ifdef PCR_FS_PROF
    const unsigned long long pt_a = __builtin_amdgcn_s_memrealtime();
    unsigned long long pt_b = pt_a;
#endif
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    const bool mine = i < n4;
    const uint32_t base = 4 * i;
    // everything that depends on nothing else is requested in one go, the state first: it is on the critical path and loads retire in order
    uint32_t stw = 0;
    if (threadIdx.x < ST_WORDS) stw = reinterpret_cast<const uint32_t*>(st_in)[threadIdx.x];
    float4 px = make_float4(0.f, 0.f, 0.f, 0.f), py = px, pz = px;
    unsigned long long sk[4] = { ~0ull, ~0ull, ~0ull, ~0ull };             // (no pair: NaN distance, no target)
    uint32_t og[4] = { base, base + 1, base + 2, base + 3 };
    if (mine) {
        px = reinterpret_cast<float4*>(x)[i]; py = reinterpret_cast<float4*>(y)[i]; pz = reinterpret_cast<float4*>(z)[i];
        if (base + 3 < n) {
            const ulonglong2 k01 = reinterpret_cast<const ulonglong2*>(keys)[2 * i], k23 = reinterpret_cast<const ulonglong2*>(keys)[2 * i + 1];
            sk[0] = k01.x; sk[1] = k01.y; sk[2] = k23.x; sk[3] = k23.y;
            if (orig) { const uint4 o = reinterpret_cast<const uint4*>(orig)[i]; og[0] = o.x; og[1] = o.y; og[2] = o.z; og[3] = o.w; }
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (base + u < n) { sk[u] = keys[base + u]; if (orig) og[u] = orig[base + u]; }
        }
    }
    // the target points of the four pairs, gathered ONCE: they serve the sums and the seeds of the next search
    float sq[4][3] = { { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f } };
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t j = (uint32_t)(sk[u] & 0xFFFFFFFFull);
        if (j < nt) { sq[u][0] = tx[j]; sq[u][1] = ty[j]; sq[u][2] = tz[j]; }
    }
    if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(&s_st)[threadIdx.x] = stw;
    __syncthreads();
    // uniform over the GRID: every workgroup reads the same st_in (a raised barrier_timeout ends the loop like a stop)
    const int phase = (s_st.stop || s_st.barrier_timeout) ? 0 : (s_st.stop_after_transform ? 1 : 2);
    if (phase == 2) {
        double c0[6], c1[6], p0[9], p1[9], p2[9], cnt = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) { c0[k] = 0.0; c1[k] = 0.0; }
#pragma unroll
        for (int k = 0; k < 9; k++) { p0[k] = 0.0; p1[k] = 0.0; p2[k] = 0.0; }
        unsigned long long lastkey = 0;
        int overflow = 0;
        const float sx4[4] = { px.x, px.y, px.z, px.w }, sy4[4] = { py.x, py.y, py.z, py.w }, sz4[4] = { pz.x, pz.y, pz.z, pz.w };
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t d2b = (uint32_t)(sk[u] >> 32);
            const float d2 = __uint_as_float(d2b);
            const uint32_t j = (uint32_t)(sk[u] & 0xFFFFFFFFull);
            if (d2 < max_corr && j < nt) {                       // registration.cpp:936 (kabsch_partial_kernel's gate, term for term)
                const float pf0 = sx4[u], pf1 = sy4[u], pf2 = sz4[u];
                if (!(fabsf(pf0) < plan.lim && fabsf(pf1) < plan.lim && fabsf(pf2) < plan.lim)) { overflow = 1; continue; }
                const double P[3] = { pf0, pf1, pf2 }, Q[3] = { sq[u][0], sq[u][1], sq[u][2] };
#pragma unroll
                for (int c = 0; c < 3; c++) { acc2(P[c], plan.sc, c0[c], c1[c]); acc2(Q[c], plan.sc, c0[3 + c], c1[3 + c]); }
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) acc3(Q[r] * P[c], plan.sp, p0[3 * r + c], p1[3 * r + c], p2[3 * r + c]);
                cnt += 1.0;
                const unsigned long long lk = ((unsigned long long)og[u] << 32) | d2b;
                lastkey = lk > lastkey ? lk : lastkey;
            }
        }
        double tn[KB_NL];                    // at most 4 terms per thread: no per-thread carries
#pragma unroll
        for (int c = 0; c < 6; c++) { tn[3 * c] = c0[c]; tn[3 * c + 1] = c1[c]; tn[3 * c + 2] = 0.0; }
#pragma unroll
        for (int k = 0; k < 9; k++) { tn[18 + 4 * k] = p0[k]; tn[19 + 4 * k] = p1[k]; tn[20 + 4 * k] = p2[k]; tn[21 + 4 * k] = 0.0; }
        tn[54] = cnt;
        block_reduce_limbs<true>(tn, lastkey, overflow, red_l, row, false);
#ifdef PCR_FS_PROF
        pt_b = __builtin_amdgcn_s_memrealtime();
#endif
        if (threadIdx.x < KB_ROW) partials[(size_t)blockIdx.x * KB_ROW + threadIdx.x] = row[threadIdx.x];
    }
    // ---- the barrier: wave 0 stored the row; it drains its stores, its lane 0 releases, arrives and (phase 2) waits
    if (threadIdx.x < 64) {
        if (phase == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            int tmo = 0;
            if (phase == 2) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (kept behind the fence whatever the compiler thinks of the scoreboard)
            }
            __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (phase == 2) {
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                    __builtin_amdgcn_s_sleep(2);
                    if (__builtin_amdgcn_s_memrealtime() - t0 > FS_SPIN_TICKS) { tmo = 1; break; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the invalidate is over before the barrier below lets the other waves read
#ifdef PCR_FS_PROF
                if (prof) {
                    const unsigned long long pt_c = __builtin_amdgcn_s_memrealtime();
                    atomicAdd(prof + 12, pt_c - pt_b); atomicMax(prof + 13, pt_c - pt_b); atomicAdd(prof + 14, 1ull); atomicAdd(prof + 15, pt_b - pt_a);
                }
#endif
            }
            s_tmo = tmo;
        }
    }
    __syncthreads();
    const bool tmo = s_tmo != 0;
    if (phase == 2 && !tmo) {
        reduce_rows(partials, gridDim.x, red, row);
        row_to_out18(row, plan.e, o18);
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x < 19) out[threadIdx.x] = o18[threadIdx.x];
        if (threadIdx.x < 64) icp_state_step_wave((int)threadIdx.x, &s_st, o18, o18[16] >= 0.0, (float)o18[17], o18[18] != 0.0);
    } else if (threadIdx.x == 0) {
        s_st.stop = 1;                         // (phase 0: stays stopped; phase 1: max_iter reached, the loop is over; timeout)
        if (tmo) {
            s_st.barrier_timeout = 1;
            // workgroup 0 may not have timed out (it writes every word but this one then): the flag goes out from whoever did
            __hip_atomic_store(&st_out->barrier_timeout, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < ST_WORDS && (threadIdx.x != FS_TMO_WORD || s_st.barrier_timeout))
        reinterpret_cast<uint32_t*>(st_out)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&s_st)[threadIdx.x];
    if (s_st.stop || !mine) return;
    const float r0 = s_st.Rd[0], r1 = s_st.Rd[1], r2 = s_st.Rd[2], r3 = s_st.Rd[3], r4 = s_st.Rd[4], r5 = s_st.Rd[5],
                r6 = s_st.Rd[6], r7 = s_st.Rd[7], r8 = s_st.Rd[8], t0 = s_st.td[0], t1 = s_st.td[1], t2 = s_st.td[2];
    float4 ox, oy, oz;
#define PCR_ROW(o, a, b, c, tt)                      \
    o.x = ((a * px.x + b * py.x) + c * pz.x) + tt;   \
    o.y = ((a * px.y + b * py.y) + c * pz.y) + tt;   \
    o.z = ((a * px.z + b * py.z) + c * pz.z) + tt;   \
    o.w = ((a * px.w + b * py.w) + c * pz.w) + tt;
    PCR_ROW(ox, r0, r1, r2, t0)
    PCR_ROW(oy, r3, r4, r5, t1)
    PCR_ROW(oz, r6, r7, r8, t2)
#undef PCR_ROW
    if (base + 3 >= n) {                             // (the padding invariant of the tail group: transform_state_kernel)
        const float inf = __builtin_inff();
        if (base + 0 >= n) { ox.x = inf; oy.x = 0.f; oz.x = 0.f; }
        if (base + 1 >= n) { ox.y = inf; oy.y = 0.f; oz.y = 0.f; }
        if (base + 2 >= n) { ox.z = inf; oy.z = 0.f; oz.z = 0.f; }
        if (base + 3 >= n) { ox.w = inf; oy.w = 0.f; oz.w = 0.f; }
    }
    reinterpret_cast<float4*>(x)[i] = ox;
    reinterpret_cast<float4*>(y)[i] = oy;
    reinterpret_cast<float4*>(z)[i] = oz;
    if (seed) {
        const float mx[4] = { ox.x, ox.y, ox.z, ox.w }, my[4] = { oy.x, oy.y, oy.z, oy.w }, mz[4] = { oz.x, oz.y, oz.z, oz.w };
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (base + u >= n) continue;
            const uint32_t j = (uint32_t)(sk[u] & 0xFFFFFFFFull);
            unsigned long long key = ~0ull;
            if (j < nt) {
                const float dx = mx[u] - sq[u][0], dy = my[u] - sq[u][1], dz = mz[u] - sq[u][2];
                const uint32_t e2 = __float_as_uint((dx * dx + dy * dy) + dz * dz);       // A1, unfused (nanoflann.hpp:403-406): seed_next_search's arithmetic
                if (e2 < 0x7F7FFFFFu) key = ((unsigned long long)e2 << 32) | j;            // FLT_MAX gate, nanoflann.hpp:163,1360
            }
            keys[base + u] = key;
        }
    }
}

// A thread's four consecutive pairs as icp_sums_update_move_kernel reads them — points, keys, original indices and the gathered target points, everything
// that depends on nothing else requested in one go — for icp_sums_solve_kernel below.  (That kernel keeps its own copy of these lines: routed through
// these functions it took 156 VGPRs instead of 142, and it is the path of every loop the chain below does not serve.)
// PP = the consecutive pairs of a thread: 4 as there, or 2 or 1, which spread the same pairs over more workgroups.
template <int PP>
struct FsPairs {
    float px[PP], py[PP], pz[PP];
    unsigned long long sk[PP];             // (no pair: NaN distance, no target)
    uint32_t og[PP];
    float sq[PP][3];
};

template <int PP>
__device__ __forceinline__ void fs_load_pairs(FsPairs<PP>& P, bool mine, uint32_t i, uint32_t n, const float* x, const float* y, const float* z,
                                              const unsigned long long* keys, const uint32_t* __restrict__ orig, const float* __restrict__ tx,
                                              const float* __restrict__ ty, const float* __restrict__ tz, uint32_t nt)
{
    static_assert(PP == 1 || PP == 2 || PP == 4, "one vector load per array");
    const uint32_t base = PP * i;
#pragma unroll
    for (int u = 0; u < PP; u++) { P.px[u] = 0.f; P.py[u] = 0.f; P.pz[u] = 0.f; P.sk[u] = ~0ull; P.og[u] = base + u; }
    if (mine) {
        // (a cloud's arrays are padded to a multiple of four points: the vector loads of the tail group stay inside them)
        if constexpr (PP == 4) {
            const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(y)[i], c = reinterpret_cast<const float4*>(z)[i];
            P.px[0] = a.x; P.px[1] = a.y; P.px[2] = a.z; P.px[3] = a.w;
            P.py[0] = b.x; P.py[1] = b.y; P.py[2] = b.z; P.py[3] = b.w;
            P.pz[0] = c.x; P.pz[1] = c.y; P.pz[2] = c.z; P.pz[3] = c.w;
        } else if constexpr (PP == 2) {
            const float2 a = reinterpret_cast<const float2*>(x)[i], b = reinterpret_cast<const float2*>(y)[i], c = reinterpret_cast<const float2*>(z)[i];
            P.px[0] = a.x; P.px[1] = a.y; P.py[0] = b.x; P.py[1] = b.y; P.pz[0] = c.x; P.pz[1] = c.y;
        } else {
            P.px[0] = x[i]; P.py[0] = y[i]; P.pz[0] = z[i];
        }
        if (base + (PP - 1) < n) {
            if constexpr (PP == 4) {
                const ulonglong2 k01 = reinterpret_cast<const ulonglong2*>(keys)[2 * i], k23 = reinterpret_cast<const ulonglong2*>(keys)[2 * i + 1];
                P.sk[0] = k01.x; P.sk[1] = k01.y; P.sk[2] = k23.x; P.sk[3] = k23.y;
                if (orig) { const uint4 o = reinterpret_cast<const uint4*>(orig)[i]; P.og[0] = o.x; P.og[1] = o.y; P.og[2] = o.z; P.og[3] = o.w; }
            } else if constexpr (PP == 2) {
                const ulonglong2 k01 = reinterpret_cast<const ulonglong2*>(keys)[i];
                P.sk[0] = k01.x; P.sk[1] = k01.y;
                if (orig) { const uint2 o = reinterpret_cast<const uint2*>(orig)[i]; P.og[0] = o.x; P.og[1] = o.y; }
            } else {
                P.sk[0] = keys[i];
                if (orig) P.og[0] = orig[i];
            }
        } else {
#pragma unroll
            for (int u = 0; u < PP; u++)
                if (base + u < n) { P.sk[u] = keys[base + u]; if (orig) P.og[u] = orig[base + u]; }
        }
    }
    // the target points of the pairs, gathered ONCE: nothing else in this launch needs them
#pragma unroll
    for (int u = 0; u < PP; u++) {
        P.sq[u][0] = 0.f; P.sq[u][1] = 0.f; P.sq[u][2] = 0.f;
        const uint32_t j = (uint32_t)(P.sk[u] & 0xFFFFFFFFull);
        if (j < nt) { P.sq[u][0] = tx[j]; P.sq[u][1] = ty[j]; P.sq[u][2] = tz[j]; }
    }
}

// ... and their limbs, added exactly as the sums pass adds them (kabsch_partial_kernel's gate, term for term), reduced to the workgroup's TOTALS in row[]:
// not normalised (block_reduce_limbs, NORM = false) — they leave the workgroup as integers
template <int PP, int WAVES>
__device__ __forceinline__ void fs_pairs_row(const FsPairs<PP>& P, float max_corr, const KabschPlan& plan, uint32_t nt, double (&red_l)[WAVES][KB_NL],
                                             double (&row)[KB_ROW])
{
    double c0[6], c1[6], p0[9], p1[9], p2[9], cnt = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) { c0[k] = 0.0; c1[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 9; k++) { p0[k] = 0.0; p1[k] = 0.0; p2[k] = 0.0; }
    unsigned long long lastkey = 0;
    int overflow = 0;
#pragma unroll
    for (int u = 0; u < PP; u++) {
        const uint32_t d2b = (uint32_t)(P.sk[u] >> 32);
        const float d2 = __uint_as_float(d2b);
        const uint32_t j = (uint32_t)(P.sk[u] & 0xFFFFFFFFull);
        if (d2 < max_corr && j < nt) {                       // registration.cpp:936 (kabsch_partial_kernel's gate, term for term)
            const float pf0 = P.px[u], pf1 = P.py[u], pf2 = P.pz[u];
            if (!(fabsf(pf0) < plan.lim && fabsf(pf1) < plan.lim && fabsf(pf2) < plan.lim)) { overflow = 1; continue; }
            const double Pd[3] = { pf0, pf1, pf2 }, Q[3] = { P.sq[u][0], P.sq[u][1], P.sq[u][2] };
#pragma unroll
            for (int c = 0; c < 3; c++) { acc2(Pd[c], plan.sc, c0[c], c1[c]); acc2(Q[c], plan.sc, c0[3 + c], c1[3 + c]); }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) acc3(Q[r] * Pd[c], plan.sp, p0[3 * r + c], p1[3 * r + c], p2[3 * r + c]);
            cnt += 1.0;
            const unsigned long long lk = ((unsigned long long)P.og[u] << 32) | d2b;
            lastkey = lk > lastkey ? lk : lastkey;
        }
    }
    double tn[KB_NL];                    // at most 4 terms per thread: no per-thread carries
#pragma unroll
    for (int c = 0; c < 6; c++) { tn[3 * c] = c0[c]; tn[3 * c + 1] = c1[c]; tn[3 * c + 2] = 0.0; }
#pragma unroll
    for (int k = 0; k < 9; k++) { tn[18 + 4 * k] = p0[k]; tn[19 + 4 * k] = p1[k]; tn[20 + 4 * k] = p2[k]; tn[21 + 4 * k] = 0.0; }
    tn[54] = cnt;
    block_reduce_limbs<true, WAVES, false>(tn, lastkey, overflow, red_l, row, false);
}

// live limb p (the numbering of block_reduce_limbs' butterfly: 12 coordinate limbs, 27 product limbs, the count) -> its slot of a row
__host__ __device__ constexpr int live_slot(int p) { return p < 12 ? 3 * (p / 2) + p % 2 : (p < 39 ? 18 + 4 * ((p - 12) / 3) + (p - 12) % 3 : 54); }

// Exhaustive loops whose NEXT SEARCH moves the cloud (nn1_sphere.hpp, MV): the sums and the solve alone.  The front half is that of
// icp_sums_update_move_kernel — same loads, same gate, same limbs, same butterfly and LDS combine — for PP pairs per thread, but nobody waits and nobody
// stores a row: a workgroup's totals are exact integers below 2^53 (T x PP terms below 2^40), so lanes 0 .. 41 of its first wave convert them to int64
// and ADD them, one atomic instruction, into replica blockIdx.x & (R - 1) of ctx->icp_acc_dev: 40 live limbs, the overflow count, and the last-kept key
// by an atomic max.  Then the wave drains (vmcnt(0): the atomics have been performed), its lane 0 releases and takes a TICKET from the monotonic counter (every
// workgroup of every launch arrives, in every phase; the host passes the value the counter has once all of this launch have).  The ONE workgroup whose
// ticket is the last acquires, reads the R replicas in one trip — whatever the geometry —, writes zeros back over them (the invariant: all zero between
// launches; the next launch is stream-ordered behind this one), adds them as integers, propagates the carries, and goes on through row_to_out18 and
// icp_state_step to publish the whole state to st_out; every other workgroup has returned.  No spin, no residency condition on the grid: the move needs
// the new R, t, but the move is the next launch's.  Phases 0 and 1 (stopped loop, stop_after_transform) add nothing and leave the zeros alone: the last
// arriver writes the stopped state.
// in every phase the publishing workgroup also writes the state into a slot of the host ring where the launch ends a chunk or the call
// (ss_snapshot below; snap, seq).  levels = 2 (tune icp_ticket_levels; measured, no gain, not the default) arrives in two steps: at a counter of the
// workgroup's own replica, and only the last of a replica at the shared counter — which then counts the replicas that have workgroups, not the workgroups.
// An accumulator holds at most n terms below 2^40: n < 2^22 (icp_sums_solve_blocks) keeps it below 2^62.
// (ACC_R, ACC_W, ACC_CNT — the replicas and the words of one: icp_finish.hpp)

// DESIGN.md 6j.  The state snapshot the host loop looks at (icp.cpp), written by the publishing workgroup itself where the launch is the last of a chunk or
// of the call (snap: a slot of the pinned, coherent host ring; null otherwise — uniform over the workgroup): the words of the state just published, from
// the threads that published them, then — behind a workgroup barrier, so that the words precede it — one lane's SYSTEM-scope release store of the
// sequence number the host waits for.  (All of it is wave 0's: ST_WORDS <= 64.)
__device__ __forceinline__ void ss_snapshot(IcpSnapSlot* snap, unsigned long long seq, const IcpState* s_st)
{
    if (!snap) return;
    if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(&snap->state)[threadIdx.x] = reinterpret_cast<const uint32_t*>(s_st)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&snap->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int T, int PP>
__global__ __launch_bounds__(T) void icp_sums_solve_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, const uint32_t* __restrict__ orig,
    const unsigned long long* __restrict__ keys, uint32_t nt, float max_corr, KabschPlan plan, long long* acc, unsigned long long* counter,
    unsigned long long target, const IcpState* __restrict__ st_in, IcpState* __restrict__ st_out, double* __restrict__ out, const float* __restrict__ x,
    const float* __restrict__ y, const float* __restrict__ z, uint32_t n, uint32_t np, IcpSnapSlot* snap, unsigned long long seq, int levels
#ifdef PCR_SS_PROF
    , unsigned long long* prof
#endif
    )
{
    constexpr int WAVES = T / 64;
    static_assert((unsigned long long)T * PP * (1ull << num::KB_W) <= (1ull << 53), "a workgroup's limb totals must be exact in f64");
    static_assert(ST_WORDS <= 64 && offsetof(IcpSnapSlot, state) == 0, "one wave stores a snapshot's words and, behind them, its sequence number");
    static_assert(T >= 64 && ACC_R * ACC_W <= 2 * T, "the last arriver reads the replicas in at most two loads per thread");
    __shared__ double red_l[WAVES][KB_NL];
    __shared__ long long s_acc[ACC_R][ACC_W];
    __shared__ double row[KB_ROW];
    __shared__ double o18[19];
    __shared__ IcpState s_st;
    __shared__ int s_last;
#ifdef PCR_SS_PROF
    const unsigned long long pt_a = __builtin_amdgcn_s_memrealtime();
    unsigned long long pt_b = pt_a, pt_c = pt_a;
#endif
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    uint32_t stw = 0;                       // (the state first: it is on the critical path and loads retire in order)
    if (threadIdx.x < ST_WORDS) stw = reinterpret_cast<const uint32_t*>(st_in)[threadIdx.x];
    FsPairs<PP> P;
    fs_load_pairs<PP>(P, i < np, i, n, x, y, z, keys, orig, tx, ty, tz, nt);
    if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(&s_st)[threadIdx.x] = stw;
    __syncthreads();
    const int phase = (s_st.stop || s_st.barrier_timeout) ? 0 : (s_st.stop_after_transform ? 1 : 2);       // uniform over the GRID
    if (phase == 2) fs_pairs_row<PP, WAVES>(P, max_corr, plan, nt, red_l, row);
    // ---- the contribution and the ticket: wave 0 adds the totals, drains, its lane 0 releases and arrives; the last arriver acquires
    if (threadIdx.x < 64) {
        if (phase == 2) {
#ifdef PCR_SS_PROF
            pt_b = __builtin_amdgcn_s_memrealtime();
#endif
            long long* mine = acc + (size_t)(blockIdx.x & (ACC_R - 1)) * ACC_W;
            const int l = threadIdx.x;
            if (l < KB_NLC) __hip_atomic_fetch_add(mine + l, (long long)row[live_slot(l)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (l == KB_NLC) __hip_atomic_fetch_add(mine + l, row[56] != 0.0 ? 1ll : 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (l == KB_NLC + 1)
                __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(mine + l), (unsigned long long)__double_as_longlong(row[55]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (threadIdx.x == 0) {
            if (phase == 2) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (kept behind the fence whatever the compiler thinks of the scoreboard)
            }
            int last;
            if (levels == 2) {
                // a ticket per replica: this workgroup arrives at its replica's counter (word ACC_CNT of the row; zero between launches like the row), and
                // only the last of the replica's icp_replica_members goes on to the final counter, where at most ACC_R arrive.  It passes on what it
                // acquired: one acquire-release fence between its two adds, in every phase (the stopped phases hand nothing on but the order of the
                // counters' own modifications: the final arriver's zeros must come after every add)
                const uint32_t r = blockIdx.x & (ACC_R - 1);
                unsigned long long* mine_cnt = reinterpret_cast<unsigned long long*>(acc + (size_t)r * ACC_W + ACC_CNT);
                if (phase != 2) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                const unsigned long long mine_t = __hip_atomic_fetch_add(mine_cnt, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
#ifdef PCR_SS_PROF
                pt_c = __builtin_amdgcn_s_memrealtime();
#endif
                last = 0;
                if (mine_t == icp_replica_members(gridDim.x, r)) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    last = __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == target;
                }
            } else {
                last = __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == target;
#ifdef PCR_SS_PROF
                pt_c = __builtin_amdgcn_s_memrealtime();
#endif
            }
#ifdef PCR_SS_PROF
            if (prof && phase == 2) { atomicAdd(prof + 12, pt_b - pt_a); atomicAdd(prof + 13, pt_c - pt_b); atomicAdd(prof + 14, 1ull); atomicMax(prof + 15, pt_c - pt_b); }
#endif
            if (last && (phase == 2 || levels == 2)) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the invalidate is over before the barrier below lets the other waves read
            }
            s_last = last;
        }
    }
    __syncthreads();
    if (!s_last) return;
    if (phase == 2) {
#ifdef PCR_SS_PROF
        const unsigned long long pt_c1 = __builtin_amdgcn_s_memrealtime();
#endif
        // the R replicas, one trip (relaxed agent-scope loads: past this CU's L1), and the zeros back over them
        for (int t = threadIdx.x; t < ACC_R * ACC_W; t += T) {
            (&s_acc[0][0])[t] = __hip_atomic_load(acc + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(acc + t, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
#ifdef PCR_SS_PROF
        const unsigned long long pt_c2 = __builtin_amdgcn_s_memrealtime();
#endif
        const int k = threadIdx.x;
        if (k < KB_NLC + 2) acc_fold_column(s_acc, k);      // word k over the replicas, into replica 0's place
        __syncthreads();
        acc_to_row(s_acc, k, row);                         // sum k: its live limbs, then the carries
        __syncthreads();
#ifdef PCR_SS_PROF
        unsigned long long pt_d = __builtin_amdgcn_s_memrealtime(), pt_e = pt_d;
#endif
        row_to_out18(row, plan.e, o18);
        __syncthreads();
        if (threadIdx.x < 19) out[threadIdx.x] = o18[threadIdx.x];
        if (threadIdx.x < 64) {
            icp_state_step_wave((int)threadIdx.x, &s_st, o18, o18[16] >= 0.0, (float)o18[17], o18[18] != 0.0);
#ifdef PCR_SS_PROF
            pt_e = __builtin_amdgcn_s_memrealtime();
#endif
        }
        __syncthreads();
        if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(st_out)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&s_st)[threadIdx.x];
#ifdef PCR_SS_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long pt_f = __builtin_amdgcn_s_memrealtime();
#endif
        ss_snapshot(snap, seq, &s_st);
#ifdef PCR_SS_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (prof && threadIdx.x == 0) {          // (the last arriver alone: plain values, ticket -> replicas reduced -> solved -> published -> snapshot in host memory)
            prof[0] = pt_d - pt_c; prof[1] = pt_e - pt_d; prof[11] = pt_f - pt_e; prof[4] = snap ? __builtin_amdgcn_s_memrealtime() - pt_f : 0ull;
            prof[2] = pt_c1 - pt_c; prof[3] = pt_c2 - pt_c1;     // (ticket -> acquired -> replicas in LDS)
        }
#endif
        return;
    }
    if (threadIdx.x == 0) s_st.stop = 1;       // (phase 0: stays stopped; phase 1: max_iter reached, the loop is over)
    // (a ticket per replica: nothing was added to the rows, but their counters have counted this launch's arrivals — back to zero, behind the acquire above)
    if (levels == 2 && threadIdx.x < ACC_R)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(acc + (size_t)threadIdx.x * ACC_W + ACC_CNT), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(st_out)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&s_st)[threadIdx.x];
    ss_snapshot(snap, seq, &s_st);
}

// Chain 5 (icp.cpp): the sums ALONE.  The front half of icp_sums_solve_kernel, unchanged — same loads, same gate, same limbs, same
// butterfly, the same 42 atomics into replica blockIdx.x & (R - 1) — and nothing behind it: no release, no ticket, no acquire, no last arriver.  The
// reduce and the solve are the NEXT launch's: every workgroup of the moving search (nn1_sphere.hpp, SV) or, behind the last iteration of a call,
// icp_finish_kernel below reads the rows for itself (icp_finish.hpp finish_iteration) — a kernel boundary of the stream stands between these adds and
// those loads.  There are TWO sets of rows: iteration k adds into set k & 1 (acc), and its last workgroup stores zeros over the other set (acc_next):
// that one's last readers were the workgroups of the search in front of this launch, its next writer is the sums launch behind the next search.  Both
// sets are all zero between calls (the finishing launch zeroes the one it read).  st_in is the state the preceding search published (the upload in
// front of the first): a stopped loop, or one behind its last transform, adds nothing — but still zeroes.
template <int T, int PP>
__global__ __launch_bounds__(T) void icp_sums_kernel(
    const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz, const uint32_t* __restrict__ orig,
    const unsigned long long* __restrict__ keys, uint32_t nt, float max_corr, KabschPlan plan, long long* acc, long long* acc_next,
    const IcpState* __restrict__ st_in, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, uint32_t n, uint32_t np
#ifdef PCR_SS_PROF
    , unsigned long long* prof
#endif
    )
{
    constexpr int WAVES = T / 64;
    static_assert((unsigned long long)T * PP * (1ull << num::KB_W) <= (1ull << 53), "a workgroup's limb totals must be exact in f64");
    __shared__ double red_l[WAVES][KB_NL];
    __shared__ double row[KB_ROW];
    __shared__ IcpState s_st;
#ifdef PCR_SS_PROF
    const unsigned long long pt_a = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    uint32_t stw = 0;                       // (the state first: it is on the critical path and loads retire in order)
    if (threadIdx.x < ST_WORDS) stw = reinterpret_cast<const uint32_t*>(st_in)[threadIdx.x];
    FsPairs<PP> P;
    fs_load_pairs<PP>(P, i < np, i, n, x, y, z, keys, orig, tx, ty, tz, nt);
    if (threadIdx.x < ST_WORDS) reinterpret_cast<uint32_t*>(&s_st)[threadIdx.x] = stw;
    if (blockIdx.x == gridDim.x - 1)
        for (int t = threadIdx.x; t < ACC_R * ACC_W; t += T) __hip_atomic_store(acc_next + t, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_st.stop || s_st.barrier_timeout || s_st.stop_after_transform) return;       // uniform over the GRID
    fs_pairs_row<PP, WAVES>(P, max_corr, plan, nt, red_l, row);
    if (threadIdx.x < 64) {
#ifdef PCR_SS_PROF
        const unsigned long long pt_b = __builtin_amdgcn_s_memrealtime();
#endif
        long long* mine = acc + (size_t)(blockIdx.x & (ACC_R - 1)) * ACC_W;
        const int l = threadIdx.x;
        if (l < KB_NLC) __hip_atomic_fetch_add(mine + l, (long long)row[live_slot(l)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (l == KB_NLC) __hip_atomic_fetch_add(mine + l, row[56] != 0.0 ? 1ll : 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (l == KB_NLC + 1)
            __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(mine + l), (unsigned long long)__double_as_longlong(row[55]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#ifdef PCR_SS_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long pt_c = __builtin_amdgcn_s_memrealtime();
        if (prof && threadIdx.x == 0) { atomicAdd(prof + 12, pt_b - pt_a); atomicAdd(prof + 13, pt_c - pt_b); atomicAdd(prof + 14, 1ull); atomicMax(prof + 15, pt_c - pt_b); }
#endif
    }
}

// ... and the finishing launch of a call on that chain, ONE wave behind the last sums launch: the iteration's back half (finish_iteration), published to
// st_out, out and — where the host handed one on — slot [RING] of its ring; then zeros over the set it read.  In the stopped phases it only forwards the
// stopped state (and zeroes all the same: the set is zero already, and stays so whatever happened in front)
__global__ __launch_bounds__(64) void icp_finish_kernel(long long* acc, int e, const IcpState* __restrict__ st_in, IcpState* __restrict__ st_out,
                                                        double* __restrict__ out, IcpSnapSlot* snap, unsigned long long seq)
{
    __shared__ IcpFinishLds F;
    const int l = threadIdx.x;
    IcpFinishLoads Q;
    finish_request(l, st_in, acc, Q);
    const bool stepped = finish_iteration(l, Q, e, F);
    for (int t = l; t < ACC_R * ACC_W; t += 64) __hip_atomic_store(acc + t, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (lane l behind its own loads of these words)
    finish_publish(l, stepped, F, st_out, out, snap, seq);
}

// multi rank, step 1: reduce the block rows into the all-reduce buffer
//   [0..54] normalised limbs, [55] overflow flag, [56 + 2r] ORDER KEY of rank r's last kept pair (0: it kept none), [57 + 2r] that pair's d2
// (every entry is summed exactly by the all-reduce: integers below 2^40 x ranks, one non-zero pair of words per rank).  The order key
// says where the pair stands in the WHOLE source cloud: global index + 1 for a shard that knows its points' indices (gidx:
// pcr_cloud_shard_spatial — any partition), rank + 1 otherwise (contiguous blocks in rank order); the loss of an iteration is that of
// the pair with the largest key (registration.cpp:939: the last pair pushed).
__global__ __launch_bounds__(KF_BLOCK) void icp_reduce_slots_kernel(const double* __restrict__ partials, uint32_t n_blocks,
                                                                    double* __restrict__ out, int nranks, int rank, int have_points,
                                                                    const uint32_t* __restrict__ gidx)
{
    __shared__ double red[KF_GROUPS][64];
    __shared__ double row[KB_ROW];
    if (have_points) {
        reduce_rows(partials, n_blocks, red, row);
    } else {
        if (threadIdx.x < KB_ROW) row[threadIdx.x] = 0.0;
        __syncthreads();
    }
    if (threadIdx.x < KB_NL) out[threadIdx.x] = row[threadIdx.x];
    if (threadIdx.x == KB_NL) out[55] = row[56];
    if ((int)threadIdx.x < 2 * nranks) {
        const int r = threadIdx.x / 2, which = threadIdx.x % 2;
        double v = 0.0;
        if (r == rank && row[54] > 0.0) {
            const unsigned long long lk = (unsigned long long)__double_as_longlong(row[55]);
            v = which == 0 ? (gidx ? (double)gidx[(uint32_t)(lk >> 32)] + 1.0 : (double)(rank + 1)) : (double)__uint_as_float((uint32_t)(lk & 0xFFFFFFFFull));
        }
        out[56 + threadIdx.x] = v;
    }
}

// multi rank, step 2 (after the all-reduce): carries and moments (thread k converts moment k, as row_to_out18 does for one rank);
// the loss comes from the highest rank that kept a pair.  One wave.
__global__ __launch_bounds__(64) void icp_update_from_sums_kernel(double* __restrict__ buf, int nranks, int e, IcpState* st)
{
    __shared__ double row[KB_NL + 1];
    __shared__ double sums[16];
    __shared__ IcpState s_st;
    const int k = threadIdx.x;
    if (k < KB_NL) row[k] = buf[k];
    icp_state_stage(st, &s_st);
    if (s_st.stop) return;
    if (k < 6) { num::limbs_normalize(row + 3 * k, 2); sums[k] = num::limbs_value(row + 3 * k, 2, e - 2 * num::KB_W); }
    else if (k < 15) { num::limbs_normalize(row + 18 + 4 * (k - 6), 3); sums[k] = num::limbs_value(row + 18 + 4 * (k - 6), 3, 2 * e - 3 * num::KB_W); }
    else if (k == 15) sums[15] = row[54];
    __syncthreads();
    const int ls = icp_last_slot(buf, nranks);                 // the pair with the largest order key (every lane alike)
    const bool any = ls >= 0;
    const float d2 = any ? (float)buf[57 + 2 * ls] : 0.0f;
    icp_state_step_wave(k, &s_st, sums, any, d2, buf[55] != 0.0);
    if (k == 0) *st = s_st;
}

__global__ __launch_bounds__(256) void transform_state_kernel(float* __restrict__ x, float* __restrict__ y,
                                                              float* __restrict__ z, uint32_t n, uint32_t n4, IcpState* st, SeedArgs sd)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    // the points, the delta pose and the stop flag are requested together (one memory round trip, not three in a row)
    float4 px = reinterpret_cast<float4*>(x)[i];
    float4 py = reinterpret_cast<float4*>(y)[i];
    float4 pz = reinterpret_cast<float4*>(z)[i];
    const float r0 = st->Rd[0], r1 = st->Rd[1], r2 = st->Rd[2], r3 = st->Rd[3], r4 = st->Rd[4], r5 = st->Rd[5],
                r6 = st->Rd[6], r7 = st->Rd[7], r8 = st->Rd[8], t0 = st->td[0], t1 = st->td[1], t2 = st->td[2];
    const int stop = st->stop;
    if (stop) return;
    float4 ox, oy, oz;
#define PCR_ROW(o, a, b, c, tt)                      \
    o.x = ((a * px.x + b * py.x) + c * pz.x) + tt;   \
    o.y = ((a * px.y + b * py.y) + c * pz.y) + tt;   \
    o.z = ((a * px.z + b * py.z) + c * pz.z) + tt;   \
    o.w = ((a * px.w + b * py.w) + c * pz.w) + tt;
    PCR_ROW(ox, r0, r1, r2, t0)
    PCR_ROW(oy, r3, r4, r5, t1)
    PCR_ROW(oz, r6, r7, r8, t2)
#undef PCR_ROW
    // keep the padding invariant (x = +inf, y = z = 0) of the tail group without a second launch
    const uint32_t base = 4 * i;
    if (base + 3 >= n) {
        const float inf = __builtin_inff();
        if (base + 0 >= n) { ox.x = inf; oy.x = 0.f; oz.x = 0.f; }
        if (base + 1 >= n) { ox.y = inf; oy.y = 0.f; oz.y = 0.f; }
        if (base + 2 >= n) { ox.z = inf; oy.z = 0.f; oz.z = 0.f; }
        if (base + 3 >= n) { ox.w = inf; oy.w = 0.f; oz.w = 0.f; }
    }
    reinterpret_cast<float4*>(x)[i] = ox;
    reinterpret_cast<float4*>(y)[i] = oy;
    reinterpret_cast<float4*>(z)[i] = oz;
    if (sd.tx) {
        seed_next_search(sd, base + 0, n, ox.x, oy.x, oz.x); seed_next_search(sd, base + 1, n, ox.y, oy.y, oz.y);
        seed_next_search(sd, base + 2, n, ox.z, oy.z, oz.z); seed_next_search(sd, base + 3, n, ox.w, oy.w, oz.w);
    }
}

int launch_icp_update(pcr_ctx* ctx, uint32_t n_blocks, IcpState* st_dev, const KabschPlan& plan)
{
    {
        ProfScope p(ctx, "icp_update");
        hipLaunchKernelGGL(icp_update_kernel, dim3(1), dim3(KF_BLOCK), 0, ctx->stream, ctx->partials, n_blocks, plan.e, st_dev, ctx->dev_out);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// seed_tgt != nullptr: the move also seeds the next exhaustive search against that target (seed_next_search) and says so on the context
static SeedArgs seed_args(pcr_ctx* ctx, const pcr_cloud* c, const pcr_cloud* seed_tgt)
{
    SeedArgs sd = { nullptr, nullptr, nullptr, nullptr, 0u };
    ctx->keys_seeded = false;
    if (seed_tgt && ctx->keys && ctx->keys_n == c->n && c->n) {
        sd = SeedArgs{ seed_tgt->x(), seed_tgt->y(), seed_tgt->z(), ctx->keys, (uint32_t)seed_tgt->n };
        ctx->keys_seeded = true; ctx->keys_seed_src = c->id; ctx->keys_seed_tgt = seed_tgt->id;
    }
    return sd;
}

int launch_icp_update_move(pcr_ctx* ctx, uint32_t n_blocks, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan, pcr_cloud* c, const pcr_cloud* seed_tgt)
{
    const uint32_t n4 = (uint32_t)((c->n + 3) / 4);
    const SeedArgs sd = seed_args(ctx, c, seed_tgt);
    {
        ProfScope p(ctx, "icp_update");
        hipLaunchKernelGGL(icp_update_move_kernel, dim3((n4 + KF_BLOCK - 1) / KF_BLOCK), dim3(KF_BLOCK), 0, ctx->stream, ctx->partials, n_blocks, plan.e, st_in,
                           st_out, ctx->dev_out, c->x(), c->y(), c->z(), (uint32_t)c->n, n4, sd);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// threads per workgroup of the fused sums + move launch (4 pairs per thread): 512 = 59 workgroups at 120 k (tune icp_fused_sums_threads: 256)
static int fs_threads(const pcr_ctx* ctx) { return tune_get(ctx, "icp_fused_sums_threads", 512) == 256 ? 256 : 512; }

// the workgroups the fused sums + move launch takes for n points, or 0 where it does not run: tune icp_fused_sums = 2 (off), more workgroups than
// min(CUs, tune icp_fused_sums_max_blocks) — one workgroup per CU BY COUNT is what makes all of them resident, with a wide margin — or fewer than
// icp_fused_sums_min points: the barrier (3.9 us from a workgroup's row store to the end of its wait) costs more than the launch boundary and the second
// pass it replaces while those are short (4 000 points: 25.0 against 22.4 us per iteration; 60 k 49.3 / 50.8, 120 k 61.2 / 63.4, 250 k 98.6 / 107.1:
// profiles/icp_fused_sums.txt)
uint32_t icp_fused_sums_blocks(const pcr_ctx* ctx, size_t n)
{
    if (n == 0 || tune_get(ctx, "icp_fused_sums", 1) != 1 || (int64_t)n < tune_get(ctx, "icp_fused_sums_min", 60000)) return 0;
    const uint64_t T = (uint64_t)fs_threads(ctx), n4 = ((uint64_t)n + 3) / 4, blocks = (n4 + T - 1) / T;
    const int64_t cus = ctx->prop.multiProcessorCount;
    const int64_t cap = std::min<int64_t>(cus, tune_get(ctx, "icp_fused_sums_max_blocks", cus));
    return (int64_t)blocks <= cap ? (uint32_t)blocks : 0u;
}

int launch_icp_sums_update_move(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud* c, float max_corr, const IcpState* st_in, IcpState* st_out,
                                const KabschPlan& plan, const pcr_cloud* seed_tgt)
{
    if (ctx->keys_n != c->n) return fail(ctx, PCR_ERR_STATE, "kabsch: no matching correspondence pass");
    const uint32_t blocks = icp_fused_sums_blocks(ctx, c->n);
    if (!blocks || !ctx->icp_barrier_dev || (seed_tgt && seed_tgt != tgt)) return fail(ctx, PCR_ERR_STATE, "launch_icp_sums_update_move");
    const uint32_t n4 = (uint32_t)((c->n + 3) / 4);
    const SeedArgs sd = seed_args(ctx, c, seed_tgt);
    const unsigned long long target = ctx->icp_barrier_arrived + blocks;      // the counter's value once every workgroup of this launch has arrived
    {
        ProfScope p(ctx, "icp_update");
#ifdef PCR_FS_PROF
#define PCR_FS_EXTRA , ctx->grid_stats_dev
#else
#define PCR_FS_EXTRA
#endif
#define PCR_FS(T)                                                                                                                                   \
        hipLaunchKernelGGL((icp_sums_update_move_kernel<T>), dim3(blocks), dim3(T), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(), c->orig, ctx->keys, \
                           (uint32_t)tgt->n, max_corr, plan, ctx->partials, ctx->icp_barrier_dev, target, st_in, st_out, ctx->dev_out, c->x(), c->y(),  \
                           c->z(), (uint32_t)c->n, n4, sd.tx ? 1 : 0 PCR_FS_EXTRA)
        if (fs_threads(ctx) == 256) PCR_FS(256); else PCR_FS(512);
#undef PCR_FS
#undef PCR_FS_EXTRA
    }
    PCR_HIP(ctx, hipGetLastError());
    ctx->icp_barrier_arrived = target;        // (counted only once the launch is on the stream)
    return PCR_OK;
}

// geometry of the sums + solve launch: threads per workgroup (tune icp_sums_solve_threads: 256 / 512) and consecutive pairs per thread (tune
// icp_sums_solve_pairs: 1 / 2 / 4); any other value is the default (profiles/icp_sums_accumulators.txt)
constexpr int SS_THREADS_DEFAULT = 512, SS_PAIRS_DEFAULT = 2;
// ... and of the sums launch of the chain sums -> search, behind the same tunes: nobody queues at a ticket there, so more and smaller workgroups pay
// (profiles/icp_solve_in_search.txt section 5: 256 x 2 = 235 workgroups at 120 k)
constexpr int SA_THREADS_DEFAULT = 256, SA_PAIRS_DEFAULT = 2;
static int ss_threads(const pcr_ctx* ctx, int dflt = SS_THREADS_DEFAULT)
{
    const int64_t t = tune_get(ctx, "icp_sums_solve_threads", dflt);
    return t == 256 ? 256 : t == 512 ? 512 : dflt;
}
static int ss_pairs(const pcr_ctx* ctx, int dflt = SS_PAIRS_DEFAULT)
{
    const int64_t p = tune_get(ctx, "icp_sums_solve_pairs", dflt);
    return p == 1 ? 1 : p == 2 ? 2 : p == 4 ? 4 : dflt;
}

// the workgroups the sums + solve launch takes for n points, or 0 where it does not run: the switch and the lower bound of the fused sums + move launch
// (icp_fused_sums = 2, icp_fused_sums_min), but no cap at one workgroup per CU — nobody waits for anybody.  From 2^22 points on it never runs, whatever
// the tunes say: an int64 accumulator takes n terms below 2^40
uint32_t icp_sums_solve_blocks(const pcr_ctx* ctx, size_t n)
{
    if (n == 0 || n >= ((size_t)1 << 22) || tune_get(ctx, "icp_fused_sums", 1) != 1 || (int64_t)n < tune_get(ctx, "icp_fused_sums_min", 60000)) return 0;
    const uint64_t T = (uint64_t)ss_threads(ctx), PP = (uint64_t)ss_pairs(ctx), np = ((uint64_t)n + PP - 1) / PP;
    return (uint32_t)((np + T - 1) / T);
}

// arrival counters of the sums + solve launch (tune icp_ticket_levels: 1 = the one counter, 2 = one per replica and the shared one behind them; any other
// value is the default; DESIGN.md 6j, profiles/icp_host_snapshots.txt)
constexpr int SS_LEVELS_DEFAULT = 1;      // (measured: the ticket per replica gains nothing at 118 or 235 workgroups)
static int ss_levels(const pcr_ctx* ctx)
{
    const int64_t l = tune_get(ctx, "icp_ticket_levels", SS_LEVELS_DEFAULT);
    return l == 1 ? 1 : l == 2 ? 2 : SS_LEVELS_DEFAULT;
}

int launch_icp_sums_solve(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* c, float max_corr, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan,
                          IcpSnapSlot* snap, unsigned long long seq)
{
    if (ctx->keys_n != c->n) return fail(ctx, PCR_ERR_STATE, "kabsch: no matching correspondence pass");
    const uint32_t blocks = icp_sums_solve_blocks(ctx, c->n);
    if (!blocks || !ctx->icp_barrier_dev || !ctx->icp_acc_dev) return fail(ctx, PCR_ERR_STATE, "launch_icp_sums_solve");
    if (ctx->icp_acc_dirty) {
        // a call that ended in an error may have left sums behind: clear them once, in front of this call's first launch (a clean call adds nothing here);
        // both sets — this launch uses set 0 alone, the chain sums -> search (launch_icp_sums) both
        PCR_HIP(ctx, hipMemsetAsync(ctx->icp_acc_dev, 0, (size_t)ICP_ACC_SETS * ICP_ACC_REPLICAS * ICP_ACC_WORDS * sizeof(long long), ctx->stream));
        ctx->icp_acc_dirty = false;
    }
    const int T = ss_threads(ctx), PP = ss_pairs(ctx), levels = ss_levels(ctx);
    const uint32_t np = (uint32_t)((c->n + PP - 1) / PP);
    // the shared counter's value once every workgroup of this launch has arrived — with a ticket per replica, once the last of every replica that has
    // workgroups has (the counter is also the grid barrier's of the fused sums + move launch: it only ever grows, by whatever a launch adds)
    const uint32_t arrivals = levels == 2 ? (blocks < (uint32_t)ICP_ACC_REPLICAS ? blocks : (uint32_t)ICP_ACC_REPLICAS) : blocks;
    const unsigned long long target = ctx->icp_barrier_arrived + arrivals;
    {
        ProfScope p(ctx, "icp_update");
#ifdef PCR_SS_PROF
#define PCR_SS_EXTRA , ctx->grid_stats_dev
#else
#define PCR_SS_EXTRA
#endif
#define PCR_SS(T, PP)                                                                                                                             \
        hipLaunchKernelGGL((icp_sums_solve_kernel<T, PP>), dim3(blocks), dim3(T), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(), c->orig, ctx->keys,  \
                           (uint32_t)tgt->n, max_corr, plan, ctx->icp_acc_dev, ctx->icp_barrier_dev, target, st_in, st_out, ctx->dev_out, c->x(),    \
                           c->y(), c->z(), (uint32_t)c->n, np, snap, seq, levels PCR_SS_EXTRA)
        if (T == 256) { if (PP == 1) PCR_SS(256, 1); else if (PP == 2) PCR_SS(256, 2); else PCR_SS(256, 4); }
        else { if (PP == 1) PCR_SS(512, 1); else if (PP == 2) PCR_SS(512, 2); else PCR_SS(512, 4); }
#undef PCR_SS
#undef PCR_SS_EXTRA
    }
    PCR_HIP(ctx, hipGetLastError());
    ctx->icp_barrier_arrived = target;        // (counted only once the launch is on the stream)
    return PCR_OK;
}

// chain 5: the sums of one iteration into accumulator set `set`, zeros over the other one (icp_sums_kernel); the geometry and its tunes are those of
// the sums + solve launch
int launch_icp_sums(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* c, float max_corr, const IcpState* st_in, const KabschPlan& plan, int set)
{
    if (ctx->keys_n != c->n) return fail(ctx, PCR_ERR_STATE, "kabsch: no matching correspondence pass");
    if (!icp_sums_solve_blocks(ctx, c->n) || !ctx->icp_acc_dev || (set != 0 && set != 1)) return fail(ctx, PCR_ERR_STATE, "launch_icp_sums");
    if (ctx->icp_acc_dirty) {
        // a call that ended in an error may have left sums behind: clear both sets once, in front of this call's first launch
        PCR_HIP(ctx, hipMemsetAsync(ctx->icp_acc_dev, 0, (size_t)ICP_ACC_SETS * ICP_ACC_REPLICAS * ICP_ACC_WORDS * sizeof(long long), ctx->stream));
        ctx->icp_acc_dirty = false;
    }
    const int T = ss_threads(ctx, SA_THREADS_DEFAULT), PP = ss_pairs(ctx, SA_PAIRS_DEFAULT);
    const uint32_t np = (uint32_t)((c->n + PP - 1) / PP), blocks = (np + (uint32_t)T - 1) / (uint32_t)T;
    long long* const acc = ctx->icp_acc_dev + (size_t)set * ICP_ACC_REPLICAS * ICP_ACC_WORDS;
    long long* const acc_next = ctx->icp_acc_dev + (size_t)(set ^ 1) * ICP_ACC_REPLICAS * ICP_ACC_WORDS;
    {
        ProfScope p(ctx, "icp_update");
#ifdef PCR_SS_PROF
#define PCR_SS_EXTRA , ctx->grid_stats_dev
#else
#define PCR_SS_EXTRA
#endif
#define PCR_SA(T, PP)                                                                                                                        \
        hipLaunchKernelGGL((icp_sums_kernel<T, PP>), dim3(blocks), dim3(T), 0, ctx->stream, tgt->x(), tgt->y(), tgt->z(), c->orig, ctx->keys, \
                           (uint32_t)tgt->n, max_corr, plan, acc, acc_next, st_in, c->x(), c->y(), c->z(), (uint32_t)c->n, np PCR_SS_EXTRA)
        if (T == 256) { if (PP == 1) PCR_SA(256, 1); else if (PP == 2) PCR_SA(256, 2); else PCR_SA(256, 4); }
        else { if (PP == 1) PCR_SA(512, 1); else if (PP == 2) PCR_SA(512, 2); else PCR_SA(512, 4); }
#undef PCR_SA
#undef PCR_SS_EXTRA
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// chain 5: the finishing launch of a call, behind its last sums launch (icp_finish_kernel): set = the set that launch added into
int launch_icp_finish(pcr_ctx* ctx, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan, int set, IcpSnapSlot* snap, unsigned long long seq)
{
    if (!ctx->icp_acc_dev || (set != 0 && set != 1)) return fail(ctx, PCR_ERR_STATE, "launch_icp_finish");
    {
        ProfScope p(ctx, "icp_finish");
        hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->icp_acc_dev + (size_t)set * ICP_ACC_REPLICAS * ICP_ACC_WORDS, plan.e,
                           st_in, st_out, ctx->dev_out, snap, seq);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

int launch_icp_reduce_slots(pcr_ctx* ctx, uint32_t n_blocks, int nranks, int rank, bool have_points, const uint32_t* gidx)
{
    hipLaunchKernelGGL(icp_reduce_slots_kernel, dim3(1), dim3(KF_BLOCK), 0, ctx->stream, ctx->partials, n_blocks, ctx->dev_out, nranks, rank,
                       have_points ? 1 : 0, gidx);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// The lane form of the Kabsch solve on its own (kabsch_wave.hpp), for tests: one wave per problem, KSB_WAVES problems per workgroup.  A problem whose
// solve returns -1 (no pair kept) leaves its R and t as they were (the launcher zeroes them)
constexpr int KSB_WAVES = 4;
__global__ __launch_bounds__(64 * KSB_WAVES) void kabsch_solve_batch_kernel(const double* __restrict__ sums, uint32_t n, float* __restrict__ R, float* __restrict__ t,
                                                                            int* __restrict__ rc)
{
    const int l = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * KSB_WAVES + (threadIdx.x >> 6);
    if (p >= n) return;                        // (a whole wave leaves, or none of it)
    const num::WaveLanes g{ l };
    float Rl = 0.0f, tl = 0.0f;
    const int r = num::kabsch_solve_lanes(g, sums + 16 * (size_t)p, Rl, tl);
    if (l == 0) rc[p] = r == 0 ? PCR_OK : PCR_ERR_EMPTY;
    if (r != 0) return;
    if (l < 9) R[9 * (size_t)p + l] = Rl;
    if (l < 3) t[3 * (size_t)p + l] = tl;
}

int kabsch_solve_batch_device(pcr_ctx* ctx, const double* sums, size_t n, float* R, float* t, int* rc)
{
    if (n == 0) return PCR_OK;
    if (n > 0x7FFFFFFFull / 16) return fail(ctx, PCR_ERR_ARG, "pcr_kabsch_solve_batch_device: too many problems");
    const size_t b_sums = n * 16 * sizeof(double), b_R = n * 9 * sizeof(float), b_t = n * 3 * sizeof(float), b_rc = n * sizeof(int);
    char* dev = nullptr;
    PCR_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&dev), b_sums + b_R + b_t + b_rc));
    double* d_sums = reinterpret_cast<double*>(dev);
    float* d_R = reinterpret_cast<float*>(dev + b_sums);
    float* d_t = reinterpret_cast<float*>(dev + b_sums + b_R);
    int* d_rc = reinterpret_cast<int*>(dev + b_sums + b_R + b_t);
    hipError_t e = hipMemcpyAsync(d_sums, sums, b_sums, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_R, 0, b_R + b_t + b_rc, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kabsch_solve_batch_kernel, dim3((uint32_t)((n + KSB_WAVES - 1) / KSB_WAVES)), dim3(64 * KSB_WAVES), 0, ctx->stream, d_sums, (uint32_t)n,
                           d_R, d_t, d_rc);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(R, d_R, b_R, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t, d_t, b_t, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rc, d_rc, b_rc, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_kabsch_solve_batch_device", e);
    return PCR_OK;
}

int launch_icp_update_from_sums(pcr_ctx* ctx, int nranks, IcpState* st_dev, const KabschPlan& plan)
{
    hipLaunchKernelGGL(icp_update_from_sums_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->dev_out, nranks, plan.e, st_dev);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

int launch_transform_state(pcr_ctx* ctx, pcr_cloud* c, IcpState* st_dev, const pcr_cloud* seed_tgt)
{
    if (c->n) {
        const uint32_t n4 = (uint32_t)((c->n + 3) / 4);
        const SeedArgs sd = seed_args(ctx, c, seed_tgt);
        ProfScope p(ctx, "transform");
        hipLaunchKernelGGL(transform_state_kernel, dim3((n4 + 255) / 256), dim3(256), 0, ctx->stream, c->x(), c->y(), c->z(),
                           (uint32_t)c->n, n4, st_dev, sd);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// ---------------------------------------------------------------------------------------------- A8
struct Rt {
    float r[9];
    float t[3];
};

__global__ __launch_bounds__(256) void transform_kernel(float* __restrict__ x, float* __restrict__ y,
                                                        float* __restrict__ z, uint32_t n4, Rt m)
{
    // n4 = number of float4 groups covering [0, n) (the tail group lies inside the cloud's padding and is
    // re-padded by the caller's invariant: padding x stays +inf because inf*R + t is never read as a target
    // beyond n; see launch_transform)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 px = reinterpret_cast<float4*>(x)[i];
    float4 py = reinterpret_cast<float4*>(y)[i];
    float4 pz = reinterpret_cast<float4*>(z)[i];
    float4 ox, oy, oz;
#define PCR_ROW(o, r0, r1, r2, tt)                                   \
    o.x = ((m.r[r0] * px.x + m.r[r1] * py.x) + m.r[r2] * pz.x) + m.t[tt]; \
    o.y = ((m.r[r0] * px.y + m.r[r1] * py.y) + m.r[r2] * pz.y) + m.t[tt]; \
    o.z = ((m.r[r0] * px.z + m.r[r1] * py.z) + m.r[r2] * pz.z) + m.t[tt]; \
    o.w = ((m.r[r0] * px.w + m.r[r1] * py.w) + m.r[r2] * pz.w) + m.t[tt];
    PCR_ROW(ox, 0, 1, 2, 0)
    PCR_ROW(oy, 3, 4, 5, 1)
    PCR_ROW(oz, 6, 7, 8, 2)
#undef PCR_ROW
    reinterpret_cast<float4*>(x)[i] = ox;
    reinterpret_cast<float4*>(y)[i] = oy;
    reinterpret_cast<float4*>(z)[i] = oz;
}

// restore the padding invariant (x = +inf, y = z = 0) of the partially transformed tail group
__global__ void repad_kernel(float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, uint32_t n,
                             uint32_t n_end)
{
    const uint32_t i = n + threadIdx.x;
    if (i < n_end) { x[i] = __builtin_inff(); y[i] = 0.0f; z[i] = 0.0f; }
}

// out of place, the destination's padding written too: group i < n4 = the transformed points (the tail group's lanes beyond n get the padding),
// groups behind it = padding
__global__ __launch_bounds__(256) void transform_into_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                                                             float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, uint32_t n, uint32_t n4,
                                                             uint32_t cap4, Rt m)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap4) return;
    const float inf = __builtin_inff();
    float4 ox = make_float4(inf, inf, inf, inf), oy = make_float4(0.f, 0.f, 0.f, 0.f), oz = oy;
    if (i < n4) {
        const float4 px = reinterpret_cast<const float4*>(sx)[i], py = reinterpret_cast<const float4*>(sy)[i], pz = reinterpret_cast<const float4*>(sz)[i];
#define PCR_ROW(o, r0, r1, r2, tt)                                   \
    o.x = ((m.r[r0] * px.x + m.r[r1] * py.x) + m.r[r2] * pz.x) + m.t[tt]; \
    o.y = ((m.r[r0] * px.y + m.r[r1] * py.y) + m.r[r2] * pz.y) + m.t[tt]; \
    o.z = ((m.r[r0] * px.z + m.r[r1] * py.z) + m.r[r2] * pz.z) + m.t[tt]; \
    o.w = ((m.r[r0] * px.w + m.r[r1] * py.w) + m.r[r2] * pz.w) + m.t[tt];
        PCR_ROW(ox, 0, 1, 2, 0)
        PCR_ROW(oy, 3, 4, 5, 1)
        PCR_ROW(oz, 6, 7, 8, 2)
#undef PCR_ROW
        const uint32_t base = 4 * i;
        if (base + 3 >= n) {
            if (base + 0 >= n) { ox.x = inf; oy.x = 0.f; oz.x = 0.f; }
            if (base + 1 >= n) { ox.y = inf; oy.y = 0.f; oz.y = 0.f; }
            if (base + 2 >= n) { ox.z = inf; oy.z = 0.f; oz.z = 0.f; }
            if (base + 3 >= n) { ox.w = inf; oy.w = 0.f; oz.w = 0.f; }
        }
    }
    reinterpret_cast<float4*>(x)[i] = ox;
    reinterpret_cast<float4*>(y)[i] = oy;
    reinterpret_cast<float4*>(z)[i] = oz;
}

int launch_transform_into(pcr_ctx* ctx, const pcr_cloud* src, pcr_cloud* dst, const float R[9], const float t[3])
{
    if (dst->cap != src->cap || dst->n != src->n || dst->cap % 4) return fail(ctx, PCR_ERR_ARG, "launch_transform_into");
    Rt m;
    memcpy(m.r, R, sizeof m.r);
    memcpy(m.t, t, sizeof m.t);
    const uint32_t n4 = (uint32_t)((src->n + 3) / 4), cap4 = (uint32_t)(src->cap / 4);
    {
        ProfScope p(ctx, "transform");
        hipLaunchKernelGGL(transform_into_kernel, dim3((cap4 + 255) / 256), dim3(256), 0, ctx->stream, src->x(), src->y(), src->z(), dst->x(), dst->y(), dst->z(),
                           (uint32_t)src->n, n4, cap4, m);
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

int launch_transform(pcr_ctx* ctx, pcr_cloud* c, const float R[9], const float t[3])
{
    if (c->n == 0) return PCR_OK;
    Rt m;
    memcpy(m.r, R, sizeof m.r);
    memcpy(m.t, t, sizeof m.t);
    const uint32_t n4 = (uint32_t)((c->n + 3) / 4);
    {
        ProfScope p(ctx, "transform");
        hipLaunchKernelGGL(transform_kernel, dim3((n4 + 255) / 256), dim3(256), 0, ctx->stream, c->x(), c->y(),
                           c->z(), n4, m);
    }
    PCR_HIP(ctx, hipGetLastError());
    if (c->n % 4) {
        hipLaunchKernelGGL(repad_kernel, dim3(1), dim3(4), 0, ctx->stream, c->x(), c->y(), c->z(), (uint32_t)c->n,
                           (uint32_t)(n4 * 4));
        PCR_HIP(ctx, hipGetLastError());
    }
    return PCR_OK;
}

}  // namespace pcr
