// nn1_sphere.hpp — part of nn1_brute.hip (included there, inside namespace pcr, behind nn1_strack_kernel).
//
// STRACK3: the exhaustive search with the sign filter applied to a HIERARCHY OF BOUNDING SPHERES (round 4).  STRACK spends one matrix instruction and
// eight half-rate v_or3_b32 per 32 queries x 32 RECORDS, for every record of the target — and at the settled pose of an ICP loop all but a handful of
// them lie metres beyond the query's threshold.  The sign test is bilinear, so it works on sets of records as well: a set inside the sphere (c, rho)
// cannot matter to a query unless |r - c| <= sqrt(thr) + rho, which is again "a sum of K-slot products is negative" (grid_common.hpp, LEVEL 1: the
// statement and what makes it a theorem).  Three levels of MFMA rows (BtIndex, built by bt_ensure_l1):
//   level 0: one row per level-1 TILE of 512 records, in the scale of a level-0 super-tile of 131 072 records — EVERY row of the slice gets its sign for
//            every query (still exhaustive: nothing is skipped without a computed sign that says it cannot matter);
//   level 1: one row per CHUNK of 16 records of the level-1 tiles level 0 flagged, level-1 super-tiles of 4 096 records share a centre and a scale;
//   level 2: the tiles of 32 records that hold a flagged chunk through STRACK's per-record rows, with operands in the scale of their LEVEL-1 super-tile
//            (BtIndex::l1_rec_ops: no operand setup of its own); the flagged (query, chunk) pairs of THAT are evaluated with the exact A1 arithmetic,
//            four lanes per chunk — the canonical (d2 bits, index) minimum decides, thresholds fall after every level-1 super-tile.
// History: the two-level form without level 0 (STRACK2, every chunk row for every query) ran 0.085 ms per 120 k x 120 k search against
// STRACK's 0.44 and was removed when this kernel (0.034 ms) took its place.
// Same keys bit for bit as every other kernel of this file (parity sweeps: nn1_variant 10; device check of the sphere statement:
// pcr_selftest_sphere_f16, part of the once-per-context verdict).  Matches: registration.cpp:925-941.
#pragma once

constexpr int S2_TILES = 512;                 // level-2 tiles a wave may collect per level-1 super-tile (of its 128: the list is flushed when full)
constexpr int S2_CAP = 128;                   // flagged (query, chunk) pairs a wave lists before it evaluates them

// the listed chunks against their queries: four lanes per chunk, four records each, sixteen chunks per round
// (Measured and dropped: the second round skipped wave-uniformly when e0 + 16 >= cnt — a wave lists ~37 chunks per search over several flushes, so
// that round is mostly empty lanes: 0.0307-0.0321 ms per 120 k search with both rounds, 0.0308-0.0318 with the skip: no difference to measure.)
template <int QG, class LDS>
__device__ __forceinline__ void s2_flush(LDS& L, uint32_t cnt, const float4* __restrict__ records, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (uint32_t e0 = 0; e0 < cnt; e0 += 32) {               // two rounds of sixteen chunks per trip to memory
        uint32_t slot[2];
        bool valid[2];
        float4 q[2], rec[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t e = e0 + 16u * r + (lane >> 2);
            valid[r] = e < cnt;
            const uint32_t ent = L.list[valid[r] ? e : 0];
            slot[r] = ent & 127u;
            q[r] = L.q[slot[r]];
            const float4* rp = records + (size_t)(ent >> 7) * 16 + (lane & 3u);
#pragma unroll
            for (int j = 0; j < 4; j++) rec[r][j] = rp[4 * j];             // (padding records: x = +inf, never accepted)
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            unsigned long long key = ~0ull;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t d = d2_exact_bits(q[r].x, q[r].y, q[r].z, rec[r][j].x, rec[r][j].y, rec[r][j].z);
                const unsigned long long k = ((unsigned long long)d << 32) | __float_as_uint(rec[r][j].w);
                if (d < 0x7F7FFFFFu && k < key) key = k;                   // FLT_MAX gate
            }
            if (!valid[r]) key = ~0ull;
            key = key_min_dpp<0xB1>(key); key = key_min_dpp<0x4E>(key);    // quad xor 1, xor 2: the four lanes of the chunk
            if ((lane & 3u) == 0u && key != ~0ull) atomicMin(&L.best[slot[r]], key);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__device__ __forceinline__ uint32_t s2_or16(const f32x16 acc)
{
    uint32_t a = __float_as_uint(acc[0]) | __float_as_uint(acc[1]) | __float_as_uint(acc[2]);
#pragma unroll
    for (int j = 3; j + 1 < 16; j += 2) a = a | __float_as_uint(acc[j]) | __float_as_uint(acc[j + 1]);
    return a | __float_as_uint(acc[15]);
}

#ifdef PCR_S2_PROF
#define PCR_S2_TICK(acc) { pt_b = __builtin_amdgcn_s_memrealtime(); acc += pt_b - pt_a; pt_a = pt_b; }
#else
#define PCR_S2_TICK(acc)
#endif
#ifndef PCR_S2_WAVES
#define PCR_S2_WAVES 4
#endif
#ifndef PCR_SV_SOLVER_SHIFT
#define PCR_SV_SOLVER_SHIFT 0                 // SV: wave (blockIdx.x >> shift) & 3 of a workgroup finishes the iteration (A/B builds; a matter of speed only)
#endif
// ---- the kernel.  (Measured on the two-level predecessor, sorted queries, 120 000 x 120 000, profile build: 86 % of a wave's life went into level 1 —
// every chunk row of the target for every group of queries, 300 SIMD cycles per level-1 tile — and 10 % into level 2 and the exact evaluation.  With
// level 0 a wave looks at 8 level-0 tiles, then only at the level-1 tiles whose sphere some query's ball reaches: a few of 240.)
constexpr int S3_L1LIST = 256;                // level-1 tiles of one level-0 super-tile

// LISTS: the rows form and the instances with several query groups keep their flagged level-1 tiles and level-2 tiles as lists in LDS, written by lane 0,
// fenced, and read back per run / per batch (ds_read_b32 + v_readfirstlane per entry).  The default instance — ONE group, transposed — gets every flag
// set as a wave-uniform ballot, i.e. in scalar registers, and walks it there (S3 SCALAR WALK below): no list, no fence, no read-back, and a group mask
// that is always 1 is not carried.  Its four waves hold 9 216 B per workgroup instead of 21 504.  Per wave of 32 queries at the settled 120 k pose
// (PMC): 1 500 -> 1 263 vector, 1 163 -> 994 scalar, 109 -> 21 LDS instructions, the 32 MFMAs unchanged; a settled search 26.8 -> 21.5 us
// (profiles/strack3_scalar_walk.txt).
template <int QG, bool LISTS>
struct S3WaveLds {
    float4 q[QG * 32];
    unsigned long long best[QG * 32];
    uint32_t l1list[S3_L1LIST];               // level-1 tile | groups that flagged it << 28
    uint32_t tiles[S2_TILES];                 // level-2 tile | groups << 28
    uint32_t list[S2_CAP + 256 * QG];         // (chunk << 7) | query slot: what a batch of four level-2 tiles can add fits behind S2_CAP entries
};
template <int QG>
struct S3WaveLds<QG, false> {
    float4 q[QG * 32];
    unsigned long long best[QG * 32];
    uint32_t list[S2_CAP + 256 * QG];
};

// ---- S3 SCALAR WALK: the index arithmetic of the default instance's walk over its flag masks, shared by the kernel and by the host enumeration
// (pcr_s3_walk_visits, tests/test_strack3_scalar_walk.py).  Level 0 leaves eight 32-bit row masks per level-0 super-tile S0: bit j of word t is
// level-1 tile T1 = (S0 * 8 + t) * 32 + j.  Two words make one 64-bit scalar; level-1 super-tile S0 * 32 + 8 i + B (eight level-1 tiles, one RUN) is
// byte B of scalar i.  Level 1 leaves one 16-bit mask per level-1 tile of the run: 128 bits, bit 16 u + k = level-2 tile (S1 * 8 + u) * 16 + k.
// Rows / tiles [first, first + 32 or 64) that lie below n (the index is padded to whole super-tiles; rows behind the records are never visited):
__host__ __device__ __forceinline__ uint32_t s3w_valid32(uint32_t first, uint32_t n)
{
    return n <= first ? 0u : n - first >= 32u ? ~0u : (1u << (n - first)) - 1u;
}
__host__ __device__ __forceinline__ unsigned long long s3w_valid64(uint32_t first, uint32_t n)
{
    return n <= first ? 0ull : n - first >= 64u ? ~0ull : (1ull << (n - first)) - 1ull;
}
// the lowest non-empty byte of cur: its position B and its eight bits (the flagged level-1 tiles of the run); the byte is cleared
__host__ __device__ __forceinline__ uint32_t s3w_take_run(unsigned long long& cur, uint32_t& rm)
{
    const uint32_t B = (uint32_t)__builtin_ctzll(cur) >> 3;
    rm = (uint32_t)(cur >> (8u * B)) & 0xFFu;
    cur &= ~(0xFFull << (8u * B));
    return B;
}
// the lowest set bit of the 128 (lo, hi; at least one is set): its position, cleared.  hi moves down once lo is used up — base counts the 64 it stood for
__host__ __device__ __forceinline__ uint32_t s3w_next(unsigned long long& lo, unsigned long long& hi, uint32_t& base)
{
    if (!lo) { lo = hi; hi = 0ull; base += 64u; }
    const uint32_t b = (uint32_t)__builtin_ctzll(lo);
    lo &= lo - 1ull;
    return base + b;
}

// TR: how levels 0 and 1 read "which sphere rows did any of the 32 queries flag" (tune nn1_s3_transposed: 1 = true and default, 2 = false).
//   true:  the product runs TRANSPOSED — the queries' operand as A, the stored sphere tile as B (both operands of v_mfma_f32_32x32x16_f16 have the
//          same register layout: lane l carries row / column l % 32, K-slots 8 (l / 32) .. + 7; the same pairs of f16 values meet, so the signs
//          are the same).  Lane (n, h) then holds sphere row n of the tile against the 16 queries 8 (i >> 2) + 4 h + (i & 3): one s2_or16 and ONE
//          ballot give a 64-bit mask whose halves are the two halves of the queries — the row mask is lo | hi.
//   false: spheres as A, queries as B, one ballot per accumulator (16 per level-0 tile behind a repeated MFMA, 8 per level-1 tile): each is a
//          chain of v_cmp / s_cmp / s_cselect / 64-bit v_cmp of the mask / s_and / s_cselect / s_or / s_or, 8 instructions alternating between
//          the vector and the scalar unit — 4 095 static instructions in <1> (1 940 scalar, 1 582 vector, 28 MFMA) against 2 423 (832, 1 069, 20);
//          0.033-0.035 against 0.027-0.029 ms per settled 120 k search (profiles/strack3_transposed.txt).  Kept as nn1_strack3_rows_kernel for
//          A/B runs in one process.
// Both read the same index: bt_l0_ops_kernel / bt_l1_ops_kernel store the rows in the order the B role wants (see l1_chunk_operand).
//
// MV: the search of an ICP loop that MOVES its own queries first (icp.cpp, the chain search -> sums + solve).  mv is the state the solve of
// the previous iteration published (kabsch.hip icp_sums_solve_kernel): its stop flags are this launch's stop flags, its Rd, td the pending move.  A lane
// loads its point and the previous winner's key as always, gathers that winner's target point, moves the point with transform_state_kernel's arithmetic
// term for term — ((a x + b y) + c z) + t, unfused — and evaluates the seed of THIS search with seed_next_search's expression and gate (kabsch.hip): the
// same point, the same seed and the same threshold the move launch would have left in memory.  The owner of a query stores the moved point before the
// scan; the seed key goes into the wave's best[] instead of keys[], so the one store of keys[i] at the end is min(seed, what the scan found) — what
// merge_key makes of the two — and no lane reads back from memory what another wrote in this launch.  In place, hence only for launches in which ONE
// workgroup reads a query (one slice; the host checks: s3_move_route).  A stopped loop's launch moves nothing and writes nothing.
struct S3Move {
    const IcpState* st;                                       // stop flags + Rd, td
    const float* tx; const float* ty; const float* tz;        // the target in its own order (keys[] index it)
    uint32_t nt;
};
template <bool MV> struct S3Src { typedef const float* __restrict__ ptr; };
template <> struct S3Src<true> { typedef float* ptr; };        // (read and written in place)

// SV (with MV; chain 5 of the loop): the search that FINISHES the previous iteration before it moves.  mv.st is then that iteration's INPUT
// state, and the sums of the iteration lie complete in sv.acc since an earlier launch (kabsch.hip icp_sums_kernel).  Every lane requests what the MV
// prologue requests — its point and key, then the previous winner's target point: none of it depends on the solve — and then ONE wave of the workgroup
// runs icp_finish.hpp's finish_iteration into LDS; behind a workgroup barrier every lane takes Rd, td and the stop flags from there and goes on as MV
// does, with the same move and seed expressions.  Every workgroup computes the same state from the same inputs; workgroup 0 alone writes it out (state
// slot, sums, the host's ring slot).  The surplus waves of the last workgroup stay for the barrier.  The solving wave is blockIdx.x & 3 — a matter of speed only:
// the four workgroups of a CU should not all solve on one SIMD.  Measured (profiles/icp_solve_in_search.txt section 5): (blockIdx.x >> 8) & 3, which
// supposes that workgroups b, b + 256, ... share a CU, is the SLOWEST of the four rules tried, 2 us per iteration behind this one; always wave 0 and
// (blockIdx.x >> 3) & 3 lie 0.3 - 1 us behind it.
template <int QG, bool TR, bool MV, bool SV = false>
__device__ __forceinline__ void nn1_strack3_body(
    const float4* __restrict__ l0_centres, const uint4* __restrict__ l0_ops, const float4* __restrict__ l1_centres, const uint4* __restrict__ l1_ops,
    const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_l0, uint32_t l0_per_slice,
    typename S3Src<MV>::ptr sx, typename S3Src<MV>::ptr sy, typename S3Src<MV>::ptr sz, uint32_t ns,
    unsigned long long* __restrict__ keys, const int* __restrict__ stop, unsigned long long* __restrict__ stats, uint32_t flush_at, uint32_t flush_end, const S3Move mv,
    const IcpSolveArgs sv = IcpSolveArgs{})
{
    static_assert(QG == 4 || QG == 2 || QG == 1, "query groups per wave: pairs (a lane owns query n of the groups 2 p + h) or ONE (both half-lanes own query n)");
    static_assert(MV || !SV, "the search that finishes an iteration is a moving search");
    constexpr int NP = QG == 1 ? 1 : QG / 2;
    int stopv = SV ? 0 : MV ? (mv.st->stop | mv.st->stop_after_transform) : stop ? (stop[0] | stop[1]) : 0;
    float mr[9] = {}, mt[3] = {};                             // (MV: the pending move, requested with the stop flags)
    if (MV && !SV) {
#pragma unroll
        for (int k = 0; k < 9; k++) mr[k] = mv.st->Rd[k];
#pragma unroll
        for (int k = 0; k < 3; k++) mt[k] = mv.st->td[k];
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = lane & 31;
    const bool h = lane >= 32;
    const uint32_t qb = blockIdx.x, sl = blockIdx.y;
    constexpr bool SW = QG == 1 && TR;                        // the scalar walk: flag masks stay in SGPRs, no lists
    __shared__ S3WaveLds<QG, !SW> lds_all[NN_BLOCK / 64];
    S3WaveLds<QG, !SW>& L = lds_all[wave];
    const uint32_t qbase = (qb * (NN_BLOCK / 64) + wave) * (32 * QG);
    if (!SV && qbase >= ns) return;                           // (a surplus wave: no workgroup barrier below — SV: it leaves behind its barrier)
    float qx[NP], qy[NP], qz[NP], thr[NP];
    bool ok[NP];
    bool okg[QG];
    auto slot_of = [&](int p) { return QG == 1 ? n : (uint32_t)(2 * p + (h ? 1 : 0)) * 32 + n; };
    unsigned long long k0[NP];
    float ux[NP], uy[NP], uz[NP];
    // the prologue's loads of pair p: the point and the candidate (or what other slices published) ...
    auto load_query = [&](int p) {
        const uint32_t i = min(qbase + slot_of(p), ns - 1);
        qx[p] = sx[i]; qy[p] = sy[i]; qz[p] = sz[i];
        k0[p] = __atomic_load_n(&keys[i], __ATOMIC_RELAXED);
    };
    // ... MV: the previous winner's target point ...
    auto gather_target = [&](int p) {
        const uint32_t j = (uint32_t)(k0[p] & 0xFFFFFFFFull);
        ux[p] = 0.0f; uy[p] = 0.0f; uz[p] = 0.0f;
        if (j < mv.nt) { ux[p] = mv.tx[j]; uy[p] = mv.ty[j]; uz[p] = mv.tz[j]; }
    };
    // ... MV: the move, the seed of THIS search and the owner's store of the moved point
    auto move_and_seed = [&](int p) {
        const uint32_t slot = slot_of(p), i = min(qbase + slot, ns - 1);
        const uint32_t j = (uint32_t)(k0[p] & 0xFFFFFFFFull);
        const float x = qx[p], y = qy[p], z = qz[p];
        qx[p] = ((mr[0] * x + mr[1] * y) + mr[2] * z) + mt[0];                               // transform_state_kernel's PCR_ROW, term for term
        qy[p] = ((mr[3] * x + mr[4] * y) + mr[5] * z) + mt[1];
        qz[p] = ((mr[6] * x + mr[7] * y) + mr[8] * z) + mt[2];
        k0[p] = ~0ull;
        if (j < mv.nt) {
            const float dx = qx[p] - ux[p], dy = qy[p] - uy[p], dz = qz[p] - uz[p];
            const uint32_t e = __float_as_uint((dx * dx + dy * dy) + dz * dz);               // A1, unfused: seed_next_search's arithmetic
            if (e < 0x7F7FFFFFu) k0[p] = ((unsigned long long)e << 32) | j;                   // FLT_MAX gate
        }
        if constexpr (MV) if ((QG > 1 || !h) && qbase + slot < ns) { sx[i] = qx[p]; sy[i] = qy[p]; sz[i] = qz[p]; }      // (the slot's one owner; lanes past ns read point ns - 1 and store nothing)
    };
    auto stage_query = [&](int p) {
        const uint32_t slot = slot_of(p);
        const uint32_t cb = (uint32_t)(k0[p] >> 32);
        ok[p] = fabsf(qx[p]) < 1e18f && fabsf(qy[p]) < 1e18f && fabsf(qz[p]) < 1e18f && cb < 0x7F7FFFFFu;
        thr[p] = ok[p] ? __uint_as_float(cb) : -INFINITY;
        L.q[slot] = make_float4(qx[p], qy[p], qz[p], 0.0f);
        L.best[slot] = MV ? k0[p] : ~0ull;
        if (!ok[p]) { qx[p] = 0.0f; qy[p] = 0.0f; qz[p] = 0.0f; }                                // (finite operands; thr = -inf: no flag, ever)
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok[p]);
        okg[QG == 1 ? 0 : 2 * p] = (uint32_t)okm == 0xFFFFFFFFu;
        if (QG > 1) okg[QG == 1 ? 0 : 2 * p + 1] = (uint32_t)(okm >> 32) == 0xFFFFFFFFu;
    };
#ifdef PCR_SV_PROF
    // profile build (stats != nullptr: tune grid_stats = 1): the solving wave of workgroup 1 stamps its prologue, 10 ns ticks into words 11 .. 15 of the
    // diagnostics — entry -> loads requested -> replicas in LDS -> solved -> barrier passed -> prologue done (the first level-0 set-up follows)
    unsigned long long pv_entry = __builtin_amdgcn_s_memrealtime(), pv_loads = 0, pv_replicas = 0, pv_solved = 0, pv_barrier = 0;
    bool pv_mine = false;
#endif
    if constexpr (SV) {
        __shared__ IcpFinishLds F;
        const uint32_t solver = (blockIdx.x >> PCR_SV_SOLVER_SHIFT) & (NN_BLOCK / 64 - 1);
        IcpFinishLoads Q = {};
        if (wave == solver) finish_request((int)lane, mv.st, sv.acc, Q);      // (first: loads retire in order, and the solve is the longer chain)
#pragma unroll
        for (int p = 0; p < NP; p++) load_query(p);
#pragma unroll
        for (int p = 0; p < NP; p++) gather_target(p);
#ifdef PCR_SV_PROF
        pv_mine = stats && wave == solver && blockIdx.x == min(1u, gridDim.x - 1u) && lane == 0;
        pv_loads = __builtin_amdgcn_s_memrealtime();
#endif
        bool stepped = false;
        if (wave == solver) stepped = finish_iteration((int)lane, Q, sv.e, F);
#ifdef PCR_SV_PROF
        pv_solved = __builtin_amdgcn_s_memrealtime();
#endif
        __syncthreads();
#ifdef PCR_SV_PROF
        pv_barrier = __builtin_amdgcn_s_memrealtime();
        pv_replicas = F.pt_replicas;
#endif
        if (wave == solver && blockIdx.x == 0 && blockIdx.y == 0) finish_publish((int)lane, stepped, F, sv.st_out, sv.out, sv.snap, sv.seq);
        stopv = F.st.stop | F.st.stop_after_transform;
        if (qbase >= ns) return;                              // (a surplus wave)
#pragma unroll
        for (int k = 0; k < 9; k++) mr[k] = F.st.Rd[k];
#pragma unroll
        for (int k = 0; k < 3; k++) mt[k] = F.st.td[k];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (!stopv) move_and_seed(p);
            stage_query(p);
        }
    }
    else {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            load_query(p);
            if constexpr (MV) if (!stopv) { gather_target(p); move_and_seed(p); }
            stage_query(p);
        }
    }
    if (stopv) return;
#ifdef PCR_SV_PROF
    if (SV && pv_mine) {
        const unsigned long long pv_done = __builtin_amdgcn_s_memrealtime();
        stats[11] = pv_loads - pv_entry; stats[12] = pv_replicas - pv_loads; stats[13] = pv_solved - pv_replicas; stats[14] = pv_barrier - pv_solved; stats[15] = pv_done - pv_barrier;
    }
#endif
#ifdef PCR_S2_PROF
    unsigned long long* const stats_p = stats;
    stats = nullptr;
    unsigned long long pt_pro = 0, pt_l0 = 0, pt_l1 = 0, pt_l2 = 0, pt_epi = 0, pt_a = __builtin_amdgcn_s_memrealtime(), pt_b = 0;
    const unsigned long long pt_begin = pt_a;
#endif
    unsigned long long st_l0 = 0, st_l1 = 0, st_l1flag = 0, st_l2flag = 0, st_l2 = 0, st_eval = 0, st_flushes = 0;       // diagnostics (stats != nullptr)
    unsigned long long clk0 = 0, rt0 = 0;
    if (stats) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    const uint32_t sb = sl * l0_per_slice, se = min(sb + l0_per_slice, n_l0);
    f32x16 zero;
#pragma unroll
    for (int j = 0; j < 16; j++) zero[j] = 0.0f;
    uint32_t cnt = 0;                                         // entries in the wave's list of flagged (query, chunk) pairs (wave-uniform)
    auto refresh = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const uint32_t fb = (uint32_t)(L.best[slot_of(p)] >> 32);       // (~0 >> 32 is a NaN pattern: fminf keeps thr)
            thr[p] = ok[p] ? fminf(thr[p], __uint_as_float(fb)) : thr[p];
        }
    };
    // the queries' operands (A where the product runs transposed, B otherwise): bq0 = sphere rows in a level-0 super-tile's scale; bq1 / bq2 = sphere rows / record rows in a level-1 super-tile's scale
    // (lane (n, h) builds the whole operand of query n of group 2 p + h, the halves change places by v_permlane32_swap: nn1_strack_kernel)
    uint4 bq0[QG], bq1[QG], bq2[QG];
    auto setup0 = [&](const float4 C) {
        const float sc2 = C.w * C.w;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            uint32_t P[4], Q[4];
            st_setup_l1(qx[p], qy[p], qz[p], C, thr[p], sc2, P, Q);
            if (QG == 1) { bq0[0] = h ? make_uint4(Q[0], Q[1], Q[2], Q[3]) : make_uint4(P[0], P[1], P[2], P[3]); continue; }     // (both half-lanes built query n's operand)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const auto r = __builtin_amdgcn_permlane32_swap(P[j], Q[j], false, false);
                P[j] = r[0]; Q[j] = r[1];
            }
            bq0[(2 * p) % QG] = make_uint4(P[0], P[1], P[2], P[3]);
            bq0[(2 * p + 1) % QG] = make_uint4(Q[0], Q[1], Q[2], Q[3]);
        }
    };
    auto setup1 = [&](const float4 C) {
        const float sc2 = C.w * C.w;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            uint32_t P[4], Q[4], Q2[4], P2[4];
            st_setup_l1(qx[p], qy[p], qz[p], C, thr[p], sc2, P, Q, Q2);
            if (QG == 1) {
                bq1[0] = h ? make_uint4(Q[0], Q[1], Q[2], Q[3]) : make_uint4(P[0], P[1], P[2], P[3]);
                bq2[0] = h ? make_uint4(Q2[0], Q2[1], Q2[2], Q2[3]) : make_uint4(P[0], P[1], P[2], P[3]);
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                P2[j] = P[j];
                const auto r = __builtin_amdgcn_permlane32_swap(P[j], Q[j], false, false);
                P[j] = r[0]; Q[j] = r[1];
                const auto r2 = __builtin_amdgcn_permlane32_swap(P2[j], Q2[j], false, false);
                P2[j] = r2[0]; Q2[j] = r2[1];
            }
            bq1[(2 * p) % QG] = make_uint4(P[0], P[1], P[2], P[3]);
            bq1[(2 * p + 1) % QG] = make_uint4(Q[0], Q[1], Q[2], Q[3]);
            bq2[(2 * p) % QG] = make_uint4(P2[0], P2[1], P2[2], P2[3]);
            bq2[(2 * p + 1) % QG] = make_uint4(Q2[0], Q2[1], Q2[2], Q2[3]);
        }
    };
    // LEVEL 2 over the collected tiles of 32 records: the per-record filter for the groups that flagged the tile, four tiles per trip to memory;
    // flagged (query, chunk) pairs are listed and evaluated exactly between batches (from flush_at entries) and at the end (from flush_end);
    // thresholds fall after an evaluation
    auto l2_tile = [&](const uint4 A, uint32_t T, uint32_t gm) {      // one level-2 tile for the groups gm (wave-uniform): its flagged (query, chunk) pairs go on the list
        const uint32_t chunk = 2u * T + (h ? 1u : 0u);
#pragma unroll
        for (int g = 0; g < QG; g++) {
            if (!((gm >> g) & 1u)) continue;                  // (wave-uniform)
            const uint32_t og = s2_or16(__builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, bq2[g]), zero, 0, 0, 0));
            if (stats) st_l2++;
            const unsigned long long m = __builtin_amdgcn_ballot_w64((int)og < 0);
            if (!m) continue;
            if ((int)og < 0) L.list[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (chunk << 7) | (uint32_t)(g * 32) | n;
            cnt += (uint32_t)__popcll(m);
        }
    };
    auto flush_from = [&](uint32_t at) {                      // evaluate the listed pairs once there are at least `at` of them; thresholds fall behind an evaluation
        if (cnt >= at) { s2_flush<QG>(L, cnt, records, lane); st_flushes++; st_eval += cnt; cnt = 0; refresh(); }
    };
    auto level2 = [&](auto& LL, uint32_t n_tiles) {           // (the list form; LL = L, a parameter so that the instance without lists never names them)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // (lane 0 wrote the list)
        for (uint32_t k0 = 0; k0 < n_tiles; k0 += 4) {
            uint32_t Eb[4];
            uint4 Ab[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                Eb[u] = (uint32_t)__builtin_amdgcn_readfirstlane((int)LL.tiles[min(k0 + u, n_tiles - 1)]);
                Ab[u] = ops[(size_t)(Eb[u] & 0x0FFFFFFFu) * 64 + lane];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (k0 + u >= n_tiles) break;                 // (wave-uniform)
                l2_tile(Ab[u], Eb[u] & 0x0FFFFFFFu, Eb[u] >> 28);
            }
            flush_from(flush_at);                             // (flush_at <= S2_CAP: host)
        }
        flush_from(flush_end);
    };
    const uint32_t n_l1_tiles = (n_rec + 511u) / 512u;        // level-1 tiles that hold records (rows behind them: W = +inf, never flagged)
    for (uint32_t S0 = sb; S0 < se; S0++) {
        // LEVEL 0: the eight level-0 tiles of the super-tile, every group — the level-1 tiles some query's ball reaches go on the list
        setup0(l0_centres[S0]);
        PCR_S2_TICK(pt_pro)
        uint32_t n1 = 0;
        uint32_t w0[8];                                       // (SW) the flagged rows of the eight level-0 tiles: 256 bits, one per level-1 tile
        uint4 A0s[8];                                         // the eight level-0 tiles at once: one round trip to memory instead of eight
#pragma unroll
        for (int t = 0; t < 8; t++) A0s[t] = l0_ops[((size_t)S0 * 8 + t) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const uint32_t T0 = S0 * 8 + t;
            const uint4 A0 = A0s[t];
            uint32_t rmask[QG];                               // bit j: row j of this level-0 tile (level-1 tile T0 * 32 + j) flagged by the group
            if (TR) {
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    const uint32_t og = s2_or16(__builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bq0[g]), __builtin_bit_cast(f16x8, A0), zero, 0, 0, 0));
                    const unsigned long long m = __builtin_amdgcn_ballot_w64((int)og < 0);       // lane (j, h): row j against the queries of half h
                    rmask[g] = (uint32_t)m | (uint32_t)(m >> 32);
                }
                if (stats) st_l0 += QG;
            }
            else {
                uint32_t anyg[QG];
#pragma unroll
                for (int g = 0; g < QG; g++)
                    anyg[g] = s2_or16(__builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A0), __builtin_bit_cast(f16x8, bq0[g]), zero, 0, 0, 0));
                if (stats) st_l0 += QG;
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    rmask[g] = 0u;
                    if (!__builtin_amdgcn_ballot_w64((int)anyg[g] < 0)) continue;
                    const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A0), __builtin_bit_cast(f16x8, bq0[g]), zero, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 16; i++) {            // (accumulator i of lane-half h <-> MFMA row 8 (i >> 2) + 4 h + (i & 3) = row j of the tile)
                        const unsigned long long m = __builtin_amdgcn_ballot_w64((int)__float_as_uint(acc[i]) < 0);
                        rmask[g] |= ((uint32_t)m != 0u ? 1u : 0u) << (8 * (i >> 2) + (i & 3));
                        rmask[g] |= ((uint32_t)(m >> 32) != 0u ? 1u : 0u) << (8 * (i >> 2) + 4 + (i & 3));
                    }
                }
            }
            if constexpr (SW) {                               // the word IS the list: rows behind the records masked once, not bit by bit
                w0[t] = rmask[0] & s3w_valid32(T0 * 32u, n_l1_tiles);
                n1 += (uint32_t)__popc(w0[t]);
            }
            else {
                uint32_t un = rmask[0];
#pragma unroll
                for (int g = 1; g < QG; g++) un |= rmask[g];
                while (un) {                                  // wave-uniform; ascending level-1 tiles
                    const uint32_t j = (uint32_t)__builtin_ctz(un);
                    un &= un - 1u;
                    uint32_t gm = 0u;
#pragma unroll
                    for (int g = 0; g < QG; g++) gm |= ((rmask[g] >> j) & 1u) << g;
                    const uint32_t T1 = T0 * 32u + j;
                    if (T1 < n_l1_tiles) { if (lane == 0) L.l1list[n1] = T1 | (gm << 28); n1++; }      // (n1 <= 256 = the rows of a level-0 super-tile)
                }
            }
        }
        if (stats) st_l1flag += n1;
        PCR_S2_TICK(pt_l0)
        if (!n1) continue;
        // (Measured and dropped: the level-0 tiles of a super-tile dealt to 2 / 4 waves per group of queries — twice / four times the waves, each with a
        // share of the level-0 rows and what hangs under them: 0.036 / 0.034 ms, the same.)
        // (Measured and dropped: the k-th eighth of the sorted query blocks on XCD k, so that an XCD's L2 holds one region of the target's rows instead
        // of all of them — PMC: 31 MB fetched per launch for a 4 MB working set, every XCD its own copy: 0.036-0.037 ms against 0.034; the regions
        // differ in work, and the launch is not bound by those fetches.)
        // (Measured and dropped: the whole of a SHORT list — up to eight level-1 tiles in up to four super-tiles, the settled pose's case — in one go:
        // all operands in one trip, four operand sets side by side, all level-2 tiles, one evaluation.  Three links in the wave's chain of trips to
        // memory instead of three per super-tile, and the same 0.034-0.035 ms: PMC counts 1 950 vector + 1 800 scalar instructions per wave of 32
        // queries, four waves per SIMD — the launch is bound by their issue, not by the chain.)
        // LEVEL 1 over the listed level-1 tiles, for the groups that reached them: chunk rows.  The list is ascending, so the (at most eight) tiles
        // of one level-1 super-tile follow each other: their operands come in ONE trip to memory, the super-tile's scale serves level 1 and
        // level 2, and the level-2 tiles with a flagged chunk are filtered and evaluated before the next super-tile's operands are built
        if constexpr (SW) {
            // the 256 row bits as four 64-bit scalars, walked from the lowest: a RUN — the flagged level-1 tiles of one level-1 super-tile — is one
            // non-empty byte, its operands the contiguous 8 KB at l1_ops + S1 * 8 * 64: one address, the eight tiles at immediate offsets of
            // -4 KB ... +3 KB around the middle of the block (global loads of gfx950 carry a signed 13-bit offset)
            unsigned long long m0 = w0[0] | ((unsigned long long)w0[1] << 32), m1 = w0[2] | ((unsigned long long)w0[3] << 32),
                               m2 = w0[4] | ((unsigned long long)w0[5] << 32), m3 = w0[6] | ((unsigned long long)w0[7] << 32);
            const uint32_t n_l2 = (n_rec + 31u) / 32u;        // level-2 tiles that hold records (tiles of the index's padding hold nothing)
#pragma nounroll
            for (uint32_t s1b = S0 * 32u; m0 | m1 | m2 | m3; s1b += 8u) {
                unsigned long long cur = m0;
                m0 = m1; m1 = m2; m2 = m3; m3 = 0ull;
                while (cur) {                                 // wave-uniform; ascending level-1 super-tiles
                    uint32_t rm;
                    const uint32_t S1 = s1b + s3w_take_run(cur, rm);
                    const uint4* const mid = l1_ops + ((size_t)S1 * 8 + 4) * 64 + lane;
                    uint4 Ar[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) Ar[u] = mid[(u - 4) * 64];
                    // (Measured and dropped: the loads of the run's unflagged tiles skipped by wave-uniform branches — eight branches in front of the
                    // one trip to memory: 53.7-54.2 us per step of the headline against 52.8-54.3 with all eight loads, medians 53.9 / 53.0,
                    // four processes each, alternating: profiles/strack3_scalar_walk.txt.)
                    setup1(l1_centres[S1]);
                    unsigned long long tl = 0ull, th = 0ull;  // the flagged level-2 tiles of the run: 8 x 16 bits
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        if (!((rm >> u) & 1u)) continue;      // (wave-uniform)
                        const uint32_t og = s2_or16(__builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bq1[0]), __builtin_bit_cast(f16x8, Ar[u]), zero, 0, 0, 0));
                        if (stats) st_l1++;
                        const unsigned long long m = __builtin_amdgcn_ballot_w64((int)og < 0);      // (stored row n of the tile = chunk 2 (n & 15) + (n >> 4): level-2 tile k is rows k and k + 16)
                        const uint32_t cm = (uint32_t)m | (uint32_t)(m >> 32);
                        const uint32_t tm = (cm | (cm >> 16)) & 0xFFFFu;
                        if (stats) st_l2flag += (unsigned long long)__popc(tm);
                        if (u < 4) tl |= (unsigned long long)tm << (16 * (u & 3)); else th |= (unsigned long long)tm << (16 * (u & 3));
                    }
                    const uint32_t t2b = S1 * 128u;           // the run's first level-2 tile
                    tl &= s3w_valid64(t2b, n_l2); th &= s3w_valid64(t2b + 64u, n_l2);
                    PCR_S2_TICK(pt_l1)
                    // LEVEL 2: the 128 bits in ascending order, four tiles per trip to memory (operands: ops + (t2b + bit) * 64)
                    const uint4* const rb = ops + (size_t)t2b * 64 + lane;
                    uint32_t left = (uint32_t)__popcll(tl) + (uint32_t)__popcll(th), tb = 0u;
                    while (left) {
                        const uint32_t nb = min(left, 4u);
                        uint32_t id[4];
                        uint4 Ab[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if (u && (uint32_t)u >= nb) break;               // (wave-uniform: a short batch loads what it has)
                            id[u] = s3w_next(tl, th, tb);
                            Ab[u] = rb[id[u] * 64u];
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if ((uint32_t)u >= nb) break;     // (wave-uniform)
                            l2_tile(Ab[u], t2b + id[u], 1u);
                        }
                        left -= nb;
                        flush_from(flush_at);                 // (flush_at <= S2_CAP: host)
                    }
                    flush_from(flush_end);
                    PCR_S2_TICK(pt_l2)
                }
            }
        }
        else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // (lane 0 wrote the list)
            for (uint32_t k = 0; k < n1;) {
                uint32_t Er[8];
                uint4 Ar[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    Er[u] = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.l1list[min(k + u, n1 - 1)]);
                    Ar[u] = l1_ops[(size_t)(Er[u] & 0x0FFFFFFFu) * 64 + lane];
                }
                const uint32_t S1 = (Er[0] & 0x0FFFFFFFu) >> 3;
                setup1(l1_centres[S1]);
                uint32_t n_tiles = 0, run = 0;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (k + u >= n1 || ((Er[u] & 0x0FFFFFFFu) >> 3) != S1) break;       // (wave-uniform: the end of the list or of this super-tile's run)
                    run++;
                    const uint32_t T1 = Er[u] & 0x0FFFFFFFu, gm1 = Er[u] >> 28;
                    uint32_t tmask[QG];                           // bit k: level-2 tile k of this level-1 tile (chunks 2 k, 2 k + 1) flagged by the group
                    uint32_t un = 0u;
#pragma unroll
                    for (int g = 0; g < QG; g++) {
                        tmask[g] = 0u;
                        if (!((gm1 >> g) & 1u)) continue;         // (wave-uniform)
                        if (TR) {                                 // (stored row n of the tile = chunk 2 (n & 15) + (n >> 4): level-2 tile k is rows k and k + 16)
                            const uint32_t og = s2_or16(__builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bq1[g]), __builtin_bit_cast(f16x8, Ar[u]), zero, 0, 0, 0));
                            if (stats) st_l1++;
                            const unsigned long long m = __builtin_amdgcn_ballot_w64((int)og < 0);
                            const uint32_t cm = (uint32_t)m | (uint32_t)(m >> 32);
                            tmask[g] = (cm | (cm >> 16)) & 0xFFFFu;
                        }
                        else {
                            const f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, Ar[u]), __builtin_bit_cast(f16x8, bq1[g]), zero, 0, 0, 0);
                            if (stats) st_l1++;
                            if (!__builtin_amdgcn_ballot_w64((int)s2_or16(acc) < 0)) continue;
#pragma unroll
                            for (int i = 0; i < 8; i++) {         // (accumulators i and i + 8 of lane-half h: rows k and k + 16, k = 8 (i >> 2) + 4 h + (i & 3))
                                const unsigned long long m = __builtin_amdgcn_ballot_w64((int)(__float_as_uint(acc[i]) | __float_as_uint(acc[i + 8])) < 0);
                                tmask[g] |= ((uint32_t)m != 0u ? 1u : 0u) << (8 * (i >> 2) + (i & 3));
                                tmask[g] |= ((uint32_t)(m >> 32) != 0u ? 1u : 0u) << (8 * (i >> 2) + 4 + (i & 3));
                            }
                        }
                        un |= tmask[g];
                    }
                    if (stats) st_l2flag += (unsigned long long)__popc(un);
                    while (un) {                                  // wave-uniform (at most 8 x 16 = 128 tiles per super-tile: the list of 512 holds them)
                        const uint32_t k2 = (uint32_t)__builtin_ctz(un);
                        un &= un - 1u;
                        uint32_t gm = 0u;
#pragma unroll
                        for (int g = 0; g < QG; g++) gm |= ((tmask[g] >> k2) & 1u) << g;
                        const uint32_t T2 = T1 * 16u + k2;
                        if ((size_t)T2 * 32 < n_rec) { if (lane == 0) L.tiles[n_tiles] = T2 | (gm << 28); n_tiles++; }      // (tiles of the index's padding hold nothing)
                    }
                }
                k += run;
                PCR_S2_TICK(pt_l1)
                if (n_tiles) level2(L, n_tiles);
                PCR_S2_TICK(pt_l2)
            }
        }
        flush_from(1u);
        PCR_S2_TICK(pt_l2)
    }
#pragma unroll
    for (int g = 0; g < QG; g++) {
        unsigned long long kbest = L.best[g * 32 + n];
        if (!okg[g] && sb < se) {
            // a query without finite coordinates or without a candidate: the wave scans the slice exactly for this group, each half-lane one half
            // of it (rare: NaN / inf queries, a seed kernel that found nothing acceptable)
            const float4 q = L.q[g * 32 + n];
            const uint32_t r0 = (uint32_t)min((unsigned long long)sb * BT_L0_SUPER, (unsigned long long)n_rec),
                           r1 = (uint32_t)min((unsigned long long)se * BT_L0_SUPER, (unsigned long long)n_rec), mid = r0 + (r1 - r0) / 2;
            for (uint32_t j = h ? mid : r0; j < (h ? r1 : mid); j++) {
                const float4 rec = records[j];
                const uint32_t e = d2_exact_bits(q.x, q.y, q.z, rec.x, rec.y, rec.z);
                const unsigned long long key = ((unsigned long long)e << 32) | __float_as_uint(rec.w);
                if (e < 0x7F7FFFFFu && key < kbest) kbest = key;
            }
            const unsigned long long ko = key_xor32(kbest);
            kbest = ko < kbest ? ko : kbest;
            if (kbest == ~0ull) kbest = 0x7F800000FFFFFFFFull;           // "no neighbour" is the key (+inf, no index), as every other kernel writes it
        }
        const uint32_t i = qbase + g * 32 + n;
        if (MV) { if (!h && i < ns) keys[i] = kbest; }                   // (best[] started from the seed: this IS the merged key, ~0 = no claim included)
        else if (!h && i < ns && kbest != ~0ull) merge_key(&keys[i], kbest);
    }
#ifdef PCR_S2_PROF
    PCR_S2_TICK(pt_epi)
    if (stats_p && lane == 0 && ((blockIdx.x * 7u + blockIdx.y * 3u + wave) & 15u) == 0u) {     // one wave in 16 reports: [0] prologue + level-0 setup [1] level 0 [2] level 1 [3] level 2 + evaluation
        const unsigned long long life = pt_a - pt_begin;                                          // [4] epilogue ticks (10 ns), [5] waves, [6] sum of lives, [7] longest, [8..15] lives by 5 us bins
        atomicAdd(&stats_p[0], pt_pro); atomicAdd(&stats_p[1], pt_l0); atomicAdd(&stats_p[2], pt_l1); atomicAdd(&stats_p[3], pt_l2); atomicAdd(&stats_p[4], pt_epi);
        atomicAdd(&stats_p[5], 1ull); atomicAdd(&stats_p[6], life); atomicMax(&stats_p[7], life);
        atomicAdd(&stats_p[8 + min((int)(life / 500), 7)], 1ull);
    }
#endif
    if (stats && threadIdx.x == 0) {                                      // shader clock under this kernel's load: cycles / 100 MHz ticks (bench.py)
        atomicAdd(&stats[4], (unsigned long long)__builtin_amdgcn_s_memtime() - clk0);
        atomicAdd(&stats[5], (unsigned long long)__builtin_amdgcn_s_memrealtime() - rt0);
    }
    if (stats && lane == 0) {
        if (st_flushes) atomicAdd(&stats[2], st_flushes);                 // joint evaluations (wave level)
        if (st_l1flag) atomicAdd(&stats[3], st_l1flag);                   // level-1 tiles flagged by level 0 (per wave: union of its groups)
        if (st_eval) atomicAdd(&stats[6], st_eval);                       // (query, chunk) pairs evaluated exactly
        if (st_l0) atomicAdd(&stats[7], st_l0);                           // level-0 MFMAs
        if (st_l1) atomicAdd(&stats[8], st_l1);                           // level-1 MFMAs
        if (st_l2flag) atomicAdd(&stats[9], st_l2flag);                   // level-2 tiles flagged by level 1
        if (st_l2) atomicAdd(&stats[10], st_l2);                          // level-2 MFMAs
    }
}

#define PCR_S3_PARAMS                                                                                                                                   \
    const float4* __restrict__ l0_centres, const uint4* __restrict__ l0_ops, const float4* __restrict__ l1_centres, const uint4* __restrict__ l1_ops,   \
    const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_l0, uint32_t l0_per_slice,                            \
    const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, uint32_t ns,                                              \
    unsigned long long* __restrict__ keys, const int* __restrict__ stop, unsigned long long* __restrict__ stats, uint32_t flush_at, uint32_t flush_end
#define PCR_S3_ARGS l0_centres, l0_ops, l1_centres, l1_ops, ops, records, n_rec, n_l0, l0_per_slice, sx, sy, sz, ns, keys, stop, stats, flush_at, flush_end
template <int QG>
__global__ __launch_bounds__(NN_BLOCK, PCR_S2_WAVES) void nn1_strack3_kernel(PCR_S3_PARAMS) { nn1_strack3_body<QG, true, false>(PCR_S3_ARGS, S3Move{}); }
template <int QG>
__global__ __launch_bounds__(NN_BLOCK, PCR_S2_WAVES) void nn1_strack3_rows_kernel(PCR_S3_PARAMS) { nn1_strack3_body<QG, false, false>(PCR_S3_ARGS, S3Move{}); }      // tune nn1_s3_transposed = 2
#undef PCR_S3_PARAMS
// the transposed form that moves its queries first (MV above): the working cloud is read AND written, one slice only
template <int QG>
__global__ __launch_bounds__(NN_BLOCK, PCR_S2_WAVES) void nn1_strack3_move_kernel(
    const float4* __restrict__ l0_centres, const uint4* __restrict__ l0_ops, const float4* __restrict__ l1_centres, const uint4* __restrict__ l1_ops,
    const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_l0, uint32_t l0_per_slice,
    float* sx, float* sy, float* sz, uint32_t ns, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ stats, uint32_t flush_at,
    uint32_t flush_end, const S3Move mv)
{
    const int* stop = nullptr;
    nn1_strack3_body<QG, true, true>(PCR_S3_ARGS, mv);
}
// ... and the one that finishes the previous iteration first (SV above)
template <int QG>
__global__ __launch_bounds__(NN_BLOCK, PCR_S2_WAVES) void nn1_strack3_solve_move_kernel(
    const float4* __restrict__ l0_centres, const uint4* __restrict__ l0_ops, const float4* __restrict__ l1_centres, const uint4* __restrict__ l1_ops,
    const uint4* __restrict__ ops, const float4* __restrict__ records, uint32_t n_rec, uint32_t n_l0, uint32_t l0_per_slice,
    float* sx, float* sy, float* sz, uint32_t ns, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ stats, uint32_t flush_at,
    uint32_t flush_end, const S3Move mv, const IcpSolveArgs sv)
{
    const int* stop = nullptr;
    nn1_strack3_body<QG, true, true, true>(PCR_S3_ARGS, mv, sv);
}
#undef PCR_S3_ARGS
