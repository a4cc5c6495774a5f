// icp.cpp — host loop of point-to-point ICP (A9), a restatement of
// Registration::ICPpoint2point, Homework9/hw9/src/registration.cpp:862-1011, driving the gfx950 kernels:
//   per iteration: nn1 (correspondences) -> kabsch partial/final (16 f64 sums) -> [one all-reduce when the
//   sources are sharded over GPUs] -> 3x3 SVD on the host (identical on every rank) -> in-place transform.
// The reference's quirks are kept: squared distance vs un-squared max_corr (:936), loss = d2*d2 of the last
// kept pair (:939), `unchanged` never reset (:948-951), det<0 branch (:990-996).
#include "pcr_internal.hpp"
#include "numerics.hpp"

#include <chrono>
#include <cmath>

using namespace pcr;

// the dispatcher's rule (api.cpp nn1_auto_grid) for the searches of a loop
static bool icp_uses_grid(const pcr_ctx* ctx, const pcr_cloud* tgt) { return nn1_auto_grid(ctx, tgt, true, 0); }

// a brute-force loop over a target that takes the matrix-core kernels (>= 8 192 points): the working cloud in the order of the
// target's super-tiles when the loop is long enough to pay for the sort (csrc/grid.hip bt_sort_working_cloud)
static int icp_sort_for_brute(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud** work, uint64_t max_iter)
{
    // (the sort costs ~0.1 ms at 120 k; an iteration of STRACK gains ~0.02 ms from it, one of the sphere forms — targets from 32 768 points — ~0.05 ms:
    // their level-0 / level-1 rows are shared by the 32 queries of a group only when those are neighbours)
    if (max_iter < (tgt->n >= 32768 ? 3u : 8u) || tgt->n < 8192 || tune_get(ctx, "nn1_bf16", 0) == 2) return PCR_OK;
    const int64_t v = tune_get(ctx, "nn1_variant", 0);
    if (v != 0 && v != 6 && v != 7) return PCR_OK;
    return bt_sort_working_cloud(ctx, tgt, work);
}

// The chain search (moves the cloud by the previous solve) -> sums + solve: the loop's own conditions and the search's (nn1_brute.hip
// s3_move_route), from plain numbers — raw tune values, 0 = default.  One rank; tune icp_move_in_search: 0 = auto, 1 = on where possible, 2 = off; the switch
// and the lower bound of the fused sums launch (icp_fused_sums = 2 keeps the three-launch chain, icp_fused_sums_min); STRACK3 in its transposed form with one
// slice of n_l0 level-0 super-tiles.  (What only the running loop knows — the solve + move fused at all, an exhaustive search that seeds itself, the kernel
// family the dispatcher really took — is checked there.)
// Auto = on: the headline A/B of profiles/icp_move_in_search.txt (61.8 -> 59.0 us per step of the bench line, a gain by the rule).
constexpr bool ICP_MOVE_IN_SEARCH_AUTO = true;
bool pcr::icp_move_route(uint64_t n_src, uint64_t n_l0, int nranks, int64_t move_in_search_tune, int64_t fused_sums_tune, int64_t fused_sums_min_tune,
                         int64_t transposed_tune, int64_t qg_tune, int64_t l0_per_slice_tune, int64_t blocks_tune)
{
    if (nranks != 1 || n_src == 0) return false;
    if (move_in_search_tune == 2 || (move_in_search_tune != 1 && !ICP_MOVE_IN_SEARCH_AUTO)) return false;
    if (fused_sums_tune != 0 && fused_sums_tune != 1) return false;
    if ((int64_t)n_src < (fused_sums_min_tune ? fused_sums_min_tune : 60000)) return false;
    return s3_move_route(n_l0, n_src, transposed_tune, qg_tune, l0_per_slice_tune, blocks_tune);
}

// The chain sums -> search (finishes the previous iteration, then moves the cloud), taken only where the chain above would be: whether
// the solve goes into the next search as well.  Tune icp_solve_in_search: 0 = auto, 1 = on where possible, 2 = off; auto holds only while
// icp_move_in_search is at its own default too — a caller that sets that tune to 1 asked for the chain above and keeps it.
// Auto = on up to 131 072 source points: the headline A/B of profiles/icp_solve_in_search.txt (49.06 -> 47.26 us per step of the bench line, a gain by the
// rule; in one process 37.7 -> 35.1 us per iteration at 60 k, 47.6 -> 45.4 at 120 k).  Every workgroup of the search pays the solve before its first
// query is staged, so the launch pays it once per ROUND of resident workgroups: 131 072 points are the 1 024 workgroups of 128 queries that 256 CUs
// hold at four waves per SIMD, and at 250 k (two rounds) the chain loses, 80.5 -> 83.9 us.
constexpr bool ICP_SOLVE_IN_SEARCH_AUTO = true;
constexpr uint64_t ICP_SOLVE_IN_SEARCH_AUTO_MAX = 131072;
bool pcr::icp_solve_route(uint64_t n_src, int64_t solve_in_search_tune, int64_t move_in_search_tune)
{
    if (solve_in_search_tune == 1) return true;
    if (solve_in_search_tune == 2) return false;
    return move_in_search_tune == 0 && ICP_SOLVE_IN_SEARCH_AUTO && n_src <= ICP_SOLVE_IN_SEARCH_AUTO_MAX;
}

// ---- synchronous loop: one host round trip per iteration (needed by the host-callback transport; also the
// reference implementation of the loop the pipelined variant below must reproduce bit for bit)
static int icp_sync(pcr_ctx* ctx, const pcr_cloud* src, const pcr_cloud* tgt, const float init_T[16],
                    const pcr_icp_params* prm, float out_T[16], pcr_icp_stats* stats)
{
    const auto t_begin = std::chrono::steady_clock::now();
    pcr_icp_stats st;
    memset(&st, 0, sizeof st);
    const LoopHint hint(ctx, prm->max_iter);
    ctx->keys_seeded = false;            // (seeds a move of an earlier loop left behind describe positions that no longer exist)
    ctx->icp_last_chain = 0;
    ctx->icp_last_snapshots = 0;

    // prof bookkeeping: report only this call's nn1 time
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    const uint64_t nn_l0 = ctx->prof["nn1_brute"].launches + ctx->prof["nn1_grid"].launches;
    const double nn_ms0 = ctx->prof["nn1_brute"].total_ms + ctx->prof["nn1_grid"].total_ms;

    // pairs are kept only if d2 < max_corr (:936), so the grid search need not look farther (tune icp_bounded_search: 2 = off)
    const float gate = tune_get(ctx, "icp_bounded_search", 1) == 1 ? prm->max_corr : __builtin_inff();
    pcr_cloud* work = nullptr;
    int rc = cloud_alloc(ctx, src->n, &work);                                    // :872 (the copy and the initial transform are one launch)
    if (rc) return rc;
    const float R0[9] = { init_T[0], init_T[1], init_T[2], init_T[4], init_T[5], init_T[6], init_T[8], init_T[9], init_T[10] };
    const float t0[3] = { init_T[3], init_T[7], init_T[11] };
    rc = launch_transform_into(ctx, src, work, R0, t0);                          // :874
    if (rc == PCR_OK) rc = icp_uses_grid(ctx, tgt) ? grid_sort_working_cloud(ctx, tgt, &work) : icp_sort_for_brute(ctx, tgt, &work, prm->max_iter);
    float T_total[16] = { R0[0], R0[1], R0[2], t0[0], R0[3], R0[4], R0[5], t0[1],
                          R0[6], R0[7], R0[8], t0[2], 0, 0, 0, 1 };              // :910-913
    float last_loss = 0.0f;                                                      // :915
    uint64_t unchanged = 0;                                                      // :916
    const int nranks = ctx->comm.nranks, rank = ctx->comm.rank;
    const int nred = icp_nred(nranks);   // limbs of the 16 sums + overflow flag + one (kept flag, last d2) slot per rank
    if (nranks > PCR_MAX_RANKS) { pcr_cloud_destroy(ctx, work); return fail(ctx, PCR_ERR_ARG, "too many ranks"); }
    KabschPlan plan;                     // the fixed-point grid of the exact sums: the same on every rank (target + gate)
    if (rc == PCR_OK) rc = kabsch_plan(ctx, tgt, prm->max_corr, &plan);
    bool overflow = false;

    for (uint64_t iter = 0; rc == PCR_OK && iter < prm->max_iter; iter++) {      // :917
        if ((rc = launch_nn1(ctx, tgt, work, true, gate))) break;                      // :925-934
        double* h = ctx->host_out;
        double sums16[16];
        double last_kept, last_d2;
        hipError_t e = hipSuccess;
        if (nranks > 1 || (ctx->comm.rccl && tune_get(ctx, "icp_force_slots", 0) > 0)) {
            // sharded sources: the block rows are reduced on the device into the all-reduce buffer — the limbs of the exact sums
            // + one (kept flag, last d2) slot per rank so that `loss` is that of the globally last kept pair — which is summed
            // over the ranks by the ONE collective of the iteration (RCCL in place on the context stream, or the caller's
            // reducer on the host copy).  Integer limbs: the result does not depend on the number of ranks.
            uint32_t blocks = 0;
            if (work->n && (rc = launch_kabsch_partial(ctx, tgt, work, prm->max_corr, plan, &blocks))) break;   // :936-940,:964-985
            if ((rc = launch_icp_reduce_slots(ctx, blocks, nranks, rank, work->n != 0, src->gidx))) break;
            if (ctx->comm.rccl && (rc = comm_allreduce_f64_device(ctx, ctx->dev_out, nred))) break;
            e = hipMemcpyAsync(h, ctx->dev_out, nred * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { rc = fail(ctx, PCR_ERR_HIP, "icp d2h", e); break; }
            if (!ctx->comm.rccl && (rc = comm_allreduce_f64(ctx, h, ctx->dev_out, nred))) break;       // host-callback transport
            num::limbs_normalize_row(h);
            num::limbs_to_sums(h, plan.e, sums16);
            overflow = h[55] != 0.0;
            last_kept = -1.0; last_d2 = 0.0;
            const int ls = icp_last_slot(h, nranks);             // the pair with the largest order key: the globally last kept one
            if (ls >= 0) { last_kept = 1.0; last_d2 = h[57 + 2 * ls]; }
        } else {
            if (work->n) {
                if ((rc = launch_kabsch_sums(ctx, tgt, work, prm->max_corr, plan))) break; // :936-940,:964-985
            } else {
                e = hipMemsetAsync(ctx->dev_out, 0, 19 * sizeof(double), ctx->stream);
                if (e != hipSuccess) { rc = fail(ctx, PCR_ERR_HIP, "memset", e); break; }
            }
            e = hipMemcpyAsync(h, ctx->dev_out, 19 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { rc = fail(ctx, PCR_ERR_HIP, "icp d2h", e); break; }
            memcpy(sums16, h, sizeof sums16);
            last_kept = work->n ? h[16] : -1.0;
            last_d2 = work->n ? h[17] : 0.0;
            overflow = work->n && h[18] != 0.0;
        }
        if (overflow) { rc = fail(ctx, PCR_ERR_STATE, "ICP: a kept source point lies more than 2^20 target extents away from the target"); break; }
        float loss = 0.0f;
        if (last_kept >= 0) { const float d2 = (float)last_d2; loss = d2 * d2; } // :939
        st.last_pairs = (uint64_t)sums16[15];
        st.last_loss = loss;
        if (std::fabs(last_loss - loss) < prm->eps) unchanged++;                 // :948-951
        if (unchanged > 15) { st.converged = 1; break; }                         // :954-958
        last_loss = loss;                                                        // :961
        float Rd[9], td[3];
        if (kabsch_solve(sums16, Rd, td) != PCR_OK) { st.empty_pairs = 1; break; }    // :979-998
        const float T_delta[16] = { Rd[0], Rd[1], Rd[2], td[0], Rd[3], Rd[4], Rd[5], td[1],
                                    Rd[6], Rd[7], Rd[8], td[2], 0, 0, 0, 1 };
        mat4_mul_f32(T_delta, T_total, T_total);                                 // :1000-1002
        rc = launch_transform(ctx, work, Rd, td);                                // :1003
        st.iters_run++;
    }
    hipStreamSynchronize(ctx->stream);
    cloud_release(ctx, work);             // (the loop's own working copy: parked for the next call's clone)
    if (rc) return rc;
    memcpy(out_T, T_total, sizeof T_total);                                      // :1008-1009
    prof_flush(ctx);
    st.nn_launches = ctx->prof["nn1_brute"].launches + ctx->prof["nn1_grid"].launches - nn_l0;
    st.ms_nn = ctx->prof["nn1_brute"].total_ms + ctx->prof["nn1_grid"].total_ms - nn_ms0;
    st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return PCR_OK;
}

// ---- pipelined loop: the state machine, the Kabsch solve and the pose composition live on the GPU (IcpState,
// kabsch.hip); iterations are enqueued back to back on the context stream in chunks, the host only looks at a snapshot
// of the state two chunks behind to learn when to stop enqueuing — a copy on the stream behind an event, or, on the chain
// search -> sums + solve, a slot of the host ring that launch writes itself (below).  With RCCL the per-iteration all-reduce is
// enqueued on the same stream, so even the sharded loop needs no host round trip.
static int icp_pipelined(pcr_ctx* ctx, const pcr_cloud* src, const pcr_cloud* tgt, const float init_T[16],
                         const pcr_icp_params* prm, float out_T[16], pcr_icp_stats* stats)
{
    const auto t_begin = std::chrono::steady_clock::now();
    pcr_icp_stats st;
    memset(&st, 0, sizeof st);
    const LoopHint hint(ctx, prm->max_iter);
    ctx->keys_seeded = false;            // (seeds a move of an earlier loop left behind describe positions that no longer exist)
    ctx->icp_last_chain = 0;
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    const uint64_t nn_l0 = ctx->prof["nn1_brute"].launches + ctx->prof["nn1_grid"].launches;
    const double nn_ms0 = ctx->prof["nn1_brute"].total_ms + ctx->prof["nn1_grid"].total_ms;

    constexpr int RING = 4;
    if (!ctx->icp_state_dev) {
        // [1]: the other buffer of the fused solve + move; behind the two states, on a line of its own, the counter of the grid barrier of
        // the fused sums + move launch (kabsch.hip).  Zeroed ONCE: the counter only ever grows, and [1].barrier_timeout must not start as garbage
        static_assert(2 * sizeof(IcpState) <= 512, "the barrier counter lies 512 bytes behind the states");
        // behind the counter's line, on lines of their own: the accumulators of the sums + solve launch (kabsch.hip icp_sums_solve_kernel), zeroed
        // here and left all zero by every launch — two sets of them: the chain sums -> search alternates between the two, every other
        // chain has set 0 alone, and BOTH are all zero between calls
        constexpr size_t acc_bytes = (size_t)ICP_ACC_SETS * ICP_ACC_REPLICAS * ICP_ACC_WORDS * sizeof(long long);
        PCR_HIP(ctx, hipMalloc((void**)&ctx->icp_state_dev, 512 + 128 + acc_bytes));
        PCR_HIP(ctx, hipMemsetAsync(ctx->icp_state_dev, 0, 512 + 128 + acc_bytes, ctx->stream));
        ctx->icp_barrier_dev = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ctx->icp_state_dev) + 512);
        ctx->icp_barrier_arrived = 0;
        ctx->icp_acc_dev = reinterpret_cast<long long*>(reinterpret_cast<char*>(ctx->icp_state_dev) + 512 + 128);
        ctx->icp_acc_dirty = false;
        // the host ring: pinned and explicitly coherent, because the sums + solve launch may store a slot itself (below) and the host
        // reads it while the stream runs on; zeroed, so that no slot carries a sequence number before a launch has written one
        PCR_HIP(ctx, hipHostMalloc((void**)&ctx->icp_state_host, (RING + 1) * sizeof(IcpSnapSlot), hipHostMallocCoherent | hipHostMallocMapped));
        memset(ctx->icp_state_host, 0, (RING + 1) * sizeof(IcpSnapSlot));
        PCR_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->icp_state_host_dev, ctx->icp_state_host, 0));
        for (int k = 0; k < RING; k++) PCR_HIP(ctx, hipEventCreateWithFlags(&ctx->icp_events[k], hipEventDisableTiming));
    }
    if (!ctx->icp_state_host || !ctx->icp_state_host_dev) return fail(ctx, PCR_ERR_STATE, "icp host ring");      // (an earlier call failed half way through the set-up above)
    IcpState* dev = ctx->icp_state_dev;
    IcpSnapSlot* host = ctx->icp_state_host;   // [0..RING) ring of snapshots, [RING] upload / final state
    ctx->icp_last_snapshots = 0;

    // pairs are kept only if d2 < max_corr (:936), so the grid search need not look farther (tune icp_bounded_search: 2 = off)
    const float gate = tune_get(ctx, "icp_bounded_search", 1) == 1 ? prm->max_corr : __builtin_inff();
    pcr_cloud* work = nullptr;
    int rc = cloud_alloc(ctx, src->n, &work);                                    // :872 (the copy and the initial transform are one launch)
    if (rc) return rc;
    const float R0[9] = { init_T[0], init_T[1], init_T[2], init_T[4], init_T[5], init_T[6], init_T[8], init_T[9], init_T[10] };
    const float t0[3] = { init_T[3], init_T[7], init_T[11] };
    rc = launch_transform_into(ctx, src, work, R0, t0);                          // :874
    if (rc == PCR_OK) rc = icp_uses_grid(ctx, tgt) ? grid_sort_working_cloud(ctx, tgt, &work) : icp_sort_for_brute(ctx, tgt, &work, prm->max_iter);
    IcpState& h0 = host[RING].state;
    memset(&h0, 0, sizeof h0);
    const float T0[16] = { R0[0], R0[1], R0[2], t0[0], R0[3], R0[4], R0[5], t0[1], R0[6], R0[7], R0[8], t0[2], 0, 0, 0, 1 };
    memcpy(h0.T_total, T0, sizeof T0);                                           // :910-913
    h0.eps = prm->eps;
    h0.max_iter = prm->max_iter;
    if (prm->max_iter == 0) h0.stop = 1;
    hipError_t e = hipMemcpyAsync(dev, &h0, sizeof h0, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, PCR_ERR_HIP, "icp state upload", e);

    const int nranks = ctx->comm.nranks, rank = ctx->comm.rank;
    const int nred = icp_nred(nranks);
    if (nranks > PCR_MAX_RANKS) { pcr_cloud_destroy(ctx, work); return fail(ctx, PCR_ERR_ARG, "too many ranks"); }   // dev_out / host_out hold 128 f64
    KabschPlan plan;
    if (rc == PCR_OK) rc = kabsch_plan(ctx, tgt, prm->max_corr, &plan);
    int64_t chunk = tune_get(ctx, "icp_chunk", 4);
    if (chunk < 1) chunk = 1;
    const bool force_slots = tune_get(ctx, "icp_force_slots", 0) > 0;
    // small clouds on one rank: the solve and the move share a launch (kabsch.hip icp_update_move_kernel; tune icp_fused_move: 2 = off);
    // the state then alternates between dev[0] and dev[1]: iteration k reads dev[k & 1] and writes dev[(k + 1) & 1]
    // (round 3: up to 262 144 points — with the seed of the next search folded in as well, the chain of a 120 k iteration is search ->
    // sums -> solve + move + seed: three launches instead of five)
    const int64_t fused_max = tune_get(ctx, "icp_fused_max", 262144);
    const bool fused = nranks == 1 && !force_slots && work->n > 0 && work->n <= (size_t)fused_max && tune_get(ctx, "icp_fused_move", 1) == 1;
    // exhaustive searches of a loop seed themselves from the previous correspondences: the move writes those seeds (tune icp_seed_in_move: 2 = off)
    const pcr_cloud* seed_tgt = (!icp_uses_grid(ctx, tgt) && tune_get(ctx, "icp_seed_in_move", 1) == 1 && tune_get(ctx, "nn1_warm_start", 1) == 1) ? tgt : nullptr;
    // the sums as well in that launch (kabsch.hip icp_sums_update_move_kernel; tune icp_fused_sums: 2 = off): search -> sums + solve + move
    // + seed, two launches, where the cloud has at least icp_fused_sums_min points and takes at most one workgroup per CU (icp_fused_sums_max_blocks);
    // otherwise the three-launch chain.  Exhaustive loops only by default: the kernel serves the grid loop too (targets by index; icp_fused_sums_grid = 1,
    // same bits), but that was measured only at hw9's 4 000 points, where it loses
    const bool fused_sums = fused && (!icp_uses_grid(ctx, tgt) || tune_get(ctx, "icp_fused_sums_grid", 0) == 1) && icp_fused_sums_blocks(ctx, work->n) != 0;
    // A third chain (tune icp_move_in_search: 2 = off): search -> sums + solve (kabsch.hip icp_sums_solve_kernel), and the search of iteration
    // k + 1 moves the cloud by the Rd, td of solve k while it loads its queries, seeding itself on the way (nn1_sphere.hpp, MV) — no grid barrier, no
    // residency condition, and no move at all behind the last solve: the working cloud is released, only T_total is returned.  Conditions: those of the
    // fused solve + move above, a search that seeds itself (seed_tgt), the switch and the lower bound of the fused sums launch, and STRACK3 in its transposed
    // form with ONE slice (every target of up to 131 072 records; larger ones where the queries alone fill the launch) — icp_move_route.  The dispatcher decides the kernel family late, so the chain is chosen behind
    // the FIRST search, which runs as ever (nothing to move yet): if it did not take STRACK3, the whole call keeps one of the chains above; a later search
    // that cannot carry the move is an error of the dispatcher, not a fallback.
    // The sums + solve launch hands a workgroup's limb totals on as int64 atomic adds into eight accumulator rows, not as a row per workgroup (DESIGN.md
    // 6i, profiles/icp_sums_accumulators.txt): the last arriver reads eight short rows whatever the geometry, so the launch runs 512 threads x 2 pairs
    // on 118 workgroups — kernel 19.9 -> 17.5 us, a step of the bench line 53.4 -> 50.9 us (8 + 8 alternating processes, spreads 2.5 / 0.9).  What
    // now bounds it: the last arriver has its ticket back and its acquire done ~35 ns per arriving workgroup later (4 - 5 us at 118, 9 at 235, 16 at 469),
    // then the solve.  A ticket per replica (tune icp_ticket_levels = 2: arrivals queue as 15 + 8) does not shorten that wait — 4.1 - 5.5 us
    // at 118 workgroups, 8.1 - 11.2 at 235 — so they are not a queue at one address; one counter stays the default.  What the chain sums -> search
    // (below, DESIGN.md 6k, profiles/icp_solve_in_search.txt) found about that wait: it is a cost of handing the sums over INSIDE a launch and of nothing
    // else.  The same front half with the same atomics and no release, ticket or acquire behind them is a launch of 7.8 us at 118 workgroups (17.4 with
    // the hand-over and the solve) and 6.8 us at 235; the next launch finds the rows complete and has them in LDS 0.15 us after the loads it requests
    // beside its own come back.  The solve itself does not get cheaper by moving: 5.5 - 6.2 us in the last arriver, 6.8 - 9.4 us as one wave of each of
    // 938 workgroups, which all wait for it.
    const bool move_cand = fused && seed_tgt && icp_sums_solve_blocks(ctx, work->n) != 0;
    bool move_in_search = false;
    // A fourth chain (tune icp_solve_in_search): search -> sums (kabsch.hip icp_sums_kernel), and the search of iteration k + 1 FINISHES
    // iteration k in its prologue — every workgroup reads the eight accumulator rows and reduces, solves and steps the state for itself (nn1_sphere.hpp,
    // SV; icp_finish.hpp) — before it moves the cloud; behind the last sums launch of a call ONE wave does the same (icp_finish_kernel).  No release, no
    // ticket and no acquire anywhere: every dependency is a launch boundary of the stream.  Taken where the chain above is (icp_solve_route).  State k
    // (after k iterations) is published by workgroup 0 of search k into dev[k & 1]; iteration k adds into accumulator set k & 1 and zeroes the other.
    bool solve_in_search = false;
    // (Measured and dropped, round 4: the Kabsch sums taken by the search kernel itself — STRACK3 ends with every query's final key in one wave, so each
    // wave added its 32 pairs' limbs (wave sums, a row per workgroup, f64 atomics into 64 rows; same bits) and the streaming pass + its launch gap
    // (7 + 4.5 us) went away: the search grew from 0.034 to 0.049 ms — 41 limbs x 6 f64 shuffle-adds per wave, four waves per SIMD ending together on
    // the LDS crossbar and the half-rate f64 pipe — and an iteration from 0.0707 to 0.0755 ms.  A second form without any cross-lane traffic (lane l takes
    // moment l of the wave's 32 pairs from LDS) still cost the search 7.5 us — the block waits for its slowest wave, every wave ends 2 us later — for 0-1.3 us
    // per iteration.  Also measured: the 3 x 3 solve is 4.6 of the 17.5 us of the solve + move.
    // Measured now (profiles/icp_fused_sums.txt): the sums in the solve + move launch instead, behind one grid barrier — 7.8 + 17.3 us of kernels become 23.1 us,
    // the search keeps its 26.2 us, and a step of the bench line goes from 63.6 to 61.8 us.)
    // State snapshots of that chain (profiles/icp_host_snapshots.txt; tune icp_host_snapshots: 2 = off): the sums + solve launch that ends
    // a chunk, or the call, is handed a slot of the host ring and a sequence number; its publishing workgroup stores the state there itself and then
    // the number, a system-scope release (0.6 us on the launches that do it).  No copy and no event on the stream: the blit kernel (4.3 us) and the
    // event's marker (5 - 6 us before the next search started) stood in the dependent chain once per chunk.  The host polls the slot two chunks back
    // for its number (the stream bounds the poll, below) and reads the final state from the slot of the last launch once the stream has drained: a
    // step of the bench line 50.9 -> 48.9 us.  Every other chain, and a call of no iteration, keeps its copies and events.
    const bool snap_cand = tune_get(ctx, "icp_host_snapshots", 1) == 1;
    bool snaps = false;
    unsigned long long ring_seq[RING + 1] = { 0, 0, 0, 0, 0 };      // the number each slot was last promised
    int last_slot = -1;                                              // the slot the last sums + solve launch of the call writes
    uint64_t enq = 0, chunks = 0;
    bool stopped = false;
    while (rc == PCR_OK && !stopped && enq < prm->max_iter) {
        for (int64_t c = 0; rc == PCR_OK && c < chunk && enq < prm->max_iter; c++, enq++) {   // :917
            IcpState* cur = fused ? dev + (enq & 1) : dev;                                        // the state this iteration starts from
            ctx->stop_flag_dev = &cur->stop;     // correspondence kernels no-op once stop or stop_after_transform is set
            ctx->nn1_move_state = move_in_search ? cur : nullptr;        // (iteration 0 decides: nothing to move in front of it)
            IcpSolveArgs sv = { nullptr, nullptr, nullptr, nullptr, 0ull, 0 };
            if (solve_in_search) {
                // this search finishes iteration enq - 1: from the state that one started from and the set its sums went into, to `cur`.  The first
                // search of a chunk thereby publishes the state behind the previous chunk: it gets that chunk's slot of the ring
                const int slot = snaps && c == 0 ? (int)((chunks - 1) % RING) : -1;
                if (slot >= 0) ring_seq[slot] = ++ctx->icp_snap_seq;
                sv = IcpSolveArgs{ ctx->icp_acc_dev + (size_t)((enq - 1) & 1) * ICP_ACC_REPLICAS * ICP_ACC_WORDS, cur, ctx->dev_out,
                                   slot >= 0 ? ctx->icp_state_host_dev + slot : nullptr, slot >= 0 ? ring_seq[slot] : 0ull, plan.e };
                ctx->nn1_move_state = dev + ((enq - 1) & 1);
                ctx->nn1_solve = &sv;
            }
            rc = launch_nn1(ctx, tgt, work, true, gate);                                          // :925-934
            ctx->nn1_move_state = nullptr;
            ctx->nn1_solve = nullptr;
            if (rc) break;
            if (enq == 0)
                move_in_search = move_cand && ctx->nn1_move_l0 != 0 &&
                                 icp_move_route(work->n, ctx->nn1_move_l0, nranks, tune_get(ctx, "icp_move_in_search", 0), tune_get(ctx, "icp_fused_sums", 0),
                                                tune_get(ctx, "icp_fused_sums_min", 0), tune_get(ctx, "nn1_s3_transposed", 0), tune_get(ctx, "nn1_sphere_qg", 0),
                                                tune_get(ctx, "nn1_sphere_l0_per_slice", 0), tune_get(ctx, "nn1_sphere_blocks", 0));
            else if (move_in_search && !ctx->nn1_moved) { rc = fail(ctx, PCR_ERR_STATE, "ICP: a search of the chain search -> sums + solve did not move the cloud"); break; }
            if (enq == 0) snaps = move_in_search && snap_cand;
            if (enq == 0) solve_in_search = move_in_search && icp_solve_route(work->n, tune_get(ctx, "icp_solve_in_search", 0), tune_get(ctx, "icp_move_in_search", 0));
            if (solve_in_search) {
                if ((rc = launch_icp_sums(ctx, tgt, work, prm->max_corr, cur, plan, (int)(enq & 1)))) break;                                          // :936-940
                continue;
            }
            if (move_in_search) {
                // the last launch of the call writes slot [RING], the last of any other chunk the chunk's slot of the ring, the others none
                const bool ends_call = enq + 1 == prm->max_iter, ends_chunk = c + 1 == chunk;
                const int slot = !snaps ? -1 : ends_call ? RING : ends_chunk ? (int)(chunks % RING) : -1;
                if (slot >= 0) ring_seq[slot] = ++ctx->icp_snap_seq;
                if ((rc = launch_icp_sums_solve(ctx, tgt, work, prm->max_corr, cur, dev + ((enq + 1) & 1), plan,                                     // :936-1002
                                                slot >= 0 ? ctx->icp_state_host_dev + slot : nullptr, slot >= 0 ? ring_seq[slot] : 0ull))) break;
                if (slot >= 0) last_slot = slot;
                continue;
            }
            if (fused_sums) {
                if ((rc = launch_icp_sums_update_move(ctx, tgt, work, prm->max_corr, cur, dev + ((enq + 1) & 1), plan, seed_tgt))) break;   // :936-1003
                continue;
            }
            uint32_t blocks = 0;
            if (work->n && (rc = launch_kabsch_partial(ctx, tgt, work, prm->max_corr, plan, &blocks))) break;   // :936-940,:964-985
            if (fused) {
                if ((rc = launch_icp_update_move(ctx, blocks, cur, dev + ((enq + 1) & 1), plan, work, seed_tgt))) break;   // :948-1003
                continue;
            }
            if (nranks == 1 && work->n && !force_slots) {
                if ((rc = launch_icp_update(ctx, blocks, dev, plan))) break;                // :948-1002
            } else {
                if ((rc = launch_icp_reduce_slots(ctx, blocks, nranks, rank, work->n != 0, src->gidx))) break;
                if ((rc = comm_allreduce_f64_device(ctx, ctx->dev_out, nred))) break;       // the ONE collective
                if ((rc = launch_icp_update_from_sums(ctx, nranks, dev, plan))) break;
            }
            if ((rc = launch_transform_state(ctx, work, dev, seed_tgt))) break;             // :1003
        }
        ctx->stop_flag_dev = nullptr;
        if (rc) break;
        const int slot = (int)(chunks % RING);
        if (!snaps) {
            // (the chain sums -> search: the state behind this chunk is the next search's to publish — the copy takes the newest one there is, one
            // iteration older; what the host sees only decides when it stops enqueuing)
            e = hipMemcpyAsync(&host[slot].state, solve_in_search ? dev + ((enq - 1) & 1) : fused ? dev + (enq & 1) : dev, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ctx->icp_events[slot], ctx->stream);
            if (e != hipSuccess) { rc = fail(ctx, PCR_ERR_HIP, "icp snapshot", e); break; }
        }
        chunks++;
        if (chunks >= 2) {
            // look two chunks back: deterministic (the same on every rank), and the GPU never runs dry
            const int old = (int)((chunks - 2) % RING);
            if (snaps) {
                // the slot carries its number once the launch that ends that chunk has published.  The poll is bounded by the stream, not by a clock:
                // any answer of hipStreamQuery but "not ready" ends it, and a stream that has drained has run that launch, so the slot must carry
                // the number then.  But the stream is asked only once the number is SNAP_PATIENCE late — many times a chunk of the loops that take
                // this chain — and between all reads from then on: the first query behind a kernel launch puts a marker packet on the stream to
                // have something to ask after, and that marker, asked for at every chunk, was the 5.9 us gap in front of the next chunk's first
                // search all over again (profiles/icp_host_snapshots.txt section 2)
                constexpr auto SNAP_PATIENCE = std::chrono::milliseconds(2);
                hipError_t q = hipErrorNotReady;
                bool seen = false, ask = false;
                const auto t_poll = std::chrono::steady_clock::now();
                for (uint32_t spin = 0; ; spin++) {
                    seen = __atomic_load_n(&host[old].seq, __ATOMIC_ACQUIRE) == ring_seq[old];
                    if (seen || q != hipErrorNotReady) break;        // (behind an answer of the stream the slot has been read once more)
                    if (!ask && (spin & 255u) == 255u) ask = std::chrono::steady_clock::now() - t_poll > SNAP_PATIENCE;
                    if (ask) q = hipStreamQuery(ctx->stream);
                }
                if (q == hipErrorNotReady) (void)hipGetLastError();  // (the stream's "not ready" is no launch's error: the next launch check must not find it)
                if (!seen) {
                    rc = q == hipSuccess ? fail(ctx, PCR_ERR_STATE, "ICP: the stream drained and a state snapshot never arrived in the host ring")
                                         : fail(ctx, PCR_ERR_HIP, "icp snapshot wait", q);
                    break;
                }
            } else {
                e = hipEventSynchronize(ctx->icp_events[old]);
                if (e != hipSuccess) { rc = fail(ctx, PCR_ERR_HIP, "icp snapshot wait", e); break; }
            }
            const IcpState& o = host[old].state;
            if (o.stop || o.stop_after_transform || o.barrier_timeout) stopped = true;
        }
    }
    ctx->stop_flag_dev = nullptr;
    // the chain sums -> search: the last iteration enqueued is finished by a launch of its own, which publishes like the sums + solve launch of a call's end
    if (rc == PCR_OK && solve_in_search && enq > 0) {
        if (snaps) ring_seq[RING] = ++ctx->icp_snap_seq;
        rc = launch_icp_finish(ctx, dev + ((enq - 1) & 1), dev + (enq & 1), plan, (int)((enq - 1) & 1), snaps ? ctx->icp_state_host_dev + RING : nullptr,
                               snaps ? ring_seq[RING] : 0ull);
        if (rc == PCR_OK && snaps) last_slot = RING;
    }
    // the final state: from the slot the last sums + solve launch wrote, once the stream has drained — or, on every other chain and behind a call that
    // enqueued no such launch (max_iter = 0), by a copy behind the last launch
    const bool final_in_slot = snaps && last_slot >= 0;
    const IcpState& f = host[final_in_slot ? last_slot : RING].state;
    if (rc == PCR_OK) {
        e = final_in_slot ? hipSuccess : hipMemcpyAsync(&host[RING].state, fused ? dev + (enq & 1) : dev, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, PCR_ERR_HIP, "icp state download", e);
        else if (final_in_slot && __atomic_load_n(&host[last_slot].seq, __ATOMIC_ACQUIRE) != ring_seq[last_slot])
            rc = fail(ctx, PCR_ERR_STATE, "ICP: the stream drained and the final state never arrived in the host ring");
    } else {
        hipStreamSynchronize(ctx->stream);
    }
    cloud_release(ctx, work);             // (synchronised above; the loop's own working copy: parked for the next call's clone)
    // the accumulators of the sums + solve launch are all zero behind a call that ran to its end; one that did not says so, and the next call clears them
    if (move_in_search && (rc || f.overflow || f.barrier_timeout)) ctx->icp_acc_dirty = true;
    if (rc) return rc;
    ctx->icp_last_chain = solve_in_search ? 5 : move_in_search ? 4 : fused_sums ? 3 : fused ? 2 : 1;
    ctx->icp_last_snapshots = final_in_slot ? 1 : 0;
    if (f.overflow) return fail(ctx, PCR_ERR_STATE, "ICP: a kept source point lies more than 2^20 target extents away from the target");
    if (f.barrier_timeout) {
        // (the flag must not outlive the call in the state buffer the next call does not upload)
        hipMemsetAsync(dev, 0, 2 * sizeof(IcpState), ctx->stream);
        return fail(ctx, PCR_ERR_STATE, "ICP: the workgroups of the fused sums + move launch did not meet at their grid barrier in time (tune icp_fused_sums = 2 runs the three-launch chain)");
    }
    memcpy(out_T, f.T_total, sizeof f.T_total);                                  // :1008-1009
    st.iters_run = f.iters_run;
    st.converged = f.converged;
    st.empty_pairs = f.empty;
    st.last_pairs = f.last_pairs;
    st.last_loss = f.loss;
    prof_flush(ctx);
    st.nn_launches = ctx->prof["nn1_brute"].launches + ctx->prof["nn1_grid"].launches - nn_l0;
    st.ms_nn = ctx->prof["nn1_brute"].total_ms + ctx->prof["nn1_grid"].total_ms - nn_ms0;
    st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = st;
    return PCR_OK;
}

extern "C" int pcr_icp_last_chain(const pcr_ctx* ctx) { return ctx ? ctx->icp_last_chain : 0; }
extern "C" int pcr_icp_last_snapshots(const pcr_ctx* ctx) { return ctx ? ctx->icp_last_snapshots : 0; }
extern "C" uint32_t pcr_icp_replica_members(uint32_t blocks, uint32_t replica) { return icp_replica_members(blocks, replica); }

extern "C" int pcr_icp_move_route(uint64_t n_src, uint64_t n_tgt, int nranks, int64_t move_in_search, int64_t fused_sums, int64_t fused_sums_min,
                                  int64_t s3_transposed, int64_t sphere_qg, int64_t sphere_l0_per_slice, int64_t sphere_blocks)
{
    return icp_move_route(n_src, s3_l0_super_tiles(n_tgt), nranks, move_in_search, fused_sums, fused_sums_min, s3_transposed, sphere_qg, sphere_l0_per_slice,
                          sphere_blocks) ? 1 : 0;
}

extern "C" int pcr_icp_solve_route(uint64_t n_src, uint64_t n_tgt, int nranks, int64_t solve_in_search, int64_t move_in_search, int64_t fused_sums,
                                   int64_t fused_sums_min, int64_t s3_transposed, int64_t sphere_qg, int64_t sphere_l0_per_slice, int64_t sphere_blocks)
{
    return pcr_icp_move_route(n_src, n_tgt, nranks, move_in_search, fused_sums, fused_sums_min, s3_transposed, sphere_qg, sphere_l0_per_slice, sphere_blocks) &&
           icp_solve_route(n_src, solve_in_search, move_in_search) ? 1 : 0;
}
extern "C" uint64_t pcr_icp_solve_in_search_auto(void) { return ICP_SOLVE_IN_SEARCH_AUTO ? ICP_SOLVE_IN_SEARCH_AUTO_MAX : 0; }

extern "C" int pcr_icp_p2p_f32(pcr_ctx* ctx, const pcr_cloud* src, const pcr_cloud* tgt, const float init_T[16],
                               const pcr_icp_params* prm, float out_T[16], pcr_icp_stats* stats)
{
    if (!ctx || !src || !tgt || !init_T || !prm || !out_T) return fail(ctx, PCR_ERR_ARG, "pcr_icp_p2p_f32");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    // tune "icp_pipeline": 1 = device-resident pipelined loop, -1 = synchronous loop (one host round trip per iteration),
    // 0 = auto = pipelined.  Measured on MI355X in round 2 (brute force, 120 k target, 20 iterations): 1.237 vs 1.242 ms per
    // iteration with all 120 k sources, 0.211 vs 0.217 ms with a 1/8 shard (what one rank of an 8-GPU strong-scaling run
    // holds), tens of microseconds per iteration with the grid search — the device-resident loop is never slower, and with
    // RCCL it keeps the per-iteration all-reduce on the stream.  The host-callback transport reduces on the host and
    // therefore always runs synchronously.  Both loops give bit-identical results.
    const bool callback = ctx->comm.nranks > 1 && ctx->comm.cb != nullptr;
    const int64_t mode = tune_get(ctx, "icp_pipeline", 0);
    const bool pipelined = !callback && mode >= 0;
    return pipelined ? icp_pipelined(ctx, src, tgt, init_T, prm, out_T, stats) : icp_sync(ctx, src, tgt, init_T, prm, out_T, stats);
}
