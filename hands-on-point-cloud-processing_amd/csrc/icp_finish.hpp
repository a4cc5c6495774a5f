// icp_finish.hpp — the back half of an ICP iteration on one rank, shared by the launches that run it: accumulator rows -> carries -> the 16 moments ->
// state machine, Kabsch solve and pose composition (registration.cpp:939-1002).  kabsch.hip's sums + solve launch (chain 4) runs these
// steps in its last arriver; the chain sums -> search (chain 5) runs them, as ONE WAVE (finish_iteration), in every workgroup of the moving
// search (nn1_sphere.hpp) and in the finishing launch of a call (kabsch.hip).  One text for all of them: the bits are the same by construction.  The solve and
// the pose composition are worked by a whole wave (icp_state_step_wave, kabsch_wave.hpp) wherever the state is stepped on the device.
#pragma once

#include "pcr_internal.hpp"
#include "numerics.hpp"
#include "kabsch_wave.hpp"

#include <cstddef>

#pragma clang fp contract(off)

namespace pcr {

constexpr int KB_NL = num::KB_NL;     // 55 normalised limbs (numerics.hpp)
constexpr int KB_ROW = 58;            // a partial row: KB_NL limbs, [55] last-kept key (u64 bits), [56] overflow flag, [57] pad
constexpr int KB_NLC = 40;            // the limbs that are not carry slots (12 + 27) + the count

// thread / lane k converts moment k of a normalised row; 16: the last kept pair and the overflow flag
__device__ __forceinline__ void row_to_out18(int k, const double (&row)[KB_ROW], int e, double* out)
{
    if (k < 6) out[k] = num::limbs_value(row + 3 * k, 2, e - 2 * num::KB_W);
    else if (k < 15) out[k] = num::limbs_value(row + 18 + 4 * (k - 6), 3, 2 * e - 3 * num::KB_W);
    else if (k == 15) out[15] = row[54];
    else if (k == 16) {
        const unsigned long long lk = (unsigned long long)__double_as_longlong(row[55]);
        out[16] = row[54] > 0.0 ? (double)(uint32_t)(lk >> 32) : -1.0;
        out[17] = row[54] > 0.0 ? (double)__uint_as_float((uint32_t)(lk & 0xFFFFFFFFull)) : 0.0;
        out[18] = row[56];
    }
}
__device__ __forceinline__ void row_to_out18(const double (&row)[KB_ROW], int e, double* out) { row_to_out18((int)threadIdx.x, row, e, out); }

// ---------------------------------------------------------------------------------------------- device-resident ICP state
// The pipelined ICP loop (icp.cpp) keeps the whole state machine of registration.cpp:915-1006 on the GPU so that
// iterations are enqueued back to back without a host round trip: nn1 -> kabsch_partial -> icp_update -> transform.

// state machine + Kabsch solve + pose composition, one thread (registration.cpp:939-1002).  `st` is the workgroup's LDS copy of
// the state (icp_state_stage): the step is one thread's serial chain, and every field it touched in HBM was a dependent memory
// round trip of that chain (stop -> stop_after_transform -> last_loss, eps -> unchanged -> T_total ...).
__device__ __forceinline__ void icp_state_step(IcpState* st, const double* sums16, bool any_kept, float last_d2, bool overflow)
{
    if (st->stop) return;
    if (st->stop_after_transform) { st->stop = 1; return; }   // max_iter reached: the loop is over
    if (overflow) { st->overflow = 1; st->stop = 1; return; }  // a kept source beyond the accumulation grid (kabsch_plan)
    float loss = 0.0f;
    if (any_kept) loss = last_d2 * last_d2;                                      // :939
    st->last_pairs = (unsigned long long)sums16[15];
    st->loss = loss;
    if (fabsf(st->last_loss - loss) < st->eps) st->unchanged++;                  // :948-951
    if (st->unchanged > 15) { st->converged = 1; st->stop = 1; return; }         // :954-958
    st->last_loss = loss;                                                        // :961
    float Rd[9], td[3];
    if (num::kabsch_solve(sums16, Rd, td) != 0) { st->empty = 1; st->stop = 1; return; }   // :979-998
    const float T_delta[16] = { Rd[0], Rd[1], Rd[2], td[0], Rd[3], Rd[4], Rd[5], td[1],
                                Rd[6], Rd[7], Rd[8], td[2], 0, 0, 0, 1 };
    num::mat4_mul_f32(T_delta, st->T_total, st->T_total);                        // :1000-1002
    for (int k = 0; k < 9; k++) st->Rd[k] = Rd[k];
    for (int k = 0; k < 3; k++) st->td[k] = td[k];
    st->iters_run++;
    // max_iter reached: this iteration's transform must still run, everything after it must not
    if (st->iters_run >= st->max_iter) st->stop_after_transform = 1;
}

// the whole state in ONE coalesced read: thread w copies 32-bit word w
constexpr int ST_WORDS = (int)(sizeof(IcpState) / 4);
static_assert(sizeof(IcpState) % 4 == 0 && ST_WORDS <= 64, "IcpState is staged by one wave, one word per lane");

// carry propagation of one sum in integer arithmetic, the rule of num::limbs_normalize (quotient truncated toward zero, remainder with the dividend's
// sign, carry into the next limb): L[0..n) limbs, L[n] the carry limb; out[] the normalised f64 limbs.  The quotient by 2^40 is a shift of the
// dividend, biased by 2^40 - 1 where it is negative (an arithmetic shift alone rounds toward minus infinity)
__device__ __forceinline__ void limbs_normalize_i64(long long* L, int n, double* out)
{
    constexpr long long W = 1ll << num::KB_W;
    for (int j = 0; j < n; j++) {
        const long long c = (L[j] + ((L[j] >> 63) & (W - 1))) >> num::KB_W;
        L[j] -= c * W;
        L[j + 1] += c;
        out[j] = (double)L[j];
    }
    out[n] = (double)L[n];
}

constexpr int ACC_R = ICP_ACC_REPLICAS, ACC_W = ICP_ACC_WORDS;      // words of a replica: [0..40) live limbs, [40] overflow count, [41] key, pad to 3 lines
constexpr int ACC_CNT = KB_NLC + 2;                                  // [42] the replica's arrival counter where every replica has a ticket of its own (6j)
static_assert((ACC_R & (ACC_R - 1)) == 0 && ACC_W * 8 % 128 == 0 && ACC_W >= KB_NLC + 3, "replicas: a power of two, whole 128-byte lines");

// word k of the replicas in s_acc -> replica 0's place: the sums of the limbs and of the overflow counts, the maximum of the keys (thread k alone reads and
// writes column k)
__device__ __forceinline__ void acc_fold_column(long long (&s_acc)[ACC_R][ACC_W], int k)
{
    long long v = s_acc[0][k];
#pragma unroll
    for (int r = 1; r < ACC_R; r++) {
        const long long o = s_acc[r][k];
        v = k == KB_NLC + 1 ? (long long)((unsigned long long)o > (unsigned long long)v ? o : v) : v + o;
    }
    s_acc[0][k] = v;
}

// ... and the folded words -> a normalised row: thread k < 15 takes sum k (its 2 or 3 live limbs, then the carries), 15 the count, 16 the key and the flag
__device__ __forceinline__ void acc_to_row(const long long (&s_acc)[ACC_R][ACC_W], int k, double (&row)[KB_ROW])
{
    if (k < 15) {
        const int nl = k < 6 ? 2 : 3, p0 = k < 6 ? 2 * k : 12 + 3 * (k - 6), s0 = k < 6 ? 3 * k : 18 + 4 * (k - 6);
        long long L[4] = { 0, 0, 0, 0 };
        for (int j = 0; j < nl; j++) L[j] = s_acc[0][p0 + j];
        limbs_normalize_i64(L, nl, row + s0);
    } else if (k == 15) {
        row[54] = (double)s_acc[0][KB_NLC - 1];
    } else if (k == 16) {
        row[55] = __longlong_as_double(s_acc[0][KB_NLC + 1]);
        row[56] = s_acc[0][KB_NLC] != 0 ? 1.0 : 0.0;
        row[57] = 0.0;
    }
}

// ---- chain 5: the steps above as ONE WAVE, for a caller that owns no workgroup barrier at this point.  The lanes of a wave run in
// lockstep and their LDS accesses complete in order; what the steps need between them is that the compiler keeps that order
__device__ __forceinline__ void fin_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// icp_state_step by ONE WAVE, all 64 lanes of it: the Kabsch solve and the pose composition are kabsch_wave.hpp's lane form — the same
// operations on the same operands, spread over the lanes —; the state machine's decisions are made by every lane alike on what it read from `st` before
// any lane wrote there, and lane 0 alone writes the scalar fields.  `st` and `sums16` are in LDS, complete (the caller's fin_wave_sync or barrier stands
// in front); behind the call's closing fin_wave_sync every lane may read the new state.  -DPCR_SOLVE_SCALAR: lane 0 runs the scalar step (the A/B arm)
__device__ __forceinline__ void icp_state_step_wave(int l, IcpState* st, const double* sums16, bool any_kept, float last_d2, bool overflow)
{
#ifdef PCR_SOLVE_SCALAR
    if (l == 0) icp_state_step(st, sums16, any_kept, last_d2, overflow);
    fin_wave_sync();
#else
    const int stop = st->stop, after = st->stop_after_transform;
    const float last_loss = st->last_loss, eps = st->eps, T_mine = st->T_total[l & 15];
    unsigned long long unchanged = st->unchanged;
    const unsigned long long iters_run = st->iters_run, max_iter = st->max_iter;
    fin_wave_sync();                           // (every lane has read what it decides on)
    if (!__builtin_amdgcn_readfirstlane(stop)) {
        if (__builtin_amdgcn_readfirstlane(after)) { if (l == 0) st->stop = 1; }       // max_iter reached: the loop is over
        else if (__builtin_amdgcn_readfirstlane((int)overflow)) { if (l == 0) { st->overflow = 1; st->stop = 1; } }  // a kept source beyond the accumulation grid
        else {
            float loss = 0.0f;
            if (any_kept) loss = last_d2 * last_d2;                                      // :939
            if (fabsf(last_loss - loss) < eps) unchanged++;                              // :948-951
            const bool converged = __builtin_amdgcn_readfirstlane((int)(unchanged > 15)) != 0;
            if (l == 0) {
                st->last_pairs = (unsigned long long)sums16[15];
                st->loss = loss;
                st->unchanged = unchanged;
                if (converged) { st->converged = 1; st->stop = 1; }                      // :954-958
                else st->last_loss = loss;                                               // :961
            }
            if (!converged) {
                const num::WaveLanes g{ l };
                float R = 0.0f, t = 0.0f;
                if (num::kabsch_solve_lanes(g, sums16, R, t) != 0) { if (l == 0) { st->empty = 1; st->stop = 1; } }   // :979-998
                else {
                    const float T_new = num::pose_compose_lanes(g, R, t, T_mine);         // :1000-1002
                    if (l < 9) st->Rd[l] = R;
                    if (l < 3) st->td[l] = t;
                    if (l < 16) st->T_total[l] = T_new;
                    // max_iter reached: this iteration's transform must still run, everything after it must not
                    if (l == 0) { st->iters_run = iters_run + 1; if (iters_run + 1 >= max_iter) st->stop_after_transform = 1; }
                }
            }
        }
    }
    fin_wave_sync();
#endif
}

struct IcpFinishLds {
    long long acc[ACC_R][ACC_W];
    double row[KB_ROW];
    double o18[19];
    IcpState st;
#ifdef PCR_SV_PROF
    unsigned long long pt_replicas;        // (profile build: when the solving wave had the replicas in LDS)
#endif
};

// What a lane of that wave requests up front, in ONE trip beside the caller's own loads: word l of the iteration's INPUT state (lanes below ST_WORDS)
// and its share of the iteration's accumulator set — complete since an earlier launch (icp_sums_kernel) and only read here; relaxed agent-scope loads,
// past this CU's L1.  The rows are requested whatever the state will say: in the stopped phases they are zeros nobody looks at
constexpr int FIN_ACC_PER_LANE = ACC_R * ACC_W / 64;
static_assert(ACC_R * ACC_W % 64 == 0, "a wave reads the replicas in whole rounds");
struct IcpFinishLoads {
    uint32_t stw;
    long long acc[FIN_ACC_PER_LANE];
};
__device__ __forceinline__ void finish_request(int l, const IcpState* st_in, const long long* acc, IcpFinishLoads& Q)
{
    Q.stw = 0;
    if (l < ST_WORDS) Q.stw = reinterpret_cast<const uint32_t*>(st_in)[l];
#pragma unroll
    for (int i = 0; i < FIN_ACC_PER_LANE; i++) Q.acc[i] = __hip_atomic_load(acc + l + 64 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Lane l of one wave, with what it requested.  Leaves the iteration's OUTPUT state in F.st and, where the iteration stepped (returns true), the 19
// doubles of the sums in F.o18.  A stopped loop or one behind its last transform only forwards the state, stopped, as the sums + solve launch does in
// its phases 0 and 1
__device__ __forceinline__ bool finish_iteration(int l, const IcpFinishLoads& Q, int e, IcpFinishLds& F)
{
    const uint32_t stw = Q.stw;
    if (l < ST_WORDS) reinterpret_cast<uint32_t*>(&F.st)[l] = stw;
    fin_wave_sync();
    if (F.st.stop || F.st.barrier_timeout || F.st.stop_after_transform) {
        fin_wave_sync();                   // (every lane has read the flags)
        if (l == 0) F.st.stop = 1;
        fin_wave_sync();
        return false;
    }
#pragma unroll
    for (int i = 0; i < FIN_ACC_PER_LANE; i++) (&F.acc[0][0])[l + 64 * i] = Q.acc[i];
    fin_wave_sync();
#ifdef PCR_SV_PROF
    if (l == 0) F.pt_replicas = __builtin_amdgcn_s_memrealtime();
#endif
    if (l < KB_NLC + 2) acc_fold_column(F.acc, l);
    fin_wave_sync();
    acc_to_row(F.acc, l, F.row);
    fin_wave_sync();
    row_to_out18(l, F.row, e, F.o18);
    fin_wave_sync();
    icp_state_step_wave(l, &F.st, F.o18, F.o18[16] >= 0.0, (float)F.o18[17], F.o18[18] != 0.0);
    return true;
}

// ... and what the ONE publisher of an iteration does with it (workgroup 0 of the moving search, or the finishing launch): the sums to out, the state to
// the other state slot, and — where the host handed a slot of its ring on — the state's words there and, behind them, one lane's
// SYSTEM-scope release store of the sequence number the host waits for.  All from one wave: the release's wait covers every lane's stores
__device__ __forceinline__ void finish_publish(int l, bool stepped, const IcpFinishLds& F, IcpState* st_out, double* out, IcpSnapSlot* snap, unsigned long long seq)
{
    static_assert(offsetof(IcpSnapSlot, state) == 0, "a snapshot's words, and behind them its sequence number");
    if (stepped && l < 19) out[l] = F.o18[l];
    if (l < ST_WORDS) reinterpret_cast<uint32_t*>(st_out)[l] = reinterpret_cast<const uint32_t*>(&F.st)[l];
    if (!snap) return;
    if (l < ST_WORDS) reinterpret_cast<uint32_t*>(&snap->state)[l] = reinterpret_cast<const uint32_t*>(&F.st)[l];
    fin_wave_sync();
    if (l == 0) __hip_atomic_store(&snap->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace pcr
