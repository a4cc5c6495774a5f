// kabsch_wave.hpp — the Kabsch step (num::kabsch_solve, T_FIRST = false) and the pose composition T_delta * T_total of numerics.hpp, worked by a GROUP
// OF LANES instead of one thread.  One text, a template over a "lane group" G that offers only: my lane index, the value another lane
// holds (get: a lane the whole group names; pick: a lane each lane names for itself), a uniform vote, selects and the two casts.  The device instance
// (WaveLanes) is a wavefront: its value types are plain double / float / int / bool, get is v_readlane, pick is ds_bpermute.  The host instance
// (HostLanes<N>) holds N lanes in arrays and loops over them: it exists so that the bits of this form can be compared with the scalar form on a machine
// without a GPU.  The scalar form stays the oracle (numerics.hpp; the synchronous loop, desc.hip and ground.hip keep it).
//
// Every elementary operation of the scalar form is here with its operands, its operator and its place in its own dependency chain; only the lane that
// executes it changed.  Sums of three terms keep the written order (a + b) + c; / and sqrt are spelled as there.  Where the lanes are:
//   six quotients sums[c] / M                      lane c of 0..5
//   H, U = W / sv, both mul3, the (float) casts    lane 3 r + c of 0..8 holds element (r, c)
//   the Jacobi sweeps, the ordering network        lane r of 0..5 holds row r of the stacked [W; R]: a rotation is six operations and no exchange; the
//                                                  three column dots are one product each on lanes 0..2 and a fixed-order sum every lane repeats
//   sv = sqrt(col_dot)                             lane c of 0..2
//   t = qbar - R pbar                              lane r of 0..2
//   T_delta * T_total                              lane 4 r + c of 0..15
// Serial, and repeated by every lane (so a rotation needs no broadcast): alpha, beta, gamma, the convergence test — a branch, uniform over the group —,
// zeta, tn, c, s of one pair, the order of the pairs, det, and the rank repairs of svd3 (rare; on values every lane holds).
#pragma once

#include "numerics.hpp"

#pragma clang fp contract(off)

namespace pcr {
namespace num {

// ---------------------------------------------------------------------------------------------- the host instance
template <class T, int N>
struct LaneVec {
    T v[N];
    LaneVec() = default;
    LaneVec(T s) { for (int i = 0; i < N; i++) v[i] = s; }
};
#define PCR_LV_BIN(OP, RT)                                                                                                                                \
    template <class T, int N> inline LaneVec<RT, N> operator OP(const LaneVec<T, N>& a, const LaneVec<T, N>& b) { LaneVec<RT, N> r; for (int i = 0; i < N; i++) r.v[i] = a.v[i] OP b.v[i]; return r; } \
    template <class T, int N> inline LaneVec<RT, N> operator OP(const LaneVec<T, N>& a, T b) { LaneVec<RT, N> r; for (int i = 0; i < N; i++) r.v[i] = a.v[i] OP b; return r; }                     \
    template <class T, int N> inline LaneVec<RT, N> operator OP(T a, const LaneVec<T, N>& b) { LaneVec<RT, N> r; for (int i = 0; i < N; i++) r.v[i] = a OP b.v[i]; return r; }
PCR_LV_BIN(+, T) PCR_LV_BIN(-, T) PCR_LV_BIN(*, T) PCR_LV_BIN(/, T) PCR_LV_BIN(&, T)
PCR_LV_BIN(<, bool) PCR_LV_BIN(<=, bool) PCR_LV_BIN(>, bool) PCR_LV_BIN(>=, bool) PCR_LV_BIN(==, bool)
#undef PCR_LV_BIN
template <class T, int N> inline LaneVec<T, N> operator-(const LaneVec<T, N>& a) { LaneVec<T, N> r; for (int i = 0; i < N; i++) r.v[i] = -a.v[i]; return r; }
using ::sqrt;            // (beside the overload below, so that sqrt(x) in the step is numerics.hpp's sqrt for a double)
template <int N> inline LaneVec<double, N> sqrt(const LaneVec<double, N>& a) { LaneVec<double, N> r; for (int i = 0; i < N; i++) r.v[i] = ::sqrt(a.v[i]); return r; }

template <int N>
struct HostLanes {
    using D = LaneVec<double, N>; using F = LaneVec<float, N>; using I = LaneVec<int, N>; using B = LaneVec<bool, N>;
    I lane() const { I r; for (int i = 0; i < N; i++) r.v[i] = i; return r; }
    template <class T> LaneVec<T, N> get(const LaneVec<T, N>& v, int k) const { return LaneVec<T, N>(v.v[k]); }
    template <class T> LaneVec<T, N> pick(const LaneVec<T, N>& v, const I& k) const { LaneVec<T, N> r; for (int i = 0; i < N; i++) r.v[i] = v.v[k.v[i] % N]; return r; }
    mutable bool split = false;                                       // a vote the lanes did not agree on: the algorithm votes only on values every lane holds alike,
    bool uniform(const B& b) const                                    // (the device instance reads lane 0's and relies on that), so the host instance checks it
    {
        for (int i = 1; i < N; i++) if (b.v[i] != b.v[0]) split = true;
        return b.v[0];
    }
    template <class T> LaneVec<T, N> sel(const B& c, const LaneVec<T, N>& a, const LaneVec<T, N>& b) const { LaneVec<T, N> r; for (int i = 0; i < N; i++) r.v[i] = c.v[i] ? a.v[i] : b.v[i]; return r; }
    F to_f32(const D& a) const { F r; for (int i = 0; i < N; i++) r.v[i] = (float)a.v[i]; return r; }
    D to_f64(const F& a) const { D r; for (int i = 0; i < N; i++) r.v[i] = (double)a.v[i]; return r; }
    D ld(const double* p, const I& k) const { D r; for (int i = 0; i < N; i++) r.v[i] = p[k.v[i]]; return r; }
};

// ---------------------------------------------------------------------------------------------- the device instance: one wavefront, every lane active
#if defined(__HIPCC__)
struct WaveLanes {
    using D = double; using F = float; using I = int; using B = bool;
    int l;
    __device__ __forceinline__ I lane() const { return l; }
    __device__ __forceinline__ D get(D v, int k) const
    {
        const long long b = __double_as_longlong(v);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b & 0xFFFFFFFFll), k), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), k);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    __device__ __forceinline__ D pick(D v, I k) const
    {
        const long long b = __double_as_longlong(v);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(k << 2, (int)(uint32_t)(b & 0xFFFFFFFFll)), hi = (uint32_t)__builtin_amdgcn_ds_bpermute(k << 2, (int)(uint32_t)((unsigned long long)b >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    __device__ __forceinline__ F pick(F v, I k) const { return __int_as_float(__builtin_amdgcn_ds_bpermute(k << 2, __float_as_int(v))); }
    __device__ __forceinline__ bool uniform(B b) const { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
    __device__ __forceinline__ D sel(B c, D a, D b) const { return c ? a : b; }
    __device__ __forceinline__ F sel(B c, F a, F b) const { return c ? a : b; }
    __device__ __forceinline__ I sel(B c, I a, I b) const { return c ? a : b; }
    __device__ __forceinline__ F to_f32(D a) const { return (float)a; }
    __device__ __forceinline__ D to_f64(F a) const { return (double)a; }
    __device__ __forceinline__ D ld(const double* p, I k) const { return p[k]; }
};
#endif

// ---------------------------------------------------------------------------------------------- the step
template <class G>
PCR_HD typename G::D lanes_abs(const G& g, const typename G::D& v) { return g.sel(v < 0.0, -v, v); }                  // dabs

// the sum over the rows of W — lanes 0, 1, 2 — of a per-row product, in col_dot's order; every lane ends up with it
template <class G>
PCR_HD typename G::D rows_sum3(const G& g, const typename G::D& p) { return (g.get(p, 0) + g.get(p, 1)) + g.get(p, 2); }

// jacobi_pair<P, Q>: x = my row of [W; R]
template <int P, int Q, class G>
PCR_HD bool jacobi_pair_lanes(const G& g, typename G::D (&x)[3])
{
    using D = typename G::D;
    const double eps = 2.220446049250313e-16;   // DBL_EPSILON
    const D alpha = rows_sum3(g, x[P] * x[P]), beta = rows_sum3(g, x[Q] * x[Q]), gamma = rows_sum3(g, x[P] * x[Q]);
    if (g.uniform(gamma == 0.0)) return false;
    if (g.uniform(lanes_abs(g, gamma) <= eps * sqrt(alpha * beta))) return false;
    const D zeta = (beta - alpha) / (2.0 * gamma);
    const D tn = g.sel(zeta >= 0.0, D(1.0), D(-1.0)) / (lanes_abs(g, zeta) + sqrt(1.0 + zeta * zeta));
    const D c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
    const D mp = x[P], mq = x[Q];
    x[P] = c * mp - s * mq;
    x[Q] = s * mp + c * mq;
    return true;
}

// order_cols<A, B> on my row
template <int A, int B, class G>
PCR_HD void order_cols_lanes(const G& g, typename G::D (&sv)[3], typename G::D (&x)[3])
{
    using D = typename G::D;
    const typename G::B sw = sv[B] > sv[A];
    const D sa = sv[A], sb = sv[B], xa = x[A], xb = x[B];
    sv[A] = g.sel(sw, sb, sa); sv[B] = g.sel(sw, sa, sb);
    x[A] = g.sel(sw, xb, xa); x[B] = g.sel(sw, xa, xb);
}

// the rank repairs of svd3 on a U every lane holds whole (values alike in every lane; have[] as svd3 computed them)
template <class G>
PCR_HD void svd3_repair_lanes(const G& g, typename G::D (&U)[9], const bool (&have)[3])
{
    using D = typename G::D; using I = typename G::I; using B = typename G::B;
    if (!have[0]) {   // A == 0
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) U[3 * r + c] = D(r == c ? 1.0 : 0.0);
        return;
    }
    if (!have[1]) {   // rank 1: any unit vector orthogonal to u0
        const D u0[3] = { U[0], U[3], U[6] };
        I k = I(0);
        D uk = u0[0];
        const B b1 = lanes_abs(g, u0[1]) < lanes_abs(g, uk);
        k = g.sel(b1, I(1), k); uk = g.sel(b1, u0[1], uk);
        const B b2 = lanes_abs(g, u0[2]) < lanes_abs(g, uk);
        k = g.sel(b2, I(2), k); uk = g.sel(b2, u0[2], uk);
        D v[3] = { -uk * u0[0], -uk * u0[1], -uk * u0[2] };
        for (int i = 0; i < 3; i++) v[i] = g.sel(k == i, v[i] + 1.0, v[i]);
        const D nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        U[1] = v[0] / nv; U[4] = v[1] / nv; U[7] = v[2] / nv;
    }
    if (!have[2]) {   // u2 = u0 x u1
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

// of three values every lane holds, the one my index names
template <class G, class T>
PCR_HD T lanes_of3(const G& g, const typename G::I& k, const T& a0, const T& a1, const T& a2) { return g.sel(k == 0, a0, g.sel(k == 1, a1, a2)); }

// num::kabsch_solve by a lane group: R[3 r + c] comes out in lane 3 r + c (0..8), t[r] in lane r (0..2); what the other lanes hold means nothing.
// Returns what the scalar form returns, alike in every lane.  sums: 16 doubles every lane may read
template <class G>
PCR_HD int kabsch_solve_lanes(const G& g, const double* sums, typename G::F& R_out, typename G::F& t_out)
{
    using D = typename G::D; using F = typename G::F; using I = typename G::I;
    const double eps = 2.220446049250313e-16;   // DBL_EPSILON
    const I l = g.lane();
    const D M = g.ld(sums, I(15));
    if (!g.uniform(M > 0.0)) return -1;
    // pbar, qbar: one division on six lanes; then every lane holds the six
    const D mean = g.ld(sums, g.sel(l < 6, l, I(5))) / M;
    const D pbar[3] = { g.get(mean, 0), g.get(mean, 1), g.get(mean, 2) }, qbar[3] = { g.get(mean, 3), g.get(mean, 4), g.get(mean, 5) };
    // H: element (r, c) on lane i9 = 3 r + c
    const I i9 = g.sel(l < 9, l, I(8)), r9 = i9 / 3, c9 = i9 - 3 * r9;
    const D h = g.ld(sums, 6 + i9) - M * lanes_of3(g, r9, qbar[0], qbar[1], qbar[2]) * lanes_of3(g, c9, pbar[0], pbar[1], pbar[2]);
    // my row of the stacked [W; R]: W = H on lanes 0..2, R = I on lanes 3..5 (the lanes behind them carry zeros along)
    const I rw = g.sel(l < 3, l, I(0)), rr = l - 3;
    D x[3];
    for (int c = 0; c < 3; c++) x[c] = g.sel(l < 3, g.pick(h, 3 * rw + c), g.sel(rr == c, D(1.0), D(0.0)));
    for (int sweep = 0; sweep < 60; sweep++) {
        const bool r01 = jacobi_pair_lanes<0, 1>(g, x);
        const bool r02 = jacobi_pair_lanes<0, 2>(g, x);
        const bool r12 = jacobi_pair_lanes<1, 2>(g, x);
        if (!(r01 || r02 || r12)) break;
    }
    // sv: the three dots on every lane, one square root on three lanes
    const D d0 = rows_sum3(g, x[0] * x[0]), d1 = rows_sum3(g, x[1] * x[1]), d2 = rows_sum3(g, x[2] * x[2]);
    const D root = sqrt(lanes_of3(g, l, d0, d1, d2));
    D sv[3] = { g.get(root, 0), g.get(root, 1), g.get(root, 2) };
    order_cols_lanes<0, 1>(g, sv, x);          // the exchange network (0,1) (0,2) (1,2) on '>' — ties keep their column order
    order_cols_lanes<0, 2>(g, sv, x);
    order_cols_lanes<1, 2>(g, sv, x);
    const D smax = sv[0];
    bool have[3];
    for (int c = 0; c < 3; c++) have[c] = g.uniform((sv[c] > 0.0) & (sv[c] > smax * eps * 8.0));
    // U: element (r, c) = W[r][c] / sv[c] on lane i9, one division
    const D w9 = lanes_of3(g, c9, g.pick(x[0], r9), g.pick(x[1], r9), g.pick(x[2], r9)), sv9 = lanes_of3(g, c9, sv[0], sv[1], sv[2]);
    D u9 = g.sel((sv9 > 0.0) & (sv9 > smax * eps * 8.0), w9 / sv9, D(0.0));
    if (!(have[0] && have[1] && have[2])) {
        D U[9];
        for (int k = 0; k < 9; k++) U[k] = g.get(u9, k);
        svd3_repair_lanes(g, U, have);
        u9 = U[8];
        for (int k = 7; k >= 0; k--) u9 = g.sel(i9 == k, U[k], u9);
    }
    // Rd = U V^T: row r of U, row c of V (= row 3 + c of the stack)
    D rd9;
    {
        const D u0 = g.pick(u9, 3 * r9), u1 = g.pick(u9, 3 * r9 + 1), u2 = g.pick(u9, 3 * r9 + 2);
        const D v0 = g.pick(x[0], 3 + c9), v1 = g.pick(x[1], 3 + c9), v2 = g.pick(x[2], 3 + c9);
        rd9 = u0 * v0 + u1 * v1 + u2 * v2;
    }
    D Rd[9];
    for (int k = 0; k < 9; k++) Rd[k] = g.get(rd9, k);
    const D det = Rd[0] * (Rd[4] * Rd[8] - Rd[5] * Rd[7]) - Rd[1] * (Rd[3] * Rd[8] - Rd[5] * Rd[6])
                + Rd[2] * (Rd[3] * Rd[7] - Rd[4] * Rd[6]);
    if (g.uniform(det < 0.0)) {   // V * B * U^T: row r of V with its last entry times det, row c of U
        const D v0 = g.pick(x[0], 3 + r9), v1 = g.pick(x[1], 3 + r9), v2 = g.pick(x[2], 3 + r9) * det;
        const D u0 = g.pick(u9, 3 * c9), u1 = g.pick(u9, 3 * c9 + 1), u2 = g.pick(u9, 3 * c9 + 2);
        rd9 = v0 * u0 + v1 * u1 + v2 * u2;
    }
    const F Rf = g.to_f32(rd9);
    // t: row r of R on lane r
    const I r3 = g.sel(l < 3, l, I(2));
    const D Rp = (g.to_f64(g.pick(Rf, 3 * r3)) * pbar[0] + g.to_f64(g.pick(Rf, 3 * r3 + 1)) * pbar[1]) + g.to_f64(g.pick(Rf, 3 * r3 + 2)) * pbar[2];
    R_out = Rf;
    t_out = g.to_f32(lanes_of3(g, r3, qbar[0], qbar[1], qbar[2]) - Rp);
    return 0;
}

// T_delta * T_total (num::mat4_mul_f32 with T_delta = [R t; 0 0 0 1]): R, t as kabsch_solve_lanes leaves them, T_total[k] in lane k (0..15); the
// product's element k comes out in lane k
template <class G>
PCR_HD typename G::F pose_compose_lanes(const G& g, const typename G::F& R, const typename G::F& t, const typename G::F& T_total)
{
    using F = typename G::F; using I = typename G::I; using B = typename G::B;
    const I l = g.lane();
    const I i16 = g.sel(l < 16, l, I(15)), r4 = i16 / 4, c4 = i16 - 4 * r4;
    const B top = r4 < 3;                      // the rows of [R t]; the last one is 0 0 0 1
    const I rr = g.sel(top, r4, I(0));
    const F a0 = g.sel(top, g.pick(R, 3 * rr), F(0.0f)), a1 = g.sel(top, g.pick(R, 3 * rr + 1), F(0.0f)), a2 = g.sel(top, g.pick(R, 3 * rr + 2), F(0.0f)),
            a3 = g.sel(top, g.pick(t, rr), F(1.0f));
    F acc = a0 * g.pick(T_total, c4);
    acc = acc + a1 * g.pick(T_total, 4 + c4);
    acc = acc + a2 * g.pick(T_total, 8 + c4);
    acc = acc + a3 * g.pick(T_total, 12 + c4);
    return acc;
}

// the host instance, whole: what pcr_kabsch_solve_lanes runs (-2: a vote was not uniform)
inline int kabsch_solve_host_lanes(const double sums[16], float R[9], float t[3])
{
    using G = HostLanes<16>;
    const G g;
    G::F Rl(0.0f), tl(0.0f);
    const int rc = kabsch_solve_lanes(g, sums, Rl, tl);
    if (g.split) return -2;
    if (rc != 0) return rc;
    for (int k = 0; k < 9; k++) R[k] = Rl.v[k];
    for (int k = 0; k < 3; k++) t[k] = tl.v[k];
    return 0;
}

}  // namespace num
}  // namespace pcr
