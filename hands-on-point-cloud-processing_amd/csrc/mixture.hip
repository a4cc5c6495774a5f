// mixture.hip — Homework3's clustering chapter: K-Means (Homework3/hw3/sript/KMeans.py, spectralClustering.cpp:337-427), the
// k-means++-style seeding both classes share (init_choice) and Gaussian-mixture EM (Homework3/nano_vs_my/sript/GMM.py) over row-major
// f64 data resident in HBM (pcr_mat64).  The contracts are written out in include/pcr.h; DESIGN §8k records the launch shapes.
//
//   K-Means pass   km_assign (labels + per-cluster limb sums, one launch) -> km_finish (centres, convergence test, status record)
//   seeding        seed_min (running minimum + limb sum of d) -> seed_weight -> rocPRIM inclusive scan -> seed_pick (search for u)
//   EM pass        em_prep (Cholesky per component) -> em_resp (responsibilities) -> em_moments<first> -> em_finish1 (N_k, pi, mean)
//                  -> em_moments<second> (around the NEW mean) -> em_finish2 (covariance, reset rule, convergence test)
//
// Every sum over points is ORDER-FREE: a term is cut into three signed 32-bit limbs on one fixed-point grid per call (unit 2^(e-96),
// 2^e bounding the term), limbs are added as 64-bit integers (fewer than 2^31 terms: no overflow), and the 128-bit total is rounded to
// f64 ONCE.  The kernel boundary is the only hand-off between workgroups; every loop is bounded by n, k or max_iter.
#include "pcr_internal.hpp"

#include <rocprim/device/device_scan.hpp>

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int MX_BLOCK = 256;
constexpr int MX_KMAX = 64, MX_DMAX = 8;
constexpr int MX_ACC1 = MX_KMAX * (1 + MX_DMAX) * 3;                    // K-Means rows (3 dim + 1 <= 25 words) and the first EM moments (27 words)
constexpr int MX_ACC2 = MX_KMAX * (MX_DMAX * (MX_DMAX + 1) / 2) * 3;    // second EM moments
constexpr int MX_ACCS = 4;                                              // seeding: limb sum of the running minimum
constexpr int MX_ACC_WORDS = MX_ACC1 + MX_ACC2 + MX_ACCS;
constexpr int MX_EM_P = 4;                                              // points per lane of a moments tile
constexpr int MX_EMAX = 400;                                            // |e| of the data grid the arithmetic is laid out for

enum { MX_STEP = 0, MX_FIT_PY = 1, MX_FIT_CPP = 2 };

// the small record the host reads back per batch of iterations
struct MxRec {
    int iters, converged, stop, status, resets, pad_[3];
};

struct MxState {
    MxRec rec;
    int k, dim, mode, max_iter, unit_e, pad_[3];
    unsigned long long seed, n;
    double tol, amplitude;
    double centres[MX_KMAX * MX_DMAX];      // K-Means centres / mixture means of the current iteration
    double cnew[MX_KMAX * MX_DMAX];         // ... of the pass just finished
    double cov[MX_KMAX * MX_DMAX * MX_DMAX], cov_new[MX_KMAX * MX_DMAX * MX_DMAX];
    double pi[MX_KMAX], pi_new[MX_KMAX], nk[MX_KMAX];
    double linv[MX_KMAX * MX_DMAX * MX_DMAX], logc[MX_KMAX];
    long long counts[MX_KMAX];
};

__host__ __device__ inline unsigned long long mx_key(unsigned long long seed, unsigned long long a)
{
    unsigned long long zz = seed ^ (0x9E3779B97F4A7C15ull * (a + 1ull));
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    return zz ^ (zz >> 31);
}

// v 2^sh (|.| < 2^96 by the caller's choice of grid) cut towards zero into three signed 32-bit limbs
__device__ __forceinline__ void mx_limbs(double v, int sh, long long& l0, long long& l1, long long& l2)
{
    double a = ldexp(fabs(v), sh);                                       // a power-of-two scaling: exact
    a = a < 7.9228162514264329e28 ? a : 7.9228162514264329e28;           // 2^96 - 2^43 (never reached inside the contract; NaN -> the bound)
    const unsigned long long hi = (unsigned long long)(a * 2.3283064365386963e-10);        // trunc(a 2^-32) < 2^64
    const unsigned long long lo = (unsigned long long)(a - (double)hi * 4294967296.0);     // exact: the low bits of a's mantissa
    long long m0 = (long long)lo, m1 = (long long)(hi & 0xffffffffull), m2 = (long long)(hi >> 32);
    if (v < 0) { m0 = -m0; m1 = -m1; m2 = -m2; }
    l0 = m0; l1 = m1; l2 = m2;
}

// (s0 + s1 2^32 + s2 2^64) 2^unit_exp, rounded to f64 once (round to nearest even: a sticky bit under the top 64 bits)
__device__ inline double mx_value(long long s0, long long s1, long long s2, int unit_exp)
{
    const __int128 t = (__int128)s0 + (__int128)s1 * 4294967296ll + ((__int128)s2 * 4294967296ll) * 4294967296ll;
    const bool neg = t < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)(-t) : (unsigned __int128)t;
    const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
    double r;
    int ex = 0;
    if (hi == 0) {
        r = (double)lo;
    } else {
        const int sh = 64 - __clzll((long long)hi);                      // 1 .. 64
        unsigned long long top = sh == 64 ? hi : ((hi << (64 - sh)) | (lo >> sh));
        const unsigned long long rest = sh == 64 ? lo : (lo << (64 - sh));
        top |= rest != 0 ? 1ull : 0ull;
        r = (double)top;
        ex = sh;
    }
    r = ldexp(r, ex + unit_exp);
    return neg ? -r : r;
}

__device__ __forceinline__ long long mx_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void mx_lds_add(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// ---- K-Means ------------------------------------------------------------------------------------------------------------------
// s = sum_d (x_d - c_d)^2 in ascending d, f64, unfused; the minimum with the lowest centre index
template <int DIM>
__device__ __forceinline__ int km_nearest(const double* xi, const double* c, int k)
{
    int best = 0;
    double bs = 0.0;
    for (int j = 0; j < k; j++) {
        double t = xi[0] - c[j * DIM];
        double s = t * t;
#pragma unroll
        for (int d = 1; d < DIM; d++) { t = xi[d] - c[j * DIM + d]; s = s + t * t; }
        if (j == 0 || s < bs || (bs != bs && s == s)) { bs = s; best = j; }
    }
    return best;
}

// LDS: [k DIM centres][copies x k x (3 DIM + 1) limb words]; wave w adds into copy w % copies
template <int DIM>
__global__ __launch_bounds__(MX_BLOCK) void km_assign_kernel(const double* __restrict__ x, uint32_t n, int k, const MxState* __restrict__ st,
                                                             int sh, int32_t* __restrict__ labels, long long* __restrict__ acc, int copies, int accumulate)
{
    extern __shared__ long long mx_lds[];
    if (st->rec.stop) return;
    constexpr int W = 3 * DIM + 1;
    double* c = (double*)mx_lds;
    long long* bins = mx_lds + k * DIM;
    for (int t = threadIdx.x; t < k * DIM; t += blockDim.x) c[t] = st->centres[t];
    const int nb = accumulate ? copies * k * W : 0;
    for (int t = threadIdx.x; t < nb; t += blockDim.x) bins[t] = 0;
    __syncthreads();
    long long* mine = bins + ((threadIdx.x >> 6) % copies) * k * W;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double xi[DIM];
#pragma unroll
        for (int d = 0; d < DIM; d++) xi[d] = x[(size_t)i * DIM + d];
        const int best = km_nearest<DIM>(xi, c, k);
        labels[i] = best;
        if (accumulate) {
            long long* row = mine + best * W;
#pragma unroll
            for (int d = 0; d < DIM; d++) {
                long long l0, l1, l2;
                mx_limbs(xi[d], sh, l0, l1, l2);
                mx_lds_add(row + 3 * d, l0); mx_lds_add(row + 3 * d + 1, l1); mx_lds_add(row + 3 * d + 2, l2);
            }
            mx_lds_add(row + 3 * DIM, 1);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nb; t += blockDim.x) {
        const long long v = bins[t];
        if (v != 0) atomicAdd((unsigned long long*)&acc[t % (k * W)], (unsigned long long)v);
    }
}

// one workgroup: limb rows -> centres, the convergence test of the mode, the status record; clears the rows for the next pass
__global__ __launch_bounds__(MX_BLOCK) void km_finish_kernel(long long* __restrict__ acc, MxState* __restrict__ st)
{
    __shared__ int not_conv, empty;
    if (st->rec.stop) return;
    const int k = st->k, dim = st->dim, W = 3 * dim + 1, mode = st->mode;
    if (threadIdx.x == 0) { not_conv = 0; empty = 0; }
    __syncthreads();
    for (int t = threadIdx.x; t < k * dim; t += blockDim.x) {
        const int j = t / dim, d = t % dim;
        const long long* row = acc + j * W;
        const long long cnt = row[3 * dim];
        const double v = mx_value(row[3 * d], row[3 * d + 1], row[3 * d + 2], st->unit_e) / (double)cnt;     // 0 / 0 = NaN: np.mean of an empty slice
        const double diff = v - st->centres[t];
        const bool ok = mode == MX_FIT_CPP ? fabs(diff) < st->tol : diff < st->tol;                        // KMeans.py:66 is signed, as written
        if (!ok) not_conv = 1;
        if (cnt == 0) empty = 1;
        st->cnew[t] = v;
        if (d == 0) st->counts[j] = cnt;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < k * W; t += blockDim.x) acc[t] = 0;
    for (int t = threadIdx.x; t < k * dim; t += blockDim.x) st->centres[t] = st->cnew[t];
    if (threadIdx.x == 0) {
        const int iters = ++st->rec.iters;
        if (empty) { st->rec.status = PCR_EMPTY_CLUSTER; st->rec.stop = 1; }
        else if (mode == MX_STEP) st->rec.stop = 1;
        else if (mode == MX_FIT_PY) {
            if (!not_conv) { st->rec.converged = 1; st->rec.stop = 1; }
            else if (iters > st->max_iter) st->rec.stop = 1;
        } else {
            if (!not_conv && iters < st->max_iter) { st->rec.converged = 1; st->rec.stop = 1; }
            else if (iters > st->max_iter) st->rec.stop = 1;
        }
    }
}

// ---- seeding ------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(MX_BLOCK) void seed_min_kernel(const double* __restrict__ x, uint32_t n, const int32_t* __restrict__ chosen, int j,
                                                            double* __restrict__ dmin, int sh, long long* __restrict__ accs)
{
    const size_t ci = (size_t)chosen[j - 1];
    double c[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) c[d] = x[ci * DIM + d];
    long long a0 = 0, a1 = 0, a2 = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double t = x[(size_t)i * DIM] - c[0];
        double s = t * t;
#pragma unroll
        for (int d = 1; d < DIM; d++) { t = x[(size_t)i * DIM + d] - c[d]; s = s + t * t; }
        double dd = sqrt(s);
        if (j > 1) { const double o = dmin[i]; dd = o < dd ? o : dd; }
        dmin[i] = dd;
        long long l0, l1, l2;
        mx_limbs(dd, sh, l0, l1, l2);
        a0 += l0; a1 += l1; a2 += l2;
    }
    a0 = mx_wave_sum(a0); a1 = mx_wave_sum(a1); a2 = mx_wave_sum(a2);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd((unsigned long long*)&accs[0], (unsigned long long)a0);
        atomicAdd((unsigned long long*)&accs[1], (unsigned long long)a1);
        atomicAdd((unsigned long long*)&accs[2], (unsigned long long)a2);
    }
}

// w_i = 0 where d_i < factor mean_d, else exp(d_i); flag[0] = 1 when an exp overflowed
__global__ __launch_bounds__(MX_BLOCK) void seed_weight_kernel(const double* __restrict__ dmin, uint32_t n, const long long* __restrict__ accs, int unit_e,
                                                               double factor, double* __restrict__ w, int* __restrict__ flag)
{
    const double mean = mx_value(accs[0], accs[1], accs[2], unit_e) / (double)n;
    const double thr = factor * mean;
    bool over = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double d = dmin[i];
        const double v = d < thr ? 0.0 : exp(d);
        over = over || !(v <= DBL_MAX);
        w[i] = v;
    }
    if (over) flag[0] = 1;
}

// chosen[j] = searchsorted(cdf / cdf[n - 1], u, side = 'right'); one lane, at most 32 probes.  flag[1] = 1 when the weights do not sum to a
// positive finite number.  Clears the limb sum for the next pick.
__global__ void seed_pick_kernel(const double* __restrict__ cdf, uint32_t n, double u, int32_t* __restrict__ chosen, int j, long long* __restrict__ accs,
                                 int* __restrict__ flag)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    accs[0] = 0; accs[1] = 0; accs[2] = 0;
    const double total = cdf[n - 1];
    if (!(total > 0.0) || !(total <= DBL_MAX)) { flag[1] = 1; chosen[j] = 0; return; }
    uint32_t lo = 0, hi = n;                   // first i with cdf[i] / total > u
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cdf[mid] / total > u) hi = mid; else lo = mid + 1;
    }
    chosen[j] = (int32_t)(lo < n ? lo : n - 1);
}

__global__ __launch_bounds__(MX_BLOCK) void seed_prob_kernel(const double* __restrict__ w, const double* __restrict__ cdf, uint32_t n, double* __restrict__ p)
{
    const double total = cdf[n - 1];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = w[i] / total;
}

// ---- Gaussian mixture -----------------------------------------------------------------------------------------------------------
// one lane per component: Sigma = L L^T, L^-1, logc = log pi - (dim log 2 pi + log det Sigma) / 2.  Not positive definite: PCR_ERR_STATE.
__global__ void em_prep_kernel(MxState* __restrict__ st)
{
    const int k = st->k, dim = st->dim, j = threadIdx.x;
    if (st->rec.stop || j >= k) return;
    double L[MX_DMAX][MX_DMAX], Li[MX_DMAX][MX_DMAX];
    const double* S = st->cov + j * dim * dim;
    bool bad = false;
    double logdet = 0.0;
    for (int a = 0; a < dim; a++) {
        for (int b = 0; b <= a; b++) {
            double s = S[a * dim + b];
            for (int t = 0; t < b; t++) s = s - L[a][t] * L[b][t];
            if (a == b) {
                if (!(s > 0.0) || !(s <= DBL_MAX)) { bad = true; s = 1.0; }
                L[a][a] = sqrt(s);
                logdet = logdet + 2.0 * log(L[a][a]);
            } else {
                L[a][b] = s / L[b][b];
            }
        }
    }
    for (int c = 0; c < dim; c++)
        for (int a = 0; a < dim; a++) {
            if (a < c) { Li[a][c] = 0.0; continue; }
            double s = a == c ? 1.0 : 0.0;
            for (int t = c; t < a; t++) s = s - L[a][t] * Li[t][c];
            Li[a][c] = s / L[a][a];
        }
    for (int a = 0; a < dim; a++)
        for (int b = 0; b < dim; b++) st->linv[(j * dim + a) * dim + b] = Li[a][b];
    st->logc[j] = log(st->pi[j]) - 0.5 * ((double)dim * 1.8378770664093453 + logdet);
    if (bad) { st->rec.status = PCR_ERR_STATE; }
}

__global__ void em_prep_check_kernel(MxState* __restrict__ st)
{
    if (threadIdx.x == 0 && st->rec.status == PCR_ERR_STATE) st->rec.stop = 1;
}

// log pi_k N(x; mu_k, Sigma_k) = logc_k - |L_k^-1 (x - mu_k)|^2 / 2
template <int DIM>
__device__ __forceinline__ double em_logp(const double* xi, const double* mu, const double* li, double logc)
{
    double df[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) df[d] = xi[d] - mu[d];
    double m = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; a++) {
        double y = li[a * DIM] * df[0];
#pragma unroll
        for (int b = 1; b <= a; b++) y = y + li[a * DIM + b] * df[b];
        m = m + y * y;
    }
    return logc - 0.5 * m;
}

// post[j n + i] = gamma_ij (log-sum-exp over j), or labels[i] = the first maximum of the log posterior (PREDICT).
// LDS: [k DIM means][k DIM DIM inverse factors][k logc]
template <int DIM, bool PREDICT>
__global__ __launch_bounds__(MX_BLOCK) void em_resp_kernel(const double* __restrict__ x, uint32_t n, int k, const MxState* __restrict__ st,
                                                           double* __restrict__ post, int32_t* __restrict__ labels)
{
    extern __shared__ long long mx_lds[];
    if (st->rec.stop) return;
    double* mu = (double*)mx_lds;
    double* li = mu + k * DIM;
    double* lc = li + k * DIM * DIM;
    for (int t = threadIdx.x; t < k * DIM; t += blockDim.x) mu[t] = st->centres[t];
    for (int t = threadIdx.x; t < k * DIM * DIM; t += blockDim.x) li[t] = st->linv[t];
    for (int t = threadIdx.x; t < k; t += blockDim.x) lc[t] = st->logc[t];
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double xi[DIM];
#pragma unroll
        for (int d = 0; d < DIM; d++) xi[d] = x[(size_t)i * DIM + d];
        double m = 0.0;
        int best = 0;
        for (int j = 0; j < k; j++) {
            const double lp = em_logp<DIM>(xi, mu + j * DIM, li + j * DIM * DIM, lc[j]);
            if (!PREDICT) post[(size_t)j * n + i] = lp;
            if (j == 0 || lp > m) { m = lp; best = j; }
        }
        if (PREDICT) { labels[i] = best; continue; }
        double s = 0.0;
        for (int j = 0; j < k; j++) {
            const double ev = exp(post[(size_t)j * n + i] - m);
            post[(size_t)j * n + i] = ev;
            s = s + ev;
        }
        for (int j = 0; j < k; j++) post[(size_t)j * n + i] = post[(size_t)j * n + i] / s;
    }
}

// FIRST moments: per component N = sum gamma (grid 2^-95) and sum gamma x (the data's grid); SECOND: sum (gamma (x - mu)_a) (x - mu)_b, a <= b,
// around the NEW mean (grid 2^(2e + 2 - 96)).  A lane keeps MX_EM_P points in registers and walks the components: its terms are added as
// integers in registers, then across the wave, and lane 0 adds the wave's words to the workgroup's rows in LDS; one flush per workgroup.
template <int DIM, bool SECOND>
__global__ __launch_bounds__(MX_BLOCK) void em_moments_kernel(const double* __restrict__ x, uint32_t n, int k, const MxState* __restrict__ st,
                                                              const double* __restrict__ post, int sh_x, int sh_xx, long long* __restrict__ acc)
{
    extern __shared__ long long mx_lds[];
    if (st->rec.stop) return;
    constexpr int T = SECOND ? DIM * (DIM + 1) / 2 : 1 + DIM;
    long long* bins = mx_lds;
    double* mu = (double*)(mx_lds + k * T * 3);
    for (int t = threadIdx.x; t < k * T * 3; t += blockDim.x) bins[t] = 0;
    if (SECOND) for (int t = threadIdx.x; t < k * DIM; t += blockDim.x) mu[t] = st->cnew[t];
    __syncthreads();
    const uint32_t tile = blockDim.x * MX_EM_P;
    const uint32_t tiles = (n + tile - 1) / tile;
    for (uint32_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        double xp[MX_EM_P][DIM];
        uint32_t ip[MX_EM_P];
#pragma unroll
        for (int p = 0; p < MX_EM_P; p++) {
            ip[p] = tl * tile + p * blockDim.x + threadIdx.x;
#pragma unroll
            for (int d = 0; d < DIM; d++) xp[p][d] = ip[p] < n ? x[(size_t)ip[p] * DIM + d] : 0.0;
        }
        for (int j = 0; j < k; j++) {
            double g[MX_EM_P];
#pragma unroll
            for (int p = 0; p < MX_EM_P; p++) g[p] = ip[p] < n ? post[(size_t)j * n + ip[p]] : 0.0;
            if (!SECOND) {
                long long a[T][3];
#pragma unroll
                for (int t = 0; t < T; t++) { a[t][0] = 0; a[t][1] = 0; a[t][2] = 0; }
#pragma unroll
                for (int p = 0; p < MX_EM_P; p++) {
                    long long l0, l1, l2;
                    mx_limbs(g[p], 95, l0, l1, l2);
                    a[0][0] += l0; a[0][1] += l1; a[0][2] += l2;
#pragma unroll
                    for (int d = 0; d < DIM; d++) {
                        mx_limbs(g[p] * xp[p][d], sh_x, l0, l1, l2);
                        a[1 + d][0] += l0; a[1 + d][1] += l1; a[1 + d][2] += l2;
                    }
                }
#pragma unroll
                for (int t = 0; t < T; t++)
#pragma unroll
                    for (int l = 0; l < 3; l++) {
                        const long long v = mx_wave_sum(a[t][l]);
                        if ((threadIdx.x & 63) == 0 && v != 0) mx_lds_add(bins + (j * T + t) * 3 + l, v);
                    }
            } else {
                int base = 0;
#pragma unroll
                for (int r = 0; r < DIM; r++) {
                    long long a[DIM][3];
#pragma unroll
                    for (int t = 0; t < DIM; t++) { a[t][0] = 0; a[t][1] = 0; a[t][2] = 0; }
#pragma unroll
                    for (int p = 0; p < MX_EM_P; p++) {
                        const double gr = g[p] * (xp[p][r] - mu[j * DIM + r]);
#pragma unroll
                        for (int c = r; c < DIM; c++) {
                            long long l0, l1, l2;
                            mx_limbs(gr * (xp[p][c] - mu[j * DIM + c]), sh_xx, l0, l1, l2);
                            a[c][0] += l0; a[c][1] += l1; a[c][2] += l2;
                        }
                    }
#pragma unroll
                    for (int c = r; c < DIM; c++)
#pragma unroll
                        for (int l = 0; l < 3; l++) {
                            const long long v = mx_wave_sum(a[c][l]);
                            if ((threadIdx.x & 63) == 0 && v != 0) mx_lds_add(bins + (j * T + base + (c - r)) * 3 + l, v);
                        }
                    base += DIM - r;
                }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < k * T * 3; t += blockDim.x) {
        const long long v = bins[t];
        if (v != 0) atomicAdd((unsigned long long*)&acc[t], (unsigned long long)v);
    }
}

// N_k, pi_new = N_k / n, mean_new = sum gamma x / N_k
__global__ __launch_bounds__(MX_BLOCK) void em_finish1_kernel(long long* __restrict__ acc, MxState* __restrict__ st)
{
    if (st->rec.stop) return;
    const int k = st->k, dim = st->dim, T = 1 + dim;
    for (int t = threadIdx.x; t < k * T; t += blockDim.x) {
        const int j = t / T, c = t % T;
        const long long* row = acc + (j * T) * 3;
        const double nk = mx_value(row[0], row[1], row[2], -95);
        if (c == 0) { st->nk[j] = nk; st->pi_new[j] = nk / (double)st->n; }
        else st->cnew[j * dim + c - 1] = mx_value(row[3 * c], row[3 * c + 1], row[3 * c + 2], st->unit_e) / nk;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < k * T * 3; t += blockDim.x) acc[t] = 0;
}

// cov_new = sum gamma (x - mean_new)(x - mean_new)^T / N_k; in a fit: the reset rule, the three max-abs differences, the stop test, new -> current
__global__ __launch_bounds__(MX_BLOCK) void em_finish2_kernel(long long* __restrict__ acc, const double* __restrict__ x, MxState* __restrict__ st)
{
    __shared__ int not_conv;
    if (st->rec.stop) return;
    const int k = st->k, dim = st->dim, T = dim * (dim + 1) / 2, mode = st->mode;
    const int unit = 2 * (st->unit_e + 96) + 2 - 96;
    if (threadIdx.x == 0) not_conv = 0;
    for (int t = threadIdx.x; t < k * dim * dim; t += blockDim.x) {
        const int j = t / (dim * dim), a = (t / dim) % dim, b = t % dim;
        const int r = a < b ? a : b, c = a < b ? b : a;
        const long long* row = acc + (j * T + r * dim - r * (r - 1) / 2 + (c - r)) * 3;
        st->cov_new[t] = mx_value(row[0], row[1], row[2], unit) / st->nk[j];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < k * T * 3; t += blockDim.x) acc[t] = 0;
    if (mode != MX_STEP) {
        const int iters = st->rec.iters + 1;
        if (threadIdx.x < k) {                                 // GMM.py: ||Sigma_k||_F < 0.01 -> amplitude I and a keyed random data point as the mean
            const int j = threadIdx.x;
            double f = 0.0;
            for (int t = 0; t < dim * dim; t++) f = f + st->cov_new[j * dim * dim + t] * st->cov_new[j * dim * dim + t];
            if (sqrt(f) < 0.01) {
                for (int t = 0; t < dim * dim; t++) st->cov_new[j * dim * dim + t] = (t / dim == t % dim) ? st->amplitude : 0.0;
                const unsigned long long pick = mx_key(st->seed, ((unsigned long long)iters << 32) | (unsigned long long)j) % st->n;
                for (int d = 0; d < dim; d++) st->cnew[j * dim + d] = x[pick * dim + d];
                atomicAdd(&st->rec.resets, 1);
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < k * dim * dim; t += blockDim.x) if (!(fabs(st->cov_new[t] - st->cov[t]) < st->tol)) not_conv = 1;
        for (int t = threadIdx.x; t < k * dim; t += blockDim.x) if (!(fabs(st->cnew[t] - st->centres[t]) < st->tol)) not_conv = 1;
        for (int t = threadIdx.x; t < k; t += blockDim.x) if (!(fabs(st->pi_new[t] - st->pi[t]) < st->tol)) not_conv = 1;
        __syncthreads();
        for (int t = threadIdx.x; t < k * dim * dim; t += blockDim.x) st->cov[t] = st->cov_new[t];
        for (int t = threadIdx.x; t < k * dim; t += blockDim.x) st->centres[t] = st->cnew[t];
        for (int t = threadIdx.x; t < k; t += blockDim.x) st->pi[t] = st->pi_new[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int iters = ++st->rec.iters;
        if (mode == MX_STEP) st->rec.stop = 1;
        else if (!not_conv || iters == st->max_iter) { st->rec.converged = !not_conv; st->rec.stop = 1; }
    }
}

}  // namespace

}  // namespace pcr

using namespace pcr;

struct pcr_mat64 {
    size_t n = 0;
    int dim = 0;
    int e = 0;                       // 2^e bounds every |x| (strictly)
    double* x = nullptr;             // device, row-major n x dim
    int32_t* labels = nullptr;       // device, n
    double* post = nullptr;          // device, k-major k x n responsibilities (grown on demand)
    size_t post_cap = 0;
    double* seedbuf = nullptr;       // device, 3 n: running minimum | weights | cdf
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    long long* acc = nullptr;        // device, MX_ACC_WORDS limb words (zero between calls)
    int32_t* chosen = nullptr;       // device, 64 picks + 2 flags
    MxState* st_dev = nullptr;
    MxState* st_host = nullptr;      // pinned
};

namespace {

#define MX_DISPATCH_DIM(dim, CALL)                                                                            \
    switch (dim) {                                                                                            \
    case 1: { constexpr int D = 1; CALL; } break;                                                             \
    case 2: { constexpr int D = 2; CALL; } break;                                                             \
    case 3: { constexpr int D = 3; CALL; } break;                                                             \
    case 4: { constexpr int D = 4; CALL; } break;                                                             \
    case 5: { constexpr int D = 5; CALL; } break;                                                             \
    case 6: { constexpr int D = 6; CALL; } break;                                                             \
    case 7: { constexpr int D = 7; CALL; } break;                                                             \
    default: { constexpr int D = 8; CALL; } break;                                                            \
    }

struct MxGeom {
    int block, blocks, copies;
};

// tune "mixture_geometry": 0 = 256 lanes, up to two workgroups per CU, as many private limb rows per workgroup as fit 48 KB;
// 1 = 128 lanes, at most 24 workgroups, one shared row set (the results are the same bits: tests/test_hw3_clustering.py)
MxGeom mx_geom(const pcr_ctx* ctx, size_t n, int row_words, int per_lane)
{
    MxGeom g;
    const bool alt = tune_get(ctx, "mixture_geometry", 0) == 1;
    g.block = alt ? 128 : MX_BLOCK;
    const size_t want = (n + (size_t)g.block * per_lane - 1) / ((size_t)g.block * per_lane);
    const size_t cap = alt ? 24 : (size_t)2 * (size_t)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256);
    g.blocks = (int)(want < 1 ? 1 : (want > cap ? cap : want));
    int copies = alt ? 1 : (int)((48 * 1024) / ((size_t)row_words * 8));
    if (copies < 1) copies = 1;
    if (copies > g.block / 64) copies = g.block / 64;
    g.copies = copies;
    return g;
}

bool mx_shape_ok(const pcr_mat64* m, int k) { return m && m->x && k >= 1 && k <= MX_KMAX && (size_t)k <= m->n; }

bool mx_finite(const double* v, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!(std::fabs(v[i]) <= DBL_MAX)) return false;
    return true;
}

int mx_state_push(pcr_ctx* ctx, pcr_mat64* m)
{
    PCR_HIP(ctx, hipMemcpyAsync(m->st_dev, m->st_host, sizeof(MxState), hipMemcpyHostToDevice, ctx->stream));
    return PCR_OK;
}

int mx_state_pull(pcr_ctx* ctx, pcr_mat64* m, size_t bytes)
{
    PCR_HIP(ctx, hipMemcpyAsync(m->st_host, m->st_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

void mx_state_init(pcr_mat64* m, int k, int mode, int max_iter, double tol)
{
    MxState* s = m->st_host;
    memset(s, 0, sizeof(MxState));
    s->k = k; s->dim = m->dim; s->mode = mode; s->max_iter = max_iter; s->unit_e = m->e - 96; s->n = m->n; s->tol = tol;
}

int mx_launch_assign(pcr_ctx* ctx, pcr_mat64* m, int k, bool accumulate)
{
    const int W = 3 * m->dim + 1;
    const MxGeom g = mx_geom(ctx, m->n, k * W, 1);
    const size_t lds = ((size_t)k * m->dim + (accumulate ? (size_t)g.copies * k * W : 0)) * 8;
    ProfScope ps(ctx, "km_assign");
    MX_DISPATCH_DIM(m->dim, (km_assign_kernel<D><<<g.blocks, g.block, lds, ctx->stream>>>(m->x, (uint32_t)m->n, k, m->st_dev, 96 - m->e, m->labels, m->acc,
                                                                                         g.copies, accumulate ? 1 : 0)));
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

int mx_fetch_labels(pcr_ctx* ctx, pcr_mat64* m, int32_t* labels)
{
    if (!labels) return PCR_OK;
    PCR_HIP(ctx, hipMemcpyAsync(labels, m->labels, m->n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

int mx_ensure_post(pcr_ctx* ctx, pcr_mat64* m, int k)
{
    const size_t need = (size_t)k * m->n;
    if (need <= m->post_cap) return PCR_OK;
    if (m->post) { PCR_HIP(ctx, hipStreamSynchronize(ctx->stream)); PCR_HIP(ctx, hipFree(m->post)); m->post = nullptr; m->post_cap = 0; }
    if (hipMalloc(&m->post, need * sizeof(double)) != hipSuccess) return fail(ctx, PCR_ERR_NOMEM, "pcr_mat64: responsibilities");
    m->post_cap = need;
    return PCR_OK;
}

// one EM pass on the stream (the state holds the parameters)
int mx_launch_em(pcr_ctx* ctx, pcr_mat64* m, int k)
{
    const int dim = m->dim;
    const uint32_t n = (uint32_t)m->n;
    em_prep_kernel<<<1, 64, 0, ctx->stream>>>(m->st_dev);
    em_prep_check_kernel<<<1, 64, 0, ctx->stream>>>(m->st_dev);
    {
        const MxGeom g = mx_geom(ctx, m->n, 1, 1);
        const size_t lds = ((size_t)k * dim + (size_t)k * dim * dim + k) * 8;
        ProfScope ps(ctx, "em_resp");
        MX_DISPATCH_DIM(dim, (em_resp_kernel<D, false><<<g.blocks, g.block, lds, ctx->stream>>>(m->x, n, k, m->st_dev, m->post, m->labels)));
    }
    {
        const MxGeom g = mx_geom(ctx, m->n, 1, MX_EM_P);
        const size_t lds = ((size_t)k * (1 + dim) * 3 + (size_t)k * dim) * 8;
        ProfScope ps(ctx, "em_moments1");
        MX_DISPATCH_DIM(dim, (em_moments_kernel<D, false><<<g.blocks, g.block, lds, ctx->stream>>>(m->x, n, k, m->st_dev, m->post, 96 - m->e, 0, m->acc)));
    }
    em_finish1_kernel<<<1, MX_BLOCK, 0, ctx->stream>>>(m->acc, m->st_dev);
    {
        const MxGeom g = mx_geom(ctx, m->n, 1, MX_EM_P);
        const size_t lds = ((size_t)k * (dim * (dim + 1) / 2) * 3 + (size_t)k * dim) * 8;
        ProfScope ps(ctx, "em_moments2");
        MX_DISPATCH_DIM(dim, (em_moments_kernel<D, true><<<g.blocks, g.block, lds, ctx->stream>>>(m->x, n, k, m->st_dev, m->post, 0, 96 - (2 * m->e + 2),
                                                                                                 m->acc + MX_ACC1)));
    }
    em_finish2_kernel<<<1, MX_BLOCK, 0, ctx->stream>>>(m->acc + MX_ACC1, m->x, m->st_dev);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

bool mx_params_ok(const pcr_mat64* m, int k, const double* mean, const double* cov, const double* pi)
{
    const int dim = m->dim;
    return mean && cov && pi && mx_finite(mean, (size_t)k * dim) && mx_finite(cov, (size_t)k * dim * dim) && mx_finite(pi, k);
}

}  // namespace

extern "C" int pcr_mat64_create(pcr_ctx* ctx, const double* rows, size_t n, int dim, pcr_mat64** out)
{
    if (!ctx || !rows || !out || n < 1 || n >= ((size_t)1 << 31) || dim < 1 || dim > MX_DMAX) return fail(ctx, PCR_ERR_ARG, "pcr_mat64_create: 1 <= dim <= 8, 1 <= n < 2^31");
    double amax = 0.0;
    for (size_t i = 0; i < n * (size_t)dim; i++) {
        const double a = std::fabs(rows[i]);
        if (!(a <= DBL_MAX)) return fail(ctx, PCR_ERR_ARG, "pcr_mat64_create: non-finite datum");
        amax = a > amax ? a : amax;
    }
    int e = 0;
    if (amax > 0.0) std::frexp(amax, &e);          // amax = f 2^e, f in [0.5, 1): amax < 2^e
    if (e > MX_EMAX || e < -MX_EMAX) return fail(ctx, PCR_ERR_ARG, "pcr_mat64_create: the largest |x| must lie within 2^-400 .. 2^400 (or be 0)");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    pcr_mat64* m = new pcr_mat64();
    m->n = n; m->dim = dim; m->e = e;
    bool ok = hipMalloc(&m->x, n * dim * sizeof(double)) == hipSuccess && hipMalloc(&m->labels, n * sizeof(int32_t)) == hipSuccess &&
              hipMalloc(&m->acc, MX_ACC_WORDS * sizeof(long long)) == hipSuccess && hipMalloc(&m->chosen, (MX_KMAX + 2) * sizeof(int32_t)) == hipSuccess &&
              hipMalloc(&m->st_dev, sizeof(MxState)) == hipSuccess && hipHostMalloc(&m->st_host, sizeof(MxState)) == hipSuccess;
    ok = ok && hipMemcpyAsync(m->x, rows, n * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
         hipMemsetAsync(m->acc, 0, MX_ACC_WORDS * sizeof(long long), ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        pcr_mat64_destroy(ctx, m);
        return fail(ctx, PCR_ERR_NOMEM, "pcr_mat64_create");
    }
    *out = m;
    return PCR_OK;
}

extern "C" int pcr_mat64_destroy(pcr_ctx* ctx, pcr_mat64* m)
{
    if (!m) return PCR_OK;
    if (ctx && ctx->stream) hipStreamSynchronize(ctx->stream);
    if (m->x) hipFree(m->x);
    if (m->labels) hipFree(m->labels);
    if (m->post) hipFree(m->post);
    if (m->seedbuf) hipFree(m->seedbuf);
    if (m->scan_tmp) hipFree(m->scan_tmp);
    if (m->acc) hipFree(m->acc);
    if (m->chosen) hipFree(m->chosen);
    if (m->st_dev) hipFree(m->st_dev);
    if (m->st_host) hipHostFree(m->st_host);
    delete m;
    return PCR_OK;
}

namespace pcr {
const double* mat64_rows_dev(const pcr_mat64* m) { return m ? m->x : nullptr; }
}

extern "C" int pcr_mat64_info(const pcr_mat64* m, size_t* n, int* dim, int* grid_exponent)
{
    if (!m) return PCR_ERR_ARG;
    if (n) *n = m->n;
    if (dim) *dim = m->dim;
    if (grid_exponent) *grid_exponent = m->e;
    return PCR_OK;
}

extern "C" int pcr_kmeans_step_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* centres_in, int32_t* labels, int64_t* counts, double* centres_out)
{
    if (!ctx || !mx_shape_ok(m, k) || !centres_in || !mx_finite(centres_in, (size_t)k * m->dim)) return fail(ctx, PCR_ERR_ARG, "pcr_kmeans_step_f64: 1 <= k <= 64, k <= n, finite centres");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    mx_state_init(m, k, MX_STEP, 0, 0.0);
    memcpy(m->st_host->centres, centres_in, (size_t)k * m->dim * sizeof(double));
    int rc = mx_state_push(ctx, m);
    if (rc == PCR_OK) rc = mx_launch_assign(ctx, m, k, true);
    if (rc != PCR_OK) return rc;
    km_finish_kernel<<<1, MX_BLOCK, 0, ctx->stream>>>(m->acc, m->st_dev);
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = mx_state_pull(ctx, m, sizeof(MxState))) != PCR_OK) return rc;
    if ((rc = mx_fetch_labels(ctx, m, labels)) != PCR_OK) return rc;
    if (counts) for (int j = 0; j < k; j++) counts[j] = (int64_t)m->st_host->counts[j];
    if (centres_out) memcpy(centres_out, m->st_host->cnew, (size_t)k * m->dim * sizeof(double));
    return m->st_host->rec.status;
}

extern "C" int pcr_kmeans_fit_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* init_centres, double tol, int max_iter, int mode, double* centres,
                                  int32_t* labels, int* iters, int* converged)
{
    if (!ctx || !mx_shape_ok(m, k) || !init_centres || !mx_finite(init_centres, (size_t)k * m->dim) || max_iter < 0 || max_iter > (1 << 30) || tol != tol ||
        (mode != PCR_KMEANS_PY && mode != PCR_KMEANS_CPP))
        return fail(ctx, PCR_ERR_ARG, "pcr_kmeans_fit_f64");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    mx_state_init(m, k, mode == PCR_KMEANS_PY ? MX_FIT_PY : MX_FIT_CPP, max_iter, tol);
    memcpy(m->st_host->centres, init_centres, (size_t)k * m->dim * sizeof(double));
    int rc = mx_state_push(ctx, m);
    if (rc != PCR_OK) return rc;
    const long long total = (long long)max_iter + 1;              // both loops make at most max_iter + 1 passes
    long long batch = tune_get(ctx, "mixture_batch", 8);
    if (batch < 1) batch = 1;                                     // a batch of no passes would never end the loop below
    long long done = 0;
    while (done < total) {
        const long long b = total - done < batch ? total - done : batch;
        for (long long t = 0; t < b; t++) {
            if ((rc = mx_launch_assign(ctx, m, k, true)) != PCR_OK) return rc;
            km_finish_kernel<<<1, MX_BLOCK, 0, ctx->stream>>>(m->acc, m->st_dev);
        }
        PCR_HIP(ctx, hipGetLastError());
        if ((rc = mx_state_pull(ctx, m, sizeof(MxRec))) != PCR_OK) return rc;       // the status record, nothing else
        done += b;
        if (m->st_host->rec.stop) break;
    }
    if ((rc = mx_state_pull(ctx, m, sizeof(MxState))) != PCR_OK) return rc;
    const int status = m->st_host->rec.status;
    if (centres) memcpy(centres, m->st_host->centres, (size_t)k * m->dim * sizeof(double));
    if (iters) *iters = m->st_host->rec.iters;
    if (converged) *converged = m->st_host->rec.converged;
    if (labels && status == PCR_OK) {                              // KMeans.predict under the final centres
        m->st_host->rec.stop = 0;
        if ((rc = mx_state_push(ctx, m)) != PCR_OK) return rc;
        if ((rc = mx_launch_assign(ctx, m, k, false)) != PCR_OK) return rc;
        if ((rc = mx_fetch_labels(ctx, m, labels)) != PCR_OK) return rc;
    }
    return status;
}

extern "C" int pcr_kmeans_predict_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* centres, int32_t* labels)
{
    if (!ctx || !m || !m->x || k < 1 || k > MX_KMAX || !centres || !labels || !mx_finite(centres, (size_t)k * m->dim)) return fail(ctx, PCR_ERR_ARG, "pcr_kmeans_predict_f64");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    mx_state_init(m, k, MX_STEP, 0, 0.0);
    memcpy(m->st_host->centres, centres, (size_t)k * m->dim * sizeof(double));
    int rc = mx_state_push(ctx, m);
    if (rc == PCR_OK) rc = mx_launch_assign(ctx, m, k, false);
    if (rc == PCR_OK) rc = mx_fetch_labels(ctx, m, labels);
    return rc;
}

extern "C" int pcr_kmeanspp_init_f64(pcr_ctx* ctx, pcr_mat64* m, int k, double factor, const double* u, uint64_t seed, int32_t* idx_out, double* p_last)
{
    if (!ctx || !mx_shape_ok(m, k) || !idx_out || !(factor >= 0.0) || !(factor <= DBL_MAX)) return fail(ctx, PCR_ERR_ARG, "pcr_kmeanspp_init_f64");
    double uu[MX_KMAX];
    for (int j = 0; j < k; j++) {
        uu[j] = u ? u[j] : (double)(mx_key(seed, (unsigned long long)j) >> 11) * (1.0 / 9007199254740992.0);
        if (!(uu[j] >= 0.0) || !(uu[j] < 1.0)) return fail(ctx, PCR_ERR_ARG, "pcr_kmeanspp_init_f64: 0 <= u < 1");
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)m->n;
    if (!m->seedbuf && hipMalloc(&m->seedbuf, 3 * m->n * sizeof(double)) != hipSuccess) return fail(ctx, PCR_ERR_NOMEM, "pcr_kmeanspp_init_f64");
    double *dmin = m->seedbuf, *w = m->seedbuf + m->n, *cdf = m->seedbuf + 2 * m->n;
    if (!m->scan_tmp) {
        size_t bytes = 0;
        PCR_HIP(ctx, rocprim::inclusive_scan(nullptr, bytes, w, cdf, m->n, rocprim::plus<double>(), ctx->stream));
        if (hipMalloc(&m->scan_tmp, bytes ? bytes : 8) != hipSuccess) return fail(ctx, PCR_ERR_NOMEM, "pcr_kmeanspp_init_f64");
        m->scan_bytes = bytes;
    }
    int32_t head[MX_KMAX + 2] = { 0 };
    size_t first = (size_t)std::floor(uu[0] * (double)m->n);
    head[0] = (int32_t)(first < m->n ? first : m->n - 1);
    PCR_HIP(ctx, hipMemcpyAsync(m->chosen, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    long long* accs = m->acc + MX_ACC1 + MX_ACC2;
    int* flag = (int*)(m->chosen + MX_KMAX);
    const MxGeom g = mx_geom(ctx, m->n, 1, 1);
    for (int j = 1; j < k; j++) {
        // d < 2 sqrt(dim) 2^e < 2^(e + 3): the limb grid of the running minimum
        MX_DISPATCH_DIM(m->dim, (seed_min_kernel<D><<<g.blocks, g.block, 0, ctx->stream>>>(m->x, n, m->chosen, j, dmin, 96 - (m->e + 3), accs)));
        seed_weight_kernel<<<g.blocks, g.block, 0, ctx->stream>>>(dmin, n, accs, m->e + 3 - 96, factor, w, flag);
        PCR_HIP(ctx, rocprim::inclusive_scan(m->scan_tmp, m->scan_bytes, w, cdf, m->n, rocprim::plus<double>(), ctx->stream));
        seed_pick_kernel<<<1, 64, 0, ctx->stream>>>(cdf, n, uu[j], m->chosen, j, accs, flag);
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(head, m->chosen, sizeof(head), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (head[MX_KMAX] || head[MX_KMAX + 1])
        return fail(ctx, PCR_ERR_STATE, head[MX_KMAX] ? "pcr_kmeanspp_init_f64: exp(d) overflows (d > 709)" : "pcr_kmeanspp_init_f64: the weights do not sum to a positive number");
    for (int j = 0; j < k; j++) idx_out[j] = head[j];
    if (p_last) {
        if (k < 2) return fail(ctx, PCR_ERR_ARG, "pcr_kmeanspp_init_f64: p_last needs k >= 2");
        seed_prob_kernel<<<g.blocks, g.block, 0, ctx->stream>>>(w, cdf, n, dmin);
        PCR_HIP(ctx, hipMemcpyAsync(p_last, dmin, m->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PCR_OK;
}

extern "C" int pcr_gmm_em_step_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* mean_in, const double* cov_in, const double* pi_in, double* mean_out,
                                   double* cov_out, double* pi_out, double* post)
{
    if (!ctx || !mx_shape_ok(m, k) || !mx_params_ok(m, k, mean_in, cov_in, pi_in)) return fail(ctx, PCR_ERR_ARG, "pcr_gmm_em_step_f64");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const int dim = m->dim;
    int rc = mx_ensure_post(ctx, m, k);
    if (rc != PCR_OK) return rc;
    mx_state_init(m, k, MX_STEP, 0, 0.0);
    memcpy(m->st_host->centres, mean_in, (size_t)k * dim * sizeof(double));
    memcpy(m->st_host->cov, cov_in, (size_t)k * dim * dim * sizeof(double));
    memcpy(m->st_host->pi, pi_in, (size_t)k * sizeof(double));
    if ((rc = mx_state_push(ctx, m)) != PCR_OK) return rc;
    if ((rc = mx_launch_em(ctx, m, k)) != PCR_OK) return rc;
    if ((rc = mx_state_pull(ctx, m, sizeof(MxState))) != PCR_OK) return rc;
    if (m->st_host->rec.status != PCR_OK) return fail(ctx, PCR_ERR_STATE, "pcr_gmm_em_step_f64: a covariance is not positive definite");
    if (mean_out) memcpy(mean_out, m->st_host->cnew, (size_t)k * dim * sizeof(double));
    if (cov_out) memcpy(cov_out, m->st_host->cov_new, (size_t)k * dim * dim * sizeof(double));
    if (pi_out) memcpy(pi_out, m->st_host->pi_new, (size_t)k * sizeof(double));
    if (post) {                                     // k-major on the device, n x k for the caller (GMM.posterior's shape)
        std::vector<double> tmp((size_t)k * m->n);
        PCR_HIP(ctx, hipMemcpy(tmp.data(), m->post, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m->n; i++)
            for (int j = 0; j < k; j++) post[i * k + j] = tmp[(size_t)j * m->n + i];
    }
    return PCR_OK;
}

extern "C" int pcr_gmm_fit_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* init_mean, double amplitude, double eps, int max_iter, uint64_t seed,
                               double* mean, double* cov, double* pi, int* iters, int* converged, int* resets)
{
    if (!ctx || !mx_shape_ok(m, k) || !init_mean || !mx_finite(init_mean, (size_t)k * m->dim) || !(amplitude > 0.0) || !(amplitude <= DBL_MAX) || eps != eps ||
        max_iter < 1 || max_iter > (1 << 30))
        return fail(ctx, PCR_ERR_ARG, "pcr_gmm_fit_f64");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const int dim = m->dim;
    int rc = mx_ensure_post(ctx, m, k);
    if (rc != PCR_OK) return rc;
    mx_state_init(m, k, MX_FIT_PY, max_iter, eps);
    MxState* s = m->st_host;
    s->seed = seed; s->amplitude = amplitude;
    memcpy(s->centres, init_mean, (size_t)k * dim * sizeof(double));
    for (int j = 0; j < k; j++) {
        for (int a = 0; a < dim; a++) s->cov[(j * dim + a) * dim + a] = amplitude;
        s->pi[j] = 1.0 / (double)k;
    }
    if ((rc = mx_state_push(ctx, m)) != PCR_OK) return rc;
    long long batch = tune_get(ctx, "mixture_batch", 8);
    if (batch < 1) batch = 1;                                     // a batch of no passes would never end the loop below
    long long done = 0;
    while (done < max_iter) {
        const long long b = max_iter - done < batch ? max_iter - done : batch;
        for (long long t = 0; t < b; t++)
            if ((rc = mx_launch_em(ctx, m, k)) != PCR_OK) return rc;
        if ((rc = mx_state_pull(ctx, m, sizeof(MxRec))) != PCR_OK) return rc;
        done += b;
        if (m->st_host->rec.stop) break;
    }
    if ((rc = mx_state_pull(ctx, m, sizeof(MxState))) != PCR_OK) return rc;
    if (iters) *iters = s->rec.iters;
    if (converged) *converged = s->rec.converged;
    if (resets) *resets = s->rec.resets;
    if (s->rec.status != PCR_OK) return fail(ctx, PCR_ERR_STATE, "pcr_gmm_fit_f64: a covariance is not positive definite");
    if (mean) memcpy(mean, s->centres, (size_t)k * dim * sizeof(double));
    if (cov) memcpy(cov, s->cov, (size_t)k * dim * dim * sizeof(double));
    if (pi) memcpy(pi, s->pi, (size_t)k * sizeof(double));
    return PCR_OK;
}

extern "C" int pcr_gmm_predict_f64(pcr_ctx* ctx, pcr_mat64* m, int k, const double* mean, const double* cov, const double* pi, int32_t* labels)
{
    if (!ctx || !m || !m->x || k < 1 || k > MX_KMAX || !labels || !mx_params_ok(m, k, mean, cov, pi)) return fail(ctx, PCR_ERR_ARG, "pcr_gmm_predict_f64");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const int dim = m->dim;
    mx_state_init(m, k, MX_STEP, 0, 0.0);
    memcpy(m->st_host->centres, mean, (size_t)k * dim * sizeof(double));
    memcpy(m->st_host->cov, cov, (size_t)k * dim * dim * sizeof(double));
    memcpy(m->st_host->pi, pi, (size_t)k * sizeof(double));
    int rc = mx_state_push(ctx, m);
    if (rc != PCR_OK) return rc;
    em_prep_kernel<<<1, 64, 0, ctx->stream>>>(m->st_dev);
    em_prep_check_kernel<<<1, 64, 0, ctx->stream>>>(m->st_dev);
    const MxGeom g = mx_geom(ctx, m->n, 1, 1);
    const size_t lds = ((size_t)k * dim + (size_t)k * dim * dim + k) * 8;
    MX_DISPATCH_DIM(dim, (em_resp_kernel<D, true><<<g.blocks, g.block, lds, ctx->stream>>>(m->x, (uint32_t)m->n, k, m->st_dev, nullptr, m->labels)));
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = mx_state_pull(ctx, m, sizeof(MxRec))) != PCR_OK) return rc;
    if (m->st_host->rec.status != PCR_OK) return fail(ctx, PCR_ERR_STATE, "pcr_gmm_predict_f64: a covariance is not positive definite");
    return mx_fetch_labels(ctx, m, labels);
}
