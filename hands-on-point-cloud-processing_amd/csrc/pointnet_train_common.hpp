// pointnet_train_common.hpp — what the two training passes share (pointnet2_train.hip: PointNet++, SSG and MSG; pointnet_train.hip: the vanilla PointNet).
// Kernels: the strided MFMA product, the chunked f64 statistics, BatchNorm / ReLU forward and backward, the in-place dropout, the max with its argmax, the loss.
// Every kernel here keeps its profile name in both passes.
// Host: the trainer handle; layer_push (the weight layout of a layer); trainer_finish (what both creates do behind their shape check); trainer_info_common;
// the optimiser's part of the handle (pointnet_optim.hip holds its kernel and calls); keep_rule (the dropout mask by rule); PlanBase (the shared part of a call's device block); call_head / call_upload / call_tail (the checks, the staging and
// the downloads of a call); LayerRun (one layer forward, one layer backward, the bias gradient, the max's scatter back: the only place that launches them).
// What a pass keeps to itself: its plan's own buffers, and what happens between the layers (its layers, limits and weight count: pointnet_layers.hpp).
// The contracts are above pcr_pn2_trainer_create, pcr_pn2_msg_trainer_create and pcr_pn1_trainer_create in include/pcr.h.
#pragma once
#include "pcr_internal.hpp"
#include "pointnet_layers.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

using namespace pcr;

namespace {

constexpr int T_BLOCK = 256;
constexpr uint32_t T_DEFAULT_CHUNK = 256;
constexpr uint32_t T_NONE = 0xFFFFFFFFu;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct TLayer {
    uint32_t K, N;
    bool bn;
    size_t w, b, gamma, beta, rmean, rvar;      // offsets into the flat weight array
};

struct GemmArgs {
    const float* a;      // A(i, k) = a[i * sai + k * sak]
    const float* b;      // B(k, j) = b[k * sbk + j * sbj]
    const float* init;   // N floats the accumulators start from, or NULL: +0
    float* c;            // C(i, j) = c[chunk * c_stride + i * N + j]
    uint32_t M, N, Kt, chunk;
    size_t sai, sak, sbk, sbj, c_stride;
};

// C = init + A B, chunk by chunk of k (one chunk = all of k for the forward and the dx product).  A wave owns 32 rows x 64 columns (two row tiles share
// the B operands, four column tiles the A operands); MFMA number m of its loop takes k = 4 m + (lane >> 4), so that every output is one chain over
// ascending k.  Operands past an edge are read as +0.
constexpr int T_RT = 2;                  // 16-row tiles per wave
constexpr int T_ROWS = 4 * 16 * T_RT;    // rows per workgroup
__global__ __launch_bounds__(T_BLOCK) void pn2t_gemm_kernel(const GemmArgs g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, h = lane >> 4;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * 4 + (unsigned)wave) * (16 * T_RT);
    if (i0 >= g.M) return;                                      // wave-uniform; the kernel has no barrier
    const uint32_t j0 = blockIdx.y * 64;
    const uint32_t kb = blockIdx.z * g.chunk, ke = g.Kt - kb < g.chunk ? g.Kt : kb + g.chunk;
    f32x4 acc[T_RT][4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t col = j0 + 16 * t + j;
        const float v = (g.init && col < g.N) ? g.init[col] : 0.0f;
#pragma unroll
        for (int rt = 0; rt < T_RT; rt++) acc[rt][t] = f32x4{ v, v, v, v };
    }
    bool row_ok[T_RT];
    const float* ap[T_RT];
#pragma unroll
    for (int rt = 0; rt < T_RT; rt++) {
        row_ok[rt] = i0 + 16 * rt + j < g.M;
        ap[rt] = g.a + (row_ok[rt] ? (size_t)(i0 + 16 * rt + j) * g.sai : 0);
    }
    const int nt = (int)std::min<uint32_t>(4u, (g.N - j0 + 15u) / 16u);      // wave-uniform: the 16-column tiles that hold a column
    const bool two = i0 + 16 < g.M;                                           // wave-uniform: the second row tile holds a row
#pragma unroll 2
    for (uint32_t k = kb; k < ke; k += 4) {
        const uint32_t kk = k + (uint32_t)h;
        const bool k_ok = kk < ke;
        float av[T_RT], bv[4];
#pragma unroll
        for (int rt = 0; rt < T_RT; rt++) av[rt] = (row_ok[rt] && k_ok) ? ap[rt][(size_t)kk * g.sak] : 0.0f;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t col = j0 + 16 * t + j;
            bv[t] = (k_ok && col < g.N) ? g.b[(size_t)kk * g.sbk + (size_t)col * g.sbj] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (t < nt) {
                acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[t], acc[0][t], 0, 0, 0);
                if (two) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[t], acc[1][t], 0, 0, 0);
            }
    }
    float* cp = g.c + (size_t)blockIdx.z * g.c_stride;
#pragma unroll
    for (int rt = 0; rt < T_RT; rt++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t col = j0 + 16 * t + j;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const unsigned long long row = i0 + 16 * rt + 4 * h + reg;
                if (row < g.M && col < g.N) cp[(size_t)row * g.N + col] = acc[rt][t][reg];
            }
        }
}

// the rows of one branch of an SA layer.  grouped: row r = (centre q = r / nsample, member k = r % nsample) reads point idx[q][k] of its object;
// group_all (idx == NULL): row r is point r.  x[r] = (xyz - centre | features), or (features | xyz - centre) with xyz_last; row_pt[r] = the point
// (T_NONE: a member outside its object, a row of zeros)
__global__ __launch_bounds__(T_BLOCK) void pn2t_gather_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                              const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                              const float* __restrict__ feat, const uint32_t* __restrict__ idx, uint32_t rows, uint32_t nsample,
                                                              uint32_t npoint, uint32_t n_prev, uint32_t D, uint32_t xyz_last, float* __restrict__ x,
                                                              uint32_t* __restrict__ row_pt)
{
    const uint32_t r = blockIdx.x * T_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const uint32_t K = 3 + D, cx0 = xyz_last ? D : 0u, cf0 = xyz_last ? 0u : 3u;      // the first xyz column, the first feature column
    float* xr = x + (size_t)r * K;
    uint32_t p = r;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    bool sub = false;
    if (idx) {
        const uint32_t q = r / nsample, o = q / npoint, i = idx[r];
        if (i >= n_prev) {
            for (uint32_t c = 0; c < K; c++) xr[c] = 0.0f;
            row_pt[r] = T_NONE;
            return;
        }
        p = o * n_prev + i;
        cx = qx[q]; cy = qy[q]; cz = qz[q];
        sub = true;
    }
    row_pt[r] = p;
    xr[cx0] = sub ? px[p] - cx : px[p];
    xr[cx0 + 1] = sub ? py[p] - cy : py[p];
    xr[cx0 + 2] = sub ? pz[p] - cz : pz[p];
    for (uint32_t c = 0; c < D; c++) xr[cf0 + c] = feat[(size_t)p * D + c];
}

__global__ __launch_bounds__(T_BLOCK) void pn2t_centres_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                               const uint32_t* __restrict__ fps, uint32_t n, uint32_t npoint, uint32_t total,
                                                               float* __restrict__ cx, float* __restrict__ cy, float* __restrict__ cz)
{
    const uint32_t q = blockIdx.x * T_BLOCK + threadIdx.x;
    if (q >= total) return;
    uint32_t i = fps[q];
    if (i >= n) i = n - 1;      // (never: a pick is a member)
    const size_t p = (size_t)(q / npoint) * n + i;
    cx[q] = x[p]; cy[q] = y[p]; cz[q] = z[p];
}

// part[c][n] <- the f64 sum over the rows of chunk c, ascending, of v (mu == NULL) or of (v - mu[n])^2
__global__ __launch_bounds__(T_BLOCK) void pn2t_stat_part_kernel(const float* __restrict__ v, uint32_t M, uint32_t N, uint32_t chunk, uint32_t chunks,
                                                                 const double* __restrict__ mu, double* __restrict__ part)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= (size_t)chunks * N) return;
    const uint32_t c = (uint32_t)(e / N), n = (uint32_t)(e - (size_t)c * N);
    const uint32_t r0 = c * chunk, r1 = M - r0 < chunk ? M : r0 + chunk;
    double s = 0.0;
    if (mu) {
        const double m = mu[n];
#pragma unroll 8
        for (uint32_t r = r0; r < r1; r++) { const double d = (double)v[(size_t)r * N + n] - m; s = s + d * d; }
    } else {
#pragma unroll 8
        for (uint32_t r = r0; r < r1; r++) s = s + (double)v[(size_t)r * N + n];
    }
    part[e] = s;
}

// pass 0: mu <- the sum / M.  pass 1: var <- the sum / M, rstd, and the running statistics (f64, rounded once).  pass 2: out32 <- the sum (a bias gradient)
__global__ __launch_bounds__(T_BLOCK) void pn2t_stat_fin_kernel(const double* __restrict__ part, uint32_t chunks, uint32_t N, uint32_t M, int pass, double* __restrict__ mu,
                                                                double* __restrict__ var, double* __restrict__ rstd, double eps, double mom, float* __restrict__ rmean,
                                                                float* __restrict__ rvar, float* __restrict__ out32)
{
    const uint32_t n = blockIdx.x * T_BLOCK + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (uint32_t c = 0; c < chunks; c++) s = s + part[(size_t)c * N + n];
    if (pass == 0) {
        mu[n] = s / (double)M;
    } else if (pass == 1) {
        const double vv = s / (double)M;
        var[n] = vv;
        rstd[n] = 1.0 / sqrt(vv + eps);
        rmean[n] = (float)((1.0 - mom) * (double)rmean[n] + mom * mu[n]);
        rvar[n] = (float)((1.0 - mom) * (double)rvar[n] + mom * (vv * (double)M / (double)(M - 1)));
    } else {
        out32[n] = (float)s;
    }
}

// y = relu((z - mu) rstd gamma + beta) (RELU == false: without the relu), evaluated in f64 and rounded once; a (head) = y keep s
template <bool RELU>
__global__ __launch_bounds__(T_BLOCK) void pn2t_bn_relu_kernel(const float* __restrict__ z, size_t total, uint32_t N, const double* __restrict__ mu,
                                                               const double* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ y, const uint8_t* __restrict__ keep, float s, float* __restrict__ a)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const uint32_t n = (uint32_t)(e % N);
    float v = (float)(((double)z[e] - mu[n]) * rstd[n] * (double)gamma[n] + (double)beta[n]);
    if (RELU) v = v > 0.0f ? v : 0.0f;
    y[e] = v;
    if (a) a[e] = (!keep || keep[e]) ? v * s : 0.0f;
}

// feat[g][off + c] = the max over the gsize rows of group g; arg[g][off + c] = the lowest position that holds it, T_NONE where the max is 0.
// feat and arg have rows of `stride` cells: a branch writes its own columns [off, off + N) of the layer's concatenated row
__global__ __launch_bounds__(T_BLOCK) void pn2t_max_kernel(const float* __restrict__ y, uint32_t groups, uint32_t gsize, uint32_t N, uint32_t stride, uint32_t off,
                                                           float* __restrict__ feat, uint32_t* __restrict__ arg)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= (size_t)groups * N) return;
    const uint32_t g = (uint32_t)(e / N), c = (uint32_t)(e - (size_t)g * N);
    const float* p = y + (size_t)g * gsize * N + c;
    float m = p[0];
    uint32_t best = 0;
    for (uint32_t k = 1; k < gsize; k++) {
        const float v = p[(size_t)k * N];
        if (v > m) { m = v; best = k; }
    }
    const size_t o = (size_t)g * stride + off + c;
    feat[o] = m;
    arg[o] = m > 0.0f ? best : T_NONE;
}

// dy[r][c] = dfeat[g][off + c] where row r is position arg[g][off + c] of its group g, +0 elsewhere (dfeat and arg: rows of `stride` cells)
__global__ __launch_bounds__(T_BLOCK) void pn2t_max_back_kernel(const float* __restrict__ dfeat, const uint32_t* __restrict__ arg, size_t total, uint32_t gsize, uint32_t N,
                                                                uint32_t stride, uint32_t off, float* __restrict__ dy)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const size_t r = e / N;
    const uint32_t c = (uint32_t)(e - r * N);
    const size_t g = r / gsize;
    const uint32_t k = (uint32_t)(r - g * gsize);
    const size_t o = g * stride + off + c;
    dy[e] = arg[o] == k ? dfeat[o] : 0.0f;
}

// the gradient that reaches BN's output at element e: dropout (the same mask and s), then ReLU (passes where y > 0; RELU == false: everywhere)
template <bool RELU>
__device__ __forceinline__ float pn2t_gy(const float* dy, const float* y, const uint8_t* keep, float s, size_t e)
{
    float g = dy[e];
    if (keep) g = keep[e] ? g * s : 0.0f;
    return (!RELU || y[e] > 0.0f) ? g : 0.0f;
}

// part[c][0][n] <- sum gy, part[c][1][n] <- sum gy xhat over the rows of chunk c, ascending, in f64
template <bool RELU>
__global__ __launch_bounds__(T_BLOCK) void pn2t_bnb_part_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                                                const uint8_t* __restrict__ keep, float s, uint32_t M, uint32_t N, uint32_t chunk, uint32_t chunks,
                                                                const double* __restrict__ mu, const double* __restrict__ rstd, double* __restrict__ part)
{
    const size_t t = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (t >= (size_t)chunks * N) return;
    const uint32_t c = (uint32_t)(t / N), n = (uint32_t)(t - (size_t)c * N);
    const uint32_t r0 = c * chunk, r1 = M - r0 < chunk ? M : r0 + chunk;
    const double m = mu[n], rs = rstd[n];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (uint32_t r = r0; r < r1; r++) {
        const size_t e = (size_t)r * N + n;
        const double g = (double)pn2t_gy<RELU>(dy, y, keep, s, e);
        s0 = s0 + g;
        s1 = s1 + g * (((double)z[e] - m) * rs);
    }
    part[((size_t)c * 2) * N + n] = s0;
    part[((size_t)c * 2 + 1) * N + n] = s1;
}

__global__ __launch_bounds__(T_BLOCK) void pn2t_bnb_fin_kernel(const double* __restrict__ part, uint32_t chunks, uint32_t N, uint32_t M, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, double* __restrict__ mean_g, double* __restrict__ mean_gx)
{
    const uint32_t n = blockIdx.x * T_BLOCK + threadIdx.x;
    if (n >= N) return;
    double s0 = 0.0, s1 = 0.0;
    for (uint32_t c = 0; c < chunks; c++) {
        s0 = s0 + part[((size_t)c * 2) * N + n];
        s1 = s1 + part[((size_t)c * 2 + 1) * N + n];
    }
    dbeta[n] = (float)s0;
    dgamma[n] = (float)s1;
    mean_g[n] = s0 / (double)M;
    mean_gx[n] = s1 / (double)M;
}

// dy <- dz = rstd gamma (gy - mean(gy) - xhat mean(gy xhat)), in f64, rounded once
template <bool RELU>
__global__ __launch_bounds__(T_BLOCK) void pn2t_bnb_dz_kernel(float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z, const uint8_t* __restrict__ keep,
                                                              float s, size_t total, uint32_t N, const double* __restrict__ mu, const double* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const double* __restrict__ mean_g, const double* __restrict__ mean_gx)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const uint32_t n = (uint32_t)(e % N);
    const double g = (double)pn2t_gy<RELU>(dy, y, keep, s, e);
    const double xhat = ((double)z[e] - mu[n]) * rstd[n];
    dy[e] = (float)(rstd[n] * (double)gamma[n] * (g - mean_g[n] - xhat * mean_gx[n]));
}

__global__ __launch_bounds__(T_BLOCK) void pn2t_dw_reduce_kernel(const float* __restrict__ part, uint32_t chunks, size_t cells, float* __restrict__ dw)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= cells) return;
    float s = part[e];
    for (uint32_t c = 1; c < chunks; c++) s = s + part[(size_t)c * cells + e];
    dw[e] = s;
}

// one branch's part of the f64 sum per (point p, channel c), rows ascending, of dx[r][col0 + c] over the rows r of p's object that read point p (col0: the
// first feature column, 3 or, with xyz_last, 0).  The sum starts at +0 (acc_in == NULL: the first branch) or goes on from acc_in[p][c]; it is handed on in
// acc_out[p][c], or (acc_out == NULL: the last branch) rounded once into dfeat[p][c].  Branches ascending, one launch each: one chain over all the rows.
// One workgroup per point.  Every wave walks row_pt 64 rows at a time (one coalesced load, one ballot) and takes the matching rows in ascending order,
// so a thread's sums are chains over ascending rows; a thread owns channels threadIdx.x + 256 j, at most four of them (D <= PN_MAX_WIDTH - 3)
__global__ __launch_bounds__(T_BLOCK) void pn2t_gather_back_kernel(const float* __restrict__ dx, const uint32_t* __restrict__ row_pt, uint32_t points, uint32_t n_prev,
                                                                   uint32_t rows_per_obj, uint32_t D, uint32_t col0, const double* acc_in, double* acc_out,
                                                                   float* __restrict__ dfeat)
{
    constexpr int CH = (PN_MAX_WIDTH + T_BLOCK - 1) / T_BLOCK;
    const uint32_t p = blockIdx.x;
    if (p >= points) return;
    const uint32_t o = p / n_prev, K = 3 + D, lane = threadIdx.x & 63;
    const size_t r0 = (size_t)o * rows_per_obj;
    double s[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) {
        const uint32_t c = threadIdx.x + (uint32_t)j * T_BLOCK;
        s[j] = (acc_in && c < D) ? acc_in[(size_t)p * D + c] : 0.0;
    }
    for (uint32_t k0 = 0; k0 < rows_per_obj; k0 += 64) {         // wave-uniform trip count; the kernel has no barrier
        const uint32_t k = k0 + lane;
        unsigned long long m = __ballot(k < rows_per_obj && row_pt[r0 + k] == p);
        while (m) {                                              // the matching rows of these 64, ascending
            const uint32_t bit = (uint32_t)__ffsll((long long)m) - 1u;
            m &= m - 1;
            const float* row = dx + (r0 + k0 + bit) * K + col0;
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const uint32_t c = threadIdx.x + (uint32_t)j * T_BLOCK;
                if (c < D) s[j] = s[j] + (double)row[c];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CH; j++) {
        const uint32_t c = threadIdx.x + (uint32_t)j * T_BLOCK;
        if (c >= D) continue;
        if (acc_out) acc_out[(size_t)p * D + c] = s[j];
        else dfeat[(size_t)p * D + c] = (float)s[j];
    }
}

// one workgroup: log_softmax of every row as the eval pass takes it, dlogits = (exp(logp) - onehot) / n_obj, loss = -(1 / n_obj) sum_b logp[b][target[b]] over
// ascending b in f64
__global__ __launch_bounds__(T_BLOCK) void pn2t_loss_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, uint32_t n_obj, uint32_t n_class,
                                                            float* __restrict__ logp, float* __restrict__ dlogits, double* __restrict__ loss)
{
    for (uint32_t o = threadIdx.x; o < n_obj; o += T_BLOCK) {
        const float* r = logits + (size_t)o * n_class;
        float m = r[0];
        for (uint32_t c = 1; c < n_class; c++)
            if (r[c] > m) m = r[c];
        float s = 0.0f;
        for (uint32_t c = 0; c < n_class; c++) s = s + expf(r[c] - m);
        const float ls = logf(s);
        for (uint32_t c = 0; c < n_class; c++) {
            const float lp = (r[c] - m) - ls;
            logp[(size_t)o * n_class + c] = lp;
            dlogits[(size_t)o * n_class + c] = (float)((exp((double)lp) - ((int32_t)c == target[o] ? 1.0 : 0.0)) / (double)n_obj);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t o = 0; o < n_obj; o++) s = s + (double)logp[(size_t)o * n_class + (uint32_t)target[o]];
        *loss = -s / (double)n_obj;
    }
}

// v <- keep ? v s : +0: a dropout BEFORE BatchNorm, in place (pointnet_cls's head: forward on the product, backward on its gradient)
__global__ __launch_bounds__(T_BLOCK) void pn1t_dropout_kernel(float* __restrict__ v, const uint8_t* __restrict__ keep, float s, size_t total)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    v[e] = keep[e] ? v[e] * s : 0.0f;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + T_BLOCK - 1) / T_BLOCK); }

}  // namespace

// the handle of every trainer.  kind 0: pcr_pn2_trainer_create and pcr_pn2_msg_trainer_create (desc: the superset descriptor; sa_*, head_first, n_sampling);
// kind 1: pcr_pn1_trainer_create (desc1, the first layer of its five parts, reg_scale; desc.bn_eps mirrors desc1.bn_eps)
struct pcr_pn2_trainer {
    pcr_pn2_msg_desc desc;
    int device = 0;
    std::vector<TLayer> layers;          // weight order
    uint32_t sa_first[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH];      // the first layer of every (SA stage, branch)
    uint32_t sa_in[PCR_PN2_MAX_SA], sa_out[PCR_PN2_MAX_SA];
    uint32_t head_first = 0, n_sampling = 0;
    uint64_t n_weights = 0;
    float drop_p[PCR_PN2_MAX_FC] = {}, drop_s[PCR_PN2_MAX_FC] = { 1.0f, 1.0f, 1.0f, 1.0f };      // per head layer (layer index - head_first): p and f32(1 / (1 - p))
    double momentum = 0.1;
    uint32_t chunk_rows = T_DEFAULT_CHUNK;
    float* w_dev = nullptr;              // the flat weight array, running statistics included
    float* grad_dev = nullptr;           // the same layout
    int kind = 0;
    pcr_pn1_desc desc1;
    uint32_t stn_first = 0, enc_first = 0, fstn_first = 0;      // kind 1: [stn3's six layers] [the encoder] [fstn's six layers] [the head at head_first]
    double reg_scale = 0.0;
    // the optimiser (pointnet_optim.hip; the contract is above pcr_pn2_trainer_optim_set in include/pcr.h)
    bool pass_ran = false;               // a pass has left a gradient in grad_dev
    bool opt_on = false;
    pcr_optim_desc opt;
    uint64_t opt_step = 0;               // updates applied
    double opt_p1 = 1.0, opt_p2 = 1.0;   // beta1^opt_step, beta2^opt_step: the f64 product chain from 1
    float *opt_s0 = nullptr, *opt_s1 = nullptr;      // Adam: exp_avg, exp_avg_sq; SGD: momentum_buffer, none.  The weight layout
    void* opt_ranges = nullptr;          // the parameter ranges of the flat array on the device (OptRange), opt_n_ranges of them
    uint32_t opt_n_ranges = 0;
};

namespace pcr {
// pcr_pn2_trainer_info for a kind-1 trainer (pointnet_train.hip)
int pn1_trainer_info(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, pcr_pn2_train_info* info);
// pointnet_optim.hip: what is wrong with an update of `t` at `lr` (NULL: nothing); the update launch on the context's stream behind whatever the
// stream holds, the step count advanced; the state freed
const char* optim_bad(const pcr_pn2_trainer* t, double lr);
int optim_launch(pcr_ctx* ctx, pcr_pn2_trainer* t, double lr, const char* who);
void optim_free(pcr_pn2_trainer* t);
}

namespace {

inline const char* weights_ok(const pcr_pn2_trainer* t, const float* w)
{
    for (uint64_t i = 0; i < t->n_weights; i++)
        if (!std::isfinite(w[i])) return ": a non-finite weight";
    for (const TLayer& L : t->layers)
        if (L.bn)
            for (uint32_t n = 0; n < L.N; n++)
                if (!((double)w[L.rvar + n] + t->desc.bn_eps > 0.0)) return ": running_var + eps must be positive";
    return nullptr;
}

// one more layer behind the ones the trainer has, in weight order: w, b and, with BN, gamma, beta, running_mean, running_var.  t.n_weights is the running end
inline void layer_push(pcr_pn2_trainer& t, const LayerShape& s)
{
    const size_t N = s.N;
    TLayer L;
    L.K = s.K; L.N = s.N; L.bn = s.bn;
    L.w = t.n_weights;
    L.b = L.w + (size_t)s.K * N;
    L.gamma = L.beta = L.rmean = L.rvar = 0;
    if (s.bn) { L.gamma = L.b + N; L.beta = L.b + 2 * N; L.rmean = L.b + 3 * N; L.rvar = L.b + 4 * N; }
    t.layers.push_back(L);
    t.n_weights += weight_count(s);
}

// what both creates do once the layers are known: the parameter checks, the two device arrays, the upload.  Every message starts with the caller's name.
// own_bad: the caller's own finding or NULL; it ranks behind bn_momentum.  dropout_p: n_dropout <= PCR_PN2_MAX_FC values, head layer by head layer
inline int trainer_finish(pcr_ctx* ctx, const char* who, std::unique_ptr<pcr_pn2_trainer> t, const char* own_bad, const float* weights, size_t n_weights,
                          const double* dropout_p, size_t n_dropout, double bn_momentum, uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str()); };
    for (size_t i = 0; i < n_dropout; i++)
        if (!(dropout_p[i] >= 0.0 && dropout_p[i] < 1.0)) return bad(": dropout_p must lie in [0, 1)");
    if (!(bn_momentum >= 0.0 && bn_momentum <= 1.0)) return bad(": bn_momentum must lie in [0, 1]");
    if (own_bad) return bad(own_bad);
    if (n_weights != t->n_weights) return bad(": n_weights is not the model's count");
    if (const char* what = weights_ok(t.get(), weights)) return bad(what);
    for (size_t i = 0; i < n_dropout; i++) {
        t->drop_p[i] = (float)dropout_p[i];
        t->drop_s[i] = (float)(1.0 / (1.0 - dropout_p[i]));
    }
    t->momentum = bn_momentum;
    t->chunk_rows = chunk_rows ? chunk_rows : T_DEFAULT_CHUNK;
    t->device = ctx->device;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipMalloc((void**)&t->w_dev, t->n_weights * 4));
    hipError_t e = hipMalloc((void**)&t->grad_dev, t->n_weights * 4);
    if (e == hipSuccess) e = hipMemcpy(t->w_dev, weights, t->n_weights * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->grad_dev, 0, t->n_weights * 4);
    if (e != hipSuccess) {
        (void)hipFree(t->w_dev);
        if (t->grad_dev) (void)hipFree(t->grad_dev);
        return fail(ctx, PCR_ERR_HIP, (std::string(who) + ": the upload of the weights").c_str(), e);
    }
    *out = t.release();
    return PCR_OK;
}

// the fields of pcr_pn2_train_info that the model does not decide; n_sampling, keep_per_object and device_bytes are the caller's
inline void trainer_info_common(const pcr_pn2_trainer* t, pcr_pn2_train_info* info)
{
    memset(info, 0, sizeof(*info));
    info->n_weights = t->n_weights;
    info->chunk_rows = t->chunk_rows;
    info->n_class = t->layers.back().N;
    info->dropout_p = (double)t->drop_p[0];      // the first hidden layer's
    info->bn_momentum = t->momentum;
}

// the dropout mask where the caller gives none: K(seed, (0x100 + layer) << 32 | cell) as a uniform in [0, 1) >= p
inline uint8_t keep_rule(uint64_t seed, uint32_t layer, size_t cell, float p)
{
    return (double)(splitmix_key(seed, ((unsigned long long)(0x100u + layer) << 32) | (unsigned long long)cell) >> 11) * 0x1.0p-53 >= (double)p ? 1 : 0;
}

// the chunked chain product: dW and dT in both passes, z and dx in the SSG pass
inline int launch_gemm(pcr_ctx* ctx, const char* prof, const GemmArgs& g, const char* who)
{
    if (g.M == 0 || g.N == 0) return PCR_OK;
    const uint32_t chunks = g.Kt == 0 ? 1u : (g.Kt + g.chunk - 1) / g.chunk;
    if (chunks > 65535u) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": more than 65535 chunks of rows (raise chunk_rows)").c_str());
    ProfScope ps(ctx, prof);
    hipLaunchKernelGGL(pn2t_gemm_kernel, dim3((g.M + T_ROWS - 1) / T_ROWS, (g.N + 63) / 64, chunks), dim3(T_BLOCK), 0, ctx->stream, g);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// the part of a call's device block that both passes have.  Several Layouts (scratch_layout.hpp holds 24 slots each) laid one behind the other: `up` (the
// uploaded part), `own` (the model's: sampling / per-stack buffers), `work`, then one per layer and whatever the model appends.  The model's make_plan declares
// `up` and `own`, calls layers(), add_layer() per layer and finish()
struct PlanBase {
    int32_t* target = nullptr;       // in `up`
    uint8_t* keep = nullptr;
    size_t upload_bytes = 0;
    // per layer
    std::vector<float*> z, y, a;     // a: y keep s, where the dropout is fused behind the ReLU
    std::vector<double*> stat;       // 5 N doubles: mu, var, rstd, mean_g, mean_gx
    // shared
    float *dyA = nullptr, *dyB = nullptr, *dfeat = nullptr, *dw_part = nullptr, *logp = nullptr;
    double *part = nullptr, *loss = nullptr, *dacc = nullptr;
    size_t dy_cells = 1, part_cells = 1, dw_cells = 1, dfeat_cells = 0, dacc_cells = 0;      // the running maxima; dfeat is the PointNet++ pass's, dacc (the f64 sum
                                                                                             // that travels from branch to branch) its multi-branch layers' (no cells: no room)
    Layout up, own, work;
    std::vector<Layout> per_layer;
    size_t total = 0;

    void layers(size_t nl, size_t more)
    {
        z.assign(nl, nullptr); y.assign(nl, nullptr); a.assign(nl, nullptr); stat.assign(nl, nullptr);
        per_layer.assign(nl + more, Layout());
    }
    void add_layer(size_t i, size_t M, const TLayer& Ly, uint32_t chunk_rows, bool with_a)
    {
        const size_t chunks = (M + chunk_rows - 1) / chunk_rows;
        Layout& L = per_layer[i];
        L.add(&z[i], M * Ly.N);
        L.add(&y[i], Ly.bn ? M * Ly.N : 0);
        L.add(&a[i], with_a && Ly.bn ? M * Ly.N : 0);
        L.add(&stat[i], 5 * (size_t)Ly.N);
        dy_cells = std::max(dy_cells, M * std::max(Ly.N, Ly.K));
        part_cells = std::max(part_cells, 2 * chunks * Ly.N);
        dw_cells = std::max(dw_cells, chunks * Ly.N * Ly.K);
    }
    void finish(size_t n_obj, uint32_t n_class, size_t n_loss)
    {
        upload_bytes = up.bytes();
        work.add(&dyA, dy_cells);
        work.add(&dyB, dy_cells);
        work.add(&dfeat, dfeat_cells);
        work.add(&dw_part, dw_cells);
        work.add(&part, part_cells);
        work.add(&logp, n_obj * n_class);
        work.add(&loss, n_loss);
        work.add(&dacc, dacc_cells);
        total = up.bytes() + own.bytes() + work.bytes();
        for (const Layout& L : per_layer) total += L.bytes();
    }
    void bind(void* base)
    {
        char* p = (char*)base;
        up.bind(p); p += up.bytes();
        own.bind(p); p += own.bytes();
        work.bind(p); p += work.bytes();
        for (Layout& L : per_layer) { L.bind(p); p += L.bytes(); }
    }
};

// the common head of a call: the argument checks in their order of precedence (own_bad: the caller's own finding or NULL, behind npts), the targets, the
// model's plan (make() -> what is wrong with it, or NULL), the device and the pinned block, `up` bound to the latter with the targets in it.
// run stays false where the call ends here: an error, or no objects
template <class MakePlan>
int call_head(pcr_ctx* ctx, const pcr_pn2_trainer* t, int kind, const char* who, const char* own_bad, bool null_arg, const int32_t* target, size_t n_obj, size_t npts,
              PlanBase& P, MakePlan make, bool& run, bool with_grad = true)
{
    run = false;
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str()); };
    if (!ctx || !t) return fail(ctx, PCR_ERR_ARG, who);
    if (t->kind != kind)
        return bad(kind == 0 ? ": the trainer was made by pcr_pn1_trainer_create (use pcr_pointnet_train_grad_f32 / _step_f32)"
                             : ": the trainer was made by pcr_pn2_trainer_create or pcr_pn2_msg_trainer_create (use pcr_pn2_train_grad_f32 / _step_f32)");
    if (t->device != ctx->device) return bad(": the trainer lives on another device");
    if (npts < 1) return bad(": npts must be >= 1");
    if (own_bad) return bad(own_bad);
    if (n_obj == 0) return PCR_OK;
    if (n_obj < 2) return bad(": BatchNorm's batch statistics need n_obj >= 2");
    if (null_arg) return bad(with_grad ? ": objects / target / loss / logp / grad is NULL" : ": objects / target / loss / logp is NULL");
    const uint32_t n_class = t->layers.back().N;
    for (size_t o = 0; o < n_obj; o++)
        if (target[o] < 0 || (uint32_t)target[o] >= n_class) return bad(": a target outside [0, n_class)");
    if (const char* what = make()) return bad(what);
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_scratch(ctx, P.total);
    if (rc) return rc;
    rc = ensure_stage(ctx, P.upload_bytes);
    if (rc) return rc;
    P.up.bind(ctx->host_stage);             // the uploaded part, laid out the same way in the pinned staging block
    for (size_t o = 0; o < n_obj; o++) P.target[o] = target[o];
    run = true;
    return PCR_OK;
}

// the staging block is full: the plan onto the scratch block, the upload, +0 into the gradient array (where the contract says so: pre-BN biases, the running
// statistics' slots)
inline int call_upload(pcr_ctx* ctx, pcr_pn2_trainer* t, PlanBase& P)
{
    P.bind(ctx->scratch);
    PCR_HIP(ctx, hipMemcpyAsync(ctx->scratch, ctx->host_stage, P.upload_bytes, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemsetAsync(t->grad_dev, 0, t->n_weights * 4, ctx->stream));
    return PCR_OK;
}

struct Download { void* dst; const void* src; size_t bytes; };      // dst NULL: not wanted

// the tail of a call: with step_lr the optimiser's update behind the pass's last kernel (only where the pass has no error); then logp, the n_loss loss doubles,
// the gradient array (grad NULL: it stays on the device) and `more` to the host, the one wait, rc before the HIP error
inline int call_tail(pcr_ctx* ctx, pcr_pn2_trainer* t, const char* who, int rc, const PlanBase& P, size_t n_obj, float* logp, double* loss, size_t n_loss, float* grad,
                     std::initializer_list<Download> more = {}, const double* step_lr = nullptr)
{
    hipError_t e = hipSuccess;
    if (rc == PCR_OK) {
        e = hipGetLastError();
        if (e == hipSuccess) {
            t->pass_ran = true;
            if (step_lr) rc = pcr::optim_launch(ctx, t, *step_lr, who);
        }
    }
    if (rc == PCR_OK) {
        if (e == hipSuccess) e = hipMemcpyAsync(logp, P.logp, n_obj * t->layers.back().N * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(loss, P.loss, n_loss * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && grad) e = hipMemcpyAsync(grad, t->grad_dev, t->n_weights * 4, hipMemcpyDeviceToHost, ctx->stream);
        for (const Download& d : more)
            if (e == hipSuccess && d.dst) e = hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);      // the one wait: the staging block (and the SSG pass's FPS jobs) are read until here
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, who, e != hipSuccess ? e : e2);
    prof_flush(ctx);
    return PCR_OK;
}

// what a layer is beyond its shapes.  The dropout of a layer sits nowhere, behind its ReLU (fused: bn_relu also writes a = y keep s, which the next layer
// reads, and the BatchNorm-backward kernels apply the same keep and s; the SSG head), or in front of its BatchNorm (pre_bn: in place on z and, backward, on dz,
// and the bias in front of the BatchNorm then has a gradient; pointnet_cls's head)
enum class Drop { none, fused, pre_bn };

// the RELU instances of the BatchNorm kernels
struct BnKernels {
    decltype(&pn2t_bn_relu_kernel<true>) bn_relu;
    decltype(&pn2t_bnb_part_kernel<true>) part;
    decltype(&pn2t_bnb_dz_kernel<true>) dz;
};
inline BnKernels bn_kernels(bool relu)
{
    if (relu) return { pn2t_bn_relu_kernel<true>, pn2t_bnb_part_kernel<true>, pn2t_bnb_dz_kernel<true> };
    return { pn2t_bn_relu_kernel<false>, pn2t_bnb_part_kernel<false>, pn2t_bnb_dz_kernel<false> };
}

// the product that takes z and dx: launch_gemm (one f32 chain) or pointnet_train.hip's launch_gemm1 (blocked over 64 k, f64 joins); DESIGN 8t has the reason
typedef int (*ProductFn)(pcr_ctx* ctx, const char* prof, const GemmArgs& g, const char* who);

// one call's launches, layer by layer.  Made once the plan is bound to the scratch block; after a failure (rc) every method returns at once
struct LayerRun {
    pcr_ctx* ctx;
    pcr_pn2_trainer* t;
    PlanBase& P;
    const char* who;
    ProductFn product;
    const char *prof_fwd, *prof_dx;
    const float* W;
    float* G;
    uint32_t chunk;
    float *cur, *nxt;        // the gradient that travels backward, and the block the next one is written to
    int rc = PCR_OK;

    LayerRun(pcr_ctx* c, pcr_pn2_trainer* tr, PlanBase& plan, const char* name, ProductFn f, const char* pf, const char* pd)
        : ctx(c), t(tr), P(plan), who(name), product(f), prof_fwd(pf), prof_dx(pd), W(tr->w_dev), G(tr->grad_dev), chunk(tr->chunk_rows), cur(plan.dyA), nxt(plan.dyB)
    {
    }

    uint32_t chunks_of(uint32_t M) const { return (M + chunk - 1) / chunk; }

    // the dropout scale of layer i: a head layer's own, 1 where there is no dropout
    float scale_of(uint32_t i, Drop drop) const
    {
        return drop != Drop::none && i >= t->head_first && i - t->head_first < PCR_PN2_MAX_FC ? t->drop_s[i - t->head_first] : 1.0f;
    }

    void dropout(float* v, const uint8_t* keep, float s, size_t cells)
    {
        ProfScope ps(ctx, "pn1t_dropout");
        hipLaunchKernelGGL(pn1t_dropout_kernel, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, v, keep, s, cells);
    }

    // z = x W^T + b (-> the pre_bn dropout) -> the statistics -> y = BN(z) with or without the ReLU (-> a, the fused dropout)
    void fwd(uint32_t i, const float* x, uint32_t M, bool relu, Drop drop = Drop::none, const uint8_t* keep = nullptr)
    {
        if (rc) return;
        const TLayer& L = t->layers[i];
        GemmArgs g;
        g.a = x; g.b = W + L.w; g.init = W + L.b; g.c = P.z[i];
        g.M = M; g.N = L.N; g.Kt = L.K; g.chunk = L.K;
        g.sai = L.K; g.sak = 1; g.sbk = 1; g.sbj = L.K; g.c_stride = 0;
        rc = product(ctx, prof_fwd, g, who);
        if (rc) return;
        const size_t cells = (size_t)M * L.N;
        if (drop == Drop::pre_bn) dropout(P.z[i], keep, scale_of(i, drop), cells);
        if (!L.bn) return;
        const uint32_t chunks = chunks_of(M);
        double *mu = P.stat[i], *var = mu + L.N, *rstd = var + L.N;
        {
            ProfScope ps(ctx, "pn2t_stat");
            for (int pass = 0; pass < 2; pass++) {
                hipLaunchKernelGGL(pn2t_stat_part_kernel, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, P.z[i], M, L.N, chunk, chunks,
                                   pass ? mu : (const double*)nullptr, P.part);
                hipLaunchKernelGGL(pn2t_stat_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, M, pass, mu, var, rstd, t->desc.bn_eps,
                                   t->momentum, t->w_dev + L.rmean, t->w_dev + L.rvar, (float*)nullptr);
            }
        }
        const bool fused = drop == Drop::fused;
        ProfScope ps(ctx, "pn2t_bn_relu");
        hipLaunchKernelGGL(bn_kernels(relu).bn_relu, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, P.z[i], cells, L.N, mu, rstd, W + L.gamma, W + L.beta, P.y[i],
                           fused ? keep : (const uint8_t*)nullptr, fused ? scale_of(i, drop) : 1.0f, fused ? P.a[i] : (float*)nullptr);
    }

    // the column sums of cur -> the bias gradient
    void bias_grad(const TLayer& L, uint32_t M)
    {
        const uint32_t chunks = chunks_of(M);
        ProfScope ps(ctx, "pn2t_stat");
        hipLaunchKernelGGL(pn2t_stat_part_kernel, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, cur, M, L.N, chunk, chunks, (const double*)nullptr,
                           P.part);
        hipLaunchKernelGGL(pn2t_stat_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, M, 2, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, 0.0, 0.0, (float*)nullptr, (float*)nullptr, G + L.b);
    }

    // cur holds the gradient at the layer's output (a, y, or z without BN) -> the parameter gradients; with need_dx, cur <- the gradient of x
    void bwd(uint32_t i, const float* x, uint32_t M, bool relu, bool need_dx, Drop drop = Drop::none, const uint8_t* keep = nullptr)
    {
        if (rc) return;
        const TLayer& L = t->layers[i];
        const size_t cells = (size_t)M * L.N;
        const uint32_t chunks = chunks_of(M);
        if (L.bn) {
            double *mu = P.stat[i], *rstd = mu + 2 * (size_t)L.N, *mg = mu + 3 * (size_t)L.N, *mgx = mu + 4 * (size_t)L.N;
            const uint8_t* fk = drop == Drop::fused ? keep : nullptr;
            const float s = fk ? scale_of(i, drop) : 1.0f;
            const BnKernels k = bn_kernels(relu);
            ProfScope ps(ctx, "pn2t_bn_back");
            hipLaunchKernelGGL(k.part, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], fk, s, M, L.N, chunk, chunks, mu, rstd, P.part);
            hipLaunchKernelGGL(pn2t_bnb_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, M, G + L.gamma, G + L.beta, mg, mgx);
            hipLaunchKernelGGL(k.dz, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], fk, s, cells, L.N, mu, rstd, W + L.gamma, mg, mgx);
        }
        if (drop == Drop::pre_bn) dropout(cur, keep, scale_of(i, drop), cells);
        if (!L.bn || drop == Drop::pre_bn) bias_grad(L, M);      // the biases the contract gives a gradient: no BatchNorm behind it, or a dropout in between
        {                                                        // dW[n][k] = sum_r dz[r][n] x[r][k]
            GemmArgs g;
            g.a = cur; g.b = x; g.init = nullptr; g.c = P.dw_part;
            g.M = L.N; g.N = L.K; g.Kt = M; g.chunk = chunk;
            g.sai = 1; g.sak = L.N; g.sbk = L.K; g.sbj = 1; g.c_stride = (size_t)L.N * L.K;
            rc = launch_gemm(ctx, "pn2t_gemm_dw", g, who);
            if (rc) return;
            ProfScope ps(ctx, "pn2t_dw_reduce");
            hipLaunchKernelGGL(pn2t_dw_reduce_kernel, dim3(blocks_for(g.c_stride)), dim3(T_BLOCK), 0, ctx->stream, P.dw_part, chunks, g.c_stride, G + L.w);
        }
        if (!need_dx) return;
        GemmArgs g;                                              // dx[r][k] = sum_n dz[r][n] W[n][k]
        g.a = cur; g.b = W + L.w; g.init = nullptr; g.c = nxt;
        g.M = M; g.N = L.K; g.Kt = L.N; g.chunk = L.N;
        g.sai = L.N; g.sak = 1; g.sbk = L.K; g.sbj = 1; g.c_stride = 0;
        rc = product(ctx, prof_dx, g, who);
        if (rc == PCR_OK) std::swap(cur, nxt);
    }

    // the gradient dfeat of the maxima of M rows in groups of gsize -> cur, the gradient of the rows.  dfeat may be cur: then the rows go to nxt and the two swap.
    // stride, off: the C columns are [off, off + C) of rows of `stride` cells in dfeat and arg (stride 0: the rows are the C columns)
    void max_back(const float* dfeat, const uint32_t* arg, uint32_t M, uint32_t gsize, uint32_t C, uint32_t stride = 0, uint32_t off = 0)
    {
        if (rc) return;
        float* dst = dfeat == cur ? nxt : cur;
        {
            ProfScope ps(ctx, "pn2t_max_back");
            hipLaunchKernelGGL(pn2t_max_back_kernel, dim3(blocks_for((size_t)M * C)), dim3(T_BLOCK), 0, ctx->stream, dfeat, arg, (size_t)M * C, gsize, C, stride ? stride : C, off,
                               dst);
        }
        if (dst == nxt) std::swap(cur, nxt);
    }
};

}  // namespace
