// pointnet_train_common.hpp — what the two training passes share (pointnet2_train.hip: PointNet++ SSG; pointnet_train.hip: the vanilla PointNet): the strided
// MFMA product, the chunked f64 statistics, BatchNorm / ReLU forward and backward, the max with its argmax, the loss kernel and the trainer handle.
// Every kernel here keeps its pn2t_* profile name in both passes.  The contracts are above pcr_pn2_trainer_create and pcr_pn1_trainer_create in include/pcr.h.
#pragma once
#include "pcr_internal.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

using namespace pcr;

namespace {

constexpr int T_BLOCK = 256;
constexpr uint32_t T_MAX_WIDTH = 1024;
constexpr unsigned long long T_MAX_ROWS = 0x7FFFFFF0ull;
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

// the rows of an SA layer.  grouped: row r = (centre q = r / nsample, member k = r % nsample) reads point idx[q][k] of its object;
// group_all (idx == NULL): row r is point r.  x[r] = (xyz - centre | features), row_pt[r] = the point (T_NONE: a member outside its object, a row of zeros)
__global__ __launch_bounds__(T_BLOCK) void pn2t_gather_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                              const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                              const float* __restrict__ feat, const uint32_t* __restrict__ idx, uint32_t rows, uint32_t nsample,
                                                              uint32_t npoint, uint32_t n_prev, uint32_t D, float* __restrict__ x, uint32_t* __restrict__ row_pt)
{
    const uint32_t r = blockIdx.x * T_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const uint32_t K = 3 + D;
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
    xr[0] = sub ? px[p] - cx : px[p];
    xr[1] = sub ? py[p] - cy : py[p];
    xr[2] = sub ? pz[p] - cz : pz[p];
    for (uint32_t c = 0; c < D; c++) xr[3 + c] = feat[(size_t)p * D + c];
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

// feat[g][c] = the max over the gsize rows of group g; arg[g][c] = the lowest position that holds it, T_NONE where the max is 0
__global__ __launch_bounds__(T_BLOCK) void pn2t_max_kernel(const float* __restrict__ y, uint32_t groups, uint32_t gsize, uint32_t N, float* __restrict__ feat,
                                                           uint32_t* __restrict__ arg)
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
    feat[e] = m;
    arg[e] = m > 0.0f ? best : T_NONE;
}

__global__ __launch_bounds__(T_BLOCK) void pn2t_max_back_kernel(const float* __restrict__ dfeat, const uint32_t* __restrict__ arg, size_t total, uint32_t gsize, uint32_t N,
                                                                float* __restrict__ dy)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const size_t r = e / N;
    const uint32_t c = (uint32_t)(e - r * N);
    const size_t g = r / gsize;
    const uint32_t k = (uint32_t)(r - g * gsize);
    dy[e] = arg[g * N + c] == k ? dfeat[g * N + c] : 0.0f;
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

// dfeat[p][c] <- the f64 sum, rows ascending, of dx[r][3 + c] over the rows r of p's object that read point p; rounded once
__global__ __launch_bounds__(T_BLOCK) void pn2t_gather_back_kernel(const float* __restrict__ dx, const uint32_t* __restrict__ row_pt, uint32_t points, uint32_t n_prev,
                                                                   uint32_t rows_per_obj, uint32_t D, float* __restrict__ dfeat)
{
    const uint32_t p = blockIdx.x;                              // one workgroup per point: row_pt is read uniformly
    if (p >= points) return;
    const uint32_t o = p / n_prev, K = 3 + D;
    const size_t r0 = (size_t)o * rows_per_obj;
    for (uint32_t c = threadIdx.x; c < D; c += T_BLOCK) {
        double s = 0.0;
        for (uint32_t k = 0; k < rows_per_obj; k++)
            if (row_pt[r0 + k] == p) s = s + (double)dx[(r0 + k) * K + 3 + c];
        dfeat[(size_t)p * D + c] = (float)s;
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

inline unsigned blocks_for(size_t n) { return (unsigned)((n + T_BLOCK - 1) / T_BLOCK); }

}  // namespace

// the handle of both trainers.  kind 0: pcr_pn2_trainer_create (desc, sa_*, head_first, n_sampling); kind 1: pcr_pn1_trainer_create (desc1, the
// first layer of its five parts, reg_scale; desc.bn_eps mirrors desc1.bn_eps)
struct pcr_pn2_trainer {
    pcr_pn2_desc desc;
    int device = 0;
    std::vector<TLayer> layers;          // weight order
    uint32_t sa_first[PCR_PN2_MAX_SA];   // the first layer of every SA stage
    uint32_t sa_in[PCR_PN2_MAX_SA], sa_out[PCR_PN2_MAX_SA];
    uint32_t head_first = 0, n_sampling = 0;
    uint64_t n_weights = 0;
    float dropout_p = 0.0f, dropout_s = 1.0f;
    double momentum = 0.1;
    uint32_t chunk_rows = T_DEFAULT_CHUNK;
    float* w_dev = nullptr;              // the flat weight array, running statistics included
    float* grad_dev = nullptr;           // the same layout
    int kind = 0;
    pcr_pn1_desc desc1;
    uint32_t stn_first = 0, enc_first = 0, fstn_first = 0;      // kind 1: [stn3's six layers] [the encoder] [fstn's six layers] [the head at head_first]
    double reg_scale = 0.0;
};

namespace pcr {
// pcr_pn2_trainer_info for a kind-1 trainer (pointnet_train.hip)
int pn1_trainer_info(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, pcr_pn2_train_info* info);
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

inline int launch_gemm(pcr_ctx* ctx, const char* prof, GemmArgs g, const char* who = "pcr_pn2_train_grad_f32")
{
    if (g.M == 0 || g.N == 0) return PCR_OK;
    const uint32_t chunks = g.Kt == 0 ? 1u : (g.Kt + g.chunk - 1) / g.chunk;
    if (chunks > 65535u) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": more than 65535 chunks of rows (raise chunk_rows)").c_str());
    ProfScope ps(ctx, prof);
    hipLaunchKernelGGL(pn2t_gemm_kernel, dim3((g.M + T_ROWS - 1) / T_ROWS, (g.N + 63) / 64, chunks), dim3(T_BLOCK), 0, ctx->stream, g);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

}  // namespace
