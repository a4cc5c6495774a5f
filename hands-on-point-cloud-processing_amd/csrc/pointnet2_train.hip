// pointnet2_train.hip — the training pass of HomeworkFinal's PointNet++ (SSG) classifier: training-mode forward, loss, the gradient of every
// parameter (models/pointnet2_cls_ssg.py, get_loss :50-52; train_cls.py's step without its optimiser).  The contract is written out above
// pcr_pn2_trainer_create in include/pcr.h.
//
// Batch statistics break the eval pass's layer fusion: the pass goes layer by layer and keeps every layer's z and y in HBM.
//   pn2t_gather        the padded rows of an SA layer: (xyz - centre | features) per row, and the point every row read
//   pn2t_gemm_fwd      z = x W^T + b        one wave = 32 rows x 64 outputs on v_mfma_f32_16x16x4_f32, the accumulators start at the bias; every
//   pn2t_gemm_dx       dx = dz W            MFMA takes four consecutive k, so an output is ONE fma chain over ascending k (channel, output or row)
//   pn2t_gemm_dw       dW partials = dz^T x one chain over the rows of a chunk per (chunk, output, input), from +0
//   pn2t_dw_reduce     dW = the chunk partials added in ascending order (f32)
//   pn2t_stat_part / pn2t_stat_fin     f64 sums per (chunk, channel) over ascending rows, then over ascending chunks: mean, variance (two passes),
//                      the running statistics; also the bias gradient of the last FC layer
//   pn2t_bn_relu       y = relu(BN(z)) and, in the head, the dropout
//   pn2t_max / pn2t_max_back            the max over a group with the lowest position among the maxima / its gradient
//   pn2t_bnb_part / pn2t_bnb_fin / pn2t_bnb_dz      dropout, ReLU and BatchNorm backward: dbeta, dgamma, then dz in place of dy
//   pn2t_gather_back   the gradient of a layer's input features summed per point over the rows that read it, rows ascending, in f64
//   pn2t_loss          log_softmax, the loss, dlogits
// No floating-point atomic anywhere; every sum over rows is ordered by the row index and chunk_rows alone.
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

// y = relu((z - mu) rstd gamma + beta), evaluated in f64 and rounded once; a (head) = y keep s
__global__ __launch_bounds__(T_BLOCK) void pn2t_bn_relu_kernel(const float* __restrict__ z, size_t total, uint32_t N, const double* __restrict__ mu,
                                                               const double* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ y, const uint8_t* __restrict__ keep, float s, float* __restrict__ a)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const uint32_t n = (uint32_t)(e % N);
    float v = (float)(((double)z[e] - mu[n]) * rstd[n] * (double)gamma[n] + (double)beta[n]);
    v = v > 0.0f ? v : 0.0f;
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

// the gradient that reaches BN's output at element e: dropout (the same mask and s), then ReLU (passes where y > 0)
__device__ __forceinline__ float pn2t_gy(const float* dy, const float* y, const uint8_t* keep, float s, size_t e)
{
    float g = dy[e];
    if (keep) g = keep[e] ? g * s : 0.0f;
    return y[e] > 0.0f ? g : 0.0f;
}

// part[c][0][n] <- sum gy, part[c][1][n] <- sum gy xhat over the rows of chunk c, ascending, in f64
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
        const double g = (double)pn2t_gy(dy, y, keep, s, e);
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
__global__ __launch_bounds__(T_BLOCK) void pn2t_bnb_dz_kernel(float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z, const uint8_t* __restrict__ keep,
                                                              float s, size_t total, uint32_t N, const double* __restrict__ mu, const double* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const double* __restrict__ mean_g, const double* __restrict__ mean_gx)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    const uint32_t n = (uint32_t)(e % N);
    const double g = (double)pn2t_gy(dy, y, keep, s, e);
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

struct pcr_pn2_trainer {
    pcr_pn2_desc desc;
    int device = 0;
    std::vector<TLayer> layers;          // weight order: the SA layers' convolutions, then the head
    uint32_t sa_first[PCR_PN2_MAX_SA];   // the first layer of every SA stage
    uint32_t sa_in[PCR_PN2_MAX_SA], sa_out[PCR_PN2_MAX_SA];
    uint32_t head_first = 0, n_sampling = 0;
    uint64_t n_weights = 0;
    float dropout_p = 0.0f, dropout_s = 1.0f;
    double momentum = 0.1;
    uint32_t chunk_rows = T_DEFAULT_CHUNK;
    float* w_dev = nullptr;              // the flat weight array, running statistics included
    float* grad_dev = nullptr;           // the same layout
};

namespace {

// the layers of a descriptor, or false for one outside the limits of pcr_pn2_model_create
bool trainer_shapes(const pcr_pn2_desc& d, pcr_pn2_trainer& t)
{
    if (d.n_sa < 1 || d.n_sa > PCR_PN2_MAX_SA || d.n_fc < 1 || d.n_fc > PCR_PN2_MAX_FC) return false;
    if (d.D0 > T_MAX_WIDTH - 3 || !std::isfinite(d.bn_eps)) return false;
    size_t off = 0;
    auto push = [&](uint32_t K, uint32_t N, bool bn) {
        TLayer L;
        L.K = K; L.N = N; L.bn = bn;
        L.w = off; off += (size_t)K * N;
        L.b = off; off += N;
        L.gamma = L.beta = L.rmean = L.rvar = 0;
        if (bn) { L.gamma = off; L.beta = off + N; L.rmean = off + 2 * (size_t)N; L.rvar = off + 3 * (size_t)N; off += 4 * (size_t)N; }
        t.layers.push_back(L);
    };
    uint32_t D = d.D0;
    t.n_sampling = 0;
    for (uint32_t l = 0; l < d.n_sa; l++) {
        const pcr_pn2_sa_desc& s = d.sa[l];
        if (s.group_all > 1 || (s.group_all && l + 1 != d.n_sa)) return false;
        if (s.n_mlp < 1 || s.n_mlp > PCR_PN2_MAX_MLP) return false;
        if (!s.group_all && (s.npoint < 1 || s.nsample < 1 || s.nsample > 65536 || !(s.radius >= 0.0) || std::isinf(s.radius))) return false;
        uint32_t K = 3 + D;
        if (K > T_MAX_WIDTH) return false;
        t.sa_first[l] = (uint32_t)t.layers.size();
        t.sa_in[l] = K;
        for (uint32_t i = 0; i < s.n_mlp; i++) {
            if (s.widths[i] < 1 || s.widths[i] > T_MAX_WIDTH) return false;
            push(K, s.widths[i], true);
            K = s.widths[i];
        }
        t.sa_out[l] = K;
        D = K;
        if (!s.group_all) t.n_sampling++;
    }
    t.head_first = (uint32_t)t.layers.size();
    uint32_t K = D;
    for (uint32_t i = 0; i < d.n_fc; i++) {
        if (d.fc_widths[i] < 1 || d.fc_widths[i] > T_MAX_WIDTH) return false;
        push(K, d.fc_widths[i], i + 1 < d.n_fc);
        K = d.fc_widths[i];
    }
    t.n_weights = off;
    return true;
}

const char* weights_ok(const pcr_pn2_trainer* t, const float* w)
{
    for (uint64_t i = 0; i < t->n_weights; i++)
        if (!std::isfinite(w[i])) return ": a non-finite weight";
    for (const TLayer& L : t->layers)
        if (L.bn)
            for (uint32_t n = 0; n < L.N; n++)
                if (!((double)w[L.rvar + n] + t->desc.bn_eps > 0.0)) return ": running_var + eps must be positive";
    return nullptr;
}

// the stages of one call: every SA layer, then the head
struct Stage {
    uint32_t first, count;       // its layers
    uint32_t M;                  // rows
    uint32_t gsize;              // rows per group (head: 0, no max)
    uint32_t groups;
};

// the device block of one call.  Several Layouts (scratch_layout.hpp holds 24 slots each) laid one behind the other.
struct Plan {
    size_t N[PCR_PN2_MAX_SA + 1];
    std::vector<Stage> stages;
    // uploaded
    float *x0 = nullptr, *feat0 = nullptr;
    int32_t* target = nullptr;
    uint8_t* keep = nullptr;
    uint32_t *seg[PCR_PN2_MAX_SA + 1], *cseg[PCR_PN2_MAX_SA];
    size_t upload_bytes = 0;
    // sampling
    uint32_t *fps[PCR_PN2_MAX_SA], *bidx[PCR_PN2_MAX_SA], *bcnt[PCR_PN2_MAX_SA];
    float* cxyz[PCR_PN2_MAX_SA];
    // per SA stage
    float *xin[PCR_PN2_MAX_SA], *feat[PCR_PN2_MAX_SA];
    uint32_t *row_pt[PCR_PN2_MAX_SA], *arg[PCR_PN2_MAX_SA];
    // per layer
    std::vector<float*> z, y, a;
    std::vector<double*> stat;       // 5 N doubles: mu, var, rstd, mean_g, mean_gx
    // shared
    float *dyA = nullptr, *dyB = nullptr, *dfeat = nullptr, *dw_part = nullptr, *logp = nullptr;
    double *part = nullptr, *loss = nullptr;
    Layout up, samp, work;
    std::vector<Layout> per_layer;
    size_t total = 0;

    void bind(void* base)
    {
        char* p = (char*)base;
        up.bind(p); p += up.bytes();
        samp.bind(p); p += samp.bytes();
        work.bind(p); p += work.bytes();
        for (Layout& L : per_layer) { L.bind(p); p += L.bytes(); }
    }
};

// false: too large
bool make_plan(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, Plan& P)
{
    const pcr_pn2_desc& d = t->desc;
    const uint32_t ns = t->n_sampling, C0 = 3 + d.D0;
    if (n_obj > T_MAX_ROWS || npts > T_MAX_ROWS || (unsigned long long)n_obj * npts > T_MAX_ROWS / C0) return false;
    P.N[0] = npts;
    for (uint32_t l = 0; l < ns; l++) {
        P.N[l + 1] = d.sa[l].npoint;
        const unsigned long long rows = (unsigned long long)n_obj * d.sa[l].npoint * d.sa[l].nsample;
        if (rows > T_MAX_ROWS / T_MAX_WIDTH) return false;
        P.stages.push_back({ t->sa_first[l], d.sa[l].n_mlp, (uint32_t)rows, d.sa[l].nsample, (uint32_t)(n_obj * d.sa[l].npoint) });
    }
    if (d.sa[d.n_sa - 1].group_all) {
        const unsigned long long rows = (unsigned long long)n_obj * P.N[ns];
        if (rows > T_MAX_ROWS / T_MAX_WIDTH) return false;
        P.stages.push_back({ t->sa_first[ns], d.sa[ns].n_mlp, (uint32_t)rows, (uint32_t)P.N[ns], (uint32_t)n_obj });
    }
    P.stages.push_back({ t->head_first, d.n_fc, (uint32_t)n_obj, 0u, (uint32_t)n_obj });
    const size_t pts = n_obj * npts;
    size_t keep_bytes = 0;
    for (uint32_t i = 0; i + 1 < d.n_fc; i++) keep_bytes += n_obj * d.fc_widths[i];
    P.up.add(&P.x0, 3 * pts);
    P.up.add(&P.feat0, pts * d.D0);
    P.up.add(&P.target, n_obj);
    P.up.add(&P.keep, keep_bytes);
    for (uint32_t l = 0; l <= ns; l++) P.up.add(&P.seg[l], n_obj + 1);
    for (uint32_t l = 0; l < ns; l++) P.up.add(&P.cseg[l], n_obj * P.N[l + 1]);
    P.upload_bytes = P.up.bytes();
    for (uint32_t l = 0; l < ns; l++) {
        const size_t nq = n_obj * P.N[l + 1];
        P.samp.add(&P.fps[l], nq);
        P.samp.add(&P.cxyz[l], 3 * nq);
        P.samp.add(&P.bidx[l], nq * d.sa[l].nsample);
        P.samp.add(&P.bcnt[l], nq);
    }
    const size_t nl = t->layers.size();
    P.z.assign(nl, nullptr); P.y.assign(nl, nullptr); P.a.assign(nl, nullptr); P.stat.assign(nl, nullptr);
    P.per_layer.assign(nl + d.n_sa, Layout());
    size_t dy_cells = 1, part_cells = 1, dw_cells = 1, dfeat_cells = 1;
    for (size_t s = 0; s < P.stages.size(); s++) {
        const Stage& st = P.stages[s];
        const uint32_t chunks = (st.M + t->chunk_rows - 1) / t->chunk_rows;
        const bool head = st.gsize == 0;
        if (!head) {
            Layout& L = P.per_layer[nl + s];
            L.add(&P.xin[s], (size_t)st.M * t->sa_in[s]);
            L.add(&P.row_pt[s], (size_t)st.M);
            L.add(&P.feat[s], (size_t)st.groups * t->sa_out[s]);
            L.add(&P.arg[s], (size_t)st.groups * t->sa_out[s]);
            dfeat_cells = std::max(dfeat_cells, (size_t)st.groups * t->sa_out[s]);
        }
        for (uint32_t i = st.first; i < st.first + st.count; i++) {
            const TLayer& Ly = t->layers[i];
            Layout& L = P.per_layer[i];
            L.add(&P.z[i], (size_t)st.M * Ly.N);
            L.add(&P.y[i], Ly.bn ? (size_t)st.M * Ly.N : 0);
            L.add(&P.a[i], head && Ly.bn ? (size_t)st.M * Ly.N : 0);
            L.add(&P.stat[i], 5 * (size_t)Ly.N);
            dy_cells = std::max(dy_cells, (size_t)st.M * std::max(Ly.N, Ly.K));
            part_cells = std::max(part_cells, 2 * (size_t)chunks * Ly.N);
            dw_cells = std::max(dw_cells, (size_t)chunks * Ly.N * Ly.K);
        }
    }
    P.work.add(&P.dyA, dy_cells);
    P.work.add(&P.dyB, dy_cells);
    P.work.add(&P.dfeat, dfeat_cells);
    P.work.add(&P.dw_part, dw_cells);
    P.work.add(&P.part, part_cells);
    P.work.add(&P.logp, n_obj * t->layers.back().N);
    P.work.add(&P.loss, (size_t)1);
    P.total = P.up.bytes() + P.samp.bytes() + P.work.bytes();
    for (const Layout& L : P.per_layer) P.total += L.bytes();
    return true;
}

int launch_gemm(pcr_ctx* ctx, const char* prof, GemmArgs g)
{
    if (g.M == 0 || g.N == 0) return PCR_OK;
    const uint32_t chunks = g.Kt == 0 ? 1u : (g.Kt + g.chunk - 1) / g.chunk;
    if (chunks > 65535u) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_train_grad_f32: more than 65535 chunks of rows (raise chunk_rows)");
    ProfScope ps(ctx, prof);
    hipLaunchKernelGGL(pn2t_gemm_kernel, dim3((g.M + T_ROWS - 1) / T_ROWS, (g.N + 63) / 64, chunks), dim3(T_BLOCK), 0, ctx->stream, g);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

}  // namespace

extern "C" int pcr_pn2_trainer_create(pcr_ctx* ctx, const pcr_pn2_desc* desc, const float* weights, size_t n_weights, double dropout_p, double bn_momentum,
                                      uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create");
    std::unique_ptr<pcr_pn2_trainer> t(new pcr_pn2_trainer());
    t->desc = *desc;
    if (!trainer_shapes(*desc, *t)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: a descriptor outside the limits (see include/pcr.h)");
    if (!desc->sa[desc->n_sa - 1].group_all) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: the last SA layer must be group_all");
    if (!(dropout_p >= 0.0 && dropout_p < 1.0)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: dropout_p must lie in [0, 1)");
    if (!(bn_momentum >= 0.0 && bn_momentum <= 1.0)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: bn_momentum must lie in [0, 1]");
    if (n_weights != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: n_weights is not the model's count");
    if (const char* what = weights_ok(t.get(), weights)) return fail(ctx, PCR_ERR_ARG, (std::string("pcr_pn2_trainer_create") + what).c_str());
    t->dropout_p = (float)dropout_p;
    t->dropout_s = (float)(1.0 / (1.0 - dropout_p));
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
        return fail(ctx, PCR_ERR_HIP, "pcr_pn2_trainer_create: the upload of the weights", e);
    }
    *out = t.release();
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_destroy(pcr_ctx* ctx, pcr_pn2_trainer* t)
{
    if (!t) return PCR_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (t->w_dev) (void)hipFree(t->w_dev);
    if (t->grad_dev) (void)hipFree(t->grad_dev);
    delete t;
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_info(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, pcr_pn2_train_info* info)
{
    if (!t || !info) return PCR_ERR_ARG;
    memset(info, 0, sizeof(*info));
    info->n_weights = t->n_weights;
    info->chunk_rows = t->chunk_rows;
    info->n_class = t->layers.back().N;
    info->n_sampling = t->n_sampling;
    for (uint32_t i = 0; i + 1 < t->desc.n_fc; i++) info->keep_per_object += t->desc.fc_widths[i];
    info->dropout_p = (double)t->dropout_p;
    info->bn_momentum = t->momentum;
    if (n_obj && npts) {
        Plan P;
        if (!make_plan(t, n_obj, npts, P)) return PCR_ERR_ARG;
        info->device_bytes = P.total + 2 * t->n_weights * 4;
    }
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_set_weights(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* weights, size_t n, int keep_running_stats)
{
    if (!ctx || !t || !weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_set_weights");
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_set_weights: the trainer lives on another device");
    if (n != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_set_weights: n is not the model's count");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!keep_running_stats) {
        if (const char* what = weights_ok(t, weights)) return fail(ctx, PCR_ERR_ARG, (std::string("pcr_pn2_trainer_set_weights") + what).c_str());
        PCR_HIP(ctx, hipMemcpy(t->w_dev, weights, n * 4, hipMemcpyHostToDevice));
        return PCR_OK;
    }
    std::vector<float> w(weights, weights + n), cur(n);
    PCR_HIP(ctx, hipMemcpy(cur.data(), t->w_dev, n * 4, hipMemcpyDeviceToHost));
    for (const TLayer& L : t->layers)
        if (L.bn) std::copy(cur.begin() + L.rmean, cur.begin() + L.rmean + 2 * (size_t)L.N, w.begin() + L.rmean);      // running_mean and running_var lie side by side
    if (const char* what = weights_ok(t, w.data())) return fail(ctx, PCR_ERR_ARG, (std::string("pcr_pn2_trainer_set_weights") + what).c_str());
    PCR_HIP(ctx, hipMemcpy(t->w_dev, w.data(), n * 4, hipMemcpyHostToDevice));
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_get_weights(pcr_ctx* ctx, const pcr_pn2_trainer* t, float* weights, size_t n)
{
    if (!ctx || !t || !weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_weights");
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_weights: the trainer lives on another device");
    if (n != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_weights: n is not the model's count");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCR_HIP(ctx, hipMemcpy(weights, t->w_dev, n * 4, hipMemcpyDeviceToHost));
    return PCR_OK;
}

extern "C" int pcr_pn2_train_grad_f32(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* objects, size_t n_obj, size_t npts, const int32_t* target, const uint32_t* starts,
                                      uint64_t seed, const uint8_t* keep, double* loss, float* logp, float* grad)
{
    const char* who = "pcr_pn2_train_grad_f32";
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str()); };
    if (!ctx || !t) return fail(ctx, PCR_ERR_ARG, who);
    if (t->device != ctx->device) return bad(": the trainer lives on another device");
    if (npts < 1) return bad(": npts must be >= 1");
    if (n_obj == 0) return PCR_OK;
    if (n_obj < 2) return bad(": BatchNorm's batch statistics need n_obj >= 2");
    if (!objects || !target || !loss || !logp || !grad) return bad(": objects / target / loss / logp / grad is NULL");
    const pcr_pn2_desc& d = t->desc;
    const uint32_t ns = t->n_sampling, D0 = d.D0, C0 = 3 + D0, n_class = t->layers.back().N;
    for (size_t o = 0; o < n_obj; o++)
        if (target[o] < 0 || (uint32_t)target[o] >= n_class) return bad(": a target outside [0, n_class)");
    Plan P;
    if (!make_plan(t, n_obj, npts, P)) return bad(": too large");
    for (const Stage& st : P.stages)
        if (st.M < 2) return bad(": a layer with one row (BatchNorm's batch statistics need two)");
    std::vector<uint32_t> st0((size_t)ns * n_obj);
    for (uint32_t l = 0; l < ns; l++)
        for (size_t o = 0; o < n_obj; o++) {
            uint32_t v;
            if (starts) {
                v = starts[(size_t)l * n_obj + o];
                if (v >= P.N[l]) return bad(": a start outside its object");
            } else {
                v = (uint32_t)(splitmix_key(seed, ((unsigned long long)(l + 1) << 32) | (unsigned long long)o) % (unsigned long long)P.N[l]);
            }
            st0[(size_t)l * n_obj + o] = v;
        }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_scratch(ctx, P.total);
    if (rc) return rc;
    rc = ensure_stage(ctx, P.upload_bytes);
    if (rc) return rc;
    const size_t pts = n_obj * npts;
    P.up.bind(ctx->host_stage);             // the uploaded part, laid out the same way in the pinned staging block
    {
        float *hx = P.x0, *hy = P.x0 + pts, *hz = P.x0 + 2 * pts;
        for (size_t i = 0; i < pts; i++) {
            const float* r = objects + i * C0;
            for (uint32_t c = 0; c < C0; c++)
                if (!(fabsf(r[c]) <= FLT_MAX)) return bad(": a non-finite coordinate or feature");
            hx[i] = r[0]; hy[i] = r[1]; hz[i] = r[2];
            for (uint32_t c = 0; c < D0; c++) P.feat0[i * D0 + c] = r[3 + c];
        }
        for (size_t o = 0; o < n_obj; o++) P.target[o] = target[o];
        size_t off = 0;
        for (uint32_t i = 0; i + 1 < d.n_fc; i++) {              // the masks: the caller's bytes, or K(seed, (0x100 + layer) << 32 | cell) as a uniform in [0, 1) >= p
            const size_t cells = n_obj * d.fc_widths[i];
            for (size_t e = 0; e < cells; e++) {
                uint8_t k;
                if (keep) k = keep[off + e] ? 1 : 0;
                else k = (double)(splitmix_key(seed, ((unsigned long long)(0x100u + i) << 32) | (unsigned long long)e) >> 11) * 0x1.0p-53 >= (double)t->dropout_p ? 1 : 0;
                P.keep[off + e] = k;
            }
            off += cells;
        }
        for (uint32_t l = 0; l <= ns; l++)
            for (size_t o = 0; o <= n_obj; o++) P.seg[l][o] = (uint32_t)(o * P.N[l]);
        for (uint32_t l = 0; l < ns; l++)
            for (size_t q = 0; q < n_obj * P.N[l + 1]; q++) P.cseg[l][q] = (uint32_t)(q / P.N[l + 1]);
    }
    P.bind(ctx->scratch);
    PCR_HIP(ctx, hipMemcpyAsync(ctx->scratch, ctx->host_stage, P.upload_bytes, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemsetAsync(t->grad_dev, 0, t->n_weights * 4, ctx->stream));      // +0 where the contract says so: pre-BN biases, the running statistics' slots
    const float *W = t->w_dev;
    float* G = t->grad_dev;
    const uint32_t chunk = t->chunk_rows;
    const float drop_s = t->dropout_s;
    HostKeep hold;
    // ---- forward
    const float *cx = P.x0, *cy = P.x0 + pts, *cz = P.x0 + 2 * pts, *feat = P.feat0;
    uint32_t D = D0;
    size_t keep_off = 0;
    std::vector<const uint8_t*> keep_of(t->layers.size(), nullptr);
    for (size_t s = 0; s < P.stages.size() && rc == PCR_OK; s++) {
        const Stage& st = P.stages[s];
        const bool head = st.gsize == 0;
        const float* x = nullptr;
        if (!head) {
            const bool grouped = s < ns;
            const float *qx = nullptr, *qy = nullptr, *qz = nullptr;
            if (grouped) {
                const pcr_pn2_sa_desc& sd = d.sa[s];
                const size_t nq = n_obj * P.N[s + 1];
                std::vector<FpsJob> jobs(n_obj);
                for (size_t o = 0; o < n_obj; o++) jobs[o] = { (uint32_t)(o * P.N[s]), (uint32_t)P.N[s], st0[s * n_obj + o], (uint32_t)o };
                rc = fps_device(ctx, cx, cy, cz, std::move(jobs), sd.npoint, PCR_FPS_F32, P.fps[s], &hold);
                if (rc) break;
                float *wx = P.cxyz[s], *wy = wx + nq, *wz = wy + nq;
                {
                    ProfScope ps(ctx, "pn2t_centres");
                    hipLaunchKernelGGL(pn2t_centres_kernel, dim3(blocks_for(nq)), dim3(T_BLOCK), 0, ctx->stream, cx, cy, cz, P.fps[s], (uint32_t)P.N[s], sd.npoint, (uint32_t)nq,
                                       wx, wy, wz);
                }
                rc = ball_query_device(ctx, cx, cy, cz, wx, wy, wz, P.seg[s], P.cseg[s], nq, sd.radius, sd.nsample, P.bidx[s], P.bcnt[s]);
                if (rc) break;
                qx = wx; qy = wy; qz = wz;
            }
            {
                ProfScope ps(ctx, "pn2t_gather");
                hipLaunchKernelGGL(pn2t_gather_kernel, dim3(blocks_for(st.M)), dim3(T_BLOCK), 0, ctx->stream, cx, cy, cz, qx, qy, qz, feat, grouped ? P.bidx[s] : nullptr, st.M,
                                   grouped ? d.sa[s].nsample : 1u, grouped ? d.sa[s].npoint : 1u, (uint32_t)P.N[s], D, P.xin[s], P.row_pt[s]);
            }
            x = P.xin[s];
            if (grouped) { cx = qx; cy = qy; cz = qz; }
        } else {
            x = feat;
        }
        const uint32_t chunks = (st.M + chunk - 1) / chunk;
        for (uint32_t i = st.first; i < st.first + st.count && rc == PCR_OK; i++) {
            const TLayer& L = t->layers[i];
            GemmArgs g;
            g.a = x; g.b = W + L.w; g.init = W + L.b; g.c = P.z[i];
            g.M = st.M; g.N = L.N; g.Kt = L.K; g.chunk = L.K;
            g.sai = L.K; g.sak = 1; g.sbk = 1; g.sbj = L.K; g.c_stride = 0;
            rc = launch_gemm(ctx, "pn2t_gemm_fwd", g);
            if (rc || !L.bn) break;
            double *mu = P.stat[i], *var = mu + L.N, *rstd = var + L.N;
            const size_t cells = (size_t)st.M * L.N;
            {
                ProfScope ps(ctx, "pn2t_stat");
                for (int pass = 0; pass < 2; pass++) {
                    hipLaunchKernelGGL(pn2t_stat_part_kernel, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, P.z[i], st.M, L.N, chunk, chunks,
                                       pass ? mu : (const double*)nullptr, P.part);
                    hipLaunchKernelGGL(pn2t_stat_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, st.M, pass, mu, var, rstd, d.bn_eps,
                                       t->momentum, t->w_dev + L.rmean, t->w_dev + L.rvar, (float*)nullptr);
                }
            }
            const uint8_t* kp = nullptr;
            if (head) {
                kp = P.keep + keep_off;
                keep_off += cells;
                keep_of[i] = kp;
            }
            {
                ProfScope ps(ctx, "pn2t_bn_relu");
                hipLaunchKernelGGL(pn2t_bn_relu_kernel, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, P.z[i], cells, L.N, mu, rstd, W + L.gamma, W + L.beta, P.y[i], kp,
                                   drop_s, head ? P.a[i] : (float*)nullptr);
            }
            x = head ? P.a[i] : P.y[i];
        }
        if (rc) break;
        if (!head) {
            const uint32_t last = st.first + st.count - 1, C = t->layers[last].N;
            ProfScope ps(ctx, "pn2t_max");
            hipLaunchKernelGGL(pn2t_max_kernel, dim3(blocks_for((size_t)st.groups * C)), dim3(T_BLOCK), 0, ctx->stream, P.y[last], st.groups, st.gsize, C, P.feat[s], P.arg[s]);
            feat = P.feat[s];
            D = C;
        }
    }
    // ---- the loss, then backward
    float *cur = P.dyA, *nxt = P.dyB;
    if (rc == PCR_OK) {
        ProfScope ps(ctx, "pn2t_loss");
        hipLaunchKernelGGL(pn2t_loss_kernel, dim3(1), dim3(T_BLOCK), 0, ctx->stream, P.z[t->layers.size() - 1], P.target, (uint32_t)n_obj, n_class, P.logp, cur, P.loss);
    }
    for (size_t s = P.stages.size(); s-- > 0 && rc == PCR_OK;) {
        const Stage& st = P.stages[s];
        const bool head = st.gsize == 0;
        const uint32_t chunks = (st.M + chunk - 1) / chunk;
        if (!head) {                                             // the gradient of the stage's output -> its last layer's rows
            const uint32_t last = st.first + st.count - 1, C = t->layers[last].N;
            const float* dfeat = P.dfeat;
            float* dst = cur;
            if (s + 1 == P.stages.size() - 1) { dfeat = cur; dst = nxt; }      // below the head: the head's dx IS the gradient of the global feature
            {
                ProfScope ps(ctx, "pn2t_max_back");
                hipLaunchKernelGGL(pn2t_max_back_kernel, dim3(blocks_for((size_t)st.M * C)), dim3(T_BLOCK), 0, ctx->stream, dfeat, P.arg[s], (size_t)st.M * C, st.gsize, C, dst);
            }
            if (dst == nxt) std::swap(cur, nxt);
        }
        for (uint32_t i = st.first + st.count; i-- > st.first && rc == PCR_OK;) {
            const TLayer& L = t->layers[i];
            const size_t cells = (size_t)st.M * L.N;
            const float* x = i > st.first ? (head ? P.a[i - 1] : P.y[i - 1]) : (head ? P.feat[s - 1] : P.xin[s]);
            if (L.bn) {
                double *mu = P.stat[i], *rstd = mu + 2 * (size_t)L.N, *mg = mu + 3 * (size_t)L.N, *mgx = mu + 4 * (size_t)L.N;
                ProfScope ps(ctx, "pn2t_bn_back");
                hipLaunchKernelGGL(pn2t_bnb_part_kernel, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], keep_of[i], drop_s, st.M, L.N,
                                   chunk, chunks, mu, rstd, P.part);
                hipLaunchKernelGGL(pn2t_bnb_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, st.M, G + L.gamma, G + L.beta, mg, mgx);
                hipLaunchKernelGGL(pn2t_bnb_dz_kernel, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], keep_of[i], drop_s, cells, L.N, mu, rstd,
                                   W + L.gamma, mg, mgx);
            } else {                                             // the last FC layer: its bias has a gradient, the column sums of dz
                ProfScope ps(ctx, "pn2t_stat");
                hipLaunchKernelGGL(pn2t_stat_part_kernel, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, cur, st.M, L.N, chunk, chunks,
                                   (const double*)nullptr, P.part);
                hipLaunchKernelGGL(pn2t_stat_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, st.M, 2, (double*)nullptr, (double*)nullptr,
                                   (double*)nullptr, 0.0, 0.0, (float*)nullptr, (float*)nullptr, G + L.b);
            }
            {                                                    // dW[n][k] = sum_r dz[r][n] x[r][k]
                GemmArgs g;
                g.a = cur; g.b = x; g.init = nullptr; g.c = P.dw_part;
                g.M = L.N; g.N = L.K; g.Kt = st.M; g.chunk = chunk;
                g.sai = 1; g.sak = L.N; g.sbk = L.K; g.sbj = 1; g.c_stride = (size_t)L.N * L.K;
                rc = launch_gemm(ctx, "pn2t_gemm_dw", g);
                if (rc) break;
                ProfScope ps(ctx, "pn2t_dw_reduce");
                hipLaunchKernelGGL(pn2t_dw_reduce_kernel, dim3(blocks_for(g.c_stride)), dim3(T_BLOCK), 0, ctx->stream, P.dw_part, chunks, g.c_stride, G + L.w);
            }
            if (i == 0) break;                                   // the input points take no gradient
            {                                                    // dx[r][k] = sum_n dz[r][n] W[n][k]
                GemmArgs g;
                g.a = cur; g.b = W + L.w; g.init = nullptr; g.c = nxt;
                g.M = st.M; g.N = L.K; g.Kt = L.N; g.chunk = L.N;
                g.sai = L.N; g.sak = 1; g.sbk = L.K; g.sbj = 1; g.c_stride = 0;
                rc = launch_gemm(ctx, "pn2t_gemm_dx", g);
                if (rc) break;
                std::swap(cur, nxt);
            }
        }
        if (rc == PCR_OK && !head && s > 0) {                    // the feature columns of dx back to the points of the stage before
            const uint32_t Dp = t->sa_in[s] - 3;
            const uint32_t points = (uint32_t)(n_obj * P.N[s]);
            ProfScope ps(ctx, "pn2t_gather_back");
            hipLaunchKernelGGL(pn2t_gather_back_kernel, dim3(points), dim3(T_BLOCK), 0, ctx->stream, cur, P.row_pt[s], points, (uint32_t)P.N[s], st.M / (uint32_t)n_obj, Dp, P.dfeat);
        }
    }
    hipError_t e = hipSuccess;
    if (rc == PCR_OK) {
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(logp, P.logp, n_obj * n_class * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(loss, P.loss, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(grad, G, t->n_weights * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);      // the one wait: `hold` and the staging block are read until here
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, who, e != hipSuccess ? e : e2);
    prof_flush(ctx);
    return PCR_OK;
}
