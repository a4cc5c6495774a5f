// spectral.hip — Homework3's third algorithm: spectral clustering (Homework3/hw3/spectralClustering.cpp) on the GPU.  Contracts: include/pcr.h;
// design and measurements: DESIGN §8n.
//
//   kNN            sp_knn_kernel: exhaustive and tiled.  A lane owns one row, the targets pass through LDS in ascending index order and the lane keeps
//                  its k best in registers, ordered by (d2, index) — a later target with an equal d2 has the larger index and stays behind.
//   graph          sp_graph_kernel: a lane turns its row of the kNN result into a row of L = I - D^-1 W with ascending columns.
//   embedding      block iteration X <- (I - L / 2) X on n x 16 row-major blocks (n_basis <= 16 columns in use, the others stay zero), Cholesky-QR
//                  every SP_STEPS steps, and every SP_ROUNDS rounds a Rayleigh-Ritz step: T = Q^T L Q to the host, its eigenpairs back, the Ritz
//                  vectors V = Q Y and the residual L V - V Theta on the device.
//                  n <= 4 096: sp_iterate_one_kernel, ONE workgroup of 1 024 lanes, runs all the steps and factorizations between two checks; its
//                  lanes meet at workgroup barriers only.  Larger n: one launch per step (sp_axpy_kernel), per Gram matrix (sp_gram_kernel +
//                  sp_chol_kernel) and per basis change (sp_apply_kernel), in stream order.  No grid barrier, no floating-point atomics: a Gram entry
//                  is a per-lane sum over rows i = lane, lane + 64, ..., a butterfly over the wave, and a sum over the workgroups in index order.
//                  n <= 32 with n_basis left at 0: no iteration.  L goes to the host as a dense matrix and eig_dense returns its eigenpairs: the
//                  iteration cannot serve every such graph (a 16-column block may be the whole space, L of a 2-row cloud has the eigenvalue 2 that
//                  A = I - L / 2 maps to 0, and with k_neighbors = 2 L is defective, where block iteration stalls near sqrt(eps)).
#include "pcr_internal.hpp"

#include <cfloat>
#include <cmath>

namespace pcr {

namespace {

constexpr int SP_NB = 16;            // columns of a block (row stride)
constexpr int SP_KMAX = 32;
constexpr int SP_STEPS = 8;          // applications of A between two orthonormalisations (even: the block returns to its first buffer)
constexpr int SP_ROUNDS = 32;        // orthonormalisations between two Ritz checks
constexpr int SP_ONE_MAX = 4096;     // rows up to which one workgroup iterates alone
constexpr int SP_WG = 1024;          // lanes of the Gram / one-workgroup kernels: 16 waves, wave a owns row a of a 16 x 16 product
constexpr int SP_GRAM_MAX = 256;     // workgroups of a Gram launch at most
constexpr int SP_DENSE_MAX = 32;     // rows up to which the default call solves the dense problem on the host (eig_dense's limit; twice the widest block)

// ---------------------------------------------------------------------------------------------------------------------------- kNN
template <int DIM, int KC>
__global__ void sp_knn_kernel(const double* __restrict__ x, uint32_t n, int k, int32_t* __restrict__ idx_out, double* __restrict__ d2_out)
{
    extern __shared__ double tile[];                      // blockDim.x x DIM
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    double q[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) q[d] = live ? x[(size_t)i * DIM + d] : 0.0;
    double bd[KC];
    int32_t bi[KC];
#pragma unroll
    for (int s = 0; s < KC; s++) { bd[s] = __builtin_inf(); bi[s] = -1; }
    for (uint32_t base = 0; base < n; base += blockDim.x) {
        const uint32_t cnt = n - base < blockDim.x ? n - base : blockDim.x;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < cnt * DIM; e += blockDim.x) tile[e] = x[(size_t)base * DIM + e];
        __syncthreads();
        if (!live) continue;
        for (uint32_t t = 0; t < cnt; t++) {
            double s2 = 0.0;
#pragma unroll
            for (int d = 0; d < DIM; d++) {
                const double df = q[d] - tile[t * DIM + d];
                s2 = s2 + df * df;
            }
            if (s2 < bd[KC - 1]) {
                const int32_t j = (int32_t)(base + t);
#pragma unroll
                for (int s = KC - 1; s >= 0; s--) {
                    const double pd = s > 0 ? bd[s > 0 ? s - 1 : 0] : -1.0;      // d2 >= 0: nothing lies before slot 0
                    const int32_t pi = s > 0 ? bi[s > 0 ? s - 1 : 0] : -1;
                    if (s2 < bd[s]) {
                        const bool shift = s2 < pd;
                        bd[s] = shift ? pd : s2;
                        bi[s] = shift ? pi : j;
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int s = 0; s < KC; s++)
        if (s < k) { idx_out[(size_t)i * k + s] = bi[s]; d2_out[(size_t)i * k + s] = bd[s]; }
}

// ---------------------------------------------------------------------------------------------------------------------------- graph
// row i of L in place in col / val (k entries): the neighbours j != i by ascending column with the diagonal among them
__global__ void sp_graph_kernel(const int32_t* __restrict__ nn_idx, const double* __restrict__ nn_d2, uint32_t n, int k, int32_t* __restrict__ col,
                                double* __restrict__ val, int* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t* c = col + (size_t)i * k;
    double* v = val + (size_t)i * k;
    int m = 0;
    bool self = false, dup = false;
    for (int s = 0; s < k; s++) {
        const int32_t j = nn_idx[(size_t)i * k + s];
        const double d2 = nn_d2[(size_t)i * k + s];
        if (j == (int32_t)i) { self = true; continue; }
        if (!(d2 > 0.0) || j < 0 || (uint32_t)j >= n) { dup = true; continue; }
        if (m == k - 1) { dup = true; continue; }          // k neighbours beside the row itself: only duplicates push it out of its own list
        const double w = 1.0 / sqrt(d2);
        int p = m;                                         // insertion by column
        while (p > 0 && c[p - 1] > j) { c[p] = c[p - 1]; v[p] = v[p - 1]; p--; }
        c[p] = j; v[p] = w;
        m++;
    }
    if (dup || !self || m != k - 1) { atomicOr(flags, 1); return; }
    double sum = 0.0;
    for (int s = 0; s < m; s++) sum = sum + v[s];
    int p = m;                                             // the diagonal takes its place
    while (p > 0 && c[p - 1] > (int32_t)i) { c[p] = c[p - 1]; v[p] = -(v[p - 1] / sum); p--; }
    c[p] = (int32_t)i; v[p] = 1.0;
    for (int s = 0; s < p; s++) v[s] = -(v[s] / sum);
}

// ---------------------------------------------------------------------------------------------------------------------------- block kernels
__device__ inline uint64_t sp_mix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the start block: uniform in (-1, 1) from a hash of (row, column); columns >= nb are zero
__global__ void sp_init_kernel(double* X, uint32_t n, int nb)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < SP_NB; c++) {
        const uint64_t h = sp_mix(((uint64_t)i << 8) | (uint64_t)c);
        X[(size_t)i * SP_NB + c] = c < nb ? ((double)(h >> 11) * 0x1p-52 - 1.0) + 0x1p-53 : 0.0;
    }
}

// acc = (L X)_i: the entries of the row in column order
__device__ inline void sp_row_mul(const int32_t* __restrict__ col, const double* __restrict__ val, int k, const double* X, uint32_t i, double acc[SP_NB])
{
#pragma unroll
    for (int c = 0; c < SP_NB; c++) acc[c] = 0.0;
    for (int e = 0; e < k; e++) {
        const int32_t j = col[(size_t)i * k + e];
        const double w = val[(size_t)i * k + e];
        const double* xr = X + (size_t)j * SP_NB;
#pragma unroll
        for (int c = 0; c < SP_NB; c++) acc[c] = acc[c] + w * xr[c];
    }
}

// out_i = beta X_i + alpha (L X)_i - X_i Theta   (Theta: 16 x 16 row-major or nullptr)
__device__ inline void sp_row_axpy(const int32_t* __restrict__ col, const double* __restrict__ val, int k, const double* X, double* out, uint32_t i,
                                   double alpha, double beta, const double* theta)
{
    double acc[SP_NB];
    sp_row_mul(col, val, k, X, i, acc);
    const double* xi = X + (size_t)i * SP_NB;
    if (theta) {
        double xr[SP_NB];
#pragma unroll
        for (int c = 0; c < SP_NB; c++) xr[c] = xi[c];
#pragma unroll
        for (int c = 0; c < SP_NB; c++) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < SP_NB; a++) t = t + xr[a] * theta[a * SP_NB + c];
            out[(size_t)i * SP_NB + c] = (beta * xr[c] + alpha * acc[c]) - t;
        }
    } else {
#pragma unroll
        for (int c = 0; c < SP_NB; c++) out[(size_t)i * SP_NB + c] = beta * xi[c] + alpha * acc[c];
    }
}

__global__ void sp_axpy_kernel(const int32_t* __restrict__ col, const double* __restrict__ val, int k, uint32_t n, const double* X, double* out, double alpha,
                               double beta, const double* theta)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sp_row_axpy(col, val, k, X, out, i, alpha, beta, theta);
}

// X_i <- X_i M in place (M: 16 x 16 row-major), or out_i = X_i M
__device__ inline void sp_row_apply(const double* X, double* out, uint32_t i, const double* M)
{
    double xr[SP_NB];
#pragma unroll
    for (int c = 0; c < SP_NB; c++) xr[c] = X[(size_t)i * SP_NB + c];
#pragma unroll
    for (int c = 0; c < SP_NB; c++) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < SP_NB; a++) t = t + xr[a] * M[a * SP_NB + c];
        out[(size_t)i * SP_NB + c] = t;
    }
}

__global__ void sp_apply_kernel(const double* X, double* out, uint32_t n, const double* __restrict__ M)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sp_row_apply(X, out, i, M);
}

// out[a][b] = sum over rows [r0, r1) of A_ia B_ib, by a workgroup of SP_WG lanes: wave a, lanes stride the rows, a butterfly over the wave
__device__ inline void sp_block_gram(const double* A, const double* B, uint32_t r0, uint32_t r1, double* out)
{
    const int a = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[SP_NB];
#pragma unroll
    for (int b = 0; b < SP_NB; b++) acc[b] = 0.0;
    for (uint32_t i = r0 + lane; i < r1; i += 64) {
        const double xa = A[(size_t)i * SP_NB + a];
        const double* br = B + (size_t)i * SP_NB;
#pragma unroll
        for (int b = 0; b < SP_NB; b++) acc[b] = acc[b] + xa * br[b];
    }
#pragma unroll
    for (int b = 0; b < SP_NB; b++) {
        double v = acc[b];
        for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
        if (lane == 0) out[a * SP_NB + b] = v;
    }
}

// G (16 x 16, symmetric positive definite in its leading nb x nb) -> Rinv with G = R^T R, R upper triangular (R: 16 x 16 of workspace in LDS); one lane.
// Returns false on a pivot <= 0
__device__ inline bool sp_chol_inverse(const double* G, int nb, double* Rinv, double (*R)[SP_NB])
{
    for (int a = 0; a < SP_NB; a++)
        for (int b = 0; b < SP_NB; b++) R[a][b] = 0.0;
    for (int a = 0; a < nb; a++) {
        for (int b = a; b < nb; b++) {
            double s = G[a * SP_NB + b];
            for (int t = 0; t < a; t++) s = s - R[t][a] * R[t][b];
            if (b == a) {
                if (!(s > 0.0)) return false;
                R[a][a] = sqrt(s);
            } else {
                R[a][b] = s / R[a][a];
            }
        }
    }
    for (int a = 0; a < SP_NB; a++)
        for (int b = 0; b < SP_NB; b++) Rinv[a * SP_NB + b] = 0.0;
    for (int c = 0; c < nb; c++) {                          // column c of R^-1 by back-substitution
        for (int a = c; a >= 0; a--) {
            double s = a == c ? 1.0 : 0.0;
            for (int t = a + 1; t <= c; t++) s = s - R[a][t] * Rinv[t * SP_NB + c];
            Rinv[a * SP_NB + c] = s / R[a][a];
        }
    }
    return true;
}

__global__ __launch_bounds__(SP_WG) void sp_gram_kernel(const double* A, const double* B, uint32_t n, uint32_t rows_per_block, double* __restrict__ partials)
{
    const uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    sp_block_gram(A, B, (uint32_t)(r0 < n ? r0 : n), (uint32_t)r1, partials + (size_t)blockIdx.x * SP_NB * SP_NB);
}

// out = the partial products added in workgroup order; chol != 0: out <- R^-1 of its Cholesky factor (flags |= 2 on failure, out = identity)
__global__ __launch_bounds__(256) void sp_sum_kernel(const double* __restrict__ partials, uint32_t blocks, int nb, int chol, double* __restrict__ out,
                                                      int* __restrict__ flags)
{
    __shared__ double G[SP_NB * SP_NB];
    __shared__ double Ri[SP_NB * SP_NB];
    __shared__ double Rw[SP_NB][SP_NB];
    const int t = threadIdx.x;
    double s = 0.0;
    for (uint32_t b = 0; b < blocks; b++) s = s + partials[(size_t)b * SP_NB * SP_NB + t];
    G[t] = s;
    __syncthreads();
    if (!chol) { out[t] = G[t]; return; }
    if (t == 0 && !sp_chol_inverse(G, nb, Ri, Rw)) {
        atomicOr(flags, 2);
        for (int a = 0; a < SP_NB * SP_NB; a++) Ri[a] = (a / SP_NB == a % SP_NB) ? 1.0 : 0.0;
    }
    __syncthreads();
    out[t] = Ri[t];
}

// the one-workgroup iteration: rounds x (SP_STEPS applications of A = I - L / 2, Cholesky-QR; twice in the last round).  The block starts and ends in Xa.
__global__ __launch_bounds__(SP_WG) void sp_iterate_one_kernel(const int32_t* __restrict__ col, const double* __restrict__ val, int k, uint32_t n, int nb,
                                                               double* Xa, double* Xb, int rounds, int* __restrict__ flags)
{
    __shared__ double G[SP_NB * SP_NB];
    __shared__ double Ri[SP_NB * SP_NB];
    __shared__ double Rw[SP_NB][SP_NB];
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int r = 0; r < rounds; r++) {
        double* cur = Xa;
        double* nxt = Xb;
        for (int s = 0; s < SP_STEPS; s++) {
            for (uint32_t i = threadIdx.x; i < n; i += SP_WG) sp_row_axpy(col, val, k, cur, nxt, i, -0.5, 1.0, nullptr);
            __syncthreads();
            double* t = cur; cur = nxt; nxt = t;
        }
        const int passes = r == rounds - 1 ? 2 : 1;
        for (int p = 0; p < passes; p++) {
            sp_block_gram(Xa, Xa, 0, n, G);
            __syncthreads();
            if (threadIdx.x == 0 && !sp_chol_inverse(G, nb, Ri, Rw)) bad = 1;
            __syncthreads();
            if (bad) break;
            for (uint32_t i = threadIdx.x; i < n; i += SP_WG) sp_row_apply(Xa, Xa, i, Ri);
            __syncthreads();
        }
        if (bad) break;
    }
    if (threadIdx.x == 0 && bad) atomicOr(flags, 2);
}

}  // namespace

}  // namespace pcr

using namespace pcr;

struct pcr_spgraph {
    size_t n = 0;
    int k = 0;                       // entries of every row
    int32_t* col = nullptr;          // device, n k
    double* val = nullptr;           // device, n k
};

namespace {

#define SP_DISPATCH_DIM(dim, CALL)                                                                            \
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

// the kNN of every row, left on the device (idx: n k int32, d2: n k)
int sp_knn_device(pcr_ctx* ctx, const double* x, size_t n, int dim, int k, int32_t* idx_dev, double* d2_dev)
{
    const int block = n < 64 * 512 ? 64 : 256;
    const uint32_t blocks = (uint32_t)((n + block - 1) / block);
    const size_t lds = (size_t)block * dim * sizeof(double);
    ProfScope ps(ctx, "sp_knn");
    if (k <= 16) {
        SP_DISPATCH_DIM(dim, (sp_knn_kernel<D, 16><<<blocks, block, lds, ctx->stream>>>(x, (uint32_t)n, k, idx_dev, d2_dev)));
    } else {
        SP_DISPATCH_DIM(dim, (sp_knn_kernel<D, 32><<<blocks, block, lds, ctx->stream>>>(x, (uint32_t)n, k, idx_dev, d2_dev)));
    }
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

bool sp_mat_ok(const pcr_mat64* m, size_t* n, int* dim)
{
    return m && pcr_mat64_info(m, n, dim, nullptr) == PCR_OK && mat64_rows_dev(m) != nullptr;
}

struct SpBufs {
    double *Xa = nullptr, *Xb = nullptr, *Z = nullptr, *partials = nullptr, *small = nullptr;
    int* flags = nullptr;
};
// `small` holds four 16 x 16 matrices
constexpr int SP_M_T = 0, SP_M_Y = 256, SP_M_TH = 512, SP_M_N = 768, SP_SMALL = 1024;

struct SpRun {
    pcr_ctx* ctx;
    const pcr_spgraph* g;
    SpBufs b;
    uint32_t n, rowblocks, gram_blocks, rows_per_gram;
    int nb;
};

int sp_gram(const SpRun& r, const double* A, const double* B, int chol, double* out)
{
    sp_gram_kernel<<<r.gram_blocks, SP_WG, 0, r.ctx->stream>>>(A, B, r.n, r.rows_per_gram, r.b.partials);
    sp_sum_kernel<<<1, 256, 0, r.ctx->stream>>>(r.b.partials, r.gram_blocks, r.nb, chol, out, r.b.flags);
    PCR_HIP(r.ctx, hipGetLastError());
    return PCR_OK;
}

// one round of the many-launch path: SP_STEPS steps, then `passes` Cholesky-QR passes
int sp_round_many(const SpRun& r, int passes)
{
    const pcr_spgraph* g = r.g;
    double* cur = r.b.Xa;
    double* nxt = r.b.Xb;
    {
        ProfScope ps(r.ctx, "sp_step");
        for (int s = 0; s < SP_STEPS; s++) {
            sp_axpy_kernel<<<r.rowblocks, 256, 0, r.ctx->stream>>>(g->col, g->val, g->k, r.n, cur, nxt, -0.5, 1.0, nullptr);
            double* t = cur; cur = nxt; nxt = t;
        }
    }
    for (int p = 0; p < passes; p++) {
        int rc = sp_gram(r, r.b.Xa, r.b.Xa, 1, r.b.small + SP_M_N);
        if (rc != PCR_OK) return rc;
        sp_apply_kernel<<<r.rowblocks, 256, 0, r.ctx->stream>>>(r.b.Xa, r.b.Xa, r.n, r.b.small + SP_M_N);
    }
    PCR_HIP(r.ctx, hipGetLastError());
    return PCR_OK;
}

// the eigenvectors in V (n rows of stride ld, m_cols columns in use): normalise, fix the sign, hand out the first n_eig columns
void sp_hand_out(double* V, size_t ld, size_t n, int n_eig, int m_cols, uint32_t cmask, const double* wr, const double* wi, double* eigenvalues, double* vectors)
{
    for (int j = 0; j < m_cols; j++) {
        const bool cpx = cmask >> j & 1;
        if (cpx && !(wi[j] > 0.0)) continue;               // handled with its partner
        const int w = cpx ? 2 : 1;
        double s = 0.0;
        for (size_t i = 0; i < n; i++)
            for (int c = j; c < j + w; c++) s += V[i * ld + c] * V[i * ld + c];
        double big = 0.0, sign = 1.0;
        for (size_t i = 0; i < n; i++)
            if (std::fabs(V[i * ld + j]) > big) { big = std::fabs(V[i * ld + j]); sign = V[i * ld + j] < 0.0 ? -1.0 : 1.0; }
        const double sc = s > 0.0 ? sign / std::sqrt(s) : 0.0;
        for (size_t i = 0; i < n; i++)
            for (int c = j; c < j + w; c++) V[i * ld + c] *= sc;
    }
    if (vectors)
        for (size_t i = 0; i < n; i++)
            for (int j = 0; j < n_eig; j++) vectors[i * n_eig + j] = V[i * ld + j];
    if (eigenvalues) for (int j = 0; j < n_eig; j++) eigenvalues[j] = wr[j];
}

void sp_fill_info(pcr_spectral_info* info, int n_eig, int n_basis, int steps, int one, uint32_t cmask, int m_cols, double residual, const double* wr, const double* wi)
{
    memset(info, 0, sizeof(*info));
    info->n_eig = n_eig; info->n_basis = n_basis; info->solver_steps = steps; info->one_workgroup = one;
    info->complex_mask = cmask & ((1u << n_eig) - 1u);
    if (m_cols > n_eig) info->complex_mask |= 1u << (n_eig - 1);
    info->residual = residual;
    for (int j = 0; j < n_eig; j++) { info->eigenvalues[j] = wr[j]; info->eigenvalues_im[j] = wi[j]; }
}

// n <= SP_DENSE_MAX: L as a dense matrix on the host, every eigenpair from eig_dense, the residuals of the wanted ones in plain loops
int sp_embed_dense(pcr_ctx* ctx, const pcr_spgraph* g, int n_eig, double tol, double* eigenvalues, double* vectors, pcr_spectral_info* info)
{
    const int n = (int)g->n, k = g->k;
    int32_t col[SP_DENSE_MAX * SP_KMAX];
    double val[SP_DENSE_MAX * SP_KMAX], Ld[SP_DENSE_MAX * SP_DENSE_MAX], wr[SP_DENSE_MAX], wi[SP_DENSE_MAX], Y[SP_DENSE_MAX * SP_DENSE_MAX];
    double V[SP_DENSE_MAX * (SP_NB + 1)], W[SP_DENSE_MAX * (SP_NB + 1)];
    PCR_HIP(ctx, hipMemcpyAsync(col, g->col, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(val, g->val, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < n * n; a++) Ld[a] = 0.0;
    for (int i = 0; i < n; i++)
        for (int e = 0; e < k; e++) {
            const int32_t j = col[i * k + e];
            if (j < 0 || j >= n) return fail(ctx, PCR_ERR_STATE, "pcr_spectral_embed_f64: a column outside the graph");
            Ld[i * n + j] = val[i * k + e];
        }
    const int rc = eig_dense(n, Ld, wr, wi, Y);
    if (rc != PCR_OK) return fail(ctx, rc, "pcr_spectral_embed_f64: the dense eigenproblem");
    // the wanted columns: the n_eig of smallest real part, one more if a conjugate pair would be cut
    const int m_cols = wi[n_eig - 1] > 0.0 && n_eig < n ? n_eig + 1 : n_eig;
    const size_t ld = (size_t)m_cols;
    uint32_t cmask = 0;
    for (int j = 0; j < m_cols; j++) {
        if (wi[j] > 0.0 && j + 1 < m_cols) cmask |= 3u << j;
        for (int i = 0; i < n; i++) V[i * ld + j] = Y[i * n + j];
    }
    // W = L V - V Theta (Theta block diagonal: a pair is the 2 x 2 block [wr wi; -wi wr]), the entries of a row of L in column order
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m_cols; j++) {
            double acc = 0.0;
            for (int e = 0; e < k; e++) acc = acc + val[i * k + e] * V[(size_t)col[i * k + e] * ld + j];
            double t = wr[j] * V[i * ld + j];
            if (cmask >> j & 1) t = wi[j] > 0.0 ? t - wi[j] * V[i * ld + j + 1] : t - wi[j] * V[i * ld + j - 1];
            W[i * ld + j] = acc - t;
        }
    double residual = 0.0;
    for (int j = 0; j < m_cols; j++) {
        const int j0 = (cmask >> j & 1) && !(wi[j] > 0.0) ? j - 1 : j, j1 = (cmask >> j & 1) ? j0 + 1 : j0;
        double nv = 0.0, nr = 0.0;
        for (int i = 0; i < n; i++)
            for (int c = j0; c <= j1; c++) { nv += V[i * ld + c] * V[i * ld + c]; nr += W[i * ld + c] * W[i * ld + c]; }
        const double res = nv > 0.0 ? std::sqrt(nr / nv) : __builtin_inf();
        residual = res > residual || res != res ? res : residual;
    }
    sp_hand_out(V, ld, (size_t)n, n_eig, m_cols, cmask, wr, wi, eigenvalues, vectors);
    if (info) sp_fill_info(info, n_eig, 0, 0, 0, cmask, m_cols, residual, wr, wi);
    return residual <= tol ? PCR_OK : PCR_SPECTRAL_NOT_CONVERGED;
}

}  // namespace

extern "C" int pcr_mat64_knn_f64(pcr_ctx* ctx, pcr_mat64* m, int k, int32_t* idx, double* d2)
{
    size_t n = 0;
    int dim = 0;
    if (!ctx || !sp_mat_ok(m, &n, &dim) || k < 1 || k > SP_KMAX || (size_t)k > n || !idx || !d2) return fail(ctx, PCR_ERR_ARG, "pcr_mat64_knn_f64: 1 <= k <= 32, k <= n");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* idx_dev = nullptr;
    double* d2_dev = nullptr;
    Layout L;
    L.add(&d2_dev, n * k);
    L.add(&idx_dev, n * k);
    int rc = bind_scratch(ctx, L);
    if (rc != PCR_OK) return rc;
    if ((rc = sp_knn_device(ctx, mat64_rows_dev(m), n, dim, k, idx_dev, d2_dev)) != PCR_OK) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(idx, idx_dev, n * k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(d2, d2_dev, n * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" int pcr_spgraph_destroy(pcr_ctx* ctx, pcr_spgraph* g)
{
    if (!g) return PCR_OK;
    if (ctx && ctx->stream) hipStreamSynchronize(ctx->stream);
    if (g->col) hipFree(g->col);
    if (g->val) hipFree(g->val);
    delete g;
    return PCR_OK;
}

extern "C" int pcr_spectral_graph_f64(pcr_ctx* ctx, pcr_mat64* m, int k, pcr_spgraph** out)
{
    size_t n = 0;
    int dim = 0;
    if (!ctx || !sp_mat_ok(m, &n, &dim) || !out || k < 2 || k > SP_KMAX || (size_t)k > n) return fail(ctx, PCR_ERR_ARG, "pcr_spectral_graph_f64: 2 <= k_neighbors <= 32, k_neighbors <= n");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* idx_dev = nullptr;
    double* d2_dev = nullptr;
    int* flags = nullptr;
    Layout L;
    L.add(&d2_dev, n * k);
    L.add(&idx_dev, n * k);
    L.add(&flags, 1);
    int rc = bind_scratch(ctx, L);
    if (rc != PCR_OK) return rc;
    pcr_spgraph* g = new pcr_spgraph();
    g->n = n; g->k = k;
    if (hipMalloc(&g->col, n * k * sizeof(int32_t)) != hipSuccess || hipMalloc(&g->val, n * k * sizeof(double)) != hipSuccess) {
        pcr_spgraph_destroy(ctx, g);
        return fail(ctx, PCR_ERR_NOMEM, "pcr_spectral_graph_f64");
    }
    int host_flags = 0;
    hipError_t e = hipMemsetAsync(flags, 0, sizeof(int), ctx->stream);
    if (e == hipSuccess) {
        rc = sp_knn_device(ctx, mat64_rows_dev(m), n, dim, k, idx_dev, d2_dev);
        if (rc == PCR_OK) {
            ProfScope ps(ctx, "sp_graph");
            sp_graph_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, ctx->stream>>>(idx_dev, d2_dev, (uint32_t)n, k, g->col, g->val, flags);
            e = hipGetLastError();
        }
    }
    if (rc == PCR_OK && e == hipSuccess) e = hipMemcpyAsync(&host_flags, flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (rc == PCR_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (rc != PCR_OK || e != hipSuccess) {
        pcr_spgraph_destroy(ctx, g);
        return rc != PCR_OK ? rc : fail(ctx, PCR_ERR_HIP, "pcr_spectral_graph_f64", e);
    }
    if (host_flags) {
        pcr_spgraph_destroy(ctx, g);
        *out = nullptr;
        return PCR_SPECTRAL_DUPLICATE;
    }
    *out = g;
    return PCR_OK;
}

extern "C" int pcr_spgraph_info(const pcr_spgraph* g, size_t* n, size_t* nnz)
{
    if (!g) return PCR_ERR_ARG;
    if (n) *n = g->n;
    if (nnz) *nnz = g->n * (size_t)g->k;
    return PCR_OK;
}

extern "C" int pcr_spgraph_read(pcr_ctx* ctx, const pcr_spgraph* g, int64_t* row_ptr, int32_t* col, double* val)
{
    if (!ctx || !g) return fail(ctx, PCR_ERR_ARG, "pcr_spgraph_read");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    if (row_ptr) for (size_t i = 0; i <= g->n; i++) row_ptr[i] = (int64_t)(i * (size_t)g->k);
    if (col) PCR_HIP(ctx, hipMemcpyAsync(col, g->col, g->n * g->k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (val) PCR_HIP(ctx, hipMemcpyAsync(val, g->val, g->n * g->k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" int pcr_spectral_embed_f64(pcr_ctx* ctx, pcr_spgraph* g, int n_eig, int n_basis, double tol, int max_iter, double* eigenvalues, double* vectors,
                                      pcr_spectral_info* info)
{
    if (!ctx || !g || !g->col || !g->val || g->n < 1) return fail(ctx, PCR_ERR_ARG, "pcr_spectral_embed_f64");
    const size_t n = g->n;
    if (n_eig == 0) n_eig = (int)(n < 8 ? n : 8);
    const bool dense = n_basis == 0 && n <= (size_t)SP_DENSE_MAX;
    if (n_basis == 0) { n_basis = n_eig + 5 > SP_NB ? SP_NB : n_eig + 5; if ((size_t)n_basis > n) n_basis = (int)n; }
    if (n_eig < 1 || n_basis < n_eig || n_basis > SP_NB || (size_t)n_basis > n || tol != tol) return fail(ctx, PCR_ERR_ARG, "pcr_spectral_embed_f64: 1 <= n_eig <= n_basis <= 16, n_basis <= n");
    if (!(tol > 0.0)) tol = 1e-10;
    if (max_iter <= 0) max_iter = 400000;
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    if (dense) return sp_embed_dense(ctx, g, n_eig, tol, eigenvalues, vectors, info);
    SpRun r;
    r.ctx = ctx; r.g = g; r.n = (uint32_t)n; r.nb = n_basis;
    r.rowblocks = (uint32_t)((n + 255) / 256);
    size_t gb = (n + 2047) / 2048;
    r.gram_blocks = (uint32_t)(gb < 1 ? 1 : (gb > SP_GRAM_MAX ? SP_GRAM_MAX : gb));
    r.rows_per_gram = (uint32_t)((n + r.gram_blocks - 1) / r.gram_blocks);
    Layout L;
    L.add(&r.b.Xa, n * SP_NB);
    L.add(&r.b.Xb, n * SP_NB);
    L.add(&r.b.Z, n * SP_NB);
    L.add(&r.b.partials, (size_t)r.gram_blocks * SP_NB * SP_NB);
    L.add(&r.b.small, (size_t)SP_SMALL);
    L.add(&r.b.flags, 1);
    int rc = bind_scratch(ctx, L);
    if (rc != PCR_OK) return rc;
    hipStream_t st = ctx->stream;
    PCR_HIP(ctx, hipMemsetAsync(r.b.flags, 0, sizeof(int), st));
    sp_init_kernel<<<r.rowblocks, 256, 0, st>>>(r.b.Xa, r.n, n_basis);
    PCR_HIP(ctx, hipGetLastError());
    const bool one = n <= (size_t)SP_ONE_MAX && tune_get(ctx, "spectral_path", 0) != 2;       // tune spectral_path 2: the many-launch path at any n (tests)
    const int nbk = n_basis;
    double T[SP_NB * SP_NB], Tn[SP_NB * SP_NB], wr[SP_NB], wi[SP_NB], Yn[SP_NB * SP_NB], Y[SP_NB * SP_NB], TH[SP_NB * SP_NB], NV[SP_NB * SP_NB], NR[SP_NB * SP_NB];
    int steps = 0, m_cols = n_eig, status = PCR_SPECTRAL_NOT_CONVERGED;
    double residual = __builtin_inf();
    uint32_t cmask = 0;
    while (steps < max_iter) {
        if (one) {
            ProfScope ps(ctx, "sp_iterate_one");
            sp_iterate_one_kernel<<<1, SP_WG, 0, st>>>(g->col, g->val, g->k, r.n, nbk, r.b.Xa, r.b.Xb, SP_ROUNDS, r.b.flags);
            PCR_HIP(ctx, hipGetLastError());
        } else {
            for (int q = 0; q < SP_ROUNDS; q++)
                if ((rc = sp_round_many(r, q == SP_ROUNDS - 1 ? 2 : 1)) != PCR_OK) return rc;
        }
        steps += SP_ROUNDS * SP_STEPS;
        // Rayleigh-Ritz: T = Q^T (L Q)
        sp_axpy_kernel<<<r.rowblocks, 256, 0, st>>>(g->col, g->val, g->k, r.n, r.b.Xa, r.b.Z, 1.0, 0.0, nullptr);
        if ((rc = sp_gram(r, r.b.Xa, r.b.Z, 0, r.b.small + SP_M_T)) != PCR_OK) return rc;
        int host_flags = 0;
        PCR_HIP(ctx, hipMemcpyAsync(T, r.b.small + SP_M_T, sizeof(T), hipMemcpyDeviceToHost, st));
        PCR_HIP(ctx, hipMemcpyAsync(&host_flags, r.b.flags, sizeof(int), hipMemcpyDeviceToHost, st));
        PCR_HIP(ctx, hipStreamSynchronize(st));
        if (host_flags) return fail(ctx, PCR_ERR_STATE, "pcr_spectral_embed_f64: the block lost rank (Cholesky-QR met a pivot <= 0)");
        for (int a = 0; a < nbk; a++)
            for (int b = 0; b < nbk; b++) Tn[a * nbk + b] = T[a * SP_NB + b];
        if ((rc = eig_small(nbk, Tn, wr, wi, Yn)) != PCR_OK) return fail(ctx, rc, "pcr_spectral_embed_f64: the Ritz matrix");
        // the wanted columns: the n_eig of smallest real part, one more if a conjugate pair would be cut
        m_cols = n_eig;
        if (wi[n_eig - 1] > 0.0 && n_eig < nbk) m_cols = n_eig + 1;
        memset(Y, 0, sizeof(Y));
        memset(TH, 0, sizeof(TH));
        cmask = 0;
        for (int j = 0; j < m_cols; j++) {
            for (int a = 0; a < nbk; a++) Y[a * SP_NB + j] = Yn[a * nbk + j];
            TH[j * SP_NB + j] = wr[j];
            if (wi[j] > 0.0 && j + 1 < m_cols) { TH[j * SP_NB + j + 1] = wi[j]; TH[(j + 1) * SP_NB + j] = -wi[j]; cmask |= 3u << j; }
        }
        PCR_HIP(ctx, hipMemcpyAsync(r.b.small + SP_M_Y, Y, sizeof(Y), hipMemcpyHostToDevice, st));
        PCR_HIP(ctx, hipMemcpyAsync(r.b.small + SP_M_TH, TH, sizeof(TH), hipMemcpyHostToDevice, st));
        // V = Q Y (into Z), W = L V - V Theta (into Xb), and their column norms
        sp_apply_kernel<<<r.rowblocks, 256, 0, st>>>(r.b.Xa, r.b.Z, r.n, r.b.small + SP_M_Y);
        sp_axpy_kernel<<<r.rowblocks, 256, 0, st>>>(g->col, g->val, g->k, r.n, r.b.Z, r.b.Xb, 1.0, 0.0, r.b.small + SP_M_TH);
        if ((rc = sp_gram(r, r.b.Z, r.b.Z, 0, r.b.small + SP_M_N)) != PCR_OK) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(NV, r.b.small + SP_M_N, sizeof(NV), hipMemcpyDeviceToHost, st));
        if ((rc = sp_gram(r, r.b.Xb, r.b.Xb, 0, r.b.small + SP_M_N)) != PCR_OK) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(NR, r.b.small + SP_M_N, sizeof(NR), hipMemcpyDeviceToHost, st));
        PCR_HIP(ctx, hipStreamSynchronize(st));
        residual = 0.0;
        for (int j = 0; j < m_cols; j++) {
            double nv = NV[j * SP_NB + j], nr = NR[j * SP_NB + j];
            if (cmask >> j & 1) {
                const int j0 = (wi[j] > 0.0) ? j : j - 1;
                nv = NV[j0 * SP_NB + j0] + NV[(j0 + 1) * SP_NB + j0 + 1];
                nr = NR[j0 * SP_NB + j0] + NR[(j0 + 1) * SP_NB + j0 + 1];
            }
            const double res = nv > 0.0 ? std::sqrt(nr / nv) : __builtin_inf();
            residual = res > residual || res != res ? res : residual;
        }
        if (residual <= tol) { status = PCR_OK; break; }
    }
    // the Ritz vectors of the last check lie in Z
    if (ensure_stage(ctx, n * SP_NB * sizeof(double)) != PCR_OK) return fail(ctx, PCR_ERR_NOMEM, "pcr_spectral_embed_f64: staging");
    double* V = (double*)ctx->host_stage;
    PCR_HIP(ctx, hipMemcpyAsync(V, r.b.Z, n * SP_NB * sizeof(double), hipMemcpyDeviceToHost, st));
    PCR_HIP(ctx, hipStreamSynchronize(st));
    sp_hand_out(V, SP_NB, n, n_eig, m_cols, cmask, wr, wi, eigenvalues, vectors);
    if (info) sp_fill_info(info, n_eig, n_basis, steps, one ? 1 : 0, cmask, m_cols, residual, wr, wi);
    return status;
}

extern "C" int pcr_spectral_cluster_f64(pcr_ctx* ctx, pcr_mat64* m, int k_neighbors, int n_eig, int n_clusters, int32_t* labels, double* features,
                                        pcr_spectral_info* info)
{
    size_t n = 0;
    int dim = 0;
    if (!ctx || !sp_mat_ok(m, &n, &dim) || !labels || n_clusters < 0 || n_clusters > 8 || n_eig < 0 || n_eig > SP_NB) return fail(ctx, PCR_ERR_ARG, "pcr_spectral_cluster_f64: 0 <= n_clusters <= 8, n_eig <= 16");
    if (n_eig == 0) n_eig = (int)(n < 8 ? n : 8);
    if (n_clusters > n_eig) return fail(ctx, PCR_ERR_ARG, "pcr_spectral_cluster_f64: n_clusters <= n_eig");
    pcr_spgraph* g = nullptr;
    int rc = pcr_spectral_graph_f64(ctx, m, k_neighbors, &g);
    if (rc != PCR_OK) return rc;
    pcr_spectral_info inf{};                              // an embedding that refuses its arguments fills nothing: the caller then reads zeros
    std::vector<double> vec(n * (size_t)n_eig), eig(n_eig);
    rc = pcr_spectral_embed_f64(ctx, g, n_eig, 0, 0.0, 0, eig.data(), vec.data(), &inf);
    pcr_spgraph_destroy(ctx, g);
    if (info) *info = inf;
    if (rc != PCR_OK) return rc;
    int K = n_clusters > 0 ? n_clusters : spectral_select_k(eig.data(), n_eig);
    if (K > 8) K = 8;
    if (info) info->k_clusters = K;
    if (inf.complex_mask & ((1u << K) - 1u)) return PCR_SPECTRAL_COMPLEX;
    std::vector<double> feat(n * (size_t)K);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < K; c++) feat[i * K + c] = vec[i * n_eig + c];
    if (features) memcpy(features, feat.data(), feat.size() * sizeof(double));
    // initial_choice (:249-289)
    std::vector<double> centres;
    centres.reserve((size_t)K * K);
    centres.insert(centres.end(), feat.begin(), feat.begin() + K);
    for (size_t row = 1; row < n && centres.size() < (size_t)K * K; row++) {
        bool add = true;
        for (size_t t = 0; t < centres.size() / K && add; t++) {
            double diff = 0.0;
            for (int c = 0; c < K; c++) { const double e = centres[t * K + c] - feat[row * K + c]; diff += e * e; }
            if (diff < 0.0001) add = false;
        }
        if (add) centres.insert(centres.end(), feat.begin() + row * K, feat.begin() + (row + 1) * K);
    }
    if (centres.size() < (size_t)K * K) return PCR_SPECTRAL_FEW_SEEDS;
    pcr_mat64* fm = nullptr;
    if ((rc = pcr_mat64_create(ctx, feat.data(), n, K, &fm)) != PCR_OK) return rc;
    int iters = 0, conv = 0;
    rc = pcr_kmeans_fit_f64(ctx, fm, K, centres.data(), 1e-4, 200, PCR_KMEANS_CPP, nullptr, labels, &iters, &conv);
    pcr_mat64_destroy(ctx, fm);
    if (info) { info->kmeans_iters = iters; info->kmeans_converged = conv; }
    return rc;
}
