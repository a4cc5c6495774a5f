// pointnet_train.hip — the training pass of HomeworkFinal's vanilla PointNet classifier: training-mode forward, get_loss with the feature-transform
// regulariser, the gradient of every parameter (models/pointnet_cls.py, models/pointnet.py; train_cls.py's step without its optimiser).  The contract is
// written out above pcr_pn1_trainer_create in include/pcr.h.
//
// The dW product, the statistics, BatchNorm / ReLU, the max after a ReLU, the NLL (pn2t_*) and pn1t_dropout (the head's dropout BEFORE BatchNorm, in place:
// forward on the product, backward on its gradient) are pointnet_train_common.hpp's, and so are the layer step (LayerRun, here on the blocked product), the plan
// base and the create / info / call head and tail.  What this model adds:
//   pn1t_gemm_fwd / pn1t_gemm_dx     z = x W^T + b and dx = dz W on the same MFMA tiles, blocked over k: f32 chains over 64 k, the blocks added in f64
//   pn1t_transform3    xyz . trans per object in plain fmaf, the features pass through
//   pn1t_transform     x . T (forward) or dy . T^T (backward) per object: a workgroup serves rows of ONE object, its K x K matrix staged in LDS in the
//                      operand order of v_mfma_f32_16x16x4_f32; every output is one chain from +0 over ascending k
//   pn1t_identity      + 1 on the diagonal entries of a T-Net's last layer
//   pn1t_smax          the SIGNED max over an object's points on the integer key that orders all floats, the lowest position among the maxima
//   pn1t_reg           per object, in f64: M = A A^T - A, its Frobenius norm, and dA
//   pn1t_loss_fin      reg = the mean of the norms, total = nll + reg_scale reg
//   pn1t_add           one f32 addition per element: the two gradient paths into conv 0's activation, dA into dT
// dT[b] = x[b]^T dy[b] is the shared dW product with one chunk per object (pn1t_gemm_dt).  No floating-point atomic anywhere.
#include "pointnet_train_common.hpp"
#include "f32_key.hpp"

namespace {

constexpr uint32_t T1_KB = 64;          // the products z and dx: f32 chains over blocks of 64 k, the blocks added in f64

// C = init + A B as pn2t_gemm_kernel lays it out (one chunk: all of k), but BLOCKED over k: inside a block of T1_KB consecutive k an output is one f32 fma
// chain from +0 over ascending k on v_mfma_f32_16x16x4_f32; the block results join an f64 sum that starts at init (+0 without one), blocks ascending; the sum
// is rounded ONCE.  A 1024-term product then errs like a 64-term one: the single chain put the small T fixture 40 reference errors away.
__global__ __launch_bounds__(T_BLOCK) void pn1t_gemm_kernel(const GemmArgs g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, h = lane >> 4;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * 4 + (unsigned)wave) * (16 * T_RT);
    if (i0 >= g.M) return;                                      // wave-uniform; the kernel has no barrier
    const uint32_t j0 = blockIdx.y * 64;
    double sum[T_RT][4][4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t col = j0 + 16 * t + j;
        const double v = (g.init && col < g.N) ? (double)g.init[col] : 0.0;
#pragma unroll
        for (int rt = 0; rt < T_RT; rt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) sum[rt][t][reg] = v;
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
    for (uint32_t k0 = 0; k0 < g.Kt; k0 += T1_KB) {
        const uint32_t ke = g.Kt - k0 < T1_KB ? g.Kt : k0 + T1_KB;
        f32x4 acc[T_RT][4];
#pragma unroll
        for (int rt = 0; rt < T_RT; rt++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[rt][t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll 2
        for (uint32_t k = k0; k < ke; k += 4) {
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
#pragma unroll
        for (int rt = 0; rt < T_RT; rt++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) sum[rt][t][reg] = sum[rt][t][reg] + (double)acc[rt][t][reg];
    }
#pragma unroll
    for (int rt = 0; rt < T_RT; rt++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t col = j0 + 16 * t + j;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const unsigned long long row = i0 + 16 * rt + 4 * h + reg;
                if (row < g.M && col < g.N) g.c[(size_t)row * g.N + col] = (float)sum[rt][t][reg];
            }
        }
}

// the blocked product of one stage: z (from the bias) or dx (from +0)
int launch_gemm1(pcr_ctx* ctx, const char* prof, const GemmArgs& g, const char*)
{
    if (g.M == 0 || g.N == 0) return PCR_OK;
    ProfScope ps(ctx, prof);
    hipLaunchKernelGGL(pn1t_gemm_kernel, dim3((g.M + T_ROWS - 1) / T_ROWS, (g.N + 63) / 64, 1), dim3(T_BLOCK), 0, ctx->stream, g);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

__global__ __launch_bounds__(T_BLOCK) void pn1t_transform3_kernel(const float* __restrict__ x, const float* __restrict__ T, size_t rows, uint32_t npts, uint32_t C0,
                                                                  float* __restrict__ y)
{
    const size_t r = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (r >= rows) return;
    const float* t = T + (r / npts) * 9;
    const float* xr = x + r * C0;
    float* yr = y + r * C0;
    for (int j = 0; j < 3; j++) {
        float c = 0.0f;
        for (int k = 0; k < 3; k++) c = fmaf(xr[k], t[3 * k + j], c);
        yr[j] = c;
    }
    for (uint32_t c = 3; c < C0; c++) yr[c] = xr[c];
}

// y[b][r][j] = c_K, c_0 = +0, c_(k+1) = fma(x[b][r][k], B(k, j), c_k), B(k, j) = T[b][k sk + j sj]: (sk, sj) = (K, 1) is x . T, (1, K) is x . T^T.
// grid (ceil(npts / 64), n_obj): a wave owns 16 rows of object blockIdx.y.  LDS holds B as [ceil(K / 4)][ceil(K / 16)][64]: the B operand of MFMA m and
// column tile t is 64 consecutive floats (lane l: k = 4 m + (l >> 4), column 16 t + (l & 15)), +0 past an edge.
__global__ __launch_bounds__(T_BLOCK) void pn1t_transform_kernel(const float* __restrict__ x, const float* __restrict__ T, uint32_t npts, uint32_t K, uint32_t sk, uint32_t sj,
                                                                 float* __restrict__ y)
{
    extern __shared__ float lds_b[];
    const uint32_t b = blockIdx.y, KT = (K + 15u) / 16u, KM = (K + 3u) / 4u;
    const float* Tb = T + (size_t)b * K * K;
    for (uint32_t e = threadIdx.x; e < KM * KT * 64u; e += T_BLOCK) {
        const uint32_t l = e & 63u, mt = e >> 6, t = mt % KT, m = mt / KT;
        const uint32_t k = 4u * m + (l >> 4), col = 16u * t + (l & 15u);
        lds_b[e] = (k < K && col < K) ? Tb[(size_t)k * sk + (size_t)col * sj] : 0.0f;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, h = lane >> 4;
    const uint32_t r0 = (blockIdx.x * 4u + wave) * 16u;
    if (r0 >= npts) return;                                     // wave-uniform, past the only barrier
    const bool row_ok = r0 + j < npts;
    const float* xr = x + ((size_t)b * npts + (row_ok ? r0 + j : 0u)) * K;
    float* yb = y + (size_t)b * npts * K;
    for (uint32_t t0 = 0; t0 < KT; t0 += 4) {
        const uint32_t nt = KT - t0 < 4u ? KT - t0 : 4u;        // wave-uniform
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
        for (uint32_t m = 0; m < KM; m++) {
            const uint32_t k = 4u * m + h;
            const float av = (row_ok && k < K) ? xr[k] : 0.0f;
            const float* bp = lds_b + ((size_t)m * KT + t0) * 64u + lane;
#pragma unroll
            for (int t = 0; t < 4; t++)
                if ((uint32_t)t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[t * 64], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const uint32_t row = r0 + 4u * h + reg, col = 16u * (t0 + t) + j;
                if ((uint32_t)t < nt && row < npts && col < K) yb[(size_t)row * K + col] = acc[t][reg];
            }
    }
}

// T[b][i][i] <- T[b][i][i] + 1, one f32 addition to the finished chain
__global__ __launch_bounds__(T_BLOCK) void pn1t_identity_kernel(float* __restrict__ T, size_t n_obj, uint32_t k)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= n_obj * k) return;
    const size_t b = e / k, i = e - b * k;
    float* p = T + b * k * k + i * (k + 1);
    *p = *p + 1.0f;
}

// feat[g][c] = the max over the gsize rows of group g in the order -inf < ... < -0 < +0 < ... < +inf; arg[g][c] = the lowest position that holds it
__global__ __launch_bounds__(T_BLOCK) void pn1t_smax_kernel(const float* __restrict__ y, uint32_t groups, uint32_t gsize, uint32_t N, float* __restrict__ feat,
                                                            uint32_t* __restrict__ arg)
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= (size_t)groups * N) return;
    const uint32_t g = (uint32_t)(e / N), c = (uint32_t)(e - (size_t)g * N);
    const float* p = y + (size_t)g * gsize * N + c;
    float m = p[0];
    uint32_t mk = f32_key(m), best = 0;
    for (uint32_t k = 1; k < gsize; k++) {
        const float v = p[(size_t)k * N];
        const uint32_t vk = f32_key(v);
        if (vk > mk) { m = v; mk = vk; best = k; }
    }
    feat[e] = m;
    arg[e] = best;
}

__global__ __launch_bounds__(T_BLOCK) void pn1t_add_kernel(const float* a, const float* b, size_t total, float* out)      // out may be a or b
{
    const size_t e = (size_t)blockIdx.x * T_BLOCK + threadIdx.x;
    if (e >= total) return;
    out[e] = a[e] + b[e];
}

// one workgroup per object, all in f64 from the f32 A (K x K, K <= 128), products and sums rounded separately:
//   M[i][j] = (sum over ascending k of A[i][k] A[j][k]) - A[i][j];  row[i] = sum over ascending j of M[i][j]^2;  norm = sqrt(sum over ascending i of row[i])
//   dA[p][q] = f32(scale / (n_obj norm) ((sum over ascending j of (M[p][j] + M[j][p]) A[j][q]) - M[p][q])), +0 where norm == 0
__global__ __launch_bounds__(T_BLOCK) void pn1t_reg_kernel(const float* __restrict__ A, uint32_t K, uint32_t n_obj, double scale, double* __restrict__ Mb,
                                                           double* __restrict__ norm, float* __restrict__ dA)
{
    __shared__ double rows[PN_MAX_TRANSFORM];
    __shared__ double nrm_s;
    const size_t b = blockIdx.x;
    const float* Ab = A + b * K * K;
    double* M = Mb + b * K * K;
    for (uint32_t e = threadIdx.x; e < K * K; e += T_BLOCK) {
        const uint32_t i = e / K, j = e - i * K;
        double s = 0.0;
        for (uint32_t k = 0; k < K; k++) s = s + (double)Ab[i * K + k] * (double)Ab[j * K + k];
        M[e] = s - (double)Ab[e];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < K; i += T_BLOCK) {
        double s = 0.0;
        for (uint32_t j = 0; j < K; j++) s = s + M[i * K + j] * M[i * K + j];
        rows[i] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t i = 0; i < K; i++) s = s + rows[i];
        nrm_s = sqrt(s);
        norm[b] = nrm_s;
    }
    __syncthreads();
    const double nrm = nrm_s;
    const double f = nrm > 0.0 ? scale / ((double)n_obj * nrm) : 0.0;
    for (uint32_t e = threadIdx.x; e < K * K; e += T_BLOCK) {
        const uint32_t p = e / K, q = e - p * K;
        double s = 0.0;
        for (uint32_t j = 0; j < K; j++) s = s + (M[p * K + j] + M[j * K + p]) * (double)Ab[j * K + q];
        dA[b * K * K + e] = nrm > 0.0 ? (float)(f * (s - M[e])) : 0.0f;
    }
}

// loss[1] holds the NLL.  loss[2] <- reg = (sum over ascending b of norm[b]) / n_obj (norm == NULL: 0), loss[0] <- nll + scale reg
__global__ void pn1t_loss_fin_kernel(const double* __restrict__ norm, uint32_t n_obj, double scale, double* __restrict__ loss)
{
    if (threadIdx.x || blockIdx.x) return;
    double reg = 0.0;
    if (norm) {
        double s = 0.0;
        for (uint32_t b = 0; b < n_obj; b++) s = s + norm[b];
        reg = s / (double)n_obj;
    }
    loss[2] = reg;
    loss[0] = loss[1] + scale * reg;
}

// the device block of one call: PlanBase's, with the per-stack buffers in `own`
struct Plan1 : PlanBase {
    uint32_t rows = 0, n_obj = 0, npts = 0;
    float* obj = nullptr;            // uploaded
    // per stack
    float *xt = nullptr, *xf = nullptr, *feat_s = nullptr, *feat_f = nullptr, *gfeat = nullptr, *g1 = nullptr, *dA = nullptr;
    uint32_t *arg_s = nullptr, *arg_f = nullptr, *garg = nullptr;
    double *Mb = nullptr, *norm = nullptr;
};

inline uint32_t keep_width(const pcr_pn1_desc& d) { return d.n_fc >= 2 ? d.fc_widths[d.n_fc - 2] : 0u; }

// false: too large
bool make_plan1(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, Plan1& P)
{
    const pcr_pn1_desc& d = t->desc1;
    const uint32_t C0 = 3 + d.D0, K = d.widths[0];
    if (n_obj > 65535u || npts > PN_MAX_ROWS || (unsigned long long)n_obj * npts > PN_MAX_ROWS / PN_MAX_WIDTH) return false;
    const size_t rows = n_obj * npts;
    P.rows = (uint32_t)rows; P.n_obj = (uint32_t)n_obj; P.npts = (uint32_t)npts;
    P.up.add(&P.obj, rows * C0);
    P.up.add(&P.target, n_obj);
    P.up.add(&P.keep, n_obj * keep_width(d));
    const uint32_t Ct = d.tnet_conv[2], Cg = d.widths[d.n_mlp - 1];
    P.own.add(&P.xt, d.stn3 ? rows * C0 : 0);
    P.own.add(&P.feat_s, d.stn3 ? n_obj * Ct : 0);
    P.own.add(&P.arg_s, d.stn3 ? n_obj * Ct : 0);
    P.own.add(&P.xf, d.fstn ? rows * K : 0);
    P.own.add(&P.g1, d.fstn ? rows * K : 0);
    P.own.add(&P.feat_f, d.fstn ? n_obj * Ct : 0);
    P.own.add(&P.arg_f, d.fstn ? n_obj * Ct : 0);
    P.own.add(&P.dA, d.fstn ? n_obj * K * K : 0);
    P.own.add(&P.Mb, d.fstn ? n_obj * K * K : 0);
    P.own.add(&P.norm, d.fstn ? n_obj : 0);
    P.own.add(&P.gfeat, n_obj * Cg);
    P.own.add(&P.garg, n_obj * Cg);
    const size_t nl = t->layers.size();
    P.layers(nl, 0);
    P.dy_cells = std::max(rows * C0, n_obj * (size_t)K * K);     // the gradient of the input rows; dT
    P.dw_cells = n_obj * (size_t)K * K;                          // dT: one chunk per object
    auto is_conv = [&](size_t i) {
        if (d.stn3 && i < t->stn_first + 3u) return true;
        if (i >= t->enc_first && i < t->fstn_first) return true;
        return d.fstn && i >= t->fstn_first && i < t->fstn_first + 3u;
    };
    for (size_t i = 0; i < nl; i++) P.add_layer(i, is_conv(i) ? rows : n_obj, t->layers[i], t->chunk_rows, false);
    P.finish(n_obj, t->layers.back().N, 3);
    return true;
}

// LayerRun on the blocked product, and what the T-Nets add to it
struct ClsRun : LayerRun {
    Plan1& P;                // LayerRun's plan, with this model's fields in reach

    ClsRun(pcr_ctx* c, pcr_pn2_trainer* tr, Plan1& plan, const char* name) : LayerRun(c, tr, plan, name, launch_gemm1, "pn1t_gemm_fwd", "pn1t_gemm_dx"), P(plan) {}

    // a T-Net: x (rows x cin) -> its k x k matrices, identity added, in P.z[first + 5]
    void tnet_fwd(uint32_t first, const float* x, uint32_t k, float* feat, uint32_t* arg)
    {
        fwd(first, x, P.rows, true);
        fwd(first + 1, P.y[first], P.rows, true);
        fwd(first + 2, P.y[first + 1], P.rows, true);
        if (rc) return;
        const uint32_t C = t->layers[first + 2].N;
        {
            ProfScope ps(ctx, "pn2t_max");
            hipLaunchKernelGGL(pn2t_max_kernel, dim3(blocks_for((size_t)P.n_obj * C)), dim3(T_BLOCK), 0, ctx->stream, P.y[first + 2], P.n_obj, P.npts, C, C, 0u, feat,
                               arg);
        }
        fwd(first + 3, feat, P.n_obj, true);
        fwd(first + 4, P.y[first + 3], P.n_obj, true);
        fwd(first + 5, P.y[first + 4], P.n_obj, false);
        if (rc) return;
        ProfScope ps(ctx, "pn1t_identity");
        hipLaunchKernelGGL(pn1t_identity_kernel, dim3(blocks_for((size_t)P.n_obj * k)), dim3(T_BLOCK), 0, ctx->stream, P.z[first + 5], (size_t)P.n_obj, k);
    }

    // cur holds the gradient of the T-Net's matrices; with need_dx, cur <- the gradient of x
    void tnet_bwd(uint32_t first, const float* x, const float* feat, const uint32_t* arg, bool need_dx)
    {
        bwd(first + 5, P.y[first + 4], P.n_obj, false, true);
        bwd(first + 4, P.y[first + 3], P.n_obj, true, true);
        bwd(first + 3, feat, P.n_obj, true, true);
        max_back(cur, arg, P.rows, P.npts, t->layers[first + 2].N);
        bwd(first + 2, P.y[first + 1], P.rows, true, true);
        bwd(first + 1, P.y[first], P.rows, true, true);
        bwd(first, x, P.rows, true, need_dx);
    }

    // nxt <- dT[b] = x[b]^T dy[b] (the first k columns of rows `width` wide): one f32 chain from +0 over the ascending rows of object b
    void grad_t(const float* x, uint32_t width, uint32_t k)
    {
        if (rc) return;
        GemmArgs g;
        g.a = x; g.b = cur; g.init = nullptr; g.c = nxt;
        g.M = k; g.N = k; g.Kt = P.rows; g.chunk = P.npts;
        g.sai = 1; g.sak = width; g.sbk = width; g.sbj = 1; g.c_stride = (size_t)k * k;
        rc = launch_gemm(ctx, "pn1t_gemm_dt", g, who);
    }

    void transform(const float* x, const float* T, uint32_t K, bool transposed, float* y)
    {
        if (rc) return;
        const uint32_t KT = (K + 15u) / 16u, KM = (K + 3u) / 4u;
        ProfScope ps(ctx, "pn1t_transform");
        hipLaunchKernelGGL(pn1t_transform_kernel, dim3((P.npts + 63u) / 64u, P.n_obj), dim3(T_BLOCK), (size_t)KM * KT * 64u * 4u, ctx->stream, x, T, P.npts, K,
                           transposed ? 1u : K, transposed ? K : 1u, y);
    }

    void add(const float* a, const float* b, size_t cells, float* out)
    {
        if (rc) return;
        ProfScope ps(ctx, "pn1t_add");
        hipLaunchKernelGGL(pn1t_add_kernel, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, a, b, cells, out);
    }
};

}  // namespace

int pcr::pn1_trainer_info(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, pcr_pn2_train_info* info)
{
    trainer_info_common(t, info);
    info->keep_per_object = keep_width(t->desc1);
    if (n_obj && npts) {
        Plan1 P;
        if (!make_plan1(t, n_obj, npts, P)) return PCR_ERR_ARG;
        info->device_bytes = P.total + 2 * t->n_weights * 4;
    }
    return PCR_OK;
}

extern "C" int pcr_pn1_trainer_create(pcr_ctx* ctx, const pcr_pn1_desc* desc, const float* weights, size_t n_weights, double dropout_p, double bn_momentum,
                                      double reg_scale, uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, "pcr_pn1_trainer_create");
    std::unique_ptr<pcr_pn2_trainer> t(new pcr_pn2_trainer());
    memset(&t->desc, 0, sizeof(t->desc));
    t->kind = 1;
    t->desc1 = *desc;
    t->desc.bn_eps = desc->bn_eps;
    Pn1Layers ly;                            // the layers a model of the same descriptor has
    if (!pn1_layers(*desc, ly)) return fail(ctx, PCR_ERR_ARG, "pcr_pn1_trainer_create: a descriptor outside the limits (see include/pcr.h)");
    for (const LayerShape& s : ly.shapes) layer_push(*t, s);
    t->stn_first = ly.stn_first; t->enc_first = ly.enc_first; t->fstn_first = ly.fstn_first; t->head_first = ly.head_first;
    t->reg_scale = reg_scale;
    const double ps[PCR_PN2_MAX_FC] = { dropout_p, dropout_p, dropout_p, dropout_p };      // one p: the dropped layer's, whichever it is
    return trainer_finish(ctx, "pcr_pn1_trainer_create", std::move(t), std::isfinite(reg_scale) ? nullptr : ": reg_scale must be finite", weights, n_weights, ps,
                          PCR_PN2_MAX_FC, bn_momentum, chunk_rows, out);
}

namespace {

// the pass, and behind it (step_lr) the optimiser's update: pcr_pointnet_train_grad_f32 (grad wanted) and pcr_pointnet_train_step_f32 (grad optional)
int train_pass1(pcr_ctx* ctx, pcr_pn2_trainer* t, const char* who, const float* objects, size_t n_obj, size_t npts, const int32_t* target, uint64_t seed,
                const uint8_t* keep, double* loss, float* logp, float* trans, float* trans_feat, float* grad, const double* step_lr)
{
    const char* own_bad = t && t->kind == 1 && ((trans && !t->desc1.stn3) || (trans_feat && !t->desc1.fstn)) ? ": trans / trans_feat must be NULL when the model has no such T-Net" : nullptr;
    if (!own_bad && t && step_lr) own_bad = optim_bad(t, *step_lr);
    Plan1 P;
    bool run;
    int rc = call_head(ctx, t, 1, who, own_bad, !objects || !target || !loss || !logp || (!grad && !step_lr), target, n_obj, npts, P,
                       [&]() -> const char* { return make_plan1(t, n_obj, npts, P) ? nullptr : ": too large"; }, run, !step_lr);
    if (!run) return rc;
    const pcr_pn1_desc& d = t->desc1;
    const uint32_t C0 = 3 + d.D0, K = d.widths[0], n_class = t->layers.back().N, kw = keep_width(d);
    const size_t rows = n_obj * npts;
    for (size_t i = 0; i < rows * C0; i++) {
        if (!(fabsf(objects[i]) <= FLT_MAX)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a non-finite coordinate or feature").c_str());
        P.obj[i] = objects[i];
    }
    for (size_t e = 0; e < n_obj * kw; e++) P.keep[e] = keep ? (keep[e] ? 1 : 0) : keep_rule(seed, d.n_fc - 2u, e, t->drop_p[d.n_fc - 2u]);      // the mask: the caller's bytes, or the rule
    rc = call_upload(ctx, t, P);
    if (rc) return rc;
    ClsRun R(ctx, t, P, who);
    const uint32_t M = P.rows, nm = d.n_mlp, e0 = t->enc_first, s0 = t->stn_first, f0 = t->fstn_first, h0 = t->head_first;
    const uint32_t drop_layer = d.n_fc >= 2 ? h0 + d.n_fc - 2 : T_NONE;
    const float *T3 = nullptr, *TK = nullptr;
    // ---- forward
    const float* xt = P.obj;
    if (d.stn3) {
        R.tnet_fwd(s0, P.obj, 3, P.feat_s, P.arg_s);
        T3 = P.z[s0 + 5];
        if (R.rc == PCR_OK) {
            ProfScope ps(ctx, "pn1t_transform3");
            hipLaunchKernelGGL(pn1t_transform3_kernel, dim3(blocks_for(rows)), dim3(T_BLOCK), 0, ctx->stream, P.obj, T3, rows, (uint32_t)npts, C0, P.xt);
        }
        xt = P.xt;
    }
    R.fwd(e0, xt, M, true);
    const float* xf = P.y[e0];
    if (d.fstn) {
        R.tnet_fwd(f0, P.y[e0], K, P.feat_f, P.arg_f);
        TK = P.z[f0 + 5];
        R.transform(P.y[e0], TK, K, false, P.xf);
        xf = P.xf;
    }
    for (uint32_t i = 1; i < nm; i++) R.fwd(e0 + i, i == 1 ? xf : P.y[e0 + i - 1], M, i + 1 < nm);
    const uint32_t Cg = d.widths[nm - 1];
    if (R.rc == PCR_OK) {
        ProfScope ps(ctx, "pn1t_smax");
        hipLaunchKernelGGL(pn1t_smax_kernel, dim3(blocks_for(n_obj * Cg)), dim3(T_BLOCK), 0, ctx->stream, P.y[e0 + nm - 1], (uint32_t)n_obj, (uint32_t)npts, Cg, P.gfeat, P.garg);
    }
    for (uint32_t i = 0; i < d.n_fc; i++)
        R.fwd(h0 + i, i == 0 ? P.gfeat : P.y[h0 + i - 1], (uint32_t)n_obj, true, h0 + i == drop_layer ? Drop::pre_bn : Drop::none, P.keep);
    // ---- the loss
    if (R.rc == PCR_OK) {
        {
            ProfScope ps(ctx, "pn2t_loss");
            hipLaunchKernelGGL(pn2t_loss_kernel, dim3(1), dim3(T_BLOCK), 0, ctx->stream, P.z[h0 + d.n_fc - 1], P.target, (uint32_t)n_obj, n_class, P.logp, R.cur, P.loss + 1);
        }
        if (d.fstn) {
            ProfScope ps(ctx, "pn1t_reg");
            hipLaunchKernelGGL(pn1t_reg_kernel, dim3((unsigned)n_obj), dim3(T_BLOCK), 0, ctx->stream, TK, K, (uint32_t)n_obj, t->reg_scale, P.Mb, P.norm, P.dA);
        }
        ProfScope ps(ctx, "pn1t_loss_fin");
        hipLaunchKernelGGL(pn1t_loss_fin_kernel, dim3(1), dim3(64), 0, ctx->stream, d.fstn ? P.norm : (const double*)nullptr, (uint32_t)n_obj, t->reg_scale, P.loss);
    }
    // ---- backward
    for (uint32_t i = d.n_fc; i-- > 0;)
        R.bwd(h0 + i, i == 0 ? P.gfeat : P.y[h0 + i - 1], (uint32_t)n_obj, true, true, h0 + i == drop_layer ? Drop::pre_bn : Drop::none, P.keep);
    R.max_back(R.cur, P.garg, M, (uint32_t)npts, Cg);
    for (uint32_t i = nm; i-- > 1;) R.bwd(e0 + i, i == 1 ? xf : P.y[e0 + i - 1], M, i + 1 < nm, true);
    if (d.fstn) {                                                // cur: the gradient of the transformed rows
        const size_t tc = n_obj * (size_t)K * K;
        R.grad_t(P.y[e0], K, K);                                 // nxt <- dT through the transform
        R.add(R.nxt, P.dA, tc, R.nxt);                           //      + the regulariser's dA
        R.transform(R.cur, TK, K, true, P.g1);                   // the transform's path into conv 0's activation
        std::swap(R.cur, R.nxt);
        R.tnet_bwd(f0, P.y[e0], P.feat_f, P.arg_f, true);        // cur <- the T-Net's path
        R.add(P.g1, R.cur, (size_t)M * K, R.cur);                // the transform's path + the T-Net's path
    }
    R.bwd(e0, xt, M, true, d.stn3 != 0);
    if (d.stn3) {
        R.grad_t(P.obj, C0, 3);
        std::swap(R.cur, R.nxt);
        R.tnet_bwd(s0, P.obj, P.feat_s, P.arg_s, false);
    }
    return call_tail(ctx, t, who, R.rc, P, n_obj, logp, loss, 3, grad, { { trans, T3, n_obj * 9 * 4 }, { trans_feat, TK, n_obj * (size_t)K * K * 4 } }, step_lr);
}

}  // namespace

extern "C" int pcr_pointnet_train_grad_f32(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* objects, size_t n_obj, size_t npts, const int32_t* target, uint64_t seed,
                                           const uint8_t* keep, double* loss, float* logp, float* trans, float* trans_feat, float* grad)
{
    return train_pass1(ctx, t, "pcr_pointnet_train_grad_f32", objects, n_obj, npts, target, seed, keep, loss, logp, trans, trans_feat, grad, nullptr);
}

extern "C" int pcr_pointnet_train_step_f32(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* objects, size_t n_obj, size_t npts, const int32_t* target, uint64_t seed,
                                           const uint8_t* keep, double lr, double* loss, float* logp, float* trans, float* trans_feat, float* grad)
{
    return train_pass1(ctx, t, "pcr_pointnet_train_step_f32", objects, n_obj, npts, target, seed, keep, loss, logp, trans, trans_feat, grad, &lr);
}
