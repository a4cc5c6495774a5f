// pointnet2_train.hip — the training pass of HomeworkFinal's PointNet++ (SSG) classifier: training-mode forward, loss, the gradient of every
// parameter (models/pointnet2_cls_ssg.py, get_loss :50-52; train_cls.py's step without its optimiser).  The contract is written out above
// pcr_pn2_trainer_create in include/pcr.h.
//
// Batch statistics break the eval pass's layer fusion: the pass goes layer by layer and keeps every layer's z and y in HBM.  The kernels live in
// pointnet_train_common.hpp, which the vanilla PointNet's pass (pointnet_train.hip) includes too:
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
#include "pointnet_train_common.hpp"

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
    if (t->kind == 1) return pn1_trainer_info(t, n_obj, npts, info);
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
    if (t->kind != 0) return bad(": the trainer was made by pcr_pn1_trainer_create (use pcr_pointnet_train_grad_f32)");
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
                hipLaunchKernelGGL(pn2t_bn_relu_kernel<true>, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, P.z[i], cells, L.N, mu, rstd, W + L.gamma, W + L.beta, P.y[i], kp,
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
                hipLaunchKernelGGL(pn2t_bnb_part_kernel<true>, dim3(blocks_for((size_t)chunks * L.N)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], keep_of[i], drop_s, st.M, L.N,
                                   chunk, chunks, mu, rstd, P.part);
                hipLaunchKernelGGL(pn2t_bnb_fin_kernel, dim3(blocks_for(L.N)), dim3(T_BLOCK), 0, ctx->stream, P.part, chunks, L.N, st.M, G + L.gamma, G + L.beta, mg, mgx);
                hipLaunchKernelGGL(pn2t_bnb_dz_kernel<true>, dim3(blocks_for(cells)), dim3(T_BLOCK), 0, ctx->stream, cur, P.y[i], P.z[i], keep_of[i], drop_s, cells, L.N, mu, rstd,
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
