// pointnet2_train.hip — the training pass of HomeworkFinal's PointNet++ (SSG) classifier: training-mode forward, loss, the gradient of every
// parameter (models/pointnet2_cls_ssg.py, get_loss :50-52; train_cls.py's step without its optimiser).  The contract is written out above
// pcr_pn2_trainer_create in include/pcr.h.
//
// Batch statistics break the eval pass's layer fusion: the pass goes layer by layer and keeps every layer's z and y in HBM.  This file holds the SSG model's
// own part: its plan's sampling and per-stage buffers, FPS / centres / ball query / gather per stage, the max, the gather back.  The layer step
// (LayerRun), the plan base, the create / info / call head and tail and the kernels live in pointnet_train_common.hpp, which the vanilla PointNet's pass
// (pointnet_train.hip) includes too:
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

// the stages of one call: every SA layer, then the head
struct Stage {
    uint32_t first, count;       // its layers
    uint32_t M;                  // rows
    uint32_t gsize;              // rows per group (head: 0, no max)
    uint32_t groups;
};

// the device block of one call: PlanBase's, with the sampling buffers in `own` and one more Layout per SA stage behind the layers'
struct Plan : PlanBase {
    size_t N[PCR_PN2_MAX_SA + 1];
    std::vector<Stage> stages;
    // uploaded
    float *x0 = nullptr, *feat0 = nullptr;
    uint32_t *seg[PCR_PN2_MAX_SA + 1], *cseg[PCR_PN2_MAX_SA];
    // sampling
    uint32_t *fps[PCR_PN2_MAX_SA], *bidx[PCR_PN2_MAX_SA], *bcnt[PCR_PN2_MAX_SA];
    float* cxyz[PCR_PN2_MAX_SA];
    // per SA stage
    float *xin[PCR_PN2_MAX_SA], *feat[PCR_PN2_MAX_SA];
    uint32_t *row_pt[PCR_PN2_MAX_SA], *arg[PCR_PN2_MAX_SA];
};

// false: too large
bool make_plan(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, Plan& P)
{
    const pcr_pn2_desc& d = t->desc;
    const uint32_t ns = t->n_sampling, C0 = 3 + d.D0;
    if (n_obj > PN_MAX_ROWS || npts > PN_MAX_ROWS || (unsigned long long)n_obj * npts > PN_MAX_ROWS / C0) return false;
    P.N[0] = npts;
    for (uint32_t l = 0; l < ns; l++) {
        P.N[l + 1] = d.sa[l].npoint;
        const unsigned long long rows = (unsigned long long)n_obj * d.sa[l].npoint * d.sa[l].nsample;
        if (rows > PN_MAX_ROWS / PN_MAX_WIDTH) return false;
        P.stages.push_back({ t->sa_first[l], d.sa[l].n_mlp, (uint32_t)rows, d.sa[l].nsample, (uint32_t)(n_obj * d.sa[l].npoint) });
    }
    if (d.sa[d.n_sa - 1].group_all) {
        const unsigned long long rows = (unsigned long long)n_obj * P.N[ns];
        if (rows > PN_MAX_ROWS / PN_MAX_WIDTH) return false;
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
    for (uint32_t l = 0; l < ns; l++) {
        const size_t nq = n_obj * P.N[l + 1];
        P.own.add(&P.fps[l], nq);
        P.own.add(&P.cxyz[l], 3 * nq);
        P.own.add(&P.bidx[l], nq * d.sa[l].nsample);
        P.own.add(&P.bcnt[l], nq);
    }
    const size_t nl = t->layers.size();
    P.layers(nl, d.n_sa);
    P.dfeat_cells = 1;
    for (size_t s = 0; s < P.stages.size(); s++) {
        const Stage& st = P.stages[s];
        const bool head = st.gsize == 0;
        if (!head) {
            Layout& L = P.per_layer[nl + s];
            L.add(&P.xin[s], (size_t)st.M * t->sa_in[s]);
            L.add(&P.row_pt[s], (size_t)st.M);
            L.add(&P.feat[s], (size_t)st.groups * t->sa_out[s]);
            L.add(&P.arg[s], (size_t)st.groups * t->sa_out[s]);
            P.dfeat_cells = std::max(P.dfeat_cells, (size_t)st.groups * t->sa_out[s]);
        }
        for (uint32_t i = st.first; i < st.first + st.count; i++) P.add_layer(i, st.M, t->layers[i], t->chunk_rows, head);
    }
    P.finish(n_obj, t->layers.back().N, 1);
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
    pcr_pn2_msg_desc md;                     // the models' superset descriptor: the trainer's layers are the ones a model of the same descriptor has
    Pn2Layers ly;
    if (!pn2_msg_desc_of(*desc, md) || !pn2_layers(md, ly)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: a descriptor outside the limits (see include/pcr.h)");
    for (const LayerShape& s : ly.shapes) layer_push(*t, s);
    for (uint32_t l = 0; l < desc->n_sa; l++) { t->sa_first[l] = ly.first[l][0]; t->sa_in[l] = ly.sa_in[l]; t->sa_out[l] = ly.sa_out[l]; }
    t->head_first = ly.head_first;
    t->n_sampling = ly.n_sampling;
    if (!desc->sa[desc->n_sa - 1].group_all) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: the last SA layer must be group_all");
    return trainer_finish(ctx, "pcr_pn2_trainer_create", std::move(t), nullptr, weights, n_weights, dropout_p, bn_momentum, chunk_rows, out);
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
    trainer_info_common(t, info);
    info->n_sampling = t->n_sampling;
    for (uint32_t i = 0; i + 1 < t->desc.n_fc; i++) info->keep_per_object += t->desc.fc_widths[i];
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
    Plan P;
    std::vector<uint32_t> st0;               // the first FPS pick of every (sampling layer, object)
    bool run;
    int rc = call_head(ctx, t, 0, who, nullptr, !objects || !target || !loss || !logp || !grad, target, n_obj, npts, P, [&]() -> const char* {
        if (!make_plan(t, n_obj, npts, P)) return ": too large";
        for (const Stage& st : P.stages)
            if (st.M < 2) return ": a layer with one row (BatchNorm's batch statistics need two)";
        st0.resize((size_t)t->n_sampling * n_obj);
        for (uint32_t l = 0; l < t->n_sampling; l++)
            for (size_t o = 0; o < n_obj; o++) {
                uint32_t v;
                if (starts) {
                    v = starts[(size_t)l * n_obj + o];
                    if (v >= P.N[l]) return ": a start outside its object";
                } else {
                    v = (uint32_t)(splitmix_key(seed, ((unsigned long long)(l + 1) << 32) | (unsigned long long)o) % (unsigned long long)P.N[l]);
                }
                st0[(size_t)l * n_obj + o] = v;
            }
        return nullptr;
    }, run);
    if (!run) return rc;
    const pcr_pn2_desc& d = t->desc;
    const uint32_t ns = t->n_sampling, D0 = d.D0, C0 = 3 + D0, n_class = t->layers.back().N;
    const size_t pts = n_obj * npts;
    {
        float *hx = P.x0, *hy = P.x0 + pts, *hz = P.x0 + 2 * pts;
        for (size_t i = 0; i < pts; i++) {
            const float* r = objects + i * C0;
            for (uint32_t c = 0; c < C0; c++)
                if (!(fabsf(r[c]) <= FLT_MAX)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a non-finite coordinate or feature").c_str());
            hx[i] = r[0]; hy[i] = r[1]; hz[i] = r[2];
            for (uint32_t c = 0; c < D0; c++) P.feat0[i * D0 + c] = r[3 + c];
        }
        size_t off = 0;
        for (uint32_t i = 0; i + 1 < d.n_fc; i++) {              // the masks: the caller's bytes, or the rule
            const size_t cells = n_obj * d.fc_widths[i];
            for (size_t e = 0; e < cells; e++) P.keep[off + e] = keep ? (keep[off + e] ? 1 : 0) : keep_rule(seed, i, e, t->dropout_p);
            off += cells;
        }
        for (uint32_t l = 0; l <= ns; l++)
            for (size_t o = 0; o <= n_obj; o++) P.seg[l][o] = (uint32_t)(o * P.N[l]);
        for (uint32_t l = 0; l < ns; l++)
            for (size_t q = 0; q < n_obj * P.N[l + 1]; q++) P.cseg[l][q] = (uint32_t)(q / P.N[l + 1]);
    }
    rc = call_upload(ctx, t, P);
    if (rc) return rc;
    LayerRun R(ctx, t, P, who, launch_gemm, "pn2t_gemm_fwd", "pn2t_gemm_dx");
    HostKeep hold;
    // ---- forward
    const float *cx = P.x0, *cy = P.x0 + pts, *cz = P.x0 + 2 * pts, *feat = P.feat0;
    uint32_t D = D0;
    size_t keep_off = 0;
    std::vector<const uint8_t*> keep_of(t->layers.size(), nullptr);      // the mask of every head layer that has a dropout (fused behind its ReLU)
    for (size_t s = 0; s < P.stages.size() && R.rc == PCR_OK; s++) {
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
                R.rc = fps_device(ctx, cx, cy, cz, std::move(jobs), sd.npoint, PCR_FPS_F32, P.fps[s], &hold);
                if (R.rc) break;
                float *wx = P.cxyz[s], *wy = wx + nq, *wz = wy + nq;
                {
                    ProfScope ps(ctx, "pn2t_centres");
                    hipLaunchKernelGGL(pn2t_centres_kernel, dim3(blocks_for(nq)), dim3(T_BLOCK), 0, ctx->stream, cx, cy, cz, P.fps[s], (uint32_t)P.N[s], sd.npoint, (uint32_t)nq,
                                       wx, wy, wz);
                }
                R.rc = ball_query_device(ctx, cx, cy, cz, wx, wy, wz, P.seg[s], P.cseg[s], nq, sd.radius, sd.nsample, P.bidx[s], P.bcnt[s]);
                if (R.rc) break;
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
        for (uint32_t i = st.first; i < st.first + st.count; i++) {
            const TLayer& L = t->layers[i];
            if (head && L.bn) {
                keep_of[i] = P.keep + keep_off;
                keep_off += (size_t)st.M * L.N;
            }
            R.fwd(i, x, st.M, true, keep_of[i] ? Drop::fused : Drop::none, keep_of[i]);
            x = head ? P.a[i] : P.y[i];
        }
        if (R.rc) break;
        if (!head) {
            const uint32_t last = st.first + st.count - 1, C = t->layers[last].N;
            ProfScope ps(ctx, "pn2t_max");
            hipLaunchKernelGGL(pn2t_max_kernel, dim3(blocks_for((size_t)st.groups * C)), dim3(T_BLOCK), 0, ctx->stream, P.y[last], st.groups, st.gsize, C, P.feat[s], P.arg[s]);
            feat = P.feat[s];
            D = C;
        }
    }
    // ---- the loss, then backward
    if (R.rc == PCR_OK) {
        ProfScope ps(ctx, "pn2t_loss");
        hipLaunchKernelGGL(pn2t_loss_kernel, dim3(1), dim3(T_BLOCK), 0, ctx->stream, P.z[t->layers.size() - 1], P.target, (uint32_t)n_obj, n_class, P.logp, R.cur, P.loss);
    }
    for (size_t s = P.stages.size(); s-- > 0 && R.rc == PCR_OK;) {
        const Stage& st = P.stages[s];
        const bool head = st.gsize == 0;
        if (!head)      // the gradient of the stage's output -> its last layer's rows.  Below the head, the head's dx IS the gradient of the global feature
            R.max_back(s + 2 == P.stages.size() ? R.cur : P.dfeat, P.arg[s], st.M, st.gsize, t->layers[st.first + st.count - 1].N);
        for (uint32_t i = st.first + st.count; i-- > st.first;) {
            const float* x = i > st.first ? (head ? P.a[i - 1] : P.y[i - 1]) : (head ? P.feat[s - 1] : P.xin[s]);
            R.bwd(i, x, st.M, true, i != 0, keep_of[i] ? Drop::fused : Drop::none, keep_of[i]);      // layer 0: the input points take no gradient
        }
        if (R.rc == PCR_OK && !head && s > 0) {                  // the feature columns of dx back to the points of the stage before
            const uint32_t Dp = t->sa_in[s] - 3;
            const uint32_t points = (uint32_t)(n_obj * P.N[s]);
            ProfScope ps(ctx, "pn2t_gather_back");
            hipLaunchKernelGGL(pn2t_gather_back_kernel, dim3(points), dim3(T_BLOCK), 0, ctx->stream, R.cur, P.row_pt[s], points, (uint32_t)P.N[s], st.M / (uint32_t)n_obj, Dp, P.dfeat);
        }
    }
    return call_tail(ctx, t, who, R.rc, P, n_obj, logp, loss, 1, grad);      // `hold` lives until its wait is over
}
