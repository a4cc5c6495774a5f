// pointnet2_train.hip — the training pass of HomeworkFinal's PointNet++ classifiers, single-scale (SSG) and multi-scale (MSG): training-mode forward, loss,
// the gradient of every parameter (models/pointnet2_cls_ssg.py, models/pointnet2_cls_msg.py, get_loss; train_cls.py's step without its optimiser).  The
// contracts are written out above pcr_pn2_trainer_create and pcr_pn2_msg_trainer_create in include/pcr.h.  There is ONE pass, over the superset descriptor:
// an SSG trainer is the case of one xyz-first branch per layer and one dropout probability.
// pcr_pn2_train_step_f32 is the same pass with the optimiser's update (pointnet_optim.hip) behind its last kernel and the gradient download optional.
//
// Batch statistics break the eval pass's layer fusion: the pass goes layer by layer and keeps every layer's z and y in HBM.  This file holds the model's
// own part: its plan's sampling and per-(stage, branch) buffers, FPS / centres / ball query once per stage, then per branch the gather, the layers and the max
// into the branch's columns of the stage's concatenated row; backward per branch the max's scatter from those columns, the layers, and the branch's part of
// the gather back.  The layer step (LayerRun), the plan base, the create / info / call head and tail and the kernels live in pointnet_train_common.hpp,
// which the vanilla PointNet's pass (pointnet_train.hip) includes too:
//   pn2t_gather        the padded rows of one branch: (xyz - centre | features) or (features | xyz - centre) per row, and the point every row read
//   pn2t_gemm_fwd      z = x W^T + b        one wave = 32 rows x 64 outputs on v_mfma_f32_16x16x4_f32, the accumulators start at the bias; every
//   pn2t_gemm_dx       dx = dz W            MFMA takes four consecutive k, so an output is ONE fma chain over ascending k (channel, output or row)
//   pn2t_gemm_dw       dW partials = dz^T x one chain over the rows of a chunk per (chunk, output, input), from +0
//   pn2t_dw_reduce     dW = the chunk partials added in ascending order (f32)
//   pn2t_stat_part / pn2t_stat_fin     f64 sums per (chunk, channel) over ascending rows, then over ascending chunks: mean, variance (two passes),
//                      the running statistics; also the bias gradient of the last FC layer
//   pn2t_bn_relu       y = relu(BN(z)) and, in the head, the layer's dropout
//   pn2t_max / pn2t_max_back            the max over a group with the lowest position among the maxima, into a column slice of the stage's row / its gradient
//   pn2t_bnb_part / pn2t_bnb_fin / pn2t_bnb_dz      dropout, ReLU and BatchNorm backward: dbeta, dgamma, then dz in place of dy
//   pn2t_gather_back   the gradient of a layer's input features summed per point over the rows of every branch that read it, in f64: one launch per
//                      branch, branches ascending, the sum handed on in f64 and rounded by the last
//   pn2t_loss          log_softmax, the loss, dlogits
// No floating-point atomic anywhere; every sum over rows is ordered by the row index and chunk_rows alone.
#include "pointnet_train_common.hpp"

namespace {

// one branch of a stage: its layers, its rows, its columns [off, off + the last layer's width) of the stage's row
struct Branch {
    uint32_t first, count;       // its layers
    uint32_t M;                  // rows
    uint32_t gsize;              // rows per group (head: 0, no max)
    uint32_t off;
};

// the stages of one call: every SA layer, then the head (one "branch" without a max)
struct Stage {
    uint32_t groups, n_branch;
    Branch br[PCR_PN2_MAX_BRANCH];
    bool head() const { return br[0].gsize == 0; }
};

// the device block of one call: PlanBase's, with the sampling buffers in `own` and one more Layout per SA stage behind the layers'
struct Plan : PlanBase {
    size_t N[PCR_PN2_MAX_SA + 1];
    std::vector<Stage> stages;
    // uploaded
    float *x0 = nullptr, *feat0 = nullptr;
    uint32_t *seg[PCR_PN2_MAX_SA + 1], *cseg[PCR_PN2_MAX_SA];
    // sampling: bidx holds the branches' row blocks one after the other (block b = centres x nsample_b), bcnt n_branch x centres
    uint32_t *fps[PCR_PN2_MAX_SA], *bidx[PCR_PN2_MAX_SA], *bcnt[PCR_PN2_MAX_SA];
    float* cxyz[PCR_PN2_MAX_SA];
    // per (SA stage, branch), and per SA stage at the concatenated width
    float *xin[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH], *feat[PCR_PN2_MAX_SA];
    uint32_t *row_pt[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH], *arg[PCR_PN2_MAX_SA];
};

// false: too large
bool make_plan(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, Plan& P)
{
    const pcr_pn2_msg_desc& d = t->desc;
    const uint32_t ns = t->n_sampling, C0 = 3 + d.D0;
    if (n_obj > PN_MAX_ROWS || npts > PN_MAX_ROWS || (unsigned long long)n_obj * npts > PN_MAX_ROWS / C0) return false;
    P.N[0] = npts;
    for (uint32_t l = 0; l < d.n_sa; l++) {
        const pcr_pn2_msg_sa_desc& sd = d.sa[l];
        Stage st;
        memset(&st, 0, sizeof(st));
        if (!sd.group_all) P.N[l + 1] = sd.npoint;
        const unsigned long long groups = sd.group_all ? n_obj : (unsigned long long)n_obj * sd.npoint;
        if (groups > PN_MAX_ROWS) return false;
        st.groups = (uint32_t)groups;
        st.n_branch = sd.n_branch;
        uint32_t off = 0;
        for (uint32_t b = 0; b < sd.n_branch; b++) {
            const uint32_t gsize = sd.group_all ? (uint32_t)P.N[l] : sd.branch[b].nsample;
            const unsigned long long rows = (unsigned long long)st.groups * gsize;
            unsigned long long widest = t->sa_in[l];             // the widest row of the branch, its input included
            for (uint32_t i = 0; i < sd.branch[b].n_mlp; i++) widest = std::max<unsigned long long>(widest, sd.branch[b].widths[i]);
            if (rows > (1ull << 21) || rows * widest > PN_MAX_ROWS) return false;      // 2^21 rows, and every buffer's cells within PN_MAX_ROWS
            st.br[b] ={ t->sa_first[l][b], sd.branch[b].n_mlp, (uint32_t)rows, gsize, off };
            off += sd.branch[b].widths[sd.branch[b].n_mlp - 1];
        }
        P.stages.push_back(st);
    }
    {
        Stage st;
        memset(&st, 0, sizeof(st));
        st.groups = (uint32_t)n_obj;
        st.n_branch = 1;
        st.br[0] = { t->head_first, d.n_fc, (uint32_t)n_obj, 0u, 0u };
        P.stages.push_back(st);
    }
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
        size_t row = 0;
        for (uint32_t b = 0; b < d.sa[l].n_branch; b++) row += d.sa[l].branch[b].nsample;
        P.own.add(&P.fps[l], nq);
        P.own.add(&P.cxyz[l], 3 * nq);
        P.own.add(&P.bidx[l], nq * row);
        P.own.add(&P.bcnt[l], nq * d.sa[l].n_branch);
    }
    const size_t nl = t->layers.size();
    P.layers(nl, d.n_sa);
    P.dfeat_cells = 1;
    for (size_t s = 0; s < P.stages.size(); s++) {
        const Stage& st = P.stages[s];
        const bool head = st.head();
        if (!head) {
            Layout& L = P.per_layer[nl + s];
            for (uint32_t b = 0; b < st.n_branch; b++) {
                L.add(&P.xin[s][b], (size_t)st.br[b].M * t->sa_in[s]);
                L.add(&P.row_pt[s][b], (size_t)st.br[b].M);
            }
            L.add(&P.feat[s], (size_t)st.groups * t->sa_out[s]);
            L.add(&P.arg[s], (size_t)st.groups * t->sa_out[s]);
            P.dfeat_cells = std::max(P.dfeat_cells, (size_t)st.groups * t->sa_out[s]);
            if (s > 0 && st.n_branch > 1) P.dacc_cells = std::max(P.dacc_cells, n_obj * P.N[s] * (t->sa_in[s] - 3));
        }
        for (uint32_t b = 0; b < st.n_branch; b++)
            for (uint32_t i = st.br[b].first; i < st.br[b].first + st.br[b].count; i++) P.add_layer(i, st.br[b].M, t->layers[i], t->chunk_rows, head);
    }
    P.finish(n_obj, t->layers.back().N, 1);
    return true;
}

// what both creates share: the layers of the superset descriptor, the group_all rule, the upload
int create_from(pcr_ctx* ctx, const char* who, const pcr_pn2_msg_desc& md, const float* weights, size_t n_weights, const double* dropout_p, size_t n_dropout,
                double bn_momentum, uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    std::unique_ptr<pcr_pn2_trainer> t(new pcr_pn2_trainer());
    t->desc = md;
    Pn2Layers ly;
    if (!pn2_layers(md, ly)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a descriptor outside the limits (see include/pcr.h)").c_str());
    for (const LayerShape& s : ly.shapes) layer_push(*t, s);
    for (uint32_t l = 0; l < md.n_sa; l++) {
        for (uint32_t b = 0; b < md.sa[l].n_branch; b++) t->sa_first[l][b] = ly.first[l][b];
        t->sa_in[l] = ly.sa_in[l];
        t->sa_out[l] = ly.sa_out[l];
    }
    t->head_first = ly.head_first;
    t->n_sampling = ly.n_sampling;
    if (!md.sa[md.n_sa - 1].group_all) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": the last SA layer must be group_all").c_str());
    return trainer_finish(ctx, who, std::move(t), nullptr, weights, n_weights, dropout_p, n_dropout, bn_momentum, chunk_rows, out);
}

}  // namespace

extern "C" int pcr_pn2_trainer_create(pcr_ctx* ctx, const pcr_pn2_desc* desc, const float* weights, size_t n_weights, double dropout_p, double bn_momentum,
                                      uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    const char* who = "pcr_pn2_trainer_create";
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, who);
    pcr_pn2_msg_desc md;                     // the models' superset descriptor: the trainer's layers are the ones a model of the same descriptor has
    if (!pn2_msg_desc_of(*desc, md)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_create: a descriptor outside the limits (see include/pcr.h)");
    const double ps[PCR_PN2_MAX_FC] = { dropout_p, dropout_p, dropout_p, dropout_p };      // every hidden layer's
    return create_from(ctx, who, md, weights, n_weights, ps, PCR_PN2_MAX_FC, bn_momentum, chunk_rows, out);
}

extern "C" int pcr_pn2_msg_trainer_create(pcr_ctx* ctx, const pcr_pn2_msg_desc* desc, const float* weights, size_t n_weights, const double* dropout_p, size_t n_dropout,
                                          double bn_momentum, uint32_t chunk_rows, pcr_pn2_trainer** out)
{
    const char* who = "pcr_pn2_msg_trainer_create";
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, who);
    if (desc->n_fc < 1 || desc->n_fc > PCR_PN2_MAX_FC) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_msg_trainer_create: a descriptor outside the limits (see include/pcr.h)");
    if (n_dropout != desc->n_fc - 1) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_msg_trainer_create: n_dropout must be n_fc - 1, one p per hidden FC layer");
    if (n_dropout && !dropout_p) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_msg_trainer_create: dropout_p is NULL");
    return create_from(ctx, who, *desc, weights, n_weights, dropout_p, n_dropout, bn_momentum, chunk_rows, out);
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
    optim_free(t);
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

extern "C" int pcr_pn2_msg_trainer_info(const pcr_pn2_trainer* t, size_t n_obj, size_t npts, pcr_pn2_train_info* info, pcr_pn2_msg_desc* desc, double* dropout_p)
{
    if (!t || !info || t->kind != 0) return PCR_ERR_ARG;
    const int rc = pcr_pn2_trainer_info(t, n_obj, npts, info);
    if (rc) return rc;
    if (desc) *desc = t->desc;
    if (dropout_p)
        for (uint32_t i = 0; i + 1 < PCR_PN2_MAX_FC; i++) dropout_p[i] = i + 1 < t->desc.n_fc ? (double)t->drop_p[i] : 0.0;
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

namespace {

// the pass, and behind it (step_lr) the optimiser's update: pcr_pn2_train_grad_f32 (grad wanted) and pcr_pn2_train_step_f32 (grad optional)
int train_pass(pcr_ctx* ctx, pcr_pn2_trainer* t, const char* who, const float* objects, size_t n_obj, size_t npts, const int32_t* target, const uint32_t* starts,
               uint64_t seed, const uint8_t* keep, double* loss, float* logp, float* grad, const double* step_lr)
{
    Plan P;
    std::vector<uint32_t> st0;               // the first FPS pick of every (sampling layer, object)
    bool run;
    const char* own_bad = t && step_lr ? optim_bad(t, *step_lr) : nullptr;
    int rc = call_head(ctx, t, 0, who, own_bad, !objects || !target || !loss || !logp || (!grad && !step_lr), target, n_obj, npts, P, [&]() -> const char* {
        if (!make_plan(t, n_obj, npts, P)) return ": too large";
        for (const Stage& st : P.stages)
            for (uint32_t b = 0; b < st.n_branch; b++)
                if (st.br[b].M < 2) return ": a layer with one row (BatchNorm's batch statistics need two)";
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
    }, run, !step_lr);
    if (!run) return rc;
    const pcr_pn2_msg_desc& d = t->desc;
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
        for (uint32_t i = 0; i + 1 < d.n_fc; i++) {              // the masks: the caller's bytes, or the rule with the layer's own p
            const size_t cells = n_obj * d.fc_widths[i];
            for (size_t e = 0; e < cells; e++) P.keep[off + e] = keep ? (keep[off + e] ? 1 : 0) : keep_rule(seed, i, e, t->drop_p[i]);
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
        const bool head = st.head(), grouped = s < ns;
        const float *qx = nullptr, *qy = nullptr, *qz = nullptr;
        const uint32_t* bidx[PCR_PN2_MAX_BRANCH] = {};           // the branches' row blocks
        if (grouped) {                                           // once per stage: FPS, the centres, every branch's ball in one walk
            const pcr_pn2_msg_sa_desc& sd = d.sa[s];
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
            double radii[PCR_PN2_MAX_BRANCH];
            uint32_t nsamples[PCR_PN2_MAX_BRANCH], *ib[PCR_PN2_MAX_BRANCH], *cb[PCR_PN2_MAX_BRANCH];
            size_t at = 0;
            for (uint32_t b = 0; b < sd.n_branch; b++) {
                radii[b] = sd.branch[b].radius; nsamples[b] = sd.branch[b].nsample;
                ib[b] = P.bidx[s] + at; cb[b] = P.bcnt[s] + (size_t)b * nq;
                bidx[b] = ib[b];
                at += nq * nsamples[b];
            }
            if (sd.n_branch == 1) R.rc = ball_query_device(ctx, cx, cy, cz, wx, wy, wz, P.seg[s], P.cseg[s], nq, radii[0], nsamples[0], ib[0], cb[0]);
            else R.rc = ball_query_multi_device(ctx, cx, cy, cz, wx, wy, wz, P.seg[s], P.cseg[s], nq, sd.n_branch, radii, nsamples, ib, cb);
            if (R.rc) break;
            qx = wx; qy = wy; qz = wz;
        }
        for (uint32_t b = 0; b < st.n_branch && R.rc == PCR_OK; b++) {
            const Branch& br = st.br[b];
            const float* x = feat;
            if (!head) {
                ProfScope ps(ctx, "pn2t_gather");
                hipLaunchKernelGGL(pn2t_gather_kernel, dim3(blocks_for(br.M)), dim3(T_BLOCK), 0, ctx->stream, cx, cy, cz, qx, qy, qz, feat, bidx[b], br.M, grouped ? br.gsize : 1u,
                                   grouped ? d.sa[s].npoint : 1u, (uint32_t)P.N[s], D, d.sa[s].xyz_last, P.xin[s][b], P.row_pt[s][b]);
                x = P.xin[s][b];
            }
            for (uint32_t i = br.first; i < br.first + br.count; i++) {
                const TLayer& L = t->layers[i];
                if (head && L.bn) {
                    keep_of[i] = P.keep + keep_off;
                    keep_off += (size_t)br.M * L.N;
                }
                R.fwd(i, x, br.M, true, keep_of[i] ? Drop::fused : Drop::none, keep_of[i]);
                x = head ? P.a[i] : P.y[i];
            }
            if (R.rc) break;
            if (!head) {                                         // the branch's columns of the stage's row
                const uint32_t last = br.first + br.count - 1;
                ProfScope ps(ctx, "pn2t_max");
                hipLaunchKernelGGL(pn2t_max_kernel, dim3(blocks_for((size_t)st.groups * t->layers[last].N)), dim3(T_BLOCK), 0, ctx->stream, P.y[last], st.groups, br.gsize,
                                   t->layers[last].N, t->sa_out[s], br.off, P.feat[s], P.arg[s]);
            }
        }
        if (!head) {
            feat = P.feat[s];
            D = t->sa_out[s];
            if (grouped) { cx = qx; cy = qy; cz = qz; }
        }
    }
    // ---- the loss, then backward
    if (R.rc == PCR_OK) {
        ProfScope ps(ctx, "pn2t_loss");
        hipLaunchKernelGGL(pn2t_loss_kernel, dim3(1), dim3(T_BLOCK), 0, ctx->stream, P.z[t->layers.size() - 1], P.target, (uint32_t)n_obj, n_class, P.logp, R.cur, P.loss);
    }
    for (size_t s = P.stages.size(); s-- > 0 && R.rc == PCR_OK;) {
        const Stage& st = P.stages[s];
        const bool head = st.head();
        for (uint32_t b = 0; b < st.n_branch && R.rc == PCR_OK; b++) {
            const Branch& br = st.br[b];
            if (!head)      // the branch's columns of the gradient of the stage's row -> its last layer's rows.  Below the head, the head's dx IS that gradient
                R.max_back(s + 2 == P.stages.size() ? R.cur : P.dfeat, P.arg[s], br.M, br.gsize, t->layers[br.first + br.count - 1].N, t->sa_out[s], br.off);
            for (uint32_t i = br.first + br.count; i-- > br.first;) {
                const float* x = i > br.first ? (head ? P.a[i - 1] : P.y[i - 1]) : (head ? P.feat[s - 1] : P.xin[s][b]);
                R.bwd(i, x, br.M, true, head || s > 0 || i > br.first, keep_of[i] ? Drop::fused : Drop::none, keep_of[i]);      // the input points take no gradient
            }
            if (R.rc == PCR_OK && !head && s > 0) {              // the feature columns of dx back to the points of the stage before: this branch's part of the sum.
                                                                 // P.dfeat is free once the last branch has scattered its maxima, and only the last branch writes it
                const uint32_t Dp = t->sa_in[s] - 3;
                const uint32_t points = (uint32_t)(n_obj * P.N[s]);
                ProfScope ps(ctx, "pn2t_gather_back");
                hipLaunchKernelGGL(pn2t_gather_back_kernel, dim3(points), dim3(T_BLOCK), 0, ctx->stream, R.cur, P.row_pt[s][b], points, (uint32_t)P.N[s], br.M / (uint32_t)n_obj,
                                   Dp, d.sa[s].xyz_last ? 0u : 3u, b > 0 ? P.dacc : (const double*)nullptr, b + 1 < st.n_branch ? P.dacc : (double*)nullptr, P.dfeat);
            }
        }
    }
    return call_tail(ctx, t, who, R.rc, P, n_obj, logp, loss, 1, grad, {}, step_lr);      // `hold` lives until its wait is over
}

}  // namespace

extern "C" int pcr_pn2_train_grad_f32(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* objects, size_t n_obj, size_t npts, const int32_t* target, const uint32_t* starts,
                                      uint64_t seed, const uint8_t* keep, double* loss, float* logp, float* grad)
{
    return train_pass(ctx, t, "pcr_pn2_train_grad_f32", objects, n_obj, npts, target, starts, seed, keep, loss, logp, grad, nullptr);
}

extern "C" int pcr_pn2_train_step_f32(pcr_ctx* ctx, pcr_pn2_trainer* t, const float* objects, size_t n_obj, size_t npts, const int32_t* target, const uint32_t* starts,
                                      uint64_t seed, const uint8_t* keep, double lr, double* loss, float* logp, float* grad)
{
    return train_pass(ctx, t, "pcr_pn2_train_step_f32", objects, n_obj, npts, target, starts, seed, keep, loss, logp, grad, &lr);
}
