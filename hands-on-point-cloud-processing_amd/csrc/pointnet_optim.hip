// pointnet_optim.hip — the optimiser of the PointNet trainers: torch.optim.Adam (amsgrad off, coupled weight decay) and torch.optim.SGD (momentum,
// dampening, weight decay, no nesterov) as train_cls.py:147-155 builds them, on the device, for every trainer kind at once.  The contract is written out
// above pcr_pn2_trainer_optim_set in include/pcr.h.
//
// The state (exp_avg, exp_avg_sq / momentum_buffer) is f32 in the weight layout beside w_dev and grad_dev; the step count is a host integer.  ONE launch per
// update over the flat array, on the context's stream:
//   pnopt_adam / pnopt_sgd     a workgroup takes tiles of OPT_TILE consecutive elements, the tiles 16-byte aligned in the ARRAY (not in a layer: a layer starts
//                              anywhere).  A tile that lies inside one parameter range takes four 16-byte loads and three 16-byte stores per thread; a tile
//                              inside the running statistics is skipped; a tile that holds a border, or the array's end, goes element by element against the
//                              range table.  Every element is evaluated in f64 from its own f32 values: the bits depend on nothing else.
// The range table (opt_ranges) lists the PARAMETERS of the flat array, ascending and merged: everything but the running_mean / running_var slots, which the
// kernel neither reads nor writes.
#include "pointnet_train_common.hpp"

namespace {

constexpr int OPT_VEC = 4;
constexpr uint32_t OPT_TILE = T_BLOCK * OPT_VEC;      // elements per workgroup and trip
constexpr unsigned OPT_MAX_BLOCKS = 1024;             // four workgroups a CU; the rest of the array by grid stride

struct OptRange { uint64_t begin, end; };             // elements [begin, end) are parameters

struct OptArgs {
    float* w;
    const float* g;
    float *s0, *s1;
    const OptRange* ranges;
    uint32_t n_ranges;
    int first;               // SGD: the update that sets the buffer
    uint64_t n;
    double step;             // Adam: lr / (1 - beta1^t); SGD: lr
    double wd;
    double c1, b2, c2;       // Adam: 1 - beta1, beta2, 1 - beta2
    double sbc2, eps;        // Adam: sqrt(1 - beta2^t), eps
    double mu, cd;           // SGD: momentum, 1 - dampening
};

// the parameter ranges of a trainer's flat array: per layer [w, b, gamma, beta] (without BatchNorm: [w, b]); neighbours merged
std::vector<OptRange> build_ranges(const pcr_pn2_trainer* t)
{
    std::vector<OptRange> out;
    for (const TLayer& L : t->layers) {
        const uint64_t b = L.w, e = L.bn ? L.rmean : L.b + L.N;
        if (e == b) continue;
        if (!out.empty() && out.back().end == b) out.back().end = e;
        else out.push_back({ b, e });
    }
    return out;
}

// one element, in f64 from the f32 state, every operation rounded on its own (no contraction), every stored value rounded once
template <int KIND>
__device__ __forceinline__ void opt_element(const OptArgs& a, float& w, float g, float& s0, float& s1)
{
    const double wv = (double)w;
    const double gp = (double)g + a.wd * wv;
    if (KIND == PCR_OPTIM_ADAM) {
        const double m0 = (double)s0;
        const double m = m0 + a.c1 * (gp - m0);
        const double v = a.b2 * (double)s1 + a.c2 * (gp * gp);
        s0 = (float)m;
        s1 = (float)v;
        w = (float)(wv - a.step * (m / (sqrt(v) / a.sbc2 + a.eps)));
    } else {
        const double b = a.first ? gp : a.mu * (double)s0 + a.cd * gp;
        s0 = (float)b;
        w = (float)(wv - a.step * b);
    }
}

template <int KIND>
__global__ __launch_bounds__(T_BLOCK) void pnopt_update_kernel(const OptArgs a)
{
    const uint64_t tiles = (a.n + OPT_TILE - 1) / OPT_TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // workgroup-uniform; the kernel has no barrier
        const uint64_t t0 = tile * OPT_TILE, t1 = t0 + OPT_TILE;
        uint32_t lo = 0, hi = a.n_ranges;                                    // the first range that ends behind t0 (uniform)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.ranges[mid].end <= t0) lo = mid + 1;
            else hi = mid;
        }
        if (lo == a.n_ranges) return;                                        // nothing but running statistics from here on
        const OptRange r = a.ranges[lo];
        if (r.begin >= t1) continue;                                         // the tile holds running statistics only
        if (r.begin <= t0 && t1 <= r.end) {                                  // the tile lies in one range (so t1 <= n): the array's own 16-byte alignment
            const uint64_t e = t0 + (uint64_t)threadIdx.x * OPT_VEC;
            f32x4 w = *(const f32x4*)(a.w + e);
            const f32x4 g = *(const f32x4*)(a.g + e);
            f32x4 s0 = *(const f32x4*)(a.s0 + e);
            f32x4 s1 = KIND == PCR_OPTIM_ADAM ? *(const f32x4*)(a.s1 + e) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int j = 0; j < OPT_VEC; j++) {
                float wj = w[j], s0j = s0[j], s1j = s1[j];
                opt_element<KIND>(a, wj, g[j], s0j, s1j);
                w[j] = wj; s0[j] = s0j; s1[j] = s1j;
            }
            *(f32x4*)(a.w + e) = w;
            *(f32x4*)(a.s0 + e) = s0;
            if (KIND == PCR_OPTIM_ADAM) *(f32x4*)(a.s1 + e) = s1;
            continue;
        }
#pragma unroll
        for (int j = 0; j < OPT_VEC; j++) {                                  // a border or the array's end: element by element, consecutive lanes on consecutive elements
            const uint64_t e = t0 + (uint64_t)j * T_BLOCK + threadIdx.x;
            if (e >= a.n) continue;
            uint32_t k = lo;
            while (k < a.n_ranges && a.ranges[k].end <= e) k++;
            if (k == a.n_ranges || a.ranges[k].begin > e) continue;          // a running statistic: neither read nor written
            float w = a.w[e], s0 = a.s0[e], s1 = KIND == PCR_OPTIM_ADAM ? a.s1[e] : 0.0f;
            opt_element<KIND>(a, w, a.g[e], s0, s1);
            a.w[e] = w;
            a.s0[e] = s0;
            if (KIND == PCR_OPTIM_ADAM) a.s1[e] = s1;
        }
    }
}

const char* desc_bad(const pcr_optim_desc& d)
{
    if (d.kind != PCR_OPTIM_ADAM && d.kind != PCR_OPTIM_SGD) return ": an unknown kind";
    if (!(d.beta1 >= 0.0 && d.beta1 < 1.0) || !(d.beta2 >= 0.0 && d.beta2 < 1.0)) return ": beta1 and beta2 must lie in [0, 1)";
    if (!(d.eps >= 0.0) || !std::isfinite(d.eps)) return ": eps must be finite and >= 0";
    if (!(d.weight_decay >= 0.0) || !std::isfinite(d.weight_decay)) return ": weight_decay must be finite and >= 0";
    if (!(d.momentum >= 0.0) || !std::isfinite(d.momentum)) return ": momentum must be finite and >= 0";
    if (!std::isfinite(d.dampening)) return ": dampening must be finite";
    return nullptr;
}

inline size_t n_state(const pcr_pn2_trainer* t) { return t->opt.kind == PCR_OPTIM_ADAM ? 2 : 1; }

}  // namespace

const char* pcr::optim_bad(const pcr_pn2_trainer* t, double lr)
{
    if (!t->opt_on) return ": no optimiser is attached (pcr_pn2_trainer_optim_set)";
    if (!std::isfinite(lr)) return ": lr must be finite";
    return nullptr;
}

void pcr::optim_free(pcr_pn2_trainer* t)
{
    if (t->opt_s0) (void)hipFree(t->opt_s0);
    if (t->opt_s1) (void)hipFree(t->opt_s1);
    if (t->opt_ranges) (void)hipFree(t->opt_ranges);
    t->opt_s0 = t->opt_s1 = nullptr;
    t->opt_ranges = nullptr;
    t->opt_n_ranges = 0;
    t->opt_on = false;
    t->opt_step = 0;
    t->opt_p1 = t->opt_p2 = 1.0;
}

int pcr::optim_launch(pcr_ctx* ctx, pcr_pn2_trainer* t, double lr, const char* who)
{
    const pcr_optim_desc& d = t->opt;
    const double p1 = t->opt_p1 * d.beta1, p2 = t->opt_p2 * d.beta2;      // beta^t, t = the count after this update: one more product of the chain
    OptArgs a;
    memset(&a, 0, sizeof(a));
    a.w = t->w_dev; a.g = t->grad_dev; a.s0 = t->opt_s0; a.s1 = t->opt_s1;
    a.ranges = (const OptRange*)t->opt_ranges; a.n_ranges = t->opt_n_ranges; a.n = t->n_weights;
    a.wd = d.weight_decay;
    const uint64_t tiles = (t->n_weights + OPT_TILE - 1) / OPT_TILE;
    const unsigned blocks = (unsigned)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), OPT_MAX_BLOCKS);
    if (d.kind == PCR_OPTIM_ADAM) {
        const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
        a.step = lr / bc1;
        a.c1 = 1.0 - d.beta1; a.b2 = d.beta2; a.c2 = 1.0 - d.beta2;
        a.sbc2 = std::sqrt(bc2); a.eps = d.eps;
        ProfScope ps(ctx, "pnopt_adam");
        hipLaunchKernelGGL(pnopt_update_kernel<PCR_OPTIM_ADAM>, dim3(blocks), dim3(T_BLOCK), 0, ctx->stream, a);
    } else {
        a.step = lr;
        a.first = (t->opt_step == 0 || d.momentum == 0.0) ? 1 : 0;
        a.mu = d.momentum; a.cd = 1.0 - d.dampening;
        ProfScope ps(ctx, "pnopt_sgd");
        hipLaunchKernelGGL(pnopt_update_kernel<PCR_OPTIM_SGD>, dim3(blocks), dim3(T_BLOCK), 0, ctx->stream, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, who, e);
    t->opt_step++;
    t->opt_p1 = p1; t->opt_p2 = p2;
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_optim_set(pcr_ctx* ctx, pcr_pn2_trainer* t, const pcr_optim_desc* desc)
{
    const char* who = "pcr_pn2_trainer_optim_set";
    if (!ctx || !t) return fail(ctx, PCR_ERR_ARG, who);
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set: the trainer lives on another device");
    if (desc)
        if (const char* what = desc_bad(*desc)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str());
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    optim_free(t);
    if (!desc) return PCR_OK;
    t->opt = *desc;
    const std::vector<OptRange> ranges = build_ranges(t);
    const size_t bytes = t->n_weights * 4;
    hipError_t e = hipMalloc((void**)&t->opt_s0, std::max<size_t>(bytes, 4));
    if (e == hipSuccess) e = hipMemset(t->opt_s0, 0, bytes);
    if (e == hipSuccess && desc->kind == PCR_OPTIM_ADAM) {
        e = hipMalloc((void**)&t->opt_s1, std::max<size_t>(bytes, 4));
        if (e == hipSuccess) e = hipMemset(t->opt_s1, 0, bytes);
    }
    if (e == hipSuccess && !ranges.empty()) {
        e = hipMalloc(&t->opt_ranges, ranges.size() * sizeof(OptRange));
        if (e == hipSuccess) e = hipMemcpy(t->opt_ranges, ranges.data(), ranges.size() * sizeof(OptRange), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        optim_free(t);
        return fail(ctx, PCR_ERR_HIP, "pcr_pn2_trainer_optim_set: the optimiser's state", e);
    }
    t->opt_n_ranges = (uint32_t)ranges.size();
    t->opt_on = true;
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_optim_step(pcr_ctx* ctx, pcr_pn2_trainer* t, double lr)
{
    const char* who = "pcr_pn2_trainer_optim_step";
    if (!ctx || !t) return fail(ctx, PCR_ERR_ARG, who);
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_step: the trainer lives on another device");
    if (const char* what = optim_bad(t, lr)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str());
    if (!t->pass_ran) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_step: no pass has run on this trainer (there is no gradient)");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = optim_launch(ctx, t, lr, who);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, who, e);
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_optim_info(const pcr_pn2_trainer* t, pcr_optim_info* info)
{
    if (!t || !info) return PCR_ERR_ARG;
    memset(info, 0, sizeof(*info));
    if (!t->opt_on) return PCR_OK;
    info->desc = t->opt;
    info->step = t->opt_step;
    info->state_bytes = n_state(t) * t->n_weights * 4 + (uint64_t)t->opt_n_ranges * sizeof(OptRange);
    info->attached = 1;
    info->n_ranges = t->opt_n_ranges;
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_optim_get_state(pcr_ctx* ctx, const pcr_pn2_trainer* t, uint64_t* step, float* state0, float* state1, size_t n)
{
    if (!ctx || !t || !step || !state0) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_get_state");
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_get_state: the trainer lives on another device");
    if (!t->opt_on) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_get_state: no optimiser is attached");
    if (n != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_get_state: n is not the model's count");
    if (t->opt.kind == PCR_OPTIM_ADAM && !state1) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_get_state: Adam has two state arrays");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCR_HIP(ctx, hipMemcpy(state0, t->opt_s0, n * 4, hipMemcpyDeviceToHost));
    if (t->opt_s1) PCR_HIP(ctx, hipMemcpy(state1, t->opt_s1, n * 4, hipMemcpyDeviceToHost));
    *step = t->opt_step;
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_optim_set_state(pcr_ctx* ctx, pcr_pn2_trainer* t, uint64_t step, const float* state0, const float* state1, size_t n)
{
    if (!ctx || !t || !state0) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state");
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: the trainer lives on another device");
    if (!t->opt_on) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: no optimiser is attached");
    if (n != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: n is not the model's count");
    const bool adam = t->opt.kind == PCR_OPTIM_ADAM;
    if (adam && !state1) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: Adam has two state arrays");
    for (size_t i = 0; i < n; i++) {
        if (!std::isfinite(state0[i])) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: a non-finite state value");
        if (adam && !(state1[i] >= 0.0f && std::isfinite(state1[i]))) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_optim_set_state: exp_avg_sq must be finite and >= 0");
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCR_HIP(ctx, hipMemcpy(t->opt_s0, state0, n * 4, hipMemcpyHostToDevice));
    if (adam) PCR_HIP(ctx, hipMemcpy(t->opt_s1, state1, n * 4, hipMemcpyHostToDevice));
    t->opt_step = step;
    t->opt_p1 = t->opt_p2 = 1.0;
    for (uint64_t i = 0; i < step; i++) { t->opt_p1 = t->opt_p1 * t->opt.beta1; t->opt_p2 = t->opt_p2 * t->opt.beta2; }      // the chain, from its start
    return PCR_OK;
}

extern "C" int pcr_pn2_trainer_get_grad(pcr_ctx* ctx, const pcr_pn2_trainer* t, float* grad, size_t n)
{
    if (!ctx || !t || !grad) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_grad");
    if (t->device != ctx->device) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_grad: the trainer lives on another device");
    if (n != t->n_weights) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_grad: n is not the model's count");
    if (!t->pass_ran) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_trainer_get_grad: no pass has run on this trainer (there is no gradient)");
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCR_HIP(ctx, hipMemcpy(grad, t->grad_dev, n * 4, hipMemcpyDeviceToHost));
    return PCR_OK;
}
