// pointnet_layers.hpp — the layers of a classifier's descriptor in weight order, stated once (host only; includes nothing from HIP).
// The eval models (pointnet2.hip) and the training passes (pointnet2_train.hip, pointnet_train.hip) all take their layers, their limits and their
// weight count from here, so a model and a trainer made from one descriptor agree on every layer: a checkpoint trained here loads here.
//   pn2_layers(msg_desc, L) / pn1_layers(pn1_desc, L): false for a descriptor outside the limits written out above pcr_pn2_model_create,
//   pcr_pn2_msg_model_create and pcr_pn1_model_create in include/pcr.h; an SSG descriptor goes through pn2_msg_desc_of first
#pragma once

#include "pcr.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace pcr {

constexpr uint32_t PN_MAX_WIDTH = 1024;                    // the widest layer, and the most input channels (3 + D)
constexpr uint32_t PN_MAX_TRANSFORM = 128;                 // the largest K x K feature transform: the matrix is staged in LDS
constexpr unsigned long long PN_MAX_ROWS = 0x7FFFFFF0ull;  // rows (and cells) of a stage: 2^31 - 16
constexpr uint32_t PN_MAX_NSAMPLE = 65536;

struct LayerShape { uint32_t K, N; bool bn; };

// a layer's floats in the flat weight array: W [N][K], bias [N] and, with BN, gamma, beta, running_mean, running_var
inline uint64_t weight_count(const LayerShape& s) { return (uint64_t)s.K * s.N + s.N + (s.bn ? 4ull * s.N : 0ull); }
inline uint64_t weight_count(const std::vector<LayerShape>& shapes)
{
    uint64_t n = 0;
    for (const LayerShape& s : shapes) n += weight_count(s);
    return n;
}

inline bool width_ok(uint32_t w) { return w >= 1 && w <= PN_MAX_WIDTH; }

// ---- PointNet++ -------------------------------------------------------------------------------------------------------------------------------
struct Pn2Layers {
    std::vector<LayerShape> shapes;                         // SA layer by SA layer, branch by branch, convolution by convolution, then the FC layers
    uint32_t first[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH] = {};   // the first layer of every (SA layer, branch)
    uint32_t sa_in[PCR_PN2_MAX_SA] = {};                    // input channels of every SA layer (3 + D)
    uint32_t sa_out[PCR_PN2_MAX_SA] = {};                   // its width: the sum of its branches' last widths
    uint32_t head_first = 0;                                // the first FC layer
    uint32_t n_sampling = 0;                                // SA layers that are not group_all
};

// the same model in the superset descriptor: one xyz-first branch per layer.  false: n_sa outside 1 ... PCR_PN2_MAX_SA
inline bool pn2_msg_desc_of(const pcr_pn2_desc& s, pcr_pn2_msg_desc& d)
{
    memset(&d, 0, sizeof(d));
    if (s.n_sa < 1 || s.n_sa > PCR_PN2_MAX_SA) return false;
    d.D0 = s.D0; d.n_sa = s.n_sa; d.n_fc = s.n_fc; d.bn_eps = s.bn_eps;
    for (uint32_t k = 0; k < PCR_PN2_MAX_FC; k++) d.fc_widths[k] = s.fc_widths[k];
    for (uint32_t l = 0; l < s.n_sa; l++) {
        const pcr_pn2_sa_desc& a = s.sa[l];
        d.sa[l].npoint = a.npoint; d.sa[l].group_all = a.group_all; d.sa[l].xyz_last = 0; d.sa[l].n_branch = 1;
        d.sa[l].branch[0].radius = a.radius; d.sa[l].branch[0].nsample = a.nsample; d.sa[l].branch[0].n_mlp = a.n_mlp;
        for (uint32_t k = 0; k < PCR_PN2_MAX_MLP; k++) d.sa[l].branch[0].widths[k] = a.widths[k];
    }
    return true;
}

// the validated layers of a descriptor; false for a descriptor outside the limits (L is then half filled)
inline bool pn2_layers(const pcr_pn2_msg_desc& d, Pn2Layers& L)
{
    L = Pn2Layers();
    if (d.n_sa < 1 || d.n_sa > PCR_PN2_MAX_SA || d.n_fc < 1 || d.n_fc > PCR_PN2_MAX_FC) return false;
    if (d.D0 > PN_MAX_WIDTH - 3 || !std::isfinite(d.bn_eps)) return false;
    uint32_t D = d.D0;
    for (uint32_t l = 0; l < d.n_sa; l++) {
        const pcr_pn2_msg_sa_desc& s = d.sa[l];
        if (s.n_branch < 1 || s.n_branch > PCR_PN2_MAX_BRANCH || s.group_all > 1 || s.xyz_last > 1) return false;
        if (s.group_all && (l + 1 != d.n_sa || s.n_branch != 1)) return false;
        if (!s.group_all && s.npoint < 1) return false;
        const uint32_t K0 = 3 + D;
        if (K0 > PN_MAX_WIDTH) return false;
        L.sa_in[l] = K0;
        uint32_t width = 0;
        for (uint32_t b = 0; b < s.n_branch; b++) {
            const pcr_pn2_branch_desc& br = s.branch[b];
            if (br.n_mlp < 1 || br.n_mlp > PCR_PN2_MAX_MLP) return false;
            if (!s.group_all && (br.nsample < 1 || br.nsample > PN_MAX_NSAMPLE || !(br.radius >= 0.0) || std::isinf(br.radius))) return false;
            L.first[l][b] = (uint32_t)L.shapes.size();
            uint32_t K = K0;
            for (uint32_t i = 0; i < br.n_mlp; i++) {
                if (!width_ok(br.widths[i])) return false;
                L.shapes.push_back({ K, br.widths[i], true });
                K = br.widths[i];
            }
            width += K;
        }
        if (width > PN_MAX_WIDTH) return false;
        L.sa_out[l] = width;
        D = width;
        if (!s.group_all) L.n_sampling++;
    }
    L.head_first = (uint32_t)L.shapes.size();
    uint32_t K = D;
    for (uint32_t i = 0; i < d.n_fc; i++) {
        if (!width_ok(d.fc_widths[i])) return false;
        L.shapes.push_back({ K, d.fc_widths[i], i + 1 < d.n_fc });
        K = d.fc_widths[i];
    }
    return true;
}

// ---- the vanilla PointNet ---------------------------------------------------------------------------------------------------------------------
struct Pn1Layers {
    std::vector<LayerShape> shapes;      // [stn3's six layers] [the encoder's convolutions] [fstn's six layers] [the head's FC layers]
    uint32_t stn_first = 0, enc_first = 0, fstn_first = 0, head_first = 0;      // a T-Net the flags leave out has no layers: its part is empty
};

inline bool pn1_layers(const pcr_pn1_desc& d, Pn1Layers& L)
{
    L = Pn1Layers();
    if (d.D0 > PN_MAX_WIDTH - 3 || d.stn3 > 1 || d.fstn > 1 || d.n_mlp < 2 || d.n_mlp > PCR_PN2_MAX_MLP || d.n_fc < 1 || d.n_fc > PCR_PN2_MAX_FC) return false;
    if (!std::isfinite(d.bn_eps)) return false;
    for (uint32_t i = 0; i < d.n_mlp; i++)
        if (!width_ok(d.widths[i])) return false;
    for (uint32_t i = 0; i < d.n_fc; i++)
        if (!width_ok(d.fc_widths[i])) return false;
    if (d.stn3 || d.fstn) {
        for (uint32_t w : d.tnet_conv) if (!width_ok(w)) return false;
        for (uint32_t w : d.tnet_fc) if (!width_ok(w)) return false;
    }
    if (d.fstn && d.widths[0] > PN_MAX_TRANSFORM) return false;
    auto tnet = [&](uint32_t K, uint32_t k) {      // the last layer has k k outputs (up to 16 384): PN_MAX_WIDTH does not apply to it
        for (uint32_t w : d.tnet_conv) { L.shapes.push_back({ K, w, true }); K = w; }
        for (uint32_t w : d.tnet_fc) { L.shapes.push_back({ K, w, true }); K = w; }
        L.shapes.push_back({ K, k * k, false });
    };
    const uint32_t C0 = 3 + d.D0;
    if (d.stn3) tnet(C0, 3);
    L.enc_first = (uint32_t)L.shapes.size();
    uint32_t K = C0;
    for (uint32_t i = 0; i < d.n_mlp; i++) { L.shapes.push_back({ K, d.widths[i], true }); K = d.widths[i]; }
    L.fstn_first = (uint32_t)L.shapes.size();
    if (d.fstn) tnet(d.widths[0], d.widths[0]);
    L.head_first = (uint32_t)L.shapes.size();
    for (uint32_t i = 0; i < d.n_fc; i++) { L.shapes.push_back({ K, d.fc_widths[i], i + 1 < d.n_fc }); K = d.fc_widths[i]; }
    return true;
}

}  // namespace pcr
