// pointnet_layers_check.cpp — host-only driver of csrc/pointnet_layers.hpp (tests/test_pointnet_layers.py compiles and runs it).
// For a list of descriptors built by rule (both kinds at their smallest legal shape, every limit at its last accepted and its first rejected value) it
// prints one JSON object per line: the case's name, the descriptor itself (doubles as %a strings), accept / reject, the weight count, every marker and
// every layer as [K, N, bn].  It includes nothing but the header under test.
#include "pointnet_layers.hpp"

#include <cstdio>
#include <limits>
#include <string>

using namespace pcr;

namespace {

// ---- PointNet++: the smallest legal model, and the ways to leave it ------------------------------------------------------------------------------
pcr_pn2_desc ssg_min()      // n_sa = 1 group_all, n_mlp = 1, n_fc = 1, D0 = 0
{
    pcr_pn2_desc d;
    memset(&d, 0, sizeof(d));
    d.D0 = 0; d.n_sa = 1; d.n_fc = 1; d.bn_eps = 1e-5;
    d.sa[0].group_all = 1; d.sa[0].n_mlp = 1; d.sa[0].widths[0] = 8;
    d.fc_widths[0] = 5;
    return d;
}

pcr_pn2_desc ssg_two(uint32_t D0)      // one sampling layer (npoint 4, nsample 3, radius 0.5, widths 8 16), then group_all (widths 16), head 8 5
{
    pcr_pn2_desc d = ssg_min();
    d.D0 = D0; d.n_sa = 2; d.n_fc = 2;
    d.sa[0].group_all = 0; d.sa[0].npoint = 4; d.sa[0].nsample = 3; d.sa[0].radius = 0.5; d.sa[0].n_mlp = 2; d.sa[0].widths[0] = 8; d.sa[0].widths[1] = 16;
    d.sa[1].group_all = 1; d.sa[1].n_mlp = 1; d.sa[1].widths[0] = 16;
    d.fc_widths[0] = 8; d.fc_widths[1] = 5;
    return d;
}

pcr_pn2_msg_desc msg_of(const pcr_pn2_desc& s)
{
    pcr_pn2_msg_desc d;
    (void)pn2_msg_desc_of(s, d);
    return d;
}

// ssg_two with n_branch branches on the sampling layer: branch b has nsample 3 + b, radius 0.25 (b + 1), n_mlp 1 and the width `width` (the last: `last_width`)
pcr_pn2_msg_desc msg_branches(uint32_t n_branch, uint32_t width, uint32_t last_width, uint32_t xyz_last)
{
    pcr_pn2_msg_desc d = msg_of(ssg_two(3));
    d.sa[0].n_branch = n_branch;
    d.sa[0].xyz_last = xyz_last;
    for (uint32_t b = 0; b < n_branch && b < PCR_PN2_MAX_BRANCH; b++) {
        pcr_pn2_branch_desc& br = d.sa[0].branch[b];
        br.radius = 0.25 * (b + 1); br.nsample = 3 + b; br.n_mlp = 1;
        br.widths[0] = b + 1 == n_branch ? last_width : width;
    }
    return d;
}

void print_u32s(const uint32_t* v, size_t n)
{
    std::printf("[");
    for (size_t i = 0; i < n; i++) std::printf("%s%u", i ? ", " : "", v[i]);
    std::printf("]");
}

void print_shapes(const std::vector<LayerShape>& shapes)
{
    std::printf("[");
    for (size_t i = 0; i < shapes.size(); i++) std::printf("%s[%u, %u, %d]", i ? ", " : "", shapes[i].K, shapes[i].N, shapes[i].bn ? 1 : 0);
    std::printf("]");
}

// ssg: the single-scale descriptor the case was made from (the GPU test gives it to the model AND the trainer), or NULL
void run_pn2(const char* name, const pcr_pn2_msg_desc& d, const pcr_pn2_desc* ssg)
{
    std::printf("{\"name\": \"%s\", \"kind\": \"pn2\", \"ssg\": %d, \"desc\": {\"D0\": %u, \"n_sa\": %u, \"n_fc\": %u, \"bn_eps\": \"%a\", \"fc_widths\": ", name, ssg ? 1 : 0, d.D0,
                d.n_sa, d.n_fc, d.bn_eps);
    print_u32s(d.fc_widths, PCR_PN2_MAX_FC);
    std::printf(", \"sa\": [");
    for (uint32_t l = 0; l < PCR_PN2_MAX_SA; l++) {
        const pcr_pn2_msg_sa_desc& s = d.sa[l];
        std::printf("%s{\"npoint\": %u, \"group_all\": %u, \"xyz_last\": %u, \"n_branch\": %u, \"branch\": [", l ? ", " : "", s.npoint, s.group_all, s.xyz_last, s.n_branch);
        for (uint32_t b = 0; b < PCR_PN2_MAX_BRANCH; b++) {
            std::printf("%s{\"radius\": \"%a\", \"nsample\": %u, \"n_mlp\": %u, \"widths\": ", b ? ", " : "", s.branch[b].radius, s.branch[b].nsample, s.branch[b].n_mlp);
            print_u32s(s.branch[b].widths, PCR_PN2_MAX_MLP);
            std::printf("}");
        }
        std::printf("]}");
    }
    std::printf("]}, ");
    Pn2Layers L;
    const bool ok = pn2_layers(d, L);
    std::printf("\"ok\": %d", ok ? 1 : 0);
    if (ok) {
        std::printf(", \"n_weights\": %llu, \"n_sampling\": %u, \"head_first\": %u, \"sa_in\": ", (unsigned long long)weight_count(L.shapes), L.n_sampling, L.head_first);
        print_u32s(L.sa_in, d.n_sa);
        std::printf(", \"sa_out\": ");
        print_u32s(L.sa_out, d.n_sa);
        std::printf(", \"first\": [");
        for (uint32_t l = 0; l < d.n_sa; l++) {
            std::printf("%s", l ? ", " : "");
            print_u32s(L.first[l], d.sa[l].n_branch);
        }
        std::printf("], \"shapes\": ");
        print_shapes(L.shapes);
    }
    std::printf("}\n");
}

void run_ssg(const char* name, const pcr_pn2_desc& s)
{
    pcr_pn2_msg_desc d;
    if (!pn2_msg_desc_of(s, d)) {            // n_sa outside its range: the conversion itself rejects; the superset descriptor then carries n_sa as it is
        d.n_sa = s.n_sa; d.D0 = s.D0; d.n_fc = s.n_fc; d.bn_eps = s.bn_eps;
        for (uint32_t k = 0; k < PCR_PN2_MAX_FC; k++) d.fc_widths[k] = s.fc_widths[k];
    }
    run_pn2(name, d, &s);
}

// ---- the vanilla PointNet ----------------------------------------------------------------------------------------------------------------------
pcr_pn1_desc pn1_min(uint32_t stn3, uint32_t fstn)      // n_mlp = 2, n_fc = 1
{
    pcr_pn1_desc d;
    memset(&d, 0, sizeof(d));
    d.D0 = 0; d.stn3 = stn3; d.fstn = fstn; d.n_mlp = 2; d.n_fc = 1; d.bn_eps = 1e-5;
    d.widths[0] = 8; d.widths[1] = 16;
    d.tnet_conv[0] = 8; d.tnet_conv[1] = 8; d.tnet_conv[2] = 16;
    d.tnet_fc[0] = 8; d.tnet_fc[1] = 8;
    d.fc_widths[0] = 5;
    return d;
}

void run_pn1(const char* name, const pcr_pn1_desc& d)
{
    std::printf("{\"name\": \"%s\", \"kind\": \"pn1\", \"desc\": {\"D0\": %u, \"stn3\": %u, \"fstn\": %u, \"n_mlp\": %u, \"n_fc\": %u, \"bn_eps\": \"%a\", \"widths\": ", name, d.D0,
                d.stn3, d.fstn, d.n_mlp, d.n_fc, d.bn_eps);
    print_u32s(d.widths, PCR_PN2_MAX_MLP);
    std::printf(", \"tnet_conv\": ");
    print_u32s(d.tnet_conv, 3);
    std::printf(", \"tnet_fc\": ");
    print_u32s(d.tnet_fc, 2);
    std::printf(", \"fc_widths\": ");
    print_u32s(d.fc_widths, PCR_PN2_MAX_FC);
    std::printf("}, ");
    Pn1Layers L;
    const bool ok = pn1_layers(d, L);
    std::printf("\"ok\": %d", ok ? 1 : 0);
    if (ok) {
        std::printf(", \"n_weights\": %llu, \"stn_first\": %u, \"enc_first\": %u, \"fstn_first\": %u, \"head_first\": %u, \"shapes\": ", (unsigned long long)weight_count(L.shapes),
                    L.stn_first, L.enc_first, L.fstn_first, L.head_first);
        print_shapes(L.shapes);
    }
    std::printf("}\n");
}

}  // namespace

int main()
{
    const double inf = std::numeric_limits<double>::infinity();
    // ---- PointNet++, single-scale descriptors (through the conversion)
    run_ssg("ssg_min", ssg_min());
    run_ssg("ssg_two", ssg_two(0));
    run_ssg("ssg_two_D0_3", ssg_two(3));
    for (uint32_t w : { 1024u, 1025u }) {
        pcr_pn2_desc d = ssg_min();
        d.sa[0].widths[0] = w;
        run_ssg(("ssg_mlp_width_" + std::to_string(w)).c_str(), d);
        d = ssg_min();
        d.fc_widths[0] = w;
        run_ssg(("ssg_fc_width_" + std::to_string(w)).c_str(), d);
    }
    {
        pcr_pn2_desc d = ssg_min();
        d.sa[0].widths[0] = 0;
        run_ssg("ssg_mlp_width_0", d);
    }
    for (uint32_t D0 : { 1021u, 1022u }) run_ssg(("ssg_D0_" + std::to_string(D0)).c_str(), ssg_two(D0));
    for (uint32_t ns : { 65536u, 65537u, 0u }) {
        pcr_pn2_desc d = ssg_two(0);
        d.sa[0].nsample = ns;
        run_ssg(("ssg_nsample_" + std::to_string(ns)).c_str(), d);
    }
    {
        pcr_pn2_desc d = ssg_two(0);
        d.sa[0].npoint = 0;
        run_ssg("ssg_npoint_0", d);
        d = ssg_two(0);
        d.sa[0].group_all = 1;               // group_all on a layer that is not the last
        run_ssg("ssg_group_all_not_last", d);
        d = ssg_two(0);
        d.sa[1].group_all = 2;
        run_ssg("ssg_group_all_2", d);
        d = ssg_two(0);
        d.sa[0].radius = -1.0;
        run_ssg("ssg_radius_negative", d);
        d.sa[0].radius = inf;
        run_ssg("ssg_radius_inf", d);
        d.sa[0].radius = std::numeric_limits<double>::quiet_NaN();
        run_ssg("ssg_radius_nan", d);
        d.sa[0].radius = 0.0;
        run_ssg("ssg_radius_0", d);
        d = ssg_two(0);
        d.bn_eps = inf;
        run_ssg("ssg_bn_eps_inf", d);
    }
    for (uint32_t n : { 0u, 5u }) {
        pcr_pn2_desc d = ssg_min();
        d.n_sa = n;
        run_ssg(("ssg_n_sa_" + std::to_string(n)).c_str(), d);
        d = ssg_min();
        d.n_fc = n;
        run_ssg(("ssg_n_fc_" + std::to_string(n)).c_str(), d);
        d = ssg_min();
        d.sa[0].n_mlp = n;
        run_ssg(("ssg_n_mlp_" + std::to_string(n)).c_str(), d);
    }
    {
        pcr_pn2_desc d = ssg_two(0);         // every count at its largest: 4 SA layers of 4 widths, 4 FC layers
        d.n_sa = 4; d.n_fc = 4;
        for (uint32_t l = 0; l < 4; l++) {
            d.sa[l] = ssg_two(0).sa[l < 3 ? 0 : 1];
            d.sa[l].n_mlp = 4;
            for (uint32_t k = 0; k < 4; k++) d.sa[l].widths[k] = 8 + 4 * l + k;
        }
        for (uint32_t k = 0; k < 4; k++) d.fc_widths[k] = 9 - k;
        run_ssg("ssg_full", d);
    }
    // ---- PointNet++, multi-scale descriptors
    run_pn2("msg_two_branches", msg_branches(2, 8, 12, 1), nullptr);
    run_pn2("msg_n_branch_4", msg_branches(4, 8, 8, 1), nullptr);
    run_pn2("msg_n_branch_5", msg_branches(5, 8, 8, 1), nullptr);
    run_pn2("msg_n_branch_0", msg_branches(0, 8, 8, 1), nullptr);
    for (uint32_t last : { 256u, 257u }) {   // a layer as wide as 1024 can only be the last one: the next would take 3 + 1024 channels
        pcr_pn2_msg_desc d = msg_branches(4, 256, last, 0);
        d.n_sa = 1;
        run_pn2(("msg_branch_sum_" + std::to_string(768 + last)).c_str(), d, nullptr);
        d.n_sa = 2;
        d.sa[0].branch[3].widths[0] = last - 3;      // 1021 / 1022 in front of a group_all layer
        run_pn2(("msg_branch_sum_" + std::to_string(765 + last) + "_not_last").c_str(), d, nullptr);
    }
    {
        pcr_pn2_msg_desc d = msg_branches(2, 8, 8, 0);
        d.sa[0].xyz_last = 2;
        run_pn2("msg_xyz_last_2", d, nullptr);
        d = msg_branches(2, 8, 8, 0);
        d.sa[0].branch[1].nsample = 65537;
        run_pn2("msg_second_branch_nsample_65537", d, nullptr);
        d = msg_of(ssg_two(3));
        d.sa[1].n_branch = 2;                // group_all takes one branch
        d.sa[1].branch[1] = d.sa[1].branch[0];
        run_pn2("msg_group_all_two_branches", d, nullptr);
    }
    // ---- the vanilla PointNet
    run_pn1("pn1_min_plain", pn1_min(0, 0));
    run_pn1("pn1_min_stn3", pn1_min(1, 0));
    run_pn1("pn1_min_fstn", pn1_min(0, 1));
    run_pn1("pn1_min_both", pn1_min(1, 1));
    {
        pcr_pn1_desc d = pn1_min(1, 1);
        d.D0 = 3; d.n_mlp = 4; d.n_fc = 4;
        d.widths[0] = 12; d.widths[1] = 16; d.widths[2] = 20; d.widths[3] = 24;
        d.fc_widths[0] = 16; d.fc_widths[1] = 12; d.fc_widths[2] = 8; d.fc_widths[3] = 5;
        run_pn1("pn1_full", d);
    }
    for (uint32_t w : { 1024u, 1025u }) {
        pcr_pn1_desc d = pn1_min(0, 0);
        d.widths[1] = w;
        run_pn1(("pn1_width_" + std::to_string(w)).c_str(), d);
        d = pn1_min(0, 0);
        d.fc_widths[0] = w;
        run_pn1(("pn1_fc_width_" + std::to_string(w)).c_str(), d);
        d = pn1_min(1, 0);
        d.tnet_conv[2] = w;
        run_pn1(("pn1_tnet_conv_" + std::to_string(w)).c_str(), d);
        d = pn1_min(0, 1);
        d.tnet_fc[0] = w;
        run_pn1(("pn1_tnet_fc_" + std::to_string(w)).c_str(), d);
    }
    {
        pcr_pn1_desc d = pn1_min(0, 0);      // without a T-Net its widths are not read
        d.tnet_conv[0] = 1025; d.tnet_fc[1] = 0;
        run_pn1("pn1_plain_ignores_tnet_widths", d);
    }
    for (uint32_t D0 : { 1021u, 1022u }) {
        pcr_pn1_desc d = pn1_min(1, 1);
        d.D0 = D0;
        run_pn1(("pn1_D0_" + std::to_string(D0)).c_str(), d);
    }
    for (uint32_t k : { 128u, 129u }) {
        pcr_pn1_desc d = pn1_min(1, 1);      // a feature transform of k x k: the T-Net's last layer has k k outputs
        d.widths[0] = k;
        run_pn1(("pn1_fstn_k_" + std::to_string(k)).c_str(), d);
    }
    {
        pcr_pn1_desc d = pn1_min(1, 0);
        d.widths[0] = 129;
        run_pn1("pn1_stn3_only_k_129", d);
        d = pn1_min(1, 1);
        d.stn3 = 2;
        run_pn1("pn1_stn3_2", d);
        d = pn1_min(1, 1);
        d.fstn = 2;
        run_pn1("pn1_fstn_2", d);
        d = pn1_min(1, 1);
        d.bn_eps = -inf;
        run_pn1("pn1_bn_eps_inf", d);
    }
    for (uint32_t n : { 1u, 5u }) {
        pcr_pn1_desc d = pn1_min(0, 0);
        d.n_mlp = n;
        run_pn1(("pn1_n_mlp_" + std::to_string(n)).c_str(), d);
    }
    for (uint32_t n : { 0u, 5u }) {
        pcr_pn1_desc d = pn1_min(0, 0);
        d.n_fc = n;
        run_pn1(("pn1_n_fc_" + std::to_string(n)).c_str(), d);
    }
    return 0;
}
