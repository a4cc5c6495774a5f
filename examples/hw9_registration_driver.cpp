// hw9_registration_driver.cpp — the registration driver of Homework9/hw9/main.cpp (doRegistration :19-122 and the CSV
// row of processDataSet :152-165) reduced to the part that is on the hot path: read a source / target pair, run
// point-to-point ICP with the shipped parameters (main.cpp:88-95) on the MI355X, print
//     idx1,idx2,t_x,t_y,t_z,q_w,q_x,q_y,q_z
// This driver is built without PCL, so the initial pose is the identity.  With PCL's point types at hand the upstream stages plug
// into the drop-in class as GPU bodies:
//     pcr::Registration reg;  reg.setHarris3Dparams(voxel_size * 2, 1e-8, 8, true, false);  reg.setFPFHparams(voxel_size * 4);
//     reg.stages.keypoints = reg.gpuHarris3DStage();      // getHarris3DKeypoints on the GPU (pcr_harris3d_f32)
//     reg.stages.fpfh33 = reg.gpuFPFH33Stage();           // getFPFH33Descriptors on the GPU (pcr_fpfh33_f32)
//     reg.compute(cloud_source, cloud_target, normals_source, normals_target, R, t);
//     reg.stages.normal_space_sampling = reg.gpuNormalSpaceSamplingStage();   // normalSpaceSampling on the GPU (pcr_normal_space_sample_f32)
// and pcr::readBinaryAndVoxelDown(file, cloud, normals, voxel_size) reads and voxels the two files (pcr_voxel_grid_normals_f32).
// With --global this driver runs that whole shipped flow itself through the C ABI, still without PCL (doRegistration, main.cpp:19-99):
// the reader of readBinaryAndVoxelDown (its extra all-zero row included) -> voxel grid with normals at voxel_size -> Harris3D (2 voxel
// sizes, 1e-8) -> FPFH33 (4 voxel sizes) -> union matching (0.5) -> RANSAC (80 000 hypotheses, 4 voxel sizes) -> normal-space sampling of
// the moved source and of the target (10^3 bins, 4 000 points, seed 0) -> point-to-point ICP.  The stages are the library's
// restatements of the PCL algorithms hw9 calls (include/pcr.h says what is not pinned to PCL).
//   usage: hw9_registration_driver <src.bin> <tgt.bin> <floats_per_point: 4 (KITTI x y z i) | 6 (hw9 x y z nx ny nz)>
//                                  [idx_src idx_tgt [max_iter]] [--global [voxel_size [ransac_seed [pose_out.bin]]]]
//   --global needs 6 floats per point; pose_out.bin receives the RANSAC pose and the final pose (2 x 16 f32, row-major 4 x 4).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "registration.hpp"

// file layout: registration.cpp:25-26 (6 floats) or test.hpp:26-28 (4 floats); returns the rows unchanged
static std::vector<float> read_cloud(const std::string& path, int floats_per_point)
{
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) { std::cerr << "Read file " << path << " failed!" << std::endl; std::exit(EXIT_FAILURE); }
    in.seekg(0, std::ios::end);
    const size_t bytes = (size_t)in.tellg();
    in.seekg(0, std::ios::beg);
    std::vector<float> raw(bytes / sizeof(float));
    in.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)(raw.size() * sizeof(float)));
    raw.resize(raw.size() / (size_t)floats_per_point * (size_t)floats_per_point);
    return raw;      // handed to the library as is: PCR_AOS4 / PCR_AOS6 rows
}

// Eigen::Quaternionf(R) (main.cpp:121): the standard trace-based conversion, w >= 0 branch first
static void quaternion_from_R(const float R[9], float q[4])
{
    const float t = R[0] + R[4] + R[8];
    if (t > 0.0f) {
        float s = std::sqrt(t + 1.0f);
        q[0] = 0.5f * s;
        s = 0.5f / s;
        q[1] = (R[7] - R[5]) * s; q[2] = (R[2] - R[6]) * s; q[3] = (R[3] - R[1]) * s;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        float s = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0f);
        float v[3];
        v[i] = 0.5f * s;
        s = 0.5f / s;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * s;
        v[j] = (R[3 * j + i] + R[3 * i + j]) * s;
        v[k] = (R[3 * k + i] + R[3 * i + k]) * s;
        q[1] = v[0]; q[2] = v[1]; q[3] = v[2];
    }
}

// one cloud of the shipped flow: readBinaryAndVoxelDown, then the keypoints and descriptors compute() makes of it
struct Hw9Cloud {
    pcr_cloud* cloud = nullptr;
    pcr_cloud* normals = nullptr;
    std::vector<float> kp;        // keypoints whose descriptor is finite, xyz rows
    std::vector<float> fpfh;      // their FPFH33 rows
};

static int hw9_front(pcr_ctx* ctx, std::vector<float> rows, float voxel_size, Hw9Cloud& out)
{
    rows.insert(rows.end(), 6, 0.0f);                               // the reader's loop appends one all-zero point (registration.cpp:22-28)
    const size_t n = rows.size() / 6;
    std::vector<float> n3(3 * n);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) n3[3 * i + c] = rows[6 * i + 3 + c];
    pcr_cloud *raw = nullptr, *raw_n = nullptr, *ck = nullptr;
    uint64_t m = 0;
    int rc = pcr_cloud_create(ctx, rows.data(), n, PCR_AOS6, &raw);
    if (rc == PCR_OK) rc = pcr_cloud_create(ctx, n3.data(), n, PCR_AOS3, &raw_n);
    if (rc == PCR_OK) rc = pcr_voxel_grid_normals_f32(ctx, raw, raw_n, voxel_size, 1, &out.cloud, &out.normals, nullptr, nullptr, &m);
    pcr_cloud_destroy(ctx, raw);
    pcr_cloud_destroy(ctx, raw_n);
    if (rc != PCR_OK) return rc;
    std::vector<float> xyz(3 * (size_t)m + 3);
    std::vector<uint8_t> key((size_t)m + 1, 0);
    pcr_harris3d_params hp;
    hp.radius = voxel_size * 2; hp.threshold = 1e-8f; hp.method = 0; hp.non_max_suppression = 1;      // main.cpp:75-80
    rc = pcr_cloud_read(ctx, out.cloud, xyz.data(), PCR_AOS3);
    if (rc == PCR_OK) rc = pcr_harris3d_f32(ctx, out.cloud, out.normals, &hp, key.data(), nullptr, nullptr, nullptr);
    if (rc != PCR_OK) return rc;
    std::vector<float> kp;
    for (size_t i = 0; i < (size_t)m; i++)
        if (key[i]) kp.insert(kp.end(), xyz.begin() + 3 * i, xyz.begin() + 3 * i + 3);
    const size_t k = kp.size() / 3;
    std::vector<float> fp(33 * k + 33);
    if (k > 0) {
        rc = pcr_cloud_create(ctx, kp.data(), k, PCR_AOS3, &ck);
        if (rc == PCR_OK) rc = pcr_fpfh33_f32(ctx, out.cloud, out.normals, ck, voxel_size * 4, fp.data(), nullptr, nullptr);      // main.cpp:84
        pcr_cloud_destroy(ctx, ck);
        if (rc != PCR_OK) return rc;
    }
    for (size_t i = 0; i < k; i++) {                                // a keypoint without a descriptor (a NaN row) takes no part in the matching
        bool ok = true;
        for (int b = 0; b < 33; b++) ok = ok && fp[33 * i + b] == fp[33 * i + b];
        if (!ok) continue;
        out.kp.insert(out.kp.end(), kp.begin() + 3 * i, kp.begin() + 3 * i + 3);
        out.fpfh.insert(out.fpfh.end(), fp.begin() + 33 * i, fp.begin() + 33 * i + 33);
    }
    std::cerr << n << " rows -> " << m << " voxels, " << k << " Harris3D keypoints, " << out.kp.size() / 3 << " with a descriptor" << std::endl;
    return PCR_OK;
}

// doRegistration (main.cpp:19-99) through the C ABI; T0 = the RANSAC pose, T = the final pose (row-major 4 x 4)
static int hw9_global(const std::vector<float>& src_rows, const std::vector<float>& tgt_rows, float voxel_size, uint64_t ransac_seed, size_t max_iter,
                      float T0[16], float T[16], pcr_icp_stats* stats)
{
    pcr_ctx* ctx = pcr::default_ctx();
    Hw9Cloud s, t;
    pcr_cloud *moved = nullptr, *ss = nullptr, *st = nullptr;
    int rc = hw9_front(ctx, src_rows, voxel_size, s);
    if (rc == PCR_OK) rc = hw9_front(ctx, tgt_rows, voxel_size, t);
    for (int k = 0; k < 16; k++) T0[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    if (rc == PCR_OK) {
        const size_t ns = s.kp.size() / 3, nt = t.kp.size() / 3;
        std::vector<uint32_t> pairs(2 * (ns + nt) + 2), quads(4 * (size_t)80000 + 4);
        std::vector<float> dist(ns + nt + 1);
        size_t kept = 0;
        rc = pcr_match_union_f32(ctx, s.fpfh.data(), ns, t.fpfh.data(), nt, 33, 0.5f, pairs.data(), dist.data(), &kept);      // main.cpp:86
        if (rc == PCR_OK && kept < 4) { std::cerr << "Correspondences are fewer than 4! Failed!" << std::endl; rc = PCR_ERR_STATE; }
        if (rc == PCR_OK) rc = pcr_ransac_sample_quads(s.kp.data(), ns, pairs.data(), kept, 80000, ransac_seed, quads.data());
        float R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, tr[3] = { 0, 0, 0 };
        uint32_t best = 0;
        int64_t winner = -1;
        if (rc == PCR_OK)
            rc = pcr_ransac_global_f32(ctx, s.kp.data(), ns, t.kp.data(), nt, pairs.data(), kept, quads.data(), 80000, voxel_size * 4, R, tr, &best, &winner, nullptr);
        if (rc == PCR_OK) {
            std::cerr << kept << " correspondences, RANSAC winner " << winner << ", consensus " << best << std::endl;
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) T0[4 * r + c] = R[3 * r + c];
                T0[4 * r + 3] = tr[r];
            }
        }
    }
    if (rc == PCR_OK) {
        // registration.cpp:872-881: the source's normals are rotated by the initial pose before they are binned; the sample is taken from the
        // source as it is, and ICP moves it by T0 itself
        float Tn[16];
        for (int k = 0; k < 16; k++) Tn[k] = T0[k];
        Tn[3] = Tn[7] = Tn[11] = 0.0f;
        const uint32_t bins[3] = { 10, 10, 10 };                    // main.cpp:88-89
        std::vector<uint32_t> idx(4000);
        size_t m = 0;
        rc = pcr_cloud_clone(ctx, s.normals, &moved);
        if (rc == PCR_OK) rc = pcr_transform_f32(ctx, moved, Tn);
        if (rc == PCR_OK) rc = pcr_normal_space_sample_f32(ctx, moved, bins, 4000, 0, idx.data(), &m, s.cloud, &ss, nullptr);
        if (rc == PCR_OK) rc = pcr_normal_space_sample_f32(ctx, t.normals, bins, 4000, 0, idx.data(), &m, t.cloud, &st, nullptr);
    }
    if (rc == PCR_OK) {
        pcr_icp_params prm;
        prm.max_corr = 1.0f; prm.max_iter = max_iter; prm.eps = 1e-8f;     // main.cpp:90-95
        std::cerr << "normal-space samples: " << pcr_cloud_size(ss) << " + " << pcr_cloud_size(st) << " points" << std::endl;
        rc = pcr_icp_p2p_f32(ctx, ss, st, T0, &prm, T, stats);
    }
    if (rc != PCR_OK) std::cerr << pcr_ctx_last_error(ctx) << std::endl;
    for (pcr_cloud* c : { s.cloud, s.normals, t.cloud, t.normals, moved, ss, st }) pcr_cloud_destroy(ctx, c);
    return rc;
}

int main(int argc, char** argv)
{
    int global_at = -1;
    for (int k = 1; k < argc; k++)
        if (std::strcmp(argv[k], "--global") == 0) { global_at = k; break; }
    const int argc_all = argc;
    if (global_at >= 0) argc = global_at;                           // the arguments in front of the flag keep their meaning
    if (argc < 4) {
        std::cerr << "usage: " << argv[0] << " src.bin tgt.bin floats_per_point [idx_src idx_tgt [max_iter]] [--global [voxel_size [ransac_seed [pose_out.bin]]]]"
                  << std::endl;
        return 2;
    }
    const int fpp = std::atoi(argv[3]);
    if (fpp != 4 && fpp != 6) { std::cerr << "floats_per_point must be 4 or 6" << std::endl; return 2; }
    const std::string idx_src = argc > 4 ? argv[4] : "0", idx_tgt = argc > 5 ? argv[5] : "1";
    const size_t max_iter = argc > 6 ? (size_t)std::atol(argv[6]) : 800;
    std::vector<float> src = read_cloud(argv[1], fpp), tgt = read_cloud(argv[2], fpp);

    if (global_at >= 0) {
        if (fpp != 6) { std::cerr << "--global needs 6 floats per point (hw9's x y z nx ny nz rows)" << std::endl; return 2; }
        const float voxel_size = argc_all > global_at + 1 ? (float)std::atof(argv[global_at + 1]) : 0.3f;        // main.cpp:30
        const uint64_t seed = argc_all > global_at + 2 ? std::strtoull(argv[global_at + 2], nullptr, 10) : 5489u;
        float T0[16], T[16];
        pcr_icp_stats stats{};
        const int grc = hw9_global(src, tgt, voxel_size, seed, max_iter, T0, T, &stats);
        if (grc != PCR_OK) { std::cerr << "global registration failed, rc = " << grc << std::endl; return 1; }
        if (argc_all > global_at + 3) {
            std::ofstream po(argv[global_at + 3], std::ios::binary);
            po.write(reinterpret_cast<const char*>(T0), sizeof(T0));
            po.write(reinterpret_cast<const char*>(T), sizeof(T));
        }
        const float Rg[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
        float qg[4];
        quaternion_from_R(Rg, qg);
        std::cerr << "ICP: " << stats.iters_run << " iterations, " << stats.last_pairs << " pairs" << (stats.converged ? ", converged" : ", max_iter reached")
                  << ", " << stats.ms_total << " ms" << std::endl;
        std::printf("idx1,idx2,t_x,t_y,t_z,q_w,q_x,q_y,q_z\n");
        std::printf("%s,%s,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", idx_tgt.c_str(), idx_src.c_str(), T[3], T[7], T[11], qg[0], qg[1], qg[2], qg[3]);
        return 0;
    }

    pcr::IcpPoint2Point reg;
    reg.setICPparams(10, 4000, 1.0f, max_iter, 1e-8f);              // main.cpp:88-95
    float R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 };
    const int rc = reg.run(src.data(), src.size() / (size_t)fpp, tgt.data(), tgt.size() / (size_t)fpp, fpp == 4 ? PCR_AOS4 : PCR_AOS6, R, t);
    if (rc != PCR_OK) { std::cerr << "ICP failed, rc = " << rc << std::endl; return 1; }
    float q[4];
    quaternion_from_R(R, q);
    std::cerr << "ICP: " << reg.last_stats.iters_run << " iterations, " << reg.last_stats.last_pairs << " pairs"
              << (reg.last_stats.converged ? ", converged" : ", max_iter reached") << ", " << reg.last_stats.ms_total << " ms" << std::endl;
    std::printf("idx1,idx2,t_x,t_y,t_z,q_w,q_x,q_y,q_z\n");
    std::printf("%s,%s,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", idx_tgt.c_str(), idx_src.c_str(), t[0], t[1], t[2], q[0], q[1], q[2], q[3]);
    return 0;
}
