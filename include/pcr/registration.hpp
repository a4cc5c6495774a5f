// registration.hpp — the ICP end of Homework9/hw9 (include/registration.hpp, src/registration.cpp) on the MI355X.
//
// Two layers:
//  (0) pcr::GlobalRegistration — descriptor matching + feature RANSAC (the initial pose ICP starts from), arrays only
//  (1) pcr::IcpPoint2Point — dependency-free core with the reference's parameter set
//      (Registration::setICPparams, registration.hpp:126-137) and the semantics of
//      Registration::ICPpoint2point (registration.hpp:204-211, registration.cpp:862-1011): R and t are
//      IN/OUT (pre-loaded with the initial guess, registration.cpp:1141-1142 / :874), clouds are the
//      already-sampled clouds (normal-space sampling, :880-881, is upstream of the hot path).
//  (2) When PCL and Eigen are available (__has_include): `class pcr::Registration` with the reference's member signatures —
//        setICPparams(int, size_t, float, size_t, float)                                            registration.hpp:126-137
//        compute(const PointCloud&, const PointCloud&, const NormalCloud&, const NormalCloud&, Matrix3f& R, Vector3f& t)   :139-144
//        ICPpoint2point(const Matrix3f& init_R, const Vector3f& init_t, const PointCloud&, const PointCloud&,
//                       const NormalCloud&, const NormalCloud&, Matrix3f& R, Vector3f& t)           :204-211 (and ICPpoint2plane, RANSAC,
//        findRANSACCorrespondencesUnion / Inter) — plus the free transformCloudInplace / transformNormalsInplace (:58-64).
//      
#ifndef PCR_DROPIN_REGISTRATION_HPP
#define PCR_DROPIN_REGISTRATION_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pcr_host.hpp"

namespace pcr {

class IcpPoint2Point
{
    // defaults = the shipped parameters, Homework9/hw9/main.cpp:88-95
    int m_ICP_normal_bins = 10;
    size_t m_ICP_sampled_size = 4000;
    float m_ICP_max_corres_dist = 1.0f;
    size_t m_ICP_max_iter = 800;
    float m_ICP_loss_epsilon = 1e-8f;

public:
    pcr_icp_stats last_stats{};

    // same argument order and meaning as Registration::setICPparams
    void setICPparams(int normal_bins, size_t sampled_size, float max_corres_dist, size_t max_iter, float loss_epsilon)
    {
        m_ICP_normal_bins = normal_bins;
        m_ICP_sampled_size = sampled_size;
        m_ICP_max_corres_dist = max_corres_dist;
        m_ICP_max_iter = max_iter;
        m_ICP_loss_epsilon = loss_epsilon;
    }

    // src/tgt: host points in `layout` (PCR_AOS4 == pcl::PointXYZ array, PCR_SOA == column-major N x 3 matrix).
    // R (row-major 3x3) and t: in = initial guess, out = final pose.  Returns the C-ABI status.
    int run(const float* src_xyz, size_t n_src, const float* tgt_xyz, size_t n_tgt, int layout, float R[9], float t[3])
    {
        pcr_ctx* ctx = default_ctx();
        pcr_cloud *cs = nullptr, *ct = nullptr;
        int rc = pcr_cloud_create(ctx, src_xyz, n_src, layout, &cs);
        if (rc == PCR_OK) rc = pcr_cloud_create(ctx, tgt_xyz, n_tgt, layout, &ct);
        if (rc == PCR_OK) {
            const float init_T[16] = { R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1 };
            float out_T[16];
            pcr_icp_params prm;
            prm.max_corr = m_ICP_max_corres_dist;
            prm.max_iter = m_ICP_max_iter;
            prm.eps = m_ICP_loss_epsilon;
            rc = pcr_icp_p2p_f32(ctx, cs, ct, init_T, &prm, out_T, &last_stats);
            if (rc == PCR_OK) {
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) R[3 * r + c] = out_T[4 * r + c];
                    t[r] = out_T[4 * r + 3];
                }
            }
        }
        pcr_cloud_destroy(ctx, cs);
        pcr_cloud_destroy(ctx, ct);
        return rc;
    }
};

// The global-registration front half (next row N4): Registration::setRANSACparams (registration.hpp:115-124),
// findRANSACCorrespondencesUnion (:191-193, registration.cpp:535-615) and RANSAC (:179-185, registration.cpp:288-434)
// with plain arrays in place of pcl::PointCloud<FPFHSignature33> / PointCloud.
class GlobalRegistration
{
    // defaults = reg.setRANSACparams(80000, voxel_size * 4, 10, 0.5) with voxel_size 0.3 (Homework9/hw9/main.cpp:30,86)
    uint32_t m_RANSAC_max_iter = 80000;
    float m_RANSAC_dist_threshold = 1.2f;
    float m_RANSAC_angle_threshold = 10.0f;      // unused by the reference too (:419, commented out)
    float m_RANSAC_corres_rejection_rate = 0.5f;

public:
    uint64_t seed = 5489u;                        // the reference seeds std::mt19937 from std::random_device (:298-299)
    uint32_t max_consensus_set_size = 0;          // what the reference prints with DEBUG (:433)

    void setRANSACparams(const uint32_t max_iter, const float dist_threshold, const float angle_threshold, const float corres_rejection_rate)
    {
        m_RANSAC_max_iter = max_iter;
        m_RANSAC_dist_threshold = dist_threshold;
        m_RANSAC_angle_threshold = angle_threshold;
        m_RANSAC_corres_rejection_rate = corres_rejection_rate;
    }

    // descriptors: row-major n x dim (pcl::FPFHSignature33::histogram rows, dim 33).  correspondences[i] = {idx_src, idx_tar}
    void findRANSACCorrespondencesUnion(const float* fpfh_source, size_t N_source, const float* fpfh_target, size_t N_target, int dim,
                                        std::vector<std::vector<size_t>>& correspondences)
    {
        std::vector<uint32_t> pairs(2 * (N_source + N_target) + 2);
        std::vector<float> dist(N_source + N_target + 1);
        size_t kept = 0;
        check(pcr_match_union_f32(default_ctx(), fpfh_source, N_source, fpfh_target, N_target, dim, m_RANSAC_corres_rejection_rate, pairs.data(),
                                  dist.data(), &kept),
              "pcr_match_union_f32");
        correspondences.resize(kept);
        for (size_t i = 0; i < kept; i++) correspondences[i] = std::vector<size_t>{ pairs[2 * i], pairs[2 * i + 1] };
    }

    // the mutual-nearest-neighbour variant (registration.hpp:187-189, registration.cpp:437-533)
    void findRANSACCorrespondencesInter(const float* fpfh_source, size_t N_source, const float* fpfh_target, size_t N_target, int dim,
                                        std::vector<std::vector<size_t>>& correspondences)
    {
        std::vector<uint32_t> pairs(2 * N_source + 2);
        std::vector<float> dist(N_source + 1);
        size_t kept = 0;
        check(pcr_match_inter_f32(default_ctx(), fpfh_source, N_source, fpfh_target, N_target, dim, m_RANSAC_corres_rejection_rate, pairs.data(),
                                  dist.data(), &kept),
              "pcr_match_inter_f32");
        correspondences.resize(kept);
        for (size_t i = 0; i < kept; i++) correspondences[i] = std::vector<size_t>{ pairs[2 * i], pairs[2 * i + 1] };
    }

    // keypoints: AoS xyz (n x 3).  R (row-major) and t are written only when a non-empty consensus set exists, as in the
    // reference (:423-428).  Returns the C-ABI status.
    int RANSAC(const std::vector<std::vector<size_t>>& correspondences, const float* kp_source_xyz, size_t n_source, const float* kp_target_xyz,
               size_t n_target, float R[9], float t[3])
    {
        const size_t M = correspondences.size();
        std::vector<uint32_t> pairs(2 * M + 2);
        for (size_t i = 0; i < M; i++) {
            pairs[2 * i] = (uint32_t)correspondences[i][0];
            pairs[2 * i + 1] = (uint32_t)correspondences[i][1];
        }
        std::vector<uint32_t> quads(4 * (size_t)m_RANSAC_max_iter + 4);
        int rc = pcr_ransac_sample_quads(kp_source_xyz, n_source, pairs.data(), M, m_RANSAC_max_iter, seed, quads.data());
        if (rc != PCR_OK) return rc;
        int64_t winner = -1;
        return pcr_ransac_global_f32(default_ctx(), kp_source_xyz, n_source, kp_target_xyz, n_target, pairs.data(), M, quads.data(), m_RANSAC_max_iter,
                                     m_RANSAC_dist_threshold, R, t, &max_consensus_set_size, &winner, nullptr);
    }
};

}  // namespace pcr

#if defined(__has_include)
#if __has_include(<pcl/point_cloud.h>) && __has_include(<pcl/point_types.h>) && __has_include(<Eigen/Core>)
#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#if __has_include(<pcl/impl/point_types.hpp>)
#include <pcl/impl/point_types.hpp>                             // pcl::PointNormal's definition (PCL's point_types.h includes it itself)
#endif

#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <string>

// ---- (2) the reference's own types and signatures (Homework9/hw9/include/registration.hpp) --------------------------------
// Everything below compiles only where PCL + Eigen exist (the reference's build environment).  In this repository it is
// compile- and run-checked against minimal test-only stand-ins for the three headers (tests/mock/, tests/test_registration_class.py):
// a compile check of the SIGNATURES, never a pin of Eigen/PCL numerics.
namespace pcr {

using PointT = pcl::PointXYZ;                                   // registration.hpp:42-44
using PointCloud = pcl::PointCloud<PointT>;
using NormalT = pcl::Normal;                                    // registration.hpp:46-48
using NormalCloud = pcl::PointCloud<pcl::Normal>;
static_assert(sizeof(pcl::PointXYZ) == 4 * sizeof(float), "pcl::PointXYZ is expected to be a 16-byte xyz+pad record");

// registration.hpp:58-60 / registration.cpp:165-178 on the GPU (bit-identical f32 arithmetic)
inline void transformCloudInplace(PointCloud& cloud, const Eigen::Matrix3f& R, const Eigen::Vector3f& t)
{
    if (cloud.size() == 0) return;
    pcr_ctx* ctx = default_ctx();
    pcr_cloud* c = nullptr;
    check(pcr_cloud_create(ctx, reinterpret_cast<const float*>(cloud.points.data()), cloud.size(), PCR_AOS4, &c), "pcr_cloud_create");
    const float T[16] = { R(0, 0), R(0, 1), R(0, 2), t(0), R(1, 0), R(1, 1), R(1, 2), t(1), R(2, 0), R(2, 1), R(2, 2), t(2), 0, 0, 0, 1 };
    int rc = pcr_transform_f32(ctx, c, T);
    if (rc == PCR_OK) {
        // PCR_AOS4 read-back writes x, y, z and leaves the 4th float of every record untouched
        rc = pcr_cloud_read(ctx, c, reinterpret_cast<float*>(cloud.points.data()), PCR_AOS4);
    }
    pcr_cloud_destroy(ctx, c);
    check(rc, "pcr_transform_f32");
}

// registration.hpp:62-64 / registration.cpp:181-194: normal <- R * normal (t unused there too).  Only the sampling stage
// upstream of the hot path reads the result, so this stays a host loop with the reference's row-wise f32 arithmetic.
inline void transformNormalsInplace(NormalCloud& cloud, const Eigen::Matrix3f& R, const Eigen::Vector3f& /*t*/)
{
    for (size_t i = 0; i < cloud.size(); i++) {
        const float x = cloud.points[i].normal_x, y = cloud.points[i].normal_y, z = cloud.points[i].normal_z;
        cloud.points[i].normal_x = (R(0, 0) * x + R(0, 1) * y) + R(0, 2) * z;
        cloud.points[i].normal_y = (R(1, 0) * x + R(1, 1) * y) + R(1, 2) * z;
        cloud.points[i].normal_z = (R(2, 0) * x + R(2, 1) * y) + R(2, 2) * z;
    }
}

// The voxel grid of hw9 (pcl::VoxelGrid<pcl::PointNormal> with setDownsampleAllData(true): pcr_voxel_grid_normals_f32, normal_mode 1,
// include/pcr.h — the library's restatement, not PCL bit for bit) over a cloud and its normals: the filter of readBinaryAndVoxelDown
// (registration.cpp:37-41) and the whole of VoxelGridSampling (:665-707).  Rows come out in ascending voxel id.
inline void voxelGridWithNormals(const PointCloud& input_cloud, const NormalCloud& input_normals, float leaf, PointCloud& out_cloud, NormalCloud& out_normals)
{
    const size_t n = input_cloud.size();
    std::vector<float> n3(3 * input_normals.size() + 3);
    for (size_t i = 0; i < input_normals.size(); i++) {
        n3[3 * i] = input_normals.points[i].normal_x; n3[3 * i + 1] = input_normals.points[i].normal_y; n3[3 * i + 2] = input_normals.points[i].normal_z;
    }
    pcr_ctx* ctx = default_ctx();
    pcr_cloud *cs = nullptr, *cn = nullptr, *oc = nullptr, *on = nullptr;
    uint64_t m = 0;
    std::vector<PointT> pts;
    std::vector<float> nr;
    int rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(input_cloud.points.data()), n, PCR_AOS4, &cs);
    if (rc == PCR_OK) rc = pcr_cloud_create(ctx, n3.data(), input_normals.size(), PCR_AOS3, &cn);
    if (rc == PCR_OK) rc = pcr_voxel_grid_normals_f32(ctx, cs, cn, leaf, 1, &oc, &on, nullptr, nullptr, &m);
    if (rc == PCR_OK) {
        pts.resize((size_t)m);                                      // default-constructed: data[3] = 1, as PCL's points have
        nr.resize(3 * (size_t)m + 3);
        rc = pcr_cloud_read(ctx, oc, reinterpret_cast<float*>(pts.data()), PCR_AOS4);
        if (rc == PCR_OK) rc = pcr_cloud_read(ctx, on, nr.data(), PCR_AOS3);
    }
    pcr_cloud_destroy(ctx, cs);
    pcr_cloud_destroy(ctx, cn);
    pcr_cloud_destroy(ctx, oc);
    pcr_cloud_destroy(ctx, on);
    check(rc, "pcr_voxel_grid_normals_f32");
    out_cloud.points = pts;
    out_normals.points.assign((size_t)m, NormalT());
    for (size_t i = 0; i < (size_t)m; i++) {
        out_normals.points[i].normal_x = nr[3 * i]; out_normals.points[i].normal_y = nr[3 * i + 1]; out_normals.points[i].normal_z = nr[3 * i + 2];
    }
    out_cloud.height = 1;                                           // :61-66, :690-696
    out_cloud.width = (uint32_t)out_cloud.points.size();
    out_cloud.is_dense = true;
    out_normals.height = 1;
    out_normals.width = (uint32_t)out_normals.points.size();
    out_normals.is_dense = true;
}

// readBinaryAndVoxelDown, registration.hpp:50-53 / registration.cpp:8-68, with the reference's signature: the reader loop as written
// there and the voxel grid on the GPU.  The `good() && !eof()` loop tests the stream BEFORE each read, so the read that hits the end of
// the file still appends its point: one extra default-constructed pcl::PointNormal (all zeros) follows the last row, and it takes part
// in the voxel grid like any other point (a voxel at the origin with a zero normal) — the same kind of quirk as readBinary's extra
// point in Homework2, kept because it is what hw9 computes.
inline void readBinaryAndVoxelDown(const std::string& fileName, PointCloud& cloud, NormalCloud& normals, float voxel_size)
{
    std::fstream input(fileName.c_str(), std::ios::in | std::ios::binary);
    input.seekg(0, std::ios::beg);
    if (!input.good()) {
        std::cerr << "Read file " << fileName << " failed!";
        std::exit(EXIT_FAILURE);
    }
    PointCloud raw_cloud;
    NormalCloud raw_normals;
    for (int i = 0; input.good() && !input.eof(); i++) {
        pcl::PointNormal point_normal_tmp;
        input.read((char*)&point_normal_tmp.x, 3 * sizeof(float));
        input.read((char*)&point_normal_tmp.normal_x, 3 * sizeof(float));
        PointT p;
        p.x = point_normal_tmp.x; p.y = point_normal_tmp.y; p.z = point_normal_tmp.z;
        NormalT nn;
        nn.normal_x = point_normal_tmp.normal_x; nn.normal_y = point_normal_tmp.normal_y; nn.normal_z = point_normal_tmp.normal_z;
        raw_cloud.points.push_back(p);
        raw_normals.points.push_back(nn);
    }
    input.close();
    voxelGridWithNormals(raw_cloud, raw_normals, voxel_size, cloud, normals);
}

// class Registration, registration.hpp:67-251 — same public interface (the seven setters and compute) and the same private
// members for the stages this library accelerates (RANSAC, findRANSACCorrespondencesUnion / Inter, ICPpoint2point,
// ICPpoint2plane), each with the reference's exact signature.  The remaining private stages of the reference are PCL
// library calls (Harris3D / ISS keypoints, FPFH / SHOT descriptors, NormalSpaceSampling, VoxelGrid); they are
// pluggable `stages` so that a maintainer passes the reference's own bodies or the GPU ones below: with
// gpuHarris3DStage(), gpuFPFH33Stage() and gpuNormalSpaceSamplingStage() set, and readBinaryAndVoxelDown above in front, the whole
// shipped flow runs without a PCL algorithm.
class Registration
{
public:
    Registration() {}
    ~Registration() = default;

    void setISSparams(const float iss_salient_radius, const float iss_non_max_radius, const float iss_gamma_21, const float iss_gamma_32,
                      const int iss_min_neighbors, const int iss_threads)
    {
        m_iss_salient_radius = iss_salient_radius; m_iss_non_max_radius = iss_non_max_radius; m_iss_gamma_21 = iss_gamma_21;
        m_iss_gamma_32 = iss_gamma_32; m_iss_min_neighbors = iss_min_neighbors; m_iss_threads = iss_threads;
    }
    void setHarris3Dparams(const float harris3d_radius, const float harris3d_nms_threshold, const int harris3d_threads, const bool harris3d_is_nms,
                           const bool harris3d_is_refine)
    {
        m_harris3d_radius = harris3d_radius; m_harris3d_nms_threshold = harris3d_nms_threshold; m_harris3d_threads = harris3d_threads;
        m_harris3d_is_nms = harris3d_is_nms; m_harris3d_is_refine = harris3d_is_refine;
    }
    void setFPFHparams(const float fpfh_feature_radius) { m_fpfh_feature_radius = fpfh_feature_radius; }
    void setSHOTparams(const float shot_feature_radius) { m_shot_feature_radius = shot_feature_radius; }
    void setRANSACparams(const uint32_t max_iter, const float dist_threshold, const float angle_threshold, const float corres_rejection_rate)
    {
        m_greg.setRANSACparams(max_iter, dist_threshold, angle_threshold, corres_rejection_rate);
    }
    // registration.hpp:126-137
    void setICPparams(const int normal_bins, const size_t sampled_size, const float max_corres_dist, const size_t max_iter, const float loss_epsilon)
    {
        m_ICP_normal_bins = normal_bins; m_ICP_sampled_size = sampled_size; m_ICP_max_corres_dist = max_corres_dist;
        m_ICP_max_iter = max_iter; m_ICP_loss_epsilon = loss_epsilon;
    }

    // The PCL-internal stages of compute() / ICPpoint2point().  Unset keypoints or fpfh33: compute() has no global
    // registration to run and starts ICP from the identity (gpuHarris3DStage() / gpuFPFH33Stage() below are GPU bodies for them).  Unset
    // normal_space_sampling: ICP runs on the full clouds (the reference's own commented alternative, registration.cpp:883-884);
    // gpuNormalSpaceSamplingStage() / gpuVoxelGridSamplingStage() below are GPU bodies for it.
    struct Stages {
        // getHarris3DKeypoints (registration.hpp:152-154, registration.cpp:214-251)
        std::function<void(const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& keypoints_cloud)> keypoints;
        // getFPFH33Descriptors (registration.hpp:156-159, registration.cpp:253-272)
        std::function<void(const PointCloud& input_cloud, const PointCloud& input_keypoints_cloud, const NormalCloud& input_normals,
                           pcl::PointCloud<pcl::FPFHSignature33>& fpfh_descriptors)> fpfh33;
        // normalSpaceSampling (registration.hpp:170-173, registration.cpp:630-662)
        std::function<void(const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& sampled_cloud, NormalCloud& sampled_normals)>
            normal_space_sampling;
    } stages;

    // getFPFH33Descriptors on the GPU (pcr_fpfh33_f32, include/pcr.h: the library's restatement of PCL's FPFHEstimation) with the
    // radius of setFPFHparams, read when the stage runs.  Opt-in: `reg.stages.fpfh33 = reg.gpuFPFH33Stage();`;
    // an unset stage keeps its meaning.  The stage refers to this Registration, so it must not outlive it.
    decltype(Stages::fpfh33) gpuFPFH33Stage()
    {
        return [this](const PointCloud& input_cloud, const PointCloud& input_keypoints_cloud, const NormalCloud& input_normals,
                      pcl::PointCloud<pcl::FPFHSignature33>& fpfh_descriptors) {
            gpuFPFH33(input_cloud, input_keypoints_cloud, input_normals, fpfh_descriptors);
        };
    }

    // getHarris3DKeypoints on the GPU (pcr_harris3d_f32, include/pcr.h: the library's restatement of PCL's HarrisKeypoint3D, method
    // HARRIS) with the radius, threshold and nms flag of setHarris3Dparams, read when the stage runs (threads: ignored; is_refine =
    // true is not provided and is reported like a failed call).  Opt-in: `reg.stages.keypoints = reg.gpuHarris3DStage();`
    // (INTEGRATION.md, hw9); an unset stage keeps its meaning.  The stage refers to this Registration, so it must not outlive it.
    decltype(Stages::keypoints) gpuHarris3DStage()
    {
        return [this](const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& keypoints_cloud) {
            gpuHarris3D(input_cloud, input_normals, keypoints_cloud);
        };
    }

    // normalSpaceSampling on the GPU (pcr_normal_space_sample_f32, include/pcr.h: the library's restatement of PCL's NormalSpaceSampling —
    // PCL's round-robin over the normal bins with the library's own seeded keys, not boost's stream) with the bins and the sample size
    // of setICPparams, read when the stage runs, and seed 0 (registration.cpp:638-640).  Opt-in:
    // `reg.stages.normal_space_sampling = reg.gpuNormalSpaceSamplingStage();`; an unset stage keeps its meaning
    // (ICP on the full clouds).  Fewer samplable points than the sample size: all of them come back (the reference asserts instead, :646).
    // The stage refers to this Registration, so it must not outlive it.
    decltype(Stages::normal_space_sampling) gpuNormalSpaceSamplingStage()
    {
        return [this](const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& sampled_cloud, NormalCloud& sampled_normals) {
            gpuNormalSpaceSampling(input_cloud, input_normals, sampled_cloud, sampled_normals);
        };
    }

    // VoxelGridSampling (registration.hpp:175-177, registration.cpp:665-707: the reference's own commented alternative, :883-884) as a
    // second body for the same stage: the voxel grid over points and normals at leaf 1.75 (pcr_voxel_grid_normals_f32, normal_mode 1).
    decltype(Stages::normal_space_sampling) gpuVoxelGridSamplingStage()
    {
        return [](const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& sampled_cloud, NormalCloud& sampled_normals) {
            voxelGridWithNormals(input_cloud, input_normals, 1.75f, sampled_cloud, sampled_normals);
        };
    }

    uint64_t ransac_seed = 5489u;          // the reference seeds std::mt19937 from std::random_device (registration.cpp:298-299)
    pcr_icp_stats last_icp_stats{};        // iterations run, kept pairs, ... of the last ICP
    bool use_point2plane = false;          // compute() calls ICPpoint2point (registration.cpp:1150); the sibling is selectable

    // registration.hpp:139-144 / registration.cpp:1014-1157
    void compute(const PointCloud& cloud_source, const PointCloud& cloud_target, const NormalCloud& normals_source, const NormalCloud& normals_target,
                 Eigen::Matrix3f& R, Eigen::Vector3f& t)
    {
        Eigen::Matrix3f init_R = Eigen::Matrix3f::Identity();
        Eigen::Vector3f init_t = Eigen::Vector3f::Zero();
        if (stages.keypoints && stages.fpfh33) {
            PointCloud kp_cloud_source, kp_cloud_target;
            stages.keypoints(cloud_source, normals_source, kp_cloud_source);                     // :1030-1031
            stages.keypoints(cloud_target, normals_target, kp_cloud_target);
            pcl::PointCloud<pcl::FPFHSignature33> fpfh_source, fpfh_target;
            stages.fpfh33(cloud_source, kp_cloud_source, normals_source, fpfh_source);           // :1071-1072
            stages.fpfh33(cloud_target, kp_cloud_target, normals_target, fpfh_target);
            std::vector<std::vector<size_t>> correspondences;
            findRANSACCorrespondencesUnion(fpfh_source, fpfh_target, correspondences);           // :1080
            if (correspondences.size() < 4) {                                                    // :1087-1091
                std::cerr << "Correspondences are fewer than 4! Failed!" << std::endl;
                return;
            }
            RANSAC(correspondences, kp_cloud_source, kp_cloud_target, init_R, init_t);           // :1133
        }
        R = init_R;                                                                              // :1136-1137
        t = init_t;
        if (use_point2plane) ICPpoint2plane(init_R, init_t, cloud_source, cloud_target, normals_source, normals_target, R, t);
        else ICPpoint2point(init_R, init_t, cloud_source, cloud_target, normals_source, normals_target, R, t);   // :1150
    }

private:
    // registration.hpp:179-185 / registration.cpp:288-434
    void RANSAC(const std::vector<std::vector<size_t>>& correspondences, const PointCloud& kp_cloud_source, const PointCloud& kp_cloud_target,
                Eigen::Matrix3f& R, Eigen::Vector3f& t)
    {
        std::vector<float> ks = xyz3(kp_cloud_source), kt = xyz3(kp_cloud_target);
        float Rr[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, tr[3] = { 0, 0, 0 };
        to_rows(R, t, Rr, tr);                          // written only when a non-empty consensus set exists (:423-428)
        m_greg.seed = ransac_seed;
        check(m_greg.RANSAC(correspondences, ks.data(), kp_cloud_source.size(), kt.data(), kp_cloud_target.size(), Rr, tr), "pcr_ransac_global_f32");
        from_rows(Rr, tr, R, t);
    }

    // registration.hpp:187-189 / registration.cpp:437-533
    void findRANSACCorrespondencesInter(const pcl::PointCloud<pcl::FPFHSignature33>& fpfh_source, const pcl::PointCloud<pcl::FPFHSignature33>& fpfh_target,
                                        std::vector<std::vector<size_t>>& correspondences)
    {
        std::vector<float> a = rows33(fpfh_source), b = rows33(fpfh_target);
        m_greg.findRANSACCorrespondencesInter(a.data(), fpfh_source.size(), b.data(), fpfh_target.size(), 33, correspondences);
    }

    // registration.hpp:191-193 / registration.cpp:535-615
    void findRANSACCorrespondencesUnion(const pcl::PointCloud<pcl::FPFHSignature33>& fpfh_source, const pcl::PointCloud<pcl::FPFHSignature33>& fpfh_target,
                                        std::vector<std::vector<size_t>>& correspondences)
    {
        std::vector<float> a = rows33(fpfh_source), b = rows33(fpfh_target);
        m_greg.findRANSACCorrespondencesUnion(a.data(), fpfh_source.size(), b.data(), fpfh_target.size(), 33, correspondences);
    }

    // registration.hpp:195-202 / registration.cpp:710-860
    void ICPpoint2plane(const Eigen::Matrix3f& init_R, const Eigen::Vector3f& init_t, const PointCloud& input_cloud_src, const PointCloud& input_cloud_tar,
                        const NormalCloud& input_normals_src, const NormalCloud& input_normals_tar, Eigen::Matrix3f& R, Eigen::Vector3f& t)
    {
        run_icp(true, init_R, init_t, input_cloud_src, input_cloud_tar, input_normals_src, input_normals_tar, R, t);
    }

    // registration.hpp:204-211 / registration.cpp:862-1011
    void ICPpoint2point(const Eigen::Matrix3f& init_R, const Eigen::Vector3f& init_t, const PointCloud& input_cloud_src, const PointCloud& input_cloud_tar,
                        const NormalCloud& input_normals_src, const NormalCloud& input_normals_tar, Eigen::Matrix3f& R, Eigen::Vector3f& t)
    {
        run_icp(false, init_R, init_t, input_cloud_src, input_cloud_tar, input_normals_src, input_normals_tar, R, t);
    }

    // Both ICP members share their prologue in the reference (:870-881 == :718-729): the source is moved by the R, t passed IN
    // (pre-loaded with the initial guess by compute(), :1136-1137), both clouds are normal-space sampled, T_total starts from
    // init_R / init_t (:910-913).  compute() passes the same pose twice; when a caller does not, the in/out pose moves the
    // source and init_R / init_t seed T_total, as written there.
    void run_icp(bool plane, const Eigen::Matrix3f& init_R, const Eigen::Vector3f& init_t, const PointCloud& input_cloud_src,
                 const PointCloud& input_cloud_tar, const NormalCloud& input_normals_src, const NormalCloud& input_normals_tar, Eigen::Matrix3f& R,
                 Eigen::Vector3f& t)
    {
        float Rin[9], tin[3], Ri[9], ti[3];
        to_rows(R, t, Rin, tin);
        to_rows(init_R, init_t, Ri, ti);
        bool same = true;
        for (int k = 0; k < 9; k++) same = same && Rin[k] == Ri[k];
        for (int k = 0; k < 3; k++) same = same && tin[k] == ti[k];
        const PointCloud* src = &input_cloud_src;
        const PointCloud* tgt = &input_cloud_tar;
        const NormalCloud* ntgt = &input_normals_tar;
        PointCloud trans_cloud_src, sampled_cloud_src, sampled_cloud_tar;
        NormalCloud trans_normals_src, sampled_normals_src, sampled_normals_tar;
        bool moved = false;                                   // the source handed to the library has R, t applied already
        if (stages.normal_space_sampling || !same) {
            trans_cloud_src = input_cloud_src;                                                   // :872-875
            trans_normals_src = input_normals_src;
            transformCloudInplace(trans_cloud_src, R, t);
            transformNormalsInplace(trans_normals_src, R, t);
            moved = true;
            src = &trans_cloud_src;
            if (stages.normal_space_sampling) {                                                  // :880-881
                stages.normal_space_sampling(trans_cloud_src, trans_normals_src, sampled_cloud_src, sampled_normals_src);
                stages.normal_space_sampling(input_cloud_tar, input_normals_tar, sampled_cloud_tar, sampled_normals_tar);
                src = &sampled_cloud_src;
                tgt = &sampled_cloud_tar;
                ntgt = &sampled_normals_tar;
            }
        }
        pcr_ctx* ctx = default_ctx();
        pcr_cloud *cs = nullptr, *ct = nullptr, *cn = nullptr;
        int rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(src->points.data()), src->size(), PCR_AOS4, &cs);
        if (rc == PCR_OK) rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(tgt->points.data()), tgt->size(), PCR_AOS4, &ct);
        if (rc == PCR_OK && plane) {
            std::vector<float> n3(3 * ntgt->size() + 3);
            for (size_t i = 0; i < ntgt->size(); i++) {
                n3[3 * i] = ntgt->points[i].normal_x; n3[3 * i + 1] = ntgt->points[i].normal_y; n3[3 * i + 2] = ntgt->points[i].normal_z;
            }
            rc = pcr_cloud_create(ctx, n3.data(), ntgt->size(), PCR_AOS3, &cn);
        }
        float out_T[16];
        if (rc == PCR_OK) {
            const float I16[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
            const float init_T[16] = { Ri[0], Ri[1], Ri[2], ti[0], Ri[3], Ri[4], Ri[5], ti[1], Ri[6], Ri[7], Ri[8], ti[2], 0, 0, 0, 1 };
            pcr_icp_params prm;
            prm.max_corr = m_ICP_max_corres_dist;
            prm.max_iter = m_ICP_max_iter;
            prm.eps = m_ICP_loss_epsilon;
            // the library moves the source by init_T itself and starts T_total from it; a source moved here starts from I
            const float* T0 = moved ? I16 : init_T;
            rc = plane ? pcr_icp_p2plane_f32(ctx, cs, ct, cn, T0, &prm, out_T, &last_icp_stats) : pcr_icp_p2p_f32(ctx, cs, ct, T0, &prm, out_T, &last_icp_stats);
            if (rc == PCR_OK && moved) {
                // T_total = (T_delta_k ... T_delta_1) * [init_R init_t]: the product of the deltas times the seed of :910-913.
                // (The reference folds the seed in first; the f32 rounding of the 4x4 products may differ in the last bit.)
                float seeded[16];
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) {
                        float acc = out_T[4 * r] * init_T[c];
                        acc = acc + out_T[4 * r + 1] * init_T[4 + c];
                        acc = acc + out_T[4 * r + 2] * init_T[8 + c];
                        acc = acc + out_T[4 * r + 3] * init_T[12 + c];
                        seeded[4 * r + c] = acc;
                    }
                for (int k = 0; k < 16; k++) out_T[k] = seeded[k];
            }
        }
        pcr_cloud_destroy(ctx, cs);
        pcr_cloud_destroy(ctx, ct);
        pcr_cloud_destroy(ctx, cn);
        check(rc, plane ? "pcr_icp_p2plane_f32" : "pcr_icp_p2p_f32");
        for (int r = 0; r < 3; ++r) {                                                            // :1008-1009
            for (int c = 0; c < 3; ++c) R(r, c) = out_T[4 * r + c];
            t(r) = out_T[4 * r + 3];
        }
    }

    // the body of gpuNormalSpaceSamplingStage: the sampled points and their normals in the order of the draw, filled as :641-660 does
    void gpuNormalSpaceSampling(const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& sampled_cloud, NormalCloud& sampled_normals) const
    {
        const size_t n = input_normals.size();
        std::vector<uint32_t> indices(n + 1);
        size_t m = 0;
        int rc = input_cloud.size() == n && m_ICP_normal_bins >= 1 ? PCR_OK : PCR_ERR_ARG;
        if (rc == PCR_OK) {
            std::vector<float> n3(3 * n + 3);
            for (size_t i = 0; i < n; i++) {
                n3[3 * i] = input_normals.points[i].normal_x; n3[3 * i + 1] = input_normals.points[i].normal_y; n3[3 * i + 2] = input_normals.points[i].normal_z;
            }
            pcr_ctx* ctx = default_ctx();
            pcr_cloud* cn = nullptr;
            const uint32_t bins[3] = { (uint32_t)m_ICP_normal_bins, (uint32_t)m_ICP_normal_bins, (uint32_t)m_ICP_normal_bins };
            rc = pcr_cloud_create(ctx, n3.data(), n, PCR_AOS3, &cn);
            if (rc == PCR_OK) rc = pcr_normal_space_sample_f32(ctx, cn, bins, m_ICP_sampled_size, 0, indices.data(), &m, nullptr, nullptr, nullptr);
            pcr_cloud_destroy(ctx, cn);
        }
        check(rc, "pcr_normal_space_sample_f32");
        sampled_cloud.points.clear();
        NormalCloud new_normals;
        for (size_t i = 0; i < m; i++) {
            sampled_cloud.points.push_back(input_cloud.points[indices[i]]);
            NormalT nn;
            nn.normal_x = input_normals.points[indices[i]].normal_x;
            nn.normal_y = input_normals.points[indices[i]].normal_y;
            nn.normal_z = input_normals.points[indices[i]].normal_z;
            new_normals.points.push_back(nn);
        }
        sampled_cloud.height = 1;
        sampled_cloud.width = (uint32_t)m;
        sampled_cloud.is_dense = true;
        new_normals.height = 1;                                                                  // :651-653
        new_normals.width = (uint32_t)m;
        new_normals.is_dense = true;
        sampled_normals = new_normals;
    }

    // the body of gpuHarris3DStage: the keypoints in ascending input index, filled as registration.cpp:239-249 does
    void gpuHarris3D(const PointCloud& input_cloud, const NormalCloud& input_normals, PointCloud& keypoints_cloud) const
    {
        const size_t n = input_cloud.size();
        std::vector<uint8_t> key(n + 1, 0);
        int rc = m_harris3d_is_refine ? PCR_ERR_ARG : PCR_OK;                                    // setRefine(true): not provided
        if (rc == PCR_OK && n > 0) {
            std::vector<float> n3(3 * input_normals.size() + 3);
            for (size_t i = 0; i < input_normals.size(); i++) {
                n3[3 * i] = input_normals.points[i].normal_x; n3[3 * i + 1] = input_normals.points[i].normal_y; n3[3 * i + 2] = input_normals.points[i].normal_z;
            }
            pcr_ctx* ctx = default_ctx();
            pcr_cloud *cs = nullptr, *cn = nullptr;
            pcr_harris3d_params prm;
            prm.radius = m_harris3d_radius; prm.threshold = m_harris3d_nms_threshold; prm.method = 0;
            prm.non_max_suppression = m_harris3d_is_nms ? 1 : 0;
            rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(input_cloud.points.data()), n, PCR_AOS4, &cs);
            if (rc == PCR_OK) rc = pcr_cloud_create(ctx, n3.data(), input_normals.size(), PCR_AOS3, &cn);
            if (rc == PCR_OK) rc = pcr_harris3d_f32(ctx, cs, cn, &prm, key.data(), nullptr, nullptr, nullptr);
            pcr_cloud_destroy(ctx, cs);
            pcr_cloud_destroy(ctx, cn);
        }
        check(rc, m_harris3d_is_refine ? "pcr_harris3d_f32: setRefine(true) is not provided" : "pcr_harris3d_f32");
        keypoints_cloud.points.clear();
        for (size_t i = 0; i < n; i++)
            if (key[i]) keypoints_cloud.points.push_back(input_cloud.points[i]);
        keypoints_cloud.height = 1;                                                              // :246-248
        keypoints_cloud.width = (uint32_t)keypoints_cloud.points.size();
        keypoints_cloud.is_dense = true;
    }

    // the body of gpuFPFH33Stage: one row per keypoint, NaN rows (and is_dense = false) where PCL's computeFeature writes them
    void gpuFPFH33(const PointCloud& input_cloud, const PointCloud& input_keypoints_cloud, const NormalCloud& input_normals,
                   pcl::PointCloud<pcl::FPFHSignature33>& fpfh_descriptors) const
    {
        const size_t m = input_keypoints_cloud.size(), n = input_cloud.size();
        std::vector<float> rows(33 * m + 33, std::numeric_limits<float>::quiet_NaN());
        int rc = PCR_OK;
        if (m > 0 && n > 0) {
            std::vector<float> n3(3 * input_normals.size() + 3);
            for (size_t i = 0; i < input_normals.size(); i++) {
                n3[3 * i] = input_normals.points[i].normal_x; n3[3 * i + 1] = input_normals.points[i].normal_y; n3[3 * i + 2] = input_normals.points[i].normal_z;
            }
            pcr_ctx* ctx = default_ctx();
            pcr_cloud *cs = nullptr, *ck = nullptr, *cn = nullptr;
            rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(input_cloud.points.data()), n, PCR_AOS4, &cs);
            if (rc == PCR_OK) rc = pcr_cloud_create(ctx, reinterpret_cast<const float*>(input_keypoints_cloud.points.data()), m, PCR_AOS4, &ck);
            if (rc == PCR_OK) rc = pcr_cloud_create(ctx, n3.data(), input_normals.size(), PCR_AOS3, &cn);
            if (rc == PCR_OK) rc = pcr_fpfh33_f32(ctx, cs, cn, ck, m_fpfh_feature_radius, rows.data(), nullptr, nullptr);
            pcr_cloud_destroy(ctx, cs);
            pcr_cloud_destroy(ctx, ck);
            pcr_cloud_destroy(ctx, cn);
        }
        check(rc, "pcr_fpfh33_f32");
        fpfh_descriptors.points.resize(m);
        fpfh_descriptors.width = (uint32_t)m;
        fpfh_descriptors.height = 1;
        fpfh_descriptors.is_dense = true;
        for (size_t i = 0; i < m; i++)
            for (int k = 0; k < 33; k++) {
                const float v = rows[33 * i + k];
                fpfh_descriptors.points[i].histogram[k] = v;
                if (v != v) fpfh_descriptors.is_dense = false;
            }
    }

    static void to_rows(const Eigen::Matrix3f& R, const Eigen::Vector3f& t, float Rr[9], float tr[3])
    {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rr[3 * r + c] = R(r, c);
            tr[r] = t(r);
        }
    }
    static void from_rows(const float Rr[9], const float tr[3], Eigen::Matrix3f& R, Eigen::Vector3f& t)
    {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R(r, c) = Rr[3 * r + c];
            t(r) = tr[r];
        }
    }
    static std::vector<float> xyz3(const PointCloud& c)
    {
        std::vector<float> v(3 * c.size() + 3);
        for (size_t i = 0; i < c.size(); i++) { v[3 * i] = c.points[i].x; v[3 * i + 1] = c.points[i].y; v[3 * i + 2] = c.points[i].z; }
        return v;
    }
    static std::vector<float> rows33(const pcl::PointCloud<pcl::FPFHSignature33>& f)
    {
        std::vector<float> v(33 * f.size() + 33);
        for (size_t i = 0; i < f.size(); i++)
            for (int k = 0; k < 33; k++) v[33 * i + k] = f.points[i].histogram[k];
        return v;
    }

private:
    float m_iss_salient_radius = 0.f, m_iss_non_max_radius = 0.f, m_iss_gamma_21 = 0.f, m_iss_gamma_32 = 0.f;
    int m_iss_min_neighbors = 0, m_iss_threads = 0;
    float m_harris3d_radius = 0.f, m_harris3d_nms_threshold = 0.f;
    int m_harris3d_threads = 0;
    bool m_harris3d_is_nms = false, m_harris3d_is_refine = false;
    float m_fpfh_feature_radius = 0.f, m_shot_feature_radius = 0.f;
    // defaults = the shipped parameters, Homework9/hw9/main.cpp:88-95
    int m_ICP_normal_bins = 10;
    size_t m_ICP_sampled_size = 4000;
    float m_ICP_max_corres_dist = 1.0f;
    size_t m_ICP_max_iter = 800;
    float m_ICP_loss_epsilon = 1e-8f;
    GlobalRegistration m_greg;
};

}  // namespace pcr
#endif
#endif

#endif  // PCR_DROPIN_REGISTRATION_HPP
