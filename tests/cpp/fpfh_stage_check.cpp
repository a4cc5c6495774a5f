// The GPU FPFH33 stage of the drop-in Registration (include/pcr/registration.hpp, gpuFPFH33Stage) driven through the reference's
// own stage signature, compiled against the test-only PCL / Eigen stand-ins of tests/mock/ (tests/test_fpfh.py).
// usage: fpfh_stage_check scene.bin out.bin
//   scene.bin: u32 n, u32 m, f32 radius, then surface [n][3], normals [n][3], keypoints [m][3] (f32)
//   out.bin:   u32 m, u32 is_dense, then the m x 33 descriptor rows (f32)
#include <cstdio>
#include <type_traits>
#include <vector>

#include "registration.hpp"

static_assert(std::is_same<decltype(std::declval<pcr::Registration&>().gpuFPFH33Stage()), decltype(pcr::Registration::Stages::fpfh33)>::value,
              "gpuFPFH33Stage() returns a Stages::fpfh33 body");

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t n = 0, m = 0;
    float radius = 0.f;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&m, 4, 1, f) != 1 || std::fread(&radius, 4, 1, f) != 1) return 4;
    std::vector<float> s(3 * (size_t)n), nr(3 * (size_t)n), k(3 * (size_t)m);
    if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(nr.data(), 4, nr.size(), f) != nr.size() || std::fread(k.data(), 4, k.size(), f) != k.size())
        return 5;
    std::fclose(f);
    pcr::PointCloud surface, keypoints;
    pcr::NormalCloud normals;
    for (uint32_t i = 0; i < n; i++) {
        surface.push_back(pcl::PointXYZ(s[3 * i], s[3 * i + 1], s[3 * i + 2]));
        pcl::Normal nn;
        nn.normal_x = nr[3 * i]; nn.normal_y = nr[3 * i + 1]; nn.normal_z = nr[3 * i + 2];
        normals.push_back(nn);
    }
    for (uint32_t i = 0; i < m; i++) keypoints.push_back(pcl::PointXYZ(k[3 * i], k[3 * i + 1], k[3 * i + 2]));

    pcr::Registration reg;
    reg.setFPFHparams(radius);
    reg.stages.fpfh33 = reg.gpuFPFH33Stage();                // the INTEGRATION.md snippet
    pcl::PointCloud<pcl::FPFHSignature33> out;
    reg.stages.fpfh33(surface, keypoints, normals, out);

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const uint32_t hdr[2] = { (uint32_t)out.size(), out.is_dense ? 1u : 0u };
    std::fwrite(hdr, 4, 2, o);
    for (size_t i = 0; i < out.size(); i++) std::fwrite(out.points[i].histogram, 4, 33, o);
    std::fclose(o);
    std::printf("fpfh stage: %zu rows\n", out.size());
    return 0;
}
