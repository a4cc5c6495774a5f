// The GPU Harris3D stage of the drop-in Registration (include/pcr/registration.hpp, gpuHarris3DStage) driven through the reference's
// own stage signature, compiled against the test-only PCL / Eigen stand-ins of tests/mock/ (tests/test_harris3d.py).
// usage: harris_stage_check scene.bin out.bin
//   scene.bin: u32 n, f32 radius, f32 threshold, u32 is_nms, u32 is_refine, then points [n][3], normals [n][3] (f32)
//   out.bin:   u32 m, u32 width, u32 height, u32 is_dense, then the m keypoints [m][3] (f32)
// exit status 7: the stage threw (what() on stderr)
#include <cstdio>
#include <exception>
#include <type_traits>
#include <vector>

#include "registration.hpp"

static_assert(std::is_same<decltype(std::declval<pcr::Registration&>().gpuHarris3DStage()), decltype(pcr::Registration::Stages::keypoints)>::value,
              "gpuHarris3DStage() returns a Stages::keypoints body");

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t n = 0, is_nms = 0, is_refine = 0;
    float radius = 0.f, threshold = 0.f;
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&radius, 4, 1, f) != 1 || std::fread(&threshold, 4, 1, f) != 1 || std::fread(&is_nms, 4, 1, f) != 1 ||
        std::fread(&is_refine, 4, 1, f) != 1)
        return 4;
    std::vector<float> s(3 * (size_t)n), nr(3 * (size_t)n);
    if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(nr.data(), 4, nr.size(), f) != nr.size()) return 5;
    std::fclose(f);
    pcr::PointCloud cloud, keypoints;
    pcr::NormalCloud normals;
    for (uint32_t i = 0; i < n; i++) {
        cloud.push_back(pcl::PointXYZ(s[3 * i], s[3 * i + 1], s[3 * i + 2]));
        pcl::Normal nn;
        nn.normal_x = nr[3 * i]; nn.normal_y = nr[3 * i + 1]; nn.normal_z = nr[3 * i + 2];
        normals.push_back(nn);
    }

    pcr::Registration reg;
    reg.stages.keypoints = reg.gpuHarris3DStage();           // the INTEGRATION.md snippet; the parameters are read when the stage runs
    reg.setHarris3Dparams(radius, threshold, 8, is_nms != 0, is_refine != 0);
    try {
        reg.stages.keypoints(cloud, normals, keypoints);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 7;
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const uint32_t hdr[4] = { (uint32_t)keypoints.size(), keypoints.width, keypoints.height, keypoints.is_dense ? 1u : 0u };
    std::fwrite(hdr, 4, 4, o);
    for (size_t i = 0; i < keypoints.size(); i++) {
        const float p[3] = { keypoints.points[i].x, keypoints.points[i].y, keypoints.points[i].z };
        std::fwrite(p, 4, 3, o);
    }
    std::fclose(o);
    std::printf("harris stage: %zu keypoints\n", keypoints.size());
    return 0;
}
