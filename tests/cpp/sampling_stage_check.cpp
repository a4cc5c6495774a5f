// The sampling pieces of the drop-in Registration (include/pcr/registration.hpp): pcr::readBinaryAndVoxelDown with the reference's
// signature, gpuNormalSpaceSamplingStage() and gpuVoxelGridSamplingStage() driven through the reference's own stage signature, compiled
// against the test-only PCL / Eigen stand-ins of tests/mock/ (tests/test_voxel_grid_normals.py).
// usage: sampling_stage_check scan.bin voxel_size normal_bins sampled_size out.bin
//   scan.bin: hw9's rows, 6 f32 each (x y z nx ny nz)
//   out.bin:  three sections — the voxel grid of the file, its normal-space sample, its voxel-grid sample — each
//             u32 m, u32 flags (bit 0 width == m, bit 1 height == 1, bit 2 is_dense of the cloud; bits 3-5 the same of the normals),
//             points [m][3], normals [m][3] (f32)
// exit status 7: a stage threw (what() on stderr)
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <type_traits>

#include "registration.hpp"

static_assert(std::is_same<decltype(&pcr::readBinaryAndVoxelDown), void (*)(const std::string&, pcr::PointCloud&, pcr::NormalCloud&, float)>::value,
              "readBinaryAndVoxelDown has the reference's signature (registration.hpp:50-53)");
static_assert(std::is_same<decltype(std::declval<pcr::Registration&>().gpuNormalSpaceSamplingStage()),
                           decltype(pcr::Registration::Stages::normal_space_sampling)>::value,
              "gpuNormalSpaceSamplingStage() returns a Stages::normal_space_sampling body");
static_assert(std::is_same<decltype(std::declval<pcr::Registration&>().gpuVoxelGridSamplingStage()),
                           decltype(pcr::Registration::Stages::normal_space_sampling)>::value,
              "gpuVoxelGridSamplingStage() returns a Stages::normal_space_sampling body");
static_assert(sizeof(pcl::PointNormal) == 12 * sizeof(float), "pcl::PointNormal is a 48-byte xyz + normal + curvature record");

static void write_section(FILE* o, const pcr::PointCloud& c, const pcr::NormalCloud& n)
{
    const uint32_t m = (uint32_t)c.size();
    uint32_t flags = 0;
    if (c.width == m) flags |= 1u;
    if (c.height == 1) flags |= 2u;
    if (c.is_dense) flags |= 4u;
    if (n.width == m && n.size() == c.size()) flags |= 8u;
    if (n.height == 1) flags |= 16u;
    if (n.is_dense) flags |= 32u;
    std::fwrite(&m, 4, 1, o);
    std::fwrite(&flags, 4, 1, o);
    for (size_t i = 0; i < c.size(); i++) {
        const float p[3] = { c.points[i].x, c.points[i].y, c.points[i].z };
        std::fwrite(p, 4, 3, o);
    }
    for (size_t i = 0; i < n.size(); i++) {
        const float p[3] = { n.points[i].normal_x, n.points[i].normal_y, n.points[i].normal_z };
        std::fwrite(p, 4, 3, o);
    }
}

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const float voxel_size = (float)std::atof(argv[2]);
    const int bins = std::atoi(argv[3]);
    const size_t sampled = (size_t)std::atol(argv[4]);
    pcr::PointCloud cloud, sc, vc;
    pcr::NormalCloud normals, sn, vn;
    pcr::Registration reg;
    reg.stages.normal_space_sampling = reg.gpuNormalSpaceSamplingStage();      // the INTEGRATION.md snippet; the parameters are read when the stage runs
    reg.setICPparams(bins, sampled, 1.0f, 800, 1e-8f);
    try {
        pcr::readBinaryAndVoxelDown(argv[1], cloud, normals, voxel_size);
        reg.stages.normal_space_sampling(cloud, normals, sc, sn);
        reg.stages.normal_space_sampling = reg.gpuVoxelGridSamplingStage();
        reg.stages.normal_space_sampling(cloud, normals, vc, vn);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 7;
    }
    FILE* o = std::fopen(argv[5], "wb");
    if (!o) return 6;
    write_section(o, cloud, normals);
    write_section(o, sc, sn);
    write_section(o, vc, vn);
    std::fclose(o);
    std::printf("sampling stages: %zu voxels, %zu sampled, %zu voxel-sampled\n", cloud.size(), sc.size(), vc.size());
    return 0;
}
