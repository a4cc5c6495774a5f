// TEST-ONLY stand-in (tests/mock/README.md): the record layout of pcl::PointNormal, which <pcl/point_types.h> only declares — in PCL
// itself this header is where the point structs are defined, and <pcl/point_types.h> includes it.
#pragma once
namespace pcl {
struct alignas(16) PointNormal {
    union {
        float data[4];
        struct { float x, y, z; };
    };
    union {
        float data_n[4];
        float normal[3];
        struct { float normal_x, normal_y, normal_z; };
    };
    union {
        struct { float curvature; };
        float data_c[4];
    };
    PointNormal() : data{ 0.f, 0.f, 0.f, 1.f }, data_n{ 0.f, 0.f, 0.f, 0.f }, data_c{ 0.f, 0.f, 0.f, 0.f } {}
};
}  // namespace pcl
