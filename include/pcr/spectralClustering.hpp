// spectralClustering.hpp — drop-in for Homework3/hw3/include/spectralClustering.hpp: the same public spelling (my_matrix_t, class Spec_Cluster
// with the (int, size_t) constructor and fit(const my_matrix_t&), readPoints, converged), the work done by libpcr_hip.so on the GPU
// (pcr_spectral_cluster_f64, include/pcr.h).  Needs neither Eigen, Spectra nor Boost.  Not provided: the (double r, size_t) constructor — it
// selects buildRNNGraph, which the reference never calls — and initial_choice, whose signature is an Eigen matrix.
#ifndef HW3_SPECTRALCLUSTERING_HPP
#define HW3_SPECTRALCLUSTERING_HPP

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "pcr_host.hpp"

typedef std::vector<std::vector<double>> my_matrix_t;

class Spec_Cluster
{
private:
    size_t K_clusters;
    size_t K_neighbors;
    size_t K_clusters_estimation;
    size_t forced_clusters;
    pcr_spectral_info last_info;

public:
    Spec_Cluster(int k_neigh, size_t k_clus_estimation)
    {
        K_neighbors = k_neigh;
        K_clusters = 1;
        K_clusters_estimation = k_clus_estimation;
        forced_clusters = 0;
        last_info = pcr_spectral_info();
    }

    // extensions: K fixed instead of the eigengap rule (0 = the rule), and what the last fit found
    void set_n_clusters(size_t k) { forced_clusters = k; }
    size_t n_clusters() const { return K_clusters; }
    const pcr_spectral_info& info() const { return last_info; }

    std::vector<int> fit(const my_matrix_t& points)
    {
        const size_t N = points.size();
        if (N == 0) throw std::runtime_error("Spec_Cluster::fit: no points");
        const size_t dim = points[0].size();
        std::vector<double> rows(N * dim);
        for (size_t i = 0; i < N; i++) {
            if (points[i].size() != dim) throw std::runtime_error("Spec_Cluster::fit: ragged points");
            for (size_t d = 0; d < dim; d++) rows[i * dim + d] = points[i][d];
        }
        pcr_ctx* ctx = pcr::default_ctx();
        pcr_mat64* m = nullptr;
        pcr::check(pcr_mat64_create(ctx, rows.data(), N, (int)dim, &m), "pcr_mat64_create");
        std::vector<int32_t> labels(N);
        const int rc = pcr_spectral_cluster_f64(ctx, m, (int)K_neighbors, (int)K_clusters_estimation, (int)forced_clusters, labels.data(), nullptr, &last_info);
        pcr_mat64_destroy(ctx, m);
        if (rc < 0) pcr::check(rc, "pcr_spectral_cluster_f64");
        if (rc > 0) throw std::runtime_error("Spec_Cluster::fit: status " + std::to_string(rc) + " (include/pcr.h: PCR_EMPTY_CLUSTER / PCR_SPECTRAL_*)");
        K_clusters = (size_t)last_info.k_clusters;
        std::cout << "Clusters number = " << K_clusters << std::endl;
        return std::vector<int>(labels.begin(), labels.end());
    }
};

// the reference splits every line at ',' and keeps the first two fields (spectralClustering.cpp:430-455)
inline my_matrix_t readPoints(const std::string& path)
{
    std::cout << "Read points from " << path << std::endl;
    my_matrix_t points;
    std::ifstream file(path);
    if (!file.good()) {
        std::cerr << "Read file " << path << "failed!";
        exit(EXIT_FAILURE);
    }
    std::string line;
    while (getline(file, line)) {
        const size_t comma = line.find(',');
        if (comma == std::string::npos) continue;
        points.emplace_back(std::vector<double>{ std::stod(line.substr(0, comma)), std::stod(line.substr(comma + 1)) });
    }
    file.close();
    std::cout << "Points dim = " << points.size() << ", " << (points.empty() ? 0 : points[0].size()) << std::endl;
    return points;
}

inline bool converged(const my_matrix_t& A, const my_matrix_t& B, double threshold)
{
    for (size_t i = 0; i < A.size(); i++)
        for (size_t j = 0; j < A[i].size(); j++)
            if (!(std::fabs(A[i][j] - B[i][j]) < threshold)) return false;
    return true;
}

#endif  // HW3_SPECTRALCLUSTERING_HPP
