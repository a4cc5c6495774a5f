// hw3_spectral_driver.cpp — what Homework3/hw3/main.cpp does, without Eigen or Boost: for each of the five data sets read ../data/<set>.txt,
// run Spec_Cluster(10, 8).fit on the GPU through the drop-in header, and write one label per line to ../result/predict_<set>.txt.
//
//   usage: hw3_spectral_driver [<set>=<K> ...]        e.g. blobs=3 fixes the number of clusters of one set instead of the eigengap rule
//   build: g++ -std=c++14 -Iinclude/pcr examples/hw3_spectral_driver.cpp -L<libdir> -lpcr_hip
#include "spectralClustering.hpp"

#include <fstream>
#include <iostream>
#include <map>

int main(int argc, char** argv)
{
    std::vector<std::string> files = { "aniso.txt", "blobs.txt", "circle.txt", "moons.txt", "varied.txt" };
    std::map<std::string, size_t> forced;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) { std::cerr << "usage: hw3_spectral_driver [<set>=<K> ...]" << std::endl; return 2; }
        forced[arg.substr(0, eq) + ".txt"] = (size_t)std::stoul(arg.substr(eq + 1));
    }
    for (auto& file : files) {
        std::cout << "********* Data set: " << file << " *********" << std::endl;
        auto points = readPoints("../data/" + file);
        Spec_Cluster test_sc(10, 8);
        if (forced.count(file)) test_sc.set_n_clusters(forced[file]);
        auto result = test_sc.fit(points);
        const pcr_spectral_info& info = test_sc.info();
        std::cout << "Eigenvalues found" << std::endl;
        for (int j = 0; j < info.n_eig; j++) std::cout << info.eigenvalues[j] << std::endl;
        std::cout << "Solver steps = " << info.solver_steps << ", residual = " << info.residual << ", K-Means passes = " << info.kmeans_iters << std::endl;
        std::ofstream output("../result/predict_" + file);
        for (auto& item : result) output << item << std::endl;
        output.close();
        std::cout << "Done!\n" << std::endl;
    }
    return 0;
}
