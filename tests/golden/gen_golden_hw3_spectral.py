"""Writes tests/golden/hw3_spectral_ref.npz: the labels the reference's spectral-clustering binary recorded for its five data sets
(Homework3/hw3/result/predict_<name>.txt, one integer per line, 1 500 lines each).  The fixture holds DATA only.

The clouds themselves (Homework3/hw3/data/<name>.txt) are already in tests/golden/hw3_clustering_ref.npz as data_<name>; this script checks
that they are the same bits and stores a cloud again only if they are not (clouds_shared = 1 says none had to be).

Runs on a CPU (numpy):   python tests/golden/gen_golden_hw3_spectral.py <reference root>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = ("aniso", "blobs", "circle", "moons", "varied")


def main(root):
    have = np.load(os.path.join(HERE, "hw3_clustering_ref.npz"))
    out = {}
    shared = 1
    for name in SETS:
        x = np.loadtxt(os.path.join(root, f"Homework3/hw3/data/{name}.txt"), delimiter=",")
        labels = np.loadtxt(os.path.join(root, f"Homework3/hw3/result/predict_{name}.txt"), dtype=np.int64)
        assert x.shape == (1500, 2) and labels.shape == (1500,) and labels.min() == 0 and labels.max() < 8
        if not (f"data_{name}" in have.files and np.array_equal(have[f"data_{name}"], x)):
            out[f"data_{name}"] = x
            shared = 0
        out[f"labels_{name}"] = labels.astype(np.uint8)
        print(name, "clusters", np.bincount(labels).tolist())
    out["clouds_shared"] = np.int32(shared)
    path = os.path.join(HERE, "hw3_spectral_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", "clouds shared" if shared else "clouds stored")


if __name__ == "__main__":
    main(sys.argv[1])
