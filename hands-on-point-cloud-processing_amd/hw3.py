"""Homework3's clustering classes on the GPU: K_Means (Homework3/hw3/sript/KMeans.py) and GMM (Homework3/hw3/sript/GMM.py with the working
`posterior` of Homework3/nano_vs_my/sript/GMM.py), with the reference's attributes and methods, behind the C ABI of include/pcr.h
(csrc/mixture.hip).  compare_cluster.py runs with its two import lines changed.  Spec_Cluster is the C++ class of
Homework3/hw3/spectralClustering.cpp (csrc/spectral.hip).

The reference draws its initial points unseeded.  Here the draws are keyed by `seed` (SplitMix64, include/pcr.h), or the initial indices
are given outright with `init_idx`.  There is no CPU fall-back: a missing library or GPU is an error.
"""
from __future__ import annotations

import numpy as np

from . import PCR_KMEANS_PY, Context, PcrError

_ctx = None


def _context() -> Context:
    global _ctx
    if _ctx is None or not _ctx.h:
        _ctx = Context(0)
    return _ctx


class K_Means(object):
    def __init__(self, n_clusters=2, tolerance=0.0001, max_iter=200, seed=0, init_idx=None, ctx=None):
        self.k_ = n_clusters
        self.tolerance_ = tolerance
        self.max_iter_ = max_iter
        self.center_ = None
        self.init_center = None
        self.seed = seed
        self.init_idx = None if init_idx is None else [int(i) for i in init_idx]
        self.iterations_ = 0
        self.status_ = 0                     # PCR_EMPTY_CLUSTER when a pass left a cluster without members (the loop stops there)
        self._ctx = ctx

    def init_choice(self, data, _mat=None):
        """kmeans++ with the reference's weights: exp(d) for points at least mean(d) away from the chosen ones"""
        if self.init_idx is not None:
            return list(self.init_idx)
        m = _mat if _mat is not None else (self._ctx or _context()).mat64(data)
        try:
            return [int(i) for i in m.kmeanspp_init(self.k_, 1.0, seed=self.seed)]
        finally:
            if _mat is None:
                m.free()

    def fit(self, data):
        data = np.ascontiguousarray(data, np.float64)
        m = (self._ctx or _context()).mat64(data)
        try:
            center = data[self.init_choice(data, m), :]
            self.init_center = center
            centres, _, self.iterations_, converged, self.status_ = m.kmeans_fit(center, self.tolerance_, self.max_iter_, PCR_KMEANS_PY, want_labels=False)
            if converged:
                self.center_ = centres
        finally:
            m.free()

    def predict(self, p_datas):
        if self.center_ is None:
            print("Fit model first!")
            return None
        m = (self._ctx or _context()).mat64(p_datas)
        try:
            return m.kmeans_predict(self.center_).astype(np.int64)
        finally:
            m.free()


class GMM(object):
    def __init__(self, n_clusters, max_iter=100, seed=0, init_idx=None, amplitude=0.3, eps=1e-4, ctx=None):
        self.n_clusters = n_clusters
        self.max_iter = max_iter
        self.model_params = None
        self.init_center = None
        self.seed = seed
        self.init_idx = None if init_idx is None else [int(i) for i in init_idx]
        self.amplitude = amplitude
        self.eps = eps
        self.iterations_ = 0
        self.resets_ = 0                     # how often the reference's ||Sigma_k|| < 0.01 rule re-seeded a component
        self._ctx = ctx

    def init_choice(self, data, _mat=None):
        if self.init_idx is not None:
            return list(self.init_idx)
        m = _mat if _mat is not None else (self._ctx or _context()).mat64(data)
        try:
            return [int(i) for i in m.kmeanspp_init(self.n_clusters, 1.25, seed=self.seed)]
        finally:
            if _mat is None:
                m.free()

    def fit(self, data):
        data = np.ascontiguousarray(data, np.float64)
        m = (self._ctx or _context()).mat64(data)
        try:
            mean_k = data[self.init_choice(data, m)]
            self.init_center = mean_k
            mean, cov, pi, info = m.gmm_fit(mean_k, self.amplitude, self.eps, self.max_iter, seed=self.seed)
            self.iterations_, self.resets_ = info["iters"], info["resets"]
            self.model_params = (mean, cov, pi)
        finally:
            m.free()

    def predict(self, data):
        m = (self._ctx or _context()).mat64(data)
        try:
            return m.gmm_predict(*self.model_params).astype(np.int64)
        finally:
            m.free()


class Spec_Cluster(object):
    """Spec_Cluster of Homework3/hw3/include/spectralClustering.hpp: the (k_neigh, k_clus_estimation) constructor and fit(points) -> labels.
    n_clusters > 0 fixes K instead of the eigengap rule.  After fit: eigenvalues_ (k_clus_estimation values, ascending), K_clusters,
    features_ (n x K_clusters), info_ (solver steps, residual, K-Means passes)."""

    def __init__(self, k_neigh, k_clus_estimation, n_clusters=0, ctx=None):
        self.K_neighbors = int(k_neigh)
        self.K_clusters_estimation = int(k_clus_estimation)
        self.n_clusters = int(n_clusters)
        self.K_clusters = 1
        self.eigenvalues_ = None
        self.features_ = None
        self.info_ = None
        self.status_ = 0
        self._ctx = ctx

    def fit(self, points):
        points = np.ascontiguousarray(points, np.float64)
        m = (self._ctx or _context()).mat64(points)
        try:
            labels, self.features_, self.info_, self.status_ = m.spectral_cluster(self.K_neighbors, self.K_clusters_estimation, self.n_clusters)
        finally:
            m.free()
        self.eigenvalues_ = self.info_["eigenvalues"]
        self.K_clusters = self.info_["K"]
        if self.status_ != 0:
            raise PcrError(f"Spec_Cluster.fit: status {self.status_} (include/pcr.h: PCR_EMPTY_CLUSTER / PCR_SPECTRAL_*)")
        return labels
