"""Homework3's clustering classes on the GPU: K_Means (Homework3/hw3/sript/KMeans.py) and GMM (Homework3/hw3/sript/GMM.py with the working
`posterior` of Homework3/nano_vs_my/sript/GMM.py), with the reference's attributes and methods, behind the C ABI of include/pcr.h
(csrc/mixture.hip).  compare_cluster.py runs with its two import lines changed.

The reference draws its initial points unseeded.  Here the draws are keyed by `seed` (SplitMix64, include/pcr.h), or the initial indices
are given outright with `init_idx`.  There is no CPU fall-back: a missing library or GPU is an error.
"""
from __future__ import annotations

import numpy as np

from . import PCR_KMEANS_PY, Context

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
