"""Homework3 clustering: wall time of one K-Means pass, one EM pass and the seeding — the library against the same iteration written in
torch on the same GPU (cdist / argmin / index_add_, batched logsumexp) and, for the 1 500 x 2 sets, against the numpy formulation on the
host.  Median of 20 calls after 3 warm-ups, each call synchronised.  Prints the table kept in profiles/hw3_clustering.txt.
    python tools/run_hw3_clustering.py [--quick]
"""
import importlib
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcr = importlib.import_module("hands-on-point-cloud-processing_amd")


def med(fn, calls=20, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t), max(t)


def torch_kmeans_step(x, c):
    lab = torch.cdist(x, c).argmin(dim=1)
    s = torch.zeros_like(c).index_add_(0, lab, x)
    cnt = torch.zeros(c.shape[0], dtype=x.dtype, device=x.device).index_add_(0, lab, torch.ones_like(x[:, 0]))
    out = s / cnt[:, None]
    torch.cuda.synchronize()
    return out


def torch_em_step(x, mean, cov, pi):
    L = torch.linalg.cholesky(cov)
    df = x[None, :, :] - mean[:, None, :]                                   # k x n x dim
    y = torch.linalg.solve_triangular(L, df.transpose(1, 2), upper=False)   # k x dim x n
    lp = torch.log(pi)[:, None] - 0.5 * (x.shape[1] * math.log(2 * math.pi) + 2 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1))[:, None] - 0.5 * (y * y).sum(1)
    post = torch.exp(lp - torch.logsumexp(lp, dim=0, keepdim=True))          # k x n
    nk = post.sum(1)
    m2 = (post @ x) / nk[:, None]
    d2 = x[None, :, :] - m2[:, None, :]
    c2 = torch.einsum("kn,kna,knb->kab", post, d2, d2) / nk[:, None, None]
    torch.cuda.synchronize()
    return m2, c2, nk / x.shape[0]


def numpy_kmeans_step(x, c):
    lab = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1).argmin(1)
    return np.array([x[lab == j].mean(0) for j in range(c.shape[0])])


def main():
    quick = "--quick" in sys.argv
    z = np.load(os.path.join(ROOT, "tests", "golden", "hw3_clustering_ref.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))
    key = [k for k in scan.files if scan[k].ndim == 2 and scan[k].shape[1] >= 3][0]
    pts = scan[key][:, :3].astype(np.float64)
    scan100k = np.concatenate([pts + np.array([37.0 * r, -11.0 * r, 0.25 * r]) for r in range(-(-100000 // pts.shape[0]))])[:100000]
    rng = np.random.default_rng(5)
    cases = [("blobs 1500x2", z["data_blobs"], 3), ("moons 1500x2", z["data_moons"], 2), ("scan 100000x3", scan100k, 8), ("scan 100000x3", scan100k, 64)]
    if not quick:
        cases += [("synthetic 1000000x3", rng.normal(size=(1000000, 3)) * 10.0, 8), ("synthetic 1000000x3", rng.normal(size=(1000000, 3)) * 10.0, 64)]
    ctx = pcr.Context(0)
    print(f"{'data':<22}{'k':>4}  {'stage':<13}{'library ms':>12}{'torch ms':>12}{'host ms':>12}{'torch/lib':>11}")
    for name, x, k in cases:
        x = np.ascontiguousarray(x)
        m = ctx.mat64(x)
        c = x[(np.arange(k) * (x.shape[0] // k) + 17) % x.shape[0]].copy()
        xt, ct = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
        lib = med(lambda: m.kmeans_step(c))
        tor = med(lambda: torch_kmeans_step(xt, ct))
        host = med(lambda: numpy_kmeans_step(x, c), 5, 1)[0] if x.shape[0] <= 1500 else float("nan")
        print(f"{name:<22}{k:>4}  {'kmeans pass':<13}{lib[0]:>12.3f}{tor[0]:>12.3f}{host:>12.3f}{tor[0] / lib[0]:>11.2f}")
        fit = med(lambda: m.kmeans_fit(c, 1e-4, 20, want_labels=False), 10, 2)
        iters = m.kmeans_fit(c, 1e-4, 20, want_labels=False)[2]
        print(f"{name:<22}{k:>4}  {'kmeans fit':<13}{fit[0]:>12.3f}{'':>12}{'':>12}   ({iters} passes: {fit[0] / iters:.3f} ms each)")
        dim = x.shape[1]
        cov = np.array([np.cov(x.T) for _ in range(k)])
        pi = np.full(k, 1.0 / k)
        covt, pit = torch.from_numpy(cov).cuda(), torch.from_numpy(pi).cuda()
        lib = med(lambda: m.gmm_em_step(c, cov, pi))
        tor = med(lambda: torch_em_step(xt, ct, covt, pit))
        print(f"{name:<22}{k:>4}  {'EM pass':<13}{lib[0]:>12.3f}{tor[0]:>12.3f}{float('nan'):>12.3f}{tor[0] / lib[0]:>11.2f}")
        if np.abs(x).max() < 200:
            sd = med(lambda: m.kmeanspp_init(min(k, 8), 1.0, seed=3), 10, 2)
            print(f"{name:<22}{min(k, 8):>4}  {'seeding':<13}{sd[0]:>12.3f}")
        m.free()
        del xt, ct
    ctx.close()


if __name__ == "__main__":
    main()
