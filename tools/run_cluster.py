#!/usr/bin/env python3
"""Homework4 foreground stage on one MI355X: pcr_dbscan_f32 at (0.8, 20) on the foreground (z > -1.4) of synth.kitti_like_scan(120 000)
with the per-pass times (prof_get), the same on a 10 M scan, and pcr_statistical_outlier_f32 at (20, 2.7) on the 120 k scan.

The 10 M foreground is ~83 times denser than the 120 k one: at eps = 0.8 its mean neighbourhood would be ~2 x 10^5 points, so it runs at
eps = 0.8 sqrt(120 000 / 10 000 000), which keeps the neighbourhood of the 120 k case (the scaling in n at a fixed neighbourhood).
Wall times are medians of `reps` calls without profiling events; the per-pass times come from one more call with them.
usage: run_cluster.py [reps]"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
synth = importlib.import_module("hands-on-point-cloud-processing_amd.synth")

DB_PASSES = ("dbscan_grid", "dbscan_count", "dbscan_union", "dbscan_border", "dbscan_label")
SOR_PASSES = ("sor_knn", "sor_stats", "sor_gather")


def timed(ctx, fn, reps):
    fn()                                                            # warm-up (code objects, scratch)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def passes(ctx, fn, names):
    ctx.tune("prof", 2)
    ctx.prof_reset()
    fn()
    out = {k: ctx.prof_get(k)[1] for k in names}
    ctx.tune("prof", 0)
    return out


def dbscan_case(ctx, label, scan, eps, min_points, reps):
    fg = np.ascontiguousarray(scan[:, scan[2] > -1.4])
    cloud = ctx.cloud(fg)
    res = {}

    def run():
        res["out"] = ctx.dbscan(cloud, eps, min_points)

    med, best = timed(ctx, run, reps)
    p = passes(ctx, run, DB_PASSES)
    labels, core, counts, nc = res["out"]
    print(f"{label}: foreground {fg.shape[1]} points, eps {eps:.4f}, min_points {min_points}: {nc} clusters, {int(core.sum())} core, "
          f"{int((labels >= 0).sum() - core.sum())} border, {int((labels < 0).sum())} noise; mean |N(p)| {counts.mean():.0f}, max {counts.max()}")
    print(f"  pcr_dbscan_f32 wall {med:.3f} ms median of {reps} (min {best:.3f}); scratch {38 * fg.shape[1] / 2**20:.1f} MiB + grid")
    print("  passes (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in p.items()))
    cloud.free()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = pcr.Context(0)
    print(f"device = {ctx.device_info()}")
    scan = synth.kitti_like_scan(120_000)
    dbscan_case(ctx, "synth 120k", scan, 0.8, 20, reps)

    xyz = np.ascontiguousarray(scan.T)
    crop = np.ascontiguousarray(xyz[(xyz[:, 1] < 30) & (xyz[:, 1] > -15)])
    cloud = ctx.cloud(crop, 1)
    res = {}

    def run():
        res["out"] = ctx.statistical_outlier(cloud, 20, 2.7)
        res["out"][3].free()

    med, best = timed(ctx, run, reps)
    p = passes(ctx, run, SOR_PASSES)
    keep, avg, st, _ = res["out"]
    print(f"synth 120k after the y crop: {crop.shape[0]} points, SOR (20, 2.7): kept {int(keep.sum())}, mean {st[0]:.6f}, std {st[1]:.6f}, thr {st[2]:.6f}")
    print(f"  pcr_statistical_outlier_f32 wall {med:.3f} ms median of {reps} (min {best:.3f})")
    print("  passes (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in p.items()))
    cloud.free()

    t0 = time.perf_counter()
    big = synth.kitti_like_scan(10_000_000)
    print(f"(10 M scan generated on the host in {time.perf_counter() - t0:.1f} s)")
    dbscan_case(ctx, "synth 10M", big, 0.8 * (120_000 / 10_000_000) ** 0.5, 20, max(3, reps // 3))
    ctx.close()


if __name__ == "__main__":
    main()
