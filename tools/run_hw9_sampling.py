#!/usr/bin/env python3
"""The two sampling stages of hw9's shipped flow on one MI355X: pcr_voxel_grid_normals_f32 (readBinaryAndVoxelDown's filter) and
pcr_normal_space_sample_f32 (normalSpaceSampling), wall time and the per-pass split (prof_get).
  * voxel grid, leaf 0.3, normal_mode 1: the raw KITTI scan of tests/golden/kat_kitti_q5.npz (100 000 points, pcr_normals_knn_f64
    normals), synth.kitti_like_scan(120 000) and synth.kitti_like_scan(1 000 000) with random unit normals (the cost does not depend on
    the normals' values) — each next to pcr_voxel_filter_f32 (Homework1's filter: xyz only) on the same input and leaf, the yardstick;
    for every input an estimate of the bytes the passes move, against the kernel time;
  * normal-space sampling at hw9's parameters (10^3 bins, 4 000 samples, seed 0) on the voxelled KITTI scan and the voxelled 120 k scan,
    with and without the two gathered clouds, next to one point-to-point ICP iteration on the 4 000 + 4 000 samples.
Wall times are medians of `reps` calls without profiling events; the per-pass times come from one more call with them.
usage: run_hw9_sampling.py [reps]"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
synth = importlib.import_module("hands-on-point-cloud-processing_amd.synth")

VGN = ("vgn_bounds", "vgn_keys", "vgn_sort", "vgn_segments", "vgn_accum", "vgn_finalize")
NSS = ("nss_keys", "nss_sort", "nss_rank", "nss_gather")


def timed(fn, reps):
    fn()
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


def voxel_case(ctx, label, cloud, normals, leaf, reps):
    res = {}

    def run():
        res["o"] = ctx.voxel_grid_normals(cloud, normals, leaf, 1)

    def run_xyz():
        res["x"] = ctx.voxel_grid_normals(cloud, None, leaf, 1)

    def run_hw1():
        res["h"] = ctx.voxel_filter(cloud, leaf)

    med, best = timed(run, reps)
    medx, _ = timed(run_xyz, reps)
    medh, besth = timed(run_hw1, reps)
    p = passes(ctx, run, VGN)
    ph = passes(ctx, run_hw1, ("voxel_centroid",))["voxel_centroid"]
    n, m = len(cloud), len(res["o"][0])
    xyz = cloud.numpy()
    ids = np.floor(xyz * (np.float32(1) / np.float32(leaf)))
    span = (ids.max(1) - ids.min(1) + 1).astype(np.int64)
    bits = int(span[0] * span[1] * span[2]).bit_length()
    sort_passes = (bits + 7) // 8
    # bounds read 12; keys read 12 + write 12; sort (8 + 4) in and out per pass; heads 8 + 4; scan 4 + 4; accum 8 + 4 + 4 + 4 keys / order / flags / rows,
    # 24 gathered coordinates and normals, 4 voxel_of_point; per voxel 56 zeroed + 56 added + 56 read + 28 written
    moved = n * (12 + 24 + 24 * sort_passes + 12 + 8 + 20 + 24 + 4) + m * (3 * 56 + 28)
    kern = sum(p.values())
    print(f"{label}: n {n} -> {m} voxels (leaf {leaf}, {bits}-bit ids, {sort_passes} sort passes)")
    print(f"  pcr_voxel_grid_normals_f32: wall {med:.3f} ms median of {reps} (min {best:.3f}); without normals {medx:.3f}; passes "
          + ", ".join(f"{k} {v:.3f}" for k, v in p.items()) + f" = {kern:.3f} ms of kernels")
    print(f"  pcr_voxel_filter_f32 (Homework1, xyz only, {len(res['h'])} voxels): wall {medh:.3f} ms median (min {besth:.3f}), voxel_centroid {ph:.3f} ms; "
          f"wall ratio new / old {med / medh:.2f}")
    print(f"  about {moved / 1e6:.1f} MB moved by the passes / {kern:.3f} ms = {moved / kern / 1e9:.3f} TB/s ({100 * moved / kern / 1e9 / 8.0:.1f} % of 8 TB/s)")
    return res["o"]


def nss_case(ctx, label, cloud, normals, reps):
    res = {}

    def run():
        res["i"] = ctx.normal_space_sample(normals, (10, 10, 10), 4000, 0)

    def run_gather():
        res["g"] = ctx.normal_space_sample(normals, (10, 10, 10), 4000, 0, gather=(cloud, normals))

    med, best = timed(run, reps)
    medg, bestg = timed(run_gather, reps)
    p = passes(ctx, run_gather, NSS)
    print(f"{label}: n {len(normals)}: pcr_normal_space_sample_f32 wall {med:.3f} ms median of {reps} (min {best:.3f}); with the two gathered clouds "
          f"{medg:.3f} (min {bestg:.3f}); passes " + ", ".join(f"{k} {v:.3f}" for k, v in p.items()))
    _, sc, _ = res["g"]
    T, st = ctx.icp_point2point(sc.clone(), sc, max_corr=1.0, max_iter=200, eps=0.0)
    ctx.icp_point2point(sc.clone(), sc, max_corr=1.0, max_iter=200, eps=0.0)
    t0 = time.perf_counter()
    T, st = ctx.icp_point2point(sc.clone(), sc, max_corr=1.0, max_iter=200, eps=0.0)
    dt = (time.perf_counter() - t0) * 1e3
    print(f"  one ICP call on the {len(sc)} + {len(sc)} samples: {st['iters_run']} iterations in {dt:.3f} ms wall = {1e3 * dt / max(st['iters_run'], 1):.1f} us / iteration")


def unit_normals(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
    ctx = pcr.Context(0)
    print(f"device = {ctx.device_info()}")
    raw = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))["db_f32"], np.float32)
    c = ctx.cloud(raw, 1)
    nc = ctx.cloud(ctx.normals(c, 10, 1.2).astype(np.float32), 1)
    oc, on, _, _ = voxel_case(ctx, "kitti q5 raw", c, nc, 0.3, reps)
    nss_case(ctx, "kitti q5 voxelled", oc, on, reps)
    for n in (120_000, 1_000_000):
        sc = ctx.cloud(synth.kitti_like_scan(n))
        sn = ctx.cloud(unit_normals(n, 1), 1)
        oc, on, _, _ = voxel_case(ctx, f"synth {n}", sc, sn, 0.3, reps if n < 500_000 else max(5, reps // 2))
        if n == 120_000:
            nss_case(ctx, f"synth {n} voxelled", oc, on, reps)
    ctx.close()


if __name__ == "__main__":
    main()
