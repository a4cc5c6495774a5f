#!/usr/bin/env python3
"""FPFH33 descriptors (pcr_fpfh33_f32) on one MI355X, with the per-pass split (prof_get) and |N| statistics:
  * the real KITTI scan of tests/golden/kat_kitti_q5.npz voxelled at 0.3 (hw9's voxel_size), pcr_normals_knn_f64 normals, radius 1.2
    (voxel_size * 4): with hw9's ISS keypoints (0.9 / 0.9, gamma 0.52 / 0.52, min 6) and with every point as a keypoint;
  * synth.kitti_like_scan(120 000) at radius 1.2, every point a keypoint: the stress case (dense rings near the sensor);
  * each fpfh_lanes value on both all-point cases;
  * the numpy restatement of tests/test_fpfh.py on the same inputs (one host thread), as a CPU reference point.
Wall times are medians of `reps` calls without profiling events; the per-pass times come from one more call with them.
usage: run_fpfh.py [reps] [--no-numpy]"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
synth = importlib.import_module("hands-on-point-cloud-processing_amd.synth")

PASSES = ("fpfh_grid_build", "fpfh_spfh", "fpfh_weight")


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def passes(ctx, fn):
    ctx.tune("prof", 2)
    ctx.prof_reset()
    fn()
    out = {k: ctx.prof_get(k)[1] for k in PASSES}
    ctx.tune("prof", 0)
    return out


def case(ctx, label, cloud, nrm, radius, kp, reps, lanes=(16,)):
    res = {}

    def run():
        res["out"] = ctx.fpfh33(cloud, nrm, radius, keypoints=kp)

    for G in lanes:
        ctx.tune("fpfh_lanes", G)
        med, best = timed(run, reps)
        p = passes(ctx, run)
        fp, cnt = res["out"]
        print(f"{label} fpfh_lanes={G}: n {len(cloud)}, m {fp.shape[0]}: wall {med:.3f} ms median of {reps} (min {best:.3f}); "
              + ", ".join(f"{k} {v:.3f}" for k, v in p.items()))
    ctx.tune("fpfh_lanes", 0)
    fp, cnt = res["out"]
    print(f"  |N(q)| min {cnt.min()} median {int(np.median(cnt))} mean {cnt.mean():.1f} p99 {int(np.percentile(cnt, 99))} max {cnt.max()}; "
          f"NaN rows {int(np.isnan(fp).any(1).sum())}")


def numpy_ref(label, xyz, nrm, radius):
    T = importlib.import_module("test_fpfh")
    t0 = time.perf_counter()
    sp, _, _ = T.spfh_numpy(xyz, nrm, radius)
    t1 = time.perf_counter()
    T.fpfh_numpy(xyz, sp, radius)
    t2 = time.perf_counter()
    print(f"{label} numpy restatement (host, one thread): SPFH {(t1 - t0) * 1e3:.0f} ms + FPFH {(t2 - t1) * 1e3:.0f} ms")


def numpy_ref_sampled(label, xyz, nrm, radius, k=1000):
    """the stress case holds ~3 x 10^8 (point, neighbour) pairs: too many for the restatement's flat arrays, so it runs the SPFH
    pair features of k sampled centre points and scales by n / k (the FPFH pass costs about as much again)"""
    T = importlib.import_module("test_fpfh")
    rng = np.random.default_rng(0)
    pick = rng.choice(xyz.shape[0], k, replace=False)
    t0 = time.perf_counter()
    qi, j, _ = T.neighbours(xyz, xyz[pick], radius)
    p = pick[qi]
    other = p != j
    T.pair_features(xyz[p[other]], nrm[p[other]], xyz[j[other]], nrm[j[other]])
    dt = time.perf_counter() - t0
    print(f"{label} numpy restatement (host, one thread), SPFH of {k} sampled points: {dt * 1e3:.0f} ms for {qi.size} pairs "
          f"-> about {dt * xyz.shape[0] / k:.0f} s for the SPFH of all {xyz.shape[0]} points")


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
    with_numpy = "--no-numpy" not in sys.argv
    all_lanes = (1, 2, 4, 8, 16, 32)
    ctx = pcr.Context(0)
    print(f"device = {ctx.device_info()}")
    raw = np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))["db_f32"]
    c = ctx.voxel_filter(ctx.cloud(np.ascontiguousarray(raw, np.float32), 1), 0.3)
    xyz = np.ascontiguousarray(c.numpy().T)
    nrm = ctx.normals(c, 10, 1.2).astype(np.float32)
    idx, _, _ = ctx.iss_keypoints(c, 0.9, 0.9, 0.52, 0.52, 6, False)
    print(f"kitti q5: {raw.shape[0]} points -> {xyz.shape[0]} after the 0.3 voxel filter, {idx.size} ISS keypoints")
    case(ctx, "kitti voxel 0.3, r 1.2, ISS keypoints", c, nrm, 1.2, xyz[idx], reps)
    case(ctx, "kitti voxel 0.3, r 1.2, all points", c, nrm, 1.2, None, reps, all_lanes)
    if with_numpy:
        numpy_ref("kitti voxel 0.3, r 1.2, all points:", xyz, nrm, 1.2)

    scan = synth.kitti_like_scan(120_000)
    sc = ctx.cloud(scan)
    snrm = ctx.normals(sc, 10, 1.2).astype(np.float32)
    case(ctx, "synth 120k, r 1.2, all points", sc, snrm, 1.2, None, max(3, reps // 4), all_lanes)
    if with_numpy:
        numpy_ref_sampled("synth 120k, r 1.2, all points:", np.ascontiguousarray(scan.T), snrm, 1.2)
    ctx.close()


if __name__ == "__main__":
    main()
