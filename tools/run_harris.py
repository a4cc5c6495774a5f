#!/usr/bin/env python3
"""Harris3D keypoints (pcr_harris3d_f32) on one MI355X, with the per-pass split (prof_get) and |N| statistics:
  * the real KITTI scan of tests/golden/kat_kitti_q5.npz voxelled at 0.3 (hw9's voxel_size), pcr_normals_knn_f64 normals, at radius 0.6
    (hw9: voxel_size * 2) and 1.2, threshold 1e-8, nms on;
  * synth.kitti_like_scan(120 000) at radius 1.2: the stress case (dense rings near the sensor);
  * each harris_lanes value on every input;
  * fpfh_spfh of pcr_fpfh33_f32 on the same input at the same lane count: it walks the same neighbourhoods and does more per pair;
  * the numpy restatement of tests/test_harris3d.py on the same inputs (one host thread), as a CPU reference point.
Wall times are medians of `reps` calls without profiling events; the per-pass times come from one more call with them.
usage: run_harris.py [reps] [--no-numpy]"""
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

PASSES = ("harris_grid_build", "harris_response", "harris_nms")


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


def case(ctx, label, cloud, nrm, radius, reps, lanes):
    res = {}

    def run():
        res["out"] = ctx.harris3d(cloud, nrm, radius, 1e-8)

    def run_fpfh():
        ctx.fpfh33(cloud, nrm, radius)

    for G in lanes:
        ctx.tune("harris_lanes", G)
        ctx.tune("fpfh_lanes", G)
        med, best = timed(run, reps)
        run_fpfh()
        p = passes(ctx, run, PASSES)
        sp = passes(ctx, run_fpfh, ("fpfh_spfh",))["fpfh_spfh"]
        idx, resp, cnt = res["out"]
        print(f"{label} harris_lanes={G}: n {len(cloud)}, {idx.size} keypoints: wall {med:.3f} ms median of {reps} (min {best:.3f}); "
              + ", ".join(f"{k} {v:.3f}" for k, v in p.items()) + f"; fpfh_spfh at fpfh_lanes={G}: {sp:.3f}")
    ctx.tune("harris_lanes", 0)
    ctx.tune("fpfh_lanes", 0)
    idx, resp, cnt = res["out"]
    early = ~np.isfinite(resp) | (resp < np.float32(1e-8))
    print(f"  |N(i)| min {cnt.min()} median {int(np.median(cnt))} mean {cnt.mean():.1f} p99 {int(np.percentile(cnt, 99))} max {cnt.max()}; "
          f"{early.mean():.4f} of the points fail the threshold before the suppression walk")


def numpy_ref(label, xyz, nrm, radius):
    T = importlib.import_module("test_harris3d")
    t0 = time.perf_counter()
    key, _, _ = T.harris_numpy(xyz, nrm, radius, 1e-8)
    print(f"{label} numpy restatement (host, one thread): {(time.perf_counter() - t0) * 1e3:.0f} ms, {int(key.sum())} keypoints")


def numpy_ref_sampled(label, xyz, nrm, radius, k=1000):
    """the stress case holds ~3 x 10^8 (point, neighbour) pairs: too many for the restatement's flat arrays, so it runs the moments of k
    sampled centre points and scales by n / k (the suppression pass walks the same pairs once more)"""
    T = importlib.import_module("test_harris3d")
    rng = np.random.default_rng(0)
    pick = np.sort(rng.choice(xyz.shape[0], k, replace=False))
    t0 = time.perf_counter()
    r2 = np.float32(np.float64(radius) ** 2)
    tree = T.cKDTree(xyz.astype(np.float64))
    lists = tree.query_ball_point(xyz[pick].astype(np.float64), r=radius * (1 + 1e-5))
    lens = np.array([len(l) for l in lists], np.int64)
    qi = np.repeat(np.arange(k), lens)
    j = np.concatenate([np.asarray(l, np.int64) for l in lists])
    d = xyz[j] - xyz[pick][qi]
    keep = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < r2
    c, _, _ = T.moments(nrm, qi[keep], j[keep], k)
    T.response_f32(c)
    dt = time.perf_counter() - t0
    print(f"{label} numpy restatement (host, one thread), responses of {k} sampled points: {dt * 1e3:.0f} ms for {int(keep.sum())} pairs "
          f"-> about {dt * xyz.shape[0] / k:.0f} s for all {xyz.shape[0]} points")


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
    print(f"kitti q5: {raw.shape[0]} points -> {xyz.shape[0]} after the 0.3 voxel filter; normals pcr_normals_knn_f64(10, 1.2)")
    for radius in (0.6, 1.2):
        case(ctx, f"kitti voxel 0.3, r {radius}", c, nrm, radius, reps, all_lanes)
        if with_numpy:
            numpy_ref(f"kitti voxel 0.3, r {radius}:", xyz, nrm, radius)

    scan = synth.kitti_like_scan(120_000)
    sc = ctx.cloud(scan)
    snrm = ctx.normals(sc, 10, 1.2).astype(np.float32)
    case(ctx, "synth 120k, r 1.2", sc, snrm, 1.2, max(3, reps // 4), all_lanes)
    if with_numpy:
        numpy_ref_sampled("synth 120k, r 1.2:", np.ascontiguousarray(scan.T), snrm, 1.2)
    ctx.close()


if __name__ == "__main__":
    main()
