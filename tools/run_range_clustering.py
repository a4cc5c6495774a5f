#!/usr/bin/env python3
"""Homework4's range-image clustering on one MI355X: pcr_range_cluster_f32 and its stages (create, label, assign) at 0.7 deg and 0.2 deg
(theta 30, nn_mode 7) on the three KITTI foregrounds of tests/golden/range_hw4_ref.npz (every 5th / 6th point of the scans' foreground) and on
the foreground (z > -1.4) of synth.kitti_like_scan(120 000), next to pcr_dbscan_f32(0.8, 20) on the same clouds in the same session and to
the Python loops of foreground_clustering_range.py on the host (the restatement of tests/test_range_clustering.py, once per cloud, 0.7 deg).
Wall time per call: median of 20 after 3 warm-ups, every call synchronised (each returns host arrays).  Writes profiles/range_clustering.txt.
usage: run_range_clustering.py [reps]"""
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
PASSES = ("ri_project", "ri_crop", "ri_union", "ri_label", "ri_assign")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def case(ctx, name, pts, reps, host_loops):
    cloud = ctx.cloud(np.ascontiguousarray(pts, np.float32), 1)
    say(f"{name}: {pts.shape[0]} points")
    for res in (0.7, 0.2):
        out = {}

        def whole():
            out["r"] = ctx.range_cluster(cloud, res, 30.0, 7)

        def create():
            out["ri"] = ctx.range_image(cloud, res)

        med, best = timed(whole, reps)
        _, nc, st = out["r"]
        say(f"  {res} deg: image {st['rows']} x {st['cols']} of {st['full_pixels']} pixels, {nc} clusters, {st['dropped']} points dropped")
        say(f"    pcr_range_cluster_f32     {med:8.3f} ms median of {reps} (min {best:.3f})")
        create()
        ri = out["ri"]
        m_create = timed(lambda: ctx.range_image(cloud, res).free(), reps)
        m_label = timed(lambda: ri.label(res, 30.0, 7), reps)
        m_assign = timed(ri.assign, reps)
        say(f"    stages: create + destroy {m_create[0]:.3f}, label {m_label[0]:.3f}, assign {m_assign[0]:.3f} ms")
        ctx.tune("prof", 2)
        ctx.prof_reset()
        whole()
        say("    kernels (ms, event pairs): " + ", ".join(f"{k} {ctx.prof_get(k)[1]:.3f}" for k in PASSES))
        ctx.tune("prof", 0)
        if host_loops and res == 0.7:
            import test_range_clustering as t
            img = ri.image()
            t0 = time.perf_counter()
            t.label_loops(img, res, 30.0, 7)
            say(f"    the reference's Python loops on the host (range_image_labeling alone): {(time.perf_counter() - t0) * 1e3:.0f} ms")
        ri.free()
    med, best = timed(lambda: ctx.dbscan(cloud, 0.8, 20), reps)
    say(f"  pcr_dbscan_f32(0.8, 20)       {med:8.3f} ms median of {reps} (min {best:.3f}), {ctx.dbscan(cloud, 0.8, 20)[3]} clusters")
    cloud.free()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ctx = pcr.Context(0)
    say(f"device = {ctx.device_info()}")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "range_hw4_ref.npz"))
    for name in (str(s) for s in fx["cases"]):
        if name + "_points" in fx.files:
            case(ctx, name, fx[name + "_points"], reps, True)
    scan = synth.kitti_like_scan(120_000)
    case(ctx, "synth 120k foreground", np.ascontiguousarray(scan[:, scan[2] > -1.4].T), reps, True)
    ctx.close()
    with open(os.path.join(ROOT, "profiles", "range_clustering.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
