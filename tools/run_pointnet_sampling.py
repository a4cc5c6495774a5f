#!/usr/bin/env python3
"""Measures the PointNet++ sampling / grouping operators (pcr_fps_f32, pcr_ball_query_f32, pcr_objects_from_labels_f32) against the
reference's own formulation — a loop of torch tensor operations, one iteration per pick (HomeworkFinal/models/pointnet_util.py:66-116) —
restated here from the contract in include/pcr.h and run on the same GPU under torch.  The record is profiles/pointnet_sampling.txt.

Protocol: wall time of the whole call, host copies included on both sides (the library takes and returns host arrays; the comparator
uploads its input and downloads its result), median of --reps calls (default 20) after --warmup calls.  The kernel-only figures
(microseconds per pick) come from the library's HIP-event profile (tune prof = 2) in a separate pass.

    python tools/run_pointnet_sampling.py [--reps 20] [--warmup 3] [--skip-scan]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
pn = importlib.import_module("hands-on-point-cloud-processing_amd.pointnet")


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t), max(t)


def torch_fps(torch, xyz_host, npoint, start_host):
    """the reference's formulation: per pick gather the centre, subtract, square, sum, compare, masked update, argmax"""
    xyz = torch.from_numpy(xyz_host).cuda()
    B, N, _ = xyz.shape
    out = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    dist = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
    far = torch.from_numpy(np.asarray(start_host, np.int64)).cuda()
    rows = torch.arange(B, device=xyz.device)
    for i in range(npoint):
        out[:, i] = far
        c = xyz[rows, far, :].view(B, 1, 3)
        d = torch.sum((xyz - c) ** 2, -1)
        m = d < dist
        dist[m] = d[m]
        far = torch.max(dist, -1)[1]
    return out.cpu().numpy()


def torch_ball(torch, radius, nsample, xyz_host, new_xyz_host):
    xyz, q = torch.from_numpy(xyz_host).cuda(), torch.from_numpy(new_xyz_host).cuda()
    B, N, _ = xyz.shape
    S = q.shape[1]
    idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    d = -2 * torch.matmul(q, xyz.permute(0, 2, 1)) + torch.sum(q ** 2, -1).view(B, S, 1) + torch.sum(xyz ** 2, -1).view(B, 1, N)
    idx[d > radius ** 2] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, 0].view(B, S, 1).repeat(1, 1, nsample)
    m = idx == N
    idx[m] = first[m]
    return idx.cpu().numpy()


def report(name, lib, cmp_):
    print(f"{name:<58s} library {lib[0]:9.3f} ms (min {lib[1]:.3f}, max {lib[2]:.3f})   torch loop {cmp_[0]:9.3f} ms (min {cmp_[1]:.3f}, max {cmp_[2]:.3f})   "
          f"ratio {cmp_[0] / lib[0]:7.1f} x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-scan", action="store_true", help="leave out the 100 000-point shape (its comparator takes seconds)")
    a = ap.parse_args()
    import torch
    scan = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))["db_f32"][:, :3], np.float32)
    ctx = pcr.Context(0)
    print(f"device {ctx.device_info()['arch']}, torch {torch.__version__}; wall, median of {a.reps} calls after {a.warmup} warm-up calls, host copies included")
    rng = np.random.default_rng(0)

    def lib_fps(x, S, st, mode=0):
        return pn.farthest_point_sample(x, S, st, ctx=ctx, mode=mode)

    def layer_pair(x, tag):
        """the model's two set-abstraction layers on a batch x [B, 256, 3]"""
        B = x.shape[0]
        st = rng.integers(0, x.shape[1], B)
        f1 = lib_fps(x, 64, st)
        assert np.array_equal(f1, torch_fps(torch, x, 64, st)), "the comparator and the library disagree"
        c1 = pn.index_points(x, f1)
        report(f"{tag} FPS B={B} 256 -> 64", median_ms(lambda: lib_fps(x, 64, st), a.reps, a.warmup), median_ms(lambda: torch_fps(torch, x, 64, st), a.reps, a.warmup))
        report(f"{tag} ball r 0.2 k 8, B={B} S=64 N=256", median_ms(lambda: pn.query_ball_point(0.2, 8, x, c1, ctx=ctx), a.reps, a.warmup),
               median_ms(lambda: torch_ball(torch, 0.2, 8, x, c1), a.reps, a.warmup))
        st2 = rng.integers(0, 64, B)
        report(f"{tag} FPS B={B} 64 -> 32", median_ms(lambda: lib_fps(c1, 32, st2), a.reps, a.warmup), median_ms(lambda: torch_fps(torch, c1, 32, st2), a.reps, a.warmup))
        c2 = pn.index_points(c1, lib_fps(c1, 32, st2))
        report(f"{tag} ball r 0.4 k 16, B={B} S=32 N=64", median_ms(lambda: pn.query_ball_point(0.4, 16, c1, c2, ctx=ctx), a.reps, a.warmup),
               median_ms(lambda: torch_ball(torch, 0.4, 16, c1, c2), a.reps, a.warmup))
        report(f"{tag} sample_and_group(64, 0.2, 8) B={B} (one upload)", median_ms(lambda: pn.sample_and_group(64, 0.2, 8, x, None, start=st, ctx=ctx), a.reps, a.warmup),
               median_ms(lambda: (torch_ball(torch, 0.2, 8, x, pn.index_points(x, torch_fps(torch, x, 64, st)))), a.reps, a.warmup))

    # 1. the model's batch: 128 objects of 256 points (2 m cubes of the real scan, centred)
    objs = []
    while len(objs) < 128:
        c = scan[rng.integers(len(scan))]
        m = np.flatnonzero((np.abs(scan - c) < 1.0).all(1))
        if m.size >= 256:
            o = scan[m[:256]].astype(np.float64)
            objs.append((o - o.mean(0)).astype(np.float32))
    layer_pair(np.stack(objs), "model batch:")
    # 2. one real scan's objects
    t = median_ms(lambda: pn.classify_foreground_objects(scan, ctx=ctx), 5, 1)
    objects, codes, res = pn.classify_foreground_objects(scan, ctx=ctx)
    fg = np.ascontiguousarray(res["points"][res["foreground_idx"]], np.float32)
    cloud = ctx.cloud(fg, pcr.PCR_AOS3)
    t2 = median_ms(lambda: ctx.objects_from_labels(cloud, res["labels"], res["n_clusters"], 256, res["ground_z"]), a.reps, a.warmup)
    cloud.free()
    print(f"real scan: {len(fg)} foreground points, {res['n_clusters']} clusters, {len(objects)} objects; classify_foreground_objects {t[0]:.1f} ms (median of 5), "
          f"of which objects_from_labels {t2[0]:.3f} ms (min {t2[1]:.3f}, max {t2[2]:.3f})")
    if len(objects) >= 2:
        layer_pair(np.ascontiguousarray(objects), "scan objects:")
    # 3. a whole scan as one segment
    if not a.skip_scan:
        x = scan[None, :100000].copy()
        st = np.array([12345])
        got = lib_fps(x, 4096, st)
        assert np.array_equal(got, torch_fps(torch, x, 4096, st)), "the comparator and the library disagree"
        report("scan: FPS B=1 100 000 -> 4 096 (one launch per pick)", median_ms(lambda: lib_fps(x, 4096, st), a.reps, a.warmup), median_ms(lambda: torch_fps(torch, x, 4096, st), a.reps, 1))
    # 4. kernel-only figures from the HIP-event profile
    ctx.tune("prof", 2)
    x = np.stack(objs)
    for mode, label in ((0, "f32"), (1, "f64")):
        ctx.prof_reset()
        for _ in range(a.reps):
            lib_fps(x, 64, np.zeros(128, np.int64), mode)
        n, ms = ctx.prof_get("fps_small")
        print(f"kernel fps_small ({label} mode) B=128 256 -> 64: {1e3 * ms / n:.2f} us per launch, {1e3 * ms / n / 63:.3f} us per pick (one wave per segment)")
    if not a.skip_scan:
        x = scan[None, :100000].copy()
        ctx.prof_reset()
        for _ in range(3):
            lib_fps(x, 4096, np.array([12345]))
        n, ms = ctx.prof_get("fps_large")
        per_step = 1e3 * ms / n / 4096
        d = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
        e = torch.empty_like(d)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e.copy_(d)
        ev[0].record()
        for _ in range(10):
            e.copy_(d)
        ev[1].record()
        torch.cuda.synchronize()
        bw = 10 * 2 * d.numel() * 4 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9
        floor = 100000 * 16 / (bw * 1e9) * 1e6
        print(f"kernel fps_large 100 000 -> 4 096: {per_step:.2f} us per pick including the launch gap (event pair around the 4 096 launches); the step's compulsory 16 B / point "
              f"at the measured copy bandwidth of {bw:.0f} GB/s would be {floor:.2f} us")
    ctx.close()


if __name__ == "__main__":
    main()
