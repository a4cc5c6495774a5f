#!/usr/bin/env python3
"""Measures pcr_points_in_boxes_f64 (the operator under HomeworkFinal's dataset build) on one MI355X: the kernel time of its passes from the
library's HIP-event profile (tune prof = 2), the bytes each pass moves against the HBM rate, the same membership test as a plain torch f64
expression on the same GPU (data resident, synchronised), and the reference's numpy form on the CPU.  The record is profiles/dataset_build.txt.

Shapes: one frame of 120 000 points x 16 boxes, and 64 such frames in ONE call (64 segments, 16 boxes each).  The frames are the synthetic scan
shifted by a drawn offset; the boxes are car-sized, centred on seeded scan points above the ground, with a drawn yaw.

    python tools/run_dataset_build.py [--reps 10] [--warmup 2] [--frames 64] [--no-torch]
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
synth = importlib.import_module("hands-on-point-cloud-processing_amd.synth")

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12      # bytes / s: a float4 copy on this part, and the data sheet
N, NBOX = 120000, 16
TILE_DEFAULT = 512                            # PIB_TILE_DEFAULT of csrc/boxes.hip


def draw_boxes(points, rng, k=NBOX):
    cand = np.flatnonzero((points[:, 2] > -1.3) & (points[:, 2] < 0.5) & (np.linalg.norm(points[:, :2], axis=1) < 45))
    out = np.zeros((k, 15))
    for b, i in enumerate(rng.choice(cand, k, replace=False)):
        a = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        out[b] = np.concatenate([[points[i, 0], points[i, 1], -1.73 + 0.75], R.reshape(9), [1.15 * 3.9, 1.25 * 1.6, 1.5]])
    return out


def numpy_form(points, boxes):
    """get_point_indices_within_bounding_box per box, elementwise f64 (the rule of include/pcr.h)"""
    p = points.astype(np.float64)
    rows = []
    for b in boxes:
        c, R, e = b[0:3], b[3:12].reshape(3, 3), b[12:15]
        d0, d1, d2 = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        m = np.ones(p.shape[0], bool)
        for a in range(3):
            m &= np.abs((d0 * R[0, a] + d1 * R[1, a]) + d2 * R[2, a]) <= e[a] * 0.5
        rows.append(np.flatnonzero(m))
    return rows


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    scan = np.ascontiguousarray(synth.kitti_like_scan(N).T, np.float32)
    boxes1 = draw_boxes(scan, rng)
    torch = None
    if not args.no_torch:
        import torch
        torch.zeros(1).cuda()                      # torch opens the device before the library's context does
    ctx = pcr.Context(0)
    print(f"device: {ctx.device_info()}")
    print(f"shapes: {N} points x {NBOX} boxes per frame; pib_tile default ({TILE_DEFAULT}); times in ms, median of {args.reps} after {args.warmup} warm-up calls")
    for frames in (1, args.frames):
        shifts = np.zeros((frames, 3), np.float32)
        shifts[1:, :2] = rng.uniform(-1, 1, (frames - 1, 2)).astype(np.float32)
        pts = np.concatenate([scan + s for s in shifts])
        boxes = np.concatenate([boxes1 + np.concatenate([s.astype(np.float64), np.zeros(12)]) for s in shifts])
        seg = (np.arange(frames + 1) * N).astype(np.uint32)
        bseg = (np.arange(frames + 1) * NBOX).astype(np.uint32)
        cloud = ctx.cloud(pts, pcr.PCR_AOS3)
        rp, idx, hits = ctx.points_in_boxes(cloud, seg, boxes, bseg)
        total = int(rp[-1])
        wall, wall_min = median(lambda: ctx.points_in_boxes(cloud, seg, boxes, bseg), args.reps, args.warmup)
        ctx.tune("prof", 2)
        ctx.prof_reset()
        for _ in range(args.reps):
            ctx.points_in_boxes(cloud, seg, boxes, bseg)
        ctx.tune("prof", 0)
        # Context.points_in_boxes is two C calls (count, then count + fill): 2 pib_count and 2 pib_scan per pib_fill
        k = {name: float(np.median(ctx.prof_get_each(name))) for name in ("pib_count", "pib_scan", "pib_fill")}
        n = pts.shape[0]
        tiles = frames * -(-N // TILE_DEFAULT)
        E = tiles * NBOX
        b_count = 12 * n + 4 * n + 4 * E + 120 * NBOX * frames          # the coordinates, hits, the (tile, box) counts, the boxes once per frame
        b_fill = 12 * n + 8 * E + 4 * total + 120 * NBOX * frames       # the coordinates, the offsets, the index lists
        print(f"\n== {frames} frame(s): {n} points, {NBOX * frames} boxes, {total} memberships, {tiles} tiles")
        print(f"  library, one C call that fills (count + scan + fill kernels): {k['pib_count'] + k['pib_scan'] + k['pib_fill']:.4f} ms  "
              f"(pib_count {k['pib_count']:.4f}, pib_scan {k['pib_scan']:.4f} (4 launches), pib_fill {k['pib_fill']:.4f})")
        for name, b, t in (("pib_count", b_count, k["pib_count"]), ("pib_fill", b_fill, k["pib_fill"])):
            print(f"  {name}: {b / 1e6:.2f} MB moved -> {b / (t * 1e-3) / 1e12:.3f} TB/s = {100 * b / (t * 1e-3) / HBM_MEASURED:.1f} % of the measured HBM rate "
                  f"({HBM_MEASURED / 1e12:.2f} TB/s; spec {HBM_SPEC / 1e12:.1f}); at that rate the pass would take {b / HBM_MEASURED * 1e3:.4f} ms")
        print(f"  library, Context.points_in_boxes wall (host arrays in and out, counting call + filling call): {wall:.3f} ms (min {wall_min:.3f})")
        for tile in (64, 256, 512, 1024, 2048):                                  # the same call under other tile sizes (the same lists)
            ctx.tune("pib_tile", tile)
            got = ctx.points_in_boxes(cloud, seg, boxes, bseg)
            ctx.tune("prof", 2)
            ctx.prof_reset()
            for _ in range(args.reps):
                ctx.points_in_boxes(cloud, seg, boxes, bseg)
            ctx.tune("prof", 0)
            kt = [float(np.median(ctx.prof_get_each(name))) for name in ("pib_count", "pib_scan", "pib_fill")]
            print(f"    pib_tile {tile:5d}: count {kt[0]:.4f} + scan {kt[1]:.4f} + fill {kt[2]:.4f} = {sum(kt):.4f} ms; same lists: {np.array_equal(got[1], idx)}", flush=True)
        ctx.tune("pib_tile", 0)
        if torch is not None:
            P = torch.from_numpy(pts.astype(np.float64)).cuda()
            B = torch.from_numpy(boxes).cuda()

            def torch_form():
                out = []
                for f in range(frames):
                    p = P[f * N:(f + 1) * N]
                    bx = B[f * NBOX:(f + 1) * NBOX]
                    d = p[None, :, :] - bx[:, None, 0:3]
                    R = bx[:, 3:12].reshape(NBOX, 3, 3)
                    t = (d[:, :, 0:1] * R[:, None, 0, :] + d[:, :, 1:2] * R[:, None, 1, :]) + d[:, :, 2:3] * R[:, None, 2, :]
                    out.append(((t.abs() <= bx[:, None, 12:15] * 0.5).all(-1)).nonzero())
                torch.cuda.synchronize()
                return out
            got = torch_form()
            same = np.array_equal(np.concatenate([g[:, 1].cpu().numpy() for g in got]), idx)
            tt, tt_min = median(torch_form, args.reps, args.warmup)
            print(f"  torch f64 expression on the same GPU (points and boxes resident, one nonzero per frame, synchronised): {tt:.3f} ms (min {tt_min:.3f}); "
                  f"same lists: {same}")
            print(f"    ratio torch / library kernels: {tt / (k['pib_count'] + k['pib_scan'] + k['pib_fill']):.1f} x")
            del P, B
        a = time.perf_counter()
        rows = []
        for f in range(frames):
            rows += numpy_form(pts[f * N:(f + 1) * N], boxes[f * NBOX:(f + 1) * NBOX])
        tn = (time.perf_counter() - a) * 1e3
        print(f"  numpy form on the CPU (one pass, elementwise f64 per box): {tn:.1f} ms; same lists: {np.array_equal(np.concatenate(rows), idx)}")
        print(f"    ratio numpy / library wall: {tn / wall:.1f} x")
        cloud.free()
    ctx.close()


if __name__ == "__main__":
    main()
