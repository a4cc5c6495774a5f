#!/usr/bin/env python3
"""Measures the Homework6 evaluator (csrc/kitti_eval.hip) on one MI355X and writes the record, profiles/hw6_eval.txt.

The reference's full result set (3 769 PointRCNN files) is not shipped with the tests, so the input is the fixture tests/golden/hw6_eval_ref.npz
(200 frames, ground truth drawn by rule) tiled to 3 769 frames.  Timed: ONE pcr_kitti_eval_f64 call (class Car: 3 metrics x 3 difficulties;
host arrays in, curves out, synchronised by the call itself; warm; median of --reps), its kernels from the library's HIP-event profile (tune
prof = 2): the three overlap launches alone, the collecting pass, the thresholds and the matching pass.  For scale, the scalar f64 restatement
of evaluate_object.cpp (tests/golden/gen_golden_hw6.py) on the CPU: on the 200 fixture frames, times 3 769 / 200 (its cost is linear in the
frames; --restatement-full runs it on the tiled input instead).  There is no bar: the reference binary needs boost::geometry and was never
timed here, so the numbers are recorded, not gated.

    python tools/run_hw6_eval.py [--reps 10] [--warmup 2] [--frames 3769] [--out profiles/hw6_eval.txt] [--restatement-full]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INDEX_LINE = ("| `hw6_eval.txt` | Homework6's KITTI object evaluator (`csrc/kitti_eval.hip`), from `tools/run_hw6_eval.py` on a device: one `pcr_kitti_eval_f64` call on the "
              "fixture tiled to 3 769 frames — wall, the three overlap launches alone, the collecting pass, the thresholds and the matching pass — and the scalar "
              "f64 restatement on the CPU for scale; recorded, not gated |\n")


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t)


def restatement(ref, gts, dets, aos):
    a = time.perf_counter()
    out = [[ref.eval_class(0, gts, dets, aos and m == 0, d, m) for d in range(3)] for m in range(3)]
    return (time.perf_counter() - a) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hw6_eval.txt"))
    ap.add_argument("--restatement-full", action="store_true")
    args = ap.parse_args()
    pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
    spec = importlib.util.spec_from_file_location("gen_golden_hw6", os.path.join(ROOT, "tests", "golden", "gen_golden_hw6.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    z = np.load(os.path.join(ROOT, "tests", "golden", "hw6_eval_ref.npz"))
    gp, dp = z["gt_ptr"].astype(int), z["det_ptr"].astype(int)
    nf = len(gp) - 1
    gts = [z["gt_rows"][gp[f]:gp[f + 1]] for f in range(nf)]
    dets = [z["det_rows"][dp[f]:dp[f + 1]] for f in range(nf)]
    aos = bool(z["compute_aos"])
    pick = [f % nf for f in range(args.frames)]
    G, D = [gts[f] for f in pick], [dets[f] for f in pick]
    g = np.concatenate(G).reshape(-1, 15)
    d = np.concatenate(D).reshape(-1, 15)
    gptr = np.concatenate([[0], np.cumsum([len(x) for x in G])]).astype(np.uint64)
    dptr = np.concatenate([[0], np.cumsum([len(x) for x in D])]).astype(np.uint64)
    pairs = int(sum(len(a) * len(b) for a, b in zip(G, D)))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = pcr.Context(0)
    say("pcr_kitti_eval_f64 on one MI355X — tools/run_hw6_eval.py; recorded, not gated (nobody measured this stage before)")
    say(f"device: {ctx.device_info()}")
    say(f"input: the fixture's {nf} frames tiled to {args.frames}: {len(g)} ground-truth rows, {len(d)} detections (at most {max(len(x) for x in D)} in a frame), "
        f"{pairs} (gt, det) pairs per metric; class Car, AOS {'on' if aos else 'off'}")
    say(f"times in ms, median of {args.reps} after {args.warmup} warm-up calls (min in brackets)")
    run = lambda: ctx.kitti_eval(0, aos, g, gptr, d, dptr)
    got = run()
    wall, wall_min = median(run, args.reps, args.warmup)
    say(f"  one call, host arrays in, nine curves out (one host wait): {wall:.3f} ({wall_min:.3f})")
    ctx.tune("prof", 2)
    ctx.prof_reset()
    for _ in range(args.reps):
        run()
    ctx.tune("prof", 0)
    each = {n: np.array(ctx.prof_get_each(n), np.float64) for n in ("kitti_overlap", "kitti_collect", "kitti_thresholds", "kitti_match")}
    ov = each["kitti_overlap"].reshape(-1, 3)
    say(f"  kernels of that call (HIP events): the three overlap launches {np.median(ov.sum(axis=1)):.4f} "
        f"(IMAGE {np.median(ov[:, 0]):.4f}, GROUND {np.median(ov[:, 1]):.4f}, BOX3D {np.median(ov[:, 2]):.4f}: {pairs / (np.median(ov[:, 1]) * 1e-3) / 1e9:.2f} G pairs/s for GROUND)")
    say(f"    collecting pass {np.median(each['kitti_collect']):.4f}, thresholds (walk + rank, 9 pools) {np.median(each['kitti_thresholds']):.4f}, "
        f"matching pass ({args.frames * 9} waves, up to 41 thresholds each) {np.median(each['kitti_match']):.4f}")
    ksum = float(np.median(ov.sum(axis=1)) + sum(np.median(each[n]) for n in ("kitti_collect", "kitti_thresholds", "kitti_match")))
    say(f"    kernel sum {ksum:.4f}; the rest of the wall is the host: rows -> boxes with cos / sin, cleanData's codes, one upload, one download")
    mp, o = ctx.box_overlap(1, -1, g, gptr, d, dptr)
    t_ov, t_ov_min = median(lambda: ctx.box_overlap(1, -1, g, gptr, d, dptr), args.reps, args.warmup)
    say(f"  pcr_box_overlap_f64 alone (GROUND, union; sizing call + filling call, {o.size * 8 / 1e6:.2f} MB back): {t_ov:.3f} ({t_ov_min:.3f})")
    if args.restatement_full:
        t_ref, want = restatement(ref, G, D, aos)
        scale = ""
    else:
        t_fix, want = restatement(ref, gts, dets, aos)
        t_ref = t_fix * args.frames / nf
        scale = f" (= {t_fix:.0f} ms on the {nf} fixture frames x {args.frames}/{nf})"
        got = ctx.kitti_eval(0, aos, z["gt_rows"], z["gt_ptr"], z["det_rows"], z["det_ptr"])
    same = all(got[m][k]["tp"].tolist() == list(want[m][k]["tp"]) and got[m][k]["fp"].tolist() == list(want[m][k]["fp"])
               and np.array_equal(got[m][k]["precision"], np.array(want[m][k]["precision"]), equal_nan=True) for m in range(3) for k in range(3))
    say(f"  scalar f64 restatement on the CPU (Python, overlaps memoised per frame): {t_ref:.0f} ms{scale}; same counts and curves: {same}")
    say(f"    ratio restatement / library wall: {t_ref / wall:.0f} x")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")
    index = os.path.join(ROOT, "profiles", "INDEX.md")
    if os.path.exists(index) and "`hw6_eval.txt`" not in open(index).read():
        with open(index, "a") as fp:
            fp.write(INDEX_LINE)


if __name__ == "__main__":
    main()
